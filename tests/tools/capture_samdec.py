"""Golden capture for the SAM prompt encoder + mask decoder: writes tests/golden/samdec.npz, tests/golden/samdec_select.json and tests/golden/samdec.META.txt.
Runs on the CPU; needs `transformers`, whose SamPromptEncoder + SamMaskDecoder are segment_anything's PromptEncoder + MaskDecoder under other key names.

  weights   seeded synthetic, by the rule in lightdiffusion-next_amd/weights.py (sam_decoder_synth_tensor); the tests regenerate them and never import transformers.
  network   the reference is the transformers modules in fp64, built with layer_norm_eps = 1e-5 (segment_anything's nn.LayerNorm default; transformers' 1e-6 is
            not) and given the unit-scale [2][C / 2] positional matrix (transformers draws its own at scale hidden // 2); attention through
            torch's scaled_dot_product_attention (transformers' eager path takes the softmax in fp32 even in an fp64 module).
  samdec.npz  per case the fp64 low-res logits [P][4][4g][4g] and IoU predictions [P][4], the three multimask masks of torch's F.interpolate chain on them
            (Sam.postprocess_masks in fp64, > 0) bit-packed, and the figures the tests' bounds come from.  The full-size fp64 logits themselves are not stored
            (they would not fit a committed file): the tests rebuild them with the same chain from the stored low-res logits, and the packed masks pin the result.
  samdec_select.json  inputs and results of the reference's own sam_predict and make_sam_mask (src/AutoDetailer/SAM.py), run here on a stand-in
            segment_anything whose predictor returns canned scores and masks: recorded data, nothing of the reference's text.
  META      the figures, and the fixture conditions, which the tool asserts.  Lines under the "measured on the GPU" marker are kept when the tool runs again.
Run:
    python tests/tools/capture_samdec.py [path of the reference checkout, for samdec_select.json; without it that file is left as it is]
"""
import json
import os
import sys
import types

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
GOLDEN = os.path.join(ROOT, "tests", "golden")
SEED = 31337
MARK = "---- measured on the GPU ----"
HOST_LIMIT = 2e-5          # the fp32 host statement must stay within this (rel-L2) of the fp64 golden on every case


def networks():
    import ldx_amd as ldx
    C = ldx.weights.SAMDecoderConfig
    return {"A": C.tiny(), "B": C(image_size=320, hidden=256, num_heads=8, mlp_dim=2048, iou_head_hidden=256)}


# case -> (network, original (H, W), points [P][n][2] | None, labels | None, boxes [P][4] | None), coordinates in the resized frame
def cases():
    return {
        "A": ("A", (97, 128), [[[35.0, 50.0]], [[95.5, 48.0]]], [[1], [1]], [[10.0, 20.0, 60.0, 80.0], [64.0, 0.0, 127.0, 96.0]]),
        "B": ("B", (320, 200), [[[60.0, 100.0]], [[150.0, 250.5]], [[100.0, 160.0]]], [[1], [1], [1]],
              [[20.0, 40.0, 100.0, 160.0], [110.0, 200.0, 190.0, 301.0], [5.0, 10.0, 195.0, 310.0]]),
        "Ci": ("A", (128, 128), None, None, [[30.0, 40.0, 100.0, 90.0]]),
        "Cii": ("A", (128, 128), [[[40.0, 64.0], [100.0, 20.0]]], [[1, 0]], None),
    }


def fixture_weights(net):
    import ldx_amd as ldx
    return ldx.weights.sam_decoder_synth_state_dict(networks()[net], seed=SEED + ord(net))


def fixture_embedding(net):
    cfg = networks()[net]
    g = torch.Generator().manual_seed(SEED * 7 + ord(net))
    return torch.randn((cfg.hidden, cfg.grid, cfg.grid), generator=g)


def to_transformers_key(k):
    k = k.replace("prompt_encoder.pe_layer.positional_encoding_gaussian_matrix", "prompt_encoder.shared_embedding.positional_embedding")
    k = k.replace("prompt_encoder.point_embeddings.", "prompt_encoder.point_embed.")
    for i in range(1, 5):
        k = k.replace(f".norm{i}.", f".layer_norm{i}.")
    k = k.replace(".norm_final_attn.", ".layer_norm_final_attn.")
    k = k.replace("output_upscaling.0.", "upscale_conv1.").replace("output_upscaling.1.", "upscale_layer_norm.").replace("output_upscaling.3.", "upscale_conv2.")
    if "output_hypernetworks_mlps" in k or "iou_prediction_head" in k:
        k = k.replace(".layers.0.", ".proj_in.").replace(".layers.1.", ".layers.0.").replace(".layers.2.", ".proj_out.")
    return k


def reference_modules(cfg, sd):
    from transformers import SamConfig, SamMaskDecoderConfig, SamPromptEncoderConfig, SamVisionConfig
    from transformers.models.sam.modeling_sam import SamMaskDecoder, SamPromptEncoder
    pc = SamPromptEncoderConfig(hidden_size=cfg.hidden, image_size=cfg.image_size, patch_size=16, mask_input_channels=16, num_point_embeddings=4)
    mc = SamMaskDecoderConfig(hidden_size=cfg.hidden, mlp_dim=cfg.mlp_dim, num_hidden_layers=cfg.depth, num_attention_heads=cfg.num_heads,
                              attention_downsample_rate=2, num_multimask_outputs=cfg.num_multimask, iou_head_depth=3, iou_head_hidden_dim=cfg.iou_head_hidden,
                              layer_norm_eps=1e-5, hidden_act="relu")
    vc = SamVisionConfig(output_channels=cfg.hidden, image_size=cfg.image_size, patch_size=16, num_pos_feats=cfg.hidden // 2)
    conf = SamConfig(vision_config=vc, prompt_encoder_config=pc, mask_decoder_config=mc)
    # transformers' eager attention takes its softmax in fp32 whatever the module's type; torch's scaled_dot_product_attention keeps fp64
    conf.mask_decoder_config._attn_implementation = "sdpa"
    pe, md = SamPromptEncoder(conf).double().eval(), SamMaskDecoder(conf.mask_decoder_config).double().eval()
    mapped = {to_transformers_key(k): v.double() for k, v in sd.items()}
    r = pe.load_state_dict({k[len("prompt_encoder."):]: v for k, v in mapped.items() if k.startswith("prompt_encoder.")}, strict=False)
    assert not r.unexpected_keys and all(k.startswith("mask_embed.") for k in r.missing_keys), r          # the mask prompt's layers alone keep their own initialisation
    r = md.load_state_dict({k[len("mask_decoder."):]: v for k, v in mapped.items() if k.startswith("mask_decoder.")}, strict=True)
    assert not r.missing_keys and not r.unexpected_keys
    return pe, md


@torch.no_grad()
def reference_predict(cfg, sd, emb, points, labels, boxes):
    pe, md = reference_modules(cfg, sd)
    g = cfg.grid
    pts = None if points is None else torch.tensor(points, dtype=torch.float64)[None]
    lab = None if labels is None else torch.tensor(labels, dtype=torch.int64)[None]
    box = None if boxes is None else torch.tensor(boxes, dtype=torch.float64)[None]
    sparse, dense = pe(pts, lab, box, None)
    cell = (torch.arange(g, dtype=torch.float64) + 0.5) / g
    grid = torch.stack([cell[None, :].expand(g, g), cell[:, None].expand(g, g)], dim=-1)
    pos = pe.shared_embedding(grid).permute(2, 0, 1)[None]
    masks, iou = md(image_embeddings=emb.double()[None], image_positional_embeddings=pos, sparse_prompt_embeddings=sparse, dense_prompt_embeddings=dense,
                    multimask_output=False)
    masks1, iou1 = md(image_embeddings=emb.double()[None], image_positional_embeddings=pos, sparse_prompt_embeddings=sparse, dense_prompt_embeddings=dense,
                      multimask_output=True)
    return torch.cat([masks[0], masks1[0]], dim=1), torch.cat([iou[0], iou1[0]], dim=1), sparse[0]


def torch_postprocess(lowres, image_size, input_hw, out_hw):
    """Sam.postprocess_masks, torch's own F.interpolate chain in the dtype of `lowres`."""
    m = F.interpolate(lowres, (image_size, image_size), mode="bilinear", align_corners=False)
    m = m[..., :input_hw[0], :input_hw[1]]
    return F.interpolate(m, out_hw, mode="bilinear", align_corners=False)


def rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


# ---- the reference's own selection and wrapper, on a stand-in segment_anything -------------------------------------------------------------------------
SELECT_CASES = {
    "all_below": ([0.5, 0.7, 0.6], 0.93), "several": ([0.95, 0.5, 0.97], 0.93), "tie": ([0.8, 0.8, 0.3], 0.93), "none_positive": ([-0.1, 0.0, -0.5], 0.93),
    "one_at_top": ([0.2, 0.94, 0.1], 0.93),
}
WRAPPER_CASES = {
    # name: (H, W, bboxes, bbox_expansion, threshold, per-segment scores)
    "two_segments": (97, 128, [[10, 20, 60, 80], [100, 5, 128, 50]], 10, 0.93, [[0.5, 0.95, 0.97], [0.99, 0.2, 0.3]]),
    "first_below": (97, 128, [[10, 20, 60, 80], [100, 5, 128, 50]], 0, 0.93, [[0.5, 0.7, 0.6], [0.99, 0.2, 0.3]]),
    "clamped": (64, 80, [[2, 3, 78, 60]], 12, 0.5, [[0.1, 0.2, 0.9]]),
    "nothing": (64, 80, [[2, 3, 78, 60]], 12, 0.5, [[-0.1, 0.0, -0.9]]),
}


def canned_masks(name, seg, H, W):
    g = np.random.default_rng(SEED + sum(map(ord, name)) * 31 + seg)
    return g.random((3, H, W)) > 0.5


def capture_selection(ref_root):
    sys.path.insert(0, ref_root)
    calls = []

    class FakePredictor:
        script = None

        def __init__(self, model):
            self.model = model

        def set_image(self, image, fmt):
            calls.append({"image_shape": list(image.shape), "format": fmt})

        def predict(self, point_coords=None, point_labels=None, box=None):
            masks, scores = FakePredictor.script.pop(0)
            calls.append({"points": np.asarray(point_coords).tolist(), "labels": np.asarray(point_labels).tolist(), "box": np.asarray(box).tolist()})
            return masks, np.asarray(scores, dtype=np.float32), None

    standin = types.ModuleType("segment_anything")
    standin.SamPredictor, standin.sam_model_registry = FakePredictor, {}
    sys.modules["segment_anything"] = standin
    if "src.Device" not in sys.modules:
        try:
            import src.Device.Device  # noqa: F401
        except Exception:
            pkg, dev = types.ModuleType("src.Device"), types.ModuleType("src.Device.Device")
            pkg.Device = dev
            sys.modules["src.Device"], sys.modules["src.Device.Device"] = pkg, dev
    from src.AutoDetailer import SAM as R
    out = {"select": {}, "wrapper": {}}
    for name, (scores, thr) in SELECT_CASES.items():
        masks = [f"m{i}" for i in range(len(scores))]
        FakePredictor.script = [(masks, scores)]
        got = R.sam_predict(FakePredictor(None), [[1.0, 2.0]], [1], [0, 0, 4, 4], thr)
        out["select"][name] = {"scores": scores, "threshold": thr, "picked": [masks.index(m) for m in got]}
    for name, (H, W, bboxes, expansion, thr, scores) in WRAPPER_CASES.items():
        del calls[:]
        FakePredictor.script = [(canned_masks(name, i, H, W), s) for i, s in enumerate(scores)]
        segs = ((H, W), [types.SimpleNamespace(bbox=b) for b in bboxes])
        model = types.SimpleNamespace()
        model.sam_wrapper = R.SAMWrapper(model, is_auto_mode=False, safe_to_gpu=object())
        res = R.SAMDetectorCombined().doit(model, segs, torch.rand((1, H, W, 3)), True, 0, thr, expansion, 0.7, False)
        rec = {"H": H, "W": W, "bboxes": bboxes, "bbox_expansion": expansion, "threshold": thr, "scores": scores, "calls": list(calls)}
        if res is None:
            rec["result"] = None
        else:
            m = res[0]
            assert tuple(m.shape) == (1, H, W) and m.dtype == torch.float32
            rec["result"] = {"shape": list(m.shape), "packed": np.packbits(m.numpy().astype(np.uint8)).tolist()}
        out["wrapper"][name] = rec
    with open(os.path.join(GOLDEN, "samdec_select.json"), "w") as f:
        json.dump(out, f, separators=(",", ":"))
    return out


def main():
    import ldx_amd as ldx
    from ldx_amd import sam
    import transformers
    torch.manual_seed(0)
    g = {}
    meta = [f"samdec.npz: tests/tools/capture_samdec.py, seed {SEED}, torch {torch.__version__}, transformers {transformers.__version__}",
            "reference: transformers SamPromptEncoder + SamMaskDecoder in fp64 on the CPU (layer_norm_eps 1e-5, unit-scale positional matrix), synthetic weights",
            f"q_proj / k_proj gain {ldx.weights.SAM_DECODER_QK_GAIN}; the fp32 host statement must stay within {HOST_LIMIT:.0e} (rel-L2) of the golden",
            "bound of the engine per case = 10 x the rel-L2 of sam_decoder_host (fp32) from the golden low-res logits", ""]
    moved = {a: 0.0 for a in sam.DECODER_ABLATIONS}
    worst_bound = 0.0
    for case, (net, hw, points, labels, boxes) in cases().items():
        cfg, sd, emb = networks()[net], fixture_weights(net), fixture_embedding(net)
        ref, ref_iou, ref_sparse = reference_predict(cfg, sd, emb, points, labels, boxes)
        P = ref.shape[0]
        assert tuple(ref.shape) == (P, 4, 4 * cfg.grid, 4 * cfg.grid) and tuple(ref_iou.shape) == (P, 4)
        h64, i64 = sam.sam_decoder_host(sd, emb, points, labels, boxes, torch.float64, num_heads=cfg.num_heads)
        p64 = sam.sam_prompt_host(sd, points, labels, boxes, cfg.image_size, torch.float64)
        d64, dp64 = rel(h64, ref), rel(p64, ref_sparse)
        assert d64 <= 1e-9 and rel(i64, ref_iou) <= 1e-9 and dp64 <= 1e-12, (case, d64, dp64)
        h32, i32 = sam.sam_decoder_host(sd, emb, points, labels, boxes, torch.float32, num_heads=cfg.num_heads)
        d32, di32 = rel(h32, ref), rel(i32, ref_iou)
        assert d32 <= HOST_LIMIT, (case, d32)
        worst_bound = max(worst_bound, 10 * d32)
        # full size: the resized image is the original here (the longest side is image_size), so the crop is the original size
        assert sam.preprocess_shape(hw[0], hw[1], cfg.image_size) == hw
        full = torch_postprocess(ref[:, 1:], cfg.image_size, hw, hw)
        masks = (full > 0).numpy()
        _, host_full = sam.postprocess_host(h32[:, 1:].reshape(-1, 4 * cfg.grid, 4 * cfg.grid).numpy(), cfg.image_size, hw, hw)
        margin = 10 * float(np.abs(host_full.reshape(full.shape).astype(np.float64) - full.numpy()).max())
        _, pp = sam.postprocess_host(ref[:, 1:].float().reshape(-1, 4 * cfg.grid, 4 * cfg.grid).numpy(), cfg.image_size, hw, hw)
        tp = torch_postprocess(ref[:, 1:].float(), cfg.image_size, hw, hw).numpy()
        pp_diff = float(np.abs(pp.reshape(tp.shape) - tp).max())
        band = [float((np.abs(full[p, k].numpy()) < margin).mean()) for p in range(P) for k in range(3)]
        fg = [float(masks[p, k].mean()) for p in range(P) for k in range(3)]
        assert max(band) <= 0.02, (case, band)
        assert min(fg) >= 0.05 and max(fg) <= 0.95, (case, fg)
        g[f"{case}.lowres"], g[f"{case}.iou"] = ref.numpy(), ref_iou.numpy()
        g[f"{case}.masks"] = np.packbits(masks.astype(np.uint8))
        g[f"{case}.figures"] = np.array([d32, di32, margin, pp_diff, float((h32.double() - ref).abs().max())])
        meta += [f"case {case}: network {net} (image {cfg.image_size}, hidden {cfg.hidden}, heads {cfg.num_heads}, mlp {cfg.mlp_dim}), original {hw[0]} x {hw[1]}, P {P}, "
                 f"points {None if points is None else len(points[0])}, box {boxes is not None}; logit rms {float(ref.pow(2).mean().sqrt()):.4f}",
                 f"  host fp64 rel-L2 = {d64:.3e} (tokens {dp64:.3e})   host fp32 rel-L2 = {d32:.3e}, max-abs {float((h32.double() - ref).abs().max()):.3e}, IoU rel-L2 {di32:.3e}   (engine bound 10 x)",
                 f"  full size: margin = 10 x max-abs of the fp32 host chain from the golden = {margin:.3e}; share of |logit| < margin per mask: max {max(band):.4%}; "
                 f"foreground {min(fg):.1%} .. {max(fg):.1%}",
                 f"  postprocess_host vs torch's fp32 F.interpolate chain on the golden low-res logits: max-abs {pp_diff:.3e}"]
        for a in sam.DECODER_ABLATIONS:
            d = rel(sam.sam_decoder_host(sd, emb, points, labels, boxes, torch.float64, a, cfg.num_heads)[0], h64)
            moved[a] = max(moved[a], d)
            meta.append(f"  ablation {a}: moves the low-res logits by {d:.3e}")
        meta.append("")
    meta.append(f"fixture condition: every ablation must move some case by >= 5 x the largest engine bound = {5 * worst_bound:.3e}")
    for a, d in moved.items():
        meta.append(f"  {a}: largest move {d:.3e}  {'ok' if d >= 5 * worst_bound else 'TOO SMALL'}")
    assert all(d >= 5 * worst_bound for d in moved.values()), (moved, worst_bound)
    g["ablation_floor"] = np.array([5 * worst_bound])
    np.savez_compressed(os.path.join(GOLDEN, "samdec.npz"), **g)
    if len(sys.argv) > 1:
        sel = capture_selection(sys.argv[1])
        meta += ["", "samdec_select.json: the reference's sam_predict and make_sam_mask on canned scores and masks"]
        meta += [f"  select {k}: scores {v['scores']} threshold {v['threshold']} -> {v['picked']}" for k, v in sel["select"].items()]
        meta += [f"  wrapper {k}: {len(v['scores'])} segment(s), expansion {v['bbox_expansion']} -> {'None' if v['result'] is None else 'mask'}" for k, v in sel["wrapper"].items()]
    meta_path, measured = os.path.join(GOLDEN, "samdec.META.txt"), ""
    if os.path.exists(meta_path):
        old = open(meta_path).read()
        if MARK in old:
            measured = old[old.index(MARK):]
    with open(meta_path, "w") as f:
        f.write("\n".join(meta) + "\n\n" + (measured or MARK + "\n"))
    print("\n".join(meta))
    print("wrote", os.path.join(GOLDEN, "samdec.npz"), os.path.getsize(os.path.join(GOLDEN, "samdec.npz")), "bytes")


if __name__ == "__main__":
    main()
