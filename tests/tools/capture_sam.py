"""Golden capture for the SAM image encoder: writes tests/golden/sam.npz and tests/golden/sam.META.txt.  Runs on the CPU; needs `transformers`, whose
SamVisionEncoder is the same network as segment_anything's ImageEncoderViT under other key names.  Nothing of the reference is imported.

  weights   seeded synthetic, by the rule in lightdiffusion-next_amd/weights.py (sam_synth_tensor): the tests regenerate them and never import transformers.
            transformers initialises the rel_pos tables to zero, so its own initialisation could not tell a kernel without them from a correct one.
  inputs    fixture_input(case): gaussian, scaled like a normalised image, the bottom quarter zero as after Sam.preprocess of a wide image; regenerated too.
  sam.npz   per case the fp32 output of SamVisionEncoder (`<case>.out`), and the key list with shapes of its state dict mapped to segment_anything's names.
  META      per case: the distance of sam_encoder_host (fp32) from the golden, the distances of sam_encoder_host16 in bf16 / f16 (the engine's bound is
            2 x those), and how far each of four deliberately wrong networks lands from the right one.  The tool fails unless every one of the four moves
            some case's output by at least 5 x the bf16 bound.  Lines under the "measured on the GPU" marker are kept when the tool runs again.
Run:
    python tests/tools/capture_sam.py
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
GOLDEN = os.path.join(ROOT, "tests", "golden")
SEED = 20260
MARK = "---- measured on the GPU ----"


def cases():
    import ldx_amd as ldx
    C = ldx.SAMConfig
    return {
        "T": (C(image_size=128, embed_dim=128, depth=2, num_heads=2, mlp_dim=256, out_chans=64, window_size=3, global_attn_indexes=(1,)), 2),
        "M": (C(image_size=320, embed_dim=128, depth=3, num_heads=2, mlp_dim=256, out_chans=64, window_size=14, global_attn_indexes=(1,)), 1),
        "W": (C(image_size=320, embed_dim=768, depth=2, num_heads=12, mlp_dim=3072, out_chans=256, window_size=14, global_attn_indexes=(1,)), 1),
    }


def fixture_weights(case):
    import ldx_amd as ldx
    return ldx.weights.sam_synth_state_dict(cases()[case][0], seed=SEED + ord(case))


def fixture_input(case):
    cfg, B = cases()[case]
    g = torch.Generator().manual_seed(SEED * 7 + ord(case))
    x = torch.randn((B, 3, cfg.image_size, cfg.image_size), generator=g)
    x[:, :, cfg.image_size * 3 // 4:] = 0.0
    return x


def to_transformers_key(k):
    k = k.replace("patch_embed.proj.", "patch_embed.projection.").replace("blocks.", "layers.").replace(".norm1.", ".layer_norm1.").replace(".norm2.", ".layer_norm2.")
    return k.replace("neck.0.", "neck.conv1.").replace("neck.1.", "neck.layer_norm1.").replace("neck.2.", "neck.conv2.").replace("neck.3.", "neck.layer_norm2.")


def reference_encoder(cfg, sd):
    from transformers import SamVisionConfig
    from transformers.models.sam.modeling_sam import SamVisionEncoder
    c = SamVisionConfig(hidden_size=cfg.embed_dim, output_channels=cfg.out_chans, num_hidden_layers=cfg.depth, num_attention_heads=cfg.num_heads,
                        image_size=cfg.image_size, patch_size=16, window_size=cfg.window_size, global_attn_indexes=list(cfg.global_attn_indexes),
                        mlp_dim=cfg.mlp_dim, layer_norm_eps=1e-6, hidden_act="gelu", qkv_bias=True, use_abs_pos=True, use_rel_pos=True)
    m = SamVisionEncoder(c).eval()
    missing, unexpected = m.load_state_dict({to_transformers_key(k): v for k, v in sd.items()}, strict=True)
    assert not missing and not unexpected
    return m


def rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def main():
    import ldx_amd as ldx
    from ldx_amd import sam
    import transformers
    torch.manual_seed(0)
    g, meta = {}, [f"sam.npz: tests/tools/capture_sam.py, seed {SEED}, torch {torch.__version__}, transformers {transformers.__version__}",
                   "reference: transformers.models.sam.modeling_sam.SamVisionEncoder in fp32 on the CPU, synthetic weights (weights.sam_synth_tensor)",
                   "bound of the engine per case and type = 2 x the rel-L2 of sam_encoder_host16 from the golden (host16 lines below)", ""]
    moved = {a: 0.0 for a in sam.ABLATIONS}
    worst_bound = 0.0
    for case, (cfg, B) in cases().items():
        sd, x = fixture_weights(case), fixture_input(case)
        model = reference_encoder(cfg, sd)
        with torch.no_grad():
            ref = model(x).last_hidden_state.float()
        assert tuple(ref.shape) == (B, cfg.out_chans, cfg.grid, cfg.grid)
        g[f"{case}.out"] = ref.numpy()
        g[f"{case}.keys"] = np.array([k for k, _ in ldx.weights.sam_encoder_state_dict_spec(cfg)])
        ref_sd = model.state_dict()
        g[f"{case}.ref_keys"] = np.array(sorted(ref_sd))
        host = sam.sam_encoder_host(sd, x)
        d32, dbf, df16 = rel(host, ref), rel(sam.sam_encoder_host16(sd, x, torch.bfloat16), ref), rel(sam.sam_encoder_host16(sd, x, torch.float16), ref)
        rms = float(ref.pow(2).mean().sqrt())
        meta += [f"case {case}: image {cfg.image_size}, E {cfg.embed_dim}, heads {cfg.num_heads}, mlp {cfg.mlp_dim}, C {cfg.out_chans}, window {cfg.window_size}, "
                 f"depth {cfg.depth}, global {list(cfg.global_attn_indexes)}, B {B}; output rms {rms:.4f}",
                 f"  host fp32 rel-L2 = {d32:.3e}   (tests assert 10 x)",
                 f"  host16 bf16 rel-L2 = {dbf:.3e}   host16 f16 rel-L2 = {df16:.3e}   (the engine's bound is 2 x)"]
        worst_bound = max(worst_bound, 2 * dbf)
        for a in sam.ABLATIONS:
            d = rel(sam.sam_encoder_host(sd, x, a), host)
            moved[a] = max(moved[a], d)
            meta.append(f"  ablation {a}: moves the output by {d:.3e}")
        meta.append("")
    meta.append(f"fixture condition: every ablation must move some case by >= 5 x the largest bf16 bound = {5 * worst_bound:.3e}")
    for a, d in moved.items():
        meta.append(f"  {a}: largest move {d:.3e}  {'ok' if d >= 5 * worst_bound else 'TOO SMALL'}")
    assert all(d >= 5 * worst_bound for d in moved.values()), (moved, worst_bound)
    np.savez_compressed(os.path.join(GOLDEN, "sam.npz"), **g)
    meta_path, measured = os.path.join(GOLDEN, "sam.META.txt"), ""
    if os.path.exists(meta_path):
        old = open(meta_path).read()
        if MARK in old:
            measured = old[old.index(MARK):]
    with open(meta_path, "w") as f:
        f.write("\n".join(meta) + "\n\n" + (measured or MARK + "\n"))
    print("\n".join(meta))
    print("wrote", os.path.join(GOLDEN, "sam.npz"), os.path.getsize(os.path.join(GOLDEN, "sam.npz")), "bytes")


if __name__ == "__main__":
    main()
