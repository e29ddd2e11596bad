"""SAM prompt encoder + mask decoder on the GPU (csrc/samdec.hip, SamDecoderEngine): the prompt tokens against the fp64 statement, the engine against the fp64
outputs of transformers' SamPromptEncoder + SamMaskDecoder (tests/golden/samdec.npz, tests/tools/capture_samdec.py), the post-processing kernel against its numpy
statement float for float, masks against the golden's, batch independence, graph mode, SAMDetector, refused arguments and one full-size ViT-B call.

Bounds (tests/golden/samdec.META.txt has the figures measured on an MI355X):
  engine      rel-L2 of the low-res logits (and of the IoU predictions) to the golden <= 10 x that of sam_decoder_host in fp32, per case: the rule
              tests/test_sam_gpu.py uses for fp32 statements
  tokens      max-abs to the fp64 statement <= 10 ulp (fp32) of the largest angle 2 pi (cx g0 + cy g1): the angle is rounded a handful of times on its way
  masks       equal to the golden's wherever the golden's full-size |logit| >= margin (10 x the fp32 host chain's max-abs distance), a band of <= 2 % of a mask
  post        bytes and floats equal to postprocess_host"""
import math
import os
import sys
import types

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import capture_samdec as CD  # noqa: E402

pytestmark = pytest.mark.gpu
CASES = list(CD.cases())
_ENGINES = {}


def rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "samdec.npz"))


def _engine(ldx, net, graph=False):
    key = (net, graph)
    if key not in _ENGINES:
        eng = ldx.SAMMaskDecoderEngine(CD.networks()[net], CD.fixture_weights(net), graph=graph)
        eng.set_image(CD.fixture_embedding(net))
        _ENGINES[key] = eng
    return _ENGINES[key]


def _predict(ldx, case, graph=False):
    net, hw, points, labels, boxes = CD.cases()[case]
    return _engine(ldx, net, graph).predict(points, labels, boxes, None)


@pytest.mark.parametrize("case", CASES)
def test_prompt_tokens(ldx, ldx_lib, case):
    net, hw, points, labels, boxes = CD.cases()[case]
    cfg, sd = CD.networks()[net], CD.fixture_weights(net)
    got = _engine(ldx, net).prompt_tokens(points, labels, boxes, None).cpu()
    sparse = ldx.sam.sam_prompt_host(sd, points, labels, boxes, cfg.image_size, torch.float64)
    head = torch.cat([sd["mask_decoder.iou_token.weight"], sd["mask_decoder.mask_tokens.weight"]]).double()[None].expand(sparse.shape[0], -1, -1)
    want = torch.cat([head, sparse], dim=1)
    gm = sd["prompt_encoder.pe_layer.positional_encoding_gaussian_matrix"].double().abs()
    bound = 10 * 2.0 ** -23 * 2 * math.pi * float((gm[0] + gm[1]).max())          # |cx|, |cy| <= 1 inside the image
    diff = float((got.double() - want).abs().max())
    print(f"case {case}: tokens {tuple(got.shape)} max-abs {diff:.3e} (bound {bound:.3e})")
    assert got.shape == want.shape and torch.equal(got[:, :5].double(), want[:, :5])
    assert diff <= bound


@pytest.mark.parametrize("case", CASES)
def test_engine_matches_the_golden(ldx, ldx_lib, golden, case):
    lowres, iou = _predict(ldx, case)
    ref, ref_iou = torch.from_numpy(golden[f"{case}.lowres"])[:, 1:], torch.from_numpy(golden[f"{case}.iou"])[:, 1:]
    d, di = rel(lowres.cpu(), ref), rel(iou.cpu(), ref_iou)
    b, bi = 10 * float(golden[f"{case}.figures"][0]), 10 * float(golden[f"{case}.figures"][1])
    print(f"case {case}: low-res logits rel-L2 {d:.3e} (bound {b:.3e}), max-abs {float((lowres.cpu().double() - ref).abs().max()):.3e}; IoU rel-L2 {di:.3e} (bound {bi:.3e})")
    assert tuple(lowres.shape) == tuple(ref.shape) and bool(torch.isfinite(lowres).all())
    assert d <= b and di <= bi


@pytest.mark.parametrize("L,size,out_hw,n", [(32, 128, (97, 128), 3), (80, 320, (320, 200), 2), (256, 1024, (1024, 1024), 1), (256, 1024, (683, 1024), 1)])
def test_postprocess_kernel_equals_host_statement(ldx, ldx_lib, L, size, out_hw, n):
    g = torch.Generator().manual_seed(L + out_hw[0])
    low = torch.randn(n, L, L, generator=g)
    low[0, :2, :3] = 0.0          # exact zeros: not foreground
    eng = types.SimpleNamespace(cfg=types.SimpleNamespace(image_size=size), device=torch.device("cuda", 0), _lib=ldx_lib)
    mask, logits = ldx.SAMMaskDecoderEngine.masks(eng, low, out_hw, return_logits=True)
    want_mask, want = ldx.sam.postprocess_host(low.numpy(), size, ldx.sam.preprocess_shape(out_hw[0], out_hw[1], size), out_hw)
    got, got_mask = logits.cpu().numpy(), mask.cpu().numpy()
    print(f"{L}^2 -> {out_hw}: {int((got != want).sum())} floats and {int((got_mask != want_mask).sum())} bytes differ of {want.size}")
    assert got.dtype == np.float32 and got_mask.dtype == np.uint8 and got.shape == want.shape
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)) and np.array_equal(got_mask, want_mask)
    assert np.array_equal(ldx.SAMMaskDecoderEngine.masks(eng, low, out_hw).cpu().numpy(), want_mask)          # without the logits


@pytest.mark.parametrize("case", CASES)
def test_masks_match_the_golden_outside_the_band(ldx, ldx_lib, golden, case):
    net, hw, points, labels, boxes = CD.cases()[case]
    cfg = CD.networks()[net]
    lowres, _ = _predict(ldx, case)
    P = lowres.shape[0]
    got = _engine(ldx, net).masks(lowres, hw).cpu().numpy()
    want = np.unpackbits(golden[f"{case}.masks"])[:P * 3 * hw[0] * hw[1]].reshape(P, 3, hw[0], hw[1])
    full = CD.torch_postprocess(torch.from_numpy(golden[f"{case}.lowres"])[:, 1:], cfg.image_size, hw, hw).numpy()
    outside = np.abs(full) >= float(golden[f"{case}.figures"][2])
    band = 1.0 - outside.reshape(P * 3, -1).mean(axis=1)
    print(f"case {case}: band share max {band.max():.4%}; {int((got != want).sum())} of {want.size} pixels differ, {int((got != want)[outside].sum())} of them outside the band")
    assert got.shape == want.shape and band.max() <= 0.02
    assert np.array_equal(got[outside], want[outside])


@pytest.mark.parametrize("case", ["A", "B"])
def test_prompts_in_one_call_equal_single_calls(ldx, ldx_lib, case):
    net, hw, points, labels, boxes = CD.cases()[case]
    eng = _engine(ldx, net)
    lowres, iou = eng.predict(points, labels, boxes, None)
    lowres, iou = lowres.clone(), iou.clone()
    for p in range(len(boxes)):
        l1, i1 = eng.predict(points[p:p + 1], labels[p:p + 1], boxes[p:p + 1], None)
        assert torch.equal(l1[0], lowres[p]) and torch.equal(i1[0], iou[p]), (case, p)


def test_graph_replay_equals_eager(ldx, ldx_lib):
    eager = [t.clone() for t in _predict(ldx, "A")]
    eng = _engine(ldx, "A", graph=True)
    c0, r0 = eng.graph_stats()
    for i in range(4):
        lowres, iou = _predict(ldx, "A", graph=True)
        assert torch.equal(lowres, eager[0]) and torch.equal(iou, eager[1]), i
    c1, r1 = eng.graph_stats()
    print("captures", c1 - c0, "replays", r1 - r0)
    assert c1 - c0 == 1 and r1 - r0 == 2
    eng.set_image(2.0 * CD.fixture_embedding("A"))          # a new image: the graph reads the engine's own per-image buffers
    moved = _predict(ldx, "A", graph=True)[0]
    eng.set_image(CD.fixture_embedding("A"))
    assert not torch.equal(moved, eager[0]) and torch.equal(_predict(ldx, "A", graph=True)[0], eager[0]) and eng.graph_stats()[0] == c1


@pytest.mark.parametrize("combine", ["first", "or"])
def test_detector_equals_the_host_chain(ldx, ldx_lib, combine):
    ecfg, dcfg = ldx.SAMConfig.tiny(), CD.networks()["A"]
    key = ("detector",)
    if key not in _ENGINES:
        _ENGINES[key] = (ldx.SAMImageEncoderEngine(ecfg, ldx.weights.sam_synth_state_dict(ecfg, seed=5)), ldx.SAMMaskDecoderEngine(dcfg, CD.fixture_weights("A")))
    enc, dec = _ENGINES[key]
    det = ldx.SAMDetector(enc, dec)
    H, W = 97, 128
    image = torch.rand((1, H, W, 3), generator=torch.Generator().manual_seed(3))
    bboxes = [[10, 20, 60, 80], [100, 5, 128, 50], [30, 40, 90, 97]]
    segs = ((H, W), [types.SimpleNamespace(bbox=b) for b in bboxes])
    # the host chain on the engine's embedding: prompts, the decoder in fp32, selection, post-processing
    emb = enc.set_image(image.cuda())[0].cpu()
    pts, boxes = ldx.sam.detector_prompts_host(bboxes, (H, W), 8)
    pts_r = ldx.sam.apply_coords_host(pts, (H, W), dcfg.image_size).astype(np.float32)
    box_r = ldx.sam.apply_boxes_host(boxes, (H, W), dcfg.image_size).astype(np.float32)
    sd = CD.fixture_weights("A")
    h_low, h_iou = ldx.sam.sam_decoder_host(sd, emb, pts_r, [[1]] * 3, box_r, torch.float32, num_heads=dcfg.num_heads)
    scores = np.sort(h_iou[:, 1:].numpy().reshape(-1))
    gap = int(np.argmax(np.diff(scores)))
    threshold = float((scores[gap] + scores[gap + 1]) / 2)          # in the widest gap between two scores: the engine's fp32 error cannot move one across
    picked = ldx.sam.detector_selection_host(h_iou[:, 1:].numpy(), threshold, combine)
    assert picked
    L = h_low.shape[-1]
    h_mask, h_logits = ldx.sam.postprocess_host(np.stack([h_low[p, 1 + k].numpy() for p, k in picked]), dcfg.image_size, (H, W), (H, W))
    got = det.detect(image.cuda(), segs, threshold, 8, combine)
    assert got.dtype == torch.float32 and tuple(got.shape) == (1, H, W) and got.is_cuda
    # ... and bit for bit the host post-processing of the engine's own low-res logits for the same selection
    e_low, e_iou = dec.predict(pts, [[1]] * 3, boxes, (H, W))
    assert ldx.sam.detector_selection_host(e_iou.cpu().numpy(), threshold, combine) == picked
    e_mask, _ = ldx.sam.postprocess_host(np.stack([e_low[p, k].cpu().numpy() for p, k in picked]), dcfg.image_size, (H, W), (H, W))
    assert np.array_equal(got.cpu().numpy()[0], e_mask.max(axis=0).astype(np.float32))
    sure = (np.abs(h_logits) >= 1e-4).all(axis=0)          # 10 x the fp32 statements' distance at full size (META), rounded up
    diff = got.cpu().numpy()[0] != h_mask.max(axis=0)
    print(f"combine {combine}: threshold {threshold:.4f}, picked {picked}, foreground {float(got.mean()):.1%}, {int(diff.sum())} pixels differ from the host chain, {int(diff[sure].sum())} of them sure")
    assert sure.mean() >= 0.98 and not diff[sure].any()
    assert det.doit(None, segs, image.cuda(), True, 0, threshold, 8, 0.7, False, combine=combine)[0].equal(got)
    assert det.detect(image.cuda(), ((H, W), []), threshold, 8, combine) is None


def test_refused_configurations_launch_nothing(ldx, ldx_lib):
    C, lib = ldx.weights.SAMDecoderConfig, ldx.lib
    for bad in (C(image_size=128, hidden=96, num_heads=2, mlp_dim=128, iou_head_hidden=64), C(image_size=128, hidden=64, num_heads=3, mlp_dim=128, iou_head_hidden=64)):
        with pytest.raises(lib.LdxError, match="unsupported SAM decoder config"):
            ldx.SAMMaskDecoderEngine(bad, {})
    eng = _engine(ldx, "A")
    g = eng.cfg.grid
    lowres, iou = torch.full((65, 4, 4 * g, 4 * g), 7.0, device="cuda"), torch.full((65, 4), 7.0, device="cuda")
    pts, lab, box = torch.zeros((65, 9, 2), device="cuda"), torch.ones((65, 9), device="cuda", dtype=torch.int32), torch.zeros((65, 4), device="cuda")
    st = lib.current_stream_ptr()
    for n, P, p, l, b in ((9, 1, pts, lab, box), (0, 1, None, None, None), (1, 65, pts, lab, box), (1, 0, pts, lab, box), (1, 1, pts, None, box)):
        rc = ldx_lib.ldx_samdec_predict(eng._h, lib.ptr(p), lib.ptr(l), n, lib.ptr(b), P, lib.ptr(lowres), lib.ptr(iou), st)
        assert rc == -1 and b"ldx_samdec_predict" in ldx_lib.ldx_last_error(), (n, P, rc)
    torch.cuda.synchronize()
    assert bool((lowres == 7.0).all()) and bool((iou == 7.0).all())
    with pytest.raises(ValueError):
        eng.predict(None, None, None, None)
    fresh = ldx.SAMMaskDecoderEngine(CD.networks()["A"], CD.fixture_weights("A"))
    with pytest.raises(lib.LdxError, match="no image set"):
        fresh.predict(None, None, [[1.0, 2.0, 30.0, 40.0]], None)


def test_full_size_vit_b(ldx, ldx_lib):
    cfg = ldx.weights.SAMDecoderConfig.vit_b()
    eng = ldx.SAMMaskDecoderEngine(cfg, ldx.weights.sam_decoder_synth_state_dict(cfg, seed=9))
    eng.set_image(torch.randn((256, 64, 64), generator=torch.Generator().manual_seed(1)))
    boxes = [[100.0, 120.0, 500.0, 640.0], [0.0, 0.0, 1023.0, 1023.0], [600.0, 300.0, 900.0, 700.0], [10.0, 800.0, 400.0, 1000.0]]
    points = [[[(b[0] + b[2]) / 2, (b[1] + b[3]) / 2]] for b in boxes]
    lowres, iou = eng.predict(points, [[1]] * 4, boxes, None)
    masks = eng.masks(lowres, (1024, 1024))
    info = eng.plan_info()
    print(f"ViT-B sizes, P = 4: {info['launches']} launches; logit rms {float(lowres.pow(2).mean().sqrt()):.3f}; foreground {float(masks.float().mean()):.1%}")
    assert tuple(lowres.shape) == (4, 3, 256, 256) and tuple(iou.shape) == (4, 3) and tuple(masks.shape) == (4, 3, 1024, 1024)
    assert bool(torch.isfinite(lowres).all()) and bool(torch.isfinite(iou).all()) and 0 < info["launches"] <= 64
