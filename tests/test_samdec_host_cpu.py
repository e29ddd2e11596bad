"""SAM prompt encoder + mask decoder, host side (no GPU): the torch statement sam_decoder_host against the fp64 outputs of transformers' SamPromptEncoder +
SamMaskDecoder (tests/golden/samdec.npz, written by tests/tools/capture_samdec.py with the figures in tests/golden/samdec.META.txt), the fixture's
conditions, postprocess_host against torch's own F.interpolate chain, the selection rule and SAMDetector's host logic against results recorded from the
reference's sam_predict / make_sam_mask (tests/golden/samdec_select.json), and ResizeLongestSide's coordinate transforms."""
import json
import os
import sys
import types

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import capture_samdec as CD  # noqa: E402

CASES = list(CD.cases())


def rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "samdec.npz"))


@pytest.fixture(scope="module")
def select(golden_dir):
    return json.load(open(os.path.join(golden_dir, "samdec_select.json")))


def _case(case):
    net, hw, points, labels, boxes = CD.cases()[case]
    return CD.networks()[net], CD.fixture_weights(net), CD.fixture_embedding(net), hw, points, labels, boxes


def test_state_dict_spec_is_what_the_fixture_maps(ldx):
    cfg = ldx.weights.SAMDecoderConfig.vit_b()
    spec = ldx.weights.sam_decoder_state_dict_spec(cfg)
    keys = [k for k, _ in spec]
    assert len(set(keys)) == len(keys) and all(k.startswith(("prompt_encoder.", "mask_decoder.")) for k in keys)
    assert sum(int(np.prod(s)) for _, s in spec) == 4058340 + (6220 - 4684) + 256          # the published counts: mask decoder + prompt encoder without the mask prompt's 4 684, + the gaussian matrix (a buffer)
    sd = ldx.weights.sam_decoder_synth_state_dict(ldx.weights.SAMDecoderConfig.tiny())
    assert all(bool((v != 0).all()) for k, v in sd.items() if k.endswith(".bias") or "embed" in k or "token" in k), "every embedding and bias is non-zero"


@pytest.mark.parametrize("case", CASES)
def test_host_statement_matches_the_golden(ldx, golden, case):
    cfg, sd, emb, hw, points, labels, boxes = _case(case)
    ref, ref_iou = torch.from_numpy(golden[f"{case}.lowres"]), torch.from_numpy(golden[f"{case}.iou"])
    d32_rec = float(golden[f"{case}.figures"][0])
    h64, i64 = ldx.sam.sam_decoder_host(sd, emb, points, labels, boxes, torch.float64, num_heads=cfg.num_heads)
    h32, i32 = ldx.sam.sam_decoder_host(sd, emb, points, labels, boxes, torch.float32, num_heads=cfg.num_heads)
    d64, d32 = rel(h64, ref), rel(h32, ref)
    print(f"case {case}: fp64 rel-L2 {d64:.3e} (IoU {rel(i64, ref_iou):.3e}), fp32 rel-L2 {d32:.3e} (recorded {d32_rec:.3e}), IoU {rel(i32, ref_iou):.3e}")
    assert d64 <= 1e-9 and rel(i64, ref_iou) <= 1e-9
    assert d32 <= 10 * d32_rec and d32_rec <= CD.HOST_LIMIT and rel(i32, ref_iou) <= 10 * float(golden[f"{case}.figures"][1])


def test_every_ablation_moves_some_case(ldx, golden):
    floor = float(golden["ablation_floor"][0])
    moved = {a: 0.0 for a in ldx.sam.DECODER_ABLATIONS}
    for case in CASES:
        cfg, sd, emb, hw, points, labels, boxes = _case(case)
        base = ldx.sam.sam_decoder_host(sd, emb, points, labels, boxes, torch.float64, num_heads=cfg.num_heads)[0]
        for a in moved:
            moved[a] = max(moved[a], rel(ldx.sam.sam_decoder_host(sd, emb, points, labels, boxes, torch.float64, a, cfg.num_heads)[0], base))
    print(moved, "floor", floor)
    assert len(moved) == 5 and all(d >= floor for d in moved.values()), (moved, floor)


@pytest.mark.parametrize("case", CASES)
def test_postprocess_host_against_torch_chain(ldx, golden, case):
    cfg, sd, emb, hw, points, labels, boxes = _case(case)
    ref = torch.from_numpy(golden[f"{case}.lowres"])[:, 1:]
    P, L = ref.shape[0], ref.shape[-1]
    margin, pp_rec = float(golden[f"{case}.figures"][2]), float(golden[f"{case}.figures"][3])
    full = CD.torch_postprocess(ref, cfg.image_size, hw, hw).numpy()                      # fp64: the golden's full-size logits
    want = np.unpackbits(golden[f"{case}.masks"])[:P * 3 * hw[0] * hw[1]].reshape(P, 3, hw[0], hw[1])
    assert np.array_equal((full > 0).astype(np.uint8), want)
    mask, logits = ldx.sam.postprocess_host(ref.float().reshape(-1, L, L).numpy(), cfg.image_size, hw, hw)
    assert mask.dtype == np.uint8 and logits.dtype == np.float32 and mask.shape == (P * 3, hw[0], hw[1])
    t32 = CD.torch_postprocess(ref.float(), cfg.image_size, hw, hw).numpy().reshape(logits.shape)
    diff = float(np.abs(logits - t32).max())
    outside = np.abs(full.reshape(logits.shape)) >= margin
    band = 1.0 - outside.reshape(P * 3, -1).mean(axis=1)
    fg = want.reshape(P * 3, -1).mean(axis=1)
    print(f"case {case}: max-abs to torch's fp32 chain {diff:.3e} (recorded {pp_rec:.3e}); band share max {band.max():.4%}; foreground {fg.min():.1%} .. {fg.max():.1%}")
    assert diff <= pp_rec
    assert band.max() <= 0.02 and fg.min() >= 0.05 and fg.max() <= 0.95
    assert np.array_equal(mask[outside], want.reshape(mask.shape)[outside])


@pytest.mark.parametrize("L,size,in_hw,out_hw", [(32, 128, (97, 128), (97, 128)), (32, 128, (86, 128), (683, 1024)), (16, 64, (64, 43), (200, 133))])
def test_postprocess_host_scales(ldx, L, size, in_hw, out_hw):
    """... and where both resamplings change the size, against torch's chain in fp64: the fp32 rounding of a few products of values of magnitude ~3."""
    g = torch.Generator().manual_seed(L + out_hw[0])
    low = torch.randn(2, L, L, generator=g)
    mask, logits = ldx.sam.postprocess_host(low.numpy(), size, in_hw, out_hw)
    want = CD.torch_postprocess(low.double()[None], size, in_hw, out_hw)[0].numpy()
    assert float(np.abs(logits - want).max()) <= 5e-6
    sure = np.abs(want) >= 5e-5
    assert np.array_equal(mask[sure], (want > 0).astype(np.uint8)[sure])


def test_select_masks_matches_the_reference(ldx, select):
    assert set(select["select"]) == set(CD.SELECT_CASES)
    for name, rec in select["select"].items():
        got = ldx.sam.select_masks_host(np.asarray(rec["scores"], dtype=np.float32), rec["threshold"])
        assert got == rec["picked"], (name, got, rec["picked"])
    assert select["select"]["none_positive"]["picked"] == [] and select["select"]["tie"]["picked"] == [0] and len(select["select"]["several"]["picked"]) == 2


@pytest.mark.parametrize("name", list(CD.WRAPPER_CASES))
def test_detector_host_logic_matches_the_reference(ldx, select, name):
    """make_sam_mask's prompts and its result, from the recorded calls of the reference on canned scores and masks."""
    rec = select["wrapper"][name]
    H, W = rec["H"], rec["W"]
    points, boxes = ldx.sam.detector_prompts_host(rec["bboxes"], (H, W), rec["bbox_expansion"])
    calls = [c for c in rec["calls"] if "box" in c]
    assert len(calls) == len(rec["bboxes"])
    for i, c in enumerate(calls):
        assert np.array_equal(np.asarray(c["points"], dtype=np.float64), points[i]) and c["labels"] == [1]
        assert np.array_equal(np.asarray(c["box"], dtype=np.float64).reshape(4), boxes[i])
    picked = ldx.sam.detector_selection_host(np.asarray(rec["scores"], dtype=np.float32), rec["threshold"], "first")
    if rec["result"] is None:
        assert picked == [] and ldx.sam.detector_selection_host(np.asarray(rec["scores"], dtype=np.float32), rec["threshold"], "or") == []
        return
    want = np.unpackbits(np.asarray(rec["result"]["packed"], dtype=np.uint8))[:H * W].reshape(H, W)
    assert len(picked) == 1
    p, k = picked[0]
    assert np.array_equal(CD.canned_masks(name, p, H, W)[k].astype(np.uint8), want)
    every = ldx.sam.detector_selection_host(np.asarray(rec["scores"], dtype=np.float32), rec["threshold"], "or")
    assert every[0] == picked[0] and len(every) == sum(len(ldx.sam.select_masks_host(np.asarray(s, dtype=np.float32), rec["threshold"])) for s in rec["scores"])


def test_detector_without_segments_is_none(ldx):
    det = object.__new__(ldx.SAMDetector)
    assert det.detect(torch.zeros(1, 8, 8, 3), ((8, 8), []), 0.93, 0) is None
    assert det.doit(segs=((8, 8), []), image=torch.zeros(1, 8, 8, 3)) is None


def test_coordinate_transforms(ldx):
    S = ldx.sam
    assert S.preprocess_shape(600, 1200, 1024) == (512, 1024)
    c = S.apply_coords_host([[100.0, 50.0], [1199.0, 599.0]], (600, 1200), 1024)
    assert c.dtype == np.float64 and np.array_equal(c, np.array([[100.0 * (1024 / 1200), 50.0 * (512 / 600)], [1199.0 * (1024 / 1200), 599.0 * (512 / 600)]]))
    b = S.apply_boxes_host([[10, 20, 30, 40], [0, 0, 1200, 600]], (600, 1200), 1024)
    assert b.shape == (2, 4) and np.array_equal(b[1], np.array([0.0, 0.0, 1024.0, 512.0])) and np.array_equal(b[0, 2:], np.array([30 * (1024 / 1200), 40 * (512 / 600)]))
    # a portrait image whose rounded short side is not the plain product (ResizeLongestSide rounds new_w: 683, not 682.67)
    assert S.preprocess_shape(1536, 1024, 1024) == (1024, 683)
    assert np.array_equal(S.apply_coords_host([[1024.0, 1536.0]], (1536, 1024), 1024), np.array([[1024.0 * (683 / 1024), 1536.0 * (1024 / 1536)]]))
    src = np.array([[1.0, 2.0]])
    S.apply_coords_host(src, (10, 10), 1024)
    assert np.array_equal(src, np.array([[1.0, 2.0]])), "the input is not changed in place"
