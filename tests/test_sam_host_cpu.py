"""Host side of the SAM image encoder, no GPU: the torch statement of the network (ldx_amd.sam.sam_encoder_host) against the outputs of transformers'
SamVisionEncoder (tests/golden/sam.npz, written by tests/tools/capture_sam.py), Sam.preprocess and ResizeLongestSide's rules, the BILINEAR coefficients
against Pillow byte for byte, the key spec, the Sam.image_encoder shim with a counting stand-in engine, and the engine through the C ABI of the host-only
build (tests/tools/plan_trace.py): its plan's launches, its refusals, and ldx_sam_encode refused by another model's engine with nothing launched.

host fp32 against the golden, measured (tests/golden/sam.META.txt): 9.5e-7 / 1.0e-6 / 1.3e-6 on T / M / W; asserted: 10 x."""
import ctypes as C
import os
import shutil
import sys
import tempfile

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import capture_sam as CS  # noqa: E402
import plan_trace as T  # noqa: E402

LDX_OK, LDX_EINVAL, LDX_EMISSING, LDX_ESTATE = 0, -1, -2, -4
P = T.P
HOST_FP32_MEASURED = {"T": 9.544e-07, "M": 1.033e-06, "W": 1.304e-06}          # sam.META.txt


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "sam.npz"))


@pytest.mark.parametrize("case", ["T", "M", "W"])
def test_host_statement_matches_the_reference_encoder(ldx, golden, case):
    ref = torch.from_numpy(golden[f"{case}.out"])
    out = ldx.sam.sam_encoder_host(CS.fixture_weights(case), CS.fixture_input(case))
    d = CS.rel(out, ref)
    print(f"case {case}: sam_encoder_host rel-L2 to SamVisionEncoder = {d:.3e} (bound {10 * HOST_FP32_MEASURED[case]:.3e})")
    assert out.shape == ref.shape and d <= 10 * HOST_FP32_MEASURED[case]


@pytest.mark.parametrize("case", ["T", "M", "W"])
def test_key_spec_is_segment_anythings(ldx, golden, case):
    cfg, _ = CS.cases()[case]
    spec = ldx.weights.sam_encoder_state_dict_spec(cfg)
    keys = [k for k, _ in spec]
    assert keys == list(golden[f"{case}.keys"])
    assert sorted(CS.to_transformers_key(k) for k in keys) == list(golden[f"{case}.ref_keys"])          # the reference encoder's own state dict, renamed
    names = set()
    for k in keys:
        parts = k.split(".")
        names.add(".".join(p for p in parts if not p.isdigit()) if parts[0] == "blocks" else k)
    assert names == {"pos_embed", "patch_embed.proj.weight", "patch_embed.proj.bias", "blocks.norm1.weight", "blocks.norm1.bias", "blocks.norm2.weight",
                     "blocks.norm2.bias", "blocks.attn.qkv.weight", "blocks.attn.qkv.bias", "blocks.attn.proj.weight", "blocks.attn.proj.bias",
                     "blocks.attn.rel_pos_h", "blocks.attn.rel_pos_w", "blocks.mlp.lin1.weight", "blocks.mlp.lin1.bias", "blocks.mlp.lin2.weight",
                     "blocks.mlp.lin2.bias", "neck.0.weight", "neck.1.weight", "neck.1.bias", "neck.2.weight", "neck.3.weight", "neck.3.bias"}
    assert ldx.sam.config_of(CS.fixture_weights(case)) == cfg


def test_vit_b_config(ldx):
    cfg = ldx.SAMConfig.vit_b()
    assert (cfg.image_size, cfg.embed_dim, cfg.depth, cfg.num_heads, cfg.mlp_dim, cfg.out_chans, cfg.window_size) == (1024, 768, 12, 12, 3072, 256, 14)
    assert cfg.global_attn_mask == (1 << 2 | 1 << 5 | 1 << 8 | 1 << 11) and cfg.grid == 64
    spec = dict(ldx.weights.sam_encoder_state_dict_spec(cfg))
    assert spec["blocks.0.attn.rel_pos_h"] == (27, 64) and spec["blocks.2.attn.rel_pos_w"] == (127, 64)
    assert ldx.weights.param_count(list(spec.items())) == 89670912          # 89.67 M


def test_preprocess_shape(ldx):
    f = ldx.sam.preprocess_shape
    assert f(1024, 1024) == (1024, 1024) and f(512, 512) == (1024, 1024) and f(1024, 1536) == (683, 1024) and f(1536, 1024) == (1024, 683)
    assert f(48, 80, 128) == (77, 128) and f(37, 64, 64) == (37, 64) and f(3, 1000) == (3, 1024)


def test_preprocess_host_is_the_torch_expression(ldx):
    g = torch.Generator().manual_seed(3)
    img = torch.randint(0, 256, (37, 64, 3), generator=g, dtype=torch.uint8)
    mean, std = torch.tensor([123.675, 116.28, 103.53]).view(-1, 1, 1), torch.tensor([58.395, 57.12, 57.375]).view(-1, 1, 1)
    want = torch.zeros(3, 64, 64)
    want[:, :37, :64] = (img.permute(2, 0, 1).float() - mean) / std
    got = ldx.sam.preprocess_host(img.numpy(), 64)
    assert got.dtype == torch.float32 and torch.equal(got, want)


@pytest.mark.parametrize("w,h,ow,oh", [(512, 512, 1024, 1024), (1536, 1024, 1024, 683), (80, 48, 128, 77), (333, 517, 660, 1024), (1024, 37, 64, 2), (64, 37, 64, 80)])
def test_bilinear_coefficients_are_pillows(ldx, w, h, ow, oh):
    from PIL import Image
    rng = np.random.default_rng(w * 31 + h)
    img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    img[: h // 3, : w // 2] = rng.integers(0, 2, (h // 3, w // 2, 1), dtype=np.uint8) * 255          # hard edges: the rounding of every tap shows
    want = np.asarray(Image.fromarray(img).resize((ow, oh), Image.BILINEAR))
    got = ldx.detailer.resize_host(img, ow, oh, ldx.usdu.BILINEAR)
    assert got.shape == want.shape and np.array_equal(got, want), int(np.abs(got.astype(int) - want.astype(int)).max())


class _CountingEngine:
    """What LdxSAMPatch needs of a SAMImageEncoderEngine: cfg.image_size and encode()."""

    def __init__(self, ldx):
        self.cfg, self.calls = ldx.SAMConfig.tiny(), 0

    def encode(self, x):
        self.calls += 1
        return x.float().mean(dim=(1, 2, 3), keepdim=True).expand(x.shape[0], 64, 8, 8).double()          # another dtype than the input's, like the engine's fp32


class _Sam:
    def __init__(self):
        self.image_encoder = torch.nn.Identity()


def test_shim_reuses_the_features_of_an_equal_input(ldx):
    eng = _CountingEngine(ldx)
    patch = ldx.LdxSAMPatch(eng)
    assert isinstance(patch, torch.nn.Module) and not list(patch.parameters()) and patch.img_size == 128
    sam = patch.install(_Sam())
    assert sam.image_encoder is patch
    x = torch.randn(1, 3, 128, 128, dtype=torch.float16)
    outs = [sam.image_encoder(x), sam.image_encoder(x.clone()), sam.image_encoder(x)]
    y = x.clone()
    y[0, 0, 0, 0] += 1
    outs.append(sam.image_encoder(y))
    assert (patch.encodes, patch.reuses, eng.calls) == (2, 2, 2)
    assert all(o.dtype == torch.float16 and o.device == x.device and tuple(o.shape) == (1, 64, 8, 8) for o in outs)
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2]) and not torch.equal(outs[0], outs[3])


# ---- the engine through the host-only build ------------------------------------------------------------------------------------------------
def _last_error(H):
    return H.L.ldx_last_error().decode(errors="replace")


def _sam_engine(H, cfg, sd, dtype=0, finalize=True):
    c = H.ldx.lib.ldx_sam_config()
    c.compute_dtype = dtype
    for k in ("image_size", "embed_dim", "depth", "num_heads", "mlp_dim", "out_chans", "window_size", "global_attn_mask"):
        setattr(c, k, getattr(cfg, k))
    h = C.c_void_p()
    H.check(H.L.ldx_sam_create(C.byref(c), 0, C.byref(h)), "ldx_sam_create")
    H.load(h, sd)
    if finalize:
        H.check(H.L.ldx_finalize(h), "ldx_finalize")
    return h


@pytest.fixture(scope="module")
def host(ldx_lib):
    """(Host, SAM handle, TAESD handle) on a private copy of the host library (its stand-in runtime opens one trace file per loaded image)."""
    T.build_host()
    tmp = tempfile.mkdtemp(prefix="ldx_sam_host_")
    private = os.path.join(tmp, "libldx_host_sam.so")
    shutil.copy(T.HOST_LIB, private)
    orig, T.HOST_LIB = T.HOST_LIB, private
    try:
        H = T.Host()
    finally:
        T.HOST_LIB = orig
    cfg = H.ldx.SAMConfig.tiny()
    sam = _sam_engine(H, cfg, H.ldx.weights.sam_synth_state_dict(cfg))
    taesd, _ = T._engine(H, ("taesd", "tiny", "bf16", "build", 0, 0, 0, 0, 0))
    H.check(H.L.ldx_finalize(taesd), "ldx_finalize")
    H.take()
    yield H, sam, taesd
    for e in (sam, taesd):
        H.L.ldx_destroy(e)
    os.unlink(H.path)
    shutil.rmtree(tmp, ignore_errors=True)


def test_encode_refused_on_another_models_engine(host):
    H, _, taesd = host
    assert H.L.ldx_profile_report(None, None, 0) == LDX_EINVAL          # another call's text is in place
    H.take()
    rc = H.L.ldx_sam_encode(taesd, P["x"], 1, P["out"], None)
    err = _last_error(H)
    assert rc == LDX_ESTATE and "ldx_sam_encode" in err, (rc, err)
    assert H.take() == [], "ldx_sam_encode on a TAESD engine launched, copied or set memory"
    assert H.L.ldx_sam_encode(None, P["x"], 1, P["out"], None) == LDX_EINVAL and "ldx_sam_encode" in _last_error(H)
    assert H.take() == []


def test_sam_engine_refuses_another_models_entry_point_and_bad_arguments(host):
    H, sam, _ = host
    H.take()
    assert H.L.ldx_taesd_decode(sam, P["x"], 1, 5, 7, P["out"], None, 0, None) == LDX_ESTATE and "ldx_taesd_decode" in _last_error(H)
    assert H.L.ldx_sam_encode(sam, None, 1, P["out"], None) == LDX_EINVAL and "ldx_sam_encode" in _last_error(H)
    assert H.L.ldx_sam_encode(sam, P["x"], 0, P["out"], None) == LDX_EINVAL
    assert H.L.ldx_sam_preprocess(P["x"], 10, 4, 4, P["out"], 8, None) == LDX_EINVAL and "ldx_sam_preprocess" in _last_error(H)          # pitch < w * 3
    assert H.L.ldx_sam_preprocess(P["x"], 64, 9, 4, P["out"], 8, None) == LDX_EINVAL                                                   # h > size
    assert H.L.ldx_op_sam_window(P["x"], P["x"], None, 1, 8, 3, 128, 0, 0, None) == LDX_EINVAL and "ldx_op_sam_window" in _last_error(H)      # src == dst
    assert H.L.ldx_op_sam_window(P["x"], P["out"], None, 1, 8, 3, 100, 0, 0, None) == LDX_EINVAL                                            # C % 8
    assert H.L.ldx_op_sam_relpos(P["x"], 100, P["bias"], P["bias"], P["out"], 1, 2, 3, 0, None) == LDX_EINVAL and "ldx_op_sam_relpos" in _last_error(H)
    assert H.L.ldx_op_sam_attention(P["x"], P["x"], P["x"], 384, P["bias"], P["out"], 128, 40000, 2, 3, 0.125, 0, None) == LDX_EINVAL and "ldx_op_sam_attention" in _last_error(H)
    assert H.take() == []


def test_plan_launches(host):
    """Tiny config (2 blocks, the second global), B = 2: patch, patch_embed, pos; a window block = ln, gather, qkv, relpos, attention, proj, scatter, ln, lin1, gelu,
    lin2; a global block the same without gather and scatter; the neck = conv 1x1, ln, conv 3x3, ln, out."""
    H, sam, _ = host
    H.take()
    H.check(H.L.ldx_sam_encode(sam, P["x"], 2, P["out"], None), "ldx_sam_encode")
    launches = [r for r in H.take() if r.startswith("L ")]
    count = lambda name: sum(name in r for r in launches)          # noqa: E731
    assert (count("sam_patch_kernel"), count("sam_window_kernel"), count("sam_relpos_kernel"), count("sam_attn_kernel"), count("sam_rowvec_kernel"), count("sam_out_kernel")) == (1, 2, 2, 2, 3, 1)
    assert "sam_patch_kernel" in launches[0] and "sam_out_kernel" in launches[-1]
    attn = [r for r in launches if "sam_attn_kernel" in r]
    # window block: N = 9 -> 1 query block, 2 images x 9 windows x 2 heads; global block: N = 64 -> 1 query block, 2 x 2
    assert [r.split()[2:4] for r in attn] == [["1,36,1", "256,1,1"], ["1,4,1", "256,1,1"]], attn
    n, f, ar = C.c_int64(), C.c_double(), C.c_int64()
    H.check(H.L.ldx_plan_info(sam, C.byref(n), C.byref(f), C.byref(ar)), "ldx_plan_info")
    assert n.value >= 3 + 11 + 9 + 5 and f.value > 0 and ar.value > 0
    H.check(H.L.ldx_sam_encode(sam, P["x"], 2, P["out"], None), "ldx_sam_encode")
    assert [r.split()[1:5] for r in H.take() if r.startswith("L ")] == [r.split()[1:5] for r in launches]


def test_bad_configs_and_tables_are_refused(host):
    H, _, _ = host
    cfg = H.ldx.SAMConfig(image_size=128, embed_dim=160, depth=2, num_heads=2, mlp_dim=256, out_chans=64, window_size=3, global_attn_indexes=(1,))      # head dimension 80
    c = H.ldx.lib.ldx_sam_config()
    for k in ("image_size", "embed_dim", "depth", "num_heads", "mlp_dim", "out_chans", "window_size", "global_attn_mask"):
        setattr(c, k, getattr(cfg, k))
    h = C.c_void_p()
    assert H.L.ldx_sam_create(C.byref(c), 0, C.byref(h)) == LDX_EINVAL and "64" in _last_error(H) and not h.value
    tiny = H.ldx.SAMConfig.tiny()
    sd = H.ldx.weights.sam_synth_state_dict(tiny)
    bad = dict(sd)
    bad["blocks.0.attn.rel_pos_w"] = torch.zeros(7, 64)          # 2 n - 1 = 5 for window 3
    e = _sam_engine(H, tiny, bad, finalize=False)
    assert H.L.ldx_finalize(e) == LDX_EINVAL and "rel_pos_w" in _last_error(H)
    assert H.L.ldx_sam_encode(e, P["x"], 1, P["out"], None) == LDX_ESTATE
    H.L.ldx_destroy(e)
    miss = dict(sd)
    del miss["neck.2.weight"]
    e = _sam_engine(H, tiny, miss, finalize=False)
    assert H.L.ldx_finalize(e) == LDX_EMISSING and "neck.2.weight" in _last_error(H)
    H.L.ldx_destroy(e)
    H.take()
