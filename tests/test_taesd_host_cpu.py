"""The TAESD engine through the C ABI of the host-only build (tests/tools/plan_trace.py: a stand-in HIP runtime records every launch, asynchronous copy and
memset), as tests/test_engine_kinds_cpu.py does for the six other models: a TAESD engine is created, finalized and run, and its launches are recorded;
ldx_taesd_decode is refused by every other model's engine, and the other models' entry points by the TAESD engine, with LDX_ESTATE, the entry point's name in
ldx_last_error and nothing recorded; a null handle is LDX_EINVAL; what every model answers alike, TAESD answers too.  No GPU."""
import ctypes as C
import os
import shutil
import sys
import tempfile

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import plan_trace as T  # noqa: E402

LDX_OK, LDX_EINVAL, LDX_ESTATE = 0, -1, -4
OTHERS = ("unet", "vae", "clip", "t5", "esrgan", "flux")
P = T.P
F32 = 2


def _decode_args(B=1, h=5, w=7, flux=0):
    return (P["x"], B, h, w, P["out"], P["out2"], flux, None)


@pytest.fixture(scope="module")
def host(ldx_lib):
    """(Host, TAESD handle, {model: handle}).  The stand-in runtime opens its trace file once per loaded image of the library, so this module loads a private
    copy: another test module's recorder in the same process keeps its own file."""
    T.build_host()
    tmp = tempfile.mkdtemp(prefix="ldx_taesd_host_")
    private = os.path.join(tmp, "libldx_host_taesd.so")
    shutil.copy(T.HOST_LIB, private)
    orig, T.HOST_LIB = T.HOST_LIB, private
    try:
        H = T.Host()
    finally:
        T.HOST_LIB = orig
    h, _ = T._engine(H, ("taesd", "tiny", "bf16", "build", 0, 0, 0, 0, 0))
    H.check(H.L.ldx_finalize(h), "ldx_finalize")
    others = {}
    for model in OTHERS:
        e, _ = T._engine(H, (model, "tiny", "bf16", "build", 0, 0, 0, 0, 0))
        H.check(H.L.ldx_finalize(e), "ldx_finalize")
        others[model] = e
    H.take()
    yield H, h, others
    for e in list(others.values()) + [h]:
        H.L.ldx_destroy(e)
    os.unlink(H.path)
    shutil.rmtree(tmp, ignore_errors=True)


def _last_error(H):
    return H.L.ldx_last_error().decode(errors="replace")


def test_bad_config_is_refused(host):
    H, _, _ = host
    c = H.ldx.lib.ldx_taesd_config()
    c.compute_dtype, c.latent_channels = 0, 16
    h = C.c_void_p()
    assert H.L.ldx_taesd_create(C.byref(c), 0, C.byref(h)) == LDX_EINVAL and "latent_channels" in _last_error(H) and not h.value


def test_decode_plans_and_launches(host):
    """prep + conv_in + 10 Blocks of 3 + 3 upconvs + conv_out = 36 launches, all of the TAESD kernels; the plan's figures answer as for the other models."""
    H, h, _ = host
    H.take()
    H.check(H.L.ldx_taesd_decode(h, *_decode_args(B=2)), "ldx_taesd_decode")
    launches = [r for r in H.take() if r.startswith("L ")]
    assert len(launches) == 36, launches
    assert sum("taesd_prep_kernel" in r for r in launches) == 1 and sum("taesd_conv_kernel" in r for r in launches) == 35
    assert "taesd_prep_kernel" in launches[0] and "Li1ELb1E" in launches[-1]          # the 64 -> 3 instantiation comes last
    for r in launches[1:]:
        grid, block, lds = r.split()[2], r.split()[3], int(r.split()[4])
        assert block == "256,1,1" and lds == (123712 if r is not launches[-1] else (32 * 584 + 340 * 72) * 2), r
        assert 1 <= int(grid.split(",")[0]) <= 256, r
    n, f, ar = C.c_int64(), C.c_double(), C.c_int64()
    H.check(H.L.ldx_plan_info(h, C.byref(n), C.byref(f), C.byref(ar)), "ldx_plan_info")
    pix = [2 * 5 * 7 * 4 ** k for k in range(4)]
    want = 2.0 * 576 * 64 * (pix[0] * 10 + pix[1] * 10 + pix[2] * 10 + pix[3] * 4) + 2.0 * 576 * 3 * pix[3]
    assert n.value == 36 and f.value == want and ar.value >= pix[3] * 64 * 2 * 3
    # the same shape again launches the same plan; a second shape plans anew
    H.check(H.L.ldx_taesd_decode(h, *_decode_args(B=2)), "ldx_taesd_decode")
    assert [r.split()[1:5] for r in H.take() if r.startswith("L ")] == [r.split()[1:5] for r in launches]
    H.check(H.L.ldx_taesd_decode(h, *_decode_args(B=1, h=33, w=17, flux=1)), "ldx_taesd_decode")
    assert len([r for r in H.take() if r.startswith("L ")]) == 36


def test_bad_arguments(host):
    H, h, _ = host
    H.take()
    assert H.L.ldx_taesd_decode(h, None, 1, 5, 7, P["out"], None, 0, None) == LDX_EINVAL and "ldx_taesd_decode" in _last_error(H)
    assert H.L.ldx_taesd_decode(h, P["x"], 1, 5, 7, None, None, 0, None) == LDX_EINVAL and "ldx_taesd_decode" in _last_error(H)
    assert H.L.ldx_taesd_decode(h, P["x"], 0, 5, 7, P["out"], None, 0, None) == LDX_EINVAL
    assert H.L.ldx_taesd_decode(h, P["x"], 1, 8192, 8192, P["out"], None, 0, None) == LDX_EINVAL
    assert H.L.ldx_taesd_conv64(None, P["x"], None, None, None, P["out"], None, 1, 5, 7, 0, 0, 0, None) == LDX_EINVAL and "ldx_taesd_conv64" in _last_error(H)
    assert H.L.ldx_taesd_conv64(P["x"], P["ctx"], None, None, None, P["out"], None, 1, 5, 7, 2, 0, 0, None) == LDX_EINVAL
    assert H.L.ldx_taesd_conv64(P["x"], P["ctx"], None, P["y"], P["cc"], P["out"], None, 1, 5, 7, 0, 0, 0, None) == LDX_EINVAL          # both residuals
    assert H.take() == []
    H.check(H.L.ldx_taesd_conv64(P["x"], P["ctx"], P["bias"], None, P["y"], P["out"], P["out2"], 2, 33, 17, 1, 1, 0, None), "ldx_taesd_conv64")
    rec = H.take()
    assert len(rec) == 1 and "taesd_conv_kernel" in rec[0] and "Li2ELb0E" in rec[0] and rec[0].split()[2] == f"{2 * 9 * 2},1,1", rec      # 66 x 34 pixels: 9 x 2 tiles per image


@pytest.mark.parametrize("other", OTHERS)
def test_other_models_refuse_taesd_decode(host, other):
    H, _, others = host
    assert H.L.ldx_profile_report(None, None, 0) == LDX_EINVAL and "ldx_profile_report" in _last_error(H)      # another call's text is in place
    H.take()
    rc = H.L.ldx_taesd_decode(others[other], *_decode_args())
    err = _last_error(H)
    print(f"ldx_taesd_decode on a {other} engine: {rc} {err!r}")
    assert rc == LDX_ESTATE and "ldx_taesd_decode" in err, (other, rc, err)
    assert H.take() == [], f"ldx_taesd_decode on a {other} engine launched, copied or set memory"


@pytest.mark.parametrize("name,args", [("ldx_vae_decode", lambda: (P["x"], 1, 8, 8, P["out"], None)), ("ldx_esrgan_forward", lambda: (P["x"], 1, 16, 16, P["out"], None)),
                                       ("ldx_unet_denoise", lambda: (P["x"], P["s"], P["ctx"], 2, 16, 16, T.MC, P["out"], None)),
                                       ("ldx_t5_encode", lambda: (P["ids"], 1, 40, P["bias"], P["out"], None)),
                                       ("ldx_load_tensor_device", lambda: (b"1.bias", P["x"], F32, (C.c_int64 * 1)(64), 1))])
def test_taesd_engine_refuses_other_models_entry_points(host, name, args):
    H, h, _ = host
    assert H.L.ldx_profile_report(None, None, 0) == LDX_EINVAL
    H.take()
    rc = getattr(H.L, name)(h, *args())
    err = _last_error(H)
    assert rc == LDX_ESTATE and name in err, (name, rc, err)
    assert H.take() == [], f"{name} on the TAESD engine launched, copied or set memory"


def test_null_handle_is_a_bad_argument(host):
    H, _, _ = host
    H.take()
    assert H.L.ldx_taesd_decode(None, *_decode_args()) == LDX_EINVAL and "ldx_taesd_decode" in _last_error(H)
    assert H.take() == []


def test_common_entry_points_answer_as_for_the_other_models(host):
    H, h, others = host
    i64 = lambda: C.byref(C.c_int64())          # noqa: E731
    common = {
        "ldx_plan_info": (LDX_OK, lambda: (i64(), C.byref(C.c_double()), i64())),
        "ldx_plan_flops": (LDX_OK, lambda: (C.byref(C.c_double()), C.byref(C.c_double()))),
        "ldx_profile": (LDX_OK, lambda: (0, 1)),
        "ldx_profile_report": (LDX_OK, lambda: (C.create_string_buffer(64), 64)),
        "ldx_set_graph_mode": (LDX_OK, lambda: (0,)),
        "ldx_graph_stats": (LDX_OK, lambda: (i64(), i64())),
        "ldx_finalize": (LDX_OK, lambda: ()),
        "ldx_load_tensor": (LDX_ESTATE, lambda: (b"some.weight", C.cast((C.c_float * 4)(), C.c_void_p), F32, (C.c_int64 * 1)(4), 1)),
    }
    for name, (code, args) in common.items():
        assert getattr(H.L, name)(h, *args()) == code, (name, _last_error(H))
        assert getattr(H.L, name)(others["esrgan"], *args()) == code, name


def test_missing_weight_is_reported(host):
    H, _, _ = host
    W = H.ldx.weights
    c = H.ldx.lib.ldx_taesd_config()
    c.compute_dtype, c.latent_channels = 1, 4
    h = C.c_void_p()
    H.check(H.L.ldx_taesd_create(C.byref(c), 0, C.byref(h)), "ldx_taesd_create")
    sd = W.synth_state_dict(W.taesd_decoder_state_dict_spec(), dtype=torch.float32)
    del sd["12.weight"]
    H.load(h, sd)
    assert H.L.ldx_finalize(h) == -2 and "12.weight" in _last_error(H)
    assert H.L.ldx_taesd_decode(h, *_decode_args()) == LDX_ESTATE
    H.L.ldx_destroy(h)
    H.take()
