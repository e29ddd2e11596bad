"""A model's entry points are reachable only through that model's engine.  The tiny net of each of the six models is created and finalized through the C ABI of
the host-only build (tests/tools/plan_trace.py: a stand-in HIP runtime records every launch, asynchronous copy and memset), and every model-specific entry point is
called on the five engines of the OTHER models with made-up pointers of valid shape: the answer is the code of the table below, ldx_last_error names the entry
point, and the stand-in runtime has recorded nothing.  The same call on the model's own engine returns LDX_OK and launches.  No GPU."""
import ctypes as C
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import plan_trace as T  # noqa: E402

LDX_OK, LDX_EINVAL, LDX_ESTATE = 0, -1, -4
MODELS = ("unet", "vae", "clip", "t5", "esrgan", "flux")
P, MC = T.P, T.MC
F32 = 2


def _u64():
    return C.byref(C.c_uint64())


def _i64():
    return C.byref(C.c_int64())


# entry point -> (its model, the code a finalized engine of another model answers, arguments behind the handle)
ENTRY_POINTS = {
    "ldx_unet_denoise": ("unet", LDX_ESTATE, lambda: (P["x"], P["s"], P["ctx"], 2, 16, 16, MC, P["out"], None)),
    "ldx_unet_denoise_concat": ("unet", LDX_ESTATE, lambda: (P["x"], P["s"], P["ctx"], P["cc"], 5, 2, 16, 16, MC, P["out"], None)),
    "ldx_unet_denoise_cfg": ("unet", LDX_ESTATE, lambda: (P["x"], 3.0, P["ctx"], 1, 16, 16, MC, P["out"], None)),
    "ldx_unet_denoise_cfg_t": ("unet", LDX_ESTATE, lambda: (P["x"], 3.0, 500, P["ctx"], 1, 16, 16, MC, P["out"], None)),
    "ldx_unet_denoise_t": ("unet", LDX_ESTATE, lambda: (P["x"], P["s"], P["t"], P["ctx"], 2, 16, 16, MC, P["out"], None)),
    "ldx_unet_forward": ("unet", LDX_ESTATE, lambda: (P["x"], P["s"], P["ctx"], 2, 16, 16, MC, P["out"], None)),
    "ldx_unet_timestep": ("unet", LDX_ESTATE, lambda: (P["s"], 4, P["out"], None)),
    "ldx_unet_cfg_share": ("unet", LDX_ESTATE, lambda: (1,)),
    "ldx_unet_context_cache": ("unet", LDX_ESTATE, lambda: (0,)),
    "ldx_unet_refresh_begin": ("unet", LDX_ESTATE, lambda: ()),
    "ldx_unet_refresh_commit": ("unet", LDX_ESTATE, lambda: ()),
    "ldx_unet_refresh_abort": ("unet", LDX_ESTATE, lambda: ()),
    "ldx_weights_digest": ("unet", LDX_ESTATE, lambda: (_u64(),)),
    "ldx_load_tensor_device": ("unet", LDX_ESTATE, lambda: (b"time_embed.0.bias", P["x"], F32, (C.c_int64 * 1)(256), 1)),
    # the one answer that differs from the commit before the engines were split, where a handle of another model fell through to the UNet's own checks
    "ldx_set_tables": ("unet", LDX_ESTATE, lambda: (P["s"], 1000, P["t"], 64)),
    "ldx_vae_decode": ("vae", LDX_ESTATE, lambda: (P["x"], 1, 8, 8, P["out"], None)),
    "ldx_vae_encode": ("vae", LDX_ESTATE, lambda: (P["x"], 1, 64, 64, P["out"], None)),
    "ldx_clip_encode": ("clip", LDX_ESTATE, lambda: (P["ids"], 1, 77, 0, P["out"], None, None)),
    "ldx_clip_pooled": ("clip", LDX_ESTATE, lambda: (P["x"], P["ids"], 1, 77, 2, P["out"], None)),
    "ldx_clip_set_extra_embeddings": ("clip", LDX_ESTATE, lambda: (None, 0)),
    "ldx_t5_encode": ("t5", LDX_ESTATE, lambda: (P["ids"], 1, 40, P["bias"], P["out"], None)),
    "ldx_esrgan_forward": ("esrgan", LDX_ESTATE, lambda: (P["x"], 1, 16, 16, P["out"], None)),
    "ldx_flux_forward": ("flux", LDX_ESTATE, lambda: (P["x"], P["s"], P["ctx"], P["y"], P["guid"], P["cos"], P["sin"], 1, 16, 16, 40, 1, P["out"], None)),
    "ldx_flux_fbcache": ("flux", LDX_EINVAL, lambda: (0.1,)),
    "ldx_flux_set_fp8": ("flux", LDX_EINVAL, lambda: (1,)),
    "ldx_flux_fbcache_stats": ("flux", LDX_EINVAL, lambda: (_i64(), _i64())),
}
# what every model answers alike, on a finalized engine: LDX_OK, but for ldx_load_tensor, whose loader ldx_finalize has closed
COMMON = {
    "ldx_plan_info": (LDX_OK, lambda: (_i64(), C.byref(C.c_double()), _i64())),
    "ldx_plan_flops": (LDX_OK, lambda: (C.byref(C.c_double()), C.byref(C.c_double()))),
    "ldx_profile": (LDX_OK, lambda: (0, 1)),
    "ldx_profile_report": (LDX_OK, lambda: (C.create_string_buffer(64), 64)),
    "ldx_set_graph_mode": (LDX_OK, lambda: (0,)),
    "ldx_graph_stats": (LDX_OK, lambda: (_i64(), _i64())),
    "ldx_finalize": (LDX_OK, lambda: ()),
    "ldx_load_tensor": (LDX_ESTATE, lambda: (b"some.weight", C.cast((C.c_float * 4)(), C.c_void_p), F32, (C.c_int64 * 1)(4), 1)),
}
# one run per model on its own engine (plan_trace rows)
RUNS = {
    "unet": ("unet", "tiny", "bf16", "denoise", 16, 16, 1, 1, 0),
    "vae": ("vae", "tiny", "bf16", "decode", 8, 8, 1, 0, 0),
    "clip": ("clip", "tiny", "bf16", "encode", 77, 0, 1, 0, 0),
    "t5": ("t5", "tiny", "bf16", "encode", 40, 0, 1, 0, 0),
    "esrgan": ("esrgan", "tiny", "bf16", "forward", 16, 16, 1, 0, 0),
    "flux": ("flux", "tiny", "bf16", "forward", 16, 16, 1, 0, 40),
}


@pytest.fixture(scope="module")
def host(ldx_lib):
    """(Host, {model: (handle, config)}): the six tiny engines, finalized."""
    T.build_host()
    H = T.Host()
    engines = {}
    for model in MODELS:
        h, cfg = T._engine(H, (model, "tiny", "bf16", "build", 0, 0, 0, 0, 0))
        H.check(H.L.ldx_finalize(h), "ldx_finalize")
        engines[model] = (h, cfg)
    H.take()
    yield H, engines
    for h, _ in engines.values():
        H.L.ldx_destroy(h)
    os.unlink(H.path)


def _last_error(H):
    return H.L.ldx_last_error().decode(errors="replace")


def test_every_model_entry_point_is_listed(ldx):
    """Whatever takes an engine handle is either a model's own (ENTRY_POINTS) or answers every model alike (COMMON); creation and destruction aside."""
    takes_handle = {n for n, (_, args) in ldx.lib._SIGS.items() if n.startswith(("ldx_unet_", "ldx_vae_", "ldx_clip_", "ldx_t5_", "ldx_esrgan_", "ldx_flux_"))
                    and not n.endswith("_create")}
    assert takes_handle <= set(ENTRY_POINTS)
    assert {e[0] for e in ENTRY_POINTS.values()} == set(MODELS) and not set(ENTRY_POINTS) & set(COMMON)


@pytest.mark.parametrize("name", ENTRY_POINTS)
def test_wrong_model_is_refused_before_anything_runs(host, name):
    H, engines = host
    model, code, args = ENTRY_POINTS[name]
    for other in MODELS:
        if other == model:
            continue
        assert H.L.ldx_profile_report(None, None, 0) == LDX_EINVAL and "ldx_profile_report" in _last_error(H)      # another call's text is in place
        H.take()
        rc = getattr(H.L, name)(engines[other][0], *args())
        err = _last_error(H)
        print(f"{name} on a {other} engine: {rc} {err!r}")
        assert rc == code, (name, other, rc, err)
        assert name in err, (name, other, err)
        assert H.take() == [], f"{name} on a {other} engine launched, copied or set memory"


@pytest.mark.parametrize("model", MODELS)
def test_own_model_runs(host, model):
    H, engines = host
    H.take()
    T._run(H, *engines[model], RUNS[model])          # asserts LDX_OK
    records = H.take()
    assert any(r.startswith("L ") for r in records), f"{RUNS[model]}: no launch recorded"


@pytest.mark.parametrize("name", COMMON)
def test_common_entry_points_answer_every_model_alike(host, name):
    H, engines = host
    code, args = COMMON[name]
    for model in MODELS:
        rc = getattr(H.L, name)(engines[model][0], *args())
        assert rc == code, (name, model, rc, _last_error(H))


@pytest.mark.parametrize("name", list(ENTRY_POINTS) + list(COMMON))
def test_null_handle_is_a_bad_argument(host, name):
    H, _ = host
    args = (ENTRY_POINTS[name][2] if name in ENTRY_POINTS else COMMON[name][1])()
    H.take()
    assert getattr(H.L, name)(None, *args) == LDX_EINVAL and _last_error(H)
    assert H.take() == []
