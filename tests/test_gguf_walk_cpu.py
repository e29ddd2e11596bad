"""The Flux and T5 weight walks read device-resident sources (ldx_load_tensor_dev; the fp16 expansions of ldx_load_tensor_q8_0 are such sources too).  On the
host-only build (tests/tools/plan_trace.py: a stand-in HIP runtime that records every launch and copy) the tiny net of each is loaded three ways: every tensor
from the host, every tensor at a made-up device address, every third key from the host.  The walks ask for the same buffers in the same order either way; with
device sources every 16-bit matrix and fp32 vector is written by pack.hip's kernels (linear1's row split and T5's two-tensor wi slabs included: no layout is
left on a host getter), and host tensors that share a walk with device tensors are staged as raw copies.  No GPU."""
import os
import shutil
import sys
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import plan_trace as T  # noqa: E402


@pytest.fixture(scope="module")
def host(ldx_lib):
    """The recorder on a private copy of the host library: the stand-in runtime opens its trace file once per loaded image, and other test modules of the
    same process keep their own."""
    T.build_host()
    tmp = tempfile.mkdtemp(prefix="ldx_gguf_walk_")
    private = os.path.join(tmp, "libldx_host_gguf.so")
    shutil.copy(T.HOST_LIB, private)
    orig, T.HOST_LIB = T.HOST_LIB, private
    try:
        H = T.Host()
    finally:
        T.HOST_LIB = orig
    H.take()
    yield H
    os.unlink(H.path)
    shutil.rmtree(tmp, ignore_errors=True)


def _load(H, model, how):
    h, _ = T._engine(H, (model, "tiny", "bf16", "build", 0, 0, 0, 0, 0)) if how == "build" else _engine_dev(H, model, how)
    H.take()
    H.check(H.L.ldx_finalize(h), "ldx_finalize")
    rec = H.take()
    H.L.ldx_destroy(h)
    return rec


def _engine_dev(H, model, how):
    """plan_trace._engine with the tensors registered through ldx_load_tensor_dev."""
    real = H.L.ldx_load_tensor_device
    H.L.ldx_load_tensor_device = H.L.ldx_load_tensor_dev          # Host.load calls it for "build_dev" / "build_mixed"
    load = H.load
    H.load = lambda h, sd, strip=(), how_=how: load(h, sd, strip, how)
    try:
        return T._engine(H, (model, "tiny", "bf16", "build", 0, 0, 0, 0, 0))
    finally:
        H.L.ldx_load_tensor_device = real
        del H.load


@pytest.mark.parametrize("model", ["flux", "t5"])
def test_device_sources_walk_like_host_sources(host, model):
    base = _load(host, model, "build")
    launches = lambda rec: [r for r in rec if r.startswith("L ")]
    assert not launches(base), "a host-only load launches nothing"
    for how in ("build_dev", "build_mixed"):
        rec = _load(host, model, how)
        names = {r.split()[1] for r in launches(rec)}
        print(model, how, len(rec), "records,", len(launches(rec)), "launches:", sorted(names))
        assert names and all("pack16_kernel" in n or "pack32_kernel" in n for n in names), names
        if how == "build_dev":
            # one launch per piece, and a piece per source tensor, but for linear1, whose weight and bias are each read as two sub-views
            W = host.ldx.weights
            if model == "flux":
                cfg = W.FluxConfig.tiny()
                want = len(W.flux_state_dict_spec(cfg)) + 2 * cfg.depth_single_blocks
            else:
                want = len(W.t5_state_dict_spec(W.T5Config.tiny())) - 1          # the relative-attention table stays with the host
            assert len(launches(rec)) == want == len(rec)
