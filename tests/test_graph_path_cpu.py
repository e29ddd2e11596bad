"""The bind / capture / replay call path of the engines, through the C ABI of the host-only build (tests/tools/plan_trace.py).  The stand-in HIP runtime
(tests/tools/hip_standin.cpp) keeps the node list of a captured graph: begin, end, instantiate and launch write one `G` line each, a launch is followed by its
nodes' records, what must stay out of a capture writes a `!` line, and LDX_STANDIN_FAIL makes one graph call fail.  So a call is told apart as

    eager     no G line
    capture   G begin, G end, G instantiate, G launch (+ the nodes), nothing launched between begin and end outside the graph
    replay    G launch (+ the nodes)

and its launches and copies (the `L` / `C` records, those of a launched graph included) are compared with an eager call's byte for byte.  One tiny UNet at a
16 x 16 latent and one TAESD engine at 8 x 8, B = 1; the five models without a graph mode only ignore ldx_set_graph_mode.  No GPU."""
import ctypes as C
import os
import shutil
import sys
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import plan_trace as T  # noqa: E402
from test_engine_kinds_cpu import RUNS  # noqa: E402

LDX_OK, LDX_EHIP = 0, -3
P, MC = T.P, T.MC
EAGER, CAPTURE, REPLAY = [], ["begin", "end", "instantiate", "launch"], ["launch"]
GRAPHED = ("unet", "taesd")
UNGRAPHED = ("vae", "clip", "t5", "esrgan", "flux")
GRAPH_APIS = ("hipStreamEndCapture", "hipGraphInstantiate", "hipGraphLaunch")


@pytest.fixture(scope="module")
def H(ldx_lib):
    """The recorder on a private copy of the host library: the stand-in runtime opens its trace file once per loaded image, and other test modules of the
    same process keep their own."""
    T.build_host()
    tmp = tempfile.mkdtemp(prefix="ldx_graph_path_")
    private = os.path.join(tmp, "libldx_host_graph.so")
    shutil.copy(T.HOST_LIB, private)
    orig, T.HOST_LIB = T.HOST_LIB, private
    try:
        host = T.Host()
    finally:
        T.HOST_LIB = orig
    host.take()
    yield host
    os.unlink(host.path)
    shutil.rmtree(tmp, ignore_errors=True)


@pytest.fixture
def engine(H):
    """engine(model) -> handle of a fresh, finalized tiny engine (fresh: the counters of ldx_graph_stats start at zero); destroyed after the test."""
    made = []

    def make(model):
        h, _ = T._engine(H, (model, "tiny", "bf16", "build", 0, 0, 0, 0, 0))
        H.check(H.L.ldx_finalize(h), "ldx_finalize")
        made.append(h)
        H.take()
        return h
    yield make
    for h in made:
        H.L.ldx_destroy(h)
    H.take()


class Call:
    """The records of one call: .rc, .g (the G lines' verbs in order), .lc (launches and copies), .bang (`!` lines), .nodes (the nodes of the graph launched)."""

    def __init__(self, H, rc):
        self.rc, self.all = rc, H.take()
        self.g = [r.split()[1] for r in self.all if r.startswith("G ")]
        self.lc = [r for r in self.all if r[:2] in ("L ", "C ")]
        self.bang = [r for r in self.all if r.startswith("!")]
        self.nodes = None
        at = [i for i, r in enumerate(self.all) if r.startswith("G launch")]
        if at:
            self.nodes = self.all[at[-1] + 1:]
            assert len(self.nodes) == int(self.all[at[-1]].split()[3]), self.all[at[-1]]
        if "begin" in self.g and "end" in self.g:          # nothing of a capture runs beside the graph, and the graph launched is the graph captured
            b, e = (next(i for i, r in enumerate(self.all) if r.startswith("G " + v)) for v in ("begin", "end"))
            assert e == b + 1, self.all[b:e + 1]
            if self.nodes is not None:
                assert int(self.all[e].split()[3]) == len(self.nodes)


def unet(H, h, out="out", hw=(16, 16), entry="cfg_t"):
    if entry == "cfg_t":          # the sigma fill is launched in front of the plan, outside the graph
        return Call(H, H.L.ldx_unet_denoise_cfg_t(h, P["x"], 3.0, 500, P["ctx"], 1, hw[0], hw[1], MC, P[out], None))
    return Call(H, H.L.ldx_unet_denoise(h, P["x"], P["s"], P["ctx"], 1, hw[0], hw[1], MC, P[out], None))


def taesd(H, h, out="out", hw=(8, 8), u8="out2", flux=0):
    return Call(H, H.L.ldx_taesd_decode(h, P["x"], 1, hw[0], hw[1], P[out], P[u8] if u8 else None, flux, None))


RUN = {"unet": unet, "taesd": taesd}


def stats(H, h):
    c, r = C.c_int64(), C.c_int64()
    H.check(H.L.ldx_graph_stats(h, C.byref(c), C.byref(r)), "ldx_graph_stats")
    return c.value, r.value


def graph_mode(H, h, on):
    H.check(H.L.ldx_set_graph_mode(h, int(on)), "ldx_set_graph_mode")


def expect(H, calls, kinds, same_as=None):
    """Every call succeeded, wrote no `!` line, was of its kind, and launched what `same_as` (default: the first of them) launched."""
    same_as = same_as or calls[0]
    for i, (c, kind) in enumerate(zip(calls, kinds)):
        assert c.rc == LDX_OK, (i, c.rc, H.L.ldx_last_error())
        assert c.bang == [], (i, c.bang)
        assert c.g == kind, (i, c.g, kind)
        assert c.lc == same_as.lc, f"call {i}: launches differ from the eager call's"
        assert any(r.startswith("L ") for r in c.lc)


def three(H, run, h, **kw):
    return [run(H, h, **kw) for _ in range(3)]


# ---- (a) the same pointers three times
@pytest.mark.parametrize("model", GRAPHED)
def test_same_pointers_eager_capture_replay(H, engine, model):
    h = engine(model)
    graph_mode(H, h, 1)
    calls = three(H, RUN[model], h)
    expect(H, calls, [EAGER, CAPTURE, REPLAY])
    assert stats(H, h) == (1, 1)
    if model == "unet":          # the sigma fill stays in front of the graph in all three
        assert all("fill" in c.all[0] and c.all[0].startswith("L ") for c in calls)
        assert calls[1].nodes == calls[0].lc[1:] and calls[2].nodes == calls[0].lc[1:]
    else:
        assert calls[1].nodes == calls[0].lc and calls[2].nodes == calls[0].lc
        assert len(calls[0].lc) == 36


# ---- (b) a stale graph is never replayed
@pytest.mark.parametrize("model", GRAPHED)
def test_other_pointers_run_eagerly_and_invalidate(H, engine, model):
    h, run = engine(model), RUN[model]
    graph_mode(H, h, 1)
    a = three(H, run, h)
    expect(H, a, [EAGER, CAPTURE, REPLAY])
    b = three(H, run, h, out="cc")          # another out pointer
    expect(H, b, [EAGER, CAPTURE, REPLAY])
    assert b[0].lc != a[0].lc
    back = three(H, run, h)                   # the first graph is gone: its pointers were captured again, not replayed
    expect(H, back, [EAGER, CAPTURE, REPLAY], same_as=a[0])
    assert stats(H, h) == (3, 3)


@pytest.mark.parametrize("model", GRAPHED)
def test_eager_call_with_other_pointers_between_graph_calls(H, engine, model):
    """Graph mode off for one call with other pointers, then on again: the graph of the first pointers is not replayed."""
    h, run = engine(model), RUN[model]
    graph_mode(H, h, 1)
    a = three(H, run, h)
    expect(H, a, [EAGER, CAPTURE, REPLAY])
    graph_mode(H, h, 0)
    expect(H, [run(H, h, out="cc")], [EAGER])
    graph_mode(H, h, 1)
    expect(H, three(H, run, h), [EAGER, CAPTURE, REPLAY], same_as=a[0])
    assert stats(H, h) == (2, 2)


def test_taesd_flux_flag_and_u8_output_are_bindings(H, engine):
    h = engine("taesd")
    graph_mode(H, h, 1)
    a = three(H, taesd, h)
    expect(H, a, [EAGER, CAPTURE, REPLAY])
    f = three(H, taesd, h, flux=1)
    expect(H, f, [EAGER, CAPTURE, REPLAY])
    u = three(H, taesd, h, flux=1, u8=None)
    expect(H, u, [EAGER, CAPTURE, REPLAY])
    assert a[0].lc[:-1] == f[0].lc[:-1] == u[0].lc[:-1] and len({a[0].lc[-1], f[0].lc[-1], u[0].lc[-1]}) == 3          # conv_out alone takes them
    assert stats(H, h) == (3, 3)


# ---- (c) shape switches
def test_unet_keeps_the_graph_of_each_shape(H, engine):
    h = engine("unet")
    graph_mode(H, h, 1)
    a = three(H, unet, h)
    expect(H, a, [EAGER, CAPTURE, REPLAY])
    b = three(H, unet, h, hw=(24, 16))
    expect(H, b, [EAGER, CAPTURE, REPLAY])
    assert stats(H, h) == (2, 2)
    expect(H, [unet(H, h)], [REPLAY], same_as=a[0])          # at once, no new capture
    expect(H, [unet(H, h, hw=(24, 16))], [REPLAY], same_as=b[0])
    assert stats(H, h) == (2, 4)


def test_taesd_replans_and_recaptures_each_shape(H, engine):
    h = engine("taesd")
    graph_mode(H, h, 1)
    for i, hw in enumerate(((8, 8), (5, 7), (8, 8))):
        expect(H, three(H, taesd, h, hw=hw), [EAGER, CAPTURE, REPLAY])
        assert stats(H, h) == (i + 1, i + 1)


# ---- (d) the UNet's context cache
def test_unet_context_pass_stays_outside_the_graph(H, engine):
    h = engine("unet")
    ctx_hex = P["ctx"].to_bytes(8, "little").hex()
    full = unet(H, h, entry="denoise")          # cache off: every op
    expect(H, [full], [EAGER])
    graph_mode(H, h, 1)
    H.check(H.L.ldx_unet_context_cache(h, 1), "ldx_unet_context_cache")
    c = three(H, unet, h, entry="denoise")
    for x in c:
        assert x.rc == LDX_OK and x.bang == []
    assert [x.g for x in c] == [EAGER, CAPTURE, REPLAY]
    rest = c[1].nodes
    k = len(full.lc) - len(rest)
    ctx_ops = c[0].lc[:k]          # the first call of a (plan, ctx, epoch): the ctx_only ops eagerly in front, then the rest eagerly
    assert k > 0 and c[0].lc == ctx_ops + rest and sorted(c[0].lc) == sorted(full.lc)
    assert ctx_hex in ctx_ops[0] and not any(ctx_hex in r for r in rest) and not set(ctx_ops) & set(rest)
    assert c[1].lc == rest and c[2].lc == rest and c[2].nodes == rest
    assert stats(H, h) == (1, 1)
    H.check(H.L.ldx_unet_context_cache(h, 1), "ldx_unet_context_cache")          # the epoch bumps
    again = unet(H, h, entry="denoise")
    assert again.rc == LDX_OK and again.bang == [] and again.g == REPLAY
    assert again.all[:k] == ctx_ops and again.all[k].startswith("G launch") and again.nodes == rest
    nxt = unet(H, h, entry="denoise")
    assert nxt.g == REPLAY and nxt.lc == rest
    assert stats(H, h) == (1, 3)


# ---- (e) the models without a graph mode
@pytest.mark.parametrize("model", UNGRAPHED)
def test_graph_mode_is_ignored(H, engine, model):
    h = engine(model)
    graph_mode(H, h, 1)
    calls = []
    for _ in range(3):
        T._run(H, h, None, RUNS[model])          # asserts LDX_OK
        calls.append(Call(H, LDX_OK))
    for c in calls:
        assert c.g == [] and c.bang == [] and any(r.startswith("L ") for r in c.lc)
    assert calls[1].lc == calls[2].lc
    assert stats(H, h) == (0, 0)


# ---- (g) a failing graph call leaves no capture open and no half-made graph behind
@pytest.mark.parametrize("api", GRAPH_APIS)
@pytest.mark.parametrize("model", GRAPHED)
def test_failed_capture_is_closed_and_tried_again(H, engine, monkeypatch, model, api):
    h, run = engine(model), RUN[model]
    graph_mode(H, h, 1)
    first = run(H, h)
    expect(H, [first], [EAGER])
    monkeypatch.setenv("LDX_STANDIN_FAIL", api)
    bad = run(H, h)
    err = H.L.ldx_last_error().decode(errors="replace")
    monkeypatch.delenv("LDX_STANDIN_FAIL")
    assert bad.rc == LDX_EHIP and api in err, (bad.rc, err)
    assert bad.g[:2] == ["begin", "end"] and bad.bang == [], bad.g          # the capture ended
    assert stats(H, h) == (0, 0)
    expect(H, [run(H, h), run(H, h)], [CAPTURE, REPLAY], same_as=first)          # as after an eager call
    assert stats(H, h) == (1, 1)
