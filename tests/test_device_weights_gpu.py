"""Weights packed on the device (ldx_load_tensor_device, csrc/pack.hip) and replaced in place in a finalized engine (ldx_unet_refresh_begin / _commit).

Nothing here has a tolerance: the device packers must produce the bits of the host packers (ldx_weights_digest over every weight buffer is equal) and a
refreshed engine must compute what a fresh engine built from the same state dict computes (torch.equal).  The UNets are the smallest that reach every
packed layout: model_channels 64, channel_mult (1, 2) - ResBlocks with Cin != Cout (the fused 1x1 skip as conv2's last K segment), skip concatenation,
conv_in padded 4 / 9 -> 64 channels - one transformer block at both levels and in the middle (q|k|v with the prescaled q rows, the GEGLU row permutation, the
batched emb_layers and k|v projections, the LayerNorm-folded copies).  Source tensors mix fp16, fp32 and bf16 key by key.  The folded copies are built by
default; the plan switch that leaves them out (LDX_LNFOLD=0) is read when the library loads, so that variant runs this file as a script in a child process.
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MIXED = (torch.float16, torch.float32, torch.bfloat16)


def small_cfg(ldx, in_channels=4):
    return ldx.UNetConfig(in_channels=in_channels, out_channels=4, model_channels=64, channel_mult=(1, 2), num_res_blocks=(1, 1),
                          transformer_depth=(1, 1), transformer_depth_output=(1, 1, 1, 1), transformer_depth_middle=1, num_heads=8, context_dim=128)


def synth(ldx, cfg, seed, dtypes=MIXED, only=None, base=None):
    """A state dict whose tensors cycle through `dtypes`; with `only` (a predicate on the key) and `base`: base with just those keys drawn again."""
    out = {}
    for i, (k, shape) in enumerate(ldx.weights.unet_state_dict_spec(cfg)):
        if base is not None and not only(k):
            out[k] = base[k]
        else:
            out[k] = ldx.weights.synth_tensor(k, shape, seed, torch.float32).to(dtypes[i % len(dtypes)])
    return out


def cuda(sd):
    return {k: v.cuda() for k, v in sd.items()}


class Inputs:
    """One fixed set of call arguments per (config, latent size); the tensors persist, so graph replays and the context cache see the same addresses."""

    def __init__(self, cfg, h, w, seed=11):
        g = torch.Generator().manual_seed(seed)
        self.cfg = cfg
        self.x = torch.randn([2, 4, h, w], generator=g).cuda()
        self.x_in = torch.randn([2, cfg.in_channels, h, w], generator=g).cuda()
        self.cc = torch.randn([2, cfg.in_channels - 4, h, w], generator=g).cuda() if cfg.in_channels > 4 else None
        self.ctx = torch.randn([2, 77, cfg.context_dim], generator=g).cuda()
        self.sigma = torch.tensor([3.7, 0.45]).cuda()
        self.t = torch.tensor([500.0, 17.0]).cuda()
        self.out = torch.empty([2, 4, h, w], device="cuda")

    def denoise(self, eng, ctx_cached=False):
        return eng.denoise(self.x, self.sigma, self.ctx, out=self.out, c_concat=self.cc, ctx_cached=ctx_cached).clone()

    def everything(self, eng):
        """denoise, forward and (4-channel UNets: the CFG call takes no c_concat) denoise_cfg with the shared prefix off and forced."""
        res = {"denoise": self.denoise(eng), "forward": eng.forward(self.x_in, self.t, self.ctx).clone()}
        if self.cc is None:
            for share in (0, 2):
                eng.set_cfg_share(share)
                res[f"cfg_share{share}"] = eng.denoise_cfg(self.x[:1].contiguous(), 3.7, self.ctx).clone()
            eng.set_cfg_share(1)
        return res


def assert_same(got, want, what):
    assert got.keys() == want.keys()
    for k in want:
        assert torch.equal(got[k], want[k]), f"{what}: {k} differs (max abs {float((got[k] - want[k]).abs().max()):.3e})"


def check_device_equals_host(ldx, in_channels, dt, h, w):
    cfg = small_cfg(ldx, in_channels)
    sd = synth(ldx, cfg, seed=3)
    inp = Inputs(cfg, h, w)
    host = ldx.UNetEngine(cfg, sd, device=0, dtype=dt)
    dev = ldx.UNetEngine(cfg, cuda(sd), device=0, dtype=dt)
    # host and device tensors mixed key by key: every third key from the host, so fused buffers (conv2 | skip, q|k|v, emb_all, kv_all) see both kinds
    mixed = ldx.UNetEngine(cfg, {k: (v if i % 3 == 0 else v.cuda()) for i, (k, v) in enumerate(sd.items())}, device=0, dtype=dt)
    want_digest, want = host.weights_digest(), inp.everything(host)
    for name, e in (("device", dev), ("mixed", mixed)):
        assert e.weights_digest() == want_digest, f"{name}: packed weights differ from the host path's"
        assert_same(inp.everything(e), want, name)
    for e in (host, dev, mixed):
        e.close()


@pytest.mark.parametrize("in_channels,dt,h,w", [(4, "bf16", 16, 16), (9, "f16", 24, 16), (4, "f16", 24, 16), (9, "bf16", 16, 16)])
def test_device_build_equals_host_build(ldx, ldx_lib, in_channels, dt, h, w):
    check_device_equals_host(ldx, in_channels, dt, h, w)


@pytest.fixture(scope="module")
def base(ldx, ldx_lib):
    """S_A, the arguments and what a fresh engine computes from S_A (shared, never modified)."""
    cfg = small_cfg(ldx)
    sd_a = synth(ldx, cfg, seed=3)
    inp = Inputs(cfg, 16, 16)
    e = ldx.UNetEngine(cfg, sd_a, device=0, dtype="bf16")
    out_a, digest_a = inp.denoise(e), e.weights_digest()
    e.close()
    return cfg, sd_a, inp, out_a, digest_a


def fresh(ldx, cfg, sd, inp):
    e = ldx.UNetEngine(cfg, sd, device=0, dtype="bf16")
    try:
        return inp.denoise(e), e.weights_digest()
    finally:
        e.close()


def test_refresh_in_place_keeps_plans_and_graphs(ldx, base):
    cfg, sd_a, inp, out_a, digest_a = base
    sd_b = synth(ldx, cfg, seed=4)
    want_b, digest_b = fresh(ldx, cfg, sd_b, inp)
    other = Inputs(cfg, 24, 16, seed=12)              # a shape the refreshed engine has not planned yet: its first call runs eagerly
    eb = ldx.UNetEngine(cfg, sd_b, device=0, dtype="bf16")
    want_other = other.denoise(eb)
    eb.close()
    assert not torch.equal(want_b, out_a)

    e = ldx.UNetEngine(cfg, cuda(sd_a), device=0, dtype="bf16", graph=True)
    for _ in range(5):                                  # eager warm-up passes, the capture, replays
        assert torch.equal(inp.denoise(e), out_a)
    captures, replays = e.graph_stats()
    assert captures >= 1 and replays >= 1, (captures, replays)
    info = e.plan_info()

    e.refresh(cuda(sd_b))
    assert e.weights_digest() == digest_b
    assert torch.equal(inp.denoise(e), want_b), "replayed graph after the refresh"
    assert e.plan_info() == info
    c2, r2 = e.graph_stats()
    assert c2 == captures and r2 == replays + 1, "the captured graph must be replayed, not captured again"
    assert torch.equal(other.denoise(e), want_other), "eager pass of a new plan after the refresh"

    e.refresh(sd_a)                                     # and back, from host tensors this time
    assert e.weights_digest() == digest_a
    assert torch.equal(inp.denoise(e), out_a)
    e.close()


def test_refresh_rebuilds_the_emb_table(ldx, base):
    cfg, sd_a, inp, out_a, _ = base
    sd_b = synth(ldx, cfg, seed=5, only=lambda k: k.startswith("time_embed.") or ".emb_layers." in k, base=sd_a)
    want, digest = fresh(ldx, cfg, sd_b, inp)
    assert not torch.equal(want, out_a)
    e = ldx.UNetEngine(cfg, sd_a, device=0, dtype="bf16")
    assert torch.equal(inp.denoise(e), out_a)
    e.refresh(cuda(sd_b))
    assert e.weights_digest() == digest
    assert torch.equal(inp.denoise(e), want)
    e.close()


def test_refresh_drops_the_context_cache(ldx, base):
    cfg, sd_a, inp, out_a, _ = base
    sd_b = synth(ldx, cfg, seed=6, only=lambda k: ".attn2.to_k." in k or ".attn2.to_v." in k, base=sd_a)
    want, _ = fresh(ldx, cfg, sd_b, inp)
    assert not torch.equal(want, out_a)
    e = ldx.UNetEngine(cfg, sd_a, device=0, dtype="bf16")
    for _ in range(2):                                  # the second call reuses the cached k|v projections of inp.ctx
        assert torch.equal(inp.denoise(e, ctx_cached=True), out_a)
    e.refresh(cuda(sd_b))
    assert torch.equal(inp.denoise(e, ctx_cached=True), want), "projections cached before the refresh were used after it"
    e.close()


def test_lora_through_the_hook(ldx, ldx_lib, golden_dir):
    """The project's own host LoRA merge (checkpoint.merge_lora, tests/golden/lora.npz) applied to S_A gives S_B; a patch refreshed to S_B answers the recorded
    hook arguments exactly as a patch built from S_B."""
    ck = ldx.checkpoint
    cfg = ldx.UNetConfig.tiny(64, 128)
    sd_a = ldx.weights.synth_state_dict(ldx.weights.unet_state_dict_spec(cfg), seed=1234)
    g = np.load(os.path.join(golden_dir, "lora.npz"))
    lora = {k[len("lora::"):]: torch.from_numpy(g[k]) for k in g.files if k.startswith("lora::")}
    merged, n = ck.merge_lora({k: v.float() for k, v in sd_a.items()}, lora, ck.lora_key_map_unet(cfg, sd_a.keys()), strength=0.7)
    assert n == 4
    sd_b = {k: v.half() for k, v in merged.items()}
    rec = np.load(os.path.join(golden_dir, "unet_mc64.npz"))
    calls = [{"input": torch.from_numpy(rec[f"hook{i}_input"]), "timestep": torch.from_numpy(rec[f"hook{i}_timestep"]),
              "c": {"c_crossattn": torch.from_numpy(rec[f"hook{i}_ctx"]), "transformer_options": {}}, "cond_or_uncond": list(rec[f"hook{i}_cou"])}
             for i in range(int(rec["hook_n"]))]
    patch_b = ldx.LdxUNetPatch.from_state_dict(sd_b, cfg, device=0, dtype="bf16")
    patch = ldx.LdxUNetPatch.from_state_dict(cuda(sd_a), cfg, device=0, dtype="bf16")
    before = [patch(None, p) for p in calls]
    patch.refresh(cuda(sd_b))
    assert patch.engine.weights_digest() == patch_b.engine.weights_digest()
    after, want = [patch(None, p) for p in calls], [patch_b(None, p) for p in calls]
    assert all(torch.equal(a, w) for a, w in zip(after, want))
    assert any(not torch.equal(a, b) for a, b in zip(after, before)), "the LoRA changes the output: the refresh is actually exercised"
    patch.engine.close(); patch_b.engine.close()


def test_errors_leave_the_engine_as_it_was(ldx, base):
    cfg, sd_a, inp, out_a, digest_a = base
    LdxError = ldx.lib.LdxError
    e = ldx.UNetEngine(cfg, cuda(sd_a), device=0, dtype="bf16")
    sd_b = cuda(synth(ldx, cfg, seed=7))

    def still_a():
        assert e.weights_digest() == digest_a and torch.equal(inp.denoise(e), out_a)

    still_a()
    # a load after finalize without begin
    t = sd_b["out.0.weight"].float().contiguous()
    shape = (C.c_int64 * 1)(t.shape[0])
    for fn, arg in ((e._lib.ldx_load_tensor_device, t), (e._lib.ldx_load_tensor, t.cpu())):
        with pytest.raises(LdxError, match="after ldx_finalize"):
            ldx.lib.check(fn(e._h, b"out.0.weight", ldx.lib.ptr(arg), ldx.lib.LDX_F32, shape, 1), "load")
    with pytest.raises(LdxError, match="refresh_begin"):
        ldx.lib.check(e._lib.ldx_unet_refresh_commit(e._h), "commit")
    # a key missing: one of the last the structure walk asks for (a walk that did not validate first would have rewritten everything in front of it)
    for key in ("out.2.weight", "middle_block.1.transformer_blocks.0.attn2.to_k.weight"):
        with pytest.raises(LdxError, match=key.replace(".", r"\.")):
            e.refresh({k: v for k, v in sd_b.items() if k != key})
        still_a()
    # a wrong shape
    key = "output_blocks.0.0.skip_connection.weight"
    bad = dict(sd_b)
    bad[key] = sd_b[key][:, :-1].contiguous()
    with pytest.raises(LdxError, match=key.replace(".", r"\.")):
        e.refresh(bad)
    still_a()
    # rejected in Python: a non-contiguous device tensor (one on another GPU: test_tensor_on_another_device_is_rejected)
    key = "time_embed.2.weight"
    bad = dict(sd_b)
    bad[key] = sd_b[key].t().contiguous().t()
    assert bad[key].shape == sd_b[key].shape and not bad[key].is_contiguous()
    with pytest.raises(ValueError, match="contiguous"):
        e.refresh(bad)
    still_a()
    with pytest.raises(ValueError, match="contiguous"):
        ldx.UNetEngine(cfg, bad, device=0, dtype="bf16")
    # the refresh that Python gave up is closed: the loaders answer LDX_ESTATE again
    with pytest.raises(LdxError, match="after ldx_finalize"):
        ldx.lib.check(e._lib.ldx_load_tensor_device(e._h, b"out.0.weight", ldx.lib.ptr(t), ldx.lib.LDX_F32, shape, 1), "load")
    # and the engine still takes a proper refresh
    e.refresh(sd_b)
    assert e.weights_digest() != digest_a
    e.close()


def test_tensor_on_another_device_is_rejected(ldx, base):
    """The engine reads a device tensor where it lies, so one on another GPU is refused in Python before its address is used.  With a second GPU the
    tensor is a real one; on a one-GPU machine an object with the three attributes the loader looks at (detach, is_cuda, device) stands in for it:
    the refusal is decided on those alone."""
    cfg, sd_a, inp, out_a, digest_a = base

    class Elsewhere:
        is_cuda, device = True, torch.device("cuda", 1)

        def detach(self):
            return self

    key = "time_embed.2.weight"
    bad = cuda(sd_a)
    bad[key] = sd_a[key].to("cuda:1") if torch.cuda.device_count() > 1 else Elsewhere()
    with pytest.raises(ValueError, match="cuda:1"):
        ldx.UNetEngine(cfg, bad, device=0, dtype="bf16")
    e = ldx.UNetEngine(cfg, sd_a, device=0, dtype="bf16")
    with pytest.raises(ValueError, match="cuda:1"):
        e.refresh(bad)
    assert e.weights_digest() == digest_a and torch.equal(inp.denoise(e), out_a)
    e.close()


def test_device_build_equals_host_build_without_ln_fold(ldx_lib):
    """LDX_LNFOLD=0 (plain weights only, read at library load): the same comparison in a child process.  Last in the file, and a child that does not
    come back ends the session: nothing is started on a GPU that may be hung."""
    try:
        r = subprocess.run([sys.executable, os.path.abspath(__file__)], env=dict(os.environ, LDX_LNFOLD="0"), capture_output=True, text=True, timeout=300)
    except subprocess.TimeoutExpired:          # run() has killed the child
        pytest.exit("the LDX_LNFOLD=0 child process did not finish: stopping the session", returncode=1)
    print(r.stdout[-2000:], r.stderr[-2000:])
    assert r.returncode == 0 and "NOFOLD_OK" in r.stdout


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    import ldx_amd

    assert os.environ.get("LDX_LNFOLD") == "0"
    check_device_equals_host(ldx_amd, 4, "bf16", 16, 16)
    check_device_equals_host(ldx_amd, 9, "f16", 24, 16)
    print("NOFOLD_OK")
