"""GroupNorm statistics taken from the producer (conv / GEMM epilogue, round 3; split-K reduce launch, round 3 late) against the plain
statistics pass: the switches are read once per process, so each variant runs the SD1.5 UNet at 1024^2 in a subprocess on the same seeded
inputs.  The variants differ only in the fp32 summation order of the statistics (values summed are the stored 16-bit outputs in every
variant), so the outputs agree to well inside the engine-vs-oracle tolerance (2.5e-2), and every fusion removes launches."""
import os
import subprocess
import sys
import tempfile

import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SCRIPT = r"""
import sys, torch
sys.path.insert(0, %r)
import ldx_amd as ldx
cfg = ldx.UNetConfig.sd15()
sd = ldx.weights.synth_state_dict(ldx.weights.unet_state_dict_spec(cfg), seed=1234)
eng = ldx.UNetEngine(cfg, sd, device=0, dtype="bf16")
g = torch.Generator().manual_seed(11)
x = (torch.randn(2, 4, 128, 128, generator=g) * 3.0).cuda(); sig = torch.tensor([2.5, 2.5]).cuda(); ctx = torch.randn(2, 77, 768, generator=g).cuda()
out = eng.denoise(x, sig, ctx).clone()
assert torch.equal(out, eng.denoise(x, sig, ctx))
torch.save({"out": out.cpu(), "launches": eng.plan_info()["launches"]}, sys.argv[1])
"""


def _run(env, path):
    r = subprocess.run([sys.executable, "-c", SCRIPT % ROOT, path], cwd=ROOT, env=dict(os.environ, **env), capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return torch.load(path)


def test_gn_statistics_from_producers_match_the_plain_pass(ldx_lib):
    with tempfile.TemporaryDirectory() as d:
        plain = _run({"LDX_GN_FUSE": "0"}, os.path.join(d, "a.pt"))
        epi = _run({"LDX_GN_FUSE_SPLITK": "0"}, os.path.join(d, "b.pt"))
        full = _run({}, os.path.join(d, "c.pt"))
    rel = lambda a, b: float((a.double() - b.double()).norm() / b.double().norm())
    r1, r2 = rel(epi["out"], plain["out"]), rel(full["out"], plain["out"])
    print(f"launches plain {plain['launches']}  epilogue {epi['launches']}  + split-K reduce {full['launches']};  rel-L2 vs plain {r1:.2e} / {r2:.2e}")
    assert plain["launches"] > epi["launches"] > full["launches"]
    assert torch.isfinite(full["out"]).all() and r1 <= 1e-2 and r2 <= 1e-2      # measured 5.8e-3: one bf16 flip early in the net decorrelates the roundings after it


def test_fused_c320_sub_blocks_match_the_separate_launches(ldx_lib):
    """rowgemm / xattn_block / ff_block (LayerNorm + q|k|v, GroupNorm + proj_in, to_out + residual, the cross-attention and feed-forward sub-blocks
    of the C = 320 level as single launches) against the same engine with the separate launches: same roundings, other summation orders."""
    with tempfile.TemporaryDirectory() as d:
        sep = _run({"LDX_XATTN_FUSE": "0", "LDX_FF_FUSE": "0", "LDX_ROWGEMM": "0"}, os.path.join(d, "a.pt"))
        fused = _run({}, os.path.join(d, "b.pt"))
    r = float((fused["out"].double() - sep["out"].double()).norm() / sep["out"].double().norm())
    print(f"launches separate {sep['launches']}  fused {fused['launches']};  rel-L2 {r:.2e}")
    assert sep["launches"] - fused["launches"] >= 30          # 35 at 1024^2: 6 per transformer block + the proj_in pair, 5 blocks
    assert torch.isfinite(fused["out"]).all() and r <= 1e-2


# The same comparison where it takes seconds: the two-level net of 320 / 640 channels (tests/tools/xf_picks.py CONFIGS) at a 32 x 32 latent, evaluation batch 2.  The C = 320
# level has 2048 rows (16 row blocks, HW % 128 == 0), the C = 640 level 512 (HW % 64 == 0): the smallest shapes at which every stage choice of the planner is taken once
# the chip-fill limits are lifted.  Once as a plain evaluation, once as a CFG evaluation with the shared prefix (share mode 2: the prefix limit and the dual stores).
SMALL_SCRIPT = r"""
import ctypes as C, os, sys, torch
sys.path.insert(0, %r)
sys.path.insert(0, os.path.join(%r, "tests", "tools"))
import ldx_amd as ldx
import xf_picks
cfg = ldx.UNetConfig(**xf_picks.CONFIGS["two_level_320"])
sd = ldx.weights.synth_state_dict(ldx.weights.unet_state_dict_spec(cfg), seed=1234)
eng = ldx.UNetEngine(cfg, sd, device=0, dtype="bf16")
g = torch.Generator().manual_seed(11)
x = (torch.randn(2, 4, 32, 32, generator=g) * 3.0).cuda(); sig = torch.tensor([2.5, 2.5]).cuda(); ctx = torch.randn(2, 77, 768, generator=g).cuda()
out = eng.denoise(x, sig, ctx).clone()
assert torch.equal(out, eng.denoise(x, sig, ctx))
res = {"out": out.cpu(), "launches": eng.plan_info()["launches"]}
eng.set_cfg_share(2)
x1 = x[:1].contiguous()
cfg_out = eng.denoise_cfg(x1, 2.5, ctx).clone()
assert torch.equal(cfg_out, eng.denoise_cfg(x1, 2.5, ctx))
assert eng.plan_info()["flops_shared"] > 0
res.update(cfg_out=cfg_out.cpu(), cfg_launches=eng.plan_info()["launches"])
probe = (C.c_int32 * len(xf_picks.FIELDS))()
for name, row in (("p320", (320, 8, 2, 1024, 77, 0, 1, 0)), ("p320_shared", (320, 8, 2, 1024, 77, 1, 1, 0)), ("p640", (640, 8, 2, 256, 77, 0, 1, 0))):
    assert ldx.lib.load().ldx_op_xf_pick(*row, probe) == 0
    res[name] = dict(zip(xf_picks.FIELDS, probe))
torch.save(res, sys.argv[1])
"""


def test_planner_row_block_path_on_a_small_net_matches_the_separate_launches(ldx_lib):
    """What a plan reaches only through the planner's stage choice (rowgemm with every prologue, xattn_block, ff_block, the prefix limit, the dual stores) against the
    same engine on separate launches.  Measured rel-L2 on MI355X: see the assertion."""
    def run(env, path):
        r = subprocess.run([sys.executable, "-c", SMALL_SCRIPT % (ROOT, ROOT), path], cwd=ROOT, env=dict(os.environ, **env), capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        return torch.load(path)
    with tempfile.TemporaryDirectory() as d:
        sep = run({"LDX_ROWGEMM": "0", "LDX_XATTN_FUSE": "0", "LDX_FF_FUSE": "0"}, os.path.join(d, "a.pt"))
        fused = run({"LDX_ROWBLOCK_MINWG": "0", "LDX_ROWBLOCK_MINWG_PREFIX": "0"}, os.path.join(d, "b.pt"))
    for k in ("p320", "p320_shared"):          # the probe: every stage of the C = 320 level is a row-block launch ...
        p = fused[k]
        assert not p["fold"] and p["proj_out"] == 1 and all(p[f"{b}.{f}"] == 1 for b in ("first", "rest") for f in ("qkv", "o1", "xattn", "ffblock")), (k, p)
    p = fused["p640"]                          # ... and of the C = 640 level every projection next to an attention (the sub-block kernels are C = 320 only)
    assert not p["fold"] and p["proj_out"] == 1 and all(p[f"first.{f}"] == 1 for f in ("qkv", "o1", "q2", "o2")) and not p["first.xattn"] and not p["first.ffblock"], p
    assert not any(v == 1 for k in ("p320", "p640") for f, v in sep[k].items() if f.split(".")[-1] in ("qkv", "o1", "xattn", "q2", "o2", "ffblock", "ff1", "proj_out")), sep
    rel = lambda a, b: float((a.double() - b.double()).norm() / b.double().norm())
    r, rc = rel(fused["out"], sep["out"]), rel(fused["cfg_out"], sep["cfg_out"])
    print(f"launches separate {sep['launches']} / {sep['cfg_launches']} (CFG)  fused {fused['launches']} / {fused['cfg_launches']};  rel-L2 {r:.2e} / {rc:.2e} (CFG)")
    assert fused["launches"] < sep["launches"] and fused["cfg_launches"] < sep["cfg_launches"]
    assert torch.isfinite(fused["out"]).all() and torch.isfinite(fused["cfg_out"]).all()
    assert r <= 1e-2 and rc <= 1e-2          # the bound of the same comparison on SD1.5 above
