"""Host side of the TAESD previews, no GPU: the decoder's state-dict spec against the fixture's key list (tests/golden/taesd.npz, written by
tests/tools/capture_taesd.py from the reference's own Decoder2), LatentPreviewer's cadence and delivery order with a stand-in engine, and the preview hook of the
five sampler loops over a stand-in model: with preview=None nothing changes, a callback sees exactly the iterations 0, 5, 10, ... and the x of those iterations."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import capture_taesd as CT  # noqa: E402


@pytest.fixture(scope="module")
def fx(golden_dir):
    return np.load(os.path.join(golden_dir, "taesd.npz"))


def test_spec_is_the_reference_decoders(ldx, fx):
    spec = ldx.weights.taesd_decoder_state_dict_spec(ldx.TAESDConfig())
    assert [k for k, _ in spec] == [str(k) for k in fx["keys"]]
    assert [list(s) + [0] * (4 - len(s)) for _, s in spec] == fx["shapes"].tolist()
    assert len(spec) == 67 and ldx.weights.param_count(spec) == 1222531


def test_fixture_weights_regenerate(fx):
    """The fixture stores no weights (1.2 M parameters): the tests rebuild them from the seed, and the stored per-tensor sums say they are the captured ones."""
    assert int(fx["seed"]) == CT.SEED
    sd = CT.fixture_state_dict(float(fx["last_scale"]))
    assert list(sd) == [str(k) for k in fx["keys"]]
    np.testing.assert_allclose([float(v.double().sum()) for v in sd.values()], fx["sums"], rtol=0, atol=1e-9)
    for name, shape, _ in CT.CASES:
        assert np.array_equal(CT.fixture_latent(name).numpy(), fx[f"x_{name}"]) and fx[f"x_{name}"].shape == shape


def test_fixture_condition_and_quantisation_rule(fx):
    """>= 90 % of the reference's decoder(x) inside (0.02, 0.98), and the reference's bytes are the quantisation rule applied to its own decode output."""
    for name, _, flux in CT.CASES:
        dec = torch.from_numpy(fx[f"decode_{name}"])
        y = dec / 2 + 0.5
        assert float(((y > 0.02) & (y < 0.98)).float().mean()) >= 0.9, name
        assert torch.equal(CT.quantise(dec, flux), torch.from_numpy(fx[f"bytes_{name}"])), name
        assert 0 < float(fx[f"restate_rel_{name}"]) < 2e-2 and 0 <= float(fx[f"restate_gt2_{name}"]) < 1e-3


class _StandInEngine:
    """preview(x, flux) on the host: bytes that identify the call"""

    def __init__(self):
        self.calls = []

    def preview(self, x, flux=False):
        self.calls.append(bool(flux))
        return torch.full((x.shape[0], 8 * x.shape[2], 8 * x.shape[3], 3), int(x.flatten()[0]) % 256, dtype=torch.uint8)


def test_latent_previewer_delivers_in_order(ldx):
    eng, got = _StandInEngine(), []
    pv = ldx.LatentPreviewer(eng, lambda step, images: got.append((step, images.clone())), flux=True)
    for step in (0, 5, 10):
        pv(step, torch.full((2, 4, 3, 5), float(step + 1)))
        assert [s for s, _ in got] == [s for s in (0, 5, 10) if s < step]          # a finished image is handed over at the NEXT call
    pv.flush()
    assert [s for s, _ in got] == [0, 5, 10] and eng.calls == [True] * 3
    for step, images in got:
        assert images.shape == (2, 24, 40, 3) and images.dtype == torch.uint8 and int(images.unique()) == step + 1
    pv.flush()
    assert len(got) == 3


class _StandInModel:
    """model(x, sigma) -> (uncond, cond): two fixed linear functions of x"""
    cfg = 3.0

    def __call__(self, x, sigma):
        return 0.5 * x, 0.6 * x + 0.01


def _host_step(kind, x, du, dc, cfg, c0, c1, denoised_out=None):
    """ldx_sampler_step's four rules (csrc/ldx_kernels.h StepArgs) in torch, for the loops to run on the host"""
    cfg, c0, c1 = float(cfg), float(c0), float(c1)
    d = torch.lerp(du, dc, cfg)
    if kind == 0:
        x.add_((x - d) / c0 * c1)
    elif kind == 1:
        x.copy_(c0 * x - c1 * d)
    elif kind == 2:
        denoised_out.copy_(d)
    else:
        x.add_(du * c0)


SAMPLERS = ("sample_euler", "sample_dpmpp_2m_cfgpp", "sample_euler_ancestral_cfgpp", "sample_euler_cfgpp", "sample_dpmpp_sde_cfgpp")


@pytest.mark.parametrize("name", SAMPLERS)
def test_preview_hook_of_the_sampler_loops(ldx, monkeypatch, name):
    S = ldx.sampling
    monkeypatch.setattr(S, "_step", _host_step)
    monkeypatch.setattr(S, "_bilinear", lambda t, size: torch.nn.functional.interpolate(t, size=size, mode="bilinear", align_corners=False))
    fn = getattr(S, name)
    sigmas = S.sigmas_for(S.ModelSamplingDiscrete(), "karras", 12)
    x0 = torch.randn(1, 4, 16, 16, generator=torch.Generator().manual_seed(3))

    def run(**kw):
        torch.manual_seed(11)                      # the ancestral loops draw their default noise from the global generator
        extra = {"seed": 5} if name == "sample_dpmpp_sde_cfgpp" else {}
        return fn(_StandInModel(), x0.clone(), sigmas, **extra, **kw)

    plain = run()
    every5, every1 = [], []
    assert torch.equal(run(preview=lambda i, x: every5.append((i, x.clone()))), plain)
    assert torch.equal(run(preview=lambda i, x: every1.append((i, x.clone())), preview_every=1), plain)
    assert [i for i, _ in every1] == list(range(12)) and [i for i, _ in every5] == [0, 5, 10]
    for i, x in every5:
        assert torch.equal(x, every1[i][1])
    assert torch.equal(every1[-1][1], plain)       # the last iteration's x is the result
    assert not torch.equal(every5[0][1], every5[1][1])
