"""Golden capture for the TAESD latent previews: writes tests/golden/taesd.npz and tests/golden/taesd.META.txt.  Build container only (needs the reference,
safetensors and Pillow; see oracle/ref_capture.py for how the reference is entered).

  weights        seeded synthetic tensors under Decoder2's own keys (fixture_state_dict below, also what the tests load: 1.2 M parameters are regenerated, not
                 stored; the file keeps the key list, the shapes and one fp64 sum per tensor).  Plain fan-in scaling drives the decoder's output far outside
                 [0, 1], where every preview byte is 0 or 255, so the output conv is scaled down (19.weight * last_scale, 19.bias = 0.5 + the seeded bias) until at
                 least 90 % of the reference's fp32 decoder(x) values lie in (0.02, 0.98) for EVERY fixture input; the share reached is written to META.
  per input      the reference's TAESD.decode output and the bytes taesd_preview hands to app.update_image (through the reference's own functions, the
                 decoder loaded from a temporary safetensors file), and the distance of two CPU restatements to them.  `restatement`: bf16-rounded weights,
                 activations rounded to bf16 after every conv (and after a Block's sum), fp32 accumulation, fp32 output: every activation 16-bit.
                 `engine_restatement`: what the engine computes, up to the order of its sums: the skip stream stays fp32 (conv.4's fp32 sum + the fp32
                 stream, no rounding in between), the convs multiply bf16 copies.  The GPU tests take their bounds from those distances: decode from both,
                 the byte counts from the first.
  keys           the key list and shapes are the reference decoder's own state_dict(), not this project's spec (tests/test_taesd_cpu.py compares the two).

    python tests/tools/capture_taesd.py
"""
import os
import sys
import tempfile

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
GOLDEN = os.path.join(REPO, "tests", "golden")
SEED = 4321
MEASURED = "---- measured on the GPU"
# (name, latent shape, flux): a base case, odd sizes with batch 2, one that crosses the kernel's tile edges at all four levels, the smallest possible latent,
# and one 16-channel latent for the Flux branch of taesd_preview
CASES = (("base", (1, 4, 8, 12), False), ("odd", (2, 4, 5, 7), False), ("edges", (1, 4, 33, 17), False), ("one", (1, 4, 1, 1), False),
         ("flux", (1, 16, 6, 9), True))


def fixture_latent(name):
    """The seeded latent of a case: N(0, 2^2), the spread of a sampler's x half-way through a run (the Clamp layer sees its tanh bend)."""
    i = [c[0] for c in CASES].index(name)
    g = torch.Generator().manual_seed(SEED + 17 * i)
    return 2.0 * torch.randn(CASES[i][1], generator=g, dtype=torch.float32)


def fixture_state_dict(last_scale):
    """fp32 state dict under Decoder2's keys: weights.synth_state_dict with the output conv scaled as described above."""
    sys.path.insert(0, REPO)
    import ldx_amd as ldx
    sd = ldx.weights.synth_state_dict(ldx.weights.taesd_decoder_state_dict_spec(), seed=SEED, dtype=torch.float32)
    sd["19.weight"] = sd["19.weight"] * float(last_scale)
    sd["19.bias"] = sd["19.bias"] + 0.5
    return sd


def bf16(t):
    return t.to(torch.bfloat16).float()


def restatement(sd, x):
    """Decoder2 + TAESD.decode with the engine's number formats, on the CPU: weights and every stored activation rounded to bf16, sums in fp32."""
    F = torch.nn.functional
    w = {k: bf16(v) if k.endswith("weight") else v for k, v in sd.items()}

    def conv(h, pre, bias=True):
        return F.conv2d(h, w[pre + ".weight"], w[pre + ".bias"] if bias else None, padding=1)

    def block(h, i):
        t = bf16(F.relu(conv(h, f"{i}.conv.0")))
        t = bf16(F.relu(conv(t, f"{i}.conv.2")))
        return bf16(F.relu(bf16(conv(t, f"{i}.conv.4")) + h))

    h = bf16(torch.tanh(x / 3) * 3)
    h = bf16(F.relu(conv(h, "1")))
    for i in (3, 4, 5):
        h = block(h, i)
    for up, blocks in ((7, (8, 9, 10)), (12, (13, 14, 15)), (17, (18,))):
        h = bf16(conv(F.interpolate(h, scale_factor=2, mode="nearest"), str(up), bias=False))
        for i in blocks:
            h = block(h, i)
    return conv(h, "19").sub(0.5).mul(2)


def engine_restatement(sd, x):
    """The engine's arithmetic (engine_taesd.cpp) on the CPU: bf16 weights, every conv input a bf16 copy, the skip stream of a level in fp32."""
    F = torch.nn.functional
    w = {k: bf16(v) if k.endswith("weight") else v for k, v in sd.items()}

    def conv(h, pre, bias=True):
        return F.conv2d(h, w[pre + ".weight"], w[pre + ".bias"] if bias else None, padding=1)

    def block(h, i):
        t = bf16(F.relu(conv(bf16(h), f"{i}.conv.0")))
        t = bf16(F.relu(conv(t, f"{i}.conv.2")))
        return F.relu(conv(t, f"{i}.conv.4") + h)

    h = F.relu(conv(bf16(torch.tanh(x / 3) * 3), "1"))
    for i in (3, 4, 5):
        h = block(h, i)
    for up, blocks in ((7, (8, 9, 10)), (12, (13, 14, 15)), (17, (18,))):
        h = conv(F.interpolate(bf16(h), scale_factor=2, mode="nearest"), str(up), bias=False)
        for i in blocks:
            h = block(h, i)
    return conv(bf16(h), "19").sub(0.5).mul(2)


def quantise(decoded, flux):
    """taesd_preview's arithmetic (taesd.py:291-304) on a decoded batch [B,3,H,W] -> uint8 [B,H,W,3], in torch fp32."""
    d = decoded
    if flux:
        d = d[:, [2, 1, 0]].clamp(-1, 1)
    v = (d + 1.0) / 2.0 * 255.0
    return v.clamp(0, 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous()


def share_gt2(a, b):
    return float((a.to(torch.int16) - b.to(torch.int16)).abs().gt(2).float().mean())


def main():
    sys.path.insert(0, os.path.join(REPO, "oracle"))
    import ref_capture
    ref_capture.enter_reference()
    from safetensors.torch import save_file
    from src.AutoEncoders import taesd as T
    from src.user import app_instance
    torch.set_num_threads(8)
    tmp = tempfile.mkdtemp(prefix="ldx_taesd_")
    path = os.path.join(tmp, "taesd_decoder.safetensors")

    def reference(last_scale):
        sd = fixture_state_dict(last_scale)
        save_file({k: v.contiguous() for k, v in sd.items()}, path)
        return sd, T.TAESD(decoder_path=path)

    # the condition on the fixture: shrink the output conv until every input's decoder(x) lies inside (0.02, 0.98) for >= 90 % of its values
    last_scale, inside = 1.0, {}
    while True:
        sd, model = reference(last_scale)
        with torch.no_grad():
            for name, _, _ in CASES:
                y = model.taesd_decoder(fixture_latent(name)[:, :4])
                inside[name] = float(((y > 0.02) & (y < 0.98)).float().mean())
        if min(inside.values()) >= 0.9:
            break
        last_scale *= 0.7
        assert last_scale > 1e-3, inside
    ref_sd = model.taesd_decoder.state_dict()          # the reference's own keys and shapes go into the fixture
    assert all(torch.equal(ref_sd[k], v) for k, v in sd.items()) and len(ref_sd) == len(sd)

    g = {"seed": np.int64(SEED), "last_scale": np.float64(last_scale), "keys": np.array(list(ref_sd)),
         "shapes": np.array([list(v.shape) + [0] * (4 - v.dim()) for v in ref_sd.values()]),
         "sums": np.array([float(v.double().sum()) for v in sd.values()]), "cases": np.array([c[0] for c in CASES])}
    meta = [f"taesd.npz: tests/tools/capture_taesd.py, seed {SEED}, torch {torch.__version__}", f"last_scale (19.weight) = {last_scale:.6g}; 19.bias = 0.5 + seeded N(0, 0.02)",
            "share of the reference's fp32 decoder(x) inside (0.02, 0.98) per input (the fixture's condition: >= 0.9):"]
    meta += [f"  {n}: {inside[n]:.4f}" for n, _, _ in CASES]
    meta.append("CPU restatement (bf16 weights / activations, fp32 sums) against the reference: rel-L2 of decode, share of preview bytes off by more than 2 codes:")

    # taesd_preview builds its own TAESD() from a path that does not exist here: it gets the temporary file, and app.update_image is recorded
    shown = []
    orig_taesd, orig_update = T.TAESD, app_instance.app.update_image
    T.TAESD = lambda *a, **k: orig_taesd(decoder_path=path)
    app_instance.app.update_image = lambda images: shown.append(np.stack([np.asarray(im) for im in images]))
    app_instance.app.previewer_var.set(True)
    try:
        with torch.no_grad():
            for name, _, flux in CASES:
                x = fixture_latent(name)
                dec = model.decode(x[:, :4])
                del shown[:]
                T.taesd_preview(x, flux)
                ref_bytes = torch.from_numpy(shown[0])
                assert torch.equal(ref_bytes, quantise(dec, flux)), f"{name}: the tensor rule restated here is not the reference's"
                rs = restatement(sd, x[:, :4])
                rel = float((rs - dec).norm() / dec.norm())
                off = share_gt2(quantise(rs, flux), ref_bytes)
                g[f"x_{name}"], g[f"decode_{name}"], g[f"bytes_{name}"] = x.numpy(), dec.numpy(), ref_bytes.numpy()
                g[f"restate_rel_{name}"], g[f"restate_gt2_{name}"] = np.float64(rel), np.float64(off)
                es = engine_restatement(sd, x[:, :4])
                erel = float((es - dec).norm() / dec.norm())
                eoff = share_gt2(quantise(es, flux), ref_bytes)
                g[f"engine_rel_{name}"], g[f"engine_gt2_{name}"] = np.float64(erel), np.float64(eoff)
                meta.append(f"  {name} {tuple(x.shape)}{' flux' if flux else ''}: rel-L2 {rel:.3e}, bytes off by > 2: {off:.3e}; in the engine's order (fp32 skip stream): "
                            f"rel-L2 {erel:.3e}, bytes off by > 2: {eoff:.3e}")
                print(meta[-1])
    finally:
        T.TAESD, app_instance.app.update_image = orig_taesd, orig_update
        app_instance.app.previewer_var.set(False)
        os.unlink(path)
        os.rmdir(tmp)
    np.savez_compressed(os.path.join(GOLDEN, "taesd.npz"), **g)
    meta_path, measured = os.path.join(GOLDEN, "taesd.META.txt"), ""
    if os.path.exists(meta_path):                  # what was measured on the GPU is written by hand below MEASURED and survives a re-capture
        old = open(meta_path).read()
        measured = old[old.index(MEASURED):] if MEASURED in old else ""
    with open(meta_path, "w") as f:
        f.write("\n".join(meta) + "\n" + measured)
    print("\n".join(meta[:8]))
    print("wrote", os.path.join(GOLDEN, "taesd.npz"), os.path.getsize(os.path.join(GOLDEN, "taesd.npz")), "bytes")


if __name__ == "__main__":
    main()
