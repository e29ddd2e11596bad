"""AutoHDR after the VAE: ms per 1024^2 image of ldx_amd.AutoHDR.apply following VAEDecoderEngine.decode on the same stream (HIP events around the
apply alone), and of the route a caller needed before: device -> host copy, then the reference's chain in PIL + LittleCMS + numpy on the CPU (only
where PIL with LittleCMS is importable).  Synthetic VAE weights decode to an image that is mostly clamped, which flatters the table reads (few nodes,
always cached), so apply is also timed on its own on a smooth image and on uniformly random colours (every pixel in another cell of both 33^3 tables:
the worst case for the 2 x 287 496 B of tables in L2), next to one table read alone (ldx_hdr_table).  Writes profiles/hdr_probe.json.

    python profiles/hdr_probe.py [size=1024] [iters=500]
"""
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import ldx_amd as ldx  # noqa: E402

size = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
iters = int(sys.argv[2]) if len(sys.argv) > 2 else 500
assert torch.cuda.is_available(), "hdr_probe.py measures on the GPU; there is no CPU fallback"
res = {"size": size, "iters": iters, "device": torch.cuda.get_device_name(0)}


def timed(fn, n):
    """ms per call: n calls between two events, after two warm-up calls"""
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


fx = ldx.AutoHDR(device=0)
g = torch.Generator().manual_seed(7)
yy, xx = torch.meshgrid(torch.linspace(0, 1, size), torch.linspace(0, 1, size), indexing="ij")
smooth = torch.stack([xx, yy, 0.5 + 0.5 * torch.sin(6.28 * (xx + yy))], -1)[None].contiguous().cuda()
noise = torch.rand((1, size, size, 3), generator=g).cuda()

# ---- apply alone, on images that use the tables differently
for name, img in (("smooth", smooth), ("random_colours", noise)):
    res[f"apply_ms_{name}"] = timed(lambda: fx.apply(img), iters)
    u8 = (img * 255).to(torch.uint8)
    res[f"apply_u8_to_u8_ms_{name}"] = timed(lambda: fx.apply(u8, out_u8=True), iters)
    out = fx.apply(img, out_u8=True)
    q = np.clip(np.float32(255.0) * img[0].cpu().numpy(), 0, 255).astype(np.uint8)
    res[f"equals_host_{name}"] = bool(np.array_equal(out[0].cpu().numpy(), ldx.hdr.autohdr_host(q)))
    # one table read alone: bytes in, bytes out
    u = (img[0] * 255).to(torch.uint8).contiguous()
    o = torch.empty_like(u)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    res[f"table_read_ms_{name}"] = timed(lambda: ldx.lib.check(fx._lib.ldx_hdr_table(ldx.lib.ptr(u), size * 3, size, size, ldx.lib.ptr(fx._fwd), ldx.lib.ptr(o),
                                                                                        size * 3, st), "ldx_hdr_table"), iters)
# the bytes the two launches move per image (fp32 in, 3 B workspace out and in again, fp32 out), not counting the tables
res["bytes_per_image_fp32"] = size * size * (12 + 3 + 3 + 12)
res["stream_GBps_random_colours"] = res["bytes_per_image_fp32"] / (res["apply_ms_random_colours"] * 1e-3) / 1e9

# ---- after the VAE, on the same stream
vcfg = ldx.VAEConfig()
vae = ldx.VAEDecoderEngine(vcfg, ldx.weights.synth_state_dict(ldx.weights.vae_decoder_state_dict_spec(vcfg), seed=1, dtype=torch.float32), dtype="bf16")
z = torch.randn((1, 4, size // 8, size // 8), generator=g).cuda()
for _ in range(2):
    img = vae.decode(z)
    fx.apply(img)
torch.cuda.synchronize()
n, pairs = 10, []
for _ in range(n):
    e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
    e[0].record()
    img = vae.decode(z)
    e[1].record()
    out = fx.apply(img)
    e[2].record()
    pairs.append(e)
torch.cuda.synchronize()
res["vae_decode_ms"] = sum(e[0].elapsed_time(e[1]) for e in pairs) / n
res["apply_after_vae_ms"] = sum(e[1].elapsed_time(e[2]) for e in pairs) / n
res["vae_image_share_clamped"] = float(((img <= 0) | (img >= 1)).float().mean())

# ---- the host route: device -> host copy, then PIL + LittleCMS + numpy (the reference's chain: tensor2pil, two profileToProfile, the luminance chain on
# the L channel, ImageEnhance.Contrast and .Color, pil2tensor)
try:
    from PIL import Image, ImageCms, ImageEnhance
    srgb, lab_p = ImageCms.createProfile("sRGB"), ImageCms.createProfile("LAB")
except Exception as ex:                                                     # noqa: BLE001
    res["host_route"] = f"not measured: PIL with LittleCMS not importable ({type(ex).__name__})"
else:
    lut = ldx.hdr.luminance_lut()

    def host_route(dev):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        a = dev.cpu(); t1 = time.perf_counter()
        im = Image.fromarray(np.clip(255.0 * a.numpy().squeeze(), 0, 255).astype(np.uint8))
        big_l, ca, cb = ImageCms.profileToProfile(im, srgb, lab_p, outputMode="LAB").split()
        adj = Image.merge("LAB", (Image.fromarray(lut[np.array(big_l)]), ca, cb))
        rgb = ImageCms.profileToProfile(adj, lab_p, srgb, outputMode="RGB")
        rgb = ImageEnhance.Color(ImageEnhance.Contrast(rgb).enhance(1.1)).enhance(1.05)
        ret = torch.from_numpy(np.array(rgb).astype(np.float32) / 255.0).unsqueeze(0)
        return t1 - t0, time.perf_counter() - t1, ret

    host_route(noise)
    runs = [host_route(noise) for _ in range(3)]
    res["host_d2h_ms"] = 1e3 * min(r[0] for r in runs)
    res["host_pil_ms"] = 1e3 * min(r[1] for r in runs)
    dev = fx.apply(noise).cpu()
    res["host_route_bytes_differing_from_device"] = int((runs[0][2] != dev).sum())

path = os.path.join(ROOT, "profiles", "hdr_probe.json")
with open(path, "w") as f:
    json.dump(res, f, indent=1, sort_keys=True)
print(json.dumps(res, indent=1, sort_keys=True))
