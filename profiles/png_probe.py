"""SaveImage on the device: ms per 1024^2 image of ldx_amd.PNGEncoder (HIP events around the launches alone), of the same right after AutoHDR.apply on
the same stream, of its stages on their own (ldx_png_filter; ldx_zlib_deflate = the deflate and pack launches on the filtered stream), of the device ->
host copy of the finished file, and, as wall time on this machine's CPU, of what the reference does with the same bytes: Pillow's PNG writer at
compress_level=4.  Both file sizes; and Pillow decodes the device's file back to the input bytes.  Three contents: a smooth image, blurred noise, and
the VAE's decode of random latents (synthetic weights: mostly clamped, so nearly flat).  Writes profiles/png_probe.json (or the path given).

    python profiles/png_probe.py [size=1024] [iters=50] [out.json]
"""
import ctypes as C
import io
import json
import os
import sys
import time

import numpy as np
import torch
from PIL import Image, ImageFilter

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import ldx_amd as ldx  # noqa: E402

size = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
iters = int(sys.argv[2]) if len(sys.argv) > 2 else 50
path = sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "profiles", "png_probe.json")
assert torch.cuda.is_available(), "png_probe.py measures on the GPU; there is no CPU fallback"
res = {"size": size, "iters": iters, "device": torch.cuda.get_device_name(0), "cpu": "", "chunk_bytes": ldx.png.CHUNK}
try:
    with open("/proc/cpuinfo") as f:
        res["cpu"] = next(line.split(":", 1)[1].strip() for line in f if line.startswith("model name"))
except Exception:                                                           # noqa: BLE001
    pass


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


L = ldx.lib.load()
enc = ldx.PNGEncoder(device=0)
fx = ldx.AutoHDR(device=0)
g = torch.Generator().manual_seed(7)
rng = np.random.default_rng(7)
yy, xx = np.mgrid[0:size, 0:size]
images = {
    "smooth": np.stack([127 + 100 * np.sin(xx / 97.0 + c) * np.cos(yy / 61.0 - c) for c in range(3)], -1).astype(np.uint8),
    "blurred_noise": np.asarray(Image.fromarray(rng.integers(0, 256, (size, size, 3), dtype=np.uint8)).filter(ImageFilter.GaussianBlur(6))),
}
vcfg = ldx.VAEConfig()
vae = ldx.VAEDecoderEngine(vcfg, ldx.weights.synth_state_dict(ldx.weights.vae_decoder_state_dict_spec(vcfg), seed=1, dtype=torch.float32), dtype="bf16")
z = torch.randn((1, 4, size // 8, size // 8), generator=g).cuda()
decoded = vae.decode(z)                                                     # fp32 [1][H][W][3]
images["vae_random_latents"] = ldx.png.quantize(decoded[0].cpu().numpy())

n_stream = size * (1 + 3 * size)
stream = torch.empty(n_stream, dtype=torch.uint8, device="cuda")
zws = torch.empty(int(L.ldx_zlib_workspace_bytes(n_stream)), dtype=torch.uint8, device="cuda")
zout = torch.empty(int(L.ldx_zlib_bound_bytes(n_stream)), dtype=torch.uint8, device="cuda")
zlen = torch.zeros(1, dtype=torch.int32, device="cuda")
st = C.c_void_p(torch.cuda.current_stream().cuda_stream)

for name, img in images.items():
    r = res[name] = {}
    dev = torch.from_numpy(np.ascontiguousarray(img)).cuda()[None]
    dev_f = (dev.float() / 255 + 0.001).contiguous()
    r["encode_ms"] = timed(lambda: enc.encode_device(dev), iters)
    r["encode_fp32_in_ms"] = timed(lambda: enc.encode_device(dev_f), iters)
    r["filter_ms"] = timed(lambda: L.ldx_png_filter(None, ldx.lib.ptr(dev), size * 3, 1, size, size, ldx.lib.ptr(stream), None, st), iters)
    r["deflate_pack_ms"] = timed(lambda: L.ldx_zlib_deflate(ldx.lib.ptr(stream), n_stream, ldx.lib.ptr(zws), ldx.lib.ptr(zout), ldx.lib.ptr(zlen), st), iters)
    # right after AutoHDR on the same stream: events around each of the two
    pairs = []
    for i in range(12):
        e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        e[0].record()
        hdr_out = fx.apply(dev_f, out_u8=True)
        e[1].record()
        enc.encode_device(hdr_out)
        e[2].record()
        if i >= 2:
            pairs.append(e)
    torch.cuda.synchronize()
    r["autohdr_apply_ms"] = sum(e[0].elapsed_time(e[1]) for e in pairs) / len(pairs)
    r["encode_after_autohdr_ms"] = sum(e[1].elapsed_time(e[2]) for e in pairs) / len(pairs)
    # the file, its copy to the host, and Pillow's reading of it
    out, lens = enc.encode_device(dev)
    torch.cuda.synchronize()
    n = int(lens.cpu()[0])
    copies = []
    for _ in range(5):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        data = out[0, :n].cpu()
        copies.append(time.perf_counter() - t0)
    r["file_d2h_ms"] = 1e3 * min(copies)
    data = data.numpy().tobytes()
    r["file_bytes"] = n
    with Image.open(io.BytesIO(data)) as im:
        r["pillow_decodes_to_input"] = bool(np.array_equal(np.asarray(im), img))
    # the reference's route: Pillow's writer at compress_level=4 on this machine's CPU (after the copy of the raw image, timed as well)
    saves = []
    for _ in range(3):
        buf = io.BytesIO(); t0 = time.perf_counter()
        Image.fromarray(img).save(buf, "PNG", compress_level=4)
        saves.append(time.perf_counter() - t0)
    r["pillow_level4_ms"] = 1e3 * min(saves)
    r["pillow_level4_bytes"] = len(buf.getvalue())
    r["size_ratio"] = n / len(buf.getvalue())
    torch.cuda.synchronize(); t0 = time.perf_counter()
    dev.cpu()
    r["raw_image_d2h_ms"] = 1e3 * (time.perf_counter() - t0)
    r["dominant_stage"] = "deflate + pack" if r["deflate_pack_ms"] > r["filter_ms"] else "filter"

with open(path, "w") as f:
    json.dump(res, f, indent=1, sort_keys=True)
print(json.dumps(res, indent=1, sort_keys=True))
