"""ADetailer on the device: ms per stage and per segment of ldx_amd.Detailer.detail on one 1024^2 image with three segments at the pipeline's settings
(guide_size 512, max_size 768, 20 steps, cfg 6.5, karras, denoise 0.5, feather 5; SD1.5 UNet and VAE with synthetic weights, bf16).  HIP events are
recorded on the stream between the stages (Detailer.timings), so a stage's time is device time plus the host's enqueue gaps inside it; one warm-up
call plans and captures every shape, then the median over the timed calls is taken.  Stages: mask (upload + ldx_detail_blur_mask), crop_encode
(ldx_detail_crop_quantize, LANCZOS up, to float, vae.encode), sample (KSampler.sample: 20 steps x 2 CFG branches), decode (vae.decode), paste
(quantise, LANCZOS down, to float, ldx_detail_paste).  Writes profiles/detailer_probe.json (or the path given).

    python profiles/detailer_probe.py [iters=5] [out.json]
"""
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import ldx_amd as ldx  # noqa: E402

iters = int(sys.argv[1]) if len(sys.argv) > 1 else 5
path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "detailer_probe.json")
assert torch.cuda.is_available(), "detailer_probe.py measures on the GPU; there is no CPU fallback"

SIZE = 1024
SETTINGS = dict(guide_size=512, guide_size_for=False, max_size=768, seed=1, steps=20, cfg=6.5, sampler_name="dpmpp_2m_cfgpp", scheduler="karras", denoise=0.5,
                feather=5, noise_mask=True, force_inpaint=True, wildcard="", cycle=1, inpaint_model=False, noise_mask_feather=20)
# bbox, crop_factor: crops 400 x 560, 512 x 512 and 600 x 400, sampled at 512 x 716, 512 x 512 and 768 x 512 (latents 64 x 89, 64 x 64, 96 x 64)
BOXES = [([100, 100, 300, 380], 2.0), ([600, 200, 856, 456], 2.0), ([500, 640, 800, 840], 2.0)]
STAGES = ("mask", "crop_encode", "sample", "decode", "paste")

ucfg, vcfg = ldx.UNetConfig.sd15(), ldx.VAEConfig()
unet = ldx.UNetEngine(ucfg, ldx.weights.synth_state_dict(ldx.weights.unet_state_dict_spec(ucfg), seed=1234), device=0, dtype="bf16")
vae = ldx.VAEEngine(vcfg, ldx.weights.synth_state_dict(ldx.weights.vae_state_dict_spec(vcfg), seed=4321, dtype=torch.float32), device=0, dtype="bf16")
det = ldx.Detailer(unet, vae)

yy, xx = np.mgrid[0:SIZE, 0:SIZE]
img = np.stack([0.5 + 0.4 * np.sin(xx / 97.0 + c) * np.cos(yy / 61.0 - c) for c in range(3)], -1).astype(np.float32)[None]
items = []
for bbox, factor in BOXES:
    x1, y1, x2, y2 = ldx.detailer.make_crop_region(SIZE, SIZE, bbox, factor)
    mask = np.zeros((y2 - y1, x2 - x1), np.float32)
    mask[bbox[1] - y1:bbox[3] - y1, bbox[0] - x1:bbox[2] - x1] = 1.0
    items.append(ldx.SEG(None, mask, 1.0, [x1, y1, x2, y2], bbox, "seg", None))
segs = ((SIZE, SIZE), items)
g = torch.Generator().manual_seed(7)
P, N = torch.randn([1, 77, ucfg.context_dim], generator=g), torch.randn([1, 77, ucfg.context_dim], generator=g)
dev = torch.from_numpy(img).cuda()

res = {"size": SIZE, "iters": iters, "device": torch.cuda.get_device_name(0), "dtype": "bf16", "settings": {k: v for k, v in SETTINGS.items()}, "segments": []}
for s in items:
    w, h = s.crop_region[2] - s.crop_region[0], s.crop_region[3] - s.crop_region[1]
    nw, nh = ldx.detailer.detail_size(w, h, SETTINGS["guide_size"], SETTINGS["max_size"])
    res["segments"].append({"crop_wh": [w, h], "sample_wh": [nw, nh], "latent_hw": [nh // 8, nw // 8]})

det.detail(dev, segs, P, N, **SETTINGS)                      # warm-up: plans, graph captures and resample tables of every shape
torch.cuda.synchronize()
per_stage = [{k: [] for k in STAGES} for _ in items]
totals, walls = [], []
for _ in range(iters):
    det.timings = {}
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    e0.record()
    det.detail(dev, segs, P, N, **SETTINGS)
    e1.record()
    torch.cuda.synchronize()
    walls.append(1e3 * (time.perf_counter() - t0))
    totals.append(e0.elapsed_time(e1))
    ev = det.timings
    for i in range(len(items)):
        prev = ev["start"][i]
        for k in STAGES:
            per_stage[i][k].append(prev.elapsed_time(ev[k][i]))
            prev = ev[k][i]
det.timings = None
for i, seg in enumerate(res["segments"]):
    seg["ms"] = {k: statistics.median(v) for k, v in per_stage[i].items()}
    seg["ms_min_max"] = {k: [min(v), max(v)] for k, v in per_stage[i].items()}
    seg["ms_per_unet_step"] = seg["ms"]["sample"] / SETTINGS["steps"]
    seg["sample_share"] = seg["ms"]["sample"] / sum(seg["ms"].values())
res["detail_ms"] = statistics.median(totals)
res["detail_ms_min_max"] = [min(totals), max(totals)]
res["detail_wall_ms"] = statistics.median(walls)
res["stage_ms_sum"] = {k: sum(seg["ms"][k] for seg in res["segments"]) for k in STAGES}
res["dominant_stage"] = max(res["stage_ms_sum"], key=res["stage_ms_sum"].get)

with open(path, "w") as f:
    json.dump(res, f, indent=1, sort_keys=True)
print(json.dumps(res, indent=1, sort_keys=True))
