"""SAM mask decoder on the device: ms per call of ldx_amd.SAMMaskDecoderEngine at ViT-B sizes (grid 64^2, width 256, image 1024^2) with synthetic weights,
beside the torch statement of the same decoder + post-processing (sam_decoder_host + F.interpolate chain) in fp32 on the same GPU, in the same process, eager
and through torch.cuda.graph.  HIP events around 50 calls after a warm-up, the mean per call.  Measured: set_image; predict at P = 1 and P = 8 (eager launches
and graph replay); post-processing of one 1024^2 mask; SAMDetector.detect with 1 and 3 segments right after VAEDecoderEngine.decode (image encoder included);
the per-launch split of predict (ldx_profile: an event pair around every launch).  Writes profiles/samdec_probe.json (or the path given).

    python profiles/samdec_probe.py [iters=50] [out.json]
"""
import json
import os
import sys
import types

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import ldx_amd as ldx  # noqa: E402

iters = int(sys.argv[1]) if len(sys.argv) > 1 else 50
path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "samdec_probe.json")
assert torch.cuda.is_available(), "samdec_probe.py measures on the GPU; there is no CPU fallback"


def timed(fn, n=iters, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / n


cfg = ldx.SAMDecoderConfig.vit_b()
sd = ldx.weights.sam_decoder_synth_state_dict(cfg, seed=9)
emb = torch.randn((256, 64, 64), generator=torch.Generator().manual_seed(1)).cuda()
BOXES = [[100.0, 120.0, 500.0, 640.0], [0.0, 0.0, 1023.0, 1023.0], [600.0, 300.0, 900.0, 700.0], [10.0, 800.0, 400.0, 1000.0],
         [300.0, 30.0, 700.0, 400.0], [50.0, 500.0, 350.0, 900.0], [512.0, 512.0, 1000.0, 1000.0], [200.0, 200.0, 800.0, 800.0]]


def prompts(P):
    boxes = BOXES[:P]
    return [[[(b[0] + b[2]) / 2, (b[1] + b[3]) / 2]] for b in boxes], [[1]] * P, boxes


res = {"device": torch.cuda.get_device_name(0), "iters": iters, "sizes": {"image": 1024, "grid": 64, "hidden": 256, "heads": 8, "mlp": 2048}}
eager, graph = ldx.SAMMaskDecoderEngine(cfg, sd), ldx.SAMMaskDecoderEngine(cfg, sd, graph=True)
res["set_image_ms"] = timed(lambda: eager.set_image(emb))
graph.set_image(emb)
sd_dev = {k: v.cuda() for k, v in sd.items()}
for P in (1, 8):
    pts, lab, box = prompts(P)
    r = {"engine_eager_ms": timed(lambda: eager.predict(pts, lab, box, None)), "engine_graph_ms": timed(lambda: graph.predict(pts, lab, box, None)),
         "launches": eager.plan_info()["launches"]}
    # the decoder alone, prompts already on the device (what the engine's figures above include: the host -> device copy of the prompts)
    dp, dl, db = torch.tensor(pts).cuda(), torch.tensor(lab).cuda(), torch.tensor(box).cuda()

    def statement():
        low, iou = ldx.sam.sam_decoder_host(sd_dev, emb, dp, dl, db, torch.float32)
        return low, iou

    r["torch_eager_ms"] = timed(statement)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        for _ in range(3):
            statement()
    torch.cuda.current_stream().wait_stream(stream)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = statement()
    r["torch_graph_ms"] = timed(g.replay)
    low_e, _ = eager.predict(pts, lab, box, None)
    r["engine_vs_torch_rel_l2"] = float((low_e.double() - out[0][:, 1:].double()).norm() / out[0][:, 1:].double().norm())
    eager.profile(True)
    for _ in range(10):
        eager.predict(pts, lab, box, None)
    rep = eager.profile_report()
    eager.profile(False)
    r["per_launch_us"] = {k: round(1000.0 * v["ms"] / 10, 2) for k, v in sorted(rep.items(), key=lambda kv: -kv[1]["ms"])}
    res[f"predict_P{P}"] = r

low = torch.randn((1, 256, 256), generator=torch.Generator().manual_seed(2)).cuda()
res["postprocess_1024_ms"] = timed(lambda: eager.masks(low, (1024, 1024)))


def torch_post():
    m = F.interpolate(low[None], (1024, 1024), mode="bilinear", align_corners=False)
    return F.interpolate(m[..., :1024, :1024], (1024, 1024), mode="bilinear", align_corners=False) > 0


res["torch_postprocess_1024_ms"] = timed(torch_post)

# SAMDetector.detect right after the VAE's decode: image encoder + decoder + selection + post-processing
ecfg, vcfg = ldx.SAMConfig.vit_b(), ldx.VAEConfig()
enc = ldx.SAMImageEncoderEngine(ecfg, ldx.weights.sam_synth_state_dict(ecfg, seed=5), graph=True)
vae = ldx.VAEEngine(vcfg, ldx.weights.synth_state_dict(ldx.weights.vae_state_dict_spec(vcfg), seed=4321, dtype=torch.float32), device=0, dtype="bf16")
det = ldx.SAMDetector(enc, graph)
z = torch.randn((1, 4, 128, 128), generator=torch.Generator().manual_seed(3)).cuda()
img = ((vae.decode(z) + 1) / 2).clamp(0, 1)          # fp32 [1, 1024, 1024, 3] on the device, as the pipeline holds it
res["encoder_set_image_ms"] = timed(lambda: enc.set_image(img), n=max(5, iters // 5))
for nseg in (1, 3):
    segs = ((1024, 1024), [types.SimpleNamespace(bbox=[int(v) for v in b]) for b in BOXES[:nseg]])
    res[f"detect_{nseg}_segments_ms"] = timed(lambda: det.detect(img, segs, -1.0, 10), n=max(5, iters // 5))

with open(path, "w") as f:
    json.dump(res, f, indent=1)
print(json.dumps(res, indent=1))
