"""SAM image encoder on the device: ViT-B at 1024^2 with synthetic weights (weights.sam_synth_state_dict).  HIP events around `iters` calls after a warm-up:
ms per SAMImageEncoderEngine.encode, eager and as a replayed hipGraph; the split of one eager encode between global attention, window attention, the linears
and the rest (ldx_profile: events around every launch); the attention kernel's rate at N = 4096; ms of set_image from a 1024^2 fp32 image right after
VAEDecoderEngine.decode on the same stream; and, in the same process, the torch statement of the same network (sam.sam_encoder_host, what segment_anything
computes) on the GPU in fp32, the reference's type, and in bf16 autocast.  Writes profiles/sam_probe.json (or the path given).

    python profiles/sam_probe.py [iters=50] [out.json]
"""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import ldx_amd as ldx  # noqa: E402

iters = int(sys.argv[1]) if len(sys.argv) > 1 else 50
path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "sam_probe.json")
assert torch.cuda.is_available(), "sam_probe.py measures on the GPU; there is no CPU fallback"
res = {"iters": iters, "device": torch.cuda.get_device_name(0), "config": "ViT-B, image 1024, synthetic weights", "dtype": "bf16"}


def timed(fn, n, warm=3):
    """ms per call: n calls between two events, after `warm` warm-up calls"""
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


cfg = ldx.SAMConfig.vit_b()
sd = ldx.weights.sam_synth_state_dict(cfg, seed=11)
g = torch.Generator().manual_seed(11)
x = torch.randn(1, 3, 1024, 1024, generator=g)
x[:, :, 768:] = 0.0
xd = x.cuda()

eng = ldx.SAMImageEncoderEngine(cfg, sd, device=0, dtype="bf16")
res["encode_eager_ms"] = timed(lambda: eng.encode(xd), iters)
info = eng.plan_info()
res["launches"], res["flops"] = info["launches"], info["flops"]
res["encode_eager_tflops"] = info["flops"] / res["encode_eager_ms"] / 1e9

# the split of an eager encode: events around every launch (they serialise the launches, so the parts add up to more than an unprofiled encode)
eng.profile(True)
for _ in range(5):
    eng.encode(xd)
torch.cuda.synchronize()
rep = eng.profile_report()
eng.profile(False)
split = {"global_attention": 0.0, "window_attention": 0.0, "relpos": 0.0, "linears_and_convs": 0.0, "other": 0.0}
for k, v in rep.items():
    ms = v["ms"] / 5
    if "sam_attn_kernel" in k:
        split["global_attention" if "global" in k else "window_attention"] += ms
        if "global" in k:
            res["attention_n4096_tflops"] = v["flops"] / v["ms"] / 1e9
            res["attention_n4096_ms_per_block"] = v["ms"] / v["count"]
        else:
            res["attention_n196_tflops"] = v["flops"] / v["ms"] / 1e9
    elif "sam_relpos" in k:
        split["relpos"] += ms
    elif k.startswith("gemm_kernel"):
        split["linears_and_convs"] += ms
    else:
        split["other"] += ms
res["profiled_split_ms"] = split
res["profiled_total_ms"] = sum(split.values())

geng = ldx.SAMImageEncoderEngine(cfg, sd, device=0, dtype="bf16", graph=True)
res["encode_graph_ms"] = timed(lambda: geng.encode(xd), iters, warm=4)
res["graph_stats"] = list(geng.graph_stats())
res["graph_equals_eager"] = bool(torch.equal(geng.encode(xd), eng.encode(xd)))

# set_image right after the VAE's decode on the same stream
vcfg = ldx.VAEConfig()
vae = ldx.VAEDecoderEngine(vcfg, ldx.weights.synth_state_dict(ldx.weights.vae_decoder_state_dict_spec(vcfg), seed=1, dtype=torch.float32), dtype="bf16")
z = torch.randn((1, 4, 128, 128), generator=g).cuda()
pairs = []
for i in range(12):
    e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
    e[0].record()
    img = vae.decode(z)                                                   # fp32 [1][1024][1024][3]
    e[1].record()
    eng.set_image(img)
    e[2].record()
    if i >= 2:
        pairs.append(e)
torch.cuda.synchronize()
res["vae_decode_ms"] = sum(e[0].elapsed_time(e[1]) for e in pairs) / len(pairs)
res["set_image_after_vae_ms"] = sum(e[1].elapsed_time(e[2]) for e in pairs) / len(pairs)
res["preprocess_ms"] = timed(lambda: eng.preprocess(img), 20)

# the torch statement of the network on the same GPU: fp32 (what the reference runs) and bf16 autocast
sdd = {k: v.cuda() for k, v in sd.items()}
n_torch = max(5, iters // 10)
res["torch_fp32_ms"] = timed(lambda: ldx.sam.sam_encoder_host(sdd, xd), n_torch, warm=2)
ref = ldx.sam.sam_encoder_host(sdd, xd)
out = eng.encode(xd)
res["engine_vs_torch_fp32_rel_l2"] = float((out - ref).norm() / ref.norm())

def torch_bf16():
    with torch.autocast("cuda", dtype=torch.bfloat16):
        return ldx.sam.sam_encoder_host(sdd, xd)


res["torch_bf16_ms"] = timed(torch_bf16, n_torch, warm=2)
res["torch_bf16_vs_torch_fp32_rel_l2"] = float((torch_bf16().float() - ref).norm() / ref.norm())

with open(path, "w") as f:
    json.dump(res, f, indent=1, sort_keys=True)
print(json.dumps(res, indent=1, sort_keys=True))
