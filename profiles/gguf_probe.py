"""Time from Q8_0 blocks in host memory to a finalized Flux engine, by three routes (bf16 engine, synthetic blocks at flux-dev shapes with finite scales
around 1e-3; every 2-D weight Q8_0, every 1-D tensor F32, as in the reference's flux1-dev-Q8_0.gguf):

  (a) dense     GGUFTensor.dequantize() of everything on the host into a dense dict, then FluxEngine(cfg, dense): the only route before ldx_load_tensor_q8_0
  (b) host      FluxEngine(cfg, tensors, device_weights=False): the C++ host expansion (csrc/weight_convert.h), host packers
  (c) device    FluxEngine(cfg, tensors, device_weights=True): raw blocks copied to the device tensor by tensor, csrc/q8.hip, device packers

Each is wall time with the device synchronised in front and behind.  Inside (c) two parts are measured again on their own, over the same tensors: the
host-to-device copies of the raw blocks (wall time, synchronised) and the q8.hip kernel (HIP events around ldx_op_dequant_q8_0), with its bytes per second
(1.0625 bytes read + 2 written per weight).  depth / depth_single below flux-dev's 19 / 38 shorten all three routes alike; the JSON says which were run.
Writes profiles/gguf_probe.json (or the path given).

    python profiles/gguf_probe.py [depth=19] [depth_single=38] [out.json]
"""
import gc
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import ldx_amd as ldx  # noqa: E402

GGUFTensor, GGML_F32, GGML_Q8_0 = ldx.gguf.GGUFTensor, ldx.gguf.GGML_F32, ldx.gguf.GGML_Q8_0

depth = int(sys.argv[1]) if len(sys.argv) > 1 else 19
depth_single = int(sys.argv[2]) if len(sys.argv) > 2 else 38
path = sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "profiles", "gguf_probe.json")
assert torch.cuda.is_available(), "gguf_probe.py measures on the GPU; there is no CPU fallback"

cfg = ldx.FluxConfig(depth=depth, depth_single_blocks=depth_single)
spec = ldx.weights.flux_state_dict_spec(cfg)
# one pool of random blocks as large as the largest tensor; every tensor is its own copy of the head of it, in memory of its own as the tensors of a mapped
# file are (the routes' times do not depend on the values, only on their being finite)
largest = max(int(np.prod(s)) for _, s in spec)
rng = np.random.default_rng(0)
pool = np.empty((largest // 32, 34), np.uint8)
pool[:, :2] = (1e-3 * (0.5 + rng.random(largest // 32))).astype(np.float16).view(np.uint8).reshape(-1, 2)
pool[:, 2:] = rng.integers(-127, 128, (largest // 32, 32), dtype=np.int8).view(np.uint8)
pool = torch.from_numpy(pool.reshape(-1))
tensors = {}
for k, s in spec:
    n = int(np.prod(s))
    if len(s) == 2:
        tensors[k] = GGUFTensor(pool[:n // 32 * 34].clone(), GGML_Q8_0, s, name=k)
    else:
        tensors[k] = GGUFTensor(torch.full((n,), 0.01, dtype=torch.float32).view(torch.uint8), GGML_F32, s, name=k)
n_q8 = sum(t.numel() for t in tensors.values() if t.is_quantized)
print(f"depth {depth} / {depth_single}: {len(tensors)} tensors, {n_q8 / 1e9:.2f} G Q8_0 weights ({n_q8 / 32 * 34 / 2**30:.2f} GiB of blocks)", flush=True)


def timed(fn):
    gc.collect()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, time.perf_counter() - t0


def route_dense():
    t0 = time.perf_counter()
    dense = {k: t.dequantize() for k, t in tensors.items()}
    route_dense.dequantize_s = time.perf_counter() - t0
    return ldx.FluxEngine(cfg, dense, device=0, dtype="bf16")


torch.zeros(1, device="cuda")          # the context and the library are up before the first route
ldx.lib.load()
res = {"device": torch.cuda.get_device_name(0), "dtype": "bf16", "depth": depth, "depth_single_blocks": depth_single, "full_depth": (depth, depth_single) == (19, 38),
       "tensors": len(tensors), "q8_0_weights": n_q8, "q8_0_block_bytes": n_q8 // 32 * 34}
digests = {}
for name, fn in (("c_device", lambda: ldx.FluxEngine(cfg, tensors, device=0, dtype="bf16", device_weights=True)),
                 ("b_host", lambda: ldx.FluxEngine(cfg, tensors, device=0, dtype="bf16", device_weights=False)),
                 ("a_dense", route_dense)):
    eng, s = timed(fn)
    digests[name] = eng.packed_digest()
    eng.close()
    del eng
    torch.cuda.empty_cache()
    res[name + "_s"] = s
    print(f"{name}: {s:.2f} s", flush=True)
res["a_dense_dequantize_s"] = route_dense.dequantize_s
res["same_packed_weights"] = len(set(digests.values())) == 1

# inside (c): the copies and the kernel on their own
L = ldx.lib.load()
out = torch.empty(largest, device="cuda", dtype=torch.float16)
copy_s, kernel_ms = 0.0, 0.0
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
for t in tensors.values():
    if not t.is_quantized:
        continue
    raw, s = timed(lambda: t.raw.to("cuda"))
    copy_s += s
    e0.record()
    ldx.lib.check(L.ldx_op_dequant_q8_0(ldx.lib.ptr(raw), t.numel(), ldx.lib.LDX_F16, ldx.lib.ptr(out), ldx.lib.current_stream_ptr()), "ldx_op_dequant_q8_0")
    e1.record()
    e1.synchronize()
    kernel_ms += e0.elapsed_time(e1)
    del raw
res["c_upload_s"] = copy_s
res["c_upload_GBps"] = res["q8_0_block_bytes"] / copy_s / 1e9
res["c_kernel_ms"] = kernel_ms
res["c_kernel_GBps"] = (res["q8_0_block_bytes"] + 2 * n_q8) / (kernel_ms * 1e-3) / 1e9
print(json.dumps(res, indent=1, sort_keys=True))
os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
with open(path, "w") as f:
    json.dump(res, f, indent=1, sort_keys=True)
    f.write("\n")
