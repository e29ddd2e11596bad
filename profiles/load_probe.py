"""How long the SD1.5 UNet engine takes to come up from a state dict that is resident on the GPU (what the reference's hook holds after
ModelPatcher.patch_model) and from the same state dict on the host (the CPU packers), and how long UNetEngine.refresh takes to replace the
weights of a running engine.

    python profiles/load_probe.py [--runs 3] [--dtype bf16] [--tree DIR]

--tree DIR imports the package from another checkout (a tree without UNetEngine.refresh reports the constructor alone), so one process per tree,
started alternately on the same box, gives the before / after pair.  Weights are random fp16 drawn on the device: the time does not depend on the
values.  The device is synchronized before and after every timed region.  One JSON line per measurement.
"""
import argparse
import json
import os
import sys
import time


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--dtype", default="bf16")
    ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--label", default="")
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.tree))
    import torch
    import ldx_amd as ldx

    cfg = ldx.UNetConfig.sd15()
    g = torch.Generator(device="cuda").manual_seed(0)
    sd = {}
    for k, shape in ldx.weights.unet_state_dict_spec(cfg):
        t = torch.randn(tuple(shape), generator=g, device="cuda", dtype=torch.float32) * 0.02
        sd[k] = (t + 1.0 if len(shape) == 1 and k.endswith(".weight") else t).half()
    label = args.label or os.path.basename(os.path.abspath(args.tree))

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        return r, time.perf_counter() - t0

    eng = None
    for i in range(args.runs):
        if eng is not None:
            eng.close()
        eng, dt = timed(lambda: ldx.UNetEngine(cfg, sd, device=0, dtype=args.dtype))
        print(json.dumps({"tree": label, "what": "UNetEngine(sd15, fp16 state dict on the GPU)", "run": i, "seconds": round(dt, 4)}), flush=True)
    sd_host = {k: v.cpu() for k, v in sd.items()}
    for i in range(args.runs):
        eng.close()
        eng, dt = timed(lambda: ldx.UNetEngine(cfg, sd_host, device=0, dtype=args.dtype))
        print(json.dumps({"tree": label, "what": "UNetEngine(sd15, fp16 state dict on the host)", "run": i, "seconds": round(dt, 4)}), flush=True)
    if hasattr(eng, "refresh"):
        for i in range(args.runs):
            _, dt = timed(lambda: eng.refresh(sd))
            print(json.dumps({"tree": label, "what": "refresh(fp16 state dict on the GPU)", "run": i, "seconds": round(dt, 4)}), flush=True)
    eng.close()


if __name__ == "__main__":
    main()
