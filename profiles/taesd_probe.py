"""Device time of one TAESD preview at a 128^2 latent (a 1024^2 image): TAESDEngine.preview in graph mode (hipGraph replays: the probe checks the engine's
replay counter) and as eager launches, and next to it the same network run as torch.nn.functional.conv2d in bf16, channels-last, in the same process on the
same GPU, as eager ops (about 80 per pass) and, with --torch-graph, replayed through torch.cuda.graph.
Synthetic weights from a seed; reads nothing outside the repository.

    python profiles/taesd_probe.py [--out FILE] [--latent 128] [--batch 1] [--iters 30] [--step-ms 13.3] [--limit 300] [--torch-graph]

Prints one JSON line (and writes it to --out): both times in ms (HIP events around `iters` back-to-back previews after a warm-up, divided by iters), the
algorithmic TFLOP/s of each, their agreement (share of bytes that differ by more than 2 codes), and the preview's share of a sampler step at the every-fifth
cadence: preview_ms / (5 * step_ms).  step_ms is NOT measured here: it is the CFG-batched 1024^2 UNet step that bench.py reports (README.md: 13.07-13.46 ms
by box), 13.3 unless given.
--limit: seconds after which the probe gives up (SIGALRM), so a wedged run ends by itself."""
import argparse
import json
import os
import signal
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def torch_decoder(sd, dtype=torch.bfloat16):
    """Decoder2 + the preview's quantisation as plain torch ops on channels-last `dtype` tensors (the baseline a port without kernels of its own would run)."""
    F = torch.nn.functional
    w = {k: (v.to("cuda", dtype).contiguous(memory_format=torch.channels_last) if v.dim() == 4 else v.to("cuda", dtype)) for k, v in sd.items()}

    def conv(h, pre, bias=True):
        return F.conv2d(h, w[pre + ".weight"], w[pre + ".bias"] if bias else None, padding=1)

    def block(h, i):
        t = F.relu(conv(h, f"{i}.conv.0"))
        t = F.relu(conv(t, f"{i}.conv.2"))
        return F.relu(conv(t, f"{i}.conv.4") + h)

    def run(x):
        h = (torch.tanh(x / 3) * 3).to(dtype).contiguous(memory_format=torch.channels_last)
        h = F.relu(conv(h, "1"))
        for i in (3, 4, 5):
            h = block(h, i)
        for up, blocks in ((7, (8, 9, 10)), (12, (13, 14, 15)), (17, (18,))):
            h = conv(F.interpolate(h, scale_factor=2, mode="nearest"), str(up), bias=False)
            for i in blocks:
                h = block(h, i)
        d = conv(h, "19").float().sub(0.5).mul(2)
        return ((d + 1.0) / 2.0 * 255.0).clamp(0, 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous()
    return run


def timed(fn, iters, warmup=5):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--latent", type=int, default=128)
    ap.add_argument("--batch", type=int, default=1)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--step-ms", type=float, default=13.3)
    ap.add_argument("--limit", type=int, default=300)
    ap.add_argument("--torch-graph", action="store_true", help="also time the torch baseline replayed through torch.cuda.graph")
    a = ap.parse_args()
    signal.signal(signal.SIGALRM, lambda *_: sys.exit(f"taesd_probe: gave up after {a.limit} s"))
    signal.alarm(a.limit)
    assert torch.cuda.is_available(), "taesd_probe needs a GPU"
    import ldx_amd as ldx
    sd = ldx.weights.synth_state_dict(ldx.weights.taesd_decoder_state_dict_spec(), seed=4321, dtype=torch.float32)
    sd["19.weight"] = sd["19.weight"] * 0.343
    sd["19.bias"] = sd["19.bias"] + 0.5
    eng = ldx.TAESDEngine(ldx.TAESDConfig(), sd, device=0, dtype="bf16", graph=True)
    eager = ldx.TAESDEngine(ldx.TAESDConfig(), sd, device=0, dtype="bf16")
    x = 2.0 * torch.randn(a.batch, 4, a.latent, a.latent, generator=torch.Generator().manual_seed(1)).cuda()
    base = torch_decoder(sd)
    with torch.no_grad():
        ours, theirs = eng.preview(x), base(x)
        off = float((ours.to(torch.int16) - theirs.to(torch.int16)).abs().gt(2).float().mean())
        assert torch.equal(eager.preview(x), ours)
        # the torch baseline as a graph too, where it captures: both sides then pay no launch overhead
        tgraph, tg_out = None, None
        try:
            if not a.torch_graph:
                raise RuntimeError("not asked for (--torch-graph)")
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                for _ in range(3):
                    base(x)
            torch.cuda.current_stream().wait_stream(side)
            tgraph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(tgraph):
                tg_out = base(x)
            tgraph.replay()
            torch.cuda.synchronize()
            assert torch.equal(tg_out, theirs)
        except Exception as e:          # reported, not hidden: the eager figure stands alone then
            print(f"taesd_probe: torch.cuda.graph did not capture the baseline: {type(e).__name__}: {e}", file=sys.stderr)
            tgraph = None
        # alternate them, twice each, and keep the better pass of each: other work shares the host
        t_ldx, t_eager, t_torch, t_tgraph = [], [], [], []
        for _ in range(2):
            t_ldx.append(timed(lambda: eng.preview(x), a.iters))
            t_eager.append(timed(lambda: eager.preview(x), a.iters))
            t_torch.append(timed(lambda: base(x), a.iters))
            if tgraph is not None:
                t_tgraph.append(timed(tgraph.replay, a.iters))
    captures, replays = eng.graph_stats()
    assert captures == 1 and replays >= 2 * (a.iters + 5) - 2, (captures, replays)          # the timed passes were replays
    info = eng.plan_info()
    best_torch = min(t_torch + t_tgraph)
    res = {"probe": "taesd_preview", "latent": a.latent, "batch": a.batch, "iters": a.iters, "device": torch.cuda.get_device_name(0),
           "ldx_preview_ms": round(min(t_ldx), 4), "ldx_preview_ms_passes": [round(t, 4) for t in t_ldx], "ldx_mode": "hipGraph replay (engine graph mode)",
           "ldx_graph_captures": captures, "ldx_graph_replays": replays,
           "ldx_eager_preview_ms": round(min(t_eager), 4), "ldx_eager_ms_passes": [round(t, 4) for t in t_eager],
           "torch_bf16_channels_last_ms": round(min(t_torch), 4), "torch_ms_passes": [round(t, 4) for t in t_torch], "torch_mode": "eager ops",
           "torch_graph_ms": round(min(t_tgraph), 4) if t_tgraph else None, "torch_graph_ms_passes": [round(t, 4) for t in t_tgraph],
           "speedup_over_torch": round(best_torch / min(t_ldx), 3), "speedup_is_against": "the faster of torch eager and torch graph", "launches": info["launches"], "gflop": round(info["flops"] / 1e9, 2),
           "ldx_tflops": round(info["flops"] / min(t_ldx) / 1e9, 1), "torch_tflops": round(info["flops"] / best_torch / 1e9, 1),
           "bytes_off_by_more_than_2_vs_torch": off, "step_ms_assumed": a.step_ms, "step_ms_source": "not measured here: bench.py's 1024^2 step (README.md) or --step-ms",
           "share_of_step_at_every_5th": round(min(t_ldx) / (5 * a.step_ms), 4)}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
