"""What every engine plans and launches, recorded without a GPU: `make -C lightdiffusion-next_amd/csrc host` links the library's own sources (compiled for the host
alone) against a stand-in HIP runtime (tests/tools/hip_standin.cpp) that hands out made-up device addresses and writes one record per kernel launch, asynchronous
copy and memset: the kernel's mangled name, grid, block, dynamic LDS bytes and the bytes of every explicit argument (sizes from the code objects' metadata of the
real libldx.so).  This tool builds small nets through the C ABI of that library (ctypes, made-up device pointers, no torch.cuda), runs every case below and digests
the records of each; tests/golden/plan_traces.json keeps (number of records, 32-bit digest) per case and environment, and
tests/test_plan_trace_cpu.py holds the current planner to it.  A planner change that is meant to leave plans alone is proven by this table staying as it is.

Cases (CASES below; bf16 and fp16 each): the tiny UNet and the three small nets of xf_picks.CONFIGS at latents 16^2, 24 x 16 and 40 x 24 through ldx_unet_forward /
denoise / denoise_t / denoise_cfg_t (share modes 0, 1, 2) with the context cache off and on (two calls, so that the ctx_only split shows), a 9-channel tiny UNet through
ldx_unet_denoise_concat; the tiny VAE (decode and encode), CLIP (with and without an intermediate layer), T5 and ESRGAN; the tiny Flux net, and a 256-wide one with
head dim 128 in fp8 modes 0, 1 and 3 (the tiny net's width of 64 cannot run MX fp8).  The cases of one engine run in order in one process: a plan's addresses depend
on the allocations before it, so the FIRST differing case of an environment is the one to look at: `--records N` of this tree against the same of the tree the
table was written from (diff the two outputs) shows the first differing record.

    python tests/tools/plan_trace.py            # the current build against the table: per environment the cases that differ
    python tests/tools/plan_trace.py --write    # accept the current build's traces as the new table (only for a change that MEANS to change plans)
    python tests/tools/plan_trace.py --dump     # the digests of the current environment on stdout (what the test's subprocesses run)
    python tests/tools/plan_trace.py --rows     # the cases, one per line
    python tests/tools/plan_trace.py --show     # the committed table, readable
    python tests/tools/plan_trace.py --records N        # the records of case N in the current environment, kernel names demangled
    python tests/tools/plan_trace.py --full [DIR]       # not in the table: SD1.5 at latents 64^2 and 128^2, CFG batch 2, share 0 / 1 (the shapes at which dup_rows
                                                        # producers and the 8192-row share threshold are live); prints the digests, writes the traces into DIR

--weights in front of any of the first six turns them to the second table, tests/golden/weight_bytes.json (tests/test_weight_bytes_cpu.py): the packed weights.  With
LDX_STANDIN_WEIGHTS set the stand-in runtime also records every synchronous host-to-device copy as (destination, bytes, 64-bit FNV-1a of the bytes), so the records of
a "build" case hold every packed buffer's address and content.  The cases (weight_rows) are the "build" cases above, then the UNets twice more: with every tensor
registered through ldx_load_tensor_device at a made-up device address ("build_dev": the pack kernels' launches, grids and argument bytes, sizes from libldx_pack.so's
code objects), and with every third key on the host ("build_mixed": the staging copies too).  The environments (WEIGHT_ENVS) are the four that change packed weights.
A change to the packers or to a layout's description that is meant to leave the weights alone leaves this table alone.
"""
import ctypes as C
import hashlib
import json
import os
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from pick_table import ROOT, env_key, rows_digest  # noqa: E402,F401  (the test asks this module for them)
import kernel_resources  # noqa: E402
import pick_table  # noqa: E402
import xf_picks  # noqa: E402

TABLE = os.path.join(ROOT, "tests", "golden", "plan_traces.json")
CSRC = os.path.join(ROOT, "lightdiffusion-next_amd", "csrc")
HOST_LIB = os.path.join(ROOT, "lightdiffusion-next_amd", "libldx_host.so")
ARG_SIZES = os.path.join(CSRC, "build", "host", "kernel_args.txt")
FIELDS = ("records", "sha256[:8]")
WEIGHT_TABLE = os.path.join(ROOT, "tests", "golden", "weight_bytes.json")
WEIGHT_ENVS = [{}, {"LDX_NO_FUSED_SKIP": "1"}, {"LDX_NO_QPRESCALE": "1"}, {"LDX_LNFOLD": "0"}]

# the planner switches that live in PlanSwitches or are read at planning time, flipped, and the dispatch switches a plan depends on.  No level of the small nets
# fills the chip with row blocks, so LDX_ROWGEMM=0, LDX_XATTN_FUSE=0 and LDX_FF_FUSE=0 alone change nothing here (DEAD; they are held to the default's digests all the
# same): ROWBLOCKS lifts the chip-fill rule, which makes rowgemm, xattn_block and ff_block launches part of the plans, and the three switches are flipped under it too.
# LDX_VAE_ATTN_CHUNK_MIB=1 is dead as well: the smallest chunk is 256 score rows, the tiny VAE attends over 64.
ROWBLOCKS = {"LDX_ROWBLOCK_MINWG": "0", "LDX_ROWBLOCK_MINWG_PREFIX": "0"}
DEAD = [{"LDX_ROWGEMM": "0"}, {"LDX_XATTN_FUSE": "0"}, {"LDX_FF_FUSE": "0"}, {"LDX_VAE_ATTN_CHUNK_MIB": "1"}]
ENVS = ([{}] + [{k: v} for k, v in (("LDX_CFG_SHARE_COPY", "1"), ("LDX_CFG_SHARE_MINROWS", "0"), ("LDX_NO_FUSED_SKIP", "1"), ("LDX_NO_QPRESCALE", "1"), ("LDX_LNFOLD", "0"),
                                    ("LDX_EMB_TABLE", "0"), ("LDX_PLAN_CACHE_GIB", "0"), ("LDX_MX_FUSE", "0"), ("LDX_FLUX_FP8_ATTN", "0"), ("LDX_FLUX_GROUP", "0"),
                                    ("LDX_FLUX_MOD_FP8", "0"), ("LDX_GN_FUSE", "0"), ("LDX_PP", "0"), ("LDX_SPLITK", "2"))]
        + DEAD + [ROWBLOCKS] + [dict(ROWBLOCKS, **e) for e in DEAD[:3]])

DTYPES = ("bf16", "f16")
LATENTS = ((16, 16), (24, 16), (40, 24))
UNETS = dict(xf_picks.CONFIGS, tiny=None)
del UNETS["sd15"]
FLUX256 = dict(in_channels=16, vec_in_dim=64, context_in_dim=128, hidden_size=256, num_heads=2, depth=2, depth_single_blocks=3, axes_dim=(16, 56, 56))
MC = 77


def _unet_rows(cfg, dt):
    """(model, net, dtype, entry point, h, w, batch, share mode, context cache) — batch: the evaluation batch, for cfg_t the latent batch."""
    rows = []
    for h, w in LATENTS:
        rows += [("unet", cfg, dt, "denoise", h, w, b, 1, 0) for b in (1, 2, 4)]
        rows += [("unet", cfg, dt, e, h, w, 2, 1, 0) for e in ("forward", "denoise_t")]
        rows += [("unet", cfg, dt, "cfg_t", h, w, b, share, 0) for b in (1, 2) for share in (0, 2)] + [("unet", cfg, dt, "cfg_t", h, w, 1, 1, 0)]
        rows += [("unet", cfg, dt, e, h, w, b, share, 1) for e, b, share in (("denoise", 2, 1), ("cfg_t", 1, 0), ("cfg_t", 1, 2))]
    return rows + [("unet", cfg, dt, "denoise", 16, 16, 1, 1, 2)]          # a shape seen before: the plan cache (LDX_PLAN_CACHE_GIB) decides whether it is planned again


def all_rows():
    rows = []
    for cfg in UNETS:
        for dt in DTYPES:
            rows += [("unet", cfg, dt, "build", 0, 0, 0, 0, 0)] + _unet_rows(cfg, dt)
    for dt in DTYPES:
        rows += [("unet", "tiny_in9", dt, "build", 0, 0, 0, 0, 0)] + [("unet", "tiny_in9", dt, "denoise_concat", h, w, b, 1, 0) for h, w in LATENTS for b in (1, 2)]
        rows += [("vae", "tiny", dt, "build", 0, 0, 0, 0, 0)] + [("vae", "tiny", dt, "decode", h, w, b, 0, 0) for h, w in ((8, 8), (9, 8)) for b in (1, 2)]
        rows += [("vae", "tiny", dt, "encode", h, w, b, 0, 0) for h, w in ((64, 64), (72, 64)) for b in (1, 2)]
        rows += [("clip", "tiny", dt, "build", 0, 0, 0, 0, 0)] + [("clip", "tiny", dt, "encode", 77, inter, b, 0, 0) for b in (1, 2) for inter in (0, -2)]      # w: inter_layer (0 = no intermediate output)
        rows += [("t5", "tiny", dt, "build", 0, 0, 0, 0, 0)] + [("t5", "tiny", dt, "encode", L, 0, b, 0, 0) for L in (40, 77) for b in (1, 2)]
        rows += [("esrgan", "tiny", dt, "build", 0, 0, 0, 0, 0)] + [("esrgan", "tiny", dt, "forward", h, w, 1, 0, 0) for h, w in ((16, 16), (24, 16))]
        for net, modes in (("tiny", (0,)), ("w256", (0, 1, 3))):
            for mode in modes:            # share column: ldx_flux_set_fp8 mode; cache column: text tokens
                rows += [("flux", net, dt, "build", 0, 0, 0, mode, 0)] + [("flux", net, dt, "forward", h, w, b, mode, lt) for h, w, b, lt in ((16, 16, 1, 40), (16, 24, 2, 33))]
    return rows


def weight_rows():
    build = [r for r in all_rows() if r[3] == "build"]
    return build + [r[:3] + (how,) + r[4:] for how in ("build_dev", "build_mixed") for r in build if r[0] == "unet"]


FULL_ROWS = [("unet", "sd15", "bf16", "build", 0, 0, 0, 0, 0)] + [("unet", "sd15", "bf16", "cfg_t", n, n, b, share, 0) for n in (64, 128) for b in (1, 2) for share in (0, 1)]


# ---- kernel argument sizes, from the code objects of the real library
def kernel_arg_sizes(lib_path=kernel_resources.LIB):
    """{mangled kernel name: [bytes of every explicit argument]} from `llvm-readelf --notes` of every gfx950 code object (hidden arguments left out)."""
    import shutil
    tmp = tempfile.mkdtemp(prefix="ldx_args_")
    try:
        so = os.path.join(tmp, "libldx.so")
        shutil.copy(lib_path, so)
        subprocess.run([os.path.join(kernel_resources.LLVM, "llvm-objdump"), "--offloading", so], check=True, capture_output=True, cwd=tmp)
        out = {}
        for f in sorted(os.listdir(tmp)):
            if "amdgcn" not in f:
                continue
            notes = subprocess.run([os.path.join(kernel_resources.LLVM, "llvm-readelf"), "--notes", os.path.join(tmp, f)], check=True, capture_output=True, text=True).stdout
            args, name = [], None
            for line in notes.splitlines() + ["  - .end:"]:
                if line.startswith("  - ."):                        # next kernel record
                    if name:
                        out[name] = [a["size"] for a in args if not a.get("value_kind", "").startswith("hidden")]
                    args, name = [], None
                if line.startswith("      - ."):                    # next argument record
                    args.append({})
                key, _, val = line.strip().lstrip("- ").partition(":")
                if line.startswith("    .name:"):
                    name = val.strip()
                elif line.startswith("      ") and args and key in (".size", ".value_kind"):
                    args[-1][key[1:]] = int(val) if key == ".size" else val.strip()
        return out
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def build_host():
    """The host library and the argument-size file, built on demand (the real library too: its code objects give the sizes)."""
    if not os.path.exists(kernel_resources.LIB):
        subprocess.run(["make", "-C", CSRC, "-j8"], check=True, capture_output=True)
    subprocess.run(["make", "-C", CSRC, "host", "-j8"], check=True, capture_output=True)
    # the load-time packers' kernels are in the second, the TAESD decoder's in the third, the phase-form up conv's in the fourth
    libs = (kernel_resources.LIB,) + tuple(os.path.join(os.path.dirname(kernel_resources.LIB), n) for n in ("libldx_pack.so", "libldx_taesd.so", "libldx_upconv.so"))
    if not os.path.exists(ARG_SIZES) or os.path.getmtime(ARG_SIZES) < max(map(os.path.getmtime, libs)):
        sizes = {}
        for lib in reversed(libs):
            sizes.update(kernel_arg_sizes(lib))
        with open(ARG_SIZES, "w") as f:
            f.write("".join(f"{k} {' '.join(map(str, v))}\n" for k, v in sorted(sizes.items())))


# ---- driving the C ABI of the host library
class Host:
    """libldx_host.so through ctypes; the records the stand-in runtime has written since the last take()."""

    def __init__(self):
        fd, self.path = tempfile.mkstemp(prefix="ldx_trace_")
        os.close(fd)
        os.environ["LDX_STANDIN_TRACE"], os.environ["LDX_STANDIN_ARGS"] = self.path, ARG_SIZES
        sys.path.insert(0, ROOT)
        import ldx_amd
        self.ldx, self.L = ldx_amd, C.CDLL(HOST_LIB)
        for name, (res, args) in ldx_amd.lib._SIGS.items():
            fn = getattr(self.L, name)
            fn.restype, fn.argtypes = res, args
        self.f = None

    def take(self):
        self.f = self.f or open(self.path)
        return self.f.read().splitlines()

    def check(self, rc, what):
        assert rc == 0, (what, rc, self.L.ldx_last_error().decode(errors="replace"))

    def load(self, h, sd, strip=(), how="build"):
        """how: "build" every tensor from the host; "build_dev" every tensor as device memory at a made-up address (nothing reads it); "build_mixed" every third
        key from the host."""
        import torch
        for i, (k, t) in enumerate(sd.items()):
            for pre in strip:
                if k.startswith(pre):
                    k = k[len(pre):]
            t = t.detach().contiguous()
            if t.dtype not in (torch.float16, torch.bfloat16, torch.float32):
                t = t.float()
            if how == "build_dev" or (how == "build_mixed" and i % 3):
                self.check(self.L.ldx_load_tensor_device(h, k.encode(), C.c_void_p(DEV_SRC + (i << 28)), self.ldx.lib.torch_dtype_code(t.dtype), (C.c_int64 * t.dim())(*t.shape), t.dim()), k)
                continue
            self.check(self.L.ldx_load_tensor(h, k.encode(), C.c_void_p(t.data_ptr()), self.ldx.lib.torch_dtype_code(t.dtype), (C.c_int64 * t.dim())(*t.shape), t.dim()), k)


DEV_SRC = 0x7e0000000000                                                      # ... and its state dict's tensors, 256 MiB apart (build_dev / build_mixed)
P = {n: 0x7f0000000000 + (i << 32) for i, n in enumerate(("x", "s", "ctx", "out", "cc", "t", "ids", "out2", "bias", "y", "guid", "cos", "sin"))}      # the caller's "device" buffers


def _struct(cls, dt, **kw):
    c = cls()
    c.compute_dtype = 0 if dt == "bf16" else 1
    for k, v in kw.items():
        if isinstance(v, (tuple, list)):
            for i, x in enumerate(v):
                getattr(c, k)[i] = x
        else:
            setattr(c, k, int(v))
    return c


_SD = {}


def _synth(W, name, spec):
    """weights.synth_state_dict, once per net (both compute types load the same tensors)."""
    if name not in _SD:
        _SD.clear()
        _SD[name] = W.synth_state_dict(spec)
    return _SD[name]


def _engine(H, row):
    """Create and load the engine of a "build" row (the caller finalizes it)."""
    import dataclasses
    ldx, L, W = H.ldx, H.L, H.ldx.weights
    model, net, dt, mode = row[0], row[1], row[2], row[7]
    h = C.c_void_p()
    if model == "unet":
        cfg = W.UNetConfig.tiny(64, 128) if net.startswith("tiny") else W.UNetConfig(**dict({} if net == "sd15" else {"context_dim": 128}, **xf_picks.CONFIGS[net]))
        if net == "tiny_in9":
            cfg = dataclasses.replace(cfg, in_channels=9)
        c = _struct(ldx.lib.ldx_unet_config, dt, in_channels=cfg.in_channels, out_channels=cfg.out_channels, model_channels=cfg.model_channels, num_levels=len(cfg.channel_mult),
                    channel_mult=cfg.channel_mult, num_res_blocks=cfg.num_res_blocks, transformer_depth=cfg.transformer_depth, transformer_depth_output=cfg.transformer_depth_output,
                    transformer_depth_middle=cfg.transformer_depth_middle, num_heads=cfg.num_heads, context_dim=cfg.context_dim)
        H.check(L.ldx_create(C.byref(c), 0, C.byref(h)), "ldx_create")
        H.load(h, _synth(W, net, W.unet_state_dict_spec(cfg)), how=row[3])
        _, ls = ldx.engine.sd15_sigmas()
        temb = ldx.engine.timestep_embedding_table(ls.numel(), cfg.model_channels)
        H.check(L.ldx_set_tables(h, C.c_void_p(ls.data_ptr()), ls.numel(), C.c_void_p(temb.data_ptr()), temb.shape[1]), "ldx_set_tables")
        return h, cfg
    if model == "vae":
        cfg = W.VAEConfig.tiny()
        c = _struct(ldx.lib.ldx_vae_config, dt, z_channels=cfg.z_channels, ch=cfg.ch, num_levels=len(cfg.ch_mult), ch_mult=cfg.ch_mult, num_res_blocks=cfg.num_res_blocks,
                    out_ch=cfg.out_ch, use_post_quant=cfg.use_post_quant)
        H.check(L.ldx_vae_create(C.byref(c), 0, C.byref(h)), "ldx_vae_create")
        H.load(h, W.synth_state_dict(W.vae_state_dict_spec(cfg)))
    elif model == "clip":
        cfg = W.CLIPConfig.tiny()
        c = _struct(ldx.lib.ldx_clip_config, dt, hidden_size=cfg.hidden_size, num_layers=cfg.num_layers, num_heads=cfg.num_heads, intermediate_size=cfg.intermediate_size,
                    max_positions=cfg.max_positions, vocab_size=cfg.vocab_size)
        H.check(L.ldx_clip_create(C.byref(c), 0, C.byref(h)), "ldx_clip_create")
        H.load(h, W.synth_state_dict(W.clip_state_dict_spec(cfg)))
    elif model == "t5":
        cfg = W.T5Config.tiny()
        c = _struct(ldx.lib.ldx_t5_config, dt, d_model=cfg.d_model, d_ff=cfg.d_ff, num_layers=cfg.num_layers, num_heads=cfg.num_heads, vocab_size=cfg.vocab_size)
        H.check(L.ldx_t5_create(C.byref(c), 0, C.byref(h)), "ldx_t5_create")
        H.load(h, {k: v for k, v in W.synth_state_dict(W.t5_state_dict_spec(cfg)).items() if "relative_attention_bias" not in k})
    elif model == "esrgan":
        cfg = W.ESRGANConfig.tiny()
        c = _struct(ldx.lib.ldx_esrgan_config, dt, in_nc=cfg.in_nc, out_nc=cfg.out_nc, nf=cfg.nf, gc=cfg.gc, num_blocks=cfg.num_blocks, num_upscale=2)
        H.check(L.ldx_esrgan_create(C.byref(c), 0, C.byref(h)), "ldx_esrgan_create")
        H.load(h, W.synth_state_dict(W.esrgan_state_dict_spec(cfg)))
    elif model == "taesd":
        import torch
        cfg = None
        c = _struct(ldx.lib.ldx_taesd_config, dt, latent_channels=4)
        H.check(L.ldx_taesd_create(C.byref(c), 0, C.byref(h)), "ldx_taesd_create")
        H.load(h, W.synth_state_dict(W.taesd_decoder_state_dict_spec(), dtype=torch.float32))
    else:
        cfg = W.FluxConfig.tiny() if net == "tiny" else W.FluxConfig(**FLUX256)
        c = _struct(ldx.lib.ldx_flux_config, dt, in_channels=cfg.in_channels, vec_in_dim=cfg.vec_in_dim, context_in_dim=cfg.context_in_dim, hidden_size=cfg.hidden_size,
                    mlp_hidden=cfg.mlp_hidden, num_heads=cfg.num_heads, depth=cfg.depth, depth_single=cfg.depth_single_blocks, guidance_embed=cfg.guidance_embed)
        H.check(L.ldx_flux_create(C.byref(c), 0, C.byref(h)), "ldx_flux_create")
        if mode:
            H.check(L.ldx_flux_set_fp8(h, mode), "ldx_flux_set_fp8")
        H.load(h, W.synth_state_dict(W.flux_state_dict_spec(cfg)))
    return h, cfg


def _run(H, h, cfg, row):
    L = H.L
    model, _, _, entry, a, b, n, share, cache = row
    if model == "unet":
        H.check(L.ldx_unet_cfg_share(h, share), "ldx_unet_cfg_share")
        H.check(L.ldx_unet_context_cache(h, int(cache == 1)), "ldx_unet_context_cache")
        for _ in range(2 if cache == 1 else 1):
            if entry == "cfg_t":
                rc = L.ldx_unet_denoise_cfg_t(h, P["x"], 3.0, 500, P["ctx"], n, a, b, MC, P["out"], None)
            elif entry == "denoise_t":
                rc = L.ldx_unet_denoise_t(h, P["x"], P["s"], P["t"], P["ctx"], n, a, b, MC, P["out"], None)
            elif entry == "denoise_concat":
                rc = L.ldx_unet_denoise_concat(h, P["x"], P["s"], P["ctx"], P["cc"], 5, n, a, b, MC, P["out"], None)
            else:
                rc = getattr(L, "ldx_unet_" + entry)(h, P["x"], P["s"], P["ctx"], n, a, b, MC, P["out"], None)
            H.check(rc, row)
        return
    if model == "vae":
        rc = getattr(L, "ldx_vae_" + entry)(h, P["x"], n, a, b, P["out"], None)
    elif model == "clip":
        rc = L.ldx_clip_encode(h, P["ids"], n, a, b, P["out"], P["out2"] if b else None, None)
    elif model == "t5":
        rc = L.ldx_t5_encode(h, P["ids"], n, a, P["bias"], P["out"], None)
    elif model == "esrgan":
        rc = L.ldx_esrgan_forward(h, P["x"], n, a, b, P["out"], None)
    else:
        rc = L.ldx_flux_forward(h, P["x"], P["s"], P["ctx"], P["y"], P["guid"], P["cos"], P["sin"], n, a, b, cache, 1, P["out"], None)
    H.check(rc, row)


def traces_of_current_env(rows):
    """[records] per row, in this process's environment."""
    H = Host()
    H.take()
    out, h, cfg = [], None, None
    for row in rows:
        if row[3].startswith("build"):
            if h:
                H.L.ldx_destroy(h)
            h, cfg = _engine(H, row)
            H.check(H.L.ldx_finalize(h), "ldx_finalize")
        else:
            _run(H, h, cfg, row)
            n, f, ar = C.c_int64(), C.c_double(), C.c_int64()
            H.check(H.L.ldx_plan_info(h, C.byref(n), C.byref(f), C.byref(ar)), "ldx_plan_info")
        out.append(H.take() + ([f"P launches={n.value} flops={f.value!r} arena={ar.value}"] if not row[3].startswith("build") else []))
    if h:
        H.L.ldx_destroy(h)
    os.unlink(H.path)
    return out


def digest(records):
    return (len(records), hashlib.sha256("\n".join(records).encode()).hexdigest()[:8])


def picks_of_current_env(rows):
    traces = traces_of_current_env(rows)
    for row, t in zip(rows, traces):          # a kernel without argument sizes would drop its argument bytes from the digest
        assert not any(r.endswith(" ?") for r in t), f"{row}: a launch of a kernel that {ARG_SIZES} does not list: {[r for r in t if r.endswith(' ?')][:1]}"
    return [digest(t) for t in traces]


def picks_of_env(env):
    return pick_table.picks_of_env(__file__, dict(env, OMP_NUM_THREADS="1", MKL_NUM_THREADS="1"))      # several environments run at a time: one thread each for torch


def picks_of_envs(envs, workers=8):
    """picks_of_env of every environment, `workers` processes at a time."""
    from concurrent.futures import ThreadPoolExecutor
    with ThreadPoolExecutor(max(1, min(workers, os.cpu_count() or 1))) as pool:
        return dict(zip(map(env_key, envs), pool.map(picks_of_env, envs)))


def records_of_env(env, index):
    """The records of case `index` under `env` (a fresh process, as the digests are taken), kernel names demangled."""
    clean = {k: v for k, v in os.environ.items() if not k.startswith("LDX_")}
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--records", str(index)], env=dict(clean, **env), capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    return r.stdout.splitlines()


# ---- the table (pick_table's digest format)
def load_table():
    return pick_table.load_table(TABLE)


decode = pick_table.decode_digests


def write_table(per_env, rows, path=TABLE):
    return pick_table.write_digest_table(path, per_env, rows, fields=list(FIELDS))


def describe(row, pick):
    return f"{row} -> {pick[0]} records, digest {pick[1]}"


def mismatch(env, index, row, got, want):
    """One line about a differing case.  The table holds one digest per case, so it cannot say WHICH record differs: the records of this tree and of the tree the table
    was written from, listed with --records, have to be compared for that."""
    recs = records_of_env(env, index)
    return (f"{env_key(env)}: case {index} {row}: {got[0]} records, digest {got[1]} (table: {want[0]}, {want[1]}); the table cannot name the record that differs - "
            f"`{' '.join(f'{k}={v}' for k, v in env.items())} python tests/tools/plan_trace.py --records {index}` lists the records of this tree "
            f"(the first of {len(recs)}: {recs[0][:300] if recs else None})")


def demangle(names):
    """{mangled: demangled} by c++filt.  binutils knows neither 16-bit float mangling (DF16_, DF16b): they are given as two builtin types that no kernel here uses
    (half, char32_t) and renamed in the output."""
    out = subprocess.run(["c++filt"], input="\n".join(n.replace("DF16b", "Di").replace("DF16_", "Dh") for n in names), capture_output=True, text=True, check=True).stdout.splitlines()
    assert len(out) == len(names) and not any(o.startswith("_Z") for o in out), f"c++filt left names mangled: {[o for o in out if o.startswith('_Z')][:2]}"
    return {n: o.replace("char32_t", "__bf16").replace("half", "_Float16") for n, o in zip(names, out)}


def _demangled(records):
    dm = demangle(sorted({r.split()[1] for r in records if r.startswith("L ")}))
    return [" ".join([r.split()[0], dm[r.split()[1]]] + r.split()[2:]) if r.startswith("L ") else r for r in records]


class Weights:
    """The tool (pick_table.cli) of the second table; its --dump processes are told apart by LDX_STANDIN_WEIGHTS, which the stand-in runtime reads too."""
    ENVS, TABLE, all_rows = WEIGHT_ENVS, WEIGHT_TABLE, staticmethod(weight_rows)
    picks_of_current_env, decode, describe = staticmethod(picks_of_current_env), staticmethod(pick_table.decode_digests), staticmethod(describe)

    @staticmethod
    def picks_of_envs(envs):
        return dict(zip(map(env_key, envs), picks_of_envs([dict(e, LDX_STANDIN_WEIGHTS="1") for e in envs]).values()))

    @staticmethod
    def load_table():
        return pick_table.load_table(WEIGHT_TABLE)

    @staticmethod
    def write_table(per_env, rows):
        return write_table(per_env, rows, WEIGHT_TABLE)

    @staticmethod
    def mismatch(env, index, row, got, want):
        return (f"{env_key(env)}: case {index} {row}: {got[0]} records, digest {got[1]} (table: {want[0]}, {want[1]}); `{' '.join(f'{k}={v}' for k, v in env.items())} "
                f"python tests/tools/plan_trace.py --weights --records {index}` lists this tree's records, to be compared with those of the tree the table was written from")


if __name__ == "__main__":
    weights = "--weights" in sys.argv or "LDX_STANDIN_WEIGHTS" in os.environ
    if weights:
        os.environ["LDX_STANDIN_WEIGHTS"] = "1"
    if "--rows" not in sys.argv and "--show" not in sys.argv:
        build_host()
    if "--records" in sys.argv:
        n = int(sys.argv[sys.argv.index("--records") + 1])
        print("\n".join(_demangled(traces_of_current_env((weight_rows() if weights else all_rows())[:n + 1])[n])))
    elif "--full" in sys.argv:
        i = sys.argv.index("--full")
        out_dir = sys.argv[i + 1] if i + 1 < len(sys.argv) else None
        for row, t in zip(FULL_ROWS, traces_of_current_env(FULL_ROWS)):
            print(row, *digest(t))
            if out_dir:
                os.makedirs(out_dir, exist_ok=True)
                with open(os.path.join(out_dir, "_".join(map(str, row)) + ".txt"), "w") as f:
                    f.write("\n".join(t) + "\n")
    else:
        pick_table.cli(Weights if weights else sys.modules[__name__])
