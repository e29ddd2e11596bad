"""Python handles on the native engines (libldx.so): UNetEngine, VAEDecoderEngine, CLIPTextEngine, ESRGANEngine, T5Engine and FluxEngine over one base.

Host-side responsibilities only: hand the state dict to the C ABI once, build the lookup tables the
reference builds on the host (the UNet's sigma table and sinusoidal timestep embeddings), and pass device pointers.
Reference counterparts: BaseModel.__init__/load_model_weights/apply_model (src/Model/ModelBase.py:38-202).
"""
import ctypes as C
import math

import numbers

import torch

from . import lib
from .weights import T5Config  # noqa: F401
from .weights import UNetConfig, VAEConfig, CLIPConfig, FluxConfig


def sd15_sigmas():
    """ModelSamplingDiscrete._register_schedule + set_sigmas (src/sample/sampling.py:224-289) with
    make_beta_schedule("linear", 1000, 0.00085, 0.012) (src/sample/sampling_util.py:18-39).
    Returns (sigmas fp32 [1000], log_sigmas fp32 [1000]); fp64 until the final cast, like the reference."""
    betas = torch.linspace(0.00085 ** 0.5, 0.012 ** 0.5, 1000, dtype=torch.float64) ** 2
    alphas_cumprod = torch.cumprod(1.0 - betas, dim=0)
    sigmas = ((1 - alphas_cumprod) / alphas_cumprod) ** 0.5
    return sigmas.float(), sigmas.log().float()


def timestep_index(log_sigmas: torch.Tensor, sigma) -> torch.Tensor:
    """ModelSamplingDiscrete.timestep (src/sample/sampling.py:309-320, called from BaseModel.apply_model, ModelBase.py:112) on the HOST: the reference's
    expression `dists = sigma.log() - log_sigmas[:, None]; dists.abs().argmin(dim=0)`.  Integer work, so it has to be exact — and one ulp of log(sigma)
    decides the index at a near-tie (sigma at the geometric midpoint of two table entries: the `normal` scheduler's fractional timesteps).
    sigma: float / host tensor; returns int64 [n]."""
    sg = torch.as_tensor(sigma, dtype=torch.float32, device="cpu").reshape(-1)
    # the logarithm CORRECTLY ROUNDED (fp64 log, rounded once): torch's fp32 CPU log is correctly rounded for 99.98 % of inputs, and where it is not its last
    # bit follows the host's vector ISA — the GPU box's host put the golden near-tie sigma 0.3473117 (tests/golden/schedules.npz, captured in the build
    # container: index 101) on the other side.  The correctly rounded value reproduces every golden index on every host, and the device lookup
    # (csrc/misc.hip nearest_log_sigma) computes the same function.
    log_sigma = sg.double().log().float()
    return (log_sigma - log_sigmas[:, None]).abs().argmin(dim=0)


def timestep_embedding_table(n: int, dim: int, max_period: int = 10000) -> torch.Tensor:
    """timestep_embedding (src/sample/sampling_util.py:56-76) evaluated at t = 0..n-1 -> [n][dim] fp32."""
    half = dim // 2
    freqs = torch.exp(-math.log(max_period) * torch.arange(start=0, end=half, dtype=torch.float32) / half)
    args = torch.arange(n)[:, None].float() * freqs[None]
    return torch.cat([torch.cos(args), torch.sin(args)], dim=-1).contiguous()


_DTYPE_CODES = {"bf16": lib.LDX_BF16, "f16": lib.LDX_F16, "fp16": lib.LDX_F16}


class _Engine:
    """What the seven engines share: the library, the native handle and its lifetime, the way a state dict reaches it, the profile and the plan's figures."""

    def __init__(self, cfg, device: int):
        self._lib = lib.load()
        self._h = C.c_void_p()
        self.cfg, self.device = cfg, torch.device("cuda", device)

    def _create(self, struct, create, dtype: str, **fields):
        """The native engine: `create` (the name of an ldx_*_create) on a `struct` filled from `fields` (a list fills the head of an array)."""
        c = struct()
        c.compute_dtype = _DTYPE_CODES[dtype]
        for k, v in fields.items():
            if isinstance(v, (list, tuple)):
                for i, x in enumerate(v):
                    getattr(c, k)[i] = x
            else:
                setattr(c, k, int(v))
        lib.check(getattr(self._lib, create)(C.byref(c), self.device.index, C.byref(self._h)), create)

    def _load_state_dict(self, state_dict, strip=(), allow_device=False):
        """Register every tensor of a state dict, its key without the prefixes in `strip`.  A tensor goes through ldx_load_tensor, which copies it from the
        host.  allow_device (the UNet): a tensor on the engine's device is handed over where it lies instead (ldx_load_tensor_device: not copied, packed
        by device kernels).  Returns the tensors whose memory the engine refers to: the caller keeps them alive until ldx_finalize /
        ldx_unet_refresh_commit has returned."""
        keep = []
        for k, t in state_dict.items():
            for pre in strip:
                if k.startswith(pre):
                    k = k[len(pre):]
            t = t.detach()
            on_device = allow_device and t.is_cuda
            if on_device:
                if t.device != self.device:
                    raise ValueError(f"{k}: tensor on {t.device}, the engine is on {self.device} (move the state dict to the host or to that device)")
                if not t.is_contiguous():
                    raise ValueError(f"{k}: a device tensor must be contiguous (it is read where it lies, not copied)")
            else:
                t = t.to("cpu").contiguous()
            if t.dtype not in (torch.float16, torch.bfloat16, torch.float32):
                t = t.float()
            if on_device:
                keep.append(t)
            name = "ldx_load_tensor_device" if on_device else "ldx_load_tensor"
            shape = (C.c_int64 * t.dim())(*t.shape)
            lib.check(getattr(self._lib, name)(self._h, k.encode(), lib.ptr(t), lib.torch_dtype_code(t.dtype), shape, t.dim()), f"{name}({k})")
        if keep:
            torch.cuda.synchronize(self.device)      # whatever produced the device tensors (a LoRA merge on another stream) has finished
        return keep

    def _load_gguf_tensors(self, state_dict, strip=(), device_weights=True):
        """Register a state dict whose values are gguf.GGUFTensor (dense torch tensors among them take _load_state_dict's host route).
        device_weights: each tensor's raw bytes are copied to the device and registered there, tensor by tensor, so at most one raw tensor is alive beside
        the engine's own buffers: Q8_0 through ldx_load_tensor_q8_0(on_device = 1), which expands it into a buffer of the engine's before it returns, the
        rest through ldx_load_tensor_dev, whose tensors are returned (the caller keeps them until ldx_finalize has returned).  Otherwise the host
        route: ldx_load_tensor_q8_0(on_device = 0) expands on the host, ldx_load_tensor copies."""
        from .gguf import GGUFTensor, GGML_Q8_0, _TORCH
        keep, dense = [], {}
        for k, t in state_dict.items():
            if not isinstance(t, GGUFTensor):
                dense[k] = t
                continue
            for pre in strip:
                if k.startswith(pre):
                    k = k[len(pre):]
            shape = (C.c_int64 * len(t.tensor_shape))(*t.tensor_shape)
            raw = t.raw.to(self.device) if device_weights else t.raw.contiguous()
            if t.tensor_type == GGML_Q8_0:
                lib.check(self._lib.ldx_load_tensor_q8_0(self._h, k.encode(), lib.ptr(raw), shape, len(t.tensor_shape), int(device_weights)), f"ldx_load_tensor_q8_0({k})")
            elif device_weights:
                keep.append(raw)
                lib.check(self._lib.ldx_load_tensor_dev(self._h, k.encode(), lib.ptr(raw), lib.torch_dtype_code(_TORCH[t.tensor_type]), shape, len(t.tensor_shape)),
                          f"ldx_load_tensor_dev({k})")
            else:
                lib.check(self._lib.ldx_load_tensor(self._h, k.encode(), lib.ptr(raw), lib.torch_dtype_code(_TORCH[t.tensor_type]), shape, len(t.tensor_shape)),
                          f"ldx_load_tensor({k})")
            del raw
        if dense:
            self._load_state_dict(dense, strip=strip)
        if device_weights:
            torch.cuda.synchronize(self.device)
        return keep

    def _load_any(self, state_dict, strip=(), device_weights=True):
        """A dense torch state dict takes _load_state_dict's path; one that holds gguf.GGUFTensor values takes _load_gguf_tensors'."""
        from .gguf import GGUFTensor
        if any(isinstance(t, GGUFTensor) for t in state_dict.values()):
            return self._load_gguf_tensors(state_dict, strip=strip, device_weights=device_weights)
        return self._load_state_dict(state_dict, strip=strip)

    def packed_digest(self) -> int:
        """ldx_packed_digest: FNV-1a over every packed weight buffer (diagnostic: equal digests = bit-identical weights, however they were loaded)."""
        d = C.c_uint64()
        lib.check(self._lib.ldx_packed_digest(self._h, C.byref(d)), "ldx_packed_digest")
        return d.value

    def _finalize(self):
        lib.check(self._lib.ldx_finalize(self._h), "ldx_finalize")

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self._lib.ldx_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def profile(self, on: bool, reset: bool = True):
        lib.check(self._lib.ldx_profile(self._h, int(on), int(reset)), "ldx_profile")

    def profile_report(self) -> dict:
        import json
        buf = C.create_string_buffer(1 << 18)
        lib.check(self._lib.ldx_profile_report(self._h, buf, len(buf)), "ldx_profile_report")
        return json.loads(buf.value.decode())

    def plan_info(self):
        """launches / algorithmic flops (the reference's arithmetic for this evaluation) / arena bytes of the current plan, plus the flops as EXECUTED
        (`flops_executed`; smaller than `flops` by `flops_shared` when the plan computes the shared CFG prefix once, ldx_unet_cfg_share)."""
        n, f, a = C.c_int64(), C.c_double(), C.c_int64()
        lib.check(self._lib.ldx_plan_info(self._h, C.byref(n), C.byref(f), C.byref(a)), "ldx_plan_info")
        ex, sh = C.c_double(), C.c_double()
        lib.check(self._lib.ldx_plan_flops(self._h, C.byref(ex), C.byref(sh)), "ldx_plan_flops")
        return {"launches": n.value, "flops": f.value, "arena_bytes": a.value, "flops_executed": ex.value, "flops_shared": sh.value}


def _encode_token_weights(token_weight_pairs, empty_tokens, encode):
    """ClipTokenWeightEncoder.encode_token_weights (SDClip.py:36-97) around an encoder: the chunks of (id, weight) pairs go through `encode` in one batch,
    with the empty prompt (`empty_tokens(length)`, gen_empty_tokens, SDClip.py:10-22) behind them where a weight differs from 1; a weighted token's output
    is then moved along the line from the empty prompt's.  encode(chunks) -> (host tensor [n, T, E], second result); returns (cond [1, sum T, E], second result)."""
    to_encode, has_weights, max_len = [], False, 0
    for x in token_weight_pairs:
        toks = [a[0] for a in x]
        max_len = max(max_len, len(toks))
        has_weights = has_weights or not all(a[1] == 1.0 for a in x)
        to_encode.append(toks)
    sections = len(to_encode)
    if has_weights or sections == 0:
        to_encode.append(empty_tokens(max_len))
    out, second = encode(to_encode)
    output = []
    for k in range(sections):
        z = out[k:k + 1].clone()
        if has_weights:
            z_empty = out[-1]
            for j in range(z.shape[1]):
                wgt = token_weight_pairs[k][j][1]
                if wgt != 1.0:
                    z[0][j] = (z[0][j] - z_empty[j]) * wgt + z_empty[j]
        output.append(z)
    return (out[-1:] if not output else torch.cat(output, dim=-2)), second


class _GraphMode:
    """The hipGraph mode of the three engines that have one (UNetEngine, TAESDEngine, SAMImageEncoderEngine); the native engines of the other models ignore ldx_set_graph_mode."""

    def set_graph_mode(self, on: bool):
        lib.check(self._lib.ldx_set_graph_mode(self._h, int(on)), "ldx_set_graph_mode")

    def graph_stats(self):
        """(captures, replays) of the engine's hipGraph path since it was created."""
        c, r = C.c_int64(0), C.c_int64(0)
        lib.check(self._lib.ldx_graph_stats(self._h, C.byref(c), C.byref(r)), "ldx_graph_stats")
        return int(c.value), int(r.value)


class UNetEngine(_GraphMode, _Engine):
    def __init__(self, cfg: UNetConfig, state_dict, device: int = 0, dtype: str = "bf16", graph: bool = False):
        super().__init__(cfg, device)
        self.dtype = dtype
        self._create(lib.ldx_unet_config, "ldx_create", dtype, in_channels=cfg.in_channels, out_channels=cfg.out_channels, model_channels=cfg.model_channels,
                     num_levels=len(cfg.channel_mult), channel_mult=cfg.channel_mult, num_res_blocks=cfg.num_res_blocks, transformer_depth=cfg.transformer_depth,
                     transformer_depth_output=cfg.transformer_depth_output, transformer_depth_middle=cfg.transformer_depth_middle,
                     num_heads=cfg.num_heads, context_dim=cfg.context_dim)
        try:
            keep = self._load_state_dict(state_dict, strip=("model.diffusion_model.",), allow_device=True)
            self.sigmas, self.log_sigmas = sd15_sigmas()
            temb = timestep_embedding_table(self.sigmas.numel(), cfg.model_channels)
            lib.check(self._lib.ldx_set_tables(self._h, lib.ptr(self.log_sigmas), self.log_sigmas.numel(),
                                               lib.ptr(temb), temb.shape[1]), "ldx_set_tables")
            self._finalize()
            del keep
        except Exception:
            self.close()
            raise
        if graph:
            self.set_graph_mode(True)

    def refresh(self, state_dict):
        """Replace the weights in place (ldx_unet_refresh_begin / _commit) from a FULL state dict, host or device tensors as in the constructor: what the
        reference's ModelPatcher.patch_model / unpatch_model does to its modules when a LoRA changes (ModelPatcher.py:515,652).  Plans, arenas and
        captured graphs stay; the emb_layers table is rebuilt and cached context projections are dropped.  A state dict with a key missing or
        mis-shaped raises LdxError naming it and leaves the engine computing with its present weights."""
        lib.check(self._lib.ldx_unet_refresh_begin(self._h), "ldx_unet_refresh_begin")
        try:
            keep = self._load_state_dict(state_dict, strip=("model.diffusion_model.",), allow_device=True)
        except Exception:
            self._lib.ldx_unet_refresh_abort(self._h)      # forget what was registered and close the loaders again
            raise
        lib.check(self._lib.ldx_unet_refresh_commit(self._h), "ldx_unet_refresh_commit")
        del keep

    def weights_digest(self) -> int:
        """ldx_weights_digest: FNV-1a over every packed weight buffer (diagnostic: equal digests = bit-identical weights)."""
        d = C.c_uint64(0)
        lib.check(self._lib.ldx_weights_digest(self._h, C.byref(d)), "ldx_weights_digest")
        return int(d.value)

    def set_context_cache(self, on: bool = True):
        """ldx_unet_context_cache: promise that a ctx buffer's contents stay put until the next call of this method (which invalidates the cache)."""
        lib.check(self._lib.ldx_unet_context_cache(self._h, int(on)), "ldx_unet_context_cache")
        self._ctx_cached = bool(on)

    def invalidate_context(self):
        """A cached context buffer was rewritten in place: drop its projections (the mode stays as it is)."""
        self.set_context_cache(getattr(self, "_ctx_cached", False))

    def _ctx_mode(self, cached: bool):
        # every entry point states whether ITS ctx may be cached; the default is the reference's behaviour (recompute): a caller that hands over a
        # fresh tensor per step (the hook) may get the address of the previous one back from the allocator, with other contents
        if bool(cached) != getattr(self, "_ctx_cached", False):
            self.set_context_cache(cached)

    def timestep_index(self, sigma):
        """ModelSamplingDiscrete.timestep (sample/sampling.py:309-320) with the reference's own torch expression on the HOST: integer work, so it has to be
        bit-exact, and a device logf may differ from the host's log in the last bit (near-ties pick the other index).  sigma: host tensor / float."""
        return timestep_index(self.log_sigmas, sigma)

    def timestep_device(self, sigma):
        """The device's own lookup (ldx_unet_timestep): what ldx_unet_denoise runs when sigma lives on the GPU.  Returns int32 [n] on the device."""
        sg = sigma.to(device=self.device, dtype=torch.float32).contiguous().reshape(-1)
        out = torch.empty(sg.numel(), dtype=torch.int32, device=sg.device)
        lib.check(self._lib.ldx_unet_timestep(self._h, lib.ptr(sg), sg.numel(), lib.ptr(out), lib.current_stream_ptr()), "ldx_unet_timestep")
        return out

    def _ctx_arg(self, ctx, device, ctx_cached):
        """ctx as the C ABI wants it.  With the context cache on, the engine keys the cached k|v projections on the POINTER: a conversion here would hand it a
        temporary whose address the allocator gives to the next temporary too (other contents, same key) - so a cached ctx must already be in place."""
        if ctx_cached:
            assert ctx.is_cuda and ctx.dtype == torch.float32 and ctx.is_contiguous(), "ctx_cached=True needs a contiguous CUDA fp32 ctx (the cache is keyed on its address)"
            return ctx
        return ctx.to(device=device, dtype=torch.float32).contiguous()

    def _run(self, fn, x, s, ctx, out, ctx_cached=False, t_idx=None):
        self._ctx_mode(ctx_cached)
        assert x.is_cuda and x.dtype == torch.float32 and x.dim() == 4, "x must be a CUDA fp32 NCHW tensor"
        b2, ch, h, w = x.shape
        assert ch == self.cfg.in_channels
        x = x.contiguous()
        s = s.to(device=x.device, dtype=torch.float32).contiguous()
        ctx = self._ctx_arg(ctx, x.device, ctx_cached)
        assert s.numel() == b2 and ctx.dim() == 3 and ctx.shape[0] == b2 and ctx.shape[2] == self.cfg.context_dim
        if out is None:
            out = torch.empty((b2, self.cfg.out_channels, h, w), device=x.device, dtype=torch.float32)
        if t_idx is not None:
            t = t_idx.to(device=x.device, dtype=torch.float32).contiguous()
            assert t.numel() == b2
            lib.check(self._lib.ldx_unet_denoise_t(self._h, lib.ptr(x), lib.ptr(s), lib.ptr(t), lib.ptr(ctx), b2, h, w, ctx.shape[1], lib.ptr(out),
                                                   lib.current_stream_ptr()), "ldx_unet_denoise_t")
            return out
        lib.check(fn(self._h, lib.ptr(x), lib.ptr(s), lib.ptr(ctx), b2, h, w, ctx.shape[1], lib.ptr(out),
                     lib.current_stream_ptr()), fn.__name__)
        return out

    def denoise(self, x, sigma, ctx, out=None, c_concat=None, ctx_cached=False):
        """BaseModel.apply_model (ModelBase.py:72-133): x fp32 [B2,4,h,w], sigma [B2] (values), ctx [B2,M,768].
        c_concat [B2,in_channels-4,h,w] (inpainting UNets, ModelBase.py:100-101): appended unscaled behind the scaled x inside the engine's prep kernel."""
        if c_concat is None:
            # sigma on the host (the reference's CPU path, the hook's recorded calls): the timestep index comes from the reference's own torch expression
            t_idx = self.timestep_index(sigma) if (torch.is_tensor(sigma) and not sigma.is_cuda) else None
            return self._run(self._lib.ldx_unet_denoise, x, sigma, ctx, out, ctx_cached, t_idx=t_idx)
        self._ctx_mode(ctx_cached)
        assert x.is_cuda and x.dtype == torch.float32 and x.dim() == 4, "x must be a CUDA fp32 NCHW tensor"
        b2, ch, h, w = x.shape
        cc = c_concat.to(device=x.device, dtype=torch.float32).contiguous()
        assert cc.dim() == 4 and cc.shape[0] == b2 and cc.shape[2:] == x.shape[2:] and ch + cc.shape[1] == self.cfg.in_channels, "c_concat must be [B2, in_channels - C(x), h, w]"
        x = x.contiguous()
        s = sigma.to(device=x.device, dtype=torch.float32).contiguous()
        ctx = self._ctx_arg(ctx, x.device, ctx_cached)
        assert s.numel() == b2 and ctx.dim() == 3 and ctx.shape[0] == b2 and ctx.shape[2] == self.cfg.context_dim
        if out is None:
            out = torch.empty((b2, self.cfg.out_channels, h, w), device=x.device, dtype=torch.float32)
        lib.check(self._lib.ldx_unet_denoise_concat(self._h, lib.ptr(x), lib.ptr(s), lib.ptr(ctx), lib.ptr(cc), cc.shape[1], b2, h, w, ctx.shape[1],
                                                    lib.ptr(out), lib.current_stream_ptr()), "ldx_unet_denoise_concat")
        return out

    def denoise_cfg(self, x, sigma: float, ctx, out=None, ctx_cached=False):
        """One CFG evaluation (calc_cond_batch, cond.py:186-226): x fp32 [B,4,h,w] is read by both halves of the [uncond x B; cond x B]
        batch, sigma is one scalar, ctx [2B,M,768]; returns [2B,4,h,w].  No torch kernel runs: the broadcast of x and sigma happens in
        the engine's own boundary kernels (ldx_unet_denoise_cfg)."""
        self._ctx_mode(ctx_cached)
        assert x.is_cuda and x.dtype == torch.float32 and x.dim() == 4 and x.is_contiguous(), "x must be a contiguous CUDA fp32 NCHW tensor"
        b, ch, h, w = x.shape
        assert ch == self.cfg.in_channels
        assert ctx.is_cuda and ctx.dtype == torch.float32 and ctx.is_contiguous() and ctx.dim() == 3 and ctx.shape[0] == 2 * b and ctx.shape[2] == self.cfg.context_dim
        if out is None:
            out = torch.empty((2 * b, self.cfg.out_channels, h, w), device=x.device, dtype=torch.float32)
        # sigma is a host scalar here: its timestep index is computed with the reference's own torch ops (bit-exact by construction, see timestep_index)
        t_index = int(self.timestep_index(float(sigma))[0])
        lib.check(self._lib.ldx_unet_denoise_cfg_t(self._h, lib.ptr(x), float(sigma), t_index, lib.ptr(ctx), b, h, w, ctx.shape[1], lib.ptr(out),
                                                   lib.current_stream_ptr()), "ldx_unet_denoise_cfg_t")
        return out

    def forward(self, x, timesteps, ctx, out=None):
        """UNetModel1.forward (unet.py:679-770): integer timesteps (as floats), unscaled input."""
        return self._run(self._lib.ldx_unet_forward, x, timesteps, ctx, out)

    def set_cfg_share(self, mode=True):
        """ldx_unet_cfg_share: denoise_cfg computes the part of the UNet in front of the first cross-attention once for both CFG halves.
        False / 0: never; True / 1 (default): where it pays (>= 8192 rows per half); 2: whenever possible (tests on small latents)."""
        lib.check(self._lib.ldx_unet_cfg_share(self._h, int(mode)), "ldx_unet_cfg_share")


class VAEDecoderEngine(_Engine):
    """VAE.decode (src/AutoEncoders/VariationalAE.py:690-722): latent (already / 0.18215) -> NHWC fp32 in [0, 1]."""

    def __init__(self, cfg: VAEConfig, state_dict, device: int = 0, dtype: str = "bf16"):
        super().__init__(cfg, device)
        self._create(lib.ldx_vae_config, "ldx_vae_create", dtype, z_channels=cfg.z_channels, ch=cfg.ch, num_levels=len(cfg.ch_mult), ch_mult=cfg.ch_mult,
                     num_res_blocks=cfg.num_res_blocks, out_ch=cfg.out_ch, use_post_quant=cfg.use_post_quant)
        self._load_state_dict(state_dict, strip=("first_stage_model.",))
        self._finalize()

    def decode(self, z):
        assert z.is_cuda and z.dtype == torch.float32 and z.dim() == 4
        b, _, h, w = z.shape
        out = torch.empty((b, 8 * h, 8 * w, self.cfg.out_ch), device=z.device, dtype=torch.float32)
        lib.check(self._lib.ldx_vae_decode(self._h, lib.ptr(z.contiguous()), b, h, w, lib.ptr(out), lib.current_stream_ptr()),
                  "ldx_vae_decode")
        return out

    def encode_moments(self, pixels):
        """Deterministic part of VAE.encode (VariationalAE.py:725-760): pixels [B,H,W,3] fp32 in [0,1] ->
        moments [B, 2*z, H/8, W/8] (mean | logvar).  Needs encoder.* / quant_conv.* in the state dict."""
        assert pixels.is_cuda and pixels.dtype == torch.float32 and pixels.dim() == 4 and pixels.shape[-1] == 3
        b, h, w, _ = pixels.shape
        f = 2 ** (len(self.cfg.ch_mult) - 1)
        out = torch.empty((b, 2 * self.cfg.z_channels, h // f, w // f), device=pixels.device, dtype=torch.float32)
        lib.check(self._lib.ldx_vae_encode(self._h, lib.ptr(pixels.contiguous()), b, h, w, lib.ptr(out), lib.current_stream_ptr()),
                  "ldx_vae_encode")
        return out

    def encode(self, pixels):
        """VAE.encode (VariationalAE.py:725-760).  vae_encode_crop_pixels (:677-688) computes the cropped sizes and
        throws them away, so nothing is cropped: every Downsample floors.  Then DiagonalGaussianDistribution.sample
        (:42-51) — torch.randn(mean.shape) from the *global CPU RNG* exactly as the reference draws it, uploaded."""
        mom = self.encode_moments(pixels[..., :3].to(self.device, torch.float32))
        mean, logvar = torch.chunk(mom, 2, dim=1)
        eps = torch.randn(mean.shape).to(self.device)
        return mean + torch.exp(0.5 * torch.clamp(logvar, -30.0, 20.0)) * eps


def _bislerp_data(length_old: int, length_new: int):
    """generate_bilinear_data (src/Utilities/upscale.py:61-97): the reference builds the index / ratio arrays with
    F.interpolate(mode="bilinear") of an arange; reproduced verbatim on the host (length_new floats)."""
    c1 = torch.arange(length_old, dtype=torch.float32).reshape(1, 1, 1, -1)
    c1 = torch.nn.functional.interpolate(c1, size=(1, length_new), mode="bilinear")
    ratios = (c1 - c1.floor()).reshape(-1)
    c2 = torch.arange(length_old, dtype=torch.float32).reshape(1, 1, 1, -1) + 1
    c2[:, :, :, -1] -= 1
    c2 = torch.nn.functional.interpolate(c2, size=(1, length_new), mode="bilinear")
    return ratios.contiguous(), c1.reshape(-1).to(torch.int32), c2.reshape(-1).to(torch.int32)


def bislerp(samples, width: int, height: int):
    """bislerp (src/Utilities/upscale.py:5-128) = LatentUpscale.upscale's resampler (HiresFix, pipeline.py:346-350):
    a slerp pass along W then one along H, each one ldx_bislerp_pass launch on fp32 NCHW device tensors."""
    assert samples.is_cuda and samples.dim() == 4
    L = lib.load()
    x = samples.float().contiguous()
    n, c, h, w = x.shape
    dev = x.device
    r, c1, c2 = (t.to(dev) for t in _bislerp_data(w, width))
    y = torch.empty((n, c, h, width), device=dev, dtype=torch.float32)
    lib.check(L.ldx_bislerp_pass(lib.ptr(x), lib.ptr(y), n, c, h, w, 1, width, lib.ptr(c1), lib.ptr(c2), lib.ptr(r),
                                 lib.current_stream_ptr()), "ldx_bislerp_pass")
    r2, d1, d2 = (t.to(dev) for t in _bislerp_data(h, height))
    z = torch.empty((n, c, height, width), device=dev, dtype=torch.float32)
    lib.check(L.ldx_bislerp_pass(lib.ptr(y), lib.ptr(z), n, c, h, width, 0, height, lib.ptr(d1), lib.ptr(d2), lib.ptr(r2),
                                 lib.current_stream_ptr()), "ldx_bislerp_pass")
    return z.to(samples.dtype)


def latent_upscale(samples, width: int, height: int):
    """LatentUpscale.upscale (upscale.py:149-166): target latent size = pixel size // 8."""
    return bislerp(samples, width // 8, height // 8)


class CLIPTextEngine(_Engine):
    """CLIPTextModel_.forward (src/clip/CLIPTextModel.py:51-107) + the token-weight logic of
    ClipTokenWeightEncoder.encode_token_weights (src/SD15/SDClip.py:36-97) on the host."""

    def __init__(self, cfg: CLIPConfig, state_dict, device: int = 0, dtype: str = "bf16"):
        super().__init__(cfg, device)
        self._create(lib.ldx_clip_config, "ldx_clip_create", dtype, hidden_size=cfg.hidden_size, num_layers=cfg.num_layers, num_heads=cfg.num_heads,
                     intermediate_size=cfg.intermediate_size, max_positions=cfg.max_positions, vocab_size=cfg.vocab_size)
        self._load_state_dict(state_dict, strip=("text_model.",))       # incl. the optional "text_projection.weight"
        self._finalize()
        self._tok_dtype = next(v.dtype for k, v in state_dict.items() if k.endswith("embeddings.token_embedding.weight"))

    def forward(self, tokens, intermediate_output=None):
        """tokens: int tensor [B][T] -> (last [B,T,E] after final LN, intermediate (final-LN'd) or None, pooled)."""
        ids = tokens.to(self.device, torch.int32).contiguous()
        b, t = ids.shape
        last = torch.empty((b, t, self.cfg.hidden_size), device=self.device, dtype=torch.float32)
        inter = torch.empty_like(last) if intermediate_output is not None else None
        lib.check(self._lib.ldx_clip_encode(self._h, lib.ptr(ids), b, t, int(intermediate_output or 0), lib.ptr(last),
                                            lib.ptr(inter), lib.current_stream_ptr()), "ldx_clip_encode")
        # pooled output: row at argmax(tokens == eos_token_id) (CLIPTextModel.py:98-106; eos id 2 -> position 0 quirk), then the optional
        # text_projection (CLIPTextModel.py:152-163) — both inside the engine (ldx_clip_pooled), no torch kernel
        pooled = torch.empty((b, self.cfg.hidden_size), device=self.device, dtype=torch.float32)
        lib.check(self._lib.ldx_clip_pooled(self._h, lib.ptr(last), lib.ptr(ids), b, t, int(self.cfg.eos_token_id), lib.ptr(pooled),
                                            lib.current_stream_ptr()), "ldx_clip_pooled")
        return last, inter, pooled

    _extra_rows = 0

    def _textual_embeddings(self, chunks, pad_token):
        """SDClipModel.set_up_textual_embeddings (SDClip.py:213-267): a token that is a vector of the model's width becomes
        the id vocab_size + k of an appended table row; a vector of another width is dropped and the chunk re-padded."""
        e, nxt, rows, out = self.cfg.hidden_size, self.cfg.vocab_size, [], []
        for chunk in chunks:
            ids = []
            for t in chunk:
                if isinstance(t, numbers.Integral):
                    ids.append(int(t))
                elif t.shape[0] == e:
                    rows.append(torch.as_tensor(t)); ids.append(nxt); nxt += 1
            ids += [pad_token] * (len(chunk) - len(ids))
            out.append(ids)
        return out, rows

    def encode_token_weights(self, token_weight_pairs, layer_idx=-2, special_tokens=(49406, 49407, 49407)):
        """ClipTokenWeightEncoder.encode_token_weights (SDClip.py:36-97) for a list of 77-token (id, weight) chunks; an id
        may be a textual-inversion vector (prompt.tokenize_with_weights with embeddings=...)."""
        start, end, pad = special_tokens

        def encode(to_encode):
            to_encode, extra = self._textual_embeddings(to_encode, pad)
            if extra or self._extra_rows:
                # the reference copies the vectors into a table of the stored weights' dtype (SDClip.py:249-258): same rounding here
                rows = torch.stack(extra).to(self._tok_dtype).float().contiguous() if extra else None
                lib.check(self._lib.ldx_clip_set_extra_embeddings(self._h, None if rows is None else C.c_void_p(rows.data_ptr()), len(extra)),
                          "ldx_clip_set_extra_embeddings")
                self._extra_rows = len(extra)
            last, inter, pooled = self.forward(torch.tensor(to_encode, dtype=torch.int64), intermediate_output=layer_idx)
            return (inter if layer_idx is not None else last).float().cpu(), pooled[0:1].float().cpu()

        return _encode_token_weights(token_weight_pairs, lambda n: [start, end] + [pad] * (n - 2), encode)


class ESRGANEngine(_Engine):
    """RRDBNet.forward (src/UltimateSDUpscale/RDRB.py:216-471) + tiled_scale (src/Utilities/util.py:406-640) as
    UpscaleModelLoader / ImageUpscaleWithModel use them (USDU_upscaler.py:48-96)."""

    def __init__(self, cfg, state_dict, device: int = 0, dtype: str = "bf16"):
        from .weights import esrgan_new_to_old_arch
        super().__init__(cfg, device)
        self._create(lib.ldx_esrgan_config, "ldx_esrgan_create", dtype, in_nc=cfg.in_nc, out_nc=cfg.out_nc, nf=cfg.nf, gc=cfg.gc, num_blocks=cfg.num_blocks,
                     num_upscale=math.log2(cfg.scale))
        self._load_state_dict(esrgan_new_to_old_arch(state_dict))
        self._finalize()

    def forward(self, pixels):
        """pixels [B,H,W,in_nc] fp32 (device) -> [B, s*H, s*W, out_nc] fp32."""
        assert pixels.is_cuda and pixels.dtype == torch.float32 and pixels.dim() == 4
        b, h, w, _ = pixels.shape
        s = self.cfg.scale
        out = torch.empty((b, s * h, s * w, self.cfg.out_nc), device=pixels.device, dtype=torch.float32)
        lib.check(self._lib.ldx_esrgan_forward(self._h, lib.ptr(pixels.contiguous()), b, h, w, lib.ptr(out), lib.current_stream_ptr()),
                  "ldx_esrgan_forward")
        return out

    def upscale(self, image, tile: int = 512, overlap: int = 32):
        """ImageUpscaleWithModel.upscale (USDU_upscaler.py:48-96): tiled_scale(tile 512, overlap 32) then clamp to [0, 1].
        image [B,H,W,3] fp32 in [0,1] (any device) -> [B, sH, sW, 3] on the engine's device.  Tile positions, the
        single-tile shortcut and the feather mask follow tiled_scale_multidim (util.py:406-600) exactly."""
        L, s = self._lib, self.cfg.scale
        image = image.to(self.device, torch.float32).contiguous()
        b, h, w, c = image.shape
        outs = []
        for bi in range(b):
            img = image[bi:bi + 1]
            if h <= tile and w <= tile:
                out = self.forward(img)
                lib.check(L.ldx_tile_finish(lib.ptr(out), None, out.numel(), 1, lib.current_stream_ptr()), "ldx_tile_finish")
                outs.append(out)
                continue
            out = torch.zeros((1, s * h, s * w, self.cfg.out_nc), device=self.device, dtype=torch.float32)
            div = torch.zeros_like(out)
            ys = range(0, h - overlap, tile - overlap) if h > tile else [0]
            xs = range(0, w - overlap, tile - overlap) if w > tile else [0]
            for y in ys:
                for x in xs:
                    py, px = max(0, min(h - overlap, y)), max(0, min(w - overlap, x))
                    ly, lx = min(tile, h - py), min(tile, w - px)
                    ps = self.forward(img[:, py:py + ly, px:px + lx, :].contiguous())
                    lib.check(L.ldx_tile_blend(lib.ptr(ps), s * ly, s * lx, lib.ptr(out), lib.ptr(div), s * h, s * w, self.cfg.out_nc,
                                               round(s * py), round(s * px), round(s * overlap), lib.current_stream_ptr()), "ldx_tile_blend")
            lib.check(L.ldx_tile_finish(lib.ptr(out), lib.ptr(div), out.numel(), 1, lib.current_stream_ptr()), "ldx_tile_finish")
            outs.append(out)
        return torch.cat(outs, 0)


class TAESDEngine(_GraphMode, _Engine):
    """The tiny autoencoder's decoder (src/AutoEncoders/taesd.py): TAESD.decode and the tensor part of taesd_preview, the sampler loops' latent preview.
    state_dict: Decoder2's own keys (weights.taesd_decoder_state_dict_spec; include/vae_approx/taesd_decoder.safetensors as it is).
    graph=True: the 36 launches of a shape are captured into a hipGraph on the second call and replayed from the third.  A captured graph has its pointers
    baked in, so in graph mode the engine keeps one latent buffer and one output buffer per (shape, output, flux), copies the latent in and returns a copy
    of the result (3 MB of bytes for a 1024^2 preview)."""

    def __init__(self, cfg=None, state_dict=None, device: int = 0, dtype: str = "bf16", graph: bool = False):
        from .weights import TAESDConfig
        cfg = cfg or TAESDConfig()
        super().__init__(cfg, device)
        self._create(lib.ldx_taesd_config, "ldx_taesd_create", dtype, latent_channels=cfg.latent_channels)
        self._load_state_dict(state_dict, strip=("taesd_decoder.",))
        self._finalize()
        self.set_graph_mode(graph)

    def set_graph_mode(self, on: bool):
        super().set_graph_mode(on)
        self._graph, self._static = bool(on), {}          # buffers kept for another mode's calls are dropped

    def _latent(self, x):
        """taesd_preview's channel rule (taesd.py:268-277): more than 4 channels are cut, fewer are zero-padded."""
        assert x.dim() == 4
        x = x.to(self.device, torch.float32)
        c = x.shape[1]
        if c > 4:
            x = x[:, :4]
        elif c < 4:
            x = torch.cat([x, x.new_zeros((x.shape[0], 4 - c) + tuple(x.shape[2:]))], dim=1)
        return x.contiguous()

    def _decode(self, x, want_f32, want_u8, flux):
        b, _, h, w = x.shape

        def buffers():
            f32 = torch.empty((b, 3, 8 * h, 8 * w), device=self.device, dtype=torch.float32) if want_f32 else None
            u8 = torch.empty((b, 8 * h, 8 * w, 3), device=self.device, dtype=torch.uint8) if want_u8 else None
            return f32, u8
        if not self._graph:
            f32, u8 = buffers()
        else:
            key = (b, h, w, want_f32, want_u8, bool(flux))
            if key not in self._static:
                if len(self._static) >= 4:
                    self._static.clear()
                self._static[key] = (torch.empty_like(x),) + buffers()
            xs, f32, u8 = self._static[key]
            xs.copy_(x)
            x = xs
        lib.check(self._lib.ldx_taesd_decode(self._h, lib.ptr(x), b, h, w, lib.ptr(f32), lib.ptr(u8), int(bool(flux)), lib.current_stream_ptr()), "ldx_taesd_decode")
        if self._graph:
            f32, u8 = (None if f32 is None else f32.clone()), (None if u8 is None else u8.clone())
        return f32, u8

    def decode(self, x):
        """TAESD.decode (taesd.py:224-237; vae_shift 0, vae_scale 1): latent [B,4,h,w] -> [B,3,8h,8w] fp32 = (decoder(x) - 0.5) * 2."""
        assert x.shape[1] == 4, "TAESD.decode takes 4 latent channels (preview() cuts or pads)"
        return self._decode(self._latent(x), True, False, False)[0]

    def preview(self, x, flux: bool = False):
        """The tensor part of taesd_preview (taesd.py:264-304): latent [B,C,h,w] -> device uint8 [B,8h,8w,3], the bytes the reference hands to PIL."""
        return self._decode(self._latent(x), False, True, flux)[1]


class SAMImageEncoderEngine(_GraphMode, _Engine):
    """segment_anything's image encoder (ImageEncoderViT; the reference's SAM.py loads ViT-B): the network behind ADetailer's masks, once per image.
    state_dict: segment_anything's own keys, with or without "image_encoder." (weights.sam_encoder_state_dict_spec); a whole Sam checkpoint may be passed,
    the prompt encoder's and mask decoder's tensors are left out.
    graph=True: the launches of a batch size are captured into a hipGraph on the second call and replayed from the third.  A captured graph has its
    pointers baked in, so in graph mode the engine keeps one input and one output buffer per batch size and returns a copy of the result."""

    def __init__(self, cfg=None, state_dict=None, device: int = 0, dtype: str = "bf16", graph: bool = False):
        from .weights import SAMConfig
        cfg = cfg or SAMConfig.vit_b()
        super().__init__(cfg, device)
        self.dtype = dtype
        self._create(lib.ldx_sam_config, "ldx_sam_create", dtype, image_size=cfg.image_size, embed_dim=cfg.embed_dim, depth=cfg.depth, num_heads=cfg.num_heads,
                     mlp_dim=cfg.mlp_dim, out_chans=cfg.out_chans, window_size=cfg.window_size, global_attn_mask=cfg.global_attn_mask)
        try:
            other = ("prompt_encoder.", "mask_decoder.", "pixel_mean", "pixel_std")
            self._load_state_dict({k: v for k, v in state_dict.items() if not k.startswith(other)}, strip=("image_encoder.",))
            self._finalize()
        except Exception:
            self.close()
            raise
        self._ops = None
        self.set_graph_mode(graph)

    def set_graph_mode(self, on: bool):
        super().set_graph_mode(on)
        self._graph, self._static = bool(on), {}

    def encode(self, x):
        """ImageEncoderViT.forward: the preprocessed image(s) [B,3,size,size] -> fp32 [B,out_chans,size/16,size/16] on the device."""
        cfg = self.cfg
        assert x.dim() == 4 and tuple(x.shape[1:]) == (3, cfg.image_size, cfg.image_size), tuple(x.shape)
        x = x.to(self.device, torch.float32).contiguous()
        b = x.shape[0]
        if not self._graph:
            out = torch.empty((b, cfg.out_chans, cfg.grid, cfg.grid), device=self.device, dtype=torch.float32)
        else:
            if b not in self._static:
                if len(self._static) >= 4:
                    self._static.clear()
                self._static[b] = (torch.empty_like(x), torch.empty((b, cfg.out_chans, cfg.grid, cfg.grid), device=self.device, dtype=torch.float32))
            xs, out = self._static[b]
            xs.copy_(x)
            x = xs
        lib.check(self._lib.ldx_sam_encode(self._h, lib.ptr(x), b, lib.ptr(out), lib.current_stream_ptr()), "ldx_sam_encode")
        return out.clone() if self._graph else out

    def preprocess(self, image):
        """What SamPredictor.set_image does to an image in front of the encoder, on the device: image fp32 [1,H,W,3] or [H,W,3] in [0, 1] (quantised as
        make_sam_mask does, SAM.py:225: clip, times 255, truncate) or uint8 -> longest side to image_size with Pillow's 8-bit BILINEAR
        (ResizeLongestSide.apply_image) -> Sam.preprocess.  Returns fp32 [1,3,size,size]."""
        from .sam import preprocess_shape
        from .usdu import BILINEAR, ImageOps, _Image
        if self._ops is None:
            self._ops = ImageOps()
            self._ops._init_ops(self.device)
        if image.dim() == 3:
            image = image[None]
        assert image.dim() == 4 and image.shape[0] == 1 and image.shape[3] == 3, tuple(image.shape)
        _, h, w, _ = image.shape
        size = self.cfg.image_size
        if image.dtype == torch.uint8:
            img = _Image(h, w, 3, self.device)
            img.view().copy_(image[0].to(self.device))
        else:
            img = self._ops._quantize(image)
        nh, nw = preprocess_shape(h, w, size)
        if (nh, nw) != (h, w):
            img = self._ops._resize(img, None, nw, nh, BILINEAR)
        x = torch.empty((1, 3, size, size), device=self.device, dtype=torch.float32)
        lib.check(self._lib.ldx_sam_preprocess(img.ptr(), img.pitch, nh, nw, lib.ptr(x), size, lib.current_stream_ptr()), "ldx_sam_preprocess")
        return x

    def set_image(self, image):
        """preprocess + encode: the image embedding fp32 [1,out_chans,size/16,size/16] of what the pipeline holds on the device."""
        return self.encode(self.preprocess(image))


class SAMMaskDecoderEngine(_GraphMode, _Engine):
    """segment_anything's prompt encoder and mask decoder (the same for ViT-B, ViT-L and ViT-H) and Sam.postprocess_masks, in fp32 on the device: what
    SamPredictor.predict runs behind the image encoder, for P prompts of one image at once.  state_dict: segment_anything's own keys (prompt_encoder.*,
    mask_decoder.*; weights.sam_decoder_state_dict_spec); a whole Sam checkpoint may be passed, image_encoder.*, pixel_* and the mask prompt's
    mask_downscaling are left out.  Mask prompts and the single-mask output are not built.
    graph=True: predict's launches are captured per (P, n, box or not) on the second call and replayed from the third; the engine then keeps its own
    prompt and result buffers per shape and returns copies of the results."""

    def __init__(self, cfg=None, state_dict=None, device: int = 0, graph: bool = False):
        from .weights import SAMDecoderConfig, sam_decoder_state_dict_spec
        cfg = cfg or SAMDecoderConfig.vit_b()
        super().__init__(cfg, device)
        self._create(lib.ldx_samdec_config, "ldx_samdec_create", "bf16", image_size=cfg.image_size, hidden=cfg.hidden, num_heads=cfg.num_heads, mlp_dim=cfg.mlp_dim,
                     iou_head_hidden=cfg.iou_head_hidden, depth=cfg.depth, num_multimask=cfg.num_multimask)
        try:
            keys = {k for k, _ in sam_decoder_state_dict_spec(cfg)}
            self._load_state_dict({k: v.float() for k, v in (state_dict or {}).items() if k in keys})
            self._finalize()
        except Exception:
            self.close()
            raise
        self.set_graph_mode(graph)

    def set_graph_mode(self, on: bool):
        super().set_graph_mode(on)
        self._graph, self._static = bool(on), {}

    def set_image(self, embedding):
        """The image encoder's output [1,C,g,g] or [C,g,g] (SAMImageEncoderEngine.encode): the per-image part of the decoder, once per image."""
        cfg = self.cfg
        e = embedding[0] if embedding.dim() == 4 else embedding
        assert tuple(e.shape) == (cfg.hidden, cfg.grid, cfg.grid), tuple(embedding.shape)
        e = e.to(self.device, torch.float32).contiguous()
        lib.check(self._lib.ldx_samdec_set_image(self._h, lib.ptr(e), lib.current_stream_ptr()), "ldx_samdec_set_image")

    def _prompts(self, points, labels, boxes, original_size):
        """Host prompts in the original image's frame -> (points [P,n,2] | None, labels int32 | None, boxes [P,4] | None, P, n) in the resized frame, fp32 as
        SamPredictor hands them to the model.  original_size None: they are in the resized frame already."""
        import numpy as np
        from .sam import apply_boxes_host, apply_coords_host
        size = self.cfg.image_size
        pts = lab = box = None
        if points is not None:
            pts = np.asarray(points, dtype=np.float64)
            pts = pts.reshape((1,) + pts.shape) if pts.ndim == 2 else pts
            lab = np.asarray(labels, dtype=np.int32).reshape(pts.shape[:2])
            if original_size is not None:
                pts = apply_coords_host(pts, original_size, size)
            pts, lab = torch.from_numpy(pts.astype(np.float32)), torch.from_numpy(lab)
        if boxes is not None:
            box = np.asarray(boxes, dtype=np.float64).reshape(-1, 4)
            if original_size is not None:
                box = apply_boxes_host(box, original_size, size)
            box = torch.from_numpy(box.astype(np.float32))
        if pts is None and box is None:
            raise ValueError("SAMMaskDecoderEngine.predict: neither points nor boxes")
        P = pts.shape[0] if pts is not None else box.shape[0]
        if pts is not None and box is not None and box.shape[0] != P:
            raise ValueError("SAMMaskDecoderEngine.predict: points and boxes of different prompt counts")
        return pts, lab, box, P, 0 if pts is None else pts.shape[1]

    def _buffers(self, pts, lab, box, P, n):
        cfg, dev = self.cfg, self.device
        key = (P, n, box is not None)
        if self._graph and key in self._static:
            bufs = self._static[key]
        else:
            bufs = (None if pts is None else torch.empty((P, n, 2), device=dev, dtype=torch.float32), None if pts is None else torch.empty((P, n), device=dev, dtype=torch.int32),
                    None if box is None else torch.empty((P, 4), device=dev, dtype=torch.float32),
                    torch.empty((P, 4, 4 * cfg.grid, 4 * cfg.grid), device=dev, dtype=torch.float32), torch.empty((P, 4), device=dev, dtype=torch.float32))
            if self._graph:
                if len(self._static) >= 8:
                    self._static.clear()
                self._static[key] = bufs
        for dst, src in zip(bufs[:3], (pts, lab, box)):
            if dst is not None:
                dst.copy_(src)
        return bufs

    def predict(self, points=None, labels=None, boxes=None, original_size=None):
        """SamPredictor.predict with its defaults (multimask_output=True, no mask prompt) for P prompts at once: points [P][n][2] (or [n][2]) with labels, and /
        or boxes [P][4], in the original image's frame (original_size = (H, W); None: already in the resized frame).  Returns (low-res logits [P,3,4g,4g],
        IoU predictions [P,3]) on the device: the three multimask outputs."""
        pts, lab, box, P, n = self._prompts(points, labels, boxes, original_size)
        dp, dl, db, lowres, iou = self._buffers(pts, lab, box, P, n)
        lib.check(self._lib.ldx_samdec_predict(self._h, lib.ptr(dp), lib.ptr(dl), n, lib.ptr(db), P, lib.ptr(lowres), lib.ptr(iou), lib.current_stream_ptr()), "ldx_samdec_predict")
        lowres, iou = lowres[:, 1:], iou[:, 1:]
        return (lowres.clone(), iou.clone()) if self._graph else (lowres, iou)

    def prompt_tokens(self, points=None, labels=None, boxes=None, original_size=None):
        """Test surface: the decoder's input tokens [P, 5 + ns, C] (iou_token | mask_tokens | prompt encodings)."""
        pts, lab, box, P, n = self._prompts(points, labels, boxes, original_size)
        dev = self.device
        dp, dl, db = (None if t is None else t.to(dev) for t in (pts, lab, box))
        out = torch.empty((P, 5 + n + (2 if box is not None else 1), self.cfg.hidden), device=dev, dtype=torch.float32)
        lib.check(self._lib.ldx_samdec_prompt_tokens(self._h, lib.ptr(dp), lib.ptr(dl), n, lib.ptr(db), P, lib.ptr(out), lib.current_stream_ptr()), "ldx_samdec_prompt_tokens")
        return out

    def masks(self, lowres, original_size, return_logits: bool = False):
        """Sam.postprocess_masks + threshold: low-res logits [..,L,L] -> uint8 0/1 masks [..,H,W] on the device (and the fp32 logits at that size on request).
        One launch; the image_size-square intermediate is never stored."""
        from .sam import preprocess_shape
        H, W = int(original_size[0]), int(original_size[1])
        L = lowres.shape[-1]
        lead = tuple(lowres.shape[:-2])
        x = lowres.to(self.device, torch.float32).reshape(-1, L, L).contiguous()
        n = x.shape[0]
        in_h, in_w = preprocess_shape(H, W, self.cfg.image_size)
        mask = torch.empty((n, H, W), device=self.device, dtype=torch.uint8)
        logits = torch.empty((n, H, W), device=self.device, dtype=torch.float32) if return_logits else None
        lib.check(self._lib.ldx_samdec_postprocess(lib.ptr(x), n, L, in_h, in_w, H, W, lib.ptr(mask), lib.ptr(logits), self.cfg.image_size, lib.current_stream_ptr()),
                  "ldx_samdec_postprocess")
        mask = mask.reshape(lead + (H, W))
        return (mask, logits.reshape(lead + (H, W))) if return_logits else mask


def t5_relative_position_bucket(relative_position, num_buckets=32, max_distance=128):
    """T5Attention._relative_position_bucket, bidirectional (src/clip/FluxClip.py:152-205) — same torch ops in the same
    order, so bucket boundaries (float32 log) agree bit for bit with the reference."""
    import math as _m
    num_buckets //= 2
    relative_buckets = (relative_position > 0).to(torch.long) * num_buckets
    relative_position = torch.abs(relative_position)
    max_exact = num_buckets // 2
    is_small = relative_position < max_exact
    large = max_exact + (torch.log(relative_position.float() / max_exact) / _m.log(max_distance / max_exact)
                         * (num_buckets - max_exact)).to(torch.long)
    large = torch.min(large, torch.full_like(large, num_buckets - 1))
    return relative_buckets + torch.where(is_small, relative_position, large)


def t5_bias_table(rel_bias_weight, length: int, num_buckets=32, max_distance=128):
    """T5Attention.compute_bias (FluxClip.py:207-243) -> fp32 [H][L][Lp], Lp = L rounded up to 64 (zero padded): the
    layout ldx_t5_encode reads."""
    ctx = torch.arange(length, dtype=torch.long)[:, None]
    mem = torch.arange(length, dtype=torch.long)[None, :]
    bucket = t5_relative_position_bucket(mem - ctx, num_buckets, max_distance)           # [L, L]
    vals = rel_bias_weight.float()[bucket].permute(2, 0, 1).contiguous()                 # [H, L, L]
    lp = (length + 63) // 64 * 64
    out = torch.zeros((vals.shape[0], length, lp), dtype=torch.float32)
    out[:, :, :length] = vals
    return out


class T5Engine(_Engine):
    """T5.forward (src/clip/FluxClip.py:441-519): token ids -> final_layer_norm(encoder output), fp32.  Host side keeps
    the 32 x heads relative-attention embedding and builds the bias table per sequence length (cached)."""

    def __init__(self, cfg, state_dict, device: int = 0, dtype: str = "bf16", device_weights: bool = True):
        """state_dict: dense torch tensors, or gguf.GGUFTensor values (gguf.gguf_t5_state_dict; device_weights: _load_gguf_tensors)."""
        super().__init__(cfg, device)
        self._create(lib.ldx_t5_config, "ldx_t5_create", dtype, d_model=cfg.d_model, d_ff=cfg.d_ff, num_layers=cfg.num_layers, num_heads=cfg.num_heads,
                     vocab_size=cfg.vocab_size)
        rk = "encoder.block.0.layer.0.SelfAttention.relative_attention_bias.weight"
        rel = state_dict[rk]
        self._rel = (rel.dequantize() if hasattr(rel, "dequantize") else rel).float().cpu()      # the bias table stays with the host
        keep = self._load_any({k: v for k, v in state_dict.items() if k != rk}, strip=("t5xxl.transformer.",), device_weights=device_weights)
        self._finalize()
        del keep
        self._bias = {}

    @classmethod
    def from_gguf(cls, path, cfg=None, device: int = 0, dtype: str = "bf16", device_weights: bool = True):
        """The reference's t5-v1_1-xxl-encoder-Q8_0.gguf (DualCLIPLoaderGGUF, pipeline.py:218-236); cfg=None: T5-XXL."""
        from .gguf import gguf_t5_state_dict
        cfg = cfg or T5Config()
        return cls(cfg, gguf_t5_state_dict(path, cfg.num_layers), device=device, dtype=dtype, device_weights=device_weights)

    def bias(self, length: int):
        if length not in self._bias:
            self._bias[length] = t5_bias_table(self._rel, length, self.cfg.num_buckets, self.cfg.max_distance).to(self.device)
        return self._bias[length]

    def forward(self, tokens):
        """tokens: int tensor [B][L] -> [B, L, d_model] fp32."""
        ids = tokens.to(self.device, torch.int32).contiguous()
        b, l = ids.shape
        out = torch.empty((b, l, self.cfg.d_model), device=self.device, dtype=torch.float32)
        lib.check(self._lib.ldx_t5_encode(self._h, lib.ptr(ids), b, l, lib.ptr(self.bias(l)), lib.ptr(out), lib.current_stream_ptr()),
                  "ldx_t5_encode")
        return out

    def encode_token_weights(self, token_weight_pairs):
        """ClipTokenWeightEncoder.encode_token_weights (SDClip.py:36-97) as T5XXLModel runs it (FluxClip.py:521-545):
        special tokens {end: 1, pad: 0}, layer "last", no pooled output.  Returns (cond [1, sum L, d_model], None)."""
        return _encode_token_weights(token_weight_pairs, lambda n: [1] + [0] * (n - 1),
                                     lambda chunks: (self.forward(torch.tensor(chunks, dtype=torch.int64)).float().cpu(), None))


def flux_rope_tables(cfg: FluxConfig, batch_txt_len: int, h: int, w: int):
    """pe for ids = [txt_ids (zeros) ; img_ids] exactly as Flux3.forward + EmbedND + rope() build it
    (src/BlackForest/Flux.py:36-70, 96-103, 750-771): returns (cos, sin) fp32 [Lt + (h/2)(w/2)][head_dim/2]."""
    h_len, w_len = (h + 1) // 2, (w + 1) // 2
    img_ids = torch.zeros((h_len, w_len, 3), dtype=torch.float32)
    img_ids[..., 1] = img_ids[..., 1] + torch.linspace(0, h_len - 1, steps=h_len, dtype=torch.float32)[:, None]
    img_ids[..., 2] = img_ids[..., 2] + torch.linspace(0, w_len - 1, steps=w_len, dtype=torch.float32)[None, :]
    ids = torch.cat([torch.zeros((batch_txt_len, 3), dtype=torch.float32), img_ids.reshape(-1, 3)], dim=0)
    cos, sin = [], []
    for i, dim in enumerate(cfg.axes_dim):
        scale = torch.linspace(0, (dim - 2) / dim, steps=dim // 2, dtype=torch.float64)
        omega = 1.0 / (cfg.theta ** scale)
        out = torch.einsum("n,d->nd", ids[:, i].to(torch.float32), omega)          # float32 x float64 -> float64, as rope()
        cos.append(torch.cos(out).to(torch.float32)); sin.append(torch.sin(out).to(torch.float32))
    return torch.cat(cos, dim=-1).contiguous(), torch.cat(sin, dim=-1).contiguous()


class FluxEngine(_Engine):
    """Flux3.forward behind BaseModel.apply_model with CONST prediction."""

    def __init__(self, cfg: FluxConfig, state_dict, device: int = 0, dtype: str = "bf16", fp8: bool = False, device_weights: bool = True):
        """state_dict: dense torch tensors, or gguf.GGUFTensor values (gguf.gguf_state_dict; device_weights: _load_gguf_tensors).
        fp8=True (or "linears"): the block linears (and the adaLN modulation projections) run on MX fp8 operands, attention in 16 bit (ldx_flux_set_fp8 mode 1;
        approximate, opt-in, own parity class).  fp8="attn": explicit opt-in to the less precise full mode (mode 3): at head dim 128 QK^T / PV of the joint attention run on MX fp8 too."""
        super().__init__(cfg, device)
        self._create(lib.ldx_flux_config, "ldx_flux_create", dtype, in_channels=cfg.in_channels, vec_in_dim=cfg.vec_in_dim, context_in_dim=cfg.context_in_dim,
                     hidden_size=cfg.hidden_size, mlp_hidden=cfg.mlp_hidden, num_heads=cfg.num_heads, depth=cfg.depth, depth_single=cfg.depth_single_blocks,
                     guidance_embed=cfg.guidance_embed)
        if fp8:
            assert fp8 in (True, "linears", "attn"), "fp8 must be False, True / 'linears', or 'attn'"
            lib.check(self._lib.ldx_flux_set_fp8(self._h, 3 if fp8 == "attn" else 1), "ldx_flux_set_fp8")
        keep = self._load_any(state_dict, strip=("model.diffusion_model.",), device_weights=device_weights)
        self._finalize()
        del keep
        self._pe = {}

    @classmethod
    def from_gguf(cls, path, cfg=None, device: int = 0, dtype: str = "bf16", fp8: bool = False, device_weights: bool = True):
        """The reference's flux1-dev-Q8_0.gguf (UnetLoaderGGUF, pipeline.py:218-236); cfg=None: flux-dev."""
        from .gguf import gguf_state_dict
        return cls(cfg or FluxConfig(), gguf_state_dict(path), device=device, dtype=dtype, fp8=fp8, device_weights=device_weights)

    def _run(self, x, sigma, ctx, y, guidance, denoise):
        assert x.is_cuda and x.dtype == torch.float32 and x.dim() == 4
        b, _, h, w = x.shape
        lt = ctx.shape[1]
        key = (lt, h, w)
        if key not in self._pe:
            cos, sin = flux_rope_tables(self.cfg, lt, h, w)
            self._pe[key] = (cos.to(self.device), sin.to(self.device))
        cos, sin = self._pe[key]
        f32 = lambda t: None if t is None else t.to(self.device, torch.float32).contiguous()
        x, sigma, ctx, y, guidance = f32(x), f32(sigma), f32(ctx), f32(y), f32(guidance)
        out = torch.empty_like(x)
        lib.check(self._lib.ldx_flux_forward(self._h, lib.ptr(x), lib.ptr(sigma), lib.ptr(ctx), lib.ptr(y), lib.ptr(guidance),
                                             lib.ptr(cos), lib.ptr(sin), b, h, w, lt, int(denoise), lib.ptr(out),
                                             lib.current_stream_ptr()), "ldx_flux_forward")
        return out

    def set_fbcache(self, residual_diff_threshold: float):
        """ApplyFBCacheOnModel.patch (fbcache_nodes.py:8-201): opt-in approximate first-block cache; 0 disables."""
        lib.check(self._lib.ldx_flux_fbcache(self._h, float(residual_diff_threshold)), "ldx_flux_fbcache")

    def fbcache_stats(self):
        h, m = C.c_int64(), C.c_int64()
        lib.check(self._lib.ldx_flux_fbcache_stats(self._h, C.byref(h), C.byref(m)), "ldx_flux_fbcache_stats")
        return {"hits": h.value, "misses": m.value}

    def forward(self, x, timestep, ctx, y, guidance):
        """Flux3.forward(x, timestep, context, y, guidance) (Flux.py:732-778)."""
        return self._run(x, timestep, ctx, y, guidance, False)

    def denoise(self, x, sigma, ctx, y, guidance):
        """BaseModel.apply_model for ModelType.FLUX: x - Flux3(x, sigma, ...) * sigma (sampling.py:100-155)."""
        return self._run(x, sigma, ctx, y, guidance, True)
