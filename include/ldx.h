/* ldx.h — C ABI of libldx.so, the MI355X-native drop-in for LightDiffusion-Next's denoising hot path.
 *
 * The reference (Aatricks/LightDiffusion-Next, 100 % Python) exposes one plugin boundary for an
 * accelerated UNet: model_options["model_function_wrapper"], called at src/cond/cond.py:254-263 as
 *     wrapper(model.apply_model, {"input", "timestep", "c", "cond_or_uncond"})
 * and installed with ModelPatcher.set_model_unet_function_wrapper (src/Model/ModelPatcher.py:138-144);
 * Stable-Fast (src/StableFast/StableFast.py:230-274) and FBCache (src/WaveSpeed/fbcache_nodes.py:96-111)
 * sit behind it.  Everything below is what a ctypes binding for that hook needs: plain pointers and
 * sizes, no torch types.  All `const float*` / `void*` tensor arguments of the compute calls are
 * DEVICE pointers on the engine's device; ldx_load_tensor takes HOST pointers (ldx_load_tensor_device: device pointers).
 *
 * Conventions: every call returns 0 on success or a negative LDX_E* code; ldx_last_error() returns a
 * thread-local human-readable message.  One engine per device, not thread-safe (the reference has a
 * single caller thread).  `stream` is a hipStream_t passed as void* (NULL = default).
 */
#ifndef LDX_H
#define LDX_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define LDX_OK 0
#define LDX_EINVAL (-1)      /* bad argument / unsupported configuration */
#define LDX_EMISSING (-2)    /* a required weight tensor was not loaded */
#define LDX_EHIP (-3)        /* HIP runtime error */
#define LDX_ESTATE (-4)      /* call sequence error (e.g. denoise before finalize) */

/* element types */
#define LDX_BF16 0
#define LDX_F16 1
#define LDX_F32 2

typedef struct ldx_engine ldx_engine;

/* Mirrors the keyword arguments of UNetModel1.__init__ (src/NeuralNetwork/unet.py:208-252) that the
 * SD1.5 family uses (src/SD15/SD15.py:10-77 + detect_unet_config unet.py:773-1080). */
typedef struct ldx_unet_config {
    int32_t compute_dtype;              /* LDX_BF16 (default) or LDX_F16: activation + weight storage type */
    int32_t in_channels;                /* 4 */
    int32_t out_channels;               /* 4 */
    int32_t model_channels;             /* 320; must be a multiple of 64 */
    int32_t num_levels;                 /* len(channel_mult) = 4 */
    int32_t channel_mult[8];            /* 1,2,4,4 */
    int32_t num_res_blocks[8];          /* 2,2,2,2 */
    int32_t transformer_depth[32];      /* per input res block, consumed front-to-back: 1,1,1,1,1,1,0,0 */
    int32_t transformer_depth_output[48]; /* per output block, stored in the reference's order (popped from the END) */
    int32_t transformer_depth_middle;   /* 1 ; -1 = no transformer, -2 = no middle block */
    int32_t num_heads;                  /* 8 */
    int32_t context_dim;                /* 768; multiple of 64 */
} ldx_unet_config;

/* VAE decoder (AutoencoderKL) — kwargs of Decoder.__init__ (src/AutoEncoders/VariationalAE.py:416-530) with the
 * ddconfig VAE.__init__ builds (VariationalAE.py:612-640). */
typedef struct ldx_vae_config {
    int32_t compute_dtype;      /* LDX_BF16 | LDX_F16 (the reference decodes in fp32 on CPU/ROCm, VAE_DTYPE) */
    int32_t z_channels;         /* 4 */
    int32_t ch;                 /* 128 ; multiple of 64 */
    int32_t num_levels;         /* 4 */
    int32_t ch_mult[8];         /* 1,2,4,4 */
    int32_t num_res_blocks;     /* 2 */
    int32_t out_ch;             /* 3 */
    int32_t use_post_quant;     /* 1 for SD1.5 (AutoencodingEngine.decode, VariationalAE.py:130-145); 0 for Flux */
} ldx_vae_config;

/* CLIP text encoder — keys of include/clip/sd1_clip_config.json read by CLIPTextModel_ (src/clip/CLIPTextModel.py:3-50). */
typedef struct ldx_clip_config {
    int32_t compute_dtype;
    int32_t hidden_size;            /* 768 */
    int32_t num_layers;             /* 12 */
    int32_t num_heads;              /* 12 */
    int32_t intermediate_size;      /* 3072 */
    int32_t max_positions;          /* 77 */
    int32_t vocab_size;             /* 49408 */
} ldx_clip_config;

/* T5 encoder — src/clip/clip/t5_config_xxl.json as read by T5 (src/clip/FluxClip.py:476-519): gated tanh-GELU FF,
 * RMS T5LayerNorm (eps 1e-6), relative-position bias from block 0 shared by every block, inner_dim = d_model. */
typedef struct ldx_t5_config {
    int32_t compute_dtype;
    int32_t d_model;               /* 4096 ; multiple of 64 */
    int32_t d_ff;                  /* 10240 ; multiple of 64 */
    int32_t num_layers;            /* 24 */
    int32_t num_heads;             /* 64 ; head dim = d_model / num_heads, multiple of 8, <= 160 */
    int32_t vocab_size;            /* 32128 */
} ldx_t5_config;

/* ESRGAN RRDBNet (src/UltimateSDUpscale/RDRB.py:216-471): nf 64 / gc 32 dense blocks, 2^num_upscale nearest+conv upsampling. */
typedef struct ldx_esrgan_config {
    int32_t compute_dtype;
    int32_t in_nc;                 /* 3 */
    int32_t out_nc;                /* 3 */
    int32_t nf;                    /* 64 */
    int32_t gc;                    /* 32 */
    int32_t num_blocks;            /* 23 RRDBs */
    int32_t num_upscale;           /* 2 -> x4 */
} ldx_esrgan_config;

/* TAESD decoder (src/AutoEncoders/taesd.py:105-135, Decoder2): the tiny autoencoder behind the sampler loops' latent previews. */
typedef struct ldx_taesd_config {
    int32_t compute_dtype;
    int32_t latent_channels;       /* 4 */
} ldx_taesd_config;

/* SAM image encoder (segment_anything ImageEncoderViT; the reference loads ViT-B, src/AutoDetailer/SAM.py:157-182).  Patch size 16, absolute and decomposed
 * relative position embeddings; the head dimension embed_dim / num_heads must be 64 (ViT-B, ViT-L), anything else is LDX_EINVAL. */
typedef struct ldx_sam_config {
    int32_t compute_dtype;
    int32_t image_size;            /* 1024 ; multiple of 16 */
    int32_t embed_dim;             /* 768 */
    int32_t depth;                 /* 12 ; at most 32 */
    int32_t num_heads;             /* 12 */
    int32_t mlp_dim;               /* 3072 */
    int32_t out_chans;             /* 256 ; multiple of 64 */
    int32_t window_size;           /* 14 */
    uint32_t global_attn_mask;     /* bit i set: block i attends globally (ViT-B: blocks 2, 5, 8, 11 = 0x924) */
} ldx_sam_config;

/* SAM prompt encoder + mask decoder (segment_anything PromptEncoder, MaskDecoder with its TwoWayTransformer; the same for ViT-B, ViT-L and ViT-H).  fp32
 * throughout, so there is no compute_dtype.  The grid is image_size / 16 a side.  LDX_EINVAL at creation: hidden % 64 != 0, hidden / 2 not divisible by
 * num_heads, a cross-attention head dimension hidden / 2 / num_heads other than 8, 16 or 32, depth != 2, num_multimask != 3, mlp_dim or iou_head_hidden
 * not a positive multiple of 4, image_size not a positive multiple of 16. */
typedef struct ldx_samdec_config {
    int32_t image_size;            /* 1024 */
    int32_t hidden;                /* 256 : transformer_dim = prompt embed_dim */
    int32_t num_heads;             /* 8 */
    int32_t mlp_dim;               /* 2048 */
    int32_t iou_head_hidden;       /* 256 */
    int32_t depth;                 /* 2 */
    int32_t num_multimask;         /* 3 : with the single-mask token, 4 mask tokens */
} ldx_samdec_config;

/* Flux DiT — FluxParams (src/BlackForest/Flux.py:293-306); flux-dev: 16, 768, 4096, 3072, 4.0, 24, 19, 38,
 * axes [16,56,56], theta 10000, qkv_bias 1, guidance_embed 1. */
typedef struct ldx_flux_config {
    int32_t compute_dtype;
    int32_t in_channels;          /* latent channels (16); tokens carry 4x that after the 2x2 patchify */
    int32_t vec_in_dim;           /* 768  (pooled CLIP-L) */
    int32_t context_in_dim;       /* 4096 (T5-XXL) ; multiple of 8 */
    int32_t hidden_size;          /* 3072 ; multiple of 64 */
    int32_t mlp_hidden;           /* int(hidden_size * mlp_ratio) = 12288 ; multiple of 64 */
    int32_t num_heads;            /* 24 ; head dim = hidden/heads in {16,32,64,128} */
    int32_t depth;                /* 19 double-stream blocks */
    int32_t depth_single;         /* 38 single-stream blocks */
    int32_t guidance_embed;       /* 1 */
} ldx_flux_config;

/* ---- lifecycle -------------------------------------------------------------------------------- */
const char* ldx_version(void);
const char* ldx_last_error(void);
/* Create an engine for `device` (HIP ordinal).  Replaces BaseModel.__init__ + UNetModel1.__init__
 * (src/Model/ModelBase.py:38-57, unet.py:208-677) for the accelerated path. */
int ldx_create(const ldx_unet_config* cfg, int device, ldx_engine** out);
void ldx_destroy(ldx_engine* e);
/* Hand one state-dict tensor to the engine (HOST pointer; dtype LDX_F16|LDX_BF16|LDX_F32).  Keys use
 * the SD1.5 `model.diffusion_model.` layout with that prefix stripped, e.g.
 * "input_blocks.1.1.transformer_blocks.0.attn1.to_q.weight".  Replaces BaseModel.load_model_weights
 * (ModelBase.py:178-202) + the per-forward cast of cond/cast.py:44-78 (cast happens once, here). */
int ldx_load_tensor(ldx_engine* e, const char* key, const void* data, int dtype, const int64_t* shape, int ndim);
/* The same for a tensor that already lives on the engine's DEVICE (UNet engines only): contiguous, dtype LDX_F16|LDX_BF16|LDX_F32.  The tensor is
 * NOT copied: it must stay valid and unchanged until ldx_finalize (or ldx_unet_refresh_commit) returns, and work queued on other streams that
 * writes it must have completed.  The weights are packed by device kernels (csrc/pack.hip) into exactly the bits the host path produces.
 * Host and device tensors may be mixed key by key; a later registration of a key replaces the earlier one.  This is how the reference's
 * hook hands over its model: the state dict is on the GPU after ModelPatcher.patch_model (ModelPatcher.py:515). */
int ldx_load_tensor_device(ldx_engine* e, const char* key, const void* dev_ptr, int dtype, const int64_t* shape, int ndim);
/* Sigma / timestep tables built by the host exactly as the reference builds them
 * (ModelSamplingDiscrete.set_sigmas sampling.py:285-289 -> log_sigmas[n];
 *  timestep_embedding sampling_util.py:56-76 evaluated at t = 0..n-1 -> temb[n][model_channels]).
 * UNet engines only: on a handle of any other model LDX_ESTATE ("not a UNet engine"), like every ldx_unet_* entry point,
 * before an argument is looked at. */
int ldx_set_tables(ldx_engine* e, const float* log_sigmas, int n, const float* temb, int temb_dim);
/* Pack weights into MFMA-friendly layouts and upload them.  After this the host copies are dropped. */
int ldx_finalize(ldx_engine* e);
/* Replace the weights of a FINALIZED UNet engine in place: what the reference does to its torch modules at run time with
 * ModelPatcher.patch_model / unpatch_model (ModelPatcher.py:515,652) when a LoRA is applied, removed or re-weighted.
 *   ldx_unet_refresh_begin   re-opens ldx_load_tensor / ldx_load_tensor_device (without it both answer LDX_ESTATE after ldx_finalize) and
 *                            forgets tensors registered by an unfinished refresh.  LDX_ESTATE unless the engine is a finalized UNet engine.
 *   ldx_unet_refresh_commit  needs the FULL key set again.  It first resolves every key and shape: LDX_EMISSING names the key, nothing has been
 *                            written and the engine keeps computing with its present weights.  Then every packed buffer is derived again into
 *                            the SAME device allocations (no allocation of weight memory, no pointer changes: cached plans and captured graphs
 *                            stay valid), the per-timestep emb_layers table is rebuilt and the cached context projections
 *                            (ldx_unet_context_cache) are dropped.  Synchronous like ldx_finalize: it waits for the device before (no call may
 *                            still be reading the weights) and after.  Success or failure, the refresh is over when it returns.
 *   ldx_unet_refresh_abort   gives up a refresh that was begun: forgets the tensors registered since ldx_unet_refresh_begin and closes the two
 *                            loaders again.  The weights are untouched.  A no-op on a finalized UNet engine with no refresh open.
 * The plan switches read from the environment (LDX_LNFOLD, LDX_NO_FUSED_SKIP, ...) must be as they were at ldx_finalize: LDX_ESTATE otherwise. */
int ldx_unet_refresh_begin(ldx_engine* e);
int ldx_unet_refresh_commit(ldx_engine* e);
int ldx_unet_refresh_abort(ldx_engine* e);
/* Diagnostic (tests): 64-bit FNV-1a over every packed weight buffer of a finalized UNet engine, in allocation order, computed on the host
 * from copies of the buffers.  Equal digests = bit-identical weights, however they were loaded. */
int ldx_weights_digest(ldx_engine* e, uint64_t* out);
/* The same digest for ANY finalized engine (on a UNet engine it equals ldx_weights_digest): the buffers are the packed 16-bit matrices and fp32
 * vectors of ldx_finalize, in allocation order (a Flux engine's MX fp8 copies are derived from them and are not counted). */
int ldx_packed_digest(ldx_engine* e, uint64_t* out);
/* ldx_load_tensor_device for UNet, Flux and T5 engines (the same contract: not copied, valid and unchanged until ldx_finalize returns).  The F32,
 * F16 and BF16 tensors of a GGUF file go this way.  Any other engine: LDX_ESTATE, before an argument is looked at. */
int ldx_load_tensor_dev(ldx_engine* e, const char* key, const void* dev_ptr, int dtype, const int64_t* shape, int ndim);
/* A GGML Q8_0 tensor (the reference's Flux and T5 files, Quantize/Quantizer.py:94-112): `blocks` = numel / 32 blocks of 34 bytes, each an fp16 scale d
 * followed by 32 int8 values q along the INNERMOST axis of `shape` (the logical torch shape).  A weight is fp16_rne(float(d) * q): torch's
 * d.view(float16) * q.view(int8), one rounding of an exact product, so the tensor is from here on an ordinary LDX_F16 tensor of that shape.
 * Flux and T5 engines before ldx_finalize; any other engine LDX_ESTATE before an argument is looked at.  LDX_EINVAL: ndim == 0, an innermost extent
 * that is no multiple of 32, a null or odd pointer (blocks are 2-byte aligned, no more).
 *   on_device = 0: `blocks` is a HOST pointer; expanded on the host (csrc/weight_convert.h) and kept like an ldx_load_tensor copy.
 *   on_device = 1: `blocks` is a DEVICE pointer; expanded by csrc/q8.hip on the null stream into an fp16 device buffer the engine owns (released when
 *                  ldx_finalize returns) and registered like an ldx_load_tensor_dev tensor.  `blocks` may be freed as soon as the call returns. */
int ldx_load_tensor_q8_0(ldx_engine* e, const char* key, const void* blocks, const int64_t* shape, int ndim, int on_device);

/* ---- the hot path ----------------------------------------------------------------------------- */
/* The wrapper body: denoised = x - UNet(x / sqrt(sigma^2+1), t(sigma), ctx) * sigma — i.e. all of
 * BaseModel.apply_model (ModelBase.py:72-133) for EPS prediction (sampling.py:26-56).
 *   x_nchw  [B2][C][h][w] fp32, sigma [B2] fp32 (sigma VALUES, as the hook passes them),
 *   ctx     [B2][M][context_dim] fp32 (c["c_crossattn"]), out_nchw like x_nchw.  */
int ldx_unet_denoise(ldx_engine* e, const float* x_nchw, const float* sigma, const float* ctx,
                     int B2, int h, int w, int M, float* out_nchw, void* stream);
/* The same with the concat conditioning of inpainting UNets (BaseModel.apply_model, ModelBase.py:100-101:
 * xc = torch.cat((x / sqrt(sigma^2 + 1), c_concat), dim=1)): x_nchw [B2][in_channels - cc_channels][h][w] is the latent (scaled, and the x of
 * denoised = x - eps * sigma), c_concat [B2][cc_channels][h][w] fp32 is appended UNSCALED; the engine's in_channels (9 for SD1.5 inpainting) counts
 * both.  LDX_EINVAL unless in_channels - cc_channels == out_channels. */
int ldx_unet_denoise_concat(ldx_engine* e, const float* x_nchw, const float* sigma, const float* ctx, const float* c_concat, int cc_channels,
                            int B2, int h, int w, int M, float* out_nchw, void* stream);
/* One CFG evaluation as calc_cond_batch builds it (cond/cond.py:186-226: input_x = cat([x] * 2), timestep = cat([sigma] * 2),
 * c_crossattn = cat([uncond, cond])): x_nchw [B][C][h][w] is read by BOTH halves of the [uncond x B ; cond x B] batch, sigma is
 * one host scalar shared by every sample, ctx [2B][M][context_dim], out_nchw [2B][C][h][w].  Same arithmetic as
 * ldx_unet_denoise on the concatenated inputs (bit-identical); replaces two device copies and a fill per sampler step. */
int ldx_unet_denoise_cfg(ldx_engine* e, const float* x_nchw, float sigma, const float* ctx,
                         int B, int h, int w, int M, float* out_nchw, void* stream);
/* The same with the timestep index supplied by the caller.  ModelSamplingDiscrete.timestep (sample/sampling.py:309-320, called from
 * BaseModel.apply_model, ModelBase.py:112) is INTEGER work: argmin_k |log(sigma) - log_sigmas[k]|.  The device lookup (ldx_unet_denoise*,
 * ldx_unet_timestep) runs the GPU's logf, which may differ from the host's log in the last bit — at a near-tie (sigma at the geometric midpoint of two
 * table entries, e.g. the `normal` scheduler's fractional timesteps) that picks the other index.  Where sigma is a host scalar (every sampler
 * loop) the host side therefore evaluates the reference's own torch expression and passes the result here: bit-exact by construction.
 * t_index in [0, n_sigmas); t_index < 0 = ldx_unet_denoise_cfg (device lookup). */
int ldx_unet_denoise_cfg_t(ldx_engine* e, const float* x_nchw, float sigma, int t_index, const float* ctx,
                           int B, int h, int w, int M, float* out_nchw, void* stream);
/* ldx_unet_denoise with per-sample timestep indices from the caller: t_index [B2] fp32 DEVICE array (integer-valued), same reasoning. */
int ldx_unet_denoise_t(ldx_engine* e, const float* x_nchw, const float* sigma, const float* t_index, const float* ctx,
                       int B2, int h, int w, int M, float* out_nchw, void* stream);
/* The device's sigma -> timestep lookup alone (the device function the boundary kernel of ldx_unet_denoise* runs): sigma [n] fp32 and
 * t_out [n] int32 are DEVICE arrays.  For tests of the index as an integer (tests/test_timestep_gpu.py). */
int ldx_unet_timestep(ldx_engine* e, const float* sigma, int n, int32_t* t_out, void* stream);
/* Context cache for a sampling run.  The reference recomputes to_k(context) / to_v(context) of all 16 cross-attentions in every step
 * (CrossAttention.forward, src/Attention/Attention.py:100-124, called from transformer.py:186-245) although `c_crossattn` is the same tensor content
 * for every step of a run (calc_cond_batch rebuilds it from the same conditioning, cond/cond.py:150-288).  enable = 1: the CALLER PROMISES that the
 * bytes behind a given ctx pointer stay unchanged until its next call of this function (any argument); the engine then converts / projects the
 * context once per (input shape, ctx pointer) and every later ldx_unet_denoise* call with that pointer reuses the projections (identical bits:
 * the same kernels produced them).  Every call of this function — also with enable = 1 again — INVALIDATES what is cached: call it after
 * rewriting a context buffer in place.  enable = 0 (the default): projections recomputed on every call, as the reference does.
 * The hook object (LdxUNetPatch) leaves it off: the reference hands the hook a fresh torch.cat every step. */
int ldx_unet_context_cache(ldx_engine* e, int enable);
/* Raw UNetModel1.forward (unet.py:679-770): x (already scaled), integer timesteps given as fp32. */
int ldx_unet_forward(ldx_engine* e, const float* x_nchw, const float* timesteps, const float* ctx,
                     int B2, int h, int w, int M, float* out_nchw, void* stream);
/* Number of kernel launches in the current plan, algorithmic FLOPs of one forward at the planned shape
 * (2*MACs of every Linear/Conv + 4*B*H*N*M*D per attention), arena bytes.  STEADY-STATE numbers: while the context cache is on
 * (ldx_unet_context_cache) the context's 16-bit copy and k|v projections are not part of them (they run once per context, not per step). */
int ldx_plan_info(ldx_engine* e, int64_t* n_launches, double* flops, int64_t* arena_bytes);
/* Shared CFG prefix.  calc_cond_batch evaluates [uncond; cond] over cat([x] * 2) and cat([sigma] * 2) (cond/cond.py:186-226): until the context enters at the
 * first cross-attention (input_blocks.1.1.transformer_blocks.0.attn2 in SD1.5) both halves of the batch hold IDENTICAL values — conv_in, the first
 * ResBlock, norm / proj_in, norm1, q|k|v, the first self-attention and its to_out compute every number twice.  ldx_unet_denoise_cfg* (the one entry
 * point that KNOWS the halves share x and sigma) plans those ops on one half and copies the results into the other half's rows where the first
 * cross-attention and the skip connections read them; the outputs equal the concatenated ldx_unet_denoise call up to the summation order of
 * GroupNorm statistics (tile shapes follow the row count).  enable = 0: every op on the full batch (bit-identical to the concatenated call);
 * 1 (default; environment LDX_CFG_SHARE overrides the default): where it pays — at least LDX_CFG_SHARE_MINROWS (8192) rows per half, below that the
 * half-batch launches no longer fill the chip (512^2 at bs = 1 measured 5.73 against 5.69 ms per step shared); 2: whenever the model has a
 * cross-attention for the prefix to end at (tests). */
int ldx_unet_cfg_share(ldx_engine* e, int enable);
/* FLOPs of the current plan as EXECUTED in steady state, and the part of ldx_plan_info's algorithmic count that the shared CFG prefix does not
 * execute.  algorithmic = executed + shared + what the phase form of the up convs leaves out: a nearest-2x upsample + 3x3 conv run as four 2 x 2 convs
 * over the stored image executes 4/9 of the reference's arithmetic, and the other 5/9 stay in the algorithmic count only (no plan below the sizes
 * where the form is taken has such a term; environment LDX_UPCONV_PHASE=0: none has).  Roofline fractions are quoted on the executed number. */
int ldx_plan_flops(ldx_engine* e, double* executed, double* shared);
/* Memory behaviour: an engine keeps the launch plan, arena and captured graph of its CURRENT input shape plus up to four earlier
 * shapes (the multi-scale samplers and HiresFix alternate between resolutions; Flux plans are per (B, h, w, prompt length)).  Each
 * cached plan holds its own arena; the cache is trimmed oldest-first to at most 4 entries and LDX_PLAN_CACHE_GIB (default 16) GiB. */
/* Per-kernel-class timing of subsequent eager forwards with HIP events recorded on the launch stream
 * (used by bench.py for the roofline line).  ldx_profile_report writes a JSON object
 * {"<kernel>": {"count", "ms", "flops", "bytes"}, ...} (algorithmic flops/bytes, summed) into buf.
 * enable = 2 keys the report by kernel class *and* op shape (tuning aid). */
int ldx_profile(ldx_engine* e, int enable, int reset);
int ldx_profile_report(ldx_engine* e, char* buf, int64_t cap);
/* Capture the planned forward into a hipGraph for replay (0 = eager launches).  UNet, TAESD and SAM engines; every other engine accepts the call and
 * keeps launching eagerly. */
int ldx_set_graph_mode(ldx_engine* e, int enable);
/* UNet, TAESD and SAM engines (0, 0 on every other): how many times a forward was captured into a hipGraph and how many times a captured graph was replayed since the engine was
 * created (a captured graph is tied to the pointers of the call that recorded it: a caller that alternates buffers re-captures instead of
 * replaying — sampling.CFGDenoiser stages such inputs through one persistent buffer per shape). */
int ldx_graph_stats(ldx_engine* e, int64_t* captures, int64_t* replays);
/* Every LDX_* switch of the library is read from the environment ONCE when the library is loaded (two when a UNet engine is created) — never on a launch path.
 * This re-reads the attention dispatch switches, all of them and nothing else: the fields of AttnSwitches (csrc/ldx_switches.h; LDX_ATTN_PIPE*, LDX_ATTN32*,
 * LDX_ATTN_KPF, LDX_ATTN512, LDX_ATTN512_SPLITS).  For tests and same-process A/B runs that change one after loading; the GEMM and planner switches stay as
 * loaded, because plans bake them into their op lists. */
int ldx_reload_env(void);

/* ---- VAE decode and CLIP text encode (same ldx_engine handle type; load/finalize/destroy as above) ---------- */
/* Keys for ldx_load_tensor: the reference's first_stage_model state dict ("decoder.*", "post_quant_conv.*"). */
int ldx_vae_create(const ldx_vae_config* cfg, int device, ldx_engine** out);
/* VAE.decode (VariationalAE.py:690-722): z [B][z_channels][h][w] fp32 (already divided by the latent scale) ->
 * clamp((decoder(post_quant_conv(z)) + 1) / 2, 0, 1) as NHWC fp32 [B][8h][8w][3]. */
int ldx_vae_decode(ldx_engine* e, const float* z_nchw, int B, int h, int w, float* out_nhwc, void* stream);
/* VAE.encode's deterministic part (VariationalAE.py:725-760, Encoder.forward :378-413, quant_conv :160-166): pixels
 * [B][H][W][3] fp32 in [0,1] -> process_input (x*2-1) -> Encoder -> quant_conv -> moments [B][2*z_channels][H/8][W/8]
 * fp32 (mean | logvar).  Needs the "encoder.*" / "quant_conv.*" tensors to have been loaded.  The stochastic
 * DiagonalGaussianRegularizer.sample (VariationalAE.py:42-51, global CPU RNG) stays on the host. */
int ldx_vae_encode(ldx_engine* e, const float* pixels_nhwc, int B, int H, int W, float* moments_nchw, void* stream);
/* Keys: the transformer's state dict with the "text_model." prefix stripped ("embeddings.token_embedding.weight",
 * "encoder.layers.0.self_attn.q_proj.weight", ..., "final_layer_norm.weight"). */
int ldx_clip_create(const ldx_clip_config* cfg, int device, ldx_engine** out);
/* CLIPTextModel_.forward (src/clip/CLIPTextModel.py:51-107): ids [B][T] int32 -> out_last = final_layer_norm(x_L)
 * [B][T][hidden] fp32; if out_inter != NULL, out_inter = final_layer_norm(x after layer `inter_layer`)
 * (negative counts from the end, e.g. -2 = clip-skip 2; Clip.py:218-236).  Causal mask, no padding mask. */
int ldx_clip_encode(ldx_engine* e, const int32_t* ids, int B, int T, int inter_layer,
                    float* out_last, float* out_inter, void* stream);
/* Pooled output: the row of `last` [B][T][hidden] (ldx_clip_encode's out_last) at the first position whose id equals eos_token_id —
 * position 0 when there is none, as torch's argmax over an all-zero row gives (CLIPTextModel_.forward, CLIPTextModel.py:98-106) —
 * and, when the optional tensor "text_projection.weight" [hidden][hidden] was loaded, that row times its transpose
 * (CLIPTextModel.forward, CLIPTextModel.py:130,152-163; fp32).  out_pooled [B][hidden] fp32. */
int ldx_clip_pooled(ldx_engine* e, const float* last, const int32_t* ids, int B, int T, int eos_token_id,
                    float* out_pooled, void* stream);
/* Textual-inversion vectors (SDClipModel.set_up_textual_embeddings, src/SD15/SDClip.py:213-267): rows_host [n][hidden] fp32
 * (HOST pointer) become token ids vocab_size .. vocab_size + n - 1 for the following ldx_clip_encode calls; n = 0 removes
 * them.  Synchronous.  The reference rebuilds its nn.Embedding per forward; the engine keeps one side table instead. */
int ldx_clip_set_extra_embeddings(ldx_engine* e, const float* rows_host, int n);

/* ---- ESRGAN upscaler --------------------------------------------------------------------------- */
/* Keys: RRDBNet's own module names ("model.0.weight", "model.1.sub.0.RDB1.conv1.0.weight", ..., "model.1.sub.<nb>.weight",
 * "model.3.weight", "model.6.weight", "model.8.weight", "model.10.weight"); newer checkpoint layouts are renamed by the host
 * exactly as RRDBNet.new_to_old_arch does (RDRB.py:381-441). */
int ldx_esrgan_create(const ldx_esrgan_config* cfg, int device, ldx_engine** out);
/* RRDBNet.forward: pixels [B][H][W][in_nc] fp32 -> [B][sH][sW][out_nc] fp32, s = 2^num_upscale (no clamp). */
int ldx_esrgan_forward(ldx_engine* e, const float* pixels_nhwc, int B, int H, int W, float* out_nhwc, void* stream);
/* TAESD decoder.  State-dict keys are Decoder2's nn.Sequential indices ("1.weight", "3.conv.0.weight", ..., "19.bias"; 67 tensors). */
int ldx_taesd_create(const ldx_taesd_config* cfg, int device, ldx_engine** out);
/* TAESD.decode / the tensor part of taesd_preview (taesd.py:224-237, 257-304) of a latent [B][4][h][w] fp32.  Each output may be NULL (not both):
 * out_f32 [B][3][8h][8w] fp32 = (decoder(latent) - 0.5) * 2;  out_u8 [B][8h][8w][3] = trunc(clip(((d + 1) / 2) * 255, 0, 255)) of that d, and with
 * flux_flag != 0 channel c of it from d[2 - c] clamped to [-1, 1].  A handle of another model: LDX_ESTATE, nothing is launched. */
int ldx_taesd_decode(ldx_engine* e, const float* latent, int B, int h, int w, float* out_f32, uint8_t* out_u8, int flux_flag, void* stream);
/* Test surface: ONE launch of the decoder's conv kernel.  Y [B][H][W][64] = relu?(conv3x3(X) + bias + R) on 16-bit rows, H = Hin << up, W = Win << up
 * (up = 1: nearest x2 of X [B][Hin][Win][64] folded into the gather); Wt [64][(ky * 3 + kx) * 64 + ci] 16-bit; bias [64] fp32 or NULL; R like Y or NULL;
 * Rf: the residual as fp32 [B][H][W][64] instead (not both); Yf: the unrounded result as fp32 as well, or NULL. */
int ldx_taesd_conv64(const void* X, const void* Wt, const float* bias, const void* R, const float* Rf, void* Y, float* Yf, int B, int Hin, int Win, int up, int relu, int dtype, void* stream);
/* SAM image encoder.  State-dict keys are segment_anything's own with "image_encoder." stripped: pos_embed, patch_embed.proj.{weight,bias},
 * blocks.<i>.norm1|norm2.{weight,bias}, blocks.<i>.attn.qkv|proj.{weight,bias}, blocks.<i>.attn.rel_pos_h|rel_pos_w, blocks.<i>.mlp.lin1|lin2.{weight,bias},
 * neck.0.weight, neck.1.{weight,bias}, neck.2.weight, neck.3.{weight,bias}.  A rel_pos table must have 2 n - 1 rows (n = window_size, or image_size / 16 in a
 * global block), as the official checkpoints do: ldx_finalize answers LDX_EINVAL otherwise (the interpolation of other lengths is not built). */
int ldx_sam_create(const ldx_sam_config* cfg, int device, ldx_engine** out);
/* ImageEncoderViT.forward: x [B][3][size][size] fp32, already preprocessed (ldx_sam_preprocess) -> out [B][out_chans][size / 16][size / 16] fp32.
 * A handle of another model: LDX_ESTATE, nothing is launched. */
int ldx_sam_encode(ldx_engine* e, const float* x_nchw_f32, int B, float* out_nchw_f32, void* stream);
/* Sam.preprocess: img u8 [h][w][3] with rows `pitch` bytes apart -> out fp32 [3][size][size] = (float(img) - mean_c) / std_c with the pixel mean
 * (123.675, 116.28, 103.53) and std (58.395, 57.12, 57.375), IEEE subtraction and division; zeros right of w and below h.  h, w <= size. */
int ldx_sam_preprocess(const uint8_t* img, int64_t pitch, int h, int w, float* out, int size, void* stream);
/* SAM prompt encoder + mask decoder.  State-dict keys are segment_anything's own: prompt_encoder.pe_layer.positional_encoding_gaussian_matrix,
 * prompt_encoder.point_embeddings.<0..3>.weight, prompt_encoder.not_a_point_embed.weight, prompt_encoder.no_mask_embed.weight, mask_decoder.iou_token.weight,
 * mask_decoder.mask_tokens.weight, mask_decoder.transformer.layers.<i>.{self_attn,cross_attn_token_to_image,cross_attn_image_to_token}.{q,k,v,out}_proj.*,
 * .norm<1..4>.*, .mlp.lin<1,2>.*, mask_decoder.transformer.final_attn_token_to_image.*, .norm_final_attn.*, mask_decoder.output_upscaling.<0,1,3>.*,
 * mask_decoder.output_hypernetworks_mlps.<0..3>.layers.<0..2>.*, mask_decoder.iou_prediction_head.layers.<0..2>.*.  Mask prompts (mask_downscaling) are not built.
 * LayerNorm eps 1e-5 in the transformer, 1e-6 in the upscaling's LayerNorm2d.  Every model-specific call on a handle of another model: LDX_ESTATE, nothing is launched.
 * Graph mode (ldx_set_graph_mode) captures predict per (P, n, boxes or not) once the same buffers have been seen twice, as the image encoder does. */
int ldx_samdec_create(const ldx_samdec_config* cfg, int device, ldx_engine** out);
/* Once per image: embedding fp32 [hidden][g][g] (the image encoder's output) -> the engine's rows embedding + no_mask_embed, and what layer 0 computes from
 * them alone (the token-to-image k and v projections, the image-to-token q projection).  Three launches. */
int ldx_samdec_set_image(ldx_engine* e, const float* embedding, void* stream);
/* SamPredictor.predict_torch for P prompts at once: points fp32 [P][n][2] and labels int32 [P][n] (n <= 8; both NULL with n = 0), boxes fp32 [P][4] or NULL, all
 * in the resized frame (ResizeLongestSide.apply_coords); a padding point (label -1) is added exactly when boxes is NULL.  lowres_out fp32 [P][4][4 g][4 g] and
 * iou_out fp32 [P][4]: index 0 is the single-mask output, 1 .. 3 the multimask ones.  LDX_EINVAL before any launch: n outside 0 .. 8, neither points nor
 * boxes, P outside 1 .. 64; LDX_ESTATE without ldx_samdec_set_image.  A prompt's result does not depend on what else shares the call. */
int ldx_samdec_predict(ldx_engine* e, const float* points, const int32_t* labels, int n, const float* boxes, int P, float* lowres_out, float* iou_out, void* stream);
/* Test surface: the prompt tokens alone, out fp32 [P][5 + ns][hidden], ns = n + (boxes ? 2 : 1): iou_token | mask_tokens | points | padding point or corners. */
int ldx_samdec_prompt_tokens(ldx_engine* e, const float* points, const int32_t* labels, int n, const float* boxes, int P, float* out, void* stream);
/* Sam.postprocess_masks + the threshold, stateless, one launch: lowres fp32 [n][L][L] -> bilinear (align_corners = false, no antialias) to image_size a side ->
 * crop to [in_h][in_w] -> bilinear to [H][W]; mask_u8 [n][H][W] = value > 0, logits fp32 [n][H][W] or NULL.  Per axis: scale = (float)in / (float)out,
 * s = max(scale * (dst + 0.5f) - 0.5f, 0), i0 = (int)s, i1 = min(i0 + 1, in - 1), l = s - i0; a sample is (v00 * (1 - lx) + v01 * lx) * (1 - ly) +
 * (v10 * (1 - lx) + v11 * lx) * ly, every product and sum rounded to fp32 on its own.  The image_size intermediate is never stored. */
int ldx_samdec_postprocess(const float* lowres, int n, int L, int in_h, int in_w, int H, int W, uint8_t* mask_u8, float* logits, int image_size, void* stream);
/* Test surface: ONE launch of each of the encoder's own kernels, on 16-bit rows (dtype).
 * ldx_op_sam_window: scatter = 0: dst [B * nw * nw][win * win][C] = the window partition of src [B][S][S][C], zero rows for the padding up to nw = ceil(S / win)
 * windows a side; scatter = 1: dst [B][S][S][C] = R + the inverse of src (the crop), R like dst (dst itself allowed) or NULL.  C % 8 == 0, src != dst.
 * ldx_op_sam_relpos: out fp32 [BW * H][n * n][2 n]: out[.][q][j] = sum_c Q[q][c] th[q / n - j + n - 1][c] for j < n, sum_c Q[q][c] tw[q % n - (j - n) + n - 1][c]
 * above; Q rows bw * n * n + q (row stride ldq, ldq % 8 == 0), head h at columns h * 64; th, tw fp32 [2 n - 1][64].
 * ldx_op_sam_attention: O[bw * N + q][h * 64 + d] = sum_k softmax_k(scale * q.k + rel[q][k / n] + rel[q][n + k % n]) v[k][d] over the N = n * n tokens of
 * (bw, h); Q, K, V share the row stride ld (ld % 8 == 0); rel as ldx_op_sam_relpos writes it; ldo % 4 == 0; BW * H <= 65535. */
int ldx_op_sam_window(const void* src, void* dst, const void* R, int B, int S, int win, int C, int scatter, int dtype, void* stream);
int ldx_op_sam_relpos(const void* Q, int ldq, const float* th, const float* tw, float* out, int BW, int H, int n, int dtype, void* stream);
int ldx_op_sam_attention(const void* Q, const void* K, const void* V, int ld, const float* rel, void* O, int ldo, int BW, int H, int n, float scale, int dtype, void* stream);
/* tiled_scale's feathered accumulation (src/Utilities/util.py:557-590): out/div [H][W][C] fp32 += tile [th][tw][C] * mask /
 * mask at (y0, x0); then ldx_tile_finish: out = out / div (div may be NULL), optionally clamped to [0,1] (USDU_upscaler.py:94). */
int ldx_tile_blend(const float* tile, int th, int tw, float* out, float* div, int H, int W, int C, int y0, int x0, int feather, void* stream);
int ldx_tile_finish(float* out, const float* div, int64_t n, int clamp01, void* stream);

/* First-block cache (WaveSpeed, src/WaveSpeed/first_block_cache.py:105-384 + fbcache_nodes.py:8-201; the reference's Flux
 * pipeline enables it with threshold 0.12, pipeline.py:228-231): opt-in APPROXIMATE mode — outputs differ from the exact
 * forward by design.  After double block 0, r = img_after - img_before; if mean|r_prev - r| / mean|r_prev| < threshold the
 * remaining blocks are skipped and the cached (final - after-block-0) residual of both streams is added instead; otherwise
 * they run and both caches refresh.  State resets when the shape changes or sigma[0] does not decrease between calls.
 * threshold <= 0 disables (default).  Stats count forwards that used / refreshed the cache. */
int ldx_flux_fbcache(ldx_engine* e, float residual_diff_threshold);
int ldx_flux_fbcache_stats(ldx_engine* e, int64_t* hits, int64_t* misses);
/* MX fp8 mode (BASELINE config 4 "fp8 MFMA"; opt-in, approximate, own parity class): the linears of the double / single
 * blocks run the block-scaled 16x16x128 MFMA on e4m3fn operands with one E8M0 scale per 32 consecutive k (weights
 * quantised once in ldx_finalize, activations per forward), and the batched adaLN modulation projections (img_mod / txt_mod /
 * modulation / final adaLN: one skinny GEMM) read MX weights against the MX-quantised SiLU(vec) (round 6; LDX_FLUX_MOD_FP8=0 keeps them
 * 16-bit); everything else stays 16-bit.  Call before ldx_finalize;
 * needs hidden_size % 128 == 0 and mlp_hidden % 128 == 0.  The reference runs Flux from Q8_0 weights (also 32-element
 * blocks, src/Quantize/Quantizer.py:94-112) dequantised to 16-bit, i.e. W8A16; this mode is W8A8.
 * enable = 1 (2 is an alias): the linears only; attention stays 16-bit.
 * enable = 3 (explicit opt-in; a DIFFERENT, less precise workload than mode 1): ... and, at head dim 128, QK^T and PV of the joint attention on the
 * block-scaled 32x32x64 MFMA as well (the rule of ldx_op_attention_fp8 below: Q / K quantised by the QKNorm + RoPE kernel, V by a transposing quantiser,
 * P rounded to e4m3) — the whole block is fp8 MFMA.  (Round 5 had this behind enable = 1; callers of mode 1 get the linears-only arithmetic back.) */
int ldx_flux_set_fp8(ldx_engine* e, int enable);

/* ---- T5-XXL text encoder (Flux conditioning) ---------------------------------------------------- */
/* Keys: T5's state dict ("shared.weight", "encoder.block.0.layer.0.SelfAttention.q.weight", ...,
 * "encoder.block.0.layer.1.DenseReluDense.wi_0.weight", "encoder.final_layer_norm.weight").  The relative-attention
 * embedding (encoder.block.0.layer.0.SelfAttention.relative_attention_bias.weight) stays with the host, which builds
 * the bias table exactly as T5Attention.compute_bias does (FluxClip.py:150-243). */
int ldx_t5_create(const ldx_t5_config* cfg, int device, ldx_engine** out);
/* T5.forward -> T5Stack.forward (FluxClip.py:441-519): ids [B][L] int32; bias = relative-position bias fp32
 * [num_heads][L][Lp], Lp = L rounded up to 64 (padding ignored), shared by the batch and by all blocks; no padding mask;
 * attention is unscaled (the reference pre-multiplies k by sqrt(d) to cancel SDPA's scale, :265-268).
 * out = final_layer_norm(x_L) [B][L][d_model] fp32. */
int ldx_t5_encode(ldx_engine* e, const int32_t* ids, int B, int L, const float* bias, float* out, void* stream);

/* ---- Flux DiT ------------------------------------------------------------------------------ */
/* Keys for ldx_load_tensor: Flux3's state dict ("img_in.weight", "double_blocks.0.img_mod.lin.weight", ...). */
int ldx_flux_create(const ldx_flux_config* cfg, int device, ldx_engine** out);
/* Flux3.forward (Flux.py:732-778) behind BaseModel.apply_model with CONST prediction (sampling.py:100-155):
 *   denoise != 0: out = x - Flux3(x, t = sigma, ctx, y, guidance) * sigma ; denoise == 0: raw model output.
 *   x [B][C][h][w] fp32 (h, w even), sigma [B], ctx [B][Lt][context_in_dim], y [B][vec_in_dim], guidance [B] (may be
 *   NULL when guidance_embed == 0); pe_cos / pe_sin: [Lt + h*w/4][head_dim/2] fp32 rotary tables the host builds
 *   with the reference's rope() (Flux.py:36-70) for ids = [txt_ids ; img_ids]. */
int ldx_flux_forward(ldx_engine* e, const float* x, const float* sigma, const float* ctx, const float* y,
                     const float* guidance, const float* pe_cos, const float* pe_sin,
                     int B, int h, int w, int Lt, int denoise, float* out, void* stream);

/* ---- sampler-side elementwise ops (src/sample/samplers.py, src/sample/CFG.py) ------------------ */
/* d = lerp(den_uncond, den_cond, cfg) (CFG.py:60), then
 * kind 0: Euler  x = x + ((x - d)/c0)*c1, c0 = sigma_hat, c1 = sigma_next - sigma_hat (samplers.py:308; util.py:26-37)
 * kind 1: DPM++ first order  x = c0*x - c1*d, c0 = sigma_next/sigma, c1 = expm1(-h)   (samplers.py:945-946)
 * kind 2: CFG combine only (denoised_out = d; x untouched) — low-resolution multiscale steps.
 * kind 3: noise injection  x = x + den_uncond * c0 (den_uncond = the noise tensor; samplers.py:723).
 * Same fp32 operation order as the reference expressions, no FMA contraction.  denoised_out may be NULL for kinds
 * 0, 1, 3; kind 2 REQUIRES it (LDX_EINVAL otherwise); kind 0 requires c0 != 0 (LDX_EINVAL otherwise). */
int ldx_sampler_step(int kind, float* x, const float* den_uncond, const float* den_cond, float* denoised_out,
                     int64_t n, float cfg, float c0, float c1, void* stream);
/* One pass of bislerp (src/Utilities/upscale.py:5-128; LatentUpscale for HiresFix, pipeline.py:346-366): slerp of the
 * C-vector (C <= 16) between source indices c1[i], c2[i] with ratio ratios[i] along axis 1 (width) or 0 (height);
 * fp32 NCHW in/out.  The index/ratio arrays are built by the host exactly as generate_bilinear_data does. */
int ldx_bislerp_pass(const float* in, float* out, int N, int C, int H, int W, int axis, int new_len,
                     const int32_t* c1, const int32_t* c2, const float* ratios, void* stream);
/* F.interpolate(mode="bilinear", align_corners=False) on fp32 [planes][H][W] (samplers.py:227-241). */
int ldx_bilinear(const float* in, float* out, int planes, int hin, int win, int hout, int wout, void* stream);

/* ---- 8-bit image ops of the img2img path (Ultimate SD Upscale, src/UltimateSDUpscale/UltimateSDUpscale.py:126-245) ---------------------- */
/* What the reference does in PIL between the networks.  Images are HWC uint8 on the device, C = 3 (RGB) or 1 (mask), with a row pitch in BYTES
 * (>= W * C), so a crop of a canvas is a source or a destination without a copy.  Pillow's 8-bit paths are integer arithmetic: the results are
 * Pillow's bytes, not approximations of them.  Stateless; every rectangle must lie inside its image (LDX_EINVAL otherwise). */
/* tensor_to_pil (image_util.py:133-178): in fp32 [H][W][C] dense -> out = (uint8) trunc(clamp(v, 0, 1) * 255.0f).  No rounding: k / 255.0f * 255.0f may
 * land just under k and give k - 1, as in the reference. */
int ldx_image_quantize(const float* in_hwc, int H, int W, int C, uint8_t* out, int64_t out_pitch, void* stream);
/* pil_to_tensor (image_util.py:181-203) of the crop (x0, y0, w, h) of img [H][W][C]: out fp32 [h][w][C] dense = v / 255.0f, the correctly rounded
 * IEEE quotient: the NHWC tensor ldx_vae_encode reads. */
int ldx_image_to_float(const uint8_t* img, int64_t pitch, int H, int W, int C, int x0, int y0, int w, int h, float* out_hwc, void* stream);
/* One axis of Pillow's 8-bit ImagingResample (Image.resize, UltimateSDUpscale.py:178,220-222,356-358): in [H][W][C] -> out with W (axis 1) or H
 * (axis 0) replaced by new_len.  Per output index i the host supplies bounds[2 i] = first source index, bounds[2 i + 1] = number of taps (<= ksize)
 * and kk[i][ksize] = the coefficients in 2^-22 units, built in double precision exactly as Pillow's precompute_coeffs / normalize_coeffs_8bpc do;
 *   out = clip8((2^21 + sum_j kk[i][j] * in[first + j]) >> 22).
 * A 2-D resize is the axis-1 pass, then the axis-0 pass, through a uint8 intermediate.  in and out must not overlap. */
int ldx_image_resample_pass(const uint8_t* in, int64_t in_pitch, int H, int W, int C, int axis, int new_len,
                            const int32_t* bounds, const int32_t* kk, int ksize, uint8_t* out, int64_t out_pitch, void* stream);
/* One pass of Pillow's box blur on a single-channel image (ImageFilter.GaussianBlur on mode L, UltimateSDUpscale.py:166-167, = three axis-1 passes
 * then three axis-0 passes with the box radius fr of gaussian_box_params): R = (int) fr, ww = (uint32)(16777216.0f / (fr * 2 + 1)),
 * fw = (2^24 - (2 R + 1) ww) / 2,
 *   out[x] = (ww * sum_{i = -R..R} in[clamp(x + i)] + fw * (in[clamp(x - R - 1)] + in[clamp(x + R + 1)]) + 2^23) >> 24,
 * indices clamped to the line.  0 <= fr < 256; lines shorter than the window work.  in and out must not overlap. */
int ldx_image_box_blur_pass(const uint8_t* in, int64_t in_pitch, int H, int W, int axis, float box_radius, uint8_t* out, int64_t out_pitch, void* stream);
/* process_images' paste + alpha_composite (UltimateSDUpscale.py:224-242) in place: for every pixel of the rectangle (x0, y0, w, h) of canvas
 * [H][W][C], with a = mask [H][W] at the same position, s = tile [h][w][C], d = canvas: a == 0 leaves d; otherwise
 *   coef1 = a * 255 * 255 * 128 / (a * 255 + 255 * (255 - a)), coef2 = 255 * 128 - coef1, t = s * coef1 + d * coef2 + (0x80 << 7),
 *   d = (((t >> 8) + t) >> 8) >> 7. */
int ldx_image_composite(uint8_t* canvas, int64_t canvas_pitch, int H, int W, int C, int x0, int y0, int w, int h,
                        const uint8_t* tile, int64_t tile_pitch, const uint8_t* mask, int64_t mask_pitch, void* stream);
/* img [H][W][C]: every byte of the rectangle (x0, y0, w, h) = value (ImageDraw.rectangle / Image.new for the tile masks, :471,514-518). */
int ldx_image_fill_rect(uint8_t* img, int64_t pitch, int H, int W, int C, int x0, int y0, int w, int h, int value, void* stream);

/* ---- fp32 canvas ops of the ADetailer path (DetailerForEach.do_detail, src/AutoDetailer/ADetailer.py:643-871) ----------------------------- */
/* What the reference does in torch on the CPU around the networks of one segment.  The canvas is fp32 [H][W][3] dense on the device and stays fp32
 * between segments; each product and each sum below is rounded on its own (no fused multiply-add), so the results are the floats of the numpy
 * statement of the same rules (lightdiffusion-next_amd/detailer.py).  Stateless, on the caller's stream, nothing is allocated. */
/* tensor2pil (tensor_util.py:18-40) of the rectangle (x0, y0, w, h) of the canvas, which must lie inside it: out [h][w][3] with a row pitch in bytes
 * = (uint8) trunc(clamp(v, 0, 1) * 255.0f), ldx_image_quantize's rule: the image ldx_image_resample_pass reads. */
int ldx_detail_crop_quantize(const float* canvas, int H, int W, int x0, int y0, int w, int h, uint8_t* out, int64_t out_pitch, void* stream);
/* torchvision's GaussianBlur as tensor_gaussian_blur_mask calls it (tensor_util.py:218-254): in fp32 [h][w], table fp32 [k][k] (k odd, <= 63; the host
 * builds it as the outer product of the normalised 1-D kernel, detailer.blur_table),
 *   out[y][x] = sum over (dy, dx) in row-major order of table[dy][dx] * in[reflect(y + dy - k/2)][reflect(x + dx - k/2)],
 * the accumulator starting at 0.0f, each tap one rounded product and one rounded add.  reflect has no edge repeat (-1 -> 1, n -> n - 2);
 * k / 2 >= h or k / 2 >= w is LDX_EINVAL (torch refuses the same padding).  in and out must not overlap. */
int ldx_detail_blur_mask(const float* in, int h, int w, const float* table, int k, float* out, void* stream);
/* tensor_paste (tensor_util.py:121-151) in place: the tile src [h][w][3] with mask [h][w], both dense, is put at (x0, y0), which must lie inside the
 * canvas; the tile is clipped at the canvas's right and bottom border.  With d the canvas value, s the tile's and m the mask's:
 *   t0 = 1.0f - m;  t1 = t0 * d;  t2 = m * s;  d = t1 + t2. */
int ldx_detail_paste(float* canvas, int H, int W, int x0, int y0, const float* src, const float* mask, int h, int w, void* stream);

/* ---- AutoHDR, the default post-effect of every pipeline exit (src/AutoHDR/ahdr.py:83-127, HDREffects.apply_hdr2) ------------------------- */
/* What the reference does in PIL + LittleCMS + numpy after the VAE, on B HWC images of the device, C = 3.  Every step is an integer rule or a single
 * float32 operation, so the results are the bytes of the numpy statement of the same rules (lightdiffusion-next_amd/hdr.py: autohdr_host), which
 * differ from Pillow's in about one byte of 10^4 (tests/golden/autohdr.META.txt).  Stateless: every buffer is the caller's, nothing is allocated,
 * nothing waits for the device; the launches are ordered on `stream` and can be captured in a graph.
 *
 * Tables: uint16 [33][33][33][4] (the fourth value is padding), 8-byte aligned, the first input channel on the first axis: what lcms's resampling
 * optimisation makes of an 8-bit transform (hdr.py: lcms_tables).  The read of input bytes (v0, v1, v2), per channel c:
 *   a = 32 * 257 * v,  fx = a + (a + 0x7FFF) / 0xFFFF,  i0 = fx >> 16,  r = fx & 0xFFFF,  i1 = min(i0 + 1, 32);
 * with the channels ordered by r, descending, node_0 = (i0, i0, i0) and node_k = node_k-1 with the k-th channel's coordinate raised to its i1,
 *   rest = sum_k (T[node_k] - T[node_k-1]) * r_k + 0x8001,  out16 = T[node_0] + ((rest + (rest >> 16)) >> 16)  (signed 64-bit, arithmetic shifts),
 *   out8 = (out16 * 65281 + 8388608) >> 24. */
/* out [H][W][3] = the read of `table` at in [H][W][3]; pitches in bytes, >= W * 3. */
int ldx_hdr_table(const uint8_t* in, int64_t in_pitch, int H, int W, const uint16_t* table, uint8_t* out, int64_t out_pitch, void* stream);
/* Bytes of workspace the whole effect needs for B images of H x W (LDX_EINVAL, negative, for a shape it refuses: B > 65535, H * W > 16 843 009). */
int64_t ldx_hdr_workspace_bytes(int B, int H, int W);
/* The whole effect.  Input: in_f32 dense fp32 [B][H][W][3], quantised as tensor2pil does, (uint8) trunc(clamp(255.0f * v, 0, 255)), OR in_u8
 * [B][H][W][3] with rows of in_pitch bytes and images H * in_pitch bytes apart; exactly one of the two is non-null.  Per image:
 *   lab = read of fwd at the bytes;  lab.L = lum_lut[lab.L] (256 bytes; hdr.py: luminance_lut);  rgb = read of inv at lab;
 *   grey(p) = (R * 19595 + G * 38470 + B * 7471 + 0x8000) >> 16  (Pillow's RGB -> L);  mean = (2 * sum grey(rgb) + n) / (2 n), n = H * W, in integers;
 *   blend(deg, v, f) = t <= 0 ? 0 : t >= 255 ? 255 : trunc(t),  t = (float) deg + f * ((float) v - (float) deg) in float32, product rounded before the sum;
 *   c = blend(mean, rgb, contrast_factor)  (ImageEnhance.Contrast, factor 1 + contrast);
 *   o = blend(grey(c), c, color_factor)    (ImageEnhance.Color, factor 1 + enhance_color * 0.2).
 * Output, each if non-null (at least one): out_u8 = o with rows of out_pitch bytes, images H * out_pitch apart; out_f32 dense = o / 255.0f, the
 * correctly rounded quotient (pil2tensor).  The sum is a uint32: H * W <= 16 843 009.  workspace: ldx_hdr_workspace_bytes(B, H, W) bytes, 4-aligned. */
int ldx_hdr_apply(const float* in_f32, const uint8_t* in_u8, int64_t in_pitch, int B, int H, int W, const uint16_t* fwd, const uint16_t* inv,
                  const uint8_t* lum_lut, float contrast_factor, float color_factor, void* workspace, uint8_t* out_u8, int64_t out_pitch, float* out_f32,
                  void* stream);

/* ---- SaveImage, the last stage of every pipeline exit (src/FileManaging/ImageSaver.py:79-220) ------------------------------------------------ */
/* What the reference does with numpy + Pillow + zlib after AutoHDR (clip(i * 255, 0, 255).astype(uint8), Image.fromarray, img.save(pnginfo=None,
 * compress_level=4)), on B HWC images of the device, C = 3: the finished PNG files.  The file is not Pillow's (zlib's hash chains are sequential); it
 * decodes to the same pixels, has a comparable size (tests/golden/png.META.txt) and is a pure function of the bytes: every step below is an integer
 * rule, so the results are the bytes of the numpy statement of the same rules (lightdiffusion-next_amd/png.py: png_host).  Stateless: every buffer
 * is the caller's, nothing is allocated, nothing waits for the device; the launches are ordered on `stream` and can be captured in a graph.
 *
 * Filter.  Per row the filter type t of 0 None, 1 Sub, 2 Up, 3 Average (floor), 4 Paeth, with bpp = 3 and zeros left of and above the image, whose
 *   residuals r (mod 256) have the smallest sum of (r < 128 ? r : 256 - r); ties go to the lowest type.  The filtered stream is H rows of the type byte
 *   and the 3 W residuals, N = H * (1 + 3 W) bytes; N <= 2^30.
 * Deflate.  The stream is cut into chunks of 16 384 bytes (the last may be shorter); each chunk becomes deflate blocks on its own and ends on a byte
 *   boundary.  Tokens: a position breaks when it is the chunk's first or its byte differs from the one before.  A position that does not break lies in
 *   a run; with a = the last break before it, R = the positions from a + 1 up to the next break or the chunk's end, k = its index among them: R < 4
 *   makes it a literal; otherwise the run is cut into pieces of 258 from its start, a piece shorter than 3 is literals, and any other piece is one
 *   match (length = the piece, distance 1) at its first position.  Breaks are literals.  Literal / length alphabet: the 286 symbols, counted with one
 *   end-of-block.  Code lengths (limit 15; 7 for the code-length code): the used symbols sorted by (count, symbol); Huffman's algorithm on two queues,
 *   a leaf before an internal node of equal weight; depths above the limit are set to it and, while the Kraft sum exceeds 1, one code of the limit
 *   leaves and the deepest shorter code moves one down, taking the leaver along; the lengths go to the symbols in sorted order, the rarest the longest;
 *   canonical codes.  Two distance codes of one bit each are declared, so distance 1 is the bit 0.  Header: HLIT = the last used symbol + 1 (at least
 *   257), HDIST = 2; the lengths, greedy from the left: at a zero, a run of >= 11 zeros is (18, min(run, 138)), of >= 3 is (17, run); at a length equal
 *   to the one before it, a run of >= 3 is (16, min(run, 6)); anything else the length itself; HCLEN trimmed to the last used, at least 4.  If the
 *   dynamic block's bytes (rounded up) are fewer than the chunk + 5, it is written, followed, except in the last chunk, by an empty stored block (000,
 *   pad, 00 00 FF FF); otherwise a stored block.  BFINAL is set in the last chunk's block.  The first chunk opens with the zlib header 78 01.
 * Container.  Signature; IHDR (W, H, 8, 2, 0, 0, 0); one IDAT per chunk; one IDAT of 4 bytes with the Adler-32 of the filtered stream; IEND; CRC-32s
 *   as PNG defines them.  No other chunks (the reference passes pnginfo=None).
 * Sizes: a chunk of n bytes makes at most n + 9, so a file is at most 63 + N + 21 * ceil(N / 16384) bytes: ldx_png_bound_bytes. */
/* Bytes of workspace ldx_png_encode needs for B images of H x W, and the largest file of one H x W image (LDX_EINVAL, negative, for a shape they
 * refuse: B > 65535, H or W < 1, N > 2^30). */
int64_t ldx_png_workspace_bytes(int B, int H, int W);
int64_t ldx_png_bound_bytes(int H, int W);
/* The whole encoder.  Input: in_f32 dense fp32 [B][H][W][3], quantised as the reference does, (uint8) trunc(clamp(255.0f * v, 0, 255)) (NaN -> 0), OR
 * in_u8 [B][H][W][3] with rows of in_pitch bytes and images H * in_pitch bytes apart (ldx_hdr_apply's out_u8 in place); exactly one of the two is
 * non-null.  Output: file b at out + b * out_stride (out_stride >= ldx_png_bound_bytes(H, W)), its length in out_len[b] (device, uint32 [B]); bytes
 * past the length are left alone.  workspace: ldx_png_workspace_bytes(B, H, W) bytes, 16-aligned. */
int ldx_png_encode(const float* in_f32, const uint8_t* in_u8, int64_t in_pitch, int B, int H, int W, void* workspace, uint8_t* out, int64_t out_stride,
                   uint32_t* out_len, void* stream);
/* The filter stage alone: filtered [B][H][1 + 3 W] (the stream of every image) and, if non-null, types [B][H]. */
int ldx_png_filter(const float* in_f32, const uint8_t* in_u8, int64_t in_pitch, int B, int H, int W, uint8_t* filtered, uint8_t* types, void* stream);
/* The deflate stage alone on n arbitrary device bytes (1 <= n <= 2^30): a complete zlib stream (78 01, the chunks as above, Adler-32) at out, at most
 * ldx_zlib_bound_bytes(n) = 6 + n + 9 * ceil(n / 16384) bytes, its length in out_len[0] (device).  workspace: ldx_zlib_workspace_bytes(n) bytes,
 * 16-aligned. */
int64_t ldx_zlib_workspace_bytes(int64_t n);
int64_t ldx_zlib_bound_bytes(int64_t n);
int ldx_zlib_deflate(const uint8_t* bytes, int64_t n, void* workspace, uint8_t* out, uint32_t* out_len, void* stream);

/* ---- single-op entry points (parity tests call the kernels through these) ----------------------- */
/* 16-bit tensors are device pointers to bf16/fp16 per `dtype`.  Layouts: see csrc/ldx_kernels.h.
 * Extent contract of every entry point of this section (and of the kernels behind them, which the engines hand strided views of one shared arena): an operand
 * means its LOGICAL extent only — rows [0, rows) and columns [0, cols) of an ld-strided matrix, keys [0, Mk), elements [0, n) of a vector.  A kernel reads
 * meaning only from, and writes only to, that extent: bytes in the ld padding behind a row and in rows outside [0, rows) belong to another tensor, may hold
 * anything, non-finite values included, and neither reach a result (a masked tail is selected away, not multiplied by zero) nor are written.  A fused view
 * (q|k|v, [K | V], [value | gate]) is one logical matrix.  tests/test_guard_bands_gpu.py holds every entry point below to this, bit for bit; the MX fp8 ones
 * (byte and E8M0 operands) are not covered by that test yet. */
int ldx_op_convert(const float* in_f32, void* out_16, int64_t n, int dtype, int to_f32, void* stream);
/* The Q8_0 expansion of ldx_load_tensor_q8_0 alone (csrc/q8.hip): n / 32 blocks of 34 bytes (2-byte aligned) -> out[n], n % 32 == 0.  out_dtype LDX_F16:
 * the fp16 value; LDX_BF16 / LDX_F32: that fp16 value converted (bf16 round-to-nearest-even; fp32 exact).  out is 16-byte aligned.  LDX_EINVAL otherwise. */
int ldx_op_dequant_q8_0(const void* blocks, int64_t n, int out_dtype, void* out, void* stream);
int ldx_op_gemm(const void* A, int lda, const void* W, int M, int N, int K, const float* bias,
                const float* rowvec, int rowvec_ld, int rows_per_batch, int geglu,
                const void* R, int ldr, void* C, int ldc, float* Cf, int ldcf, int dtype, void* stream);
/* MX fp8 operands for the block-scaled MFMA (OCP microscaling: blocks of 32 consecutive k share one E8M0 scale
 * 2^ceil(log2(amax/448)), elements are e4m3fn = x / scale rounded to nearest even; BASELINE config 4 "fp8 MFMA").
 * ldx_op_mx_quant: 16-bit X [rows][K] (stride ldx) -> Y bytes [rows][ldy] + scales: uint32 [K/128][scales_ld], byte j of
 * word [t][r] = scale of block 4 t + j of row r.  ldx_op_gemm_mx: C = act(A W^T + bias) (+ R) on such operands (A [M][K],
 * W [N][K]); fp32 accumulation; act as ldx_kernels.h GemmArgs::act; outputs 16-bit C and / or fp32 Cf — or, with C8 / SC
 * (N % 128 == 0, no R / C / Cf), the result quantised in the epilogue exactly as ldx_op_mx_quant would quantise the 16-bit
 * C: the operand of the next block-scaled GEMM without a separate pass. */
/* LayerNorm whose output is quantised as ldx_op_mx_quant would quantise the 16-bit Y (C % 128 == 0). */
int ldx_op_layernorm_mx(const void* X, int ldx, int rows, int C, float eps, const float* gamma, const float* beta,
                        void* Y8, int ldy8, void* S8, int s8_ld, int dtype, void* stream);
/* ---- MX fp8 attention for head dim 128 (csrc/attn_mx.hip; round 5: the Flux "fp8 MFMA" mode of BASELINE config 4 with QK^T and PV on the block-scaled
 * 32x32x64 MFMA instead of 16-bit).  No reference counterpart (BlackForest/Flux.py:18-33 runs SDPA in 16 bit): pinned by the stated rule only.
 *   Q, K: ldx_op_mx_quant's format on the [rows][H * 128] matrix — e4m3 bytes, one E8M0 scale per (row, head, 32 consecutive d), scale dwords [H][s_ld]
 *         (byte j of dword [h][row] = d block j).  ldx_op_qk_norm_rope_mx produces them from the fused q|k|v projection in one pass (QKNorm + RoPE +
 *         quantiser), bit-identical to the 16-bit rope followed by ldx_op_mx_quant.
 *   V:    ldx_op_mx_vt_quant — transposed, V8T [B][H][128 d][Lp] with Lp = L rounded up to 128, one scale per (d, 32 consecutive keys) in
 *         SV [B][H][Lp / 128][128 d] dwords (byte t = keys 32 t .. 32 t + 31 of that 128-key block); inside every 64-key step the bytes are in the MFMA's
 *         contraction order: byte k holds key 32 (k >> 5) + 8 ((k & 15) >> 2) + 4 ((k >> 4) & 1) + (k & 3).
 *   P:    2^(s c - m) with m = ceil of the scaled row maximum, updated lazily (an integer exponent: P <= 4), rounded to e4m3 at the fixed scale 2^-6; the row sums add the ROUNDED values (an all-ones row of V^T).
 * Output: 16-bit O [rows][ldo] (O8 == NULL) or MX fp8 O8 / SO as ldx_op_attention_mx writes them. */
int ldx_op_qk_norm_rope_mx(const void* QKV, int ld, int rows, int L, int H, const float* qscale, const float* kscale, const float* cosT, const float* sinT, float eps,
                           void* Q8, void* K8, int ld8, void* SQ, void* SK, int s_ld, int dtype, void* stream);
int ldx_op_mx_vt_quant(const void* V, int ldv, int B, int H, int L, void* V8T, void* SV, int Lp, int dtype, void* stream);
int ldx_op_attention_fp8(const void* Q8, int ldq8, const void* SQ, int sq_ld, const void* K8, int ldk8, const void* SK, int sk_ld, const void* V8T, const void* SV, int Lp,
                         void* O, int ldo, void* O8, int ldo8, void* SO, int so_ld, int B, int H, int Nq, int Mk, float scale, int dtype, void* stream);
/* Attention (head dim 128, no mask) whose output is quantised in the epilogue exactly as ldx_op_mx_quant would quantise the
 * 16-bit O [B*Nq][H*128]: O8 bytes (row stride ldo8) + scales uint32 [H][so_ld] (one word per row and head).  Needs
 * B * H * ceil(Nq / 128) >= 16 workgroups (smaller problems: ldx_op_attention + ldx_op_mx_quant). */
int ldx_op_attention_mx(const void* Q, int ldq, const void* K, int ldk, const void* V, int ldv, void* O8, int ldo8, void* SO, int so_ld,
                        int B, int H, int Nq, int Mk, float scale, int dtype, void* stream);
int ldx_op_mx_quant(const void* X, int ldx, int rows, int K, void* Y, int ldy, void* scales, int scales_ld, int dtype, void* stream);
int ldx_op_gemm_mx(const void* A8, int lda, const void* SA, int sa_ld, const void* W8, const void* SW, int sw_ld, int M, int N, int K,
                   const float* bias, int act, const void* R, int ldr, void* C, int ldc, float* Cf, int ldcf,
                   void* C8, int ldc8, void* SC, int sc_ld, int dtype, void* stream);
/* Two independent plain GEMMs C_i = A_i W_i^T + bias_i in ONE launch: the image and text token streams of a Flux double block each
 * meet their own weights (src/BlackForest/Flux.py:260-340 DoubleStreamBlock img_* / txt_* linears), and a
 * launch of its own for the 512-row text stream would leave most of the chip idle.  16-bit operands, or MX fp8 operands laid out as for
 * ldx_op_gemm_mx.  Large pairs run on the 256-row ping-pong tiles. */
int ldx_op_gemm2(const void* A1, int lda1, const void* W1, int M1, int N1, int K1, const float* bias1, void* C1, int ldc1,
                 const void* A2, int lda2, const void* W2, int M2, int N2, int K2, const float* bias2, void* C2, int ldc2, int dtype, void* stream);
int ldx_op_gemm2_mx(const void* A1, int lda1, const void* SA1, int sa_ld1, const void* W1, const void* SW1, int sw_ld1, int M1, int N1, int K1,
                    const float* bias1, void* C1, int ldc1,
                    const void* A2, int lda2, const void* SA2, int sa_ld2, const void* W2, const void* SW2, int sw_ld2, int M2, int N2, int K2,
                    const float* bias2, void* C2, int ldc2, int dtype, void* stream);
/* Read-only probe: which kernel ldx_op_gemm / ldx_op_gemm_mx / ldx_op_conv3x3[_skip] (M2 > 0: ldx_op_gemm2[_mx] with the second problem M2, N2, K2) and the engines'
 * plans would launch for a problem described by plain integers.  Launches nothing and touches no device.  mode 0 plain / 1 conv3x3 (Cin .. stride: the conv
 * geometry, K = 9 * Cin + the channels of a fused 1x1 skip); geglu as GemmArgs::geglu; splitk = K splits, -1: the planner's own choice; f8: MX fp8 operands,
 * c8: MX fp8 output, ln_fold: LayerNorm folded in.  gn_hw > 0 (one problem only): the output feeds a GroupNorm of gn_groups groups over images of gn_hw rows
 * whose statistics workspace holds gn_max_chunks chunks per image — the launch is the one the planner would make after asking for the fused statistics.
 * out[0 .. 9] = kernel family (0 register-staged tile, 1 the same for two problems, 2 ping-pong, 3 ping-pong for two problems, 4 ring, 5 patch-resident conv,
 * 6 .. 9 = 0 .. 3 with MX fp8 operands), tile rows BM, tile columns BN (as instantiated), WM (register-staged tiles: threads / 128), f8, ln_fold, K splits in effect,
 * reduce (0 none, 1 reduce launch, 2 reduce launch + GroupNorm statistics, 3 inside the kernel), kernel launches, GroupNorm chunks per image (0: statistics not fused). */
int ldx_op_gemm_pick(int M, int N, int K, int mode, int geglu, int splitk, int f8, int c8, int ln_fold,
                     int Cin, int Hin, int Win, int Hout, int Wout, int stride, int M2, int N2, int K2,
                     int gn_hw, int gn_groups, int gn_max_chunks, int32_t* out);
/* Read-only probe: which kernel ldx_op_attention / ldx_op_attention_bias / ldx_op_attention_mx and the engines' plans would launch for a problem described by plain
 * integers.  Launches nothing and touches no device.  causal / bias / o8 (MX fp8 output, D = 128 only) / knorm_ws (the key-norm workspace of the pipelined kernels) say
 * what is present; ldq .. ldo are the row strides in elements (ldo also the byte stride of an MX fp8 output); operands count as 16-byte aligned.
 * out[0 .. 12] = kernel family (0 attn_kernel on 16x16 MFMAs, 1 attn32_kernel, 2 attn32ap_kernel, 3 attn32g_kernel, 4 attn40p_kernel, 5 attn128p_kernel, 6 attn512_kernel),
 * three template arguments as instantiated (attn_kernel KS, DT, QT; attn32g_kernel NKS, NDT, ONES; attn32_kernel KVB, VAR; attn32ap_kernel VAR; else 0), attn32g's K prefetch
 * ring on / off, queries per workgroup, threads per workgroup, workgroups, dynamic LDS bytes, key-norm launch first (0 / 1), key splits in effect (attn512, with the
 * workspace the planner gives it; > 1: a merge launch follows), MX fp8 output allowed for the shape (0 / 1), kernel launches. */
int ldx_op_attn_pick(int B, int H, int Nq, int Mk, int D, int causal, int bias, int o8, int ldq, int ldk, int ldv, int ldo, int knorm_ws, int32_t* out);
/* Read-only probe: the stage choice of one SpatialTransformer of a UNet plan (xf_pick).  Launches nothing and touches no device.  C level width, B evaluation
 * batch, HW pixels per image, Mc context tokens, share the batch of the shared CFG prefix (0 = none), ln_fold whether folded LayerNorm weights were loaded,
 * gn_stats_chunks the statistics rows per image the producer of the transformer's input wrote (0 = none).
 * out[0 .. 19] = LayerNorms folded (0 / 1), norm + proj_in as one rowgemm launch (0 / 1), proj_out stage; then for the first block and for every later block eight
 * values each: norm1 + q|k|v stage, to_out 1 stage, cross-attention as one xattn_block launch (0 / 1), norm2 + q stage, to_out 2 stage, feed-forward as one ff_block
 * launch (0 / 1), norm3 + GEGLU projection stage, ops of the block; last the ops of norm + proj_in and proj_out together.  Stages: 0 tile GEMM, 1 row-block launch
 * (rowgemm), 2 one GEMM on folded weights, 3 LayerNorm + GEMM, 4 affine-free LayerNorm + GEMM on folded weights.  norm2 / to_out 2 / norm3 stages say what runs when
 * the one-launch sub-block does not.  An op is one launch unless gemm_pick / attn_pick say more (split-K reduce, key norms). */
int ldx_op_xf_pick(int C, int heads, int B, int HW, int Mc, int share, int ln_fold, int gn_stats_chunks, int32_t* out);
int ldx_op_conv3x3(const void* X, int ldx, const void* W, int B, int Hin, int Win, int Cin, int Cout,
                   int stride, int Hout, int Wout, int resize_to_out, const float* bias,
                   const float* rowvec, int rowvec_ld, const void* R, int ldr, void* Y, int ldy,
                   int dtype, void* stream);
/* Upsample1 (ResBlock.py:75-138: F.interpolate(nearest, x2) then conv3x3, pad 1) in PHASE form: output pixel (2 i + py, 2 j + px) sees a 2 x 2 neighbourhood of
 * the stored image, so the op runs as four 2 x 2 convs, one per output parity, whose weights are sums of 1, 2 or 4 of the 3 x 3 taps (fp32 sums, rounded once):
 * 4/9 of the arithmetic of ldx_op_conv3x3(resize_to_out = 1), which computes the same thing.  X [B][Hin][Win][ldx] and W9 — the packed 9-tap matrix
 * [Cout][(ky * 3 + kx) * Cin + ci] that ldx_op_conv3x3 takes — in `dtype`, bias [Cout] fp32 (required), Y [B][2 Hin][2 Win][ldy].  The phase weights are derived
 * into the single-op workspace on every call (one stream per device at a time, as for the split-K ops).  LDX_EINVAL where the form does not exist:
 * Win % 16, Cin % 64 or Cout % 16 != 0.  The UNet engine derives the phase weights once and takes the form where it pays (LDX_UPCONV_PHASE=0: never). */
int ldx_op_upconv2x(const void* X, int ldx, const void* W9, int B, int Hin, int Win, int Cin, int Cout, const float* bias, void* Y, int ldy, int dtype, void* stream);
/* ResBlock1 tail (ResBlock.py:315-335) as ONE implicit GEMM: Y = conv3x3(X, W[:, :9*Cin]) + X2 W[:, 9*Cin:]^T + bias, i.e. conv2(h) +
 * skip_connection(x) with W = [Cout][ky][kx][Cin | Cin2] and the two biases summed; stride 1, pad 1, X2 rows = output rows. */
int ldx_op_conv3x3_skip(const void* X, int ldx, const void* X2, int ldx2, int Cin2, const void* W, int B, int H, int Wd, int Cin, int Cout,
                        const float* bias, void* Y, int ldy, int dtype, void* stream);
int ldx_op_groupnorm(const void* X, int ldx, void* Y, int ldy, int B, int HW, int C, int G, float eps, int silu,
                     const float* gamma, const float* beta, float* workspace, int dtype, void* stream);
int64_t ldx_op_groupnorm_workspace_floats(int B, int G);
/* ---- test surface: GroupNorm statistics written by the launch in front of the GroupNorm ---------------------------------------------------------
 * Almost every GroupNorm of a production plan skips its own statistics pass: its producer writes, next to the 16-bit output, the sum and the sum of
 * squares of the values AS STORED, per (image, chunk of the image's rows, group), into
 *     partial [B][nchunk][G][2] fp32 = (sum, sum of squares),  B = rows / HW images of HW rows, nchunk chunks per image,
 * and the GroupNorm folds those rows in a fixed order (deterministic; GroupNormArgs::partial, csrc/ldx_kernels.h).  The engines plan this in
 * Engine::fuse_gn_stats; the four entry points below build the same launch arguments and ask the same host rules (gemm_gn_fuse, rowgemm_gn_chunks), so
 * a test reaches every producer and both consumers one op at a time.  Which rows make chunk c of an image depends on the kernel that runs
 * (ldx_op_gemm_pick shows it): tile epilogues BM consecutive rows; the split-K reduce launch HW / nchunk consecutive rows; the patch-resident conv
 * (N = 128) the 16-row x 32-column pixel tiles in row-major tile order; the row-block kernel 128 (K = 320) or 64 (K = 640) consecutive rows.
 * max_chunks: the rows per image `partial` has room for; at most B * max_chunks rows are written, *nchunk_out = the chunks per image in effect, and rows
 * behind B * nchunk are left alone.  Where the launch cannot produce the statistics — the kernel or tile picked has no such output stage, the chunk
 * count exceeds max_chunks, or the consumer would be the one-launch small GroupNorm, which takes no producer rows — the answer is LDX_EINVAL with
 * NOTHING launched and nothing written: the plain op (ldx_op_conv3x3 / ldx_op_gemm / ldx_op_rowgemm) is the launch the planner makes then.
 * Split-K launches use the single-op workspace: one stream per device at a time, as for the plain ops. */
/* ldx_op_conv3x3 (arguments as there), optionally with the fused 1x1 skip of ldx_op_conv3x3_skip (X2 [rows][ldx2], Cin2 channels, W = [Cout][9 Cin | Cin2];
 * Cin2 = 0: none; with it stride 1, output extent = input extent, no resize), as the producer of a GroupNorm(gn_groups) over Y [B][Hout * Wout][Cout].
 * dup_rows != 0: every row m of Y is also stored at row m + dup_rows (GemmArgs::dup_rows, the shared CFG prefix) — Y then needs dup_rows + B * Hout * Wout
 * rows, and the statistics still count every row once. */
int ldx_op_conv3x3_gn(const void* X, int ldx, const void* X2, int ldx2, int Cin2, const void* W, int B, int Hin, int Win, int Cin, int Cout,
                      int stride, int Hout, int Wout, int resize_to_out, const float* bias, const float* rowvec, int rowvec_ld,
                      const void* R, int ldr, void* Y, int ldy, int64_t dup_rows, float* partial, int gn_groups, int max_chunks, int32_t* nchunk_out,
                      int dtype, void* stream);
/* ldx_op_gemm without GEGLU (arguments as there; the 16-bit C is required) as the producer of a GroupNorm(gn_groups) over C [M / gn_hw][gn_hw][N]. */
int ldx_op_gemm_gn(const void* A, int lda, const void* W, int M, int N, int K, const float* bias, const float* rowvec, int rowvec_ld, int rows_per_batch,
                   const void* R, int ldr, void* C, int ldc, float* Cf, int ldcf, int gn_hw, float* partial, int gn_groups, int max_chunks, int32_t* nchunk_out,
                   int dtype, void* stream);
/* ldx_op_rowgemm with pro 0 or 1 (arguments as there) as the producer of a GroupNorm(32) over Y [M / HW][HW][N]: gn_out is `partial` above with
 * nchunk = HW / 128 (K = 320) or HW / 64 (K = 640), dup_rows as for ldx_op_conv3x3_gn.  The planner's conditions for a row-block producer: N == K, M a multiple
 * of HW, HW a multiple of the row block — LDX_EINVAL otherwise, as above. */
int ldx_op_rowgemm_gn(const void* X, int ldx, void* Y, int ldy, int64_t M, int N, int K, const void* W, const float* bias, const void* R, int ldr,
                      int pro, const float* gamma, const float* beta, float eps, int HW, int64_t dup_rows, float* gn_out, int max_chunks, int32_t* nchunk_out,
                      int dtype, void* stream);
/* ldx_op_groupnorm without its statistics pass: apply from the caller's rows partial [B][stats_chunks][G][2] (any split of each image's HW rows into
 * stats_chunks chunks, 1 <= stats_chunks <= 32768).  More than 256 rows per image are first folded, in a fixed order, into 64 rows per image that
 * the launch writes BEHIND the caller's rows: partial must hold ldx_op_groupnorm_stats_floats(B, G, stats_chunks) floats = the rows + that fold target. */
int ldx_op_groupnorm_stats(const void* X, int ldx, void* Y, int ldy, int B, int HW, int C, int G, float eps, int silu,
                           const float* gamma, const float* beta, float* partial, int stats_chunks, int dtype, void* stream);
int64_t ldx_op_groupnorm_stats_floats(int B, int G, int stats_chunks);
int ldx_op_layernorm(const void* X, int ldx, void* Y, int ldy, int rows, int C, float eps,
                     const float* gamma, const float* beta, int dtype, void* stream);
int ldx_op_attention(const void* Q, int ldq, const void* K, int ldk, const void* V, int ldv, void* O, int ldo,
                     int B, int H, int Nq, int Mk, int D, float scale, int causal, int dtype, void* stream);
/* Cross-attention sub-block of a BasicTransformerBlock as ONE kernel (reference: transformer.py:186-245 attn2 + Attention.py:100-124):
 * H[m][:] += to_out(softmax(to_q(LayerNorm(H[m][:])) . K_b^T * scale) . V_b) + bo, in place, m in [0, M), image b = m / N.  Wq / Wo [C][C]
 * 16-bit (row = output feature), K / V = the projected context (rows b * Mk + key, head h at columns h * (C / heads)).  Shapes the kernel
 * takes: C = 320, heads = 8, Mk <= 80, N % 128 == 0, M % N == 0 — anything else returns LDX_EINVAL (use the separate ops). */
int ldx_op_xattn_block(void* H, int ldh, int64_t M, int N, int C, int heads, const float* ln_gamma, const float* ln_beta, float eps,
                       const void* Wq, const void* Wo, const float* bo, const void* K, int ldk, const void* V, int ldv, int Mk,
                       float scale, int dtype, void* stream);
/* Feed-forward sub-block of a BasicTransformerBlock as ONE kernel (reference: transformer.py:19-70, 240-244; Activation.py:6-31):
 * H[m][:] += W2 . (a * gelu_erf(g)) + b2 with [a | g] = W1 . LayerNorm(H[m][:]) + b1, in place.  W1 [2 * inner][C] and b1 in the engine's GEGLU
 * row layout: slab s (64 rows) = value rows of inner features 32 s .. 32 s + 31, then their gate rows (reference rows i and inner + i);
 * W2 [C][inner].  Shapes the kernel takes: C = 320, inner = 1280 — anything else returns LDX_EINVAL (use the separate ops). */
int ldx_op_ff_block(void* H, int ldh, int64_t M, int C, int inner, const float* ln_gamma, const float* ln_beta, float eps,
                    const void* W1, const float* b1, const void* W2, const float* b2, int dtype, void* stream);
/* Row-block GEMM with a normalisation prologue (csrc/rowgemm.hip): Y[m][0:N) = pro(X[m][0:K)) . W^T + bias (+ R[m][:]), K = 320 or 640, N a multiple of K, W [N][K].
 * pro 0: identity; 1: LayerNorm(gamma, beta, eps) (transformer.py:199 norm1 in front of to_q|k|v); 2: GroupNorm apply, 32 groups
 * (transformer.py:361-367 norm in front of proj_in) with the statistics given as partial sums partial[b][chunk][32][2] = (sum, sum of squares)
 * over any split of image b's HW pixels (HW a multiple of 128 at K = 320, of 64 at K = 640) into `nchunk` <= 256 chunks (what the producing
 * conv's epilogue writes).  Other shapes: LDX_EINVAL. */
int ldx_op_rowgemm(const void* X, int ldx, void* Y, int ldy, int64_t M, int N, int K, const void* W, const float* bias, const void* R, int ldr,
                   int pro, const float* gamma, const float* beta, float eps, const float* partial, int nchunk, int HW, int dtype, void* stream);
/* attention with an additive fp32 score bias [H][>= Nq][bias_ld] (bias_ld >= Mk rounded up to 64), added before the scale */
int ldx_op_attention_bias(const void* Q, int ldq, const void* K, int ldk, const void* V, int ldv, void* O, int ldo,
                          int B, int H, int Nq, int Mk, int D, float scale, const float* bias, int bias_ld,
                          int64_t bias_head_stride, int dtype, void* stream);
int ldx_op_skinny(const float* x, int ldx, const void* W, const float* bias, float* out, int ldo,
                  int M, int N, int K, int in_act, int out_act, int dtype, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* LDX_H */
