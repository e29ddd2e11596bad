// ldx — MI355X (gfx950 / CDNA4) kernels for the LightDiffusion-Next denoising hot path.
// Internal header: argument structs + host launchers for every device kernel.
// All activations are NHWC ("token-major") 16-bit (bf16 or fp16) with an explicit row stride
// (ld*) so that channel-concatenation (reference: torch.cat([h, hs.pop()], 1), unet.py:750)
// is a pointer offset, never a copy.  Accumulation, norm statistics and softmax are fp32.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <functional>

#include "ldx_geometry.h"

namespace ldx {

enum DType : int { DT_BF16 = 0, DT_F16 = 1 };

// One-time hipFuncSetAttribute(MaxDynamicSharedMemorySize) PER DEVICE (function attributes are per device: a process that
// builds engines on two GPUs must raise the limit on both).  One DevOnce per launcher instantiation; bit = device ordinal.
struct DevOnce { unsigned long long mask = 0; };
inline void set_dyn_lds(DevOnce& once, const void* fn, int bytes) {
    int dev = 0;
    (void)hipGetDevice(&dev);
    const unsigned long long bit = 1ull << (dev & 63);
    if (__atomic_load_n(&once.mask, __ATOMIC_RELAXED) & bit) return;
    (void)hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
    __atomic_fetch_or(&once.mask, bit, __ATOMIC_RELAXED);
}

// ---------------------------------------------------------------------------------------------
// GEMM / implicit-GEMM convolution:  C[M][N] = epilogue( A[M][K] * W[N][K]^T )
// mode 0: A is a plain row-major matrix (row stride lda), K % 64 == 0.
// mode 1: A is an NHWC image [B][Hin][Win][lda]; 3x3 window, pad 1, stride 1|2, optional
//         nearest-neighbour resize of the input to (Hv,Wv) fused into the gather
//         (reference Upsample1: F.interpolate(nearest) then conv, ResBlock.py:75-138).
//         K = 9*Cin with k = (ky*3+kx)*Cin + ci, Cin % 64 == 0.
// Epilogue (all optional, applied in this order): + bias[n], + rowvec[(m / rows_per_batch)][n],
//         GEGLU pairing (out = a * gelu_erf(g); reference cond/Activation.py:6-31),
//         + R[m][n] residual, store 16-bit C (ldc) and/or fp32 Cf (ldcf).
struct GemmArgs {
    const void* A;  int lda;
    const void* W;                 // [N][K] 16-bit, K contiguous
    int M, N, K;
    int mode;                      // 0 plain, 1 conv3x3
    int Cin, Hin, Win;             // conv: stored input image
    int Hv, Wv;                    // conv: virtual (resized) input extent seen by the 3x3 window
    int Hout, Wout, stride;        // conv: output extent
    int resize;                    // conv: 1 if (Hv,Wv) != (Hin,Win) -> nearest gather
    // conv: optional second input read as a 10th "tap" (1x1, same pixel as the output row): K = 9*Cin + Cin2, W = [N][9*Cin | Cin2].
    // ResBlock1's out = conv2(h) + skip_connection(x) (ResBlock.py:315-335) becomes ONE implicit GEMM: no separate 1x1 launch, no
    // write + re-read of its result.  A2 rows are the output rows ([M][lda2]); stride 1 only.
    const void* A2; int lda2; int Cin2;
    int pad0;                      // conv: 1 -> no top/left padding (VAE Downsample: F.pad (0,1,0,1) + stride-2 conv, VariationalAE.py:224-254)
    const float* bias;             // [N] or null
    const float* rowvec; int rowvec_ld; int rows_per_batch;   // per-batch channel vector or null
    int geglu;                     // 1: N is 2*inner with slab-interleaved (a|g) rows, out width N/2: a * gelu_erf(g); 2: a * gelu_tanh(g)
    int act;                       // 0 none, 1 quick-GELU x*sigmoid(1.702x) after bias (CLIP MLP, clip/Clip.py:74-77),
                                   // 2 tanh-GELU (Flux MLPs, BlackForest/Flux.py:279,388), 3 LeakyReLU(0.2) (ESRGAN, USDU_util.py:7-10)
    const float* gate; int gate_ld; // per-batch channel gate (Flux adaLN): v *= gate[(m / rows_per_batch)][n] before + R
    const void* R; int ldr;        // residual (16-bit) or null
    float oscale;                  // != 0: v *= oscale before + R   (ResidualDenseBlock_5C: x5 * 0.2 + x, RDRB.py:205)
    const void* R2; int ldr2; float oscale2;   // R2 != null: v = v * oscale2 + R2 after + R  (RRDB: out * 0.2 + x, RDRB.py:76)
    void* C; int ldc;              // 16-bit output or null
    float* Cf; int ldcf;           // fp32 output or null
    // f8 = 1 (plain mode only): A and W are MX fp8 (OCP e4m3fn bytes, K % 128 == 0) with one E8M0 scale per 32 consecutive
    // k; scales are stored K-tile-major as dwords SA[K/128][sa_ld] (byte j of dword [kt][m] = block 4*kt + j of row m)
    int f8; const uint32_t* SA; int sa_ld; const uint32_t* SW; int sw_ld;
    // C8 != null: the output is written as MX fp8 instead of 16-bit C (bias and act only; N % 32 == 0, tile width 64 or 128):
    // bytes C8[m][c8_col + n], scales SC (SA layout, row stride sc_ld) for the blocks (c8_col + n) / 32 — the operand of the
    // next block-scaled GEMM, produced without a separate quantisation pass
    void* C8; int ldc8; int c8_col; uint32_t* SC; int sc_ld;
    // ln_c1 != null: a LayerNorm over the K columns is folded into this plain 16-bit GEMM (no split-K): A = the UN-normalised rows,
    // W = W .* gamma, bias = W beta + b, ln_c1[n] = sum_k W[n][k] of the stored 16-bit values.  The kernel accumulates each row's
    // sum / sum of squares from its A fragments and stores  rstd[m] * (acc - mean[m] * ln_c1[n]) + bias[n]  (then GEGLU etc.)
    const float* ln_c1; float ln_eps;
    int splitk; float* ws;         // splitk > 1: K range split over `splitk` workgroups per tile; fp32 partials go to
                                   // ws[splitk][M][N] and a second kernel reduces them and applies the epilogue ...
    unsigned* sk_count;            // ... unless gemm_sk_fixup(a): sk_count points at zeroed per-tile counters (SK_COUNTERS of them, left at zero by every
                                   // launch) and splitk <= SK_FIXUP_MAX_S: then the partials go to private per-(tile, split) slabs — ws needs
                                   // gemm_sk_ws_floats() floats — and the LAST workgroup to finish a tile sums them in split order and runs the fused
                                   // epilogue itself (round 4: no reduce launch; gemm_common.h)
    // gn_partial != null: the consumer of C is a GroupNorm over the same [B][gn_hw][N] tensor (gn_cpg channels per group, gn_G groups): every
    // tile also writes the sum / sum of squares of the 16-bit values it stores, per group, to gn_partial[b][tile row][group][2] with
    // gn_nchunk tile rows per batch image — GroupNormArgs::partial's layout, so the GroupNorm skips its statistics pass (one full read of the
    // activation).  Only set by gemm_gn_fuse() below: no split-K / GEGLU / MX output, tile width % gn_cpg == 0, gn_hw % tile height == 0.
    float* gn_partial; int gn_cpg, gn_G, gn_hw, gn_nchunk;
    // dup_rows != 0: every 16-bit row m of C is ALSO stored at row m + dup_rows (same columns).  The shared CFG prefix (Engine::plan, share): the
    // ops in front of the first cross-attention run on one half of the [uncond; cond] batch, and what later full-batch ops read of their results
    // (skip connections, the residual stream) is written for both halves by the producer — no copy launch, no re-read.
    long dup_rows;
    int ep_general;                // experiment switch (LDX_EP_GENERAL=1, set by launch_gemm): the general output stage for every epilogue (A/B against the lean paths of gemm_common.h)
    // up2x != 0 (conv mode, stride 1; 1 / 2: tile rows band-major / phase-major, gemm_pp.inc): the nearest-2x upsample + 3x3 conv of Upsample1 in PHASE form.  Output pixel (2 i + py, 2 j + px) sees a 2 x 2 neighbourhood of the
    // stored image, so the op is four 2 x 2 convs, one per output parity: W = the phase weights [4][N][4 * Cin] (weight_layout.h up_phase_group, derived from the packed
    // 9-tap matrix), K = 4 * Cin, (Hin, Win) = (Hv, Wv) = the stored extent, (Hout, Wout) = twice that, M = B * Hout * Wout as for the 9-tap op.  One launch of the
    // ping-pong kernel's MODE 2 covers the four phases; bias is the only epilogue operand.  gemm_upconv_phase() below builds these arguments from the 9-tap op's.
    int up2x;
};
// Can the 9-tap conv `g` (as op_conv / ldx_op_conv3x3 build it, W still the packed 9-tap matrix) run in phase form?  Geometry (an exact x2 of a stored image whose rows
// are whole 16-pixel blocks) and epilogue (bias only, 16-bit output, no split-K).  If so `*ph` = the phase-form arguments, but for W, which the caller points at the
// phase weights and may ask for the phase-major tile order (up2x = 2).  planned: the planner's question — also no K splits chosen for the 9-tap op and no dispatch switch that takes the ping-pong kernels away.
bool gemm_upconv_phase(const GemmArgs& g, bool planned, GemmArgs* ph);
// The phase weights of one up conv: Wp[4][N][4 * Cin] from the packed 9-tap W9[N][9 * Cin] (both 16-bit, on the device); weight_layout.h up_phase_group
struct UpPhaseArgs { const void* W9; void* Wp; int N, Cin; DType dt; };
// ... with every byte defined, the tail padding too (the launch recorders, tests/tools/plan_trace.py and tests/test_op_trace_cpu.py, compare argument bytes)
inline UpPhaseArgs up_phase_args(const void* W9, void* Wp, int N, int Cin, DType dt) {
    UpPhaseArgs a; memset(&a, 0, sizeof(a));
    a.W9 = W9; a.Wp = Wp; a.N = N; a.Cin = Cin; a.dt = dt;
    return a;
}
void launch_up_phase(const UpPhaseArgs& a, hipStream_t s);
// Can launch_gemm(a) produce GroupNorm statistics for a consumer GroupNorm(G groups) over [B][HW][a.N]?  If yes, returns the number of
// tile rows per batch image (the consumer's chunk count) and fills a.gn_* except gn_partial; 0 = not fusable (the GroupNorm runs its own pass).
// It asks gemm_pick() below for the kernel and applies that kernel's epilogue conditions; launch_gemm() holds a set gn_partial to the same answer and aborts otherwise.
int gemm_gn_fuse(GemmArgs& a, int HW, int G, int max_chunks);
bool gemm_gn_fuse_enabled();                                // LDX_GN_FUSE != 0 (the engine's row-block producers ask)
void launch_gemm(const GemmArgs& a, DType dt, hipStream_t s);
// two independent plain GEMMs (mode 0, no split-K / GEGLU, both 16-bit or both MX) as one launch of 128x128 tiles
void launch_gemm2(const GemmArgs& a, const GemmArgs& b, DType dt, hipStream_t s);
int gemm_choose_splitk(int M, int N, int K, bool geglu);   // 1 = no split
// Which kernel launch_gemm(a) — launch_gemm2(a, *b) with a second problem — runs: pure host arithmetic (gemm_pick.cpp) over the arguments and the LDX_* dispatch switches, which are
// read once when the library loads (ldx_switches.h: GemmSwitches).  The launchers switch on it, the planner asks it (gemm_gn_fuse, Engine::n_launches), ldx_op_gemm_pick shows it to tests.
enum GemmFamily : int { GF_TILE = 0, GF_TILE2, GF_PP, GF_PP2, GF_RING, GF_CONV_PATCH, GF_TILE_MX, GF_TILE2_MX, GF_PP_MX, GF_PP2_MX };      // register-staged tile (gemm.hip), ping-pong (gemm_pp.inc), ring, patch-resident conv; 2: two problems; MX: fp8 operands
enum GemmReduce : int { RED_NONE = 0, RED_LAUNCH, RED_LAUNCH_GN, RED_IN_KERNEL };      // split-K partials: no split / reduce launch / reduce launch that also writes the GroupNorm statistics / last workgroup of a tile
struct GemmPick {
    GemmFamily family;
    int bm, bn;                    // the tile as the instantiation has it (not as the heuristics asked for it)
    int wm;                        // register-staged tiles: workgroup threads / 128; 0 elsewhere
    bool f8, lnf;                  // MX fp8 operands; LayerNorm folded in
    int S;                         // K splits in effect (1: none)
    GemmReduce reduce;
    int launches;                  // kernel launches in all (0: empty problem)
};
GemmPick gemm_pick(const GemmArgs& a, const GemmArgs* b = nullptr);
// The shape rules gemm_pick asks, and what launch_gemm asks back (all of it host arithmetic in gemm_pick.cpp, next to the pick):
bool gemm_ring_ok(int M, int N, int K, bool plain, int splitk);      // gemm_ring.hip: 64 x 160 LDS-DMA ring tiles for mid-size plain GEMMs
bool conv_patch_ok(const GemmArgs& a);                               // conv_patch.hip: patch-resident 3x3 conv for N = 32 / 64 / 128 (ESRGAN, VAE last level) and the 3 / 4-channel tails
int conv_patch_gn_chunks(const GemmArgs& a, int HW, int G);
int splitk_gn_geom(const GemmArgs& a, int HW, int G, int max_chunks, int* R_out);      // geometry of the reduce + GroupNorm-statistics launch
void gemm_gn_check(const GemmArgs& a);                               // aborts unless a set GemmArgs::gn_partial carries the geometry gemm_gn_fuse gives this very launch
constexpr int SK_FIXUP_MAX_S = 4;                          // in-kernel fix-up up to this many splits (the last arriver reads S slabs back to back); above: reduce launch
constexpr int SK_COUNTERS = 8192;                          // per-tile counters a caller keeps for it
#ifdef LDX_SK_FIXUP_BUILD
inline size_t gemm_sk_ws_floats(int M, int N, int S) { return (size_t)S * ((size_t)M + 255) * ((size_t)N + 255); }      // slabs of whole tiles (tile <= 256 x 256), or the [S][M][N] layout
#else
inline size_t gemm_sk_ws_floats(int M, int N, int S) { return (size_t)S * (size_t)M * (size_t)N; }      // [S][M][N] fp32 partials for the reduce launch (the slab layout only exists in fix-up builds)
#endif
bool gemm_sk_fixup(const GemmArgs& a);                     // will launch_gemm(a) reduce inside the kernel?  (opt-in: LDX_SK_FIXUP=1; measured slower than the reduce launch)

// ---- where launch arguments are built: the planner's op emitters (engine.cpp) and the single-op C ABI (capi.cpp) both come here ----
// What a builder takes scratch from: bytes(n) = n bytes that live for the launch being built (the engine: an arena range; the single-op entry points: their one
// per-device buffer, so no launch may ask twice, and none does), counters() = the zeroed split-K tile counters.
struct Scratch { std::function<void*(size_t)> bytes; std::function<unsigned*()> counters; };
// The base fill of a plain GEMM / a 3x3 conv (K = 9 * Cin, + Cin2 with GemmArgs::A2; resize_to_out: the window walks the input resized to the output extent), every
// other byte zero, the padding too (the launch recorders compare argument bytes).  The caller adds the epilogue operands, then gemm_attach_splitk.
inline GemmArgs gemm_linear_args(const void* A, int lda, const void* W, int M, int N, int K) {
    GemmArgs g; memset(&g, 0, sizeof(g));
    g.A = A; g.lda = lda; g.W = W; g.M = M; g.N = N; g.K = K; g.rows_per_batch = 1;
    return g;
}
inline GemmArgs gemm_conv_args(const void* X, int ldx, const void* W, int B, int Hin, int Win, int Cin, int N, int K, int stride, int Hout, int Wout, bool resize_to_out) {
    GemmArgs g = gemm_linear_args(X, ldx, W, B * Hout * Wout, N, K);
    g.mode = 1; g.Cin = Cin; g.Hin = Hin; g.Win = Win; g.Hout = Hout; g.Wout = Wout; g.stride = stride;
    g.Hv = resize_to_out ? Hout : Hin; g.Wv = resize_to_out ? Wout : Win;
    g.resize = (g.Hv != Hin || g.Wv != Win) ? 1 : 0;
    g.rows_per_batch = Hout * Wout;
    return g;
}
// MX fp8 operands: A (already the e4m3 bytes) with scales SA, W8 with scales SW
inline void gemm_mx_operands(GemmArgs& g, const uint32_t* SA, int sa_ld, const void* W8, const uint32_t* SW, int sw_ld) { g.f8 = 1; g.SA = SA; g.sa_ld = sa_ld; g.W = W8; g.SW = SW; g.sw_ld = sw_ld; }
// The K splits of `g` as it stands, their workspace and counters: an MX fp8 K-tile is twice as deep, GEGLU and MX output never split.  Whoever changes the epilogue
// afterwards may only lower splitk to 1 (the workspace then stays in the arguments, unused) ...
inline void gemm_attach_splitk(GemmArgs& g, const Scratch& s) {
    g.splitk = g.C8 ? 1 : gemm_choose_splitk(g.M, g.N, g.f8 ? g.K / 2 : g.K, g.geglu != 0);
    if (g.splitk > 1) { g.ws = (float*)s.bytes(gemm_sk_ws_floats(g.M, g.N, g.splitk) * 4); g.sk_count = s.counters(); }
}
// ... and must, for the epilogues launch_gemm has no split-K form of: such a launch would compute a K slice and never reduce it
inline bool gemm_splitk_ok(const GemmArgs& g) { return g.splitk <= 1 || !(g.ln_c1 || g.gate || g.C8 || g.geglu || g.up2x); }
// 256-row ping-pong tiles (gemm_pp.hip; GemmPick family GF_PP* ): bn = the tile width as gemm_pick gives it, lnf = GemmArgs::ln_c1 fold, S = K splits
void launch_gemm_pp(const GemmArgs& a, int bn, bool lnf, int S, DType dt, hipStream_t s);
void launch_gemm_pp2(const GemmArgs& a, const GemmArgs& b, int bn, DType dt, hipStream_t s);

// MX quantisation of a 16-bit [rows][K] matrix (row stride ldx): per 32-element block, scale = 2^ceil(log2(amax / 448))
// (E8M0, no clipping), y = e4m3fn(x / scale).  Y [rows][ldy] bytes; S as GemmArgs::SA (dwords [K/128][s_ld]).  K % 128 == 0.
struct MxQuantArgs { const void* X; int ldx; int rows, K; void* Y; int ldy; uint32_t* S; int s_ld; };
void launch_mx_quant(const MxQuantArgs& a, DType dt, hipStream_t s);

// Skinny GEMM for tiny M (time embedding path): out[m][n] = bias[n] + sum_k act(x[m][k]) W[n][k]
// x, out fp32; W 16-bit [N][K]; act: 0 none, 1 SiLU on the input (reference ResBlock emb_layers:
// nn.SiLU() then Linear, ResBlock.py:283-295); out_act: 1 SiLU on the output (time_embed, unet.py:334-342).
struct SkinnyArgs {
    const float* x; int ldx; const void* W; const float* bias; float* out; int ldo;
    int M, N, K; int in_act; int out_act;
    int accum;                     // 1: out += result (sums the Flux time / guidance / vector embedders)
    // W8 != null (K % 32 == 0): MX fp8 weights (e4m3 bytes [N][K], scales SW as GemmArgs::SW) and the activation MX fake-quantised while it is staged
    // (Flux fp8 mode, round 6: the 77 adaLN modulation projections stream 3.2 GB of weights per forward instead of 6.4)
    const void* W8; const uint32_t* SW; int sw_ld;
};
void launch_skinny(const SkinnyArgs& a, DType dt, hipStream_t s);

// ---------------------------------------------------------------------------------------------
// Flash attention (online softmax): O[b][n][h*D+d] = softmax(q k^T * scale) v
// q rows: Q + (b*Nq + n)*ldq + h*D ;  k/v rows: K + (b*Mk + m)*ldk + h*D  (same for V with ldv)
// D % 8 == 0, D <= 160.  causal: 1 -> key m allowed iff m <= n (CLIP text encoder).
struct AttnArgs {
    const void* Q; int ldq; const void* K; int ldk; const void* V; int ldv;
    void* O; int ldo;
    int B, H, Nq, Mk, D; float scale; int causal;
    // optional additive score bias (T5 relative-position bias): fp32 [H][>= Nq][bias_ld], bias_ld = Mk rounded up to 64,
    // shared by the batch, added to q.k BEFORE the scale (pass bias / scale); padded entries are ignored
    const float* bias; int bias_ld; long bias_hs;
    // O8 != null (only when attn_pick(a).mx_out): the output is written as MX fp8 instead of 16-bit O — bytes
    // O8[b*Nq + n][h*D + d] (row stride ldo8) and, D being 128, one scale dword per (row, head): SO[h][b*Nq + n] (row stride so_ld)
    void* O8; int ldo8; uint32_t* SO; int so_ld;
    // optional workspace of B * H * ceil(Mk / 64) floats (attn_pipe.hip, attn_pipe128.hip): with it the pipelined kernels prove most key blocks safe from the
    // norms of their keys (Cauchy-Schwarz) instead of taking the maximum of every score; null: the exact maximum on every block
    float* knorm_ws;
    // D = 512 (attn512.hip, the VAE's single-head AttnBlock): the keys of a query block are split over `nsplit` workgroups when N / 128 query blocks
    // alone would leave CUs idle; split_ws holds attn512_ws_floats() floats of per-split partial results (un-normalised O, running maximum,
    // denominator) that a merge launch folds.  nsplit <= 1 or split_ws == null: one workgroup per query block, output written directly
    float* split_ws; int nsplit;
};
void launch_attention(const AttnArgs& a, DType dt, hipStream_t s);
// Which kernel launch_attention(a) runs: pure host arithmetic (attn_pick.cpp) over the arguments and the LDX_ATTN* dispatch switches (ldx_switches.h: AttnSwitches).
// launch_attention switches on it, the planner asks it (Engine::op_attn, Engine::n_launches, the single-op C ABI), ldx_op_attn_pick shows it to tests.
enum AttnFamily : int { AF_ATTN = 0, AF_ATTN32, AF_ATTN32AP, AF_ATTN32G, AF_ATTN40P, AF_ATTN128P, AF_ATTN512 };      // attn_kernel (16x16 MFMAs), attn32_kernel, attn32ap_kernel, attn32g_kernel (attention.hip, attn32ap.inc); attn40p_kernel (attn_pipe.hip), attn128p_kernel (attn_pipe128.hip), attn512_kernel (attn512.hip)
struct AttnPick {
    AttnFamily family;
    int targ[3];                   // the template arguments after the type, as instantiated: attn_kernel KS, DT, QT; attn32g_kernel NKS, NDT, ONES; attn32_kernel KVB, VAR; attn32ap_kernel VAR; 0 elsewhere
    bool kpf;                      // attn32g_kernel: with the K fragment prefetch ring (its KPFON argument)
    int qb, block;                 // queries per workgroup, threads per workgroup
    unsigned grid; int lds;        // workgroups, dynamic LDS bytes
    bool knorm;                    // pipelined kernels: a key-norm launch runs first (AttnArgs::knorm_ws given and LDX_ATTN_PIPE_KB != 0)
    float thr;                     // pipelined kernels: rescale threshold override (LDX_ATTN_PIPE_THR), NaN = the type's own
    int nsplit;                    // key splits in effect: 1, or attn512 with AttnArgs::nsplit and its workspace; > 1: a merge launch follows
    int nsplit_want;               // attn512: the splits a caller should ask for, with attn512_ws_floats() floats in AttnArgs::split_ws
    bool mx_out;                   // a caller may set AttnArgs::O8: the generic D = 128 gate holds, so attn128p_kernel or attn32g_kernel<8, 4> takes the launch
    int launches;                  // kernel launches in all (0: empty problem)
};
AttnPick attn_pick(const AttnArgs& a);
bool attn_pipe_ok(const AttnArgs& a);      // the shape rule of the two pipelined kernels, grid-fill gates aside: the planner provides AttnArgs::knorm_ws for these

// The kernels of the other files, launched by launch_attention with the pick that chose them (grid, LDS size; threshold and key-norm launch; key splits).
// attn_pipe.hip: software-pipelined D = 40 kernel (round 4); attn_pipe128.hip: the same pipeline for D = 128 (Flux joint attention), 16-bit or MX fp8 output (AttnArgs::O8);
// attn512.hip: flash attention for D = 512 heads, keys split over AttnPick::nsplit workgroups per query block
void launch_attn_pipe(const AttnArgs& a, const AttnPick& p, DType dt, hipStream_t s);
void launch_attn_pipe128(const AttnArgs& a, const AttnPick& p, DType dt, hipStream_t s);
void launch_attn512(const AttnArgs& a, const AttnPick& p, DType dt, hipStream_t s);
size_t attn512_ws_floats(const AttnArgs& a, int nsplit);
void launch_attn_knorm(const AttnArgs& a, DType dt, hipStream_t s);      // key-block norms for either pipelined kernel (AttnArgs::knorm_ws)
// The base fill of an attention launch, every other byte zero (the padding too), and the scratch of `a` once every other field is final: the key-block norms where
// the pipelined kernels' shape rule holds, the partials of attn512's key splits where attn_pick asks for them (never both: D = 40 / 128 against D = 512); returns the pick
inline AttnArgs attn_args(const void* Q, int ldq, const void* K, int ldk, const void* V, int ldv, void* O, int ldo, int B, int H, int Nq, int Mk, int D, float scale) {
    AttnArgs a; memset(&a, 0, sizeof(a));
    a.Q = Q; a.ldq = ldq; a.K = K; a.ldk = ldk; a.V = V; a.ldv = ldv; a.O = O; a.ldo = ldo; a.B = B; a.H = H; a.Nq = Nq; a.Mk = Mk; a.D = D; a.scale = scale;
    return a;
}
inline AttnPick attn_attach_scratch(AttnArgs& a, const Scratch& s) {
    if (attn_pipe_ok(a)) a.knorm_ws = (float*)s.bytes((size_t)a.B * a.H * ((a.Mk + 63) / 64) * 4);
    const AttnPick p = attn_pick(a);
    if (p.nsplit_want <= 1) return p;
    a.nsplit = p.nsplit_want;
    a.split_ws = (float*)s.bytes(attn512_ws_floats(a, a.nsplit) * 4);
    return attn_pick(a);
}

// Cross-attention sub-block as one kernel (xattn_block.hip): H[m][:] += to_out(softmax(to_q(LayerNorm(H[m][:])) . K_b^T) . V_b) + bo, in place,
// for m in [0, M), image b = m / N.  Wq / Wo: [C][C] 16-bit, row = output feature.  K / V: the projected context, rows b * Mk + key, head h at
// columns h * D.  xattn_block_ok() says whether the kernel takes the shape (C = 320, 8 heads, Mk <= 80, N % 128 == 0; LDX_XATTN_FUSE=0: never).
struct XAttnArgs {
    void* H; int ldh; long M; int N, C, heads;
    const float* ln_g; const float* ln_b; float eps;
    const void* Wq; const void* Wo; const float* bo;
    const void* K; int ldk; const void* V; int ldv; int Mk;
    float scale;
};
// Feed-forward sub-block as one kernel (ff_block.hip): H[m][:] += W2 . GEGLU(W1 . LayerNorm(H[m][:]) + b1) + b2, in place.  W1 [2 * inner][C] in
// the engine's GEGLU row layout (slabs of 32 value rows + their 32 gate rows), erf GELU; W2 [C][inner].  ff_block_ok(): C = 320, inner = 1280.
struct FFBlockArgs {
    void* H; int ldh; long M; int C, inner;
    const float* ln_g; const float* ln_b; float eps;
    const void* W1; const float* b1; const void* W2; const float* b2;
};
bool ff_block_ok(const FFBlockArgs& a);
void launch_ff_block(const FFBlockArgs& a, DType dt, hipStream_t s);
// Row-block GEMM with a normalisation prologue (rowgemm.hip): Y[m][0:N) = pro(X[m][0:K)) . W^T + bias (+ R), K = 320 or 640, N a multiple of K.
// pro 0: identity, 1: LayerNorm(g, b, eps), 2: GroupNorm apply (32 groups; statistics = the producer-written partial sums of the consumer
// GroupNorm's layout, `nchunk` rows per image of HW pixels).  Y may be X's own buffer only for pro = 0 with R = Y (rows are workgroup-private).
struct RowGemmArgs {
    const void* X; int ldx; void* Y; int ldy; long M; int N, K;
    const void* W; const float* bias; const void* R; int ldr;
    int pro; const float* g; const float* b; float eps;
    const float* partial; int nchunk, HW, G;
    // gn_out != null (engine only, pro != 2, N == K): the consumer of Y is a GroupNorm over [M / HW][HW][N] — every workgroup also writes the sum / sum of
    // squares of the 16-bit values it stores, per group, to gn_out[b][chunk = its row block within the image][32][2] (gn_nchunk = HW / rows per block)
    float* gn_out; int gn_nchunk;
    int abl;                       // timing ablations (LDX_RG_ABL, set by the launcher; wrong results): 1 no residual loads, 2 no MFMA loop, 4 no row loads, 8 no stores
    long dup_rows;                 // != 0: row m of Y is also stored at row m + dup_rows (GemmArgs::dup_rows)
};
bool rowgemm_ok(const RowGemmArgs& a);
// Can launch_rowgemm(a) produce the statistics of a consumer GroupNorm(G groups) over [a.M / HW][HW][a.N] (RowGemmArgs::gn_out)?  If yes, the row blocks per image (the
// consumer's chunk count), else 0: LDX_GN_FUSE=0, the GroupNorm prologue (pro = 2), N != K, G != 32, images that are not whole row blocks, more chunks than max_chunks, or a
// GroupNorm the one-launch small kernel takes.  Engine::fuse_gn_stats and ldx_op_rowgemm_gn ask it (xf_pick.cpp); the caller sets gn_out / gn_nchunk / HW.
int rowgemm_gn_chunks(const RowGemmArgs& a, int HW, int G, int max_chunks);
void launch_rowgemm(const RowGemmArgs& a, DType dt, hipStream_t s);
bool xattn_block_ok(const XAttnArgs& a);
void launch_xattn_block(const XAttnArgs& a, DType dt, hipStream_t s);

// The stage choice of one SpatialTransformer: pure host arithmetic over the level's shape, the planner's switches (ldx_switches.h: PlanSwitches) and the kernels' own shape rules (rowgemm_ok,
// xattn_block_ok, ff_block_ok).  Engine::emit_xf emits what it says, Engine::fuse_gn_rowgemm asks xf_proj_in_rowgemm again once the producer's statistics are known,
// ldx_op_xf_pick shows it to tests (xf_pick.cpp).
struct XfShape {
    int C, heads, B, HW, Mc;       // level width, heads, evaluation batch, pixels per image, context tokens
    int Bshare;                    // batch of the shared CFG prefix (0 = none): norm / proj_in and the self-attention half of the FIRST block run on Bshare images
    bool ln_fold;                  // folded LayerNorm copies of the weights were loaded (XfBlockW::ln_fold)
    int gn_chunks;                 // statistics rows per image the producer of the input wrote for norm (0 = none)
};
enum XfStage : int { XS_TILE = 0,          // to_out / proj_out: the tile GEMM
                     XS_ROWBLOCK,          // one row-block launch (rowgemm, prologue 1 in front of a projection, 0 for to_out / proj_out)
                     XS_FOLDED,            // one GEMM on the folded weights (GemmArgs::ln_c1)
                     XS_LN_GEMM,           // affine LayerNorm + GEMM
                     XS_LN_FOLDED };       // affine-free LayerNorm + GEMM on the folded weights (the folded GEMM would be split-K)
struct XfBlockPick {
    XfStage qkv, o1, q2, o2, ff1;  // norm1 + q|k|v, to_out 1, norm2 + q, to_out 2, norm3 + GEGLU projection (q2 / o2 / ff1 unused inside xattn / ffblock)
    bool xattn, ffblock;           // the cross-attention / feed-forward sub-block as one launch (xattn_block / ff_block)
    int ops;                       // ops of the block; Engine::n_launches adds what gemm_pick / attn_pick say an op launches beyond one (split-K reduce, key norms)
};
struct XfPick {
    bool fold;                     // the level runs its LayerNorms folded into the consuming GEMMs
    bool proj_in_rowgemm;          // norm + proj_in as one rowgemm launch (GroupNorm prologue) instead of GroupNorm + GEMM
    XfStage proj_out;
    XfBlockPick first, rest;       // the first block and every later one (they differ under a shared prefix)
    int ops_outer;                 // ops of norm + proj_in and proj_out; the transformer has ops_outer + first.ops + (depth - 1) * rest.ops
};
XfPick xf_pick(const XfShape& s);
static inline int rowblock_rows(int K) { return 128 * 320 / K; }      // rows of one row block at width K = 320 / 640
long rowblock_count(long M, int K);                          // workgroups of a row-block launch over M rows at width K (128 rows x 320 columns each)
bool rowblock_fills_chip(long workgroups, bool prefix);      // the planner's chip-fill rule for them; prefix: the launch belongs to a shared CFG prefix
bool xf_proj_in_rowgemm(int C, long M, int HW, bool prefix, int gn_chunks);      // XfPick::proj_in_rowgemm for M rows

// ---------------------------------------------------------------------------------------------
// GroupNorm(32 groups) over NHWC + optional SiLU.  Two launches: partial statistics, then apply.
struct GroupNormArgs {
    const void* X; int ldx; void* Y; int ldy;
    int B, HW, C, G; float eps; int silu;
    const float* gamma; const float* beta;
    float* partial;                // workspace [B][GN_NCHUNK][G][2]
    int nchunk;                    // pixel chunks actually used (<= GN_NCHUNK), set by the launcher
    int stats_chunks;              // > 0: the producer's epilogue already wrote `stats_chunks` partial rows per batch (GemmArgs::gn_partial): no statistics
                                   // pass; more than GN_NCHUNK rows are first folded (fixed order) into partial[B][GN_FOLD][G][2] behind them
};
constexpr int GN_NCHUNK = 256;
constexpr int GN_FOLD = 64;         // fold target: partial rows per batch after folding a long producer list
constexpr int GN_MAX_PRODUCER_CHUNKS = 32768;      // most partial rows per batch a producer may write (VAE 2048^2: 4 Mi pixels in 128-row tiles)
// floats of GroupNorm workspace for B images whose largest GroupNorm'ed map has HWmax pixels: producer rows (>= GN_NCHUNK) + the fold target
static inline size_t gn_workspace_rows(long HWmax) { long r = HWmax / 64; if (r < GN_NCHUNK) r = GN_NCHUNK; if (r > GN_MAX_PRODUCER_CHUNKS) r = GN_MAX_PRODUCER_CHUNKS; return (size_t)r; }
void launch_groupnorm(const GroupNormArgs& a, DType dt, hipStream_t s);
// the dispatch rule of launch_groupnorm for its one-launch kernel (statistics + apply in one workgroup per (image, group)); the planner asks it too:
// such a GroupNorm does not take producer-written statistics (LDX_GN_SMALL_MAX overrides the element bound)
bool gn_uses_small_kernel(int B, long HW, int C, int G);
// What launch_groupnorm(a) launches: pure host arithmetic.  The launcher switches on it, Engine::n_launches and the profile labels ask it.
enum GnKind : int { GN_SMALL = 0, GN_STATS_APPLY, GN_APPLY, GN_FOLD_APPLY };      // gn_small_kernel / gn_stats_kernel + gn_apply_kernel / gn_apply_kernel on the producer's statistics / gn_fold_kernel first
struct GnPick {
    GnKind kind;
    int CH, TX, RY;                // gn_stats_kernel / gn_apply_kernel: chunks per thread (the template argument), threads per pixel, pixel rows per workgroup
    int nchunk;                    // statistics rows per image that gn_apply_kernel reads (GroupNormArgs::nchunk)
    unsigned grid1[2], grid2[2];   // workgroups (x, y) of the first launch (small, statistics or fold; 0 = none) and of gn_apply_kernel (0 = none)
    int lds;                       // dynamic LDS bytes of gn_stats_kernel
    int launches;
};
GnPick gn_pick(const GroupNormArgs& a);

// LayerNorm over the last dim C of [rows][ldx] -> [rows][ldy]
// gamma/beta may be null (elementwise_affine=False); optional adaLN modulation (Flux):
// y = (1 + scale[b][c]) * y + shift[b][c] with b = row / rows_per_batch.  C <= 3072.
struct LayerNormArgs {
    const void* X; int ldx; void* Y; int ldy; int rows, C; float eps;
    const float* gamma; const float* beta;
    const float* scale; const float* shift; int mod_ld; int rows_per_batch;
    int rms;                       // 1: T5LayerNorm (no mean subtraction, no beta): x * rsqrt(mean(x^2) + eps) * gamma
    // Y8 != null (C % 32 == 0): the output is written as MX fp8 instead of 16-bit Y: bytes Y8[row][c] (row stride ldy8) and
    // scales S8 in the GemmArgs::SA layout (row stride s8_ld), exactly what launch_mx_quant would produce from Y
    void* Y8; int ldy8; uint32_t* S8; int s8_ld;
};
void launch_layernorm(const LayerNormArgs& a, DType dt, hipStream_t s);

// ---------------------------------------------------------------------------------------------
// Edge / scheduler kernels (fp32 NCHW at the boundary, reference ModelBase.py:72-133).
// prep: xc = x / sqrt(sigma^2 + 1) -> NHWC 16-bit with Cpad channels (zeros above C);
//       t = argmin_k |ln sigma - log_sigmas[k]| ; temb_out[b][:] = temb_table[t][:]
struct PrepArgs {
    const float* x; const float* sigma; int B, C, H, W; int Cpad; void* xc;     // xc [B][H*W][Cpad]
    const float* log_sigmas; int n_sigmas; const float* temb_table; int temb_dim;
    float* temb_out; float* t_out;   // [B][temb_dim], [B]
    int scale_input;                 // 1: divide by sqrt(sigma^2+1) ; 0: raw (ldx_unet_forward)
    const float* t_in;               // if non-null: timestep indices given directly (no sigma lookup)
    int xB;                          // batch of x (0 = B): sample b reads x[b % xB] — the [uncond; cond] halves of a CFG evaluation share one latent
    // c_concat (ModelBase.py:100-101: xc = cat((x / sqrt(sigma^2 + 1), c_concat), 1); inpainting UNets, in_channels = 9): x carries Cx channels,
    // channels Cx .. C - 1 come UNSCALED from cc [B][C - Cx][H][W].  cc == null: x carries all C channels (Cx is ignored)
    const float* cc; int Cx;
    // emb_table != null: out_emb[b][0:emb_n) = emb_table[t][0:emb_n) — the row of the per-timestep table of every ResBlock's emb_layers output
    // (Engine::build_emb_table): the time-embedding MLP is a pure function of the integer timestep, so it is evaluated once per timestep at load
    const float* emb_table; int emb_n; float* emb_out;
};
void launch_prep(const PrepArgs& a, DType dt, hipStream_t s);
// out[i] = nearest log-sigma table index of sigma[i] (the prep kernel's own lookup; ldx_unet_timestep)
void launch_timestep(const float* sigma, const float* log_sigmas, int n_sigmas, int n, int* out, hipStream_t s);
// finish: out_nchw[b][c][p] = x_nchw[b][c][p] - eps_nhwc[b][p][c] * sigma[b]   (or raw eps if x == null)
struct FinishArgs { const float* eps; int ld; const float* x; const float* sigma; float* out; int B, C, HW; int xB; };       // xB as in PrepArgs
void launch_fill_f32(float* dst, float v, int n, hipStream_t s);
void launch_fill2_f32(float* a, float va, float* b, float vb, int n, hipStream_t s);      // a[i] = va, b[i] = vb (the sigma and timestep-index slots of a CFG evaluation: one launch)
// dst[r][0:C) = src[r][0:C) for r in [0, rows): 16-bit elements, both with row stride ld, C % 8 == 0 (the shared CFG prefix's hand-over, Engine::op_dup)
struct DupRowsArgs { const void* src; void* dst; int rows, C, ld; };
void launch_dup_rows(const DupRowsArgs& a, DType dt, hipStream_t s);
// CLIP pooled output: row of last[b] at the first position whose id == eos_id (position 0 if none: torch argmax of an all-zero row),
// then, if proj != null, out[b] = row @ proj^T (proj [E][E] fp32, row-major [out][in])
void launch_clip_pooled(const float* last, const int* ids, int B, int T, int E, int eos_id, const float* proj, float* out, hipStream_t s);
void launch_finish(const FinishArgs& a, hipStream_t s);

// 16-bit <-> fp32 conversion helpers for tests / host plumbing
void launch_f32_to_t(const float* in, void* out, size_t n, DType dt, hipStream_t s);
void launch_t_to_f32(const void* in, float* out, size_t n, DType dt, hipStream_t s);
// the same as ops of a plan (fp32 context -> 16 bit, 16-bit result -> fp32 output), and the device-to-device copy of a finished fp32 result (ESRGAN)
struct CvtArgs { const float* in; void* out; size_t n; };
struct CvtOutArgs { const void* in; float* out; size_t n; };
struct CopyOutArgs { const void* src; void* dst; size_t bytes; };
inline void launch_f32_to_t(const CvtArgs& a, DType dt, hipStream_t s) { launch_f32_to_t(a.in, a.out, a.n, dt, s); }
inline void launch_t_to_f32(const CvtOutArgs& a, DType dt, hipStream_t s) { launch_t_to_f32(a.in, a.out, a.n, dt, s); }
inline hipError_t launch_copy_out(const CopyOutArgs& a, hipStream_t s) { return hipMemcpyAsync(a.dst, a.src, a.bytes, hipMemcpyDeviceToDevice, s); }
// NCHW fp32 <-> NHWC 16-bit (VAE boundary)
void launch_nchw_to_nhwc(const float* in, void* out, int B, int C, int HW, int Cpad, float scale, DType dt, hipStream_t s);

// VAE boundary (AutoEncoders/VariationalAE.py:130-145, 690-722): z fp32 NCHW [B][C][HW] -> optional 1x1 mix
// (post_quant_conv, fp32: out[c] = b[c] + sum_k w[c][k] z[k]) -> NHWC 16-bit with Cpad channels.
struct VaePrepArgs { const float* z; void* out; int B, C, HW, Cpad; const float* mix_w; const float* mix_b; };
void launch_vae_prep(const VaePrepArgs& a, DType dt, hipStream_t s);
// encoder input: pixels NHWC fp32 [B][HW][C] in [0,1] -> x*2-1 (process_input, VariationalAE.py:593) -> NHWC 16-bit, Cpad channels
struct PixelsPrepArgs { const float* px; void* out; int B, C, HW, Cpad; float scale, shift; };
void launch_pixels_prep(const PixelsPrepArgs& a, DType dt, hipStream_t s);
// pixel post-process: out = clamp((x + 1) / 2, 0, 1) on fp32 (process_output, VariationalAE.py:595-597)
struct ClampArgs { const float* in; float* out; size_t n; };
void launch_clamp01(const ClampArgs& a, hipStream_t s);
// row softmax in place on a 16-bit [rows][ld] matrix: p = softmax(x * scale) (VAE AttnBlock, D = 512 single head)
struct SoftmaxArgs { void* X; int rows, cols, ld; float scale; };
void launch_softmax_rows(const SoftmaxArgs& a, DType dt, hipStream_t s);
// CLIP embeddings (clip/Clip.py:254-294): x[b][t][:] = tok[id[b][t]][:] + pos[t][:]  (fp32 tables -> 16-bit)
// ids in [vocab, vocab + n_extra) read row id - vocab of `extra` (textual-inversion vectors, SD15/SDClip.py:213-267)
// pos == null: token rows alone (T5)
struct ClipEmbedArgs { const int* ids; const float* tok; const float* pos; void* out; int B, T, C, vocab; const float* extra; int n_extra; };
void launch_clip_embed(const ClipEmbedArgs& a, DType dt, hipStream_t s);

// First-block cache helpers on the joint token buffer X [B][L][C] (16-bit; rows [0, Lt) text, [Lt, L) image per batch).
// fb_diff: sums[0] = sum |(X - S0) - F| , sums[1] = sum |F| over the image rows (deterministic two-stage reduction through
// `partial`, >= 2 * 1024 floats).  fb_first: F = X - S0 (image rows, fp32).  fb_residual: R = X - S1 (all rows, fp32).
// fb_apply: X += R.
void launch_fb_diff(const void* X, const void* S0, const float* F, int B, int L, int Lt, int C, float* partial, float* sums, DType dt, hipStream_t s);
void launch_fb_first(const void* X, const void* S0, float* F, int B, int L, int Lt, int C, DType dt, hipStream_t s);
void launch_fb_residual(const void* X, const void* S1, float* R, size_t n, DType dt, hipStream_t s);
void launch_fb_apply(void* X, const float* R, size_t n, DType dt, hipStream_t s);

// tiled_scale blending (Utilities/util.py:406-600): out[y0+y][x0+x][c] += tile[y][x][c] * mask(y, x), div += mask, where mask
// ramps (t + 1) / feather over the first / last `feather` rows and columns of the tile (all four edges, skipped per axis if
// feather >= tile extent); finish: out = clamp(out / div, 0, 1) (USDU_upscaler.py:94).  NHWC fp32, C channels.
void launch_tile_blend(const float* tile, int th, int tw, float* out, float* div, int H, int W, int C, int y0, int x0, int feather, hipStream_t s);
void launch_tile_finish(float* out, const float* div, size_t n, int clamp01, hipStream_t s);

// Flux: per-head RMSNorm of q and k (QKNorm, BlackForest/Flux.py:148-200, eps 1e-6) followed by RoPE
// (apply_rope :73-82) in place on a fused [rows][ld] q|k|v buffer (q at column 0, k at column C = H*D).
// cos/sin: [L][D/2] fp32 tables built by the host exactly as rope() does (:36-70); token = row % L.
struct QkRopeArgs {
    void* QKV; int ld; int rows; int L; int H, D; const float* qscale; const float* kscale;
    const float* cosT; const float* sinT; float eps;
    // launch_qk_norm_rope_mx only (D = 128): the normalised + rotated q / k leave as MX fp8 in ldx_op_mx_quant's format instead of being written back in 16 bit:
    // Q8 / K8 [row8 + row][ld8] bytes (head h at columns h * 128), SQ / SK dwords [H][s8_ld] (byte j of dword [h][row8 + row] = the scale of d block j)
    void* Q8; void* K8; int ld8; uint32_t* SQ; uint32_t* SK; int s8_ld; long row8;
};
void launch_qk_norm_rope(const QkRopeArgs& a, DType dt, hipStream_t s);
void launch_qk_norm_rope_mx(const QkRopeArgs& a, DType dt, hipStream_t s);
// MX fp8 attention for D = 128 (attn_mx.hip).  Q8 / K8 + SQ / SK: the format above, rows b * Nq + q / b * Mk + key.  V8T [B][H][128][Lp] + SV [B][H][Lp / 128][128]:
// launch_mx_vt_quant's output (V transposed, keys in the MFMA's order inside every 64-key step, one scale per (d, 32 consecutive keys)); Lp = Mk rounded up to 128.
// Output: 16-bit O [rows][ldo] (head h at columns h * 128), or MX fp8 O8 / SO exactly as AttnArgs::O8 / SO.
struct AttnMxArgs {
    const void* Q8; int ldq8; const uint32_t* SQ; int sq_ld;
    const void* K8; int ldk8; const uint32_t* SK; int sk_ld;
    const void* V8T; const uint32_t* SV; int Lp;
    void* O; int ldo;
    void* O8; int ldo8; uint32_t* SO; int so_ld;
    int B, H, Nq, Mk; float scale;
};
bool attn_mx_ok(const AttnMxArgs& a);
void launch_attn_mx(const AttnMxArgs& a, DType dt, hipStream_t s);
// V (16 bit, rows b * L + token, head h at columns h * 128 of a row of ldv elements) -> V8T / SV (see AttnMxArgs)
struct MxVtArgs { const void* V; int ldv; int B, H, L; void* V8T; uint32_t* SV; int Lp; };
void launch_mx_vt_quant(const MxVtArgs& a, DType dt, hipStream_t s);
// timestep_embedding_flux (sample/sampling_util.py:78-104): out[b][:] = [cos(1000 t f_j) | sin(1000 t f_j)], dim 256
struct FluxTembArgs { const float* t; float* out; int B, dim; float factor; };
void launch_flux_temb(const FluxTembArgs& a, hipStream_t s);
struct SiluArgs { const float* in; float* out; size_t n; };
void launch_silu_f32(const SiluArgs& a, hipStream_t s);
// patchify  x[B][C][H][W] fp32 -> tokens [B*(H/2)*(W/2)][4C] 16-bit, column = c*4 + ph*2 + pw   (Flux3.forward :742-748)
struct FluxPatchArgs { const float* x; void* out; int B, C, H, W; };
void launch_flux_patchify(const FluxPatchArgs& a, DType dt, hipStream_t s);
// unpatchify + CONST.calculate_denoised (sampling.py:108-122): out = x - tok*sigma (or tok if x == null), fp32 NCHW
struct FluxUnpatchArgs { const float* tok; int ld; const float* x; const float* sigma; float* out; int B, C, H, W; };
void launch_flux_unpatchify(const FluxUnpatchArgs& a, hipStream_t s);

// Sampler elementwise kernels (fp32, reference samplers.py / CFG.py):
//  d = lerp(den_uncond, den_cond, cfg)                             (torch.lerp, CFG.py:60)
//  kind 0 euler: x = x + ((x - d) / c0) * c1   c0 = sigma_hat, c1 = sigma_next - sigma_hat (samplers.py:308, util.py:26-37)
//  kind 1 dpmpp: x = c0 * x - c1 * d           c0 = sigma_next/sigma, c1 = expm1(-h)       (samplers.py:945-946)
//  kind 2      : denoised_out = d only (multiscale steps combine at low resolution first)
//  kind 3      : x = x + den_uncond * c0   (ancestral noise injection: x + noise * s_noise * sigma_up, samplers.py:728-729)
// den_*: the two [B] chunks [uncond; cond] returned by the wrapper (cond.py:194-195 order).
struct StepArgs {
    float* x; const float* den_uncond; const float* den_cond; float* denoised_out;  // denoised_out optional
    size_t n; float cfg; int kind;
    float c0, c1;
};
void launch_sampler_step(const StepArgs& a, hipStream_t s);
// one pass of bislerp (Utilities/upscale.py:5-128): per-pixel spherical interpolation of the C-vector between source
// positions c1[i], c2[i] with ratio r[i] along the last (axis = 1) or second-to-last (axis = 0) spatial axis.
void launch_bislerp_pass(const float* in, float* out, int N, int C, int H, int W, int axis, int new_len,
                         const int* c1, const int* c2, const float* r, hipStream_t s);
// VAE encoder tail: moments_nchw[b][c][p] = bias[c] + sum_k w[c][k] * in_nhwc[b][p][k]   (quant_conv 1x1, fp32)
struct MixArgs { const float* in; int ld; float* out; int B, C, HW; const float* w; const float* bias; };
void launch_mix_nhwc_to_nchw(const MixArgs& a, hipStream_t s);
// bilinear resize (align_corners=False, antialias=False) of fp32 NCHW planes
void launch_bilinear(const float* in, float* out, int planes, int Hin, int Win, int Hout, int Wout, hipStream_t s);

// ---------------------------------------------------------------------------------------------
// Weight packing (Engine::pack16 / pack32 / mk_ln_folded): the three argument structs describe one piece each, and weight_layout.h interprets them, for
// pack.hip's kernels (state-dict tensors that already live on the GPU, ldx_load_tensor_device) and for the host packers alike, so the two agree bit for
// bit.  sdt / *_dt are LDX_F32 | LDX_F16 | LDX_BF16 codes of the SOURCE tensors; out_dt is the engine's.  The pointers are device pointers for the
// launchers below, host pointers in the host loops.
// One piece of a packed 16-bit matrix: out[r][col0 + c] = scale * src(r, c), r in [0, N), c in [0, K), out row stride ldo (elements).
//   CinPad == 0: src(r, c) = src[srow(r) * K + c], srow = the GEGLU slab permutation when geglu_inner > 0 (geglu_src_row), else r
//   CinPad  > 0: 3x3 conv [N][Cin][3][3] -> [N][ky][kx][CinPad] (K = 9 * CinPad): src(r, tap * CinPad + ci) = ci < Cin ? src[(r * Cin + ci) * 9 + tap] : 0
// For a launch K, ldo, col0 and CinPad are multiples of 8 and `out` is 16-byte aligned: every store is 16 bytes (the host loop takes any shape).
struct PackArgs {
    const void* src; int sdt;
    void* out; long ldo; long col0; DType out_dt;
    int N, K;
    int Cin, CinPad;
    int geglu_inner;
    float scale;
};
void launch_pack16(const PackArgs& a, hipStream_t s);
// fp32 vector: out[i] = a[srow(i)] (+ b[srow(i)] when b != null), i in [0, n)
struct PackVecArgs { const void* a; int a_dt; const void* b; int b_dt; float* out; int n; int geglu_inner; };
void launch_pack32(const PackVecArgs& a, hipStream_t s);
// Rows [0, N) of a LayerNorm-folded projection (Engine::mk_ln_folded): w = scale * src[srow(r)][k];
//   out[r][k] = 16-bit(w * gamma[k]);  c1[r] = (float) sum_k (double) out[r][k];  c2[r] = (float)(sum_k (double) w * beta[k] + bias[srow(r)])   (bias == null: 0)
// both sums in fp64, ascending k.  For a launch K is a multiple of 8.
struct LnFoldArgs {
    const void* src; int sdt; const void* gamma; int g_dt; const void* beta; int b_dt; const void* bias; int bias_dt;
    void* out; DType out_dt; float* c1; float* c2;
    int N, K; int geglu_inner; float scale;
};
void launch_ln_fold(const LnFoldArgs& a, hipStream_t s);
// GGML Q8_0 blocks (34 bytes: fp16 scale, 32 int8; 2-byte aligned) -> out[n] (q8.hip, libldx_q8.so): the fp16 value fp16_rne(float(d) * q) as
// out_dt = LDX_F16, or that value as LDX_BF16 / LDX_F32.  n % 32 == 0, out 16-byte aligned.
struct DequantQ8Args { const void* blocks; void* out; size_t n; int out_dt; };
void launch_dequant_q8_0(const DequantQ8Args& a, hipStream_t s);

// ---------------------------------------------------------------------------------------------
// 8-bit image ops of the img2img path (image.hip, libldx_image.so): HWC uint8 device images with a row pitch in bytes; include/ldx.h states each rule.
// The launchers take validated arguments (capi.cpp): rectangles inside the image, pitch >= W * C, box radius <= image_box_max_radius().
void launch_image_quantize(const float* in, uint8_t* out, int H, int W, int C, long out_pitch, hipStream_t s);
void launch_image_to_float(const uint8_t* in, long in_pitch, float* out, int H, int W, int C, hipStream_t s);
void launch_image_resample_pass(const uint8_t* in, long in_pitch, uint8_t* out, long out_pitch, int H, int W, int C, int axis, int new_len,
                                const int* bounds, const int* kk, int ksize, hipStream_t s);
int image_box_max_radius();
void launch_image_box_blur_pass(const uint8_t* in, long in_pitch, uint8_t* out, long out_pitch, int H, int W, int axis, float radius, hipStream_t s);
void launch_image_composite(uint8_t* canvas, long canvas_pitch, const uint8_t* tile, long tile_pitch, const uint8_t* mask, long mask_pitch,
                            int h, int w, int C, hipStream_t s);
void launch_image_fill(uint8_t* img, long pitch, int h, int rowlen, int value, hipStream_t s);

// ---------------------------------------------------------------------------------------------
// TAESD decoder (taesd.hip, libldx_taesd.so): the latent preview of the sampler loops (src/AutoEncoders/taesd.py:105-135).
// 3x3 / stride 1 / pad 1 conv, 64 -> 64 channels, on 16-bit rows [B * H * W][64] with the whole weight matrix resident in LDS:
//   Y[m][n] = relu?( sum_k W[n][k] X(m, k) + bias[n] + R[m][n] ),  k = (ky * 3 + kx) * 64 + ci,  W [64][576] 16-bit (conv_piece layout, CinPad 64).
// up = 1: the 3x3 window walks the nearest x2 upsampled image (output [B][2 Hin][2 Win]), X stays [B][Hin][Win].  bias, R may be null.
// Rf != null: the residual row is fp32 [M][64] instead of R; Yf != null: the value is ALSO stored unrounded as fp32 [M][64].  The decoder's skip stream runs
// through ten Blocks: kept in fp32 beside the 16-bit copy the next conv multiplies, it is not rounded once per Block (engine_taesd.cpp).
// out3 = 1: the 64 -> 3 output conv (W [32][576], rows 3 .. 31 zero; bias [3]); instead of Y it writes, each if non-null,
//   out_f32 [B][3][H][W] = (y - 0.5) * 2  (TAESD.decode, taesd.py:224-237) and
//   out_u8  [B][H][W][3] = trunc(clip(((d + 1) / 2) * 255, 0, 255))  (taesd_preview :291-304; flux: channel c from d[2 - c] clamped to [-1, 1]).
struct TaesdConvArgs {
    const void* X; const void* W; const float* bias; const void* R; void* Y;
    const float* Rf; float* Yf;
    float* out_f32; uint8_t* out_u8;
    int B, Hin, Win; int up, relu, out3, flux;
};
bool taesd_conv_ok(const TaesdConvArgs& a);                 // pointers there, up 0 | 1, fewer than 2^31 output pixels
void launch_taesd_conv(const TaesdConvArgs& a, DType dt, hipStream_t s);
// Clamp (tanh(z / 3) * 3, taesd.py:30-42) of the latent fp32 NCHW [B][C][HW], C <= 8 -> 16-bit rows [B * HW][64], the other channels zero
struct TaesdPrepArgs { const float* z; void* out; int B, C; long HW; };
void launch_taesd_prep(const TaesdPrepArgs& a, DType dt, hipStream_t s);

// ---------------------------------------------------------------------------------------------
// AutoHDR (hdr.hip, libldx_hdr.so): the reference's default post-effect (src/AutoHDR/ahdr.py:83-127) on B HWC images; include/ldx.h states each rule.
// Exactly one of in_f32 (dense [B][H][W][3]) and in_u8 (rows of in_pitch bytes, images H * in_pitch apart) is set; out_u8 (out_pitch likewise) and
// out_f32 (dense) each if non-null.  fwd, inv: the two lcms tables, uint16 [33][33][33][4], 8-byte aligned; lut: the 256 luminance bytes.
// The launchers take validated arguments (capi.cpp): pitches >= W * 3, H * W <= hdr_max_pixels(), workspace of hdr_workspace_bytes(B, H, W) bytes, 4-aligned.
struct HdrArgs {
    const float* in_f32; const uint8_t* in_u8; long in_pitch;
    int B, H, W;
    const uint16_t* fwd; const uint16_t* inv; const uint8_t* lut;
    float f_contrast, f_color;
    void* workspace;
    uint8_t* out_u8; long out_pitch; float* out_f32;
};
constexpr long hdr_max_pixels() { return 0xFFFFFFFFL / 255; }      // the sum of an image's grey bytes is a uint32
long hdr_workspace_bytes(int B, int H, int W);
void launch_hdr_apply(const HdrArgs& a, hipStream_t s);
// one table read of an HWC byte image: out = tetrahedral read of `table` at in
void launch_hdr_table(const uint8_t* in, long in_pitch, uint8_t* out, long out_pitch, int H, int W, const uint16_t* table, hipStream_t s);

// ---------------------------------------------------------------------------------------------
// SaveImage (png.hip, libldx_png.so): the PNG file of B HWC images, C = 3, made on the device; include/ldx.h states each rule of the format.
// Exactly one of in_f32 (dense [B][H][W][3]) and in_u8 (rows of in_pitch bytes, images H * in_pitch apart) is set.  The launchers take validated
// arguments (capi.cpp): the filtered stream of one image, png_stream_bytes(H, W) = H * (1 + 3 W), is at most png_max_stream_bytes(); B <= 65535;
// workspace of png_workspace_bytes(B, H, W) (zlib_workspace_bytes(n)) bytes, 16-aligned; out_stride >= png_bound_bytes(H, W).
struct PngArgs {
    const float* in_f32; const uint8_t* in_u8; long in_pitch;
    int B, H, W;
    void* workspace;
    uint8_t* out; long out_stride; uint32_t* out_len;
};
constexpr long png_max_stream_bytes() { return 1L << 30; }         // chunk offsets and the file length are 32-bit
long png_stream_bytes(int H, int W);
long png_workspace_bytes(int B, int H, int W);
long png_bound_bytes(int H, int W);
long zlib_workspace_bytes(long n);
long zlib_bound_bytes(long n);
// stream [B][H][1 + 3 W]: every row's filter type and filtered bytes; types [B][H] if non-null
void launch_png_filter(const float* in_f32, const uint8_t* in_u8, long in_pitch, int B, int H, int W, uint8_t* stream, uint8_t* types, hipStream_t s);
void launch_png_encode(const PngArgs& a, hipStream_t s);
// the zlib stream of n device bytes -> out, its length -> out_len[0]
void launch_zlib_deflate(const uint8_t* bytes, long n, void* workspace, uint8_t* out, uint32_t* out_len, hipStream_t s);

// ---------------------------------------------------------------------------------------------
// fp32 canvas ops of the ADetailer path (detail.hip, libldx_detail.so): a dense fp32 [H][W][3] device canvas; include/ldx.h states each rule.
// The launchers take validated arguments (capi.cpp): rectangles inside the canvas, k odd, k / 2 < h and w, in != out.
constexpr int detail_max_kernel() { return 63; }
void launch_detail_crop_quantize(const float* canvas, int W, int x0, int y0, int w, int h, uint8_t* out, long out_pitch, hipStream_t s);
void launch_detail_blur_mask(const float* in, int h, int w, const float* table, int k, float* out, hipStream_t s);
// the rectangle (x0, y0, w, h) of the canvas from the first h rows and w columns of src [..][src_w][3] and mask [..][src_w]
void launch_detail_paste(float* canvas, int W, int x0, int y0, const float* src, const float* mask, int src_w, int h, int w, hipStream_t s);

// ---------------------------------------------------------------------------------------------
// SAM image encoder (sam.hip, libldx_sam.so): what ImageEncoderViT needs beyond the shared GEMM / LayerNorm / conv kernels; include/ldx.h states each rule.
// Head dimension 64, patch 16.  Tokens are 16-bit rows [B * S * S][E]; a window block's rows are [B * nw * nw][win * win][E], nw = ceil(S / win).
// The launchers take validated arguments (the *_ok functions; capi.cpp and SamEngine::plan ask them).
// Patch gather: img fp32 [B][3][16 S][16 S] -> out 16-bit [B * S * S][768], column = (c * 16 + ky) * 16 + kx (patch_embed.proj.weight's own K order)
struct SamPatchArgs { const float* img; void* out; int B, S; };
void launch_sam_patch(const SamPatchArgs& a, DType dt, hipStream_t s);
// scatter = 0: dst[window row] = src[pixel row], zero rows for the padding below and right of the S x S grid.
// scatter = 1: dst[pixel row] = R[pixel row] + src[window row] (the crop; the sum in fp32; R may be dst, or null for the bare inverse)
struct SamWindowArgs { const void* src; void* dst; const void* R; int B, S, win, C; int scatter; };
bool sam_window_ok(const SamWindowArgs& a);
void launch_sam_window(const SamWindowArgs& a, DType dt, hipStream_t s);
// out fp32 [BW * H][n * n][2 n] = rel_h | rel_w of every query: rel_h[q][j] = sum_c Q[q][c] * th[q_h - j + n - 1][c], rel_w[q][j] likewise with q_w and tw.
// Q 16-bit rows bw * n * n + q (row stride ldq), head h at columns h * 64; th, tw fp32 [2 n - 1][64].
struct SamRelposArgs { const void* Q; int ldq; const float* th; const float* tw; float* out; int BW, H, n; };
bool sam_relpos_ok(const SamRelposArgs& a);
void launch_sam_relpos(const SamRelposArgs& a, DType dt, hipStream_t s);
// O[bw * N + q][h * 64 + d] = sum_k softmax_k(scale * q.k + rel[q][k / n] + rel[q][n + k % n]) v[k][d], N = n * n keys and queries per (bw, h); Q, K, V
// rows bw * N + token with one row stride ld, head h at columns h * 64; rel = SamRelposArgs::out.  Flash attention: no N x N matrix is ever stored.
struct SamAttnArgs { const void* Q; const void* K; const void* V; int ld; const float* rel; void* O; int ldo; int BW, H, n; float scale; };
bool sam_attn_ok(const SamAttnArgs& a);
void launch_sam_attention(const SamAttnArgs& a, DType dt, hipStream_t s);
// X[m][c] = act(X[m][c] + vec[m % period][c]) in place: act 1 with period 1 = bias + erf-GELU (the MLP), act 0 with period S * S = + pos_embed.  C % 8 == 0.
struct SamRowvecArgs { void* X; int ld; long rows; int C; const float* vec; int period; int act; };
void launch_sam_rowvec(const SamRowvecArgs& a, DType dt, hipStream_t s);
// out fp32 [B][C][HW] = X 16-bit [B * HW][ld]
struct SamOutArgs { const void* X; int ld; float* out; int B, C, HW; };
void launch_sam_out(const SamOutArgs& a, DType dt, hipStream_t s);
// Sam.preprocess: out fp32 [3][size][size] = (float(in[y][x][c]) - mean_c) / std_c, zeros right of w and below h; in u8 [h][w][3], rows `pitch` bytes apart
struct SamPreprocessArgs { const uint8_t* in; long pitch; int h, w; float* out; int size; };
void launch_sam_preprocess(const SamPreprocessArgs& a, hipStream_t s);

// ---------------------------------------------------------------------------------------------
// SAM prompt encoder + mask decoder (samdec.hip, libldx_samdec.so): fp32 throughout.  Tokens are rows [P * T][C], image rows [P * g * g][C].
// The launchers take validated arguments (the *_ok functions; SamDecoderEngine asks them when it plans).
// out [P][5 + ns][C]: iou_token | mask_tokens[4] | n points (labels 1 / 0 / -1) | the padding point (no box) or the two box corners; ns = n + (boxes ? 2 : 1).
// points [P][n][2] and boxes [P][4] (x, y in the resized frame), labels int32 [P][n]; gauss [2][C / 2]; point_emb [4][C]; size = image_size
struct SamDecPromptArgs { const float* points; const int* labels; const float* boxes; int P, n, ns, C; float size; const float* gauss; const float* point_emb; const float* not_a_point;
                          const float* iou_token; const float* mask_tokens; float* out; };
void launch_samdec_prompt(const SamDecPromptArgs& a, hipStream_t s);
// out [M][C] = emb [C][M] + add [C]
void launch_samdec_transpose(const float* emb, const float* add, float* out, int C, int M, hipStream_t s);
// Y[z][m][n] = act(LN(X[z][m % x_period] (+ PE[m % pe_period], for the column blocks that start below pe_cols) . W[z][n] + bias[z][n] + R[m % r_period][n])).
// W [N][K]; nb <= 256 columns per workgroup; ln_group > 0: LayerNorm over every group of ln_group consecutive columns with gamma / beta [ln_group] (N <= nb);
// act 1 ReLU, 2 erf-GELU; a period of 0: the row itself.  K, ldx, ldpe and the z strides of X and W are multiples of 4 and X, PE, W 16-byte aligned (float4 loads).  hyper [P][4][N / 4] != null: rows are [P][g * g][2 x 2] and the N columns [2 x 2][N / 4]; instead of Y,
// logits [P][4][4 g][4 g] = the four products of every column group with the prompt's hypernetwork vectors (MaskDecoder's `hyper_in @ upscaled_embedding`)
struct SamDecGemmArgs {
    const float* X; int ldx; long x_period; const float* PE; int ldpe; long pe_period; int pe_cols;
    const float* W; const float* bias; const float* R; int ldr; long r_period;
    const float* gamma; const float* beta; int ln_group; float eps; int act;
    float* Y; int ldy; long M; int N, K, nb; int nz; long xz, wz, bz, yz;
    const float* hyper; int g; float* logits;
};
bool samdec_gemm_ok(const SamDecGemmArgs& a);
void launch_samdec_gemm(const SamDecGemmArgs& a, hipStream_t s);
// O[b * Tq + q][h * hd + d] = softmax_t(scale * Q[q] . K[b * Tk + t]) V[b * Tk + t][d] over Tk <= 16 keys; q_shared: Q has Tq rows, the same for every b
struct SamDecAttnSmallArgs { const float* Q; int ldq; int q_shared; const float* K; int ldk; const float* V; int ldv; float* O; int ldo; int B; long Tq; int Tk, H, hd; float scale; };
bool samdec_attn_small_ok(const SamDecAttnSmallArgs& a);
void launch_samdec_attn_small(const SamDecAttnSmallArgs& a, hipStream_t s);
// The T <= 16 token queries of every (prompt, head) against M image keys in S ranges of `chunk` keys (samdec_t2i_ranges; two launches: partials, merge).
// kv_shared: K, V have M rows, the same for every prompt.  part: B * H * S * 16 * (hd + 2) floats.  hd 8, 16 or 32.
struct SamDecAttnT2IArgs { const float* Q; int ldq; const float* K; int ldk; const float* V; int ldv; int kv_shared; float* part; float* O; int ldo; int B, T, M, H, hd, S, chunk; float scale; };
int samdec_t2i_ranges(int M);
bool samdec_attn_t2i_ok(const SamDecAttnT2IArgs& a);
void launch_samdec_attn_t2i(const SamDecAttnT2IArgs& a, hipStream_t s);
// Sam.postprocess_masks + threshold: lowres [n][L][L] -> bilinear to size x size -> crop [in_h][in_w] -> bilinear to [H][W]; mask u8 = value > 0, logits optional
struct SamDecPostArgs { const float* lowres; int n, L, size, in_h, in_w, H, W; uint8_t* mask; float* logits; };
bool samdec_post_ok(const SamDecPostArgs& a);
void launch_samdec_post(const SamDecPostArgs& a, hipStream_t s);

}  // namespace ldx
