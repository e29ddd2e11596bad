// SAM prompt encoder + mask decoder kernels (segment_anything's PromptEncoder, MaskDecoder / TwoWayTransformer and Sam.postprocess_masks: what turns the image
// embedding and ADetailer's boxes into masks).  Everything is fp32: in 16-bit the full-size logits sit 0.2 - 0.5 (rel-L2) from the fp32 ones.  Linked into
// libldx_samdec.so (csrc/Makefile says why).
//
//   samdec_prompt_kernel     all P prompts' tokens [P][5 + ns][C]: iou_token | mask_tokens | random-Fourier encodings of the points and box corners + label embeddings
//   samdec_transpose_kernel  image embedding [C][g * g] + no_mask_embed -> rows [g * g][C]
//   samdec_gemm_kernel       Y = epilogue((X (+ PE)) W^T + bias) on the exact-fp32 MFMA (16 x 16 x 4), rows of 32 per workgroup (16 where there are no more).  Epilogue, in this order: residual,
//                            LayerNorm over column groups (the whole row, or LayerNorm2d's channels of one output pixel of a 2 x 2 transposed convolution), ReLU / erf-GELU,
//                            and either a store or the product with the hypernetwork vectors, which writes the low-res logits and never the upscaled embedding
//   samdec_attn_small_kernel softmax attention against at most 16 keys (the tokens): the tokens' self-attention and the image rows' attention to the tokens
//   samdec_attn_t2i_kernel   the at most 16 token queries of a (prompt, head) against one range of the g * g image keys: online softmax, partial (max, sum, o)
//   samdec_attn_merge_kernel the ranges' partials -> attention rows
//   samdec_post_kernel       Sam.postprocess_masks + threshold: both bilinear resamplings per output pixel straight from the low-res logits, float for float
//
// No result depends on how many prompts share a launch: a row's arithmetic never involves another row and the key ranges depend on the grid size alone.
#include "../../include/ldx.h"
#include "ldx_device.h"
#include "ldx_kernels.h"

#pragma clang fp contract(off)

namespace ldx {

namespace {
constexpr int GR = 32;                  // rows per workgroup
constexpr int GK = 32, GS = GK + 4;     // K chunk and its LDS row stride (floats)
constexpr int GO = 256 + 4;             // row stride of the epilogue's tile
constexpr float TWO_PI = 6.283185307179586f;
}  // namespace

__global__ __launch_bounds__(256) void samdec_prompt_kernel(const SamDecPromptArgs a) {
    const int C = a.C, half = C / 2, T = 5 + a.ns;
    const long total = (long)a.P * T * C;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const int c = (int)(i % C); const long pt = i / C; const int t = (int)(pt % T), p = (int)(pt / T);
        float v;
        if (t == 0) v = a.iou_token[c];
        else if (t < 5) v = a.mask_tokens[(t - 1) * C + c];
        else {
            const int j = t - 5, npt = a.ns - (a.boxes ? 2 : 0);          // points first (the padding point last of them), then the two corners
            float x = 0.f, y = 0.f; int label = -1, extra = -1;
            if (j < a.n) { x = a.points[((long)p * a.n + j) * 2] + 0.5f; y = a.points[((long)p * a.n + j) * 2 + 1] + 0.5f; label = a.labels[(long)p * a.n + j]; }
            else if (j >= npt) { const int k = j - npt; x = a.boxes[(long)p * 4 + 2 * k] + 0.5f; y = a.boxes[(long)p * 4 + 2 * k + 1] + 0.5f; label = -2; extra = 2 + k; }
            if (label == -1) v = a.not_a_point[c];
            else {
                const float cx = 2.0f * (x / a.size) - 1.0f, cy = 2.0f * (y / a.size) - 1.0f;
                const int f = c < half ? c : c - half;
                const float ang = TWO_PI * (cx * a.gauss[f] + cy * a.gauss[half + f]);
                v = c < half ? sinf(ang) : cosf(ang);
                if (label == 0 || label == 1) extra = label;
                if (extra >= 0) v = v + a.point_emb[extra * C + c];
            }
        }
        a.out[i] = v;
    }
}

__global__ __launch_bounds__(256) void samdec_transpose_kernel(const float* __restrict__ emb, const float* __restrict__ add, float* __restrict__ out, int C, int M) {
    const long total = (long)C * M;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const int c = (int)(i % C); const long m = i / C;
        out[i] = emb[(long)c * M + m] + add[c];
    }
}

// NT: a workgroup covers 32 * NT columns.  FEW = false: waves 0 | 1 take rows 0 .. 15 | 16 .. 31 of the left half of the columns, waves 2 | 3 of the right half, NT
// 16-column MFMA tiles each.  FEW = true (M <= 16: the tokens of one prompt): the four waves share the columns of rows 0 .. 15 instead, NT / 2 tiles each (NT = 1:
// waves 0 and 1 one tile each).  An output element is the same MFMA chain either way.
template <int NT, bool FEW>
__global__ __launch_bounds__(256) void samdec_gemm_kernel(const SamDecGemmArgs a) {
    constexpr int TL = FEW ? (NT > 1 ? NT / 2 : 1) : NT;
    __shared__ float smem[(GR + 256) * GS];
    float* const sX = smem; float* const sW = smem + GR * GS; float* const sOut = smem;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l15 = lane & 15, l4 = lane >> 4;
    const int z = blockIdx.z;
    const long row0 = (long)blockIdx.x * GR;
    const int n0 = blockIdx.y * a.nb;
    const float* const X = a.X + (long)z * a.xz;
    const float* const W = a.W + (long)z * a.wz;
    const bool use_pe = a.PE && n0 < a.pe_cols;

    f32x4 acc[TL];
#pragma unroll
    for (int nt = 0; nt < TL; ++nt) acc[nt] = (f32x4){0.f, 0.f, 0.f, 0.f};
    const int rbase = FEW ? 0 : (wave & 1) * 16, cbase = FEW ? wave * TL * 16 : (wave >> 1) * NT * 16;
    const bool computes = !FEW || NT > 1 || wave < 2;
    const int arow = rbase + l15, bcol = cbase + l15;

    // staging: a thread moves one float4 of the X tile (32 rows x 8) and NT of the W tile (32 NT rows x 8) per chunk.  Every load is unconditional, from an
    // address clamped into the operand, and zeroed afterwards where it is outside it: the loads of a chunk are all in flight at once, and the next chunk's
    // are issued before this chunk's MFMAs
    const int sr = tid >> 3, sk = (tid & 7) * 4;
    const long xgr = row0 + sr;
    const bool x_live = xgr < a.M;
    const float* const xp = X + (x_live ? (a.x_period ? xgr % a.x_period : xgr) : 0) * a.ldx;
    const float* const pp = use_pe ? a.PE + (x_live ? xgr % a.pe_period : 0) * a.ldpe : xp;
    const f32x4 zero4 = (f32x4){0.f, 0.f, 0.f, 0.f};
    f32x4 xv = zero4, wv[NT];
#pragma unroll
    for (int it = 0; it < NT; ++it) wv[it] = zero4;
    for (int k0 = -GK; k0 < a.K; k0 += GK) {          // pass k0: chunk k0 goes from registers to LDS, chunk k0 + GK from memory to registers, then chunk k0's MFMAs
        if (k0 >= 0) {
            __syncthreads();
            *(f32x4*)(sX + sr * GS + sk) = xv;
#pragma unroll
            for (int it = 0; it < NT; ++it) *(f32x4*)(sW + (it * 32 + sr) * GS + sk) = wv[it];
            __syncthreads();
        }
        if (k0 + GK < a.K) {
            const int k = k0 + GK + sk; const bool kin = k < a.K; const int kc = kin ? k : 0;
            f32x4 v = *(const f32x4*)(xp + kc);
            if (use_pe) v = v + *(const f32x4*)(pp + kc);
            xv = x_live && kin ? v : zero4;
#pragma unroll
            for (int it = 0; it < NT; ++it) {
                const int n = it * 32 + sr; const bool w_live = n < a.nb && n0 + n < a.N;
                const f32x4 w = *(const f32x4*)(W + (long)(w_live ? n0 + n : n0) * a.K + kc);
                wv[it] = w_live && kin ? w : zero4;
            }
        }
        if (k0 >= 0 && computes) {
#pragma unroll
            for (int kk = 0; kk < GK / 4; ++kk) {
                const float av = sX[arow * GS + kk * 4 + l4];
#pragma unroll
                for (int nt = 0; nt < TL; ++nt) acc[nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, sW[(bcol + nt * 16) * GS + kk * 4 + l4], acc[nt], 0, 0, 0);
            }
        }
    }
    __syncthreads();
#pragma unroll
    for (int nt = 0; nt < TL; ++nt)
#pragma unroll
        for (int r = 0; r < 4; ++r) if (computes) sOut[(rbase + 4 * l4 + r) * GO + cbase + nt * 16 + l15] = acc[nt][r];
    __syncthreads();

    // row space: eight consecutive lanes own a row, lane `sub` its columns sub, sub + 8, ...
    const int r = tid >> 3, sub = tid & 7;
    const long gr = row0 + r;
    const bool live = gr < a.M;
    int nv = a.N - n0; if (nv > a.nb) nv = a.nb;
    float* const row = sOut + r * GO;
    const float* const bias = a.bias ? a.bias + (long)z * a.bz + n0 : nullptr;
    if (bias || a.R)
        for (int c = sub; c < nv; c += 8) {
            float v = row[c];
            if (bias) v = v + bias[c];
            if (a.R && live) v = v + a.R[(a.r_period ? gr % a.r_period : gr) * a.ldr + n0 + c];
            row[c] = v;
        }
    if (a.ln_group > 0) {
        const float inv = 1.0f / (float)a.ln_group;
        for (int g0 = 0; g0 < nv; g0 += a.ln_group) {
            float s = 0.f;
            for (int c = g0 + sub; c < g0 + a.ln_group; c += 8) s += row[c];
            s += __shfl_xor(s, 1); s += __shfl_xor(s, 2); s += __shfl_xor(s, 4);
            const float mean = s * inv;
            float q = 0.f;
            for (int c = g0 + sub; c < g0 + a.ln_group; c += 8) { const float d = row[c] - mean; q += d * d; }
            q += __shfl_xor(q, 1); q += __shfl_xor(q, 2); q += __shfl_xor(q, 4);
            const float rstd = 1.0f / sqrtf(q * inv + a.eps);
            for (int c = g0 + sub; c < g0 + a.ln_group; c += 8) row[c] = (row[c] - mean) * rstd * a.gamma[c - g0] + a.beta[c - g0];
        }
    }
    if (a.act)
        for (int c = sub; c < nv; c += 8) { const float v = row[c]; row[c] = a.act == 1 ? fmaxf(v, 0.f) : 0.5f * v * (1.0f + erff(v * 0.70710678118654752440f)); }
    if (!a.hyper) {
        if (live) {
            float* const y = a.Y + (long)z * a.yz + gr * a.ldy + n0;
            for (int c = sub; c < nv; c += 8) y[c] = row[c];
        }
        return;
    }
    // rows are the 2 x 2 children of the grid's pixels, column group q the child's own 2 x 2 children; lane sub: group sub >> 1, masks 2 (sub & 1) and + 1
    __syncthreads();
    if (live) {
        const int G = a.N / 4, q = sub >> 1, g = a.g;
        const long per = 4L * g * g, p = gr / per; const int rem = (int)(gr - p * per), pix = rem >> 2, d1 = rem & 3;
        const int py = pix / g, px = pix - py * g;
        const int oy = 4 * py + 2 * (d1 >> 1) + (q >> 1), ox = 4 * px + 2 * (d1 & 1) + (q & 1);
#pragma unroll
        for (int mm = 0; mm < 2; ++mm) {
            const int m = 2 * (sub & 1) + mm;
            const float* const hv = a.hyper + (p * 4 + m) * G;
            float s = 0.f;
            for (int c = 0; c < G; ++c) s += row[q * G + c] * hv[c];
            a.logits[((p * 4 + m) * (4L * g) + oy) * (4L * g) + ox] = s;
        }
    }
}

__global__ __launch_bounds__(256) void samdec_attn_small_kernel(const SamDecAttnSmallArgs a) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;          // one (row, head) per thread; hd % 4 == 0, rows 16-byte aligned
    if (i >= (long)a.B * a.Tq * a.H) return;
    const int h = (int)(i % a.H), hd = a.hd, Tk = a.Tk; const long row = i / a.H, b = row / a.Tq;
    const float* const q = a.Q + (a.q_shared ? row - b * a.Tq : row) * a.ldq + h * hd;
    const float* const K = a.K + b * Tk * a.ldk + h * hd;
    float s[16];
#pragma unroll
    for (int t = 0; t < 16; ++t) s[t] = 0.f;
    for (int e = 0; e < hd; e += 4) {
        const f32x4 qv = *(const f32x4*)(q + e);
#pragma unroll
        for (int t = 0; t < 16; ++t)
            if (t < Tk) { const f32x4 kv = *(const f32x4*)(K + (long)t * a.ldk + e); s[t] += qv[0] * kv[0]; s[t] += qv[1] * kv[1]; s[t] += qv[2] * kv[2]; s[t] += qv[3] * kv[3]; }
    }
    float m = -INFINITY;
#pragma unroll
    for (int t = 0; t < 16; ++t) if (t < Tk) { s[t] = s[t] * a.scale; m = fmaxf(m, s[t]); }
    float sum = 0.f;
#pragma unroll
    for (int t = 0; t < 16; ++t) { const float p = t < Tk ? expf(s[t] - m) : 0.f; s[t] = p; sum += p; }
    const float inv = 1.0f / sum;
    const float* const V = a.V + b * Tk * a.ldv + h * hd;
    float* const o = a.O + row * a.ldo + h * hd;
    for (int e = 0; e < hd; e += 4) {
        f32x4 acc = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int t = 0; t < 16; ++t) if (t < Tk) acc = acc + s[t] * *(const f32x4*)(V + (long)t * a.ldv + e);
        *(f32x4*)(o + e) = acc * inv;
    }
}

// grid (ranges, heads, prompts); thread (query t = tid >> 4, key lane tid & 15).  Partial: part[((b H + h) S + s) 16 + t][HD + 2] = max, sum, o[HD]
template <int HD>
__global__ __launch_bounds__(256) void samdec_attn_t2i_kernel(const SamDecAttnT2IArgs a) {
    const int tid = threadIdx.x, t = tid >> 4, kl = tid & 15;
    const int s = blockIdx.x, h = blockIdx.y, b = blockIdx.z;
    const bool active = t < a.T;
    float q[HD], o[HD];
    const float* const qp = a.Q + ((long)b * a.T + (active ? t : 0)) * a.ldq + h * HD;
#pragma unroll
    for (int e = 0; e < HD; ++e) { q[e] = qp[e]; o[e] = 0.f; }
    const long kbase = a.kv_shared ? 0 : (long)b * a.M;
    const int k_end = min(a.M, (s + 1) * a.chunk);
    float m = -INFINITY, l = 0.f;
    for (int k = s * a.chunk + kl; k < k_end; k += 16) {
        const float* const kp = a.K + (kbase + k) * a.ldk + h * HD;
        const float* const vp = a.V + (kbase + k) * a.ldv + h * HD;
        float d = 0.f;
#pragma unroll
        for (int e = 0; e < HD; e += 4) { const float4 kv = *(const float4*)(kp + e); d += q[e] * kv.x; d += q[e + 1] * kv.y; d += q[e + 2] * kv.z; d += q[e + 3] * kv.w; }
        d = d * a.scale;
        const float mn = fmaxf(m, d), al = expf(m - mn), p = expf(d - mn);
        m = mn; l = l * al + p;
#pragma unroll
        for (int e = 0; e < HD; e += 4) {
            const float4 vv = *(const float4*)(vp + e);
            o[e] = o[e] * al + p * vv.x; o[e + 1] = o[e + 1] * al + p * vv.y; o[e + 2] = o[e + 2] * al + p * vv.z; o[e + 3] = o[e + 3] * al + p * vv.w;
        }
    }
    // the 16 key lanes of a query: consecutive lanes of one wave
    float mt = m;
#pragma unroll
    for (int x = 1; x < 16; x <<= 1) mt = fmaxf(mt, __shfl_xor(mt, x));
    const float f = m == -INFINITY ? 0.f : expf(m - mt);
    l = l * f;
#pragma unroll
    for (int x = 1; x < 16; x <<= 1) l += __shfl_xor(l, x);
#pragma unroll
    for (int e = 0; e < HD; ++e) {
        float v = o[e] * f;
#pragma unroll
        for (int x = 1; x < 16; x <<= 1) v += __shfl_xor(v, x);
        o[e] = v;
    }
    if (active && kl == 0) {
        float* const out = a.part + ((((long)b * a.H + h) * a.S + s) * 16 + t) * (HD + 2);
        out[0] = mt; out[1] = l;
#pragma unroll
        for (int e = 0; e < HD; ++e) out[2 + e] = o[e];
    }
}

__global__ __launch_bounds__(256) void samdec_attn_merge_kernel(const SamDecAttnT2IArgs a) {
    const int hd = a.hd;
    const long total = (long)a.B * a.T * a.H * hd;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const int e = (int)(i % hd); long r = i / hd; const int h = (int)(r % a.H); r /= a.H; const int t = (int)(r % a.T); const long b = r / a.T;
        const float* const base = a.part + (((b * a.H + h) * a.S) * 16 + t) * (hd + 2);
        const long step = 16L * (hd + 2);
        float m = -INFINITY;
        for (int s = 0; s < a.S; ++s) m = fmaxf(m, base[s * step]);
        float l = 0.f, o = 0.f;
        for (int s = 0; s < a.S; ++s) { const float f = expf(base[s * step] - m); l += f * base[s * step + 1]; o += f * base[s * step + 2 + e]; }
        a.O[(b * a.T + t) * a.ldo + h * hd + e] = o / l;
    }
}

// One bilinear tap pair of F.interpolate(align_corners=False): source index scale * (dst + 0.5) - 0.5 clamped at 0, its floor, the next sample (clamped) and the weight
__device__ __forceinline__ void bil_src(int dst, float scale, int in, int& i0, int& i1, float& lam) {
    float s = scale * ((float)dst + 0.5f) - 0.5f;
    if (s < 0.f) s = 0.f;
    i0 = (int)s; if (i0 > in - 1) i0 = in - 1;
    i1 = i0 + (i0 < in - 1 ? 1 : 0);
    lam = s - (float)i0;
}
// the first resampling (4 g -> size) at (y, x) of the size x size frame
__device__ __forceinline__ float post_stage1(const float* __restrict__ lr, int L, float sc1, int y, int x) {
    int y0, y1, x0, x1; float ly, lx;
    bil_src(y, sc1, L, y0, y1, ly);
    bil_src(x, sc1, L, x0, x1, lx);
    const float wy = 1.0f - ly, wx = 1.0f - lx;
    const float top = lr[(long)y0 * L + x0] * wx + lr[(long)y0 * L + x1] * lx;
    const float bot = lr[(long)y1 * L + x0] * wx + lr[(long)y1 * L + x1] * lx;
    return top * wy + bot * ly;
}
__global__ __launch_bounds__(256) void samdec_post_kernel(const SamDecPostArgs a) {
    const long plane = (long)a.H * a.W, total = (long)a.n * plane;
    const float sc1 = (float)a.L / (float)a.size, sch = (float)a.in_h / (float)a.H, scw = (float)a.in_w / (float)a.W;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const long k = i / plane; const long r = i - k * plane; const int y = (int)(r / a.W), x = (int)(r - (long)y * a.W);
        const float* const lr = a.lowres + k * a.L * a.L;
        int y0, y1, x0, x1; float ly, lx;
        bil_src(y, sch, a.in_h, y0, y1, ly);
        bil_src(x, scw, a.in_w, x0, x1, lx);
        const float wy = 1.0f - ly, wx = 1.0f - lx;
        const float top = post_stage1(lr, a.L, sc1, y0, x0) * wx + post_stage1(lr, a.L, sc1, y0, x1) * lx;
        const float bot = post_stage1(lr, a.L, sc1, y1, x0) * wx + post_stage1(lr, a.L, sc1, y1, x1) * lx;
        const float v = top * wy + bot * ly;
        a.mask[i] = v > 0.0f ? 1 : 0;
        if (a.logits) a.logits[i] = v;
    }
}

static unsigned flat_grid(long total) { const long g = (total + 255) / 256; return (unsigned)(g < 1 ? 1 : g > 16384 ? 16384 : g); }

void launch_samdec_prompt(const SamDecPromptArgs& a, hipStream_t s) {
    if (!a.out || a.P <= 0 || a.ns <= 0) return;
    hipLaunchKernelGGL(samdec_prompt_kernel, dim3(flat_grid((long)a.P * (5 + a.ns) * a.C)), dim3(256), 0, s, a);
}

void launch_samdec_transpose(const float* emb, const float* add, float* out, int C, int M, hipStream_t s) {
    if (!emb || !add || !out || C <= 0 || M <= 0) return;
    hipLaunchKernelGGL(samdec_transpose_kernel, dim3(flat_grid((long)C * M)), dim3(256), 0, s, emb, add, out, C, M);
}

bool samdec_gemm_ok(const SamDecGemmArgs& a) {
    if (!a.X || !a.W || a.M <= 0 || a.N <= 0 || a.K <= 0 || a.nb <= 0 || a.nb > 256 || a.nz <= 0 || a.nz > 65535 || a.ldx <= 0) return false;
    if ((a.M + GR - 1) / GR > 0x7fffffffL || (a.N + a.nb - 1) / a.nb > 65535) return false;
    if (a.K % 4 || a.ldx % 4 || a.xz % 4 || a.wz % 4 || (uintptr_t)a.X % 16 || (uintptr_t)a.W % 16) return false;          // float4 loads
    if (a.PE && (a.pe_period <= 0 || a.ldpe <= 0 || a.ldpe % 4 || (uintptr_t)a.PE % 16)) return false;
    if (a.R && a.ldr <= 0) return false;
    if (a.ln_group && (a.ln_group % 8 || a.nb % a.ln_group || a.N % a.ln_group || (a.N > a.nb && a.nb % a.ln_group) || !a.gamma || !a.beta)) return false;
    if (a.act < 0 || a.act > 2) return false;
    if (a.hyper) return a.logits && a.N % 4 == 0 && a.N <= a.nb && a.g > 0 && a.nz == 1 && a.M % (4L * a.g * a.g) == 0;
    return a.Y && a.ldy > 0;
}
void launch_samdec_gemm(const SamDecGemmArgs& a, hipStream_t s) {
    if (!samdec_gemm_ok(a)) return;
    const dim3 grid((unsigned)((a.M + GR - 1) / GR), (unsigned)((a.N + a.nb - 1) / a.nb), (unsigned)a.nz);
    const int nt = a.nb <= 32 ? 1 : a.nb <= 64 ? 2 : a.nb <= 128 ? 4 : 8;
    if (a.M <= 16) {
        if (nt == 1) hipLaunchKernelGGL((samdec_gemm_kernel<1, true>), grid, dim3(256), 0, s, a);
        else if (nt == 2) hipLaunchKernelGGL((samdec_gemm_kernel<2, true>), grid, dim3(256), 0, s, a);
        else if (nt == 4) hipLaunchKernelGGL((samdec_gemm_kernel<4, true>), grid, dim3(256), 0, s, a);
        else hipLaunchKernelGGL((samdec_gemm_kernel<8, true>), grid, dim3(256), 0, s, a);
    } else {
        if (nt == 1) hipLaunchKernelGGL((samdec_gemm_kernel<1, false>), grid, dim3(256), 0, s, a);
        else if (nt == 2) hipLaunchKernelGGL((samdec_gemm_kernel<2, false>), grid, dim3(256), 0, s, a);
        else if (nt == 4) hipLaunchKernelGGL((samdec_gemm_kernel<4, false>), grid, dim3(256), 0, s, a);
        else hipLaunchKernelGGL((samdec_gemm_kernel<8, false>), grid, dim3(256), 0, s, a);
    }
}

bool samdec_attn_small_ok(const SamDecAttnSmallArgs& a) {
    return a.Q && a.K && a.V && a.O && a.B > 0 && a.Tq > 0 && a.Tk > 0 && a.Tk <= 16 && a.H > 0 && a.hd > 0 && a.hd % 4 == 0 && a.ldq % 4 == 0 && a.ldk % 4 == 0 && a.ldv % 4 == 0 && a.ldo % 4 == 0 &&
           (uintptr_t)a.Q % 16 == 0 && (uintptr_t)a.K % 16 == 0 && (uintptr_t)a.V % 16 == 0 && (uintptr_t)a.O % 16 == 0 && (long)a.B * a.Tq * a.H < (1L << 39) && a.ldq >= a.H * a.hd && a.ldk >= a.H * a.hd && a.ldv >= a.H * a.hd && a.ldo >= a.H * a.hd;
}
void launch_samdec_attn_small(const SamDecAttnSmallArgs& a, hipStream_t s) {
    if (!samdec_attn_small_ok(a)) return;
    hipLaunchKernelGGL(samdec_attn_small_kernel, dim3((unsigned)(((long)a.B * a.Tq * a.H + 255) / 256)), dim3(256), 0, s, a);
}

int samdec_t2i_ranges(int M) { int S = (M + 255) / 256; if (S > 16) S = 16; if (S < 1) S = 1; const int chunk = (M + S - 1) / S; return (M + chunk - 1) / chunk; }
bool samdec_attn_t2i_ok(const SamDecAttnT2IArgs& a) {
    if (!a.Q || !a.K || !a.V || !a.part || !a.O || a.B <= 0 || a.B > 65535 || a.T <= 0 || a.T > 16 || a.M <= 0 || a.H <= 0 || a.H > 65535) return false;
    if (a.hd != 8 && a.hd != 16 && a.hd != 32) return false;
    if (a.S <= 0 || a.chunk <= 0 || (long)(a.S - 1) * a.chunk >= a.M || (long)a.S * a.chunk < a.M) return false;          // every range holds a key
    return a.ldq >= a.H * a.hd && a.ldk % 4 == 0 && a.ldv % 4 == 0 && a.ldk >= a.H * a.hd && a.ldv >= a.H * a.hd && a.ldo >= a.H * a.hd &&
           (uintptr_t)a.K % 16 == 0 && (uintptr_t)a.V % 16 == 0;
}
void launch_samdec_attn_t2i(const SamDecAttnT2IArgs& a, hipStream_t s) {
    if (!samdec_attn_t2i_ok(a)) return;
    const dim3 grid((unsigned)a.S, (unsigned)a.H, (unsigned)a.B);
    if (a.hd == 8) hipLaunchKernelGGL(samdec_attn_t2i_kernel<8>, grid, dim3(256), 0, s, a);
    else if (a.hd == 16) hipLaunchKernelGGL(samdec_attn_t2i_kernel<16>, grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL(samdec_attn_t2i_kernel<32>, grid, dim3(256), 0, s, a);
    hipLaunchKernelGGL(samdec_attn_merge_kernel, dim3(flat_grid((long)a.B * a.T * a.H * a.hd)), dim3(256), 0, s, a);
}

bool samdec_post_ok(const SamDecPostArgs& a) {
    return a.lowres && a.mask && a.n > 0 && a.L > 0 && a.size > 0 && a.in_h > 0 && a.in_w > 0 && a.in_h <= a.size && a.in_w <= a.size && a.H > 0 && a.W > 0 &&
           a.L <= 16384 && a.size <= 16384 && a.H <= 32768 && a.W <= 32768;
}
void launch_samdec_post(const SamDecPostArgs& a, hipStream_t s) {
    if (!samdec_post_ok(a)) return;
    hipLaunchKernelGGL(samdec_post_kernel, dim3(flat_grid((long)a.n * a.H * a.W)), dim3(256), 0, s, a);
}

}  // namespace ldx
