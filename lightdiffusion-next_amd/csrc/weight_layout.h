// The packed weight layouts, interpreted once for both sides.  A packed buffer is described by pieces (Engine::Piece / VecPiece -> PackArgs / PackVecArgs /
// LnFoldArgs, ldx_kernels.h); the functions below turn a piece into bits.  pack.hip's kernels are grid-stride loops over them with device pointers, the host
// packers (engine.cpp pack16 / pack32 / mk_ln_folded) are CPU loops over them with host pointers: the two cannot disagree about an index.  Nor about a bit:
// the 16-bit rounding is weight_convert.h's integer code, and every floating-point operation that rounds goes through one of the four wrappers below, a single
// correctly rounded operation on either side whatever the target's contraction default is.
#pragma once
#include "../../include/ldx.h"
#include "ldx_kernels.h"
#include "weight_convert.h"

namespace ldx {

// The plain operator with contraction switched off where it is written, the same text for both sides.  (Not the __fmul_rn family: in HIP those are header
// inlines of the plain operator, and the pragma, being lexical, would not reach into them: hipcc fuses add_rn(mul_rn(a, b), c) built on them to one FMA.)
__host__ __device__ inline float mul_rn(float a, float b) { _Pragma("clang fp contract(off)") return a * b; }
__host__ __device__ inline float add_rn(float a, float b) { _Pragma("clang fp contract(off)") return a + b; }
__host__ __device__ inline double dmul_rn(double a, double b) { _Pragma("clang fp contract(off)") return a * b; }
__host__ __device__ inline double dadd_rn(double a, double b) { _Pragma("clang fp contract(off)") return a + b; }

__host__ __device__ inline float src_at(const void* p, int dt, size_t i) {
    if (dt == LDX_F32) return ((const float*)p)[i];
    const uint16_t h = ((const uint16_t*)p)[i];
    return dt == LDX_F16 ? half_to_float(h) : bf16_to_float(h);
}
// scale == 1 (the k | v rows, every layout without a q prescale): the value itself
__host__ __device__ inline float scaled(float v, float scale) { return scale == 1.0f ? v : mul_rn(v, scale); }
__host__ __device__ inline uint16_t to16(float v, DType dt) { return dt == DT_BF16 ? float_to_bf16(v) : float_to_half(v); }
__host__ __device__ inline float from16(uint16_t h, DType dt) { return dt == DT_BF16 ? bf16_to_float(h) : half_to_float(h); }
// GEGLU row layout: slab s of 64 packed rows = value rows 32 s .. 32 s + 31 of the source, then their gate rows (inner <= 0: rows as they are)
__host__ __device__ inline size_t geglu_src_row(size_t r, int inner) {
    if (inner <= 0) return r;
    const size_t slab = r / 64, within = r % 64;
    return within < 32 ? slab * 32 + within : (size_t)inner + slab * 32 + (within - 32);
}
// n <= 8 packed elements to their place: one 16-byte store for a full group (the kernels launch only where every group is full and aligned)
__host__ __device__ inline void store16s(uint16_t* dst, const uint16_t (&h)[8], int n) {
#ifdef __HIP_DEVICE_COMPILE__
    if (n == 8) {
        uint4 u;
        u.x = h[0] | ((uint32_t)h[1] << 16); u.y = h[2] | ((uint32_t)h[3] << 16);
        u.z = h[4] | ((uint32_t)h[5] << 16); u.w = h[6] | ((uint32_t)h[7] << 16);
        *(uint4*)dst = u;
        return;
    }
#endif
    for (int j = 0; j < n; ++j) dst[j] = h[j];
}

// PackArgs: elements (r, c) .. (r, c + n - 1), n <= 8, of the piece, stored at out[r][col0 + c ..]
__host__ __device__ inline void pack16_group(const PackArgs& p, size_t r, size_t c, int n) {
    uint16_t h[8];
    if (p.CinPad > 0) {          // 3x3 conv: column = tap * CinPad + ci, zero beyond Cin
        size_t tap = c / p.CinPad, ci = c % p.CinPad;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            if (j < n) h[j] = to16((int)ci < p.Cin ? scaled(src_at(p.src, p.sdt, (r * p.Cin + ci) * 9 + tap), p.scale) : 0.f, p.out_dt);
            if (++ci == (size_t)p.CinPad) { ci = 0; ++tap; }
        }
    } else {
        const size_t s0 = geglu_src_row(r, p.geglu_inner) * p.K + c;
#pragma unroll
        for (int j = 0; j < 8; ++j) if (j < n) h[j] = to16(scaled(src_at(p.src, p.sdt, s0 + j), p.scale), p.out_dt);
    }
    store16s((uint16_t*)p.out + r * (size_t)p.ldo + (size_t)p.col0 + c, h, n);
}

// PackVecArgs: element i
__host__ __device__ inline void pack32_at(const PackVecArgs& p, size_t i) {
    const size_t s = geglu_src_row(i, p.geglu_inner);
    const float v = src_at(p.a, p.a_dt, s);
    p.out[i] = p.b ? add_rn(v, src_at(p.b, p.b_dt, s)) : v;
}

// LnFoldArgs: row r — the folded 16-bit row, c1[r] and c2[r]; the two fp64 sums run in ascending k
__host__ __device__ inline void ln_fold_group(const LnFoldArgs& p, size_t r, size_t sr, int k, int n, double& s1, double& s2) {
    uint16_t h[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) if (j < n) {
        const float w = scaled(src_at(p.src, p.sdt, sr * p.K + k + j), p.scale);
        h[j] = to16(mul_rn(w, src_at(p.gamma, p.g_dt, k + j)), p.out_dt);
        s1 = dadd_rn(s1, (double)from16(h[j], p.out_dt));
        s2 = dadd_rn(s2, dmul_rn((double)w, (double)src_at(p.beta, p.b_dt, k + j)));
    }
    store16s((uint16_t*)p.out + r * (size_t)p.K + k, h, n);
}
__host__ __device__ inline void ln_fold_row(const LnFoldArgs& p, size_t r) {
    const size_t sr = geglu_src_row(r, p.geglu_inner);
    double s1 = 0.0, s2 = 0.0;
    int k = 0;
    for (; k + 8 <= p.K; k += 8) ln_fold_group(p, r, sr, k, 8, s1, s2);
    if (k < p.K) ln_fold_group(p, r, sr, k, p.K - k, s1, s2);
    p.c1[r] = (float)s1;
    p.c2[r] = (float)dadd_rn(s2, (double)(p.bias ? src_at(p.bias, p.bias_dt, sr) : 0.f));
}

// UpPhaseArgs: the phase weights of a nearest-2x upsample + 3x3 conv (GemmArgs::up2x), [phase = 2 py + px][N][(ty * 2 + tx) * Cin + ci].  Output pixel (2 i + py, 2 j + px)
// reads the stored rows i - 1 + py + ty, ty = 0 / 1: at py = 0 they stand for the taps ky = {0} / {1, 2}, at py = 1 for ky = {0, 1} / {2}; columns alike.  An entry is the sum of
// its 1, 2 or 4 taps of the packed 9-tap matrix [N][(ky * 3 + kx) * Cin + ci], added in fp32 in ascending (ky, kx) and rounded once.
// up_phase_taps: the taps k0 .. k1 behind position t of parity par.  up_phase_group: elements (row, c) .. (row, c + 7) of the [4 * N][4 * Cin] buffer, Cin % 8 == 0.
__host__ __device__ inline void up_phase_taps(int par, int t, int& k0, int& k1) { k0 = t ? 1 + par : 0; k1 = t ? 2 : par; }
__host__ __device__ inline void up_phase_group(const UpPhaseArgs& p, size_t row, size_t c) {
    const int phase = (int)(row / p.N), tap = (int)(c / p.Cin);
    const size_t n = row % p.N, ci = c % p.Cin;
    int ky0, ky1, kx0, kx1;
    up_phase_taps(phase >> 1, tap >> 1, ky0, ky1);
    up_phase_taps(phase & 1, tap & 1, kx0, kx1);
    float acc[8];
    for (int ky = ky0; ky <= ky1; ++ky)
        for (int kx = kx0; kx <= kx1; ++kx) {
            const uint16_t* src = (const uint16_t*)p.W9 + (n * 9 + ky * 3 + kx) * p.Cin + ci;
#pragma unroll
            for (int j = 0; j < 8; ++j) { const float v = from16(src[j], p.dt); acc[j] = (ky == ky0 && kx == kx0) ? v : add_rn(acc[j], v); }
        }
    uint16_t h[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) h[j] = to16(acc[j], p.dt);
    store16s((uint16_t*)p.Wp + row * 4 * (size_t)p.Cin + c, h, 8);
}

}  // namespace ldx
