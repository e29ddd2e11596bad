// Shared pieces of the row-block kernels (rowgemm.hip, xattn_block.hip, ff_block.hip): the LayerNorm prologue of the two C = 320 sub-block kernels
// and the output stage of all three.
// Output stage: their MFMAs leave the results transposed — a lane
// holds one row and 4 consecutive features per accumulator tile — and storing those 8-byte pieces directly wrote every 128-byte line in four or
// more partial bursts from different waves: WRITE_SIZE was 2x the algorithmic bytes (profiles/r03/pmc_util_rowblock.txt) and the store phase
// 11 of xattn_block's 45 us.  Here the finished 16-bit values of 64 rows x 320 features go through an LDS tile and leave as whole 640-byte rows
// (16 bytes per lane, consecutive lanes = consecutive chunks).
#pragma once
#include "ldx_device.h"

namespace ldx {

constexpr int RB_SROW = 320 * 2 + 16;              // bytes per staged row
constexpr int RB_STAGE_BYTES = 64 * RB_SROW;       // 41 984
constexpr int RB_C = 320, RB_BM = 128;             // LayerNorm prologue: features per row, rows per workgroup
constexpr int RB_AROW = RB_C * 2 + 16;             // 656 B per row of the 16-bit A tile: 16 consecutive rows start in 16 different 16-byte bank groups

// LayerNorm of rows m0 .. m0 + 127 of H (rows >= M: zeros) -> 16-bit A tile in LDS (xattn_block.hip, ff_block.hip): 4 lanes per row, the row's 320
// values in registers (80 per lane, as 16-byte chunks part + 4 j), two-pass statistics.  sG / sBt: gamma / beta in LDS, written by the caller before the
// call: the barrier inside makes them visible.  Every thread of the 512-thread workgroup must call it; the caller's barrier after it publishes A.
// no_loads: timing ablation (wrong results), false in normal builds.
template <typename T>
__device__ __forceinline__ void rb_layernorm_rows(const T* __restrict__ Hp, const int ldh, const long m0, const long M, const float eps, const float* sG,
                                                  const float* sBt, char* sA, const int tid, const bool no_loads) {
    const int row = tid >> 2, part = tid & 3;
    const long m = m0 + row;
    float x[80];
    if (m < M && !no_loads) {
#pragma unroll
        for (int j = 0; j < 10; ++j) {
            const uint4 u = *(const uint4*)(Hp + m * ldh + (part + 4 * j) * 8);
            float f[8];
            unpack8<T>(u, f);
#pragma unroll
            for (int e = 0; e < 8; ++e) x[8 * j + e] = f[e];
        }
    } else {
#pragma unroll
        for (int e = 0; e < 80; ++e) x[e] = 0.f;
    }
    float su = 0.f;
#pragma unroll
    for (int e = 0; e < 80; ++e) su += x[e];
    su += dpp_f<0xB1>(su); su += dpp_f<0x4E>(su);
    const float mean = su * (1.0f / RB_C);
    float sq = 0.f;
#pragma unroll
    for (int e = 0; e < 80; ++e) { const float d = x[e] - mean; sq = fmaf(d, d, sq); }
    sq += dpp_f<0xB1>(sq); sq += dpp_f<0x4E>(sq);
    const float rstd = rsqrtf(sq * (1.0f / RB_C) + eps);
    __syncthreads();                                 // gamma / beta in LDS
#pragma unroll
    for (int j = 0; j < 10; ++j) {
        const int c0 = (part + 4 * j) * 8;
        float f[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) f[e] = fmaf((x[8 * j + e] - mean) * rstd, sG[c0 + e], sBt[c0 + e]);
        *(uint4*)(sA + row * RB_AROW + c0 * 2) = pack8<T>(f);
    }
}

// out[t][qt]: the lane's packed values for row 16 qt + l15, features 40 wave + 16 t + 4 g4 .. + 3 (valid when 16 t + 4 g4 < 40) of a 320-wide pass;
// QT = 8 (128 rows, two halves) or 4 (64 rows).  Y + col0 = first feature of the pass; rows m0 .. m0 + 16 QT - 1 (clipped at M).
// dup_rows != 0: every row is also stored at row m + dup_rows.  Every thread of the 512-thread workgroup must call it (barriers inside); sS must not alias anything a slower wave may still read.
template <typename T, int QT>
__device__ __forceinline__ void rb_store_rows(T* __restrict__ Y, const int ldy, const long m0, const long M, const int col0, const int wave, const int l15,
                                              const int g4, const int tid, const uint2 (&out)[3][QT], char* sS, const long dup_rows = 0) {
    // the addresses below are invariant across the callers' pass / chunk loops; left to LICM they are all precomputed and kept live through the
    // MFMA loops (23 spilled dwords in rowgemm): make the lane ids opaque here so that they are recomputed where they are used
    int tid_ = tid, l15_ = l15;
    asm volatile("" : "+v"(tid_), "+v"(l15_));
#pragma unroll
    for (int hh = 0; hh < QT / 4; ++hh) {
#pragma unroll
        for (int t = 0; t < 3; ++t) {
            const int nl = 16 * t + 4 * g4;
            if (nl < 40) {
#pragma unroll
                for (int q4 = 0; q4 < 4; ++q4) *(uint2*)(sS + (16 * q4 + l15_) * RB_SROW + (wave * 40 + nl) * 2) = out[t][4 * hh + q4];
            }
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < 5; ++j) {
            const int idx = tid_ + 512 * j, row = idx / 40, ch = idx - row * 40;
            const long m = m0 + 64 * hh + row;
            if (m < M) {
                const uint4 v = *(const uint4*)(sS + row * RB_SROW + ch * 16);
                *(uint4*)(Y + m * ldy + col0 + ch * 8) = v;
                if (dup_rows) *(uint4*)(Y + (m + dup_rows) * ldy + col0 + ch * 8) = v;       // second half of a shared CFG prefix (RowGemmArgs::dup_rows)
            }
        }
        __syncthreads();
    }
}

}  // namespace ldx
