// Weight packing on the device: the layouts Engine::finalize builds (engine.cpp), from state-dict tensors that already live on the GPU
// (ldx_load_tensor_device).  Run once per load / refresh, memory bound and small next to one sampling run, so the kernels are plain: what
// matters is that every bit equals the host packer's.  Hence
//   - the 16-bit rounding is weight_convert.h's integer code, the one the host calls;
//   - products are single fp32 multiplies (__fmul_rn), sums single fp64 operations (__dadd_rn / __dmul_rn): hipcc contracts a * b + c to an FMA
//     by default and the host build does not.
#include "../../include/ldx.h"
#include "ldx_kernels.h"
#include "weight_convert.h"

namespace ldx {

__device__ __forceinline__ float src_at(const void* p, int dt, size_t i) {
    if (dt == LDX_F32) return ((const float*)p)[i];
    const uint16_t h = ((const uint16_t*)p)[i];
    return dt == LDX_F16 ? half_to_float(h) : bf16_to_float(h);
}
// scale == 1 (the k | v rows, every layout without a q prescale): the host's product is the value itself
__device__ __forceinline__ float scaled(float v, float scale) { return scale == 1.0f ? v : __fmul_rn(v, scale); }
__device__ __forceinline__ uint16_t to16(float v, DType dt) { return dt == DT_BF16 ? float_to_bf16(v) : float_to_half(v); }
__device__ __forceinline__ float from16(uint16_t h, DType dt) { return dt == DT_BF16 ? bf16_to_float(h) : half_to_float(h); }
// GEGLU row layout (engine.cpp src_row): slab s of 64 packed rows = value rows 32 s .. 32 s + 31 of the source, then their gate rows
__device__ __forceinline__ size_t geglu_src_row(size_t r, int inner) {
    if (inner <= 0) return r;
    const size_t slab = r / 64, within = r % 64;
    return within < 32 ? slab * 32 + within : (size_t)inner + slab * 32 + (within - 32);
}
__device__ __forceinline__ uint4 pack8x16(const uint16_t (&h)[8]) {
    uint4 u;
    u.x = h[0] | ((uint32_t)h[1] << 16); u.y = h[2] | ((uint32_t)h[3] << 16);
    u.z = h[4] | ((uint32_t)h[5] << 16); u.w = h[6] | ((uint32_t)h[7] << 16);
    return u;
}

// one thread = eight consecutive output columns of one row (one 16-byte store)
__global__ __launch_bounds__(256) void pack16_kernel(const PackArgs p) {
    const size_t per_row = (size_t)p.K / 8, total = (size_t)p.N * per_row;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        const size_t r = i / per_row, c = (i % per_row) * 8;
        uint16_t h[8];
        if (p.CinPad > 0) {
            const size_t tap = c / p.CinPad, ci = c % p.CinPad;          // CinPad % 8 == 0: the eight columns share the tap
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const float v = (int)(ci + j) < p.Cin ? scaled(src_at(p.src, p.sdt, (r * p.Cin + ci + j) * 9 + tap), p.scale) : 0.f;
                h[j] = to16(v, p.out_dt);
            }
        } else {
            const size_t s0 = geglu_src_row(r, p.geglu_inner) * p.K + c;
#pragma unroll
            for (int j = 0; j < 8; ++j) h[j] = to16(scaled(src_at(p.src, p.sdt, s0 + j), p.scale), p.out_dt);
        }
        *(uint4*)((uint16_t*)p.out + r * (size_t)p.ldo + (size_t)p.col0 + c) = pack8x16(h);
    }
}

__global__ __launch_bounds__(256) void pack32_kernel(const PackVecArgs p) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= p.n) return;
    const size_t s = geglu_src_row((size_t)i, p.geglu_inner);
    float v = src_at(p.a, p.a_dt, s);
    if (p.b) v = __fadd_rn(v, src_at(p.b, p.b_dt, s));
    p.out[i] = v;
}

// one thread per output row: the two fp64 sums run in ascending k, as on the host
__global__ __launch_bounds__(64) void ln_fold_kernel(const LnFoldArgs p) {
    const int r = blockIdx.x * 64 + threadIdx.x;
    if (r >= p.N) return;
    const size_t sr = geglu_src_row((size_t)r, p.geglu_inner);
    double s1 = 0.0, s2 = 0.0;
    for (int k = 0; k < p.K; k += 8) {
        uint16_t h[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const float w = scaled(src_at(p.src, p.sdt, sr * p.K + k + j), p.scale);
            h[j] = to16(__fmul_rn(w, src_at(p.gamma, p.g_dt, k + j)), p.out_dt);
            s1 = __dadd_rn(s1, (double)from16(h[j], p.out_dt));
            s2 = __dadd_rn(s2, __dmul_rn((double)w, (double)src_at(p.beta, p.b_dt, k + j)));
        }
        *(uint4*)((uint16_t*)p.out + (size_t)r * p.K + k) = pack8x16(h);
    }
    p.c1[r] = (float)s1;
    p.c2[r] = (float)__dadd_rn(s2, (double)(p.bias ? src_at(p.bias, p.bias_dt, sr) : 0.f));
}

static int pack_grid(size_t n) { size_t g = (n + 255) / 256; if (g > 16384) g = 16384; if (g < 1) g = 1; return (int)g; }

void launch_pack16(const PackArgs& a, hipStream_t s) {
    if (a.N <= 0 || a.K <= 0) return;
    hipLaunchKernelGGL(pack16_kernel, dim3(pack_grid((size_t)a.N * (a.K / 8))), dim3(256), 0, s, a);
}
void launch_pack32(const PackVecArgs& a, hipStream_t s) {
    if (a.n <= 0) return;
    hipLaunchKernelGGL(pack32_kernel, dim3((a.n + 255) / 256), dim3(256), 0, s, a);
}
void launch_ln_fold(const LnFoldArgs& a, hipStream_t s) {
    if (a.N <= 0) return;
    hipLaunchKernelGGL(ln_fold_kernel, dim3((a.N + 63) / 64), dim3(64), 0, s, a);
}

}  // namespace ldx
