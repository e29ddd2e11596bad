// AutoHDR, the reference's default post-effect (src/AutoHDR/ahdr.py:83-127, HDREffects.apply_hdr2), on HWC images of the device: two launches per call.
// Every step is an integer rule or a single float32 operation (include/ldx.h states them; lightdiffusion-next_amd/hdr.py is the same thing in numpy),
// so the bytes are those of the numpy statement whatever the order of the threads.  Plain C++, linked into libldx_hdr.so (csrc/Makefile says why).
//
// The two LittleCMS transforms are 33^3 tables of 4 x uint16 per node (287 496 B each, the fourth value padding): too large for LDS, shared by every
// workgroup, served from L2; a pixel reads four nodes per table, one 8-byte load each.  The 256-byte luminance table sits in LDS.
#include "../../include/ldx.h"
#include "ldx_kernels.h"

namespace ldx {

constexpr int HDR_GRID = 33;

// lcms's 8-bit input stage: byte -> cell index (i0 * stride), rest r in 1/65536 of a cell, and the step to the cell's far node (0 at the last node)
struct HdrAxis { int base, step, r; };
__device__ __forceinline__ HdrAxis hdr_axis(unsigned v, int stride) {
    const unsigned a = 32u * 257u * v;
    const unsigned fx = a + (a + 0x7FFFu) / 0xFFFFu;
    const int i0 = (int)(fx >> 16);
    HdrAxis x;
    x.base = i0 * stride;
    x.step = i0 < HDR_GRID - 1 ? stride : 0;
    x.r = (int)(fx & 0xFFFFu);
    return x;
}
__device__ __forceinline__ void hdr_order(HdrAxis& hi, HdrAxis& lo) {
    if (lo.r > hi.r) { const HdrAxis t = hi; hi = lo; lo = t; }
}
__device__ __forceinline__ unsigned hdr_out8(unsigned t0, unsigned t1, unsigned t2, unsigned t3, int r0, int r1, int r2) {
    // differences of 16-bit values times 16-bit rests: each product fits 33 bits, the sum 35: 64-bit, arithmetic shifts
    long long rest = (long long)((int)t1 - (int)t0) * r0 + (long long)((int)t2 - (int)t1) * r1 + (long long)((int)t3 - (int)t2) * r2 + 0x8001;
    const int out16 = (int)t0 + (int)((rest + (rest >> 16)) >> 16);
    return ((unsigned)out16 * 65281u + 8388608u) >> 24;
}
// The tetrahedral read: from node (i0, i0, i0) raise one coordinate at a time, largest rest first (equal rests give the same sum in either order).
// x, y, z in, x, y, z out; the first channel has the largest stride.  Every index lies inside the table for any byte: i0 <= 32, and step is 0 there.
__device__ __forceinline__ void hdr_table_read(const uint2* __restrict__ T, unsigned& x, unsigned& y, unsigned& z) {
    HdrAxis a = hdr_axis(x, HDR_GRID * HDR_GRID), b = hdr_axis(y, HDR_GRID), c = hdr_axis(z, 1);
    const int n0 = a.base + b.base + c.base;
    hdr_order(a, b); hdr_order(a, c); hdr_order(b, c);
    const int n1 = n0 + a.step, n2 = n1 + b.step, n3 = n2 + c.step;
    const uint2 q0 = T[n0], q1 = T[n1], q2 = T[n2], q3 = T[n3];
    x = hdr_out8(q0.x & 0xFFFFu, q1.x & 0xFFFFu, q2.x & 0xFFFFu, q3.x & 0xFFFFu, a.r, b.r, c.r);
    y = hdr_out8(q0.x >> 16, q1.x >> 16, q2.x >> 16, q3.x >> 16, a.r, b.r, c.r);
    z = hdr_out8(q0.y & 0xFFFFu, q1.y & 0xFFFFu, q2.y & 0xFFFFu, q3.y & 0xFFFFu, a.r, b.r, c.r);
}

// tensor2pil: (uint8) trunc(clamp(255.0f * v, 0, 255)); NaN -> 0
__device__ __forceinline__ unsigned hdr_quantize(float v) {
    float c = v * 255.0f;
    c = c >= 0.0f ? c : 0.0f;
    c = c <= 255.0f ? c : 255.0f;
    return (unsigned)(int)c;
}
// Pillow's RGB -> L
__device__ __forceinline__ unsigned hdr_grey(unsigned r, unsigned g, unsigned b) { return (r * 19595u + g * 38470u + b * 7471u + 0x8000u) >> 16; }
// Pillow's Image.blend: a float32 product and a float32 sum, each rounded, t <= 0 -> 0, t >= 255 -> 255, else truncate.  hipcc contracts a * b + c to an
// fma by default, and HIP's __fmul_rn / __fadd_rn are plain operators that it contracts as well (the first build did: bytes one code off); the pragma
// takes the contract flag off these operations, through inlining too.
__device__ __forceinline__ unsigned hdr_blend(float deg, unsigned v, float f) {
#pragma clang fp contract(off)
    const float d = (float)v - deg;
    const float p = f * d;
    const float t = deg + p;
    return t <= 0.0f ? 0u : (t >= 255.0f ? 255u : (unsigned)(int)t);
}
// sum over the 256 threads of a block, returned in every thread
__device__ __forceinline__ unsigned hdr_block_sum(unsigned v, unsigned* red) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return red[0] + red[1] + red[2] + red[3];
}

// ---- the single table read (parity tests) --------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void hdr_table_kernel(const uint8_t* __restrict__ in, long in_pitch, uint8_t* __restrict__ out, long out_pitch,
                                                        int H, int W, const uint2* __restrict__ T) {
    const long total = (long)H * W;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const long row = i / W; const int col = (int)(i % W);
        const uint8_t* s = in + row * in_pitch + (long)col * 3;
        unsigned x = s[0], y = s[1], z = s[2];
        hdr_table_read(T, x, y, z);
        uint8_t* d = out + row * out_pitch + (long)col * 3;
        d[0] = (uint8_t)x; d[1] = (uint8_t)y; d[2] = (uint8_t)z;
    }
}

// ---- kernel A: quantise, sRGB -> Lab, L = lut[L], Lab -> sRGB into the workspace, per-block sums of Pillow's grey ---------------------------------
// grid (blocks, B); block (x, b) writes partial[b][x], so the sum needs no zeroed memory and no atomics
template <bool F32>
__global__ __launch_bounds__(256) void hdr_lab_kernel(const float* __restrict__ in_f, const uint8_t* __restrict__ in_u, long in_pitch, int H, int W,
                                                      const uint2* __restrict__ fwd, const uint2* __restrict__ inv, const uint8_t* __restrict__ lut_g,
                                                      uint8_t* __restrict__ rgb, unsigned* __restrict__ partial) {
    __shared__ uint8_t lut[256];
    __shared__ unsigned red[4];
    lut[threadIdx.x] = lut_g[threadIdx.x];
    __syncthreads();
    const int b = blockIdx.y;
    const long total = (long)H * W;
    const float* sf = F32 ? in_f + (long)b * total * 3 : nullptr;
    const uint8_t* su = F32 ? nullptr : in_u + (long)b * H * in_pitch;
    uint8_t* dst = rgb + (long)b * total * 3;
    unsigned sum = 0;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        unsigned x, y, z;
        if (F32) { x = hdr_quantize(sf[i * 3]); y = hdr_quantize(sf[i * 3 + 1]); z = hdr_quantize(sf[i * 3 + 2]); }
        else { const uint8_t* s = su + (i / W) * in_pitch + (i % W) * 3; x = s[0]; y = s[1]; z = s[2]; }
        hdr_table_read(fwd, x, y, z);
        x = lut[x];
        hdr_table_read(inv, x, y, z);
        dst[i * 3] = (uint8_t)x; dst[i * 3 + 1] = (uint8_t)y; dst[i * 3 + 2] = (uint8_t)z;
        sum += hdr_grey(x, y, z);
    }
    sum = hdr_block_sum(sum, red);
    if (threadIdx.x == 0) partial[(long)b * gridDim.x + blockIdx.x] = sum;
}

// ---- kernel B: the image's integer mean from the partials, ImageEnhance.Contrast, ImageEnhance.Color, store bytes and / or bytes / 255.0f ---------
__global__ __launch_bounds__(256) void hdr_enhance_kernel(const uint8_t* __restrict__ rgb, const unsigned* __restrict__ partial, int npartial, int H, int W,
                                                          float f_contrast, float f_color, uint8_t* __restrict__ out_u, long out_pitch, float* __restrict__ out_f) {
    __shared__ unsigned red[4];
    const int b = blockIdx.y;
    const long total = (long)H * W;
    unsigned s = 0;
    for (int i = threadIdx.x; i < npartial; i += 256) s += partial[(long)b * npartial + i];
    s = hdr_block_sum(s, red);
    const float mean = (float)(unsigned)((2ull * s + (unsigned long long)total) / (2ull * (unsigned long long)total));   // int(sum / n + 0.5)
    const uint8_t* src = rgb + (long)b * total * 3;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        unsigned x = src[i * 3], y = src[i * 3 + 1], z = src[i * 3 + 2];
        x = hdr_blend(mean, x, f_contrast); y = hdr_blend(mean, y, f_contrast); z = hdr_blend(mean, z, f_contrast);
        const float g = (float)hdr_grey(x, y, z);
        x = hdr_blend(g, x, f_color); y = hdr_blend(g, y, f_color); z = hdr_blend(g, z, f_color);
        if (out_u) {
            uint8_t* d = out_u + ((long)b * H + i / W) * out_pitch + (i % W) * 3;
            d[0] = (uint8_t)x; d[1] = (uint8_t)y; d[2] = (uint8_t)z;
        }
        if (out_f) {
            float* d = out_f + ((long)b * total + i) * 3;
            d[0] = __fdiv_rn((float)x, 255.0f); d[1] = __fdiv_rn((float)y, 255.0f); d[2] = __fdiv_rn((float)z, 255.0f);
        }
    }
}

// ---- launchers ----------------------------------------------------------------------------------------------------------------------------------
// workspace: the partial sums [B][hdr_blocks] uint32 (rounded to 256 B), then the Lab-adjusted RGB bytes [B][H][W][3]
constexpr int HDR_MAX_BLOCKS = 1024;
static int hdr_blocks(long pixels) { long g = (pixels + 255) / 256; return (int)(g > HDR_MAX_BLOCKS ? HDR_MAX_BLOCKS : g); }
static long hdr_partial_bytes(int B, long pixels) { return ((long)B * hdr_blocks(pixels) * 4 + 255) / 256 * 256; }
long hdr_workspace_bytes(int B, int H, int W) { return hdr_partial_bytes(B, (long)H * W) + (long)B * H * W * 3; }

void launch_hdr_table(const uint8_t* in, long in_pitch, uint8_t* out, long out_pitch, int H, int W, const uint16_t* table, hipStream_t s) {
    long g = ((long)H * W + 255) / 256; if (g > 16384) g = 16384;
    hipLaunchKernelGGL(hdr_table_kernel, dim3((int)g), dim3(256), 0, s, in, in_pitch, out, out_pitch, H, W, (const uint2*)table);
}
void launch_hdr_apply(const HdrArgs& a, hipStream_t s) {
    const long pixels = (long)a.H * a.W;
    const int nb = hdr_blocks(pixels);
    unsigned* partial = (unsigned*)a.workspace;
    uint8_t* rgb = (uint8_t*)a.workspace + hdr_partial_bytes(a.B, pixels);
    const dim3 grid(nb, a.B);
    if (a.in_f32)
        hipLaunchKernelGGL(hdr_lab_kernel<true>, grid, dim3(256), 0, s, a.in_f32, (const uint8_t*)nullptr, 0L, a.H, a.W, (const uint2*)a.fwd,
                           (const uint2*)a.inv, a.lut, rgb, partial);
    else
        hipLaunchKernelGGL(hdr_lab_kernel<false>, grid, dim3(256), 0, s, (const float*)nullptr, a.in_u8, a.in_pitch, a.H, a.W, (const uint2*)a.fwd,
                           (const uint2*)a.inv, a.lut, rgb, partial);
    hipLaunchKernelGGL(hdr_enhance_kernel, grid, dim3(256), 0, s, (const uint8_t*)rgb, (const unsigned*)partial, nb, a.H, a.W, a.f_contrast, a.f_color,
                       a.out_u8, a.out_pitch, a.out_f32);
}

}  // namespace ldx
