// 8-bit image ops of the img2img path (Ultimate SD Upscale, src/UltimateSDUpscale/UltimateSDUpscale.py:126-245): what the reference does in PIL between the
// networks, on HWC uint8 device images with a row pitch.  Everything after the float -> byte step is integer arithmetic in Pillow, so any summation order
// gives Pillow's bytes; the kernels are plain C++ loops, one launch per pass, linked into libldx_image.so (csrc/Makefile says why).
#include "../../include/ldx.h"
#include "ldx_kernels.h"

namespace ldx {

// ---- a / b: fp32 <-> uint8 -------------------------------------------------------------------------------------------
// tensor_to_pil (image_util.py:133-178): clamp to [0, 1], times 255.0f, truncate.  V consecutive elements of one row per thread.
template <int V>
__global__ __launch_bounds__(256) void image_quantize_kernel(const float* __restrict__ in, uint8_t* __restrict__ out, int H, int rowlen, long out_pitch) {
    const int per_row = rowlen / V;
    const long total = (long)H * per_row;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const long y = i / per_row; const int x = (int)(i % per_row) * V;
        const float* src = in + y * rowlen + x;
        uint8_t* dst = out + y * out_pitch + x;
        float v[V];
        if (V == 4) { const float4 f = *(const float4*)src; v[0] = f.x; v[1] = f.y; v[2] = f.z; v[3] = f.w; }
        else v[0] = src[0];
        uint8_t b[V];
#pragma unroll
        for (int k = 0; k < V; ++k) {
            float c = v[k];
            c = c >= 0.0f ? c : 0.0f;                       // NaN -> 0, as the cast of a clamped NaN is undefined in numpy anyway
            c = c <= 1.0f ? c : 1.0f;
            b[k] = (uint8_t)(int)(c * 255.0f);
        }
        if (V == 4) *(uchar4*)dst = make_uchar4(b[0], b[1], b[2], b[3]);
        else dst[0] = b[0];
    }
}

// pil_to_tensor (image_util.py:181-203): v / 255.0f, the correctly rounded IEEE quotient (__fdiv_rn is never turned into a reciprocal multiply).
template <int V>
__global__ __launch_bounds__(256) void image_to_float_kernel(const uint8_t* __restrict__ in, long in_pitch, float* __restrict__ out, int H, int rowlen) {
    const int per_row = rowlen / V;
    const long total = (long)H * per_row;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const long y = i / per_row; const int x = (int)(i % per_row) * V;
        const uint8_t* src = in + y * in_pitch + x;
        float* dst = out + y * rowlen + x;
        float v[V];
#pragma unroll
        for (int k = 0; k < V; ++k) v[k] = __fdiv_rn((float)src[k], 255.0f);
        if (V == 4) *(float4*)dst = make_float4(v[0], v[1], v[2], v[3]);
        else dst[0] = v[0];
    }
}

// ---- c: one pass of Pillow's 8-bit ImagingResample --------------------------------------------------------------------
// clip8(acc >> 22), with the clamp in front of the shift.  Written as shift-then-clamp, hipcc (ROCm 7) packs pairs of results with gfx950's
// v_ashr_pk_u8_i32, which keeps the upper half of its destination register where the compiler assumes zeros: on the MI355X byte 2 of a packed word
// came out OR-ed with stale bits (tests/test_image_ops_gpu.py, the resize cases, catch it).
__device__ __forceinline__ uint8_t clip8(int acc) {
    acc = acc < 0 ? 0 : acc;
    acc = acc > (256 << 22) - 1 ? (256 << 22) - 1 : acc;
    return (uint8_t)(acc >> 22);
}

// along the row: one thread = one output pixel (its C bytes); taps of neighbouring threads overlap, so the reads stay in L1 / L2
template <int C>
__global__ __launch_bounds__(256) void image_resample_h_kernel(const uint8_t* __restrict__ in, long in_pitch, uint8_t* __restrict__ out, long out_pitch,
                                                               int H, int W, int new_w, const int* __restrict__ bounds, const int* __restrict__ kk, int ksize) {
    const long total = (long)H * new_w;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const long y = i / new_w; const int xx = (int)(i % new_w);
        int x0 = bounds[2 * xx], n = bounds[2 * xx + 1];
        x0 = x0 < 0 ? 0 : (x0 > W ? W : x0);                 // a wrong table reads a wrong pixel, never outside the row
        n = n > ksize ? ksize : n; n = n > W - x0 ? W - x0 : n;
        const int* k = kk + (long)xx * ksize;
        const uint8_t* src = in + y * in_pitch + (long)x0 * C;
        int acc[C];
#pragma unroll
        for (int c = 0; c < C; ++c) acc[c] = 1 << 21;
        for (int j = 0; j < n; ++j) {
            const int w = k[j];
#pragma unroll
            for (int c = 0; c < C; ++c) acc[c] += w * (int)src[j * C + c];
        }
        uint8_t* dst = out + y * out_pitch + (long)xx * C;
#pragma unroll
        for (int c = 0; c < C; ++c) dst[c] = clip8(acc[c]);
    }
}

// down the column: the channels do not matter, a row is W * C bytes; one thread = V consecutive bytes of an output row, so each tap is one V-byte load
template <int V>
__global__ __launch_bounds__(256) void image_resample_v_kernel(const uint8_t* __restrict__ in, long in_pitch, uint8_t* __restrict__ out, long out_pitch,
                                                               int H, int rowlen, int new_h, const int* __restrict__ bounds, const int* __restrict__ kk, int ksize) {
    const int per_row = (rowlen + V - 1) / V;
    const long total = (long)new_h * per_row;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const int yy = (int)(i / per_row); const int x = (int)(i % per_row) * V;
        int y0 = bounds[2 * yy], n = bounds[2 * yy + 1];
        y0 = y0 < 0 ? 0 : (y0 > H ? H : y0);
        n = n > ksize ? ksize : n; n = n > H - y0 ? H - y0 : n;
        const int* k = kk + (long)yy * ksize;
        const uint8_t* src = in + (long)y0 * in_pitch + x;
        uint8_t* dst = out + (long)yy * out_pitch + x;
        if (V == 16 && x + 16 <= rowlen) {
            int acc[16];
#pragma unroll
            for (int b = 0; b < 16; ++b) acc[b] = 1 << 21;
            for (int j = 0; j < n; ++j) {
                const int w = k[j];
                const uint4 q = *(const uint4*)(src + (long)j * in_pitch);
                const unsigned qq[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
                for (int b = 0; b < 16; ++b) acc[b] += w * (int)((qq[b >> 2] >> (8 * (b & 3))) & 0xffu);
            }
            unsigned r[4] = {0, 0, 0, 0};
#pragma unroll
            for (int b = 0; b < 16; ++b) r[b >> 2] |= (unsigned)clip8(acc[b]) << (8 * (b & 3));
            *(uint4*)dst = make_uint4(r[0], r[1], r[2], r[3]);
        } else {
            const int m = rowlen - x < V ? rowlen - x : V;   // the row's tail (V = 16) or the single byte (V = 1)
            for (int b = 0; b < m; ++b) {
                int acc = 1 << 21;
                for (int j = 0; j < n; ++j) acc += k[j] * (int)src[(long)j * in_pitch + b];
                dst[b] = clip8(acc);
            }
        }
    }
}

// ---- d: one pass of Pillow's box blur on a single-channel image (BoxBlur.c; GaussianBlur = 3 passes along x, then 3 along y) -------------------
struct BoxParams { int R; unsigned ww, fw; };
__device__ __forceinline__ uint8_t box_out(const BoxParams& p, unsigned sum, unsigned edges) {
    return (uint8_t)((p.ww * sum + p.fw * edges + (1u << 23)) >> 24);
}
__device__ __forceinline__ int clampi(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

// along the row: a block stages 256 outputs' worth of the row plus R + 1 bytes on either side (edge replicated) in LDS; one thread = one windowed sum
constexpr int BOX_TILE = 256, BOX_MAX_R = 255;
__global__ __launch_bounds__(256) void image_box_h_kernel(const uint8_t* __restrict__ in, long in_pitch, uint8_t* __restrict__ out, long out_pitch,
                                                          int W, BoxParams p) {
    __shared__ uint8_t line[BOX_TILE + 2 * (BOX_MAX_R + 1)];
    const int y = blockIdx.y, x0 = blockIdx.x * BOX_TILE, halo = p.R + 1;
    const uint8_t* src = in + (long)y * in_pitch;
    for (int i = threadIdx.x; i < BOX_TILE + 2 * halo; i += 256) line[i] = src[clampi(x0 - halo + i, W - 1)];
    __syncthreads();
    const int x = x0 + threadIdx.x;
    if (x >= W) return;
    const uint8_t* w = line + threadIdx.x;                   // w[0] = in[x - R - 1], w[2R + 2] = in[x + R + 1]
    unsigned sum = 0;
    for (int i = 1; i <= 2 * p.R + 1; ++i) sum += w[i];
    out[(long)y * out_pitch + x] = box_out(p, sum, (unsigned)w[0] + w[2 * p.R + 2]);
}

// down the column: one thread = one column of a band of BOX_BAND output rows; the window slides (exact: integers), lanes read consecutive bytes of a row
constexpr int BOX_BAND = 32;
__global__ __launch_bounds__(256) void image_box_v_kernel(const uint8_t* __restrict__ in, long in_pitch, uint8_t* __restrict__ out, long out_pitch,
                                                          int H, int W, BoxParams p) {
    const int x = blockIdx.x * 256 + threadIdx.x;
    if (x >= W) return;
    const int y0 = blockIdx.y * BOX_BAND, y1 = y0 + BOX_BAND < H ? y0 + BOX_BAND : H;
    const uint8_t* src = in + x;
    unsigned sum = 0;
    for (int i = -p.R; i <= p.R; ++i) sum += src[(long)clampi(y0 + i, H - 1) * in_pitch];
    for (int y = y0; y < y1; ++y) {
        const unsigned lo = src[(long)clampi(y - p.R - 1, H - 1) * in_pitch], hi = src[(long)clampi(y + p.R + 1, H - 1) * in_pitch];
        out[(long)y * out_pitch + x] = box_out(p, sum, lo + hi);
        sum += hi;
        sum -= src[(long)clampi(y - p.R, H - 1) * in_pitch];
    }
}

// ---- e: paste + alpha_composite over an opaque canvas (UltimateSDUpscale.py:224-242; Pillow's AlphaComposite.c with destination alpha 255) ------
template <int C>
__global__ __launch_bounds__(256) void image_composite_kernel(uint8_t* __restrict__ canvas, long canvas_pitch, const uint8_t* __restrict__ tile, long tile_pitch,
                                                              const uint8_t* __restrict__ mask, long mask_pitch, int h, int w) {
    const long total = (long)h * w;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const long y = i / w; const int x = (int)(i % w);
        const unsigned a = mask[y * mask_pitch + x];
        if (a == 0) continue;
        const unsigned coef1 = a * 255u * 255u * 128u / (a * 255u + 255u * (255u - a)), coef2 = 255u * 128u - coef1;
        uint8_t* d = canvas + y * canvas_pitch + (long)x * C;
        const uint8_t* s = tile + y * tile_pitch + (long)x * C;
#pragma unroll
        for (int c = 0; c < C; ++c) {
            const unsigned t = s[c] * coef1 + d[c] * coef2 + (0x80u << 7);
            d[c] = (uint8_t)((((t >> 8) + t) >> 8) >> 7);
        }
    }
}

__global__ __launch_bounds__(256) void image_fill_kernel(uint8_t* __restrict__ img, long pitch, int h, int rowlen, int value) {
    const long total = (long)h * rowlen;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) img[(i / rowlen) * pitch + i % rowlen] = (uint8_t)value;
}

// ---- launchers ---------------------------------------------------------------------------------------------------------
static int image_grid(long n) { long g = (n + 255) / 256; if (g > 16384) g = 16384; if (g < 1) g = 1; return (int)g; }
static bool aligned(const void* p, long pitch, int a) { return (uintptr_t)p % a == 0 && pitch % a == 0; }

void launch_image_quantize(const float* in, uint8_t* out, int H, int W, int C, long out_pitch, hipStream_t s) {
    const int rowlen = W * C;
    if (rowlen % 4 == 0 && aligned(in, 0, 16) && aligned(out, out_pitch, 4))
        hipLaunchKernelGGL(image_quantize_kernel<4>, dim3(image_grid((long)H * rowlen / 4)), dim3(256), 0, s, in, out, H, rowlen, out_pitch);
    else
        hipLaunchKernelGGL(image_quantize_kernel<1>, dim3(image_grid((long)H * rowlen)), dim3(256), 0, s, in, out, H, rowlen, out_pitch);
}
void launch_image_to_float(const uint8_t* in, long in_pitch, float* out, int H, int W, int C, hipStream_t s) {
    const int rowlen = W * C;
    if (rowlen % 4 == 0 && aligned(out, 0, 16))
        hipLaunchKernelGGL(image_to_float_kernel<4>, dim3(image_grid((long)H * rowlen / 4)), dim3(256), 0, s, in, in_pitch, out, H, rowlen);
    else
        hipLaunchKernelGGL(image_to_float_kernel<1>, dim3(image_grid((long)H * rowlen)), dim3(256), 0, s, in, in_pitch, out, H, rowlen);
}
void launch_image_resample_pass(const uint8_t* in, long in_pitch, uint8_t* out, long out_pitch, int H, int W, int C, int axis, int new_len,
                                const int* bounds, const int* kk, int ksize, hipStream_t s) {
    if (axis == 1) {
        const dim3 g(image_grid((long)H * new_len));
        if (C == 3) hipLaunchKernelGGL(image_resample_h_kernel<3>, g, dim3(256), 0, s, in, in_pitch, out, out_pitch, H, W, new_len, bounds, kk, ksize);
        else hipLaunchKernelGGL(image_resample_h_kernel<1>, g, dim3(256), 0, s, in, in_pitch, out, out_pitch, H, W, new_len, bounds, kk, ksize);
        return;
    }
    const int rowlen = W * C;
    if (aligned(in, in_pitch, 16) && aligned(out, out_pitch, 16))
        hipLaunchKernelGGL(image_resample_v_kernel<16>, dim3(image_grid((long)new_len * ((rowlen + 15) / 16))), dim3(256), 0, s, in, in_pitch, out, out_pitch,
                           H, rowlen, new_len, bounds, kk, ksize);
    else
        hipLaunchKernelGGL(image_resample_v_kernel<1>, dim3(image_grid((long)new_len * rowlen)), dim3(256), 0, s, in, in_pitch, out, out_pitch,
                           H, rowlen, new_len, bounds, kk, ksize);
}
int image_box_max_radius() { return BOX_MAX_R; }
void launch_image_box_blur_pass(const uint8_t* in, long in_pitch, uint8_t* out, long out_pitch, int H, int W, int axis, float radius, hipStream_t s) {
    // BoxBlur.c ImagingLineBoxBlur8: float32 arithmetic for the weights, as Pillow's
    BoxParams p;
    p.R = (int)radius;
    p.ww = (unsigned)(16777216.0f / (radius * 2 + 1));
    p.fw = ((1u << 24) - (unsigned)(p.R * 2 + 1) * p.ww) / 2;
    if (axis == 1) hipLaunchKernelGGL(image_box_h_kernel, dim3((W + BOX_TILE - 1) / BOX_TILE, H), dim3(256), 0, s, in, in_pitch, out, out_pitch, W, p);
    else hipLaunchKernelGGL(image_box_v_kernel, dim3((W + 255) / 256, (H + BOX_BAND - 1) / BOX_BAND), dim3(256), 0, s, in, in_pitch, out, out_pitch, H, W, p);
}
void launch_image_composite(uint8_t* canvas, long canvas_pitch, const uint8_t* tile, long tile_pitch, const uint8_t* mask, long mask_pitch,
                            int h, int w, int C, hipStream_t s) {
    const dim3 g(image_grid((long)h * w));
    if (C == 3) hipLaunchKernelGGL(image_composite_kernel<3>, g, dim3(256), 0, s, canvas, canvas_pitch, tile, tile_pitch, mask, mask_pitch, h, w);
    else hipLaunchKernelGGL(image_composite_kernel<1>, g, dim3(256), 0, s, canvas, canvas_pitch, tile, tile_pitch, mask, mask_pitch, h, w);
}
void launch_image_fill(uint8_t* img, long pitch, int h, int rowlen, int value, hipStream_t s) {
    hipLaunchKernelGGL(image_fill_kernel, dim3(image_grid((long)h * rowlen)), dim3(256), 0, s, img, pitch, h, rowlen, value);
}

}  // namespace ldx
