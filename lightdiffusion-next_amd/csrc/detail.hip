// fp32 canvas ops of the ADetailer path (DetailerForEach.do_detail, src/AutoDetailer/ADetailer.py:643-871): what the reference does in torch on the CPU around
// the networks of one segment, on a dense fp32 [H][W][3] device canvas.  The crop is quantised for the 8-bit LANCZOS pass of image.hip, the segment mask is
// feathered by torchvision's GaussianBlur rule and the redrawn crop is blended back through it.  Every result is the float of the numpy statement of the
// same rule (lightdiffusion-next_amd/detailer.py: blur_mask_host, paste_host): each product and each sum is rounded on its own, in the stated order.
// hipcc contracts a * b + c to an fma by default (hdr.hip met it); the pragma below takes the contract flag off every operation of this file, and the
// Makefile compiles it with -ffp-contract=off as well.  Plain C++ loops, one launch per call, linked into libldx_detail.so (csrc/Makefile says why).
#include "../../include/ldx.h"
#include "ldx_kernels.h"

#pragma clang fp contract(off)

namespace ldx {

// tensor2pil (tensor_util.py:18-40) of the rectangle (x0, y0, w, h): clamp to [0, 1], times 255.0f, truncate: the rule of image_quantize_kernel, which the
// LANCZOS pass reads.  `canvas` points at the rectangle's first float; one thread = one byte of the output.
__global__ __launch_bounds__(256) void detail_crop_quantize_kernel(const float* __restrict__ canvas, long canvas_rowlen, uint8_t* __restrict__ out,
                                                                   long out_pitch, int h, int rowlen) {
    const long total = (long)h * rowlen;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const long y = i / rowlen; const int x = (int)(i % rowlen);
        float c = canvas[y * canvas_rowlen + x];
        c = c >= 0.0f ? c : 0.0f;                           // NaN -> 0, as image_quantize_kernel
        c = c <= 1.0f ? c : 1.0f;
        out[y * out_pitch + x] = (uint8_t)(int)(c * 255.0f);
    }
}

// torch's reflect padding: no edge repeat, -1 -> 1 and n -> n - 2.  One reflection is enough: the launcher's caller refuses k / 2 >= n.
__device__ __forceinline__ int reflect(int i, int n) { return i < 0 ? -i : (i >= n ? 2 * (n - 1) - i : i); }

// torchvision's GaussianBlur (tensor_gaussian_blur_mask, tensor_util.py:218-254) as a k x k correlation over the reflect-padded mask; one thread = one
// output value, the taps in row-major order into an accumulator that starts at 0.0f.  Every lane of a wave reads the same table entry (one scalar load);
// neighbouring lanes read neighbouring mask values.
__global__ __launch_bounds__(256) void detail_blur_mask_kernel(const float* __restrict__ in, const float* __restrict__ table, float* __restrict__ out,
                                                               int h, int w, int k) {
    const long total = (long)h * w;
    const int r = k / 2;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const int y = (int)(i / w), x = (int)(i % w);
        float acc = 0.0f;
        for (int dy = 0; dy < k; ++dy) {
            const float* row = in + (long)reflect(y + dy - r, h) * w;
            const float* t = table + dy * k;
            for (int dx = 0; dx < k; ++dx) {
                const float p = t[dx] * row[reflect(x + dx - r, w)];
                acc = acc + p;
            }
        }
        out[i] = acc;
    }
}

// tensor_paste (tensor_util.py:121-151) on the clipped rectangle: canvas = (1 - m) * canvas + m * src, four rounded operations.  `canvas` points at the
// rectangle's first float; src [..][src_w][3] and mask [..][src_w] are the whole tile's, of which h rows and w columns are used; one thread = one pixel.
__global__ __launch_bounds__(256) void detail_paste_kernel(float* __restrict__ canvas, long canvas_rowlen, const float* __restrict__ src,
                                                           const float* __restrict__ mask, int src_w, int h, int w) {
    const long total = (long)h * w;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const long y = i / w; const int x = (int)(i % w);
        const float m = mask[y * src_w + x];
        const float t0 = 1.0f - m;
        float* d = canvas + y * canvas_rowlen + (long)x * 3;
        const float* s = src + (y * src_w + x) * 3;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float t1 = t0 * d[c];
            const float t2 = m * s[c];
            d[c] = t1 + t2;
        }
    }
}

// ---- launchers ---------------------------------------------------------------------------------------------------------
static int detail_grid(long n) { long g = (n + 255) / 256; if (g > 16384) g = 16384; if (g < 1) g = 1; return (int)g; }

void launch_detail_crop_quantize(const float* canvas, int W, int x0, int y0, int w, int h, uint8_t* out, long out_pitch, hipStream_t s) {
    hipLaunchKernelGGL(detail_crop_quantize_kernel, dim3(detail_grid((long)h * w * 3)), dim3(256), 0, s, canvas + ((long)y0 * W + x0) * 3, (long)W * 3, out,
                       out_pitch, h, w * 3);
}
void launch_detail_blur_mask(const float* in, int h, int w, const float* table, int k, float* out, hipStream_t s) {
    hipLaunchKernelGGL(detail_blur_mask_kernel, dim3(detail_grid((long)h * w)), dim3(256), 0, s, in, table, out, h, w, k);
}
void launch_detail_paste(float* canvas, int W, int x0, int y0, const float* src, const float* mask, int src_w, int h, int w, hipStream_t s) {
    hipLaunchKernelGGL(detail_paste_kernel, dim3(detail_grid((long)h * w)), dim3(256), 0, s, canvas + ((long)y0 * W + x0) * 3, (long)W * 3, src, mask, src_w,
                       h, w);
}

}  // namespace ldx
