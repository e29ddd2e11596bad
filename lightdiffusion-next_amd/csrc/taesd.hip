// TAESD decoder kernels (src/AutoEncoders/taesd.py:105-135, Decoder2): the latent preview of the sampler loops.  Linked into libldx_taesd.so
// (csrc/Makefile says why).  Almost all of the network is 3x3 / stride 1 / pad 1 convs with 64 channels in and out, from the latent's size up to
// 8 x that; a [64][9 * 64] 16-bit weight matrix is 72 KiB, so ONE workgroup keeps all of it in LDS for the whole launch and strides over pixel tiles.
//
// taesd_conv_kernel: a tile is TH x TW = 8 x 32 output pixels.  Its 10 x 34 input pixels (halo included; zero outside the image; nearest x2 upsampling
// folded into the gather) are staged through registers into LDS, the next tile's loads being in flight while this one is multiplied.  Wave w owns tile rows
// 2w, 2w + 1.  D[channel][pixel] = W[channel][k] * X[k][pixel] per 3x3 tap and 16-channel step with mfma 32x32x16 (weights are the A operand, so a lane
// ends up with four CONSECUTIVE channels of one pixel per register group: 8-byte stores).  LDS rows are padded by 16 bytes: weight rows 1168 B, pixel rows
// 144 B = 292 / 36 dwords, both 4 * odd, so the 16 lanes that share a ds_read_b128 cycle start on 16 different 4-bank slots.
// Epilogue: + bias, + residual row (16-bit or fp32), ReLU, 16-bit store (and the unrounded fp32 value where the skip stream goes on); OUT3 (the 64 -> 3
// output conv, its weight rows 3 .. 31 zero): + bias, then the two outputs of TAESD.decode / taesd_preview, fp32 NCHW (y - 0.5) * 2 and the 8-bit NHWC preview.
#include "../../include/ldx.h"
#include "ldx_device.h"
#include "ldx_kernels.h"

namespace ldx {

namespace {
constexpr int TW = 32, TH = 8, PW = TW + 2, PH = TH + 2;      // output tile, staged input patch
constexpr int PSTR = 64 + 8, WSTR = 9 * 64 + 8;               // LDS row strides in elements
constexpr int NPIX = PW * PH, NCHUNK = NPIX * 8;              // 16-byte chunks of a patch
constexpr int THREADS = 256, NPRE = (NCHUNK + THREADS - 1) / THREADS;
constexpr int conv_lds_bytes(int ncb) { return (ncb * 32 * WSTR + NPIX * PSTR) * 2; }
}  // namespace

// the 8-bit preview value of one decoded sample d = (y - 0.5) * 2 (taesd.py:291-304): ((d + 1) / 2) * 255, clipped to 0 .. 255, truncated; flux: d clamped to
// [-1, 1] first.  Every step is rounded on its own (no contraction), as the host's fp32 expression is.
__device__ __forceinline__ uint8_t taesd_quant(float d, int flux) {
    if (flux) { d = d >= -1.0f ? d : -1.0f; d = d <= 1.0f ? d : 1.0f; }
    float v = __fmul_rn(__fmul_rn(__fadd_rn(d, 1.0f), 0.5f), 255.0f);
    v = v >= 0.0f ? v : 0.0f;                              // NaN -> 0
    v = v <= 255.0f ? v : 255.0f;
    return (uint8_t)(int)v;
}

template <typename T, int NCB, bool OUT3>
__global__ __launch_bounds__(THREADS) void taesd_conv_kernel(const TaesdConvArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    T* const sW = (T*)smem;
    T* const sX = sW + NCB * 32 * WSTR;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 31, h = lane >> 5;
    const int Hout = a.Hin << a.up, Wout = a.Win << a.up;
    const int tiles_x = (Wout + TW - 1) / TW, tiles_y = (Hout + TH - 1) / TH, per_img = tiles_x * tiles_y;
    const long ntiles = (long)a.B * per_img;

    for (int i = tid; i < NCB * 32 * 72; i += THREADS) {
        const int row = i / 72, c = i - row * 72;
        *(uint4*)(sW + row * WSTR + c * 8) = ((const uint4*)a.W)[i];
    }

    uint4 pre[NPRE];
    auto fetch = [&](long t) {
        const int b = (int)(t / per_img), rem = (int)(t - (long)b * per_img);
        const int ty0 = rem / tiles_x * TH, tx0 = rem % tiles_x * TW;
#pragma unroll
        for (int j = 0; j < NPRE; ++j) {
            const int idx = tid + j * THREADS, p = idx >> 3, c = idx & 7;
            const int py = p / PW, px = p - py * PW;
            const int vy = ty0 + py - 1, vx = tx0 + px - 1;
            pre[j] = make_uint4(0, 0, 0, 0);
            if (idx < NCHUNK && vy >= 0 && vy < Hout && vx >= 0 && vx < Wout)
                pre[j] = *(const uint4*)((const T*)a.X + (((long)b * a.Hin + (vy >> a.up)) * a.Win + (vx >> a.up)) * 64 + c * 8);
        }
    };
    auto stash = [&]() {
#pragma unroll
        for (int j = 0; j < NPRE; ++j) {
            const int idx = tid + j * THREADS;
            if (idx < NCHUNK) *(uint4*)(sX + (idx >> 3) * PSTR + (idx & 7) * 8) = pre[j];
        }
    };

    // this lane's channels: cb * 32 + 8 g + 4 h + (0 .. 3)
    float4 bias[NCB][4];
#pragma unroll
    for (int cb = 0; cb < NCB; ++cb)
#pragma unroll
        for (int g = 0; g < 4; ++g) bias[cb][g] = (a.bias && !OUT3) ? *(const float4*)(a.bias + cb * 32 + 8 * g + 4 * h) : make_float4(0.f, 0.f, 0.f, 0.f);

    long t = blockIdx.x;
    if (t < ntiles) fetch(t);
    for (; t < ntiles; t += gridDim.x) {
        __syncthreads();                       // the previous tile's reads of sX are done
        stash();
        __syncthreads();
        if (t + gridDim.x < ntiles) fetch(t + gridDim.x);

        f32x16 acc[2][NCB];
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int cb = 0; cb < NCB; ++cb)
#pragma unroll
                for (int q = 0; q < 16; ++q) acc[i][cb][q] = 0.f;
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) {
            const int dy = tap / 3, dx = tap % 3;
#pragma unroll
            for (int kk = 0; kk < 4; ++kk) {
                const int c0 = kk * 16 + 8 * h;
                typename Vec<T>::v8 xf[2], wf[NCB];
#pragma unroll
                for (int i = 0; i < 2; ++i) xf[i] = *(const typename Vec<T>::v8*)(sX + ((2 * wave + i + dy) * PW + r + dx) * PSTR + c0);
#pragma unroll
                for (int cb = 0; cb < NCB; ++cb) wf[cb] = *(const typename Vec<T>::v8*)(sW + (cb * 32 + r) * WSTR + tap * 64 + c0);
#pragma unroll
                for (int i = 0; i < 2; ++i)
#pragma unroll
                    for (int cb = 0; cb < NCB; ++cb) acc[i][cb] = mfma32(wf[cb], xf[i], acc[i][cb]);
            }
        }

        const int b = (int)(t / per_img), rem = (int)(t - (long)b * per_img);
        const int x = rem % tiles_x * TW + r;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int y = rem / tiles_x * TH + 2 * wave + i;
            if (y >= Hout || x >= Wout) continue;
            const long m = ((long)b * Hout + y) * Wout + x;
            if constexpr (OUT3) {
                if (h) continue;                    // channels 0 .. 2 are registers 0 .. 2 of the lower lane half
                const long hw = (long)Hout * Wout, pix = (long)y * Wout + x;
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const float v = acc[i][0][c] + (a.bias ? a.bias[c] : 0.f);
                    const float d = __fmul_rn(__fsub_rn(v, 0.5f), 2.0f);
                    if (a.out_f32) a.out_f32[((long)b * 3 + c) * hw + pix] = d;
                    if (a.out_u8) a.out_u8[m * 3 + (a.flux ? 2 - c : c)] = taesd_quant(d, a.flux);
                }
            } else {
#pragma unroll
                for (int cb = 0; cb < NCB; ++cb)
#pragma unroll
                    for (int g = 0; g < 4; ++g) {
                        const int ch = cb * 32 + 8 * g + 4 * h;
                        float v[4] = {acc[i][cb][4 * g] + bias[cb][g].x, acc[i][cb][4 * g + 1] + bias[cb][g].y,
                                      acc[i][cb][4 * g + 2] + bias[cb][g].z, acc[i][cb][4 * g + 3] + bias[cb][g].w};
                        if (a.Rf) {
                            const float4 rf = *(const float4*)(a.Rf + m * 64 + ch);
                            v[0] += rf.x; v[1] += rf.y; v[2] += rf.z; v[3] += rf.w;
                        } else if (a.R) {
                            float rv[4];
                            unpack4<T>(*(const uint2*)((const T*)a.R + m * 64 + ch), rv);
#pragma unroll
                            for (int e = 0; e < 4; ++e) v[e] += rv[e];
                        }
                        if (a.relu) {
#pragma unroll
                            for (int e = 0; e < 4; ++e) v[e] = fmaxf(v[e], 0.f);
                        }
                        *(uint2*)((T*)a.Y + m * 64 + ch) = pack4<T>(v[0], v[1], v[2], v[3]);
                        if (a.Yf) *(float4*)(a.Yf + m * 64 + ch) = make_float4(v[0], v[1], v[2], v[3]);
                    }
            }
        }
    }
}

// Clamp (taesd.py:30-42: tanh(x / 3) * 3) and fp32 NCHW [B][C][HW] -> 16-bit rows [B * HW][64], channels C .. 63 zero.  One thread per pixel.
template <typename T>
__global__ __launch_bounds__(256) void taesd_prep_kernel(const float* __restrict__ z, T* __restrict__ out, int B, int C, long HW) {
    const long total = (long)B * HW;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const long b = i / HW, p = i - b * HW;
        float f[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        for (int c = 0; c < C && c < 8; ++c) f[c] = tanhf(z[(b * C + c) * HW + p] / 3.0f) * 3.0f;
        uint4* dst = (uint4*)(out + i * 64);
        dst[0] = pack8<T>(f);
#pragma unroll
        for (int k = 1; k < 8; ++k) dst[k] = make_uint4(0, 0, 0, 0);
    }
}

static unsigned conv_grid(const TaesdConvArgs& a) {
    static int cus[64] = {0};
    int dev = 0;
    (void)hipGetDevice(&dev);
    dev &= 63;
    if (!cus[dev]) { int n = 0; (void)hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev); cus[dev] = n > 0 ? n : 256; }
    const long Hout = (long)a.Hin << a.up, Wout = (long)a.Win << a.up;
    const long ntiles = (long)a.B * ((Wout + TW - 1) / TW) * ((Hout + TH - 1) / TH);
    return (unsigned)(ntiles < cus[dev] ? ntiles : cus[dev]);      // one workgroup per CU (its LDS holds one), each striding over the tiles
}

template <typename T, int NCB, bool OUT3> static void launch_conv_t(const TaesdConvArgs& a, hipStream_t s) {
    static DevOnce once;
    constexpr int lds = conv_lds_bytes(NCB);
    set_dyn_lds(once, (const void*)taesd_conv_kernel<T, NCB, OUT3>, lds);
    hipLaunchKernelGGL((taesd_conv_kernel<T, NCB, OUT3>), dim3(conv_grid(a)), dim3(THREADS), lds, s, a);
}

bool taesd_conv_ok(const TaesdConvArgs& a) {
    const long Hout = (long)a.Hin << a.up, Wout = (long)a.Win << a.up;
    return a.X && a.W && a.B > 0 && a.Hin > 0 && a.Win > 0 && (a.up == 0 || a.up == 1) && (long)a.B * Hout * Wout < (1L << 31) &&
           (a.out3 ? (a.out_f32 || a.out_u8) && !a.R && !a.Rf && !a.Y && !a.Yf : a.Y != nullptr && !(a.R && a.Rf));
}

void launch_taesd_conv(const TaesdConvArgs& a, DType dt, hipStream_t s) {
    if (!taesd_conv_ok(a)) return;
    if (a.out3) { if (dt == DT_BF16) launch_conv_t<__bf16, 1, true>(a, s); else launch_conv_t<_Float16, 1, true>(a, s); }
    else if (dt == DT_BF16) launch_conv_t<__bf16, 2, false>(a, s);
    else launch_conv_t<_Float16, 2, false>(a, s);
}

void launch_taesd_prep(const TaesdPrepArgs& a, DType dt, hipStream_t s) {
    const long total = (long)a.B * a.HW;
    if (total <= 0 || !a.z || !a.out) return;
    const unsigned grid = (unsigned)((total + 255) / 256 < 4096 ? (total + 255) / 256 : 4096);
    if (dt == DT_BF16) hipLaunchKernelGGL(taesd_prep_kernel<__bf16>, dim3(grid), dim3(256), 0, s, a.z, (__bf16*)a.out, a.B, a.C, a.HW);
    else hipLaunchKernelGGL(taesd_prep_kernel<_Float16>, dim3(grid), dim3(256), 0, s, a.z, (_Float16*)a.out, a.B, a.C, a.HW);
}

}  // namespace ldx
