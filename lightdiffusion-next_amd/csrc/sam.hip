// SAM image encoder kernels (segment_anything's ImageEncoderViT, the network behind ADetailer's masks): everything the encoder needs that the shared GEMM,
// LayerNorm and conv kernels do not do.  Linked into libldx_sam.so (csrc/Makefile says why).  Head dimension 64, patch size 16.
//
//   sam_patch_kernel       fp32 NCHW image -> 16-bit patch rows in the K order of patch_embed.proj.weight (the patch embedding is then a plain GEMM)
//   sam_window_kernel      window partition (zero rows for the padding) and its inverse with the crop and the residual add
//   sam_relpos_kernel      the decomposed relative-position terms rel_h | rel_w of every query, fp32
//   sam_attn_kernel        flash attention for D = 64 whose score bias is rel_h[q][k / n] + rel_w[q][k % n], added inside the kernel
//   sam_rowvec_kernel      bias + erf-GELU in place (the MLP), + pos_embed in place
//   sam_out_kernel         16-bit rows -> the fp32 NCHW result
//   sam_preprocess_kernel  Sam.preprocess of an 8-bit image, float for float (IEEE subtraction and division, nothing contracted)
//
// sam_attn_kernel: a workgroup of four waves owns 64 queries of one (window, head), a wave 16 of them; 64 keys at a time are staged in LDS, K row-major and V
// transposed.  S^T = K Q^T runs on mfma 16x16x32 with the keys as rows, so a lane holds scores of ONE query (column l & 15) and the softmax state is a scalar
// per lane, shared by the four lanes l, l ^ 16, l ^ 32, l ^ 48.  The probabilities stay in registers: the MFMA's k index of O^T = V^T P^T is mapped onto the
// keys a lane already holds (two 16-key tiles, four keys of each per lane), and the V^T fragment is read from LDS in that same order.  Keys at and above N
// are staged as zero rows and their scores are -inf: they enter neither the maximum nor the sum.
#include "../../include/ldx.h"
#include "ldx_device.h"
#include "ldx_kernels.h"

#pragma clang fp contract(off)

namespace ldx {

namespace {
constexpr int AQ = 64, AK = 64;               // queries per workgroup, keys per step
constexpr int KSTR = 64 + 8, VSTR = AK + 8;   // LDS row strides in elements: 144 bytes = 36 dwords, 4 * odd
}  // namespace

template <typename T>
__global__ __launch_bounds__(256) void sam_patch_kernel(const float* __restrict__ img, T* __restrict__ out, int B, int S) {
    const long total = (long)B * S * S * 96;             // 16-byte chunks: 768 / 8 per patch
    const long side = 16L * S;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const long row = i / 96; const int ch = (int)(i - row * 96);
        const int c = ch >> 5, ky = (ch >> 1) & 15, kx = (ch & 1) * 8;
        const long b = row / ((long)S * S); const int p = (int)(row - b * S * S), py = p / S, px = p - py * S;
        const float* src = img + ((b * 3 + c) * side + (py * 16 + ky)) * side + px * 16 + kx;
        const float4 lo = *(const float4*)src, hi = *(const float4*)(src + 4);
        const float f[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
        *(uint4*)(out + row * 768 + ch * 8) = pack8<T>(f);
    }
}

template <typename T>
__global__ __launch_bounds__(256) void sam_window_kernel(const SamWindowArgs a) {
    const int nw = (a.S + a.win - 1) / a.win, c8 = a.C / 8, ww = a.win * a.win;
    if (!a.scatter) {
        const long total = (long)a.B * nw * nw * ww * c8;
        for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
            const long row = i / c8; const int c = (int)(i - row * c8);
            const long wi = row / ww; const int in = (int)(row - wi * ww), iy = in / a.win, ix = in - iy * a.win;
            const long b = wi / (nw * nw); const int wr = (int)(wi - b * nw * nw), wy = wr / nw, wx = wr - wy * nw;
            const int y = wy * a.win + iy, x = wx * a.win + ix;
            uint4 v = make_uint4(0, 0, 0, 0);
            if (y < a.S && x < a.S) v = *(const uint4*)((const T*)a.src + ((b * a.S + y) * a.S + x) * a.C + c * 8);
            *(uint4*)((T*)a.dst + row * a.C + c * 8) = v;
        }
    } else {
        const long total = (long)a.B * a.S * a.S * c8;
        for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
            const long row = i / c8; const int c = (int)(i - row * c8);
            const long b = row / ((long)a.S * a.S); const int p = (int)(row - b * a.S * a.S), y = p / a.S, x = p - y * a.S;
            const int wy = y / a.win, iy = y - wy * a.win, wx = x / a.win, ix = x - wx * a.win;
            const long wrow = ((b * nw + wy) * nw + wx) * ww + iy * a.win + ix;
            uint4 v = *(const uint4*)((const T*)a.src + wrow * a.C + c * 8);
            if (a.R) {
                float f[8], r[8];
                unpack8<T>(v, f);
                unpack8<T>(*(const uint4*)((const T*)a.R + row * a.C + c * 8), r);
#pragma unroll
                for (int e = 0; e < 8; ++e) f[e] = r[e] + f[e];
                v = pack8<T>(f);
            }
            *(uint4*)((T*)a.dst + row * a.C + c * 8) = v;
        }
    }
}

template <typename T>
__global__ __launch_bounds__(256) void sam_relpos_kernel(const SamRelposArgs a) {
    const int n = a.n, N = n * n, n2 = 2 * n;
    const long total = (long)a.BW * a.H * N * n2;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const long rq = i / n2; const int jj = (int)(i - rq * n2);
        const long bh = rq / N; const int q = (int)(rq - bh * N);
        const long bw = bh / a.H; const int h = (int)(bh - bw * a.H);
        const int qh = q / n, qw = q - qh * n;
        const float* tp = jj < n ? a.th + (long)(qh - jj + n - 1) * 64 : a.tw + (long)(qw - (jj - n) + n - 1) * 64;
        const T* qp = (const T*)a.Q + (bw * N + q) * a.ldq + h * 64;
        float acc = 0.f;
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            float f[8];
            unpack8<T>(*(const uint4*)(qp + c * 8), f);
            const float4 t0 = *(const float4*)(tp + c * 8), t1 = *(const float4*)(tp + c * 8 + 4);
            acc = fmaf(f[0], t0.x, acc); acc = fmaf(f[1], t0.y, acc); acc = fmaf(f[2], t0.z, acc); acc = fmaf(f[3], t0.w, acc);
            acc = fmaf(f[4], t1.x, acc); acc = fmaf(f[5], t1.y, acc); acc = fmaf(f[6], t1.z, acc); acc = fmaf(f[7], t1.w, acc);
        }
        a.out[i] = acc;
    }
}

template <typename T>
__global__ __launch_bounds__(256) void sam_attn_kernel(const SamAttnArgs a) {
    __shared__ __attribute__((aligned(16))) T sK[AK * KSTR];
    __shared__ __attribute__((aligned(16))) T sVt[64 * VSTR];
    using v8 = typename Vec<T>::v8;
    using v4 = typename Vec<T>::v4;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, j = lane & 15, g = lane >> 4;
    const int n = a.n, N = n * n;
    const int bh = blockIdx.y, bw = bh / a.H, h = bh - bw * a.H;
    const int q = blockIdx.x * AQ + wave * 16 + j, qc = q < N ? q : N - 1;          // a query past N computes on the last one's data and stores nothing
    const long base = (long)bw * N;
    const T* const Qp = (const T*)a.Q + (base + qc) * a.ld + h * 64;
    const v8 qf[2] = {*(const v8*)(Qp + 8 * g), *(const v8*)(Qp + 32 + 8 * g)};
    const float* const relq = a.rel + ((long)bh * N + qc) * (2 * n);

    float m = -INFINITY, lsum = 0.f;
    f32x4 o[4];
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) o[dt] = (f32x4){0.f, 0.f, 0.f, 0.f};

    for (int kb = 0; kb < N; kb += AK) {
        __syncthreads();                                   // the previous step's reads of sK / sVt are done
#pragma unroll
        for (int it = 0; it < 2; ++it) {
            const int idx = tid + it * 256, key = idx >> 3, c = idx & 7, kg = kb + key;
            uint4 kv = make_uint4(0, 0, 0, 0), vv = make_uint4(0, 0, 0, 0);
            if (kg < N) {
                const long off = (base + kg) * a.ld + h * 64 + c * 8;
                kv = *(const uint4*)((const T*)a.K + off);
                vv = *(const uint4*)((const T*)a.V + off);
            }
            *(uint4*)(sK + key * KSTR + c * 8) = kv;
            const v8 ve = as_v8<T>(vv);
#pragma unroll
            for (int e = 0; e < 8; ++e) sVt[(c * 8 + e) * VSTR + key] = ve[e];
        }
        __syncthreads();

        // S^T tile t: keys kb + 16 t + 4 g + r (rows), query j (column)
        f32x4 s[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            s[t] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int kk = 0; kk < 2; ++kk) s[t] = mfma16(*(const v8*)(sK + (16 * t + j) * KSTR + kk * 32 + 8 * g), qf[kk], s[t]);
        }
        float mloc = -INFINITY;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int k0 = kb + 16 * t + 4 * g;
            int kh = k0 / n, kw = k0 - kh * n;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                float v = -INFINITY;
                if (k0 + r < N) v = s[t][r] * a.scale + (relq[kh] + relq[n + kw]);
                s[t][r] = v;
                mloc = fmaxf(mloc, v);
                if (++kw == n) { kw = 0; ++kh; }
            }
        }
        mloc = quad_max(mloc);                             // over the four lanes of query j: block 0 holds key 0, so the maximum is finite from the first step on
        const float mnew = fmaxf(m, mloc), alpha = __expf(m - mnew);
        m = mnew;
        lsum *= alpha;
#pragma unroll
        for (int dt = 0; dt < 4; ++dt)
#pragma unroll
            for (int r = 0; r < 4; ++r) o[dt][r] *= alpha;
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) { const float p = __expf(s[t][r] - mnew); s[t][r] = p; lsum += p; }

        // O^T += V^T P^T, 32 keys per MFMA: its k index 8 g + e is key 16 t0 + 4 g + e (e < 4), 16 t1 + 4 g + e - 4 (e >= 4)
#pragma unroll
        for (int pr = 0; pr < 2; ++pr) {
            const int t0 = 2 * pr, t1 = 2 * pr + 1;
            v8 pb;
#pragma unroll
            for (int r = 0; r < 4; ++r) { pb[r] = (T)s[t0][r]; pb[4 + r] = (T)s[t1][r]; }
#pragma unroll
            for (int dt = 0; dt < 4; ++dt) {
                const T* vrow = sVt + (16 * dt + j) * VSTR + 4 * g;
                const v4 lo = *(const v4*)(vrow + 16 * t0), hi = *(const v4*)(vrow + 16 * t1);
                v8 vf;
#pragma unroll
                for (int r = 0; r < 4; ++r) { vf[r] = lo[r]; vf[4 + r] = hi[r]; }
                o[dt] = mfma16(vf, pb, o[dt]);
            }
        }
    }
    lsum = quad_sum(lsum);
    const float inv = 1.0f / lsum;
    if (q < N) {
        T* const Op = (T*)a.O + (base + q) * a.ldo + h * 64 + 4 * g;          // o[dt][r] = O[q][16 dt + 4 g + r]
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) *(uint2*)(Op + 16 * dt) = pack4<T>(o[dt][0] * inv, o[dt][1] * inv, o[dt][2] * inv, o[dt][3] * inv);
    }
}

template <typename T>
__global__ __launch_bounds__(256) void sam_rowvec_kernel(const SamRowvecArgs a) {
    const int c8 = a.C / 8;
    const long total = a.rows * c8;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const long row = i / c8; const int c = (int)(i - row * c8) * 8;
        T* const p = (T*)a.X + row * a.ld + c;
        const float* const vp = a.vec + (row % a.period) * a.C + c;
        float f[8];
        unpack8<T>(*(const uint4*)p, f);
        const float4 v0 = *(const float4*)vp, v1 = *(const float4*)(vp + 4);
        const float v[8] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w};
#pragma unroll
        for (int e = 0; e < 8; ++e) { f[e] = f[e] + v[e]; if (a.act) f[e] = gelu_erf_f(f[e]); }
        *(uint4*)p = pack8<T>(f);
    }
}

template <typename T>
__global__ __launch_bounds__(256) void sam_out_kernel(const T* __restrict__ X, int ld, float* __restrict__ out, int B, int C, int HW) {
    const long total = (long)B * C * HW;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const long bc = i / HW; const int p = (int)(i - bc * HW);
        const long b = bc / C; const int c = (int)(bc - b * C);
        out[i] = (float)X[(b * HW + p) * ld + c];
    }
}

__global__ __launch_bounds__(256) void sam_preprocess_kernel(const uint8_t* __restrict__ in, long pitch, int h, int w, float* __restrict__ out, int size) {
    const long plane = (long)size * size, total = 3 * plane;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const int c = (int)(i / plane); const long r = i - c * plane;
        const int y = (int)(r / size), x = (int)(r - (long)y * size);
        const float mean = c == 0 ? 123.675f : c == 1 ? 116.28f : 103.53f, sd = c == 0 ? 58.395f : c == 1 ? 57.12f : 57.375f;
        float v = 0.0f;
        if (y < h && x < w) v = __fdiv_rn(__fsub_rn((float)in[y * pitch + (long)x * 3 + c], mean), sd);
        out[i] = v;
    }
}

static unsigned flat_grid(long total) { const long g = (total + 255) / 256; return (unsigned)(g < 1 ? 1 : g > 16384 ? 16384 : g); }

void launch_sam_patch(const SamPatchArgs& a, DType dt, hipStream_t s) {
    if (!a.img || !a.out || a.B <= 0 || a.S <= 0) return;
    const unsigned grid = flat_grid((long)a.B * a.S * a.S * 96);
    if (dt == DT_BF16) hipLaunchKernelGGL(sam_patch_kernel<__bf16>, dim3(grid), dim3(256), 0, s, a.img, (__bf16*)a.out, a.B, a.S);
    else hipLaunchKernelGGL(sam_patch_kernel<_Float16>, dim3(grid), dim3(256), 0, s, a.img, (_Float16*)a.out, a.B, a.S);
}

bool sam_window_ok(const SamWindowArgs& a) {
    if (!a.src || !a.dst || a.src == a.dst || a.B <= 0 || a.S <= 0 || a.win <= 0 || a.C <= 0 || a.C % 8 || (a.scatter != 0 && a.scatter != 1) || (a.R && !a.scatter)) return false;
    const long nw = (a.S + a.win - 1) / a.win;
    return (long)a.B * nw * nw * a.win * a.win * a.C < (1L << 40);
}
void launch_sam_window(const SamWindowArgs& a, DType dt, hipStream_t s) {
    if (!sam_window_ok(a)) return;
    const long nw = (a.S + a.win - 1) / a.win;
    const unsigned grid = flat_grid((a.scatter ? (long)a.B * a.S * a.S : (long)a.B * nw * nw * a.win * a.win) * (a.C / 8));
    if (dt == DT_BF16) hipLaunchKernelGGL(sam_window_kernel<__bf16>, dim3(grid), dim3(256), 0, s, a);
    else hipLaunchKernelGGL(sam_window_kernel<_Float16>, dim3(grid), dim3(256), 0, s, a);
}

bool sam_relpos_ok(const SamRelposArgs& a) {
    return a.Q && a.th && a.tw && a.out && a.BW > 0 && a.H > 0 && a.n > 0 && a.n <= 1024 && a.ldq % 8 == 0 && a.ldq >= a.H * 64 && (long)a.BW * a.H < (1L << 31);
}
void launch_sam_relpos(const SamRelposArgs& a, DType dt, hipStream_t s) {
    if (!sam_relpos_ok(a)) return;
    const unsigned grid = flat_grid((long)a.BW * a.H * a.n * a.n * 2 * a.n);
    if (dt == DT_BF16) hipLaunchKernelGGL(sam_relpos_kernel<__bf16>, dim3(grid), dim3(256), 0, s, a);
    else hipLaunchKernelGGL(sam_relpos_kernel<_Float16>, dim3(grid), dim3(256), 0, s, a);
}

bool sam_attn_ok(const SamAttnArgs& a) {
    return a.Q && a.K && a.V && a.rel && a.O && a.BW > 0 && a.H > 0 && a.n > 0 && a.n <= 1024 && a.ld % 8 == 0 && a.ld >= a.H * 64 && a.ldo % 4 == 0 && a.ldo >= a.H * 64 &&
           (long)a.BW * a.H <= 65535;          // grid.y
}
void launch_sam_attention(const SamAttnArgs& a, DType dt, hipStream_t s) {
    if (!sam_attn_ok(a)) return;
    const dim3 grid((unsigned)((a.n * a.n + AQ - 1) / AQ), (unsigned)(a.BW * a.H));
    if (dt == DT_BF16) hipLaunchKernelGGL(sam_attn_kernel<__bf16>, grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL(sam_attn_kernel<_Float16>, grid, dim3(256), 0, s, a);
}

void launch_sam_rowvec(const SamRowvecArgs& a, DType dt, hipStream_t s) {
    if (!a.X || !a.vec || a.rows <= 0 || a.C <= 0 || a.C % 8 || a.ld % 8 || a.period <= 0) return;
    const unsigned grid = flat_grid(a.rows * (a.C / 8));
    if (dt == DT_BF16) hipLaunchKernelGGL(sam_rowvec_kernel<__bf16>, dim3(grid), dim3(256), 0, s, a);
    else hipLaunchKernelGGL(sam_rowvec_kernel<_Float16>, dim3(grid), dim3(256), 0, s, a);
}

void launch_sam_out(const SamOutArgs& a, DType dt, hipStream_t s) {
    if (!a.X || !a.out || a.B <= 0 || a.C <= 0 || a.HW <= 0) return;
    const unsigned grid = flat_grid((long)a.B * a.C * a.HW);
    if (dt == DT_BF16) hipLaunchKernelGGL(sam_out_kernel<__bf16>, dim3(grid), dim3(256), 0, s, (const __bf16*)a.X, a.ld, a.out, a.B, a.C, a.HW);
    else hipLaunchKernelGGL(sam_out_kernel<_Float16>, dim3(grid), dim3(256), 0, s, (const _Float16*)a.X, a.ld, a.out, a.B, a.C, a.HW);
}

void launch_sam_preprocess(const SamPreprocessArgs& a, hipStream_t s) {
    if (!a.in || !a.out || a.size <= 0 || a.h <= 0 || a.w <= 0) return;
    hipLaunchKernelGGL(sam_preprocess_kernel, dim3(flat_grid(3L * a.size * a.size)), dim3(256), 0, s, a.in, a.pitch, a.h, a.w, a.out, a.size);
}

}  // namespace ldx
