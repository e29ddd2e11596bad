// GGML Q8_0 -> fp16 on the device (ldx_load_tensor_q8_0, ldx_op_dequant_q8_0): the weights of the reference's Flux and T5 files
// (Quantize/Quantizer.py:94-112).  A block is 34 bytes: an fp16 scale d and 32 int8 values q; a weight is fp16_rne(float(d) * q), torch's
// d.view(float16) * q.view(int8).  The product of an 11-bit and an 8-bit significand is exact in fp32, so the one rounding is weight_convert.h's
// float_to_half: the integer code the host expansion (q8_0_value below, called by Engine::load_tensor_q8_0) runs too.  Run once per tensor at load time,
// memory bound: 1.06 bytes read and 2 written per weight.
#include "../../include/ldx.h"
#include "ldx_kernels.h"
#include "weight_convert.h"

namespace ldx {

// one thread = eight consecutive weights of one block: the scale and four 16-bit loads (a block is 2-byte aligned, no more), one 16-byte store
// (two for fp32).  Grid-stride over size_t groups: T5-XXL's embedding has 132 M weights.
__global__ __launch_bounds__(256) void dequant_q8_0_kernel(const DequantQ8Args p) {
    const size_t groups = p.n / 8;
    const uint16_t* src = (const uint16_t*)p.blocks;
    for (size_t g = (size_t)blockIdx.x * 256 + threadIdx.x; g < groups; g += (size_t)gridDim.x * 256) {
        const uint16_t* blk = src + (g / 4) * (Q8_0_BYTES / 2);
        const uint16_t d = blk[0];
        const uint16_t* q = blk + 1 + (g % 4) * 4;
        uint16_t h[8];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const uint16_t two = q[j];
            h[2 * j] = q8_0_value(d, (int8_t)(two & 0xff));
            h[2 * j + 1] = q8_0_value(d, (int8_t)(two >> 8));
        }
        if (p.out_dt == LDX_F32) {
            float4 a, b;
            a.x = half_to_float(h[0]); a.y = half_to_float(h[1]); a.z = half_to_float(h[2]); a.w = half_to_float(h[3]);
            b.x = half_to_float(h[4]); b.y = half_to_float(h[5]); b.z = half_to_float(h[6]); b.w = half_to_float(h[7]);
            float4* o = (float4*)p.out + g * 2;
            o[0] = a; o[1] = b;
        } else {
            if (p.out_dt == LDX_BF16) {
#pragma unroll
                for (int j = 0; j < 8; ++j) h[j] = float_to_bf16(half_to_float(h[j]));
            }
            uint4 u;
            u.x = h[0] | ((uint32_t)h[1] << 16); u.y = h[2] | ((uint32_t)h[3] << 16);
            u.z = h[4] | ((uint32_t)h[5] << 16); u.w = h[6] | ((uint32_t)h[7] << 16);
            ((uint4*)p.out)[g] = u;
        }
    }
}

void launch_dequant_q8_0(const DequantQ8Args& a, hipStream_t s) {
    if (a.n == 0) return;
    size_t grid = (a.n / 8 + 255) / 256;
    if (grid > 16384) grid = 16384;
    hipLaunchKernelGGL(dequant_q8_0_kernel, dim3((unsigned)grid), dim3(256), 0, s, a);
}

}  // namespace ldx
