// The phase-form up conv (GemmArgs::up2x): the ping-pong kernel's MODE 2 (gemm_pp.inc) at 256 x 160, the one width gemm_pick gives it, in bf16 and f16, and the kernel
// that derives the phase weights.  Linked into libldx_upconv.so next to libldx.so, like the packers, the image ops, the TAESD decoder and AutoHDR:
// tests/golden/kernel_resources.json keeps pinning the kernels of libldx.so as they were; tests/test_upconv_resources_cpu.py holds these to the no-scratch rule.
#include "gemm_common.h"
#include "weight_layout.h"

namespace ldx {

#include "gemm_pp.inc"

void launch_pp_up2x_bf16(const GemmArgs& a, hipStream_t s) { launch_pp_inst<__bf16, 2, 160>(a, 1, s); }
void launch_pp_up2x_f16(const GemmArgs& a, hipStream_t s) { launch_pp_inst<_Float16, 2, 160>(a, 1, s); }

// the phase weights of an up conv (GemmArgs::up2x): one thread = eight consecutive columns of one row of the [4 * N][4 * Cin] buffer.  Run when the first plan that
// wants the phase form is built and after a weight refresh, so a plain loop over weight_layout.h's element function.
__global__ __launch_bounds__(256) void up_phase_kernel(const UpPhaseArgs p) {
    const size_t per_row = (size_t)p.Cin / 2, total = (size_t)4 * p.N * per_row;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) up_phase_group(p, i / per_row, (i % per_row) * 8);
}
void launch_up_phase(const UpPhaseArgs& a, hipStream_t s) {
    if (a.N <= 0 || a.Cin <= 0) return;
    size_t grid = ((size_t)4 * a.N * (a.Cin / 2) + 255) / 256; if (grid > 8192) grid = 8192;
    hipLaunchKernelGGL(up_phase_kernel, dim3((unsigned)grid), dim3(256), 0, s, a);
}

}  // namespace ldx
