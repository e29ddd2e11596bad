// Weight packing on the device: the layouts of the UNet's structure walk (engine.cpp walk_weights), from state-dict tensors that already live on the GPU
// (ldx_load_tensor_device).  Run once per load / refresh, memory bound and small next to one sampling run, so the kernels are plain loops over
// weight_layout.h's element functions: the very code the host packers run over host pointers, so every bit equals the host's by construction.
#include "../../include/ldx.h"
#include "ldx_kernels.h"
#include "weight_layout.h"

namespace ldx {

// one thread = eight consecutive output columns of one row (one 16-byte store)
__global__ __launch_bounds__(256) void pack16_kernel(const PackArgs p) {
    const size_t per_row = (size_t)p.K / 8, total = (size_t)p.N * per_row;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) pack16_group(p, i / per_row, (i % per_row) * 8, 8);
}

__global__ __launch_bounds__(256) void pack32_kernel(const PackVecArgs p) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < p.n) pack32_at(p, (size_t)i);
}

// one thread per output row
__global__ __launch_bounds__(64) void ln_fold_kernel(const LnFoldArgs p) {
    const int r = blockIdx.x * 64 + threadIdx.x;
    if (r < p.N) ln_fold_row(p, (size_t)r);
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
