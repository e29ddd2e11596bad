// Stand-in HIP runtime for libldx_host.so (`make -C lightdiffusion-next_amd/csrc host`): every entry point the library imports, on the host, with no GPU and no
// GPU memory.  hipMalloc hands out addresses from a deterministic bump allocator with nothing behind them; copies, memsets and synchronisation succeed and do
// nothing; hipLaunchKernel, hipMemcpyAsync and hipMemset append one line each to the file named by LDX_STANDIN_TRACE:
//     L <mangled kernel name> <grid x,y,z> <block x,y,z> <dynamic LDS bytes> <hex bytes of argument 0>:<argument 1>:...
//     C <dst> <src> <bytes> <kind>
//     S <dst> <value> <bytes>
// With LDX_STANDIN_WEIGHTS set, a synchronous host-to-device hipMemcpy (how every packed weight buffer and every staged source arrives) adds
//     W <dst> <bytes> <64-bit FNV-1a of the bytes>
// so that the packed bytes themselves can be held to a table (tests/tools/plan_trace.py --weights); without it hipMemcpy records nothing.
// The size of every explicit kernel argument comes from the file named by LDX_STANDIN_ARGS (one line per kernel: name, then the sizes; tests/tools/plan_trace.py
// writes it from the metadata of the real libldx.so's code objects).  tests/tools/plan_trace.py drives the C ABI of the library linked against this file.
#include <hip/hip_runtime_api.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <unordered_map>
#include <vector>

namespace {
struct State {
    std::unordered_map<const void*, std::string> names;                    // host stub -> mangled device name
    std::unordered_map<std::string, std::vector<int>> arg_sizes;
    FILE* trace = nullptr;
    uintptr_t next = 0x100000000000ull;                                    // bump allocator: 4 KiB aligned, never reused
    bool env_read = false, weights = false;
    dim3 grid, block; size_t lds = 0; hipStream_t stream = nullptr;        // __hipPushCallConfiguration
};
State& S() { static State* s = new State; return *s; }                     // never destroyed: module destructors of the library still call in at exit
FILE* trace() {
    State& s = S();
    if (!s.env_read) {
        s.env_read = true;
        if (const char* p = getenv("LDX_STANDIN_TRACE")) s.trace = fopen(p, "w");
        s.weights = getenv("LDX_STANDIN_WEIGHTS") != nullptr;
        if (s.trace) setvbuf(s.trace, nullptr, _IOLBF, 1 << 16);           // a reader sees every record as soon as the call that made it returns
        if (const char* p = getenv("LDX_STANDIN_ARGS")) {
            if (FILE* f = fopen(p, "r")) {
                char line[8192];
                while (fgets(line, sizeof(line), f)) {
                    char* tok = strtok(line, " \n");
                    if (!tok) continue;
                    std::vector<int>& v = s.arg_sizes[tok];
                    while ((tok = strtok(nullptr, " \n"))) v.push_back(atoi(tok));
                }
                fclose(f);
            }
        }
    }
    return s.trace;
}
}  // namespace

extern "C" {
void** __hipRegisterFatBinary(const void*) { static void* handle; return &handle; }
void __hipUnregisterFatBinary(void**) {}
void __hipRegisterFunction(void**, const void* host_fn, char*, const char* device_name, unsigned, void*, void*, void*, void*, int*) { S().names[host_fn] = device_name; }
hipError_t __hipPushCallConfiguration(dim3 grid, dim3 block, size_t lds, hipStream_t st) { State& s = S(); s.grid = grid; s.block = block; s.lds = lds; s.stream = st; return hipSuccess; }
hipError_t __hipPopCallConfiguration(dim3* grid, dim3* block, size_t* lds, hipStream_t* st) { State& s = S(); *grid = s.grid; *block = s.block; *lds = s.lds; *st = s.stream; return hipSuccess; }

hipError_t hipLaunchKernel(const void* fn, dim3 grid, dim3 block, void** args, size_t lds, hipStream_t) {
    FILE* f = trace();
    if (!f) return hipSuccess;
    State& s = S();
    auto it = s.names.find(fn);
    const std::string name = it == s.names.end() ? "?" : it->second;
    fprintf(f, "L %s %u,%u,%u %u,%u,%u %zu ", name.c_str(), grid.x, grid.y, grid.z, block.x, block.y, block.z, lds);
    auto sz = s.arg_sizes.find(name);
    if (sz == s.arg_sizes.end()) fputs("?", f);
    else for (size_t i = 0; i < sz->second.size(); ++i) {
        if (i) fputc(':', f);
        for (int b = 0; b < sz->second[i]; ++b) { const unsigned char c = ((const unsigned char*)args[i])[b]; fputc("0123456789abcdef"[c >> 4], f); fputc("0123456789abcdef"[c & 15], f); }
    }
    fputc('\n', f);
    return hipSuccess;
}
hipError_t hipMemcpyAsync(void* dst, const void* src, size_t n, hipMemcpyKind kind, hipStream_t) {
    if (FILE* f = trace()) fprintf(f, "C %p %p %zu %d\n", kind == hipMemcpyDeviceToHost ? nullptr : dst, src, n, (int)kind);      // a host destination is no part of the plan
    return hipSuccess;
}
hipError_t hipMemset(void* dst, int v, size_t n) {
    if (FILE* f = trace()) fprintf(f, "S %p %d %zu\n", dst, v, n);
    return hipSuccess;
}
hipError_t hipMalloc(void** p, size_t n) { State& s = S(); *p = (void*)s.next; s.next += (n + 4095) & ~(size_t)4095; if (!n) s.next += 4096; return hipSuccess; }
hipError_t hipFree(void*) { return hipSuccess; }
hipError_t hipMemcpy(void* dst, const void* src, size_t n, hipMemcpyKind kind) {
    FILE* f = trace();
    if (!f || !S().weights || kind != hipMemcpyHostToDevice) return hipSuccess;
    uint64_t h = 0xcbf29ce484222325ull;
    for (size_t i = 0; i < n; ++i) { h ^= ((const unsigned char*)src)[i]; h *= 0x100000001b3ull; }
    fprintf(f, "W %p %zu %016llx\n", dst, n, (unsigned long long)h);
    return hipSuccess;
}
hipError_t hipGetDeviceCount(int* n) { *n = 1; return hipSuccess; }
hipError_t hipGetDevice(int* d) { *d = 0; return hipSuccess; }
hipError_t hipSetDevice(int d) { return d == 0 ? hipSuccess : hipErrorInvalidDevice; }
hipError_t hipDeviceGetAttribute(int* v, hipDeviceAttribute_t a, int) { *v = a == hipDeviceAttributeMultiprocessorCount ? 256 : 0; return hipSuccess; }
hipError_t hipDeviceSynchronize() { return hipSuccess; }
hipError_t hipStreamSynchronize(hipStream_t) { return hipSuccess; }
hipError_t hipStreamCreateWithFlags(hipStream_t* s, unsigned) { *s = nullptr; return hipSuccess; }
hipError_t hipStreamDestroy(hipStream_t) { return hipSuccess; }
hipError_t hipFuncSetAttribute(const void*, hipFuncAttribute, int) { return hipSuccess; }
hipError_t hipGetLastError() { return hipSuccess; }
const char* hipGetErrorString(hipError_t e) { return e == hipSuccess ? "no error" : "stand-in runtime error"; }
hipError_t hipEventCreate(hipEvent_t* e) { *e = nullptr; return hipSuccess; }
hipError_t hipEventDestroy(hipEvent_t) { return hipSuccess; }
hipError_t hipEventRecord(hipEvent_t, hipStream_t) { return hipSuccess; }
hipError_t hipEventElapsedTime(float* ms, hipEvent_t, hipEvent_t) { *ms = 0.f; return hipSuccess; }
// the recorder never enables graph mode
hipError_t hipStreamBeginCapture(hipStream_t, hipStreamCaptureMode) { return hipErrorNotSupported; }
hipError_t hipStreamEndCapture(hipStream_t, hipGraph_t*) { return hipErrorNotSupported; }
hipError_t hipGraphInstantiate(hipGraphExec_t*, hipGraph_t, hipGraphNode_t*, char*, size_t) { return hipErrorNotSupported; }
hipError_t hipGraphLaunch(hipGraphExec_t, hipStream_t) { return hipErrorNotSupported; }
hipError_t hipGraphDestroy(hipGraph_t) { return hipErrorNotSupported; }
hipError_t hipGraphExecDestroy(hipGraphExec_t) { return hipErrorNotSupported; }
}
