// Stand-in HIP runtime for libldx_host.so (`make -C lightdiffusion-next_amd/csrc host`): every entry point the library imports, on the host, with no GPU and no
// GPU memory.  hipMalloc hands out addresses from a deterministic bump allocator with nothing behind them; copies, memsets and synchronisation succeed and do
// nothing; hipLaunchKernel, hipMemcpyAsync and hipMemset append one line each to the file named by LDX_STANDIN_TRACE:
//     L <mangled kernel name> <grid x,y,z> <block x,y,z> <dynamic LDS bytes> <hex bytes of argument 0>:<argument 1>:...
//     C <dst> <src> <bytes> <kind>
//     S <dst> <value> <bytes>
// With LDX_STANDIN_WEIGHTS set, a synchronous host-to-device hipMemcpy (how every packed weight buffer and every staged source arrives) adds
//     W <dst> <bytes> <64-bit FNV-1a of the bytes>
// so that the packed bytes themselves can be held to a table (tests/tools/plan_trace.py --weights); without it hipMemcpy records nothing.
// Graphs: hipStreamBeginCapture(s) starts a node list for s, and a launch or asynchronous copy on a capturing stream appends its record to that list instead of the
// file; hipStreamEndCapture hands the list out as the graph.  Begin, end, instantiate and launch write one line each, a launch followed by its nodes' records:
//     G begin <stream> / G end <stream> <nodes> / G instantiate <nodes> / G launch <stream> <nodes>
// What a real runtime refuses or serialises while a capture is open (hipFuncSetAttribute, hipMalloc, hipFree, synchronous hipMemcpy / hipMemset,
// hipDeviceSynchronize, hipStreamSynchronize of the capturing stream) writes
//     ! <api> during capture
// LDX_STANDIN_FAIL=<api name>, read at every call of hipStreamEndCapture, hipGraphInstantiate and hipGraphLaunch, makes that call return hipErrorUnknown (the
// capture is ended all the same, and no graph is handed out).
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
    uintptr_t next_stream = 0x5000;                                        // stream handles: distinct, never null, never reused
    std::unordered_map<hipStream_t, std::vector<std::string>*> capturing;  // capturing stream -> the node list of its graph so far
};
typedef std::vector<std::string> Nodes;                                    // a graph, and an executable graph (its own copy): the records of the nodes
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
// a record: into the node list of a capturing stream, else into the file
void record(hipStream_t st, const std::string& line) {
    FILE* f = trace();
    auto it = S().capturing.find(st);
    if (it != S().capturing.end()) it->second->push_back(line);
    else if (f) { fputs(line.c_str(), f); fputc('\n', f); }
}
void not_in_capture(const char* api) {
    FILE* f = trace();
    if (f && !S().capturing.empty()) fprintf(f, "! %s during capture\n", api);
}
bool fails(const char* api) { const char* p = getenv("LDX_STANDIN_FAIL"); return p && !strcmp(p, api); }
}  // namespace

extern "C" {
void** __hipRegisterFatBinary(const void*) { static void* handle; return &handle; }
void __hipUnregisterFatBinary(void**) {}
void __hipRegisterFunction(void**, const void* host_fn, char*, const char* device_name, unsigned, void*, void*, void*, void*, int*) { S().names[host_fn] = device_name; }
hipError_t __hipPushCallConfiguration(dim3 grid, dim3 block, size_t lds, hipStream_t st) { State& s = S(); s.grid = grid; s.block = block; s.lds = lds; s.stream = st; return hipSuccess; }
hipError_t __hipPopCallConfiguration(dim3* grid, dim3* block, size_t* lds, hipStream_t* st) { State& s = S(); *grid = s.grid; *block = s.block; *lds = s.lds; *st = s.stream; return hipSuccess; }

hipError_t hipLaunchKernel(const void* fn, dim3 grid, dim3 block, void** args, size_t lds, hipStream_t st) {
    State& s = S();
    if (!trace() && s.capturing.empty()) return hipSuccess;
    auto it = s.names.find(fn);
    const std::string name = it == s.names.end() ? "?" : it->second;
    char head[128];
    snprintf(head, sizeof(head), " %u,%u,%u %u,%u,%u %zu ", grid.x, grid.y, grid.z, block.x, block.y, block.z, lds);
    std::string line = "L " + name + head;
    auto sz = s.arg_sizes.find(name);
    if (sz == s.arg_sizes.end()) line += '?';
    else for (size_t i = 0; i < sz->second.size(); ++i) {
        if (i) line += ':';
        for (int b = 0; b < sz->second[i]; ++b) { const unsigned char c = ((const unsigned char*)args[i])[b]; line += "0123456789abcdef"[c >> 4]; line += "0123456789abcdef"[c & 15]; }
    }
    record(st, line);
    return hipSuccess;
}
hipError_t hipMemcpyAsync(void* dst, const void* src, size_t n, hipMemcpyKind kind, hipStream_t st) {
    char line[128];
    snprintf(line, sizeof(line), "C %p %p %zu %d", kind == hipMemcpyDeviceToHost ? nullptr : dst, src, n, (int)kind);      // a host destination is no part of the plan
    record(st, line);
    return hipSuccess;
}
hipError_t hipMemset(void* dst, int v, size_t n) {
    not_in_capture("hipMemset");
    if (FILE* f = trace()) fprintf(f, "S %p %d %zu\n", dst, v, n);
    return hipSuccess;
}
hipError_t hipMalloc(void** p, size_t n) { not_in_capture("hipMalloc"); State& s = S(); *p = (void*)s.next; s.next += (n + 4095) & ~(size_t)4095; if (!n) s.next += 4096; return hipSuccess; }
hipError_t hipFree(void*) { not_in_capture("hipFree"); return hipSuccess; }
hipError_t hipMemcpy(void* dst, const void* src, size_t n, hipMemcpyKind kind) {
    not_in_capture("hipMemcpy");
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
hipError_t hipDeviceSynchronize() { not_in_capture("hipDeviceSynchronize"); return hipSuccess; }
hipError_t hipStreamSynchronize(hipStream_t st) { if (S().capturing.count(st)) not_in_capture("hipStreamSynchronize"); return hipSuccess; }
hipError_t hipStreamCreateWithFlags(hipStream_t* s, unsigned) { *s = (hipStream_t)S().next_stream; S().next_stream += 0x100; return hipSuccess; }
hipError_t hipStreamDestroy(hipStream_t) { return hipSuccess; }
hipError_t hipFuncSetAttribute(const void*, hipFuncAttribute, int) { not_in_capture("hipFuncSetAttribute"); return hipSuccess; }
hipError_t hipGetLastError() { return hipSuccess; }
const char* hipGetErrorString(hipError_t e) { return e == hipSuccess ? "no error" : "stand-in runtime error"; }
hipError_t hipEventCreate(hipEvent_t* e) { *e = nullptr; return hipSuccess; }
hipError_t hipEventDestroy(hipEvent_t) { return hipSuccess; }
hipError_t hipEventRecord(hipEvent_t, hipStream_t) { return hipSuccess; }
hipError_t hipEventElapsedTime(float* ms, hipEvent_t, hipEvent_t) { *ms = 0.f; return hipSuccess; }
hipError_t hipStreamBeginCapture(hipStream_t st, hipStreamCaptureMode) {
    if (S().capturing.count(st)) return hipErrorIllegalState;
    S().capturing[st] = new Nodes;
    if (FILE* f = trace()) fprintf(f, "G begin %p\n", (void*)st);
    return hipSuccess;
}
hipError_t hipStreamEndCapture(hipStream_t st, hipGraph_t* g) {
    auto it = S().capturing.find(st);
    if (it == S().capturing.end()) return hipErrorIllegalState;
    Nodes* nodes = it->second;
    S().capturing.erase(it);
    if (FILE* f = trace()) fprintf(f, "G end %p %zu\n", (void*)st, nodes->size());
    if (fails("hipStreamEndCapture")) { delete nodes; *g = nullptr; return hipErrorUnknown; }
    *g = (hipGraph_t)nodes;
    return hipSuccess;
}
hipError_t hipGraphInstantiate(hipGraphExec_t* e, hipGraph_t g, hipGraphNode_t*, char*, size_t) {
    if (fails("hipGraphInstantiate")) return hipErrorUnknown;
    if (FILE* f = trace()) fprintf(f, "G instantiate %zu\n", ((Nodes*)g)->size());
    *e = (hipGraphExec_t) new Nodes(*(Nodes*)g);
    return hipSuccess;
}
hipError_t hipGraphLaunch(hipGraphExec_t e, hipStream_t st) {
    if (fails("hipGraphLaunch")) return hipErrorUnknown;
    const Nodes& nodes = *(Nodes*)e;
    if (FILE* f = trace()) fprintf(f, "G launch %p %zu\n", (void*)st, nodes.size());
    for (const std::string& n : nodes) record(st, n);          // into st's own capture, were it capturing
    return hipSuccess;
}
hipError_t hipGraphDestroy(hipGraph_t g) { delete (Nodes*)g; return hipSuccess; }
hipError_t hipGraphExecDestroy(hipGraphExec_t e) { delete (Nodes*)e; return hipSuccess; }
}
