// ldx engines: the host-side planner / executor every model shares, behind the C ABI (include/ldx.h).  The models themselves are the classes
// derived from Engine (engine_unet.cpp, engine_vae.cpp, engine_clip.cpp, engine_t5.cpp, engine_esrgan.cpp, engine_flux.cpp, engine_taesd.cpp, engine_sam.cpp).
//
// A model runs as a static launch plan over one activation arena: weights are packed once into MFMA-friendly
// [N][K] 16-bit matrices (conv3x3 -> [Cout][ky][kx][Cin], q/k/v fused, GEGLU rows slab-interleaved),
// activations stay NHWC 16-bit, channel concat is a column offset, and every op is one of the HIP
// kernels in csrc/*.hip.  No CPU fallback exists: without a HIP device every call fails.
#include "engine.h"
#include "weight_layout.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <thread>

namespace ldx {

thread_local std::string g_last_error;
void set_error(const std::string& s) { g_last_error = s; }
int launch_status() {
    const hipError_t e = hipGetLastError();
    if (e == hipSuccess) return LDX_OK;
    set_error(std::string("kernel launch: ") + hipGetErrorString(e));
    return LDX_EHIP;
}

// ---------------------------------------------------------------------------------------------
// 16-bit conversions (round-to-nearest-even): weight_convert.h, one copy for the host and the device packers
float HostTensor::at(size_t i) const {
    switch (dtype) {
        case LDX_F32: return ((const float*)data.data())[i];
        case LDX_F16: return half_to_float(((const uint16_t*)data.data())[i]);
        default: return bf16_to_float(((const uint16_t*)data.data())[i]);
    }
}

static void parallel_for(size_t n, const std::function<void(size_t, size_t)>& fn) {
    unsigned nt = std::thread::hardware_concurrency();
    if (nt == 0) nt = 4;
    if (nt > 32) nt = 32;
    if (n < 1u << 16) { fn(0, n); return; }
    std::vector<std::thread> th;
    const size_t per = (n + nt - 1) / nt;
    for (unsigned t = 0; t < nt; ++t) {
        const size_t b = t * per, e = std::min(n, b + per);
        if (b >= e) break;
        th.emplace_back([=, &fn] { fn(b, e); });
    }
    for (auto& x : th) x.join();
}

// ---------------------------------------------------------------------------------------------
Engine::~Engine() {
    (void)hipSetDevice(device);
    for (void* p : dev_allocs) (void)hipFree(p);
    drop_staged();
    cur.release();
    for (Plan& p : plan_cache) p.release();
    if (cap_stream) (void)hipStreamDestroy(cap_stream);
    for (hipEvent_t ev : prof_events) (void)hipEventDestroy(ev);
}

int Engine::load_tensor(const char* key, const void* data, int dtype, const int64_t* shape, int ndim) {
    if (finalized && !refreshing) { set_error("ldx_load_tensor after ldx_finalize"); return LDX_ESTATE; }
    if (!key || !data || ndim < 0 || ndim > 8) { set_error("ldx_load_tensor: bad argument"); return LDX_EINVAL; }
    if (dtype != LDX_F32 && dtype != LDX_F16 && dtype != LDX_BF16) { set_error("ldx_load_tensor: bad dtype"); return LDX_EINVAL; }
    HostTensor t;
    t.dtype = dtype;
    size_t n = 1;
    for (int i = 0; i < ndim; ++i) { t.shape.push_back(shape[i]); n *= (size_t)shape[i]; }
    t.numel = n;
    const size_t esz = dtype == LDX_F32 ? 4 : 2;
    t.data.resize(n * esz);
    memcpy(t.data.data(), data, n * esz);
    host[key] = std::move(t);
    return LDX_OK;
}

int Engine::load_tensor_dev(const char* fn, const char* key, const void* dev_ptr, int dtype, const int64_t* shape, int ndim) {
    const std::string f(fn);
    if (finalized && !refreshing) { set_error(f + " after ldx_finalize"); return LDX_ESTATE; }
    if (!key || !dev_ptr || ndim < 0 || ndim > 8 || (ndim && !shape)) { set_error(f + ": bad argument"); return LDX_EINVAL; }
    if (dtype != LDX_F32 && dtype != LDX_F16 && dtype != LDX_BF16) { set_error(f + ": bad dtype"); return LDX_EINVAL; }
    if ((uintptr_t)dev_ptr % (dtype == LDX_F32 ? 4 : 2)) { set_error(f + ": misaligned pointer"); return LDX_EINVAL; }
    HostTensor t;
    t.dtype = dtype;
    t.numel = 1;
    for (int i = 0; i < ndim; ++i) {
        if (shape[i] < 0) { set_error(f + ": negative extent"); return LDX_EINVAL; }
        t.shape.push_back(shape[i]); t.numel *= (size_t)shape[i];
    }
    t.dev = dev_ptr;
    host[key] = std::move(t);
    return LDX_OK;
}

// A Q8_0 tensor becomes an LDX_F16 one here, by the one rule of weight_convert.h (q8_0_value): nothing behind this call knows the file was quantised
int Engine::load_tensor_q8_0(const char* key, const void* blocks, const int64_t* shape, int ndim, bool on_device) {
    if (finalized) { set_error("ldx_load_tensor_q8_0 after ldx_finalize"); return LDX_ESTATE; }
    if (!key || !blocks || !shape || ndim <= 0 || ndim > 8 || (uintptr_t)blocks % 2) { set_error("ldx_load_tensor_q8_0: bad argument (null or odd pointer, ndim outside 1..8)"); return LDX_EINVAL; }
    HostTensor t;
    t.dtype = LDX_F16;
    t.numel = 1;
    for (int i = 0; i < ndim; ++i) {
        if (shape[i] < 0) { set_error("ldx_load_tensor_q8_0: negative extent"); return LDX_EINVAL; }
        t.shape.push_back(shape[i]); t.numel *= (size_t)shape[i];
    }
    if (shape[ndim - 1] % Q8_0_BLOCK) { set_error("ldx_load_tensor_q8_0: the innermost extent must be a multiple of 32"); return LDX_EINVAL; }
    if (on_device) {
        HIP_OK(hipSetDevice(device));
        void* p = nullptr;
        HIP_OK(hipMalloc(&p, std::max<size_t>(t.numel * 2, 16)));
        q8_bufs.push_back(p);
        launch_dequant_q8_0(DequantQ8Args{blocks, p, t.numel, LDX_F16}, nullptr);
        if (int rc = launch_status()) return rc;
        HIP_OK(hipDeviceSynchronize());            // `blocks` may be freed when this returns
        t.dev = p;
    } else {
        t.data.resize(t.numel * 2);
        uint16_t* out = (uint16_t*)t.data.data();
        const uint8_t* src = (const uint8_t*)blocks;
        parallel_for(t.numel / Q8_0_BLOCK, [&](size_t b, size_t e) {
            for (size_t i = b; i < e; ++i) {
                const uint8_t* blk = src + i * Q8_0_BYTES;
                const uint16_t d = (uint16_t)(blk[0] | (blk[1] << 8));
                for (int j = 0; j < Q8_0_BLOCK; ++j) out[i * Q8_0_BLOCK + j] = q8_0_value(d, (int8_t)blk[2 + j]);
            }
        });
    }
    host[key] = std::move(t);
    return LDX_OK;
}

int Engine::packed_digest(const char* fn, uint64_t* out) {
    if (!finalized) { set_error(std::string(fn) + ": not a finalized engine"); return LDX_ESTATE; }
    if (!out) { set_error(std::string(fn) + ": bad argument"); return LDX_EINVAL; }
    HIP_OK(hipSetDevice(device));
    HIP_OK(hipDeviceSynchronize());
    uint64_t h = 0xcbf29ce484222325ull;
    std::vector<uint8_t> buf;
    for (const WeightAlloc& a : weight_allocs) {
        buf.resize(a.bytes);
        HIP_OK(hipMemcpy(buf.data(), a.p, a.bytes, hipMemcpyDeviceToHost));
        for (size_t i = 0; i < a.bytes; ++i) { h ^= buf[i]; h *= 0x100000001b3ull; }
    }
    *out = h;
    return LDX_OK;
}

const HostTensor* Engine::get(const std::string& key, std::initializer_list<int64_t> shape) {
    auto it = host.find(key);
    if (it == host.end()) { missing = key; return nullptr; }
    const HostTensor& t = it->second;
    if (shape.size()) {
        bool ok = t.shape.size() == shape.size();
        size_t i = 0;
        if (ok) for (int64_t s : shape) ok = ok && (t.shape[i++] == s);
        if (!ok) { missing = key + " (shape mismatch)"; return nullptr; }
    }
    return &t;
}

// the next weight buffer of a model: a new allocation (ALLOC) or the one the same step of finalize()'s walk made (CHECK / REFILL)
void* Engine::weight_buf(size_t bytes) {
    if (walk_mode == WALK_ALLOC) {
        void* p = nullptr;
        if (hipMalloc(&p, bytes) != hipSuccess) return nullptr;
        dev_allocs.push_back(p);
        weight_allocs.push_back({p, bytes});      // read by the UNet's refresh and digest
        weight_bytes += bytes;
        return p;
    }
    if (walk_next >= weight_allocs.size() || weight_allocs[walk_next].bytes != bytes) {
        walk_err = "the weight layout differs from the one ldx_finalize built (plan switches changed since?)";
        return nullptr;
    }
    return weight_allocs[walk_next++].p;
}

// a [rows][cols] matrix produced by getter(r, c) as 16-bit / a vector produced by getter(i): the few layouts that are no piece list (engine.h)
void* Engine::upload16(size_t rows, size_t cols, const std::function<float(size_t, size_t)>& getter) {
    void* p = weight_buf(rows * cols * 2);
    if (!p || walk_mode == WALK_CHECK) return p;
    std::vector<uint16_t> buf(rows * cols);
    parallel_for(rows, [&](size_t b, size_t e) {
        for (size_t r = b; r < e; ++r)
            for (size_t c = 0; c < cols; ++c) buf[r * cols + c] = to16(getter(r, c), dt);
    });
    if (hipMemcpy(p, buf.data(), buf.size() * 2, hipMemcpyHostToDevice) != hipSuccess) return nullptr;
    return p;
}
float* Engine::upload32(size_t n, const std::function<float(size_t)>& getter) {
    void* p = weight_buf(n * 4);
    if (!p || walk_mode == WALK_CHECK) return (float*)p;
    std::vector<float> buf(n);
    for (size_t i = 0; i < n; ++i) buf[i] = getter(i);
    if (hipMemcpy(p, buf.data(), n * 4, hipMemcpyHostToDevice) != hipSuccess) return nullptr;
    return (float*)p;
}

// ---- packed buffers from pieces (weight_layout.h): pack.hip's kernels where a source lives on the GPU, the same functions on the CPU where none does ----
// the device address of a source: its own, or a staged raw copy of a host tensor that shares a packed buffer with device tensors
const void* Engine::dev_src(const HostTensor* t) {
    if (t->dev) return t->dev;
    auto it = staged.find(t);
    if (it != staged.end()) return it->second;
    void* p = nullptr;
    if (hipMalloc(&p, std::max<size_t>(t->data.size(), 4)) != hipSuccess) return nullptr;
    staged[t] = p;
    if (hipMemcpy(p, t->data.data(), t->data.size(), hipMemcpyHostToDevice) != hipSuccess) return nullptr;
    return p;
}
void Engine::drop_staged() {
    for (auto& kv : staged) (void)hipFree(kv.second);
    staged.clear();
    for (void* p : q8_bufs) (void)hipFree(p);
    q8_bufs.clear();
}
void* Engine::pack16(size_t rows, size_t cols, const std::vector<Piece>& pieces) {
    void* p = weight_buf(rows * cols * 2);
    if (!p) return p;
    bool dev = false;
    for (const Piece& pc : pieces) dev = dev || pc.src->dev;
    for (const Piece& pc : pieces) {
        // The pieces must lie inside [rows][cols] and match their sources; the kernel's 16-byte stores need more, which UNetEngine::validate() guarantees for every
        // UNet it accepts (all channel counts and context_dim are multiples of 64, conv_in is padded to 64).  Tested in every walk mode, so a refresh
        // reports it before anything is written.
        if (pc.row0 + pc.N > rows || pc.col0 + pc.K > cols || (dev && (pc.K % 8 || cols % 8 || pc.col0 % 8 || pc.CinPad % 8)) ||
            (pc.CinPad ? (pc.K != 9 * pc.CinPad || pc.Cin > pc.CinPad || pc.src->numel != (size_t)pc.N * pc.Cin * 9 || pc.src_rows)
                       : pc.src_rows ? (pc.src_row0 + pc.N > pc.src_rows || pc.src->numel != pc.src_rows * pc.K || pc.geglu_inner)
                                     : pc.src->numel != (size_t)(pc.geglu_inner ? 2 * pc.geglu_inner : pc.N) * pc.K) ||
            (pc.geglu_inner && (pc.N != 2 * pc.geglu_inner || pc.geglu_inner % 32))) {
            walk_err = dev ? "pack16: piece outside the packed matrix or not 16-byte granular" : "pack16: piece outside the packed matrix";
            return nullptr;
        }
    }
    if (walk_mode == WALK_CHECK) return p;
    std::vector<uint16_t> buf(dev ? 0 : rows * cols);
    for (const Piece& pc : pieces) {
        PackArgs a; memset(&a, 0, sizeof(a));
        a.src = piece_src(pc.src, dev); a.sdt = pc.src->dtype;
        if (!a.src) return nullptr;
        a.src = (const char*)a.src + pc.src_row0 * (size_t)pc.K * (a.sdt == LDX_F32 ? 4 : 2);      // a sub-view starts at its first row
        a.out = (uint16_t*)(dev ? p : buf.data()) + pc.row0 * cols; a.ldo = (long)cols; a.col0 = (long)pc.col0; a.out_dt = dt;
        a.N = pc.N; a.K = pc.K; a.Cin = pc.Cin; a.CinPad = pc.CinPad; a.geglu_inner = pc.geglu_inner; a.scale = pc.scale;
        if (dev) launch_pack16(a, nullptr);
        else parallel_for(pc.N, [&](size_t b, size_t e) {
            for (size_t r = b; r < e; ++r)
                for (int c = 0; c < a.K; c += 8) pack16_group(a, r, c, std::min(8, a.K - c));
        });
    }
    if (!dev && hipMemcpy(p, buf.data(), buf.size() * 2, hipMemcpyHostToDevice) != hipSuccess) return nullptr;
    return p;
}
float* Engine::pack32(size_t n, const std::vector<VecPiece>& pieces) {
    float* p = (float*)weight_buf(n * 4);
    if (!p) return p;
    bool dev = false;
    for (const VecPiece& pc : pieces) {
        dev = dev || pc.a->dev || (pc.b && pc.b->dev);
        if (pc.off + pc.n > n || (pc.src_n ? (pc.src0 + pc.n > pc.src_n || pc.a->numel != pc.src_n || pc.b || pc.geglu_inner) : pc.a->numel != (size_t)pc.n) ||
            (pc.b && pc.b->numel != (size_t)pc.n) || (pc.geglu_inner && pc.n != 2 * pc.geglu_inner)) {
            walk_err = "pack32: piece outside the packed vector";
            return nullptr;
        }
    }
    if (walk_mode == WALK_CHECK) return p;
    std::vector<float> buf(dev ? 0 : n);
    for (const VecPiece& pc : pieces) {
        PackVecArgs a; memset(&a, 0, sizeof(a));
        a.a = piece_src(pc.a, dev); a.a_dt = pc.a->dtype;
        if (!a.a) return nullptr;
        a.a = (const char*)a.a + pc.src0 * (a.a_dt == LDX_F32 ? 4 : 2);
        if (pc.b) { a.b = piece_src(pc.b, dev); a.b_dt = pc.b->dtype; if (!a.b) return nullptr; }
        a.out = (dev ? p : buf.data()) + pc.off; a.n = pc.n; a.geglu_inner = pc.geglu_inner;
        if (dev) launch_pack32(a, nullptr);
        else for (int i = 0; i < a.n; ++i) pack32_at(a, i);
    }
    if (!dev && hipMemcpy(p, buf.data(), n * 4, hipMemcpyHostToDevice) != hipSuccess) return nullptr;
    return p;
}

bool Engine::mk_linear(const std::string& pre, int N, int K, bool bias, LinearW& out, bool conv1x1) {
    const HostTensor* w = conv1x1 ? get(pre + ".weight", {N, K, 1, 1}) : get(pre + ".weight", {N, K});
    if (!w) return false;
    out.N = N; out.K = K;
    out.w = pack16(N, K, {rows_piece(w, 0, N, K)});
    out.b = nullptr;
    if (bias) {
        const HostTensor* b = get(pre + ".bias", {N});
        if (!b) return false;
        out.b = pack32(N, {{b, nullptr, 0, N, 0}});
        if (!out.b) return false;
    }
    return out.w != nullptr;
}
bool Engine::mk_conv3(const std::string& pre, int Cout, int Cin, int CinPad, LinearW& out) {
    const HostTensor* w = get(pre + ".weight", {Cout, Cin, 3, 3});
    const HostTensor* b = get(pre + ".bias", {Cout});
    if (!w || !b) return false;
    out.N = Cout; out.K = 9 * CinPad;
    out.w = pack16(Cout, (size_t)9 * CinPad, {conv_piece(w, Cout, Cin, CinPad)});
    out.b = pack32(Cout, {{b, nullptr, 0, Cout, 0}});
    return out.w && out.b;
}
bool Engine::mk_norm(const std::string& pre, int C, NormW& out) {
    const HostTensor* w = get(pre + ".weight", {C});
    const HostTensor* b = get(pre + ".bias", {C});
    if (!w || !b) return false;
    out.C = C;
    out.g = pack32(C, {{w, nullptr, 0, C, 0}});
    out.b = pack32(C, {{b, nullptr, 0, C, 0}});
    return out.g && out.b;
}

// Linear(LayerNorm(x)) with the norm folded in: y = rstd (x W'^T - mean c1) + c2 with W' = W .* gamma (per input column), c1[n] = sum_k W'[n][k]
// (of the values as STORED in 16 bit: the epilogue subtracts exactly what the MFMA accumulated for a constant row) and c2 = W beta + b.
// W = the pieces (row ranges of one [N][K] matrix), b = bias_t (may be null); weight_layout.h ln_fold_row writes a row of all three buffers.
bool Engine::mk_ln_folded(int N, int K, const std::vector<Piece>& pieces, const HostTensor* bias_t, const std::string& norm_pre, LinearW& out, float*& c1) {
    const HostTensor* g = get(norm_pre + ".weight", {K});
    const HostTensor* be = get(norm_pre + ".bias", {K});
    if (!g || !be) return false;
    bool dev = g->dev || be->dev || (bias_t && bias_t->dev);
    for (const Piece& pc : pieces) dev = dev || pc.src->dev;
    out.N = N; out.K = K;
    out.w = weight_buf((size_t)N * K * 2);
    c1 = (float*)weight_buf((size_t)N * 4);
    out.b = (float*)weight_buf((size_t)N * 4);
    if (!out.w || !c1 || !out.b) return false;
    for (const Piece& pc : pieces)
        if ((dev && K % 8) || pc.K != K || pc.row0 + pc.N > (size_t)N || (pc.geglu_inner && (pc.N != 2 * pc.geglu_inner || pc.N != N)) ||
            pc.src->numel != (size_t)pc.N * K || (bias_t && (pieces.size() != 1 || pc.row0 || bias_t->numel != (size_t)N))) {
            walk_err = "mk_ln_folded: piece outside the packed matrix";
            return false;
        }
    if (walk_mode == WALK_CHECK) return true;
    std::vector<uint16_t> hw(dev ? 0 : (size_t)N * K);
    std::vector<float> h1(dev ? 0 : N), h2(dev ? 0 : N);
    for (const Piece& pc : pieces) {
        LnFoldArgs a; memset(&a, 0, sizeof(a));
        a.src = piece_src(pc.src, dev); a.sdt = pc.src->dtype;
        a.gamma = piece_src(g, dev); a.g_dt = g->dtype; a.beta = piece_src(be, dev); a.b_dt = be->dtype;
        if (bias_t) { a.bias = piece_src(bias_t, dev); a.bias_dt = bias_t->dtype; if (!a.bias) return false; }
        if (!a.src || !a.gamma || !a.beta) return false;
        a.out = (uint16_t*)(dev ? out.w : hw.data()) + pc.row0 * K; a.out_dt = dt; a.c1 = (dev ? c1 : h1.data()) + pc.row0; a.c2 = (dev ? out.b : h2.data()) + pc.row0;
        a.N = pc.N; a.K = K; a.geglu_inner = pc.geglu_inner; a.scale = pc.scale;
        if (dev) launch_ln_fold(a, nullptr);
        else parallel_for(pc.N, [&](size_t b, size_t e) { for (size_t r = b; r < e; ++r) ln_fold_row(a, r); });
    }
    return dev || (hipMemcpy(out.w, hw.data(), hw.size() * 2, hipMemcpyHostToDevice) == hipSuccess && hipMemcpy(c1, h1.data(), (size_t)N * 4, hipMemcpyHostToDevice) == hipSuccess &&
                   hipMemcpy(out.b, h2.data(), (size_t)N * 4, hipMemcpyHostToDevice) == hipSuccess);
}

// out = conv2(h) + skip(x) as one implicit GEMM over K = 9 * Cout + Cin (GemmArgs::A2): weights [Cout][ky][kx][Cout] | [Cout][Cin], bias b2 + bskip
bool Engine::mk_fused_skip(const std::string& conv, const std::string& skip, int Cin, int Cout, ResW& r) {
    const HostTensor* w2 = get(conv + ".weight", {Cout, Cout, 3, 3});
    const HostTensor* b2 = get(conv + ".bias", {Cout});
    const HostTensor* ws = get(skip + ".weight", {Cout, Cin, 1, 1});
    const HostTensor* bs = get(skip + ".bias", {Cout});
    if (!w2 || !b2 || !ws || !bs) return false;
    r.fused_skip = true;
    r.conv2.N = Cout; r.conv2.K = 9 * Cout + Cin;
    r.conv2.w = pack16(Cout, (size_t)9 * Cout + Cin, {conv_piece(w2, Cout, Cout, Cout), Piece{ws, 0, (size_t)9 * Cout, Cout, Cin, 1.0f, 0, 0, 0}});
    r.conv2.b = pack32(Cout, {{b2, bs, 0, Cout, 0}});
    return r.conv2.w && r.conv2.b;
}

// rows of several tensors stacked into one [sum n][K] matrix, their biases (where they have one) into one vector
bool Engine::mk_stacked(const std::vector<EmbSrc>& srcs, int K, LinearW& out) {
    std::vector<Piece> wp; std::vector<VecPiece> bp;
    size_t row = 0;
    for (const EmbSrc& s : srcs) {
        wp.push_back(rows_piece(s.w, row, s.n, K));
        if (s.b) bp.push_back({s.b, nullptr, row, s.n, 0});
        row += s.n;
    }
    out.N = (int)row; out.K = K;
    out.w = pack16(row, K, wp);
    out.b = bp.empty() ? nullptr : pack32(row, bp);
    return out.w && (bp.empty() || out.b);
}

int Engine::weights_failed() {
    if (!missing.empty()) { set_error("missing or mis-shaped weight: " + missing); return LDX_EMISSING; }
    if (!walk_err.empty()) { set_error(walk_err); return LDX_ESTATE; }
    set_error(std::string("weight upload failed: ") + hipGetErrorString(hipGetLastError()));
    return LDX_EHIP;
}

// ---------------------------------------------------------------------------------------------
// arena allocator used at plan time (offsets), first-fit with coalescing
size_t Engine::a_alloc(size_t bytes) {
    bytes = (bytes + 255) & ~(size_t)255;
    for (size_t i = 0; i < free_list.size(); ++i) {
        if (free_list[i].second >= bytes) {
            const size_t off = free_list[i].first;
            if (free_list[i].second == bytes) free_list.erase(free_list.begin() + i);
            else { free_list[i].first += bytes; free_list[i].second -= bytes; }
            live[off] = bytes;
            return off;
        }
    }
    const size_t off = arena_top;
    arena_top += bytes;
    arena_peak = std::max(arena_peak, arena_top);
    live[off] = bytes;
    return off;
}
void Engine::a_free(size_t off) {
    auto it = live.find(off);
    if (it == live.end()) return;
    size_t sz = it->second;
    live.erase(it);
    free_list.emplace_back(off, sz);
    std::sort(free_list.begin(), free_list.end());
    for (size_t i = 0; i + 1 < free_list.size();) {
        if (free_list[i].first + free_list[i].second == free_list[i + 1].first) {
            free_list[i].second += free_list[i + 1].second;
            free_list.erase(free_list.begin() + i + 1);
        } else ++i;
    }
    if (!free_list.empty() && free_list.back().first + free_list.back().second == arena_top) {
        arena_top = free_list.back().first;
        free_list.pop_back();
    }
}

// Tile counters of the in-kernel split-K reduction (GemmArgs::sk_count): the engine's launches run in stream order and each leaves them at zero.
unsigned* Engine::sk_counters() {
#ifndef LDX_SK_FIXUP_BUILD
    return nullptr;                         // the in-kernel split-K reduction is not compiled in (gemm_sk_fixup() is constant false): no counters
#endif
    if (!d_sk_count) {
        if (hipMalloc((void**)&d_sk_count, sizeof(unsigned) * SK_COUNTERS) != hipSuccess) { d_sk_count = nullptr; return nullptr; }
        if (hipMemset(d_sk_count, 0, sizeof(unsigned) * SK_COUNTERS) != hipSuccess) { (void)hipFree(d_sk_count); d_sk_count = nullptr; return nullptr; }
        dev_allocs.push_back(d_sk_count);
    }
    return d_sk_count;
}

// ---- op emitters ---------------------------------------------------------------------------------
Op& Engine::emit(OpKind kind, const char* name) {
    cur.ops.emplace_back();
    Op& o = cur.ops.back();
    memset(&o, 0, sizeof(o)); o.kind = kind; o.name = name;
    return o;
}
// a_elems: 16-bit elements of the A operand as stored (a conv reads its image once, not nine times)
void Engine::seal_gemm(Op& o, const GemmEdit& edit, double a_elems, bool residual) {
    GemmArgs& g = o.g;
    gemm_attach_splitk(g, scratch);
    edit(o);
    if (!gemm_splitk_ok(g)) {          // what the planners' guards (xf_pick's folded stages, the edits that lower splitk) promise, checked where it matters
        set_error(std::string("planner bug: op ") + o.name + " keeps " + std::to_string(g.splitk) + " K splits with an epilogue that has no split-K form (ln_c1, gate, C8, geglu, up2x)");
        plan_rc = LDX_ESTATE;
    }
    o.flops = 2.0 * g.M * (double)g.N * g.K;
    o.bytes = 2.0 * (a_elems + (double)g.N * g.K + (double)g.M * (g.geglu ? g.N / 2 : g.N) * (residual ? 2 : 1));
    snprintf(o.klabel, sizeof(o.klabel), "gemm_kernel<%s,%d>", g.f8 ? "mxfp8" : dt_name(), g.mode);
    cur.flops += o.flops;
}
void Engine::op_gemm(const char* name, Act A, const LinearW& w, Act C, Act R, int geglu, const GemmEdit& edit) {
    Op& o = emit(OP_GEMM, name);
    GemmArgs& g = o.g = gemm_linear_args(ptr(A), A.ld, w.w, A.rows, w.N, w.K);
    g.bias = w.b; g.geglu = geglu; g.R = R.valid ? ptr(R) : nullptr; g.ldr = R.ld; g.C = ptr(C); g.ldc = C.ld;
    seal_gemm(o, edit, (double)g.M * g.K, R.valid);
}
void Engine::op_conv(const char* name, Act X, int B, int Hin, int Win, int Cin, const LinearW& w, int stride, int Hout, int Wout,
                     Act Y, Act R, const float* rowvec, int rv_ld, float* Cf, int ldcf, const GemmEdit& edit) {
    Op& o = emit(OP_GEMM, name);
    GemmArgs& g = o.g = gemm_conv_args(ptr(X), X.ld, w.w, B, Hin, Win, Cin, w.N, w.K, stride, Hout, Wout, stride == 1);      // a stride-1 conv whose output is larger reads its input resized
    g.bias = w.b; g.rowvec = rowvec; g.rowvec_ld = rv_ld; g.R = R.valid ? ptr(R) : nullptr; g.ldr = R.ld;
    g.C = Y.valid ? ptr(Y) : nullptr; g.ldc = Y.ld; g.Cf = Cf; g.ldcf = ldcf;
    seal_gemm(o, edit, (double)B * Hin * Win * Cin, R.valid);
}
// the kernels launch_groupnorm runs for the op as it stands (fuse_gn_stats asks again once the statistics come from the producer)
static void gn_label(Op& o) {
    static const char* const names[] = {"gn_small", "gn_stats+gn_apply", "gn_apply(fused stats)", "gn_fold+gn_apply(fused stats)"};      // by GnKind
    snprintf(o.klabel, sizeof(o.klabel), "%s", names[gn_pick(o.gn).kind]);
}
void Engine::op_gn(const char* name, Act X, Act Y, int B, int HW, const NormW& n, float eps, bool silu, const GnEdit& edit) {
    Op& o = emit(OP_GN, name);
    GroupNormArgs& g = o.gn;
    g.X = ptr(X); g.ldx = X.ld; g.Y = ptr(Y); g.ldy = Y.ld; g.B = B; g.HW = HW; g.C = n.C; g.G = 32; g.eps = eps; g.silu = silu;
    g.gamma = n.g; g.beta = n.b; g.partial = (float*)(cur.arena ? (char*)cur.arena + cur.gn_ws_off : nullptr);
    edit(o);
    o.bytes = 2.0 * 3.0 * (double)g.B * g.HW * g.C;       // read (stats) + read + write (apply)
    gn_label(o);
}
// SURVEY §8 a10-a11 / VERDICT r2 item 1c: GroupNorm statistics from the producing conv / GEMM epilogue.  A GroupNorm whose input tensor was written by
// the op right before it (so nothing else touches the shared statistics workspace in between) and whose producer launch can do it
// (gemm_gn_fuse: no split-K, tile width a multiple of the group width, tiles inside one image) drops its statistics pass — one full read
// of the activation and one launch.  The sums are still deterministic (fixed order per tile, then per tile row); what is given up is the
// bit-for-bit equality between different BATCH SIZES (the producer's tile shape, hence the summation order, depends on M).
void Engine::fuse_gn_stats() {
    for (size_t i = 1; i < cur.ops.size(); ++i) {
        if (cur.ops[i].kind == OP_GN && cur.ops[i - 1].kind == OP_ROWGEMM) {          // row-block producer (proj_out + residual): statistics from its output stage
            RowGemmArgs& r = cur.ops[i - 1].rg;
            GroupNormArgs& n = cur.ops[i].gn;
            if (r.Y != n.X || r.ldy != n.ldx || r.N != n.C || (long)r.M != (long)n.B * n.HW) continue;
            const int nchunk = rowgemm_gn_chunks(r, n.HW, n.G, gn_ws_rows);      // (xf_pick.cpp: whole row blocks per image, not the one-launch small GroupNorm, ...)
            if (!nchunk) continue;
            r.gn_out = n.partial; r.gn_nchunk = nchunk; r.HW = n.HW;
            n.stats_chunks = nchunk;
            cur.ops[i].bytes = 2.0 * 2.0 * (double)n.B * n.HW * n.C;
            gn_label(cur.ops[i]);
            continue;
        }
        if (cur.ops[i].kind != OP_GN || cur.ops[i - 1].kind != OP_GEMM) continue;
        GemmArgs& g = cur.ops[i - 1].g;
        GroupNormArgs& n = cur.ops[i].gn;
        if (g.C != n.X || g.ldc != n.ldx || g.N != n.C || (long)g.M != (long)n.B * n.HW) continue;
        const int nchunk = gemm_gn_fuse(g, n.HW, n.G, gn_ws_rows);
        if (!nchunk) continue;
        g.gn_partial = n.partial;
        n.stats_chunks = nchunk;
        cur.ops[i].bytes = 2.0 * 2.0 * (double)n.B * n.HW * n.C;       // read + write (apply only)
        gn_label(cur.ops[i]);
    }
}
// Row-block GEMM (rowgemm.hip) in place of [LayerNorm +] an N = k K, K = 320 / 640 projection, where xf_pick says so
void Engine::op_rowgemm(const char* name, Act X, const LinearW& w, Act Y, Act R, int pro, const NormW* nw) {
    Op& o = emit(OP_ROWGEMM, name);
    RowGemmArgs& a = o.rg;
    a.X = ptr(X); a.ldx = X.ld; a.Y = ptr(Y); a.ldy = Y.ld; a.M = X.rows; a.N = w.N; a.K = w.K; a.W = w.w; a.bias = w.b;
    a.R = R.valid ? ptr(R) : nullptr; a.ldr = R.ld; a.pro = pro; a.eps = 1e-5f;
    if (nw) { a.g = nw->g; a.b = nw->b; }
    o.flops = 2.0 * a.M * (double)a.N * a.K;
    o.bytes = 2.0 * ((double)a.M * a.K + (double)a.N * a.K + (double)a.M * a.N * (R.valid ? 2 : 1));
    snprintf(o.klabel, sizeof(o.klabel), "rowgemm<%s,%d>", dt_name(), pro);
    cur.flops += o.flops;
}
// SpatialTransformer norm + proj_in, as emit_xf emitted them, become one rowgemm launch with the GroupNorm apply as its prologue where xf_proj_in_rowgemm says so.
// Runs after fuse_gn_stats() (the statistics must come from norm's producer) and after the hand-over of a shared prefix (a proj_in that also stores the second
// half's rows stays a GEMM).
void Engine::fuse_gn_rowgemm() {
    for (size_t i = 0; i + 1 < cur.ops.size(); ++i) {
        if (cur.ops[i].kind != OP_GN || cur.ops[i + 1].kind != OP_GEMM || strcmp(cur.ops[i].name, "xf.norm") || strcmp(cur.ops[i + 1].name, "xf.proj_in")) continue;
        const GroupNormArgs& n = cur.ops[i].gn;
        const GemmArgs& g = cur.ops[i + 1].g;
        if (n.silu || g.dup_rows || !xf_proj_in_rowgemm(n.C, g.M, n.HW, i < cur.prefix_end, n.stats_chunks)) continue;
        Op o{}; o.kind = OP_ROWGEMM; o.name = cur.ops[i + 1].name;
        RowGemmArgs& a = o.rg;
        a.X = n.X; a.ldx = n.ldx; a.Y = g.C; a.ldy = g.ldc; a.M = g.M; a.N = g.N; a.K = g.K; a.W = g.W; a.bias = g.bias; a.R = g.R; a.ldr = g.ldr;
        a.pro = 2; a.g = n.gamma; a.b = n.beta; a.eps = n.eps; a.partial = n.partial; a.nchunk = n.stats_chunks; a.HW = n.HW; a.G = n.G;
        o.flops = cur.ops[i + 1].flops; o.bytes = cur.ops[i + 1].bytes;
        snprintf(o.klabel, sizeof(o.klabel), "rowgemm<%s,2>", dt_name());
        cur.ops[i] = o;
        cur.ops.erase(cur.ops.begin() + (long)i + 1);
        if (i + 1 < cur.prefix_end) --cur.prefix_end;
    }
}
void Engine::op_ln(const char* name, Act X, Act Y, const NormW& n, const LnEdit& edit) {
    Op& o = emit(OP_LN, name);
    LayerNormArgs& l = o.ln;
    l.X = ptr(X); l.ldx = X.ld; l.Y = ptr(Y); l.ldy = Y.ld; l.rows = X.rows; l.C = n.C; l.eps = 1e-5f; l.gamma = n.g; l.beta = n.b;
    edit(o);
    o.bytes = 2.0 * 2.0 * (double)l.rows * l.C;
    snprintf(o.klabel, sizeof(o.klabel), "ln_kernel");
}
void Engine::op_attn(const char* name, const void* Q, int ldq, const void* K, int ldk, const void* V, int ldv, Act O, int B, int H, int Nq, int Mk, int D, const AttnEdit& edit) {
    Op& o = emit(OP_ATTN, name);
    AttnArgs& a = o.at = attn_args(Q, ldq, K, ldk, V, ldv, ptr(O), O.ld, B, H, Nq, Mk, D, 1.0f / std::sqrt((float)D));
    edit(o);
    const AttnPick p = attn_attach_scratch(a, scratch);      // key-block norms of the pipelined kernels, partials of attn512's key splits (the VAE): live for this op only
    o.flops = 4.0 * B * H * (double)Nq * Mk * D;
    o.bytes = 2.0 * (double)B * H * D * (2.0 * Nq + 2.0 * Mk);
    {
        // the device kernel's own name with its template arguments (rocprofv3 reports the same), then self / cross or attn512's key splits
        static const char* const fmt[] = {"attn_kernel<%s,%d,%d,%d>", "attn32_kernel<%s,%d,144,192,%d>", "attn32ap_kernel<%s,144,192,%d>", "attn32g_kernel<%s,%d,%d,1,%d,%d>",
                                          "attn40p_kernel<%s>", "attn128p_kernel<%s>", "attn512_kernel<%s>"};      // by AttnFamily
        const int n = snprintf(o.klabel, sizeof(o.klabel), fmt[p.family], dt_name(), p.targ[0], p.targ[1], p.targ[2], (int)p.kpf);
        if (p.family == AF_ATTN512) snprintf(o.klabel + n, sizeof(o.klabel) - n, "x%d", a.nsplit);
        else snprintf(o.klabel + n, sizeof(o.klabel) - n, "%s", Nq == Mk ? "self" : "cross");
    }
    cur.flops += o.flops;
}

Act Engine::new_act(int rows, int C) {
    Act a; a.valid = true; a.owned = true; a.rows = rows; a.C = C; a.ld = C; a.col = 0;
    a.off = a_alloc((size_t)rows * C * 2);
    return a;
}
Act Engine::view(const Act& base, int col, int C) {
    Act a = base; a.owned = false; a.col = base.col + col; a.C = C; return a;
}
void Engine::release(const Act& a) { if (a.valid && a.owned) a_free(a.off); }

// ResBlock1._forward (ResBlock.py:315-335)
void Engine::emit_res(const ResW& r, Act X, Act OUT, int B, int H, int W, const float* emb, int emb_ld) {
    const int M = B * H * W;
    Act t1 = new_act(M, r.Cin);
    op_gn("res.gn1", X, t1, B, H * W, r.gn1, r.eps, true);
    Act t2 = new_act(M, r.Cout);
    op_conv("res.conv1", t1, B, H, W, r.Cin, r.conv1, 1, H, W, t2, Act{}, r.has_emb && emb ? emb + r.emb_off : nullptr, r.has_emb ? emb_ld : 0);
    release(t1);
    Act t3 = new_act(M, r.Cout);
    op_gn("res.gn2", t2, t3, B, H * W, r.gn2, r.eps, true);
    release(t2);
    if (r.has_skip && r.fused_skip) {
        op_conv("res.conv2+skip", t3, B, H, W, r.Cout, r.conv2, 1, H, W, OUT, Act{}, nullptr, 0, nullptr, 0, [&](GemmArgs& g) { g.A2 = ptr(X); g.lda2 = X.ld; g.Cin2 = r.Cin; });
    } else if (r.has_skip) {
        Act t4 = new_act(M, r.Cout);
        op_gemm("res.skip", X, r.skip, t4, Act{});
        op_conv("res.conv2", t3, B, H, W, r.Cout, r.conv2, 1, H, W, OUT, t4);
        release(t4);
    } else {
        op_conv("res.conv2", t3, B, H, W, r.Cout, r.conv2, 1, H, W, OUT, X);
    }
    release(t3);
}

double Engine::steady_flops() const {
    double f = cur.flops;
    if (ctx_cache) for (const Op& o : cur.ops) if (o.ctx_only) f -= o.flops;
    return f;
}
// the reference's arithmetic for the same evaluation: what runs plus what the shared CFG prefix computes once instead of twice
double Engine::algorithmic_flops() const { return steady_flops() + cur.flops_shared + cur.flops_up2x; }

void Plan::release() {
    if (arena) (void)hipFree(arena);
    arena = nullptr;
    graph.release();
}

int Engine::build_plan(const PlanKey& key, const std::function<int()>& emit, bool zero_arena) {
    auto reset = [&] {
        free_list.clear(); live.clear(); arena_top = 0; arena_peak = 0;
        cur.ops.clear(); cur.flops = 0; cur.flops_shared = 0; cur.flops_up2x = 0; cur.prefix_end = 0;
        plan_rc = LDX_OK;
    };
    cur.key = PlanKey{};                  // no plan until the bound pass has completed
    reset();
    void* const arena = cur.arena;
    cur.arena = nullptr;
    int rc = emit();
    cur.arena = arena;
    if (!rc) rc = plan_rc;                // an emitter's own finding (seal_gemm)
    if (rc) return rc;
    cur.arena_peak_dry = arena_peak;
    if (cur.arena && cur.arena_cap < cur.arena_peak_dry) { HIP_OK(hipFree(cur.arena)); cur.arena = nullptr; cur.arena_cap = 0; }
    if (!cur.arena) { HIP_OK(hipMalloc(&cur.arena, cur.arena_peak_dry)); cur.arena_cap = cur.arena_peak_dry; }
    if (zero_arena) HIP_OK(hipMemset(cur.arena, 0, cur.arena_cap));
    reset();
    if ((rc = emit()) || (rc = plan_rc)) return rc;
    cur.key = key;
    cur.graph.reset();
    cur.kv_ptr = nullptr; cur.kv_epoch = 0;          // a fresh arena holds no projected context
    return LDX_OK;
}

// keep_plans (the UNet and Flux): the plans of other shapes stay in plan_cache; the other models re-plan into the current plan, whose arena is
// reused when it is large enough.
int Engine::select_plan(const PlanKey& key, hipStream_t st, const std::function<int()>& replan, bool* switched) {
    if (key == cur.key) return LDX_OK;
    HIP_OK(hipStreamSynchronize(st));
    if (switched) *switched = true;
    if (keep_plans) {
        if (cur.key.B > 0) plan_stash();
        if (plan_restore(key)) return LDX_OK;
    }
    return replan();
}

void Engine::plan_stash() {
    plan_cache.push_back(std::move(cur));
    cur = Plan{};
    // every cached plan keeps its own arena resident: bound the cache by count (4) AND by bytes (LDX_PLAN_CACHE_GIB, default 16 GiB of
    // stashed arenas — a Flux plan per prompt length, a 2048^2 VAE plan of several GiB ...); oldest first, the newest entry always stays
    const size_t cap_bytes = (size_t)(g_plan_sw.plan_cache_gib * (double)(1ull << 30));
    auto cached_bytes = [&]() { size_t n = 0; for (const Plan& p : plan_cache) n += p.arena_cap; return n; };
    while (plan_cache.size() > 4 || (plan_cache.size() > 1 && cached_bytes() > cap_bytes)) {
        plan_cache.front().release();
        plan_cache.erase(plan_cache.begin());
    }
}
bool Engine::plan_restore(const PlanKey& key) {
    for (size_t i = 0; i < plan_cache.size(); ++i) {
        if (plan_cache[i].key != key) continue;
        cur = std::move(plan_cache[i]);
        plan_cache.erase(plan_cache.begin() + (long)i);
        return true;
    }
    return false;
}

// The op's launcher on its argument struct.  A case at most copies the struct and fills in what belongs to the call (bind).
int Engine::launch_op(const Op& o, hipStream_t ls) {
    switch (o.kind) {
        case OP_PREP: {
            PrepArgs p = o.prep;
            p.x = bind.x; p.sigma = bind.s; p.scale_input = bind.den ? 1 : 0; p.t_in = bind.den ? bind.t : bind.s; p.xB = bind.xB;      // bind.t: indices from the caller (null: looked up from sigma on the device)
            p.cc = bind.cc; p.Cx = p.C - bind.ccn;
            launch_prep(p, dt, ls);
        } break;
        case OP_FINISH: { FinishArgs f = o.fin; f.x = bind.den ? bind.x : nullptr; f.sigma = bind.s; f.out = bind.out; f.xB = bind.xB; launch_finish(f, ls); } break;
        case OP_CVT: { CvtArgs a = o.cvt; a.in = bind.ctx; launch_f32_to_t(a, dt, ls); } break;
        case OP_CVT_OUT: { CvtOutArgs a = o.out; a.out = o.second_output ? bind.out2 : bind.out; if (a.out) launch_t_to_f32(a, dt, ls); } break;
        case OP_COPY_OUT: { CopyOutArgs a = o.copy; a.dst = bind.out; HIP_OK(launch_copy_out(a, ls)); } break;
        case OP_SKINNY: launch_skinny(o.sk, dt, ls); break;
        case OP_FX_SKINNY_Y: { SkinnyArgs a = o.sk; a.x = bind.y; launch_skinny(a, dt, ls); } break;
        case OP_GEMM: launch_gemm(o.g, dt, ls); break;
        case OP_GEMM2: launch_gemm2(o.g, o.g2, dt, ls); break;
        case OP_MXQ: launch_mx_quant(o.mq, dt, ls); break;
        case OP_ATTN_MX: launch_attn_mx(o.am, dt, ls); break;
        case OP_MXVT: launch_mx_vt_quant(o.vt, dt, ls); break;
        case OP_XATTN: launch_xattn_block(o.xa, dt, ls); break;
        case OP_FFBLOCK: launch_ff_block(o.fb, dt, ls); break;
        case OP_ROWGEMM: launch_rowgemm(o.rg, dt, ls); break;
        case OP_GN: launch_groupnorm(o.gn, dt, ls); break;
        case OP_LN: launch_layernorm(o.ln, dt, ls); break;
        case OP_ATTN: { AttnArgs a = o.at; if (o.bias_from_call) a.bias = bind.bias; launch_attention(a, dt, ls); } break;      // T5's relative-position table is the call's
        case OP_VAEPREP: { VaePrepArgs a = o.vprep; a.z = bind.x; launch_vae_prep(a, dt, ls); } break;
        case OP_PIXPREP: { PixelsPrepArgs a = o.pix; a.px = bind.x; launch_pixels_prep(a, dt, ls); } break;
        case OP_SOFTMAX: launch_softmax_rows(o.sm, dt, ls); break;
        case OP_CLAMP: { ClampArgs a = o.clamp; a.out = bind.out; launch_clamp01(a, ls); } break;
        case OP_MOMENTS: { MixArgs a = o.mix; a.out = bind.out; launch_mix_nhwc_to_nchw(a, ls); } break;
        case OP_EMBED: { ClipEmbedArgs a = o.emb; a.ids = bind.ids; a.extra = bind.extra; a.n_extra = bind.n_extra; launch_clip_embed(a, dt, ls); } break;      // the textual-inversion rows change between calls
        case OP_DUP: launch_dup_rows(o.dup, dt, ls); break;
        case OP_TAESD_PREP: { TaesdPrepArgs a = o.tprep; a.z = bind.x; launch_taesd_prep(a, dt, ls); } break;
        case OP_TAESD_CONV: { TaesdConvArgs a = o.tconv; if (a.out3) { a.out_f32 = bind.out; a.out_u8 = bind.out8; a.flux = bind.flux; } launch_taesd_conv(a, dt, ls); } break;
        case OP_SAM_PATCH: { SamPatchArgs a = o.spatch; a.img = bind.x; launch_sam_patch(a, dt, ls); } break;
        case OP_SAM_WINDOW: launch_sam_window(o.swin, dt, ls); break;
        case OP_SAM_RELPOS: launch_sam_relpos(o.srel, dt, ls); break;
        case OP_SAM_ATTN: launch_sam_attention(o.sattn, dt, ls); break;
        case OP_SAM_ROWVEC: launch_sam_rowvec(o.srv, dt, ls); break;
        case OP_SAM_OUT: { SamOutArgs a = o.sout; a.out = bind.out; launch_sam_out(a, dt, ls); } break;
        case OP_FX_TEMB: { FluxTembArgs a = o.temb; a.t = o.of_guidance ? bind.guid : bind.s; launch_flux_temb(a, ls); } break;
        case OP_FX_SILU: launch_silu_f32(o.silu, ls); break;
        case OP_FX_PATCH: { FluxPatchArgs a = o.patch; a.x = bind.x; launch_flux_patchify(a, dt, ls); } break;
        case OP_FX_ROPE: { QkRopeArgs a = o.rp; const int hp = a.D / 2; a.cosT = bind.pe_cos + (size_t)o.tok0 * hp; a.sinT = bind.pe_sin + (size_t)o.tok0 * hp;
                           if (a.Q8) launch_qk_norm_rope_mx(a, dt, ls); else launch_qk_norm_rope(a, dt, ls); } break;
        case OP_FX_UNPATCH: { FluxUnpatchArgs a = o.unpatch; a.x = bind.den ? bind.x : nullptr; a.sigma = bind.s; a.out = bind.out; launch_flux_unpatchify(a, ls); } break;
    }
    return LDX_OK;
}

// LDX_DEBUG_NAN: after every GEMM with a 16-bit output, scan it on the host and report NaN / Inf (synchronises: never inside a stream capture)
static void debug_scan_nan(const Op& o, size_t oi, DType dt, hipStream_t ls) {
    (void)hipStreamSynchronize(ls);
    const int Nout = o.g.geglu ? o.g.N / 2 : o.g.N;
    std::vector<uint16_t> hb((size_t)o.g.M * o.g.ldc);
    (void)hipMemcpy(hb.data(), o.g.C, ((size_t)(o.g.M - 1) * o.g.ldc + Nout) * 2, hipMemcpyDeviceToHost);
    long bad = 0, first = -1;
    for (long m = 0; m < o.g.M; ++m) for (int n = 0; n < Nout; ++n) {
        const uint16_t v = hb[(size_t)m * o.g.ldc + n];
        const bool b = dt == DT_BF16 ? ((v & 0x7f80) == 0x7f80) : ((v & 0x7c00) == 0x7c00);
        if (b) { ++bad; if (first < 0) first = m * (long)Nout + n; }
    }
    fprintf(stderr, "[nan] op %zu %-14s M%d N%d K%d sk%d ln%d rs%d: %ld bad%s\n", oi, o.name, o.g.M, o.g.N, o.g.K, o.g.splitk, o.g.ln_c1 ? 1 : 0,
            0, bad, bad ? (std::string(" first at row ") + std::to_string(first / Nout) + " col " + std::to_string(first % Nout)).c_str() : "");
}

std::string Engine::prof_key(const Op& o) const {
    std::string key = o.klabel[0] ? o.klabel : o.name;
    if (!prof_detail) return key;
    char sh[96] = "";
    if (o.kind == OP_GEMM) snprintf(sh, sizeof(sh), " M%d N%d K%d sk%d%s", o.g.M, o.g.N, o.g.K, o.g.splitk, o.g.geglu ? " geglu" : o.g.up2x ? " up2x" : "");
    else if (o.kind == OP_ATTN) snprintf(sh, sizeof(sh), " B%d H%d N%d M%d D%d", o.at.B, o.at.H, o.at.Nq, o.at.Mk, o.at.D);
    else if (o.kind == OP_ATTN_MX) snprintf(sh, sizeof(sh), " B%d H%d N%d M%d D128", o.am.B, o.am.H, o.am.Nq, o.am.Mk);
    else if (o.kind == OP_GN) snprintf(sh, sizeof(sh), " B%d HW%d C%d", o.gn.B, o.gn.HW, o.gn.C);
    else if (o.kind == OP_ROWGEMM) snprintf(sh, sizeof(sh), " M%ld N%d K%d", o.rg.M, o.rg.N, o.rg.K);
    else if (o.kind == OP_XATTN) snprintf(sh, sizeof(sh), " M%ld C%d", (long)o.xa.M, o.xa.C);
    else if (o.kind == OP_FFBLOCK) snprintf(sh, sizeof(sh), " M%ld C%d", (long)o.fb.M, o.fb.C);
    else if (o.kind == OP_LN) snprintf(sh, sizeof(sh), " R%d C%d", o.ln.rows, o.ln.C);
    else if (o.kind == OP_MXQ) snprintf(sh, sizeof(sh), " R%d K%d", o.mq.rows, o.mq.K);
    else if (o.kind == OP_SAM_ATTN) snprintf(sh, sizeof(sh), " B%d H%d n%d", o.sattn.BW, o.sattn.H, o.sattn.n);
    else if (o.kind == OP_GEMM2) snprintf(sh, sizeof(sh), " M%d+%d N%d K%d", o.g.M, o.g2.M, o.g.N, o.g.K);
    return key + sh;
}

int Engine::exec_ops(hipStream_t ls, size_t op_begin, size_t op_end, int ctx_sel) {
    if (op_end > cur.ops.size()) op_end = cur.ops.size();
    const bool dbg_nan = g_launch_sw.debug_nan;          // debug: first GEMM whose 16-bit output holds a NaN / Inf
    const bool prof_now = profiling && !prof_graph;
    if (prof_now && prof_events.size() < 2 * cur.ops.size()) {
        const size_t old = prof_events.size();
        prof_events.resize(2 * cur.ops.size());
        for (size_t i = old; i < prof_events.size(); ++i) HIP_OK(hipEventCreate(&prof_events[i]));
    }
    auto skipped = [&](const Op& o) { return (ctx_sel == 1 && o.ctx_only) || (ctx_sel == 2 && !o.ctx_only); };
    for (size_t oi = op_begin; oi < op_end; ++oi) {
        const Op& o = cur.ops[oi];
        if (skipped(o)) continue;
        if (prof_now) HIP_OK(hipEventRecord(prof_events[2 * oi], ls));
        if (int rc = launch_op(o, ls)) return rc;
        if (dbg_nan && o.kind == OP_GEMM && o.g.C && !prof_graph) debug_scan_nan(o, oi, dt, ls);
        if (prof_now) HIP_OK(hipEventRecord(prof_events[2 * oi + 1], ls));
    }
    if (prof_now) {
        HIP_OK(hipStreamSynchronize(ls));
        for (size_t i = op_begin; i < op_end; ++i) {
            const Op& o = cur.ops[i];
            if (skipped(o)) continue;
            float ms = 0.f;
            HIP_OK(hipEventElapsedTime(&ms, prof_events[2 * i], prof_events[2 * i + 1]));
            ProfEntry& pe = prof[prof_key(o)];
            pe.count += 1; pe.ms += ms; pe.flops += o.flops; pe.bytes += o.bytes;
        }
    }
    return LDX_OK;
}

int Engine::run_planned(const PlanKey& key, const std::function<int()>& replan, const Bindings& b, hipStream_t st) {
    if (int rc = select_plan(key, st, replan)) return rc;
    bind = b;
    return run_bound(st);
}

// The current plan on this call's bindings.  A captured graph has the call's pointers and flags baked in, so it is replayed only for the bindings it was
// captured with: once a call arrives with others (in ANY mode: the eager path records them in graph.b) that graph is never replayed again (round 3: a
// stale graph was replayed after an eager call had moved the pointers).  A plan is captured only once the same (plan, bindings) have run eagerly: that
// pass also makes the one-time hipFuncSetAttribute calls, which are illegal during capture.
int Engine::run_bound(hipStream_t st, int ctx_sel) {
    Plan::Graph& g = cur.graph;
    const bool graphs = captures && graph_mode, same = g.b == bind;
    if (!same) g.valid = false;
    if (graphs && g.valid) {
        HIP_OK(hipGraphLaunch(g.exec, st));
        ++n_graph_replays;
        return LDX_OK;
    }
    const bool capture = graphs && g.warm && same;
    g.b = bind; g.warm = true;
    prof_graph = capture;
    if (!capture) {
        if (int rc = exec_ops(st, 0, (size_t)-1, ctx_sel)) return rc;
        return launch_status();
    }
    g.release();
    if (!cap_stream) HIP_OK(hipStreamCreateWithFlags(&cap_stream, hipStreamNonBlocking));
    HIP_OK(hipStreamSynchronize(st));
    HIP_OK(hipStreamBeginCapture(cap_stream, hipStreamCaptureModeThreadLocal));
    // From here every way out ends the capture and destroys the graph it got; the executable is kept, valid and counted only once its first launch has
    // succeeded.  After a failure the plan is as after an eager call: the next call with these bindings captures again.
    int rc = exec_ops(cap_stream, 0, (size_t)-1, ctx_sel);
    hipGraph_t graph = nullptr;
    const char* what = "hipStreamEndCapture";
    hipError_t err = hipStreamEndCapture(cap_stream, &graph);
    if (!rc && err == hipSuccess) { what = "hipGraphInstantiate"; err = hipGraphInstantiate(&g.exec, graph, nullptr, nullptr, 0); }
    if (graph) (void)hipGraphDestroy(graph);
    if (!rc && err == hipSuccess) { what = "hipGraphLaunch"; err = hipGraphLaunch(g.exec, st); }
    if (!rc && err != hipSuccess) { set_error(std::string(what) + ": " + hipGetErrorString(err)); rc = LDX_EHIP; }
    if (rc) { g.release(); return rc; }
    g.valid = true;
    ++n_graph_captures;
    return launch_status();
}

std::string Engine::profile_json() const {
    std::string s = "{";
    bool first = true;
    char buf[256];
    for (auto& kv : prof) {
        snprintf(buf, sizeof(buf), "%s\"%s\": {\"count\": %ld, \"ms\": %.6f, \"flops\": %.6e, \"bytes\": %.6e}", first ? "" : ", ",
                 kv.first.c_str(), kv.second.count, kv.second.ms, kv.second.flops, kv.second.bytes);
        s += buf; first = false;
    }
    return s + "}";
}

int64_t Engine::n_launches() const {
    int64_t n = 0;
    for (const Op& o : cur.ops) {
        if (ctx_cache && o.ctx_only) continue;            // steady state of a sampling run: the context's projections are cached
        if (o.kind == OP_GN) n += gn_pick(o.gn).launches;          // one for the small kernel and for apply-only, two with a statistics or fold launch
        else if (o.kind == OP_GEMM) n += gemm_pick(o.g).launches;          // with its split-K reduce launch, if it has one
        else if (o.kind == OP_GEMM2) n += gemm_pick(o.g, &o.g2).launches;
        else if (o.kind == OP_ATTN) n += attn_pick(o.at).launches;      // with the pipelined kernels' key-norm launch / attn512's merge launch
        else n += 1;
    }
    return n;
}

}  // namespace ldx
