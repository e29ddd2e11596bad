// ldx UNet engine: host-side planner / executor behind the C ABI (include/ldx.h).
//
// Mirrors, for the accelerated path only, what the reference spreads over
//   UNetModel1.__init__/forward          src/NeuralNetwork/unet.py:208-770
//   ResBlock1 / Downsample1 / Upsample1  src/AutoEncoders/ResBlock.py:75-335
//   SpatialTransformer / BasicTransformerBlock / FeedForward   src/NeuralNetwork/transformer.py:19-377
//   CrossAttention                       src/Attention/Attention.py:53-124
//   BaseModel.apply_model                src/Model/ModelBase.py:72-133
// but as a static launch plan over one activation arena: weights are packed once into MFMA-friendly
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
Engine::Engine(const ldx_unet_config& c, int dev) : cfg(c), device(dev) {
    dt = (c.compute_dtype == LDX_F16) ? DT_F16 : DT_BF16;
    cfg_share = getenv("LDX_CFG_SHARE") ? atoi(getenv("LDX_CFG_SHARE")) : 1;      // 0 off, 1 where it pays (share_for), 2 whenever possible
}
Engine::~Engine() {
    (void)hipSetDevice(device);
    for (void* p : dev_allocs) (void)hipFree(p);
    if (d_sigma_cfg) (void)hipFree(d_sigma_cfg);
    cur.release();
    for (Plan& p : plan_cache) p.release();
    for (hipEvent_t ev : prof_events) (void)hipEventDestroy(ev);
    if (cap_stream) (void)hipStreamDestroy(cap_stream);
}

int Engine::validate() const {
    auto bad = [&](const char* m) { set_error(std::string("unsupported UNet config: ") + m); return LDX_EINVAL; };
    if (cfg.model_channels <= 0 || cfg.model_channels % 64) return bad("model_channels must be a multiple of 64");
    if (cfg.context_dim <= 0 || cfg.context_dim % 64) return bad("context_dim must be a multiple of 64");
    // these two (every level's channels = model_channels * channel_mult) are also what the pack kernels' 16-byte stores need (Engine::pack16)
    if (cfg.num_levels < 1 || cfg.num_levels > 8) return bad("num_levels out of range");
    if (cfg.num_heads < 1) return bad("num_heads");
    if (cfg.in_channels < 1 || cfg.in_channels > 64 || cfg.out_channels < 1 || cfg.out_channels > 128) return bad("in/out channels");
    for (int l = 0; l < cfg.num_levels; ++l) {
        const int ch = cfg.model_channels * cfg.channel_mult[l];
        if (ch % cfg.num_heads || (ch / cfg.num_heads) % 8 || ch / cfg.num_heads > 160) return bad("head dim must be a multiple of 8 and <= 160");
        if (ch % 32) return bad("channels not divisible by 32 groups");
    }
    return LDX_OK;
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

int Engine::load_tensor_device(const char* key, const void* dev_ptr, int dtype, const int64_t* shape, int ndim) {
    if (kind != KIND_UNET) { set_error("ldx_load_tensor_device: UNet engines only"); return LDX_ESTATE; }
    if (finalized && !refreshing) { set_error("ldx_load_tensor_device after ldx_finalize"); return LDX_ESTATE; }
    if (!key || !dev_ptr || ndim < 0 || ndim > 8 || (ndim && !shape)) { set_error("ldx_load_tensor_device: bad argument"); return LDX_EINVAL; }
    if (dtype != LDX_F32 && dtype != LDX_F16 && dtype != LDX_BF16) { set_error("ldx_load_tensor_device: bad dtype"); return LDX_EINVAL; }
    if ((uintptr_t)dev_ptr % (dtype == LDX_F32 ? 4 : 2)) { set_error("ldx_load_tensor_device: misaligned pointer"); return LDX_EINVAL; }
    HostTensor t;
    t.dtype = dtype;
    t.numel = 1;
    for (int i = 0; i < ndim; ++i) {
        if (shape[i] < 0) { set_error("ldx_load_tensor_device: negative extent"); return LDX_EINVAL; }
        t.shape.push_back(shape[i]); t.numel *= (size_t)shape[i];
    }
    t.dev = dev_ptr;
    host[key] = std::move(t);
    return LDX_OK;
}

int Engine::set_tables(const float* ls, int n, const float* temb, int dim) {
    // after finalize the per-timestep emb_layers table (build_emb_table) and every cached plan depend on these tables
    if (finalized) { set_error("ldx_set_tables after ldx_finalize"); return LDX_ESTATE; }
    if (!ls || !temb || n <= 0 || dim != cfg.model_channels) { set_error("ldx_set_tables: bad argument (temb_dim must equal model_channels)"); return LDX_EINVAL; }
    HIP_OK(hipSetDevice(device));
    void* p = nullptr;
    HIP_OK(hipMalloc(&p, (size_t)n * 4)); dev_allocs.push_back(p);
    HIP_OK(hipMemcpy(p, ls, (size_t)n * 4, hipMemcpyHostToDevice));
    d_log_sigmas = (float*)p; n_sigmas = n;
    HIP_OK(hipMalloc(&p, (size_t)n * dim * 4)); dev_allocs.push_back(p);
    HIP_OK(hipMemcpy(p, temb, (size_t)n * dim * 4, hipMemcpyHostToDevice));
    d_temb = (float*)p;
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

// the next weight buffer of the structure walk: a new allocation (ALLOC) or the one the same step of finalize()'s walk made (CHECK / REFILL)
void* Engine::weight_buf(size_t bytes) {
    if (walk_mode == WALK_ALLOC) {
        void* p = nullptr;
        if (hipMalloc(&p, bytes) != hipSuccess) return nullptr;
        dev_allocs.push_back(p);
        if (kind == KIND_UNET) weight_allocs.push_back({p, bytes});      // the other engines share the packers but have no refresh and no digest
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
}
void* Engine::pack16(size_t rows, size_t cols, const std::vector<Piece>& pieces) {
    void* p = weight_buf(rows * cols * 2);
    if (!p) return p;
    bool dev = false;
    for (const Piece& pc : pieces) dev = dev || pc.src->dev;
    for (const Piece& pc : pieces) {
        // The pieces must lie inside [rows][cols] and match their sources; the kernel's 16-byte stores need more, which validate() guarantees for every
        // UNet it accepts (all channel counts and context_dim are multiples of 64, conv_in is padded to 64).  Tested in every walk mode, so a refresh
        // reports it before anything is written.
        if (pc.row0 + pc.N > rows || pc.col0 + pc.K > cols || (dev && (pc.K % 8 || cols % 8 || pc.col0 % 8 || pc.CinPad % 8)) ||
            (pc.CinPad ? (pc.K != 9 * pc.CinPad || pc.Cin > pc.CinPad || pc.src->numel != (size_t)pc.N * pc.Cin * 9)
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
        if (pc.off + pc.n > n || pc.a->numel != (size_t)pc.n || (pc.b && pc.b->numel != (size_t)pc.n) || (pc.geglu_inner && pc.n != 2 * pc.geglu_inner)) {
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

static int stacked_rows(const std::vector<EmbSrc>& srcs) { int n = 0; for (const EmbSrc& s : srcs) n += s.n; return n; }
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

bool Engine::mk_res(const std::string& pre, int Cin, int Cout, ResW& r) {
    r.Cin = Cin; r.Cout = Cout;
    if (!mk_norm(pre + ".in_layers.0", Cin, r.gn1)) return false;
    if (!mk_conv3(pre + ".in_layers.2", Cout, Cin, Cin, r.conv1)) return false;
    // emb_layers.1 is batched with every other ResBlock's projection (one skinny GEMM per forward)
    const HostTensor* ew = get(pre + ".emb_layers.1.weight", {Cout, 4 * cfg.model_channels});
    const HostTensor* eb = get(pre + ".emb_layers.1.bias", {Cout});
    if (!ew || !eb) return false;
    r.emb_off = stacked_rows(emb_srcs);
    emb_srcs.push_back({ew, eb, Cout});
    if (!mk_norm(pre + ".out_layers.0", Cout, r.gn2)) return false;
    r.has_skip = Cin != Cout;
    if (r.has_skip && Cin % 64 == 0 && g_plan_sw.fused_skip) return mk_fused_skip(pre + ".out_layers.3", pre + ".skip_connection", Cin, Cout, r);
    if (!mk_conv3(pre + ".out_layers.3", Cout, Cout, Cout, r.conv2)) return false;
    return !r.has_skip || mk_linear(pre + ".skip_connection", Cout, Cin, true, r.skip, true);
}

static inline bool q_prescale() { return g_plan_sw.q_prescale; }

bool Engine::mk_xf(const std::string& pre, int C, int depth, XfW& x) {
    x.C = C; x.depth = depth;
    const int ctx = cfg.context_dim;
    if (!mk_norm(pre + ".norm", C, x.gn)) return false;
    if (!mk_linear(pre + ".proj_in", C, C, true, x.proj_in, true)) return false;
    if (!mk_linear(pre + ".proj_out", C, C, true, x.proj_out, true)) return false;
    x.blocks.resize(depth);
    for (int d = 0; d < depth; ++d) {
        XfBlockW& b = x.blocks[d];
        const std::string bp = pre + ".transformer_blocks." + std::to_string(d);
        if (!mk_norm(bp + ".norm1", C, b.ln1) || !mk_norm(bp + ".norm2", C, b.ln2) || !mk_norm(bp + ".norm3", C, b.ln3)) return false;
        // fused q|k|v for self attention
        const HostTensor* q = get(bp + ".attn1.to_q.weight", {C, C});
        const HostTensor* k = get(bp + ".attn1.to_k.weight", {C, C});
        const HostTensor* v = get(bp + ".attn1.to_v.weight", {C, C});
        if (!q || !k || !v) return false;
        // LDX_LNFOLD=1: fold norm1/2/3 into the q|k|v / q / GEGLU projections (48 launches and the normalised copies of h less per step).
        // Correct and tested, but measured neutral on MI355X (17.26 vs 17.14 ms per step): with every part of the fold switched off the
        // consuming GEMM is still 16 us slower at level 0 when it follows the GEMM that wrote h than when a LayerNorm launch sits between
        // them (50 -> 66 us; the statistics MFMAs, the LDS exchange and the epilogue add 8 more) - profiles/ubench/README.md.  Off by default.
        // Round 4: it does pay where the row-block kernels are not taken (512^2 step 6.01 -> 5.87 ms) and loses where they are (1024^2: 14.31 -> 15.04 with
        // the fold everywhere), so both copies of the three weights are kept (+0.3 GB for SD1.5) and the planner decides per input shape
        // (emit_xf: LDX_LNFOLD_MAXROWS); LDX_LNFOLD=0: plain weights only.
        b.ln_fold = g_plan_sw.lnfold;
        // softmax_scale * log2(e) folded into the q projections at load time (one rounding of c * Wq instead of rounding q and multiplying
        // every score): the attention ops then run with scale = 1 / log2(e), i.e. exp2(q.k - m) as before; LDX_NO_QPRESCALE=1 keeps the plain weights
        const float cq = q_prescale() ? (1.0f / std::sqrt((float)(C / cfg.num_heads))) * 1.44269504088896340736f : 1.0f;
        const HostTensor* q2w = get(bp + ".attn2.to_q.weight", {C, C});
        if (!q2w) return false;
        const std::vector<Piece> qkv_p{rows_piece(q, 0, C, C, cq), rows_piece(k, C, C, C), rows_piece(v, (size_t)2 * C, C, C)}, q2_p{rows_piece(q2w, 0, C, C, cq)};
        if (b.ln_fold) {
            if (!mk_ln_folded(3 * C, C, qkv_p, nullptr, bp + ".norm1", b.qkv_f, b.c1_qkv)) return false;
            if (!mk_ln_folded(C, C, q2_p, nullptr, bp + ".norm2", b.q2_f, b.c1_q2)) return false;
        }
        b.qkv.N = 3 * C; b.qkv.K = C; b.qkv.b = nullptr;
        b.qkv.w = pack16((size_t)3 * C, C, qkv_p);
        b.q2.N = C; b.q2.K = C; b.q2.b = nullptr;
        b.q2.w = pack16(C, C, q2_p);
        if (!b.qkv.w || !b.q2.w) return false;
        if (!mk_linear(bp + ".attn1.to_out.0", C, C, true, b.o1)) return false;
        const HostTensor* k2 = get(bp + ".attn2.to_k.weight", {C, ctx});
        const HostTensor* v2 = get(bp + ".attn2.to_v.weight", {C, ctx});
        if (!k2 || !v2) return false;
        b.kv2.N = 2 * C; b.kv2.K = ctx; b.kv2.b = nullptr; b.kv2.w = nullptr;
        b.kv_off = stacked_rows(kv_srcs);          // columns [kv_off, kv_off + 2C) of the batched k|v projection
        kv_srcs.push_back({k2, nullptr, C}); kv_srcs.push_back({v2, nullptr, C});
        if (!mk_linear(bp + ".attn2.to_out.0", C, C, true, b.o2)) return false;
        // GEGLU projection: rows permuted so each 64-column slab holds 32 value rows then their 32 gate rows (geglu_src_row)
        const int inner = 4 * C;
        const HostTensor* fw = get(bp + ".ff.net.0.proj.weight", {2 * inner, C});
        const HostTensor* fb = get(bp + ".ff.net.0.proj.bias", {2 * inner});
        if (!fw || !fb) return false;
        const std::vector<Piece> ff1_p{rows_piece(fw, 0, 2 * inner, C, 1.0f, inner)};
        if (b.ln_fold && !mk_ln_folded(2 * inner, C, ff1_p, fb, bp + ".norm3", b.ff1_f, b.c1_ff1)) return false;
        b.ff1.N = 2 * inner; b.ff1.K = C;
        b.ff1.w = pack16((size_t)2 * inner, C, ff1_p);
        b.ff1.b = pack32((size_t)2 * inner, {{fb, nullptr, 0, 2 * inner, inner}});
        if (!b.ff1.w || !b.ff1.b) return false;
        if (!mk_linear(bp + ".ff.net.2", C, inner, true, b.ff2)) return false;
    }
    return true;
}

// The structure walk: every packed weight buffer of the UNet from the registered tensors, in one fixed order.  walk_mode says what a buffer is:
// a new allocation (finalize), nothing (refresh: keys and shapes only) or the allocation finalize made (refresh: refill).  Whatever the mode, the
// walk builds a fresh UNetW which, when it succeeds, holds the same pointers as the one before; only then does it replace `un`.
int Engine::walk_weights() {
    UNetW w;
    emb_srcs.clear(); kv_srcs.clear();
    missing.clear(); walk_err.clear(); walk_next = 0;
    const int mc = cfg.model_channels, ted = 4 * mc;
    bool ok = true;
    // --- structure walk, identical in order to UNetModel1.__init__ (unet.py:344-677) ---
    ok = ok && mk_linear("time_embed.0", ted, mc, true, w.te0) && mk_linear("time_embed.2", ted, ted, true, w.te2);
    ok = ok && mk_conv3("input_blocks.0.0", mc, cfg.in_channels, 64, w.conv_in);
    int ch = mc, td_i = 0, ib = 1;
    std::vector<int> chans{mc};
    for (int level = 0; ok && level < cfg.num_levels; ++level) {
        for (int nr = 0; ok && nr < cfg.num_res_blocks[level]; ++nr) {
            BlockW blk;
            const std::string pre = "input_blocks." + std::to_string(ib);
            const int co = cfg.channel_mult[level] * mc;
            blk.has_res = true;
            ok = ok && mk_res(pre + ".0", ch, co, blk.res);
            ch = co;
            const int depth = cfg.transformer_depth[td_i++];
            if (ok && depth > 0) { blk.has_xf = true; ok = mk_xf(pre + ".1", ch, depth, blk.xf); }
            w.in_blocks.push_back(std::move(blk)); chans.push_back(ch); ++ib;
        }
        if (ok && level != cfg.num_levels - 1) {
            BlockW blk; blk.has_down = true;
            ok = mk_conv3("input_blocks." + std::to_string(ib) + ".0.op", ch, ch, ch, blk.down);
            w.in_blocks.push_back(std::move(blk)); chans.push_back(ch); ++ib;
        }
    }
    if (ok && cfg.transformer_depth_middle >= -1) {
        w.has_middle = true;
        ok = mk_res("middle_block.0", ch, ch, w.mid_res0);
        if (ok && cfg.transformer_depth_middle >= 0) {
            w.mid_has_xf = true;
            ok = mk_xf("middle_block.1", ch, std::max(1, (int)cfg.transformer_depth_middle), w.mid_xf) && mk_res("middle_block.2", ch, ch, w.mid_res1);
            if (cfg.transformer_depth_middle == 0) { set_error("transformer_depth_middle == 0 unsupported"); return LDX_EINVAL; }
        }
    }
    int n_out = 0;
    for (int l = 0; l < cfg.num_levels; ++l) n_out += cfg.num_res_blocks[l] + 1;
    int td_o = n_out, ob = 0;
    for (int level = cfg.num_levels - 1; ok && level >= 0; --level) {
        for (int i = 0; ok && i <= cfg.num_res_blocks[level]; ++i) {
            BlockW blk;
            const std::string pre = "output_blocks." + std::to_string(ob);
            const int ich = chans.back(); chans.pop_back();
            const int co = mc * cfg.channel_mult[level];
            blk.has_res = true; blk.skip_ch = ich;
            ok = mk_res(pre + ".0", ch + ich, co, blk.res);
            ch = co;
            int sub = 1;
            const int depth = cfg.transformer_depth_output[--td_o];
            if (ok && depth > 0) { blk.has_xf = true; ok = mk_xf(pre + ".1", ch, depth, blk.xf); ++sub; }
            if (ok && level && i == cfg.num_res_blocks[level]) {
                blk.has_up = true;
                ok = mk_conv3(pre + "." + std::to_string(sub) + ".conv", ch, ch, ch, blk.up);
            }
            w.out_blocks.push_back(std::move(blk)); ++ob;
        }
    }
    ok = ok && mk_norm("out.0", ch, w.out_gn) && mk_conv3("out.2", cfg.out_channels, mc, mc, w.conv_out);
    ok = ok && mk_stacked(emb_srcs, ted, w.emb_all) && (kv_srcs.empty() || mk_stacked(kv_srcs, cfg.context_dim, w.kv_all));
    w.emb_total = w.emb_all.N; w.kv_total = w.kv_all.N;
    emb_srcs.clear(); kv_srcs.clear();
    if (ok && walk_mode != WALK_ALLOC && walk_next != weight_allocs.size()) { ok = false; walk_err = "the weight layout differs from the one ldx_finalize built (plan switches changed since?)"; }
    // the device packers run on the null stream, in order behind the host path's copies: one wait for all of them, then the staged copies can go
    hipError_t sync = ok && walk_mode != WALK_CHECK ? hipDeviceSynchronize() : hipSuccess;
    if (sync == hipSuccess && walk_mode != WALK_CHECK) sync = hipGetLastError();
    drop_staged();
    if (!ok) return weights_failed();
    if (sync != hipSuccess) { set_error(std::string("weight packing failed: ") + hipGetErrorString(sync)); return LDX_EHIP; }
    un = std::move(w);
    return LDX_OK;
}

int Engine::weights_failed() {
    if (!missing.empty()) { set_error("missing or mis-shaped weight: " + missing); return LDX_EMISSING; }
    if (!walk_err.empty()) { set_error(walk_err); return LDX_ESTATE; }
    set_error(std::string("weight upload failed: ") + hipGetErrorString(hipGetLastError()));
    return LDX_EHIP;
}

int Engine::finalize() {
    if (finalized) return LDX_OK;
    if (kind != KIND_UNET) { set_error("finalize(): wrong engine kind"); return LDX_ESTATE; }
    int rc = validate();
    if (rc) return rc;
    HIP_OK(hipSetDevice(device));
    if (!d_log_sigmas) { set_error("ldx_finalize: call ldx_set_tables first"); return LDX_ESTATE; }
    walk_mode = WALK_ALLOC;
    if ((rc = walk_weights())) return rc;
    host.clear();
    { const int rc2 = build_emb_table(); if (rc2) return rc2; }
    finalized = true;
    return LDX_OK;
}

int Engine::refresh_begin() {
    if (kind != KIND_UNET || !finalized) { set_error("ldx_unet_refresh_begin: not a finalized UNet engine"); return LDX_ESTATE; }
    host.clear();                          // a second begin starts over
    refreshing = true;
    return LDX_OK;
}

int Engine::refresh_abort() {
    if (kind != KIND_UNET || !finalized) { set_error("ldx_unet_refresh_abort: not a finalized UNet engine"); return LDX_ESTATE; }
    host.clear();
    refreshing = false;
    return LDX_OK;
}

int Engine::refresh_commit() {
    if (kind != KIND_UNET || !finalized || !refreshing) { set_error("ldx_unet_refresh_commit: call ldx_unet_refresh_begin first"); return LDX_ESTATE; }
    HIP_OK(hipSetDevice(device));
    HIP_OK(hipDeviceSynchronize());        // no forward still reads the buffers about to be rewritten
    // every key and shape first, with nothing written (a failing walk leaves `un` as it is)
    walk_mode = WALK_CHECK;
    int rc = walk_weights();
    if (rc == LDX_OK) {
        walk_mode = WALK_REFILL;
        rc = walk_weights();               // an error from here on (a HIP failure) leaves the weights partly rewritten
    }
    walk_mode = WALK_ALLOC;
    host.clear();
    refreshing = false;                    // either way the refresh is over: the engine holds the new weights, or (validation failed) still the old ones
    if (rc) return rc;
    ++ctx_epoch;                           // cached k|v projections of the context were made with the old weights
    return build_emb_table();
}

int Engine::weights_digest(uint64_t* out) {
    if (kind != KIND_UNET || !finalized) { set_error("ldx_weights_digest: not a finalized UNet engine"); return LDX_ESTATE; }
    if (!out) { set_error("ldx_weights_digest: bad argument"); return LDX_EINVAL; }
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

// Split-K workspace of one op: dead as soon as the op's reduce launch has run, so it is freed at once (the next buffer may reuse it).
size_t Engine::ws_alloc(size_t bytes) { const size_t off = a_alloc(bytes); a_free(off); return off; }

// ---- op emitters ---------------------------------------------------------------------------------
Op& Engine::emit(OpKind kind, const char* name) {
    cur.ops.emplace_back();
    Op& o = cur.ops.back();
    memset(&o, 0, sizeof(o)); o.kind = kind; o.name = name;
    return o;
}
void Engine::op_gemm(const char* name, Act A, const LinearW& w, Act C, Act R, bool geglu, const float* rowvec, int rv_ld, int rpb) {
    Op& o = emit(OP_GEMM, name);
    GemmArgs& g = o.g;
    g.A = ptr(A); g.lda = A.ld; g.W = w.w; g.M = A.rows; g.N = w.N; g.K = w.K; g.mode = 0;
    g.bias = w.b; g.rowvec = rowvec; g.rowvec_ld = rv_ld; g.rows_per_batch = rpb > 0 ? rpb : 1;
    g.geglu = geglu ? 1 : 0;
    g.R = R.valid ? ptr(R) : nullptr; g.ldr = R.ld;
    g.C = ptr(C); g.ldc = C.ld; g.Cf = nullptr;
    g.splitk = gemm_choose_splitk(g.M, g.N, g.K, geglu);
    if (g.splitk > 1) { g.ws = (float*)((uintptr_t)cur.arena + ws_alloc(gemm_sk_ws_floats(g.M, g.N, g.splitk) * 4)); g.sk_count = sk_counters(); }
    o.flops = 2.0 * g.M * (double)g.N * g.K;
    o.bytes = 2.0 * ((double)g.M * g.K + (double)g.N * g.K + (double)g.M * (geglu ? g.N / 2 : g.N) * (R.valid ? 2 : 1));
    snprintf(o.klabel, sizeof(o.klabel), "gemm_kernel<%s,0>", dt == DT_BF16 ? "bf16" : "f16");
    cur.flops += o.flops;
}
void Engine::op_conv(const char* name, Act X, int B, int Hin, int Win, int Cin, const LinearW& w, int stride, int Hout, int Wout,
                     Act Y, Act R, const float* rowvec, int rv_ld, float* Cf, int ldcf) {
    Op& o = emit(OP_GEMM, name);
    GemmArgs& g = o.g;
    g.A = ptr(X); g.lda = X.ld; g.W = w.w; g.M = B * Hout * Wout; g.N = w.N; g.K = w.K; g.mode = 1;
    g.Cin = Cin; g.Hin = Hin; g.Win = Win; g.Hout = Hout; g.Wout = Wout; g.stride = stride;
    if (stride == 1) { g.Hv = Hout; g.Wv = Wout; } else { g.Hv = Hin; g.Wv = Win; }
    g.resize = (g.Hv != Hin || g.Wv != Win) ? 1 : 0;
    g.bias = w.b; g.rowvec = rowvec; g.rowvec_ld = rv_ld; g.rows_per_batch = Hout * Wout;
    g.R = R.valid ? ptr(R) : nullptr; g.ldr = R.ld;
    g.C = Y.valid ? ptr(Y) : nullptr; g.ldc = Y.ld; g.Cf = Cf; g.ldcf = ldcf;
    g.splitk = gemm_choose_splitk(g.M, g.N, g.K, false);
    if (g.splitk > 1) { g.ws = (float*)((uintptr_t)cur.arena + ws_alloc(gemm_sk_ws_floats(g.M, g.N, g.splitk) * 4)); g.sk_count = sk_counters(); }
    o.flops = 2.0 * g.M * (double)g.N * g.K;
    o.bytes = 2.0 * ((double)B * Hin * Win * Cin + (double)g.N * g.K + (double)g.M * g.N * (R.valid ? 2 : 1));
    snprintf(o.klabel, sizeof(o.klabel), "gemm_kernel<%s,1>", dt == DT_BF16 ? "bf16" : "f16");
    cur.flops += o.flops;
}
// the kernels launch_groupnorm runs for the op as it stands (fuse_gn_stats asks again once the statistics come from the producer)
static void gn_label(Op& o) {
    static const char* const names[] = {"gn_small", "gn_stats+gn_apply", "gn_apply(fused stats)", "gn_fold+gn_apply(fused stats)"};      // by GnKind
    snprintf(o.klabel, sizeof(o.klabel), "%s", names[gn_pick(o.gn).kind]);
}
void Engine::op_gn(const char* name, Act X, Act Y, int B, int HW, const NormW& n, float eps, bool silu) {
    Op& o = emit(OP_GN, name);
    GroupNormArgs& g = o.gn;
    g.X = ptr(X); g.ldx = X.ld; g.Y = ptr(Y); g.ldy = Y.ld; g.B = B; g.HW = HW; g.C = n.C; g.G = 32; g.eps = eps; g.silu = silu;
    g.gamma = n.g; g.beta = n.b; g.partial = (float*)(cur.arena ? (char*)cur.arena + cur.gn_ws_off : nullptr);
    o.bytes = 2.0 * 3.0 * (double)B * HW * n.C;       // read (stats) + read + write (apply)
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
            const int bm = rowblock_rows(r.K);
            if (!gemm_gn_fuse_enabled() || r.pro == 2 || r.Y != n.X || r.ldy != n.ldx || r.N != n.C || r.N != r.K || n.G != 32 || (long)r.M != (long)n.B * n.HW || n.HW % bm || n.HW / bm > gn_ws_rows ||
                gn_uses_small_kernel(n.B, n.HW, n.C, n.G)) continue;      // last term: the one-launch small GroupNorm kernel takes it (norm.hip)
            r.gn_out = n.partial; r.gn_nchunk = n.HW / bm; r.HW = n.HW;
            n.stats_chunks = n.HW / bm;
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
    snprintf(o.klabel, sizeof(o.klabel), "rowgemm<%s,%d>", dt == DT_BF16 ? "bf16" : "f16", pro);
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
        snprintf(o.klabel, sizeof(o.klabel), "rowgemm<%s,2>", dt == DT_BF16 ? "bf16" : "f16");
        cur.ops[i] = o;
        cur.ops.erase(cur.ops.begin() + (long)i + 1);
        if (i + 1 < cur.prefix_end) --cur.prefix_end;
    }
}
void Engine::op_ln(const char* name, Act X, Act Y, const NormW& n) {
    Op& o = emit(OP_LN, name);
    LayerNormArgs& l = o.ln;
    l.X = ptr(X); l.ldx = X.ld; l.Y = ptr(Y); l.ldy = Y.ld; l.rows = X.rows; l.C = n.C; l.eps = 1e-5f; l.gamma = n.g; l.beta = n.b;
    o.bytes = 2.0 * 2.0 * (double)X.rows * n.C;
    snprintf(o.klabel, sizeof(o.klabel), "ln_kernel");
}
void Engine::op_attn(const char* name, const void* Q, int ldq, const void* K, int ldk, const void* V, int ldv, Act O, int B, int H, int Nq, int Mk, int D) {
    Op& o = emit(OP_ATTN, name);
    AttnArgs& a = o.at;
    a.Q = Q; a.ldq = ldq; a.K = K; a.ldk = ldk; a.V = V; a.ldv = ldv; a.O = ptr(O); a.ldo = O.ld;
    a.B = B; a.H = H; a.Nq = Nq; a.Mk = Mk; a.D = D; a.scale = 1.0f / std::sqrt((float)D); a.causal = 0;
    if (attn_pipe_ok(a)) {       // key-block norms for the pipelined kernels' score bound (attn_pipe.hip): a few KiB, live for this op only
        const size_t off = a_alloc((size_t)B * H * ((Mk + 63) / 64) * 4); a.knorm_ws = (float*)((uintptr_t)cur.arena + off); a_free(off);
    }
    const AttnPick p = attn_pick(a);
    if (p.nsplit_want > 1) {          // D = 512 (VAE): key splits when the query blocks alone leave CUs idle; fp32 partials live for this op only
        a.nsplit = p.nsplit_want;
        const size_t off = a_alloc(attn512_ws_floats(a, a.nsplit) * 4); a.split_ws = (float*)((uintptr_t)cur.arena + off); a_free(off);
    }
    o.flops = 4.0 * B * H * (double)Nq * Mk * D;
    o.bytes = 2.0 * (double)B * H * D * (2.0 * Nq + 2.0 * Mk);
    {
        // the device kernel's own name with its template arguments (rocprofv3 reports the same), then self / cross or attn512's key splits
        static const char* const fmt[] = {"attn_kernel<%s,%d,%d,%d>", "attn32_kernel<%s,%d,144,192,%d>", "attn32ap_kernel<%s,144,192,%d>", "attn32g_kernel<%s,%d,%d,1,%d,%d>",
                                          "attn40p_kernel<%s>", "attn128p_kernel<%s>", "attn512_kernel<%s>"};      // by AttnFamily
        const int n = snprintf(o.klabel, sizeof(o.klabel), fmt[p.family], dt == DT_BF16 ? "bf16" : "f16", p.targ[0], p.targ[1], p.targ[2], (int)p.kpf);
        if (p.family == AF_ATTN512) snprintf(o.klabel + n, sizeof(o.klabel) - n, "x%d", a.nsplit);
        else snprintf(o.klabel + n, sizeof(o.klabel) - n, "%s", Nq == Mk ? "self" : "cross");
    }
    cur.flops += o.flops;
}

// rows [0, rows) of the view -> rows [rows, 2 * rows): the second half of a CFG batch takes over what was computed once for both (plan(): share)
void Engine::op_dup(const Act& a, int rows) {
    Op& o = emit(OP_DUP, "cfg.dup");
    o.dup = DupRowsArgs{ptr(a), cur.arena ? (char*)ptr(a) + (size_t)rows * a.ld * 2 : nullptr, rows, a.C, a.ld};
    o.bytes = 2.0 * 2.0 * (double)rows * a.C;
    snprintf(o.klabel, sizeof(o.klabel), "dup_rows");
}

void Engine::dup_second_half(const DupReq& d) {
    if (!g_plan_sw.cfg_share_copy && d.producer < cur.ops.size()) {
        Op& o = cur.ops[d.producer];
        if (o.kind == OP_GEMM && o.g.C == ptr(d.a) && o.g.ldc == d.a.ld && o.g.M == d.rows && !o.g.geglu && !o.g.C8) { o.g.dup_rows = d.rows; return; }
        if (o.kind == OP_ROWGEMM && o.rg.Y == ptr(d.a) && o.rg.ldy == d.a.ld && o.rg.M == d.rows) { o.rg.dup_rows = d.rows; return; }
    }
    op_dup(d.a, d.rows);
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
void Engine::emit_res(const ResW& r, Act X, Act OUT, int B, int H, int W) {
    const int M = B * H * W;
    Act t1 = new_act(M, r.Cin);
    op_gn("res.gn1", X, t1, B, H * W, r.gn1, r.eps, true);
    Act t2 = new_act(M, r.Cout);
    if (r.has_emb) op_conv("res.conv1", t1, B, H, W, r.Cin, r.conv1, 1, H, W, t2, Act{}, cur.d_emb_all ? cur.d_emb_all + r.emb_off : nullptr, un.emb_total);
    else op_conv("res.conv1", t1, B, H, W, r.Cin, r.conv1, 1, H, W, t2, Act{});
    release(t1);
    Act t3 = new_act(M, r.Cout);
    op_gn("res.gn2", t2, t3, B, H * W, r.gn2, r.eps, true);
    release(t2);
    if (r.has_skip && r.fused_skip) {
        op_conv("res.conv2+skip", t3, B, H, W, r.Cout, r.conv2, 1, H, W, OUT, Act{});
        GemmArgs& g = cur.ops.back().g;
        g.A2 = ptr(X); g.lda2 = X.ld; g.Cin2 = r.Cin;
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

// SpatialTransformer.forward (transformer.py:342-377) + BasicTransformerBlock._forward (:186-245)
void Engine::emit_xf(const XfW& x, Act X, Act OUT, int B, int H, int W, Act ctx16, int Mc, int Bshare, const std::vector<DupReq>* dups) {
    const int M = B * H * W, C = x.C, heads = cfg.num_heads, D = C / heads;
    // Shared CFG prefix (plan(): share): up to the first cross-attention both halves of the batch hold the same values, so norm / proj_in / norm1 / q|k|v /
    // self-attention / to_out of the FIRST transformer block run on the first Bq samples (rows [0, Mq)) only
    int Bq = Bshare > 0 ? Bshare : B, Mq = Bq * H * W;
    // which launches the level's stages run as; norm + proj_in become one rowgemm launch in fuse_gn_rowgemm, once norm's statistics come from its producer
    const XfPick pick = xf_pick(XfShape{C, heads, B, H * W, Mc, Bshare, x.blocks[0].ln_fold, 0});
    auto head = [&](const Act& a) { Act v = a; v.rows = Mq; v.owned = false; return v; };      // the first Mq rows of a buffer
    Act t1 = new_act(M, C);
    op_gn("xf.norm", X, t1, Bq, H * W, x.gn, 1e-6f, false);
    Act h = new_act(M, C);
    op_gemm("xf.proj_in", head(t1), x.proj_in, head(h), Act{});
    release(t1);
    Act n{};
    // LayerNorm + projection of the first Mq rows of h, by stage: `w` behind a LayerNorm (its own launch or rowgemm's prologue), the folded copy `wf` otherwise
    auto norm_gemm = [&](XfStage st, const char* rowgemm_name, const char* ln_name, const char* name, const NormW& ln, const LinearW& w, const LinearW& wf, const float* c1, Act Cc, bool geglu) {
        if (st == XS_ROWBLOCK) { op_rowgemm(rowgemm_name, head(h), w, head(Cc), Act{}, 1, &ln); return; }
        if (st == XS_FOLDED) {
            op_gemm(name, head(h), wf, head(Cc), Act{}, geglu);
            GemmArgs& g = cur.ops.back().g;
            g.ln_c1 = c1; g.ln_eps = 1e-5f;
            return;
        }
        if (!n.valid) n = new_act(M, C);
        NormW plain = ln;
        if (st == XS_LN_FOLDED) { plain.g = nullptr; plain.b = nullptr; }     // gamma / beta already live in the folded weights / bias
        op_ln(ln_name, head(h), head(n), plain);
        op_gemm(name, head(n), st == XS_LN_FOLDED ? wf : w, head(Cc), Act{}, geglu);
    };
    // projection + residual into h, in place: x += W . a + b
    auto out_gemm = [&](XfStage st, const char* name, Act a, const LinearW& w) {
        if (st == XS_ROWBLOCK) op_rowgemm(name, a, w, head(h), head(h), 0, nullptr); else op_gemm(name, a, w, head(h), head(h));
    };
    for (int d = 0; d < x.depth; ++d) {
        const XfBlockW& b = x.blocks[d];
        const XfBlockPick& bp = d == 0 ? pick.first : pick.rest;
        Act qkv = new_act(M, 3 * C);
        norm_gemm(bp.qkv, "xf.ln1+qkv", "xf.ln1", "xf.qkv", b.ln1, b.qkv, b.qkv_f, b.c1_qkv, qkv, false);
        Act a = new_act(M, C);
        const char* base = (const char*)ptr(qkv);
        op_attn("xf.attn1", base, 3 * C, base + (size_t)C * 2, 3 * C, base + (size_t)2 * C * 2, 3 * C, a, Bq, heads, H * W, H * W, D);
        if (q_prescale()) cur.ops.back().at.scale = 1.0f / 1.44269504088896340736f;       // the q rows of the projection already carry scale * log2(e)
        release(qkv);
        out_gemm(bp.o1, "xf.o1", head(a), b.o1);                   // x += attn1(norm1(x))
        if (Bq != B) {
            // the context enters here: from now on the halves differ.  The second half's rows take over the shared results that full-batch ops still read.
            cur.prefix_end = cur.ops.size();                               // every op so far ran on one half of the batch
            if (dups) for (const DupReq& dq : *dups) dup_second_half(dq);
            dup_second_half(DupReq{h, Mq, cur.ops.size() - 1});       // the op just emitted (to_out + residual) wrote h
            Bq = B; Mq = M;
        }
        // k|v of the context come from the one batched projection emitted at the start of the forward
        const char* kvb = (const char*)((uintptr_t)cur.arena + cur.kv_all_off) + (size_t)b.kv_off * 2;
        if (bp.xattn) {
            // LayerNorm + q projection + attention over the context + out projection + residual as ONE launch (xattn_block.hip)
            Op& o = emit(OP_XATTN, "xf.xattn2");
            XAttnArgs& xa = o.xa;
            xa.H = ptr(h); xa.ldh = h.ld; xa.M = M; xa.N = H * W; xa.C = C; xa.heads = heads; xa.ln_g = b.ln2.g; xa.ln_b = b.ln2.b; xa.eps = 1e-5f;
            xa.Wq = b.q2.w; xa.Wo = b.o2.w; xa.bo = b.o2.b; xa.K = kvb; xa.ldk = un.kv_total; xa.V = kvb + (size_t)C * 2; xa.ldv = un.kv_total; xa.Mk = Mc;
            xa.scale = q_prescale() ? 1.0f / 1.44269504088896340736f : 1.0f / std::sqrt((float)D);
            o.flops = 2.0 * 2.0 * M * (double)C * C + 4.0 * B * heads * (double)(H * W) * Mc * D;
            o.bytes = 2.0 * 2.0 * (double)M * C;
            snprintf(o.klabel, sizeof(o.klabel), "xattn_block<%s>", dt == DT_BF16 ? "bf16" : "f16");
            cur.flops += o.flops;
        } else {
            Act q = new_act(M, C);
            norm_gemm(bp.q2, "xf.ln2+q2", "xf.ln2", "xf.q2", b.ln2, b.q2, b.q2_f, b.c1_q2, q, false);
            op_attn("xf.attn2", ptr(q), C, kvb, un.kv_total, kvb + (size_t)C * 2, un.kv_total, a, B, heads, H * W, Mc, D);
            if (q_prescale()) cur.ops.back().at.scale = 1.0f / 1.44269504088896340736f;       // the q rows of the projection already carry scale * log2(e)
            release(q);
            out_gemm(bp.o2, "xf.o2", a, b.o2);                     // x += attn2(norm2(x), ctx)
        }
        release(a);
        if (bp.ffblock) {
            // LayerNorm + GEGLU projection + down projection + residual as ONE launch (ff_block.hip): the [M][4C] activation never leaves the CUs
            Op& o = emit(OP_FFBLOCK, "xf.ffblock");
            FFBlockArgs& fa = o.fb;
            fa.H = ptr(h); fa.ldh = h.ld; fa.M = M; fa.C = C; fa.inner = 4 * C; fa.ln_g = b.ln3.g; fa.ln_b = b.ln3.b; fa.eps = 1e-5f;
            fa.W1 = b.ff1.w; fa.b1 = b.ff1.b; fa.W2 = b.ff2.w; fa.b2 = b.ff2.b;
            o.flops = 2.0 * M * (double)C * (8.0 * C) + 2.0 * M * (double)C * (4.0 * C);
            o.bytes = 2.0 * 2.0 * (double)M * C;
            snprintf(o.klabel, sizeof(o.klabel), "ff_block<%s>", dt == DT_BF16 ? "bf16" : "f16");
            cur.flops += o.flops;
        } else {
            Act f = new_act(M, 4 * C);
            norm_gemm(bp.ff1, "", "xf.ln3", "xf.ff1", b.ln3, b.ff1, b.ff1_f, b.c1_ff1, f, true);        // GEGLU
            op_gemm("xf.ff2", f, b.ff2, h, h);                     // x = ff(norm3(x)) + x
            release(f);
        }
    }
    if (n.valid) release(n);
    if (pick.proj_out == XS_ROWBLOCK) op_rowgemm("xf.proj_out", h, x.proj_out, OUT, X, 0, nullptr);
    else op_gemm("xf.proj_out", h, x.proj_out, OUT, X);         // + x_in
    release(h);
}

// The batch of the shared CFG prefix for an evaluation (0 = every op on the full batch): a CFG evaluation over ONE latent batch (xB > 0, B2 == 2 xB, no
// c_concat), a model with a cross-attention for the prefix to end at, and enough rows per half that the prefix ops still fill the chip — below
// LDX_CFG_SHARE_MINROWS (default 8192: 512^2 at bs = 1 has 4096 and measured 5.73 against 5.69 ms per step shared) nothing is shared.
int Engine::share_for(int B2, int h, int w, int xB, bool denoise, bool concat) const {
    const long share_minrows = g_plan_sw.cfg_share_minrows;
    if (!cfg_share || !denoise || concat || xB <= 0 || B2 != 2 * xB || (cfg_share == 1 && (long)xB * h * w < share_minrows)) return 0;
    for (auto& blk : un.in_blocks) if (blk.has_xf) return xB;
    return 0;
}

int Engine::plan(int B2, int h, int w, int Mc, int share) {
    return build_plan(PlanKey{B2, h, w, Mc, share}, [&]() -> int {
        const int mc = cfg.model_channels, ted = 4 * mc;
        // fixed small buffers
        const size_t o_temb = a_alloc((size_t)B2 * mc * 4), o_e1 = a_alloc((size_t)B2 * ted * 4), o_e2 = a_alloc((size_t)B2 * ted * 4);
        const size_t o_emb = a_alloc((size_t)B2 * un.emb_total * 4);
        cur.gn_ws_off = a_alloc(gn_ws_bytes(B2, (long)h * w));
        const size_t o_eps = a_alloc((size_t)B2 * h * w * cfg.out_channels * 4);
        auto f32p = [&](size_t off) { return cur.arena ? (float*)((char*)cur.arena + off) : (float*)nullptr; };
        cur.d_temb_out = f32p(o_temb); cur.d_e1 = f32p(o_e1); cur.d_e2 = f32p(o_e2); cur.d_emb_all = f32p(o_emb); cur.d_eps = f32p(o_eps);

        // ---- level geometry & concat buffers (so skips are written in place, no torch.cat copy) ----
        struct Skip { Act act; int H, W; };
        std::vector<int> Hs{h}, Ws{w};
        for (int l = 1; l < cfg.num_levels; ++l) { Hs.push_back((Hs.back() + 1) / 2); Ws.push_back((Ws.back() + 1) / 2); }
        // simulate the channel bookkeeping of the ctor to size the concat buffers of the output blocks
        std::vector<int> in_ch{mc}, in_lv{0};
        { int c = mc; for (int l = 0; l < cfg.num_levels; ++l) { for (int r = 0; r < cfg.num_res_blocks[l]; ++r) { c = mc * cfg.channel_mult[l]; in_ch.push_back(c); in_lv.push_back(l); }
              if (l != cfg.num_levels - 1) { in_ch.push_back(c); in_lv.push_back(l + 1); } } }
        const int n_skips = (int)in_ch.size();
        // output block k consumes skip (n_skips-1-k); its h channels:
        std::vector<int> out_hch(n_skips);
        { int c = in_ch.back(); int k = 0;
          for (int l = cfg.num_levels - 1; l >= 0; --l) for (int i = 0; i <= cfg.num_res_blocks[l]; ++i) { out_hch[k++] = c; c = mc * cfg.channel_mult[l]; } }
        std::vector<Act> cat(n_skips);
        for (int k = 0; k < n_skips; ++k) {
            const int s = n_skips - 1 - k, lv = in_lv[s];
            cat[k] = new_act(B2 * Hs[lv] * Ws[lv], out_hch[k] + in_ch[s]);
        }
        auto skip_view = [&](int s) { const int k = n_skips - 1 - s; return view(cat[k], out_hch[k], in_ch[s]); };

        // ---- ops ----
        Act xin = new_act(B2 * h * w, 64);
        cur.prep_xc_off = xin.off;
        {
            PrepArgs& p = emit(OP_PREP, "prep").prep;          // x, sigma / timesteps and c_concat are the call's
            p.B = B2; p.C = cfg.in_channels; p.H = h; p.W = w; p.Cpad = 64; p.xc = ptr(xin);
            p.log_sigmas = d_log_sigmas; p.n_sigmas = n_sigmas; p.temb_table = d_temb; p.temb_dim = mc; p.temb_out = cur.d_temb_out;
            if (d_emb_table) { p.emb_table = d_emb_table; p.emb_n = un.emb_total; p.emb_out = cur.d_emb_all; }
        }
        Act ctx16 = new_act(B2 * Mc, cfg.context_dim);
        { Op& o = emit(OP_CVT, "ctx.cvt"); o.cvt = CvtArgs{nullptr, ptr(ctx16), (size_t)B2 * Mc * cfg.context_dim}; o.ctx_only = true; }
        if (!d_emb_table) {       // per-step time-embedding MLP (LDX_EMB_TABLE=0); otherwise the prep kernel gathers the timestep's row of the table
            emit(OP_SKINNY, "time_embed.0").sk = skinny_args(cur.d_temb_out, mc, un.te0.w, un.te0.b, cur.d_e1, ted, B2, ted, mc, 0, 1);
            emit(OP_SKINNY, "time_embed.2").sk = skinny_args(cur.d_e1, ted, un.te2.w, un.te2.b, cur.d_e2, ted, B2, ted, ted, 0, 1);
            emit(OP_SKINNY, "emb_layers").sk = skinny_args(cur.d_e2, ted, un.emb_all.w, un.emb_all.b, cur.d_emb_all, un.emb_total, B2, un.emb_total, ted, 0, 0);
            cur.flops += 2.0 * B2 * ((double)ted * mc + (double)ted * ted + (double)un.emb_total * ted);
        }
        Act kvall = new_act(B2 * Mc, un.kv_total);
        cur.kv_all_off = kvall.off;
        op_gemm("xf.kv2_all", ctx16, un.kv_all, kvall, Act{});
        cur.ops.back().ctx_only = true;

        int lv = 0, s = 0;
        Act hcur = skip_view(0);
        // Bp: batch of the ops in front of the first cross-attention (share > 0: one half of the CFG batch stands for both); `pend` = what they produce
        // that later full-batch ops read (the skip connections), duplicated into the second half's rows when the prefix ends (emit_xf)
        int Bp = share > 0 ? share : B2;
        std::vector<DupReq> pend;
        op_conv("conv_in", xin, Bp, h, w, 64, un.conv_in, 1, h, w, hcur, Act{});
        cur.flops -= 2.0 * Bp * h * w * (double)mc * 9.0 * (64 - cfg.in_channels);   // padded channels are not algorithmic work
        release(xin);
        if (Bp != B2) pend.push_back({hcur, Bp * h * w, cur.ops.size() - 1});
        for (auto& blk : un.in_blocks) {
            ++s;
            Act dst = skip_view(s);
            if (blk.has_down) {
                op_conv("down", hcur, Bp, Hs[lv], Ws[lv], in_ch[s - 1], blk.down, 2, Hs[lv + 1], Ws[lv + 1], dst, Act{});
                ++lv;
                if (Bp != B2) pend.push_back({dst, Bp * Hs[lv] * Ws[lv], cur.ops.size() - 1});
            } else if (blk.has_xf) {
                Act mid = new_act(B2 * Hs[lv] * Ws[lv], blk.res.Cout);
                emit_res(blk.res, hcur, mid, Bp, Hs[lv], Ws[lv]);
                if (Bp != B2) {
                    pend.push_back({mid, Bp * Hs[lv] * Ws[lv], cur.ops.size() - 1});          // proj_out's residual reads it for every sample (emit_res ends with the conv that writes it)
                    emit_xf(blk.xf, mid, dst, B2, Hs[lv], Ws[lv], ctx16, Mc, Bp, &pend);
                    Bp = B2; pend.clear();
                } else {
                    emit_xf(blk.xf, mid, dst, B2, Hs[lv], Ws[lv], ctx16, Mc);
                }
                release(mid);
            } else {
                emit_res(blk.res, hcur, dst, Bp, Hs[lv], Ws[lv]);
                if (Bp != B2) pend.push_back({dst, Bp * Hs[lv] * Ws[lv], cur.ops.size() - 1});
            }
            hcur = dst;
        }
        // middle block (unet.py:537-584); its last op writes column 0 of the first concat buffer
        {
            const int Mm = B2 * Hs[lv] * Ws[lv];
            Act dst = view(cat[0], 0, out_hch[0]);
            if (!un.has_middle) { set_error("UNet config without a middle block is not supported by the planner"); return LDX_EINVAL; }
            if (un.mid_has_xf) {
                Act m0 = new_act(Mm, un.mid_res0.Cout);
                emit_res(un.mid_res0, hcur, m0, B2, Hs[lv], Ws[lv]);
                Act m1 = new_act(Mm, un.mid_res0.Cout);
                emit_xf(un.mid_xf, m0, m1, B2, Hs[lv], Ws[lv], ctx16, Mc);
                release(m0);
                emit_res(un.mid_res1, m1, dst, B2, Hs[lv], Ws[lv]);
                release(m1);
            } else {
                emit_res(un.mid_res0, hcur, dst, B2, Hs[lv], Ws[lv]);
            }
        }
        // output blocks: input of block k is the whole concat buffer cat[k]
        int k = 0;
        Act final_h{};
        for (auto& blk : un.out_blocks) {
            const int sidx = n_skips - 1 - k; (void)sidx;
            const bool last = (k == n_skips - 1);
            const int Hc = Hs[lv], Wc = Ws[lv], Mrows = B2 * Hc * Wc;
            // where does this block's result go?  column 0 of the next concat buffer (at the next block's resolution)
            const int co = blk.res.Cout;
            int nsub = 1 + (blk.has_xf ? 1 : 0) + (blk.has_up ? 1 : 0);
            auto target = [&](bool is_final_sub, int rows) -> Act {
                if (is_final_sub && !last) return view(cat[k + 1], 0, out_hch[k + 1]);
                return new_act(rows, co);
            };
            int sub = 0;
            Act x = cat[k];
            Act r_out = target(++sub == nsub, Mrows);
            emit_res(blk.res, x, r_out, B2, Hc, Wc);
            release(cat[k]);
            x = r_out;
            if (blk.has_xf) {
                Act x_out = target(++sub == nsub, Mrows);
                emit_xf(blk.xf, x, x_out, B2, Hc, Wc, ctx16, Mc);
                release(x);
                x = x_out;
            }
            if (blk.has_up) {
                const int Hn = Hs[lv - 1], Wn = Ws[lv - 1];       // output_shape = hs[-1].shape (unet.py:754)
                Act u_out = target(++sub == nsub, B2 * Hn * Wn);
                op_conv("up", x, B2, Hc, Wc, co, blk.up, 1, Hn, Wn, u_out, Act{});
                release(x);
                x = u_out; --lv;
            }
            final_h = x;
            ++k;
        }
        // out: GroupNorm -> SiLU -> conv3x3 (unet.py:663-677), fp32 NHWC eps
        {
            const int Mrows = B2 * h * w;
            Act t = new_act(Mrows, mc);
            op_gn("out.gn", final_h, t, B2, h * w, un.out_gn, 1e-5f, true);
            release(final_h);
            op_conv("out.conv", t, B2, h, w, mc, un.conv_out, 1, h, w, Act{}, Act{}, nullptr, 0, cur.d_eps, cfg.out_channels);
            release(t);
        }
        { FinishArgs& f = emit(OP_FINISH, "finish").fin; f.eps = cur.d_eps; f.ld = cfg.out_channels; f.B = B2; f.C = cfg.out_channels; f.HW = h * w; }          // x, sigma and out are the call's
        release(ctx16); release(kvall);
        // what the shared prefix saves: every op in front of the first hand-over copy ran on half the batch (the context-only ops are not part of it)
        if (share > 0) {
            for (size_t i = 0; i < cur.prefix_end && i < cur.ops.size(); ++i) if (!cur.ops[i].ctx_only) cur.flops_shared += cur.ops[i].flops;
            cur.flops_shared -= 2.0 * share * h * w * (double)mc * 9.0 * (64 - cfg.in_channels);        // conv_in's padded channels are not algorithmic work (see above)
        }
        fuse_gn_stats();
        fuse_gn_rowgemm();
        return LDX_OK;
    });
}

// The 22 emb_layers outputs for EVERY timestep of the table (ldx_set_tables), by the same three skinny launches a forward would run on its B2 rows:
// row t of d_emb_table is bit-identical to what those launches write for a sample whose timestep index is t (the skinny kernel's rows are independent).
int Engine::build_emb_table() {
    if (!g_plan_sw.emb_table || !d_temb || n_sigmas <= 0 || un.emb_total <= 0 || un.emb_total % 4) return LDX_OK;
    if (finalized && !d_emb_table) return LDX_OK;        // a refresh rebuilds the table finalize() built, in place (the plans hold its address); it never adds one
    const bool refill = d_emb_table != nullptr;
    const int mc = cfg.model_channels, ted = 4 * mc, n = n_sigmas;
    float *e1 = nullptr, *e2 = nullptr, *tab = d_emb_table;
    auto fail = [&](hipError_t err, const char* what) {       // nothing of a half-built table survives an error
        if (e1) (void)hipFree(e1);
        if (e2) (void)hipFree(e2);
        if (tab && !refill) (void)hipFree(tab);
        set_error(std::string(what) + ": " + hipGetErrorString(err));
        return LDX_EHIP;
    };
    hipError_t err;
    if ((err = hipMalloc((void**)&e1, (size_t)n * ted * 4)) != hipSuccess) return fail(err, "build_emb_table: hipMalloc");
    if ((err = hipMalloc((void**)&e2, (size_t)n * ted * 4)) != hipSuccess) return fail(err, "build_emb_table: hipMalloc");
    if (!refill && (err = hipMalloc((void**)&tab, (size_t)n * un.emb_total * 4)) != hipSuccess) return fail(err, "build_emb_table: hipMalloc");
    launch_skinny(skinny_args(d_temb, mc, un.te0.w, un.te0.b, e1, ted, n, ted, mc, 0, 1), dt, nullptr);
    launch_skinny(skinny_args(e1, ted, un.te2.w, un.te2.b, e2, ted, n, ted, ted, 0, 1), dt, nullptr);
    launch_skinny(skinny_args(e2, ted, un.emb_all.w, un.emb_all.b, tab, un.emb_total, n, un.emb_total, ted, 0, 0), dt, nullptr);
    if ((err = hipStreamSynchronize(nullptr)) != hipSuccess) return fail(err, "build_emb_table: hipStreamSynchronize");
    if ((err = hipGetLastError()) != hipSuccess) return fail(err, "build_emb_table: kernel launch");
    (void)hipFree(e1); (void)hipFree(e2);
    if (refill) return LDX_OK;
    dev_allocs.push_back(tab);
    d_emb_table = tab;
    weight_bytes += (size_t)n * un.emb_total * 4;
    return LDX_OK;
}

double Engine::steady_flops() const {
    double f = cur.flops;
    if (ctx_cache) for (const Op& o : cur.ops) if (o.ctx_only) f -= o.flops;
    return f;
}
// the reference's arithmetic for the same evaluation: what runs plus what the shared CFG prefix computes once instead of twice
double Engine::algorithmic_flops() const { return steady_flops() + cur.flops_shared; }

void Plan::release() {
    if (arena) (void)hipFree(arena);
    if (graph_exec) (void)hipGraphExecDestroy(graph_exec);
    arena = nullptr; graph_exec = nullptr;
}

int Engine::build_plan(const PlanKey& key, const std::function<int()>& emit, bool zero_arena) {
    auto reset = [&] {
        free_list.clear(); live.clear(); arena_top = 0; arena_peak = 0;
        cur.ops.clear(); cur.flops = 0; cur.flops_shared = 0; cur.prefix_end = 0;
    };
    cur.key = PlanKey{};                  // no plan until the bound pass has completed
    reset();
    void* const arena = cur.arena;
    cur.arena = nullptr;
    int rc = emit();
    cur.arena = arena;
    if (rc) return rc;
    cur.arena_peak_dry = arena_peak;
    if (cur.arena && cur.arena_cap < cur.arena_peak_dry) { HIP_OK(hipFree(cur.arena)); cur.arena = nullptr; cur.arena_cap = 0; }
    if (!cur.arena) { HIP_OK(hipMalloc(&cur.arena, cur.arena_peak_dry)); cur.arena_cap = cur.arena_peak_dry; }
    if (zero_arena) HIP_OK(hipMemset(cur.arena, 0, cur.arena_cap));
    reset();
    if ((rc = emit())) return rc;
    cur.key = key;
    cur.graph_valid = false; cur.warm = false;
    cur.kv_ptr = nullptr; cur.kv_epoch = 0;          // a fresh arena holds no projected context
    return LDX_OK;
}

// The UNet and Flux keep the plans of other shapes (plan_cache); the other models re-plan into the current plan, whose arena is reused when
// it is large enough.
int Engine::select_plan(const PlanKey& key, hipStream_t st, const std::function<int()>& replan, bool* switched) {
    if (key == cur.key) return LDX_OK;
    HIP_OK(hipStreamSynchronize(st));
    if (switched) *switched = true;
    if (kind == KIND_UNET || kind == KIND_FLUX) {
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
        case OP_EMBED: { ClipEmbedArgs a = o.emb; a.ids = bind.ids; a.extra = clip_extra; a.n_extra = clip_extra_n; launch_clip_embed(a, dt, ls); } break;      // the textual-inversion rows change between calls
        case OP_DUP: launch_dup_rows(o.dup, dt, ls); break;
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
    if (o.kind == OP_GEMM) snprintf(sh, sizeof(sh), " M%d N%d K%d sk%d%s", o.g.M, o.g.N, o.g.K, o.g.splitk, o.g.geglu ? " geglu" : "");
    else if (o.kind == OP_ATTN) snprintf(sh, sizeof(sh), " B%d H%d N%d M%d D%d", o.at.B, o.at.H, o.at.Nq, o.at.Mk, o.at.D);
    else if (o.kind == OP_ATTN_MX) snprintf(sh, sizeof(sh), " B%d H%d N%d M%d D128", o.am.B, o.am.H, o.am.Nq, o.am.Mk);
    else if (o.kind == OP_GN) snprintf(sh, sizeof(sh), " B%d HW%d C%d", o.gn.B, o.gn.HW, o.gn.C);
    else if (o.kind == OP_ROWGEMM) snprintf(sh, sizeof(sh), " M%ld N%d K%d", o.rg.M, o.rg.N, o.rg.K);
    else if (o.kind == OP_XATTN) snprintf(sh, sizeof(sh), " M%ld C%d", (long)o.xa.M, o.xa.C);
    else if (o.kind == OP_FFBLOCK) snprintf(sh, sizeof(sh), " M%ld C%d", (long)o.fb.M, o.fb.C);
    else if (o.kind == OP_LN) snprintf(sh, sizeof(sh), " R%d C%d", o.ln.rows, o.ln.C);
    else if (o.kind == OP_MXQ) snprintf(sh, sizeof(sh), " R%d K%d", o.mq.rows, o.mq.K);
    else if (o.kind == OP_GEMM2) snprintf(sh, sizeof(sh), " M%d+%d N%d K%d", o.g.M, o.g2.M, o.g.N, o.g.K);
    return key + sh;
}

int Engine::exec_ops(hipStream_t ls, size_t op_begin, size_t op_end, int ctx_sel) {
    if (op_end > cur.ops.size()) op_end = cur.ops.size();
    static const bool dbg_nan = getenv("LDX_DEBUG_NAN") != nullptr;          // debug: first GEMM whose 16-bit output holds a NaN / Inf
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
    bind = b; prof_graph = false;
    if (int rc = exec_ops(st)) return rc;
    return launch_status();
}

int Engine::run_cfg(const float* x, float sigma, const float* ctx, int B, int h, int w, int Mc, float* out, hipStream_t st, int t_index) {
    if (B <= 0) { set_error("ldx_unet_denoise_cfg: bad argument"); return LDX_EINVAL; }
    if (t_index >= n_sigmas) { set_error("ldx_unet_denoise_cfg_t: t_index outside the sigma table"); return LDX_EINVAL; }
    HIP_OK(hipSetDevice(device));
    if (sigma_cfg_cap < 2 * B) {
        HIP_OK(hipStreamSynchronize(st));
        if (d_sigma_cfg) (void)hipFree(d_sigma_cfg);
        d_sigma_cfg = nullptr; sigma_cfg_cap = 0;
        HIP_OK(hipMalloc((void**)&d_sigma_cfg, sizeof(float) * 4 * B));
        sigma_cfg_cap = 2 * B;
    }
    float* d_t = d_sigma_cfg + sigma_cfg_cap;
    if (t_index >= 0) launch_fill2_f32(d_sigma_cfg, sigma, d_t, (float)t_index, 2 * B, st);          // outside the captured graph: the values change every step
    else launch_fill_f32(d_sigma_cfg, sigma, 2 * B, st);
    return run(x, d_sigma_cfg, ctx, 2 * B, h, w, Mc, out, true, st, B, nullptr, 0, t_index >= 0 ? d_t : nullptr);
}
int Engine::timestep_lookup(const float* sigma_dev, int n, int* out_dev, hipStream_t st) {
    if (kind != KIND_UNET || !d_log_sigmas) { set_error("ldx_unet_timestep: needs a UNet engine with its sigma table (ldx_set_tables)"); return LDX_ESTATE; }
    if (!sigma_dev || !out_dev || n < 0) { set_error("ldx_unet_timestep: bad argument"); return LDX_EINVAL; }
    HIP_OK(hipSetDevice(device));
    launch_timestep(sigma_dev, d_log_sigmas, n_sigmas, n, out_dev, st);
    HIP_OK(hipGetLastError());
    return LDX_OK;
}

int Engine::run(const float* x, const float* sigma_or_t, const float* ctx, int B2, int h, int w, int Mc, float* out, bool denoise, hipStream_t st, int xB,
                const float* c_concat, int cc_channels, const float* t_idx) {
    if (!denoise) t_idx = nullptr;            // forward mode: sigma_or_t already carries the indices
    if (c_concat && (cc_channels <= 0 || cc_channels >= cfg.in_channels || (denoise && cfg.in_channels - cc_channels != cfg.out_channels))) {
        set_error("ldx_unet_denoise_concat: c_concat channels must leave the latent's channels (in_channels - cc_channels == out_channels)"); return LDX_EINVAL;
    }
    if (!c_concat) cc_channels = 0;
    if (xB < 0 || (xB > 0 && B2 % xB != 0)) { set_error("ldx_unet_*: the batch of x must divide the evaluation batch"); return LDX_EINVAL; }
    if (!finalized) { set_error("ldx_unet_*: engine not finalized"); return LDX_ESTATE; }
    if (!x || !sigma_or_t || !ctx || !out || B2 <= 0 || h <= 0 || w <= 0 || Mc <= 0) { set_error("ldx_unet_*: bad argument"); return LDX_EINVAL; }
    HIP_OK(hipSetDevice(device));
    // CFG evaluation over one latent batch (ldx_unet_denoise_cfg*: xB > 0 and B2 == 2 xB): the two halves are identical up to the first cross-attention, which
    // the plan then computes once (plan(): share).  LDX_CFG_SHARE=0: every op on the full batch, as the concatenated ldx_unet_denoise call runs it.
    const int share = share_for(B2, h, w, xB, denoise, c_concat != nullptr);
    if (int rc = select_plan(PlanKey{B2, h, w, Mc, share}, st, [&] { return plan(B2, h, w, Mc, share); })) return rc;
    bind = Bindings{};
    bind.x = x; bind.s = sigma_or_t; bind.ctx = ctx; bind.out = out; bind.den = denoise; bind.xB = xB; bind.cc = c_concat; bind.ccn = cc_channels; bind.t = t_idx;
    bind.ctxc = ctx_cache;
    // context cache: the ctx_only ops run here, eagerly, only when this plan's buffers do not hold the projections of (ctx, epoch) yet; every
    // other op (and the captured graph) then leaves them out
    if (bind.ctxc && !(cur.kv_ptr == ctx && cur.kv_epoch == ctx_epoch && cur.kv_stream == st)) {
        const bool pg = prof_graph; prof_graph = false;
        const int rc = exec_ops(st, 0, (size_t)-1, 2);
        prof_graph = pg;
        if (rc) return rc;
        cur.kv_ptr = ctx; cur.kv_epoch = ctx_epoch; cur.kv_stream = st;
    }
    const bool same = cur.graph_b == bind;
    // a captured graph has its pointers baked in: once a call arrives with other bindings (in ANY mode — the eager path below re-records
    // graph_b), that graph must never be replayed against the new graph_b (round 3: a stale graph was replayed after an eager call had moved them)
    if (!same) cur.graph_valid = false;
    if (graph_mode && cur.graph_valid && same) {
        HIP_OK(hipGraphLaunch(cur.graph_exec, st));
        ++n_graph_replays;
        return LDX_OK;
    }
    // capture only once the same (plan, pointers) have been run eagerly before: the first eager pass
    // also performs the one-time hipFuncSetAttribute calls, which are illegal during capture.
    const bool use_graph = graph_mode && cur.warm && same;
    cur.graph_b = bind; cur.warm = true;
    hipStream_t ls = st;
    if (use_graph) {
        if (cur.graph_exec) { (void)hipGraphExecDestroy(cur.graph_exec); cur.graph_exec = nullptr; }
        if (!cap_stream) HIP_OK(hipStreamCreateWithFlags(&cap_stream, hipStreamNonBlocking));
        HIP_OK(hipStreamSynchronize(st));
        HIP_OK(hipStreamBeginCapture(cap_stream, hipStreamCaptureModeThreadLocal));
        ls = cap_stream;
    }
    prof_graph = use_graph;
    { int rc = exec_ops(ls, 0, (size_t)-1, bind.ctxc ? 1 : 0); if (rc) return rc; }
    if (use_graph) {
        hipGraph_t g = nullptr;
        HIP_OK(hipStreamEndCapture(cap_stream, &g));
        HIP_OK(hipGraphInstantiate(&cur.graph_exec, g, nullptr, nullptr, 0));
        (void)hipGraphDestroy(g);
        cur.graph_valid = true;
        ++n_graph_captures;
        HIP_OK(hipGraphLaunch(cur.graph_exec, st));
    }
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
