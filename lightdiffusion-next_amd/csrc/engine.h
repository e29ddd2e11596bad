// Internal declarations of the ldx engines: the shared planner / executor (engine.cpp) and one class per model (engine_<model>.cpp).
#pragma once
#include <cstring>
#include <functional>
#include <initializer_list>
#include <map>
#include <string>
#include <type_traits>
#include <unordered_map>
#include <utility>
#include <vector>

#include "../../include/ldx.h"
#include "ldx_kernels.h"
#include "ldx_switches.h"

namespace ldx {

extern thread_local std::string g_last_error;
void set_error(const std::string& s);
int launch_status();          // LDX_EHIP (and the error text) when a kernel launch since the last check failed
// inside a function that returns an LDX_* code: leave with LDX_EHIP (and the error text) when a HIP call fails
#define HIP_OK(expr)                                                                         \
    do {                                                                                     \
        hipError_t _e = (expr);                                                              \
        if (_e != hipSuccess) {                                                              \
            set_error(std::string(#expr) + ": " + hipGetErrorString(_e));                    \
            return LDX_EHIP;                                                                 \
        }                                                                                    \
    } while (0)

// A state-dict tensor as registered: a host copy (ldx_load_tensor: `data`), or device memory (`dev`, `data` empty): the caller's own, not copied
// (ldx_load_tensor_device / ldx_load_tensor_dev; UNet, Flux and T5 engines), or the engine's fp16 expansion of a Q8_0 tensor (ldx_load_tensor_q8_0).
// at() reads the host copy (the getter-style upload16 / upload32; the piece packers read `data` themselves).
struct HostTensor {
    int dtype = LDX_F32;
    std::vector<int64_t> shape;
    std::vector<uint8_t> data;
    size_t numel = 0;
    const void* dev = nullptr;
    float at(size_t i) const;
};

struct LinearW { void* w = nullptr; float* b = nullptr; int N = 0, K = 0;
                 void* w8 = nullptr; uint32_t* sw = nullptr; };     // MX fp8 copy + E8M0 scales [K/128][N] (Flux fp8 mode)
struct NormW { float* g = nullptr; float* b = nullptr; int C = 0; };
struct ResW { NormW gn1, gn2; LinearW conv1, conv2, skip; bool has_skip = false; bool fused_skip = false; /* fused_skip: conv2 holds [W2 | Wskip], bias b2 + bskip */ int Cin = 0, Cout = 0; int emb_off = 0;
              float eps = 1e-5f; bool has_emb = true; };
struct XfBlockW { NormW ln1, ln2, ln3; LinearW qkv, o1, q2, kv2, o2, ff1, ff2; LinearW qkv_f, q2_f, ff1_f; /* LayerNorm-folded copies (ln_fold) */ int kv_off = 0;
    // ln_fold: folded copies exist: norm1/2/3 folded into qkv_f / q2_f / ff1_f (weights W .* gamma, bias W beta + b, c1_* = row sums of the stored weights);
    // the planner picks them per input shape (small row counts, where the row-block kernels are not taken):
    // the GEMM reads the un-normalised rows and applies rstd * (acc - mean * c1) + bias in its epilogue (GemmArgs::ln_stat)
    bool ln_fold = false; float *c1_qkv = nullptr, *c1_q2 = nullptr, *c1_ff1 = nullptr; };
struct XfW { NormW gn; LinearW proj_in, proj_out; std::vector<XfBlockW> blocks; int C = 0, depth = 0; };
// level, ch (the walk's bookkeeping, read by UNetEngine::plan): an input block's output, the skip it leaves, has `ch` channels at resolution level `level`; an output block runs at `level` on `ch` channels of h beside its skip_ch
struct BlockW { bool has_res = false, has_xf = false, has_down = false, has_up = false; ResW res; XfW xf; LinearW down, up; int skip_ch = 0, level = 0, ch = 0; };
// Every weight of the UNet, as the structure walk (UNetEngine::walk_weights) builds it; emb_all / kv_all: the emb_layers of every ResBlock and the k | v projections of
// every cross-attention, each batched into one GEMM per forward ([emb_total][4 mc] and [kv_total][context_dim])
struct UNetW {
    LinearW te0, te2, conv_in, conv_out, emb_all, kv_all;
    NormW out_gn;
    std::vector<BlockW> in_blocks, out_blocks;
    bool has_middle = false, mid_has_xf = false;
    ResW mid_res0, mid_res1;
    XfW mid_xf;
    int emb_total = 0, kv_total = 0;
};

// activation view inside the arena: rows x C 16-bit elements, row stride ld, starting at column col
struct Act { bool valid = false; bool owned = false; size_t off = 0; int rows = 0, C = 0, ld = 0, col = 0; };

enum OpKind { OP_PREP, OP_CVT, OP_SKINNY, OP_GEMM, OP_GN, OP_LN, OP_ATTN, OP_FINISH,
              OP_VAEPREP, OP_SOFTMAX, OP_CLAMP, OP_EMBED, OP_CVT_OUT,
              OP_PIXPREP, OP_MOMENTS, OP_COPY_OUT,
              OP_FX_PATCH, OP_FX_TEMB, OP_FX_SILU, OP_FX_ROPE, OP_FX_UNPATCH, OP_FX_SKINNY_Y, OP_MXQ, OP_GEMM2, OP_XATTN, OP_FFBLOCK, OP_ROWGEMM, OP_ATTN_MX, OP_MXVT, OP_DUP,
              OP_TAESD_PREP, OP_TAESD_CONV,
              OP_SAM_PATCH, OP_SAM_WINDOW, OP_SAM_RELPOS, OP_SAM_ATTN, OP_SAM_ROWVEC, OP_SAM_OUT };
// One launch of a plan.  The rule: every kind has ONE argument struct (ldx_kernels.h, beside its launcher), filled by the planner, and Engine::launch_op hands it to
// that launcher after filling in the pointers of the call (Bindings).  Nothing here has a meaning that depends on `kind`.
struct Op {
    OpKind kind; const char* name;
    GemmArgs g; GemmArgs g2; GroupNormArgs gn; LayerNormArgs ln; AttnArgs at; SkinnyArgs sk; QkRopeArgs rp; MxQuantArgs mq; XAttnArgs xa; FFBlockArgs fb; RowGemmArgs rg; AttnMxArgs am; MxVtArgs vt;
    PrepArgs prep; FinishArgs fin; CvtArgs cvt; CvtOutArgs out; CopyOutArgs copy; VaePrepArgs vprep; PixelsPrepArgs pix; ClampArgs clamp; SoftmaxArgs sm; ClipEmbedArgs emb; MixArgs mix; DupRowsArgs dup;
    FluxTembArgs temb; SiluArgs silu; FluxPatchArgs patch; FluxUnpatchArgs unpatch; TaesdPrepArgs tprep; TaesdConvArgs tconv;
    SamPatchArgs spatch; SamWindowArgs swin; SamRelposArgs srel; SamAttnArgs sattn; SamRowvecArgs srv; SamOutArgs sout;
    bool ctx_only;                 // depends on the context alone (16-bit copy of ctx, the batched k|v projection): skipped while Engine::ctx_cache holds
    // which of the call's buffers (Bindings) launch_op binds, where the kind alone does not say
    bool bias_from_call;           // the attention's score bias table is the call's (T5)
    bool second_output;            // the converted result goes to the call's optional second output (CLIP's intermediate layer)
    bool of_guidance;              // the embedded scalar is the call's guidance, not its sigma (Flux)
    int tok0;                      // first token of the rope op's rows in the call's rotary tables
    double flops; double bytes; char klabel[48];
};
// What a planner has to say about an op beyond its emitter's parameters: a callable on the op's argument struct — [&](GemmArgs& g) { g.act = 1; } — or, where it
// sets one of the flags above, on the Op.  The emitter runs it BEFORE it derives what depends on the arguments (attention scratch and kernel pick, label, flops,
// bytes), so nothing is patched after an emitter has returned.  Split-K alone is chosen in front of it: an edit may lower GemmArgs::splitk to 1, never raise it.
template <class Args, Args Op::*member> struct OpEdit {
    std::function<void(Op&)> fn;
    OpEdit() = default;
    template <class F> OpEdit(F f) { if constexpr (std::is_invocable_v<F, Op&>) fn = f; else fn = [f](Op& o) { f(o.*member); }; }
    void operator()(Op& o) const { if (fn) fn(o); }
};
using GemmEdit = OpEdit<GemmArgs, &Op::g>; using AttnEdit = OpEdit<AttnArgs, &Op::at>; using LnEdit = OpEdit<LayerNormArgs, &Op::ln>; using GnEdit = OpEdit<GroupNormArgs, &Op::gn>;
struct ProfEntry { long count = 0; double ms = 0, flops = 0, bytes = 0; };

// What a plan was built for.  Per model: UNet (B2, h, w, Mc, share), Flux (B, h, w, Lt), VAE (B, h, w, 1) decode / (B, Hpx, Wpx, 2) encode,
// CLIP (B, T, 0, inter_layer), T5 (B, L), ESRGAN (B, H, W), TAESD (B, h, w), SAM (B).  B = 0: no plan.
struct PlanKey {
    int B = 0, h = 0, w = 0, m = 0, share = 0;
    bool operator==(const PlanKey& o) const { return B == o.B && h == o.h && w == o.w && m == o.m && share == o.share; }
    bool operator!=(const PlanKey& o) const { return !(*this == o); }
};

// The caller's buffers of one call, read by exec_ops.  Pointers and ints alone, laid out without padding (the assertion below), so that == is the bytes':
// a field added here takes part in it.
struct Bindings {
    const float *x = nullptr, *s = nullptr, *ctx = nullptr; float* out = nullptr; int den = 0, xB = 0;
    const float *cc = nullptr, *t = nullptr;      // UNet: c_concat; caller-supplied timestep indices (run(): t_idx)
    int ccn = 0, ctxc = 0;                        // UNet: channels of c_concat; context-cache mode (the ctx_only ops are left out)
    const int* ids = nullptr; float* out2 = nullptr; const float* bias = nullptr;       // CLIP / T5
    const float* extra = nullptr;                                                         // CLIP: textual-inversion rows for ids >= vocab_size (T5: none) ...
    const float *y = nullptr, *guid = nullptr, *pe_cos = nullptr, *pe_sin = nullptr;     // Flux
    uint8_t* out8 = nullptr; int n_extra = 0, flux = 0;                                   // ... and their number; TAESD: the 8-bit preview and its channel order
    bool operator==(const Bindings& o) const { return memcmp(this, &o, sizeof(Bindings)) == 0; }
};
static_assert(std::has_unique_object_representations_v<Bindings>, "Bindings: a bool, a float or padding would make == compare bytes that are no value");

// Everything that belongs to one planned input shape: the launch list over one activation arena, the buffers inside that arena and the graph
// captured from it.  Plans move as a whole (Engine::cur <-> Engine::plan_cache); release() frees what a plan owns.
struct Plan {
    PlanKey key;
    std::vector<Op> ops;
    double flops = 0;
    double flops_up2x = 0;                 // flops the plan does NOT execute because its up convs run in phase form (GemmArgs::up2x): 5/9 of their 9-tap arithmetic
    double flops_shared = 0;               // flops the plan does NOT execute because of the shared CFG prefix (the second half's copy of the prefix ops)
    size_t prefix_end = 0;                 // UNet: number of ops in front of the first cross-attention (they ran on `share` samples)
    void* arena = nullptr;
    size_t arena_cap = 0, arena_peak_dry = 0;
    size_t gn_ws_off = 0;
    // UNet
    size_t prep_xc_off = 0, kv_all_off = 0;
    float *d_temb_out = nullptr, *d_e1 = nullptr, *d_e2 = nullptr, *d_emb_all = nullptr, *d_eps = nullptr;
    const void* kv_ptr = nullptr; uint64_t kv_epoch = 0;       // context cache: what the kvall buffer holds
    hipStream_t kv_stream = nullptr;                            // ... and the stream whose order it was filled in: a call on another stream refills (no cross-stream dependency is assumed)
    // The graph captured from the plan (Engine::run_bound).  b: the bindings of the last eager or capturing pass, what a graph captured now has baked in;
    // warm: that pass has happened; valid: exec was captured with b and has been launched once
    struct Graph {
        hipGraphExec_t exec = nullptr;
        bool valid = false, warm = false;
        Bindings b;
        void reset() { valid = false; warm = false; }          // a new plan: nothing has run, nothing may be replayed
        void release() { if (exec) (void)hipGraphExecDestroy(exec); exec = nullptr; valid = false; }
    } graph;
    // Flux: buffers inside the arena, first-block-cache buffers and op ranges ([0, fb_a_end) through double block 0, [fb_a_end, fb_b_end) the rest)
    float *fx_temb = nullptr, *fx_gemb = nullptr, *fx_h1 = nullptr, *fx_vec = nullptr, *fx_svec = nullptr, *fx_mod = nullptr, *fx_tok = nullptr;
    void *fb_s0 = nullptr, *fb_s1 = nullptr, *fb_x = nullptr; float *fb_first = nullptr, *fb_res = nullptr, *fb_part = nullptr;
    int fb_B = 0, fb_L = 0, fb_Lt = 0, fb_C = 0; size_t fb_a_end = 0, fb_b_end = 0;
    void release();                        // the arena and the graph
};

// SkinnyArgs with every byte defined, the padding too (the plan recorder, tests/tools/plan_trace.py, compares launch arguments byte for byte)
inline SkinnyArgs skinny_args(const float* x, int ldx, const void* W, const float* bias, float* out, int ldo, int M, int N, int K, int in_act, int out_act, int accum = 0) {
    SkinnyArgs a; memset(&a, 0, sizeof(a));
    a.x = x; a.ldx = ldx; a.W = W; a.bias = bias; a.out = out; a.ldo = ldo; a.M = M; a.N = N; a.K = K; a.in_act = in_act; a.out_act = out_act; a.accum = accum;
    return a;
}

struct EmbSrc { const HostTensor* w; const HostTensor* b; int n; };      // n rows of a stacked matrix (Engine::mk_stacked); b may be null

struct VaeAttnW { NormW norm; LinearW q, k, v, proj; LinearW qkv; /* C = 512: fused q | k | v projection [3C][C] for the flash kernel (attn512.hip); bias = [bq | bk | 0], bv folded into proj's */ };
struct ClipLayerW { NormW ln1, ln2; LinearW qkv, out, fc1, fc2; };
struct RdbW { LinearW c[5]; };
struct T5LayerW { NormW ln1, ln2; LinearW qkv, o, wi, wo; };
struct FluxStreamW { LinearW qkv, proj, mlp0, mlp2; float* qs = nullptr; float* ks = nullptr; int mod_off = 0; };
struct FluxDoubleW { FluxStreamW img, txt; };
struct FluxSingleW { LinearW lin1_qkv, lin1_mlp, lin2; float* qs = nullptr; float* ks = nullptr; int mod_off = 0; };

// The planner / executor every model is built on, and what every model's weights go through.  A model is a derived class (UNetEngine, VaeEngine, ClipEngine,
// T5Engine, EsrganEngine, FluxEngine, TaesdEngine, SamEngine) that owns its config, its weight tables, finalize(), its plan functions and its run entry points; the C ABI reaches a model
// entry point only through that class (capi.cpp engine_as), so nothing here or there asks an engine what it is.
class Engine {
public:
    static constexpr const char* model = "valid";
    // keep_plans: plans of other input shapes stay in plan_cache (UNet, Flux); otherwise a new shape re-plans into the current plan
    // captures: graph_mode captures and replays this model's plans (UNet, TAESD, SAM); the other models accept the mode and ignore it
    Engine(int dev, int compute_dtype, bool keep_plans, bool captures = false)
        : device(dev), dt(compute_dtype == LDX_F16 ? DT_F16 : DT_BF16), captures(captures), keep_plans(keep_plans) {}
    virtual ~Engine();
    Engine(const Engine&) = delete;
    Engine& operator=(const Engine&) = delete;
    int validate() const { return LDX_OK; }              // config checks at creation; a model that has some hides this (ldx_*_create calls it on the model's class)
    int load_tensor(const char* key, const void* data, int dtype, const int64_t* shape, int ndim);
    // What a model's weight walk can read besides host copies: device-resident sources (every layout a piece list), Q8_0 tensors (Flux, T5: the reference's GGUF files)
    virtual bool takes_device_tensors() const { return false; }
    virtual bool takes_q8_0() const { return false; }
    // fn: the entry point's name for the error text (ldx_load_tensor_device, ldx_load_tensor_dev)
    int load_tensor_dev(const char* fn, const char* key, const void* dev_ptr, int dtype, const int64_t* shape, int ndim);
    // blocks of 34 bytes -> an LDX_F16 tensor: on the host (weight_convert.h), or by q8.hip into a device buffer of the engine's (q8_bufs, freed with the staged sources)
    int load_tensor_q8_0(const char* key, const void* blocks, const int64_t* shape, int ndim, bool on_device);
    int packed_digest(const char* fn, uint64_t* out);    // FNV-1a over host copies of weight_allocs, in allocation order
    virtual int finalize() = 0;
    // context cache (ldx_unet_context_cache): the caller promises that the bytes behind a ctx pointer do not change until it calls
    //     ldx_unet_context_cache again; the 16-bit copy of ctx and the batched k|v projection of every cross-attention (transformer.py:186-245 recomputes
    //     them every step only because a torch module has no notion of a sampling run) are then computed on the first evaluation of a (plan, ctx) only.
    //     Set by the UNet alone; here because the executor and the plan's counts leave the ctx_only ops out while it holds.
    bool ctx_cache = false;
    double algorithmic_flops() const;                           // steady_flops() + flops_shared + flops_up2x
    double steady_flops() const;                                // algorithmic flops of one forward as executed in steady state (cached ops excluded)
    virtual int64_t n_launches() const;
    int64_t n_graph_captures = 0, n_graph_replays = 0;      // ldx_graph_stats (tests: the sampler loops must replay, not re-capture)
    // per-kernel-class HIP-event profile of subsequent forwards (bench.py roofline leg)
    bool profiling = false, prof_detail = false;   // detail: key the report by op shape as well
    std::map<std::string, ProfEntry> prof;
    std::string profile_json() const;

    const int device;
    const DType dt;
    bool finalized = false;
    bool graph_mode = false;
    size_t weight_bytes = 0;
    Plan cur;                              // the plan being run (while a plan function runs: being built)

protected:
    // weights
    std::unordered_map<std::string, HostTensor> host;
    std::string missing;
    std::vector<void*> dev_allocs;
    const HostTensor* get(const std::string& key, std::initializer_list<int64_t> shape);
    // A model's weight buffers are asked for in one fixed order, which lets the UNet run the same sequence of mk_* calls in three modes (UNetEngine::walk_weights):
    // ALLOC (every model's finalize) allocates each buffer, CHECK (refresh) only resolves keys and shapes, REFILL (refresh) writes into the allocations ALLOC made.
    enum WalkMode { WALK_ALLOC, WALK_CHECK, WALK_REFILL };
    WalkMode walk_mode = WALK_ALLOC;
    struct WeightAlloc { void* p; size_t bytes; };
    std::vector<WeightAlloc> weight_allocs;                // every packed buffer (weight_buf), in allocation order
    size_t walk_next = 0;                                  // CHECK / REFILL: the next entry of weight_allocs
    std::string walk_err;
    bool refreshing = false;                               // UNet, between refresh_begin and refresh_commit: load_tensor is open again
    void* weight_buf(size_t bytes);                        // the next weight buffer (null: error)
    int weights_failed();                                  // the tail of a failed walk / finalize: missing key -> LDX_EMISSING, walk_err -> LDX_ESTATE, else the HIP error
    // A packed buffer is described ONCE, as pieces of source tensors; weight_layout.h turns a piece into bits, for both sides.  Per buffer: some source is on
    // the device (ldx_load_tensor_device) -> one launch per piece of pack.hip's loops over those functions, host sources of that buffer staged as raw copies
    // (freed when the walk ends); no source on the device -> a CPU loop over the same functions and one copy.  Same buffers in the same order either way:
    // either can refill what the other allocated.  16-byte granularity (K, cols, col0, CinPad multiples of 8) is asked of the launches only.
    // src_rows > 0: the piece is rows [src_row0, src_row0 + N) of a source of src_rows rows (a sub-view: the packers get the address of its first row)
    struct Piece { const HostTensor* src; size_t row0, col0; int N, K; float scale; int geglu_inner; int Cin, CinPad; size_t src_row0 = 0, src_rows = 0; };
    static Piece rows_piece(const HostTensor* src, size_t row0, int N, int K, float scale = 1.0f, int geglu_inner = 0) { return Piece{src, row0, 0, N, K, scale, geglu_inner, 0, 0}; }
    static Piece conv_piece(const HostTensor* src, int Cout, int Cin, int CinPad) { return Piece{src, 0, 0, Cout, 9 * CinPad, 1.0f, 0, Cin, CinPad}; }      // [Cout][ky][kx][CinPad] <- [Cout][Cin][ky][kx]
    static Piece rows_view(const HostTensor* src, size_t src_row0, size_t src_rows, size_t row0, int N, int K) { Piece p = rows_piece(src, row0, N, K); p.src_row0 = src_row0; p.src_rows = src_rows; return p; }
    // out[off + i] = a[i] (+ b[i]); src_n > 0: a[src0 + i] of a source of src_n elements (b must be null)
    struct VecPiece { const HostTensor* a; const HostTensor* b; size_t off; int n; int geglu_inner; size_t src0 = 0, src_n = 0; };
    std::unordered_map<const HostTensor*, void*> staged;
    std::vector<void*> q8_bufs;                            // fp16 expansions of device Q8_0 tensors: sources like `staged`, dropped with them
    const void* dev_src(const HostTensor* t);
    const void* piece_src(const HostTensor* t, bool dev) { return dev ? dev_src(t) : t->numel ? (const void*)t->data.data() : (const void*)t; }      // never null for an empty host tensor (nothing is read)
    void drop_staged();
    void* pack16(size_t rows, size_t cols, const std::vector<Piece>& pieces);
    float* pack32(size_t n, const std::vector<VecPiece>& pieces);
    // What no piece list describes stays on a getter, element by element on the host (all in engines that load from the host only):
    //   VaeEngine::mk_vae_attn  proj.b    Wp . bv + bp, an fp64 dot product per element
    //   VaeEngine::mk_vae_attn  qkv.b     [bq | bk | 0]: the zero tail has no source
    void* upload16(size_t rows, size_t cols, const std::function<float(size_t, size_t)>& getter);
    float* upload32(size_t n, const std::function<float(size_t)>& getter);
    bool mk_linear(const std::string& pre, int N, int K, bool bias, LinearW& out, bool conv1x1 = false);
    bool mk_conv3(const std::string& pre, int Cout, int Cin, int CinPad, LinearW& out);
    bool mk_norm(const std::string& pre, int C, NormW& out);
    bool mk_ln_folded(int N, int K, const std::vector<Piece>& pieces, const HostTensor* bias_t, const std::string& norm_pre, LinearW& out, float*& c1);
    bool mk_fused_skip(const std::string& conv, const std::string& skip, int Cin, int Cout, ResW& r);      // conv2 | skip in one matrix (UNet and VAE ResBlocks)
    bool mk_stacked(const std::vector<EmbSrc>& srcs, int K, LinearW& out);                                   // rows of several tensors in one matrix, their biases in one vector

    // executor
    int exec_ops(hipStream_t ls, size_t op_begin = 0, size_t op_end = (size_t)-1, int ctx_sel = 0);      // ctx_sel: 0 all ops, 1 skip ctx_only ops, 2 ONLY ctx_only ops
    int launch_op(const Op& o, hipStream_t ls);           // the op's launcher on its argument struct, with this call's pointers (bind) filled in
    std::string prof_key(const Op& o) const;              // profile label of an op (prof_detail: with its shape)
    // the calls that keep one plan and run it whole: make the plan of `key` current, bind the call's buffers, run_bound
    int run_planned(const PlanKey& key, const std::function<int()>& replan, const Bindings& b, hipStream_t st);
    // the tail of every such call: the current plan on `bind`, as a graph replay, a capture or eager launches (ctx_sel: exec_ops')
    int run_bound(hipStream_t st, int ctx_sel = 0);
    const bool captures;
    hipStream_t cap_stream = nullptr;                     // graph capture; made by the first one
    Bindings bind;                                        // this call's
    std::vector<hipEvent_t> prof_events;
    bool prof_graph = false;

    // planner toolkit; the state is that of the plan being built (build_plan resets it)
    Op& emit(OpKind kind, const char* name);              // appends a zeroed op to the plan being built; the reference holds until the next emit
    // GroupNorm workspace: gn_ws_rows producer rows per image + GN_FOLD folded rows, x 32 groups x 2 floats (ldx_kernels.h gn_workspace_rows)
    int gn_ws_rows = 256;
    size_t gn_ws_bytes(int B, long HWmax) { gn_ws_rows = (int)gn_workspace_rows(HWmax); return (size_t)B * (gn_ws_rows + GN_FOLD) * 32 * 2 * 4; }
    unsigned* d_sk_count = nullptr;                       // split-K tile counters (sk_counters()): one zeroed buffer per engine, every launch leaves it zeroed
    unsigned* sk_counters();
    // What the argument builders (ldx_kernels.h gemm_attach_splitk, attn_attach_scratch) take scratch from.  An op's scratch (split-K partials, attention key
    // norms / split partials) is dead as soon as the op's launches have run, so its arena range is freed at once: the next buffer may reuse it
    const Scratch scratch{[this](size_t bytes) -> void* { const size_t off = a_alloc(bytes); a_free(off); return (void*)((uintptr_t)cur.arena + off); }, [this] { return sk_counters(); }};
    int plan_rc = LDX_OK;                                 // an emitter found a planner bug (set_error holds the text): build_plan fails the plan with it
    void seal_gemm(Op& o, const GemmEdit& edit, double a_elems, bool residual);      // the tail of op_gemm / op_conv: K splits, the edit, the split-K check, then flops, bytes and label
    void fuse_gn_stats();                                 // post-pass over ops: GroupNorms whose input was just written by a fusable GEMM / conv get their statistics from its epilogue
    void fuse_gn_rowgemm();                               // post-pass: xf.norm (producer statistics) + xf.proj_in -> one rowgemm launch where xf_proj_in_rowgemm says so
    void op_rowgemm(const char* name, Act X, const LinearW& w, Act Y, Act R, int pro, const NormW* nw);
    std::vector<std::pair<size_t, size_t>> free_list;
    std::map<size_t, size_t> live;
    size_t arena_top = 0, arena_peak = 0;
    // Two passes of `emit` into cur: a dry one (arena == nullptr) measures the peak, the second binds real pointers into an arena of that
    // size (the current plan's when it is large enough; zero_arena: zero-filled).  cur.key = key on success.
    int build_plan(const PlanKey& key, const std::function<int()>& emit, bool zero_arena = false);
    // make the plan for `key` current (replan: builds it into cur); *switched: cur is another plan than before the call
    int select_plan(const PlanKey& key, hipStream_t st, const std::function<int()>& replan, bool* switched = nullptr);
    size_t a_alloc(size_t bytes);
    void a_free(size_t off);
    void* ptr(const Act& a) const { return (void*)((uintptr_t)cur.arena + a.off + (size_t)a.col * 2); }
    // a new arena buffer of `bytes` that is no activation (never released by the plans that use it), as a T* (the dry pass: an offset from a null arena)
    template <class T> T* arena_ptr(size_t bytes) { return (T*)((uintptr_t)cur.arena + a_alloc(bytes)); }
    const char* dt_name() const { return dt == DT_BF16 ? "bf16" : "f16"; }      // the compute type as the kernels' labels spell it
    Act new_act(int rows, int C);
    Act view(const Act& base, int col, int C);
    static Act rows(const Act& t, int r0, int nr) { Act v = t; v.owned = false; v.off = t.off + (size_t)r0 * t.ld * 2; v.rows = nr; return v; }      // rows [r0, r0 + nr) of a buffer
    void release(const Act& a);
    // The op emitters.  `edit` (OpEdit above) is applied before anything is derived from the arguments.
    void op_gemm(const char* name, Act A, const LinearW& w, Act C, Act R, int geglu = 0, const GemmEdit& edit = {});      // geglu: GemmArgs::geglu (1 erf, 2 tanh)
    void op_conv(const char* name, Act X, int B, int Hin, int Win, int Cin, const LinearW& w, int stride, int Hout, int Wout,
                 Act Y, Act R, const float* rowvec = nullptr, int rv_ld = 0, float* Cf = nullptr, int ldcf = 0, const GemmEdit& edit = {});
    void op_gn(const char* name, Act X, Act Y, int B, int HW, const NormW& n, float eps, bool silu, const GnEdit& edit = {});
    void op_ln(const char* name, Act X, Act Y, const NormW& n, const LnEdit& edit = {});
    void op_attn(const char* name, const void* Q, int ldq, const void* K, int ldk, const void* V, int ldv, Act O, int B, int H, int Nq, int Mk, int D, const AttnEdit& edit = {});
    // UNet and VAE ResBlock; emb [.][emb_ld]: the batched emb_layers output a block with has_emb adds its columns [emb_off, emb_off + Cout) of (null in the dry pass)
    void emit_res(const ResW& r, Act X, Act OUT, int B, int H, int W, const float* emb = nullptr, int emb_ld = 0);

    // Plans of other input shapes seen (keep_plans: multi-scale samplers alternate between two resolutions, prompts of different lengths change
    // Flux's Lt): launch plan, arena and captured graph are kept per shape, so switching back costs nothing (a re-plan + two eager passes
    // before the graph is usable again cost ~17 ms per switch)
    const bool keep_plans;
    std::vector<Plan> plan_cache;
    void plan_stash();                    // move the current plan into plan_cache (evicting the oldest beyond 4)
    bool plan_restore(const PlanKey& key);
};

class UNetEngine final : public Engine {
public:
    static constexpr const char* model = "UNet";
    UNetEngine(const ldx_unet_config& c, int dev);
    ~UNetEngine() override;
    int validate() const;
    bool takes_device_tensors() const override { return true; }
    int set_tables(const float* ls, int n, const float* temb, int dim);
    int finalize() override;
    // Replace the weights of a finalized engine in place (ldx_unet_refresh_begin / _commit): begin re-opens the two loaders, commit validates
    // the full key set (nothing written on LDX_EMISSING, and `un` stays as it was), then runs the structure walk again into the SAME device allocations,
    // rebuilds the emb_layers table and drops the cached context projections.  No pointer a plan or a captured graph holds changes.
    int refresh_begin();
    int refresh_commit();
    int refresh_abort();                   // forget an unfinished refresh: the loaders close again, the weights are untouched
    // c_concat [B2][cc_channels][h][w] (fp32, may be null): appended unscaled behind the scaled x, which then carries in_channels - cc_channels channels
    // t_idx [B2] (device fp32, may be null; denoise only): timestep indices supplied by the caller instead of the device's own sigma -> index lookup
    int run(const float* x, const float* sigma_or_t, const float* ctx, int B2, int h, int w, int Mc, float* out, bool denoise, hipStream_t st, int xB = 0,
            const float* c_concat = nullptr, int cc_channels = 0, const float* t_idx = nullptr);
    // one CFG evaluation: x [B] is read by both halves of the [uncond; cond] batch (cond.py:186-226), sigma is one host scalar for every sample
    // t_index >= 0: the sigma -> timestep index computed by the caller (the reference's own host arithmetic); < 0: the device lookup
    int run_cfg(const float* x, float sigma, const float* ctx, int B, int h, int w, int Mc, float* out, hipStream_t st, int t_index = -1);
    int timestep_lookup(const float* sigma_dev, int n, int* out_dev, hipStream_t st);      // ldx_unet_timestep: the prep kernel's lookup alone
    int set_context_cache(int enable) { ctx_cache = enable != 0; ++ctx_epoch; return LDX_OK; }      // Engine::ctx_cache
    int cfg_share = 1;                     // ldx_unet_cfg_share / LDX_CFG_SHARE: plan CFG evaluations with the shared prefix (0 never, 1 where it pays, 2 whenever possible)
    const ldx_unet_config cfg;

private:
    UNetW un;
    // sources of un.emb_all / un.kv_all (k, v, k, v, ...), collected by the walk
    std::vector<EmbSrc> emb_srcs, kv_srcs;
    bool mk_res(const std::string& pre, int Cin, int Cout, ResW& r);
    bool mk_xf(const std::string& pre, int C, int depth, XfW& x);
    int walk_weights();                                    // the mk_* calls in UNetModel1.__init__ order, in walk_mode: builds a fresh UNetW and installs it as `un` on success only
    float* d_log_sigmas = nullptr; float* d_temb = nullptr; int n_sigmas = 0;
    float* d_sigma_cfg = nullptr; int sigma_cfg_cap = 0;      // [2 * cap] sigma followed by [2 * cap] timestep indices
    // ---- step-invariant work (round 5) ----
    // per-timestep table of the 22 emb_layers outputs: time_embed -> SiLU -> emb_layers is a pure function of the INTEGER timestep (a8: t = argmin
    //     index; unet.py:333-342, ResBlock.py:283-295), so all n_sigmas rows are computed once by the SAME skinny kernels (bit-identical to the per-step
    //     launches) and the prep kernel gathers the row: three launches per forward gone.  LDX_EMB_TABLE=0 keeps the per-step launches.
    float* d_emb_table = nullptr;
    int build_emb_table();
    // phase weights of the up convs that some plan runs in phase form (GemmArgs::up2x; weight_layout.h up_phase_group): derived from the packed 9-tap matrix when the
    //     first such plan is built — never at finalize, never inside a stream capture (plans are built in front of it) — and again, in place, by refresh_commit: the
    //     same contract as the table above, plans and captured graphs keep their pointers.  LDX_UPCONV_PHASE=0: every up conv stays a 9-tap op.
    struct UpPhase { const void* w9; void* wp; int N, Cin; };
    std::vector<UpPhase> up_phase;
    int upconv_phase = 1;
    int up_to_phase(const LinearW& w);                     // the op just emitted (an "up" conv) in phase form, where gemm_upconv_phase admits it
    int derive_up_phase();                                 // every buffer of up_phase from its 9-tap matrix
    uint64_t ctx_epoch = 1;                // context cache: bumped whenever cached k|v projections stop being valid
    // share > 0 (ldx_unet_denoise_cfg*): the evaluation batch is [uncond x share ; cond x share] over ONE latent batch x [share] — everything in front of the
    // first cross-attention (conv_in, the ResBlocks / Downsamples / self-attention up to it) sees identical inputs in both halves and is planned on `share`
    // samples; its results are copied into the second half's rows where the first cross-attention (and the skip connections) need them (OP_DUP).
    int plan(int B2, int h, int w, int Mc, int share = 0);
    int share_for(int B2, int h, int w, int xB, bool denoise, bool concat) const;
    // Bshare > 0: the ops in front of the first cross-attention run on Bshare samples (see plan()); `dups` = views whose first Bshare * (their own H * W)
    // rows are to be copied into the following rows at that point (plus h itself)
    struct DupReq { Act a; int rows; size_t producer; };       // producer: index of the op that writes `a` (its dual store is preferred to a copy launch)
    void emit_xf(const XfW& x, Act X, Act OUT, int B, int H, int W, Act ctx16, int Mc, int Bshare = 0, const std::vector<DupReq>* dups = nullptr);
    void op_dup(const Act& a, int rows);          // rows [0, rows) of view a -> rows [rows, 2 rows)
    void dup_second_half(const DupReq& d);        // the producer's dual store (GemmArgs / RowGemmArgs::dup_rows) where it has one, else op_dup
};

class VaeEngine final : public Engine {
public:
    static constexpr const char* model = "VAE";
    VaeEngine(const ldx_vae_config& c, int dev) : Engine(dev, c.compute_dtype, false), cfg(c) {}
    int finalize() override;
    int run_decode(const float* z, int B, int h, int w, float* out_nhwc, hipStream_t st);
    int run_encode(const float* px, int B, int H, int W, float* moments, hipStream_t st);
    const ldx_vae_config cfg;

private:
    std::vector<std::vector<ResW>> vae_up; std::vector<LinearW> vae_upconv; std::vector<bool> vae_has_up;
    ResW vae_mid1, vae_mid2; VaeAttnW vae_attn; NormW vae_norm_out; LinearW vae_conv_in, vae_conv_out; float* vae_pq = nullptr;
    // encoder (optional: only when encoder.* weights were loaded)
    bool vae_has_enc = false;
    std::vector<std::vector<ResW>> enc_down; std::vector<LinearW> enc_downconv;
    ResW enc_mid1, enc_mid2; VaeAttnW enc_attn; NormW enc_norm_out; LinearW enc_conv_in, enc_conv_out; float* enc_qc = nullptr;
    bool mk_vae_res(const std::string& pre, int Cin, int Cout, ResW& r);
    bool mk_vae_attn(const std::string& pre, int C, VaeAttnW& a);
    void emit_vae_attn(const VaeAttnW& a, Act X, Act OUT, int B, int H, int W);
    int plan_decode(int B, int h, int w);
    int plan_encode(int B, int H, int W);
};

class ClipEngine final : public Engine {
public:
    static constexpr const char* model = "CLIP";
    ClipEngine(const ldx_clip_config& c, int dev) : Engine(dev, c.compute_dtype, false), cfg(c) {}
    int finalize() override;
    int run(const int* ids, int B, int T, int inter_layer, float* out_last, float* out_inter, hipStream_t st);
    int set_clip_extra(const float* rows_host, int n);
    int clip_pooled(const float* last, const int* ids, int B, int T, int eos_id, float* out, hipStream_t st);
    const ldx_clip_config cfg;

private:
    std::vector<ClipLayerW> clip_layers; NormW clip_final_ln; float* clip_tok = nullptr; float* clip_pos = nullptr;
    float* clip_extra = nullptr; int clip_extra_n = 0, clip_extra_cap = 0;     // textual-inversion rows for ids >= vocab_size
    float* clip_proj = nullptr;                                                // optional text_projection.weight [E][E] fp32 (CLIPTextModel.py:130,152-163)
    int plan(int B, int T, int inter);
};

class T5Engine final : public Engine {
public:
    static constexpr const char* model = "T5";
    T5Engine(const ldx_t5_config& c, int dev) : Engine(dev, c.compute_dtype, false), cfg(c) {}
    bool takes_device_tensors() const override { return true; }
    bool takes_q8_0() const override { return true; }
    int finalize() override;
    int run(const int* ids, int B, int L, const float* bias, float* out, hipStream_t st);
    const ldx_t5_config cfg;

private:
    std::vector<T5LayerW> t5_layers; NormW t5_final_ln; float* t5_tok = nullptr;
    int plan(int B, int L);
};

class EsrganEngine final : public Engine {
public:
    static constexpr const char* model = "ESRGAN";
    EsrganEngine(const ldx_esrgan_config& c, int dev) : Engine(dev, c.compute_dtype, false), cfg(c) {}
    int finalize() override;
    int run(const float* px, int B, int H, int W, float* out, hipStream_t st);
    const ldx_esrgan_config cfg;

private:
    std::vector<RdbW> es_rdb; LinearW es_first, es_trunk, es_hr, es_last; std::vector<LinearW> es_up;
    int plan(int B, int H, int W);
};

// TAESD decoder (engine_taesd.cpp): latent fp32 NCHW -> decoded fp32 NCHW and / or the 8-bit NHWC preview
struct TaesdBlockW { LinearW c[3]; };
class TaesdEngine final : public Engine {
public:
    static constexpr const char* model = "TAESD";
    TaesdEngine(const ldx_taesd_config& c, int dev) : Engine(dev, c.compute_dtype, false, true), cfg(c) {}
    int validate() const;
    int finalize() override;
    int run(const float* z, int B, int h, int w, float* out_f32, uint8_t* out_u8, int flux, hipStream_t st);
    const ldx_taesd_config cfg;

private:
    LinearW ta_first, ta_last, ta_up[3]; TaesdBlockW ta_blocks[10];
    bool mk_conv64(const std::string& pre, int Cout, int Cin, bool bias, LinearW& out);
    int plan(int B, int h, int w);
};

// SAM image encoder (engine_sam.cpp): the preprocessed image fp32 [B][3][size][size] -> the image embedding fp32 [B][out_chans][size / 16][size / 16]
struct SamBlockW { NormW ln1, ln2; LinearW qkv, proj, lin1, lin2; float* rel_h = nullptr; float* rel_w = nullptr; bool global = false; };
class SamEngine final : public Engine {
public:
    static constexpr const char* model = "SAM";
    SamEngine(const ldx_sam_config& c, int dev) : Engine(dev, c.compute_dtype, false, true), cfg(c) {}
    int validate() const;
    int finalize() override;
    int run(const float* x, int B, float* out, hipStream_t st);
    const ldx_sam_config cfg;

private:
    LinearW sam_patch, sam_neck0, sam_neck2; NormW sam_neck1, sam_neck3; float* sam_pos = nullptr; std::vector<SamBlockW> sam_blocks;
    int plan(int B);
};

// SAM prompt encoder + mask decoder (engine_samdec.cpp), fp32: the image embedding and P prompts -> low-res mask logits and IoU predictions.  It plans no Op list:
// a call is a fixed sequence of samdec.hip launches over buffers kept per (P, n, boxes or not), captured into a hipGraph in graph mode.
struct SamDecAttnW { float* wq = nullptr; float* bq = nullptr; float* wkv = nullptr; float* bkv = nullptr; float* wo = nullptr; float* bo = nullptr; };      // wkv: k | v rows stacked
struct SamDecLayerW { float* wqkv = nullptr; float* bqkv = nullptr; float* wo = nullptr; float* bo = nullptr; NormW n1, n2, n3, n4; SamDecAttnW t2i, i2t;
                      float* w1 = nullptr; float* b1 = nullptr; float* w2 = nullptr; float* b2 = nullptr; };
class SamDecoderEngine final : public Engine {
public:
    static constexpr const char* model = "SAM decoder";
    SamDecoderEngine(const ldx_samdec_config& c, int dev) : Engine(dev, LDX_BF16, false, true), cfg(c) {}
    ~SamDecoderEngine() override;
    int validate() const;
    int finalize() override;
    int64_t n_launches() const override { return last_launches; }
    int set_image(const float* emb, hipStream_t st);
    // tokens_out != null: the prompt tokens alone (ldx_samdec_prompt_tokens)
    int predict(const float* points, const int* labels, int n, const float* boxes, int P, float* lowres, float* iou, float* tokens_out, hipStream_t st);
    const ldx_samdec_config cfg;

private:
    struct Call { const float* points; const int* labels; const float* boxes; float* lowres; float* iou; };
    struct DecPlan {
        int P = 0, n = 0, box = 0;
        float* ws = nullptr; size_t ws_floats = 0;
        hipGraphExec_t exec = nullptr; bool valid = false, warm = false; Call c{};
    };
    std::vector<DecPlan> plans;
    SamDecLayerW layers[2]; SamDecAttnW fin; NormW nfin;
    float *gauss = nullptr, *point_emb = nullptr, *not_a_point = nullptr, *no_mask = nullptr, *iou_token = nullptr, *mask_tokens = nullptr, *dense_pe = nullptr;
    float *up1_w = nullptr, *up1_b = nullptr, *up2_w = nullptr, *up2_b = nullptr; NormW up_ln;
    float *hyp_w[3] = {nullptr, nullptr, nullptr}, *hyp_b[3] = {nullptr, nullptr, nullptr}, *iou_w[3] = {nullptr, nullptr, nullptr}, *iou_b[3] = {nullptr, nullptr, nullptr};
    float *src0 = nullptr, *k0v0 = nullptr, *q0 = nullptr;          // per image: rows, layer 0's k | v of the tokens' attention, layer 0's q of the rows' attention
    bool have_image = false, capturing = false;
    int64_t last_launches = 0;
    bool mk_attn(const std::string& pre, int inner, SamDecAttnW& w);
    float* stack32(const std::vector<std::string>& keys, std::initializer_list<int64_t> shape);
    int run_ops(DecPlan& p, const Call& c, float* tokens_out, hipStream_t st);
};

class FluxEngine final : public Engine {
public:
    static constexpr const char* model = "Flux";
    FluxEngine(const ldx_flux_config& c, int dev) : Engine(dev, c.compute_dtype, true), cfg(c) {}
    bool takes_device_tensors() const override { return true; }
    bool takes_q8_0() const override { return true; }
    int finalize() override;
    int run(const float* x, const float* sigma, const float* ctx, const float* y, const float* guidance,
            const float* pe_cos, const float* pe_sin, int B, int h, int w, int Lt, bool denoise, float* out, hipStream_t st);
    // First-block cache (WaveSpeed/first_block_cache.py:105-384, fbcache_nodes.py:8-201): opt-in approximate mode
    float fb_threshold = 0.f; bool fb_have_first = false, fb_have_res = false; float fb_prev_t = 0.f; bool fb_prev_valid = false;
    long fb_hits = 0, fb_misses = 0;
    void fb_reset() { fb_have_first = fb_have_res = false; fb_prev_valid = false; }
    // MX fp8 mode (BASELINE config 4 "fp8 MFMA"): the block linears run on block-scaled fp8 operands; opt-in, own parity class
    bool fx_fp8 = false;
    bool fx_fp8_attn = false;        // ... and QK^T / PV of the joint attention on MX fp8 too (attn_mx.hip; ldx_flux_set_fp8 mode 1, head dim 128)
    const ldx_flux_config cfg;

private:
    std::vector<FluxDoubleW> fx_double; std::vector<FluxSingleW> fx_single;
    LinearW fx_img_in, fx_txt_in, fx_time0, fx_time1, fx_vec0, fx_vec1, fx_gd0, fx_gd1, fx_mod_all, fx_final;
    int fx_mod_total = 0, fx_final_mod_off = 0;
    std::vector<EmbSrc> fx_mod_srcs;
    bool mx_quantize_weight(LinearW& w);
    int plan(int B, int h, int w, int Lt);
};

}  // namespace ldx
