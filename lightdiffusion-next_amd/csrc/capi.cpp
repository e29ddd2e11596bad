// extern "C" surface of libldx.so (include/ldx.h).  No exceptions cross the ABI.
#include <cstring>
#include <memory>
#include <mutex>
#include <new>

#include "engine.h"
#include "weight_convert.h"

using namespace ldx;

struct ldx_engine { Engine* impl; };

#define GUARD_BEGIN try {
#define GUARD_END                                                                  \
    }                                                                              \
    catch (const std::bad_alloc&) { set_error("out of host memory"); return LDX_EINVAL; } \
    catch (const std::exception& ex) { set_error(std::string("internal error: ") + ex.what()); return LDX_EINVAL; }

// The engine behind a handle as the class an entry point belongs to: Engine for what every model answers, a model's class for its own entry points.
// Null, with the error text set and *rc the code to return, for a null handle (LDX_EINVAL) or another model's engine (wrong_model).
template <class T> static T* engine_as(ldx_engine* e, const char* fn, int* rc, int wrong_model = LDX_ESTATE) {
    T* t = e ? dynamic_cast<T*>(e->impl) : nullptr;
    if (!t) { set_error(std::string(fn) + ": not a " + T::model + " engine"); *rc = e ? wrong_model : LDX_EINVAL; }
    return t;
}
// `m`: the engine of handle `e` as a T, or leave the entry point with engine_as's code
#define ENGINE_AS(T, m, ...)                                          \
    int m##_rc = LDX_OK;                                              \
    T* const m = engine_as<T>(e, __func__, &m##_rc, ##__VA_ARGS__);   \
    if (!m) return m##_rc

static int check_device(int device) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) { set_error("no HIP device available (libldx has no CPU fallback)"); return LDX_EHIP; }
    if (device < 0 || device >= n) { set_error("device ordinal out of range"); return LDX_EINVAL; }
    return LDX_OK;
}
template <class T, class Config> static int create_engine(const Config* cfg, int device, ldx_engine** out, const char* fn) {
    GUARD_BEGIN
    if (!cfg || !out) { set_error(std::string(fn) + ": null argument"); return LDX_EINVAL; }
    int rc = check_device(device);
    if (rc) return rc;
    std::unique_ptr<T> e(new T(*cfg, device));
    if ((rc = e->validate())) return rc;
    *out = new ldx_engine{e.release()};
    return LDX_OK;
    GUARD_END
}
static inline DType dtype_of(int d) { return d == LDX_F16 ? DT_F16 : DT_BF16; }
static int check_launch(const char* what) {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) { set_error(std::string(what) + ": " + hipGetErrorString(e)); return LDX_EHIP; }
    return LDX_OK;
}

// scratch for the single-op entry points (split-K partials); grown on demand, never shrunk
// One buffer PER DEVICE (the current one), growth under a mutex.  The single-op entry points are test / probe
// surface: calls that split K share this buffer, so they must be issued on ONE stream per device at a time
// (include/ldx.h says so); the engines own their workspaces and never come here.
static float* op_workspace(size_t floats) {
    static std::mutex mu;
    static float* buf[64] = {nullptr}; static size_t cap[64] = {0};
    int dev = 0;
    (void)hipGetDevice(&dev);
    dev &= 63;
    std::lock_guard<std::mutex> lock(mu);
    if (floats > cap[dev]) {
        if (buf[dev]) { (void)hipDeviceSynchronize(); (void)hipFree(buf[dev]); buf[dev] = nullptr; cap[dev] = 0; }
        if (hipMalloc((void**)&buf[dev], floats * 4) != hipSuccess) return nullptr;
        cap[dev] = floats;
    }
    return buf[dev];
}
// tile counters of the in-kernel split-K reduction for the single-op entry points: per device, zeroed once, left at zero by every launch (same
// one-stream-per-device rule as the workspace)
static unsigned* op_sk_counters() {
    static std::mutex mu;
    static unsigned* buf[64] = {nullptr};
    int dev = 0;
    (void)hipGetDevice(&dev);
    dev &= 63;
    std::lock_guard<std::mutex> lock(mu);
    if (!buf[dev]) {
        if (hipMalloc((void**)&buf[dev], sizeof(unsigned) * SK_COUNTERS) != hipSuccess) { buf[dev] = nullptr; return nullptr; }
        if (hipMemset(buf[dev], 0, sizeof(unsigned) * SK_COUNTERS) != hipSuccess) { (void)hipFree(buf[dev]); buf[dev] = nullptr; return nullptr; }
    }
    return buf[dev];
}
// what the argument builders (ldx_kernels.h) take scratch from here
static const Scratch op_scratch{[](size_t bytes) -> void* { return op_workspace((bytes + 3) / 4); }, op_sk_counters};
static int attach_splitk(GemmArgs& g) {
    gemm_attach_splitk(g, op_scratch);
    if (g.splitk > 1 && !g.ws) { set_error("split-K workspace allocation failed"); return LDX_EHIP; }
    return LDX_OK;
}
// ... and operands that are only ever tested for being there and for their alignment (ldx_op_gemm_pick, ldx_op_attn_pick)
alignas(16) static char pick_operand[16];
static const Scratch pick_scratch{[](size_t) -> void* { return pick_operand; }, [] { return (unsigned*)pick_operand; }};

extern "C" {

const char* ldx_version(void) { return "ldx 0.1 (gfx950)"; }
const char* ldx_last_error(void) { return g_last_error.c_str(); }

int ldx_create(const ldx_unet_config* cfg, int device, ldx_engine** out) { return create_engine<UNetEngine>(cfg, device, out, __func__); }
void ldx_destroy(ldx_engine* e) { if (e) { delete e->impl; delete e; } }

int ldx_vae_create(const ldx_vae_config* cfg, int device, ldx_engine** out) { return create_engine<VaeEngine>(cfg, device, out, __func__); }
int ldx_clip_create(const ldx_clip_config* cfg, int device, ldx_engine** out) { return create_engine<ClipEngine>(cfg, device, out, __func__); }
int ldx_vae_decode(ldx_engine* e, const float* z, int B, int h, int w, float* out, void* stream) {
    GUARD_BEGIN
    ENGINE_AS(VaeEngine, m);
    return m->run_decode(z, B, h, w, out, (hipStream_t)stream);
    GUARD_END
}
int ldx_clip_encode(ldx_engine* e, const int32_t* ids, int B, int T, int inter_layer, float* out_last, float* out_inter, void* stream) {
    GUARD_BEGIN
    ENGINE_AS(ClipEngine, m);
    return m->run((const int*)ids, B, T, inter_layer, out_last, out_inter, (hipStream_t)stream);
    GUARD_END
}
int ldx_clip_pooled(ldx_engine* e, const float* last, const int32_t* ids, int B, int T, int eos_token_id, float* out_pooled, void* stream) {
    GUARD_BEGIN
    ENGINE_AS(ClipEngine, m);
    return m->clip_pooled(last, (const int*)ids, B, T, eos_token_id, out_pooled, (hipStream_t)stream);
    GUARD_END
}
int ldx_clip_set_extra_embeddings(ldx_engine* e, const float* rows_host, int n) {
    GUARD_BEGIN
    ENGINE_AS(ClipEngine, m);
    return m->set_clip_extra(rows_host, n);
    GUARD_END
}
int ldx_esrgan_create(const ldx_esrgan_config* cfg, int device, ldx_engine** out) { return create_engine<EsrganEngine>(cfg, device, out, __func__); }
int ldx_esrgan_forward(ldx_engine* e, const float* pixels_nhwc, int B, int H, int W, float* out_nhwc, void* stream) {
    GUARD_BEGIN
    ENGINE_AS(EsrganEngine, m);
    return m->run(pixels_nhwc, B, H, W, out_nhwc, (hipStream_t)stream);
    GUARD_END
}
int ldx_taesd_create(const ldx_taesd_config* cfg, int device, ldx_engine** out) { return create_engine<TaesdEngine>(cfg, device, out, __func__); }
int ldx_taesd_decode(ldx_engine* e, const float* latent, int B, int h, int w, float* out_f32, uint8_t* out_u8, int flux_flag, void* stream) {
    GUARD_BEGIN
    ENGINE_AS(TaesdEngine, m);
    return m->run(latent, B, h, w, out_f32, out_u8, flux_flag, (hipStream_t)stream);
    GUARD_END
}
int ldx_taesd_conv64(const void* X, const void* Wt, const float* bias, const void* R, const float* Rf, void* Y, float* Yf, int B, int Hin, int Win, int up, int relu, int dtype, void* stream) {
    TaesdConvArgs a{};
    a.X = X; a.W = Wt; a.bias = bias; a.R = R; a.Rf = Rf; a.Y = Y; a.Yf = Yf; a.B = B; a.Hin = Hin; a.Win = Win; a.up = up; a.relu = relu ? 1 : 0;
    if (!taesd_conv_ok(a)) { set_error("ldx_taesd_conv64: bad argument (null pointer, both residuals, up not 0 | 1, 2^31 output pixels or more)"); return LDX_EINVAL; }
    launch_taesd_conv(a, dtype_of(dtype), (hipStream_t)stream);
    return check_launch("ldx_taesd_conv64");
}
int ldx_sam_create(const ldx_sam_config* cfg, int device, ldx_engine** out) { return create_engine<SamEngine>(cfg, device, out, __func__); }
int ldx_sam_encode(ldx_engine* e, const float* x_nchw_f32, int B, float* out_nchw_f32, void* stream) {
    GUARD_BEGIN
    ENGINE_AS(SamEngine, m);
    return m->run(x_nchw_f32, B, out_nchw_f32, (hipStream_t)stream);
    GUARD_END
}
int ldx_sam_preprocess(const uint8_t* img, int64_t pitch, int h, int w, float* out, int size, void* stream) {
    if (!img || !out || h <= 0 || w <= 0 || size <= 0 || size > 16384 || h > size || w > size || pitch < (int64_t)w * 3) {
        set_error("ldx_sam_preprocess: bad argument (null pointer, h or w outside 1 .. size, pitch < w * 3)"); return LDX_EINVAL; }
    launch_sam_preprocess(SamPreprocessArgs{img, (long)pitch, h, w, out, size}, (hipStream_t)stream);
    return check_launch("ldx_sam_preprocess");
}
int ldx_samdec_create(const ldx_samdec_config* cfg, int device, ldx_engine** out) { return create_engine<SamDecoderEngine>(cfg, device, out, __func__); }
int ldx_samdec_set_image(ldx_engine* e, const float* embedding, void* stream) {
    GUARD_BEGIN
    ENGINE_AS(SamDecoderEngine, m);
    return m->set_image(embedding, (hipStream_t)stream);
    GUARD_END
}
int ldx_samdec_predict(ldx_engine* e, const float* points, const int32_t* labels, int n, const float* boxes, int P, float* lowres_out, float* iou_out, void* stream) {
    GUARD_BEGIN
    ENGINE_AS(SamDecoderEngine, m);
    return m->predict(points, (const int*)labels, n, boxes, P, lowres_out, iou_out, nullptr, (hipStream_t)stream);
    GUARD_END
}
int ldx_samdec_prompt_tokens(ldx_engine* e, const float* points, const int32_t* labels, int n, const float* boxes, int P, float* out, void* stream) {
    GUARD_BEGIN
    ENGINE_AS(SamDecoderEngine, m);
    return m->predict(points, (const int*)labels, n, boxes, P, nullptr, nullptr, out, (hipStream_t)stream);
    GUARD_END
}
int ldx_samdec_postprocess(const float* lowres, int n, int L, int in_h, int in_w, int H, int W, uint8_t* mask_u8, float* logits, int image_size, void* stream) {
    const SamDecPostArgs a{lowres, n, L, image_size, in_h, in_w, H, W, mask_u8, logits};
    if (!samdec_post_ok(a)) { set_error("ldx_samdec_postprocess: bad argument (null pointer, a size <= 0, in_h or in_w above image_size)"); return LDX_EINVAL; }
    launch_samdec_post(a, (hipStream_t)stream);
    return check_launch("ldx_samdec_postprocess");
}
int ldx_op_sam_window(const void* src, void* dst, const void* R, int B, int S, int win, int C, int scatter, int dtype, void* stream) {
    const SamWindowArgs a{src, dst, R, B, S, win, C, scatter};
    if (!sam_window_ok(a)) { set_error("ldx_op_sam_window: bad argument (null pointer, src == dst, C % 8, scatter not 0 | 1, R without scatter)"); return LDX_EINVAL; }
    launch_sam_window(a, dtype_of(dtype), (hipStream_t)stream);
    return check_launch("ldx_op_sam_window");
}
int ldx_op_sam_relpos(const void* Q, int ldq, const float* th, const float* tw, float* out, int BW, int H, int n, int dtype, void* stream) {
    const SamRelposArgs a{Q, ldq, th, tw, out, BW, H, n};
    if (!sam_relpos_ok(a)) { set_error("ldx_op_sam_relpos: bad argument (null pointer, ldq % 8, ldq < H * 64, n outside 1 .. 1024)"); return LDX_EINVAL; }
    launch_sam_relpos(a, dtype_of(dtype), (hipStream_t)stream);
    return check_launch("ldx_op_sam_relpos");
}
int ldx_op_sam_attention(const void* Q, const void* K, const void* V, int ld, const float* rel, void* O, int ldo, int BW, int H, int n, float scale, int dtype, void* stream) {
    const SamAttnArgs a{Q, K, V, ld, rel, O, ldo, BW, H, n, scale};
    if (!sam_attn_ok(a)) { set_error("ldx_op_sam_attention: bad argument (null pointer, ld % 8, ldo % 4, rows narrower than H * 64, BW * H > 65535, n outside 1 .. 1024)"); return LDX_EINVAL; }
    launch_sam_attention(a, dtype_of(dtype), (hipStream_t)stream);
    return check_launch("ldx_op_sam_attention");
}
int ldx_tile_blend(const float* tile, int th, int tw, float* out, float* div, int H, int W, int C, int y0, int x0, int feather, void* stream) {
    if (!tile || !out || !div || th <= 0 || tw <= 0 || C <= 0 || y0 < 0 || x0 < 0 || y0 + th > H || x0 + tw > W || feather < 0) {
        set_error("ldx_tile_blend: bad argument (tile must lie inside the output)"); return LDX_EINVAL; }
    launch_tile_blend(tile, th, tw, out, div, H, W, C, y0, x0, feather, (hipStream_t)stream);
    return check_launch("ldx_tile_blend");
}
int ldx_tile_finish(float* out, const float* div, int64_t n, int clamp01, void* stream) {
    if (!out || n < 0) { set_error("ldx_tile_finish: bad argument"); return LDX_EINVAL; }
    launch_tile_finish(out, div, (size_t)n, clamp01, (hipStream_t)stream);
    return check_launch("ldx_tile_finish");
}
// ---- 8-bit image ops (image.hip) -------------------------------------------------------------------------------------------------------
static bool image_ok(const void* p, int64_t pitch, int H, int W, int C) { return p && H > 0 && W > 0 && (C == 1 || C == 3) && pitch >= (int64_t)W * C; }
static bool rect_ok(int x0, int y0, int w, int h, int W, int H) { return x0 >= 0 && y0 >= 0 && w > 0 && h > 0 && x0 <= W - w && y0 <= H - h; }
int ldx_image_quantize(const float* in, int H, int W, int C, uint8_t* out, int64_t out_pitch, void* stream) {
    if (!in || !image_ok(out, out_pitch, H, W, C)) { set_error("ldx_image_quantize: bad argument (null pointer, C not 1 | 3, pitch < W * C)"); return LDX_EINVAL; }
    launch_image_quantize(in, out, H, W, C, (long)out_pitch, (hipStream_t)stream);
    return check_launch("ldx_image_quantize");
}
int ldx_image_to_float(const uint8_t* img, int64_t pitch, int H, int W, int C, int x0, int y0, int w, int h, float* out, void* stream) {
    if (!out || !image_ok(img, pitch, H, W, C) || !rect_ok(x0, y0, w, h, W, H)) {
        set_error("ldx_image_to_float: bad argument (null pointer, C not 1 | 3, pitch < W * C, crop outside the image)"); return LDX_EINVAL; }
    launch_image_to_float(img + (int64_t)y0 * pitch + (int64_t)x0 * C, (long)pitch, out, h, w, C, (hipStream_t)stream);
    return check_launch("ldx_image_to_float");
}
int ldx_image_resample_pass(const uint8_t* in, int64_t in_pitch, int H, int W, int C, int axis, int new_len,
                            const int32_t* bounds, const int32_t* kk, int ksize, uint8_t* out, int64_t out_pitch, void* stream) {
    if (!image_ok(in, in_pitch, H, W, C) || (axis != 0 && axis != 1) || new_len <= 0 || !bounds || !kk || ksize <= 0 || in == out ||
        !image_ok(out, out_pitch, axis == 0 ? new_len : H, axis == 1 ? new_len : W, C)) {
        set_error("ldx_image_resample_pass: bad argument (null pointer, C not 1 | 3, axis 0 | 1, pitch < W * C, in == out)"); return LDX_EINVAL; }
    launch_image_resample_pass(in, (long)in_pitch, out, (long)out_pitch, H, W, C, axis, new_len, bounds, kk, ksize, (hipStream_t)stream);
    return check_launch("ldx_image_resample_pass");
}
int ldx_image_box_blur_pass(const uint8_t* in, int64_t in_pitch, int H, int W, int axis, float box_radius, uint8_t* out, int64_t out_pitch, void* stream) {
    if (!image_ok(in, in_pitch, H, W, 1) || !image_ok(out, out_pitch, H, W, 1) || (axis != 0 && axis != 1) || in == out ||
        !(box_radius >= 0.0f) || !(box_radius < (float)(image_box_max_radius() + 1))) {
        set_error("ldx_image_box_blur_pass: bad argument (null pointer, axis 0 | 1, pitch < W, in == out, box radius outside [0, 256))"); return LDX_EINVAL; }
    launch_image_box_blur_pass(in, (long)in_pitch, out, (long)out_pitch, H, W, axis, box_radius, (hipStream_t)stream);
    return check_launch("ldx_image_box_blur_pass");
}
int ldx_image_composite(uint8_t* canvas, int64_t canvas_pitch, int H, int W, int C, int x0, int y0, int w, int h,
                        const uint8_t* tile, int64_t tile_pitch, const uint8_t* mask, int64_t mask_pitch, void* stream) {
    if (!image_ok(canvas, canvas_pitch, H, W, C) || !rect_ok(x0, y0, w, h, W, H) || !image_ok(tile, tile_pitch, h, w, C) || !image_ok(mask, mask_pitch, H, W, 1)) {
        set_error("ldx_image_composite: bad argument (null pointer, C not 1 | 3, pitch < W * C, rectangle outside the canvas)"); return LDX_EINVAL; }
    launch_image_composite(canvas + (int64_t)y0 * canvas_pitch + (int64_t)x0 * C, (long)canvas_pitch, tile, (long)tile_pitch,
                           mask + (int64_t)y0 * mask_pitch + x0, (long)mask_pitch, h, w, C, (hipStream_t)stream);
    return check_launch("ldx_image_composite");
}
int ldx_image_fill_rect(uint8_t* img, int64_t pitch, int H, int W, int C, int x0, int y0, int w, int h, int value, void* stream) {
    if (!image_ok(img, pitch, H, W, C) || !rect_ok(x0, y0, w, h, W, H) || value < 0 || value > 255) {
        set_error("ldx_image_fill_rect: bad argument (null pointer, C not 1 | 3, pitch < W * C, rectangle outside the image, value outside 0..255)"); return LDX_EINVAL; }
    launch_image_fill(img + (int64_t)y0 * pitch + (int64_t)x0 * C, (long)pitch, h, w * C, value, (hipStream_t)stream);
    return check_launch("ldx_image_fill_rect");
}
// ---- fp32 canvas ops of the ADetailer path (detail.hip) ---------------------------------------------------------------------------------
static bool canvas_ok(const void* p, int H, int W) { return p && H > 0 && W > 0 && (int64_t)H * W <= (int64_t)1 << 29; }
int ldx_detail_crop_quantize(const float* canvas, int H, int W, int x0, int y0, int w, int h, uint8_t* out, int64_t out_pitch, void* stream) {
    if (!canvas_ok(canvas, H, W) || !rect_ok(x0, y0, w, h, W, H) || !image_ok(out, out_pitch, h, w, 3)) {
        set_error("ldx_detail_crop_quantize: bad argument (null pointer, rectangle outside the canvas, pitch < w * 3)"); return LDX_EINVAL; }
    launch_detail_crop_quantize(canvas, W, x0, y0, w, h, out, (long)out_pitch, (hipStream_t)stream);
    return check_launch("ldx_detail_crop_quantize");
}
int ldx_detail_blur_mask(const float* in, int h, int w, const float* table, int k, float* out, void* stream) {
    if (!canvas_ok(in, h, w) || !table || !out || in == out || k < 1 || k > detail_max_kernel() || k % 2 == 0 || k / 2 >= h || k / 2 >= w) {
        set_error("ldx_detail_blur_mask: bad argument (null pointer, in == out, k even or outside 1..63, reflect padding k / 2 not below h and w)");
        return LDX_EINVAL;
    }
    launch_detail_blur_mask(in, h, w, table, k, out, (hipStream_t)stream);
    return check_launch("ldx_detail_blur_mask");
}
int ldx_detail_paste(float* canvas, int H, int W, int x0, int y0, const float* src, const float* mask, int h, int w, void* stream) {
    if (!canvas_ok(canvas, H, W) || !canvas_ok(src, h, w) || !mask || x0 < 0 || y0 < 0 || x0 >= W || y0 >= H) {
        set_error("ldx_detail_paste: bad argument (null pointer, empty tile, corner outside the canvas)"); return LDX_EINVAL; }
    launch_detail_paste(canvas, W, x0, y0, src, mask, w, (h < H - y0 ? h : H - y0), (w < W - x0 ? w : W - x0), (hipStream_t)stream);
    return check_launch("ldx_detail_paste");
}
// ---- AutoHDR (hdr.hip) -----------------------------------------------------------------------------------------------------------------------
static bool hdr_shape_ok(int B, int H, int W) { return B > 0 && B <= 65535 && H > 0 && W > 0 && (int64_t)H * W <= hdr_max_pixels(); }
int64_t ldx_hdr_workspace_bytes(int B, int H, int W) {
    if (!hdr_shape_ok(B, H, W)) { set_error("ldx_hdr_workspace_bytes: bad shape (1 <= B <= 65535, 1 <= H * W <= 16 843 009)"); return LDX_EINVAL; }
    return hdr_workspace_bytes(B, H, W);
}
int ldx_hdr_table(const uint8_t* in, int64_t in_pitch, int H, int W, const uint16_t* table, uint8_t* out, int64_t out_pitch, void* stream) {
    if (!image_ok(in, in_pitch, H, W, 3) || !image_ok(out, out_pitch, H, W, 3) || !table || (uintptr_t)table % 8) {
        set_error("ldx_hdr_table: bad argument (null pointer, pitch < W * 3, table not 8-byte aligned)"); return LDX_EINVAL; }
    launch_hdr_table(in, (long)in_pitch, out, (long)out_pitch, H, W, table, (hipStream_t)stream);
    return check_launch("ldx_hdr_table");
}
int ldx_hdr_apply(const float* in_f32, const uint8_t* in_u8, int64_t in_pitch, int B, int H, int W, const uint16_t* fwd, const uint16_t* inv,
                  const uint8_t* lum_lut, float contrast_factor, float color_factor, void* workspace, uint8_t* out_u8, int64_t out_pitch, float* out_f32,
                  void* stream) {
    const int64_t row = (int64_t)W * 3;
    if (!hdr_shape_ok(B, H, W) || (in_f32 != nullptr) == (in_u8 != nullptr) || (in_u8 && in_pitch < row) || (!out_u8 && !out_f32) || (out_u8 && out_pitch < row) ||
        !fwd || !inv || (uintptr_t)fwd % 8 || (uintptr_t)inv % 8 || !lum_lut || !workspace || (uintptr_t)workspace % 4 ||
        !(contrast_factor == contrast_factor) || !(color_factor == color_factor)) {
        set_error("ldx_hdr_apply: bad argument (1 <= B <= 65535, 1 <= H * W <= 16 843 009, exactly one input, at least one output, pitch < W * 3, "
                  "tables not 8-byte aligned, workspace null or not 4-byte aligned, NaN factor)");
        return LDX_EINVAL;
    }
    HdrArgs a{};
    a.in_f32 = in_f32; a.in_u8 = in_u8; a.in_pitch = (long)in_pitch; a.B = B; a.H = H; a.W = W; a.fwd = fwd; a.inv = inv; a.lut = lum_lut;
    a.f_contrast = contrast_factor; a.f_color = color_factor; a.workspace = workspace; a.out_u8 = out_u8; a.out_pitch = (long)out_pitch; a.out_f32 = out_f32;
    launch_hdr_apply(a, (hipStream_t)stream);
    return check_launch("ldx_hdr_apply");
}
// ---- SaveImage (png.hip) ---------------------------------------------------------------------------------------------------------------------
static bool png_shape_ok(int B, int H, int W) {
    return B > 0 && B <= 65535 && H > 0 && W > 0 && W <= (1 << 28) && (int64_t)H * (1 + 3 * (int64_t)W) <= png_max_stream_bytes();
}
int64_t ldx_png_workspace_bytes(int B, int H, int W) {
    if (!png_shape_ok(B, H, W)) { set_error("ldx_png_workspace_bytes: bad shape (1 <= B <= 65535, H, W >= 1, H * (1 + 3 W) <= 2^30)"); return LDX_EINVAL; }
    return png_workspace_bytes(B, H, W);
}
int64_t ldx_png_bound_bytes(int H, int W) {
    if (!png_shape_ok(1, H, W)) { set_error("ldx_png_bound_bytes: bad shape (H, W >= 1, H * (1 + 3 W) <= 2^30)"); return LDX_EINVAL; }
    return png_bound_bytes(H, W);
}
int ldx_png_filter(const float* in_f32, const uint8_t* in_u8, int64_t in_pitch, int B, int H, int W, uint8_t* filtered, uint8_t* types, void* stream) {
    if (!png_shape_ok(B, H, W) || (in_f32 != nullptr) == (in_u8 != nullptr) || (in_u8 && in_pitch < (int64_t)W * 3) || !filtered) {
        set_error("ldx_png_filter: bad argument (1 <= B <= 65535, H, W >= 1, H * (1 + 3 W) <= 2^30, exactly one input, pitch < W * 3, null output)");
        return LDX_EINVAL;
    }
    launch_png_filter(in_f32, in_u8, (long)in_pitch, B, H, W, filtered, types, (hipStream_t)stream);
    return check_launch("ldx_png_filter");
}
int ldx_png_encode(const float* in_f32, const uint8_t* in_u8, int64_t in_pitch, int B, int H, int W, void* workspace, uint8_t* out, int64_t out_stride,
                   uint32_t* out_len, void* stream) {
    if (!png_shape_ok(B, H, W) || (in_f32 != nullptr) == (in_u8 != nullptr) || (in_u8 && in_pitch < (int64_t)W * 3) || !workspace ||
        (uintptr_t)workspace % 16 || !out || !out_len || (uintptr_t)out_len % 4 || out_stride < png_bound_bytes(H, W)) {
        set_error("ldx_png_encode: bad argument (1 <= B <= 65535, H, W >= 1, H * (1 + 3 W) <= 2^30, exactly one input, pitch < W * 3, workspace null or "
                  "not 16-byte aligned, null output, out_stride < ldx_png_bound_bytes)");
        return LDX_EINVAL;
    }
    PngArgs a{};
    a.in_f32 = in_f32; a.in_u8 = in_u8; a.in_pitch = (long)in_pitch; a.B = B; a.H = H; a.W = W; a.workspace = workspace; a.out = out;
    a.out_stride = (long)out_stride; a.out_len = out_len;
    launch_png_encode(a, (hipStream_t)stream);
    return check_launch("ldx_png_encode");
}
int64_t ldx_zlib_workspace_bytes(int64_t n) {
    if (n <= 0 || n > png_max_stream_bytes()) { set_error("ldx_zlib_workspace_bytes: 1 <= n <= 2^30"); return LDX_EINVAL; }
    return zlib_workspace_bytes((long)n);
}
int64_t ldx_zlib_bound_bytes(int64_t n) {
    if (n <= 0 || n > png_max_stream_bytes()) { set_error("ldx_zlib_bound_bytes: 1 <= n <= 2^30"); return LDX_EINVAL; }
    return zlib_bound_bytes((long)n);
}
int ldx_zlib_deflate(const uint8_t* bytes, int64_t n, void* workspace, uint8_t* out, uint32_t* out_len, void* stream) {
    if (!bytes || n <= 0 || n > png_max_stream_bytes() || !workspace || (uintptr_t)workspace % 16 || !out || !out_len || (uintptr_t)out_len % 4) {
        set_error("ldx_zlib_deflate: bad argument (null pointer, 1 <= n <= 2^30, workspace not 16-byte aligned)"); return LDX_EINVAL; }
    launch_zlib_deflate(bytes, (long)n, workspace, out, out_len, (hipStream_t)stream);
    return check_launch("ldx_zlib_deflate");
}
int ldx_t5_create(const ldx_t5_config* cfg, int device, ldx_engine** out) { return create_engine<T5Engine>(cfg, device, out, __func__); }
int ldx_t5_encode(ldx_engine* e, const int32_t* ids, int B, int L, const float* bias, float* out, void* stream) {
    GUARD_BEGIN
    ENGINE_AS(T5Engine, m);
    return m->run((const int*)ids, B, L, bias, out, (hipStream_t)stream);
    GUARD_END
}
int ldx_flux_fbcache(ldx_engine* e, float residual_diff_threshold) {
    GUARD_BEGIN
    ENGINE_AS(FluxEngine, m, LDX_EINVAL);
    m->fb_threshold = residual_diff_threshold > 0.f ? residual_diff_threshold : 0.f;
    m->fb_reset(); m->fb_hits = m->fb_misses = 0;
    return LDX_OK;
    GUARD_END
}
int ldx_flux_set_fp8(ldx_engine* e, int enable) {
    GUARD_BEGIN
    ENGINE_AS(FluxEngine, m, LDX_EINVAL);
    if (m->finalized) { set_error("ldx_flux_set_fp8: call before ldx_finalize (the weights are quantised there)"); return LDX_ESTATE; }
    if (enable < 0 || enable > 3) { set_error("ldx_flux_set_fp8: mode must be 0 (off), 1 / 2 (linears) or 3 (linears + attention)"); return LDX_EINVAL; }
    m->fx_fp8 = enable != 0;
    m->fx_fp8_attn = enable == 3;        // 1 (= 2): the linears only, QK^T / PV stay 16-bit — what the mode has meant since round 2; 3: linears AND attention (explicit opt-in)
    return LDX_OK;
    GUARD_END
}
int ldx_flux_fbcache_stats(ldx_engine* e, int64_t* hits, int64_t* misses) {
    GUARD_BEGIN
    ENGINE_AS(FluxEngine, m, LDX_EINVAL);
    if (hits) *hits = m->fb_hits;
    if (misses) *misses = m->fb_misses;
    return LDX_OK;
    GUARD_END
}
int ldx_flux_create(const ldx_flux_config* cfg, int device, ldx_engine** out) { return create_engine<FluxEngine>(cfg, device, out, __func__); }
int ldx_flux_forward(ldx_engine* e, const float* x, const float* sigma, const float* ctx, const float* y, const float* guidance,
                     const float* pe_cos, const float* pe_sin, int B, int h, int w, int Lt, int denoise, float* out, void* stream) {
    GUARD_BEGIN
    ENGINE_AS(FluxEngine, m);
    return m->run(x, sigma, ctx, y, guidance, pe_cos, pe_sin, B, h, w, Lt, denoise != 0, out, (hipStream_t)stream);
    GUARD_END
}
int ldx_load_tensor(ldx_engine* e, const char* key, const void* data, int dtype, const int64_t* shape, int ndim) {
    GUARD_BEGIN
    ENGINE_AS(Engine, m);
    return m->load_tensor(key, data, dtype, shape, ndim);
    GUARD_END
}
int ldx_load_tensor_device(ldx_engine* e, const char* key, const void* dev_ptr, int dtype, const int64_t* shape, int ndim) {
    GUARD_BEGIN
    ENGINE_AS(UNetEngine, m);
    return m->load_tensor_dev(__func__, key, dev_ptr, dtype, shape, ndim);
    GUARD_END
}
int ldx_load_tensor_dev(ldx_engine* e, const char* key, const void* dev_ptr, int dtype, const int64_t* shape, int ndim) {
    GUARD_BEGIN
    ENGINE_AS(Engine, m);
    if (!m->takes_device_tensors()) { set_error("ldx_load_tensor_dev: not a UNet, Flux or T5 engine"); return LDX_ESTATE; }
    return m->load_tensor_dev(__func__, key, dev_ptr, dtype, shape, ndim);
    GUARD_END
}
int ldx_load_tensor_q8_0(ldx_engine* e, const char* key, const void* blocks, const int64_t* shape, int ndim, int on_device) {
    GUARD_BEGIN
    ENGINE_AS(Engine, m);
    if (!m->takes_q8_0()) { set_error("ldx_load_tensor_q8_0: not a Flux or T5 engine"); return LDX_ESTATE; }
    return m->load_tensor_q8_0(key, blocks, shape, ndim, on_device != 0);
    GUARD_END
}
int ldx_packed_digest(ldx_engine* e, uint64_t* out) {
    GUARD_BEGIN
    ENGINE_AS(Engine, m);
    return m->packed_digest(__func__, out);
    GUARD_END
}
int ldx_unet_refresh_begin(ldx_engine* e) {
    GUARD_BEGIN
    ENGINE_AS(UNetEngine, m);
    return m->refresh_begin();
    GUARD_END
}
int ldx_unet_refresh_commit(ldx_engine* e) {
    GUARD_BEGIN
    ENGINE_AS(UNetEngine, m);
    return m->refresh_commit();
    GUARD_END
}
int ldx_unet_refresh_abort(ldx_engine* e) {
    GUARD_BEGIN
    ENGINE_AS(UNetEngine, m);
    return m->refresh_abort();
    GUARD_END
}
int ldx_weights_digest(ldx_engine* e, uint64_t* out) {
    GUARD_BEGIN
    ENGINE_AS(UNetEngine, m);
    return m->packed_digest(__func__, out);
    GUARD_END
}
int ldx_set_tables(ldx_engine* e, const float* log_sigmas, int n, const float* temb, int temb_dim) {
    GUARD_BEGIN
    ENGINE_AS(UNetEngine, m);
    return m->set_tables(log_sigmas, n, temb, temb_dim);
    GUARD_END
}
int ldx_finalize(ldx_engine* e) {
    GUARD_BEGIN
    ENGINE_AS(Engine, m);
    return m->finalize();
    GUARD_END
}
int ldx_unet_denoise(ldx_engine* e, const float* x, const float* sigma, const float* ctx, int B2, int h, int w, int M, float* out, void* stream) {
    GUARD_BEGIN
    ENGINE_AS(UNetEngine, m);
    return m->run(x, sigma, ctx, B2, h, w, M, out, true, (hipStream_t)stream);
    GUARD_END
}
int ldx_unet_denoise_concat(ldx_engine* e, const float* x, const float* sigma, const float* ctx, const float* c_concat, int cc_channels, int B2, int h, int w, int M,
                            float* out, void* stream) {
    GUARD_BEGIN
    ENGINE_AS(UNetEngine, m);
    if (!c_concat) { set_error("ldx_unet_denoise_concat: c_concat is null (use ldx_unet_denoise)"); return LDX_EINVAL; }
    return m->run(x, sigma, ctx, B2, h, w, M, out, true, (hipStream_t)stream, 0, c_concat, cc_channels);
    GUARD_END
}
int ldx_unet_denoise_cfg(ldx_engine* e, const float* x, float sigma, const float* ctx, int B, int h, int w, int M, float* out, void* stream) {
    GUARD_BEGIN
    ENGINE_AS(UNetEngine, m);
    return m->run_cfg(x, sigma, ctx, B, h, w, M, out, (hipStream_t)stream);
    GUARD_END
}
int ldx_unet_denoise_cfg_t(ldx_engine* e, const float* x, float sigma, int t_index, const float* ctx, int B, int h, int w, int M, float* out, void* stream) {
    GUARD_BEGIN
    ENGINE_AS(UNetEngine, m);
    return m->run_cfg(x, sigma, ctx, B, h, w, M, out, (hipStream_t)stream, t_index < 0 ? -1 : t_index);
    GUARD_END
}
int ldx_unet_denoise_t(ldx_engine* e, const float* x, const float* sigma, const float* t_index, const float* ctx, int B2, int h, int w, int M, float* out, void* stream) {
    GUARD_BEGIN
    ENGINE_AS(UNetEngine, m);
    if (!t_index) { set_error("ldx_unet_denoise_t: t_index is null (use ldx_unet_denoise)"); return LDX_EINVAL; }
    return m->run(x, sigma, ctx, B2, h, w, M, out, true, (hipStream_t)stream, 0, nullptr, 0, t_index);
    GUARD_END
}
int ldx_unet_timestep(ldx_engine* e, const float* sigma, int n, int32_t* t_out, void* stream) {
    GUARD_BEGIN
    ENGINE_AS(UNetEngine, m);
    return m->timestep_lookup(sigma, n, (int*)t_out, (hipStream_t)stream);
    GUARD_END
}
int ldx_unet_forward(ldx_engine* e, const float* x, const float* t, const float* ctx, int B2, int h, int w, int M, float* out, void* stream) {
    GUARD_BEGIN
    ENGINE_AS(UNetEngine, m);
    return m->run(x, t, ctx, B2, h, w, M, out, false, (hipStream_t)stream);
    GUARD_END
}
int ldx_plan_info(ldx_engine* e, int64_t* n_launches, double* flops, int64_t* arena_bytes) {
    ENGINE_AS(Engine, m);
    if (n_launches) *n_launches = m->n_launches();
    if (flops) *flops = m->algorithmic_flops();
    if (arena_bytes) *arena_bytes = (int64_t)m->cur.arena_cap;
    return LDX_OK;
}
int ldx_plan_flops(ldx_engine* e, double* executed, double* shared) {
    ENGINE_AS(Engine, m);
    if (executed) *executed = m->steady_flops();
    if (shared) *shared = m->cur.flops_shared;
    return LDX_OK;
}
int ldx_unet_cfg_share(ldx_engine* e, int enable) {
    ENGINE_AS(UNetEngine, m);
    m->cfg_share = enable < 0 ? 0 : (enable > 2 ? 2 : enable);
    return LDX_OK;
}
int ldx_profile(ldx_engine* e, int enable, int reset) {
    ENGINE_AS(Engine, m);
    m->profiling = enable != 0;
    m->prof_detail = enable == 2;
    if (reset) m->prof.clear();
    return LDX_OK;
}
int ldx_profile_report(ldx_engine* e, char* buf, int64_t cap) {
    if (!e || !buf || cap <= 0) { set_error("ldx_profile_report: bad argument"); return LDX_EINVAL; }
    const std::string s = e->impl->profile_json();
    if ((int64_t)s.size() + 1 > cap) { set_error("ldx_profile_report: buffer too small"); return LDX_EINVAL; }
    memcpy(buf, s.c_str(), s.size() + 1);
    return LDX_OK;
}
int ldx_set_graph_mode(ldx_engine* e, int enable) {
    ENGINE_AS(Engine, m);
    m->graph_mode = enable != 0;
    return LDX_OK;
}
int ldx_unet_context_cache(ldx_engine* e, int enable) {
    ENGINE_AS(UNetEngine, m);
    return m->set_context_cache(enable);
}
int ldx_reload_env(void) {
    reload_dispatch_env();
    return LDX_OK;
}
int ldx_graph_stats(ldx_engine* e, int64_t* captures, int64_t* replays) {
    if (!e || !captures || !replays) { set_error("ldx_graph_stats: bad argument"); return LDX_EINVAL; }
    *captures = e->impl->n_graph_captures; *replays = e->impl->n_graph_replays;
    return LDX_OK;
}

int ldx_sampler_step(int kind, float* x, const float* du, const float* dc, float* dout, int64_t n, float cfg, float c0, float c1, void* stream) {
    if (!x || !du || !dc || n < 0 || (kind < 0 || kind > 3)) { set_error("ldx_sampler_step: bad argument"); return LDX_EINVAL; }
    if (kind == 2 && !dout) { set_error("ldx_sampler_step: kind 2 (CFG combine only) needs denoised_out"); return LDX_EINVAL; }
    if (kind == 0 && c0 == 0.f) { set_error("ldx_sampler_step: kind 0 (Euler) divides by c0 = sigma_hat, which must be non-zero"); return LDX_EINVAL; }
    StepArgs a{x, du, dc, dout, (size_t)n, cfg, kind, c0, c1};
    launch_sampler_step(a, (hipStream_t)stream);
    return check_launch("ldx_sampler_step");
}
int ldx_bislerp_pass(const float* in, float* out, int N, int C, int H, int W, int axis, int new_len,
                     const int32_t* c1, const int32_t* c2, const float* ratios, void* stream) {
    if (!in || !out || !c1 || !c2 || !ratios || N <= 0 || C <= 0 || C > 16 || H <= 0 || W <= 0 || new_len <= 0 || (axis != 0 && axis != 1)) {
        set_error("ldx_bislerp_pass: bad argument (C <= 16, axis 0|1)"); return LDX_EINVAL; }
    launch_bislerp_pass(in, out, N, C, H, W, axis, new_len, (const int*)c1, (const int*)c2, ratios, (hipStream_t)stream);
    return check_launch("ldx_bislerp_pass");
}
int ldx_vae_encode(ldx_engine* e, const float* pixels_nhwc, int B, int H, int W, float* moments_nchw, void* stream) {
    GUARD_BEGIN
    ENGINE_AS(VaeEngine, m);
    return m->run_encode(pixels_nhwc, B, H, W, moments_nchw, (hipStream_t)stream);
    GUARD_END
}
int ldx_bilinear(const float* in, float* out, int planes, int hin, int win, int hout, int wout, void* stream) {
    if (!in || !out || planes <= 0 || hin <= 0 || win <= 0 || hout <= 0 || wout <= 0) { set_error("ldx_bilinear: bad argument"); return LDX_EINVAL; }
    launch_bilinear(in, out, planes, hin, win, hout, wout, (hipStream_t)stream);
    return check_launch("ldx_bilinear");
}

int ldx_op_convert(const float* in_f32, void* out_16, int64_t n, int dtype, int to_f32, void* stream) {
    if (!in_f32 || !out_16 || n < 0) { set_error("ldx_op_convert: bad argument"); return LDX_EINVAL; }
    if (to_f32) launch_t_to_f32(out_16, (float*)in_f32, (size_t)n, dtype_of(dtype), (hipStream_t)stream);
    else launch_f32_to_t(in_f32, out_16, (size_t)n, dtype_of(dtype), (hipStream_t)stream);
    return check_launch("ldx_op_convert");
}
int ldx_op_dequant_q8_0(const void* blocks, int64_t n, int out_dtype, void* out, void* stream) {
    if (!blocks || (uintptr_t)blocks % 2 || !out || (uintptr_t)out % 16 || n < 0 || n % Q8_0_BLOCK || (out_dtype != LDX_F16 && out_dtype != LDX_BF16 && out_dtype != LDX_F32)) {
        set_error("ldx_op_dequant_q8_0: bad argument (null or odd block pointer, out not 16-byte aligned, n % 32, out_dtype)"); return LDX_EINVAL; }
    launch_dequant_q8_0(DequantQ8Args{blocks, out, (size_t)n, out_dtype}, (hipStream_t)stream);
    return check_launch("ldx_op_dequant_q8_0");
}
int ldx_op_gemm(const void* A, int lda, const void* W, int M, int N, int K, const float* bias, const float* rowvec, int rowvec_ld,
                int rows_per_batch, int geglu, const void* R, int ldr, void* C, int ldc, float* Cf, int ldcf, int dtype, void* stream) {
    if (!A || !W || M <= 0 || N <= 0 || K <= 0 || K % 8 || lda % 8 || (!C && !Cf)) { set_error("ldx_op_gemm: bad argument (K % 8, lda % 8)"); return LDX_EINVAL; }
    GemmArgs g = gemm_linear_args(A, lda, W, M, N, K);
    g.bias = bias; g.rowvec = rowvec; g.rowvec_ld = rowvec_ld; if (rows_per_batch > 0) g.rows_per_batch = rows_per_batch;
    g.geglu = geglu; g.R = R; g.ldr = ldr; g.C = C; g.ldc = ldc; g.Cf = Cf; g.ldcf = ldcf;
    if (int rc = attach_splitk(g)) return rc;
    launch_gemm(g, dtype_of(dtype), (hipStream_t)stream);
    return check_launch("ldx_op_gemm");
}
int ldx_op_layernorm_mx(const void* X, int ldx_, int rows, int C, float eps, const float* gamma, const float* beta,
                        void* Y8, int ldy8, void* S8, int s8_ld, int dtype, void* stream) {
    if (!X || !Y8 || !S8 || !gamma || !beta || rows <= 0 || C % 128 || C > 4096 || ldx_ % 8 || ldy8 % 16 || ldy8 < C || s8_ld < rows) {
        set_error("ldx_op_layernorm_mx: bad argument (C % 128, C <= 4096, ldy8 % 16, s8_ld >= rows)"); return LDX_EINVAL; }
    LayerNormArgs a{X, ldx_, nullptr, 0, rows, C, eps, gamma, beta};
    a.Y8 = Y8; a.ldy8 = ldy8; a.S8 = (uint32_t*)S8; a.s8_ld = s8_ld;
    launch_layernorm(a, dtype_of(dtype), (hipStream_t)stream);
    return check_launch("ldx_op_layernorm_mx");
}
int ldx_op_attention_mx(const void* Q, int ldq, const void* K, int ldk, const void* V, int ldv, void* O8, int ldo8, void* SO, int so_ld,
                        int B, int H, int Nq, int Mk, float scale, int dtype, void* stream) {
    AttnArgs a = attn_args(Q, ldq, K, ldk, V, ldv, nullptr, 0, B, H, Nq, Mk, 128, scale);
    a.O8 = O8; a.ldo8 = ldo8; a.SO = (uint32_t*)SO; a.so_ld = so_ld;
    if (!Q || !K || !V || !O8 || !SO || B <= 0 || H <= 0 || Nq <= 0 || Mk <= 0 || ldq % 8 || ldk % 8 || ldv % 8 || ldo8 % 16 || ldo8 < H * 128 || so_ld < B * Nq) {
        set_error("ldx_op_attention_mx: bad argument"); return LDX_EINVAL; }
    if (!attn_attach_scratch(a, op_scratch).mx_out) { set_error("ldx_op_attention_mx: needs head dim 128 and at least 16 query blocks of 128 (B * H * ceil(Nq / 128))"); return LDX_EINVAL; }
    launch_attention(a, dtype_of(dtype), (hipStream_t)stream);
    return check_launch("ldx_op_attention_mx");
}
int ldx_op_mx_vt_quant(const void* V, int ldv, int B, int H, int L, void* V8T, void* SV, int Lp, int dtype, void* stream) {
    if (!V || !V8T || !SV || B <= 0 || H <= 0 || L <= 0 || ldv % 8 || Lp % 128 || Lp < L) { set_error("ldx_op_mx_vt_quant: bad argument (ldv % 8, Lp % 128 == 0, Lp >= L)"); return LDX_EINVAL; }
    MxVtArgs a{V, ldv, B, H, L, V8T, (uint32_t*)SV, Lp};
    launch_mx_vt_quant(a, dtype_of(dtype), (hipStream_t)stream);
    return check_launch("ldx_op_mx_vt_quant");
}
int ldx_op_attention_fp8(const void* Q8, int ldq8, const void* SQ, int sq_ld, const void* K8, int ldk8, const void* SK, int sk_ld, const void* V8T, const void* SV, int Lp,
                         void* O, int ldo, void* O8, int ldo8, void* SO, int so_ld, int B, int H, int Nq, int Mk, float scale, int dtype, void* stream) {
    AttnMxArgs a{};
    a.Q8 = Q8; a.ldq8 = ldq8; a.SQ = (const uint32_t*)SQ; a.sq_ld = sq_ld; a.K8 = K8; a.ldk8 = ldk8; a.SK = (const uint32_t*)SK; a.sk_ld = sk_ld;
    a.V8T = V8T; a.SV = (const uint32_t*)SV; a.Lp = Lp; a.O = O; a.ldo = ldo; a.O8 = O8; a.ldo8 = ldo8; a.SO = (uint32_t*)SO; a.so_ld = so_ld;
    a.B = B; a.H = H; a.Nq = Nq; a.Mk = Mk; a.scale = scale;
    if (!attn_mx_ok(a) || sq_ld < B * Nq || sk_ld < B * Mk) { set_error("ldx_op_attention_fp8: bad argument (head dim 128; ld % 16; Lp % 128 == 0, Lp >= Mk; scale strides >= rows)"); return LDX_EINVAL; }
    launch_attn_mx(a, dtype_of(dtype), (hipStream_t)stream);
    return check_launch("ldx_op_attention_fp8");
}
int ldx_op_qk_norm_rope_mx(const void* QKV, int ld, int rows, int L, int H, const float* qscale, const float* kscale, const float* cosT, const float* sinT, float eps,
                           void* Q8, void* K8, int ld8, void* SQ, void* SK, int s_ld, int dtype, void* stream) {
    if (!QKV || !qscale || !kscale || !cosT || !sinT || !Q8 || !K8 || !SQ || !SK || rows <= 0 || L <= 0 || H <= 0 || ld % 8 || ld8 % 16 || ld8 < H * 128 || s_ld < rows) {
        set_error("ldx_op_qk_norm_rope_mx: bad argument (head dim 128; ld % 8, ld8 % 16, s_ld >= rows)"); return LDX_EINVAL; }
    QkRopeArgs a{};
    a.QKV = (void*)QKV; a.ld = ld; a.rows = rows; a.L = L; a.H = H; a.D = 128; a.qscale = qscale; a.kscale = kscale; a.cosT = cosT; a.sinT = sinT; a.eps = eps;
    a.Q8 = Q8; a.K8 = K8; a.ld8 = ld8; a.SQ = (uint32_t*)SQ; a.SK = (uint32_t*)SK; a.s8_ld = s_ld; a.row8 = 0;
    launch_qk_norm_rope_mx(a, dtype_of(dtype), (hipStream_t)stream);
    return check_launch("ldx_op_qk_norm_rope_mx");
}
int ldx_op_mx_quant(const void* X, int ldx_, int rows, int K, void* Y, int ldy, void* scales, int scales_ld, int dtype, void* stream) {
    if (!X || !Y || !scales || rows <= 0 || K <= 0 || K % 128 || ldx_ % 8 || ldy % 16 || ldy < K || scales_ld < rows) {
        set_error("ldx_op_mx_quant: bad argument (K % 128, ldx % 8, ldy % 16, scales_ld >= rows)"); return LDX_EINVAL; }
    MxQuantArgs a{X, ldx_, rows, K, Y, ldy, (uint32_t*)scales, scales_ld};
    launch_mx_quant(a, dtype_of(dtype), (hipStream_t)stream);
    return check_launch("ldx_op_mx_quant");
}
int ldx_op_gemm_mx(const void* A8, int lda, const void* SA, int sa_ld, const void* W8, const void* SW, int sw_ld, int M, int N, int K,
                   const float* bias, int act, const void* R, int ldr, void* C, int ldc, float* Cf, int ldcf,
                   void* C8, int ldc8, void* SC, int sc_ld, int dtype, void* stream) {
    if (!A8 || !W8 || !SA || !SW || M <= 0 || N <= 0 || K <= 0 || K % 128 || lda % 16 || sa_ld < M || sw_ld < N || (!C && !Cf && !C8) || act < 0 || act > 3) {
        set_error("ldx_op_gemm_mx: bad argument (K % 128, lda % 16, sa_ld >= M, sw_ld >= N)"); return LDX_EINVAL; }
    if (C8 && (!SC || N % 128 || ldc8 % 16 || ldc8 < N || sc_ld < M || R || C || Cf)) {
        set_error("ldx_op_gemm_mx: MX output needs N % 128 == 0, ldc8 % 16 == 0, scales_ld >= M and no other output / residual"); return LDX_EINVAL; }
    GemmArgs g = gemm_linear_args(A8, lda, W8, M, N, K);
    gemm_mx_operands(g, (const uint32_t*)SA, sa_ld, W8, (const uint32_t*)SW, sw_ld);
    g.bias = bias; g.act = act; g.R = R; g.ldr = ldr; g.C = C; g.ldc = ldc; g.Cf = Cf; g.ldcf = ldcf; g.C8 = C8; g.ldc8 = ldc8; g.SC = (uint32_t*)SC; g.sc_ld = sc_ld;
    if (int rc = attach_splitk(g)) return rc;
    launch_gemm(g, dtype_of(dtype), (hipStream_t)stream);
    return check_launch("ldx_op_gemm_mx");
}
int ldx_op_gemm2(const void* A1, int lda1, const void* W1, int M1, int N1, int K1, const float* bias1, void* C1, int ldc1,
                 const void* A2, int lda2, const void* W2, int M2, int N2, int K2, const float* bias2, void* C2, int ldc2, int dtype, void* stream) {
    if (!A1 || !W1 || !C1 || !A2 || !W2 || !C2 || M1 <= 0 || N1 <= 0 || K1 <= 0 || M2 <= 0 || N2 <= 0 || K2 <= 0 || K1 % 8 || K2 % 8 || lda1 % 8 || lda2 % 8) {
        set_error("ldx_op_gemm2: bad argument (K % 8, lda % 8)"); return LDX_EINVAL; }
    GemmArgs a = gemm_linear_args(A1, lda1, W1, M1, N1, K1), b = gemm_linear_args(A2, lda2, W2, M2, N2, K2);
    a.bias = bias1; a.C = C1; a.ldc = ldc1; b.bias = bias2; b.C = C2; b.ldc = ldc2;
    launch_gemm2(a, b, dtype_of(dtype), (hipStream_t)stream);
    return check_launch("ldx_op_gemm2");
}
int ldx_op_gemm2_mx(const void* A1, int lda1, const void* SA1, int sa_ld1, const void* W1, const void* SW1, int sw_ld1, int M1, int N1, int K1,
                    const float* bias1, void* C1, int ldc1,
                    const void* A2, int lda2, const void* SA2, int sa_ld2, const void* W2, const void* SW2, int sw_ld2, int M2, int N2, int K2,
                    const float* bias2, void* C2, int ldc2, int dtype, void* stream) {
    if (!A1 || !W1 || !SA1 || !SW1 || !C1 || !A2 || !W2 || !SA2 || !SW2 || !C2 || M1 <= 0 || N1 <= 0 || K1 <= 0 || M2 <= 0 || N2 <= 0 || K2 <= 0 ||
        K1 % 128 || K2 % 128 || lda1 % 16 || lda2 % 16 || sa_ld1 < M1 || sw_ld1 < N1 || sa_ld2 < M2 || sw_ld2 < N2) {
        set_error("ldx_op_gemm2_mx: bad argument (K % 128, lda % 16, sa_ld >= M, sw_ld >= N)"); return LDX_EINVAL; }
    GemmArgs a = gemm_linear_args(A1, lda1, W1, M1, N1, K1), b = gemm_linear_args(A2, lda2, W2, M2, N2, K2);
    gemm_mx_operands(a, (const uint32_t*)SA1, sa_ld1, W1, (const uint32_t*)SW1, sw_ld1);
    gemm_mx_operands(b, (const uint32_t*)SA2, sa_ld2, W2, (const uint32_t*)SW2, sw_ld2);
    a.bias = bias1; a.C = C1; a.ldc = ldc1; b.bias = bias2; b.C = C2; b.ldc = ldc2;
    launch_gemm2(a, b, dtype_of(dtype), (hipStream_t)stream);
    return check_launch("ldx_op_gemm2_mx");
}
int ldx_op_gemm_pick(int M, int N, int K, int mode, int geglu, int splitk, int f8, int c8, int ln_fold,
                     int Cin, int Hin, int Win, int Hout, int Wout, int stride, int M2, int N2, int K2,
                     int gn_hw, int gn_groups, int gn_max_chunks, int32_t* out) {
    if (!out || M <= 0 || N <= 0 || K <= 0 || (mode != 0 && mode != 1) || (mode == 1 && (Cin <= 0 || Hout <= 0 || Wout <= 0 || (M2 > 0)))) {
        set_error("ldx_op_gemm_pick: bad argument"); return LDX_EINVAL; }
    void* const P = pick_operand;
    // the planner's geometry (resize to the output extent at stride 1) for one image, then the caller's M
    GemmArgs g = mode ? gemm_conv_args(P, Cin, P, 1, Hin, Win, Cin, N, K, stride, Hout, Wout, stride == 1) : gemm_linear_args(P, K, P, M, N, K);
    g.M = M; g.geglu = geglu;
    if (mode && K > 9 * Cin) { g.A2 = P; g.lda2 = g.Cin2 = K - 9 * Cin; }
    if (f8) gemm_mx_operands(g, (const uint32_t*)P, M, P, (const uint32_t*)P, N);
    if (c8) { g.C8 = P; g.ldc8 = N; g.SC = (uint32_t*)P; g.sc_ld = M; } else { g.C = P; g.ldc = N; }
    if (ln_fold) g.ln_c1 = (const float*)P;
    if (splitk < 0) gemm_attach_splitk(g, pick_scratch);
    else if ((g.splitk = splitk) > 1) { g.ws = (float*)P; g.sk_count = (unsigned*)P; }      // the caller's K splits instead of the rule's
    GemmArgs b = gemm_linear_args(P, K2, P, M2, N2, K2); b.C = P; b.ldc = N2; b.f8 = g.f8;
    int gn = 0;
    if (gn_hw > 0 && M2 <= 0 && (gn = gemm_gn_fuse(g, gn_hw, gn_groups, gn_max_chunks)) != 0) g.gn_partial = (float*)P;
    const GemmPick p = gemm_pick(g, M2 > 0 ? &b : nullptr);
    const int32_t r[10] = {p.family, p.bm, p.bn, p.wm, p.f8, p.lnf, p.S, p.reduce, p.launches, gn};
    for (int i = 0; i < 10; ++i) out[i] = r[i];
    return LDX_OK;
}
int ldx_op_attn_pick(int B, int H, int Nq, int Mk, int D, int causal, int bias, int o8, int ldq, int ldk, int ldv, int ldo, int knorm_ws, int32_t* out) {
    if (!out || B <= 0 || H <= 0 || Nq <= 0 || Mk <= 0 || D <= 0 || D % 8 || (D > 160 && D != 512) || ldq <= 0 || ldk <= 0 || ldv <= 0 || ldo <= 0 || (o8 && D != 128)) {
        set_error("ldx_op_attn_pick: bad argument (D % 8, D <= 160 or D == 512; MX fp8 output: D == 128)"); return LDX_EINVAL; }
    void* const P = pick_operand;
    AttnArgs a = attn_args(P, ldq, P, ldk, P, ldv, P, ldo, B, H, Nq, Mk, D, 1.f); a.causal = causal;
    if (bias) { a.bias = (const float*)P; a.bias_ld = (Mk + 63) / 64 * 64; }
    if (o8) { a.O8 = P; a.ldo8 = ldo; a.SO = (uint32_t*)P; a.so_ld = B * Nq; }
    AttnPick p = attn_attach_scratch(a, pick_scratch);      // as the planner and ldx_op_attention launch it ...
    if (!knorm_ws && a.knorm_ws) { a.knorm_ws = nullptr; p = attn_pick(a); }      // ... or, on request, without the key-block norms
    const int32_t r[13] = {p.family, p.targ[0], p.targ[1], p.targ[2], p.kpf, p.qb, p.block, (int32_t)p.grid, p.lds, p.knorm, p.nsplit, p.mx_out, p.launches};
    for (int i = 0; i < 13; ++i) out[i] = r[i];
    return LDX_OK;
}
int ldx_op_xf_pick(int C, int heads, int B, int HW, int Mc, int share, int ln_fold, int gn_stats_chunks, int32_t* out) {
    if (!out || C <= 0 || heads <= 0 || C % heads || B <= 0 || HW <= 0 || Mc <= 0 || share < 0 || share > B || gn_stats_chunks < 0) {
        set_error("ldx_op_xf_pick: bad argument (positive sizes, C % heads == 0, 0 <= share <= B)"); return LDX_EINVAL; }
    const XfPick p = xf_pick(XfShape{C, heads, B, HW, Mc, share, ln_fold != 0, gn_stats_chunks});
    int n = 0;
    out[n++] = p.fold; out[n++] = p.proj_in_rowgemm; out[n++] = p.proj_out;
    for (const XfBlockPick* b : {&p.first, &p.rest})
        for (int v : {(int)b->qkv, (int)b->o1, (int)b->xattn, (int)b->q2, (int)b->o2, (int)b->ffblock, (int)b->ff1, b->ops}) out[n++] = v;
    out[n++] = p.ops_outer;
    return LDX_OK;
}
int ldx_op_conv3x3(const void* X, int ldx_, const void* W, int B, int Hin, int Win, int Cin, int Cout, int stride, int Hout, int Wout,
                   int resize_to_out, const float* bias, const float* rowvec, int rowvec_ld, const void* R, int ldr, void* Y, int ldy,
                   int dtype, void* stream) {
    if (!X || !W || !Y || Cin % 64 || ldx_ % 8 || (stride != 1 && stride != 2)) { set_error("ldx_op_conv3x3: bad argument (Cin % 64)"); return LDX_EINVAL; }
    GemmArgs g = gemm_conv_args(X, ldx_, W, B, Hin, Win, Cin, Cout, 9 * Cin, stride, Hout, Wout, resize_to_out != 0);
    g.bias = bias; g.rowvec = rowvec; g.rowvec_ld = rowvec_ld; g.R = R; g.ldr = ldr; g.C = Y; g.ldc = ldy;
    if (int rc = attach_splitk(g)) return rc;
    launch_gemm(g, dtype_of(dtype), (hipStream_t)stream);
    return check_launch("ldx_op_conv3x3");
}
int ldx_op_upconv2x(const void* X, int ldx_, const void* W9, int B, int Hin, int Win, int Cin, int Cout, const float* bias, void* Y, int ldy, int dtype, void* stream) {
    if (!X || !W9 || !Y || !bias || B <= 0 || Hin <= 0 || Win <= 0 || Cin <= 0 || Cout <= 0 || ldx_ % 8 || ldx_ < Cin || ldy % 4 || ldy < Cout) {
        set_error("ldx_op_upconv2x: bad argument (X, W9, bias, Y; ldx % 8, ldy % 4)"); return LDX_EINVAL; }
    GemmArgs g = gemm_conv_args(X, ldx_, W9, B, Hin, Win, Cin, Cout, 9 * Cin, 1, 2 * Hin, 2 * Win, true), ph;
    g.bias = bias; g.C = Y; g.ldc = ldy;
    if (!gemm_upconv_phase(g, false, &ph)) { set_error("ldx_op_upconv2x: no phase form for this shape (Win % 16, Cin % 64, Cout % 16)"); return LDX_EINVAL; }
    void* wp = op_workspace((size_t)16 * Cout * Cin / 2);      // [4][Cout][4 Cin] 16-bit
    if (!wp) { set_error("ldx_op_upconv2x: workspace allocation failed"); return LDX_EHIP; }
    launch_up_phase(up_phase_args(W9, wp, Cout, Cin, dtype_of(dtype)), (hipStream_t)stream);
    ph.W = wp; ph.up2x = 2;        // phase-major tiles, as the engine plans it
    launch_gemm(ph, dtype_of(dtype), (hipStream_t)stream);
    return check_launch("ldx_op_upconv2x");
}
int ldx_op_conv3x3_skip(const void* X, int ldx_, const void* X2, int ldx2, int Cin2, const void* W, int B, int H, int Wd, int Cin, int Cout,
                        const float* bias, void* Y, int ldy, int dtype, void* stream) {
    if (!X || !X2 || !W || !Y || Cin % 64 || Cin2 % 64 || ldx_ % 8 || ldx2 % 8 || B <= 0 || H <= 0 || Wd <= 0) {
        set_error("ldx_op_conv3x3_skip: bad argument (Cin % 64, Cin2 % 64)"); return LDX_EINVAL; }
    GemmArgs g = gemm_conv_args(X, ldx_, W, B, H, Wd, Cin, Cout, 9 * Cin + Cin2, 1, H, Wd, false);
    g.A2 = X2; g.lda2 = ldx2; g.Cin2 = Cin2; g.bias = bias; g.C = Y; g.ldc = ldy;
    if (int rc = attach_splitk(g)) return rc;
    launch_gemm(g, dtype_of(dtype), (hipStream_t)stream);
    return check_launch("ldx_op_conv3x3_skip");
}
// The producers of GroupNorm statistics as the planner launches them (Engine::fuse_gn_stats): the arguments are complete but for the statistics; ask gemm_gn_fuse,
// refuse before anything is launched where it says no (so launch_gemm's gemm_gn_check can never fire from here), else point the launch at the caller's rows.
static int launch_gemm_gn(GemmArgs& g, int HW, float* partial, int gn_groups, int max_chunks, int32_t* nchunk_out, int dtype, void* stream, const char* fn) {
    if (int rc = attach_splitk(g)) return rc;
    const int nchunk = gemm_gn_fuse(g, HW, gn_groups, max_chunks);
    if (!nchunk) { set_error(std::string(fn) + ": this launch does not produce GroupNorm statistics (gemm_gn_fuse: kernel, tile or chunk count; the one-launch small GroupNorm)"); return LDX_EINVAL; }
    g.gn_partial = partial;
    launch_gemm(g, dtype_of(dtype), (hipStream_t)stream);
    *nchunk_out = nchunk;
    return check_launch(fn);
}
int ldx_op_conv3x3_gn(const void* X, int ldx_, const void* X2, int ldx2, int Cin2, const void* W, int B, int Hin, int Win, int Cin, int Cout, int stride, int Hout, int Wout,
                      int resize_to_out, const float* bias, const float* rowvec, int rowvec_ld, const void* R, int ldr, void* Y, int ldy, int64_t dup_rows,
                      float* partial, int gn_groups, int max_chunks, int32_t* nchunk_out, int dtype, void* stream) {
    if (!X || !W || !Y || !partial || !nchunk_out || B <= 0 || Hin <= 0 || Win <= 0 || Hout <= 0 || Wout <= 0 || Cin <= 0 || Cin % 64 || Cout <= 0 || ldx_ % 8 || ldx_ < Cin ||
        (stride != 1 && stride != 2) || ldy % 8 || ldy < Cout || (R && (ldr % 8 || ldr < Cout)) || (rowvec && rowvec_ld < Cout) || dup_rows < 0 || gn_groups <= 0 || max_chunks <= 0 ||
        Cin2 < 0 || (Cin2 && (!X2 || Cin2 % 64 || ldx2 % 8 || ldx2 < Cin2 || stride != 1 || Hout != Hin || Wout != Win || resize_to_out))) {
        set_error("ldx_op_conv3x3_gn: bad argument (Cin % 64, Cin2 % 64, ldx % 8, ldy % 8, ldr % 8; the fused skip: stride 1, output extent = input extent)"); return LDX_EINVAL; }
    GemmArgs g = gemm_conv_args(X, ldx_, W, B, Hin, Win, Cin, Cout, 9 * Cin + Cin2, stride, Hout, Wout, resize_to_out != 0);
    if (Cin2) { g.A2 = X2; g.lda2 = ldx2; g.Cin2 = Cin2; }
    g.bias = bias; g.rowvec = rowvec; g.rowvec_ld = rowvec_ld; g.R = R; g.ldr = ldr; g.C = Y; g.ldc = ldy; g.dup_rows = (long)dup_rows;
    return launch_gemm_gn(g, Hout * Wout, partial, gn_groups, max_chunks, nchunk_out, dtype, stream, __func__);
}
int ldx_op_gemm_gn(const void* A, int lda, const void* W, int M, int N, int K, const float* bias, const float* rowvec, int rowvec_ld, int rows_per_batch,
                   const void* R, int ldr, void* C, int ldc, float* Cf, int ldcf, int gn_hw, float* partial, int gn_groups, int max_chunks, int32_t* nchunk_out,
                   int dtype, void* stream) {
    if (!A || !W || !C || !partial || !nchunk_out || M <= 0 || N <= 0 || K <= 0 || K % 8 || lda % 8 || lda < K || ldc % 8 || ldc < N || (R && (ldr % 8 || ldr < N)) ||
        (rowvec && rowvec_ld < N) || (Cf && ldcf < N) || gn_hw <= 0 || M % gn_hw || gn_groups <= 0 || max_chunks <= 0) {
        set_error("ldx_op_gemm_gn: bad argument (K % 8, lda % 8, ldc % 8, ldr % 8, M % gn_hw; a 16-bit C is required)"); return LDX_EINVAL; }
    GemmArgs g = gemm_linear_args(A, lda, W, M, N, K);
    g.bias = bias; g.rowvec = rowvec; g.rowvec_ld = rowvec_ld; if (rows_per_batch > 0) g.rows_per_batch = rows_per_batch;
    g.R = R; g.ldr = ldr; g.C = C; g.ldc = ldc; g.Cf = Cf; g.ldcf = ldcf;
    return launch_gemm_gn(g, gn_hw, partial, gn_groups, max_chunks, nchunk_out, dtype, stream, __func__);
}
int ldx_op_rowgemm_gn(const void* X, int ldx_, void* Y, int ldy, int64_t M, int N, int K, const void* W, const float* bias, const void* R, int ldr,
                      int pro, const float* gamma, const float* beta, float eps, int HW, int64_t dup_rows, float* gn_out, int max_chunks, int32_t* nchunk_out,
                      int dtype, void* stream) {
    RowGemmArgs a{};
    a.X = X; a.ldx = ldx_; a.Y = Y; a.ldy = ldy; a.M = (long)M; a.N = N; a.K = K; a.W = W; a.bias = bias; a.R = R; a.ldr = ldr;
    a.pro = pro; a.g = gamma; a.b = beta; a.eps = eps; a.HW = HW; a.G = 32; a.dup_rows = (long)dup_rows;
    if (!X || !Y || !W || !gn_out || !nchunk_out || ldx_ < K || ldy < N || (R && ldr < N) || pro < 0 || pro > 1 || dup_rows < 0 || max_chunks <= 0 || !rowgemm_ok(a)) {
        set_error("ldx_op_rowgemm_gn: shape not taken (K = 320 or 640, N a multiple of K, pro 0 or 1)"); return LDX_EINVAL; }
    const int nchunk = rowgemm_gn_chunks(a, HW, 32, max_chunks);
    if (!nchunk) { set_error("ldx_op_rowgemm_gn: this launch does not produce GroupNorm statistics (N == K, HW a multiple of the row block, M of HW; the one-launch small GroupNorm)"); return LDX_EINVAL; }
    a.gn_out = gn_out; a.gn_nchunk = nchunk;
    launch_rowgemm(a, dtype_of(dtype), (hipStream_t)stream);
    *nchunk_out = nchunk;
    return check_launch("ldx_op_rowgemm_gn");
}
int64_t ldx_op_groupnorm_workspace_floats(int B, int G) { return (int64_t)B * GN_NCHUNK * G * 2; }
int64_t ldx_op_groupnorm_stats_floats(int B, int G, int stats_chunks) {
    if (B <= 0 || G <= 0 || stats_chunks <= 0) return 0;
    return (int64_t)B * ((int64_t)stats_chunks + GN_FOLD) * G * 2;
}
int ldx_op_groupnorm_stats(const void* X, int ldx_, void* Y, int ldy, int B, int HW, int C, int G, float eps, int silu,
                           const float* gamma, const float* beta, float* partial, int stats_chunks, int dtype, void* stream) {
    if (!X || !Y || !gamma || !beta || !partial || B <= 0 || HW <= 0 || C <= 0 || G <= 0 || C % 8 || C % G || G > 32 || ldx_ % 8 || ldy % 8 || ldx_ < C || ldy < C ||
        stats_chunks <= 0 || stats_chunks > GN_MAX_PRODUCER_CHUNKS) {
        set_error("ldx_op_groupnorm_stats: bad argument (C % 8, C % G, G <= 32, 1 <= stats_chunks <= 32768)"); return LDX_EINVAL; }
    GroupNormArgs a{X, ldx_, Y, ldy, B, HW, C, G, eps, silu, gamma, beta, partial};
    a.stats_chunks = stats_chunks;
    launch_groupnorm(a, dtype_of(dtype), (hipStream_t)stream);
    return check_launch("ldx_op_groupnorm_stats");
}
int ldx_op_groupnorm(const void* X, int ldx_, void* Y, int ldy, int B, int HW, int C, int G, float eps, int silu,
                     const float* gamma, const float* beta, float* workspace, int dtype, void* stream) {
    if (!X || !Y || !gamma || !beta || !workspace || C % 8 || C % G || G > 32 || ldx_ % 8 || ldy % 8) { set_error("ldx_op_groupnorm: bad argument"); return LDX_EINVAL; }
    GroupNormArgs a{X, ldx_, Y, ldy, B, HW, C, G, eps, silu, gamma, beta, workspace};
    launch_groupnorm(a, dtype_of(dtype), (hipStream_t)stream);
    return check_launch("ldx_op_groupnorm");
}
int ldx_op_layernorm(const void* X, int ldx_, void* Y, int ldy, int rows, int C, float eps, const float* gamma, const float* beta, int dtype, void* stream) {
    if (!X || !Y || !gamma || !beta || C % 8 || C > 4096) { set_error("ldx_op_layernorm: bad argument (C % 8, C <= 4096)"); return LDX_EINVAL; }
    LayerNormArgs a{X, ldx_, Y, ldy, rows, C, eps, gamma, beta};
    launch_layernorm(a, dtype_of(dtype), (hipStream_t)stream);
    return check_launch("ldx_op_layernorm");
}
int ldx_op_attention(const void* Q, int ldq, const void* K, int ldk, const void* V, int ldv, void* O, int ldo, int B, int H, int Nq, int Mk, int D,
                     float scale, int causal, int dtype, void* stream) {
    if (!Q || !K || !V || !O || D % 8 || (D > 160 && D != 512) || D <= 0 || ldq % 8 || ldk % 8 || ldv % 8 || ldo % 4 || Mk <= 0) { set_error("ldx_op_attention: bad argument (D % 8, D <= 160 or D == 512)"); return LDX_EINVAL; }
    AttnArgs a = attn_args(Q, ldq, K, ldk, V, ldv, O, ldo, B, H, Nq, Mk, D, scale); a.causal = causal;
    if (D == 512 && attn_pick(a).family != AF_ATTN512) { set_error("ldx_op_attention: D = 512 without a mask only (attn512.hip)"); return LDX_EINVAL; }
    attn_attach_scratch(a, op_scratch);      // (shared single-op scratch: one stream per device, include/ldx.h)
    if (a.nsplit > 1 && !a.split_ws) { set_error("attention split workspace allocation failed"); return LDX_EHIP; }
    launch_attention(a, dtype_of(dtype), (hipStream_t)stream);
    return check_launch("ldx_op_attention");
}
int ldx_op_xattn_block(void* H, int ldh, int64_t M, int N, int C, int heads, const float* ln_gamma, const float* ln_beta, float eps,
                       const void* Wq, const void* Wo, const float* bo, const void* K, int ldk, const void* V, int ldv, int Mk,
                       float scale, int dtype, void* stream) {
    XAttnArgs a{};
    a.H = H; a.ldh = ldh; a.M = (long)M; a.N = N; a.C = C; a.heads = heads; a.ln_g = ln_gamma; a.ln_b = ln_beta; a.eps = eps;
    a.Wq = Wq; a.Wo = Wo; a.bo = bo; a.K = K; a.ldk = ldk; a.V = V; a.ldv = ldv; a.Mk = Mk; a.scale = scale;
    if (!H || !ln_gamma || !ln_beta || !Wq || !Wo || !K || !V || M <= 0 || N <= 0 || ldh < C || !xattn_block_ok(a)) {
        set_error("ldx_op_xattn_block: shape not taken by the fused kernel (C = 320, 8 heads, Mk <= 80, N % 128 == 0, M % N == 0)"); return LDX_EINVAL; }
    launch_xattn_block(a, dtype_of(dtype), (hipStream_t)stream);
    return check_launch("ldx_op_xattn_block");
}
int ldx_op_ff_block(void* H, int ldh, int64_t M, int C, int inner, const float* ln_gamma, const float* ln_beta, float eps,
                    const void* W1, const float* b1, const void* W2, const float* b2, int dtype, void* stream) {
    FFBlockArgs a{};
    a.H = H; a.ldh = ldh; a.M = (long)M; a.C = C; a.inner = inner; a.ln_g = ln_gamma; a.ln_b = ln_beta; a.eps = eps; a.W1 = W1; a.b1 = b1; a.W2 = W2; a.b2 = b2;
    if (!H || !ln_gamma || !ln_beta || !W1 || !b1 || !W2 || M <= 0 || ldh < C || !ff_block_ok(a)) {
        set_error("ldx_op_ff_block: shape not taken by the fused kernel (C = 320, inner = 1280)"); return LDX_EINVAL; }
    launch_ff_block(a, dtype_of(dtype), (hipStream_t)stream);
    return check_launch("ldx_op_ff_block");
}
int ldx_op_rowgemm(const void* X, int ldx_, void* Y, int ldy, int64_t M, int N, int K, const void* W, const float* bias, const void* R, int ldr,
                   int pro, const float* gamma, const float* beta, float eps, const float* partial, int nchunk, int HW, int dtype, void* stream) {
    RowGemmArgs a{};
    a.X = X; a.ldx = ldx_; a.Y = Y; a.ldy = ldy; a.M = (long)M; a.N = N; a.K = K; a.W = W; a.bias = bias; a.R = R; a.ldr = ldr;
    a.pro = pro; a.g = gamma; a.b = beta; a.eps = eps; a.partial = partial; a.nchunk = nchunk; a.HW = HW; a.G = 32;
    if (!X || !Y || !W || ldx_ < K || ldy < N || !rowgemm_ok(a)) { set_error("ldx_op_rowgemm: shape not taken (K = 320 or 640, N a multiple of K, pro 0..2, GroupNorm: HW % (40960 / K) == 0, nchunk <= 256)"); return LDX_EINVAL; }
    launch_rowgemm(a, dtype_of(dtype), (hipStream_t)stream);
    return check_launch("ldx_op_rowgemm");
}
int ldx_op_attention_bias(const void* Q, int ldq, const void* K, int ldk, const void* V, int ldv, void* O, int ldo, int B, int H, int Nq, int Mk, int D,
                          float scale, const float* bias, int bias_ld, int64_t bias_head_stride, int dtype, void* stream) {
    if (!Q || !K || !V || !O || !bias || D % 8 || D > 160 || D <= 0 || ldq % 8 || ldk % 8 || ldv % 8 || ldo % 4 || Mk <= 0 || bias_ld % 4 ||
        bias_ld < ((Mk + 63) / 64) * 64 || bias_head_stride % 4) {
        set_error("ldx_op_attention_bias: bad argument (bias_ld >= Mk rounded up to 64, multiples of 4)"); return LDX_EINVAL; }
    AttnArgs a = attn_args(Q, ldq, K, ldk, V, ldv, O, ldo, B, H, Nq, Mk, D, scale);
    a.bias = bias; a.bias_ld = bias_ld; a.bias_hs = (long)bias_head_stride;
    launch_attention(a, dtype_of(dtype), (hipStream_t)stream);
    return check_launch("ldx_op_attention_bias");
}
int ldx_op_skinny(const float* x, int ldx_, const void* W, const float* bias, float* out, int ldo, int M, int N, int K, int in_act, int out_act, int dtype, void* stream) {
    if (!x || !W || !out || K % 8) { set_error("ldx_op_skinny: bad argument"); return LDX_EINVAL; }
    SkinnyArgs a{x, ldx_, W, bias, out, ldo, M, N, K, in_act, out_act};
    launch_skinny(a, dtype_of(dtype), (hipStream_t)stream);
    return check_launch("ldx_op_skinny");
}

}  // extern "C"
