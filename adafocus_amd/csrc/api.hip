// C-ABI layer (include/adafocus.h): the handle, the global options, argument validation and launch planning of the
// stand-alone ops, and the GRU classifier / FC drivers (the ResNet trunk: resnet_trunk.hip).  No PyTorch types, no allocation in forward calls.
#include <cstdarg>
#include <cstdio>
#include <cstring>

#include "adaf_internal.h"

// ---- helpers shared with the other host files (declared in adaf_internal.h) -----------
int adaf_fail(adaf_handle* h, int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    if (h) h->err = buf;
    return code;
}

int adaf_hip_fail(adaf_handle* h, hipError_t e, const char* what) {
    return adaf_fail(h, ADAF_E_LAUNCH, "%s: %s", what, hipGetErrorString(e));
}

bool adaf_aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
int adaf_check_ws(adaf_handle* h, const char* who, const void* ws, size_t ws_bytes, size_t need, AdafWsOrder order) {
    const bool small = ws_bytes < need, skew = !adaf_aligned16(ws);
    if (small && (order == ADAF_WS_SIZE_FIRST || !skew)) return adaf_fail(h, ADAF_E_NOMEM, "%s: workspace %zu < %zu bytes", who, ws_bytes, need);
    return skew ? adaf_fail(h, ADAF_E_LAYOUT, "%s: the workspace must be 16-byte aligned", who) : ADAF_OK;
}
int adaf_conv_out(int in, int k, int stride, int pad) { return (in + 2 * pad - k) / stride + 1; }

// Validates a conv description and flattens it; returns ADAF_OK or an error code.
int adaf_make_conv_args(adaf_handle* h, const adaf_conv_params* p, const float* x, const float* w, const float* scale,
                        const float* bias, const float* res, float* out, ConvArgs* a) {
    if (!p || !x || !w || !out) return adaf_fail(h, ADAF_E_BADARG, "conv: null pointer");
    if (p->n <= 0 || p->h <= 0 || p->w <= 0 || p->cin <= 0 || p->cout <= 0 || p->kh <= 0 || p->kw <= 0 ||
        p->stride <= 0 || p->pad < 0)
        return adaf_fail(h, ADAF_E_BADARG, "conv: non-positive extent");
    if (p->cin % 4) return adaf_fail(h, ADAF_E_LAYOUT, "conv: cin=%d must be a multiple of 4 (pad the channel axis)", p->cin);
    const int ldx = p->ldx ? p->ldx : p->cin, ldo = p->ldo ? p->ldo : p->cout, ldr = p->ldr ? p->ldr : p->cout;
    if (ldx < p->cin || ldo < p->cout || ldr < p->cout) return adaf_fail(h, ADAF_E_BADARG, "conv: pixel stride smaller than channels");
    if (ldx % 4 || !adaf_aligned16(x) || !adaf_aligned16(w)) return adaf_fail(h, ADAF_E_LAYOUT, "conv: x/w must be 16-byte aligned, ldx % 4 == 0");
    if (p->act < ADAF_ACT_NONE || p->act > ADAF_ACT_SWISH) return adaf_fail(h, ADAF_E_BADARG, "conv: unknown activation %d", p->act);
    const int oh = adaf_conv_out(p->h, p->kh, p->stride, p->pad), ow = adaf_conv_out(p->w, p->kw, p->stride, p->pad);
    if (oh <= 0 || ow <= 0) return adaf_fail(h, ADAF_E_BADARG, "conv: empty output");
    const long long M = (long long)p->n * oh * ow;
    if (M > 0x7fffffffLL || (long long)p->n * p->h * p->w > 0x7fffffffLL) return adaf_fail(h, ADAF_E_BADARG, "conv: too many pixels");
    int fold = 0;
    if (p->tsm_segments > 0) {
        if (p->kh != 1 || p->kw != 1 || p->stride != 1 || p->pad != 0)
            return adaf_fail(h, ADAF_E_BADARG, "conv: fused temporal shift needs a 1x1 stride-1 conv");
        if (p->tsm_div <= 0 || p->n % p->tsm_segments) return adaf_fail(h, ADAF_E_BADARG, "conv: n %% tsm_segments != 0");
        fold = p->cin / p->tsm_div;
        if (fold % 4) return adaf_fail(h, ADAF_E_LAYOUT, "conv: temporal-shift fold=%d must be a multiple of 4", fold);
    }
    a->wsp = nullptr;
    a->in16 = a->out16 = a->res16 = 0;
    a->pm_allow = h->conv_pos_major; a->pm_images = a->pm_groups = 0;
    a->split_n = 0; a->out_b = nullptr; a->ldo_b = 0; a->act_b = 0;
    a->x = x; a->w = w; a->scale = scale; a->bias = bias; a->res = res; a->out = out;
    a->M = (int)M; a->N = p->cout; a->K = p->kh * p->kw * p->cin;
    a->cin = p->cin; a->H = p->h; a->W = p->w; a->OH = oh; a->OW = ow; a->KH = p->kh; a->KW = p->kw;
    a->stride = p->stride; a->pad = p->pad; a->ldx = ldx; a->ldo = ldo; a->ldr = ldr; a->act = p->act;
    a->tsm_T = p->tsm_segments > 0 ? p->tsm_segments : 0; a->tsm_fold = fold; a->tsm_hw = p->h * p->w;
    a->tiles_n = 0; a->nblocks = 0;
    a->zeros = h->zeros;
    a->vec_epi = (p->cout % 4 == 0 && ldo % 4 == 0 && ldr % 4 == 0 && adaf_aligned16(out) && (!res || adaf_aligned16(res)) &&
                  (!scale || adaf_aligned16(scale)) && (!bias || adaf_aligned16(bias))) ? 1 : 0;
    return ADAF_OK;
}

// The half-precision part of the validation: which of a flattened conv's operands are fp16 (a residual, if there is one, always is).
int adaf_set_conv_dtypes(adaf_handle* h, bool in16, bool out16, ConvArgs* a) {
    a->in16 = in16; a->out16 = out16; a->res16 = a->res != nullptr;
    if (in16 && (a->cin % 8 || a->ldx % 8)) return adaf_fail(h, ADAF_E_LAYOUT, "conv_f16: fp16 operands need cin %% 8 == 0 (16-byte chunks)");
    if (in16 && a->tsm_T > 0 && a->tsm_fold % 8)
        return adaf_fail(h, ADAF_E_LAYOUT, "conv_f16: temporal-shift fold=%d must be a multiple of 8 with fp16 operands (whole 16-byte chunks)", a->tsm_fold);
    if (!in16 && a->res) return adaf_fail(h, ADAF_E_BADARG, "conv_f16: a residual needs fp16 operands");
    return ADAF_OK;
}

AdafOptions& adaf_options() {
    static AdafOptions o;
    return o;
}

namespace {
struct OptKey { const char* name; double lo, hi; };
// (round 6: the switches that measured as no-gain and had no user are gone -- conv_lean, pm_fill, resize_lds_kb, mb_wave, dw3_variant, gru_barrier)
const OptKey kOptKeys[] = {{"conv_pool", 0, 1}, {"mb_strip", 0, 1}, {"mbv2_chunk", 1, 1 << 20}, {"latency_rows", 0, 1 << 30}, {"latency_linear_rows", 0, 1 << 30},
                           {"effnet_plan", 0, 511}, {"effnet_chunk", 1, 1 << 20}, {"gru_scan_slices", 1, 2}, {"effnet_fused_blocks", 0, 4294967295.0},
                           {"stem_rows", 0, 2}, {"split_stage1_f32", 0, 1}, {"gru_graph_persistent", 0, 1}, {"split_lean", 0, 1}, {"tsm_lean", 0, 1}, {"conv_tile_regime", 0, 2}};
int find_opt(const char* key) {
    if (!key) return -1;
    for (size_t i = 0; i < sizeof(kOptKeys) / sizeof(kOptKeys[0]); ++i)
        if (!strcmp(kOptKeys[i].name, key)) return (int)i;
    return -1;
}
}  // namespace

// ======================================================================================
extern "C" {

int adaf_version(void) { return ADAF_VERSION; }

int adaf_create(int device, adaf_handle** out) {
    if (!out) return ADAF_E_BADARG;
    *out = nullptr;
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || device < 0 || device >= count) return ADAF_E_ARCH;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) != hipSuccess) return ADAF_E_ARCH;
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) return ADAF_E_ARCH;  // the kernels are gfx950 code objects
    adaf_handle* h = new adaf_handle();
    h->device = device;
    h->cus = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    int cur = 0;
    (void)hipGetDevice(&cur);
    (void)hipSetDevice(device);
    hipError_t e = hipMalloc(reinterpret_cast<void**>(&h->zeros), 256);
    if (e == hipSuccess) e = hipMemset(h->zeros, 0, 256);
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&h->scan_timeouts), 256);
    if (e == hipSuccess) e = hipMemset(h->scan_timeouts, 0, 256);
    for (int i = 0; i < 4 && e == hipSuccess; ++i) e = hipEventCreateWithFlags(&h->scan_done[i], hipEventDisableTiming);
    if (e == hipSuccess) {
        // The occupancy API can report one block per CU too many for kernels in this SGPR range (the scan uses 90;
        // MI355X_MICROARCH.md "Correctness boundaries"), and a grid barrier must never count on a slot that is not there:
        // budget with one block per CU less than reported (the scan's 128 blocks then still fit twice over).
        const int per_cu = adaf_gru_scan_blocks_per_cu();
        h->scan_resident = (per_cu > 1 ? per_cu - 1 : per_cu) * h->cus;
        const int slots = h->scan_resident / 128;
        h->scan_slots = slots < 1 ? 1 : (slots > 4 ? 4 : slots);
        const int bptt_per_cu = adaf_gru_bptt_blocks_per_cu();
        h->bptt_resident = (bptt_per_cu > 1 ? bptt_per_cu - 1 : bptt_per_cu) * h->cus;
    }
    (void)hipSetDevice(cur);
    if (e != hipSuccess) { delete h; return ADAF_E_NOMEM; }
    *out = h;
    return ADAF_OK;
}

int adaf_destroy(adaf_handle* h) {
    if (h && h->zeros) (void)hipFree(h->zeros);
    if (h && h->scan_timeouts) (void)hipFree(h->scan_timeouts);
    if (h)
        for (int i = 0; i < 4; ++i)
            if (h->scan_done[i]) (void)hipEventDestroy(h->scan_done[i]);
    if (h)
        for (int i = 0; i < adaf_handle::kWatched; ++i)
            if (h->watch_done[i]) (void)hipEventDestroy(h->watch_done[i]);
    delete h;
    return ADAF_OK;
}

}  // extern "C"

namespace {
bool stream_capturing(hipStream_t st) {
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    (void)hipStreamIsCapturing(st, &cap);
    return cap != hipStreamCaptureStatusNone;
}
}  // namespace

bool adaf_launches_beside(adaf_handle* h, hipStream_t st) {
    if (!h || stream_capturing(st)) return false;
    std::lock_guard<std::mutex> lock(h->watch_mu);
    for (int i = 0; i < adaf_handle::kWatched; ++i)
        if (h->watch_done[i] && h->watch_used[i] && h->watch_key[i] != st && hipEventQuery(h->watch_done[i]) == hipErrorNotReady) return true;
    return false;
}

void adaf_note_forward(adaf_handle* h, hipStream_t st) {
    if (!h || stream_capturing(st)) return;
    std::lock_guard<std::mutex> lock(h->watch_mu);
    int slot = 0;
    for (int i = 0; i < adaf_handle::kWatched; ++i) {
        if (h->watch_used[i] && h->watch_key[i] == st) { slot = i; break; }
        if (h->watch_used[i] < h->watch_used[slot]) slot = i;      // a free slot (0) or the least recently used one
    }
    if (!h->watch_done[slot] && hipEventCreateWithFlags(&h->watch_done[slot], hipEventDisableTiming) != hipSuccess) { h->watch_done[slot] = nullptr; return; }
    h->watch_key[slot] = st;
    h->watch_used[slot] = ++h->watch_tick;
    (void)hipEventRecord(h->watch_done[slot], st);
}

extern "C" {

const char* adaf_last_error(const adaf_handle* h) { return h ? h->err.c_str() : "null handle"; }
int adaf_device_cus(const adaf_handle* h) { return h ? h->cus : 0; }
int adaf_set_conv_pos_major(adaf_handle* h, int on) {
    if (!h) return ADAF_E_BADARG;
    h->conv_pos_major = on < 0 || on > 2 ? 1 : on;    // 2: position-major rows WITHOUT tap skipping (experiments)
    return ADAF_OK;
}
int adaf_set_global_option(const char* key, double value) {
    const int k = find_opt(key);
    if (k < 0 || !(value >= kOptKeys[k].lo && value <= kOptKeys[k].hi)) return ADAF_E_BADARG;
    AdafOptions& o = adaf_options();
    switch (k) {
        case 0: o.conv_pool = (int)value; break;
        case 1: o.mb_strip = (int)value; break;
        case 2: o.mbv2_chunk = (int)value; break;
        case 3: o.latency_rows = (int)value; break;
        case 4: o.latency_linear_rows = (int)value; break;
        case 5: o.effnet_plan = (unsigned)value; break;
        case 6: o.effnet_chunk = (int)value; break;
        case 7: o.gru_scan_slices = (int)value; break;
        case 8: o.effnet_fused_blocks = (unsigned)value; break;
        case 9: o.stem_rows = (int)value; break;
        case 10: o.split_stage1_f32 = (int)value; break;
        case 11: o.gru_graph_persistent = (int)value; break;
        case 12: o.split_lean = (int)value; break;
        case 13: o.tsm_lean = (int)value; break;
        default: o.conv_tile_regime = (int)value; break;
    }
    return ADAF_OK;
}

double adaf_get_global_option(const char* key) {
    const AdafOptions& o = adaf_options();
    switch (find_opt(key)) {
        case 0: return o.conv_pool;
        case 1: return o.mb_strip;
        case 2: return o.mbv2_chunk;
        case 3: return o.latency_rows;
        case 4: return o.latency_linear_rows;
        case 5: return o.effnet_plan;
        case 6: return o.effnet_chunk;
        case 7: return o.gru_scan_slices;
        case 8: return o.effnet_fused_blocks;
        case 9: return o.stem_rows;
        case 10: return o.split_stage1_f32;
        case 11: return o.gru_graph_persistent;
        case 12: return o.split_lean;
        case 13: return o.tsm_lean;
        case 14: return o.conv_tile_regime;
        default: return __builtin_nan("");
    }
}

int adaf_set_gru_persistent(adaf_handle* h, int on) {
    if (!h) return ADAF_E_BADARG;
    if (on < 0 || on > 2) return adaf_fail(h, ADAF_E_BADARG, "set_gru_persistent: mode %d (0 off, 1 on, 2 on + cooperative launch)", on);
    h->gru_persistent = on;
    return ADAF_OK;
}

int adaf_gru_scan_timeouts(adaf_handle* h, unsigned* count_out) {
    if (!h || !count_out) return ADAF_E_BADARG;
    int cur = 0;
    (void)hipGetDevice(&cur);
    (void)hipSetDevice(h->device);
    hipError_t e = hipDeviceSynchronize();
    if (e == hipSuccess) e = hipMemcpy(count_out, h->scan_timeouts, sizeof(unsigned), hipMemcpyDeviceToHost);
    (void)hipSetDevice(cur);
    return e == hipSuccess ? ADAF_OK : adaf_hip_fail(h, e, "gru_scan_timeouts");
}

// ---- crop ------------------------------------------------------------------------------
int adaf_crop_gather_f32(adaf_handle* h, const float* frames, int n_frames, int channels, int height, int width,
                         const float* action_yx, int n_actions, int frames_per_action, int patch, float* out,
                         int out_layout, int32_t* coords_out, void* stream) {
    if (!h) return ADAF_E_BADARG;
    if (n_frames == 0) return ADAF_OK;  // empty batch: nothing to gather
    if (!frames || !action_yx || !out) return adaf_fail(h, ADAF_E_BADARG, "crop: null pointer");
    if (n_frames < 0 || channels <= 0 || height <= 0 || width <= 0 || patch <= 0 || frames_per_action <= 0)
        return adaf_fail(h, ADAF_E_BADARG, "crop: non-positive extent");
    if (patch > height) return adaf_fail(h, ADAF_E_BADARG, "crop: patch %d larger than frame height %d", patch, height);
    if (width < height) return adaf_fail(h, ADAF_E_BADARG, "crop: width < height (the reference scales both axes by H-P)");
    if ((long long)n_actions * frames_per_action != n_frames)
        return adaf_fail(h, ADAF_E_BADARG, "crop: n_actions*frames_per_action=%lld != n_frames=%d",
                    (long long)n_actions * frames_per_action, n_frames);
    if (out_layout == ADAF_LAYOUT_NHWC4 && channels != 3) return adaf_fail(h, ADAF_E_LAYOUT, "crop: NHWC4 needs 3 channels");
    if (out_layout == ADAF_LAYOUT_NHWC && channels > 16) return adaf_fail(h, ADAF_E_LAYOUT, "crop: NHWC output supports <= 16 channels");
    if (out_layout < ADAF_LAYOUT_NCHW || out_layout > ADAF_LAYOUT_NHWC4) return adaf_fail(h, ADAF_E_LAYOUT, "crop: unknown layout");
    const int co = out_layout == ADAF_LAYOUT_NCHW ? 1 : (out_layout == ADAF_LAYOUT_NHWC4 ? 4 : channels);
    if ((size_t)8 * patch * co * sizeof(float) > 160 * 1024) return adaf_fail(h, ADAF_E_BADARG, "crop: patch too wide for the LDS tile");
    hipError_t e = adaf_launch_crop(frames, n_frames, channels, height, width, action_yx, frames_per_action, patch, out,
                                    out_layout, coords_out, (hipStream_t)stream);
    return e == hipSuccess ? ADAF_OK : adaf_hip_fail(h, e, "crop launch");
}

int adaf_crop_gather_nhwc4_f32(adaf_handle* h, const float* frames_nhwc4, int n_frames, int height, int width,
                               const float* action_yx, int n_actions, int frames_per_action, int patch, float* out_nhwc4,
                               int32_t* coords_out, void* stream) {
    if (!h) return ADAF_E_BADARG;
    if (n_frames == 0) return ADAF_OK;
    if (!frames_nhwc4 || !action_yx || !out_nhwc4) return adaf_fail(h, ADAF_E_BADARG, "crop_nhwc4: null pointer");
    if (n_frames < 0 || height <= 0 || width <= 0 || patch <= 0 || frames_per_action <= 0)
        return adaf_fail(h, ADAF_E_BADARG, "crop_nhwc4: non-positive extent");
    if (patch > height || width < height) return adaf_fail(h, ADAF_E_BADARG, "crop_nhwc4: patch > height or width < height");
    if ((long long)n_actions * frames_per_action != n_frames) return adaf_fail(h, ADAF_E_BADARG, "crop_nhwc4: n_actions*frames_per_action != n_frames");
    if (!adaf_aligned16(frames_nhwc4) || !adaf_aligned16(out_nhwc4)) return adaf_fail(h, ADAF_E_LAYOUT, "crop_nhwc4: 16-byte alignment required");
    adaf_launch_crop_nhwc4(frames_nhwc4, n_frames, height, width, action_yx, frames_per_action, patch, out_nhwc4, coords_out,
                           (hipStream_t)stream);
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? ADAF_OK : adaf_hip_fail(h, e, "crop_nhwc4 launch");
}

int adaf_crop_resize_f32(adaf_handle* h, const float* frames, int in_layout, int n_frames, int channels, int height, int width,
                         const float* action_yx, int n_actions, int frames_per_action, const int32_t* size_px,
                         int size_default, int patch, float* out, int out_layout, int32_t* coords_out, void* stream) {
    if (!h) return ADAF_E_BADARG;
    if (n_frames == 0) return ADAF_OK;
    if (!frames || !action_yx || !out) return adaf_fail(h, ADAF_E_BADARG, "crop_resize: null pointer");
    if (n_frames < 0 || channels <= 0 || height <= 0 || width <= 0 || patch <= 0 || frames_per_action <= 0)
        return adaf_fail(h, ADAF_E_BADARG, "crop_resize: non-positive extent");
    if (width < height) return adaf_fail(h, ADAF_E_BADARG, "crop_resize: width < height (the reference scales both axes by H-S)");
    if ((long long)n_actions * frames_per_action != n_frames)
        return adaf_fail(h, ADAF_E_BADARG, "crop_resize: n_actions*frames_per_action != n_frames");
    if (!size_px && (size_default < 1 || size_default > height))
        return adaf_fail(h, ADAF_E_BADARG, "crop_resize: window size %d outside [1, height=%d]", size_default, height);
    if (in_layout != ADAF_LAYOUT_NCHW && in_layout != ADAF_LAYOUT_NHWC4) return adaf_fail(h, ADAF_E_LAYOUT, "crop_resize: frames must be NCHW or NHWC4");
    if (out_layout < ADAF_LAYOUT_NCHW || out_layout > ADAF_LAYOUT_NHWC4) return adaf_fail(h, ADAF_E_LAYOUT, "crop_resize: unknown output layout");
    if ((in_layout == ADAF_LAYOUT_NHWC4 || out_layout == ADAF_LAYOUT_NHWC4) && channels != 3) return adaf_fail(h, ADAF_E_LAYOUT, "crop_resize: NHWC4 needs 3 channels");
    if (out_layout == ADAF_LAYOUT_NHWC && channels > 16) return adaf_fail(h, ADAF_E_LAYOUT, "crop_resize: NHWC output supports <= 16 channels");
    if ((in_layout == ADAF_LAYOUT_NHWC4 && !adaf_aligned16(frames)) || (out_layout == ADAF_LAYOUT_NHWC4 && !adaf_aligned16(out)))
        return adaf_fail(h, ADAF_E_LAYOUT, "crop_resize: 16-byte alignment required for pixel-major buffers");
    hipStream_t st = (hipStream_t)stream;
    if (!size_px && size_default == patch) {
        // scale 1: the resample IS the slice copy -- run the gather itself (bit-exact by construction)
        if (in_layout == ADAF_LAYOUT_NCHW)
            return adaf_crop_gather_f32(h, frames, n_frames, channels, height, width, action_yx, n_actions, frames_per_action, patch, out,
                                        out_layout, coords_out, stream);
        if (out_layout == ADAF_LAYOUT_NHWC4)
            return adaf_crop_gather_nhwc4_f32(h, frames, n_frames, height, width, action_yx, n_actions, frames_per_action, patch, out,
                                              coords_out, stream);
    }
    hipError_t e = adaf_launch_crop_resize(frames, in_layout == ADAF_LAYOUT_NHWC4, n_frames, channels, height, width, action_yx, size_px,
                                           size_default, frames_per_action, patch, out, out_layout, coords_out, st);
    return e == hipSuccess ? ADAF_OK : adaf_hip_fail(h, e, "crop_resize launch");
}

int adaf_resize_nearest_f32(adaf_handle* h, const float* frames, int in_layout, int n_frames, int channels, int height, int width,
                            int out_h, int out_w, float* out, int out_layout, void* stream) {
    if (!h) return ADAF_E_BADARG;
    if (n_frames == 0) return ADAF_OK;
    if (!frames || !out) return adaf_fail(h, ADAF_E_BADARG, "resize_nearest: null pointer");
    if (n_frames < 0 || channels <= 0 || height <= 0 || width <= 0 || out_h <= 0 || out_w <= 0)
        return adaf_fail(h, ADAF_E_BADARG, "resize_nearest: non-positive extent");
    if (in_layout != ADAF_LAYOUT_NCHW && in_layout != ADAF_LAYOUT_NHWC4) return adaf_fail(h, ADAF_E_LAYOUT, "resize_nearest: frames must be NCHW or NHWC4");
    if (out_layout < ADAF_LAYOUT_NCHW || out_layout > ADAF_LAYOUT_NHWC4) return adaf_fail(h, ADAF_E_LAYOUT, "resize_nearest: unknown output layout");
    if ((in_layout == ADAF_LAYOUT_NHWC4 || out_layout == ADAF_LAYOUT_NHWC4) && channels != 3) return adaf_fail(h, ADAF_E_LAYOUT, "resize_nearest: NHWC4 needs 3 channels");
    if ((in_layout == ADAF_LAYOUT_NHWC4 && !adaf_aligned16(frames)) || (out_layout == ADAF_LAYOUT_NHWC4 && !adaf_aligned16(out)))
        return adaf_fail(h, ADAF_E_LAYOUT, "resize_nearest: 16-byte alignment required for pixel-major buffers");
    hipError_t e = adaf_launch_resize_nearest(frames, in_layout == ADAF_LAYOUT_NHWC4, n_frames, channels, height, width, out_h, out_w, out,
                                              out_layout, (hipStream_t)stream);
    return e == hipSuccess ? ADAF_OK : adaf_hip_fail(h, e, "resize_nearest launch");
}

int adaf_ingest_u8_f32(adaf_handle* h, const uint8_t* clips_hwc, int n_clips, int frames, int height, int width,
                       const float* mean3, const float* std3, float* out_nhwc4, void* stream) {
    if (!h) return ADAF_E_BADARG;
    if (n_clips == 0) return ADAF_OK;
    if (!clips_hwc || !mean3 || !std3 || !out_nhwc4) return adaf_fail(h, ADAF_E_BADARG, "ingest: null pointer");
    if (n_clips < 0 || frames <= 0 || frames > 64 || height <= 0 || width <= 0) return adaf_fail(h, ADAF_E_BADARG, "ingest: non-positive extent (frames <= 64)");
    if (!adaf_aligned16(out_nhwc4)) return adaf_fail(h, ADAF_E_LAYOUT, "ingest: output must be 16-byte aligned");
    for (int c = 0; c < 3; ++c)
        if (!(std3[c] > 0.f)) return adaf_fail(h, ADAF_E_BADARG, "ingest: std must be positive");
    adaf_launch_ingest_u8(clips_hwc, n_clips, frames, height, width, mean3, std3, out_nhwc4, (hipStream_t)stream);
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? ADAF_OK : adaf_hip_fail(h, e, "ingest launch");
}

// ---- conv ------------------------------------------------------------------------------
int adaf_conv2d_bn_act_f32(adaf_handle* h, const adaf_conv_params* p, const float* x, const float* w_ohwi,
                           const float* scale, const float* bias, const float* residual, float* out, void* stream) {
    if (!h) return ADAF_E_BADARG;
    ConvArgs a;
    int rc = adaf_make_conv_args(h, p, x, w_ohwi, scale, bias, residual, out, &a);
    if (rc) return rc;
    if (p->tile < 0 || (p->tile > 80 && p->tile != 95) || (p->tile && !adaf_conv_tile_exists(p->tile)))
        return adaf_fail(h, ADAF_E_BADARG, "conv: no kernel variant with tile id %d", p->tile);
    if (adaf_launch_conv_gemm(a, p->tile, h->cus, (hipStream_t)stream) < 0) return adaf_fail(h, ADAF_E_LAUNCH, "conv: no tile");
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? ADAF_OK : adaf_hip_fail(h, e, "conv launch");
}

int adaf_conv2d_naive_f32(adaf_handle* h, const adaf_conv_params* p, const float* x, const float* w_ohwi,
                          const float* scale, const float* bias, const float* residual, float* out, void* stream) {
    if (!h) return ADAF_E_BADARG;
    ConvArgs a;
    int rc = adaf_make_conv_args(h, p, x, w_ohwi, scale, bias, residual, out, &a);
    if (rc) return rc;
    adaf_launch_conv_naive(a, (hipStream_t)stream);
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? ADAF_OK : adaf_hip_fail(h, e, "naive conv launch");
}

// ---- half-precision storage (N2) -----------------------------------------------------------------------------
int adaf_conv2d_bn_act_f16(adaf_handle* h, const adaf_conv_params* p, const void* x, int x_dtype, const void* w_ohwi,
                           const float* scale, const float* bias, const void* residual_f16, void* out, int out_dtype,
                           void* stream) {
    if (!h) return ADAF_E_BADARG;
    if ((x_dtype != ADAF_DTYPE_F32 && x_dtype != ADAF_DTYPE_F16) || (out_dtype != ADAF_DTYPE_F32 && out_dtype != ADAF_DTYPE_F16))
        return adaf_fail(h, ADAF_E_BADARG, "conv_f16: unknown dtype");
    if (x_dtype == ADAF_DTYPE_F32 && out_dtype == ADAF_DTYPE_F32) return adaf_fail(h, ADAF_E_BADARG, "conv_f16: nothing is fp16; use adaf_conv2d_bn_act_f32");
    ConvArgs a;
    int rc = adaf_make_conv_args(h, p, static_cast<const float*>(x), static_cast<const float*>(w_ohwi), scale, bias,
                            static_cast<const float*>(residual_f16), static_cast<float*>(out), &a);
    if (rc) return rc;
    if ((rc = adaf_set_conv_dtypes(h, x_dtype == ADAF_DTYPE_F16, out_dtype == ADAF_DTYPE_F16, &a))) return rc;
    if (p->tile && (p->tile < 81 || p->tile > 88)) return adaf_fail(h, ADAF_E_BADARG, "conv_f16: tile ids are 81..84, 88");
    if (adaf_launch_conv_gemm(a, p->tile, h->cus, (hipStream_t)stream) < 0)
        return adaf_fail(h, ADAF_E_LAYOUT, "conv_f16: shape not eligible (1x1: cin %% 8 == 0; k x k: cin %% 64 == 0)");
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? ADAF_OK : adaf_hip_fail(h, e, "conv_f16 launch");
}

int adaf_pack_conv_weight_f16(adaf_handle* h, const float* w_oihw, int cout, int cin, int kh, int kw, int cin_pad,
                              void* w_ohwi_f16, void* stream) {
    if (!h) return ADAF_E_BADARG;
    if (!w_oihw || !w_ohwi_f16 || cout <= 0 || cin <= 0 || kh <= 0 || kw <= 0 || cin_pad < cin || cin_pad % 8)
        return adaf_fail(h, ADAF_E_BADARG, "pack_f16: bad arguments (cin_pad %% 8 == 0)");
    adaf_launch_pack_weight_f16(w_oihw, cout, cin, kh, kw, cin_pad, w_ohwi_f16, (hipStream_t)stream);
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? ADAF_OK : adaf_hip_fail(h, e, "pack_f16 launch");
}

int adaf_cast_f32_f16(adaf_handle* h, const void* src, size_t count, void* dst, int to_f16, void* stream) {
    if (!h) return ADAF_E_BADARG;
    if (count == 0) return ADAF_OK;
    if (!src || !dst) return adaf_fail(h, ADAF_E_BADARG, "cast: null pointer");
    adaf_launch_cast(src, (long long)count, dst, to_f16 ? 1 : 0, (hipStream_t)stream);
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? ADAF_OK : adaf_hip_fail(h, e, "cast launch");
}

int adaf_dwconv3x3_bn_act_f16(adaf_handle* h, const void* x_f16, int n, int hh, int ww, int c, int stride, const float* w_33c,
                              const float* scale, const float* bias, int act, void* out_f16, void* stream) {
    if (!h) return ADAF_E_BADARG;
    if (!x_f16 || !w_33c || !scale || !bias || !out_f16 || n <= 0 || hh <= 0 || ww <= 0 || c <= 0) return adaf_fail(h, ADAF_E_BADARG, "dwconv_f16: bad arguments");
    if (stride != 1 && stride != 2) return adaf_fail(h, ADAF_E_BADARG, "dwconv_f16: stride must be 1 or 2");
    if (act < ADAF_ACT_NONE || act > ADAF_ACT_RELU6) return adaf_fail(h, ADAF_E_BADARG, "dwconv_f16: activation");
    if (c % 4 || (reinterpret_cast<uintptr_t>(x_f16) & 7) || (reinterpret_cast<uintptr_t>(out_f16) & 7) || !adaf_aligned16(w_33c) || !adaf_aligned16(scale) || !adaf_aligned16(bias))
        return adaf_fail(h, ADAF_E_LAYOUT, "dwconv_f16: c %% 4 == 0 and 8 / 16-byte alignment required");
    adaf_launch_dwconv3x3_f16(x_f16, n, hh, ww, c, stride, w_33c, scale, bias, act, out_f16, (hipStream_t)stream);
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? ADAF_OK : adaf_hip_fail(h, e, "dwconv_f16 launch");
}

int adaf_pack_conv_weight_f32(adaf_handle* h, const float* w_oihw, int cout, int cin, int kh, int kw, int cin_pad,
                              float* w_ohwi, void* stream) {
    if (!h) return ADAF_E_BADARG;
    if (!w_oihw || !w_ohwi || cout <= 0 || cin <= 0 || kh <= 0 || kw <= 0 || cin_pad < cin || cin_pad % 4)
        return adaf_fail(h, ADAF_E_BADARG, "pack: bad arguments");
    adaf_launch_pack_weight(w_oihw, cout, cin, kh, kw, cin_pad, w_ohwi, (hipStream_t)stream);
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? ADAF_OK : adaf_hip_fail(h, e, "pack launch");
}

int adaf_fold_bn_f32(adaf_handle* h, const float* gamma, const float* beta, const float* mean, const float* var,
                     float eps, int channels, float* scale, float* bias, void* stream) {
    if (!h) return ADAF_E_BADARG;
    if (!gamma || !beta || !mean || !var || !scale || !bias || channels <= 0) return adaf_fail(h, ADAF_E_BADARG, "fold_bn: bad arguments");
    adaf_launch_fold_bn(gamma, beta, mean, var, eps, channels, scale, bias, (hipStream_t)stream);
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? ADAF_OK : adaf_hip_fail(h, e, "fold_bn launch");
}

// ---- pooling / shift / glue ------------------------------------------------------------
int adaf_maxpool3x3s2_f32(adaf_handle* h, const float* x, int n, int hh, int ww, int c, float* out, void* stream) {
    if (!h) return ADAF_E_BADARG;
    if (!x || !out || n <= 0 || hh <= 0 || ww <= 0 || c <= 0) return adaf_fail(h, ADAF_E_BADARG, "maxpool: bad arguments");
    if (c % 4 || !adaf_aligned16(x) || !adaf_aligned16(out)) return adaf_fail(h, ADAF_E_LAYOUT, "maxpool: c %% 4 and 16-byte alignment required");
    adaf_launch_maxpool(x, n, hh, ww, c, out, (hipStream_t)stream);
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? ADAF_OK : adaf_hip_fail(h, e, "maxpool launch");
}

int adaf_global_avgpool_f32(adaf_handle* h, const float* x, int n, int hw, int c, float* out, int ldo, void* stream) {
    if (!h) return ADAF_E_BADARG;
    if (!x || !out || n <= 0 || hw <= 0 || c <= 0) return adaf_fail(h, ADAF_E_BADARG, "avgpool: bad arguments");
    if (ldo == 0) ldo = c;
    if (c % 4 || ldo % 4 || ldo < c || !adaf_aligned16(x) || !adaf_aligned16(out)) return adaf_fail(h, ADAF_E_LAYOUT, "avgpool: c,ldo %% 4 and 16-byte alignment required");
    adaf_launch_avgpool(x, n, hw, c, out, ldo, (hipStream_t)stream);
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? ADAF_OK : adaf_hip_fail(h, e, "avgpool launch");
}

int adaf_temporal_shift_f32(adaf_handle* h, const float* x, int nt, int c, int hw, int n_segment, int fold_div,
                            int layout, float* out, void* stream) {
    if (!h) return ADAF_E_BADARG;
    if (nt == 0) return ADAF_OK;
    if (!x || !out || nt < 0 || c <= 0 || hw <= 0 || n_segment <= 0 || fold_div <= 0) return adaf_fail(h, ADAF_E_BADARG, "tshift: bad arguments");
    if (nt % n_segment) return adaf_fail(h, ADAF_E_BADARG, "tshift: nt=%d not a multiple of n_segment=%d", nt, n_segment);
    if (layout != ADAF_LAYOUT_NCHW && layout != ADAF_LAYOUT_NHWC) return adaf_fail(h, ADAF_E_LAYOUT, "tshift: layout");
    if (x == out) return adaf_fail(h, ADAF_E_BADARG, "tshift: in-place shift is not supported (as in the reference, temporal_shift.py:36-38)");
    adaf_launch_tshift(x, nt, c, hw, n_segment, fold_div, layout, out, (hipStream_t)stream);
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? ADAF_OK : adaf_hip_fail(h, e, "tshift launch");
}

int adaf_copy2d_f32(adaf_handle* h, const float* src, int lds, float* dst, int ldd, int rows, int cols, void* stream) {
    if (!h) return ADAF_E_BADARG;
    if (rows == 0 || cols == 0) return ADAF_OK;
    if (!src || !dst || rows < 0 || cols < 0 || lds < cols || ldd < cols) return adaf_fail(h, ADAF_E_BADARG, "copy2d: bad arguments");
    adaf_launch_copy2d(src, lds, dst, ldd, rows, cols, (hipStream_t)stream);
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? ADAF_OK : adaf_hip_fail(h, e, "copy2d launch");
}

// ======================================================================================
// GRU classifier / linear + temporal mean
// ======================================================================================
struct GruClsWs { float *gi, *gh, *hs; };      // gi [B*T, 3H], gh [B, 3H], hidden states [B, T, H] (adaf_gru_seq_forward_f32 has its own)
static size_t gru_cls_layout(void* ws, int batch, int steps, int hidden, GruClsWs* r) {
    AdafCarver c(ws);
    r->gi = c.take<float>((size_t)batch * steps * 3 * hidden);
    r->gh = c.take<float>((size_t)batch * 3 * hidden);
    r->hs = c.take<float>((size_t)batch * steps * hidden);
    return c.off;
}
size_t adaf_gru_cls_workspace_bytes(int batch, int steps, int hidden) {
    GruClsWs r;
    return (batch <= 0 || steps <= 0 || hidden <= 0) ? 0 : gru_cls_layout(nullptr, batch, steps, hidden, &r);
}

static int linear_launch(adaf_handle* h, const float* x, int rows, int ldx, int in, int out_dim, const float* w,
                         const float* bias, float* out, int ldo, hipStream_t st) {
    adaf_conv_params p;
    memset(&p, 0, sizeof(p));
    p.n = rows; p.h = 1; p.w = 1; p.cin = in; p.cout = out_dim; p.kh = p.kw = 1; p.stride = 1; p.pad = 0;
    p.act = ADAF_ACT_NONE; p.ldx = ldx; p.ldo = ldo;
    ConvArgs a;
    int rc = adaf_make_conv_args(h, &p, x, w, nullptr, bias, nullptr, out, &a);
    if (rc) return rc;
    // a few rows (config 1's GRU projection: 16 x 3328 -> 3072) are one accumulator chain per block on the engine: the
    // small-batch form's chain is 3.2x shorter and bit-identical (conv_lat.hip; ADAF_LATENCY_LINEAR_ROWS, 0 = never)
    const int lat_rows = adaf_options().latency_linear_rows;
    if (rows <= lat_rows && in >= 512 && adaf_launch_conv_gemm(a, 95, h->cus, st) > 0) return ADAF_OK;
    if (adaf_launch_conv_gemm(a, 0, h->cus, st) < 0) return adaf_fail(h, ADAF_E_LAUNCH, "linear: no kernel for this shape");
    return ADAF_OK;
}

// h_t for every step: hs[b, t, :] (row stride between steps of one clip = hidden, between clips = T*hidden); with fc_w the
// per-step classifier rides along (logits_all [B*T, C], last [B, C]).
static int gru_scan(adaf_handle* h, const float* x, int ldx, int batch, int steps, int feat, int hidden,
                    const float* w_ih, const float* w_hh, const float* b_ih, const float* b_hh, const float* h0, float* gi,
                    float* gh, float* hs, const float* fc_w, const float* fc_b, int classes, float* logits_all, float* last,
                    hipStream_t st) {
    int rc;
    // all input projections at once: gi[b*T+t, :] = W_ih x[b,t] + b_ih
    if ((rc = linear_launch(h, x, batch * steps, ldx, feat, 3 * hidden, w_ih, b_ih, gi, 0, st))) return rc;
    // While `st` is being captured into a HIP graph (GFV.capture_hot_path, the small-batch latency mode) the slot events below cannot be part
    // of the capture (an event recorded outside a capture cannot be waited on inside one), so a captured persistent scan would sit OUTSIDE the
    // throttle that keeps the grid barrier's blocks co-resident: two graphs replayed side by side, or a graph beside eager hot paths, could
    // starve each other into the barrier's time-out (NaN-poisoned logits).  A capture therefore takes the launch-per-step form, which has no
    // grid barrier, unless the option "gru_graph_persistent" says the caller guarantees exclusive use (HotPathGraph then checks the time-out
    // counter every few replays).
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    (void)hipStreamIsCapturing(st, &cap);
    const bool capturing = cap != hipStreamCaptureStatusNone;
    if (h->gru_persistent && steps + 1 <= batch * 3 * hidden && (!capturing || adaf_options().gru_graph_persistent) &&
        adaf_gru_scan_persistent_ok(batch, hidden, fc_w ? classes : 0, h->scan_resident)) {
        // the whole recurrence (+ classifier) in one kernel; `gh` only lends its first steps+1 words to the grid barrier
        // a scan cut into two slices (batch > 32) takes two sets of blocks, i.e. two of the slots the resident-block budget is made of
        const AdafGruScanPlan plan = adaf_gru_scan_plan(batch, steps, (size_t)batch * 3 * hidden, h->scan_resident);
        const int need = plan.groups > h->scan_slots ? h->scan_slots : plan.groups;
        int slots[2] = {h->scan_next, (h->scan_next + 1) % h->scan_slots};
        if (!capturing) {
            h->scan_next = (h->scan_next + need) % h->scan_slots;
            for (int i = 0; i < need; ++i)
                if (h->scan_used[slots[i]]) (void)hipStreamWaitEvent(st, h->scan_done[slots[i]], 0);   // the scans that held these slots have finished
        }
        hipError_t e = adaf_launch_gru_scan_persistent(gi, w_hh, b_hh, h0, hs, reinterpret_cast<unsigned*>(gh), plan, batch, steps, fc_w, fc_b,
                                                       logits_all, last, classes, h->gru_persistent == 2, h->scan_timeouts, st);
        if (e != hipSuccess) return adaf_hip_fail(h, e, "gru scan launch");
        if (!capturing) {
            for (int i = 0; i < need; ++i) {
                (void)hipEventRecord(h->scan_done[slots[i]], st);
                h->scan_used[slots[i]] = true;
            }
        }
        return ADAF_OK;
    }
    for (int t = 0; t < steps; ++t) {
        const float* hprev = t ? hs + (size_t)(t - 1) * hidden : h0;
        const int ldprev = t ? steps * hidden : hidden;
        if (hprev) {  // gh = W_hh h_{t-1}; rows are strided views into hs
            if ((rc = linear_launch(h, hprev, batch, ldprev, hidden, 3 * hidden, w_hh, nullptr, gh, 0, st))) return rc;
        }
        adaf_launch_gru_gates(gi + (size_t)t * 3 * hidden, steps * 3 * hidden, hprev ? gh : nullptr, b_hh, hprev, ldprev,
                              hs + (size_t)t * hidden, steps * hidden, batch, hidden, st);
    }
    if (fc_w) {   // logits for every step, then the last step's rows
        if ((rc = linear_launch(h, hs, batch * steps, hidden, hidden, classes, fc_w, fc_b, logits_all, 0, st))) return rc;
        if (last) adaf_launch_copy2d(logits_all + (size_t)(steps - 1) * classes, steps * classes, last, classes, batch, classes, st);
    }
    return ADAF_OK;
}

int adaf_gru_seq_forward_f32(adaf_handle* h, const float* x, int ldx, int batch, int steps, int feat, int hidden,
                             const float* w_ih, const float* w_hh, const float* b_ih, const float* b_hh, const float* h0,
                             float* hs, void* ws, size_t ws_bytes, void* stream) {
    if (!h) return ADAF_E_BADARG;
    if (batch == 0) return ADAF_OK;
    if (!x || !w_ih || !w_hh || !b_ih || !b_hh || !hs || !ws) return adaf_fail(h, ADAF_E_BADARG, "gru_seq: null pointer");
    if (batch < 0 || steps <= 0 || feat <= 0 || hidden <= 0) return adaf_fail(h, ADAF_E_BADARG, "gru_seq: non-positive extent");
    if (ldx == 0) ldx = feat;
    if (feat % 4 || hidden % 4 || ldx % 4) return adaf_fail(h, ADAF_E_LAYOUT, "gru_seq: feat, hidden, ldx must be multiples of 4");
    if (h0 && !adaf_aligned16(h0)) return adaf_fail(h, ADAF_E_LAYOUT, "gru_seq: h0 must be 16-byte aligned");
    GruClsWs r;
    int rc = adaf_check_ws(h, "gru_seq", ws, ws_bytes, gru_cls_layout(ws, batch, steps, hidden, &r), ADAF_WS_SIZE_FIRST);
    if (rc) return rc;
    rc = gru_scan(h, x, ldx, batch, steps, feat, hidden, w_ih, w_hh, b_ih, b_hh, h0, r.gi, r.gh, hs, nullptr, nullptr, 0, nullptr,
                  nullptr, (hipStream_t)stream);
    if (rc) return rc;
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? ADAF_OK : adaf_hip_fail(h, e, "gru_seq forward");
}

int adaf_gru_cls_forward_f32(adaf_handle* h, const float* x, int ldx, int batch, int steps, int feat, int hidden,
                             int classes, const float* w_ih, const float* w_hh, const float* b_ih, const float* b_hh,
                             const float* fc_w, const float* fc_b, float* logits_all, float* last, void* ws,
                             size_t ws_bytes, void* stream) {
    if (!h) return ADAF_E_BADARG;
    if (batch == 0) return ADAF_OK;
    if (!x || !w_ih || !w_hh || !b_ih || !b_hh || !fc_w || !fc_b || !logits_all || !last || !ws)
        return adaf_fail(h, ADAF_E_BADARG, "gru_cls: null pointer");
    if (batch < 0 || steps <= 0 || feat <= 0 || hidden <= 0 || classes <= 0) return adaf_fail(h, ADAF_E_BADARG, "gru_cls: non-positive extent");
    if (ldx == 0) ldx = feat;
    if (feat % 4 || hidden % 4 || ldx % 4) return adaf_fail(h, ADAF_E_LAYOUT, "gru_cls: feat, hidden, ldx must be multiples of 4");
    GruClsWs r;
    int rc = adaf_check_ws(h, "gru_cls", ws, ws_bytes, gru_cls_layout(ws, batch, steps, hidden, &r), ADAF_WS_SIZE_FIRST);
    if (rc) return rc;
    rc = gru_scan(h, x, ldx, batch, steps, feat, hidden, w_ih, w_hh, b_ih, b_hh, nullptr, r.gi, r.gh, r.hs, fc_w, fc_b, classes,
                  logits_all, last, (hipStream_t)stream);
    if (rc) return rc;
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? ADAF_OK : adaf_hip_fail(h, e, "gru_cls forward");
}

// ---- stage-3 training of the GRU classifier (gru_bptt.hip) -------------------------------------------------------------------------
struct GruTrainWs { float *gh, *hd; };     // gh [B, 3H] (the forward scan's per-step product / barrier words), the dropped-out states [B*T, H]
static size_t gru_train_layout(void* ws, int batch, int steps, int hidden, GruTrainWs* r) {
    AdafCarver c(ws);
    r->gh = c.take<float>((size_t)batch * 3 * hidden);
    r->hd = c.take<float>((size_t)batch * steps * hidden);
    return c.off;
}
size_t adaf_gru_cls_train_workspace_bytes(int batch, int steps, int hidden) {
    GruTrainWs r;
    return (batch <= 0 || steps <= 0 || hidden <= 0) ? 0 : gru_train_layout(nullptr, batch, steps, hidden, &r);
}

int adaf_gru_cls_train_forward_f32(adaf_handle* h, const float* x, int ldx, int batch, int steps, int feat, int hidden, int classes,
                                   const float* w_ih, const float* w_hh, const float* b_ih, const float* b_hh, const float* fc_w,
                                   const float* fc_b, const float* mask, float* gi_out, float* hs_out, float* logits_all, float* last,
                                   void* ws, size_t ws_bytes, void* stream) {
    if (!h) return ADAF_E_BADARG;
    if (batch == 0) return ADAF_OK;
    if (!x || !w_ih || !w_hh || !b_ih || !b_hh || !fc_w || !fc_b || !gi_out || !hs_out || !logits_all || !ws)
        return adaf_fail(h, ADAF_E_BADARG, "gru_cls_train: null pointer");
    if (batch < 0 || steps <= 0 || feat <= 0 || hidden <= 0 || classes <= 0) return adaf_fail(h, ADAF_E_BADARG, "gru_cls_train: non-positive extent");
    if (ldx == 0) ldx = feat;
    if (feat % 4 || hidden % 16 || ldx % 4) return adaf_fail(h, ADAF_E_LAYOUT, "gru_cls_train: feat %% 4, hidden %% 16, ldx %% 4 must be 0");
    GruTrainWs r;
    int rc = adaf_check_ws(h, "gru_cls_train", ws, ws_bytes, gru_train_layout(ws, batch, steps, hidden, &r), ADAF_WS_SIZE_FIRST);
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    float* const hd = r.hd;
    const int rows = batch * steps;
    rc = gru_scan(h, x, ldx, batch, steps, feat, hidden, w_ih, w_hh, b_ih, b_hh, nullptr, gi_out, r.gh, hs_out, nullptr, nullptr, 0, nullptr,
                  nullptr, st);
    if (rc) return rc;
    const float* fc_in = hs_out;
    if (mask) {
        adaf_launch_rows_scale(hs_out, mask, hd, rows, hidden, steps, false, st);
        fc_in = hd;
    }
    if ((rc = linear_launch(h, fc_in, rows, hidden, hidden, classes, fc_w, fc_b, logits_all, 0, st))) return rc;
    if (last) adaf_launch_copy2d(logits_all + (size_t)(steps - 1) * classes, steps * classes, last, classes, batch, classes, st);
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? ADAF_OK : adaf_hip_fail(h, e, "gru_cls_train forward");
}

// dropped-out / shifted states + dY [B*T, H] each, gh + dgi + dgh [B*T, 3H] each, carry [B, H], column-sum partials (of 3H or `classes`
// columns, whichever is more), the steps + 1 barrier words of the persistent scan in whole 256-byte lines
struct GruBackwardWs { float *hd, *dy, *gh, *dgi, *dgh, *carry, *part; unsigned* bar; };
static size_t gru_backward_layout(void* ws, int batch, int steps, int hidden, int classes, GruBackwardWs* r) {
    const size_t rows = (size_t)batch * steps, h3 = 3 * (size_t)hidden, narrow = rows * hidden, wide = rows * h3;
    AdafCarver c(ws);
    r->hd = c.take<float>(narrow);
    r->dy = c.take<float>(narrow);
    r->gh = c.take<float>(wide);
    r->dgi = c.take<float>(wide);
    r->dgh = c.take<float>(wide);
    r->carry = c.take<float>((size_t)batch * hidden);
    r->part = c.take<float>(adaf_colsum_partial_floats(3 * hidden > classes ? 3 * hidden : classes, 1));
    r->bar = c.take<unsigned>((size_t)steps + 1, 256);
    return c.off;
}
size_t adaf_gru_cls_backward_workspace_bytes(int batch, int steps, int hidden, int classes) {
    GruBackwardWs r;
    return (batch <= 0 || steps <= 0 || hidden <= 0 || classes <= 0) ? 0 : gru_backward_layout(nullptr, batch, steps, hidden, classes, &r);
}

int adaf_gru_cls_backward_f32(adaf_handle* h, const float* x, int ldx, int batch, int steps, int feat, int hidden, int classes,
                              const float* w_ih, const float* w_hh, const float* b_hh, const float* fc_w, const float* gi,
                              const float* hs, const float* mask, const float* dlogits, float* dx, float* dw_ih, float* dw_hh,
                              float* db_ih, float* db_hh, float* dw_fc, float* db_fc, void* ws, size_t ws_bytes, void* stream) {
    if (!h) return ADAF_E_BADARG;
    if (!x || !w_ih || !w_hh || !b_hh || !fc_w || !gi || !hs || !dlogits || !dw_ih || !dw_hh || !db_ih || !db_hh || !dw_fc || !db_fc || !ws)
        return adaf_fail(h, ADAF_E_BADARG, "gru_cls_backward: null pointer");
    if (batch <= 0 || steps <= 0 || feat <= 0 || hidden <= 0 || classes <= 0) return adaf_fail(h, ADAF_E_BADARG, "gru_cls_backward: non-positive extent");
    if (ldx == 0) ldx = feat;
    if (feat % 4 || hidden % 16 || ldx % 4 || ldx < feat) return adaf_fail(h, ADAF_E_LAYOUT, "gru_cls_backward: feat %% 4, hidden %% 16, ldx %% 4 must be 0");
    GruBackwardWs r;
    int rc = adaf_check_ws(h, "gru_cls_backward", ws, ws_bytes, gru_backward_layout(ws, batch, steps, hidden, classes, &r), ADAF_WS_SIZE_FIRST);
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    const int rows = batch * steps, h3 = 3 * hidden;
    float *const hd = r.hd, *const dy = r.dy, *const gh = r.gh, *const dgi = r.dgi, *const dgh = r.dgh, *const carry = r.carry, *const part = r.part;
    unsigned* const bar = r.bar;
    // FC + dropout: dW_fc = dlogits^T (hs * mask), db_fc = column sums, dY = (dlogits W_fc) * mask
    adaf_launch_rows_scale(hs, mask, hd, rows, hidden, steps, false, st);
    adaf_launch_gemm_strided(dlogits, 1, classes, hd, hidden, 1, dw_fc, hidden, nullptr, 0, classes, hidden, rows, st);
    adaf_launch_colsum(dlogits, rows, classes, classes, 1, part, db_fc, st);
    adaf_launch_gemm_strided(dlogits, classes, 1, fc_w, hidden, 1, dy, hidden, mask, hidden, rows, hidden, classes, st);
    // gh = W_hh h_t + b_hh of every step in one engine GEMM (row (b, t) is step t+1's hidden projection)
    if ((rc = linear_launch(h, hs, rows, hidden, hidden, h3, w_hh, b_hh, gh, 0, st))) return rc;
    // the T-sequential part: persistent under the forward scan's rules (not under capture unless "gru_graph_persistent"), and it takes
    // EVERY scan slot -- its 104 KB of LDS leave room for one block per CU, so no forward scan of this handle may run beside it
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    (void)hipStreamIsCapturing(st, &cap);
    const bool capturing = cap != hipStreamCaptureStatusNone;
    const bool persistent = h->gru_persistent && (!capturing || adaf_options().gru_graph_persistent) &&
                            adaf_gru_bptt_persistent_ok(batch, hidden, h->bptt_resident);
    if (persistent && !capturing)
        for (int i = 0; i < h->scan_slots; ++i)
            if (h->scan_used[i]) (void)hipStreamWaitEvent(st, h->scan_done[i], 0);
    hipError_t e = adaf_launch_gru_bptt(dy, gi, gh, b_hh, hs, w_hh, dgi, dgh, carry, bar, h->scan_timeouts, batch, steps, hidden, persistent,
                                        h->gru_persistent == 2, st);
    if (e != hipSuccess) return adaf_hip_fail(h, e, "gru bptt launch");
    if (persistent && !capturing)
        for (int i = 0; i < h->scan_slots; ++i) {
            (void)hipEventRecord(h->scan_done[i], st);
            h->scan_used[i] = true;
        }
    // weight gradients: dW_ih = dgi^T x, dW_hh = dgh^T h_{t-1} (h_{-1} = 0), bias gradients, dx = dgi W_ih
    adaf_launch_rows_scale(hs, nullptr, hd, rows, hidden, steps, true, st);
    adaf_launch_gemm_strided(dgi, 1, h3, x, ldx, 1, dw_ih, feat, nullptr, 0, h3, feat, rows, st);
    adaf_launch_gemm_strided(dgh, 1, h3, hd, hidden, 1, dw_hh, hidden, nullptr, 0, h3, hidden, rows, st);
    adaf_launch_colsum(dgi, rows, h3, h3, 1, part, db_ih, st);
    adaf_launch_colsum(dgh, rows, h3, h3, 1, part, db_hh, st);
    if (dx) adaf_launch_gemm_strided(dgi, h3, 1, w_ih, feat, 1, dx, feat, nullptr, 0, rows, feat, h3, st);
    e = hipGetLastError();
    return e == hipSuccess ? ADAF_OK : adaf_hip_fail(h, e, "gru_cls backward");
}

int adaf_fc_meanpool_forward_f32(adaf_handle* h, const float* feat, int batch, int steps, int feat_dim, int classes,
                                 const float* fc_w, const float* fc_b, const float* global_logit, int global_steps,
                                 float* out, void* ws, size_t ws_bytes, void* stream) {
    if (!h) return ADAF_E_BADARG;
    if (batch == 0) return ADAF_OK;
    if (!feat || !fc_w || !fc_b || !out || !ws) return adaf_fail(h, ADAF_E_BADARG, "fc_meanpool: null pointer");
    if (batch < 0 || steps <= 0 || feat_dim <= 0 || classes <= 0 || (global_logit && global_steps <= 0))
        return adaf_fail(h, ADAF_E_BADARG, "fc_meanpool: non-positive extent");
    if (feat_dim % 4) return adaf_fail(h, ADAF_E_LAYOUT, "fc_meanpool: feat_dim %% 4");
    AdafCarver c(ws);
    float* logit = c.take<float>((size_t)batch * steps * classes);      // the whole layout: the per-step logits [B*T, C]
    int rc = adaf_check_ws(h, "fc_meanpool", ws, ws_bytes, c.off, ADAF_WS_SIZE_FIRST);
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    rc = linear_launch(h, feat, batch * steps, feat_dim, feat_dim, classes, fc_w, fc_b, logit, 0, st);
    if (rc) return rc;
    adaf_launch_segment_mean(logit, batch, steps, classes, global_logit, global_steps, out, st);
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? ADAF_OK : adaf_hip_fail(h, e, "fc_meanpool forward");
}


int adaf_pack_dw_weight_f32(adaf_handle* h, const float* w_c133, int channels, float* w_33c, void* stream) {
    if (!h) return ADAF_E_BADARG;
    if (!w_c133 || !w_33c || channels <= 0) return adaf_fail(h, ADAF_E_BADARG, "pack_dw: bad arguments");
    adaf_launch_pack_dw_weight(w_c133, channels, w_33c, (hipStream_t)stream);
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? ADAF_OK : adaf_hip_fail(h, e, "pack_dw launch");
}

int adaf_dwconv3x3_bn_act_f32(adaf_handle* h, const float* x, int n, int hh, int ww, int c, int stride,
                              const float* w_33c, const float* scale, const float* bias, int act, float* out,
                              void* stream) {
    if (!h) return ADAF_E_BADARG;
    if (!x || !w_33c || !scale || !bias || !out || n <= 0 || hh <= 0 || ww <= 0 || c <= 0) return adaf_fail(h, ADAF_E_BADARG, "dwconv: bad arguments");
    if (stride != 1 && stride != 2) return adaf_fail(h, ADAF_E_BADARG, "dwconv: stride must be 1 or 2");
    if (act < ADAF_ACT_NONE || act > ADAF_ACT_RELU6) return adaf_fail(h, ADAF_E_BADARG, "dwconv: activation");
    if (c % 4 || !adaf_aligned16(x) || !adaf_aligned16(out) || !adaf_aligned16(w_33c) || !adaf_aligned16(scale) || !adaf_aligned16(bias))
        return adaf_fail(h, ADAF_E_LAYOUT, "dwconv: c %% 4 == 0 and 16-byte alignment required");
    adaf_launch_dwconv3x3(x, n, hh, ww, c, stride, w_33c, scale, bias, act, out, (hipStream_t)stream);
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? ADAF_OK : adaf_hip_fail(h, e, "dwconv launch");
}

int adaf_grid_actions_f32(adaf_handle* h, const float* logits, int rows, int n_actions, const float* table_yx,
                          int64_t* idx_out, float* action_out, void* stream) {
    if (!h) return ADAF_E_BADARG;
    if (rows == 0) return ADAF_OK;
    if (!logits || rows < 0 || n_actions <= 0 || (!action_out && !idx_out) || (action_out && !table_yx))
        return adaf_fail(h, ADAF_E_BADARG, "grid_actions: bad arguments");
    adaf_launch_grid_actions(logits, rows, n_actions, table_yx, reinterpret_cast<long long*>(idx_out), action_out, (hipStream_t)stream);
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? ADAF_OK : adaf_hip_fail(h, e, "grid_actions launch");
}

}  // extern "C"
