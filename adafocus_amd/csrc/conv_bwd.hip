// Backward primitives of the ResNet trunk's convolutions (stage 3 of the Something-Something tree fine-tunes the local CNN with frozen
// BatchNorm statistics: STH/stage3.py:189-193, 313-317).  fp32, NHWC activations, OHWI filters -- the engine's layouts.  No
// atomics: every output element has one writer and every sum a fixed order, so the same inputs give the same bits.
//
//   the weight gradient        G[o, kh, kw, i] = sum over output pixels of g[pixel, o] x[window(pixel, kh, kw), i]: a TN GEMM whose reduction
//                              axis is the pixel axis, on splitk_wgrad_kernel (splitk_wgrad.h) -- its window source (an implicit
//                              im2col), or its pointwise source for a 1x1 stride-1 convolution --, the slice partials added in slice order
//                              by the slice sum of train_common.hip
//   conv_dgrad_pack_kernel     the filter transposed, rotated by 180 degrees, times the folded BN scale per output channel: the data
//                              gradient is then a stride-1 convolution of the gradient map on the forward engine (conv_gemm.hip)
//   conv_zero_insert_kernel    stride 2: a low-resolution map written into the even positions of a zeroed full-resolution one (gather form)
//   relu_backward_kernel, avgpool_backward_kernel, maxpool_backward_kernel, tshift_backward_kernel, conv_bn_param_grad_kernel
#include "adaf_internal.h"
#include "splitk_wgrad.h"

namespace {

inline unsigned blocks_for(size_t n, int per = 256) { return (unsigned)((n + per - 1) / per); }

// the weight gradient's launch: M = cout as one or two sets of 32 filter rows per block (the last block's rows past cout are bounded off:
// splitk_wgrad.h), K = kh * kw * cin in chunks of 128.  The slices are planned for the MI355X's 256 CUs whatever the device reports: the
// query needs no handle
struct WgradPlan { int mh; SkPlan sk; };
WgradPlan wgrad_plan(long long npix, int cout, int K) {
    const int mh = cout % 64 == 0 ? 2 : 1;
    return {mh, splitk_plan(npix, (long long)((K + 127) / 128) * ((cout + 32 * mh - 1) / (32 * mh)), kSkCus)};
}

// ---- data gradient -------------------------------------------------------------------------------------------------------------------
// o[i][kh][kw][c] = w[c][KH - 1 - kh][KW - 1 - kw][i] * scale[c]   (scale == nullptr: 1)
__global__ void conv_dgrad_pack_kernel(const float* __restrict__ w, const float* __restrict__ scale, int cout, int kh, int kw, int cin,
                                       float* __restrict__ o) {
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x, total = (size_t)cin * kh * kw * cout;
    if (idx >= total) return;
    const int c = (int)(idx % cout);
    size_t t = idx / cout;
    const int x = (int)(t % kw);
    t /= kw;
    const int y = (int)(t % kh), i = (int)(t / kh);
    const float v = w[(((size_t)c * kh + (kh - 1 - y)) * kw + (kw - 1 - x)) * cin + i];
    o[idx] = scale ? v * scale[c] : v;
}

// hi[n, y, x, :] = lo[n, y / 2, x / 2, :] where y and x are even, else 0; 4 channels per thread
__global__ void conv_zero_insert_kernel(const float* __restrict__ lo, int n, int lh, int lw, int hh, int hw, int c4, float* __restrict__ hi) {
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x, total = (size_t)n * hh * hw * c4;
    if (idx >= total) return;
    const int cq = (int)(idx % c4);
    size_t t = idx / c4;
    const int x = (int)(t % hw);
    t /= hw;
    const int y = (int)(t % hh), img = (int)(t / hh);
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (!(y & 1) && !(x & 1) && (y >> 1) < lh && (x >> 1) < lw)
        v = *reinterpret_cast<const f32x4*>(lo + ((((size_t)img * lh + (y >> 1)) * lw + (x >> 1)) * c4 + cq) * 4);
    *reinterpret_cast<f32x4*>(hi + idx * 4) = v;
}

// ---- the one-pass kernels ------------------------------------------------------------------------------------------------------------
// out = (dy [+ dy2]) where y > 0, else 0
__global__ void relu_backward_kernel(const float* __restrict__ dy, const float* __restrict__ dy2, const float* __restrict__ y, size_t n,
                                     float* __restrict__ out) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float v = dy2 ? dy[i] + dy2[i] : dy[i];
    out[i] = y[i] > 0.f ? v : 0.f;
}

// out[img, p, c] = dfeat[img * ldd + c] / hw  (where y[img, p, c] > 0 when y is given)
__global__ void avgpool_backward_kernel(const float* __restrict__ dfeat, int ldd, const float* __restrict__ y, size_t total, int hw, int c,
                                        float* __restrict__ out) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int ch = (int)(i % c);
    const size_t img = i / c / hw;
    const float v = dfeat[img * ldd + ch] / (float)hw;
    out[i] = (!y || y[i] > 0.f) ? v : 0.f;
}

// MaxPool2d(3, 2, 1) backward, one thread per INPUT element: it inspects the at most four windows that contain it and adds the gradient of
// those whose arg-max it is (ascending window order).  The arg-max of a window is its first maximum in row-major order (ATen's forward keeps
// an element only when it is greater than the best so far): an element wins iff everything before it is smaller and nothing after it is larger.
__global__ void maxpool_backward_kernel(const float* __restrict__ x, const float* __restrict__ g, int n, int h, int w, int c, int oh, int ow,
                                        float* __restrict__ dx) {
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x, total = (size_t)n * h * w * c;
    if (idx >= total) return;
    const int ch = (int)(idx % c);
    size_t t = idx / c;
    const int ix = (int)(t % w);
    t /= w;
    const int iy = (int)(t % h), img = (int)(t / h);
    const float me = x[idx];
    const float* xi = x + (size_t)img * h * w * c + ch;
    float sum = 0.f;
    for (int oy = iy / 2; oy <= (iy + 1) / 2; ++oy) {           // windows with 2 oy - 1 <= iy <= 2 oy + 1
        if (oy >= oh) continue;
        for (int ox = ix / 2; ox <= (ix + 1) / 2; ++ox) {
            if (ox >= ow) continue;
            bool win = true;
#pragma unroll
            for (int ky = 0; ky < 3; ++ky)
#pragma unroll
                for (int kx = 0; kx < 3; ++kx) {
                    const int yy = 2 * oy - 1 + ky, xx = 2 * ox - 1 + kx;
                    if (yy < 0 || yy >= h || xx < 0 || xx >= w || (yy == iy && xx == ix)) continue;
                    const float v = xi[((size_t)yy * w + xx) * c];
                    const bool before = yy < iy || (yy == iy && xx < ix);
                    win = win && (before ? v < me : v <= me);
                }
            if (win) sum += g[(((size_t)img * oh + oy) * ow + ox) * c + ch];
        }
    }
    dx[idx] = sum;
}

// The adjoint of TemporalShift.shift (tshift_kernel of misc_ops.hip): the forward moves the first fold channels from t + 1 and the next fold
// from t - 1, so their gradients travel the other way; zeros at the clip ends
__global__ void tshift_backward_kernel(const float* __restrict__ g, long long total, int c, int hw, int T, int fold, int nhwc,
                                       float* __restrict__ o) {
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= total) return;
    const long long frame_elems = (long long)c * hw;
    const long long f = idx / frame_elems;
    const int within = (int)(idx - f * frame_elems);
    const int ch = nhwc ? within % c : within / hw;
    const int t = (int)(f % T);
    float v;
    if (ch < fold) v = (t > 0) ? g[idx - frame_elems] : 0.f;               // out[t - 1] read x[t]
    else if (ch < 2 * fold) v = (t < T - 1) ? g[idx + frame_elems] : 0.f;  // out[t + 1] read x[t]
    else v = g[idx];
    o[idx] = v;
}

// One block of 256 threads per output channel o, from the unscaled weight gradient G (OHWI, cin_pad channels) and the forward's packed
// filter W (the same layout):  dW[o] = scale[o] G[o] in PyTorch's OIHW layout with the cin real channels;  dbeta[o] = colsum[o];
// dgamma[o] = invstd[o] (<W[o], G[o]> - mean[o] colsum[o]), invstd = 1 / sqrt(var + eps): nothing divides by gamma or by the folded scale.
// The dot product: thread t adds its columns t, t + 256, ... in ascending order, then a fixed tree over the 256 partials.
__global__ __launch_bounds__(256) void conv_bn_param_grad_kernel(const float* __restrict__ G, const float* __restrict__ W,
                                                                  const float* __restrict__ scale, const float* __restrict__ mean,
                                                                  const float* __restrict__ var, float eps, const float* __restrict__ colsum,
                                                                  int khw, int cin, int cin_pad, float* __restrict__ dw_oihw,
                                                                  float* __restrict__ dgamma, float* __restrict__ dbeta) {
    __shared__ float red[256];
    const int o = blockIdx.x, tid = threadIdx.x, K = khw * cin_pad;
    const float* go = G + (size_t)o * K;
    const float* wo = W + (size_t)o * K;
    const float s = scale[o];
    float dot = 0.f;
    for (int k = tid; k < K; k += 256) {
        const float gv = go[k];
        dot += wo[k] * gv;
        const int tap = k / cin_pad, i = k - tap * cin_pad;
        if (dw_oihw && i < cin) dw_oihw[((size_t)o * cin + i) * khw + tap] = s * gv;
    }
    red[tid] = dot;
    __syncthreads();
#pragma unroll
    for (int step = 128; step > 0; step >>= 1) {
        if (tid < step) red[tid] = red[tid] + red[tid + step];
        __syncthreads();
    }
    if (tid == 0) {
        const float cs = colsum[o];
        if (dgamma) dgamma[o] = (red[0] - mean[o] * cs) / sqrtf(var[o] + eps);
        if (dbeta) dbeta[o] = cs;
    }
}

// ---- host side -----------------------------------------------------------------------------------------------------------------------
struct ConvGeom { int oh, ow; long long npix_out, npix_in; int K; };
// the checks both gradients share; x / g / out may be null in a query
int conv_bwd_geom(adaf_handle* h, const char* who, const adaf_conv_params* p, ConvGeom* q) {
    if (!p) return h ? adaf_fail(h, ADAF_E_BADARG, "%s: null pointer", who) : ADAF_E_BADARG;
    if (p->n <= 0 || p->h <= 0 || p->w <= 0 || p->cin <= 0 || p->cout <= 0 || p->kh <= 0 || p->kw <= 0 || p->stride <= 0 || p->pad < 0)
        return h ? adaf_fail(h, ADAF_E_BADARG, "%s: non-positive extent", who) : ADAF_E_BADARG;
    q->oh = adaf_conv_out(p->h, p->kh, p->stride, p->pad);
    q->ow = adaf_conv_out(p->w, p->kw, p->stride, p->pad);
    if (q->oh <= 0 || q->ow <= 0) return h ? adaf_fail(h, ADAF_E_BADARG, "%s: empty output", who) : ADAF_E_BADARG;
    q->npix_out = (long long)p->n * q->oh * q->ow;
    q->npix_in = (long long)p->n * p->h * p->w;
    if (q->npix_out > 0x7fffffffLL || q->npix_in > 0x7fffffffLL) return h ? adaf_fail(h, ADAF_E_BADARG, "%s: too many pixels", who) : ADAF_E_BADARG;
    q->K = p->kh * p->kw * p->cin;
    if (p->cin % 4 || p->cout % 4 || (p->ldx && p->ldx != p->cin) || (p->ldo && p->ldo != p->cout) || p->tsm_segments > 0)
        return h ? adaf_fail(h, ADAF_E_LAYOUT, "%s: dense maps with cin %% 4 == 0 and cout %% 4 == 0, no fused temporal shift", who) : ADAF_E_LAYOUT;
    return ADAF_OK;
}

size_t wgrad_layout(void* ws, const WgradPlan& pl, int cout, int K, float** part) {
    AdafCarver c(ws);
    *part = c.take<float>((size_t)pl.sk.slices * cout * K, 16);
    return c.off;
}

// stride 1: nothing.  1x1 stride 2: the low-resolution data gradient [n, oh, ow, cin].  k x k stride 2: the zero-inserted gradient [n, h, w, cout]
size_t dgrad_layout(void* ws, const adaf_conv_params* p, const ConvGeom& q, float** buf) {
    AdafCarver c(ws);
    *buf = nullptr;
    if (p->stride == 2) *buf = c.take<float>(p->kh == 1 && p->kw == 1 ? (size_t)q.npix_out * p->cin : (size_t)q.npix_in * p->cout, 16);
    return c.off;
}

bool dgrad_shape_ok(const adaf_conv_params* p) {
    if (p->kh != p->kw || p->pad > p->kh - 1) return false;
    if (p->stride == 1) return true;
    return p->stride == 2 && ((p->kh == 1 && p->pad == 0) || (p->kh == 3 && p->pad == 1));
}

// Both weight-gradient exports: cout a multiple of `cout_mult` -- 32, whole blocks of filter rows, or 4, the last block bounded.
size_t wgrad_bytes(const adaf_conv_params* p, int cout_mult) {
    ConvGeom q;
    if (conv_bwd_geom(nullptr, "", p, &q) || p->cout % cout_mult) return 0;
    float* part;
    return wgrad_layout(nullptr, wgrad_plan(q.npix_out, p->cout, q.K), p->cout, q.K, &part);
}

int wgrad_run(adaf_handle* h, const char* who, int cout_mult, const adaf_conv_params* p, const float* x, const float* g, float* dw_ohwi, void* ws,
              size_t ws_bytes, void* stream) {
    if (!h) return ADAF_E_BADARG;
    if (!x || !g || !dw_ohwi || !ws) return adaf_fail(h, ADAF_E_BADARG, "%s: null pointer", who);
    ConvGeom q;
    int rc = conv_bwd_geom(h, who, p, &q);
    if (rc) return rc;
    if (p->cout % cout_mult) return adaf_fail(h, ADAF_E_LAYOUT, "%s: cout=%d must be a multiple of %d", who, p->cout, cout_mult);
    if (!adaf_aligned16(x) || !adaf_aligned16(g) || !adaf_aligned16(dw_ohwi)) return adaf_fail(h, ADAF_E_LAYOUT, "%s: 16-byte alignment", who);
    const WgradPlan pl = wgrad_plan(q.npix_out, p->cout, q.K);
    float* part;
    if ((rc = adaf_check_ws(h, who, ws, ws_bytes, wgrad_layout(ws, pl, p->cout, q.K, &part), ADAF_WS_ALIGN_FIRST))) return rc;
    hipStream_t st = (hipStream_t)stream;
    const int npix = (int)q.npix_out;
    auto launch = [&](const auto& src) {
        if (pl.mh == 2)
            splitk_wgrad_launch<1, 2>(src, part, npix, q.K, p->cout, pl.sk, st);
        else
            splitk_wgrad_launch<1, 1>(src, part, npix, q.K, p->cout, pl.sk, st);
    };
    if (p->kh == 1 && p->kw == 1 && p->stride == 1 && p->pad == 0)      // the window of output pixel p is input pixel p
        launch(SkPointwise<false>{x, g, nullptr, q.K, p->cout});
    else
        launch(SkWindow{x, g, p->cin, p->cout, p->h, p->w, q.oh, q.ow, p->kw, p->stride, p->pad});
    adaf_launch_slice_sum(part, pl.sk.used, (size_t)p->cout * q.K, dw_ohwi, st);
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? ADAF_OK : adaf_hip_fail(h, e, who);
}

}  // namespace

extern "C" {

size_t adaf_conv2d_wgrad_workspace_bytes(const adaf_conv_params* p) { return wgrad_bytes(p, 32); }
size_t adaf_conv2d_wgrad_rows_workspace_bytes(const adaf_conv_params* p) { return wgrad_bytes(p, 4); }

int adaf_conv2d_wgrad_f32(adaf_handle* h, const adaf_conv_params* p, const float* x, const float* g, float* dw_ohwi, void* ws,
                          size_t ws_bytes, void* stream) {
    return wgrad_run(h, "conv_wgrad", 32, p, x, g, dw_ohwi, ws, ws_bytes, stream);
}

int adaf_conv2d_wgrad_rows_f32(adaf_handle* h, const adaf_conv_params* p, const float* x, const float* g, float* dw_ohwi, void* ws,
                               size_t ws_bytes, void* stream) {
    return wgrad_run(h, "conv_wgrad_rows", 4, p, x, g, dw_ohwi, ws, ws_bytes, stream);
}

int adaf_pack_conv_dgrad_weight_f32(adaf_handle* h, const float* w_ohwi, const float* scale, int cout, int kh, int kw, int cin, float* w_dgrad,
                                    void* stream) {
    if (!h) return ADAF_E_BADARG;
    if (!w_ohwi || !w_dgrad || cout <= 0 || kh <= 0 || kw <= 0 || cin <= 0) return adaf_fail(h, ADAF_E_BADARG, "pack_dgrad: bad arguments");
    hipLaunchKernelGGL(conv_dgrad_pack_kernel, dim3(blocks_for((size_t)cin * kh * kw * cout)), dim3(256), 0, (hipStream_t)stream, w_ohwi, scale,
                       cout, kh, kw, cin, w_dgrad);
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? ADAF_OK : adaf_hip_fail(h, e, "pack_dgrad launch");
}

size_t adaf_conv2d_dgrad_workspace_bytes(const adaf_conv_params* p) {
    ConvGeom q;
    if (conv_bwd_geom(nullptr, "", p, &q) || !dgrad_shape_ok(p)) return 0;
    float* buf;
    return dgrad_layout(nullptr, p, q, &buf);
}

int adaf_conv2d_dgrad_f32(adaf_handle* h, const adaf_conv_params* p, const float* g, const float* w_dgrad, float* dx, void* ws, size_t ws_bytes,
                          void* stream) {
    if (!h) return ADAF_E_BADARG;
    if (!g || !w_dgrad || !dx) return adaf_fail(h, ADAF_E_BADARG, "conv_dgrad: null pointer");
    ConvGeom q;
    int rc = conv_bwd_geom(h, "conv_dgrad", p, &q);
    if (rc) return rc;
    if (!dgrad_shape_ok(p))
        return adaf_fail(h, ADAF_E_BADARG, "conv_dgrad: square filters with pad <= k - 1; stride 1, or stride 2 as 1x1 pad 0 / 3x3 pad 1");
    if (!adaf_aligned16(g) || !adaf_aligned16(dx)) return adaf_fail(h, ADAF_E_LAYOUT, "conv_dgrad: 16-byte alignment");
    float* buf;
    const size_t need = dgrad_layout(ws, p, q, &buf);
    if (need) {
        if (!ws) return adaf_fail(h, ADAF_E_BADARG, "conv_dgrad: null workspace");
        if ((rc = adaf_check_ws(h, "conv_dgrad", ws, ws_bytes, need, ADAF_WS_ALIGN_FIRST))) return rc;
    }
    hipStream_t st = (hipStream_t)stream;
    const bool s2 = p->stride == 2, point = p->kh == 1;
    // the engine launch: a stride-1 convolution of a gradient map with cout channels into a map with cin channels
    adaf_conv_params e = {};
    e.n = p->n; e.cin = p->cout; e.cout = p->cin; e.kh = p->kh; e.kw = p->kw; e.stride = 1; e.pad = p->kh - 1 - p->pad; e.act = ADAF_ACT_NONE;
    const float* src = g;
    float* dst = dx;
    if (!s2) { e.h = q.oh; e.w = q.ow; }
    else if (point) { e.h = q.oh; e.w = q.ow; dst = buf; }         // at the low resolution, scattered afterwards
    else {                                                          // zero-inserted to the input's size: the border comes out right for odd and even maps
        e.h = p->h; e.w = p->w; src = buf;
        hipLaunchKernelGGL(conv_zero_insert_kernel, dim3(blocks_for((size_t)q.npix_in * (p->cout / 4))), dim3(256), 0, st, g, p->n, q.oh, q.ow,
                           p->h, p->w, p->cout / 4, buf);
    }
    ConvArgs a;
    if ((rc = adaf_make_conv_args(h, &e, src, w_dgrad, nullptr, nullptr, nullptr, dst, &a))) return rc;
    if (a.OH != (s2 && point ? q.oh : p->h) || a.OW != (s2 && point ? q.ow : p->w)) return adaf_fail(h, ADAF_E_BADARG, "conv_dgrad: geometry");
    if (adaf_launch_conv_gemm(a, 0, h->cus, st) < 0) return adaf_fail(h, ADAF_E_LAUNCH, "conv_dgrad: no tile");
    if (s2 && point)
        hipLaunchKernelGGL(conv_zero_insert_kernel, dim3(blocks_for((size_t)q.npix_in * (p->cin / 4))), dim3(256), 0, st, buf, p->n, q.oh, q.ow,
                           p->h, p->w, p->cin / 4, dx);
    hipError_t er = hipGetLastError();
    return er == hipSuccess ? ADAF_OK : adaf_hip_fail(h, er, "conv_dgrad launch");
}

int adaf_relu_backward_f32(adaf_handle* h, const float* dy, const float* dy2, const float* y, size_t count, float* out, void* stream) {
    if (!h) return ADAF_E_BADARG;
    if (count == 0) return ADAF_OK;
    if (!dy || !y || !out) return adaf_fail(h, ADAF_E_BADARG, "relu_backward: null pointer");
    hipLaunchKernelGGL(relu_backward_kernel, dim3(blocks_for(count)), dim3(256), 0, (hipStream_t)stream, dy, dy2, y, count, out);
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? ADAF_OK : adaf_hip_fail(h, e, "relu_backward launch");
}

int adaf_global_avgpool_backward_f32(adaf_handle* h, const float* dfeat, int ldd, const float* y, int n, int hw, int c, float* out, void* stream) {
    if (!h) return ADAF_E_BADARG;
    if (!dfeat || !out || n <= 0 || hw <= 0 || c <= 0) return adaf_fail(h, ADAF_E_BADARG, "avgpool_backward: bad arguments");
    if (ldd == 0) ldd = c;
    if (ldd < c) return adaf_fail(h, ADAF_E_BADARG, "avgpool_backward: row stride smaller than channels");
    const size_t total = (size_t)n * hw * c;
    hipLaunchKernelGGL(avgpool_backward_kernel, dim3(blocks_for(total)), dim3(256), 0, (hipStream_t)stream, dfeat, ldd, y, total, hw, c, out);
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? ADAF_OK : adaf_hip_fail(h, e, "avgpool_backward launch");
}

int adaf_maxpool3x3s2_backward_f32(adaf_handle* h, const float* x, const float* g, int n, int hh, int ww, int c, float* dx, void* stream) {
    if (!h) return ADAF_E_BADARG;
    if (!x || !g || !dx || n <= 0 || hh <= 0 || ww <= 0 || c <= 0) return adaf_fail(h, ADAF_E_BADARG, "maxpool_backward: bad arguments");
    const size_t total = (size_t)n * hh * ww * c;
    hipLaunchKernelGGL(maxpool_backward_kernel, dim3(blocks_for(total)), dim3(256), 0, (hipStream_t)stream, x, g, n, hh, ww, c, (hh - 1) / 2 + 1,
                       (ww - 1) / 2 + 1, dx);
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? ADAF_OK : adaf_hip_fail(h, e, "maxpool_backward launch");
}

int adaf_temporal_shift_backward_f32(adaf_handle* h, const float* g, int nt, int c, int hw, int n_segment, int fold_div, int layout, float* out,
                                     void* stream) {
    if (!h) return ADAF_E_BADARG;
    if (nt == 0) return ADAF_OK;
    if (!g || !out || nt < 0 || c <= 0 || hw <= 0 || n_segment <= 0 || fold_div <= 0) return adaf_fail(h, ADAF_E_BADARG, "tshift_backward: bad arguments");
    if (nt % n_segment) return adaf_fail(h, ADAF_E_BADARG, "tshift_backward: nt=%d not a multiple of n_segment=%d", nt, n_segment);
    if (layout != ADAF_LAYOUT_NCHW && layout != ADAF_LAYOUT_NHWC) return adaf_fail(h, ADAF_E_LAYOUT, "tshift_backward: layout");
    if (g == out) return adaf_fail(h, ADAF_E_BADARG, "tshift_backward: in-place shift is not supported");
    const long long total = (long long)nt * c * hw;
    hipLaunchKernelGGL(tshift_backward_kernel, dim3(blocks_for((size_t)total)), dim3(256), 0, (hipStream_t)stream, g, total, c, hw, n_segment,
                       c / fold_div, layout == ADAF_LAYOUT_NHWC ? 1 : 0, out);
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? ADAF_OK : adaf_hip_fail(h, e, "tshift_backward launch");
}

// The stem of the training walk: the trunk's own stem kernel (stem.hip), whose k order is not the generic engine's -- with it the walk's
// features are the eval engine's bit for bit.  The workspace holds the filter bank in that kernel's layout.
size_t adaf_stem7x7_workspace_bytes(void) { return adaf_stem_weight_floats() * sizeof(float); }

int adaf_stem7x7_bn_relu_f32(adaf_handle* h, const float* patches_nhwc4, int n, int patch, const float* w_oihw, const float* scale,
                             const float* bias, float* out, void* ws, size_t ws_bytes, void* stream) {
    if (!h) return ADAF_E_BADARG;
    if (!patches_nhwc4 || !w_oihw || !scale || !bias || !out || !ws) return adaf_fail(h, ADAF_E_BADARG, "stem7x7: null pointer");
    if (n <= 0 || patch <= 0) return adaf_fail(h, ADAF_E_BADARG, "stem7x7: non-positive extent");
    if ((long long)n * patch * patch > 0x7fffffffLL) return adaf_fail(h, ADAF_E_BADARG, "stem7x7: too many pixels");
    if (!adaf_aligned16(patches_nhwc4) || !adaf_aligned16(out) || !adaf_aligned16(scale) || !adaf_aligned16(bias))
        return adaf_fail(h, ADAF_E_LAYOUT, "stem7x7: 16-byte alignment");
    int rc = adaf_check_ws(h, "stem7x7", ws, ws_bytes, adaf_stem7x7_workspace_bytes(), ADAF_WS_ALIGN_FIRST);
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    adaf_launch_pack_stem_weight(w_oihw, static_cast<float*>(ws), st);
    adaf_launch_stem7x7(patches_nhwc4, n, patch, static_cast<const float*>(ws), scale, bias, out, h->cus, st);
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? ADAF_OK : adaf_hip_fail(h, e, "stem7x7 launch");
}

// The pooled forms of the stem, each on its own: the launchers of the trunk's walk (stem.hip) with the form of adaf_stem7x7_plan or a forced one.
int adaf_stem7x7_pool_form(const adaf_handle* h, int n, int patch) {
    if (!h || n <= 0 || patch <= 0) return 0;
    return adaf_stem7x7_plan(patch, n, h->cus, true, false);
}

static int stem_pool_operands(adaf_handle* h, const char* who, const void* x, const float* w_oihw, const float* scale, const float* bias, int out_dtype,
                              const void* out, void* ws, size_t ws_bytes) {
    if (!x || !w_oihw || !scale || !bias || !out || !ws) return adaf_fail(h, ADAF_E_BADARG, "%s: null pointer", who);
    if (out_dtype != ADAF_DTYPE_F32 && out_dtype != ADAF_DTYPE_F16) return adaf_fail(h, ADAF_E_BADARG, "%s: out_dtype %d", who, out_dtype);
    if (!adaf_aligned16(x) || !adaf_aligned16(out) || !adaf_aligned16(scale) || !adaf_aligned16(bias)) return adaf_fail(h, ADAF_E_LAYOUT, "%s: 16-byte alignment", who);
    return adaf_check_ws(h, who, ws, ws_bytes, adaf_stem7x7_workspace_bytes(), ADAF_WS_ALIGN_FIRST);
}

int adaf_stem7x7_pool(adaf_handle* h, const float* patches_nhwc4, int n, int patch, const float* w_oihw, const float* scale, const float* bias,
                      int form, int out_dtype, void* out, float* conv_map, int* form_used, void* ws, size_t ws_bytes, void* stream) {
    if (!h) return ADAF_E_BADARG;
    if (n <= 0 || patch <= 0) return adaf_fail(h, ADAF_E_BADARG, "stem7x7_pool: non-positive extent");
    if ((long long)n * patch * patch > 0x7fffffffLL) return adaf_fail(h, ADAF_E_BADARG, "stem7x7_pool: too many pixels");
    if (form < ADAF_STEM_FORM_AUTO || form > ADAF_STEM_FORM_UNFUSED) return adaf_fail(h, ADAF_E_BADARG, "stem7x7_pool: form %d", form);
    int rc = stem_pool_operands(h, "stem7x7_pool", patches_nhwc4, w_oihw, scale, bias, out_dtype, out, ws, ws_bytes);
    if (rc) return rc;
    if (form == ADAF_STEM_FORM_AUTO) form = adaf_stem7x7_pool_form(h, n, patch);
    if (form == ADAF_STEM_FORM_STRIP && patch != 64 && patch != 96 && patch != 128 && patch != 144)
        return adaf_fail(h, ADAF_E_BADARG, "stem7x7_pool: the strip kernel exists for patches of 64, 96, 128 and 144, not %d", patch);
    if (form == ADAF_STEM_FORM_UNFUSED && (!conv_map || !adaf_aligned16(conv_map)))
        return adaf_fail(h, ADAF_E_BADARG, "stem7x7_pool: the unfused form needs a 16-byte aligned conv_map [n, oh, oh, 64]");
    hipStream_t st = (hipStream_t)stream;
    const bool f16 = out_dtype == ADAF_DTYPE_F16;
    const float* wr = static_cast<const float*>(ws);
    adaf_launch_pack_stem_weight(w_oihw, static_cast<float*>(ws), st);
    if (form == ADAF_STEM_FORM_UNFUSED) {
        const int oh = (patch - 1) / 2 + 1;
        adaf_launch_stem7x7(patches_nhwc4, n, patch, wr, scale, bias, conv_map, h->cus, st);
        if (f16) adaf_launch_maxpool_f16out(conv_map, n, oh, oh, 64, out, st);
        else adaf_launch_maxpool(conv_map, n, oh, oh, 64, static_cast<float*>(out), st);
    } else if (!adaf_launch_stem7x7_pool(patches_nhwc4, n, patch, wr, scale, bias, static_cast<float*>(out), h->cus, st, f16, form)) {
        return adaf_fail(h, ADAF_E_LAUNCH, "stem7x7_pool: no kernel of form %d at patch %d", form, patch);
    }
    if (form_used) *form_used = form;
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? ADAF_OK : adaf_hip_fail(h, e, "stem7x7_pool launch");
}

int adaf_stem7x7_pool_frames(adaf_handle* h, const float* frames, int frames_layout, int n_frames, int height, int width, const float* action_yx,
                             int n_actions, int frames_per_action, int patch, const float* w_oihw, const float* scale, const float* bias,
                             int out_dtype, void* out, void* ws, size_t ws_bytes, void* stream) {
    if (!h) return ADAF_E_BADARG;
    if (!action_yx || n_frames <= 0 || n_actions <= 0 || frames_per_action <= 0 || height <= 0 || width <= 0)
        return adaf_fail(h, ADAF_E_BADARG, "stem7x7_pool_frames: null pointer or empty batch");
    if (frames_layout != ADAF_LAYOUT_NCHW && frames_layout != ADAF_LAYOUT_NHWC4)
        return adaf_fail(h, ADAF_E_LAYOUT, "stem7x7_pool_frames: frames must be NCHW (3 planes) or NHWC4");
    if (n_frames % frames_per_action) return adaf_fail(h, ADAF_E_BADARG, "stem7x7_pool_frames: n_frames %% frames_per_action != 0");
    const int per_set = n_frames / frames_per_action;
    if (n_actions % per_set)
        return adaf_fail(h, ADAF_E_BADARG, "stem7x7_pool_frames: n_actions=%d is not a multiple of n_frames / frames_per_action=%d", n_actions, per_set);
    if (width < height) return adaf_fail(h, ADAF_E_BADARG, "stem7x7_pool_frames: width %d < height %d (get_patch scales both axes by H - P)", width, height);
    if (patch != 64 && patch != 96 && patch != 128 && patch != 144)
        return adaf_fail(h, ADAF_E_BADARG, "stem7x7_pool_frames: the strip kernel exists for patches of 64, 96, 128 and 144, not %d", patch);
    if (patch > height) return adaf_fail(h, ADAF_E_BADARG, "stem7x7_pool_frames: patch %d larger than the frames' height %d", patch, height);
    const long long n = (long long)(n_actions / per_set) * n_frames;        // one patch per (action set, frame)
    if (n * patch * patch > 0x7fffffffLL || (long long)n_frames * height * width > 0x7fffffffLL) return adaf_fail(h, ADAF_E_BADARG, "stem7x7_pool_frames: too many pixels");
    int rc = stem_pool_operands(h, "stem7x7_pool_frames", frames, w_oihw, scale, bias, out_dtype, out, ws, ws_bytes);
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    adaf_launch_pack_stem_weight(w_oihw, static_cast<float*>(ws), st);
    if (!adaf_launch_stem7x7_pool_frames(frames, frames_layout == ADAF_LAYOUT_NHWC4, n_frames, action_yx, frames_per_action, height, width, (int)n, patch,
                                         static_cast<const float*>(ws), scale, bias, static_cast<float*>(out), h->cus, st, out_dtype == ADAF_DTYPE_F16, true))
        return adaf_fail(h, ADAF_E_LAUNCH, "stem7x7_pool_frames: no gathering kernel for this geometry");
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? ADAF_OK : adaf_hip_fail(h, e, "stem7x7_pool_frames launch");
}

int adaf_maxpool3x3s2_f16out(adaf_handle* h, const float* x, int n, int hh, int ww, int c, void* out_f16, void* stream) {
    if (!h) return ADAF_E_BADARG;
    if (!x || !out_f16 || n <= 0 || hh <= 0 || ww <= 0 || c <= 0) return adaf_fail(h, ADAF_E_BADARG, "maxpool_f16out: bad arguments");
    if (c % 4 || !adaf_aligned16(x) || ((uintptr_t)out_f16 & 7)) return adaf_fail(h, ADAF_E_LAYOUT, "maxpool_f16out: c %% 4, 16-byte aligned x and 8-byte aligned out required");
    adaf_launch_maxpool_f16out(x, n, hh, ww, c, out_f16, (hipStream_t)stream);
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? ADAF_OK : adaf_hip_fail(h, e, "maxpool_f16out launch");
}

size_t adaf_conv_bn_param_grad_workspace_bytes(int cout) {
    if (cout <= 0) return 0;
    AdafCarver c(nullptr);
    c.take<float>(adaf_colsum_partial_floats(cout, 4), 16);
    c.take<float>((size_t)cout, 16);
    return c.off;
}

int adaf_conv_bn_param_grad_f32(adaf_handle* h, const float* g, int pixels, const float* dw_ohwi, const float* w_ohwi, const float* scale,
                                const float* mean, const float* var, float eps, int cout, int kh, int kw, int cin, int cin_pad, float* dw_oihw,
                                float* dgamma, float* dbeta, void* ws, size_t ws_bytes, void* stream) {
    if (!h) return ADAF_E_BADARG;
    if (!g || !dw_ohwi || !w_ohwi || !scale || !mean || !var || !ws) return adaf_fail(h, ADAF_E_BADARG, "conv_bn_param_grad: null pointer");
    if (pixels <= 0 || cout <= 0 || kh <= 0 || kw <= 0 || cin <= 0 || cin_pad < cin) return adaf_fail(h, ADAF_E_BADARG, "conv_bn_param_grad: bad extent");
    int rc = adaf_check_ws(h, "conv_bn_param_grad", ws, ws_bytes, adaf_conv_bn_param_grad_workspace_bytes(cout), ADAF_WS_ALIGN_FIRST);
    if (rc) return rc;
    AdafCarver c(ws);
    float* part = c.take<float>(adaf_colsum_partial_floats(cout, 4), 16);
    float* cs = c.take<float>((size_t)cout, 16);
    hipStream_t st = (hipStream_t)stream;
    adaf_launch_colsum(g, pixels, cout, cout, 4, part, cs, st);      // a gradient map: up to 10^6 rows and as few as 64 columns
    hipLaunchKernelGGL(conv_bn_param_grad_kernel, dim3(cout), dim3(256), 0, st, dw_ohwi, w_ohwi, scale, mean, var, eps, cs, kh * kw, cin, cin_pad,
                       dw_oihw, dgamma, dbeta);
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? ADAF_OK : adaf_hip_fail(h, e, "conv_bn_param_grad launch");
}

}  // extern "C"
