// Backward of the depthwise 3x3 convolution (pad 1, stride 1 or 2) of MobileNetV2's InvertedResidual: the adjoints of
// adaf_dwconv3x3_bn_act_f32's convolution in its layouts -- fp32 NHWC maps with c % 4 == 0, the filter [3][3][c] of
// adaf_pack_dw_weight_f32.  No atomics, no grid barrier, every loop bounded, 64-bit element offsets (1024 frames of 112^2 x 96 are
// 4.9 GB); the same inputs give the same bits.  Every kernel compiles to zero scratch.
//
//   dw_dgrad_kernel          a GATHER: one thread per input pixel and channel quad (16-byte accesses).  dx[iy, ix] is the sum over the output
//                            pixels whose window holds (iy, ix): oy s + kh - 1 = iy.  Stride 1: kh = 0, 1, 2 at oy = iy + 1 - kh.  Stride 2:
//                            two candidates per axis, oy = (iy + 1) / 2 - j with kh = (iy + 1) % 2 + 2 j -- kh = 3 does not exist --, so a
//                            thread reads four gradient pixels, not nine, and no zero-inserted copy of g is made.  A candidate outside the
//                            map reads a clamped address and its term is dropped (a select, not a product).  Candidates in ascending j.
//   dw_wgrad_partial_kernel  a REDUCTION over output pixels of nine products per channel, on the strip walk of bn_map.hip: a block of 256
//                            threads owns CQ channel quads and one pixel slice; its 256 / CQ pixel lanes take pixels p0 + lane, p0 + lane +
//                            RL, ... in ascending order; 36 sums per thread carried in double (a product of two floats is exact in
//                            double).  A tap in the padding reads a clamped address and is dropped.  The lanes of a block meet in lane
//                            order, tap by tap, into part[(tap * slices + slice) * c + channel].
//   dw_wgrad_final_kernel    the slices of one (tap, channel) added in slice order in two levels -- 32 groups of consecutive slices, then
//                            the 32 group sums -- and rounded once into dw[tap][channel].
//   add_kernel               out = a + b on 16-byte accesses: the join of the identity's gradient with the main path's at a block with
//                            use_res_connect, whose output has no activation (adaf_relu_backward_f32 joins under a ReLU mask).
#include "adaf_internal.h"

namespace {

constexpr int kThreads = 256;
constexpr int kFinalGroups = 32;

__device__ __forceinline__ float4 ld4(const float* p, size_t off) { return *reinterpret_cast<const float4*>(p + off); }

// ---- data gradient ------------------------------------------------------------------------------------------------------------------------
template <int S>
__global__ __launch_bounds__(kThreads) void dw_dgrad_kernel(const float* __restrict__ g, const float* __restrict__ w, int hh, int ww, int c, int oh,
                                                            int ow, size_t total, float* __restrict__ dx) {
    constexpr int NC = S == 1 ? 3 : 2;          // candidate output rows / columns per input row / column
    const size_t idx = (size_t)blockIdx.x * kThreads + threadIdx.x;      // (pixel, channel quad)
    if (idx >= total) return;
    const int c4 = c >> 2, cq = (int)(idx % c4);
    size_t t = idx / c4;
    const int ix = (int)(t % ww);
    t /= ww;
    const int iy = (int)(t % hh);
    const size_t img = t / hh;
    const int c0 = cq * 4;
    // candidate j of an axis: (output coordinate, filter tap)
    const int ky0 = S == 1 ? 0 : (iy + 1) & 1, kx0 = S == 1 ? 0 : (ix + 1) & 1;
    const int oy0 = S == 1 ? iy + 1 : (iy + 1) >> 1, ox0 = S == 1 ? ix + 1 : (ix + 1) >> 1;
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int a = 0; a < NC; ++a) {
        const int kh = ky0 + S * a, oy = oy0 - a;
        const bool oky = kh <= 2 && oy >= 0 && oy < oh;
        const int khc = min(kh, 2), oyc = min(max(oy, 0), oh - 1);
#pragma unroll
        for (int b = 0; b < NC; ++b) {
            const int kw = kx0 + S * b, ox = ox0 - b;
            const bool ok = oky && kw <= 2 && ox >= 0 && ox < ow;
            const int kwc = min(kw, 2), oxc = min(max(ox, 0), ow - 1);
            const float4 gv = ld4(g, ((img * oh + oyc) * ow + oxc) * (size_t)c + c0);
            const float4 wv = ld4(w, (size_t)(khc * 3 + kwc) * c + c0);
            acc.x += ok ? gv.x * wv.x : 0.f;
            acc.y += ok ? gv.y * wv.y : 0.f;
            acc.z += ok ? gv.z * wv.z : 0.f;
            acc.w += ok ? gv.w * wv.w : 0.f;
        }
    }
    *reinterpret_cast<float4*>(dx + idx * 4) = acc;
}

// count4 quads; out may be a or b
__global__ __launch_bounds__(kThreads) void add_kernel(const float* a, const float* b, size_t count4, float* out) {
    const size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= count4) return;
    const float4 u = ld4(a, i * 4), v = ld4(b, i * 4);
    *reinterpret_cast<float4*>(out + i * 4) = make_float4(u.x + v.x, u.y + v.y, u.z + v.z, u.w + v.w);
}

// ---- weight gradient ----------------------------------------------------------------------------------------------------------------------
// channel quads per block and the slice rule of bn_map.hip (about 2048 blocks, eight per CU), with one difference: a slice holds four
// rounds of the pixel lanes at least, so a short map does not carry thousands of empty slices through the slice sum
inline int dw_cq(int c) { return c >= 256 ? 64 : 16; }
inline int dw_col_blocks(int c) { return (c / 4 + dw_cq(c) - 1) / dw_cq(c); }
inline int dw_slices(long long npix, int c) {
    int s = 2048 / dw_col_blocks(c);
    if (s < 32) s = 32;
    const long long rounds = 4LL * (kThreads / dw_cq(c));
    const long long most = (npix + rounds - 1) / rounds;
    return (int)(most < s ? (most < 1 ? 1 : most) : s);
}

// grid (channel blocks, slices)
template <int CQ, int S>
__global__ __launch_bounds__(kThreads) void dw_wgrad_partial_kernel(const float* __restrict__ x, const float* __restrict__ g, int hh, int ww, int c,
                                                                    int oh, int ow, long long npix, long long per, double* __restrict__ part) {
    constexpr int RL = kThreads / CQ, W = CQ * 4;
    __shared__ double red[RL][W];
    const int cq = threadIdx.x % CQ, lane = threadIdx.x / CQ;
    const int c0 = (blockIdx.x * CQ + cq) * 4;
    const long long p0 = (long long)blockIdx.y * per, p1 = p0 + per < npix ? p0 + per : npix;
    double acc[9][4];
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[t][j] = 0.0;
    if (c0 < c) {
        const long long ohw = (long long)oh * ow;
        for (long long p = p0 + lane; p < p1; p += RL) {
            const long long img = p / ohw;
            const int r = (int)(p - img * ohw), oy = r / ow, ox = r - oy * ow;
            const float4 g4 = ld4(g, (size_t)p * c + c0);
            const double gd[4] = {g4.x, g4.y, g4.z, g4.w};
#pragma unroll
            for (int kh = 0; kh < 3; ++kh) {
                const int iy = oy * S + kh - 1, iyc = min(max(iy, 0), hh - 1);
#pragma unroll
                for (int kw = 0; kw < 3; ++kw) {
                    const int ix = ox * S + kw - 1, ixc = min(max(ix, 0), ww - 1);
                    const bool ok = iy >= 0 && iy < hh && ix >= 0 && ix < ww;
                    const float4 x4 = ld4(x, (((size_t)img * hh + iyc) * ww + ixc) * (size_t)c + c0);
                    const float xv[4] = {x4.x, x4.y, x4.z, x4.w};
#pragma unroll
                    for (int j = 0; j < 4; ++j) acc[kh * 3 + kw][j] += ok ? gd[j] * (double)xv[j] : 0.0;
                }
            }
        }
    }
    // the pixel lanes meet in lane order, one tap at a time through one 8 KB buffer
    const int slices = gridDim.y;
#pragma unroll
    for (int t = 0; t < 9; ++t) {
#pragma unroll
        for (int j = 0; j < 4; ++j) red[lane][cq * 4 + j] = acc[t][j];
        __syncthreads();
        if (threadIdx.x < W) {
            const int col = blockIdx.x * W + threadIdx.x;
            if (col < c) {
                double s = 0.0;
#pragma unroll
                for (int l = 0; l < RL; ++l) s += red[l][threadIdx.x];
                part[((size_t)t * slices + blockIdx.y) * (size_t)c + col] = s;
            }
        }
        __syncthreads();
    }
}

// grid (ceil(9 c / 8)), 256 threads = 32 groups x 8 outputs; output o = tap * c + channel
__global__ __launch_bounds__(kThreads) void dw_wgrad_final_kernel(const double* __restrict__ part, int slices, int c, float* __restrict__ dw) {
    __shared__ double red[kFinalGroups][8];
    const int lo = threadIdx.x & 7, grp = threadIdx.x >> 3, o = blockIdx.x * 8 + lo;
    const int per = (slices + kFinalGroups - 1) / kFinalGroups, q0 = grp * per, q1 = q0 + per < slices ? q0 + per : slices;
    double a = 0.0;
    if (o < 9 * c) {
        const int tap = o / c, col = o - tap * c;
        for (int q = q0; q < q1; ++q) a += part[((size_t)tap * slices + q) * (size_t)c + col];
    }
    red[grp][lo] = a;
    __syncthreads();
    if (grp != 0 || o >= 9 * c) return;
    double s = 0.0;
#pragma unroll
    for (int l = 0; l < kFinalGroups; ++l) s += red[l][lo];
    dw[o] = (float)s;
}

struct DwGeom { int oh, ow; long long npix_in, npix_out; };
// the checks both gradients share; with h == nullptr (a query) nothing is reported
int dw_geom(adaf_handle* h, const char* who, int n, int hh, int ww, int c, int stride, DwGeom* q) {
    if (n <= 0 || hh <= 0 || ww <= 0 || c <= 0) return h ? adaf_fail(h, ADAF_E_BADARG, "%s: non-positive extent", who) : ADAF_E_BADARG;
    if (stride != 1 && stride != 2) return h ? adaf_fail(h, ADAF_E_BADARG, "%s: stride must be 1 or 2", who) : ADAF_E_BADARG;
    if (c % 4) return h ? adaf_fail(h, ADAF_E_LAYOUT, "%s: c=%d is not a multiple of 4 (16-byte accesses)", who, c) : ADAF_E_LAYOUT;
    q->oh = (hh - 1) / stride + 1;
    q->ow = (ww - 1) / stride + 1;
    q->npix_in = (long long)n * hh * ww;
    q->npix_out = (long long)n * q->oh * q->ow;
    // (one thread per input pixel and channel quad in a one-dimensional grid)
    if (q->npix_in * (c / 4) / kThreads >= 0x7fffffffLL) return h ? adaf_fail(h, ADAF_E_BADARG, "%s: too many pixels", who) : ADAF_E_BADARG;
    return ADAF_OK;
}

size_t dw_wgrad_layout(void* ws, long long npix_out, int c, double** part) {
    AdafCarver cv(ws);
    *part = cv.take<double>(9 * (size_t)dw_slices(npix_out, c) * c, 16);
    return cv.off;
}

}  // namespace

extern "C" {

int adaf_dwconv3x3_dgrad_f32(adaf_handle* h, const float* g, int n, int hh, int ww, int c, int stride, const float* w_33c, float* dx,
                             void* stream) {
    if (!h) return ADAF_E_BADARG;
    if (!g || !w_33c || !dx) return adaf_fail(h, ADAF_E_BADARG, "dwconv_dgrad: null pointer");
    DwGeom q;
    int rc = dw_geom(h, "dwconv_dgrad", n, hh, ww, c, stride, &q);
    if (rc) return rc;
    if (!adaf_aligned16(g) || !adaf_aligned16(w_33c) || !adaf_aligned16(dx)) return adaf_fail(h, ADAF_E_LAYOUT, "dwconv_dgrad: 16-byte alignment");
    const size_t total = (size_t)q.npix_in * (c / 4);
    const dim3 grid((unsigned)((total + kThreads - 1) / kThreads));
    const hipStream_t st = (hipStream_t)stream;
    if (stride == 1)
        hipLaunchKernelGGL(dw_dgrad_kernel<1>, grid, dim3(kThreads), 0, st, g, w_33c, hh, ww, c, q.oh, q.ow, total, dx);
    else
        hipLaunchKernelGGL(dw_dgrad_kernel<2>, grid, dim3(kThreads), 0, st, g, w_33c, hh, ww, c, q.oh, q.ow, total, dx);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? ADAF_OK : adaf_hip_fail(h, e, "dwconv_dgrad launch");
}

size_t adaf_dwconv3x3_wgrad_workspace_bytes(int n, int hh, int ww, int c, int stride) {
    DwGeom q;
    double* part;
    return dw_geom(nullptr, "", n, hh, ww, c, stride, &q) ? 0 : dw_wgrad_layout(nullptr, q.npix_out, c, &part);
}

int adaf_dwconv3x3_wgrad_f32(adaf_handle* h, const float* x, const float* g, int n, int hh, int ww, int c, int stride, float* dw_33c, void* ws,
                             size_t ws_bytes, void* stream) {
    if (!h) return ADAF_E_BADARG;
    if (!x || !g || !dw_33c || !ws) return adaf_fail(h, ADAF_E_BADARG, "dwconv_wgrad: null pointer");
    DwGeom q;
    int rc = dw_geom(h, "dwconv_wgrad", n, hh, ww, c, stride, &q);
    if (rc) return rc;
    if (!adaf_aligned16(x) || !adaf_aligned16(g)) return adaf_fail(h, ADAF_E_LAYOUT, "dwconv_wgrad: 16-byte alignment");
    double* part;
    if ((rc = adaf_check_ws(h, "dwconv_wgrad", ws, ws_bytes, dw_wgrad_layout(ws, q.npix_out, c, &part), ADAF_WS_ALIGN_FIRST))) return rc;
    const int slices = dw_slices(q.npix_out, c);
    const long long per = (q.npix_out + slices - 1) / slices;
    const dim3 grid(dw_col_blocks(c), slices);
    const hipStream_t st = (hipStream_t)stream;
#define DW_WGRAD(CQ, S) \
    hipLaunchKernelGGL((dw_wgrad_partial_kernel<CQ, S>), grid, dim3(kThreads), 0, st, x, g, hh, ww, c, q.oh, q.ow, q.npix_out, per, part)
    if (dw_cq(c) == 64) {
        if (stride == 1) DW_WGRAD(64, 1); else DW_WGRAD(64, 2);
    } else {
        if (stride == 1) DW_WGRAD(16, 1); else DW_WGRAD(16, 2);
    }
#undef DW_WGRAD
    hipLaunchKernelGGL(dw_wgrad_final_kernel, dim3((9 * c + 7) / 8), dim3(kThreads), 0, st, (const double*)part, slices, c, dw_33c);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? ADAF_OK : adaf_hip_fail(h, e, "dwconv_wgrad launch");
}

int adaf_add_f32(adaf_handle* h, const float* a, const float* b, size_t count, float* out, void* stream) {
    if (!h) return ADAF_E_BADARG;
    if (count == 0) return ADAF_OK;
    if (!a || !b || !out) return adaf_fail(h, ADAF_E_BADARG, "add: null pointer");
    if (count % 4 || !adaf_aligned16(a) || !adaf_aligned16(b) || !adaf_aligned16(out))
        return adaf_fail(h, ADAF_E_LAYOUT, "add: count %% 4 == 0 and 16-byte alignment required");
    if (count / 4 / kThreads >= 0x7fffffffULL) return adaf_fail(h, ADAF_E_BADARG, "add: too many elements");
    hipLaunchKernelGGL(add_kernel, dim3((unsigned)((count / 4 + kThreads - 1) / kThreads)), dim3(kThreads), 0, (hipStream_t)stream, a, b, count / 4, out);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? ADAF_OK : adaf_hip_fail(h, e, "add launch");
}

}  // extern "C"
