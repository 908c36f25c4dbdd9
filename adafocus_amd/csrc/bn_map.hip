// BatchNorm with batch statistics over tall pixel-major maps x [rows, cols] (rows = images * OH * OW, cols = channels): what training the
// local CNN in train mode needs per layer.  The bn_* kernels of ppo_train.hip walk 32 row slices of one wave per 64 columns;
// on a trunk map (10^5 ... 10^7 rows of 64 ... 2048 columns) that is a few dozen waves on a 256-CU device.  These kernels are HBM-bound
// streaming passes over the same STRIP WALK: a block of 256 threads owns a chunk of CQ column quads (16-byte accesses) and one row slice;
// its 256 / CQ row lanes take rows r0 + lane, r0 + lane + RL, ... of the slice in ascending order.
//
//   bn_map_stat_partial_kernel   per (slice, column): S1 = sum (x - k), S2 = sum (x - k)^2 in double, k = x[0, column] -- ONE read of x
//                                for both statistics.  The shift by a value of the column itself takes the cancellation out of
//                                S2 - S1^2 / n (a column whose mean is 10^4 standard deviations loses 8 digits of the plain sum of squares);
//                                x - k is exact in double
//   bn_map_stat_final_kernel     the slices added in slice order, two levels: 32 groups of consecutive slices, then the 32 group sums;
//                                mean, invstd = 1 / sqrt(biased variance + eps), the running statistics' update; rounded once
//   bn_map_normalize_kernel      y = (x - mean) * invstd * gamma + beta [+ residual] [clipped to [0, hi]: hi = +inf is ReLU, 6 is ReLU6]
//   bn_map_bwd_partial_kernel    per (slice, column): sum dy_m, sum dy_m (x - mean) in double; dy_m = dy where 0 < y < hi (y == nullptr: dy)
//   bn_map_bwd_final_kernel      dbeta, dgamma = invstd * sum dy_m (x - mean), the same two levels
//   bn_map_bwd_dx_kernel         dx = gamma invstd / n (n dy_m - dbeta - xhat dgamma)
//
// The slice count is a function of the column count alone (bn_map_slices), so a workspace query needs no row count and about 2048 blocks
// -- eight per CU -- walk any map.  Offsets are 64-bit.  fp32 maps, no atomics, no grid barrier, every loop bounded: the same inputs give
// the same bits.  Every kernel compiles to zero scratch.
#include "adaf_internal.h"

namespace {

constexpr int kThreads = 256;
constexpr int kFinalGroups = 32;      // first level of the slice sum: groups of consecutive slices

// column quads per block: a whole 1 KB row segment per wave where the map is wide enough, else the 64 columns of the narrowest trunk map
inline int bn_map_cq(int cols) { return cols >= 256 ? 64 : 16; }
inline int bn_map_col_blocks(int cols) { return (cols / 4 + bn_map_cq(cols) - 1) / bn_map_cq(cols); }
// THE slice rule: about 2048 blocks over the column blocks, 32 slices at least
inline int bn_map_slices(int cols) {
    const int s = 2048 / bn_map_col_blocks(cols);
    return s < 32 ? 32 : s;
}

struct Strip {      // what a thread of the strip walk owns
    int c;          // its first column (a multiple of 4); >= cols: no work
    int lane;       // its row lane
    long long r0, r1;
};
template <int CQ> __device__ __forceinline__ Strip strip_of(int rows, int cols, int per) {
    Strip s;
    s.c = (blockIdx.x * CQ + (int)(threadIdx.x % CQ)) * 4;
    s.lane = threadIdx.x / CQ;
    s.r0 = (long long)blockIdx.y * per;
    s.r1 = s.r0 + per < rows ? s.r0 + per : rows;
    return s;
}
__device__ __forceinline__ float4 ld4(const float* p, long long r, int cols, int c) {
    return *reinterpret_cast<const float4*>(p + (size_t)r * (size_t)cols + c);
}
__device__ __forceinline__ void st4(float* p, long long r, int cols, int c, float4 v) {
    *reinterpret_cast<float4*>(p + (size_t)r * (size_t)cols + c) = v;
}
__device__ __forceinline__ float4 col4(const float* p, int c) { return make_float4(p[c], p[c + 1], p[c + 2], p[c + 3]); }

// The row lanes of a block meet in lane order: a[0..3], b[0..3] are a thread's two sums of its four columns;
// part[(stat * slices + slice) * cols + column] receives lane 0 + lane 1 + ... of each.
template <int CQ> __device__ __forceinline__ void strip_store_partials(const double* a, const double* b, int cols, double* part) {
    constexpr int RL = kThreads / CQ, W = CQ * 4;
    __shared__ double red[RL][2 * W];
    const int cq = threadIdx.x % CQ, lane = threadIdx.x / CQ;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        red[lane][cq * 4 + j] = a[j];
        red[lane][W + cq * 4 + j] = b[j];
    }
    __syncthreads();
    const int slices = gridDim.y;
    for (int v = threadIdx.x; v < 2 * W; v += kThreads) {
        const int stat = v / W, c = blockIdx.x * W + v % W;
        if (c >= cols) continue;
        double t = 0.0;
#pragma unroll
        for (int l = 0; l < RL; ++l) t += red[l][v];
        part[((size_t)stat * slices + blockIdx.y) * (size_t)cols + c] = t;
    }
}

// grid (column blocks, slices)
template <int CQ> __global__ __launch_bounds__(kThreads) void bn_map_stat_partial_kernel(const float* __restrict__ x, int rows, int cols, int per,
                                                                                          double* __restrict__ part) {
    const Strip s = strip_of<CQ>(rows, cols, per);
    double a[4] = {0.0, 0.0, 0.0, 0.0}, b[4] = {0.0, 0.0, 0.0, 0.0};
    if (s.c < cols) {
        const float4 k4 = ld4(x, 0, cols, s.c);
        const double k[4] = {k4.x, k4.y, k4.z, k4.w};
#pragma unroll 4
        for (long long r = s.r0 + s.lane; r < s.r1; r += kThreads / CQ) {
            const float4 v4 = ld4(x, r, cols, s.c);
            const float v[4] = {v4.x, v4.y, v4.z, v4.w};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const double d = (double)v[j] - k[j];
                a[j] += d;
                b[j] += d * d;
            }
        }
    }
    strip_store_partials<CQ>(a, b, cols, part);
}

// The slice sum of two statistics of a column pair, two levels in a fixed order: thread (group, pair) adds the slices of its group in slice
// order, then the 32 group sums are added in group order.  grid (ceil(cols / 16)), 256 threads = 32 groups x 8 column pairs (16-byte loads).
// Returns true in the threads that hold a result (group 0, pair inside the map): s1[0..1], s2[0..1] of columns c, c + 1.
__device__ __forceinline__ bool slice_sum2(const double* __restrict__ part, int slices, int cols, int* c_out, double* s1, double* s2) {
    __shared__ double red[kFinalGroups][8][4];
    const int cp = threadIdx.x & 7, g = threadIdx.x >> 3, c = (blockIdx.x * 8 + cp) * 2;
    const int per = (slices + kFinalGroups - 1) / kFinalGroups, q0 = g * per, q1 = q0 + per < slices ? q0 + per : slices;
    double2 a = make_double2(0.0, 0.0), b = make_double2(0.0, 0.0);
    if (c < cols) {
#pragma unroll 4
        for (int q = q0; q < q1; ++q) {
            const double2 u = *reinterpret_cast<const double2*>(part + (size_t)q * cols + c);
            const double2 w = *reinterpret_cast<const double2*>(part + ((size_t)slices + q) * cols + c);
            a.x += u.x; a.y += u.y; b.x += w.x; b.y += w.y;
        }
    }
    red[g][cp][0] = a.x; red[g][cp][1] = a.y; red[g][cp][2] = b.x; red[g][cp][3] = b.y;
    __syncthreads();
    *c_out = c;
    if (g != 0 || c >= cols) return false;
    s1[0] = s1[1] = s2[0] = s2[1] = 0.0;
#pragma unroll
    for (int l = 0; l < kFinalGroups; ++l) {
        s1[0] += red[l][cp][0]; s1[1] += red[l][cp][1]; s2[0] += red[l][cp][2]; s2[1] += red[l][cp][3];
    }
    return true;
}

__global__ __launch_bounds__(kThreads) void bn_map_stat_final_kernel(const double* __restrict__ part, const float* __restrict__ x, int rows, int cols,
                                                                      int slices, float eps, float momentum, float* __restrict__ mean,
                                                                      float* __restrict__ invstd, float* running_mean, float* running_var) {
    int c;
    double s1[2], s2[2];
    if (!slice_sum2(part, slices, cols, &c, s1, s2)) return;
    const double n = (double)rows, m = momentum;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const double mu = (double)x[c + j] + s1[j] / n;
        double ss = s2[j] - s1[j] * s1[j] / n;          // sum of squared deviations from the mean
        ss = ss > 0.0 ? ss : 0.0;
        mean[c + j] = (float)mu;
        invstd[c + j] = (float)(1.0 / sqrt(ss / n + (double)eps));
        if (running_mean) running_mean[c + j] = (float)((1.0 - m) * (double)running_mean[c + j] + m * mu);
        if (running_var) running_var[c + j] = (float)((1.0 - m) * (double)running_var[c + j] + m * (ss / (n - 1.0)));
    }
}

template <int CQ> __global__ __launch_bounds__(kThreads) void bn_map_normalize_kernel(const float* __restrict__ x, const float* __restrict__ mean,
                                                                                       const float* __restrict__ invstd, const float* __restrict__ gamma,
                                                                                       const float* __restrict__ beta, const float* __restrict__ res,
                                                                                       int rows, int cols, int per, int relu, float hi,
                                                                                       float* __restrict__ y) {
    const Strip s = strip_of<CQ>(rows, cols, per);
    if (s.c >= cols) return;
    const float4 m4 = col4(mean, s.c), i4 = col4(invstd, s.c), g4 = col4(gamma, s.c), b4 = col4(beta, s.c);
    const float m[4] = {m4.x, m4.y, m4.z, m4.w}, is[4] = {i4.x, i4.y, i4.z, i4.w}, g[4] = {g4.x, g4.y, g4.z, g4.w}, b[4] = {b4.x, b4.y, b4.z, b4.w};
#pragma unroll 4
    for (long long r = s.r0 + s.lane; r < s.r1; r += kThreads / CQ) {
        const float4 v4 = ld4(x, r, cols, s.c);
        const float4 r4 = res ? ld4(res, r, cols, s.c) : make_float4(0.f, 0.f, 0.f, 0.f);
        const float v[4] = {v4.x, v4.y, v4.z, v4.w}, rr[4] = {r4.x, r4.y, r4.z, r4.w};
        float o[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float t = (v[j] - m[j]) * is[j] * g[j] + b[j];
            if (res) t += rr[j];
            o[j] = relu ? fminf(fmaxf(t, 0.f), hi) : t;      // (hi = +inf: the minimum changes nothing)
        }
        st4(y, r, cols, s.c, make_float4(o[0], o[1], o[2], o[3]));
    }
}

template <int CQ> __global__ __launch_bounds__(kThreads) void bn_map_bwd_partial_kernel(const float* __restrict__ x, const float* __restrict__ y,
                                                                                         const float* __restrict__ dy, const float* __restrict__ mean,
                                                                                         int rows, int cols, int per, float hi,
                                                                                         double* __restrict__ part) {
    const Strip s = strip_of<CQ>(rows, cols, per);
    double a[4] = {0.0, 0.0, 0.0, 0.0}, b[4] = {0.0, 0.0, 0.0, 0.0};
    if (s.c < cols) {
        const float4 m4 = col4(mean, s.c);
        const double m[4] = {m4.x, m4.y, m4.z, m4.w};
#pragma unroll 2
        for (long long r = s.r0 + s.lane; r < s.r1; r += kThreads / CQ) {
            const float4 v4 = ld4(x, r, cols, s.c), d4 = ld4(dy, r, cols, s.c);
            const float4 y4 = y ? ld4(y, r, cols, s.c) : make_float4(1.f, 1.f, 1.f, 1.f);
            const float v[4] = {v4.x, v4.y, v4.z, v4.w}, d[4] = {d4.x, d4.y, d4.z, d4.w}, yy[4] = {y4.x, y4.y, y4.z, y4.w};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const double gd = yy[j] > 0.f && yy[j] < hi ? d[j] : 0.f;
                a[j] += gd;
                b[j] += gd * ((double)v[j] - m[j]);
            }
        }
    }
    strip_store_partials<CQ>(a, b, cols, part);
}

__global__ __launch_bounds__(kThreads) void bn_map_bwd_final_kernel(const double* __restrict__ part, const float* __restrict__ invstd, int cols, int slices,
                                                                     float* __restrict__ dgamma, float* __restrict__ dbeta) {
    int c;
    double sb[2], sg[2];
    if (!slice_sum2(part, slices, cols, &c, sb, sg)) return;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        dbeta[c + j] = (float)sb[j];
        dgamma[c + j] = (float)(sg[j] * (double)invstd[c + j]);
    }
}

template <int CQ> __global__ __launch_bounds__(kThreads) void bn_map_bwd_dx_kernel(const float* __restrict__ x, const float* __restrict__ y,
                                                                                    const float* __restrict__ dy, const float* __restrict__ gamma,
                                                                                    const float* __restrict__ mean, const float* __restrict__ invstd,
                                                                                    const float* __restrict__ dgamma, const float* __restrict__ dbeta,
                                                                                    int rows, int cols, int per, float hi, float* __restrict__ dx) {
    const Strip s = strip_of<CQ>(rows, cols, per);
    if (s.c >= cols) return;
    const float4 m4 = col4(mean, s.c), i4 = col4(invstd, s.c), g4 = col4(gamma, s.c), a4 = col4(dgamma, s.c), b4 = col4(dbeta, s.c);
    const float m[4] = {m4.x, m4.y, m4.z, m4.w}, is[4] = {i4.x, i4.y, i4.z, i4.w}, g[4] = {g4.x, g4.y, g4.z, g4.w};
    const float dg[4] = {a4.x, a4.y, a4.z, a4.w}, db[4] = {b4.x, b4.y, b4.z, b4.w};
    const float n = (float)rows;
#pragma unroll 2
    for (long long r = s.r0 + s.lane; r < s.r1; r += kThreads / CQ) {
        const float4 v4 = ld4(x, r, cols, s.c), d4 = ld4(dy, r, cols, s.c);
        const float4 y4 = y ? ld4(y, r, cols, s.c) : make_float4(1.f, 1.f, 1.f, 1.f);
        const float v[4] = {v4.x, v4.y, v4.z, v4.w}, d[4] = {d4.x, d4.y, d4.z, d4.w}, yy[4] = {y4.x, y4.y, y4.z, y4.w};
        float o[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float gd = yy[j] > 0.f && yy[j] < hi ? d[j] : 0.f;
            const float xh = (v[j] - m[j]) * is[j];
            o[j] = g[j] * is[j] / n * (n * gd - db[j] - xh * dg[j]);
        }
        st4(dx, r, cols, s.c, make_float4(o[0], o[1], o[2], o[3]));
    }
}

// The workspace of both calls, written once: the slice partials of two statistics per column, in double.
size_t bn_map_layout(void* ws, int cols, double** part) {
    AdafCarver c(ws);
    *part = c.take<double>(2 * (size_t)bn_map_slices(cols) * cols, 16);
    return c.off;
}

struct Launch {
    dim3 grid;
    int slices, per;
    bool wide;
};
Launch launch_of(int rows, int cols) {
    Launch l;
    l.slices = bn_map_slices(cols);
    l.per = (rows + l.slices - 1) / l.slices;
    l.grid = dim3(bn_map_col_blocks(cols), l.slices);
    l.wide = bn_map_cq(cols) == 64;
    return l;
}
// one strip-walk launch in the column-chunk width of the map
#define BN_MAP_STRIP(kernel, l, st, ...)                                                              \
    do {                                                                                              \
        if ((l).wide) hipLaunchKernelGGL(kernel<64>, (l).grid, dim3(kThreads), 0, st, __VA_ARGS__);   \
        else hipLaunchKernelGGL(kernel<16>, (l).grid, dim3(kThreads), 0, st, __VA_ARGS__);            \
    } while (0)

// the checks both calls share: extents, the 16-byte accesses of the maps, the workspace
int bn_map_check(adaf_handle* h, const char* who, int rows, int cols, const void* const* maps, int nmaps, void* ws, size_t ws_bytes, double** part) {
    if (rows <= 0 || cols <= 0) return adaf_fail(h, ADAF_E_BADARG, "%s: non-positive extent", who);
    if (rows < 2) return adaf_fail(h, ADAF_E_BADARG, "%s: more than one value per channel expected", who);
    if (cols % 4 != 0) return adaf_fail(h, ADAF_E_LAYOUT, "%s: cols %d is not a multiple of 4 (16-byte accesses)", who, cols);
    for (int i = 0; i < nmaps; ++i)
        if (maps[i] && !adaf_aligned16(maps[i])) return adaf_fail(h, ADAF_E_LAYOUT, "%s: a map is not 16-byte aligned", who);
    return adaf_check_ws(h, who, ws, ws_bytes, bn_map_layout(ws, cols, part), ADAF_WS_ALIGN_FIRST);
}

constexpr float kNoCeiling = __builtin_inff();      // the clip ceiling of ReLU: fminf(t, inf) and y < inf change nothing on a finite map

// relu: clip to [0, hi]
int bn_map_forward(adaf_handle* h, const char* who, const float* x, int rows, int cols, const float* gamma, const float* beta, float eps,
                   float momentum, float* running_mean, float* running_var, const float* residual, int relu, float hi, float* y_out,
                   float* mean_out, float* invstd_out, void* ws, size_t ws_bytes, void* stream) {
    if (!x || !gamma || !beta || !y_out || !mean_out || !invstd_out || !ws) return adaf_fail(h, ADAF_E_BADARG, "%s: null pointer", who);
    double* part;
    const void* maps[3] = {x, residual, y_out};
    int rc = bn_map_check(h, who, rows, cols, maps, 3, ws, ws_bytes, &part);
    if (rc) return rc;
    const hipStream_t st = (hipStream_t)stream;
    const Launch l = launch_of(rows, cols);
    BN_MAP_STRIP(bn_map_stat_partial_kernel, l, st, x, rows, cols, l.per, part);
    hipLaunchKernelGGL(bn_map_stat_final_kernel, dim3((cols + 15) / 16), dim3(kThreads), 0, st, (const double*)part, x, rows, cols, l.slices, eps,
                       momentum, mean_out, invstd_out, running_mean, running_var);
    BN_MAP_STRIP(bn_map_normalize_kernel, l, st, x, (const float*)mean_out, (const float*)invstd_out, gamma, beta, residual, rows, cols, l.per,
                 relu, hi, y_out);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? ADAF_OK : adaf_hip_fail(h, e, who);
}

// y == nullptr: no mask; else dy passes where 0 < y < hi
int bn_map_backward(adaf_handle* h, const char* who, const float* x, const float* y, float hi, const float* dy, int rows, int cols,
                    const float* gamma, const float* mean, const float* invstd, float* dx_out, float* dgamma_out, float* dbeta_out, void* ws,
                    size_t ws_bytes, void* stream) {
    if (!x || !dy || !gamma || !mean || !invstd || !dx_out || !dgamma_out || !dbeta_out || !ws) return adaf_fail(h, ADAF_E_BADARG, "%s: null pointer", who);
    double* part;
    const void* maps[4] = {x, y, dy, dx_out};
    int rc = bn_map_check(h, who, rows, cols, maps, 4, ws, ws_bytes, &part);
    if (rc) return rc;
    const hipStream_t st = (hipStream_t)stream;
    const Launch l = launch_of(rows, cols);
    BN_MAP_STRIP(bn_map_bwd_partial_kernel, l, st, x, y, dy, mean, rows, cols, l.per, hi, part);
    hipLaunchKernelGGL(bn_map_bwd_final_kernel, dim3((cols + 15) / 16), dim3(kThreads), 0, st, (const double*)part, invstd, cols, l.slices, dgamma_out,
                       dbeta_out);
    BN_MAP_STRIP(bn_map_bwd_dx_kernel, l, st, x, y, dy, gamma, mean, invstd, (const float*)dgamma_out, (const float*)dbeta_out, rows, cols, l.per,
                 hi, dx_out);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? ADAF_OK : adaf_hip_fail(h, e, who);
}

}  // namespace

size_t adaf_bn_map_workspace_bytes(int rows, int cols) {
    double* part;
    return (rows <= 0 || cols <= 0 || cols % 4 != 0) ? 0 : bn_map_layout(nullptr, cols, &part);
}

int adaf_bn_map_train_forward_f32(adaf_handle* h, const float* x, int rows, int cols, const float* gamma, const float* beta, float eps,
                                  float momentum, float* running_mean, float* running_var, const float* residual, int relu, float* y_out,
                                  float* mean_out, float* invstd_out, void* ws, size_t ws_bytes, void* stream) {
    return bn_map_forward(h, "bn_map_train_forward", x, rows, cols, gamma, beta, eps, momentum, running_mean, running_var, residual, relu ? 1 : 0,
                          kNoCeiling, y_out, mean_out, invstd_out, ws, ws_bytes, stream);
}

int adaf_bn_map_train_forward_act_f32(adaf_handle* h, const float* x, int rows, int cols, const float* gamma, const float* beta, float eps,
                                      float momentum, float* running_mean, float* running_var, const float* residual, int act, float* y_out,
                                      float* mean_out, float* invstd_out, void* ws, size_t ws_bytes, void* stream) {
    if (act != ADAF_ACT_NONE && act != ADAF_ACT_RELU && act != ADAF_ACT_RELU6)
        return adaf_fail(h, ADAF_E_BADARG, "bn_map_train_forward_act: ADAF_ACT_NONE, ADAF_ACT_RELU or ADAF_ACT_RELU6 expected");
    return bn_map_forward(h, "bn_map_train_forward_act", x, rows, cols, gamma, beta, eps, momentum, running_mean, running_var, residual,
                          act != ADAF_ACT_NONE, act == ADAF_ACT_RELU6 ? 6.f : kNoCeiling, y_out, mean_out, invstd_out, ws, ws_bytes, stream);
}

int adaf_bn_map_train_backward_f32(adaf_handle* h, const float* x, const float* y, const float* dy, int rows, int cols, const float* gamma,
                                   const float* mean, const float* invstd, float* dx_out, float* dgamma_out, float* dbeta_out, void* ws,
                                   size_t ws_bytes, void* stream) {
    return bn_map_backward(h, "bn_map_train_backward", x, y, kNoCeiling, dy, rows, cols, gamma, mean, invstd, dx_out, dgamma_out, dbeta_out, ws,
                           ws_bytes, stream);
}

int adaf_bn_map_train_backward_act_f32(adaf_handle* h, const float* x, const float* y, int act, const float* dy, int rows, int cols,
                                       const float* gamma, const float* mean, const float* invstd, float* dx_out, float* dgamma_out,
                                       float* dbeta_out, void* ws, size_t ws_bytes, void* stream) {
    if (act != ADAF_ACT_NONE && act != ADAF_ACT_RELU && act != ADAF_ACT_RELU6)
        return adaf_fail(h, ADAF_E_BADARG, "bn_map_train_backward_act: ADAF_ACT_NONE, ADAF_ACT_RELU or ADAF_ACT_RELU6 expected");
    if (act != ADAF_ACT_NONE && !y) return adaf_fail(h, ADAF_E_BADARG, "bn_map_train_backward_act: the mask of an activation needs y");
    return bn_map_backward(h, "bn_map_train_backward_act", x, act == ADAF_ACT_NONE ? nullptr : y, act == ADAF_ACT_RELU6 ? 6.f : kNoCeiling, dy, rows,
                           cols, gamma, mean, invstd, dx_out, dgamma_out, dbeta_out, ws, ws_bytes, stream);
}
