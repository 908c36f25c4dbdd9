// What the backward passes share (the GRU classifier's of api.hip + gru_bptt.hip, the PPO encoder's of ppo_train.hip, the trunk
// convolutions' of conv_bwd.hip): the strided fp32 GEMM on the matrix engine, column sums in two forms, the slice sum that ends every
// sliced reduction (the column sums' and the split-K weight gradient's of splitk_wgrad.h), and the row-wise mask / shift.  fp32, no
// atomics: every output element has one writer and every sum a fixed order, so the same inputs give the same bits.
#include "adaf_internal.h"

typedef float f32x16 __attribute__((ext_vector_type(16)));

namespace {

// ---- strided fp32 GEMM on the matrix engine: C[m, n] = (sum_k A(m, k) B(k, n)) (* mul[m, n]) -------------------------------------------
// A(m, k) = A[m * a_m + k * a_k], B(k, n) = B[k * b_k + n * b_n]: the NN, TN and NT forms of one kernel.  128 x 128 tile per block, 4 waves
// of 64 x 64 (2 x 2 accumulators of mfma_f32_32x32x2f32), K in slices of 16 through LDS.  Each output is one chain in ascending k:
// deterministic, no atomics.
struct GemmArgs {
    const float* A; long long a_m, a_k;
    const float* B; long long b_k, b_n;
    float* C; int ldc;
    const float* mul; int ldm;
    int M, N, K;
};

constexpr int GT = 128, GK = 16;

__global__ __launch_bounds__(256) void bptt_gemm_kernel(const GemmArgs g) {
    __shared__ float As[GK][GT + 4];
    __shared__ float Bs[GK][GT + 4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, half = lane >> 5, nl = lane & 31;
    const int m0 = blockIdx.y * GT, n0 = blockIdx.x * GT;
    const int wm = (wave & 1) * 64, wn = (wave >> 1) * 64;
    const bool a_kc = g.a_k == 1, b_nc = g.b_n == 1;
    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
    for (int k0 = 0; k0 < g.K; k0 += GK) {
#pragma unroll
        for (int i = 0; i < GT * GK / 256; ++i) {
            const int e = tid + 256 * i;
            const int m = a_kc ? e / GK : e % GT, k = a_kc ? e % GK : e / GT;
            const int gm = m0 + m, gk = k0 + k;
            As[k][m] = (gm < g.M && gk < g.K) ? g.A[(long long)gm * g.a_m + (long long)gk * g.a_k] : 0.f;
            const int n = b_nc ? e % GT : e / GK, kb = b_nc ? e / GT : e % GK;
            const int gn = n0 + n, gkb = k0 + kb;
            Bs[kb][n] = (gn < g.N && gkb < g.K) ? g.B[(long long)gkb * g.b_k + (long long)gn * g.b_n] : 0.f;
        }
        __syncthreads();
#pragma unroll
        for (int kk = 0; kk < GK; kk += 2) {
            const float a0 = As[kk + half][wm + nl], a1 = As[kk + half][wm + 32 + nl];
            const float b0 = Bs[kk + half][wn + nl], b1 = Bs[kk + half][wn + 32 + nl];
            acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, acc[0][1], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc[1][1], 0, 0, 0);
        }
        __syncthreads();
    }
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int m = m0 + wm + 32 * i + (r & 3) + 8 * (r >> 2) + 4 * half, n = n0 + wn + 32 * j + nl;
                if (m < g.M && n < g.N) {
                    float v = acc[i][j][r];
                    if (g.mul) v *= g.mul[(size_t)m * g.ldm + n];
                    g.C[(size_t)m * g.ldc + n] = v;
                }
            }
}

// ---- the slice sum: out[i] = part[0][i] + part[1][i] + ... in slice order, one ascending chain from 0 per element ------------------------
__global__ void slice_sum_kernel(const float* part, int slices, size_t n, float* out) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float v = 0.f;
    for (size_t s = 0; s < (size_t)slices; ++s) v += part[s * n + i];
    out[i] = v;
}

// ---- column sums of x [rows, cols] in two deterministic passes: row slices -> partials [slices, cols], then the slice sum ----------------
// One lane per column: 32 slices, thread (c, slice) adds the slice's rows of column c in ascending order; rows of `ld` floats.  For
// matrices with about as many columns as rows (the GRU's and the Linear's bias gradients).
constexpr int kColSlices = 32;
__global__ void colsum_partial_kernel(const float* x, int rows, int cols, int ld, float* part) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x, s = blockIdx.y;
    if (c >= cols) return;
    const int per = (rows + kColSlices - 1) / kColSlices, r0 = s * per, r1 = min(rows, r0 + per);
    float v = 0.f;
    for (int r = r0; r < r1; ++r) v += x[(size_t)r * ld + c];
    part[(size_t)s * cols + c] = v;
}
// Four lanes per column, for a gradient map with up to 10^6 rows and as few as 64 columns, which the 32 slices above walk as 32 blocks:
// about 2048 blocks -- slices by the column count alone (a workspace query knows no row count), 32 at least.  grid (ceil(cols / 64),
// slices), 256 threads: thread (lane, c) adds rows r0 + lane, r0 + lane + 4, ... of column c in ascending order, the four lanes meet as
// (l0 + l1) + (l2 + l3).  Dense rows (of `cols` floats).
inline int colsum4_slices(int cols) {
    const int s = 2048 / ((cols + 63) / 64);
    return s < kColSlices ? kColSlices : s;
}
__global__ __launch_bounds__(256) void conv_colsum_partial_kernel(const float* __restrict__ x, int rows, int cols, int per, float* __restrict__ part) {
    __shared__ float red[4][64];
    const int cl = threadIdx.x & 63, lane = threadIdx.x >> 6, c = blockIdx.x * 64 + cl;
    const long long r0 = (long long)blockIdx.y * per;
    const long long r1 = r0 + per < rows ? r0 + per : rows;
    float v = 0.f;
    if (c < cols)
        for (long long r = r0 + lane; r < r1; r += 4) v += x[(size_t)r * cols + c];
    red[lane][cl] = v;
    __syncthreads();
    if (lane == 0 && c < cols) part[(size_t)blockIdx.y * cols + c] = (red[0][cl] + red[1][cl]) + (red[2][cl] + red[3][cl]);
}

// out[b, t, :] = x[b, t, :] * mask[b, t, :]  (mask == nullptr: a copy);  shift > 0: out[b, t] = x[b, t - 1], out[b, 0] = 0
__global__ void rows_scale_kernel(const float* x, const float* mask, float* out, size_t n, int steps, int width, int shift) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    if (shift) {
        const size_t row = i / width;
        out[i] = row % steps == 0 ? 0.f : x[i - width];
    } else {
        out[i] = mask ? x[i] * mask[i] : x[i];
    }
}

}  // namespace

void adaf_launch_gemm_strided(const float* A, long long a_m, long long a_k, const float* B, long long b_k, long long b_n, float* C, int ldc,
                              const float* mul, int ldm, int M, int N, int K, hipStream_t s) {
    GemmArgs g{A, a_m, a_k, B, b_k, b_n, C, ldc, mul, ldm, M, N, K};
    hipLaunchKernelGGL(bptt_gemm_kernel, dim3((N + GT - 1) / GT, (M + GT - 1) / GT), dim3(256), 0, s, g);
}

void adaf_launch_slice_sum(const float* part, int slices, size_t n, float* out, hipStream_t s) {
    hipLaunchKernelGGL(slice_sum_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, part, slices, n, out);
}

size_t adaf_colsum_partial_floats(int cols, int lanes) { return (size_t)(lanes == 4 ? colsum4_slices(cols) : kColSlices) * cols; }

void adaf_launch_colsum(const float* x, int rows, int cols, int ld, int lanes, float* part, float* out, hipStream_t s) {
    int slices = kColSlices;
    if (lanes == 4) {
        slices = colsum4_slices(cols);
        hipLaunchKernelGGL(conv_colsum_partial_kernel, dim3((cols + 63) / 64, slices), dim3(256), 0, s, x, rows, cols, (rows + slices - 1) / slices, part);
    } else {
        hipLaunchKernelGGL(colsum_partial_kernel, dim3((cols + 255) / 256, kColSlices), dim3(256), 0, s, x, rows, cols, ld, part);
    }
    adaf_launch_slice_sum(part, slices, (size_t)cols, out, s);
}

void adaf_launch_rows_scale(const float* x, const float* mask, float* out, int rows, int width, int steps, bool shift, hipStream_t s) {
    const size_t n = (size_t)rows * width;
    hipLaunchKernelGGL(rows_scale_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, x, mask, out, n, steps, width, shift ? 1 : 0);
}
