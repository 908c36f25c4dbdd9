// The split-K weight gradient of the training kernels: G[m, k] = sum over pixels of a[pixel, m] b[pixel, k], a TN GEMM whose
// reduction axis is the pixel axis, as ONE kernel for the PPO encoder's 1x1 conv (ppo_train.hip) and the trunk's convolutions
// (conv_bwd.hip).  The callers differ in where a lane's operands come from; that is an operand source (below), everything else is here once.
//
// grid (ceil(K / (128 NQ)), ceil(M / (32 MH)), slices), 512 threads.  A block owns pixels [slice * pps, (slice + 1) * pps), rows [32 MH blockIdx.y,
// ...) and columns [128 NQ blockIdx.x, ...).  Its pixels go to its 8 waves in groups of 8 (group g to wave g % 8, ascending); a wave walks its
// groups with v_mfma_f32_32x32x2_f32 products: M = 32 rows, N = 32 lanes x 4 columns of a 16-byte load (MFMA q takes component q: output
// column nl of accumulator 4 (mh NQ + j) + q is column 128 j + 4 nl + q of the block's chunk), K = 2 pixels per product (lane half = pixel
// parity).  MH sets of 32 rows (row 32 mh + m is row m of the accumulators of set mh) are fed by the same B fragments.  Wave 0 writes the
// block's partial into part[slice] ([slices, M, K]); adaf_launch_slice_sum adds the slices in slice order.  No atomics.
// THE ROW BOUND: M need not fill the last block's rows.  A row >= M takes a zero row operand from a clamped address (row M - 1) and is
// not stored; where M is a multiple of 32 MH the clamp and the bound never act.
#pragma once
#include <hip/hip_runtime.h>

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

namespace {

constexpr int kSkThreads = 512, kSkWaves = 8, kSkU = 4;      // kSkU pixel pairs per group

// What one lane holds of one pixel: NQ fragments of 4 consecutive columns and whether they count (a tap in the padding does not), MH
// values of the row operand and the gate of each (the value passes where gate > 0; an ungated source sets 1)
template <int NQ, int MH>
struct SkFrag {
    f32x4 b[NQ];
    float d[MH], gate[MH];
    bool okb;
};

// ---- operand sources ----------------------------------------------------------------------------------------------------------------------
// A source is passed to the kernel by value.  lane(kc) is what the lane keeps of its first column kc (clamped to a real column);
// load(lane, pc, m, frag) requests the lane's operands of pixel pc (clamped into the slice) and row m (+ 32 mh, clamped below M).  Requests only: the
// masks are applied by the kernel at product time, so nothing in load waits for memory.
//
// Pointwise: b[pixel, k] = x[pixel * K + k], the PPO encoder's states and a 1x1 stride-1 convolution (the window of output pixel p is input
// pixel p).  GATED: the row operand passes where e1 > 0, the ReLU mask of the conv output applied on the way in; else e1 is not read
// (a gradient that has its mask already, after a BatchNorm backward).  NQ = 2 needs K % 256 == 0.
template <bool GATED>
struct SkPointwise {
    const float* x;      // [npix, K]
    const float* g;      // [npix, M]
    const float* e1;     // [npix, M] (GATED)
    int K, M;
    struct Lane { int k; };
    __device__ Lane lane(int kc) const { return {kc}; }
    template <int NQ, int MH>
    __device__ void load(const Lane& ln, int pc, int m, SkFrag<NQ, MH>& f) const {
        const float* xp = x + (size_t)pc * K + ln.k;
#pragma unroll
        for (int j = 0; j < NQ; ++j) f.b[j] = *reinterpret_cast<const f32x4*>(xp + 128 * j);
#pragma unroll
        for (int mh = 0; mh < MH; ++mh) {
            const int mc = min(m + 32 * mh, M - 1);
            f.d[mh] = g[(size_t)pc * M + mc];
            f.gate[mh] = GATED ? e1[(size_t)pc * M + mc] : 1.f;
        }
        f.okb = true;
    }
};

// Window: the implicit im2col of a convolution, K = the filter's flattened (kh, kw, i) axis.  cin % 4 == 0, so a lane's 4 columns are 4
// channels of ONE tap (kh, kw), and its window position per pixel is (oy s + kh - p, ox s + kw - p): range-checked, a padding tap multiplies
// zeros (the address is clamped into the map, the fragment does not count)
struct SkWindow {
    const float* x;      // [n, H, W, cin]
    const float* g;      // [n, OH, OW, M]
    int cin, M, H, W, OH, OW, KW, stride, pad;
    struct Lane { int kh, kw, ci; };
    __device__ Lane lane(int kc) const {
        const int tap = kc / cin, kh = tap / KW;
        return {kh, tap - kh * KW, kc - tap * cin};
    }
    template <int MH>
    __device__ void load(const Lane& ln, int pc, int m, SkFrag<1, MH>& f) const {
        const int ohw = OH * OW, img = pc / ohw, r = pc - img * ohw, oy = r / OW, ox = r - oy * OW;
        const int iy = oy * stride + ln.kh - pad, ix = ox * stride + ln.kw - pad;
        const int iyc = min(max(iy, 0), H - 1), ixc = min(max(ix, 0), W - 1);
        f.b[0] = *reinterpret_cast<const f32x4*>(x + (((size_t)img * H + iyc) * W + ixc) * cin + ln.ci);
#pragma unroll
        for (int mh = 0; mh < MH; ++mh) {
            f.d[mh] = g[(size_t)pc * M + min(m + 32 * mh, M - 1)];
            f.gate[mh] = 1.f;
        }
        f.okb = iy >= 0 && iy < H && ix >= 0 && ix < W;
    }
};

// ---- the kernel ---------------------------------------------------------------------------------------------------------------------------
// Property (2) of DESIGN 3 (a returning load is not interlocked against an MFMA that still reads or writes its landing register): a group's
// loads are requested behind a VALU read (an add into `fence`) of the youngest MFMA result of the group before -- every product that read
// the landing registers has retired by then --, pinned by scheduling barriers.  The latency of a group's loads is covered by the block's
// other seven waves.
template <int NQ, int MH, class Src>
__global__ __launch_bounds__(kSkThreads) void splitk_wgrad_kernel(const Src src, float* __restrict__ part, int npix, int K, int M, int pps) {
    constexpr int NA = 4 * NQ * MH;
    __shared__ float red[2][NA * 16 * 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, half = lane >> 5, nl = lane & 31;
    const int kc = blockIdx.x * 128 * NQ + 4 * nl;            // this lane's first column
    const bool kok = kc < K;                                  // (K % 4 == 0: the four columns stand or fall together; a lane past K
    const typename Src::Lane ln = src.lane(kok ? kc : 0);     //  reads column 0 into output columns nobody stores)
    const int m0 = blockIdx.y * 32 * MH;
    const int p0 = blockIdx.z * pps, p1 = min(npix, p0 + pps);
    const int ngroups = (p1 - p0 + 2 * kSkU - 1) / (2 * kSkU);
    f32x16 acc[NA];
#pragma unroll
    for (int q = 0; q < NA; ++q)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[q][r] = 0.f;

    // branch-free: a pixel past the slice reads the slice's last pixel (a cache hit) and takes a zero row operand
    SkFrag<NQ, MH> st[kSkU];
    bool okp[kSkU];
    float fence = 0.f;
    for (int grp = wave; grp < ngroups; grp += kSkWaves) {
#pragma unroll
        for (int u = 0; u < kSkU; ++u) {
            const int pix = p0 + (grp * kSkU + u) * 2 + half;
            src.load(ln, min(pix, p1 - 1), m0 + nl, st[u]);
            okp[u] = pix < p1;
        }
        __builtin_amdgcn_sched_barrier(0);
        // one MFMA per (u, mh, j, q), u ascending: with the ascending group walk, the order of the products inside every accumulator
#pragma unroll
        for (int u = 0; u < kSkU; ++u) {
            f32x4 b[NQ];
#pragma unroll
            for (int j = 0; j < NQ; ++j)
#pragma unroll
                for (int q = 0; q < 4; ++q) b[j][q] = st[u].okb ? st[u].b[j][q] : 0.f;
#pragma unroll
            for (int mh = 0; mh < MH; ++mh) {
                const float a = okp[u] && st[u].gate[mh] > 0.f && m0 + nl + 32 * mh < M ? st[u].d[mh] : 0.f;
#pragma unroll
                for (int j = 0; j < NQ; ++j)
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const int k = 4 * (mh * NQ + j) + q;
                        acc[k] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b[j][q], acc[k], 0, 0, 0);
                    }
            }
        }
#pragma unroll
        for (int q = 0; q < NA; ++q) fence += acc[q][15];      // (every accumulator: the compiler orders the independent chains as it likes)
        __builtin_amdgcn_sched_barrier(0);
    }
    asm volatile("" ::"v"(fence));      // (keeps the fence adds alive; no instruction, the result is untouched)

    // the eight wave partials meet pairwise through two LDS buffers in the fixed order ((w0 + w4) + (w2 + w6)) + ((w1 + w5) + (w3 + w7))
    auto put = [&](int buf) {
#pragma unroll
        for (int q = 0; q < NA; ++q)
#pragma unroll
            for (int r = 0; r < 16; ++r) red[buf][(q * 16 + r) * 64 + lane] = acc[q][r];
    };
    auto add = [&](int buf) {
#pragma unroll
        for (int q = 0; q < NA; ++q)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[q][r] = acc[q][r] + red[buf][(q * 16 + r) * 64 + lane];
    };
    // (writers, readers) per phase: w4, w5 -> w0, w1;  w6, w7 -> w2, w3;  w2, w3 -> w0, w1;  w1 -> w0
    const int wr0[4] = {4, 6, 2, 1}, rd0[4] = {0, 2, 0, 0};
#pragma unroll
    for (int ph = 0; ph < 4; ++ph) {
        const int pairs = ph == 3 ? 1 : 2;
        if (wave >= wr0[ph] && wave < wr0[ph] + pairs) put(wave - wr0[ph]);
        __syncthreads();
        if (wave >= rd0[ph] && wave < rd0[ph] + pairs) add(wave - rd0[ph]);
        __syncthreads();
    }
    if (wave == 0 && kok) {
        float* o = part + (size_t)blockIdx.z * M * K + kc;
#pragma unroll
        for (int mh = 0; mh < MH; ++mh)
#pragma unroll
            for (int j = 0; j < NQ; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int m = (r & 3) + 8 * (r >> 2) + 4 * half, k = 4 * (mh * NQ + j);
                    const f32x4 v = {acc[k][r], acc[k + 1][r], acc[k + 2][r], acc[k + 3][r]};
                    if (m0 + 32 * mh + m < M) *reinterpret_cast<f32x4*>(o + (size_t)(m0 + 32 * mh + m) * K + 128 * j) = v;
                }
    }
}

// ---- the plan -----------------------------------------------------------------------------------------------------------------------------
// Pixel slices of a launch with `tiles` blocks per slice: about one block per CU, at least 64 pixels (one round of the eight waves) per
// slice, an even number of pixels per slice.  Plain arithmetic: the handle-free workspace queries use it.
struct SkPlan { int slices, pps, used; };      // `used` <= slices: the slices that hold pixels (the grid's z extent and the slice sum's count)
inline SkPlan splitk_plan(long long npix, long long tiles, int cus) {
    const long long most = (npix + 63) / 64;
    long long s = cus / (tiles > 0 ? tiles : 1);
    if (s > most) s = most;
    if (s < 1) s = 1;
    SkPlan p;
    p.slices = (int)s;
    p.pps = (int)(((npix + s - 1) / s + 1) / 2 * 2);
    p.used = (int)((npix + p.pps - 1) / p.pps);
    return p;
}
constexpr int kSkCus = 256;     // workspaces are sized for the MI355X's 256 CUs whatever the device reports (never fewer slices than used)

template <int NQ, int MH, class Src>
void splitk_wgrad_launch(const Src& src, float* part, int npix, int K, int M, const SkPlan& pl, hipStream_t st) {
    const dim3 grid((K + 128 * NQ - 1) / (128 * NQ), (M + 32 * MH - 1) / (32 * MH), pl.used);
    hipLaunchKernelGGL((splitk_wgrad_kernel<NQ, MH, Src>), grid, dim3(kSkThreads), 0, st, src, part, npix, K, M, pl.pps);
}

}  // namespace
