// Backward of the GRU classifier (ACT/models/gfv_net.py:427-435) for stage-3 training: the T-sequential part as ONE persistent kernel,
// the mirror of gru_scan.hip's forward.  (The GEMMs and column sums of the weight gradients: train_common.hip.)
//
// PyTorch's GRU, per step:  r = s(gi_r + gh_r), z = s(gi_z + gh_z), n = tanh(gi_n + r * gh_n), h_t = (1 - z) n + z h_{t-1}
// with gi = W_ih x + b_ih (kept from the training forward) and gh = W_hh h_{t-1} + b_hh (recomputed by one engine GEMM over the stored
// states).  Walking t = T-1 .. 0 with dh = dY_t + carry:
//   dn = dh (1 - z), dz = dh (h_{t-1} - n), da_n = dn (1 - n^2), da_r = da_n gh_n r (1 - r), da_z = dz z (1 - z)
//   dgi_t = [da_r, da_z, da_n],  dgh_t = [da_r, da_z, da_n r],  carry_{t-1} = z dh + dgh_t . W_hh      ((B x 3H) . (3H x H))
//
//   grid  = H / 8 blocks; block j owns hidden units [8j, 8j+8): the gate math of its 8 units for every clip, and the 8 columns of the
//           carry product.  W_hh[:, 8j:8j+8] (3H x 8 = 96 KB at H = 1024) is staged in LDS once for the whole scan.
//   step  : (product of step t+1, then the gate math of step t) -- wave w sums its quarter of the 3H gate rows for 64 clips (lane = clip)
//           with FMAs in ascending k, the four partial sums meet in LDS and are added as (p0 + p1) + (p2 + p3).  The launch-per-step form
//           runs the SAME device code with W_hh read from global memory, one launch per step: same bits.
//   sync  : one grid-wide barrier per step (the product needs every block's dgh_{t+1}); the flat-counter form of gru_scan.hip with its
//           bounded spin: a block that times out bumps the time-out counter and NaN-poisons the gate gradients it still owes, so every
//           weight gradient comes out NaN instead of the device hanging.
#include "adaf_internal.h"

typedef float f32x4 __attribute__((ext_vector_type(4)));

namespace {

__device__ __forceinline__ float sigm(float v) { return 1.f / (1.f + expf(-v)); }

struct BpttArgs {
    const float* dy;     // [B, T, H] gradient of the GRU outputs (after the FC and dropout backward)
    const float* gi;     // [B, T, 3H] input projections (+ b_ih) of the forward
    const float* gh;     // [B, T, 3H] W_hh h_t + b_hh (row (b, t-1) is step t's hidden projection)
    const float* bhh;    // [3H] (step 0's hidden projection: h_{-1} = 0)
    const float* hs;     // [B, T, H]
    const float* whh;    // [3H, H]
    float* dgi;          // [B, T, 3H]
    float* dgh;          // [B, T, 3H]
    float* carry;        // [B, H] z dh + dgh . W_hh of the step above
    unsigned* bar;       // >= T zeroed counters (persistent form)
    unsigned* timeouts;  // device counter (or nullptr)
    int B, T, H;
};

constexpr int kJB = 8;       // hidden units per block

// carry[b, j0 + u] += sum_k dgh[b, t, k] W_hh[k, j0 + u] for every clip: wave w walks k in [w * 3H / 4, (w + 1) * 3H / 4), lane = clip.
// `w` points at W_hh[0, j0] with a row pitch of `ldw` floats (LDS slice: 8, global W_hh: H).
__device__ __forceinline__ void bptt_product(const BpttArgs& a, int t, int j0, const float* w, int ldw, float (*red)[64][kJB]) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int H3 = 3 * a.H, KP = H3 / 4;
    for (int b0 = 0; b0 < a.B; b0 += 64) {
        const int rows = a.B - b0 < 64 ? a.B - b0 : 64;
        float acc[kJB];
#pragma unroll
        for (int u = 0; u < kJB; ++u) acc[u] = 0.f;
        if (lane < rows) {
            const float* drow = a.dgh + ((size_t)(b0 + lane) * a.T + t) * H3 + wave * KP;
            const float* wk = w + (size_t)wave * KP * ldw;
            for (int k = 0; k < KP; k += 4) {
                const f32x4 d = *reinterpret_cast<const f32x4*>(drow + k);
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const float* wr = wk + (size_t)(k + q) * ldw;
#pragma unroll
                    for (int u = 0; u < kJB; ++u) acc[u] = fmaf(d[q], wr[u], acc[u]);
                }
            }
        }
#pragma unroll
        for (int u = 0; u < kJB; ++u) red[wave][lane][u] = acc[u];
        __syncthreads();
        for (int idx = tid; idx < rows * kJB; idx += 256) {
            const int bl = idx / kJB, u = idx - bl * kJB;
            float* c = a.carry + (size_t)(b0 + bl) * a.H + j0 + u;
            *c = *c + ((red[0][bl][u] + red[1][bl][u]) + (red[2][bl][u] + red[3][bl][u]));
        }
        __syncthreads();
    }
}

// gate gradients of step t for the block's units; leaves z dh in `carry` for the product of the next (earlier) step
__device__ __forceinline__ void bptt_gates(const BpttArgs& a, int t, int j0) {
    const int H = a.H, H3 = 3 * H;
    for (int idx = threadIdx.x; idx < a.B * kJB; idx += 256) {
        const int b = idx / kJB, j = j0 + idx - b * kJB;
        const size_t row = (size_t)b * a.T + t;
        float* c = a.carry + (size_t)b * H + j;
        const float dh = a.dy[row * H + j] + (t + 1 < a.T ? *c : 0.f);
        const float* gir = a.gi + row * H3 + j;
        const float* ghr = t > 0 ? a.gh + (row - 1) * H3 + j : a.bhh + j;
        const float hp = t > 0 ? a.hs[(row - 1) * H + j] : 0.f;
        const float ghn = ghr[2 * H];
        const float r = sigm(gir[0] + ghr[0]);
        const float z = sigm(gir[H] + ghr[H]);
        const float n = tanhf(gir[2 * H] + r * ghn);
        const float dan = dh * (1.f - z) * (1.f - n * n);
        const float dar = dan * ghn * r * (1.f - r);
        const float daz = dh * (hp - n) * z * (1.f - z);
        float* dgi = a.dgi + row * H3 + j;
        float* dgh = a.dgh + row * H3 + j;
        dgi[0] = dar; dgi[H] = daz; dgi[2 * H] = dan;
        dgh[0] = dar; dgh[H] = daz; dgh[2 * H] = dan * r;
        *c = dh * z;
    }
}

// the persistent scan (H = 1024): every step in one launch, W_hh's column slice in LDS
__global__ __launch_bounds__(256) void gru_bptt_scan_kernel(const BpttArgs a) {
    constexpr int H = 1024, H3 = 3 * H;
    __shared__ float wsl[H3 * kJB];
    __shared__ float red[4][64][kJB];
    __shared__ int timed_out;
    const int tid = threadIdx.x, j0 = blockIdx.x * kJB;
    if (tid == 0) timed_out = 0;
    for (int i = tid; i < H3 * 2; i += 256) {   // row k of the slice = W_hh[k, j0 .. j0 + 8): two float4 per row
        const int k = i >> 1, q = i & 1;
        *reinterpret_cast<f32x4*>(wsl + k * kJB + 4 * q) = *reinterpret_cast<const f32x4*>(a.whh + (size_t)k * H + j0 + 4 * q);
    }
    __syncthreads();
    for (int t = a.T - 1; t >= 0; --t) {
        if (t + 1 < a.T) {
            __syncthreads();
            if (tid == 0) {   // release (this block's dgh_{t+1} device-wide) -> arrive -> relaxed poll -> acquire, as gru_scan.hip
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                unsigned* bar = a.bar + (a.T - 2 - t);
                unsigned spins = 0;
                __hip_atomic_fetch_add(bar, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                while (__hip_atomic_load(bar, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < gridDim.x) {
                    __builtin_amdgcn_s_sleep(1);
                    if (++spins > (1u << 24)) { timed_out = 1; break; }
                }
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
            }
            __syncthreads();
            if (timed_out) {   // never observed; refuses to hang the device if the grid cannot become co-resident
                if (tid == 0 && a.timeouts) atomicAdd(a.timeouts, 1u);
                const float nan = __builtin_nanf("");
                for (int idx = tid; idx < a.B * kJB; idx += 256) {
                    const int b = idx / kJB, j = j0 + idx - b * kJB;
                    for (int tt = 0; tt <= t; ++tt) {
                        const size_t row = ((size_t)b * a.T + tt) * H3 + j;
                        a.dgi[row] = nan; a.dgi[row + H] = nan; a.dgi[row + 2 * H] = nan;
                        a.dgh[row] = nan; a.dgh[row + H] = nan; a.dgh[row + 2 * H] = nan;
                    }
                }
                return;
            }
            bptt_product(a, t + 1, j0, wsl, kJB, red);
        }
        bptt_gates(a, t, j0);
    }
}

// launch-per-step form (any H % 16 == 0, and stream capture): the product of step t+1 (written by the previous launch), then step t
__global__ __launch_bounds__(256) void gru_bptt_step_kernel(const BpttArgs a, int t) {
    __shared__ float red[4][64][kJB];
    const int j0 = blockIdx.x * kJB;
    if (t + 1 < a.T) bptt_product(a, t + 1, j0, a.whh + j0, a.H, red);
    bptt_gates(a, t, j0);
}

__global__ void bptt_zero_words_kernel(unsigned* p, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) __hip_atomic_store(p + i, 0u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
}

}  // namespace

int adaf_gru_bptt_blocks_per_cu() {
    int nb = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, gru_bptt_scan_kernel, 256, 0) != hipSuccess) {
        (void)hipGetLastError();
        return 0;
    }
    return nb;
}

bool adaf_gru_bptt_persistent_ok(int batch, int hidden, int resident_blocks) {
    return hidden == 1024 && batch >= 1 && batch <= 256 && resident_blocks >= hidden / kJB;
}

hipError_t adaf_launch_gru_bptt(const float* dy, const float* gi, const float* gh, const float* bhh, const float* hs, const float* whh,
                                float* dgi, float* dgh, float* carry, unsigned* bar, unsigned* timeouts, int batch, int steps, int hidden,
                                bool persistent, bool cooperative, hipStream_t s) {
    BpttArgs a;
    a.dy = dy; a.gi = gi; a.gh = gh; a.bhh = bhh; a.hs = hs; a.whh = whh; a.dgi = dgi; a.dgh = dgh; a.carry = carry;
    a.bar = bar; a.timeouts = timeouts; a.B = batch; a.T = steps; a.H = hidden;
    const dim3 grid(hidden / kJB);
    if (persistent) {
        const int nz = steps;
        hipLaunchKernelGGL(bptt_zero_words_kernel, dim3((nz + 63) / 64), dim3(64), 0, s, bar, nz);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
        if (cooperative) {
            void* params[] = {&a};
            return hipLaunchCooperativeKernel(reinterpret_cast<const void*>(gru_bptt_scan_kernel), grid, dim3(256), params, 0, s);
        }
        hipLaunchKernelGGL(gru_bptt_scan_kernel, grid, dim3(256), 0, s, a);
        return hipGetLastError();
    }
    for (int t = steps - 1; t >= 0; --t) {
        hipLaunchKernelGGL(gru_bptt_step_kernel, grid, dim3(256), 0, s, a, t);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}
