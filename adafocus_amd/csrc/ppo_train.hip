// Stage-2 training (ACT/models/ppo.py:84-92,98-122,147-178): what PPO needs around the GRU + Linear forward / backward of gru_bptt.hip.
//
//   ppo_sample_kernel        Categorical(softmax(logits)).sample() from caller-drawn uniforms, its log-probability, the probabilities
//   ppo_sample_actions_kernel  the same sampling for a whole roll-out in one launch: logits in the GRU scan's (B, T) row order, actions and
//                            log-probabilities in the memory's (T, B) order, crop coordinates table[action] in the trunk's (B, T) order
//   ppo_rewards_kernel       confidence = softmax probability of the target class per (clip, step), one wave per clip, and the reward of
//                            main_dist.py:574-581 from it; ppo_ce_last_kernel the mean cross-entropy of the last step
//   ce_steps_*_kernel        stage 1's loss (main_dist.py:479): the cross-entropy of every step's logits against the clip's label, one wave
//                            per row with its gradient in the same pass, then the mean over the B*T rows in row order
//   ppo_returns_kernel       R_t = r_t + gamma R_{t+1}, then (R - mean) / (std + 1e-5) over all T*B entries (unbiased std), one block
//   ppo_head_kernel<Dist>    per row of the stacked head output [actor columns | critic value]: log-probability of the stored action and
//                            entropy under the row's distribution, value, the clipped-surrogate loss terms AND d loss.mean() / d head in
//                            the same pass.  ONE kernel for both policies; Dist = Categorical (log-softmax over A logits, int64 actions)
//                            or Gaussian (see below) says what the actor columns mean
//   ppo_loss_sum_kernel      the scalar loss from the per-row terms, summed in a fixed order
//   launch_wenc_grad         dW_enc [32, C] = (relu-masked dE1)^T S over all T*B*h*w pixels: the state tensor S (257 MB at B = 64, T = 16) is
//                            read ONCE with 16-byte loads by splitk_wgrad_kernel (splitk_wgrad.h) on its pointwise source; a block owns a
//                            pixel slice and a 128- or 256-channel chunk and keeps its 32 x chunk partial in MFMA accumulators; the slice
//                            sum of train_common.hip adds the slices in slice order
//   small layout kernels     (T, B) <-> (B, T) row permutation (with the ReLU mask), the Linear gradient's pixel-major -> nn.Linear permutation
//
// The continuous policy of the Something-Something tree (STH/models/ppo_continuous.py) adds
//   ppo_gauss_sample_kernel  a = 1 - relu(1 - relu(mu + sigma z)) from caller-drawn normals, one rounding per operation, and the
//                            log-probability of the clamped action under N(mu, sigma^2 I)
//   Gaussian                 ppo_head_kernel's distribution for the stacked head [mean logits (2) | value]: sigmoid, Gaussian log-probability
//                            of the stored (y, x), the constant entropy
//   bn_* kernels             BatchNorm with batch statistics over the rows of a [rows, cols] matrix: two-pass column statistics (the mean,
//                            then the squared deviations) as slice partials in row order + a fixed-order sum over the slices (in double), the running
//                            statistics' update, normalise + affine (+ ReLU), and the backward (d gamma, d beta, dx)
//   launch_wenc_grad         also with 64 conv outputs (two 32-row accumulator sets at 128 channels per block) and with a gradient
//                            whose mask is already applied (no E1 operand)
//
// fp32 throughout, no atomics: the same inputs give the same bits.  Every kernel compiles to zero scratch.
#include "adaf_internal.h"
#include "splitk_wgrad.h"

namespace {

// ---- sampling ---------------------------------------------------------------------------------------------------------------------------
// One thread per row (A <= a few dozen): max, sum of exponentials and the running sum all in index order.
// The sampled index is the first a whose running sum exceeds u * total; the last index if rounding leaves none.
__device__ __forceinline__ void ppo_sample_row(const float* l, int A, float u, float* probs, int* pick_out, float* logprob_out) {
    float mx = l[0];
    for (int a = 1; a < A; ++a) mx = fmaxf(mx, l[a]);
    float total = 0.f;
    for (int a = 0; a < A; ++a) total += expf(l[a] - mx);
    const float thr = u * total;
    float run = 0.f;
    int pick = A - 1;
    for (int a = 0; a < A; ++a) {
        const float e = expf(l[a] - mx);
        run += e;
        if (probs) probs[a] = e / total;
        if (run > thr && pick == A - 1) pick = a;
    }
    *pick_out = pick;
    *logprob_out = (l[pick] - mx) - logf(total);
}

// rows = clips of one roll-out step
__global__ void ppo_sample_kernel(const float* logits, int ld, int rows, int A, const float* u, long long* action, float* logprob,
                                  float* probs) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= rows) return;
    int pick;
    float lp;
    ppo_sample_row(logits + (size_t)r * ld, A, u[r], probs ? probs + (size_t)r * A : nullptr, &pick, &lp);
    action[r] = pick;
    logprob[r] = lp;
}

// The whole roll-out: thread i = t * B + b reads logits row b * T + t (the GRU scan's order) and uniform i, writes action / logprob i (the
// memory's order) and the crop coordinates table[action] into row b * T + t (the order the trunk's frame-gathering launch reads)
__global__ void ppo_sample_actions_kernel(const float* logits, int ld, int T, int B, int A, const float* u, const float* table,
                                          long long* action, float* logprob, float* coords) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= T * B) return;
    const int t = i / B, b = i - t * B;
    const size_t row = (size_t)b * T + t;
    int pick;
    float lp;
    ppo_sample_row(logits + row * ld, A, u[i], nullptr, &pick, &lp);
    action[i] = pick;
    logprob[i] = lp;
    if (coords) {
        coords[2 * row] = table[2 * pick];
        coords[2 * row + 1] = table[2 * pick + 1];
    }
}

// ---- rewards ----------------------------------------------------------------------------------------------------------------------------
// max and sum of exp(l - max) of one row of C logits by one wave; every lane gets both.  The sum: lane i adds its columns i, i + 64, ... in
// index order, then six butterfly levels (lane i takes lane i ^ 32's partial, then ^ 16, 8, 4, 2, 1): a fixed tree, the same in every lane
__device__ __forceinline__ void wave_softmax_stats(const float* l, int C, int lane, float* mx_out, float* total_out) {
    float mx = -INFINITY;
    for (int c = lane; c < C; c += 64) mx = fmaxf(mx, l[c]);
    for (int s = 32; s > 0; s >>= 1) mx = fmaxf(mx, __shfl_xor(mx, s, 64));
    float part = 0.f;
    for (int c = lane; c < C; c += 64) part += expf(l[c] - mx);
    for (int s = 32; s > 0; s >>= 1) part = part + __shfl_xor(part, s, 64);
    *mx_out = mx;
    *total_out = part;
}

// grid B, 64 threads: wave b walks its clip's T steps (rows b * T + t).  kind 0: conf_t - conf_{t-1} (conf_{-1} = 0), 1: conf_t,
// 2: conf_t - the baseline's conf_t.  A target outside [0, C) reads nothing and gives NaN
__global__ __launch_bounds__(64) void ppo_rewards_kernel(const float* logits, const float* base, const long long* target, int T, int B, int C,
                                                         int kind, float* rewards, float* conf_out) {
    const int b = blockIdx.x, lane = threadIdx.x;
    const long long tg = target[b];
    const bool ok = tg >= 0 && tg < C;
    float prev = 0.f;
    for (int t = 0; t < T; ++t) {
        const size_t row = (size_t)b * T + t;
        float mx, total;
        wave_softmax_stats(logits + row * C, C, lane, &mx, &total);
        const float conf = ok ? expf(logits[row * C + tg] - mx) / total : NAN;
        float r = conf;
        if (kind == 0) {
            r = conf - prev;
            prev = conf;
        } else if (kind == 2) {
            wave_softmax_stats(base + row * C, C, lane, &mx, &total);
            r = conf - (ok ? expf(base[row * C + tg] - mx) / total : NAN);
        }
        if (lane == 0) {
            rewards[(size_t)t * B + b] = r;
            if (conf_out) conf_out[(size_t)t * B + b] = conf;
        }
    }
}

// mean over clips of the cross-entropy of step T - 1: one block of four waves; wave w takes clips w, w + 4, ... of a chunk of 256 clips,
// thread 0 adds the chunk's values in clip order -- in double: one fp32 chain over B clips drifts by B / 2 roundings of the running sum
// (5.5e-7 of the mean at B = 257, where ATen's own fp32 mean of the same values is 6e-9 from float64; tests/test_heads_domain_gpu.py)
__global__ __launch_bounds__(256) void ppo_ce_last_kernel(const float* logits, const long long* target, int T, int B, int C, float* out) {
    __shared__ float ce[256];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    double sum = 0.0;
    for (int b0 = 0; b0 < B; b0 += 256) {
        const int nb = min(256, B - b0);
        for (int k = wave; k < nb; k += 4) {
            const long long tg = target[b0 + k];
            const float* l = logits + ((size_t)(b0 + k) * T + (T - 1)) * C;
            float mx, total;
            wave_softmax_stats(l, C, lane, &mx, &total);
            if (lane == 0) ce[k] = (tg >= 0 && tg < C) ? logf(total) - (l[tg] - mx) : NAN;
        }
        __syncthreads();
        if (tid == 0)
            for (int k = 0; k < nb; ++k) sum += (double)ce[k];
        __syncthreads();
    }
    if (tid == 0) *out = (float)(sum / (double)B);
}

// ---- the per-step cross-entropy of stage 1 (ACT/main_dist.py:479: every step's logits against the clip's label) ------------------------
// One wave per row r = b * T + t, four rows per block: the row's loss log(sum exp(l - max)) - (l[target[b]] - max) into row_loss[r] and,
// when asked for, d mean-loss / d logits = (exp(l - max) / sum - [c == target]) / rows.  A target outside [0, C) reads nothing out of
// range: the row's loss and its gradient row are NaN
__global__ __launch_bounds__(256) void ce_steps_rows_kernel(const float* logits, const long long* target, long long rows, int T, int C,
                                                            float* row_loss, float* dlogits) {
    const int lane = threadIdx.x & 63;
    const long long r = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= rows) return;
    const long long tg = target[r / T];
    const bool ok = tg >= 0 && tg < C;
    const float* l = logits + (size_t)r * C;
    float mx, total;
    wave_softmax_stats(l, C, lane, &mx, &total);
    if (lane == 0) row_loss[r] = ok ? logf(total) - (l[tg] - mx) : NAN;
    if (dlogits) {
        float* d = dlogits + (size_t)r * C;
        const float n = (float)rows;
        for (int c = lane; c < C; c += 64) d[c] = ok ? (expf(l[c] - mx) / total - (c == tg ? 1.f : 0.f)) / n : NAN;
    }
}

// The mean of the per-row losses, added in row order in double (ppo_ce_last_kernel's comment has the measured reason) by one block: up to
// 256 rows thread 0 adds them all; beyond that thread i first adds its run of ceil(rows / 256) consecutive rows, then thread 0 adds the
// 256 partials in thread order -- two levels, each in row order
__global__ __launch_bounds__(256) void ce_steps_mean_kernel(const float* row_loss, long long rows, float* loss) {
    __shared__ double part[256];
    const int tid = threadIdx.x;
    const long long per = (rows + 255) / 256, r0 = tid * per, r1 = min(rows, r0 + per);
    double s = 0.0;
    for (long long r = r0; r < r1; ++r) s += (double)row_loss[r];
    part[tid] = s;
    __syncthreads();
    if (tid == 0) {
        double sum = 0.0;
        for (int i = 0; i < 256; ++i) sum += part[i];
        *loss = (float)(sum / (double)rows);
    }
}

// ---- returns ----------------------------------------------------------------------------------------------------------------------------
// sum of v over the block's 256 threads in a fixed order (a binary tree over thread indices); every thread gets the result
__device__ __forceinline__ float block_sum_256(float v, float* red) {
    const int tid = threadIdx.x;
    red[tid] = v;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (tid < s) red[tid] = red[tid] + red[tid + s];
        __syncthreads();
    }
    const float out = red[0];
    __syncthreads();
    return out;
}

__global__ __launch_bounds__(256) void ppo_returns_kernel(const float* rewards, int T, int B, float gamma, float* out) {
    __shared__ float red[256];
    const int tid = threadIdx.x, n = T * B;
    for (int b = tid; b < B; b += 256) {
        float R = 0.f;
        for (int t = T - 1; t >= 0; --t) {
            R = rewards[(size_t)t * B + b] + gamma * R;
            out[(size_t)t * B + b] = R;
        }
    }
    __syncthreads();
    float s = 0.f;
    for (int i = tid; i < n; i += 256) s += out[i];
    const float mean = block_sum_256(s, red) / (float)n;
    float q = 0.f;
    for (int i = tid; i < n; i += 256) {
        const float d = out[i] - mean;
        q += d * d;
    }
    const float sd = sqrtf(block_sum_256(q, red) / (float)(n - 1));
    const float inv = 1.f / (sd + 1e-5f);
    for (int i = tid; i < n; i += 256) out[i] = (out[i] - mean) * inv;
}

// ---- PPO head ---------------------------------------------------------------------------------------------------------------------------
struct HeadArgs {
    const float* head;        // [T*B, A + 1]: row b * T + t when head_bt, else row t * B + b
    const long long* action;  // [T, B] the stored discrete actions (Categorical only)
    const float* old_logprob; // [T, B] (loss mode)
    const float* returns;     // [T, B] (loss mode)
    const float* g_logprob;   // [T, B] upstream gradients (plain backward mode; any may be null = 0)
    const float* g_value;
    const float* g_entropy;
    float* logprob;           // [T, B] outputs (may be null)
    float* value;
    float* entropy;
    float* terms;             // [2, T*B]: -min(surr1, surr2) - 0.01 entropy, (value - return)^2   (loss mode)
    float* dhead;             // [T*B, A + 1] in the head's row order (may be null)
    int T, B, A, head_bt, mode;   // mode 0: statistics only, 1: PPO loss + its gradient, 2: gradient from g_*
    float eps_clip;
    const float* action_yx;   // [T, B, 2] the stored continuous actions and the policy's standard deviation (Gaussian only; A = 2)
    float sigma;
};

// The tail both loss heads share, from a row's log-probability of its stored action, value and entropy: the two per-row loss terms
// (-min(surr1, surr2) - 0.01 entropy, (value - return)^2) and d loss.mean() / d (logprob, value, entropy).
// autograd through torch.min / torch.clamp: an unclamped ratio carries the whole advantage (half through each equal branch); a clamped
// one carries it only when surr1 wins the min (half of it on an exact tie)
struct PpoTail { float term_pg, term_v, g_lp, g_v, g_ent; };
__device__ __forceinline__ PpoTail ppo_loss_tail(float lp_act, float old_lp, float R, float v, float ent, float eps_clip, int n) {
    PpoTail o;
    const float inv_n = 1.f / (float)n;
    const float ratio = expf(lp_act - old_lp);
    const float adv = R - v;
    const float lo = 1.f - eps_clip, hi = 1.f + eps_clip;
    const float surr1 = ratio * adv, surr2 = fminf(fmaxf(ratio, lo), hi) * adv;
    o.term_pg = -fminf(surr1, surr2) - 0.01f * ent;
    o.term_v = (v - R) * (v - R);
    float g_ratio = adv;
    if (ratio < lo || ratio > hi) g_ratio = surr1 < surr2 ? adv : (surr1 == surr2 ? 0.5f * adv : 0.f);
    o.g_lp = -g_ratio * ratio * inv_n;
    o.g_v = (v - R) * inv_n;            // 0.5 * MSE, a mean over all rows, broadcast into every row's loss
    o.g_ent = -0.01f * inv_n;
    return o;
}

constexpr float kLog2Pi = 1.8378770664093453f;

// log N(a; mu, sigma^2 I) of a two-dimensional action: -1/2 sum(((a - mu) / sigma)^2) - 2 log sigma - log 2 pi
__device__ __forceinline__ float gauss_logprob(float a0, float a1, float mu0, float mu1, float sigma) {
    const float z0 = (a0 - mu0) / sigma, z1 = (a1 - mu1) / sigma;
    return -0.5f * (z0 * z0 + z1 * z1) - 2.f * logf(sigma) - kLog2Pi;
}

// The two distributions of ppo_head_kernel.  Constructed from row i's actor columns l: lp_act = the log-probability of the row's stored
// action, ent = the entropy; pull_back writes d (g_lp * lp_act + g_ent * ent) / d l into the row's actor columns of dhead.
// Categorical(softmax(l[0..A))): max, sum of exponentials and entropy in index order; the pull-back recomputes lp / p per column.
struct Categorical {
    const float* l;
    int A, act;
    float mx, lse, lp_act, ent;
    static __device__ __forceinline__ int columns(const HeadArgs& h) { return h.A; }
    __device__ __forceinline__ Categorical(const HeadArgs& h, const float* row, int i) : l(row), A(h.A) {
        mx = l[0];
        for (int a = 1; a < A; ++a) mx = fmaxf(mx, l[a]);
        float total = 0.f;
        for (int a = 0; a < A; ++a) total += expf(l[a] - mx);
        lse = logf(total);
        ent = 0.f;
        for (int a = 0; a < A; ++a) {
            const float lp = (l[a] - mx) - lse;
            ent -= expf(lp) * lp;
        }
        act = (int)h.action[i];
        lp_act = (l[act] - mx) - lse;
    }
    __device__ __forceinline__ void pull_back(float g_lp, float g_ent, float* d) const {
        for (int a = 0; a < A; ++a) {
            const float lp = (l[a] - mx) - lse, p = expf(lp);
            d[a] = g_lp * ((a == act ? 1.f : 0.f) - p) - g_ent * p * (lp + ent);
        }
    }
};

// N(mu, sigma^2 I) over (y, x) for head rows [mean logit y, mean logit x, value] and stored actions [T, B, 2]: mu = sigmoid(logit) (the
// engine's 1 / (1 + exp(-v))), the entropy is the constant 1 + log 2 pi + 2 log sigma (no gradient: g_ent is not read),
// d logprob / d logit_k = (a_k - mu_k) / sigma^2 * mu_k (1 - mu_k)
struct Gaussian {
    float a0, a1, mu0, mu1, sigma, lp_act, ent;
    static __device__ __forceinline__ int columns(const HeadArgs&) { return 2; }
    __device__ __forceinline__ Gaussian(const HeadArgs& h, const float* l, int i) : sigma(h.sigma) {
        a0 = h.action_yx[2 * (size_t)i];
        a1 = h.action_yx[2 * (size_t)i + 1];
        mu0 = 1.f / (1.f + expf(-l[0]));
        mu1 = 1.f / (1.f + expf(-l[1]));
        lp_act = gauss_logprob(a0, a1, mu0, mu1, h.sigma);
        ent = 1.f + kLog2Pi + 2.f * logf(h.sigma);
    }
    __device__ __forceinline__ void pull_back(float g_lp, float, float* d) const {
        const float inv_var = 1.f / (sigma * sigma);
        d[0] = g_lp * ((a0 - mu0) * inv_var) * (mu0 * (1.f - mu0));
        d[1] = g_lp * ((a1 - mu1) * inv_var) * (mu1 * (1.f - mu1));
    }
};

// One thread per row; the value is the column behind the distribution's
template <class Dist>
__global__ void ppo_head_kernel(const HeadArgs h) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x, n = h.T * h.B;
    if (i >= n) return;
    const int t = i / h.B, b = i - t * h.B, A = Dist::columns(h);
    const size_t hrow = (size_t)(h.head_bt ? b * h.T + t : i) * (A + 1);
    const float* l = h.head + hrow;
    const Dist dist(h, l, i);
    const float lp_act = dist.lp_act, ent = dist.ent, v = l[A];
    if (h.logprob) h.logprob[i] = lp_act;
    if (h.value) h.value[i] = v;
    if (h.entropy) h.entropy[i] = ent;
    if (h.mode == 0) return;
    float g_lp, g_v, g_ent;
    if (h.mode == 1) {
        const PpoTail tl = ppo_loss_tail(lp_act, h.old_logprob[i], h.returns[i], v, ent, h.eps_clip, n);
        h.terms[i] = tl.term_pg;
        h.terms[n + i] = tl.term_v;
        g_lp = tl.g_lp;
        g_v = tl.g_v;
        g_ent = tl.g_ent;
    } else {
        g_lp = h.g_logprob ? h.g_logprob[i] : 0.f;
        g_v = h.g_value ? h.g_value[i] : 0.f;
        g_ent = h.g_entropy ? h.g_entropy[i] : 0.f;
    }
    if (!h.dhead) return;
    float* d = h.dhead + hrow;
    dist.pull_back(g_lp, g_ent, d);
    d[A] = g_v;
}

// loss.mean() = mean(-min(surr1, surr2) - 0.01 entropy) + 0.5 * mean((value - return)^2): per-thread strided partial sums in index order,
// then the fixed tree of block_sum_256
__global__ __launch_bounds__(256) void ppo_loss_sum_kernel(const float* terms, int n, float* loss) {
    __shared__ float red[256];
    float s = 0.f, q = 0.f;
    for (int i = threadIdx.x; i < n; i += 256) {
        s += terms[i];
        q += terms[n + i];
    }
    const float a = block_sum_256(s, red), m = block_sum_256(q, red);
    if (threadIdx.x == 0) *loss = a / (float)n + 0.5f * (m / (float)n);
}

// ---- the Gaussian policy (continuous actions) -----------------------------------------------------------------------------------------------
// One thread per row.  The action is ppo_continuous.py:98-101 on the sample mu + sigma z with one fp32 rounding per operation, in that
// order, nothing contracted: an interior value carries the torch expression's last bit (and floor(a * (H - P)) follows it)
__global__ void ppo_gauss_sample_kernel(const float* mean, const float* noise, int rows, float sigma, float* action, float* logprob) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= rows) return;
    float a[2];
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const float raw = __fadd_rn(mean[2 * r + k], __fmul_rn(sigma, noise[2 * r + k]));
        a[k] = __fsub_rn(1.f, fmaxf(__fsub_rn(1.f, fmaxf(raw, 0.f)), 0.f));
        action[2 * r + k] = a[k];
    }
    logprob[r] = gauss_logprob(a[0], a[1], mean[2 * r], mean[2 * r + 1], sigma);
}

// ---- BatchNorm with batch statistics over the rows of x [rows, cols] ---------------------------------------------------------------------
// Column sums as kBnSlices partials, each over its rows in ascending order, then added in slice order (adaf_launch_colsum's scheme).  The
// sums are carried in double and rounded once: torch's CPU BatchNorm, the yardstick of the tests, accumulates that way, and the kernels
// are a few microseconds whatever the accumulator.
constexpr int kBnSlices = 32;

// grid (ceil(cols / 64), kBnSlices), 64 threads.  mean == nullptr: part[s, c] = sum x;  else: sum (x - mean[c])^2
__global__ void bn_colstat_partial_kernel(const float* x, const float* mean, int rows, int cols, double* part) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x, s = blockIdx.y;
    if (c >= cols) return;
    const int per = (rows + kBnSlices - 1) / kBnSlices, r0 = s * per, r1 = min(rows, r0 + per);
    double v = 0.0;
    if (mean) {
        const double m = mean[c];
        for (int r = r0; r < r1; ++r) {
            const double d = (double)x[(size_t)r * cols + c] - m;
            v += d * d;
        }
    } else {
        for (int r = r0; r < r1; ++r) v += (double)x[(size_t)r * cols + c];
    }
    part[(size_t)s * cols + c] = v;
}

// pass 0: mean[c];  pass 1: invstd[c] = 1 / sqrt(biased variance + eps) and the running statistics' update (momentum; unbiased variance)
__global__ void bn_stats_final_kernel(const double* part, int rows, int cols, int pass, float eps, float momentum, float* mean, float* invstd,
                                      float* running_mean, float* running_var) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= cols) return;
    double v = 0.0;
    for (int s = 0; s < kBnSlices; ++s) v += part[(size_t)s * cols + c];
    if (pass == 0) {
        mean[c] = (float)(v / (double)rows);
        return;
    }
    invstd[c] = (float)(1.0 / sqrt(v / (double)rows + (double)eps));
    const double m = momentum;
    if (running_mean) running_mean[c] = (float)((1.0 - m) * (double)running_mean[c] + m * (double)mean[c]);
    if (running_var) running_var[c] = (float)((1.0 - m) * (double)running_var[c] + m * (v / (double)(rows - 1)));
}

// y = (x - mean) * invstd * gamma + beta (then ReLU when relu)
__global__ void bn_normalize_kernel(const float* x, const float* mean, const float* invstd, const float* gamma, const float* beta, size_t n,
                                    int cols, int relu, float* y) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int c = (int)(i % cols);
    const float v = (x[i] - mean[c]) * invstd[c] * gamma[c] + beta[c];
    y[i] = relu ? fmaxf(v, 0.f) : v;
}

// part[s, c] = sum dy_m, part[kBnSlices + s, c] = sum dy_m * (x - mean) over the slice's rows; dy_m = dy where y > 0 (y == nullptr: dy as it is)
__global__ void bn_bwd_partial_kernel(const float* x, const float* y, const float* dy, const float* mean, int rows, int cols, double* part) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x, s = blockIdx.y;
    if (c >= cols) return;
    const int per = (rows + kBnSlices - 1) / kBnSlices, r0 = s * per, r1 = min(rows, r0 + per);
    const double m = mean[c];
    double sb = 0.0, sg = 0.0;
    for (int r = r0; r < r1; ++r) {
        const size_t i = (size_t)r * cols + c;
        const double g = (!y || y[i] > 0.f) ? dy[i] : 0.f;
        sb += g;
        sg += g * ((double)x[i] - m);
    }
    part[(size_t)s * cols + c] = sb;
    part[(size_t)(kBnSlices + s) * cols + c] = sg;
}

// d beta = sum dy_m;  d gamma = sum dy_m * xhat = invstd * sum dy_m * (x - mean)
__global__ void bn_bwd_final_kernel(const double* part, const float* invstd, int cols, float* dgamma, float* dbeta) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= cols) return;
    double sb = 0.0, sg = 0.0;
    for (int s = 0; s < kBnSlices; ++s) {
        sb += part[(size_t)s * cols + c];
        sg += part[(size_t)(kBnSlices + s) * cols + c];
    }
    dbeta[c] = (float)sb;
    dgamma[c] = (float)(sg * (double)invstd[c]);
}

// dx = gamma * invstd / n * (n * dy_m - d beta - xhat * d gamma)
__global__ void bn_bwd_dx_kernel(const float* x, const float* y, const float* dy, const float* gamma, const float* mean, const float* invstd,
                                 const float* dgamma, const float* dbeta, size_t n, int rows, int cols, float* dx) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int c = (int)(i % cols);
    const float g = (!y || y[i] > 0.f) ? dy[i] : 0.f;
    const float xh = (x[i] - mean[c]) * invstd[c];
    dx[i] = gamma[c] * invstd[c] / (float)rows * ((float)rows * g - dbeta[c] - xh * dgamma[c]);
}

void launch_bn_forward(const float* x, int rows, int cols, const float* gamma, const float* beta, float eps, float momentum, float* running_mean,
                       float* running_var, int relu, float* y, float* mean, float* invstd, double* part, hipStream_t st) {
    const dim3 gp((cols + 63) / 64, kBnSlices), gc((cols + 63) / 64);
    const size_t n = (size_t)rows * cols;
    hipLaunchKernelGGL(bn_colstat_partial_kernel, gp, dim3(64), 0, st, x, (const float*)nullptr, rows, cols, part);
    hipLaunchKernelGGL(bn_stats_final_kernel, gc, dim3(64), 0, st, part, rows, cols, 0, eps, momentum, mean, invstd, running_mean, running_var);
    hipLaunchKernelGGL(bn_colstat_partial_kernel, gp, dim3(64), 0, st, x, (const float*)mean, rows, cols, part);
    hipLaunchKernelGGL(bn_stats_final_kernel, gc, dim3(64), 0, st, part, rows, cols, 1, eps, momentum, mean, invstd, running_mean, running_var);
    hipLaunchKernelGGL(bn_normalize_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, x, mean, invstd, gamma, beta, n, cols, relu, y);
}

void launch_bn_backward(const float* x, const float* y, const float* dy, int rows, int cols, const float* gamma, const float* mean,
                        const float* invstd, float* dx, float* dgamma, float* dbeta, double* part, hipStream_t st) {
    const size_t n = (size_t)rows * cols;
    hipLaunchKernelGGL(bn_bwd_partial_kernel, dim3((cols + 63) / 64, kBnSlices), dim3(64), 0, st, x, y, dy, mean, rows, cols, part);
    hipLaunchKernelGGL(bn_bwd_final_kernel, dim3((cols + 63) / 64), dim3(64), 0, st, part, invstd, cols, dgamma, dbeta);
    hipLaunchKernelGGL(bn_bwd_dx_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, x, y, dy, gamma, mean, invstd, dgamma, dbeta, n, rows,
                       cols, dx);
}
size_t bn_partial_doubles(int cols) { return 2 * (size_t)kBnSlices * cols; }

// ---- layout kernels ---------------------------------------------------------------------------------------------------------------------
// out[(j * ni + i), :] = in[(i * nj + j), :] (* (gate[(i * nj + j), :] > 0) when gate != nullptr): (T, B) <-> (B, T) rows of `width` floats
__global__ void ppo_rows_transpose_kernel(const float* in, const float* gate, float* out, int ni, int nj, int width) {
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x, n = (size_t)ni * nj * width;
    if (idx >= n) return;
    const size_t orow = idx / width;
    const int c = (int)(idx - orow * width), j = (int)(orow / ni), i = (int)(orow - (size_t)j * ni);
    const size_t src = ((size_t)i * nj + j) * width + c;
    out[idx] = gate ? (gate[src] > 0.f ? in[src] : 0.f) : in[src];
}

// dW_lin in the nn.Linear layout (column c * hw + p) from the engine's pixel-major one (column p * cmid + c)
__global__ void ppo_lin_grad_permute_kernel(const float* pm, float* out, int rows, int hw, int cmid) {
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x, cols = (size_t)hw * cmid;
    if (idx >= rows * cols) return;
    const size_t r = idx / cols;
    const int k = (int)(idx - r * cols), c = k / hw, p = k - c * hw;
    out[idx] = pm[r * cols + (size_t)p * cmid + c];
}

// x * (gate > 0): the masked operand of the single-chain form of the weight gradient
__global__ void ppo_relu_mask_kernel(const float* x, const float* gate, float* out, size_t n) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = gate[i] > 0.f ? x[i] : 0.f;
}

// ---- split-K weight gradient of the 1x1 conv --------------------------------------------------------------------------------------------
// The core of splitk_wgrad.h on its pointwise source: M = the 32 or 64 conv outputs, K = the channels, the ReLU mask of the conv output
// (e1) as the source's gate.  A block takes 256 channels of 32 conv outputs where the channel count allows, else (and always with 64
// outputs, as two 32-row accumulator sets) 128
bool sk_shape_ok(int cin, int cmid) { return (cmid == 32 || cmid == 64) && cin > 0 && cin % 128 == 0; }
bool sk_wide(int cin, int cmid) { return cmid == 32 && cin % 256 == 0; }
SkPlan sk_plan(int npix, int cin, int cmid, int cus) { return splitk_plan(npix, sk_wide(cin, cmid) ? cin / 256 : cin / 128, cus); }

template <bool GATED>
void launch_sk(const SkPointwise<GATED>& src, float* part, int npix, const SkPlan& pl, hipStream_t st) {
    if (src.M == 64)
        splitk_wgrad_launch<1, 2>(src, part, npix, src.K, src.M, pl, st);
    else if (sk_wide(src.K, src.M))
        splitk_wgrad_launch<2, 1>(src, part, npix, src.K, src.M, pl, st);
    else
        splitk_wgrad_launch<1, 1>(src, part, npix, src.K, src.M, pl, st);
}

// e1 == nullptr: de1 has its mask applied already
int launch_wenc_grad(adaf_handle* h, const float* states, const float* de1, const float* e1, int npix, int cin, int cmid, int split_k,
                     float* dw, float* ws, hipStream_t st) {
    if (split_k) {
        if (!sk_shape_ok(cin, cmid)) return adaf_fail(h, ADAF_E_LAYOUT, "ppo_wenc_grad: the split-K form needs 32 or 64 conv outputs and channels %% 128 == 0");
        const SkPlan pl = sk_plan(npix, cin, cmid, h->cus < kSkCus ? h->cus : kSkCus);
        if (e1)
            launch_sk(SkPointwise<true>{states, de1, e1, cin, cmid}, ws, npix, pl, st);
        else
            launch_sk(SkPointwise<false>{states, de1, nullptr, cin, cmid}, ws, npix, pl, st);
        adaf_launch_slice_sum(ws, pl.used, (size_t)cmid * cin, dw, st);
    } else {
        // the single-chain form: the masked gradient as a tensor, then dW[m, c] = sum_i masked[i, m] S[i, c] as one ascending chain per output
        const size_t n = (size_t)npix * cmid;
        if (e1) hipLaunchKernelGGL(ppo_relu_mask_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, de1, e1, ws, n);
        adaf_launch_gemm_strided(e1 ? ws : de1, 1, cmid, states, cin, 1, dw, cin, nullptr, 0, cmid, cin, npix, st);
    }
    return ADAF_OK;
}

size_t wenc_sk_floats(int npix, int cin, int cmid) {
    return sk_shape_ok(cin, cmid) ? (size_t)sk_plan(npix, cin, cmid, kSkCus).slices * cmid * cin : 0;
}

// ---- workspace layouts: each written once, measured by the query (null base) and carved by the call -----------------------------------
size_t ppo_head_layout(void* ws, int steps, int batch, float** terms) {
    AdafCarver c(ws);
    *terms = c.take<float>(2 * (size_t)steps * batch);      // the two per-row loss terms
    return c.off;
}
size_t ce_steps_layout(void* ws, int batch, int steps, float** row_loss) {
    AdafCarver c(ws);
    *row_loss = c.take<float>((size_t)batch * steps);       // the per-row losses
    return c.off;
}
size_t wenc_layout(void* ws, int npix, int cin, int cmid, float** buf) {      // either form of adaf_ppo_wenc_grad_f32: the partials, or the masked gradient
    const size_t sk = wenc_sk_floats(npix, cin, cmid), chain = (size_t)npix * cmid;
    AdafCarver c(ws);
    *buf = c.take<float>(sk > chain ? sk : chain);
    return c.off;
}
// dE [rows, hidden], dE1 [rows, hw * cmid], the pixel-major dW_lin [hidden, hw * cmid], column-sum partials, the split-K slice partials;
// with BatchNorm also the gradients in front of the two BatchNorms (dL [rows, hidden], dC [rows, hw * cmid]) and their column partials
struct EncBackwardWs { float *de, *de1, *dwl, *part, *wws, *dl, *dc; double* bnp; };
size_t enc_backward_layout(void* ws, int steps, int batch, int map_pixels, int channels, int conv_out, int hidden, bool bn, EncBackwardWs* r) {
    const size_t rows = (size_t)steps * batch, mid = (size_t)map_pixels * conv_out;
    AdafCarver c(ws);
    r->de = c.take<float>(rows * hidden);
    r->de1 = c.take<float>(rows * mid);
    r->dwl = c.take<float>((size_t)hidden * mid);
    r->part = c.take<float>(adaf_colsum_partial_floats(hidden, 1));
    r->wws = c.take<float>(wenc_sk_floats((int)(rows * map_pixels), channels, conv_out));
    r->dl = r->dc = nullptr;
    r->bnp = nullptr;
    if (bn) {
        r->dl = c.take<float>(rows * hidden);
        r->dc = c.take<float>(rows * mid);
        r->bnp = c.take<double>(bn_partial_doubles(hidden > conv_out ? hidden : conv_out));
    }
    return c.off;
}
size_t bn_layout(void* ws, int cols, double** part) {
    AdafCarver c(ws);
    *part = c.take<double>(bn_partial_doubles(cols));
    return c.off;
}

// What the state encoder kept and what its backward fills.  The BatchNorm members are null without BatchNorm (then e1 / e_bt are the conv's
// and the Linear's own outputs after ReLU)
struct EncBackwardArgs {
    const float *states, *e1, *e_bt, *dx_bt, *w_lin_pm;
    const float *c1, *gamma1, *mean1, *invstd1;       // BN2d: the raw conv output [rows * hw, cmid] and the statistics it was normalised with
    const float *l1, *gamma2, *mean2, *invstd2;       // BN1d: the raw Linear output [rows, hidden], rows t * B + b
    float *dw_enc, *dw_lin, *db_lin, *dgamma1, *dbeta1, *dgamma2, *dbeta2;
    int steps, batch, map_pixels, channels, conv_out, hidden;
};

int run_encoder_backward(adaf_handle* h, const EncBackwardArgs& a, const EncBackwardWs& r, hipStream_t st) {
    const int rows = a.steps * a.batch, mid = a.map_pixels * a.conv_out, hidden = a.hidden;
    const bool bn = a.c1 != nullptr;
    // dE[t * B + b] = dx[b * T + t] * (E[b * T + t] > 0): the GRU's (B, T) rows back to the states' (T, B) order, ReLU mask on the way
    {
        const size_t n = (size_t)rows * hidden;
        hipLaunchKernelGGL(ppo_rows_transpose_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, a.dx_bt, a.e_bt, r.de, a.batch, a.steps, hidden);
    }
    const float* dl = r.de;      // the gradient of the Linear's own output
    if (bn) {
        launch_bn_backward(a.l1, nullptr, r.de, rows, hidden, a.gamma2, a.mean2, a.invstd2, r.dl, a.dgamma2, a.dbeta2, r.bnp, st);
        dl = r.dl;
    }
    // Linear: dW_lin = dL^T E1 (pixel-major columns, then permuted), db_lin = column sums, dE1 = dL W_lin
    adaf_launch_gemm_strided(dl, 1, hidden, a.e1, mid, 1, r.dwl, mid, nullptr, 0, hidden, mid, rows, st);
    {
        const size_t n = (size_t)hidden * mid;
        hipLaunchKernelGGL(ppo_lin_grad_permute_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, r.dwl, a.dw_lin, hidden, a.map_pixels, a.conv_out);
    }
    adaf_launch_colsum(dl, rows, hidden, hidden, 1, r.part, a.db_lin, st);
    adaf_launch_gemm_strided(dl, hidden, 1, a.w_lin_pm, mid, 1, r.de1, mid, nullptr, 0, rows, mid, hidden, st);
    const int npix = rows * a.map_pixels;
    if (bn) {      // the ReLU mask goes into the BatchNorm backward; the conv's gradient arrives dense
        launch_bn_backward(a.c1, a.e1, r.de1, npix, a.conv_out, a.gamma1, a.mean1, a.invstd1, r.dc, a.dgamma1, a.dbeta1, r.bnp, st);
        return launch_wenc_grad(h, a.states, r.dc, nullptr, npix, a.channels, a.conv_out, 1, a.dw_enc, r.wws, st);
    }
    return launch_wenc_grad(h, a.states, r.de1, a.e1, npix, a.channels, a.conv_out, 1, a.dw_enc, r.wws, st);
}

// Both head exports behind their own null-pointer and extent checks: mode validation, workspace check, the head kernel of the export's
// distribution (action_yx: Gaussian with A = 2, else Categorical over n_actions) and the loss sum.  `name` starts every message.
int run_ppo_head(adaf_handle* h, const char* name, const float* head, int head_batch_major, int steps, int batch, int n_actions,
                 const int64_t* actions, const float* action_yx, float sigma, const float* old_logprobs, const float* returns, float eps_clip,
                 const float* g_logprob, const float* g_value, const float* g_entropy, float* logprobs_out, float* values_out,
                 float* entropy_out, float* loss_out, float* dhead_out, void* ws, size_t ws_bytes, void* stream) {
    const bool loss_mode = old_logprobs || returns || loss_out;
    const bool grad_mode = g_logprob || g_value || g_entropy;
    if (loss_mode && (!old_logprobs || !returns || !loss_out || !ws)) return adaf_fail(h, ADAF_E_BADARG, "%s: the loss needs old_logprobs, returns, loss_out and a workspace", name);
    if (loss_mode && grad_mode) return adaf_fail(h, ADAF_E_BADARG, "%s: either the PPO loss or upstream gradients", name);
    if (grad_mode && !dhead_out) return adaf_fail(h, ADAF_E_BADARG, "%s: upstream gradients without dhead_out", name);
    float* terms = static_cast<float*>(ws);       // (only the loss has a workspace; the kernel reads the argument in loss mode alone)
    int rc;
    if (loss_mode && (rc = adaf_check_ws(h, name, ws, ws_bytes, ppo_head_layout(ws, steps, batch, &terms), ADAF_WS_SIZE_FIRST))) return rc;
    hipStream_t st = (hipStream_t)stream;
    HeadArgs a = {};
    a.head = head; a.action = reinterpret_cast<const long long*>(actions); a.action_yx = action_yx; a.sigma = sigma;
    a.old_logprob = old_logprobs; a.returns = returns; a.g_logprob = g_logprob; a.g_value = g_value; a.g_entropy = g_entropy;
    a.logprob = logprobs_out; a.value = values_out; a.entropy = entropy_out; a.terms = terms; a.dhead = dhead_out;
    a.T = steps; a.B = batch; a.A = n_actions; a.head_bt = head_batch_major ? 1 : 0; a.mode = loss_mode ? 1 : (grad_mode ? 2 : 0);
    a.eps_clip = eps_clip;
    const int n = steps * batch;
    if (action_yx) hipLaunchKernelGGL(ppo_head_kernel<Gaussian>, dim3((n + 63) / 64), dim3(64), 0, st, a);
    else hipLaunchKernelGGL(ppo_head_kernel<Categorical>, dim3((n + 63) / 64), dim3(64), 0, st, a);
    if (loss_mode) hipLaunchKernelGGL(ppo_loss_sum_kernel, dim3(1), dim3(256), 0, st, a.terms, n, loss_out);
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? ADAF_OK : adaf_fail(h, ADAF_E_LAUNCH, "%s launch: %s", name, hipGetErrorString(e));
}

// Both encoder-backward exports: every check, the workspace layout, EncBackwardArgs, the chain.  The BatchNorm operands are null for the
// plain chain.  The exports refuse different shapes and that difference is kept: `plain_32` (adaf_ppo_encoder_backward_f32) takes 32 conv
// outputs only and any hidden size; the general export takes 32 or 64 outputs and refuses a hidden or map_pixels * conv_out that is no
// multiple of 4, with or without BatchNorm.
int encoder_backward(adaf_handle* h, const char* name, bool plain_32, const float* states, const float* e1, const float* e_bt,
                     const float* dx_bt, int steps, int batch, int map_pixels, int channels, int conv_out, int hidden, const float* w_lin_pm,
                     const float* c1, const float* gamma1, const float* mean1, const float* invstd1, const float* l1, const float* gamma2,
                     const float* mean2, const float* invstd2, float* dw_enc, float* dw_lin, float* db_lin, float* dgamma1, float* dbeta1,
                     float* dgamma2, float* dbeta2, void* ws, size_t ws_bytes, void* stream) {
    if (!h) return ADAF_E_BADARG;
    if (!states || !e1 || !e_bt || !dx_bt || !w_lin_pm || !dw_enc || !dw_lin || !db_lin || !ws) return adaf_fail(h, ADAF_E_BADARG, "%s: null pointer", name);
    const bool bn = c1 != nullptr;
    const void* bnp[] = {c1, gamma1, mean1, invstd1, l1, gamma2, mean2, invstd2, dgamma1, dbeta1, dgamma2, dbeta2};
    for (const void* q : bnp)
        if (!q != !bn) return adaf_fail(h, ADAF_E_BADARG, "%s: the BatchNorm operands go together (all or none)", name);
    if (steps <= 0 || batch <= 0 || map_pixels <= 0 || channels <= 0 || conv_out <= 0 || hidden <= 0)
        return adaf_fail(h, ADAF_E_BADARG, "%s: non-positive extent", name);
    if (plain_32) {
        if (conv_out != 32 || channels % 128) return adaf_fail(h, ADAF_E_LAYOUT, "%s: 32 conv outputs and channels %% 128 == 0 expected", name);
    } else {
        if (!sk_shape_ok(channels, conv_out)) return adaf_fail(h, ADAF_E_LAYOUT, "%s: 32 or 64 conv outputs and channels %% 128 == 0 expected", name);
        if (hidden % 4 || (map_pixels * conv_out) % 4) return adaf_fail(h, ADAF_E_LAYOUT, "%s: hidden and map_pixels * conv_out must be multiples of 4", name);
    }
    if (!adaf_aligned16(states)) return adaf_fail(h, ADAF_E_LAYOUT, "%s: 16-byte alignment", name);
    EncBackwardWs r;
    int rc = adaf_check_ws(h, name, ws, ws_bytes, enc_backward_layout(ws, steps, batch, map_pixels, channels, conv_out, hidden, bn, &r), ADAF_WS_ALIGN_FIRST);
    if (rc) return rc;
    EncBackwardArgs a = {};
    a.states = states; a.e1 = e1; a.e_bt = e_bt; a.dx_bt = dx_bt; a.w_lin_pm = w_lin_pm;
    a.c1 = c1; a.gamma1 = gamma1; a.mean1 = mean1; a.invstd1 = invstd1; a.l1 = l1; a.gamma2 = gamma2; a.mean2 = mean2; a.invstd2 = invstd2;
    a.dw_enc = dw_enc; a.dw_lin = dw_lin; a.db_lin = db_lin; a.dgamma1 = dgamma1; a.dbeta1 = dbeta1; a.dgamma2 = dgamma2; a.dbeta2 = dbeta2;
    a.steps = steps; a.batch = batch; a.map_pixels = map_pixels; a.channels = channels; a.conv_out = conv_out; a.hidden = hidden;
    if ((rc = run_encoder_backward(h, a, r, (hipStream_t)stream))) return rc;
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? ADAF_OK : adaf_fail(h, ADAF_E_LAUNCH, "%s launch: %s", name, hipGetErrorString(e));
}

}  // namespace

extern "C" {

int adaf_ppo_sample_f32(adaf_handle* h, const float* logits, int ld, int rows, int n_actions, const float* uniforms, int64_t* action_out,
                        float* logprob_out, float* probs_out, void* stream) {
    if (!h) return ADAF_E_BADARG;
    if (rows == 0) return ADAF_OK;
    if (!logits || !uniforms || !action_out || !logprob_out) return adaf_fail(h, ADAF_E_BADARG, "ppo_sample: null pointer");
    if (rows < 0 || n_actions <= 0) return adaf_fail(h, ADAF_E_BADARG, "ppo_sample: non-positive extent");
    if (ld == 0) ld = n_actions;
    if (ld < n_actions) return adaf_fail(h, ADAF_E_BADARG, "ppo_sample: ld < n_actions");
    hipLaunchKernelGGL(ppo_sample_kernel, dim3((rows + 63) / 64), dim3(64), 0, (hipStream_t)stream, logits, ld, rows, n_actions, uniforms,
                       reinterpret_cast<long long*>(action_out), logprob_out, probs_out);
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? ADAF_OK : adaf_hip_fail(h, e, "ppo_sample launch");
}

int adaf_ppo_sample_actions_f32(adaf_handle* h, const float* logits, int ld, int steps, int batch, int n_actions, const float* uniforms,
                                const float* table_yx, int64_t* action_out, float* logprob_out, float* coords_out, void* stream) {
    if (!h) return ADAF_E_BADARG;
    if (!logits || !uniforms || !action_out || !logprob_out) return adaf_fail(h, ADAF_E_BADARG, "ppo_sample_actions: null pointer");
    if (steps <= 0 || batch <= 0 || n_actions <= 0) return adaf_fail(h, ADAF_E_BADARG, "ppo_sample_actions: non-positive extent");
    if (!coords_out != !table_yx) return adaf_fail(h, ADAF_E_BADARG, "ppo_sample_actions: coords_out and table_yx go together");
    if (ld == 0) ld = n_actions;
    if (ld < n_actions) return adaf_fail(h, ADAF_E_BADARG, "ppo_sample_actions: ld < n_actions");
    const int n = steps * batch;
    hipLaunchKernelGGL(ppo_sample_actions_kernel, dim3((n + 63) / 64), dim3(64), 0, (hipStream_t)stream, logits, ld, steps, batch, n_actions,
                       uniforms, table_yx, reinterpret_cast<long long*>(action_out), logprob_out, coords_out);
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? ADAF_OK : adaf_hip_fail(h, e, "ppo_sample_actions launch");
}

int adaf_ppo_rewards_f32(adaf_handle* h, const float* logits, const float* base_logits, const int64_t* target, int steps, int batch,
                         int classes, int kind, float* rewards_out, float* conf_out, float* ce_last_out, void* stream) {
    if (!h) return ADAF_E_BADARG;
    if (!logits || !target || !rewards_out) return adaf_fail(h, ADAF_E_BADARG, "ppo_rewards: null pointer");
    if (steps <= 0 || batch <= 0 || classes <= 0) return adaf_fail(h, ADAF_E_BADARG, "ppo_rewards: non-positive extent");
    if (kind < ADAF_REWARD_PREV || kind > ADAF_REWARD_RANDOM) return adaf_fail(h, ADAF_E_BADARG, "ppo_rewards: kind must be 0 (prev), 1 (conf) or 2 (random)");
    if (kind == ADAF_REWARD_RANDOM && !base_logits) return adaf_fail(h, ADAF_E_BADARG, "ppo_rewards: the random reward needs base_logits");
    hipStream_t st = (hipStream_t)stream;
    const long long* tg = reinterpret_cast<const long long*>(target);
    hipLaunchKernelGGL(ppo_rewards_kernel, dim3(batch), dim3(64), 0, st, logits, base_logits, tg, steps, batch, classes, kind, rewards_out, conf_out);
    if (ce_last_out) hipLaunchKernelGGL(ppo_ce_last_kernel, dim3(1), dim3(256), 0, st, logits, tg, steps, batch, classes, ce_last_out);
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? ADAF_OK : adaf_hip_fail(h, e, "ppo_rewards launch");
}

size_t adaf_ce_steps_workspace_bytes(int batch, int steps) {
    float* row_loss;
    return (batch <= 0 || steps <= 0) ? 0 : ce_steps_layout(nullptr, batch, steps, &row_loss);
}

int adaf_ce_steps_f32(adaf_handle* h, const float* logits, const int64_t* target, int batch, int steps, int classes, float* loss_out,
                      float* dlogits_out, void* ws, size_t ws_bytes, void* stream) {
    if (!h) return ADAF_E_BADARG;
    if (!logits || !target || !loss_out || !ws) return adaf_fail(h, ADAF_E_BADARG, "ce_steps: null pointer");
    if (batch <= 0 || steps <= 0 || classes <= 0) return adaf_fail(h, ADAF_E_BADARG, "ce_steps: non-positive extent");
    const long long rows = (long long)batch * steps;
    if ((rows + 3) / 4 > 0x7fffffffLL) return adaf_fail(h, ADAF_E_BADARG, "ce_steps: more than 2^33 rows");
    float* row_loss;
    int rc = adaf_check_ws(h, "ce_steps", ws, ws_bytes, ce_steps_layout(ws, batch, steps, &row_loss), ADAF_WS_ALIGN_FIRST);
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(ce_steps_rows_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, st, logits, reinterpret_cast<const long long*>(target),
                       rows, steps, classes, row_loss, dlogits_out);
    hipLaunchKernelGGL(ce_steps_mean_kernel, dim3(1), dim3(256), 0, st, row_loss, rows, loss_out);
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? ADAF_OK : adaf_hip_fail(h, e, "ce_steps launch");
}

int adaf_ppo_returns_f32(adaf_handle* h, const float* rewards, int steps, int batch, float gamma, float* returns_out, void* stream) {
    if (!h) return ADAF_E_BADARG;
    if (!rewards || !returns_out) return adaf_fail(h, ADAF_E_BADARG, "ppo_returns: null pointer");
    if (steps <= 0 || batch <= 0) return adaf_fail(h, ADAF_E_BADARG, "ppo_returns: non-positive extent");
    hipLaunchKernelGGL(ppo_returns_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, rewards, steps, batch, gamma, returns_out);
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? ADAF_OK : adaf_hip_fail(h, e, "ppo_returns launch");
}

size_t adaf_ppo_head_workspace_bytes(int steps, int batch) {
    float* terms;
    return (steps <= 0 || batch <= 0) ? 0 : ppo_head_layout(nullptr, steps, batch, &terms);
}

int adaf_ppo_head_f32(adaf_handle* h, const float* head, int head_batch_major, int steps, int batch, int n_actions, const int64_t* actions,
                      const float* old_logprobs, const float* returns, float eps_clip, const float* g_logprob, const float* g_value,
                      const float* g_entropy, float* logprobs_out, float* values_out, float* entropy_out, float* loss_out, float* dhead_out,
                      void* ws, size_t ws_bytes, void* stream) {
    if (!h) return ADAF_E_BADARG;
    if (!head || !actions) return adaf_fail(h, ADAF_E_BADARG, "ppo_head: null pointer");
    if (steps <= 0 || batch <= 0 || n_actions <= 0) return adaf_fail(h, ADAF_E_BADARG, "ppo_head: non-positive extent");
    return run_ppo_head(h, "ppo_head", head, head_batch_major, steps, batch, n_actions, actions, nullptr, 0.f, old_logprobs, returns, eps_clip,
                        g_logprob, g_value, g_entropy, logprobs_out, values_out, entropy_out, loss_out, dhead_out, ws, ws_bytes, stream);
}

int adaf_ppo_rows_transpose_f32(adaf_handle* h, const float* in, int ni, int nj, int width, float* out, void* stream) {
    if (!h) return ADAF_E_BADARG;
    if (!in || !out) return adaf_fail(h, ADAF_E_BADARG, "ppo_rows_transpose: null pointer");
    if (ni <= 0 || nj <= 0 || width <= 0) return adaf_fail(h, ADAF_E_BADARG, "ppo_rows_transpose: non-positive extent");
    const size_t n = (size_t)ni * nj * width;
    hipLaunchKernelGGL(ppo_rows_transpose_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, in, nullptr, out, ni, nj, width);
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? ADAF_OK : adaf_hip_fail(h, e, "ppo_rows_transpose launch");
}

size_t adaf_ppo_wenc_grad_workspace_bytes(int pixels, int channels, int conv_out) {
    float* buf;
    return (pixels <= 0 || channels <= 0 || conv_out <= 0) ? 0 : wenc_layout(nullptr, pixels, channels, conv_out, &buf);
}

int adaf_ppo_wenc_grad_f32(adaf_handle* h, const float* states, const float* de1, const float* e1, int pixels, int channels, int conv_out,
                           int split_k, float* dw_out, void* ws, size_t ws_bytes, void* stream) {
    if (!h) return ADAF_E_BADARG;
    if (!states || !de1 || !dw_out || !ws) return adaf_fail(h, ADAF_E_BADARG, "ppo_wenc_grad: null pointer");
    if (pixels <= 0 || channels <= 0 || conv_out <= 0) return adaf_fail(h, ADAF_E_BADARG, "ppo_wenc_grad: non-positive extent");
    if (!adaf_aligned16(states) || !adaf_aligned16(dw_out)) return adaf_fail(h, ADAF_E_LAYOUT, "ppo_wenc_grad: 16-byte alignment");
    float* buf;
    int rc = adaf_check_ws(h, "ppo_wenc_grad", ws, ws_bytes, wenc_layout(ws, pixels, channels, conv_out, &buf), ADAF_WS_ALIGN_FIRST);
    if (rc) return rc;
    if ((rc = launch_wenc_grad(h, states, de1, e1, pixels, channels, conv_out, split_k, dw_out, buf, (hipStream_t)stream))) return rc;
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? ADAF_OK : adaf_hip_fail(h, e, "ppo_wenc_grad launch");
}

size_t adaf_ppo_encoder_backward_workspace_bytes(int steps, int batch, int map_pixels, int channels, int conv_out, int hidden) {
    EncBackwardWs r;
    if (steps <= 0 || batch <= 0 || map_pixels <= 0 || channels <= 0 || conv_out <= 0 || hidden <= 0) return 0;
    return enc_backward_layout(nullptr, steps, batch, map_pixels, channels, conv_out, hidden, false, &r);
}

int adaf_ppo_encoder_backward_f32(adaf_handle* h, const float* states, const float* e1, const float* e_bt, const float* dx_bt, int steps,
                                  int batch, int map_pixels, int channels, int conv_out, int hidden, const float* w_lin_pm, float* dw_enc,
                                  float* dw_lin, float* db_lin, void* ws, size_t ws_bytes, void* stream) {
    return encoder_backward(h, "ppo_encoder_backward", true, states, e1, e_bt, dx_bt, steps, batch, map_pixels, channels, conv_out, hidden, w_lin_pm,
                            nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, dw_enc, dw_lin, db_lin, nullptr, nullptr, nullptr,
                            nullptr, ws, ws_bytes, stream);
}

// ---- the continuous policy ------------------------------------------------------------------------------------------------
int adaf_ppo_gauss_sample_f32(adaf_handle* h, const float* mean, const float* noise, int rows, float sigma, float* action_out, float* logprob_out,
                              void* stream) {
    if (!h) return ADAF_E_BADARG;
    if (!mean || !noise || !action_out || !logprob_out) return adaf_fail(h, ADAF_E_BADARG, "ppo_gauss_sample: null pointer");
    if (rows <= 0 || !(sigma > 0.f)) return adaf_fail(h, ADAF_E_BADARG, "ppo_gauss_sample: non-positive extent or sigma");
    hipLaunchKernelGGL(ppo_gauss_sample_kernel, dim3((rows + 63) / 64), dim3(64), 0, (hipStream_t)stream, mean, noise, rows, sigma, action_out, logprob_out);
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? ADAF_OK : adaf_hip_fail(h, e, "ppo_gauss_sample launch");
}

int adaf_ppo_gauss_head_f32(adaf_handle* h, const float* head, int head_batch_major, int steps, int batch, const float* actions, float sigma,
                            const float* old_logprobs, const float* returns, float eps_clip, const float* g_logprob, const float* g_value,
                            float* logprobs_out, float* values_out, float* entropy_out, float* loss_out, float* dhead_out, void* ws,
                            size_t ws_bytes, void* stream) {
    if (!h) return ADAF_E_BADARG;
    if (!head || !actions) return adaf_fail(h, ADAF_E_BADARG, "ppo_gauss_head: null pointer");
    if (steps <= 0 || batch <= 0 || !(sigma > 0.f)) return adaf_fail(h, ADAF_E_BADARG, "ppo_gauss_head: non-positive extent or sigma");
    return run_ppo_head(h, "ppo_gauss_head", head, head_batch_major, steps, batch, 2, nullptr, actions, sigma, old_logprobs, returns, eps_clip,
                        g_logprob, g_value, nullptr, logprobs_out, values_out, entropy_out, loss_out, dhead_out, ws, ws_bytes, stream);
}

size_t adaf_bn_train_workspace_bytes(int rows, int cols) {
    double* part;
    return (rows <= 0 || cols <= 0) ? 0 : bn_layout(nullptr, cols, &part);
}

int adaf_bn_train_forward_f32(adaf_handle* h, const float* x, int rows, int cols, const float* gamma, const float* beta, float eps,
                              float momentum, float* running_mean, float* running_var, int relu, float* y_out, float* mean_out,
                              float* invstd_out, void* ws, size_t ws_bytes, void* stream) {
    if (!h) return ADAF_E_BADARG;
    if (!x || !gamma || !beta || !y_out || !mean_out || !invstd_out || !ws) return adaf_fail(h, ADAF_E_BADARG, "bn_train_forward: null pointer");
    if (rows <= 0 || cols <= 0) return adaf_fail(h, ADAF_E_BADARG, "bn_train_forward: non-positive extent");
    if (rows < 2) return adaf_fail(h, ADAF_E_BADARG, "bn_train_forward: more than one value per channel expected");
    double* part;
    int rc = adaf_check_ws(h, "bn_train_forward", ws, ws_bytes, bn_layout(ws, cols, &part), ADAF_WS_ALIGN_FIRST);
    if (rc) return rc;
    launch_bn_forward(x, rows, cols, gamma, beta, eps, momentum, running_mean, running_var, relu, y_out, mean_out, invstd_out, part, (hipStream_t)stream);
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? ADAF_OK : adaf_hip_fail(h, e, "bn_train_forward launch");
}

int adaf_bn_train_backward_f32(adaf_handle* h, const float* x, const float* y, const float* dy, int rows, int cols, const float* gamma,
                               const float* mean, const float* invstd, float* dx_out, float* dgamma_out, float* dbeta_out, void* ws,
                               size_t ws_bytes, void* stream) {
    if (!h) return ADAF_E_BADARG;
    if (!x || !dy || !gamma || !mean || !invstd || !dx_out || !dgamma_out || !dbeta_out || !ws) return adaf_fail(h, ADAF_E_BADARG, "bn_train_backward: null pointer");
    if (rows <= 0 || cols <= 0) return adaf_fail(h, ADAF_E_BADARG, "bn_train_backward: non-positive extent");
    double* part;
    int rc = adaf_check_ws(h, "bn_train_backward", ws, ws_bytes, bn_layout(ws, cols, &part), ADAF_WS_ALIGN_FIRST);
    if (rc) return rc;
    launch_bn_backward(x, y, dy, rows, cols, gamma, mean, invstd, dx_out, dgamma_out, dbeta_out, part, (hipStream_t)stream);
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? ADAF_OK : adaf_hip_fail(h, e, "bn_train_backward launch");
}

size_t adaf_ppo_encoder_bn_backward_workspace_bytes(int steps, int batch, int map_pixels, int channels, int conv_out, int hidden, int with_bn) {
    EncBackwardWs r;
    if (steps <= 0 || batch <= 0 || map_pixels <= 0 || channels <= 0 || conv_out <= 0 || hidden <= 0) return 0;
    return enc_backward_layout(nullptr, steps, batch, map_pixels, channels, conv_out, hidden, with_bn != 0, &r);
}

int adaf_ppo_encoder_bn_backward_f32(adaf_handle* h, const float* states, const float* e1, const float* e_bt, const float* dx_bt, int steps,
                                     int batch, int map_pixels, int channels, int conv_out, int hidden, const float* w_lin_pm,
                                     const float* c1, const float* gamma1, const float* mean1, const float* invstd1, const float* l1,
                                     const float* gamma2, const float* mean2, const float* invstd2, float* dw_enc, float* dw_lin,
                                     float* db_lin, float* dgamma1, float* dbeta1, float* dgamma2, float* dbeta2, void* ws, size_t ws_bytes,
                                     void* stream) {
    return encoder_backward(h, "ppo_encoder_bn_backward", false, states, e1, e_bt, dx_bt, steps, batch, map_pixels, channels, conv_out, hidden, w_lin_pm,
                            c1, gamma1, mean1, invstd1, l1, gamma2, mean2, invstd2, dw_enc, dw_lin, db_lin, dgamma1, dbeta1, dgamma2, dbeta2, ws,
                            ws_bytes, stream);
}

}  // extern "C"
