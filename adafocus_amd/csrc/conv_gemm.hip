// Implicit-GEMM convolution + folded-BN + residual + activation on the gfx950 fp32 matrix
// cores (v_mfma_f32_32x32x2_f32).  One kernel family serves every dense contraction on the
// AdaFocus hot path: the ResNet-50 1x1 / 3x3 / strided convs (ACT/models/resnet.py:94-114),
// the 7x7 stem (cin padded 3 -> 4), the GRU input/recurrent projections and the classifiers.
//
// GEMM view:  out[M = n*OH*OW pixels, N = cout] = A[M, K = kh*kw*cin] * W[N, K]^T
//   A is never materialised: each 16-byte operand chunk is gathered straight from the NHWC
//   activation tensor (zero for padding / clip-boundary TSM rows), staged in LDS and consumed
//   as MFMA fragments.  Activations are pixel-major, so an output row's `cout` values are
//   contiguous and the MFMA C layout (col = lane & 31) stores 128-byte segments.
//
// Block = 256 threads = 4 waves (64 lanes).  K is walked in BK = 32 slices, double-buffered
// in LDS (row pitch 36 floats: conflict-free for the 16-lane ds_read_b128 groups and for the
// 8-lane ds_write_b128 groups), with the next slice's global loads in flight while the current
// one is multiplied.  A lane's ds_read_b128 brings four k-values for its row; MFMA sub-step s
// consumes element s, so lanes 0-31 cover k = 8kk+s and lanes 32-63 cover k = 8kk+4+s -- the
// same permutation on A and W, hence an exact (re-ordered) fp32 fma chain.
#include <cstdlib>
#include <type_traits>
#include <utility>

#include "adaf_internal.h"

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));  // native vector: stays in VGPRs (HIP's float4 struct defeats SROA)
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));

// Ablation builds of the split tiles' production schedule (tools/exp/build_cg_abl.sh; the results are garbage, the TIME is the measurement):
// 1 = no activation split (raw bits go to the MFMAs), 2 = no wait for the DMA before the slice barrier, 4 = no DMA inside the K loop,
// 8 = no epilogue, 16 = no MFMAs; 32 = (lean kernels of BOTH pipes) every tile reads the same 1024 activation rows, i.e. activations from L2:
// what a launch would cost if its input never came from HBM -- the ceiling of fusing it behind its producer.  The product is built with 0.
#ifndef CG_ABL
#define CG_ABL 0
#endif

namespace {

// ---- fp32 operands on the bf16 matrix pipe (opt-in "split" tiles) -----------------------------------
// x = h + m + l EXACTLY with h = bf16(x), m = bf16(x - h), l = x - h - m, conversions round-to-nearest-even
// (v_cvt_pk_bf16_f32): both subtractions are exact in fp32 and the last remainder has at most 8 significant bits,
// so it is a bf16.  |m| <= 2^-8 |x|, |l| <= 2^-16 |x| with signs independent of x.  The fp32 product x*y is the sum of
// nine bf16*bf16 products, each exact in the fp32 accumulator's input; the "6" form drops m*l, l*m, l*l -- below
// 2^-24 |xy| and, because of the rounding, of either sign (with a truncating split the dropped terms all carry the
// sign of xy and the bias adds up over K and over layers: measured 2.5x the fp32 pipe's error on the whole trunk).
// Eight consecutive k values of a row -> three register quads of packed bf16 pairs.
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ void split3(const f32x4 v0, const f32x4 v1, u32x4& H, u32x4& M, u32x4& L) {
    const float x[8] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w};
    unsigned h[4], m[4], l[4];
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        const f32x2 xv = {x[2 * p], x[2 * p + 1]};
        h[p] = __builtin_bit_cast(unsigned, __builtin_convertvector(xv, bf16x2));
        const f32x2 hv = {__uint_as_float(h[p] << 16), __uint_as_float(h[p] & 0xffff0000u)};
        const f32x2 r1 = xv - hv;                                    // exact
        m[p] = __builtin_bit_cast(unsigned, __builtin_convertvector(r1, bf16x2));
        const f32x2 mv = {__uint_as_float(m[p] << 16), __uint_as_float(m[p] & 0xffff0000u)};
        const f32x2 r2 = r1 - mv;                                    // exact, <= 8 significant bits left
        l[p] = __builtin_amdgcn_perm(__float_as_uint(r2.y), __float_as_uint(r2.x), 0x07060302u);
    }
    H = u32x4{h[0], h[1], h[2], h[3]};
    M = u32x4{m[0], m[1], m[2], m[3]};
    L = u32x4{l[0], l[1], l[2], l[3]};
}
__device__ __forceinline__ f32x16 mfma_bf16(const u32x4 a, const u32x4 b, const f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
}
// ---- parts the GEMM kernels share ---------------------------------------------------------------------------------------------------
// Each of these is a function because every kernel that takes it compiles to the instructions it had with the part written out
// (tools/codeobj_compare.py).  The fragment offsets, the fragment read, the slice step and the K-loop drivers are NOT: moved into a
// function they change most instantiations, so conv_gemm_glds_kernel and phase 1 of conv_fused_tail_kernel each write them out
// (LABNOTES, "Conv engine kernels").
//
// The slice image of an operand in LDS (direct-to-LDS kernels) is [rows][32 floats] = 8 chunks of 16 bytes per row, NO padding: the DMA
// writes base + lane * 16 B.  A wave instruction fills 8 consecutive rows x 128 B; lane -> (row = 8*g + lane/8, slot = lane%8).  Bank
// conflicts are avoided by an XOR swizzle: chunk c of a row lives in slot c ^ ((row>>1)&7), applied on the per-lane GLOBAL source
// address (slot -> chunk) and again on the fragment read (chunk -> slot).
__device__ __forceinline__ int slice_chunk(int row, int slot) { return slot ^ ((row >> 1) & 7); }

// A 64-bit value that is wave-uniform by construction: pin it to SGPRs.
__device__ __forceinline__ unsigned long long pin_sgpr(unsigned long long v) {
    return ((unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((unsigned)(v >> 32)) << 32) |
           (unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((unsigned)v);
}
// Scalar-base LDS-DMA (the LEAN note at conv_gemm_glds_kernel's operand source): global_load_lds_dwordx4 voffset, s[base:base+1] -- a constant per-lane
// byte offset, a wave-uniform base the SALU advances, 16 bytes per lane to LDS byte address `lds` + lane * 16.
__device__ __forceinline__ void lds_dma_sbase(const float* sbase, unsigned voff, unsigned lds) {
    const unsigned l = (unsigned)__builtin_amdgcn_readfirstlane(lds);
    const unsigned long long sb = pin_sgpr((unsigned long long)sbase);
    // (s_nop: the M0 write -> LDS-DMA read hazard the compiler pads for its own builtin is ours to pad inside an asm block)
    asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2" ::"s"(l), "v"(voff), "s"(sb) : "memory", "m0");   // (m0 is named so that the compiler does not merge its own M0 initialisations across this block; the "reserved register" warning is expected)
}

// sub-step s4 of an 8-k step: one v_mfma_f32_32x32x2_f32 per tile pair on element s4 of the wave's 16-byte fragments
template <int TM, int TN>
__device__ __forceinline__ void mfma_step(f32x16 (&acc)[TM][TN], const f32x4 (&af)[TM], const f32x4 (&bf)[TN], int s4) {
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[i][s4], bf[j][s4], acc[i][j], 0, 0, 0);
}

// Row-major decode of an output row: m -> (image, pixel inside the image = rem, oy, ox).  A position-major tile index decodes the same
// way into (image group, the tile's pixel): group-major order, so consecutive tiles (= one XCD's share, see xcd_tile) are all pixel
// positions of the SAME images and the rows an XCD gathers stay within a few image groups and in its L2 (position-major order made every
// XCD touch every image: measured 3x less gain).
struct OutPix { int img, rem, oy, ox; };
__device__ __forceinline__ OutPix out_pixel(const ConvArgs& a, int m) {
    const int ohw = a.OH * a.OW;
    const int img = m / ohw;
    const int rem = m - img * ohw;
    const int oy = rem / a.OW;
    const int ox = rem - oy * a.OW;
    return {img, rem, oy, ox};
}
// The K walk of a k x k filter: one filter tap's 32-channel slice per step (cin % 32 == 0).  Called for kt = 0, 1, 2, ..., so the
// (tap, channel offset) pair is advanced incrementally -- scalar adds, no division.  SKIP (position-major tiles): a move to a new
// tap goes on to the next tap in `walk`, the ones that touch the image (wave-uniform; the centre tap always does).
template <bool SKIP>
__device__ __forceinline__ void tap_walk_step(int kt, const ConvArgs& a, unsigned walk, int& tap, int& c0, int& kh, int& kw) {
    bool moved = false;
    if (kt == 0) { c0 = 0; tap = 0; kh = 0; kw = 0; moved = true; }
    else {
        c0 += 32;
        if (c0 == a.cin) {
            c0 = 0;
            ++tap;
            if (++kw == a.KW) { kw = 0; ++kh; }
            moved = true;
        }
    }
    if (SKIP && moved) {
        while (!((walk >> tap) & 1u)) {
            ++tap;
            if (++kw == a.KW) { kw = 0; ++kh; }
        }
    }
}

// sig: 0 = nothing left to do, 1 = sigmoid, 2 = swish (v * sigmoid(v); efficientnet_pytorch utils.py MemoryEfficientSwish)
// The logistic function is 1 / (1 + 2^(-v log2 e)) on the hardware's exp2 / reciprocal units (v_exp_f32, v_rcp_f32: 1 ulp each,
// ~2e-7 relative overall) -- expf() + an IEEE division are ~40 VALU instructions per element, which made the swish epilogues
// of EfficientNet's expand convs (K = 24..384: hardly any MFMA work per output) VALU-bound.  Saturates correctly: v -> -inf
// gives rcp(inf) = 0, v -> +inf gives rcp(1) = 1.
// The fast form is for swish only.  A plain sigmoid (sig == 1) keeps expf + the IEEE division -- bit-comparable with conv_naive_kernel and
// with what round 2 shipped: the continuous policy's actor ends in a sigmoid whose output becomes a crop origin through floor(), where
// one ulp can move a patch by a pixel, and its epilogues are a handful of elements.
__device__ __forceinline__ float finish_act(float v, int sig) {
    if (sig == 0) return v;
    if (sig == 1) return 1.f / (1.f + expf(-v));
    return v * __builtin_amdgcn_rcpf(1.f + __builtin_amdgcn_exp2f(v * -1.4426950408889634f));
}

// ---- epilogue shared by both kernel families: BN affine, residual, activation ---------------
// C layout of the MFMA: col = lane&31, row = (r&3)+8(r>>2)+4(lane>>5).
// ET (half-precision storage variants, N2): bit 0 = `out` holds fp16, bit 1 = `res` holds fp16; strides stay in ELEMENTS.
// Row map: tile row `ml` (m0 + offset inside the tile) lives at output row ml * rstride + roff and exists iff ml < rlimit.
// Default (1, 0, a.M): the tile's rows are consecutive output pixels.  Position-major tiles (PM kernels): ml = image index,
// rstride = OH*OW, roff = the tile's pixel position, rlimit = number of images.
template <int TM, int TN, int ET = 0>
__device__ __forceinline__ void conv_epilogue(const ConvArgs& a0, float* smem, f32x16 (&acc)[TM][TN], int m0, int n0,
                                              int wm, int wn, int lane, int wave, int rstride = 1, int roff = 0, int rlimit = -1) {
    constexpr bool O16 = (ET & 1) != 0, R16 = (ET & 2) != 0;
    // a launch that carries two convs over the same input (ConvArgs::split_n): this column tile's destination and activation
    ConvArgs a = a0;
    if (a0.split_n && n0 >= a0.split_n) { a.out = a0.out_b; a.ldo = a0.ldo_b; a.act = a0.act_b; }
    if (rlimit < 0) rlimit = a.M;
    const int sig = a.act == ADAF_ACT_SIGMOID ? 1 : a.act == ADAF_ACT_SWISH ? 2 : 0;
    const float act_lo = (a.act == ADAF_ACT_NONE || sig) ? -__builtin_inff() : 0.f;
    const float act_hi = a.act == ADAF_ACT_RELU6 ? 6.f : __builtin_inff();
    const int crow = 4 * (lane >> 5);
    if (ET == 0 && a.vec_epi == 2 && !sig) {
        // ---- interior tiles (every row and column of the wave's sub-tile exists): the lean form.  fp32 MFMA and the VALU
        // share lanes on gfx950, so for the short-K launches (K = 64..256: 1024..4096 MFMA passes per wave tile) the
        // several hundred VALU passes of the general epilogue below -- 64-bit address arithmetic per row, the selects of the
        // bounds handling, four ALU ops per element -- are time the matrix pipe does not get.  Here: scalar row bases the
        // SALU advances + one constant 32-bit lane offset (global_load/store saddr form, no address VALU), no bounds
        // selects, and v_pk_fma / v_pk_add / v_med3: 2 VALU per element instead of 4.  Same arithmetic, same results.
        constexpr int WM = TM * 32, WN = TN * 32, SP = WN + 4;
        constexpr int C4 = WN / 4, RPI = 64 / C4;
        const int mrow0 = m0 + wm * WM, n0w = n0 + wn * WN;
        const size_t span_o = (size_t)(RPI - 1) * rstride * a.ldo + a.N, span_r = (size_t)(RPI - 1) * rstride * a.ldr + a.N;
        if (mrow0 + WM <= rlimit && n0w + WN <= a.N && span_o < (1u << 29) && span_r < (1u << 29)) {
            float* st = smem + wave * 32 * SP;
            const int c4 = lane % C4, rsub = lane / C4;
            const int n = n0w + 4 * c4;
            const f32x4 one4 = {1.f, 1.f, 1.f, 1.f}, zero4 = {0.f, 0.f, 0.f, 0.f};
            const f32x4 sc = a.scale ? *reinterpret_cast<const f32x4*>(a.scale + n) : one4;
            const f32x4 bi = a.bias ? *reinterpret_cast<const f32x4*>(a.bias + n) : zero4;
            const f32x2 sc0 = {sc.x, sc.y}, sc1 = {sc.z, sc.w}, bi0 = {bi.x, bi.y}, bi1 = {bi.z, bi.w};
            const unsigned vo = (unsigned)(((size_t)rsub * rstride * a.ldo + n) * 4);
            const unsigned vr = (unsigned)(((size_t)rsub * rstride * a.ldr + n) * 4);
            const size_t row0 = (size_t)mrow0 * rstride + roff;
            const unsigned long long obase = pin_sgpr((unsigned long long)a.out + row0 * a.ldo * 4);
            const unsigned long long rbase = pin_sgpr((unsigned long long)a.res + row0 * a.ldr * 4);
            const unsigned long long ostep = pin_sgpr((unsigned long long)RPI * rstride * a.ldo * 4);
            const unsigned long long rstep = pin_sgpr((unsigned long long)RPI * rstride * a.ldr * 4);
            constexpr int GPB = (32 / RPI) / 4, NGR = TM * GPB;     // groups of four row steps
            typedef __attribute__((address_space(1))) char gchar;      // (global address space: plain pointers made from
            typedef __attribute__((address_space(1))) f32x4 gf32x4;    //  integers would be FLAT accesses)
            auto run = [&](auto res_tag) {
                constexpr bool RES = decltype(res_tag)::value;
                f32x4 rv[2][4];
                auto ldres = [&](int g, int buf) {
#pragma unroll
                    for (int u = 0; u < 4; ++u)
                        rv[buf][u] = *reinterpret_cast<const gf32x4*>(reinterpret_cast<const gchar*>(rbase + (unsigned long long)(g * 4 + u) * rstep) + vr);
                };
                if (RES) ldres(0, 0);
#pragma unroll
                for (int i = 0; i < TM; ++i) {
                    __builtin_amdgcn_wave_barrier();
#pragma unroll
                    for (int j = 0; j < TN; ++j)
#pragma unroll
                        for (int r = 0; r < 16; ++r)
                            st[(crow + (r & 3) + 8 * (r >> 2)) * SP + j * 32 + (lane & 31)] = acc[i][j][r];
                    __builtin_amdgcn_wave_barrier();
#pragma unroll
                    for (int gi = 0; gi < GPB; ++gi) {
                        const int g = i * GPB + gi, cb = g & 1;
                        if (RES && g + 1 < NGR) ldres(g + 1, cb ^ 1);
#pragma unroll
                        for (int u = 0; u < 4; ++u) {
                            const int row = (gi * 4 + u) * RPI + rsub;
                            const f32x4 v = *reinterpret_cast<const f32x4*>(st + row * SP + 4 * c4);
                            f32x2 p0 = __builtin_elementwise_fma(f32x2{v.x, v.y}, sc0, bi0);
                            f32x2 p1 = __builtin_elementwise_fma(f32x2{v.z, v.w}, sc1, bi1);
                            if (RES) {
                                p0 += f32x2{rv[cb][u].x, rv[cb][u].y};
                                p1 += f32x2{rv[cb][u].z, rv[cb][u].w};
                            }
                            const f32x4 o = {__builtin_amdgcn_fmed3f(p0.x, act_lo, act_hi), __builtin_amdgcn_fmed3f(p0.y, act_lo, act_hi),
                                             __builtin_amdgcn_fmed3f(p1.x, act_lo, act_hi), __builtin_amdgcn_fmed3f(p1.y, act_lo, act_hi)};
                            *reinterpret_cast<gf32x4*>(reinterpret_cast<gchar*>(obase + (unsigned long long)(g * 4 + u) * ostep) + vo) = o;
                        }
                    }
                }
            };
            if (a.res != nullptr) run(std::true_type{});
            else run(std::false_type{});
            return;
        }
    }
    if (a.vec_epi) {
        // Transpose the wave's WM x WN tile through its private LDS slab (the K-loop buffers are
        // free after the final barrier) so every lane owns 4 consecutive channels of a row:
        // residual loads and output stores become 16-byte accesses, 4x fewer memory instructions.
        constexpr int WM = TM * 32, WN = TN * 32, SP = WN + 4;
        float* st = smem + wave * 32 * SP;
        constexpr int C4 = WN / 4, RPI = 64 / C4;   // 16-byte chunks per row, rows per wave instruction
        const int c4 = lane % C4, rsub = lane / C4;
        const int n = n0 + wn * WN + 4 * c4;
        const bool n_ok = n < a.N;
        const int nn = n_ok ? n : 0;
        const f32x4 one4 = {1.f, 1.f, 1.f, 1.f}, zero4 = {0.f, 0.f, 0.f, 0.f};
        const f32x4 sc = a.scale ? *reinterpret_cast<const f32x4*>(a.scale + nn) : one4;
        const f32x4 bi = a.bias ? *reinterpret_cast<const f32x4*>(a.bias + nn) : zero4;
        const bool has_res = a.res != nullptr;
        // Identity rows travel one group of four rows-per-lane ahead of their use: the loads of group g+1 are issued before
        // group g is finished, and group 0's before the first transposition, so no epilogue step waits on HBM / L2 with
        // nothing else to do.  Launches without a residual (most) issue no load at all.
        constexpr int GPB = (32 / RPI) / 4;      // groups per 32-row band
        constexpr int NGR = TM * GPB;
        f32x4 rv[2][4];
#pragma unroll
        for (int q = 0; q < 2; ++q)
#pragma unroll
            for (int u = 0; u < 4; ++u) rv[q][u] = zero4;
        auto ldres = [&](int g, int buf) {
            const int i = g / GPB, it = (g % GPB) * 4;
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int ml = m0 + wm * WM + i * 32 + (it + u) * RPI + rsub;
                const bool ok = n_ok && ml < rlimit;
                const size_t m = (size_t)ml * rstride + roff;
                if (R16) {
                    const f16x4 hv = *reinterpret_cast<const f16x4*>(ok ? reinterpret_cast<const _Float16*>(a.res) + m * a.ldr + n
                                                                        : reinterpret_cast<const _Float16*>(a.zeros));
                    rv[buf][u] = f32x4{(float)hv.x, (float)hv.y, (float)hv.z, (float)hv.w};
                } else
                    rv[buf][u] = *reinterpret_cast<const f32x4*>(ok ? a.res + m * a.ldr + n : a.zeros);
            }
        };
        if (has_res) ldres(0, 0);
#pragma unroll
        for (int i = 0; i < TM; ++i) {   // one 32-row band at a time
            __builtin_amdgcn_wave_barrier();  // same-wave LDS ops complete in order; just pin the order
#pragma unroll
            for (int j = 0; j < TN; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r)
                    st[(crow + (r & 3) + 8 * (r >> 2)) * SP + j * 32 + (lane & 31)] = acc[i][j][r];
            __builtin_amdgcn_wave_barrier();
#pragma unroll
            for (int gi = 0; gi < GPB; ++gi) {
                const int g = i * GPB + gi, it = gi * 4, cb = g & 1;
                if (has_res && g + 1 < NGR) ldres(g + 1, cb ^ 1);
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int row = (it + u) * RPI + rsub;
                    const int ml = m0 + wm * WM + i * 32 + row;
                    const size_t m = (size_t)ml * rstride + roff;
                    const f32x4 v = *reinterpret_cast<const f32x4*>(st + row * SP + 4 * c4);
                    f32x4 o;
                    o.x = finish_act(fminf(fmaxf(fmaf(v.x, sc.x, bi.x) + rv[cb][u].x, act_lo), act_hi), sig);
                    o.y = finish_act(fminf(fmaxf(fmaf(v.y, sc.y, bi.y) + rv[cb][u].y, act_lo), act_hi), sig);
                    o.z = finish_act(fminf(fmaxf(fmaf(v.z, sc.z, bi.z) + rv[cb][u].z, act_lo), act_hi), sig);
                    o.w = finish_act(fminf(fmaxf(fmaf(v.w, sc.w, bi.w) + rv[cb][u].w, act_lo), act_hi), sig);
                    if (n_ok && ml < rlimit) {
                        if (O16)
                            *reinterpret_cast<f16x4*>(reinterpret_cast<_Float16*>(a.out) + m * a.ldo + n) =
                                f16x4{(_Float16)o.x, (_Float16)o.y, (_Float16)o.z, (_Float16)o.w};
                        else
                            *reinterpret_cast<f32x4*>(a.out + m * a.ldo + n) = o;
                    }
                }
            }
        }
        return;
    }
    // scalar fallback (unaligned strides / channel counts that are not multiples of 4)
    const bool has_res = a.res != nullptr;
#pragma unroll
    for (int j = 0; j < TN; ++j) {
        const int n = n0 + (wn * TN + j) * 32 + (lane & 31);
        const bool n_ok = n < a.N;
        const int nn = n_ok ? n : 0;
        const float sc = a.scale ? a.scale[nn] : 1.f;
        const float bi = a.bias ? a.bias[nn] : 0.f;
#pragma unroll
        for (int i = 0; i < TM; ++i) {
            const int mb = m0 + (wm * TM + i) * 32 + crow;
            float rv[16];
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int ml = mb + (r & 3) + 8 * (r >> 2);
                const size_t m = (size_t)ml * rstride + roff;
                const bool ok = has_res && n_ok && ml < rlimit;
                if (R16) rv[r] = ok ? (float)reinterpret_cast<const _Float16*>(a.res)[m * a.ldr + n] : 0.f;
                else rv[r] = *(ok ? a.res + m * a.ldr + n : a.zeros);
            }
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int ml = mb + (r & 3) + 8 * (r >> 2);
                const size_t m = (size_t)ml * rstride + roff;
                const float v = finish_act(fminf(fmaxf(fmaf(acc[i][j][r], sc, bi) + rv[r], act_lo), act_hi), sig);
                if (n_ok && ml < rlimit) {
                    if (O16) reinterpret_cast<_Float16*>(a.out)[m * a.ldo + n] = (_Float16)v;
                    else a.out[m * a.ldo + n] = v;
                }
            }
        }
    }
}

// ---- epilogue with the global average pool folded in (ACT/models/resnet.py:222-223 avgpool + flatten) ----------
// The trunk's last conv3 (+ BN + identity + ReLU) does not write its map: a tile's rows are whole images (pool_rows = images x
// pool_hw pixels), every wave transposes its bands through its slab exactly as conv_epilogue does, applies the same arithmetic and
// parks the activated values in an LDS tile; after one barrier a thread per (image, channel) adds the pool_hw pixels IN PIXEL
// ORDER and divides by pool_hw -- the order and the operations of avgpool_kernel (misc_ops.hip), so the features are
// bit-identical to conv + separate pool (tests/test_hip_parity_r3.py).  Saves the 75 MB map's round trip and a launch.
// SIG (fp16-operand launches: EfficientNet's head conv, adaf_launch_conv_pool16): the activation may be swish / sigmoid, finished by
// finish_act exactly as conv_epilogue does (clamp bounds open for them), so the pooled features are the bits of conv + avgpool_kernel.
// RND (the fp16 ResNet trunk's last conv3, adaf_launch_conv_pool16_rounded): the residual is fp16 (widened), and every activated value is
// ROUNDED to fp16 (adaf_f16_of, the conv's fp16 store) and widened back before it is parked -- the pool averages the values the unfused
// conv would have stored, in pixel order, as avgpool_f16_kernel (misc_ops.hip) does: the same bits.
template <int TM, int TN, int BM, int BN, int NW, bool SIG = false, bool RND = false>
__device__ __forceinline__ void conv_epilogue_pool(const ConvArgs& a, float* smem, f32x16 (&acc)[TM][TN], int m0, int n0, int wm, int wn,
                                                   int lane, int wave, int tile_m) {
    constexpr int WM = TM * 32, WN = TN * 32, SP = WN + 4, PP = BN + 4;
    float* st = smem + wave * 32 * SP;
    float* P = smem + NW * 32 * SP;                    // [BM][PP]
    constexpr int C4 = WN / 4, RPI = 64 / C4;
    const int c4 = lane % C4, rsub = lane / C4;
    const int crow = 4 * (lane >> 5);
    const int n = n0 + wn * WN + 4 * c4;
    const bool n_ok = n < a.N;
    const int nn = n_ok ? n : 0;
    const f32x4 one4 = {1.f, 1.f, 1.f, 1.f}, zero4 = {0.f, 0.f, 0.f, 0.f};
    const f32x4 sc = a.scale ? *reinterpret_cast<const f32x4*>(a.scale + nn) : one4;
    const f32x4 bi = a.bias ? *reinterpret_cast<const f32x4*>(a.bias + nn) : zero4;
    const int sig = !SIG ? 0 : a.act == ADAF_ACT_SIGMOID ? 1 : a.act == ADAF_ACT_SWISH ? 2 : 0;
    const float act_lo = (a.act == ADAF_ACT_NONE || sig) ? -__builtin_inff() : 0.f;
    const float act_hi = a.act == ADAF_ACT_RELU6 ? 6.f : __builtin_inff();
#pragma unroll
    for (int i = 0; i < TM; ++i) {
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) st[(crow + (r & 3) + 8 * (r >> 2)) * SP + j * 32 + (lane & 31)] = acc[i][j][r];
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int u = 0; u < 32 / RPI; ++u) {
            const int row = u * RPI + rsub;
            const int lrow = wm * WM + i * 32 + row;                 // row inside the tile
            const int ml = m0 + lrow;
            const bool ok = n_ok && lrow < a.pool_rows && ml < a.M;
            f32x4 rv = zero4;
            if (RND) {
                if (ok && a.res) {
                    const f16x4 hv = *reinterpret_cast<const f16x4*>(reinterpret_cast<const _Float16*>(a.res) + (size_t)ml * a.ldr + n);
                    rv = f32x4{(float)hv.x, (float)hv.y, (float)hv.z, (float)hv.w};
                }
            } else if (ok && a.res) rv = *reinterpret_cast<const f32x4*>(a.res + (size_t)ml * a.ldr + n);
            const f32x4 v = *reinterpret_cast<const f32x4*>(st + row * SP + 4 * c4);
            f32x4 o;
            o.x = fminf(fmaxf(fmaf(v.x, sc.x, bi.x) + rv.x, act_lo), act_hi);
            o.y = fminf(fmaxf(fmaf(v.y, sc.y, bi.y) + rv.y, act_lo), act_hi);
            o.z = fminf(fmaxf(fmaf(v.z, sc.z, bi.z) + rv.z, act_lo), act_hi);
            o.w = fminf(fmaxf(fmaf(v.w, sc.w, bi.w) + rv.w, act_lo), act_hi);
            if constexpr (SIG) { o.x = finish_act(o.x, sig); o.y = finish_act(o.y, sig); o.z = finish_act(o.z, sig); o.w = finish_act(o.w, sig); }
            if constexpr (RND) {
                o.x = (float)adaf_f16_of(o.x); o.y = (float)adaf_f16_of(o.y); o.z = (float)adaf_f16_of(o.z); o.w = (float)adaf_f16_of(o.w);
            }
            *reinterpret_cast<f32x4*>(P + lrow * PP + wn * WN + 4 * c4) = o;
        }
    }
    __syncthreads();
    const int ipt = a.pool_rows / a.pool_hw;           // images per tile
    const int images = a.M / a.pool_hw;
    const float inv = (float)a.pool_hw;
    for (int idx = threadIdx.x; idx < ipt * (BN / 4); idx += 64 * NW) {
        const int im = idx / (BN / 4), cq = idx - im * (BN / 4);
        const int img = tile_m * ipt + im, nc = n0 + 4 * cq;
        if (img >= images || nc >= a.N) continue;
        f32x4 s = {0.f, 0.f, 0.f, 0.f};
        const float* p = P + (im * a.pool_hw) * PP + 4 * cq;
        for (int r = 0; r < a.pool_hw; ++r) s += *reinterpret_cast<const f32x4*>(p + r * PP);
        const f32x4 q = {s.x / inv, s.y / inv, s.z / inv, s.w / inv};
        *reinterpret_cast<f32x4*>(a.pool_out + (size_t)img * a.pool_ld + nc) = q;
    }
}

// FLAGS bit 0: raise wave priority around the MFMA cluster (s_setprio)
template <int BM, int BN, int WGM, int WGN, int BK, bool DENSE, int FLAGS, int ET = 0>
__global__ __launch_bounds__(64 * WGM * WGN) void conv_gemm_kernel(const ConvArgs a) {
    constexpr int NT = 64 * WGM * WGN;      // threads per block
    constexpr int LDP = BK + 4;             // LDS row pitch in floats (conflict-free b128 access)
    constexpr int QK = BK / 4;              // 16-byte chunks per k slice
    constexpr int RPP = NT / QK;            // rows staged per pass
    constexpr int TM = BM / WGM / 32, TN = BN / WGN / 32;
    constexpr int AP = BM / RPP, BP = BN / RPP;
    constexpr int STAGE = (BM + BN) * LDP;
    static_assert(BM % RPP == 0 && BN % RPP == 0 && AP >= 1 && BP >= 1, "staging shape");
    constexpr int SLAB = WGM * WGN * 32 * (TN * 32 + 4);   // epilogue transpose slabs (one 32-row band per wave)
    constexpr int SMEM = 2 * STAGE > SLAB ? 2 * STAGE : SLAB;
    __shared__ __attribute__((aligned(16))) float smem[SMEM];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int wm = wave / WGN, wn = wave % WGN;

    const int bid = xcd_tile(blockIdx.x, a.nblocks);
    const int tile_m = bid / a.tiles_n;
    const int tile_n = bid - tile_m * a.tiles_n;
    const int m0 = tile_m * BM, n0 = tile_n * BN;

    const int lrow = tid / QK;  // row inside a staging pass
    const int lq = tid % QK;    // which 16-byte chunk of the k slice

    // ---- per-thread row bookkeeping for the operand gather --------------------------------
    bool a_ok[AP];
    size_t a_off[AP];   // DENSE: row offset in floats
    int a_pix[AP];      // generic: image base pixel; DENSE+TSM: bit0 = has previous frame, bit1 = has next frame
    int a_iy[AP], a_ix[AP];
#pragma unroll
    for (int p = 0; p < AP; ++p) {
        const int m = m0 + lrow + RPP * p;
        a_ok[p] = m < a.M;
        const int mm = a_ok[p] ? m : 0;
        if (DENSE) {
            a_off[p] = (size_t)mm * a.ldx;
            a_pix[p] = 3;
            if (a.tsm_T > 0) {
                const int t = (mm / a.tsm_hw) % a.tsm_T;
                a_pix[p] = (t > 0 ? 1 : 0) | (t < a.tsm_T - 1 ? 2 : 0);
            }
            a_iy[p] = a_ix[p] = 0;
        } else {
            const OutPix px = out_pixel(a, mm);
            a_pix[p] = px.img * a.H * a.W;
            a_iy[p] = px.oy * a.stride - a.pad;
            a_ix[p] = px.ox * a.stride - a.pad;
            a_off[p] = 0;
        }
    }
    const float* wrow[BP];
    bool b_ok[BP];
#pragma unroll
    for (int p = 0; p < BP; ++p) {
        const int n = n0 + lrow + RPP * p;
        b_ok[p] = n < a.N;
        wrow[p] = a.w + (size_t)(b_ok[p] ? n : 0) * a.K;
    }
    const size_t tsm_stride = (size_t)a.tsm_hw * a.ldx;

    f32x4 ra[AP], rb[BP];

    auto gload = [&](int kt) {
        const int kidx = kt * BK + lq * 4;
        const bool k_ok = kidx < a.K;
#pragma unroll
        for (int p = 0; p < BP; ++p)
        {
            // out-of-range chunks read a handle-owned block of zeros: no select on the loaded value,
            // so nothing forces the load to complete before the multiply phase
            rb[p] = *reinterpret_cast<const f32x4*>((b_ok[p] && k_ok) ? wrow[p] + kidx : a.zeros);
        }
        if (DENSE) {
            int need = 0;           // which neighbour frame this channel chunk reads (TSM)
            long long shift = 0;
            if (a.tsm_T > 0) {
                if (kidx < a.tsm_fold) { need = 2; shift = (long long)tsm_stride; }
                else if (kidx < 2 * a.tsm_fold) { need = 1; shift = -(long long)tsm_stride; }
            }
#pragma unroll
            for (int p = 0; p < AP; ++p) {
                const bool ok = a_ok[p] && k_ok && (need == 0 || (a_pix[p] & need));
                ra[p] = *reinterpret_cast<const f32x4*>(ok ? a.x + (long long)a_off[p] + shift + kidx : a.zeros);
            }
        } else {
            const int tap = kidx / a.cin;
            const int c = kidx - tap * a.cin;
            const int kh = tap / a.KW;
            const int kw = tap - kh * a.KW;
#pragma unroll
            for (int p = 0; p < AP; ++p) {
                const int iy = a_iy[p] + kh, ix = a_ix[p] + kw;
                const bool ok = a_ok[p] && k_ok && (unsigned)iy < (unsigned)a.H && (unsigned)ix < (unsigned)a.W;
                const size_t off = (size_t)(a_pix[p] + iy * a.W + ix) * a.ldx + c;
                ra[p] = *reinterpret_cast<const f32x4*>(ok ? a.x + off : a.zeros);
            }
        }
    };
    auto lstore = [&](int buf) {
        float* As = smem + buf * STAGE;
        float* Bs = As + BM * LDP;
#pragma unroll
        for (int p = 0; p < AP; ++p) *reinterpret_cast<f32x4*>(&As[(lrow + RPP * p) * LDP + lq * 4]) = ra[p];
#pragma unroll
        for (int p = 0; p < BP; ++p) *reinterpret_cast<f32x4*>(&Bs[(lrow + RPP * p) * LDP + lq * 4]) = rb[p];
    };

    f32x16 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    const int nk = (a.K + BK - 1) / BK;
    const int frag_row = lane & 31;
    const int frag_k = (lane >> 5) * 4;

    gload(0);
    lstore(0);
    __syncthreads();
    for (int kt = 0; kt < nk; ++kt) {
        const bool more = kt + 1 < nk;
        if (more) gload(kt + 1);
        __builtin_amdgcn_sched_barrier(0);  // keep the loads issued above, their use (ds_write) below the MFMAs
        const float* As = smem + (kt & 1) * STAGE + (wm * TM * 32 + frag_row) * LDP + frag_k;
        const float* Bs = smem + (kt & 1) * STAGE + BM * LDP + (wn * TN * 32 + frag_row) * LDP + frag_k;
        if (FLAGS & 1) __builtin_amdgcn_s_setprio(1);
#pragma unroll
        for (int kk = 0; kk < BK / 8; ++kk) {
            f32x4 af[TM], bf[TN];
#pragma unroll
            for (int i = 0; i < TM; ++i) af[i] = *reinterpret_cast<const f32x4*>(As + i * 32 * LDP + kk * 8);
#pragma unroll
            for (int j = 0; j < TN; ++j) bf[j] = *reinterpret_cast<const f32x4*>(Bs + j * 32 * LDP + kk * 8);
#pragma unroll
            for (int s4 = 0; s4 < 4; ++s4) mfma_step(acc, af, bf, s4);
        }
        if (FLAGS & 1) __builtin_amdgcn_s_setprio(0);
        __builtin_amdgcn_sched_barrier(0);
        if (more) lstore((kt + 1) & 1);
        __syncthreads();
    }

    conv_epilogue<TM, TN, ET>(a, smem, acc, m0, n0, wm, wn, lane, wave);
}


// =============================================================================================
// Direct-to-LDS variant (global_load_lds_dwordx4).  Measured on gfx950 (profiles/r1_conv_ablation.md):
// with VGPR staging the 8 global_load_dwordx4 + 8 ds_write_b128 a thread issues per k slice cost
// ~17 % of the MFMA time and are NOT hidden by the co-resident wave; the LDS-DMA form has no
// register round trip, no ds_write pass and (pointers advanced by a constant per slice) almost no
// address arithmetic.
//   - LDS image per operand: the unpadded, swizzled [rows][32 floats] slice image (slice_chunk above).
//   - requirements (checked by the launcher): 1x1/stride 1: K % 4 == 0 (a partial last slice is zero-filled);
//     other filters: cin % 32 == 0, KH*KW <= 32.
//   - 2 LDS stages; per slice: s_waitcnt vmcnt(0) ; s_barrier ; issue DMA for the next slice ; multiply.
// The kernel reads in four sections -- SET-UP (tile, position-major geometry), OPERAND SOURCE (per-lane state of each form, the
// per-slice walk `prep`, one DMA instruction `issue_one`), SCHEDULE (three K loops: the split tiles' production schedule, the
// barrier-2/3 variant, the paired-slice loop) and EPILOGUE -- and each flag is described at the part that implements it:
// PM at the set-up; LEAN, LEAN + SPECIAL and SPECIAL at the operand source; EMU / BSP and DT at the schedules.
template <int BM, int BN, int WGM, int WGN, bool DENSE, int PIPE, bool SPECIAL, int EMU, bool BSP = false, int DT = 0, bool PM = false,
          bool LEAN = false, bool POOL = false>
__global__ __launch_bounds__(64 * WGM * WGN, (BM == 128 && BN == 128 && WGM * WGN == 4) ? 2 : 1)   // 128x128: two blocks per CU
void conv_gemm_glds_kernel(const ConvArgs a) {
    static_assert(!POOL || (DENSE && !SPECIAL && ((LEAN && DT == 0) || (!LEAN && (DT == 4 || DT == 6)))),
                  "pooled epilogue: the lean dense fp32 kernel, or the dense fp16-operand kernel with fp32 features (DT 6: fp16 residual, rounded values)");
    static_assert(!PM || (!DENSE && (EMU == 0 || BSP) && PIPE == 1), "position-major tiles: k x k filters on the fp32 pipe, or split tiles with pre-split weights");
    static_assert(!LEAN || ((DENSE || PM) && PIPE == 1 && ((EMU == 0 && !BSP) || (EMU != 0 && BSP)) &&
                            (!SPECIAL || (DENSE && EMU == 0 && DT == 0 && !POOL))),
                  "lean K loop: plain fp32-pipe launches, split tiles with pre-split weights, or (LEAN + SPECIAL) the fp32 pipe's temporally shifted conv1");
    constexpr bool LTSM = LEAN && SPECIAL;
    constexpr int NW = WGM * WGN;
    constexpr int TM = BM / WGM / 32, TN = BN / WGN / 32;
    constexpr int AI = BM / (8 * NW);                                   // DMA instructions per wave per slice
    constexpr int BI = BSP ? (3 * BN / 16) / NW : BN / (8 * NW);
    constexpr int STAGE = BM * 32 + BN * (BSP ? 48 : 32);
    static_assert(!BSP || (EMU != 0 && (3 * BN / 16) % NW == 0), "pre-split weights: split tiles only");
    constexpr int SLAB = NW * 32 * (TN * 32 + 4);
    constexpr int POOLF = POOL ? BM * (BN + 4) : 0;                        // pooled epilogue: the activated tile, next to the slabs
    constexpr int SMEM = 2 * STAGE > SLAB + POOLF ? 2 * STAGE : SLAB + POOLF;
    static_assert(BM % (8 * NW) == 0 && BN % (8 * NW) == 0, "staging shape");
    __shared__ __attribute__((aligned(16))) float smem[SMEM];

    // ==== set-up: the wave's place in the block, the block's tile =======================================================================
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave / WGN, wn = wave % WGN;

    const int bid = xcd_tile(blockIdx.x, a.nblocks);
    const int tile_m = bid / a.tiles_n;
    const int tile_n = bid - tile_m * a.tiles_n;
    int m0 = tile_m * (POOL ? a.pool_rows : BM);      // (pooled epilogue: a tile holds whole images; its last BM - pool_rows rows repeat the next tile's)
    const int n0 = tile_n * BN;
    // PM (k x k filters, fp32 pipe): POSITION-MAJOR tiles with padding-tap skipping.  A tile's BM rows are the SAME output
    // pixel of BM consecutive images (instead of BM consecutive pixels), so every row has the same set of filter taps inside
    // the image and the taps that only multiply padding are skipped for the whole tile -- no DMA, no MFMA: on the 3x3 maps of
    // stage 4 the corner / edge / centre pixels use 4 / 6 / 9 of the 9 taps (5.4 on average: 40 % of the products of the
    // row-major form are zeros), on 6x6 maps 7.1, on 12x12 8.0.  A skipped slice contributes exact zeros, so the result is
    // BIT-IDENTICAL to the row-major kernel.  Tile t = (image group g = t / (OH*OW), pixel p = t % (OH*OW)).
    // position-major: this tile's pixel, its first image, and the taps inside the image (uniform over the tile)
    int pm_p = 0, pm_iy0 = 0, pm_ix0 = 0;
    unsigned pm_mask = 0;
    if (PM) {
        const OutPix px = out_pixel(a, tile_m);            // (image group, the tile's pixel)
        pm_p = px.rem;
        m0 = px.img * BM;                                  // first IMAGE of the tile
        pm_iy0 = px.oy * a.stride - a.pad;
        pm_ix0 = px.ox * a.stride - a.pad;
        for (int kh = 0; kh < a.KH; ++kh)
            for (int kw = 0; kw < a.KW; ++kw)
                if ((unsigned)(pm_iy0 + kh) < (unsigned)a.H && (unsigned)(pm_ix0 + kw) < (unsigned)a.W) pm_mask |= 1u << (kh * a.KW + kw);
    }
    // taps the K walk visits: the ones inside the image (pm_allow == 2, experiments: all of them, to separate the cost of
    // the position-major row order from the gain of the skipping)
    const unsigned pm_walk = (PM && a.pm_allow == 2) ? ((1u << (a.KH * a.KW)) - 1u) : pm_mask;

    // ==== operand source: per-lane state of each form, the per-slice walk, one DMA instruction ==========================================
    // LEAN (1x1/stride-1 launches without fix-ups, and position-major tiles): NO vector ALU work in the K loop.  On gfx950 the fp32
    // MFMA and the fp32/int VALU issue to the same lanes, so every v_add in the loop is a cycle the matrix pipe does not get
    // (DESIGN.md section 3.4).  The DMA is issued in its scalar-base form -- global_load_lds_dwordx4 voffset, s[base:base+1] --
    // with a per-lane 32-bit byte offset that never changes and a wave-uniform base the SALU advances per slice (the compiler
    // builtin only emits the 64-bit-VGPR-address form: one v_lshl_add_u64 per instruction per slice).  Rows past the end of the
    // problem read a valid row instead of the zero block (their outputs are discarded by the epilogue), so no select either.
    // LEAN + SPECIAL = the lean K loop for a conv1 with the fused temporal shift (K and the shifted fold multiples of 32, checked by the launcher):
    // the activations are DMA-ed with the RANGE-CHECKED buffer form (buffer_load_dwordx4 ... lds), which writes ZEROS to LDS for a lane whose
    // offset is out of range (tools/exp/buffer_load_lds_oob.hip) -- so the rows at clip ends get their zeros from a constant per-lane offset
    // instead of a per-lane source select per slice: three constant offsets per row (own frame, next frame, previous frame), a wave-uniform
    // choice per slice, the slice's position in the SGPR offset.
    // SPECIAL = the launch has a fused temporal shift or a K that is not a multiple of 32: only then does the DMA
    // issue path carry the per-slice source fix-ups (kept out of the common instantiation so the K loop is
    // straight-line code between the MFMA groups).
    const int lr = lane >> 3;   // row within the 8-row group
    const int ls = lane & 7;    // LDS chunk slot
    // The activation rows' per-lane state is declared by the form that uses it: a form that is off keeps ONE element, and every access sits
    // under its form's flag (compile-time constants, so the other forms' code is never emitted).  The forms: lean, lean + shift (LTSM), the
    // dense pointer walk, the tap gather (row-major and position-major).  The weight rows' state (lean: vb; otherwise pb / step_b / qb) is
    // filled for both forms by one loop, and dead-code elimination drops the unused half: guarded by form, that loop changes the lean kernels.
    constexpr bool WALK = !LEAN && DENSE, GATHER = !LEAN && !DENSE;
    constexpr int LA = LEAN ? AI : 1, SA = LTSM ? AI : 1, WA = WALK ? AI : 1, GA = GATHER ? AI : 1;
    // lean
    unsigned va[LA];            // constant per-lane byte offsets of the activation rows
    unsigned vb[BI];            // ... and of the weight rows
    unsigned vnx[SA], vpv[SA];  // + shift: the same row in the next / previous frame, or out of range at a clip end
    const float* lean_a = a.x;  // wave-uniform base of the activation rows (PM: moved to the tile's first tap)
    if (LEAN && PM) lean_a = a.x + ((long long)pm_iy0 * a.W + pm_ix0) * a.ldx;
    // dense pointer walk
    const float* pa[WA];        // running source pointer (or the zero block)
    int step_a[WA];             // pointer advance per slice (0 for the zero block)
    // tap gather
    long long boff[GA];         // element offset of (image, oy*s-pad, ox*s-pad, chunk)
    unsigned amask[GA];         // bit t set <=> filter tap t is inside the image for this row
    // dense pointer walk with a temporal shift
    int tflag[WA];              // bit0 has previous frame, bit1 has next frame, bit2 row valid
    // every form
    int qa[AI];                 // source chunk (swizzled) in floats
#pragma unroll
    for (int j = 0; j < AI; ++j) {
        const int row = (j * NW + wave) * 8 + lr;
        const int m = m0 + row;
        const bool ok = m < a.M;
        const int mm = ok ? m : 0;
        qa[j] = slice_chunk(row, ls) * 4;
        if (WALK) { pa[j] = a.zeros; step_a[j] = 0; tflag[j] = 0; }
        if (GATHER) { boff[j] = 0; amask[j] = 0; }
        if (LEAN) va[j] = 0;
        if (LEAN) {
            int r = PM ? (m < a.pm_images ? m : 0) : mm;
            if (DENSE && a.stride != 1) {       // 1x1 / stride s (the downsample convs): output pixel -> input pixel, still one row per row
                const OutPix px = out_pixel(a, mm);
                r = (px.img * a.H + px.oy * a.stride) * a.W + px.ox * a.stride;
            }
            if constexpr ((CG_ABL & 32) != 0) r &= 1023;      // ablation: the activation rows of every tile come from the same 1024 rows (L2-resident)
            va[j] = (unsigned)(((size_t)r * (PM ? (size_t)a.H * a.W : (size_t)1) * a.ldx + qa[j]) * 4);
            if constexpr (LTSM) {
                const int t = (mm / a.tsm_hw) % a.tsm_T;
                const unsigned sh = (unsigned)((size_t)a.tsm_hw * a.ldx * 4);
                vnx[j] = (ok && t < a.tsm_T - 1) ? va[j] + sh : 0x7ffffff0u;      // (out of range: the buffer form writes zeros)
                vpv[j] = (ok && t > 0) ? va[j] - sh : 0x7ffffff0u;
            }
        } else if (DENSE) {
            if (ok) { pa[j] = a.x + (size_t)mm * a.ldx + qa[j]; step_a[j] = 32; }
            if (a.tsm_T > 0) {
                const int t = (mm / a.tsm_hw) % a.tsm_T;
                tflag[j] = (ok ? 4 : 0) | (t > 0 ? 1 : 0) | (t < a.tsm_T - 1 ? 2 : 0);
            }
        } else if (PM) {
            const int img = m0 + row;                       // rows = images
            const bool iok = img < a.pm_images;
            boff[j] = ((long long)(iok ? img : 0) * a.H * a.W + (long long)pm_iy0 * a.W + pm_ix0) * a.ldx + qa[j];
            amask[j] = iok ? pm_mask : 0u;
        } else {
            const OutPix px = out_pixel(a, mm);
            const int iy0 = px.oy * a.stride - a.pad, ix0 = px.ox * a.stride - a.pad;
            boff[j] = ((long long)px.img * a.H * a.W + (long long)iy0 * a.W + ix0) * a.ldx + qa[j];
            unsigned mk = 0;
            for (int kh = 0; kh < a.KH; ++kh)
                for (int kw = 0; kw < a.KW; ++kw)
                    if (ok && (unsigned)(iy0 + kh) < (unsigned)a.H && (unsigned)(ix0 + kw) < (unsigned)a.W)
                        mk |= 1u << (kh * a.KW + kw);
            amask[j] = mk;
        }
    }
    // weight rows of every form but lean: pointer walk (the weight loop fills both forms' state: guarding it changes the lean kernels)
    const float* pb[BI];
    int step_b[BI];
    int qb[BI];                 // weight-row source chunk (swizzled) in floats
#pragma unroll
    for (int j = 0; j < BI; ++j) {
        if (BSP) {
            // instruction u = j*NW + wave fills LDS floats [u*256, u*256+256): plane u / (BN/16), rows 16*(u % (BN/16)) .. +15
            const int u = j * NW + wave;
            const int plane = u / (BN / 16), row = (u % (BN / 16)) * 16 + (lane >> 2);
            const int n = n0 + row;
            const int q = ((lane & 3) ^ ((row >> 2) & 3)) * 8;   // bf16 elements
            qb[j] = q;
            vb[j] = (unsigned)((((size_t)plane * a.N + (n < a.N ? n : 0)) * a.K + q) * 2);   // LEAN: byte offset inside the bf16 planes
            if (n < a.N) {
                pb[j] = reinterpret_cast<const float*>(a.wsp + ((size_t)plane * a.N + n) * a.K + q);
                step_b[j] = 16;   // 32 bf16 = 16 floats per slice
            } else { pb[j] = a.zeros; step_b[j] = 0; }
        } else {
            const int row = (j * NW + wave) * 8 + lr;
            const int n = n0 + row;
            const int q = slice_chunk(row, ls) * 4;
            qb[j] = q;
            vb[j] = (unsigned)(((size_t)(n < a.N ? n : 0) * a.K + q) * 4);
            if (n < a.N) { pb[j] = a.w + (size_t)n * a.K + q; step_b[j] = 32; }
            else { pb[j] = a.zeros; step_b[j] = 0; }
        }
    }
    const long long tsm_stride = (long long)a.tsm_hw * a.ldx;

    typedef const __attribute__((address_space(1))) void* gptr_t;
    typedef __attribute__((address_space(3))) void* lptr_t;

    // per-slice wave-uniform state of the NEXT slice's DMA (set by prep)
    bool nx_tsm = false, nx_tail = false;
    int ltsm_ty = -1;           // LTSM: kind of the slice whose offsets are in vcur (0 next frame, 1 previous frame, 2 own frame)
    unsigned vcur[SA];
    int nx_kt = 0, nx_tap = 0, nx_c0 = 0, nx_kh = 0, nx_kw = 0;
    int nx_koff = 0;            // PM: offset of the slice inside a filter row (taps are skipped, so it is not 32 * kt)
    long long nx_toff = 0;
    auto prep = [&](int kt) {
        nx_kt = kt;
        nx_tail = SPECIAL && DENSE && (kt + 1) * 32 > a.K;      // last, partial slice of a K that is not a multiple of 32
        if (DENSE) {
            nx_tsm = SPECIAL && a.tsm_T > 0 && kt * 32 < 2 * a.tsm_fold;
            if (LTSM) {
                // the slice's kind changes twice per tile (at the fold boundaries): the lane offsets in use are swapped there, under a real
                // branch, so the K loop carries no select
                const int ty = kt * 32 < a.tsm_fold ? 0 : nx_tsm ? 1 : 2;
                if (ty != ltsm_ty) {
                    asm volatile("");
                    ltsm_ty = ty;
#pragma unroll
                    for (int j = 0; j < AI; ++j) vcur[j] = ty == 0 ? vnx[j] : ty == 1 ? vpv[j] : va[j];
                }
            }
        } else {
            tap_walk_step<PM>(kt, a, pm_walk, nx_tap, nx_c0, nx_kh, nx_kw);
            nx_toff = ((long long)nx_kh * a.W + nx_kw) * a.ldx + nx_c0;
            if (PM) nx_koff = nx_tap * a.cin + nx_c0;
        }
    };
    // one DMA instruction: q < BI -> weight rows, else activation rows
    const unsigned smem_lds = (unsigned)(size_t)(lptr_t)smem;      // LDS byte address of the block's buffer
    auto lean_dma = [&](const float* sbase, unsigned voff, const float* lds) { lds_dma_sbase(sbase, voff, smem_lds + (unsigned)((lds - smem) * 4)); };
    auto issue_one = [&](int q, int buf) {
        if (LTSM && q >= BI) {
            // buffer_load_dwordx4 voffset, s[rsrc], soffset offen lds -- written out (the compiler's builtin for it makes the HOST pass drop
            // every stub of this template without a diagnostic).  Descriptor: base, stride 0, num_records = the tensor's bytes, raw 32-bit format.
            const unsigned l = (unsigned)__builtin_amdgcn_readfirstlane(smem_lds + (unsigned)((buf * STAGE + (wave + (q - BI) * NW) * 8 * 32) * 4));
            const unsigned soff = (unsigned)__builtin_amdgcn_readfirstlane(nx_kt * 128);
            const unsigned long long b = (unsigned long long)a.x;
            const u32x4 rs = {(unsigned)__builtin_amdgcn_readfirstlane((unsigned)b), (unsigned)__builtin_amdgcn_readfirstlane((unsigned)(b >> 32) & 0xffffu),
                              (unsigned)__builtin_amdgcn_readfirstlane((unsigned)((size_t)a.M * a.ldx * 4)), 0x00020000u};
            asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %2, %3 offen lds" ::"s"(l), "v"(vcur[q - BI]), "s"(rs), "s"(soff) : "memory", "m0");
            return;
        }
        if (LEAN) {
            if (q < BI)     // (pre-split weights: a slice is 32 bf16 = 16 floats of a plane row)
                lean_dma(BSP ? reinterpret_cast<const float*>(a.wsp) + (PM ? nx_koff >> 1 : nx_kt * 16) : a.w + (PM ? nx_koff : nx_kt * 32), vb[q],
                         smem + buf * STAGE + BM * 32 + (wave + q * NW) * 8 * 32);
            else
                lean_dma(PM ? lean_a + nx_toff : lean_a + nx_kt * 32, va[q - BI], smem + buf * STAGE + (wave + (q - BI) * NW) * 8 * 32);
            return;
        }
        if (q < BI) {
            float* Bs = smem + buf * STAGE + BM * 32 + wave * 8 * 32;   // 8 rows x 128 B = 16 rows x 64 B = 256 floats per instruction
            const float* srcb = pb[q];
            if (!BSP && SPECIAL && nx_tail && nx_kt * 32 + qb[q] >= a.K) srcb = a.zeros;
            if (PM) {
                if (step_b[q]) srcb += BSP ? (nx_koff >> 1) : nx_koff;         // (rows past N point at the zero block and stay there; bf16 planes: two k per float)
            } else
                pb[q] += step_b[q];
            __builtin_amdgcn_global_load_lds((gptr_t)srcb, (lptr_t)(Bs + q * NW * 8 * 32), 16, 0, 0);
            return;
        }
        const int j = q - BI;
        float* As = smem + buf * STAGE + wave * 8 * 32;
        const float* src;
        if (DENSE) {
            src = pa[j];
            if (SPECIAL && nx_tsm) {   // this slice holds shifted channels: pick the neighbour frame per chunk
                const int c = nx_kt * 32 + qa[j];
                if (c < a.tsm_fold) src = (tflag[j] & 2) ? src + tsm_stride : a.zeros;
                else if (c < 2 * a.tsm_fold) src = (tflag[j] & 1) ? src - tsm_stride : a.zeros;
                if (!(tflag[j] & 4)) src = a.zeros;
            }
            if (SPECIAL && nx_tail && nx_kt * 32 + qa[j] >= a.K) src = a.zeros;
            pa[j] += step_a[j];
        } else {
            src = ((amask[j] >> nx_tap) & 1u) ? a.x + boff[j] + nx_toff : a.zeros;
        }
        __builtin_amdgcn_global_load_lds((gptr_t)src, (lptr_t)(As + j * NW * 8 * 32), 16, 0, 0);
    };
    constexpr int NI = AI + BI;

    f32x16 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    // fragment read offsets: row (lane&31) of a 32-row band, chunk (2kk + lane>>5) ^ swizzle(row)
    const int sw = (lane >> 1) & 7;
    const int hb = ((lane >> 5) ^ sw) & 1;
    int foff[4];
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) foff[kk] = (lane & 31) * 32 + ((((2 * kk) ^ (sw & 6)) | hb) << 2);
    const int a_base = wm * TM * 32 * 32;
    const int b_base = BM * 32 + wn * TN * 32 * 32;
    // split form: k16 step j, lane half h reads chunks 4j + 2h and 4j + 2h + 1 (8 consecutive k of its row)
    int foffe[2][2];
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int e = 0; e < 2; ++e) foffe[j][e] = (lane & 31) * 32 + (((4 * j + 2 * (lane >> 5) + e) ^ sw) << 2);
    int foffb[2];   // pre-split weights: row (lane&31) of a 64-byte-row plane, chunk (2j + lane>>5) ^ ((row>>2)&3)
#pragma unroll
    for (int j = 0; j < 2; ++j) foffb[j] = (lane & 31) * 16 + ((((2 * j + (lane >> 5)) ^ ((lane >> 2) & 3)) & 3) << 2);

    // ==== schedule: one of three K loops ================================================================================================
    // EMU = 0: v_mfma_f32_32x32x2_f32 (the default, exact fp32 FMA chain).  EMU = 6 / 9: the fragments are split into
    // three bf16 parts after the LDS read and multiplied with 6 / 9 v_mfma_f32_32x32x16_bf16 per 16 k (see split3).
    // BSP (split tiles only): the weights come pre-split as three bf16 planes (ConvArgs::wsp); their LDS image is
    // [plane][BN rows][64 B] with the 16-byte chunk index XOR-ed with (row>>2)&3, and a fragment is one ds_read_b128.
    const int nk = PM ? __builtin_popcount(pm_walk) * (a.cin >> 5) : (a.K + 31) / 32;
    prep(0);
#pragma unroll
    for (int q = 0; q < NI; ++q) issue_one(q, 0);

    if constexpr (EMU != 0 && BSP) {
        // ---- schedule 1, the production schedule of the split tiles (EMU != 0, BSP): fragments always one k16 step ahead, ONE barrier per slice placed
        // between its two steps.  At the barrier T_k every wave has (a) read all of slice k out of LDS, (b) seen its own
        // DMA of slice k+1 land -- so after it buffer k&1 can take slice k+2 and slice k+1's first fragments can be read
        // while slice k's second step multiplies.
        constexpr int TA[9] = {2, 2, 1, 2, 0, 1, 1, 0, 0};   // (A part, B part) of the products, smallest first
        constexpr int TB[9] = {2, 1, 2, 0, 2, 1, 0, 1, 0};
        f32x4 ar[2][TM][2];        // raw fp32 activation fragments of a step (8 consecutive k per lane)
        u32x4 bq[2][3][TN];        // pre-split weight fragments [h, m, l]
        auto rd = [&](int sb, const float* St, int j2) {
#pragma unroll
            for (int i = 0; i < TM; ++i) {
                ar[sb][i][0] = *reinterpret_cast<const f32x4*>(St + a_base + i * 1024 + foffe[j2][0]);
                ar[sb][i][1] = *reinterpret_cast<const f32x4*>(St + a_base + i * 1024 + foffe[j2][1]);
            }
#pragma unroll
            for (int j = 0; j < TN; ++j)
#pragma unroll
                for (int pl = 0; pl < 3; ++pl)
                    bq[sb][pl][j] = *reinterpret_cast<const u32x4*>(St + BM * 32 + pl * BN * 16 + (wn * TN + j) * 32 * 16 + foffb[j2]);
        };
        auto mm = [&](int sb, auto dma_tag, int nbuf) {
            constexpr bool dma = decltype(dma_tag)::value;
            u32x4 ap[3][TM];
#pragma unroll
            for (int i = 0; i < TM; ++i) {
                if constexpr (CG_ABL & 1) {
                    ap[0][i] = __builtin_bit_cast(u32x4, ar[sb][i][0]); ap[1][i] = __builtin_bit_cast(u32x4, ar[sb][i][1]); ap[2][i] = ap[0][i];
                } else
                    split3(ar[sb][i][0], ar[sb][i][1], ap[0][i], ap[1][i], ap[2][i]);
            }
#pragma unroll
            for (int t = 9 - EMU; t < 9; ++t) {
#pragma unroll
                for (int i = 0; i < TM; ++i)
#pragma unroll
                    for (int j = 0; j < TN; ++j) {
                        if constexpr (CG_ABL & 16) {
                            if (t == 8) acc[i][j][0] += __uint_as_float(ap[TA[t]][i].x ^ bq[sb][TB[t]][j].x);
                        } else
                            acc[i][j] = mfma_bf16(ap[TA[t]][i], bq[sb][TB[t]][j], acc[i][j]);
                    }
                if (dma && !(CG_ABL & 4)) {
                    const int g = t - (9 - EMU);
#pragma unroll
                    for (int q = 0; q < NI; ++q)
                        if ((q * EMU) / NI == g) issue_one(q, nbuf);
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
        };
        if (nk > 1) {
            prep(1);
#pragma unroll
            for (int q = 0; q < NI; ++q) issue_one(q, 1);
            asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NI) : "memory");   // slice 0 landed, slice 1 still in flight
        } else {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
        __builtin_amdgcn_s_barrier();
        rd(0, smem, 0);
        auto body = [&](int k, auto has1_tag, auto has2_tag) {
            constexpr bool has1 = decltype(has1_tag)::value, has2 = decltype(has2_tag)::value;
            const float* St = smem + (k & 1) * STAGE;
            rd(1, St, 1);
            __builtin_amdgcn_sched_barrier(0);
            mm(0, std::false_type{}, 0);
            __builtin_amdgcn_sched_barrier(0);
            if (has1) {
                if constexpr (CG_ABL & 2) asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                else asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");   // own DMA of slice k+1 landed, own reads of slice k done
                __builtin_amdgcn_s_barrier();                                   // T_k
                rd(0, smem + ((k + 1) & 1) * STAGE, 0);
                if (has2) prep(k + 2);
            }
            __builtin_amdgcn_sched_barrier(0);
            mm(1, has2_tag, k & 1);
        };
        int k = 0;
        for (; k + 2 < nk; ++k) body(k, std::true_type{}, std::true_type{});
        if (nk > 1) { body(k, std::true_type{}, std::false_type{}); ++k; }
        body(k, std::false_type{}, std::false_type{});
        __syncthreads();
        if constexpr (CG_ABL & 8) {
            float sacc = 0.f;
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j)
#pragma unroll
                    for (int r = 0; r < 16; ++r) sacc += acc[i][j][r];
            if (sacc == 12345.678f) a.out[0] = sacc;
            return;
        }
        if (PM) conv_epilogue<TM, TN>(a, smem, acc, m0, n0, wm, wn, lane, wave, a.OH * a.OW, pm_p, a.pm_images);
        else conv_epilogue<TM, TN>(a, smem, acc, m0, n0, wm, wn, lane, wave);
        return;
    }

    if constexpr (EMU == 0 && PIPE == 2) {
        // ---- schedule 2, the fp32 pipe with the barrier between steps 2 and 3 of a slice (PIPE == 2; measured variant): at T_k every wave has read all of slice k (step 3's
        // fragments were fetched during step 2) and seen its DMA of slice k+1 land, so step 3 multiplies while the first
        // fragments of slice k+1 are already being read -- no LDS latency is exposed behind a barrier.  DMA of slice k+2:
        // first half during step 3 of slice k, second half during step 0 of slice k+1.
        constexpr int QH = NI / 2;
        f32x4 af[2][TM], bf[2][TN];
        auto rdf = [&](int pb_, const float* St, int kk) {
#pragma unroll
            for (int i = 0; i < TM; ++i) af[pb_][i] = *reinterpret_cast<const f32x4*>(St + a_base + i * 1024 + foff[kk]);
#pragma unroll
            for (int j = 0; j < TN; ++j) bf[pb_][j] = *reinterpret_cast<const f32x4*>(St + b_base + j * 1024 + foff[kk]);
        };
        auto mul = [&](int cb, auto dma_tag, int qlo, int qhi, int nbuf) {
            constexpr bool dma = decltype(dma_tag)::value;
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int s4 = 0; s4 < 4; ++s4) {
                mfma_step(acc, af[cb], bf[cb], s4);
                if (dma) {
#pragma unroll
                    for (int q = 0; q < NI; ++q)
                        if (q >= qlo && q < qhi && ((q - qlo) * 4) / (qhi - qlo) == s4) issue_one(q, nbuf);
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
        };
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        if (nk > 1) {
            prep(1);
#pragma unroll
            for (int q = 0; q < QH; ++q) issue_one(q, 1);
        }
        rdf(0, smem, 0);
        auto body = [&](int k, auto has1_tag, auto has2_tag) {
            constexpr bool has1 = decltype(has1_tag)::value, has2 = decltype(has2_tag)::value;
            const float* St = smem + (k & 1) * STAGE;
            const int nb1 = (k + 1) & 1;
            rdf(1, St, 1);
            mul(0, has1_tag, QH, NI, nb1);          // second half of the DMA of slice k+1
            rdf(0, St, 2);
            mul(1, std::false_type{}, 0, 0, 0);
            rdf(1, St, 3);
            mul(0, std::false_type{}, 0, 0, 0);
            if (has1) {
                asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
                __builtin_amdgcn_s_barrier();         // T_k
                if (has2) prep(k + 2);
                rdf(0, smem + nb1 * STAGE, 0);
            }
            mul(1, has2_tag, 0, QH, k & 1);         // first half of the DMA of slice k+2
        };
        int k = 0;
        for (; k + 2 < nk; ++k) body(k, std::true_type{}, std::true_type{});
        if (nk > 1) { body(k, std::true_type{}, std::false_type{}); ++k; }
        body(k, std::false_type{}, std::false_type{});
        __syncthreads();
        conv_epilogue<TM, TN>(a, smem, acc, m0, n0, wm, wn, lane, wave);
        return;
    }

    // ---- schedule 3, the paired-slice loop (every other form: fp32, fp16 operands, splits on the fly).  PIPE = 0: the next slice's DMA at the
    // top of a slice (kept for A/B), PIPE = 1: between the MFMA groups.
    // DT (half-precision STORAGE, N2 / BASELINE config 5): bit 0 = fp16 output, bit 1 = fp16 residual, bit 2 = fp16 operands
    // (x and w): a k slice is then 64 halfs -- the same 128 bytes per row, so the DMA, the LDS image and its swizzle are
    // byte-identical and the loader simply counts in 32-bit words (the launcher halves K / cin / ldx); a lane's 16-byte
    // fragment is exactly the 8 halfs one v_mfma_f32_32x32x16_f16 wants (lanes 0-31: k 0..7, lanes 32-63: k 8..15 of a
    // 16-k step = chunk 2 kk + (lane >> 5), the f32 mapping).  Accumulation, BN and activation stay fp32.
    // (Bit 2 is the (DT & 4) branch of the slice below; bits 0 and 1 go to the epilogue as its ET.)
    // The K loop runs in pairs of slices so that the stage a slice reads is a compile-time constant: the fragment reads are
    // then ds_read_b128 at (loop-invariant VGPR) + immediate, with no address arithmetic per slice
    auto slice = [&](int kt, auto more_tag, auto stage_tag) {
        constexpr bool more = decltype(more_tag)::value;   // compile time: the last slice issues nothing
        constexpr int stage = decltype(stage_tag)::value;
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // this wave's DMA for slice kt has landed
        __builtin_amdgcn_s_barrier();                        // ... everyone's has, and slice kt-1 is consumed
        constexpr int nbuf = stage ^ 1;
        if (more) prep(kt + 1);
        const float* St = smem + stage * STAGE;
        if (!PIPE) {
            if (more) {
#pragma unroll
                for (int q = 0; q < NI; ++q) issue_one(q, nbuf);
            }
        }
        if constexpr (EMU != 0) {
#pragma unroll
            for (int j2 = 0; j2 < 2; ++j2) {
                u32x4 ap[3][TM], bp[3][TN];   // [h, m, l]
#pragma unroll
                for (int i = 0; i < TM; ++i)
                    split3(*reinterpret_cast<const f32x4*>(St + a_base + i * 1024 + foffe[j2][0]),
                           *reinterpret_cast<const f32x4*>(St + a_base + i * 1024 + foffe[j2][1]), ap[0][i], ap[1][i], ap[2][i]);
#pragma unroll
                for (int j = 0; j < TN; ++j) {
                    if (BSP) {
#pragma unroll
                        for (int pl = 0; pl < 3; ++pl)
                            bp[pl][j] = *reinterpret_cast<const u32x4*>(St + BM * 32 + pl * BN * 16 + (wn * TN + j) * 32 * 16 + foffb[j2]);
                    } else {
                        split3(*reinterpret_cast<const f32x4*>(St + b_base + j * 1024 + foffe[j2][0]),
                               *reinterpret_cast<const f32x4*>(St + b_base + j * 1024 + foffe[j2][1]), bp[0][j], bp[1][j], bp[2][j]);
                    }
                }
                if (PIPE) __builtin_amdgcn_sched_barrier(0);
                // smallest terms first; (A part, B part)
                constexpr int TA[9] = {2, 2, 1, 2, 0, 1, 1, 0, 0};
                constexpr int TB[9] = {2, 1, 2, 0, 2, 1, 0, 1, 0};
#pragma unroll
                for (int t = 9 - EMU; t < 9; ++t) {
#pragma unroll
                    for (int i = 0; i < TM; ++i)
#pragma unroll
                        for (int j = 0; j < TN; ++j) acc[i][j] = mfma_bf16(ap[TA[t]][i], bp[TB[t]][j], acc[i][j]);
                    const int g = j2 * EMU + (t - (9 - EMU));   // MFMA group index within the slice
                    if (PIPE && g < 8) {
                        if (more) {
#pragma unroll
                            for (int q = 0; q < NI; ++q)
                                if ((q * 8) / NI == g) issue_one(q, nbuf);
                        }
                        __builtin_amdgcn_sched_barrier(0);
                    }
                }
            }
            return;
        }
        f32x4 af[2][TM], bf[2][TN];
#pragma unroll
        for (int i = 0; i < TM; ++i) af[0][i] = *reinterpret_cast<const f32x4*>(St + a_base + i * 1024 + foff[0]);
#pragma unroll
        for (int j = 0; j < TN; ++j) bf[0][j] = *reinterpret_cast<const f32x4*>(St + b_base + j * 1024 + foff[0]);
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) {
            const int cb = kk & 1, nb = cb ^ 1;
            if (kk < 3) {   // next fragments are in flight while this step multiplies
#pragma unroll
                for (int i = 0; i < TM; ++i) af[nb][i] = *reinterpret_cast<const f32x4*>(St + a_base + i * 1024 + foff[kk + 1]);
#pragma unroll
                for (int j = 0; j < TN; ++j) bf[nb][j] = *reinterpret_cast<const f32x4*>(St + b_base + j * 1024 + foff[kk + 1]);
            }
            if (PIPE) __builtin_amdgcn_sched_barrier(0);
            if constexpr ((DT & 4) != 0) {
                // fp16 operands: one 32x32x16 MFMA per tile pair and 16-k step; the slice's DMA follows in four groups
#pragma unroll
                for (int i = 0; i < TM; ++i)
#pragma unroll
                    for (int j = 0; j < TN; ++j)
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, af[cb][i]),
                                                                            __builtin_bit_cast(f16x8, bf[cb][j]), acc[i][j], 0, 0, 0);
                if (PIPE) {
                    if (more) {
#pragma unroll
                        for (int q = 0; q < NI; ++q)
                            if ((q * 4) / NI == kk) issue_one(q, nbuf);
                    }
                    __builtin_amdgcn_sched_barrier(0);
                }
            } else {
#pragma unroll
            for (int s4 = 0; s4 < 4; ++s4) {
                mfma_step(acc, af[cb], bf[cb], s4);
                if (PIPE && s4 < 2) {
                    // the DMA for the next slice is issued in the shadow of the MFMAs just queued: slot = 2*kk + s4
                    if (more) {
#pragma unroll
                        for (int q = 0; q < NI; ++q)
                            if ((q * 8) / NI == 2 * kk + s4) issue_one(q, nbuf);
                    }
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
            }
        }
    };
    {
        using S0 = std::integral_constant<int, 0>;
        using S1 = std::integral_constant<int, 1>;
        int kt = 0;
        for (; kt + 2 < nk; kt += 2) {
            slice(kt, std::true_type{}, S0{});
            slice(kt + 1, std::true_type{}, S1{});
        }
        if (nk - kt == 2) {
            slice(kt, std::true_type{}, S0{});
            slice(kt + 1, std::false_type{}, S1{});
        } else {
            slice(kt, std::false_type{}, S0{});
        }
    }
    // ==== epilogue ======================================================================================================================
    __syncthreads();   // all fragment reads done before the slabs overwrite the stage buffers
    if constexpr (POOL) {
        conv_epilogue_pool<TM, TN, BM, BN, NW, DT == 4, DT == 6>(a, smem, acc, m0, n0, wm, wn, lane, wave, tile_m);
        return;
    }
    if (PM) conv_epilogue<TM, TN, (DT & 3)>(a, smem, acc, m0, n0, wm, wn, lane, wave, a.OH * a.OW, pm_p, a.pm_images);
    else conv_epilogue<TM, TN, (DT & 3)>(a, smem, acc, m0, n0, wm, wn, lane, wave);
}

// =============================================================================================
// Fused bottleneck tail for the 64-plane stage (ACT/models/resnet.py:94-114, layer1):
//     conv2 3x3 (64 -> 64) + BN + ReLU  ->  conv3 1x1 (64 -> 256) + BN + identity + ReLU  [->  next block's conv1 1x1 + BN + ReLU]
// in ONE launch per 128-pixel tile.  Unfused, these layers are HBM-bound: conv3 reads a 151 MB map to write a 604 MB one
// (14 FLOP/B against a machine balance of ~25), and the next conv1 reads the 604 MB straight back.  Here
//   phase 1  the 3x3 implicit GEMM (K = 576) exactly as conv_gemm_glds_kernel<128,64> runs it (same DMA, swizzle, k order);
//   mid      BN + ReLU on the accumulators, written to LDS in the A-operand image a DMA would have produced (the stage
//            buffers are dead by then and are reused), every wave then keeps its 32-row band's fragments in registers;
//   phase 2  conv3 in 8 passes of 32 output channels: W3 rows arrive by DMA, 32 MFMAs per wave, epilogue with the
//            16-byte residual loads / output stores of conv_epilogue; the finished (post-ReLU) values also go to LDS as
//            the A operand (one k slice) of
//   phase 3  the next block's conv1: out1[128 x N1] += chunk[128 x 32] * W1n[:, 32 pass .. +32]^T, accumulated across
//            the passes in registers -- conv3's output is consumed on chip while it is being written to HBM once.
// Every product keeps the k order of the unfused kernels, so the results are BIT-IDENTICAL to the three separate
// launches (tests: test_resnet50_fused_launches_bit_identical).  Three blocks fit a CU for N1 = 0 / 64 (48 KB of LDS: the
// phase-2 image is exactly the phase-1 ring, the epilogue's transposition slab lives in the dead half of the A2 image), two
// for N1 = 128 (56 KB), so one block's HBM-heavy phase 2 overlaps the others' MFMA-heavy phase 1.  A next conv1 that carries the fused
// temporal shift rides along in the position-major form when clips divide the 128-image tiles (round 6): a tile's rows are the same pixel of 128
// CONSECUTIVE frames, so the shifted channels of row r are rows r + 1 / r - 1 of the SAME chunk image (zeros at clip ends, which then include the
// tile's first and last row) -- phase 3 reads them with a row offset.  Clip lengths that do not divide 128 take the largest multiple below it as
// the tile group (120 images for T = 12: eight idle rows per tile).  Row-major tiles: N1 = 0.
struct FusedTailArgs {
    ConvArgs c2;          // the 3x3 conv (x, w, scale, bias, geometry; N = 64, K = 9 * 64)
    const float* w3;      // [n3][64]
    const float* s3;
    const float* b3;
    const float* res;     // identity / downsample branch [M][ldr]
    float* out;           // [M][n3]
    int n3, ldr;
    const float* w1n;     // [N1][n3] or nullptr
    const float* s1n;
    const float* b1n;
    float* out1;          // [M][N1]
    int act1n;
    int tsm_T1;           // > 0: the next conv1 carries the fused temporal shift over clips of tsm_T1 frames (PM tiles only, 128 % tsm_T1 == 0)
    int pm_gstride;       // position-major form: images per tile group (128; fewer when a shifted next conv1 needs whole clips per tile: the rows above idle)
    int tsm_np1;          // conv3 passes (32 channels each) per shifted fold: passes [0, np1) read the NEXT frame's rows, [np1, 2 np1) the previous frame's
};

// PM: position-major tiles (the 128 rows of a tile are one output pixel of 128 consecutive images): the 3x3 gather then has
// no per-row tap masks -- scalar-base DMA, no VALU in the K loop -- and skips the taps that only multiply padding, exactly as
// the stand-alone position-major conv kernel does (bit-identical).  Everything after phase 1 addresses its rows through the
// row map (tile row r -> output row (m0 + r) * rstride + roff), so the two forms share phases 2 and 3.
template <int N1, bool PM>
__global__ __launch_bounds__(256, N1 == 128 ? 2 : 3) void conv_fused_tail_kernel(const FusedTailArgs fa) {
    constexpr int BM = 128, BN = 64, NW = 4, WGN = 2;
    constexpr int TM = 2, TN = 1;
    constexpr int AI = BM / (8 * NW), BI = BN / (8 * NW), NI = AI + BI;
    constexpr int STAGE = BM * 32 + BN * 32;             // floats
    constexpr int XREG = 2 * STAGE;                      // phase-1 stage ring; phase 2: A2 / chunk image + weight chunks
    constexpr int PW = 32;                               // conv3 output channels per pass
    constexpr int TN1 = N1 / 64;                         // phase-3 wave tile: 64 rows x (N1 / 2) columns
    // phase-2 image of the ring region: stage 0 -- idle during the LAST phase-1 slice, so the first chunks are requested a
    // whole slice early -- holds the W3 chunk buffer(s) and the W1n chunk; then the [2][128][32] A2 image (its first slice
    // doubles as the conv3-output chunk image)
    constexpr int W3OFF = 0;
    // two W3 chunk buffers only when there is no W1n chunk to make room for: the N1 = 0 / 64 forms then need exactly the 48 KB
    // of the phase-1 ring and THREE blocks fit a CU (the N1 = 128 form: 56 KB, two)
    constexpr bool W3DB = N1 == 0;
    constexpr int W1OFF = (W3DB ? 2 : 1) * 2 * PW * 32;
    constexpr int A2OFF = W1OFF + N1 * 32;
    constexpr int XUSED = A2OFF + 2 * BM * 32;
    static_assert(A2OFF <= BM * 32 + BN * 32, "the weight chunk buffers must fit stage 0");
    constexpr int XSZ = XUSED > XREG ? XUSED : XREG;
    // the conv3 epilogue's transposition slab is the SECOND slice of the A2 image: every wave has its band's fragments in
    // registers by then, and only the first slice lives on as the chunk image (pitch 32, 16-byte chunks XOR-ed with row & 7)
    constexpr int SLAB = 0;
    __shared__ __attribute__((aligned(16))) float smem[XSZ + SLAB];
    const ConvArgs& a = fa.c2;

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave / WGN, wn = wave % WGN;

    const int bid = xcd_tile(blockIdx.x, a.nblocks);
    // row map of the tile
    int m0 = bid * BM, rstride = 1, roff = 0, rlimit = a.M;
    int pm_iy0 = 0, pm_ix0 = 0;
    unsigned pm_mask = 0;
    if (PM) {   // group-major order, as in conv_gemm_glds_kernel: an XCD's consecutive tiles are the pixels of the same images
        const OutPix px = out_pixel(a, bid);
        roff = px.rem;
        m0 = px.img * fa.pm_gstride;                  // (128, or the largest multiple of the clip length below it: clips never straddle tiles)
        rstride = a.OH * a.OW;
        rlimit = a.pm_images < m0 + fa.pm_gstride ? a.pm_images : m0 + fa.pm_gstride;
        pm_iy0 = px.oy * a.stride - a.pad;
        pm_ix0 = px.ox * a.stride - a.pad;
        for (int kh = 0; kh < a.KH; ++kh)
            for (int kw = 0; kw < a.KW; ++kw)
                if ((unsigned)(pm_iy0 + kh) < (unsigned)a.H && (unsigned)(pm_ix0 + kw) < (unsigned)a.W) pm_mask |= 1u << (kh * a.KW + kw);
    }

    typedef const __attribute__((address_space(1))) void* gptr_t;
    typedef __attribute__((address_space(3))) void* lptr_t;
    typedef __attribute__((address_space(1))) char gchar;
    typedef __attribute__((address_space(1))) f32x4 gf32x4;
    const unsigned smem_lds = (unsigned)(size_t)(lptr_t)smem;
    auto lean_dma = [&](const float* sbase, unsigned voff, const float* lds) { lds_dma_sbase(sbase, voff, smem_lds + (unsigned)((lds - smem) * 4)); };

    // ---- phase 1: 3x3 implicit GEMM, tile 128 x 64, K = KH*KW*64 ------------------------------------------
    const int lr = lane >> 3, ls = lane & 7;
    long long boff[AI];
    unsigned amask[AI];
    unsigned va[AI], vb[BI];
    const float* lean_a = a.x + ((long long)pm_iy0 * a.W + pm_ix0) * a.ldx;
#pragma unroll
    for (int j = 0; j < AI; ++j) {
        const int row = (j * NW + wave) * 8 + lr;
        const int m = m0 + row;
        const int qa = (ls ^ ((row >> 1) & 7)) * 4;
        boff[j] = 0; amask[j] = 0; va[j] = 0;
        if (PM) {
            va[j] = (unsigned)(((size_t)(m < rlimit ? m : 0) * a.H * a.W * a.ldx + qa) * 4);
        } else {
            const bool ok = m < a.M;
            const int mm = ok ? m : 0;
            const OutPix px = out_pixel(a, mm);
            const int iy0 = px.oy * a.stride - a.pad, ix0 = px.ox * a.stride - a.pad;
            boff[j] = ((long long)px.img * a.H * a.W + (long long)iy0 * a.W + ix0) * a.ldx + qa;
            unsigned mk = 0;
            for (int kh = 0; kh < a.KH; ++kh)
                for (int kw = 0; kw < a.KW; ++kw)
                    if (ok && (unsigned)(iy0 + kh) < (unsigned)a.H && (unsigned)(ix0 + kw) < (unsigned)a.W) mk |= 1u << (kh * a.KW + kw);
            amask[j] = mk;
        }
    }
#pragma unroll
    for (int j = 0; j < BI; ++j) {
        const int row = (j * NW + wave) * 8 + lr;           // BN = 64 = a.N: always a valid filter
        vb[j] = (unsigned)(((size_t)row * a.K + (ls ^ ((row >> 1) & 7)) * 4) * 4);
    }
    int nx_tap = 0, nx_c0 = 0, nx_kh = 0, nx_kw = 0, nx_koff = 0;
    long long nx_toff = 0;
    auto prep = [&](int kt) {
        tap_walk_step<PM>(kt, a, pm_mask, nx_tap, nx_c0, nx_kh, nx_kw);
        nx_toff = ((long long)nx_kh * a.W + nx_kw) * a.ldx + nx_c0;
        nx_koff = nx_tap * a.cin + nx_c0;
    };
    auto issue_one = [&](int q, int buf) {
        if (q < BI) {
            lean_dma(a.w + nx_koff, vb[q], smem + buf * STAGE + BM * 32 + (wave + q * NW) * 8 * 32);
            return;
        }
        const int j = q - BI;
        float* As = smem + buf * STAGE + (wave + j * NW) * 8 * 32;
        if (PM) {
            lean_dma(lean_a + nx_toff, va[j], As);
        } else {
            const float* src = ((amask[j] >> nx_tap) & 1u) ? a.x + boff[j] + nx_toff : a.zeros;
            __builtin_amdgcn_global_load_lds((gptr_t)src, (lptr_t)As, 16, 0, 0);
        }
    };

    f32x16 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[i][0][r] = 0.f;

    const int sw = (lane >> 1) & 7;
    const int hb = ((lane >> 5) ^ sw) & 1;
    int foff[4];
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) foff[kk] = (lane & 31) * 32 + ((((2 * kk) ^ (sw & 6)) | hb) << 2);
    const int a_base = wm * TM * 32 * 32;
    const int b_base = BM * 32 + wn * TN * 32 * 32;

    // ---- phase-2 helpers (declared here: the first weight chunks and residual rows are requested during phase 1)
    float* A2 = smem + A2OFF;               // [2 slices][128 rows][32], chunk index XOR-ed with (row>>1)&7
    float* W3s = smem + W3OFF;              // [2 buffers][2 slices][32 rows][32]
    float* W1s = smem + W1OFF;              // [N1 rows][32]
    float* slab = smem + A2OFF + BM * 32 + wave * 32 * 32;
    const bool full = m0 + BM <= rlimit;    // every lane stores in every pass: the counted waits below are exact
    const int c4 = lane & 7, rsub = lane >> 3;               // epilogue: 8 chunks of 4 channels per row, 8 rows per instruction
    // instruction u = j*4 + wave of a W3 chunk: slice u / 4, rows (u % 4) * 8 + lr.  Lane offsets are constants; the
    // chunk (np) moves the scalar base.
    unsigned v3[2], v1[N1 ? N1 / 32 : 1];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int u = j * NW + wave;
        const int sl = u >> 2, row = (u & 3) * 8 + lr;
        v3[j] = (unsigned)((row * 64 + sl * 32 + ((ls ^ ((row >> 1) & 7)) << 2)) * 4);
    }
#pragma unroll
    for (int j = 0; j < (N1 ? N1 / 32 : 1); ++j) {
        const int row = (j * NW + wave) * 8 + lr;
        v1[j] = (unsigned)(((size_t)row * fa.n3 + ((ls ^ ((row >> 1) & 7)) << 2)) * 4);
    }
    auto issue_w3 = [&](int np) {
#pragma unroll
        for (int j = 0; j < 2; ++j)
            lean_dma(fa.w3 + (size_t)np * PW * 64, v3[j], W3s + (W3DB ? (np & 1) * 2048 : 0) + (j * NW + wave) * 256);
    };
    auto issue_w1 = [&](int np) {
        if (N1 == 0) return;
#pragma unroll
        for (int j = 0; j < (N1 ? N1 / 32 : 1); ++j) lean_dma(fa.w1n + np * PW, v1[j], W1s + (j * NW + wave) * 256);
    };
    // identity rows in / output rows out: scalar row bases (one per 8-row step u of the wave's band) + constant lane offsets
    const unsigned vres = (unsigned)(((size_t)rsub * rstride * fa.ldr + 4 * c4) * 4);
    const unsigned vout = (unsigned)(((size_t)rsub * rstride * fa.n3 + 4 * c4) * 4);
    unsigned long long rbase[4], obase[4];
    bool row_ok[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const size_t grow = (size_t)(m0 + wave * 32 + u * 8) * rstride + roff;
        rbase[u] = pin_sgpr((unsigned long long)fa.res + grow * fa.ldr * 4);
        obase[u] = pin_sgpr((unsigned long long)fa.out + grow * fa.n3 * 4);
        row_ok[u] = m0 + wave * 32 + u * 8 + rsub < rlimit;
    }
    f32x4 rv[4];                             // identity rows of the coming conv3 pass (requested one pass ahead)
    auto load_res = [&](int np) {
        const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const gf32x4* src = reinterpret_cast<const gf32x4*>(reinterpret_cast<const gchar*>(rbase[u] + (unsigned long long)np * PW * 4) + vres);
            if (full) rv[u] = *src;
            else rv[u] = row_ok[u] ? *src : zero4;
        }
    };

    const int nk = PM ? __builtin_popcount(pm_mask) * (a.cin >> 5) : a.K / 32;     // even: cin = 64 -> two slices per tap
    prep(0);
#pragma unroll
    for (int q = 0; q < NI; ++q) issue_one(q, 0);
    auto slice = [&](int kt, auto more_tag, auto stage_tag) {
        constexpr bool more = decltype(more_tag)::value;
        constexpr int stage = decltype(stage_tag)::value;
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        constexpr int nbuf = stage ^ 1;
        if (more) prep(kt + 1);
        else {   // last slice (odd index: it reads stage 1): stage 0 is idle -> first conv3 weight chunk + identity rows
            issue_w3(0);
            issue_w1(0);
            load_res(0);
        }
        const float* St = smem + stage * STAGE;
        f32x4 af[2][TM], bf[2][TN];
#pragma unroll
        for (int i = 0; i < TM; ++i) af[0][i] = *reinterpret_cast<const f32x4*>(St + a_base + i * 1024 + foff[0]);
        bf[0][0] = *reinterpret_cast<const f32x4*>(St + b_base + foff[0]);
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) {
            const int cb = kk & 1, nb = cb ^ 1;
            if (kk < 3) {
#pragma unroll
                for (int i = 0; i < TM; ++i) af[nb][i] = *reinterpret_cast<const f32x4*>(St + a_base + i * 1024 + foff[kk + 1]);
                bf[nb][0] = *reinterpret_cast<const f32x4*>(St + b_base + foff[kk + 1]);
            }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int s4 = 0; s4 < 4; ++s4) {
                mfma_step(acc, af[cb], bf[cb], s4);
                if (s4 < 2) {
                    if (more) {
#pragma unroll
                        for (int q = 0; q < NI; ++q)
                            if ((q * 8) / NI == 2 * kk + s4) issue_one(q, nbuf);
                    }
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
        }
    };
    {
        using S0 = std::integral_constant<int, 0>;
        using S1 = std::integral_constant<int, 1>;
        int kt = 0;
        for (; kt + 2 < nk; kt += 2) {
            slice(kt, std::true_type{}, S0{});
            slice(kt + 1, std::true_type{}, S1{});
        }
        slice(kt, std::true_type{}, S0{});
        slice(kt + 1, std::false_type{}, S1{});
    }
    __syncthreads();      // every wave is done with the stage ring: it becomes the phase-2 workspace

    // ---- phase 2 set-up: BN + ReLU of conv2 into the A image (the first weight chunks are already on their way)
    {
        const int k = wn * 32 + (lane & 31);                 // conv2 output channel = conv3's k index
        const float sc = a.scale ? a.scale[k] : 1.f, bi = a.bias ? a.bias[k] : 0.f;
        const int kc = (lane & 31) >> 2, ke = lane & 3;
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = wm * 64 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
                A2[wn * (BM * 32) + row * 32 + (slice_chunk(row, kc) << 2) + ke] = fmaxf(fmaf(acc[i][0][r], sc, bi) + 0.f, 0.f);
            }
    }
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    // this wave's 32-row band of the conv3 A operand, K = 64: 8 fragments stay in registers for all passes
    f32x4 af2[2][4];
#pragma unroll
    for (int sl = 0; sl < 2; ++sl)
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) af2[sl][kk] = *reinterpret_cast<const f32x4*>(A2 + sl * (BM * 32) + wave * 1024 + foff[kk]);
    // (a wave rewrites only its own band of the image in the epilogue below, after these reads: no barrier needed)

    f32x16 acc1[TM][TN1 ? TN1 : 1];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < (TN1 ? TN1 : 1); ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc1[i][j][r] = 0.f;

    const int npass = fa.n3 / PW;
    const int crow = 4 * (lane >> 5);
    for (int np = 0; np < npass; ++np) {
        // the other W3 buffer was last read in pass np-1, two barriers ago: its refill rides under this pass
        if (W3DB && np + 1 < npass) issue_w3(np + 1);
        // ---- conv3, 32 output channels: [32 x 64] band x [64 x 32]
        f32x16 acc3;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc3[r] = 0.f;
        const float* W3c = W3s + (W3DB ? (np & 1) * 2048 : 0);
#pragma unroll
        for (int sl = 0; sl < 2; ++sl)
#pragma unroll
            for (int kk = 0; kk < 4; ++kk) {
                const f32x4 bf = *reinterpret_cast<const f32x4*>(W3c + sl * 1024 + foff[kk]);
#pragma unroll
                for (int s4 = 0; s4 < 4; ++s4) acc3 = __builtin_amdgcn_mfma_f32_32x32x2f32(af2[sl][kk][s4], bf[s4], acc3, 0, 0, 0);
            }
        // ---- epilogue: BN + identity + ReLU, 16-byte accesses; the result is also the next conv1's A chunk.  Packed
        // fma / add (2 + 2 + 4 max per 16 bytes) and scalar-base accesses: the VALU shares the matrix pipe's lanes.
        {
            const int n = np * PW + 4 * c4;
            const f32x4 sc = *reinterpret_cast<const f32x4*>(fa.s3 + n);
            const f32x4 bi = *reinterpret_cast<const f32x4*>(fa.b3 + n);
            const f32x2 sc0 = {sc.x, sc.y}, sc1 = {sc.z, sc.w}, bi0 = {bi.x, bi.y}, bi1 = {bi.z, bi.w};
            __builtin_amdgcn_wave_barrier();
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int srow = crow + (r & 3) + 8 * (r >> 2);
                slab[srow * 32 + ((((lane & 31) >> 2) ^ (srow & 7)) << 2) + (lane & 3)] = acc3[r];
            }
            __builtin_amdgcn_wave_barrier();
            f32x4 ov[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int row = u * 8 + rsub;
                const f32x4 v = *reinterpret_cast<const f32x4*>(slab + row * 32 + ((c4 ^ (row & 7)) << 2));
                const f32x2 p0 = __builtin_elementwise_fma(f32x2{v.x, v.y}, sc0, bi0) + f32x2{rv[u].x, rv[u].y};
                const f32x2 p1 = __builtin_elementwise_fma(f32x2{v.z, v.w}, sc1, bi1) + f32x2{rv[u].z, rv[u].w};
                const f32x4 o = {fmaxf(p0.x, 0.f), fmaxf(p0.y, 0.f), fmaxf(p1.x, 0.f), fmaxf(p1.y, 0.f)};
                ov[u] = o;
                if (N1) {
                    const int arow = wave * 32 + row;
                    *reinterpret_cast<f32x4*>(A2 + arow * 32 + ((c4 ^ ((arow >> 1) & 7)) << 2)) = o;
                }
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                gf32x4* dst = reinterpret_cast<gf32x4*>(reinterpret_cast<gchar*>(obase[u] + (unsigned long long)np * PW * 4) + vout);
                if (full) *dst = ov[u];
                else if (row_ok[u]) *dst = ov[u];
            }
            if (np + 1 < npass) load_res(np + 1);        // the next pass's identity rows travel under this pass's tail
        }
        // Everything this wave needs next was requested BEFORE this pass's four output stores (vmcnt retires in order), so
        // it waits for "all but the newest four" and never for its own stores; ragged last block: plain vmcnt(0).
        // (newest in flight: 4 stores + the 4 identity loads of the next pass)
        if (!full) asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
        else if (np + 1 < npass) asm volatile("s_waitcnt vmcnt(8) lgkmcnt(0)" ::: "memory");
        else asm volatile("s_waitcnt vmcnt(4) lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();     // chunk image complete; this pass's W3 rows consumed; W1n[np] (and W3[np+1]) landed
        if (!W3DB && np + 1 < npass) issue_w3(np + 1);
        if (N1) {
            // ---- next conv1: acc1 += chunk[128 x 32] x W1n[:, 32 np ..]^T, wave tile 64 x N1/2
            const int tsm_dr = (PM && fa.tsm_T1 > 0) ? (np < fa.tsm_np1 ? 1 : np < 2 * fa.tsm_np1 ? -1 : 0) : 0;
#pragma unroll
            for (int kk = 0; kk < 4; ++kk) {
                f32x4 af[TM], bf[TN1 ? TN1 : 1];
                if (PM && tsm_dr != 0) {
                    // shifted channels: the neighbouring frame's row of the chunk image (its own swizzle), zeros at a clip end
#pragma unroll
                    for (int i = 0; i < TM; ++i) {
                        const int arow = wm * 64 + i * 32 + (lane & 31);
                        const int t = (m0 + arow) % fa.tsm_T1;
                        // (idle rows of a group of fewer than 128 images are not-ok: their frame index would send row 127 to row 128, past the image)
                        const bool ok = arow < fa.pm_gstride && (tsm_dr > 0 ? t < fa.tsm_T1 - 1 : t > 0);
                        const int nrow = ok ? arow + tsm_dr : arow;
                        const int swn = (nrow >> 1) & 7;
                        const f32x4 v = *reinterpret_cast<const f32x4*>(A2 + nrow * 32 + (((2 * kk + (lane >> 5)) ^ swn) << 2));
                        af[i] = ok ? v : f32x4{0.f, 0.f, 0.f, 0.f};
                    }
                } else {
#pragma unroll
                    for (int i = 0; i < TM; ++i) af[i] = *reinterpret_cast<const f32x4*>(A2 + (wm * 64 + i * 32) * 32 + foff[kk]);
                }
#pragma unroll
                for (int j = 0; j < TN1; ++j) bf[j] = *reinterpret_cast<const f32x4*>(W1s + (wn * TN1 * 32 + j * 32) * 32 + foff[kk]);
#pragma unroll
                for (int s4 = 0; s4 < 4; ++s4) mfma_step(acc1, af, bf, s4);
            }
            if (W3DB) asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            else asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");    // single W3 buffer: its refill must have landed
            __builtin_amdgcn_s_barrier();     // chunk image and W1n[np] consumed
            if (np + 1 < npass) issue_w1(np + 1);
        }
    }
    if (N1) {
        ConvArgs o1 = a;
        o1.scale = fa.s1n; o1.bias = fa.b1n; o1.res = nullptr; o1.out = fa.out1; o1.N = N1; o1.ldo = N1; o1.ldr = N1;
        o1.act = fa.act1n; o1.vec_epi = a.vec_epi == 2 ? 2 : 1;
        __syncthreads();
        conv_epilogue<TM, (TN1 ? TN1 : 1)>(o1, smem, acc1, m0, 0, wm, wn, lane, wave, rstride, roff, rlimit);
    }
}

// One thread per output element: the plain statement of the same contract.
__global__ void conv_naive_kernel(const ConvArgs a) {
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (long long)a.M * a.N) return;
    const int m = (int)(idx / a.N), n = (int)(idx - (long long)m * a.N);
    const int ohw = a.OH * a.OW;
    const int img = m / ohw, rem = m - img * ohw, oy = rem / a.OW, ox = rem - oy * a.OW;
    float s = 0.f;
    for (int kh = 0; kh < a.KH; ++kh)
        for (int kw = 0; kw < a.KW; ++kw) {
            const int iy = oy * a.stride - a.pad + kh, ix = ox * a.stride - a.pad + kw;
            if ((unsigned)iy >= (unsigned)a.H || (unsigned)ix >= (unsigned)a.W) continue;
            const int pix = img * a.H * a.W + iy * a.W + ix;
            const float* wr = a.w + (size_t)n * a.K + (kh * a.KW + kw) * a.cin;
            for (int c = 0; c < a.cin; ++c) {
                int src = pix;
                bool ok = true;
                if (a.tsm_T > 0) {
                    const int t = (pix / a.tsm_hw) % a.tsm_T;
                    if (c < a.tsm_fold) { ok = t < a.tsm_T - 1; src = pix + a.tsm_hw; }
                    else if (c < 2 * a.tsm_fold) { ok = t > 0; src = pix - a.tsm_hw; }
                }
                if (ok) s = fmaf(a.x[(size_t)src * a.ldx + c], wr[c], s);
            }
        }
    float v = fmaf(s, a.scale ? a.scale[n] : 1.f, a.bias ? a.bias[n] : 0.f);
    if (a.res) v += a.res[(size_t)m * a.ldr + n];
    if (a.act == ADAF_ACT_RELU) v = fmaxf(v, 0.f);
    else if (a.act == ADAF_ACT_RELU6) v = fminf(fmaxf(v, 0.f), 6.f);
    else if (a.act == ADAF_ACT_SIGMOID) v = 1.f / (1.f + expf(-v));
    else if (a.act == ADAF_ACT_SWISH) v = v / (1.f + expf(-v));
    a.out[(size_t)m * a.ldo + n] = v;
}

// ---- host side: which kernel instantiation a conv gets ---------------------------------------------------------------------------------
// Three steps: kTileTable says which tiles exist, plan_conv decides -- without touching the device -- the tile and the kernel form a conv
// takes, launch_row is the one place that spells the kernels' template arguments.  adaf_conv_plan_debug shows a plan to the host tests.
enum TileFamily {
    TF_REG,        // register-staged kernel (conv_gemm_kernel): takes every shape, the fallback of all the others
    TF_DMA_TOP,    // direct-to-LDS kernel, DMA issued at the top of a slice (kept for A/B)
    TF_DMA_MID,    // direct-to-LDS kernel, DMA issued between the MFMA groups  <- what the cost model picks
    TF_BAR23,      // fp32 pipe with the barrier between steps 2 and 3 of a slice (next slice's first fragments prefetched; measured variant)
    TF_SPLIT6,     // fp32 operands split on the fly into bf16 parts on the bf16 matrix pipe, 6 products per element pair; opt-in
    TF_SPLIT9,     // the same with 9 products
    TF_PRESPLIT,   // split (6 products) with the weights pre-split at load time (ConvArgs::wsp; trunk only)
    TF_F16,        // fp16 operands (adaf_conv2d_bn_act_f16 only)
    TF_LAT,        // small-batch form on v_mfma_f32_16x16x4_f32 (conv_lat.hip, which also holds its eligibility)
};
struct TileRow {
    int id;            // adaf_conv_params.tile / adaf_resnet50_set_tiles
    int bm, bn;        // block tile
    int wgm, wgn;      // wave grid
    TileFamily fam;
    int fallback;      // the id that takes a shape this row's kernel cannot (0: none, the conv is refused)
    int presplit;      // the pre-split row the automatic split choice moves to when the weights are pre-split (0: none)
    float eff;         // rows the cost model chooses among: relative efficiency of a launch that has the device to itself, from event-bracketed
                       // sweeps (tools/conv_probe.py) -- the regime of the fp16 and split families and of option conv_tile_regime = 0
    float eff_busy;    // the same rows, for launches that run beside others (profiles/tile_regime_ab.md).  128 x 64 and 64 x 64: the MFMA-busy share
                       // of the position-major kernels' own loops (0.83 / 0.76; counter runs serialise dispatches, so these are not figures under
                       // overlap, and the dense 128 x 64 kernel reads 0.71 with the short-K conv3s in it).  128 x 128 and 64 x 128 are FITTED: the ratios
                       // to 128 x 64 of the serial sweeps (-2 %) and of the three-stream A/B table
};
constexpr int kTileAutoSplit = 40;      // not a tile: the automatic choice among the split tiles
// Everything above 4 is reachable only through an explicit override (tools/conv_probe.py, tests) or the rules of resolve_f32_tile.
constexpr TileRow kTileTable[] = {
    {1, 128, 128, 2, 2, TF_REG, 0, 0, 1.00f, 0.80f},
    {2, 128, 64, 2, 2, TF_REG, 0, 0, 1.02f, 0.82f},
    {3, 64, 64, 2, 2, TF_REG, 0, 0, 0.98f, 0.76f},
    {4, 64, 128, 2, 2, TF_REG, 0, 0, 0.99f, 0.79f},
    {5, 256, 128, 4, 2, TF_REG, 0, 0, 0.f},            // 8 waves, 1 block/CU
    {21, 128, 128, 2, 2, TF_DMA_TOP, 1, 0, 0.f},
    {22, 128, 64, 2, 2, TF_DMA_TOP, 2, 0, 0.f},
    {23, 64, 64, 2, 2, TF_DMA_TOP, 3, 0, 0.f},
    {24, 64, 128, 2, 2, TF_DMA_TOP, 4, 0, 0.f},
    {25, 256, 128, 4, 2, TF_DMA_TOP, 5, 0, 0.f},       // 8 waves of 64x64
    {26, 256, 128, 2, 2, TF_DMA_TOP, 1, 0, 0.f},       // 4 waves of 128x64
    {31, 128, 128, 2, 2, TF_DMA_MID, 1, 0, 0.f},
    {32, 128, 64, 2, 2, TF_DMA_MID, 2, 0, 0.f},
    {33, 64, 64, 2, 2, TF_DMA_MID, 3, 0, 0.f},
    {34, 64, 128, 2, 2, TF_DMA_MID, 4, 0, 0.f},
    {38, 128, 32, 4, 1, TF_DMA_MID, 1, 0, 0.f},        // narrow outputs (cout <= 32, MobileNetV2 project convs): four waves of 32x32
    {39, 256, 32, 4, 1, TF_DMA_MID, 1, 0, 0.f},        // narrow outputs: four waves of 64x32
    {41, 128, 128, 2, 2, TF_SPLIT6, 1, 65, 0.f},
    {42, 128, 64, 2, 2, TF_SPLIT6, 2, 62, 0.f},
    {43, 64, 64, 2, 2, TF_SPLIT6, 3, 63, 0.f},
    {44, 64, 128, 2, 2, TF_SPLIT6, 4, 64, 0.f},
    {45, 256, 128, 4, 2, TF_SPLIT6, 5, 0, 0.f},        // 8 waves of 64x64
    {46, 256, 128, 2, 2, TF_SPLIT6, 1, 0, 0.f},        // 4 waves of 128x64
    {51, 128, 128, 2, 2, TF_SPLIT9, 1, 0, 0.f},
    {52, 128, 64, 2, 2, TF_SPLIT9, 2, 0, 0.f},
    {53, 64, 64, 2, 2, TF_SPLIT9, 3, 0, 0.f},
    {54, 64, 128, 2, 2, TF_SPLIT9, 4, 0, 0.f},
    {61, 128, 128, 2, 2, TF_PRESPLIT, 41, 0, 0.f},
    {62, 128, 64, 2, 2, TF_PRESPLIT, 42, 0, 0.f},
    {63, 64, 64, 2, 2, TF_PRESPLIT, 43, 0, 0.f},
    {64, 64, 128, 2, 2, TF_PRESPLIT, 44, 0, 0.f},
    {65, 128, 128, 4, 1, TF_PRESPLIT, 41, 0, 0.f},     // waves of 32x128: fewest activation splits per product
    {66, 256, 128, 8, 1, TF_PRESPLIT, 41, 0, 0.f},     // 8 waves of 32x128: 30 % less L2->LDS traffic per product
    {67, 256, 128, 4, 2, TF_PRESPLIT, 41, 0, 0.f},     // 8 waves of 64x64
    {71, 128, 128, 2, 2, TF_BAR23, 1, 0, 0.f},
    {72, 128, 64, 2, 2, TF_BAR23, 2, 0, 0.f},
    {73, 64, 64, 2, 2, TF_BAR23, 3, 0, 0.f},
    {74, 64, 128, 2, 2, TF_BAR23, 4, 0, 0.f},
    {81, 128, 128, 2, 2, TF_F16, 0, 0, 0.f},
    {82, 128, 64, 2, 2, TF_F16, 0, 0, 0.f},
    {83, 64, 64, 2, 2, TF_F16, 0, 0, 0.f},
    {84, 64, 128, 2, 2, TF_F16, 0, 0, 0.f},
    {88, 128, 32, 4, 1, TF_F16, 0, 0, 0.f},
    {95, 32, 32, 2, 2, TF_LAT, 0, 0, 0.f},             // four 16x16 wave tiles
#ifdef ADAF_EXP_TILES      // 256 x 256 block tiles, 8 waves of 128x64: experiments only (tools/exp/build_exp_tiles.sh), not in the product library
    {27, 256, 256, 2, 4, TF_DMA_TOP, 1, 0, 0.f},
    {37, 256, 256, 2, 4, TF_DMA_MID, 1, 0, 0.f},
    {47, 256, 256, 2, 4, TF_SPLIT6, 1, 0, 0.f},
#endif
};
constexpr int kNumTiles = (int)(sizeof(kTileTable) / sizeof(kTileTable[0]));
constexpr int kTileOut16 = 2;           // the register-staged tile that also exists with an fp16 store (fp32 operands)
constexpr int kTileF16Lo = 81, kTileF16Hi = 88;          // the id range of the fp16-operand tiles (adaf_conv2d_bn_act_f16 refuses any other)
constexpr int kTilePoolF32 = 32, kTilePoolF16 = 82;     // the tiles that also exist with the pooled epilogue (128 x 64: whole images per 128 rows)

constexpr int tile_index(int id) {      // position in kTileTable, -1: no such tile
    for (int i = 0; i < kNumTiles; ++i)
        if (kTileTable[i].id == id) return i;
    return -1;
}
constexpr int family_tile(TileFamily fam, int bm, int bn) {     // the family's (first) tile with this block shape, 0: none
    for (int i = 0; i < kNumTiles; ++i)
        if (kTileTable[i].fam == fam && kTileTable[i].bm == bm && kTileTable[i].bn == bn) return kTileTable[i].id;
    return 0;
}
constexpr int family_tile_like(TileFamily fam, int id) { return family_tile(fam, kTileTable[tile_index(id)].bm, kTileTable[tile_index(id)].bn); }
// what a family means for conv_gemm_glds_kernel's PIPE / EMU arguments (0 where the kernel has none)
constexpr int family_pipe(TileFamily f) { return f == TF_BAR23 ? 2 : f == TF_REG || f == TF_DMA_TOP || f == TF_LAT ? 0 : 1; }
constexpr int family_split(TileFamily f) { return f == TF_SPLIT6 || f == TF_PRESPLIT ? 6 : f == TF_SPLIT9 ? 9 : 0; }
// which rows have which special form (read by the planner at run time and by the launcher at compile time)
constexpr bool has_pos_major_form(const TileRow& r) { return r.fam == TF_DMA_MID || r.fam == TF_PRESPLIT; }
// (of the pre-split tiles only the 128 x 128 tile of four 32 x 128 waves, the one the split plan uses, has the lean K loop: the planes addressed
//  from a scalar base, no pointer arithmetic on the vector ALU the split itself needs -- CG_ABL 4: the DMA issue was 8 % of the split convs' time)
constexpr bool has_lean_form(const TileRow& r) {
    return r.fam == TF_DMA_MID || (r.fam == TF_PRESPLIT && r.bm == 128 && r.bn == 128 && r.wgm == 4 && r.wgn == 1);
}
// (64x64 tiles keep the builtin form of a plain 1x1: measured equal at K = 1024 and 7 % slower at K = 2048, cout 512 -- stage 4's conv1)
constexpr bool lean_dense_pays(const TileRow& r) { return has_lean_form(r) && r.bm * r.bn > 64 * 64; }
constexpr bool has_lean_shift_form(const TileRow& r) { return r.fam == TF_DMA_MID && r.bm * r.bn > 64 * 64; }

// DT argument of conv_gemm_glds_kernel / ET of conv_gemm_kernel: which operands are fp16
enum { DT_OUT16 = 1, DT_RES16 = 2, DT_IN16 = 4 };
enum PoolKind { POOL_F32, POOL_F16, POOL_F16_ROUNDED };

// The decision for one conv: a tile and the kernel form, by name, plus the launch-time fields of ConvArgs that follow from them.
struct ConvPlan {
    int tile = -1;              // resolved tile id; < 0: no kernel takes this conv
    int row = -1;               // its row in kTileTable (block shape, wave grid, family = pipe variant / split kind / pre-split weights)
    bool dense = false;         // DENSE: operand rows are contiguous K-vectors (a 1x1 stride-1 conv, or a strided 1x1 as a row gather)
    bool gather = false;        //   ... the strided 1x1 case
    bool special = false;       // SPECIAL: temporal shift in the operand load, or a partial last K slice
    bool lean = false;          // LEAN: straight-line K loop on scalar-base DMA
    bool pos_major = false;     // PM: position-major tiles with padding-tap skipping
    bool pool = false;          // POOL: global average pool in the epilogue
    int dt = 0;                 // DT_* bits
    ConvArgs a;                 // the conv as it is launched: tiles_n, nblocks, pm_images, pm_groups, vec_epi as planned; K, cin, ldx and
                                // tsm_fold in 32-bit words (halved for fp16 operands)
    explicit ConvPlan(const ConvArgs& conv) : a(conv) {}
};

bool conv_is_dense(const ConvArgs& a) { return a.KH == 1 && a.KW == 1 && a.stride == 1 && a.pad == 0; }
int conv_images(const ConvArgs& a) { return a.OH * a.OW > 0 ? a.M / (a.OH * a.OW) : 0; }

// The scalar-base DMA of the lean forms addresses an operand with 32-bit byte offsets: is its last element within reach (4 GB)?
bool dma_reach(size_t elems, size_t elem_bytes = 4) { return elems * elem_bytes < 0xffffff00ull; }
bool operands_in_dma_reach(const ConvArgs& a) {
    return dma_reach((size_t)a.M * a.ldx) && dma_reach((size_t)a.N * a.K) &&
           (conv_is_dense(a) || dma_reach((size_t)a.H * a.W * a.ldx * (size_t)conv_images(a)));
}
// A strided 1x1 conv without padding (ResNet's downsample branch) is the dense GEMM with a row gather: lean forms only.
bool strided_1x1_as_gather(const ConvArgs& a) {
    return !conv_is_dense(a) && a.KH == 1 && a.KW == 1 && a.pad == 0 && a.stride > 1 && a.tsm_T == 0 && (a.K & 31) == 0;
}

// Share of the filter taps that touch the image, averaged over the output pixels (1 = no padding work to skip).  The
// tap mask of a pixel is the product of a row mask and a column mask, so the count factorises.
double conv_tap_fill(const ConvArgs& a) {
    auto axis = [&](int out, int in, int k) {
        long long c = 0;
        for (int o = 0; o < out; ++o)
            for (int t = 0; t < k; ++t) c += (unsigned)(o * a.stride - a.pad + t) < (unsigned)in;
        return c;
    };
    return (double)(axis(a.OH, a.H, a.KH) * axis(a.OW, a.W, a.KW)) / ((double)a.OH * a.OW * a.KH * a.KW);
}
// Position-major tiles with padding-tap skipping: a k x k conv, enough images sharing a pixel position to fill the tile rows, and at least
// 4 % of the products padding.  On the split-bf16 pipe (pre-split rows; round 5) a skipped tap is whole MFMA steps of exact zeros, so the
// result is bit-identical to the row-major split tile; pm_allow == 2 (all taps walked, an experiment) exists on the fp32 pipe only.
bool pos_major_conv(const ConvArgs& a) {        // the conv's side of the gate: the same for every tile
    const int ohw = a.OH * a.OW;
    return !conv_is_dense(a) && a.KH * a.KW > 1 && a.KH * a.KW <= 32 && conv_images(a) * ohw == a.M && ohw <= 4096 && conv_tap_fill(a) < 0.96;
}
bool pos_major_gate(const ConvArgs& a, const TileRow& r) {
    return has_pos_major_form(r) && (r.fam == TF_PRESPLIT ? a.pm_allow == 1 : a.pm_allow != 0) && pos_major_conv(a) && conv_images(a) >= r.bm;
}
// A conv1 with the fused temporal shift on the lean K loop (round 6): whole 32-channel slices on either side of the fold boundaries, every
// row's frame neighbours inside the tensor (2 GB: the buffer form's offsets stay below the out-of-range marker)
bool lean_shift_gate(const ConvArgs& a, const TileRow& r) {
    return has_lean_shift_form(r) && conv_is_dense(a) && a.tsm_T > 0 && (a.K & 31) == 0 && (a.tsm_fold & 31) == 0 && a.stride == 1 &&
           operands_in_dma_reach(a) && adaf_options().tsm_lean && (size_t)a.M * a.ldx * 4 < 0x7fff0000ull;
}

// Does the DMA kernel take the shape (fp32 operands)?
bool adaf_conv_glds_ok(const ConvArgs& a) {
    if (conv_is_dense(a)) return a.K % 4 == 0;      // partial last slice is zero-filled
    return a.K % 32 == 0 && a.cin % 32 == 0 && a.KH * a.KW <= 32;
}

// fp16 operands: word-granular eligibility of the DMA kernel
bool conv_glds16_ok(const ConvArgs& a) {
    if ((a.K & 1) || (a.cin & 1) || (a.ldx & 1)) return false;
    if (conv_is_dense(a)) return (a.K / 2) % 4 == 0;
    return (a.K / 2) % 32 == 0 && (a.cin / 2) % 32 == 0 && a.KH * a.KW <= 32;
}

// ---- what a tile costs -----------------------------------------------------------------------------------------------------------------
// How much of the CU time a launch's uneven spread of blocks leaves idle is taken by launches that run beside it (other streams of a
// pipelined caller): 0 = none, the launch pays its busiest CU's whole blocks; 1 = all, only the padding of a tile counts.  Fitted to
// profiles/tile_regime_ab.md at 1024 patches of 96^2 under three streams.  Above 0.63: stage 4's conv1 and conv2 as 576 blocks of 128 x 64
// (2.25 per CU) beat 1152 blocks of 64 x 64, and stage 3's as 1152 beat 2304 (above 0.29).  Below 1: launches of a few blocks (8 patches) keep
// the tile that spreads them over the CUs.  On ONE stream nothing fills the gaps -- every one of these moves costs more there than it gains
// here -- which is why the regime is the caller's to name (plan_conv's `beside`) and not a property of the conv.
constexpr double kNeighbourFill = 0.75;

// The price of a conv on a tile, in MFMA work per CU; pure.  M x N outputs as `groups` independent row ranges (1; the pixel positions of
// position-major tiles, M = the images of one position) on `cus` CUs: the tile's area over its loop efficiency, times a mean, weighted by
// the fill, of the blocks per CU on average (what the launch costs where neighbours fill every gap) and on the busiest CU (where nothing
// does).  busy = false is a launch that has the device to itself: the busiest CU's whole blocks and the serial efficiencies.  K is the same
// for every tile and cancels.  (How many blocks of a tile a CU holds at once does not enter: they share the CU's matrix pipe, so a CU's time
// is the sum of its blocks' work however many of them are resident.)
double conv_tile_cost(long long M, int N, int K, const TileRow& r, int cus, bool busy, int groups = 1) {
    (void)K;
    const long long blocks = (long long)groups * ((M + r.bm - 1) / r.bm) * ((N + r.bn - 1) / r.bn);
    const double fill = busy ? kNeighbourFill : 0.0;
    const double per_cu = fill * (double)blocks / cus + (1.0 - fill) * (double)((blocks + cus - 1) / cus);
    return per_cu * r.bm * r.bn / (busy ? r.eff_busy : r.eff);
}
// The cheapest of the rows the cost model chooses among: a register-staged id, which the planner moves to the family it wants (family_tile_like).
// A row taller than a group (position-major tiles need as many images as tile rows) is priced row-major, as it would run.
int pick_tile(long long M, int N, int K, int cus, bool busy, int groups = 1, long long group_rows = 0) {
    int best = 1;
    double best_t = 1e300;
    for (const TileRow& r : kTileTable) {
        if (r.eff <= 0.f) continue;
        const bool grouped = groups > 1 && group_rows >= r.bm;
        const double cost = grouped ? conv_tile_cost(group_rows, N, K, r, cus, busy, groups) : conv_tile_cost(M, N, K, r, cus, busy);
        if (cost < best_t * 0.999) { best_t = cost; best = r.id; }
    }
    return best;
}

// 32-wide column tiles when 64-wide ones would spend >= 20 % of the MFMA columns on padding (cout = 16, 24, 32, 96, 160: MobileNetV2's
// project convs)
bool narrow_output(const ConvArgs& a) { return (((a.N + 63) / 64) * 64 - a.N) * 5 >= a.N; }
long long row_tiles(const ConvArgs& a, int bm) { return (a.M + bm - 1) / bm; }

// The fp32 tile a conv takes: `tile` as asked for (0 = automatic, kTileAutoSplit), moved along the rows' fallback ids until one takes the shape.
int resolve_f32_tile(const ConvArgs& a, int tile, int cus, bool beside) {
    const bool dma_ok = adaf_conv_glds_ok(a);
    const bool presplit_ok = a.wsp != nullptr && (a.K & 31) == 0 && dma_ok;
    if (tile == kTileAutoSplit) {   // split tiles, automatic: the bigger the wave tile the fewer split instructions per product
        tile = 0;
        if (dma_ok) {
            if (a.N <= 64) tile = family_tile(TF_SPLIT6, 128, 64);
            else if (row_tiles(a, 128) * ((a.N + 127) / 128) * 2 >= cus) tile = family_tile(TF_SPLIT6, 128, 128);
            else tile = family_tile_like(TF_SPLIT6, pick_tile(a.M, a.N, a.K, cus, false));   // tiny problems: fill the CUs first
            if (presplit_ok) tile = kTileTable[tile_index(tile)].presplit;
        }
    }
    if (tile <= 0) {
        // where the caller's launches run beside others the fp32 DMA tiles are priced for that, a k x k conv that will take position-major
        // tiles by the blocks of that form; the families whose loops were not measured that way (above, and the fp16 tiles) keep the serial regime
        const int regime = adaf_options().conv_tile_regime;      // 0 never, 1 where the caller says so, 2 always (A/B)
        const bool busy = (regime == 2 || (regime == 1 && beside)) && dma_ok;
        const bool pm = busy && a.pm_allow != 0 && pos_major_conv(a);
        tile = pm ? pick_tile(a.M, a.N, a.K, cus, busy, a.OH * a.OW, conv_images(a)) : pick_tile(a.M, a.N, a.K, cus, busy);
        if (dma_ok) {
            tile = family_tile_like(TF_DMA_MID, tile);
            // narrow outputs: 128 x 32 tiles when there are enough row tiles to fill the device; with fewer rows but a long reduction
            // (MobileNetV2's 960 -> 160 project convs on 7x7 maps: 25 k rows) waves of 64 x 32 under 256-row tiles -- 65 instead of 83 us
            // per 512 frames (tools/tail_gemm_tiles.py)
            if (narrow_output(a) && row_tiles(a, 128) >= cus) tile = family_tile(TF_DMA_MID, 128, 32);
            else if (narrow_output(a) && a.K >= 512 && row_tiles(a, 256) * ((a.N + 31) / 32) >= cus) tile = family_tile(TF_DMA_MID, 256, 32);
        }
    }
    for (int i = tile_index(tile); i >= 0; i = tile_index(tile)) {
        const TileRow& r = kTileTable[i];
        if (r.fam == TF_REG || (r.fam == TF_PRESPLIT ? presplit_ok : dma_ok && r.fam != TF_F16 && r.fam != TF_LAT)) return tile;
        tile = r.fallback;      // (the fp16 and latency rows have none: they are not reached through here)
    }
    return -1;
}

void plan_row_major(ConvPlan& p, const ConvArgs& a, int tile, int bm_rows) {
    p.row = tile_index(p.tile = tile);
    p.a.tiles_n = (a.N + kTileTable[p.row].bn - 1) / kTileTable[p.row].bn;
    p.a.nblocks = ((a.M + bm_rows - 1) / bm_rows) * p.a.tiles_n;
}

// The plan of one conv.  Pure: no HIP call, no launch; reads adaf_options().  beside: the launch overlaps launches of other streams.
ConvPlan plan_conv(const ConvArgs& a, int tile, int cus, bool beside = false) {
    ConvPlan p(a);
    const bool dense = conv_is_dense(a);
    if (a.in16) {    // operands fp16; output fp16 or fp32; residual (if any) fp16.  `a` arrives in ELEMENT units; the loader counts 32-bit words
        if (!conv_glds16_ok(a) || (a.res && !a.res16)) return p;
        if (tile < kTileF16Lo || tile > kTileF16Hi) {      // not an id adaf_conv2d_bn_act_f16 passes on: the automatic choice
            tile = family_tile_like(TF_F16, pick_tile(a.M, a.N, a.K, cus, false));
            if (narrow_output(a) && row_tiles(a, 128) >= cus) tile = family_tile(TF_F16, 128, 32);
        }
        if (tile_index(tile) < 0) return p;
        plan_row_major(p, a, tile, kTileTable[tile_index(tile)].bm);
        p.a.K /= 2; p.a.cin /= 2; p.a.ldx /= 2; p.a.tsm_fold /= 2;
        p.dt = DT_IN16 | DT_RES16 | (a.out16 ? DT_OUT16 : 0);
        p.dense = dense;
        p.special = dense && (a.tsm_T > 0 || (p.a.K & 31));
        return p;
    }
    if (a.out16) {   // fp32 operands, fp16 store (the 3x3 stem of the half-precision MobileNetV2): register-staged 128x64 tile
        if (a.res) return p;
        plan_row_major(p, a, kTileOut16, kTileTable[tile_index(kTileOut16)].bm);
        p.dt = DT_OUT16;
        p.dense = dense;
        return p;
    }
    const int asked = tile_index(tile);
    if (asked >= 0 && kTileTable[asked].fam == TF_LAT) {     // the small-batch form (bit-identical); conv_lat.hip may still decline the shape
        p.row = tile_index(p.tile = tile);
        return p;
    }
    tile = resolve_f32_tile(a, tile, cus, beside);
    if (tile < 0) return p;
    const TileRow& r = kTileTable[tile_index(tile)];
    plan_row_major(p, a, tile, r.bm);
    if (a.vec_epi) p.a.vec_epi = 2;      // interior tiles take the lean epilogue
    p.dense = dense;
    if (r.fam == TF_REG) return p;
    const bool special = a.tsm_T > 0 || (a.K & 31);
    p.special = dense && special;
    // the lean K loop addresses rows with 32-bit byte offsets from a scalar base; on the pre-split tile the three bf16 planes too
    const bool lean = has_lean_form(r) && operands_in_dma_reach(a) &&
                      (r.fam != TF_PRESPLIT || (adaf_options().split_lean && dma_reach((size_t)3 * a.N * a.K, 2)));
    if (pos_major_gate(a, r)) {
        p.pos_major = true;
        p.lean = lean && a.pm_allow != 2;
        p.a.pm_images = conv_images(a);
        p.a.pm_groups = (p.a.pm_images + r.bm - 1) / r.bm;
        p.a.nblocks = a.OH * a.OW * p.a.pm_groups * p.a.tiles_n;
    } else if ((dense || strided_1x1_as_gather(a)) && !special && lean && lean_dense_pays(r)) {
        p.gather = !dense;
        p.dense = p.lean = true;
    } else if (lean_shift_gate(a, r)) {
        p.lean = true;
    }
    return p;
}

// The three pooled launches share one eligibility: a 1x1 / stride 1 conv whose images of `hw` pixels fill a 128-row tile to >= 90 % (hw = 9
// at 96^2 patches: 14 images = 126 rows; 16 at 128^2; 25 at 144^2), 16-byte epilogue, whole K slices.
ConvPlan plan_conv_pool(const ConvArgs& a, int hw, const float* pool_out, int pool_ld, PoolKind kind) {
    ConvPlan p(a);
    const bool f16 = kind != POOL_F32;
    const bool relu_like = a.act == ADAF_ACT_NONE || a.act == ADAF_ACT_RELU || a.act == ADAF_ACT_RELU6;
    if (!adaf_options().conv_pool) return p;      // 0 = conv + separate avgpool_kernel (A/B)
    if ((a.in16 != 0) != f16 || a.out16 || a.split_n || a.tsm_T > 0 || a.wsp || !conv_is_dense(a) || (a.N & 3) || !a.vec_epi) return p;
    if (hw <= 0 || hw > 128 || a.M % hw || (128 / hw) * hw * 10 < 128 * 9 || (pool_ld & 3) || (reinterpret_cast<size_t>(pool_out) & 15)) return p;
    if (kind == POOL_F32 && (a.res16 || (a.K & 31) || !relu_like || !operands_in_dma_reach(a))) return p;
    if (f16 && (!conv_glds16_ok(a) || (a.K & 63))) return p;
    if (kind == POOL_F16 && a.res) return p;      // (EfficientNet's head: swish / sigmoid allowed, no identity)
    if (kind == POOL_F16_ROUNDED && ((a.res && !a.res16) || (a.ldr & 3) || !relu_like)) return p;
    plan_row_major(p, a, f16 ? kTilePoolF16 : kTilePoolF32, (128 / hw) * hw);
    p.dense = p.pool = true;
    p.lean = !f16;
    p.a.vec_epi = f16 ? a.vec_epi : 2;
    p.dt = kind == POOL_F16 ? DT_IN16 : kind == POOL_F16_ROUNDED ? DT_IN16 | DT_RES16 : 0;
    if (f16) { p.a.K /= 2; p.a.cin /= 2; p.a.ldx /= 2; }
    return p;
}

// The one place where the kernels' positional template arguments are written: row I of kTileTable in the form the plan names.  It
// instantiates, per row, exactly the forms has_*_form() allow; every macro call launches and returns.  (A lean dense kernel exists for every
// TF_DMA_MID row although the planner asks for it only where lean_dense_pays(): the library's set of kernels is kept as it was.)
template <int I>
int launch_row(const ConvPlan& p, const ConvArgs& a, hipStream_t s) {
    constexpr TileRow R = kTileTable[I];
    const dim3 grid(a.nblocks), block(64 * R.wgm * R.wgn);
    (void)grid; (void)block;
#define CONV_REG(...) do { hipLaunchKernelGGL((conv_gemm_kernel<R.bm, R.bn, R.wgm, R.wgn, __VA_ARGS__>), grid, block, 0, s, a); return p.tile; } while (0)
#define CONV_GLDS(...) do { hipLaunchKernelGGL((conv_gemm_glds_kernel<R.bm, R.bn, R.wgm, R.wgn, __VA_ARGS__>), grid, block, 0, s, a); return p.tile; } while (0)
    if constexpr (R.fam == TF_LAT) {
        return adaf_launch_conv_lat(a, s) ? p.tile : -1;
    } else if constexpr (R.fam == TF_REG) {
        //                             BK  DENSE  FLAGS ET
        if constexpr (R.id == kTileOut16) {
            if (p.dt == DT_OUT16 && p.dense) CONV_REG(32, true, 0, DT_OUT16);
            if (p.dt == DT_OUT16) CONV_REG(32, false, 0, DT_OUT16);
        }
        if (p.dense) CONV_REG(32, true, 0);
        CONV_REG(32, false, 0);
    } else if constexpr (R.fam == TF_F16) {
        constexpr int DT = DT_IN16 | DT_RES16;
        //                                            DENSE  PIPE SPECIAL EMU BSP    DT            PM     LEAN   POOL
        if constexpr (R.id == kTilePoolF16) {
            if (p.pool && (p.dt & DT_RES16)) CONV_GLDS(true, 1, false, 0, false, DT, false, false, true);      // fp16-rounded values averaged
            if (p.pool) CONV_GLDS(true, 1, false, 0, false, DT_IN16, false, false, true);
        }
        if (p.special && (p.dt & DT_OUT16)) CONV_GLDS(true, 1, true, 0, false, DT | DT_OUT16);
        if (p.dense && (p.dt & DT_OUT16)) CONV_GLDS(true, 1, false, 0, false, DT | DT_OUT16);
        if (p.dt & DT_OUT16) CONV_GLDS(false, 1, false, 0, false, DT | DT_OUT16);
        if (p.special) CONV_GLDS(true, 1, true, 0, false, DT);
        if (p.dense) CONV_GLDS(true, 1, false, 0, false, DT);
        CONV_GLDS(false, 1, false, 0, false, DT);
    } else {
        constexpr int PIPE = family_pipe(R.fam), EMU = family_split(R.fam);
        constexpr bool BSP = R.fam == TF_PRESPLIT;
        //                                                       DENSE  PIPE  SPECIAL EMU  BSP  DT PM     LEAN  POOL
        if constexpr (R.id == kTilePoolF32)
            if (p.pool) CONV_GLDS(true, PIPE, false, EMU, BSP, 0, false, true, true);
        if constexpr (has_pos_major_form(R)) {
            if constexpr (has_lean_form(R))
                if (p.pos_major && p.lean) CONV_GLDS(false, PIPE, false, EMU, BSP, 0, true, true);
            if (p.pos_major) CONV_GLDS(false, PIPE, false, EMU, BSP, 0, true);
        }
        if constexpr (has_lean_form(R))         // a plain 1x1, or a strided one as a row gather
            if (p.lean && !p.special) CONV_GLDS(true, PIPE, false, EMU, BSP, 0, false, true);
        if constexpr (has_lean_shift_form(R))   // conv1 with the fused temporal shift
            if (p.lean && p.special) CONV_GLDS(true, PIPE, true, EMU, BSP, 0, false, true);
        if (p.special) CONV_GLDS(true, PIPE, true, EMU, BSP);
        if (p.dense) CONV_GLDS(true, PIPE, false, EMU, BSP);
        CONV_GLDS(false, PIPE, false, EMU, BSP);
    }
#undef CONV_REG
#undef CONV_GLDS
}

template <int... I>
int launch_rows(const ConvPlan& p, const ConvArgs& a, hipStream_t s, std::integer_sequence<int, I...>) {
    int rc = -1;
    (void)((p.row == I && ((rc = launch_row<I>(p, a, s)), true)) || ...);
    return rc;
}

// Launches a plan on the kernel it names.  Returns the tile id or < 0.
int launch_plan(const ConvPlan& p, hipStream_t s) {
    return p.tile < 0 ? -1 : launch_rows(p, p.a, s, std::make_integer_sequence<int, kNumTiles>());
}

int launch_conv_pool(const ConvArgs& a, int hw, float* pool_out, int pool_ld, PoolKind kind, hipStream_t s) {
    ConvPlan p = plan_conv_pool(a, hw, pool_out, pool_ld, kind);
    if (p.tile < 0) return 0;
    p.a.pool_hw = hw; p.a.pool_rows = (128 / hw) * hw; p.a.pool_out = pool_out; p.a.pool_ld = pool_ld;
    launch_plan(p, s);
    return 1;
}

}  // namespace

bool adaf_conv_tile_exists(int tile) { return tile == kTileAutoSplit || tile_index(tile) >= 0; }

int adaf_launch_conv_gemm(const ConvArgs& a, int tile, int cus, hipStream_t s, bool beside) { return launch_plan(plan_conv(a, tile, cus, beside), s); }

// The trunk's last conv3 with the global average pool in its epilogue (conv_epilogue_pool): 1x1 / stride 1 fp32.  1 = launched, 0 = not eligible.
int adaf_launch_conv_pool(ConvArgs a, int hw, float* pool_out, int pool_ld, hipStream_t s) {
    return launch_conv_pool(a, hw, pool_out, pool_ld, POOL_F32, s);
}

// The same for fp16 operands and fp32 features (EfficientNet's head conv 1x1 + BN + swish + global average pool, effnet_kernels.hip): the 128 x 64
// fp16 tile -- the tile the unfused head conv runs on, same MFMA instruction and k order -- with whole images per tile and
// conv_epilogue_pool<SIG>.  `a` arrives in ELEMENT units like adaf_launch_conv_gemm's fp16 launches.
int adaf_launch_conv_pool16(ConvArgs a, int hw, float* pool_out, int pool_ld, hipStream_t s) {
    return launch_conv_pool(a, hw, pool_out, pool_ld, POOL_F16, s);
}

// The fp16 ResNet trunk's last conv3 (ADAF_MATH_F16): 1x1 fp16 operands, fp16 identity, ReLU, global average pool of the fp16-ROUNDED
// activated values (conv_epilogue_pool RND).  Every fp16 tile shape walks k in the same order per output, so this 128 x 64 tile gives the
// bits of whichever tile the unfused conv takes; with the rounding and the pixel-order sum the features are those of conv + pool.
int adaf_launch_conv_pool16_rounded(ConvArgs a, int hw, float* pool_out, int pool_ld, hipStream_t s) {
    return launch_conv_pool(a, hw, pool_out, pool_ld, POOL_F16_ROUNDED, s);
}

// Debug hook (not in include/adafocus.h): the plan of a conv, without a device.  `flags` carries what the params do not: ADAF_PLAN_* bits
// below, pm_allow in bits 4-5, BESIDE (the caller's launches overlap others') in bit 7, the pooled epilogue's pixels per image in bits 8 and up (0 = the plain conv).  Fills up to `n` ints of `out` in
// the order of kPlanFields (tests/test_conv_plan_host.py, tools/conv_launch_digest.py name them) and returns 0, or the code with which the
// C ABI's own validation (adaf_make_conv_args, adaf_set_conv_dtypes) refuses the conv before it plans.
extern "C" int adaf_conv_plan_debug(const adaf_conv_params* p, int flags, int cus, int* out, int n) {
    enum { IN16 = 1, OUT16 = 2, RES16 = 4, PRESPLIT = 8, VEC_EPI = 64, BESIDE = 128 };
    alignas(16) static const float operand[4] = {0.f, 0.f, 0.f, 0.f};      // stands for every operand: the planner looks at no operand's contents
    alignas(16) static float result[4];
    if (!out || cus <= 0) return ADAF_E_BADARG;
    adaf_handle host;       // no device behind it: the validation reads its defaults and leaves its message there
    ConvArgs a;
    int rc = adaf_make_conv_args(&host, p, operand, operand, nullptr, nullptr, (flags & RES16) ? operand : nullptr, result, &a);
    if (!rc && (flags & (IN16 | OUT16 | RES16))) rc = adaf_set_conv_dtypes(&host, (flags & IN16) != 0, (flags & OUT16) != 0, &a);
    if (rc) return rc;
    if (flags & PRESPLIT) a.wsp = reinterpret_cast<const unsigned short*>(operand);
    a.pm_allow = (flags >> 4) & 3;
    a.vec_epi = a.vec_epi && (flags & VEC_EPI);
    const int hw = flags >> 8;
    const ConvPlan c = hw > 0 ? plan_conv_pool(a, hw, operand, p->cout, !a.in16 ? POOL_F32 : a.res16 ? POOL_F16_ROUNDED : POOL_F16)
                              : plan_conv(a, p->tile, cus, (flags & BESIDE) != 0);
    const TileRow r = c.row >= 0 ? kTileTable[c.row] : TileRow{0, 0, 0, 0, 0, TF_REG, 0, 0, 0.f, 0.f};
    const int kPlanFields[] = {c.tile, r.bm, r.bn, r.wgm, r.wgn, (int)r.fam, r.fallback, family_pipe(r.fam), family_split(r.fam),
                               r.fam == TF_PRESPLIT, c.dt, c.dense, c.gather, c.special, c.lean, c.pos_major, c.pool, c.a.tiles_n, c.a.nblocks,
                               c.a.pm_images, c.a.pm_groups, c.a.vec_epi, c.a.K, c.a.cin, c.a.ldx, c.a.tsm_fold};
    for (int i = 0; i < n && i < (int)(sizeof(kPlanFields) / sizeof(int)); ++i) out[i] = kPlanFields[i];
    return ADAF_OK;
}

void adaf_launch_conv_naive(const ConvArgs& a, hipStream_t s) {
    const long long total = (long long)a.M * a.N;
    hipLaunchKernelGGL(conv_naive_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, a);
}

// Launcher of conv_fused_tail_kernel: c2 = the 3x3 conv's flattened description (64 -> 64, cin % 32 == 0, 16-byte epilogue legal).
// position-major tiles when the images fill the 128-row groups (<= 6 % padding rows): no tap masks in the gather
static bool fused_tail_pm(const ConvArgs& c2, int n3, int ldr, int* images_out, int* groups_out, int gstride = 128) {
    const int ohw = c2.OH * c2.OW;
    const int images = ohw > 0 ? c2.M / ohw : 0;
    const int groups = (images + gstride - 1) / gstride;
    *images_out = images;
    *groups_out = groups;
    // (with a group stride below 128 the idle rows count as padding too: up to 8 %)
    return c2.pm_allow == 1 && images * ohw == c2.M && images >= 128 && ohw <= 4096 &&
           (long long)groups * 128 * 100 <= (long long)images * (gstride == 128 ? 106 : 108) && (size_t)ohw * 8 * (size_t)(n3 > ldr ? n3 : ldr) * 4 < 0xffffff00ull;
}

// The fused tail addresses conv2's input, conv3's filters and its output / identity rows (n3 wide; the next conv1's 64 or 128 are fewer) with
// 32-bit lane offsets from scalar bases: are they all within reach?  Asked by the trunk before it decides on the fused launch (beyond the
// reach the block runs as conv2 / conv3 / next conv1, each planned by plan_conv) and by the launcher as its last line of defence.
bool adaf_fused_tail_in_reach(const ConvArgs& c2, int n3) {
    return (size_t)c2.M * c2.ldx * 4 < 0xffffff00ull && (size_t)c2.M * n3 * 4 < 0x3fffffffull * 4 && (size_t)n3 * 128 * 4 < 0xffffff00ull;
}

// images per tile group of the position-major tail whose next conv1 is shifted over clips of T frames: whole clips per tile
static int fused_tail_gstride(int tsm_T1) { return tsm_T1 > 0 && tsm_T1 <= 128 ? (128 / tsm_T1) * tsm_T1 : 128; }

// May the next block's conv1 ride in the fused tail although it carries the fused temporal shift (clips of tsm_T1 frames, fold of tsm_fold1
// channels)?  Only in the position-major form, with clips dividing the 128-image tiles and whole 32-channel passes per fold.
bool adaf_fused_tail_shift_ok(const ConvArgs& c2, int n3, int ldr, int tsm_T1, int tsm_fold1) {
    int images, groups;
    return adaf_options().tsm_lean && tsm_T1 > 0 && tsm_T1 <= 128 && fused_tail_pm(c2, n3, ldr, &images, &groups, fused_tail_gstride(tsm_T1)) &&
           images % tsm_T1 == 0 && tsm_fold1 > 0 && tsm_fold1 % 32 == 0 && 2 * tsm_fold1 <= n3;
}

// tsm_T1 > 0: the next conv1 (w1n) carries the fused temporal shift (adaf_fused_tail_shift_ok must hold: -2 otherwise, nothing launched).
int adaf_launch_fused_tail(const ConvArgs& c2, const float* w3, const float* s3, const float* b3, const float* res, int ldr,
                           float* out, int n3, const float* w1n, const float* s1n, const float* b1n, float* out1, int n1,
                           hipStream_t s, int tsm_T1, int tsm_fold1) {
    if (c2.N != 64 || c2.cin != 64 || (c2.K & 31) || c2.KH * c2.KW > 32 || n3 % 32 || (n1 != 0 && n1 != 64 && n1 != 128)) return -1;
    if (!adaf_fused_tail_in_reach(c2, n3)) return -1;      // scalar-base accesses: 32-bit lane offsets
    FusedTailArgs fa;
    fa.c2 = c2;
    fa.c2.tiles_n = 1;
    fa.c2.nblocks = (c2.M + 127) / 128;
    fa.c2.vec_epi = 2;       // the next block's conv1 tile goes out through the lean epilogue
    fa.w3 = w3; fa.s3 = s3; fa.b3 = b3; fa.res = res; fa.out = out; fa.n3 = n3; fa.ldr = ldr;
    fa.w1n = w1n; fa.s1n = s1n; fa.b1n = b1n; fa.out1 = out1; fa.act1n = ADAF_ACT_RELU;
    const int ohw = c2.OH * c2.OW;
    int images, groups;
    fa.tsm_T1 = 0; fa.tsm_np1 = 0; fa.pm_gstride = 128;
    if (n1 != 0 && tsm_T1 > 0) {
        if (!adaf_fused_tail_shift_ok(c2, n3, ldr, tsm_T1, tsm_fold1)) return -2;
        fa.tsm_T1 = tsm_T1;
        fa.tsm_np1 = tsm_fold1 / 32;
        fa.pm_gstride = fused_tail_gstride(tsm_T1);
    }
    const bool pm = fused_tail_pm(c2, n3, ldr, &images, &groups, fa.pm_gstride);
    if (pm) {
        fa.c2.pm_images = images;
        fa.c2.pm_groups = groups;
        fa.c2.nblocks = ohw * groups;
    }
    const dim3 grid(fa.c2.nblocks), block(256);
    if (pm) {
        if (n1 == 0) hipLaunchKernelGGL((conv_fused_tail_kernel<0, true>), grid, block, 0, s, fa);
        else if (n1 == 64) hipLaunchKernelGGL((conv_fused_tail_kernel<64, true>), grid, block, 0, s, fa);
        else hipLaunchKernelGGL((conv_fused_tail_kernel<128, true>), grid, block, 0, s, fa);
    } else {
        if (n1 == 0) hipLaunchKernelGGL((conv_fused_tail_kernel<0, false>), grid, block, 0, s, fa);
        else if (n1 == 64) hipLaunchKernelGGL((conv_fused_tail_kernel<64, false>), grid, block, 0, s, fa);
        else hipLaunchKernelGGL((conv_fused_tail_kernel<128, false>), grid, block, 0, s, fa);
    }
    return 0;
}

// Debug hook (not in include/adafocus.h), without a device like adaf_conv_plan_debug: is the fused tail whose conv2 is `p` and whose conv3
// has n3 outputs within its 32-bit reach (1 / 0), or the code with which the C ABI's validation refuses `p`.
extern "C" int adaf_fused_tail_reach_debug(const adaf_conv_params* p, int n3) {
    alignas(16) static const float operand[4] = {0.f, 0.f, 0.f, 0.f};
    alignas(16) static float result[4];
    adaf_handle host;
    ConvArgs a;
    const int rc = adaf_make_conv_args(&host, p, operand, operand, nullptr, nullptr, nullptr, result, &a);
    return rc ? rc : (adaf_fused_tail_in_reach(a, n3) ? 1 : 0);
}
