// The EfficientNet network object (adaf_effnet): the block table of the compound scaling, the SAME-padding geometry of a forward, which
// launch form every MBConv block takes, the weight side (finalize), the workspace and the forward walk; and the C entry points of the
// stand-alone MBConv ops.  Host code only: every launch it makes is declared in adaf_internal.h (the kernels and their launchers are
// in effnet_kernels.hip -- whose header describes the network and the launch plan per block --, mbconv_whole.hip and conv_gemm.hip).
#include <cmath>
#include <cstdio>
#include <string>
#include <vector>

#include "adaf_net.h"

using EfConv = AdafNetConv;     // "stem", "b3.expand", "b3.dw", "b3.project", "head"; w16: the dense 1x1 filters in fp16 (ADAF_DTYPE_F16)
struct EfBlock {
    int k, stride, expand_ratio, cin, cout, hid, sq;
    int expand, dwc, project;       // indices into convs (expand = -1 when the ratio is 1)
    float* se_wr = nullptr;         // [sq][hid]
    float* se_br = nullptr;         // [sq]
    float* se_wet = nullptr;        // [sq][hid] (transposed _se_expand.weight)
    float* se_be = nullptr;         // [hid]
    unsigned short* wef = nullptr;  // fp16 storage: expand / project filters in MFMA B-fragment order for the whole-block kernel
    unsigned short* wpf = nullptr;  //  (mbconv_whole.hip)
    float* wdl = nullptr;           //  ... and the depthwise taps + folded BN as one row per channel
};

struct adaf_effnet {
    adaf_handle* h = nullptr;
    float width = 1.f, depth = 1.f;
    AdafParamTable params;  // what set_param registered since the last finalize
    AdafWeightArena arena;  // every derived weight buffer: packed filters, folded BN, SE matrices, B fragments
    std::vector<EfConv> convs;
    std::vector<EfBlock> blocks;
    int stem = 0, head = 0, feat = 1280;
    int dtype = ADAF_DTYPE_F32;
    // MBConv blocks whose map is small enough for a workgroup to own whole images run as ONE launch (mbconv_whole.hip; fp16 storage,
    // stride 1, maps up to 9 x 9).  On by default; adaf_effnet_set_fusion(net, 0) restores the four-launch plan (tests, A/B).
    bool fuse = true;
    bool finalized = false;
    float* stem_bank = nullptr;      // the stem filter in the packed kernel's lane order (C0 <= 48; ef_stem_packed_kernel)
    // Two patch chunks travel through the network side by side (ADAF_EF_PLAN_PAIR_CHUNKS; the second on a library-owned stream forked from
    // and joined to the caller's stream by events, one helper per caller stream -- as adaf_mobilenetv2 does): the launches of the 9 x 9 and
    // 5 x 5 stages, the SE gates and every launch's ramp and tail leave room that a neighbour fills.
    AdafAuxPool aux;        // (adaf_internal.h: LRU over caller streams, mutex-guarded)
};

namespace {

// efficientnet_pytorch utils.py round_filters / round_repeats (depth_divisor 8)
int round_filters(int filters, float width) {
    const double f = (double)filters * (double)width;
    int nf = (int)(f + 4.0) / 8 * 8;
    if (nf < 8) nf = 8;
    if ((double)nf < 0.9 * f) nf += 8;
    return nf;
}
int round_repeats(int r, float depth) { return (int)std::ceil((double)depth * r - 1e-9); }

// blocks_args of utils.py efficientnet(): repeats, kernel, stride, expand, in, out (se_ratio 0.25 everywhere)
const int kBase[7][6] = {{1, 3, 1, 1, 32, 16}, {2, 3, 2, 6, 16, 24}, {2, 5, 2, 6, 24, 40}, {3, 3, 2, 6, 40, 80},
                         {3, 5, 1, 6, 80, 112}, {4, 5, 2, 6, 112, 192}, {1, 3, 1, 6, 192, 320}};

void build(adaf_effnet* net) {
    net->convs.clear();
    net->blocks.clear();
    const int c0 = round_filters(32, net->width);
    net->stem = 0;
    net->convs.push_back(adaf_net_conv("stem", 3, c0, 3, 2, false, 4));
    int last = c0;
    for (auto& s : kBase) {
        const int i0 = round_filters(s[4], net->width), o = round_filters(s[5], net->width), rep = round_repeats(s[0], net->depth);
        for (int j = 0; j < rep; ++j) {
            EfBlock b;
            b.k = s[1]; b.stride = j == 0 ? s[2] : 1; b.expand_ratio = s[3];
            b.cin = j == 0 ? i0 : o; b.cout = o; b.hid = b.cin * s[3];
            b.sq = (int)(b.cin * 0.25); if (b.sq < 1) b.sq = 1;
            char nm[40];
            const int bi = (int)net->blocks.size();
            b.expand = -1;
            if (s[3] != 1) {
                snprintf(nm, sizeof(nm), "b%d.expand", bi);
                b.expand = (int)net->convs.size();
                net->convs.push_back(adaf_net_conv(nm, b.cin, b.hid, 1, 1, false, b.cin));
            }
            snprintf(nm, sizeof(nm), "b%d.dw", bi);
            b.dwc = (int)net->convs.size();
            net->convs.push_back(adaf_net_conv(nm, b.hid, b.hid, b.k, b.stride, true, b.hid));
            snprintf(nm, sizeof(nm), "b%d.project", bi);
            b.project = (int)net->convs.size();
            net->convs.push_back(adaf_net_conv(nm, b.hid, b.cout, 1, 1, false, b.hid));
            net->blocks.push_back(b);
            last = o;
        }
    }
    net->feat = round_filters(1280, net->width);
    net->head = (int)net->convs.size();
    net->convs.push_back(adaf_net_conv("head", last, net->feat, 1, 1, false, last));
}

inline int ceil_div(int a, int b) { return (a + b - 1) / b; }
// Conv2dStaticSamePadding (utils.py): padding for an input of `size`; returns pad_before, writes the total
inline int same_pad(int size, int k, int stride, int* total) {
    const int out = ceil_div(size, stride);
    int t = (out - 1) * stride + k - size;
    if (t < 0) t = 0;
    *total = t;
    return t / 2;
}
inline int conv_out_len(int in, int k, int stride, int pad_total) { return (in + pad_total - k) / stride + 1; }

// The SAME-padding geometry of a forward, walked ONCE: the padding is computed for an image of pad_size (Conv2dStaticSamePadding) and
// applied to the map as it is -- per conv the rows / columns in front (pad) and the output side the total padding leaves.
struct EfGeometry {
    int stem_pad, stem_hw;                      // the stem's pad_before and its output side
    struct Block { int hw, ohw, pad; };         // an MBConv block's input side, output side and the depthwise conv's pad_before
    std::vector<Block> blocks;
};
EfGeometry geometry(const adaf_effnet* net, int size, int pad_size) {
    EfGeometry G;
    int tot;
    G.stem_pad = same_pad(pad_size, 3, 2, &tot);
    G.stem_hw = conv_out_len(size, 3, 2, tot);
    int hw = G.stem_hw, ps = ceil_div(pad_size, 2);
    for (auto& b : net->blocks) {
        const int pad = same_pad(ps, b.k, b.stride, &tot);
        const int ohw = conv_out_len(hw, b.k, b.stride, tot);
        G.blocks.push_back({hw, ohw, pad});
        hw = ohw;
        ps = ceil_div(ps, b.stride);
    }
    return G;
}

// ---- which launch form a block takes ------------------------------------------------------------------------------------
enum class EfForm { Whole, FusedExpand, FourLaunches };     // one launch (mbconv_whole.hip) | expand inside the depthwise launch | expand, depthwise, gate, project

// Blocks finalize packs the whole-block kernel's operands for (fp16 storage): the part of its rule that does not depend on the map
bool whole_block_operands(const EfBlock& b) { return b.expand >= 0 && (b.stride == 1 || b.stride == 2) && b.cin % 8 == 0 && b.hid % 16 == 0; }

// Does the whole-block kernel take this block?  Its geometry: the SAME padding of the map as it is (pad rows in front as the kernel
// computes them, output = ceil(hw / stride)): stride 1 everywhere it is instantiated, stride 2 for the 9 x 9 -> 5 x 5 block.
bool ef_whole_geometry(const EfBlock& b, const EfGeometry::Block& g) {
    return b.expand >= 0 && (b.stride == 1 || b.stride == 2) && g.ohw == (g.hw + b.stride - 1) / b.stride && g.pad == adaf_mbw_pad_before(g.hw, b.k, b.stride) &&
           adaf_mbw_eligible(g.hw, b.k, b.stride, b.cin, b.hid, b.cout, b.sq);
}

// May block bi take the fused expand + depthwise launch: the switches, and the shapes adaf_launch_dw_expand accepts
bool fused_expand_takes(const adaf_effnet* net, size_t bi, const EfGeometry::Block& g) {
    const EfBlock& b = net->blocks[bi];
    return net->dtype == ADAF_DTYPE_F16 && (adaf_options().effnet_plan & ADAF_EF_PLAN_FUSED_EXPAND) && b.expand >= 0 && bi < 32 &&
           ((adaf_options().effnet_fused_blocks >> bi) & 1u) && b.cin % 8 == 0 && b.cin <= 64 &&
           adaf_effnet_dw_tiles_fused(b.hid, g.ohw, g.ohw, b.k, b.stride) > 0;
}

// THE rule: the form of block bi at geometry g under the net's dtype and fusion setting and the effnet_plan / effnet_fused_blocks options
EfForm block_form(const adaf_effnet* net, size_t bi, const EfGeometry::Block& g) {
    if (net->dtype == ADAF_DTYPE_F16 && net->fuse && (adaf_options().effnet_plan & ADAF_EF_PLAN_WHOLE_BLOCK) && ef_whole_geometry(net->blocks[bi], g))
        return EfForm::Whole;
    return fused_expand_takes(net, bi, g) ? EfForm::FusedExpand : EfForm::FourLaunches;
}

int count_form(const adaf_effnet* net, int size, int pad_size, EfForm form) {
    if (!net || size < 32) return 0;
    const EfGeometry G = geometry(net, size, pad_size > 0 ? pad_size : size);
    int count = 0;
    for (size_t bi = 0; bi < net->blocks.size(); ++bi) count += block_form(net, bi, G.blocks[bi]) == form;
    return count;
}

// elements per frame of the chunk buffers: io (block input / output, ping-pong), ex (expanded), dw (depthwise output);
// pc = the largest tiles * hid of a squeeze partial buffer
void slab_sizes(const adaf_effnet* net, const EfGeometry& G, int dtype, size_t* io, size_t* ex, size_t* dw, size_t* pc, size_t* gc) {
    *io = (size_t)G.stem_hw * G.stem_hw * net->convs[net->stem].cout;
    *ex = *dw = *pc = *gc = 0;
    for (size_t bi = 0; bi < net->blocks.size(); ++bi) {
        const EfBlock& b = net->blocks[bi];
        const int hw = G.blocks[bi].hw, ohw = G.blocks[bi].ohw;
        if (b.expand >= 0 && (size_t)hw * hw * b.hid > *ex) *ex = (size_t)hw * hw * b.hid;
        if ((size_t)ohw * ohw * b.hid > *dw) *dw = (size_t)ohw * ohw * b.hid;
        if ((size_t)ohw * ohw * b.cout > *io) *io = (size_t)ohw * ohw * b.cout;
        int tiles = adaf_effnet_dw_tiles(b.hid, ohw, ohw, b.k, b.stride, dtype);
        if (dtype == ADAF_DTYPE_F16) {                       // (the fused expand + depthwise launch has a tile plan of its own)
            const int tf = adaf_effnet_dw_tiles_fused(b.hid, ohw, ohw, b.k, b.stride);
            if (tf > tiles) tiles = tf;
        }
        if ((size_t)(tiles > 0 ? tiles : 1) * b.hid > *pc) *pc = (size_t)(tiles > 0 ? tiles : 1) * b.hid;
        if ((size_t)b.hid > *gc) *gc = b.hid;
    }
    // the head's fp32 map is parked in the expanded-map slab when the caller does not want it
    const int hw = G.blocks.back().ohw;
    const size_t headf = (size_t)hw * hw * net->feat * 4 / (dtype == ADAF_DTYPE_F16 ? 2 : 4);
    if (headf > *ex) *ex = headf;
}

int chunk_frames(int n) {
    const int c = adaf_options().effnet_chunk > 0 ? adaf_options().effnet_chunk : 1024;
    // a batch that fits one chunk but holds >= 512 patches travels as a pair of half chunks (see adaf_effnet::Aux): 1024 patches of
    // 144^2 6.21 -> 5.95 ms (tools/effnet_streams_probe.py); a patch's arithmetic does not depend on the chunk it travels in
    if ((adaf_options().effnet_plan & ADAF_EF_PLAN_PAIR_CHUNKS) && n <= c && n >= 512) return (n + 1) / 2;
    return n < c ? n : c;
}

// The workspace, stated once: per chunk A and B (block in / out ping-pong), E (expanded), D (depthwise out) in the storage type, the
// squeeze partials and the gates in fp32, each in whole 256-byte lines; a batch of more than one chunk has two chunks in flight and
// a second set behind the first.  With ws == nullptr it only measures (the query).
struct EfSlabs { char *A, *B, *E, *D; float *part, *gate; };
struct EfWorkspace { int chunk; size_t bytes; EfSlabs slot[2]; };
EfWorkspace workspace_layout(const adaf_effnet* net, const EfGeometry& G, int n, void* ws) {
    size_t io, ex, dw, pc, gc;
    slab_sizes(net, G, net->dtype, &io, &ex, &dw, &pc, &gc);
    const size_t es = net->dtype == ADAF_DTYPE_F16 ? 2 : 4;
    EfWorkspace w = {};
    w.chunk = chunk_frames(n);
    const int slots = n > w.chunk ? 2 : 1;       // two chunks in flight (whether or not the pairing is switched on)
    AdafCarver c(ws);
    for (int i = 0; i < slots; ++i) {
        w.slot[i].A = c.take<char>((size_t)w.chunk * io * es, 256);
        w.slot[i].B = c.take<char>((size_t)w.chunk * io * es, 256);
        w.slot[i].E = c.take<char>((size_t)w.chunk * ex * es, 256);
        w.slot[i].D = c.take<char>((size_t)w.chunk * dw * es, 256);
        w.slot[i].part = c.take<float>((size_t)w.chunk * pc, 256);
        w.slot[i].gate = c.take<float>((size_t)w.chunk * gc, 256);
    }
    w.bytes = c.off;
    return w;
}

int run_dense(adaf_effnet* net, const EfConv& L, const void* in, bool in16, int n, int hh, int ww, int oh, int ow, int pad, int act,
              void* out, bool out16, hipStream_t st) {
    ConvArgs a = adaf_net_conv_args(L, in16 ? static_cast<const void*>(L.w16) : L.w, in, n, hh, ww, oh, ow, pad, act, nullptr, out, net->h->zeros);
    a.in16 = in16; a.out16 = out16;
    return adaf_launch_conv_gemm(a, 0, net->h->cus, st) > 0 ? ADAF_OK : ADAF_E_LAUNCH;
}

}  // namespace

extern "C" {

int adaf_effnet_create(adaf_handle* h, float width_coefficient, float depth_coefficient, adaf_effnet** out) {
    if (!h || !out) return ADAF_E_BADARG;
    if (!(width_coefficient >= 0.5f && width_coefficient <= 4.f && depth_coefficient >= 0.5f && depth_coefficient <= 8.f))
        return adaf_fail(h, ADAF_E_BADARG, "effnet: width / depth coefficients out of range");
    adaf_effnet* net = new adaf_effnet();
    net->h = h;
    net->width = width_coefficient;
    net->depth = depth_coefficient;
    build(net);
    *out = net;
    return ADAF_OK;
}

int adaf_effnet_destroy(adaf_effnet* net) {
    if (!net) return ADAF_OK;
    net->arena.release();
    net->aux.destroy();
    delete net;
    return ADAF_OK;
}

int adaf_effnet_feature_dim(const adaf_effnet* net) { return net ? net->feat : 0; }
int adaf_effnet_block_count(const adaf_effnet* net) { return net ? (int)net->blocks.size() : 0; }

int adaf_effnet_block_info(const adaf_effnet* net, int block, int* info8) {
    if (!net || !info8 || block < 0 || block >= (int)net->blocks.size()) return ADAF_E_BADARG;
    const EfBlock& b = net->blocks[block];
    info8[0] = b.k; info8[1] = b.stride; info8[2] = b.expand_ratio; info8[3] = b.cin; info8[4] = b.cout; info8[5] = b.hid;
    info8[6] = b.sq; info8[7] = net->convs[net->stem].cout;
    return ADAF_OK;
}

int adaf_effnet_set_fusion(adaf_effnet* net, int on) {
    if (!net) return ADAF_E_BADARG;
    net->fuse = on != 0;
    return ADAF_OK;
}

int adaf_effnet_whole_blocks(const adaf_effnet* net, int size, int pad_size) { return count_form(net, size, pad_size, EfForm::Whole); }
int adaf_effnet_fused_expand_blocks(const adaf_effnet* net, int size, int pad_size) { return count_form(net, size, pad_size, EfForm::FusedExpand); }

int adaf_effnet_set_dtype(adaf_effnet* net, int dtype) {
    if (!net) return ADAF_E_BADARG;
    if (dtype != ADAF_DTYPE_F32 && dtype != ADAF_DTYPE_F16) return adaf_fail(net->h, ADAF_E_BADARG, "effnet: unknown dtype %d", dtype);
    if (dtype != net->dtype) net->finalized = false;
    net->dtype = dtype;
    return ADAF_OK;
}

int adaf_effnet_set_param(adaf_effnet* net, const char* name, const float* dev_ptr, size_t numel) {
    if (!net || !name || !dev_ptr) return ADAF_E_BADARG;
    net->params.set(name, dev_ptr, numel);
    net->finalized = false;
    return ADAF_OK;
}

static int finalize_registered(adaf_effnet* net, void* stream) {
    adaf_handle* h = net->h;
    hipStream_t st = (hipStream_t)stream;
    AdafWeightArena& arena = net->arena;
    auto get = [&](const std::string& key, size_t numel, const float** p) { return net->params.get(h, "effnet", key, numel, p); };
    const auto nomem = [&] { return adaf_fail(h, ADAF_E_NOMEM, "effnet: hipMalloc packed weights"); };
    for (auto& L : net->convs) {
        const float* w;
        if (int rc = adaf_pack_conv_bn(h, "effnet", net->params, arena, L, 1e-3f, st, &w)) return rc;     // utils.py: batch_norm_epsilon = 1e-3
        if (!L.dw && L.k == 1 && net->dtype == ADAF_DTYPE_F16) {
            if (!arena.take(&L.w16, L.packed_floats())) return nomem();
            adaf_launch_pack_weight_f16(w, L.cout, L.cin, 1, 1, L.cin_pad, L.w16, st);
        }
    }
    {
        const EfConv& S = net->convs[net->stem];
        if (S.cout <= 48 && S.k == 3 && S.cin_pad == 4) {
            if (!arena.take(&net->stem_bank, (size_t)64 * 24)) return nomem();
            adaf_launch_pack_stem_bank(S.w, S.cout, net->stem_bank, st);
        }
    }
    for (size_t bi = 0; bi < net->blocks.size(); ++bi) {
        EfBlock& b = net->blocks[bi];
        char nm[48];
        const float *wr, *br, *we, *be;
        int rc;
        snprintf(nm, sizeof(nm), "b%zu.se_reduce", bi);
        if ((rc = get(std::string(nm) + ".weight", (size_t)b.sq * b.hid, &wr)) || (rc = get(std::string(nm) + ".bias", b.sq, &br))) return rc;
        snprintf(nm, sizeof(nm), "b%zu.se_expand", bi);
        if ((rc = get(std::string(nm) + ".weight", (size_t)b.sq * b.hid, &we)) || (rc = get(std::string(nm) + ".bias", b.hid, &be))) return rc;
        if (!arena.take(&b.se_wr, (size_t)b.sq * b.hid) || !arena.take(&b.se_br, (size_t)b.sq) || !arena.take(&b.se_wet, (size_t)b.sq * b.hid) ||
            !arena.take(&b.se_be, (size_t)b.hid))
            return nomem();
        (void)hipMemcpyAsync(b.se_wr, wr, (size_t)b.sq * b.hid * 4, hipMemcpyDeviceToDevice, st);
        (void)hipMemcpyAsync(b.se_br, br, (size_t)b.sq * 4, hipMemcpyDeviceToDevice, st);
        (void)hipMemcpyAsync(b.se_be, be, (size_t)b.hid * 4, hipMemcpyDeviceToDevice, st);
        adaf_launch_transpose(we, b.hid, b.sq, b.se_wet, st);
        if (net->dtype == ADAF_DTYPE_F16 && whole_block_operands(b)) {
            // the whole-block kernel streams its filters as ready-made B fragments (one coalesced 1 KB load per wave instruction)
            const float *wexp, *wproj;
            if ((rc = get(net->convs[b.expand].name + ".weight", (size_t)b.hid * b.cin, &wexp)) ||
                (rc = get(net->convs[b.project].name + ".weight", (size_t)b.cout * b.hid, &wproj)))
                return rc;
            if (!arena.take(&b.wef, adaf_mbw_bfrag_halfs(b.hid, b.cin, true)) || !arena.take(&b.wpf, adaf_mbw_bfrag_halfs(b.cout, b.hid, false))) return nomem();
            adaf_launch_pack_bfrag_f16(wexp, b.hid, b.cin, true, b.wef, st);
            adaf_launch_pack_bfrag_f16(wproj, b.cout, b.hid, false, b.wpf, st);
            if (!arena.take(&b.wdl, (size_t)b.hid * adaf_mbw_tap_row(b.k))) return nomem();
            const EfConv& D = net->convs[b.dwc];
            adaf_launch_pack_dw_rows(D.w, D.scale, D.bias, b.hid, b.k, b.wdl, st);
        }
    }
    hipError_t e = hipStreamSynchronize(st);
    if (e != hipSuccess) return adaf_hip_fail(h, e, "effnet finalize");
    net->aux.prepare(4);        // helper streams exist before the first forward (which may be captured into a HIP graph)
    net->finalized = true;
    return ADAF_OK;
}

int adaf_effnet_finalize(adaf_effnet* net, void* stream) {
    if (!net) return ADAF_E_BADARG;
    const int rc = finalize_registered(net, stream);
    net->params.clear();       // a registration lives until here, whatever finalize returned (include/adafocus.h)
    return rc;
}

size_t adaf_effnet_workspace_bytes(const adaf_effnet* net, int n, int size, int pad_size) {
    return (!net || n <= 0 || size < 32) ? 0 : workspace_layout(net, geometry(net, size, pad_size > 0 ? pad_size : size), n, nullptr).bytes;
}

int adaf_effnet_forward(adaf_effnet* net, const float* frames_nhwc4, int n, int size, int pad_size, int upto_block, void* block_out,
                        float* featmap, float* featvec, int ldvec, void* ws, size_t ws_bytes, void* stream) {
    if (!net) return ADAF_E_BADARG;
    adaf_handle* h = net->h;
    if (!net->finalized) return adaf_fail(h, ADAF_E_STATE, "effnet: finalize() has not been called");
    if (!frames_nhwc4 || !ws) return adaf_fail(h, ADAF_E_BADARG, "effnet: null pointer");
    if (n <= 0 || size < 32) return adaf_fail(h, ADAF_E_BADARG, "effnet: need n > 0 and size >= 32");
    if (pad_size <= 0) pad_size = size;
    if (featvec && ldvec < net->feat) return adaf_fail(h, ADAF_E_LAYOUT, "effnet: ldvec >= %d required", net->feat);
    if (upto_block >= 0 && !block_out) return adaf_fail(h, ADAF_E_BADARG, "effnet: upto_block needs block_out");
    const EfGeometry G = geometry(net, size, pad_size);
    const EfWorkspace W = workspace_layout(net, G, n, ws);
    int rc = adaf_check_ws(h, "effnet", ws, ws_bytes, W.bytes, ADAF_WS_ALIGN_FIRST);
    if (rc) return rc;
    const bool f16 = net->dtype == ADAF_DTYPE_F16;
    const size_t es = f16 ? 2 : 4;
    // one chunk of patches through the whole network on stream `st` with its own slot of the workspace
    auto run_chunk = [&](int f0, int nc, int slot, hipStream_t st) -> int {
        const EfSlabs& slabs = W.slot[slot];
        char *const bufA = slabs.A, *const bufB = slabs.B, *const bufE = slabs.E, *const bufD = slabs.D;
        float *const part = slabs.part, *const gate = slabs.gate;
        int rc;
        char* cur = bufA;
        char* nxt = bufB;
        const EfConv& S = net->convs[net->stem];
        const unsigned plan = adaf_options().effnet_plan;
        const bool own_stem = (plan & ADAF_EF_PLAN_OWN_STEM) != 0;       // off = the generic engine (A/B)
        if (!(own_stem && adaf_launch_ef_stem(frames_nhwc4 + (size_t)f0 * size * size * 4, net->dtype, nc, size, G.stem_hw, G.stem_hw, G.stem_pad, S.w, net->stem_bank,
                                              S.scale, S.bias, S.cout, ADAF_ACT_SWISH, cur, st)) &&
            (rc = run_dense(net, S, frames_nhwc4 + (size_t)f0 * size * size * 4, false, nc, size, size, G.stem_hw, G.stem_hw, G.stem_pad, ADAF_ACT_SWISH, cur, f16, st)))
            return adaf_fail(h, rc, "effnet: stem launch");
        size_t out_elems = (size_t)G.stem_hw * G.stem_hw * S.cout;
        for (size_t bi = 0; bi < net->blocks.size(); ++bi) {
            if (upto_block >= 0 && (int)bi >= upto_block) break;
            const EfBlock& b = net->blocks[bi];
            const EfGeometry::Block& g = G.blocks[bi];
            const int hw = g.hw, ohw = g.ohw, pbd = g.pad;
            const void* dw_in = cur;
            const EfConv& D = net->convs[b.dwc];
            const EfConv& P = net->convs[b.project];
            const bool skip = b.stride == 1 && b.cin == b.cout;
            out_elems = (size_t)ohw * ohw * b.cout;
            // a launcher that refuses a block the rule gave it hands the block to the next form down: whole -> fused expand -> four launches
            EfForm form = block_form(net, bi, g);
            if (form == EfForm::Whole) {
                // maps small enough for a workgroup to own whole images: the block as ONE launch (mbconv_whole.hip)
                const EfConv& E = net->convs[b.expand];
                if (b.wef && adaf_launch_mbconv_whole(cur, nc, hw, b.stride, b.cin, b.hid, b.cout, b.sq, b.k, b.wef, E.scale, E.bias, b.wdl, b.se_wr,
                                                      b.se_br, b.se_wet, b.se_be, b.wpf, P.scale, P.bias, skip, nxt, st)) {
                    char* t = cur; cur = nxt; nxt = t;
                    continue;
                }
                form = fused_expand_takes(net, bi, g) ? EfForm::FusedExpand : EfForm::FourLaunches;
            }
            int tiles = -1;
            if (form == EfForm::FusedExpand) {
                // expand computed inside the depthwise launch's staging step: no expanded map in HBM
                const EfConv& E = net->convs[b.expand];
                tiles = adaf_launch_dw_expand(cur, nc, hw, hw, b.cin, E.w16, E.scale, E.bias, b.hid, b.k, b.stride, pbd, pbd, ohw, ohw, D.w,
                                              D.scale, D.bias, ADAF_ACT_SWISH, bufD, part, st);
            }
            if (tiles <= 0) {
                if (b.expand >= 0) {
                    // (the expand GEMM stays on the conv engine: routed through gated_project_kernel -- 128 x 128 tiles, swish in its
                    // 16-byte epilogue -- the fp16 network measured 12.6 instead of 11.5 ms)
                    const EfConv& E = net->convs[b.expand];
                    const bool own_expand = (plan & ADAF_EF_PLAN_STRIP_EXPAND) != 0;   // off = the conv engine for every expand (A/B)
                    if (!(own_expand && adaf_launch_ef_expand(cur, net->dtype, (long long)nc * hw * hw, b.cin, f16 ? E.w16 : static_cast<const void*>(E.w),
                                                              E.scale, E.bias, b.hid, ADAF_ACT_SWISH, bufE, h->cus, st)) &&
                        (rc = run_dense(net, E, cur, f16, nc, hw, hw, hw, hw, 0, ADAF_ACT_SWISH, bufE, f16, st)))
                        return adaf_fail(h, rc, "effnet: expand launch (block %zu)", bi);
                    dw_in = bufE;
                }
                tiles = adaf_launch_dw_same(dw_in, net->dtype, nc, hw, hw, b.hid, b.k, b.stride, pbd, pbd, ohw, ohw, D.w, D.scale,
                                            D.bias, ADAF_ACT_SWISH, bufD, part, st);
            }
            if (tiles <= 0) return adaf_fail(h, ADAF_E_LAUNCH, "effnet: depthwise launch (block %zu)", bi);
            adaf_launch_se_gate(part, tiles, ohw * ohw, nc, b.hid, b.se_wr, b.se_br, b.sq, b.se_wet, 1, b.hid, b.se_be, gate, st);
            if (adaf_launch_gated_project(bufD, net->dtype, nc * ohw * ohw, ohw * ohw, b.hid, gate, f16 ? P.w16 : static_cast<const void*>(P.w),
                                          b.cout, P.scale, P.bias, skip ? cur : nullptr, nxt, h->cus, st) < 0)
                return adaf_fail(h, ADAF_E_LAUNCH, "effnet: project launch (block %zu)", bi);
            char* t = cur; cur = nxt; nxt = t;
        }
        if (upto_block >= 0) {
            (void)hipMemcpyAsync(static_cast<char*>(block_out) + (size_t)f0 * out_elems * es, cur, (size_t)nc * out_elems * es,
                                 hipMemcpyDeviceToDevice, st);
            return ADAF_OK;
        }
        const int hw = G.blocks.back().ohw;
        float* fm = featmap ? featmap + (size_t)f0 * hw * hw * net->feat : reinterpret_cast<float*>(bufE);
        // fp16 storage, pooled features only: the head conv with the global average pool in its epilogue (conv_gemm.hip
        // adaf_launch_conv_pool16: no fp32 map -- 157 MB per 1024 patches of 144^2 -- and one launch; the bits of conv + avgpool_kernel)
        if (f16 && featvec && !featmap && (plan & ADAF_EF_PLAN_HEAD_POOL) && net->feat % 4 == 0 && ldvec % 4 == 0) {
            const EfConv& Hc = net->convs[net->head];
            ConvArgs a = adaf_net_conv_args(Hc, Hc.w16, cur, nc, hw, hw, hw, hw, 0, ADAF_ACT_SWISH, nullptr, nullptr, net->h->zeros);
            a.in16 = 1;
            if (adaf_launch_conv_pool16(a, hw * hw, featvec + (size_t)f0 * ldvec, ldvec, st)) return ADAF_OK;
        }
        if ((rc = run_dense(net, net->convs[net->head], cur, f16, nc, hw, hw, hw, hw, 0, ADAF_ACT_SWISH, fm, false, st)))
            return adaf_fail(h, rc, "effnet: head launch");
        if (featvec) {
            if (net->feat % 4 == 0 && ldvec % 4 == 0) adaf_launch_avgpool(fm, nc, hw * hw, net->feat, featvec + (size_t)f0 * ldvec, ldvec, st);
            else adaf_launch_avgpool_any(fm, nc, hw * hw, net->feat, featvec + (size_t)f0 * ldvec, ldvec, st);
        }
        return ADAF_OK;
    };
    const bool pair = (adaf_options().effnet_plan & ADAF_EF_PLAN_PAIR_CHUNKS) != 0;
    if ((rc = adaf_run_chunk_pairs(net->aux, (hipStream_t)stream, n, W.chunk, pair, run_chunk))) return rc;
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? ADAF_OK : adaf_hip_fail(h, e, "effnet forward");
}

// ---- stand-alone ops (tests, and building blocks for other MBConv networks) ---------------------------------------------
int adaf_pack_dw_weight_kxk_f32(adaf_handle* h, const float* w_c1kk, int channels, int k, float* w_kkc, void* stream) {
    if (!h || !w_c1kk || !w_kkc || channels <= 0 || k <= 0) return adaf_fail(h, ADAF_E_BADARG, "pack_dw_kxk: bad argument");
    adaf_launch_pack_dw_kxk(w_c1kk, channels, k, w_kkc, (hipStream_t)stream);
    return ADAF_OK;
}

// the pooled partials of adaf_dwconv_same_bn_act: one sum per (image, tile, channel)
static size_t dwconv_same_layout(void* ws, int n, int hh, int ww, int c, int k, int stride, int dtype, float** part) {
    const int oh = ceil_div(hh, stride), ow = ceil_div(ww, stride);
    const int tiles = adaf_effnet_dw_tiles(c, oh, ow, k, stride, dtype);
    AdafCarver cv(ws);
    // (at least one partial per (image, channel): the tiny-map kernel writes n * c sums whatever the tile planner says -- ADVICE r3)
    *part = cv.take<float>((size_t)n * (tiles > 0 ? tiles : 1) * c);
    return cv.off;
}
size_t adaf_dwconv_same_workspace_bytes(int n, int hh, int ww, int c, int k, int stride, int dtype) {
    float* part;
    return (n <= 0 || hh <= 0 || ww <= 0 || c <= 0 || stride <= 0) ? 0 : dwconv_same_layout(nullptr, n, hh, ww, c, k, stride, dtype, &part);
}

int adaf_dwconv_same_bn_act(adaf_handle* h, const void* x, int dtype, int n, int hh, int ww, int c, int k, int stride, const float* w_kkc,
                            const float* scale, const float* bias, int act, void* out, float* pool_mean, void* ws, size_t ws_bytes,
                            void* stream) {
    if (!h || !x || !w_kkc || !scale || !bias || !out) return adaf_fail(h, ADAF_E_BADARG, "dwconv_same: null pointer");
    if (n <= 0 || hh <= 0 || ww <= 0 || c <= 0 || (k != 3 && k != 5) || (stride != 1 && stride != 2))
        return adaf_fail(h, ADAF_E_BADARG, "dwconv_same: k in {3, 5}, stride in {1, 2}");
    if (dtype != ADAF_DTYPE_F32 && dtype != ADAF_DTYPE_F16) return adaf_fail(h, ADAF_E_BADARG, "dwconv_same: dtype");
    if (c % (dtype == ADAF_DTYPE_F16 ? 8 : 4)) return adaf_fail(h, ADAF_E_LAYOUT, "dwconv_same: channels must fill 16-byte chunks");
    if (act < ADAF_ACT_NONE || act > ADAF_ACT_SWISH) return adaf_fail(h, ADAF_E_BADARG, "dwconv_same: activation");
    int ty, tx;
    const int pt = same_pad(hh, k, stride, &ty), pl = same_pad(ww, k, stride, &tx);
    const int oh = ceil_div(hh, stride), ow = ceil_div(ww, stride);
    float* part = nullptr;
    if (pool_mean) {        // (only the pooled means have a workspace)
        if (!ws) return adaf_fail(h, ADAF_E_NOMEM, "dwconv_same: workspace");
        const int rc = adaf_check_ws(h, "dwconv_same", ws, ws_bytes, dwconv_same_layout(ws, n, hh, ww, c, k, stride, dtype, &part), ADAF_WS_ALIGN_FIRST);
        if (rc) return rc;
    }
    const int tiles = adaf_launch_dw_same(x, dtype, n, hh, ww, c, k, stride, pt, pl, oh, ow, w_kkc, scale, bias, act, out, part, (hipStream_t)stream);
    if (tiles <= 0) return adaf_fail(h, ADAF_E_LAYOUT, "dwconv_same: shape not supported");
    if (pool_mean) adaf_launch_pool_finish(part, n, tiles, c, oh * ow, pool_mean, (hipStream_t)stream);
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? ADAF_OK : adaf_hip_fail(h, e, "dwconv_same");
}

int adaf_se_gate_f32(adaf_handle* h, const float* pool_mean, int n, int c, const float* w_reduce, const float* b_reduce, int squeezed,
                     const float* w_expand, const float* b_expand, float* gate, void* stream) {
    if (!h || !pool_mean || !w_reduce || !b_reduce || !w_expand || !b_expand || !gate) return adaf_fail(h, ADAF_E_BADARG, "se_gate: null pointer");
    if (n <= 0 || c <= 0 || c % 4 || squeezed <= 0 || (size_t)(c + squeezed) * 16 > 60 * 1024) return adaf_fail(h, ADAF_E_BADARG, "se_gate: extents (c %% 4 == 0)");
    adaf_launch_se_gate(pool_mean, 1, 1, n, c, w_reduce, b_reduce, squeezed, w_expand, squeezed, 1, b_expand, gate, (hipStream_t)stream);
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? ADAF_OK : adaf_hip_fail(h, e, "se_gate");
}

int adaf_conv1x1_gated_bn(adaf_handle* h, const void* x, int dtype, int n_images, int hw, int cin, const float* gate, const void* w,
                          int cout, const float* scale, const float* bias, const void* residual, void* out, void* stream) {
    if (!h || !x || !w || !out) return adaf_fail(h, ADAF_E_BADARG, "conv1x1_gated: null pointer");
    if (dtype != ADAF_DTYPE_F32 && dtype != ADAF_DTYPE_F16) return adaf_fail(h, ADAF_E_BADARG, "conv1x1_gated: dtype");
    if (n_images <= 0 || hw <= 0 || cin <= 0 || cout <= 0 || cin % (dtype == ADAF_DTYPE_F16 ? 8 : 4))
        return adaf_fail(h, ADAF_E_LAYOUT, "conv1x1_gated: cin must fill 16-byte chunks");
    if ((long long)n_images * hw > 0x7fffffffLL) return adaf_fail(h, ADAF_E_BADARG, "conv1x1_gated: too many rows");
    if (adaf_launch_gated_project(x, dtype, n_images * hw, hw, cin, gate, w, cout, scale, bias, residual, out, h->cus, (hipStream_t)stream) < 0)
        return adaf_fail(h, ADAF_E_LAYOUT, "conv1x1_gated: shape not supported");
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? ADAF_OK : adaf_hip_fail(h, e, "conv1x1_gated");
}

}  // extern "C"
