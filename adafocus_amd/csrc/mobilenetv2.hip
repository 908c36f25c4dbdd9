// MobileNetV2 feature extractor (the glancer) as one object on the
// conv engine + the depthwise kernel.  ACT/models/mobilenet.py:71-148 and STH/models/mobilenetv2.py
// (with the temporal shift of STH/models/gfv_net.py:238-241 on the expand conv of residual blocks).
//
// Per inverted-residual block: expand 1x1 (+BN+ReLU6) on the MFMA engine, depthwise 3x3 (+BN+ReLU6)
// on the VALU kernel, project 1x1 (+BN, + residual in the epilogue) on the MFMA engine.  Frames are
// processed in chunks so the 6x-expanded intermediates stay within a bounded workspace.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "adaf_net.h"

using MbConv = AdafNetConv;   // "stem", "b3.expand", "b3.dw", "b3.project", "head"

struct MbBlock {
    int inp, oup, stride, t;
    int expand, dw, project;   // indices into convs (-1 = absent)
};

struct adaf_mobilenetv2 {
    adaf_handle* h = nullptr;
    AdafParamTable params;  // what set_param registered since the last finalize
    AdafWeightArena arena;  // every packed buffer of convs
    std::vector<MbConv> convs;
    std::vector<MbBlock> blocks;
    int stem = 0, head = 0;
    bool fuse = true;       // expand -> depthwise in one kernel where the shape allows (mbconv.hip)
    bool whole = true;      // ... and the whole stride-1 block (expand -> depthwise -> project + identity) where that shape allows
    bool finalized = false;
    // Two frame chunks travel through the network side by side (the second on this library-owned stream, forked from and
    // joined to the caller's stream by events -- still fully asynchronous): the tail's launches are 30-100 us each and
    // leave the device half empty on their own; a neighbour fills the ramps and tails.
    // One helper stream + event pair PER CALLER STREAM: forwards issued from different streams (pipelined batches,
    // bench --streams) must not serialise their second chunks on one shared helper.
    AdafAuxPool aux;        // (adaf_internal.h: LRU over caller streams, mutex-guarded)
    bool pair = true;
};

namespace {

const int kSetting[7][4] = {{1, 16, 1, 1}, {6, 24, 2, 2}, {6, 32, 3, 2}, {6, 64, 4, 2}, {6, 96, 3, 1}, {6, 160, 3, 2}, {6, 320, 1, 1}};

inline int cdiv_out(int in, int k, int stride, int pad) { return (in + 2 * pad - k) / stride + 1; }

void build(adaf_mobilenetv2* net) {
    net->convs.clear();
    net->blocks.clear();
    net->stem = 0;
    net->convs.push_back(adaf_net_conv("stem", 3, 32, 3, 2, false, 4));
    int cin = 32, bi = 1;
    for (auto& s : kSetting) {
        for (int i = 0; i < s[2]; ++i, ++bi) {
            MbBlock b{cin, s[1], i == 0 ? s[3] : 1, s[0], -1, -1, -1};
            const int hid = cin * s[0];
            char nm[32];
            if (s[0] != 1) {
                snprintf(nm, sizeof(nm), "b%d.expand", bi);
                b.expand = (int)net->convs.size();
                net->convs.push_back(adaf_net_conv(nm, cin, hid, 1, 1, false, cin));
            }
            snprintf(nm, sizeof(nm), "b%d.dw", bi);
            b.dw = (int)net->convs.size();
            net->convs.push_back(adaf_net_conv(nm, hid, hid, 3, b.stride, true, hid));
            snprintf(nm, sizeof(nm), "b%d.project", bi);
            b.project = (int)net->convs.size();
            net->convs.push_back(adaf_net_conv(nm, hid, s[1], 1, 1, false, hid));
            net->blocks.push_back(b);
            cin = s[1];
        }
    }
    net->head = (int)net->convs.size();
    net->convs.push_back(adaf_net_conv("head", cin, 1280, 1, 1, false, cin));
}

// floats per frame of the four chunk buffers (block in/out ping-pong, expanded, depthwise out)
void slab_sizes(const adaf_mobilenetv2* net, int size, size_t* io, size_t* ex, size_t* dw) {
    int hw = cdiv_out(size, 3, 2, 1);
    *io = (size_t)hw * hw * 32;
    *ex = 0;
    *dw = 0;
    for (auto& b : net->blocks) {
        const int hid = b.inp * b.t;
        const int ohw = cdiv_out(hw, 3, b.stride, 1);
        if (b.t != 1 && (size_t)hw * hw * hid > *ex) *ex = (size_t)hw * hw * hid;
        if ((size_t)ohw * ohw * hid > *dw) *dw = (size_t)ohw * ohw * hid;
        if ((size_t)ohw * ohw * b.oup > *io) *io = (size_t)ohw * ohw * b.oup;
        hw = ohw;
    }
    if ((size_t)hw * hw * 32 > *ex) *ex = (size_t)hw * hw * 32;
}

int chunk_size() {   // frames per pass through the network (ADAF_MBV2_CHUNK overrides, for tuning)
    const int c = adaf_options().mbv2_chunk;
    return c;
}

int chunk_frames(int n, int tsm_segments) {
    const int kChunk = chunk_size();
    int c = n < kChunk ? n : kChunk;
    // a batch that fits one chunk but is large enough for two halves to fill the machine each (>= 256 frames) travels as a PAIR of half
    // chunks on the two streams like any larger batch does: 512 frames (the Something-Something glancer at 64 clips x 8) 5.15 -> 4.9 ms
    // (tools/glancer_chunk_ab.py); a frame's arithmetic does not depend on the chunk it travels in
    const bool halve = n <= kChunk && n >= 512;
    if (halve) c = (n + 1) / 2;
    if (tsm_segments > 0) {
        if (halve) c += (tsm_segments - c % tsm_segments) % tsm_segments;     // whole clips per chunk: round the half UP
        else c -= c % tsm_segments;
        if (c <= 0) c = tsm_segments;
    }
    return c;
}

// The workspace, stated once: per chunk A and B (block in / out ping-pong), E (expanded), D (depthwise out), packed; a batch of more than
// one chunk has two chunks in flight and a second set behind the first.  With ws == nullptr it only measures (the query).
struct MbSlabs { float *A, *B, *E, *D; };
struct MbWorkspace { int chunk; size_t bytes; MbSlabs slot[2]; };
MbWorkspace workspace_layout(const adaf_mobilenetv2* net, int n, int size, int tsm_segments, void* ws) {
    size_t io, ex, dw;
    slab_sizes(net, size, &io, &ex, &dw);
    MbWorkspace w = {};
    w.chunk = chunk_frames(n, tsm_segments);
    const int slots = n > w.chunk ? 2 : 1;       // two chunks in flight (whether or not the pairing is switched on)
    AdafCarver c(ws);
    for (int i = 0; i < slots; ++i) {
        w.slot[i].A = c.take<float>((size_t)w.chunk * io);
        w.slot[i].B = c.take<float>((size_t)w.chunk * io);
        w.slot[i].E = c.take<float>((size_t)w.chunk * ex);
        w.slot[i].D = c.take<float>((size_t)w.chunk * dw);
    }
    w.bytes = c.off;
    return w;
}

// The launch form of block `bidx` on a `hw` x `hw` input map, from the frame size, the map and the options alone.  THE decision: the forward
// launches what it says and adaf_mobilenetv2_block_forms reports it (include/adafocus.h has the codes).  Block 0 stands for the stem + block 1
// pair (hw = the stem's output side): one kernel, on strips or on wave-private tiles -- or the stem conv and block 1 as launches of their own.
enum { MB_UNFUSED = 0, MB_TILE_XD = 1, MB_TILE_WHOLE = 2, MB_STRIP_WHOLE = 3, MB_STRIP_XD = 4 };
enum { MB_SHIFT_NONE = 0, MB_SHIFT_STRIP = 1, MB_SHIFT_OPERAND = 2, MB_SHIFT_COPY = 3 };
struct MbForm { int form, shift; };

MbForm block_form(const adaf_mobilenetv2* net, size_t bidx, int size, int hw, int tsm_segments, int tsm_div) {
    const MbBlock& b = net->blocks[bidx];
    MbForm f = {MB_UNFUSED, MB_SHIFT_NONE};
    if (bidx == 0) {
        if (net->fuse && b.t == 1 && b.inp == 32 && b.oup == 16 && b.stride == 1) f.form = adaf_mb_stem_b1_strip_ok(size, hw) ? MB_STRIP_WHOLE : MB_TILE_WHOLE;
        return f;
    }
    if (b.expand < 0) return f;
    const int hid = b.inp * b.t;
    const bool tile_xd = net->fuse && adaf_mb_expand_dw_ok(b.inp, hid, hw);
    // the 14 x 14 blocks (64 / 96 input channels): expand -> depthwise on strips (mbstrip.hip), the project conv stays on the engine
    const bool strip_xd = net->fuse && net->whole && !tile_xd && adaf_mb_expand_dw_strip_ok(b.inp, hid, b.stride, hw, hw);
    if (tile_xd || strip_xd) {
        // the whole block in one launch: neither expanded map reaches HBM
        if (net->whole && adaf_mb_block_ok(b.inp, hid, b.oup, b.stride, hw) && net->convs[b.project].cin_pad == hid)
            f.form = adaf_mb_block_strip_ok(b.inp, hid, b.oup, b.stride, hw, hw) ? MB_STRIP_WHOLE : MB_TILE_WHOLE;
        else f.form = strip_xd ? MB_STRIP_XD : MB_TILE_XD;
    }
    if (tsm_segments > 0 && b.stride == 1 && b.inp == b.oup) {      // STH/models/gfv_net.py:238-241: residual blocks
        // the expand -> depthwise strip kernel, whose lanes load whole 4-channel groups of one shift kind (fold % 4 == 0: the 64- / 96-channel blocks):
        // the shift rides in their pixel loads (MbFuseArgs::tsm_T), nothing is materialised and the identity rows are the input itself
        // (the whole-block strip kernel of the 32-channel blocks has no register left for the frame offset: 252 of 256; its input stays materialised)
        // (the kernel gives a frame offset to the first CIN / 4 channels of a pixel only, mbstrip.hip dsh[]: both shifted folds must lie inside them
        //  -- shift_div >= 8; a wider fold falls through to the materialised copy the whole-block strips read)
        const int fold = b.inp / tsm_div;
        if (f.form == MB_STRIP_XD && fold % 4 == 0 && 2 * fold <= b.inp / 4) f.shift = MB_SHIFT_STRIP;
        else if (f.form == MB_UNFUSED && fold % 4 == 0) f.shift = MB_SHIFT_OPERAND;     // shift fused into the operand load
        else f.shift = MB_SHIFT_COPY;   // fold not a multiple of 4 channels (24-channel block), or a fused kernel: materialise the shift once
    }
    return f;
}

int run_conv(adaf_mobilenetv2* net, const MbConv& L, const float* in, int n, int hh, int ww, int act, const float* res,
             float* out, int tsm_T, int tsm_div, hipStream_t st) {
    const int oh = cdiv_out(hh, L.k, L.stride, L.k / 2), ow = cdiv_out(ww, L.k, L.stride, L.k / 2);
    ConvArgs a = adaf_net_conv_args(L, L.w, in, n, hh, ww, oh, ow, L.k / 2, act, res, out, net->h->zeros);
    a.tsm_T = tsm_T; a.tsm_fold = tsm_T > 0 ? L.cin / tsm_div : 0; a.tsm_hw = hh * ww;
    return adaf_launch_conv_gemm(a, 0, net->h->cus, st) > 0 ? ADAF_OK : ADAF_E_LAUNCH;
}

}  // namespace

extern "C" {

int adaf_mobilenetv2_create(adaf_handle* h, adaf_mobilenetv2** out) {
    if (!h || !out) return ADAF_E_BADARG;
    adaf_mobilenetv2* net = new adaf_mobilenetv2();
    net->h = h;
    build(net);
    *out = net;
    return ADAF_OK;
}

int adaf_mobilenetv2_destroy(adaf_mobilenetv2* net) {
    if (!net) return ADAF_OK;
    net->aux.destroy();
    net->arena.release();
    delete net;
    return ADAF_OK;
}

int adaf_mobilenetv2_set_fusion(adaf_mobilenetv2* net, int on) {
    if (!net) return ADAF_E_BADARG;
    net->fuse = (on & 1) != 0;
    net->pair = (on & 4) == 0;     // bit 2 set: one frame chunk at a time (A/B)
    net->whole = (on & 8) == 0;    // bit 3 set: expand -> depthwise kernel + project launch instead of the whole-block kernel (A/B)
    return ADAF_OK;
}

int adaf_mobilenetv2_set_param(adaf_mobilenetv2* net, const char* name, const float* dev_ptr, size_t numel) {
    if (!net || !name || !dev_ptr) return ADAF_E_BADARG;
    net->params.set(name, dev_ptr, numel);
    net->finalized = false;
    return ADAF_OK;
}

int adaf_mobilenetv2_finalize(adaf_mobilenetv2* net, void* stream) {
    if (!net) return ADAF_E_BADARG;
    adaf_handle* h = net->h;
    hipStream_t st = (hipStream_t)stream;
    int rc = ADAF_OK;
    for (size_t i = 0; i < net->convs.size() && !rc; ++i) rc = adaf_pack_conv_bn(h, "mobilenetv2", net->params, net->arena, net->convs[i], 1e-5f, st);
    net->params.clear();        // a registration lives until here, whatever finalize returns (include/adafocus.h)
    if (rc) return rc;
    hipError_t e = hipStreamSynchronize(st);
    if (e != hipSuccess) return adaf_hip_fail(h, e, "mobilenetv2 finalize");
    net->aux.prepare(4);        // helper streams exist before the first forward (which may be captured into a HIP graph)
    net->finalized = true;
    return ADAF_OK;
}

size_t adaf_mobilenetv2_workspace_bytes(const adaf_mobilenetv2* net, int n, int size, int tsm_segments) {
    return (!net || n <= 0 || size <= 0) ? 0 : workspace_layout(net, n, size, tsm_segments, nullptr).bytes;
}

int adaf_mobilenetv2_block_forms(const adaf_mobilenetv2* net, int size, int tsm_segments, int tsm_div, int* forms, int count) {
    if (!net || !forms) return ADAF_E_BADARG;
    if (size < 32 || count < (int)net->blocks.size()) return adaf_fail(net->h, ADAF_E_BADARG, "mobilenetv2 block_forms: need size >= 32 and room for 17 entries");
    if (tsm_segments > 0 && tsm_div <= 0) return adaf_fail(net->h, ADAF_E_BADARG, "mobilenetv2 block_forms: tsm_div <= 0");
    int hw = cdiv_out(size, 3, 2, 1);
    for (size_t bidx = 0; bidx < net->blocks.size(); ++bidx) {
        const MbForm f = block_form(net, bidx, size, hw, tsm_segments, tsm_div);
        forms[bidx] = f.form | (f.shift << 4);
        hw = cdiv_out(hw, 3, net->blocks[bidx].stride, 1);
    }
    return ADAF_OK;
}

int adaf_mobilenetv2_forward(adaf_mobilenetv2* net, const float* frames_nhwc4, int n, int size, int tsm_segments,
                             int tsm_div, float* featmap, float* featvec, int ldvec, void* ws, size_t ws_bytes,
                             void* stream) {
    if (!net) return ADAF_E_BADARG;
    adaf_handle* h = net->h;
    if (!net->finalized) return adaf_fail(h, ADAF_E_STATE, "mobilenetv2: finalize() has not been called");
    if (!frames_nhwc4 || !featmap || !ws) return adaf_fail(h, ADAF_E_BADARG, "mobilenetv2: null pointer");
    if (n <= 0 || size < 32) return adaf_fail(h, ADAF_E_BADARG, "mobilenetv2: need n > 0 and size >= 32");
    if (tsm_segments > 0 && (n % tsm_segments || tsm_div <= 0)) return adaf_fail(h, ADAF_E_BADARG, "mobilenetv2: n %% tsm_segments != 0");
    if (featvec && (ldvec < 1280 || ldvec % 4)) return adaf_fail(h, ADAF_E_LAYOUT, "mobilenetv2: ldvec >= 1280 and %% 4 == 0 required");
    const MbWorkspace W = workspace_layout(net, n, size, tsm_segments, ws);
    int rc = adaf_check_ws(h, "mobilenetv2", ws, ws_bytes, W.bytes, ADAF_WS_ALIGN_FIRST);
    if (rc) return rc;

    // one chunk of frames through the whole network on stream `st` with its own slot of the workspace
    auto run_chunk = [&](int f0, int nc, int slot, hipStream_t st) -> int {
        float *const bufA = W.slot[slot].A, *const bufB = W.slot[slot].B, *const bufE = W.slot[slot].E, *const bufD = W.slot[slot].D;
        int hw = cdiv_out(size, 3, 2, 1);
        int rc;
        float* cur = bufA;
        float* nxt = bufB;
        size_t first_block = 0;
        const int sform = block_form(net, 0, size, hw, tsm_segments, tsm_div).form;
        if (sform != MB_UNFUSED) {      // stem + block 1 in one kernel: the two 32-channel maps at the stem's resolution never reach HBM
            const MbBlock& b1 = net->blocks[0];
            const MbConv &S = net->convs[net->stem], &D = net->convs[b1.dw], &P = net->convs[b1.project];
            MbStemArgs sa;
            memset(&sa, 0, sizeof(sa));
            sa.x = frames_nhwc4 + (size_t)f0 * size * size * 4; sa.n = nc; sa.S = size; sa.H1 = hw;
            sa.ws = S.w; sa.ss = S.scale; sa.bs = S.bias; sa.wd = D.w; sa.sd = D.scale; sa.bd = D.bias;
            sa.wp = P.w; sa.sp = P.scale; sa.bp = P.bias; sa.out = bufA; sa.zeros = net->h->zeros;
            if (sform == MB_STRIP_WHOLE) adaf_launch_mb_stem_b1_strip(sa, st);
            else adaf_launch_mb_stem_b1_tile(sa, st);
            first_block = 1;
        } else if ((rc = run_conv(net, net->convs[net->stem], frames_nhwc4 + (size_t)f0 * size * size * 4, nc, size, size,
                                  ADAF_ACT_RELU6, nullptr, bufA, 0, 0, st)))
            return adaf_fail(h, rc, "mobilenetv2: stem launch");
        for (size_t bidx = first_block; bidx < net->blocks.size(); ++bidx) {
            const MbBlock& b = net->blocks[bidx];
            const int hid = b.inp * b.t;
            const bool residual = b.stride == 1 && b.inp == b.oup;
            const float* dw_in = cur;
            const MbConv& D = net->convs[b.dw];
            const MbForm f = block_form(net, bidx, size, hw, tsm_segments, tsm_div);      // (bidx 0: block 1 behind the stem conv, unfused)
            const bool fused = f.form != MB_UNFUSED;
            if (b.expand >= 0) {
                const MbConv& E = net->convs[b.expand];
                const float* ein = cur;
                if (f.shift == MB_SHIFT_COPY) {      // into the slab the block's own launches leave free
                    float* sh = fused ? bufE : bufD;
                    adaf_launch_tshift(cur, nc, b.inp, hw * hw, tsm_segments, tsm_div, ADAF_LAYOUT_NHWC, sh, st);
                    ein = sh;
                }
                if (fused) {
                    MbFuseArgs fa;
                    memset(&fa, 0, sizeof(fa));
                    fa.x = ein; fa.n = nc; fa.H = hw; fa.W = hw; fa.cin = b.inp;
                    fa.we = E.w; fa.se = E.scale; fa.be = E.bias; fa.wd = D.w; fa.sd = D.scale; fa.bd = D.bias;
                    fa.out = bufD; fa.hid = hid; fa.OH = fa.OW = cdiv_out(hw, 3, b.stride, 1);
                    fa.zeros = net->h->zeros;
                    fa.tsm_T = f.shift == MB_SHIFT_STRIP ? tsm_segments : 0; fa.tsm_fold = fa.tsm_T ? b.inp / tsm_div : 0;
                    if (f.form == MB_STRIP_WHOLE || f.form == MB_TILE_WHOLE) {
                        const MbConv& P = net->convs[b.project];
                        fa.wp = P.w; fa.sp = P.scale; fa.bp = P.bias; fa.cout = b.oup;
                        fa.res = residual ? cur : nullptr;
                        fa.out2 = nxt;
                        if (f.form == MB_STRIP_WHOLE) adaf_launch_mb_block_strip(fa, st);
                        else adaf_launch_mb_block_tile(fa, st);
                        float* t = cur; cur = nxt; nxt = t;
                        hw = fa.OH;
                        continue;
                    }
                    if (f.form == MB_STRIP_XD) adaf_launch_mb_expand_dw_strip(fa, st);
                    else adaf_launch_mb_expand_dw(fa, b.stride, st);
                } else {
                    if ((rc = run_conv(net, E, ein, nc, hw, hw, ADAF_ACT_RELU6, nullptr, bufE, f.shift == MB_SHIFT_OPERAND ? tsm_segments : 0, tsm_div, st)))
                        return adaf_fail(h, rc, "mobilenetv2: expand launch");
                    dw_in = bufE;
                }
            }
            if (!fused) adaf_launch_dwconv3x3(dw_in, nc, hw, hw, hid, b.stride, D.w, D.scale, D.bias, ADAF_ACT_RELU6, bufD, st);
            const int ohw = cdiv_out(hw, 3, b.stride, 1);
            if ((rc = run_conv(net, net->convs[b.project], bufD, nc, ohw, ohw, ADAF_ACT_NONE, residual ? cur : nullptr, nxt, 0,
                               0, st)))
                return adaf_fail(h, rc, "mobilenetv2: project launch");
            float* t = cur; cur = nxt; nxt = t;
            hw = ohw;
        }
        float* fm = featmap + (size_t)f0 * hw * hw * 1280;
        if ((rc = run_conv(net, net->convs[net->head], cur, nc, hw, hw, ADAF_ACT_RELU6, nullptr, fm, 0, 0, st)))
            return adaf_fail(h, rc, "mobilenetv2: head launch");
        if (featvec) adaf_launch_avgpool(fm, nc, hw * hw, 1280, featvec + (size_t)f0 * ldvec, ldvec, st);
        return ADAF_OK;
    };
    if ((rc = adaf_run_chunk_pairs(net->aux, (hipStream_t)stream, n, W.chunk, net->pair, run_chunk))) return rc;
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? ADAF_OK : adaf_hip_fail(h, e, "mobilenetv2 forward");
}

}  // extern "C"
