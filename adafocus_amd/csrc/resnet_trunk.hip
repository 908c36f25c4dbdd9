// The ResNet trunk behind adaf_resnet50_* (include/adafocus.h; the Bottleneck stacks of ResNet-50, -101 and -152): parameter packing,
// the launch plan and ONE block walk for the three arithmetics (ADAF_MATH_*).  Host code only -- the kernels are in conv_gemm.hip,
// conv_lat.hip, stem.hip, misc_ops.hip and crop.hip.  No PyTorch types, no allocation in forward calls.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "adaf_net.h"

struct ConvLayer : AdafNetConv {     // (w16: the packed bank rounded to fp16, nearest-even -- ADAF_MATH_F16 only; not for the stem)
    int pad;
    bool tsm = false;      // a Bottleneck conv1 that the 'blockres' temporal shift wraps (make_temporal_shift's n_round rule)
    unsigned short* wsp = nullptr;   // the packed bank as three bf16 planes (ADAF_MATH_F32_SPLIT_BF16 only)
};

struct adaf_resnet50 {
    adaf_handle* h = nullptr;
    AdafParamTable params;         // what set_param registered since the last finalize
    AdafWeightArena arena;         // every packed buffer below and in convs
    std::vector<ConvLayer> convs;  // [0] = stem, then per block conv1, conv2, conv3, (downsample)
    std::vector<int> tiles;        // per conv launch override
    int blocks[4] = {3, 4, 6, 3};  // Bottlenecks per stage: ResNet-50, -101 or -152 (inferred from the parameter names at finalize)
    // layer1.0's conv1 (64 -> 64) and downsample (64 -> 256) read the same map with the same 1x1 / stride-1 geometry: their
    // filter banks and BN affines concatenated along the output channels, for one launch instead of two (run_trunk)
    float* l10_w = nullptr;
    float* l10_scale = nullptr;
    float* l10_bias = nullptr;
    unsigned short* l10_w16 = nullptr;   // l10_w rounded to fp16 (ADAF_MATH_F16)
    int math = ADAF_MATH_F32;      // ADAF_MATH_*: which matrix pipe the (non-stem) convs use
    bool fuse = true;              // stage 1: conv2 -> conv3 (-> next conv1) in one launch; stem + max-pool in one launch
    bool fuse_stem_always = false; // (tests, set_fusion(2)) take every fused launch at every size, not only where it is the faster plan
    bool tsm_block = false;        // temporal shift in front of the WHOLE Bottleneck (shift_place = 'block') instead of its conv1 ('blockres')
    int lat_rows = -1;             // convs with at most this many GEMM rows take the small-batch form (-1 = the "latency_rows" option, 1536)
    float* stem_w = nullptr;       // filter bank in the stem kernel's layout (stem.hip)
    bool finalized = false;
};

namespace {

const int kStagePlanes[4] = {64, 128, 256, 512};
// the Bottleneck depths the trunk runs (torchvision's resnet50 / resnet101 / resnet152, ACT/models/resnet.py:280-315)
const int kDepths[3][4] = {{3, 4, 6, 3}, {3, 4, 23, 3}, {3, 8, 36, 3}};

int total_blocks(const adaf_resnet50* net) { return net->blocks[0] + net->blocks[1] + net->blocks[2] + net->blocks[3]; }

void build_layers(adaf_resnet50* net) {
    net->convs.clear();
    auto add = [&](const std::string& name, const std::string& bn, int cin, int cout, int k, int stride, int pad, int cin_pad, bool tsm = false) {
        net->convs.push_back({{name, bn, cin, cout, k, stride, false, cin_pad}, pad, tsm});
    };
    add("conv1", "bn1", 3, 64, 7, 2, 3, 4);
    // make_temporal_shift, place 'blockres' (STH/ops/temporal_shift.py:122-136): a layer3 of 23 or more blocks gives n_round = 2,
    // and block i of every stage has its conv1 shifted iff i % n_round == 0
    const int n_round = net->blocks[2] >= 23 ? 2 : 1;
    int inplanes = 64;
    for (int s = 0; s < 4; ++s) {
        const int planes = kStagePlanes[s];
        for (int b = 0; b < net->blocks[s]; ++b) {
            char pre[32];
            snprintf(pre, sizeof(pre), "layer%d.%d.", s + 1, b);
            const int stride = (b == 0 && s > 0) ? 2 : 1;
            const std::string p(pre);
            add(p + "conv1", p + "bn1", inplanes, planes, 1, 1, 0, inplanes, b % n_round == 0);
            add(p + "conv2", p + "bn2", planes, planes, 3, stride, 1, planes);
            add(p + "conv3", p + "bn3", planes, planes * 4, 1, 1, 0, planes);
            if (b == 0) add(p + "downsample.0", p + "downsample.1", inplanes, planes * 4, 1, stride, 0, inplanes);
            inplanes = planes * 4;
        }
    }
    net->tiles.assign(net->convs.size(), 0);
}

struct Launch {   // one enqueued kernel of the forward pass, for the profiler
    double flops, bytes;
    int tile;
};

// Where the trunk's patches come from when the stem gathers them itself (adaf_resnet50_forward_frames)
struct FrameSrc {
    const float* frames;    // [nframes, 3, H, W] planar or [nframes, H, W, 4] pixel-major
    bool pixel_major;
    int nframes, H, W;
    const float* act;       // [n / fpa, 2] fp32 (y, x)
    int fpa;
};

// The conv description of layer L over n maps of hh x ww; shift, tile and strides are the caller's.
adaf_conv_params layer_params(const ConvLayer& L, int n, int hh, int ww, int act) {
    adaf_conv_params p;
    memset(&p, 0, sizeof(p));
    p.n = n; p.h = hh; p.w = ww; p.cin = L.cin_pad; p.cout = L.cout; p.kh = p.kw = L.k; p.stride = L.stride; p.pad = L.pad;
    p.act = act;
    return p;
}

// The workspace, stated once: five slabs (block input, block output, two bottleneck temporaries, downsample branch), each as
// large as the biggest activation: the stem output or the first stage's 256-channel map; a sixth for the
// shifted block input when the temporal shift wraps whole blocks (adaf_resnet50_set_shift_place).  ws == nullptr: only measures
// (adaf_resnet50_workspace_bytes, which may be asked without a net: five slabs).
size_t trunk_layout(const adaf_resnet50* net, int n, int patch, void* ws, float* buf[6]) {
    const int s1 = adaf_conv_out(patch, 7, 2, 3), s2 = adaf_conv_out(s1, 3, 2, 1);
    const size_t a = (size_t)s1 * s1 * 64, b = (size_t)s2 * s2 * 256;
    AdafCarver c(ws);
    for (int i = 0; i < 6; ++i) buf[i] = (i < 5 || (net && net->tsm_block)) ? c.take<float>((a > b ? a : b) * n) : nullptr;
    return c.off;
}

inline const float* as_f32(const void* p) { return static_cast<const float*>(p); }   // fp16 buffers travel as float* through ConvArgs

// Walks the trunk in the arithmetic net->math names; `rec` (optional) gets one hipEvent before each launch plus one at the end.
int walk_trunk(adaf_resnet50* net, const float* x4, int n, int P, int tsm_T, int tsm_div, float* feat, int ldfeat,
               void* ws, size_t ws_bytes, hipStream_t st, std::vector<hipEvent_t>* rec, std::vector<Launch>* info, float* featmap,
               const FrameSrc* src) {
    adaf_handle* h = net->h;
    if (src) x4 = src->frames;
    if (!net->finalized) return adaf_fail(h, ADAF_E_STATE, "resnet50: finalize() has not been called");
    if (!x4 || !feat || !ws) return adaf_fail(h, ADAF_E_BADARG, "resnet50: null pointer");
    if (n <= 0 || P < 32) return adaf_fail(h, ADAF_E_BADARG, "resnet50: need n > 0 and patch >= 32");
    if (ldfeat == 0) ldfeat = 2048;
    if (ldfeat < 2048 || ldfeat % 4 || !adaf_aligned16(feat) || !adaf_aligned16(x4) || !adaf_aligned16(ws))
        return adaf_fail(h, ADAF_E_LAYOUT, "resnet50: ldfeat >= 2048, %% 4 == 0 and 16-byte aligned buffers required");
    if (tsm_T > 0 && n % tsm_T) return adaf_fail(h, ADAF_E_BADARG, "resnet50: n=%d not a multiple of tsm_segments=%d", n, tsm_T);
    float* buf[6];
    // (a misaligned workspace was refused above, in front of the shift check: the order of the codes is part of the entry point's behaviour)
    if (int rc = adaf_check_ws(h, "resnet50", ws, ws_bytes, trunk_layout(net, n, P, ws, buf), ADAF_WS_ALIGN_FIRST)) return rc;

    // Small problems (BASELINE config 1: B*T = 16 patches -> 576 / 144 output pixels in stages 3 / 4): a conv whose GEMM has at most
    // `lat_rows` rows is as long as ONE accumulator chain on the engine, and runs on the latency form instead (conv_lat.hip:
    // v_mfma_f32_16x16x4_f32 chains, 3.2x shorter and bit-identical).  ADAF_LATENCY_ROWS: the row limit (0 = never).
    const int lat_rows = net->lat_rows >= 0 ? net->lat_rows : adaf_options().latency_rows;
    const bool lat_ok = lat_rows > 0 && tsm_T == 0 && net->math == ADAF_MATH_F32;     // (run_trunk's tsm_T: either shift placement)
    const bool fuse = net->fuse;
    const bool beside = adaf_launches_beside(h, st);      // the handle has work in flight on another stream: this forward's launches overlap it
    // shift_place = 'block' (STH/ops/temporal_shift.py:104-121): TemporalShift wraps the whole Bottleneck, so conv1, the downsample
    // conv AND the identity see the shifted block input.  The shifted map is materialised in a sixth slab in front of every block and
    // the block then runs exactly as a block without a shift (every fused form applies, except the next block's conv1 riding in a
    // fused tail: it needs the SHIFTED output).  'blockres' (every shipped configuration) keeps the shift inside conv1's operand load.
    // The 64-plane stage is HBM-bound layer by layer, whatever the matrix pipe: its fused launches (conv1 + downsample of layer1.0;
    // conv2 -> conv3 -> next conv1 per block) exist on the fp32 pipe only, and the opt-in split-bf16 arithmetic takes them too --
    // 2.30 ms against 2.41 ms for the ten split launches they replace (option "split_stage1_f32" = 0: A/B).  Every product of such a
    // plan is either an exact fp32 FMA chain or the 6-product bf16 form: fp32-level accuracy throughout.
    const bool stage1_f32 = net->math == ADAF_MATH_F32 || (net->math == ADAF_MATH_F32_SPLIT_BF16 && adaf_options().split_stage1_f32);
    const bool tsm_block = net->tsm_block && tsm_T > 0;
    const int tsm_c1 = tsm_block ? 0 : tsm_T;     // the temporal shift conv1's operand load carries

    // The fp16 trunk (ADAF_MATH_F16, include/adafocus.h: numerics contract).  Same slabs as the fp32 plan (an fp16 map takes half of one), same
    // block walk: stem + max-pool with an fp16 store, then every conv on the fp16-operand tiles (conv_gemm.hip, tile ids 81..84 / 88: fp16
    // activations and filters, v_mfma_f32_32x32x16_f16, fp32 BN affine / residual / ReLU, one rounding to fp16 in the epilogue).  Fused forms
    // (fusion on): stem + max-pool in one launch, layer1.0's conv1 + downsample as one GEMM (tile 82), the global average pool in the last
    // conv3's epilogue where whole images fill its tiles -- each gives the bits of the unfused launches.  No fused stage-1 tail, no latency
    // form (lat_ok and stage1_f32 are false).  Everything the walk does differently for it hangs on `f16`.
    const bool f16 = net->math == ADAF_MATH_F16;
    const double eb = f16 ? 2.0 : 4.0;     // bytes per stored activation / filter element in the profiler's figures (the stem reads fp32 in every arithmetic)
    const char* tag = f16 ? " (fp16)" : "";
    if (f16) {
        if (!net->convs[1].w16) return adaf_fail(h, ADAF_E_STATE, "resnet50: fp16 filters missing (finalize() did not complete)");
        if (tsm_T > 0 && tsm_div <= 0) return adaf_fail(h, ADAF_E_BADARG, "resnet50: tsm_div must be positive");
        if (tsm_c1 > 0)      // the shifted operand load moves whole 16-byte chunks: 8 halfs
            for (size_t i = 1; i < net->convs.size(); ++i) {
                const ConvLayer& L = net->convs[i];
                if (L.tsm && (L.cin / tsm_div) % 8)
                    return adaf_fail(h, ADAF_E_LAYOUT, "resnet50 (fp16): temporal-shift fold = %d / %d = %d of %s must be a multiple of 8", L.cin, tsm_div,
                                     L.cin / tsm_div, L.name.c_str());
            }
    }
    auto bank = [&](const ConvLayer& L) { return f16 ? as_f32(L.w16) : L.w; };     // the filter bank a conv reads
    // layer1.0's merged conv1 + downsample filters (null: not on this plan; the fp32 bank belongs to the fp32 pipe's stage-1 launches)
    const float* const l10_w = f16 ? as_f32(net->l10_w16) : (stage1_f32 ? net->l10_w : nullptr);

    auto mark = [&](double flops, double bytes, int tile) {
        if (rec) {   // events are created up front by the caller: recording is the only work between launches
            (void)hipEventRecord((*rec)[info->size()], st);
            info->push_back({flops, bytes, tile});
        }
    };
    int li = 0;
    bool pooled = false;           // the last conv3 averaged its map itself
    auto conv = [&](const float* in, int hh, int ww, int act, const float* res, float* out, bool tsm, int* oh, int* ow) -> int {
        const ConvLayer& L = net->convs[li];
        adaf_conv_params p = layer_params(L, n, hh, ww, act);
        p.tsm_segments = tsm ? tsm_T : 0; p.tsm_div = tsm_div;
        // the split plan's stage 1 is on the fp32 pipe BY LAYER (convs 1..11: layer1.* and layer2.0.conv1, the launches the fused forms
        // cover), whether or not the fused launches are taken for this batch size / shift / fusion setting: a patch's features must not
        // depend on the batch it came in
        const bool split_here = net->math == ADAF_MATH_F32_SPLIT_BF16 && !(stage1_f32 && li >= 1 && li <= 11);
        p.tile = net->tiles[li] ? net->tiles[li] : (split_here ? 40 : 0);
        ConvArgs a;
        int rc = adaf_make_conv_args(h, &p, in, bank(L), L.scale, L.bias, res, out, &a);
        if (rc) return rc;
        a.wsp = split_here ? L.wsp : nullptr;
        if (f16) { a.in16 = a.out16 = 1; a.res16 = res != nullptr; }
        const double macs = (double)a.M * L.cout * L.k * L.k * L.cin;   // algorithmic: un-padded cin
        const double bytes = eb * ((double)n * hh * ww * L.cin + (double)a.M * L.cout * (res ? 2 : 1) + (double)L.cout * L.k * L.k * L.cin);
        mark(2.0 * macs, bytes, 0);
        const bool want_lat = lat_ok && a.M <= lat_rows && li > 0 && !net->tiles[li];
        int used = adaf_launch_conv_gemm(a, want_lat ? 95 : p.tile, h->cus, st, beside);
        if (used < 0 && want_lat) used = adaf_launch_conv_gemm(a, p.tile, h->cus, st, beside);   // the latency form declined the shape: the engine takes it
        if (used < 0) return adaf_fail(h, ADAF_E_LAUNCH, "resnet50%s: no kernel for tile id %d (conv launch %d)", tag, p.tile, li);
        if (info && !info->empty()) info->back().tile = used;
        *oh = a.OH; *ow = a.OW;
        ++li;
        return ADAF_OK;
    };

    // ---- stem: conv7x7 s2 + BN + ReLU -> maxpool 3x3 s2 into buf[1].  fp32 arithmetic in every plan; the fp16 trunk stores the POOLED map
    // with one rounding to fp16 (its unfused form keeps the conv map fp32 and rounds in the pool launch)
    const ConvLayer& L0 = net->convs[0];
    const int s1 = adaf_conv_out(P, 7, 2, 3), ph = adaf_conv_out(s1, 3, 2, 1);
    const double stem_flops = 2.0 * (double)n * s1 * s1 * 64 * 147;
    const double stem_in = 4.0 * ((double)n * P * P * 3 + 64.0 * 147), conv_map = 4.0 * (double)n * s1 * s1 * 64, pool_map = eb * (double)n * ph * ph * 64;
    const bool stem_kernel = net->tiles[0] == 0;   // (a tile override != 0 runs the stem on the generic engine instead; set_tiles refuses one for the fp16 trunk)
    // one launch (the strip or the tile kernel: the conv map never reaches HBM) or two: adaf_stem7x7_plan decides, here and for adaf_stem7x7_pool
    const int stem_form = stem_kernel ? adaf_stem7x7_plan(P, n, h->cus, fuse, net->fuse_stem_always) : ADAF_STEM_FORM_UNFUSED;
    int rc;
    bool gathered = false;
    if (src) {
        // the patches are windows of resident frames at floor(action * (H - P)) (get_patch, ACT/models/utils.py:37-51).  The strip-walking
        // stem kernel gathers them itself -- no gather launch, no patch tensor; where it does not apply (other patch sizes, small batches,
        // fusion off, a stem tile override) the gather runs into a free workspace slab first: same values either way.
        if (stem_form == ADAF_STEM_FORM_STRIP) {
            mark(stem_flops, stem_in + pool_map, 94);
            gathered = adaf_launch_stem7x7_pool_frames(src->frames, src->pixel_major, src->nframes, src->act, src->fpa, src->H, src->W, n, P,
                                                       net->stem_w, L0.scale, L0.bias, buf[1], h->cus, st, f16);
            if (!gathered && rec) info->pop_back();
        }
        if (!gathered) {
            mark(0.0, 4.0 * 2.0 * (double)n * P * P * 3, 0);
            for (int g = 0; g * src->nframes < n; ++g) {      // one gather per action set over the same frames
                const float* act = src->act + (size_t)g * (src->nframes / src->fpa) * 2;
                float* dst = buf[2] + (size_t)g * src->nframes * P * P * 4;
                if (src->pixel_major) adaf_launch_crop_nhwc4(src->frames, src->nframes, src->H, src->W, act, src->fpa, P, dst, nullptr, st);
                else if (adaf_launch_crop(src->frames, src->nframes, 3, src->H, src->W, act, src->fpa, P, dst, ADAF_LAYOUT_NHWC4, nullptr, st) != hipSuccess)
                    return adaf_fail(h, ADAF_E_LAUNCH, "resnet50: gather launch");
            }
            x4 = buf[2];
        }
    }
    if (gathered) {
    } else if (stem_form != ADAF_STEM_FORM_UNFUSED) {
        mark(stem_flops, stem_in + pool_map, 90);
        if (!adaf_launch_stem7x7_pool(x4, n, P, net->stem_w, L0.scale, L0.bias, buf[1], h->cus, st, f16, stem_form))
            return adaf_fail(h, ADAF_E_LAUNCH, "resnet50%s: no strip stem kernel at patch %d", tag, P);
    } else {
        if (stem_kernel) {   // specialised stem kernel
            mark(stem_flops, stem_in + conv_map, 40);
            adaf_launch_stem7x7(x4, n, P, net->stem_w, L0.scale, L0.bias, buf[0], h->cus, st);
        } else {
            int oh, ow;      // (= s1)
            if ((rc = conv(x4, P, P, ADAF_ACT_RELU, nullptr, buf[0], false, &oh, &ow))) return rc;
        }
        mark(0.0, conv_map + pool_map, 0);
        if (f16) adaf_launch_maxpool_f16out(buf[0], n, s1, s1, 64, buf[1], st);
        else adaf_launch_maxpool(buf[0], n, s1, s1, 64, buf[1], st);
    }
    li = 1;
    int hh = ph, ww = ph;

    float* cur = buf[1];
    float* nxt = buf[0];
    float* t1 = buf[2];            // conv1 output
    float* t2 = buf[3];            // conv2 output (or, after a fused launch, the NEXT block's conv1 output)
    float* const dsb = buf[4];     // downsample branch
    bool c1_done = false;          // the previous fused launch already produced this block's conv1 output (in t1)
    for (int s = 0; s < 4; ++s) {
        for (int b = 0; b < net->blocks[s]; ++b) {
            int h1 = hh, w1 = ww, h2, w2, h3, w3;
            if (tsm_block) {       // the block's input, shifted along its clip: conv1, downsample and identity all read this copy
                const int cin = net->convs[li].cin;
                mark(0.0, 2.0 * eb * (double)n * hh * ww * cin, 0);
                if (f16) adaf_launch_tshift_f16(cur, n, cin, hh * ww, tsm_T, tsm_div, buf[5], st);
                else adaf_launch_tshift(cur, n, cin, hh * ww, tsm_T, tsm_div, ADAF_LAYOUT_NHWC, buf[5], st);
                float* t = cur; cur = buf[5]; buf[5] = t;
            }
            const int i_c2 = li + 1, i_c3 = li + 2, i_ds = li + 3;
            const int i_next = li + 3 + (b == 0 ? 1 : 0);          // the next block's conv1 (or convs.size())
            // conv1 (1x1, optional fused temporal shift) -> conv2 (3x3, stride) -> conv3 (1x1) + identity
            bool ds_done = false;
            if (s == 0 && b == 0 && !c1_done && fuse && l10_w && tsm_c1 == 0 && !net->tiles[li] && !net->tiles[i_ds]) {
                // layer1.0: conv1 and the downsample conv in ONE launch (same input, same 1x1 geometry; N = 64 + 256): the
                // pooled map is read once instead of twice and a 0.07 ms launch disappears.  128x64 tiles: column tile 0 is conv1.
                const ConvLayer &C1 = net->convs[li], &DS = net->convs[i_ds];
                adaf_conv_params p = layer_params(C1, n, hh, ww, ADAF_ACT_RELU);
                p.cout = C1.cout + DS.cout;
                ConvArgs am;
                if ((rc = adaf_make_conv_args(h, &p, cur, l10_w, net->l10_scale, net->l10_bias, nullptr, t1, &am))) return rc;
                if (f16) am.in16 = am.out16 = 1;
                am.ldo = C1.cout;                       // conv1's output rows are 64 wide
                am.split_n = C1.cout;
                // column n of the merged GEMM is channel n - 64 of the downsample output
                am.out_b = f16 ? reinterpret_cast<float*>(reinterpret_cast<_Float16*>(dsb) - C1.cout) : dsb - C1.cout;
                am.ldo_b = DS.cout;
                am.act_b = ADAF_ACT_NONE;
                const double M = (double)am.M;
                mark(2.0 * M * (C1.cout + DS.cout) * C1.cin, eb * (M * C1.cin + M * (C1.cout + DS.cout) + (double)(C1.cout + DS.cout) * C1.cin), 93);
                if (adaf_launch_conv_gemm(am, f16 ? 82 : 32, h->cus, st) < 0) return adaf_fail(h, ADAF_E_LAUNCH, "resnet50%s: merged layer1.0 launch", tag);
                h1 = am.OH; w1 = am.OW;
                ++li;
                ds_done = true;
            } else if (!c1_done) {
                if ((rc = conv(cur, hh, ww, ADAF_ACT_RELU, nullptr, t1, tsm_c1 > 0 && net->convs[li].tsm, &h1, &w1))) return rc;
            } else ++li;
            c1_done = false;
            const float* identity = cur;
            if (b == 0) {
                if (!ds_done) {
                    li = i_ds;
                    int hd, wd;
                    if ((rc = conv(cur, hh, ww, ADAF_ACT_NONE, nullptr, dsb, false, &hd, &wd))) return rc;
                }
                identity = dsb;
            }
            li = i_c2;
            const ConvLayer& L2 = net->convs[i_c2];
            // (below ~1.5 row tiles of 128 pixels per CU the fused launch is a few dozen blocks that each run conv2, eight conv3 passes and
            //  the next conv1 one after the other -- 48-55 us at 8 patches against ~30 us for the three launches it replaces, each spread over
            //  more CUs; measured crossover between 64 and 96 patches of 96^2, tools/lat_plan_probe.py.  Bit-identical either way.)
            bool fusable = fuse && stage1_f32 && L2.cin == 64 && L2.cout == 64 && L2.stride == 1 &&
                           !net->tiles[i_c2] && !net->tiles[i_c3] && (net->fuse_stem_always || (long long)n * h1 * w1 * 2 >= 3ll * 128 * h->cus);
            const ConvLayer& L3 = net->convs[i_c3];
            ConvArgs a2;
            if (fusable) {
                const adaf_conv_params p = layer_params(L2, n, h1, w1, ADAF_ACT_RELU);
                if ((rc = adaf_make_conv_args(h, &p, t1, L2.w, L2.scale, L2.bias, nullptr, t2, &a2))) return rc;
                // (the fused launch addresses its operands with 32-bit offsets: a batch whose stage-1 map is beyond that reach -- 4 GiB, 4096
                //  patches of 128^2 -- takes the three launches below, each on the form plan_conv gives it.  Bit-identical either way.)
                fusable = adaf_fused_tail_in_reach(a2, L3.cout);
            }
            if (fusable) {
                // the next block's conv1 rides along unless it carries a temporal shift or a tile override
                // ('block' placement: the next block reads a shifted COPY of this block's output, so its conv1 cannot ride; 'blockres': it rides
                //  with the shift as a row offset inside the tile, whole clips per tile -- adaf_fused_tail_shift_ok)
                const ConvLayer* Ln = ((tsm_T == 0 || tsm_c1 > 0) && i_next < (int)net->convs.size() && !net->tiles[i_next]) ? &net->convs[i_next] : nullptr;
                if (Ln && !(Ln->k == 1 && Ln->stride == 1 && Ln->cin == L3.cout && (Ln->cout == 64 || Ln->cout == 128))) Ln = nullptr;
                const int tsm_n1 = (Ln && tsm_c1 > 0 && Ln->tsm) ? tsm_c1 : 0, fold_n1 = Ln ? Ln->cin / (tsm_div > 0 ? tsm_div : 8) : 0;
                if (tsm_n1 && !adaf_fused_tail_shift_ok(a2, L3.cout, L3.cout, tsm_n1, fold_n1)) Ln = nullptr;
                const double M = (double)a2.M;
                double macs = M * 64 * 9 * 64 + M * L3.cout * 64 + (Ln ? M * Ln->cout * L3.cout : 0.0);
                double bytes = 4.0 * (M * 64 + 2.0 * M * L3.cout + (Ln ? M * Ln->cout : 0.0) + 64.0 * 576 + 64.0 * L3.cout +
                                      (Ln ? (double)Ln->cout * L3.cout : 0.0));
                mark(2.0 * macs, bytes, Ln ? 92 : 91);
                if (adaf_launch_fused_tail(a2, L3.w, L3.scale, L3.bias, identity, L3.cout, nxt, L3.cout, Ln ? Ln->w : nullptr,
                                           Ln ? Ln->scale : nullptr, Ln ? Ln->bias : nullptr, t2, Ln ? Ln->cout : 0, st, Ln ? tsm_n1 : 0, fold_n1) < 0)
                    return adaf_fail(h, ADAF_E_LAUNCH, "resnet50: fused bottleneck tail rejected the shape");
                h3 = a2.OH; w3 = a2.OW;
                if (Ln) { float* t = t1; t1 = t2; t2 = t; c1_done = true; }
            } else {
                if ((rc = conv(t1, h1, w1, ADAF_ACT_RELU, nullptr, t2, false, &h2, &w2))) return rc;
                const bool last = s == 3 && b == net->blocks[3] - 1;
                if (last && fuse && !rec && !featmap && net->math != ADAF_MATH_F32_SPLIT_BF16 && !net->tiles[li] && !(lat_ok && n * h2 * w2 <= lat_rows)) {
                    // the trunk's last conv3: the global average pool rides in its epilogue (conv_epilogue_pool) -- no 2048-channel map,
                    // no pooling launch -- when whole images fill its row tiles (3x3 / 4x4 / 5x5 maps); bit-identical to conv + pool
                    // (fp16: the fp16-ROUNDED activated values are averaged, the bits of conv with an fp16 store + adaf_launch_avgpool_f16)
                    const ConvLayer& L3 = net->convs[li];
                    const adaf_conv_params p = layer_params(L3, n, h2, w2, ADAF_ACT_RELU);
                    ConvArgs a3;
                    if ((rc = adaf_make_conv_args(h, &p, t2, bank(L3), L3.scale, L3.bias, identity, nxt, &a3))) return rc;
                    if (f16) a3.in16 = a3.res16 = 1;
                    // (the profiled pass -- one event in front of every launch -- keeps conv + pool: its per-launch table stays comparable)
                    if (f16 ? adaf_launch_conv_pool16_rounded(a3, h2 * w2, feat, ldfeat, st) : adaf_launch_conv_pool(a3, h2 * w2, feat, ldfeat, st)) {
                        pooled = true;
                        h3 = h2; w3 = w2;
                        ++li;
                    }
                }
                if (!pooled && (rc = conv(t2, h2, w2, ADAF_ACT_RELU, identity, nxt, false, &h3, &w3))) return rc;
            }
            li = i_next;
            hh = h3; ww = w3;
            float* t = cur; cur = nxt; nxt = t;
        }
    }
    if (featmap) {      // get_featmap(pooled=False): the last block's map leaves the workspace (NHWC; fp16: its exact fp32 widening)
        if (f16) adaf_launch_cast(cur, (long long)n * hh * ww * 2048, featmap, 0, st);
        else (void)hipMemcpyAsync(featmap, cur, (size_t)n * hh * ww * 2048 * sizeof(float), hipMemcpyDeviceToDevice, st);
    }
    if (!pooled) {
        mark(0.0, eb * (double)n * hh * ww * 2048 + 4.0 * (double)n * 2048, 0);
        if (f16) adaf_launch_avgpool_f16(cur, n, hh * ww, 2048, feat, ldfeat, st);
        else adaf_launch_avgpool(cur, n, hh * ww, 2048, feat, ldfeat, st);
    }
    if (rec) (void)hipEventRecord((*rec)[info->size()], st);
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? ADAF_OK : adaf_hip_fail(h, e, f16 ? "resnet50 forward (fp16)" : "resnet50 forward");
}

}  // namespace

extern "C" {

int adaf_resnet50_create(adaf_handle* h, adaf_resnet50** out) {
    if (!h || !out) return ADAF_E_BADARG;
    adaf_resnet50* net = new adaf_resnet50();
    net->h = h;
    build_layers(net);
    *out = net;
    return ADAF_OK;
}

int adaf_resnet50_destroy(adaf_resnet50* net) {
    if (!net) return ADAF_OK;
    net->arena.release();
    delete net;
    return ADAF_OK;
}

int adaf_resnet50_set_param(adaf_resnet50* net, const char* name, const float* dev_ptr, size_t numel) {
    if (!net || !name || !dev_ptr) return ADAF_E_BADARG;
    net->params.set(name, dev_ptr, numel);
    net->finalized = false;
    return ADAF_OK;
}

// A forward: the walk, then the mark other streams' forwards look for (adaf_handle: watch_*).
static int run_trunk(adaf_resnet50* net, const float* x4, int n, int P, int tsm_T, int tsm_div, float* feat, int ldfeat,
              void* ws, size_t ws_bytes, hipStream_t st, std::vector<hipEvent_t>* rec, std::vector<Launch>* info, float* featmap = nullptr,
              const FrameSrc* src = nullptr) {
    const int rc = walk_trunk(net, x4, n, P, tsm_T, tsm_div, feat, ldfeat, ws, ws_bytes, st, rec, info, featmap, src);
    if (rc == ADAF_OK) adaf_note_forward(net->h, st);
    return rc;
}

// Three bf16 planes of every packed filter bank except the stem's (idempotent; used by the split tiles 6x).
static int split_weights(adaf_resnet50* net, void* stream) {
    adaf_handle* h = net->h;
    hipStream_t st = (hipStream_t)stream;
    for (size_t i = 1; i < net->convs.size(); ++i) {
        ConvLayer& L = net->convs[i];
        const size_t wn = L.packed_floats();
        if (!net->arena.take(&L.wsp, 3 * wn))
            return adaf_fail(h, ADAF_E_NOMEM, "resnet50: hipMalloc split weights");
        adaf_launch_split_weight(L.w, wn, L.wsp, st);
    }
    hipError_t e = hipStreamSynchronize(st);
    if (e != hipSuccess) return adaf_hip_fail(h, e, "resnet50 split weights");
    return ADAF_OK;
}

// Every packed filter bank except the stem's rounded to fp16, nearest-even (ADAF_MATH_F16; idempotent).  The packed fp32 bank is a copy of
// the parameters, so this is the rounding of the fp32 parameters themselves.
static int f16_weights(adaf_resnet50* net, void* stream) {
    adaf_handle* h = net->h;
    hipStream_t st = (hipStream_t)stream;
    for (size_t i = 1; i < net->convs.size(); ++i) {
        ConvLayer& L = net->convs[i];
        const size_t wn = L.packed_floats();
        if (!net->arena.take(&L.w16, wn))
            return adaf_fail(h, ADAF_E_NOMEM, "resnet50: hipMalloc fp16 weights");
        adaf_launch_cast(L.w, (long long)wn, L.w16, 1, st);
    }
    if (net->l10_w) {
        const ConvLayer &C1 = net->convs[1], &DS = net->convs[4];
        const size_t wn = (size_t)C1.cout * C1.cin_pad + (size_t)DS.cout * DS.cin_pad;
        if (!net->arena.take(&net->l10_w16, wn))
            return adaf_fail(h, ADAF_E_NOMEM, "resnet50: hipMalloc merged fp16 filters");
        adaf_launch_cast(net->l10_w, (long long)wn, net->l10_w16, 1, st);
    }
    hipError_t e = hipStreamSynchronize(st);
    if (e != hipSuccess) return adaf_hip_fail(h, e, "resnet50 fp16 weights");
    return ADAF_OK;
}

static int finalize_registered(adaf_resnet50* net, void* stream) {
    adaf_handle* h = net->h;
    hipStream_t st = (hipStream_t)stream;
    // the depth: the highest "layerS.B." block index registered per stage
    int found[4] = {0, 0, 0, 0};
    for (const auto& kv : net->params) {
        int s = 0, b = 0, len = 0;
        if (sscanf(kv.first.c_str(), "layer%d.%d.%n", &s, &b, &len) == 2 && len > 0 && s >= 1 && s <= 4 && b >= 0 && b + 1 > found[s - 1])
            found[s - 1] = b + 1;
    }
    // (a registration that names no Bottleneck says nothing about the depth: the plan's own, and the packer names what is missing)
    if (!(found[0] | found[1] | found[2] | found[3])) memcpy(found, net->blocks, sizeof(found));
    int depth = -1;
    for (int d = 0; d < 3; ++d)
        if (!memcmp(found, kDepths[d], sizeof(found))) depth = d;
    if (depth < 0)
        return adaf_fail(h, ADAF_E_BADARG, "resnet50: parameters name {%d, %d, %d, %d} Bottlenecks per stage; the trunk runs {3, 4, 6, 3} (ResNet-50), "
                    "{3, 4, 23, 3} (ResNet-101) or {3, 8, 36, 3} (ResNet-152)", found[0], found[1], found[2], found[3]);
    if (memcmp(found, net->blocks, sizeof(found))) {   // another depth than the plan holds: drop every packed buffer, rebuild the plan
        net->arena.release();
        net->stem_w = net->l10_w = net->l10_scale = net->l10_bias = nullptr;
        net->l10_w16 = nullptr;
        memcpy(net->blocks, found, sizeof(found));
        build_layers(net);
    }
    for (auto& L : net->convs) {
        const float* w;
        if (int rc = adaf_pack_conv_bn(h, "resnet50", net->params, net->arena, L, 1e-5f, st, &w)) return rc;
        if (&L == &net->convs[0]) {
            if (!net->arena.take(&net->stem_w, adaf_stem_weight_floats()))
                return adaf_fail(h, ADAF_E_NOMEM, "resnet50: hipMalloc stem weights");
            adaf_launch_pack_stem_weight(w, net->stem_w, st);
        }
    }
    {   // conv1 ++ downsample of layer1.0 (convs[1] and convs[4]: 1x1, stride 1, 64 input channels)
        const ConvLayer &C1 = net->convs[1], &DS = net->convs[4];
        if (C1.k == 1 && DS.k == 1 && C1.stride == 1 && DS.stride == 1 && C1.cin_pad == DS.cin_pad && C1.cout % 64 == 0) {
            const size_t n1 = (size_t)C1.cout * C1.cin_pad, n2 = (size_t)DS.cout * DS.cin_pad;
            const int cm = C1.cout + DS.cout;
            if (!net->arena.take(&net->l10_w, n1 + n2) || !net->arena.take(&net->l10_scale, (size_t)cm) || !net->arena.take(&net->l10_bias, (size_t)cm))
                return adaf_fail(h, ADAF_E_NOMEM, "resnet50: hipMalloc merged layer1.0 filters");
            (void)hipMemcpyAsync(net->l10_w, C1.w, n1 * sizeof(float), hipMemcpyDeviceToDevice, st);
            (void)hipMemcpyAsync(net->l10_w + n1, DS.w, n2 * sizeof(float), hipMemcpyDeviceToDevice, st);
            (void)hipMemcpyAsync(net->l10_scale, C1.scale, C1.cout * sizeof(float), hipMemcpyDeviceToDevice, st);
            (void)hipMemcpyAsync(net->l10_scale + C1.cout, DS.scale, DS.cout * sizeof(float), hipMemcpyDeviceToDevice, st);
            (void)hipMemcpyAsync(net->l10_bias, C1.bias, C1.cout * sizeof(float), hipMemcpyDeviceToDevice, st);
            (void)hipMemcpyAsync(net->l10_bias + C1.cout, DS.bias, DS.cout * sizeof(float), hipMemcpyDeviceToDevice, st);
        }
    }
    hipError_t e = hipStreamSynchronize(st);
    if (e != hipSuccess) return adaf_hip_fail(h, e, "resnet50 finalize");
    net->finalized = true;
    if (net->math == ADAF_MATH_F32_SPLIT_BF16) return split_weights(net, stream);
    if (net->math == ADAF_MATH_F16) return f16_weights(net, stream);
    return ADAF_OK;
}

int adaf_resnet50_finalize(adaf_resnet50* net, void* stream) {
    if (!net) return ADAF_E_BADARG;
    const int rc = finalize_registered(net, stream);
    net->params.clear();       // a registration lives until here, whatever finalize returned (include/adafocus.h)
    return rc;
}

size_t adaf_resnet50_workspace_bytes(const adaf_resnet50* net, int n, int patch) {
    float* buf[6];
    return (n <= 0 || patch <= 0) ? 0 : trunk_layout(net, n, patch, nullptr, buf);
}

int adaf_resnet50_forward(adaf_resnet50* net, const float* patches_nhwc4, int n, int patch, int tsm_segments,
                          int tsm_div, float* feat, int ldfeat, void* ws, size_t ws_bytes, void* stream) {
    if (!net) return ADAF_E_BADARG;
    return run_trunk(net, patches_nhwc4, n, patch, tsm_segments, tsm_div, feat, ldfeat, ws, ws_bytes, (hipStream_t)stream,
                     nullptr, nullptr);
}

int adaf_resnet50_forward_frames(adaf_resnet50* net, const float* frames, int frames_layout, int n_frames, int height, int width,
                                 const float* action_yx, int n_actions, int frames_per_action, int patch, int tsm_segments, int tsm_div,
                                 float* feat, int ldfeat, void* ws, size_t ws_bytes, void* stream) {
    if (!net) return ADAF_E_BADARG;
    adaf_handle* h = net->h;
    if (!frames || !action_yx || n_frames <= 0 || n_actions <= 0 || frames_per_action <= 0)
        return adaf_fail(h, ADAF_E_BADARG, "resnet50 forward_frames: null pointer or empty batch");
    if (frames_layout != ADAF_LAYOUT_NCHW && frames_layout != ADAF_LAYOUT_NHWC4)
        return adaf_fail(h, ADAF_E_LAYOUT, "resnet50 forward_frames: frames must be NCHW (3 planes) or NHWC4");
    if (n_frames % frames_per_action) return adaf_fail(h, ADAF_E_BADARG, "resnet50 forward_frames: n_frames %% frames_per_action != 0");
    const int per_set = n_frames / frames_per_action;
    if (n_actions % per_set) return adaf_fail(h, ADAF_E_BADARG, "resnet50 forward_frames: n_actions=%d is not a multiple of n_frames / frames_per_action=%d", n_actions, per_set);
    // (get_patch takes its size from the frames' HEIGHT and scales both axes by H - P, ACT/models/utils.py:40-42: frames wider than high work as in
    //  adaf_crop_gather_f32 -- x is clamped to W - P; narrower ones would read past a row)
    if (width < height) return adaf_fail(h, ADAF_E_BADARG, "resnet50 forward_frames: width %d < height %d (get_patch scales both axes by H - P)", width, height);
    if (patch > height || patch < 32) return adaf_fail(h, ADAF_E_BADARG, "resnet50 forward_frames: patch %d outside [32, %d]", patch, height);
    if (!adaf_aligned16(frames)) return adaf_fail(h, ADAF_E_LAYOUT, "resnet50 forward_frames: frames must be 16-byte aligned");
    FrameSrc src{frames, frames_layout == ADAF_LAYOUT_NHWC4, n_frames, height, width, action_yx, frames_per_action};
    const int n = (n_actions / per_set) * n_frames;        // one patch per (action set, frame)
    return run_trunk(net, frames, n, patch, tsm_segments, tsm_div, feat, ldfeat, ws, ws_bytes, (hipStream_t)stream, nullptr, nullptr, nullptr, &src);
}

int adaf_resnet50_map_size(int patch) {
    if (patch < 32) return 0;
    int s = adaf_conv_out(patch, 7, 2, 3);    // conv1 7x7 / 2 / pad 3
    s = adaf_conv_out(s, 3, 2, 1);            // max-pool 3x3 / 2 / pad 1
    for (int i = 0; i < 3; ++i) s = adaf_conv_out(s, 3, 2, 1);      // layer2-4: 3x3 / 2 / pad 1
    return s;
}

int adaf_resnet50_forward_map(adaf_resnet50* net, const float* patches_nhwc4, int n, int patch, int tsm_segments, int tsm_div,
                              float* featmap_nhwc, float* feat, int ldfeat, void* ws, size_t ws_bytes, void* stream) {
    if (!net) return ADAF_E_BADARG;
    if (!featmap_nhwc || !adaf_aligned16(featmap_nhwc)) return adaf_fail(net->h, ADAF_E_BADARG, "resnet50: forward_map needs a 16-byte aligned map buffer");
    return run_trunk(net, patches_nhwc4, n, patch, tsm_segments, tsm_div, feat, ldfeat, ws, ws_bytes, (hipStream_t)stream, nullptr, nullptr,
                     featmap_nhwc);
}

int adaf_resnet50_launch_count(const adaf_resnet50* net) { return net ? (int)net->convs.size() + 2 + (net->tsm_block ? total_blocks(net) : 0) : 0; }

int adaf_resnet50_forward_profiled(adaf_resnet50* net, const float* patches_nhwc4, int n, int patch, int tsm_segments,
                                   int tsm_div, float* feat, int ldfeat, void* ws, size_t ws_bytes, void* stream,
                                   float* launch_ms, double* launch_flops, double* launch_bytes, int* launch_tile) {
    if (!net || !launch_ms || !launch_flops || !launch_bytes || !launch_tile) return ADAF_E_BADARG;
    std::vector<hipEvent_t> ev(adaf_resnet50_launch_count(net) + 1);
    for (auto& e : ev) (void)hipEventCreate(&e);
    std::vector<Launch> info;
    int rc = run_trunk(net, patches_nhwc4, n, patch, tsm_segments, tsm_div, feat, ldfeat, ws, ws_bytes, (hipStream_t)stream,
                       &ev, &info);
    if (rc == ADAF_OK) {
        hipError_t e = hipStreamSynchronize((hipStream_t)stream);
        if (e != hipSuccess) rc = adaf_hip_fail(net->h, e, "resnet50 profiled forward");
    }
    if (rc == ADAF_OK && info.size() + 1 <= ev.size()) {
        for (size_t i = info.size(); i + 1 < ev.size(); ++i) {   // fused plans use fewer launches than the table holds
            launch_ms[i] = 0.f; launch_flops[i] = 0.0; launch_bytes[i] = 0.0; launch_tile[i] = -1;
        }
        for (size_t i = 0; i < info.size(); ++i) {
            float ms = 0.f;
            (void)hipEventElapsedTime(&ms, ev[i], ev[i + 1]);
            launch_ms[i] = ms;
            launch_flops[i] = info[i].flops;
            launch_bytes[i] = info[i].bytes;
            launch_tile[i] = info[i].tile;
        }
    }
    for (auto e : ev) (void)hipEventDestroy(e);
    return rc;
}

int adaf_resnet50_set_tiles(adaf_resnet50* net, const int* tile, int count) {
    if (!net || !tile || count != (int)net->convs.size()) return ADAF_E_BADARG;
    const bool f16 = net->math == ADAF_MATH_F16;
    for (int i = 0; i < count; ++i) {
        // fp16 trunk: the fp16-operand tiles for the convs after the stem (the stem is fp32 and has its own kernels: 0 only)
        const bool ok = f16 ? (tile[i] == 0 || (i > 0 && ((tile[i] >= 81 && tile[i] <= 84) || tile[i] == 88)))
                            : !(tile[i] < 0 || tile[i] > 80 || (tile[i] && !adaf_conv_tile_exists(tile[i])));
        if (!ok) return adaf_fail(net->h, ADAF_E_BADARG, "set_tiles: no kernel variant with id %d for conv launch %d in math mode %d", tile[i], i, net->math);
    }
    for (int i = 0; i < count; ++i) net->tiles[i] = tile[i];
    return ADAF_OK;
}

int adaf_resnet50_set_fusion(adaf_resnet50* net, int on) {
    if (!net) return ADAF_E_BADARG;
    net->fuse = on != 0;
    net->fuse_stem_always = on == 2;
    return ADAF_OK;
}

int adaf_resnet50_set_shift_place(adaf_resnet50* net, int place) {
    if (!net) return ADAF_E_BADARG;
    if (place != ADAF_SHIFT_BLOCKRES && place != ADAF_SHIFT_BLOCK) return adaf_fail(net->h, ADAF_E_BADARG, "set_shift_place: unknown placement %d", place);
    net->tsm_block = place == ADAF_SHIFT_BLOCK;
    return ADAF_OK;
}

int adaf_resnet50_set_latency_rows(adaf_resnet50* net, int rows) {
    if (!net) return ADAF_E_BADARG;
    net->lat_rows = rows;          // < 0: back to the default
    return ADAF_OK;
}

int adaf_resnet50_set_math(adaf_resnet50* net, int mode) {
    if (!net) return ADAF_E_BADARG;
    if (mode != ADAF_MATH_F32 && mode != ADAF_MATH_F32_SPLIT_BF16 && mode != ADAF_MATH_F16) return adaf_fail(net->h, ADAF_E_BADARG, "set_math: unknown mode %d", mode);
    // tile overrides name kernels of one storage type: entering or leaving the fp16 trunk clears them
    if ((mode == ADAF_MATH_F16) != (net->math == ADAF_MATH_F16)) net->tiles.assign(net->convs.size(), 0);
    net->math = mode;
    if (mode == ADAF_MATH_F32_SPLIT_BF16 && net->finalized) return split_weights(net, nullptr);
    if (mode == ADAF_MATH_F16 && net->finalized) return f16_weights(net, nullptr);
    return ADAF_OK;
}

}  // extern "C"
