// The weight side the three network objects share (adaf_net.h): parameter table, weight arena, conv + BN packer, ConvArgs filler.
#include <cstring>

#include "adaf_net.h"

int AdafParamTable::get(adaf_handle* h, const char* who, const std::string& key, size_t numel, const float** p) const {
    auto it = entries.find(key);
    if (it == entries.end()) return adaf_fail(h, ADAF_E_STATE, "%s: missing parameter '%s'", who, key.c_str());
    if (it->second.second != numel)
        return adaf_fail(h, ADAF_E_BADARG, "%s: '%s' has %zu elements, expected %zu", who, key.c_str(), it->second.second, numel);
    *p = it->second.first;
    return ADAF_OK;
}

void* AdafWeightArena::carve(size_t bytes) {
    bytes = (bytes + 255) & ~(size_t)255;
    if (bytes > left) {
        const size_t sz = bytes > slab_bytes ? bytes : slab_bytes;
        void* p = nullptr;
        if (hipMalloc(&p, sz) != hipSuccess) return nullptr;
        slabs.push_back(p);
        cur = static_cast<char*>(p);
        left = sz;
    }
    void* r = cur;
    cur += bytes;
    left -= bytes;
    return r;
}

void AdafWeightArena::release() {
    for (void* p : slabs) (void)hipFree(p);
    slabs.clear();
    cur = nullptr;
    left = 0;
}

int adaf_pack_conv_bn(adaf_handle* h, const char* who, const AdafParamTable& params, AdafWeightArena& arena, AdafNetConv& L, float eps,
                      hipStream_t st, const float** w_src) {
    const float *w, *g, *b, *m, *v;
    int rc;
    const size_t wn_in = L.dw ? (size_t)L.cout * L.k * L.k : (size_t)L.cout * L.cin * L.k * L.k;
    if ((rc = params.get(h, who, L.name + ".weight", wn_in, &w))) return rc;
    if ((rc = params.get(h, who, L.bn + ".weight", L.cout, &g))) return rc;
    if ((rc = params.get(h, who, L.bn + ".bias", L.cout, &b))) return rc;
    if ((rc = params.get(h, who, L.bn + ".running_mean", L.cout, &m))) return rc;
    if ((rc = params.get(h, who, L.bn + ".running_var", L.cout, &v))) return rc;
    if (!arena.take(&L.w, L.packed_floats()) || !arena.take(&L.scale, L.cout) || !arena.take(&L.bias, L.cout))
        return adaf_fail(h, ADAF_E_NOMEM, "%s: hipMalloc packed weights", who);
    if (L.dw) adaf_launch_pack_dw_kxk(w, L.cout, L.k, L.w, st);
    else adaf_launch_pack_weight(w, L.cout, L.cin, L.k, L.k, L.cin_pad, L.w, st);
    adaf_launch_fold_bn(g, b, m, v, eps, L.cout, L.scale, L.bias, st);
    if (w_src) *w_src = w;
    return ADAF_OK;
}

ConvArgs adaf_net_conv_args(const AdafNetConv& L, const void* bank, const void* in, int n, int h, int w, int oh, int ow, int pad, int act,
                            const float* res, void* out, const float* zeros) {
    ConvArgs a;
    memset(&a, 0, sizeof(a));
    a.x = static_cast<const float*>(in); a.w = static_cast<const float*>(bank);     // fp16 buffers travel as float* through ConvArgs
    a.scale = L.scale; a.bias = L.bias; a.res = res; a.out = static_cast<float*>(out);
    a.M = n * oh * ow; a.N = L.cout; a.K = L.k * L.k * L.cin_pad;
    a.cin = L.cin_pad; a.H = h; a.W = w; a.OH = oh; a.OW = ow; a.KH = a.KW = L.k; a.stride = L.stride; a.pad = pad;
    a.ldx = L.cin_pad; a.ldo = L.cout; a.ldr = L.cout; a.act = act;
    a.zeros = zeros;
    a.vec_epi = (L.cout % 4 == 0) ? 1 : 0;
    return a;
}
