// Where a network's weights live (adaf_resnet50, adaf_mobilenetv2, adaf_effnet; net_store.hip): the table of registered parameters, the
// arena every packed copy is taken from, the conv + BN packer and the ConvArgs of a packed conv.  Host code only.
#pragma once
#include <map>
#include <string>
#include <vector>

#include "adaf_internal.h"

// The parameters set_param() registered: name -> (device pointer, elements).  A registration lives until the next finalize() of its
// network returns -- finalize() reads the pointers, makes packed copies and clears the table on every exit path -- so the caller may
// free the tensors then, and a finalize() without a complete fresh registration fails with ADAF_E_STATE, naming the missing one, instead of reading them.
struct AdafParamTable {
    std::map<std::string, std::pair<const float*, size_t>> entries;
    void set(const char* name, const float* p, size_t numel) { entries[name] = std::make_pair(p, numel); }
    // ADAF_E_STATE when `key` is not registered, ADAF_E_BADARG when it has another size than `numel`; who = "resnet50" | "mobilenetv2" | "effnet"
    int get(adaf_handle* h, const char* who, const std::string& key, size_t numel, const float** p) const;
    auto begin() const { return entries.begin(); }      // (name, ...) pairs in name order: the trunk infers its depth from the names
    auto end() const { return entries.end(); }
    void clear() { entries.clear(); }
};

// Every derived weight buffer of a network (packed filters, folded BN, SE matrices, B fragments) is carved out of a few large slabs: a
// launch of a whole-block kernel reads ~14 of them, and as separate small device allocations each sat in pages of its own.  Requests are
// rounded to 256 bytes; one larger than a slab gets a slab of its own (slab_bytes = 0: every request does).  Nothing is returned
// before release(): a network takes each buffer on first use and reuses it on every later finalize().
struct AdafWeightArena {
    size_t slab_bytes;
    std::vector<void*> slabs;
    char* cur = nullptr;
    size_t left = 0;
    explicit AdafWeightArena(size_t slab = (size_t)32 << 20) : slab_bytes(slab) {}
    void* carve(size_t bytes);      // nullptr = out of memory
    // a buffer of `count` elements on first use (finalize and set_math may run again over the same plan); false = out of memory
    template <typename T> bool take(T** p, size_t count) { return *p || (*p = static_cast<T*>(carve(count * sizeof(T)))); }
    void release();                 // frees every slab: all buffers taken from the arena are gone
};

// One conv + BN of a network and its packed copies.
struct AdafNetConv {
    std::string name;      // "layer1.0.conv1" | "stem", "b3.expand", "b3.dw", "b3.project", "head"
    std::string bn;        // prefix of its BN parameters: "layer1.0.bn1" | name + ".bn"
    int cin, cout, k, stride;
    bool dw;               // depthwise (cin == cout channels, one k x k filter each)
    int cin_pad;
    float* w = nullptr;              // dense: [cout][k][k][cin_pad] fp32; depthwise: [k*k][c]
    unsigned short* w16 = nullptr;   // the dense filters in fp16 where the network's arithmetic wants them (its finalize fills it)
    float* scale = nullptr;          // folded BN
    float* bias = nullptr;
    size_t packed_floats() const { return dw ? (size_t)k * k * cout : (size_t)cout * k * k * cin_pad; }
};
inline AdafNetConv adaf_net_conv(const std::string& name, int cin, int cout, int k, int stride, bool dw, int cin_pad) {
    return {name, name + ".bn", cin, cout, k, stride, dw, cin_pad};
}

// Reads L's filter and four BN parameters from the table, takes L.w / L.scale / L.bias from the arena, packs the filter (dense OHWI
// with the channel axis padded, or depthwise [k*k][c]) and folds the BN with `eps`.  *w_src (optional) gets the registered filter.
int adaf_pack_conv_bn(adaf_handle* h, const char* who, const AdafParamTable& params, AdafWeightArena& arena, AdafNetConv& L, float eps,
                      hipStream_t st, const float** w_src = nullptr);

// The ConvArgs of packed conv L reading filter bank `bank` (L.w or L.w16) over n maps of h x w -> oh x ow.  Every other field is zero:
// no shift, fp32 storage, position-major tiles off -- the shift fields and the dtype flags are the caller's to set.
ConvArgs adaf_net_conv_args(const AdafNetConv& L, const void* bank, const void* in, int n, int h, int w, int oh, int ow, int pad, int act,
                            const float* res, void* out, const float* zeros);
