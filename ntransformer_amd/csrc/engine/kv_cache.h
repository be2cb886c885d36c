// engine/kv_cache.h -- the KV cache of one engine: every sequence slot, in the format the engine was loaded with.  The only place in the engine that knows
// the format, the slots and the layer stride; the rows inside a layer buffer lie where csrc/kv_layout.h says.  Per slot and side ONE buffer of n_layers
// layer buffers (f16: [max_seq][n_kv][hd] half, transformer.cpp:340-346; q8_0: kv_q8_layer_bytes); q8_0 adds ONE one-layer F16 image per side and ENGINE.
// The memory is the caller's (Model::allocs_): this object holds addresses and frees nothing.  Accessors are inline and allocate nothing.
#pragma once
#include <cstdint>
#include <string>
#include <vector>
#include "../kv_layout.h"
#include "../../../include/ntk_engine.h"

namespace nt {
using ntk::KvGeom;
using ntk::KvRange;

class KvCache {
public:
    // `slots` zeroed caches through dev(bytes, zero) -> void*, in this order: slot 0's K and V, in q8 mode the two images, then K and V of slot 1, 2, ...
    // NTK_E_NOMEM + *err: an image or an 8-bit slot 0 is missing, or a further slot.  (A missing F16 slot 0 is the caller's to notice: k(0) is null.)
    template <class Alloc>
    int allocate(const KvGeom& g, bool q8, int slots, Alloc&& dev, std::string* err) {
        reset(); g_ = g; q8_ = q8;
        const size_t image = ntk::kv_f16_layer_elems(g.max_seq, g.per()) * sizeof(uint16_t);
        layer_bytes_ = q8 ? ntk::kv_q8_layer_bytes(g.max_seq, g.n_kv_heads, g.head_dim) : image;
        const size_t slot_bytes = (size_t)g.n_layers * layer_bytes_;
        for (int i = 0; i < slots; ++i) {
            k_.push_back((uint8_t*)dev(slot_bytes, true));
            v_.push_back((uint8_t*)dev(slot_bytes, true));
            if (i == 0 && q8) { image_k_ = (uint16_t*)dev(image, true); image_v_ = (uint16_t*)dev(image, true); }
            bytes_ += 2ull * slot_bytes + (i == 0 && q8 ? 2ull * image : 0);   // (the one image is counted once)
            if ((k_[i] && v_[i] && (!q8 || (image_k_ && image_v_))) || (i == 0 && !q8)) continue;
            *err = std::string("buffer allocation failed (") + (q8 ? "8-bit " : "") + "KV cache" + (i ? " of sequence slot " + std::to_string(i) : "") + ")";
            return NTK_E_NOMEM;
        }
        return NTK_OK;
    }
    void reset() { *this = KvCache(); }
    bool q8() const { return q8_; }
    int slots() const { return (int)k_.size(); }
    uint64_t bytes() const { return bytes_; }   // resident bytes: every slot's caches and, in q8 mode, the one F16 image
    uint64_t row_bytes() const { return q8_ ? ntk::kv_q8_row_bytes(g_.per()) : g_.per() * sizeof(uint16_t); }   // of one cache row, scales included
    // layer `layer` of slot `slot` in the engine's format (typed: the f16 engine's), and all layers of a slot (ntk_kv_shift / ntk_kv_shift_q8)
    void* k(int slot, int layer = 0) const { return k_[slot] + (size_t)layer * layer_bytes_; }
    void* v(int slot, int layer = 0) const { return v_[slot] + (size_t)layer * layer_bytes_; }
    uint16_t* k_f16(int slot, int layer) const { return static_cast<uint16_t*>(k(slot, layer)); }
    uint16_t* v_f16(int slot, int layer) const { return static_cast<uint16_t*>(v(slot, layer)); }
    // the F16 rows a prompt pass attends over: the slot's own layer, or -- q8 mode -- the image, into which the pass dequantises that layer first
    uint16_t* attend_k(int slot, int layer) const { return q8_ ? image_k_ : k_f16(slot, layer); }
    uint16_t* attend_v(int slot, int layer) const { return q8_ ? image_v_ : v_f16(slot, layer); }
    // the layer buffers of the rows of a batched step: row t lives in slot slots[t]
    void fill(ntk_kv_batch& out, const int* slots, int T, int layer) const {
        for (int t = 0; t < T; ++t) { out.k[t] = k(slots[t], layer); out.v[t] = v(slots[t], layer); }
    }
    // ... and of the segments of a packed prompt pass: segment j lives in slot slots[j] (F16 caches: the caller refuses the 8-bit format)
    void fill(ntk_kv_segments& out, const int* slots, int layer) const {
        for (int j = 0; j < out.n_seg; ++j) { out.k[j] = k(slots[j], layer); out.v[j] = v(slots[j], layer); }
    }
    // rows [pos0, pos0 + n) as byte ranges of a layer buffer; returns how many: f16 one, q8_0 two (quants, then scales)
    int row_ranges(int pos0, int n, KvRange out[2]) const {
        out[0] = q8_ ? ntk::kv_q8_quant_rows(g_.per(), pos0, n) : ntk::kv_f16_rows(g_.per(), pos0, n);
        out[1] = q8_ ? ntk::kv_q8_scale_rows(g_.max_seq, g_.per(), pos0, n) : KvRange{0, 0};
        return q8_ ? 2 : 1;
    }

private:
    KvGeom g_{};
    bool q8_ = false;
    size_t layer_bytes_ = 0;               // a slot buffer is n_layers of these
    std::vector<uint8_t*> k_, v_;          // [slots]
    uint16_t *image_k_ = nullptr, *image_v_ = nullptr;   // q8 mode: ONE layer's dequantised rows for the prompt path, shared by all layers and slots
    uint64_t bytes_ = 0;
};
}  // namespace nt
