// kv_layout.h -- where the rows of one layer's K (or V) cache lie, in both cache formats: the ONE statement of it.  Plain C++17
// without an include: host code, the .hip launchers and the kernels take their numbers from here.  `per` = n_kv_heads * head_dim, a row's elements.
//   F16:   half [max_seq][per]
//   Q8_0:  int8 quants [max_seq][per] at byte 0, half scales [max_seq][per / 32] at byte max_seq * per, the total rounded up to 256 bytes
#pragma once
namespace ntk {
using kv_size = decltype(sizeof 0);   // size_t
struct KvGeom {
    int n_layers, max_seq, n_kv_heads, head_dim;
    constexpr kv_size per() const { return (kv_size)n_kv_heads * (kv_size)head_dim; }
};
struct KvRange { kv_size off, bytes; };   // a byte range inside one layer buffer

constexpr kv_size kv_f16_layer_elems(int max_seq, kv_size per) { return (kv_size)max_seq * per; }
constexpr kv_size kv_f16_row(kv_size per, int pos) { return (kv_size)pos * per; }   // element offset of row `pos`
constexpr KvRange kv_f16_rows(kv_size per, int pos0, int n) { return {kv_f16_row(per, pos0) * 2, (kv_size)n * per * 2}; }   // rows [pos0, pos0 + n)

constexpr kv_size kv_q8_scale_offset(int max_seq, kv_size per) { return (kv_size)max_seq * per; }   // byte offset of the scale plane
constexpr kv_size kv_q8_row_bytes(kv_size per) { return per + per / 16; }                            // an int8 per element + a half per 32
constexpr kv_size kv_q8_layer_bytes(int max_seq, int n_kv_heads, int head_dim) {   // = ntk_kv_q8_cache_bytes; 0: not a geometry the format has
    if (max_seq <= 0 || n_kv_heads <= 0 || head_dim <= 0 || head_dim % 32 != 0) return 0;
    return ((kv_size)max_seq * kv_q8_row_bytes((kv_size)n_kv_heads * (kv_size)head_dim) + 255) / 256 * 256;
}
constexpr KvRange kv_q8_quant_rows(kv_size per, int pos0, int n) { return {(kv_size)pos0 * per, (kv_size)n * per}; }   // rows [pos0, pos0 + n), quant plane
constexpr KvRange kv_q8_scale_rows(int max_seq, kv_size per, int pos0, int n) {                                        // ... and scale plane
    return {kv_q8_scale_offset(max_seq, per) + (kv_size)pos0 * (per / 32) * 2, (kv_size)n * (per / 32) * 2};
}
}  // namespace ntk
