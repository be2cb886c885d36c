// engine/model_kv.cpp -- sequence operations on the KV caches: context shift and slot copy (see model.h)
#include "model_impl.h"

namespace nt {

int Model::validate_kv_shift(int slot, int keep, int discard, int n_past, int sequences, int max_seq, std::string* why) {
    auto refuse = [&](const char* what) { if (why) *why = std::string("kv_shift: ") + what; return NTK_E_SHAPE; };
    if (slot < 0 || slot >= sequences) return refuse("no such sequence slot");
    if (n_past < 0 || n_past > max_seq) return refuse("n_past lies outside the context");
    if (keep < 0) return refuse("keep must not be negative");
    if (discard < 1) return refuse("discard must be at least 1");
    if ((long long)keep + discard > n_past) return refuse("keep + discard exceeds n_past");
    return NTK_OK;
}

int Model::validate_kv_copy(int src_slot, int dst_slot, int pos0, int n, int sequences, int max_seq, std::string* why) {
    auto refuse = [&](const char* what) { if (why) *why = std::string("kv_copy: ") + what; return NTK_E_SHAPE; };
    if (src_slot < 0 || src_slot >= sequences || dst_slot < 0 || dst_slot >= sequences) return refuse("no such sequence slot");
    if (src_slot == dst_slot) return refuse("source and destination are the same slot");
    if (pos0 < 0 || n < 0 || pos0 > max_seq || n > max_seq - pos0) return refuse("the rows lie outside the context");
    return NTK_OK;
}

int Model::kv_shift(int slot, int keep, int discard, int n_past) {
    if (layers_.empty()) { err_ = "kv_shift: no model is loaded"; return NTK_E_NULL; }
    if (tp_world_ > 1) { err_ = "kv_shift: not supported with tensor parallelism"; return NTK_E_SHAPE; }
    NT_TRY(validate_kv_shift(slot, keep, discard, n_past, sequences_, cfg_.max_seq_len, &err_));
    const int src0 = keep + discard, n_rows = n_past - src0;
    if (n_rows > 0) {
        const int L = cfg_.n_layers, S = cfg_.max_seq_len, nkv = cfg_.n_kv_heads, hd = cfg_.head_dim;
        const int rc = kv_q8_ ? ntk_kv_shift_q8(kv_.k(slot), kv_.v(slot), L, S, nkv, hd, src0, keep, n_rows, rope_inv_freq_, cfg_.rope_theta,
                                                cfg_.rope_freq_scale, cfg_.rope_interleaved, stream_)
                            : ntk_kv_shift(static_cast<uint16_t*>(kv_.k(slot)), static_cast<uint16_t*>(kv_.v(slot)), L, S, nkv, hd, src0, keep, n_rows,
                                           rope_inv_freq_, cfg_.rope_theta, cfg_.rope_freq_scale, cfg_.rope_interleaved, stream_);
        if (rc != NTK_OK) { err_ = std::string("kv_shift: ") + ntk_status_string(rc); return rc; }
    }
    return n_past - discard;
}

int Model::kv_copy(int src_slot, int dst_slot, int pos0, int n) {
    if (layers_.empty()) { err_ = "kv_copy: no model is loaded"; return NTK_E_NULL; }
    if (tp_world_ > 1) { err_ = "kv_copy: not supported with tensor parallelism"; return NTK_E_SHAPE; }
    NT_TRY(validate_kv_copy(src_slot, dst_slot, pos0, n, sequences_, cfg_.max_seq_len, &err_));
    if (n == 0) return 0;
    hipStream_t st = static_cast<hipStream_t>(stream_);
    auto d2d = [&](void* dst, const void* src, size_t bytes) { return hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, st) == hipSuccess; };
    KvRange rows[2];   // the rows' byte ranges inside a layer buffer (f16: one; q8_0: quants, scales)
    const int n_ranges = kv_.row_ranges(pos0, n, rows);
    bool ok = true;
    for (int l = 0; l < cfg_.n_layers && ok; ++l) {
        for (int side = 0; side < 2 && ok; ++side) {
            uint8_t* const d = static_cast<uint8_t*>(side ? kv_.v(dst_slot, l) : kv_.k(dst_slot, l));
            const uint8_t* const s = static_cast<const uint8_t*>(side ? kv_.v(src_slot, l) : kv_.k(src_slot, l));
            for (int r = 0; r < n_ranges && ok; ++r) ok = d2d(d + rows[r].off, s + rows[r].off, rows[r].bytes);
        }
    }
    if (!ok) { err_ = "kv_copy: a device-to-device copy failed"; return NTK_E_LAUNCH; }
    return n;
}

}  // namespace nt
