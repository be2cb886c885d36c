// engine/model_debug.cpp -- parity instrumentation (see model.h)
#include "model_impl.h"

namespace nt {

// ---- parity instrumentation (tests; reached through nt_engine_debug_*, never from the generate loop) --------------------------
// Layers [first, first + count) on caller-supplied hidden states: hidden_in [T][H] (host) -> hidden_out [T][H] (host), tokens at
// positions start_pos...  mode 0: the 1:1 launcher sequence (prompt projections batched or per token as set_batched_prefill says);
// mode 1: the fused single-token launches (T == 1); mode 2: the same replayed from a freshly captured hipGraph.  The KV cache
// rows of the T positions are written by the layers as in a normal forward; rows of earlier positions are whatever the cache
// holds (debug_kv_write puts a checker's rows there: layer-wise teacher forcing).
int Model::debug_run_layers(const float* hidden_in, int T, int start_pos, int first, int count, int mode, float* hidden_out) {
    if (!hidden_in || !hidden_out) return NTK_E_NULL;
    if (T <= 0 || start_pos < 0 || start_pos + T > cfg_.max_seq_len || first < 0 || count < 0 || first + count > cfg_.n_layers) return NTK_E_SHAPE;
    if (mode != 0 && T != 1) return NTK_E_SHAPE;
    if (tp_world_ > 1) return NTK_E_SHAPE;
    const size_t bytes = (size_t)T * cfg_.hidden_size * 4;
    void* s = stream_;
    float* const hid = mode == 0 ? hidden_ : hidden1_;   // (the fused path's hidden state may live in the static slot)
    NT_TRY(ntk_memcpy_h2d_async(hid, hidden_in, bytes, s));
    int rc;
    if (mode == 0) {
        NT_TRY(upload_positions(T, start_pos));
        NT_TRY(ntk_stream_synchronize(s));
        rc = layers_1to1(T, start_pos, first, first + count);
    } else {
        NT_TRY(set_device_pos(start_pos));
        pick_attention_regime();
        if (mode == 1) {
            rc = enqueue_layers(first, first + count);
        } else {
            hipStream_t st = static_cast<hipStream_t>(s);
            hipGraphExec_t ex = nullptr;
            rc = capture_graph(st, hipStreamCaptureModeThreadLocal, [&] { return enqueue_layers(first, first + count); }, &ex);
            if (rc == NTK_OK && hipGraphLaunch(ex, st) != hipSuccess) rc = NTK_E_LAUNCH;
            if (rc == NTK_OK) rc = ntk_stream_synchronize(s);
            if (ex) (void)hipGraphExecDestroy(ex);
        }
    }
    if (rc != NTK_OK) return rc;
    NT_TRY(ntk_memcpy_d2h_async(hidden_out, hid, bytes, s));
    return ntk_stream_synchronize(s);
}

// cache rows [pos0, pos0 + n) of one layer, [n][n_kv_heads * head_dim] halves each (reference layout, transformer.cpp:340-346)
int Model::debug_kv(int layer, int pos0, int n, uint16_t* k, uint16_t* v, bool write, int slot) {
    if (!k || !v) return NTK_E_NULL;
    if (kv_q8_) { err_ = "debug_kv: the KV cache is q8_0 (use the _q8 form)"; return NTK_E_DTYPE; }
    if (layer < 0 || layer >= cfg_.n_layers || pos0 < 0 || n < 0 || pos0 + n > cfg_.max_seq_len || slot < 0 || slot >= kv_.slots()) return NTK_E_SHAPE;
    KvRange r[2];
    kv_.row_ranges(pos0, n, r);   // (f16: one range)
    uint8_t* const kd = static_cast<uint8_t*>(kv_.k(slot, layer)) + r[0].off;
    uint8_t* const vd = static_cast<uint8_t*>(kv_.v(slot, layer)) + r[0].off;
    void* s = stream_;
    NT_TRY(write ? ntk_memcpy_h2d_async(kd, k, r[0].bytes, s) : ntk_memcpy_d2h_async(k, kd, r[0].bytes, s));
    NT_TRY(write ? ntk_memcpy_h2d_async(vd, v, r[0].bytes, s) : ntk_memcpy_d2h_async(v, vd, r[0].bytes, s));
    return ntk_stream_synchronize(s);
}

// ... of the 8-bit cache, as canonical 34-byte GGUF block_q8_0 {half d; int8 q[32]}: [n][n_kv_heads * head_dim / 32] blocks per side.  The device
// keeps quants and scales in two planes (csrc/attention_q8.hip): the rows' slices of both are contiguous, the blocks are (de)interleaved here.
int Model::debug_kv_q8(int layer, int pos0, int n, uint8_t* k_blocks, uint8_t* v_blocks, bool write, int slot) {
    if (!k_blocks || !v_blocks) return NTK_E_NULL;
    if (!kv_q8_) { err_ = "debug_kv_q8: the KV cache is f16"; return NTK_E_DTYPE; }
    if (layer < 0 || layer >= cfg_.n_layers || pos0 < 0 || n < 0 || pos0 + n > cfg_.max_seq_len || slot < 0 || slot >= kv_.slots()) return NTK_E_SHAPE;
    if (n == 0) return NTK_OK;
    const size_t nb = (size_t)cfg_.n_kv_heads * cfg_.head_dim / 32;   // blocks of a row
    KvRange r[2];   // quants, scales
    kv_.row_ranges(pos0, n, r);
    const size_t qbytes = r[0].bytes, sbytes = r[1].bytes;
    void* s = stream_;
    std::vector<uint8_t> qh(qbytes), sh(sbytes);
    for (int side = 0; side < 2; ++side) {
        uint8_t* base = static_cast<uint8_t*>(side ? kv_.v(slot, layer) : kv_.k(slot, layer));
        uint8_t *qd = base + r[0].off, *sd = base + r[1].off;
        uint8_t* blocks = side ? v_blocks : k_blocks;
        if (write) {
            for (size_t b = 0; b < (size_t)n * nb; ++b) {
                memcpy(&sh[2 * b], blocks + 34 * b, 2);
                memcpy(&qh[32 * b], blocks + 34 * b + 2, 32);
            }
            NT_TRY(ntk_memcpy_h2d_async(qd, qh.data(), qbytes, s));
            NT_TRY(ntk_memcpy_h2d_async(sd, sh.data(), sbytes, s));
            NT_TRY(ntk_stream_synchronize(s));
        } else {
            NT_TRY(ntk_memcpy_d2h_async(qh.data(), qd, qbytes, s));
            NT_TRY(ntk_memcpy_d2h_async(sh.data(), sd, sbytes, s));
            NT_TRY(ntk_stream_synchronize(s));
            for (size_t b = 0; b < (size_t)n * nb; ++b) {
                memcpy(blocks + 34 * b, &sh[2 * b], 2);
                memcpy(blocks + 34 * b + 2, &qh[32 * b], 32);
            }
        }
    }
    return NTK_OK;
}

// Parity instrumentation: from now on every 1:1 pass (forward / debug_run_layers mode 0) leaves the F32 k (BEFORE the rotation) and v projections of
// `layer` in a capture buffer; debug_kv_inputs_read returns those of the last pass ([n][n_kv_heads * head_dim] floats each).  layer < 0: off.
int Model::debug_kv_inputs_capture(int layer) {
    if (layers_.empty()) return NTK_E_NULL;
    if (layer >= cfg_.n_layers) return NTK_E_SHAPE;
    kv_capture_layer_ = layer < 0 ? -1 : layer;
    kv_capture_T_ = 0;
    if (layer >= 0 && !kv_capture_) {
        const size_t bytes = 2 * (size_t)cfg_.max_seq_len * cfg_.n_kv_heads * cfg_.head_dim * 4;
        kv_capture_ = (float*)dev_alloc(bytes, false);
        if (!kv_capture_) { err_ = "debug_kv_inputs_capture: out of device memory"; return NTK_E_NOMEM; }
    }
    return NTK_OK;
}
int Model::debug_kv_inputs_read(int n, float* k, float* v) {
    if (!k || !v) return NTK_E_NULL;
    if (!kv_capture_ || kv_capture_layer_ < 0 || n < 0 || n > kv_capture_T_) return NTK_E_SHAPE;
    const size_t kvd = (size_t)cfg_.n_kv_heads * cfg_.head_dim;
    NT_TRY(ntk_memcpy_d2h_async(k, kv_capture_, (size_t)n * kvd * 4, stream_));
    NT_TRY(ntk_memcpy_d2h_async(v, kv_capture_ + (size_t)cfg_.max_seq_len * kvd, (size_t)n * kvd * 4, stream_));
    return ntk_stream_synchronize(stream_);
}

}  // namespace nt
