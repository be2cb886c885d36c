// engine/model_batch.cpp -- several sequences per pass over the weights: the batched decode step, its device sampling, the packed prompt pass (see model.h)
#include "model_impl.h"

namespace nt {

// ---------------------------------------------------------------------------------------------------
// Sequence slots: one decode step of B sequences in one pass over the weights (see model.h)
// ---------------------------------------------------------------------------------------------------
int Model::batch_buffers() {
    const size_t V = (size_t)cfg_.vocab_size, N = kMaxSequences;
    if (!dev_need(batch_in_, 3 * N * 4, true) || !dev_need(batch_logprob_, N * 4, true) || !dev_need(batch_next_, N * 4, true) ||
        !dev_need(batch_attn_scratch_, N * ntk_attention_split_scratch_bytes(cfg_.n_heads, cfg_.head_dim, kMaxAttnSplits), true) ||
        !dev_need(batch_logits_, N * V * 4, true)) {
        err_ = "decode_batch: no device memory for the batch buffers (16 x vocab floats of logits)";
        return NTK_E_NOMEM;
    }
    return lm_head_workspace("decode_batch");   // (nothing to do once the workspace is large enough)
}

// slot `slot` of a batch or pass: in range, and not named before (seen: one bit per slot so far).  Null, or which of the caller's two messages applies.
static const char* slot_fault(int slot, int sequences, unsigned* seen, const char* no_such, const char* twice) {
    if (slot < 0 || slot >= sequences || slot >= Model::kMaxSequences) return no_such;
    if (*seen & (1u << slot)) return twice;
    *seen |= 1u << slot;
    return nullptr;
}

int Model::validate_batch(const int* slots, const int* tokens, const int* positions, int B, int sequences, int max_seq, int vocab, std::string* why) {
    auto fail = [&](int rc, const char* msg) { if (why) *why = msg; return rc; };
    if (!slots || !tokens || !positions) return fail(NTK_E_NULL, "decode_batch: null argument");
    if (B < 1 || B > sequences || B > kMaxSequences) return fail(NTK_E_SHAPE, "decode_batch: the batch must hold 1 .. `sequences` rows");
    unsigned seen = 0;
    for (int b = 0; b < B; ++b) {
        if (const char* m = slot_fault(slots[b], sequences, &seen, "decode_batch: no such sequence slot", "decode_batch: the same sequence slot twice in one batch"))
            return fail(NTK_E_SHAPE, m);
        if (positions[b] < 0 || positions[b] >= max_seq) return fail(NTK_E_SHAPE, "decode_batch: position outside the context");
        if (tokens[b] < 0 || tokens[b] >= vocab) return fail(NTK_E_SHAPE, "decode_batch: token id out of range");
    }
    return NTK_OK;
}

// the step up to its logits: tokens | positions up, embedding, the layer loop in batch mode, final RMSNorm, LM head into batch_logits_ (all queued, no wait)
int Model::batch_logits(const int* slots, const int* tokens, const int* positions, int B) {
    const int N = kMaxSequences;
    void* s = stream_;
    tp_call_ = 0;
    int* const host = batch_host_;   // tokens | positions | "no target": ONE copy (a member: the copy may read it until the caller's synchronisation)
    KvTarget kv{0, slots, 0};
    for (int b = 0; b < N; ++b) {
        host[b] = b < B ? tokens[b] : 0;
        host[N + b] = b < B ? positions[b] : 0;
        host[2 * N + b] = -1;
        if (b < B) kv.max_pos = std::max(kv.max_pos, positions[b]);
    }
    NT_TRY(ntk_memcpy_h2d_async(batch_in_, host, sizeof batch_host_, s));
    NT_TRY(embed_rows(hidden_, batch_in_, B));

    PassStatus ok{layers_1to1(B, 0, 0, cfg_.n_layers, kv)};
    const float* rm = final_norm(residual_, hidden_, B, ok);
    ok(lm_head(batch_logits_, residual_, B, rm));
    return ok.rc;
}

int Model::decode_batch(const int* slots, const int* tokens, const int* positions, int B, float* logits_out, int* next_out) {
    NT_TRY(validate_batch(slots, tokens, positions, B, sequences_, cfg_.max_seq_len, cfg_.vocab_size, &err_));
    if ((kv_q8_ && !batch_kv_q8_) || tp_world_ > 1) { err_ = "decode_batch: not available with kv_cache=q8_0 or tensor parallelism"; return NTK_E_SHAPE; }
    NT_TRY(batch_buffers());
    const int V = cfg_.vocab_size, N = kMaxSequences;
    void* s = stream_;
    PassStatus ok{batch_logits(slots, tokens, positions, B)};
    if (next_out) ok(ntk_logprob_rows(batch_logits_, B, V, V, batch_in_ + 2 * N, batch_logprob_, batch_next_, s));
    if (ok.rc == NTK_OK && logits_out) ok(ntk_memcpy_d2h_async(logits_out, batch_logits_, (size_t)B * V * 4, s));
    if (ok.rc == NTK_OK && next_out) ok(ntk_memcpy_d2h_async(next_out, batch_next_, (size_t)B * 4, s));
    return finish_pass("decode_batch failed: ", ok.rc);
}

// ---------------------------------------------------------------------------------------------------
// The packed prompt pass: the tokens of several sequences in one pass over the weights (see model.h)
// ---------------------------------------------------------------------------------------------------
int Model::validate_forward_batch(const int* slots, const int* lens, const int* start_pos, int n, int sequences, int max_seq, std::string* why) {
    auto fail = [&](int rc, const char* msg) { if (why) *why = msg; return rc; };
    if (!slots || !lens || !start_pos) return fail(NTK_E_NULL, "forward_batch: null argument");
    if (n < 1 || n > sequences || n > kMaxSequences) return fail(NTK_E_SHAPE, "forward_batch: the pass must hold 1 .. `sequences` segments");
    unsigned seen = 0;
    long long total = 0;
    for (int i = 0; i < n; ++i) {
        if (const char* m = slot_fault(slots[i], sequences, &seen, "forward_batch: no such sequence slot", "forward_batch: the same sequence slot twice in one pass"))
            return fail(NTK_E_SHAPE, m);
        if (lens[i] < 1) return fail(NTK_E_SHAPE, "forward_batch: an empty segment");
        if (start_pos[i] < 0 || (long long)start_pos[i] + lens[i] > max_seq) return fail(NTK_E_SHAPE, "forward_batch: a segment exceeds the context");
        total += lens[i];
    }
    if (total > max_seq) return fail(NTK_E_SHAPE, "forward_batch: more rows than the context holds (the pass runs through the context-sized activation buffers)");
    return NTK_OK;
}

int Model::forward_batch(const int* slots, const int* tokens, const int* lens, const int* start_pos, int n, float* logits_out, int* next_out) {
    NT_TRY(validate_forward_batch(slots, lens, start_pos, n, sequences_, cfg_.max_seq_len, &err_));
    if (!tokens) { err_ = "forward_batch: null argument"; return NTK_E_NULL; }
    if (kv_q8_ || tp_world_ > 1) { err_ = "forward_batch: not available with kv_cache=q8_0 or tensor parallelism"; return NTK_E_SHAPE; }
    const int H = cfg_.hidden_size, V = cfg_.vocab_size, N = kMaxSequences;
    ntk_kv_segments segs{};   // rows, lengths and first positions; layers_1to1 fills in each layer's caches
    segs.n_seg = n;
    int T = 0;
    for (int i = 0; i < n; ++i) { segs.row0[i] = T; segs.n_rows[i] = lens[i]; segs.start_pos[i] = start_pos[i]; T += lens[i]; }
    for (int t = 0; t < T; ++t)   // the embedding gather indexes the table with these on the device
        if (tokens[t] < 0 || tokens[t] >= V) { err_ = "forward_batch: token id out of range"; return NTK_E_SHAPE; }
    NT_TRY(batch_buffers());
    void* s = stream_;
    tp_call_ = 0;
    packed_tokens_.assign(tokens, tokens + T);
    int* const host = batch_host_;   // the segments' last rows | unused | "no target": ONE copy, as batch_logits()
    for (int b = 0; b < N; ++b) {
        host[b] = b < n ? segs.row0[b] + segs.n_rows[b] - 1 : 0;
        host[N + b] = 0;
        host[2 * N + b] = -1;
    }
    NT_TRY(ntk_memcpy_h2d_async(tokens_dev_, packed_tokens_.data(), (size_t)T * 4, s));
    NT_TRY(ntk_memcpy_h2d_async(batch_in_, host, sizeof batch_host_, s));
    NT_TRY(embed_rows(hidden_, tokens_dev_, T));

    KvTarget kv{0, slots, 0};
    kv.segs = &segs;
    PassStatus ok{layers_1to1(T, 0, 0, cfg_.n_layers, kv)};
    // the last row of every segment, gathered (hidden_ read as an F32 table) into n contiguous rows; the final RMSNorm and the LM head over those alone
    ok(ntk_embed_rows(residual_, hidden_, batch_in_, n, H, NTK_DT_F32, s));
    const float* rm = final_norm(hidden_, residual_, n, ok);
    ok(lm_head(batch_logits_, hidden_, n, rm));
    if (next_out) ok(ntk_logprob_rows(batch_logits_, n, V, V, batch_in_ + 2 * N, batch_logprob_, batch_next_, s));
    if (ok.rc == NTK_OK && logits_out) ok(ntk_memcpy_d2h_async(logits_out, batch_logits_, (size_t)n * V * 4, s));
    if (ok.rc == NTK_OK && next_out) ok(ntk_memcpy_d2h_async(next_out, batch_next_, (size_t)n * 4, s));
    return finish_pass("forward_batch failed: ", ok.rc);
}

int Model::batch_sample_buffers() {
    const size_t N = kMaxSequences;
    if (!dev_need(batch_recent_, N * kRecentCap * 4, false) || !dev_need(batch_sample_scratch_, ntk_sample_rows_scratch_bytes((int)N, cfg_.vocab_size), false)) {
        err_ = "decode_batch_sample: no device memory for the rows' windows and the sampler's scratch";
        return NTK_E_NOMEM;
    }
    if (!h_batch_recent_) h_batch_recent_ = (int*)nt_hip_malloc_host(N * kRecentCap * 4);
    if (!h_batch_next_) h_batch_next_ = (int*)nt_hip_malloc_host(N * 4);
    if (!h_batch_recent_ || !h_batch_next_) { err_ = "decode_batch_sample: no pinned host memory for the windows and the sampled tokens"; return NTK_E_NOMEM; }
    return NTK_OK;
}

int Model::decode_batch_sample(const int* slots, const int* tokens, const int* positions, int B, const ntk_sample_rows& rows, const int* const* recent,
                               float* logits_out, float* const* row_logits, int* next_out) {
    NT_TRY(validate_batch(slots, tokens, positions, B, sequences_, cfg_.max_seq_len, cfg_.vocab_size, &err_));
    if ((kv_q8_ && !batch_kv_q8_) || tp_world_ > 1) { err_ = "decode_batch_sample: not available with kv_cache=q8_0 or tensor parallelism"; return NTK_E_SHAPE; }
    if (!next_out) { err_ = "decode_batch_sample: null argument"; return NTK_E_NULL; }
    const int V = cfg_.vocab_size;
    int pitch = 0;   // of this step's windows: the longest one a penalty reads
    for (int b = 0; b < B; ++b) {
        if (V > 131072 || !device_sampler_supports(rows.temperature[b], rows.top_k[b], V)) {
            err_ = "decode_batch_sample: a row the device sampler does not take (temperature > 0 needs 0 < top_k <= 64, top_k < vocab <= 131072)";
            return NTK_E_SHAPE;
        }
        if (rows.n_recent[b] < 0 || rows.n_recent[b] > kMaxRecent) { err_ = "decode_batch_sample: a window of 0 .. 4096 tokens per row"; return NTK_E_SHAPE; }
        if (rows.repeat_penalty[b] > 1.0f && rows.n_recent[b] > 0) {
            if (!recent || !recent[b]) { err_ = "decode_batch_sample: null window"; return NTK_E_NULL; }
            pitch = std::max(pitch, rows.n_recent[b]);
        }
    }
    NT_TRY(batch_buffers());
    NT_TRY(batch_sample_buffers());
    void* s = stream_;
    ntk_sample_rows dev = rows;   // rows without a penalty to apply read no window
    for (int b = 0; b < B; ++b) {
        if (rows.repeat_penalty[b] > 1.0f && rows.n_recent[b] > 0) memcpy(h_batch_recent_ + (size_t)b * pitch, recent[b], (size_t)rows.n_recent[b] * 4);
        else dev.n_recent[b] = 0;
    }
    // (the previous step's copy out of the pinned staging has completed: that step synchronised)
    if (pitch > 0) NT_TRY(ntk_memcpy_h2d_async(batch_recent_, h_batch_recent_, (size_t)B * pitch * 4, s));
    PassStatus ok{batch_logits(slots, tokens, positions, B)};
    // the logits as the step computed them: queued AHEAD of the sampler, whose penalty rewrites batch_logits_ in place
    if (ok.rc == NTK_OK && logits_out) ok(ntk_memcpy_d2h_async(logits_out, batch_logits_, (size_t)B * V * 4, s));
    for (int b = 0; b < B && ok.rc == NTK_OK && row_logits; ++b)
        if (row_logits[b]) ok(ntk_memcpy_d2h_async(row_logits[b], batch_logits_ + (size_t)b * V, (size_t)V * 4, s));
    if (ok.rc == NTK_OK) ok(ntk_sample_rows_top_k(batch_logits_, B, V, V, batch_recent_, pitch, &dev, batch_next_, h_batch_next_, batch_sample_scratch_, s));
    const int rc = finish_pass("decode_batch_sample failed: ", ok.rc);
    if (rc == NTK_OK) for (int b = 0; b < B; ++b) next_out[b] = h_batch_next_[b];
    return rc;
}

}  // namespace nt
