// engine/model.cpp -- lifetime and options (see model.h)
#include "model_impl.h"
#include <thread>

namespace nt {

Model::~Model() { free_all(); }

void Model::drop_graphs() {
    for (auto& row : graphs_)
        for (auto& g : row) {
            if (g) (void)hipGraphExecDestroy(reinterpret_cast<hipGraphExec_t>(g));
            g = nullptr;
        }
}

void* Model::dev_alloc(size_t bytes, bool zero) {
    void* p = nt_hip_malloc(bytes + 256);
    if (!p) return nullptr;
    allocs_.push_back(p);
    if (zero) nt_hip_memset(p, 0, bytes);
    return p;
}

void Model::dev_free(void* p) {
    if (!p) return;
    allocs_.erase(std::remove(allocs_.begin(), allocs_.end(), p), allocs_.end());
    nt_hip_free(p);
}

void Model::free_all() {
    drop_graphs();
    for (int r = 0; r < 8; ++r) {   // peers' communication buffers mapped through hipIpc
        if (tp_peer_opened_[r] && tp_peers_[r]) (void)ntk_ipc_close(tp_peers_[r]);
        tp_peers_[r] = nullptr;
        tp_peer_opened_[r] = false;
    }
    tp_connected_ = false;
    tp_comm_ = nullptr;
    tp_call_ = 0;
    if (own_stream_ && stream_) (void)hipStreamDestroy(static_cast<hipStream_t>(stream_));
    own_stream_ = false;
    stream_ = nullptr;
    for (void* p : allocs_) nt_hip_free(p);
    allocs_.clear();
    if (arena_owner_) ntk_decode_arena_release(arena_device_);
    arena_owner_ = false;
    arena_device_ = -1;
    hidden1_ = arena_attn_ = arena_gate_ = nullptr;
    auto free_host = [](auto*& p) { if (p) nt_hip_free_host(p); p = nullptr; };
    free_host(h_token_); free_host(h_ring_); free_host(h_recent_); free_host(h_batch_recent_); free_host(h_batch_next_);
    sample_scratch_ = gemm_ws_ = gemm_ws2_ = nullptr;
    d_recent_ = nullptr;
    shares_weights_ = false;   // (allocs_ held only this object's own buffers: the tensors belong to the model they were shared from)
    layers_.clear();
    // a second load() on the same object starts from a clean slate
    token_embd_ = output_norm_ = output_ = DevTensor();
    weight_bytes_ = repack_bytes_ = raw_freed_bytes_ = 0;
    raw_scratch_ = nullptr; raw_scratch_bytes_ = raw_cursor_ = 0; raw_err_ = 0;
    repack_done_ = output_tied_ = false;
    host_pos_ = attn_regime_ = 0;
    kv_.reset();
    rope_factors_.clear();
    batch_logits_ = batch_logprob_ = batch_attn_scratch_ = nullptr; batch_in_ = batch_next_ = batch_recent_ = nullptr; batch_sample_scratch_ = nullptr;
    kv_capture_ = nullptr; kv_capture_layer_ = -1; kv_capture_T_ = 0;
    moe_ws_ = nullptr; moe_rows_ = 0; moe_gemm_scratch_ = nullptr; moe_gemm_scratch_bytes_ = 0;
    hidden_ = residual_ = workspace_ = logits_ = argmax_scratch_ = rope_inv_freq_ = attn_scratch_ = row_max_ = nullptr;
    positions_ = tokens_dev_ = d_pos_ = d_token_ = nullptr;
    score_logits_ = score_logprob_ = nullptr; score_targets_ = score_top1_ = nullptr; score_cap_ = 0;   // (they were in allocs_)
    score_ws_ = nullptr; score_ws_bytes_ = 0;
}

int Model::share_weights(const Model& src, int max_context) {
    if (&src == this) { err_ = "share_weights: a model cannot share its own weights"; return NTK_E_NULL; }
    free_all();
    if (src.layers_.empty()) { err_ = "share_weights: the source model is not loaded"; return NTK_E_NULL; }
    if (src.tp_world_ != 1 || src.shares_weights_) {
        err_ = "share_weights: the source must hold whole tensors of its own (no tensor parallelism, not itself a sharing sequence)";
        return NTK_E_SHAPE;
    }
    cfg_ = src.cfg_;                     // (theta, the linear scale and ...
    rope_factors_ = src.rope_factors_;   // ... the frequency divisors: this sequence rotates as its source does, whatever its own rope options say)
    cfg_full_ = src.cfg_;
    if (max_context > 0) cfg_.max_seq_len = max_context;
    vocab_ = src.vocab_;
    layers_ = src.layers_;               // the same device pointers (raw GGUF bytes and the decode repack): read-only for every launch
    token_embd_ = src.token_embd_; output_norm_ = src.output_norm_; output_ = src.output_;
    output_tied_ = src.output_tied_;
    weight_bytes_ = src.weight_bytes_;   // (bytes_per_token: the bytes a token of THIS sequence streams)
    repack_ = src.repack_; repack_wanted_ = src.repack_; repack_done_ = true;
    repack_bytes_ = 0;                   // none of it is this object's
    shares_weights_ = true;
    if (src.raw_freed_bytes_ > 0 && src.raw_scratch_bytes_ > 0) {   // one resident copy: what still reads raw blocks (the 1:1 sequence, the prompt's LM head) unpacks
        void* d = dev_alloc(src.raw_scratch_bytes_, false);      // into a scratch of THIS sequence (stream ordered on this sequence's stream)
        if (!d) { err_ = "share_weights: no device memory for the unpack scratch"; free_all(); return NTK_E_NOMEM; }
        raw_scratch_ = d; raw_scratch_bytes_ = src.raw_scratch_bytes_;
        raw_freed_bytes_ = src.raw_freed_bytes_;
    }
    int rc = own_stream();
    if (rc == NTK_OK) rc = alloc_buffers();
    if (rc != NTK_OK) free_all();
    return rc;
}

int Model::set_attention_merge(bool on) {
    if (on == attn_merge_) return NTK_OK;
    if (!layers_.empty()) {
        NT_TRY(sync());
        drop_graphs();
    }
    attn_merge_ = on;
    return NTK_OK;
}

int Model::set_dense_fused(bool on) {
    if (on == dense_fused_) return NTK_OK;
    if (!layers_.empty()) {
        NT_TRY(sync());
        drop_graphs();
    }
    dense_fused_ = on;
    return NTK_OK;
}

bool Model::fusable(int dt) const { return is_quant(dt) || (dense_fused_ && is_dense16(dt)); }

int Model::set_repack(int level) {
    level = level < 0 ? 0 : level > 3 ? 3 : level;
    if (shares_weights_) { err_ = "set_repack: this sequence shares another model's tensors"; return NTK_E_SHAPE; }
    repack_wanted_ = level;
    if (layers_.empty()) { repack_ = level; return NTK_OK; }   // before the load: finish_load() decides
    if (level == 3) level = 2;   // (round 6: one resident copy; what is gone stays gone)
    if (level == repack_) return NTK_OK;
    NT_TRY(sync());
    drop_graphs();
    int rc = NTK_OK;
    if (level < 2 && raw_freed_bytes_ > 0) rc = restore_raw_all();           // the GGUF bytes come back first (levels 0 and 1 read them)
    if (rc == NTK_OK && level > 0 && !repack_done_) {
        rc = repack_all();
        if (rc == NTK_E_NOMEM) { fprintf(stderr, "warning: decode repack incomplete (device memory): the rest stays on the raw path\n"); rc = NTK_OK; err_.clear(); }
    }
    if (rc != NTK_OK) { err_ = std::string("set_repack: ") + ntk_status_string(rc); return rc; }
    repack_ = level;
    if (level == 2) rc = drop_raw_all();
    return rc;
}

uint64_t Model::bytes_per_token(int pos) const {
    uint64_t b = 0;
    for (const auto& L : layers_)
        for (auto m : kLayerMatrices) b += (L.*m).nbytes;
    for (const auto& L : layers_)   // a mixture-of-experts layer: the router and the K experts a token is routed to, of E
        if (L.is_moe() && cfg_.expert_count > 0)
            b += L.router.nbytes + (uint64_t)(L.gate_exps.nbytes + L.up_exps.nbytes + L.down_exps.nbytes) / (uint64_t)cfg_.expert_count * (uint64_t)cfg_.expert_used_count;
    b += output_.nbytes;
    b += (uint64_t)(2 * cfg_.n_layers + 1) * cfg_.hidden_size * 4;
    const uint64_t kv_row = kv_.row_bytes();
    b += 2ull * cfg_.n_layers * kv_row * (uint64_t)(pos + 1) + 2ull * cfg_.n_layers * kv_row;
    b += ntk_row_bytes(token_embd_.dtype, cfg_.hidden_size);
    return b;
}

int Model::set_device_token(int token) {
    if (token < 0 || token >= cfg_.vocab_size) { err_ = "token id out of range"; return NTK_E_SHAPE; }
    *h_token_ = token;
    return ntk_memcpy_h2d_async(d_token_, h_token_, 4, stream_);
}
int Model::set_device_pos(int pos) {
    host_pos_ = pos;
    // small copy, once per generation -- on the model's own stream: a blocking copy on the legacy stream would collide with a
    // hipGraph capture in progress on another thread's stream (tensor-parallel ranks sharing a process)
    NT_TRY(ntk_memcpy_h2d_async(d_pos_, &pos, 4, stream_));
    NT_TRY(ntk_stream_synchronize(stream_));
    // nothing is in flight: forget the tokens of earlier positions (a re-based position could otherwise match a stale {token, position} tag)
    if (h_ring_) memset(h_ring_, 0, 64);
    return NTK_OK;
}
int Model::sync() { return ntk_stream_synchronize(stream_); }
int Model::host_token() const { return *h_token_; }
int Model::copy_logits(float* host) {
    NT_TRY(ntk_memcpy_d2h_async(host, logits_, (size_t)cfg_.vocab_size * 4, stream_));
    return ntk_stream_synchronize(stream_);
}

int Model::sample_on_device(const int* recent, int n_recent, float repeat_penalty, float temperature, int top_k, float top_p, float r) {
    if (!sample_scratch_ || !d_recent_ || !h_recent_) return NTK_E_NOMEM;
    if (n_recent > kRecentCap) { recent += n_recent - kRecentCap; n_recent = kRecentCap; }
    void* s = stream_;
    if (repeat_penalty > 1.0f && n_recent > 0) {
        // the previous token's copy of the window has completed (the host synchronised to read that token)
        memcpy(h_recent_, recent, (size_t)n_recent * 4);
        NT_TRY(ntk_memcpy_h2d_async(d_recent_, h_recent_, (size_t)n_recent * 4, s));
    } else {
        n_recent = 0;
    }
    if (temperature <= 0.0f) {   // greedy with a repeat penalty: Sampler::sample returns argmax of the penalised logits
        NT_TRY(ntk_repeat_penalty(logits_, cfg_.vocab_size, d_recent_, n_recent, repeat_penalty, s));
        return ntk_argmax(logits_, cfg_.vocab_size, d_token_, h_token_, argmax_scratch_, s);
    }
    return ntk_sample_top_k(logits_, cfg_.vocab_size, d_recent_, n_recent, repeat_penalty, temperature, top_k, top_p, r, d_token_,
                            h_token_, sample_scratch_, s);
}

// The token decoded at position `pos` by a greedy fused step, without synchronising the stream: the final launch of the step stores
// {token, pos + 1} into slot (pos & 3) of the pinned ring; the host polls that word.  Meanwhile the NEXT step may already be queued (its
// token lands in another slot), so the GPU never waits for the host between tokens (Engine::run / decode_greedy_steps keep one step
// ahead).  A poll that sees nothing for 2 s falls back to a stream synchronisation and reports what that returns.
int Model::wait_token(int pos, int* token) {
    volatile unsigned long long* slot = h_ring_ + (pos & 3);
    const unsigned want = (unsigned)(pos + 1);
    for (unsigned spins = 0;; ++spins) {
        const unsigned long long v = *slot;
        if ((unsigned)(v >> 32) == want) { *token = (int)(unsigned)v; return NTK_OK; }
#if defined(__x86_64__) || defined(__i386__)
        __builtin_ia32_pause();
#else
        std::this_thread::yield();
#endif
        if ((spins & 0xFFFFu) == 0xFFFFu) {
            const auto now = std::chrono::steady_clock::now();
            if (spins == 0xFFFFu) wait_t0_ = now;
            else if (std::chrono::duration<double>(now - wait_t0_).count() > 2.0) break;
        }
    }
    static bool warned = false;
    if (!warned) { warned = true; fprintf(stderr, "warning: the pinned token ring was not seen updating for 2 s (host memory not coherent with a running kernel?); falling back to a stream synchronisation per token\n"); }
    NT_TRY(ntk_stream_synchronize(stream_));
    const unsigned long long v = *slot;
    if ((unsigned)(v >> 32) != want) { err_ = "decode step finished without publishing its token"; return NTK_E_LAUNCH; }
    *token = (int)(unsigned)v;
    return NTK_OK;
}

int Model::set_sequences(int n) {
    if (n < 1 || n > kMaxSequences) { err_ = "sequences must lie in 1 .. " + std::to_string(kMaxSequences); return NTK_E_SHAPE; }
    sequences_ = n;
    return NTK_OK;
}

int Model::set_batch_kv_q8(bool on) {
    if (!layers_.empty()) { err_ = "batch_kv_q8 must be set before the model is loaded"; return NTK_E_SHAPE; }
    batch_kv_q8_ = on;
    return NTK_OK;
}

int Model::set_static_activations(bool on) {
    if (!layers_.empty()) { err_ = "static_activations must be set before the model is loaded"; return NTK_E_SHAPE; }
    static_act_ = on;
    return NTK_OK;
}

int Model::set_kv_cache(const std::string& kind) {
    if (kind != "f16" && kind != "q8_0") { err_ = "kv_cache: unknown format '" + kind + "' (f16 or q8_0)"; return NTK_E_DTYPE; }
    if (!layers_.empty()) { err_ = "kv_cache must be set before the model is loaded"; return NTK_E_SHAPE; }
    const bool q8 = kind == "q8_0";
    kv_q8_ = q8;
    return NTK_OK;
}

int Model::set_rope_scaling(const std::string& text) {
    if (!layers_.empty()) { err_ = "rope_scaling must be set before the model is loaded"; return NTK_E_SHAPE; }
    RopeScalingOption o;
    if (!parse_rope_scaling(text, &o, &err_)) return NTK_E_SHAPE;
    rope_opt_ = o;
    return NTK_OK;
}

int Model::set_rope_freq_base(const std::string& text) {
    if (!layers_.empty()) { err_ = "rope_freq_base must be set before the model is loaded"; return NTK_E_SHAPE; }
    if (!parse_positive_float(text, &rope_base_opt_)) { err_ = "rope_freq_base must be a number > 0"; return NTK_E_SHAPE; }
    return NTK_OK;
}

int Model::set_rope_freq_scale(const std::string& text) {
    if (!layers_.empty()) { err_ = "rope_freq_scale must be set before the model is loaded"; return NTK_E_SHAPE; }
    if (!parse_positive_float(text, &rope_scale_opt_)) { err_ = "rope_freq_scale must be a number > 0"; return NTK_E_SHAPE; }
    return NTK_OK;
}

// The rotation of the model being loaded: cfg_ holds the file's (or the synthetic spec's) theta, linear scale and scaling type; f (null: synthetic) may
// carry the divisors.  Refusals name the tensor.
int Model::resolve_rope(const GgufFile* f) {
    rope_factors_.clear();
    const int half = cfg_.head_dim / 2;
    if (rope_base_opt_ > 0.0f) cfg_.rope_theta = rope_base_opt_;
    // the file's divisors: kept under "file" and under "linear:<f>" (which overrides the linear scale alone, as llama.cpp's --rope-scaling linear
    // does); "none" ignores them and "llama3:..." replaces them
    const bool file_factors = rope_opt_.mode == RopeScalingOption::FILE || rope_opt_.mode == RopeScalingOption::LINEAR;
    const GgufTensor* t = f && file_factors ? f->find("rope_freqs.weight") : nullptr;
    if (t) {
        if (t->dtype != NTK_DT_F32 || !t->known_type) { err_ = "rope_freqs.weight must be F32"; return NTK_E_DTYPE; }
        if (t->numel() != half) {
            err_ = "rope_freqs.weight holds " + std::to_string(t->numel()) + " factors, head_dim / 2 = " + std::to_string(half) + " are needed";
            return NTK_E_SHAPE;
        }
        rope_factors_.resize((size_t)half);
        memcpy(rope_factors_.data(), f->data(*t), (size_t)half * 4);
        for (int i = 0; i < half; ++i)
            if (!std::isfinite(rope_factors_[i]) || !(rope_factors_[i] > 0.0f)) {
                err_ = "rope_freqs.weight: factor " + std::to_string(i) + " is not a finite number > 0";
                rope_factors_.clear();
                return NTK_E_SHAPE;
            }
    }
    switch (rope_opt_.mode) {
        case RopeScalingOption::FILE:   // (cfg_.rope_freq_scale: the file's linear scale, 1 otherwise)
            if (cfg_.rope_scaling_type != "none" && cfg_.rope_scaling_type != "linear")
                fprintf(stderr, "note: RoPE scaling type '%s' is not applied: the model runs with unscaled positions\n", cfg_.rope_scaling_type.c_str());
            break;
        case RopeScalingOption::NONE:
            cfg_.rope_freq_scale = 1.0f; cfg_.rope_scaling_type = "none"; cfg_.rope_orig_ctx = 0;
            break;
        case RopeScalingOption::LINEAR:
            cfg_.rope_freq_scale = 1.0f / rope_opt_.factor; cfg_.rope_scaling_type = "linear"; cfg_.rope_orig_ctx = 0;
            break;
        case RopeScalingOption::LLAMA3: {
            rope_factors_.resize((size_t)half);
            const int st = rope_llama3_factors(cfg_.head_dim, cfg_.rope_theta, rope_opt_.factor, rope_opt_.low, rope_opt_.high, rope_opt_.orig_ctx, rope_factors_.data());
            if (st != NTK_OK) { rope_factors_.clear(); err_ = "rope_scaling: llama3 factors cannot be computed for this model"; return st; }
            cfg_.rope_freq_scale = 1.0f; cfg_.rope_scaling_type = "llama3"; cfg_.rope_orig_ctx = rope_opt_.orig_ctx;
            break;
        }
    }
    // (the decode attention's generic form -- any other head size -- derives the frequency from theta and takes no table: ntk_attention_decode_fused)
    if (!rope_factors_.empty() && cfg_.head_dim != 64 && cfg_.head_dim != 128 && cfg_.head_dim != 256) {
        rope_factors_.clear();
        err_ = "RoPE frequency factors (rope_freqs.weight / rope_scaling=llama3) need head_dim 64, 128 or 256 (this model: " + std::to_string(cfg_.head_dim) + ")";
        return NTK_E_SHAPE;
    }
    if (rope_scale_opt_ > 0.0f) cfg_.rope_freq_scale = rope_scale_opt_;
    cfg_.rope_factors = (int)rope_factors_.size();
    return NTK_OK;
}

// what decode_step_fused() emits
const char* Model::decode_path() const {
    return arena_owner_ ? "fused (5 launches/layer; static activations)" : "fused (5 launches/layer)";
}

Model::Views Model::views(int T, bool fused) const {
    const size_t qd = (size_t)T * cfg_.n_heads * cfg_.head_dim, kvd = (size_t)T * cfg_.n_kv_heads * cfg_.head_dim;
    float* const q = workspace_;
    Views v{q, q + qd, q + qd + kvd, q + qd + 2 * kvd, workspace_, workspace_ + (size_t)T * cfg_.intermediate_size};
    if (fused && T == 1 && arena_owner_) { v.attn_out = arena_attn_; v.gate = arena_gate_; }
    return v;
}

int Model::init_device() {
    const char* e = getenv("NTK_DEVICE");
    const int st = ntk_device_init(e ? atoi(e) : 0);
    if (st != NTK_OK) err_ = "no usable GPU (HIP device init failed)";
    return st;
}

int Model::own_stream() {
    hipStream_t own = nullptr;
    if (hipStreamCreateWithFlags(&own, hipStreamNonBlocking) != hipSuccess) { err_ = "stream creation failed"; return NTK_E_LAUNCH; }
    stream_ = own;
    own_stream_ = true;
    return NTK_OK;
}

}  // namespace nt
