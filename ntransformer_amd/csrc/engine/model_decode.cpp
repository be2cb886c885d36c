// engine/model_decode.cpp -- the fused single-token pass: launch sequence, hipGraph capture, profiler hook (see model.h)
#include "model_impl.h"

namespace nt {

// profiling hook (only inside profile_token(), never while capturing).  Fine mode: an event pair around every
// launch.  Coarse mode: ONE event where the launch class changes -- a run of same-class launches is timed as a
// whole (its kernels and the boundaries between them), so the cost of the events is paid once per run.
void Model::prof_mark(int cls, bool begin) {
    if (!prof_) return;
    void* s = stream_;
    if (prof_coarse_) {
        if (!begin) return;
        if (!prof_->empty() && prof_->back().cls == cls) { ++prof_->back().n; return; }
        void* e = ntk_event_create();
        ntk_event_record(e, s);
        const bool shared = !prof_->empty();
        if (shared) prof_->back().b = e;
        prof_->push_back({cls, e, nullptr, 1, shared});
        return;
    }
    void* e = ntk_event_create();
    ntk_event_record(e, s);
    if (begin) prof_->push_back({cls, e, nullptr, 1, false}); else prof_->back().b = e;
}

int Model::enqueue_token(bool greedy) {
    const int H = cfg_.hidden_size;
    void* s = stream_;
    tp_call_ = 0;
    prof_mark(2, true);
    const int est = ntk_embed_rows(hidden1_, token_embd_.ptr, d_token_, 1, H, token_embd_.dtype, s);
    prof_mark(2, false);
    if (est != NTK_OK && est != NTK_E_DTYPE) return est;
    NT_TRY(enqueue_layers(0, cfg_.n_layers));
    // final RMSNorm + LM head: one launch for a quantised or fused 16-bit output matrix (timed as one interval whichever form takes it), two 1:1 launches otherwise
    const DevTensor* const w = &output_;
    const bool timed = fusable(w->dtype);
    if (timed) prof_mark(0, true);
    NT_TRY(decode_project(&w, &logits_, 1, hidden1_, &output_norm_, nullptr, 16, 0, false));
    if (timed) prof_mark(0, false);
    prof_mark(2, true);
    // greedy: arg-max, token -> device word + pinned ring, position + 1 in ONE tail (ntk_argmax_advance); otherwise only the position
    if (greedy) NT_TRY(ntk_argmax_advance(logits_, cfg_.vocab_size, d_token_, h_token_, h_ring_, d_pos_, argmax_scratch_, s));
    else NT_TRY(ntk_advance_pos(d_pos_, s));
    if (tp_world_ > 1) NT_TRY(ntk_tp_advance_epoch(tp_comm_, s));
    prof_mark(2, false);
    return NTK_OK;
}

// y_k = W_k . f(x) for n <= 3 matrices sharing x.  Matrices with one fusable dtype (quantised; F16 / BF16 unless dense_fused = 0) go out as one fused launch
// (RMSNorm prologue when `norm`, residual epilogue when `resid`, n == 1; silu_pair: y_0 = SiLU(y_0) x y_1 in the epilogue, two matrices of one format); the
// other dense tensors, and a 16-bit group whose shape or alignment the fused kernel does not take (NTK_E_ALIGN / NTK_E_SHAPE), take the 1:1 launchers.
// Scratch: residual_[0,H) = dense output before the residual add, residual_[H,2H) = norm(x).  kind: the call site's rp_mask() bit.  timed: every
// launch is a profiler interval of its own (false: the caller times the whole call as one).
int Model::decode_project(const DevTensor* const* ws, float* const* ys, int n, const float* x, const DevTensor* norm, const float* resid, int kind,
                          int silu_pair, bool timed) {
    const int H = cfg_.hidden_size;
    void* s = stream_;
    auto mark = [&](bool begin) { if (timed) prof_mark(0, begin); };
    const float* nw = norm ? (const float*)norm->ptr : nullptr;
    // The two optional forms that take all n matrices in ONE launch, from the repack or from the GGUF blocks.  "Not taken" (formats / alignment / workgroup
    // split / LDS size): the next form takes over -- the per-format launches below take everything.
    auto one_launch = [&](bool rp, const float* r, int silu) {
        ntk_gemv_seg segs[3];
        if (!rp) raw_begin();
        for (int a = 0; a < n; ++a) segs[a] = {rp ? ws[a]->rp : raw_of(*ws[a]), ys[a], (int)ws[a]->out_f, ws[a]->dtype};
        mark(true);
        const int st = (rp ? ntk_gemv_rp_fused : ntk_gemv_fused)(segs, n, x, (int)ws[0]->in_f, nw, cfg_.norm_eps, r, silu, s);
        mark(false);
        return st;
    };
    bool all_rp = repack_ && (rp_mask() & kind), all_quant = true, mixed = false;
    for (int a = 0; a < n; ++a) {
        all_rp = all_rp && ws[a]->rp != nullptr && ws[a]->in_f == ws[0]->in_f;
        all_quant = all_quant && is_quant(ws[a]->dtype);
        mixed = mixed || ws[a]->dtype != ws[0]->dtype;
    }
    if (all_rp) {   // every matrix has its repacked form: the matrix-core GEMV, whatever the mix of K-quant formats; all-Q8_0: the lane-major rows
        const int st = one_launch(true, resid, silu_pair);
        if (!not_taken(st)) return st;
    }
    if (n > 1 && !resid && all_quant && mixed) {   // matrices in two K-quant formats (Q4_K_M's attn_v): still one launch when the library has the pair
        const int st = one_launch(false, nullptr, 0);
        if (!not_taken(st)) return st;
    }
    bool done[3] = {false, false, false};
    auto one_to_one = [&](int a) -> int {   // matrix a through the reference's launchers
        const DevTensor& w = *ws[a];
        const float* xin = x;
        if (nw) {
            NT_TRY(ntk_rmsnorm(residual_ + H, x, nw, 1, (int)w.in_f, cfg_.norm_eps, s));
            xin = residual_ + H;
        }
        float* y = resid ? residual_ : ys[a];
        raw_begin();
        NT_TRY(ntk_gemv(y, raw_of(w), xin, (int)w.out_f, (int)w.in_f, w.dtype, s));
        if (resid) NT_TRY(ntk_add(ys[a], resid, residual_, (int)w.out_f, s));
        done[a] = true;
        return NTK_OK;
    };
    for (int a = 0; a < n; ++a) {
        if (done[a]) continue;
        const DevTensor& w = *ws[a];
        if (!fusable(w.dtype)) { NT_TRY(one_to_one(a)); continue; }
        ntk_gemv_seg segs[3];
        int idx[3], m = 0;
        raw_begin();
        for (int b = a; b < n; ++b) {
            if (done[b] || ws[b]->dtype != w.dtype) continue;
            idx[m] = b;
            segs[m++] = {raw_of(*ws[b]), ys[b], (int)ws[b]->out_f, ws[b]->dtype};
        }
        mark(true);
        const int st = ntk_gemv_fused(segs, m, x, (int)w.in_f, nw, cfg_.norm_eps, resid, silu_pair, s);
        mark(false);
        if (is_dense16(w.dtype) && (st == NTK_E_ALIGN || st == NTK_E_SHAPE)) {   // nothing was launched: the group one by one, and the epilogue the launch would have run
            for (int k = 0; k < m; ++k) NT_TRY(one_to_one(idx[k]));
            if (silu_pair) NT_TRY(ntk_silu_mul(ys[idx[0]], ys[idx[0]], ys[idx[1]], (int)w.out_f, s));
            continue;
        }
        NT_TRY(st);
        for (int k = 0; k < m; ++k) done[idx[k]] = true;
    }
    return NTK_OK;
}

// layers [first, last) of the fused single-token path on hidden1_[H] (position in *d_pos_)
int Model::enqueue_layers(int first, int last_layer) {
    const int H = cfg_.hidden_size, I = cfg_.intermediate_size, hd = cfg_.head_dim, nh = cfg_.n_heads, nkv = cfg_.n_kv_heads;
    void* s = stream_;
    const float scale = 1.0f / sqrtf((float)hd);
    const Views act = views(1, true);
    auto project_add = [&](const DevTensor& w, const float* x, int kind) -> int {   // hidden += W . x
        const DevTensor* const wp = &w;
        float* y = tp_world_ > 1 ? tp_slot() : hidden1_;   // tensor parallelism: this rank's partial sum -> exchange slot -> hidden += sum over ranks
        NT_TRY(decode_project(&wp, &y, 1, x, nullptr, tp_world_ > 1 ? nullptr : hidden1_, kind));
        return tp_world_ > 1 ? tp_allreduce(hidden1_, H) : (int)NTK_OK;
    };

    for (int i = first; i < last_layer; ++i) {
        const LayerWeights& L = layers_[i];
        const DevTensor* const qkv[3] = {&L.wq, &L.wk, &L.wv};
        float* const qkv_out[3] = {act.q, act.k, act.v};
        NT_TRY(decode_project(qkv, qkv_out, 3, hidden1_, &L.attn_norm, nullptr, 1));
        if (L.has_qkv_bias()) {   // a Qwen2 layer: its projection biases, one launch (a node of the captured token); a layer without: nothing
            prof_mark(2, true);
            NT_TRY(ntk_qkv_bias(act.q, act.k, act.v, (const float*)L.bq.ptr, (const float*)L.bk.ptr, (const float*)L.bv.ptr, 1, nh * hd, nkv * hd, s));
            prof_mark(2, false);
        }
        if (L.has_qk_norm()) {   // a Qwen3 layer: the per-head RMSNorm of q and k, one launch (a node of the captured token); a layer without: nothing
            prof_mark(2, true);
            NT_TRY(ntk_qk_norm(act.q, act.k, (const float*)L.q_norm.ptr, (const float*)L.k_norm.ptr, 1, nh, nkv, hd, cfg_.norm_eps, s));
            prof_mark(2, false);
        }
        prof_mark(1, true);
        if (kv_q8_)
            NT_TRY(ntk_attention_decode_q8(act.attn_out, act.q, act.k, act.v, kv_.k(0, i), kv_.v(0, i), d_pos_, rope_inv_freq_, nh, nkv, hd,
                                           cfg_.max_seq_len, scale, cfg_.rope_theta, cfg_.rope_freq_scale, kv_q8_splits(attn_regime_), attn_scratch_, s));
        else if (attn_regime_ == 0)
            NT_TRY(ntk_attention_decode_fused(act.attn_out, act.q, act.k, act.v, kv_.k_f16(0, i), kv_.v_f16(0, i), d_pos_, rope_inv_freq_, nh, nkv, hd,
                                              cfg_.max_seq_len, scale, cfg_.rope_theta, cfg_.rope_freq_scale, s));
        else
            NT_TRY((attn_merge_ ? ntk_attention_decode_split_merged : ntk_attention_decode_split)(
                act.attn_out, act.q, act.k, act.v, kv_.k_f16(0, i), kv_.v_f16(0, i), d_pos_, rope_inv_freq_, nh, nkv, hd, cfg_.max_seq_len, scale,
                cfg_.rope_theta, cfg_.rope_freq_scale, attention_splits(attn_regime_, hd), attn_scratch_, s));
        prof_mark(1, false);
        NT_TRY(project_add(L.wo, act.attn_out, 2));
        if (L.is_moe()) {   // a mixture-of-experts layer: norm, route, gate | up, down as four nodes of the captured token, the experts chosen on the device
            NT_TRY(moe_ffn(L, hidden1_, 1, true));
            continue;
        }
        const DevTensor* const ffn[2] = {&L.w_gate, &L.w_up};
        float* const ffn_out[2] = {act.gate, act.up};
        // one fusable format: SiLU x up in the launch's epilogue, one profiler interval whichever form takes it; otherwise a launch of its own
        const bool pair = fusable(L.w_gate.dtype) && L.w_gate.dtype == L.w_up.dtype;
        if (pair) prof_mark(0, true);
        NT_TRY(decode_project(ffn, ffn_out, 2, hidden1_, &L.ffn_norm, nullptr, 4, pair, !pair));
        if (pair) prof_mark(0, false);
        else NT_TRY(ntk_silu_mul(act.gate, act.gate, act.up, I, s));
        NT_TRY(project_add(L.w_down, act.gate, 8));
    }
    return NTK_OK;
}

// The routed expert FFN of a mixture-of-experts layer on the T rows io [T][H], in place: RMSNorm with ffn_norm into F32 rows of the workspace, the router's
// top-K and work list, SiLU(gate) x up of every (row, expert) pair, the weighted down projections added to io.  Nothing here depends on the routing: ids,
// weights and the list stay on the device.  A pass of more rows than the workspace holds goes in pieces (a pair's bits do not depend on the piece).
int Model::moe_ffn(const LayerWeights& L, float* io, int T, bool marks) {
    if (!moe_ws_ || moe_rows_ <= 0) return NTK_E_NULL;
    const int H = cfg_.hidden_size, E = cfg_.expert_count, K = cfg_.expert_used_count, Ie = cfg_.expert_ff_length;
    void* s = stream_;
    float* const xn = reinterpret_cast<float*>(moe_ws_ + moe_off_[NTK_MOE_WS_XN]);
    float* const act = reinterpret_cast<float*>(moe_ws_ + moe_off_[NTK_MOE_WS_ACT]);
    float* const part = reinterpret_cast<float*>(moe_ws_ + moe_off_[NTK_MOE_WS_PART]);
    float* const w = reinterpret_cast<float*>(moe_ws_ + moe_off_[NTK_MOE_WS_W]);
    int* const ids = reinterpret_cast<int*>(moe_ws_ + moe_off_[NTK_MOE_WS_IDS]);
    int* const pairs = reinterpret_cast<int*>(moe_ws_ + moe_off_[NTK_MOE_WS_PAIRS]);
    int* const offsets = reinterpret_cast<int*>(moe_ws_ + moe_off_[NTK_MOE_WS_OFFSETS]);
    auto mark = [&](int cls, bool begin) { if (marks) prof_mark(cls, begin); };
    for (int t0 = 0; t0 < T; t0 += moe_rows_) {
        const int n = std::min(moe_rows_, T - t0);
        float* const x = io + (size_t)t0 * H;
        mark(2, true);
        NT_TRY(ntk_rmsnorm(xn, x, (const float*)L.ffn_norm.ptr, n, H, cfg_.norm_eps, s));
        mark(2, false);
        mark(2, true);
        NT_TRY(ntk_moe_route(xn, (const float*)L.router.ptr, n, H, E, K, ids, w, offsets, pairs, nullptr, s));
        mark(2, false);
        const bool gemm = moe_gemm_ && L.moe_gemm_ok && n >= std::max(2, moe_gemm_min_rows_);   // (one row: always the GEMV launches, the captured token's)
        mark(0, true);
        if (gemm) NT_TRY(ntk_moe_gemm_gate_up(act, xn, L.gate_exps.ptr, L.gate_exps.dtype, L.up_exps.ptr, L.up_exps.dtype, offsets, pairs, moe_gemm_scratch_,
                                              moe_gemm_scratch_bytes_, n, H, Ie, E, K, s));
        else NT_TRY(ntk_moe_gate_up(act, xn, L.gate_exps.ptr, L.gate_exps.dtype, L.up_exps.ptr, L.up_exps.dtype, offsets, pairs, n, H, Ie, E, K, s));
        mark(0, false);
        mark(0, true);
        if (gemm) NT_TRY(ntk_moe_gemm_down(x, x, act, L.down_exps.ptr, L.down_exps.dtype, ids, w, offsets, pairs, part, n, H, Ie, E, K, s));
        else NT_TRY(ntk_moe_down(x, x, act, L.down_exps.ptr, L.down_exps.dtype, ids, w, offsets, pairs, part, n, H, Ie, E, K, s));
        mark(0, false);
    }
    return NTK_OK;
}

void Model::pick_attention_regime() {
    attn_regime_ = (attn_scratch_ && (cfg_.head_dim == 64 || cfg_.head_dim == 128 || cfg_.head_dim == 256))
                       ? attention_regime(host_pos_, cfg_.head_dim) : 0;
    ++host_pos_;   // every fused token ends with ntk_advance_pos on the device; set_device_pos() re-bases both
}

int Model::decode_step_fused(bool greedy, bool use_graph) {
    pick_attention_regime();
    if (!use_graph) return enqueue_token(greedy);
    ihipGraphExec_t*& slot = graphs_[greedy ? 1 : 0][attn_regime_];
    hipStream_t st = static_cast<hipStream_t>(stream_);
    if (!slot) {   // capture once: every per-token quantity (token id, position) lives in device memory
        hipGraphExec_t ex = nullptr;
        // (relaxed under tensor parallelism: ranks sharing a process run their own runtime calls on other threads meanwhile)
        NT_TRY(capture_graph(st, tp_world_ > 1 ? hipStreamCaptureModeRelaxed : hipStreamCaptureModeThreadLocal, [&] { return enqueue_token(greedy); }, &ex));
        slot = reinterpret_cast<ihipGraphExec_t*>(ex);
    }
    return hipGraphLaunch(reinterpret_cast<hipGraphExec_t>(slot), st) == hipSuccess ? NTK_OK : NTK_E_LAUNCH;
}

int Model::profile_token(float ms[4], int calls[4], bool coarse) {
    std::vector<Timed> rec;
    rec.reserve(1024);
    prof_ = &rec;
    prof_coarse_ = coarse;
    pick_attention_regime();
    int rc = enqueue_token(true);
    if (coarse && !rec.empty()) {   // close the last run
        void* e = ntk_event_create();
        ntk_event_record(e, stream_);
        rec.back().b = e;
    }
    prof_ = nullptr;
    prof_coarse_ = false;
    if (rc == NTK_OK) rc = ntk_stream_synchronize(stream_);
    for (int c = 0; c < 4; ++c) { ms[c] = 0.0f; calls[c] = 0; }
    for (auto& t : rec) {
        float m = 0.0f;
        if (t.a && t.b && ntk_event_elapsed_ms(t.a, t.b, &m) == NTK_OK) { ms[t.cls] += m; calls[t.cls] += t.n; }
        ++calls[3];   // timed intervals
    }
    for (auto& t : rec) {   // coarse: record i's `b` is record i+1's `a` -- destroy every event once
        if (t.a && !t.shared_a) ntk_event_destroy(t.a);
        if (t.b) ntk_event_destroy(t.b);
    }
    return rc;
}

}  // namespace nt
