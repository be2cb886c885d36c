// engine/model_prompt.cpp -- the prompt pass (see model.h)
#include "model_impl.h"
#include <type_traits>

namespace nt {

// ---------------------------------------------------------------------------------------------------
// 1:1 path: the reference's own launcher sequence (transformer.cpp:604-669, attention.cpp:120-211,
// ffn.cpp:85-134), through the same C ABI an external caller would use
// ---------------------------------------------------------------------------------------------------
float* Model::forward(const int* tokens, int T, int start_pos, int slot) {
    if (T <= 0 || start_pos < 0 || start_pos + T > cfg_.max_seq_len) { err_ = "forward: sequence exceeds context"; return nullptr; }
    if (slot < 0 || slot >= sequences_) { err_ = "forward: no such sequence slot"; return nullptr; }
    for (int i = 0; i < T; ++i)   // the embedding gather indexes the table with these on the device
        if (tokens[i] < 0 || tokens[i] >= cfg_.vocab_size) { err_ = "forward: token id out of range"; return nullptr; }
    const int H = cfg_.hidden_size;
    void* s = stream_;
    tp_call_ = 0;
    // embedding rows are dequantised on the device (the reference does it on the host and uploads, :419-599)
    if (ntk_memcpy_h2d_async(tokens_dev_, tokens, (size_t)T * 4, s) != NTK_OK) return nullptr;
    const int est = ntk_embed_rows(hidden_, token_embd_.ptr, tokens_dev_, T, H, token_embd_.dtype, s);
    if (est == NTK_E_DTYPE) fprintf(stderr, "Error: Unsupported embedding dtype: %s\n", dtype_name(token_embd_.dtype));
    else if (est != NTK_OK) return nullptr;
    std::vector<int> pos(T);
    for (int i = 0; i < T; ++i) pos[i] = start_pos + i;
    if (ntk_memcpy_h2d_async(positions_, pos.data(), (size_t)T * 4, s) != NTK_OK) return nullptr;
    if (ntk_stream_synchronize(s) != NTK_OK) return nullptr;   // `pos` / `tokens` are host temporaries

    const KvTarget kv{slot, nullptr, 0};
    int rc = layers_1to1(T, start_pos, 0, cfg_.n_layers, kv);
    auto ok = [&](int st) { if (st != NTK_OK && rc == NTK_OK) rc = st; };
    float* last = hidden_ + (size_t)(T - 1) * H;
    ok(ntk_rmsnorm(last, last, (const float*)output_norm_.ptr, 1, H, cfg_.norm_eps, s));   // in place, :658-659
    {
        raw_begin();
        const int st = ntk_gemv(logits_, raw_of(output_), last, (int)output_.out_f, (int)output_.in_f, output_.dtype, s);
        if (st == NTK_E_DTYPE) fprintf(stderr, "Unsupported dtype for GEMV: %s\n", dtype_name(output_.dtype));   // gemm.cu:801-803
        else ok(st);
    }
    if (tp_world_ > 1) ok(ntk_tp_advance_epoch(tp_comm_, s));
    ok(ntk_stream_synchronize(s));
    if (raw_err_ != NTK_OK) { rc = raw_err_; raw_err_ = NTK_OK; }
    if (rc == NTK_OK) rc = check_tp();
    if (rc != NTK_OK) { if (err_.empty() || rc != NTK_E_LAUNCH) err_ = std::string("forward failed: ") + ntk_status_string(rc); return nullptr; }
    return logits_;
}

// The prompt pass's operand planes: the FP16 GEMM reads X split into FP16 planes, written into a workspace by its own pre-pass or by the launch that
// produced X (ntk_*_prepare_x: the projection then needs no pre-pass launch at all).  Two workspaces are used alternately.  The invariant: a producer
// never writes planes into the workspace whose partial sums it is reading -- a projection's deferred K splits lie in the workspace of its own planes, so
// the producer that consumes them takes other().
struct OperandPlanes {
    void* ws[2];
    int cur = 0;
    const float* of = nullptr;   // the X whose planes lie in ws[cur] (Q, K, V and gate, up share one X)
    void* current() const { return ws[cur]; }
    bool hold(const float* X) const { return X == of; }
    void* other() { cur ^= 1; of = nullptr; return ws[cur]; }                // a producer is about to write planes: the workspace the last projection did NOT use
    void written(const float* X, bool split) { of = split ? X : nullptr; }   // X has new contents: planes are stale unless its producer just split it
    void in_current(const float* X) { of = X; }                              // a projection's pre-pass (or such a producer) has left X's planes in ws[cur]
};

// the formats and shapes ntk_gemm_quant_f16 takes
static bool f16_ok(const DevTensor& w) {
    const bool kq = w.dtype == NTK_DT_Q4_0 || w.dtype == NTK_DT_Q4_K || w.dtype == NTK_DT_Q5_K || w.dtype == NTK_DT_Q6_K;
    return (w.dtype == NTK_DT_Q8_0 || kq) && w.in_f % (kq ? 256 : 128) == 0 && w.out_f % 16 == 0 && (w.ptr || w.rp);
}
// a K-quant matrix whose GGUF bytes were freed after the load-time repack (one resident copy): the FP16 GEMM reads it FROM THE REPACK
// (ntk_gemm_desc.weights_repacked: identical bits) -- no unpack in front of the prompt launches
static bool rp_only(const DevTensor& w) {
    return !w.ptr && w.rp && (w.dtype == NTK_DT_Q4_K || w.dtype == NTK_DT_Q5_K || w.dtype == NTK_DT_Q6_K) && w.out_f % 16 == 0;
}

// layers [first, last) of the 1:1 path on hidden_[T][H] at positions start_pos.. (positions_ already on the device)
int Model::layers_1to1(int T, int start_pos, int first, int last_layer, const KvTarget& kv) {
    const int H = cfg_.hidden_size, I = cfg_.intermediate_size, hd = cfg_.head_dim, nh = cfg_.n_heads, nkv = cfg_.n_kv_heads;
    const int qd = nh * hd, kvd = nkv * hd;
    void* s = stream_;
    const float scale = 1.0f / sqrtf((float)hd);
    const Views act = views(T);
    int rc = NTK_OK;
    auto ok = [&](int st) { if (st != NTK_OK && rc == NTK_OK) rc = st; };
    // (wp: the tensor's raw GGUF blocks -- resident, or unpacked from the repack by raw_of() once per projection, not per token)
    auto gemv = [&](float* y, const DevTensor& w, const void* wp, const float* x) {
        const int st = ntk_gemv(y, wp, x, (int)w.out_f, (int)w.in_f, w.dtype, s);
        if (st == NTK_E_DTYPE) fprintf(stderr, "Unsupported dtype for GEMV: %s\n", dtype_name(w.dtype));   // gemm.cu:801-803
        else ok(st);
    };
    // Y[t] = W . X[t] for the T tokens: one pass over W per 16 tokens on the matrix cores, or the reference's loop
    const bool batched = batched_prefill_ && T > 1;
    // the FP16 GEMM takes every prompt of 2 tokens or more (its weight-streaming form up to 32); it also reads a matrix that exists only as its decode
    // repack, where the F32-MFMA form (ntk_gemm_quant) would need the GGUF bytes unpacked first
    const bool bf16_now = bf16_prefill_ && gemm_ws_ && T > 1;
    OperandPlanes planes{{gemm_ws_, gemm_ws2_}};
    // RMSNorm / SiLU x up in front of an FP16-GEMM projection also leave the tokens' largest |x|: the GEMM's operand pre-pass then needs no pass of its
    // own over X for the token scales (row_max_: [2][max_seq]; the second array is zeroed by the layer's first RMSNorm launch for the SiLU launch's
    // atomic maxima)
    const bool with_max = batched && bf16_now && row_max_ != nullptr && prefill_row_max_;
    float* rm_a = with_max ? row_max_ : nullptr;
    float* rm_b = with_max ? row_max_ + cfg_.max_seq_len : nullptr;
    // The form the producer of X takes when X (`width` columns) feeds matrix next_w: it splits X into next_w's planes itself, leaves the tokens' maxima, or
    // neither.  The split: up to 64 tokens (a producer that owns a whole token per workgroup writes its planes in 16-byte pieces a kilobyte apart:
    // faster than the GEMM's own pre-pass at 16 - 64 tokens, slower at 1024), and not under tensor parallelism, where a rank's SiLU launch keeps its maxima
    // in the array that only ntk_rmsnorm_rowmax zeroes.
    enum class XForm { plain, row_max, split };
    auto x_form = [&](int width, const DevTensor& next_w) {
        if (with_max && prefill_fused_split_ && gemm_ws2_ != nullptr && T <= 64 && tp_world_ == 1 && f16_ok(next_w) && (int)next_w.in_f == width) return XForm::split;
        return with_max ? XForm::row_max : XForm::plain;
    };
    // The FP16 GEMM behind its descriptor (ntk_engine.h): 1..3 matrices of one format sharing X, ONE launch.  `raw`: the matrices' GGUF bytes where the
    // caller has them already; without it a group whose every matrix is rp_only is read from the repack, any other group through raw_of() (one raw_begin()
    // per group: its tensors lie side by side in the unpack scratch).  X's planes are reused when they lie in the current workspace, and lie there after
    // the launch.  rm: the tokens' largest |X| where X's producer left them.
    auto gemm_group = [&](float* const* Ys, const DevTensor* const* Ws, int n, const float* X, const float* resid, const float* rm, ntk_gemm_partials* pt,
                          const void* const* raw) {
        bool repacked = raw == nullptr;
        for (int k = 0; k < n; ++k) repacked = repacked && rp_only(*Ws[k]);
        if (!repacked && !raw) raw_begin();
        ntk_gemv_seg segs[3];
        for (int k = 0; k < n; ++k) segs[k] = {repacked ? Ws[k]->rp : raw ? raw[k] : raw_of(*Ws[k]), Ys[k], (int)Ws[k]->out_f, Ws[k]->dtype};
        ntk_gemm_desc d{};
        d.segs = segs; d.nseg = n; d.X = X; d.n_tokens = T; d.in_features = (int)Ws[0]->in_f; d.resid = resid;
        d.workspace = planes.current(); d.workspace_bytes = gemm_ws_bytes_; d.reuse_x = planes.hold(X) ? 1 : 0; d.row_max = rm; d.partials = pt;
        d.weights_repacked = repacked ? 1 : 0;
        const int st = ntk_gemm_quant_f16(&d, s);
        if (st == NTK_OK) planes.in_current(X);
        return st;
    };
    // One quantised matrix on the FP16 matrix cores (up to 1024 tokens per pass): straight from the repack where it exists only there; otherwise, or when that form
    // is not taken, from its GGUF bytes -- *wp, obtained here for the caller's F32-MFMA / per-token fallbacks too (without the FP16 option: NTK_E_DTYPE, no launch).
    auto gemm_f16 = [&](float* Y, const DevTensor& w, const float* X, const float* resid, const float* rm, ntk_gemm_partials* pt, const void** wp) {
        const DevTensor* const one = &w;
        if (bf16_now && rp_only(w)) {
            const int st = gemm_group(&Y, &one, 1, X, resid, rm, pt, nullptr);
            if (!not_taken(st)) return st;
        }
        raw_begin();
        *wp = raw_of(w);
        return bf16_now ? gemm_group(&Y, &one, 1, X, resid, rm, pt, wp) : (int)NTK_E_DTYPE;
    };
    auto project = [&](float* Y, const DevTensor& w, const float* X, size_t ystride, size_t xstride, const float* rm) {
        const bool dense = ystride == (size_t)w.out_f && xstride == (size_t)w.in_f;
        const void* wp = nullptr;
        if (batched && is_quant(w.dtype) && dense) {
            int st = gemm_f16(Y, w, X, nullptr, rm, nullptr, &wp);
            if (not_taken(st)) st = ntk_gemm_quant(Y, wp, X, T, (int)w.out_f, (int)w.in_f, w.dtype, nullptr, s);
            if (st != NTK_E_ALIGN && st != NTK_E_SHAPE) { ok(st); return; }   // those two: shapes only the per-token loop takes
        } else { raw_begin(); wp = raw_of(w); }
        for (int t = 0; t < T; ++t) gemv(Y + (size_t)t * ystride, w, wp, X + (size_t)t * xstride);
    };
    // matrices that share X (Q | K | V, gate | up): those of one format go out as ONE launch of the FP16 GEMM, the rest one by one
    auto project_many = [&](float* const* Ys, const DevTensor* const* Ws, int n, const float* X, const float* rm) {
        bool done[3] = {false, false, false};
        for (int a = 0; a < n && batched && bf16_now; ++a) {
            if (done[a]) continue;
            float* ys[3];
            const DevTensor* ws[3];
            int idx[3], m = 0;
            for (int b = a; b < n; ++b)
                if (!done[b] && Ws[b]->dtype == Ws[a]->dtype && Ws[b]->in_f == Ws[a]->in_f) { ys[m] = Ys[b]; ws[m] = Ws[b]; idx[m++] = b; }
            if (m < 2) continue;
            const int st = gemm_group(ys, ws, m, X, nullptr, rm, nullptr, nullptr);
            if (st == NTK_OK) for (int k = 0; k < m; ++k) done[idx[k]] = true;
            else if (!not_taken(st)) { ok(st); return; }
        }
        for (int a = 0; a < n; ++a)
            if (!done[a]) project(Ys[a], *Ws[a], X, (size_t)Ws[a]->out_f, (size_t)Ws[a]->in_f, rm);
    };
    // X as it lies (the attention output) in front of matrix w: row maximum + split in one launch of its own
    auto prepare_x = [&](const float* X, const DevTensor& w) {
        if (x_form((int)w.in_f, w) != XForm::split || planes.hold(X)) return;
        planes.written(X, ntk_gemm_prepare_x(X, T, (int)w.in_f, planes.other(), s) == NTK_OK);
    };
    // hidden += W . X (attention.cpp:207 + transformer.cpp:645, ffn.cpp:130 + transformer.cpp:652): the batched
    // projection adds the residual in its epilogue, the reference sequence goes through residual_ and launch_add_inplace
    auto project_add = [&](const DevTensor& w, const float* X, size_t xstride, const float* rm) {
        if (tp_world_ > 1) {   // this rank's columns give a PARTIAL sum: into the exchange slot, then hidden += sum over ranks
            project(tp_slot(), w, X, H, xstride, rm);
            ok(tp_allreduce(hidden_, T * H));
            return;
        }
        const bool dense = batched && (size_t)w.out_f == (size_t)H && xstride == (size_t)w.in_f;
        if (dense && bf16_now) prepare_x(X, w);
        if (dense && is_quant(w.dtype)) {
            const void* wp = nullptr;
            int st = gemm_f16(hidden_, w, X, hidden_, rm, nullptr, &wp);
            if (not_taken(st)) st = ntk_gemm_quant(hidden_, wp, X, T, (int)w.out_f, (int)w.in_f, w.dtype, hidden_, s);
            if (st != NTK_E_ALIGN && st != NTK_E_SHAPE) { ok(st); return; }
        }
        project(residual_, w, X, H, xstride, rm);
        ok(ntk_add_inplace(hidden_, residual_, T * H, s));
    };
    // residual_ = RMSNorm(hidden_) in the form its consumer next_w asks for
    auto norm = [&](const DevTensor& nw, bool zero_b, const DevTensor& next_w) {
        const XForm f = x_form(H, next_w);
        if (f == XForm::split) ok(ntk_rmsnorm_prepare_x(residual_, hidden_, (const float*)nw.ptr, T, H, cfg_.norm_eps, planes.other(), s));
        else if (f == XForm::row_max) ok(ntk_rmsnorm_rowmax(residual_, hidden_, (const float*)nw.ptr, T, H, cfg_.norm_eps, rm_a, zero_b ? rm_b : nullptr, s));
        else ok(ntk_rmsnorm(residual_, hidden_, (const float*)nw.ptr, T, H, cfg_.norm_eps, s));
        planes.written(residual_, f == XForm::split);
    };
    // hidden += W . X followed by the NEXT RMSNorm (nw; into residual_) as one consumer launch of the projection's K splits (ntk_gemm_quant_f16 with
    // `partials` + ntk_reduce_rmsnorm_*); false = not this shape / format: the caller runs project_add + norm
    auto project_add_norm = [&](const DevTensor& w, const float* X, const float* rm, const DevTensor& nw, bool zero_b, const DevTensor& next_w) -> bool {
        if (!with_max || tp_world_ > 1 || !is_quant(w.dtype) || (size_t)w.out_f != (size_t)H) return false;
        ntk_gemm_partials pt;
        prepare_x(X, w);
        // (a launch that does not split K adds the residual in its own epilogue, in place, as project_add does: nothing is deferred then)
        const void* wp = nullptr;
        int st = gemm_f16(hidden_, w, X, hidden_, rm, &pt, &wp);
        if (not_taken(st)) return false;
        const bool split = st == NTK_OK && x_form(H, next_w) == XForm::split;   // (the partial sums lie in the current workspace: the planes go to the other one)
        if (split) st = ntk_reduce_rmsnorm_prepare_x(hidden_, &pt, (const float*)nw.ptr, cfg_.norm_eps, residual_, planes.other(), s);
        else if (st == NTK_OK) st = ntk_reduce_rmsnorm_rowmax(hidden_, &pt, (const float*)nw.ptr, cfg_.norm_eps, residual_, rm_a, zero_b ? rm_b : nullptr, s);
        planes.written(residual_, split);
        ok(st);
        return true;
    };
    // gate | up and SiLU x up (per token in the reference, ffn.cpp:127: the same elementwise op) with the gate | up launch's K splits summed by the SiLU
    // launch itself (ntk_gemm_quant_f16 with `partials` + ntk_reduce_silu_mul_*); false = not this shape / format: the caller takes the separate launches
    auto gate_up_silu = [&](const LayerWeights& L) -> bool {
        if (!with_max || !rm_b || tp_world_ > 1 || L.w_gate.dtype != L.w_up.dtype || !is_quant(L.w_gate.dtype) || L.w_gate.in_f != L.w_up.in_f ||
            (size_t)L.w_gate.out_f != (size_t)I || (size_t)L.w_up.out_f != (size_t)I || I % 4 != 0) return false;
        float* const ys[2] = {act.gate, act.up};
        const DevTensor* const ws[2] = {&L.w_gate, &L.w_up};
        ntk_gemm_partials pt;
        int st = gemm_group(ys, ws, 2, residual_, nullptr, rm_a, &pt, nullptr);
        if (not_taken(st)) return false;
        const bool split = st == NTK_OK && x_form(I, L.w_down) == XForm::split;
        if (split) st = ntk_reduce_silu_mul_prepare_x(act.gate, &pt, planes.other(), s);
        else if (st == NTK_OK) st = ntk_reduce_silu_mul_rowmax(act.gate, &pt, rm_b, s);
        planes.written(act.gate, split);
        ok(st);
        return true;
    };
    // gate = SiLU(gate) x up in the form the down projection asks for
    auto silu_mul = [&](const DevTensor& next_w) {
        const XForm f = x_form(I, next_w);
        int st = NTK_E_SHAPE;
        if (f == XForm::split) st = ntk_silu_mul_prepare_x(act.gate, act.gate, act.up, T, I, planes.other(), s);
        else if (f == XForm::row_max && rm_b) st = ntk_silu_mul_rowmax(act.gate, act.gate, act.up, T, I, rm_b, s);
        planes.written(act.gate, f == XForm::split && st == NTK_OK);
        if (st == NTK_E_SHAPE || st == NTK_E_ALIGN) { st = ntk_silu_mul(act.gate, act.gate, act.up, T * I, s); rm_b = nullptr; }   // (then for the rest of the pass)
        ok(st);
    };
    bool normed_ahead = false;   // residual_ (with its maxima or planes) already holds this layer's normalised input, written with the previous layer's down projection
    for (int i = first; i < last_layer; ++i) {
        const LayerWeights& L = layers_[i];
        uint16_t* const kc = kv_.attend_k(kv.slot, i);   // (q8_0: the one-layer F16 image, rebuilt below)
        uint16_t* const vc = kv_.attend_v(kv.slot, i);
        if (!normed_ahead) norm(L.attn_norm, true, L.wq);
        normed_ahead = false;
        float* const qkv_out[3] = {act.q, act.k, act.v};
        const DevTensor* const qkv[3] = {&L.wq, &L.wk, &L.wv};
        project_many(qkv_out, qkv, 3, residual_, rm_a);
        if (i == kv_capture_layer_ && kv_capture_) {   // parity instrumentation: the F32 projections the store launches are about to read
            ok(ntk_copy(kv_capture_, act.k, T * kvd, s));
            ok(ntk_copy(kv_capture_ + (size_t)cfg_.max_seq_len * kvd, act.v, T * kvd, s));
            kv_capture_T_ = T;
        }
        // (every rotation below takes rope_tab(): the frequency table when the model carries frequency divisors, NULL -- the in-kernel frequency -- otherwise)
        if (kv.segs) {   // a packed prompt pass: every segment rotated, stored and attended on its own slot's cache from its own start position, one launch each
            ntk_kv_segments segs = *kv.segs;
            kv_.fill(segs, kv.slots, i);
            ok(ntk_rope_kv_store_segments_tab(act.q, act.k, act.v, &segs, nh, nkv, hd, cfg_.rope_theta, cfg_.rope_freq_scale, cfg_.rope_interleaved,
                                              cfg_.max_seq_len, rope_tab(), s));
            ok(ntk_attention_prefill_segments(act.attn_out, act.q, &segs, nh, nkv, hd, cfg_.max_seq_len, scale, s));
        } else if (kv.slots && kv_q8_) {   // ... over the 8-bit caches ("batch_kv_q8"): the single-row decode launch's splits for the batch's largest position
            ntk_kv_batch caches{};
            kv_.fill(caches, kv.slots, T, i);
            ok(ntk_attention_decode_q8_batch(act.attn_out, act.q, act.k, act.v, &caches, batch_in_ + kMaxSequences, T, rope_inv_freq_, nh, nkv, hd, cfg_.max_seq_len,
                                             scale, cfg_.rope_theta, cfg_.rope_freq_scale, kv_q8_splits(attention_regime(kv.max_pos, hd)), batch_attn_scratch_, s));
        } else if (kv.slots) {   // a batch of sequences: rope / store / attention of every row on its own cache at its own position, one launch
            ntk_kv_batch caches{};
            kv_.fill(caches, kv.slots, T, i);
            const bool splits_ok = batch_attn_scratch_ && (hd == 64 || hd == 128 || hd == 256);   // (pick_attention_regime's rule)
            const int regime = splits_ok ? attention_regime(kv.max_pos, hd) : 0;
            ok(ntk_attention_decode_batch(act.attn_out, act.q, act.k, act.v, &caches, batch_in_ + kMaxSequences, T, rope_inv_freq_, nh, nkv, hd, cfg_.max_seq_len, scale,
                                          cfg_.rope_theta, cfg_.rope_freq_scale, regime == 0 ? 1 : attention_splits(regime, hd), batch_attn_scratch_, s));
        } else if (kv_q8_) {   // 8-bit store, then rows [0, start_pos + T) rounded to half into the one-layer scratch the unchanged F16 kernels read
            void* kc8 = kv_.k(kv.slot, i);   // (kc / vc: the image, shared by all slots: rebuilt here, for this slot, every pass)
            void* vc8 = kv_.v(kv.slot, i);
            if (T >= 4) {
                ok(ntk_rope_kv_store_q8_tab(act.q, act.k, act.v, positions_, T, nh, nkv, hd, cfg_.rope_theta, cfg_.rope_freq_scale, cfg_.rope_interleaved,
                                            kc8, vc8, start_pos, cfg_.max_seq_len, rope_tab(), s));
            } else {
                ok(ntk_rope_tab(act.q, act.k, positions_, 1, T, nh, nkv, hd, cfg_.rope_theta, cfg_.rope_freq_scale, cfg_.rope_interleaved, rope_tab(), s));
                ok(ntk_kv_store_q8(kc8, vc8, act.k, act.v, T, nkv, hd, start_pos, cfg_.max_seq_len, s));
            }
            ok(ntk_kv_dequant_q8_f16(kc, vc, kc8, vc8, start_pos + T, nkv, hd, cfg_.max_seq_len, s));
        } else if (with_max && T >= 4 && hd <= 256) {   // (the prompt form of the rotation: ntk_rope takes it from 4 tokens on, too)
            ok(ntk_rope_kv_store_tab(act.q, act.k, act.v, positions_, T, nh, nkv, hd, cfg_.rope_theta, cfg_.rope_freq_scale, cfg_.rope_interleaved, kc, vc,
                                     start_pos, cfg_.max_seq_len, rope_tab(), s));
        } else {
            ok(ntk_rope_tab(act.q, act.k, positions_, 1, T, nh, nkv, hd, cfg_.rope_theta, cfg_.rope_freq_scale, cfg_.rope_interleaved, rope_tab(), s));
            ok(ntk_copy_to_kv_cache(kc, vc, act.k, act.v, T, nkv, hd, start_pos, cfg_.max_seq_len, s));
        }
        if (kv.slots) {}   // (attended above)
        else if (T == 1) ok(ntk_attention_decode(act.attn_out, act.q, kc, vc, start_pos + T, nh, nkv, hd, cfg_.max_seq_len, scale, s));
        else ok(ntk_attention_prefill(act.attn_out, act.q, kc, vc, T, start_pos, nh, nkv, hd, cfg_.max_seq_len, scale, s));
        if (!project_add_norm(L.wo, act.attn_out, nullptr, L.ffn_norm, false, L.w_gate)) {
            project_add(L.wo, act.attn_out, qd, nullptr);
            norm(L.ffn_norm, false, L.w_gate);
        }
        if (!gate_up_silu(L)) {
            float* const ys[2] = {act.gate, act.up};
            const DevTensor* const ws[2] = {&L.w_gate, &L.w_up};
            project_many(ys, ws, 2, residual_, rm_a);
            silu_mul(L.w_down);
        }
        // down projection + residual, and the NEXT layer's first RMSNorm in the same consumer launch when there is a next layer in this pass
        if (i + 1 < last_layer && project_add_norm(L.w_down, act.gate, rm_b, layers_[i + 1].attn_norm, true, layers_[i + 1].wq)) normed_ahead = true;
        else project_add(L.w_down, act.gate, I, rm_b);
        if (rc != NTK_OK) break;
    }
    if (raw_err_ != NTK_OK) { rc = raw_err_; raw_err_ = NTK_OK; }   // what raw_of() could not report through its pointer (it precedes the consumer's NTK_E_NULL)
    return rc;
}

// ---------------------------------------------------------------------------------------------------
// Scoring: the same prompt pass, then every position's logits in chunks of score_rows_ rows (see model.h)
// ---------------------------------------------------------------------------------------------------
int Model::set_score_rows(int rows) {
    if (rows < 1 || rows > 1024) { err_ = "score_rows must lie in 1 .. 1024"; return NTK_E_SHAPE; }
    score_rows_ = rows;
    return NTK_OK;
}

int Model::score_buffers() {
    const size_t S = (size_t)cfg_.max_seq_len, V = (size_t)cfg_.vocab_size;
    auto dev = [&](size_t bytes) -> void* {
        void* p = nt_hip_malloc(bytes + 256);
        if (p) allocs_.push_back(p);
        return p;
    };
    auto release = [&](auto*& p) {
        if (!p) return;
        allocs_.erase(std::remove(allocs_.begin(), allocs_.end(), (void*)p), allocs_.end());
        nt_hip_free(p);
        p = nullptr;
    };
    auto fail = [&](const char* what) { err_ = std::string("score: no device memory for ") + what; return NTK_E_NOMEM; };
    if (!score_targets_ && !(score_targets_ = (int*)dev(S * 4))) return fail("the targets");
    if (!score_logprob_ && !(score_logprob_ = (float*)dev(S * 4))) return fail("the results");
    if (!score_top1_ && !(score_top1_ = (int*)dev(S * 4))) return fail("the results");
    if (score_cap_ < score_rows_) {
        NT_TRY(sync());   // (an earlier call's launches may still read the smaller buffer)
        release(score_logits_);
        score_cap_ = 0;
        if (!(score_logits_ = (float*)dev((size_t)score_rows_ * V * 4))) return fail("the chunk of logits (score_rows x vocab floats)");
        score_cap_ = score_rows_;
    }
    return lm_head_workspace("score");
}

// the FP16 GEMM sizes its workspace by the matrix's rows: the load-time one covers the layers' projections, not always a vocabulary
int Model::lm_head_workspace(const char* who) {
    const size_t need = ntk_gemm_quant_workspace_bytes(cfg_.hidden_size, cfg_.vocab_size);
    if (!(gemm_ws_ && bf16_prefill_ && f16_ok(output_) && need > gemm_ws_bytes_ && need > score_ws_bytes_)) return NTK_OK;
    if (score_ws_) {
        NT_TRY(sync());
        allocs_.erase(std::remove(allocs_.begin(), allocs_.end(), score_ws_), allocs_.end());
        nt_hip_free(score_ws_);
        score_ws_ = nullptr;
    }
    score_ws_bytes_ = 0;
    if (!(score_ws_ = nt_hip_malloc(need + 256))) { err_ = std::string(who) + ": no device memory for the LM head's GEMM workspace"; return NTK_E_NOMEM; }
    allocs_.push_back(score_ws_);
    score_ws_bytes_ = need;
    return NTK_OK;
}

bool Model::lm_head_f16() const { return batched_prefill_ && is_quant(output_.dtype) && bf16_prefill_ && gemm_ws_ && f16_ok(output_); }

// logits of n final-normed rows: one pass over the head (see model.h)
int Model::lm_head(float* logits, const float* X, int n, const float* chunk_max) {
    const DevTensor& w = output_;
    const int H = cfg_.hidden_size, V = cfg_.vocab_size;
    void* s = stream_;
    const bool batched = batched_prefill_ && is_quant(w.dtype);
    void* const ws = score_ws_ ? score_ws_ : gemm_ws_;
    const size_t ws_bytes = score_ws_ ? score_ws_bytes_ : gemm_ws_bytes_;
    int st = NTK_E_DTYPE;
    if (lm_head_f16()) {
        const bool repacked = rp_only(w);
        if (!repacked) raw_begin();
        const ntk_gemv_seg seg{repacked ? w.rp : raw_of(w), logits, V, w.dtype};
        ntk_gemm_desc d{};
        d.segs = &seg; d.nseg = 1; d.X = X; d.n_tokens = n; d.in_features = H;
        d.workspace = ws; d.workspace_bytes = ws_bytes; d.row_max = chunk_max; d.weights_repacked = repacked ? 1 : 0;
        d.full_form = 1;   // the same bits whatever the caller cuts the rows into (the form is otherwise chosen by the call's token count)
        st = ntk_gemm_quant_f16(&d, s);
    }
    if (batched && not_taken(st)) { raw_begin(); st = ntk_gemm_quant(logits, raw_of(w), X, n, V, H, w.dtype, nullptr, s); }
    if (batched && !not_taken(st)) return st;
    raw_begin();   // dense heads and shapes the matrix-core forms do not take: the reference's GEMV, row by row
    const void* wp = raw_of(w);
    for (int t = 0; t < n; ++t) {
        st = ntk_gemv(logits + (size_t)t * V, wp, X + (size_t)t * H, V, H, w.dtype, s);
        if (st == NTK_E_DTYPE) fprintf(stderr, "Unsupported dtype for GEMV: %s\n", dtype_name(w.dtype));   // gemm.cu:801-803
        if (st != NTK_OK) return st;
    }
    return NTK_OK;
}

int Model::score(const int* tokens, const int* targets, int T, int start_pos, float* logprob_out, int* top1_out, int slot) {
    if (!tokens || !targets || !logprob_out) { err_ = "score: null argument"; return NTK_E_NULL; }
    if (tp_world_ > 1) { err_ = "score: not available under tensor parallelism"; return NTK_E_SHAPE; }
    if (T <= 0) { err_ = "score: no tokens to score"; return NTK_E_SHAPE; }
    if (start_pos < 0 || start_pos + T > cfg_.max_seq_len) { err_ = "score: sequence exceeds context"; return NTK_E_SHAPE; }
    if (slot < 0 || slot >= sequences_) { err_ = "score: no such sequence slot"; return NTK_E_SHAPE; }
    const int H = cfg_.hidden_size, V = cfg_.vocab_size;
    for (int i = 0; i < T; ++i) {   // the embedding gather and the target gather index with these on the device
        if (tokens[i] < 0 || tokens[i] >= V) { err_ = "score: token id out of range"; return NTK_E_SHAPE; }
        if (targets[i] >= V) { err_ = "score: target id out of range"; return NTK_E_SHAPE; }
    }
    NT_TRY(score_buffers());
    void* s = stream_;
    tp_call_ = 0;
    // embedding and positions as forward() has them
    NT_TRY(ntk_memcpy_h2d_async(tokens_dev_, tokens, (size_t)T * 4, s));
    NT_TRY(ntk_memcpy_h2d_async(score_targets_, targets, (size_t)T * 4, s));
    const int est = ntk_embed_rows(hidden_, token_embd_.ptr, tokens_dev_, T, H, token_embd_.dtype, s);
    if (est == NTK_E_DTYPE) fprintf(stderr, "Error: Unsupported embedding dtype: %s\n", dtype_name(token_embd_.dtype));
    else if (est != NTK_OK) return est;
    std::vector<int> pos(T);
    for (int i = 0; i < T; ++i) pos[i] = start_pos + i;
    NT_TRY(ntk_memcpy_h2d_async(positions_, pos.data(), (size_t)T * 4, s));
    NT_TRY(ntk_stream_synchronize(s));   // `pos` / `tokens` / `targets` are host memory of the caller

    const KvTarget kv{slot, nullptr, 0};
    int rc = layers_1to1(T, start_pos, 0, cfg_.n_layers, kv);
    auto ok = [&](int st) { if (st != NTK_OK && rc == NTK_OK) rc = st; };
    // the final RMSNorm of every row, beside hidden_ (with the rows' largest |x| where the FP16 GEMM reads the head)
    const float* rm = lm_head_f16() && row_max_ && prefill_row_max_ ? row_max_ : nullptr;
    if (rm) ok(ntk_rmsnorm_rowmax(residual_, hidden_, (const float*)output_norm_.ptr, T, H, cfg_.norm_eps, row_max_, nullptr, s));
    else ok(ntk_rmsnorm(residual_, hidden_, (const float*)output_norm_.ptr, T, H, cfg_.norm_eps, s));
    for (int t0 = 0; t0 < T && rc == NTK_OK; t0 += score_rows_) {
        const int n = std::min(score_rows_, T - t0);
        ok(lm_head(score_logits_, residual_ + (size_t)t0 * H, n, rm ? rm + t0 : nullptr));
        ok(ntk_logprob_rows(score_logits_, n, V, V, score_targets_ + t0, score_logprob_ + t0, top1_out ? score_top1_ + t0 : nullptr, s));
    }
    if (rc == NTK_OK) ok(ntk_memcpy_d2h_async(logprob_out, score_logprob_, (size_t)T * 4, s));
    if (rc == NTK_OK && top1_out) ok(ntk_memcpy_d2h_async(top1_out, score_top1_, (size_t)T * 4, s));
    ok(ntk_stream_synchronize(s));
    if (raw_err_ != NTK_OK) { rc = raw_err_; raw_err_ = NTK_OK; }
    if (rc != NTK_OK && (err_.empty() || rc != NTK_E_LAUNCH)) err_ = std::string("score failed: ") + ntk_status_string(rc);
    return rc;
}

// ---------------------------------------------------------------------------------------------------
// Sequence slots: one decode step of B sequences in one pass over the weights (see model.h)
// ---------------------------------------------------------------------------------------------------
int Model::batch_buffers() {
    const size_t V = (size_t)cfg_.vocab_size, N = kMaxSequences;
    // (a buffer an earlier, failed call obtained is kept: only what is missing is allocated)
    auto need = [&](auto*& p, size_t bytes) {
        if (p) return true;
        void* d = nt_hip_malloc(bytes + 256);
        if (!d) return false;
        allocs_.push_back(d);
        nt_hip_memset(d, 0, bytes);
        p = static_cast<std::remove_reference_t<decltype(p)>>(d);
        return true;
    };
    if (!need(batch_in_, 3 * N * 4) || !need(batch_logprob_, N * 4) || !need(batch_next_, N * 4) ||
        !need(batch_attn_scratch_, N * ntk_attention_split_scratch_bytes(cfg_.n_heads, cfg_.head_dim, kMaxAttnSplits)) || !need(batch_logits_, N * V * 4)) {
        err_ = "decode_batch: no device memory for the batch buffers (16 x vocab floats of logits)";
        return NTK_E_NOMEM;
    }
    return lm_head_workspace("decode_batch");   // (nothing to do once the workspace is large enough)
}

int Model::validate_batch(const int* slots, const int* tokens, const int* positions, int B, int sequences, int max_seq, int vocab, std::string* why) {
    auto fail = [&](int rc, const char* msg) { if (why) *why = msg; return rc; };
    if (!slots || !tokens || !positions) return fail(NTK_E_NULL, "decode_batch: null argument");
    if (B < 1 || B > sequences || B > kMaxSequences) return fail(NTK_E_SHAPE, "decode_batch: the batch must hold 1 .. `sequences` rows");
    unsigned seen = 0;
    for (int b = 0; b < B; ++b) {
        if (slots[b] < 0 || slots[b] >= sequences || slots[b] >= kMaxSequences) return fail(NTK_E_SHAPE, "decode_batch: no such sequence slot");
        if (seen & (1u << slots[b])) return fail(NTK_E_SHAPE, "decode_batch: the same sequence slot twice in one batch");
        seen |= 1u << slots[b];
        if (positions[b] < 0 || positions[b] >= max_seq) return fail(NTK_E_SHAPE, "decode_batch: position outside the context");
        if (tokens[b] < 0 || tokens[b] >= vocab) return fail(NTK_E_SHAPE, "decode_batch: token id out of range");
    }
    return NTK_OK;
}

// the step up to its logits: tokens | positions up, embedding, the layer loop in batch mode, final RMSNorm, LM head into batch_logits_ (all queued, no wait)
int Model::batch_logits(const int* slots, const int* tokens, const int* positions, int B) {
    const int H = cfg_.hidden_size, N = kMaxSequences;
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
    const int est = ntk_embed_rows(hidden_, token_embd_.ptr, batch_in_, B, H, token_embd_.dtype, s);
    if (est == NTK_E_DTYPE) fprintf(stderr, "Error: Unsupported embedding dtype: %s\n", dtype_name(token_embd_.dtype));
    else if (est != NTK_OK) return est;

    int rc = layers_1to1(B, 0, 0, cfg_.n_layers, kv);
    auto ok = [&](int st) { if (st != NTK_OK && rc == NTK_OK) rc = st; };
    const float* rm = lm_head_f16() && row_max_ && prefill_row_max_ ? row_max_ : nullptr;
    if (rm) ok(ntk_rmsnorm_rowmax(residual_, hidden_, (const float*)output_norm_.ptr, B, H, cfg_.norm_eps, row_max_, nullptr, s));
    else ok(ntk_rmsnorm(residual_, hidden_, (const float*)output_norm_.ptr, B, H, cfg_.norm_eps, s));
    ok(lm_head(batch_logits_, residual_, B, rm));
    return rc;
}

int Model::decode_batch(const int* slots, const int* tokens, const int* positions, int B, float* logits_out, int* next_out) {
    NT_TRY(validate_batch(slots, tokens, positions, B, sequences_, cfg_.max_seq_len, cfg_.vocab_size, &err_));
    if ((kv_q8_ && !batch_kv_q8_) || tp_world_ > 1) { err_ = "decode_batch: not available with kv_cache=q8_0 or tensor parallelism"; return NTK_E_SHAPE; }
    NT_TRY(batch_buffers());
    const int V = cfg_.vocab_size, N = kMaxSequences;
    void* s = stream_;
    int rc = batch_logits(slots, tokens, positions, B);
    auto ok = [&](int st) { if (st != NTK_OK && rc == NTK_OK) rc = st; };
    if (next_out) ok(ntk_logprob_rows(batch_logits_, B, V, V, batch_in_ + 2 * N, batch_logprob_, batch_next_, s));
    if (rc == NTK_OK && logits_out) ok(ntk_memcpy_d2h_async(logits_out, batch_logits_, (size_t)B * V * 4, s));
    if (rc == NTK_OK && next_out) ok(ntk_memcpy_d2h_async(next_out, batch_next_, (size_t)B * 4, s));
    ok(ntk_stream_synchronize(s));
    if (raw_err_ != NTK_OK) { rc = raw_err_; raw_err_ = NTK_OK; }
    if (rc != NTK_OK && (err_.empty() || rc != NTK_E_LAUNCH)) err_ = std::string("decode_batch failed: ") + ntk_status_string(rc);
    return rc;
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
        if (slots[i] < 0 || slots[i] >= sequences || slots[i] >= kMaxSequences) return fail(NTK_E_SHAPE, "forward_batch: no such sequence slot");
        if (seen & (1u << slots[i])) return fail(NTK_E_SHAPE, "forward_batch: the same sequence slot twice in one pass");
        seen |= 1u << slots[i];
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
    const int est = ntk_embed_rows(hidden_, token_embd_.ptr, tokens_dev_, T, H, token_embd_.dtype, s);
    if (est == NTK_E_DTYPE) fprintf(stderr, "Error: Unsupported embedding dtype: %s\n", dtype_name(token_embd_.dtype));
    else if (est != NTK_OK) return est;

    KvTarget kv{0, slots, 0};
    kv.segs = &segs;
    int rc = layers_1to1(T, 0, 0, cfg_.n_layers, kv);
    auto ok = [&](int st) { if (st != NTK_OK && rc == NTK_OK) rc = st; };
    // the last row of every segment, gathered (hidden_ read as an F32 table) into n contiguous rows; the final RMSNorm and the LM head over those alone
    ok(ntk_embed_rows(residual_, hidden_, batch_in_, n, H, NTK_DT_F32, s));
    const float* rm = lm_head_f16() && row_max_ && prefill_row_max_ ? row_max_ : nullptr;
    if (rm) ok(ntk_rmsnorm_rowmax(hidden_, residual_, (const float*)output_norm_.ptr, n, H, cfg_.norm_eps, row_max_, nullptr, s));
    else ok(ntk_rmsnorm(hidden_, residual_, (const float*)output_norm_.ptr, n, H, cfg_.norm_eps, s));
    ok(lm_head(batch_logits_, hidden_, n, rm));
    if (next_out) ok(ntk_logprob_rows(batch_logits_, n, V, V, batch_in_ + 2 * N, batch_logprob_, batch_next_, s));
    if (rc == NTK_OK && logits_out) ok(ntk_memcpy_d2h_async(logits_out, batch_logits_, (size_t)n * V * 4, s));
    if (rc == NTK_OK && next_out) ok(ntk_memcpy_d2h_async(next_out, batch_next_, (size_t)n * 4, s));
    ok(ntk_stream_synchronize(s));
    if (raw_err_ != NTK_OK) { rc = raw_err_; raw_err_ = NTK_OK; }
    if (rc != NTK_OK && (err_.empty() || rc != NTK_E_LAUNCH)) err_ = std::string("forward_batch failed: ") + ntk_status_string(rc);
    return rc;
}

int Model::batch_sample_buffers() {
    const size_t N = kMaxSequences;
    auto need = [&](auto*& p, size_t bytes) {
        if (p) return true;
        void* d = nt_hip_malloc(bytes + 256);
        if (!d) return false;
        allocs_.push_back(d);
        p = static_cast<std::remove_reference_t<decltype(p)>>(d);
        return true;
    };
    if (!need(batch_recent_, N * kRecentCap * 4) || !need(batch_sample_scratch_, ntk_sample_rows_scratch_bytes((int)N, cfg_.vocab_size))) {
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
    int rc = batch_logits(slots, tokens, positions, B);
    auto ok = [&](int st) { if (st != NTK_OK && rc == NTK_OK) rc = st; };
    // the logits as the step computed them: queued AHEAD of the sampler, whose penalty rewrites batch_logits_ in place
    if (rc == NTK_OK && logits_out) ok(ntk_memcpy_d2h_async(logits_out, batch_logits_, (size_t)B * V * 4, s));
    for (int b = 0; b < B && rc == NTK_OK && row_logits; ++b)
        if (row_logits[b]) ok(ntk_memcpy_d2h_async(row_logits[b], batch_logits_ + (size_t)b * V, (size_t)V * 4, s));
    if (rc == NTK_OK) ok(ntk_sample_rows_top_k(batch_logits_, B, V, V, batch_recent_, pitch, &dev, batch_next_, h_batch_next_, batch_sample_scratch_, s));
    ok(ntk_stream_synchronize(s));
    if (raw_err_ != NTK_OK) { rc = raw_err_; raw_err_ = NTK_OK; }
    if (rc == NTK_OK) for (int b = 0; b < B; ++b) next_out[b] = h_batch_next_[b];
    if (rc != NTK_OK && (err_.empty() || rc != NTK_E_LAUNCH)) err_ = std::string("decode_batch_sample failed: ") + ntk_status_string(rc);
    return rc;
}

}  // namespace nt
