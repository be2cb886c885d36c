// engine/model_prompt.cpp -- the prompt pass of one sequence: forward, its layer loop, the LM head, scoring; the steps every host-driven pass shares (see model.h)
#include "model_impl.h"
#include "../gemm_dense16_plan.h"   // (ntk::gd_worth: the token counts the 16-bit GEMM is measured to win at)

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
    if (embed_rows(hidden_, tokens_dev_, T) != NTK_OK) return nullptr;
    if (upload_positions(T, start_pos) != NTK_OK) return nullptr;
    if (ntk_stream_synchronize(s) != NTK_OK) return nullptr;   // the positions' image / `tokens` are host temporaries

    const KvTarget kv{slot, nullptr, 0};
    PassStatus ok{layers_1to1(T, start_pos, 0, cfg_.n_layers, kv)};
    float* last = hidden_ + (size_t)(T - 1) * H;
    ok(ntk_rmsnorm(last, last, (const float*)output_norm_.ptr, 1, H, cfg_.norm_eps, s));   // in place, :658-659
    raw_begin();
    const int st = gemv_logged(logits_, output_, raw_of(output_), last);
    if (st != NTK_E_DTYPE) ok(st);
    if (tp_world_ > 1) ok(ntk_tp_advance_epoch(tp_comm_, s));
    int rc = finish_pass("forward failed: ", ok.rc);
    if (rc == NTK_OK) rc = check_tp();   // (it leaves its own message)
    return rc == NTK_OK ? logits_ : nullptr;
}

// ---------------------------------------------------------------------------------------------------
// What the host-driven passes share: head (tokens' embedding, positions), tail (final norm, the end of the pass), the logged GEMV
// ---------------------------------------------------------------------------------------------------
int Model::embed_rows(float* out, const int* ids_dev, int n) {
    const int st = ntk_embed_rows(out, token_embd_.ptr, ids_dev, n, cfg_.hidden_size, token_embd_.dtype, stream_);
    if (st != NTK_E_DTYPE) return st;
    fprintf(stderr, "Error: Unsupported embedding dtype: %s\n", dtype_name(token_embd_.dtype));
    return NTK_OK;
}

int Model::upload_positions(int T, int start_pos) {
    host_positions_.resize((size_t)T);
    for (int i = 0; i < T; ++i) host_positions_[i] = start_pos + i;
    return ntk_memcpy_h2d_async(positions_, host_positions_.data(), (size_t)T * 4, stream_);
}

const float* Model::final_norm(float* dst, const float* src, int n, PassStatus& ok) {
    const float* nw = (const float*)output_norm_.ptr;
    const float* rm = lm_head_f16() && row_max_ && prefill_row_max_ ? row_max_ : nullptr;
    if (rm) ok(ntk_rmsnorm_rowmax(dst, src, nw, n, cfg_.hidden_size, cfg_.norm_eps, row_max_, nullptr, stream_));
    else ok(ntk_rmsnorm(dst, src, nw, n, cfg_.hidden_size, cfg_.norm_eps, stream_));
    return rm;
}

int Model::finish_pass(const char* failed, int rc) {
    const int sy = ntk_stream_synchronize(stream_);
    if (rc == NTK_OK) rc = sy;
    if (raw_err_ != NTK_OK) { rc = raw_err_; raw_err_ = NTK_OK; }
    if (rc != NTK_OK && (err_.empty() || rc != NTK_E_LAUNCH)) err_ = std::string(failed) + ntk_status_string(rc);
    return rc;
}

int Model::gemv_logged(float* y, const DevTensor& w, const void* wp, const float* x) {
    const int st = ntk_gemv(y, wp, x, (int)w.out_f, (int)w.in_f, w.dtype, stream_);
    if (st == NTK_E_DTYPE) fprintf(stderr, "Unsupported dtype for GEMV: %s\n", dtype_name(w.dtype));   // gemm.cu:801-803
    return st;
}

// The prompt pass's operand planes: the FP16 GEMM reads X split into FP16 planes, written into a workspace by its own pre-pass or by the launch that
// produced X (ntk_*_prepare_x: the projection then needs no pre-pass launch at all).  Two workspaces are used alternately.  The invariant: a producer
// never writes planes into the workspace whose partial sums it is reading -- a projection's deferred K splits lie in the workspace of its own planes, so
// the producer that consumes them takes other().  Planes come in two KINDS: the FP16 pieces the FP16 GEMM and the F16 matrices of the 16-bit GEMM read (what
// every producer writes), and the three bfloat16 pieces of a BF16 matrix (ntk_gemm_dense16's own pre-pass only); a workspace holds one kind at a time.
struct OperandPlanes {
    enum Kind { fp16, bf16 };
    void* ws[2];
    int cur = 0;
    const float* of = nullptr;   // the X whose planes lie in ws[cur] (Q, K, V and gate, up share one X)
    Kind kind = fp16;            // ... and which planes they are
    void* current() const { return ws[cur]; }
    bool hold(const float* X, Kind k = fp16) const { return X == of && k == kind; }
    void* other() { cur ^= 1; of = nullptr; return ws[cur]; }                // a producer is about to write planes: the workspace the last projection did NOT use
    void written(const float* X, bool split) { of = split ? X : nullptr; kind = fp16; }   // X has new contents: planes are stale unless its producer just split it
    void in_current(const float* X, Kind k = fp16) { of = X; kind = k; }     // a projection's pre-pass (or such a producer) has left X's planes in ws[cur]
};

// the formats and shapes ntk_gemm_quant_f16 takes
static bool f16_ok(const DevTensor& w) {
    const bool kq = w.dtype == NTK_DT_Q4_0 || w.dtype == NTK_DT_Q4_K || w.dtype == NTK_DT_Q5_K || w.dtype == NTK_DT_Q6_K;
    return (w.dtype == NTK_DT_Q8_0 || kq) && w.in_f % (kq ? 256 : 128) == 0 && w.out_f % 16 == 0 && (w.ptr || w.rp);
}
// a K-quant matrix whose GGUF bytes were freed after the load-time repack (one resident copy): the FP16 GEMM reads it FROM THE REPACK
// (ntk_gemm_desc.weights_repacked: identical bits) -- no unpack in front of the prompt launches
// the 16-bit matrices and shapes ntk_gemm_dense16 takes
static bool dense16_ok(const DevTensor& w) { return is_dense16(w.dtype) && w.in_f % 32 == 0 && w.out_f % 16 == 0 && w.ptr; }
static bool rp_only(const DevTensor& w) {
    return !w.ptr && w.rp && (w.dtype == NTK_DT_Q4_K || w.dtype == NTK_DT_Q5_K || w.dtype == NTK_DT_Q6_K) && w.out_f % 16 == 0;
}

// layers [first, last) of the 1:1 path on hidden_[T][H] at positions start_pos.. (positions_ already on the device)
int Model::layers_1to1(int T, int start_pos, int first, int last_layer, const KvTarget& kv) {
    const int H = cfg_.hidden_size, I = cfg_.intermediate_size, qd = cfg_.n_heads * cfg_.head_dim, kvd = cfg_.n_kv_heads * cfg_.head_dim;
    void* s = stream_;
    const Views act = views(T);
    PassStatus ok;
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
        const bool f16_planes = f16_ok(next_w) || (dense_mfma16_ && fusable(next_w.dtype) && next_w.dtype == NTK_DT_F16 && dense16_ok(next_w) && ntk::gd_worth(T));   // (BF16 matrices read planes of their own kind)
        if (with_max && prefill_fused_split_ && gemm_ws2_ != nullptr && T <= 64 && tp_world_ == 1 && f16_planes && (int)next_w.in_f == width) return XForm::split;
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
    // 1..3 F16 / BF16 matrices of one dtype sharing X on the 16-bit matrix cores (ntk_gemm_dense16), ONE launch; X's planes of that kind are reused when they
    // lie in the current workspace, and lie there after the launch.  Option dense_mfma16 = 0, or fewer tokens than the form is measured to win at
    // (gemm_dense16_plan.h: gd_worth): not taken (NTK_E_DTYPE), the caller runs the F32-MFMA form.
    auto dense16_group = [&](float* const* Ys, const DevTensor* const* Ws, int n, const float* X, const float* resid) {
        if (!dense_mfma16_ || !gemm_ws_ || !ntk::gd_worth(T)) return (int)NTK_E_DTYPE;
        ntk_gemv_seg segs[3];
        for (int k = 0; k < n; ++k) {
            if (!dense16_ok(*Ws[k])) return (int)NTK_E_SHAPE;
            segs[k] = {Ws[k]->ptr, Ys[k], (int)Ws[k]->out_f, Ws[k]->dtype};
        }
        const OperandPlanes::Kind kind = Ws[0]->dtype == NTK_DT_BF16 ? OperandPlanes::bf16 : OperandPlanes::fp16;
        ntk_gemm_desc d{};
        d.segs = segs; d.nseg = n; d.X = X; d.n_tokens = T; d.in_features = (int)Ws[0]->in_f; d.resid = resid;
        d.workspace = planes.current(); d.workspace_bytes = gemm_ws_bytes_; d.reuse_x = planes.hold(X, kind) ? 1 : 0;
        const int st = ntk_gemm_dense16(&d, s);
        if (st == NTK_OK) planes.in_current(X, kind);
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
    // Y = W . X (+ resid, which may be Y) for all T tokens on the matrix cores: the FP16 GEMM, else the F32-MFMA form.  false: a shape only the per-token
    // loop takes (NTK_E_ALIGN / NTK_E_SHAPE: nothing launched; *wp holds the GGUF bytes for it)
    auto gemm_mfma = [&](float* Y, const DevTensor& w, const float* X, const float* resid, const float* rm, const void** wp) {
        int st = NTK_E_DTYPE;
        if (is_dense16(w.dtype)) {   // 16-bit rows: the 16-bit matrix cores, else the F32-MFMA form (the FP16 GEMM has no decoder for them)
            raw_begin(); *wp = raw_of(w);
            const DevTensor* const one = &w;
            st = dense16_group(&Y, &one, 1, X, resid);
        }
        else st = gemm_f16(Y, w, X, resid, rm, nullptr, wp);
        if (not_taken(st)) st = ntk_gemm_quant(Y, *wp, X, T, (int)w.out_f, (int)w.in_f, w.dtype, resid, s);
        if (st == NTK_E_ALIGN || st == NTK_E_SHAPE) return false;
        ok(st);
        return true;
    };
    // (wp: the tensor's raw GGUF blocks -- resident, or unpacked from the repack by raw_of() once per projection, not per token)
    auto project = [&](float* Y, const DevTensor& w, const float* X, size_t ystride, size_t xstride, const float* rm) {
        const bool dense = ystride == (size_t)w.out_f && xstride == (size_t)w.in_f;
        const void* wp = nullptr;
        if (batched && fusable(w.dtype) && dense) {
            if (gemm_mfma(Y, w, X, nullptr, rm, &wp)) return;
        } else { raw_begin(); wp = raw_of(w); }
        for (int t = 0; t < T; ++t) {
            const int st = gemv_logged(Y + (size_t)t * ystride, w, wp, X + (size_t)t * xstride);
            if (st != NTK_E_DTYPE) ok(st);
        }
    };
    // matrices that share X (Q | K | V, gate | up): those of one format go out as ONE launch of the FP16 GEMM, the rest one by one
    auto project_many = [&](float* const* Ys, const DevTensor* const* Ws, int n, const float* X, const float* rm) {
        bool done[3] = {false, false, false};
        for (int a = 0; a < n && batched && (bf16_now || is_dense16(Ws[a]->dtype)); ++a) {
            if (done[a]) continue;
            const bool d16 = is_dense16(Ws[a]->dtype);
            if (d16 ? !(fusable(Ws[a]->dtype) && dense_mfma16_) : !bf16_now) continue;
            float* ys[3];
            const DevTensor* ws[3];
            int idx[3], m = 0;
            for (int b = a; b < n; ++b)
                if (!done[b] && Ws[b]->dtype == Ws[a]->dtype && Ws[b]->in_f == Ws[a]->in_f) { ys[m] = Ys[b]; ws[m] = Ws[b]; idx[m++] = b; }
            if (m < 2) continue;
            const int st = d16 ? dense16_group(ys, ws, m, X, nullptr) : gemm_group(ys, ws, m, X, nullptr, rm, nullptr, nullptr);
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
        if (dense && (bf16_now || is_dense16(w.dtype))) prepare_x(X, w);
        const void* wp = nullptr;   // (unused: project() below obtains the bytes again)
        if (dense && fusable(w.dtype) && gemm_mfma(hidden_, w, X, hidden_, rm, &wp)) return;
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
        if (!normed_ahead) norm(L.attn_norm, true, L.wq);
        normed_ahead = false;
        float* const qkv_out[3] = {act.q, act.k, act.v};
        const DevTensor* const qkv[3] = {&L.wq, &L.wk, &L.wv};
        project_many(qkv_out, qkv, 3, residual_, rm_a);
        // a Qwen2 layer's projection biases: one launch over the T rows of q | k | v, ahead of the capture and the rotation (a layer without: no launch)
        if (L.has_qkv_bias()) ok(ntk_qkv_bias(act.q, act.k, act.v, (const float*)L.bq.ptr, (const float*)L.bk.ptr, (const float*)L.bv.ptr, T, qd, kvd, s));
        // a Qwen3 layer's per-head RMSNorm of Q and K: one launch over every head of the T rows, behind the bias and ahead of the capture and the rotation
        if (L.has_qk_norm()) ok(ntk_qk_norm(act.q, act.k, (const float*)L.q_norm.ptr, (const float*)L.k_norm.ptr, T, cfg_.n_heads, cfg_.n_kv_heads, cfg_.head_dim, cfg_.norm_eps, s));
        if (i == kv_capture_layer_ && kv_capture_) {   // parity instrumentation: the F32 projections the store launches are about to read
            ok(ntk_copy(kv_capture_, act.k, T * kvd, s));
            ok(ntk_copy(kv_capture_ + (size_t)cfg_.max_seq_len * kvd, act.v, T * kvd, s));
            kv_capture_T_ = T;
        }
        ok(attend(i, T, start_pos, kv, act, with_max));
        if (L.is_moe()) {   // a mixture-of-experts layer: the plain output projection, then an unfused RMSNorm into F32 rows (no operand planes, no row maxima) and
            // the three routed-FFN launches on the T rows, in place on hidden_; the next layer's norm is not folded into anything (normed_ahead stays false)
            project_add(L.wo, act.attn_out, qd, nullptr);
            ok(moe_ffn(L, hidden_, T, false));
            if (ok.rc != NTK_OK) break;
            continue;
        }
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
        if (ok.rc != NTK_OK) break;
    }
    if (raw_err_ != NTK_OK) { ok.rc = raw_err_; raw_err_ = NTK_OK; }   // what raw_of() could not report through its pointer (it precedes the consumer's NTK_E_NULL)
    return ok.rc;
}

// One layer's KV step and attention, by what `kv` names and the cache's format (see model.h).  Every rotation takes rope_tab(): the frequency table when
// the model carries frequency divisors, NULL -- the in-kernel frequency -- otherwise.
int Model::attend(int layer, int T, int start_pos, const KvTarget& kv, const Views& act, bool fused_store) {
    const int hd = cfg_.head_dim, nh = cfg_.n_heads, nkv = cfg_.n_kv_heads, S = cfg_.max_seq_len;
    const float scale = 1.0f / sqrtf((float)hd), theta = cfg_.rope_theta, fscale = cfg_.rope_freq_scale;
    void* s = stream_;
    PassStatus ok;
    if (kv.segs) {   // a packed prompt pass: every segment rotated, stored and attended on its own slot's cache from its own start position, one launch each
        ntk_kv_segments segs = *kv.segs;
        kv_.fill(segs, kv.slots, layer);
        ok(ntk_rope_kv_store_segments_tab(act.q, act.k, act.v, &segs, nh, nkv, hd, theta, fscale, cfg_.rope_interleaved, S, rope_tab(), s));
        ok(ntk_attention_prefill_segments(act.attn_out, act.q, &segs, nh, nkv, hd, S, scale, s));
        return ok.rc;
    }
    if (kv.slots) {   // a batch of sequences: rope / store / attention of every row on its own cache at its own position, one launch
        ntk_kv_batch caches{};
        kv_.fill(caches, kv.slots, T, layer);
        const int* const positions = batch_in_ + kMaxSequences;
        if (kv_q8_) {   // ... over the 8-bit caches ("batch_kv_q8"): the single-row decode launch's splits for the batch's largest position
            return ntk_attention_decode_q8_batch(act.attn_out, act.q, act.k, act.v, &caches, positions, T, rope_inv_freq_, nh, nkv, hd, S, scale, theta, fscale,
                                                 kv_q8_splits(attention_regime(kv.max_pos, hd)), batch_attn_scratch_, s);
        }
        const bool splits_ok = batch_attn_scratch_ && (hd == 64 || hd == 128 || hd == 256);   // (pick_attention_regime's rule)
        const int regime = splits_ok ? attention_regime(kv.max_pos, hd) : 0;
        return ntk_attention_decode_batch(act.attn_out, act.q, act.k, act.v, &caches, positions, T, rope_inv_freq_, nh, nkv, hd, S, scale, theta, fscale,
                                          regime == 0 ? 1 : attention_splits(regime, hd), batch_attn_scratch_, s);
    }
    uint16_t* const kc = kv_.attend_k(kv.slot, layer);   // (q8_0: the one-layer F16 image, shared by all slots: rebuilt below, for this slot, every pass)
    uint16_t* const vc = kv_.attend_v(kv.slot, layer);
    if (kv_q8_) {   // 8-bit store, then rows [0, start_pos + T) rounded to half into the one-layer scratch the unchanged F16 kernels read
        void* kc8 = kv_.k(kv.slot, layer);
        void* vc8 = kv_.v(kv.slot, layer);
        if (T >= 4) {
            ok(ntk_rope_kv_store_q8_tab(act.q, act.k, act.v, positions_, T, nh, nkv, hd, theta, fscale, cfg_.rope_interleaved, kc8, vc8, start_pos, S, rope_tab(), s));
        } else {
            ok(ntk_rope_tab(act.q, act.k, positions_, 1, T, nh, nkv, hd, theta, fscale, cfg_.rope_interleaved, rope_tab(), s));
            ok(ntk_kv_store_q8(kc8, vc8, act.k, act.v, T, nkv, hd, start_pos, S, s));
        }
        ok(ntk_kv_dequant_q8_f16(kc, vc, kc8, vc8, start_pos + T, nkv, hd, S, s));
    } else if (fused_store && T >= 4 && hd <= 256) {   // (the prompt form of the rotation: ntk_rope takes it from 4 tokens on, too)
        ok(ntk_rope_kv_store_tab(act.q, act.k, act.v, positions_, T, nh, nkv, hd, theta, fscale, cfg_.rope_interleaved, kc, vc, start_pos, S, rope_tab(), s));
    } else {
        ok(ntk_rope_tab(act.q, act.k, positions_, 1, T, nh, nkv, hd, theta, fscale, cfg_.rope_interleaved, rope_tab(), s));
        ok(ntk_copy_to_kv_cache(kc, vc, act.k, act.v, T, nkv, hd, start_pos, S, s));
    }
    if (T == 1) ok(ntk_attention_decode(act.attn_out, act.q, kc, vc, start_pos + T, nh, nkv, hd, S, scale, s));
    else ok(ntk_attention_prefill(act.attn_out, act.q, kc, vc, T, start_pos, nh, nkv, hd, S, scale, s));
    return ok.rc;
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
    auto fail = [&](const char* what) { err_ = std::string("score: no device memory for ") + what; return NTK_E_NOMEM; };
    if (!dev_need(score_targets_, S * 4, false)) return fail("the targets");
    if (!dev_need(score_logprob_, S * 4, false)) return fail("the results");
    if (!dev_need(score_top1_, S * 4, false)) return fail("the results");
    if (score_cap_ < score_rows_) {
        NT_TRY(sync());   // (an earlier call's launches may still read the smaller buffer)
        dev_release(score_logits_);
        score_cap_ = 0;
        if (!dev_need(score_logits_, (size_t)score_rows_ * V * 4, false)) return fail("the chunk of logits (score_rows x vocab floats)");
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
        dev_release(score_ws_);
    }
    score_ws_bytes_ = 0;
    if (!dev_need(score_ws_, need, false)) { err_ = std::string(who) + ": no device memory for the LM head's GEMM workspace"; return NTK_E_NOMEM; }
    score_ws_bytes_ = need;
    return NTK_OK;
}

bool Model::lm_head_f16() const { return batched_prefill_ && is_quant(output_.dtype) && bf16_prefill_ && gemm_ws_ && f16_ok(output_); }

// logits of n final-normed rows: one pass over the head (see model.h)
int Model::lm_head(float* logits, const float* X, int n, const float* chunk_max) {
    const DevTensor& w = output_;
    const int H = cfg_.hidden_size, V = cfg_.vocab_size;
    void* s = stream_;
    const bool batched = batched_prefill_ && fusable(w.dtype) && (is_quant(w.dtype) || n > 1);   // (one row of a 16-bit head: the GEMV reads as many bytes)
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
    if (batched && is_dense16(w.dtype) && dense_mfma16_ && ws && dense16_ok(w) && ntk::gd_worth(n)) {   // a 16-bit head over more than one row: the 16-bit matrix cores
        const ntk_gemv_seg seg{w.ptr, logits, V, w.dtype};
        ntk_gemm_desc d{};
        d.segs = &seg; d.nseg = 1; d.X = X; d.n_tokens = n; d.in_features = H;
        d.workspace = ws; d.workspace_bytes = ws_bytes;
        st = ntk_gemm_dense16(&d, s);
    }
    if (batched && not_taken(st)) { raw_begin(); st = ntk_gemm_quant(logits, raw_of(w), X, n, V, H, w.dtype, nullptr, s); }
    if (batched && !not_taken(st)) return st;
    raw_begin();   // dense heads and shapes the matrix-core forms do not take: the reference's GEMV, row by row
    const void* wp = raw_of(w);
    for (int t = 0; t < n; ++t) {
        st = gemv_logged(logits + (size_t)t * V, w, wp, X + (size_t)t * H);
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
    NT_TRY(embed_rows(hidden_, tokens_dev_, T));
    NT_TRY(upload_positions(T, start_pos));
    NT_TRY(ntk_stream_synchronize(s));   // the positions' image / `tokens` / `targets` are host temporaries

    const KvTarget kv{slot, nullptr, 0};
    PassStatus ok{layers_1to1(T, start_pos, 0, cfg_.n_layers, kv)};
    const float* rm = final_norm(residual_, hidden_, T, ok);   // of every row, beside hidden_
    for (int t0 = 0; t0 < T && ok.rc == NTK_OK; t0 += score_rows_) {
        const int n = std::min(score_rows_, T - t0);
        ok(lm_head(score_logits_, residual_ + (size_t)t0 * H, n, rm ? rm + t0 : nullptr));
        ok(ntk_logprob_rows(score_logits_, n, V, V, score_targets_ + t0, score_logprob_ + t0, top1_out ? score_top1_ + t0 : nullptr, s));
    }
    if (ok.rc == NTK_OK) ok(ntk_memcpy_d2h_async(logprob_out, score_logprob_, (size_t)T * 4, s));
    if (ok.rc == NTK_OK && top1_out) ok(ntk_memcpy_d2h_async(top1_out, score_top1_, (size_t)T * 4, s));
    return finish_pass("score failed: ", ok.rc);
}

}  // namespace nt
