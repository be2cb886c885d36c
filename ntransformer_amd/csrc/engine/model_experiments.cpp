// engine/model_experiments.cpp -- the engine's hooks for the structures kept under experiments/ (persistent token kernel, layer engine, attention inside the
// Wo launch; see model.h).  experiments/Makefile compiles the bodies (-DNTK_EXPERIMENTS); the product gets the stubs: nothing is ever taken.
#include "model_impl.h"
#ifdef NTK_EXPERIMENTS
#include "ntk_experiments.h"
#endif

namespace nt {

#ifndef NTK_EXPERIMENTS
bool Model::experiments_built() { return false; }
int Model::build_persistent_plan(int) { return NTK_E_SHAPE; }
void Model::destroy_persistent_plan() { persistent_plan_ = nullptr; }
int Model::launch_persistent() { return NTK_E_SHAPE; }
int Model::attention_in_wo(const LayerWeights&, int) { return NTK_E_SHAPE; }
int Model::check_experiments() { return NTK_OK; }
#else
bool Model::experiments_built() { return true; }

void Model::destroy_persistent_plan() {   // ... and the tokens captured with it
    drop_graphs(kPersistentSlot);
    if (persistent_plan_) { if (persistent_kind_ == 2) ntk_layer_engine_plan_destroy(persistent_plan_); else ntk_persistent_plan_destroy(persistent_plan_); }
    persistent_plan_ = nullptr;
}

int Model::launch_persistent() {
    return persistent_kind_ == 2 ? ntk_layer_engine_launch(persistent_plan_, d_pos_, stream_) : ntk_persistent_launch(persistent_plan_, d_pos_, stream_);
}

// attention producers inside the Wo launch: one launch, one boundary and one first-byte latency less per layer
int Model::attention_in_wo(const LayerWeights& L, int layer) {
    if (attn_regime_ != 0 || !fuse_attention_ || kv_q8_ || !attn_sync_ || !is_quant(L.wo.dtype) || tp_world_ != 1) return NTK_E_SHAPE;
    const int hd = cfg_.head_dim, nh = cfg_.n_heads, nkv = cfg_.n_kv_heads;
    const Views act = views(1);
    raw_begin();
    ntk_gemv_seg wo = {raw_of(L.wo), hidden_, (int)L.wo.out_f, L.wo.dtype};
    prof_mark(0, true);
    const int st = ntk_attention_gemv_fused(act.attn_out, act.q, act.k, act.v, kv_.k_f16(0, layer), kv_.v_f16(0, layer), d_pos_,
                                            rope_inv_freq_, nh, nkv, hd, cfg_.max_seq_len, 1.0f / sqrtf((float)hd), cfg_.rope_theta, cfg_.rope_freq_scale, &wo,
                                            hidden_, attn_sync_, stream_);
    prof_mark(0, false);
    return st;
}

int Model::check_experiments() {
    if (attn_sync_ && fuse_attention_) {   // ntk_attention_gemv_fused: a bounded in-kernel wait that gave up
        unsigned w[3] = {0, 0, 0};
        if (ntk_memcpy_d2h_async(w, attn_sync_, sizeof w, stream_) != NTK_OK || ntk_stream_synchronize(stream_) != NTK_OK) return NTK_E_LAUNCH;
        if (w[2] != 0) {
            fuse_attention_ = false;
            nt_hip_memset(attn_sync_, 0, 4096);
            drop_graphs();
            err_ = "attention + Wo fused launch: the wait for the attention workgroups gave up; falling back to separate launches";
            fprintf(stderr, "%s\n", err_.c_str());
            return NTK_E_LAUNCH;
        }
    }
    if (!persistent_plan_ || !persistent_on_) return NTK_OK;
    int op = -1;
    int st;
    if (persistent_kind_ == 2) {
        unsigned code = 0;
        st = ntk_layer_engine_error(persistent_plan_, &code);
        op = code ? (int)((code - 1u) & 4095u) : -1;
        if (st != NTK_OK) fprintf(stderr, "layer engine: error word %u (operator %d, wait kind %u, CU %u)\n", code, op, ((code - 1u) >> 12) & 15u, (code - 1u) >> 16);
    } else {
        st = ntk_persistent_error(persistent_plan_, &op);
    }
    if (st != NTK_OK) {
        persistent_on_ = false;
        err_ = "persistent decode kernel: a bounded grid wait gave up at operator " + std::to_string(op) + "; falling back to launches";
        fprintf(stderr, "%s\n", err_.c_str());
    }
    return st;
}

// The token's operator table for the persistent kernel: exactly the sequence enqueue_token() launches.
int Model::build_persistent_plan(int kind) {
    const int H = cfg_.hidden_size, I = cfg_.intermediate_size, hd = cfg_.head_dim, nh = cfg_.n_heads, nkv = cfg_.n_kv_heads;
    if (hd != 64 && hd != 128) return NTK_E_SHAPE;
    if (const char* e = getenv("NTK_NO_PERSISTENT")) { if (atoi(e)) return NTK_E_SHAPE; }
    const float scale = 1.0f / sqrtf((float)hd);
    const Views act = views(1);
    std::vector<ntk_pop> ops;
    bool ok = true;
    // n matrices sharing x: one operator per dtype group (Q4_K_M: attn_v is Q6_K / Q5_K next to Q4_K q, k); only the first
    // waits for x, only the last signals
    auto gemv_group = [&](const DevTensor* const* ws, float* const* ys, int n, const float* x, const DevTensor* norm, const float* resid,
                          bool wait, bool arrive, bool plain, int silu_pair = 0) {
        bool done[3] = {false, false, false};
        std::vector<ntk_pop> grp;
        for (int a = 0; a < n; ++a) {
            if (done[a]) continue;
            if (!is_quant(ws[a]->dtype)) { ok = false; return; }
            ntk_pop o;
            memset(&o, 0, sizeof o);
            o.kind = NTK_POP_GEMV;
            for (int b = a; b < n; ++b) {
                if (done[b] || ws[b]->dtype != ws[a]->dtype) continue;
                o.segs[o.nseg++] = {ws[b]->ptr, ys[b], (int)ws[b]->out_f, ws[b]->dtype};
                done[b] = true;
            }
            o.in_features = (int)ws[a]->in_f;
            o.eps = cfg_.norm_eps;
            o.x = x;
            o.norm_w = norm ? (const float*)norm->ptr : nullptr;
            o.resid = resid;
            o.plain_store = plain ? 1 : 0;
            o.silu_pair = silu_pair;
            grp.push_back(o);
        }
        for (size_t i = 0; i < grp.size(); ++i) {
            grp[i].wait = (wait && i == 0) ? 1 : 0;
            grp[i].arrive = (arrive && i + 1 == grp.size()) ? 1 : 0;
            ops.push_back(grp[i]);
        }
    };
    for (int i = 0; i < cfg_.n_layers && ok; ++i) {
        const LayerWeights& L = layers_[i];
        {
            const DevTensor* ws[3] = {&L.wq, &L.wk, &L.wv};
            float* ys[3] = {act.q, act.k, act.v};
            gemv_group(ws, ys, 3, hidden_, &L.attn_norm, nullptr, i > 0, true, false);   // layer 0 reads the embedding kernel's output
        }
        ntk_pop a;
        memset(&a, 0, sizeof a);
        a.kind = NTK_POP_ATTENTION; a.wait = 1; a.arrive = 1;
        a.out = act.attn_out; a.q = act.q; a.k = act.k; a.v = act.v;
        a.k_cache = kv_.k_f16(0, i); a.v_cache = kv_.v_f16(0, i);
        a.inv_freq = rope_inv_freq_;
        a.n_heads = nh; a.n_kv_heads = nkv; a.head_dim = hd; a.max_seq = cfg_.max_seq_len;
        a.scale = scale; a.theta_base = cfg_.rope_theta; a.freq_scale = cfg_.rope_freq_scale;
        ops.push_back(a);
        {
            const DevTensor* ws[1] = {&L.wo};
            float* ys[1] = {hidden_};
            gemv_group(ws, ys, 1, act.attn_out, nullptr, hidden_, true, true, false);
        }
        if (!(is_quant(L.w_gate.dtype) && L.w_gate.dtype == L.w_up.dtype)) { ok = false; break; }
        {   // (one format: one operator, SiLU x up in its epilogue)
            const DevTensor* ws[2] = {&L.w_gate, &L.w_up};
            float* ys[2] = {act.gate, act.up};
            gemv_group(ws, ys, 2, hidden_, &L.ffn_norm, nullptr, true, true, false, 1);
        }
        {
            const DevTensor* ws[1] = {&L.w_down};
            float* ys[1] = {hidden_};
            gemv_group(ws, ys, 1, act.gate, nullptr, hidden_, true, true, false);
        }
    }
    if (ok) {
        const DevTensor* ws[1] = {&output_};
        float* ys[1] = {logits_};
        gemv_group(ws, ys, 1, hidden_, &output_norm_, nullptr, true, false, true);
    }
    if (!ok) return NTK_E_DTYPE;
    persistent_kind_ = kind;
    if (kind == 2) return ntk_layer_engine_plan_create(ops.data(), (int)ops.size(), &persistent_plan_);
    return ntk_persistent_plan_create(ops.data(), (int)ops.size(), &persistent_plan_);
}
#endif

}  // namespace nt
