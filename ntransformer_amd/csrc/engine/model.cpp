// engine/model.cpp -- see model.h
#include "model.h"
#include "../../../include/ntk_engine.h"
#ifdef NTK_EXPERIMENTS
#include "ntk_experiments.h"
#endif

#include <hip/hip_runtime.h>
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <chrono>
#include <thread>

namespace nt {

#define NT_TRY(expr)                       \
    do {                                   \
        const int st__ = (expr);           \
        if (st__ != NTK_OK) return st__;   \
    } while (0)

static bool is_quant(int dt) {
    return dt == NTK_DT_Q8_0 || dt == NTK_DT_Q4_0 || dt == NTK_DT_Q4_K || dt == NTK_DT_Q5_K || dt == NTK_DT_Q6_K;
}

// the three statuses with which a launcher says "nothing was launched: try the next form"
static bool not_taken(int st) { return st == NTK_E_DTYPE || st == NTK_E_SHAPE || st == NTK_E_ALIGN; }

Model::~Model() { free_all(); }

void Model::free_all() {
    for (auto& row : graphs_)
        for (auto& gx : row) {
            if (gx) (void)hipGraphExecDestroy(reinterpret_cast<hipGraphExec_t>(gx));
            gx = nullptr;
        }
#ifdef NTK_EXPERIMENTS
    if (persistent_plan_) { if (persistent_kind_ == 2) ntk_layer_engine_plan_destroy(persistent_plan_); else ntk_persistent_plan_destroy(persistent_plan_); }
#endif
    persistent_plan_ = nullptr;
    persistent_on_ = false;
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
    if (h_token_) nt_hip_free_host(h_token_);
    h_token_ = nullptr;
    if (h_ring_) nt_hip_free_host(h_ring_);
    h_ring_ = nullptr;
    if (h_recent_) nt_hip_free_host(h_recent_);
    h_recent_ = nullptr;
    sample_scratch_ = nullptr;
    d_recent_ = nullptr;
    attn_sync_ = nullptr;
    gemm_ws_ = gemm_ws2_ = nullptr;
    shares_weights_ = false;   // (allocs_ held only this object's own buffers: the tensors belong to the model they were shared from)
    layers_.clear();
    // a second load() on the same object starts from a clean slate
    token_embd_ = output_norm_ = output_ = DevTensor();
    weight_bytes_ = 0;
    repack_bytes_ = 0;
    raw_freed_bytes_ = 0;
    raw_scratch_ = nullptr; raw_scratch_bytes_ = raw_cursor_ = 0; raw_err_ = 0;
    repack_done_ = false;
    output_tied_ = false;
    host_pos_ = 0;
    attn_regime_ = 0;
    k_cache_ = v_cache_ = nullptr;
    kv_capture_ = nullptr; kv_capture_layer_ = -1; kv_capture_T_ = 0;
    k_cache_q8_ = v_cache_q8_ = nullptr; kv_f16_k_ = kv_f16_v_ = nullptr; kv_q8_layer_bytes_ = 0; kv_cache_bytes_ = 0;
    hidden_ = residual_ = workspace_ = logits_ = argmax_scratch_ = rope_inv_freq_ = attn_scratch_ = row_max_ = nullptr;
    positions_ = tokens_dev_ = d_pos_ = d_token_ = nullptr;
}

int Model::upload(DevTensor& dst, const void* host, int dtype, int64_t in_f, int64_t out_f, size_t nbytes) {
    void* d = nt_hip_malloc((nbytes + 255) / 256 * 256 + 256);   // tail padding: kernels may read the last 16-byte chunk whole
    if (!d) { err_ = "out of device memory"; return NTK_E_NOMEM; }
    allocs_.push_back(d);
    if (host && nbytes) {   // a failed upload must not leave silently garbage weights behind
        if (hipMemcpy(d, host, nbytes, hipMemcpyHostToDevice) != hipSuccess) { err_ = "weight upload (H2D copy) failed"; return NTK_E_LAUNCH; }
    }
    dst.ptr = d; dst.dtype = dtype; dst.in_f = in_f; dst.out_f = out_f; dst.nbytes = nbytes;
    weight_bytes_ += nbytes;
    return NTK_OK;
}

// ---- tensor parallelism: slices ---------------------------------------------------------------------------------------------
int Model::tp_configure(int rank, int world) {
    if (world < 1 || world > 8 || rank < 0 || rank >= world) { err_ = "bad tensor-parallel rank / world"; return NTK_E_SHAPE; }
    if (!layers_.empty()) { err_ = "tp_configure must precede load"; return NTK_E_SHAPE; }
    tp_rank_ = rank;
    tp_world_ = world;
    return NTK_OK;
}

int Model::slice_columns(void* dst, const void* src, int dtype, int64_t out_f, int64_t in_f, int rank, int world) {
    if (!dst || !src) return NTK_E_NULL;
    if (world < 1 || rank < 0 || rank >= world || in_f % world != 0) return NTK_E_SHAPE;
    const int64_t in_l = in_f / world;
    const size_t rb_full = ntk_row_bytes(dtype, in_f), rb_loc = ntk_row_bytes(dtype, in_l);
    if (!rb_full || !rb_loc || rb_loc * (size_t)world != rb_full) return NTK_E_SHAPE;   // the slice must be whole blocks
    const uint8_t* s8 = static_cast<const uint8_t*>(src);
    uint8_t* d8 = static_cast<uint8_t*>(dst);
    for (int64_t r = 0; r < out_f; ++r) memcpy(d8 + (size_t)r * rb_loc, s8 + (size_t)r * rb_full + (size_t)rank * rb_loc, rb_loc);
    return NTK_OK;
}

int Model::upload_shard(DevTensor& dst, const void* host_full, int dtype, int64_t in_f, int64_t out_f, size_t nbytes_full, Shard how) {
    if (tp_world_ == 1 || how == WHOLE) return upload(dst, host_full, dtype, in_f, out_f, nbytes_full);
    if (how == ROWS) {   // rows are contiguous: a byte range
        const int64_t rows = out_f / tp_world_;
        const size_t rb = ntk_row_bytes(dtype, in_f);
        if (out_f % tp_world_ != 0 || !rb) { err_ = "tensor rows do not divide over the tensor-parallel ranks"; return NTK_E_SHAPE; }
        return upload(dst, static_cast<const uint8_t*>(host_full) + (size_t)tp_rank_ * rows * rb, dtype, in_f, rows, (size_t)rows * rb);
    }
    const int64_t in_l = in_f / tp_world_;
    const size_t rb_loc = ntk_row_bytes(dtype, in_l);
    std::vector<uint8_t> tmp((size_t)out_f * rb_loc);
    const int st = slice_columns(tmp.data(), host_full, dtype, out_f, in_f, tp_rank_, tp_world_);
    if (st != NTK_OK) { err_ = "tensor columns do not divide into whole blocks over the tensor-parallel ranks"; return st; }
    return upload(dst, tmp.data(), dtype, in_l, out_f, tmp.size());
}

int Model::tp_check_shapes() {
    if (tp_world_ == 1) return NTK_OK;
    if (cfg_.n_heads % tp_world_ || cfg_.n_kv_heads % tp_world_ || cfg_.intermediate_size % tp_world_) {
        err_ = "heads / KV heads / FFN width do not divide over the tensor-parallel ranks";
        return NTK_E_SHAPE;
    }
    return NTK_OK;
}

int Model::tp_export(void* handle64, void** raw) {
    if (!tp_comm_) return NTK_E_NULL;
    if (raw) *raw = tp_comm_;
    if (handle64) return ntk_ipc_export(tp_comm_, handle64);
    return NTK_OK;
}

int Model::tp_connect(const void* handles, void* const* raws) {
    if (tp_world_ == 1) { tp_connected_ = true; return NTK_OK; }
    if (!tp_comm_ || (!handles && !raws)) return NTK_E_NULL;
    for (int r = 0; r < tp_world_; ++r) {
        if (r == tp_rank_) { tp_peers_[r] = tp_comm_; continue; }
        if (raws) { tp_peers_[r] = raws[r]; continue; }
        void* p = nullptr;
        const int st = ntk_ipc_open(static_cast<const uint8_t*>(handles) + 64 * r, &p);
        if (st != NTK_OK) { err_ = "mapping a peer's communication buffer failed (hipIpcOpenMemHandle)"; return st; }
        tp_peers_[r] = p;
        tp_peer_opened_[r] = true;
    }
    for (int r = 0; r < tp_world_; ++r)
        if (!tp_peers_[r]) return NTK_E_NULL;
    tp_connected_ = true;
    return NTK_OK;
}

unsigned Model::tp_error() {
    if (!tp_comm_) return 0u;
    unsigned v = 0;   // read on the model's own stream (no legacy-stream traffic next to another rank's capture)
    if (ntk_memcpy_d2h_async(&v, static_cast<uint8_t*>(tp_comm_) + 128, 4, stream_) != NTK_OK || ntk_stream_synchronize(stream_) != NTK_OK) return ~0u;
    return v;
}
float* Model::tp_slot() const { return ntk_tp_slot(tp_comm_, tp_max_floats_, tp_call_); }
int Model::tp_allreduce(float* hidden, int n) {
    if (!tp_connected_) { err_ = "tensor-parallel ranks are not connected (tp_connect)"; return NTK_E_NULL; }
    const int st = ntk_tp_allreduce_add(hidden, tp_peers_, tp_rank_, tp_world_, tp_max_floats_, tp_call_, n, stream_);
    ++tp_call_;
    return st;
}

int Model::load(const std::string& path, int max_context) {
    const int st = load_impl(path, max_context);
    if (st != NTK_OK) free_all();   // nothing stays resident after a failed load
    return st;
}

int Model::load_impl(const std::string& path, int max_context) {
    free_all();
    fprintf(stderr, "Loading model: %s\n", path.c_str());
    GgufFile f;
    int st = f.open(path);
    if (st != NTK_OK) { err_ = f.error(); fprintf(stderr, "%s\n", err_.c_str()); return st; }
    cfg_ = f.config();
    vocab_ = f.vocab();
    if (cfg_.max_seq_len > max_context) {   // transformer.cpp:70-74
        fprintf(stderr, "Note: Capping context from %d to %d tokens (use --ctx-size to change)\n", cfg_.max_seq_len, max_context);
        cfg_.max_seq_len = max_context;
    }
    cfg_.print();
    f.print_info();
    int dev = 0;
    if (const char* e = getenv("NTK_DEVICE")) dev = atoi(e);
    st = ntk_device_init(dev);
    if (st != NTK_OK) { err_ = "no usable GPU (HIP device init failed)"; fprintf(stderr, "%s\n", err_.c_str()); return st; }

    const int H = cfg_.hidden_size, I = cfg_.intermediate_size, hd = cfg_.head_dim;
    const int64_t qd = (int64_t)cfg_.n_heads * hd, kvd = (int64_t)cfg_.n_kv_heads * hd;
    NT_TRY(tp_check_shapes());
    auto take = [&](const std::string& name, DevTensor& dst, int64_t in_f, int64_t out_f, bool vec, Shard how = WHOLE) -> int {
        const GgufTensor* t = f.find(name);
        if (!t) { err_ = "Tensor not found: " + name; return NTK_E_FORMAT; }
        if (t->numel() != in_f * out_f || (!vec && (t->dims.size() != 2 || t->dims[0] != in_f))) {
            err_ = "Unexpected shape for " + name;
            return NTK_E_SHAPE;
        }
        if (vec && t->dtype != NTK_DT_F32) { err_ = name + " must be F32"; return NTK_E_DTYPE; }
        if (t->nbytes == 0 || !t->known_type) { err_ = "Unsupported tensor type for " + name; return NTK_E_DTYPE; }
        return upload_shard(dst, f.data(*t), t->dtype, in_f, out_f, t->nbytes, how);
    };
    NT_TRY(take("token_embd.weight", token_embd_, H, cfg_.vocab_size, false));
    if (f.find("output.weight")) {   // transformer.cpp:92-99
        NT_TRY(take("output.weight", output_, H, cfg_.vocab_size, false));
    } else {
        output_ = token_embd_;
        output_tied_ = true;
    }
    NT_TRY(take("output_norm.weight", output_norm_, H, 1, true));
    layers_.resize(cfg_.n_layers);
    for (int i = 0; i < cfg_.n_layers; ++i) {   // transformer.cpp:286-328
        const std::string p = "blk." + std::to_string(i) + ".";
        LayerWeights& L = layers_[i];
        NT_TRY(take(p + "attn_norm.weight", L.attn_norm, H, 1, true));
        NT_TRY(take(p + "attn_q.weight", L.wq, H, qd, false, ROWS));      // whole heads per rank
        NT_TRY(take(p + "attn_k.weight", L.wk, H, kvd, false, ROWS));
        NT_TRY(take(p + "attn_v.weight", L.wv, H, kvd, false, ROWS));
        NT_TRY(take(p + "attn_output.weight", L.wo, qd, H, false, COLS));  // the columns of this rank's heads
        NT_TRY(take(p + "ffn_norm.weight", L.ffn_norm, H, 1, true));
        NT_TRY(take(p + "ffn_gate.weight", L.w_gate, H, I, false, ROWS));
        NT_TRY(take(p + "ffn_up.weight", L.w_up, H, I, false, ROWS));
        NT_TRY(take(p + "ffn_down.weight", L.w_down, I, H, false, COLS));
    }
    return finish_load(max_context);
}

int Model::load_synthetic(const SynthSpec& spec, int max_context, int nthreads) {
    free_all();
    std::vector<SynthTensor> plan;
    if (!synth_plan(spec, plan)) { err_ = "bad synthetic spec"; return NTK_E_SHAPE; }
    cfg_ = ModelConfig();
    cfg_.model_name = "synthetic-" + spec.mix;
    cfg_.vocab_size = spec.vocab; cfg_.hidden_size = spec.hidden; cfg_.intermediate_size = spec.inter;
    cfg_.n_layers = spec.layers; cfg_.n_heads = spec.heads; cfg_.n_kv_heads = spec.kv_heads;
    cfg_.head_dim = spec.hidden / spec.heads;
    cfg_.norm_eps = spec.eps; cfg_.rope_theta = spec.theta;
    cfg_.max_seq_len = std::min(spec.ctx, max_context);
    cfg_.bos_token_id = spec.bos; cfg_.eos_token_id = spec.eos;
    synth_vocab(spec, vocab_.tokens, vocab_.token_types);
    int dev = 0;
    if (const char* e = getenv("NTK_DEVICE")) dev = atoi(e);
    const int st = ntk_device_init(dev);
    if (st != NTK_OK) { err_ = "no usable GPU (HIP device init failed)"; return st; }
    { const int ts = tp_check_shapes(); if (ts != NTK_OK) return ts; }

    size_t biggest = 0;
    for (const auto& t : plan) biggest = std::max(biggest, t.nbytes);
    void* stage = nt_hip_malloc_host(biggest);
    if (!stage) { err_ = "pinned staging allocation failed"; return NTK_E_NOMEM; }
    layers_.resize(cfg_.n_layers);
    int rc = NTK_OK;
    for (const auto& t : plan) {
        synth_fill(stage, t, spec.seed, nthreads);
        DevTensor* dst = nullptr;
        if (t.name == "token_embd.weight") dst = &token_embd_;
        else if (t.name == "output.weight") dst = &output_;
        else if (t.name == "output_norm.weight") dst = &output_norm_;
        else {
            int li = 0;
            char what[64] = {0};
            if (sscanf(t.name.c_str(), "blk.%d.%63s", &li, what) != 2) { rc = NTK_E_FORMAT; break; }
            LayerWeights& L = layers_[li];
            const std::string w = what;
            dst = w == "attn_norm.weight" ? &L.attn_norm : w == "attn_q.weight" ? &L.wq : w == "attn_k.weight" ? &L.wk
                : w == "attn_v.weight" ? &L.wv : w == "attn_output.weight" ? &L.wo : w == "ffn_norm.weight" ? &L.ffn_norm
                : w == "ffn_gate.weight" ? &L.w_gate : w == "ffn_up.weight" ? &L.w_up : &L.w_down;
        }
        Shard how = WHOLE;
        if (t.name.find("attn_q.") != std::string::npos || t.name.find("attn_k.") != std::string::npos || t.name.find("attn_v.") != std::string::npos ||
            t.name.find("ffn_gate.") != std::string::npos || t.name.find("ffn_up.") != std::string::npos) how = ROWS;
        else if (t.name.find("attn_output.") != std::string::npos || t.name.find("ffn_down.") != std::string::npos) how = COLS;
        rc = upload_shard(*dst, stage, ggml_type_to_dtype((uint32_t)t.ggml_type), t.in_f, t.out_f, t.nbytes, how);
        if (rc != NTK_OK) break;
    }
    nt_hip_free_host(stage);
    if (rc == NTK_OK) rc = finish_load(max_context);
    if (rc != NTK_OK) free_all();
    return rc;
}

int Model::share_weights(const Model& src, int max_context) {
    if (&src == this) { err_ = "share_weights: a model cannot share its own weights"; return NTK_E_NULL; }
    free_all();
    if (src.layers_.empty()) { err_ = "share_weights: the source model is not loaded"; return NTK_E_NULL; }
    if (src.tp_world_ != 1 || src.shares_weights_) {
        err_ = "share_weights: the source must hold whole tensors of its own (no tensor parallelism, not itself a sharing sequence)";
        return NTK_E_SHAPE;
    }
    cfg_ = src.cfg_;
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
        void* d = nt_hip_malloc(src.raw_scratch_bytes_);         // into a scratch of THIS sequence (stream ordered on this sequence's stream)
        if (!d) { err_ = "share_weights: no device memory for the unpack scratch"; free_all(); return NTK_E_NOMEM; }
        allocs_.push_back(d);
        raw_scratch_ = d; raw_scratch_bytes_ = src.raw_scratch_bytes_;
        raw_freed_bytes_ = src.raw_freed_bytes_;
    }
    hipStream_t own = nullptr;
    if (hipStreamCreateWithFlags(&own, hipStreamNonBlocking) != hipSuccess) { err_ = "stream creation failed"; free_all(); return NTK_E_LAUNCH; }
    stream_ = own;
    own_stream_ = true;
    const int rc = alloc_buffers();
    if (rc != NTK_OK) free_all();
    return rc;
}

int Model::finish_load(int /*max_context*/) {
    cfg_full_ = cfg_;
    if (tp_world_ > 1) {   // from here on this object IS a model with 1/W of the heads and of the FFN width (hidden size unchanged)
        cfg_.n_heads /= tp_world_;
        cfg_.n_kv_heads /= tp_world_;
        cfg_.intermediate_size /= tp_world_;
        hipStream_t own = nullptr;   // ranks that share a process (tests) must not queue behind each other's waiting kernels
        if (hipStreamCreateWithFlags(&own, hipStreamNonBlocking) != hipSuccess) { err_ = "stream creation failed"; return NTK_E_LAUNCH; }
        stream_ = own;
        own_stream_ = true;
    } else {
        stream_ = ntk_stream(0);
    }
    if (!stream_) { err_ = "no compute stream"; return NTK_E_NODEVICE; }
    NT_TRY(alloc_buffers());
    repack_ = repack_wanted_;   // every load decides anew (a level-3 request that ended as 1 or 2 on the previous model must not stick)
    if (repack_) {
        // ADVICE (round 4): a repack that does not fit must not fail the load -- the raw path decodes every tensor that has no repacked form
        const int st = repack_all();
        if (st == NTK_E_NOMEM) {
            int kept = 0;
            for (auto& L : layers_) for (DevTensor* t : {&L.wq, &L.wk, &L.wv, &L.wo, &L.w_gate, &L.w_up, &L.w_down}) kept += t->rp ? 0 : 1;
            fprintf(stderr, "warning: not enough device memory for the decode repack of every matrix: %d projection tensors stay on the raw-GGUF path\n", kept);
            err_.clear();
        } else if (st != NTK_OK) {
            return st;
        }
        if (repack_ == 3) repack_ = 2;   // round 6: the prompt GEMM reads the repack itself, so the second copy buys the batched paths nothing
        if (repack_ == 2) NT_TRY(drop_raw_all());
    }
    if (persistent_wanted_) set_persistent(persistent_wanted_);
    size_t fr = 0, tot = 0;
    ntk_device_mem_info(&fr, &tot);
    fprintf(stderr, "Model loaded successfully! (resident on MI355X: %.2f GB of weights%s)\nFree VRAM: %.1f GB\n",
            (weight_bytes_ - raw_freed_bytes_) / 1073741824.0, repack_bytes_ ? (" + " + std::to_string(repack_bytes_ / 1073741824.0).substr(0, 5) + " GB repacked for decode").c_str() : "",
            fr / 1073741824.0);
    return NTK_OK;
}

// ---- engine-owned repack of the K-quant projections (csrc/gemv_rp.hip): made once, on the device, from the uploaded GGUF bytes, which
//      stay resident for the 1:1 launchers and the prompt GEMM ----
int Model::repack_one(DevTensor& t) {
    if (t.rp || !t.ptr) return NTK_OK;
    if (t.out_f <= 0 || t.out_f > 0x7FFFFFFF || t.in_f <= 0 || t.in_f > 32768) return NTK_OK;
    const size_t n = ntk_rp_bytes(t.dtype, (int)t.out_f, (int)t.in_f);
    if (n == 0 || n > 0xFFFFFFF0ull) return NTK_OK;   // formats / shapes the matrix-core GEMV does not take keep the raw path
    void* d = nt_hip_malloc(n + 256);
    if (!d) return NTK_E_NOMEM;   // (the caller keeps the tensors that did fit and lets the raw path take the rest)
    allocs_.push_back(d);
    const int st = ntk_rp_pack(d, t.ptr, (int)t.out_f, (int)t.in_f, t.dtype, stream_);
    if (st != NTK_OK) { err_ = std::string("decode repack failed: ") + ntk_status_string(st); return st; }
    t.rp = d;
    t.rp_bytes = n;
    repack_bytes_ += n;
    return NTK_OK;
}

int Model::repack_all() {
    int rc = NTK_OK;
    auto one = [&](DevTensor& t) { const int st = repack_one(t); if (st != NTK_OK && rc == NTK_OK) rc = st; return st; };
    for (auto& L : layers_) {
        if (one(L.wq) == NTK_E_NOMEM) break;
        one(L.wk); one(L.wv); one(L.wo); one(L.w_gate); one(L.w_up); one(L.w_down);
        if (rc == NTK_E_NOMEM) break;
    }
    if (rc != NTK_E_NOMEM) one(output_);
    repack_done_ = true;
    const int sy = ntk_stream_synchronize(stream_);
    return rc != NTK_OK ? rc : sy;
}

// ---- one resident copy (level 2): the uploaded GGUF bytes of every repacked matrix go; raw_of() unpacks on demand ----
int Model::drop_raw_all() {
    size_t need = 0;
    auto grp = [&](std::initializer_list<DevTensor*> ts) {
        size_t g = 0;
        for (DevTensor* t : ts) if (t->rp && !(output_tied_ && t->ptr == token_embd_.ptr)) g += (t->nbytes + 255) / 256 * 256 + 256;
        need = std::max(need, g);
    };
    for (auto& L : layers_) { grp({&L.wq, &L.wk, &L.wv}); grp({&L.wo}); grp({&L.w_gate, &L.w_up}); grp({&L.w_down}); }
    grp({&output_});
    if (need == 0) return NTK_OK;
    if (!raw_scratch_ || raw_scratch_bytes_ < need) {
        void* d = nt_hip_malloc(need);
        if (!d) { fprintf(stderr, "warning: no device memory for the unpack scratch: the GGUF bytes stay resident beside the repack\n"); repack_ = 1; return NTK_OK; }
        allocs_.push_back(d);
        raw_scratch_ = d; raw_scratch_bytes_ = need;
    }
    auto drop = [&](DevTensor& t) {
        if (!t.rp || !t.ptr || (output_tied_ && t.ptr == token_embd_.ptr)) return;
        auto it = std::find(allocs_.begin(), allocs_.end(), t.ptr);
        if (it != allocs_.end()) allocs_.erase(it);
        nt_hip_free(t.ptr);
        t.ptr = nullptr;
        raw_freed_bytes_ += t.nbytes;
    };
    NT_TRY(ntk_stream_synchronize(stream_));
    for (auto& L : layers_) { drop(L.wq); drop(L.wk); drop(L.wv); drop(L.wo); drop(L.w_gate); drop(L.w_up); drop(L.w_down); }
    drop(output_);
    return NTK_OK;
}

int Model::restore_raw_all() {
    int rc = NTK_OK;
    auto back = [&](DevTensor& t) {
        if (t.ptr || !t.rp || rc != NTK_OK) return;
        void* d = nt_hip_malloc((t.nbytes + 255) / 256 * 256 + 256);
        if (!d) { rc = NTK_E_NOMEM; return; }
        const int st = ntk_rp_unpack(d, t.rp, (int)t.out_f, (int)t.in_f, t.dtype, stream_);
        if (st != NTK_OK) { nt_hip_free(d); rc = st; return; }
        allocs_.push_back(d);
        t.ptr = d;
        raw_freed_bytes_ -= t.nbytes;
    };
    for (auto& L : layers_) { back(L.wq); back(L.wk); back(L.wv); back(L.wo); back(L.w_gate); back(L.w_up); back(L.w_down); }
    back(output_);
    const int sy = ntk_stream_synchronize(stream_);
    return rc != NTK_OK ? rc : sy;
}

const void* Model::raw_of(const DevTensor& t) {
    if (t.ptr) return t.ptr;
    if (!t.rp || !raw_scratch_) { raw_err_ = NTK_E_NULL; return nullptr; }
    const size_t n = (t.nbytes + 255) / 256 * 256 + 256;
    if (raw_cursor_ + n > raw_scratch_bytes_) {   // a group never exceeds the scratch (sized for the largest in drop_raw_all): wrapping would overwrite a tensor the same launch still reads
        if (!raw_err_) raw_err_ = NTK_E_NOMEM;
        return nullptr;
    }
    void* d = static_cast<uint8_t*>(raw_scratch_) + raw_cursor_;
    raw_cursor_ += n;
    const int st = ntk_rp_unpack(d, t.rp, (int)t.out_f, (int)t.in_f, t.dtype, stream_);
    if (st != NTK_OK) { raw_err_ = st; return nullptr; }
    return d;
}

int Model::set_attention_merge(bool on) {
    if (on == attn_merge_) return NTK_OK;
    if (!layers_.empty()) {
        NT_TRY(sync());
        for (auto& row : graphs_) for (auto& gx : row) { if (gx) (void)hipGraphExecDestroy(reinterpret_cast<hipGraphExec_t>(gx)); gx = nullptr; }
    }
    attn_merge_ = on;
    return NTK_OK;
}

int Model::set_repack(int level) {
    level = level < 0 ? 0 : level > 3 ? 3 : level;
    if (shares_weights_) { err_ = "set_repack: this sequence shares another model's tensors"; return NTK_E_SHAPE; }
    repack_wanted_ = level;
    if (layers_.empty()) { repack_ = level; return NTK_OK; }   // before the load: finish_load() decides
    if (level == 3) level = 2;   // (round 6: one resident copy; what is gone stays gone)
    if (level == repack_) return NTK_OK;
    NT_TRY(sync());
    for (auto& row : graphs_) for (auto& gx : row) { if (gx) (void)hipGraphExecDestroy(reinterpret_cast<hipGraphExec_t>(gx)); gx = nullptr; }
    int rc = NTK_OK;
    if (level < 2 && raw_freed_bytes_ > 0) rc = restore_raw_all();           // the GGUF bytes come back first (levels 0 and 1 read them)
    if (rc == NTK_OK && level > 0 && !repack_done_) {
        rc = repack_all();
        if (rc == NTK_E_NOMEM) { fprintf(stderr, "warning: decode repack incomplete (device memory): the rest stays on the raw path\n"); rc = NTK_OK; err_.clear(); }
    }
    if (rc != NTK_OK) { err_ = std::string("set_repack: ") + ntk_status_string(rc); return rc; }
    repack_ = level;
    if (level == 2) {
#ifdef NTK_EXPERIMENTS
        // the persistent kernels stream the uploaded GGUF bytes through the pointers their plan recorded: a plan must not outlive them
        if (persistent_plan_) {
            for (auto& row : graphs_) { if (row[kPersistentSlot]) (void)hipGraphExecDestroy(reinterpret_cast<hipGraphExec_t>(row[kPersistentSlot])); row[kPersistentSlot] = nullptr; }
            if (persistent_kind_ == 2) ntk_layer_engine_plan_destroy(persistent_plan_); else ntk_persistent_plan_destroy(persistent_plan_);
            persistent_plan_ = nullptr;
        }
#endif
        persistent_on_ = false;
        rc = drop_raw_all();
    }
    return rc;
}

int Model::alloc_buffers() {   // transformer.cpp:330-391
    const size_t S = (size_t)cfg_.max_seq_len, H = (size_t)cfg_.hidden_size, L = (size_t)cfg_.n_layers;
    const size_t per = (size_t)cfg_.n_kv_heads * cfg_.head_dim;
    auto dev = [&](size_t bytes, bool zero) -> void* {
        void* p = nt_hip_malloc(bytes + 256);
        if (p) { allocs_.push_back(p); if (zero) nt_hip_memset(p, 0, bytes); }
        return p;
    };
    // the attention kernels address a layer's cache rows with 32-bit byte offsets (attention.hip): a context whose per-layer cache reaches
    // 3.75 GiB is refused here, at load, rather than as NTK_E_SHAPE from the first decode step (8 KV heads of 128: 1.9 M positions)
    if (S * per * sizeof(uint16_t) >= 0xF0000000ull) { err_ = "context too long: one layer's K cache must stay below 3.75 GiB (32-bit row offsets)"; return NTK_E_SHAPE; }
    const size_t kvb = L * S * per * sizeof(uint16_t);
    if (kv_q8_) {   // the 8-bit cache (csrc/attention_q8.hip) + ONE layer's F16 image for the prompt path
        if (cfg_.head_dim != 128 || cfg_.n_kv_heads <= 0 || cfg_.n_heads % cfg_.n_kv_heads != 0 || cfg_.n_heads / cfg_.n_kv_heads > 16) {
            err_ = "kv_cache=q8_0 needs head_dim 128 and at most 16 query heads per KV head (this model: head_dim " + std::to_string(cfg_.head_dim) +
                   ", " + std::to_string(cfg_.n_kv_heads > 0 ? cfg_.n_heads / cfg_.n_kv_heads : 0) + " query heads per KV head)";
            return NTK_E_SHAPE;
        }
        if (tp_world_ > 1) { err_ = "kv_cache=q8_0 is not supported with tensor parallelism"; return NTK_E_SHAPE; }
        if (fuse_attention_) { err_ = "kv_cache=q8_0 is not supported with the attention-inside-Wo launch (fuse_attention)"; return NTK_E_SHAPE; }
        kv_q8_layer_bytes_ = ntk_kv_q8_cache_bytes((int)S, cfg_.n_kv_heads, cfg_.head_dim);
        k_cache_q8_ = (uint8_t*)dev(L * kv_q8_layer_bytes_, true);
        v_cache_q8_ = (uint8_t*)dev(L * kv_q8_layer_bytes_, true);
        kv_f16_k_ = (uint16_t*)dev(S * per * sizeof(uint16_t), true);
        kv_f16_v_ = (uint16_t*)dev(S * per * sizeof(uint16_t), true);
        if (!k_cache_q8_ || !v_cache_q8_ || !kv_f16_k_ || !kv_f16_v_) { err_ = "buffer allocation failed (8-bit KV cache)"; return NTK_E_NOMEM; }
        kv_cache_bytes_ = 2ull * L * kv_q8_layer_bytes_ + 2ull * S * per * sizeof(uint16_t);
    } else {
        k_cache_ = (uint16_t*)dev(kvb, true);
        v_cache_ = (uint16_t*)dev(kvb, true);
        kv_cache_bytes_ = 2ull * kvb;
    }
    hidden_ = (float*)dev(std::max<size_t>(S, 2) * H * 4, false);
    residual_ = (float*)dev(std::max<size_t>(S, 2) * H * 4, false);
    logits_ = (float*)dev((size_t)cfg_.vocab_size * 4, false);
    const size_t attn_ws = S * (size_t)(2 * cfg_.n_heads + 2 * cfg_.n_kv_heads) * cfg_.head_dim;
    const size_t ffn_ws = 2 * S * (size_t)cfg_.intermediate_size;
    workspace_floats_ = std::max(attn_ws, ffn_ws);
    workspace_ = (float*)dev(workspace_floats_ * 4, false);
    positions_ = (int*)dev(S * 4, false);
    tokens_dev_ = (int*)dev(S * 4, false);
    d_pos_ = (int*)dev(64, true);
    d_token_ = (int*)dev(64, true);
    argmax_scratch_ = (float*)dev(2 * 1024 * 4, false);
    rope_inv_freq_ = (float*)dev((size_t)cfg_.head_dim / 2 * 4 + 64, false);
    row_max_ = (float*)dev((size_t)S * 2 * 4, true);
    attn_scratch_ = (float*)dev(ntk_attention_split_scratch_bytes(cfg_.n_heads, cfg_.head_dim, kMaxAttnSplits), true);   // (zeroed: the arrival counters in front)
    h_token_ = (int*)nt_hip_malloc_host(64);
    h_ring_ = (unsigned long long*)nt_hip_malloc_host(64);
    if (h_ring_) memset(h_ring_, 0, 64);
    sample_scratch_ = dev(ntk_sample_scratch_bytes(cfg_.vocab_size), false);
    attn_sync_ = (unsigned*)dev(4096, true);
    {   // one workspace for every projection: the largest need over the launches the prompt pass makes (Q|K|V and gate|up go out as one)
        const int H = cfg_.hidden_size, I = cfg_.intermediate_size, qkv = (cfg_.n_heads + 2 * cfg_.n_kv_heads) * cfg_.head_dim;
        const int shapes[][2] = {{H, qkv}, {H, cfg_.n_heads * cfg_.head_dim}, {H, cfg_.n_kv_heads * cfg_.head_dim}, {cfg_.n_heads * cfg_.head_dim, H},
                                 {H, 2 * I}, {H, I}, {I, H}};
        gemm_ws_bytes_ = 0;
        for (const auto& sh : shapes) gemm_ws_bytes_ = std::max(gemm_ws_bytes_, ntk_gemm_quant_workspace_bytes(sh[0], sh[1]));
    }
    gemm_ws_ = dev(gemm_ws_bytes_, false);
    gemm_ws2_ = dev(gemm_ws_bytes_, false);
    if (tp_world_ > 1) {   // communication buffer: flags + two slots of one prompt's worth of hidden vectors
        tp_max_floats_ = S * H;
        tp_comm_ = ntk_tp_comm_alloc(ntk_tp_comm_bytes(tp_max_floats_));   // fine-grained: csrc/tp.hip
        if (tp_comm_) allocs_.push_back(tp_comm_);
        if (!tp_comm_ || ntk_tp_comm_reset(tp_comm_, nullptr) != NTK_OK || ntk_device_synchronize() != NTK_OK) { err_ = "communication buffer allocation failed"; return NTK_E_NOMEM; }
    }
    d_recent_ = (int*)dev(kRecentCap * 4, false);
    h_recent_ = (int*)nt_hip_malloc_host(kRecentCap * 4);
    if ((!kv_q8_ && (!k_cache_ || !v_cache_)) || !hidden_ || !residual_ || !logits_ || !workspace_ || !positions_ || !tokens_dev_ ||
        !d_pos_ || !d_token_ || !argmax_scratch_ || !h_token_ || !h_ring_) {
        err_ = "buffer allocation failed";
        return NTK_E_NOMEM;
    }
    *h_token_ = 0;
    if (rope_inv_freq_) {
        std::vector<float> f((size_t)cfg_.head_dim / 2);
        for (int i = 0; i < cfg_.head_dim / 2; ++i) f[i] = 1.0f / powf(cfg_.rope_theta, (2.0f * i) / cfg_.head_dim);
        nt_hip_memcpy_h2d(rope_inv_freq_, f.data(), f.size() * 4);
    }
    return NTK_OK;
}

uint64_t Model::bytes_per_token(int pos) const {
    uint64_t b = 0;
    for (const auto& L : layers_)
        b += L.wq.nbytes + L.wk.nbytes + L.wv.nbytes + L.wo.nbytes + L.w_gate.nbytes + L.w_up.nbytes + L.w_down.nbytes;
    b += output_.nbytes;
    b += (uint64_t)(2 * cfg_.n_layers + 1) * cfg_.hidden_size * 4;
    const uint64_t kv_elems = (uint64_t)cfg_.n_kv_heads * cfg_.head_dim;
    const uint64_t kv_row = kv_q8_ ? kv_elems + kv_elems / 16 : kv_elems * 2;   // q8_0: an int8 per element + a half per 32
    b += 2ull * cfg_.n_layers * kv_row * (uint64_t)(pos + 1) + 2ull * cfg_.n_layers * kv_row;
    b += ntk_row_bytes(token_embd_.dtype, cfg_.hidden_size);
    return b;
}

// ---------------------------------------------------------------------------------------------------
// 1:1 path: the reference's own launcher sequence (transformer.cpp:604-669, attention.cpp:120-211,
// ffn.cpp:85-134), through the same C ABI an external caller would use
// ---------------------------------------------------------------------------------------------------
float* Model::forward(const int* tokens, int T, int start_pos) {
    if (T <= 0 || start_pos < 0 || start_pos + T > cfg_.max_seq_len) { err_ = "forward: sequence exceeds context"; return nullptr; }
    for (int i = 0; i < T; ++i)   // the embedding gather indexes the table with these on the device
        if (tokens[i] < 0 || tokens[i] >= cfg_.vocab_size) { err_ = "forward: token id out of range"; return nullptr; }
    const int H = cfg_.hidden_size, I = cfg_.intermediate_size, hd = cfg_.head_dim, nh = cfg_.n_heads, nkv = cfg_.n_kv_heads;
    const int qd = nh * hd, kvd = nkv * hd;
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

    int rc = layers_1to1(T, start_pos, 0, cfg_.n_layers);
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

// layers [first, last) of the 1:1 path on hidden_[T][H] at positions start_pos.. (positions_ already on the device)
int Model::layers_1to1(int T, int start_pos, int first, int last_layer) {
    const int H = cfg_.hidden_size, I = cfg_.intermediate_size, hd = cfg_.head_dim, nh = cfg_.n_heads, nkv = cfg_.n_kv_heads;
    const int qd = nh * hd, kvd = nkv * hd;
    void* s = stream_;
    const size_t kv_layer = (size_t)cfg_.max_seq_len * kvd;
    const float scale = 1.0f / sqrtf((float)hd);
    float* q_buf = workspace_;
    float* k_buf = q_buf + (size_t)T * qd;
    float* v_buf = k_buf + (size_t)T * kvd;
    float* attn_out = v_buf + (size_t)T * kvd;
    float* gate_buf = workspace_;
    float* up_buf = gate_buf + (size_t)T * I;
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
    auto f16_ok = [&](const DevTensor& w) {   // the formats and shapes ntk_gemm_quant_f16 takes
        const bool kq = w.dtype == NTK_DT_Q4_0 || w.dtype == NTK_DT_Q4_K || w.dtype == NTK_DT_Q5_K || w.dtype == NTK_DT_Q6_K;
        return (w.dtype == NTK_DT_Q8_0 || kq) && w.in_f % (kq ? 256 : 128) == 0 && w.out_f % 16 == 0 && (w.ptr || w.rp);
    };
    // The form the producer of X takes when X (`width` columns) feeds matrix next_w: it splits X into next_w's planes itself, leaves the tokens' maxima, or
    // neither.  The split: up to 64 tokens (a producer that owns a whole token per workgroup writes its planes in 16-byte pieces a kilobyte apart:
    // faster than the GEMM's own pre-pass at 16 - 64 tokens, slower at 1024), and not under tensor parallelism, where a rank's SiLU launch keeps its maxima
    // in the array that only ntk_rmsnorm_rowmax zeroes.
    enum class XForm { plain, row_max, split };
    auto x_form = [&](int width, const DevTensor& next_w) {
        if (with_max && prefill_fused_split_ && gemm_ws2_ != nullptr && T <= 64 && tp_world_ == 1 && f16_ok(next_w) && (int)next_w.in_f == width) return XForm::split;
        return with_max ? XForm::row_max : XForm::plain;
    };
    // a K-quant matrix whose GGUF bytes were freed after the load-time repack (one resident copy): the FP16 GEMM reads it FROM THE REPACK
    // (ntk_gemm_desc.weights_repacked: identical bits) -- no unpack in front of the prompt launches
    auto rp_only = [&](const DevTensor& w) {
        return !w.ptr && w.rp && (w.dtype == NTK_DT_Q4_K || w.dtype == NTK_DT_Q5_K || w.dtype == NTK_DT_Q6_K) && w.out_f % 16 == 0;
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
    auto gemm_one = [&](float* Y, const DevTensor& w, const float* X, const float* resid, const float* rm, ntk_gemm_partials* pt, const void* const* raw) {
        const DevTensor* const wp = &w;
        return gemm_group(&Y, &wp, 1, X, resid, rm, pt, raw);
    };
    auto project = [&](float* Y, const DevTensor& w, const float* X, size_t ystride, size_t xstride, const float* rm) {
        const bool dense = ystride == (size_t)w.out_f && xstride == (size_t)w.in_f;
        if (batched && bf16_now && rp_only(w) && dense) {   // straight from the repack
            const int st = gemm_one(Y, w, X, nullptr, rm, nullptr, nullptr);
            if (!not_taken(st)) { ok(st); return; }
        }
        raw_begin();
        const void* wp = raw_of(w);
        if (batched && is_quant(w.dtype) && dense) {
            int st = bf16_now ? gemm_one(Y, w, X, nullptr, rm, nullptr, &wp) : NTK_E_DTYPE;   // FP16 matrix cores, up to 1024 tokens per pass
            if (not_taken(st)) st = ntk_gemm_quant(Y, wp, X, T, (int)w.out_f, (int)w.in_f, w.dtype, nullptr, s);
            if (st != NTK_E_ALIGN && st != NTK_E_SHAPE) { ok(st); return; }   // those two: shapes only the per-token loop takes
        }
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
        if (dense && bf16_now && rp_only(w)) {   // straight from the repack
            const int st = gemm_one(hidden_, w, X, hidden_, rm, nullptr, nullptr);
            if (!not_taken(st)) { ok(st); return; }
        }
        if (dense && is_quant(w.dtype)) {
            raw_begin();
            const void* wp = raw_of(w);
            int st = bf16_now ? gemm_one(hidden_, w, X, hidden_, rm, nullptr, &wp) : NTK_E_DTYPE;
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
        int st = rp_only(w) ? gemm_one(hidden_, w, X, hidden_, rm, &pt, nullptr) : NTK_E_DTYPE;   // straight from the repack
        if (not_taken(st)) {
            raw_begin();
            const void* wp = raw_of(w);
            st = gemm_one(hidden_, w, X, hidden_, rm, &pt, &wp);
        }
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
        float* const ys[2] = {gate_buf, up_buf};
        const DevTensor* const ws[2] = {&L.w_gate, &L.w_up};
        ntk_gemm_partials pt;
        int st = gemm_group(ys, ws, 2, residual_, nullptr, rm_a, &pt, nullptr);
        if (not_taken(st)) return false;
        const bool split = st == NTK_OK && x_form(I, L.w_down) == XForm::split;
        if (split) st = ntk_reduce_silu_mul_prepare_x(gate_buf, &pt, planes.other(), s);
        else if (st == NTK_OK) st = ntk_reduce_silu_mul_rowmax(gate_buf, &pt, rm_b, s);
        planes.written(gate_buf, split);
        ok(st);
        return true;
    };
    // gate_buf = SiLU(gate_buf) x up_buf in the form the down projection asks for
    auto silu_mul = [&](const DevTensor& next_w) {
        const XForm f = x_form(I, next_w);
        int st = NTK_E_SHAPE;
        if (f == XForm::split) st = ntk_silu_mul_prepare_x(gate_buf, gate_buf, up_buf, T, I, planes.other(), s);
        else if (f == XForm::row_max && rm_b) st = ntk_silu_mul_rowmax(gate_buf, gate_buf, up_buf, T, I, rm_b, s);
        planes.written(gate_buf, f == XForm::split && st == NTK_OK);
        if (st == NTK_E_SHAPE || st == NTK_E_ALIGN) { st = ntk_silu_mul(gate_buf, gate_buf, up_buf, T * I, s); rm_b = nullptr; }   // (then for the rest of the pass)
        ok(st);
    };
    bool normed_ahead = false;   // residual_ (with its maxima or planes) already holds this layer's normalised input, written with the previous layer's down projection
    for (int i = first; i < last_layer; ++i) {
        const LayerWeights& L = layers_[i];
        uint16_t* kc = kv_q8_ ? nullptr : k_cache_ + (size_t)i * kv_layer;   // (q8_0: the one-layer F16 image, set below)
        uint16_t* vc = kv_q8_ ? nullptr : v_cache_ + (size_t)i * kv_layer;
        if (!normed_ahead) norm(L.attn_norm, true, L.wq);
        normed_ahead = false;
        {
            float* const ys[3] = {q_buf, k_buf, v_buf};
            const DevTensor* const ws[3] = {&L.wq, &L.wk, &L.wv};
            project_many(ys, ws, 3, residual_, rm_a);
        }
        if (i == kv_capture_layer_ && kv_capture_) {   // parity instrumentation: the F32 projections the store launches are about to read
            ok(ntk_copy(kv_capture_, k_buf, T * kvd, s));
            ok(ntk_copy(kv_capture_ + (size_t)cfg_.max_seq_len * kvd, v_buf, T * kvd, s));
            kv_capture_T_ = T;
        }
        if (kv_q8_) {   // 8-bit store, then rows [0, start_pos + T) rounded to half into the one-layer scratch the unchanged F16 kernels read
            uint8_t* kc8 = k_cache_q8_ + (size_t)i * kv_q8_layer_bytes_;
            uint8_t* vc8 = v_cache_q8_ + (size_t)i * kv_q8_layer_bytes_;
            if (T >= 4) {
                ok(ntk_rope_kv_store_q8(q_buf, k_buf, v_buf, positions_, T, nh, nkv, hd, cfg_.rope_theta, cfg_.rope_freq_scale, cfg_.rope_interleaved,
                                        kc8, vc8, start_pos, cfg_.max_seq_len, s));
            } else {
                ok(ntk_rope(q_buf, k_buf, positions_, 1, T, nh, nkv, hd, cfg_.rope_theta, cfg_.rope_freq_scale, cfg_.rope_interleaved, s));
                ok(ntk_kv_store_q8(kc8, vc8, k_buf, v_buf, T, nkv, hd, start_pos, cfg_.max_seq_len, s));
            }
            ok(ntk_kv_dequant_q8_f16(kv_f16_k_, kv_f16_v_, kc8, vc8, start_pos + T, nkv, hd, cfg_.max_seq_len, s));
            kc = kv_f16_k_; vc = kv_f16_v_;
        } else if (with_max && T >= 4 && hd <= 256) {   // (the prompt form of the rotation: ntk_rope takes it from 4 tokens on, too)
            ok(ntk_rope_kv_store(q_buf, k_buf, v_buf, positions_, T, nh, nkv, hd, cfg_.rope_theta, cfg_.rope_freq_scale, cfg_.rope_interleaved, kc, vc,
                                 start_pos, cfg_.max_seq_len, s));
        } else {
            ok(ntk_rope(q_buf, k_buf, positions_, 1, T, nh, nkv, hd, cfg_.rope_theta, cfg_.rope_freq_scale, cfg_.rope_interleaved, s));
            ok(ntk_copy_to_kv_cache(kc, vc, k_buf, v_buf, T, nkv, hd, start_pos, cfg_.max_seq_len, s));
        }
        if (T == 1) ok(ntk_attention_decode(attn_out, q_buf, kc, vc, start_pos + T, nh, nkv, hd, cfg_.max_seq_len, scale, s));
        else ok(ntk_attention_prefill(attn_out, q_buf, kc, vc, T, start_pos, nh, nkv, hd, cfg_.max_seq_len, scale, s));
        if (!project_add_norm(L.wo, attn_out, nullptr, L.ffn_norm, false, L.w_gate)) {
            project_add(L.wo, attn_out, qd, nullptr);
            norm(L.ffn_norm, false, L.w_gate);
        }
        if (!gate_up_silu(L)) {
            float* const ys[2] = {gate_buf, up_buf};
            const DevTensor* const ws[2] = {&L.w_gate, &L.w_up};
            project_many(ys, ws, 2, residual_, rm_a);
            silu_mul(L.w_down);
        }
        // down projection + residual, and the NEXT layer's first RMSNorm in the same consumer launch when there is a next layer in this pass
        if (i + 1 < last_layer && project_add_norm(L.w_down, gate_buf, rm_b, layers_[i + 1].attn_norm, true, layers_[i + 1].wq)) normed_ahead = true;
        else project_add(L.w_down, gate_buf, I, rm_b);
        if (rc != NTK_OK) break;
    }
    if (raw_err_ != NTK_OK) { rc = raw_err_; raw_err_ = NTK_OK; }   // what raw_of() could not report through its pointer (it precedes the consumer's NTK_E_NULL)
    return rc;
}

// ---------------------------------------------------------------------------------------------------
// fused single-token path
// ---------------------------------------------------------------------------------------------------
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

// which launch kinds read the repacked tensors: 1 Q|K|V, 2 Wo, 4 gate|up, 8 down, 16 LM head (tuning builds: NTK_RP_MASK)
static int rp_mask() {
#ifdef NTK_TUNE
    static const int m = [] { const char* e = getenv("NTK_RP_MASK"); return e ? atoi(e) : 31; }();
    return m;
#else
    return 31;
#endif
}

int Model::enqueue_token(bool greedy) {
    const int H = cfg_.hidden_size;
    void* s = stream_;
    tp_call_ = 0;
    prof_mark(2, true);
    const int est = ntk_embed_rows(hidden_, token_embd_.ptr, d_token_, 1, H, token_embd_.dtype, s);
    prof_mark(2, false);
    if (est != NTK_OK && est != NTK_E_DTYPE) return est;
#ifdef NTK_EXPERIMENTS
    if (use_persistent_now()) {   // every layer and the LM head in one launch
        NT_TRY(persistent_kind_ == 2 ? ntk_layer_engine_launch(persistent_plan_, d_pos_, s) : ntk_persistent_launch(persistent_plan_, d_pos_, s));
        if (greedy) NT_TRY(ntk_argmax_advance(logits_, cfg_.vocab_size, d_token_, h_token_, h_ring_, d_pos_, argmax_scratch_, s));
        else NT_TRY(ntk_advance_pos(d_pos_, s));
        return NTK_OK;
    }
#endif
    NT_TRY(enqueue_layers(0, cfg_.n_layers));
    // final RMSNorm + LM head (one launch for a quantised output matrix), then the token's tail
    {
        const DevTensor& w = output_;
        if (is_quant(w.dtype)) {
            prof_mark(0, true);
            int st = NTK_E_DTYPE;
            if (repack_ && w.rp && (rp_mask() & 16)) {
                ntk_gemv_seg rs = {w.rp, logits_, (int)w.out_f, w.dtype};
                st = ntk_gemv_rp_fused(&rs, 1, hidden_, (int)w.in_f, (const float*)output_norm_.ptr, cfg_.norm_eps, nullptr, 0, s);
                if (st != NTK_OK && !not_taken(st)) return st;
            }
            if (st != NTK_OK) {
                raw_begin();
                ntk_gemv_seg seg = {raw_of(w), logits_, (int)w.out_f, w.dtype};
                NT_TRY(ntk_gemv_fused(&seg, 1, hidden_, (int)w.in_f, (const float*)output_norm_.ptr, cfg_.norm_eps, nullptr, 0, s));
            }
            prof_mark(0, false);
        } else {
            NT_TRY(ntk_rmsnorm(residual_ + H, hidden_, (const float*)output_norm_.ptr, 1, (int)w.in_f, cfg_.norm_eps, s));
            NT_TRY(ntk_gemv(logits_, w.ptr, residual_ + H, (int)w.out_f, (int)w.in_f, w.dtype, s));
        }
    }
    prof_mark(2, true);
    // greedy: arg-max, token -> device word + pinned ring, position + 1 in ONE tail (ntk_argmax_advance); otherwise only the position
    if (greedy) NT_TRY(ntk_argmax_advance(logits_, cfg_.vocab_size, d_token_, h_token_, h_ring_, d_pos_, argmax_scratch_, s));
    else NT_TRY(ntk_advance_pos(d_pos_, s));
    if (tp_world_ > 1) NT_TRY(ntk_tp_advance_epoch(tp_comm_, s));
    prof_mark(2, false);
    return NTK_OK;
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

// layers [first, last) of the fused single-token path on hidden_[H] (position in *d_pos_)
int Model::enqueue_layers(int first, int last_layer) {
    const int H = cfg_.hidden_size, I = cfg_.intermediate_size, hd = cfg_.head_dim, nh = cfg_.n_heads, nkv = cfg_.n_kv_heads;
    const int qd = nh * hd, kvd = nkv * hd;
    void* s = stream_;
    auto mark = [&](int cls, bool begin) { prof_mark(cls, begin); };
    const float scale = 1.0f / sqrtf((float)hd);
    const size_t kv_layer = (size_t)cfg_.max_seq_len * kvd;
    float* q_buf = workspace_;
    float* k_buf = q_buf + qd;
    float* v_buf = k_buf + kvd;
    float* attn_out = v_buf + kvd;
    float* gate_buf = workspace_;
    float* up_buf = gate_buf + I;

    // y_k = W_k . f(x) for n <= 3 matrices sharing x.  Matrices with one quantised dtype go out as one fused
    // launch (RMSNorm prologue when `norm`, residual epilogue when `resid`, n == 1); dense F16/F32 tensors take
    // the 1:1 launchers.  Scratch: residual_[0,H) = dense output before the residual add, residual_[H,2H) = norm(x).
    auto project = [&](const DevTensor* const* ws, float* const* ys, int n, const float* x, const DevTensor* norm,
                       const float* resid, int kind) -> int {
        const float* nw = norm ? (const float*)norm->ptr : nullptr;
        bool done[3] = {false, false, false};
        if (repack_ && (rp_mask() & kind)) {   // every matrix has its repacked form: one launch of the matrix-core GEMV, whatever the mix of K-quant formats
            bool all = true;
            for (int a = 0; a < n; ++a) all = all && ws[a]->rp != nullptr && ws[a]->in_f == ws[0]->in_f;
            if (all) {
                ntk_gemv_seg segs[3];
                for (int a = 0; a < n; ++a) segs[a] = {ws[a]->rp, ys[a], (int)ws[a]->out_f, ws[a]->dtype};
                mark(0, true);
                const int st = ntk_gemv_rp_fused(segs, n, x, (int)ws[0]->in_f, nw, cfg_.norm_eps, resid, 0, s);
                mark(0, false);
                if (st == NTK_OK) return NTK_OK;
                if (!not_taken(st)) return st;   // (those: the raw-GGUF launches below take over)
            }
        }
        if (n > 1 && !resid) {   // matrices in two K-quant formats (Q4_K_M's attn_v): still one launch when the library has the pair
            bool all_quant = true, mixed = false;
            for (int a = 0; a < n; ++a) { all_quant = all_quant && is_quant(ws[a]->dtype); mixed = mixed || ws[a]->dtype != ws[0]->dtype; }
            if (all_quant && mixed) {
                ntk_gemv_seg segs[3];
                raw_begin();
                for (int a = 0; a < n; ++a) segs[a] = {raw_of(*ws[a]), ys[a], (int)ws[a]->out_f, ws[a]->dtype};
                mark(0, true);
                const int st = ntk_gemv_fused(segs, n, x, (int)ws[0]->in_f, nw, cfg_.norm_eps, nullptr, 0, s);
                mark(0, false);
                if (st == NTK_OK) return NTK_OK;
                // formats / alignment / workgroup split / LDS size the optional one-launch form does not take: the per-format
                // launches below do (the pair kernel is an optimisation, never the only way)
                if (!not_taken(st)) return st;
            }
        }
        for (int a = 0; a < n; ++a) {
            if (done[a]) continue;
            const DevTensor& w = *ws[a];
            if (!is_quant(w.dtype)) {
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
                continue;
            }
            ntk_gemv_seg segs[3];
            int m = 0;
            raw_begin();
            for (int b = a; b < n; ++b) {
                if (done[b] || ws[b]->dtype != w.dtype) continue;
                segs[m++] = {raw_of(*ws[b]), ys[b], (int)ws[b]->out_f, ws[b]->dtype};
                done[b] = true;
            }
            mark(0, true);
            NT_TRY(ntk_gemv_fused(segs, m, x, (int)w.in_f, nw, cfg_.norm_eps, resid, 0, s));
            mark(0, false);
        }
        return NTK_OK;
    };
    auto project1 = [&](const DevTensor& w, float* y, const float* x, const DevTensor* norm, const float* resid, int kind) -> int {
        const DevTensor* ws[1] = {&w};
        float* ys[1] = {y};
        return project(ws, ys, 1, x, norm, resid, kind);
    };

    for (int i = first; i < last_layer; ++i) {
        const LayerWeights& L = layers_[i];
        uint16_t* kc = kv_q8_ ? nullptr : k_cache_ + (size_t)i * kv_layer;   // (q8_0: the launch below takes the 8-bit caches)
        uint16_t* vc = kv_q8_ ? nullptr : v_cache_ + (size_t)i * kv_layer;
        {
            const DevTensor* ws[3] = {&L.wq, &L.wk, &L.wv};
            float* ys[3] = {q_buf, k_buf, v_buf};
            NT_TRY(project(ws, ys, 3, hidden_, &L.attn_norm, nullptr, 1));
        }
#ifdef NTK_EXPERIMENTS
        if (attn_regime_ == 0 && fuse_attention_ && !kv_q8_ && attn_sync_ && is_quant(L.wo.dtype) && tp_world_ == 1) {
            // attention producers inside the Wo launch: one launch, one boundary and one first-byte latency less per layer
            raw_begin();
            ntk_gemv_seg wo = {raw_of(L.wo), hidden_, (int)L.wo.out_f, L.wo.dtype};
            mark(0, true);
            const int st = ntk_attention_gemv_fused(attn_out, q_buf, k_buf, v_buf, kc, vc, d_pos_, rope_inv_freq_, nh, nkv, hd,
                                                    cfg_.max_seq_len, scale, cfg_.rope_theta, cfg_.rope_freq_scale, &wo, hidden_,
                                                    attn_sync_, s);
            mark(0, false);
            if (st == NTK_OK) goto ffn;
            if (!not_taken(st)) return st;   // those: shapes only the two launches take
        }
#endif
        mark(1, true);
        if (kv_q8_)
            NT_TRY(ntk_attention_decode_q8(attn_out, q_buf, k_buf, v_buf, k_cache_q8_ + (size_t)i * kv_q8_layer_bytes_,
                                           v_cache_q8_ + (size_t)i * kv_q8_layer_bytes_, d_pos_, rope_inv_freq_, nh, nkv, hd, cfg_.max_seq_len, scale,
                                           cfg_.rope_theta, cfg_.rope_freq_scale, kv_q8_splits(attn_regime_), attn_scratch_, s));
        else if (attn_regime_ == 0)
            NT_TRY(ntk_attention_decode_fused(attn_out, q_buf, k_buf, v_buf, kc, vc, d_pos_, rope_inv_freq_, nh, nkv, hd,
                                              cfg_.max_seq_len, scale, cfg_.rope_theta, cfg_.rope_freq_scale, s));
        else
            NT_TRY((attn_merge_ ? ntk_attention_decode_split_merged : ntk_attention_decode_split)(
                attn_out, q_buf, k_buf, v_buf, kc, vc, d_pos_, rope_inv_freq_, nh, nkv, hd, cfg_.max_seq_len, scale, cfg_.rope_theta,
                cfg_.rope_freq_scale, attention_splits(attn_regime_, hd), attn_scratch_, s));
        mark(1, false);
        if (tp_world_ > 1) {   // partial sum over this rank's heads -> exchange slot -> hidden += sum over ranks
            NT_TRY(project1(L.wo, tp_slot(), attn_out, nullptr, nullptr, 2));
            NT_TRY(tp_allreduce(hidden_, H));
        } else {
            NT_TRY(project1(L.wo, hidden_, attn_out, nullptr, hidden_, 2));
        }
#ifdef NTK_EXPERIMENTS
    ffn:
#endif
        if (is_quant(L.w_gate.dtype) && L.w_gate.dtype == L.w_up.dtype) {
            mark(0, true);
            int st = NTK_E_DTYPE;
            if (repack_ && L.w_gate.rp && L.w_up.rp && (rp_mask() & 4)) {
                ntk_gemv_seg rs[2] = {{L.w_gate.rp, gate_buf, I, L.w_gate.dtype}, {L.w_up.rp, up_buf, I, L.w_up.dtype}};
                st = ntk_gemv_rp_fused(rs, 2, hidden_, H, (const float*)L.ffn_norm.ptr, cfg_.norm_eps, nullptr, 1, s);
                if (st != NTK_OK && !not_taken(st)) return st;
            }
            if (st != NTK_OK) {
                raw_begin();
                ntk_gemv_seg segs[2] = {{raw_of(L.w_gate), gate_buf, I, L.w_gate.dtype}, {raw_of(L.w_up), up_buf, I, L.w_up.dtype}};
                NT_TRY(ntk_gemv_fused(segs, 2, hidden_, H, (const float*)L.ffn_norm.ptr, cfg_.norm_eps, nullptr, 1, s));
            }
            mark(0, false);
        } else {
            const DevTensor* ws[2] = {&L.w_gate, &L.w_up};
            float* ys[2] = {gate_buf, up_buf};
            NT_TRY(project(ws, ys, 2, hidden_, &L.ffn_norm, nullptr, 4));
            NT_TRY(ntk_silu_mul(gate_buf, gate_buf, up_buf, I, s));
        }
        if (tp_world_ > 1) {
            NT_TRY(project1(L.w_down, tp_slot(), gate_buf, nullptr, nullptr, 8));
            NT_TRY(tp_allreduce(hidden_, H));
        } else {
            NT_TRY(project1(L.w_down, hidden_, gate_buf, nullptr, hidden_, 8));
        }
    }
    return NTK_OK;
}

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
    NT_TRY(ntk_memcpy_h2d_async(hidden_, hidden_in, bytes, s));
    int rc;
    if (mode == 0) {
        std::vector<int> pos(T);
        for (int i = 0; i < T; ++i) pos[i] = start_pos + i;
        NT_TRY(ntk_memcpy_h2d_async(positions_, pos.data(), (size_t)T * 4, s));
        NT_TRY(ntk_stream_synchronize(s));
        rc = layers_1to1(T, start_pos, first, first + count);
    } else {
        NT_TRY(set_device_pos(start_pos));
        pick_attention_regime();
        if (mode == 1) {
            rc = enqueue_layers(first, first + count);
        } else {
            hipStream_t st = static_cast<hipStream_t>(s);
            hipGraph_t g = nullptr;
            if (hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal) != hipSuccess) return NTK_E_LAUNCH;
            rc = enqueue_layers(first, first + count);
            const hipError_t e = hipStreamEndCapture(st, &g);
            if (rc == NTK_OK && (e != hipSuccess || !g)) rc = NTK_E_LAUNCH;
            hipGraphExec_t ex = nullptr;
            if (rc == NTK_OK && hipGraphInstantiate(&ex, g, nullptr, nullptr, 0) != hipSuccess) rc = NTK_E_LAUNCH;
            if (g) (void)hipGraphDestroy(g);
            if (rc == NTK_OK && hipGraphLaunch(ex, st) != hipSuccess) rc = NTK_E_LAUNCH;
            if (rc == NTK_OK) rc = ntk_stream_synchronize(s);
            if (ex) (void)hipGraphExecDestroy(ex);
        }
    }
    if (rc != NTK_OK) return rc;
    NT_TRY(ntk_memcpy_d2h_async(hidden_out, hidden_, bytes, s));
    return ntk_stream_synchronize(s);
}

// cache rows [pos0, pos0 + n) of one layer, [n][n_kv_heads * head_dim] halves each (reference layout, transformer.cpp:340-346)
int Model::debug_kv(int layer, int pos0, int n, uint16_t* k, uint16_t* v, bool write) {
    if (!k || !v) return NTK_E_NULL;
    if (kv_q8_) { err_ = "debug_kv: the KV cache is q8_0 (use the _q8 form)"; return NTK_E_DTYPE; }
    if (layer < 0 || layer >= cfg_.n_layers || pos0 < 0 || n < 0 || pos0 + n > cfg_.max_seq_len) return NTK_E_SHAPE;
    const size_t per = (size_t)cfg_.n_kv_heads * cfg_.head_dim;
    const size_t off = ((size_t)layer * cfg_.max_seq_len + pos0) * per, bytes = (size_t)n * per * 2;
    void* s = stream_;
    if (write) {
        NT_TRY(ntk_memcpy_h2d_async(k_cache_ + off, k, bytes, s));
        NT_TRY(ntk_memcpy_h2d_async(v_cache_ + off, v, bytes, s));
    } else {
        NT_TRY(ntk_memcpy_d2h_async(k, k_cache_ + off, bytes, s));
        NT_TRY(ntk_memcpy_d2h_async(v, v_cache_ + off, bytes, s));
    }
    return ntk_stream_synchronize(s);
}

// ... of the 8-bit cache, as canonical 34-byte GGUF block_q8_0 {half d; int8 q[32]}: [n][n_kv_heads * head_dim / 32] blocks per side.  The device
// keeps quants and scales in two planes (csrc/attention_q8.hip): the rows' slices of both are contiguous, the blocks are (de)interleaved here.
int Model::debug_kv_q8(int layer, int pos0, int n, uint8_t* k_blocks, uint8_t* v_blocks, bool write) {
    if (!k_blocks || !v_blocks) return NTK_E_NULL;
    if (!kv_q8_) { err_ = "debug_kv_q8: the KV cache is f16"; return NTK_E_DTYPE; }
    if (layer < 0 || layer >= cfg_.n_layers || pos0 < 0 || n < 0 || pos0 + n > cfg_.max_seq_len) return NTK_E_SHAPE;
    if (n == 0) return NTK_OK;
    const size_t per = (size_t)cfg_.n_kv_heads * cfg_.head_dim, nb = per / 32;
    const size_t qbytes = (size_t)n * per, sbytes = (size_t)n * nb * 2;
    void* s = stream_;
    std::vector<uint8_t> qh(qbytes), sh(sbytes);
    for (int side = 0; side < 2; ++side) {
        uint8_t* base = (side ? v_cache_q8_ : k_cache_q8_) + (size_t)layer * kv_q8_layer_bytes_;
        uint8_t* qd = base + (size_t)pos0 * per;
        uint8_t* sd = base + (size_t)cfg_.max_seq_len * per + (size_t)pos0 * nb * 2;
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
        kv_capture_ = (float*)nt_hip_malloc(bytes);
        if (!kv_capture_) { err_ = "debug_kv_inputs_capture: out of device memory"; return NTK_E_NOMEM; }
        allocs_.push_back(kv_capture_);
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

int Model::set_kv_cache(const std::string& kind) {
    if (kind != "f16" && kind != "q8_0") { err_ = "kv_cache: unknown format '" + kind + "' (f16 or q8_0)"; return NTK_E_DTYPE; }
    if (!layers_.empty()) { err_ = "kv_cache must be set before the model is loaded"; return NTK_E_SHAPE; }
    const bool q8 = kind == "q8_0";
    if (q8 && fuse_attention_) { err_ = "kv_cache=q8_0 is not supported with the attention-inside-Wo launch (fuse_attention)"; return NTK_E_SHAPE; }
    kv_q8_ = q8;
    return NTK_OK;
}

int Model::set_fuse_attention(bool on) {
    if (on && kv_q8_) { err_ = "fuse_attention (attention inside the Wo launch) is not supported with kv_cache=q8_0"; return NTK_E_SHAPE; }
    fuse_attention_ = on;
    return NTK_OK;
}

// A tensor-parallel exchange whose bounded wait for a peer gave up has added garbage: surface it (and clear the sticky word)
int Model::check_tp() {
    if (tp_world_ <= 1 || !tp_comm_) return NTK_OK;
    const unsigned e = tp_error();
    if (e == 0u) return NTK_OK;
    const unsigned zero = 0u;
    (void)ntk_memcpy_h2d_async(static_cast<uint8_t*>(tp_comm_) + 128, &zero, 4, stream_);
    (void)ntk_stream_synchronize(stream_);
    err_ = "tensor-parallel exchange: a peer rank did not arrive (call tag " + std::to_string(e) + "); the token's results are invalid";
    fprintf(stderr, "%s\n", err_.c_str());
    return NTK_E_LAUNCH;
}

bool Model::use_persistent_now() const {
    return persistent_plan_ && persistent_on_ && attn_regime_ == 0 && !prof_;
}

void Model::set_persistent(int level) {   // 0 off, 1 the round-2 token kernel (decode_persistent.hip), 2 the loader / consumer engine (layer_engine.hip)
    const bool on = level != 0;
    persistent_on_ = false;
    persistent_wanted_ = level;   // (asked before the load: finish_load() applies it)
#ifndef NTK_EXPERIMENTS
    if (on) fprintf(stderr, "note: the persistent token kernels are built by experiments/Makefile only (experiments/libntransformer_hip_exp.so); this library decodes with fused launches\n");
#else
    if (persistent_plan_ && persistent_kind_ != (level == 2 ? 2 : 1)) {   // the other kernel's plan: drop it and its captured graphs
        (void)sync();
        for (auto& row : graphs_) { if (row[kPersistentSlot]) (void)hipGraphExecDestroy(reinterpret_cast<hipGraphExec_t>(row[kPersistentSlot])); row[kPersistentSlot] = nullptr; }
        if (persistent_kind_ == 2) ntk_layer_engine_plan_destroy(persistent_plan_); else ntk_persistent_plan_destroy(persistent_plan_);
        persistent_plan_ = nullptr;
    }
#endif
    if (!on || tp_world_ != 1 || layers_.empty()) return;
    if (kv_q8_) { fprintf(stderr, "note: the persistent token kernels read the F16 KV cache; kv_cache=q8_0 decodes with fused launches\n"); return; }
    if (raw_freed_bytes_ > 0) (void)set_repack(1);   // the persistent kernels stream the GGUF bytes themselves: those must be resident
    if (!persistent_plan_) (void)build_persistent_plan(level == 2 ? 2 : 1);   // built on first use (EXPERIMENTS=1 builds only): it allocates device memory
    persistent_on_ = persistent_plan_ != nullptr;
}

// what decode_step_fused() emits at the CURRENT position (the persistent form covers the single-pass attention regime only)
const char* Model::decode_path() const {
    if (persistent_plan_ && persistent_on_ && persistent_kind_ == 2)
        return attn_regime_ == 0 ? "persistent layer engine (1 launch per token: loader / consumer waves, granule hand-offs; fused launches beyond the single-pass attention regime)"
                                 : "fused (5 launches/layer; persistent layer engine below the split-attention regime)";
    if (persistent_plan_ && persistent_on_)
        return attn_regime_ == 0 ? "persistent (1 launch per token in the single-pass attention regime, fused launches beyond)"
                                 : "fused (5 launches/layer; persistent below the split-attention regime)";
    return "fused (5 launches/layer)";
}

// after a sync: NTK_OK, or NTK_E_LAUNCH when an in-kernel bounded wait gave up (tensor-parallel exchange; with
// EXPERIMENTS=1 also the persistent token kernel and the attention-in-Wo launch, which are then disabled)
int Model::check_persistent() {
    NT_TRY(check_tp());
#ifdef NTK_EXPERIMENTS
    if (attn_sync_ && fuse_attention_) {   // ntk_attention_gemv_fused: a bounded in-kernel wait that gave up
        unsigned w[3] = {0, 0, 0};
        if (ntk_memcpy_d2h_async(w, attn_sync_, sizeof w, stream_) != NTK_OK || ntk_stream_synchronize(stream_) != NTK_OK) return NTK_E_LAUNCH;
        if (w[2] != 0) {
            fuse_attention_ = false;
            nt_hip_memset(attn_sync_, 0, 4096);
            for (auto& row : graphs_) for (auto& gx : row) { if (gx) (void)hipGraphExecDestroy(reinterpret_cast<hipGraphExec_t>(gx)); gx = nullptr; }
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
#else
    return NTK_OK;
#endif
}

#ifdef NTK_EXPERIMENTS
// The token's operator table for the persistent kernel: exactly the sequence enqueue_token() launches.
int Model::build_persistent_plan(int kind) {
    const int H = cfg_.hidden_size, I = cfg_.intermediate_size, hd = cfg_.head_dim, nh = cfg_.n_heads, nkv = cfg_.n_kv_heads;
    const int qd = nh * hd, kvd = nkv * hd;
    if (hd != 64 && hd != 128) return NTK_E_SHAPE;
    if (const char* e = getenv("NTK_NO_PERSISTENT")) { if (atoi(e)) return NTK_E_SHAPE; }
    const float scale = 1.0f / sqrtf((float)hd);
    const size_t kv_layer = (size_t)cfg_.max_seq_len * kvd;
    float* q_buf = workspace_;
    float* k_buf = q_buf + qd;
    float* v_buf = k_buf + kvd;
    float* attn_out = v_buf + kvd;
    float* gate_buf = workspace_;
    float* up_buf = gate_buf + I;
    std::vector<ntk_pop> ops;
    bool ok = true;
    // n matrices sharing x: one operator per dtype group (Q4_K_M: attn_v is Q6_K / Q5_K next to Q4_K q, k); only the first
    // waits for x, only the last signals
    auto gemv_group = [&](const DevTensor* const* ws, float* const* ys, int n, const float* x, const DevTensor* norm, const float* resid,
                          bool wait, bool arrive, bool plain) {
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
            float* ys[3] = {q_buf, k_buf, v_buf};
            gemv_group(ws, ys, 3, hidden_, &L.attn_norm, nullptr, i > 0, true, false);   // layer 0 reads the embedding kernel's output
        }
        ntk_pop a;
        memset(&a, 0, sizeof a);
        a.kind = NTK_POP_ATTENTION; a.wait = 1; a.arrive = 1;
        a.out = attn_out; a.q = q_buf; a.k = k_buf; a.v = v_buf;
        a.k_cache = k_cache_ + (size_t)i * kv_layer; a.v_cache = v_cache_ + (size_t)i * kv_layer;
        a.inv_freq = rope_inv_freq_;
        a.n_heads = nh; a.n_kv_heads = nkv; a.head_dim = hd; a.max_seq = cfg_.max_seq_len;
        a.scale = scale; a.theta_base = cfg_.rope_theta; a.freq_scale = cfg_.rope_freq_scale;
        ops.push_back(a);
        {
            const DevTensor* ws[1] = {&L.wo};
            float* ys[1] = {hidden_};
            gemv_group(ws, ys, 1, attn_out, nullptr, hidden_, true, true, false);
        }
        if (!(is_quant(L.w_gate.dtype) && L.w_gate.dtype == L.w_up.dtype)) { ok = false; break; }
        {
            ntk_pop o;
            memset(&o, 0, sizeof o);
            o.kind = NTK_POP_GEMV; o.wait = 1; o.arrive = 1;
            o.segs[0] = {L.w_gate.ptr, gate_buf, I, L.w_gate.dtype};
            o.segs[1] = {L.w_up.ptr, up_buf, I, L.w_up.dtype};
            o.nseg = 2; o.in_features = H; o.silu_pair = 1; o.eps = cfg_.norm_eps;
            o.x = hidden_; o.norm_w = (const float*)L.ffn_norm.ptr;
            ops.push_back(o);
        }
        {
            const DevTensor* ws[1] = {&L.w_down};
            float* ys[1] = {hidden_};
            gemv_group(ws, ys, 1, gate_buf, nullptr, hidden_, true, true, false);
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
#else
int Model::build_persistent_plan(int) { return NTK_E_SHAPE; }
#endif

void Model::pick_attention_regime() {
    attn_regime_ = (attn_scratch_ && (cfg_.head_dim == 64 || cfg_.head_dim == 128 || cfg_.head_dim == 256))
                       ? attention_regime(host_pos_, cfg_.head_dim) : 0;
    ++host_pos_;   // every fused token ends with ntk_advance_pos on the device; set_device_pos() re-bases both
}

int Model::decode_step_fused(bool greedy, bool use_graph) {
    pick_attention_regime();
    if (!use_graph) return enqueue_token(greedy);
    ihipGraphExec_t*& slot = graphs_[greedy ? 1 : 0][use_persistent_now() ? kPersistentSlot : attn_regime_];
    hipStream_t st = static_cast<hipStream_t>(stream_);
    if (!slot) {   // capture once: every per-token quantity (token id, position) lives in device memory
        hipGraph_t g = nullptr;
        // (relaxed under tensor parallelism: ranks sharing a process run their own runtime calls on other threads meanwhile)
        if (hipStreamBeginCapture(st, tp_world_ > 1 ? hipStreamCaptureModeRelaxed : hipStreamCaptureModeThreadLocal) != hipSuccess) return NTK_E_LAUNCH;
        const int rc = enqueue_token(greedy);
        const hipError_t e = hipStreamEndCapture(st, &g);
        if (rc != NTK_OK || e != hipSuccess || !g) { if (g) (void)hipGraphDestroy(g); return rc != NTK_OK ? rc : NTK_E_LAUNCH; }
        hipGraphExec_t ex = nullptr;
        const hipError_t ie = hipGraphInstantiate(&ex, g, nullptr, nullptr, 0);
        (void)hipGraphDestroy(g);
        if (ie != hipSuccess) return NTK_E_LAUNCH;
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
