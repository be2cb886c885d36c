// engine/model_load.cpp -- weights into HBM: GGUF and synthetic loading, the decode repack and its one-resident-copy bookkeeping, buffers (see model.h)
#include "model_impl.h"

namespace nt {

int Model::upload(DevTensor& dst, const void* host, int dtype, int64_t in_f, int64_t out_f, size_t nbytes) {
    void* d = dev_alloc(padded_bytes(nbytes), false);
    if (!d) { err_ = "out of device memory"; return NTK_E_NOMEM; }
    if (host && nbytes) {   // a failed upload must not leave silently garbage weights behind
        if (hipMemcpy(d, host, nbytes, hipMemcpyHostToDevice) != hipSuccess) { err_ = "weight upload (H2D copy) failed"; return NTK_E_LAUNCH; }
    }
    dst.ptr = d; dst.dtype = dtype; dst.in_f = in_f; dst.out_f = out_f; dst.nbytes = nbytes;
    weight_bytes_ += nbytes;
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

// a layer's tensors "blk.<i>.<name>": member, shard rule over tensor-parallel ranks, [out][in] extents (h hidden, q / k query / KV heads x head_dim, i FFN
// width, 1 a vector) -- the one description both loaders go by
static const struct { const char* name; DevTensor LayerWeights::* member; Shard how; char in, out; } kLayerTensors[] = {
    {"attn_norm.weight", &LayerWeights::attn_norm, WHOLE, 'h', '1'},
    {"attn_q.weight", &LayerWeights::wq, ROWS, 'h', 'q'},             // whole heads per rank
    {"attn_k.weight", &LayerWeights::wk, ROWS, 'h', 'k'},
    {"attn_v.weight", &LayerWeights::wv, ROWS, 'h', 'k'},
    {"attn_output.weight", &LayerWeights::wo, COLS, 'q', 'h'},        // the columns of this rank's heads
    {"ffn_norm.weight", &LayerWeights::ffn_norm, WHOLE, 'h', '1'},
    {"ffn_gate.weight", &LayerWeights::w_gate, ROWS, 'h', 'i'},
    {"ffn_up.weight", &LayerWeights::w_up, ROWS, 'h', 'i'},
    {"ffn_down.weight", &LayerWeights::w_down, COLS, 'i', 'h'},
};
// ... and the optional ones, "blk.<i>.<name>": the Q | K | V projection biases (Qwen2; llama.cpp takes them under `llama` too) -- F32, one value per output
// row, so a rank's whole heads are a contiguous slice (ROWS)
static const struct { const char* name; DevTensor LayerWeights::* member; char out; } kLayerBiases[] = {
    {"attn_q.bias", &LayerWeights::bq, 'q'},
    {"attn_k.bias", &LayerWeights::bk, 'k'},
    {"attn_v.bias", &LayerWeights::bv, 'k'},
};
// the per-head RMSNorm weights of Q and K (Qwen3): F32 [head_dim], one vector for all heads of the layer, so every rank holds it WHOLE; a pair per layer
static const struct { const char* name; DevTensor LayerWeights::* member; } kLayerQkNorms[] = {
    {"attn_q_norm.weight", &LayerWeights::q_norm},
    {"attn_k_norm.weight", &LayerWeights::k_norm},
};
// per-layer tensors of neighbouring architectures that this engine has no kernel for: a file that carries one is refused rather than run without it
static const char* const kLayerUnsupported[] = {"attn_output.bias", "ffn_gate.bias", "ffn_up.bias", "ffn_down.bias",
                                                // the shared experts of Qwen2-MoE / DeepSeek and DeepSeek's biased routing: not built
                                                "ffn_gate_inp_shexp.weight", "ffn_gate_shexp.weight", "ffn_up_shexp.weight", "ffn_down_shexp.weight", "exp_probs_b.bias"};
// the routed expert FFN of a mixture-of-experts layer, in place of the dense ffn_gate / ffn_up / ffn_down trio: the F32 router, ggml dims (hidden, E), and
// three 3-D expert tensors, dims (in, out, E) -- 'h' hidden, 'e' the expert FFN width.  They stay raw GGUF bytes: no repack, never freed, shared by load_shared.
static const struct { const char* name; DevTensor LayerWeights::* member; char in, out; } kLayerExperts[] = {
    {"ffn_gate_inp.weight", &LayerWeights::router, 'h', 'E'},
    {"ffn_gate_exps.weight", &LayerWeights::gate_exps, 'h', 'e'},
    {"ffn_up_exps.weight", &LayerWeights::up_exps, 'h', 'e'},
    {"ffn_down_exps.weight", &LayerWeights::down_exps, 'e', 'h'},
};
static const char* const kLayerDenseFfn[] = {"ffn_gate.weight", "ffn_up.weight", "ffn_down.weight"};

int Model::check_layer_extras(const GgufFile& f) {
    const int64_t qd = (int64_t)cfg_.n_heads * cfg_.head_dim, kvd = (int64_t)cfg_.n_kv_heads * cfg_.head_dim;
    std::vector<const GgufTensor*> norms[2];   // the layer's q / k norm by layer index, for the pair rule below
    for (auto& v : norms) v.assign((size_t)std::max(cfg_.n_layers, 0), nullptr);
    std::vector<const GgufTensor*> experts[4];   // ... and its expert quartet, for the all-or-none rule
    for (auto& v : experts) v.assign((size_t)std::max(cfg_.n_layers, 0), nullptr);
    std::vector<const GgufTensor*> dense_ffn((size_t)std::max(cfg_.n_layers, 0), nullptr);   // (any one of the dense trio)
    const std::string pre = cfg_.architecture + ".";
    const int64_t H = cfg_.hidden_size, E = cfg_.expert_count, Ie = cfg_.expert_ff_length;
    bool any_expert = false;
    for (const GgufTensor& t : f.tensors()) {   // every "blk.<i>.<name>" of the file, whatever its index: a tensor behind the last layer is not passed over either
        int li = -1, at = 0;
        if (sscanf(t.name.c_str(), "blk.%d.%n", &li, &at) != 1 || at == 0) continue;
        const char* const rest = t.name.c_str() + at;
        for (const char* u : kLayerUnsupported)
            if (strcmp(rest, u) == 0) { err_ = "Unsupported tensor " + t.name + ": this engine runs Llama, Qwen2, Qwen3 and routed mixture-of-experts layers (no attention-output or FFN bias, no shared experts or biased routing)"; return NTK_E_FORMAT; }
        for (const char* d : kLayerDenseFfn)
            if (strcmp(rest, d) == 0 && li >= 0 && li < cfg_.n_layers) dense_ffn[(size_t)li] = &t;
        for (int w = 0; w < 4; ++w) {
            if (strcmp(rest, kLayerExperts[w].name) != 0) continue;
            if (li < 0 || li >= cfg_.n_layers) {
                err_ = "Unsupported tensor " + t.name + ": the model has " + std::to_string(cfg_.n_layers) + " layers";
                return NTK_E_FORMAT;
            }
            if (tp_world_ > 1) { err_ = "Unsupported tensor " + t.name + ": tensor parallelism over a mixture-of-experts layer is not built"; return NTK_E_SHAPE; }
            // the keys first: every extent below is measured against them
            if (E < 1 || E > 256) { err_ = pre + "expert_count = " + std::to_string(E) + ": 1 .. 256 experts are supported (" + t.name + ")"; return NTK_E_SHAPE; }
            if (cfg_.expert_used_count < 1 || cfg_.expert_used_count > std::min<int64_t>(E, 16)) {
                err_ = pre + "expert_used_count = " + std::to_string(cfg_.expert_used_count) + ": 1 .. min(expert_count, 16) experts per token are supported (" + t.name + ")";
                return NTK_E_SHAPE;
            }
            if (Ie < 1) { err_ = pre + "expert_feed_forward_length is missing or not positive (" + t.name + ")"; return NTK_E_SHAPE; }
            if (w == 0) {
                if (t.dtype != NTK_DT_F32 || !t.known_type) { err_ = t.name + " must be F32"; return NTK_E_DTYPE; }
                if (t.numel() != H * E || (t.dims.size() >= 1 && t.dims[0] != H)) {
                    err_ = t.name + " holds " + std::to_string(t.numel()) + " values, hidden x expert_count = " + std::to_string(H) + " x " + std::to_string(E) + " are needed";
                    return NTK_E_SHAPE;
                }
            } else {
                const int64_t in = kLayerExperts[w].in == 'h' ? H : Ie, out = kLayerExperts[w].out == 'h' ? H : Ie;
                if (t.dims.size() != 3 || t.dims[0] != in || t.dims[1] != out || t.dims[2] != E) {
                    err_ = "Unexpected shape for " + t.name + ": a 3-D tensor of dims (" + std::to_string(in) + ", " + std::to_string(out) + ", " + std::to_string(E) + ") is needed";
                    return NTK_E_SHAPE;
                }
                if (!t.known_type || (t.dtype != NTK_DT_Q8_0 && t.dtype != NTK_DT_Q4_K && t.dtype != NTK_DT_Q6_K)) {
                    err_ = "Unsupported tensor type for " + t.name + ": expert matrices are Q8_0, Q4_K or Q6_K";
                    return NTK_E_DTYPE;
                }
                if (ntk_row_bytes(t.dtype, in) == 0) {   // (a width the type cannot hold: Q4_K / Q6_K rows of a width that is no multiple of 256)
                    err_ = "Unexpected shape for " + t.name + ": rows of " + std::to_string(in) + " columns are not whole blocks of " + dtype_name(t.dtype);
                    return NTK_E_SHAPE;
                }
                if (ntk_moe_lds_bytes(t.dtype, -1, (int)std::min<int64_t>(in, 0x7FFFFFFF)) > NTK_MOE_LDS_MAX) {   // (one row per wave must fit the launch's LDS)
                    err_ = "Unexpected shape for " + t.name + ": rows of " + std::to_string(in) + " " + dtype_name(t.dtype) + " columns are beyond what the expert GEMV stages (" +
                           std::to_string(NTK_MOE_LDS_MAX) + " bytes of LDS for four rows)";
                    return NTK_E_SHAPE;
                }
            }
            experts[w][(size_t)li] = &t;
            any_expert = true;
        }
        for (int w = 0; w < 2; ++w) {
            if (strcmp(rest, kLayerQkNorms[w].name) != 0) continue;
            if (li < 0 || li >= cfg_.n_layers) {
                err_ = "Unsupported tensor " + t.name + ": the model has " + std::to_string(cfg_.n_layers) + " layers";
                return NTK_E_FORMAT;
            }
            if (t.dtype != NTK_DT_F32 || !t.known_type) { err_ = t.name + " must be F32"; return NTK_E_DTYPE; }
            if (t.numel() != cfg_.head_dim) {
                err_ = t.name + " holds " + std::to_string(t.numel()) + " values, " + std::to_string(cfg_.head_dim) + " (head_dim: one vector for all heads) are needed";
                return NTK_E_SHAPE;
            }
            norms[w][(size_t)li] = &t;
        }
        for (const auto& e : kLayerBiases) {
            if (strcmp(rest, e.name) != 0) continue;
            const int64_t want = e.out == 'q' ? qd : kvd;
            if (t.dtype != NTK_DT_F32 || !t.known_type) { err_ = t.name + " must be F32"; return NTK_E_DTYPE; }
            if (t.numel() != want) {
                err_ = t.name + " holds " + std::to_string(t.numel()) + " values, " + std::to_string(want) + " (one per output row) are needed";
                return NTK_E_SHAPE;
            }
        }
    }
    for (size_t i = 0; i < norms[0].size(); ++i) {   // a pair per layer: Q normalised against unnormalised K (or the reverse) is no model anyone trained
        const GgufTensor* const lone = norms[0][i] && !norms[1][i] ? norms[0][i] : norms[1][i] && !norms[0][i] ? norms[1][i] : nullptr;
        if (lone) {
            err_ = "Unsupported tensor " + lone->name + ": layer " + std::to_string(i) + " carries it without its partner (attn_q_norm.weight and attn_k_norm.weight come as a pair)";
            return NTK_E_FORMAT;
        }
    }
    for (size_t i = 0; i < dense_ffn.size(); ++i) {   // a layer carries the dense trio or the whole quartet
        int have = 0, missing = -1;
        const GgufTensor* first = nullptr;
        for (int w = 0; w < 4; ++w) {
            if (experts[w][i]) { ++have; if (!first) first = experts[w][i]; }
            else if (missing < 0) missing = w;
        }
        if (have && dense_ffn[i]) {
            err_ = "Unsupported tensor " + first->name + ": layer " + std::to_string(i) + " also carries " + dense_ffn[i]->name + " (a layer has the dense FFN or the experts, not both)";
            return NTK_E_FORMAT;
        }
        if (have == 4 && ntk_moe_lds_bytes(experts[1][i]->dtype, experts[2][i]->dtype, (int)H) > NTK_MOE_LDS_MAX) {   // gate | up stage a row of each per wave
            err_ = "Unexpected shape for " + experts[2][i]->name + ": rows of " + std::to_string(H) + " columns of " + dtype_name(experts[1][i]->dtype) + " gate and " +
                   dtype_name(experts[2][i]->dtype) + " up experts are beyond what the expert GEMV stages (" + std::to_string(NTK_MOE_LDS_MAX) + " bytes of LDS for four row pairs)";
            return NTK_E_SHAPE;
        }
        if (have && have < 4) {
            err_ = "Tensor not found: blk." + std::to_string(i) + "." + kLayerExperts[missing].name + " (layer " + std::to_string(i) + " carries " + first->name + ": the router and the three expert tensors come together)";
            return NTK_E_FORMAT;
        }
    }
    if (!any_expert && (cfg_.expert_count > 0 || cfg_.expert_used_count > 0)) {
        err_ = pre + (cfg_.expert_count > 0 ? "expert_count = " + std::to_string(cfg_.expert_count) : "expert_used_count = " + std::to_string(cfg_.expert_used_count)) +
               ": the file names experts and carries no blk.N.ffn_gate_inp.weight / ffn_*_exps.weight";
        return NTK_E_FORMAT;
    }
    return NTK_OK;
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
    st = resolve_rope(&f);   // (before anything is allocated: a bad rope_freqs.weight refuses the load)
    if (st != NTK_OK) { fprintf(stderr, "%s\n", err_.c_str()); return st; }
    st = check_layer_extras(f);   // (likewise: a bias of the wrong type or size, a tensor the layer loop would ignore)
    if (st != NTK_OK) { fprintf(stderr, "%s\n", err_.c_str()); return st; }
    cfg_.print();
    f.print_info();
    st = init_device();
    if (st != NTK_OK) { fprintf(stderr, "%s\n", err_.c_str()); return st; }

    NT_TRY(tp_check_shapes());
    auto take = [&](const std::string& name) -> int {
        const GgufTensor* t = f.find(name);
        TensorSlot sl;
        if (!t || !slot_of(name, &sl)) { err_ = "Tensor not found: " + name; return NTK_E_FORMAT; }
        const int64_t in_f = sl.in_f, out_f = sl.out_f;
        const bool vec = out_f == 1;
        if (t->numel() != in_f * out_f || (!vec && (t->dims.size() != 2 || t->dims[0] != in_f))) {
            err_ = "Unexpected shape for " + name;
            return NTK_E_SHAPE;
        }
        if (vec && t->dtype != NTK_DT_F32) { err_ = name + " must be F32"; return NTK_E_DTYPE; }
        if (t->nbytes == 0 || !t->known_type) { err_ = "Unsupported tensor type for " + name; return NTK_E_DTYPE; }
        return upload_shard(*sl.dst, f.data(*t), t->dtype, in_f, out_f, t->nbytes, sl.how);
    };
    layers_.resize(cfg_.n_layers);
    NT_TRY(take("token_embd.weight"));
    if (f.find("output.weight")) {   // transformer.cpp:92-99
        NT_TRY(take("output.weight"));
    } else {
        output_ = token_embd_;
        output_tied_ = true;
    }
    NT_TRY(take("output_norm.weight"));
    for (int i = 0; i < cfg_.n_layers; ++i) {   // transformer.cpp:286-328
        const std::string blk = "blk." + std::to_string(i) + ".";
        const bool moe = f.find(blk + kLayerExperts[0].name) != nullptr;   // (check_layer_extras: the whole quartet and no dense trio, or the reverse)
        for (const auto& e : kLayerTensors) {
            if (moe && (e.member == &LayerWeights::w_gate || e.member == &LayerWeights::w_up || e.member == &LayerWeights::w_down)) continue;
            NT_TRY(take(blk + e.name));
        }
        for (const auto& e : kLayerExperts) {   // held to type and extents by the pre-pass; uploaded whole, as the file has them
            if (!moe) break;
            const GgufTensor* t = f.find(blk + e.name);
            TensorSlot sl;
            if (!t || !slot_of(blk + e.name, &sl)) { err_ = "Tensor not found: " + blk + e.name; return NTK_E_FORMAT; }
            NT_TRY(upload(*sl.dst, f.data(*t), t->dtype, sl.in_f, sl.out_f, t->nbytes));
        }
        // the optional biases.  take()'s checks do not run here: check_layer_extras() -- called above, ahead of the device -- has held every bias of the
        // file to F32 and to its slot's element count, and a loader that gets here another way must do the same before it uploads one
        for (const auto& e : kLayerBiases) {
            const std::string name = "blk." + std::to_string(i) + "." + e.name;
            const GgufTensor* t = f.find(name);
            TensorSlot sl;
            if (!t || !slot_of(name, &sl)) continue;
            NT_TRY(upload_shard(*sl.dst, f.data(*t), t->dtype, sl.in_f, sl.out_f, t->nbytes, sl.how));
        }
        for (const auto& e : kLayerQkNorms) {   // ... and the optional Q / K norm pair, held to F32, head_dim values and a pair per layer by the same pre-pass
            const std::string name = "blk." + std::to_string(i) + "." + e.name;
            const GgufTensor* t = f.find(name);
            TensorSlot sl;
            if (!t || !slot_of(name, &sl)) continue;
            NT_TRY(upload_shard(*sl.dst, f.data(*t), t->dtype, sl.in_f, sl.out_f, t->nbytes, sl.how));
        }
    }
    return finish_load();
}

bool Model::slot_of(const std::string& name, TensorSlot* sl) {
    const int64_t H = cfg_.hidden_size, hd = cfg_.head_dim;
    auto extent = [&](char c) -> int64_t { return c == 'h' ? H : c == 'q' ? cfg_.n_heads * hd : c == 'k' ? cfg_.n_kv_heads * hd : c == 'i' ? cfg_.intermediate_size : 1; };
    if (name == "token_embd.weight") { *sl = {&token_embd_, WHOLE, H, cfg_.vocab_size}; return true; }
    if (name == "output.weight") { *sl = {&output_, WHOLE, H, cfg_.vocab_size}; return true; }
    if (name == "output_norm.weight") { *sl = {&output_norm_, WHOLE, H, 1}; return true; }
    int li = -1, at = 0;
    if (sscanf(name.c_str(), "blk.%d.%n", &li, &at) != 1 || at == 0 || li < 0 || li >= (int)layers_.size()) return false;
    for (const auto& e : kLayerTensors)
        if (name.compare(at, std::string::npos, e.name) == 0) { *sl = {&(layers_[li].*e.member), e.how, extent(e.in), extent(e.out)}; return true; }
    for (const auto& e : kLayerBiases)   // [out] values: `out` rows of one element
        if (name.compare(at, std::string::npos, e.name) == 0) { *sl = {&(layers_[li].*e.member), ROWS, 1, extent(e.out)}; return true; }
    for (const auto& e : kLayerQkNorms)   // [head_dim] values, whole on every rank
        if (name.compare(at, std::string::npos, e.name) == 0) { *sl = {&(layers_[li].*e.member), WHOLE, hd, 1}; return true; }
    for (const auto& e : kLayerExperts) {   // ONE expert's [out][in] (the router: [E][hidden]); the tensor holds expert_count of them back to back
        auto ext = [&](char c) -> int64_t { return c == 'h' ? H : c == 'E' ? cfg_.expert_count : cfg_.expert_ff_length; };
        if (name.compare(at, std::string::npos, e.name) == 0) { *sl = {&(layers_[li].*e.member), WHOLE, ext(e.in), ext(e.out)}; return true; }
    }
    return false;
}

int Model::load_synthetic(const SynthSpec& spec, int max_context, int nthreads) {
    free_all();
    std::vector<SynthTensor> plan;
    if (!synth_plan(spec, plan)) { err_ = "bad synthetic spec"; return NTK_E_SHAPE; }
    cfg_ = ModelConfig();
    cfg_.model_name = "synthetic-" + spec.mix;
    const SynthFlavour fl = synth_flavour(spec.mix);
    if (fl.qwen2 || fl.qwen3) cfg_.architecture = fl.qwen3 ? (fl.experts ? "qwen3moe" : "qwen3") : "qwen2";
    if (fl.experts) {   // (synth_plan has held the counts to the engine's limits)
        if (tp_world_ > 1) { err_ = "tensor parallelism over a mixture-of-experts model is not built"; return NTK_E_SHAPE; }
        cfg_.expert_count = fl.experts; cfg_.expert_used_count = fl.used; cfg_.expert_ff_length = fl.expert_inter > 0 ? fl.expert_inter : spec.inter;
    }
    cfg_.vocab_size = spec.vocab; cfg_.hidden_size = spec.hidden; cfg_.intermediate_size = spec.inter;
    cfg_.n_layers = spec.layers; cfg_.n_heads = spec.heads; cfg_.n_kv_heads = spec.kv_heads;
    cfg_.head_dim = fl.head_dim ? fl.head_dim : spec.hidden / spec.heads;   // (synth_plan has held it to a positive even value)
    cfg_.norm_eps = spec.eps; cfg_.rope_theta = spec.theta;
    cfg_.max_seq_len = std::min(spec.ctx, max_context);
    cfg_.bos_token_id = spec.bos; cfg_.eos_token_id = spec.eos;
    synth_vocab(spec, vocab_.tokens, vocab_.token_types);
    NT_TRY(resolve_rope(nullptr));   // (the spec carries no scaling: the rope options give a synthetic model one)
    NT_TRY(init_device());
    NT_TRY(tp_check_shapes());

    size_t biggest = 0;
    for (const auto& t : plan) biggest = std::max(biggest, t.nbytes);
    void* stage = nt_hip_malloc_host(biggest);
    if (!stage) { err_ = "pinned staging allocation failed"; return NTK_E_NOMEM; }
    layers_.resize(cfg_.n_layers);
    int rc = NTK_OK;
    for (const auto& t : plan) {
        synth_fill(stage, t, spec.seed, nthreads);
        TensorSlot sl;
        if (!slot_of(t.name, &sl)) { rc = NTK_E_FORMAT; break; }
        // (an expert tensor: ONE expert's extents, the bytes of all of them)
        if (t.experts > 0) rc = upload(*sl.dst, stage, ggml_type_to_dtype((uint32_t)t.ggml_type), sl.in_f, sl.out_f, t.nbytes);
        else rc = upload_shard(*sl.dst, stage, ggml_type_to_dtype((uint32_t)t.ggml_type), t.in_f, t.out_f, t.nbytes, sl.how);
        if (rc != NTK_OK) break;
    }
    nt_hip_free_host(stage);
    if (rc == NTK_OK && !output_.ptr) {   // a plan without output.weight (the Qwen2 flavour's tied head): as load_impl
        output_ = token_embd_;
        output_tied_ = true;
    }
    if (rc == NTK_OK) rc = finish_load();
    if (rc != NTK_OK) free_all();
    return rc;
}

int Model::finish_load() {
    cfg_full_ = cfg_;
    if (tp_world_ > 1) {   // from here on this object IS a model with 1/W of the heads and of the FFN width (hidden size unchanged)
        cfg_.n_heads /= tp_world_;
        cfg_.n_kv_heads /= tp_world_;
        cfg_.intermediate_size /= tp_world_;
        NT_TRY(own_stream());   // ranks that share a process (tests) must not queue behind each other's waiting kernels
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
            for (auto& L : layers_) for (auto m : kLayerMatrices) kept += (L.*m).rp ? 0 : 1;
            fprintf(stderr, "warning: not enough device memory for the decode repack of every matrix: %d projection tensors stay on the raw-GGUF path\n", kept);
            err_.clear();
        } else if (st != NTK_OK) {
            return st;
        }
        if (repack_ == 3) repack_ = 2;   // round 6: the prompt GEMM reads the repack itself, so the second copy buys the batched paths nothing
        if (repack_ == 2) NT_TRY(drop_raw_all());
    }
    size_t fr = 0, tot = 0;
    ntk_device_mem_info(&fr, &tot);
    uint64_t q8_twice = 0;   // Q8_0 matrices resident in both forms (GGUF blocks for the prompt pass, lane-major rows for decode)
    for_each_projection([&](DevTensor& t) { if (t.rp && t.ptr && t.dtype == NTK_DT_Q8_0) q8_twice += t.rp_bytes; });
    fprintf(stderr, "Model loaded successfully! (resident on MI355X: %.2f GB of weights%s%s)\nFree VRAM: %.1f GB\n",
            (weight_bytes_ - raw_freed_bytes_) / 1073741824.0, repack_bytes_ ? (" + " + std::to_string(repack_bytes_ / 1073741824.0).substr(0, 5) + " GB repacked for decode").c_str() : "",
            q8_twice ? (", of which " + std::to_string(q8_twice / 1073741824.0).substr(0, 5) + " GB extra: Q8_0 matrices keep their GGUF bytes beside the repack").c_str() : "",
            fr / 1073741824.0);
    if (!layers_.empty())   // the formats a user chose the file for: an unquantised model says so
        fprintf(stderr, "Weight types: attn_q %s, ffn_down %s, output %s, token_embd %s\n", dtype_name(layers_[0].wq.dtype),
                dtype_name(layers_[0].is_moe() ? layers_[0].down_exps.dtype : layers_[0].w_down.dtype), dtype_name(output_.dtype), dtype_name(token_embd_.dtype));
    return NTK_OK;
}

// ---- engine-owned repack of the K-quant projections (csrc/gemv_rp.hip) and of the Q8_0 ones (lane-major rows, csrc/gemv.hip): made once, on the device, from the uploaded GGUF bytes, which
//      stay resident for the 1:1 launchers and the prompt GEMM ----
int Model::repack_one(DevTensor& t) {
    if (t.rp || !t.ptr) return NTK_OK;
    if (t.out_f <= 0 || t.out_f > 0x7FFFFFFF || t.in_f <= 0 || t.in_f > 32768) return NTK_OK;
    const bool q8 = t.dtype == NTK_DT_Q8_0;   // (its own form and entry points: the lane-major rows)
    const size_t n = q8 ? ntk_q8l_bytes((int)t.out_f, (int)t.in_f) : ntk_rp_bytes(t.dtype, (int)t.out_f, (int)t.in_f);
    if (n == 0 || n > 0xFFFFFFF0ull) return NTK_OK;   // formats / shapes without a repacked form keep the raw path
    void* d = dev_alloc(n, false);
    if (!d) return NTK_E_NOMEM;   // (the caller keeps the tensors that did fit and lets the raw path take the rest)
    const int st = q8 ? ntk_q8l_pack(d, t.ptr, (int)t.out_f, (int)t.in_f, stream_) : ntk_rp_pack(d, t.ptr, (int)t.out_f, (int)t.in_f, t.dtype, stream_);
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
        if (one(L.*kLayerMatrices[0]) == NTK_E_NOMEM) break;
        for (size_t k = 1; k < kLayerMatrices.size(); ++k) one(L.*kLayerMatrices[k]);
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
    // (a Q8_0 matrix keeps its GGUF bytes beside the lane-major repack: the prompt GEMM, the 1:1 launchers and embed_rows read GGUF Q8_0 blocks)
    auto goes = [&](const DevTensor& t) { return t.rp && t.dtype != NTK_DT_Q8_0 && !(output_tied_ && t.ptr == token_embd_.ptr); };
    auto grp = [&](std::initializer_list<DevTensor*> ts) {
        size_t g = 0;
        for (DevTensor* t : ts) if (goes(*t)) g += padded_bytes(t->nbytes);
        need = std::max(need, g);
    };
    for (auto& L : layers_) { grp({&L.wq, &L.wk, &L.wv}); grp({&L.wo}); grp({&L.w_gate, &L.w_up}); grp({&L.w_down}); }
    grp({&output_});
    if (need == 0) return NTK_OK;
    if (!raw_scratch_ || raw_scratch_bytes_ < need) {
        void* d = dev_alloc(need, false);
        if (!d) { fprintf(stderr, "warning: no device memory for the unpack scratch: the GGUF bytes stay resident beside the repack\n"); repack_ = 1; return NTK_OK; }
        raw_scratch_ = d; raw_scratch_bytes_ = need;
    }
    auto drop = [&](DevTensor& t) {
        if (!t.ptr || !goes(t)) return;
        dev_release(t.ptr);
        raw_freed_bytes_ += t.nbytes;
    };
    NT_TRY(ntk_stream_synchronize(stream_));
    for_each_projection(drop);
    return NTK_OK;
}

int Model::restore_raw_all() {
    int rc = NTK_OK;
    auto back = [&](DevTensor& t) {
        if (t.ptr || !t.rp || rc != NTK_OK) return;
        void* d = dev_alloc(padded_bytes(t.nbytes), false);
        if (!d) { rc = NTK_E_NOMEM; return; }
        const int st = ntk_rp_unpack(d, t.rp, (int)t.out_f, (int)t.in_f, t.dtype, stream_);
        if (st != NTK_OK) { dev_free(d); rc = st; return; }
        t.ptr = d;
        raw_freed_bytes_ -= t.nbytes;
    };
    for_each_projection(back);
    const int sy = ntk_stream_synchronize(stream_);
    return rc != NTK_OK ? rc : sy;
}

const void* Model::raw_of(const DevTensor& t) {
    if (t.ptr) return t.ptr;
    if (!t.rp || !raw_scratch_) { raw_err_ = NTK_E_NULL; return nullptr; }
    const size_t n = padded_bytes(t.nbytes);
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

int Model::alloc_buffers() {   // transformer.cpp:330-391
    const size_t S = (size_t)cfg_.max_seq_len, H = (size_t)cfg_.hidden_size;
    const size_t per = (size_t)cfg_.n_kv_heads * cfg_.head_dim;
    // the attention kernels address a layer's cache rows with 32-bit byte offsets (attention.hip): a context whose per-layer cache reaches
    // 3.75 GiB is refused here, at load, rather than as NTK_E_SHAPE from the first decode step (8 KV heads of 128: 1.9 M positions)
    if (S * per * sizeof(uint16_t) >= 0xF0000000ull) { err_ = "context too long: one layer's K cache must stay below 3.75 GiB (32-bit row offsets)"; return NTK_E_SHAPE; }
    if (kv_q8_) {   // the 8-bit cache (csrc/attention_q8.hip) + ONE layer's F16 image for the prompt path
        if (cfg_.head_dim != 128 || cfg_.n_kv_heads <= 0 || cfg_.n_heads % cfg_.n_kv_heads != 0 || cfg_.n_heads / cfg_.n_kv_heads > 16) {
            err_ = "kv_cache=q8_0 needs head_dim 128 and at most 16 query heads per KV head (this model: head_dim " + std::to_string(cfg_.head_dim) +
                   ", " + std::to_string(cfg_.n_kv_heads > 0 ? cfg_.n_heads / cfg_.n_kv_heads : 0) + " query heads per KV head)";
            return NTK_E_SHAPE;
        }
        if (tp_world_ > 1) { err_ = "kv_cache=q8_0 is not supported with tensor parallelism"; return NTK_E_SHAPE; }
    }
    if (sequences_ > 1) {   // the extra sequence slots: caches of slot 0's layout
        if (kv_q8_ && !batch_kv_q8_) { err_ = "sequences > 1 is not supported with kv_cache=q8_0"; return NTK_E_SHAPE; }
        if (tp_world_ > 1) { err_ = "sequences > 1 is not supported with tensor parallelism"; return NTK_E_SHAPE; }
        // a batched step is a prompt pass of up to `sequences` rows through buffers of max_seq rows (hidden_, residual_, workspace_, row_max_, kv_capture_)
        if ((size_t)sequences_ > S) { err_ = "sequences = " + std::to_string(sequences_) + " needs a context of at least as many positions (this load: " + std::to_string(S) + ")"; return NTK_E_SHAPE; }
    }
    NT_TRY(kv_.allocate(KvGeom{cfg_.n_layers, cfg_.max_seq_len, cfg_.n_kv_heads, cfg_.head_dim}, kv_q8_, sequences_, [&](size_t bytes, bool zero) { return dev_alloc(bytes, zero); }, &err_));
    hidden_ = (float*)dev_alloc(std::max<size_t>(S, 2) * H * 4, false);
    residual_ = (float*)dev_alloc(std::max<size_t>(S, 2) * H * 4, false);
    logits_ = (float*)dev_alloc((size_t)cfg_.vocab_size * 4, false);
    const size_t attn_ws = S * (size_t)(2 * cfg_.n_heads + 2 * cfg_.n_kv_heads) * cfg_.head_dim;
    const size_t ffn_ws = 2 * S * (size_t)cfg_.intermediate_size;
    workspace_floats_ = std::max(attn_ws, ffn_ws);
    workspace_ = (float*)dev_alloc(workspace_floats_ * 4, false);
    positions_ = (int*)dev_alloc(S * 4, false);
    tokens_dev_ = (int*)dev_alloc(S * 4, false);
    d_pos_ = (int*)dev_alloc(64, true);
    d_token_ = (int*)dev_alloc(64, true);
    argmax_scratch_ = (float*)dev_alloc(2 * 1024 * 4, false);
    rope_inv_freq_ = (float*)dev_alloc((size_t)cfg_.head_dim / 2 * 4 + 64, false);
    row_max_ = (float*)dev_alloc((size_t)S * 2 * 4, true);
    attn_scratch_ = (float*)dev_alloc(ntk_attention_split_scratch_bytes(cfg_.n_heads, cfg_.head_dim, kMaxAttnSplits), true);   // (zeroed: the arrival counters in front)
    h_token_ = (int*)nt_hip_malloc_host(64);
    h_ring_ = (unsigned long long*)nt_hip_malloc_host(64);
    if (h_ring_) memset(h_ring_, 0, 64);
    sample_scratch_ = dev_alloc(ntk_sample_scratch_bytes(cfg_.vocab_size), false);
    {   // one workspace for every projection: the largest need over the launches the prompt pass makes (Q|K|V and gate|up go out as one)
        const int H = cfg_.hidden_size, I = cfg_.intermediate_size, qkv = (cfg_.n_heads + 2 * cfg_.n_kv_heads) * cfg_.head_dim;
        const int shapes[][2] = {{H, qkv}, {H, cfg_.n_heads * cfg_.head_dim}, {H, cfg_.n_kv_heads * cfg_.head_dim}, {cfg_.n_heads * cfg_.head_dim, H},
                                 {H, 2 * I}, {H, I}, {I, H}};
        gemm_ws_bytes_ = 0;
        for (const auto& sh : shapes) gemm_ws_bytes_ = std::max(gemm_ws_bytes_, ntk_gemm_quant_workspace_bytes(sh[0], sh[1]));
        // ... and the planes of the 16-bit GEMM where the model has an F16 / BF16 matrix (a quantised-only model: not a byte more)
        auto dense16_need = [&](const DevTensor& t) {
            if (is_dense16(t.dtype)) gemm_ws_bytes_ = std::max(gemm_ws_bytes_, ntk_gemm_dense16_workspace_bytes((int)t.in_f, (int)t.out_f, t.dtype));
        };
        for (const auto& L : layers_) for (auto m : kLayerMatrices) dense16_need(L.*m);
        dense16_need(output_);
    }
    gemm_ws_ = dev_alloc(gemm_ws_bytes_, false);
    gemm_ws2_ = dev_alloc(gemm_ws_bytes_, false);
    moe_ws_ = nullptr; moe_rows_ = 0;
    if (moe_layers() > 0) {   // the routed FFN's workspace: normed rows, act, per-pair products, w, ids, the work list -- for passes of up to 1024 rows (longer ones go in pieces)
        moe_rows_ = (int)std::min<size_t>(S, 1024);
        const size_t n = ntk_moe_workspace_layout(moe_rows_, cfg_.expert_count, cfg_.expert_used_count, cfg_.expert_ff_length, cfg_.hidden_size, moe_off_);
        if (n == 0) { err_ = "mixture-of-experts workspace: expert counts out of range"; return NTK_E_SHAPE; }
        moe_ws_ = (uint8_t*)dev_alloc(n, true);
        if (!moe_ws_) { err_ = "buffer allocation failed (mixture-of-experts workspace)"; return NTK_E_NOMEM; }
        moe_gemm_scratch_ = nullptr;
        moe_gemm_scratch_bytes_ = ntk_moe_gemm_scratch_bytes(moe_rows_, cfg_.expert_count, cfg_.expert_used_count, cfg_.expert_ff_length, cfg_.hidden_size);
        if (moe_gemm_scratch_bytes_) {
            moe_gemm_scratch_ = dev_alloc(moe_gemm_scratch_bytes_, false);
            if (!moe_gemm_scratch_) { err_ = "buffer allocation failed (mixture-of-experts GEMM scratch)"; return NTK_E_NOMEM; }
        }
        for (auto& L : layers_) {   // which layers the grouped prompt GEMM takes: the expert types, whole blocks per row, rows at even addresses
            auto takes = [](const DevTensor& t) {
                return (t.dtype == NTK_DT_Q8_0 || t.dtype == NTK_DT_Q4_K || t.dtype == NTK_DT_Q6_K) && t.in_f > 0 && t.in_f <= 0x7FFFFFFF &&
                       ntk_row_bytes(t.dtype, (int)t.in_f) != 0 && (uintptr_t)t.ptr % 2 == 0;
            };
            L.moe_gemm_ok = L.is_moe() && takes(L.gate_exps) && takes(L.up_exps) && takes(L.down_exps);
        }
    }
    if (tp_world_ > 1) {   // communication buffer: flags + two slots of one prompt's worth of hidden vectors
        tp_max_floats_ = S * H;
        tp_comm_ = ntk_tp_comm_alloc(ntk_tp_comm_bytes(tp_max_floats_));   // fine-grained: csrc/tp.hip
        if (tp_comm_) allocs_.push_back(tp_comm_);
        if (!tp_comm_ || ntk_tp_comm_reset(tp_comm_, nullptr) != NTK_OK || ntk_device_synchronize() != NTK_OK) { err_ = "communication buffer allocation failed"; return NTK_E_NOMEM; }
    }
    d_recent_ = (int*)dev_alloc(kRecentCap * 4, false);
    h_recent_ = (int*)nt_hip_malloc_host(kRecentCap * 4);
    if (!kv_.k(0) || !kv_.v(0) || !hidden_ || !residual_ || !logits_ || !workspace_ || !positions_ || !tokens_dev_ ||
        !d_pos_ || !d_token_ || !argmax_scratch_ || !h_token_ || !h_ring_) {
        err_ = "buffer allocation failed";
        return NTK_E_NOMEM;
    }
    *h_token_ = 0;
    if (rope_inv_freq_) {
        std::vector<float> f((size_t)cfg_.head_dim / 2);
        NT_TRY(rope_build_table(cfg_.head_dim, cfg_.rope_theta, rope_factors_.empty() ? nullptr : rope_factors_.data(), f.data()));
        nt_hip_memcpy_h2d(rope_inv_freq_, f.data(), f.size() * 4);
    }
    if (sequences_ > 1) { NT_TRY(batch_buffers()); NT_TRY(batch_sample_buffers()); }   // (none of it counted in kv_cache_bytes())
    // the fused single-token path's activations: the device's static slots if this model is the first to ask and fits them, else its own buffers
    hidden1_ = hidden_;
    const bool fits = H <= NTK_ARENA_HIDDEN_FLOATS && (size_t)cfg_.n_heads * cfg_.head_dim <= NTK_ARENA_ATTN_FLOATS &&
                      (size_t)cfg_.intermediate_size <= NTK_ARENA_GATE_FLOATS;
    if (static_act_ && fits && !shares_weights_ && tp_world_ == 1 && (arena_device_ = ntk_decode_arena_acquire()) >= 0) {
        arena_owner_ = true;
        hidden1_ = ntk_decode_arena_slot(NTK_ARENA_HIDDEN);
        arena_attn_ = ntk_decode_arena_slot(NTK_ARENA_ATTN_OUT);
        arena_gate_ = ntk_decode_arena_slot(NTK_ARENA_GATE);
    }
    return NTK_OK;
}

}  // namespace nt
