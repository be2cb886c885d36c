// engine/capi.cpp -- C API (include/ntransformer.h).  The reference declares nt_engine_* in its public header
// but ships no implementation (reference include/ntransformer.h:15-38, SURVEY.md finding 5).
#include "../../../include/ntransformer.h"
#include "../../../include/ntk_engine.h"
#include "engine.h"

#include <cstdlib>
#include <cstring>
#include <new>
#include <thread>

using nt::Engine;

namespace {
Engine* E(nt_engine_t e) { return static_cast<Engine*>(e); }
nt::SynthSpec to_spec(const nt_synth_spec& s) {
    nt::SynthSpec o;
    o.hidden = s.hidden; o.inter = s.inter; o.layers = s.layers; o.heads = s.heads; o.kv_heads = s.kv_heads;
    o.vocab = s.vocab; o.ctx = s.ctx; o.eps = s.eps; o.theta = s.theta; o.bos = s.bos; o.eos = s.eos;
    o.mix = s.mix ? s.mix : "Q8_0";
    o.seed = s.seed;
    return o;
}
int threads_or_default(int n) {
    if (n > 0) return n;
    const int h = (int)std::thread::hardware_concurrency();
    return h > 0 ? h : 8;
}
}  // namespace

extern "C" {

nt_engine_t nt_engine_create(void) { return new (std::nothrow) Engine(); }
void nt_engine_destroy(nt_engine_t e) { delete E(e); }

int nt_engine_load(nt_engine_t e, const char* path) { return nt_engine_load_ex(e, path, 4096); }

int nt_engine_load_ex(nt_engine_t e, const char* path, int max_context) {
    if (!e || !path) return NTK_E_NULL;
    try { return E(e)->load(path, max_context > 0 ? max_context : 4096); } catch (...) { return NTK_E_NOMEM; }
}

int nt_engine_load_synthetic(nt_engine_t e, const nt_synth_spec* spec, int max_context) {
    if (!e || !spec) return NTK_E_NULL;
    try { return E(e)->load_synthetic(to_spec(*spec), max_context > 0 ? max_context : 4096); } catch (...) { return NTK_E_NOMEM; }
}

int nt_engine_load_shared(nt_engine_t e, nt_engine_t src, int max_context) {
    if (!e || !src || e == src) return NTK_E_NULL;
    try { return E(e)->load_shared(*E(src), max_context > 0 ? max_context : 4096); } catch (...) { return NTK_E_NOMEM; }
}

int nt_engine_set_option(nt_engine_t e, const char* key, const char* value) {
    if (!e || !key || !value) return NTK_E_NULL;
    const bool on = atoi(value) != 0;
    const std::string k = key;
    // an option that shapes the load: refused afterwards, and the model's own refusal becomes the engine's error
    auto before_load = [&](auto set) -> int {
        if (E(e)->loaded()) { E(e)->set_error(k + " must be set before the model is loaded"); return NTK_E_SHAPE; }
        const int rc = set();
        if (rc != NTK_OK) E(e)->set_error(E(e)->model().error());
        return rc;
    };
    if (k == "fused") E(e)->options().fused = on;
    else if (k == "graph") E(e)->options().graph = on;
    else if (k == "batched_prefill") { E(e)->options().batched_prefill = on; E(e)->model().set_batched_prefill(on); }
    else if (k == "device_sampling") E(e)->options().device_sampling = on;
    else if (k == "f16_prefill" || k == "bf16_prefill") E(e)->model().set_bf16_prefill(on);   // (the round-2 name stays accepted)
    else if (k == "dense_fused") {   // "1" (default) | "0": F16 / BF16 matrices on the fused decode GEMV and the batched prompt GEMM, or the 1:1 launchers; any time
        const std::string v = value;
        if (v != "0" && v != "1") { E(e)->set_error("dense_fused must be 0 or 1"); return NTK_E_SHAPE; }
        return E(e)->model().set_dense_fused(on);
    }
    else if (k == "dense_mfma16") {   // "1" (default) | "0": the prompt pass's F16 / BF16 matrices on the 16-bit matrix cores, or the F32-MFMA form; any time (the A/B switch)
        const std::string v = value;
        if (v != "0" && v != "1") { E(e)->set_error("dense_mfma16 must be 0 or 1"); return NTK_E_SHAPE; }
        E(e)->model().set_dense_mfma16(on);
    }
    else if (k == "moe_gemm") {   // "1" (default) | "0": prompt passes over mixture-of-experts layers on the grouped matrix-core GEMM, or the expert GEMV at every row count; any time (the A/B switch)
        const std::string v = value;
        if (v != "0" && v != "1") { E(e)->set_error("moe_gemm must be 0 or 1"); return NTK_E_SHAPE; }
        E(e)->model().set_moe_gemm(on);
    }
    else if (k == "moe_gemm_min_rows") {   // 1 .. 1024: the rows of a pass from which the grouped GEMM is taken (default: the measured threshold, Model::kMoeGemmMinRows); any time
        char* end = nullptr;
        const long n = strtol(value, &end, 10);
        if (end == value || *end != 0 || n < 1 || n > 1024) { E(e)->set_error("moe_gemm_min_rows must be an integer 1 .. 1024"); return NTK_E_SHAPE; }
        return E(e)->model().set_moe_gemm_min_rows((int)n);
    }
    else if (k == "persistent" || k == "fuse_attention") {   // accepted and without effect: the structures they selected were retired
        if (on) fprintf(stderr, "note: \"%s\" selected an experiment that lost to the fused launches and was removed (profiles/NEGATIVE_RESULTS.md); the option does nothing\n", key);
    }
    else if (k == "kv_cache") return before_load([&] { return E(e)->model().set_kv_cache(value); });   // "f16" (default) | "q8_0": before the load only
    else if (k == "rope_scaling") return before_load([&] { return E(e)->model().set_rope_scaling(value); });   // file (default) | none | linear:<f> | llama3:<f>,<low>,<high>,<ctx>: before the load only (model.h)
    else if (k == "rope_freq_base") return before_load([&] { return E(e)->model().set_rope_freq_base(value); });   // theta > 0, overriding the file's
    else if (k == "rope_freq_scale") return before_load([&] { return E(e)->model().set_rope_freq_scale(value); });   // the linear scale > 0, overriding the file's
    else if (k == "sequences") return before_load([&] { return E(e)->model().set_sequences(atoi(value)); });   // "1" .. "16" sequence slots: before the load only
    else if (k == "batch_kv_q8") {   // "0" (default) | "1": sequence slots and the batched step over the 8-bit cache; before the load only (model.h)
        const std::string v = value;
        if (v != "0" && v != "1") { E(e)->set_error("batch_kv_q8 must be 0 or 1"); return NTK_E_SHAPE; }
        return before_load([&] { return E(e)->model().set_batch_kv_q8(on); });
    }
    else if (k == "static_activations") {   // "1" (default) | "0": the fused single-token path's activations in the library's static slots; before the load only (model.h)
        const std::string v = value;
        if (v != "0" && v != "1") { E(e)->set_error("static_activations must be 0 or 1"); return NTK_E_SHAPE; }
        return before_load([&] { return E(e)->model().set_static_activations(on); });
    }
    else if (k == "batch_prefill") {   // "0" (default) | "1": nt_engine_generate_batch / _ex prefill all prompts in one packed pass; any time, read per call
        const std::string v = value;
        if (v != "0" && v != "1") { E(e)->set_error("batch_prefill must be 0 or 1"); return NTK_E_SHAPE; }
        E(e)->options().batch_prefill = on;
    }
    else if (k == "context_shift") {   // "0" (default) | "1": the generate loop shifts slot 0 at the end of the context instead of stopping; any time
        const std::string v = value;
        if (v != "0" && v != "1") { E(e)->set_error("context_shift must be 0 or 1"); return NTK_E_SHAPE; }
        E(e)->options().context_shift = on;
    }
    else if (k == "context_keep") {   // N >= 0 (default 1): leading positions a context shift never drops; any time
        char* end = nullptr;
        const long n = strtol(value, &end, 10);
        if (end == value || *end != 0 || n < 0 || n > 0x7FFFFFFF) { E(e)->set_error("context_keep must be an integer >= 0"); return NTK_E_SHAPE; }
        E(e)->options().context_keep = (int)n;
    }
    else if (k == "prefill_row_max") E(e)->model().set_prefill_row_max(on);   // 1 (default): see Model::prefill_row_max_
    else if (k == "prefill_fused_split") E(e)->model().set_prefill_fused_split(on);   // 1 (default): see Model::prefill_fused_split_
    else if (k == "attention_merge") return E(e)->model().set_attention_merge(on);   // 1: split-KV attention without the combine launch (default 0: measured slower)
    else if (k == "repack") return E(e)->model().set_repack(atoi(value));   // 0 raw path, 1 repack + GGUF bytes resident, 2 one resident copy (Q8_0 matrices keep both: model.h), 3 (default): 2
    else if (k == "score_rows") {   // rows of logits per LM-head chunk of nt_engine_score_tokens, 1 .. 1024 (default 256)
        const int rc = E(e)->model().set_score_rows(atoi(value));
        if (rc != NTK_OK) E(e)->set_error(E(e)->model().error());
        return rc;
    }
    else if (k == "synth_threads") E(e)->options().synth_threads = atoi(value);
    else return NTK_E_SHAPE;
    return NTK_OK;
}

const char* nt_engine_last_error(nt_engine_t e) { return e ? E(e)->error().c_str() : "null engine"; }

void nt_gen_params_default(nt_gen_params* p) {
    if (!p) return;
    const nt::GenerateConfig d;
    p->max_tokens = d.max_tokens; p->temperature = d.temperature; p->top_k = d.top_k; p->top_p = d.top_p;
    p->repeat_penalty = d.repeat_penalty; p->repeat_window = d.repeat_window; p->seed = d.seed; p->stop_at_eos = 1;
}

char* nt_engine_generate(nt_engine_t e, const char* prompt, int max_tokens, float temperature, int top_k, float top_p) {
    if (!e || !prompt || !E(e)->loaded()) return nullptr;
    try {
        nt::GenerateConfig c;
        c.max_tokens = max_tokens; c.temperature = temperature; c.top_k = top_k; c.top_p = top_p;
        c.verbose = false;
        const std::string out = E(e)->generate(prompt, c);
        char* r = static_cast<char*>(malloc(out.size() + 1));
        if (!r) return nullptr;
        memcpy(r, out.c_str(), out.size() + 1);
        return r;
    } catch (...) { return nullptr; }
}
void nt_free(char* p) { free(p); }

int nt_engine_vocab_size(nt_engine_t e) { return e && E(e)->loaded() ? E(e)->model().config().vocab_size : -1; }
int nt_engine_n_layers(nt_engine_t e) { return e && E(e)->loaded() ? E(e)->model().config().n_layers : -1; }
int nt_engine_hidden_size(nt_engine_t e) { return e && E(e)->loaded() ? E(e)->model().config().hidden_size : -1; }
int nt_engine_max_context(nt_engine_t e) { return e && E(e)->loaded() ? E(e)->model().config().max_seq_len : -1; }

int nt_engine_generate_tokens(nt_engine_t e, const int* prompt, int n_prompt, const nt_gen_params* p, int* out, int out_cap) {
    if (!e || !prompt || !p || (!out && out_cap > 0)) return NTK_E_NULL;
    if (n_prompt <= 0) return NTK_E_SHAPE;
    try {
        nt::GenerateConfig c;
        c.max_tokens = p->max_tokens; c.temperature = p->temperature; c.top_k = p->top_k; c.top_p = p->top_p;
        c.repeat_penalty = p->repeat_penalty; c.repeat_window = p->repeat_window; c.seed = p->seed;
        std::vector<int> gen;
        const int rc = E(e)->generate_tokens(std::vector<int>(prompt, prompt + n_prompt), c, gen, p->stop_at_eos != 0);
        if (rc != NTK_OK) return rc;
        const int n = (int)std::min<size_t>(gen.size(), (size_t)out_cap);
        for (int i = 0; i < n; ++i) out[i] = gen[i];
        return n;
    } catch (...) { return NTK_E_NOMEM; }
}

int nt_engine_last_stats(nt_engine_t e, nt_stats* o) {
    if (!e || !o) return NTK_E_NULL;
    const nt::Stats& s = E(e)->last_stats();
    o->prompt_tokens = s.prompt_tokens; o->gen_tokens = s.gen_tokens; o->prefill_ms = s.prefill_ms;
    o->decode_ms = s.decode_ms; o->decode_tok_s = s.decode_tok_s();
    return NTK_OK;
}

int nt_engine_forward(nt_engine_t e, const int* tokens, int n, int start_pos, float* logits_out) {
    if (!e || !tokens || !logits_out) return NTK_E_NULL;
    if (!E(e)->loaded()) return NTK_E_NULL;
    float* d = E(e)->model().forward(tokens, n, start_pos);
    if (!d) return NTK_E_LAUNCH;
    return E(e)->model().copy_logits(logits_out);
}

int nt_engine_seq_forward(nt_engine_t e, int slot, const int* tokens, int n, int start_pos, float* logits_out) {
    if (!e || !tokens || !logits_out) return NTK_E_NULL;
    if (!E(e)->loaded()) return NTK_E_NULL;
    if (slot < 0 || slot >= E(e)->model().sequences()) { E(e)->set_error("seq_forward: no such sequence slot"); return NTK_E_SHAPE; }
    float* d = E(e)->model().forward(tokens, n, start_pos, slot);
    if (!d) { E(e)->set_error(E(e)->model().error()); return NTK_E_LAUNCH; }
    return E(e)->model().copy_logits(logits_out);
}

int nt_engine_decode_batch(nt_engine_t e, const int* slots, const int* tokens, const int* positions, int n, float* logits_out, int* next_out) {
    if (!e || !E(e)->loaded()) return NTK_E_NULL;
    try {
        const int rc = E(e)->model().decode_batch(slots, tokens, positions, n, logits_out, next_out);
        if (rc != NTK_OK) E(e)->set_error(E(e)->model().error());
        return rc;
    } catch (...) { return NTK_E_NOMEM; }
}

int nt_engine_forward_batch(nt_engine_t e, const int* slots, const int* tokens, const int* lens, const int* start_pos, int n, float* logits_out,
                            int* next_out) {
    if (!e || !E(e)->loaded()) return NTK_E_NULL;
    try {
        E(e)->model().set_batched_prefill(E(e)->options().batched_prefill);
        const int rc = E(e)->model().forward_batch(slots, tokens, lens, start_pos, n, logits_out, next_out);
        if (rc != NTK_OK) E(e)->set_error(E(e)->model().error());
        return rc;
    } catch (...) { return NTK_E_NOMEM; }
}

int nt_forward_batch_validate(const int* slots, const int* lens, const int* start_pos, int n, int sequences, int max_seq) {
    return nt::Model::validate_forward_batch(slots, lens, start_pos, n, sequences, max_seq, nullptr);   // host only
}

int nt_engine_generate_batch(nt_engine_t e, const int* const* prompts, const int* prompt_lens, int n, const nt_gen_params* p, int* out, int out_stride,
                             int* out_counts) {
    if (!e || !prompts || !prompt_lens || !p || !out || !out_counts) return NTK_E_NULL;
    try { return E(e)->generate_batch(prompts, prompt_lens, n, *p, out, out_stride, out_counts); } catch (...) { return NTK_E_NOMEM; }
}

int nt_engine_decode_batch_sample(nt_engine_t e, const int* slots, const int* tokens, const int* positions, int n, const nt_gen_params* params,
                                  const int* const* recent, const int* n_recent, const float* r, float* logits_out, int* next_out) {
    if (!e || !E(e)->loaded()) return NTK_E_NULL;
    try { return E(e)->decode_batch_sample(slots, tokens, positions, n, params, recent, n_recent, r, logits_out, next_out); } catch (...) { return NTK_E_NOMEM; }
}

int nt_engine_generate_batch_ex(nt_engine_t e, const int* const* prompts, const int* prompt_lens, int n, const nt_gen_params* params, int* out, int out_stride,
                                int* out_counts) {
    if (!e || !prompts || !prompt_lens || !params || !out || !out_counts) return NTK_E_NULL;
    try { return E(e)->generate_batch_ex(prompts, prompt_lens, n, params, out, out_stride, out_counts); } catch (...) { return NTK_E_NOMEM; }
}

int nt_engine_kv_shift(nt_engine_t e, int slot, int keep, int discard, int n_past) {
    if (!e || !E(e)->loaded()) return NTK_E_NULL;
    try {
        const int rc = E(e)->model().kv_shift(slot, keep, discard, n_past);
        if (rc < 0) E(e)->set_error(E(e)->model().error());
        return rc;
    } catch (...) { return NTK_E_NOMEM; }
}

int nt_engine_kv_copy(nt_engine_t e, int src_slot, int dst_slot, int pos0, int n) {
    if (!e || !E(e)->loaded()) return NTK_E_NULL;
    try {
        const int rc = E(e)->model().kv_copy(src_slot, dst_slot, pos0, n);
        if (rc < 0) E(e)->set_error(E(e)->model().error());
        return rc;
    } catch (...) { return NTK_E_NOMEM; }
}

int nt_kv_shift_validate(int slot, int keep, int discard, int n_past, int sequences, int max_seq) {
    return nt::Model::validate_kv_shift(slot, keep, discard, n_past, sequences, max_seq, nullptr);   // host only
}
int nt_kv_copy_validate(int src_slot, int dst_slot, int pos0, int n, int sequences, int max_seq) {
    return nt::Model::validate_kv_copy(src_slot, dst_slot, pos0, n, sequences, max_seq, nullptr);   // host only
}
int nt_context_shift_discard(int n_past, int keep) { return nt::Model::context_shift_discard(n_past, keep); }

int nt_batch_validate(const int* slots, const int* tokens, const int* positions, int n, int sequences, int max_seq, int vocab) {
    return nt::Model::validate_batch(slots, tokens, positions, n, sequences, max_seq, vocab, nullptr);   // host only
}

int nt_engine_score_tokens(nt_engine_t e, const int* tokens, const int* targets, int n, int start_pos, float* logprob_out, int* top1_out) {
    if (!e || !tokens || !targets || !logprob_out) return NTK_E_NULL;
    try {
        const int rc = E(e)->score(tokens, targets, n, start_pos, logprob_out, top1_out);
        if (rc != NTK_OK) return rc;
        int scored = 0;
        for (int i = 0; i < n; ++i) scored += targets[i] >= 0;
        return scored;
    } catch (...) { return NTK_E_NOMEM; }
}

int nt_engine_decode_fused(nt_engine_t e, int token, int pos, int use_graph, float* logits_out) {
    if (!e || !logits_out || !E(e)->loaded()) return NTK_E_NULL;
    nt::Model& m = E(e)->model();
    if (pos < 0 || pos >= m.config().max_seq_len) return NTK_E_SHAPE;
    m.set_device_pos(pos);
    int rc = m.set_device_token(token);
    if (rc != NTK_OK) return rc;
    rc = m.decode_step_fused(false, use_graph != 0);
    if (rc != NTK_OK) return rc;
    rc = m.copy_logits(logits_out);
    if (rc != NTK_OK) return rc;
    return m.check_tp();   // the tensor-parallel exchange's bounded wait that gave up invalidates the result
}

int nt_engine_debug_run_layers(nt_engine_t e, const float* hidden_in, int n_tokens, int start_pos, int first_layer, int n_layers, int mode,
                               float* hidden_out) {
    if (!e || !E(e)->loaded()) return NTK_E_NULL;
    return E(e)->model().debug_run_layers(hidden_in, n_tokens, start_pos, first_layer, n_layers, mode, hidden_out);
}
int nt_engine_debug_kv_read(nt_engine_t e, int layer, int pos0, int n, uint16_t* k_out, uint16_t* v_out) {
    if (!e || !E(e)->loaded()) return NTK_E_NULL;
    return E(e)->model().debug_kv(layer, pos0, n, k_out, v_out, false);
}
int nt_engine_debug_kv_read_slot(nt_engine_t e, int slot, int layer, int pos0, int n, uint16_t* k_out, uint16_t* v_out) {
    if (!e || !E(e)->loaded()) return NTK_E_NULL;
    return E(e)->model().debug_kv(layer, pos0, n, k_out, v_out, false, slot);
}
int nt_engine_debug_kv_write(nt_engine_t e, int layer, int pos0, int n, const uint16_t* k, const uint16_t* v) {
    if (!e || !E(e)->loaded()) return NTK_E_NULL;
    return E(e)->model().debug_kv(layer, pos0, n, const_cast<uint16_t*>(k), const_cast<uint16_t*>(v), true);
}
int nt_engine_debug_kv_write_slot(nt_engine_t e, int slot, int layer, int pos0, int n, const uint16_t* k, const uint16_t* v) {
    if (!e || !E(e)->loaded()) return NTK_E_NULL;
    return E(e)->model().debug_kv(layer, pos0, n, const_cast<uint16_t*>(k), const_cast<uint16_t*>(v), true, slot);
}
int nt_engine_debug_kv_inputs_capture(nt_engine_t e, int layer) {
    if (!e || !E(e)->loaded()) return NTK_E_NULL;
    return E(e)->model().debug_kv_inputs_capture(layer);
}
int nt_engine_debug_kv_inputs_read(nt_engine_t e, int n, float* k_out, float* v_out) {
    if (!e || !E(e)->loaded()) return NTK_E_NULL;
    return E(e)->model().debug_kv_inputs_read(n, k_out, v_out);
}
int nt_engine_debug_kv_read_q8(nt_engine_t e, int layer, int pos0, int n, void* k_blocks, void* v_blocks) {
    if (!e || !E(e)->loaded()) return NTK_E_NULL;
    return E(e)->model().debug_kv_q8(layer, pos0, n, static_cast<uint8_t*>(k_blocks), static_cast<uint8_t*>(v_blocks), false);
}
int nt_engine_debug_kv_write_q8(nt_engine_t e, int layer, int pos0, int n, const void* k_blocks, const void* v_blocks) {
    if (!e || !E(e)->loaded()) return NTK_E_NULL;
    return E(e)->model().debug_kv_q8(layer, pos0, n, static_cast<uint8_t*>(const_cast<void*>(k_blocks)), static_cast<uint8_t*>(const_cast<void*>(v_blocks)), true);
}
int nt_engine_debug_kv_read_q8_slot(nt_engine_t e, int slot, int layer, int pos0, int n, void* k_blocks, void* v_blocks) {
    if (!e || !E(e)->loaded()) return NTK_E_NULL;
    return E(e)->model().debug_kv_q8(layer, pos0, n, static_cast<uint8_t*>(k_blocks), static_cast<uint8_t*>(v_blocks), false, slot);
}
int nt_engine_debug_kv_write_q8_slot(nt_engine_t e, int slot, int layer, int pos0, int n, const void* k_blocks, const void* v_blocks) {
    if (!e || !E(e)->loaded()) return NTK_E_NULL;
    return E(e)->model().debug_kv_q8(layer, pos0, n, static_cast<uint8_t*>(const_cast<void*>(k_blocks)), static_cast<uint8_t*>(const_cast<void*>(v_blocks)), true, slot);
}

const char* nt_engine_decode_path(nt_engine_t e) { return e && E(e)->loaded() ? E(e)->model().decode_path() : ""; }

// ---- tensor parallelism (one engine per rank; csrc/tp.hip) ---------------------------------------------------------------
int nt_engine_tp_configure(nt_engine_t e, int rank, int world) { return e ? E(e)->model().tp_configure(rank, world) : NTK_E_NULL; }
int nt_engine_tp_export(nt_engine_t e, void* handle64, void** raw) {
    if (!e || !E(e)->loaded()) return NTK_E_NULL;
    return E(e)->model().tp_export(handle64, raw);
}
int nt_engine_tp_connect(nt_engine_t e, const void* handles, void* const* raws) {
    if (!e || !E(e)->loaded()) return NTK_E_NULL;
    return E(e)->model().tp_connect(handles, raws);
}
unsigned nt_engine_tp_error(nt_engine_t e) { return e && E(e)->loaded() ? E(e)->model().tp_error() : 0u; }
int nt_tp_slice_columns(void* dst, const void* src, int dtype, int64_t out_features, int64_t in_features, int rank, int world) {
    return nt::Model::slice_columns(dst, src, dtype, out_features, in_features, rank, world);   // host only
}

int nt_engine_decode_greedy_steps(nt_engine_t e, int token, int pos, int n, int* out) {
    if (!e || !E(e)->loaded()) return NTK_E_NULL;
    return E(e)->decode_greedy_steps(token, pos, n, out);
}

int nt_engine_profile_token(nt_engine_t e, int token, int pos, int coarse, float* ms4, int* calls4) {
    if (!e || !ms4 || !calls4 || !E(e)->loaded()) return NTK_E_NULL;
    nt::Model& m = E(e)->model();
    if (pos < 0 || pos >= m.config().max_seq_len) return NTK_E_SHAPE;
    m.set_device_pos(pos);
    const int rc = m.set_device_token(token);
    if (rc != NTK_OK) return rc;
    return m.profile_token(ms4, calls4, coarse != 0);
}

int nt_engine_tokenize(nt_engine_t e, const char* text, int add_bos, int* out, int cap) {
    if (!e || !text || !E(e)->loaded()) return NTK_E_NULL;
    const std::vector<int> ids = E(e)->tokenizer().encode(text, add_bos != 0);
    for (int i = 0; i < (int)ids.size() && i < cap; ++i) out[i] = ids[i];
    return (int)ids.size();
}

int nt_engine_detokenize(nt_engine_t e, const int* ids, int n, char* out, int cap) {
    if (!e || !ids || !E(e)->loaded()) return NTK_E_NULL;
    const std::string s = E(e)->tokenizer().decode(std::vector<int>(ids, ids + n));
    if (out && cap > 0) {
        const size_t k = std::min<size_t>(s.size(), (size_t)cap - 1);
        memcpy(out, s.data(), k);
        out[k] = 0;
    }
    return (int)s.size();
}

uint64_t nt_engine_bytes_per_token(nt_engine_t e, int pos) { return e && E(e)->loaded() ? E(e)->model().bytes_per_token(pos) : 0; }
uint64_t nt_engine_kv_cache_bytes(nt_engine_t e) { return e && E(e)->loaded() ? E(e)->model().kv_cache_bytes() : 0; }
uint64_t nt_engine_weight_bytes(nt_engine_t e) { return e && E(e)->loaded() ? E(e)->model().weight_bytes() : 0; }
uint64_t nt_engine_resident_weight_bytes(nt_engine_t e) { return e && E(e)->loaded() ? E(e)->model().resident_weight_bytes() : 0; }
uint64_t nt_engine_repacked_bytes(nt_engine_t e) { return e && E(e)->loaded() ? E(e)->model().repack_bytes() : 0; }

int nt_synth_write_gguf(const char* path, const nt_synth_spec* spec, int nthreads) {
    if (!path || !spec) return NTK_E_NULL;
    try { return nt::synth_write_gguf(path, to_spec(*spec), threads_or_default(nthreads)); } catch (...) { return NTK_E_NOMEM; }
}

int64_t nt_synth_tensor(const nt_synth_spec* spec, const char* name, void* dst, size_t cap, int nthreads) {
    if (!spec || !name) return NTK_E_NULL;
    std::vector<nt::SynthTensor> plan;
    const nt::SynthSpec s = to_spec(*spec);
    if (!nt::synth_plan(s, plan)) return NTK_E_SHAPE;
    for (const auto& t : plan) {
        if (t.name != name) continue;
        if (!dst) return (int64_t)t.nbytes;
        if (cap < t.nbytes) return NTK_E_SHAPE;
        nt::synth_fill(dst, t, s.seed, threads_or_default(nthreads));
        return (int64_t)t.nbytes;
    }
    return NTK_E_FORMAT;
}

// ---- host-only entry points --------------------------------------------------------------------------
static void json_escape(std::string& o, const std::string& s) {
    for (unsigned char c : s) {
        if (c == '"' || c == '\\') { o.push_back('\\'); o.push_back((char)c); }
        else if (c < 0x20) { char b[8]; snprintf(b, sizeof b, "\\u%04x", c); o += b; }
        else o.push_back((char)c);
    }
}

int nt_gguf_describe(const char* path, char* out, int cap) {
    if (!path) return NTK_E_NULL;
    try {
        nt::GgufFile f;
        const int st = f.open(path);
        if (st != NTK_OK) return st;
        const nt::ModelConfig& c = f.config();
        std::string j = "{";
        char b[512];
        snprintf(b, sizeof b,
                 "\"version\":%u,\"data_offset\":%zu,\"vocab_size\":%d,\"hidden_size\":%d,\"intermediate_size\":%d,"
                 "\"n_layers\":%d,\"n_heads\":%d,\"n_kv_heads\":%d,\"head_dim\":%d,\"max_seq_len\":%d,\"norm_eps\":%.9g,"
                 "\"rope_theta\":%.9g,\"bos\":%d,\"eos\":%d,\"n_vocab_tokens\":%zu,\"n_scores\":%zu,\"n_token_types\":%zu,",
                 f.version(), f.data_offset(), c.vocab_size, c.hidden_size, c.intermediate_size, c.n_layers, c.n_heads,
                 c.n_kv_heads, c.head_dim, c.max_seq_len, (double)c.norm_eps, (double)c.rope_theta, c.bos_token_id,
                 c.eos_token_id, f.vocab().tokens.size(), f.vocab().scores.size(), f.vocab().token_types.size());
        j += b;
        snprintf(b, sizeof b, "\"rope_freq_scale\":%.9g,\"rope_factors\":%d,\"rope_orig_ctx\":%d,\"rope_scaling_type\":\"", (double)c.rope_freq_scale, c.rope_factors,
                 c.rope_orig_ctx);
        j += b;
        json_escape(j, c.rope_scaling_type);
        j += "\",";
        int n_bias = 0, n_qk_norm = 0, n_moe = 0;   // blk.<i>.attn_{q,k,v}.bias; blk.<i>.attn_{q,k}_norm.weight; blk.<i>.ffn_gate_inp.weight (the router of a mixture-of-experts layer)
        for (const auto& t : f.tensors()) {
            int li = -1, at = 0;
            if (sscanf(t.name.c_str(), "blk.%d.%n", &li, &at) != 1 || at == 0) continue;
            const std::string rest = t.name.substr((size_t)at);
            n_bias += rest == "attn_q.bias" || rest == "attn_k.bias" || rest == "attn_v.bias";
            n_qk_norm += rest == "attn_q_norm.weight" || rest == "attn_k_norm.weight";
            n_moe += rest == "ffn_gate_inp.weight";
        }
        j += "\"expert_count\":" + std::to_string(c.expert_count) + ",\"expert_used_count\":" + std::to_string(c.expert_used_count) + ",";
        j += "\"expert_feed_forward_length\":" + std::to_string(c.expert_ff_length) + ",\"moe_layers\":" + std::to_string(n_moe) + ",";
        j += "\"qkv_bias_tensors\":" + std::to_string(n_bias) + ",";
        j += "\"qk_norm_tensors\":" + std::to_string(n_qk_norm) + ",";
        j += "\"architecture\":\""; json_escape(j, c.architecture); j += "\",\"name\":\""; json_escape(j, c.model_name);
        j += "\",\"tensors\":[";
        bool first = true;
        for (const auto& t : f.tensors()) {
            if (!first) j += ",";
            first = false;
            j += "{\"name\":\""; json_escape(j, t.name); j += "\",\"dims\":[";
            for (size_t d = 0; d < t.dims.size(); ++d) { if (d) j += ","; j += std::to_string(t.dims[d]); }
            snprintf(b, sizeof b, "],\"ggml_type\":%u,\"dtype\":%d,\"type\":\"%s\",\"offset\":%llu,\"nbytes\":%zu}", t.ggml_type, t.dtype,
                     t.known_type ? nt::dtype_name(t.dtype) : "UNKNOWN", (unsigned long long)t.offset, t.nbytes);
            j += b;
        }
        j += "]}";
        if (out && cap > 0) {
            const size_t k = std::min<size_t>(j.size(), (size_t)cap - 1);
            memcpy(out, j.data(), k);
            out[k] = 0;
        }
        return (int)j.size();
    } catch (...) { return NTK_E_NOMEM; }
}

int nt_engine_rope_info(nt_engine_t e, char* out, int cap) {
    if (!e || !E(e)->loaded()) return NTK_E_NULL;
    try {
        const nt::ModelConfig& c = E(e)->model().config();
        char b[256];
        snprintf(b, sizeof b, "{\"rope_theta\":%.9g,\"rope_freq_scale\":%.9g,\"rope_factors\":%d,\"rope_orig_ctx\":%d,\"rope_scaling_type\":\"", (double)c.rope_theta,
                 (double)c.rope_freq_scale, c.rope_factors, c.rope_orig_ctx);
        std::string j = b;
        json_escape(j, c.rope_scaling_type);
        j += "\"}";
        if (out && cap > 0) {
            const size_t k = std::min<size_t>(j.size(), (size_t)cap - 1);
            memcpy(out, j.data(), k);
            out[k] = 0;
        }
        return (int)j.size();
    } catch (...) { return NTK_E_NOMEM; }
}

int nt_engine_qkv_bias(nt_engine_t e) { return e && E(e)->loaded() ? E(e)->model().qkv_bias_layers() : -1; }
int nt_engine_qk_norm(nt_engine_t e) { return e && E(e)->loaded() ? E(e)->model().qk_norm_layers() : -1; }
int nt_engine_moe(nt_engine_t e, int* experts, int* used) {
    if (!e || !E(e)->loaded()) return -1;
    const nt::Model& m = E(e)->model();
    const int n = m.moe_layers();
    if (experts) *experts = n ? m.config().expert_count : 0;
    if (used) *used = n ? m.config().expert_used_count : 0;
    return n;
}

int nt_rope_llama3_factors(int head_dim, float theta, float factor, float low_freq_factor, float high_freq_factor, int orig_ctx, float* out) {
    return nt::rope_llama3_factors(head_dim, theta, factor, low_freq_factor, high_freq_factor, orig_ctx, out);   // host only
}
int nt_rope_build_table(int head_dim, float theta, const float* factors_or_null, float* out) {
    return nt::rope_build_table(head_dim, theta, factors_or_null, out);   // host only
}

nt_tokenizer_t nt_tokenizer_open(const char* path) {
    if (!path) return nullptr;
    try {
        nt::GgufFile f;
        if (f.open(path) != NTK_OK) return nullptr;
        auto* t = new nt::Tokenizer();
        t->init(f.vocab(), f.config().bos_token_id, f.config().eos_token_id);
        return t;
    } catch (...) { return nullptr; }
}
void nt_tokenizer_close(nt_tokenizer_t t) { delete static_cast<nt::Tokenizer*>(t); }
int nt_tokenizer_encode(nt_tokenizer_t t, const char* text, int len, int add_bos, int* out, int cap) {
    if (!t || !text) return NTK_E_NULL;
    const std::vector<int> ids = static_cast<nt::Tokenizer*>(t)->encode(std::string(text, len < 0 ? strlen(text) : (size_t)len), add_bos != 0);
    for (int i = 0; i < (int)ids.size() && i < cap; ++i) out[i] = ids[i];
    return (int)ids.size();
}
int nt_tokenizer_decode(nt_tokenizer_t t, const int* ids, int n, char* out, int cap) {
    if (!t || !ids) return NTK_E_NULL;
    const std::string s = static_cast<nt::Tokenizer*>(t)->decode(std::vector<int>(ids, ids + n));
    if (out && cap > 0) {
        const size_t k = std::min<size_t>(s.size(), (size_t)cap - 1);
        memcpy(out, s.data(), k);
        out[k] = 0;
    }
    return (int)s.size();
}
int nt_tokenizer_is_gpt2(nt_tokenizer_t t) { return t && static_cast<nt::Tokenizer*>(t)->gpt2_mode() ? 1 : 0; }

int nt_sampler_draw(const float* logits, int n, const nt_gen_params* p, const int* recent, int n_recent, int n_draws, int* out) {
    if (!logits || !p || !out || n <= 0) return NTK_E_NULL;
    nt::Sampler s;
    s.init(nt::sampler_config(*p));
    std::vector<int> rec(recent ? recent : nullptr, recent ? recent + n_recent : nullptr);
    std::vector<float> l(n);
    for (int d = 0; d < n_draws; ++d) {
        std::copy(logits, logits + n, l.begin());
        s.apply_repeat_penalty(l.data(), n, rec);
        out[d] = s.sample(l.data(), n);
        rec.push_back(out[d]);
    }
    return n_draws;
}

// draw number `skip` of that stream on its own: the generator advanced past `skip` draws, then one penalty + sample on the caller's window
int nt_sampler_draw_nth(const float* logits, int n, const nt_gen_params* p, const int* recent, int n_recent, int skip, int* out) {
    if (!logits || !p || !out || n <= 0 || (n_recent > 0 && !recent)) return NTK_E_NULL;
    if (skip < 0 || n_recent < 0) return NTK_E_SHAPE;
    nt::Sampler s;
    s.init(nt::sampler_config(*p));
    for (int d = 0; d < skip; ++d) (void)s.draw();
    const std::vector<int> rec(recent, recent + n_recent);
    std::vector<float> l(logits, logits + n);
    s.apply_repeat_penalty(l.data(), n, rec);
    *out = s.sample(l.data(), n);
    return NTK_OK;
}

// the uniform draws Sampler::sample takes from std::mt19937(seed), in order (one per sampled token): lets a test (or an embedder
// running ntk_sample_top_k itself) stay in step with the host sampler
int nt_sampler_uniforms(uint64_t seed, int n, float* out) {
    if (!out || n < 0) return NTK_E_NULL;
    nt::Sampler s;
    nt::SamplerConfig c;
    c.seed = seed;
    s.init(c);
    for (int i = 0; i < n; ++i) out[i] = s.draw();
    return n;
}

}  // extern "C"
