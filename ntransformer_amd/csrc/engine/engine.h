// engine/engine.h -- text generation loop and its statistics.
// Replaces reference src/inference/engine.{h,cpp}: Engine::load / generate / chat / benchmark / print_stats.
// The speculative and self-speculative variants (engine.cpp:150-540) depend on the tiered streaming mode
// and are out of scope.
#pragma once
#include <functional>
#include <string>
#include <vector>
#include "../../../include/ntransformer.h"
#include "model.h"
#include "sampler.h"
#include "tokenizer.h"

namespace nt {

struct GenerateConfig {   // reference engine.h:17-26, same defaults
    int max_tokens = 256;
    float temperature = 0.7f;
    int top_k = 40;
    float top_p = 0.9f;
    float repeat_penalty = 1.1f;
    int repeat_window = 64;
    uint64_t seed = 42;
    bool verbose = true;
};

struct Stats {            // reference engine.h:76-84
    int prompt_tokens = 0;
    int gen_tokens = 0;
    float prefill_ms = 0;
    float decode_ms = 0;
    float prefill_tok_s() const { return prefill_ms > 0 ? prompt_tokens / (prefill_ms / 1000.0f) : 0.0f; }
    float decode_tok_s() const { return decode_ms > 0 ? gen_tokens / (decode_ms / 1000.0f) : 0.0f; }
};

// the sampler settings of a C-API request (max_tokens / stop_at_eos are the generator's, not the sampler's)
inline SamplerConfig sampler_config(const nt_gen_params& p) {
    SamplerConfig c;
    c.temperature = p.temperature; c.top_k = p.top_k; c.top_p = p.top_p;
    c.repeat_penalty = p.repeat_penalty; c.repeat_window = p.repeat_window; c.seed = p.seed;
    return c;
}

using TokenCallback =std::function<bool(const std::string& piece, int token_id)>;

struct EngineOptions {
    bool fused = true;            // fused 5-launch/layer decode path (false: the reference's 15-launch sequence)
    bool graph = true;            // replay the fused token from a hipGraph
    bool batched_prefill = true;  // prompts: one pass over each weight matrix per 16 tokens (false: per-token GEMV loops)
    bool device_sampling = true;  // greedy argmax on the device when temperature <= 0 and repeat_penalty <= 1
    int synth_threads = 0;        // 0 = hardware concurrency
    bool context_shift = false;   // the generate loop at the end of the context: drop half of what lies behind context_keep and go on (false: stop)
    int context_keep = 1;         // leading positions a context shift never drops (the default keeps the BOS)
    bool batch_prefill = false;   // generate_batch(_ex): all prompts in ONE packed pass (Model::forward_batch) instead of one forward() per slot; read per call
};

class Engine {
public:
    int load(const std::string& path, int max_context = 4096);
    int load_synthetic(const SynthSpec& spec, int max_context = 4096);
    // a second sequence over the weights `src` holds resident (Model::share_weights): own caches, buffers and stream; `src` must outlive this engine
    int load_shared(Engine& src, int max_context = 4096);
    std::string generate(const std::string& prompt, const GenerateConfig& cfg, TokenCallback cb = nullptr);
    // the generate loop on token ids (no tokenizer, no printing): used by bench.py and the parity tests
    int generate_tokens(const std::vector<int>& prompt, const GenerateConfig& cfg, std::vector<int>& out, bool stop_at_eos);
    // n greedy decode steps continuing from (token, pos): the timed inner loop of run(), nothing else.
    int decode_greedy_steps(int token, int pos, int n, int* out);
    // log P(targets[i] | tokens[0..i]) for every position of a prompt pass at start_pos (Model::score; top1_out may be null)
    int score(const int* tokens, const int* targets, int n, int start_pos, float* logprob_out, int* top1_out);
    // n prompts generated in lockstep over the sequence slots ("sequences" option), greedy: prompt i prefilled into slot i, then one Model::decode_batch
    // per step over the sequences still alive (include/ntransformer.h: nt_engine_generate_batch)
    int generate_batch(const int* const* prompts, const int* prompt_lens, int n, const nt_gen_params& p, int* out, int out_stride, int* out_counts);
    // one batched step with every row sampled on the device by its own params[i] (include/ntransformer.h: nt_engine_decode_batch_sample)
    int decode_batch_sample(const int* slots, const int* tokens, const int* positions, int n, const nt_gen_params* params, const int* const* recent,
                            const int* n_recent, const float* r, float* logits_out, int* next_out);
    // generate_batch with per-sequence settings, sampled: one Sampler per sequence, the first token from the prefill logits on the host, then
    // Model::decode_batch_sample per step (include/ntransformer.h: nt_engine_generate_batch_ex)
    int generate_batch_ex(const int* const* prompts, const int* prompt_lens, int n, const nt_gen_params* params, int* out, int out_stride, int* out_counts);
    void chat(const GenerateConfig& cfg);
    void benchmark(const std::string& prompt, int n_tokens);
    void print_stats(const Stats& st) const;

    Model& model() { return model_; }
    const Tokenizer& tokenizer() const { return tok_; }
    const Stats& last_stats() const { return stats_; }
    EngineOptions& options() { return opt_; }
    const std::string& error() const { return err_; }
    void set_error(const std::string& e) { err_ = e; }
    bool loaded() const { return loaded_; }

private:
    int run(std::vector<int>& tokens, const GenerateConfig& cfg, std::string* text, TokenCallback cb, bool print, bool stop_at_eos);
    // The prefill of generate_batch(_ex): prompt i into slot i from position 0, row i of `logits` ([n][vocab], resized here) = its last position's logits.
    // "batch_prefill" = 1: ONE Model::forward_batch over all prompts -- unless the cache is 8-bit (that pass refuses it) or the prompts together exceed the
    // context-sized activation buffers: then, and with 0, one forward() per slot, as ever.
    int prefill_slots(const int* const* prompts, const int* prompt_lens, int n, std::vector<float>& logits);
    Model model_;
    Tokenizer tok_;
    Stats stats_;
    EngineOptions opt_;
    std::string err_;
    bool loaded_ = false;
};

}  // namespace nt
