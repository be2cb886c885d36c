// engine/engine.cpp -- see engine.h
#include "engine.h"
#include "../../../include/ntk_engine.h"

#include <chrono>
#include <cstdio>
#include <iostream>
#include <thread>

namespace nt {

using Clock = std::chrono::high_resolution_clock;
static float ms_since(Clock::time_point t0) { return std::chrono::duration<float, std::milli>(Clock::now() - t0).count(); }

int Engine::load(const std::string& path, int max_context) {
    loaded_ = false;
    const int st = model_.load(path, max_context);
    if (st != NTK_OK) { err_ = model_.error(); return st; }
    tok_.init(model_.vocab(), model_.config().bos_token_id, model_.config().eos_token_id);   // engine.cpp:21
    loaded_ = true;
    return NTK_OK;
}

int Engine::load_synthetic(const SynthSpec& spec, int max_context) {
    loaded_ = false;
    int nt = opt_.synth_threads > 0 ? opt_.synth_threads : (int)std::thread::hardware_concurrency();
    const int st = model_.load_synthetic(spec, max_context, nt > 0 ? nt : 8);
    if (st != NTK_OK) { err_ = model_.error(); return st; }
    tok_.init(model_.vocab(), model_.config().bos_token_id, model_.config().eos_token_id);
    loaded_ = true;
    return NTK_OK;
}

int Engine::load_shared(Engine& src, int max_context) {
    loaded_ = false;
    if (!src.loaded_) { err_ = "load_shared: the source engine is not loaded"; return NTK_E_NULL; }
    const int st = model_.share_weights(src.model_, max_context);
    if (st != NTK_OK) { err_ = model_.error(); return st; }
    tok_.init(model_.vocab(), model_.config().bos_token_id, model_.config().eos_token_id);
    loaded_ = true;
    return NTK_OK;
}

int Engine::prefill_slots(const int* const* prompts, const int* prompt_lens, int n, std::vector<float>& logits) {
    const size_t V = (size_t)model_.config().vocab_size;
    logits.resize((size_t)n * V);
    long long total = 0;
    for (int i = 0; i < n; ++i) total += prompt_lens[i];
    if (opt_.batch_prefill && !model_.kv_q8() && total <= model_.config().max_seq_len) {
        std::vector<int> flat, slots(n), starts(n, 0);
        flat.reserve((size_t)total);
        for (int i = 0; i < n; ++i) { slots[i] = i; flat.insert(flat.end(), prompts[i], prompts[i] + prompt_lens[i]); }
        const int rc = model_.forward_batch(slots.data(), flat.data(), prompt_lens, starts.data(), n, logits.data(), nullptr);
        if (rc != NTK_OK) err_ = model_.error();
        return rc;
    }
    for (int i = 0; i < n; ++i) {   // slot by slot
        if (!model_.forward(prompts[i], prompt_lens[i], 0, i)) { err_ = model_.error(); return NTK_E_LAUNCH; }
        if (model_.copy_logits(logits.data() + (size_t)i * V) != NTK_OK) return NTK_E_LAUNCH;
    }
    return NTK_OK;
}

int Engine::generate_batch(const int* const* prompts, const int* prompt_lens, int n, const nt_gen_params& p, int* out, int out_stride, int* out_counts) {
    stats_ = Stats();
    if (!loaded_) { err_ = "model not loaded"; return NTK_E_NULL; }
    if (n < 1 || n > model_.sequences()) { err_ = "generate_batch: the batch must hold 1 .. `sequences` prompts"; return NTK_E_SHAPE; }
    if (p.temperature > 0.0f || p.repeat_penalty != 1.0f) {
        err_ = "generate_batch: greedy only (temperature <= 0, repeat_penalty 1); sample from nt_engine_decode_batch's logits";
        return NTK_E_SHAPE;
    }
    if (p.max_tokens < 1 || out_stride < p.max_tokens) { err_ = "generate_batch: out_stride must hold max_tokens >= 1 ids per sequence"; return NTK_E_SHAPE; }
    const int V = model_.config().vocab_size, max_pos = model_.config().max_seq_len, eos = tok_.eos_id();
    for (int i = 0; i < n; ++i) {
        if (!prompts[i]) { err_ = "generate_batch: null prompt"; return NTK_E_NULL; }
        if (prompt_lens[i] < 1 || prompt_lens[i] > max_pos) { err_ = "generate_batch: a prompt is empty or exceeds the context"; return NTK_E_SHAPE; }
    }
    // prefill, slot by slot ("batch_prefill": in one packed pass); the first token of each sequence is the first maximum of its prompt's logits (Sampler::argmax)
    std::vector<float> prefill_logits;
    std::vector<int> last(n), pos(n);
    std::vector<char> live(n, 1);
    model_.set_batched_prefill(opt_.batched_prefill);
    auto t0 = Clock::now();
    { const int rc = prefill_slots(prompts, prompt_lens, n, prefill_logits); if (rc != NTK_OK) return rc; }
    for (int i = 0; i < n; ++i) {
        const float* host = prefill_logits.data() + (size_t)i * V;
        int best = 0;
        for (int j = 1; j < V; ++j) if (host[j] > host[best]) best = j;
        out[(size_t)i * out_stride] = last[i] = best;
        out_counts[i] = 1;
        pos[i] = prompt_lens[i];
        stats_.prompt_tokens += prompt_lens[i];
    }
    stats_.prefill_ms = ms_since(t0);
    int slots[Model::kMaxSequences], toks[Model::kMaxSequences], poss[Model::kMaxSequences], next[Model::kMaxSequences];
    auto d0 = Clock::now();
    int rc = NTK_OK;
    for (;;) {
        int B = 0;
        for (int i = 0; i < n; ++i) {   // who is still in: not at EOS, below max_tokens, inside the context
            if (live[i] && ((p.stop_at_eos && last[i] == eos) || out_counts[i] >= p.max_tokens || pos[i] >= max_pos)) live[i] = 0;
            if (live[i]) { slots[B] = i; toks[B] = last[i]; poss[B] = pos[i]; ++B; }
        }
        if (B == 0) break;
        if ((rc = model_.decode_batch(slots, toks, poss, B, nullptr, next)) != NTK_OK) { err_ = model_.error(); break; }
        for (int b = 0; b < B; ++b) {
            const int i = slots[b];
            out[(size_t)i * out_stride + out_counts[i]++] = last[i] = next[b];
            ++pos[i];
            ++stats_.gen_tokens;
        }
    }
    stats_.decode_ms = ms_since(d0);
    return rc == NTK_OK ? n : rc;
}

int Engine::decode_batch_sample(const int* slots, const int* tokens, const int* positions, int n, const nt_gen_params* params, const int* const* recent,
                                const int* n_recent, const float* r, float* logits_out, int* next_out) {
    if (!loaded_) { err_ = "model not loaded"; return NTK_E_NULL; }
    if (!params || !next_out) { err_ = "decode_batch_sample: null argument"; return NTK_E_NULL; }
    int rc = Model::validate_batch(slots, tokens, positions, n, model_.sequences(), model_.config().max_seq_len, model_.config().vocab_size, &err_);
    if (rc != NTK_OK) return rc;
    ntk_sample_rows rows{};
    for (int i = 0; i < n; ++i) {
        const bool sampled = params[i].temperature > 0.0f;
        if (sampled && !r) { err_ = "decode_batch_sample: a sampled row needs its uniform draw"; return NTK_E_NULL; }
        rows.temperature[i] = params[i].temperature; rows.top_k[i] = params[i].top_k; rows.top_p[i] = params[i].top_p;
        rows.repeat_penalty[i] = params[i].repeat_penalty;
        rows.r[i] = sampled ? r[i] : 0.0f;
        rows.n_recent[i] = recent && n_recent ? n_recent[i] : 0;
    }
    rc = model_.decode_batch_sample(slots, tokens, positions, n, rows, recent, logits_out, nullptr, next_out);
    if (rc != NTK_OK) err_ = model_.error();
    return rc;
}

int Engine::generate_batch_ex(const int* const* prompts, const int* prompt_lens, int n, const nt_gen_params* params, int* out, int out_stride, int* out_counts) {
    stats_ = Stats();
    if (!loaded_) { err_ = "model not loaded"; return NTK_E_NULL; }
    if (n < 1 || n > model_.sequences()) { err_ = "generate_batch_ex: the batch must hold 1 .. `sequences` prompts"; return NTK_E_SHAPE; }
    const int V = model_.config().vocab_size, max_pos = model_.config().max_seq_len, eos = tok_.eos_id();
    for (int i = 0; i < n; ++i) {
        if (params[i].max_tokens < 1 || out_stride < params[i].max_tokens) {
            err_ = "generate_batch_ex: out_stride must hold every sequence's max_tokens >= 1 ids";
            return NTK_E_SHAPE;
        }
        if (!prompts[i]) { err_ = "generate_batch_ex: null prompt"; return NTK_E_NULL; }
        if (prompt_lens[i] < 1 || prompt_lens[i] > max_pos) { err_ = "generate_batch_ex: a prompt is empty or exceeds the context"; return NTK_E_SHAPE; }
    }
    // prefill, slot by slot ("batch_prefill": in one packed pass); the first token of each sequence is sampled on the host from its prompt's logits, as Engine::run does
    std::vector<float> prefill_logits, host_rows;
    std::vector<Sampler> sampler(n);
    std::vector<std::vector<int>> seq(n);   // prompt + generated ids: the repeat-penalty windows are cut from these
    std::vector<int> pos(n);
    std::vector<char> live(n, 1), on_host(n, 0);
    model_.set_batched_prefill(opt_.batched_prefill);
    auto t0 = Clock::now();
    { const int rc = prefill_slots(prompts, prompt_lens, n, prefill_logits); if (rc != NTK_OK) return rc; }
    for (int i = 0; i < n; ++i) {
        float* const host = prefill_logits.data() + (size_t)i * V;
        sampler[i].init(sampler_config(params[i]));
        // what the device sampler does not take stays with this sequence's host Sampler (its row's logits alone are downloaded)
        on_host[i] = !Model::device_sampler_supports(params[i].temperature, params[i].top_k, V) || params[i].repeat_window > Model::kMaxRecent;
        seq[i].assign(prompts[i], prompts[i] + prompt_lens[i]);
        sampler[i].apply_repeat_penalty(host, V, seq[i]);
        const int first = sampler[i].sample(host, V);
        seq[i].push_back(first);
        out[(size_t)i * out_stride] = first;
        out_counts[i] = 1;
        pos[i] = prompt_lens[i];
        stats_.prompt_tokens += prompt_lens[i];
    }
    stats_.prefill_ms = ms_since(t0);
    int slots[Model::kMaxSequences], toks[Model::kMaxSequences], poss[Model::kMaxSequences], next[Model::kMaxSequences];
    const int* recent[Model::kMaxSequences];
    float* row_logits[Model::kMaxSequences];
    auto d0 = Clock::now();
    int rc = NTK_OK;
    for (;;) {
        int B = 0;
        bool any_host = false;
        ntk_sample_rows rows{};
        for (int i = 0; i < n; ++i) {   // who is still in: not at EOS, below its max_tokens, inside the context
            const nt_gen_params& p = params[i];
            if (live[i] && ((p.stop_at_eos && seq[i].back() == eos) || out_counts[i] >= p.max_tokens || pos[i] >= max_pos)) live[i] = 0;
            if (!live[i]) continue;
            slots[B] = i; toks[B] = seq[i].back(); poss[B] = pos[i];
            recent[B] = nullptr; row_logits[B] = nullptr;
            if (on_host[i]) {   // to the device as a greedy row without a penalty (its result is ignored)
                rows.repeat_penalty[B] = 1.0f;
                any_host = true;
            } else {
                const int have = (int)seq[i].size(), win = std::max(0, std::min(have, p.repeat_window));   // sampler.cpp:34
                rows.temperature[B] = p.temperature; rows.top_k[B] = p.top_k; rows.top_p[B] = p.top_p; rows.repeat_penalty[B] = p.repeat_penalty;
                rows.n_recent[B] = win;
                recent[B] = seq[i].data() + have - win;
                rows.r[B] = p.temperature > 0.0f ? sampler[i].draw() : 0.0f;   // one draw per sampled token, none for a greedy row
            }
            ++B;
        }
        if (B == 0) break;
        if (any_host) {   // V floats for each row the host samples
            host_rows.resize((size_t)B * V);
            for (int b = 0; b < B; ++b) if (on_host[slots[b]]) row_logits[b] = host_rows.data() + (size_t)b * V;
        }
        rc = model_.decode_batch_sample(slots, toks, poss, B, rows, recent, nullptr, any_host ? row_logits : nullptr, next);
        if (rc != NTK_OK) { err_ = model_.error(); break; }
        for (int b = 0; b < B; ++b) {
            const int i = slots[b];
            int tok = next[b];
            if (on_host[i]) {
                sampler[i].apply_repeat_penalty(row_logits[b], V, seq[i]);
                tok = sampler[i].sample(row_logits[b], V);
            }
            seq[i].push_back(tok);
            out[(size_t)i * out_stride + out_counts[i]++] = tok;
            ++pos[i];
            ++stats_.gen_tokens;
        }
    }
    stats_.decode_ms = ms_since(d0);
    return rc == NTK_OK ? n : rc;
}

// One generation, reference engine.cpp:40-145 step for step:
//   prefill (timed) -> logits -> repeat penalty -> sample first token -> decode loop (timed as a whole;
//   gen_tokens counts loop iterations, so the first sampled token is not counted) -> stop at EOS.
// `tokens` holds the prompt on entry and prompt + generated ids on return.
int Engine::run(std::vector<int>& tokens, const GenerateConfig& cfg, std::string* text, TokenCallback cb, bool print, bool stop_at_eos) {
    stats_ = Stats();
    if (!loaded_) { err_ = "model not loaded"; return NTK_E_NULL; }
    if (tokens.empty()) { err_ = "empty prompt"; return NTK_E_SHAPE; }
    Sampler sampler;
    SamplerConfig sc;
    sc.temperature = cfg.temperature; sc.top_k = cfg.top_k; sc.top_p = cfg.top_p;
    sc.repeat_penalty = cfg.repeat_penalty; sc.repeat_window = cfg.repeat_window; sc.seed = cfg.seed;
    sampler.init(sc);
    const int V = model_.config().vocab_size;
    const int eos = tok_.eos_id();
    const bool dev_greedy = opt_.fused && opt_.device_sampling && sampler.is_pure_greedy();
    // temperature / top-k / top-p / repeat penalty on the device too (ntk_sample_top_k): the host only draws the uniform number
    const bool dev_sample = opt_.fused && opt_.device_sampling && !dev_greedy &&
                            Model::device_sampler_supports(cfg.temperature, cfg.top_k, V);
    stats_.prompt_tokens = (int)tokens.size();
    if (cfg.verbose) fprintf(stderr, "Prompt tokens: %d\n", stats_.prompt_tokens);

    auto t0 = Clock::now();
    model_.set_batched_prefill(opt_.batched_prefill);
    float* logits = model_.forward(tokens.data(), (int)tokens.size(), 0);
    stats_.prefill_ms = ms_since(t0);
    if (!logits) { err_ = model_.error(); return NTK_E_LAUNCH; }

    std::vector<float> host(V);
    if (model_.copy_logits(host.data()) != NTK_OK) return NTK_E_LAUNCH;
    sampler.apply_repeat_penalty(host.data(), V, tokens);
    int next = sampler.sample(host.data(), V);
    tokens.push_back(next);
    auto emit = [&](int id) -> bool {
        const std::string piece = tok_.decode_token(id);
        if (text) *text += piece;
        if (cb) return cb(piece, id);
        if (print) { fputs(piece.c_str(), stdout); fflush(stdout); }
        return true;
    };
    if (!emit(next)) return NTK_OK;

    int pos = stats_.prompt_tokens;
    const int max_pos = model_.config().max_seq_len;
    int rc = NTK_OK;
    auto d0 = Clock::now();
    if (opt_.fused) {
        model_.set_device_pos(pos);
        model_.set_device_token(next);
    }
    // Greedy decoding on the device keeps ONE step queued ahead of the token the host is waiting for: the token id feeds the next step
    // on the device, so the next step's launches need nothing from the host, and the host's per-token work (poll, EOS check, detokenise,
    // graph launch) overlaps the GPU's.  A step queued behind what turns out to be EOS is discarded (one KV row past the end, harmless).
    int queued = 0;   // greedy steps launched and not yet consumed
    for (int i = 1; i < cfg.max_tokens; ++i) {
        if (stop_at_eos && next == eos) break;              // engine.cpp:106
        if (pos >= max_pos) {
            if (!opt_.context_shift) { fprintf(stderr, "\n[context of %d tokens exhausted]\n", max_pos); break; }
            // Context shift: half of what lies behind the kept prefix goes, the rest of slot 0 moves down (K re-rotated: Model::kv_shift).  Nothing is
            // in flight here: the run-ahead below queues no step past max_pos, and the token at max_pos - 1 has been waited for.
            const int keep = std::max(0, std::min(opt_.context_keep, max_pos - 2));
            const int shifted = model_.kv_shift(0, keep, Model::context_shift_discard(pos, keep), pos);
            if (shifted < 0) { rc = shifted; break; }
            pos = shifted;
            if (opt_.fused && (rc = model_.set_device_pos(pos)) != NTK_OK) break;   // re-bases the device position and picks the attention regime
        }
        if (opt_.fused) {
            if (dev_greedy) {
                if (queued == 0) { if ((rc = model_.decode_step_fused(true, opt_.graph)) != NTK_OK) break; ++queued; }
                if (i + 1 < cfg.max_tokens && pos + 1 < max_pos) {   // the step after this one, before this one's token is known
                    if ((rc = model_.decode_step_fused(true, opt_.graph)) != NTK_OK) break;
                    ++queued;
                }
                if ((rc = model_.wait_token(pos, &next)) != NTK_OK) break;   // first max, same as Sampler::argmax
                --queued;
            } else {
            rc = model_.decode_step_fused(false, opt_.graph);
            if (rc != NTK_OK) break;
            if (dev_sample) {
                const int have = (int)tokens.size(), win = std::min(have, cfg.repeat_window);   // sampler.cpp:34
                const float r = cfg.temperature > 0.0f ? sampler.draw() : 0.0f;                  // greedy takes no draw
                rc = model_.sample_on_device(tokens.data() + have - win, win, cfg.repeat_penalty, cfg.temperature, cfg.top_k,
                                             cfg.top_p, r);
                if (rc == NTK_OK) rc = model_.sync();
                if (rc != NTK_OK) break;
                next = model_.host_token();
            } else {
                if ((rc = model_.copy_logits(host.data())) != NTK_OK) break;
                sampler.apply_repeat_penalty(host.data(), V, tokens);
                next = sampler.sample(host.data(), V);
                model_.set_device_token(next);
            }
            }
        } else {
            logits = model_.forward(&next, 1, pos);          // engine.cpp:109
            if (!logits) { rc = NTK_E_LAUNCH; break; }
            if ((rc = model_.copy_logits(host.data())) != NTK_OK) break;
            sampler.apply_repeat_penalty(host.data(), V, tokens);
            next = sampler.sample(host.data(), V);
        }
        ++pos;
        tokens.push_back(next);
        ++stats_.gen_tokens;
        if (!emit(next)) break;
    }
    // the loop's wall time, as the reference counts it (engine.cpp:102-134): up to the last token the host saw.  A run-ahead step queued
    // behind what turned out to be the end (EOS, the callback, the token budget) is drained AFTER the clock stops: it decoded no counted
    // token.  (After run() the device position and the KV cache may therefore be one step past the returned tokens; every run re-bases
    // both -- set_device_pos -- before it decodes.)
    stats_.decode_ms = ms_since(d0);
    if (opt_.fused) { const int sr = model_.sync(); if (rc == NTK_OK) rc = sr; }
    if (rc == NTK_OK && opt_.fused) rc = model_.check_tp();   // the error word of the tensor-parallel exchange
    if (rc != NTK_OK) err_ = std::string("decode failed: ") + ntk_status_string(rc);
    return rc;
}

int Engine::decode_greedy_steps(int token, int pos, int n, int* out) {
    if (!loaded_) return NTK_E_NULL;
    if (pos < 0 || pos + n > model_.config().max_seq_len) return NTK_E_SHAPE;
    int next = token;
    if (opt_.fused) {
        model_.set_device_pos(pos);
        model_.set_device_token(next);
        // exactly n steps, one always queued ahead of the token the host is waiting for (see Engine::run); the host still sees every
        // token, in order, as Engine::generate does
        int launched = 0;
        for (int i = 0; i < n; ++i) {
            while (launched < n && launched <= i + 1) {
                const int rc = model_.decode_step_fused(true, opt_.graph);
                if (rc != NTK_OK) return rc;
                ++launched;
            }
            const int rc = model_.wait_token(pos + i, &next);
            if (rc != NTK_OK) return rc;
            if (out) out[i] = next;
        }
        { const int rc = model_.sync(); if (rc != NTK_OK) return rc; }
        return model_.check_tp();   // a bounded wait of the tensor-parallel exchange that gave up invalidates the run
    }
    std::vector<float> host(model_.config().vocab_size);
    for (int i = 0; i < n; ++i) {
        if (!model_.forward(&next, 1, pos + i)) return NTK_E_LAUNCH;
        if (model_.copy_logits(host.data()) != NTK_OK) return NTK_E_LAUNCH;
        next = Sampler::argmax(host.data(), (int)host.size());
        if (out) out[i] = next;
    }
    return NTK_OK;
}

int Engine::score(const int* tokens, const int* targets, int n, int start_pos, float* logprob_out, int* top1_out) {
    if (!loaded_) { err_ = "model not loaded"; return NTK_E_NULL; }
    model_.set_batched_prefill(opt_.batched_prefill);
    const int rc = model_.score(tokens, targets, n, start_pos, logprob_out, top1_out);
    if (rc != NTK_OK) err_ = model_.error();
    return rc;
}

std::string Engine::generate(const std::string& prompt, const GenerateConfig& cfg, TokenCallback cb) {
    std::vector<int> tokens = tok_.encode(prompt, true);
    std::string out;
    run(tokens, cfg, &out, cb, cfg.verbose, true);
    if (cfg.verbose) { fprintf(stdout, "\n"); print_stats(stats_); }
    return out;
}

int Engine::generate_tokens(const std::vector<int>& prompt, const GenerateConfig& cfg, std::vector<int>& out, bool stop_at_eos) {
    std::vector<int> tokens = prompt;
    GenerateConfig c = cfg;
    c.verbose = false;
    const int rc = run(tokens, c, nullptr, nullptr, false, stop_at_eos);
    out.assign(tokens.begin() + (long)prompt.size(), tokens.end());
    return rc;
}

void Engine::chat(const GenerateConfig& cfg) {   // engine.cpp:545-570: stateless turns
    fprintf(stdout, "NTransformer Chat (type 'quit' to exit)\nModel: %s (%d params)\n---\n", model_.config().model_name.c_str(),
            model_.config().n_layers);
    std::string line;
    for (;;) {
        fprintf(stdout, "> ");
        fflush(stdout);
        if (!std::getline(std::cin, line)) break;
        if (line == "quit" || line == "exit") break;
        if (line.empty()) continue;
        generate(line, cfg);
        fprintf(stdout, "\n");
    }
}

void Engine::benchmark(const std::string& prompt, int n_tokens) {   // engine.cpp:572-593
    GenerateConfig c;
    c.max_tokens = n_tokens;
    c.temperature = 0.0f;
    c.verbose = false;
    fprintf(stderr, "=== Benchmark ===\nPrompt: \"%s\"\nMax tokens: %d\n", prompt.c_str(), n_tokens);
    auto t0 = Clock::now();
    const std::string out = generate(prompt, c);
    fprintf(stderr, "Total time: %.1f ms\nOutput length: %zu chars\n", ms_since(t0), out.size());
    print_stats(stats_);   // the reference prints nothing here because verbose is false; the numbers are the point of a benchmark
}

void Engine::print_stats(const Stats& st) const {   // engine.cpp:595-607
    fprintf(stderr, "\n--- Stats ---\n");
    fprintf(stderr, "Prompt: %d tokens, %.1f ms (%.1f tok/s)\n", st.prompt_tokens, st.prefill_ms, st.prefill_tok_s());
    fprintf(stderr, "Decode: %d tokens, %.1f ms (%.1f tok/s)\n", st.gen_tokens, st.decode_ms, st.decode_tok_s());
    size_t fr = 0, tot = 0;
    ntk_device_mem_info(&fr, &tot);
    fprintf(stderr, "VRAM: %.1f / %.1f GB\n", (tot - fr) / 1073741824.0, tot / 1073741824.0);
}

}  // namespace nt
