// cli_main.cpp -- the `ntransformer` command line, flag for flag the reference's (reference src/main.cpp:8-174).
// Streaming-family flags exist to fit 24 GB of VRAM; on MI355X every target model is resident, so they are
// accepted for compatibility and reported as no-ops.  Added: --synthetic <preset>:<mix> to run without a file.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iterator>
#include <string>
#include <vector>
#include "engine/engine.h"
#include "../../include/ntk_engine.h"

static void usage(const char* prog) {
    fprintf(stderr,
            "NTransformer (MI355X-native) - quantized LLM decode engine\n\n"
            "Usage: %s [options] -m <model.gguf>\n\nOptions:\n"
            "  -m, --model <path>       Path to GGUF model file (required unless --synthetic)\n"
            "  -p, --prompt <text>      Prompt text (default: interactive mode)\n"
            "  -n, --n-tokens <int>     Max tokens to generate (default: 256)\n"
            "  -t, --temperature <float> Temperature (default: 0.7)\n"
            "  --top-k <int>            Top-K sampling (default: 40)\n"
            "  --top-p <float>          Top-P nucleus sampling (default: 0.9)\n"
            "  --repeat-penalty <float> Repeat penalty (default: 1.1)\n"
            "  -c, --ctx-size <int>     Context size (default: 4096)\n"
            "  --seed <int>             Random seed (default: 42)\n"
            "  --benchmark              Run benchmark mode\n"
            "  --chat                   Interactive chat mode\n"
            "  --perplexity <file>      Score the file's text in windows of the context size (BOS in front of each) and print its perplexity\n"
            "  -v, --verbose            Verbose output\n"
            "  -h, --help               Show this help\n"
            "  --no-fuse / --no-graph   Use the 15-launch/layer sequence / launch eagerly\n"
            "  --no-batched-prefill     Prompt tokens one by one (the reference's GEMV loops) instead of 16 per weight pass\n"
            "  --no-dense-fuse          F16 / BF16 matrices on the 1:1 launchers instead of the fused 16-bit GEMV and the batched prompt GEMM (A/B switch)\n"
            "  --no-moe-gemm            Prompt passes over mixture-of-experts layers on the expert GEMV instead of the grouped matrix-core GEMM (A/B switch)\n"
            "  --kv-cache <f16|q8_0>    KV cache format (default: f16; q8_0 = 8-bit Q8_0 blocks, 1.0625 bytes per element)\n"
            "  --rope-scaling <s>       file (default: the GGUF's rope_freqs.weight and linear scaling) | none | linear:<factor> |\n"
            "                           llama3:<factor>,<low>,<high>,<orig_ctx> (Llama-3.1 frequency factors computed by the engine)\n"
            "  --rope-freq-base <float> RoPE theta, overriding the model's\n"
            "  --rope-freq-scale <float> RoPE linear position scale, overriding the model's\n"
            "  --context-shift          At the end of the context drop half of the oldest positions and go on (default: stop there)\n"
            "  --keep <int>             Leading positions a context shift never drops (default: 1, the BOS)\n"
            "  --synthetic <shape:mix>  8b|70b|tiny|qwen2.5-7b|qwen3-8b|qwen3-4b|qwen3-30b-a3b|mixtral-8x7b : Q8_0|Q4_K_M|Q6_K|F16|BF16|...  seeded synthetic weights, no file\n"
            "Accepted for CLI compatibility, no effect on the output (weights are always resident in 288 GB HBM;\n"
            "speculative decoding only changes speed, and plain decode is what runs):\n"
            "  --streaming --draft-model <p> --draft-k <n> --self-spec\n"
            "Refused (in the reference they CHANGE the generated text; this engine does not implement them):\n"
            "  --early-exit <f> --skip-threshold <f> --requant-q4k --delta-model <p>\n",
            prog);
}

// --perplexity: the file's tokens in windows of ctx - 1, BOS in front of each, every window scored from position 0 (Engine::score); the first token
// of a window is context only.  exp(-mean log P) over all scored tokens, summed in double.
static int run_perplexity(nt::Engine& engine, const std::string& path, bool verbose) {
    std::ifstream in(path, std::ios::binary);
    if (!in) { fprintf(stderr, "Error: cannot read %s\n", path.c_str()); return 1; }
    const std::string text((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
    const std::vector<int> ids = engine.tokenizer().encode(text, false);
    if (ids.empty()) { fprintf(stderr, "Error: %s holds no text to score\n", path.c_str()); return 1; }
    const int ctx = engine.model().config().max_seq_len;
    if (ctx < 2) { fprintf(stderr, "Error: a context of %d tokens leaves nothing to score\n", ctx); return 1; }
    const size_t per = (size_t)ctx - 1;
    double sum = 0.0;
    size_t scored = 0;
    std::vector<int> window, targets;
    std::vector<float> lp;
    const auto t0 = std::chrono::steady_clock::now();
    for (size_t w0 = 0, k = 0; w0 < ids.size(); w0 += per, ++k) {
        const size_t n = std::min(per, ids.size() - w0);
        window.assign(1, engine.tokenizer().bos_id());
        window.insert(window.end(), ids.begin() + (long)w0, ids.begin() + (long)(w0 + n));
        targets.assign(window.begin() + 1, window.end());
        targets.push_back(-1);
        lp.assign(window.size(), 0.0f);
        if (engine.score(window.data(), targets.data(), (int)window.size(), 0, lp.data(), nullptr) != NTK_OK) {
            fprintf(stderr, "Error: scoring failed: %s\n", engine.error().c_str());
            return 1;
        }
        double ws = 0.0;
        for (size_t i = 0; i < n; ++i) ws += (double)lp[i];
        sum += ws;
        scored += n;
        if (verbose) fprintf(stdout, "window %zu: %zu tokens, perplexity %.4f\n", k, n, std::exp(-ws / (double)n));
    }
    const double secs = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    fprintf(stdout, "Perplexity: %.4f over %zu tokens (%.1f tok/s)\n", std::exp(-sum / (double)scored), scored, secs > 0 ? (double)scored / secs : 0.0);
    return 0;
}

int main(int argc, char** argv) {
    std::string model_path, prompt, synthetic, perplexity_file;
    int max_context = 4096;
    bool benchmark = false, chat = false;
    nt::GenerateConfig cfg;
    cfg.verbose = true;
    bool verbose_flag = false;
    nt::Engine engine;
    // reference main.cpp:52-103.  Streaming and speculative decoding change HOW tokens are produced, not WHICH tokens
    // (greedy speculative decoding verifies every draft token against the full model); they are accepted and plain resident
    // decode runs.  Early exit, layer skipping, Q6_K->Q4_K requantisation and delta models change the logits: silently
    // ignoring them would hand the user different text than the reference produces for the same command line, so they fail.
    auto noop = [](const char* flag, const char* why) { fprintf(stderr, "Note: %s has no effect: %s\n", flag, why); };
    auto refuse = [](const char* flag) {
        fprintf(stderr, "Error: %s is not supported by the MI355X engine (it changes the model's outputs in the reference: "
                        "layer skip / early exit / requantised or delta weights are not implemented here)\n", flag);
        return 2;
    };
    for (int i = 1; i < argc; ++i) {
        const std::string a = argv[i];
        auto val = [&]() -> const char* { return (i + 1 < argc) ? argv[++i] : nullptr; };
        if (a == "-h" || a == "--help") { usage(argv[0]); return 0; }
        else if (a == "-m" || a == "--model") { if (auto v = val()) model_path = v; }
        else if (a == "-p" || a == "--prompt") { if (auto v = val()) prompt = v; }
        else if (a == "-n" || a == "--n-tokens") { if (auto v = val()) cfg.max_tokens = std::stoi(v); }
        else if (a == "-t" || a == "--temperature") { if (auto v = val()) cfg.temperature = std::stof(v); }
        else if (a == "--top-k") { if (auto v = val()) cfg.top_k = std::stoi(v); }
        else if (a == "--top-p") { if (auto v = val()) cfg.top_p = std::stof(v); }
        else if (a == "--repeat-penalty") { if (auto v = val()) cfg.repeat_penalty = std::stof(v); }
        else if (a == "--seed") { if (auto v = val()) cfg.seed = std::stoull(v); }
        else if (a == "-c" || a == "--ctx-size") { if (auto v = val()) max_context = std::stoi(v); }
        else if (a == "--benchmark") benchmark = true;
        else if (a == "--chat") chat = true;
        else if (a == "-v" || a == "--verbose") { cfg.verbose = true; verbose_flag = true; }
        else if (a == "--perplexity") { const char* v = val(); if (!v) { fprintf(stderr, "Error: --perplexity takes a file\n"); return 1; } perplexity_file = v; }
        else if (a == "--no-fuse") { engine.options().fused = false; engine.options().batched_prefill = false; }
        else if (a == "--no-batched-prefill") engine.options().batched_prefill = false;
        else if (a == "--no-graph") engine.options().graph = false;
        else if (a == "--no-dense-fuse") (void)engine.model().set_dense_fused(false);
        else if (a == "--no-moe-gemm") engine.model().set_moe_gemm(false);
        else if (a == "--synthetic") { if (auto v = val()) synthetic = v; }
        else if (a == "--kv-cache") {
            const char* v = val();
            if (!v || engine.model().set_kv_cache(v) != NTK_OK) { fprintf(stderr, "Error: --kv-cache takes f16 or q8_0\n"); return 1; }
        }
        else if (a == "--rope-scaling" || a == "--rope-freq-base" || a == "--rope-freq-scale") {
            const char* v = val();
            const int rc = !v ? NTK_E_NULL : a == "--rope-scaling" ? engine.model().set_rope_scaling(v)
                                           : a == "--rope-freq-base" ? engine.model().set_rope_freq_base(v) : engine.model().set_rope_freq_scale(v);
            if (rc != NTK_OK) { fprintf(stderr, "Error: %s: %s\n", a.c_str(), v ? engine.model().error().c_str() : "a value is needed"); return 1; }
        }
        else if (a == "--context-shift") engine.options().context_shift = true;
        else if (a == "--keep") {
            const char* v = val();
            if (!v || atoi(v) < 0) { fprintf(stderr, "Error: --keep takes a number of positions >= 0\n"); return 1; }
            engine.options().context_keep = atoi(v);
        }
        else if (a == "--streaming") noop(a.c_str(), "weights are fully resident on MI355X");
        else if (a == "--self-spec") noop(a.c_str(), "plain decode runs (same tokens under greedy decoding, no draft pass)");
        else if (a == "--draft-model" || a == "--draft-k") { (void)val(); noop(a.c_str(), "plain decode runs (same tokens under greedy decoding, no draft model is loaded)"); }
        else if (a == "--requant-q4k") return refuse(a.c_str());
        else if (a == "--early-exit" || a == "--skip-threshold" || a == "--delta-model") { (void)val(); return refuse(a.c_str()); }
        else { fprintf(stderr, "Unknown option: %s\n", a.c_str()); usage(argv[0]); return 1; }
    }
    if (model_path.empty() && synthetic.empty()) { fprintf(stderr, "Error: model path required (-m)\n\n"); usage(argv[0]); return 1; }

    int st;
    if (!synthetic.empty()) {
        nt::SynthSpec s;
        const size_t c = synthetic.find(':');
        const std::string shape = synthetic.substr(0, c);
        if (c != std::string::npos) s.mix = synthetic.substr(c + 1);
        if (shape == "70b") { s.hidden = 8192; s.inter = 28672; s.layers = 80; s.heads = 64; }
        else if (shape == "tiny") { s.hidden = 256; s.inter = 512; s.layers = 2; s.heads = 4; s.kv_heads = 2; s.vocab = 512; s.bos = 256; s.eos = 257; s.ctx = 256; }
        else if (shape == "qwen2.5-7b" || shape == "qwen2.5-7b-nobias") {   // Qwen2.5-7B's geometry with a tied head; -nobias: the same model without the three bias vectors (the A/B twin)
            s.hidden = 3584; s.inter = 18944; s.layers = 28; s.heads = 28; s.kv_heads = 4; s.vocab = 152064; s.ctx = 32768;
            s.eps = 1e-6f; s.theta = 1e6f; s.bos = 151643; s.eos = 151645;
            s.mix = (shape == "qwen2.5-7b" ? "qwen2-tied:" : "tied:") + s.mix;
        }
        else if (shape == "qwen3-8b" || shape == "qwen3-8b-nonorm" || shape == "qwen3-4b" || shape == "qwen3-4b-nonorm") {
            // Qwen3-8B (untied head) and Qwen3-4B (32 heads of 128 over a hidden size of 2560, tied head); -nonorm: the same model without the Q / K norm vectors (the A/B twin)
            const bool b8 = shape.compare(0, 8, "qwen3-8b") == 0, norm = shape.find("-nonorm") == std::string::npos;
            s.hidden = b8 ? 4096 : 2560; s.inter = b8 ? 12288 : 9728; s.layers = 36; s.heads = 32; s.kv_heads = 8; s.vocab = 151936; s.ctx = 40960;
            s.eps = 1e-6f; s.theta = 1e6f; s.bos = 151643; s.eos = 151645;
            s.mix = std::string(norm ? "qwen3-" : "") + "hd128" + (b8 ? ":" : "-tied:") + s.mix;
        }
        else if (shape == "qwen3-30b-a3b") {   // Qwen3-30B-A3B: 128 experts of width 768, 8 per token, in every layer; Q / K norms, 32 / 4 heads of 128 over a hidden size of 2048
            s.hidden = 2048; s.inter = 6144; s.layers = 48; s.heads = 32; s.kv_heads = 4; s.vocab = 151936; s.ctx = 40960;
            s.eps = 1e-6f; s.theta = 1e6f; s.bos = 151643; s.eos = 151645;
            s.mix = "qwen3-hd128-moe128x8-i768:" + s.mix;
        }
        else if (shape == "mixtral-8x7b") {   // Mixtral 8x7B under `llama`: 8 experts of width 14336 (= feed_forward_length), 2 per token
            s.hidden = 4096; s.inter = 14336; s.layers = 32; s.heads = 32; s.kv_heads = 8; s.vocab = 32000; s.ctx = 32768;
            s.eps = 1e-5f; s.theta = 1e6f; s.bos = 1; s.eos = 2;
            s.mix = "moe8x2:" + s.mix;
        }
        else if (shape != "8b") { fprintf(stderr, "unknown synthetic shape %s\n", shape.c_str()); return 1; }
        st = engine.load_synthetic(s, max_context);
    } else {
        st = engine.load(model_path, max_context);
    }
    if (st != NTK_OK) { fprintf(stderr, "Failed to load model: %s (%s)\n", model_path.c_str(), engine.error().c_str()); return 1; }

    if (!perplexity_file.empty()) return run_perplexity(engine, perplexity_file, verbose_flag);
    if (benchmark) engine.benchmark(prompt.empty() ? "The meaning of life is" : prompt, cfg.max_tokens);
    else if (chat || prompt.empty()) engine.chat(cfg);
    else engine.generate(prompt, cfg);
    return 0;
}
