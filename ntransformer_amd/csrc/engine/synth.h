// engine/synth.h -- seeded synthetic Llama-shaped weights in GGUF block encodings.
// No reference counterpart: the reference only ever loads real checkpoints, none of which exist in this
// environment (no network).  Blocks are generated directly (quants uniform over their integer range,
// FP16 super-scales chosen so dequantised rows have RMS ~ sigma/sqrt(in)), SURVEY.md section 8(d).
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

namespace nt {

struct SynthTensor {
    std::string name;
    int ggml_type;
    int64_t in_f, out_f;   // norm vectors: in_f = n, out_f = 1; bias vectors: in_f = 1, out_f = n
    double sigma;          // matrices and biases: the scale of the values; norm vectors: 0 = 1 + 0.05 u, negative = 1 + |sigma| u, u uniform in [-1, 1)
    size_t nbytes;
    int experts = 0;       // > 0: a 3-D expert tensor -- out_f counts the rows of ALL experts (expert e: rows e out_f / experts ..), written with dims (in_f, out_f / experts, experts)
};

struct SynthSpec {
    int hidden = 4096, inter = 14336, layers = 32, heads = 32, kv_heads = 8, vocab = 128256;
    int ctx = 131072;
    float eps = 1e-5f, theta = 500000.0f;
    int bos = 128000, eos = 128009;
    std::string mix = "Q8_0";   // Q8_0 | Q4_0 | Q4_K | Q5_K | Q6_K | F16 | F32 | Q4_K_M, optionally behind a flavour prefix (synth_flavour)
    uint64_t seed = 20260925;
};

// The architecture flavour rides in front of the mix (nt_synth_spec keeps its layout): "qwen2:<mix>" = a Qwen2 model -- architecture string and
// hyper-parameter keys "qwen2", three F32 bias vectors per layer (blk.N.attn_{q,k,v}.bias, behind attn_v.weight, seeded like every other tensor);
// "qwen2-tied:<mix>" = the same without output.weight (the LM head is token_embd.weight); "tied:<mix>" = the Llama model without output.weight (the
// bias-free twin of a tied Qwen2 model).  No prefix: the Llama model.
// "qwen3[-hd<N>][-tied]:<mix>" = a Qwen3 model -- architecture and keys "qwen3", no biases, two F32 norm vectors of head_dim values per layer
// (blk.N.attn_q_norm.weight, attn_k_norm.weight, behind attn_v.weight, seeded by name, values 1 + 0.5 u with u uniform in [-1, 1)); -hd<N> gives the
// heads a size of their own: <arch>.attention.key_length = value_length = N and projections of heads x N rows, whatever the hidden size.
// "hd<N>[-tied]:<mix>" = the Llama model with such a head size (Mistral-Nemo's kind; the norm-free twin of a qwen3-hd<N> model).
// The general form is a '-'-separated list in front of the ':' -- qwen2 | qwen3 first, then hd<N>, tied in any order.
// "moe<E>x<K>[-i<I_e>]" (with or without qwen3 / hd<N> / tied in front of it) = a mixture-of-experts model: every layer carries, in place of ffn_gate / ffn_up /
// ffn_down, the F32 router blk.N.ffn_gate_inp.weight (dims (hidden, E), values of scale 2 / sqrt(hidden)) and the 3-D expert tensors ffn_gate_exps /
// ffn_up_exps (dims (hidden, I_e, E)) and ffn_down_exps ((I_e, hidden, E)) in the types the mix gives the dense matrices; keys <arch>.expert_count = E,
// expert_used_count = K and -- with -i<I_e> -- expert_feed_forward_length (without it I_e = the spec's inter: Mixtral under `llama`); the architecture of a
// qwen3 model with experts is "qwen3moe".  E in 1 .. 256, K in 1 .. min(E, 16): anything else is refused by synth_plan.
struct SynthFlavour { bool qwen2, tied; std::string mix; bool qwen3 = false; int head_dim = 0; int experts = 0, used = 0, expert_inter = 0; };
SynthFlavour synth_flavour(const std::string& mix);
// tensor list in file order (token_embd, per-layer 9 tensors -- 12 in the Qwen2, 11 in the Qwen3 flavour --, output_norm, output); false if `mix` is unknown
bool synth_plan(const SynthSpec& s, std::vector<SynthTensor>& out);
// deterministic in (seed, name, element index); multi-threaded
void synth_fill(void* dst, const SynthTensor& t, uint64_t seed, int nthreads);
// GPT-2 style synthetic vocabulary: 256 byte tokens first, specials as control tokens
void synth_vocab(const SynthSpec& s, std::vector<std::string>& tokens, std::vector<int>& types);
// write a complete GGUF v3 file; 0 on success
int synth_write_gguf(const std::string& path, const SynthSpec& s, int nthreads);

}  // namespace nt
