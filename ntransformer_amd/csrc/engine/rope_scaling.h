// engine/rope_scaling.h -- RoPE frequency scaling on the host: the Llama-3.1 per-pair divisors, the frequency table the kernels read, and the
// "rope_scaling" option's grammar.  No reference counterpart (the reference rotates with theta alone: config.h:34-36).
// Arithmetic (llama.cpp's, in the engine's F32 order): angle of pair i at position pos = (float)pos * tab[i] * freq_scale, left to right in F32;
// tab[i] = (1.0f / powf(theta, (2.0f * i) / head_dim)) / factor[i].
#pragma once
#include <string>

namespace nt {

// rope_freqs.weight as a Llama-3.1 converter computes it (double, stored as F32): out[head_dim / 2].  NTK_OK or NTK_E_NULL / NTK_E_SHAPE.
int rope_llama3_factors(int head_dim, float theta, float factor, float low, float high, int orig_ctx, float* out);
// the frequency table; factors == nullptr: the plain one.  NTK_OK or NTK_E_NULL / NTK_E_SHAPE.
int rope_build_table(int head_dim, float theta, const float* factors, float* out);

// "rope_scaling" = file | none | linear:<factor> | llama3:<factor>,<low>,<high>,<orig_ctx>
struct RopeScalingOption {
    enum Mode { FILE, NONE, LINEAR, LLAMA3 } mode = FILE;
    float factor = 1.0f, low = 1.0f, high = 4.0f;
    int orig_ctx = 0;
};
// false + *why: malformed (every number must parse completely, be finite and > 0; llama3 needs high != low)
bool parse_rope_scaling(const std::string& text, RopeScalingOption* out, std::string* why);
// a finite float > 0, the whole string
bool parse_positive_float(const std::string& text, float* out);

}  // namespace nt
