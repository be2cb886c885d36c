// engine/rope_scaling.cpp -- see rope_scaling.h
#include "rope_scaling.h"
#include "../../../include/ntk.h"

#include <cmath>
#include <cstdlib>
#include <vector>

namespace nt {

int rope_llama3_factors(int head_dim, float theta, float factor, float low, float high, int orig_ctx, float* out) {
    if (!out) return NTK_E_NULL;
    if (head_dim < 2 || (head_dim & 1) || !(theta > 0.0f) || !(factor > 0.0f) || !(low > 0.0f) || !(high > 0.0f) || high == low || orig_ctx <= 0 ||
        !std::isfinite(theta) || !std::isfinite(factor) || !std::isfinite(low) || !std::isfinite(high))
        return NTK_E_SHAPE;
    const double pi = 3.14159265358979323846;
    const double low_wavelen = (double)orig_ctx / low, high_wavelen = (double)orig_ctx / high;
    for (int i = 0; i < head_dim / 2; ++i) {
        const double wavelen = 2.0 * pi * std::pow((double)theta, 2.0 * i / head_dim);
        double f;
        if (wavelen < high_wavelen) f = 1.0;
        else if (wavelen > low_wavelen) f = factor;
        else {
            const double s = ((double)orig_ctx / wavelen - low) / ((double)high - low);
            f = 1.0 / ((1.0 - s) / factor + s);
        }
        out[i] = (float)f;
    }
    return NTK_OK;
}

int rope_build_table(int head_dim, float theta, const float* factors, float* out) {
    if (!out) return NTK_E_NULL;
    if (head_dim < 2 || (head_dim & 1)) return NTK_E_SHAPE;
    for (int i = 0; i < head_dim / 2; ++i) {
        const float plain = 1.0f / powf(theta, (2.0f * i) / head_dim);   // (the line that has always filled the decode kernels' table)
        out[i] = factors ? plain / factors[i] : plain;
    }
    return NTK_OK;
}

bool parse_positive_float(const std::string& text, float* out) {
    if (text.empty()) return false;
    char* end = nullptr;
    const float v = strtof(text.c_str(), &end);
    if (end == text.c_str() || *end != 0 || !std::isfinite(v) || !(v > 0.0f)) return false;
    *out = v;
    return true;
}

bool parse_rope_scaling(const std::string& text, RopeScalingOption* out, std::string* why) {
    auto bad = [&](const char* m) { if (why) *why = std::string("rope_scaling: ") + m + " (file | none | linear:<factor> | llama3:<factor>,<low>,<high>,<orig_ctx>)"; return false; };
    RopeScalingOption o;
    if (text == "file") { *out = o; return true; }
    if (text == "none") { o.mode = RopeScalingOption::NONE; *out = o; return true; }
    const size_t colon = text.find(':');
    if (colon == std::string::npos) return bad("unknown value");
    const std::string kind = text.substr(0, colon);
    std::vector<std::string> args;
    for (size_t at = colon + 1;;) {
        const size_t comma = text.find(',', at);
        args.push_back(text.substr(at, comma == std::string::npos ? std::string::npos : comma - at));
        if (comma == std::string::npos) break;
        at = comma + 1;
    }
    if (kind == "linear") {
        if (args.size() != 1 || !parse_positive_float(args[0], &o.factor)) return bad("linear takes one factor > 0");
        o.mode = RopeScalingOption::LINEAR;
    } else if (kind == "llama3") {
        float ctx = 0.0f;
        if (args.size() != 4 || !parse_positive_float(args[0], &o.factor) || !parse_positive_float(args[1], &o.low) || !parse_positive_float(args[2], &o.high) ||
            !parse_positive_float(args[3], &ctx))
            return bad("llama3 takes four numbers > 0");
        if (o.high == o.low) return bad("llama3 needs high != low");
        if (ctx != std::floor(ctx) || ctx >= 2147483648.0f) return bad("llama3's original context must be an integer");
        o.orig_ctx = (int)ctx;
        o.mode = RopeScalingOption::LLAMA3;
    } else {
        return bad("unknown value");
    }
    *out = o;
    return true;
}

}  // namespace nt
