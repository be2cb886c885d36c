// engine/model.h -- resident-weights Llama model on one MI355X.
// Replaces the resident subset of reference src/model/{transformer,attention,ffn,norm}.{h,cpp}
// (Transformer::load / load_layer / allocate_buffers / embed_tokens / forward, Attention::forward,
// FFN::forward, RMSNorm::forward).  The reference's streaming / tiered / delta / speculative paths exist
// to fit 24 GB of VRAM and are dropped: 288 GB of HBM holds every target model resident.
#pragma once
#include <algorithm>
#include <array>
#include <chrono>
#include <cstdint>
#include <string>
#include <vector>
#include "gguf.h"
#include "kv_cache.h"
#include "rope_scaling.h"
#include "synth.h"

struct ntk_sample_rows;   // include/ntk_engine.h
struct ntk_kv_segments;

struct ihipGraphExec_t;   // hipGraphExec_t

namespace nt {

struct DevTensor {
    void* ptr = nullptr;   // device
    int dtype = 0;
    int64_t in_f = 0, out_f = 0;
    size_t nbytes = 0;
    void* rp = nullptr;    // engine-owned repack for the decode GEMV (K-quants: csrc/gemv_rp.hip, matrix cores; Q8_0: lane-major rows, csrc/gemv.hip); nullptr: none
    size_t rp_bytes = 0;
};

struct PassStatus;   // model_impl.h

struct LayerWeights {
    DevTensor attn_norm, wq, wk, wv, wo, ffn_norm, w_gate, w_up, w_down;
    DevTensor bq, bk, bv;   // the Q | K | V projection biases of a Qwen2-family file (F32 [out]; each optional: ptr == nullptr without one)
    bool has_qkv_bias() const { return bq.ptr || bk.ptr || bv.ptr; }
    DevTensor q_norm, k_norm;   // the per-head RMSNorm weights of Q and K of a Qwen3-family file (F32 [head_dim], whole on every rank; a pair or neither)
    bool has_qk_norm() const { return q_norm.ptr && k_norm.ptr; }
    // the routed expert FFN of a mixture-of-experts layer (Qwen3-MoE, Mixtral) IN PLACE of w_gate / w_up / w_down: the F32 router [E][hidden] and the three
    // 3-D expert tensors as raw GGUF bytes (expert e: the block of out_f rows at e x out_f x row bytes; in_f / out_f are ONE expert's extents).  All four or none.
    DevTensor router, gate_exps, up_exps, down_exps;
    bool is_moe() const { return router.ptr != nullptr; }
    bool moe_gemm_ok = false;   // decided at load: the three expert tensors are types, shapes and addresses the grouped prompt GEMM (csrc/moe_gemm.hip) takes
};
// the seven projection matrices of a layer, for whoever visits them all: for (auto m : kLayerMatrices) use(L.*m);
inline constexpr std::array<DevTensor LayerWeights::*, 7> kLayerMatrices = {&LayerWeights::wq, &LayerWeights::wk, &LayerWeights::wv, &LayerWeights::wo,
                                                                            &LayerWeights::w_gate, &LayerWeights::w_up, &LayerWeights::w_down};

enum Shard { WHOLE, ROWS, COLS };   // a tensor's part on a tensor-parallel rank: all of it, a block of rows, a block of columns

class Model {
public:
    Model() = default;
    ~Model();
    Model(const Model&) = delete;
    Model& operator=(const Model&) = delete;

    // reference Transformer::load (transformer.cpp:59-126): parse, cap context, weights -> HBM, buffers
    int load(const std::string& gguf_path, int max_context);
    // same model object built from the seeded generator, tensor by tensor, without a file
    int load_synthetic(const SynthSpec& spec, int max_context, int nthreads);
    // A SECOND SEQUENCE over the weights `src` holds resident (round 6; SURVEY 8(e): the path shards across requests -- independent sequences share
    // nothing but the read-only weights): this object gets src's tensor table (the same device pointers, raw and repacked; it owns none of them), its
    // own KV caches, activation buffers, device scalars, captured graphs and its own non-blocking stream, so two host threads can decode two requests
    // on one GPU at once.  `src` must outlive this object and must not be re-loaded or switch its repack level meanwhile; a source with one resident
    // copy of its K-quant weights gives this sequence an unpack scratch of its own; tensor-parallel slices are refused (NTK_E_SHAPE).
    int share_weights(const Model& src, int max_context);

    // reference Transformer::forward (transformer.cpp:604-669): the reference's launcher sequence, 1:1,
    // any seq_len (prefill = per-token GEMV loops like the reference).  Returns device logits [vocab].
    // slot: the sequence slot whose KV cache the pass reads and writes (0 .. sequences() - 1; slot 0 is the cache every other entry point uses)
    float* forward(const int* tokens, int seq_len, int start_pos, int slot = 0);

    // Scoring (csrc/logprob.hip): the prompt pass over `tokens` at start_pos exactly as forward() runs it -- the KV cache afterwards is forward's, bit for bit --
    // and then, instead of the last position's logits: the final RMSNorm of ALL rows (into residual_), the LM head over score_rows rows at a time into a
    // [score_rows][vocab] F32 buffer (the FP16 GEMM where forward's projections take it, read from the repack when the head lies only there; otherwise the
    // F32-MFMA form or the per-row GEMV) and ntk_logprob_rows on each chunk.  logprob_out[i] = log P(targets[i] | tokens[0..i]) (natural log; 0 where
    // targets[i] < 0), top1_out[i] (optional) = the greedy token behind tokens[0..i].  One D2H copy and one synchronisation per call.  The chunk buffer and the
    // device target / result arrays are allocated by the FIRST call (NTK_E_NOMEM + error(): the model stays usable) and freed with the model.  Refused
    // (NTK_E_SHAPE + error()): ids out of range, a sequence beyond the context, tensor parallelism.
    int score(const int* tokens, const int* targets, int seq_len, int start_pos, float* logprob_out, int* top1_out, int slot = 0);

    // ---- sequence slots and the batched decode step ---------------------------------------------------------------------------------
    // "sequences" = N (1 .. kMaxSequences, default 1; BEFORE the load, kept across loads; a sharing sequence takes its own): slots 1 .. N - 1 are extra
    // caches of slot 0's format and layout (KvCache, kv_cache.h), allocated at load and counted in kv_cache_bytes(), beside a [16][vocab] F32 logits buffer, the batch
    // attention's scratch, the batched sampler's windows / scratch / pinned mirrors (batch_sample_buffers: about 0.9 MB, not counted) and -- where
    // score_buffers() would need one -- an LM-head GEMM workspace.  N = 1 allocates nothing (decode_batch with one row on slot 0 allocates the logits
    // buffers on its first call, as score() does).  Refused at load with kv_cache = q8_0 (unless "batch_kv_q8", below), tensor parallelism or a context of fewer than N positions (a
    // step is a pass of up to N rows through the max_seq-row activation buffers).
    static constexpr int kMaxSequences = 16;
    int set_sequences(int n);
    int sequences() const { return sequences_; }
    // "batch_kv_q8" = 1 (default 0; BEFORE the load, kept across loads; a sharing sequence takes its own): sequence slots and the batched step over the
    // 8-bit cache.  With kv_cache = q8_0 the load then takes sequences = 1 .. 16 -- every slot an 8-bit cache (zeroed), the one-layer F16 image of the
    // prompt path stays ONE per engine (KvCache, kv_cache.h) -- and decode_batch /
    // decode_batch_sample run: their attention is ntk_attention_decode_q8_batch with kv_q8_splits(attention_regime(largest position)) splits.
    // kv_cache = f16: accepted, changes nothing.  The option exists ONLY because the default refusals (sequences > 1 at load, decode_batch on a q8_0
    // engine) are pinned by tests/test_batch_decode_gpu.py::test_refusals_leave_the_engine_usable: with it off every refusal and message is unchanged.
    // A later change that may touch that test can fold the option away.
    int set_batch_kv_q8(bool on);
    // "static_activations" = 1 (default; BEFORE the load, kept across loads): the fused single-token path keeps its hidden state, attention output and
    // SiLU x up vector in the library's static decode slots (ntk_decode_arena_*, ntk_engine.h), where the Q8_0 decode GEMVs request x before their kernel
    // arguments have arrived.  One engine per process and device owns the slots -- the first to load, until it closes; every other one (a second engine,
    // a sharing sequence, tensor-parallel ranks, sizes beyond a slot) and = 0 run the same launches on buffers of their own.  Same bits either way.
    int set_static_activations(bool on);
    bool static_activations_active() const { return arena_owner_; }
    bool batch_kv_q8() const { return batch_kv_q8_; }
    // One decode step of B sequences in ONE pass over the weights: row b = token tokens[b] of the sequence in slot slots[b] at positions[b].  Eager and
    // host-driven: one H2D copy of tokens | positions, embedding, the layer loop as for a prompt of B tokens (layers_1to1 in batch mode: rope / store /
    // attention are one ntk_attention_decode_batch over the rows' own caches; B = 1: the projections of a 1-token forward), the final RMSNorm and the LM head
    // over the B rows (lm_head: score()'s, full_form), ntk_logprob_rows for each row's first maximum, one D2H copy of whichever of logits_out [B][vocab] /
    // next_out [B] is non-null, one synchronisation.  ARITHMETIC: the prompt pass's (FP16 matrix cores, two FP16 pieces per activation) with the decode
    // kernels' attention -- within the 1e-3 bar of the fused decode path, not its bits; within one batch size a row depends on nothing but that row.
    // Touches nothing of the fused path's slot-0 state (d_pos_, d_token_, graphs).  Refused (NTK_E_SHAPE + error()): see validate_batch.
    int decode_batch(const int* slots, const int* tokens, const int* positions, int B, float* logits_out, int* next_out);
    // The same step with the rows SAMPLED on the device: ntk_sample_rows_top_k over the step's logits in place of the greedy pass -- row b with rows'
    // settings [b], draw rows.r[b] and the window recent[b][0 .. rows.n_recent[b]) (host ints; read only where the row has a penalty to apply; each
    // n_recent at most kMaxRecent).  The windows go up in ONE further host-to-device copy, packed at the step's own pitch; next_out [B] comes back through a
    // pinned mirror; one synchronisation.  logits_out [B][vocab] (optional) and row_logits[b] (optional per row, vocab floats each: a caller that samples
    // some rows on the host downloads those alone) receive the logits BEFORE any penalty: their copies are queued ahead of the sampler.  The sampled stream
    // is the host Sampler's on this step's logits (csrc/sampling_core.hip.h).  Refused as decode_batch, and NTK_E_SHAPE for a row the device sampler does
    // not take (device_sampler_supports) or a window beyond kMaxRecent.
    static constexpr int kMaxRecent = 4096;
    int decode_batch_sample(const int* slots, const int* tokens, const int* positions, int B, const ntk_sample_rows& rows, const int* const* recent,
                            float* logits_out, float* const* row_logits, int* next_out);
    // the host-side checks of decode_batch (no device): B in 1 .. sequences, every slot in range and named once, positions in [0, max_seq), token ids in
    // [0, vocab); NTK_OK or NTK_E_NULL / NTK_E_SHAPE with the reason in *why (optional)
    static int validate_batch(const int* slots, const int* tokens, const int* positions, int B, int sequences, int max_seq, int vocab, std::string* why);
    // ---- the packed prompt pass -----------------------------------------------------------------------------------------------------
    // SEVERAL sequences' tokens in ONE pass over the weights: segment i = lens[i] consecutive tokens of the sequence in slot slots[i], the first at cache
    // position start_pos[i]; tokens_flat holds the segments' tokens back to back (a one-token segment at start_pos > 0 is a decode row, a longer one a prompt
    // chunk).  Eager: one H2D copy of the tokens and one of the gather indices, embedding, layers_1to1 over all rows with the SEGMENT form of the KV target
    // (rope / store: ntk_rope_kv_store_segments, attention: ntk_attention_prefill_segments, each over the slots' own caches), the last row of every segment
    // gathered into n contiguous rows, the final RMSNorm and the LM head over those n rows (lm_head: score()'s, full_form), ntk_logprob_rows for the first
    // maxima, one D2H copy of whichever of logits_out [n][vocab] / next_out [n] is non-null, one synchronisation.  Allocates nothing sized by the context
    // (the batch buffers of decode_batch on a first call).  ARITHMETIC: forward()'s layer arithmetic for the pass's total row count, so one
    // segment of two tokens or more leaves forward()'s cache rows bit for bit; logits within 1e-3 of forward's (another LM-head form); within one total row
    // count a segment depends on nothing but itself.  Refused (NTK_E_SHAPE + error(); nothing launched): validate_forward_batch, a token id out of range,
    // kv_cache = q8_0 (the prompt path's ONE one-layer F16 image cannot hold several slots at once), tensor parallelism.
    int forward_batch(const int* slots, const int* tokens_flat, const int* lens, const int* start_pos, int n, float* logits_out, int* next_out);
    // its host-side checks (no device): n in 1 .. sequences, slots in range and named once, every lens[i] >= 1, start_pos[i] >= 0 and start_pos[i] +
    // lens[i] <= max_seq, the lengths summing to at most max_seq (the pass runs through the max_seq-row activation buffers)
    static int validate_forward_batch(const int* slots, const int* lens, const int* start_pos, int n, int sequences, int max_seq, std::string* why);
    // ---- KV cache sequence operations (csrc/kv_ops.hip) ------------------------------------------------------------------------------
    // Context shift of one slot: positions [keep, keep + discard) are dropped, rows [keep + discard, n_past) move down to [keep, ...) in every layer, in
    // the cache format the engine was loaded with (ntk_kv_shift / ntk_kv_shift_q8 with the engine's frequency table: K re-rotated by -discard positions,
    // V byte for byte; ONE launch whatever the overlap).  Queued on the model's stream, no synchronisation; returns the new n_past - discard (>= 0) or a
    // negative status.  The fused path's device position is NOT touched when slot 0 is shifted: the caller re-bases it (set_device_pos), as every run
    // does.  keep + discard == n_past: nothing moves.  Refused (NTK_E_SHAPE + error(); nothing is launched): see validate_kv_shift, and tensor parallelism.
    int kv_shift(int slot, int keep, int discard, int n_past);
    // Rows [pos0, pos0 + n) of every layer and both sides from slot to slot, at the same positions, no rotation: stream-ordered device-to-device copies
    // (F16: one range per layer and side; q8_0: quants and scales).  Returns n or a negative status; refusals: validate_kv_copy, tensor parallelism.
    int kv_copy(int src_slot, int dst_slot, int pos0, int n);
    // the host-side checks of the two (no device): NTK_OK or NTK_E_SHAPE with the reason in *why (optional)
    static int validate_kv_shift(int slot, int keep, int discard, int n_past, int sequences, int max_seq, std::string* why);
    static int validate_kv_copy(int src_slot, int dst_slot, int pos0, int n, int sequences, int max_seq, std::string* why);
    // how many positions the generate loop drops when the context is full: half of what lies behind `keep`, one at the least
    static int context_shift_discard(int n_past, int keep) { return std::max(1, (n_past - keep) / 2); }
    int set_score_rows(int rows);   // rows of logits per LM-head chunk, 1 .. 1024 (default 256: 131 MB at a vocabulary of 128 256); any time

    // Fused single-token step: 5 launches per layer, position and token id stay on the device so the whole
    // token is one hipGraph replay.  Token comes from d_token_ (set_device_token / previous argmax).
    // If greedy: also runs the device argmax and advances the position.
    int decode_step_fused(bool greedy, bool use_graph);
    int set_device_token(int token);
    int set_device_pos(int pos);
    // attention regime by context length (each regime is its own captured graph: the grid of the attention launch is fixed in it).
    // 0: the single-pass kernel, one workgroup per query head, walks the head's cache serially (4.2 us per layer at 16 positions, 7.5 at
    //    512, 30.7 at 4095).  Beyond 544 positions: ntk_attention_decode_split = partial states of `splits` workgroups + a combine launch:
    // 1: 8 splits -- the per-query-head walk (8.7 us per layer at 1023 positions, 10.1 at 2047, 13.5 at 4095);
    // 2: head_dim 128, from 3072 positions: 32 splits -- the matrix-core form, one workgroup per (KV head, split), every cache row read
    //    once, one 32-row chunk per wave up to 4096 positions (12.75 us at 4095; 70B geometry 13.5 vs 16.5; decode behind a 3900-token
    //    prompt 467 -> 482 tokens/s; with 16 splits the two forms tie between 2300 and 3300 positions:
    //    profiles/r04_attention_kvhead_form.txt); other head sizes: the walk with 16 splits from 16384 positions.
    //    Contexts beyond 4096 (round 5; the reference's -c / --ctx-size, main.cpp:74-75): 32 splits STAY the best count however long the context --
    //    8B geometry, us per layer incl. the combine launch, caches past the Infinity Cache (tools/attn_bench.py --max-seq,
    //    profiles/r05_attention_long_context.txt): 8191 positions 17.2 / 14.6 / 19.1 / 27.2 with 16 / 32 / 64 / 128 splits; 32767: 30.1 /
    //    35.8 / 42.8 / 59.4 with 32 / 64 / 128 / 256 (4.45 TB/s of cache bytes at 32); 131071: 103 / 108 / 118 with 64 / 128 / 256 (5.2
    //    TB/s): one workgroup per CU (8 KV heads x 32), the chunks of 32 rows go round ALL waves of the launch, and every further split
    //    costs a redundant RoPE prologue and a longer serial walk in the combine launch.
    static constexpr int kAttnRegimes = 3;
    static int attention_regime(int pos, int head_dim) {
        if (pos < 544) return 0;
        return pos < (head_dim == 128 ? 3072 : 16384) ? 1 : 2;
    }
    static int attention_splits(int regime, int head_dim) { return regime <= 1 ? 8 : head_dim == 128 ? 32 : 16; }
    static constexpr int kMaxAttnSplits = 32;
    void pick_attention_regime();
    int sync();
    int host_token() const;                 // token written by the last device argmax (after sync)
    // token of the greedy fused step that decoded position `pos`, polled from the pinned ring without a stream synchronisation (the
    // caller may already have queued the next step)
    int wait_token(int pos, int* token);
    float* logits_ptr() { return logits_; }
    int copy_logits(float* host);           // D2H of [vocab] floats (blocking)
    // Sample the next token from the device logits with the reference's sampler (ntk_sample_top_k / penalty + ntk_argmax when
    // temperature <= 0): result in d_token_ and, after sync(), host_token().  recent: the last tokens (host), r: the host's draw.
    int sample_on_device(const int* recent, int n_recent, float repeat_penalty, float temperature, int top_k, float top_p, float r);
    static bool device_sampler_supports(float temperature, int top_k, int vocab) {
        return temperature <= 0.0f || (top_k > 0 && top_k <= 64 && top_k < vocab && vocab <= 131072);
    }

    const ModelConfig& config() const { return cfg_; }
    const GgufVocab& vocab() const { return vocab_; }
    const std::string& error() const { return err_; }
    uint64_t weight_bytes() const { return weight_bytes_; }
    // algorithmic bytes one decode token must move at position `pos`
    uint64_t bytes_per_token(int pos) const;
    // Prompts (seq_len > 1) project all tokens of a chunk with one pass over each weight matrix (ntk_gemm_quant) instead
    // of the reference's per-token GEMV loops; off = the reference's exact launch sequence.
    void set_batched_prefill(bool on) { batched_prefill_ = on; }
    // KV cache format: "f16" (default) or "q8_0" (csrc/attention_q8.hip: Q8_0 blocks along head_dim, 1.0625 bytes per element + ONE layer's F16
    // scratch image for the prompt path).  Set BEFORE the load (load / load_synthetic / share_weights: a sharing sequence takes its own option);
    // refused afterwards.  q8_0 needs head_dim 128, <= 16 query heads per KV head and no tensor parallelism: the load refuses otherwise.
    // Decode: ntk_attention_decode_q8 + the combine launch in every regime (splits: kv_q8_splits).  Prompt pass / 1:1 sequence: 8-bit store, then
    // rows [0, start_pos + T) dequantised (rounded to half) into the scratch that the unchanged F16 attention kernels read.
    int set_kv_cache(const std::string& kind);
    // RoPE frequency scaling (rope_scaling.h).  Three options, BEFORE the load, kept across loads, refused afterwards (NTK_E_SHAPE + error();
    // malformed text too): "rope_scaling" = file (default: the GGUF's rope_freqs.weight divisors and its linear scaling keys) | none (ignore them) |
    // linear:<factor> (the linear scale alone: the file's divisors stay) | llama3:<factor>,<low>,<high>,<orig_ctx> (the engine computes the divisors,
    // replacing the file's: how a synthetic model gets them); "rope_freq_base" =
    // theta, "rope_freq_scale" = the linear scale, each overriding what file and rope_scaling gave.  A load resolves them into cfg_.rope_theta,
    // cfg_.rope_freq_scale and rope_factors_; alloc_buffers folds the divisors into rope_inv_freq_, the table every decode launch and the context shift
    // already read.  The prompt-side launches get that table ONLY when there are divisors (rope_tab()): a model without them passes NULL as it always
    // has, so its prompt passes keep the in-kernel frequency and every bit they had.  A sharing sequence takes its source's table and scale.
    int set_rope_scaling(const std::string& text);
    int set_rope_freq_base(const std::string& text);
    int set_rope_freq_scale(const std::string& text);
    int rope_factor_count() const { return (int)rope_factors_.size(); }
    // Q | K | V projection biases (blk.N.attn_{q,k,v}.bias; Qwen2, optional under any architecture): each F32 with one value per output row, a rank's
    // slice under tensor parallelism.  A layer that carries one gets ONE more launch behind its Q | K | V projection in both layer loops (ntk_qkv_bias:
    // layers_1to1 ahead of the KV capture, enqueue_layers as a node of the captured graph); a layer without issues the launches it always has.
    // Refused at load, ahead of the device and naming the tensor: a bias of another type or size, and the tensors the engine would silently ignore
    // (attn_output.bias, ffn_gate / ffn_up / ffn_down.bias).
    int qkv_bias_layers() const { int n = 0; for (const auto& L : layers_) n += L.has_qkv_bias() ? 1 : 0; return n; }
    // Per-head RMSNorm of Q and K (blk.N.attn_q_norm.weight / attn_k_norm.weight; Qwen3, optional under any architecture): F32, head_dim values each, one
    // vector for all heads of the layer, whole on every tensor-parallel rank.  A layer that carries the pair gets ONE more launch (ntk_qk_norm) behind
    // the bias launch and ahead of the rotation in both layer loops; a layer without issues the launches it always has.  Refused at load, ahead of the
    // device and naming the tensor: a norm of another type or size, one without its partner, one on a layer the model does not have.
    int qk_norm_layers() const { int n = 0; for (const auto& L : layers_) n += L.has_qk_norm() ? 1 : 0; return n; }
    // Mixture-of-experts layers (blk.N.ffn_gate_inp.weight + ffn_{gate,up,down}_exps.weight; any architecture, a rule per layer): the FFN of such a layer is
    // ntk_rmsnorm -> ntk_moe_route -> ntk_moe_gate_up -> ntk_moe_down (csrc/moe.hip) in both layer loops, on the expert tensors' raw GGUF bytes at every
    // repack level; a dense layer issues the launches it always has.  Refused at load, ahead of the device and naming the tensor or key: both FFN forms
    // on one layer or a partial quartet, a quartet on a layer the model does not have, a router that is not F32 [E][hidden], an expert tensor that is not
    // 3-D with the model's extents or not Q8_0 / Q4_K / Q6_K, E or K outside 1 .. 256 / 1 .. min(E, 16), expert keys without a quartet, shared-expert
    // tensors, tensor parallelism.
    int moe_layers() const { int n = 0; for (const auto& L : layers_) n += L.is_moe() ? 1 : 0; return n; }
    // A pass of at least moe_gemm_min_rows_ rows over such a layer takes ntk_moe_gemm_gate_up -> ntk_moe_gemm_down (csrc/moe_gemm.hip: the grouped GEMM on the
    // matrix cores) in place of the two GEMV launches, on the same workspace sections, where option moe_gemm is on and the layer's tensors are ones the GEMM
    // takes (LayerWeights::moe_gemm_ok; a layer it does not take stays on the GEMV without a word).  The threshold is above 1 whatever is set: the decode
    // step and its captured graph stay on the GEMV launches, bit for bit.  Both options may be set at any time (the A/B switch).
    static constexpr int kMoeGemmMinRows = 2;   // profiles/moe_gemm.txt: the smallest measured row count (2 / 4 / .. / 1024) from which the GEMM form wins at that and every larger one, on both shapes
    void set_moe_gemm(bool on) { moe_gemm_ = on; }
    int set_moe_gemm_min_rows(int n) {
        if (n < 1 || n > 1024) { err_ = "moe_gemm_min_rows must be 1 .. 1024"; return NTK_E_SHAPE; }
        moe_gemm_min_rows_ = n;
        return NTK_OK;
    }
    bool kv_q8() const { return kv_q8_; }
    static int kv_q8_splits(int regime) { return regime == 0 ? 4 : regime == 1 ? 16 : 32; }
    uint64_t kv_cache_bytes() const { return kv_.bytes(); }   // resident KV bytes of this engine: every slot, the q8_0 mode's one F16 image included
    int debug_kv_inputs_capture(int layer);
    int debug_kv_inputs_read(int n, float* k, float* v);
    // cache rows [pos0, pos0 + n) of a layer of sequence slot `slot` as canonical 34-byte GGUF block_q8_0, [n][n_kv_heads * head_dim / 32] blocks per
    // side (q8_0 mode only: NTK_E_DTYPE otherwise; a slot out of range: NTK_E_SHAPE)
    int debug_kv_q8(int layer, int pos0, int n, uint8_t* k_blocks, uint8_t* v_blocks, bool write, int slot = 0);
    void set_prefill_row_max(bool on) { prefill_row_max_ = on; }
    void set_prefill_fused_split(bool on) { prefill_fused_split_ = on; }
    // Split-KV decode attention as ONE launch (the last workgroup of a head merges the partial states: attention_merge.hip.h) or -- the default --
    // with the separate combine launch of rounds 3-5; same bits either way, the one-launch form measured 0.1-0.6 us (walk) / 1.5-4 us (matrix-core
    // form) per layer slower (profiles/NEGATIVE_RESULTS.md 8).  Captured graphs are dropped when the setting changes.
    int set_attention_merge(bool on);
    // Decode GEMVs of the K-quant and Q8_0 matrices from the load-time repack (ntk_gemv_rp_fused) instead of the raw GGUF blocks (ntk_gemv_fused).
    // Q8_0 (lane-major rows: the same bytes permuted, csrc/gemv_core.hip.h) is repacked at every level > 0 and ALWAYS keeps its GGUF bytes resident beside
    // the repack (the prompt GEMM, the 1:1 launchers and the embedding lookup read GGUF Q8_0 blocks): + the Q8_0 matrices' bytes of HBM.  The levels
    // below are about the K-quant matrices.
    // level 0: no repack (raw path).  1: repack AND the uploaded GGUF bytes stay resident (K-quant weights x 2 in HBM; round 4's form).
    // 2: ONE resident copy (round 5) -- the GGUF bytes of every repacked matrix are freed after the repack; the launches that read raw blocks
    // (prompt GEMM, the 1:1 ntk_gemv sequence, fallbacks) get the tensor unpacked into a scratch right in front of them (ntk_rp_unpack:
    // byte-exact inverse; + 2 x the model's bytes of HBM traffic per PROMPT PASS whatever its length: 8B Q4_K_M +4 ms = -30 % on a 64-token
    // prompt, -6 % on 1024 tokens; 70B -7 %; decode unchanged).  3 (default): always 2 since round 6 -- the FP16 prompt
    // GEMM reads the repack itself (ntk_gemm_desc.weights_repacked: identical bits, no unpack), so the batched prompt path and the fused decode path need
    // no GGUF bytes of a repacked matrix; what still unpacks into the scratch: the 1:1 launcher sequence (--no-fuse / tests) and the prompt's LM-head GEMV.
    // The repack is made at load unless the option was switched off BEFORE the load; switching after the load works in every direction
    // (2 -> 0 / 1 re-materialises the GGUF bytes from the repack).  Returns a status (NTK_E_NOMEM: the model keeps running on what it has).
    int set_repack(int level);
    bool repack() const { return repack_ != 0; }
    int repack_level() const { return repack_; }
    uint64_t repack_bytes() const { return repack_bytes_; }
    uint64_t resident_weight_bytes() const { return weight_bytes_ - raw_freed_bytes_ + repack_bytes_ + raw_scratch_bytes_; }
    // F16 / BF16 matrices on the fused launches (1, default): the decode pass groups them like quantised ones (ntk_gemv_fused -> gemv_dense16.hip: five
    // launches per layer, norm + LM head in one) and the prompt pass sends them to the F32-MFMA GEMM ahead of the per-token loop.  0: the 1:1 launcher
    // sequence both passes had before (ntk_rmsnorm / ntk_gemv / ntk_add per matrix; one GEMV per token and projection) -- the A/B switch.  Any time;
    // captured graphs are dropped when the setting changes.
    int set_dense_fused(bool on);
    void set_dense_mfma16(bool on) { dense_mfma16_ = on; }   // F16 / BF16 matrices of the batched prompt pass: the 16-bit matrix cores (gemm_dense16.hip) or the F32-MFMA form; any time
    bool fusable(int dt) const;   // a matrix of this dtype goes out on the fused decode launches / the batched prompt GEMM
    void set_bf16_prefill(bool on) { bf16_prefill_ = on; }   // batched prompt: FP16-MFMA (gemm_f16.hip; the option keeps its round-2 name) or the F32-MFMA form (16)
    // which form decode_step_fused(…) emits at the current position: the fused launches of its attention regime
    const char* decode_path() const;
    int check_tp();   // after a sync: NTK_OK, or NTK_E_LAUNCH if the exchange kernel's bounded wait gave up (its error word, surfaced and cleared)
    // parity instrumentation (tests): layers [first, first+count) on caller-supplied hidden states; KV cache rows in / out
    int debug_run_layers(const float* hidden_in, int T, int start_pos, int first, int count, int mode, float* hidden_out);
    int debug_kv(int layer, int pos0, int n, uint16_t* k, uint16_t* v, bool write, int slot = 0);
    // One fused token launched eagerly and timed with HIP events on the compute stream.
    // ms[c] / calls[c] per class c: 0 quant GEMV, 1 attention, 2 everything else (embed, argmax, pos); calls[3] = timed
    // intervals.  fine (coarse = false): an event pair around every launch.  coarse: one event per change of class, so
    // a run of GEMV launches is timed as a whole (kernels + the boundaries between them) and the event cost is per run.
    int profile_token(float ms[4], int calls[4], bool coarse);
    void* stream() const { return stream_; }

    // ---- tensor parallelism (csrc/tp.hip) -------------------------------------------------------------
    // Call before load(): this model object holds slice `rank` of `world` -- rows [rank/world) of Wq, Wk, Wv, gate, up (whole
    // heads), columns of Wo and down -- so config() reports the LOCAL head / FFN counts.  After load(): exchange comm()
    // addresses (tp_export: a hipIpc handle and the raw pointer) and tp_connect() them on every rank before the first forward.
    int tp_configure(int rank, int world);
    int tp_rank() const { return tp_rank_; }
    int tp_world() const { return tp_world_; }
    int tp_export(void* handle64, void** raw);
    int tp_connect(const void* handles, void* const* raws);   // world x 64-byte handles (other processes) or raw pointers (same process)
    unsigned tp_error();                                      // after sync(): 0, or the call that gave up waiting for a peer
    // the host-side column slice of a GGUF matrix: columns [rank * in/world, (rank+1) * in/world) of every row, re-packed
    static int slice_columns(void* dst, const void* src, int dtype, int64_t out_f, int64_t in_f, int rank, int world);

private:
    int load_impl(const std::string& gguf_path, int max_context);
    int finish_load();
    int resolve_rope(const GgufFile* f);   // the rope options + the file (null: synthetic) -> cfg_.rope_theta / rope_freq_scale / rope_scaling_type / rope_orig_ctx / rope_factors, rope_factors_
    int check_layer_extras(const GgufFile& f);   // the bias tensors' type and size, and the per-layer tensors the engine has no kernel for: refusals that name the tensor
    int init_device();               // the GPU NTK_DEVICE names (default 0)
    int own_stream();                 // a private non-blocking stream: sequences and ranks that share a process must not queue behind each other
    int alloc_buffers();
    int upload(DevTensor& dst, const void* host, int dtype, int64_t in_f, int64_t out_f, size_t nbytes);
    // upload this rank's part of a full host tensor [out_f][in_f]: everything, rows [rank * out/world ...), or the column slice
    int upload_shard(DevTensor& dst, const void* host_full, int dtype, int64_t in_f, int64_t out_f, size_t nbytes_full, Shard how);
    // where the GGUF tensor `name` lands, how it is sharded over tensor-parallel ranks and its unsliced extents (false: no such tensor in this model)
    struct TensorSlot { DevTensor* dst; Shard how; int64_t in_f, out_f; };
    bool slot_of(const std::string& name, TensorSlot* slot);
    // every projection matrix that can have a repacked form: the layers' seven, then the LM head
    template <class F> void for_each_projection(F&& fn) { for (auto& L : layers_) for (auto m : kLayerMatrices) fn(L.*m); fn(output_); }
    int repack_all();                 // the repacked form of every K-quant projection (after the upload)
    int repack_one(DevTensor& t);
    int drop_raw_all();               // level 2: free the GGUF bytes of every repacked K-quant matrix (Q8_0 keeps them), size the unpack scratch
    int restore_raw_all();            // ... and back: the GGUF bytes re-materialised from the repack
    // the raw GGUF blocks of a projection for a launch that reads them: the resident bytes, or the tensor unpacked into the scratch (stream
    // ordered; raw_begin() starts a new group of tensors that must be valid together: Q | K | V, gate | up)
    void raw_begin() { raw_cursor_ = 0; }
    const void* raw_of(const DevTensor& t);
    int tp_check_shapes();            // the head / FFN / block divisibility the slices need
    int tp_allreduce(float* hidden, int n);   // hidden += sum over ranks of the partial vectors in the current slot
    float* tp_slot() const;           // where the next partial vector goes
    void free_all();
    void drop_graphs();               // destroy the captured tokens
    // the activations of T tokens in workspace_: q | k | v | attn_out, and gate | up over the same floats once attention is done
    struct Views { float *q, *k, *v, *attn_out, *gate, *up; };
    Views views(int T, bool fused = false) const;   // fused: the single-token path's (attention output and SiLU x up in the static slots when this model owns them)
    int enqueue_token(bool greedy);   // the fused launch sequence for one token
    int enqueue_layers(int first, int last);            // its layer loop
    // y_k = W_k . f(x) for n <= 3 matrices sharing x, in as few fused launches as their formats allow (model_decode.cpp)
    int decode_project(const DevTensor* const* ws, float* const* ys, int n, const float* x, const DevTensor* norm, const float* resid, int kind,
                       int silu_pair = 0, bool timed = true);
    // where the T rows of a layer pass keep their K / V: one slot's cache at rows start_pos .. (forward, score), or -- slots != nullptr -- row t in the cache
    // of slot slots[t] at its own position positions_[t] (decode_batch; max_pos: the largest of them, which picks the attention regime), or -- segs !=
    // nullptr -- the rows are the segments *segs describes (rows, lengths, first positions; the cache pointers are filled per layer) and segment j lives in
    // slot slots[j] (forward_batch)
    struct KvTarget { int slot; const int* slots; int max_pos; const ntk_kv_segments* segs; };
    // the layer loop of forward(), score() (model_prompt.cpp), decode_batch() and forward_batch() (model_batch.cpp)
    int layers_1to1(int T, int start_pos, int first, int last, const KvTarget& kv = KvTarget{0, nullptr, 0, nullptr});
    // one layer's KV step and attention: q | k | v of `act` rotated, k | v stored where `kv` says in the cache's format, act.attn_out = the T rows' attention.
    // fused_store: the prompt form of rotation + store (the pass runs with row maxima).  Returns the first failure; every launch goes out.
    int attend(int layer, int T, int start_pos, const KvTarget& kv, const Views& act, bool fused_store);
    // ---- the steps the host-driven passes share (model_prompt.cpp) ----
    // out [n][H] = the embedding rows of the device ids.  A table format without a kernel is said on stderr and is NOT an error (as the reference).
    int embed_rows(float* out, const int* ids_dev, int n);
    // positions_[0, T) = start_pos, start_pos + 1, ...: queued from host_positions_, which the caller's next synchronisation releases
    int upload_positions(int T, int start_pos);
    // the final RMSNorm of n rows, src -> dst, in the form the LM head wants: returns the rows' largest |x| (in row_max_) where the FP16 GEMM reads the
    // head, null otherwise
    const float* final_norm(float* dst, const float* src, int n, PassStatus& ok);
    // the end of every pass: synchronise, take over what raw_of() could not report through its pointer, and leave `failed` + the status in err_ unless
    // a launcher's own message about a launch failure is already there.  Returns the pass's status.
    int finish_pass(const char* failed, int rc);
    // ntk_gemv over w's raw blocks wp; NTK_E_DTYPE is said on stderr (gemm.cu:801-803) and returned like any status
    int gemv_logged(float* y, const DevTensor& w, const void* wp, const float* x);
    // logits [n][vocab] of the final-normed rows X [n][H] (row_max: their largest |x| or null): one pass over the LM head, in the form score() takes
    int lm_head(float* logits, const float* X, int n, const float* row_max);
    bool lm_head_f16() const;         // ... is the FP16 GEMM
    int lm_head_workspace(const char* who);   // the LM head's own GEMM workspace where gemm_ws_ is too small for vocab rows (score_ws_)
    int batch_buffers();              // the buffers of decode_batch(): at load when sequences > 1, else on its first call
    int batch_logits(const int* slots, const int* tokens, const int* positions, int B);   // decode_batch / _sample up to batch_logits_ (queued)
    int batch_sample_buffers();       // ... and what decode_batch_sample() needs beside them (windows, sampler scratch, pinned mirrors): the same rule
    int score_buffers();              // the buffers of score(), on its first call (and again when score_rows grew)
    // ---- device memory this object owns (model.cpp): freed by free_all() or, one at a time, by dev_release ----
    void* dev_alloc(size_t bytes, bool zero);   // `bytes` + 256 of tail (kernels may read a last 16-byte chunk whole), remembered in allocs_; zero: the `bytes` cleared.  Null: no memory
    void dev_free(void* p);                     // out of allocs_ and back to the device (null: nothing)
    template <class T> void dev_release(T*& p) { dev_free(p); p = nullptr; }
    // a buffer an earlier, failed call obtained is kept: only what is missing is allocated
    template <class T> bool dev_need(T*& p, size_t bytes, bool zero) { if (!p) p = static_cast<T*>(dev_alloc(bytes, zero)); return p != nullptr; }
    void prof_mark(int cls, bool begin);
    // a mixture-of-experts layer's FFN on T rows: x [T][H] -> RMSNorm with ffn_norm -> route -> gate | up -> down, io = io + ... in place (model_decode.cpp).
    // marks: profiler class marks around the launches (the fused token)
    int moe_ffn(const LayerWeights& L, float* io, int T, bool marks);

    ModelConfig cfg_;
    GgufVocab vocab_;
    std::string err_;
    std::vector<LayerWeights> layers_;
    DevTensor token_embd_, output_norm_, output_;
    bool output_tied_ = false;
    uint64_t weight_bytes_ = 0;
    std::vector<void*> allocs_;
    bool shares_weights_ = false;    // the tensor table points into ANOTHER Model's allocations (share_weights): nothing of it is freed here

    // buffers (reference transformer.cpp:330-391)
    KvCache kv_;                    // every slot's K / V cache in the loaded format (kv_cache.h); slot 0 is the one the fused path decodes on
    bool kv_q8_ = false;            // the option (kept across loads)
    int sequences_ = 1;             // the option (kept across loads)
    float* batch_logits_ = nullptr; // [kMaxSequences][V]: decode_batch's logits
    int* batch_in_ = nullptr;       // [3][kMaxSequences] device ints: tokens | positions | -1 (ntk_logprob_rows' "no target")
    int batch_host_[3 * 16] = {};   // ... and their host image
    std::vector<int> packed_tokens_;   // forward_batch's tokens between its H2D copy and its synchronisation (the caller's array may be a temporary)
    float* batch_logprob_ = nullptr;   // [kMaxSequences] (unused result of ntk_logprob_rows)
    int* batch_next_ = nullptr;     // [kMaxSequences] first maxima
    float* batch_attn_scratch_ = nullptr;   // kMaxSequences x the single-row split scratch
    int* batch_recent_ = nullptr;   // [kMaxSequences][kRecentCap] device ints: the rows' repeat-penalty windows (decode_batch_sample)
    int* h_batch_recent_ = nullptr; // pinned staging of it (a step packs its windows at the step's own pitch)
    void* batch_sample_scratch_ = nullptr;   // ntk_sample_rows_scratch_bytes(kMaxSequences, V)
    int* h_batch_next_ = nullptr;   // pinned [kMaxSequences]: the sampled tokens (ntk_sample_rows_top_k's mirror)
    bool batch_kv_q8_ = false;      // the option (kept across loads): sequence slots / the batched step over the 8-bit cache
    float* kv_capture_ = nullptr;   // parity instrumentation (debug_kv_inputs_capture): [2][max_seq][nkv * hd] F32 k (unrotated) and v of one layer's last 1:1 pass
    int kv_capture_layer_ = -1, kv_capture_T_ = 0;
    float* hidden_ = nullptr;       // [max_seq][H]
    float* hidden1_ = nullptr;      // [H]: the fused single-token path's hidden state -- hidden_, or the static slot
    bool static_act_ = true;        // the option (kept across loads)
    bool arena_owner_ = false;      // this model holds the device's static decode slots (released in free_all)
    int arena_device_ = -1;         // ... of this device: ntk_decode_arena_acquire's token
    float* arena_attn_ = nullptr;   // ... its attention-output and SiLU x up slots
    float* arena_gate_ = nullptr;
    float* residual_ = nullptr;     // [max_seq][H]
    float* workspace_ = nullptr;    // max(attention, ffn) floats, shared by all layers
    size_t workspace_floats_ = 0;
    float* logits_ = nullptr;       // [V]
    int score_rows_ = 256;          // the option (kept across loads)
    float* score_logits_ = nullptr; // [score_cap_][V]: one chunk of score()'s logits
    int score_cap_ = 0;
    int* score_targets_ = nullptr;  // [max_seq] each: score()'s targets, log-probabilities and greedy tokens
    float* score_logprob_ = nullptr;
    int* score_top1_ = nullptr;
    void* score_ws_ = nullptr;      // the FP16 GEMM's workspace for the LM head where gemm_ws_ is too small for vocab rows
    size_t score_ws_bytes_ = 0;
    int* positions_ = nullptr;      // [max_seq]
    std::vector<int> host_positions_;   // upload_positions()' host image between its H2D copy and the caller's synchronisation
    int* tokens_dev_ = nullptr;     // [max_seq]
    int* d_pos_ = nullptr;          // device scalar: position of the token being decoded
    int* d_token_ = nullptr;        // device scalar: id of the token being decoded
    int* h_token_ = nullptr;        // pinned mirror of the argmax result
    unsigned long long* h_ring_ = nullptr;   // pinned ring of 4 x {token, position + 1}: ntk_argmax_advance / wait_token
    std::chrono::steady_clock::time_point wait_t0_;
    float* argmax_scratch_ = nullptr;
    void* sample_scratch_ = nullptr;
    int* d_recent_ = nullptr;       // device copy of the repeat-penalty window
    int* h_recent_ = nullptr;       // pinned staging of it
    static constexpr int kRecentCap = kMaxRecent;
    float* rope_inv_freq_ = nullptr; // [hd/2] (1/powf(theta, 2i/hd)) / divisor[i], computed once on the host (rotary.cu:47; rope_build_table)
    std::vector<float> rope_factors_;   // the loaded model's per-pair frequency divisors (host; empty: none -- the prompt-side launches then pass NULL)
    const float* rope_tab() const { return rope_factors_.empty() ? nullptr : rope_inv_freq_; }   // the prompt-side launches' table argument
    RopeScalingOption rope_opt_;     // the options (kept across loads)
    float rope_base_opt_ = 0.0f, rope_scale_opt_ = 0.0f;   // 0: not set
    uint8_t* moe_ws_ = nullptr;      // the routed FFN's workspace (ntk_moe_workspace_layout for max_seq rows, at most 1024); null: a model without experts
    size_t moe_off_[8] = {};         // ... its sections' byte offsets
    int moe_rows_ = 0;               // ... the rows it was sized for
    void* moe_gemm_scratch_ = nullptr;   // ntk_moe_gemm_scratch_bytes for moe_rows_ rows (null where that is 0)
    size_t moe_gemm_scratch_bytes_ = 0;
    bool moe_gemm_ = true;           // option moe_gemm
    int moe_gemm_min_rows_ = kMoeGemmMinRows;   // option moe_gemm_min_rows (1 is accepted and means 2: a one-row pass never takes the GEMM)
    void* stream_ = nullptr;
    bool batched_prefill_ = true;
    struct Timed { int cls; void* a; void* b; int n; bool shared_a; };   // n launches between events a and b
    bool prof_coarse_ = false;
    std::vector<Timed>* prof_ = nullptr;   // non-null while profile_token() runs
    // one captured token per (greedy?, attention regime)
    ihipGraphExec_t* graphs_[2][kAttnRegimes] = {};   // [greedy][attention regime 0..2]
    int host_pos_ = 0;               // host mirror of *d_pos_ (set_device_pos + one per fused step): picks the regime
    int attn_regime_ = 0;            // regime enqueue_token() emits
    float* attn_scratch_ = nullptr;  // partial softmax states of the split-KV attention
    bool prefill_row_max_ = true;    // RMSNorm / SiLU launches of the prompt pass leave the tokens' largest |x| for the FP16 GEMM's pre-pass (A/B switch)
    float* row_max_ = nullptr;       // [2][max_seq]: the prompt tokens' largest |x| beside the RMSNorm / SiLU outputs (FP16 GEMM pre-pass)
    void* gemm_ws_ = nullptr;        // workspace of ntk_gemm_quant_ws (FP16 prompt projections), sized for max(H, I) columns
    void* gemm_ws2_ = nullptr;       // a second one: the launch that produces a projection's input writes that projection's planes (ntk_*_prepare_x) while it may
                                     // still read the previous projection's partial sums out of the other workspace
    bool prefill_fused_split_ = true;   // (A/B switch of that: 0 = the FP16 GEMM's own pre-pass launches)
    size_t gemm_ws_bytes_ = 0;
    bool bf16_prefill_ = true;
    bool dense_fused_ = true;
    bool dense_mfma16_ = true;
    int repack_ = 3;                 // EFFECTIVE level: 0 raw path, 1 repack + raw resident, 2 repack only (one resident copy); 3 only before a load
    int repack_wanted_ = 3;          // the level as ASKED (3 = the default: resolves to 2 at load): re-evaluated by every load
    bool repack_done_ = false;       // repack_all() ran on the loaded tensors
    uint64_t repack_bytes_ = 0;
    uint64_t raw_freed_bytes_ = 0;   // GGUF bytes released after the repack (level 2)
    void* raw_scratch_ = nullptr;    // where raw_of() unpacks to
    size_t raw_scratch_bytes_ = 0, raw_cursor_ = 0;
    int raw_err_ = 0;                // first failure inside raw_of() (it returns a pointer): ok() folds it into the forward's status
    bool attn_merge_ = false;        // split-KV attention without the combine launch (round 5; identical bits, measured 0-2 us per layer SLOWER: opt-in)
    int tp_rank_ = 0, tp_world_ = 1;
    void* tp_comm_ = nullptr;        // this rank's communication buffer (flags + two slots of max_seq x H floats)
    size_t tp_max_floats_ = 0;
    void* tp_peers_[8] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    bool tp_peer_opened_[8] = {false, false, false, false, false, false, false, false};   // mapped through hipIpc (to be closed)
    bool tp_connected_ = false;
    unsigned tp_call_ = 0;           // all-reduce calls of the forward being enqueued (call k uses slot k & 1)
    bool own_stream_ = false;        // tensor-parallel ranks that share a process need private streams
    ModelConfig cfg_full_;           // the unsliced configuration (cfg_ holds the local head / FFN counts)
};

}  // namespace nt
