/* include/ntransformer.h -- public C API of the MI355X-native engine.
 *
 * The first block is the reference's public header (reference include/ntransformer.h:12-38), name for name
 * and signature for signature, so an embedder of the reference re-links without source changes.  The
 * reference DECLARES this API but never implements it (no definition exists under reference src/); the
 * semantics below are the ones its header comments promise.  The second block are extensions.
 * No C++ exception crosses this boundary; every function tolerates a NULL engine.
 */
#ifndef NTRANSFORMER_H
#define NTRANSFORMER_H

#include <stddef.h>
#include <stdint.h>

/* the library is built with -fvisibility=hidden: exactly what this header declares is exported */
#if defined(__GNUC__)
#pragma GCC visibility push(default)
#endif
#ifdef __cplusplus
extern "C" {
#endif

typedef void* nt_engine_t;                       /* opaque handle */

nt_engine_t nt_engine_create(void);              /* never loads anything; NULL only on out-of-memory */
void        nt_engine_destroy(nt_engine_t engine);
int         nt_engine_load(nt_engine_t engine, const char* model_path);   /* 0 = ok (context capped at 4096 like the CLI default) */
/* Returns a malloc'd NUL-terminated UTF-8 string (free with nt_free), NULL on failure.
 * repeat_penalty / seed keep the reference's GenerateConfig defaults (1.1 / 42). */
char*       nt_engine_generate(nt_engine_t engine, const char* prompt, int max_tokens, float temperature,
                               int top_k, float top_p);
void        nt_free(char* ptr);
int         nt_engine_vocab_size(nt_engine_t engine);    /* -1 when no model is loaded */
int         nt_engine_n_layers(nt_engine_t engine);
int         nt_engine_hidden_size(nt_engine_t engine);

/* ------------------------------------------------------------------ extensions ------------------- */
typedef struct nt_gen_params {
    int      max_tokens;
    float    temperature;
    int      top_k;
    float    top_p;
    float    repeat_penalty;
    int      repeat_window;
    uint64_t seed;
    int      stop_at_eos;
} nt_gen_params;

typedef struct nt_stats {      /* Engine::Stats of the reference (engine.h:76-84) */
    int   prompt_tokens;
    int   gen_tokens;
    float prefill_ms;
    float decode_ms;
    float decode_tok_s;
} nt_stats;

typedef struct nt_synth_spec { /* seeded synthetic Llama-shaped model (no checkpoint exists offline) */
    int hidden, inter, layers, heads, kv_heads, vocab, ctx;
    float eps, theta;
    int bos, eos;
    const char* mix;           /* "Q8_0" "Q4_0" "Q4_K" "Q5_K" "Q6_K" "F16" "F32" "Q4_K_M" */
    uint64_t seed;
} nt_synth_spec;

int  nt_engine_load_ex(nt_engine_t e, const char* model_path, int max_context);
int  nt_engine_load_synthetic(nt_engine_t e, const nt_synth_spec* spec, int max_context);
/* A second SEQUENCE over the weights `src` already holds resident (the path shards across requests; sequences share nothing but the
 * read-only weights): `e` gets src's tensors (nothing is copied or owned), its own KV caches, activation buffers and HIP stream, so two host threads
 * can decode two requests on one GPU at once (bench.py: 8b_q8_0_x2_per_gpu).  `src` must outlive `e` and must not be re-loaded or change its
 * "repack" level meanwhile; a tensor-parallel source is refused (NTK_E_SHAPE). */
int  nt_engine_load_shared(nt_engine_t e, nt_engine_t src, int max_context);
/* "fused" / "graph" / "device_sampling" / "batched_prefill" / "f16_prefill" (alias "bf16_prefill") = "0" | "1"; "dense_fused" = "1" (default) | "0", any time: the
 * matrices of an unquantised model (F16, BF16) on the fused decode GEMV (five launches per layer, as a quantised model) and on the batched prompt GEMM, or
 * ("0") on the 1:1 launcher sequence -- one GEMV per matrix and token; the A/B switch of profiles/dense16.txt; "persistent" / "fuse_attention" are accepted
 * and do nothing (the structures they selected lost to the fused launches and were removed: profiles/NEGATIVE_RESULTS.md); "repack" = "0" raw-GGUF decode GEMVs | "1" load-time repack with the GGUF
 * bytes kept resident (K-quant weights twice in HBM) | "2" one resident copy: the GGUF bytes of a repacked matrix are freed and unpacked into a scratch
 * for the launches that read raw blocks (prompt GEMM, 1:1 sequence; a fixed cost per prompt pass) | "3" (default) "2" when both copies would leave less than
 * a fifth of the device's memory free, else "1"; "attention_merge" = "1" split-KV decode attention as one launch | "0" (default) with the separate merge
 * launch (identical results; the one-launch form measured slower);
 * "kv_cache" = "f16" (default) | "q8_0": the KV cache as GGUF Q8_0 values along head_dim (one half scale + 32 int8 per 32 elements of a head's row,
 * quantised from the F32 post-RoPE k and the F32 v: 1.0625 bytes per element instead of 2, plus ONE layer's F16 image of max_context rows shared by all
 * layers).  Set it BEFORE the load (afterwards: NTK_E_SHAPE + last_error); an nt_engine_load_shared sequence takes its own option.  Decode steps read
 * the 8-bit rows on the matrix cores using half(d) * q exactly; prompt passes (and "fused" = "0") dequantise rows [0, start_pos + n) into the F16 image
 * -- rounded to half, the chunk's own rows included -- and run the F16 attention kernels over it.  Refused at load (NTK_E_SHAPE + last_error): head_dim
 * other than 128, more than 16 query heads per KV head, tensor parallelism;
 * "sequences" = "1" .. "16" (default "1"): sequence slots of this engine for the batched decode step below.  Slot 0 is the KV cache every other entry point
 * uses, exactly as without the option; slots 1 .. N - 1 are extra F16 caches of the same layout, allocated at load (counted in nt_engine_kv_cache_bytes)
 * beside a [16][vocab] F32 logits buffer and the batched sampler's buffers (under 1 MB; neither is counted there).  Set it BEFORE the load (afterwards:
 * NTK_E_SHAPE + last_error); an nt_engine_load_shared sequence takes its own.
 * Refused at load (NTK_E_SHAPE + last_error) when > 1 together with "kv_cache" = "q8_0" (unless "batch_kv_q8"), tensor parallelism or a context of fewer
 * than N positions;
 * "batch_kv_q8" = "0" (default) | "1" (any other value: NTK_E_SHAPE + last_error): sequence slots and the batched decode step over the 8-bit KV cache.
 * Set it BEFORE the load (afterwards: NTK_E_SHAPE + last_error); it is kept across loads; an nt_engine_load_shared sequence takes its own.  With "1" and
 * "kv_cache" = "q8_0", "sequences" = "1" .. "16" loads -- slot 0 is the 8-bit cache every other entry point uses, slots 1 .. N - 1 are further 8-bit caches
 * of the same layout, zeroed at load; the one-layer F16 image stays ONE per engine, rebuilt by every prompt pass for the slot it runs on, so
 * nt_engine_kv_cache_bytes = sequences x the 8-bit caches + one image -- and nt_engine_decode_batch / _decode_batch_sample / _generate_batch / _generate_batch_ex
 * run (one row on a one-slot engine included): each row's attention is the single-sequence 8-bit decode kernel's, bit for bit at the same split count.
 * With "kv_cache" = "f16" the option is accepted and changes nothing.  With "0" every refusal and message is what it was before the option existed.
 * (The option exists ONLY because the default refusal of "sequences" > 1 with "q8_0" is pinned by a test; a later change that may touch that test can
 * fold the option away and make this the behaviour of "sequences" + "q8_0".);
 * "static_activations" = "1" (default) | "0" (any other value: NTK_E_SHAPE + last_error): the fused single-token path keeps its hidden state, attention
 * output and SiLU x up vector in the library's static decode slots (ntk_decode_arena_*, ntk_engine.h), where the Q8_0 decode GEMVs request them before their
 * kernel arguments have arrived.  Set it BEFORE the load (afterwards: NTK_E_SHAPE + last_error); kept across loads.  One engine per process and device holds
 * the slots, from its load to its close: the first to ask.  Any other engine, an nt_engine_load_shared sequence, tensor-parallel ranks and models beyond a
 * slot's size run the same launches on buffers of their own, as with "0".  The results are the same bits either way; nt_engine_decode_path says which ran;
 * "score_rows" = "1" .. "1024" (default "256"): rows of logits nt_engine_score_tokens computes per pass over the LM head (score_rows x vocab floats of device
 * memory from the first scoring call on; any time);
 * "context_shift" = "0" (default) | "1" (any other value: NTK_E_SHAPE + last_error; any time before a generate call, kept across loads): what the generate loop
 * behind nt_engine_generate, nt_engine_generate_tokens and the CLI does when the sequence reaches max_context.  "0": it prints
 * "[context of N tokens exhausted]" and stops, as ever.  "1": a CONTEXT SHIFT -- with keep = min("context_keep", max_context - 2) and discard =
 * nt_context_shift_discard(position, keep) it runs nt_engine_kv_shift(slot 0, keep, discard, position), goes on at position - discard and so returns
 * every token asked for.  The repeat-penalty window is over tokens and does not change.  A prompt longer than the context stays refused.
 * nt_engine_generate_batch / _ex keep dropping a sequence at the end of its context (a caller who drives nt_engine_decode_batch can shift a slot itself);
 * "context_keep" = N >= 0 (default "1"; otherwise NTK_E_SHAPE + last_error; any time, kept across loads): the leading positions a context shift never
 * discards -- the default keeps the BOS;
 * "batch_prefill" = "0" (default) | "1" (any other value: NTK_E_SHAPE + last_error; any time, read per call): with "1" nt_engine_generate_batch / _ex prefill
 * all their prompts with ONE nt_engine_forward_batch pass (below) instead of one nt_engine_seq_forward per slot; everything behind the prefill -- the first
 * token from each sequence's own row of logits, the lockstep steps -- is unchanged.  Ignored (slot by slot, as with "0") on a "kv_cache" = "q8_0" engine and
 * when the prompts together hold more tokens than max_context;
 * RoPE FREQUENCY SCALING -- three options, all BEFORE the load (afterwards: NTK_E_SHAPE + last_error), kept across loads, malformed values NTK_E_SHAPE +
 * last_error; an nt_engine_load_shared sequence runs with its source's table and scale whatever its own options say:
 * "rope_scaling" = "file" (default): what the GGUF says -- the tensor rope_freqs.weight (F32 [head_dim / 2] per-pair frequency DIVISORS, Llama 3.1 / 3.2)
 * and <arch>.rope.scaling.type = "linear" with .factor (or the legacy <arch>.rope.scale_linear): freq_scale = 1 / factor; "yarn" and unknown types load
 * unscaled with one line on stderr | "none": the file's factors and scaling keys are ignored (the engine's behaviour before it read them) | "linear:<factor>":
 * freq_scale = 1 / factor whatever the file's scaling keys say, while the file's rope_freqs.weight divisors STAY (as under llama.cpp's --rope-scaling linear)
 * | "llama3:<factor>,<low_freq_factor>,<high_freq_factor>,<original_context>": the engine computes the Llama-3.1 divisors itself (nt_rope_llama3_factors), in
 * place of the file's --
 * the way a synthetic model gets a Llama-3.1-shaped rotation.  The angle of pair i at position pos is (float)pos * tab[i] * freq_scale, left to right in F32,
 * tab[i] = (1 / powf(theta, 2i / head_dim)) / divisor[i] (nt_rope_build_table);
 * "rope_freq_base" = F > 0: theta, overriding the file's <arch>.rope.freq_base (a synthetic spec's theta);
 * "rope_freq_scale" = F > 0: freq_scale, overriding whatever "rope_scaling" resolved to. */
int  nt_engine_set_option(nt_engine_t e, const char* key, const char* value);
const char* nt_engine_last_error(nt_engine_t e);
void nt_gen_params_default(nt_gen_params* p);
/* The generate loop on token ids; writes up to out_cap generated ids, returns their count or a negative NTK_E_* */
int  nt_engine_generate_tokens(nt_engine_t e, const int* prompt, int n_prompt, const nt_gen_params* p, int* out, int out_cap);
int  nt_engine_last_stats(nt_engine_t e, nt_stats* out);
/* Transformer::forward: tokens [n] at start_pos -> logits of the last position copied to host (vocab floats) */
int  nt_engine_forward(nt_engine_t e, const int* tokens, int n, int start_pos, float* logits_out);
/* ---- sequence slots: several requests per pass over the weights ("sequences" option) -------------------------------------------------------
 * ARITHMETIC CONTRACT of the batched step: every row is computed with the PROMPT PASS's arithmetic -- projections on the FP16 matrix cores with two FP16
 * pieces per activation -- and the decode kernels' attention; NOT the decode GEMV's arithmetic.  A sequence's logits therefore agree with its solo
 * nt_engine_decode_fused run to the project's 1e-3 bar, not bit for bit, and its greedy stream may differ at a near tie.  Within one batch size a row's
 * result depends on nothing but that row (every output element of the GEMM is accumulated on its own, the launch form is chosen by the row count alone):
 * companions, their order and their slots do not matter.  No bit claim across batch sizes.
 * nt_engine_seq_forward: nt_engine_forward into the KV cache of sequence slot `slot` (slot 0: the same call as nt_engine_forward, bit for bit).
 * nt_engine_decode_batch: ONE decode step of n sequences: row i = token tokens[i] of the sequence in slots[i] at position positions[i] (its K / V row is
 * stored there, attention runs over rows 0 .. positions[i] of that slot).  logits_out [n][vocab] and next_out [n] (each row's greedy token: first maximum)
 * may each be NULL.  Eager, one synchronisation; leaves the fused path's slot-0 state (device position / token, captured graphs) alone.  Refused
 * (NTK_E_SHAPE + last_error; the engine stays usable): n outside 1 .. "sequences", a slot out of range or named twice, a position outside the context,
 * a token id out of range.
 * nt_engine_generate_batch: n prompts (prompts[i][0 .. prompt_lens[i])) generated in lockstep, GREEDY: prompt i is prefilled into slot i, then all live
 * sequences step together; a sequence leaves the batch at EOS (stop_at_eos; the EOS token is written) or at max_tokens.  out [n][out_stride] receives the
 * generated ids, out_counts [n] how many.  Returns n or a negative NTK_E_*; temperature > 0 or repeat_penalty != 1: NTK_E_SHAPE + last_error (sample from
 * nt_engine_decode_batch's logits instead).  nt_engine_last_stats: prompt and generated tokens summed over the sequences (as nt_engine_generate_tokens
 * counts them: without each sequence's first token), the aggregate decode rate.
 * SAMPLED batches, every sequence with its own settings.  CONTRACT: the sampled stream = the host sampler (reference src/inference/sampler.cpp) on the
 * batched step's logits -- ntk_sample_rows_top_k runs the single-sequence device sampler's code on every row, the uniform draws come from one
 * std::mt19937 per sequence on the host.
 * nt_engine_decode_batch_sample: ONE step, caller-driven: nt_engine_decode_batch with row i sampled on the device by params[i] (temperature, top_k, top_p,
 * repeat_penalty; max_tokens / stop_at_eos / seed / repeat_window ignored) over the window recent[i][0 .. n_recent[i]) -- the caller passes the window it
 * wants applied, the last repeat_window tokens (recent / n_recent may be NULL: no windows) -- with the uniform draw r[i] (ignored where temperature <= 0:
 * that row gets the first maximum of its penalised logits; r may be NULL when no row is sampled).  logits_out [n][vocab] (may be NULL) receives the logits
 * BEFORE any penalty: nt_engine_decode_batch's bits.  next_out [n]: the tokens.  One synchronisation, no logits download unless asked for.  Refused
 * (NTK_E_SHAPE + last_error; the engine stays usable) as nt_engine_decode_batch, and: a sampled row with top_k outside 1 .. 64 or top_k >= vocab, a
 * vocabulary beyond 131 072, an n_recent[i] outside 0 .. 4096.
 * nt_engine_generate_batch_ex: nt_engine_generate_batch with params[i] = sequence i's temperature, top_k, top_p, repeat_penalty, repeat_window, seed,
 * max_tokens and stop_at_eos.  Sequence i has its own sampler seeded with params[i].seed; its first token is sampled on the host from the prefill logits
 * (penalty over the prompt, then the draw), every further one on the device in the lockstep step, with the window = the last min(have, repeat_window) ids
 * of prompt + generated -- the stream nt_engine_generate_tokens' sampler would produce on those logits.  A sequence whose settings the device sampler
 * does not take (top_k <= 0, > 64 or >= vocab; repeat_window > 4096) is sampled by its host sampler from its own row of logits (vocab floats per step).
 * A sequence leaves at its own max_tokens, at EOS if its own stop_at_eos is set, or at the end of the context; out_stride must hold the largest
 * max_tokens.  Returns n or a negative NTK_E_*; stats as nt_engine_generate_batch. */
/* ---- the packed prompt pass: the tokens of several sequences in ONE pass over the weights --------------------------------------------------------
 * nt_engine_forward_batch: the rows of the pass are n SEGMENTS back to back; segment i = lens[i] consecutive tokens of the sequence in slot slots[i], the
 * first at position start_pos[i] of that slot's cache; `tokens` holds sum(lens) ids, segment after segment.  Every segment's K / V rows are stored at
 * [start_pos[i], start_pos[i] + lens[i]) of its slot and its rows attend causally over rows 0 .. their own position of that slot alone.  So one call
 * prefills several prompts (start 0), continues a chunked prefill (start > 0), steps decoding sequences (one token at their position) or mixes the three.
 * logits_out [n][vocab]: the logits behind each segment's LAST token; next_out [n]: their first maxima; each may be NULL.  Eager, one synchronisation;
 * leaves the fused path's slot-0 state alone.
 * ARITHMETIC CONTRACT: (1) a segment's logits agree with nt_engine_seq_forward of the same tokens to the project's 1e-3 bar, not bit for bit (the LM head runs
 * in nt_engine_decode_batch's form, and the GEMM form follows the pass's TOTAL row count); (2) a call with ONE segment of two tokens or more leaves exactly
 * the cache rows nt_engine_seq_forward(slot, tokens, start_pos) leaves, in every layer; (3) within one total row count a segment's logits and cache rows
 * depend on nothing but that segment -- not on its companions, their order, its row offset in the pass or the slot numbers; (4) no bit claim across total
 * row counts; (5) no performance claim for one-token segments at long contexts: nt_engine_decode_batch stays the step for pure decoding; (6) caches of
 * slots not named, and rows of a named slot outside its segment, are not written.
 * Refused (NTK_E_SHAPE + last_error, nothing launched, the engine stays usable): n outside 1 .. "sequences", a slot out of range or named twice, a length
 * below 1, a negative start, start + length beyond max_context, more than max_context tokens in all, a token id out of range, "kv_cache" = "q8_0" (with or
 * without "batch_kv_q8": the prompt path's single one-layer F16 image cannot hold several slots at once), a tensor-parallel engine.
 * nt_forward_batch_validate: TEST SUPPORT, host only (no engine, no device): those argument checks (token ids aside) for an engine of `sequences` slots and
 * `max_seq` positions -- NTK_OK, NTK_E_NULL or NTK_E_SHAPE. */
int  nt_engine_forward_batch(nt_engine_t e, const int* slots, const int* tokens, const int* lens, const int* start_pos, int n, float* logits_out,
                             int* next_out);
int  nt_forward_batch_validate(const int* slots, const int* lens, const int* start_pos, int n, int sequences, int max_seq);
int  nt_engine_seq_forward(nt_engine_t e, int slot, const int* tokens, int n, int start_pos, float* logits_out);
int  nt_engine_decode_batch(nt_engine_t e, const int* slots, const int* tokens, const int* positions, int n, float* logits_out, int* next_out);
int  nt_engine_generate_batch(nt_engine_t e, const int* const* prompts, const int* prompt_lens, int n, const nt_gen_params* p, int* out, int out_stride,
                              int* out_counts);
int  nt_engine_decode_batch_sample(nt_engine_t e, const int* slots, const int* tokens, const int* positions, int n, const nt_gen_params* params,
                                   const int* const* recent, const int* n_recent, const float* r, float* logits_out, int* next_out);
int  nt_engine_generate_batch_ex(nt_engine_t e, const int* const* prompts, const int* prompt_lens, int n, const nt_gen_params* params, int* out,
                                 int out_stride, int* out_counts);
/* ---- KV cache sequence operations (csrc/kv_ops.hip; llama.cpp's seq_rm + seq_add, and seq_cp) ------------------------------------------------------
 * nt_engine_kv_shift: the CONTEXT SHIFT of sequence slot `slot` (0 on a one-slot engine) whose cache holds n_past positions: positions [keep, keep +
 * discard) are dropped and rows [keep + discard, n_past) of every layer move down to [keep, ...), in the cache format the engine was loaded with.  V rows
 * move byte for byte; K rows -- cached after RoPE -- are rotated by -discard positions with the engine's frequency table, so they are the keys the model
 * would have cached at the new positions: to half an ulp of half per shift ("kv_cache" = "f16"), to half a quantisation step per shift ("q8_0": the head
 * is dequantised, rotated and requantised).  Rows below keep, rows from the new n_past upward and every other slot keep their bytes.  Queued on the
 * engine's stream (one launch whatever the overlap), no synchronisation.  Returns the new n_past = n_past - discard, where the caller's next token goes.
 * The fused path's device position is not touched: nt_engine_decode_fused / _decode_greedy_steps / the generate calls re-base it themselves.
 * nt_engine_kv_copy: rows [pos0, pos0 + n) of every layer and both sides from slot src_slot to slot dst_slot at the same positions, no rotation
 * (stream-ordered device-to-device copies): a prefix prefilled once into one slot serves the others.  Returns n.
 * Both: works with "kv_cache" = "f16" and "q8_0" (slots of a q8_0 engine: "batch_kv_q8"), "fused" = "0" and "1".  Refused with NTK_E_SHAPE + last_error, the
 * engine staying usable: a slot outside 0 .. "sequences" - 1, src_slot == dst_slot, rows or n_past outside 0 .. max_context, keep < 0, discard < 1,
 * keep + discard > n_past, a tensor-parallel engine.
 * nt_kv_shift_validate / nt_kv_copy_validate: TEST SUPPORT, host only (no engine, no device): those argument checks for an engine of `sequences` slots and
 * `max_seq` positions -- NTK_OK or NTK_E_SHAPE.  nt_context_shift_discard: the generate loop's discard rule, max(1, (n_past - keep) / 2). */
int  nt_engine_kv_shift(nt_engine_t e, int slot, int keep, int discard, int n_past);
int  nt_engine_kv_copy(nt_engine_t e, int src_slot, int dst_slot, int pos0, int n);
int  nt_kv_shift_validate(int slot, int keep, int discard, int n_past, int sequences, int max_seq);
int  nt_kv_copy_validate(int src_slot, int dst_slot, int pos0, int n, int sequences, int max_seq);
int  nt_context_shift_discard(int n_past, int keep);
/* Scoring: logprob_out[i] = log P(targets[i] | tokens[0..i]) (natural log) for targets[i] >= 0, 0 where targets[i] < 0; top1_out (optional, may be NULL):
 * the greedy token behind tokens[0..i] for every i.  Runs the prompt pass over tokens at start_pos (the KV cache afterwards = nt_engine_forward's), then
 * the LM head over "score_rows" positions at a time; returns the number of scored positions or a negative NTK_E_* (+ nt_engine_last_error: an id out of
 * range, n + start_pos beyond the context, a tensor-parallel engine, no device memory for the first call's buffers -- the engine stays usable). */
int  nt_engine_score_tokens(nt_engine_t e, const int* tokens, const int* targets, int n, int start_pos, float* logprob_out, int* top1_out);
/* one fused decode step for `token` at position `pos` (device-resident state), logits copied to host */
int  nt_engine_decode_fused(nt_engine_t e, int token, int pos, int use_graph, float* logits_out);
/* n greedy decode steps from (token, pos): exactly the timed inner loop of generate (device argmax, one host
 * sync per token); generated ids to out[n] (may be NULL) */
int  nt_engine_decode_greedy_steps(nt_engine_t e, int token, int pos, int n, int* out);
/* one fused token launched eagerly and timed with HIP events on the compute stream:
 * ms4/calls4[0] quantised GEMV launches, [1] attention, [2] embedding + argmax + position; calls4[3] = timed intervals.
 * coarse = 0: an event pair around every launch; coarse = 1: one event per change of launch class (a run of GEMV
 * launches is timed as a whole: event cost paid once per run, the boundaries inside a run included) */
int  nt_engine_profile_token(nt_engine_t e, int token, int pos, int coarse, float* ms4, int* calls4);
int  nt_engine_tokenize(nt_engine_t e, const char* text, int add_bos, int* out, int out_cap);   /* returns count */
int  nt_engine_detokenize(nt_engine_t e, const int* ids, int n, char* out, int out_cap);       /* returns bytes */
uint64_t nt_engine_bytes_per_token(nt_engine_t e, int pos);   /* algorithmic HBM bytes of one decode token */
uint64_t nt_engine_kv_cache_bytes(nt_engine_t e);          /* resident KV cache of this sequence, all its slots ("kv_cache" = "q8_0": the slots' 8-bit caches + the ONE one-layer F16 image) */
uint64_t nt_engine_weight_bytes(nt_engine_t e);            /* the model's tensors in their GGUF encoding */
uint64_t nt_engine_resident_weight_bytes(nt_engine_t e);   /* what they occupy in HBM now: GGUF bytes still resident + the decode repack + the unpack scratch */
uint64_t nt_engine_repacked_bytes(nt_engine_t e);          /* of which the decode repack (tensors that did not fit stay on the raw path and are not counted) */
int  nt_engine_max_context(nt_engine_t e);
/* which form the fused decode step takes: "fused (5 launches/layer)", or "fused (5 launches/layer; static activations)" when this engine
 * holds the device's static decode slots */
const char* nt_engine_decode_path(nt_engine_t e);
/* Tensor-parallel decoding over `world` GPUs, one engine (normally one process) per rank -- SURVEY 8(f) rank 4, no reference
 * counterpart.  nt_engine_tp_configure BEFORE load: the engine then keeps rows [rank/world) of Wq/Wk/Wv/gate/up (whole heads) and
 * the matching columns of Wo/down; n_heads, n_kv_heads and the FFN width must divide by `world`, column slices must be whole
 * quantisation blocks.  After load: nt_engine_tp_export gives this rank's communication buffer as a 64-byte hipIpc handle
 * (other processes) and as a raw device pointer (ranks sharing a process); every rank then calls nt_engine_tp_connect with
 * world x 64 bytes of handles OR world raw pointers, in rank order.  Every rank must then run the same calls with the same
 * tokens: after Wo and after down the ranks' partial vectors are added in rank order by one kernel that reads the peers'
 * buffers over xGMI (ntk_tp_allreduce_add), so hidden states, logits and sampled tokens are bit-identical on all ranks.
 * nt_engine_tp_error after a call: 0, or non-zero if a bounded wait for a peer gave up. */
int  nt_engine_tp_configure(nt_engine_t e, int rank, int world);
int  nt_engine_tp_export(nt_engine_t e, void* handle64, void** raw_ptr);
int  nt_engine_tp_connect(nt_engine_t e, const void* handles, void* const* raw_ptrs);
unsigned nt_engine_tp_error(nt_engine_t e);
/* host only: columns [rank * in/world, (rank + 1) * in/world) of every row of a GGUF matrix, re-packed row-major into dst */
int  nt_tp_slice_columns(void* dst, const void* src, int dtype, int64_t out_features, int64_t in_features, int rank, int world);
/* ---- parity instrumentation (tests/test_parity_depth.py; never used by generate) --------------------------------------------
 * nt_engine_debug_run_layers: layers [first, first + count) of the loaded model on CALLER-SUPPLIED hidden states -- hidden_in
 * [n_tokens][hidden] (host) in, hidden_out [n_tokens][hidden] (host) out -- for tokens at positions start_pos...: layer-wise teacher
 * forcing against a checker (no error amplification through depth).  mode 0: the reference's 1:1 launcher sequence (prompt
 * projections batched or per token, as "batched_prefill" says); mode 1: the fused single-token launches (n_tokens == 1); mode 2: the
 * same captured into a hipGraph and replayed.  The layers write the KV-cache rows of these positions as in a normal forward.
 * nt_engine_debug_kv_read / _write: rows [pos0, pos0 + n) of one layer's K and V cache, [n][n_kv_heads * head_dim] IEEE halves. */
int  nt_engine_debug_run_layers(nt_engine_t e, const float* hidden_in, int n_tokens, int start_pos, int first_layer, int n_layers,
                                int mode, float* hidden_out);
int  nt_engine_debug_kv_read(nt_engine_t e, int layer, int pos0, int n, uint16_t* k_out, uint16_t* v_out);
int  nt_engine_debug_kv_write(nt_engine_t e, int layer, int pos0, int n, const uint16_t* k, const uint16_t* v);
/* TEST SUPPORT, host only (no engine, no device): the argument checks of nt_engine_decode_batch for an engine of `sequences` slots, `max_seq` positions and
 * `vocab` ids -- NTK_OK, NTK_E_NULL or NTK_E_SHAPE (tests/test_batch_validate_cpu.py) */
int  nt_batch_validate(const int* slots, const int* tokens, const int* positions, int n, int sequences, int max_seq, int vocab);
int  nt_engine_debug_kv_read_slot(nt_engine_t e, int slot, int layer, int pos0, int n, uint16_t* k_out, uint16_t* v_out);   /* ... of sequence slot `slot` */
int  nt_engine_debug_kv_write_slot(nt_engine_t e, int slot, int layer, int pos0, int n, const uint16_t* k, const uint16_t* v);   /* _write into slot `slot`, the same checks */
/* ... of a "kv_cache" = "q8_0" engine: the rows as canonical 34-byte GGUF block_q8_0 {half d; int8 q[32]}, [n][n_kv_heads * head_dim / 32] blocks per
 * side.  Each pair returns NTK_E_DTYPE on an engine of the other cache format. */
int  nt_engine_debug_kv_read_q8(nt_engine_t e, int layer, int pos0, int n, void* k_blocks_out, void* v_blocks_out);
int  nt_engine_debug_kv_write_q8(nt_engine_t e, int layer, int pos0, int n, const void* k_blocks, const void* v_blocks);
/* ... of sequence slot `slot` of a q8_0 engine ("batch_kv_q8"; slot 0: the calls above): the checks of the F16 slot pair -- a slot outside
 * 0 .. "sequences" - 1: NTK_E_SHAPE -- and NTK_E_DTYPE on an F16 engine */
int  nt_engine_debug_kv_read_q8_slot(nt_engine_t e, int slot, int layer, int pos0, int n, void* k_blocks_out, void* v_blocks_out);
int  nt_engine_debug_kv_write_q8_slot(nt_engine_t e, int slot, int layer, int pos0, int n, const void* k_blocks, const void* v_blocks);
/* The F32 inputs of the KV store: after nt_engine_debug_kv_inputs_capture(layer) every prompt pass / 1:1 pass leaves that layer's k projection (BEFORE
 * the rotation) and v projection aside; _read returns those of the last pass, [n][n_kv_heads * head_dim] floats each (n <= its token count).  layer < 0: off. */
int  nt_engine_debug_kv_inputs_capture(nt_engine_t e, int layer);
int  nt_engine_debug_kv_inputs_read(nt_engine_t e, int n, float* k_out, float* v_out);
/* write a synthetic GGUF v3 file with the same generator (0 = ok) */
int  nt_synth_write_gguf(const char* path, const nt_synth_spec* spec, int nthreads);
/* fill one tensor of the synthetic plan into host memory (for CPU baselines); returns bytes or negative */
int64_t nt_synth_tensor(const nt_synth_spec* spec, const char* name, void* dst, size_t dst_cap, int nthreads);


/* ------------------------------------------------------------------ host-only entry points ---------
 * GGUF parsing, tokenisation and sampling never touch the GPU; these let tools (and the CPU test-suite)
 * use them without a device. */
/* JSON description of a GGUF file: config, tensor table, vocab size. Returns bytes needed (excl. NUL) or negative.  RoPE scaling as the FILE states it:
 * "rope_scaling_type" (<arch>.rope.scaling.type; "linear" for a bare legacy rope.scale_linear; "none" without either), "rope_freq_scale" (1 / factor for
 * linear, else 1), "rope_factors" (elements of rope_freqs.weight, 0 without the tensor), "rope_orig_ctx" (.original_context_length, 0 when absent).
 * "qkv_bias_tensors": how many blk.*.attn_{q,k,v}.bias tensors the file carries (3 per layer in a Qwen2 file, 0 in a Llama file); "qk_norm_tensors": how
 * many blk.*.attn_{q,k}_norm.weight (2 per layer in a Qwen3 file).  "head_dim" is <arch>.attention.key_length where the file has the key (Qwen3,
 * Mistral-Nemo: heads x head_dim differs from the hidden size), hidden_size / n_heads otherwise. */
int   nt_gguf_describe(const char* path, char* json_out, int cap);
/* In how many layers the LOADED engine adds a Q | K | V projection bias (blk.N.attn_{q,k,v}.bias, each optional, F32, one value per output row, added
 * ahead of the rotation: ntk_qkv_bias); 0 for a Llama model, whose launches are unchanged; -1 without a loaded engine. */
int   nt_engine_qkv_bias(nt_engine_t e);
/* In how many layers the LOADED engine normalises every head of Q and K (blk.N.attn_q_norm.weight + attn_k_norm.weight, F32 [head_dim], a pair per layer;
 * RMSNorm behind the bias and ahead of the rotation: ntk_qk_norm); 0 for a Llama or Qwen2 model, whose launches are unchanged; -1 without a loaded engine. */
int   nt_engine_qk_norm(nt_engine_t e);
/* How many layers of the loaded model are mixture-of-experts layers (blk.N.ffn_gate_inp.weight + ffn_{gate,up,down}_exps.weight: their FFN is
 * ntk_rmsnorm -> ntk_moe_route -> ntk_moe_gate_up -> ntk_moe_down, the experts chosen on the device); *experts / *used (each optional) receive the
 * expert count E and the experts per token K, 0 for a model without such a layer, whose launches are unchanged; -1 without a loaded engine.
 * nt_gguf_describe reports "expert_count", "expert_used_count", "expert_feed_forward_length" (0 where the file names none) and "moe_layers". */
int   nt_engine_moe(nt_engine_t e, int* experts, int* used);
/* The rotation a LOADED engine runs with, as JSON: "rope_theta", "rope_scaling_type" ("none" | "linear" | "llama3"; a file's "yarn" / unknown type is
 * reported as it is named, and is not applied), "rope_freq_scale", "rope_factors" (per-pair divisors folded into the frequency table: 0 or head_dim / 2),
 * "rope_orig_ctx".  Returns bytes needed (excl. NUL) or negative. */
int   nt_engine_rope_info(nt_engine_t e, char* json_out, int cap);
/* Llama-3.1 frequency divisors (what a converter writes into rope_freqs.weight): out[head_dim / 2], computed in double, stored as F32.  Pair i of
 * wavelength 2 pi theta^(2i / head_dim): 1 below orig_ctx / high, `factor` above orig_ctx / low, 1 / ((1 - s) / factor + s) with s = (orig_ctx / wavelen -
 * low) / (high - low) in between.  NTK_E_SHAPE: head_dim odd or < 2, theta / factor / low / high / orig_ctx not > 0, high == low. */
int   nt_rope_llama3_factors(int head_dim, float theta, float factor, float low_freq_factor, float high_freq_factor, int orig_ctx, float* out);
/* The engine's frequency table: out[i] = (1.0f / powf(theta, (2.0f * i) / head_dim)) / factors[i] in F32 (factors NULL: no division -- the plain table). */
int   nt_rope_build_table(int head_dim, float theta, const float* factors_or_null, float* out);
typedef void* nt_tokenizer_t;
nt_tokenizer_t nt_tokenizer_open(const char* gguf_path);       /* NULL on failure */
void  nt_tokenizer_close(nt_tokenizer_t t);
int   nt_tokenizer_encode(nt_tokenizer_t t, const char* text, int text_len, int add_bos, int* out, int cap);
int   nt_tokenizer_decode(nt_tokenizer_t t, const int* ids, int n, char* out, int cap);
int   nt_tokenizer_is_gpt2(nt_tokenizer_t t);
/* n_draws successive Sampler::sample calls on the same logits (penalty applied once per draw over `recent`) */
int   nt_sampler_draw(const float* logits, int n, const nt_gen_params* p, const int* recent, int n_recent,
                      int n_draws, int* out);
/* TEST SUPPORT, host only: a sampler seeded with p->seed, `skip` draws discarded, then ONE repeat penalty over recent[0 .. n_recent) (its last
 * repeat_window entries) + one sample on a copy of `logits`: draw number `skip` of nt_sampler_draw's stream, given the window it had then */
int   nt_sampler_draw_nth(const float* logits, int n, const nt_gen_params* p, const int* recent, int n_recent, int skip, int* out);
/* the first n uniform draws a sampler seeded with `seed` consumes (one per sampled token) */
int   nt_sampler_uniforms(uint64_t seed, int n, float* out);

#ifdef __cplusplus
}
#endif
#if defined(__GNUC__)
#pragma GCC visibility pop
#endif
#endif /* NTRANSFORMER_H */
