/* include/ntk_engine.h -- the engine-private part of libntransformer_hip.so's C ABI (round 6: split off include/ntk.h, which keeps the
 * reference's surface -- the 17 launchers of reference src/cuda/kernels.h:14-71 and the nt_cuda_* runtime of src/core/device.h:79-88).
 *
 * What is here has NO counterpart in the reference's headers: fused forms of launcher sequences (each cites the sequence it computes), the
 * engine-owned repack and the matrix-core GEMV that reads it, the prompt projections on the matrix cores, the split-KV decode attention,
 * device-side embedding / sampling, the tensor-parallel exchange, and parity / measurement instrumentation (ntk_debug_*).  Same conventions
 * as ntk.h: plain pointers and sizes, stream ordered, no allocation, NTK_OK or a negative NTK_E_* code.  Used by csrc/engine/ (nt_engine_*),
 * integration/nt_hip_repack.h, the tests and bench.py.
 */
#ifndef NTK_ENGINE_H
#define NTK_ENGINE_H

#include "ntk.h"

#if defined(__GNUC__)
#pragma GCC visibility push(default)
#endif
#ifdef __cplusplus
extern "C" {
#endif

/* launch_rope + launch_copy_to_kv_cache of a prompt as ONE launch (the two calls back to back in reference attention.cpp:164-184): q rotated in
 * place, the rotated k and v converted to F16 (RNE) into the caches at start_pos; k and v are only read.  Identical q and cache rows.  head_dim <= 256. */
int ntk_rope_kv_store(float* q, const float* k, const float* v, const int* positions, int seq_len, int n_heads, int n_kv_heads, int head_dim,
                      float theta_base, float freq_scale, int interleaved, void* k_cache, void* v_cache, int start_pos, int max_seq, void* stream);
/* RoPE FREQUENCY TABLE forms of the prompt-side rotations (ntk_rope of ntk.h, ntk_rope_kv_store above, ntk_rope_kv_store_segments and
 * ntk_rope_kv_store_q8 below): the same arguments plus inv_freq, a DEVICE table of head_dim / 2 floats or NULL -- the convention of the decode
 * launches (ntk_attention_decode_fused ...): entry i replaces the in-kernel 1 / pow(theta_base, 2i / head_dim), so a model's frequency factors
 * (Llama 3.1's rope_freqs.weight) are folded in on the host once; the angle of pair i stays (float)pos * inv_freq[i] * freq_scale, left to right in
 * F32.  NULL: the in-kernel frequency -- the entry points without _tab ARE these with NULL, same kernels, same bits.  A workgroup reads its
 * head_dim / 2 entries once, where it otherwise evaluates pow. */
int ntk_rope_tab(float* q, float* k, const int* positions, int batch_size, int seq_len, int n_heads, int n_kv_heads, int head_dim, float theta_base,
                 float freq_scale, int interleaved, const float* inv_freq, void* stream);
int ntk_rope_kv_store_tab(float* q, const float* k, const float* v, const int* positions, int seq_len, int n_heads, int n_kv_heads, int head_dim,
                          float theta_base, float freq_scale, int interleaved, void* k_cache, void* v_cache, int start_pos, int max_seq,
                          const float* inv_freq, void* stream);
/* ---------------------------------------------------------------------------------------------
 * Engine-level fused operators (no reference counterpart; they compute exactly what the listed
 * sequence of reference launchers computes, in fewer launches, with device-resident positions so a
 * whole token can be replayed from a hipGraph).  Used by nt_engine_*; exported for tests/benchmarks.
 * ------------------------------------------------------------------------------------------- */
typedef struct ntk_gemv_seg {
    const void* W;      /* raw GGUF blocks [rows][in]              */
    float*      y;      /* output [rows]                            */
    int         rows;
    int         dtype;  /* one format per call, or two for the plain (no resid / SiLU) form: Q4_K with Q6_K or Q5_K;
                           NTK_DT_F16 / NTK_DT_BF16 (unquantised rows of 16-bit words): one of them per call */
} ntk_gemv_seg;

/* y_s = W_s . f(x) for up to 3 row segments sharing x (fused Q|K|V or gate|up):
 *   norm_w != NULL : f(x) = rmsnorm(x, norm_w, eps)           (launch_rmsnorm + launch_gemv ...)
 *   resid  != NULL : y_0[r] = resid[r] + (W_0 . f(x))[r]      (launch_gemv + launch_add_inplace); resid may == y_0
 *   silu_pair != 0 : nseg == 2, y_0[r] = silu(W_0.f(x))[r] * (W_1.f(x))[r]   (2 x launch_gemv + launch_silu_mul)
 * F16 / BF16 segments (csrc/gemv_dense16.hip): every form above; in_features a multiple of 8 (<= 32768) and W, x, norm_w 16-byte aligned, NTK_E_ALIGN
 * otherwise -- nothing is launched, y is untouched, the caller runs ntk_rmsnorm / ntk_gemv / ntk_add; F16 mixed with BF16 is NTK_E_DTYPE. */
int ntk_gemv_fused(const ntk_gemv_seg* segs, int nseg, const float* x, int in_features, const float* norm_w,
                   float eps, const float* resid, int silu_pair, void* stream);

/* Engine-owned load-time repack of a Q8_0 matrix, LANE-MAJOR (csrc/gemv.hip, layout: csrc/gemv_core.hip.h): a byte permutation of every row slice, the GGUF
 * size, read by the row-per-wave decode GEMV with identical bits to ntk_gemv_fused over the GGUF blocks.  Taken when in_features % 256 == 0 and every column
 * slice of the launch is a multiple of 256 columns: otherwise ntk_q8l_bytes == 0 / NTK_E_SHAPE.  The K-quant entry points below (ntk_rp_bytes / _pack /
 * _unpack / ntk_gemv_rp) keep refusing Q8_0; the decode launch is ntk_gemv_rp_fused with ALL segments Q8_0 and segs[i].W pointing at ntk_q8l_pack output
 * (Q8_0 beside a K-quant in one list: NTK_E_DTYPE).  pack: raw 4-byte aligned, dst 16-byte; unpack: the exact inverse.  Stream ordered. */
size_t ntk_q8l_bytes(int rows, int in_features);
int ntk_q8l_pack(void* dst, const void* raw, int rows, int in_features, void* stream);
int ntk_q8l_unpack(void* raw, const void* packed, int rows, int in_features, void* stream);

/* Engine-owned load-time repack of a K-quant matrix and the decode GEMV on the int8 matrix cores that reads it (csrc/gemv_rp.hip; SURVEY
 * 7.1 step 7 / 8(b) "Ownership": repack buffers belong to the engine object, the 1:1 ntk_gemv above keeps taking raw GGUF).  Q4_K, Q5_K,
 * Q6_K; in_features % 256 == 0 and <= 32768; rows padded to tiles of 16 inside the buffer.  Same integers, same scales (ntk_rp_dequant gives
 * the GGUF dequantisation bit for bit), 1.028 x / 1.023 x / 1.000 x the GGUF bytes.  Arithmetic: x -> per 256-column super-block three
 * signed base-256 digit planes of rint(x 2^(22-e)) (e = exponent of the block's largest |x|: <= 2^-22 of it per term), exact integer dot
 * products per sub-block on v_mfma_i32_16x16x64_i8, the reference's factorisation (gemm.cu:190-244, 297-354, 421-459) around them.
 *   ntk_rp_bytes        size of the repacked form (0: unsupported dtype / shape)
 *   ntk_rp_pack         raw GGUF [rows][in] -> dst (16-byte aligned, ntk_rp_bytes); stream ordered
 *   ntk_rp_dequant      parity instrumentation: the weights as F32 [rows][in] from the repacked form
 *   ntk_rp_unpack       the raw GGUF bytes back (exact inverse of ntk_rp_pack)
 *   ntk_gemv_rp(_fused) = ntk_gemv / ntk_gemv_fused with segs[i].W pointing at REPACKED tensors (same epilogues; one or two formats) */
size_t ntk_rp_bytes(int dtype, int rows, int in_features);
int ntk_rp_pack(void* dst, const void* raw, int rows, int in_features, int dtype, void* stream);
int ntk_rp_dequant(float* out, const void* rp, int rows, int in_features, int dtype, void* stream);
/* the raw GGUF blocks [rows][in] back from the repacked form, byte for byte (the engine keeps ONE resident copy of a K-quant matrix and unpacks into
 * a scratch in front of the launches that read raw blocks); raw: 4-byte aligned (Q6_K: 2); stream ordered */
int ntk_rp_unpack(void* raw, const void* rp, int rows, int in_features, int dtype, void* stream);
int ntk_gemv_rp(float* y, const void* rp, const float* x, int out_features, int in_features, int weight_dtype, void* stream);
int ntk_gemv_rp_fused(const ntk_gemv_seg* segs, int nseg, const float* x, int in_features, const float* norm_w, float eps,
                      const float* resid, int silu_pair, void* stream);
/* The static decode activations (csrc/gemv.hip): fixed slots of one module-scope device buffer for the single-token vectors the decode GEMVs
 * read as x.  Their addresses are link-time constants of the kernels, so a lane-major Q8_0 launch (ntk_gemv_rp_fused, all segments Q8_0) whose
 * x IS a slot -- and whose in_features is the slot's form: hidden x 4096 with a fused RMSNorm, attention output x 4096, SiLU x up x 14336 -- requests x before
 * its kernel arguments have arrived (same loads, same values, same bits; any other x / width: the ordinary kernel).  One owner per process and
 * device: an engine's fused single-token path; everything else keeps buffers of its own.
 *   ntk_decode_arena_acquire   >= 0: the caller owns the current device's arena until _release -- the value is that device's index, the token
 *                              _release takes; -1: somebody else owns it (or no device)
 *   ntk_decode_arena_release   by the owner, with the index _acquire returned (whichever device is current by then)
 *   ntk_decode_arena_slot      the slot's device address on the current device (NULL: no such slot / no device); owning is not needed to ask
 *   ntk_debug_gemv_static_x    parity instrumentation: the slot whose early-x form this thread's last lane-major Q8_0 launch took (0: the ordinary kernel) */
#define NTK_ARENA_HIDDEN 1
#define NTK_ARENA_ATTN_OUT 2
#define NTK_ARENA_GATE 3
#define NTK_ARENA_HIDDEN_FLOATS 8192
#define NTK_ARENA_ATTN_FLOATS 8192
#define NTK_ARENA_GATE_FLOATS 32768
int ntk_decode_arena_acquire(void);
void ntk_decode_arena_release(int device);
float* ntk_decode_arena_slot(int slot);
int ntk_debug_gemv_static_x(void);

/* parity instrumentation of the above: the LDS image its prologue builds from x (4 in + 68 in/256 bytes: three digit planes, a zero plane,
 * 64 bytes of sub-block-sum digits and one 2^(e-22) per super-block; nsub = 8: 32-column sub-blocks (Q4_K / Q5_K), 16: Q6_K), and
 * D[16][16] = A[16][64] . B[64][16] on the matrix instruction under the lane maps the kernel assumes */
int ntk_debug_rp_prologue(uint8_t* out, const float* x, const float* norm_w, float eps, int in_features, int nsub, int nwaves, void* stream);
int ntk_debug_mfma_i8_probe(int* D, const int8_t* A, const int8_t* B, void* stream);

/* RoPE(q,k at *d_pos) + KV store + GQA decode attention over keys 0..*d_pos, one launch
 * (launch_rope + launch_copy_to_kv_cache + launch_attention_decode; attention.cpp:165-190).
 * q [nh*hd], k,v [nkv*hd] are the raw projections (left untouched); d_pos is a DEVICE int.
 * inv_freq: optional DEVICE table [hd/2] of 1/powf(theta, 2i/hd) (NULL = computed in the kernel). */
int ntk_attention_decode_fused(float* output, const float* q, const float* k, const float* v, void* k_cache,
                               void* v_cache, const int* d_pos, const float* inv_freq, int n_heads, int n_kv_heads,
                               int head_dim, int max_seq, float scale, float theta_base, float freq_scale,
                               void* stream);

/* Long-context form of ntk_attention_decode_fused: `nsplit` workgroups share a head (positions interleaved), partial
 * softmax states go through `scratch` (ntk_attention_split_scratch_bytes) and a second launch merges them.  Same
 * arguments and results (summation order aside); head_dim 64 / 128 / 256, 16-byte aligned caches.
 * head_dim 128 with nsplit >= 16 and at most 16 query heads per KV head: one workgroup per (KV head, split) on the F16
 * matrix cores, every cache row read once (q * scale and the softmax weights enter as two F16 pieces each: <= 2^-22 of
 * the operand); rows past *d_pos are loaded but take no part whatever they hold. */
size_t ntk_attention_split_scratch_bytes(int n_heads, int head_dim, int nsplit);
int ntk_attention_decode_split(float* output, const float* q, const float* k, const float* v, void* k_cache,
                               void* v_cache, const int* d_pos, const float* inv_freq, int n_heads, int n_kv_heads,
                               int head_dim, int max_seq, float scale, float theta_base, float freq_scale, int nsplit,
                               float* scratch, void* stream);
/* The same as ONE launch: the workgroup that finishes last among the nsplit (<= 64) of a head merges their states itself -- the same
 * operations in the same order as the merge launch, identical bits.  The first ntk_attention_split_scratch_bytes' n_heads u32 of
 * `scratch` are arrival counters: zero them ONCE after allocating (ntk_attention_split_scratch_init, stream ordered); every launch
 * leaves them zero.  One scratch serves one stream at a time. */
int ntk_attention_split_scratch_init(float* scratch, int n_heads, void* stream);
int ntk_attention_decode_split_merged(float* output, const float* q, const float* k, const float* v, void* k_cache,
                                      void* v_cache, const int* d_pos, const float* inv_freq, int n_heads, int n_kv_heads,
                                      int head_dim, int max_seq, float scale, float theta_base, float freq_scale, int nsplit,
                                      float* scratch, void* stream);

/* Decode attention for a BATCH of sequences (csrc/attention_batch.hip; no reference counterpart): for each of n_rows rows, 1 <= n_rows <=
 * NTK_ATTN_BATCH_MAX, what ntk_attention_decode_fused (nsplit == 1) / ntk_attention_decode_split (nsplit > 1: + ONE combine launch for all rows) do for
 * one row, in one launch -- the same device functions, the same bits as the single-row launch of the same form, and a row's result depends on nothing
 * but that row (permuting the rows permutes the outputs).  q [n_rows][n_heads * head_dim], k, v [n_rows][n_kv_heads * head_dim] F32, unrotated, only
 * read; positions DEVICE int [n_rows]; caches: HOST struct with the rows' K and V cache base pointers for this layer ([max_seq][n_kv_heads][head_dim]
 * half each; entries past n_rows are ignored), copied BY VALUE into the launch -- no device table.  Row b: RoPE of q and k at positions[b] (inv_freq as
 * in the single-row kernels), k and v stored as F16 (RNE) into row positions[b] of cache b -- the ONLY cache rows written -- and attention over rows
 * 0 .. positions[b] of cache b into output[b]; rows past positions[b] may hold anything.  A split that lies wholly past a row's position contributes
 * nothing.  nsplit >= 16 at head_dim 128 with <= 16 query heads per KV head: the matrix-core form.  scratch (nsplit > 1): n_rows x
 * ntk_attention_split_scratch_bytes(n_heads, head_dim, nsplit).  Two rows must not name the same cache (unchecked; every position must lie in
 * [0, max_seq): the caller validates).  NTK_E_SHAPE: n_rows outside 1 .. 16, head sizes / split counts the single-row kernels refuse; NTK_E_NULL. */
#define NTK_ATTN_BATCH_MAX 16
typedef struct ntk_kv_batch {
    void* k[NTK_ATTN_BATCH_MAX];
    void* v[NTK_ATTN_BATCH_MAX];
} ntk_kv_batch;
int ntk_attention_decode_batch(float* output, const float* q, const float* k, const float* v, const ntk_kv_batch* caches, const int* positions,
                               int n_rows, const float* inv_freq, int n_heads, int n_kv_heads, int head_dim, int max_seq, float scale,
                               float theta_base, float freq_scale, int nsplit, float* scratch, void* stream);

/* The PACKED PROMPT PASS (csrc/attention.hip, csrc/attention_mfma.hip; no reference counterpart): the rows of one pass are the concatenation of SEGMENTS,
 * a segment being n_rows consecutive tokens of one sequence whose first row sits at cache position start_pos of that sequence's own F16 caches (a
 * segment of one row at start_pos > 0 is a decode row, a longer one at start_pos > 0 a prompt chunk).  The descriptor is a HOST struct, copied BY VALUE
 * into the launches as ntk_kv_batch is -- no device table; entries past n_seg are ignored.
 *   ntk_kv_segments_validate       host only: NTK_E_SHAPE unless 1 <= n_seg <= NTK_ATTN_BATCH_MAX, row0[0] == 0, row0[s + 1] == row0[s] + n_rows[s], every
 *                                  n_rows >= 1, the rows sum to total_rows, start_pos >= 0, start_pos + n_rows <= max_seq and no two segments name the same
 *                                  k cache; NTK_E_NULL for a NULL descriptor or a NULL cache among the first n_seg.  Both launchers call it first.
 *   ntk_rope_kv_store_segments     ntk_rope_kv_store for every segment in ONE launch, one workgroup per row: row r of segment s is rotated at position
 *                                  start_pos[s] + (r - row0[s]) -- q in place; k and v are only read -- and its rotated k and its v go as F16 (RNE) into row
 *                                  `position` of caches s: the device function of ntk_rope_kv_store's kernel, so a segment's q and cache rows are that
 *                                  launch's bits on the segment alone.  No other cache byte is written.  q [total_rows][n_heads * head_dim], k, v
 *                                  [total_rows][n_kv_heads * head_dim] F32.  head_dim <= 256 and even (NTK_E_SHAPE).
 *   ntk_attention_prefill_segments ntk_attention_prefill for every segment: row t of segment s attends over rows 0 .. start_pos[s] + t of caches s and nothing
 *                                  else.  A segment's output has the bits of ntk_attention_prefill on that segment alone, because every segment runs the
 *                                  code that call would run: at head_dim 128 with 16-byte aligned operands all segments of two rows or more share ONE launch
 *                                  of the matrix-core kernel's body (a workgroup finds its segment and query tile with a uniform scan of the <= 16 per-segment
 *                                  tile counts in its arguments) and all single-row segments ONE launch of the single-query kernel's body, which is what
 *                                  ntk_attention_prefill runs for a one-row prompt (head_dim 64 / 128 / 256, aligned caches); longer segments at other
 *                                  head sizes, and unaligned operands, take ntk_attention_prefill's own launch, once per segment.  Q, output [total_rows][n_heads * head_dim] F32; cache rows past a segment's last key may
 *                                  hold anything.  F16 caches only. */
typedef struct ntk_kv_segments {
    int   n_seg;                          /* 1 .. NTK_ATTN_BATCH_MAX */
    int   row0[NTK_ATTN_BATCH_MAX];       /* first row of the segment in q / k / v / output; ascending, contiguous from 0 */
    int   n_rows[NTK_ATTN_BATCH_MAX];     /* >= 1 */
    int   start_pos[NTK_ATTN_BATCH_MAX];  /* cache position of the segment's first row */
    void* k[NTK_ATTN_BATCH_MAX];          /* this layer's F16 cache of the segment's slot, [max_seq][n_kv_heads][head_dim] */
    void* v[NTK_ATTN_BATCH_MAX];
} ntk_kv_segments;
int ntk_kv_segments_validate(const ntk_kv_segments* segs, int total_rows, int max_seq);
int ntk_rope_kv_store_segments(float* q, const float* k, const float* v, const ntk_kv_segments* segs, int n_heads, int n_kv_heads, int head_dim,
                               float theta_base, float freq_scale, int interleaved, int max_seq, void* stream);
int ntk_rope_kv_store_segments_tab(float* q, const float* k, const float* v, const ntk_kv_segments* segs, int n_heads, int n_kv_heads, int head_dim,
                                   float theta_base, float freq_scale, int interleaved, int max_seq, const float* inv_freq, void* stream);   /* (the table forms: above) */
int ntk_attention_prefill_segments(float* output, const float* Q, const ntk_kv_segments* segs, int n_heads, int n_kv_heads, int head_dim, int max_seq,
                                   float scale, void* stream);

/* ---------------------------------------------------------------------------------------------
 * The 8-bit (Q8_0) KV cache (csrc/attention_q8.hip; no reference counterpart).  A cache row holds Q8_0 values along head_dim: every 32
 * consecutive elements of a head's row share one IEEE-half scale d and carry 32 int8 q -- ggml's quantize_row_q8_0_ref arithmetic in F32
 * on the F32 post-RoPE k and the F32 v (amax, d = amax / 127, id = d ? 1 / d : 0, q = roundf(x * id), d stored RNE; where that arithmetic
 * is undefined -- a subnormal amax makes id infinite -- x * id = NaN counts as 0 and the product is clamped to +-127).
 * Device layout: ONE buffer per layer and side (K or V) of ntk_kv_q8_cache_bytes bytes, 16-byte aligned: int8 quants [max_seq][n_kv_heads *
 * head_dim], then (at byte max_seq * n_kv_heads * head_dim) half scales [max_seq][n_kv_heads * head_dim / 32] -- 1.0625 bytes per element.
 * head_dim % 32 == 0.  The decode kernel uses half(d) * q EXACTLY (int8 -> F16 is exact; scales are applied to F32 block sums / folded into
 * the F32 softmax weights as an exact mantissa part, the exact power of two going onto the quants): nothing rounds d * q to half.
 *   ntk_kv_store_q8          F32 rows k, v [seq_len][n_kv_heads * head_dim] (k already rotated) -> cache rows [start_pos, start_pos + seq_len)
 *   ntk_rope_kv_store_q8     ntk_rope_kv_store with the 8-bit store: q and the cache bit-identical to ntk_rope + ntk_kv_store_q8 (seq_len >= 4)
 *   ntk_attention_decode_q8  ntk_attention_decode_split over the 8-bit caches: RoPE of q and the new k, quantise + store the new row, GQA
 *                            attention over rows 0 .. *d_pos (the new row included) on the F16 matrix cores, one workgroup per (KV head,
 *                            split), partial states in `scratch` (ntk_attention_split_scratch_bytes) + the combine launch.  Any position
 *                            from 0, any nsplit in 1 .. 1024; rows past *d_pos may hold any bytes.  head_dim 128 and <= 16 query heads per
 *                            KV head (NTK_E_SHAPE otherwise).
 *   ntk_kv_dequant_q8_f16    cache rows [0, n_rows) -> F16 K and V images [n_rows][n_kv_heads * head_dim] (the layout ntk_attention_prefill /
 *                            ntk_attention_decode read): half_rne(half(d) * q)
 *   ntk_attention_decode_q8_batch  ntk_attention_decode_q8 for n_rows sequences (1 .. NTK_ATTN_BATCH_MAX) in ONE launch + ONE combine launch for all
 *                            rows: the same device function (csrc/attention_q8_decode.hip.h), so row b has the bits of the single-row launch with
 *                            the same nsplit, and depends on nothing but row b.  q [n_rows][n_heads * head_dim], k, v [n_rows][n_kv_heads *
 *                            head_dim] F32, unrotated, only read; positions DEVICE int [n_rows], each in [0, max_seq) (the caller validates);
 *                            caches: HOST struct with the rows' 8-bit K and V buffers of this layer (ntk_kv_q8_cache_bytes each), copied BY VALUE
 *                            into the launch; entries past n_rows are ignored.  The only cache bytes written are row positions[b] of caches b.
 *                            Two rows must not name the same cache (unchecked).  A split that lies wholly past a row's position contributes
 *                            nothing.  scratch: n_rows x ntk_attention_split_scratch_bytes(n_heads, head_dim, nsplit).  Refusals: those of
 *                            ntk_attention_decode_q8, NTK_E_SHAPE for n_rows outside 1 .. 16, NTK_E_NULL for a NULL cache among the first n_rows.
 * ------------------------------------------------------------------------------------------- */
size_t ntk_kv_q8_cache_bytes(int max_seq, int n_kv_heads, int head_dim);
int ntk_kv_store_q8(void* k_cache, void* v_cache, const float* k, const float* v, int seq_len, int n_kv_heads, int head_dim, int start_pos,
                    int max_seq, void* stream);
int ntk_rope_kv_store_q8(float* q, const float* k, const float* v, const int* positions, int seq_len, int n_heads, int n_kv_heads, int head_dim,
                         float theta_base, float freq_scale, int interleaved, void* k_cache, void* v_cache, int start_pos, int max_seq,
                         void* stream);
int ntk_rope_kv_store_q8_tab(float* q, const float* k, const float* v, const int* positions, int seq_len, int n_heads, int n_kv_heads, int head_dim,
                             float theta_base, float freq_scale, int interleaved, void* k_cache, void* v_cache, int start_pos, int max_seq,
                             const float* inv_freq, void* stream);   /* (the table forms: above) */
int ntk_attention_decode_q8(float* output, const float* q, const float* k, const float* v, void* k_cache, void* v_cache, const int* d_pos,
                            const float* inv_freq, int n_heads, int n_kv_heads, int head_dim, int max_seq, float scale, float theta_base,
                            float freq_scale, int nsplit, float* scratch, void* stream);
int ntk_kv_dequant_q8_f16(void* k_f16, void* v_f16, const void* k_cache, const void* v_cache, int n_rows, int n_kv_heads, int head_dim,
                          int max_seq, void* stream);
int ntk_attention_decode_q8_batch(float* output, const float* q, const float* k, const float* v, const ntk_kv_batch* caches, const int* positions,
                                  int n_rows, const float* inv_freq, int n_heads, int n_kv_heads, int head_dim, int max_seq, float scale,
                                  float theta_base, float freq_scale, int nsplit, float* scratch, void* stream);

/* ---------------------------------------------------------------------------------------------
 * KV cache sequence operations (csrc/kv_ops.hip; no reference counterpart): the CONTEXT SHIFT.  In every one of n_layers layers, rows
 * [src0, src0 + n_rows) of both caches move to [dst0, dst0 + n_rows), 0 <= dst0 < src0, src0 + n_rows <= max_seq.  V rows move byte for byte (Q8:
 * quants and scales).  K rows -- cached AFTER RoPE -- are rotated by delta = dst0 - src0 positions, which makes them the keys the model would have
 * cached at the new positions.  Every byte of both caches outside the destination rows keeps its value.
 * Layouts: ntk_kv_shift      F16 [n_layers][max_seq][n_kv_heads][head_dim] halves, head_dim 64 / 80 / 128;
 *          ntk_kv_shift_q8   n_layers consecutive layer buffers of ntk_kv_q8_cache_bytes(max_seq, n_kv_heads, head_dim) bytes each (int8 quants
 *                            [max_seq][row], then half scales [max_seq][row / 32]); head_dim 128 only, as the 8-bit store.
 * Rotation: the frequency of pair i is inv_freq[i] (DEVICE table [head_dim / 2]) or, inv_freq == NULL, 1 / (float)pow((double)theta_base,
 * (double)((2.0f * i) / head_dim)); angle = (float)delta * freq * freq_scale in F32, left to right (the forward kernels' pos * freq * fscale);
 * c, s = cosf, sinf; a' = a c - b s, b' = a s + b c in F32, each operation rounded on its own; the pair is (i, i + head_dim / 2), or (2 i, 2 i + 1)
 * when `interleaved`.  F16: the result rounded to nearest even.  Q8: the head dequantised as half(d) * q (exact in F32), rotated as a whole (a pair
 * spans two 32-blocks), every block requantised by the store's rule (ggml quantize_row_q8_0_ref) -- so an 8-bit K row loses up to half a
 * quantisation step per shift, an F16 row half an ulp of half.
 * Overlapping ranges (n_rows > src0 - dst0) are moved correctly for every src0 - dst0 >= 1 in ONE launch: a thread owns the rows of one residue class
 * modulo src0 - dst0 and walks them in ascending order, so every write lands on a row the same thread has already read (csrc/kv_ops.hip).  Stream
 * ordered, no allocation, no scratch.  Refused before any launch -- NTK_E_NULL: a NULL cache; NTK_E_SHAPE: a head size not listed, n_rows < 1,
 * dst0 < 0, dst0 >= src0, src0 + n_rows > max_seq, n_layers outside 1 .. 65535; NTK_E_ALIGN: a cache that is not 16-byte aligned.
 * ------------------------------------------------------------------------------------------- */
int ntk_kv_shift(uint16_t* k_cache, uint16_t* v_cache, int n_layers, int max_seq, int n_kv_heads, int head_dim, int src0, int dst0, int n_rows,
                 const float* inv_freq, float theta_base, float freq_scale, int interleaved, void* stream);
int ntk_kv_shift_q8(void* k_cache_q8, void* v_cache_q8, int n_layers, int max_seq, int n_kv_heads, int head_dim, int src0, int dst0, int n_rows,
                    const float* inv_freq, float theta_base, float freq_scale, int interleaved, void* stream);

/* Parity instrumentation: ntk_gemv_fused with the activation form of its Q4_K / Q6_K launches chosen by the CALL.  Those launches take,
 * from 48 MiB of weights on (a constant of the library: below it the conversion costs what the decode saves), the integer-activation
 * decoders of csrc/gemv_core.hip.h (three int8 digit planes per 32-column sub-block on v_dot4).  integer_activations = 1: whenever the
 * launch is eligible, 0: never, -1: the size rule -- so that the tests reach both decoders at small sizes.  No global state. */
int ntk_debug_gemv_fused_form(const ntk_gemv_seg* segs, int nseg, const float* x, int in_features, const float* norm_w, float eps,
                              const float* resid, int silu_pair, int integer_activations, void* stream);

/* Tensor-parallel exchange (csrc/tp.hip): hidden[0..n) += sum over ranks of their partial vectors, in rank
 * order, by one kernel that reads the peers' communication buffers (mapped with ntk_ipc_open or shared in-process) -- no RCCL
 * call, no second stream, hipGraph-capturable.  A communication buffer = ntk_tp_comm_bytes(max_floats) device bytes, reset once
 * with ntk_tp_comm_reset before the peers map it.  Call k of a forward writes its partial vector to ntk_tp_slot(comm, max_floats,
 * k) (slot k & 1) with any kernel on the same stream, then runs ntk_tp_allreduce_add(..., k, n, stream); calls per forward must be
 * even in number and < 1023; ntk_tp_advance_epoch ends the forward.  All ranks must issue the same sequence.  n % 4 == 0,
 * n <= max_floats, world <= 8.  ntk_tp_error after a synchronise: 0, or non-zero if a bounded wait for a peer gave up. */
size_t   ntk_tp_comm_bytes(size_t max_floats);
void*    ntk_tp_comm_alloc(size_t bytes);   /* fine-grained device memory (peer-visible without relying on a cache write-back); nt_hip_free */
int      ntk_tp_comm_reset(void* comm, void* stream);
float*   ntk_tp_slot(void* comm, size_t max_floats, unsigned call_index);
int      ntk_tp_allreduce_add(float* hidden, void* const* peers, int rank, int world, size_t max_floats, unsigned call_index, int n, void* stream);
int      ntk_tp_advance_epoch(void* comm, void* stream);
unsigned ntk_tp_error(void* comm);
int      ntk_ipc_export(void* devptr, void* handle64);
int      ntk_ipc_open(const void* handle64, void** devptr);
int      ntk_ipc_close(void* devptr);

/* Batched prompt projection on the matrix cores (replaces the per-token launch_gemv loops of
 * attention.cpp:144-162,200-210 and ffn.cpp:96-133):  Y[t,:] = W . X[t,:] (+ resid[t,:]) for t < n_tokens.
 * X [n_tokens][in] and Y/resid [n_tokens][out] are F32, token-major; W raw GGUF blocks [out][in] (the quantised dtypes, and
 * NTK_DT_F16 / NTK_DT_BF16 rows of 16-bit words: those with W 16-byte aligned and in_features a multiple of 32, widened exactly);
 * X 16-byte aligned.  W is streamed once per 16 tokens; F32 activations, F32 MFMA accumulate.  resid may == Y. */
int ntk_gemm_quant(float* Y, const void* W, const float* X, int n_tokens, int out_features, int in_features,
                   int weight_dtype, const float* resid, void* stream);

/* The same projection on the FP16 matrix cores, up to 1024 tokens per pass over W (csrc/gemm_f16.hip) -- ONE entry point behind a descriptor
 * (round 6: the six ntk_gemm_quant_ws* names of round 5 were this call with different optional fields).
 * Arithmetic: the integer part of every weight is exact in FP16; every F32 activation x is scaled by a power of two s (one per token: the token's
 * largest |x| s lies in [2^14, 2^15)) and split into two FP16 pieces h1 = rn16(x s), h2 = rn16(x s - h1), so that |x s - h1 - h2| <= 2^-23 |x s|
 * -- one F32 ulp of the activation (and <= 2^-39 of the token's largest |x| for activations more than 2^17 below it: the matrix cores take FP16
 * subnormals as they are, tools/micro/mfma_f16_subnormal.hip); the FP16 x FP16 products are exact in the F32 accumulator, block scales / K-quant
 * minima are applied to the F32 block sums and 1 / s to the finished sum (exact).  Against ntk_gemv the summation order differs and the
 * activations carry that one-ulp rounding.
 * Limits: Q8_0, Q4_0, Q4_K, Q5_K and Q6_K (NTK_E_DTYPE otherwise: use ntk_gemm_quant), one format per call; in_features a multiple of 128 (Q8_0) /
 * 256 (the others), rows % 16 == 0 and rows * row_bytes < 4 GiB (NTK_E_SHAPE); W, X, Y, resid 16-byte aligned (NTK_E_ALIGN).
 * (Row pitches that are not a multiple of 4 bytes -- Q8_0 with in_features % 64 != 0, Q6_K with in_features % 512 != 0 -- run the
 * same kernel with 2-byte aligned LDS reads, several times slower; no projection of the target models has one.)
 *   segs / nseg   1..3 matrices of one format that share X (Q | K | V, gate | up): {W_i raw GGUF [rows_i][in], y = Y_i [n_tokens][rows_i], rows_i, dtype}
 *   resid         optional [n_tokens][rows_0], nseg == 1 only, may alias Y_0: Y = W . X + resid
 *   workspace     ntk_gemm_quant_workspace_bytes(in_features, sum of rows_i) device bytes, 16-byte aligned, shared by every call (the FP16 planes and
 *                 scales of up to sixteen 64-token chunks of X + the partial sums of the K splits); contents need no initialisation
 *   reuse_x       != 0: X (same pointer, n_tokens <= 1024) has not changed since the previous call with this workspace -- its planes are not rebuilt
 *   row_max       optional DEVICE [n_tokens]: the tokens' largest |X[t, :]| (NULL = computed by a pass over X): the operand pre-pass is then ONE
 *                 launch, identical results.  The kernels that usually PRODUCE X in the reference's prompt path leave it beside X: ntk_rmsnorm_rowmax
 *                 (reference src/model/norm.cpp -> launch_rmsnorm, rmsnorm.cu:60-68; same expressions and sums as ntk_rmsnorm, identical output;
 *                 zero_tokens (optional): n_tokens floats set to 0 for a later ntk_silu_mul_rowmax) and ntk_silu_mul_rowmax (reference ffn.cpp:127 ->
 *                 launch_silu_mul, gemm.cu:719-724; identical output; width % 4 == 0, 16-byte aligned pointers, output may alias gate), whose row_max
 *                 must hold zeros (or earlier maxima of the same tokens) on entry
 *   partials      optional: the split-K sums are left to the launch that CONSUMES the projection.  The same launch runs but, when it splits K, the
 *                 partial sums stay in the workspace and *partials describes them (nsplit > 1; valid until the next call with this workspace) -- or
 *                 says nsplit == 1, in which case Y was written as usual (with `resid` added by the launch's epilogue; a launch that does split K
 *                 ignores `resid`: its consumer adds the residual).  Consumers:
 *                   ntk_reduce_rmsnorm_rowmax : hidden[t] = (sum of the splits, in order) + hidden[t]  (= the residual epilogue's association; nsplit == 1:
 *                       nothing to add when the launch ran with Y = resid = hidden, else hidden += Y), x_out = rmsnorm(hidden) with row_max /
 *                       zero_tokens as ntk_rmsnorm_rowmax: Wo / down projection + residual + the next RMSNorm, one launch;
 *                   ntk_reduce_silu_mul_rowmax: output[t] = silu(gate[t]) * up[t] of a deferred two-matrix gate | up launch, row_max as ntk_silu_mul_rowmax.
 *                 Identical bits to the separate launches (same sums in the same order).
 *   weights_repacked  != 0: segs[i].W point at the engine's DECODE REPACK of the matrices (ntk_rp_pack: tiles of 16 rows x 256-column super-blocks) instead
 *                 of raw GGUF blocks -- Q4_K / Q5_K / Q6_K (NTK_E_DTYPE otherwise).  Round 6: with one resident copy of a K-quant matrix the prompt pass
 *                 needs no unpack any more.  The same integers and scale products in the same order: IDENTICAL bits to the raw form.
 *   full_form     != 0: the launch takes the form, K split and chunk pairing of a FULL pass (1024 tokens) whatever n_tokens is, never the short-prompt
 *                 forms: a token's outputs are then the same bits however the caller cuts its tokens into calls (Model::score: the LM head over
 *                 "score_rows" rows at a time).  0 (every other caller): the form is chosen for n_tokens, as before.
 * Stream ordered, no allocation, no synchronisation. */
typedef struct ntk_gemm_partials {
    const float* part[3];   /* per matrix: [nsplit][n_tokens][rows] partial sums (NULL when nsplit == 1) */
    float*       y[3];      /* per matrix: the Y passed to the launch (written when nsplit == 1)            */
    int          rows[3];
    int          nseg, n_tokens, nsplit;
} ntk_gemm_partials;
typedef struct ntk_gemm_desc {
    const ntk_gemv_seg* segs;
    int                 nseg;
    const float*        X;            /* [n_tokens][in_features] */
    int                 n_tokens, in_features;
    const float*        resid;
    void*               workspace;
    size_t              workspace_bytes;
    int                 reuse_x;
    const float*        row_max;
    ntk_gemm_partials*  partials;
    int                 weights_repacked;   /* != 0: segs[i].W are tensors of the decode repack (ntk_rp_pack; Q4_K / Q5_K / Q6_K), read as they lie */
    int                 full_form;          /* != 0: the form of a full 1024-token pass whatever n_tokens is (chunking-independent bits) */
} ntk_gemm_desc;
size_t ntk_gemm_quant_workspace_bytes(int in_features, int out_features);
int ntk_gemm_quant_f16(const ntk_gemm_desc* desc, void* stream);
int ntk_reduce_rmsnorm_rowmax(float* hidden, const ntk_gemm_partials* partials, const float* weight, float eps, float* x_out, float* row_max,
                              float* zero_tokens, void* stream);
int ntk_reduce_silu_mul_rowmax(float* output, const ntk_gemm_partials* partials, float* row_max, void* stream);
int ntk_rmsnorm_rowmax(float* output, const float* input, const float* weight, int n_tokens, int hidden_size, float eps, float* row_max,
                       float* zero_tokens, void* stream);
int ntk_silu_mul_rowmax(float* output, const float* gate, const float* up, int n_tokens, int width, float* row_max, void* stream);
/* The operand pre-pass INSIDE the launch that produces X (round 6): each of these owns a whole token per workgroup, so the workgroup that has written a
 * token's row also splits it -- planes, step sums and 1 / s go straight into `workspace` (the bits ntk_gemm_quant_f16's own pre-pass would write) and the
 * projection that follows runs with reuse_x = 1 on that workspace: no separate pre-pass launch (four to five of the fourteen launches of a prompt layer).
 *   ntk_gemm_prepare_x            X as it lies (e.g. the attention output in front of Wo): row maximum + split, one launch instead of two
 *   ntk_rmsnorm_prepare_x         ntk_rmsnorm (reference rmsnorm.cu:60-68; identical output) + the split of its output
 *   ntk_reduce_rmsnorm_prepare_x  ntk_reduce_rmsnorm_rowmax (identical hidden / x_out) + the split of x_out
 *   ntk_silu_mul_prepare_x        ntk_silu_mul (reference gemm.cu:719-724; identical output, may alias gate) + the split of its output
 *   ntk_reduce_silu_mul_prepare_x ntk_reduce_silu_mul_rowmax (identical output) + the split; `workspace` must NOT be the one the partial sums lie in
 *                                 (the launch reads those while it writes the planes: the engine alternates between two workspaces)
 * n_tokens <= 1024 (one pass), the row length a multiple of 32 (NTK_E_SHAPE), 16-byte aligned pointers (NTK_E_ALIGN).  Stream ordered, no allocation. */
int ntk_gemm_prepare_x(const float* X, int n_tokens, int in_features, void* workspace, void* stream);
int ntk_rmsnorm_prepare_x(float* output, const float* input, const float* weight, int n_tokens, int hidden_size, float eps, void* workspace, void* stream);
int ntk_reduce_rmsnorm_prepare_x(float* hidden, const ntk_gemm_partials* partials, const float* weight, float eps, float* x_out, void* workspace, void* stream);
int ntk_silu_mul_prepare_x(float* output, const float* gate, const float* up, int n_tokens, int width, void* workspace, void* stream);
int ntk_reduce_silu_mul_prepare_x(float* output, const ntk_gemm_partials* partials, void* workspace, void* stream);

/* The same projection over UNQUANTISED 16-bit rows on the 16-bit matrix cores (csrc/gemm_dense16.hip; plan: csrc/gemm_dense16_plan.h): the descriptor of
 * ntk_gemm_quant_f16 with segs[i].dtype NTK_DT_F16 or NTK_DT_BF16 -- one of them per call -- and segs[i].W the matrix as it lies in the file, [rows_i][in]
 * 16-bit words.  The weights reach the matrix instructions without a conversion; products are exact, sums F32.
 *   F16   v_mfma_f32_16x16x32_f16 over the FP16 GEMM's own operand planes (two FP16 pieces of x s, 1 / s on the finished sum: the bound above).  The
 *         workspace has the layout ntk_gemm_prepare_x and the other ntk_*_prepare_x producers write: with reuse_x != 0 their planes are read as they lie.
 *   BF16  v_mfma_f32_16x16x32_bf16 over THREE bfloat16 pieces of x and no token scale: p1 = rn(x), p2 = rn(x - p1), p3 = rn(x - p1 - p2), rn to nearest
 *         even and never from a finite x to infinity; p1 + p2 + p3 == x for every x whose last bit is >= 2^-133, |x - sum| <= 2^-134 below.  Its planes are
 *         a layout of their own in the same workspace (a workspace holds ONE kind of planes at a time); reuse_x != 0 reads those of the previous BF16 call.
 * A token's outputs do not depend on the other tokens, on n_tokens or on the segments sharing the launch: full_form has nothing to select and is ignored,
 * as is row_max (the F16 pre-pass is one launch either way).  K is never split: partials, if given, reports nsplit = 1 and Y is written with the residual.
 * Limits: rows_i % 16 == 0, in_features % 32 == 0, 1..3 segments, weights_repacked == 0 (NTK_E_SHAPE); dtypes other than F16 / BF16 or two kinds in one
 * call (NTK_E_DTYPE); W_i, Y_i, X, resid, workspace 16-byte aligned (NTK_E_ALIGN) -- a refused call launches nothing and leaves Y as it was.  Rows of Y
 * behind n_tokens are never written.  resid: one segment only, may alias Y.  More than 1024 tokens run as passes of 1024 (reuse_x is then ignored).
 * workspace: ntk_gemm_dense16_workspace_bytes(in_features, rows, dtype) bytes (0: not a 16-bit dtype); for F16 never more than
 * ntk_gemm_quant_workspace_bytes of the same shape.  Stream ordered, no allocation, the same bits on every launch. */
size_t ntk_gemm_dense16_workspace_bytes(int in_features, int out_features, int dtype);
int ntk_gemm_dense16(const ntk_gemm_desc* desc, void* stream);

/* Dequantise rows of a (quantised) embedding table on the device: out[t,:] = table[tokens[t],:].
 * Same arithmetic as the host loop in reference src/model/transformer.cpp:419-599; Q5_K is zero-filled
 * exactly as the reference does (:595-598).  tokens is a DEVICE int array. */
int ntk_embed_rows(float* out, const void* table, const int* tokens, int n_tokens, int hidden, int dtype,
                   void* stream);

/* Greedy sampling on the device: first index of the maximum (reference src/inference/sampler.cpp:18-28).
 * Writes the index to *d_out_token (device) -- and to *h_mirror if it is a pinned host pointer (may be NULL).
 * scratch: device buffer of >= 2*1024 floats. */
int ntk_argmax(const float* logits, int n, int* d_out_token, int* h_mirror, float* scratch, void* stream);

/* Scoring (csrc/logprob.hip; no reference counterpart): per row of logits the log-probability of one target token and, optionally, the greedy token.
 * logits [n_rows][ld] F32 (ld >= vocab, row pitch in floats; any 4-byte aligned address), targets DEVICE int [n_rows].
 * logprob[r] = logits[r][targets[r]] - log(sum_j exp(logits[r][j]))   (natural log; targets[r] < 0: logprob[r] = 0, and the row is not read unless top1 is asked for)
 * top1[r] (optional, may be NULL) = first index of the row's maximum (strict >, as ntk_argmax: NaN never wins, a row without a finite or +inf entry gives 0)
 * One pass over the row (online softmax), accurate expf / logf, a fixed reduction order: the same bits on every launch.  -inf logits add 0 to the sum; a row of
 * -inf only, or one that holds a NaN, gives NaN for that row alone.  The caller validates targets[r] < vocab (the kernel clamps: it never leaves the row). */
int ntk_logprob_rows(const float* logits, int n_rows, int vocab, int ld, const int* targets, float* logprob, int* top1, void* stream);

/* The reference's sampler on the device (reference src/inference/sampler.cpp:30-117), for temperature > 0 and
 * 0 < top_k <= 64 (NTK_E_SHAPE otherwise: the caller samples on the host): repeat penalty over d_recent[n_recent] (DEVICE
 * ints, applied in place to `logits`, once per occurrence), logits / temperature, top-k, softmax, top-p cut, and the walk of the
 * cumulative distribution against `r` -- the uniform draw the caller takes from ITS std::mt19937, one per token, so the token
 * stream equals the host sampler's for the same seed.  Result to *d_out_token and *h_mirror (pinned, may be NULL).
 * scratch: ntk_sample_scratch_bytes(n) device bytes.  Vocabularies up to 131 072. */
size_t ntk_sample_scratch_bytes(int n);
int ntk_sample_top_k(float* logits, int n, const int* d_recent, int n_recent, float repeat_penalty, float temperature,
                     int top_k, float top_p, float r, int* d_out_token, int* h_mirror, void* scratch, void* stream);
/* the repeat penalty alone (greedy decoding with a penalty = this + ntk_argmax) */
int ntk_repeat_penalty(float* logits, int n, const int* d_recent, int n_recent, float repeat_penalty, void* stream);

/* The sampler over the rows of a batched decode step, every row with its own settings (csrc/sampling_batch.hip): at most three launches whatever n_rows
 * is -- the penalty (one thread per row), stage 1 over a (chunk, row) grid, stage 2 with one workgroup per row.
 * logits [n_rows][ld] F32, ld >= vocab: only [b][0 .. vocab) is read or written.  d_recent: DEVICE int [n_rows][recent_ld], row b uses its first
 * n_recent[b] entries (may be NULL when no row has a penalty to apply).  d_out: device int [n_rows]; h_mirror: pinned int [n_rows], may be NULL.
 * `rows` is a HOST struct, copied by value into the launches (as ntk_kv_batch is): the caller may reuse it as soon as the call returns.
 * Row b with temperature[b] > 0: exactly ntk_sample_top_k on logits + b * ld with row b's settings and draw r[b] -- the same device code, the same bits.
 * Row b with temperature[b] <= 0: the penalty (if repeat_penalty[b] > 1 and n_recent[b] > 0), then the FIRST maximum of the row (Sampler::argmax:
 * it starts at id 0 and moves on a strict >, so -0 and +0 tie, a NaN above id 0 never wins and a NaN AT id 0 gives 0); no division, r[b] / top_k[b] /
 * top_p[b] ignored.
 * A row's penalty touches that row only; rows are independent: the same bits whatever the companions and the row order.
 * scratch: ntk_sample_rows_scratch_bytes(n_rows, vocab) device bytes.
 * Refused before any launch -- NTK_E_NULL: logits / rows / d_out / scratch, or d_recent where a penalty needs it; NTK_E_SHAPE: n_rows outside 1 .. 16,
 * ld < vocab, vocab beyond 131 072, a sampled row's top_k outside 1 .. 64, an n_recent[b] negative or beyond recent_ld. */
#define NTK_SAMPLE_ROWS_MAX 16
typedef struct ntk_sample_rows {
    float temperature[NTK_SAMPLE_ROWS_MAX], top_p[NTK_SAMPLE_ROWS_MAX], repeat_penalty[NTK_SAMPLE_ROWS_MAX], r[NTK_SAMPLE_ROWS_MAX];
    int   top_k[NTK_SAMPLE_ROWS_MAX], n_recent[NTK_SAMPLE_ROWS_MAX];
} ntk_sample_rows;
size_t ntk_sample_rows_scratch_bytes(int n_rows, int vocab);
int ntk_sample_rows_top_k(float* logits, int n_rows, int vocab, int ld, const int* d_recent, int recent_ld, const ntk_sample_rows* rows, int* d_out,
                          int* h_mirror, void* scratch, void* stream);

/* The greedy tail of a decode token in two launches instead of three: ntk_argmax, then -- in the same final launch -- the token id to the
 * pinned host ring h_ring4 (4 x 8 bytes, may be NULL): slot (*d_pos & 3) receives ONE 8-byte store {token, *d_pos + 1 in the high
 * word}, and *d_pos += 1.  The ring lets a host loop keep the NEXT token's launches queued while it polls for this one (a token that
 * runs one ahead lands in another slot), instead of synchronising the stream per token. */
int ntk_argmax_advance(const float* logits, int n, int* d_out_token, int* h_mirror, unsigned long long* h_ring4, int* d_pos,
                       float* scratch, void* stream);

/* measurement instrumentation: the shader clock right now.  d_out2 (DEVICE, 3 x 8 bytes): [0] shader cycles (s_memtime) and [1] 10 ns ticks
 * (s_memrealtime) over ~50 us of one spinning wave: MHz = 100 * [0] / [1].  bench.py records it right behind the timed region. */
int ntk_debug_sclk(unsigned long long* d_out2, void* stream);
/* ... and the AVERAGE shader clock over a span of work: _begin starts a one-wave kernel on `side_stream` (a stream other than the workload's,
 * e.g. ntk_stream(1)) that sleeps and polls until _end raises d_flag (4 DEVICE bytes) through `other_stream` (e.g. ntk_stream(2)), or 3 s
 * pass; after synchronising side_stream, d_out2 = {shader cycles, 10 ns ticks} of the span.  bench.py runs it over extra decode steps right
 * behind the timed region (never inside it). */
int ntk_debug_sclk_begin(unsigned* d_flag, unsigned long long* d_out2, void* side_stream);
int ntk_debug_sclk_end(unsigned* d_flag, void* other_stream);

/* test instrumentation: after this call nt_hip_malloc hands out at most `bytes` more device bytes and then fails like an exhausted device
 * (NULL + the reference's message); bytes < 0 removes the budget.  Process-wide; tests only (the load-time repack's "does not fit" path). */
void ntk_debug_malloc_budget(long long bytes);

/* *d_pos += 1 (one thread); keeps positions on the device across graph replays */
int ntk_advance_pos(int* d_pos, void* stream);

/* The Q | K | V projection bias of Qwen2-family models (csrc/qkv_bias.hip), in place and in ONE launch for the three buffers and all rows:
 * q[r][c] += bq[c] (q: [n_rows][q_dim], contiguous), k[r][c] += bk[c], v[r][c] += bv[c] (k, v: [n_rows][kv_dim]).  Every element is one F32 add.
 * A bias pointer may be NULL: that buffer is left untouched (and need not exist); all three NULL: NTK_OK, nothing launched.  A buffer is walked in
 * 16-byte pieces when its base and bias are 16-byte aligned and its dimension is a multiple of 4, element by element otherwise: no alignment is
 * assumed.  NTK_E_NULL: a bias without its buffer; NTK_E_SHAPE: n_rows < 0 or a dimension <= 0, or a row of more than 65535 x 256 work items over
 * the three buffers (a work item is one 16-byte piece or one element: 16.7 M elements per row at the least); n_rows == 0: NTK_OK, nothing launched. */
int ntk_qkv_bias(float* q, float* k, float* v, const float* bq, const float* bk, const float* bv, int n_rows, int q_dim, int kv_dim, void* stream);

/* The per-head RMSNorm of Q and K of Qwen3-family models (csrc/qk_norm.hip), in place and in ONE launch for both buffers and all rows: every head of
 * q [n_rows][n_heads * head_dim] becomes x * (1 / sqrtf(sum(x^2) / head_dim + eps)) * wq[head_dim], every head of k [n_rows][n_kv_heads * head_dim] the
 * same with wk; one weight vector serves all heads of its buffer.  One wave per (row, head), the head in registers: a float2 per lane at head_dim 128
 * (buffer and weight 8-byte aligned), a float4 at 256 (16-byte aligned), lane-strided elements for every other even head_dim or base.  The order of the
 * sum depends on head_dim and alignment alone: a row of a T-row launch has the bits of its one-row launch.  NTK_E_NULL: any NULL pointer; NTK_E_SHAPE:
 * head_dim <= 0 or odd, n_heads <= 0, n_kv_heads <= 0, n_rows < 0 (the buffers untouched); n_rows == 0: NTK_OK, nothing launched. */
int ntk_qk_norm(float* q, float* k, const float* wq, const float* wk, int n_rows, int n_heads, int n_kv_heads, int head_dim, float eps, void* stream);

/* ---- The routed expert FFN of mixture-of-experts models (csrc/moe.hip; Qwen3-MoE, Mixtral) ---------------------------------------------------------
 * T rows of a pass (1 .. 1024), E experts (1 .. 256), K experts per row (1 .. min(E, 16)); a PAIR is p = t K + k.  Expert e of a 3-D GGUF tensor is the
 * contiguous block of `rows` rows at e x rows x ntk_row_bytes(dtype, columns); expert matrices are NTK_DT_Q8_0, NTK_DT_Q4_K or NTK_DT_Q6_K, each tensor
 * its own type, rows at any even address (a Q6_K row of 768 columns is 630 bytes).  Everything about the routing -- ids, the work list -- is read from
 * device memory by the launches: no launch parameter depends on it, so the three calls can be captured into a graph.  Nothing here allocates or
 * synchronises.  Every call returns, with the outputs untouched: NTK_E_NULL (a required pointer is NULL), NTK_E_SHAPE (T, E or K outside the limits,
 * K > E, a size <= 0, columns that are not whole blocks of the type, a row too long for the 64 KiB of LDS the four waves share: beyond about 16 000
 * columns), NTK_E_DTYPE (another expert type), NTK_E_ALIGN (float rows not 16-byte aligned, weights at an odd address).
 *
 * ntk_moe_route: logits[t][e] = router[e] . xn[t] (router F32 [E][hidden], F32 accumulation), ids[t][0 .. K) = the K largest in descending order (equal
 * logits: the lower expert first), w[t][k] = exp(l_k - l_0) / sum_j exp(l_j - l_0) over those K (llama.cpp's softmax -> top-K -> renormalise), and the
 * expert-major work list: offsets[E + 1], pairs[T K] = the pair indices sorted by (expert, pair index), i.e. numpy's stable argsort of ids.ravel().
 * logits (optional, [T][E]): the raw logits, for tests.  The same bits on every launch: no atomics.
 * ntk_moe_gate_up: act[p][0 .. inter) = SiLU(Wg[e] . xn[t]) x (Wu[e] . xn[t]), e = ids[p] as the work list names it (w_gate / w_up: [E][inter][hidden]).
 * ntk_moe_down: y[t][0 .. hidden) = resid[t] + sum over k ascending of w[t][k] x (Wd[e_k] . act[t K + k]) (w_down: [E][hidden][inter]); y may be resid.
 * part: scratch of T K hidden floats (every pair's products before the sum).  A pair's result does not depend on T or on which pairs share its expert.
 *
 * ntk_moe_workspace_layout: byte offsets of the NTK_MOE_WS_* sections (each 256-byte aligned) of one workspace for a pass of up to T rows, and its size
 * (0: arguments out of range); ntk_moe_workspace_bytes: the size alone. */
enum { NTK_MOE_WS_XN = 0, NTK_MOE_WS_ACT, NTK_MOE_WS_PART, NTK_MOE_WS_W, NTK_MOE_WS_IDS, NTK_MOE_WS_PAIRS, NTK_MOE_WS_OFFSETS, NTK_MOE_WS_SECTIONS };
size_t ntk_moe_workspace_layout(int T, int E, int K, int inter, int hidden, size_t off[NTK_MOE_WS_SECTIONS]);
size_t ntk_moe_workspace_bytes(int T, int E, int K, int inter, int hidden);
/* LDS bytes a launch needs for rows of `columns` columns: ntk_moe_gate_up stages a row of each of its two matrices per wave (dt_a, dt_b), ntk_moe_down one
 * (dt_b < 0); 0: a type that is not taken or columns that are not whole blocks.  A launch beyond NTK_MOE_LDS_MAX returns NTK_E_SHAPE: the engine refuses
 * such a file at load. */
#define NTK_MOE_LDS_MAX 65536
size_t ntk_moe_lds_bytes(int dt_a, int dt_b, int columns);
int ntk_moe_route(const float* xn, const float* router, int T, int hidden, int E, int K, int* ids, float* w, int* offsets, int* pairs, float* logits,
                  void* stream);
int ntk_moe_gate_up(float* act, const float* xn, const void* w_gate, int dt_gate, const void* w_up, int dt_up, const int* offsets, const int* pairs,
                    int T, int hidden, int inter, int E, int K, void* stream);
int ntk_moe_down(float* y, const float* resid, const float* act, const void* w_down, int dt_down, const int* ids, const float* w, const int* offsets,
                 const int* pairs, float* part, int T, int hidden, int inter, int E, int K, void* stream);
/* The PROMPT forms of ntk_moe_gate_up / ntk_moe_down (csrc/moe_gemm.hip): a grouped GEMM on the F32 matrix cores.  Every argument means what it means
 * above -- the same work list, the same act / part / y layouts, y may be resid -- so either form runs on the same buffers; the limits, the expert types
 * and every refusal (code for code, outputs untouched) are the GEMV form's, except that no row is too long.  Weights are dequantised to F32 as the dense
 * prompt GEMM does (csrc/gemm_deq.hip.h) and multiplied with the unrounded F32 activations by v_mfma_f32_16x16x4_f32 with F32 accumulation: results
 * within the GEMV bar of the GEMV form, in another summation order.  A TILE is up to 16 consecutive work-list entries of one expert; the grid holds
 * ceil(T K / 16) + E tile slots and each workgroup finds its tile from the offsets on the device (csrc/moe_tiles.h), so no launch parameter depends on
 * the routing and nothing is atomic.  Offsets are clamped to the list and a pair index outside [0, T K) is skipped, as in the GEMV form.  A pair's bits
 * do not depend on T, on the pairs it shares a tile with, on its tile or column, or on the launch; a NaN row stays in its own pairs.
 * ntk_moe_gemm_gate_up: two launches, the gate products waiting in act for the up launch's SiLU(g) x u epilogue, g / (1 + expf(-g)) * u as above;
 * scratch / scratch_bytes: at least ntk_moe_gemm_scratch_bytes (today 0 for every shape: scratch may then be NULL; fewer bytes: NTK_E_SHAPE).
 * ntk_moe_gemm_down: the products into part, then the GEMV form's combine, resid[t] + sum_k fmaf(w[p], part[p], s): the same bits for the same part. */
size_t ntk_moe_gemm_scratch_bytes(int T, int E, int K, int inter, int hidden);   /* may be 0; 0 also for counts out of range */
int ntk_moe_gemm_gate_up(float* act, const float* xn, const void* w_gate, int dt_gate, const void* w_up, int dt_up, const int* offsets, const int* pairs,
                         void* scratch, size_t scratch_bytes, int T, int hidden, int inter, int E, int K, void* stream);
int ntk_moe_gemm_down(float* y, const float* resid, const float* act, const void* w_down, int dt_down, const int* ids, const float* w, const int* offsets,
                      const int* pairs, float* part, int T, int hidden, int inter, int E, int K, void* stream);

#ifdef __cplusplus
}
#endif
#if defined(__GNUC__)
#pragma GCC visibility pop
#endif
#endif /* NTK_ENGINE_H */
