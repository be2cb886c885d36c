# the product's device sources
KERNELS  := gemv.hip gemv_dense16.hip gemv_rp.hip gemm_prefill.hip attention.hip elementwise.hip sampling.hip sampling_batch.hip gemm_f16.hip gemm_dense16.hip tp.hip attention_mfma.hip attention_q8.hip attention_batch.hip logprob.hip kv_ops.hip qkv_bias.hip qk_norm.hip moe.hip moe_gemm.hip
