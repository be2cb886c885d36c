"""What the scoring tests (test_score_cpu.py, test_score_gpu.py) compare against: a float64 log-softmax + gather + first maximum of F32 logits, the
40-token prompt they score, and the oracle's logits at EVERY position of it (OracleModel keeps the last row only)."""
import numpy as np

from ntransformer_amd import gguf as G
from oracle import oracle as O

SEED = 20261018      # of the random tail of the prompt; test_score_gpu.py asserts what it was chosen for (clear top-2 margins on half of the rows)
N_TOKENS = 40
MODELS = [("tiny_q8_0", G.TINY, "Q8_0"), ("tiny_q4_k_m", G.TINY, "Q4_K_M"), ("tiny_mixed", G.TINY, "MIXED"),
          ("small_q8_0", G.SMALL, "Q8_0"), ("small_q4_k_m", G.SMALL, "Q4_K_M")]


def logprob_ref(logits, targets):
    """(float64 log softmax(logits[r])[targets[r]] -- 0 where targets[r] < 0 --, first index of each row's maximum).  Rows as ntk_logprob_rows defines them:
    -inf entries add nothing, a row of -inf only or one with a NaN is NaN, and the maximum ignores NaN (no candidate at all: index 0)."""
    x = np.asarray(logits, np.float32).astype(np.float64)
    t = np.asarray(targets, np.int64)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        m = x.max(axis=1)
        lse = m + np.log(np.exp(x - m[:, None]).sum(axis=1))
        lp = x[np.arange(len(t)), np.clip(t, 0, x.shape[1] - 1)] - lse
    lp[t < 0] = 0.0
    top1 = np.where(np.isnan(x), -np.inf, x).argmax(axis=1)
    return lp, top1.astype(np.int32)


def prompt_of(z, vocab):
    """the golden prompt, extended with seeded random ids to N_TOKENS tokens"""
    p = [int(t) for t in z["prompt"]][:N_TOKENS]
    r = np.random.default_rng(SEED)
    return p + [int(t) for t in r.integers(0, vocab, N_TOKENS - len(p))]


def oracle_all_logits(path, ctx, tokens, start_pos=0):
    """F32 logits [len(tokens)][vocab] of the oracle: the final layer_out of OracleModel.forward, O.rmsnorm and O.gemv of every row over the head"""
    m = O.OracleModel(path, ctx)
    trace = {}
    m.forward(tokens, start_pos, trace=trace)
    normed = O.rmsnorm(trace["layer_out"][-1], m.f.f32("output_norm.weight"), m.eps)
    return np.stack([m._gemv(m.out_name, normed[t], m.vocab, m.hidden) for t in range(len(tokens))])


_CASES = {}


def oracle_case(name, tmp_path_factory):
    """(path, ctx, tokens, oracle logits [N_TOKENS][vocab]) of a golden model (test_oracle_golden.golden_model: committed, or regenerated from its seed) --
    computed once per session, shared by the tests, never written to"""
    if name not in _CASES:
        from test_oracle_golden import golden_model
        shape, mix = next((s, m) for n, s, m in MODELS if n == name)
        path, z = golden_model(name, shape, mix, tmp_path_factory.mktemp(name))
        tokens = prompt_of(z, shape.vocab)
        logits = oracle_all_logits(path, int(z["ctx"]), tokens)
        logits.setflags(write=False)
        _CASES[name] = (path, int(z["ctx"]), tokens, logits)
    return _CASES[name]
