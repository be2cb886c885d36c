"""The reference of the Qwen2 tests: a bias-aware oracle, and the test models with what it computes on them.

patch_oracle() gives the tests an oracle that adds the Q | K | V projection biases without touching oracle/: OracleModel._gemv(name, ...) is keyed by tensor
name, and the wrapper adds the F32 values of `<name minus ".weight">.bias` to the result when the file carries that tensor -- one float32 add per element, ahead
of the rotation, as llama.cpp's Qwen2 graph does.  OracleModel already reads the hyper-parameters under the file's own architecture prefix.

The models (written by make_synthetic_llama(arch="qwen2", qkv_bias=scale) into a temporary directory, context 1024, theta 1e6, eps 1e-6, two layers):
  qt64    the TINY shape: hidden 256, 4 / 2 heads, head_dim 64, Q8_0
  qt128   hidden 256, 2 / 1 heads, head_dim 128, Q4_K_M
  q7      hidden 1792, inter 512, vocab 512, 14 / 2 heads, head_dim 128, Q8_0: Qwen2.5-7B's 7 query heads per KV head
BIAS_SCALE and the seeds were chosen on the CPU with the oracle alone (tests/test_qkv_bias_cpu.py asserts what they were chosen for: the bias-aware oracle's
logits are at least ten logit bars away from the plain oracle's at every tested prompt length)."""
from __future__ import annotations

import numpy as np
import pytest

from ntransformer_amd import gguf as G
from oracle import oracle as O

TOL, SCORE_TOL, CTX = 1e-3, 2e-3, 1024
BIAS_SCALE, SEED = 0.5, 20261021
MODELS = {"qt64": (G.QWEN_T64, "Q8_0"), "qt128": (G.QWEN_T128, "Q4_K_M"), "q7": (G.QWEN_7, "Q8_0")}
LENGTHS = (1, 3, 4, 37, 70)
GUARD_LENGTHS = (3, 4, 37, 70)
N_STEPS = 8


def patch_oracle(monkeypatch):
    """OracleModel._gemv -> the same product plus the tensor's bias where the file has one"""
    plain = O.OracleModel._gemv

    def with_bias(self, name, x, out_f, in_f):
        y = plain(self, name, x, out_f, in_f)
        bias = name[:-len(".weight")] + ".bias" if name.endswith(".weight") else None
        if bias is not None and bias in self.f.tensors:
            y = (np.asarray(y, np.float32) + self.f.f32(bias)).astype(np.float32)
        return y

    monkeypatch.setattr(O.OracleModel, "_gemv", with_bias)


def prompt_tokens(n=70, seed=41):
    r = np.random.Generator(np.random.Philox(key=[SEED, seed]))
    return [256] + [int(t) for t in r.integers(0, 256, n - 1)]


def dist(a, b):
    return float(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)).max())


_files, _refs = {}, {}


def model_file(name, tmp_path_factory, **kw):
    """the model's GGUF, written once per session; kw: other arguments of make_synthetic_llama, under their own key"""
    key = (name, repr(sorted((k, repr(v)) for k, v in kw.items())))
    if key not in _files:
        shape, mix = MODELS[name]
        args = dict(arch="qwen2", qkv_bias=BIAS_SCALE)
        args.update(kw)
        path = str(tmp_path_factory.mktemp(name) / "model.gguf")
        G.make_synthetic_llama(path, shape, mix, seed=SEED, **args)
        _files[key] = path
    return _files[key]


def oracle_ref(name, tmp_path_factory):
    """The bias-aware oracle on the model, once per session, read only: logits behind prompts of LENGTHS tokens, N_STEPS teacher-forced decode steps behind the
    37-token prompt, the logits at every position of that prompt (score), the chunked 37 + 33 pass -- and the PLAIN oracle's prompt logits (the guard)."""
    if name not in _refs:
        path = model_file(name, tmp_path_factory)
        toks = prompt_tokens()
        ref = dict(path=path, tokens=toks)
        ref["plain"] = {T: O.OracleModel(path, CTX).forward(toks[:T], 0) for T in GUARD_LENGTHS}
        with pytest.MonkeyPatch.context() as mp:
            patch_oracle(mp)
            ref["prompt"] = {T: O.OracleModel(path, CTX).forward(toks[:T], 0) for T in LENGTHS}
            m = O.OracleModel(path, CTX)
            trace = {}
            lg = m.forward(toks[:37], 0, trace=trace)
            normed = O.rmsnorm(trace["layer_out"][-1], m.f.f32("output_norm.weight"), m.eps)
            ref["all37"] = np.stack([m._gemv(m.out_name, normed[t], m.vocab, m.hidden) for t in range(37)])
            fed, steps = [int(np.argmax(lg))], []
            for i in range(N_STEPS):
                steps.append(m.forward([fed[-1]], 37 + i))
                fed.append(int(np.argmax(steps[-1])))
            ref["fed"], ref["steps"] = fed[:N_STEPS], steps
            m2 = O.OracleModel(path, CTX)
            m2.forward(toks[:37], 0)
            ref["chunked"] = m2.forward(toks[37:70], 37)
        _refs[name] = ref
    return _refs[name]
