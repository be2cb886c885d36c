"""The reference of the Qwen3 tests: an oracle that knows the per-head Q / K RMSNorm and a head size of its own, and the test models with what it computes.

Qwen3Oracle subclasses OracleModel without touching oracle/:
  * where the file has <arch>.attention.key_length it takes hd from it, scale = 1 / sqrt(hd), and re-sizes k_cache / v_cache (OracleModel computes
    hidden / heads); forward() already carries heads x hd separately from the hidden size;
  * _gemv(name, ...) is keyed by tensor name: the wrapper adds `<name minus ".weight">.bias` where the file has one (tests/qkv_bias_ref.py's wrapper) and
    then, for attn_q.weight / attn_k.weight, applies O.rmsnorm(y.reshape(-1, hd), f32(attn_q_norm.weight | attn_k_norm.weight), eps) where the file has
    that tensor -- bias first, norm second, both ahead of the rotation: llama.cpp's order.
The constructor's switches build the WRONG oracles the guard measures against: norms="none" (no norm), "swapped" (q's vector on k and k's on q),
decoupled=False (hd stays hidden / heads, the norm vector cut to it), bias_first=False (the norm ahead of the bias).

The models (make_synthetic_llama into a temporary directory; two layers, context 1024, theta 1e6, eps 1e-6, norm weights 1 + 0.5 u):
  q3n64     hidden 256, 4 / 2 heads, head_dim 64 = hidden / heads, norms, Q8_0
  q3w128    hidden 256, 4 / 2 heads, head_dim 128: heads x head_dim = 512 > hidden, norms, Q4_K_M
  q3g128    hidden 1024, 8 / 2 heads, head_dim 128 = hidden / heads, norms, 4 query heads per KV head, BF16
  nemo128   hidden 512, 2 / 1 heads, head_dim 128: heads x head_dim = 256 < hidden, architecture `llama`, key_length and NO norms, Q8_0
NORM_AMP and SEED were chosen on the CPU with the oracle alone; tests/test_qwen3_cpu.py asserts what they were chosen for."""
from __future__ import annotations

import numpy as np

from ntransformer_amd import gguf as G
from oracle import oracle as O

TOL, SCORE_TOL, CTX = 1e-3, 2e-3, 1024
NORM_AMP, SEED = 0.5, 20261022
BIAS_SCALE = 0.5          # of the model that carries biases AND norms (the order of the two)
# name: (shape, mix, architecture, norms?)
MODELS = {"q3n64": (G.QWEN3_N64, "Q8_0", "qwen3", True), "q3w128": (G.QWEN3_W128, "Q4_K_M", "qwen3", True),
          "q3g128": (G.QWEN3_G128, "BF16", "qwen3", True), "nemo128": (G.NEMO_128, "Q8_0", "llama", False)}
LENGTHS = (1, 3, 4, 37, 70)
GUARD_LENGTHS = (3, 4, 37, 70)
N_STEPS = 8


class Qwen3Oracle(O.OracleModel):
    def __init__(self, gguf_path, max_context=4096, norms="own", decoupled=True, bias_first=True):
        super().__init__(gguf_path, max_context)
        assert norms in ("own", "swapped", "none")
        self.norms, self.bias_first = norms, bias_first
        m = self.f.meta
        arch = m.get("general.architecture", b"llama")
        arch = arch.decode() if isinstance(arch, bytes) else arch
        if decoupled and arch + ".attention.key_length" in m:
            self.hd = G.model_head_dim(m)
            self.scale = np.float32(1.0) / np.sqrt(np.float32(self.hd))
            per = self.nkv * self.hd
            self.k_cache = np.zeros((self.n_layers, self.max_seq * per), np.uint16)
            self.v_cache = np.zeros((self.n_layers, self.max_seq * per), np.uint16)

    def _gemv(self, name, x, out_f, in_f):
        y = super()._gemv(name, x, out_f, in_f)
        stem = name[:-len(".weight")] if name.endswith(".weight") else None
        biased = stem is not None and stem + ".bias" in self.f.tensors
        if biased and self.bias_first:
            y = (np.asarray(y, np.float32) + self.f.f32(stem + ".bias")).astype(np.float32)
        if stem is not None and self.norms != "none" and (stem.endswith(".attn_q") or stem.endswith(".attn_k")):
            which = stem[-1] if self.norms == "own" else ("k" if stem[-1] == "q" else "q")
            norm = stem[:-1] + which + "_norm.weight"
            if norm in self.f.tensors:
                w = np.asarray(self.f.f32(norm), np.float32)[:self.hd]          # (cut only by the decoupled=False oracle)
                y = O.rmsnorm(np.asarray(y, np.float32).reshape(-1, self.hd), w, self.eps).reshape(-1)
        if biased and not self.bias_first:          # (the wrong order, for the guard of the bias + norm model)
            y = (np.asarray(y, np.float32) + self.f.f32(stem + ".bias")).astype(np.float32)
        return y


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
        shape, mix, arch, norms = MODELS[name]
        args = dict(arch=arch, qk_norm=NORM_AMP if norms else None)
        args.update(kw)
        path = str(tmp_path_factory.mktemp(name) / "model.gguf")
        G.make_synthetic_llama(path, shape, mix, seed=SEED, **args)
        _files[key] = path
    return _files[key]


_twins = {}


def oracle_file(path):
    """The file the oracle reads for the engine's file `path`: the oracle has no BF16, so a file with BF16 tensors gets a twin holding the SAME values as F32
    (gguf.write_f32_twin: bfloat16 -> float is exact; tests/test_engine_unquantised_gpu.py's construction); every other file is read as it is."""
    if path not in _twins:
        f = G.read_gguf(path)
        bf16 = any(t.ggml_type == G.GGML_BF16 for t in f.tensors.values())
        f.close()
        if bf16:
            G.write_f32_twin(path, path + ".f32twin.gguf")
        _twins[path] = path + ".f32twin.gguf" if bf16 else path
    return _twins[path]


def oracle_passes(path, passes, **kw):
    """the norm-aware oracle through a list of (tokens, start_pos) passes on one model object: the logits of each"""
    m = Qwen3Oracle(oracle_file(path), CTX, **kw)
    return [m.forward(list(t), s) for t, s in passes]


def oracle_ref(name, tmp_path_factory):
    """The norm-aware oracle on the model, once per session, read only: logits behind prompts of LENGTHS tokens, N_STEPS teacher-forced decode steps behind
    the 37-token prompt, the logits at every position of that prompt (score), the chunked 37 + 33 pass -- and, for the guard, the prompt logits of the
    plain oracle's arithmetic ("none": no norm; the file's head size), of the swapped vectors, and of hidden / heads where that oracle runs at all."""
    if name not in _refs:
        path = model_file(name, tmp_path_factory)
        shape, mix, arch, norms = MODELS[name]
        toks = prompt_tokens()
        ref = dict(path=path, tokens=toks)
        path = oracle_file(path)          # (from here on `path` is what the oracle reads; ref["path"] is the engine's file)
        ref["prompt"] = {T: Qwen3Oracle(path, CTX).forward(toks[:T], 0) for T in LENGTHS}
        if norms:
            ref["none"] = {T: Qwen3Oracle(path, CTX, norms="none").forward(toks[:T], 0) for T in GUARD_LENGTHS}
            ref["swapped"] = {T: Qwen3Oracle(path, CTX, norms="swapped").forward(toks[:T], 0) for T in GUARD_LENGTHS}
        # hidden / heads: it "runs" where its projections stay inside the file's tensors -- heads x (hidden / heads) rows at most heads x head_dim
        if shape.head_dim and shape.hidden // shape.heads < shape.head_dim:
            ref["coupled"] = {T: Qwen3Oracle(path, CTX, decoupled=False).forward(toks[:T], 0) for T in GUARD_LENGTHS}
        m = Qwen3Oracle(path, CTX)
        trace = {}
        lg = m.forward(toks[:37], 0, trace=trace)
        normed = O.rmsnorm(trace["layer_out"][-1], m.f.f32("output_norm.weight"), m.eps)
        ref["all37"] = np.stack([m._gemv(m.out_name, normed[t], m.vocab, m.hidden) for t in range(37)])
        fed, steps = [int(np.argmax(lg))], []
        for i in range(N_STEPS):
            steps.append(m.forward([fed[-1]], 37 + i))
            fed.append(int(np.argmax(steps[-1])))
        ref["fed"], ref["steps"] = fed[:N_STEPS], steps
        m2 = Qwen3Oracle(path, CTX)
        m2.forward(toks[:37], 0)
        ref["chunked"] = m2.forward(toks[37:70], 37)
        _refs[name] = ref
    return _refs[name]
