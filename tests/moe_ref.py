"""The reference of the mixture-of-experts tests: an oracle that runs the routed expert FFN, the test models, and what the oracle computes on them.

MoEOracle subclasses tests/qwen3_ref.Qwen3Oracle (so it keeps the Q | K | V biases, the per-head Q / K norms and key_length) without touching oracle/, and
overrides forward(): a layer that carries blk.N.ffn_gate_inp.weight runs, per row of the pass,
  logits = O.gemv(router F32 [E][hidden], xn)          xn = O.rmsnorm(hidden, ffn_norm)
  ids    = the K largest logits in descending order, equal logits to the lower expert (a stable argsort of -logits)
  w      = softmax over those K, max-subtracted, float32 (llama.cpp: softmax over all E, top-K, renormalise -- the same numbers)
  act_k  = O.silu_mul(O.gemv(gate_exps bytes of expert ids[k], xn), O.gemv(up_exps bytes of ids[k], xn))
  y      = sum over k ASCENDING of w[k] * O.gemv(down_exps bytes of ids[k], act_k), float32; hidden += y
where the bytes of expert e are the contiguous block e x rows x row_bytes of the 3-D tensor.  A layer without the router runs OracleModel's dense FFN.
Every routed row's logits are kept in .routing: [(layer, logits[E])], for the guard's gap condition.

The constructor's switches build the WRONG oracles the guard measures against: weights="full" (the softmax over all E, not renormalised), "uniform" (1 / K);
select="smallest" (the K smallest logits); swap_gate_up; reverse_down (expert E - 1 - e for the down matrix only).

The models (make_synthetic_llama into a temporary directory; two layers, context 1024, theta 1e6):
  moe8q8    qwen3moe, hidden 256, 4 / 2 heads of 64, norms, E 8 / K 2, I_e 96, Q8_0
  moe4k     qwen3moe, hidden 256, 4 / 2 heads of 128 (key_length), norms, E 4 / K 2, I_e 768, Q4_K_M with Q6_K ffn_down_exps: 630-byte rows
  mixtral4  llama, hidden 512, 4 / 2 heads, no norms, E 4 / K 2, I_e = feed_forward_length = 256 (no expert_feed_forward_length key), Q8_0
  half      moe8q8's shape with layer 0 dense and layer 1 routed
SEEDS and ROUTER_SCALE were searched on the CPU with the oracle alone (tests/test_moe_cpu.py asserts what they were searched for: every wrong oracle ten
bars away, and at every row the GPU tests run a gap between the K-th and (K + 1)-th router logit of at least 16 GEMV bars)."""
from __future__ import annotations

import numpy as np

from ntransformer_amd import gguf as G
from oracle import oracle as O
from qwen3_ref import Qwen3Oracle, dist, oracle_file  # noqa: F401  (dist: re-exported for the tests)

TOL, SCORE_TOL, CTX = 1e-3, 2e-3, 1024
NORM_AMP = 0.5
ROUTER_SCALE = 2.0
# name: (shape, mix, architecture, norms?, E, K, I_e or None (feed_forward_length), routed layers or None (all), overrides)
MODELS = {
    "moe8q8": (G.MOE_8Q8, "Q8_0", "qwen3moe", True, 8, 2, 96, None, None),
    "moe4k": (G.MOE_4K, "Q4_K_M", "qwen3moe", True, 4, 2, 768, None, {"ffn_down_exps": "Q6_K"}),
    "mixtral4": (G.MIXTRAL_4, "Q8_0", "llama", False, 4, 2, None, None, None),
    "half": (G.MOE_8Q8, "Q8_0", "qwen3moe", True, 8, 2, 96, (1,), None),
}
SEEDS = {"moe8q8": 20261101, "moe4k": 20261101, "mixtral4": 20261101, "half": 20261101}
LENGTHS = (1, 3, 4, 37, 70)
GUARD_LENGTHS = (3, 4, 37, 70)
N_STEPS = 8
WRONG = {"full": dict(weights="full"), "uniform": dict(weights="uniform"), "smallest": dict(select="smallest"), "swapped": dict(swap_gate_up=True),
         "reversed": dict(reverse_down=True)}


def tol_for(y, in_f):
    """the project's GEMV bar (tests/test_hip_kernels.py): 4e-6 sqrt(in) max(1, |y|max)"""
    return 4e-6 * np.sqrt(in_f) * max(1.0, float(np.abs(y).max()))


def select_experts(logits, K, smallest=False):
    """the K largest (smallest) logits in descending (ascending) order, equal values to the lower index"""
    key = np.asarray(logits, np.float32)
    order = np.argsort(key if smallest else -key, kind="stable")
    return order[:K].astype(np.int32)


def route_weights(logits, ids, how="renorm"):
    lg = np.asarray(logits, np.float32)
    if how == "uniform":
        return np.full(len(ids), np.float32(1.0 / len(ids)), np.float32)
    pool = lg if how == "full" else lg[ids]
    ex = np.exp((pool - pool.max()).astype(np.float32)).astype(np.float32)
    den = np.float32(0.0)
    for v in ex:
        den = np.float32(den + v)
    sel = np.exp((lg[ids] - pool.max()).astype(np.float32)).astype(np.float32)
    return (sel / den).astype(np.float32)


def work_list(ids, E):
    """the expert-major work list of ids [T][K]: offsets [E + 1] and pairs [T K] = the pair indices t K + k sorted by (expert, pair index), built the way
    the launch builds it: every expert walks the pairs in ascending order"""
    flat = np.asarray(ids, np.int32).reshape(-1)
    offsets, pairs = np.zeros(E + 1, np.int32), []
    for e in range(E):
        mine = [p for p in range(flat.size) if flat[p] == e]
        pairs += mine
        offsets[e + 1] = offsets[e] + len(mine)
    return offsets, np.asarray(pairs, np.int32)


class MoEOracle(Qwen3Oracle):
    def __init__(self, gguf_path, max_context=4096, weights="renorm", select="largest", swap_gate_up=False, reverse_down=False, **kw):
        super().__init__(gguf_path, max_context, **kw)
        assert weights in ("renorm", "full", "uniform") and select in ("largest", "smallest")
        self.weights, self.select, self.swap_gate_up, self.reverse_down = weights, select, swap_gate_up, reverse_down
        m = self.f.meta
        arch = m.get("general.architecture", b"llama")
        arch = arch.decode() if isinstance(arch, bytes) else arch
        self.E = int(m.get(arch + ".expert_count", 0))
        self.K = int(m.get(arch + ".expert_used_count", 0))
        self.Ie = int(m.get(arch + ".expert_feed_forward_length", self.inter))
        self.routing = []

    def expert(self, name, e, rows, cols):
        """(bytes, dtype) of expert e of a 3-D tensor: the contiguous block e x rows x row_bytes"""
        t = self.f.tensors[name].ggml_type
        n = rows * G.row_bytes(t, cols)
        return self.f.raw(name)[e * n:(e + 1) * n], G.GGML_TO_DT[t]

    def moe_ffn_row(self, layer, xn):
        p, H, Ie = "blk.%d." % layer, self.hidden, self.Ie
        logits = O.gemv(self.f.raw(p + "ffn_gate_inp.weight"), xn, self.E, H, G.DT_F32)
        self.routing.append((layer, logits.copy()))
        ids = select_experts(logits, self.K, self.select == "smallest")
        w = route_weights(logits, ids, self.weights)
        y = np.zeros(H, np.float32)
        for k, e in enumerate(int(i) for i in ids):
            wg, dg = self.expert(p + "ffn_gate_exps.weight", e, Ie, H)
            wu, du = self.expert(p + "ffn_up_exps.weight", e, Ie, H)
            g, u = O.gemv(wg, xn, Ie, H, dg), O.gemv(wu, xn, Ie, H, du)
            act = O.silu_mul(u, g) if self.swap_gate_up else O.silu_mul(g, u)
            wd, dd = self.expert(p + "ffn_down_exps.weight", self.E - 1 - e if self.reverse_down else e, H, Ie)
            y = (y + w[k] * O.gemv(wd, act, H, Ie, dd)).astype(np.float32)
        return y

    def forward(self, tokens, start_pos, trace=None):
        """OracleModel.forward with the FFN of a routed layer replaced (see the module docstring); the attention side goes through self._gemv, Qwen3Oracle's"""
        T, H = len(tokens), self.hidden
        q_dim, kv_dim = self.nh * self.hd, self.nkv * self.hd
        hidden = self.embed(tokens)
        positions = [start_pos + i for i in range(T)]
        if trace is not None:
            trace["layer_in"], trace["layer_out"] = [], []
        for i in range(self.n_layers):
            p = "blk.%d." % i
            if trace is not None:
                trace["layer_in"].append(hidden.copy())
            resid = O.rmsnorm(hidden, self.f.f32(p + "attn_norm.weight"), self.eps)
            q = np.stack([self._gemv(p + "attn_q.weight", resid[t], q_dim, H) for t in range(T)])
            k = np.stack([self._gemv(p + "attn_k.weight", resid[t], kv_dim, H) for t in range(T)])
            v = np.stack([self._gemv(p + "attn_v.weight", resid[t], kv_dim, H) for t in range(T)])
            q, k = O.rope(q.reshape(-1), k.reshape(-1), positions, self.nh, self.nkv, self.hd, self.theta)
            O.copy_to_kv_cache(self.k_cache[i], self.v_cache[i], k, v.reshape(-1), T, self.nkv, self.hd, start_pos, self.max_seq)
            total = start_pos + T
            if T == 1:
                att = O.attention_decode(q, self.k_cache[i], self.v_cache[i], total, self.nh, self.nkv, self.hd, self.max_seq, self.scale)
            else:
                att = O.attention_prefill(q, self.k_cache[i], self.v_cache[i], T, start_pos, self.nh, self.nkv, self.hd, self.max_seq, self.scale)
            att = att.reshape(T, q_dim)
            hidden = hidden + np.stack([self._gemv(p + "attn_output.weight", att[t], H, q_dim) for t in range(T)])
            resid = O.rmsnorm(hidden, self.f.f32(p + "ffn_norm.weight"), self.eps)
            if p + "ffn_gate_inp.weight" in self.f.tensors:
                outs = [self.moe_ffn_row(i, resid[t]) for t in range(T)]
            else:
                outs = []
                for t in range(T):
                    gate = self._gemv(p + "ffn_gate.weight", resid[t], self.inter, H)
                    up = self._gemv(p + "ffn_up.weight", resid[t], self.inter, H)
                    outs.append(self._gemv(p + "ffn_down.weight", O.silu_mul(gate, up), H, self.inter))
            hidden = hidden + np.stack(outs)
            if trace is not None:
                trace["layer_out"].append(hidden.copy())
        last = O.rmsnorm(hidden[T - 1], self.f.f32("output_norm.weight"), self.eps)
        return self._gemv(self.out_name, last, self.vocab, H)

    def min_gap_ratio(self):
        """over every routed row seen so far: (K-th largest logit - (K + 1)-th) / (16 tol_for(logits, hidden)); inf where K = E"""
        worst = np.inf
        for _, lg in self.routing:
            s = np.sort(np.asarray(lg, np.float64))[::-1]
            if self.K < len(s):
                worst = min(worst, float(s[self.K - 1] - s[self.K]) / (16.0 * tol_for(lg, self.hidden)))
        return worst


def prompt_tokens(n=70, seed=41, key=20261101):
    r = np.random.Generator(np.random.Philox(key=[key, seed]))
    return [256] + [int(t) for t in r.integers(0, 256, n - 1)]


_files, _refs = {}, {}


def model_file(name, tmp_path_factory, seed=None, **kw):
    """the model's GGUF, written once per session; kw: other arguments of make_synthetic_llama, under their own key"""
    seed = SEEDS[name] if seed is None else seed
    key = (name, seed, repr(sorted((k, repr(v)) for k, v in kw.items())))
    if key not in _files:
        shape, mix, arch, norms, E, K, Ie, layers, over = MODELS[name]
        args = dict(arch=arch, qk_norm=NORM_AMP if norms else None, experts=E, experts_used=K, expert_inter=Ie, router_scale=ROUTER_SCALE,
                    moe_layers=layers, overrides=over)
        args.update(kw)
        path = str(tmp_path_factory.mktemp(name) / "model.gguf")
        G.make_synthetic_llama(path, shape, mix, seed=seed, **args)
        _files[key] = path
    return _files[key]


def oracle_passes(path, passes, **kw):
    """the oracle through a list of (tokens, start_pos) passes on one model object: the logits of each"""
    m = MoEOracle(path, CTX, **kw)
    return [m.forward(list(t), s) for t, s in passes]


# the passes of the engine tests beyond the 70-token prompt and the decode steps: (slot tests) short prompts and their steps, (q8_0) a 3-token pass at 37
SLOT_PASSES = lambda toks: [[(toks[:4], 0), ([9], 4)], [(toks[:3], 0), ([10], 3)]]


def oracle_ref(name, tmp_path_factory, seed=None, guard=True):
    """The oracle on the model, once per session, read only: logits behind prompts of LENGTHS tokens, N_STEPS teacher-forced decode steps behind the 37-token
    prompt, the logits at every position of that prompt (score), the chunked 37 + 33 pass, the slot tests' passes -- every routed row of all of them in
    "gap" (the smallest gap ratio, see MoEOracle.min_gap_ratio) -- and, for the guard, the prompt logits of every wrong oracle."""
    key = (name, SEEDS[name] if seed is None else seed, guard)
    if key not in _refs:
        path = model_file(name, tmp_path_factory, seed=seed)
        toks = prompt_tokens()
        ref = dict(path=path, tokens=toks)
        gaps = []
        ref["prompt"] = {}
        for T in LENGTHS:
            m = MoEOracle(path, CTX)
            ref["prompt"][T] = m.forward(toks[:T], 0)
            gaps.append(m.min_gap_ratio())
        if guard:
            for wrong, kw in WRONG.items():
                ref[wrong] = {T: MoEOracle(path, CTX, **kw).forward(toks[:T], 0) for T in GUARD_LENGTHS}
        m = MoEOracle(path, CTX)
        trace = {}
        lg = m.forward(toks[:37], 0, trace=trace)
        normed = O.rmsnorm(trace["layer_out"][-1], m.f.f32("output_norm.weight"), m.eps)
        ref["all37"] = np.stack([m._gemv(m.out_name, normed[t], m.vocab, m.hidden) for t in range(37)])
        fed, steps = [int(np.argmax(lg))], []
        for i in range(N_STEPS):
            steps.append(m.forward([fed[-1]], 37 + i))
            fed.append(int(np.argmax(steps[-1])))
        ref["fed"], ref["steps"] = fed[:N_STEPS], steps
        gaps.append(m.min_gap_ratio())
        m2 = MoEOracle(path, CTX)
        m2.forward(toks[:37], 0)
        ref["chunked"] = m2.forward(toks[37:70], 37)
        gaps.append(m2.min_gap_ratio())
        ref["slots"] = []
        for passes in SLOT_PASSES(toks):
            m3 = MoEOracle(path, CTX)
            ref["slots"].append([m3.forward(list(t), s) for t, s in passes][-1])
            gaps.append(m3.min_gap_ratio())
        # the q8_0 test (tests/test_engine_qwen2_gpu.py::q8_distances): a 3-token pass behind the 37-token prompt, then the fed tokens from position 40
        m4 = MoEOracle(path, CTX)
        m4.forward(toks[:37], 0)
        m4.forward(toks[37:40], 37)
        for i, tok in enumerate(ref["fed"]):
            m4.forward([tok], 40 + i)
        gaps.append(m4.min_gap_ratio())
        ref["gap"] = min(gaps)
        _refs[key] = ref
    return _refs[key]
