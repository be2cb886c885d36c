"""GPU tests of the engine on models whose widths are NOT multiples of 256 columns: the tensor-by-tensor fallbacks (Model::repack_one; not_taken() in
model_prompt.cpp (layers_1to1, lm_head) / model_decode.cpp) that no other test forces.

  model   shape                                             what it forces
  w320    hidden 320, inter 864, 2 layers, 5 / 1 heads      every projection and the LM head refused by the FP16 prompt GEMM -> the ragged-tail
          (head_dim 64); Q8_0, Q4_0                         ntk_gemm_quant; decode on rows that end in a half lane; nothing repacked
  w384    hidden 384, inter 896, 2 layers, 6 / 2 heads      Q8_0: the FP16 GEMM and its operand-plane producers at half a sum unit (128 columns) through
          (head_dim 64); Q8_0, Q4_0                         a whole layer; Q4_0: refused (384 and 896 are not multiples of 256)
  w512    hidden 512, inter 11008, 1 layer, 4 / 2 heads     lane-major Q | K | V, Wo, gate | up and LM head beside a RAW three-slice down projection
          (head_dim 128); Q8_0; also kv_cache = q8_0        (11008 = 3 x 3712: no lane-major form) in one layer
  w320x   hidden 320, inter 4128, 1 layer, 5 / 1 heads      a ragged two-slice down projection (2112 + 2016 columns): the cross-slice combine with the
          Q8_0, Q4_0                                        residual

The models are written with gguf.make_synthetic_llama (vocab 512, bos 256, eos 257, ctx 256); the oracle is oracle.OracleModel on the same file.  Bars
(tests/test_engine_gpu.py): every logits row within TOL = 1e-3 of the oracle's, the greedy choice equal wherever the oracle's top-two margin exceeds
2 TOL.

kv_cache = q8_0 (w512): the oracle keeps an F16 cache and is not that engine's reference -- an 8-bit cache moves logits by 2 .. 4 e-2 of their RMS
(profiles/kv_q8_0_quality.txt) -- so that variant is held to the exact properties: repack on / off give the same bits, eager and hipGraph steps give the
same bits; its distance from the oracle is printed, not asserted.

Run on the MI355X box:  python -m pytest tests/test_engine_narrow_widths_gpu.py -m gpu -x -q
"""
import numpy as np
import pytest

from ntransformer_amd import engine as E
from ntransformer_amd import gguf as G
from ntransformer_amd import ops
from oracle import oracle as O

pytestmark = pytest.mark.gpu
TOL = 1e-3          # tests/test_engine_gpu.py
CTX = 256
STEPS = 4
SEED = 20261019


def shape_of(name, hidden, inter, layers, heads, kv_heads):
    return G.LlamaShape(name, hidden, inter, layers, heads, kv_heads, 512, ctx=CTX, bos=256, eos=257)


SHAPES = {"w320": shape_of("w320", 320, 864, 2, 5, 1), "w384": shape_of("w384", 384, 896, 2, 6, 2),
          "w512": shape_of("w512", 512, 11008, 1, 4, 2), "w320x": shape_of("w320x", 320, 4128, 1, 5, 1)}
CASES = [("w320", "Q8_0"), ("w320", "Q4_0"), ("w384", "Q8_0"), ("w384", "Q4_0"), ("w512", "Q8_0"), ("w320x", "Q8_0"), ("w320x", "Q4_0")]
IDS = ["%s-%s" % c for c in CASES]
LENGTHS = (7, 17, 40)

_files, _oracle = {}, {}


def prompt_of(n, seed=0):
    r = np.random.Generator(np.random.Philox(key=[20261022, 1000 * seed + n]))
    return [256] + [int(t) for t in r.integers(0, 256, n - 1)]


@pytest.fixture(scope="module")
def model_file(tmp_path_factory):
    """(model, mix) -> path of its GGUF file, written once per module run"""
    root = tmp_path_factory.mktemp("narrow")

    def get(name, mix):
        if (name, mix) not in _files:
            path = str(root / ("%s_%s.gguf" % (name, mix.lower())))
            G.make_synthetic_llama(path, SHAPES[name], mix, seed=SEED)
            _files[(name, mix)] = path
        return _files[(name, mix)]
    return get


def oracle_run(path, key, prompt):
    """the oracle's logits of the prompt and of STEPS greedy steps behind it: (fed tokens, logits [1 + STEPS][V]); computed once, shared, read only"""
    k = key + (tuple(prompt),)
    if k not in _oracle:
        m = O.OracleModel(path, CTX)
        lg = [m.forward(prompt, 0)]
        fed, pos = [], len(prompt)
        for _ in range(STEPS):
            fed.append(m.argmax(lg[-1]))
            lg.append(m.forward([fed[-1]], pos))
            pos += 1
        out = np.stack(lg)
        out.setflags(write=False)
        _oracle[k] = (fed, out)
    return _oracle[k]


def engine_for(path, **opts):
    eng = E.Engine()
    for k, v in opts.items():
        eng.set_option(k, v)
    eng.load(path, CTX)
    return eng


def check_rows(got, want, what):
    assert got.shape == want.shape and np.isfinite(got).all(), what
    err = float(np.abs(got - want).max())
    print("%s: max |dlogit| = %.3g (bar %.0e)" % (what, err, TOL))
    assert err <= TOL, (what, err)
    top2 = np.sort(want, axis=1)[:, -2:]
    clear = (top2[:, 1] - top2[:, 0]) > 2 * TOL
    assert np.array_equal(got.argmax(1)[clear], want.argmax(1)[clear]), what


def repacked_bytes_expected(name, mix):
    """Q8_0 matrices whose width has a lane-major form (q8l_layout: every slice whole 256 columns), in GGUF bytes -- the repack is a permutation"""
    s = SHAPES[name]
    if mix != "Q8_0":
        return 0
    hd = s.hidden // s.heads
    mats = [(s.heads * hd, s.hidden), (s.kv_heads * hd, s.hidden), (s.kv_heads * hd, s.hidden), (s.hidden, s.heads * hd),
            (s.inter, s.hidden), (s.inter, s.hidden), (s.hidden, s.inter)]
    total = 0
    for rows, in_f in mats * s.layers + [(s.vocab, s.hidden)]:
        total += ops.q8l_bytes(rows, in_f)
    return total


# ------------------------------------------------------------------------------- prompt passes and decode steps against the oracle
@pytest.mark.parametrize("n_prompt,batched", [(7, 1), (7, 0), (17, 1), (40, 1)], ids=["p7", "p7-per-token", "p17", "p40"])
@pytest.mark.parametrize("name,mix", CASES, ids=IDS)
def test_prompt_pass_and_decode_steps_match_the_oracle(name, mix, n_prompt, batched, model_file):
    """A prompt of 7 / 17 / 40 tokens (17 and 40: several 16-token passes of the F32 GEMM, both forms of the FP16 one; 7 also with batched_prefill = 0,
    the per-token loop), then 4 teacher-forced steps through each of forward([t], pos) (the 1:1 launchers), decode_fused eager and decode_fused as a
    hipGraph -- every one of the 1 + 3 x 4 logits rows against the oracle."""
    path = model_file(name, mix)
    prompt = prompt_of(n_prompt)
    fed, want = oracle_run(path, (name, mix), prompt)
    eng = engine_for(path)
    if not batched: eng.set_option("batched_prefill", 0)
    assert eng.repacked_bytes() == repacked_bytes_expected(name, mix)          # which matrices took the lane-major form: none / all but w512's down
    if name == "w512": assert 0 < eng.repacked_bytes() < eng.weight_bytes()
    else: assert eng.repacked_bytes() == 0
    got = eng.forward(prompt, 0)
    check_rows(got[None, :], want[:1], "%s %s prompt of %d%s" % (name, mix, n_prompt, "" if batched else " (per token)"))
    for mode in ("launchers", "fused", "graph"):
        rows = []
        for i, t in enumerate(fed):                                            # (each mode rewrites the same cache rows with the same tokens)
            pos = n_prompt + i
            rows.append(eng.forward([t], pos) if mode == "launchers" else eng.decode_fused(t, pos, graph=mode == "graph"))
        check_rows(np.stack(rows), want[1:], "%s %s %s steps behind %d tokens" % (name, mix, mode, n_prompt))
    eng.close()


# ------------------------------------------------------------------------------- the repack changes no bit
@pytest.mark.parametrize("name,mix,kv", [c + ("f16",) for c in CASES] + [("w512", "Q8_0", "q8_0")], ids=IDS + ["w512-Q8_0-kv_q8_0"])
def test_repack_on_and_off_give_the_same_bits(name, mix, kv, model_file):
    """repack = 0 against the default on the 7-token prompt and 4 fused steps (eager, then the same steps as a hipGraph): identical logits bits -- in
    w512 across a layer whose down projection stays on GGUF blocks while every other matrix is read lane-major; in the other models nothing is
    repacked and the option must change nothing.  kv_cache = q8_0: the same, over the 8-bit cache (see the module docstring)."""
    path = model_file(name, mix)
    prompt = prompt_of(7)
    fed, want = oracle_run(path, (name, mix), prompt)
    outs = {}
    for level in (0, None):
        opts = {"kv_cache": kv}
        if level is not None: opts["repack"] = level
        eng = engine_for(path, **opts)
        lg = [eng.forward(prompt, 0)]
        for graph in (False, True):
            lg += [eng.decode_fused(t, 7 + i, graph=graph) for i, t in enumerate(fed)]
        outs[level] = np.stack(lg)
        if level == 0: assert eng.repacked_bytes() == 0
        else: assert eng.repacked_bytes() == repacked_bytes_expected(name, mix)
        eng.close()
    a, b = outs[0], outs[None]
    assert np.isfinite(b).all()
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), float(np.abs(a - b).max())
    assert np.array_equal(b[1:1 + STEPS].view(np.uint32), b[1 + STEPS:].view(np.uint32))      # eager = hipGraph
    err = float(np.abs(b[:1 + STEPS] - want).max())
    print("%s %s kv=%s: max |dlogit| against the oracle = %.3g" % (name, mix, kv, err))
    if kv == "f16": assert err <= TOL, err


# ------------------------------------------------------------------------------- batched decode
@pytest.mark.parametrize("mix", ["Q8_0", "Q4_0"])
def test_batched_decode_step_on_half_lane_rows(mix, model_file):
    """w320, sequences = 2: two different prompts (7 and 17 tokens) through seq_forward, then ONE decode_batch step -- both rows against their oracles"""
    path = model_file("w320", mix)
    prompts = [prompt_of(7, seed=1), prompt_of(17, seed=2)]
    runs = [oracle_run(path, ("w320", mix), p) for p in prompts]
    eng = engine_for(path, sequences=2)
    for s, (p, (fed, want)) in enumerate(zip(prompts, runs)):
        check_rows(eng.seq_forward(s, p, 0)[None, :], want[:1], "w320 %s slot %d prompt" % (mix, s))
    got, nxt = eng.decode_batch([0, 1], [runs[0][0][0], runs[1][0][0]], [len(prompts[0]), len(prompts[1])])
    want = np.stack([runs[0][1][1], runs[1][1][1]])
    check_rows(got, want, "w320 %s decode_batch" % mix)
    top2 = np.sort(want, axis=1)[:, -2:]
    clear = (top2[:, 1] - top2[:, 0]) > 2 * TOL
    assert np.array_equal(np.array(nxt)[clear], want.argmax(1)[clear])
    eng.close()
