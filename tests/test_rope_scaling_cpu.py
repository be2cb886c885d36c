"""RoPE frequency scaling on the host: the Llama-3.1 factors, the frequency table, what the GGUF readers see of both, the option grammar and the
load-time refusals of a bad rope_freqs.weight (decided before the device is touched) -- and the CPU test that makes tests/rope_ref.py a reference.

Not here, because it needs a loaded engine (a GPU): the refusal of the three options AFTER a load (tests/test_rope_scaling_engine_gpu.py)."""
import numpy as np
import pytest

from ntransformer_amd import engine as E
from ntransformer_amd import gguf as G
from ntransformer_amd import _lib
from oracle import oracle as O
from rope_ref import mixed_factors, plain_table, rope_ref, scaled_table

DTYPE, SHAPE, NODEVICE = -1, -2, -6
TINY64 = G.LlamaShape("tiny", 256, 512, 2, 4, 2, 512, ctx=256, bos=256, eos=257)          # head_dim 64


# ------------------------------------------------------------------------------------------------ the reference
@pytest.mark.parametrize("hd", [64, 128])
@pytest.mark.parametrize("interleaved", [False, True])
def test_rope_ref_with_the_plain_table_is_the_oracle_rope(hd, interleaved):
    nh, nkv, theta = 4, 2, 500000.0
    positions = [0, 1, 4095]
    r = np.random.default_rng(hd + interleaved)
    q = r.standard_normal(len(positions) * nh * hd).astype(np.float32)
    k = r.standard_normal(len(positions) * nkv * hd).astype(np.float32)
    want_q, want_k = O.rope(q, k, positions, nh, nkv, hd, theta, 1.0, interleaved)
    got_q, got_k = rope_ref(q, k, positions, nh, nkv, hd, plain_table(hd, theta), 1.0, interleaved)
    assert np.abs(got_q - want_q).max() <= 1e-6 and np.abs(got_k - want_k).max() <= 1e-6
    sq, sk = rope_ref(q, k, positions, nh, nkv, hd, scaled_table(hd, theta, mixed_factors(hd, 1)), 0.25, interleaved)
    assert np.abs(sq - want_q).max() > 0.1        # ... and a table is not ignored
    assert np.array_equal(sq[:nh * hd], q[:nh * hd])   # position 0 rotates nothing


# ------------------------------------------------------------------------------------------------ factors and table
def numpy_llama3(hd, theta, factor, low, high, orig):
    i = np.arange(hd // 2, dtype=np.float64)
    wavelen = 2 * np.pi * np.float64(theta) ** (2 * i / hd)
    s = (orig / wavelen - low) / (high - low)
    ramp = 1.0 / ((1.0 - s) / factor + s)
    return np.where(wavelen < orig / high, 1.0, np.where(wavelen > orig / low, factor, ramp))


@pytest.mark.parametrize("hd,theta,factor,low,high,orig", [(128, 500000.0, 8.0, 1.0, 4.0, 8192), (64, 10000.0, 8.0, 1.0, 4.0, 8192),
                                                           (64, 500000.0, 8.0, 1.0, 4.0, 64), (256, 1e6, 32.0, 1.0, 4.0, 8192),
                                                           (80, 10000.0, 4.0, 2.0, 8.0, 4096)])
def test_llama3_factors_against_the_numpy_formula(hd, theta, factor, low, high, orig):
    want = numpy_llama3(hd, theta, factor, low, high, orig)
    for got in (E.rope_llama3_factors(hd, theta, factor, low, high, orig), G.llama3_rope_factors(hd, theta, factor, low, high, orig)):
        assert got.dtype == np.float32 and got.shape == (hd // 2,)
        assert np.abs(got.astype(np.float64) - want).max() <= 1e-6 * factor
        assert (np.abs(got.astype(np.float64) - want) <= 1e-6 * want).all()
    assert np.array_equal(E.rope_llama3_factors(hd, theta, factor, low, high, orig), G.llama3_rope_factors(hd, theta, factor, low, high, orig))


@pytest.mark.parametrize("hd,theta,split,ramp", [(128, 500000.0, (29, 6, 29), [1.2075, 1.5534, 2.0263, 2.6945, 3.6843, 5.2573]), (64, 10000.0, (21, 4, 7), None)])
def test_llama3_default_factors_split_into_exact_ones_a_ramp_and_exact_eights(hd, theta, split, ramp):
    f = E.rope_llama3_factors(hd, theta)
    a, b, c = split
    assert a + b + c == hd // 2
    assert (f[:a] == np.float32(1.0)).all() and (f[a + b:] == np.float32(8.0)).all()
    mid = f[a:a + b]
    assert ((mid > 1.0) & (mid < 8.0)).all() and (np.diff(mid) > 0).all()
    if ramp is not None:
        assert np.abs(mid - np.array(ramp)).max() <= 5e-5, mid


def test_llama3_factors_refuse_bad_arguments():
    L = E._bind()
    out = np.zeros(64, np.float32)
    p = out.ctypes.data
    assert L.nt_rope_llama3_factors(128, 500000.0, 8.0, 1.0, 4.0, 8192, None) == -5
    for args in [(127, 5e5, 8.0, 1.0, 4.0, 8192), (0, 5e5, 8.0, 1.0, 4.0, 8192), (128, 0.0, 8.0, 1.0, 4.0, 8192), (128, 5e5, 0.0, 1.0, 4.0, 8192),
                 (128, 5e5, 8.0, 4.0, 4.0, 8192), (128, 5e5, 8.0, 1.0, 4.0, 0), (128, 5e5, float("nan"), 1.0, 4.0, 8192)]:
        assert L.nt_rope_llama3_factors(*args, p) == SHAPE, args


@pytest.mark.parametrize("hd,theta", [(64, 10000.0), (128, 500000.0), (256, 1e6), (80, 500000.0)])
def test_build_table(hd, theta):
    """NULL factors: the table the engine has always uploaded, 1.0f / powf(theta, (2.0f * i) / head_dim), bit for bit.  The numpy statement of that line
    takes the power in float64 and rounds once (= a correctly rounded powf, kv_ops.pair_freqs' expression): numpy's float32 power, which
    test_attention_decode_fused_equals_rope_store_attend writes, is a vector routine that differs from libm's powf in the last bit of some entries (7 of
    32 at head_dim 64 where this was written, up to 2 ulp after the reciprocal), so it can only be held to a few ulp."""
    plain = E.rope_build_table(hd, theta)
    want = plain_table(hd, theta)
    assert np.array_equal(plain.view(np.uint32), want.view(np.uint32))                     # NULL factors: today's table, bit for bit
    from ntransformer_amd import kv_ops as KO
    assert np.array_equal(plain.view(np.uint32), KO.pair_freqs(hd, theta).view(np.uint32))
    i = np.arange(hd // 2, dtype=np.float32)
    np32 = (np.float32(1.0) / np.power(np.float32(theta), (np.float32(2.0) * i) / np.float32(hd))).astype(np.float32)
    assert np.abs(plain.view(np.int32) - np32.view(np.int32)).max() <= 4        # (a power a few ulp off, then the reciprocal's rounding)
    f = mixed_factors(hd, 3)
    assert np.array_equal(E.rope_build_table(hd, theta, f).view(np.uint32), (want / f).astype(np.float32).view(np.uint32))   # ... divided in F32
    ones = np.ones(hd // 2, np.float32)
    assert np.array_equal(E.rope_build_table(hd, theta, ones), plain)
    assert E._bind().nt_rope_build_table(63, 1e4, None, plain.ctypes.data) == SHAPE


# ------------------------------------------------------------------------------------------------ files
def write(tmp_path, name, **kw):
    p = str(tmp_path / name)
    G.make_synthetic_llama(p, TINY64, "Q8_0", seed=5, **kw)
    return p


def test_a_file_written_with_default_arguments_has_no_new_key_or_tensor(tmp_path):
    import os
    p = write(tmp_path, "plain.gguf")
    f = G.read_gguf(p)
    assert not [k for k in f.meta if "rope.scal" in k or "scale_linear" in k] and "rope_freqs.weight" not in f.tensors
    golden = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tiny_q8_0.gguf")
    g = G.read_gguf(golden)
    assert sorted(g.meta) == sorted(f.meta) and sorted(g.tensors) == sorted(f.tensors)    # the key / tensor set of the committed fixture
    d = E.gguf_describe(p)
    assert (d["rope_scaling_type"], d["rope_freq_scale"], d["rope_factors"], d["rope_orig_ctx"]) == ("none", 1.0, 0, 0)
    assert d["rope_theta"] == 500000.0


def test_describe_and_the_python_reader_agree_on_factors_and_scaling(tmp_path):
    fac = G.llama3_rope_factors(64, 500000.0, orig_ctx=64)
    p = write(tmp_path, "l3.gguf", rope_freqs=fac, rope_scaling={"original_context_length": 8192})
    d, f = E.gguf_describe(p), G.read_gguf(p)
    assert (d["rope_scaling_type"], d["rope_freq_scale"], d["rope_factors"], d["rope_orig_ctx"]) == ("none", 1.0, 32, 8192)
    t = [x for x in d["tensors"] if x["name"] == "rope_freqs.weight"][0]
    ti = f.tensors["rope_freqs.weight"]
    assert (t["dims"], t["ggml_type"], t["offset"], t["nbytes"]) == ([32], G.GGML_F32, ti.offset, ti.nbytes) and ti.nbytes == 128
    assert np.array_equal(f.f32("rope_freqs.weight"), fac)
    assert f.meta["llama.rope.scaling.original_context_length"] == 8192

    p = write(tmp_path, "lin.gguf", rope_scaling={"type": "linear", "factor": 4.0})
    d = E.gguf_describe(p)
    assert (d["rope_scaling_type"], d["rope_freq_scale"], d["rope_factors"], d["rope_orig_ctx"]) == ("linear", 0.25, 0, 0)
    assert G.read_gguf(p).meta["llama.rope.scaling.type"] == b"linear"

    d = E.gguf_describe(write(tmp_path, "legacy.gguf", rope_scaling={"scale_linear": 2.0}))
    assert (d["rope_scaling_type"], d["rope_freq_scale"]) == ("linear", 0.5)

    d = E.gguf_describe(write(tmp_path, "yarn.gguf", rope_scaling={"type": "yarn", "factor": 4.0, "original_context_length": 4096}))
    assert (d["rope_scaling_type"], d["rope_freq_scale"], d["rope_factors"], d["rope_orig_ctx"]) == ("yarn", 1.0, 0, 4096)   # named, not applied


# ------------------------------------------------------------------------------------------------ options (an engine that never loads touches no device)
@pytest.mark.parametrize("text", ["file", "none", "linear:4", "linear:0.5", "llama3:8,1,4,8192", "llama3:8.0,1.0,4.0,64", "llama3:32,1,4,8192"])
def test_good_rope_scaling_strings(text):
    e = E.Engine()
    e.set_option("rope_scaling", text)
    e.set_option("rope_freq_base", 10000.0)
    e.set_option("rope_freq_scale", "0.5")
    e.close()


def test_set_option_sends_real_numbers_to_the_float_options_and_integers_to_the_rest():
    e = E.Engine()
    for v in (0.25, np.float32(0.25), np.float64(0.25), 2, np.int32(2)):      # (as int(v) 0.25 would arrive as "0" and be refused)
        e.set_option("rope_freq_scale", v)
        e.set_option("rope_freq_base", v)
    for v in (1, 1.0, True, np.int64(1), np.float32(1.0)):                    # integer options keep receiving "1", never "1.0"
        e.set_option("context_shift", v)
        e.set_option("batch_kv_q8", v)
    e.set_option("sequences", 4.0)
    e.close()


@pytest.mark.parametrize("key,text", [("rope_scaling", t) for t in ["", "linear", "linear:", "linear:0", "linear:-2", "linear:4x", "linear:4,2", "linear:nan",
                                                                   "linear:inf", "llama3", "llama3:8,1,4", "llama3:8,1,4,8192,1", "llama3:8,1,4,0",
                                                                   "llama3:8,4,4,8192", "llama3:8,1,4,81.5", "llama3:0,1,4,8192", "llama3:8,,4,8192",
                                                                   "yarn", "yarn:4", "File", "1"]]
                         + [(k, t) for k in ("rope_freq_base", "rope_freq_scale") for t in ["", "0", "-1", "abc", "1e4x", "nan", "inf"]])
def test_malformed_rope_options_are_refused_with_a_message(key, text):
    e = E.Engine()
    with pytest.raises(_lib.NtkError) as ei:
        e.set_option(key, text)
    assert ei.value.status == SHAPE and key in str(ei.value)
    e.set_option("rope_scaling", "none")      # the engine stays usable
    e.close()


# ------------------------------------------------------------------------------------------------ refusals at load (decided on the host, before the device)
@pytest.mark.parametrize("name,freqs,status", [("short", np.ones(31, np.float32), SHAPE), ("long", np.ones(64, np.float32), SHAPE),
                                               ("f16", np.ones(32, np.float16), DTYPE),
                                               ("zero", np.r_[np.ones(31, np.float32), np.float32(0)], SHAPE),
                                               ("negative", np.r_[np.float32(-1), np.ones(31, np.float32)], SHAPE),
                                               ("nan", np.r_[np.ones(16, np.float32), np.float32(np.nan), np.ones(15, np.float32)], SHAPE),
                                               ("inf", np.r_[np.ones(31, np.float32), np.float32(np.inf)], SHAPE)])
def test_a_bad_rope_freqs_tensor_refuses_the_load_naming_the_tensor(tmp_path, name, freqs, status):
    p = write(tmp_path, name + ".gguf", rope_freqs=freqs)
    e = E.Engine()
    with pytest.raises(_lib.NtkError) as ei:
        e.load(p, 64)
    assert ei.value.status == status and "rope_freqs.weight" in str(ei.value)
    e.close()


def test_factors_at_a_head_size_the_decode_attention_has_no_table_for_are_refused(tmp_path):
    """head_dim 80: ntk_attention_decode_fused's generic form derives the frequency from theta and takes no table, so factors -- from the file or from
    rope_scaling=llama3 -- are refused at load (on the host, before the device) rather than applied in the prompt pass and ignored in decode."""
    hd80 = G.LlamaShape("hd80", 320, 640, 1, 4, 2, 512, ctx=64, bos=256, eos=257)
    with_factors = str(tmp_path / "hd80_factors.gguf")
    G.make_synthetic_llama(with_factors, hd80, "Q8_0", seed=5, rope_freqs=G.llama3_rope_factors(80, 500000.0, orig_ctx=64))
    plain = str(tmp_path / "hd80.gguf")
    G.make_synthetic_llama(plain, hd80, "Q8_0", seed=5)
    for path, opts in ((with_factors, {}), (with_factors, {"rope_scaling": "linear:2"}), (plain, {"rope_scaling": "llama3:8,1,4,64"})):
        e = E.Engine()
        for k, v in opts.items():
            e.set_option(k, v)
        with pytest.raises(_lib.NtkError) as ei:
            e.load(path, 64)
        assert ei.value.status == SHAPE and "head_dim" in str(ei.value) and "80" in str(ei.value), (path, opts)
        e.close()
