"""Python view of the engine C API (include/ntransformer.h): the reference's nt_engine_* surface plus the
extensions the tests and bench.py use.  Mirrors reference src/inference/engine.h (Engine::load / generate / Stats)."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import List, Optional, Sequence

import numpy as np

from . import _lib
from ._lib import check


class GenParams(C.Structure):
    _fields_ = [("max_tokens", C.c_int), ("temperature", C.c_float), ("top_k", C.c_int), ("top_p", C.c_float),
                ("repeat_penalty", C.c_float), ("repeat_window", C.c_int), ("seed", C.c_uint64), ("stop_at_eos", C.c_int)]


class CStats(C.Structure):
    _fields_ = [("prompt_tokens", C.c_int), ("gen_tokens", C.c_int), ("prefill_ms", C.c_float), ("decode_ms", C.c_float),
                ("decode_tok_s", C.c_float)]


class SynthSpec(C.Structure):
    _fields_ = [("hidden", C.c_int), ("inter", C.c_int), ("layers", C.c_int), ("heads", C.c_int), ("kv_heads", C.c_int),
                ("vocab", C.c_int), ("ctx", C.c_int), ("eps", C.c_float), ("theta", C.c_float), ("bos", C.c_int),
                ("eos", C.c_int), ("mix", C.c_char_p), ("seed", C.c_uint64)]


PRESETS = {
    "tiny": dict(hidden=256, inter=512, layers=2, heads=4, kv_heads=2, vocab=512, ctx=256, bos=256, eos=257),
    "small": dict(hidden=1024, inter=2048, layers=4, heads=8, kv_heads=2, vocab=2048, ctx=2048, bos=256, eos=257),
    "8b": dict(hidden=4096, inter=14336, layers=32, heads=32, kv_heads=8, vocab=128256, ctx=131072, bos=128000, eos=128009),
    "70b": dict(hidden=8192, inter=28672, layers=80, heads=64, kv_heads=8, vocab=128256, ctx=131072, bos=128000, eos=128009),
    # Qwen2.5-7B's geometry with a tied head; the flavour rides in front of the mix (csrc/engine/synth.h: synth_flavour): three F32 bias vectors per layer
    "qwen2.5-7b": dict(hidden=3584, inter=18944, layers=28, heads=28, kv_heads=4, vocab=152064, ctx=32768, bos=151643, eos=151645, eps=1e-6, theta=1e6,
                       flavour="qwen2-tied"),
    "qwen2.5-7b-nobias": dict(hidden=3584, inter=18944, layers=28, heads=28, kv_heads=4, vocab=152064, ctx=32768, bos=151643, eos=151645, eps=1e-6, theta=1e6,
                              flavour="tied"),   # its bias-free twin (the A/B of tools/prefill_bench.py --ab-qkv-bias)
    # Qwen3-8B (untied head) and Qwen3-4B (32 heads of 128 over a hidden size of 2560: heads x head_dim = 4096, tied head): two F32 norm vectors of
    # head_dim values per layer; -nonorm: the same seeded matrices without them (the A/B of tools/prefill_bench.py --ab-qk-norm)
    "qwen3-8b": dict(hidden=4096, inter=12288, layers=36, heads=32, kv_heads=8, vocab=151936, ctx=40960, bos=151643, eos=151645, eps=1e-6, theta=1e6,
                     flavour="qwen3-hd128"),
    "qwen3-8b-nonorm": dict(hidden=4096, inter=12288, layers=36, heads=32, kv_heads=8, vocab=151936, ctx=40960, bos=151643, eos=151645, eps=1e-6, theta=1e6,
                            flavour="hd128"),
    "qwen3-4b": dict(hidden=2560, inter=9728, layers=36, heads=32, kv_heads=8, vocab=151936, ctx=40960, bos=151643, eos=151645, eps=1e-6, theta=1e6,
                     flavour="qwen3-hd128-tied"),
    "qwen3-4b-nonorm": dict(hidden=2560, inter=9728, layers=36, heads=32, kv_heads=8, vocab=151936, ctx=40960, bos=151643, eos=151645, eps=1e-6, theta=1e6,
                            flavour="hd128-tied"),
    # mixture-of-experts: Qwen3-30B-A3B (128 experts of width 768, 8 per token, every layer) and Mixtral 8x7B under `llama` (8 experts of width 14336, 2 per token)
    "qwen3-30b-a3b": dict(hidden=2048, inter=6144, layers=48, heads=32, kv_heads=4, vocab=151936, ctx=40960, bos=151643, eos=151645, eps=1e-6, theta=1e6,
                          flavour="qwen3-hd128-moe128x8-i768"),
    "mixtral-8x7b": dict(hidden=4096, inter=14336, layers=32, heads=32, kv_heads=8, vocab=32000, ctx=32768, bos=1, eos=2, eps=1e-5, theta=1e6,
                         flavour="moe8x2"),
}


def synth_spec(preset: str, mix: str = "Q8_0", seed: int = 20260925, layers: Optional[int] = None) -> SynthSpec:
    p = dict(PRESETS[preset])
    if layers is not None:
        p["layers"] = layers
    if p.get("flavour"):
        mix = p["flavour"] + ":" + mix
    return SynthSpec(p["hidden"], p["inter"], p["layers"], p["heads"], p["kv_heads"], p["vocab"], p["ctx"], p.get("eps", 1e-5), p.get("theta", 500000.0),
                     p["bos"], p["eos"], mix.encode(), seed)


def _bind():
    L = _lib.lib()
    if getattr(L, "_engine_bound", False):
        return L
    vp, i, f = C.c_void_p, C.c_int, C.c_float
    L.nt_engine_create.restype = vp
    L.nt_engine_destroy.argtypes = [vp]
    L.nt_engine_load.argtypes = [vp, C.c_char_p]
    L.nt_engine_load_ex.argtypes = [vp, C.c_char_p, i]
    L.nt_engine_load_synthetic.argtypes = [vp, C.POINTER(SynthSpec), i]
    L.nt_engine_set_option.argtypes = [vp, C.c_char_p, C.c_char_p]
    L.nt_engine_last_error.argtypes = [vp]
    L.nt_engine_last_error.restype = C.c_char_p
    L.nt_engine_generate.argtypes = [vp, C.c_char_p, i, f, i, f]
    L.nt_engine_generate.restype = vp
    L.nt_free.argtypes = [vp]
    for n in ("vocab_size", "n_layers", "hidden_size", "max_context"):
        getattr(L, "nt_engine_" + n).argtypes = [vp]
    L.nt_gen_params_default.argtypes = [C.POINTER(GenParams)]
    L.nt_engine_generate_tokens.argtypes = [vp, C.POINTER(i), i, C.POINTER(GenParams), C.POINTER(i), i]
    L.nt_engine_last_stats.argtypes = [vp, C.POINTER(CStats)]
    L.nt_engine_forward.argtypes = [vp, C.POINTER(i), i, i, vp]
    L.nt_engine_decode_fused.argtypes = [vp, i, i, i, vp]
    L.nt_engine_seq_forward.argtypes = [vp, i, C.POINTER(i), i, i, vp]
    L.nt_engine_decode_batch.argtypes = [vp, C.POINTER(i), C.POINTER(i), C.POINTER(i), i, vp, vp]
    L.nt_engine_forward_batch.argtypes = [vp, C.POINTER(i), C.POINTER(i), C.POINTER(i), C.POINTER(i), i, vp, vp]
    L.nt_forward_batch_validate.argtypes = [C.POINTER(i), C.POINTER(i), C.POINTER(i), i, i, i]
    L.nt_engine_generate_batch.argtypes = [vp, C.POINTER(C.POINTER(i)), C.POINTER(i), i, C.POINTER(GenParams), C.POINTER(i), i, C.POINTER(i)]
    L.nt_engine_decode_batch_sample.argtypes = [vp, C.POINTER(i), C.POINTER(i), C.POINTER(i), i, C.POINTER(GenParams), C.POINTER(C.POINTER(i)), C.POINTER(i),
                                                C.POINTER(f), vp, vp]
    L.nt_engine_generate_batch_ex.argtypes = [vp, C.POINTER(C.POINTER(i)), C.POINTER(i), i, C.POINTER(GenParams), C.POINTER(i), i, C.POINTER(i)]
    L.nt_sampler_draw_nth.argtypes = [vp, i, C.POINTER(GenParams), C.POINTER(i), i, i, C.POINTER(i)]
    L.nt_sampler_uniforms.argtypes = [C.c_uint64, i, vp]
    L.nt_batch_validate.argtypes = [C.POINTER(i), C.POINTER(i), C.POINTER(i), i, i, i, i]
    L.nt_engine_debug_kv_read_slot.argtypes = [vp, i, i, i, i, vp, vp]
    L.nt_engine_debug_kv_write_slot.argtypes = [vp, i, i, i, i, vp, vp]
    L.nt_engine_score_tokens.argtypes = [vp, C.POINTER(i), C.POINTER(i), i, i, vp, vp]
    L.nt_engine_tokenize.argtypes = [vp, C.c_char_p, i, C.POINTER(i), i]
    L.nt_engine_detokenize.argtypes = [vp, C.POINTER(i), i, C.c_char_p, i]
    L.nt_engine_bytes_per_token.argtypes = [vp, i]
    L.nt_engine_bytes_per_token.restype = C.c_uint64
    L.nt_engine_weight_bytes.argtypes = [vp]
    L.nt_engine_weight_bytes.restype = C.c_uint64
    L.nt_engine_resident_weight_bytes.argtypes = [vp]
    L.nt_engine_resident_weight_bytes.restype = C.c_uint64
    L.nt_engine_decode_path.argtypes = [vp]
    L.nt_engine_decode_path.restype = C.c_char_p
    L.nt_synth_write_gguf.argtypes = [C.c_char_p, C.POINTER(SynthSpec), i]
    L.nt_synth_tensor.argtypes = [C.POINTER(SynthSpec), C.c_char_p, vp, C.c_size_t, i]
    L.nt_synth_tensor.restype = C.c_int64
    L.nt_engine_decode_greedy_steps.argtypes = [vp, i, i, i, C.POINTER(i)]
    L.nt_engine_profile_token.argtypes = [vp, i, i, i, C.POINTER(f), C.POINTER(i)]
    L.nt_engine_tp_configure.argtypes = [vp, i, i]
    L.nt_engine_tp_export.argtypes = [vp, vp, C.POINTER(vp)]
    L.nt_engine_tp_connect.argtypes = [vp, vp, C.POINTER(vp)]
    L.nt_engine_tp_error.argtypes = [vp]
    L.nt_engine_tp_error.restype = C.c_uint
    L.nt_tp_slice_columns.argtypes = [vp, vp, i, C.c_int64, C.c_int64, i, i]
    L.nt_engine_debug_run_layers.argtypes = [vp, vp, i, i, i, i, i, vp]
    L.nt_engine_debug_kv_read.argtypes = [vp, i, i, i, vp, vp]
    L.nt_engine_debug_kv_write.argtypes = [vp, i, i, i, vp, vp]
    L.nt_engine_debug_kv_read_q8.argtypes = [vp, i, i, i, vp, vp]
    L.nt_engine_debug_kv_write_q8.argtypes = [vp, i, i, i, vp, vp]
    L.nt_engine_debug_kv_read_q8_slot.argtypes = [vp, i, i, i, i, vp, vp]
    L.nt_engine_debug_kv_write_q8_slot.argtypes = [vp, i, i, i, i, vp, vp]
    L.nt_engine_debug_kv_inputs_capture.argtypes = [vp, i]
    L.nt_engine_debug_kv_inputs_read.argtypes = [vp, i, vp, vp]
    L.nt_engine_kv_cache_bytes.argtypes = [vp]
    L.nt_engine_kv_shift.argtypes = [vp, i, i, i, i]
    L.nt_engine_kv_copy.argtypes = [vp, i, i, i, i]
    L.nt_kv_shift_validate.argtypes = [i, i, i, i, i, i]
    L.nt_kv_copy_validate.argtypes = [i, i, i, i, i, i]
    L.nt_context_shift_discard.argtypes = [i, i]
    L.nt_engine_kv_cache_bytes.restype = C.c_uint64
    L.nt_rope_llama3_factors.argtypes = [i, f, f, f, f, i, vp]
    L.nt_rope_build_table.argtypes = [i, f, vp, vp]
    L.nt_engine_rope_info.argtypes = [vp, C.c_char_p, i]
    L.nt_gguf_describe.argtypes = [C.c_char_p, C.c_char_p, i]
    L.nt_engine_qkv_bias.argtypes = [vp]
    L.nt_engine_qk_norm.argtypes = [vp]
    L.nt_engine_moe.argtypes = [vp, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L._engine_bound = True
    return L


@dataclass
class Stats:
    prompt_tokens: int
    gen_tokens: int
    prefill_ms: float
    decode_ms: float
    decode_tok_s: float


class Engine:
    def __init__(self):
        self.L = _bind()
        self.h = self.L.nt_engine_create()
        if not self.h:
            raise MemoryError("nt_engine_create")

    def close(self):
        if self.h:
            self.L.nt_engine_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, st, what):
        if st != 0:
            raise _lib.NtkError(st, "%s: %s" % (what, (self.L.nt_engine_last_error(self.h) or b"").decode()))

    def load(self, path: str, max_context: int = 4096):
        self._check(self.L.nt_engine_load_ex(self.h, path.encode(), max_context), "load")

    def load_synthetic(self, spec: SynthSpec, max_context: int = 4096):
        self._spec = spec
        self._check(self.L.nt_engine_load_synthetic(self.h, C.byref(spec), max_context), "load_synthetic")

    # ---- tensor parallelism (include/ntransformer.h: nt_engine_tp_*) ----
    def tp_configure(self, rank: int, world: int) -> None:
        """before load(): this engine keeps slice `rank` of `world` of every projection"""
        self._check(self.L.nt_engine_tp_configure(self.h, rank, world), "tp_configure")

    def tp_export(self):
        """after load(): (64-byte hipIpc handle, raw device pointer) of this rank's communication buffer"""
        handle = C.create_string_buffer(64)
        raw = C.c_void_p()
        self._check(self.L.nt_engine_tp_export(self.h, handle, C.byref(raw)), "tp_export")
        return handle.raw, raw.value

    def tp_connect(self, handles: Optional[Sequence[bytes]] = None, raws: Optional[Sequence[int]] = None) -> None:
        """every rank, in rank order: the peers' handles (other processes) or raw pointers (ranks sharing this process)"""
        if raws is not None:
            arr = (C.c_void_p * len(raws))(*raws)
            self._check(self.L.nt_engine_tp_connect(self.h, None, arr), "tp_connect")
        else:
            blob = C.create_string_buffer(b"".join(handles), 64 * len(handles))
            self._check(self.L.nt_engine_tp_connect(self.h, blob, None), "tp_connect")

    def tp_error(self) -> int:
        return int(self.L.nt_engine_tp_error(self.h))

    def set_option(self, key: str, value) -> None:
        # ("kv_cache" takes "f16" / "q8_0", "rope_scaling" its own strings; "rope_freq_base" / "rope_freq_scale" a float)
        if isinstance(value, str):
            text = value
        elif key in ("rope_freq_base", "rope_freq_scale"):
            text = repr(float(value))          # (any real number type: float, numpy.float32, int)
        else:
            text = str(int(value))
        self._check(self.L.nt_engine_set_option(self.h, key.encode(), text.encode()), "set_option " + key)

    def rope_info(self) -> dict:
        """The rotation the loaded model runs with (nt_engine_rope_info): rope_theta, rope_scaling_type ("none", "linear", "llama3", or the file's
        type where it is not applied), rope_freq_scale, rope_factors (how many per-pair divisors the frequency table carries: 0 or head_dim / 2),
        rope_orig_ctx."""
        import json
        buf = C.create_string_buffer(512)
        n = self.L.nt_engine_rope_info(self.h, buf, len(buf))
        if n < 0:
            self._check(n, "rope_info")
        return json.loads(buf.value.decode())

    @property
    def rope_scaling_type(self) -> str: return self.rope_info()["rope_scaling_type"]
    @property
    def rope_freq_scale(self) -> float: return float(self.rope_info()["rope_freq_scale"])
    @property
    def rope_factors(self) -> int: return int(self.rope_info()["rope_factors"])
    @property
    def rope_orig_ctx(self) -> int: return int(self.rope_info()["rope_orig_ctx"])

    @property
    def qkv_bias(self) -> int:
        """in how many layers the loaded model adds a Q | K | V projection bias (nt_engine_qkv_bias): 0 for a Llama model"""
        return int(self.L.nt_engine_qkv_bias(self.h))

    @property
    def qk_norm(self) -> int:
        """in how many layers the loaded model normalises every head of Q and K (nt_engine_qk_norm): 0 for a Llama or Qwen2 model"""
        return int(self.L.nt_engine_qk_norm(self.h))

    def moe(self) -> int:
        """how many layers of the loaded model are mixture-of-experts layers (nt_engine_moe): 0 for a dense model; moe_experts() gives (E, K)"""
        return int(self.L.nt_engine_moe(self.h, None, None))

    def moe_experts(self):
        """(expert count E, experts per token K) of the loaded model; (0, 0) for a dense model"""
        e, k = C.c_int(0), C.c_int(0)
        self.L.nt_engine_moe(self.h, C.byref(e), C.byref(k))
        return int(e.value), int(k.value)

    @property
    def vocab_size(self): return self.L.nt_engine_vocab_size(self.h)
    @property
    def n_layers(self): return self.L.nt_engine_n_layers(self.h)
    @property
    def hidden_size(self): return self.L.nt_engine_hidden_size(self.h)

    def forward(self, tokens: Sequence[int], start_pos: int) -> np.ndarray:
        out = np.empty(self.vocab_size, np.float32)
        arr = (C.c_int * len(tokens))(*[int(t) for t in tokens])
        self._check(self.L.nt_engine_forward(self.h, arr, len(tokens), start_pos, out.ctypes.data_as(C.c_void_p)), "forward")
        return out

    def decode_fused(self, token: int, pos: int, graph: bool = False) -> np.ndarray:
        out = np.empty(self.vocab_size, np.float32)
        self._check(self.L.nt_engine_decode_fused(self.h, int(token), pos, int(graph), out.ctypes.data_as(C.c_void_p)), "decode_fused")
        return out

    # ---- sequence slots ("sequences" option; include/ntransformer.h) ----
    def seq_forward(self, slot: int, tokens: Sequence[int], start_pos: int) -> np.ndarray:
        """forward() into the KV cache of sequence slot `slot`"""
        out = np.empty(self.vocab_size, np.float32)
        arr = (C.c_int * len(tokens))(*[int(t) for t in tokens])
        self._check(self.L.nt_engine_seq_forward(self.h, int(slot), arr, len(tokens), start_pos, out.ctypes.data_as(C.c_void_p)), "seq_forward")
        return out

    def decode_batch(self, slots: Sequence[int], tokens: Sequence[int], positions: Sequence[int], logits: bool = True):
        """One decode step of len(slots) sequences in one pass over the weights: (logits [n, vocab] or None, greedy tokens [n])."""
        n = len(slots)
        ia = lambda xs: (C.c_int * max(len(xs), 1))(*[int(x) for x in xs])
        out = np.empty((n, self.vocab_size), np.float32) if logits else None
        nxt = (C.c_int * max(n, 1))()
        self._check(self.L.nt_engine_decode_batch(self.h, ia(slots), ia(tokens), ia(positions), n,
                                                  out.ctypes.data_as(C.c_void_p) if logits else None, C.cast(nxt, C.c_void_p)), "decode_batch")
        return out, list(nxt[:n])

    def forward_batch(self, slots: Sequence[int], token_lists: Sequence[Sequence[int]], start_positions: Sequence[int], logits: bool = True):
        """The packed prompt pass: token_lists[i] goes into slot slots[i] from position start_positions[i], all in one pass over the weights:
        (logits behind each list's last token [n, vocab] or None, their greedy tokens [n])."""
        n = len(slots)
        ia = lambda xs: (C.c_int * max(len(xs), 1))(*[int(x) for x in xs])
        out = np.empty((n, self.vocab_size), np.float32) if logits else None
        nxt = (C.c_int * max(n, 1))()
        flat = [t for q in token_lists for t in q]
        self._check(self.L.nt_engine_forward_batch(self.h, ia(slots), ia(flat), ia([len(q) for q in token_lists]), ia(start_positions), n,
                                                   out.ctypes.data_as(C.c_void_p) if logits else None, C.cast(nxt, C.c_void_p)), "forward_batch")
        return out, list(nxt[:n])

    def generate_batch(self, prompts: Sequence[Sequence[int]], max_tokens: int, stop_at_eos: bool = True, temperature: float = 0.0,
                       repeat_penalty: float = 1.0) -> List[List[int]]:
        """Greedy generation of len(prompts) sequences in lockstep (prompt i in slot i): the generated ids per sequence."""
        n = len(prompts)
        p = GenParams(max_tokens, temperature, 40, 0.9, repeat_penalty, 64, 42, int(stop_at_eos))
        rows = [(C.c_int * max(len(q), 1))(*[int(t) for t in q]) for q in prompts]
        ptrs = (C.POINTER(C.c_int) * max(n, 1))(*[C.cast(r, C.POINTER(C.c_int)) for r in rows])
        lens = (C.c_int * max(n, 1))(*[len(q) for q in prompts])
        stride = max(max_tokens, 1)
        out = (C.c_int * (max(n, 1) * stride))()
        counts = (C.c_int * max(n, 1))()
        st = self.L.nt_engine_generate_batch(self.h, ptrs, lens, n, C.byref(p), out, stride, counts)
        if st < 0:
            self._check(st, "generate_batch")
        return [list(out[i * stride: i * stride + counts[i]]) for i in range(n)]

    def decode_batch_sample(self, slots: Sequence[int], tokens: Sequence[int], positions: Sequence[int], params: Sequence[GenParams],
                            recent: Sequence[Sequence[int]], r: Sequence[float], logits: bool = True):
        """decode_batch with every row sampled on the device: row i by params[i] over the window recent[i] (the caller cuts it: the last repeat_window
        tokens) with the uniform draw r[i] (ignored where temperature <= 0).  (logits [n, vocab] BEFORE any penalty or None, tokens [n])."""
        n = len(slots)
        ia = lambda xs: (C.c_int * max(len(xs), 1))(*[int(x) for x in xs])
        pa = (GenParams * max(n, 1))(*params)
        wins = [ia(w) for w in recent]
        ptrs = (C.POINTER(C.c_int) * max(n, 1))(*[C.cast(w, C.POINTER(C.c_int)) for w in wins])
        ra = (C.c_float * max(n, 1))(*[float(x) for x in r])
        out = np.empty((n, self.vocab_size), np.float32) if logits else None
        nxt = (C.c_int * max(n, 1))()
        self._check(self.L.nt_engine_decode_batch_sample(self.h, ia(slots), ia(tokens), ia(positions), n, pa, ptrs, ia([len(w) for w in recent]), ra,
                                                         out.ctypes.data_as(C.c_void_p) if logits else None, C.cast(nxt, C.c_void_p)), "decode_batch_sample")
        return out, list(nxt[:n])

    def generate_batch_ex(self, prompts: Sequence[Sequence[int]], params: Sequence[GenParams]) -> List[List[int]]:
        """Generation of len(prompts) sequences in lockstep (prompt i in slot i), sequence i sampled with params[i] -- its own temperature, top_k, top_p,
        repeat penalty and window, seed, max_tokens and stop_at_eos: the generated ids per sequence."""
        n = len(prompts)
        pa = (GenParams * max(n, 1))(*params)
        rows = [(C.c_int * max(len(q), 1))(*[int(t) for t in q]) for q in prompts]
        ptrs = (C.POINTER(C.c_int) * max(n, 1))(*[C.cast(r, C.POINTER(C.c_int)) for r in rows])
        lens = (C.c_int * max(n, 1))(*[len(q) for q in prompts])
        stride = max([int(p.max_tokens) for p in params] + [1])
        out = (C.c_int * (max(n, 1) * stride))()
        counts = (C.c_int * max(n, 1))()
        st = self.L.nt_engine_generate_batch_ex(self.h, ptrs, lens, n, pa, out, stride, counts)
        if st < 0:
            self._check(st, "generate_batch_ex")
        return [list(out[i * stride: i * stride + counts[i]]) for i in range(n)]

    def kv_read_slot(self, slot: int, layer: int, pos0: int, n: int, row_halves: int):
        """kv_read of sequence slot `slot`"""
        k = np.empty((n, row_halves), np.uint16)
        v = np.empty((n, row_halves), np.uint16)
        self._check(self.L.nt_engine_debug_kv_read_slot(self.h, int(slot), layer, pos0, n, k.ctypes.data_as(C.c_void_p), v.ctypes.data_as(C.c_void_p)),
                    "kv_read_slot")
        return k, v

    def kv_write_slot(self, slot: int, layer: int, pos0: int, k: np.ndarray, v: np.ndarray) -> None:
        """kv_write into sequence slot `slot`"""
        k = np.ascontiguousarray(k, dtype=np.uint16)
        v = np.ascontiguousarray(v, dtype=np.uint16)
        self._check(self.L.nt_engine_debug_kv_write_slot(self.h, int(slot), layer, pos0, k.shape[0], k.ctypes.data_as(C.c_void_p),
                                                         v.ctypes.data_as(C.c_void_p)), "kv_write_slot")

    # ---- KV cache sequence operations (include/ntransformer.h: nt_engine_kv_shift / nt_engine_kv_copy) ----
    def kv_shift(self, slot: int, keep: int, discard: int, n_past: int) -> int:
        """Context shift of sequence slot `slot`: positions [keep, keep + discard) go, rows [keep + discard, n_past) move down to keep (K re-rotated, V as
        it is).  Returns the new n_past - discard."""
        n = self.L.nt_engine_kv_shift(self.h, int(slot), int(keep), int(discard), int(n_past))
        if n < 0:
            self._check(n, "kv_shift")
        return int(n)

    def kv_copy(self, src_slot: int, dst_slot: int, pos0: int, n: int) -> int:
        """Rows [pos0, pos0 + n) of every layer and both sides from slot to slot at the same positions, no rotation.  Returns n."""
        got = self.L.nt_engine_kv_copy(self.h, int(src_slot), int(dst_slot), int(pos0), int(n))
        if got < 0:
            self._check(got, "kv_copy")
        return int(got)

    @property
    def max_context(self): return self.L.nt_engine_max_context(self.h)

    def score(self, tokens: Sequence[int], start_pos: int = 0, targets: Optional[Sequence[int]] = None, top1: bool = False):
        """log P(targets[i] | tokens[0..i]) (natural log) as float32 [len(tokens)], 0 where targets[i] < 0 -- one prompt pass at start_pos
        (nt_engine_score_tokens; the KV cache afterwards is forward's).  targets default to the next token: tokens[1:] + [-1].
        top1=True: (logprobs, int32 greedy token behind every prefix)."""
        n = len(tokens)
        tg = (list(tokens[1:]) + [-1])[:n] if targets is None else list(targets)
        if len(tg) != n:
            raise ValueError("score: %d targets for %d tokens" % (len(tg), n))
        arr = (C.c_int * n)(*[int(t) for t in tokens])
        tarr = (C.c_int * n)(*[int(t) for t in tg])
        lp = np.empty(n, np.float32)
        ids = np.empty(n, np.int32) if top1 else None
        st = self.L.nt_engine_score_tokens(self.h, arr, tarr, n, start_pos, lp.ctypes.data_as(C.c_void_p),
                                           ids.ctypes.data_as(C.c_void_p) if top1 else None)
        if st < 0:
            self._check(st, "score")
        return (lp, ids) if top1 else lp

    def perplexity(self, tokens: Sequence[int], window: Optional[int] = None, bos: Optional[int] = None):
        """(exp(-mean log P), number of scored tokens) over windows of at most `window` tokens (default and at most the context), each scored from
        position 0, the sum kept in float64.
        bos=None: the windows are cut from `tokens` as they are; a window's first token is context only and is not scored (n_scored = len(tokens)
        - the number of windows), and a last window of ONE token has nothing to score.
        bos=<id>: what `ntransformer --perplexity` computes on text tokenised WITHOUT a BOS -- windows of window - 1 tokens with `bos` put in front of
        each, every token of `tokens` scored (n_scored = len(tokens))."""
        ctx = self.max_context
        window = ctx if window is None else max(2, min(int(window), ctx))
        per = window if bos is None else window - 1
        total, count = 0.0, 0
        for w0 in range(0, len(tokens), per):
            chunk = ([] if bos is None else [int(bos)]) + list(tokens[w0:w0 + per])
            if len(chunk) < 2:
                break
            total += float(self.score(chunk)[:-1].astype(np.float64).sum())
            count += len(chunk) - 1
        if count == 0:
            raise ValueError("perplexity: nothing to score (fewer than two tokens in a window)")
        return float(np.exp(-total / count)), count

    # ---- parity instrumentation (include/ntransformer.h: nt_engine_debug_*) ----
    def debug_run_layers(self, hidden_in: np.ndarray, start_pos: int, first: int, count: int = 1, mode: int = 0) -> np.ndarray:
        """layers [first, first+count) on caller-supplied hidden states [T, H]; mode 0 = 1:1 launchers, 1 = fused, 2 = fused via hipGraph"""
        x = np.ascontiguousarray(hidden_in, dtype=np.float32)
        if x.ndim == 1:
            x = x[None, :]
        out = np.empty_like(x)
        self._check(self.L.nt_engine_debug_run_layers(self.h, x.ctypes.data_as(C.c_void_p), x.shape[0], start_pos, first, count, mode,
                                                      out.ctypes.data_as(C.c_void_p)), "debug_run_layers")
        return out

    def kv_read(self, layer: int, pos0: int, n: int, row_halves: int):
        """(K, V) cache rows [pos0, pos0+n) of one layer as uint16 [n, n_kv_heads * head_dim]"""
        k = np.empty((n, row_halves), np.uint16)
        v = np.empty((n, row_halves), np.uint16)
        self._check(self.L.nt_engine_debug_kv_read(self.h, layer, pos0, n, k.ctypes.data_as(C.c_void_p), v.ctypes.data_as(C.c_void_p)), "kv_read")
        return k, v

    def kv_write(self, layer: int, pos0: int, k: np.ndarray, v: np.ndarray) -> None:
        k = np.ascontiguousarray(k, dtype=np.uint16)
        v = np.ascontiguousarray(v, dtype=np.uint16)
        self._check(self.L.nt_engine_debug_kv_write(self.h, layer, pos0, k.shape[0], k.ctypes.data_as(C.c_void_p), v.ctypes.data_as(C.c_void_p)), "kv_write")

    def kv_read_q8(self, layer: int, pos0: int, n: int, row_elems: int):
        """(K, V) rows [pos0, pos0+n) of a kv_cache=q8_0 engine as canonical GGUF block_q8_0 bytes, uint8 [n, row_elems / 32, 34]"""
        k = np.empty((n, row_elems // 32, 34), np.uint8)
        v = np.empty((n, row_elems // 32, 34), np.uint8)
        self._check(self.L.nt_engine_debug_kv_read_q8(self.h, layer, pos0, n, k.ctypes.data_as(C.c_void_p), v.ctypes.data_as(C.c_void_p)), "kv_read_q8")
        return k, v

    def kv_write_q8(self, layer: int, pos0: int, k_blocks: np.ndarray, v_blocks: np.ndarray) -> None:
        k = np.ascontiguousarray(k_blocks, dtype=np.uint8)
        v = np.ascontiguousarray(v_blocks, dtype=np.uint8)
        self._check(self.L.nt_engine_debug_kv_write_q8(self.h, layer, pos0, k.shape[0], k.ctypes.data_as(C.c_void_p), v.ctypes.data_as(C.c_void_p)), "kv_write_q8")

    def kv_read_q8_slot(self, slot: int, layer: int, pos0: int, n: int, row_elems: int):
        """kv_read_q8 of sequence slot `slot` ("batch_kv_q8" option)"""
        k = np.empty((n, row_elems // 32, 34), np.uint8)
        v = np.empty((n, row_elems // 32, 34), np.uint8)
        self._check(self.L.nt_engine_debug_kv_read_q8_slot(self.h, int(slot), layer, pos0, n, k.ctypes.data_as(C.c_void_p), v.ctypes.data_as(C.c_void_p)),
                    "kv_read_q8_slot")
        return k, v

    def kv_write_q8_slot(self, slot: int, layer: int, pos0: int, k_blocks: np.ndarray, v_blocks: np.ndarray) -> None:
        k = np.ascontiguousarray(k_blocks, dtype=np.uint8)
        v = np.ascontiguousarray(v_blocks, dtype=np.uint8)
        self._check(self.L.nt_engine_debug_kv_write_q8_slot(self.h, int(slot), layer, pos0, k.shape[0], k.ctypes.data_as(C.c_void_p),
                                                            v.ctypes.data_as(C.c_void_p)), "kv_write_q8_slot")

    def kv_inputs_capture(self, layer: int) -> None:
        self._check(self.L.nt_engine_debug_kv_inputs_capture(self.h, layer), "kv_inputs_capture")

    def kv_inputs_read(self, n: int, row_elems: int):
        """(k before the rotation, v) F32 [n, row_elems] that the captured layer's KV store read in the last prompt pass"""
        k = np.empty((n, row_elems), np.float32)
        v = np.empty((n, row_elems), np.float32)
        self._check(self.L.nt_engine_debug_kv_inputs_read(self.h, n, k.ctypes.data_as(C.c_void_p), v.ctypes.data_as(C.c_void_p)), "kv_inputs_read")
        return k, v

    def kv_cache_bytes(self) -> int:
        return int(self.L.nt_engine_kv_cache_bytes(self.h))

    def generate_tokens(self, prompt: Sequence[int], max_tokens: int, temperature: float = 0.0, top_k: int = 40,
                        top_p: float = 0.9, repeat_penalty: float = 1.0, repeat_window: int = 64, seed: int = 42,
                        stop_at_eos: bool = True) -> List[int]:
        p = GenParams(max_tokens, temperature, top_k, top_p, repeat_penalty, repeat_window, seed, int(stop_at_eos))
        arr = (C.c_int * len(prompt))(*[int(t) for t in prompt])
        out = (C.c_int * max(max_tokens, 1))()
        n = self.L.nt_engine_generate_tokens(self.h, arr, len(prompt), C.byref(p), out, max_tokens)
        if n < 0:
            self._check(n, "generate_tokens")
        return list(out[:n])

    def generate(self, prompt: str, max_tokens: int, temperature: float = 0.7, top_k: int = 40, top_p: float = 0.9) -> str:
        r = self.L.nt_engine_generate(self.h, prompt.encode(), max_tokens, temperature, top_k, top_p)
        if not r:
            raise _lib.NtkError(-3, "generate")
        s = C.string_at(r).decode("utf-8", "replace")
        self.L.nt_free(r)
        return s

    def decode_greedy_steps(self, token: int, pos: int, n: int) -> List[int]:
        out = (C.c_int * max(n, 1))()
        self._check(self.L.nt_engine_decode_greedy_steps(self.h, int(token), pos, n, out), "decode_greedy_steps")
        return list(out[:n])

    def profile_token(self, token: int, pos: int, coarse: bool = True):
        """One eager fused token timed with HIP events; see nt_engine_profile_token (coarse: one event per run of
        same-class launches)."""
        ms, calls = (C.c_float * 4)(), (C.c_int * 4)()
        self._check(self.L.nt_engine_profile_token(self.h, int(token), pos, 1 if coarse else 0, ms, calls), "profile_token")
        return list(ms), list(calls)

    def stats(self) -> Stats:
        s = CStats()
        self.L.nt_engine_last_stats(self.h, C.byref(s))
        return Stats(s.prompt_tokens, s.gen_tokens, s.prefill_ms, s.decode_ms, s.decode_tok_s)

    def bytes_per_token(self, pos: int = 0) -> int:
        return int(self.L.nt_engine_bytes_per_token(self.h, pos))

    def decode_path(self) -> str:
        return (self.L.nt_engine_decode_path(self.h) or b"").decode()

    def weight_bytes(self) -> int:
        return int(self.L.nt_engine_weight_bytes(self.h))

    def resident_weight_bytes(self) -> int:
        return int(self.L.nt_engine_resident_weight_bytes(self.h))

    def load_shared(self, src: "Engine", max_context: int = 4096) -> None:
        """a second sequence over the weights `src` holds resident (nt_engine_load_shared): own caches / buffers / stream; keep `src` alive"""
        self.L.nt_engine_load_shared.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
        self._check(self.L.nt_engine_load_shared(self.h, src.h, max_context), "load_shared")
        self._shared_from = src

    def repacked_bytes(self) -> int:
        self.L.nt_engine_repacked_bytes.restype = C.c_uint64
        self.L.nt_engine_repacked_bytes.argtypes = [C.c_void_p]
        return int(self.L.nt_engine_repacked_bytes(self.h))

    def tokenize(self, text: str, add_bos: bool = True) -> List[int]:
        out = (C.c_int * 4096)()
        n = self.L.nt_engine_tokenize(self.h, text.encode(), int(add_bos), out, 4096)
        return list(out[:n])


def forward_batch_validate(slots: Sequence[int], lens: Sequence[int], start_positions: Sequence[int], sequences: int, max_seq: int, n: Optional[int] = None) -> int:
    """Host only (nt_forward_batch_validate): the argument checks of Engine.forward_batch (token ids aside) for an engine of `sequences` slots and
    `max_seq` positions: 0, NTK_E_NULL or NTK_E_SHAPE.  n: the segment count passed (default: len(slots))."""
    ia = lambda xs: (C.c_int * max(len(xs), 1))(*[int(x) for x in xs])
    return int(_bind().nt_forward_batch_validate(ia(slots), ia(lens), ia(start_positions), len(slots) if n is None else int(n), int(sequences), int(max_seq)))


def kv_shift_validate(slot: int, keep: int, discard: int, n_past: int, sequences: int, max_seq: int) -> int:
    """Host only (nt_kv_shift_validate): the argument checks of Engine.kv_shift for an engine of `sequences` slots and `max_seq` positions: 0 or NTK_E_SHAPE."""
    return int(_bind().nt_kv_shift_validate(int(slot), int(keep), int(discard), int(n_past), int(sequences), int(max_seq)))


def kv_copy_validate(src_slot: int, dst_slot: int, pos0: int, n: int, sequences: int, max_seq: int) -> int:
    """Host only (nt_kv_copy_validate): the argument checks of Engine.kv_copy: 0 or NTK_E_SHAPE."""
    return int(_bind().nt_kv_copy_validate(int(src_slot), int(dst_slot), int(pos0), int(n), int(sequences), int(max_seq)))


def context_shift_discard(n_past: int, keep: int) -> int:
    """Host only (nt_context_shift_discard): how many positions the generate loop drops when the context is full: max(1, (n_past - keep) // 2)."""
    return int(_bind().nt_context_shift_discard(int(n_past), int(keep)))


def rope_llama3_factors(head_dim: int, theta: float, factor: float = 8.0, low_freq_factor: float = 1.0, high_freq_factor: float = 4.0,
                        orig_ctx: int = 8192) -> np.ndarray:
    """Host only (nt_rope_llama3_factors): the Llama-3.1 frequency divisors as the engine computes them for rope_scaling=llama3:..., float32 [head_dim / 2]."""
    out = np.zeros(head_dim // 2, np.float32)
    check(_bind().nt_rope_llama3_factors(int(head_dim), theta, factor, low_freq_factor, high_freq_factor, int(orig_ctx), out.ctypes.data_as(C.c_void_p)),
          "rope_llama3_factors")
    return out


def rope_build_table(head_dim: int, theta: float, factors: Optional[np.ndarray] = None) -> np.ndarray:
    """Host only (nt_rope_build_table): the engine's frequency table, (1 / powf(theta, 2i / head_dim)) / factors[i] in F32, float32 [head_dim / 2]."""
    out = np.zeros(head_dim // 2, np.float32)
    fa = None if factors is None else np.ascontiguousarray(factors, dtype=np.float32)
    check(_bind().nt_rope_build_table(int(head_dim), theta, None if fa is None else fa.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)),
          "rope_build_table")
    return out


def gguf_describe(path: str) -> dict:
    """Host only (nt_gguf_describe): the C++ reader's view of a GGUF file -- hyper-parameters, the RoPE scaling fields and the tensor table."""
    import json
    L = _bind()
    n = L.nt_gguf_describe(path.encode(), None, 0)
    if n < 0:
        raise _lib.NtkError(int(n), "gguf_describe " + path)
    buf = C.create_string_buffer(n + 1)
    L.nt_gguf_describe(path.encode(), buf, n + 1)
    return json.loads(buf.value.decode())


def sampler_draw_nth(logits: np.ndarray, params: GenParams, recent: Sequence[int], skip: int) -> int:
    """Host only (nt_sampler_draw_nth): the token a Sampler seeded with params.seed returns for its draw number `skip` -- one repeat penalty over `recent`
    (its last repeat_window entries), then one sample -- on `logits`."""
    x = np.ascontiguousarray(logits, dtype=np.float32)
    rec = (C.c_int * max(len(recent), 1))(*[int(t) for t in recent])
    out = C.c_int()
    check(_bind().nt_sampler_draw_nth(x.ctypes.data_as(C.c_void_p), x.size, C.byref(params), rec, len(recent), int(skip), C.byref(out)), "sampler_draw_nth")
    return int(out.value)


def sampler_uniforms(seed: int, n: int) -> np.ndarray:
    """Host only (nt_sampler_uniforms): the first n uniform draws of a sampler seeded with `seed`, float32."""
    out = np.zeros(max(n, 1), np.float32)
    got = _bind().nt_sampler_uniforms(int(seed), n, out.ctypes.data_as(C.c_void_p))
    if got != n:
        raise _lib.NtkError(int(got), "sampler_uniforms")
    return out[:n]


def synth_write_gguf(path: str, spec: SynthSpec, nthreads: int = 0) -> None:
    check(_bind().nt_synth_write_gguf(path.encode(), C.byref(spec), nthreads), "synth_write_gguf")


def synth_tensor(spec: SynthSpec, name: str, nthreads: int = 0) -> np.ndarray:
    L = _bind()
    n = L.nt_synth_tensor(C.byref(spec), name.encode(), None, 0, nthreads)
    if n < 0:
        raise _lib.NtkError(int(n), "synth_tensor " + name)
    buf = np.empty(n, np.uint8)
    L.nt_synth_tensor(C.byref(spec), name.encode(), buf.ctypes.data_as(C.c_void_p), n, nthreads)
    return buf
