"""The "batch_kv_q8" option and the entry points of the batched step over the 8-bit KV cache, as far as they go without a GPU: the option's values
before any load, and the new C symbols through the library handle."""
import pytest

from ntransformer_amd import _lib
from ntransformer_amd import engine as E


def test_batch_kv_q8_accepts_0_and_1_before_a_load_and_refuses_other_values():
    e = E.Engine()
    for value in ("0", "1", 0, 1, "1", "0"):
        e.set_option("batch_kv_q8", value)
    for value in ("2", "-1", "yes", "", "01", "1 "):
        with pytest.raises(_lib.NtkError) as ei:
            e.set_option("batch_kv_q8", value)
        assert ei.value.status == -2 and "must be 0 or 1" in str(ei.value)   # NTK_E_SHAPE + last_error
    e.set_option("batch_kv_q8", "1")                                      # (a refusal leaves the engine usable)
    e.close()


def test_the_new_c_symbols_resolve():
    L = _lib.lib()
    for name in ("ntk_attention_decode_q8_batch", "nt_engine_debug_kv_read_q8_slot", "nt_engine_debug_kv_write_q8_slot"):
        assert getattr(L, name) is not None, name
    E._bind()
    assert len(L.ntk_attention_decode_q8_batch.argtypes) == 18
    assert len(L.nt_engine_debug_kv_read_q8_slot.argtypes) == 7 and len(L.nt_engine_debug_kv_write_q8_slot.argtypes) == 7
    # unloaded engine: the slot calls answer NTK_E_NULL, they do not crash
    e = E.Engine()
    assert L.nt_engine_debug_kv_read_q8_slot(e.h, 0, 0, 0, 1, None, None) == -5
    assert L.nt_engine_debug_kv_write_q8_slot(e.h, 0, 0, 0, 1, None, None) == -5
    e.close()
