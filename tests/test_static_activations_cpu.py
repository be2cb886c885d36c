"""The "static_activations" option and the static decode slots' entry points, as far as they go without a GPU: the option's values before any load,
and the new C symbols through the library handle."""
import pytest

from ntransformer_amd import _lib
from ntransformer_amd import engine as E


def test_static_activations_accepts_0_and_1_before_a_load_and_refuses_other_values():
    e = E.Engine()
    for value in ("0", "1", 0, 1, "1", "0"):
        e.set_option("static_activations", value)
    for value in ("2", "-1", "yes", "", "01", "1 "):
        with pytest.raises(_lib.NtkError) as ei:
            e.set_option("static_activations", value)
        assert ei.value.status == -2 and "must be 0 or 1" in str(ei.value)   # NTK_E_SHAPE + last_error
    e.set_option("static_activations", "1")                                  # (a refusal leaves the engine usable)
    e.close()


def test_the_new_c_symbols_resolve_and_refuse_slots_that_do_not_exist():
    L = _lib.lib()
    for name in ("ntk_decode_arena_acquire", "ntk_decode_arena_release", "ntk_decode_arena_slot", "ntk_debug_gemv_static_x"):
        assert getattr(L, name) is not None, name
    assert L.ntk_decode_arena_slot(0) is None and L.ntk_decode_arena_slot(4) is None and L.ntk_decode_arena_slot(-1) is None
    assert 0 <= L.ntk_debug_gemv_static_x() <= 3
