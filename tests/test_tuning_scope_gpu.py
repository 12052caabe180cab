"""The scope of a tuning override (ops.tuning over mg_set_tuning / mg_get_tuning, include/moegan_hip.h): ABI calls only,
no kernel is launched.  The slot is NARROW_BLOCKS (17), a numeric grid target that nothing here reads.  Every test
leaves the slot as it found it, so a session-wide MOEGAN_TUNE override survives them."""
import pytest

from moegan_mi import _lib as L
from moegan_mi import ops

pytestmark = pytest.mark.gpu
SLOT = L.TUNE["NARROW_BLOCKS"]


def get(key=SLOT):
    return L.lib().mg_get_tuning(key)


def test_set_and_get_round_trip():
    before = get()
    with ops.tuning(NARROW_BLOCKS=before + 3):
        assert get() == before + 3
    assert get() == before


def test_restored_after_an_exception():
    before = get()
    with pytest.raises(ZeroDivisionError):
        with ops.tuning(NARROW_BLOCKS=before + 3):
            assert get() == before + 3
            1 / 0
    assert get() == before


def test_nested_scopes_restore_in_order():
    before = get()
    with ops.tuning(NARROW_BLOCKS=before + 1):
        with ops.tuning(NARROW_BLOCKS=before + 2):
            with ops.tuning(NARROW_BLOCKS=before + 3):
                assert get() == before + 3
            assert get() == before + 2
        assert get() == before + 1
    assert get() == before


def test_restores_the_prior_value_not_zero():
    before = get()
    L.call("mg_set_tuning", SLOT, 5)
    try:
        with ops.tuning(NARROW_BLOCKS=7):
            assert get() == 7
        assert get() == 5
    finally:
        L.call("mg_set_tuning", SLOT, before)


def test_several_slots_in_one_scope():
    """Two slots set by one scope are both visible inside it and both back after an exception."""
    wide = L.TUNE["WIDE_BLOCKS"]
    before = get(), get(wide)
    with pytest.raises(RuntimeError, match="inside"):
        with ops.tuning(NARROW_BLOCKS=before[0] + 1, WIDE_BLOCKS=before[1] + 1):
            assert (get(), get(wide)) == (before[0] + 1, before[1] + 1)
            raise RuntimeError("inside")
    assert (get(), get(wide)) == before


@pytest.mark.parametrize("slot", [8, 23])
def test_retired_slots_accept_only_zero(slot):
    lib = L.lib()
    assert lib.mg_set_tuning(slot, 1) == -1  # MG_ERR_ARG
    msg = lib.mg_last_error().decode()
    assert "retired" in msg and str(slot) in msg, msg
    assert lib.mg_get_tuning(slot) == 0
    assert lib.mg_set_tuning(slot, 0) == 0
    with pytest.raises(L.MGError, match="retired"):
        L.call("mg_set_tuning", slot, 1)


def test_get_refuses_a_key_out_of_range():
    lib = L.lib()
    assert lib.mg_get_tuning(31) == -1  # MG_ERR_ARG
    assert "out of range" in lib.mg_last_error().decode()
    assert lib.mg_get_tuning(-1) == -1
