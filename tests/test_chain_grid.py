"""The grid seam of the receive and transmit chain (WCE_VARIANT_GRID = 6, csrc/wce_internal.h
chain_grid), on the host: every looping chain launcher asks chain_grid for its grid, and
wce_debug_chain_grid returns its answer.  Knob 0: min(blocks, the launcher's own cap).  Knob set:
min(blocks, 3), so that tests/test_chain_loops_gpu.py makes every wave loop at a few dozen frames.
No device is needed."""
import pytest

GRID = 6   # WCE_VARIANT_GRID
# the launchers' own caps (csrc): launch_front 256 * 40; launch_sync 4 per CU, 256 CUs on an MI355X; DM_GRID_CAP,
# DC_GRID_CAP and RE_GRID_CAP 4096; VT_GRID_CAP 2^16; TX_GRID_CAP 2^20
CAPS = {"front": 10240, "sync": 4 * 256, "demod": 4096, "demap": 4096, "viterbi": 1 << 16, "reencode": 4096,
        "transmit": 1 << 20}
BLOCKS = (1, 2, 3, 4, 17, 1023, 1024, 1025, 4096, 4097, 10240, 10241, 65536, 65537, (1 << 20) - 1, 1 << 20,
          (1 << 20) + 1, 1 << 31, (1 << 31) + 5)


@pytest.fixture()
def lib(wce):
    lib = wce.load()
    assert lib.wce_debug_set_variant(GRID, 0) == 0
    yield lib
    assert lib.wce_debug_set_variant(GRID, 0) == 0


@pytest.mark.parametrize("name", sorted(CAPS))
def test_knob_off_is_each_launchers_own_cap(lib, name):
    cap = CAPS[name]
    for blocks in BLOCKS:
        assert lib.wce_debug_chain_grid(blocks, cap) == min(blocks, cap), (name, blocks)


@pytest.mark.parametrize("value", [1, 2, 31])
def test_knob_on_is_three_workgroups(lib, value):
    assert lib.wce_debug_set_variant(GRID, value) == 0
    for cap in CAPS.values():
        for blocks in BLOCKS:
            assert lib.wce_debug_chain_grid(blocks, cap) == min(blocks, 3), (cap, blocks)
    assert lib.wce_debug_set_variant(GRID, 0) == 0
    assert lib.wce_debug_chain_grid(4097, 4096) == 4096


def test_refused_values_leave_the_knob_alone(lib):
    for value in (-1, 32, 1 << 20):
        assert lib.wce_debug_set_variant(GRID, value) == -1, value
        assert lib.wce_last_error()
        assert lib.wce_debug_chain_grid(100, 50) == 50            # still off
    assert lib.wce_debug_set_variant(GRID, 1) == 0
    for value in (-1, 32):
        assert lib.wce_debug_set_variant(GRID, value) == -1, value
        assert lib.wce_debug_chain_grid(100, 50) == 3             # still on
    assert lib.wce_debug_set_variant(GRID, 0) == 0
    assert lib.wce_debug_chain_grid(100, 50) == 50


def test_variant_7_does_not_exist(lib):
    assert lib.wce_debug_set_variant(7, 0) == -1
    assert lib.wce_debug_set_variant(-1, 0) == -1


def test_the_other_variants_do_not_move_the_grid(lib):
    """which 5 = 4 caps launch_mmse_rank1's grid, not the chain's"""
    assert lib.wce_debug_set_variant(5, 4) == 0
    try:
        assert lib.wce_debug_chain_grid(100, 50) == 50
    finally:
        assert lib.wce_debug_set_variant(5, 0) == 0
