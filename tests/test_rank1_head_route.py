"""Which of the closed form's two kernels a launch runs, decided on the CPU by rank1_head_shape
(csrc/wce_route.cpp) through wce_debug_rank1_head, and the head kernel's placement of its groups
(rank1_head_group through wce_debug_rank1_head_groups).

mmse_rank1_head_kernel takes the headline's launch only: a shared u, no MATLAB split, no per-frame noise,
no given w, a State with a = 1 and a full mask, the default cache policy, strides below 2^32 and fewer
than 2^31 frames -- the 32-bit limits are what no small GPU test reaches.  WCE_VARIANT_R1 = 14..19 name
its shapes, 13 switches it off, 0 runs what was adopted, 1..12 are mmse_rank1_kernel's own.  No GPU."""
import ctypes
import itertools

import pytest

NX = 8
FS, WS, NFR = 795, 53, 65536   # bench.py's headline: frames of 15 blocks, H rows of 53
SHAPES = {14: (64, 0), 15: (128, 0), 16: (256, 0), 17: (64, 1), 18: (128, 1), 19: (256, 1)}
OFF = 13


def _head(wce, shared=1, split=0, noise=0, cw=0, plain=1, nt=0, variant=17, fs=FS, ws=WS, n=NFR, nx=NX):
    remap = ctypes.c_int(-1)
    t = wce.load().wce_debug_rank1_head(shared, split, noise, cw, plain, nt, variant, fs, ws, n, nx, ctypes.byref(remap))
    assert remap.value in (0, 1)
    return t, remap.value


def test_symbols_are_exported(wce):
    lib = wce.load()
    for name in ("wce_debug_rank1_head", "wce_debug_rank1_head_groups"):
        assert hasattr(lib, name) and name in wce.wce.ABI


@pytest.mark.parametrize("variant", sorted(SHAPES))
def test_truth_table(wce, variant):
    """Every combination of the six facts: the one eligible row takes the variant's shape, every other row
    mmse_rank1_kernel."""
    n = 0
    for shared, split, noise, cw, plain, nt in itertools.product((0, 1), repeat=6):
        got = _head(wce, shared, split, noise, cw, plain, nt, variant)
        eligible = (shared, split, noise, cw, plain, nt) == (1, 0, 0, 0, 1, 0)
        assert got == (SHAPES[variant] if eligible else (0, 0)), (shared, split, noise, cw, plain, nt)
        n += eligible
    assert n == 1


def test_other_variants_keep_the_old_kernel(wce):
    """1..12 are mmse_rank1_kernel's launch shapes, policies and builds; 13 is the head kernel switched off."""
    for v in list(range(1, 13)) + [OFF, 20, 31]:
        assert _head(wce, variant=v) == (0, 0), v


def test_default_is_one_of_the_named_shapes(wce):
    """Variant 0 on the eligible launch runs what one of 13..19 runs, and never the head kernel elsewhere."""
    assert _head(wce, variant=0) in [(0, 0)] + list(SHAPES.values())
    for kw in (dict(shared=0), dict(split=1), dict(noise=1), dict(cw=1, shared=0), dict(plain=0), dict(nt=1)):
        assert _head(wce, variant=0, **kw) == (0, 0), kw


@pytest.mark.parametrize("variant", sorted(SHAPES))
def test_32_bit_limits(wce, variant):
    want = SHAPES[variant]
    assert _head(wce, variant=variant, fs=2**32 - 1, ws=2**32 - 1, n=2**31 - 1) == want
    assert _head(wce, variant=variant, fs=0, ws=0, n=1) == want
    assert _head(wce, variant=variant, fs=2**32) == (0, 0)
    assert _head(wce, variant=variant, ws=2**32) == (0, 0)
    assert _head(wce, variant=variant, n=2**31) == (0, 0)
    assert _head(wce, variant=variant, fs=-1) == (0, 0)
    assert _head(wce, variant=variant, ws=-FS) == (0, 0)


@pytest.mark.parametrize("variant", sorted(SHAPES))
def test_no_remap_on_one_xcd(wce, variant):
    assert _head(wce, variant=variant, nx=1) == (SHAPES[variant][0], 0)


@pytest.mark.parametrize("nx", [1, 8])
def test_group_map_serves_every_group_once(wce, nx):
    lib = wce.load()
    for G in range(1, 71):
        per = -(-G // nx)
        out = (ctypes.c_uint32 * (nx * per))()
        grid = lib.wce_debug_rank1_head_groups(G, nx, out, len(out))
        assert grid == nx * per and G <= grid < G + nx, (G, nx, grid)
        got = list(out)
        live = [L for L in got if L < G]
        assert sorted(live) == list(range(G)), (G, nx)             # each group exactly once
        assert sorted(got) == list(range(grid)), (G, nx)           # a bijection of the grid
        if nx == 1:
            assert got == list(range(G))
        else:   # workgroup b runs on XCD b % nx: the groups of one XCD are neighbours
            for x in range(nx):
                mine = sorted(L for b, L in enumerate(got) if b % nx == x)
                assert mine == list(range(x * per, x * per + per)), (G, x)


def test_group_map_rejects_bad_arguments(wce):
    lib = wce.load()
    out = (ctypes.c_uint32 * 8)()
    assert lib.wce_debug_rank1_head_groups(0, 8, out, 8) < 0
    assert lib.wce_debug_rank1_head_groups(5, 0, out, 8) < 0
    assert lib.wce_debug_rank1_head_groups(9, 8, out, 8) < 0    # grid 16 > cap
    assert lib.wce_debug_rank1_head_groups(5, 8, None, 8) < 0
