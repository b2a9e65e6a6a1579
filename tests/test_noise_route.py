"""The route of a wce_estimate_noise call (per-frame ow2), planned on the CPU by
csrc/wce_route.cpp through wce_debug_route_noise: without the noise fact it is
wce_debug_route's plan on every row of the fact grid tests/test_route.py walks
(tests/golden/mmse_routes.json); with it a TEXTBOOK request always takes the
closed form (mmse_rank1_kernel), whatever the border dot and WCE_VARIANT_R1 say,
and every other context or a mask without PS_MMSE is WCE_EINVAL.  No GPU."""
import ctypes
import itertools
import json
import os

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
EINVAL = -1


@pytest.fixture(scope="module")
def rows():
    with open(os.path.join(HERE, "golden", "mmse_routes.json")) as f:
        return [r[:12] for r in json.load(f)["rows"]]


def test_symbols_are_exported(wce):
    lib = wce.load()
    assert hasattr(lib, "wce_estimate_noise") and hasattr(lib, "wce_debug_route_noise")
    assert "wce_estimate_noise" in wce.wce.ABI and "wce_debug_route_noise" in wce.wce.ABI


def test_noise_off_is_wce_debug_route(wce, rows):
    lib = wce.load()
    assert len(rows) > 1000
    buf = ctypes.create_string_buffer(256)
    for facts in rows:
        assert lib.wce_debug_route_noise(*facts, 0, buf, len(buf)) == 0, facts
        assert buf.value.decode() == wce.debug_route(*facts) == wce.debug_route(*facts, noise=False), facts


def _tb(wce, sem, mask, bdot=1, r1=0, fuse=1, f32=0, ref_fc=0):
    return wce.debug_route(wce.MMSE_TEXTBOOK, bdot, fuse, 0, -1, 0, sem, mask, f32, r1, ref_fc, 0, noise=True)


# (bdot, r1): the default, the border dot off, the factorisation variant, both
KNOBS = [(1, 0), (0, 0), (1, 1), (0, 1)]


@pytest.mark.parametrize("bdot,r1", KNOBS)
def test_textbook_noise_takes_the_closed_form(wce, bdot, r1):
    PS, FC, LT = wce.PS_MMSE, wce.FRAME_COV, wce.LT_LS
    C, ML = wce.SEM_C, wce.SEM_MATLAB
    kw = dict(bdot=bdot, r1=r1)
    assert _tb(wce, C, PS, **kw) == "mmse_rank1"
    assert _tb(wce, C, PS | wce.PS_LINEAR, **kw) == "ls;mmse_rank1"
    assert _tb(wce, C, PS | wce.EQUALIZE, **kw) == "ls;mmse_rank1"
    assert _tb(wce, C, wce.ALL, **kw) == "ls;mmse_rank1"
    assert _tb(wce, C, PS | FC, **kw) == "fc_u;mmse_rank1"
    assert _tb(wce, C, PS | FC | wce.PS_SINC, **kw) == "ls;fc_u;mmse_rank1"
    assert _tb(wce, C, PS | FC | LT, **kw) == "ls;matvec;mmse_rank1"      # the caller's LT_LS output is H_LT
    assert _tb(wce, C, wce.ALL | FC, **kw) == "ls;matvec;mmse_rank1"
    assert _tb(wce, ML, PS, **kw) == "mmse_rank1;fc_finish"
    assert _tb(wce, ML, wce.ALL, **kw) == "ls;mmse_rank1;fc_finish"
    assert _tb(wce, ML, PS | FC, **kw) == "ls;matvec;mmse_rank1;fc_finish"   # MATLAB's LT_LS: the general factors
    assert _tb(wce, ML, wce.ALL | FC, **kw) == "ls;matvec;mmse_rank1;fc_finish"


@pytest.mark.parametrize("bdot", [0, 1])
def test_nontemporal_variant(wce, bdot):
    PS, FC = wce.PS_MMSE, wce.FRAME_COV
    assert _tb(wce, wce.SEM_C, PS, bdot=bdot, r1=2) == "mmse_rank1_nt"
    assert _tb(wce, wce.SEM_C, wce.ALL | FC, bdot=bdot, r1=2) == "ls;matvec;mmse_rank1_nt"
    assert _tb(wce, wce.SEM_MATLAB, wce.ALL, bdot=bdot, r1=2) == "ls;mmse_rank1_nt;fc_finish"


def test_no_factorising_kernel_on_any_noise_route(wce):
    """Every combination of the knobs and the request: the solve is mmse_rank1(_nt), split finishes with
    fc_finish, and no fused_*, factor_* or apply family appears."""
    PS, FC = wce.PS_MMSE, wce.FRAME_COV
    masks = [PS, PS | wce.LT_LS, PS | wce.PS_CUBIC, PS | wce.EQUALIZE, wce.ALL]
    n = 0
    for bdot, fuse, sem, m, fc, f32, r1, ref_fc in itertools.product((0, 1), (0, 1), (0, 1), masks, (0, FC), (0, 1),
                                                                     (0, 1, 2), (0, 1)):
        fams = _tb(wce, sem, m | fc, bdot=bdot, r1=r1, fuse=fuse, f32=f32, ref_fc=ref_fc).split(";")
        solve = "mmse_rank1_nt" if r1 == 2 else "mmse_rank1"
        assert fams.count(solve) == 1 and (fams[-1] == "fc_finish") == (sem == wce.SEM_MATLAB), fams
        assert fams[-2 if sem == wce.SEM_MATLAB else -1] == solve, fams
        assert not any(f.startswith(("fused_", "factor_")) or f == "apply" for f in fams), fams
        assert ("ls" in fams) == bool(m & ~PS or (fc and "fc_u" not in fams)), fams
        n += 1
    assert n == 960


def test_rejected_noise_facts(wce):
    PS, FC = wce.PS_MMSE, wce.FRAME_COV
    bad = [
        (wce.MMSE_REF, 1, 1, 0, -1, 0, 0, PS, 0, 0, 0, 0),
        (wce.MMSE_REF, 0, 1, 0, -1, 0, 1, wce.ALL | FC, 0, 0, 0, 0),
        (wce.MMSE_COV, 1, 1, 0, -1, 53, 0, PS, 0, 0, 0, 0),            # dense
        (wce.MMSE_COV, 1, 1, 0, 5, 8, 0, PS, 0, 0, 0, 0),              # low-rank
        (wce.MMSE_COV, 1, 1, 0, -1, 53, 0, PS | FC, 0, 0, 0, 0),       # FRAME_COV does not make it the .m model's ctx
        (wce.MMSE_TEXTBOOK, 1, 1, 0, -1, 0, 0, wce.LS_ALL, 0, 0, 0, 0),
        (wce.MMSE_TEXTBOOK, 1, 1, 0, -1, 0, 1, wce.LT_LS | wce.EQUALIZE, 0, 0, 0, 0),
        (wce.MMSE_TEXTBOOK, 1, 1, 0, -1, 0, 0, 0, 0, 0, 0, 0),
    ]
    for facts in bad:
        assert wce.debug_route(*facts) is not None, facts   # a plan exists without the noise fact
        with pytest.raises(wce.WceError) as e:
            wce.debug_route(*facts, noise=True)
        assert e.value.code == EINVAL, facts
    # what wce_debug_route rejects stays rejected
    with pytest.raises(wce.WceError):
        wce.debug_route(wce.MMSE_TEXTBOOK, 1, 1, 0, -1, 0, 0, FC, 0, 0, 0, 0, noise=True)
    buf = ctypes.create_string_buffer(4)
    args = (wce.MMSE_TEXTBOOK, 1, 1, 0, -1, 0, wce.SEM_MATLAB, wce.ALL | FC, 0, 0, 0, 0, 1)
    assert wce.load().wce_debug_route_noise(*args, buf, len(buf)) == EINVAL   # short buffer
