"""Packet detection and symbol timing, the parts that need no GPU: the three
entry points exist (libwce.so, include/wce.h, the Python mirror and its
keywords), and the bounds the GPU tests hold the kernel to
(tests/test_sync_gpu.py) are ones an fp64 implementation can meet.

TOL_M.  metric = 2 |c[d]| |c[d+64]| / (El E[d]) <= 1.  With u = 2^-53, a
64-term complex dot product summed directly carries a relative error of
(64 + 2) u against sum |x| |ltf|, which Cauchy-Schwarz bounds by sqrt(El E)
per factor: 2 * 66 u for the two of them on M <= 1; E[d], 128 terms of two
squares each, summed directly: 256 u relative; moduli, products and the
quotient: 10 u more.  |dM| <~ (2 * 66 + 256 + 10) 2^-53 = 4.4e-14; TOL_M = 1e-13.

start is compared exactly, which is legitimate only where the best lag beats
every other by more than the metric's error: every data set has a gap above
MIN_GAP = 1e-9 on the long double model (four decades over TOL_M), no frame
left out.

Measured: fp64 against long double at most 1.4e-15 on every set, every lag;
smallest gap 3.8e-04 (shape B=777 L=191)."""
import inspect
import os
import re

import numpy as np

import sync_model as sm

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMS = {"wce_front_end_sync": 11, "wce_front_end_preamble_at": 12, "wce_front_end_blocks_at": 13}


def test_symbols_exported_and_declared(wce):
    lib = wce.load()
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "wce.h")).read(), flags=re.S)
    for s, n in SYMS.items():
        assert hasattr(lib, s), s
        assert re.search(r"\bint\s+%s\s*\(" % s, hdr), s
        params = re.search(r"\b%s\s*\(([^)]*)\)" % s, hdr).group(1).split(",")
        assert len(params) == len(wce.wce.ABI[s]) == n, s


def test_python_keywords(wce):
    C = wce.Context
    for fn, kws in ((C.front_end_sync, {"backoff": 0, "start": None, "metric": None, "capture_stride": None,
                                        "stream": None}),
                    (C.front_end_blocks, {"start": None, "capture_len": None, "cfo": None, "sample_offset": 0}),
                    (C.front_end_preamble, {"start": None, "capture_len": None, "cfo": None, "estimate_cfo": True}),
                    (C.receive_capture_host, {"backoff": 0, "mask": wce.ALL, "semantics": wce.SEM_MATLAB,
                                              "cfo": False, "sample_offset": 0})):
        p = inspect.signature(fn).parameters
        for k, default in kws.items():
            assert k in p and p[k].default == default, (fn.__name__, k)
    names = list(inspect.signature(C.front_end_sync).parameters)
    assert names[1:6] == ["capture", "n_frames", "capture_len", "ltf", "threshold"]
    names = list(inspect.signature(C.receive_capture_host).parameters)
    assert names[1:5] == ["tx_packets", "tx_lptot", "rx_capture", "threshold"]


def test_tolerance_is_reachable_and_gaps_are_wide(golden):
    assert (2 * 66 + 256 + 10) * 2.0 ** -53 < sm.TOL_M / 2
    worst, tight = 0.0, np.inf
    for name, (cap, ltf) in sm.all_sets(golden["matlab"]).items():
        M_ld, M_64 = sm.metric(cap, ltf), sm.metric(cap, ltf, np.float64)
        assert M_64.dtype == np.float64 and M_ld.dtype == np.longdouble
        err = float(np.max(np.abs(M_64 - M_ld)))          # every lag, not the best one only
        gap = float(sm.gaps(cap, ltf).min())
        print(f"{name}: fp64 vs long double {err:.2e}, smallest gap {gap:.2e}, M up to {float(M_ld.max()):.3f}")
        assert err <= sm.TOL_M, name
        assert gap > sm.MIN_GAP, name
        assert float(M_ld.max()) <= 1.0 and float(M_ld.min()) >= 0.0, name
        worst, tight = max(worst, err), min(tight, gap)
    print(f"worst {worst:.2e}, tightest gap {tight:.2e}")


def test_data_puts_peaks_where_the_tests_need_them(golden):
    m = golden["matlab"]
    ltf = sm.clean_ltf()
    for B, L in sm.SHAPES:
        cap, pos = sm.shape_set(B, L)
        assert np.all(cap[:, L:] == sm.SENT)
        d = sm.sync(cap[:, :L], ltf, 0.0)[2]
        assert 0 in d, (B, L)                              # a peak at lag 0
        if B > 1:
            assert L - 128 in d, (B, L)                    # and one at the last lag
    for prefix in (0, 37, 100):                            # the recorded packet: the field's sample 32, whatever
        cap, l = sm.recorded(m, prefix)                    # the rotation
        s, M, d = sm.sync(cap, l, 0.25, 0)
        assert np.all(s == prefix + 32), prefix
        assert np.allclose(M, [0.776, 0.740, 0.344], atol=2e-3), M
    cap, pos = sm.loud_then_quiet()
    assert np.all(np.abs(sm.sync(cap, ltf, 0.0)[2] - pos) <= 3)
    assert float(sm.sync(sm.noise_only(), ltf, 0.0)[1].max()) < 0.1


def test_model_rules():
    """threshold, backoff and poison in the model itself, on one small set"""
    cap, _ = sm.shape_set(9, 192)
    cap, ltf = cap[:, :192], sm.clean_ltf()
    s0, M, d = sm.sync(cap, ltf, 0.0)
    assert np.array_equal(s0, d)
    assert np.all(sm.sync(cap, ltf, 1.0)[0] == -1)
    s5 = sm.sync(cap, ltf, 0.0, 5)[0]
    assert np.array_equal(s5, np.where(d >= 5, d - 5, -1)) and (s5 == -1).any() and (s5 >= 0).any()
    thr = float(np.sort(M)[4])
    assert np.array_equal(sm.sync(cap, ltf, thr)[0] >= 0, M >= thr)
    bad = cap.copy()
    bad[3, 100] = np.nan
    s, Mb, _ = sm.sync(bad, ltf, 0.0)
    assert s[3] == -1 and np.isnan(Mb[3]) and np.array_equal(np.delete(Mb, 3), np.delete(M, 3))
    # half a field scores nothing: only the later copy inside the window
    half = np.zeros((1, 192), complex)
    half[0, :64] = ltf
    assert float(sm.metric(half, ltf).max()) == 0.0
