"""Receive diversity, the parts that need no GPU: the entry points exist (libwce.so,
include/wce.h, the Python mirrors and their keywords), every refusal of the header is
made before the context is touched, the model keeps the rules of the definition, the
bounds the GPU tests hold the kernel to (tests/test_combine_gpu.py) are derived from
the model's own error, and combining does what it is there for.

The tolerances (tests/combine_model.py): TOL_RX and TOL_H are MARGIN = 8 times the
largest gap between the fp64 model and the long double model over the parity sets
(A = 1, 2, 3, 8 branches of 67 packets, with and without ow2), rx_c relative to
bound = sum_a v_a |h_a| |rx_a| / g (the numerator can cancel) and h_c relative to g.
Measured: 6.4e-16 of the bound (5.7 u, u = 2^-53) and 2.8e-16 of g (2.5 u), so
TOL_RX = 5.1e-15 and TOL_H = 2.2e-15.  The worst case of the arithmetic is about
3 A + 6 = 30 u at A = 8; 8 times the measured gap covers it.

The link experiment's model (16-QAM rate 1/2 at nominal 10 dB, 67 packets, six static
taps per branch, LINK_SEED) on the model transmitter's captures, bit errors of the
combined chain / of each branch alone, no frame marginal:
    2 equal branches              0 / 771, 954
    2 branches, 6 dB apart        weighted 276, unweighted 2657 / 1034, 43189
    4 equal branches              0 / 1598, 1635, 1204, 1539
    4 branches, 6 dB steps        weighted 184, unweighted 47928 / 1141, 43158, 47949, 47761"""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

import combine_model as cb
import demod_model as dm
import tx_model as tm

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1
U = 2.0 ** -53


# ---------------------------------------------------------------- 1. the interface
def test_symbols_exported_and_declared(wce):
    lib = wce.load()
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "wce.h")).read(), flags=re.S)
    for name, nargs in (("wce_combine", 5), ("wce_sync_share", 8)):
        assert hasattr(lib, name), name
        assert re.search(r"\bint\s+%s\s*\(" % name, hdr), name
        params = re.search(r"\b%s\s*\(([^)]*)\)" % name, hdr).group(1).split(",")
        assert len(params) == len(wce.wce.ABI[name]) == nargs, name
    assert re.search(r"#define\s+WCE_COMBINE_MAX_BRANCHES\s+8\b", hdr) and wce.COMBINE_MAX_BRANCHES == 8
    W = wce.wce
    assert [f[0] for f in W.CombinePar._fields_] == [
        "rx", "rx_branch_stride", "rx_frame_stride", "rx_block_stride", "h", "h_branch_stride", "h_stride", "ow2",
        "ow2_branch_stride", "n_branches"]
    assert [f[0] for f in W.CombineOut._fields_] == ["rx", "rx_frame_stride", "rx_block_stride", "h", "h_stride"]
    assert ctypes.sizeof(W.CombinePar) == 80 and ctypes.sizeof(W.CombineOut) == 40
    for struct, cls in (("wce_combine_par", W.CombinePar), ("wce_combine_out", W.CombineOut)):
        body = re.search(r"typedef\s+struct\s*\{([^}]*)\}\s*%s\s*;" % struct, hdr)
        assert body, struct
        assert re.findall(r"\b(\w+)\s*(?=[,;])", body.group(1)) == [f[0] for f in cls._fields_], struct
    assert wce.CombinePar is W.CombinePar and wce.CombineOut is W.CombineOut


def test_python_keywords(wce):
    C = wce.Context
    for fn, kws in ((C.combine, {"ow2": None, "out_rx": None, "out_h": None, "rx_branch_stride": None,
                                 "rx_frame_stride": None, "rx_block_stride": wce.NSC, "h_branch_stride": None,
                                 "h_stride": wce.NSC, "ow2_branch_stride": None, "stream": None}),
                    (C.sync_share, {"start": None, "cfo": None, "branch_stride": None, "stream": None}),
                    (C.combine_host, {"ow2": None}),
                    (C.link_mrc_host, {"branch_loss_db": None, "share_sync": True, "weighted": True, "stf": False,
                                       "tracker": None, "dd_iterations": 0,
                                       "sources": (wce.LT_LS, wce.PS_LINEAR, wce.PS_MMSE)})):
        p = inspect.signature(fn).parameters
        for k, default in kws.items():
            assert k in p and p[k].default == default, (fn.__name__, k)
    assert list(inspect.signature(C.combine).parameters)[1:5] == ["rx", "h", "n_frames", "n_branches"]
    assert list(inspect.signature(C.sync_share).parameters)[1:4] == ["metric", "n_packets", "n_branches"]
    assert list(inspect.signature(C.link_mrc_host).parameters)[1:7] == [
        "modulation", "rate", "snr_db", "n_frames", "n_rx", "taps"]
    # link_host is as it was
    assert "n_rx" not in inspect.signature(C.link_host).parameters


# ---------------------------------------------------------------- 2. the refusals
def _combine_base(n=3, A=2):
    fs = 15 * 53
    par = dict(rx=0x1000, rx_branch_stride=n * fs, rx_frame_stride=fs, rx_block_stride=53, h=0x1000,
               h_branch_stride=n * 53, h_stride=53, ow2=0x1000, ow2_branch_stride=n, n_branches=A)
    out = dict(rx=0x1000, rx_frame_stride=fs, rx_block_stride=53, h=0x1000, h_stride=53)
    return par, out, n


FS = 15 * 53
COMBINE_REFUSALS = [
    ({"n_branches": 0}, {}, None, "n_branches"), ({"n_branches": 9}, {}, None, "n_branches"),
    ({"rx": None}, {}, None, "rx and h"), ({"h": None}, {}, None, "rx and h"),
    ({}, {"rx": None, "h": None}, None, "no output"),
    ({"rx_block_stride": 52}, {}, None, "rx strides"), ({"rx_frame_stride": 14 * 53 + 52}, {}, None, "rx strides"),
    ({"h_stride": 52}, {}, None, "h_stride"),
    ({}, {"rx_block_stride": 52}, None, "output rx strides"),
    ({}, {"rx_frame_stride": 14 * 53 + 52}, None, "output rx strides"),
    ({}, {"h_stride": 52}, None, "output h_stride"),
    # branch strides: too short to span a branch, too long to fit inside a block or a frame, negative, below a row
    ({"rx_branch_stride": 3 * FS - 1}, {}, None, "rx_branch_stride"),
    ({"rx_branch_stride": 52}, {}, None, "rx_branch_stride"),
    ({"rx_branch_stride": -3 * FS}, {}, None, "rx_branch_stride"),
    ({"rx_branch_stride": 53, "rx_block_stride": 105, "rx_frame_stride": 15 * 105}, {}, None, "rx_branch_stride"),
    ({"rx_branch_stride": FS, "rx_frame_stride": 2 * FS - 1}, {}, None, "rx_branch_stride"),
    ({"h_branch_stride": 3 * 53 - 1}, {}, None, "h_branch_stride"),
    ({"h_branch_stride": 53, "h_stride": 105}, {}, None, "h_branch_stride"),
    ({"ow2_branch_stride": 2}, {}, None, "ow2_branch_stride"),
    ({"rx": 0x1008}, {}, None, "16-byte"), ({"h": 0x1008}, {}, None, "16-byte"),
    ({}, {"rx": 0x1008}, None, "16-byte"), ({}, {"h": 0x1008}, None, "16-byte"),
    ({"ow2": 0x1004}, {}, None, "8-byte"),
    ({}, {}, -1, "n_frames"), ({}, {}, 2 ** 31, "n_frames"),
]
# layouts that hold: branch-minor inside a block, between frame and block, one frame, one branch with any stride
COMBINE_ACCEPTED = [
    ({"rx_branch_stride": 53, "rx_block_stride": 106, "rx_frame_stride": 15 * 106, "h_branch_stride": 53,
      "h_stride": 106}, {}),
    ({"rx_branch_stride": FS, "rx_frame_stride": 2 * FS}, {}),
    ({"n_branches": 1, "rx_branch_stride": 0, "h_branch_stride": -5, "ow2_branch_stride": 0}, {}),
    ({"ow2": None, "ow2_branch_stride": 0}, {}), ({}, {"rx": None}), ({}, {"h": None}),
]


def _call_combine(wce, lib, ctx, par, out, n):
    W = wce.wce
    return lib.wce_combine(ctx, ctypes.byref(W.CombinePar(**par)), n, ctypes.byref(W.CombineOut(**out)), None)


def test_combine_refusals_before_the_ctx_is_touched(wce):
    """every WCE_EINVAL of the header, with an opaque non-NULL ctx and opaque pointers: nothing is launched.  The
    calls that hold are made with n_frames = 0, which returns WCE_OK after the same validation."""
    lib = wce.load()
    ctx = 0x10
    for pch, och, n, text in COMBINE_REFUSALS:
        par, out, n0 = _combine_base()
        assert _call_combine(wce, lib, ctx, {**par, **pch}, {**out, **och}, n0 if n is None else n) == EINVAL, (pch, och, n)
        assert text in lib.wce_last_error().decode(), (pch, och, n, lib.wce_last_error())
    par, out, n = _combine_base()
    assert _call_combine(wce, lib, None, par, out, n) == EINVAL and "null ctx" in lib.wce_last_error().decode()
    W = wce.wce
    assert lib.wce_combine(ctx, None, n, ctypes.byref(W.CombineOut(**out)), None) == EINVAL
    assert lib.wce_combine(ctx, ctypes.byref(W.CombinePar(**par)), n, None, None) == EINVAL
    assert _call_combine(wce, lib, ctx, par, out, 0) == 0
    # one frame: the frame strides are free, and a branch stride need only clear the blocks
    one = {**par, "rx_frame_stride": 0, "rx_branch_stride": 14 * 53 + 53, "h_branch_stride": 53,
           "ow2_branch_stride": 1}
    assert _call_combine(wce, lib, ctx, {**one, "rx_branch_stride": 14 * 53 + 52}, out, 1) == EINVAL
    # the layouts that hold pass the validation: the same calls at n_frames = 0 are WCE_OK, and the refusals above
    # are refusals at n_frames = 0 too where they do not depend on it
    for pch, och in COMBINE_ACCEPTED:
        par, out, n = _combine_base(n=0)
        par.update(rx_branch_stride=3 * FS, h_branch_stride=3 * 53, ow2_branch_stride=3)
        assert _call_combine(wce, lib, ctx, {**par, **pch}, {**out, **och}, 0) == 0, (pch, och)
    par, out, n = _combine_base(n=0)
    assert _call_combine(wce, lib, ctx, {**par, "rx_branch_stride": 52}, out, 0) == EINVAL


SHARE_REFUSALS = [({"n_branches": 0}, "n_branches"), ({"n_branches": 9}, "n_branches"),
                  ({"metric": None}, "metric"), ({"metric": 0x1004}, "8-byte"),
                  ({"start": None, "cfo": None}, "both null"), ({"start": 0x1002}, "4-byte"),
                  ({"cfo": 0x1004}, "8-byte"), ({"n_packets": -1}, "n_packets"), ({"n_packets": 2 ** 31}, "n_packets"),
                  ({"branch_stride": 66}, "branch_stride")]


def test_sync_share_refusals_before_the_ctx_is_touched(wce):
    lib = wce.load()
    base = dict(n_branches=2, branch_stride=67, n_packets=67, metric=0x1000, start=0x1000, cfo=0x1000)
    for ch, text in SHARE_REFUSALS:
        assert lib.wce_sync_share(0x10, *{**base, **ch}.values(), None) == EINVAL, ch
        assert text in lib.wce_last_error().decode(), (ch, lib.wce_last_error())
    assert lib.wce_sync_share(None, *base.values(), None) == EINVAL and "null ctx" in lib.wce_last_error().decode()
    for ch in ({"n_packets": 0}, {"n_packets": 0, "start": None}, {"n_packets": 0, "cfo": None},
               {"n_packets": 0, "n_branches": 1, "branch_stride": 0}):
        assert lib.wce_sync_share(0x10, *{**base, **ch}.values(), None) == 0, ch


def test_link_mrc_host_refuses_before_the_device(wce):
    c = object.__new__(wce.Context)
    c.handle, c.tx_pre = None, tm.chain_pre()
    taps = np.ones((2, 6)) / 6
    for kw, text in (({"n_rx": 0}, "n_rx"), ({"n_rx": 9}, "n_rx"), ({"n_rx": 3}, "taps"),
                     ({"branch_loss_db": [0.0]}, "branch_loss_db"), ({"sources": (64,)}, "sources"),
                     ({"tracker": (0.5, 2), "dd_iterations": 1}, "tracker"),
                     ({"stf": True, "delay": 100, "capture_len": 1600}, "cannot hold")):
        args = {"modulation": wce.MOD_QPSK, "rate": wce.RATE_1_2, "snr_db": 30.0, "n_frames": 2, "n_rx": 2,
                "taps": taps, **kw}
        with pytest.raises(ValueError, match=text):
            c.link_mrc_host(**args)


# ---------------------------------------------------------------- 3. the model's rules
def test_one_branch_identities():
    tx, rx, h, ow2 = cb.parity_set(1)
    c = cb.combine(rx, h)
    hl, rl = np.asarray(h[0], np.clongdouble), np.asarray(rx[0], np.clongdouble)
    V = cb.V
    assert np.all(c["h"].imag == 0) and np.all(c["h"][:, dm.DC] == 0) and np.all(c["rx"][:, :, dm.DC] == 0)
    assert float(np.max(np.abs(c["h"][:, V].real - np.abs(hl[:, V])) / np.abs(hl[:, V]))) < 4 * 2.0 ** -64
    want = np.conj(hl)[:, None, V] * rl[:, :, V] / np.abs(hl)[:, None, V]
    assert float(np.max(np.abs(c["rx"][:, :, V] - want) / np.abs(want))) < 8 * 2.0 ** -64
    # and the equalized symbol is the branch's own: rx_c / h_c = rx / h
    e = c["rx"][:, :, V] / c["h"][:, None, V]
    assert float(np.max(np.abs(e - rl[:, :, V] / hl[:, None, V]) / np.abs(e))) < 8 * 2.0 ** -64


@pytest.mark.parametrize("A", (2, 4))
def test_a_common_factor_on_ow2_changes_no_equalized_symbol(A):
    tx, rx, h, ow2 = cb.parity_set(A) if A in cb.PARITY_A else cb.branches(A, loss_db=3.0 * np.arange(A))
    base = cb.combine(rx, h, ow2, np.float64)
    d0 = dm.demodulate(tx, base["rx"], base["h"], None, dm.QAM16, real=np.float64)
    # a power of 4 scales every weight and g exactly: the demodulator's eq keeps its bits
    c4 = cb.combine(rx, h, 4.0 * ow2, np.float64)
    assert np.array_equal(c4["h"], base["h"] / 2) and np.array_equal(c4["rx"], base["rx"] / 2)
    d4 = dm.demodulate(tx, c4["rx"], c4["h"], None, dm.QAM16, real=np.float64)
    assert np.array_equal(d4["eq"], d0["eq"]) and np.array_equal(d4["theta"], d0["theta"])
    # any other factor: to rounding (demod_model's bound on eq), and the same decisions
    c3 = cb.combine(rx, h, 3.7 * ow2, np.float64)
    d3 = dm.demodulate(tx, c3["rx"], c3["h"], None, dm.QAM16, real=np.float64)
    assert float(dm.relmax_frames(d3["eq"], d0["eq"]).max()) < dm.TOL_EQ
    assert np.array_equal(d3["sym"], d0["sym"])
    # while the combined stream itself is whitened: its noise does not know the branches' scale
    assert float(np.max(np.abs(c3["h"].real * np.sqrt(3.7) - base["h"].real) / np.maximum(base["h"].real, 1e-300))) < 1e-15


def test_live_branch_rule():
    tx, rx, h, ow2 = (np.array(a) for a in cb.parity_set(3))
    h[1, 4, 17] = np.nan                    # a NaN in an h row
    h[2, 5, dm.DC] = np.inf                 # entry 26 is outside V: the branch stays live
    ow2[0, 6], ow2[1, 7], ow2[2, 8], ow2[0, 9] = 0.0, -1.0, np.inf, np.nan
    h[:, 10, 3] = np.nan                    # no live branch
    rx[1, 11, 2, 40] = np.nan               # a NaN sample of a live branch
    c = cb.combine(rx, h, ow2, np.float64)
    live = c["live"]
    dead = {(1, 4), (0, 6), (1, 7), (2, 8), (0, 9), (0, 10), (1, 10), (2, 10)}
    assert {(a, f) for a in range(3) for f in range(cb.PARITY_B) if not live[a, f]} == dead
    # a dead branch: the call on the live ones alone, bit for bit
    for f, gone in ((4, 1), (6, 0), (7, 1), (8, 2), (9, 0)):
        keep = [a for a in range(3) if a != gone]
        alone = cb.combine(rx[keep][:, f:f + 1], h[keep][:, f:f + 1], ow2[keep][:, f:f + 1], np.float64)
        assert np.array_equal(c["rx"][f], alone["rx"][0]) and np.array_equal(c["h"][f], alone["h"][0]), f
    assert np.isnan(c["rx"][10]).all() and np.isnan(c["h"][10]).all()
    bad = ~np.isfinite(c["rx"])
    assert int(bad.sum()) == 15 * 53 + 1 and bad[11, 2, 40]
    assert np.isfinite(c["h"][np.arange(cb.PARITY_B) != 10]).all()
    # nothing else moved
    clean = cb.combine(*cb.parity_set(3)[1:], np.float64)
    same = [f for f in range(cb.PARITY_B) if f not in (4, 6, 7, 8, 9, 10, 11)]
    assert np.array_equal(c["rx"][same], clean["rx"][same]) and np.array_equal(c["h"][same], clean["h"][same])
    assert np.array_equal(np.delete(c["rx"][11], 40, axis=1), np.delete(clean["rx"][11], 40, axis=1))
    # a zero gain: every branch's h[k] == 0 gives 0, not NaN
    h0 = np.array(cb.parity_set(2)[2])
    h0[:, 3, 9] = 0
    z = cb.combine(cb.parity_set(2)[1], h0, None, np.float64)
    assert np.all(z["rx"][3, :, 9] == 0) and z["h"][3, 9] == 0 and np.isfinite(z["rx"]).all()


@pytest.mark.parametrize("A", (1, 2, 4, 8))
def test_sync_share_model(A):
    metric, start, cfo = cb.sync_share_set(A)
    s, c = cb.sync_share(metric, start, cfo)
    for p in range(metric.shape[1]):
        live = [a for a in range(A) if np.isfinite(metric[a, p]) and start[a, p] >= 0]
        if not live:
            assert np.array_equal(s[:, p], start[:, p]) and np.array_equal(c[:, p], cfo[:, p])
            continue
        best = max(live, key=lambda a: (metric[a, p], -a))
        assert np.all(s[:, p] == start[best, p]) and np.all(c[:, p] == cfo[best, p]), p
    assert np.all(s[:, 3] == 10)            # a tie of every branch: the lowest
    assert np.all(s[:, 7] == -1)            # none live: untouched
    assert np.array_equal(s[:, 11], start[:, 11])
    if A > 1:
        assert np.all(s[:, 5] == 77) and np.all(s[:, 9] == 12)
    # each array alone: the start rule without cfo, and a finite metric alone without start
    assert np.array_equal(cb.sync_share(metric, start, None)[0], s)
    c_only = cb.sync_share(metric, None, cfo)[1]
    for p in range(metric.shape[1]):
        live = [a for a in range(A) if np.isfinite(metric[a, p])]
        want = cfo[max(live, key=lambda a: (metric[a, p], -a)), p] if live else cfo[:, p]
        assert np.all(c_only[:, p] == want), p


# ---------------------------------------------------------------- 4. the tolerances
def test_tolerances_are_derived_and_the_data_is_well_conditioned():
    g_rx, g_h = cb.measured_gaps()
    tol_rx, tol_h = cb.tolerances()
    print(f"fp64 vs long double: rx {g_rx:.2e} of the bound ({g_rx / U:.1f} u), h {g_h:.2e} of g ({g_h / U:.1f} u); "
          f"TOL_RX {tol_rx:.2e}, TOL_H {tol_h:.2e}")
    assert tol_rx == cb.MARGIN * g_rx and tol_h == cb.MARGIN * g_h and cb.MARGIN == 8
    # the gap is a handful of roundings, and the tolerance covers the arithmetic's worst case at A = 8 (30 u)
    assert U <= g_rx <= 10 * U and 0.5 * U <= g_h <= 6 * U
    assert tol_rx >= 30 * U and tol_h >= 12 * U
    for A in cb.PARITY_A:
        for weighted in (False, True):
            ld, f64 = cb.parity_model(A, weighted), cb.parity_model(A, weighted, np.float64)
            assert ld["rx"].dtype == np.clongdouble and f64["rx"].dtype == np.complex128
            assert ld["live"].all() and np.isfinite(ld["rx"]).all()
            assert np.all(ld["bound"][:, :, cb.V] > 0) and np.all(ld["g"][:, cb.V] > 0)
            # the bound is what the comparison has to be relative to: the branches' terms do not all align, and
            # somewhere the sum is a small part of them (measured: 0.09 at A = 2)
            if A > 1:
                assert float(np.min(np.abs(ld["rx"][:, :, cb.V]) / ld["bound"][:, :, cb.V])) < 0.5


# ---------------------------------------------------------------- 5. why it exists
def test_why_the_combiner_exists():
    """16-QAM on the drifting branches at 22 dB: two branches make fewer symbol errors than the better one alone,
    four fewer still, and with branches 6 dB apart the noise weights are worth having."""
    tx, rx, h, ow2 = cb.branches(4, seed=1)
    alone = [int(dm.demodulate(tx, rx[a], h[a], None, dm.QAM16, real=np.float64)["nerr"].sum()) for a in range(4)]

    def errors(A, rx, h, ow2):
        c = cb.combine(rx[:A], h[:A], None if ow2 is None else ow2[:A], np.float64)
        return int(dm.demodulate(tx, c["rx"], c["h"], None, dm.QAM16, real=np.float64)["nerr"].sum())
    two, four = errors(2, rx, h, ow2), errors(4, rx, h, ow2)
    print(f"symbol errors: branches alone {alone}, two combined {two}, four {four}")
    assert two < min(alone[:2]) and four < two
    tx, rx, h, ow2 = cb.branches(4, seed=1, snr_db=16.0, loss_db=6.0 * np.arange(4), tx=tx)
    weighted, flat = errors(4, rx, h, ow2), errors(4, rx, h, None)
    best = int(dm.demodulate(tx, rx[0], h[0], None, dm.QAM16, real=np.float64)["nerr"].sum())
    print(f"6 dB steps at 16 dB: weighted {weighted}, unweighted {flat}, the best branch alone {best}")
    assert weighted < flat and weighted < best


LINK_CASES = ((2, False), (2, True), (4, False), (4, True))
LINK_COUNTS = {(2, False, True): (0, [771, 954]), (2, True, True): (276, [1034, 43189]),
               (2, True, False): (2657, [1034, 43189]), (4, False, True): (0, [1598, 1635, 1204, 1539]),
               (4, True, True): (184, [1141, 43158, 47949, 47761]),
               (4, True, False): (47928, [1141, 43158, 47949, 47761])}


@pytest.mark.parametrize("A,unequal", LINK_CASES)
def test_link_model_seed(A, unequal):
    """LINK_SEED on the model transmitter's captures: every packet detected after sharing, no frame marginal in
    any chain, the counts the docstring states, and the relations tests/test_combine_gpu.py asserts of the device"""
    c = cb.link_set(A, unequal)
    cap = cb.link_capture(A, unequal)
    front = cb.link_front(cap)
    res = {}
    for weighted in ((True, False) if unequal else (True,)):
        r = cb.link_model(cap, c["bits"], weighted, front=front)
        assert not r["marginal"].any() and not r["branch_marginal"].any(), (weighted, "marginal frames")
        got = (int(r["combined"].sum()), [int(x) for x in r["branch"].sum(axis=1)])
        print(f"A = {A}, unequal {unequal}, weighted {weighted}: combined {got[0]}, branches {got[1]}")
        assert got == LINK_COUNTS[(A, unequal, weighted)]
        if weighted:
            assert got[0] < min(got[1])
        res[weighted] = got[0]
    if unequal:
        assert res[True] < res[False]
