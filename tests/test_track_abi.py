"""Per-block tracking, the parts that need no GPU: the entry points exist
(libwce.so, include/wce.h, the Python mirrors and their keywords), the model
keeps the rules of the definition, the bounds the GPU tests hold the kernel to
(tests/test_track_gpu.py) are ones an fp64 implementation can meet on data that
makes the exact comparisons legitimate, and tracking does what it is there for.

The bounds.  A block of the tracker is a block of wce_demodulate (TOL_EQ's 33 u of
|e|, u = 2^-53) on an estimate that carries the rounding of the blocks before it:
G = rx r / x^ rounds like e (about 33 u), the window sum of up to 9 terms adds 9 u,
the update 3 u, and H_{b+1} = (1 - mu) H_b + mu S_b does not amplify what H_b
carries, so after 15 blocks H is within about 15 * 45 u = 7.5e-14 of its modulus in
the worst case and random rounding stays far below that; e inherits it through
1 / H, amplified where |H| is small against the frame's largest (the drifting sets
fade by up to 25 dB, and with mu = 1, beta = 0 a wrong decision can leave an H_b close
to 0).  The tolerances are set from the measured deviation of the fp64 model from the
long double model (below), each at least 37 times it:

    TOL_EQ_T = 1e-12 of the frame's max |e|, TOL_H_T = 1e-13 of the frame's max |H|,
    TOL_TH = 1e-13 rad (demod_model's), TOL_EVM_T = 1e-11 relative,

and the test below holds the fp64 model to a tenth of each on every set and every
combination the GPU test runs.

sym and nerr are compared exactly, which is legitimate only where no coordinate
sits within the arithmetic's error of a slicer boundary: every sliced coordinate
of every block of every set and combination lies farther than dm.MARGIN * scale
from every boundary on the long double model, no frame left out.  A decision
that fell the other way would also change every later H of that frame.

Measured with the committed generator (fp64 model against long double; the four
sets, (mu, beta) in (0.5, 2), (1, 0), (0.25, 4), the phase flag on and off, tx known
and decided): eq 2.7e-14 of max |e| and evm 2.6e-14 relative (both QPSK, mu = 1, beta =
0, no phase flag, decided tx; at mu = 0.5, beta = 2 eq 6.3e-15), h_blocks 6.9e-16 of max
|H|, theta 6.9e-16 rad, labels identical, smallest margin 1.40e-7 scale (2.06e-6 at
mu = 0.5, beta = 2), smallest |z| / sum |term| 0.248.
Symbol errors over 67 x 720 data symbols at rho = 0.995 (static / tracked mu = 0.5,
beta = 2 / known tx): BPSK 10 dB 2287 / 1526 / 1348, QPSK 15 dB 4542 / 3307 / 2395,
16-QAM 22 dB 10784 / 6424 / 4619, 64-QAM 28 dB 25701 / 18497 / 12779: ratios 0.67,
0.73, 0.60, 0.72.  The coded 16-QAM rate 1/2 set of the chain test: 945 bit errors
tracked, 3126 static."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

import demod_model as dm
import track_model as tm

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------- 1. the interface
def test_symbols_exported_and_declared(wce):
    lib = wce.load()
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "wce.h")).read(), flags=re.S)
    for name, nargs in (("wce_track_demodulate", 5), ("wce_soft_demap_blocks", 14)):
        assert hasattr(lib, name), name
        assert re.search(r"\bint\s+%s\s*\(" % name, hdr), name
        params = re.search(r"\b%s\s*\(([^)]*)\)" % name, hdr).group(1).split(",")
        assert len(params) == len(wce.wce.ABI[name]) == nargs, name
    assert (wce.TRACK_PHASE, wce.TRACK_REF_TX, wce.TRACK_KNOWN_TX) == (1, 2, 4)
    for name, bit in (("WCE_TRACK_PHASE", 0), ("WCE_TRACK_REF_TX", 1), ("WCE_TRACK_KNOWN_TX", 2)):
        assert re.search(r"#define\s+%s\s+\(1u << %d\)" % (name, bit), hdr), name
    # the two structures, field for field and in the header's order (x86-64: 48 and 112 bytes)
    W = wce.wce
    assert [f[0] for f in W.Track._fields_] == ["h", "h_stride", "modulation", "flags", "scale", "mu", "beta"]
    assert [f[0] for f in W.TrackOut._fields_] == [
        "eq", "sym", "theta", "evm", "nerr", "eq_frame_stride", "eq_block_stride", "sym_frame_stride",
        "sym_block_stride", "h_blocks", "hb_frame_stride", "hb_block_stride", "h_last", "h_last_stride"]
    assert ctypes.sizeof(W.Track) == 48 and ctypes.sizeof(W.TrackOut) == 112
    for struct, cls in (("wce_track", W.Track), ("wce_track_out", W.TrackOut)):
        body = re.search(r"typedef\s+struct\s*\{([^}]*)\}\s*%s\s*;" % struct, hdr)
        assert body, struct
        names = re.findall(r"\b(\w+)\s*(?=[,;])", body.group(1))
        assert names == [f[0] for f in cls._fields_], struct
    assert wce.Track is W.Track and wce.TrackOut is W.TrackOut


def test_python_keywords(wce):
    C = wce.Context
    common = {"modulation": wce.MOD_BPSK, "scale": 8.8753, "phase": True, "ref_tx": True, "known_tx": False}
    outs = {k: None for k in ("eq", "sym", "theta", "evm", "nerr", "h_blocks", "h_last", "stream")}
    for fn, kws in ((C.track_demodulate, {**common, "h_stride": wce.NSC, **outs}),
                    (C.track_demodulate_host, {**common, "mu": 0.5, "beta": 2}),
                    (C.track_decode_host, {"modulation": wce.MOD_BPSK, "rate": wce.RATE_1_2, "mu": 0.5, "beta": 2,
                                           "ref_bits": None}),
                    (C.soft_demap_blocks, {"modulation": wce.MOD_BPSK, "scale": 8.8753, "llr": None, "stream": None}),
                    (C.receive_host, {"tracker": None})):
        p = inspect.signature(fn).parameters
        for k, default in kws.items():
            assert k in p and p[k].default == default, (fn.__name__, k)
    assert list(inspect.signature(C.track_demodulate).parameters)[1:5] == ["frames", "h", "mu", "beta"]
    assert list(inspect.signature(C.track_demodulate_host).parameters)[1:4] == ["tx", "rx", "h"]
    assert list(inspect.signature(C.track_decode_host).parameters)[1:6] == ["tx", "rx", "h", "modulation", "rate"]
    assert list(inspect.signature(C.soft_demap_blocks).parameters)[1:4] == ["eq", "h_blocks", "n_frames"]


# ---------------------------------------------------------------- 2. the model's rules
@pytest.mark.parametrize("mod", dm.MODS)
def test_mu_zero_is_the_static_demodulator(mod):
    tx, rx, h = tm.drifting_set(mod)
    for phase in (True, False):
        a = tm.track(tx, rx, h, mod, 0.0, 3, phase=phase)
        d = dm.demodulate(tx, rx, h, None, mod, track=phase)
        for k in ("eq", "sym", "theta", "evm", "nerr"):
            assert np.array_equal(a[k], d[k]), (phase, k)
        assert np.array_equal(a["h_blocks"], np.repeat(np.asarray(h, np.clongdouble)[:, None], dm.NBLK, 1))
        assert np.array_equal(a["h_last"], np.asarray(h, np.clongdouble))


def test_full_weight_without_smoothing_is_the_instantaneous_estimate():
    tx, rx, h = (a[:5] for a in tm.drifting_set(dm.QAM16))
    r = tm.track(tx, rx, h, dm.QAM16, 1.0, 0, known_tx=True)
    rot = np.exp(-1j * r["theta"])[:, :, None]
    want = np.asarray(rx, np.clongdouble) * rot / np.where(tx == 0, 1, tx)
    nxt = np.concatenate([r["h_blocks"][:, 1:], r["h_last"][:, None]], axis=1)
    assert float(np.max(np.abs(nxt[:, :, tm.V] - want[:, :, tm.V]) / np.abs(want[:, :, tm.V]))) < 1e-17
    # entry 26 is carried from h, and block 0 is equalized with h itself
    assert np.all(nxt[:, :, dm.DC] == np.asarray(h)[:, None, dm.DC])
    assert np.array_equal(r["h_blocks"][:, 0], np.asarray(h, np.clongdouble))
    # decided symbols that are right give the same estimate as the known ones
    d = tm.track(tx, rx, h, dm.QAM16, 1.0, 0)
    # (with mu = 1 and beta = 0, H_15[k] depends on block 14's symbol k and its rotor alone)
    right = d["sym"][:, 14] == dm.slice_points(tx, dm.QAM16, dm.SCALE)[0][:, 14]
    right[:, dm.DC] = False
    assert right.any() and not right[:, dm.DATA].all()
    assert float(np.max(np.abs(d["h_last"][right] - want[:, 14][right]) / np.abs(want[:, 14][right]))) < 1e-12


def test_window_sizes():
    want = {0: {0: 1, 22: 1, 23: 1, 24: 1, 25: 1, 27: 1, 28: 1, 29: 1, 30: 1, 52: 1},
            1: {0: 2, 22: 3, 23: 3, 24: 3, 25: 2, 27: 2, 28: 3, 29: 3, 30: 3, 52: 2},
            2: {0: 3, 22: 5, 23: 5, 24: 4, 25: 4, 27: 4, 28: 4, 29: 5, 30: 5, 52: 3},
            3: {0: 4, 22: 7, 23: 6, 24: 6, 25: 6, 27: 6, 28: 6, 29: 6, 30: 7, 52: 4},
            4: {0: 5, 22: 8, 23: 8, 24: 8, 25: 8, 27: 8, 28: 8, 29: 8, 30: 8, 52: 5}}
    for beta, sizes in want.items():
        W, cnt = tm.window(beta)
        for k, n in sizes.items():
            assert cnt[k] == n, (beta, k)
        assert cnt[dm.DC] == 0 and not W[:, dm.DC].any() and not W[dm.DC].any()
        # the mean of a ramp over a window that is symmetric in index space and does not touch DC is the ramp
        G = np.arange(dm.N) + 1j * (dm.N - np.arange(dm.N))
        S = tm.smooth(G[None], beta)[0]
        inner = [k for k in range(beta, dm.N - beta) if abs(k - dm.DC) > beta]
        assert np.all(S[inner] == G[inner]) and S[dm.DC] == 0
        if beta:
            assert S[dm.DC - 1] != G[dm.DC - 1] and S[0] != G[0]


# ---------------------------------------------------------------- 3. the tolerances and the data
def test_tolerances_are_reachable_and_data_is_well_conditioned():
    worst = {"eq": 0.0, "h": 0.0, "theta": 0.0, "evm": 0.0}
    where = {}
    tol = {"eq": tm.TOL_EQ_T, "h": tm.TOL_H_T, "theta": tm.TOL_TH, "evm": tm.TOL_EVM_T}
    margin = zratio = np.inf
    for mod, _ in tm.SETS:
        for mu, beta, phase, known in tm.COMBOS:
            ld = tm.model(mod, mu, beta, phase, known)
            f64 = tm.model(mod, mu, beta, phase, known, real=np.float64)
            assert ld["eq"].dtype == np.clongdouble and f64["eq"].dtype == np.complex128
            hl, h64 = (np.concatenate([r["h_blocks"], r["h_last"][:, None]], axis=1) for r in (ld, f64))
            err = {"eq": float(dm.relmax_frames(f64["eq"], ld["eq"]).max()),
                   "h": float(dm.relmax_frames(h64, hl).max()),
                   "theta": float(np.max(np.abs(f64["theta"] - ld["theta"]))),
                   "evm": float(np.max(np.abs(f64["evm"] - ld["evm"]) / ld["evm"]))}
            for k in err:
                assert 10 * err[k] <= tol[k], (mod, mu, beta, phase, known, k, err[k])
                if err[k] > worst[k]:
                    worst[k], where[k] = err[k], (mod, mu, beta, phase, known)
            mg = float(np.min(ld["margin"])) / dm.SCALE
            assert mg > dm.MARGIN, (mod, mu, beta, phase, known, mg)
            margin = min(margin, mg)
            assert np.array_equal(f64["sym"], ld["sym"]) and np.array_equal(f64["nerr"], ld["nerr"])
            assert not np.any(ld["sym"] == dm.BAD)
            if phase:
                # dtheta <= 9 u sum |term| / |z| (tests/test_demod_abi.py): at 10 dB the pilots of a faded block
                # cancel further than demod_model's sets do; down to a tenth that is 90 u = 1e-14, a tenth of TOL_TH
                zratio = min(zratio, float(np.min(np.abs(ld["z"]) / ld["zabs"])))
                assert zratio >= 0.1
                assert float(np.min(np.pi - np.abs(ld["theta"]))) > 1e-9
            else:
                assert not np.any(ld["theta"])
            assert float(np.min(ld["evm"])) >= 0.01
    print(f"fp64 vs long double: eq {worst['eq']:.2e}, h_blocks {worst['h']:.2e}, theta {worst['theta']:.2e}, "
          f"evm {worst['evm']:.2e}; margin {margin:.2e} scale, |z|/sum|term| {zratio:.3f}; worst at {where}")
    # the chain test's coded set is as well conditioned
    s = tm.coded_set()
    assert float(np.min(tm.track(s["tx"], s["rx"], s["h"], dm.QAM16)["margin"])) > dm.MARGIN * dm.SCALE


# ---------------------------------------------------------------- 4. why it exists
def test_why_the_tracker_exists():
    """On a channel that decorrelates by rho = 0.995 per block the tracked receiver (mu = 0.5, beta = 2) makes at
    most 0.8 of the static receiver's symbol errors on every set (measured 0.67, 0.73, 0.60, 0.72), and the known-tx
    bound lies below both."""
    for mod, _ in tm.SETS:
        static, tracked, known = tm.symbol_errors(*tm.drifting_set(mod), mod)
        print(f"{mod} bits: static {static}, tracked {tracked} ({tracked / static:.2f}), known tx {known}")
        assert tracked <= 0.8 * static, mod
        assert known < tracked and known < static, mod
    tracked, static = tm.decode_chain(tm.coded_set())
    print(f"coded 16-QAM rate 1/2: {int(tracked.sum())} bit errors tracked, {int(static.sum())} static")
    assert tracked.sum() < static.sum()
