"""Demodulation, the parts that need no GPU: the entry point exists (libwce.so,
include/wce.h, the Python mirror and its keywords), the model's Gray labels are
802.11's, the bounds the GPU tests hold the kernel to (tests/test_demod_gpu.py)
are ones an fp64 implementation can meet on data that makes the exact
comparisons legitimate, and a residual carrier offset does what the tracking is
there to undo.

With u = 2^-53:

TOL_EQ, relative to the frame's max |e|.  e = (rx / Hu) r.  The blend rounds 3
times and the quotient 7 (|Hu|^2 2, its reciprocal 1, each numerator 2, each
product 1), relative to |e|.  z_b: each of the 4 terms 6 u of its own modulus,
their sum 3 u more, so dz <= 9 u sum |term| <= 18 u |z| where |z| >= sum |term| / 2
(a data condition); the modulus and the division 2 u; the product e r 3 u.
|de| <~ (10 + 20 + 3) u |e| = 3.7e-15 |e|; TOL_EQ = 1e-13.

TOL_TH, absolute.  dtheta <= |dz| / |z| <= 18 u, and atan2 within 2 ulp of pi:
(18 + 8) u = 2.9e-15; TOL_TH = 1e-13.

TOL_EVM, relative.  evm^2 = num / den, num = sum |e - ref|^2, den = sum |ref|^2: an
error |de_k| <= 33 u |e_k| moves num by at most 2 sum |e_k - ref_k| 33 u |e_k| <=
66 u sqrt(num) sqrt(sum |e_k|^2) (Cauchy-Schwarz over the 720 symbols), so
d(evm) / evm = d(num) / (2 num) <= 33 u A / evm with A = sqrt(sum |e|^2 / den), which
is <= 1 + evm; plus 21 u for the sums (15 terms per lane, 6 butterfly steps) and
3 u for the quotient and the root.  The difference e - ref amplifies e's error by
1 / evm, so the smallest EVM of the data sets the bound: the largest
(33 A / evm + 24) u over every frame is checked to stay under TOL_EVM / 2;
TOL_EVM = 1e-12.

sym and nerr are compared exactly, which is legitimate only where no coordinate
sits within the arithmetic's error of a slicer boundary: every coordinate of
every set lies farther than MARGIN * scale = 1e-9 * scale from every boundary on the
long double model, no symbol and no frame left out.

Measured (fp64 model against long double; every set, every combination of
tracking, reference and blend): eq 6.1e-16 of max |e|, theta 2.1e-16 rad, evm
8.1e-16 relative; smallest margin 1.65e-6 scale, smallest |z| / sum |term| 0.995,
smallest EVM 0.0489 (the recorded frames, untracked, against tx), derived EVM
bound 7.8e-14.  The residual offset of 5e-5 cycles per sample on the matlab.mat
packet: EVM 0.04888 as recorded and untracked, 0.04947 tracked (the pilots'
noise: 1.012); rotated 0.19628 untracked, 0.05025 tracked: 1.016 of the unrotated
tracked EVM, and the untracked one 3.91 times the tracked."""
import inspect
import os
import re

import numpy as np
import pytest

import demod_model as dm

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -53

def test_symbol_exported_and_declared(wce):
    lib = wce.load()
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "wce.h")).read(), flags=re.S)
    assert hasattr(lib, "wce_demodulate")
    assert re.search(r"\bint\s+wce_demodulate\s*\(", hdr)
    params = re.search(r"\bwce_demodulate\s*\(([^)]*)\)", hdr).group(1).split(",")
    assert len(params) == len(wce.wce.ABI["wce_demodulate"]) == 5
    for name, value in (("WCE_MOD_BPSK", 1), ("WCE_MOD_QPSK", 2), ("WCE_MOD_QAM16", 4), ("WCE_MOD_QAM64", 6)):
        assert re.search(r"\b%s\s*=\s*%d\b" % (name, value), hdr), name
    assert (wce.MOD_BPSK, wce.MOD_QPSK, wce.MOD_QAM16, wce.MOD_QAM64) == (1, 2, 4, 6) == dm.MODS
    assert (wce.DEMOD_TRACK, wce.DEMOD_REF_TX) == (1, 2)
    assert re.search(r"#define\s+WCE_DEMOD_TRACK\s+\(1u << 0\)", hdr)
    assert re.search(r"#define\s+WCE_DEMOD_REF_TX\s+\(1u << 1\)", hdr)
    # the two structures, field for field (x86-64: 40 and 72 bytes)
    import ctypes
    assert [f[0] for f in wce.wce.Demod._fields_] == ["h", "h_lt", "h_stride", "modulation", "flags", "scale"]
    assert [f[0] for f in wce.wce.DemodOut._fields_] == ["eq", "sym", "theta", "evm", "nerr", "eq_frame_stride",
                                                         "eq_block_stride", "sym_frame_stride", "sym_block_stride"]
    assert ctypes.sizeof(wce.wce.Demod) == 40 and ctypes.sizeof(wce.wce.DemodOut) == 72
    for struct in ("wce_demod", "wce_demod_out"):
        assert re.search(r"\}\s*%s\s*;" % struct, hdr), struct


def test_python_keywords(wce):
    C = wce.Context
    common = {"h_lt": None, "modulation": wce.MOD_BPSK, "scale": 8.8753, "track": True, "ref_tx": True}
    outs = {"eq": None, "sym": None, "theta": None, "evm": None, "nerr": None, "stream": None}
    chain = {"demod_source": None, "modulation": wce.MOD_BPSK, "scale": 8.8753, "track": True}
    for fn, kws in ((C.demodulate, {**common, "h_stride": wce.NSC, **outs}), (C.demodulate_host, common),
                    (C.receive_host, chain), (C.receive_capture_host, chain)):
        p = inspect.signature(fn).parameters
        for k, default in kws.items():
            assert k in p and p[k].default == default, (fn.__name__, k)
    assert list(inspect.signature(C.demodulate).parameters)[1:3] == ["frames", "h"]
    assert list(inspect.signature(C.demodulate_host).parameters)[1:4] == ["tx", "rx", "h"]


# IEEE 802.11-2020 Tables 17-9 and 17-10 (16- and 64-QAM): input bits, b0 first, to the I (or Q) level
QAM16_TABLE = {"00": -3, "01": -1, "11": 1, "10": 3}
QAM64_TABLE = {"000": -7, "001": -5, "011": -3, "010": -1, "110": 1, "111": 3, "101": 5, "100": 7}


@pytest.mark.parametrize("mod,table", [(dm.QAM16, QAM16_TABLE), (dm.QAM64, QAM64_TABLE)])
def test_gray_labels_are_802_11(mod, table):
    nb = mod // 2
    d = float(dm.spacing(mod, dm.SCALE))
    for bi, li in table.items():
        for bq, lq in table.items():
            e = np.zeros((1, 1, dm.N), complex)
            e[0, 0, dm.DATA] = (li + 1j * lq) * d * (1 + 1e-3)          # a little off the point itself
            sym, dec, _ = dm.slice_points(e, mod, dm.SCALE)
            assert np.all(sym[0, 0, dm.DATA] == int(bi + bq, 2)), (bi, bq)   # b0 is the label's top bit
            assert np.allclose(np.asarray(dec[0, 0, dm.DATA], complex), (li + 1j * lq) * d, rtol=1e-15)
            assert format(int(sym[0, 0, dm.DATA[0]]), "0%db" % mod) == bi + bq
    assert nb == len(next(iter(table)))
    # BPSK and QPSK: one bit per axis, 0 -> -1 (Tables 17-7 and 17-8); the pilots are BPSK whatever the data are
    e = np.zeros((1, 1, dm.N), complex)
    e[0, 0, :] = (-0.4 + 0.3j) * dm.SCALE
    assert np.all(dm.slice_points(e, dm.QPSK, dm.SCALE)[0][0, 0, dm.DATA] == 0b01)
    assert np.all(dm.slice_points(e, dm.BPSK, dm.SCALE)[0][0, 0, dm.DATA] == 0)
    for mod_ in dm.MODS:
        sym, dec, _ = dm.slice_points(-e, mod_, dm.SCALE)
        assert np.all(sym[0, 0, list(dm.PILOTS)] == 1) and sym[0, 0, dm.DC] == 0
        assert np.all(np.asarray(dec[0, 0, list(dm.PILOTS)], complex) == dm.SCALE)
    # clamping: far outside the constellation is the outermost level
    e[0, 0, :] = (100 - 100j) * dm.SCALE
    assert np.all(dm.slice_points(e, dm.QAM64, dm.SCALE)[0][0, 0, dm.DATA] == (0b100 << 3 | 0b000))
    e[0, 0, 3] = np.nan
    assert dm.slice_points(e, dm.QAM64, dm.SCALE)[0][0, 0, 3] == dm.BAD


def _combos():
    return [(t, r, b) for t in (True, False) for r in (True, False) for b in (True, False)]


def test_tolerances_are_reachable_and_data_is_well_conditioned(golden):
    assert 33 * U < dm.TOL_EQ / 2 and 26 * U < dm.TOL_TH / 2
    worst = {"eq": 0.0, "theta": 0.0, "evm": 0.0}
    margin, zratio, evm_min, bound, errs64 = np.inf, np.inf, np.inf, 0.0, 0
    for name, (tx, rx, h, h_lt, mod) in dm.all_sets(golden).items():
        for track, ref_tx, bl in _combos():
            kw = dict(h_lt=h_lt if bl else None, modulation=mod, track=track, ref_tx=ref_tx)
            ld, f64 = dm.demodulate(tx, rx, h, **kw), dm.demodulate(tx, rx, h, real=np.float64, **kw)
            assert ld["eq"].dtype == np.clongdouble and f64["eq"].dtype == np.complex128
            err = {"eq": float(dm.relmax_frames(f64["eq"], ld["eq"]).max()),
                   "theta": float(np.max(np.abs(f64["theta"] - ld["theta"]))),
                   "evm": float(np.max(np.abs(f64["evm"] - ld["evm"]) / ld["evm"]))}
            tol = {"eq": dm.TOL_EQ, "theta": dm.TOL_TH, "evm": dm.TOL_EVM}
            for k in err:
                assert 2 * err[k] <= tol[k], (name, track, ref_tx, bl, k, err[k])
                worst[k] = max(worst[k], err[k])
            # the data conditions, on the long double model: no symbol and no frame left out
            mg = float(np.min(ld["margin"])) / dm.SCALE
            assert mg > dm.MARGIN, (name, track, ref_tx, bl, mg)
            assert np.array_equal(f64["sym"], ld["sym"]) and np.array_equal(f64["nerr"], ld["nerr"])
            assert not np.any(ld["sym"] == dm.BAD)
            if track:
                zr = float(np.min(np.abs(ld["z"]) / ld["zabs"]))
                assert zr >= 0.5, (name, zr)
                assert float(np.min(np.pi - np.abs(ld["theta"]))) > 1e-9, name
                zratio = min(zratio, zr)
            else:
                assert not np.any(ld["theta"])
            ev = float(np.min(ld["evm"]))
            assert ev >= 0.01, (name, track, ref_tx, bl, ev)
            ed = ld["eq"][:, :, dm.DATA]
            ref = (np.asarray(tx) if ref_tx else dm.slice_points(ld["eq"], mod, dm.SCALE)[1])[:, :, dm.DATA]
            A = np.sqrt(np.sum(np.abs(ed) ** 2, axis=(1, 2)) / np.sum(np.abs(ref) ** 2, axis=(1, 2)))
            assert np.all(A <= 1 + ld["evm"] + 1e-15)
            margin, evm_min = min(margin, mg), min(evm_min, ev)
            bound = max(bound, float(np.max(33 * A / ld["evm"] + 24)) * U)
            if mod == dm.QAM64 and track and bl:
                errs64 = max(errs64, int(ld["nerr"].max()))
        print(f"{name}: evm {float(np.min(ld['evm'])):.4f} .. {float(np.max(ld['evm'])):.4f}, "
              f"nerr up to {int(ld['nerr'].max())}")
    print(f"fp64 vs long double: eq {worst['eq']:.2e}, theta {worst['theta']:.2e}, evm {worst['evm']:.2e}; "
          f"margin {margin:.2e} scale, |z|/sum|term| {zratio:.3f}, smallest evm {evm_min:.4f}, "
          f"derived evm bound {bound:.2e}")
    assert bound <= dm.TOL_EVM / 2
    assert errs64 > 0                                    # 64-QAM at 25 dB does make symbol errors


def test_phase_set_wraps(golden):
    """the wrap test's rotations carry theta across +-pi and leave it well conditioned"""
    tx, rx, h, h_lt, rot = dm.phase_set()
    a = dm.demodulate(tx, rx, h, h_lt, dm.QPSK)
    b = dm.demodulate(tx, rot, h, h_lt, dm.QPSK)
    assert np.max(np.abs(dm.wrap(b["theta"] - a["theta"] - dm.PHI[None, :]))) < 1e-15
    assert np.any(np.abs(b["theta"] - a["theta"] - dm.PHI[None, :]) > 6)      # some did wrap
    assert np.any(b["theta"] > 3.0) and np.any(b["theta"] < -3.0)
    assert np.array_equal(a["sym"], b["sym"]) and float(np.min(b["margin"])) > dm.MARGIN * dm.SCALE
    assert float(dm.relmax_frames(b["eq"], a["eq"]).max()) < 1e-15
    assert float(np.min(np.abs(b["z"]) / b["zabs"])) >= 0.5


def test_model_rules():
    """zero pilots, non-finite symbols and the reference switch in the model itself"""
    tx, rx, h, h_lt = dm.synthetic(dm.QAM16, 3, seed=1)
    base = dm.demodulate(tx, rx, h, h_lt, dm.QAM16)
    off = dm.demodulate(tx, rx, h, h_lt, dm.QAM16, track=False)
    z = rx.copy()
    z[1, 4, list(dm.PILOTS)] = 0
    r = dm.demodulate(tx, z, h, h_lt, dm.QAM16)
    assert r["theta"][1, 4] == 0 and np.array_equal(r["eq"][1, 4, dm.DATA], off["eq"][1, 4, dm.DATA])
    assert np.array_equal(np.delete(r["theta"], 1, 0), np.delete(base["theta"], 1, 0))
    bad = rx.copy()
    bad[2, 7, 11] = np.inf
    r = dm.demodulate(tx, bad, h, h_lt, dm.QAM16)
    assert r["sym"][2, 7, 11] == dm.BAD and np.isnan(r["evm"][2]) and r["nerr"][2] >= 1
    assert np.array_equal(r["evm"][:2], base["evm"][:2]) and np.array_equal(r["sym"][:2], base["sym"][:2])
    dec = dm.demodulate(tx, rx, h, h_lt, dm.QAM16, ref_tx=False)
    assert np.array_equal(dec["eq"], base["eq"]) and np.array_equal(dec["nerr"], base["nerr"])
    clean = base["nerr"] == 0                            # no symbol error: the decided points are tx
    assert clean.any() and np.allclose(np.asarray(dec["evm"][clean], float), np.asarray(base["evm"][clean], float),
                                       rtol=1e-12)
    assert np.all(base["eq"][:, :, dm.DC] == 0) and np.all(base["sym"][:, :, dm.DC] == 0)


def test_why_tracking_exists(golden):
    """A residual carrier offset of 5e-5 cycles per sample (500 Hz at 10 MHz) on the recorded packet, through
    the model's chain (front end, LT_LS, PS_Linear, blend), EVM against tx.  Tracked, the EVM stays within 1.1 of
    the unrotated packet's tracked EVM (measured 1.016: what is left is the turn inside a block and on the
    estimates); untracked it is at least twice the tracked one (measured 3.91)."""
    m = golden["matlab"]
    evm = {}
    for name, (lp, pk) in (("as recorded", (m["rx_lptot"], m["rx_packet"])), ("rotated", dm.rotated_packet(m))):
        tx, rx, h, h_lt = dm.chain(m, lp, pk)
        for track in (True, False):
            r = dm.demodulate(tx, rx, h, h_lt, dm.BPSK, track=track)
            evm[name, track] = float(r["evm"][0])
            assert r["nerr"][0] == 0
    print({k: round(v, 5) for k, v in evm.items()})
    print(f"tracked rotated / tracked recorded {evm['rotated', True] / evm['as recorded', True]:.4f}, "
          f"untracked / tracked {evm['rotated', False] / evm['rotated', True]:.3f}, "
          f"cost of tracking with no residual {evm['as recorded', True] / evm['as recorded', False]:.4f}")
    assert evm["rotated", True] <= 1.1 * evm["as recorded", True]
    assert evm["rotated", False] >= 2 * evm["rotated", True]
    assert abs(evm["as recorded", False] - 0.0489) < 5e-4      # the issue's figure for the packet as recorded
