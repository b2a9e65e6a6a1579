"""The short training field, the parts that need no GPU: both entry points exist
(libwce.so, include/wce.h, the Python mirror and its keywords), every refusal
that needs no device, the host's table of the field, and the bounds the GPU
tests hold the kernel to (tests/test_stf_gpu.py) with the conditions that make
their exact comparisons legitimate.  u = 2^-53 throughout.

TOL_MS.  Ms = |P|^2 / (A B) <= 1.  P is a 128-term complex sum of products: an
error of (128 + 2) u against sum |q|, and sum |q| <= sqrt(A B) by Cauchy-Schwarz,
as |P| is: |d |P|^2| <= 2 * 130 u A B.  A and B, 128 terms of two squares each,
256 u relative apiece; product, modulus and quotient 4 u more.
|dMs| <= (260 + 512 + 4) u = 8.6e-14; TOL_MS = 2e-13.

e_c = arg P / (32 pi).  |dP| / |P| <= 130 u sum |q| / |P| <= 130 u / sqrt(Ms): for a
detected frame, Ms >= threshold_stf, about 130 u / sqrt(threshold_stf) radians.
Ml is written for every frame, detected or not, so the bound that counts is the
one at the smallest Ms any window here has, MS_MIN = 1e-4 (asserted; the all-zero
window has P = 0 and e_c = 0 exactly on both sides): 130 u / 1e-2 plus atan2's
own 8 u pi, over 32 pi: |de_c| <= 1.5e-14 cycles per sample, half TOL_EC = 3.2e-14.

TOL_ML.  wce_front_end_sync's bound on M, 4.4e-14 (tests/test_sync_abi.py), the
rotor's 10 u on each sample (20 u on M), and M's sensitivity to e_c: the turned
template moves c by |dc| <= 2 pi |de_c| sum n |x| |ltf| <= 2 pi 63 |de_c| sqrt(El E),
relative to each of the two factors of M <= 1, so |dM| <= 2 * 2 pi 63 |de_c| =
792 * 1.5e-14 = 1.2e-11.  Together 1.2e-11; TOL_ML = 5e-11, a twentieth of MIN_GAP.

TOL_CFO.  cfo = e_f + k / 64 with k = rint((e_c - e_f) 64) an integer that both
sides agree on (the fraction stays 1e-6 away from 1/2, asserted).  e_f = arg c /
(128 pi), c a 64-term sum whose modulus is at least 0.1 of its terms' (asserted):
(64 + 2) u / 0.1 + atan2's 8 u pi radians, over 128 pi, is 1.7 u; the last
addition rounds by u / 32 at most.  |dcfo| <= 1.8 u = 2.0e-16; TOL_CFO = 1e-15.

start is compared exactly: every set's best lag of M leads by more than
sync_model.MIN_GAP = 1e-9, and every Ms and Ml is at least 1e-6 from its
threshold, no frame left out.  d_s is not an output, and on a noise-free short
field |P|^2 ties from lag to lag up to rounding: at every lag within 1e-9
(relative) of the maximum, Ms and e_c agree within a tenth of TOL_MS and TOL_EC.

Measured (this file, fp64 model against long double, every set): Ms within
2.7e-15, Ml 1.4e-15, cfo 2.6e-18; smallest gap 1.7e-06 (L=191 B=777), smallest Ms
8.2e-04, the two-copy sum's modulus at least 0.75 of its terms', the unwrapping's
fraction at least 0.44 from 1/2; spread on the plateau below 1e-18 (the tiled
period is periodic bit for bit); the table within 0.35 ulp."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

import stf_model as st
import sync_model as sm
import tx_model as tm

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMS = {"wce_front_end_sync_stf": 14, "wce_short_field": 6}
EINVAL = -1
LD = np.longdouble
SHAPES = st.BASE_SHAPES + [(L, st.TILE_B) for L in st.tile_lengths(432, 448)]


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
    for fn, kws in ((C.front_end_sync_stf, {"backoff": 0, "start": None, "cfo": None, "metric_stf": None,
                                            "metric_ltf": None, "capture_stride": None, "stream": None}),
                    (C.transmit_host, {"stf": False}),
                    (C.link_host, {"stf": False, "stf_threshold": 0.25}),
                    (C.receive_capture_host, {"stf": False, "stf_threshold": 0.25})):
        p = inspect.signature(fn).parameters
        for k, default in kws.items():
            assert k in p and p[k].default == default, (fn.__name__, k)
    names = list(inspect.signature(C.front_end_sync_stf).parameters)
    assert names[1:7] == ["capture", "n_frames", "capture_len", "ltf", "threshold_stf", "threshold_ltf"]
    assert "1,648" in C.link_host.__doc__
    assert hasattr(C, "short_field")


def _sync_stf_base():
    return dict(capture=0x1000, capture_stride=488, capture_len=488, n_frames=3, ltf=0x1000, threshold_stf=0.25,
                threshold_ltf=0.25, backoff=0, start=0x1000, cfo=0x1000, metric_stf=0x1000, metric_ltf=None)


SYNC_REFUSALS = [({"capture_len": 143, "capture_stride": 143}, "capture_len"),
                 ({"capture_len": 2 ** 31, "capture_stride": 2 ** 31}, "capture_len"),
                 ({"capture_stride": 487}, "capture_stride <"),
                 ({"threshold_stf": -0.01}, "threshold_stf"), ({"threshold_stf": 1.01}, "threshold_stf"),
                 ({"threshold_stf": float("nan")}, "threshold_stf"), ({"threshold_ltf": float("inf")}, "threshold_ltf"),
                 ({"threshold_ltf": -1e-300}, "threshold_ltf"), ({"threshold_ltf": float("nan")}, "threshold_ltf"),
                 ({"backoff": -1}, "backoff"), ({"backoff": 32}, "backoff"),
                 ({"start": None}, "start"), ({"start": 0x1002}, "4-byte"),
                 ({"cfo": None}, "cfo"), ({"cfo": 0x1004}, "8-byte"),
                 ({"metric_stf": 0x1004}, "8-byte"), ({"metric_ltf": 0x1004}, "8-byte"),
                 ({"ltf": None}, "ltf"), ({"ltf": 0x1008}, "16-byte"),
                 ({"capture": None}, "capture"), ({"capture": 0x1008}, "16-byte"),
                 ({"n_frames": -1}, "n_frames")]
FIELD_REFUSALS = [({"wave": None}, "wave"), ({"wave": 0x1008}, "16-byte"), ({"wave_stride": 159}, "wave_stride"),
                  ({"amplitude": float("nan")}, "amplitude"), ({"amplitude": float("inf")}, "amplitude"),
                  ({"n_frames": -1}, "n_frames")]


def test_refusals_before_the_ctx_is_touched(wce):
    """every WCE_EINVAL of the header, with an opaque non-NULL ctx and opaque pointers: nothing is launched"""
    lib = wce.load()
    h = 0x10
    for ch, text in SYNC_REFUSALS:
        kw = {**_sync_stf_base(), **ch}
        assert lib.wce_front_end_sync_stf(h, *kw.values(), None) == EINVAL, ch
        assert text in lib.wce_last_error().decode(), (ch, lib.wce_last_error())
    assert lib.wce_front_end_sync_stf(None, *_sync_stf_base().values(), None) == EINVAL
    assert "null ctx" in lib.wce_last_error().decode()
    assert lib.wce_front_end_sync_stf(h, *{**_sync_stf_base(), "n_frames": 0}.values(), None) == 0
    base = dict(amplitude=1.0, wave=0x1000, wave_stride=160, n_frames=3)
    for ch, text in FIELD_REFUSALS:
        kw = {**base, **ch}
        assert lib.wce_short_field(h, *kw.values(), None) == EINVAL, ch
        assert text in lib.wce_last_error().decode(), (ch, lib.wce_last_error())
    assert lib.wce_short_field(None, *base.values(), None) == EINVAL
    assert lib.wce_short_field(h, *{**base, "n_frames": 0}.values(), None) == 0
    # link_host refuses a window the packet cannot fit in before it touches the device: 1520 + 6 - 1 + 100 > 1600
    c = object.__new__(wce.Context)
    c.handle, c.tx_pre = None, tm.chain_pre()
    with pytest.raises(ValueError, match="cannot hold"):
        c.link_host(wce.MOD_QPSK, wce.RATE_1_2, 30.0, 2, taps=np.ones(6) / 6, delay=100, stf=True, capture_len=1600)


def test_short_field_table(wce):
    """the 16 values the kernel replicates, through the host hook; and the model's own claims about the field"""
    t = np.zeros(32)
    assert wce.load().wce_debug_short_field_period(t.ctypes.data_as(ctypes.c_void_p)) == 0
    ref = st.short_period()
    ulp = np.spacing(float(np.max(np.abs(ref))))
    err = max(float(np.max(np.abs(np.asarray(t[0::2], LD) - ref.real))),
              float(np.max(np.abs(np.asarray(t[1::2], LD) - ref.imag))))
    print(f"table within {err / ulp:.2f} ulp of max |t|")
    assert err <= st.TOL_T * ulp
    full = tm.idft64(st.short_bins()[None, :])[0]
    assert float(np.max(np.abs(full - np.tile(ref, 4)))) < 1e-18            # period 16
    assert abs(float(np.mean(st.abs2(full))) - 52.0 / 4096.0) < 1e-18       # the long field's power for unit bins
    assert abs(float(np.mean(st.abs2(np.asarray(sm.clean_ltf(), np.clongdouble)))) - 52.0 / 4096.0) < 1e-15
    assert np.count_nonzero(st.short_bins()) == 12 and st.short_bins()[26] == 0
    assert abs(complex(ref[0]) - (0.046 + 0.046j)) < 1e-3 and abs(complex(ref[1]) - (-0.1324 + 0.0023j)) < 1e-3


def test_tolerances_are_reachable_and_comparisons_legitimate():
    u = 2.0 ** -53
    assert (260 + 512 + 4) * u <= st.TOL_MS / 2
    d_ec = (130 * u / np.sqrt(st.MS_MIN) + 8 * u * np.pi) / (32 * np.pi)
    assert d_ec <= st.TOL_EC / 2
    assert (2 * 66 + 256 + 10 + 20) * u + 2 * 2 * np.pi * 63 * d_ec <= st.TOL_ML / 2 and st.TOL_ML <= sm.MIN_GAP / 20
    assert ((66 * u / 0.1 + 8 * u * np.pi) / (128 * np.pi) + u / 32) <= st.TOL_CFO / 2
    assert 130 * u / np.sqrt(st.THR_STF) < 3e-14      # a detected frame's arg P: the issue's 130 u / sqrt(threshold)
    worst = {"ms": 0.0, "ml": 0.0, "cfo": 0.0, "gap": np.inf, "msmin": np.inf, "cond": np.inf, "wrap": np.inf,
             "sp_ms": 0.0, "sp_ec": 0.0}
    for L, B in SHAPES:
        cap, info, ltf = st.shape_set(L, B)
        an, a64 = st.shape_model(L, B), st.analyse(cap, ltf, np.float64)
        assert a64["ms"].dtype == np.float64 and an["ms"].dtype == np.longdouble
        name = f"L={L} B={B}"
        assert float(an["gap"].min()) > sm.MIN_GAP, name
        assert float(an["ms"].min()) >= st.MS_MIN and float(an["ms"].max()) <= 1.0, name
        assert float(an["ml"].min()) >= 0.0 and float(an["ml"].max()) <= 1.0, name
        assert float(np.min(np.abs(an["ms"] - st.THR_STF))) >= 1e-6, name
        assert float(np.min(np.abs(an["ml"] - st.THR_LTF))) >= 1e-6, name
        assert an["ms_spread"].max() <= st.TOL_MS / 10 and an["ec_spread"].max() <= st.TOL_EC / 10, name
        for backoff in (0, 5):
            r = st.sync_stf(cap, ltf, backoff=backoff, an=an)
            r64 = st.sync_stf(cap, ltf, backoff=backoff, real=np.float64, an=a64)
            det = r["detected"]
            assert np.array_equal(r["start"], r64["start"]), name
            if det.any():
                assert float(np.min(np.abs(r["wrap"][det] - 0.5))) > 1e-6, name
                assert float(r["cond"][det].min()) >= 0.1, name
                assert float(np.max(np.abs(np.asarray(r["cfo"][det], np.float64)))) < 1.0 / 32
                worst["cond"] = min(worst["cond"], float(r["cond"][det].min()))
                worst["wrap"] = min(worst["wrap"], float(np.min(np.abs(r["wrap"][det] - 0.5))))
            for k, key, tol in (("metric_stf", "ms", st.TOL_MS), ("metric_ltf", "ml", st.TOL_ML),
                                ("cfo", "cfo", st.TOL_CFO)):
                fin = np.isfinite(np.asarray(r[k], np.float64))
                assert np.array_equal(fin, np.isfinite(r64[k])), (name, k)
                if fin.any():
                    e = float(np.max(np.abs(np.asarray(r64[k], LD)[fin] - r[k][fin])))
                    assert e <= tol, (name, k, e)
                    worst[key] = max(worst[key], e)
        worst["gap"] = min(worst["gap"], float(an["gap"].min()))
        worst["msmin"] = min(worst["msmin"], float(an["ms"].min()))
        worst["sp_ms"] = max(worst["sp_ms"], float(an["ms_spread"].max()))
        worst["sp_ec"] = max(worst["sp_ec"], float(an["ec_spread"].max()))
    print(" ".join(f"{k} {v:.2e}" for k, v in worst.items()))


def test_model_claims_on_the_shared_data():
    """start on the first path, the estimate near the truth, cut and noise-only windows undetected, and today's
    sync missing every packet at |e| >= 0.02"""
    for L, B in ((488, 67), (1648, 67)):
        cap, info, ltf = st.shape_set(L, B)
        r = st.sync_stf(cap, ltf, an=st.shape_model(L, B))
        iw = st.in_window(info, L) & (info["snr"] >= 5)
        assert iw.sum() >= 30 and np.all(r["detected"][iw])
        off = r["start"][iw] - info["pos"][iw] - 192      # the short field, then the long field's 32-sample prefix
        assert off.min() >= 0 and off.max() <= 5           # on one of the six paths
        assert np.all(off[info["ntap"][iw] == 1] == 0)
        assert float(np.max(np.abs(np.asarray(r["cfo"][iw], np.float64) - info["eps"][iw]))) < 1e-3
        assert set(info["eps"][iw]) == set(st.EPS) and set(info["snr"][iw]) == set(st.SNR)
        assert not r["detected"][(info["kind"] == "cut") | (info["kind"] == "noise")].any()
        assert (info["kind"] == "cut").any() and (info["kind"] == "noise").any()
        far = iw & (np.abs(info["eps"]) >= 0.02)
        s, M, _ = sm.sync(cap, ltf, 0.25)
        assert far.sum() >= 10 and not np.any((s[far] >= info["pos"][far] + 192) & (s[far] <= info["pos"][far] + 197))
        if L == 1648:       # a packet on the window's first sample, one ending on its last, one running past its end
            k = info["kind"]
            assert np.all(info["pos"][k == "first"] == 0) and np.all(r["detected"][(k == "first") & (info["snr"] >= 5)])
            last = (k == "last")
            assert np.all(info["pos"][last] + 1520 + info["ntap"][last] - 1 == L) and np.all(r["detected"][last])
            short = (k == "short")
            assert np.all(info["pos"][short] + 1520 > L) and np.all(r["detected"][short])
            assert np.all(r["start"][short] + 128 + 1200 > L)      # so the _at calls give NaN rows
    zc, zl = st.zeros_set()
    z = st.sync_stf(zc, zl)
    assert np.all(z["start"] == -1) and np.all(z["metric_stf"] == 0) and np.all(z["metric_ltf"] == 0)
    assert np.isnan(np.asarray(z["cfo"], np.float64)).all()


def test_model_rules():
    """thresholds, backoff and poison in the model itself, on one small set"""
    cap, info, ltf = st.shape_set(488, 67)
    an = st.shape_model(488, 67)
    r0 = st.sync_stf(cap, ltf, 0.0, 0.0, an=an)
    assert np.array_equal(r0["start"], an["dstar"]) and np.isfinite(np.asarray(r0["cfo"], np.float64)).all()
    assert np.all(st.sync_stf(cap, ltf, 1.0, 0.0, an=an)["start"][an["ms"] < 1] == -1)
    r5 = st.sync_stf(cap, ltf, 0.0, 0.0, 5, an=an)
    assert np.array_equal(r5["start"], np.where(an["dstar"] >= 5, an["dstar"] - 5, -1))
    only_l = st.sync_stf(cap, ltf, 0.0, st.THR_LTF, an=an)["detected"]
    only_s = st.sync_stf(cap, ltf, st.THR_STF, 0.0, an=an)["detected"]
    both = st.sync_stf(cap, ltf, an=an)["detected"]
    assert np.array_equal(both, only_l & only_s) and only_l.sum() > both.sum()     # each threshold decides on its own
    bad = cap.copy()
    bad[3, 100] = np.nan
    rb = st.sync_stf(bad, ltf)
    assert rb["start"][3] == -1 and all(np.isnan(np.float64(rb[k][3])) for k in ("cfo", "metric_stf", "metric_ltf"))
    good = st.sync_stf(cap, ltf, an=an)
    assert np.array_equal(np.delete(rb["start"], 3), np.delete(good["start"], 3))


def test_chain_seed():
    """the chain's seed: the model detects all 67 at +-0.025 cycles per sample with wide margins, and today's
    receiver, on the same packets without the short field, none"""
    taps = st.chain_taps()
    m = st.chain_model(tm.chain_pre(), taps)
    assert np.all(m["start"] >= 192) and np.all(m["start"] <= 197)
    assert float(m["gap"].min()) > 1e-6 and np.all(m["nbiterr"] == 0)
    assert float(np.min(m["metric_stf"])) > 0.9 and float(np.min(m["metric_ltf"])) > st.THR_LTF + 0.05
    assert float(np.min(np.abs(m["wrap"] - 0.5))) > 0.4
    start, metric = st.chain_plain(tm.chain_pre(), taps)
    assert np.all(start == -1) and st.THR_LTF - float(metric.max()) > 1e-4
