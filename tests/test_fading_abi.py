"""The time-varying channel (wce_channel_tv, wce_transmit_tv), the parts that need no
GPU: the entry points exist (libwce.so, include/wce.h, the Python mirror and its
keywords) and refuse what the header says they refuse, fading_taps is the process it
says it is, the model of tests/fading_model.py is tx_model's where the knots are
constant and an fp64 implementation can meet cap_tol_tv, and the link experiment that
tests/test_fading_gpu.py runs on the device shows, in the model, what the tracker is for.

cap_tol_tv (fading_model's docstring has the derivation) counts n_taps + 4 roundings
against sum_t max_k |a[k][t]| max |s|.  Measured below, fp64 model against long double
over tx_model.SHAPES with moving knots at P = 16, 37, 80 and one segment: at most 0.47
of it -- the count is not widened."""
import ctypes
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import fading_model as fd
import tx_model as tm

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMS = {"wce_channel_tv": 10, "wce_transmit_tv": 13}
PAR_FIELDS = ["knots", "frame_stride", "knot_stride", "n_knots", "knot_period", "n_taps", "field", "cfo", "ow2",
              "delay", "seed", "first_frame"]


# ---------------------------------------------------------------- 1. the entry points
def test_symbols_exported_and_declared(wce):
    lib = wce.load()
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "wce.h")).read(), flags=re.S)
    for s, n in SYMS.items():
        assert hasattr(lib, s), s
        assert re.search(r"\bint\s+%s\s*\(" % s, hdr), s
        params = re.search(r"\b%s\s*\(([^)]*)\)" % s, hdr).group(1).split(",")
        assert len(params) == len(wce.wce.ABI[s]) == n, s
    assert re.search(r"\}\s*wce_fading_par\s*;", hdr)
    assert [f[0] for f in wce.wce.FadingPar._fields_] == PAR_FIELDS
    assert wce.FadingPar is wce.wce.FadingPar


def test_fading_par_layout_is_the_compilers(wce, tmp_path):
    src = tmp_path / "offsets.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "wce.h"\nint main(void) {\n'
                   + "".join(f'    printf("{f} %zu\\n", offsetof(wce_fading_par, {f}));\n' for f in PAR_FIELDS)
                   + '    printf("sizeof %zu\\n", sizeof(wce_fading_par));\n    return 0;\n}\n')
    exe = tmp_path / "offsets"
    subprocess.check_call(["gcc", "-std=gnu11", "-I", os.path.join(REPO, "include"), str(src), "-o", str(exe)])
    table = dict(line.split() for line in subprocess.check_output([str(exe)], text=True).splitlines())
    P = wce.wce.FadingPar
    assert ctypes.sizeof(P) == int(table.pop("sizeof"))
    assert {f: getattr(P, f).offset for f in PAR_FIELDS} == {f: int(v) for f, v in table.items()}


def test_python_keywords(wce):
    C = wce.Context
    knots = {"knot_period": 80, "n_taps": 1, "knot_stride": None, "knots_frame_stride": 0}
    want = {
        C.channel_tv: (["wave", "n_frames", "wave_len", "capture", "capture_len", "knots", "n_knots"],
                       {**knots, "field": True, "cfo": None, "ow2": None, "delay": None, "seed": 0x80211,
                        "first_frame": 0, "wave_stride": None, "capture_stride": None, "stream": None}),
        C.transmit_tv: (["sym", "n_frames", "capture", "capture_len", "knots", "n_knots"],
                        {**knots, "n_blocks": wce.NBLK, "tx_pre": None, "pre_stride": 0, "frame_stride": None,
                         "block_stride": wce.NSC, "cfo": None, "ow2": None, "delay": None, "seed": 0x80211,
                         "first_frame": 0, "capture_stride": None, "stream": None}),
    }
    for fn, (pos, kws) in want.items():
        p = inspect.signature(fn).parameters
        assert list(p)[1:1 + len(pos)] == pos, fn.__name__
        assert list(p)[1 + len(pos):1 + len(pos) + len(kws)] == list(kws), fn.__name__
        for k, default in kws.items():
            assert p[k].default == default, (fn.__name__, k)
    # the new keywords come behind the ones the static paths had, with defaults that leave those paths alone
    p = inspect.signature(C.transmit_host).parameters
    assert list(p)[-1] == "knot_period" and p["knot_period"].default is None
    p = inspect.signature(C.link_host).parameters
    assert list(p)[-2:] == ["knot_period", "tracker"]
    assert p["knot_period"].default == 80 and p["tracker"].default is None
    assert list(inspect.signature(wce.fading_taps).parameters) == ["rng", "n_frames", "power", "rho", "n_knots"]


def test_refusals_before_the_ctx_is_touched(wce):
    lib, W = wce.load(), wce.wce
    table = fd.refusals(W)
    assert len(table) == 30 + 36
    for name, kw, text in table:
        rc = fd.call_abi(W, lib, 0x10, name, kw)
        msg = lib.wce_last_error().decode()
        assert rc == -1 and msg.startswith(name + ":") and text in msg, (name, text, msg)
    par, base = fd.base_args(W)
    for name, kw in base.items():
        assert fd.call_abi(W, lib, 0x10, name, {**kw, "n_frames": 0}) == 0, name          # n_frames == 0 is WCE_OK
        assert fd.call_abi(W, lib, None, name, kw) == -1 and "null ctx" in lib.wce_last_error().decode()
        # the smallest count that covers, and a shared trajectory, hold
        ok = par(n_knots=fd.min_knots(1360, 6, 80), frame_stride=0)
        assert ok.n_knots == 19 and fd.call_abi(W, lib, 0x10, name, {**kw, "p": ok, "n_frames": 0}) == 0, name


# ---------------------------------------------------------------- 2. fading_taps
def test_fading_taps(wce):
    power = np.exp(-0.5 * np.arange(6))
    # rho = 1: every knot is pdp_taps of the same generator state
    frozen = wce.fading_taps(np.random.default_rng(1), 40, power, 1.0, 19)
    h = wce.pdp_taps(np.random.default_rng(1), 40, power)
    assert frozen.shape == (40, 19, 6) and frozen.dtype == np.complex128
    assert all(np.array_equal(frozen[:, k], h) for k in range(19))
    # knot 0 is pdp_taps at any rho, and the package's process is the model's
    a = wce.fading_taps(np.random.default_rng(1), 40, power, 0.9, 5)
    assert a.shape == (40, 5, 6) and np.array_equal(a[:, 0], h)
    assert np.array_equal(a, fd.fading_taps(np.random.default_rng(1), 40, power, 0.9, 5))
    assert not np.array_equal(a[:, 1], a[:, 0])
    assert wce.fading_taps(np.random.default_rng(1), 3, [1.0], 0.0, 2).shape == (3, 2, 1)
    for rho, n_knots in ((-0.01, 19), (1.01, 19), (float("nan"), 19), (0.5, 1), (0.5, 0)):
        with pytest.raises(ValueError):
            wce.fading_taps(np.random.default_rng(1), 4, power, rho, n_knots)
    with pytest.raises(ValueError):
        wce.fading_taps(np.random.default_rng(1), 4, np.ones(17), 0.5, 2)


@pytest.mark.parametrize("rho", [0.995, 0.5])
def test_fading_taps_lag_one_correlation(wce, rho):
    """x[k+1] = rho x[k] + sqrt(1 - rho^2) w with w ~ CN(0, p) independent of x[k] ~ CN(0, p), so
    E[x[k+1] conj x[k]] = rho p.  fading_taps scales frame f's whole trajectory by the factor c[f] that normalised
    its knot 0; dividing by it (c is recomputed from the same generator state, as pdp_taps draws) gives the
    unnormalised process.  z[f] = Re(x[1] conj x[0]) of tap 0 is independent over the n = 4,096 frames, so its
    mean has the standard error std(z) / sqrt(n), estimated from the sample; four of them."""
    n, power = 4096, np.exp(-0.5 * np.arange(6))
    a = wce.fading_taps(np.random.default_rng(7), n, power, rho, 3)
    rng = np.random.default_rng(7)
    raw = (rng.standard_normal((n, 6)) + 1j * rng.standard_normal((n, 6))) * np.sqrt(power / 2)
    x = a * np.sqrt(np.sum(np.abs(raw) ** 2, axis=1))[:, None, None]
    assert np.allclose(x[:, 0], raw, rtol=1e-13, atol=0)
    for k in (0, 1):
        z = np.real(x[:, k + 1, 0] * np.conj(x[:, k, 0]))
        se = float(np.std(z, ddof=1) / np.sqrt(n))
        print(f"\nrho {rho}, knots {k}, {k + 1}: mean {z.mean():.4f}, expected {rho * power[0]:.4f}, s.e. {se:.4f}")
        assert abs(z.mean() - rho * power[0]) <= 4 * se
        assert abs(np.mean(np.abs(x[:, k + 1, 0]) ** 2) - power[0]) <= 4 * np.std(np.abs(x[:, k + 1, 0]) ** 2) / np.sqrt(n)


# ---------------------------------------------------------------- 3. the model
KNOT_CASES = ((16, 0), (37, 0), (80, 0), (1500, 0), (80, 3))     # (P, knots beyond the smallest count)


def test_constant_knots_are_the_static_model():
    rng = np.random.default_rng(0xFAD0)
    for real in (np.longdouble, np.float64):
        for B, nb, field in tm.SHAPES:
            sym, pre = tm.shape_set(B, nb, field)
            wave = np.asarray(tm.modulate(sym, pre), np.complex128)
            wl = wave.shape[1]
            for (P, extra), nt in zip(KNOT_CASES, (1, 6, 16, 2, 6)):
                taps = tm.random_taps(rng, B, nt)
                knots = np.repeat(taps[:, None, :], fd.min_knots(wl, nt, P) + extra, axis=1)
                kw = dict(field=field, cfo=rng.uniform(-0.002, 0.002, B), ow2=1e-3,
                          delay=rng.integers(-40, 120, B), real=real)
                got = fd.channel_tv(wave, wl + 100, knots, P, **kw)
                assert got.dtype == tm._cplx(real)
                assert np.array_equal(got, tm.channel(wave, wl + 100, taps, **kw)), (real, B, nb, P)
    sym, pre = tm.shape_set(9, 7, 1)
    taps = tm.random_taps(rng, 9, 6)
    knots = np.repeat(taps[:, None, :], 19, axis=1)
    assert np.array_equal(fd.transmit_tv(sym, 800, knots, 80, pre, np.float64, cfo=0.001, delay=5),
                          tm.transmit(sym, 800, pre, np.float64, taps=taps, cfo=0.001, delay=5))
    # the guard: a non-finite knot, used or not, is a NaN window and touches no other frame
    ref = fd.transmit_tv(sym, 800, knots, 80, pre, np.float64)
    for k, v in ((0, np.nan), (18, np.inf), (12, -np.inf * 1j)):
        bad = knots.copy()
        bad[4, k, 2] = v
        got = fd.transmit_tv(sym, 800, bad, 80, pre, np.float64)
        assert np.isnan(got[4]).all() and np.array_equal(np.delete(got, 4, 0), np.delete(ref, 4, 0))


def test_fp64_model_agrees_with_long_double():
    worst = 0.0
    rng = np.random.default_rng(0xFAD2)
    for B, nb, field in tm.SHAPES:
        sym, pre = tm.shape_set(B, nb, field)
        wave = np.asarray(tm.modulate(sym, pre), np.complex128)      # what a device would have written
        wl = wave.shape[1]
        for (P, extra), (nt, cfo) in zip(KNOT_CASES, ((1, None), (16, 0.0077), (6, 0.002), (16, -0.002), (2, None))):
            knots = fd.moving_knots(rng, B, fd.min_knots(wl, nt, P) + extra, nt)
            L = wl + nt - 1
            kw = dict(field=field, cfo=cfo)
            c_ld, c_64 = fd.channel_tv(wave, L, knots, P, **kw), fd.channel_tv(wave, L, knots, P, real=np.float64, **kw)
            assert c_64.dtype == np.complex128 and c_ld.dtype == np.clongdouble
            ratio = tm.relmax_rows(c_64, c_ld) / fd.cap_tol_tv(wave, knots, cfo, c_ld, field, with_wave=False)
            worst = max(worst, float(ratio.max()))
            # moving knots move the capture: the static model with knot 0's taps is far outside the bound
            if nb:
                far = tm.relmax_rows(tm.channel(wave, L, knots[:, 0], real=np.float64, **kw), c_ld)
                assert far.min() > 1e-3
    print(f"\nfp64 vs long double: capture {worst:.2f} of cap_tol_tv")
    assert worst <= 1.0


def test_interpolation_is_the_definition():
    """the taps of a handful of outputs, spelled out in exact rational arithmetic"""
    from fractions import Fraction as F
    a = fd.moving_knots(np.random.default_rng(5), 1, 4, 3)
    h = fd.taps_tv(a, 37, 100, np.longdouble)[0]
    for m in (0, 1, 36, 37, 38, 73, 74, 99):
        k, j = divmod(m, 37)
        for t in range(3):
            for part in (np.real, np.imag):
                lo, hi = F(float(part(a[0, k, t]))), F(float(part(a[0, k + 1, t])))
                want = lo + (hi - lo) * j / 37
                assert abs(F(float(part(h[t, m]))) - want) <= abs(want) * F(1, 2 ** 50) + F(1, 2 ** 60)
    assert np.array_equal(h[:, 0], a[0, 0]) and np.array_equal(h[:, 37], a[0, 1]) and np.array_equal(h[:, 74], a[0, 2])


# ---------------------------------------------------------------- 4. the link experiment
def test_link_experiment_in_the_model():
    """fading_model.link_set: 67 packets of 16-QAM rate 1/2 at nominal 22 dB, six taps of amplitudes exp(-0.5 t)
    fading by rho = 0.995 a block, offsets within +-0.002 cycles per sample, delays 0..99, mu = 0.5, beta = 2.
    Every packet is detected; the tracked chain leaves 695 bit errors of 96,480 where the static one leaves 4,264,
    a factor of 6.1; frozen (rho = 1) both decode without error."""
    c = fd.link_set()
    assert c["taps"].shape == (67, 19, 6) and np.abs(c["cfo"]).max() <= 0.002
    assert c["delay"].min() >= 0 and c["delay"].max() <= 99 and c["bits"].shape == (67, 1440)
    r = fd.link_model()
    assert np.all(r["start"] >= 0)
    trk_e, sta_e = int(r["tracked"].sum()), int(r["static"].sum())
    frozen = fd.link_model(1.0)
    print(f"\nlink model, {c['bits'].size} bits: rho 0.995 static {sta_e} tracked {trk_e}; "
          f"rho 1 static {int(frozen['static'].sum())} tracked {int(frozen['tracked'].sum())}")
    assert trk_e < sta_e
    assert np.all(frozen["start"] >= 0)
