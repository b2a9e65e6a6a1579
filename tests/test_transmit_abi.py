"""The transmitter and the channel (wce_modulate, wce_channel, wce_transmit), the
parts that need no GPU: the entry points exist (libwce.so, include/wce.h, the
Python mirror and its keywords) and refuse what the header says they refuse, the
model of tests/tx_model.py reproduces the recorded packet, its noise is Gaussian
where wce_synth_frames' is not, its conventions are WiFi_RX.m's, and the bounds
the GPU tests hold the kernels to (tests/test_transmit_gpu.py) are ones an fp64
implementation can meet.

The refusals run here with an opaque non-NULL ctx: every one of them returns
before the ctx is touched (the table is tx_model.refusals).  tests/test_transmit_gpu.py repeats them on a real
context and checks that nothing was written.

Tolerances, u = 2^-53, each measured below as the fp64 model against long double:

TOL_WAVE = 1e-14 of the frame's largest sample, the front end's tolerance for
the same transform run the other way.  A sample is a sum of 53 terms |X| / 64;
the 8 x 8 transform rounds each about 8 times (3 + 3 butterflies, a twiddle, the
scale is exact): |dy| <= 8 u 53 Xmax / 64 = 7.4e-16 Xmax.  The largest sample is
at least the rms one, sqrt(52) Xrms / 64, and Xmax / Xrms <= 1.53 (64-QAM), so
Xmax <= 13.6 ymax and |dy| <= 1.0e-14 ymax.

Capture without noise, against the frame's largest clean output (tx_model.cap_tol):
what a sample is made of is A = sum_t |h_t| max |s|; the waveform's own error
(TOL_WAVE, when the comparison starts from the symbols) and the FIR's n_taps + 2
roundings count against A; the rotor adds the phase term 2 pi |cfo n| u (a phase
formed in fp64, as the model's is; the device's exact phase is inside it) and the
product 4 u.

TOL_NOISE = 2e-14 sqrt(ow2).  |w| <= R / sqrt 2 sqrt(ow2) with R = sqrt(-2 ln u1)
<= sqrt(2 * 53 ln 2) = 8.58.  log, sqrt and sincos within 2 ulp each, sqrt(ow2 / 2)
and two products: about 8 u relative, 5.4e-15 at the largest R; the fp64 model's
angle 2 pi u2 is itself rounded, 2 pi u of 6.07: 4.2e-15.  Twice their sum.

Measured (fp64 model against long double): waveform 9.2e-16 over the twelve
shapes; capture without noise at most 0.54 of cap_tol (without its waveform
term); noise 1.8e-15 sqrt(ow2), largest R 4.91 in 67 x 1,488 draws.  The
recording: blocks 4.0e-5, field 3.7e-5.  Chain sets: smallest gap 0.21, the
model's offset estimate within 1.13e-5 cycles per sample of the given one, 0 bit
errors."""
import ctypes
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import cfo_model as cm
import demod_model as dm
import sync_model as sm
import tx_model as tm

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMS = {"wce_modulate": 11, "wce_channel": 10, "wce_transmit": 13}
PAR_FIELDS = ["taps", "taps_stride", "n_taps", "field", "cfo", "ow2", "delay", "seed", "first_frame"]


# ---------------------------------------------------------------- 1. the entry points
def test_symbols_exported_and_declared(wce):
    lib = wce.load()
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "wce.h")).read(), flags=re.S)
    for s, n in SYMS.items():
        assert hasattr(lib, s), s
        assert re.search(r"\bint\s+%s\s*\(" % s, hdr), s
        params = re.search(r"\b%s\s*\(([^)]*)\)" % s, hdr).group(1).split(",")
        assert len(params) == len(wce.wce.ABI[s]) == n, s
    assert re.search(r"\}\s*wce_channel_par\s*;", hdr)
    assert [f[0] for f in wce.wce.ChannelPar._fields_] == PAR_FIELDS


def test_channel_par_layout_is_the_compilers(wce, tmp_path):
    src = tmp_path / "offsets.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "wce.h"\nint main(void) {\n'
                   + "".join(f'    printf("{f} %zu\\n", offsetof(wce_channel_par, {f}));\n' for f in PAR_FIELDS)
                   + '    printf("sizeof %zu\\n", sizeof(wce_channel_par));\n    return 0;\n}\n')
    exe = tmp_path / "offsets"
    subprocess.check_call(["gcc", "-std=gnu11", "-I", os.path.join(REPO, "include"), str(src), "-o", str(exe)])
    table = dict(line.split() for line in subprocess.check_output([str(exe)], text=True).splitlines())
    P = wce.wce.ChannelPar
    assert ctypes.sizeof(P) == int(table.pop("sizeof"))
    assert {f: getattr(P, f).offset for f in PAR_FIELDS} == {f: int(v) for f, v in table.items()}


def test_python_keywords(wce):
    C = wce.Context
    want = {
        C.modulate: (["sym", "n_frames", "wave"],
                     {"n_blocks": wce.NBLK, "tx_pre": None, "pre_stride": 0, "frame_stride": None,
                      "block_stride": wce.NSC, "wave_stride": None, "stream": None}),
        C.channel: (["wave", "n_frames", "wave_len", "capture", "capture_len"],
                    {"taps": None, "n_taps": 1, "taps_stride": 0, "field": True, "cfo": None, "ow2": None,
                     "delay": None, "seed": 0x80211, "first_frame": 0, "wave_stride": None, "capture_stride": None,
                     "stream": None}),
        C.transmit: (["sym", "n_frames", "capture", "capture_len"],
                     {"n_blocks": wce.NBLK, "tx_pre": None, "pre_stride": 0, "frame_stride": None,
                      "block_stride": wce.NSC, "taps": None, "n_taps": 1, "taps_stride": 0, "cfo": None, "ow2": None,
                      "delay": None, "seed": 0x80211, "first_frame": 0, "capture_stride": None, "stream": None}),
        C.transmit_host: (["sym"], {"tx_pre": None, "taps": None, "cfo": None, "ow2": None, "delay": None,
                                    "capture_len": None, "seed": 0x80211, "first_frame": 0, "fused": True}),
        C.link_host: (["modulation", "rate", "snr_db", "n_frames"],
                      {"sources": (wce.LT_LS, wce.PS_LINEAR, wce.PS_MMSE), "taps": None, "cfo": None, "delay": None,
                       "capture_len": 1488, "threshold": 0.25, "backoff": 0, "seed": 0x80211, "dd_iterations": 0}),
    }
    for fn, (pos, kws) in want.items():
        p = inspect.signature(fn).parameters
        assert list(p)[1:1 + len(pos)] == pos, fn.__name__
        assert list(p)[1 + len(pos):1 + len(pos) + len(kws)] == list(kws), fn.__name__
        for k, default in kws.items():
            assert p[k].default == default, (fn.__name__, k)
    assert list(inspect.signature(wce.pdp_taps).parameters) == ["rng", "n_frames", "power"]
    assert "Rhh" in wce.pdp_taps.__doc__ and "np.diag(power" in wce.pdp_taps.__doc__


def test_pdp_taps(wce):
    power = np.exp(-0.5 * np.arange(6))
    h = wce.pdp_taps(np.random.default_rng(1), 4000, power)
    assert h.shape == (4000, 6) and h.dtype == np.complex128
    assert np.allclose(np.sum(np.abs(h) ** 2, axis=1), 1.0, rtol=0, atol=1e-14)
    mean = np.mean(np.abs(h) ** 2, axis=0)          # normalising each frame flattens the profile a little
    assert np.all(np.diff(mean) < 0) and np.allclose(mean, power / power.sum(), rtol=0, atol=0.05)
    one = wce.pdp_taps(np.random.default_rng(2), 5, [0.0, 0.0, 3.0])
    assert np.allclose(np.abs(one), [[0, 0, 1]] * 5, rtol=0, atol=1e-15)
    with pytest.raises(ValueError):
        wce.pdp_taps(np.random.default_rng(1), 4, np.ones(17))


def test_refusals_before_the_ctx_is_touched(wce):
    lib, W = wce.load(), wce.wce
    table = tm.refusals(W)
    assert len(table) == 14 + 20 + 26
    for name, kw, text in table:
        rc = tm.call_abi(W, lib, 0x10, name, kw)
        msg = lib.wce_last_error().decode()
        assert rc == -1 and msg.startswith(name) and text in msg, (name, text, msg)
    for name, kw in tm.base_args(W)[1].items():
        assert tm.call_abi(W, lib, 0x10, name, {**kw, "n_frames": 0}) == 0, name          # n_frames == 0 is WCE_OK
        assert tm.call_abi(W, lib, None, name, kw) == -1 and "null ctx" in lib.wce_last_error().decode()


# ---------------------------------------------------------------- 2. the recording
def test_model_reproduces_the_recorded_packet(golden):
    """1e-3 absolute: the recording is rounded to four decimals, which moves a sample by at most 7.1e-5 and a
    64-vector by at most 5.7e-4 in 2-norm; that bounds any sample of its projection off the 11 null bins.  A
    wrong bin map, scale or sign errs by O(1)."""
    m = golden["matlab"]
    sym, pre = tm.matlab_bins(m)
    wave = np.asarray(tm.modulate(sym, pre), np.complex128)[0]
    assert wave.shape == (1360,)
    field, blocks = wave[:160], wave[160:].reshape(15, 80)
    rec = m["tx_packet"].reshape(15, 80)
    d_blocks = float(np.max(np.abs(blocks[:, 16:] - rec[:, 16:])))
    d_field = float(max(np.max(np.abs(field[32:96] - m["tx_lptot"][32:96])),
                        np.max(np.abs(field[96:] - m["tx_lptot"][96:]))))
    print(f"\nrecording: blocks {d_blocks:.2e}, field {d_field:.2e}")
    assert d_blocks <= 1e-3 and d_field <= 1e-3
    assert float(np.max(np.abs(blocks[0, 16:]))) > 0.05           # against samples of this size
    # the prefix is the body's tail exactly (sample 0 is windowed in the recording, and left out there)
    assert np.array_equal(blocks[:, 1:16], blocks[:, 65:80]) and np.array_equal(field[1:32], field[65:96])
    assert np.array_equal(blocks[:, 0], blocks[:, 64]) and np.array_equal(field[32:96], field[96:])
    assert float(np.max(np.abs(rec[:, 1:16] - blocks[:, 1:16]))) <= 1e-3
    # and the front end's inverse: np.fft of the model's waveform returns the bins
    back = np.roll(np.fft.fft(blocks[:, 16:], axis=-1), 26, axis=-1)[:, :53]
    assert cm.relmax(back, sym[0]) < 1e-14


# ---------------------------------------------------------------- 3. tolerances
def test_fp64_model_agrees_with_long_double():
    worst_w, worst_c, worst_n = 0.0, 0.0, 0.0
    assert 8 * 53 / 64 * tm.U * 13.6 <= tm.TOL_WAVE * 1.001
    rng = np.random.default_rng(0x7CA0)
    for B, nb, field in tm.SHAPES:
        sym, pre = tm.shape_set(B, nb, field)
        w_ld, w_64 = tm.modulate(sym, pre), tm.modulate(sym, pre, np.float64)
        assert w_64.dtype == np.complex128 and w_ld.dtype == np.clongdouble
        assert w_ld.shape == (B, 160 * field + 80 * nb)
        worst_w = max(worst_w, float(tm.relmax_rows(w_64, w_ld).max()))
        wave = np.asarray(w_ld, np.complex128)      # what a device would have written
        for nt, cfo in ((1, None), (2, 0.002), (16, 0.0077), (16, -0.002)):
            taps = tm.random_taps(rng, B, nt)
            L = wave.shape[1] + nt - 1
            kw = dict(taps=taps, field=field, cfo=cfo, delay=None)
            c_ld, c_64 = tm.channel(wave, L, **kw), tm.channel(wave, L, real=np.float64, **kw)
            ratio = tm.relmax_rows(c_64, c_ld) / tm.cap_tol(wave, taps, cfo, c_ld, field, with_wave=False)
            worst_c = max(worst_c, float(ratio.max()))
    n_ld, n_64 = tm.noise(tm.NOISE_B, tm.NOISE_L, 1.0), tm.noise(tm.NOISE_B, tm.NOISE_L, 1.0, real=np.float64)
    worst_n = float(np.max(np.abs(n_64 - n_ld)))
    print(f"\nfp64 vs long double: waveform {worst_w:.2e}, capture {worst_c:.2f} of cap_tol, noise {worst_n:.2e}, "
          f"largest R {float(np.max(np.abs(n_ld)) * np.sqrt(2)):.2f}")
    assert worst_w <= tm.TOL_WAVE and worst_c <= 1.0 and worst_n <= tm.TOL_NOISE
    assert 2 * (8 * tm.U * 8.58 / np.sqrt(2) + 2 * np.pi * tm.U * 8.58 / np.sqrt(2)) <= tm.TOL_NOISE


# ---------------------------------------------------------------- 4. noise statistics
def test_noise_is_gaussian_where_irwin_hall_is_not():
    w = np.asarray(tm.noise(tm.NOISE_B, tm.NOISE_L, 2.0, seed=tm.SEED, real=np.float64))
    n = w.size
    for part in (w.real.ravel(), w.imag.ravel()):
        assert abs(part.mean()) < 4 / np.sqrt(n)                   # sigma = 1: ow2 / 2
        var = part.var()
        assert abs(var - 1.0) < 0.02
        kurt = np.mean((part - part.mean()) ** 4) / var ** 2 - 3.0
        assert abs(kurt) < 0.05, kurt                              # standard error 0.015; Irwin-Hall(4): -0.3
        assert np.max(np.abs(part)) > 3.6                          # Irwin-Hall(4) ends at 3.46
    ih = (np.random.default_rng(0).uniform(size=(n, 4)).sum(axis=1) - 2.0) * np.sqrt(3.0)
    assert np.max(np.abs(ih)) < 3.47 and np.mean(ih ** 4) / ih.var() ** 2 - 3.0 < -0.25
    # streams: frames differ, first_frame shifts the rows, the seed matters, ow2 only scales
    assert len({w[f, :8].tobytes() for f in range(tm.NOISE_B)}) == tm.NOISE_B
    shard = np.asarray(tm.noise(27, tm.NOISE_L, 2.0, first_frame=40, real=np.float64))
    assert np.array_equal(shard, w[40:])
    assert not np.array_equal(np.asarray(tm.noise(27, tm.NOISE_L, 2.0, first_frame=39, real=np.float64)), w[40:])
    assert not np.array_equal(np.asarray(tm.noise(3, 64, 2.0, seed=tm.SEED + 1, real=np.float64)), w[:3, :64])
    assert np.array_equal(np.asarray(tm.noise(3, 64, 8.0, real=np.float64)), 2 * w[:3, :64])


# ---------------------------------------------------------------- 5. conventions
def test_ow2_is_what_wifi_rx_estimates(golden):
    """WiFi_RX.m:31's estimate, sum |p2 - p1|^2 / 128 of the received field, is the channel's ow2: per frame a
    chi-square of 128 degrees of freedom over 128, 1.5% for the mean of 67"""
    _, pre = tm.matlab_bins(golden["matlab"])
    B = 67
    ow2 = np.random.default_rng(5).uniform(0.5, 2.0, B) * 1e-6
    none = np.zeros((B, 0, 53))
    cap = np.asarray(tm.transmit(none, 160, pre, np.float64, ow2=ow2), np.complex128)
    est = cm.preamble(cap, np.zeros(B), np.float64)[1]
    ratio = float(np.mean(est / ow2))
    print(f"\nmean estimate / ow2 = {ratio:.4f}")
    assert abs(ratio - 1.0) < 0.05
    clean = np.asarray(tm.transmit(none, 160, pre, np.float64), np.complex128)
    assert np.all(cm.preamble(clean, np.zeros(B), np.float64)[1] == 0.0)
    # nominal SNR: a frame of unit-mean-energy points at SCALE has the sample power 52 SCALE^2 / 4096
    sym = tm.symbols(np.random.default_rng(6), 40, 15, dm.QAM16)
    p = float(np.mean(np.abs(np.asarray(tm.modulate(sym, None, np.float64))[:, 16:]) ** 2))
    assert abs(p / float(tm.nominal_ow2(0.0)) - 1.0) < 0.02


# ---------------------------------------------------------------- 6. the chain's sets
@pytest.mark.parametrize("mod,rate", tm.CHAIN)
def test_chain_sets_decode_in_the_model(mod, rate):
    pre = tm.chain_pre()
    c = tm.chain_set(mod, rate)
    cap, tx = tm.chain_capture(mod, rate, pre)
    r = tm.chain_receive(cap, tx, pre, mod, rate)
    err = np.sum(r["bits"] != c["bits"], axis=1)
    d_cfo = float(np.max(np.abs(r["cfo"] - c["cfo"])))
    print(f"\nmod {mod} rate {rate}: start {r['start']}, smallest gap {r['gap'].min():.2e}, cfo error {d_cfo:.2e}, "
          f"bit errors {err}")
    assert np.array_equal(r["start"], c["delay"] + 32)
    assert r["gap"].min() > sm.MIN_GAP
    assert np.all(err == 0)
    assert d_cfo < tm.CHAIN_CFO_TOL
