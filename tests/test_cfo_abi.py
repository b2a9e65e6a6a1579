"""Carrier frequency offset correction, the parts that need no GPU: the two
entry points exist (libwce.so, include/wce.h, the Python mirror and its
keywords), and the reference model of tests/cfo_model.py in fp64 agrees with
itself in long double, so that the bounds the GPU tests hold the kernels to
(tests/test_cfo_gpu.py) are bounds an fp64 implementation can meet.

Measured, 40 random frames: blocks 3.5e-15, preamble 3.7e-16, estimate 1e-18
cycles per sample, ow2 2.5e-14."""
import inspect
import os
import re

import numpy as np

import cfo_model as cm

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMS = ("wce_front_end_blocks_cfo", "wce_front_end_preamble_cfo")


def test_symbols_exported_and_declared(wce):
    lib = wce.load()
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "wce.h")).read(), flags=re.S)
    for s in SYMS:
        assert hasattr(lib, s), s
        assert re.search(r"\bint\s+%s\s*\(" % s, hdr), s
        assert s in wce.wce.ABI
    # the declared parameter lists are the mirror's: 11 each
    for s in SYMS:
        params = re.search(r"\b%s\s*\(([^)]*)\)" % s, hdr).group(1).split(",")
        assert len(params) == len(wce.wce.ABI[s]) == 11, s


def test_python_keywords(wce):
    C = wce.Context
    for fn, kws in ((C.front_end_blocks, {"cfo": None, "sample_offset": 0}),
                    (C.front_end_preamble, {"cfo": None, "estimate_cfo": True}),
                    (C.front_end_host, {"cfo": False}),
                    (C.receive_host, {"cfo": False, "sample_offset": 0})):
        p = inspect.signature(fn).parameters
        for k, default in kws.items():
            assert k in p and p[k].default == default, (fn.__name__, k)


def test_model_matches_numpy_fft_without_offset():
    """eps = 0: the model is the plain front end (np.fft as in tests/test_front_gpu.py)"""
    rng = np.random.default_rng(0xCF0)
    pk, lp = cm.random_packets(rng, 4, cm.NBLK * 80 + 9), cm.random_packets(rng, 4, 171)
    z = np.zeros(4)
    ref = np.roll(np.fft.fft(pk[:, :1200].reshape(4, 15, 80)[:, :, 16:], axis=-1), 26, axis=-1)[..., :cm.N]
    assert cm.relmax(cm.blocks(pk, z, 400), ref) < 1e-14
    pre, ow2 = cm.preamble(lp[:, :160], z)
    p1, p2 = lp[:, 96:160], lp[:, 32:96]
    assert cm.relmax(pre, np.roll(np.fft.fft((p1 + p2) / 2, axis=-1), 26, axis=-1)[:, :cm.N]) < 1e-14
    assert np.max(np.abs(ow2 / (np.sum(np.abs(p2 - p1) ** 2, axis=1) / 128) - 1)) < 1e-14


def test_model_undoes_an_applied_offset():
    """x exp(2 pi i eps n) derotated with eps is x: blocks and preamble of the rotated data are those of the
    clean data with eps = 0, to the rounding of the rotated samples (2^-53 each)"""
    rng = np.random.default_rng(0xCF1)
    B = 8
    eps = cm.draw_eps(rng, B)
    pk, lp = cm.random_packets(rng, B, 1200), cm.random_packets(rng, B, 160)
    for off in (0, 160, -7, 400):
        rot = cm.apply_cfo(pk, eps[:, None], (np.arange(1200) + off)[None, :])
        assert cm.relmax(cm.blocks(rot, eps, off), cm.blocks(pk, np.zeros(B))) < 1e-15
    rot = cm.apply_cfo(lp, eps[:, None], (np.arange(160) - 160)[None, :])
    assert cm.relmax(cm.preamble(rot, eps)[0], cm.preamble(lp, np.zeros(B))[0]) < 1e-15


def test_fp64_model_agrees_with_long_double():
    """The GPU tests' bounds, met by the same arithmetic in fp64: 2e-14 for bins (1e-14, the front end's
    tolerance, plus the phase rounding 2 pi |eps n| 2^-53 <= 7e-15 rounded up), 1e-16 cycles per sample for
    the estimate (64 products move arg c by <= 64 * 2^-53 rad = 1.8e-17 cycles per sample, atan2 a few 1e-18;
    5x over that), 1e-12 for ow2 (2^-53 |p| per derotated sample against |d| = |p| / sqrt(SNR), SNR <= 1e6)."""
    rng = np.random.default_rng(0xCF2)
    B = 40
    lp, eps, snr = cm.ltf_batch(rng, B)
    pk = cm.random_packets(rng, B, 1209)
    e_ld, e_64 = cm.estimate(lp[:, :160]), cm.estimate(lp[:, :160], np.float64)
    d_est = float(np.max(np.abs(e_64 - e_ld)))
    # the data carries the offsets it claims: 64 pairs at 10 dB leave 1e-4 rms; an estimate wraps at +-1/128
    wrapped = (np.asarray(e_ld - eps, np.float64) + cm.EPS_MAX) % (2 * cm.EPS_MAX) - cm.EPS_MAX
    assert np.max(np.abs(wrapped)) < 6e-4
    worst_b = max(cm.relmax(cm.blocks(pk, eps, off, real=np.float64), cm.blocks(pk, eps, off))
                  for off in (0, 160, -7, 400))
    e_dev = np.asarray(e_ld, np.float64)               # what a device would have written
    (pre_ld, ow_ld), (pre_64, ow_64) = cm.preamble(lp[:, :160], e_dev), cm.preamble(lp[:, :160], e_dev, np.float64)
    d_pre = cm.relmax(pre_64, pre_ld)
    d_ow = float(np.max(np.abs(ow_64 / ow_ld - 1)))
    print(f"\nfp64 vs long double: blocks {worst_b:.2e}, preamble {d_pre:.2e}, estimate {d_est:.2e}, ow2 {d_ow:.2e}")
    assert worst_b <= 2e-14 and d_pre <= 2e-14 and d_est <= 1e-16 and d_ow <= 1e-12
    # corrected, ow2 is the noise the data was made with; uncorrected it is not
    p = np.mean(np.abs(lp[:, 32:160]) ** 2, axis=1)
    sigma2 = p / (1 + 10 ** (snr / 10))
    assert np.all(np.abs(np.asarray(ow_ld, np.float64) / sigma2 - 1) < 0.6)   # 64 pairs: a chi-square of 128 dof
    raw = cm.preamble(lp[:, :160], np.zeros(B))[1]
    assert raw[0] > 10 * ow_ld[0] and raw[1] > 10 * ow_ld[1]
