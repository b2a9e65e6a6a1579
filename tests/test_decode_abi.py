"""Decoding (wce_soft_demap, wce_viterbi_decode), the parts that need no GPU: the
entry points exist (libwce.so, include/wce.h, the Python mirror and its
keywords), the model of tests/fec_model.py is 802.11's code, puncturing and
interleaver, and the data the GPU tests (tests/test_decode_gpu.py) compare on
makes their comparisons legitimate.

Bound (c) on a soft bit, |L_dev - L_ld| <= 2^-23 |L_ld| + TOL_ABS max |L_ld| of
the frame.  The first term is the one rounding to float.  For the second, with
u = 2^-53, w = |Hu|^2 and S = (|v| + (M-1) d)^2, which bounds every (v - level)^2:
  - the blend rounds 3 times per part (tests/test_demod_abi.py), w = x^2 + y^2
    twice more: dw <= (2 * 3 + 2) u w = 8 u w;
  - the definition: a level is one product, the difference one rounding, the
    square one: dD_c <= (2 * 2 + 1) u D_c <= 5 u S, so d(D0 - D1) <= 11 u S with the
    subtraction's own rounding, and the product with w adds (8 + 1) u w |D0 - D1|:
    |dL| <= 20 u w S;
  - the closed form (q1 - q0) d (2 v - (q0 + q1) d) the kernel may use: its two terms
    are at most 1.2 S together (worst at the outermost 64-QAM level), five
    roundings and dw: |dL| <= (5 * 1.2 + 8) u w S = 14 u w S.
Either way |dL| <= 20 u w S.  How w S of a frame's symbols compares with the
frame's largest |L| is a data condition: the symbol with the largest w S has a
bit (the axis's sign bit when |v| is large, the next one when it is small)
whose |L| is a good part of it; on every frame of the clean set
max w S <= 8 max |L| is checked (measured: at most 3.02), so |dL| <= 160 u max |L| =
1.8e-14 max |L|; TOL_ABS = 1e-13.

Measured (fp64 model against long double, all four modulations, with and
without the blend): 7.1e-16 of the frame's max |L|.

The decoder is compared exactly.  On the clean set (a) that is legitimate
because the model decodes every frame without a bit error whether its metrics
are float32 or float64; on the integer set (b) because every partial sum is an
integer below 2^24 (3240 steps of at most 2 * 31), so float arithmetic is exact
and ties are ties in every precision."""
import inspect
import os
import re

import numpy as np
import pytest

import demod_model as dm
import fec_model as fm

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -53
ARITY = {"wce_soft_demap": 10, "wce_viterbi_decode": 14, "wce_decode_info_bits": 2}


def test_symbols_exported_and_declared(wce):
    lib = wce.load()
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "wce.h")).read(), flags=re.S)
    for name, arity in ARITY.items():
        assert hasattr(lib, name), name
        assert re.search(r"\bint\s+%s\s*\(" % name, hdr), name
        params = re.search(r"\b%s\s*\(([^)]*)\)" % name, hdr).group(1).split(",")
        assert len(params) == len(wce.wce.ABI[name]) == arity, name
    for name, value in (("WCE_RATE_1_2", 0), ("WCE_RATE_2_3", 1), ("WCE_RATE_3_4", 2)):
        assert re.search(r"\b%s\s*=\s*%d\b" % (name, value), hdr), name
    assert re.search(r"#define\s+WCE_DEC_TERMINATED\s+\(1u << 0\)", hdr)
    assert (wce.RATE_1_2, wce.RATE_2_3, wce.RATE_3_4) == (0, 1, 2) == fm.RATES
    assert wce.DEC_TERMINATED == 1


def test_python_keywords(wce):
    C = wce.Context
    demap = {"h_lt": None, "h_stride": wce.NSC, "modulation": wce.MOD_BPSK, "scale": 8.8753, "llr": None,
             "eq_frame_stride": None, "eq_block_stride": wce.NSC, "llr_frame_stride": None, "llr_block_stride": None,
             "stream": None}
    vit = {"terminated": True, "bits": None, "bits_stride": None, "ref_bits": None, "ref_stride": None,
           "nbiterr": None, "llr_frame_stride": None, "llr_block_stride": None, "stream": None}
    host = {"h_lt": None, "modulation": wce.MOD_BPSK, "rate": wce.RATE_1_2, "scale": 8.8753, "terminated": True,
            "ref_bits": None}
    chain = {"decode_rate": None, "ref_bits": None, "terminated": True}
    for fn, kws in ((C.soft_demap, demap), (C.viterbi_decode, vit), (C.decode_host, host), (C.receive_host, chain),
                    (C.receive_capture_host, chain)):
        p = inspect.signature(fn).parameters
        for k, default in kws.items():
            assert k in p and p[k].default == default, (fn.__name__, k)
    assert list(inspect.signature(C.soft_demap).parameters)[1:4] == ["eq", "h", "n_frames"]
    assert list(inspect.signature(C.viterbi_decode).parameters)[1:5] == ["llr", "n_frames", "modulation", "rate"]
    assert list(inspect.signature(C.decode_host).parameters)[1:3] == ["eq", "h"]
    for fn in (C.receive_host, C.receive_capture_host):         # trailing, behind the keywords there were
        assert list(inspect.signature(fn).parameters)[-3:] == ["decode_rate", "ref_bits", "terminated"]


def test_info_bits(wce):
    lib = wce.load()
    for mod, rate in fm.COMBOS:
        assert wce.info_bits(mod, rate) == lib.wce_decode_info_bits(mod, rate) == fm.info_bits(mod, rate)
    assert wce.info_bits(wce.MOD_BPSK, wce.RATE_1_2) == 360 and wce.info_bits(wce.MOD_QAM64, wce.RATE_3_4) == 3240
    for mod, rate in ((3, 0), (0, 0), (8, 1), (1, 3), (1, -1)):
        assert lib.wce_decode_info_bits(mod, rate) == -1 and lib.wce_last_error()
        with pytest.raises(wce.WceError):
            wce.info_bits(mod, rate)


# ---------------------------------------------------------------- the model is 802.11's
def test_encoder_impulse_response():
    out = fm.encode(np.array([[1, 0, 0, 0, 0, 0, 0, 0]], np.uint8))[0]
    assert "".join(map(str, out[0:14:2])) == "1011011" and "".join(map(str, out[1:14:2])) == "1111001"
    assert not out[14:].any()
    pred, cA, cB = fm.trellis()
    assert np.array_equal(cA[0] ^ cA[1], np.ones(64, int)) and np.array_equal(cB[0] ^ cB[1], np.ones(64, int))
    for s in range(64):                                     # the successor of s on input u is (u << 5) | (s >> 1)
        for u in (0, 1):
            assert s in pred[:, (u << 5) | (s >> 1)]


def test_interleaver():
    assert list(fm.interleave_index(dm.BPSK)[:17]) == list(range(0, 48, 3)) + [1]
    assert list(fm.interleave_index(dm.QAM16)[:8]) == [0, 13, 24, 37, 48, 61, 72, 85]
    assert list(fm.interleave_index(dm.QAM64)[:8]) == [0, 20, 37, 54, 74, 91, 108, 128]
    for mod in fm.MODS:
        j = fm.interleave_index(mod)
        assert sorted(j) == list(range(fm.n_cbps(mod)))
        assert np.min(np.abs(np.diff(j // mod))) >= 3      # adjacent coded bits: at least 3 subcarriers apart


def test_puncturing():
    mother = np.arange(24)[None, :]
    assert list(fm.puncture(mother, fm.RATE_1_2)[0]) == list(range(24))
    assert list(fm.puncture(mother, fm.RATE_2_3)[0][:6]) == [0, 1, 2, 4, 5, 6]            # A0 B0 A1, A2 B2 A3
    assert list(fm.puncture(mother, fm.RATE_3_4)[0][:8]) == [0, 1, 2, 5, 6, 7, 8, 11]     # A0 B0 A1 B2, A3 B3 A4 B5
    for rate in fm.RATES:
        x = fm.puncture(mother + 1, rate)
        back = fm.depuncture(x, rate)
        assert back.shape == mother.shape and np.array_equal(back[back != 0], x[0])
        assert np.array_equal(back != 0, fm.keep_mask(rate, 24)[None, :])
    for mod, rate in fm.COMBOS:
        T = fm.info_bits(mod, rate)
        assert fm.puncture(np.zeros((1, 2 * T), np.uint8), rate).shape[1] == fm.n_tx(mod)


@pytest.mark.parametrize("mod,rate", fm.COMBOS)
def test_noiseless_round_trip(mod, rate):
    rng = np.random.default_rng(100 * mod + rate)
    for tail in (True, False):
        u = fm.random_info(rng, 3, mod, rate, tail=tail)
        tx, coded = fm.transmit(u, mod, rate)
        L = fm.llr(tx, np.ones_like(tx), mod, real=np.float64)
        assert np.array_equal(L > 0, coded.astype(bool)) and np.all(L != 0)
        sym = dm.slice_points(tx, mod, dm.SCALE)[0]         # b0 is the top bit of the slicer's label
        txb = np.zeros_like(coded)
        txb[:, :, fm.interleave_index(mod)] = coded
        lab = txb.reshape(3, fm.NBLK, 48, mod) @ (1 << np.arange(mod - 1, -1, -1))
        assert np.array_equal(sym[:, :, dm.DATA], lab)
        for terminated in ((True, False) if tail else (False,)):
            for dtype in (np.float32, np.float64):
                assert np.array_equal(fm.decode(L, mod, rate, terminated, dtype), u)
    assert np.array_equal(np.unpackbits(fm.pack(u), axis=1, bitorder="little")[:, :u.shape[1]], u)


# ---------------------------------------------------------------- data conditions
@pytest.mark.parametrize("mod,rate", fm.COMBOS)
def test_clean_set_decodes_clean(mod, rate):
    """(a): every frame, float32 and float64 metrics, terminated; raw symbol errors from QPSK up"""
    s, m = fm.clean_set(mod, rate), fm.clean_model(mod, rate)
    assert s["u"].shape == (67, fm.info_bits(mod, rate)) and not s["u"][:, -6:].any()
    L = np.asarray(m["llr"], np.float64).astype(np.float32)
    for dtype in (np.float32, np.float64):
        assert np.array_equal(fm.decode(L, mod, rate, True, dtype), s["u"]), dtype
    raw = int(m["nerr"].sum())
    print(f"{mod} bits rate {rate}: {raw} raw symbol errors in 67 frames, 0 bit errors")
    assert raw > 0 or mod == dm.BPSK


@pytest.mark.parametrize("mod,rate", fm.COMBOS)
def test_integer_set(mod, rate):
    """(b): integers in [-31, 31], about a tenth zeros; float32 and float64 decodes identical; frames with and
    without errors"""
    s = fm.integer_set(mod, rate)
    L = s["llr"]
    assert L.dtype == np.float32 and np.array_equal(L, np.rint(L)) and np.abs(L).max() <= 31
    assert 0.05 <= np.mean(L == 0) <= 0.15
    assert fm.info_bits(mod, rate) * 2 * 31 < 2 ** 24
    for terminated in (True, False):
        b32, n32 = fm.integer_model(mod, rate, terminated, np.float32)
        b64, n64 = fm.integer_model(mod, rate, terminated, np.float64)
        assert np.array_equal(b32, b64) and np.array_equal(n32, n64)
        print(f"{mod} bits rate {rate} at {fm.int_snr(mod, rate)} dB terminated={terminated}: "
              f"{int((n32 > 0).sum())} of 67 frames with errors, {int(n32.sum())} bit errors")
        assert (n32 > 0).any() and (n32 == 0).any()


@pytest.mark.parametrize("mod", fm.MODS)
def test_llr_bound_is_reachable(mod):
    """(c): the float64 model rounded to float32 meets the bound with a factor 2 to spare; max w S <= 8 max |L|"""
    assert 160 * U <= fm.TOL_ABS / 2
    s = fm.clean_set(mod, fm.RATE_1_2)
    d = dm.spacing(mod, dm.SCALE)
    M = 1 << max(mod // 2, 1)
    worst = ratio = 0.0
    for h_lt in (s["h_lt"], None):
        e64 = dm.demodulate(s["tx"], s["rx"], s["h"], h_lt, mod, real=np.float64)["eq"]
        ld = fm.llr(e64, dm.blend(s["h"], h_lt), mod)
        f64 = fm.llr(e64, dm.blend(s["h"], h_lt, np.float64), mod, real=np.float64)
        assert ld.dtype == np.longdouble and f64.dtype == np.float64
        mx = np.max(np.abs(ld), axis=(1, 2), keepdims=True)
        err64 = np.abs(f64.astype(np.longdouble) - ld) / mx
        err32 = np.abs(f64.astype(np.float32).astype(np.longdouble) - ld)
        assert np.all(2 * err32 <= 2.0 ** -23 * np.abs(ld) + fm.TOL_ABS * mx)
        hu = np.asarray(dm.blend(s["h"], h_lt))[:, :, dm.DATA]
        v = np.asarray(e64, np.clongdouble)[:, :, dm.DATA]
        S = (np.maximum(np.abs(v.real), np.abs(v.imag) if mod > 1 else 0) + (M - 1) * d) ** 2
        wS = np.max((hu.real ** 2 + hu.imag ** 2) * S, axis=(1, 2))
        worst, ratio = max(worst, float(err64.max())), max(ratio, float(np.max(wS / mx[:, 0, 0])))
    print(f"{mod} bits: fp64 model within {worst:.2e} of the frame's max |L|; max w S / max |L| = {ratio:.2f}")
    assert ratio <= 8 and worst <= 20 * 8 * U
