"""Decision-directed estimation (wce_reencode), the parts that need no GPU: the
entry point exists (libwce.so, include/wce.h, the Python mirror and its
keywords), it refuses what the header says it refuses, the model of
tests/reencode_model.py is 802.11's transmitter, the data the GPU tests
(tests/test_reencode_gpu.py) compare on makes their comparisons legitimate, and
the feature earns its place: a second pass on the data-aided estimate removes
more than 40% of the first pass's bit errors at low SNR.

The refusals run here with an opaque non-NULL ctx: every one of them returns
before the ctx is touched, and a context cannot be made without a device.
tests/test_reencode_gpu.py repeats them on an `empty=True` context and checks
that nothing was launched.

Bound on H_dd, |H_dev - H_ld| <= TOL_H max_k |H_ld| of the frame, TOL_H = TOL_EQ =
1e-13.  With u = 2^-53, t_b = conj(x_b) rx_b r_b, S = sum_b |x_b| |rx_b| and
D = sum_b |x_b|^2 of a subcarrier (x^ itself is exact: the definition is in fp64):
  - a complex product rounds three times per part (two products and a sum; an fma
    saves one), so its error is at most 3 sqrt2 u of the product of the moduli;
  - the rotor: cos and sin within two ulp each, 2 sqrt2 u |r|;
  - so |dt_b| <= (3 + 2 + 3) sqrt2 u |x_b| |rx_b| to first order;
  - the 15-term sum adds 14 roundings of partial sums that are at most S per part:
    |dN| <= (8 + 14) sqrt2 u S < 32 u S;
  - D is a sum of non-negative terms, three roundings each and 14 in the sum:
    relative error 17 u; the division rounds once more per part.
  |dH| <= |dN| / D + (|N| / D) 18 u <= 50 u S / D, since |N| <= S.
How S / D of a subcarrier compares with the frame's largest |H_dd| is a data
condition: S / D is about |H[k]| + sigma / |x|, and the frame's strongest
subcarrier is well above the noise.  On every frame of every set used,
S / D <= COND max_k |H_dd| with COND = 4 is checked (measured: at most 1.01), so
|dH| <= 200 u max |H_dd| = 2.2e-14 max |H_dd|, 4.5 times inside TOL_H.

Measured (fp64 model against long double, the five sets of the GPU test, with
and without theta): 8.3e-16 of the frame's max |H_dd|; the test asks for 10 times
inside TOL_H.

Low-SNR sets (seed LOW_SNR_SEED, 67 frames each; bit errors, frames in error):
  QPSK 1/2 at 5 dB:      pass 1 3199 (49), pass 2 1496 (26), ratio 0.47; true bits re-encoded 445
  16-QAM 1/2 at 11 dB:   pass 1 2419 (33), pass 2  990 (21), ratio 0.41; true bits re-encoded 218
  64-QAM 2/3 at 19 dB:   pass 1 2516 (29), pass 2  903 (9),  ratio 0.36; true bits re-encoded 296"""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

import demod_model as dm
import fec_model as fm
import reencode_model as rm

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -53
H_SETS = [(m, fm.RATE_1_2) for m in fm.MODS] + [(dm.QAM64, fm.RATE_3_4)]


# ---------------------------------------------------------------- the entry point
def test_symbol_exported_and_declared(wce):
    lib = wce.load()
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "wce.h")).read(), flags=re.S)
    assert hasattr(lib, "wce_reencode")
    assert re.search(r"\bint\s+wce_reencode\s*\(", hdr)
    params = re.search(r"\bwce_reencode\s*\(([^)]*)\)", hdr).group(1).split(",")
    assert len(params) == len(wce.wce.ABI["wce_reencode"]) == 6
    for name in ("wce_reencode_par", "wce_reencode_out"):
        assert re.search(r"\}\s*%s\s*;" % name, hdr), name
    W = wce.wce
    assert [f[0] for f in W.ReencodePar._fields_] == ["bits", "bits_stride", "modulation", "rate", "scale", "theta"]
    assert [f[0] for f in W.ReencodeOut._fields_] == ["tx", "tx_frame_stride", "tx_block_stride", "h", "h_stride"]
    assert ctypes.sizeof(W.ReencodePar) == 40 and ctypes.sizeof(W.ReencodeOut) == 40


def test_python_keywords(wce):
    C = wce.Context
    re_kw = {"scale": 8.8753, "bits_stride": None, "theta": None, "frames": None, "tx": None, "tx_frame_stride": None,
             "tx_block_stride": wce.NSC, "h": None, "h_stride": wce.NSC, "stream": None}
    p = inspect.signature(C.reencode).parameters
    assert list(p) == ["self", "bits", "n_frames", "modulation", "rate"] + list(re_kw)
    for k, default in re_kw.items():
        assert p[k].default == default, k
    # decode_host: the keywords there were, in their order, then the new ones
    assert list(inspect.signature(C.decode_host).parameters) == [
        "self", "eq", "h", "h_lt", "modulation", "rate", "scale", "terminated", "ref_bits", "dd_iterations", "rx",
        "tx_pilots"]
    p = inspect.signature(C.decode_host).parameters
    assert p["dd_iterations"].default == 0 and p["rx"].default is None and p["tx_pilots"].default is None
    # receive_host keeps its signature (tests/test_decode_abi.py pins its last keywords); the iterated receiver
    # is receive_iterated_host
    assert list(inspect.signature(C.receive_host).parameters)[-3:] == ["decode_rate", "ref_bits", "terminated"]
    p = inspect.signature(C.receive_iterated_host).parameters
    assert list(p)[1:8] == ["tx_packets", "tx_lptot", "rx_packets", "rx_lptot", "demod_source", "decode_rate",
                            "dd_iterations"]
    assert p["dd_iterations"].default == 1


# ---------------------------------------------------------------- refusals
def test_refusals(wce):
    lib, W = wce.load(), wce.wce
    mod, rate, B = dm.QAM16, fm.RATE_3_4, 5
    nby = (fm.info_bits(mod, rate) + 7) // 8
    raw = (ctypes.c_char * 4096)()
    base = (ctypes.addressof(raw) + 15) & ~15          # 16-byte aligned; nothing is read or written there
    ctx = ctypes.c_void_p(base)

    def call(ctx=ctx, p=None, null_p=False, fr=None, null_in=False, out=None, null_out=False, n=B):
        P = W.ReencodePar(base, nby + 3, mod, rate, dm.SCALE, base)
        F = W.Frames(base, base, None, None, 15 * 56 + 3, 56, 0, n, 0, 0)
        O = W.ReencodeOut(base, 15 * 56 + 3, 56, base, 56)
        for s, kv in ((P, p), (F, fr), (O, out)):
            for k, v in (kv or {}).items():
                setattr(s, k, v)
        return lib.wce_reencode(ctx, None if null_p else ctypes.byref(P), None if null_in else ctypes.byref(F), n,
                                None if null_out else ctypes.byref(O), None)

    cases = [("null ctx", dict(ctx=None)), ("null p", dict(null_p=True)), ("null out", dict(null_out=True)),
             ("null bits", dict(p={"bits": None})), ("both outputs null", dict(out={"tx": None, "h": None})),
             ("h without in", dict(null_in=True)), ("h without rx", dict(fr={"rx": None})),
             ("n_frames of in", dict(fr={"n_frames": B + 1})), ("modulation 3", dict(p={"modulation": 3})),
             ("modulation 0", dict(p={"modulation": 0})), ("rate 3", dict(p={"rate": 3})),
             ("rate -1", dict(p={"rate": -1})), ("scale 0", dict(p={"scale": 0.0})),
             ("scale < 0", dict(p={"scale": -1.0})), ("scale nan", dict(p={"scale": float("nan")})),
             ("scale inf", dict(p={"scale": float("inf")})), ("bits_stride", dict(p={"bits_stride": nby - 1})),
             ("tx block stride", dict(out={"tx_block_stride": 52})),
             ("tx frame stride", dict(out={"tx_frame_stride": 14 * 56 + 52})),
             ("in block stride", dict(fr={"block_stride": 52})),
             ("in frame stride", dict(fr={"frame_stride": 14 * 56 + 52})), ("h_stride", dict(out={"h_stride": 52})),
             ("tx alignment", dict(out={"tx": base + 8})), ("h alignment", dict(out={"h": base + 8})),
             ("rx alignment", dict(fr={"rx": base + 8})), ("theta alignment", dict(p={"theta": base + 4})),
             ("n_frames < 0", dict(n=-1)), ("n_frames 2^31", dict(n=2 ** 31))]
    for name, kw in cases:
        assert lib.wce_decode_info_bits(0, 0) == -1                            # leaves its own text behind
        marker = lib.wce_last_error()
        assert call(**kw) == -1, name
        text = lib.wce_last_error()
        assert text and text != marker, name
    # n_frames == 0 is WCE_OK, with and without frames, whatever the strides
    assert call(n=0) == 0 and call(n=0, null_in=True, out={"h": None}) == 0
    assert call(n=0, out={"tx_frame_stride": 0}, fr={"frame_stride": 0}) == 0


# ---------------------------------------------------------------- the model is 802.11's transmitter
@pytest.mark.parametrize("mod,rate", fm.COMBOS)
def test_model_against_transmit(mod, rate):
    rng = np.random.default_rng(900 + 16 * mod + rate)
    u = np.concatenate([fm.random_info(rng, 4, mod, rate, tail=False), rm.impulse_set(mod, rate)])
    tx, coded = fm.transmit(u, mod, rate)
    assert np.array_equal(rm.punctured_stream(u, rate).reshape(coded.shape), coded)
    x = rm.xhat(u, mod, rate)
    assert x.dtype == np.complex128 and x.shape == tx.shape
    # the labels are identical; lev K scale against lev fl(scale K): within one ulp per part
    for part in (np.real, np.imag):
        assert np.all(np.abs(part(x) - part(tx)) <= np.spacing(np.abs(part(tx))))
    assert np.array_equal(dm.slice_points(x, mod, dm.SCALE)[0], dm.slice_points(tx, mod, dm.SCALE)[0])
    assert not x[:, :, dm.DC].any()
    assert np.array_equal(x[:, :, list(dm.PILOTS)], tx[:, :, list(dm.PILOTS)])
    # a re-encoded symbol is the point the slicer decides for it, bit for bit
    dec = np.asarray(dm.slice_points(x, mod, dm.SCALE, np.float64)[1], np.complex128)
    assert np.array_equal(dec.view(np.uint64), x.view(np.uint64))
    # given pilots are copied
    pil = -0.5 * rm.standard_pilots(u.shape[0])
    assert np.array_equal(rm.xhat(u, mod, rate, pilots=pil)[:, :, list(dm.PILOTS)], pil)


def test_impulse_set_catches_the_carries():
    for mod, rate in fm.COMBOS:
        T = fm.info_bits(mod, rate)
        u = rm.impulse_set(mod, rate)
        assert u.shape == (10, T) and list(np.flatnonzero(u[:8].sum(axis=0))) == sorted({0, 25, 31, 32, 63, 64, T - 7, T - 1})
        assert u[8].all() and not u[9].any()
        x = rm.xhat(u, mod, rate)
        assert len({x[i].tobytes() for i in range(10)}) == 10              # every row transmits something else


# ---------------------------------------------------------------- the bound on H_dd
@pytest.mark.parametrize("mod,rate", H_SETS)
def test_h_dd_bound_is_reachable(mod, rate):
    """the fp64 model sits 10 times inside TOL_H of the long double model; S / D <= COND max |H_dd|"""
    assert 50 * rm.COND * U <= rm.TOL_H / 4
    s = fm.clean_set(mod, rate)
    x = rm.xhat(s["u"], mod, rate)
    assert np.array_equal(dm.slice_points(x, mod, dm.SCALE)[0], dm.slice_points(s["tx"], mod, dm.SCALE)[0])
    worst = ratio = 0.0
    exact = s["h"][:, None, :] * x                                          # the set of the exact-channel test
    for rx, theta in ((s["rx"], rm.clean_theta(mod, rate)), (s["rx"], None), (exact, None)):
        ld, cond = rm.h_dd(x, rx, theta)
        f64, _ = rm.h_dd(x, rx, theta, np.float64)
        assert ld.dtype == np.clongdouble and f64.dtype == np.complex128
        assert not ld[:, dm.DC].any() and np.all(np.isfinite(ld.real)) and np.all(np.isfinite(ld.imag))
        worst = max(worst, float(rm.relmax_rows(f64, ld).max()))
        ratio = max(ratio, float(np.max(cond / np.max(np.abs(ld), axis=1, keepdims=True))))
    # with rx = H x^ exactly and no rotation the estimate is H, to the rounding of the products
    h = s["h"].copy()
    h[:, dm.DC] = 0
    assert rm.relmax_rows(rm.h_dd(x, exact)[0], h).max() <= rm.TOL_H / 10
    print(f"{mod} bits rate {rate}: fp64 model within {worst:.2e} of the frame's max |H_dd|; "
          f"max S / D / max |H_dd| = {ratio:.2f}")
    assert ratio <= rm.COND and worst <= rm.TOL_H / 10


# ---------------------------------------------------------------- the feature earns its place
@pytest.mark.parametrize("mod,rate,snr", rm.LOW_SNR)
def test_second_pass_removes_bit_errors(mod, rate, snr):
    s = rm.low_snr_set(mod, rate, snr)
    assert s["u"].shape == (67, fm.info_bits(mod, rate)) and not s["u"][:, -6:].any()
    sigma = dm.SCALE * 10 ** (-snr / 20) / np.sqrt(2)
    dev = np.std((s["h0"] - s["H"]).view(np.float64))                      # the first estimate's noise, per part
    assert abs(dev / (sigma / dm.SCALE / np.sqrt(2)) - 1) < 0.05
    r = rm.two_pass(mod, rate, snr)
    n1, n2, ng = int(r["nbiterr1"].sum()), int(r["nbiterr2"].sum()), int(r["nbiterr_genie"].sum())
    print(f"{mod} bits rate {rate} at {snr} dB: bit errors {n1} -> {n2} (ratio {n2 / max(n1, 1):.2f}), frames in error "
          f"{int((r['nbiterr1'] > 0).sum())} -> {int((r['nbiterr2'] > 0).sum())}; true bits re-encoded: {ng}")
    assert n1 > 0 and n2 <= 0.6 * n1
    assert ng <= n2
