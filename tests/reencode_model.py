"""Reference model of the re-encoder and the data-aided LS estimate (wce_reencode),
in numpy, and the test data its tests share.  The reference project has neither;
the definition is the one in include/wce.h:

    encoder    from state 0 over the frame's T bits: A_t = u_t ^ u_{t-2} ^ u_{t-3} ^ u_{t-5} ^ u_{t-6},
               B_t = u_t ^ u_{t-1} ^ u_{t-2} ^ u_{t-3} ^ u_{t-6}; mother stream A0 B0 A1 B1 ...
    punctured  rate 2/3 keeps 1 1 1 0, rate 3/4 keeps 1 1 1 0 0 1; coded bit k of block b is bit b N_CBPS + k
    interleave coded bit k is transmitted as bit j(k); data subcarrier floor(j / bpsc) gets bit j mod bpsc, b0 first
    symbol     an axis whose Gray label is g: the level index i with i ^ (i >> 1) = g, coordinate
               fl((2 i - (M - 1)) d), d = fl(scale K); BPSK: Im = 0; DC: 0; pilots given, or 802.11's
    H_dd[k]    = sum_b conj(x_b[k]) rx_b[k] r_b / sum_b |x_b[k]|^2,  r_b = cos theta_b - i sin theta_b,  0 at DC

Nothing here is shared with the kernel or with fec_model's transmitter: the parity
is summed tap by tap, the puncturing walks the pattern, and the levels are found
by searching the Gray table.  `real` is np.longdouble (the reference) or
np.float64 (the same arithmetic in the device's precision)."""
import copy
import functools

import numpy as np

import demod_model as dm
import fec_model as fm

LD = np.longdouble
N, NBLK, DC = dm.N, dm.NBLK, dm.DC
DELAYS = {"A": (0, 2, 3, 5, 6), "B": (0, 1, 2, 3, 6)}          # 133 and 171 octal, as delays of u
PATTERN = {fm.RATE_1_2: "AB", fm.RATE_2_3: "ABA.", fm.RATE_3_4: "ABA..B"}   # kept generators per input bit, '.' dropped
# the bound of the GPU tests on H_dd, derived and checked in tests/test_reencode_abi.py:
# |H_dd - model| <= TOL_H max_k |model H_dd| of the frame, on data with sum_b |x rx| / sum_b |x|^2 <= COND max_k |H_dd|
TOL_H = dm.TOL_EQ
COND = 4.0
# the low-SNR sets: (modulation, rate, SNR in dB); 67 frames each
LOW_SNR = ((dm.QPSK, fm.RATE_1_2, 5.0), (dm.QAM16, fm.RATE_1_2, 11.0), (dm.QAM64, fm.RATE_2_3, 19.0))
LOW_SNR_SEED = 0xDD01


def _cplx(real):
    return np.clongdouble if real is LD else np.complex128


def punctured_stream(u, rate):
    """information bits [B][T] -> the kept coded bits [B][N_TX], the encoder starting in state 0"""
    u = np.asarray(u, np.uint8)
    B, T = u.shape
    past = lambda d: np.concatenate([np.zeros((B, d), np.uint8), u[:, :T - d]], axis=1)   # u_{t-d}
    gen = {}
    for name, delays in DELAYS.items():
        acc = np.zeros((B, T), np.uint8)
        for d in delays:
            acc = acc ^ past(d)
        gen[name] = acc
    pat = PATTERN[rate]
    out = []
    for t in range(T):
        for g in pat[2 * (t % (len(pat) // 2)):2 * (t % (len(pat) // 2)) + 2]:
            if g != ".":
                out.append(gen[g][:, t])
    return np.stack(out, axis=1)


def transmitted_bits(coded, mod):
    """coded bits [B][15][N_CBPS] -> transmitted bits [B][15][N_CBPS]: bit k goes to j(k)"""
    n = coded.shape[-1]
    s = max(mod // 2, 1)
    out = np.zeros_like(coded)
    for k in range(n):
        i = (n // 16) * (k % 16) + k // 16
        j = s * (i // s) + (i + n - 16 * i // n) % s
        out[:, :, j] = coded[:, :, k]
    return out


def axis_coordinate(labels, nbits, d):
    """Gray labels (b0 first, as integers) -> fl((2 i - (M - 1)) d), the level found by search"""
    M = 1 << nbits
    table = [i ^ (i >> 1) for i in range(M)]
    idx = np.array([table.index(g) for g in range(M)])
    return (2 * idx[labels] - (M - 1)).astype(np.float64) * np.float64(d)


def standard_pilots(B, scale=dm.SCALE):
    """[B][15][4]: scale {1, 1, 1, -1} p_b"""
    return np.broadcast_to(np.float64(scale) * dm.PILOT_SIGN[None, :] * dm.POLARITY[:, None], (B, NBLK, 4)).astype(
        np.complex128)


def xhat(u, mod, rate, scale=dm.SCALE, pilots=None):
    """information bits [B][T] -> x^ [B][15][53] complex128 (x^ is defined in fp64); pilots [B][15][4] or 802.11's"""
    u = np.asarray(u, np.uint8)
    B = u.shape[0]
    n = 48 * mod
    txb = transmitted_bits(punctured_stream(u, rate).reshape(B, NBLK, n), mod).reshape(B, NBLK, 48, mod).astype(np.int64)
    d = dm.spacing(mod, scale, np.float64)
    assert type(d) is np.float64
    if mod == dm.BPSK:
        data = axis_coordinate(txb[..., 0], 1, d) + 0j
    else:
        h = mod // 2
        w = 1 << np.arange(h - 1, -1, -1)
        data = axis_coordinate(txb[..., :h] @ w, h, d) + 1j * axis_coordinate(txb[..., h:] @ w, h, d)
    x = np.zeros((B, NBLK, N), np.complex128)
    x[:, :, dm.DATA] = data
    x[:, :, list(dm.PILOTS)] = standard_pilots(B, scale) if pilots is None else pilots
    return x


def h_dd(x, rx, theta=None, real=LD):
    """x^, rx [B][15][53], theta [B][15] or None -> (H_dd [B][53] in `real`, sum_b |x rx| / sum_b |x|^2 [B][53])"""
    x, r = np.asarray(x).astype(_cplx(real)), np.asarray(rx).astype(_cplx(real))
    num = np.zeros((x.shape[0], N), _cplx(real))
    den = np.zeros((x.shape[0], N), real)
    mag = np.zeros((x.shape[0], N), real)
    with np.errstate(all="ignore"):
        for b in range(NBLK):
            t = np.conj(x[:, b]) * r[:, b]
            if theta is not None:
                th = np.asarray(theta)[:, b].astype(real)
                t = t * (np.cos(th) - 1j * np.sin(th))[:, None]
            num = num + t
            den = den + (x[:, b].real ** 2 + x[:, b].imag ** 2)
            mag = mag + np.abs(x[:, b]) * np.abs(r[:, b])
        H = num / den
        cond = mag / den
    H[:, DC] = 0
    cond[:, DC] = 0
    return H, cond


def relmax_rows(a, ref):
    """per frame max_k |a - ref| / max_k |ref|, in long double"""
    a, ref = np.asarray(a).astype(np.clongdouble), np.asarray(ref).astype(np.clongdouble)
    return np.asarray(np.max(np.abs(a - ref), axis=1) / np.max(np.abs(ref), axis=1), np.float64)


# ---------------------------------------------------------------- test data
def impulse_set(mod, rate):
    """information bits that catch carries across words, bytes and blocks: a single 1 at t in {0, 25, 31, 32, 63,
    64, T - 7, T - 1}, all ones, and all zeros -> [10][T]"""
    T = fm.info_bits(mod, rate)
    rows = []
    for t in (0, 25, 31, 32, 63, 64, T - 7, T - 1):
        r = np.zeros(T, np.uint8)
        r[t] = 1
        rows.append(r)
    rows += [np.ones(T, np.uint8), np.zeros(T, np.uint8)]
    return np.stack(rows)


@functools.lru_cache(maxsize=None)
def clean_theta(mod, rate):
    """the clean set's block phases from the model's tracked, blended demodulation in fp64 -> [67][15] float64"""
    s = fm.clean_set(mod, rate)
    return np.asarray(dm.demodulate(s["tx"], s["rx"], s["h"], s["h_lt"], mod, real=np.float64)["theta"], np.float64)


@functools.lru_cache(maxsize=None)
def low_snr_set(mod, rate, snr_db, B=67):
    """B coded frames (six zero tail bits) through fec_model.channel's channel at snr_db, and a first estimate
    h0 = the true channel plus noise of sigma / scale / sqrt 2 per part (the level of LT_LS) -> dict u, tx, rx, h0"""
    rng = np.random.default_rng(LOW_SNR_SEED + 16 * mod + rate)
    u = fm.random_info(rng, B, mod, rate)
    tx, _ = fm.transmit(u, mod, rate)
    # the channel itself: the same draw once more at an SNR whose estimation noise is below an ulp of H
    H = fm.channel(copy.deepcopy(rng), tx, 400.0)[1]
    rx = fm.channel(rng, tx, snr_db)[0]
    sigma = dm.SCALE * 10 ** (-snr_db / 20) / np.sqrt(2)
    h0 = H + sigma / dm.SCALE / np.sqrt(2) * (rng.standard_normal(H.shape) + 1j * rng.standard_normal(H.shape))
    return {"u": u, "tx": tx, "rx": rx, "h0": h0, "H": H}


def _decode_pass(tx, rx, h, mod, rate):
    """tracked, unblended demodulation, soft bits and a terminated decode, in fp64 with float metrics"""
    r = dm.demodulate(tx, rx, h, None, mod, real=np.float64)
    L = np.asarray(fm.llr(r["eq"], dm.blend(h, None, np.float64), mod, real=np.float64), np.float64)
    return fm.decode(L.astype(np.float32), mod, rate, True), np.asarray(r["theta"], np.float64)


@functools.lru_cache(maxsize=None)
def two_pass(mod, rate, snr_db):
    """the low-SNR set through decode -> re-encode -> data-aided LS -> decode again, all in the model
    -> dict nbiterr1, nbiterr2 [67], and nbiterr_genie: the second pass with the true bits re-encoded"""
    s = low_snr_set(mod, rate, snr_db)
    bits1, theta1 = _decode_pass(s["tx"], s["rx"], s["h0"], mod, rate)
    out = {"nbiterr1": np.sum(bits1 != s["u"], axis=1)}
    for name, bits in (("nbiterr2", bits1), ("nbiterr_genie", s["u"])):
        x = xhat(bits, mod, rate)
        H = np.asarray(h_dd(x, s["rx"], theta1, np.float64)[0], np.complex128)
        bits2, _ = _decode_pass(x, s["rx"], H, mod, rate)
        out[name] = np.sum(bits2 != s["u"], axis=1)
    return out
