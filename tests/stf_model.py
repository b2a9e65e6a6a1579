"""Reference model of the short training field (wce_short_field) and of detection,
coarse carrier offset, timing and the unwrapped fine offset on it
(wce_front_end_sync_stf), in numpy, and the test data their tests share.  The
reference project has neither; the definition is the one in include/wce.h:

    P[d] = sum_{n<128} x[d+n+16] conj(x[d+n]),  A[d] = sum_{n<128} |x[d+n]|^2,  B[d] = A[d+16]   0 <= d <= L - 144
    d_s  = the smallest d attaining max |P|^2;  Ms = |P[d_s]|^2 / (A[d_s] B[d_s])  (0 where the denominator is 0)
    e_c  = arg P[d_s] / (2 pi 16)
    c[d] = sum_{n<64} x[d+n] conj(ltf[n] exp(2 pi i e_c n)),  E, El, M as sync_model's, 0 <= d <= L - 128
    d*   = the smallest d attaining max M;  Ml = M[d*];  s = d* - backoff
    detected iff Ms >= threshold_stf, Ml >= threshold_ltf, s >= 0:  start = s, else -1 and cfo NaN
    e_f  = arg(sum_{n<64} x[s+64+n] conj(x[s+n])) / (2 pi 64);  cfo = e_f + rint((e_c - e_f) 64) / 64

Every sum is taken directly, term by term in ascending n.  `real` is
np.longdouble (the reference) or np.float64 (the same arithmetic in the device's
precision; tests/test_stf_abi.py compares the two and derives the tolerances)."""
import functools

import numpy as np

import cfo_model as cm
import demod_model as dm
import fec_model as fm
import sync_model as sm
import tx_model as tm

LD = np.longdouble
NFFT, STF, PERIOD, SPAN = 64, 160, 16, 128
U = 2.0 ** -53

# derived in tests/test_stf_abi.py
TOL_MS = 2e-13       # |metric_stf - long double|, absolute, on Ms <= 1
TOL_ML = 5e-11       # |metric_ltf - long double|, absolute, on Ml <= 1: carries e_c's rounding
TOL_CFO = 1e-15      # |cfo - long double|, absolute, cycles per sample, on |cfo| < 1/32
TOL_EC = TOL_ML / (4 * 2 * np.pi * 63)   # e_c's share of TOL_ML (half of it, over the sensitivity 2 x 2 pi 63)
TOL_T = 4            # wce_short_field against the long double table, in ulp of amplitude max |t|
MS_MIN = 1e-4        # every window but the all-zero one has Ms above this, which bounds arg P's error
THR_STF = THR_LTF = 0.25
TIE = 1e-9           # lags whose |P|^2 is within this (relative) of the maximum may each be the device's d_s
SHORT_SIGN = (+1, -1, +1, -1, -1, +1, -1, -1, +1, +1, +1, +1)   # k = -24, -20 .. -4, 4 .. 24


def _cplx(real):
    return np.clongdouble if real is LD else np.complex128


# ---------------------------------------------------------------- the transmitter's field
def short_bins(real=LD):
    """S[i], i < 53 (bin k = i - 26): sqrt(13/6) (1 + j) s_k on k = -24, -20 .. 24 without DC"""
    S = np.zeros(53, _cplx(real))
    ks = [k for k in range(-24, 25, 4) if k]
    for k, s in zip(ks, SHORT_SIGN):
        S[k + 26] = np.sqrt(real(13) / real(6)) * s * (1 + 1j)
    return S


def short_period(real=LD):
    """t[0..16): the 64-point inverse DFT (1/64) of short_bins through the library's bin map, its first period"""
    return tm.idft64(short_bins(real)[None, :], real)[0, :PERIOD]


def short_field(amplitude=1.0, real=LD):
    """[160]: amplitude t[m mod 16]"""
    return np.tile(short_period(real), STF // PERIOD) * real(amplitude)


# ---------------------------------------------------------------- the receiver
def detect(x, real=LD):
    """x [B][L] -> (P [B][L-143] complex, A, B [B][L-143]) in `real`"""
    x = np.asarray(x).astype(_cplx(real))
    L = x.shape[1]
    nd = L - SPAN - PERIOD + 1
    q = x[:, PERIOD:] * np.conj(x[:, :L - PERIOD])
    p = x.real * x.real + x.imag * x.imag
    P = np.zeros((x.shape[0], nd), _cplx(real))
    A = np.zeros((x.shape[0], nd + PERIOD), real)
    for n in range(SPAN):
        P += q[:, n:n + nd]
        A += p[:, n:n + nd + PERIOD]
    return P, A[:, :nd], A[:, PERIOD:]


def abs2(z):
    return z.real * z.real + z.imag * z.imag


def stf_metric(P, A, B, d, real=LD):
    """Ms and e_c [B] at lags d [B]"""
    r = np.arange(len(P))
    Pd, den = P[r, d], A[r, d] * B[r, d]
    with np.errstate(divide="ignore", invalid="ignore"):
        ms = np.where(den == 0, real(0), abs2(Pd) / np.where(den == 0, real(1), den))
    return ms, np.arctan2(Pd.imag, Pd.real) / (2 * cm._pi(real) * PERIOD)


def ltf_metric(x, ltf, ec, real=LD):
    """x [B][L], ltf [64], ec [B] -> M [B][L - 127]: sync_model.metric with each frame's template turned by ec"""
    x = np.asarray(x).astype(_cplx(real))
    tl = np.conj(np.asarray(ltf).astype(_cplx(real))[None, :] *
                 np.conj(cm.rotor(np.asarray(ec, real)[:, None], np.arange(NFFT)[None, :], real)))
    L = x.shape[1]
    nc, nm = L - NFFT + 1, L - 2 * NFFT + 1
    c = np.zeros((x.shape[0], nc), _cplx(real))
    for n in range(NFFT):
        c += x[:, n:n + nc] * tl[:, n:n + 1]
    p = x.real * x.real + x.imag * x.imag
    E = np.zeros((x.shape[0], nm), real)
    for n in range(2 * NFFT):
        E += p[:, n:n + nm]
    El = real(0)
    for v in np.asarray(ltf).astype(_cplx(real)):
        El += v.real * v.real + v.imag * v.imag
    den = El * E
    num = 2 * np.abs(c[:, :nm]) * np.abs(c[:, NFFT:NFFT + nm])
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(den == 0, real(0), num / np.where(den == 0, real(1), den))


def analyse(x, ltf, real=LD):
    """everything that does not depend on thresholds and backoff -> dict: ms, ec, d_s, ml, dstar [B], gap [B] (max M
    minus the largest M elsewhere), and what the tie check needs: ms_spread, ec_spread [B] over the lags whose
    |P|^2 is within TIE of the maximum.  Non-finite samples are taken as 0 here; sync_stf marks their frames"""
    x = np.asarray(x)
    xz = np.where(np.isfinite(x), x, 0)
    P, A, B = detect(xz, real)
    pp = abs2(P)
    d_s = np.argmax(pp, axis=1)
    ms, ec = stf_metric(P, A, B, d_s, real)
    r = np.arange(len(xz))
    ms_spread, ec_spread = np.zeros(len(xz)), np.zeros(len(xz))
    near = pp >= pp[r, d_s][:, None] * (1 - real(TIE))
    for f in np.nonzero(near.sum(axis=1) > 1)[0]:
        for d in np.nonzero(near[f])[0]:
            m1, e1 = stf_metric(P[f:f + 1], A[f:f + 1], B[f:f + 1], np.array([d]), real)
            ms_spread[f] = max(ms_spread[f], float(abs(m1[0] - ms[f])))
            ec_spread[f] = max(ec_spread[f], float(abs(e1[0] - ec[f])))
    M = np.array(ltf_metric(xz, ltf, ec, real))
    dstar = np.argmax(M, axis=1)
    ml = M[r, dstar].copy()
    if M.shape[1] > 1:
        M[r, dstar] = -np.inf
        gap = np.asarray(ml - M.max(axis=1), np.float64)
    else:
        gap = np.full(len(xz), np.inf)
    return {"ms": ms, "ec": ec, "d_s": d_s, "ml": ml, "dstar": dstar, "gap": gap, "ms_spread": ms_spread,
            "ec_spread": ec_spread}


def two_copy(x, s, real=LD):
    """frame by frame at s [B] (>= 0): (e_f, |sum| / sum |terms|)"""
    x = np.asarray(x).astype(_cplx(real))
    ef, cond = np.zeros(len(x), real), np.ones(len(x))
    for f in range(len(x)):
        t = x[f, s[f] + NFFT:s[f] + 2 * NFFT] * np.conj(x[f, s[f]:s[f] + NFFT])
        c = _cplx(real)(0)
        for v in t:
            c += v
        ef[f] = np.arctan2(c.imag, c.real) / (2 * cm._pi(real) * NFFT)
        tot = float(np.sum(np.abs(t)))
        cond[f] = float(abs(c)) / tot if tot else 1.0
    return ef, cond


def sync_stf(x, ltf, threshold_stf=THR_STF, threshold_ltf=THR_LTF, backoff=0, real=LD, an=None):
    """-> dict: start int32 [B], cfo, metric_stf, metric_ltf [B] in `real` (NaN as the header says), and ec, ef,
    cond (the two-copy sum's modulus over its terms' moduli), wrap (the fraction of (e_c - e_f) 64) for the
    detected frames; an: analyse(x, ltf, real) if the caller has it"""
    x = np.asarray(x)
    an = analyse(x, ltf, real) if an is None else an
    bad = ~np.isfinite(x).all(axis=1) | ~np.isfinite(np.asarray(ltf)).all()
    s = an["dstar"] - backoff
    det = (an["ms"] >= real(threshold_stf)) & (an["ml"] >= real(threshold_ltf)) & (s >= 0) & ~bad
    sc = np.where(det, s, 0)
    ef, cond = two_copy(np.where(np.isfinite(x), x, 0), sc, real)
    k = (an["ec"] - ef) * 64
    cfo = ef + np.rint(k) / 64
    nan = real(np.nan)
    return {"start": np.where(det, s, -1).astype(np.int32), "cfo": np.where(det, cfo, nan),
            "metric_stf": np.where(bad, nan, an["ms"]), "metric_ltf": np.where(bad, nan, an["ml"]),
            "detected": det, "ec": an["ec"], "ef": ef, "cond": cond, "wrap": np.asarray(k - np.floor(k), np.float64)}


# ---------------------------------------------------------------- test data
EPS = (0.0, 0.002, -0.002, 0.0077, -0.0077, 0.02, -0.02, 0.03, -0.03)   # cycles per sample, frame f: EPS[f % 9]
SNR = (np.inf, 5.0, 10.0, 30.0)                                          # dB, frame f: SNR[(f // 2) % 4]
KINDS = ("first", "last", "short", "cut", "noise", "any", "any")         # frame f: KINDS[f % 7]
P0 = 52.0 / 4096.0                                                       # a packet sample's mean power
PLEN = STF + 160 + 1200


def packets(seed, B, L):
    """B capture windows [B][L] and what was put there -> (capture, info).  A packet is the short field, the long
    field of sync_model.clean_ltf() (32-sample prefix, two copies) and 1,200 Gaussian samples at the fields'
    power, through 1 tap (odd frames) or 6 exponentially decaying taps of unit energy, turned by EPS, placed at
    info["pos"] (clipped to the window) with noise at SNR all over the window (none at all for SNR inf).  Kinds:
    first / last: the packet begins on the window's first sample / ends on its last (a window shorter than the
    packet then holds its end only); short: field and data run past the window's end; cut: 150 of the short
    field's 160 samples lie before the window; noise: no packet (noise at 10 dB under the nominal power when
    its SNR is inf, so that no window here is all-zero); any: somewhere it fits, if it does.  Windows shorter than the
    two fields (320) take 40 dB in place of no noise."""
    rng = np.random.default_rng(seed)
    f = np.arange(B)
    eps = np.array(EPS)[f % 9]
    snr = np.array(SNR)[(f // 2) % 4]
    if L < STF + 160:   # no room for both fields: a noise-free window would hold the periodic short field alone,
        snr = np.where(np.isfinite(snr), snr, 40.0)   # whose M ties from period to period; 40 dB there
    kind = np.array(KINDS)[f % 7]
    ntap = np.where(f % 2 == 1, 1, 6)
    ltf = sm.clean_ltf()
    head = np.concatenate([np.asarray(short_field(1.0), np.complex128), ltf[32:], ltf, ltf])
    cap = np.zeros((B, L), np.complex128)
    pos = np.zeros(B, np.int64)
    for b in range(B):
        data = cm.random_packets(rng, 1, 1200, np.sqrt(P0 / 2))[0]
        h = tm.random_taps(rng, 1, 6)[0] if ntap[b] == 6 else np.exp(2j * np.pi * rng.uniform(size=1))
        y = np.convolve(np.concatenate([head, data]), h)
        y = cm.apply_cfo(y, eps[b], np.arange(len(y)))
        room = L - len(y)
        pos[b] = {"first": 0, "last": room, "short": max(L - (330 if L < 1100 else 700), 0), "cut": -150,
                  "noise": 0, "any": rng.integers(0, room + 1) if room >= 0 else rng.integers(0, max(L - 320, 0) + 1)
                  }[kind[b]]
        s2 = P0 / 10 ** (snr[b] / 10) if np.isfinite(snr[b]) else (P0 / 10 if kind[b] == "noise" else 0.0)
        cap[b] = cm.random_packets(rng, 1, L, np.sqrt(s2 / 2))[0]
        if kind[b] != "noise":
            lo, hi = max(pos[b], 0), min(pos[b] + len(y), L)
            if hi > lo:
                cap[b, lo:hi] += y[lo - pos[b]:hi - pos[b]]
    return cap, {"pos": pos, "eps": eps, "snr": snr, "kind": kind, "ntap": ntap}


def tile_lengths(lags_stf, lags_ltf):
    """window lengths around which the kernel's tile counts change (the first two boundaries of each pass, +-1)"""
    out = set()
    for k in (1, 2):
        for edge in (144 + k * lags_stf, 128 + k * lags_ltf):
            out |= {edge - 1, edge, edge + 1}
    return sorted(out)


BASE_SHAPES = [(144, 1), (145, 5), (191, 777), (488, 67), (1648, 67)]   # (L, B)
TILE_B = 67


@functools.lru_cache(maxsize=None)
def shape_set(L, B):
    """-> (capture [B][L], info, ltf)"""
    cap, info = packets(0x57F0 + 1000 * B + L, B, L)
    return cap, info, sm.clean_ltf()


@functools.lru_cache(maxsize=None)
def shape_model(L, B):
    """the long double analysis of shape_set(L, B), computed once per process"""
    cap, _, ltf = shape_set(L, B)
    return analyse(cap, ltf)


def zeros_set(L=488, B=3):
    return np.zeros((B, L), np.complex128), sm.clean_ltf()


def in_window(info, L):
    """frames whose short and long field lie inside the window whole"""
    return (info["kind"] != "noise") & (info["pos"] >= 0) & (info["pos"] + STF + 160 + 5 <= L)


# ---------------------------------------------------------------- the chain
CHAIN_B, CHAIN_LEN, CHAIN_SNR = 67, 1648, 30.0
CHAIN_MOD, CHAIN_RATE = dm.QPSK, fm.RATE_1_2
CHAIN_SEED = 0x5810   # a seed at which the model detects all 67 and, without the short field, sync_model.sync none
                      # (this preamble's |ltf|^2 is not flat, so at +-0.025 its metric reaches 0.249 and, at three
                      # seeds in four, 0.26 in a frame or two)


def chain_cfo(B=CHAIN_B):
    return np.where(np.arange(B) % 2 == 0, 0.025, -0.025)


def chain_model(tx_pre, taps, seed=CHAIN_SEED, B=CHAIN_B, real=np.float64):
    """link_host(CHAIN_MOD, CHAIN_RATE, CHAIN_SNR, B, taps=taps, cfo=chain_cfo(), stf=True, capture_len=CHAIN_LEN,
    seed=seed) in numpy, LT_LS as the estimate: tx_model's modulator and channel behind the short field,
    sync_stf, cfo_model's field and blocks at its start and offset, demod_model (tracked, no blend),
    fec_model's soft bits and decoder -> dict start, cfo, metric_stf, metric_ltf, gap, nbiterr, bits"""
    T = fm.info_bits(CHAIN_MOD, CHAIN_RATE)
    rng = np.random.default_rng(seed)
    bits = rng.integers(0, 2, (B, T), dtype=np.uint8)
    bits[:, T - 6:] = 0
    tx = fm.transmit(bits, CHAIN_MOD, CHAIN_RATE)[0]
    p = np.abs(np.asarray(tx_pre))
    amp = float(np.sqrt(np.mean(p[p != 0] ** 2)))
    wave = np.concatenate([np.broadcast_to(short_field(amp, real), (B, STF)), tm.modulate(tx, tx_pre, real)], axis=1)
    ow2 = np.full(B, float(tm.nominal_ow2(CHAIN_SNR)))
    cap = np.asarray(tm.channel(wave, CHAIN_LEN, taps, 1, chain_cfo(B), ow2, None, seed, 0, real), np.complex128)
    ltf = np.asarray(tm.idft64(tx_pre, LD), np.complex128)
    an = analyse(cap, ltf, real)
    r = sync_stf(cap, ltf, THR_STF, THR_LTF, 0, real, an)
    start = r["start"]
    ok = start >= 0
    s0 = np.where(ok, start, 0)
    field = np.stack([cap[f, s0[f]:s0[f] + 128] for f in range(B)])
    pk = np.stack([cap[f, s0[f] + 128:s0[f] + 128 + 1200] for f in range(B)])
    eps = np.asarray(np.where(ok, r["cfo"], 0), np.float64)
    rx_pre, _ = cm.preamble(field, eps, real)
    rx = cm.blocks(pk, eps, 0, tm.NBLK, real)
    with np.errstate(invalid="ignore", divide="ignore"):      # DC: 0 / 0, then set to 0
        h = dm.lt_ls(np.broadcast_to(tx_pre, (B, tm.N)), rx_pre, real)
    d = dm.demodulate(tx, rx, h, None, CHAIN_MOD, tm.SCALE, True, True, real)
    dec = fm.decode(fm.llr(d["eq"], dm.blend(h, None, real), CHAIN_MOD, tm.SCALE, real), CHAIN_MOD, CHAIN_RATE)
    return {"start": start, "cfo": np.asarray(r["cfo"], np.float64), "metric_stf": r["metric_stf"],
            "metric_ltf": r["metric_ltf"], "gap": an["gap"], "nbiterr": np.sum(dec != bits, axis=1).astype(np.uint32),
            "bits": bits, "capture": cap, "ltf": ltf, "wrap": r["wrap"]}


def chain_plain(tx_pre, taps, seed=CHAIN_SEED, B=CHAIN_B, real=np.float64):
    """the same packets without the short field through sync_model.sync, today's receiver -> (start, metric)"""
    T = fm.info_bits(CHAIN_MOD, CHAIN_RATE)
    rng = np.random.default_rng(seed)
    bits = rng.integers(0, 2, (B, T), dtype=np.uint8)
    bits[:, T - 6:] = 0
    tx = fm.transmit(bits, CHAIN_MOD, CHAIN_RATE)[0]
    cap = tm.transmit(tx, CHAIN_LEN, tx_pre, real, taps=taps, cfo=chain_cfo(B),
                      ow2=np.full(B, float(tm.nominal_ow2(CHAIN_SNR))), seed=seed)
    start, metric, _ = sm.sync(np.asarray(cap, np.complex128), np.asarray(tm.idft64(tx_pre, LD), np.complex128),
                               THR_LTF, 0, real)
    return start, metric


def chain_taps(seed=CHAIN_SEED, B=CHAIN_B):
    """wce.pdp_taps(default_rng(seed), B, exp(-t), t < 6) without the package: six taps, 4.3 dB a tap, unit energy"""
    rng = np.random.default_rng(seed)
    power = np.exp(-np.arange(6.0))
    h = (rng.standard_normal((B, 6)) + 1j * rng.standard_normal((B, 6))) * np.sqrt(power / 2)
    return h / np.sqrt(np.sum(np.abs(h) ** 2, axis=1, keepdims=True))
