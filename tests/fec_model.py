"""Reference model of the coded receive path (wce_soft_demap, wce_viterbi_decode),
in numpy, and the test data its tests share.  The reference project has no
decoder; the definitions are the ones in include/wce.h (IEEE 802.11-2020
17.3.5.6 and 17.3.5.7):

    code         A_t = u_t ^ u_{t-2} ^ u_{t-3} ^ u_{t-5} ^ u_{t-6}   (133 octal)
                 B_t = u_t ^ u_{t-1} ^ u_{t-2} ^ u_{t-3} ^ u_{t-6}   (171 octal); mother stream A0 B0 A1 B1 ...
    puncturing   rate 2/3 keeps 1 1 1 0, rate 3/4 keeps 1 1 1 0 0 1 of the mother stream
    interleaver  coded bit k -> i = (N_CBPS/16)(k mod 16) + floor(k/16)
                 -> j = s floor(i/s) + (i + N_CBPS - floor(16 i / N_CBPS)) mod s,  s = max(bpsc/2, 1)
    mapping      transmitted bit j: data subcarrier floor(j/bpsc), bit j mod bpsc, b0 first; the first bpsc/2
                 bits give the I level, the rest the Q level, by 802.11's Gray tables
    soft bit     L = |Hu|^2 (D0 - D1), D_c = min over the axis levels whose label bit is c of (v - level)^2;
                 0 for every bit of a symbol whose e or Hu is not finite, else clamped to +-LLR_MAX = 2^100;
                 in deinterleaved coded order
    decoder      maximum-correlation Viterbi over the depunctured stream (0 at the punctured places), 64
                 states, p0 wins a tie, no renormalisation

Nothing here is shared with the kernels: the levels are searched by brute force
and the trellis is built from the generator taps."""
import functools

import numpy as np

import demod_model as dm

LD = np.longdouble
N, NBLK, NDATA = dm.N, dm.NBLK, 48
MODS = dm.MODS
RATE_1_2, RATE_2_3, RATE_3_4 = 0, 1, 2
RATES = (RATE_1_2, RATE_2_3, RATE_3_4)
FRACTION = {RATE_1_2: (1, 2), RATE_2_3: (2, 3), RATE_3_4: (3, 4)}
KEEP = {RATE_1_2: (1, 1), RATE_2_3: (1, 1, 1, 0), RATE_3_4: (1, 1, 1, 0, 0, 1)}
COMBOS = [(m, r) for m in MODS for r in RATES]
TAPS_A = (0, 2, 3, 5, 6)      # 133 octal = 1011011
TAPS_B = (0, 1, 2, 3, 6)      # 171 octal = 1111001
# bound (c) of the GPU tests, derived and checked in tests/test_decode_abi.py:
# |L_dev - L_ld| <= 2^-23 |L_ld| + TOL_ABS max |L_ld| of the frame
TOL_ABS = 1e-13
LLR_MAX = 2.0 ** 100          # WCE_LLR_MAX: a finite soft bit saturates there
# SNR of the integer set per bits per subcarrier (BPSK rate 1/2 runs at INT_SNR_BPSK_1_2: at 6 dB one frame
# of its 67 decodes with errors, at 2 dB 19 do)
INT_SNR = {1: 6.0, 2: 9.0, 4: 14.0, 6: 19.0}
INT_SNR_BPSK_1_2 = 2.0
# the clean set's draw: of the draws 0..3 the first on which all 12 combinations decode without a bit error
# (draws 0 to 2 leave one to four frames of 64-QAM rate 3/4 in a fade the code does not bridge at 25 dB)
CLEAN_SEED = 3


def n_cbps(mod):
    return NDATA * mod


def n_tx(mod):
    return NBLK * n_cbps(mod)


def info_bits(mod, rate):
    num, den = FRACTION[rate]
    return n_tx(mod) * num // den


# ---------------------------------------------------------------- transmitter
def encode(u):
    """information bits [B][T] -> mother stream [B][2T], from state 0"""
    u = np.asarray(u, np.uint8)
    B, T = u.shape
    pad = np.concatenate([np.zeros((B, 6), np.uint8), u], axis=1)
    out = np.zeros((B, 2 * T), np.uint8)
    for taps, off in ((TAPS_A, 0), (TAPS_B, 1)):
        acc = np.zeros((B, T), np.uint8)
        for d in taps:
            acc ^= pad[:, 6 - d:6 - d + T]
        out[:, off::2] = acc
    return out


def keep_mask(rate, n_mother):
    pat = np.array(KEEP[rate], bool)
    assert n_mother % len(pat) == 0
    return np.tile(pat, n_mother // len(pat))


def puncture(mother, rate):
    return mother[:, keep_mask(rate, mother.shape[1])]


def depuncture(x, rate, fill=0):
    """[B][N_TX] -> [B][2T] with `fill` at the punctured places"""
    num, den = FRACTION[rate]
    n_mother = x.shape[1] * num // den * 2
    out = np.full((x.shape[0], n_mother), fill, x.dtype)
    out[:, keep_mask(rate, n_mother)] = x
    return out


def interleave_index(mod):
    """j[k]: where coded bit k of a block is transmitted"""
    n = n_cbps(mod)
    s = max(mod // 2, 1)
    k = np.arange(n)
    i = (n // 16) * (k % 16) + k // 16
    return s * (i // s) + (i + n - (16 * i) // n) % s


def axis_levels(nbits):
    """label (b0 first, as an integer) -> level in units of d, for an axis of nbits bits"""
    M = 1 << nbits
    lev = np.zeros(M, np.int64)
    for i in range(M):
        lev[i ^ (i >> 1)] = 2 * i - (M - 1)
    return lev


def map_bits(tx_bits, mod):
    """transmitted bits [B][15][N_CBPS] -> unit-energy data symbols [B][15][48]"""
    B = tx_bits.shape[0]
    b = tx_bits.reshape(B, NBLK, NDATA, mod).astype(np.int64)
    K = float(dm.spacing(mod, 1.0))
    if mod == 1:
        return ((2 * b[..., 0] - 1) * K).astype(np.complex128)
    h = mod // 2
    w = 1 << np.arange(h - 1, -1, -1)
    lev = axis_levels(h)
    return lev[b[..., :h] @ w] * K + 1j * (lev[b[..., h:] @ w] * K)


def transmit(u, mod, rate):
    """information bits [B][T] -> (tx [B][15][53] scaled by SCALE with pilots and DC, coded bits [B][15][N_CBPS])"""
    coded = puncture(encode(u), rate).reshape(u.shape[0], NBLK, n_cbps(mod))
    txb = np.zeros_like(coded)
    txb[:, :, interleave_index(mod)] = coded
    tx = np.zeros((u.shape[0], NBLK, N), np.complex128)
    tx[:, :, dm.DATA] = map_bits(txb, mod) * dm.SCALE
    tx[:, :, list(dm.PILOTS)] = dm.SCALE * dm.PILOT_SIGN[None, None, :] * dm.POLARITY[None, :, None]
    return tx, coded


def random_info(rng, B, mod, rate, tail=True):
    u = rng.integers(0, 2, (B, info_bits(mod, rate))).astype(np.uint8)
    if tail:
        u[:, -6:] = 0
    return u


def pack(bits):
    """[B][T] -> [B][ceil(T/8)] uint8, LSB first"""
    return np.packbits(np.asarray(bits, np.uint8), axis=1, bitorder="little")


# ---------------------------------------------------------------- soft bits
def llr(eq, hu, mod, scale=dm.SCALE, real=LD):
    """eq, hu [B][15][53] -> L [B][15][N_CBPS] in `real`, deinterleaved order: a brute-force search of the levels"""
    cplx = np.clongdouble if real is LD else np.complex128
    e, H = np.asarray(eq).astype(cplx)[:, :, dm.DATA], np.asarray(hu).astype(cplx)[:, :, dm.DATA]
    d = dm.spacing(mod, scale, real)
    nax = max(mod // 2, 1)
    M = 1 << nax
    level = (2 * np.arange(M) - (M - 1)).astype(real) * d
    label = np.arange(M) ^ (np.arange(M) >> 1)
    with np.errstate(all="ignore"):
        w = H.real ** 2 + H.imag ** 2
        ok = np.isfinite(e.real) & np.isfinite(e.imag) & np.isfinite(H.real) & np.isfinite(H.imag)
        out = np.zeros(e.shape + (mod,), real)
        for ax, v in enumerate((e.real, e.imag)[:1 if mod == 1 else 2]):
            dist = (v[..., None] - level) ** 2
            for j in range(nax):
                one = ((label >> (nax - 1 - j)) & 1).astype(bool)
                d0 = np.min(np.where(one, np.inf, dist), axis=-1)
                d1 = np.min(np.where(one, dist, np.inf), axis=-1)
                out[..., ax * nax + j] = w * (d0 - d1)
        out = np.where(np.isnan(out), real(0), np.clip(out, real(-LLR_MAX), real(LLR_MAX)))   # saturate
        out = np.where(ok[..., None], out, real(0))
    txorder = out.reshape(e.shape[0], NBLK, n_cbps(mod))
    return txorder[:, :, interleave_index(mod)]


# ---------------------------------------------------------------- decoder
@functools.lru_cache(maxsize=None)
def trellis():
    """for every successor state s': predecessors (p0, p1) and the coded bits (A, B) of both branches"""
    s = np.arange(64)
    u = s >> 5
    pred = np.stack([2 * (s & 31), 2 * (s & 31) + 1])
    reg = (u[None, :] << 6) | pred                      # bit 6 = u_t, bit 5 = u_{t-1}, ..., bit 0 = u_{t-6}
    bit = lambda taps: np.bitwise_xor.reduce(np.stack([(reg >> (6 - d)) & 1 for d in taps]), axis=0)
    return pred, bit(TAPS_A), bit(TAPS_B)


def viterbi(mother_llr, terminated=True, dtype=np.float32):
    """depunctured LLRs [B][2T] -> decoded bits [B][T] uint8; metrics in `dtype`"""
    L = np.asarray(mother_llr).astype(dtype)
    L = np.where(np.isfinite(L), L, dtype(0))
    B, T = L.shape[0], L.shape[1] // 2
    pred, cA, cB = trellis()
    sA, sB = (2 * cA - 1).astype(dtype), (2 * cB - 1).astype(dtype)      # [2][64]
    pm = np.full((B, 64), -np.inf, dtype)
    pm[:, 0] = 0
    dec = np.zeros((T, B, 64), bool)
    for t in range(T):
        la, lb = L[:, 2 * t, None], L[:, 2 * t + 1, None]
        c0 = pm[:, pred[0]] + (sA[0] * la + sB[0] * lb)
        c1 = pm[:, pred[1]] + (sA[1] * la + sB[1] * lb)
        dec[t] = c1 > c0
        pm = np.where(dec[t], c1, c0)
        assert pm.dtype == dtype
    s = np.zeros(B, np.int64) if terminated else np.argmax(pm, axis=1)
    bits = np.zeros((B, T), np.uint8)
    rows = np.arange(B)
    for t in range(T - 1, -1, -1):
        bits[:, t] = s >> 5
        s = 2 * (s & 31) + dec[t, rows, s]
    return bits


def decode(llr_blocks, mod, rate, terminated=True, dtype=np.float32):
    """L [B][15][N_CBPS] (deinterleaved) -> bits [B][T]"""
    L = np.asarray(llr_blocks)
    return viterbi(depuncture(L.reshape(L.shape[0], -1), rate), terminated, dtype)


# ---------------------------------------------------------------- test data
def channel(rng, tx, snr_db):
    """demod_model.synthetic's channel on given frames: a 6-tap channel per frame, a residual phase that
    drifts over the blocks, noise at snr_db; h and h_lt the channel plus estimation noise 10 dB below"""
    B = tx.shape[0]
    taps = (rng.standard_normal((B, 6)) + 1j * rng.standard_normal((B, 6))) * np.exp(-0.5 * np.arange(6))
    taps /= np.sqrt(np.sum(np.abs(taps) ** 2, axis=1))[:, None]
    H = taps @ np.exp(-2j * np.pi * np.outer(np.arange(6), np.arange(N) - dm.DC) / 64)
    phi = rng.uniform(-0.5, 0.5, (B, 1)) + rng.uniform(-0.03, 0.03, (B, 1)) * np.arange(NBLK)[None, :]
    sigma = dm.SCALE * 10 ** (-snr_db / 20) / np.sqrt(2)
    noise = lambda shape, s: s * (rng.standard_normal(shape) + 1j * rng.standard_normal(shape))
    rx = H[:, None, :] * tx * np.exp(1j * phi)[:, :, None] + noise(tx.shape, sigma)
    h = H + noise(H.shape, sigma / dm.SCALE / np.sqrt(10))
    h_lt = H + noise(H.shape, sigma / dm.SCALE / np.sqrt(10))
    h_lt[:, dm.DC] = 0
    return rx, h, h_lt


@functools.lru_cache(maxsize=None)
def clean_set(mod, rate, B=67, snr_db=25.0, seed=CLEAN_SEED):
    """set (a): B coded frames (random information bits, six zero tail bits) through the synthetic channel at
    25 dB -> dict u, tx, rx, h, h_lt"""
    rng = np.random.default_rng(0xFEC0 + 256 * seed + 16 * mod + rate)
    u = random_info(rng, B, mod, rate)
    tx, _ = transmit(u, mod, rate)
    rx, h, h_lt = channel(rng, tx, snr_db)
    return {"u": u, "tx": tx, "rx": rx, "h": h, "h_lt": h_lt}


@functools.lru_cache(maxsize=None)
def clean_model(mod, rate, real=np.float64):
    """set (a) through the model's demodulator (tracked, blended) in `real` -> dict eq, hu, nerr (raw symbol
    errors), llr"""
    s = clean_set(mod, rate)
    r = dm.demodulate(s["tx"], s["rx"], s["h"], s["h_lt"], mod, real=real)
    hu = dm.blend(s["h"], s["h_lt"], real)
    return {"eq": r["eq"], "hu": hu, "nerr": r["nerr"], "llr": llr(r["eq"], hu, mod, real=real)}


def int_snr(mod, rate):
    return INT_SNR_BPSK_1_2 if (mod, rate) == (1, RATE_1_2) else INT_SNR[mod]


@functools.lru_cache(maxsize=None)
def integer_set(mod, rate, B=67, snr_db=None):
    """set (b): the soft bits of B coded frames (six zero tail bits) through the synthetic channel at a low SNR
    (int_snr), scaled so that about a tenth of them round to 0, rounded to integers and clipped to [-31, 31]
    -> dict u, llr [B][15][N_CBPS] float32"""
    rng = np.random.default_rng(0x1B00 + 16 * mod + rate)
    u = random_info(rng, B, mod, rate)
    tx, _ = transmit(u, mod, rate)
    rx, h, h_lt = channel(rng, tx, int_snr(mod, rate) if snr_db is None else snr_db)
    r = dm.demodulate(tx, rx, h, h_lt, mod, real=np.float64)
    L = np.asarray(llr(r["eq"], dm.blend(h, h_lt, np.float64), mod, real=np.float64), np.float64)
    g = 0.5 / np.quantile(np.abs(L), 0.10)
    return {"u": u, "llr": np.clip(np.rint(L * g), -31, 31).astype(np.float32)}


@functools.lru_cache(maxsize=None)
def integer_model(mod, rate, terminated, dtype=np.float32):
    s = integer_set(mod, rate)
    bits = decode(s["llr"], mod, rate, terminated, dtype)
    return bits, np.sum(bits != s["u"], axis=1).astype(np.uint32)
