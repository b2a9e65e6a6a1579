"""Reference model of packet detection and symbol timing (wce_front_end_sync),
in numpy, and the test data its tests share.  The reference project declares a
detection threshold (WiFi_RX.m:7) and never uses it; the definition is the one
in include/wce.h:

    c[d] = sum_{n<64}  x[d+n] conj(ltf[n])           0 <= d <= L - 64
    E[d] = sum_{n<128} |x[d+n]|^2,  El = sum |ltf|^2
    M[d] = 2 |c[d]| |c[d+64]| / (El E[d])            0 <= d <= L - 128   (0 where El E[d] == 0)
    d*   = the smallest d attaining max M;  metric = M[d*]
    start = d* - backoff if M[d*] >= threshold and d* - backoff >= 0, else -1

Every sum is taken directly, term by term in ascending n.  `real` is
np.longdouble (the reference) or np.float64 (the same arithmetic in the device's
precision; tests/test_sync_abi.py compares the two)."""
import numpy as np

import cfo_model as cm

LD = np.longdouble
NFFT = 64
TOL_M = 1e-13        # |metric - long double metric|, absolute, on M <= 1 (derived in tests/test_sync_abi.py)
MIN_GAP = 1e-9       # every data set's best-to-second gap exceeds this, so start is compared exactly
ROT = (0.0, 0.002, 0.0077)   # as recorded, 20 kHz and 77 kHz at 10 MHz, cycles per sample


def _cplx(real):
    return np.clongdouble if real is LD else np.complex128


def metric(x, ltf, real=LD):
    """x [B][L], ltf [64] -> M [B][L - 127] in `real`"""
    x = np.asarray(x).astype(_cplx(real))
    l = np.conj(np.asarray(ltf).astype(_cplx(real)))
    L = x.shape[1]
    nc, nm = L - NFFT + 1, L - 2 * NFFT + 1
    c = np.zeros((x.shape[0], nc), _cplx(real))
    for n in range(NFFT):
        c += x[:, n:n + nc] * l[n]
    p = x.real * x.real + x.imag * x.imag
    E = np.zeros((x.shape[0], nm), real)
    for n in range(2 * NFFT):
        E += p[:, n:n + nm]
    El = real(0)
    for v in l:
        El += v.real * v.real + v.imag * v.imag
    den = El * E
    num = 2 * np.abs(c[:, :nm]) * np.abs(c[:, NFFT:NFFT + nm])
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(den == 0, real(0), num / np.where(den == 0, real(1), den))


def sync(x, ltf, threshold, backoff=0, real=LD):
    """-> (start [B] int32, metric [B] float64 rounded from `real`, d* [B]); a window (or an ltf) holding a
    non-finite sample: start -1, metric NaN"""
    x = np.asarray(x)
    M = metric(np.where(np.isfinite(x), x, 0), ltf, real)
    d = np.argmax(M, axis=1)                     # the first maximum
    m = M[np.arange(len(M)), d]
    s = np.where((m >= real(threshold)) & (d - backoff >= 0), d - backoff, -1)
    bad = ~np.isfinite(x).all(axis=1) | ~np.isfinite(np.asarray(ltf)).all()
    return (np.where(bad, -1, s).astype(np.int32), np.where(bad, np.nan, np.asarray(m, np.float64)), d)


def gaps(x, ltf):
    """per frame, max M minus the largest M at any other lag, long double (inf for a single lag)"""
    M = np.array(metric(x, ltf))
    d = np.argmax(M, axis=1)
    best = M[np.arange(len(M)), d].copy()
    M[np.arange(len(M)), d] = -np.inf
    return np.asarray(best - M.max(axis=1), np.float64) if M.shape[1] > 1 else np.full(len(M), np.inf)


# ---------------------------------------------------------------- test data
def clean_ltf():
    """one period of a long training symbol: a fixed +-1 sequence on 52 subcarriers, 64 samples"""
    X = np.zeros(NFFT)
    X[np.r_[1:27, 38:64]] = np.random.default_rng(0x17F).choice([-1.0, 1.0], 52)
    return np.fft.ifft(X)


def fields(rng, B, snr_db, eps, amp=1.0, first_tap=None):
    """B received long training fields [B][128] (two copies) of clean_ltf(): each through a 6-tap channel of
    its own (which acts circularly on a repeated symbol; frames of the mask first_tap: the later taps 20 dB
    down, so that the first path is the strongest), scaled to rms amplitude amp, rotated by eps[f] cycles per
    sample, plus noise at snr_db[f].  Returns (field, sigma [B], the per-sample noise deviation)."""
    h = (rng.standard_normal((B, 6)) + 1j * rng.standard_normal((B, 6))) * np.exp(-0.5 * np.arange(6))
    if first_tap is not None:
        h[first_tap, 1:] *= 0.1
    sym = np.fft.ifft(np.fft.fft(clean_ltf()) * np.fft.fft(h, NFFT, axis=1), axis=1)
    sym *= amp / np.sqrt(np.mean(np.abs(sym) ** 2, axis=1))[:, None]
    f = cm.apply_cfo(np.tile(sym, (1, 2)), np.asarray(eps)[:, None], np.arange(2 * NFFT)[None, :])
    sigma = amp / np.sqrt(2 * 10 ** (np.asarray(snr_db) / 10))
    return f + sigma[:, None] * (rng.standard_normal(f.shape) + 1j * rng.standard_normal(f.shape)), sigma


def forced_positions(rng, B, L):
    """frame 0 (mod 3): lag 0; frame 1: the last lag; frame 2: anywhere"""
    pos = rng.integers(0, L - 2 * NFFT + 1, B)
    pos[0::3] = 0
    pos[1::3] = L - 2 * NFFT
    return pos


def captures(seed, B, L, stride=None, amp=1.0):
    """B capture windows [B][stride] (stride defaults to L + 5; the padding holds SENT): noise, a field of
    `fields` at forced_positions, then packet-like samples at the field's power, 15 ... 40 dB, offsets within
    +-20 kHz.  Returns (capture, pos)."""
    rng = np.random.default_rng(seed)
    stride = L + 5 if stride is None else stride
    snr, eps = rng.uniform(15.0, 40.0, B), rng.uniform(-0.002, 0.002, B)
    f, sigma = fields(rng, B, snr, eps, amp, np.arange(B) % 3 != 2)   # the forced peaks: no later path wins
    pos = forced_positions(rng, B, L)
    cap = np.full((B, stride), SENT, np.complex128)
    cap[:, :L] = cm.random_packets(rng, B, L, 1.0) * sigma[:, None]
    after = cm.random_packets(rng, B, L, amp / np.sqrt(2))
    for b in range(B):
        cap[b, pos[b] + 2 * NFFT:L] += after[b, pos[b] + 2 * NFFT:L]
        cap[b, pos[b]:pos[b] + 2 * NFFT] = f[b]
    return cap, pos


SENT = 7.0 - 3.0j
SHAPES = [(B, L) for B in (1, 9, 777) for L in (128, 129, 191, 192, 488)]


def shape_set(B, L):
    return captures(0x5C00 + 1000 * B + L, B, L)


def recorded(m, prefix):
    """matlab_pins' rx_lptot + rx_packet behind `prefix` noise samples at the packet's own sigma^2, as recorded
    and under ROT: [3][prefix + 1360], and the ltf (tx_lptot[-64:]).  The field's earlier copy starts at
    prefix + 32."""
    rng = np.random.default_rng(0x5C10 + prefix)
    lp, pk = m["rx_lptot"], m["rx_packet"]
    s2 = np.sum(np.abs(lp[-128:-64] - lp[-64:]) ** 2) / 128
    noise = cm.random_packets(rng, 1, prefix, np.sqrt(s2 / 2))[0]
    x = np.concatenate([noise, lp, pk])
    cap = np.stack([cm.apply_cfo(x, e, np.arange(len(x))) for e in ROT])
    return cap, np.ascontiguousarray(m["tx_lptot"][-NFFT:])


def loud_then_quiet(B=4, L=488):
    """200 samples at amplitude 1e3, then a field at amplitude 1e-2 and 30 dB, quiet noise around it"""
    rng = np.random.default_rng(0x5C20)
    f, sigma = fields(rng, B, np.full(B, 30.0), np.zeros(B), 1e-2)
    cap = cm.random_packets(rng, B, L, 1.0) * sigma[:, None]
    cap[:, :200] = cm.random_packets(rng, B, 200, 1e3 / np.sqrt(2))
    pos = rng.integers(200, L - 2 * NFFT + 1, B)
    for b in range(B):
        cap[b, pos[b]:pos[b] + 2 * NFFT] = f[b]
    return cap, pos


def noise_only(B=3, L=488):
    return cm.random_packets(np.random.default_rng(0x5C30), B, L, 1.0)


CHAIN_PREFIX = 37
CHAIN_NOISE = 2      # the chain's window without a packet


def chain(m):
    """B = 5 windows [5][1397] for the whole receive chain: the recorded packet behind 37 noise samples and its
    20 kHz copy, twice over, with one noise-only window (at the packet's sigma^2) in the middle; and the ltf"""
    cap, ltf = recorded(m, CHAIN_PREFIX)
    s2 = np.mean(np.abs(cap[0, :CHAIN_PREFIX]) ** 2)
    noise = cm.random_packets(np.random.default_rng(0x5C40), 1, cap.shape[1], np.sqrt(s2 / 2))[0]
    return np.stack([cap[0], cap[1], noise, cap[1], cap[0]]), ltf


def all_sets(m):
    """name -> (capture [B][L] without padding, ltf): every data set the GPU tests run sync on"""
    out = {}
    for B, L in SHAPES:
        out[f"shape B={B} L={L}"] = (shape_set(B, L)[0][:, :L], clean_ltf())
    for prefix in (0, 37, 100):
        out[f"recorded +{prefix}"] = recorded(m, prefix)
    out["loud then quiet"] = (loud_then_quiet()[0], clean_ltf())
    out["noise only"] = (noise_only(), clean_ltf())
    out["chain"] = chain(m)
    return out
