"""Reference model of the front end's carrier frequency offset correction
(wce_front_end_preamble_cfo, wce_front_end_blocks_cfo), in numpy long double,
and the test data its tests share.  The reference project has no CFO code; the
construction is that of oracle.front_blocks / front_preamble (a direct 64-point
DFT in long double), with the derotation in front of it.

Time axis: sample n counts from the end of the long training field.  lptot[i]
is n = i - len(lptot); packet sample m is n = m + sample_offset.  A frame with
offset eps (cycles per sample) is derotated by exp(-2 pi i frac(eps n)).

Every function takes `real`: np.longdouble (the reference) or np.float64 (the
same arithmetic in the device's precision; tests/test_cfo_abi.py compares the
two)."""
import numpy as np

N, NBLK, NFFT, BLK = 53, 15, 64, 80
LD = np.longdouble
EPS_FIXED = (0.002, -0.002, 0.0077, -0.0077, 0.0)   # 20 kHz and 77 kHz at 10 MHz, both signs, and none
EPS_MAX = 1.0 / 128                                  # the two-copy estimate's range
SNR_FIXED = (60.0, 35.0, 10.0, 45.0, 20.0)           # dB, for the EPS_FIXED frames: both ends of 10 ... 60


def _cplx(real):
    return np.clongdouble if real is LD else np.complex128


def _pi(real):
    return 4 * np.arctan(real(1))   # np.pi is pi rounded to double


def rotor(eps, n, real=LD):
    """exp(-2 pi i frac(eps n)); eps and n broadcast"""
    t = np.asarray(eps, real) * np.asarray(n, real)
    ang = -2 * _pi(real) * (t - np.rint(t))
    return (np.cos(ang) + 1j * np.sin(ang)).astype(_cplx(real))


def _dft_bins(y, real):
    """[..., 64] -> circshift(DFT64, 26)[:53], a direct DFT with exact twiddle arguments"""
    k = (np.arange(N) - 26) % NFFT
    ang = -2 * _pi(real) * np.asarray((np.outer(k, np.arange(NFFT)) % NFFT), real) / NFFT
    W = (np.cos(ang) + 1j * np.sin(ang)).astype(_cplx(real))
    return np.matmul(y.astype(_cplx(real)), W.T)


def blocks(packets, eps, sample_offset=0, n_blocks=NBLK, real=LD):
    """packets [B][>= 80 n_blocks], eps [B] -> symbols [B][n_blocks][53]"""
    pk = np.asarray(packets)[:, :BLK * n_blocks].astype(_cplx(real))
    n = np.arange(BLK * n_blocks) + sample_offset
    y = pk * rotor(np.asarray(eps)[:, None], n[None, :], real)
    return _dft_bins(y.reshape(len(pk), n_blocks, BLK)[:, :, BLK - NFFT:], real)


def estimate(lptot, real=LD):
    """lptot [B][L] -> the two-copy estimate [B], cycles per sample (all-zero field: 0)"""
    lp = np.asarray(lptot).astype(_cplx(real))
    L = lp.shape[1]
    c = np.sum(lp[:, L - NFFT:] * np.conj(lp[:, L - 2 * NFFT:L - NFFT]), axis=1)
    return np.arctan2(c.imag, c.real) / (2 * _pi(real) * NFFT)


def preamble(lptot, eps, real=LD):
    """lptot [B][L], eps [B] -> (pre_fft [B][53], ow2 [B]) from the derotated copies (WiFi_RX.m:24-30)"""
    lp = np.asarray(lptot).astype(_cplx(real))
    L = lp.shape[1]
    y = lp * rotor(np.asarray(eps)[:, None], (np.arange(L) - L)[None, :], real)
    p2, p1 = y[:, L - 2 * NFFT:L - NFFT], y[:, L - NFFT:]
    return _dft_bins((p1 + p2) / 2, real), np.sum(np.abs(p2 - p1) ** 2, axis=1) / (2 * NFFT)


def relmax(a, ref):
    """max |a - ref| / max |ref| over everything, in long double"""
    a, ref = np.asarray(a, np.clongdouble), np.asarray(ref, np.clongdouble)
    return float(np.max(np.abs(a - ref)) / np.max(np.abs(ref)))


def apply_cfo(x, eps, n):
    """x exp(+2 pi i eps n): what an offset of eps does to samples at positions n (rounded from long double)"""
    return (np.asarray(x).astype(np.clongdouble) * np.conj(rotor(eps, n))).astype(np.complex128)


# ---------------------------------------------------------------- test data
def draw_eps(rng, B):
    """frame f < 5: EPS_FIXED[f]; the rest uniform in +-1/128"""
    e = rng.uniform(-EPS_MAX, EPS_MAX, B)
    e[:min(B, 5)] = EPS_FIXED[:B]
    return e


def random_packets(rng, B, stride, scale=0.01):
    return (rng.standard_normal((B, stride)) + 1j * rng.standard_normal((B, stride))) * scale


def ltf_batch(rng, B, L=160, stride=171):
    """B long training fields [B][stride] (only the first L samples belong to the field; the rest is filler
    no call may read into its result): a +-1 sequence on 52 subcarriers, its 64-sample symbol repeated over L
    samples, through a 6-tap channel of its own per frame, rotated by the frame's eps, plus noise at the
    frame's SNR (10 ... 60 dB).  Returns (lptot, eps, snr_db)."""
    eps = draw_eps(rng, B)
    snr = rng.uniform(10.0, 60.0, B)
    snr[:min(B, 5)] = SNR_FIXED[:B]
    X = np.zeros((B, NFFT))
    X[:, np.r_[1:27, 38:64]] = rng.choice([-1.0, 1.0], (B, 52))
    h = (rng.standard_normal((B, 6)) + 1j * rng.standard_normal((B, 6))) * np.exp(-0.5 * np.arange(6))
    sym = np.fft.ifft(X * np.fft.fft(h, NFFT, axis=1), axis=1)          # the channel acts circularly on a repeated symbol
    field = np.tile(sym, (1, 3))[:, 3 * NFFT - L:]                      # ends on a symbol boundary
    field = apply_cfo(field, eps[:, None], (np.arange(L) - L)[None, :])
    p = np.mean(np.abs(field) ** 2, axis=1)
    sigma = np.sqrt(p / 10 ** (snr / 10) / 2)[:, None]
    field = field + sigma * (rng.standard_normal((B, L)) + 1j * rng.standard_normal((B, L)))
    lp = random_packets(rng, B, stride)
    lp[:, :L] = field
    return lp, eps, snr
