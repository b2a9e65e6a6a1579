"""Reference model of the time-varying channel (wce_channel_tv, wce_transmit_tv), in
numpy, and the test data their tests share.  Everything but the FIR is
tests/tx_model.py's: the definitions are those of include/wce.h,

    k = floor(m / P), j = m - k P;   d[k][t] = (a[k+1][t] - a[k][t]) / P   (part by part)
    h_t(m) = (fma(j, d.re, a.re), fma(j, d.im, a.im));   y[m] = sum_{t ascending} h_t(m) s[m - t]

and the rotor, the placement, the clipping and the noise are tx_model.channel's, run on y
with a unit tap (a product with 1 + 0i and a sum with 0: no rounding).

`real` is np.longdouble (the reference) or np.float64.  In fp64 the subtraction and the
division are the device's own.  numpy has no fma; the fp64 tap is formed in long double,
where j d is exact for P <= 2048 (11 + 53 bits), and rounded to fp64 from there: the fma's
single rounding except where the 64-bit sum falls on an fp64 tie.  The sums are numpy's
complex products, as tx_model.channel's: with constant knots the capture is
tx_model.channel's bit for bit, in both precisions.

cap_tol_tv is tx_model.cap_tol with sum_t max_k |a[k][t]| in place of sum |h_t| (a tap
between two knots is no larger than the larger of them) and two more roundings a term for
the interpolated tap (d's subtraction and division count as one each against the tap, the
fma one: (n_taps + 4) u where the static bound has (n_taps + 2) u).
tests/test_fading_abi.py measures the fp64 model against the long-double one under it."""
import functools

import numpy as np

import demod_model as dm
import fec_model as fm
import sync_model as sm
import cfo_model as cm
import track_model as trk
import tx_model as tm

LD = np.longdouble
U = tm.U


def min_knots(wave_len, n_taps, P):
    """the smallest n_knots that covers the output of a waveform of wave_len samples"""
    return (wave_len + n_taps - 2) // P + 2


def _knots(knots, B):
    """[K][nt] or [B][K][nt] -> [B][K][nt] (a view)"""
    a = np.asarray(knots)
    return np.broadcast_to(a, (B,) + a.shape[-2:])


def taps_tv(knots, knot_period, n_out, real=LD):
    """knots [B][K][nt] -> h [B][nt][n_out], the interpolated tap of every output"""
    a = np.asarray(knots)
    P = int(knot_period)
    m = np.arange(n_out)
    k, j = m // P, m % P
    assert a.shape[1] >= 2 and (a.shape[1] - 1) * P > n_out - 1, "the knots do not cover the output"
    out = []
    for part in (a.real, a.imag):
        p = np.asarray(part, real)
        d = (p[:, 1:] - p[:, :-1]) / real(P)                                 # [B][K-1][nt], in `real`
        ak, dk = np.moveaxis(p[:, k], 1, 2), np.moveaxis(d[:, k], 1, 2)       # [B][nt][n_out]
        out.append(np.asarray(np.asarray(j, LD) * dk.astype(LD) + ak.astype(LD), real))
    return (out[0] + 1j * out[1]).astype(tm._cplx(real))


def fir_tv(wave, knots, knot_period, real=LD):
    """wave [B][wl] -> y [B][wl + nt - 1]"""
    s = np.asarray(wave).astype(tm._cplx(real))
    B, wl = s.shape
    a = _knots(knots, B)
    nt = a.shape[2]
    h = taps_tv(a, knot_period, wl + nt - 1, real)
    y = np.zeros((B, wl + nt - 1), tm._cplx(real))
    for t in range(nt):
        y[:, t:t + wl] += h[:, t, t:t + wl] * s
    return y


def channel_tv(wave, capture_len, knots, knot_period, field=1, cfo=None, ow2=None, delay=None, seed=tm.SEED,
               first_frame=0, real=LD):
    """wave [B][wave_len] -> capture [B][capture_len]; knots [K][n_taps] or [B][K][n_taps]; the rest as
    tx_model.channel.  A bad frame (include/wce.h's guard) is NaN throughout."""
    wave = np.asarray(wave)
    B = wave.shape[0]
    a = _knots(knots, B)
    bad = ~np.isfinite(wave).all(axis=1) | ~np.isfinite(a).all(axis=(1, 2))
    with np.errstate(all="ignore"):
        y = fir_tv(np.where(bad[:, None], 0, wave), np.where(bad[:, None, None], 0, a), knot_period, real)
    cap = tm.channel(y, capture_len, None, field, cfo, ow2, delay, seed, first_frame, real)
    cap[bad] = np.nan + 1j * np.nan
    return cap


def transmit_tv(sym, capture_len, knots, knot_period, tx_pre=None, real=LD, **chan):
    return channel_tv(tm.modulate(sym, tx_pre, real), capture_len, knots, knot_period, field=tx_pre is not None,
                      real=real, **chan)


def cap_tol_tv(wave, knots, cfo, ref, field=1, with_wave=True):
    """tx_model.cap_tol for the time-varying channel, per frame (the module's docstring)"""
    wave = np.asarray(wave)
    B, wl = wave.shape
    a = _knots(knots, B)
    nt = a.shape[2]
    amp = np.sum(np.max(np.abs(a), axis=1), axis=1) * np.max(np.abs(wave), axis=1) / \
        np.max(np.abs(np.asarray(ref)), axis=1)
    tol = ((tm.TOL_WAVE if with_wave else 0.0) + (nt + 4) * U) * amp + 4 * U
    if cfo is not None:
        nmax = max(wl + nt - 1 - tm.FIELD * int(bool(field)), tm.FIELD)
        tol = tol + 2 * np.pi * np.abs(np.broadcast_to(np.asarray(cfo, float), (B,))) * nmax * U
    return np.asarray(tol, np.float64)


# ---------------------------------------------------------------- test data
def pdp_taps(rng, n_frames, power):
    """the package's pdp_taps, restated"""
    power = np.asarray(power, np.float64)
    shape = (n_frames, power.size)
    h = (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)) * np.sqrt(power / 2)
    return h / np.sqrt(np.sum(np.abs(h) ** 2, axis=1, keepdims=True))


def fading_taps(rng, n_frames, power, rho, n_knots, normalise=True):
    """the package's fading_taps, restated: knot 0 as pdp_taps, knot k+1 = rho knot k + sqrt(1 - rho^2) CN(0, power)
    c, c the factor that normalised knot 0 (1 with normalise off) -> [n_frames][n_knots][len(power)]"""
    power = np.asarray(power, np.float64)
    shape = (n_frames, power.size)
    h = (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)) * np.sqrt(power / 2)
    nrm = np.sqrt(np.sum(np.abs(h) ** 2, axis=1, keepdims=True)) if normalise else np.ones((n_frames, 1))
    out = np.empty((n_frames, n_knots, power.size), np.complex128)
    out[:, 0] = h / nrm
    for k in range(1, n_knots):
        w = (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)) * np.sqrt(power / 2)
        out[:, k] = rho * out[:, k - 1] + np.sqrt(1.0 - rho * rho) * w * (1.0 / nrm)
    return out


def moving_knots(rng, B, n_knots, n_taps, shared=False):
    """knots for the parity tests: tx_model.random_taps' profile at knot 0, each further knot 0.9 of the one
    before plus an innovation of the same profile (a fast channel: the taps move by half their size a knot)"""
    n = 1 if shared else B
    a = np.empty((n, n_knots, n_taps), np.complex128)
    a[:, 0] = tm.random_taps(rng, n, n_taps)
    for k in range(1, n_knots):
        a[:, k] = 0.9 * a[:, k - 1] + 0.44 * tm.random_taps(rng, n, n_taps)
    return a[0] if shared else a


def padded_knots(a, knot_stride, frame_stride):
    """[B][K][nt] -> [B][frame_stride] with sync_model.SENT in every gap"""
    B, K, nt = a.shape
    out = np.full((B, frame_stride), sm.SENT, np.complex128)
    for k in range(K):
        out[:, k * knot_stride:k * knot_stride + nt] = a[:, k]
    return out


# ---------------------------------------------------------------- the refusals
# every refusal of the header, for tests/test_fading_abi.py (opaque pointers) and tests/test_fading_gpu.py (real ones)
CALLS = ("wce_channel_tv", "wce_transmit_tv")


def base_args(W, knots=0x1000, cfo=0x1000, ow2=0x1000, delay=0x1000, pre=0x1000, sym=0x1000, wave=0x1000,
              capture=0x1000, n=3):
    """-> (par, {call: its keyword arguments in the C order, ctx and stream left out}) of two calls that hold"""
    par = lambda **kw: W.FadingPar(**{**dict(knots=knots, frame_stride=19 * 16, knot_stride=16, n_knots=19,
                                             knot_period=80, n_taps=6, field=1, cfo=cfo, ow2=ow2, delay=delay, seed=1,
                                             first_frame=0), **kw})
    symside = dict(tx_pre=pre, pre_stride=0, sym=sym, frame_stride=15 * 53, block_stride=53, n_blocks=15, n_frames=n)
    return par, {
        "wce_channel_tv": dict(wave=wave, wave_stride=1360, wave_len=1360, n_frames=n, p=par(), capture=capture,
                               capture_stride=1488, capture_len=1488),
        "wce_transmit_tv": dict(**symside, p=par(), capture=capture, capture_stride=1488, capture_len=1488)}


def refusals(W, **ptrs):
    """-> list of (call, its arguments with one thing wrong, a piece of the expected text): the static calls'
    (tx_model.refusals, those that do not concern taps) and the knots'"""
    par, base = base_args(W, **ptrs)
    a = lambda name: ptrs.get(name, 0x1000)
    sym_side = [({"sym": None}, "sym required"), ({"n_blocks": 16}, "n_blocks outside"),
                ({"n_blocks": -1}, "n_blocks outside"), ({"tx_pre": None, "n_blocks": 0}, "no field and n_blocks == 0"),
                ({"block_stride": 52}, "block_stride < 53"), ({"frame_stride": 14 * 53 + 52}, "frame_stride <"),
                ({"pre_stride": 52}, "pre_stride neither"), ({"tx_pre": a("pre") + 8}, "16-byte"),
                ({"sym": a("sym") + 8}, "16-byte"), ({"n_frames": -1}, "n_frames"), ({"n_frames": 2 ** 31}, "n_frames")]
    chan_side = [({"p": None}, "null parameters"), ({"capture": None}, "null parameters"),
                 ({"p": par(n_taps=0)}, "n_taps outside"), ({"p": par(n_taps=17, knot_stride=17)}, "n_taps outside"),
                 ({"capture_stride": 1487}, "capture_stride <"),
                 ({"capture_len": 0, "capture_stride": 0}, "capture_len"),
                 ({"capture_len": 2 ** 31, "capture_stride": 2 ** 31}, "capture_len"),
                 ({"capture": a("capture") + 8}, "16-byte"),
                 ({"p": par(cfo=a("cfo") + 4)}, "8-byte"), ({"p": par(ow2=a("ow2") + 4)}, "8-byte"),
                 ({"p": par(delay=a("delay") + 2)}, "4-byte"), ({"n_frames": -1}, "n_frames"),
                 ({"n_frames": 2 ** 31}, "n_frames")]
    knot_side = [({"p": par(knots=None)}, "knots required"), ({"p": par(knots=a("knots") + 8)}, "knots not 16-byte"),
                 ({"p": par(n_knots=1)}, "n_knots < 2"), ({"p": par(n_knots=-3)}, "n_knots < 2"),
                 ({"p": par(knot_period=15, n_knots=200)}, "knot_period outside"),
                 ({"p": par(knot_period=2 ** 20 + 1)}, "knot_period outside"),
                 ({"p": par(knot_stride=5)}, "knot_stride < n_taps"),
                 ({"p": par(frame_stride=18 * 16 + 5)}, "frame_stride neither"),
                 ({"p": par(frame_stride=-1)}, "frame_stride neither"),
                 # 18 segments of 80 reach sample 1,439: 1,360 + 6 - 2 = 1,364 is covered, with one knot fewer
                 # (1,360) or a period of 75 (1,350) it is not; exactly reaching the last output is not enough
                 ({"p": par(n_knots=18, frame_stride=18 * 16)}, "do not cover"),
                 ({"p": par(knot_period=75)}, "do not cover"),
                 ({"p": par(knot_period=682, n_knots=3)}, "do not cover")]
    wave_in = [({"wave": None}, "wave required"), ({"wave_stride": 1359}, "wave_stride <"),
               ({"wave": a("wave") + 8}, "16-byte"), ({"wave_len": 0}, "wave_len"),
               ({"wave_len": 2 ** 31, "wave_stride": 2 ** 31}, "wave_len")]
    out = []
    for name, cases in (("wce_channel_tv", chan_side + knot_side + wave_in),
                        ("wce_transmit_tv", sym_side + chan_side + knot_side)):
        out += [(name, {**base[name], **ch}, text) for ch, text in cases]
    return out


def call_abi(W, lib, ctx, name, kw):
    import ctypes
    vals = [ctypes.byref(v) if isinstance(v, W.FadingPar) else v for v in kw.values()]
    return getattr(lib, name)(ctx, *vals, None)


# ---- the link experiment: 16-QAM rate 1/2 at nominal 22 dB through six taps that fade by rho a block
LINK_B, LINK_MOD, LINK_RATE, LINK_SNR = 67, dm.QAM16, fm.RATE_1_2, 22.0
LINK_P, LINK_KNOTS, LINK_RHO = 80, 19, 0.995
LINK_POWER = np.exp(-0.5 * np.arange(6)) ** 2      # amplitudes exp(-0.5 t)
LINK_LEN, LINK_SEED = 1488, 0xFAD1
LINK_MU, LINK_BETA = trk.MU, trk.BETA


@functools.lru_cache(maxsize=None)
def link_set(rho=LINK_RHO):
    """what Context.link_host is given, and what it draws itself from the seed (the bits) -> dict"""
    rng = np.random.default_rng(LINK_SEED)
    taps = fading_taps(rng, LINK_B, LINK_POWER, rho, LINK_KNOTS)
    cfo = rng.uniform(-0.002, 0.002, LINK_B)
    delay = rng.integers(0, 100, LINK_B).astype(np.int32)
    T = fm.info_bits(LINK_MOD, LINK_RATE)
    bits = np.random.default_rng(LINK_SEED).integers(0, 2, (LINK_B, T), dtype=np.uint8)     # link_host's draw
    bits[:, T - 6:] = 0
    return {"taps": taps, "cfo": cfo, "delay": delay, "bits": bits, "ow2": float(tm.nominal_ow2(LINK_SNR)),
            "seed": LINK_SEED}


@functools.lru_cache(maxsize=None)
def link_model(rho=LINK_RHO, real=np.float64):
    """link_set through the model: transmit_tv, then tx_model.chain_receive's steps to the LT_LS estimate, then the
    tracked run (track_model.track, soft bits on h_blocks, Viterbi) and the static one (demod_model.demodulate,
    soft bits on h) -> dict start [B], tracked, static (bit errors [B])"""
    c = link_set(rho)
    mod, rate, B = LINK_MOD, LINK_RATE, LINK_B
    pre = tm.chain_pre()
    tx = fm.transmit(c["bits"], mod, rate)[0]
    cap = np.asarray(transmit_tv(tx, LINK_LEN, c["taps"], LINK_P, pre, real, cfo=c["cfo"], ow2=c["ow2"],
                                 delay=c["delay"], seed=c["seed"]), np.complex128)
    ltf = np.asarray(tm.idft64(pre, LD), np.complex128)
    start, _, _ = sm.sync(cap, ltf, tm.CHAIN_THRESHOLD, 0, real)
    if np.any(start < 0):
        return {"start": start}
    field = np.stack([cap[f, start[f]:start[f] + 128] for f in range(B)])
    pk = np.stack([cap[f, start[f] + 128:start[f] + 128 + 1200] for f in range(B)])
    eps = np.asarray(cm.estimate(field, real), np.float64)
    rx_pre, _ = cm.preamble(field, eps, real)
    rx = cm.blocks(pk, eps, 0, tm.NBLK, real)
    with np.errstate(invalid="ignore", divide="ignore"):      # DC: 0 / 0, then set to 0
        h = dm.lt_ls(np.broadcast_to(pre, (B, tm.N)), rx_pre, real)
    t = trk.track(tx, rx, h, mod, LINK_MU, LINK_BETA, real=real)
    d = dm.demodulate(tx, rx, h, None, mod, tm.SCALE, True, True, real)
    out = {"start": start}
    for name, eq, hu in (("tracked", t["eq"], t["h_blocks"]), ("static", d["eq"], dm.blend(h, None, real))):
        L = np.asarray(fm.llr(eq, hu, mod, tm.SCALE, real), np.float64).astype(np.float32)
        out[name] = np.sum(fm.decode(L, mod, rate) != c["bits"], axis=1).astype(np.uint32)
    return out
