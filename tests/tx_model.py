"""Reference model of the transmitter and the channel (wce_modulate, wce_channel,
wce_transmit), in numpy, and the test data their tests share.  The reference
project has neither: WiFi_RX.m:4-9 declares SNR, channel_model, FO and Pawgn and
uses none of them.  The definitions are those of include/wce.h:

    block     Y[(i - 26) mod 64] = X[i], i < 53;  y[n] = (1/64) sum_k Y[k] e^(+2 pi i k n / 64)
    field     y[32..63], y, y of tx_pre (160 samples);   data block: y[48..63], y (80 samples)
    channel   y[m] = sum_{t ascending} h[t] s[m - t];  r[m] = y[m] exp(+2 pi i cfo (m - 160 field))
              capture[i] = w[i] + r[i - delay] where 0 <= i - delay < wave_len + n_taps - 1
    noise     key = mix64(seed ^ mix64(first_frame + f)); a, b = mix64(key ^ 2i), mix64(key ^ (2i + 1));
              u1 = ((a >> 11) + 1) 2^-53, u2 = (b >> 11) 2^-53;
              w = sqrt(ow2 / 2) sqrt(-2 ln u1) (cos 2 pi u2 + i sin 2 pi u2)

The inverse DFT is a direct sum with exact twiddle arguments, the FIR runs term
by term with t ascending, the rotor is cfo_model.rotor's exact-phase one
conjugated.  `real` is np.longdouble (the reference) or np.float64 (the same
arithmetic in the device's precision; tests/test_transmit_abi.py compares the two
and derives the tolerances below)."""
import ctypes
import functools

import numpy as np

import cfo_model as cm
import demod_model as dm
import fec_model as fm
import sync_model as sm

LD = np.longdouble
N, NBLK, NFFT, BLK, FIELD = 53, 15, 64, 80, 160
U = 2.0 ** -53
SEED = 0x80211
SCALE = dm.SCALE

# derived in tests/test_transmit_abi.py
TOL_WAVE = 1e-14      # |wave - model| / the frame's largest sample
TOL_NOISE = 2e-14     # |w - model| / sqrt(ow2)


def _cplx(real):
    return np.clongdouble if real is LD else np.complex128


# ---------------------------------------------------------------- modulate
def idft64(X, real=LD):
    """[..., 53] bins -> [..., 64] samples"""
    k = (np.arange(N) - 26) % NFFT
    ang = 2 * cm._pi(real) * np.asarray((np.outer(k, np.arange(NFFT)) % NFFT), real) / NFFT
    W = (np.cos(ang) + 1j * np.sin(ang)).astype(_cplx(real))
    return np.matmul(np.asarray(X).astype(_cplx(real)), W) / real(NFFT)


def modulate(sym, tx_pre=None, real=LD):
    """sym [B][n_blocks][53] (n_blocks may be 0), tx_pre None, [53] or [B][53] -> wave [B][160 [field] + 80 n_blocks]"""
    sym = np.asarray(sym)
    B, nb = sym.shape[0], sym.shape[1]
    parts = []
    if tx_pre is not None:
        y = idft64(np.broadcast_to(np.asarray(tx_pre), (B, N)), real)
        parts += [y[:, 32:], y, y]
    if nb:
        y = idft64(sym, real)
        parts.append(np.concatenate([y[:, :, 48:], y], axis=2).reshape(B, nb * BLK))
    return np.concatenate(parts, axis=1)


# ---------------------------------------------------------------- noise
def mix64(x):
    x = np.asarray(x, np.uint64).copy()
    x += np.uint64(0x9E3779B97F4A7C15)
    x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return x ^ (x >> np.uint64(31))


def noise(B, L, ow2, seed=SEED, first_frame=0, real=LD):
    """w [B][L]; ow2 [B] (or a scalar)"""
    f = (np.arange(B, dtype=np.int64) + np.int64(first_frame)).astype(np.uint64)
    key = mix64(np.uint64(seed) ^ mix64(f))[:, None]
    i = np.arange(L, dtype=np.uint64)[None, :]
    a, b = mix64(key ^ (np.uint64(2) * i)), mix64(key ^ (np.uint64(2) * i + np.uint64(1)))
    u1 = ((a >> np.uint64(11)) + np.uint64(1)).astype(real) * real(U)
    u2 = (b >> np.uint64(11)).astype(real) * real(U)
    amp = np.sqrt(np.broadcast_to(np.asarray(ow2, real), (B,)) / 2)[:, None] * np.sqrt(-2 * np.log(u1))
    ang = 2 * cm._pi(real) * u2
    return (amp * np.cos(ang) + 1j * (amp * np.sin(ang))).astype(_cplx(real))


# ---------------------------------------------------------------- channel
def _per_frame(x, B, dtype):
    return None if x is None else np.broadcast_to(np.asarray(x, dtype), (B,))


def channel(wave, capture_len, taps=None, field=1, cfo=None, ow2=None, delay=None, seed=SEED, first_frame=0,
            real=LD):
    """wave [B][wave_len] -> capture [B][capture_len]; taps None, [n_taps] or [B][n_taps]; cfo, ow2, delay None,
    scalars or [B].  A bad frame (include/wce.h's guard) is NaN throughout."""
    s = np.asarray(wave).astype(_cplx(real))
    B, wl = s.shape
    h = np.ones((B, 1)) if taps is None else np.broadcast_to(np.asarray(taps), (B, np.shape(taps)[-1]))
    nt = h.shape[1]
    cfo, ow2, delay = _per_frame(cfo, B, np.float64), _per_frame(ow2, B, np.float64), _per_frame(delay, B, np.int64)
    bad = ~np.isfinite(np.asarray(wave)).all(axis=1) | ~np.isfinite(h).all(axis=1)
    if cfo is not None:
        bad |= ~np.isfinite(cfo)
    if ow2 is not None:
        bad |= ~np.isfinite(ow2) | (ow2 < 0)
    ok = ~bad
    with np.errstate(all="ignore"):
        y = np.zeros((B, wl + nt - 1), _cplx(real))
        hh = h.astype(_cplx(real))
        for t in range(nt):
            y[:, t:t + wl] += hh[:, t:t + 1] * s
        if cfo is not None:
            n = np.arange(wl + nt - 1) - FIELD * int(bool(field))
            rot = np.conj(cm.rotor(np.where(ok, cfo, 0.0)[:, None], n[None, :], real))
            y = np.where((cfo != 0)[:, None], y * rot, y)
        cap = np.zeros((B, capture_len), _cplx(real))
        for f in range(B):
            d = 0 if delay is None else int(delay[f])
            lo, hi = max(d, 0), min(d + wl + nt - 1, capture_len)
            if hi > lo:
                cap[f, lo:hi] = y[f, lo - d:hi - d]
        if ow2 is not None:
            w = noise(B, capture_len, np.where(ok, ow2, 0.0), seed, first_frame, real)
            cap = np.where((ow2 != 0)[:, None], w + cap, cap)
    cap[bad] = np.nan + 1j * np.nan
    return cap


def transmit(sym, capture_len, tx_pre=None, real=LD, **chan):
    return channel(modulate(sym, tx_pre, real), capture_len, field=tx_pre is not None, real=real, **chan)


def relmax_rows(a, ref):
    """per frame max |a - ref| / max |ref|, in long double"""
    a, ref = np.asarray(a).astype(np.clongdouble), np.asarray(ref).astype(np.clongdouble)
    return np.asarray(np.max(np.abs(a - ref), axis=1) / np.max(np.abs(ref), axis=1), np.float64)


def cap_tol(wave, taps, cfo, ref, field=1, with_wave=True):
    """The bound on |capture - model| / the frame's largest clean output `ref` [B][.], per frame: the waveform's
    own error (with_wave: the capture is compared from the symbols on) and n_taps + 2 roundings of the FIR, both
    against sum |h_t| max |s| (what the frame's outputs are made of) over its largest output; the phase term
    2 pi |cfo n| 2^-53 of a rotor whose phase is formed in fp64; 4 roundings for the product."""
    wave = np.asarray(wave)
    B, wl = wave.shape
    h = np.ones((B, 1)) if taps is None else np.broadcast_to(np.asarray(taps), (B, np.shape(taps)[-1]))
    amp = np.sum(np.abs(h), axis=1) * np.max(np.abs(wave), axis=1) / np.max(np.abs(np.asarray(ref)), axis=1)
    tol = ((TOL_WAVE if with_wave else 0.0) + (h.shape[1] + 2) * U) * amp + 4 * U
    if cfo is not None:
        nmax = max(wl + h.shape[1] - 1 - FIELD * int(bool(field)), FIELD)
        tol = tol + 2 * np.pi * np.abs(np.broadcast_to(np.asarray(cfo, float), (B,))) * nmax * U
    return np.asarray(tol, np.float64)


# ---------------------------------------------------------------- test data
def symbols(rng, B, n_blocks, modulation):
    """B frames of n_blocks blocks of `modulation` at SCALE with 802.11's pilots and a zero DC -> [B][n_blocks][53]"""
    x = dm.constellation(rng, modulation, (B, n_blocks, N)) * SCALE
    x[:, :, list(dm.PILOTS)] = SCALE * dm.PILOT_SIGN[None, None, :] * dm.POLARITY[None, :n_blocks, None]
    x[:, :, dm.DC] = 0
    return x


def preambles(rng, B):
    """B preambles [B][53]: +-SCALE on 52 subcarriers, DC 0"""
    p = rng.choice([-SCALE, SCALE], (B, N)).astype(np.complex128)
    p[:, dm.DC] = 0
    return p


def random_taps(rng, B, n_taps):
    """[B][n_taps] complex, an exponential profile (8.7 dB a tap), each frame's of unit energy"""
    h = (rng.standard_normal((B, n_taps)) + 1j * rng.standard_normal((B, n_taps))) * np.exp(-1.0 * np.arange(n_taps))
    return h / np.sqrt(np.sum(np.abs(h) ** 2, axis=1))[:, None]


def padded(a, stride):
    """[B][L] -> [B][stride] with sync_model.SENT behind each row"""
    a = np.asarray(a)
    out = np.full((a.shape[0], stride), sm.SENT, np.complex128)
    out[:, :a.shape[1]] = a
    return out


SHAPES = [(B, nb, field) for B in (1, 9, 67) for nb, field in ((15, 1), (1, 0), (0, 1), (7, 1))]
MODS = (dm.BPSK, dm.QPSK, dm.QAM16, dm.QAM64)


@functools.lru_cache(maxsize=None)
def shape_set(B, n_blocks, field, per_frame_pre=True):
    """the symbols (and preambles) of a shape: frame-strided and block-strided with SENT padding is the caller's
    business; -> (sym [B][n_blocks][53], tx_pre [B][53] or [53] or None)"""
    rng = np.random.default_rng(0x7C00 + 100 * B + 4 * n_blocks + field)
    sym = symbols(rng, B, n_blocks, MODS[(B + n_blocks) % 4])
    pre = None
    if field:
        pre = preambles(rng, B)
        if not per_frame_pre:
            pre = pre[0]
    return sym, pre


NOISE_B, NOISE_L = 67, 1488


def matlab_bins(m):
    """the recording's bins as cfo_model / np.fft extract them: (sym [1][15][53], tx_pre [53])"""
    sym = cm.blocks(m["tx_packet"][None, :], np.zeros(1))
    lp = m["tx_lptot"]
    pre = np.roll(np.fft.fft((lp[32:96] + lp[96:160]) / 2), 26)[:N]
    return np.asarray(sym, np.complex128), pre


# ---- the chain's sets
CHAIN = ((dm.QPSK, fm.RATE_1_2), (dm.QAM16, fm.RATE_1_2), (dm.QAM64, fm.RATE_3_4))
CHAIN_SNR = 30.0
CHAIN_LEN = 1488
CHAIN_SEED = 0x7C66     # a seed whose 15 frames all have the first path strongest (the start is compared exactly)
CHAIN_THRESHOLD = 0.25
# |estimated - given offset|, cycles per sample: the two-copy estimator's deviation at 30 dB is about
# 1 / (2 pi 64 sqrt(64 SNR)) = 1e-5, twice that; the model's own error on these sets is 1.13e-5
# (tests/test_transmit_abi.py), and the device's estimate is the model's to 1e-16
CHAIN_CFO_TOL = 2e-5


def chain_pre():
    """the chain's tx preamble: a fixed +-SCALE sequence on 52 subcarriers"""
    return preambles(np.random.default_rng(CHAIN_SEED), 1)[0]


def nominal_ow2(snr_db, scale=SCALE):
    return (52.0 * scale * scale / 4096.0) / 10.0 ** (np.asarray(snr_db, float) / 10.0)


@functools.lru_cache(maxsize=None)
def chain_set(mod, rate):
    """B = 5 packets of random information bits (six zero tail bits) at nominal 30 dB: six exponential taps,
    offsets within +-20 kHz at 10 MHz, delays 0, 37, 100, the last that fits, 64 -> dict"""
    rng = np.random.default_rng(CHAIN_SEED + 16 * mod + rate)
    B = 5
    u = fm.random_info(rng, B, mod, rate)
    taps = random_taps(rng, B, 6)
    cfo = rng.uniform(-0.002, 0.002, B)
    delay = np.array([0, 37, 100, CHAIN_LEN - 1360 - 5, 64], np.int32)
    return {"bits": u, "taps": taps, "cfo": cfo, "delay": delay, "ow2": np.full(B, float(nominal_ow2(CHAIN_SNR))),
            "seed": CHAIN_SEED + mod}


def chain_capture(mod, rate, tx_pre, real=np.float64):
    c = chain_set(mod, rate)
    tx = fm.transmit(c["bits"], mod, rate)[0]
    return transmit(tx, CHAIN_LEN, tx_pre, real, taps=c["taps"], cfo=c["cfo"], ow2=c["ow2"], delay=c["delay"],
                    seed=c["seed"]), tx


def chain_receive(cap, tx, tx_pre, mod, rate, real=np.float64):
    """the numpy receive chain with LT_LS as the estimate: sync_model.sync -> cfo_model (the two-copy estimate,
    the derotated field and blocks) -> demod_model (tracked, no blend) -> fec_model's soft bits and decoder
    -> dict start, gap, cfo, bits"""
    ltf = np.asarray(idft64(tx_pre, LD), np.complex128)
    cap = np.asarray(cap, np.complex128)
    start, M, _ = sm.sync(cap, ltf, CHAIN_THRESHOLD, 0, real)
    B = len(cap)
    field = np.stack([cap[f, start[f]:start[f] + 128] for f in range(B)])
    pk = np.stack([cap[f, start[f] + 128:start[f] + 128 + 1200] for f in range(B)])
    eps = np.asarray(cm.estimate(field, real), np.float64)
    rx_pre, _ = cm.preamble(field, eps, real)
    rx = cm.blocks(pk, eps, 0, NBLK, real)
    with np.errstate(invalid="ignore", divide="ignore"):      # DC: 0 / 0, then set to 0
        h = dm.lt_ls(np.broadcast_to(tx_pre, (B, N)), rx_pre, real)
    d = dm.demodulate(tx, rx, h, None, mod, SCALE, True, True, real)
    hu = dm.blend(h, None, real)
    bits = fm.decode(fm.llr(d["eq"], hu, mod, SCALE, real), mod, rate)
    return {"start": start, "gap": sm.gaps(cap, ltf), "cfo": eps, "bits": bits}


# ---------------------------------------------------------------- the refusals
# every refusal of the header, for tests/test_transmit_abi.py (opaque pointers) and tests/test_transmit_gpu.py (real ones)
def base_args(W, taps=0x1000, cfo=0x1000, ow2=0x1000, delay=0x1000, pre=0x1000, sym=0x1000, wave=0x1000,
              capture=0x1000, n=3):
    """-> (par, {call: its keyword arguments in the C order, ctx and stream left out}) of three calls that hold"""
    par = lambda **kw: W.ChannelPar(**{**dict(taps=taps, taps_stride=16, n_taps=6, field=1, cfo=cfo, ow2=ow2,
                                              delay=delay, seed=1, first_frame=0), **kw})
    symside = dict(tx_pre=pre, pre_stride=0, sym=sym, frame_stride=15 * 53, block_stride=53, n_blocks=15, n_frames=n)
    return par, {
        "wce_modulate": dict(**symside, wave=wave, wave_stride=1360),
        "wce_channel": dict(wave=wave, wave_stride=1360, wave_len=1360, n_frames=n, p=par(), capture=capture,
                            capture_stride=1488, capture_len=1488),
        "wce_transmit": dict(**symside, p=par(), capture=capture, capture_stride=1488, capture_len=1488)}


def refusals(W, **ptrs):
    """-> list of (call, its arguments with one thing wrong, a piece of the expected text)"""
    par, base = base_args(W, **ptrs)
    a = lambda name: ptrs.get(name, 0x1000)
    sym_side = [({"sym": None}, "sym required"), ({"n_blocks": 16}, "n_blocks outside"),
                ({"n_blocks": -1}, "n_blocks outside"), ({"tx_pre": None, "n_blocks": 0}, "no field and n_blocks == 0"),
                ({"block_stride": 52}, "block_stride < 53"), ({"frame_stride": 14 * 53 + 52}, "frame_stride <"),
                ({"pre_stride": 52}, "pre_stride neither"), ({"tx_pre": a("pre") + 8}, "16-byte"),
                ({"sym": a("sym") + 8}, "16-byte"), ({"n_frames": -1}, "n_frames"), ({"n_frames": 2 ** 31}, "n_frames")]
    chan_side = [({"p": None}, "null parameters"), ({"capture": None}, "null parameters"),
                 ({"p": par(n_taps=0)}, "n_taps outside"), ({"p": par(n_taps=17)}, "n_taps outside"),
                 ({"p": par(taps_stride=5)}, "taps_stride neither"), ({"capture_stride": 1487}, "capture_stride <"),
                 ({"capture_len": 0, "capture_stride": 0}, "capture_len"),
                 ({"capture_len": 2 ** 31, "capture_stride": 2 ** 31}, "capture_len"),
                 ({"capture": a("capture") + 8}, "16-byte"), ({"p": par(taps=a("taps") + 8)}, "16-byte"),
                 ({"p": par(cfo=a("cfo") + 4)}, "8-byte"), ({"p": par(ow2=a("ow2") + 4)}, "8-byte"),
                 ({"p": par(delay=a("delay") + 2)}, "4-byte"), ({"n_frames": -1}, "n_frames"),
                 ({"n_frames": 2 ** 31}, "n_frames")]
    wave_out = [({"wave": None}, "wave required"), ({"wave_stride": 1359}, "wave_stride <"),
                ({"wave": a("wave") + 8}, "16-byte")]
    wave_in = wave_out + [({"wave_len": 0}, "wave_len"), ({"wave_len": 2 ** 31, "wave_stride": 2 ** 31}, "wave_len")]
    out = []
    for name, cases in (("wce_modulate", sym_side + wave_out), ("wce_channel", chan_side + wave_in),
                        ("wce_transmit", sym_side + chan_side)):
        out += [(name, {**base[name], **ch}, text) for ch, text in cases]
    return out


def call_abi(W, lib, ctx, name, kw):
    vals = [ctypes.byref(v) if isinstance(v, W.ChannelPar) else v for v in kw.values()]
    return getattr(lib, name)(ctx, *vals, None)
