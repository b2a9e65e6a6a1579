"""Reference model of demodulation (wce_demodulate), in numpy, and the test data
its tests share.  The reference project stops at the equalized symbols
(WiFi_Equalization.m); the definition is the one in include/wce.h:

    Hu_b    = h                                             (h_lt None)
            = ((15-(b+1))/15) h_lt + ((b+1)/15) h           (WiFi_Equalization.m:4-5)
    z_b     = sum_{p in 5, 19, 33, 47} rx_b[p] conj(Hu_b[p] tx_b[p]);  theta_b = arg z_b
    r_b     = conj(z_b) / |z_b|     (1 where z_b = 0, and without tracking)
    e_b[k]  = (rx_b[k] / Hu_b[k]) r_b                       (0 at k = 26)
    level   i = clamp(floor(v / (2d) + M/2), 0, M-1), point (2i - (M-1)) d, label i ^ (i >> 1)
    evm     = sqrt(sum |e - ref|^2 / sum |ref|^2) over the 48 x 15 data symbols
    nerr    = data symbols whose label differs from the tx symbol's (a non-finite e counts)

`real` is np.longdouble (the reference) or np.float64 (the same arithmetic in the
device's precision; tests/test_demod_abi.py compares the two)."""
import numpy as np

import cfo_model as cm

LD = np.longdouble
N, NBLK, DC = 53, 15, 26
PILOTS = (5, 19, 33, 47)
DATA = np.array([k for k in range(N) if k not in PILOTS and k != DC])
SCALE = 8.8753                      # inputs.h: amplitude of the BPSK points
BPSK, QPSK, QAM16, QAM64 = 1, 2, 4, 6
MODS = (BPSK, QPSK, QAM16, QAM64)
BAD = 0xFF
# bounds of the GPU tests, derived and checked in tests/test_demod_abi.py
TOL_EQ = 1e-13       # |eq - model| / max |model eq| of the frame
TOL_TH = 1e-13       # |theta - model|, radians
TOL_EVM = 1e-12      # |evm - model| / model
MARGIN = 1e-9        # every coordinate is farther than MARGIN * scale from every slicer boundary
# 802.11 pilot values on subcarriers 5, 19, 33, 47 and the first 15 terms of the polarity sequence p_n
PILOT_SIGN = np.array([1.0, 1.0, 1.0, -1.0])
POLARITY = np.array([1, 1, 1, 1, -1, -1, -1, 1, -1, -1, -1, -1, 1, 1, -1], float)


def _cplx(real):
    return np.clongdouble if real is LD else np.complex128


def levels(modulation):
    """levels per axis"""
    return {BPSK: 2, QPSK: 2, QAM16: 4, QAM64: 8}[modulation]


def spacing(modulation, scale, real=LD):
    """d = scale K, K the double nearest to 1 / sqrt(1, 2, 10, 42)"""
    K = np.float64(1 / np.sqrt(LD({BPSK: 1, QPSK: 2, QAM16: 10, QAM64: 42}[modulation])))
    return real(scale) * real(K)


def _axis(v, M, d):
    """level index of coordinate v (non-finite: 0)"""
    v = np.where(np.isfinite(v), v, 0)
    return np.clip(np.floor(v / (2 * d) + v.dtype.type(M) / 2), 0, M - 1).astype(np.int64)


def slice_points(e, modulation, scale, real=LD):
    """e [..., 53] -> (sym uint8, decided points, margin): per subcarrier the data slicer, BPSK with d = scale on
    the pilots, 0 at DC; margin = each point's distance to the nearest slicer boundary on any axis it is sliced
    on (inf at DC)"""
    e = np.asarray(e).astype(_cplx(real))
    sym = np.zeros(e.shape, np.uint8)
    dec = np.zeros(e.shape, _cplx(real))
    margin = np.full(e.shape, np.inf, real)
    for ks, mod, d in ((DATA, modulation, spacing(modulation, scale, real)), (np.array(PILOTS), BPSK, real(scale))):
        M, v = levels(mod), e[..., ks]
        bounds = (np.arange(1, M) - real(M) / 2) * 2 * d
        ii = _axis(v.real, M, d)
        mg = np.min(np.abs(v.real[..., None] - bounds), axis=-1)
        if mod == BPSK:
            s, p = ii, ((2 * ii - (M - 1)) * d).astype(_cplx(real))
        else:
            iq = _axis(v.imag, M, d)
            s = ((ii ^ (ii >> 1)) << (mod // 2)) | (iq ^ (iq >> 1))
            p = (2 * ii - (M - 1)) * d + 1j * ((2 * iq - (M - 1)) * d)
            mg = np.minimum(mg, np.min(np.abs(v.imag[..., None] - bounds), axis=-1))
        fin = np.isfinite(v.real) & np.isfinite(v.imag)
        sym[..., ks] = np.where(fin, s, BAD)
        dec[..., ks] = p
        margin[..., ks] = np.where(fin, mg, np.inf)
    return sym, dec, margin


def blend(h, h_lt, real=LD):
    """-> Hu [B][15][53]"""
    h = np.asarray(h).astype(_cplx(real))
    if h_lt is None:
        return np.repeat(h[:, None, :], NBLK, axis=1)
    hl = np.asarray(h_lt).astype(_cplx(real))
    b1 = np.arange(1, NBLK + 1)
    wlt, wps = (real(NBLK) - b1.astype(real)) / NBLK, b1.astype(real) / NBLK
    return hl[:, None, :] * wlt[None, :, None] + h[:, None, :] * wps[None, :, None]


def demodulate(tx, rx, h, h_lt=None, modulation=BPSK, scale=SCALE, track=True, ref_tx=True, real=LD):
    """tx, rx [B][15][53], h (and h_lt) [B][53] -> dict: eq, sym, theta, evm, nerr as wce_demodulate defines
    them, in `real`; and what the data conditions read: z [B][15], zabs = sum_p |term_p| [B][15], margin."""
    tx, rx = np.asarray(tx).astype(_cplx(real)), np.asarray(rx).astype(_cplx(real))
    hu = blend(h, h_lt, real)
    P = list(PILOTS)
    with np.errstate(all="ignore"):
        z = np.zeros(rx.shape[:2], _cplx(real))
        zabs = np.zeros(rx.shape[:2], real)
        if track:
            for p in P:
                t = rx[:, :, p] * np.conj(hu[:, :, p] * tx[:, :, p])
                z = z + t
                zabs = zabs + np.abs(t)
        nz = z != 0
        mod = np.where(nz, np.abs(z), 1)
        r = np.where(nz, np.conj(z) / mod, 1)
        theta = np.where(nz, np.arctan2(z.imag, z.real), 0)
        e = rx / hu * r[:, :, None]
        e[:, :, DC] = 0
        sym, dec, margin = slice_points(e, modulation, scale, real)
        tsym, _, tmargin = slice_points(tx, modulation, scale, real)
        ref = (tx if ref_tx else dec)[:, :, DATA]
        ed = e[:, :, DATA]
        dif = ed - ref
        num = np.sum(dif.real ** 2 + dif.imag ** 2, axis=(1, 2))
        den = np.sum(ref.real ** 2 + ref.imag ** 2, axis=(1, 2))
        badsym = sym[:, :, DATA] == BAD
        evm = np.where(badsym.any(axis=(1, 2)), real(np.nan), np.sqrt(num / den))
        nerr = np.sum(badsym | (sym[:, :, DATA] != tsym[:, :, DATA]), axis=(1, 2)).astype(np.uint32)
    return {"eq": e, "sym": sym, "theta": theta, "evm": evm, "nerr": nerr, "z": z, "zabs": zabs,
            "margin": np.minimum(margin, np.where(np.isin(np.arange(N), DATA), tmargin, np.inf))}


def relmax_frames(a, ref):
    """per frame max |a - ref| / max |ref|, in long double"""
    a, ref = np.asarray(a).astype(np.clongdouble), np.asarray(ref).astype(np.clongdouble)
    ax = tuple(range(1, ref.ndim))
    return np.asarray(np.max(np.abs(a - ref), axis=ax) / np.max(np.abs(ref), axis=ax), np.float64)


# ---------------------------------------------------------------- estimators of the model's chain
def lt_ls(tx_pre, rx_pre, real=LD):
    """WiFi_channel_estimation_LT_LS.m: conj(tx) rx / (conj(tx) tx), 0 at DC; [..., 53]"""
    t, r = np.asarray(tx_pre).astype(_cplx(real)), np.asarray(rx_pre).astype(_cplx(real))
    h = np.conj(t) * r / (t.real ** 2 + t.imag ** 2)
    h[..., DC] = 0
    return h


def ps_linear(tx, rx, nblk=4, real=LD):
    """WiFi_channel_estimation_PS_Linear.m: the pilot LS estimates averaged over blocks 0..nblk-1, then
    main.c:86-99's three segments (k < 19, k < 33, the rest; the outer ones extrapolate); [B][53]"""
    tx, rx = np.asarray(tx).astype(_cplx(real)), np.asarray(rx).astype(_cplx(real))
    P = list(PILOTS)
    hp = np.mean(rx[:, :nblk, P] / tx[:, :nblk, P], axis=1)
    k = np.arange(N)
    seg = np.where(k < 19, 0, np.where(k < 33, 1, 2))
    alpha = (k - np.array(P)[seg]).astype(real) / 14
    return hp[:, seg] + (hp[:, seg + 1] - hp[:, seg]) * alpha


# ---------------------------------------------------------------- test data
def constellation(rng, modulation, shape):
    """random points of the unit-energy constellation"""
    M = levels(modulation)
    K = float(spacing(modulation, 1.0))
    re = (2 * rng.integers(0, M, shape) - (M - 1)) * K
    if modulation == BPSK:
        return re.astype(np.complex128)
    return re + 1j * (2 * rng.integers(0, M, shape) - (M - 1)) * K


def synthetic(modulation, B=67, seed=0, snr_db=25.0):
    """B frames of `modulation`: random constellation points x SCALE, the 802.11 pilots, a 6-tap channel per
    frame, a residual phase that drifts over the blocks, noise at snr_db; h and h_lt are the channel plus
    estimation noise 10 dB below the data's.  -> (tx, rx, h, h_lt), complex128"""
    rng = np.random.default_rng(0xDE00 + 16 * modulation + seed)
    tx = constellation(rng, modulation, (B, NBLK, N)) * SCALE
    tx[:, :, list(PILOTS)] = SCALE * PILOT_SIGN[None, None, :] * POLARITY[None, :, None]
    tx[:, :, DC] = 0
    taps = (rng.standard_normal((B, 6)) + 1j * rng.standard_normal((B, 6))) * np.exp(-0.5 * np.arange(6))
    taps /= np.sqrt(np.sum(np.abs(taps) ** 2, axis=1))[:, None]
    k = np.arange(N) - DC
    H = taps @ np.exp(-2j * np.pi * np.outer(np.arange(6), k) / 64)
    phi = rng.uniform(-0.5, 0.5, (B, 1)) + rng.uniform(-0.03, 0.03, (B, 1)) * np.arange(NBLK)[None, :]
    sigma = SCALE * 10 ** (-snr_db / 20) / np.sqrt(2)
    noise = lambda shape, s: s * (rng.standard_normal(shape) + 1j * rng.standard_normal(shape))
    rx = H[:, None, :] * tx * np.exp(1j * phi)[:, :, None] + noise(tx.shape, sigma)
    h = H + noise(H.shape, sigma / SCALE / np.sqrt(10))
    h_lt = H + noise(H.shape, sigma / SCALE / np.sqrt(10))
    h_lt[:, DC] = 0
    return tx, rx, h, h_lt


def recorded(golden):
    """the inputs.h frame and the matlab.mat frame, BPSK: name -> (tx, rx, h, h_lt) with h the model's
    PS_Linear (inputs.h: block 0, as main.c; matlab.mat: the recorded H_EST_PS_Linear) and h_lt the LT_LS"""
    i, m = golden["inputs"], golden["matlab"]
    f64 = lambda a: np.asarray(a).astype(np.complex128)
    tx, rx = i["tx_symb"][None], i["rx_symb"][None]
    out = {"inputs.h": (tx, rx, f64(ps_linear(tx, rx, 1)), f64(lt_ls(i["tx_pre"], i["rx_pre"]))[None])}
    out["matlab.mat"] = (np.ascontiguousarray(m["tx_symb"].T)[None], np.ascontiguousarray(m["rx_symb"].T)[None],
                         m["H_EST_PS_Linear"][None], m["H_EST_LT_LS"][None])
    return out


def all_sets(golden):
    """name -> (tx, rx, h, h_lt, modulation): every data set the parity tests run"""
    out = {n: v + (BPSK,) for n, v in recorded(golden).items()}
    for mod in MODS:
        out[f"synthetic {mod} bits"] = synthetic(mod) + (mod,)
    return out


PHI = np.array([3.1, -3.1, 0.7, -2.0, 3.14159, 1.0, -0.3, 2.5, -3.14159, 0.01, -1.2, 3.0, -3.0, 1.57, -0.9])


def phase_set():
    """the wrap test's set: 5 QPSK frames and the per-block rotations PHI (which include +-3.1, and +-3.14159
    that carry a block's phase across +-pi) -> (tx, rx, h, h_lt, rx with block b turned by PHI[b])"""
    tx, rx, h, h_lt = synthetic(QPSK, 5, seed=7)
    return tx, rx, h, h_lt, rx * np.exp(1j * PHI)[None, :, None]


def wrap(a):
    """an angle difference reduced to [-pi, pi)"""
    return (np.asarray(a, np.longdouble) + np.pi) % (2 * np.pi) - np.pi


# ---------------------------------------------------------------- the residual carrier offset (why tracking exists)
RESIDUAL = 5e-5      # cycles per sample: 500 Hz at 10 MHz


def rotated_packet(m, eps=RESIDUAL):
    """matlab.mat's received field and packet under a carrier offset of eps on one time axis (the field ends
    at sample 0, the packet starts there) -> (rx_lptot, rx_packet), complex128"""
    lp, pk = m["rx_lptot"], m["rx_packet"]
    return (cm.apply_cfo(lp, eps, np.arange(len(lp)) - len(lp)), cm.apply_cfo(pk, eps, np.arange(len(pk))))


def chain(m, rx_lptot, rx_packet, real=LD):
    """the model's receive chain on one packet: front end (cfo_model, no derotation), LT_LS, PS_Linear in
    MATLAB semantics -> (tx, rx [1][15][53], h, h_lt [1][53]) in `real`"""
    z = np.zeros(1)
    tx = cm.blocks(m["tx_packet"][None], z, real=real)
    rx = cm.blocks(np.asarray(rx_packet)[None], z, real=real)
    tp = cm.preamble(m["tx_lptot"][None], z, real=real)[0]
    rp = cm.preamble(np.asarray(rx_lptot)[None], z, real=real)[0]
    return tx, rx, ps_linear(tx, rx, 4, real), lt_ls(tp, rp, real)
