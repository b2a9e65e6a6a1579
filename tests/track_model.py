"""Reference model of the per-block decision-directed tracker (wce_track_demodulate),
in numpy, and the drifting-channel data its tests share.  The definition is the one
in include/wce.h ("spectral temporal averaging": Fernandez et al., IEEE Trans. Veh.
Technol., 2012), frame by frame from H_0 = h, V = {0..52} without 26, b = 0..14:

    z_b, theta_b, r_b  demod_model's, with Hu_b = H_b
    e_b[k]   = (rx_b[k] / H_b[k]) r_b                     (0 at k = 26)
    dec_b    = the slicer's decided point of e_b          (demod_model.slice_points)
    x^_b[k]  = tx_b[k] on the pilots (and everywhere with known_tx), else dec_b[k]
    G_b[k]   = rx_b[k] r_b / x^_b[k]                      (k in V)
    S_b[k]   = sum of G_b[j] over N_k = {j in V : |j - k| <= beta}, divided by |N_k|
    H_{b+1}  = H_b + mu (S_b - H_b) on V                  (mu = 0: no update; entry 26 carried)

`real` is np.longdouble (the reference) or np.float64 (the same arithmetic in the
device's precision; tests/test_track_abi.py compares the two)."""
import functools

import numpy as np

import demod_model as dm

LD = np.longdouble
N, NBLK, DC = dm.N, dm.NBLK, dm.DC
V = np.array([k for k in range(N) if k != DC])
# bounds of the GPU tests, derived and checked in tests/test_track_abi.py
TOL_EQ_T = 1e-12     # |eq - model| / max |model eq| of the frame
TOL_H_T = 1e-13      # |h_blocks - model| / max |model H| of the frame (h_last likewise)
TOL_TH = dm.TOL_TH   # |theta - model|, radians
TOL_EVM_T = 1e-11    # |evm - model| / model
# the drifting sets: (modulation, SNR in dB) at RHO
SETS = ((dm.BPSK, 10.0), (dm.QPSK, 15.0), (dm.QAM16, 22.0), (dm.QAM64, 28.0))
RHO = 0.995
MU, BETA = 0.5, 2    # the operating point the tests and the documentation quote


def window(beta):
    """-> (W [53][53] of 0 / 1: W[k][j] = 1 where j is in N_k, |N_k| [53]); row 26 is empty"""
    k = np.arange(N)
    W = (np.abs(k[:, None] - k[None, :]) <= beta) & (k[None, :] != DC) & (k[:, None] != DC)
    return W.astype(np.int64), W.sum(axis=1)


def smooth(G, beta, real=LD):
    """S [..., 53] of G [..., 53]: the window mean over N_k, summed in ascending j; 0 at k = 26"""
    cplx = dm._cplx(real)
    G = np.asarray(G).astype(cplx)
    W, cnt = window(beta)
    S = np.zeros(G.shape, cplx)
    for o in range(-beta, beta + 1):
        for k in V:
            j = k + o
            if 0 <= j < N and W[k, j]:
                S[..., k] = S[..., k] + G[..., j]
    S[..., V] = S[..., V] / cnt[V].astype(real)
    return S


def track(tx, rx, h, modulation=dm.BPSK, mu=MU, beta=BETA, scale=dm.SCALE, phase=True, ref_tx=True, known_tx=False,
          real=LD):
    """tx, rx [B][15][53], h [B][53] -> dict: eq, sym, theta, evm, nerr as wce_track_demodulate defines them, in
    `real`; h_blocks [B][15][53] (H_b, what block b was equalized with), h_last [B][53] (H_15); and what the
    data conditions read: z, zabs [B][15], margin [B][15][53]."""
    cplx = dm._cplx(real)
    tx, rx = np.asarray(tx).astype(cplx), np.asarray(rx).astype(cplx)
    H = np.asarray(h).astype(cplx).copy()
    B = rx.shape[0]
    P = list(dm.PILOTS)
    mu = real(mu)
    e = np.zeros(rx.shape, cplx)
    hb = np.zeros(rx.shape, cplx)
    z = np.zeros((B, NBLK), cplx)
    zabs = np.zeros((B, NBLK), real)
    with np.errstate(all="ignore"):
        for b in range(NBLK):
            hb[:, b] = H
            zb = np.zeros(B, cplx)
            za = np.zeros(B, real)
            if phase:
                for p in P:
                    t = rx[:, b, p] * np.conj(H[:, p] * tx[:, b, p])
                    zb = zb + t
                    za = za + np.abs(t)
            z[:, b], zabs[:, b] = zb, za
            nz = zb != 0
            r = np.where(nz, np.conj(zb) / np.where(nz, np.abs(zb), 1), 1)
            eb = rx[:, b] / H * r[:, None]
            eb[:, DC] = 0
            e[:, b] = eb
            if mu == 0:
                continue
            xh = tx[:, b].copy()
            if not known_tx:
                dec = dm.slice_points(eb, modulation, scale, real)[1]
                xh[:, dm.DATA] = dec[:, dm.DATA]
            G = np.zeros(eb.shape, cplx)
            G[:, V] = rx[:, b][:, V] * r[:, None] / xh[:, V]
            S = smooth(G, beta, real)
            Hn = H.copy()
            Hn[:, V] = H[:, V] + mu * (S[:, V] - H[:, V])
            H = Hn
        nzz = z != 0
        theta = np.where(nzz, np.arctan2(z.imag, z.real), 0)
        sym, dec, margin = dm.slice_points(e, modulation, scale, real)
        tsym, _, tmargin = dm.slice_points(tx, modulation, scale, real)
        ref = (tx if ref_tx else dec)[:, :, dm.DATA]
        dif = e[:, :, dm.DATA] - ref
        num = np.sum(dif.real ** 2 + dif.imag ** 2, axis=(1, 2))
        den = np.sum(ref.real ** 2 + ref.imag ** 2, axis=(1, 2))
        badsym = sym[:, :, dm.DATA] == dm.BAD
        evm = np.where(badsym.any(axis=(1, 2)), real(np.nan), np.sqrt(num / den))
        nerr = np.sum(badsym | (sym[:, :, dm.DATA] != tsym[:, :, dm.DATA]), axis=(1, 2)).astype(np.uint32)
    return {"eq": e, "sym": sym, "theta": theta, "evm": evm, "nerr": nerr, "h_blocks": hb, "h_last": H,
            "z": z, "zabs": zabs,
            "margin": np.minimum(margin, np.where(np.isin(np.arange(N), dm.DATA), tmargin, np.inf))}


# ---------------------------------------------------------------- test data
def drifting(mod, B=67, seed=0, snr_db=25.0, rho=RHO, L=6, tx=None):
    """B frames of `mod` over a channel that moves inside the frame: L taps of an exponential power-delay
    profile, each a Gauss-Markov process with per-block correlation rho; a residual phase that drifts over the
    blocks; noise at snr_db.  h is the channel before block 0 plus the noise of a long-training estimate.
    tx given ([B][15][53], e.g. coded frames): it is sent in place of the random points, which are still drawn.
    -> (tx, rx [B][15][53], h [B][53]), complex128"""
    rng = np.random.default_rng(0x7AC0 + 16 * mod + seed)
    drawn = dm.constellation(rng, mod, (B, NBLK, N)) * dm.SCALE
    tx = drawn if tx is None else np.array(tx, np.complex128)
    tx[:, :, list(dm.PILOTS)] = dm.SCALE * dm.PILOT_SIGN[None, None, :] * dm.POLARITY[None, :, None]
    tx[:, :, DC] = 0
    pdp = np.exp(-0.5 * np.arange(L))
    pdp /= np.sqrt(np.sum(pdp ** 2))
    cn = lambda s: (rng.standard_normal(s) + 1j * rng.standard_normal(s)) / np.sqrt(2)
    F = np.exp(-2j * np.pi * np.outer(np.arange(L), np.arange(N) - DC) / 64)
    t = cn((B, L)) * pdp
    H0 = t @ F
    Hb = np.empty((B, NBLK, N), np.complex128)
    for b in range(NBLK):
        t = rho * t + np.sqrt(1 - rho ** 2) * cn((B, L)) * pdp
        Hb[:, b] = t @ F
    phi = rng.uniform(-.5, .5, (B, 1)) + rng.uniform(-.03, .03, (B, 1)) * np.arange(NBLK)
    sigma = dm.SCALE * 10 ** (-snr_db / 20)
    rx = Hb * tx * np.exp(1j * phi)[:, :, None] + sigma * cn(tx.shape)
    h = H0 + sigma / dm.SCALE / np.sqrt(2) * cn(H0.shape)
    h[:, DC] = 0
    return tx, rx, h


def drifting_sets(B=67):
    """modulation -> (tx, rx, h) of the four sets"""
    return {mod: drifting(mod, B, snr_db=snr) for mod, snr in SETS}


@functools.lru_cache(maxsize=None)
def coded_set(mod=dm.QAM16, rate=0, B=67, snr_db=22.0):
    """the chain test's set: B coded frames of `mod` at code rate `rate` (fec_model's transmitter: random
    information bits, six zero tail bits) through the drifting channel -> dict u, tx, rx, h"""
    import fec_model as fm
    u = fm.random_info(np.random.default_rng(0x7AC0C0DE + 16 * mod + rate), B, mod, rate)
    tx, rx, h = drifting(mod, B, seed=1, snr_db=snr_db, tx=fm.transmit(u, mod, rate)[0])
    return {"u": u, "tx": tx, "rx": rx, "h": h}


def decode_chain(s, mod=dm.QAM16, rate=0, mu=MU, beta=BETA, real=np.float64):
    """coded_set's frames through the model chains in `real` -> (bit errors per frame of the tracked chain: track,
    soft bits weighed by |H_b|^2, Viterbi; of the static chain: demodulate with h, soft bits weighed by |h|^2)"""
    import fec_model as fm
    t = track(s["tx"], s["rx"], s["h"], mod, mu, beta, real=real)
    d = dm.demodulate(s["tx"], s["rx"], s["h"], None, mod, real=real)
    out = []
    for eq, hu in ((t["eq"], t["h_blocks"]), (d["eq"], dm.blend(s["h"], None, real))):
        L = np.asarray(fm.llr(eq, hu, mod, real=real), np.float64).astype(np.float32)
        out.append(np.sum(fm.decode(L, mod, rate) != s["u"], axis=1).astype(np.uint32))
    return out[0], out[1]


# every (mu, beta) the GPU parity test runs, each with the phase flag on and off and a known tx on and off
OPERATING_POINTS = ((0.5, 2), (1.0, 0), (0.25, 4))
COMBOS = [(mu, beta, phase, known) for mu, beta in OPERATING_POINTS for phase in (True, False)
          for known in (False, True)]


@functools.lru_cache(maxsize=None)
def drifting_set(mod):
    return drifting(mod, snr_db=dict(SETS)[mod])


@functools.lru_cache(maxsize=None)
def model(mod, mu, beta, phase=True, known_tx=False, ref_tx=True, real=LD):
    """track() on drifting_set(mod), computed once and shared by the tests (read it, do not write to it)"""
    tx, rx, h = drifting_set(mod)
    return track(tx, rx, h, mod, mu, beta, phase=phase, ref_tx=ref_tx, known_tx=known_tx, real=real)


def symbol_errors(tx, rx, h, mod):
    """-> (static, tracked at MU / BETA, known-tx bound): symbol errors over the set, phase tracking on"""
    static = int(dm.demodulate(tx, rx, h, None, mod, real=np.float64)["nerr"].sum())
    trk = int(track(tx, rx, h, mod, real=np.float64)["nerr"].sum())
    known = int(track(tx, rx, h, mod, known_tx=True, real=np.float64)["nerr"].sum())
    return static, trk, known
