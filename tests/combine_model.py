"""Reference models of receive diversity (wce_combine, wce_sync_share), in numpy, the
branch data their tests share, and the tolerances the GPU tests hold the kernel to.
The definitions are those of include/wce.h.  Branch a < A of packet f, V = {0..52}
without 26, v_a = 1 / ow2_a[f] (1 without ow2):

    live(a)    every h_a[k], k in V, finite, and (no ow2, or ow2_a[f] finite and > 0)
    g2[k]      = sum over live a, ascending, of v_a |h_a[k]|^2,   g = sqrt(g2)
    rx_c[b][k] = (sum over live a, ascending, of v_a conj(h_a[k]) rx_a[b][k]) / g[k]
    h_c[k]     = g[k];   entry 26 and every entry with g[k] == 0 are 0
    no live branch: NaN in every entry of the packet's rows, entry 26 included

`real` is np.longdouble (the reference) or np.float64 (the same arithmetic in the
device's precision).

The tolerances are derived, not chosen: TOL_RX and TOL_H are the largest gap between the
fp64 model and the long double model over the parity sets (A = 1, 2, 3, 8, with and
without ow2), times MARGIN.  rx_c is measured against bound = sum_a v_a |h_a| |rx_a| / g,
because the numerator can cancel; h_c against g.  MARGIN = 8: a term of the numerator
carries about 3 roundings (v h, the product, the sum) and g about A + 3, so the fp64
model's error is a random walk of at most 3 A + 6 = 30 steps of u = 2^-53 of the bound,
whose largest excursion over the sets' entries measures 5.7 u (2.5 u for g), while the
worst case is the full 30 u; the device orders the same operations as the model, with
fmas for product-and-sum (fewer roundings, not more) and one more rounding for 1 / g.
8 times the measured gap therefore covers the worst case of either."""
import functools

import numpy as np

import cfo_model as cm
import demod_model as dm
import fec_model as fm
import sync_model as sm
import tx_model as tm

LD = np.longdouble
N, NBLK, DC = dm.N, dm.NBLK, dm.DC
V = np.array([k for k in range(N) if k != DC])
MARGIN = 8
PARITY_A = (1, 2, 3, 8)
PARITY_B = 67


def _finite(z):
    return np.isfinite(z.real) & np.isfinite(z.imag)


# ---------------------------------------------------------------- the two calls
def live_branches(h, ow2=None):
    """h [A][B][53], ow2 [A][B] or None -> bool [A][B]"""
    ok = _finite(np.asarray(h))[:, :, V].all(axis=2)
    if ow2 is not None:
        o = np.asarray(ow2, np.float64)
        with np.errstate(invalid="ignore"):
            ok = ok & np.isfinite(o) & (o > 0)
    return ok


def combine(rx, h, ow2=None, real=LD):
    """rx [A][B][15][53], h [A][B][53], ow2 [A][B] or None -> dict rx [B][15][53], h [B][53] (complex `real`),
    live [A][B], and what the tolerances are relative to: bound [B][15][53] = sum v |h| |rx| / g, g [B][53]"""
    cplx = dm._cplx(real)
    rx, h = np.asarray(rx).astype(cplx), np.asarray(h).astype(cplx)
    A, B = h.shape[:2]
    live = live_branches(h, ow2)
    num = np.zeros((B, NBLK, N), cplx)
    bound = np.zeros((B, NBLK, N), real)
    g2 = np.zeros((B, N), real)
    with np.errstate(all="ignore"):
        for a in range(A):
            m = live[a]
            v = real(1) / np.asarray(ow2, np.float64)[a][m].astype(real)[:, None] if ow2 is not None else real(1)
            ha = h[a][m]
            w = (v * ha.real) - 1j * (v * ha.imag)
            g2[m] = g2[m] + ((v * ha.real) * ha.real + (v * ha.imag) * ha.imag)
            num[m] = num[m] + w[:, None, :] * rx[a][m]
            bound[m] = bound[m] + np.abs(w)[:, None, :] * np.abs(np.where(_finite(rx[a][m]), rx[a][m], 0))
        g = np.sqrt(g2)
        zero = g == 0
        zero[:, DC] = True
        ig = real(1) / np.where(zero, real(1), g)
        out = np.where(zero[:, None, :], 0, num * ig[:, None, :])
        hc = np.where(zero, 0, g).astype(cplx)
        bound = np.where(zero[:, None, :], 0, bound * ig[:, None, :])
    dead = ~live.any(axis=0)
    out[dead] = complex(np.nan, np.nan)
    hc[dead] = complex(np.nan, np.nan)
    return {"rx": out, "h": hc, "live": live, "bound": bound, "g": np.where(zero, 0, g)}


def sync_share(metric, start=None, cfo=None):
    """metric [A][P], start int32 [A][P] or None, cfo [A][P] or None -> (start, cfo) after the call (copies)"""
    metric = np.asarray(metric, np.float64)
    A, P = metric.shape
    live = np.isfinite(metric)
    if start is not None:
        start = np.array(start, np.int32)
        live = live & (start >= 0)
    if cfo is not None:
        cfo = np.array(cfo, np.float64)
    m = np.where(live, metric, -np.inf)
    best = np.argmax(m, axis=0)                 # the first largest: the lowest branch on a tie
    any_live = live.any(axis=0)
    cols = np.arange(P)[any_live]
    if start is not None:
        start[:, cols] = start[best[cols], cols][None, :]
    if cfo is not None:
        cfo[:, cols] = cfo[best[cols], cols][None, :]
    return start, cfo


# ---------------------------------------------------------------- branch data
def branches(A, mod=dm.QAM16, B=PARITY_B, seed=0, snr_db=22.0, loss_db=None, rho=0.995, L=6, tx=None):
    """B packets of `mod` seen by A antennas: per branch its own L taps of an exponential power-delay profile,
    each a Gauss-Markov process with per-block correlation rho, and its own noise at snr_db - loss_db[a]; one
    residual phase drift shared by the branches (one oscillator).  h_a is the branch's channel before block 0
    plus the noise of a long-training estimate; ow2_a the branch's noise variance per complex sample, known to
    the 10% an estimate from one preamble gives.
    -> (tx [B][15][53], rx [A][B][15][53], h [A][B][53], ow2 [A][B]), complex128 / float64"""
    rng = np.random.default_rng(0xC0B1 + 64 * A + 16 * mod + seed)
    drawn = dm.constellation(rng, mod, (B, NBLK, N)) * dm.SCALE
    tx = drawn if tx is None else np.array(tx, np.complex128)
    tx[:, :, list(dm.PILOTS)] = dm.SCALE * dm.PILOT_SIGN[None, None, :] * dm.POLARITY[None, :, None]
    tx[:, :, DC] = 0
    loss = np.zeros(A) if loss_db is None else np.asarray(loss_db, float)
    pdp = np.exp(-0.5 * np.arange(L))
    pdp /= np.sqrt(np.sum(pdp ** 2))
    cn = lambda s: (rng.standard_normal(s) + 1j * rng.standard_normal(s)) / np.sqrt(2)
    F = np.exp(-2j * np.pi * np.outer(np.arange(L), np.arange(N) - DC) / 64)
    phi = rng.uniform(-.5, .5, (B, 1)) + rng.uniform(-.03, .03, (B, 1)) * np.arange(NBLK)
    rx = np.empty((A, B, NBLK, N), np.complex128)
    h = np.empty((A, B, N), np.complex128)
    ow2 = np.empty((A, B))
    for a in range(A):
        t = cn((B, L)) * pdp
        H0 = t @ F
        Hb = np.empty((B, NBLK, N), np.complex128)
        for b in range(NBLK):
            t = rho * t + np.sqrt(1 - rho ** 2) * cn((B, L)) * pdp
            Hb[:, b] = t @ F
        sigma = dm.SCALE * 10 ** (-(snr_db - loss[a]) / 20)
        rx[a] = Hb * tx * np.exp(1j * phi)[:, :, None] + sigma * cn(tx.shape)
        h[a] = H0 + sigma / dm.SCALE / np.sqrt(2) * cn(H0.shape)
        h[a][:, DC] = 0
        ow2[a] = sigma ** 2 * (1 + 0.1 * rng.standard_normal(B))
    return tx, rx, h, ow2


@functools.lru_cache(maxsize=None)
def parity_set(A):
    """the GPU parity test's branches: each next branch 3 dB noisier (read it, do not write to it)"""
    return branches(A, loss_db=3.0 * np.arange(A))


@functools.lru_cache(maxsize=None)
def parity_model(A, weighted, real=LD):
    tx, rx, h, ow2 = parity_set(A)
    return combine(rx, h, ow2 if weighted else None, real)


def gaps(got, ref):
    """(largest |got rx - ref rx| / bound, largest |got h - ref h| / g) over the entries with a bound, in long
    double; ref is a long double combine() result, got any dict with rx and h"""
    ok = ref["bound"] > 0
    e_rx = np.abs(np.asarray(got["rx"], np.clongdouble) - ref["rx"])[ok] / ref["bound"][ok]
    okh = ref["g"] > 0
    e_h = np.abs(np.asarray(got["h"], np.clongdouble) - ref["h"])[okh] / ref["g"][okh]
    return float(np.max(e_rx)), float(np.max(e_h))


@functools.lru_cache(maxsize=None)
def measured_gaps():
    """fp64 model against long double over the parity sets -> (rx, h)"""
    worst = np.zeros(2)
    for A in PARITY_A:
        for weighted in (False, True):
            worst = np.maximum(worst, gaps(parity_model(A, weighted, np.float64), parity_model(A, weighted)))
    return float(worst[0]), float(worst[1])


def tolerances():
    """-> (TOL_RX of bound, TOL_H of g): MARGIN times the measured gaps"""
    g_rx, g_h = measured_gaps()
    return MARGIN * g_rx, MARGIN * g_h


def sync_share_set(A, P=PARITY_B, seed=0):
    """metric, start, cfo [A][P] with every kind of packet: one live branch, several, ties between live branches,
    ties with a dead one, no live branch (start -1 everywhere; NaN metrics), a NaN metric beside a live branch"""
    rng = np.random.default_rng(0x5A4E + 16 * A + seed)
    metric = rng.uniform(0.05, 1.0, (A, P))
    start = rng.integers(0, 200, (A, P)).astype(np.int32)
    start[rng.uniform(size=(A, P)) < 0.3] = -1
    cfo = rng.uniform(-0.002, 0.002, (A, P))
    metric[rng.uniform(size=(A, P)) < 0.05] = np.inf
    metric[:, 3] = 0.75                             # a tie of every branch
    start[:, 3] = np.arange(A) + 10
    if A > 1:
        start[:, 5], start[:, 9] = -1, -1
        metric[0, 5], metric[1, 5] = 0.5, 0.5       # the best is tied with a dead branch below it
        start[1, 5] = 77
        metric[0, 9], start[0, 9] = np.nan, 11      # a NaN metric is not live whatever its start
        metric[1, 9], start[1, 9] = 0.3, 12
    start[:, 7] = -1                                # none live
    metric[:, 11] = np.nan
    start[:, 11] = np.abs(start[:, 11])
    return metric, start, cfo


# ---------------------------------------------------------------- the link experiment
LINK_B, LINK_MOD, LINK_RATE, LINK_SNR = 67, dm.QAM16, fm.RATE_1_2, 10.0
LINK_LEN, LINK_THRESHOLD, LINK_STEP_DB = 1488, tm.CHAIN_THRESHOLD, 6.0
# chosen on the CPU (tests/test_combine_abi.py::test_link_model_seed): with it the model leaves out no frame of any
# of the four cases, on the model transmitter's captures
LINK_SEED = 0x4007


@functools.lru_cache(maxsize=None)
def link_set(A, unequal, seed=LINK_SEED):
    """what Context.link_mrc_host is given, and the bits it draws itself from the seed -> dict: taps [A][B][6]
    (static, independent per branch), cfo and delay [B] (shared by the branches), loss [A] (dB), bits"""
    rng = np.random.default_rng(seed + 16 * A + int(unequal))
    taps = np.stack([tm.random_taps(rng, LINK_B, 6) for _ in range(A)])
    cfo = rng.uniform(-0.002, 0.002, LINK_B)
    delay = rng.integers(0, 100, LINK_B).astype(np.int32)
    T = fm.info_bits(LINK_MOD, LINK_RATE)
    bits = np.random.default_rng(seed).integers(0, 2, (LINK_B, T), dtype=np.uint8)      # link_mrc_host's draw
    bits[:, T - 6:] = 0
    loss = LINK_STEP_DB * np.arange(A) if unequal else np.zeros(A)
    return {"taps": taps, "cfo": cfo, "delay": delay, "bits": bits, "loss": loss, "seed": seed,
            "ow2": float(tm.nominal_ow2(LINK_SNR)) * 10.0 ** (loss / 10.0)}


def link_capture(A, unequal, seed=LINK_SEED, real=np.float64):
    """the captures of link_set through the model transmitter, branch a at first_frame = a B -> [A][B][L]"""
    c = link_set(A, unequal, seed)
    tx = fm.transmit(c["bits"], LINK_MOD, LINK_RATE)[0]
    pre = tm.chain_pre()
    return np.stack([np.asarray(tm.transmit(tx, LINK_LEN, pre, real, taps=c["taps"][a], cfo=c["cfo"],
                                            ow2=np.full(LINK_B, c["ow2"][a]), delay=c["delay"], seed=seed,
                                            first_frame=a * LINK_B), np.complex128) for a in range(A)])


def decode_with_gap(llr_blocks, mod, rate):
    """fec_model.decode (terminated, float metrics) that also reports how close the decoded path came to losing:
    -> (bits [B][T], gap [B]: the smallest |c1 - c0| of the add-compare-selects on the surviving path,
    mass [B]: sum |L| of the frame's soft bits)"""
    L = np.asarray(llr_blocks)
    L = fm.depuncture(L.reshape(L.shape[0], -1), rate).astype(np.float32)
    L = np.where(np.isfinite(L), L, np.float32(0))
    B, T = L.shape[0], L.shape[1] // 2
    pred, cA, cB = fm.trellis()
    sA, sB = (2 * cA - 1).astype(np.float32), (2 * cB - 1).astype(np.float32)
    pm = np.full((B, 64), -np.inf, np.float32)
    pm[:, 0] = 0
    dec = np.zeros((T, B, 64), bool)
    dif = np.zeros((T, B, 64), np.float32)
    with np.errstate(invalid="ignore"):
        for t in range(T):
            la, lb = L[:, 2 * t, None], L[:, 2 * t + 1, None]
            c0 = pm[:, pred[0]] + (sA[0] * la + sB[0] * lb)
            c1 = pm[:, pred[1]] + (sA[1] * la + sB[1] * lb)
            dec[t] = c1 > c0
            dif[t] = np.abs(c1 - c0)
            pm = np.where(dec[t], c1, c0)
    s = np.zeros(B, np.int64)
    bits = np.zeros((B, T), np.uint8)
    gap = np.full(B, np.inf)
    rows = np.arange(B)
    for t in range(T - 1, -1, -1):
        bits[:, t] = s >> 5
        d = dif[t, rows, s].astype(np.float64)
        gap = np.where(np.isnan(d), gap, np.minimum(gap, d))     # -inf against -inf: no contest
        s = 2 * (s & 31) + dec[t, rows, s]
    return bits, gap, np.sum(np.abs(L.astype(np.float64)), axis=1)


# A device soft bit is the model's up to fp64 rounding (1e-13 of its value), which can carry it across a float
# rounding boundary: it then differs by one float ulp.  The decoder's metrics are float sums, so from that step on
# every path metric may round the other way, by one ulp of the metric: at most 2^-24 |pm| <= 2^-24 sum |L|, since a
# path metric is a signed sum of the frame's soft bits.  The two candidates of an add-compare-select can each be
# off by that, so their difference moves by at most 2^-23 sum |L|.  A frame whose surviving path won some comparison
# by less is marginal: its decoded bits may legitimately differ between two fp64 implementations.  The static chain
# feeds no sliced symbol back, so no slicer margin enters its bits.
GAP_TOL = 2.0 ** -23


def _chain_counts(tx, rx, h, bits, real):
    d = dm.demodulate(tx, rx, h, None, LINK_MOD, tm.SCALE, True, True, real)
    L = np.asarray(fm.llr(d["eq"], dm.blend(h, None, real), LINK_MOD, tm.SCALE, real), np.float64).astype(np.float32)
    dec, gap, mass = decode_with_gap(L, LINK_MOD, LINK_RATE)
    return np.sum(dec != bits, axis=1).astype(np.uint32), gap < GAP_TOL * mass


def link_front(cap, share=True, real=np.float64):
    """everything in front of the combiner, from the captures cap [A][B][L] -> dict start, metric, cfo, ow2 [A][B]
    (after sharing), rx [A][B][15][53], h [A][B][53] (LT_LS)"""
    cap = np.asarray(cap, np.complex128)
    A, B, Lc = cap.shape
    share = share and A > 1
    pre = tm.chain_pre()
    flat = cap.reshape(A * B, Lc)
    ltf = np.asarray(tm.idft64(pre, LD), np.complex128)
    start, M, _ = sm.sync(flat, ltf, LINK_THRESHOLD, 0, real)
    start, M = start.reshape(A, B), M.reshape(A, B)
    if share:
        start, _ = sync_share(M, start, None)
    if np.any(start < 0) or np.any(start + 128 + 1200 > Lc):
        raise ValueError("the link model expects every packet detected and inside its window")
    s = start.reshape(-1)
    field = np.stack([flat[f, s[f]:s[f] + 128] for f in range(A * B)])
    pk = np.stack([flat[f, s[f] + 128:s[f] + 128 + 1200] for f in range(A * B)])
    eps = np.asarray(cm.estimate(field, real), np.float64)
    if share:
        eps = sync_share(M, None, eps.reshape(A, B))[1].reshape(-1)
    rx_pre, ow2 = cm.preamble(field, eps, real)
    rx = cm.blocks(pk, eps, 0, NBLK, real)
    with np.errstate(invalid="ignore", divide="ignore"):      # DC: 0 / 0, then set to 0
        h = dm.lt_ls(np.broadcast_to(pre, (A * B, N)), rx_pre, real)
    return {"start": start, "metric": M, "cfo": eps.reshape(A, B), "rx": np.asarray(rx).reshape(A, B, NBLK, N),
            "h": np.asarray(h).reshape(A, B, N), "ow2": np.asarray(ow2, np.float64).reshape(A, B)}


def link_model(cap, bits, weighted, share=True, front=None, real=np.float64):
    """Context.link_mrc_host's receiver with LT_LS as the estimate, from the captures cap [A][B][L]:
    sync_model.sync over the A B windows, sync_share, cfo_model (the two-copy estimate, shared, the derotated
    fields with their ow2, the blocks), LT_LS, then per branch and for combine() (weighted by the fields' ow2 or
    not) demod_model (tracked, no blend), fec_model's soft bits and the decoder.  front: link_front's dict of the
    same captures, so that calls that differ in `weighted` alone share everything in front of the combiner.
    -> dict combined [B], branch [A][B] (bit errors), marginal [B], branch_marginal [A][B] (bool), start [A][B]"""
    f = front if front is not None else link_front(cap, share, real)
    A, B = f["start"].shape
    tx = fm.transmit(bits, LINK_MOD, LINK_RATE)[0]
    c = combine(f["rx"], f["h"], f["ow2"] if weighted else None, real)
    comb, cm_ = _chain_counts(tx, c["rx"], c["h"], bits, real)
    br, bm = _chain_counts(np.tile(tx, (A, 1, 1)), f["rx"].reshape(A * B, NBLK, N), f["h"].reshape(A * B, N),
                           np.tile(bits, (A, 1)), real)
    return {"combined": comb, "branch": br.reshape(A, B), "marginal": cm_, "branch_marginal": bm.reshape(A, B),
            "start": f["start"]}
