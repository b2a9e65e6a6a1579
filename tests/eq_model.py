"""Host model of the equalization epilogue ls_store_rv (csrc/wce_kernels.hip) -- TEST INFRASTRUCTURE ONLY.

    eq_f32(rx, hlt, hps)   the WCE_OUT_LS_F32 branch, operation for operation: frexp of the largest of the four
                           parts and the +-120 clamp, sc = 2^-e and sf = (float)sc, the fp64 fma blend
                           hlt sc + ((hps - hlt) sc) (b+1)/15 rounded to fp32, (float)rx * sf, the fmaf forms of
                           the denominator and the two numerators, a correctly rounded reciprocal where the kernel
                           has v_rcp_f32 (1 ulp), DC = 0.
    ls_f64(...)            the LS family in fp64 in the kernels' order (lt_ls_lane, ps_lane; cdiv and clerp with their
                           fmas, an IEEE 1/x where the kernel has rcp_nr)
    eq_f64(rx, hlt, hps)   rx / (wlt hlt + wps hps) in plain fp64, the fp64 branch's formula
    kappa(hlt, hps)        the blend's condition number (wlt |hlt| + wps |hps|) / |wlt hlt + wps hps|  [15][53]

and the data sets that tests/test_eq_model.py measures these on against the long double WiFi_Equalization.m
(oracle_py.equalize), and that tests/test_equalize_gpu.py runs on the device (datasets(), measure()).

Errors are per element and by complex modulus: |q - exact| / |exact|, never per component.
"""
import functools

import numpy as np

N, NBLK, DC = 53, 15, 26
PILOTS = (5, 19, 33, 47)
AMP = 8.8753
B0 = 37                      # frames per set
TX_BLOCK = 2                 # the block C semantics estimates from in these sets (MATLAB: blocks 0..3)
SOURCES = ("ps_linear", "ps_cubic", "ps_sinc")
SEMS = ("C", "MATLAB")
F32, F64 = np.float32, np.float64
GATE_F32 = 1e-6              # the project's fp32 gate (BASELINE G4)

# fade set: (frame, k, b0, delta) -- hlt[k] = -hps[k] (wps / wlt) (1 + delta) at block b0, so that block's blend
# is -delta wps hps[k].  One k of each linear segment (k < 19, < 33, >= 33) and k = 52 at every delta; frames 0
# and 4 (inside the B = 1 and B = 5 runs), 16 and 17 (a workgroup border of ls_kernel), 35 and 36 (its last,
# partial group).
FADES = (
    (0, 11, 0, 1e-2), (0, 25, 7, 1e-4), (0, 40, 13, 1e-6), (0, 52, 3, 1e-2),
    (1, 3, 13, 1e-6), (4, 30, 0, 1e-2), (4, 52, 7, 1e-4),
    (9, 16, 3, 1e-4), (16, 45, 7, 1e-2), (17, 21, 13, 1e-6), (17, 52, 0, 1e-6),
    (31, 36, 3, 1e-4), (35, 8, 7, 1e-2), (36, 27, 0, 1e-6), (36, 50, 13, 1e-4),
)


# ------------------------------------------------------------------ exact fp32 / fp64 fused multiply-add in numpy
def _two_sum(a, b):
    s = a + b
    bb = s - a
    return s, (a - (s - bb)) + (b - bb)


def _round_odd_sum(a, b):
    """a + b in fp64 rounded to odd: an inexact sum takes the neighbour with an odd last bit, so that a later
    rounding to fewer bits is the rounding of the exact sum (Boldo and Melquiond, 2008)."""
    s, e = _two_sum(a, b)
    bits = s.view(np.int64).copy()
    fix = (e != 0) & ((bits & 1) == 0) & np.isfinite(s)
    step = np.where((e > 0) == (s > 0), 1, -1)
    bits[fix] += step[fix]
    return bits.view(F64)


def fmaf(a, b, c):
    """fmaf on fp32 arrays: the product is exact in fp64, the sum is rounded to odd there, then once to fp32"""
    a, b, c = (np.asarray(x, F32).astype(F64) for x in np.broadcast_arrays(a, b, c))
    with np.errstate(invalid="ignore", over="ignore"):
        return _round_odd_sum(a * b, c).astype(F32)


def _split(a):
    t = a * 134217729.0   # 2^27 + 1 (Veltkamp)
    hi = t - (t - a)
    return hi, a - hi


def fma(a, b, c):
    """fma on fp64 arrays (exact product by Dekker, TwoSum with c, the low parts rounded to odd, one final
    rounding; Boldo and Melquiond, 2008).  For operands whose product stays clear of fp64's range ends."""
    a, b, c = (np.array(x, F64) for x in np.broadcast_arrays(a, b, c))
    with np.errstate(invalid="ignore", over="ignore"):
        uh = a * b
        ah, al = _split(a)
        bh, bl = _split(b)
        ul = ((ah * bh - uh) + ah * bl + al * bh) + al * bl
        th, tl = _two_sum(c, uh)
        out = th + _round_odd_sum(tl, ul)
    bad = ~np.isfinite(out)
    out[bad] = (a * b + c)[bad]   # non-finite operands: whatever IEEE gives
    return out


def rcp_f32(d):
    """the correctly rounded fp32 reciprocal (1/d in fp64 rounds innocuously twice: 53 >= 2 * 24 + 2)"""
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        return (1.0 / np.asarray(d, F32).astype(F64)).astype(F32)


# ------------------------------------------------------------------ the fp32 branch of ls_store_rv
def eq_f32(rx, hlt, hps):
    """rx [..., 15, 53], hlt and hps [..., 53], complex128 -> complex64 [..., 15, 53]"""
    rx, hlt, hps = np.asarray(rx, np.complex128), np.asarray(hlt, np.complex128), np.asarray(hps, np.complex128)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore", under="ignore"):
        dps = hps - hlt
        big = np.fmax(np.fmax(np.abs(hlt.real), np.abs(hlt.imag)), np.fmax(np.abs(hps.real), np.abs(hps.imag)))
        e = np.where(np.isfinite(big), np.frexp(np.where(np.isfinite(big), big, 0.0))[1], 0)
        e = np.clip(e, -120, 120)
        sc = np.ldexp(1.0, -e)
        sf = sc.astype(F32)
        h0r, h0i, d0r, d0i = hlt.real * sc, hlt.imag * sc, dps.real * sc, dps.imag * sc
        out = np.zeros(rx.shape, np.complex64)
        for b in range(NBLK):
            t = F64(b + 1) / NBLK
            ur, ui = fma(d0r, t, h0r).astype(F32), fma(d0i, t, h0i).astype(F32)
            xr, xi = rx[..., b, :].real.astype(F32) * sf, rx[..., b, :].imag.astype(F32) * sf
            inv = rcp_f32(fmaf(ur, ur, ui * ui))
            out[..., b, :] = fmaf(xr, ur, xi * ui) * inv + 1j * (fmaf(xi, ur, -(xr * ui)) * inv)
        out[..., DC] = 0
    return out


# ------------------------------------------------------------------ plain fp64
def _cdiv(a, b):
    """cdiv of csrc/wce_device.h, its fmas included; an IEEE 1/x where it has rcp_nr"""
    a, b = np.broadcast_arrays(np.asarray(a, np.complex128), np.asarray(b, np.complex128))
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        inv = 1.0 / fma(b.real, b.real, b.imag * b.imag)
        return fma(a.real, b.real, a.imag * b.imag) * inv + 1j * (fma(a.imag, b.real, -(a.real * b.imag)) * inv)


def sinc_table():
    a = (np.arange(N)[None, :] - np.array(PILOTS)[:, None]) / 14.0
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(a != 0, np.sin(np.pi * a) / (np.pi * a), 1.0)


def ls_f64(tx_pre, rx_pre, tx, rx, matlab=False, block=TX_BLOCK):
    """tx_pre [53], rx_pre [B][53], tx and rx [B][15][53] -> dict of lt_ls, ps_linear, ps_cubic, ps_sinc [B][53]"""
    tp = np.asarray(tx_pre, np.complex128)
    rp, tx, rx = (np.asarray(a, np.complex128) for a in (rx_pre, tx, rx))
    if matlab:
        hlt = (tp.conj() * rp) * (1.0 / (tp.real * tp.real + tp.imag * tp.imag))
    else:
        cq = tp.real - tp.imag
        hlt = _cdiv(cq * rp, cq * tp)
    hlt[..., DC] = 0
    P = list(PILOTS)
    if matlab:   # the wave's butterfly: ((b0 + b1) + (b2 + b3)) / 4
        hb = _cdiv(rx[:, :4, P], tx[:, :4, P])
        hp = ((hb[:, 0] + hb[:, 1]) + (hb[:, 2] + hb[:, 3])) * 0.25
    else:
        hp = _cdiv(rx[:, block, P], tx[:, block, P])
    h0, h1, h2, h3 = (hp[:, i:i + 1] for i in range(4))
    k = np.arange(N)
    seg = np.where(k < PILOTS[1], 0, np.where(k < PILOTS[2], 1, 2))
    alpha = (k - np.array(PILOTS)[seg]) * (1.0 / 14.0)
    lo, hi = hp[:, seg], hp[:, seg + 1]
    d = hi - lo   # clerp: one fma per component
    lin = fma(d.real, alpha, lo.real) + 1j * fma(d.imag, alpha, lo.imag)
    r = 1.0 / 14.0
    r2, r3 = (1.0 / 28.0, 1.0 / 42.0) if matlab else (r, r)
    dk0, dk1, dk2 = (k - PILOTS[0]).astype(F64), (k - PILOTS[1]).astype(F64), (k - PILOTS[2]).astype(F64)
    f01, f12, f23 = (h1 - h0) * r, (h2 - h1) * r, (h3 - h2) * r
    f012, f123 = (f12 - f01) * r2, (f23 - f12) * r2
    f0123 = (f123 - f012) * r3
    cub = ((h0 + f01 * dk0) + (f012 * dk0) * dk1) + ((f0123 * dk0) * dk1) * dk2
    s = sinc_table()
    snc = ((h0 * s[0] + h1 * s[1]) + h2 * s[2]) + h3 * s[3]
    return dict(lt_ls=hlt, ps_linear=lin, ps_cubic=cub, ps_sinc=snc)


def eq_f64(rx, hlt, hps):
    rx, hlt, hps = np.asarray(rx, np.complex128), np.asarray(hlt, np.complex128), np.asarray(hps, np.complex128)
    out = np.zeros(rx.shape, np.complex128)
    for b in range(NBLK):
        wlt, wps = F64(NBLK - (b + 1)) / NBLK, F64(b + 1) / NBLK
        out[..., b, :] = _cdiv(rx[..., b, :], hlt * wlt + hps * wps)
    out[..., DC] = 0
    return out


def kappa(hlt, hps):
    """[..., 15, 53] in long double; 1 where the blend is a single term (block 14; DC, where hlt = 0)"""
    hlt, hps = np.asarray(hlt, np.clongdouble), np.asarray(hps, np.clongdouble)
    w = (np.arange(1, NBLK + 1, dtype=np.longdouble) / NBLK)[:, None]
    hl, hp = hlt[..., None, :], hps[..., None, :]
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.asarray(((1 - w) * np.abs(hl) + w * np.abs(hp)) / np.abs((1 - w) * hl + w * hp), np.longdouble)


def relerr(q, exact):
    """|q - exact| / |exact| per element by complex modulus, [..., 15, 53] float64; 0 where both are 0 (DC)"""
    q, exact = np.asarray(q, np.clongdouble), np.asarray(exact, np.clongdouble)
    num, den = np.abs(q - exact), np.abs(exact)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.asarray(np.where((num == 0) & (den == 0), 0, num / den), F64)


# ------------------------------------------------------------------ data sets
def _symbols(rng, kind, shape):
    if kind == 0:
        x = (2.0 * rng.integers(0, 2, shape) - 1.0).astype(np.complex128)
    elif kind == 1:
        x = ((2.0 * rng.integers(0, 2, shape) - 1) + 1j * (2.0 * rng.integers(0, 2, shape) - 1)) / np.sqrt(2.0)
    else:
        lv = np.array([-3.0, -1.0, 1.0, 3.0]) / np.sqrt(10.0)
        x = lv[rng.integers(0, 4, shape)] + 1j * lv[rng.integers(0, 4, shape)]
    return AMP * x


class Sets:
    """The inputs of every set, the long double answers, and the model's figures on them; nothing is written
    after construction.  One tx for all sets; a set is (rx, rx_pre), the fade sets one rx_pre per (semantics,
    source)."""

    def __init__(self, oracle, tx_pre, ow2):
        self.oracle = oracle
        rng = np.random.default_rng(0xE9A11)
        # the callers' preamble: the context's with every third entry negated (LsArgs::tx_pre)
        self.tx_pre = np.array(tx_pre, np.complex128)
        self.tx_pre[::3] *= -1.0
        # plain: frame f is BPSK / QPSK / 16-QAM by f % 3, every block its own symbols, its own 3-tap channel
        tx = np.stack([_symbols(rng, f % 3, (NBLK, N)) for f in range(B0)])
        tx[..., DC] = 0.0
        taps = (rng.standard_normal((B0, 3)) + 1j * rng.standard_normal((B0, 3))) * np.sqrt([0.6, 0.3, 0.1])
        h = 0.0122 / np.sqrt(2.0) * (taps @ np.exp(-2j * np.pi * np.outer(np.arange(3), np.arange(N) - DC) / 64.0))
        sd = np.sqrt(ow2 / 2.0)
        rx = h[:, None, :] * tx + sd * (rng.standard_normal(tx.shape) + 1j * rng.standard_normal(tx.shape))
        pre = h * self.tx_pre + sd * (rng.standard_normal(h.shape) + 1j * rng.standard_normal(h.shape))
        self.tx = tx
        self.inputs = {("plain", s, n): (rx, pre) for s in SEMS for n in SOURCES}
        # scale: the channel times 2^100 (frames 0..18) and 2^-100 (19..36); rx stays a normal fp32 number
        sc = np.ldexp(1.0, np.where(np.arange(B0) < 19, 100, -100))
        rxs, pres = rx * sc[:, None, None], pre * sc[:, None]
        parts = np.abs(np.stack([rxs.real, rxs.imag]))
        assert parts.min() >= np.ldexp(1.0, -126) and parts.max() <= np.finfo(F32).max, "rx outside fp32's normal range"
        for s in SEMS:
            for n in SOURCES:
                self.inputs["scale", s, n] = (rxs, pres)
        # fade: rx_pre chosen against the long double hps of each (semantics, source)
        for s in SEMS:
            for n in SOURCES:
                p = np.array(pre)
                for f, k, b0, delta in FADES:
                    hps = self._ps(s, n, tx[f], rx[f])[k]
                    wps, wlt = np.longdouble(b0 + 1) / NBLK, np.longdouble(NBLK - b0 - 1) / NBLK
                    p[f, k] = np.complex128(-hps * (wps / wlt) * (1 + np.longdouble(delta)) * self.tx_pre[k])
                self.inputs["fade", s, n] = (rx, p)
        for a in (self.tx, self.tx_pre, rx, pre, rxs, pres, *(v[1] for v in self.inputs.values())):
            a.setflags(write=False)

    def _ps(self, sem, name, tx, rx):
        o = self.oracle
        return o.matlab(name, tx, rx) if sem == "MATLAB" else getattr(o, name)(tx[TX_BLOCK], rx[TX_BLOCK])

    @functools.lru_cache(maxsize=None)
    def exact(self, kind, sem, name):
        """long double lt_ls [37][53], the source's estimate [37][53], eq [37][15][53] and kappa [37][15][53]"""
        o = self.oracle
        rx, pre = self.inputs[kind, sem, name]
        lt = np.stack([(o.matlab_lt_ls if sem == "MATLAB" else o.lt_ls)(self.tx_pre, pre[f]) for f in range(B0)])
        ps = np.stack([self._ps(sem, name, self.tx[f], rx[f]) for f in range(B0)])
        eq = np.stack([o.equalize(rx[f], lt[f], ps[f]) for f in range(B0)])
        return dict(lt_ls=lt, ps=ps, eq=eq, kappa=kappa(lt, ps))

    @functools.lru_cache(maxsize=None)
    def measure(self, kind, sem, name):
        """The host figures of one set: f32 = the fp32 model's worst element; f64 = the fp64 formula's worst
        element over kappa.  The device bounds follow from these alone."""
        rx, pre = self.inputs[kind, sem, name]
        ex = self.exact(kind, sem, name)
        ls = ls_f64(self.tx_pre, pre, self.tx, rx, matlab=sem == "MATLAB")
        e32 = relerr(eq_f32(rx, ls["lt_ls"], ls[name]), ex["eq"])
        e64 = relerr(eq_f64(rx, ls["lt_ls"], ls[name]), ex["eq"]) / np.asarray(ex["kappa"], F64)
        e64[..., DC] = 0.0
        return dict(f32=float(e32.max()), f64=float(e64.max()))

    def bound_f32(self, kind, sem, name):
        """per element: twice the model's worst (v_rcp_f32's ulp against the exact reciprocal adds <= 2^-23)"""
        return 2.0 * self.measure(kind, sem, name)["f32"]

    def bound_f64(self, kind, sem, name):
        """[37][15][53]: kappa x (the fp64 formula's worst over kappa) x 4 (rcp_nr, contraction order)"""
        return np.asarray(self.exact(kind, sem, name)["kappa"], F64) * (4.0 * self.measure(kind, sem, name)["f64"])


_sets = {}


def datasets(oracle, golden):
    """the one Sets of a session (golden: conftest's fixture)"""
    if "s" not in _sets:
        inp = golden["inputs"]
        _sets["s"] = Sets(oracle, inp["tx_pre"], float(inp["ow2"]))
    return _sets["s"]
