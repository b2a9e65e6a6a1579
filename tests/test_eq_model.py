"""The host model of the equalizer (tests/eq_model.py) against the long double WiFi_Equalization.m
(oracle_py.equalize) on the data sets tests/test_equalize_gpu.py runs on the device -- no GPU here.

Per element, |q - exact| / |exact| by complex modulus, 37 frames x 15 blocks x 52 subcarriers per set:

    f32   the worst element of eq_f32 (ls_store_rv's WCE_OUT_LS_F32 branch, operation for operation, with a
          correctly rounded reciprocal).  The device bound is twice this: v_rcp_f32's one ulp against the exact
          reciprocal adds at most 2^-23 = 1.2e-7 to a figure of 2.3e-7 or more.
    f64   the worst element of eq_f64 (the fp64 formula on the fp64 LS family) divided by the blend's condition
          number kappa_b[k] = (wlt |hlt| + wps |hps|) / |wlt hlt + wps hps|.  The device bound of an element is
          kappa_b[k] x this x 4 (rcp_nr for 1/x, the compiler's contraction order).

Measured (the same on plain, fade and scale: the fades' own elements stay below the worst plain one once divided
by kappa = 2 / delta, and a power of two scales exactly):

    semantics   source      f32        2 x f32     f64 / kappa
    C           ps_linear   2.34e-7    4.68e-7     1.90e-15
    C           ps_cubic    2.77e-7    5.53e-7     5.86e-15
    C           ps_sinc     2.53e-7    5.05e-7     2.58e-15
    MATLAB      ps_linear   2.47e-7    4.95e-7     4.53e-15
    MATLAB      ps_cubic    2.71e-7    5.41e-7     2.26e-14
    MATLAB      ps_sinc     2.62e-7    5.24e-7     2.26e-15

so every fp32 device bound stays under the project's 1e-6 gate.  f64 / kappa is tens of ulps, not one: where the
interpolated estimate itself passes near zero between two pilots its own rounding is large against |hps|, which
kappa does not see; the long double answer for PS_Sinc is formed in double (main.c:124-146, oracle/wce_oracle.c).

The blend formed from fp32-rounded hlt and hps -- the form ls_store_rv's comment rules out -- is measured too: on
the fade set 5.1e-2 (at delta = 1e-6), five orders past the bound; 8.5e-7 on the plain set.
"""
from fractions import Fraction

import numpy as np
import pytest

import eq_model as em
from eq_model import DC, FADES, NBLK, SEMS, SOURCES

KINDS = ("plain", "fade", "scale")


@pytest.fixture(scope="module")
def sets(oracle, golden):
    return em.datasets(oracle, golden)


def test_fma_emulations_are_exact():
    """eq_model.fma / fmaf against rational arithmetic, cancelling sums included"""
    rng = np.random.default_rng(0xF3A)
    a, b, c = rng.standard_normal((3, 600))
    c[:300] = -(a * b)[:300] * (1 + 1e-13 * rng.standard_normal(300))
    want = [float(Fraction(x) * Fraction(y) + Fraction(z)) for x, y, z in zip(a, b, c)]
    assert np.array_equal(em.fma(a, b, c), np.array(want))
    a, b, c = (v.astype(np.float32) for v in (a, b, c))
    c[:300] = -(a * b)[:300]
    # exact: the sum of a 48-bit product and a 24-bit addend whose exponents lie close fits a long double
    wide = a.astype(np.longdouble) * b.astype(np.longdouble) + c.astype(np.longdouble)
    assert np.array_equal(em.fmaf(a, b, c), wide.astype(np.float32))


def test_fades_are_what_they_say(sets):
    """kappa at a faded element is (2 + delta) / delta, and the sources differ from one another on these frames"""
    for sem in SEMS:
        for name in SOURCES:
            k = sets.exact("fade", sem, name)["kappa"]
            for f, sub, b0, delta in FADES:
                assert abs(float(k[f, b0, sub]) * delta / (2 + delta) - 1) < 1e-6, (sem, name, f, sub, b0)
        ps = [sets.exact("plain", sem, n)["ps"] for n in SOURCES]
        off = np.setdiff1d(np.arange(em.N), em.PILOTS)
        for i in range(3):
            d = np.abs(ps[i] - ps[(i + 1) % 3])[:, off] / np.abs(ps[i])[:, off]
            assert float(d.min()) > 1e-9, (sem, SOURCES[i], float(d.min()))   # fp64 would tell them apart anywhere


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("sem", SEMS)
def test_model_figures(sets, sem, kind):
    for name in SOURCES:
        m = sets.measure(kind, sem, name)
        print(f"\n{sem} {kind} {name}: f32 {m['f32']:.3e} (bound {2 * m['f32']:.3e}), f64 / kappa {m['f64']:.3e}")
        # the fp32 branch rounds to 24 bits several times over: at least one ulp, and the bound under the gate
        assert 2.0 ** -24 < m["f32"] and sets.bound_f32(kind, sem, name) < em.GATE_F32, m
        # fp64: some ulps, and nowhere near fp32
        assert 2.0 ** -53 < m["f64"] < 1e-12, m
        ex = sets.exact(kind, sem, name)
        assert np.all(ex["eq"][..., DC] == 0) and np.isfinite(np.asarray(ex["eq"], np.complex128)).all()


def test_fp32_blend_from_fp32_operands_is_out(sets):
    """What the fp64 fma in the fp32 branch is for: hlt and hps rounded to fp32 before the blend miss the bound
    on the fade set by orders of magnitude, and only there."""
    name = "ps_linear"
    for kind, floor in (("plain", 0.0), ("fade", 1e-3)):
        rx, pre = sets.inputs[kind, "C", name]
        ls = em.ls_f64(sets.tx_pre, pre, sets.tx, rx)
        r32 = lambda z: z.astype(np.complex64).astype(np.complex128)
        e = em.relerr(em.eq_f32(rx, r32(ls["lt_ls"]), r32(ls[name])), sets.exact(kind, "C", name)["eq"])
        print(f"\n{kind}: fp32 operands {e.max():.2e}, bound {sets.bound_f32(kind, 'C', name):.2e}")
        assert e.max() > floor
        if kind == "fade":
            f, sub, b0, _ = max(FADES, key=lambda t: -t[3])
            assert e[f, b0, sub] > 1e3 * sets.bound_f32(kind, "C", name)


def test_exponent_clamp():
    """|h| past 2^+-120: the scale stops at 2^-+120 and the quotient keeps fp32 accuracy while |H_UTIL|^2 is an
    fp32 number (2^-130 here: u = 2^-10)."""
    rng = np.random.default_rng(5)
    for ex in (-130, 125):
        h = (rng.standard_normal((2, em.N)) + 1j * rng.standard_normal((2, em.N))) * 2.0 ** ex
        rx = (rng.standard_normal((NBLK, em.N)) + 1j * rng.standard_normal((NBLK, em.N))) * 2.0 ** (ex // 2)
        want = em.eq_f64(rx, h[0], h[1])
        got = em.eq_f32(rx, h[0], h[1])
        k = np.asarray(em.kappa(h[0], h[1]), np.float64)
        ok = k < 4      # away from chance cancellations of the random pair
        ok[:, DC] = False
        assert np.isfinite(got[ok]).all() and em.relerr(got, want)[ok].max() < 1e-6
