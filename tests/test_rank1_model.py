"""The closed-form rank-1 PS_MMSE (csrc/wce_rank1.hip) as an fp64 model on the CPU.

`model_h` transcribes `rank1_s` / `mmse_rank1_kernel` operation by operation:
the same lane layout (lane i of 16 owns subcarriers i + 16 m), the same
per-lane partial sums in the order m = 0..3, the same 16-lane butterfly
(xor 1, xor 2, half mirror, mirror) and only plain IEEE products, sums and
quotients on separate real and imaginary parts -- the device function is
compiled with contraction off, so no FMA rounds differently there.  The
model is checked against the long double closed form
(`oracle_py.mmse_textbook_closed`) at the project's 1e-10 norm-relative.

Measured maxima (500 frames per class, seed 0x51, cond(Ryy) = 4.3e6 on the
inputs.h preamble with its symbol amplitude, a DC null in every frame):

    BPSK   matched 4.2e-13   unrelated 4.4e-13
    QPSK   matched 6.0e-12   unrelated 1.2e-14
    16-QAM matched 8.2e-12   unrelated 1.2e-14
    nulls / |x_k| down to 1e-150 (QPSK, matched): 5.5e-11; all-zero frame: H = 0 exactly
    the naive (rho^T rx - (rho^T al) t) / b on BPSK matched: 8.0e-10 (why it is not used)

The BPSK figures are the oracle's own error, not the model's: the oracle
evaluates the one-line closed form, which cancels ~cond digits even in long
double (4e6 x 5e-20).  Against the split form evaluated in long double the
model is at 3.6e-16 / 2.3e-15 on BPSK and unchanged elsewhere.  The complex
matched cases are the form's own: rx_k - al_k t is a difference of nearly
equal fp64 numbers there, ~eps cond / sqrt(live subcarriers).

The branch for a given w (`cwg`: complex g, complex division) has no caller
with g != 0, so `model_s(..., cwg=True)` is pinned against mpmath instead
(tests/golden/make_rank1_cw_mp.py: the 53 x 53 matrix inverted by LU at 50
digits, w = conj(u) with phases turned by up to 0.3 rad and amplitudes scaled
by up to 20%, x zeroed off the mask as `masked` does).  Maxima, relative in
s, 4 frames per class at the same operating point:

    BPSK   matched 1.0e-16   unrelated 2.7e-16
    QPSK   matched 5.6e-13   unrelated 2.6e-15
    16-QAM matched 4.9e-13   unrelated 1.4e-15
    a = 0, the four pilots in the mask (REF's shape): 5.1e-16
"""
import os

import numpy as np
import pytest

from oracle_py import N, normrel

TOL = 1e-10
B = 500
DC = 26
AMP = 8.8753   # the symbol amplitude of inputs.h (and of the synthetic frames): cond(Ryy) ~ 4e6


# ---- the device arithmetic on (re, im) pairs of float64 arrays
def _mul(a, b):
    return a[0] * b[0] - a[1] * b[1], a[0] * b[1] + a[1] * b[0]


def _add(a, b):
    return a[0] + b[0], a[1] + b[1]


def _row16_sum(v):
    i = np.arange(16)
    for x in (1, 2, 7, 15):   # quad_perm [1,0,3,2], [2,3,0,1], row_half_mirror, row_mirror
        v = v + v[..., i ^ x]
    return v


def _lanes(z):
    """[..., 53] complex -> (re, im) arrays [..., 4, 16] (m, lane i): subcarrier i + 16 m, zero past 52."""
    p = np.zeros(z.shape[:-1] + (64,), np.complex128)
    p[..., :N] = z
    p = p.reshape(z.shape[:-1] + (4, 16))
    return np.ascontiguousarray(p.real), np.ascontiguousarray(p.imag)


def model_s(x, r, u, w, ac, bc, cwg=False):
    """rank1_s: x, r, u, w as _lanes() pairs; returns s (re, im) per unit, lane 0's copy."""
    g = q = None
    for m in range(4):
        xm, rm, um, wm = [(v[0][..., m, :], v[1][..., m, :]) for v in (x, r, u, w)]
        p = _mul(wm, um) if cwg else (um[0] * um[0] + um[1] * um[1], np.zeros_like(um[0]))
        ax2 = ac * (xm[0] * xm[0] + xm[1] * xm[1])
        gk = (ax2 * p[0], ax2 * p[1])
        qk = _mul(_mul(wm, (xm[0], -xm[1])), rm)
        g = gk if m == 0 else _add(g, gk)
        q = qk if m == 0 else _add(q, qk)
    g = (_row16_sum(g[0]), _row16_sum(g[1]))
    q = (_row16_sum(q[0]), _row16_sum(q[1]))
    d = (bc + g[0], g[1])
    if cwg:
        den = d[0] * d[0] + d[1] * d[1]
        t = ((q[0] * d[0] + q[1] * d[1]) / den, (q[1] * d[0] - q[0] * d[1]) / den)
    else:
        t = (q[0] / d[0], q[1] / d[0])
    c = None
    for m in range(4):
        xm, rm, um, wm = [(v[0][..., m, :], v[1][..., m, :]) for v in (x, r, u, w)]
        xu = _mul(xm, um)
        at = _mul((ac * xu[0], ac * xu[1]), t)
        rho = (rm[0] - at[0], rm[1] - at[1])
        ti = 2.0 * xm[1]
        ck = _mul(wm, (-(ti * rho[1]), ti * rho[0]))
        c = ck if m == 0 else _add(c, ck)
    c = (_row16_sum(c[0]), _row16_sum(c[1]))
    s = (t[0] + c[0] / bc, t[1] + c[1] / bc)
    assert np.array_equal(s[0], s[0][..., :1].repeat(16, -1)), "every lane holds the same bits"
    return s


def masked(x, mask):
    """x as mmse_rank1_kernel holds it: zero off State::xmask (mask: [..., 53] of 0 / 1); rx is left alone."""
    return np.where(np.asarray(mask, bool), np.asarray(x, np.complex128), 0.0)


def model_h(cvec, tx, rx, ow2):
    """H[f] = u s_f for TEXTBOOK (a = 1, b = ow2, w = conj(u)); tx, rx [B, 53] complex128."""
    u = _lanes(np.broadcast_to(np.asarray(cvec, np.complex128), tx.shape))
    w = (u[0], -u[1])
    with np.errstate(all="ignore"):
        s = model_s(_lanes(tx), _lanes(rx), u, w, 1.0, float(ow2))
        h = _mul(u, (s[0][..., None, :], s[1][..., None, :]))
    return (h[0] + 1j * h[1]).reshape(tx.shape[0], 64)[:, :N]


def naive_h(cvec, tx, rx, ow2):
    """(rho^T rx - (rho^T al) t) / b in fp64: the form the kernel does NOT use."""
    u = np.asarray(cvec, np.complex128)
    al, be, rho = tx * u, u.conj() * tx.conj(), u.conj() * tx
    t = (be * rx).sum(-1) / (ow2 + (be * al).sum(-1))
    s = ((rho * rx).sum(-1) - (rho * al).sum(-1) * t) / ow2
    return u[None] * s[:, None]


# ---- frames
def _symbols(rng, kind, shape):
    if kind == "bpsk":
        x = (2.0 * rng.integers(0, 2, shape) - 1.0).astype(np.complex128)
    elif kind == "qpsk":
        x = ((2.0 * rng.integers(0, 2, shape) - 1) + 1j * (2.0 * rng.integers(0, 2, shape) - 1)) / np.sqrt(2.0)
    else:
        lv = np.array([-3.0, -1.0, 1.0, 3.0]) / np.sqrt(10.0)
        x = lv[rng.integers(0, 4, shape)] + 1j * lv[rng.integers(0, 4, shape)]
    x[..., DC] = 0.0
    return AMP * x


def make_frames(rng, kind, matched, hlt, ow2, n=B):
    x = _symbols(rng, kind, (n, N))
    if matched:
        h = np.broadcast_to(hlt, (n, N))
    else:
        amp = np.sqrt(np.mean(np.abs(hlt) ** 2) / 2.0)
        h = amp * (rng.standard_normal((n, N)) + 1j * rng.standard_normal((n, N)))
    noise = np.sqrt(ow2 / 2.0) * (rng.standard_normal((n, N)) + 1j * rng.standard_normal((n, N)))
    return x, h * x + noise


@pytest.fixture(scope="module")
def setup(golden, oracle):
    inp = golden["inputs"]
    F = oracle.fmatrix()
    hls = oracle.lt_ls(inp["tx_pre"], inp["rx_pre"])
    c = F @ (F.conj() @ hls / N)   # long double; the kernel reads it rounded to fp64 (State::cvec)
    return inp, c, np.asarray(hls, np.complex128)


def _closed(oracle, c, tx, rx, ow2):
    return np.stack([oracle.mmse_textbook_closed(c, tx[f], rx[f], ow2) for f in range(tx.shape[0])])


@pytest.mark.parametrize("matched", [True, False], ids=["matched", "unrelated"])
@pytest.mark.parametrize("kind", ["bpsk", "qpsk", "qam16"])
def test_model_against_long_double(setup, oracle, kind, matched):
    inp, c, hlt = setup
    rng = np.random.default_rng([0x51, ["bpsk", "qpsk", "qam16"].index(kind), int(matched)])
    tx, rx = make_frames(rng, kind, matched, hlt, inp["ow2"])
    cond = 1.0 + float(np.sum(np.abs(tx[0] * np.asarray(c, np.complex128)) ** 2)) / float(inp["ow2"])
    assert cond > 1e6, cond   # the ill-conditioned regime the form is built for
    err = normrel(model_h(c, tx, rx, inp["ow2"]), _closed(oracle, c, tx, rx, inp["ow2"]))
    print(f"\n{kind} {'matched' if matched else 'unrelated'}: max {err.max():.2e} (cond {cond:.1e})")
    assert err.max() < TOL, (int(err.argmax()), err.max())


def test_naive_form_is_worse(setup, oracle):
    """The reason for the split read-out: the one-line form loses ~6 digits on BPSK frames."""
    inp, c, hlt = setup
    rng = np.random.default_rng([0x51, 0, 1])
    tx, rx = make_frames(rng, "bpsk", True, hlt, inp["ow2"])
    ref = _closed(oracle, c, tx, rx, inp["ow2"])
    e_model = normrel(model_h(c, tx, rx, inp["ow2"]), ref).max()
    e_naive = normrel(naive_h(c, tx, rx, inp["ow2"]), ref).max()
    print(f"\nBPSK matched: model {e_model:.2e}, naive {e_naive:.2e}")
    assert e_model < 1e-12 and e_naive > 100 * e_model


def test_null_zero_and_tiny_symbols(setup, oracle):
    inp, c, hlt = setup
    rng = np.random.default_rng(0x52)
    tx, rx = make_frames(rng, "qpsk", True, hlt, inp["ow2"], n=8)
    # frame 0: only the DC null (already there); frame 1: more nulls; frame 2: all zero;
    # frames 3..: |x_k| scaled down to 1e-150 across the band (x^2 stays normal, 1e-300)
    tx[1, ::5] = 0.0
    tx[2] = 0.0
    rx[2] = 0.0
    scale = np.logspace(0, -150, N)
    for f in range(3, 8):
        tx[f] *= rng.permutation(scale)
        rx[f] = hlt * tx[f] + np.sqrt(inp["ow2"] / 2.0) * (rng.standard_normal(N) + 1j * rng.standard_normal(N))
    got = model_h(c, tx, rx, inp["ow2"])
    assert np.isfinite(got).all()
    assert np.all(got[2] == 0.0), "all-zero frame: s = 0, H = 0"
    live = [0, 1, 3, 4, 5, 6, 7]
    err = normrel(got[live], _closed(oracle, c, tx[live], rx[live], inp["ow2"]))
    print(f"\nnull / tiny symbols: max {err.max():.2e}")
    assert err.max() < TOL, err


# ---- the given-w branch (cwg) with a nonzero complex g: no public route reaches it
# (REF, its only caller, has a = 0), so the arithmetic is pinned here only
CW_PINS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rank1_cw_mp.npz")


def test_given_w_branch_against_mpmath():
    """model_s(..., cwg=True) against tests/golden/make_rank1_cw_mp.py: the 53 x 53
    matrix a diag(x) u w^T diag(x)^H + b I inverted by LU in mpmath at 50 digits,
    w a non-conjugate vector, plus REF's shape (a = 0, pilots only).  1e-10
    relative in s; the same algebra in long double stays below 1.3e-11 over 500
    frames per class, so the bound leaves the reference's own error out."""
    p = np.load(CW_PINS)
    tx, rx, mask, cls = p["tx"], p["rx"], p["mask"], p["cls"]
    n = tx.shape[0]
    assert n == 28 and len(p["cls_name"]) == 7
    assert np.all(p["a"][cls == 6] == 0.0) and np.all(mask[cls == 6].sum(-1) == 4), "the REF-shaped class"
    assert np.all(mask[cls < 6] == 1) and np.all(p["a"][cls < 6] == 1.0)
    u = _lanes(np.broadcast_to(p["u"], (n, N)))
    w = _lanes(p["w"][cls])
    assert np.abs(p["w"] - p["u"].conj()).max() > 0.05 * np.abs(p["u"]).max(), "w is not conj(u)"
    with np.errstate(all="ignore"):
        s = model_s(_lanes(masked(tx, mask)), _lanes(rx), u, w, p["a"][:, None], p["b"][:, None], cwg=True)
    got = (s[0][:, 0] + 1j * s[1][:, 0]).astype(np.clongdouble)
    ref = p["s_hi"].astype(np.clongdouble) + p["s_lo"].astype(np.clongdouble)
    err = np.asarray(np.abs(got - ref) / np.abs(ref), np.float64)
    for ci, nm in enumerate(p["cls_name"]):
        print(f"\n{nm}: max {err[cls == ci].max():.2e}", end="")
    assert err.max() < TOL, (int(err.argmax()), err.max())
    # the mask matters: with x left whole off the pilots the REF-shaped class moves
    with np.errstate(all="ignore"):
        s2 = model_s(_lanes(tx), _lanes(rx), u, w, p["a"][:, None], p["b"][:, None], cwg=True)
    assert not np.array_equal(s2[0][cls == 6], s[0][cls == 6])
    # and so does the branch: the real-g form on the same inputs is far off
    with np.errstate(all="ignore"):
        s3 = model_s(_lanes(masked(tx, mask)), _lanes(rx), u, w, p["a"][:, None], p["b"][:, None], cwg=False)
    g3 = (s3[0][:, 0] + 1j * s3[1][:, 0]).astype(np.clongdouble)
    assert np.asarray(np.abs(g3 - ref) / np.abs(ref), np.float64)[cls < 6].min() > 1e-6
