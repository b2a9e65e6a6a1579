"""Per-frame noise variance in the closed-form rank-1 PS_MMSE, on the CPU model.

wce_estimate_noise gives frame f its own b = ow2[f] in mmse_rank1_kernel
(csrc/wce_rank1.hip); nothing else in the kernel changes, so the fp64
transcription of tests/test_rank1_model.py (`model_h`, one call per frame with
that frame's ow2) is the device arithmetic.  It is checked here against the long
double closed form `oracle_py.mmse_textbook_closed(c, tx, rx, ow2[f])` at the
project's 1e-10 norm-relative, before anything runs on a GPU.

The range this fixes for tests/test_noise_gpu.py: ow2 log-uniform in
[OW2_LO, OW2_HI] = [1e-9, 1e-2], both ends included in every class -- the whole
range the issue asked for held, so the low end was not raised.  cond(Ryy) = 1 +
g / ow2 with g = 0.41 on the inputs.h preamble and symbol amplitude: 4e8 at the
low end, 42 at the high end (4.3e6 at the golden ow2 = 9.6172e-8).

Measured maxima (200 frames per class, the noise in rx drawn at each frame's own
ow2; the worst frame lies within a factor 3 of the low end, except QPSK
unrelated, which is flat):

    BPSK  matched 2.4e-11   unrelated 2.6e-11
    QPSK  matched 6.2e-12   unrelated 1.1e-14

Three other seeds of 300 frames per class gave at most 3.1e-11, 2.7e-11, 2.2e-11
and 1.6e-14.  With the low end at 3e-9 the same four read 7.8e-12, 7.3e-12,
1.5e-11, 2.8e-14; at 1e-8: 2.2e-12, 2.8e-12, 6.4e-12, 2.8e-14.  The BPSK figures are the oracle's own cancellation in long double (its
one-line form loses ~cond digits: 4e8 x 5e-20), as in tests/test_rank1_model.py.
"""
import numpy as np
import pytest

from oracle_py import N, normrel
from test_rank1_model import make_frames, model_h

TOL = 1e-10
OW2_LO, OW2_HI = 1e-9, 1e-2   # the range that held; tests/test_noise_gpu.py imports it
B = 200


def draw_ow2(rng, n, lo=OW2_LO, hi=OW2_HI):
    """n noise variances, log-uniform in [lo, hi], all different; the first two are the ends (n >= 2)."""
    v = np.exp(rng.uniform(np.log(lo), np.log(hi), n))
    v[:2] = (lo, hi)[:min(n, 2)]
    assert len(set(v.tolist())) == n
    return v


@pytest.fixture(scope="module")
def setup(golden, oracle):
    inp = golden["inputs"]
    F = oracle.fmatrix()
    hls = oracle.lt_ls(inp["tx_pre"], inp["rx_pre"])
    return F @ (F.conj() @ hls / N), np.asarray(hls, np.complex128)


@pytest.mark.parametrize("matched", [True, False], ids=["matched", "unrelated"])
@pytest.mark.parametrize("kind", ["bpsk", "qpsk"])
def test_model_with_per_frame_ow2(setup, oracle, kind, matched):
    c, hlt = setup
    rng = np.random.default_rng([0x0E2, ["bpsk", "qpsk"].index(kind), int(matched)])
    ow2 = draw_ow2(rng, B)
    tx, rx = make_frames(rng, kind, matched, hlt, 0.0, n=B)   # noiseless; each frame's noise at its own variance
    rx = rx + np.sqrt(ow2 / 2.0)[:, None] * (rng.standard_normal((B, N)) + 1j * rng.standard_normal((B, N)))
    got = np.concatenate([model_h(c, tx[f:f + 1], rx[f:f + 1], ow2[f]) for f in range(B)])
    ref = np.stack([oracle.mmse_textbook_closed(c, tx[f], rx[f], ow2[f]) for f in range(B)])
    err = normrel(got, ref)
    w = int(err.argmax())
    print(f"\n{kind} {'matched' if matched else 'unrelated'}: max {err.max():.2e} at ow2 = {ow2[w]:.2e}; "
          f"at the ends {err[0]:.2e}, {err[1]:.2e}")
    assert np.isfinite(got).all()
    assert err.max() < TOL, (w, ow2[w], err.max())


def test_a_frames_answer_moves_with_its_ow2(setup):
    """The check above is not vacuous: the same frame at two variances of the range differs far beyond 1e-10,
    and a batch at one common variance is model_h's batched answer bit for bit."""
    c, hlt = setup
    rng = np.random.default_rng(0x0E3)
    tx, rx = make_frames(rng, "qpsk", True, hlt, 9.6172e-8, n=8)
    a = model_h(c, tx, rx, 9.6172e-8)
    one = np.concatenate([model_h(c, tx[f:f + 1], rx[f:f + 1], 9.6172e-8) for f in range(8)])
    assert np.array_equal(a, one)
    b = model_h(c, tx, rx, 1e-4)
    assert normrel(b, a).min() > 1e-6
