"""wce_estimate_noise on the GPU: PS_MMSE with each frame's own noise variance
ow2[f] (mmse_rank1_kernel<*, true>, csrc/wce_rank1.hip), and Context.receive_host,
the batched WiFi_RX.m:17-60 receive chain built on it.

Frames are synthesised on the device (ctx.synth: BPSK data, 802.11 pilots, a DC
null, a 6-tap channel and a preamble of its own per frame, CN(0, 9.6172e-8)
noise); the estimator's ow2[f] is drawn log-uniformly from the range
tests/test_noise_model.py fixed on the CPU model, [1e-9, 1e-2], both ends
included, different for every frame.  Oracles, at the project's 1e-10
norm-relative: the long double closed form mmse_textbook_closed(c, tx, rx, ow2[f])
on every frame, and the long double 53 x 53 factorisation mmse_unified(C, ones, 1,
ow2[f], tx, rx) on the frames with ow2[f] >= the golden 9.6172e-8, the
conditioning at which the project's tests hold that bound for it.

The route a request takes is pinned on the CPU (tests/test_noise_route.py).

Measured on an MI355X, max norm-relative over the 33 frames (PS_MMSE alone and
ALL give the same figures; the worst frame is always the one at ow2 = 1e-9, where
the long double closed form itself cancels ~cond = 4e8 digits, as on the CPU):

    route                         closed form    factorisation (24 frames)
    shared covariance   C         2.5e-11        1.2e-13
    FRAME_COV           C         2.1e-11        1.2e-15
    shared covariance   MATLAB    1.4e-11        7.4e-15   (B <= 5: 3 frames)
    FRAME_COV           MATLAB    1.9e-11        9.2e-16   (B <= 5: 3 frames)

Receive chain, six packets (ow2 9.6e-8 ... 1.2e-3): 7.7e-13, 2.0e-13, 2.4e-13,
1.9e-13, 2.7e-14, 4.6e-14 against the long double chain.
"""
import contextlib

import numpy as np
import pytest

from oracle_py import N, NBLK, normrel
from test_noise_model import OW2_HI, OW2_LO, draw_ow2
from test_rank1_gpu import _cvec

pytestmark = pytest.mark.gpu

TOL = 1e-10
TOL_LS = 1e-13      # the LS family and eq against matlab.mat (tests/test_front_gpu.py)
OW2_GOLD = 9.6172e-8
BMAX = 33
BLOCK = 2           # C semantics estimates this block
OS = 61             # H row stride: columns 53..60 hold a sentinel that must survive
SENT = 7.0 - 3.0j
R1 = 5              # WCE_VARIANT_R1
LS_NAMES = ("lt_ls", "ps_linear", "ps_cubic", "ps_sinc")
BITS = ("lt_ls", "ps_linear", "ps_cubic", "ps_sinc", "ps_mmse")


class Env:
    """One TEXTBOOK context, 33 device-made frames with their preambles and noise variances, and the long
    double answers per (frame covariance, semantics), each computed once and left unchanged."""

    def __init__(self, wce, golden, oracle):
        self.wce, self.oracle = wce, oracle
        inp = self.inp = golden["inputs"]
        self.ctx = wce.Context(inp["tx_pre"], inp["rx_pre"], inp["ow2"], wce.MMSE_TEXTBOOK)
        self.ctx.reserve(BMAX)
        self.F = oracle.fmatrix()
        dtx, drx, dpre = wce.DeviceArray((BMAX, NBLK, N)), wce.DeviceArray((BMAX, NBLK, N)), wce.DeviceArray((BMAX, N))
        self.ctx.synth(dtx, drx, dpre, BMAX, seed=0x0E2)
        wce.synchronize()
        self.tx, self.rx, self.pre = dtx.numpy(), drx.numpy(), dpre.numpy()
        self.ow2 = draw_ow2(np.random.default_rng(0x0E4), BMAX)
        assert self.ow2.min() == OW2_LO and self.ow2.max() == OW2_HI
        assert 8 <= int((self.ow2 >= OW2_GOLD).sum()) < BMAX
        for a in (self.tx, self.rx, self.pre, self.ow2):
            a.setflags(write=False)
        self._ref = {}

    def expected(self, fc, sem):
        """([33][53] closed form, {frame: factorisation} for ow2[f] >= the golden value), long double"""
        if (fc, sem) not in self._ref:
            o, inp = self.oracle, self.inp
            ml = sem == "MATLAB"
            blocks = range(4) if ml else (BLOCK,)
            ones = np.ones(N, np.uint8)
            closed, fact = [], {}
            for f in range(BMAX):
                rp = self.pre[f] if fc else inp["rx_pre"]
                cf = _cvec(o, self.F, inp["tx_pre"], rp, matlab=ml and fc)
                closed.append(np.mean(np.stack([o.mmse_textbook_closed(cf, self.tx[f, b], self.rx[f, b], self.ow2[f])
                                                for b in blocks]), axis=0))
                if self.ow2[f] >= OW2_GOLD:
                    hls = (o.matlab_lt_ls if ml and fc else o.lt_ls)(inp["tx_pre"], rp)
                    C = o.mmse_textbook_cmatrix(self.F, hls)
                    fact[f] = np.mean(np.stack([o.mmse_unified(C, ones, 1, np.longdouble(self.ow2[f]), self.tx[f, b],
                                                               self.rx[f, b]) for b in blocks]), axis=0)
            self._ref[fc, sem] = (np.stack(closed), fact)
        return self._ref[fc, sem]


@pytest.fixture(scope="module")
def env(gpu_wce, golden, oracle):
    return Env(gpu_wce, golden, oracle)


def _run(wce, ctx, tx, rx, pre, mask, sem, ow2=None, ow2_offset=0, raw=None):
    """One wce_estimate (ow2 None) or wce_estimate_noise call on host frames: every H output in rows of stride
    OS, prefilled with a sentinel; returns the outputs (H: the 53 live columns).  ow2_offset: bytes added to
    the ow2 pointer (the misaligned-pointer error); raw: a dict that receives every output buffer as the device
    holds it after the call, also when the call raises."""
    B = tx.shape[0]
    dev = wce.DeviceArray.from_numpy
    dtx, drx = dev(np.asarray(tx, np.complex128)), dev(np.asarray(rx, np.complex128))
    dpre = dev(np.asarray(pre, np.complex128)) if pre is not None else None
    bufs = {n: dev(np.full((B, OS), SENT, np.complex128)) for i, n in enumerate(BITS) if mask & (1 << i)}
    deq = dev(np.full((B, NBLK, N), SENT, np.complex128)) if mask & wce.EQUALIZE else None
    o = wce.Outputs(*[(bufs[n].addr if n in bufs else None) for n in BITS], deq.addr if deq is not None else None,
                    OS, NBLK * N, N, wce.PS_LINEAR, 0)
    fr = ctx.frames(dtx, drx, B, rx_pre=dpre, block=BLOCK, semantics=wce.SEM_MATLAB if sem == "MATLAB" else wce.SEM_C)
    dow2 = None
    if ow2 is not None:
        dow2 = dev(np.concatenate([np.asarray(ow2, np.float64), [0.0]]))   # a spare double behind the B entries
    raw = {} if raw is None else raw
    try:
        ctx.estimate(fr, o, mask, ow2=None if dow2 is None else dow2.addr + ow2_offset)
    finally:
        wce.synchronize()
        raw.update({n: d.numpy() for n, d in bufs.items()})
        if deq is not None:
            raw["eq"] = deq.numpy()
    res = {}
    for n in bufs:
        assert np.all(raw[n][:, N:] == SENT), f"{n}: columns past 52 were written"
        res[n] = np.ascontiguousarray(raw[n][:, :N])
    if deq is not None:
        res["eq"] = raw["eq"]
    return res


def _request(env, B, fc, full, sem, ow2="own", frames=None):
    """the first B frames (or `frames`) through one call; ow2: "own" (each frame's), None (wce_estimate), or an array"""
    wce = env.wce
    idx = np.arange(B) if frames is None else np.asarray(frames)
    mask = (wce.ALL if full else wce.PS_MMSE) | (wce.FRAME_COV if fc else 0)
    pre = env.pre[idx] if fc or full else None
    v = env.ow2[idx] if isinstance(ow2, str) else ow2
    return _run(wce, env.ctx, env.tx[idx], env.rx[idx], pre, mask, sem, ow2=v)


def _check_parity(env, out, B, fc, sem, tag):
    closed, fact = env.expected(fc, sem)
    assert np.isfinite(out).all()
    e = normrel(out, closed[:B])
    big = [f for f in fact if f < B]
    e2 = normrel(out[big], np.stack([fact[f] for f in big])) if big else np.zeros(1)
    print(f"\n{tag} B={B}: closed form max {e.max():.2e} at ow2 = {env.ow2[int(e.argmax())]:.1e}; "
          f"factorisation ({len(big)} frames) max {e2.max():.2e}")
    assert e.max() < TOL, (int(e.argmax()), e.max())
    assert e2.max() < TOL, (big[int(e2.argmax())], e2.max())


@pytest.mark.parametrize("full", [False, True], ids=["mmse", "all"])
@pytest.mark.parametrize("fc", [False, True], ids=["shared", "frame_cov"])
@pytest.mark.parametrize("B", [1, 15, 16, 17, 33])
def test_parity_c(env, B, fc, full):
    """16 units per 256-thread workgroup: a lone row, one short of a workgroup, a full one, ragged last ones."""
    out = _request(env, B, fc, full, "C")
    _check_parity(env, out["ps_mmse"], B, fc, "C", f"C {'frame_cov' if fc else 'shared'} {'all' if full else 'mmse'}")
    if full:   # the LS family and the equalized symbols do not depend on ow2: wce_estimate's bits
        plain = _request(env, B, fc, full, "C", ow2=None)
        for k in LS_NAMES + ("eq",):
            assert np.array_equal(out[k], plain[k]), k
        assert not np.array_equal(out["ps_mmse"], plain["ps_mmse"])


@pytest.mark.parametrize("fc", [False, True], ids=["shared", "frame_cov"])
@pytest.mark.parametrize("B", [1, 3, 4, 5])
def test_parity_matlab(env, B, fc):
    """Split: unit g = 4 f + b, 4, 12, 16 and 20 units; b = ow2[f] for all four blocks of frame f.  The
    oracle: the mean over blocks 0..3 of its per-block answers."""
    out = _request(env, B, fc, False, "MATLAB")
    _check_parity(env, out["ps_mmse"], B, fc, "MATLAB", f"MATLAB {'frame_cov' if fc else 'shared'}")


@pytest.mark.parametrize("fc", [False, True], ids=["shared", "frame_cov"])
@pytest.mark.parametrize("sem", ["C", "MATLAB"])
def test_bit_contract(env, sem, fc):
    # every ow2[f] = the context's ow2: wce_estimate's bits, every output
    same = np.full(BMAX, env.inp["ow2"], np.float64)
    plain = _request(env, BMAX, fc, True, sem, ow2=None)
    got = _request(env, BMAX, fc, True, sem, ow2=same)
    assert set(got) == set(plain) == set(BITS) | {"eq"}
    for k in plain:
        assert np.array_equal(got[k], plain[k]), k
    # a frame's bits depend on its own data and its own ow2[f]: permuting both permutes the rows
    own = _request(env, BMAX, fc, True, sem)
    perm = np.random.default_rng(0x0E5).permutation(BMAX)
    assert not np.array_equal(perm, np.arange(BMAX))
    moved = _request(env, BMAX, fc, True, sem, frames=perm)
    for k in own:
        assert np.array_equal(moved[k], own[k][perm]), k
    # and not on the batch: a frame estimated alone
    alone = _request(env, 1, fc, True, sem, frames=[BMAX - 1])
    for k in own:
        assert np.array_equal(alone[k][0], own[k][BMAX - 1]), k


@contextlib.contextmanager
def _knobs(wce, ctx, variant, bdot):
    lib = wce.load()
    try:
        assert lib.wce_debug_set_variant(R1, variant) == 0
        ctx.set_border_dot(bdot)
        yield
    finally:
        assert lib.wce_debug_set_variant(R1, 0) == 0
        ctx.set_border_dot(True)


@pytest.mark.parametrize("fc", [False, True], ids=["shared", "frame_cov"])
@pytest.mark.parametrize("sem", ["C", "MATLAB"])
def test_knob_independence(env, sem, fc):
    """The factorising kernels have no per-frame-noise build: the A/B knobs that select them for wce_estimate
    leave a noise request on the closed form, bit for bit; the nontemporal build gives the same bits too."""
    want = _request(env, BMAX, fc, True, sem)
    for variant, bdot in ((1, True), (0, False), (1, False), (2, True)):
        with _knobs(env.wce, env.ctx, variant, bdot):
            got = _request(env, BMAX, fc, True, sem)
        for k in want:
            assert np.array_equal(got[k], want[k]), (variant, bdot, k)


@pytest.mark.parametrize("fc", [False, True], ids=["shared", "frame_cov"])
@pytest.mark.parametrize("sem", ["C", "MATLAB"])
def test_invalid_entries(env, sem, fc):
    """A value check, not a fault: every memory access is the one a valid run makes."""
    wce, B = env.wce, 20
    bad = {3: 0.0, 7: -1e-8, 11: np.nan, 19: np.inf}
    ow2 = np.array(env.ow2[:B])
    for f, v in bad.items():
        ow2[f] = v
    valid = _request(env, B, fc, True, sem)
    got = _request(env, B, fc, True, sem, ow2=ow2)
    H = got["ps_mmse"]
    for f in range(B):
        if f in bad:
            assert np.isnan(H[f].real).all() and np.isnan(H[f].imag).all(), f
        else:
            assert np.array_equal(H[f], valid["ps_mmse"][f]), f
    for k in LS_NAMES + ("eq",):   # no other output of those frames is affected
        assert np.array_equal(got[k], valid[k]), k
    bits, count = env.ctx.nonfinite_scan(wce.DeviceArray.from_numpy(H), B)
    assert count == 4 and bits.tolist() == [sum(1 << f for f in bad)]
    # -0.0 and a subnormal: zero is not positive, the smallest positive double is
    ow2 = np.array(env.ow2[:B])
    ow2[5], ow2[6] = -0.0, 5e-324
    H = _request(env, B, fc, False, sem, ow2=ow2)["ps_mmse"]
    assert np.isnan(H[5].view(np.float64)).all() and not np.isnan(H[6].view(np.float64)).any()
    assert np.array_equal(np.delete(H, [5, 6], 0), np.delete(valid["ps_mmse"], [5, 6], 0))


def test_errors_write_nothing(env, golden):
    """Rejected before any launch: nothing is written, and wce_last_error() says why."""
    wce, inp = env.wce, env.inp
    B = 5
    pdp = np.exp(-0.05 * np.arange(N))
    ref = wce.Context(inp["tx_pre"], inp["rx_pre"], inp["ow2"], wce.MMSE_REF)
    cov = wce.Context(inp["tx_pre"], inp["rx_pre"], inp["ow2"], Rhh=np.diag(pdp / pdp.sum() * 1.1e-4 + 0j))
    cases = [(c, wce.ALL | fcb, "C", 0, "TEXTBOOK") for c in (ref, cov) for fcb in (0, wce.FRAME_COV)]
    cases += [(env.ctx, wce.LS_ALL | wce.EQUALIZE, "C", 0, "without WCE_EST_PS_MMSE"),
              (env.ctx, wce.LT_LS, "MATLAB", 0, "without WCE_EST_PS_MMSE"),
              (env.ctx, wce.ALL, "C", 4, "aligned"), (env.ctx, wce.PS_MMSE | wce.FRAME_COV, "MATLAB", 4, "aligned")]
    for ctx, mask, sem, off, what in cases:
        raw = {}
        with pytest.raises(wce.WceError) as e:
            _run(wce, ctx, env.tx[:B], env.rx[:B], env.pre[:B], mask, sem, ow2=env.ow2[:B], ow2_offset=off, raw=raw)
        assert e.value.code == -1 and what in wce.load().wce_last_error().decode(), (what, str(e.value))
        assert raw and all(np.all(a == SENT) for a in raw.values()), what
        # the same request without ow2 is served (the misaligned ones: with the pointer as allocated)
        out = _run(wce, ctx, env.tx[:B], env.rx[:B], env.pre[:B], mask, sem,
                   ow2=env.ow2[:B] if off else None)
        assert all(np.isfinite(v).all() for v in out.values()), what


def test_receive_chain(gpu_wce, golden, oracle):
    """Context.receive_host, WiFi_RX.m:17-60 for 6 packets in one pass: matlab.mat's packet, and the same
    received packet and long training field under added noise of five powers, so that every packet has its
    own preamble estimate and its own sigma^2 (WiFi_RX.m:30), both consumed on the device."""
    wce, m = gpu_wce, golden["matlab"]
    B = 6
    rng = np.random.default_rng(0x0E6)
    power = np.array([0.0, 1e-7, 1e-6, 1e-5, 1e-4, 1e-3])   # per complex sample; ow2 rises by about as much

    def noisy(a):
        z = rng.standard_normal((B,) + a.shape) + 1j * rng.standard_normal((B,) + a.shape)
        return a[None] + np.sqrt(power / 2.0)[:, None] * z

    rx_pk, rx_lp = noisy(m["rx_packet"]), noisy(m["rx_lptot"])
    tx_pk, tx_lp = np.repeat(m["tx_packet"][None], B, 0), np.repeat(m["tx_lptot"][None], B, 0)
    ctx = wce.Context(m["tx_preamble_fft"], m["rx_preamble_fft"], 9.6172e-8, wce.MMSE_TEXTBOOK)
    out = ctx.receive_host(tx_pk, tx_lp, rx_pk, rx_lp, mask=wce.ALL, semantics=wce.SEM_MATLAB)
    # frame 0 is the one-packet chain of tests/test_front_gpu.py
    for name, key in (("lt_ls", "H_EST_LT_LS"), ("ps_linear", "H_EST_PS_Linear"), ("ps_cubic", "H_EST_PS_Cubic"),
                      ("ps_sinc", "H_EST_PS_Sinc")):
        assert normrel(out[name][0], m[key]) < TOL_LS, name
    ref_eq = m["eq_symbols"].T
    assert np.max(np.abs(out["eq"][0] - ref_eq)) / np.max(np.abs(ref_eq)) < TOL_LS
    ow2 = out["ow2"]
    print("\nreceive chain ow2:", " ".join(f"{v:.3e}" for v in ow2))
    assert ow2.shape == (B,) and np.all(ow2 >= 9.6e-8) and len(set(ow2.tolist())) == B
    assert abs(ow2[0] - 9.6172e-8) < 1e-11
    # every frame's PS_MMSE: the oracle's chain in long double, with that frame's own preamble and sigma^2
    F = oracle.fmatrix()
    tpre, _ = oracle.front_preamble(m["tx_lptot"])
    tsym = oracle.front_blocks(m["tx_packet"], 4)
    ones = np.ones(N, np.uint8)
    errs = []
    for f in range(B):
        rpre, s2 = oracle.front_preamble(rx_lp[f])
        assert abs(ow2[f] - float(s2)) <= 1e-14 * float(s2)
        rsym = oracle.front_blocks(rx_pk[f], 4)
        C = oracle.mmse_textbook_cmatrix(F, oracle.matlab_lt_ls(tpre, rpre))
        ref = np.mean(np.stack([oracle.mmse_unified(C, ones, 1, s2, tsym[b], rsym[b]) for b in range(4)]), axis=0)
        errs.append(float(normrel(out["ps_mmse"][f], ref)))
    print("receive chain ps_mmse vs oracle:", " ".join(f"{e:.2e}" for e in errs))
    assert max(errs) < TOL, errs
    bits, count = ctx.nonfinite_scan(wce.DeviceArray.from_numpy(out["ps_mmse"]), B)
    assert count == 0 and not bits.any()
