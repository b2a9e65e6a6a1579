"""Carrier frequency offset estimation and correction in the front end, on the
GPU: wce_front_end_preamble_cfo (front_cfo_kernel<true>: the two-copy estimate
and the derotation of the long training field) and wce_front_end_blocks_cfo
(front_cfo_kernel<false>: the derotation of the packet), csrc/wce_front.hip,
and Context.receive_host(cfo=True) on top of them.

The reference is the long double model of tests/cfo_model.py.  It always
derotates with the cfo[f] the device wrote (read back), so the estimate and the
derotation are judged separately.  Bounds (tests/test_cfo_abi.py derives them
and shows fp64 arithmetic meets them): bins 2e-14 max-norm relative, the estimate
1e-16 cycles per sample, ow2 1e-12 relative.

Measured on an MI355X: blocks with a given offset 2.0e-16 ... 3.9e-16 (B = 3 and
777, sample offsets 0, 160, -7, 400); preamble with a given offset 3.5e-16, ow2
6.2e-16; estimate (B = 1, 9, 777) within 1.3e-18 cycles per sample of the long
double one, bins 4.9e-16, ow2 3.0e-14.  matlab.mat's packet and the same packet
under 20 kHz through receive_host(cfo=True): cfo -2.580319e-07 and 1.999742e-03
(difference off 0.002 by 4.3e-19), the LS family within 1.0e-15, eq 4.4e-15,
ps_mmse 8.2e-16; symbols against rx_symb 1.85e-3 (bound 3.89e-3).
"""
import numpy as np
import pytest

import cfo_model as cm
from oracle_py import N, NBLK, normrel

pytestmark = pytest.mark.gpu

TOL_BINS = 2e-14
TOL_EST = 1e-16
TOL_OW2 = 1e-12
SENT = 7.0 - 3.0j
L, LSTRIDE, PRESTRIDE = 160, 171, 56
PSTRIDE, FS, BS = NBLK * 80 + 9, NBLK * 64 + 3, 60      # the padded strides of test_front_end_batch_vs_oracle
EINVAL = -1


@pytest.fixture(scope="module")
def fe_ctx(gpu_wce):
    return gpu_wce.Context(empty=True)


def _nan(a):
    return np.isnan(np.ascontiguousarray(a).view(np.float64))


def _blocks(wce, ctx, pk, cfo, off=0, fs=NBLK * N, bs=N, fill=0.0, raw_null=False, cfo_shift=0):
    """One blocks call on host packets [B][stride]: cfo None -> wce_front_end_blocks; an array -> _cfo with it;
    raw_null -> _cfo with cfo == NULL.  Returns sym [B][fs] as the device holds it, also when the call raises
    (then as the second value of the exception's args)."""
    B = pk.shape[0]
    dpk = wce.DeviceArray.from_numpy(np.ascontiguousarray(pk, np.complex128))
    dsym = wce.DeviceArray.from_numpy(np.full((B, fs), fill, np.complex128))
    dcfo = None if cfo is None else wce.DeviceArray.from_numpy(np.concatenate([np.asarray(cfo, np.float64), [0.0]]))
    try:
        if raw_null:
            rc = wce.load().wce_front_end_blocks_cfo(ctx.handle, dpk.addr, pk.shape[1], B, NBLK, None, off, dsym.addr,
                                                     fs, bs, None)
            assert rc == 0
        else:
            ctx.front_end_blocks(dpk, B, NBLK, dsym, packet_stride=pk.shape[1], frame_stride=fs, block_stride=bs,
                                 cfo=None if dcfo is None else dcfo.addr + cfo_shift, sample_offset=off)
    except wce.WceError as e:
        wce.synchronize()
        e.args += (dsym.numpy(),)
        raise
    wce.synchronize()
    return dsym.numpy()


def _preamble(wce, ctx, lp, cfo=None, estimate=True, fill=0.0, lptot_len=L, cfo_shift=0):
    """One preamble call on host fields [B][LSTRIDE]: cfo None -> the plain call; "new" -> _cfo writing its
    estimate into a buffer prefilled with 9.0; an array -> _cfo reading it (estimate False) or overwriting it.
    Returns (pre [B][PRESTRIDE], ow2 [B], cfo [B] or None), also when the call raises (as for _blocks)."""
    B = lp.shape[0]
    dlp = wce.DeviceArray.from_numpy(np.ascontiguousarray(lp, np.complex128))
    dpre = wce.DeviceArray.from_numpy(np.full((B, PRESTRIDE), fill, np.complex128))
    dow2 = wce.DeviceArray.from_numpy(np.full(B, np.real(fill), np.float64))
    dcfo = None
    if cfo is not None:
        init = np.full(B, 9.0) if isinstance(cfo, str) else np.asarray(cfo, np.float64)
        dcfo = wce.DeviceArray.from_numpy(np.concatenate([init, [0.0]]))
    out = lambda: (dpre.numpy(), dow2.numpy(), None if dcfo is None else dcfo.numpy()[:B])
    try:
        ctx.front_end_preamble(dlp, B, lptot_len, dpre, dow2, lptot_stride=lp.shape[1], pre_stride=PRESTRIDE,
                               cfo=None if dcfo is None else dcfo.addr + cfo_shift, estimate_cfo=estimate)
    except wce.WceError as e:
        wce.synchronize()
        e.args += (out(),)
        raise
    wce.synchronize()
    return out()


def _bins(sym, bs):
    return np.stack([sym[:, b * bs:b * bs + N] for b in range(NBLK)], axis=1)


class Big:
    """777 random frames with the padded strides, their offsets, and the long double answers, made once"""

    def __init__(self):
        rng = np.random.default_rng(0xCF3)
        self.B = 777
        self.pk = cm.random_packets(rng, self.B, PSTRIDE)
        self.lp = cm.random_packets(rng, self.B, LSTRIDE)
        self.eps = cm.draw_eps(rng, self.B)
        for a in (self.pk, self.lp, self.eps):
            a.setflags(write=False)
        self._ref = {}

    def blocks_ref(self, off):
        if off not in self._ref:
            self._ref[off] = cm.blocks(self.pk, self.eps, off)
        return self._ref[off]


@pytest.fixture(scope="module")
def big():
    return Big()


# ---------------------------------------------------------------- 1. derotation with a given eps
@pytest.mark.parametrize("off", [0, 160, -7, 400])
def test_blocks_given_small(gpu_wce, fe_ctx, off):
    """B = 3: 45 units, 5 full waves of 8 and a last one with 5 live groups and 3 dead ones"""
    rng = np.random.default_rng(0xCF4)
    pk, eps = cm.random_packets(rng, 3, NBLK * 80), cm.draw_eps(rng, 3)
    eps[2] = rng.uniform(-cm.EPS_MAX, cm.EPS_MAX)      # 0.002, -0.002 and a random one
    sym = _blocks(gpu_wce, fe_ctx, pk, eps, off)
    err = cm.relmax(sym.reshape(3, NBLK, N), cm.blocks(pk, eps, off))
    print(f"\nblocks B=3 offset {off}: {err:.2e}")
    assert err <= TOL_BINS


@pytest.mark.parametrize("off", [400, -7])
def test_blocks_given_batch(gpu_wce, fe_ctx, big, off):
    sym = _blocks(gpu_wce, fe_ctx, big.pk, big.eps, off, FS, BS)
    got = _bins(sym, BS)
    err = cm.relmax(got, big.blocks_ref(off))
    per = np.max(np.abs(got - big.blocks_ref(off)), axis=(1, 2)) / np.max(np.abs(big.blocks_ref(off)))
    print(f"\nblocks B=777 offset {off}: {err:.2e}; the fixed offsets {cm.EPS_FIXED}: "
          + " ".join(f"{float(x):.1e}" for x in per[:5]))
    assert err <= TOL_BINS
    for b in range(NBLK - 1):   # untouched padding stays zero
        assert np.all(sym[:, b * BS + N:(b + 1) * BS] == 0)
    assert np.all(sym[:, (NBLK - 1) * BS + N:] == 0)


def test_preamble_given_batch(gpu_wce, fe_ctx, big):
    pre, ow2, cfo = _preamble(gpu_wce, fe_ctx, big.lp, big.eps, estimate=False)
    assert np.array_equal(cfo, big.eps)                 # read, not written
    rp, rw = cm.preamble(big.lp[:, :L], big.eps)
    err, ew = cm.relmax(pre[:, :N], rp), float(np.max(np.abs(ow2 / rw - 1)))
    print(f"\npreamble given B=777: bins {err:.2e}, ow2 {ew:.2e}")
    assert err <= TOL_BINS and ew <= TOL_OW2
    assert np.all(pre[:, N:] == 0)


# ---------------------------------------------------------------- 2. bit identity
def test_zero_offset_is_the_plain_call(gpu_wce, fe_ctx, big):
    wce = gpu_wce
    plain = _blocks(wce, fe_ctx, big.pk, None, 0, FS, BS)
    assert np.array_equal(_blocks(wce, fe_ctx, big.pk, None, 123, FS, BS, raw_null=True).view(np.uint64),
                          plain.view(np.uint64))
    for off in (0, 400):
        assert np.array_equal(_blocks(wce, fe_ctx, big.pk, np.zeros(big.B), off, FS, BS).view(np.uint64),
                              plain.view(np.uint64))
    assert not np.array_equal(_blocks(wce, fe_ctx, big.pk, big.eps, 0, FS, BS), plain)
    pre0, ow0, _ = _preamble(wce, fe_ctx, big.lp)
    pre1, ow1, _ = _preamble(wce, fe_ctx, big.lp, np.zeros(big.B), estimate=False)
    assert np.array_equal(pre1.view(np.uint64), pre0.view(np.uint64))
    assert np.array_equal(ow1.view(np.uint64), ow0.view(np.uint64))


# ---------------------------------------------------------------- 3. estimate
@pytest.mark.parametrize("B", [1, 9, 777])
def test_estimate(gpu_wce, fe_ctx, B):
    rng = np.random.default_rng(0xCF5)
    lp, eps, snr = cm.ltf_batch(rng, B, L, LSTRIDE)
    pre, ow2, cfo = _preamble(gpu_wce, fe_ctx, lp, "new")
    e_ld = cm.estimate(lp[:, :L])
    d_est = float(np.max(np.abs(cfo - e_ld)))
    rp, rw = cm.preamble(lp[:, :L], cfo)                # derotated with what the device wrote
    d_pre, d_ow = cm.relmax(pre[:, :N], rp), float(np.max(np.abs(ow2 / rw - 1)))
    print(f"\nestimate B={B}: cfo {d_est:.2e} cycles/sample, bins {d_pre:.2e}, ow2 {d_ow:.2e}")
    assert d_est <= TOL_EST
    assert d_pre <= TOL_BINS
    assert d_ow <= TOL_OW2
    assert np.all(pre[:, N:] == 0)
    # the data exercises the feature: uncorrected, the 20 kHz frames' sigma^2 is more than 10x too large
    raw = _preamble(gpu_wce, fe_ctx, lp)[1]
    for f in range(min(B, 2)):
        assert abs(eps[f]) == 0.002 and raw[f] > 10 * float(rw[f]), f
    # an all-zero field: c = 0, cfo = 0, the frame as the plain call leaves it
    z = np.zeros((2, LSTRIDE), np.complex128)
    z[1, :L] = -0.0
    pz, oz, cz = _preamble(gpu_wce, fe_ctx, z, "new")
    assert np.all(cz == 0) and np.all(oz == 0) and np.all(pz == 0)


# ---------------------------------------------------------------- 4. shift invariance through the chain
def test_receive_chain_shift_invariance(gpu_wce, golden):
    wce, m = gpu_wce, golden["matlab"]
    e0 = 0.002                                           # 20 kHz at 10 MHz (WiFi_RX.m:4-9)
    pk0, lp0 = m["rx_packet"], m["rx_lptot"]
    pk1 = cm.apply_cfo(pk0, e0, np.arange(len(pk0)))
    lp1 = cm.apply_cfo(lp0, e0, np.arange(len(lp0)) - len(lp0))
    ctx = wce.Context(m["tx_preamble_fft"], m["rx_preamble_fft"], 9.6172e-8, wce.MMSE_TEXTBOOK)
    run = lambda pk, lp, cfo: ctx.receive_host(m["tx_packet"][None], m["tx_lptot"][None], pk[None], lp[None],
                                               mask=wce.ALL, semantics=wce.SEM_MATLAB, cfo=cfo)
    a, b = run(pk0, lp0, True), run(pk1, lp1, True)
    d = abs((b["cfo"][0] - a["cfo"][0]) - e0)
    print(f"\ncfo {a['cfo'][0]:.6e} and {b['cfo'][0]:.6e}: difference off 0.002 by {d:.2e}")
    assert d <= 2e-16
    for k in ("lt_ls", "ps_linear", "ps_cubic", "ps_sinc"):
        e = float(normrel(b[k][0], a[k][0]))
        print(f"{k}: {e:.2e}")
        assert e <= 1e-11, k
    e = cm.relmax(b["eq"], a["eq"])
    em = float(normrel(b["ps_mmse"][0], a["ps_mmse"][0]))
    print(f"eq: {e:.2e}  ps_mmse: {em:.2e}  ow2: {a['ow2'][0]:.6e} {b['ow2'][0]:.6e}")
    assert e <= 1e-11 and em <= 1e-10
    # uncorrected, the rotated packet is far off
    plain = run(pk1, lp1, False)
    assert "cfo" not in plain
    assert float(normrel(plain["ps_linear"][0], a["ps_linear"][0])) > 0.1
    # against the recording, which was corrected before it was stored: a tiny residual offset
    assert abs(a["cfo"][0]) < 1e-6
    sym, pre, ow2, cfo = wce.Context(empty=True).front_end_host(pk0[None], lp0[None], cfo=True)
    assert cfo[0] == a["cfo"][0] and ow2[0] == a["ow2"][0]
    es = cm.relmax(sym[0], m["rx_symb"].T)
    bound = 2 * 2 * np.pi * abs(cfo[0]) * 1200
    print(f"symbols against rx_symb: {es:.2e} (bound {bound:.2e})")
    assert es <= bound


# ---------------------------------------------------------------- 5. mixed batch
def test_mixed_batch_is_frame_by_frame(gpu_wce, golden):
    wce, m = gpu_wce, golden["matlab"]
    B = 6
    rng = np.random.default_rng(0xCF6)
    offs = np.array([0.0, 20e3, -20e3, 70e3, -70e3, 5e3]) / 10e6
    # added noise per complex sample, on a signal of 1e-4 that carries 9.6e-8 already: 30 ... 10 dB; the two-copy
    # estimate's rms error at 10 dB is 1 / (2 pi 64 sqrt(64 * 10)) = 1e-4 cycles per sample
    power = np.array([0.0, 1e-7, 3e-7, 1e-6, 3e-6, 1e-5])
    npk, nlp = len(m["rx_packet"]), len(m["rx_lptot"])
    noise = lambda n: np.sqrt(power / 2)[:, None] * (rng.standard_normal((B, n)) + 1j * rng.standard_normal((B, n)))
    rx_pk = cm.apply_cfo(m["rx_packet"][None] + noise(npk), offs[:, None], np.arange(npk)[None, :])
    rx_lp = cm.apply_cfo(m["rx_lptot"][None] + noise(nlp), offs[:, None], (np.arange(nlp) - nlp)[None, :])
    tx_pk, tx_lp = np.repeat(m["tx_packet"][None], B, 0), np.repeat(m["tx_lptot"][None], B, 0)
    ctx = wce.Context(m["tx_preamble_fft"], m["rx_preamble_fft"], 9.6172e-8, wce.MMSE_TEXTBOOK)
    kw = dict(mask=wce.ALL, semantics=wce.SEM_MATLAB, cfo=True)
    out = ctx.receive_host(tx_pk, tx_lp, rx_pk, rx_lp, **kw)
    print("\nmixed batch cfo:", " ".join(f"{v:+.6f}" for v in out["cfo"]))
    assert np.max(np.abs(out["cfo"] - offs)) < 5e-4 and len(set(out["ow2"].tolist())) == B
    assert all(np.isfinite(v).all() for v in out.values())
    for f in range(B):
        one = ctx.receive_host(tx_pk[f:f + 1], tx_lp[f:f + 1], rx_pk[f:f + 1], rx_lp[f:f + 1], **kw)
        assert set(one) == set(out)
        for k in out:
            assert np.array_equal(np.ascontiguousarray(one[k][0]).view(np.uint8),
                                  np.ascontiguousarray(out[k][f]).view(np.uint8)), (f, k)


# ---------------------------------------------------------------- 6. bad input and errors
def test_nonfinite_offset_poisons_its_frame_only(gpu_wce, fe_ctx):
    wce = gpu_wce
    rng = np.random.default_rng(0xCF7)
    B, bad = 6, {2: np.nan, 4: np.inf}
    pk, lp, eps = cm.random_packets(rng, B, NBLK * 80), cm.random_packets(rng, B, LSTRIDE), cm.draw_eps(rng, B)
    dirty = eps.copy()
    for f, v in bad.items():
        dirty[f] = v
    clean_sym, (clean_pre, clean_ow, _) = _blocks(wce, fe_ctx, pk, eps, 160), _preamble(wce, fe_ctx, lp, eps, False)
    sym, (pre, ow, _) = _blocks(wce, fe_ctx, pk, dirty, 160), _preamble(wce, fe_ctx, lp, dirty, False)
    for f in range(B):
        if f in bad:
            assert _nan(sym[f]).all() and _nan(pre[f, :N]).all() and np.isnan(ow[f]), f
            assert np.all(pre[f, N:] == 0)
        else:
            assert np.array_equal(sym[f].view(np.uint64), clean_sym[f].view(np.uint64)), f
            assert np.array_equal(pre[f].view(np.uint64), clean_pre[f].view(np.uint64)) and ow[f] == clean_ow[f], f
    bits, count = fe_ctx.nonfinite_scan(wce.DeviceArray.from_numpy(pre), B, stride=PRESTRIDE)
    assert count == 2 and bits.tolist() == [sum(1 << f for f in bad)]
    bits, count = fe_ctx.nonfinite_scan(wce.DeviceArray.from_numpy(sym), B * NBLK)   # one row per block
    want = sum(1 << u for f in bad for u in range(f * NBLK, (f + 1) * NBLK))
    assert count == 2 * NBLK and sum(int(w) << (32 * i) for i, w in enumerate(bits)) == want


def test_nonfinite_sample_poisons_its_frame_only(gpu_wce, fe_ctx):
    wce = gpu_wce
    rng = np.random.default_rng(0xCF8)
    B = 9
    lp, _, _ = cm.ltf_batch(rng, B, L, LSTRIDE)
    dirty = lp.copy()
    dirty[3, L - 70] = complex(np.nan, 1.0)      # in p2
    dirty[7, L - 1] = complex(2.0, np.inf)       # the last sample of p1
    dirty[5, L] = complex(np.nan, np.nan)        # behind the field: not part of it
    dirty[6, L - 129] = complex(np.inf, 0.0)     # before p2: not read
    clean = _preamble(wce, fe_ctx, lp, "new")
    for est in (True, False):
        pre, ow, cfo = _preamble(wce, fe_ctx, dirty, "new" if est else clean[2], est)
        for f in range(B):
            if f in (3, 7):
                assert _nan(pre[f, :N]).all() and np.isnan(ow[f]) and np.all(pre[f, N:] == 0), (est, f)
                assert np.isnan(cfo[f]) if est else cfo[f] == clean[2][f]
            else:
                assert np.array_equal(pre[f].view(np.uint64), clean[0][f].view(np.uint64)), (est, f)
                assert ow[f] == clean[1][f] and cfo[f] == clean[2][f], (est, f)
        bits, count = fe_ctx.nonfinite_scan(wce.DeviceArray.from_numpy(pre), B, stride=PRESTRIDE)
        assert count == 2 and bits.tolist() == [(1 << 3) | (1 << 7)]


def test_errors_write_nothing(gpu_wce, fe_ctx):
    wce = gpu_wce
    rng = np.random.default_rng(0xCF9)
    B = 4
    pk, lp, eps = cm.random_packets(rng, B, NBLK * 80), cm.random_packets(rng, B, LSTRIDE), cm.draw_eps(rng, B)
    last = lambda: wce.load().wce_last_error().decode()

    def refused(call, what):
        with pytest.raises(wce.WceError) as e:
            call()
        assert e.value.code == EINVAL and what in last(), (what, last())
        return e.value.args[-1]

    sym = refused(lambda: _blocks(wce, fe_ctx, pk, eps, fill=SENT, cfo_shift=4), "aligned")
    assert np.all(sym == SENT)
    for off in (1 << 31, -(1 << 31), 1 << 40):
        sym = refused(lambda: _blocks(wce, fe_ctx, pk, eps, off, fill=SENT), "sample_offset")
        assert np.all(sym == SENT)
    sym = refused(lambda: _blocks(wce, fe_ctx, pk[:, :1199], eps, fill=SENT), "packet_stride")   # a plain call's check
    assert np.all(sym == SENT)
    assert np.isfinite(_blocks(wce, fe_ctx, pk, eps, (1 << 31) - 1, fill=SENT)).all()              # the largest offset
    assert np.isfinite(_blocks(wce, fe_ctx, pk, eps, -(1 << 31) + 1, fill=SENT)).all()
    for est in (True, False):
        pre, ow, cfo = refused(lambda: _preamble(wce, fe_ctx, lp, eps, est, fill=SENT, cfo_shift=4), "aligned")
        assert np.all(pre == SENT) and np.all(ow == SENT.real) and np.array_equal(cfo, eps)
        pre, ow, cfo = refused(lambda: _preamble(wce, fe_ctx, lp, eps, est, fill=SENT, lptot_len=127), "lptot_len")
        assert np.all(pre == SENT) and np.all(ow == SENT.real) and np.array_equal(cfo, eps)
    # NULL cfo in the preamble call, through the C ABI (the Python method takes None for the plain call)
    dlp = wce.DeviceArray.from_numpy(lp)
    dpre = wce.DeviceArray.from_numpy(np.full((B, PRESTRIDE), SENT, np.complex128))
    for est in (1, 0):
        rc = wce.load().wce_front_end_preamble_cfo(fe_ctx.handle, dlp.addr, LSTRIDE, L, B, dpre.addr, PRESTRIDE, None,
                                                   None, est, None)
        assert rc == EINVAL and "null cfo" in last()
    wce.synchronize()
    assert np.all(dpre.numpy() == SENT)
    # an empty batch is a no-op
    dcfo = wce.DeviceArray.from_numpy(eps)
    fe_ctx.front_end_blocks(dlp, 0, NBLK, dpre, cfo=dcfo, sample_offset=5)
    fe_ctx.front_end_preamble(dlp, 0, L, dpre, cfo=dcfo)
    wce.synchronize()
    assert np.all(dpre.numpy() == SENT) and np.array_equal(dcfo.numpy(), eps)
