"""Receive diversity on the device: wce_combine against the long double model with the
derived tolerances of tests/combine_model.py (test_combine_abi.py derives them), in
every layout and output set and under the frame loop; the live-branch rule, bit for
bit; 64-bit offsets; wce_sync_share against its model and on real captures; and the
link experiment Context.link_mrc_host against the fp64 model chain on its own captures.

All of them fail on a library without the two symbols.

The link experiment (16-QAM rate 1/2, nominal 10 dB, 67 packets, six static taps per
branch, LT_LS, combine_model.LINK_SEED = 0x4007), bit errors in 96,480 of the combined
chain / of each branch alone, measured on an MI355X (profiles/combine_65536.txt); the
fp64 model on the device's captures gives the same counts frame by frame with no frame
marginal, and so it does on the model transmitter's own captures
(tests/test_combine_abi.py):
    2 equal branches              0 / 771, 954
    2 branches, 6 dB apart        weighted 276, unweighted 2657 / 1034, 43189
    4 equal branches              0 / 1598, 1635, 1204, 1539
    4 branches, 6 dB steps        weighted 184, unweighted 47928 / 1141, 43158, 47949, 47761
wce_combine against long double on the parity sets: 3.6 to 7.5 u of the bound for rx_c
(TOL_RX is 46 u) and 1.7 to 3.1 u of g for h_c (TOL_H is 20 u), u = 2^-53."""
import contextlib

import numpy as np
import pytest

import combine_model as cb
import demod_model as dm
import fec_model as fm
import tx_model as tm

pytestmark = pytest.mark.gpu

N, NBLK, DC = dm.N, dm.NBLK, dm.DC
B = cb.PARITY_B
SENT = complex(7.0, -3.0)


@pytest.fixture(scope="module")
def ctx(gpu_wce):
    pre = tm.chain_pre()
    c = gpu_wce.Context(pre, pre, 1e-6, gpu_wce.MMSE_TEXTBOOK)
    yield c
    c.close()


@contextlib.contextmanager
def grid_knob(wce, on):
    lib = wce.load()
    try:
        assert lib.wce_debug_set_variant(6, 1 if on else 0) == 0      # WCE_VARIANT_GRID: three workgroups
        yield
    finally:
        assert lib.wce_debug_set_variant(6, 0) == 0


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


# ---------------------------------------------------------------- layouts
class Layout:
    """element offsets of a branch layout with padding everywhere: rows of 53 in strides that are no multiple of
    anything, so that a wrong stride lands on a sentinel"""

    def __init__(self, A, n, minor):
        self.A, self.n, self.minor = A, n, minor
        if minor:      # the branches of a block next to each other; the branches' h rows of a packet likewise
            self.rbs, self.rks = 55, A * 55 + 3
            self.rfs = NBLK * self.rks + 5
            self.hbs, self.hs = 54, A * 54 + 1
            self.rx_size = n * self.rfs + 9
            self.h_size = n * self.hs + 9
        else:          # branch-major
            self.rks, self.rfs = 55, NBLK * 55 + 7
            self.rbs = n * self.rfs + 11
            self.hs = 57
            self.hbs = n * self.hs + 3
            self.rx_size = A * self.rbs + 9
            self.h_size = A * self.hbs + 9
        self.obs = n + 3
        a, f, b, k = np.arange(A), np.arange(n), np.arange(NBLK), np.arange(N)
        self.rx_idx = (a[:, None, None, None] * self.rbs + f[None, :, None, None] * self.rfs +
                       b[None, None, :, None] * self.rks + k[None, None, None, :])
        self.h_idx = a[:, None, None] * self.hbs + f[None, :, None] * self.hs + k[None, None, :]
        self.o_idx = a[:, None] * self.obs + f[None, :]
        # the outputs: padded too
        self.oks, self.ofs, self.ohs = 56, NBLK * 56 + 2, 59
        self.orx_idx = f[:, None, None] * self.ofs + b[None, :, None] * self.oks + k[None, None, :]
        self.oh_idx = f[:, None] * self.ohs + k[None, :]
        assert len(np.unique(self.rx_idx)) == self.rx_idx.size and self.rx_idx.max() < self.rx_size
        assert len(np.unique(self.h_idx)) == self.h_idx.size and self.h_idx.max() < self.h_size

    def run(self, wce, ctx, rx, h, ow2, want_rx=True, want_h=True):
        """-> (rx_c [n][15][53] or None, h_c [n][53] or None); asserts that nothing outside the rows was written"""
        A, n = self.A, self.n
        frx = np.full(self.rx_size, SENT, np.complex128)
        frx[self.rx_idx] = rx
        fh = np.full(self.h_size, SENT, np.complex128)
        fh[self.h_idx] = h
        D = wce.DeviceArray.from_numpy
        drx, dh, dow2 = D(frx), D(fh), None
        if ow2 is not None:
            fo = np.full(A * self.obs, -5.0)
            fo[self.o_idx] = ow2
            dow2 = D(fo)
        orx_host = np.full(n * self.ofs + 13, SENT, np.complex128)
        oh_host = np.full(n * self.ohs + 13, SENT, np.complex128)
        dorx = D(orx_host) if want_rx else None
        doh = D(oh_host) if want_h else None
        ctx.combine(drx, dh, n, A, dow2, dorx, doh, rx_branch_stride=self.rbs, rx_frame_stride=self.rfs,
                    rx_block_stride=self.rks, h_branch_stride=self.hbs, h_stride=self.hs, ow2_branch_stride=self.obs,
                    out_frame_stride=self.ofs, out_block_stride=self.oks, out_h_stride=self.ohs)
        wce.synchronize()
        assert same_bits(drx.numpy(), frx) and same_bits(dh.numpy(), fh)          # the inputs are read only
        out = []
        for d, idx, host in ((dorx, self.orx_idx, orx_host), (doh, self.oh_idx, oh_host)):
            if d is None:
                out.append(None)
                continue
            got = d.numpy()
            rest = np.ones(got.size, bool)
            rest[idx.reshape(-1)] = False
            assert np.all(got[rest] == SENT), "written outside the rows"
            out.append(got[idx])
        return out[0], out[1]


def check_parity(got_rx, got_h, ref, tol_rx, tol_h):
    ok = ref["bound"] > 0
    if got_rx is not None:
        assert np.all(got_rx[~ok] == 0)                                  # entry 26
        err = np.abs(np.asarray(got_rx, np.clongdouble) - ref["rx"])[ok] / ref["bound"][ok]
        assert float(err.max()) <= tol_rx, float(err.max())
    if got_h is not None:
        okh = ref["g"] > 0
        assert np.all(got_h[~okh] == 0) and np.all(got_h.imag == 0)
        err = np.abs(np.asarray(got_h, np.clongdouble) - ref["h"])[okh] / ref["g"][okh]
        assert float(err.max()) <= tol_h, float(err.max())


# ---------------------------------------------------------------- 1. parity
@pytest.mark.parametrize("weighted", (False, True))
@pytest.mark.parametrize("A", cb.PARITY_A)
def test_parity(gpu_wce, ctx, A, weighted):
    """67 packets (odd, and more workgroups than the knob's 3: the frame loop runs, its last trip ragged) against the
    long double model; both layouts; each output alone gives the bits of both together; knob 0 and 1 agree"""
    wce = gpu_wce
    tx, rx, h, ow2 = cb.parity_set(A)
    ref = cb.parity_model(A, weighted)
    tol_rx, tol_h = cb.tolerances()
    o = ow2 if weighted else None
    first = None
    for minor in (False, True):
        lay = Layout(A, B, minor)
        with grid_knob(wce, True):
            grx, gh = lay.run(wce, ctx, rx, h, o)
            only_rx, none = lay.run(wce, ctx, rx, h, o, want_h=False)
            none2, only_h = lay.run(wce, ctx, rx, h, o, want_rx=False)
        assert none is None and none2 is None
        check_parity(grx, gh, ref, tol_rx, tol_h)
        assert same_bits(only_rx, grx) and same_bits(only_h, gh), "an output alone differs from both together"
        with grid_knob(wce, False):
            prx, ph = lay.run(wce, ctx, rx, h, o)
        assert same_bits(prx, grx) and same_bits(ph, gh), "the grid knob changes bits"
        if first is None:
            first = (grx, gh)
        assert same_bits(grx, first[0]) and same_bits(gh, first[1]), "the layout changes bits"
    worst = cb.gaps({"rx": first[0], "h": first[1]}, ref)
    print(f"\nA = {A}, ow2 {weighted}: rx {worst[0]:.2e} of the bound (tolerance {tol_rx:.2e}), "
          f"h {worst[1]:.2e} of g (tolerance {tol_h:.2e})")
    # the convenience call on dense arrays is the same call
    d = ctx.combine_host(rx, h, o)
    assert same_bits(d["rx"], first[0]) and same_bits(d["h"], first[1])


# ---------------------------------------------------------------- 2. the guards
def test_guards(gpu_wce, ctx):
    wce = gpu_wce
    tx, rx, h, ow2 = (np.array(a) for a in cb.parity_set(3))
    clean = ctx.combine_host(rx, h, ow2)
    h[1, 4, 17] = np.nan                    # a NaN in an h row
    h[2, 5, DC] = np.inf                    # entry 26 is outside V: the branch stays live
    h[1, 12] = complex(np.nan, np.nan)      # a NaN row, as the _at calls leave one
    ow2[0, 6], ow2[1, 7], ow2[2, 8], ow2[0, 9] = 0.0, -1.0, np.inf, np.nan
    h[:, 10, 3] = np.nan                    # no live branch
    rx[1, 11, 2, 40] = np.nan               # a NaN sample of a live branch
    rx[1, 4] = complex(np.nan, np.inf)      # what a dead branch holds is never looked at
    with grid_knob(wce, True):
        got = ctx.combine_host(rx, h, ow2)
    model = cb.combine(rx, h, ow2, np.float64)
    # a dead branch: the call without it, bit for bit
    for f, gone in ((4, 1), (12, 1), (6, 0), (7, 1), (8, 2), (9, 0)):
        keep = [a for a in range(3) if a != gone]
        assert not model["live"][gone, f] and model["live"][keep, f].all()
        alone = ctx.combine_host(rx[keep][:, f:f + 1], h[keep][:, f:f + 1], ow2[keep][:, f:f + 1])
        assert same_bits(got["rx"][f], alone["rx"][0]) and same_bits(got["h"][f], alone["h"][0]), f
        assert np.isfinite(got["rx"][f]).all()
    # none live: NaN rows
    assert np.isnan(got["rx"][10].real).all() and np.isnan(got["rx"][10].imag).all()
    assert np.isnan(got["h"][10].real).all() and np.isnan(got["h"][10].imag).all()
    # a NaN sample reaches exactly one entry
    bad = ~np.isfinite(got["rx"])
    assert int(bad.sum()) == NBLK * N + 1 and bad[11, 2, 40]
    assert np.isfinite(np.delete(got["h"], 10, axis=0)).all()
    # no other packet changes by a bit, nor the rest of packet 11; packet 5 ignores its entry 26
    same = [f for f in range(B) if f not in (4, 6, 7, 8, 9, 10, 11, 12)]
    assert same_bits(got["rx"][same], clean["rx"][same]) and same_bits(got["h"][same], clean["h"][same])
    assert same_bits(np.delete(got["rx"][11], 40, axis=1), np.delete(clean["rx"][11], 40, axis=1))
    assert same_bits(got["h"][11], clean["h"][11])
    # without ow2 the same h rows decide alone
    flat = ctx.combine_host(rx, h, None)
    for f, gone in ((4, 1), (12, 1)):
        keep = [a for a in range(3) if a != gone]
        alone = ctx.combine_host(rx[keep][:, f:f + 1], h[keep][:, f:f + 1])
        assert same_bits(flat["rx"][f], alone["rx"][0]) and same_bits(flat["h"][f], alone["h"][0]), f
    assert np.isfinite(flat["rx"][[6, 7, 8, 9]]).all()
    # a zero gain is 0, not NaN
    h0 = np.array(cb.parity_set(2)[2])
    h0[:, 3, 9] = 0
    z = ctx.combine_host(cb.parity_set(2)[1], h0)
    assert np.all(z["rx"][3, :, 9] == 0) and z["h"][3, 9] == 0 and np.isfinite(z["rx"]).all()


@pytest.mark.parametrize("A", (2, 8))
def test_batch_independence(gpu_wce, ctx, A):
    tx, rx, h, ow2 = cb.parity_set(A)
    with grid_knob(gpu_wce, True):
        full = ctx.combine_host(rx, h, ow2)
    for p in (0, 1, 33, 66):
        alone = ctx.combine_host(rx[:, p:p + 1], h[:, p:p + 1], ow2[:, p:p + 1])
        assert same_bits(alone["rx"][0], full["rx"][p]) and same_bits(alone["h"][0], full["h"][p]), p


# ---------------------------------------------------------------- 3. 64-bit offsets
def test_big_branch_stride(gpu_wce, ctx):
    """A = 2, 5 packets, branch 1 of rx 2^31 + 64 elements behind branch 0 (one 34 GB allocation, touched at both
    ends only), and the outputs behind it: the dense run's bits"""
    wce = gpu_wce
    lib = wce.load()
    n, S = 5, 2 ** 31 + 64
    tx, rx, h, ow2 = (np.ascontiguousarray(a[:, :n]) for a in cb.parity_set(2))
    want = ctx.combine_host(rx, h, ow2)
    row = n * NBLK * N
    try:
        big = wce.DeviceArray((S + row,), np.complex128)
    except wce.WceError as e:
        pytest.skip(f"no room for a 34 GB buffer on this device: {e}")
    try:
        D = wce.DeviceArray.from_numpy
        drx, dh, dow2 = D(rx), D(h), D(ow2)
        for a in range(2):
            assert lib.wce_memcpy_dtod(big.addr + a * S * 16, drx.addr + a * row * 16, row * 16, None) == 0
        orx, oh = wce.DeviceArray((n, NBLK, N), zero=True), wce.DeviceArray((n, N), zero=True)
        ctx.combine(big, dh, n, 2, dow2, orx, oh, rx_branch_stride=S)
        wce.synchronize()
        assert same_bits(orx.numpy(), want["rx"]) and same_bits(oh.numpy(), want["h"])
        assert np.any(want["rx"] != 0)
    finally:
        wce.synchronize()
        big.free()


# ---------------------------------------------------------------- 4. wce_sync_share
@pytest.mark.parametrize("A", (1, 2, 4, 8))
def test_sync_share_parity(gpu_wce, ctx, A):
    wce = gpu_wce
    D = wce.DeviceArray.from_numpy
    metric, start, cfo = cb.sync_share_set(A)
    P, bs = metric.shape[1], metric.shape[1] + 5
    pad = lambda a, fill: np.concatenate([a, np.full((A, bs - P), fill, a.dtype)], axis=1)
    want_s, want_c = cb.sync_share(metric, start, cfo)
    for knob in (True, False):
        for use_s, use_c in ((True, True), (True, False), (False, True)):
            ds, dc, dm_ = D(pad(start, -77)), D(pad(cfo, 9.0)), D(pad(metric, 2.0))
            with grid_knob(wce, knob):
                ctx.sync_share(dm_, P, A, ds if use_s else None, dc if use_c else None, branch_stride=bs)
            wce.synchronize()
            s, c = ds.numpy().reshape(A, bs), dc.numpy().reshape(A, bs)
            assert np.all(s[:, P:] == -77) and np.all(c[:, P:] == 9.0) and same_bits(dm_.numpy().reshape(A, bs), pad(metric, 2.0))
            ws, wc = cb.sync_share(metric, start if use_s else None, cfo if use_c else None)
            assert np.array_equal(s[:, :P], ws if use_s else start), (knob, use_s, use_c)
            assert same_bits(c[:, :P], wc if use_c else cfo), (knob, use_s, use_c)
    assert np.all(want_s[:, 3] == 10) and np.all(want_s[:, 7] == -1)
    assert np.any(want_s != start) or A == 1


def test_sync_share_rescues_a_faded_branch(gpu_wce, ctx):
    """two antennas, branch 1 attenuated by 40 dB under the same noise: its own front_end_sync misses at the test's
    threshold; with branch 0's start the _at call gives it a finite row"""
    wce = gpu_wce
    D, Z = wce.DeviceArray.from_numpy, lambda shape, dt=np.complex128: wce.DeviceArray(shape, dt, zero=True)
    n, L, thr = 5, 1488, 0.25
    mod, rate = dm.QAM16, fm.RATE_1_2
    rng = np.random.default_rng(0x5A4E)
    pre = tm.chain_pre()
    sym = fm.transmit(fm.random_info(rng, n, mod, rate), mod, rate)[0]
    taps = tm.random_taps(rng, n, 6)
    delay = np.array([0, 37, 100, 64, 11], np.int32)
    ow2 = float(tm.nominal_ow2(30.0))
    cap = np.concatenate([ctx.transmit_host(sym, pre, t, 0.001, ow2, delay, L, seed=0x5A4E, first_frame=a * n)
                          for a, t in enumerate((taps, 0.01 * taps))])
    dcap, dltf = D(cap), D(np.asarray(tm.idft64(pre), np.complex128))
    ds, dm_, dcfo = Z((2 * n,), np.int32), Z((2 * n,), np.float64), Z((2 * n,), np.float64)
    ctx.front_end_sync(dcap, 2 * n, L, dltf, thr, 0, ds, dm_)
    wce.synchronize()
    start, metric = ds.numpy().reshape(2, n), dm_.numpy().reshape(2, n)
    assert np.all(start[0] >= 0) and np.all(start[1] == -1) and np.all(metric[1] < thr) and np.all(metric[0] >= thr)

    def rows():
        dpre, dow2 = Z((2 * n, N)), Z((2 * n,), np.float64)
        ctx.front_end_preamble(dcap, 2 * n, L, dpre, dow2, cfo=dcfo, start=ds)
        wce.synchronize()
        return dpre.numpy().reshape(2, n, N)
    before = rows()
    assert np.isnan(before[1].real).all() and np.isfinite(before[0]).all()
    ctx.sync_share(dm_, n, 2, ds, None)
    wce.synchronize()
    shared = ds.numpy().reshape(2, n)
    assert np.array_equal(shared[0], start[0]) and np.array_equal(shared[1], start[0])
    after = rows()
    assert np.isfinite(after[1]).all() and same_bits(after[0], before[0])
    # the offsets, shared without the start: every branch has a finite metric, the larger one's offset wins
    own = dcfo.numpy().reshape(2, n)
    ctx.sync_share(dm_, n, 2, None, dcfo)
    wce.synchronize()
    assert same_bits(dcfo.numpy().reshape(2, n), np.stack([own[0], own[0]]))


# ---------------------------------------------------------------- 5. the link experiment
_FRONTS = {}


def _link(wce, ctx, A, unequal, weighted):
    c = cb.link_set(A, unequal)
    res = ctx.link_mrc_host(cb.LINK_MOD, cb.LINK_RATE, cb.LINK_SNR, cb.LINK_B, A, c["taps"], sources=(wce.LT_LS,),
                            branch_loss_db=c["loss"], weighted=weighted, cfo=c["cfo"], delay=c["delay"],
                            capture_len=cb.LINK_LEN, threshold=cb.LINK_THRESHOLD, seed=c["seed"], keep_capture=True)
    assert np.array_equal(res["bits"], c["bits"]) and np.allclose(res["ow2"], c["ow2"][:, None], rtol=1e-12)
    key = (A, unequal)
    if key not in _FRONTS:
        _FRONTS[key] = (res["capture"], cb.link_front(res["capture"]))
    cap, front = _FRONTS[key]
    assert same_bits(res["capture"], cap)                     # the same seed: the same captures, weighted or not
    model = cb.link_model(cap, c["bits"], weighted, front=front)
    return res, model


@pytest.mark.parametrize("A,unequal", ((2, False), (2, True), (4, False), (4, True)))
def test_link_mrc(gpu_wce, ctx, A, unequal):
    """67 packets of 16-QAM rate 1/2 through six taps per branch at nominal 10 dB (each next branch 6 dB noisier
    with `unequal`): the combined chain beats the best branch, the noise weights beat none, and every count is the
    fp64 model's on the same captures, frame by frame, but for the frames the model itself marks marginal (at most
    2; combine_model.LINK_SEED leaves none on the model transmitter's captures)."""
    wce = gpu_wce
    totals = {}
    for weighted in ((True, False) if unequal else (True,)):
        res, model = _link(wce, ctx, A, unequal, weighted)
        r = res[wce.LT_LS]
        assert r["combined"].shape == (cb.LINK_B,) and r["branch"].shape == (A, cb.LINK_B)
        assert r["combined"].dtype == np.uint32 and r["branch"].dtype == np.uint32
        assert np.array_equal(res["start"], model["start"]) and np.all(res["start"] >= 0)
        assert np.all(res["start"] == res["start"][0])        # shared
        comb, branch = int(r["combined"].sum()), [int(x) for x in r["branch"].sum(axis=1)]
        out = model["marginal"] | model["branch_marginal"].any(axis=0)
        print(f"\nA = {A}, unequal {unequal}, weighted {weighted}: device combined {comb}, branches {branch}; model "
              f"combined {int(model['combined'].sum())}, branches {[int(x) for x in model['branch'].sum(axis=1)]}; "
              f"{int(out.sum())} marginal frames left out")
        assert int(out.sum()) <= 2
        assert np.array_equal(r["combined"][~out], model["combined"][~out])
        assert np.array_equal(r["branch"][:, ~out], model["branch"][:, ~out])
        if weighted:
            assert comb < min(branch)
        totals[weighted] = comb
    if unequal:
        assert totals[True] < totals[False]


def test_one_antenna_is_link_host(gpu_wce, ctx):
    wce = gpu_wce
    n = 16
    rng = np.random.default_rng(0x3C01)
    taps = tm.random_taps(rng, n, 6)
    kw = dict(cfo=rng.uniform(-0.002, 0.002, n), delay=rng.integers(0, 100, n).astype(np.int32), seed=0x3C01,
              threshold=cb.LINK_THRESHOLD)
    want = ctx.link_host(cb.LINK_MOD, cb.LINK_RATE, cb.LINK_SNR, n, taps=taps, **kw)
    got = ctx.link_mrc_host(cb.LINK_MOD, cb.LINK_RATE, cb.LINK_SNR, n, 1, taps[None], weighted=False, **kw)
    assert sum(int(want[s].sum()) for s in (wce.LT_LS, wce.PS_LINEAR, wce.PS_MMSE)) > 0
    for s in (wce.LT_LS, wce.PS_LINEAR, wce.PS_MMSE):
        assert np.array_equal(got[s]["branch"][0], want[s]), s
    # one branch combined is that branch equalized by itself: LT_LS, which link_host does not blend, decodes alike
    assert np.array_equal(got[wce.LT_LS]["combined"], want[wce.LT_LS])
    for k in ("start", "metric", "cfo"):
        assert same_bits(got[k][0], want[k]), k
    assert np.array_equal(got["bits"], want["bits"])


def test_link_mrc_options(gpu_wce, ctx):
    """the other paths of link_mrc_host on two antennas: a short field in front (front_end_sync_stf, start and
    offset shared in one call), taps that fade within the packet with the tracker on the combined stream, and a
    decision-directed round; without sharing every branch keeps its own start"""
    wce = gpu_wce
    n, A = cb.LINK_B, 2
    rng = np.random.default_rng(0x3C02)
    power = np.exp(-0.5 * np.arange(6)) ** 2
    fading = np.stack([wce.fading_taps(rng, n, power, 0.995, 19) for _ in range(A)])      # [A][B][19][6]
    kw = dict(sources=(wce.LT_LS,), cfo=rng.uniform(-0.002, 0.002, n), delay=rng.integers(0, 100, n).astype(np.int32),
              seed=0x3C02, threshold=cb.LINK_THRESHOLD)
    t = ctx.link_mrc_host(cb.LINK_MOD, cb.LINK_RATE, 22.0, n, A, fading, tracker=(0.5, 2), **kw)
    s, tr = t[wce.LT_LS], t["tracked"][wce.LT_LS]
    print(f"\nfading, rho 0.995, 22 dB: static combined {int(s['combined'].sum())} branches "
          f"{[int(x) for x in s['branch'].sum(axis=1)]}; tracked combined {int(tr['combined'].sum())} branches "
          f"{[int(x) for x in tr['branch'].sum(axis=1)]}")
    assert tr["combined"].shape == (n,) and tr["branch"].shape == (A, n)
    assert s["combined"].sum() < s["branch"].sum(axis=1).min()
    assert tr["combined"].sum() < tr["branch"].sum(axis=1).min()
    assert tr["combined"].sum() < s["combined"].sum()                 # the tracker composes with the combiner
    static = fading[:, :, 0]
    d = ctx.link_mrc_host(cb.LINK_MOD, cb.LINK_RATE, cb.LINK_SNR, n, A, static, dd_iterations=1, **kw)
    p = ctx.link_mrc_host(cb.LINK_MOD, cb.LINK_RATE, cb.LINK_SNR, n, A, static, **kw)
    print(f"static taps, {cb.LINK_SNR} dB: combined {int(p[wce.LT_LS]['combined'].sum())}, after one decision-directed "
          f"round {int(d[wce.LT_LS]['combined'].sum())}; branches {[int(x) for x in p[wce.LT_LS]['branch'].sum(axis=1)]} "
          f"and {[int(x) for x in d[wce.LT_LS]['branch'].sum(axis=1)]}")
    for r in (p, d):
        assert r[wce.LT_LS]["combined"].sum() < r[wce.LT_LS]["branch"].sum(axis=1).min()
    assert not same_bits(d[wce.LT_LS]["branch"], p[wce.LT_LS]["branch"])      # the round ran
    f = ctx.link_mrc_host(cb.LINK_MOD, cb.LINK_RATE, cb.LINK_SNR, n, A, static, stf=True, capture_len=1648,
                          **{**kw, "cfo": rng.uniform(-0.02, 0.02, n)})
    assert f["metric_stf"].shape == (A, n) and np.all(f["start"] >= 0) and np.all(f["start"][0] == f["start"][1])
    assert same_bits(f["cfo"][0], f["cfo"][1])
    assert f[wce.LT_LS]["combined"].sum() < f[wce.LT_LS]["branch"].sum(axis=1).min()
    own = ctx.link_mrc_host(cb.LINK_MOD, cb.LINK_RATE, cb.LINK_SNR, n, A, static, share_sync=False, **kw)
    assert not same_bits(own["cfo"][0], own["cfo"][1]) and same_bits(p["cfo"][0], p["cfo"][1])
    # what sharing is worth: offsets estimated per branch at 10 dB differ by about 1e-4 cycles per sample, so the
    # branches' phases drift apart over the packet and one common pilot phase cannot follow both (measured: 4,112
    # bit errors combined against 2,836 and 2,919 alone, and 0 with the shared offset)
    print(f"own start and offset per branch: combined {int(own[wce.LT_LS]['combined'].sum())}, branches "
          f"{[int(x) for x in own[wce.LT_LS]['branch'].sum(axis=1)]}")
    assert p[wce.LT_LS]["combined"].sum() < own[wce.LT_LS]["combined"].sum()
