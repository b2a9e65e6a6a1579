"""Packet detection and symbol timing on the GPU: wce_front_end_sync
(csrc/wce_sync.hip), the front end reading each frame at its own start
(wce_front_end_preamble_at / wce_front_end_blocks_at, front_at_kernel of
csrc/wce_front.hip), and Context.receive_capture_host on top of them.

The reference for sync is the long double model of tests/sync_model.py: start
is compared exactly (tests/test_sync_abi.py shows every data set's best lag
leads by more than 1e-9), metric within TOL_M = 1e-13 absolute (derived there).
The reference for the _at calls is the existing front end on aligned copies of
the same samples, bit for bit.

Measured on an MI355X: metric within 1.4e-15 of the long double model on every
data set (B = 777, L = 192 the largest), start equal everywhere; the recorded
packet at prefix + 32 with metric 0.7757, 0.7399 and 0.3436 as recorded, under
20 kHz and under 77 kHz; the chain's noise window 0.0658.
"""
import numpy as np
import pytest

import cfo_model as cm
import sync_model as sm
from oracle_py import N, NBLK

pytestmark = pytest.mark.gpu

EINVAL = -1
SENT_START, SENT_METRIC = -77, 123.25


@pytest.fixture(scope="module")
def fe_ctx(gpu_wce):
    return gpu_wce.Context(empty=True)


@pytest.fixture(scope="module")
def refs(golden):
    """the long double answers at threshold 0, backoff 0, computed once: name -> (cap, ltf, start, metric, d*)"""
    cache = {}

    def get(name, make):
        if name not in cache:
            cap, ltf = make()
            cap.setflags(write=False)
            cache[name] = (cap, ltf) + sm.sync(cap, ltf, 0.0)
        return cache[name]
    return get


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def _sync(wce, ctx, cap, L, ltf, threshold=0.0, backoff=0, B=None, with_metric=True):
    """one sync call on host windows [B][stride] (the first L samples of each row are the window) ->
    (start [B + 1], metric [B + 1], the capture as the device holds it afterwards); the extra slot holds a sentinel"""
    B = cap.shape[0] if B is None else B
    dcap = wce.DeviceArray.from_numpy(np.ascontiguousarray(cap, np.complex128))
    dltf = wce.DeviceArray.from_numpy(np.ascontiguousarray(ltf, np.complex128))
    dstart = wce.DeviceArray.from_numpy(np.full(B + 1, SENT_START, np.int32))
    dmetric = wce.DeviceArray.from_numpy(np.full(B + 1, SENT_METRIC, np.float64))
    ctx.front_end_sync(dcap, B, L, dltf, threshold, backoff, dstart, dmetric if with_metric else None,
                       capture_stride=cap.shape[1])
    wce.synchronize()
    return dstart.numpy(), dmetric.numpy(), dcap.numpy()


def _check_sync(got, want_start, want_metric, what):
    start, metric, _ = got
    B = len(want_start)
    err = float(np.max(np.abs(metric[:B] - want_metric)))
    print(f"\n{what}: metric within {err:.2e} of long double (TOL_M {sm.TOL_M:.0e}), "
          f"start equal: {np.array_equal(start[:B], want_start)}")
    assert np.array_equal(start[:B], want_start), what
    assert err <= sm.TOL_M, what
    assert start[B] == SENT_START and metric[B] == SENT_METRIC, what


# ---------------------------------------------------------------- 1. shapes
@pytest.mark.parametrize("B,L", sm.SHAPES)
def test_shapes(gpu_wce, fe_ctx, refs, B, L):
    cap, pos = sm.shape_set(B, L)                        # stride L + 5, sentinels in the padding
    _, ltf, start, metric, d = refs(f"shape {B} {L}", lambda: (cap[:, :L].copy(), sm.clean_ltf()))
    assert 0 in d and (B == 1 or L - 128 in d)           # peaks at lag 0 and at the last lag
    got = _sync(gpu_wce, fe_ctx, cap, L, ltf)
    _check_sync(got, start, metric, f"B={B} L={L}")
    assert np.array_equal(_bits(got[2]), _bits(cap))
    assert np.array_equal(start, d)


# ---------------------------------------------------------------- 2. the recorded packet
@pytest.mark.parametrize("prefix", [0, 37, 100])
def test_recorded_packet(gpu_wce, fe_ctx, refs, golden, prefix):
    cap, ltf, start, metric, d = refs(f"recorded {prefix}", lambda: sm.recorded(golden["matlab"], prefix))
    assert np.all(start == prefix + 32)
    got = _sync(gpu_wce, fe_ctx, cap, cap.shape[1], ltf, 0.25)
    print("\nmetric as recorded, 20 kHz, 77 kHz:", " ".join(f"{v:.4f}" for v in got[1][:3]))
    _check_sync(got, np.full(3, prefix + 32, np.int32), metric, f"recorded +{prefix}")


# ---------------------------------------------------------------- 3. loud, then quiet
def test_loud_then_quiet(gpu_wce, fe_ctx, refs):
    made = sm.loud_then_quiet()
    cap, ltf, start, metric, d = refs("loud", lambda: (made[0], sm.clean_ltf()))
    assert np.all(np.abs(d - made[1]) <= 3) and np.all(d >= 200)   # the field, behind the interferer
    _check_sync(_sync(gpu_wce, fe_ctx, cap, cap.shape[1], ltf), start, metric, "loud then quiet")


# ---------------------------------------------------------------- 4. threshold and backoff
def test_threshold_and_backoff(gpu_wce, fe_ctx, refs):
    wce = gpu_wce
    cap, ltf, start, metric, d = refs("noise", lambda: (sm.noise_only(), sm.clean_ltf()))
    assert metric.max() < 0.1
    _check_sync(_sync(wce, fe_ctx, cap, cap.shape[1], ltf, 0.2), np.full(len(cap), -1, np.int32), metric, "noise only")
    B, L = 9, 488
    cap, ltf, start, metric, d = refs(f"shape {B} {L}", lambda: (sm.shape_set(B, L)[0][:, :L].copy(), sm.clean_ltf()))
    _check_sync(_sync(wce, fe_ctx, cap, L, ltf, 0.9999), np.full(B, -1, np.int32), metric, "threshold above the peak")
    ms = np.sort(metric)
    thr = float(ms[3] + ms[4]) / 2                       # between two frames' metrics, far from both
    assert ms[4] - ms[3] > 1e-6
    _check_sync(_sync(wce, fe_ctx, cap, L, ltf, thr), np.where(metric >= thr, d, -1).astype(np.int32), metric,
                "threshold between two metrics")
    want = np.where(d >= 5, d - 5, -1).astype(np.int32)
    assert (want == -1).any() and (want >= 0).any()      # backoff larger than d*, and not
    _check_sync(_sync(wce, fe_ctx, cap, L, ltf, 0.0, 5), want, metric, "backoff 5")
    want31 = np.where(d >= 31, d - 31, -1).astype(np.int32)
    _check_sync(_sync(wce, fe_ctx, cap, L, ltf, 0.0, 31), want31, metric, "backoff 31")
    # metric == NULL: start alone
    s, mt, _ = _sync(wce, fe_ctx, cap, L, ltf, with_metric=False)
    assert np.array_equal(s[:B], start) and np.all(mt == SENT_METRIC)


# ---------------------------------------------------------------- 5. poison and batch independence
@pytest.mark.parametrize("bad", [complex(np.nan, 0.0), complex(1.0, np.inf), complex(-np.inf, np.nan)])
def test_poison_stays_in_its_frame(gpu_wce, fe_ctx, refs, bad):
    wce = gpu_wce
    B, L = 9, 488
    cap, ltf, start, metric, d = refs(f"shape {B} {L}", lambda: (sm.shape_set(B, L)[0][:, :L].copy(), sm.clean_ltf()))
    clean = _sync(wce, fe_ctx, cap, L, ltf)
    for where in (0, 300, L - 1):
        dirty = cap.copy()
        dirty[3, where] = bad
        s, mt, _ = _sync(wce, fe_ctx, dirty, L, ltf)
        assert s[3] == -1 and np.isnan(mt[3]), where
        keep = np.arange(B + 1) != 3
        assert np.array_equal(s[keep], clean[0][keep]) and np.array_equal(_bits(mt[keep]), _bits(clean[1][keep]))
    # behind the window: not part of it
    padded = np.concatenate([cap, np.full((B, 5), bad)], axis=1)
    s, mt, _ = _sync(wce, fe_ctx, padded, L, ltf)
    assert np.array_equal(s, clean[0]) and np.array_equal(_bits(mt), _bits(clean[1]))
    # a non-finite ltf marks every frame
    l2 = ltf.copy()
    l2[17] = bad
    s, mt, _ = _sync(wce, fe_ctx, cap, L, l2)
    assert np.all(s[:B] == -1) and np.isnan(mt[:B]).all() and s[B] == SENT_START and mt[B] == SENT_METRIC


def test_batch_independence(gpu_wce, fe_ctx, refs):
    wce = gpu_wce
    B, L = 777, 488
    cap, pos = sm.shape_set(B, L)
    ltf = sm.clean_ltf()
    s, mt, _ = _sync(wce, fe_ctx, cap, L, ltf)
    for f in (0, 5, 401, 776):
        s1, m1, _ = _sync(wce, fe_ctx, cap[f:f + 1], L, ltf)
        assert s1[0] == s[f] and np.array_equal(_bits(m1[0]), _bits(mt[f])), f
    s2, m2, _ = _sync(wce, fe_ctx, cap[::-1], L, ltf)    # another place in the batch
    assert np.array_equal(s2[:B][::-1], s[:B]) and np.array_equal(_bits(m2[:B][::-1]), _bits(mt[:B]))


# ---------------------------------------------------------------- 6. refused arguments
def test_errors_write_nothing(gpu_wce, fe_ctx):
    wce = gpu_wce
    lib = wce.load()
    B, L = 4, 192
    cap, _ = sm.shape_set(9, L)
    cap = cap[:B]
    stride = cap.shape[1]
    dcap = wce.DeviceArray.from_numpy(cap)
    dltf = wce.DeviceArray.from_numpy(np.concatenate([sm.clean_ltf(), [0.0]]))
    dstart = wce.DeviceArray.from_numpy(np.full(B + 1, SENT_START, np.int32))
    dmetric = wce.DeviceArray.from_numpy(np.full(B + 1, SENT_METRIC, np.float64))
    good = dict(capture=dcap.addr, stride=stride, len=L, n=B, ltf=dltf.addr, thr=0.5, backoff=0, start=dstart.addr,
                metric=dmetric.addr)

    def call(**kw):
        a = dict(good, **kw)
        return lib.wce_front_end_sync(fe_ctx.handle, a["capture"], a["stride"], a["len"], a["n"], a["ltf"], a["thr"],
                                      a["backoff"], a["start"], a["metric"], None)

    cases = [dict(len=127), dict(len=1 << 31, stride=1 << 32), dict(stride=L - 1),
             dict(thr=float("nan")), dict(thr=float("inf")), dict(thr=-1e-9), dict(thr=1.0 + 1e-9),
             dict(backoff=-1), dict(backoff=32),
             dict(start=None), dict(start=dstart.addr + 2), dict(metric=dmetric.addr + 4),
             dict(ltf=None), dict(ltf=dltf.addr + 8), dict(capture=None), dict(capture=dcap.addr + 8),
             dict(n=-1)]
    for kw in cases:
        assert call(**kw) == EINVAL, kw
        assert lib.wce_last_error().decode(), kw
    assert call(n=0) == 0 and call(n=0, thr=1.0, backoff=31, metric=None) == 0      # an empty batch: no launch
    wce.synchronize()
    assert np.all(dstart.numpy() == SENT_START) and np.all(dmetric.numpy() == SENT_METRIC)
    assert call(thr=0.0) == 0 and call(thr=1.0) == 0                                  # the ends of [0, 1]
    wce.synchronize()
    assert np.all(dstart.numpy()[:B] == -1) and dstart.numpy()[B] == SENT_START       # nothing reaches 1.0

    # the _at calls: their own refusals and those of the calls they extend
    SENT = sm.SENT
    dpre = wce.DeviceArray.from_numpy(np.full((B, 56), SENT, np.complex128))
    dsym = wce.DeviceArray.from_numpy(np.full((B, NBLK * N), SENT, np.complex128))
    dow2 = wce.DeviceArray.from_numpy(np.full(B, SENT_METRIC, np.float64))
    dcfo = wce.DeviceArray.from_numpy(np.full(B + 1, SENT_METRIC, np.float64))
    dst = wce.DeviceArray.from_numpy(np.zeros(B + 1, np.int32))
    W = 1500
    dwin = wce.DeviceArray.from_numpy(cm.random_packets(np.random.default_rng(1), B, W))
    pgood = dict(capture=dwin.addr, stride=W, len=W, n=B, start=dst.addr, pre=dpre.addr, ps=56, ow2=dow2.addr,
                 cfo=dcfo.addr, est=1)
    bgood = dict(capture=dwin.addr, stride=W, len=W, n=B, nb=NBLK, start=dst.addr, cfo=dcfo.addr, off=0, sym=dsym.addr,
                 fs=NBLK * N, bs=N)

    def pcall(**kw):
        a = dict(pgood, **kw)
        return lib.wce_front_end_preamble_at(fe_ctx.handle, a["capture"], a["stride"], a["len"], a["n"], a["start"],
                                             a["pre"], a["ps"], a["ow2"], a["cfo"], a["est"], None)

    def bcall(**kw):
        a = dict(bgood, **kw)
        return lib.wce_front_end_blocks_at(fe_ctx.handle, a["capture"], a["stride"], a["len"], a["n"], a["nb"],
                                           a["start"], a["cfo"], a["off"], a["sym"], a["fs"], a["bs"], None)

    for kw in (dict(start=None), dict(start=dst.addr + 2), dict(len=127), dict(len=1 << 31, stride=1 << 32),
               dict(stride=W - 1), dict(cfo=None, est=1), dict(cfo=dcfo.addr + 4), dict(ps=52), dict(n=-1),
               dict(capture=None), dict(pre=None)):
        assert pcall(**kw) == EINVAL, kw
        assert lib.wce_last_error().decode(), kw
    for kw in (dict(start=None), dict(start=dst.addr + 2), dict(len=127), dict(len=1 << 31, stride=1 << 32),
               dict(stride=W - 1), dict(cfo=dcfo.addr + 4), dict(off=1 << 31), dict(off=-(1 << 31)), dict(bs=52),
               dict(nb=0), dict(n=-1), dict(capture=None), dict(sym=None)):
        assert bcall(**kw) == EINVAL, kw
        assert lib.wce_last_error().decode(), kw
    assert pcall(n=0) == 0 and bcall(n=0) == 0
    wce.synchronize()
    assert np.all(dpre.numpy() == SENT) and np.all(dsym.numpy() == SENT)
    assert np.all(dow2.numpy() == SENT_METRIC) and np.all(dcfo.numpy() == SENT_METRIC)


# ---------------------------------------------------------------- 7. the front end at a per-frame start
AT_B, AT_W, AT_PRE = 777, 1700, 56
AT_SPECIAL = (5, 300, 776)      # start -1, one sample over the window's end, exactly fitting


class AtData:
    def __init__(self):
        rng = np.random.default_rng(0x5C70)
        self.cap = cm.random_packets(rng, AT_B, AT_W + 5)
        self.cap[:, AT_W:] = np.nan                      # whoever reads past a window gets NaN
        self.eps = cm.draw_eps(rng, AT_B)
        self.start = rng.integers(0, AT_W - 128 - 160 - NBLK * 80 + 1, AT_B).astype(np.int32)

    def starts(self, fit):
        """the common starts with the three special frames set; fit = the largest start that fits the call"""
        s = self.start.copy()
        s[AT_SPECIAL[0]], s[AT_SPECIAL[1]], s[AT_SPECIAL[2]] = -1, fit + 1, fit
        return s

    def aligned(self, s, first, count):
        """[B][count] copies of cap[f, s[f] + first : ...]; frames that do not fit get zeros"""
        out = np.zeros((AT_B, count), np.complex128)
        for f in range(AT_B):
            a = int(s[f]) + first
            if s[f] >= 0 and a >= 0 and a + count <= AT_W:
                out[f] = self.cap[f, a:a + count]
        return out


@pytest.fixture(scope="module")
def at():
    return AtData()


def _pre_call(wce, ctx, data, B, L, stride, cfo, est, start=None):
    dl = wce.DeviceArray.from_numpy(data)
    dpre = wce.DeviceArray.from_numpy(np.full((B, AT_PRE), sm.SENT, np.complex128))
    dow2 = wce.DeviceArray.from_numpy(np.full(B, SENT_METRIC, np.float64))
    dcfo = None if cfo is None else wce.DeviceArray.from_numpy(np.asarray(cfo, np.float64))
    dst = None if start is None else wce.DeviceArray.from_numpy(start)
    ctx.front_end_preamble(dl, B, L, dpre, dow2, lptot_stride=stride, pre_stride=AT_PRE, cfo=dcfo, estimate_cfo=est,
                           start=dst, capture_len=None if start is None else L)
    wce.synchronize()
    return dpre.numpy(), dow2.numpy(), None if dcfo is None else dcfo.numpy()


@pytest.mark.parametrize("mode", ["given", "estimated", "null"])
def test_preamble_at_is_the_aligned_call(gpu_wce, fe_ctx, at, mode):
    wce = gpu_wce
    s = at.starts(AT_W - 128)
    cfo = None if mode == "null" else (at.eps if mode == "given" else np.full(AT_B, 9.0))
    est = mode == "estimated"
    pre, ow2, e = _pre_call(wce, fe_ctx, at.cap, AT_B, AT_W, AT_W + 5, cfo, est, s)
    rpre, row2, re_ = _pre_call(wce, fe_ctx, at.aligned(s, 0, 128), AT_B, 128, 128, cfo, est)
    nan = np.zeros(AT_B, bool)
    nan[list(AT_SPECIAL[:2])] = True
    for f in np.flatnonzero(nan):
        assert np.isnan(pre[f, :N].view(np.float64)).all() and np.isnan(ow2[f]), (mode, f)
        assert np.all(pre[f, N:] == sm.SENT)
        if est:
            assert np.isnan(e[f])
        elif e is not None:
            assert e[f] == at.eps[f]
    ok = ~nan
    assert np.isfinite(pre[AT_SPECIAL[2], :N]).all() and np.isfinite(ow2[AT_SPECIAL[2]])
    assert np.array_equal(_bits(pre[ok]), _bits(rpre[ok])), mode
    assert np.array_equal(_bits(ow2[ok]), _bits(row2[ok])), mode
    if e is not None:
        assert np.array_equal(_bits(e[ok]), _bits(re_[ok])), mode
        assert est or np.array_equal(e, at.eps)


def _blk_call(wce, ctx, data, B, stride, cfo, off, start=None, L=None):
    dp = wce.DeviceArray.from_numpy(data)
    dsym = wce.DeviceArray.from_numpy(np.full((B, NBLK * 64 + 3), sm.SENT, np.complex128))
    dcfo = None if cfo is None else wce.DeviceArray.from_numpy(np.asarray(cfo, np.float64))
    dst = None if start is None else wce.DeviceArray.from_numpy(start)
    ctx.front_end_blocks(dp, B, NBLK, dsym, packet_stride=stride, frame_stride=NBLK * 64 + 3, block_stride=60, cfo=dcfo,
                         sample_offset=off, start=dst, capture_len=L)
    wce.synchronize()
    return dsym.numpy()


@pytest.mark.parametrize("off", [0, 160])
@pytest.mark.parametrize("mode", ["given", "null"])
def test_blocks_at_is_the_aligned_call(gpu_wce, fe_ctx, at, mode, off):
    wce = gpu_wce
    s = at.starts(AT_W - 128 - off - NBLK * 80)
    cfo = None if mode == "null" else at.eps
    sym = _blk_call(wce, fe_ctx, at.cap, AT_B, AT_W + 5, cfo, off, s, AT_W)
    ref = _blk_call(wce, fe_ctx, at.aligned(s, 128 + off, NBLK * 80), AT_B, NBLK * 80, cfo, off)
    bins = np.zeros(NBLK * 64 + 3, bool)
    for b in range(NBLK):
        bins[b * 60:b * 60 + N] = True
    nan = np.zeros(AT_B, bool)
    nan[list(AT_SPECIAL[:2])] = True
    for f in np.flatnonzero(nan):
        assert np.isnan(sym[f, bins].view(np.float64)).all(), (mode, off, f)
        assert np.all(sym[f, ~bins] == sm.SENT)
    assert np.isfinite(sym[AT_SPECIAL[2], bins]).all()
    assert np.array_equal(_bits(sym[~nan]), _bits(ref[~nan])), (mode, off)


def test_blocks_at_after_an_estimate(gpu_wce, fe_ctx, at):
    """the estimated offsets of preamble_at feed blocks_at as preamble_cfo's feed blocks_cfo"""
    wce = gpu_wce
    s = at.starts(AT_W - 128 - NBLK * 80)
    _, _, e = _pre_call(wce, fe_ctx, at.cap, AT_B, AT_W, AT_W + 5, np.full(AT_B, 9.0), True, s)
    _, _, re_ = _pre_call(wce, fe_ctx, at.aligned(s, 0, 128), AT_B, 128, 128, np.full(AT_B, 9.0), True)
    sym = _blk_call(wce, fe_ctx, at.cap, AT_B, AT_W + 5, e, 0, s, AT_W)
    ref = _blk_call(wce, fe_ctx, at.aligned(s, 128, NBLK * 80), AT_B, NBLK * 80, re_, 0)
    nan = np.zeros(AT_B, bool)
    nan[list(AT_SPECIAL[:2])] = True
    assert np.isnan(e[AT_SPECIAL[0]]) and np.isnan(sym[nan][:, :N].view(np.float64)).all()
    assert np.array_equal(_bits(sym[~nan]), _bits(ref[~nan]))


# ---------------------------------------------------------------- 8. the chain
def test_receive_capture_chain(gpu_wce, golden):
    wce, m = gpu_wce, golden["matlab"]
    cap, ltf = sm.chain(m)
    B, P = len(cap), sm.CHAIN_PREFIX
    assert np.array_equal(ltf, m["tx_lptot"][-64:])
    ctx = wce.Context(m["tx_preamble_fft"], m["rx_preamble_fft"], 9.6172e-8, wce.MMSE_TEXTBOOK)
    tx_pk, tx_lp = np.repeat(m["tx_packet"][None], B, 0), np.repeat(m["tx_lptot"][None], B, 0)
    out = ctx.receive_capture_host(tx_pk, tx_lp, cap, 0.25, mask=wce.ALL, semantics=wce.SEM_MATLAB, cfo=True)
    s_ref, m_ref, _ = sm.sync(cap, ltf, 0.25)
    print("\nstart", out["start"], "metric", " ".join(f"{v:.4f}" for v in out["metric"]))
    assert np.array_equal(out["start"], s_ref) and np.max(np.abs(out["metric"] - m_ref)) <= sm.TOL_M
    det = np.arange(B) != sm.CHAIN_NOISE
    assert np.all(out["start"][det] == P + 32) and out["start"][sm.CHAIN_NOISE] == -1
    # the aligned inputs of the detected frames through the existing chain
    ref = ctx.receive_host(tx_pk[det], tx_lp[det], cap[det][:, P + 160:], cap[det][:, P:P + 160], mask=wce.ALL,
                           semantics=wce.SEM_MATLAB, cfo=True)
    assert set(out) == set(ref) | {"start", "metric"}
    for k in ref:
        assert np.array_equal(_bits(out[k][det]), _bits(ref[k])), k
    assert abs(out["cfo"][1] - out["cfo"][0] - 0.002) < 1e-15
    # the window without a packet: a NaN row, which the scan finds
    f = sm.CHAIN_NOISE
    assert np.isnan(out["ps_mmse"][f].view(np.float64)).all() and np.isnan(out["ow2"][f]) and np.isnan(out["cfo"][f])
    bits, count = ctx.nonfinite_scan(wce.DeviceArray.from_numpy(out["ps_mmse"]), B)
    assert count == 1 and bits.tolist() == [1 << f]
