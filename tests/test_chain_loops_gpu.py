"""The frame loops of the receive and transmit chain on the device, at sizes where every wave takes
several trips round its loop.

At the batches the kernels' own test files use (1, 5, 67, 777) a launcher's own grid cap is never
reached: no wave loads a second frame, so a missing reset, a prefetch from the wrong frame or a dropped
trailing LDS sync would pass them all.  WCE_VARIANT_GRID (wce_debug_set_variant(6, 1), csrc/wce_internal.h
chain_grid, tests/test_chain_grid.py) caps the looping launchers at 3 workgroups: a sweep is then 12
frames for the kernels with four waves per workgroup (96 units of the front end, 3 frames of the
transmitter), so B = 67 makes five full sweeps and a ragged one of 7, and B = 13 a second trip of one
wave.

Every call runs twice from the same sentinel-filled contents of the same padded device buffers, knob 0
then knob 1.  A frame's outputs depend on its own data alone, so every output byte, padding included,
must be the same; and knob 1's result must still meet the bound of the kernel's own test file against
that file's model.  Frames are arranged so that what one frame could leave behind (NaN flags, a strong
metric, rows in LDS, path metrics, a rotor) would show in the frame the same wave takes next.

Shown by mutation on an MI355X, in a scratch build that was never committed: without the `bq = -1.0`
reset behind a frame of sync_kernel, knob 0 still gives the model's answers and test_sync fails at all
three window lengths on the comparison of the two runs -- under knob 1 nearly every window from a wave's
second trip on keeps the q of the window before, finds no better lag and returns start -1."""
import contextlib
import ctypes

import numpy as np
import pytest

import cfo_model as cm
import demod_model as dm
import fec_model as fm
import reencode_model as rm
import sync_model as sm
import track_model as trm
import tx_model as tm
import test_cfo_gpu as tcfo
import test_decode_gpu as tdec
import test_demod_gpu as tdem
import test_reencode_gpu as tre
import test_sync_gpu as tsy
import test_track_gpu as ttr
import test_transmit_gpu as ttx

pytestmark = pytest.mark.gpu

GRID = 6                    # WCE_VARIANT_GRID
N, NBLK = dm.N, dm.NBLK
SWEEP = 12                  # frames per sweep of a four-wave kernel under the knob
BATCHES = (67, 13)
SENT = 7.0 - 3.0j


@contextlib.contextmanager
def _grid(wce, v):
    lib = wce.load()
    try:
        assert lib.wce_debug_set_variant(GRID, v) == 0
        yield
    finally:
        assert lib.wce_debug_set_variant(GRID, 0) == 0


def _u8(a):
    """any array -> its bytes, so that NaN rows compare too"""
    return np.ascontiguousarray(a).view(np.uint8)


def _refill(wce, d, a):
    a = np.ascontiguousarray(a)
    assert a.nbytes == d.nbytes
    assert wce.load().wce_memcpy_htod(d.ptr, a.ctypes.data_as(ctypes.c_void_p), a.nbytes) == 0


def _both(wce, outs, call):
    """outs: name -> (DeviceArray, its sentinel-filled initial contents).  call() under knob 0, then under knob 1,
    each from the initial contents -> knob 1's raw arrays, which must be knob 0's byte for byte"""
    raw = []
    for knob in (0, 1):
        for d, init in outs.values():
            _refill(wce, d, init)
        with _grid(wce, knob):
            call()
            wce.synchronize()
        raw.append({k: d.numpy() for k, (d, _) in outs.items()})
    for k in outs:
        assert np.array_equal(_u8(raw[0][k]), _u8(raw[1][k])), f"{k}: three workgroups give other bytes"
    return raw[1]


def _dev(wce, init):
    """name -> initial contents  ->  name -> (DeviceArray, initial contents)"""
    return {k: (wce.DeviceArray.from_numpy(v), v) for k, v in init.items()}


def _isnan(a):
    return np.isnan(np.ascontiguousarray(a).view(np.float64))


@pytest.fixture(scope="module")
def ctx(gpu_wce):
    c = gpu_wce.Context(empty=True)     # the ctx only selects the device
    lib = gpu_wce.load()
    assert lib.wce_debug_set_variant(GRID, 1) == 0
    assert lib.wce_debug_chain_grid((67 + 3) // 4, 4096) == 3      # the seam is in the library under test
    assert lib.wce_debug_set_variant(GRID, 0) == 0
    return c


# ---------------------------------------------------------------- front end
FE_FS, FE_BS = tcfo.FS, tcfo.BS         # 15 * 64 + 3, 60


@pytest.fixture(scope="module")
def fe_big():
    return tcfo.Big()


def _fe_bins(raw, B):
    """sym [B][FE_FS] -> ([B][15][53], the padding still holds SENT)"""
    mask = np.zeros(FE_FS, bool)
    for b in range(NBLK):
        mask[b * FE_BS:b * FE_BS + N] = True
    return tcfo._bins(raw, FE_BS), bool(np.all(raw[:, ~mask] == SENT))


@pytest.mark.parametrize("build", ["plain", "cfo"])
def test_front_end_blocks(gpu_wce, ctx, fe_big, build):
    """67 frames of 15 blocks: 1005 units, ten sweeps of 96 and a ragged one of 45; frames straddle the sweeps"""
    wce, B, off = gpu_wce, 67, 400
    pk, eps = fe_big.pk[:B], fe_big.eps[:B]
    D = wce.DeviceArray.from_numpy
    dpk = D(pk)
    dcfo = D(np.concatenate([eps, [9.0]])) if build == "cfo" else None
    outs = _dev(wce, {"sym": np.full((B, FE_FS), SENT, np.complex128)})
    got = _both(wce, outs, lambda: ctx.front_end_blocks(
        dpk, B, NBLK, outs["sym"][0], packet_stride=pk.shape[1], frame_stride=FE_FS, block_stride=FE_BS, cfo=dcfo,
        sample_offset=off if build == "cfo" else 0))
    bins, ok = _fe_bins(got["sym"], B)
    assert ok, "sym: padding overwritten"
    ref = cm.blocks(pk, eps, off) if build == "cfo" else cm.blocks(pk, np.zeros(B))
    err = cm.relmax(bins, ref)
    print(f"\nblocks {build} B={B}: {err:.2e} (TOL_BINS {tcfo.TOL_BINS:.0e})")
    assert err <= tcfo.TOL_BINS
    assert np.array_equal(_u8(dpk.numpy()), _u8(pk))


@pytest.mark.parametrize("build", ["plain", "given", "estimated"])
def test_front_end_preamble(gpu_wce, ctx, fe_big, build):
    """a unit is a frame here, so a sweep is 96 frames: 200 frames make two sweeps and a ragged one of 8"""
    wce, B, L = gpu_wce, 200, tcfo.L
    D = wce.DeviceArray.from_numpy
    if build == "estimated":
        lp, eps, _ = cm.ltf_batch(np.random.default_rng(0xC6A1), B, L, tcfo.LSTRIDE)
    else:
        lp, eps = fe_big.lp[:B], fe_big.eps[:B]
    dlp = D(lp)
    init = {"pre": np.full((B, tcfo.PRESTRIDE), SENT, np.complex128), "ow2": np.full(B + 1, 9.0)}
    dcfo = None
    if build == "estimated":
        init["cfo"] = np.full(B + 1, 9.0)
    elif build == "given":
        dcfo = D(np.concatenate([eps, [9.0]]))
    outs = _dev(wce, init)
    if build == "estimated":
        dcfo = outs["cfo"][0]
    got = _both(wce, outs, lambda: ctx.front_end_preamble(
        dlp, B, L, outs["pre"][0], outs["ow2"][0], lptot_stride=lp.shape[1], pre_stride=tcfo.PRESTRIDE, cfo=dcfo,
        estimate_cfo=build == "estimated"))
    assert np.all(got["pre"][:, N:] == SENT) and got["ow2"][B] == 9.0
    used = np.zeros(B)
    if build == "given":
        used = eps
        assert np.array_equal(dcfo.numpy()[:B], eps)             # read, not written
    elif build == "estimated":
        assert got["cfo"][B] == 9.0
        used = got["cfo"][:B]                                    # derotated with what the device wrote
        d_est = float(np.max(np.abs(used - cm.estimate(lp[:, :L]))))
        print(f"\npreamble estimated B={B}: cfo {d_est:.2e} (TOL_EST {tcfo.TOL_EST:.0e})")
        assert d_est <= tcfo.TOL_EST
    rp, rw = cm.preamble(lp[:, :L], used)
    err, ew = cm.relmax(got["pre"][:, :N], rp), float(np.max(np.abs(got["ow2"][:B] / rw - 1)))
    print(f"\npreamble {build} B={B}: bins {err:.2e}, ow2 {ew:.2e}")
    assert err <= tcfo.TOL_BINS and ew <= tcfo.TOL_OW2


AT_BAD = (5, 9)      # start -1; one sample over the window's end


@pytest.fixture(scope="module")
def at():
    return tsy.AtData()


@pytest.mark.parametrize("mode", ["given", "null"])
def test_front_end_blocks_at(gpu_wce, ctx, at, mode):
    """unit u and unit u + 96 meet on the same lanes of the same wave: a frame's 15 units are followed there by
    units of the frames 6 and 7 behind it.  Frames 5 and 9 have no usable start; 11, 12, 15 and 16 are good"""
    wce, B, W, off = gpu_wce, 67, tsy.AT_W, 160
    D = wce.DeviceArray.from_numpy
    fit = W - 128 - off - NBLK * 80
    s = at.start.copy()
    s[AT_BAD[0]], s[AT_BAD[1]], s[20] = -1, fit + 1, fit
    s, cap, eps = s[:B], at.cap[:B], at.eps[:B]
    dcap, dst = D(cap), D(s)
    dcfo = D(eps) if mode == "given" else None
    outs = _dev(wce, {"sym": np.full((B, FE_FS), SENT, np.complex128)})
    got = _both(wce, outs, lambda: ctx.front_end_blocks(
        dcap, B, NBLK, outs["sym"][0], packet_stride=cap.shape[1], frame_stride=FE_FS, block_stride=FE_BS, cfo=dcfo,
        sample_offset=off, start=dst, capture_len=W))
    bins, ok = _fe_bins(got["sym"], B)
    assert ok, "sym: padding overwritten"
    good = np.ones(B, bool)
    good[list(AT_BAD)] = False
    assert _isnan(bins[~good]).all()
    assert all(good[f + 6] and good[f + 7] for f in AT_BAD)
    aligned = at.aligned(np.concatenate([s, at.start[B:]]), 128 + off, NBLK * 80)[:B]
    err = cm.relmax(bins[good], cm.blocks(aligned, eps if mode == "given" else np.zeros(B), off)[good])
    print(f"\nblocks_at {mode}: {err:.2e}")
    assert err <= tcfo.TOL_BINS


@pytest.mark.parametrize("mode", ["given", "estimated", "null"])
def test_front_end_preamble_at(gpu_wce, ctx, at, mode):
    """200 frames, a sweep is 96: frames 5 and 9 have no usable start, 101 and 105 follow them on their lanes"""
    wce, B, W = gpu_wce, 200, tsy.AT_W
    D = wce.DeviceArray.from_numpy
    s = at.start.copy()
    s[AT_BAD[0]], s[AT_BAD[1]], s[20] = -1, W - 128 + 1, W - 128
    s, cap, eps = s[:B], at.cap[:B], at.eps[:B]
    dcap, dst = D(cap), D(s)
    init = {"pre": np.full((B, tsy.AT_PRE), SENT, np.complex128), "ow2": np.full(B + 1, 9.0)}
    dcfo = None
    if mode == "estimated":
        init["cfo"] = np.full(B + 1, 9.0)
    elif mode == "given":
        dcfo = D(eps)
    outs = _dev(wce, init)
    if mode == "estimated":
        dcfo = outs["cfo"][0]
    got = _both(wce, outs, lambda: ctx.front_end_preamble(
        dcap, B, W, outs["pre"][0], outs["ow2"][0], lptot_stride=cap.shape[1], pre_stride=tsy.AT_PRE, cfo=dcfo,
        estimate_cfo=mode == "estimated", start=dst, capture_len=W))
    good = np.ones(B, bool)
    good[list(AT_BAD)] = False
    assert all(good[f + 96] for f in AT_BAD)
    assert np.all(got["pre"][:, N:] == SENT) and got["ow2"][B] == 9.0
    assert _isnan(got["pre"][~good, :N]).all() and np.isnan(got["ow2"][:B][~good]).all()
    used = np.zeros(B)
    if mode == "given":
        used = eps
    elif mode == "estimated":
        assert got["cfo"][B] == 9.0 and np.isnan(got["cfo"][:B][~good]).all()
        used = got["cfo"][:B]
    aligned = at.aligned(np.concatenate([s, at.start[B:]]), 0, 128)[:B]
    if mode == "estimated":
        assert float(np.max(np.abs(used[good] - cm.estimate(aligned)[good]))) <= tcfo.TOL_EST
    rp, rw = cm.preamble(aligned[good], used[good])
    err = cm.relmax(got["pre"][good, :N], rp)
    ew = float(np.max(np.abs(got["ow2"][:B][good] / rw - 1)))
    print(f"\npreamble_at {mode}: bins {err:.2e}, ow2 {ew:.2e}")
    assert err <= tcfo.TOL_BINS and ew <= tcfo.TOL_OW2


# ---------------------------------------------------------------- sync
SYNC_THRESHOLD = 0.25


def _sync_windows(L):
    """the 777-window set of sync_model at length L (L = 1100: the same generator at 67 windows, since the set's
    longest window, 488 samples, is one tile of 448 lags and this one is three), with the pairs f, f + 12:
    0 NaN-poisoned, 12 a clean packet; 1 a strong packet at the last lag, 13 noise alone; 2 a peak at the last
    lag (in the last tile), 14 a peak at lag 0"""
    B = 777 if L <= 488 else 67
    cap, _ = sm.shape_set(B, L) if L <= 488 else sm.captures(0x5C00 + 1000 * B + L, B, L)
    orig = cap.copy()
    cap = cap.copy()
    rng = np.random.default_rng(0x5CC0 + L)
    ltf = sm.clean_ltf()
    cap[0, min(300, L - 1)] = complex(np.nan, 0.0)
    strong = cm.random_packets(rng, 1, L, 1e-4)[0]
    strong[L - 128:L] += np.tile(ltf, 2)
    cap[1, :L] = strong
    cap[13, :L] = cm.random_packets(rng, 1, L, 1.0)[0]
    cap[2], cap[14] = orig[1], orig[3]
    return cap, ltf


@pytest.mark.parametrize("L", [192, 488, 1100])
def test_sync(gpu_wce, ctx, L):
    wce = gpu_wce
    cap, ltf = _sync_windows(L)
    B = cap.shape[0]
    start, metric, d = sm.sync(cap[:, :L], ltf, SYNC_THRESHOLD)
    assert np.min(np.abs(metric[np.isfinite(metric)] - SYNC_THRESHOLD)) > 1e-9       # the threshold decides exactly
    assert start[0] == -1 and np.isnan(metric[0]) and start[12] >= 0
    assert metric[1] > 0.999 and d[1] == L - 128 and start[13] == -1 and 0 < metric[13] < 0.2
    assert d[2] == L - 128 and d[14] == 0 and start[14] == 0
    assert L - 128 < 448 or d[2] >= 448 * ((L - 128) // 448)                        # in the window's last tile
    D = wce.DeviceArray.from_numpy
    dcap, dltf = D(cap), D(ltf)
    outs = _dev(wce, {"start": np.full(B + 1, tsy.SENT_START, np.int32),
                      "metric": np.full(B + 1, tsy.SENT_METRIC, np.float64)})
    got = _both(wce, outs, lambda: ctx.front_end_sync(dcap, B, L, dltf, SYNC_THRESHOLD, 0, outs["start"][0],
                                                      outs["metric"][0], capture_stride=cap.shape[1]))
    assert got["start"][B] == tsy.SENT_START and got["metric"][B] == tsy.SENT_METRIC
    fin = np.isfinite(metric)
    err = float(np.max(np.abs(got["metric"][:B][fin] - metric[fin])))
    print(f"\nsync L={L} B={B}: metric within {err:.2e} (TOL_M {sm.TOL_M:.0e}); frames 1, 13: "
          f"{got['metric'][1]:.6f} {got['metric'][13]:.6f} (model {metric[13]:.6f})")
    assert np.array_equal(got["start"][:B], start)
    assert np.array_equal(np.isnan(got["metric"][:B]), ~fin) and err <= sm.TOL_M
    assert np.array_equal(_u8(dcap.numpy()), _u8(cap))


# ---------------------------------------------------------------- demodulate
DEMOD_SUBSETS = [s for s in (("eq",), ("sym",), ("theta",), ("eq", "sym"), ("eq", "theta"), ("sym", "theta"),
                             ("eq", "sym", "theta"))]


def _demod_unpad(r, raw, B):
    out = {}
    for k, a in raw.items():
        if k in ("eq", "sym"):
            out[k], ok = tdem._unpad(a, tdem.SENT if k == "eq" else tdem.SENT8)
            assert ok, f"{k}: padding overwritten"
        else:
            assert a[-1] == r.init[k][-1], f"{k}: written past the end"
            out[k] = a[:-1].reshape(B, NBLK) if k == "theta" else a[:-1]
    return out


def _demod_both(wce, ctx, r, B):
    """r: a tdem.Run, whose constructor made the call (under knob 0) -> knob 1's outputs on the same buffers, unpadded"""
    raw0 = {k: d.numpy() for k, d in r.dev.items()}
    for k, d in r.dev.items():
        _refill(wce, d, r.init[k])
    with _grid(wce, 1):
        ctx.demodulate(r.fr, r.keep[2], **r.kw, **r.dev)
        wce.synchronize()
    raw1 = {k: d.numpy() for k, d in r.dev.items()}
    for k in raw0:
        assert np.array_equal(_u8(raw0[k]), _u8(raw1[k])), f"{k}: three workgroups give other bytes"
    return _demod_unpad(r, raw1, B)


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("track", [True, False])
def test_demodulate_without_the_sums(gpu_wce, ctx, track, B):
    mod = dm.QAM16
    tx, rx, h, h_lt = (a[:B] for a in tdem._synthetic(mod))
    ref = tdem._model(mod, track, True, True)
    for outs in DEMOD_SUBSETS:
        r = tdem.Run(gpu_wce, ctx, tx, rx, h, h_lt, mod, track, True, outs=outs)
        out = _demod_both(gpu_wce, ctx, r, B)
        assert set(out) == set(outs)
        if "eq" in out:
            assert dm.relmax_frames(out["eq"], ref["eq"][:B]).max() <= dm.TOL_EQ, outs
        if "sym" in out:
            assert np.array_equal(out["sym"], ref["sym"][:B]), outs
        if "theta" in out:
            assert np.max(np.abs(out["theta"] - np.asarray(ref["theta"][:B], np.float64))) <= dm.TOL_TH, outs
            assert track or not np.any(out["theta"])


def test_demodulate_with_the_sums_covers_the_batch(gpu_wce, ctx):
    """the evm / nerr builds have no frame loop: the knob must leave their grid alone, every entry written"""
    mod, B = dm.QAM16, 67
    tx, rx, h, h_lt = tdem._synthetic(mod)
    r = tdem.Run(gpu_wce, ctx, tx, rx, h, h_lt, mod, True, True)
    out = _demod_both(gpu_wce, ctx, r, B)
    assert np.all(out["evm"] != 9.0) and np.all(out["nerr"] != 0xDEAD)
    tdem._compare(out, tdem._model(mod, True, True, True), slice(0, B), "evm / nerr under the knob")


# ---------------------------------------------------------------- track
def test_track_demodulate_ignores_the_knob(gpu_wce, ctx):
    """launch_track has no frame loop and never reads the knob: one call at 67 frames, every output written"""
    wce, mod, B = gpu_wce, dm.QAM16, 67
    tx, rx, h = trm.drifting_set(mod)
    r = ttr.Run(wce, ctx, tx, rx, h, mod, trm.MU, trm.BETA)
    raw0 = {k: d.numpy() for k, d in r.dev.items()}
    for k, d in r.dev.items():
        _refill(wce, d, r.init[k])
    with _grid(wce, 1):
        ctx.track_demodulate(r.fr, r.keep[2], trm.MU, trm.BETA, **r.kw, **r.dev)
        wce.synchronize()
    for k, d in r.dev.items():
        assert np.array_equal(_u8(raw0[k]), _u8(d.numpy())), k
    ttr._compare(r.out, trm.model(mod, trm.MU, trm.BETA), slice(0, B), "track under the knob")


# ---------------------------------------------------------------- soft demap
def _demap_data(mod, bl):
    """the clean set's eq, h, h_lt with the erasures of test_soft_bits_of_non_finite_symbols_are_erasures in the
    frames 0 and 12; 24 and 36, the next two of wave 0, are clean"""
    s = fm.clean_set(mod, fm.RATE_1_2)
    eq, h = tdec._demap_ref(mod, bl)[0].copy(), s["h"].copy()
    h_lt = s["h_lt"].copy() if bl else None
    for f in (0, SWEEP):
        eq[f, 7, 30] = np.nan                       # one symbol
        h[f, 11] = np.inf                           # a data subcarrier of the estimate: its 15 symbols
        eq[f, 0, 5] = np.nan                        # a pilot: no soft bit comes from it
    return eq, h, h_lt


def _erased(mod, shape):
    inv = np.argsort(fm.interleave_index(mod))
    where = lambda k: inv[mod * int(np.searchsorted(dm.DATA, k)) + np.arange(mod)]
    zero = np.zeros(shape, bool)
    for f in (0, SWEEP):
        zero[f, 7, where(30)] = True
        zero[f, :, where(11)] = True
    return zero


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("blocks", [False, True])
@pytest.mark.parametrize("mod", fm.MODS)
def test_soft_demap(gpu_wce, ctx, mod, blocks, B):
    wce = gpu_wce
    D = wce.DeviceArray.from_numpy
    lbs, lfs = tdec._strides(mod)
    for bl in (True, False):
        eq, h, h_lt = _demap_data(mod, bl)
        with np.errstate(all="ignore"):                 # the Inf of frames 0 and 12 goes through the blend
            hu = np.asarray(dm.blend(h, h_lt, np.float64), np.complex128)
            ld = fm.llr(eq, hu if blocks else dm.blend(h, h_lt), mod)[:B]
        clean = fm.llr(tdec._demap_ref(mod, bl)[0][:B], dm.blend(fm.clean_set(mod, fm.RATE_1_2)["h"][:B],
                                                                 h_lt[:B] if bl else None), mod)
        deq = D(tdec._pad_eq(eq[:B]))
        outs = _dev(wce, {"llr": np.full((B, lfs), tdec.SENTF, np.float32)})
        if blocks:
            dhb = D(tdec._pad_eq(hu[:B]))
            call = lambda: ctx.soft_demap_blocks(deq, dhb, B, mod, llr=outs["llr"][0], eq_frame_stride=tdec.EFS,
                                                 eq_block_stride=tdec.EBS, hb_frame_stride=tdec.EFS,
                                                 hb_block_stride=tdec.EBS, llr_frame_stride=lfs, llr_block_stride=lbs)
        else:
            dh = D(tdec._pad_rows(h[:B]))
            dhl = D(tdec._pad_rows(h_lt[:B])) if bl else None
            call = lambda: ctx.soft_demap(deq, dh, B, h_lt=dhl, h_stride=tdec.HS, modulation=mod, llr=outs["llr"][0],
                                          eq_frame_stride=tdec.EFS, eq_block_stride=tdec.EBS, llr_frame_stride=lfs,
                                          llr_block_stride=lbs)
        got = _both(wce, outs, call)
        L, ok = tdec._unpad_llr(got["llr"], mod)
        assert ok, "llr: padding overwritten"
        tdec._within_bound(L, ld, f"{mod} bits B={B} blocks={blocks} blend={bl}")
        zero = _erased(mod, L.shape)
        assert np.all(L[zero] == 0) and not np.any(np.signbit(L[zero])) and np.all(np.asarray(clean)[zero] != 0)
        if B > 3 * SWEEP:       # nothing of an erased row is left for the frames behind it
            assert np.all(L[2 * SWEEP] != 0) and np.all(L[3 * SWEEP] != 0)


# ---------------------------------------------------------------- viterbi
def _viterbi_frames(mod, rate):
    """the integer set with the frames 0..11 all-zero and 12..23 a tenth non-finite: at a sweep of 12, 6 or 3
    frames (4, 2 or 1 waves a workgroup) every wave decodes both kinds before an ordinary frame"""
    s = fm.integer_set(mod, rate)
    L = s["llr"].copy()
    rng = np.random.default_rng(0x71 + 16 * mod + rate)
    L[:SWEEP] = 0
    hit = rng.random(L[SWEEP:2 * SWEEP].shape) < 0.1
    zeroed = L[SWEEP:2 * SWEEP].copy()
    zeroed[hit] = 0
    L[SWEEP:2 * SWEEP][hit] = rng.choice(np.array([np.nan, np.inf, -np.inf], np.float32), int(hit.sum()))
    return L, zeroed, s["u"]


@pytest.mark.parametrize("mod,rate", fm.COMBOS)
def test_viterbi(gpu_wce, ctx, mod, rate):
    wce = gpu_wce
    D = wce.DeviceArray.from_numpy
    T = fm.info_bits(mod, rate)
    nby = (T + 7) // 8
    lbs, lfs = tdec._strides(mod)
    L, zeroed, u = _viterbi_frames(mod, rate)
    r = np.full((67, nby + 2), 0xFF, np.uint8)
    r[:, :nby] = fm.pack(u)
    if T % 8:
        r[:, nby - 1] |= (0xFF << (T % 8)) & 0xFF
    for terminated in (True, False):
        bits, _ = fm.integer_model(mod, rate, terminated)
        want = bits.copy()
        want[:SWEEP] = 0
        want[SWEEP:2 * SWEEP] = fm.decode(zeroed, mod, rate, terminated)
        nerr = np.sum(want != u, axis=1).astype(np.uint32)
        for B in BATCHES:
            dl, dref = D(tdec._pad_llr(L[:B], mod)), D(r[:B])
            outs = _dev(wce, {"bits": np.full((B, nby + 3), tdec.SENT8, np.uint8),
                              "nbiterr": np.full(B + 1, 0xDEAD, np.uint32)})
            got = _both(wce, outs, lambda: ctx.viterbi_decode(
                dl, B, mod, rate, terminated=terminated, bits=outs["bits"][0], bits_stride=nby + 3, ref_bits=dref,
                ref_stride=nby + 2, nbiterr=outs["nbiterr"][0], llr_frame_stride=lfs, llr_block_stride=lbs))
            assert np.all(got["bits"][:, nby:] == tdec.SENT8) and got["nbiterr"][B] == 0xDEAD
            out = np.unpackbits(got["bits"][:, :nby], axis=1, bitorder="little")
            assert not out[:, T:].any()
            assert np.array_equal(out[:, :T], want[:B]), (terminated, B)
            assert np.array_equal(got["nbiterr"][:B], nerr[:B]), (terminated, B)


# ---------------------------------------------------------------- re-encode
@pytest.mark.parametrize("mod,rate", fm.COMBOS)
def test_reencode_symbols(gpu_wce, ctx, mod, rate):
    """tx alone, with 802.11's pilots and with the frames' own"""
    wce = gpu_wce
    D = wce.DeviceArray.from_numpy
    u, x = tre._x_set(mod, rate)           # 77 frames: six sweeps and a ragged one of 5
    pil = -0.5 * rm.standard_pilots(len(u))
    for B in (len(u), 13):
        for own in (False, True):
            packed = tre._pack(u[:B])
            dbits = D(packed)
            fr, dptx = None, None
            want = x[:B].copy()
            if own:
                dptx = D(tre._pad_frames(tre._poisoned(pil[:B]), np.nan))
                fr = ctx.frames(dptx, None, B, frame_stride=tre.FS, block_stride=tre.BS)
                want[:, :, tre.P] = pil[:B]
            outs = _dev(wce, {"tx": np.full((B, tre.FS), SENT, np.complex128)})
            got = _both(wce, outs, lambda: ctx.reencode(dbits, B, mod, rate, bits_stride=packed.shape[1], frames=fr,
                                                        tx=outs["tx"][0], tx_frame_stride=tre.FS,
                                                        tx_block_stride=tre.BS))
            tx, ok = tre._unpad_frames(got["tx"])
            assert ok, "tx: padding overwritten"
            assert tre._same_bits(tx, want), (B, own)


GUARD = 16      # doubles of NaN on either side of theta's 15 B


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("mod,rate", tre.H_SETS)
def test_reencode_estimate(gpu_wce, ctx, mod, rate, B):
    """h alone and with tx, with and without theta, with and without the frames' own pilots.  Every angle of the
    batch is another, so a rotor from the frame one sweep on (or back) moves H_dd; theta ends where the batch
    ends, so the last trip's prefetch must stop at f + step < n"""
    wce = gpu_wce
    D = wce.DeviceArray.from_numpy
    s = fm.clean_set(mod, rate)
    u, rx, theta = s["u"][:B], s["rx"][:B], rm.clean_theta(mod, rate)[:B]
    assert len(np.unique(theta)) == B * NBLK and np.min(np.abs(theta)) > 1e-6
    x = rm.xhat(u, mod, rate)
    pil = x[:, :, tre.P]
    packed = tre._pack(u)
    dbits = D(packed)
    drx = D(tre._pad_frames(rx, np.nan))
    dptx = D(tre._pad_frames(tre._poisoned(pil), np.nan))
    guarded = np.full(B * NBLK + 2 * GUARD, np.nan)
    guarded[GUARD:GUARD + B * NBLK] = theta.reshape(-1)
    dth = D(guarded)
    ld = {True: rm.h_dd(x, rx, theta)[0], False: rm.h_dd(x, rx, None)[0]}
    assert rm.relmax_rows(np.asarray(ld[True], np.complex128), ld[False]).min() > 1e-3      # theta matters everywhere
    ref = {}
    for with_tx in (False, True):
        for turn in (True, False):
            for own in (True, False):
                fr = ctx.frames(dptx if own else None, drx, B, frame_stride=tre.FS, block_stride=tre.BS)
                init = {"h": np.full((B, tre.HS), SENT, np.complex128)}
                if with_tx:
                    init["tx"] = np.full((B, tre.FS), SENT, np.complex128)
                outs = _dev(wce, init)
                got = _both(wce, outs, lambda: ctx.reencode(
                    dbits, B, mod, rate, bits_stride=packed.shape[1], theta=dth.addr + 8 * GUARD if turn else None,
                    frames=fr, tx=outs["tx"][0] if with_tx else None, tx_frame_stride=tre.FS, tx_block_stride=tre.BS,
                    h=outs["h"][0], h_stride=tre.HS))
                assert np.all(got["h"][:, N:] == SENT), "h: padding overwritten"
                tre._within(got["h"][:, :N], ld[turn], f"{mod} bits rate {rate} B={B} tx={with_tx} theta={turn} own={own}")
                if with_tx:
                    tx, ok = tre._unpad_frames(got["tx"])
                    assert ok and tre._same_bits(tx, x)
                # the builds round H_dd alike, and the set's pilots are 802.11's
                assert tre._same_bits(got["h"], ref.setdefault(turn, got["h"])), (with_tx, turn, own)
    assert np.array_equal(dth.numpy(), guarded, equal_nan=True) and np.array_equal(dbits.numpy(), packed)


# ---------------------------------------------------------------- modulate, channel, transmit
TX_B = 10           # a sweep is 3 frames: three full ones and one frame more
TX_SHAPES = sorted({(nb, field) for _, nb, field in tm.SHAPES})
TX_BAD = 2          # its symbols (or its preamble, or its waveform) hold a NaN; frame 5 follows it on its workgroup


def _tx_layout(wce, nb, field):
    """ttx.Layout at 10 frames with a NaN in frame 2 -> (layout, the clean symbols and preambles)"""
    lay = ttx.Layout(wce, TX_B, nb, field)
    sym, pre = lay.sym.copy(), None if lay.pre is None else lay.pre.copy()
    if nb:
        sym[TX_BAD, nb - 1, 52] = np.nan
        lay.dsym = ttx.dev(wce, ttx.padded_sym(sym, lay.bs, lay.fs))
    else:
        pre[TX_BAD, 10] = np.nan
        lay.dpre = ttx.dev(wce, tm.padded(pre, 55))
        lay.sym_kw["tx_pre"] = lay.dpre
    return lay


def _tx_chan(rng, L, S, nt):
    """per-frame taps, offsets, noise and delays.  In the long window frame 1 starts 600 samples in and frame 7 600
    samples before it: channel_kernel stages nothing for frame 1's first tile and frame 7's last, where frame 4,
    between them on the same workgroup, stages every tile"""
    delay = rng.integers(-20, 60, TX_B)
    if L > 1100:
        delay[1], delay[7] = 600, -600
    return dict(taps=tm.random_taps(rng, TX_B, nt), cfo=rng.uniform(-0.002, 0.002, TX_B),
                ow2=rng.uniform(0.5, 2.0, TX_B) * 1e-4, delay=delay, first_frame=11)


def _tx_check(got, L, lay, wave, chan, nt, from_symbols, what):
    """the capture [B][L + pad] against the model as test_transmit_is_the_pair_bit_for_bit holds it: from the
    symbols on, or (the channel alone) from the clean waveform `wave` the device was given"""
    good = np.arange(TX_B) != TX_BAD
    assert np.all(got[:, L:] == SENT), what
    assert np.all(np.isnan(got[TX_BAD, :L].real) & np.isnan(got[TX_BAD, :L].imag)), what
    quiet = dict(chan, ow2=None, delay=None)
    if from_symbols:
        ref = tm.transmit(lay.sym, L, lay.pre, **chan)
        full = tm.transmit(lay.sym, lay.S + nt - 1, lay.pre, **quiet)
    else:
        ref = tm.channel(wave, L, field=lay.field, **chan)
        full = tm.channel(wave, lay.S + nt - 1, field=lay.field, **quiet)
    scale = np.max(np.abs(full), axis=1).astype(np.float64)
    tol = tm.cap_tol(wave, chan["taps"], chan["cfo"], full, lay.field, from_symbols) + \
        tm.TOL_NOISE * np.sqrt(chan["ow2"]) / scale
    err = np.max(np.abs(got[:, :L].astype(np.clongdouble) - ref), axis=1).astype(np.float64) / scale
    assert np.all(err[good] <= tol[good]), (what, float(np.max(err[good] / tol[good])))


@pytest.mark.parametrize("nb,field", TX_SHAPES)
def test_modulate_channel_transmit(gpu_wce, ctx, nb, field):
    wce = gpu_wce
    lay = _tx_layout(wce, nb, field)
    S, B = lay.S, TX_B
    good = np.arange(B) != TX_BAD
    rng = np.random.default_rng(0x7CC0 + 4 * nb + field)
    # modulate
    outs = _dev(wce, {"wave": np.full((B, S + 5), SENT, np.complex128)})
    got = _both(wce, outs, lambda: ctx.modulate(lay.dsym, B, outs["wave"][0], wave_stride=S + 5, **lay.sym_kw))
    assert np.all(got["wave"][:, S:] == SENT)
    wave = got["wave"][:, :S]
    model_wave = tm.modulate(lay.sym, lay.pre)
    assert float(tm.relmax_rows(wave[good], model_wave[good]).max()) <= tm.TOL_WAVE
    assert np.isnan(wave[TX_BAD].real).any()
    for nt, L in ((16, 1488), (6, S + 5), (1, 129)):
        chan = _tx_chan(rng, L, S, nt)
        # channel, on the model's waveform with frame 2 poisoned
        clean = np.asarray(model_wave, np.complex128)
        dirty = clean.copy()
        dirty[TX_BAD, S // 2] = complex(0.0, np.nan)
        kw, keep = ttx.chan_inputs(wce, B, **{k: v for k, v in chan.items() if k != "first_frame"})
        dw = ttx.dev(wce, tm.padded(dirty, S + 2))
        outs = _dev(wce, {"cap": np.full((B, L + 3), SENT, np.complex128)})
        got = _both(wce, outs, lambda: ctx.channel(dw, B, S, outs["cap"][0], L, field=bool(field), seed=tm.SEED,
                                                   first_frame=11, wave_stride=S + 2, capture_stride=L + 3, **kw))
        _tx_check(got["cap"], L, lay, clean, chan, nt, False, ("channel", nb, field, nt, L))
        # transmit, from the symbols
        outs = _dev(wce, {"cap": np.full((B, L + 3), SENT, np.complex128)})
        got = _both(wce, outs, lambda: ctx.transmit(lay.dsym, B, outs["cap"][0], L, seed=tm.SEED, first_frame=11,
                                                    capture_stride=L + 3, **lay.sym_kw, **kw))
        _tx_check(got["cap"], L, lay, clean, chan, nt, True, ("transmit", nb, field, nt, L))
