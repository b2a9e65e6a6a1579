"""The frame law on the device: every row of tests/frame_model.py through the
library's calls.  The reference of every comparison is the same call on the
base batch in the same process, and no tolerance is used anywhere: a frame
moved to another place, run in a smaller batch or given hostile neighbours keeps
its bits.  Every stride is padded with sentinels that must survive (the drivers
are tests/test_gain_gpu.py's).  tests/test_frame_model.py has proved each row
and each input set on the numpy models.

Batches, and the packing unit each makes ragged (read from the launchers):
    67 = 4 * 16 + 3   ls_kernel's 4 frames per wave and 16 per workgroup; mmse_rank1_kernel's 16 units per
                      workgroup and the head kernel's rows; the quad kernels' 4 frames per wave and 16 per
                      workgroup (launch_mmse_lr, launch_lr_quad2); the 16-frame MFMA tiles of apply_kernel and
                      matvec_kernel; avg_blocks_kernel's and fc_finish_kernel's 4 frames per workgroup; the lane
                      kernels' 64-frame waves; mmse_ref_flat_kernel's 512-element chunks (9.66 frames: ragged at
                      any size).  MATLAB semantics makes 268 units of them, ragged for the 256-unit staged
                      workgroups as well
    261 = 256 + 5     C semantics, ranks 4 and 8: the lane kernels' 64-lane waves and the staged form's 256-thread
                      workgroups, one full workgroup and a 5-lane tail
    5                 the chain calls, beside 67: less than any unit
No kernel needed a third size.

Builds reached through a knob (wce_debug_set_variant), each named before it runs by wce.debug_route,
wce_debug_rank1_head or wce_debug_lr_kernel, so that a test fails if the route it believes it runs is not the
one planned.  What the knob of a launcher decides by itself (mmse_ref_elem_kernel against the flat kernel,
ls_elem_kernel against the light ls_kernel) has no name to ask for: there the knob is the name.
Not reached: mmse_lr_lane_kernel at fewer than 64 units per wave (LR_FPW_BELOW switches on the batch size alone,
and at and below it the direct form already runs 64 per wave, which variant 2 covers).

Outputs excepted from the law.  An entry is allowed only for an output whose dependence on position
include/wce.h states, quoted here; never for an estimator output, eq, sym, start, bits or a wce_combine output:

    call    output    the header's words
    (none)
"""
import functools

import numpy as np
import pytest

import combine_model as cb
import demod_model as dm
import fec_model as fm
import frame_model as fr
import gain_model as gm
import psdu_model as pm
import test_gain_gpu as tg
from oracle_py import N, NBLK
from test_cov_lowrank_gpu import pdp_rhh
from test_decode_gpu import viterbi
from test_gain_gpu import BS, FS, HS, ROUTES, SENT, SENT8, SENTD, _dev, _rows, _tail, _unblocks, _unrows, _untail

pytestmark = pytest.mark.gpu

EXCEPTIONS = {}                      # the table above
BATCHES = (5, 67)
REF, LS, REF_LS, LR, REF_FC, R1 = 0, 1, 2, 3, 4, 5      # WCE_VARIANT_*


@pytest.fixture(scope="module")
def ctx(gpu_wce):
    import tx_model as tm
    pre = tm.chain_pre()
    c = gpu_wce.Context(pre, pre, 1e-6, gpu_wce.MMSE_TEXTBOOK)
    yield c
    c.close()


def hold(key, run, args, B, covered=False):
    assert not EXCEPTIONS
    row = fr.BY_KEY[key] if isinstance(key, str) else key

    def checked(x):      # a driver sizes its call by one buffer: every other one must hold as many frames
        sizes = {x[n].shape[ax] for n, ax in row.frame.items() if x.get(n) is not None}
        assert len(sizes) <= 1, f"{row.key}: per-frame buffers of {sorted(sizes)} frames in one call"
        return run(x)
    return fr.hold(row, checked, args, fr.transforms(row, B, covered))


# ---------------------------------------------------------------- the estimators
@functools.lru_cache(maxsize=None)
def _estimate_args(B):
    return fr.vary_tx(dict(tg._estimate_set(B), Rhh=None))


def _mode(wce, r):
    return {"ref": wce.MMSE_REF, "textbook": wce.MMSE_TEXTBOOK}[r["mode"]]


def _planned(wce, r, sem, mask, knobs):
    """the kernel families wce.debug_route plans for a route that is not WCE_MMSE_COV"""
    knobs = knobs or {}
    full = mask | (wce.FRAME_COV if r.get("fc") else 0)
    return wce.debug_route(_mode(wce, r), r.get("bdot", True), r.get("fuse", True), False, -1, 0,
                           wce.SEM_MATLAB if sem == "MATLAB" else wce.SEM_C, full, bool(r.get("f32")),
                           knobs.get(R1, r.get("variant", 0)), knobs.get(REF_FC, 0), knobs.get(REF_LS, 0),
                           noise=bool(r.get("noise"))).split(";")


def estimate_law(wce, r, sem, B, mask=None, knobs=None, family=None, kernel=None, head=None):
    """all transforms of one route.  family: a kernel family the planner must name; kernel: what
    wce_debug_lr_kernel must answer (its beginning); head: the threads wce_debug_rank1_head must answer"""
    a = dict(_estimate_args(B))
    if r["mode"] == "cov":
        a["Rhh"] = pdp_rhh(*r["rhh"])
    if not r.get("noise"):
        a["ow2"] = None
    if mask is None:
        mask = wce.PS_MMSE if r.get("mmse_only") else wce.ALL
    if family is not None:
        plan = _planned(wce, r, sem, mask, knobs)
        assert any(f == family or f.startswith(family + "_") for f in plan), (family, plan)
    if head is not None:
        v = (knobs or {}).get(R1, r.get("variant", 0))
        got = wce.load().wce_debug_rank1_head(1, 0, 0, 0, 1, 0, v, FS, HS, B, 8, None)
        assert got == head, (v, got)

    def probe(c, units):
        if kernel is not None:
            assert c.lr_kernel(units).startswith(kernel), (c.lr_kernel(units), kernel)
    run = lambda x: tg.run_estimate(wce, x, r, sem, mask=mask, knobs=knobs, probe=probe)
    base = hold("estimate", run, a, B)
    assert base and all(np.isfinite(v.view(v.real.dtype)).all() for v in base.values())


@pytest.mark.parametrize("sem", ["C", "MATLAB"])
@pytest.mark.parametrize("route", list(ROUTES))
def test_estimate(gpu_wce, route, sem):
    """every route of tests/test_gain_gpu.py at 67 frames, all five estimators and eq wherever asked for"""
    estimate_law(gpu_wce, ROUTES[route], sem, 67)


_TB1 = dict(mode="textbook", mmse_only=True)
KNOBS = {     # name -> (route facts, semantics, frames, knobs, what names the build)
    "ref-flat": (dict(mode="ref", mmse_only=True), "C", 67, {REF: 0}, dict(family="ref_pilots")),
    "ref-elem": (dict(mode="ref", mmse_only=True), "C", 67, {REF: 3}, dict(family="ref_pilots")),
    "ref-solve_ls": (dict(mode="ref"), "C", 67, {REF_LS: 1}, dict(family="fused")),
    "frame_cov-general": (dict(mode="textbook", fc=True), "C", 67, {REF_FC: 1}, dict(family="matvec")),
    "ref-frame_cov-general": (dict(mode="ref", fc=True), "C", 67, {REF_FC: 1}, dict(family="ref_w")),
    "rank4-staged": (dict(mode="cov", rhh=(4, 0.5)), "C", 261, {}, dict(kernel="mmse_lr_lane_staged_kernel<4")),
    "rank8-staged": (dict(mode="cov", rhh=(8, 0.5)), "C", 261, {}, dict(kernel="mmse_lr_lane_staged_kernel<8, 1")),
    "rank8-staged-matlab": (dict(mode="cov", rhh=(8, 0.5)), "MATLAB", 67, {},
                            dict(kernel="mmse_lr_lane_staged_kernel<8, 1")),
    "rank4-direct": (dict(mode="cov", rhh=(4, 0.5)), "C", 261, {LR: 2}, dict(kernel="mmse_lr_lane_kernel<4>")),
    "rank8-direct": (dict(mode="cov", rhh=(8, 0.5)), "C", 261, {LR: 2}, dict(kernel="mmse_lr_lane_kernel<8>")),
    "rank4-wave": (dict(mode="cov", rhh=(4, 0.5)), "C", 67, {LR: 1}, dict(kernel="mmse_lr_kernel<")),
    "rank12-wave": (dict(mode="cov", rhh=(12, 0.5)), "C", 67, {LR: 1}, dict(kernel="mmse_lr_kernel<")),
    "rank8-two_workgroups": (dict(mode="cov", rhh=(8, 0.5)), "C", 261, {LR: 4},
                             dict(kernel="mmse_lr_lane_staged_kernel<8, 2")),
    "rank8-product_gram": (dict(mode="cov", rhh=(8, 0.5)), "C", 261, {LR: 5},
                           dict(kernel="mmse_lr_lane_staged_kernel<8>")),
    "rank12-product_gram": (dict(mode="cov", rhh=(12, 0.5)), "C", 67, {LR: 5}, dict(kernel="mmse_lr_quad_kernel<12>")),
    "rank24-product_gram": (dict(mode="cov", rhh=(24, 0.3)), "C", 67, {LR: 5}, dict(kernel="mmse_lr_kernel<")),
    "rank1-nontemporal": (_TB1, "C", 67, {R1: 2}, dict(family="mmse_rank1_nt")),
    "rank1-head_off": (_TB1, "C", 67, {R1: 13}, dict(family="mmse_rank1", head=0)),
    "rank1-head_64": (_TB1, "C", 67, {R1: 14}, dict(family="mmse_rank1", head=64)),
    "rank1-head_128": (_TB1, "C", 67, {R1: 15}, dict(family="mmse_rank1", head=128)),
    "rank1-head_256": (_TB1, "C", 67, {R1: 16}, dict(family="mmse_rank1", head=256)),
    "rank1-head_adopted": (_TB1, "C", 67, {R1: 0}, dict(family="mmse_rank1", head=128)),
}


@pytest.mark.parametrize("name", list(KNOBS))
def test_estimate_knob_builds(gpu_wce, name):
    r, sem, B, knobs, named = KNOBS[name]
    estimate_law(gpu_wce, r, sem, B, knobs=knobs, **named)


@pytest.mark.parametrize("sem", ["C", "MATLAB"])
@pytest.mark.parametrize("request_", ["lt_ls+ps_linear", "lt_ls+ps_linear-light", "ls_family+eq"])
def test_estimate_ls_only(gpu_wce, request_, sem):
    """requests without PS_MMSE: ls_elem_kernel (C semantics; ls_kernel's light build in MATLAB semantics), the
    light ls_kernel by WCE_VARIANT_LS = 3, and all four LS estimators with the equalizer"""
    wce = gpu_wce
    mask = wce.LT_LS | wce.PS_LINEAR
    if request_ == "ls_family+eq":
        mask |= wce.PS_CUBIC | wce.PS_SINC | wce.EQUALIZE
    knobs = {LS: 3} if request_.endswith("light") else {}
    r = dict(mode="textbook")
    assert _planned(wce, r, sem, mask, knobs) == ["ls"]
    estimate_law(wce, r, sem, 67, mask=mask, knobs=knobs)


# ---------------------------------------------------------------- wce_mmse_solve, wce_mmse_apply
def test_mmse_solve_and_apply(gpu_wce):
    """a dense WCE_MMSE_COV context, 67 frames: W per frame from the solve, H per frame from the apply in its
    separate and its in-place form"""
    wce = gpu_wce
    B = 67
    a = dict(_estimate_args(B), Rhh=pdp_rhh(53, 0.12))
    c = wce.Context(a["ctx_tx_pre"], a["ctx_rx_pre"], a["ctx_ow2"], Rhh=a["Rhh"])
    assert c.lr_kernel(B) == "", "the dense path"

    def solve(x):
        n = x["tx"].shape[0]
        keep = [_dev(wce, tg._blocks(x["tx"])), _dev(wce, tg._blocks(x["rx"]))]
        W = _dev(wce, np.full((n, HS), SENT))
        c.mmse_solve(c.frames(keep[0], keep[1], n, frame_stride=FS, block_stride=BS), W, HS)
        wce.synchronize()
        return {"w": _unrows(W.numpy(), N, SENT, "w")}
    w = hold("mmse_solve", solve, a, B)["w"]
    assert np.isfinite(w.view(np.float64)).all()

    def apply(x, in_place):
        n = x["w"].shape[0]
        W = _dev(wce, _rows(x["w"], HS))
        H = W if in_place else _dev(wce, np.full((n, HS), SENT))
        c.mmse_apply(W, H, n, HS)
        wce.synchronize()
        if not in_place:
            assert np.array_equal(W.numpy(), _rows(x["w"], HS), equal_nan=True), "w: the input was written"
        return {"h": _unrows(H.numpy(), N, SENT, "h")}
    got = [hold("mmse_apply", lambda x: apply(x, p), dict(w=w), B)["h"] for p in (False, True)]
    assert gm.same_bits(got[0], got[1])
    c.close()


# ---------------------------------------------------------------- the front end
@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("form", ["plain", "cfo", "at"])
def test_front_end(gpu_wce, ctx, form, B):
    a = gm.first(gm.front_set(), B)
    hold("blocks", lambda x: tg.run_blocks(gpu_wce, ctx, x, form), a, B)
    base = hold("preamble", lambda x: tg.run_preamble(gpu_wce, ctx, x, form), a, B)
    assert np.all(base["ow2"] > 0)


@pytest.mark.parametrize("B", BATCHES)
def test_sync(gpu_wce, ctx, B):
    """tests/test_sync_gpu.py and test_stf_gpu.py permute a batch and run frames alone: the rotation and the
    poison here"""
    base = hold("sync", lambda x: tg.run_sync(gpu_wce, ctx, x), gm.first(gm.sync_set(), B), B, covered=True)
    assert (base["start"] >= 0).any()
    base = hold("sync_stf", lambda x: tg.run_sync_stf(gpu_wce, ctx, x), gm.first(gm.stf_set(), B), B, covered=True)
    assert (base["start"] >= 0).any()


@pytest.mark.parametrize("B", BATCHES)
def test_short_field(gpu_wce, ctx, B):
    def run(x):
        n = x["n_frames"]
        out = _dev(gpu_wce, np.full((n, 165), SENT))
        ctx.short_field(out, n, x["amplitude"], 165)
        gpu_wce.synchronize()
        return {"wave": _unrows(out.numpy(), 160, SENT, "wave")}
    hold("short_field", run, dict(amplitude=dm.SCALE, n_frames=B), B)


# ---------------------------------------------------------------- demodulators (rotation and poison), soft bits
@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("mod,rate,snr", gm.DEMOD_SETS)
def test_demodulate(gpu_wce, ctx, mod, rate, snr, B):
    a = gm.first(gm.demod_set(mod, rate, snr), B)
    base = hold("demodulate", lambda x: tg.run_demodulate(gpu_wce, ctx, x), a, B, covered=True)
    assert B == 5 or base["nerr"].sum() > 0, "a low-SNR set has symbol errors"


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("mod", dm.MODS)
def test_track_demodulate(gpu_wce, ctx, mod, B):
    hold("track", lambda x: tg.run_track(gpu_wce, ctx, x), gm.first(gm.track_set(mod), B), B, covered=True)


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("mod,rate,snr", gm.DEMOD_SETS)
def test_soft_demap(gpu_wce, ctx, mod, rate, snr, B):
    a = gm.first(gm.demap_set(mod, rate, snr), B)
    hold("soft_demap", lambda x: tg.run_demap(gpu_wce, ctx, x), a, B)
    hold("soft_demap_blocks", lambda x: tg.run_demap_blocks(gpu_wce, ctx, x), a, B)


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("terminated", [True, False])
@pytest.mark.parametrize("mod,rate", gm.DECODE_SETS)
def test_viterbi(gpu_wce, ctx, mod, rate, terminated, B):
    s = fm.integer_set(mod, rate)
    a = dict(llr=s["llr"][:B], u=s["u"][:B])
    base = hold("viterbi", lambda x: viterbi(gpu_wce, ctx, x["llr"], mod, rate, terminated, x["u"]), a, B)
    assert np.array_equal(base["bits"], fm.integer_model(mod, rate, terminated)[0][:B])


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("mod,rate,snr", gm.DEMOD_SETS)
def test_reencode(gpu_wce, ctx, mod, rate, snr, B):
    hold("reencode", lambda x: tg.run_reencode(gpu_wce, ctx, x), gm.first(gm.reencode_set(mod, rate, snr), B), B)


# ---------------------------------------------------------------- the PSDU
def _bytes(wce, a, stride):
    return _dev(wce, _rows(np.asarray(a, np.uint8), stride, SENT8))


def run_psdu_frame(wce, ctx, a):
    mod, rate, n = a["mod"], a["rate"], len(a["lengths"])
    mx, nby = pm.max_len(mod, rate), pm.nbytes(mod, rate)
    keep = [_bytes(wce, a["payload"], mx - 4 + 3), _dev(wce, a["lengths"]), _dev(wce, a["seeds"])]
    out = _dev(wce, np.full((n, nby + 3), SENT8, np.uint8))
    ctx.psdu_frame(keep[0], n, mod, rate, lengths=keep[1], seeds=keep[2], bits=out, payload_stride=mx - 4 + 3,
                   bits_stride=nby + 3)
    wce.synchronize()
    return {"bits": _unrows(out.numpy(), nby, SENT8, "bits")}


def run_psdu_deframe(wce, ctx, a):
    """psdu [n][max] with the sentinel wherever the call writes nothing (beyond L_f; a refused frame)"""
    mod, rate, n = a["mod"], a["rate"], len(a["lengths"])
    mx, nby = pm.max_len(mod, rate), pm.nbytes(mod, rate)
    keep = [_bytes(wce, a["bits"], nby + 3), _dev(wce, a["lengths"])]
    psdu = _dev(wce, np.full((n, mx + 3), fr.PSDU_SENT, np.uint8))
    seed, ok = _tail(wce, n, SENT8, np.uint8), _tail(wce, n, 0xA5A5A5A5, np.uint32)
    good = _dev(wce, np.array([5, 0xA5A5A5A5], np.uint32))
    ctx.psdu_deframe(keep[0], n, mod, rate, lengths=keep[1], psdu=psdu, seed=seed, fcs_ok=ok, n_good=good,
                     bits_stride=nby + 3, psdu_stride=mx + 3)
    wce.synchronize()
    g = good.numpy()
    assert g[1] == 0xA5A5A5A5, "n_good: written past the counter"
    return {"psdu": _unrows(psdu.numpy(), mx, fr.PSDU_SENT, "psdu"), "seed": _untail(seed, SENT8, "seed"),
            "fcs_ok": _untail(ok, 0xA5A5A5A5, "fcs_ok"), "n_good": np.array([g[0] - 5], np.uint32)}


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("mod,rate", gm.DECODE_SETS)
def test_psdu(gpu_wce, ctx, mod, rate, B):
    a = fr.psdu_frame_set(mod, rate, B)
    base = hold("psdu_frame", lambda x: run_psdu_frame(gpu_wce, ctx, x), a, B)
    assert np.array_equal(base["bits"], fr.psdu_frame_model(a)["bits"])
    a = fr.psdu_deframe_set(mod, rate, B)
    base = hold("psdu_deframe", lambda x: run_psdu_deframe(gpu_wce, ctx, x), a, B)
    want = fr.psdu_deframe_model(a)
    assert all(np.array_equal(base[n], want[n]) for n in want), "the base run is the model's"
    assert 0 < base["n_good"][0] < B


# ---------------------------------------------------------------- diversity
@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("weighted", [True, False])
def test_combine(gpu_wce, ctx, weighted, B):
    a = gm.first(gm.combine_set(), B, axis=1)
    hold("combine", lambda x: tg.run_combine(gpu_wce, ctx, x, weighted), a, B, covered=True)


@pytest.mark.parametrize("B", BATCHES)
def test_sync_share(gpu_wce, ctx, B):
    wce = gpu_wce
    A = 3
    metric, start, cfo = (np.ascontiguousarray(v[:, :B]) for v in cb.sync_share_set(A, 23 if B < 23 else B))

    def run(x):
        n = x["metric"].shape[1]
        keep = _dev(wce, _rows(x["metric"], n + 3, SENTD))
        s, c = _dev(wce, _rows(x["start"], n + 3, -77)), _dev(wce, _rows(x["cfo"], n + 3, SENTD))
        ctx.sync_share(keep, n, A, s, c, branch_stride=n + 3)
        wce.synchronize()
        return {"start": _unrows(s.numpy(), n, -77, "start"), "cfo": _unrows(c.numpy(), n, SENTD, "cfo")}
    a = dict(metric=metric, start=start, cfo=cfo)
    base = hold("sync_share", run, a, B)
    s, c = cb.sync_share(metric, start, cfo)
    assert np.array_equal(base["start"], s) and gm.same_bits(base["cfo"], c)


# ---------------------------------------------------------------- the transmit side
TX_CALLS = ("modulate", "channel", "transmit", "channel_tv", "transmit_tv")


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("call", TX_CALLS)
def test_transmit_side(gpu_wce, ctx, call, B):
    """moved with the noise off, windows with the noise on and first_frame raised by the window's start: "shards
    regenerate identical windows" (include/wce.h)"""
    a = dict(gm.first(gm.tx_set(), B), first_frame=3)
    a["wave"] = tg.run_tx(gpu_wce, ctx, a, "modulate")["wave"]
    row = fr.BY_KEY[call]
    if "sym" not in row.frame:       # run_tx takes the batch size and the wave's length from sym: it moves with the wave
        row = row._replace(frame=dict(row.frame, sym=0))

    base = hold(row, lambda x: tg.run_tx(gpu_wce, ctx, x, call), a, B)
    assert all(np.isfinite(v.view(np.float64)).all() for v in base.values())
    if call != "modulate":       # the noise was on: another first_frame gives other windows
        other = tg.run_tx(gpu_wce, ctx, dict(a, first_frame=4), call)
        assert not gm.same_bits(other["capture"], base["capture"])


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("shared", [False, True], ids=["own_taps", "h_shared"])
def test_synth_frames(gpu_wce, ctx, shared, B):
    wce = gpu_wce
    h = _dev(wce, np.exp(-0.2 * np.arange(N)) * np.exp(0.3j * np.arange(N))) if shared else None

    def run(x):
        n = x["n_frames"]
        tx, rx, pre = (_dev(wce, np.full((n, FS), SENT)), _dev(wce, np.full((n, FS), SENT)),
                       _dev(wce, np.full((n, HS), SENT)))
        ctx.synth(tx, rx, pre, n, first_frame=x["first_frame"], seed=x["seed"], h_shared=h, frame_stride=FS,
                  block_stride=BS, pre_stride=HS)
        wce.synchronize()
        return {"tx": _unblocks(tx.numpy(), NBLK, N, SENT, "tx"), "rx": _unblocks(rx.numpy(), NBLK, N, SENT, "rx"),
                "rx_pre": _unrows(pre.numpy(), N, SENT, "rx_pre")}
    a = dict(n_frames=B, first_frame=3, seed=0x6A26)
    base = hold("synth_frames", run, a, B)
    assert not gm.same_bits(base["rx"][1:], base["rx"][:-1]) and np.isfinite(base["rx"].view(np.float64)).all()


# ---------------------------------------------------------------- the guard
@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
def test_nonfinite_scan(gpu_wce, ctx, f32, B):
    """bit f moves with frame f, the bits past the batch stay 0, and the count is the sum"""
    wce = gpu_wce

    def run(x):
        n = x["H"].shape[0]
        words = (n + 31) // 32
        H = _dev(wce, _rows(x["H"], HS, x["H"].dtype.type(SENT)))
        bitmap = _dev(wce, np.full(words + 1, 0xA5A5A5A5, np.uint32))
        count = _dev(wce, np.array([77, 0xA5A5], np.uint64))
        ctx.nonfinite_scan(H, n, stride=HS, f32=f32, bitmap=bitmap, n_bad=count)
        wce.synchronize()
        bm, cnt = bitmap.numpy(), count.numpy()
        assert bm[-1] == 0xA5A5A5A5 and cnt[1] == 0xA5A5, "written past the end"
        bits = (bm[:words, None] >> np.arange(32, dtype=np.uint32)[None, :]) & 1
        bits = bits.reshape(-1).astype(np.uint8)
        assert not bits[n:].any(), "a bit past the batch is set"
        return {"bad": bits[:n], "n_bad": cnt[:1]}
    a = fr.scan_set(B)
    if f32:
        a = dict(H=a["H"].astype(np.complex64))
    base = hold("nonfinite_scan", run, a, B)
    assert np.array_equal(base["bad"], fr.scan_model(fr.scan_set(B))["bad"]) and 0 < base["n_bad"][0] < B
