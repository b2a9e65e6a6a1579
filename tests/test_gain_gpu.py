"""Signal level on the device: every row of tests/gain_model.py through the
library's calls.  The reference of a row is the same call at k = 0 in the same
process; the inputs moved by g = 2^k must move every output as the row says, bit
for bit (integers: equal).  Batches of 5 and 67 frames, every stride padded with
sentinels that must survive.  tests/test_gain_model.py has proved each row, at
each gain used here, on the numpy models.

On top of the rows, two chains: receive_capture_host on a capture times g (with
and without the short field), and two antenna branches whose captures carry the
gains 2^11 and 2^-11 through sync, front end, estimate, wce_combine, demodulate
and decode; and the soft bits' saturation at +-WCE_LLR_MAX.

Outputs held by tolerance instead of bit equality.  Only a library function
(atan2, hypot, a reciprocal seed) may put an output here, never an estimator
output, wce_estimate's eq, sym, start, bits or a wce_combine output; the bound
is the sum of the two bounds the call's own model test holds that output to
(two evaluations, each within its bound of the model):

    call    output    operation    bound
    (none: every output of every row is bit-equal)
"""
import contextlib
import functools

import numpy as np
import pytest

import combine_model as cb
import demod_model as dm
import fec_model as fm
import gain_model as gm
import tx_model as tm
from oracle_py import N, NBLK
from test_cov_lowrank_gpu import pdp_rhh
from test_decode_gpu import _within_bound, demap, viterbi

pytestmark = pytest.mark.gpu

TOLERANT = {}                        # law key -> {output: bound}; the table above
BATCHES = (5, 67)
BS, FS, HS = 56, 15 * 56 + 3, 56     # complex frames: block and frame stride; estimates: row stride
SENT, SENTD, SENTF, SENT8, SENT32 = 7.0 - 3.0j, 123.25, np.float32(-777.25), 0xA5, 0xDEAD
R1 = 5                               # WCE_VARIANT_R1


# ---------------------------------------------------------------- layouts
def _blocks(a, fill=SENT, dtype=np.complex128):
    """[B][nb][n <= BS] -> [B][nb BS + 3], the padding filled"""
    B, nb = a.shape[:2]
    out = np.full((B, nb * BS + 3), fill, dtype)
    for b in range(nb):
        out[:, b * BS:b * BS + a.shape[2]] = a[:, b]
    return out


def _unblocks(flat, nb, n, fill, what):
    mask = np.zeros(flat.shape[1], bool)
    for b in range(nb):
        mask[b * BS:b * BS + n] = True
    assert np.all(flat[:, ~mask] == fill), f"{what}: padding overwritten"
    return np.stack([flat[:, b * BS:b * BS + n] for b in range(nb)], axis=1)


def _rows(a, stride, fill=SENT):
    a = np.asarray(a)
    out = np.full(a.shape[:-1] + (stride,), fill, a.dtype)
    out[..., :a.shape[-1]] = a
    return out


def _unrows(flat, n, fill, what):
    assert np.all(flat[..., n:] == fill), f"{what}: padding overwritten"
    return np.ascontiguousarray(flat[..., :n])


def _tail(wce, B, fill, dtype):
    """a per-frame output one element longer than the batch"""
    return wce.DeviceArray.from_numpy(np.full(B + 1, fill, dtype))


def _untail(d, fill, what):
    a = d.numpy()
    assert a[-1] == fill, f"{what}: written past the batch"
    return a[:-1]


def _dev(wce, a):
    return None if a is None else wce.DeviceArray.from_numpy(np.ascontiguousarray(a))


@pytest.fixture(scope="module")
def ctx(gpu_wce):
    pre = tm.chain_pre()
    c = gpu_wce.Context(pre, pre, 1e-6, gpu_wce.MMSE_TEXTBOOK)
    yield c
    c.close()


def hold(law, run, args, narrow=False, names=None):
    """the row at every gain it may use, against the k = 0 run"""
    law = gm.BY_KEY[law] if isinstance(law, str) else law
    base = run(args)
    for k in gm.gains(law, narrow):
        kk = gm.branch_gains(k, gm.COMBINE_A) if law.branch else k
        bad = gm.check(law, run, args, kk, names, TOLERANT.get(law.key), base)
        assert not bad, f"{law.key}: at g = 2^{k} these outputs do not follow the law: {bad}"
    return base


# ---------------------------------------------------------------- front end
def run_blocks(wce, ctx, a, form):
    B, L = a["samples"].shape
    d = _dev(wce, _rows(a["samples"], L + 5))
    out = _dev(wce, np.full((B, FS), SENT))
    kw = dict(packet_stride=L + 5, frame_stride=FS, block_stride=BS)
    keep = [_dev(wce, a["eps"]), _dev(wce, a["start"])]
    if form == "plain":
        ctx.front_end_blocks(d, B, NBLK, out, **kw)
    elif form == "cfo":
        ctx.front_end_blocks(d, B, NBLK, out, cfo=keep[0], sample_offset=3, **kw)
    else:
        ctx.front_end_blocks(d, B, NBLK, out, cfo=keep[0], sample_offset=3, start=keep[1], capture_len=L, **kw)
    wce.synchronize()
    return {"sym": _unblocks(out.numpy(), NBLK, N, SENT, "sym")}


def run_preamble(wce, ctx, a, form):
    B, L = a["lptot"].shape
    d = _dev(wce, _rows(a["lptot"], L + 5))
    pre, ow2, cfo = _dev(wce, np.full((B, HS), SENT)), _tail(wce, B, SENTD, np.float64), _tail(wce, B, SENTD, np.float64)
    kw = dict(lptot_stride=L + 5, pre_stride=HS)
    start = _dev(wce, (a["start"] % (L - 127)).astype(np.int32))
    if form == "plain":
        ctx.front_end_preamble(d, B, L, pre, ow2, **kw)
    elif form == "cfo":
        ctx.front_end_preamble(d, B, L, pre, ow2, cfo=cfo, **kw)
    else:
        ctx.front_end_preamble(d, B, L, pre, ow2, cfo=cfo, start=start, **kw)
    wce.synchronize()
    out = {"pre_fft": _unrows(pre.numpy(), N, SENT, "pre_fft"), "ow2": _untail(ow2, SENTD, "ow2")}
    if form != "plain":
        out["cfo"] = _untail(cfo, SENTD, "cfo")
    return out


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("form", ["plain", "cfo", "at"])
def test_front_end(gpu_wce, ctx, form, B):
    a = gm.first(gm.front_set(), B)
    hold("blocks", lambda x: run_blocks(gpu_wce, ctx, x, form), a)
    base = hold("preamble", lambda x: run_preamble(gpu_wce, ctx, x, form), a)
    assert np.all(base["ow2"] > 0)


def run_sync(wce, ctx, a):
    B, L = a["capture"].shape
    d, dl = _dev(wce, _rows(a["capture"], L + 5)), _dev(wce, a["ltf"])
    s, m = _tail(wce, B, -77, np.int32), _tail(wce, B, SENTD, np.float64)
    ctx.front_end_sync(d, B, L, dl, a["threshold"], 0, s, m, capture_stride=L + 5)
    wce.synchronize()
    return {"start": _untail(s, -77, "start"), "metric": _untail(m, SENTD, "metric")}


def run_sync_stf(wce, ctx, a):
    B, L = a["capture"].shape
    d, dl = _dev(wce, _rows(a["capture"], L + 5)), _dev(wce, a["ltf"])
    s = _tail(wce, B, -77, np.int32)
    o = {n: _tail(wce, B, SENTD, np.float64) for n in ("cfo", "metric_stf", "metric_ltf")}
    ctx.front_end_sync_stf(d, B, L, dl, a["threshold_stf"], a["threshold_ltf"], 0, s, o["cfo"], o["metric_stf"],
                           o["metric_ltf"], capture_stride=L + 5)
    wce.synchronize()
    return {"start": _untail(s, -77, "start"), **{n: _untail(v, SENTD, n) for n, v in o.items()}}


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("which", ["capture", "ltf"])
def test_sync(gpu_wce, ctx, which, B):
    base = hold("sync/" + which, lambda x: run_sync(gpu_wce, ctx, x), gm.first(gm.sync_set(), B))
    assert (base["start"] >= 0).any()
    base = hold("sync_stf/" + which, lambda x: run_sync_stf(gpu_wce, ctx, x), gm.first(gm.stf_set(), B))
    assert (base["start"] >= 0).any() and (B == 5 or (base["start"] < 0).any())


# ---------------------------------------------------------------- the estimators, route by route
# name -> what makes the route (wce.debug_route's facts: mode, border dot, fusion, constant modulus, the low-rank
# kernel and rank, the request, fp32 storage, the rank-1 variant, FRAME_COV, per-frame noise)
ROUTES = {
    "ref": dict(mode="ref"),
    "ref-bdot_off-frame_cov": dict(mode="ref", bdot=False, fc=True),
    "ref-unfused": dict(mode="ref", fuse=False),
    "textbook": dict(mode="textbook"),
    "textbook-mmse_only": dict(mode="textbook", mmse_only=True),
    "textbook-factorised": dict(mode="textbook", variant=1),
    "textbook-f32": dict(mode="textbook", f32=True),
    "frame_cov": dict(mode="textbook", fc=True),
    "frame_cov-noise": dict(mode="textbook", fc=True, noise=True),
    "frame_cov-noise-f32": dict(mode="textbook", fc=True, noise=True, f32=True),
    "cov-rank4": dict(mode="cov", rhh=(4, 0.5)),
    "cov-rank12": dict(mode="cov", rhh=(12, 0.5)),
    "cov-rank24": dict(mode="cov", rhh=(24, 0.3)),
    "cov-rank53-dense": dict(mode="cov", rhh=(53, 0.12)),
    "cov-rank53-gram": dict(mode="cov", rhh=(53, 0.5)),
    "cov-rank12-f32": dict(mode="cov", rhh=(12, 0.5), f32=True),
    "cov-rank12-constant_modulus": dict(mode="cov", rhh=(12, 0.5), cm=True),
    "cov-rank53-constant_modulus": dict(mode="cov", rhh=(53, 0.12), cm=True),
}
EST = ("lt_ls", "ps_linear", "ps_cubic", "ps_sinc", "ps_mmse")


@functools.lru_cache(maxsize=None)
def _estimate_set(B):
    """B frames around the recorded inputs.h frame (BPSK: constant modulus) with noise of its own variance on the
    symbols and on each frame's preamble, and each frame's own ow2"""
    g = dict(np.load(gm.HEADER.replace("include/wce.h", "tests/golden/inputs_h.npz")))
    rng = np.random.default_rng(0x6A19)
    amp = np.sqrt(g["ow2"] / 2)
    noise = lambda shape: amp * (rng.standard_normal(shape) + 1j * rng.standard_normal(shape))
    tx = np.repeat(g["tx_symb"][None], B, axis=0)
    return dict(tx=tx, rx=np.repeat(g["rx_symb"][None], B, axis=0) + noise(tx.shape),
                rx_pre=g["rx_pre"][None] + noise((B, N)), tx_pre=np.array(g["tx_pre"], np.complex128),
                ctx_tx_pre=np.array(g["tx_pre"], np.complex128), ctx_rx_pre=np.array(g["rx_pre"], np.complex128),
                ctx_ow2=float(g["ow2"]), ow2=float(g["ow2"]) * rng.uniform(0.5, 2.0, B),
                x_ref=np.array(g["tx_symb"][0], np.complex128))


VARIANT_DEFAULT = {1: 2}             # wce_debug_set_variant: WCE_VARIANT_LS starts at 2, every other knob at 0


@contextlib.contextmanager
def _variant(wce, v, knobs=None):
    """WCE_VARIANT_R1 = v, and every further knob of `knobs` (which -> value), for one call"""
    lib = wce.load()
    knobs = dict(knobs or {})
    knobs.setdefault(R1, v)
    try:
        for which, value in knobs.items():
            assert lib.wce_debug_set_variant(which, value) == 0
        yield
    finally:
        for which in knobs:
            assert lib.wce_debug_set_variant(which, VARIANT_DEFAULT.get(which, 0)) == 0


def run_estimate(wce, a, route, sem, mask=None, knobs=None, probe=None):
    """a context of the route from the (scaled) preamble, noise variance and covariance, then one estimate call.
    mask: the request (the route's own where None); knobs: further wce_debug_set_variant settings for the call
    (which -> value); probe(ctx, units): called under the knobs before the launch, to name the kernel; a route
    may be given as its dict of facts"""
    r = ROUTES[route] if isinstance(route, str) else route
    B = a["tx"].shape[0]
    mode = {"ref": wce.MMSE_REF, "textbook": wce.MMSE_TEXTBOOK, "cov": None}[r["mode"]]
    if r["mode"] == "cov":
        c = wce.Context(a["ctx_tx_pre"], a["ctx_rx_pre"], a["ctx_ow2"], Rhh=a["Rhh"])
        assert c.cov_info()[0] == r["rhh"][0], "the rank does not move with the level"
        if r.get("cm"):
            c.set_modulus(a["x_ref"])
    else:
        c = wce.Context(a["ctx_tx_pre"], a["ctx_rx_pre"], a["ctx_ow2"], mode)
    c.set_border_dot(r.get("bdot", True))
    c.set_fusion(r.get("fuse", True))
    f32 = bool(r.get("f32"))
    lsdt = np.complex64 if f32 else np.complex128
    sent = lsdt(SENT)
    if mask is None:
        mask = wce.PS_MMSE if r.get("mmse_only") else wce.ALL
    names = [n for n, bit in zip(EST, (wce.LT_LS, wce.PS_LINEAR, wce.PS_CUBIC, wce.PS_SINC, wce.PS_MMSE)) if mask & bit]
    bufs = {n: _dev(wce, np.full((B, HS), SENT, np.complex128 if n == "ps_mmse" else lsdt)) for n in names}
    deq = _dev(wce, np.full((B, FS), sent, lsdt)) if mask & wce.EQUALIZE else None
    o = wce.Outputs(*[(bufs[n].addr if n in bufs else None) for n in EST], deq.addr if deq is not None else None,
                    HS, FS, BS, wce.PS_LINEAR, wce.OUT_LS_F32 if f32 else 0)
    keep = [_dev(wce, _blocks(a["tx"])), _dev(wce, _blocks(a["rx"])), _dev(wce, _rows(a["rx_pre"], HS)),
            _dev(wce, a["tx_pre"]), _dev(wce, a["ow2"]) if r.get("noise") else None]
    fr = c.frames(keep[0], keep[1], B, frame_stride=FS, block_stride=BS, rx_pre=keep[2], pre_stride=HS,
                  tx_pre=keep[3], block=0, semantics=wce.SEM_MATLAB if sem == "MATLAB" else wce.SEM_C)
    with _variant(wce, r.get("variant", 0), knobs):
        if probe is not None:
            probe(c, B * (4 if sem == "MATLAB" else 1))
        c.estimate(fr, o, mask | (wce.FRAME_COV if r.get("fc") else 0), ow2=keep[4])
        wce.synchronize()
    out = {n: _unrows(d.numpy(), N, sent if n != "ps_mmse" else SENT, n) for n, d in bufs.items()}
    if deq is not None:
        out["eq"] = _unblocks(deq.numpy(), NBLK, N, sent, "eq")
    c.close()
    return out


@pytest.mark.parametrize("sem", ["C", "MATLAB"])
@pytest.mark.parametrize("route", list(ROUTES))
def test_estimate(gpu_wce, route, sem):
    """both laws on one route: 67 frames in C semantics, 5 in MATLAB semantics"""
    a = dict(_estimate_set(67 if sem == "C" else 5), Rhh=None)
    r = ROUTES[route]
    if r["mode"] == "cov":
        a["Rhh"] = pdp_rhh(*r["rhh"])
    for law in ("estimate/channel", "estimate/tx"):
        base = hold(law, lambda x: run_estimate(gpu_wce, x, route, sem), a, narrow=bool(r.get("f32")))
        assert all(np.isfinite(v.view(v.real.dtype)).all() for v in base.values())


# ---------------------------------------------------------------- demodulators
def _frames(wce, ctx, a, B):
    keep = [_dev(wce, _blocks(a["tx"])), _dev(wce, _blocks(a["rx"]))]
    return ctx.frames(keep[0], keep[1], B, frame_stride=FS, block_stride=BS), keep


def _demod_outputs(wce, B, tracked):
    o = dict(eq=_dev(wce, np.full((B, FS), SENT)), sym=_dev(wce, np.full((B, FS), SENT8, np.uint8)),
             theta=_dev(wce, np.full((B + 1, NBLK), SENTD)), evm=_tail(wce, B, SENTD, np.float64),
             nerr=_tail(wce, B, SENT32, np.uint32))
    if tracked:
        o.update(h_blocks=_dev(wce, np.full((B, FS), SENT)), h_last=_dev(wce, np.full((B, HS), SENT)))
    return o


def _demod_results(o):
    out = {"eq": _unblocks(o["eq"].numpy(), NBLK, N, SENT, "eq"),
           "sym": _unblocks(o["sym"].numpy(), NBLK, N, SENT8, "sym"),
           "evm": _untail(o["evm"], SENTD, "evm"), "nerr": _untail(o["nerr"], SENT32, "nerr")}
    th = o["theta"].numpy()
    assert np.all(th[-1] == SENTD), "theta: written past the batch"
    out["theta"] = th[:-1]
    if "h_blocks" in o:
        out["h_blocks"] = _unblocks(o["h_blocks"].numpy(), NBLK, N, SENT, "h_blocks")
        out["h_last"] = _unrows(o["h_last"].numpy(), N, SENT, "h_last")
    return out


def run_demodulate(wce, ctx, a):
    B = a["tx"].shape[0]
    fr, keep = _frames(wce, ctx, a, B)
    dh, dhl = _dev(wce, _rows(a["h"], HS)), _dev(wce, _rows(a["h_lt"], HS))
    o = _demod_outputs(wce, B, False)
    ctx.demodulate(fr, dh, dhl, HS, a["mod"], a["scale"], eq_frame_stride=FS, eq_block_stride=BS,
                   sym_frame_stride=FS, sym_block_stride=BS, **o)
    wce.synchronize()
    return _demod_results(o)


def run_track(wce, ctx, a):
    B = a["tx"].shape[0]
    fr, keep = _frames(wce, ctx, a, B)
    dh = _dev(wce, _rows(a["h"], HS))
    o = _demod_outputs(wce, B, True)
    ctx.track_demodulate(fr, dh, 0.5, 2, HS, a["mod"], a["scale"], eq_frame_stride=FS, eq_block_stride=BS,
                         sym_frame_stride=FS, sym_block_stride=BS, hb_frame_stride=FS, hb_block_stride=BS,
                         h_last_stride=HS, **o)
    wce.synchronize()
    return _demod_results(o)


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("mod,rate,snr", gm.DEMOD_SETS)
def test_demodulate(gpu_wce, ctx, mod, rate, snr, B):
    a = gm.first(gm.demod_set(mod, rate, snr), B)
    for law in ("demodulate/channel", "demodulate/tx"):
        base = hold(law, lambda x: run_demodulate(gpu_wce, ctx, x), a)
    assert base["nerr"].sum() > 0, "a low-SNR set has symbol errors"


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("mod", dm.MODS)
def test_track_demodulate(gpu_wce, ctx, mod, B):
    a = gm.first(gm.track_set(mod), B)
    for law in ("track/channel", "track/tx"):
        hold(law, lambda x: run_track(gpu_wce, ctx, x), a)


# ---------------------------------------------------------------- soft bits, decoder
def run_demap_blocks(wce, ctx, a):
    B, mod = a["eq"].shape[0], a["mod"]
    lbs = 48 * mod + 5
    lfs = 15 * lbs + 7
    keep = [_dev(wce, _blocks(a["eq"])), _dev(wce, _blocks(a["hb"]))]
    dl = _dev(wce, np.full((B, lfs), SENTF, np.float32))
    ctx.soft_demap_blocks(keep[0], keep[1], B, mod, a["scale"], dl, eq_frame_stride=FS, eq_block_stride=BS,
                          hb_frame_stride=FS, hb_block_stride=BS, llr_frame_stride=lfs, llr_block_stride=lbs)
    wce.synchronize()
    flat = dl.numpy()
    mask = np.zeros(lfs, bool)
    for b in range(NBLK):
        mask[b * lbs:b * lbs + 48 * mod] = True
    assert np.all(flat[:, ~mask] == SENTF), "llr: padding overwritten"
    return {"llr": np.stack([flat[:, b * lbs:b * lbs + 48 * mod] for b in range(NBLK)], axis=1)}


def run_demap(wce, ctx, a):
    """test_decode_gpu's padded call, with the set's scale"""
    B, mod = a["eq"].shape[0], a["mod"]
    lbs = 48 * mod + 5
    lfs = 15 * lbs + 7
    keep = [_dev(wce, _blocks(a["eq"])), _dev(wce, _rows(a["h"], HS)), _dev(wce, _rows(a["h_lt"], HS))]
    dl = _dev(wce, np.full((B, lfs), SENTF, np.float32))
    ctx.soft_demap(keep[0], keep[1], B, h_lt=keep[2], h_stride=HS, modulation=mod, scale=a["scale"], llr=dl,
                   eq_frame_stride=FS, eq_block_stride=BS, llr_frame_stride=lfs, llr_block_stride=lbs)
    wce.synchronize()
    flat = dl.numpy()
    mask = np.zeros(lfs, bool)
    for b in range(NBLK):
        mask[b * lbs:b * lbs + 48 * mod] = True
    assert np.all(flat[:, ~mask] == SENTF), "llr: padding overwritten"
    return {"llr": np.stack([flat[:, b * lbs:b * lbs + 48 * mod] for b in range(NBLK)], axis=1)}


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("mod,rate,snr", gm.DEMOD_SETS)
def test_soft_demap(gpu_wce, ctx, mod, rate, snr, B):
    a = gm.first(gm.demap_set(mod, rate, snr), B)
    for call, run in (("soft_demap", run_demap), ("soft_demap_blocks", run_demap_blocks)):
        for way in ("channel", "tx"):
            base = hold(f"{call}/{way}", lambda x: run(gpu_wce, ctx, x), a)
            assert gm.normal(base["llr"].astype(np.float64) * 2.0 ** 80, np.float32)
            assert gm.normal(base["llr"].astype(np.float64) * 2.0 ** -80, np.float32)


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("mod,rate", gm.DECODE_SETS)
def test_viterbi(gpu_wce, ctx, mod, rate, B):
    s = fm.integer_set(mod, rate)
    a = dict(llr=s["llr"][:B], u=s["u"][:B])
    for terminated in (True, False):
        base = hold("viterbi", lambda x: viterbi(gpu_wce, ctx, x["llr"], mod, rate, terminated, x["u"]), a)
        assert np.array_equal(base["bits"], fm.integer_model(mod, rate, terminated)[0][:B])


# ---------------------------------------------------------------- re-encoder
def run_reencode(wce, ctx, a):
    B, mod, rate = a["u"].shape[0], a["mod"], a["rate"]
    nby = (a["u"].shape[1] + 7) // 8
    packed = np.full((B, nby + 3), SENT8, np.uint8)
    packed[:, :nby] = fm.pack(a["u"])
    tx = np.full((B, NBLK, N), np.nan + 1j * np.nan)      # nothing but the pilots is read
    tx[:, :, list(dm.PILOTS)] = a["pilots"]
    keep = [_dev(wce, packed), _dev(wce, _blocks(tx, np.nan)), _dev(wce, _blocks(a["rx"], np.nan)), _dev(wce, a["theta"])]
    fr = ctx.frames(keep[1], keep[2], B, frame_stride=FS, block_stride=BS)
    dx, dh = _dev(wce, np.full((B, FS), SENT)), _dev(wce, np.full((B, HS), SENT))
    ctx.reencode(keep[0], B, mod, rate, a["scale"], bits_stride=nby + 3, theta=keep[3], frames=fr, tx=dx,
                 tx_frame_stride=FS, tx_block_stride=BS, h=dh, h_stride=HS)
    wce.synchronize()
    return {"tx": _unblocks(dx.numpy(), NBLK, N, SENT, "tx"), "h": _unrows(dh.numpy(), N, SENT, "h")}


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("mod,rate,snr", gm.DEMOD_SETS)
def test_reencode(gpu_wce, ctx, mod, rate, snr, B):
    a = gm.first(gm.reencode_set(mod, rate, snr), B)
    for law in ("reencode/channel", "reencode/tx"):
        hold(law, lambda x: run_reencode(gpu_wce, ctx, x), a)


# ---------------------------------------------------------------- diversity
def run_combine(wce, ctx, a, weighted=True):
    A, B = a["h"].shape[:2]
    rx = np.stack([_blocks(a["rx"][i]) for i in range(A)])                 # [A][B][FS]
    rx = _rows(rx.reshape(A, B * FS), B * FS + 11)                          # a gap between the branches
    h = _rows(_rows(a["h"], HS).reshape(A, B * HS), B * HS + 5)
    ow2 = _rows(a["ow2"], B + 3, SENTD)
    keep = [_dev(wce, rx), _dev(wce, h), _dev(wce, ow2) if weighted else None]
    drx, dh = _dev(wce, np.full((B, FS), SENT)), _dev(wce, np.full((B, HS), SENT))
    ctx.combine(keep[0], keep[1], B, A, keep[2], drx, dh, rx_branch_stride=B * FS + 11, rx_frame_stride=FS,
                rx_block_stride=BS, h_branch_stride=B * HS + 5, h_stride=HS, ow2_branch_stride=B + 3,
                out_frame_stride=FS, out_block_stride=BS, out_h_stride=HS)
    wce.synchronize()
    return {"rx_c": _unblocks(drx.numpy(), NBLK, N, SENT, "rx_c"), "h_c": _unrows(dh.numpy(), N, SENT, "h_c")}


@pytest.mark.parametrize("B", BATCHES)
def test_combine(gpu_wce, ctx, B):
    a = gm.first(gm.combine_set(), B, axis=1)
    run = lambda x: run_combine(gpu_wce, ctx, x)
    base = hold("combine/weighted", run, a)        # each branch its own gain: +k, -k, +k
    # include/wce.h: "A common factor on every ow2 changes no equalized symbol rx_c / h_c"
    for c in (4.0, 2.0 ** -40, 2.0 ** 40):
        r = run(dict(a, ow2=a["ow2"] * c))
        with np.errstate(invalid="ignore", divide="ignore"):
            assert gm.same_bits(r["rx_c"] / r["h_c"][:, None, :], base["rx_c"] / base["h_c"][:, None, :]), c
    hold("combine/unweighted", lambda x: run_combine(gpu_wce, ctx, x, False), a)


# ---------------------------------------------------------------- the transmit side
def _sym_kw(wce, a):
    B, nb = a["sym"].shape[:2]
    keep = [_dev(wce, _blocks(a["sym"])), _dev(wce, _rows(a["tx_pre"], HS))]
    return dict(n_blocks=nb, tx_pre=keep[1], pre_stride=HS, frame_stride=nb * BS + 3, block_stride=BS), keep


def _chan_kw(wce, a, taps=True):
    B = a["sym"].shape[0]
    nt = a["taps"].shape[-1]
    keep = [_dev(wce, _rows(a["taps"], nt + 1)), _dev(wce, a["cfo"]), _dev(wce, a["ow2"]), _dev(wce, a["delay"])]
    kw = dict(cfo=keep[1], ow2=keep[2], delay=keep[3], seed=a["seed"], first_frame=a.get("first_frame", 3))
    if taps:
        kw.update(taps=keep[0], n_taps=nt, taps_stride=nt + 1)
    return kw, keep


def _knot_kw(wce, a):
    B, K, nt = a["knots"].shape
    ks, kfs = nt + 1, K * (nt + 1) + 2
    flat = np.full((B, kfs), SENT)
    for k in range(K):
        flat[:, k * ks:k * ks + nt] = a["knots"][:, k]
    d = _dev(wce, flat)
    return dict(knots=d, n_knots=K, knot_period=80, n_taps=nt, knot_stride=ks, knots_frame_stride=kfs), d


def run_tx(wce, ctx, a, call):
    B, L = a["sym"].shape[0], a["capture_len"]
    S = 160 + 80 * a["sym"].shape[1]
    skw, k1 = _sym_kw(wce, a)
    if call == "modulate":
        out = _dev(wce, np.full((B, S + 5), SENT))
        ctx.modulate(k1[0], B, out, wave_stride=S + 5, **skw)
        wce.synchronize()
        return {"wave": _unrows(out.numpy(), S, SENT, "wave")}
    ckw, k2 = _chan_kw(wce, a, taps=not call.endswith("_tv"))
    kkw, k3 = _knot_kw(wce, a) if call.endswith("_tv") else ({}, None)
    out = _dev(wce, np.full((B, L + 3), SENT))
    if call.startswith("channel"):
        dw = _dev(wce, _rows(a["wave"], S + 2))
        getattr(ctx, call)(dw, B, S, out, L, field=True, wave_stride=S + 2, capture_stride=L + 3, **ckw, **kkw)
    else:
        getattr(ctx, call)(k1[0], B, out, L, capture_stride=L + 3, **skw, **ckw, **kkw)
    wce.synchronize()
    return {"capture": _unrows(out.numpy(), L, SENT, "capture")}


TX_ROWS = [("modulate", "modulate"), ("channel/taps", "channel"), ("channel/wave", "channel"),
           ("transmit/taps", "transmit"), ("transmit/sym", "transmit"), ("channel_tv/knots", "channel_tv"),
           ("transmit_tv/knots", "transmit_tv"), ("transmit_tv/sym", "transmit_tv")]


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("law,call", TX_ROWS, ids=[r[0] for r in TX_ROWS])
def test_transmit_side(gpu_wce, ctx, law, call, B):
    a = gm.first(gm.tx_set(), B)
    a["wave"] = run_tx(gpu_wce, ctx, a, "modulate")["wave"]
    base = hold(law, lambda x: run_tx(gpu_wce, ctx, x, call), a)
    assert all(np.isfinite(v.view(np.float64)).all() for v in base.values())


@pytest.mark.parametrize("B", BATCHES)
def test_short_field(gpu_wce, ctx, B):
    def run(x):
        out = _dev(gpu_wce, np.full((B, 165), SENT))
        ctx.short_field(out, B, x["amplitude"], 165)
        gpu_wce.synchronize()
        return {"wave": _unrows(out.numpy(), 160, SENT, "wave")}
    hold("short_field", run, dict(amplitude=dm.SCALE))


# ---------------------------------------------------------------- chain 1: a capture at another level
CHAIN_MOD, CHAIN_RATE, CHAIN_SNR, CHAIN_B = dm.QPSK, fm.RATE_1_2, 8.0, 5


@pytest.mark.parametrize("stf", [False, True], ids=["ltf", "stf"])
def test_capture_chain(gpu_wce, ctx, stf):
    """receive_capture_host on a capture times g, the context built from the preamble at that level: the k = 0
    run's start, symbols, bits and error counts"""
    wce = gpu_wce
    rng = np.random.default_rng(0x6A20 + stf)
    B, pre = CHAIN_B, tm.chain_pre()
    u = fm.random_info(rng, B, CHAIN_MOD, CHAIN_RATE)
    tx = fm.transmit(u, CHAIN_MOD, CHAIN_RATE)[0]
    ow2 = float(tm.nominal_ow2(CHAIN_SNR))
    cap = ctx.transmit_host(tx, pre, tm.random_taps(rng, B, 6), cfo=0.002, ow2=ow2,
                            delay=np.array([0, 37, 100, 123, 64], np.int32), capture_len=1648, stf=stf)
    tx_pk = np.asarray(tm.modulate(tx, None, np.float64), np.complex128)
    tx_lp = np.asarray(tm.modulate(np.zeros((B, 0, N)), pre, np.float64), np.complex128)

    def run(k):
        g = 2.0 ** k
        c = wce.Context(pre, pre * g, ow2 * g * g, wce.MMSE_TEXTBOOK)
        out = c.receive_capture_host(tx_pk, tx_lp, gm.times(cap, 1, k), 0.25, cfo=True, demod_source=wce.PS_MMSE,
                                     modulation=CHAIN_MOD, stf=stf, decode_rate=CHAIN_RATE, ref_bits=u)
        c.close()
        return out
    base = run(0)
    assert np.all(base["start"] >= 0) and base["demod"]["nerr"].sum() > 0, "detected, and hard enough to err"
    for k in gm.GAINS:
        out = run(k)
        assert np.array_equal(out["start"], base["start"]), k
        assert np.array_equal(out["demod"]["sym"], base["demod"]["sym"]), k
        assert np.array_equal(out["demod"]["nerr"], base["demod"]["nerr"]), k
        assert np.array_equal(out["decode"]["bits"], base["decode"]["bits"]), k
        assert np.array_equal(out["decode"]["nbiterr"], base["decode"]["nbiterr"]), k
        # and the fp64 outputs on the way follow their rows
        for n in EST:
            assert gm.same_bits(out[n], gm.times(base[n], 1, k)), (k, n)
        assert gm.same_bits(out["ow2"], gm.times(base["ow2"], 2, k)), k
        assert gm.same_bits(out["demod"]["eq"], base["demod"]["eq"]), k
        assert gm.same_bits(out["decode"]["llr"], gm.times(base["decode"]["llr"], 2, k)), k


# ---------------------------------------------------------------- chain 2: two antennas, two AGCs
def _mrc_receive(wce, ctx, cap, dtx, mod, rate, u):
    """Context.link_mrc_host's receiver on given captures cap [A][B][L] (LT_LS, shared sync, weighted by the
    front end's ow2): sync, sync_share, the _at front end, estimate, combine, demodulate, soft_demap, decode"""
    A, B, L = cap.shape
    n = A * B
    D = wce.DeviceArray
    dcap, dpre = _dev(wce, cap.reshape(n, L)), _dev(wce, ctx.tx_pre)
    dfield = D((160,), zero=True)
    ctx.modulate(None, 1, dfield, 0, dpre)
    dstart, dmetric = D((n,), np.int32, zero=True), D((n,), np.float64, zero=True)
    dow2, dcfo = D((n,), np.float64, zero=True), D((n,), np.float64, zero=True)
    drx, drxpre, dh = D((n, NBLK, N), zero=True), D((n, N), zero=True), D((n, N), zero=True)
    ctx.front_end_sync(dcap, n, L, dfield.addr + 32 * 16, 0.25, 0, dstart, dmetric)
    ctx.sync_share(dmetric, B, A, dstart, None)
    ctx.front_end_preamble(dcap, n, L, drxpre, dow2, cfo=dcfo, start=dstart)
    ctx.sync_share(dmetric, B, A, None, dcfo)
    ctx.front_end_preamble(dcap, n, L, drxpre, dow2, cfo=dcfo, estimate_cfo=False, start=dstart)
    ctx.front_end_blocks(dcap, n, NBLK, drx, cfo=dcfo, start=dstart, capture_len=L)
    o = wce.Outputs(dh.addr, None, None, None, None, None, N, NBLK * N, N, wce.PS_LINEAR, 0)
    ctx.estimate(ctx.frames(dtx, drx, n, rx_pre=drxpre, tx_pre=dpre), o, wce.LT_LS)
    drxc, dhc = D((B, NBLK, N), zero=True), D((B, N), zero=True)
    ctx.combine(drx, dh, B, A, dow2, drxc, dhc)
    dem = ctx._demod_device(ctx.frames(dtx, drxc, B), B, dhc, None, mod, dm.SCALE, True, True)
    dec = ctx._decode_device(dem["eq"], dhc, None, B, mod, rate, dm.SCALE, True, u)
    wce.synchronize()
    res = ctx._decode_result(dec, mod, rate)
    return dict(rx_c=drxc.numpy(), h_c=dhc.numpy(), bits=res["bits"], nbiterr=res["nbiterr"], sym=dem["sym"].numpy(),
                start=dstart.numpy(), ow2=dow2.numpy().reshape(A, B), h=dh.numpy().reshape(A, B, N))


def _mrc_sym(wce, dtx, B):
    """the labels of the transmitted symbols"""
    return dm.slice_points(dtx.numpy()[:B], cb.LINK_MOD, dm.SCALE, np.float64)[0]


def test_diversity_chain(gpu_wce, ctx):
    """two branches whose captures carry the gains 2^11 and 2^-11 (and 2^40, 2^-40): rx_c, h_c and the bits of
    the equal-gain run"""
    wce = gpu_wce
    A, B, mod, rate = 2, 5, cb.LINK_MOD, cb.LINK_RATE
    taps = wce.pdp_taps(np.random.default_rng(0x6A21), A * B, np.exp(-np.arange(6.0))).reshape(A, B, 6)
    res = ctx.link_mrc_host(mod, rate, 12.0, B, A, taps, sources=(wce.LT_LS,), branch_loss_db=[0.0, 3.0], cfo=0.001,
                            delay=np.array([0, 37, 100, 5, 64], np.int32), keep_capture=True)
    cap, u = res["capture"], res["bits"]
    dtx = wce.DeviceArray((A * B, NBLK, N), zero=True)     # the same symbols once per branch
    ctx.reencode(_dev(wce, fm.pack(np.tile(u, (A, 1)))), A * B, mod, rate, dm.SCALE, tx=dtx)
    base = _mrc_receive(wce, ctx, cap, dtx, mod, rate, u)
    assert np.all(base["start"] >= 0) and np.array_equal(base["nbiterr"], res[wce.LT_LS]["combined"])
    assert (base["sym"] != _mrc_sym(wce, dtx, B)).any(), "hard enough to err"
    for k in (11, 40):
        kk = np.array([k, -k])
        out = _mrc_receive(wce, ctx, gm.times(cap, 1, kk), dtx, mod, rate, u)
        for n in ("start", "sym", "bits", "nbiterr"):
            assert np.array_equal(out[n], base[n]), (k, n)
        assert gm.same_bits(out["h"], gm.times(base["h"], 1, kk)), k
        assert gm.same_bits(out["ow2"], gm.times(base["ow2"], 2, kk)), k
        assert gm.same_bits(out["rx_c"], base["rx_c"]) and gm.same_bits(out["h_c"], base["h_c"]), k


# ---------------------------------------------------------------- soft bits beyond float: saturate, not erase
@pytest.mark.parametrize("mod,rate", [(dm.BPSK, fm.RATE_1_2), (dm.QAM16, fm.RATE_1_2), (dm.QAM64, fm.RATE_3_4)])
def test_soft_bits_saturate(gpu_wce, mod, rate):
    """h times 2^45 (some soft bits clamp) and 2^60 (all do): finite, the sign of the k = 0 soft bit, the model's
    clamped value within bound (c), and decoded exactly as the model decodes its clamped soft bits.  The
    unclamped demapper wrote +-Inf at 2^60 for every soft bit of 2^7 and more at k = 0, the most reliable ones,
    which the decoder reads as erasures"""
    wce = gpu_wce
    c = wce.Context(empty=True)
    s = fm.clean_set(mod, rate)
    B = 5
    h, h_lt = s["h"][:B], s["h_lt"][:B]
    eq = np.asarray(dm.demodulate(s["tx"][:B], s["rx"][:B], h, h_lt, mod, real=np.float64)["eq"], np.complex128)
    L0 = demap(wce, c, eq, h, h_lt, mod)
    assert np.all(np.isfinite(L0)) and np.abs(L0).max() < fm.LLR_MAX
    for k, every in ((45, False), (60, True)):
        g = 2.0 ** k
        L = demap(wce, c, eq, h * g, h_lt * g, mod)
        ld = fm.llr(eq, dm.blend(h * g, h_lt * g), mod)
        clamped = np.abs(np.asarray(ld, np.float64)) == fm.LLR_MAX
        print(f"{mod} bits, h 2^{k}: {int(clamped.sum())} of {clamped.size} soft bits at the clamp, "
              f"largest |L| at k = 0 {float(np.abs(L0).max()):.1f}")
        # 2^45: the soft bits of 2^10 and more at k = 0 clamp -- 13 of BPSK's (the largest 1073); 16-QAM's and
        # 64-QAM's largest, 456 and 401, stay below, so that gain runs those two sets unclamped up to 2^99.
        # 2^60: every soft bit clamps (the smallest non-zero one at k = 0 is 3.9e-4 > 2^-20)
        assert clamped[L0 != 0].all() if every else (not clamped.all() and (clamped.any() or mod != dm.BPSK)), k
        assert np.all(np.isfinite(L)), k
        assert np.all(np.abs(L) <= np.float32(fm.LLR_MAX)), k
        assert np.array_equal(np.sign(L), np.sign(L0)) and np.array_equal(np.signbit(L), np.signbit(L0)), k
        _within_bound(L, ld, f"{mod} bits, h 2^{k}")
        for terminated in (True, False):
            got = viterbi(wce, c, L, mod, rate, terminated, s["u"][:B])
            want = fm.decode(np.asarray(ld, np.float64).astype(np.float32), mod, rate, terminated)
            assert np.array_equal(got["bits"], want), (k, terminated)
            assert np.array_equal(got["nbiterr"], np.sum(want != s["u"][:B], axis=1)), (k, terminated)
        assert got["bits"].any(), "erasures alone decode to all-zero bits"
