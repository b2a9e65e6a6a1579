"""tests/frame_model.py on the CPU: the table is complete (every function of
include/wce.h with a frame count has a row or a reason), and every row that has a
numpy model (the long double oracle for the estimators) obeys the law under all
three transforms, bit for bit.  That proves the per-frame / shared split of each
row and that the poison values mean what the table says, and it settles the
inputs tests/test_frame_law_gpu.py uses: gain_model's low-SNR sets, on which
the models obey the law with no exception."""
import warnings

import numpy as np
import pytest

import cfo_model as cm
import combine_model as cb
import demod_model as dm
import fading_model as fd
import fec_model as fm
import frame_model as fr
import gain_model as gm
import reencode_model as rm
import stf_model as st
import sync_model as sm
import track_model as tk
import tx_model as tm
from oracle_py import N, NBLK
from test_gain_model import _estimate_args, _estimate_run

F64 = np.float64
B = 9       # frames of a set the models run (the device runs 5, 67 and 261)


def _quietly(run):
    """the models on hostile frames divide by zero and overflow; that is the point"""
    def f(a):
        with np.errstate(all="ignore"), warnings.catch_warnings():
            warnings.simplefilter("ignore")
            return run(a)
    return f


# numpy picks the order of a matrix product and of a pairwise sum by the shape of the batch, so these models do
# not give one frame alone the bits they give it in a batch.  They run a frame at a time, as batches of one: what
# the test then proves is the row's split into per-frame and shared arguments, and the poison values
BY_FRAME = ("preamble", "demodulate", "track", "modulate", "transmit", "transmit_tv", "channel", "channel_tv")


def _by_frame(row, run):
    def f(a):
        outs = [run(fr.window(row, a, i, 1)) for i in range(fr.n_frames(row, a))]
        return {n: np.concatenate([np.asarray(o[n]) for o in outs], axis=ax) for n, ax in row.outputs.items()
                if n in outs[0]}
    return f


def _hold(key, run, args, n=B):
    row = fr.BY_KEY[key]
    run = _quietly(_by_frame(row, run) if key in BY_FRAME else run)
    return fr.hold(row, run, args, fr.transforms(row, n))


# ---------------------------------------------------------------- the table
def test_every_batched_call_has_a_row_or_a_reason():
    bound = {c for r in fr.ROWS for c in r.calls}
    declared, batched = gm.declared_calls(), fr.batched_calls()
    assert bound <= declared and set(fr.UNBATCHED) <= declared, (bound | set(fr.UNBATCHED)) - declared
    assert len(batched) >= 30 and {"wce_estimate", "wce_sync_share", "wce_combine", "wce_psdu_deframe"} <= batched
    assert not batched - bound - set(fr.UNBATCHED), f"no row and no reason: {sorted(batched - bound - set(fr.UNBATCHED))}"
    assert not bound & set(fr.UNBATCHED)
    assert all(len(why) > 10 for why in fr.UNBATCHED.values())
    for r in fr.ROWS:
        assert not set(r.frame) & set(r.shared), r.key
        assert set(r.totals.values()) <= set(r.outputs), r.key
        assert r.indexed == ("first_frame" in r.shared), r.key
    text = open(gm.HEADER).read()
    assert "tests/frame_model.py" in text and "first_frame + f" in text


def test_transforms():
    for n in (5, 9, 67, 261):
        rot, der = fr.permutations(n)
        assert rot[1][0] == n - 1 and not np.any(der[1] == np.arange(n))
        odd, run = fr.poison_sets(n)
        assert len(odd[1]) <= n // 2 and len(run[1]) <= n // 2 and 0 in run[1]
        clean = np.setdiff1d(np.arange(n), odd[1])
        assert all((f + 1 in odd[1]) or (f - 1 in odd[1]) for f in clean), "a clean frame beside no poisoned one"
        assert fr.windows(n)[-1][1] == n // 2 + 1
    assert len(fr.poison_sets(67)[1][1]) == 17 and len(fr.poison_sets(261)[1][1]) == 17
    row = fr.BY_KEY["combine"]
    a = dict(rx=np.arange(24.0).reshape(2, 4, 3), h=None, ow2=np.arange(8.0).reshape(2, 4))
    m = fr.moved(row, a, fr.rotation(4))
    assert np.array_equal(m["rx"][:, 0], a["rx"][:, 3]) and np.array_equal(m["ow2"][:, 1], a["ow2"][:, 0])
    p = fr.poisoned(row, a, [1])
    assert np.isnan(p["rx"][:, 1]).all() and np.array_equal(p["rx"][:, 0], a["rx"][:, 0])
    w = fr.window(fr.BY_KEY["channel"], dict(wave=np.zeros((6, 2)), first_frame=3), 2, 3)
    assert w["first_frame"] == 5 and w["wave"].shape == (3, 2)
    assert fr.poison_values("lengths", np.int32)[0] == 3 and fr.poison_values("u", np.uint8) == (0, 255)
    # check() reports the output and the first frame that differs, and counts a sign of zero
    row = fr.BY_KEY["nonfinite_scan"]
    def leaky(x):          # every frame reports its left neighbour
        bad = np.r_[0, fr.scan_model(x)["bad"][:-1]].astype(np.uint8)
        return {"bad": bad, "n_bad": np.array([bad.sum()])}
    args = fr.scan_set(12)
    assert fr.check(row, fr.scan_model, args, ("window", 3, 5)) == []
    assert fr.check(row, leaky, args, ("window", 3, 5)) == [("bad", 0)]
    assert fr.check(row, leaky, args, fr.poison_sets(12)[0]) == [("bad", 2)]
    short = lambda x: dict(fr.scan_model(x), n_bad=np.array([0]))
    assert fr.check(row, short, args, ("window", 0, 5)) == [("n_bad", -1)]
    assert fr.first_difference(np.array([0.0, 0.0]), np.array([0.0, -0.0])) == 1
    assert fr.first_difference(np.array([np.nan]), np.array([np.nan])) is None


# ---------------------------------------------------------------- front end
def test_front_end():
    s = gm.first(gm.front_set(), B)
    for form in ("plain", "cfo"):
        eps = lambda a: np.zeros(len(a["samples"])) if form == "plain" else a["eps"]
        _hold("blocks", lambda a: {"sym": cm.blocks(a["samples"], eps(a), 3, NBLK, F64)}, s)

    def run(a):
        e = np.asarray(cm.estimate(a["lptot"], F64), F64)
        pre, ow2 = cm.preamble(a["lptot"], e, F64)
        return {"pre_fft": pre, "ow2": ow2, "cfo": e}
    _hold("preamble", run, s)


def test_sync():
    def run(a):
        start, metric, _ = sm.sync(a["capture"], a["ltf"], a["threshold"], 0, F64)
        return {"start": start, "metric": metric}
    base = _hold("sync", run, gm.first(gm.sync_set(), 23), 23)
    assert (base["start"] >= 0).sum() >= 5

    def run_stf(a):
        r = st.sync_stf(a["capture"], a["ltf"], a["threshold_stf"], a["threshold_ltf"], 0, F64)
        return {n: np.asarray(r[n]) for n in ("start", "cfo", "metric_stf", "metric_ltf")}
    base = _hold("sync_stf", run_stf, gm.first(gm.stf_set(), 23), 23)
    assert (base["start"] >= 0).sum() >= 5 and (base["start"] < 0).sum() >= 2


# ---------------------------------------------------------------- the estimators (the long double oracle)
@pytest.mark.parametrize("matlab", [False, True], ids=["C", "MATLAB"])
@pytest.mark.parametrize("mode", ["ref", "textbook", "frame_cov", "noise", "cov"])
def test_estimate(golden, oracle, mode, matlab):
    args = fr.vary_tx(_estimate_args(golden, np.random.default_rng(0x6A19)))
    if mode == "cov":
        p = np.exp(-0.3 * np.arange(12))
        args["Rhh"] = np.diag(np.r_[p / p.sum() * 1.1e-4, np.zeros(N - 12)]).astype(complex)
    if mode != "noise":
        args["ow2"] = None
    n = len(args["tx"])
    _hold("estimate", _estimate_run(oracle, golden, mode, matlab), args, n)


# ---------------------------------------------------------------- demodulators
@pytest.mark.parametrize("mod,rate,snr", gm.DEMOD_SETS)
def test_demodulate(mod, rate, snr):
    def run(a):
        r = dm.demodulate(a["tx"], a["rx"], a["h"], a["h_lt"], mod, a["scale"], real=F64)
        return {n: np.asarray(r[n]) for n in fr.BY_KEY["demodulate"].outputs}
    base = _hold("demodulate", run, gm.first(gm.demod_set(mod, rate, snr), B))
    assert base["nerr"].sum() > 0, "a low-SNR set has symbol errors"


@pytest.mark.parametrize("mod", dm.MODS)
def test_track_demodulate(mod):
    def run(a):
        r = tk.track(a["tx"], a["rx"], a["h"], mod, scale=a["scale"], real=F64)
        return {n: np.asarray(r[n]) for n in fr.BY_KEY["track"].outputs}
    _hold("track", run, gm.first(gm.track_set(mod), B))


# ---------------------------------------------------------------- soft bits, decoder, re-encoder, PSDU
@pytest.mark.parametrize("mod,rate,snr", gm.DEMOD_SETS)
def test_soft_demap(mod, rate, snr):
    s = gm.first(gm.demap_set(mod, rate, snr), B)
    f32 = lambda L: {"llr": np.asarray(L, F64).astype(np.float32)}
    _hold("soft_demap", lambda a: f32(fm.llr(a["eq"], dm.blend(a["h"], a["h_lt"], F64), mod, a["scale"], F64)), s)
    _hold("soft_demap_blocks", lambda a: f32(fm.llr(a["eq"], a["hb"], mod, a["scale"], F64)), s)


@pytest.mark.parametrize("mod,rate", gm.DECODE_SETS)
def test_viterbi(mod, rate):
    s = fm.integer_set(mod, rate)
    args = dict(llr=s["llr"][:B], u=s["u"][:B])
    for terminated in (True, False):
        def run(a):
            bits = fm.decode(a["llr"], mod, rate, terminated)
            return {"bits": bits, "nbiterr": np.sum(bits != a["u"], axis=1).astype(np.uint32)}
        base = _hold("viterbi", run, args)
    assert base["nbiterr"].sum() > 0, "the integer set decodes with errors"


@pytest.mark.parametrize("mod,rate,snr", gm.DEMOD_SETS)
def test_reencode(mod, rate, snr):
    def run(a):
        x = rm.xhat(a["u"] & 1, mod, rate, a["scale"], a["pilots"])
        return {"tx": x, "h": np.asarray(rm.h_dd(x, a["rx"], a["theta"], F64)[0])}
    _hold("reencode", run, gm.first(gm.reencode_set(mod, rate, snr), B))


@pytest.mark.parametrize("mod,rate", [(1, fm.RATE_1_2), (4, fm.RATE_2_3), (6, fm.RATE_3_4)])
def test_psdu(mod, rate):
    a = fr.psdu_frame_set(mod, rate, B)
    base = _hold("psdu_frame", fr.psdu_frame_model, a)
    assert base["bits"].any(axis=1).all()
    base = _hold("psdu_deframe", fr.psdu_deframe_model, fr.psdu_deframe_set(mod, rate, B))
    assert 0 < base["n_good"][0] < B and (base["seed"] == 0).any()


# ---------------------------------------------------------------- diversity
def test_combine():
    s = gm.first(gm.combine_set(), B, axis=1)
    for weighted in (True, False):
        def run(a):
            r = cb.combine(a["rx"], a["h"], a["ow2"] if weighted else None, F64)
            return {"rx_c": np.asarray(r["rx"]), "h_c": np.asarray(r["h"])}
        _hold("combine", run, s)


def test_sync_share():
    metric, start, cfo = cb.sync_share_set(3, 23)

    def run(a):
        s, c = cb.sync_share(a["metric"], a["start"], a["cfo"])
        return {"start": s, "cfo": c}
    _hold("sync_share", run, dict(metric=metric, start=start, cfo=cfo), 23)


# ---------------------------------------------------------------- transmit side
def _chan(a):
    return dict(cfo=a["cfo"], ow2=a["ow2"], delay=a["delay"], seed=a["seed"], first_frame=a.get("first_frame", 0))


def test_transmit_side():
    s = gm.first(gm.tx_set(), B)
    _hold("modulate", lambda a: {"wave": tm.modulate(a["sym"], a["tx_pre"], F64)}, s)
    s["wave"] = np.asarray(tm.modulate(s["sym"], s["tx_pre"], F64), np.complex128)
    L = s["capture_len"]
    runs = {"channel": lambda a: tm.channel(a["wave"], L, a["taps"], 1, real=F64, **_chan(a)),
            "transmit": lambda a: tm.transmit(a["sym"], L, a["tx_pre"], F64, taps=a["taps"], **_chan(a)),
            "channel_tv": lambda a: fd.channel_tv(a["wave"], L, a["knots"], 80, 1, real=F64, **_chan(a)),
            "transmit_tv": lambda a: fd.transmit_tv(a["sym"], L, a["knots"], 80, a["tx_pre"], F64, **_chan(a))}
    for key, f in runs.items():
        base = _hold(key, lambda a: {"capture": f(a)}, dict(s, first_frame=3))
        assert np.isfinite(base["capture"]).all()
    # the windows above ran with the noise on: two frames' noise differs, and a shifted first_frame moves it
    a, b = runs["channel"](dict(s, first_frame=3)), runs["channel"](dict(s, first_frame=4))
    assert not gm.same_bits(a[1:], b[1:]) and not gm.same_bits(a[1:] - a[:-1], np.zeros_like(a[1:]))


def test_short_field():
    run = lambda a: {"wave": np.tile(st.short_field(a["amplitude"], F64), (a["n_frames"], 1))}
    _hold("short_field", run, dict(amplitude=dm.SCALE, n_frames=B))


# ---------------------------------------------------------------- the guard
def test_nonfinite_scan():
    base = _hold("nonfinite_scan", fr.scan_model, fr.scan_set(B))
    assert 0 < base["n_bad"][0] < B
