"""Every row of tests/gain_model.py on the project's own numpy models (fp64, and
the long double oracle for the estimators): the inputs moved by g = 2^k move
the outputs as the row says, bit for bit.  This proves the table before a GPU
sees it and settles the gains: a row runs on the device at the k it passes here,
with no overflow and no subnormal on the way."""
import numpy as np
import pytest

import cfo_model as cm
import combine_model as cb
import demod_model as dm
import fading_model as fd
import fec_model as fm
import gain_model as gm
import reencode_model as rm
import stf_model as st
import sync_model as sm
import track_model as tk
import tx_model as tm
from oracle_py import N, NBLK, from_split

F64 = np.float64
B = 7     # frames of a set the models run (the device runs 5 and 67)


def _first(args, n=B, axis=0):
    return gm.first(args, n, axis)


def _hold(law, run, args, ks=None, names=None):
    base = run(args)
    for k in (gm.gains(law) if ks is None else ks):
        bad = gm.check(law, run, args, k, names, base=base)
        assert not bad, (law.key, k, bad)
    return base


def test_the_header_declares_every_call():
    declared = gm.declared_calls()
    for law in gm.LAWS:
        for c in law.calls:
            assert c in declared, (law.key, c)
    text = open(gm.HEADER).read()
    assert "WCE_LLR_MAX" in text and "Signal level" in text


def test_gains():
    assert gm.gains(gm.BY_KEY["modulate"]) == (-40, -11, 11, 40, -100, 100)
    assert gm.gains(gm.BY_KEY["soft_demap/channel"]) == (-40, -11, 11, 40)
    assert gm.gains(gm.BY_KEY["viterbi"]) == (-40, -11, 11, 40)
    a = np.array([1.5 - 2j, 0.0, -0.0 + 1e-300j])
    assert gm.same_bits(a, a.copy()) and not gm.same_bits(a, a * (1 + 2.0 ** -52))
    assert not gm.same_bits(np.array([0.0]), np.array([-0.0]))
    assert gm.normal(np.float32(2.0 ** -126), np.float32) and not gm.normal(2.0 ** -127, np.float32)
    assert not gm.normal(2.0 ** 128, np.float32)


# ---------------------------------------------------------------- front end
def test_front_end_blocks():
    s = gm.front_set()
    for eps in (np.zeros(B), s["eps"][:B]):
        run = lambda a: {"sym": cm.blocks(a["samples"], eps, 3, NBLK, F64)}
        _hold(gm.BY_KEY["blocks"], run, _first(s))


def test_front_end_preamble():
    def run(a):
        e = np.asarray(cm.estimate(a["lptot"], F64), F64)
        pre, ow2 = cm.preamble(a["lptot"], e, F64)
        return {"pre_fft": pre, "ow2": ow2, "cfo": e}
    _hold(gm.BY_KEY["preamble"], run, _first(gm.front_set()))


@pytest.mark.parametrize("which", ["capture", "ltf"])
def test_sync(which):
    def run(a):
        start, metric, _ = sm.sync(a["capture"], a["ltf"], a["threshold"], 0, F64)
        return {"start": start, "metric": metric}
    base = _hold(gm.BY_KEY["sync/" + which], run, _first(gm.sync_set(), 23))
    assert (base["start"] >= 0).sum() >= 5


@pytest.mark.parametrize("which", ["capture", "ltf"])
def test_sync_stf(which):
    def run(a):
        r = st.sync_stf(a["capture"], a["ltf"], a["threshold_stf"], a["threshold_ltf"], 0, F64)
        return {n: np.asarray(r[n]) for n in ("start", "cfo", "metric_stf", "metric_ltf")}
    base = _hold(gm.BY_KEY["sync_stf/" + which], run, _first(gm.stf_set(), 23))
    assert (base["start"] >= 0).sum() >= 5 and (base["start"] < 0).sum() >= 2


# ---------------------------------------------------------------- the estimators (the long double oracle)
def _estimate_args(golden, rng):
    inp = golden["inputs"]
    tx = np.repeat(inp["tx_symb"][None], B, axis=0)
    amp = np.sqrt(inp["ow2"] / 2)
    noise = lambda shape: amp * (rng.standard_normal(shape) + 1j * rng.standard_normal(shape))
    rx = np.repeat(inp["rx_symb"][None], B, axis=0) + noise(tx.shape)
    return dict(tx=tx, rx=rx, rx_pre=inp["rx_pre"][None] + noise((B, N)), tx_pre=np.array(inp["tx_pre"], complex),
                ctx_tx_pre=np.array(inp["tx_pre"], complex), ctx_rx_pre=np.array(inp["rx_pre"], complex),
                ctx_ow2=float(inp["ow2"]), ow2=inp["ow2"] * rng.uniform(0.5, 2.0, B), Rhh=None)


def _estimate_run(oracle, golden, mode, matlab):
    """the estimators of one frame batch in the oracle: C semantics from block 0, MATLAB semantics averaged over
    blocks 0..3; PS_MMSE by `mode`: ref, textbook, frame_cov, noise (frame_cov with each frame's own ow2), cov"""
    r = golden["ref"]
    F, Fr, invF = oracle.fmatrix(), from_split(r["F"]), from_split(r["invF"])
    lt = oracle.matlab_lt_ls if matlab else oracle.lt_ls
    cvec = lambda h: F @ (F.conj() @ h / N)

    def run(a):
        out = {n: [] for n in gm.BY_KEY["estimate/channel"].outputs}
        C = F @ oracle._ld(a["Rhh"]) @ F.conj().T if mode == "cov" else None
        h_ctx = lt(a["ctx_tx_pre"], a["ctx_rx_pre"])
        for f in range(len(a["tx"])):
            t, x = a["tx"][f], a["rx"][f]
            h_f = lt(a["tx_pre"], a["rx_pre"][f])
            out["lt_ls"].append(h_f)
            for n in ("ps_linear", "ps_cubic", "ps_sinc"):
                out[n].append(oracle.matlab(n, t, x) if matlab else getattr(oracle, n)(t[0], x[0]))
            per = []
            for b in (range(4) if matlab else (0,)):
                if mode == "ref":
                    per.append(oracle.mmse_ref_repaired(t[b], x[b], Fr, a["ctx_ow2"], h_ctx, invF))
                elif mode == "cov":
                    per.append(oracle.mmse_unified(C, np.ones(N, np.uint8), 1.0, a["ctx_ow2"], t[b], x[b]))
                else:
                    c = cvec(h_ctx if mode == "textbook" else h_f)
                    per.append(oracle.mmse_textbook_closed(c, t[b], x[b], a["ow2"][f] if mode == "noise" else a["ctx_ow2"]))
            out["ps_mmse"].append(np.mean(np.stack(per), axis=0))
            out["eq"].append(oracle.equalize(x, h_f, out["ps_linear"][-1]))
        return {n: np.stack(v) for n, v in out.items()}
    return run


@pytest.mark.parametrize("matlab", [False, True], ids=["C", "MATLAB"])
@pytest.mark.parametrize("mode", ["ref", "textbook", "frame_cov", "noise", "cov"])
def test_estimate(golden, oracle, mode, matlab):
    args = _estimate_args(golden, np.random.default_rng(0x6A19))
    if mode == "cov":
        p = np.exp(-0.3 * np.arange(12))
        args["Rhh"] = np.diag(np.r_[p / p.sum() * 1.1e-4, np.zeros(N - 12)]).astype(complex)
    run = _estimate_run(oracle, golden, mode, matlab)
    for key in ("estimate/channel", "estimate/tx"):
        _hold(gm.BY_KEY[key], run, args)


# ---------------------------------------------------------------- demodulators
@pytest.mark.parametrize("mod,rate,snr", gm.DEMOD_SETS)
def test_demodulate(mod, rate, snr):
    def run(a):
        r = dm.demodulate(a["tx"], a["rx"], a["h"], a["h_lt"], mod, a["scale"], real=F64)
        return {n: np.asarray(r[n]) for n in gm.BY_KEY["demodulate/tx"].outputs}
    args = _first(gm.demod_set(mod, rate, snr))
    for key in ("demodulate/channel", "demodulate/tx"):
        base = _hold(gm.BY_KEY[key], run, args)
    assert base["nerr"].sum() > 0, "a low-SNR set has symbol errors"


@pytest.mark.parametrize("mod", dm.MODS)
def test_track_demodulate(mod):
    def run(a):
        r = tk.track(a["tx"], a["rx"], a["h"], mod, scale=a["scale"], real=F64)
        return {n: np.asarray(r[n]) for n in gm.BY_KEY["track/tx"].outputs}
    args = _first(gm.track_set(mod))
    for key in ("track/channel", "track/tx"):
        _hold(gm.BY_KEY[key], run, args)


# ---------------------------------------------------------------- soft bits, decoder
@pytest.mark.parametrize("mod,rate,snr", gm.DEMOD_SETS)
def test_soft_demap(mod, rate, snr):
    s = _first(gm.demap_set(mod, rate, snr))
    runs = {"soft_demap": lambda a: fm.llr(a["eq"], dm.blend(a["h"], a["h_lt"], F64), mod, a["scale"], F64),
            "soft_demap_blocks": lambda a: fm.llr(a["eq"], a["hb"], mod, a["scale"], F64)}
    for call, f in runs.items():
        run = lambda a: {"llr": np.asarray(f(a), F64).astype(np.float32)}
        for way in ("channel", "tx"):
            law = gm.BY_KEY[f"{call}/{way}"]
            base = _hold(law, run, s)
            # the gains keep every soft bit of the set a normal float: 2^+-40 moves them by 2^+-80
            for k in gm.gains(law):
                assert gm.normal(base["llr"].astype(np.longdouble) * np.longdouble(2.0) ** (2 * k), np.float32), k
            assert np.max(np.abs(base["llr"])) * 2.0 ** 80 < fm.LLR_MAX


@pytest.mark.parametrize("mod,rate", gm.DECODE_SETS)
def test_viterbi(mod, rate):
    s = fm.integer_set(mod, rate)
    args = dict(llr=s["llr"][:B], u=s["u"][:B])
    for terminated in (True, False):
        def run(a):
            bits = fm.decode(a["llr"], mod, rate, terminated)
            return {"bits": bits, "nbiterr": np.sum(bits != a["u"], axis=1).astype(np.uint32)}
        base = _hold(gm.BY_KEY["viterbi"], run, args)
        # the largest path metric and the smallest soft bit stay normal floats
        assert gm.normal(np.float64(31 * 2 * 3240) * 2.0 ** 40, np.float32) and gm.normal(2.0 ** -40, np.float32)
    assert base["nbiterr"].sum() > 0, "the integer set decodes with errors"


# ---------------------------------------------------------------- re-encoder
@pytest.mark.parametrize("mod,rate,snr", gm.DEMOD_SETS)
def test_reencode(mod, rate, snr):
    def run(a):
        x = rm.xhat(a["u"], mod, rate, a["scale"], a["pilots"])
        return {"tx": x, "h": np.asarray(rm.h_dd(x, a["rx"], a["theta"], F64)[0])}
    args = _first(gm.reencode_set(mod, rate, snr))
    for key in ("reencode/channel", "reencode/tx"):
        _hold(gm.BY_KEY[key], run, args)


# ---------------------------------------------------------------- diversity
def test_combine():
    s = _first(gm.combine_set(), axis=1)
    law = gm.BY_KEY["combine/weighted"]

    def run(a, weighted=True):
        r = cb.combine(a["rx"], a["h"], a["ow2"] if weighted else None, F64)
        return {"rx_c": np.asarray(r["rx"]), "h_c": np.asarray(r["h"])}
    base = run(s)
    for k in gm.gains(law):   # each branch its own gain: +k, -k, +k
        assert not gm.check(law, run, s, gm.branch_gains(k, gm.COMBINE_A), base=base), k
    # "a common factor on every ow2 changes no equalized symbol rx_c / h_c" (include/wce.h)
    for c in (4.0, 2.0 ** -40, 2.0 ** 40):
        r = run(dict(s, ow2=s["ow2"] * c))
        with np.errstate(invalid="ignore", divide="ignore"):
            assert gm.same_bits(r["rx_c"] / r["h_c"][:, None, :], base["rx_c"] / base["h_c"][:, None, :])
    _hold(gm.BY_KEY["combine/unweighted"], lambda a: run(a, False), s)


# ---------------------------------------------------------------- transmit side
def test_modulate():
    run = lambda a: {"wave": tm.modulate(a["sym"], a["tx_pre"], F64)}
    _hold(gm.BY_KEY["modulate"], run, _first(gm.tx_set()))


def _chan(a):
    return dict(cfo=a["cfo"], ow2=a["ow2"], delay=a["delay"], seed=a["seed"])


@pytest.mark.parametrize("noise", [True, False])
def test_channel_and_transmit(noise):
    s = _first(gm.tx_set())
    if not noise:
        s["ow2"] = None
    s["wave"] = np.asarray(tm.modulate(s["sym"], s["tx_pre"], F64), np.complex128)
    L = s["capture_len"]
    chan = lambda a: {"capture": tm.channel(a["wave"], L, a["taps"], 1, real=F64, **_chan(a))}
    xmit = lambda a: {"capture": tm.transmit(a["sym"], L, a["tx_pre"], F64, taps=a["taps"], **_chan(a))}
    chan_tv = lambda a: {"capture": fd.channel_tv(a["wave"], L, a["knots"], 80, 1, real=F64, **_chan(a))}
    xmit_tv = lambda a: {"capture": fd.transmit_tv(a["sym"], L, a["knots"], 80, a["tx_pre"], F64, **_chan(a))}
    for key, run in (("channel/taps", chan), ("channel/wave", chan), ("transmit/taps", xmit), ("transmit/sym", xmit),
                     ("channel_tv/knots", chan_tv), ("transmit_tv/knots", xmit_tv), ("transmit_tv/sym", xmit_tv)):
        _hold(gm.BY_KEY[key], run, s)


def test_short_field():
    run = lambda a: {"wave": st.short_field(a["amplitude"], F64)}
    _hold(gm.BY_KEY["short_field"], run, dict(amplitude=dm.SCALE))
