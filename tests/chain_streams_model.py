"""The two scripted links of tests/test_chain_streams_gpu.py on the numpy chain models: what is sent, and which
packets a receiver built from sync_model, stf_model, cfo_model, demod_model, track_model, combine_model, fec_model,
reencode_model and psdu_model finds good.  16-QAM rate 1/2, the pair whose counts the link tests pin.

The noise is set per packet, on the CPU, before the device saw either link: every packet is sent at nominal 30 dB
but each fifth (link P) or fourth (link Q, on both antennas), which is sent at 5 dB.  The models below then detect
every packet and find the 5 dB packets bad and the others good, but for packet 12 of link P: its second tap is the
stronger one (0.72 against 0.69), the timing locks one sample late and the packet is lost at any SNR -- 119 good of
150, the same after the first decode and after the decision-directed round.  Measured on the models, the pattern
stays the same with the good packets anywhere from 22 to 40 dB and the bad ones from 3 to 7 dB (link P) or from 4
to 6.5 dB (link Q: at 3.5 dB one antenna of one packet falls under the short field's threshold, at 7 dB two
antennas carry packet 3 through).  The device's chain differs from the models by roundings of 1e-13, not by
decibels, so the FCS counts of both links are known before the device runs."""
import functools

import numpy as np

import cfo_model as cm
import combine_model as cb
import demod_model as dm
import fading_model as fd
import fec_model as fm
import psdu_model as pm
import reencode_model as rm
import stf_model as st
import sync_model as sm
import track_model as trk
import tx_model as tm

MOD, RATE = dm.QAM16, fm.RATE_1_2
T, NBY, PSDU_LEN = pm.info_bits(MOD, RATE), pm.nbytes(MOD, RATE), pm.max_len(MOD, RATE)
SNR_GOOD, SNR_BAD = 30.0, 5.0
THRESHOLD = tm.CHAIN_THRESHOLD

P_B, P_LEN, P_SEED, P_EVERY = 150, 1488, 0x57A3, 5
P_SHARDS = ((0, 67), (67, 13), (80, 41), (121, 29))           # (first frame, frames)

Q_B, Q_A, Q_LEN, Q_SEED, Q_EVERY = 20, 2, 1648, 0x57A9, 4
Q_KNOTS, Q_PERIOD, Q_RHO = 21, 80, 0.995                      # (21 - 1) 80 > 1520 + 6 - 2
Q_SHARDS = ((0, 13), (13, 7))
Q_MU, Q_BETA = trk.MU, trk.BETA


def _draw(rng, B, every):
    payload = rng.integers(0, 256, (B, PSDU_LEN - 4)).astype(np.uint8)
    seeds = rng.integers(1, 128, B).astype(np.uint8)
    cfo = rng.uniform(-0.002, 0.002, B)
    delay = rng.integers(0, 100, B).astype(np.int32)
    bad = np.arange(B) % every == every - 1
    ow2 = np.where(bad, float(tm.nominal_ow2(SNR_BAD)), float(tm.nominal_ow2(SNR_GOOD)))
    return {"payload": payload, "seeds": seeds, "bits": pm.frame(payload, seeds, MOD, RATE), "cfo": cfo,
            "delay": delay, "ow2": ow2, "bad": bad}


@functools.lru_cache(maxsize=None)
def link_p_set():
    """150 packets behind six static taps each, with a carrier offset, a delay and its own noise -> dict"""
    rng = np.random.default_rng(P_SEED)
    c = _draw(rng, P_B, P_EVERY)
    c["taps"] = tm.random_taps(rng, P_B, 6)
    return c


@functools.lru_cache(maxsize=None)
def link_q_set():
    """20 packets seen by two antennas through six taps that fade by rho a block, one offset and delay for both
    antennas, each antenna its own noise draw (first_frame = a 20 + f) -> dict, knots [A][B][21][6]"""
    rng = np.random.default_rng(Q_SEED)
    c = _draw(rng, Q_B, Q_EVERY)
    c["knots"] = np.stack([fd.fading_taps(rng, Q_B, fd.LINK_POWER, Q_RHO, Q_KNOTS) for _ in range(Q_A)])
    return c


def _fields(cap, start, eps, real):
    n = len(cap)
    field = np.stack([cap[f, start[f]:start[f] + 128] for f in range(n)])
    pk = np.stack([cap[f, start[f] + 128:start[f] + 1328] for f in range(n)])
    rx_pre, ow2 = cm.preamble(field, eps, real)
    return field, rx_pre, np.asarray(ow2, np.float64), cm.blocks(pk, eps, 0, 15, real)


def _decode(eq, hu, real):
    L = np.asarray(fm.llr(eq, hu, MOD, tm.SCALE, real), np.float64).astype(np.float32)
    return fm.decode(L, MOD, RATE, terminated=False)


@functools.lru_cache(maxsize=None)
def link_p_model(real=np.float64):
    """link P on the CPU: tx_model's transmitter, sync, the two-copy offset, LT_LS, a tracked demodulation, soft
    bits and the unterminated decoder, one decision-directed round on its bits and phases, the deframer
    -> dict detected [B] bool, fcs_first and fcs_ok uint32 [B] (after the first decode and after the round)"""
    c = link_p_set()
    pre = tm.chain_pre()
    tx = fm.transmit(c["bits"], MOD, RATE)[0]
    cap = np.asarray(tm.transmit(tx, P_LEN, pre, real, taps=c["taps"], cfo=c["cfo"], ow2=c["ow2"], delay=c["delay"],
                                 seed=P_SEED), np.complex128)
    ltf = np.asarray(tm.idft64(pre, tm.LD), np.complex128)
    start = sm.sync(cap, ltf, THRESHOLD, 0, real)[0]
    det = (start >= 0) & (start + 1328 <= P_LEN)
    s0 = np.where(det, start, 0)
    field = np.stack([cap[f, s0[f]:s0[f] + 128] for f in range(P_B)])
    eps = np.asarray(cm.estimate(field, real), np.float64)
    _, rx_pre, _, rx = _fields(cap, s0, eps, real)
    with np.errstate(invalid="ignore", divide="ignore"):
        h = dm.lt_ls(np.broadcast_to(pre, (P_B, 53)), rx_pre, real)
    d = dm.demodulate(tx, rx, h, None, MOD, tm.SCALE, True, True, real)
    bits1 = _decode(d["eq"], dm.blend(h, None, real), real)
    lengths = np.full(P_B, PSDU_LEN)
    first = pm.deframe(bits1, lengths, MOD, RATE)[2]
    hdd = rm.h_dd(rm.xhat(bits1, MOD, RATE), rx, np.asarray(d["theta"], np.float64), real)[0]
    d2 = dm.demodulate(tx, rx, hdd, None, MOD, tm.SCALE, True, True, real)
    bits2 = _decode(d2["eq"], dm.blend(hdd, None, real), real)
    return {"detected": det, "fcs_first": first, "fcs_ok": pm.deframe(bits2, lengths, MOD, RATE)[2]}


@functools.lru_cache(maxsize=None)
def link_q_model(real=np.float64):
    """link Q on the CPU: the short field in front, fading_model's channel per antenna, sync_stf, sync_share,
    the fields at the shared start and offset, LT_LS, combine weighted by the fields' noise estimates, the tracker,
    soft bits on its per-block estimates, the unterminated decoder, the deframer
    -> dict detected [A][B] bool (before sharing), fcs_ok uint32 [B]"""
    c = link_q_set()
    A, B = Q_A, Q_B
    pre = tm.chain_pre()
    tx = fm.transmit(c["bits"], MOD, RATE)[0]
    p = np.abs(np.asarray(pre))
    amp = float(np.sqrt(np.mean(p[p != 0] ** 2)))
    wave = np.concatenate([np.broadcast_to(st.short_field(amp, real), (B, st.STF)), tm.modulate(tx, pre, real)],
                          axis=1)
    cap = np.concatenate([np.asarray(fd.channel_tv(wave, Q_LEN, c["knots"][a], Q_PERIOD, 1, c["cfo"], c["ow2"],
                                                   c["delay"], Q_SEED, a * B, real), np.complex128)
                          for a in range(A)])
    ltf = np.asarray(tm.idft64(pre, tm.LD), np.complex128)
    r = st.sync_stf(cap, ltf, st.THR_STF, THRESHOLD, 0, real)
    det = np.asarray(r["start"]).reshape(A, B) >= 0
    start, eps = cb.sync_share(np.asarray(r["metric_ltf"], np.float64).reshape(A, B), r["start"].reshape(A, B),
                               np.asarray(r["cfo"], np.float64).reshape(A, B))
    ok = (start >= 0) & (start + 1328 <= Q_LEN)
    s0 = np.where(ok, start, 0).reshape(-1)
    e0 = np.where(ok, eps, 0.0).reshape(-1)
    _, rx_pre, ow2, rx = _fields(cap, s0, e0, real)
    with np.errstate(invalid="ignore", divide="ignore"):
        h = dm.lt_ls(np.broadcast_to(pre, (A * B, 53)), rx_pre, real)
    comb = cb.combine(np.asarray(rx).reshape(A, B, 15, 53), np.asarray(h).reshape(A, B, 53), ow2.reshape(A, B), real)
    t = trk.track(tx, comb["rx"], comb["h"], MOD, Q_MU, Q_BETA, real=real)
    bits = _decode(t["eq"], t["h_blocks"], real)
    return {"detected": det, "fcs_ok": pm.deframe(bits, np.full(B, PSDU_LEN), MOD, RATE)[2]}
