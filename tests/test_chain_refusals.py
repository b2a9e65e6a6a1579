"""Every refusal of the 24 entry points of the receive and transmit chain (csrc/wce_chain_api.cpp), on the CPU.

The chain calls validate their arguments before they look into the context, so a call made with the opaque context
0x10 and opaque aligned addresses is refused, or returns WCE_OK at a count of 0, without a device.  One table per
call: each row changes one argument of a valid base call (a second one only where the first would otherwise make it
invalid too) and states the return code and the whole text of wce_last_error().  A row's last element says what the
same call does at a count of 0: AT0 (the default) the same refusal, N0 WCE_OK, because the check depends on the
count or, in the front-end block and preamble calls, stands behind their early return at 0 frames.

Rows that several calls share are made by the function named after the check they come from (check_symbols,
check_channel, ...), with the call's name in front where the call puts it there; the front-end and sync calls'
messages are bare.

Not in the tables, because no argument set reaches them with an opaque context:
  * wce_viterbi_decode's "the survivor memory of T steps does not fit the LDS" and every "... launch" message:
    they come back from the launcher;
  * "lptot_len < 128 or stride < len" of wce_front_end_preamble_at: the window check before it refuses both;
  * check_frames' own "tx/rx required" in wce_demodulate and wce_track_demodulate: the calls' prefixed one is first
    (its block, semantics and preamble refusals cannot arise: the calls pass block 0, C semantics, no preambles);
  * "taps_stride neither 0 nor >= n_taps" in wce_channel_tv and wce_transmit_tv: they pass no taps."""
import ctypes

import pytest

OK, EINVAL = 0, -1
AT0, N0 = "refused at a count of 0 too", "WCE_OK at a count of 0"
FS = 15 * 53
T31 = 2 ** 31
NAN, INF = float("nan"), float("inf")


def rows(prefix, table):
    """(changes, text[, at 0]) -> (changes, EINVAL, prefix + text, at 0)"""
    return [(r[0], EINVAL, prefix + r[1], r[2] if len(r) > 2 else AT0) for r in table]


# ---------------------------------------------------------------- the front end
def blocks_rows(at=False, cfo=False):
    t = [({"n_frames": -1}, "n_frames < 0 or n_blocks < 1"), ({"n_blocks": 0}, "n_frames < 0 or n_blocks < 1"),
         ({"capture" if at else "samples": None}, "null buffer", N0), ({"sym": None}, "null buffer", N0),
         ({"block_stride": 52}, "output strides too small", N0), ({"frame_stride": 105}, "output strides too small", N0),
         ({"n_frames": 2 ** 30}, "n_frames * n_blocks >= 2^31")]
    if at:
        t += window_rows()
    else:
        t += [({"packet_stride": 159}, "packet_stride < 80 n_blocks", N0)]
    if at or cfo:
        t += [({"cfo": 0x3004}, "cfo not 8-byte aligned", N0), ({"sample_offset": T31}, "|sample_offset| >= 2^31", N0),
              ({"sample_offset": -T31}, "|sample_offset| >= 2^31", N0)]
    return rows("", t)


def window_rows():
    return [({"start": None}, "null start", N0), ({"start": 0x4002}, "start not 4-byte aligned", N0),
            ({"capture_len": 127}, "capture_len outside [128, 2^31)", N0),
            ({"capture_len": T31, "capture_stride": T31}, "capture_len outside [128, 2^31)", N0),
            ({"capture_stride": 399}, "capture_stride < capture_len", N0)]


def preamble_rows(at=False, cfo=False):
    t = [({"n_frames": -1}, "n_frames < 0"),
         ({"capture" if at else "lptot": None}, "null buffer", N0), ({"pre_fft": None}, "null buffer", N0),
         ({"pre_stride": 52}, "pre_stride < 53", N0), ({"n_frames": T31}, "n_frames >= 2^31")]
    if at:
        t += window_rows() + [({"cfo": None}, "estimate without cfo", N0)]
    else:
        t += [({"lptot_len": 127}, "lptot_len < 128 or stride < len", N0),
              ({"lptot_stride": 159}, "lptot_len < 128 or stride < len", N0)]
    if cfo:
        t += [({"cfo": None}, "null cfo")]
    if at or cfo:
        t += [({"cfo": 0x4004}, "cfo not 8-byte aligned", N0)]
    return rows("", t)


def sync_rows(stf):
    t = [({"n_frames": -1}, "n_frames < 0"),
         ({"capture_len": 143 if stf else 127}, "capture_len outside [%d, 2^31)" % (144 if stf else 128)),
         ({"capture_len": T31, "capture_stride": T31}, "capture_len outside [%d, 2^31)" % (144 if stf else 128)),
         ({"capture_stride": 399}, "capture_stride < capture_len"),
         ({"backoff": -1}, "backoff outside [0, 31]"), ({"backoff": 32}, "backoff outside [0, 31]"),
         ({"start": None}, "start null or not 4-byte aligned"), ({"start": 0x3002}, "start null or not 4-byte aligned"),
         ({"ltf": None}, "ltf null or not 16-byte aligned"), ({"ltf": 0x2008}, "ltf null or not 16-byte aligned"),
         ({"capture": None}, "capture null or not 16-byte aligned"),
         ({"capture": 0x1008}, "capture null or not 16-byte aligned")]
    for name in (("threshold_stf", "threshold_ltf") if stf else ("threshold",)):
        t += [({name: v}, name + " outside [0, 1]") for v in (-0.01, 1.01, NAN)]
    if stf:
        t += [({"cfo": None}, "cfo null or not 8-byte aligned"), ({"cfo": 0x5004}, "cfo null or not 8-byte aligned"),
              ({"metric_stf": 0x4004}, "metric not 8-byte aligned"), ({"metric_ltf": 0x6004}, "metric not 8-byte aligned")]
    else:
        t += [({"metric": 0x4004}, "metric not 8-byte aligned")]
    return rows("", t)


# ---------------------------------------------------------------- demodulation, tracking, decoding
def scale_rows(key):
    return [({key: v}, "scale not positive and finite") for v in (0.0, -1.0, INF, NAN)]


def demod_rows(name, track):
    outs = ["eq", "sym", "theta", "evm", "nerr"] + (["h_blocks", "h_last"] if track else [])
    t = [({"in": None}, "null frames, parameters or outputs"), ({"p": None}, "null frames, parameters or outputs"),
         ({"out": None}, "null frames, parameters or outputs"),
         ({"in.tx": None}, "tx/rx required"), ({"in.rx": None}, "tx/rx required"), ({"p.h": None}, "h required"),
         ({"out." + o: None for o in outs}, "no output requested"),
         ({"p.h_stride": 52}, "h_stride < 53"),
         ({"p.modulation": 3}, "unknown modulation"), ({"p.modulation": 0}, "unknown modulation"),
         ({"p.flags": 8 if track else 4}, "unknown flag bits"), *scale_rows("p.scale"),
         ({"out.eq_block_stride": 52}, "eq strides too small"),
         ({"out.eq_frame_stride": FS - 1}, "eq strides too small", N0),
         ({"out.sym_block_stride": 52}, "sym strides too small"),
         ({"out.sym_frame_stride": FS - 1}, "sym strides too small", N0),
         ({"out.theta": 0x7004}, "theta or evm not 8-byte aligned"), ({"out.evm": 0x8004}, "theta or evm not 8-byte aligned"),
         ({"out.nerr": 0x9002}, "nerr not 4-byte aligned")]
    if track:
        t += [({"p.mu": v}, "mu outside [0, 1]") for v in (-0.01, 1.01, NAN)]
        t += [({"p.beta": -1}, "beta outside 0..4"), ({"p.beta": 5}, "beta outside 0..4"),
              ({"out.hb_block_stride": 52}, "h_blocks strides too small"),
              ({"out.hb_frame_stride": FS - 1}, "h_blocks strides too small", N0),
              ({"out.h_last_stride": 52}, "h_last_stride < 53"),
              ({"p.h": 0x3008}, "h or eq not 16-byte aligned"), ({"out.eq": 0x5008}, "h or eq not 16-byte aligned"),
              ({"out.h_blocks": 0xa008}, "h_blocks or h_last not 16-byte aligned"),
              ({"out.h_last": 0xb008}, "h_blocks or h_last not 16-byte aligned")]
    else:
        t += [({k: v}, "h, h_lt or eq not 16-byte aligned")
              for k, v in (("p.h", 0x3008), ("p.h_lt", 0x4008), ("out.eq", 0x5008))]
    # the frames' own refusals come bare
    return rows(name + ": ", t) + rows("", [
        ({"in.n_frames": -1}, "n_frames < 0"),
        ({"in.n_frames": T31}, "n_frames > 2^31 - 1 (one wave per frame in a 1-D grid)"),
        ({"in.block_stride": 52}, "block_stride < 53", N0), ({"in.frame_stride": FS - 1}, "frame_stride too small", N0)])


N_ROWS = [({"n": -1}, "n_frames < 0 or > 2^31 - 1"), ({"n": T31}, "n_frames < 0 or > 2^31 - 1")]
LLR_ROWS = [({"llr_block_stride": 191}, "llr strides too small"),
            ({"llr_frame_stride": 14 * 192 + 191}, "llr strides too small", N0)]
EQ_ROWS = [({"eq_block_stride": 52}, "eq strides too small"), ({"eq_frame_stride": FS - 1}, "eq strides too small", N0)]

SOFT_DEMAP = rows("wce_soft_demap: ", [
    ({"eq": None}, "null eq, parameters or llr"), ({"p": None}, "null eq, parameters or llr"),
    ({"llr": None}, "null eq, parameters or llr"), ({"p.h": None}, "h required"), ({"p.h_stride": 52}, "h_stride < 53"),
    ({"p.modulation": 3}, "unknown modulation"), ({"p.modulation": 0}, "unknown modulation"),
    *scale_rows("p.scale"), *N_ROWS, *EQ_ROWS, *LLR_ROWS,
    ({"eq": 0x1008}, "eq, h or h_lt not 16-byte aligned"), ({"p.h": 0x3008}, "eq, h or h_lt not 16-byte aligned"),
    ({"p.h_lt": 0x4008}, "eq, h or h_lt not 16-byte aligned"), ({"llr": 0x5002}, "llr not 4-byte aligned")])

SOFT_DEMAP_BLOCKS = rows("wce_soft_demap_blocks: ", [
    ({"eq": None}, "null eq, hb or llr"), ({"hb": None}, "null eq, hb or llr"), ({"llr": None}, "null eq, hb or llr"),
    ({"modulation": 3}, "unknown modulation"), ({"modulation": 0}, "unknown modulation"),
    *scale_rows("scale"), *N_ROWS, *EQ_ROWS,
    ({"hb_block_stride": 52}, "hb strides too small"), ({"hb_frame_stride": FS - 1}, "hb strides too small", N0),
    *LLR_ROWS, ({"eq": 0x1008}, "eq or hb not 16-byte aligned"), ({"hb": 0x2008}, "eq or hb not 16-byte aligned"),
    ({"llr": 0x5002}, "llr not 4-byte aligned")])

VITERBI = rows("wce_viterbi_decode: ", [
    ({"llr": None}, "null llr"), ({"modulation": 3}, "unknown modulation or rate"),
    ({"rate": 3}, "unknown modulation or rate"), ({"rate": -1}, "unknown modulation or rate"),
    ({"flags": 2}, "unknown flag bits"), ({"bits": None, "nbiterr": None}, "no output requested"),
    ({"ref_bits": None}, "nbiterr needs ref_bits"), *N_ROWS, *LLR_ROWS,
    ({"bits_stride": 179}, "bits_stride < ceil(T / 8)"), ({"ref_stride": 179}, "ref_stride < ceil(T / 8)"),
    ({"llr": 0x1002}, "llr or nbiterr not 4-byte aligned"), ({"nbiterr": 0x4002}, "llr or nbiterr not 4-byte aligned")])

REENCODE = rows("wce_reencode: ", [
    ({"p": None}, "null parameters or outputs"), ({"out": None}, "null parameters or outputs"),
    ({"p.bits": None}, "bits required"), ({"out.tx": None, "out.h": None}, "no output requested"),
    ({"in": None}, "h needs the frames' rx"), ({"in.rx": None}, "h needs the frames' rx"),
    ({"n": -1, "in.n_frames": -1}, "n_frames < 0 or > 2^31 - 1"),
    ({"n": T31, "in.n_frames": T31}, "n_frames < 0 or > 2^31 - 1"),
    ({"in.n_frames": 4}, "the frames' n_frames differs from n_frames"),
    ({"p.modulation": 3}, "unknown modulation or rate"), ({"p.rate": 3}, "unknown modulation or rate"),
    *scale_rows("p.scale"), ({"p.bits_stride": 179}, "bits_stride < ceil(T / 8)"),
    ({"out.tx_block_stride": 52}, "tx strides too small"), ({"out.tx_frame_stride": FS - 1}, "tx strides too small", N0),
    ({"in.block_stride": 52}, "the frames' strides too small"),
    ({"in.frame_stride": FS - 1}, "the frames' strides too small", N0),
    ({"out.h_stride": 52}, "h_stride < 53"),
    *[({k: v}, "tx, h or the frames' rx or tx not 16-byte aligned")
      for k, v in (("out.tx", 0x5008), ("out.h", 0x6008), ("in.rx", 0x4008), ("in.tx", 0x3008))],
    ({"p.theta": 0x2004}, "theta not 8-byte aligned")])


# ---------------------------------------------------------------- receive diversity
COMBINE = rows("wce_combine: ", [
    ({"p": None}, "null parameters or outputs"), ({"out": None}, "null parameters or outputs"),
    ({"p.rx": None}, "rx and h required"), ({"p.h": None}, "rx and h required"),
    ({"out.rx": None, "out.h": None}, "no output requested"),
    ({"p.n_branches": 0}, "n_branches outside 1..8"), ({"p.n_branches": 9}, "n_branches outside 1..8"),
    ({"n_frames": -1}, "n_frames < 0 or > 2^31 - 1"), ({"n_frames": T31}, "n_frames < 0 or > 2^31 - 1"),
    ({"p.rx_block_stride": 52}, "rx strides too small"), ({"p.rx_frame_stride": FS - 1}, "rx strides too small", N0),
    ({"p.h_stride": 52}, "h_stride < 53"), ({"out.rx_block_stride": 52}, "output rx strides too small"),
    ({"out.rx_frame_stride": FS - 1}, "output rx strides too small", N0), ({"out.h_stride": 52}, "output h_stride < 53"),
    ({"p.rx_branch_stride": 3 * FS - 1}, "rx_branch_stride makes branches overlap", N0),
    ({"p.rx_branch_stride": 52}, "rx_branch_stride makes branches overlap"),
    ({"p.rx_branch_stride": -3 * FS}, "rx_branch_stride makes branches overlap"),
    ({"p.h_branch_stride": 3 * 53 - 1}, "h_branch_stride makes branches overlap", N0),
    ({"p.h_branch_stride": 52}, "h_branch_stride makes branches overlap"),
    ({"p.ow2_branch_stride": 2}, "ow2_branch_stride < n_frames", N0),
    *[({k: v}, "rx, h or an output not 16-byte aligned")
      for k, v in (("p.rx", 0x1008), ("p.h", 0x2008), ("out.rx", 0x4008), ("out.h", 0x5008))],
    ({"p.ow2": 0x3004}, "ow2 not 8-byte aligned")])

SYNC_SHARE = rows("wce_sync_share: ", [
    ({"metric": None}, "metric null or not 8-byte aligned"), ({"metric": 0x1004}, "metric null or not 8-byte aligned"),
    ({"start": None, "cfo": None}, "start and cfo both null"), ({"start": 0x2002}, "start not 4-byte aligned"),
    ({"cfo": 0x3004}, "cfo not 8-byte aligned"),
    ({"n_branches": 0}, "n_branches outside 1..8"), ({"n_branches": 9}, "n_branches outside 1..8"),
    ({"n_packets": -1}, "n_packets < 0 or > 2^31 - 1"), ({"n_packets": T31}, "n_packets < 0 or > 2^31 - 1"),
    ({"branch_stride": 66}, "branch_stride < n_packets", N0)])


# ---------------------------------------------------------------- framing the payload
def psdu_rows(framing):
    t = [({"p.modulation": 3}, "unknown modulation or rate"), ({"p.rate": 3}, "unknown modulation or rate"),
         ({"p.length": 3}, "length outside 4..max"), ({"p.length": 178}, "length outside 4..max"),
         ({"bits_stride": 179}, "bits_stride < ceil(T / 8)"), ({"p.lengths": 0x3002}, "lengths not 4-byte aligned"),
         *N_ROWS]
    if framing:
        t += [({"p.seed": 0}, "seed outside 1..127"), ({"p.seed": 128}, "seed outside 1..127")]
    return t


PSDU_FRAME = rows("wce_psdu_frame: ", [
    ({"p": None}, "null parameters or bits"), ({"bits": None}, "null parameters or bits"), *psdu_rows(True),
    ({"payload": None}, "payload NULL with length > 4 or with lengths"),
    ({"payload": None, "p.length": 4, "p.lengths": 0x3000}, "payload NULL with length > 4 or with lengths"),
    ({"payload_stride": 95}, "payload_stride < L - 4 (max - 4 with lengths)"),
    ({"payload_stride": 172, "p.lengths": 0x3000}, "payload_stride < L - 4 (max - 4 with lengths)")])

PSDU_DEFRAME = rows("wce_psdu_deframe: ", [
    ({"p": None}, "null parameters, bits or outputs"), ({"bits": None}, "null parameters, bits or outputs"),
    ({"out": None}, "null parameters, bits or outputs"),
    ({"out.psdu": None, "out.seed": None, "out.fcs_ok": None, "out.n_good": None}, "no output requested"),
    *psdu_rows(False), ({"out.psdu_stride": 99}, "psdu_stride < L (max with lengths)"),
    ({"out.psdu_stride": 176, "p.lengths": 0x3000}, "psdu_stride < L (max with lengths)"),
    ({"out.fcs_ok": 0x4002}, "fcs_ok or n_good not 4-byte aligned"),
    ({"out.n_good": 0x5002}, "fcs_ok or n_good not 4-byte aligned")])


# ---------------------------------------------------------------- transmitter and channel
FRAMES_ROWS = [({"n_frames": -1}, "n_frames < 0 or > 2^31 - 1"), ({"n_frames": T31}, "n_frames < 0 or > 2^31 - 1")]
SYMBOLS_ROWS = [   # check_symbols
    ({"n_blocks": -1}, "n_blocks outside 0..15"), ({"n_blocks": 16}, "n_blocks outside 0..15"),
    ({"tx_pre": None, "n_blocks": 0}, "no field and n_blocks == 0"), ({"sym": None}, "sym required"), *FRAMES_ROWS,
    ({"block_stride": 52}, "block_stride < 53"),
    ({"frame_stride": FS - 1}, "frame_stride < (n_blocks - 1) block_stride + 53", N0),
    ({"pre_stride": 52}, "pre_stride neither 0 nor >= 53"),
    ({"tx_pre": 0x1008}, "tx_pre or sym not 16-byte aligned"), ({"sym": 0x2008}, "tx_pre or sym not 16-byte aligned")]
CAPTURE_ROWS = [   # check_channel, the part check_fading shares
    ({"p": None}, "null parameters or capture"), ({"capture": None}, "null parameters or capture"),
    ({"p.n_taps": 0}, "n_taps outside 1..16"),
    ({"capture_len": 0}, "capture_len < 1 or >= 2^31"),
    ({"capture_len": T31, "capture_stride": T31}, "capture_len < 1 or >= 2^31"),
    ({"capture_stride": 1599}, "capture_stride < capture_len"),
    ({"capture": 0x6008}, "taps or capture not 16-byte aligned"),
    ({"p.cfo": 0x3004}, "cfo or ow2 not 8-byte aligned"), ({"p.ow2": 0x4004}, "cfo or ow2 not 8-byte aligned"),
    ({"p.delay": 0x5002}, "delay not 4-byte aligned")]
CHANNEL_ROWS = CAPTURE_ROWS + [   # check_channel
    ({"p.n_taps": 17, "p.taps_stride": 17}, "n_taps outside 1..16"),
    ({"p.taps_stride": 5}, "taps_stride neither 0 nor >= n_taps"),
    ({"p.taps": 0x2008}, "taps or capture not 16-byte aligned")]
FADING_ROWS = CAPTURE_ROWS + [   # check_fading
    ({"p.n_taps": 17, "p.knot_stride": 17}, "n_taps outside 1..16"),
    ({"p.knots": None}, "knots required"), ({"p.knots": 0x2008}, "knots not 16-byte aligned"),
    ({"p.n_knots": 1}, "n_knots < 2"),
    ({"p.knot_period": 15}, "knot_period outside 16..2^20"), ({"p.knot_period": 2 ** 20 + 1}, "knot_period outside 16..2^20"),
    ({"p.knot_stride": 5}, "knot_stride < n_taps"),
    ({"p.frame_stride": 113}, "frame_stride neither 0 nor >= (n_knots - 1) knot_stride + n_taps"),
    ({"p.n_knots": 18}, "the knots do not cover the output")]
WAVE_IN_ROWS = [   # the waveform wce_channel and wce_channel_tv read
    ({"wave": None}, "wave required"), ({"wave_len": 0}, "wave_len < 1 or >= 2^31"),
    ({"wave_len": T31, "wave_stride": T31}, "wave_len < 1 or >= 2^31"),
    ({"wave_stride": 1359}, "wave_stride < wave_len"), ({"wave": 0x1008}, "wave not 16-byte aligned")]

MODULATE = rows("wce_modulate: ", SYMBOLS_ROWS + [
    ({"wave": None}, "wave required"), ({"wave_stride": 1359}, "wave_stride < the waveform's length"),
    ({"wave": 0x3008}, "wave not 16-byte aligned")])


# ---------------------------------------------------------------- the calls
# name -> (parameters between ctx and stream: (name, the structure it points to or None), the count's argument(s),
#          the valid base call, the refusals)
def frames(W):
    return dict({f[0]: 0 for f in W.Frames._fields_}, tx=0x1000, rx=0x2000, frame_stride=FS, block_stride=53,
                n_frames=3)


DEMOD_PAR = dict(h=0x3000, h_lt=0x4000, h_stride=53, modulation=4, flags=0, scale=1.0)
DEMOD_OUT = dict(eq=0x5000, sym=0x6000, theta=0x7000, evm=0x8000, nerr=0x9000, eq_frame_stride=FS, eq_block_stride=53,
                 sym_frame_stride=FS, sym_block_stride=53)
SYMBOLS = dict(tx_pre=0x1000, pre_stride=53, sym=0x2000, frame_stride=FS, block_stride=53, n_blocks=15, n_frames=3)
SYMBOLS_PAR = [(k, None) for k in SYMBOLS]
CAPTURE = dict(capture=0x6000, capture_stride=1600, capture_len=1600)
WAVE_IN = dict(wave=0x1000, wave_stride=1360, wave_len=1360, n_frames=3)
SHARED_PAR = dict(field=1, cfo=0x3000, ow2=0x4000, delay=0x5000, seed=1, first_frame=0)
CHANNEL_PAR = dict(taps=0x2000, taps_stride=6, n_taps=6, **SHARED_PAR)
FADING_PAR = dict(knots=0x2000, frame_stride=0, knot_stride=6, n_knots=19, knot_period=80, n_taps=6, **SHARED_PAR)
SYNC = dict(capture=0x1000, capture_stride=400, capture_len=400, n_frames=3, ltf=0x2000)
AT = dict(capture=0x1000, capture_stride=400, capture_len=400, n_frames=3)
BLOCKS_OUT = dict(sym=0x2000, frame_stride=106, block_stride=53)


def plain(base):
    return [(k, None) for k in base]


def calls(W):
    c = {}

    def add(name, params, count, base, table):
        c[name] = (params, count, base, table)

    base = dict(samples=0x1000, packet_stride=160, n_frames=3, n_blocks=2, **BLOCKS_OUT)
    add("wce_front_end_blocks", plain(base), ["n_frames"], base, blocks_rows())
    base = dict(samples=0x1000, packet_stride=160, n_frames=3, n_blocks=2, cfo=0x3000, sample_offset=0, **BLOCKS_OUT)
    add("wce_front_end_blocks_cfo", plain(base), ["n_frames"], base, blocks_rows(cfo=True))
    base = dict(**AT, n_blocks=2, start=0x4000, cfo=0x3000, sample_offset=0, **BLOCKS_OUT)
    add("wce_front_end_blocks_at", plain(base), ["n_frames"], base, blocks_rows(at=True))
    base = dict(lptot=0x1000, lptot_stride=160, lptot_len=160, n_frames=3, pre_fft=0x2000, pre_stride=53, ow2=0x3000)
    add("wce_front_end_preamble", plain(base), ["n_frames"], base, preamble_rows())
    base = dict(**base, cfo=0x4000, estimate=1)
    add("wce_front_end_preamble_cfo", plain(base), ["n_frames"], base, preamble_rows(cfo=True))
    base = dict(**AT, start=0x4000, pre_fft=0x2000, pre_stride=53, ow2=0x3000, cfo=0x4000, estimate=1)
    add("wce_front_end_preamble_at", plain(base), ["n_frames"], base, preamble_rows(at=True))
    base = dict(**SYNC, threshold=0.5, backoff=4, start=0x3000, metric=0x4000)
    add("wce_front_end_sync", plain(base), ["n_frames"], base, sync_rows(False))
    base = dict(**SYNC, threshold_stf=0.5, threshold_ltf=0.5, backoff=4, start=0x3000, cfo=0x5000, metric_stf=0x4000,
                metric_ltf=0x6000)
    add("wce_front_end_sync_stf", plain(base), ["n_frames"], base, sync_rows(True))
    base = dict(amplitude=1.0, wave=0x1000, wave_stride=160, n_frames=3)
    add("wce_short_field", plain(base), ["n_frames"], base, rows("", [
        ({"n_frames": -1}, "n_frames < 0"), ({"wave": None}, "wave null or not 16-byte aligned"),
        ({"wave": 0x1008}, "wave null or not 16-byte aligned"), ({"wave_stride": 159}, "wave_stride < 160"),
        ({"amplitude": INF}, "amplitude not finite"), ({"amplitude": NAN}, "amplitude not finite")]))

    base = {"in": frames(W), "p": DEMOD_PAR, "out": DEMOD_OUT}
    add("wce_demodulate", [("in", W.Frames), ("p", W.Demod), ("out", W.DemodOut)], ["in.n_frames"], base,
        demod_rows("wce_demodulate", False))
    base = {"in": frames(W), "p": dict(h=0x3000, h_stride=53, modulation=4, flags=0, scale=1.0, mu=0.5, beta=2),
            "out": dict(DEMOD_OUT, h_blocks=0xa000, hb_frame_stride=FS, hb_block_stride=53, h_last=0xb000,
                        h_last_stride=53)}
    add("wce_track_demodulate", [("in", W.Frames), ("p", W.Track), ("out", W.TrackOut)], ["in.n_frames"], base,
        demod_rows("wce_track_demodulate", True))
    base = {"p": dict(rx=0x1000, rx_branch_stride=3 * FS, rx_frame_stride=FS, rx_block_stride=53, h=0x2000,
                      h_branch_stride=3 * 53, h_stride=53, ow2=0x3000, ow2_branch_stride=3, n_branches=2),
            "n_frames": 3, "out": dict(rx=0x4000, rx_frame_stride=FS, rx_block_stride=53, h=0x5000, h_stride=53)}
    add("wce_combine", [("p", W.CombinePar), ("n_frames", None), ("out", W.CombineOut)], ["n_frames"], base, COMBINE)
    base = dict(n_branches=2, branch_stride=67, n_packets=67, metric=0x1000, start=0x2000, cfo=0x3000)
    add("wce_sync_share", plain(base), ["n_packets"], base, SYNC_SHARE)

    llr = dict(llr=0x5000, llr_frame_stride=15 * 192, llr_block_stride=192)
    base = dict(eq=0x1000, eq_frame_stride=FS, eq_block_stride=53, p=DEMOD_PAR, n=3, **llr)
    add("wce_soft_demap", [(k, W.Demod if k == "p" else None) for k in base], ["n"], base, SOFT_DEMAP)
    base = dict(eq=0x1000, eq_frame_stride=FS, eq_block_stride=53, hb=0x2000, hb_frame_stride=FS, hb_block_stride=53,
                modulation=4, scale=1.0, n=3, **llr)
    add("wce_soft_demap_blocks", plain(base), ["n"], base, SOFT_DEMAP_BLOCKS)
    # 16-QAM at rate 1/2: T = 1440 information bits in 180 bytes, a PSDU of at most 177
    base = dict(llr=0x1000, llr_frame_stride=15 * 192, llr_block_stride=192, modulation=4, rate=0, flags=1, n=3,
                bits=0x2000, bits_stride=180, ref_bits=0x3000, ref_stride=180, nbiterr=0x4000)
    add("wce_viterbi_decode", plain(base), ["n"], base, VITERBI)
    base = {"p": dict(bits=0x1000, bits_stride=180, modulation=4, rate=0, scale=1.0, theta=0x2000),
            "in": dict(frames(W), tx=0x3000, rx=0x4000), "n": 3,
            "out": dict(tx=0x5000, tx_frame_stride=FS, tx_block_stride=53, h=0x6000, h_stride=53)}
    add("wce_reencode", [("p", W.ReencodePar), ("in", W.Frames), ("n", None), ("out", W.ReencodeOut)],
        ["n", "in.n_frames"], base, REENCODE)
    psdu = dict(modulation=4, rate=0, length=100, seed=93, lengths=None, seeds=None)
    base = dict(p=psdu, payload=0x1000, payload_stride=200, n=3, bits=0x2000, bits_stride=180)
    add("wce_psdu_frame", [(k, W.PsduPar if k == "p" else None) for k in base], ["n"], base, PSDU_FRAME)
    base = dict(p=psdu, bits=0x1000, bits_stride=180, n=3,
                out=dict(psdu=0x2000, psdu_stride=200, seed=0x3000, fcs_ok=0x4000, n_good=0x5000))
    add("wce_psdu_deframe", [("p", W.PsduPar), ("bits", None), ("bits_stride", None), ("n", None), ("out", W.PsduOut)],
        ["n"], base, PSDU_DEFRAME)

    base = dict(**SYMBOLS, wave=0x3000, wave_stride=1360)
    add("wce_modulate", plain(base), ["n_frames"], base, MODULATE)
    for name, par, struct, table in (("wce_channel", CHANNEL_PAR, W.ChannelPar, CHANNEL_ROWS),
                                     ("wce_channel_tv", FADING_PAR, W.FadingPar, FADING_ROWS)):
        base = dict(**WAVE_IN, p=par, **CAPTURE)
        add(name, [(k, struct if k == "p" else None) for k in base], ["n_frames"], base,
            rows(name + ": ", table + FRAMES_ROWS + WAVE_IN_ROWS))
    for name, par, struct, table in (("wce_transmit", CHANNEL_PAR, W.ChannelPar, CHANNEL_ROWS),
                                     ("wce_transmit_tv", FADING_PAR, W.FadingPar, FADING_ROWS)):
        base = dict(**SYMBOLS, p=par, **CAPTURE)
        add(name, [(k, struct if k == "p" else None) for k in base], ["n_frames"], base,
            rows(name + ": ", SYMBOLS_ROWS + table))
    return c


NAMES = ["wce_front_end_blocks", "wce_front_end_blocks_cfo", "wce_front_end_blocks_at", "wce_front_end_preamble",
         "wce_front_end_preamble_cfo", "wce_front_end_preamble_at", "wce_front_end_sync", "wce_front_end_sync_stf",
         "wce_short_field", "wce_demodulate", "wce_track_demodulate", "wce_combine", "wce_sync_share", "wce_soft_demap",
         "wce_soft_demap_blocks", "wce_viterbi_decode", "wce_reencode", "wce_psdu_frame", "wce_psdu_deframe",
         "wce_modulate", "wce_channel", "wce_transmit", "wce_channel_tv", "wce_transmit_tv"]


def changed(base, changes):
    args = {k: dict(v) if isinstance(v, dict) else v for k, v in base.items()}
    for key, v in changes.items():
        s, _, f = key.partition(".")
        if f:
            if args[s] is not None:   # a field of a structure the row passes as NULL
                args[s][f] = v
        else:
            args[s] = v
    return args


def call(lib, name, params, args, ctx=0x10):
    """the call with no stream; (return code, wce_last_error())"""
    vals = [args[k] if kind is None or args[k] is None else ctypes.byref(kind(**args[k])) for k, kind in params]
    rc = getattr(lib, name)(ctx, *vals, None)
    return rc, lib.wce_last_error().decode()


def test_every_chain_call_has_a_table(wce):
    assert sorted(calls(wce.wce)) == sorted(NAMES) and len(set(NAMES)) == 24
    for name, (params, count, base, table) in calls(wce.wce).items():
        assert len(params) + 2 == len(wce.wce.ABI[name]), name   # ctx and stream around them
        assert len(table) == len({(repr(sorted(ch.items())), text) for ch, _, text, _ in table}), name
    # the two sizes that go with them take no context
    lib = wce.load()
    assert (lib.wce_decode_info_bits(4, 0), lib.wce_psdu_max_len(4, 0)) == (1440, 177)
    for mod, rate in ((3, 0), (4, 3)):
        assert lib.wce_decode_info_bits(mod, rate) == EINVAL
        assert lib.wce_last_error().decode() == "wce_decode_info_bits: unknown modulation or rate"
        assert lib.wce_psdu_max_len(mod, rate) == EINVAL
        assert lib.wce_last_error().decode() == "wce_psdu_max_len: unknown modulation or rate"


@pytest.mark.parametrize("name", NAMES)
def test_refusals_before_the_ctx_is_touched(wce, name):
    lib = wce.load()
    params, count, base, table = calls(wce.wce)[name]
    zero = {k: 0 for k in count}
    assert call(lib, name, params, base, ctx=None) == (EINVAL, "null ctx")
    assert call(lib, name, params, changed(base, zero), ctx=None) == (EINVAL, "null ctx")
    assert call(lib, name, params, changed(base, zero))[0] == OK
    for changes, rc, text, at0 in table:
        assert call(lib, name, params, changed(base, changes)) == (rc, text), changes
        if set(changes) & set(count):
            continue   # the row is about the count itself
        got = call(lib, name, params, changed(base, {**changes, **zero}))
        assert got == ((rc, text) if at0 == AT0 else (OK, got[1])), (changes, at0)
