"""The gain laws of the library's calls: what a change of signal level by g = 2^k
must do to every output.  A receiver does not choose its level (int16 counts,
volts, unit power; two antennas run two AGCs), so no result may depend on it
beyond the factor its definition in include/wce.h carries.  A power of two
commutes with every IEEE rounding of + - x / sqrt fma while nothing overflows or
goes subnormal, so a law holds bit for bit: the reference of a row is the same
call at k = 0, and "the same" means the same bits.

LAWS is the table, one row per law.  A row names

    calls     the functions of include/wce.h it binds (the builder checks that the header declares each)
    inputs    name -> p: the input is multiplied by g^p
    outputs   name -> p: the output comes out multiplied by g^p (0: unchanged, bit for bit)
    ints      the outputs that are integers (plain equality; their power is 0)
    f32       the outputs stored as float (their level moves by g^p inside float's range)
    branch    the gain is one per antenna branch (axis 0 of every scaled input), not one for the call

tests/test_gain_model.py runs every row on the numpy models (which proves the
table and settles the gains a row may use), tests/test_gain_gpu.py on the device.
Both take their data from here: the low-SNR sets, where a decision sits near a
boundary and any inexactness flips it."""
import collections
import functools
import os
import re

import numpy as np

import cfo_model as cm
import combine_model as cb
import demod_model as dm
import fading_model as fd
import fec_model as fm
import reencode_model as rm
import stf_model as st
import sync_model as sm
import track_model as tk
import tx_model as tm

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "wce.h")
# 2^11: int16 full scale against unit scale.  2^+-40 moves a float soft bit by 2^+-80, inside float's normal range
# for the sets below (asserted where a row has float outputs).  2^+-100: rows whose outputs are all fp64.
GAINS = (-40, -11, 11, 40)
GAINS_F64 = (-100, 100)

Law = collections.namedtuple("Law", "key calls inputs outputs ints f32 branch")


def _law(key, calls, inputs, outputs, ints=(), f32=(), branch=False):
    assert all(outputs[n] == 0 for n in ints) and set(ints) | set(f32) <= set(outputs)
    return Law(key, tuple(calls.split()), dict(inputs), dict(outputs), tuple(ints), tuple(f32), branch)


_EST = ("lt_ls", "ps_linear", "ps_cubic", "ps_sinc", "ps_mmse")
_DEM0 = dict(eq=0, sym=0, theta=0, evm=0, nerr=0)
_SYNC0 = dict(start=0, metric=0)
_STF0 = dict(start=0, cfo=0, metric_stf=0, metric_ltf=0)

LAWS = [
    # ---- front end
    _law("blocks", "wce_front_end_blocks wce_front_end_blocks_cfo wce_front_end_blocks_at",
         dict(samples=1), dict(sym=1)),
    _law("preamble", "wce_front_end_preamble wce_front_end_preamble_cfo wce_front_end_preamble_at",
         dict(lptot=1), dict(pre_fft=1, ow2=2, cfo=0)),
    _law("sync/capture", "wce_front_end_sync", dict(capture=1), _SYNC0, ints=("start",)),
    _law("sync/ltf", "wce_front_end_sync", dict(ltf=1), _SYNC0, ints=("start",)),
    _law("sync_stf/capture", "wce_front_end_sync_stf", dict(capture=1), _STF0, ints=("start",)),
    _law("sync_stf/ltf", "wce_front_end_sync_stf", dict(ltf=1), _STF0, ints=("start",)),
    # ---- the estimators: the channel's gain, and the transmitter's convention
    _law("estimate/channel", "wce_estimate wce_estimate_noise",
         dict(rx=1, rx_pre=1, ctx_rx_pre=1, ctx_ow2=2, ow2=2, Rhh=2), dict({n: 1 for n in _EST}, eq=0)),
    _law("estimate/tx", "wce_estimate wce_estimate_noise",
         # (a COV context's model covariance is the channel's, which this convention divides by g: Rhh / g^2;
         # and the constant-modulus pattern x_ref is a transmitted symbol)
         dict(tx=1, tx_pre=1, ctx_tx_pre=1, Rhh=-2, x_ref=1), dict({n: -1 for n in _EST}, eq=1)),
    # ---- demodulators
    _law("demodulate/channel", "wce_demodulate", dict(rx=1, h=1, h_lt=1), _DEM0, ints=("sym", "nerr")),
    _law("demodulate/tx", "wce_demodulate", dict(tx=1, rx=1, scale=1), dict(_DEM0, eq=1), ints=("sym", "nerr")),
    _law("track/channel", "wce_track_demodulate", dict(rx=1, h=1), dict(_DEM0, h_blocks=1, h_last=1),
         ints=("sym", "nerr")),
    _law("track/tx", "wce_track_demodulate", dict(tx=1, rx=1, scale=1), dict(_DEM0, eq=1, h_blocks=0, h_last=0),
         ints=("sym", "nerr")),
    # ---- soft bits and the decoder
    _law("soft_demap/channel", "wce_soft_demap", dict(h=1, h_lt=1), dict(llr=2), f32=("llr",)),
    _law("soft_demap/tx", "wce_soft_demap", dict(eq=1, scale=1), dict(llr=2), f32=("llr",)),
    _law("soft_demap_blocks/channel", "wce_soft_demap_blocks", dict(hb=1), dict(llr=2), f32=("llr",)),
    _law("soft_demap_blocks/tx", "wce_soft_demap_blocks", dict(eq=1, scale=1), dict(llr=2), f32=("llr",)),
    _law("viterbi", "wce_viterbi_decode", dict(llr=1), dict(bits=0, nbiterr=0), ints=("bits", "nbiterr")),
    # ---- the re-encoder
    _law("reencode/channel", "wce_reencode", dict(rx=1), dict(tx=0, h=1)),
    _law("reencode/tx", "wce_reencode", dict(scale=1, pilots=1), dict(tx=1, h=-1)),
    # ---- diversity: each branch its own AGC (weighted), or one common gain (unit weights)
    _law("combine/weighted", "wce_combine", dict(rx=1, h=1, ow2=2), dict(rx_c=0, h_c=0), branch=True),
    _law("combine/unweighted", "wce_combine", dict(rx=1, h=1), dict(rx_c=1, h_c=1)),
    # ---- the transmit side
    _law("modulate", "wce_modulate", dict(sym=1, tx_pre=1), dict(wave=1)),
    _law("channel/taps", "wce_channel", dict(taps=1, ow2=2), dict(capture=1)),
    _law("channel/wave", "wce_channel", dict(wave=1, ow2=2), dict(capture=1)),
    _law("transmit/taps", "wce_transmit", dict(taps=1, ow2=2), dict(capture=1)),
    _law("transmit/sym", "wce_transmit", dict(sym=1, tx_pre=1, ow2=2), dict(capture=1)),
    _law("channel_tv/knots", "wce_channel_tv", dict(knots=1, ow2=2), dict(capture=1)),
    _law("transmit_tv/knots", "wce_transmit_tv", dict(knots=1, ow2=2), dict(capture=1)),
    _law("transmit_tv/sym", "wce_transmit_tv", dict(sym=1, tx_pre=1, ow2=2), dict(capture=1)),
    _law("short_field", "wce_short_field", dict(amplitude=1), dict(wave=1)),
]
BY_KEY = {l.key: l for l in LAWS}
assert len(BY_KEY) == len(LAWS)


def declared_calls():
    """the functions include/wce.h declares"""
    with open(HEADER) as f:
        return set(re.findall(r"^int (wce_\w+)\(", f.read(), re.M))


def gains(law, narrow=False):
    """the k of g = 2^k a row runs at; narrow: a run whose outputs include floats (WCE_OUT_LS_F32)"""
    return GAINS if (law.f32 or law.ints or narrow) else GAINS + GAINS_F64


def branch_gains(k, A):
    """a row with a gain per branch: +k, -k, +k ... over the branches"""
    return np.array([k if a % 2 == 0 else -k for a in range(A)])


def times(a, p, k):
    """a g^p with g = 2^k, exact; k [A]: one gain per branch along axis 0 of an array.  A complex array is scaled
    part by part: numpy's complex product with g + 0i would turn a part of -0 into +0"""
    e = np.asarray(p * np.asarray(k), np.int64)
    assert np.all(np.abs(e) < 1000)
    if not np.ndim(a):
        return float(a) * float(np.ldexp(1.0, int(np.max(e))))
    a = np.asarray(a)
    g = np.ldexp(1.0, e).reshape(e.shape + (1,) * (a.ndim - e.ndim))
    if a.dtype.kind == "c":
        out = np.empty(a.shape, a.dtype)
        out.real, out.imag = a.real * g, a.imag * g
        return out
    return (a * g).astype(a.dtype)


def scaled(law, args, k):
    """args with the row's inputs multiplied by their powers of 2^k (inputs the args lack are skipped)"""
    out = dict(args)
    for n, p in law.inputs.items():
        if out.get(n) is not None:
            out[n] = times(out[n], p, k)
    return out


def expected(law, base, k, name):
    """output `name` of the k = 0 run as the law moves it"""
    p = law.outputs[name]
    assert p == 0 or not law.branch
    return np.asarray(base[name]) if p == 0 else times(base[name], p, k)


def same_bits(a, b):
    """the same type, shape, values and signs of zero (long double has padding bytes, so the values are compared,
    not the storage; a NaN matches a NaN whatever its payload)"""
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    if a.dtype.kind == "c":
        return same_bits(a.real, b.real) and same_bits(a.imag, b.imag)
    if a.dtype.kind != "f":
        return np.array_equal(a, b)
    return bool(np.all(((a == b) & (np.signbit(a) == np.signbit(b))) | (np.isnan(a) & np.isnan(b))))


def normal(a, dtype):
    """every finite non-zero value of `a` is a normal number of `dtype` (neither overflowed nor subnormal)"""
    a = np.abs(np.asarray(a, np.longdouble).ravel())
    a = a[np.isfinite(a) & (a != 0)]
    fi = np.finfo(dtype)
    return bool(np.all((a >= np.longdouble(fi.tiny)) & (a <= np.longdouble(fi.max))))


def check(law, run, args, k, names=None, tolerant=None, base=None):
    """run(args) at k = 0 and with the inputs moved by 2^k: every output the law names (and the run returns) moved
    as the law says, bit for bit (base: the k = 0 run, where the caller has it).  tolerant: name -> bound, the outputs
    held within |got - want| <= bound (library functions only; tests/test_gain_gpu.py's table).  -> the names that differ (empty: the law holds)"""
    base = run(args) if base is None else base
    got = run(scaled(law, args, k))
    bad = []
    for n in (names or law.outputs):
        if n not in base:
            continue
        want = expected(law, base, k, n)
        if n in law.ints:
            ok = np.array_equal(np.asarray(got[n]), want)
        elif tolerant and n in tolerant:
            with np.errstate(invalid="ignore"):
                d = np.abs(np.asarray(got[n], np.longdouble) - np.asarray(want, np.longdouble))
            ok = bool(np.all((d <= tolerant[n]) | (np.isnan(got[n]) & np.isnan(want))))
        else:
            ok = same_bits(np.asarray(got[n]), want)
        if not ok:
            bad.append(n)
    return bad


def first(args, n, axis=0, whole=("ltf", "tx_pre1")):
    """the first n frames of every per-frame array of a set (`axis`: where the frames are)"""
    out = {}
    for k, v in args.items():
        if isinstance(v, np.ndarray) and v.ndim > axis and v.shape[axis] >= n and k not in whole:
            v = np.ascontiguousarray(v[(slice(None),) * axis + (slice(0, n),)])
        out[k] = v
    return out


# ---------------------------------------------------------------- the data: the existing low-SNR sets
DEMOD_SETS = rm.LOW_SNR                                   # (modulation, rate, dB)
DECODE_SETS = ((dm.BPSK, fm.RATE_1_2), (dm.QAM16, fm.RATE_2_3), (dm.QAM64, fm.RATE_3_4))
COMBINE_A = 3


def c128(a):
    return np.ascontiguousarray(np.asarray(a).astype(np.complex128))


@functools.lru_cache(maxsize=None)
def demod_set(mod, rate, snr):
    """reencode_model's low-SNR frames: tx, rx, h (the noisy first estimate), h_lt (the channel itself, DC 0)"""
    s = rm.low_snr_set(mod, rate, snr)
    h_lt = np.array(s["H"])
    h_lt[:, dm.DC] = 0
    return dict(tx=s["tx"], rx=s["rx"], h=s["h0"], h_lt=h_lt, mod=mod, scale=dm.SCALE)


@functools.lru_cache(maxsize=None)
def track_set(mod):
    """the tracker's rho = 0.995 set"""
    snr = dict(tk.SETS)[mod]
    tx, rx, h = tk.drifting(mod, snr_db=snr)
    return dict(tx=tx, rx=rx, h=h, mod=mod, scale=dm.SCALE)


@functools.lru_cache(maxsize=None)
def demap_set(mod, rate, snr):
    """the low-SNR frames' equalized symbols (the fp64 model's, tracked and blended) with their estimates, and the
    model tracker's per-block estimates hb of the same frames for wce_soft_demap_blocks"""
    s = demod_set(mod, rate, snr)
    eq = c128(dm.demodulate(s["tx"], s["rx"], s["h"], s["h_lt"], mod, real=np.float64)["eq"])
    hb = c128(tk.track(s["tx"], s["rx"], s["h"], mod, real=np.float64)["h_blocks"])
    return dict(eq=eq, h=s["h"], h_lt=s["h_lt"], hb=hb, mod=mod, scale=dm.SCALE)


@functools.lru_cache(maxsize=None)
def reencode_set(mod, rate, snr):
    """the low-SNR frames' information bits, received symbols and the model demodulator's block phases"""
    s = rm.low_snr_set(mod, rate, snr)
    theta = np.asarray(dm.demodulate(s["tx"], s["rx"], s["h0"], None, mod, real=np.float64)["theta"], np.float64)
    return dict(u=s["u"], rx=s["rx"], theta=theta, pilots=rm.standard_pilots(len(s["u"])), mod=mod, rate=rate,
                scale=dm.SCALE)


@functools.lru_cache(maxsize=None)
def combine_set():
    """combine_model's unequal branches: each next branch 3 dB noisier"""
    tx, rx, h, ow2 = cb.parity_set(COMBINE_A)
    return dict(rx=rx, h=h, ow2=ow2)


SYNC_SHAPE = (777, 488)        # sync_model's (B, L); the first 67 windows are used
STF_SHAPE = (488, 67)          # stf_model's (L, B)


@functools.lru_cache(maxsize=None)
def sync_set():
    cap, _ = sm.shape_set(*SYNC_SHAPE)
    return dict(capture=np.ascontiguousarray(cap[:67, :SYNC_SHAPE[1]]), ltf=sm.clean_ltf(), threshold=0.25)


@functools.lru_cache(maxsize=None)
def stf_set():
    cap, _, ltf = st.shape_set(*STF_SHAPE)
    return dict(capture=cap, ltf=ltf, threshold_stf=st.THR_STF, threshold_ltf=st.THR_LTF)


@functools.lru_cache(maxsize=None)
def front_set(B=67):
    """cfo_model's long training fields (offsets within +-1/128, 10 to 60 dB) and packets of noise-like samples"""
    rng = np.random.default_rng(0x6A17)
    lp, eps, _ = cm.ltf_batch(rng, B)
    return dict(lptot=np.ascontiguousarray(lp[:, :160]), samples=cm.random_packets(rng, B, 1400), eps=eps,
                start=(np.arange(B) * 5 % 64).astype(np.int32))


@functools.lru_cache(maxsize=None)
def tx_set(B=67, nb=15):
    """tx_model's (B, 15, field) shape with per-frame preambles, six taps, an offset, a delay and noise; and moving
    knots (fading_model's) for the time-varying pair"""
    sym, pre = tm.shape_set(B, nb, 1)
    rng = np.random.default_rng(0x6A18)
    S = 160 + 80 * nb
    K = fd.min_knots(S, 6, 80)
    return dict(sym=sym, tx_pre=pre, taps=tm.random_taps(rng, B, 6), cfo=rng.uniform(-0.002, 0.002, B),
                ow2=np.full(B, float(tm.nominal_ow2(20.0))) * rng.uniform(0.5, 2.0, B),
                delay=rng.integers(-20, 60, B).astype(np.int32), knots=fd.moving_knots(rng, B, K, 6), n_knots=K,
                capture_len=1488, seed=tm.SEED)
