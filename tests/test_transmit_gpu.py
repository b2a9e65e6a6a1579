"""wce_modulate, wce_channel and wce_transmit on the device against the long double
model of tests/tx_model.py, at the tolerances tests/test_transmit_abi.py derives;
the fused call against the pair, bit for bit; the guard; the refusals on real
buffers; and the whole chain, bits -> capture windows -> bits, on one stream.

Measured on an MI355X: waveform 1.4e-16 to 3.7e-16 of the frame's largest sample
(TOL_WAVE 1e-14); noise 7.7e-16 sqrt(ow2) (TOL_NOISE 2e-14); the fused capture
against the model, from the symbols on, at most 0.08 of its tolerance; the
chain's offset estimates within 1.13e-5 cycles per sample, as the model's."""

import numpy as np
import pytest

import cfo_model as cm
import fec_model as fm
import sync_model as sm
import tx_model as tm
from tx_model import base_args, call_abi, refusals

pytestmark = pytest.mark.gpu
TOL_FE = 1e-14
SENT = sm.SENT
LENS = (None, 1397, 1488, 129)     # None: the exact fit, S + n_taps - 1


@pytest.fixture(scope="module")
def ctx(gpu_wce):
    pre = tm.chain_pre()
    c = gpu_wce.Context(pre, pre, 1e-6, gpu_wce.MMSE_TEXTBOOK)
    yield c
    c.close()


def dev(wce, a):
    return None if a is None else wce.DeviceArray.from_numpy(np.ascontiguousarray(a))


def padded_sym(sym, bs, fs):
    """[B][nb][53] -> [B][fs] with block stride bs, SENT in the padding"""
    B, nb = sym.shape[:2]
    out = np.full((B, fs), SENT, np.complex128)
    for b in range(nb):
        out[:, b * bs:b * bs + 53] = sym[:, b]
    return out


class Layout:
    """a shape's device inputs with padded strides"""

    def __init__(self, wce, B, nb, field, per_frame_pre=True):
        self.B, self.nb, self.field = B, nb, field
        self.sym, self.pre = tm.shape_set(B, nb, field, per_frame_pre)
        self.S = 160 * field + 80 * nb
        self.bs, self.fs = 57, max(nb, 1) * 57 + 3
        self.dsym = dev(wce, padded_sym(self.sym, self.bs, self.fs)) if nb else None
        self.ps = 0
        self.dpre = None
        if field:
            self.ps = 55 if per_frame_pre else 0
            self.dpre = dev(wce, tm.padded(self.pre, 55) if per_frame_pre else self.pre)
        self.sym_kw = dict(n_blocks=nb, tx_pre=self.dpre, pre_stride=self.ps, frame_stride=self.fs,
                           block_stride=self.bs)


def run_modulate(wce, ctx, lay, pad=5):
    out = dev(wce, np.full((lay.B, lay.S + pad), SENT, np.complex128))
    ctx.modulate(lay.dsym, lay.B, out, wave_stride=lay.S + pad, **lay.sym_kw)
    wce.synchronize()
    return out.numpy()


def chan_inputs(wce, B, taps=None, shared_taps=False, cfo=None, ow2=None, delay=None):
    """-> (keywords for channel / transmit, the device arrays they point to)"""
    kw, keep = {}, []
    if taps is not None:
        taps = np.asarray(taps, np.complex128)
        nt = taps.shape[-1]
        d = dev(wce, taps if shared_taps else tm.padded(taps, nt + 1))
        kw.update(taps=d, n_taps=nt, taps_stride=0 if shared_taps else nt + 1)
        keep.append(d)
    for name, v, dt in (("cfo", cfo, np.float64), ("ow2", ow2, np.float64), ("delay", delay, np.int32)):
        if v is not None:
            d = dev(wce, np.broadcast_to(np.asarray(v, dt), (B,)))
            kw[name] = d
            keep.append(d)
    return kw, keep


def run_channel(wce, ctx, wave, L, field=True, pad=3, seed=tm.SEED, first_frame=0, **chan):
    wave = np.asarray(wave, np.complex128)
    B, S = wave.shape
    kw, keep = chan_inputs(wce, B, **chan)
    dw = dev(wce, tm.padded(wave, S + 2))
    out = dev(wce, np.full((B, L + pad), SENT, np.complex128))
    ctx.channel(dw, B, S, out, L, field=field, seed=seed, first_frame=first_frame, wave_stride=S + 2,
                capture_stride=L + pad, **kw)
    wce.synchronize()
    return out.numpy()


def run_transmit(wce, ctx, lay, L, pad=3, seed=tm.SEED, first_frame=0, **chan):
    kw, keep = chan_inputs(wce, lay.B, **chan)
    out = dev(wce, np.full((lay.B, L + pad), SENT, np.complex128))
    ctx.transmit(lay.dsym, lay.B, out, L, seed=seed, first_frame=first_frame, capture_stride=L + pad, **lay.sym_kw,
                 **kw)
    wce.synchronize()
    return out.numpy()


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


# ---------------------------------------------------------------- 1. modulate
@pytest.mark.parametrize("B,nb,field", tm.SHAPES)
def test_modulate_against_the_model(gpu_wce, ctx, B, nb, field):
    for per_frame in ((True, False) if field else (True,)):
        lay = Layout(gpu_wce, B, nb, field, per_frame)
        got = run_modulate(gpu_wce, ctx, lay)
        assert np.all(got[:, lay.S:] == SENT)
        wave = got[:, :lay.S]
        ref = tm.modulate(lay.sym, lay.pre)
        err = float(tm.relmax_rows(wave, ref).max())
        print(f"B={B} nb={nb} field={field} per-frame pre={per_frame}: {err:.2e}")
        assert err <= tm.TOL_WAVE
        # the copies are the bits of their sources
        if field:
            assert same_bits(wave[:, 32:96], wave[:, 96:160]) and same_bits(wave[:, :32], wave[:, 64:96])
        blocks = wave[:, 160 * field:].reshape(B, nb, 80)
        assert same_bits(blocks[:, :, :16], blocks[:, :, 64:])
        # round trip through the front end
        dw = dev(gpu_wce, got)
        if nb:
            dsym = gpu_wce.DeviceArray((B, nb, 53), zero=True)
            ctx.front_end_blocks(dw.addr + 16 * 160 * field, B, nb, dsym, packet_stride=got.shape[1],
                                 frame_stride=nb * 53)
            gpu_wce.synchronize()
            assert cm.relmax(dsym.numpy(), lay.sym) <= TOL_FE
        if field:
            dpre, dow2 = gpu_wce.DeviceArray((B, 53), zero=True), dev(gpu_wce, np.ones(B))
            ctx.front_end_preamble(dw, B, 160, dpre, dow2, lptot_stride=got.shape[1])
            gpu_wce.synchronize()
            assert cm.relmax(dpre.numpy(), np.broadcast_to(lay.pre, (B, 53))) <= TOL_FE
            assert np.all(dow2.numpy() == 0.0)


# ---------------------------------------------------------------- 2. channel without noise
@pytest.fixture(scope="module")
def waves():
    """clean waveforms for the channel's tests: the long double model's, rounded; (15, 1) and (1, 0), B = 9"""
    out = {}
    for nb, field in ((15, 1), (1, 0)):
        sym, pre = tm.shape_set(9, nb, field)
        out[field] = np.asarray(tm.modulate(sym, pre), np.complex128)
    return out


def check_capture(got, ref, tol, L, what):
    """got [B][L + pad] against the model's [B][L]: per frame within tol of the frame's largest clean output"""
    assert np.all(got[:, L:] == SENT), what
    for f in range(len(ref)):
        scale = tol["scale"][f]
        err = float(np.max(np.abs(got[f, :L].astype(np.clongdouble) - ref[f]))) / scale
        assert err <= tol["tol"][f], (what, f, err, tol["tol"][f])


def capture_tol(wave, taps, cfo, field, with_wave=False):
    B, S = wave.shape
    nt = 1 if taps is None else np.shape(taps)[-1]
    full = tm.channel(wave, S + nt - 1, taps=taps, field=field, cfo=cfo)
    return {"scale": np.max(np.abs(full), axis=1).astype(np.float64),
            "tol": tm.cap_tol(wave, taps, cfo, full, field, with_wave)}


@pytest.mark.parametrize("field", (1, 0))
def test_channel_taps(gpu_wce, ctx, waves, field):
    wave = waves[field]
    B, S = wave.shape
    rng = np.random.default_rng(0x7C10 + field)
    # a unit tap, given or implied: the input, bit for bit
    for taps in (None, np.ones((B, 1))):
        got = run_channel(gpu_wce, ctx, wave, S, field, taps=taps)
        assert same_bits(got[:, :S], wave) and np.all(got[:, S:] == SENT)
    # a unit tap delayed: the input shifted
    delta = np.zeros(4, complex)
    delta[3] = 1
    got = run_channel(gpu_wce, ctx, wave, S + 3, field, taps=delta, shared_taps=True)
    assert np.array_equal(got[:, 3:S + 3], wave) and np.all(got[:, :3] == 0) and np.all(got[:, S + 3:] == SENT)
    # 2 and 16 random taps, per frame and shared, every window length
    for nt, shared in ((2, False), (16, False), (16, True)):
        taps = tm.random_taps(rng, B, nt)
        taps = taps[0] if shared else taps
        tol = capture_tol(wave, taps, None, field)
        for L in LENS:
            L = S + nt - 1 if L is None else L
            got = run_channel(gpu_wce, ctx, wave, L, field, taps=taps, shared_taps=shared)
            check_capture(got, tm.channel(wave, L, taps=taps, field=field), tol, L, (nt, shared, L))


def test_channel_offsets(gpu_wce, ctx, waves):
    rng = np.random.default_rng(0x7C20)
    for field in (1, 0):
        wave = waves[field]
        B, S = wave.shape
        taps = tm.random_taps(rng, B, 6)
        L = S + 5
        none = run_channel(gpu_wce, ctx, wave, L, field, taps=taps)
        zero = run_channel(gpu_wce, ctx, wave, L, field, taps=taps, cfo=np.zeros(B))
        assert same_bits(none, zero)
        cfo = np.resize([0.002, -0.002, 0.0077, 0.0, -0.0077], B)
        got = run_channel(gpu_wce, ctx, wave, L, field, taps=taps, cfo=cfo)
        check_capture(got, tm.channel(wave, L, taps=taps, field=field, cfo=cfo), capture_tol(wave, taps, cfo, field),
                      L, ("cfo", field))
        assert same_bits(got[3], none[3])                 # a zero offset among others: the product is skipped
        # the time origin: the sample 160 [field] of a unit-tap frame is not turned
        one = run_channel(gpu_wce, ctx, wave, S, field, cfo=cfo)
        k = 160 * field
        assert same_bits(one[:, k], wave[:, k]) and not same_bits(one[:3, k + 40], wave[:3, k + 40])


def test_channel_delays(gpu_wce, ctx, waves):
    wave = waves[1]
    B, S = wave.shape
    taps = tm.random_taps(np.random.default_rng(0x7C30), B, 6)
    tol = capture_tol(wave, taps, 0.002, 1)
    for L in (1397, 1488, 129):
        delay = np.array([0, 37, -50, L + 5, L - 100, -(S + 5) + 1, -(S + 5), L - 1, 2 ** 31 - 1][:B], np.int64)
        delay = delay.astype(np.int32)
        got = run_channel(gpu_wce, ctx, wave, L, 1, taps=taps, cfo=0.002, delay=delay)
        ref = tm.channel(wave, L, taps=taps, field=1, cfo=0.002, delay=delay)
        check_capture(got, ref, tol, L, ("delay", L))
        assert np.all(got[3, :L] == 0) and np.all(got[6, :L] == 0) and np.all(got[8, :L] == 0)   # beyond the window
        assert np.any(got[5, :L] != 0) and np.all(got[5, 1:L] == 0)                            # the very last sample
        assert np.any(got[7, L - 1] != 0) and np.all(got[7, :L - 1] == 0)
    minimum = np.full(B, -2 ** 31, np.int64).astype(np.int32)
    assert np.all(run_channel(gpu_wce, ctx, wave, 129, 1, taps=taps, delay=minimum)[:, :129] == 0)


# ---------------------------------------------------------------- 3. noise
def test_noise(gpu_wce, ctx, waves):
    B, L = tm.NOISE_B, tm.NOISE_L
    ow2 = np.random.default_rng(0x7C50).uniform(0.5, 2.0, B) * 1e-3
    ow2[5] = 0.0
    silent = np.zeros((B, 80), complex)
    # the signal off: a zero tap
    got = run_channel(gpu_wce, ctx, silent + 1.0, L, 0, taps=np.zeros(1), shared_taps=True, ow2=ow2)
    ref = tm.noise(B, L, ow2)
    assert np.all(got[:, L:] == SENT)
    with np.errstate(invalid="ignore", divide="ignore"):
        err = np.abs(got[:, :L].astype(np.clongdouble) - ref) / np.sqrt(ow2)[:, None]
    err[5] = 0
    print(f"noise: {float(err.max()):.2e} sqrt(ow2)")
    assert float(err.max()) <= tm.TOL_NOISE
    assert np.all(got[5, :L] == 0)
    # a shard, and one frame alone, are the rows of the batch
    shard = run_channel(gpu_wce, ctx, silent[:27] + 1.0, L, 0, taps=np.zeros(1), shared_taps=True, ow2=ow2[40:],
                        first_frame=40)
    assert same_bits(shard, got[40:])
    # with a signal: ow2 == 0 frames are the noiseless bits; two channels under one seed differ by their signals
    wave = waves[1]
    b, S = wave.shape
    rng = np.random.default_rng(0x7C51)
    o = np.resize([1e-3, 0.0, 2e-3], b)
    caps = []
    for _ in range(2):
        taps = tm.random_taps(rng, b, 6)
        quiet = run_channel(gpu_wce, ctx, wave, 1488, 1, taps=taps, cfo=0.002, delay=37)
        loud = run_channel(gpu_wce, ctx, wave, 1488, 1, taps=taps, cfo=0.002, delay=37, ow2=o)
        assert same_bits(loud[1::3], quiet[1::3]) and not same_bits(loud[0], quiet[0])
        caps.append((quiet, loud))
    d_loud, d_quiet = caps[0][1] - caps[1][1], caps[0][0] - caps[1][0]
    assert float(np.max(np.abs(d_loud - d_quiet))) <= 8 * tm.U * float(np.max(np.abs(caps[0][1])))
    # position independence: frame 3 of 9 alone, given first_frame = 3
    taps = tm.random_taps(rng, b, 6)
    full = run_channel(gpu_wce, ctx, wave, 1488, 1, taps=taps, cfo=0.002, delay=37, ow2=o)
    alone = run_channel(gpu_wce, ctx, wave[3:4], 1488, 1, taps=taps[3:4], cfo=0.002, delay=37, ow2=o[3:4],
                        first_frame=3)
    assert same_bits(alone[0], full[3])


# ---------------------------------------------------------------- 4. transmit is modulate + channel
@pytest.mark.parametrize("B,nb,field", tm.SHAPES)
def test_transmit_is_the_pair_bit_for_bit(gpu_wce, ctx, B, nb, field):
    rng = np.random.default_rng(0x7C60 + B + nb)
    worst = 0.0
    for nt, per_frame, L in ((1, True, None), (2, False, 1397), (16, True, 1488), (16, True, 129), (16, False, None)):
        if not field and not per_frame:
            continue
        lay = Layout(gpu_wce, B, nb, field, per_frame)
        L = lay.S + nt - 1 if L is None else L
        taps = tm.random_taps(rng, B, nt)
        chan = dict(taps=taps[0] if not per_frame else taps, shared_taps=not per_frame,
                    cfo=rng.uniform(-0.002, 0.002, B), ow2=rng.uniform(0.5, 2.0, B) * 1e-4,
                    delay=rng.integers(-20, 60, B) if L > lay.S else None, first_frame=11)
        fused = run_transmit(gpu_wce, ctx, lay, L, **chan)
        wave = run_modulate(gpu_wce, ctx, lay)[:, :lay.S]
        pair = run_channel(gpu_wce, ctx, wave, L, field, **chan)
        assert same_bits(fused, pair), (nt, per_frame, L)
        assert np.all(fused[:, L:] == SENT)
        # and the model's capture, from the symbols on
        kw = {k: v for k, v in chan.items() if k != "shared_taps"}
        ref = tm.transmit(lay.sym, L, lay.pre, **kw)
        nokw = dict(kw, ow2=None, delay=None)
        full = tm.transmit(lay.sym, lay.S + nt - 1, lay.pre, **nokw)
        scale = np.max(np.abs(full), axis=1).astype(np.float64)
        tol = tm.cap_tol(np.asarray(tm.modulate(lay.sym, lay.pre), np.complex128), chan["taps"], chan["cfo"], full,
                         field) + tm.TOL_NOISE * np.sqrt(chan["ow2"]) / scale
        err = np.max(np.abs(fused[:, :L].astype(np.clongdouble) - ref), axis=1).astype(np.float64) / scale
        worst = max(worst, float(np.max(err / tol)))
        assert np.all(err <= tol), (nt, per_frame, L, float(np.max(err / tol)))
    print(f"B={B} nb={nb} field={field}: fused against the model at most {worst:.2f} of its tolerance")


def test_transmit_host(gpu_wce, ctx):
    """the numpy convenience: fused or not the same bits, the model's capture, scalars broadcast, the default length"""
    sym, pre = tm.shape_set(9, 7, 1, False)
    taps = tm.random_taps(np.random.default_rng(0x7C68), 9, 6)
    ow2 = np.resize([1e-4, 0.0, 3e-4], 9)
    kw = dict(taps=taps, cfo=0.0015, ow2=ow2, delay=-3, seed=77, first_frame=5)
    fused = ctx.transmit_host(sym, pre, **kw)
    pair = ctx.transmit_host(sym, pre, fused=False, **kw)
    S = 160 + 7 * 80
    assert fused.shape == (9, S + 5) and same_bits(fused, pair)
    ref = tm.transmit(sym, S + 5, pre, **kw)
    full = tm.transmit(sym, S + 5, pre, taps=taps, cfo=0.0015)
    scale = np.max(np.abs(full), axis=1).astype(np.float64)
    tol = tm.cap_tol(np.asarray(tm.modulate(sym, pre), np.complex128), taps, 0.0015, full) + \
        tm.TOL_NOISE * np.sqrt(ow2) / scale
    err = np.max(np.abs(fused.astype(np.clongdouble) - ref), axis=1).astype(np.float64) / scale
    assert np.all(err <= tol), float(np.max(err / tol))
    # no preamble, one shared tap set, a longer window
    got = ctx.transmit_host(sym[:, :1], taps=taps[0], capture_len=129)
    check_capture(tm.padded(got, 129), tm.channel(tm.modulate(sym[:, :1]), 129, taps=taps[0], field=0),
                  capture_tol(np.asarray(tm.modulate(sym[:, :1]), np.complex128), taps[0], None, 0, True), 129, "host")
    with pytest.raises(ValueError):
        ctx.transmit_host(np.zeros((2, 16, 53)))


# ---------------------------------------------------------------- 5. guard and refusals
def test_guard(gpu_wce, ctx):
    B, L = 9, 1488
    lay = Layout(gpu_wce, B, 15, 1, per_frame_pre=False)
    rng = np.random.default_rng(0x7C70)
    taps = tm.random_taps(rng, B, 6)
    taps[:, 1:] *= 0.1                       # the first path is the strongest: sync's start is compared exactly
    chan = dict(taps=taps, cfo=rng.uniform(-0.002, 0.002, B), ow2=np.full(B, 1e-4), delay=np.full(B, 37))
    clean = run_transmit(gpu_wce, ctx, lay, L, **chan)
    assert np.isfinite(clean[:, :L]).all()
    wave = run_modulate(gpu_wce, ctx, lay)[:, :lay.S]
    ltf = dev(gpu_wce, wave[0, 32:96])

    def poisoned(frame, fused, got):
        assert np.all(np.isnan(got[frame, :L].real) & np.isnan(got[frame, :L].imag)), (frame, fused)
        assert np.all(got[frame, L:] == SENT)
        keep = np.arange(B) != frame
        assert same_bits(got[keep], clean[keep]), (frame, fused)
        start, metric = dev(gpu_wce, np.zeros(B, np.int32)), dev(gpu_wce, np.zeros(B))
        ctx.front_end_sync(dev(gpu_wce, got), B, L, ltf, 0.25, 0, start, metric, capture_stride=got.shape[1])
        gpu_wce.synchronize()
        s = start.numpy()
        assert s[frame] == -1 and np.all(s[keep] == 37 + 32), s

    cases = []
    for name, idx, value in (("ow2", 1, np.nan), ("ow2", 2, -1e-4), ("ow2", 8, np.inf), ("cfo", 3, np.inf),
                             ("cfo", 0, np.nan), ("taps", 4, np.nan)):
        c = {k: np.array(v, copy=True) for k, v in chan.items()}
        if name == "taps":
            c["taps"][idx, 5] = value
        else:
            c[name][idx] = value
        cases.append((idx, c))
    for idx, c in cases:
        poisoned(idx, True, run_transmit(gpu_wce, ctx, lay, L, **c))
        poisoned(idx, False, run_channel(gpu_wce, ctx, wave, L, 1, **c))
    # a NaN symbol (fused), a NaN sample of the waveform (the channel alone); an Inf preamble bin
    sym = lay.sym.copy()
    sym[6, 14, 52] = np.nan
    bad = Layout(gpu_wce, B, 15, 1, per_frame_pre=False)
    bad.dsym = dev(gpu_wce, padded_sym(sym, bad.bs, bad.fs))
    poisoned(6, True, run_transmit(gpu_wce, ctx, bad, L, **chan))
    w = wave.copy()
    w[6, 1359] = np.nan
    poisoned(6, False, run_channel(gpu_wce, ctx, w, L, 1, **chan))
    pre = tm.padded(np.tile(lay.pre, (B, 1)), 55)      # the shared preamble, per frame
    pre[7, 0] = np.inf
    bad = Layout(gpu_wce, B, 15, 1, per_frame_pre=False)
    bad.dpre = dev(gpu_wce, pre)
    bad.sym_kw.update(tx_pre=bad.dpre, pre_stride=55)
    poisoned(7, True, run_transmit(gpu_wce, ctx, bad, L, **chan))


def test_refusals_write_nothing(gpu_wce, ctx):
    lib, W = gpu_wce.load(), gpu_wce.wce
    buf = {n: dev(gpu_wce, np.full(3 * 1500, SENT, np.complex128)) for n in ("taps", "pre", "sym", "wave", "capture")}
    small = {n: dev(gpu_wce, np.zeros(4)) for n in ("cfo", "ow2", "delay")}
    ptrs = {n: d.addr for n, d in {**buf, **small}.items()}
    table = refusals(W, **ptrs)
    for name, kw, text in table:
        rc = call_abi(W, lib, ctx.handle, name, kw)
        msg = lib.wce_last_error().decode()
        assert rc == -1 and msg.startswith(name) and text in msg, (name, text, msg)
    gpu_wce.synchronize()
    for n, d in buf.items():
        assert np.all(d.numpy() == SENT), n
    for name, kw in base_args(W, **ptrs)[1].items():
        assert call_abi(W, lib, ctx.handle, name, {**kw, "n_frames": 0}) == 0
    gpu_wce.synchronize()
    assert np.all(buf["capture"].numpy() == SENT) and np.all(buf["wave"].numpy() == SENT)


# ---------------------------------------------------------------- 6. the chain
@pytest.mark.parametrize("mod,rate", tm.CHAIN)
def test_chain(gpu_wce, ctx, mod, rate):
    wce = gpu_wce
    c = tm.chain_set(mod, rate)
    B, L, T = 5, tm.CHAIN_LEN, fm.info_bits(mod, rate)
    pre = tm.chain_pre()
    dbits = dev(wce, fm.pack(c["bits"]))
    dtx, dpre = wce.DeviceArray((B, 15, 53), zero=True), dev(wce, pre)
    dfield, dcap = wce.DeviceArray((160,), zero=True), wce.DeviceArray((B, L), zero=True)
    kw, keep = chan_inputs(wce, B, taps=c["taps"], cfo=c["cfo"], ow2=c["ow2"], delay=c["delay"])
    dstart, dmetric = dev(wce, np.zeros(B, np.int32)), dev(wce, np.zeros(B))
    dow2, dcfo = dev(wce, np.zeros(B)), dev(wce, np.zeros(B))
    drx, drxpre = wce.DeviceArray((B, 15, 53), zero=True), wce.DeviceArray((B, 53), zero=True)
    dh = wce.DeviceArray((B, 53), zero=True)
    deq, dllr = wce.DeviceArray((B, 15, 53), zero=True), wce.DeviceArray((B, 15, 48 * mod), np.float32, zero=True)
    dnerr = dev(wce, np.zeros(B, np.uint32))
    # one (null) stream, nothing read back in between
    ctx.reencode(dbits, B, mod, rate, tx=dtx)
    ctx.modulate(None, 1, dfield, 0, dpre)
    ctx.transmit(dtx, B, dcap, L, tx_pre=dpre, seed=c["seed"], **kw)
    ctx.front_end_sync(dcap, B, L, dfield.addr + 32 * 16, tm.CHAIN_THRESHOLD, 0, dstart, dmetric)
    ctx.front_end_preamble(dcap, B, L, drxpre, dow2, cfo=dcfo, start=dstart)
    ctx.front_end_blocks(dcap, B, 15, drx, cfo=dcfo, start=dstart, capture_len=L)
    fr = ctx.frames(dtx, drx, B, rx_pre=drxpre, tx_pre=dpre)
    out = wce.Outputs(dh.addr, None, None, None, None, None, 53, 15 * 53, 53, wce.PS_LINEAR, 0)
    ctx.estimate(fr, out, wce.LT_LS)
    ctx.demodulate(fr, dh, None, 53, mod, tm.SCALE, True, True, eq=deq)
    ctx.soft_demap(deq, dh, B, None, 53, mod, tm.SCALE, dllr)
    ctx.viterbi_decode(dllr, B, mod, rate, True, ref_bits=dbits, nbiterr=dnerr)
    wce.synchronize()
    start, cfo, nerr = dstart.numpy(), dcfo.numpy(), dnerr.numpy()
    d_cfo = float(np.max(np.abs(cfo - c["cfo"])))
    print(f"mod {mod} rate {rate}: start {start}, cfo error {d_cfo:.2e}, bit errors {nerr}")
    assert np.array_equal(start, c["delay"] + 32)
    assert d_cfo <= tm.CHAIN_CFO_TOL
    assert np.all(nerr == 0)
    # the same experiment through link_host: its own bits, the same channel
    res = ctx.link_host(mod, rate, tm.CHAIN_SNR, B, taps=c["taps"], cfo=c["cfo"], delay=c["delay"], capture_len=L,
                        threshold=tm.CHAIN_THRESHOLD, seed=c["seed"])
    assert np.array_equal(res["start"], c["delay"] + 32)
    assert np.array_equal(res[wce.LT_LS], nerr)
    assert res["bits"].shape == (B, T) and np.all(res["bits"][:, -6:] == 0)
    for s in (wce.PS_LINEAR, wce.PS_MMSE):
        assert res[s].shape == (B,) and res[s].dtype == np.uint32 and np.all(res[s] <= T)
    assert np.allclose(res["ow2"], c["ow2"], rtol=1e-15)


def test_link_host_reports_an_undetected_packet(gpu_wce, ctx):
    wce = gpu_wce
    mod, rate = tm.CHAIN[0]
    c = tm.chain_set(mod, rate)
    delay = c["delay"].copy()
    delay[2] = -200                          # the field lies before the window: data blocks and no field to detect
    res = ctx.link_host(mod, rate, tm.CHAIN_SNR, 5, sources=(wce.LT_LS,), taps=c["taps"], cfo=c["cfo"], delay=delay,
                        capture_len=tm.CHAIN_LEN, seed=c["seed"])
    assert res["start"][2] == -1 and np.all(np.delete(res["start"], 2) == np.delete(delay, 2) + 32)
    T = fm.info_bits(mod, rate)
    assert 0 < res[wce.LT_LS][2] <= T and np.all(np.delete(res[wce.LT_LS], 2) == 0)
    assert res[wce.LT_LS][2] == np.sum(res["bits"][2])     # an all-zero decode: every 1 sent is an error
    # decision-directed rounds, a scalar offset and per-frame SNRs run; LT_LS's count stays 0 at 30 dB and more
    res = ctx.link_host(mod, rate, np.linspace(30.0, 40.0, 5), 5, sources=(wce.LT_LS, wce.PS_LINEAR), taps=c["taps"],
                        cfo=0.001, delay=c["delay"], capture_len=tm.CHAIN_LEN, seed=c["seed"], dd_iterations=1)
    assert np.all(res[wce.LT_LS] == 0) and np.all(res[wce.PS_LINEAR] <= T)
    assert np.allclose(res["ow2"], tm.nominal_ow2(np.linspace(30.0, 40.0, 5)), rtol=1e-15)
