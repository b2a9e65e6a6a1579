"""wce_channel_tv and wce_transmit_tv on the device: constant knots against the static
calls, bit for bit; moving knots against the long double model of tests/fading_model.py
at cap_tol_tv (tests/test_fading_abi.py confirms the bound); the fused call against the
pair; the guard, the refusals, shards, the frame loop and 64-bit indexing; and the link
experiment the calls exist for, bits -> a fading channel -> tracked and static bit errors,
through Context.link_host.

Measured on an MI355X: channel_tv with moving knots at most 0.17 of cap_tol_tv (P = 16,
37, 80 and one segment; B = 1, 9, 67), 0.12 over the six tiles of a 3,000-sample waveform,
the fused call from the symbols on at most 0.05 of its tolerance.  The link experiment:
every packet detected at the model's start; LT_LS 4,264 bit errors of 96,480 static and
695 tracked, the model's counts; PS_MMSE 47,898 and 47,880 on this context (printed, not
asserted); frozen knots 0 and 0."""
import contextlib

import numpy as np
import pytest

import fading_model as fd
import sync_model as sm
import test_chain_bigindex_gpu as big
import test_transmit_gpu as ttx
import tx_model as tm
from test_transmit_gpu import Layout, chan_inputs, dev, run_channel, run_modulate, run_transmit, same_bits

pytestmark = pytest.mark.gpu
SENT = sm.SENT
KNOT_CASES = ((16, None), (37, None), (80, 19), (1500, 2))      # (P, n_knots; None: the smallest that covers)


@pytest.fixture(scope="module")
def ctx(gpu_wce):
    pre = tm.chain_pre()
    c = gpu_wce.Context(pre, pre, 1e-6, gpu_wce.MMSE_TEXTBOOK)
    yield c
    c.close()


def knot_inputs(wce, knots, P, shared=False):
    """knots [B][K][nt] (or [K][nt], shared) on the device with padded strides -> the knot keywords"""
    a = np.asarray(knots, np.complex128)
    K, nt = a.shape[-2:]
    ks = nt + 1
    fs = (K - 1) * ks + nt + 2
    d = dev(wce, fd.padded_knots(a[None] if shared else a, ks, fs))
    return dict(knots=d, n_knots=K, knot_period=P, n_taps=nt, knot_stride=ks, knots_frame_stride=0 if shared else fs)


def run_channel_tv(wce, ctx, wave, L, kn, field=True, pad=3, seed=tm.SEED, first_frame=0, **chan):
    wave = np.asarray(wave, np.complex128)
    B, S = wave.shape
    kw, keep = chan_inputs(wce, B, **chan)
    dw = dev(wce, tm.padded(wave, S + 2))
    out = dev(wce, np.full((B, L + pad), SENT, np.complex128))
    ctx.channel_tv(dw, B, S, out, L, field=field, seed=seed, first_frame=first_frame, wave_stride=S + 2,
                   capture_stride=L + pad, **kn, **kw)
    wce.synchronize()
    return out.numpy()


def run_transmit_tv(wce, ctx, lay, L, kn, pad=3, seed=tm.SEED, first_frame=0, **chan):
    kw, keep = chan_inputs(wce, lay.B, **chan)
    out = dev(wce, np.full((lay.B, L + pad), SENT, np.complex128))
    ctx.transmit_tv(lay.dsym, lay.B, out, L, seed=seed, first_frame=first_frame, capture_stride=L + pad,
                    **lay.sym_kw, **kn, **kw)
    wce.synchronize()
    return out.numpy()


def n_knots(S, nt, P, K):
    return fd.min_knots(S, nt, P) if K is None else K


# ---------------------------------------------------------------- 1. constant knots are the static call
@pytest.mark.parametrize("B,nb,field", tm.SHAPES)
def test_constant_knots_are_the_static_call(gpu_wce, ctx, B, nb, field):
    wce = gpu_wce
    rng = np.random.default_rng(0xFA10 + B + nb)
    lay = Layout(wce, B, nb, field)
    wave = run_modulate(wce, ctx, lay)[:, :lay.S]
    L = lay.S + 100
    for nt in (1, 6, 16):
        taps = tm.random_taps(rng, B, nt)
        chan = dict(cfo=rng.uniform(-0.002, 0.002, B), ow2=rng.uniform(0.5, 2.0, B) * 1e-4,
                    delay=rng.integers(-40, 120, B), first_frame=11)
        static_c = run_channel(wce, ctx, wave, L, field, taps=taps, **chan)
        static_t = run_transmit(wce, ctx, lay, L, taps=taps, **chan)
        assert same_bits(static_c, static_t)
        for P, K in KNOT_CASES:
            K = n_knots(lay.S, nt, P, K)
            kn = knot_inputs(wce, np.repeat(taps[:, None, :], K, axis=1), P)
            got_c = run_channel_tv(wce, ctx, wave, L, kn, field, **chan)
            got_t = run_transmit_tv(wce, ctx, lay, L, kn, **chan)
            assert same_bits(got_c, static_c), ("channel_tv", nt, P, K)       # the sentinels behind every row too
            assert same_bits(got_t, static_t), ("transmit_tv", nt, P, K)
        # one trajectory for all frames: frame 0's taps for everyone
        kn = knot_inputs(wce, np.repeat(taps[:1], 19, axis=0), 80, shared=True)
        got = run_transmit_tv(wce, ctx, lay, L, kn, **chan)
        assert same_bits(got, run_transmit(wce, ctx, lay, L, taps=taps[0], shared_taps=True, **chan)), nt


# ---------------------------------------------------------------- 2. moving knots against the model
def place(full, L, delay):
    """the model's outputs [B][n] -> windows [B][L], output 0 at delay[f]: tx_model.channel's placement"""
    B, n = full.shape
    cap = np.zeros((B, L), full.dtype)
    for f, d in enumerate(np.broadcast_to(0 if delay is None else np.asarray(delay), (B,))):
        lo, hi = max(int(d), 0), min(int(d) + n, L)
        if hi > lo:
            cap[f, lo:hi] = full[f, lo - int(d):hi - int(d)]
    return cap


def check_tv(got, wave, knots, P, L, field, what, cfo=None, ow2=None, delay=None, seed=tm.SEED, first_frame=0,
             with_wave=False, full=None):
    """got [B][L + pad] within cap_tol_tv of the long double model (`full`: its unplaced outputs, where the caller
    has them already), the model's noise subtracted; -> (the largest error over its tolerance, full)"""
    B, S = wave.shape
    nt = np.shape(knots)[-1]
    if full is None:
        full = fd.channel_tv(wave, S + nt - 1, knots, P, field=field, cfo=cfo)
    scale = np.max(np.abs(full), axis=1).astype(np.float64)
    tol = fd.cap_tol_tv(wave, knots, cfo, full, field, with_wave)
    d = got[:, :L].astype(np.clongdouble) - place(full, L, delay)
    if ow2 is not None:
        d = d - tm.noise(B, L, ow2, seed, first_frame)
        tol = tol + tm.TOL_NOISE * np.sqrt(np.broadcast_to(ow2, (B,))) / scale
    err = np.max(np.abs(d), axis=1).astype(np.float64) / scale
    assert np.all(got[:, L:] == SENT), what
    assert np.all(err <= tol), (what, float(np.max(err / tol)))
    return float(np.max(err / tol)), full


@pytest.mark.parametrize("B", (1, 9, 67))
def test_moving_knots_against_the_model(gpu_wce, ctx, B):
    wce = gpu_wce
    rng = np.random.default_rng(0xFA20 + B)
    sym, pre = tm.shape_set(B, 15, 1)
    wave = np.asarray(tm.modulate(sym, pre), np.complex128)
    S, L = wave.shape[1], 1397
    delay = np.resize([-37, 0, 5, 100], B)         # runs unaligned with the segments, clipped on both sides
    worst = 0.0
    for P, nt, shared, cfo in ((16, 16, False, 0.002), (37, 1, True, None), (37, 16, False, -0.0077),
                               (80, 16, True, 0.002), (80, 6, False, None), (1500, 6, False, 0.002)):
        K = fd.min_knots(S, nt, P)
        knots = fd.moving_knots(rng, B, K, nt, shared)
        kn = knot_inputs(wce, knots, P, shared)
        what = (B, P, nt, shared)
        quiet = run_channel_tv(wce, ctx, wave, L, kn, 1, cfo=cfo, delay=delay)
        r, full = check_tv(quiet, wave, knots, P, L, 1, what, cfo=cfo, delay=delay)
        worst = max(worst, r)
        ow2 = rng.uniform(0.5, 2.0, B) * 1e-4
        loud = run_channel_tv(wce, ctx, wave, L, kn, 1, cfo=cfo, delay=delay, ow2=ow2, first_frame=5)
        check_tv(loud, wave, knots, P, L, 1, what, cfo=cfo, delay=delay, ow2=ow2, first_frame=5, full=full)
        assert not same_bits(loud, quiet)
    print(f"B={B}: channel_tv against the model at most {worst:.2f} of cap_tol_tv")


# ---------------------------------------------------------------- 3. a long waveform: per-tile staging, the seams
def test_long_waveform(gpu_wce, ctx):
    wce = gpu_wce
    rng = np.random.default_rng(0xFA30)
    B, S = 3, 3000
    wave = rng.standard_normal((B, S)) + 1j * rng.standard_normal((B, S))
    delay = np.array([0, 5, -37])
    for P, nt in ((16, 16), (16, 1), (37, 6)):
        K = fd.min_knots(S, nt, P)
        assert P != 16 or K in (189, 190)
        knots = fd.moving_knots(rng, B, K, nt)
        kn = knot_inputs(wce, knots, P)
        L = S + nt - 1 + 20                       # six tiles
        got = run_channel_tv(wce, ctx, wave, L, kn, 0, cfo=0.0005, delay=delay)
        r = check_tv(got, wave, knots, P, L, 0, ("long", P, nt), cfo=0.0005, delay=delay)[0]
        print(f"wave_len {S}, P={P}, {K} knots, {nt} taps: {r:.2f} of cap_tol_tv")


# ---------------------------------------------------------------- 4. transmit_tv is modulate + channel_tv
@pytest.mark.parametrize("B,nb,field", tm.SHAPES)
def test_transmit_tv_is_the_pair_bit_for_bit(gpu_wce, ctx, B, nb, field):
    wce = gpu_wce
    rng = np.random.default_rng(0xFA40 + B + nb)
    lay = Layout(wce, B, nb, field)
    wave = run_modulate(wce, ctx, lay)[:, :lay.S]
    worst = 0.0
    for (P, K), nt, shared, L in zip(KNOT_CASES, (16, 6, 16, 1), (False, True, False, False), (None, 1397, 1488, 129)):
        K = n_knots(lay.S, nt, P, K)
        L = lay.S + nt - 1 if L is None else L
        knots = fd.moving_knots(rng, B, K, nt, shared)
        kn = knot_inputs(wce, knots, P, shared)
        chan = dict(cfo=rng.uniform(-0.002, 0.002, B), ow2=rng.uniform(0.5, 2.0, B) * 1e-4,
                    delay=rng.integers(-20, 60, B) if L > lay.S else None, first_frame=11)
        fused = run_transmit_tv(wce, ctx, lay, L, kn, **chan)
        pair = run_channel_tv(wce, ctx, wave, L, kn, field, **chan)
        assert same_bits(fused, pair), (P, K, nt, shared, L)
        # and the model's capture, from the symbols on
        ideal = np.asarray(tm.modulate(lay.sym, lay.pre), np.complex128)
        worst = max(worst, check_tv(fused, ideal, knots, P, L, field, (P, nt), with_wave=True, **chan)[0])
    print(f"B={B} nb={nb} field={field}: fused against the model at most {worst:.2f} of its tolerance")


def test_transmit_host_routes_knots(gpu_wce, ctx):
    """3-D taps, and 2-D ones with knot_period, go through the time-varying calls; fused or not the same bits"""
    sym, pre = tm.shape_set(9, 7, 1, False)
    rng = np.random.default_rng(0xFA48)
    S = 160 + 7 * 80
    knots = fd.moving_knots(rng, 9, fd.min_knots(S, 6, 80), 6)
    kw = dict(cfo=0.0015, ow2=np.resize([1e-4, 0.0, 3e-4], 9), delay=-3, seed=77, first_frame=5)
    fused = ctx.transmit_host(sym, pre, taps=knots, **kw)                    # knot_period None: 80
    assert fused.shape == (9, S + 5) and same_bits(fused, ctx.transmit_host(sym, pre, taps=knots, fused=False, **kw))
    check_tv(tm.padded(fused, S + 5), np.asarray(tm.modulate(sym, pre), np.complex128), knots, 80, S + 5, 1, "host",
             with_wave=True, **kw)
    shared = ctx.transmit_host(sym, pre, taps=knots[0], knot_period=80, **kw)
    assert same_bits(shared[0], fused[0]) and not same_bits(shared[1], fused[1])
    # 2-D taps without knot_period stay per-frame static taps
    per_frame = ctx.transmit_host(sym, pre, taps=knots[:, 0], **kw)
    assert same_bits(per_frame, ctx.transmit_host(sym, pre, taps=np.repeat(knots[:, :1], knots.shape[1], 1), **kw))
    with pytest.raises(gpu_wce.WceError):
        ctx.transmit_host(sym, pre, taps=knots[:, :9], **kw)                 # the knots do not cover the output


# ---------------------------------------------------------------- 5. guard
def test_guard(gpu_wce, ctx):
    wce = gpu_wce
    B, L = 9, 1488
    lay = Layout(wce, B, 15, 1, per_frame_pre=False)
    rng = np.random.default_rng(0xFA50)
    knots = fd.moving_knots(rng, B, 19, 6)
    delay = np.full(B, 37)
    delay[3] = 600                              # frame 3's window ends at output 887: knots 12 .. 18 are beyond it
    chan = dict(cfo=rng.uniform(-0.002, 0.002, B), ow2=np.full(B, 1e-4), delay=delay)
    wave = run_modulate(wce, ctx, lay)[:, :lay.S]
    clean = run_transmit_tv(wce, ctx, lay, L, knot_inputs(wce, knots, 80), **chan)
    assert np.isfinite(clean[:, :L]).all()

    def poisoned(frame, what, got):
        assert np.all(np.isnan(got[frame, :L].real) & np.isnan(got[frame, :L].imag)), (frame, what)
        assert np.all(got[frame, L:] == SENT)
        keep = np.arange(B) != frame
        assert same_bits(got[keep], clean[keep]), (frame, what)

    def both(frame, what, k=knots, c=chan):
        kn = knot_inputs(wce, k, 80)
        poisoned(frame, (what, "fused"), run_transmit_tv(wce, ctx, lay, L, kn, **c))
        poisoned(frame, (what, "pair"), run_channel_tv(wce, ctx, wave, L, kn, 1, **c))

    for frame, k, t, value in ((1, 0, 0, np.nan), (2, 18, 5, np.inf), (3, 15, 2, np.nan), (8, 7, 3, -np.inf * 1j),
                               (0, 18, 0, np.nan)):
        bad = knots.copy()
        bad[frame, k, t] = value
        both(frame, ("knot", k, t), k=bad)
    for name, idx, value in (("ow2", 1, np.nan), ("ow2", 2, -1e-4), ("ow2", 8, np.inf), ("cfo", 3, np.inf),
                             ("cfo", 0, np.nan)):
        c = {n: np.array(v, copy=True) for n, v in chan.items()}
        c[name][idx] = value
        both(idx, (name, value), c=c)
    kn = knot_inputs(wce, knots, 80)
    sym = lay.sym.copy()
    sym[6, 14, 52] = np.nan
    bad = Layout(wce, B, 15, 1, per_frame_pre=False)
    bad.dsym = dev(wce, ttx.padded_sym(sym, bad.bs, bad.fs))
    poisoned(6, "symbol", run_transmit_tv(wce, ctx, bad, L, kn, **chan))
    w = wave.copy()
    w[6, 1359] = np.nan
    poisoned(6, "sample", run_channel_tv(wce, ctx, w, L, kn, 1, **chan))
    # a shared trajectory with a bad knot: every window
    bad = knots[0].copy()
    bad[18, 5] = np.nan
    got = run_transmit_tv(wce, ctx, lay, L, knot_inputs(wce, bad, 80, shared=True), **chan)
    assert np.isnan(got[:, :L]).all() and np.all(got[:, L:] == SENT)


# ---------------------------------------------------------------- 6. refusals
def test_refusals_write_nothing(gpu_wce, ctx):
    lib, W = gpu_wce.load(), gpu_wce.wce
    buf = {n: dev(gpu_wce, np.full(3 * 1500, SENT, np.complex128)) for n in ("knots", "pre", "sym", "wave", "capture")}
    small = {n: dev(gpu_wce, np.zeros(4)) for n in ("cfo", "ow2", "delay")}
    ptrs = {n: d.addr for n, d in {**buf, **small}.items()}
    for name, kw, text in fd.refusals(W, **ptrs):
        rc = fd.call_abi(W, lib, ctx.handle, name, kw)
        msg = lib.wce_last_error().decode()
        assert rc == -1 and msg.startswith(name + ":") and text in msg, (name, text, msg)
    gpu_wce.synchronize()
    for n, d in buf.items():
        assert np.all(d.numpy() == SENT), n
    for name, kw in fd.base_args(W, **ptrs)[1].items():
        assert fd.call_abi(W, lib, ctx.handle, name, {**kw, "n_frames": 0}) == 0
    gpu_wce.synchronize()
    assert np.all(buf["capture"].numpy() == SENT) and np.all(buf["wave"].numpy() == SENT)


# ---------------------------------------------------------------- 7. shards
def test_shards(gpu_wce, ctx):
    wce = gpu_wce
    B, L, lo, hi = 67, 1488, 23, 50
    rng = np.random.default_rng(0xFA70)
    lay = Layout(wce, B, 15, 1)
    knots = fd.moving_knots(rng, B, 19, 6)
    chan = dict(cfo=rng.uniform(-0.002, 0.002, B), ow2=rng.uniform(0.5, 2.0, B) * 1e-4, delay=rng.integers(0, 100, B))
    full = run_transmit_tv(wce, ctx, lay, L, knot_inputs(wce, knots, 80), **chan)
    part = Layout(wce, hi - lo, 15, 1)
    part.dsym = dev(wce, ttx.padded_sym(lay.sym[lo:hi], part.bs, part.fs))
    part.dpre = dev(wce, tm.padded(lay.pre[lo:hi], 55))
    part.sym_kw.update(tx_pre=part.dpre)
    sub = {k: v[lo:hi] for k, v in chan.items()}
    kn = knot_inputs(wce, knots[lo:hi], 80)
    assert same_bits(run_transmit_tv(wce, ctx, part, L, kn, first_frame=lo, **sub), full[lo:hi])
    assert not same_bits(run_transmit_tv(wce, ctx, part, L, kn, first_frame=lo + 1, **sub), full[lo:hi])
    wave = run_modulate(wce, ctx, lay)[:, :lay.S]
    assert same_bits(run_channel_tv(wce, ctx, wave[lo:hi], L, kn, 1, first_frame=lo, **sub), full[lo:hi])


# ---------------------------------------------------------------- 8. the frame loop
@contextlib.contextmanager
def three_workgroups(wce):
    lib = wce.load()
    try:
        assert lib.wce_debug_set_variant(6, 1) == 0          # WCE_VARIANT_GRID: chain kernels launch three workgroups
        yield
    finally:
        assert lib.wce_debug_set_variant(6, 0) == 0


@pytest.mark.parametrize("B", (67, 13))
def test_frame_loop(gpu_wce, ctx, B):
    """Under the knob a workgroup takes frames g, g + 3, g + 6, ...: what one frame leaves in LDS (staged knots, the
    waveform, the tile's sums) would show in the frame three on.  A frame with a non-finite knot is followed by a
    clean one, and the delays alternate between windows that hold the whole packet, its head, its tail and nothing,
    so that a frame that stages no knots at all follows one that staged many."""
    wce = gpu_wce
    rng = np.random.default_rng(0xFA80 + B)
    lay = Layout(wce, B, 15, 1)
    wave = run_modulate(wce, ctx, lay)[:, :lay.S]
    L = 1488
    delay = np.resize([0, 600, -700, 37, 1600, -1300, 90, -1400, 100, 1487], B)
    chan = dict(cfo=rng.uniform(-0.002, 0.002, B), ow2=rng.uniform(0.5, 2.0, B) * 1e-4, delay=delay, first_frame=3)
    for P, nt, shared in ((16, 16, False), (80, 6, False), (80, 6, True), (37, 1, False)):
        knots = fd.moving_knots(rng, B, fd.min_knots(lay.S, nt, P), nt, shared)
        if not shared:
            knots[1, 0, 0] = np.nan
            knots[min(8, B - 1), -1, nt - 1] = np.inf
        kn = knot_inputs(wce, knots, P, shared)
        want_t = run_transmit_tv(wce, ctx, lay, L, kn, **chan)
        want_c = run_channel_tv(wce, ctx, wave, L, kn, 1, **chan)
        assert same_bits(want_t, want_c)
        with three_workgroups(wce):
            got_t = run_transmit_tv(wce, ctx, lay, L, kn, **chan)
            got_c = run_channel_tv(wce, ctx, wave, L, kn, 1, **chan)
        assert same_bits(got_t, want_t), ("transmit_tv", P, nt, shared)
        assert same_bits(got_c, want_c), ("channel_tv", P, nt, shared)
        if not shared:
            assert np.isnan(want_t[1, :L]).all() and np.isfinite(want_t[4, :L]).all()


# ---------------------------------------------------------------- 9. the link experiment
def test_link_experiment(gpu_wce, ctx):
    wce = gpu_wce
    c = fd.link_set()
    model = fd.link_model()
    call = dict(cfo=c["cfo"], delay=c["delay"], capture_len=fd.LINK_LEN, threshold=tm.CHAIN_THRESHOLD, seed=c["seed"],
                sources=(wce.LT_LS, wce.PS_MMSE))
    res = ctx.link_host(fd.LINK_MOD, fd.LINK_RATE, fd.LINK_SNR, fd.LINK_B, taps=c["taps"], knot_period=fd.LINK_P,
                        tracker=(fd.LINK_MU, fd.LINK_BETA), **call)
    assert np.array_equal(res["bits"], c["bits"])
    assert np.all(res["start"] >= 0)
    t = res["tracked"]
    assert set(t) == {wce.LT_LS, wce.PS_MMSE}
    for s in t:
        assert t[s].shape == (fd.LINK_B,) and t[s].dtype == np.uint32
    print(f"link, {c['bits'].size} bits, rho {fd.LINK_RHO}: LT_LS static {int(res[wce.LT_LS].sum())} tracked "
          f"{int(t[wce.LT_LS].sum())} (model: static {int(model['static'].sum())} tracked "
          f"{int(model['tracked'].sum())}); PS_MMSE static {int(res[wce.PS_MMSE].sum())} tracked "
          f"{int(t[wce.PS_MMSE].sum())}; starts differing from the model's: "
          f"{int(np.sum(res['start'] != model['start']))}")
    assert t[wce.LT_LS].sum() < res[wce.LT_LS].sum()
    # frozen knots: every key the two calls share has the values of the static link with knot 0's taps
    frozen = fd.link_set(1.0)["taps"]
    a = ctx.link_host(fd.LINK_MOD, fd.LINK_RATE, fd.LINK_SNR, fd.LINK_B, taps=frozen, knot_period=fd.LINK_P,
                      tracker=(fd.LINK_MU, fd.LINK_BETA), **call)
    b = ctx.link_host(fd.LINK_MOD, fd.LINK_RATE, fd.LINK_SNR, fd.LINK_B, taps=frozen[:, 0], **call)
    assert "tracked" in a and "tracked" not in b and set(a) - {"tracked"} == set(b)
    for k in b:
        assert same_bits(a[k], b[k]), k
    print(f"frozen: LT_LS static {int(a[wce.LT_LS].sum())} tracked {int(a['tracked'][wce.LT_LS].sum())}")
    with pytest.raises(ValueError):
        ctx.link_host(fd.LINK_MOD, fd.LINK_RATE, fd.LINK_SNR, fd.LINK_B, taps=c["taps"], tracker=(0.5, 2),
                      dd_iterations=1, **call)


# ---------------------------------------------------------------- 10. 64-bit indexing
def test_big_strides(gpu_wce, ctx):
    """tests/test_chain_bigindex_gpu.py's method: 600 frames, the knots and the captures at a frame stride of 2^22
    complex elements (frame 599 starts 40 GB in), the knots 2^16 apart inside a slot; two big buffers"""
    wce = gpu_wce
    B, S, BS = big.B, big.S, big.BS
    D, Z = wce.DeviceArray.from_numpy, lambda shape: wce.DeviceArray(shape, np.complex128, zero=True)
    rng = np.random.default_rng(0xFAB1)
    sym0, pre0 = tm.shape_set(67, 15, 1)
    sym, pre = np.ascontiguousarray(sym0[np.arange(B) % 67]), np.ascontiguousarray(pre0[np.arange(B) % 67])
    nt, P, K, L, S_wave = 16, 80, 19, 1488, 1360
    knots = fd.moving_knots(rng, B, K, nt)
    dsym, dpre, dknots = D(sym), D(pre), D(knots)
    chan = dict(n_taps=nt, knot_period=P, cfo=D(rng.uniform(-0.002, 0.002, B)), ow2=D(rng.uniform(0.5, 2.0, B) * 1e-4),
                delay=D(rng.integers(-20, 60, B).astype(np.int32)), seed=tm.SEED, first_frame=11)
    bigk, bigcap = big.Slots(wce, np.complex128, S), big.Slots(wce, np.complex128, S)
    try:
        bigk.put(dknots, 0, BS)
        dwave, dcap, dcap2 = Z((B, S_wave)), Z((B, L)), Z((B, L))
        ctx.modulate(dsym, B, dwave, 15, dpre, 53)
        ctx.transmit_tv(dsym, B, dcap, L, dknots, K, knot_stride=nt, knots_frame_stride=K * nt, tx_pre=dpre,
                        pre_stride=53, **chan)
        ctx.transmit_tv(dsym, B, bigcap.at(), L, bigk.at(), K, knot_stride=BS, knots_frame_stride=S, tx_pre=dpre,
                        pre_stride=53, capture_stride=S, **chan)
        wce.synchronize()
        want = dcap.numpy()
        big._same({"capture": bigcap.get((B, L))}, {"capture": want}, "transmit_tv")
        ctx.channel_tv(dwave, B, S_wave, dcap2, L, dknots, K, knot_stride=nt, knots_frame_stride=K * nt, **chan)
        wce.synchronize()
        assert same_bits(dcap2.numpy(), want)
        wce.load().wce_memset(bigcap.d.ptr, 0, 16 * L)          # frame 0's row: the second call must write it again
        ctx.channel_tv(dwave, B, S_wave, bigcap.at(), L, bigk.at(), K, knot_stride=BS, knots_frame_stride=S,
                       capture_stride=S, **chan)
        wce.synchronize()
        big._same({"capture": bigcap.get((B, L))}, {"capture": want}, "channel_tv")
    finally:
        for b in (bigk, bigcap):
            b.free()
