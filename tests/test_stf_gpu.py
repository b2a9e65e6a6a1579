"""The short training field on the GPU: wce_short_field and wce_front_end_sync_stf
(csrc/wce_sync_stf.hip), and the host conveniences that use them (transmit_host,
link_host and receive_capture_host with stf=True).

The reference is the long double model of tests/stf_model.py.  start is compared
exactly and both metrics and cfo within TOL_MS, TOL_ML and TOL_CFO, absolute;
tests/test_stf_abi.py derives the three and asserts, on the same data, what makes
the exact comparisons legitimate (gaps, thresholds, the unwrapping's margin, the
plateau of the noise-free short field).  Window lengths: the issue's 144, 145,
191, 488 and 1,648, and the lengths at which a window takes another tile of the
kernel's first or second pass, +-1, from the kernel's own constants.

Measured on an MI355X: Ms within 1.3e-15, Ml 1.3e-15 and cfo 2.4e-18 of the long
double model on every set, start equal everywhere; the short field within 0.81 ulp
of amplitude max |t|; the chain's 67 packets at starts 192..194 with Ms >= 0.995,
Ml >= 0.347, the offset within 3.1e-5 of the one applied and no bit error, the
model's counts.

Without wce_front_end_sync_stf and wce_short_field every test here fails at the
missing symbol or keyword; test_link_host also shows why they are there:
wce_front_end_sync alone finds none of the 67 packets at +-0.025 cycles per sample."""
import ctypes

import numpy as np
import pytest

import cfo_model as cm
import fec_model as fm
import stf_model as st
import sync_model as sm
import tx_model as tm

pytestmark = pytest.mark.gpu

LD = np.longdouble
SENT_START, SENT_F64 = -77, 123.25
LAGS_STF, LAGS_LTF = 432, 448       # sync_stf_kernel's SS_LAGS_STF, SS_LAGS_LTF (wce_debug_sync_stf_tiles)
SHAPES = st.BASE_SHAPES + [(L, st.TILE_B) for L in st.tile_lengths(LAGS_STF, LAGS_LTF)]
GRID = 6                            # WCE_VARIANT_GRID


@pytest.fixture(scope="module")
def ctx(gpu_wce):
    pre = tm.chain_pre()
    c = gpu_wce.Context(pre, pre, 1e-6, gpu_wce.MMSE_TEXTBOOK)
    yield c
    c.close()


def _u8(a):
    return np.ascontiguousarray(a).view(np.uint8)


def run(wce, ctx, cap, ltf, backoff=0, thr=(st.THR_STF, st.THR_LTF), metrics=True, pad=5):
    """wce_front_end_sync_stf on cap [B][L] laid out with `pad` sentinel samples behind each row, into
    sentinel-filled outputs one element longer than the batch -> dict of the B results"""
    B, L = cap.shape
    dcap = wce.DeviceArray.from_numpy(tm.padded(cap, L + pad))
    dltf = wce.DeviceArray.from_numpy(np.ascontiguousarray(ltf, np.complex128))
    ds = wce.DeviceArray.from_numpy(np.full(B + 1, SENT_START, np.int32))
    d = {k: wce.DeviceArray.from_numpy(np.full(B + 1, SENT_F64)) for k in ("cfo", "metric_stf", "metric_ltf")}
    ctx.front_end_sync_stf(dcap, B, L, dltf, thr[0], thr[1], backoff, ds, d["cfo"],
                           d["metric_stf"] if metrics else None, d["metric_ltf"] if metrics else None,
                           capture_stride=L + pad)
    wce.synchronize()
    out = {"start": ds.numpy(), **{k: v.numpy() for k, v in d.items()}}
    assert out["start"][B] == SENT_START and all(out[k][B] == SENT_F64 for k in d), "written past the batch"
    if not metrics:
        assert np.all(out["metric_stf"] == SENT_F64) and np.all(out["metric_ltf"] == SENT_F64)
    assert np.array_equal(_u8(dcap.numpy()), _u8(tm.padded(cap, L + pad))), "the capture changed"
    return {k: v[:B] for k, v in out.items()}


def parity(got, ref, what):
    """got against the long double model's dict: start exact, NaN where the model has NaN, the rest within TOL"""
    assert np.array_equal(got["start"], ref["start"]), what
    errs = {}
    for k, tol in (("metric_stf", st.TOL_MS), ("metric_ltf", st.TOL_ML), ("cfo", st.TOL_CFO)):
        r = np.asarray(ref[k], LD)
        fin = np.isfinite(np.asarray(r, np.float64))
        assert np.array_equal(np.isnan(got[k]), ~fin), (what, k)
        errs[k] = float(np.max(np.abs(np.asarray(got[k], LD)[fin] - r[fin]))) if fin.any() else 0.0
    print(f"\n{what}: detected {int(np.sum(ref['start'] >= 0))} of {len(ref['start'])}; Ms within "
          f"{errs['metric_stf']:.2e} ({st.TOL_MS:.0e}), Ml {errs['metric_ltf']:.2e} ({st.TOL_ML:.0e}), "
          f"cfo {errs['cfo']:.2e} ({st.TOL_CFO:.0e})")
    assert errs["metric_stf"] <= st.TOL_MS and errs["metric_ltf"] <= st.TOL_ML and errs["cfo"] <= st.TOL_CFO, what
    return errs


def test_tile_constants(gpu_wce):
    a, b = ctypes.c_int(), ctypes.c_int()
    assert gpu_wce.load().wce_debug_sync_stf_tiles(ctypes.byref(a), ctypes.byref(b)) == 0
    assert (a.value, b.value) == (LAGS_STF, LAGS_LTF)       # SHAPES was made from these


@pytest.mark.parametrize("L,B", SHAPES)
def test_model_parity(gpu_wce, ctx, L, B):
    cap, info, ltf = st.shape_set(L, B)
    an = st.shape_model(L, B)
    for backoff in (0, 5):
        ref = st.sync_stf(cap, ltf, backoff=backoff, an=an)
        got = run(gpu_wce, ctx, cap, ltf, backoff)
        parity(got, ref, f"L={L} B={B} backoff={backoff}")
    if L >= 488:
        # the cases the data is there for (tests/test_stf_abi.py asserts them on the model)
        iw = st.in_window(info, L) & (info["snr"] >= 5)
        assert iw.any() and np.all(got["start"][iw] >= 0)
        assert np.all(got["start"][(info["kind"] == "cut") | (info["kind"] == "noise")] == -1)


def test_metrics_are_optional(gpu_wce, ctx):
    cap, _, ltf = st.shape_set(145, 5)
    full = run(gpu_wce, ctx, cap, ltf)
    bare = run(gpu_wce, ctx, cap, ltf, metrics=False)
    for k in ("start", "cfo"):
        assert np.array_equal(_u8(full[k]), _u8(bare[k])), k


def test_all_zero_window(gpu_wce, ctx):
    cap, ltf = st.zeros_set()
    got = run(gpu_wce, ctx, cap, ltf)
    assert np.all(got["start"] == -1) and np.isnan(got["cfo"]).all()
    assert np.all(got["metric_stf"] == 0.0) and np.all(got["metric_ltf"] == 0.0)


def test_short_field(gpu_wce, ctx):
    wce = gpu_wce
    t = np.asarray(st.short_period(), np.clongdouble)
    for B, stride, amp in ((1, 160, 1.0), (67, 171, tm.SCALE), (5, 1520, 0.3)):
        init = np.full((B + 1, stride), sm.SENT, np.complex128)
        d = wce.DeviceArray.from_numpy(init)
        ctx.short_field(d, B, amp, stride)
        wce.synchronize()
        w = d.numpy()
        assert np.all(w[B] == sm.SENT) and np.all(w[:B, 160:] == sm.SENT), "written outside the 160 samples"
        assert np.array_equal(_u8(w[:B, :144]), _u8(w[:B, 16:160])), "rows are not periodic bit for bit"
        assert np.array_equal(_u8(w[:B, :160]), _u8(np.broadcast_to(w[0, :160], (B, 160))))
        ref = np.tile(t, 10) * LD(amp)
        d_re = np.max(np.abs(np.asarray(w[0, :160].real, LD) - ref.real))
        d_im = np.max(np.abs(np.asarray(w[0, :160].imag, LD) - ref.imag))
        ulp = np.spacing(amp * float(np.max(np.abs(t))))
        print(f"\nshort field B={B} amplitude {amp}: within {float(max(d_re, d_im)) / ulp:.2f} ulp of amplitude max|t|")
        assert max(d_re, d_im) <= st.TOL_T * ulp
    # n_frames == 0 writes nothing
    d = wce.DeviceArray.from_numpy(np.full((1, 160), sm.SENT, np.complex128))
    ctx.short_field(d, 0, 1.0, 160)
    wce.synchronize()
    assert np.all(d.numpy() == sm.SENT)


def test_nonfinite(gpu_wce, ctx):
    cap, _, ltf = st.shape_set(488, 67)
    clean = run(gpu_wce, ctx, cap, ltf)
    for f, i, v in ((9, 0, complex(np.nan, 0.0)), (40, 487, complex(0.0, np.inf)), (23, 300, complex(-np.inf, 1.0))):
        bad = cap.copy()
        bad[f, i] = v
        got = run(gpu_wce, ctx, bad, ltf)
        assert got["start"][f] == -1
        assert np.isnan(got["cfo"][f]) and np.isnan(got["metric_stf"][f]) and np.isnan(got["metric_ltf"][f])
        for k in got:
            assert np.array_equal(_u8(np.delete(got[k], f)), _u8(np.delete(clean[k], f))), (k, f)
    bad_ltf = ltf.copy()
    bad_ltf[17] = complex(np.nan, 0.0)
    got = run(gpu_wce, ctx, cap, bad_ltf)
    assert np.all(got["start"] == -1)
    assert all(np.isnan(got[k]).all() for k in ("cfo", "metric_stf", "metric_ltf"))


def test_batch_independence(gpu_wce, ctx):
    cap, _, ltf = st.shape_set(191, 777)
    base = run(gpu_wce, ctx, cap, ltf)
    perm = np.random.default_rng(0x57F1).permutation(777)
    got = run(gpu_wce, ctx, cap[perm], ltf)
    sub = np.array([776, 3, 400, 12, 77])
    few = run(gpu_wce, ctx, cap[sub], ltf)
    for k in base:
        assert np.array_equal(_u8(got[k]), _u8(base[k][perm])), k
        assert np.array_equal(_u8(few[k]), _u8(base[k][sub])), k


# ---------------------------------------------------------------- the frame loop
LOOP_L = (191, 577, 1100)


def _loop_windows(L):
    """shape_set's generator at 67 windows of L samples, rearranged so that, under three workgroups (a sweep of
    12 frames), a wave meets a bad or strong window and then a weak one: frame 0 is NaN-poisoned and 12 a packet;
    1 is a noise-free packet at the window's first sample and 13 noise alone"""
    cap, info = st.packets(0x57F0 + 67000 + L, 67, L)
    cap = cap.copy()
    rng = np.random.default_rng(0x57F2 + L)
    cap[0, min(300, L - 1)] = complex(np.nan, 0.0)
    clean, _ = st.packets(0x57F3 + L, 1, L)        # frame 0 of a set: "first", noise-free (40 dB below 320 samples)
    cap[1] = clean[0]
    cap[13] = cm.random_packets(rng, 1, L, np.sqrt(st.P0 / 20))[0]
    return cap, sm.clean_ltf()


@pytest.mark.parametrize("L", LOOP_L)
def test_frame_loop(gpu_wce, ctx, L):
    wce, lib = gpu_wce, gpu_wce.load()
    cap, ltf = _loop_windows(L)
    ref = st.sync_stf(cap, ltf)
    assert ref["start"][0] == -1 and np.isnan(np.float64(ref["metric_stf"][0])) and ref["start"][13] == -1
    assert float(ref["metric_stf"][1]) > 0.9 and float(ref["metric_stf"][13]) < 0.2
    if L >= 320:
        assert ref["start"][1] == 192 and ref["start"][12] >= 0
    assert (lib.wce_debug_chain_grid((67 + 3) // 4, 4096), lib.wce_debug_chain_grid((13 + 3) // 4, 4096)) == (17, 4)
    for B in (67, 13):
        res = []
        for knob in (0, 1):
            assert lib.wce_debug_set_variant(GRID, knob) == 0
            try:
                assert lib.wce_debug_chain_grid((B + 3) // 4, 4096) == (3 if knob else (B + 3) // 4)
                res.append(run(wce, ctx, cap[:B], ltf))
            finally:
                assert lib.wce_debug_set_variant(GRID, 0) == 0
        for k in res[0]:
            assert np.array_equal(_u8(res[0][k]), _u8(res[1][k])), f"{k}: three workgroups give other bytes (B={B})"
        parity(res[1], {k: v[:B] for k, v in ref.items()}, f"frame loop L={L} B={B}, three workgroups")


# ---------------------------------------------------------------- the chain
def test_link_host(gpu_wce, ctx):
    wce = gpu_wce
    B, T = st.CHAIN_B, fm.info_bits(st.CHAIN_MOD, st.CHAIN_RATE)
    taps = wce.pdp_taps(np.random.default_rng(st.CHAIN_SEED), B, np.exp(-np.arange(6.0)))
    assert np.array_equal(taps, st.chain_taps())
    model = st.chain_model(tm.chain_pre(), taps)
    assert np.all(model["start"] >= 0), "the seed was chosen so that the model detects all 67"
    kw = dict(sources=(wce.LT_LS, wce.PS_LINEAR), taps=taps, cfo=st.chain_cfo(), capture_len=st.CHAIN_LEN,
              seed=st.CHAIN_SEED)
    res = ctx.link_host(st.CHAIN_MOD, st.CHAIN_RATE, st.CHAIN_SNR, B, stf=True, **kw)
    print(f"\nlink_host stf: start {res['start'].min()}..{res['start'].max()}, Ms >= {res['metric_stf'].min():.3f}, "
          f"Ml >= {res['metric'].min():.3f}, |cfo - given| <= {np.max(np.abs(res['cfo'] - st.chain_cfo())):.2e}, "
          f"LT_LS errors {int(res[wce.LT_LS].sum())}, model {int(model['nbiterr'].sum())}")
    assert np.all(res["start"] >= 0)
    assert np.array_equal(res["start"], model["start"])
    assert np.array_equal(res["bits"], model["bits"])
    assert np.array_equal(res[wce.LT_LS], model["nbiterr"])
    assert res[wce.PS_LINEAR].shape == (B,) and np.all(res[wce.PS_LINEAR] <= T)
    assert np.max(np.abs(res["cfo"] - model["cfo"])) <= 1e-13      # the float64 chain's: the captures differ by rounding
    assert np.max(np.abs(res["cfo"] - st.chain_cfo())) < 1e-3
    # today's behaviour and the reason for the change: without the short field nothing is found at this offset
    plain = ctx.link_host(st.CHAIN_MOD, st.CHAIN_RATE, st.CHAIN_SNR, B, stf=False, **kw)
    assert np.all(plain["start"] == -1) and np.array_equal(plain["start"], st.chain_plain(tm.chain_pre(), taps)[0])
    omitted = ctx.link_host(st.CHAIN_MOD, st.CHAIN_RATE, st.CHAIN_SNR, B, **kw)
    assert set(plain) == set(omitted) and "metric_stf" not in plain
    for k in plain:
        assert np.array_equal(_u8(plain[k]), _u8(omitted[k])), k
    with pytest.raises(ValueError):
        ctx.link_host(st.CHAIN_MOD, st.CHAIN_RATE, st.CHAIN_SNR, 2, taps=taps[:2], stf=True, capture_len=1524)


def test_receive_capture_host(gpu_wce, ctx):
    wce = gpu_wce
    B = 5
    rng = np.random.default_rng(0x57F4)
    pre = tm.chain_pre()
    sym = tm.symbols(rng, B, tm.NBLK, tm.MODS[1])
    taps = tm.random_taps(rng, B, 6)
    ow2 = float(tm.nominal_ow2(30.0))
    delay = np.array([0, 37, 100, 128 - 5, 64], np.int32)
    cap = ctx.transmit_host(sym, pre, taps, cfo=0.02, ow2=ow2, delay=delay, capture_len=1648, stf=True)
    assert cap.shape == (B, 1648)
    plain = ctx.transmit_host(sym, pre, taps, cfo=0.02, ow2=ow2, delay=delay, capture_len=1648, stf=False)
    assert np.array_equal(_u8(plain), _u8(ctx.transmit_host(sym, pre, taps, cfo=0.02, ow2=ow2, delay=delay,
                                                             capture_len=1648)))
    tx_pk = np.asarray(tm.modulate(sym, None, np.float64), np.complex128)
    tx_lp = np.asarray(tm.modulate(np.zeros((B, 0, tm.N)), pre, np.float64), np.complex128)
    out = ctx.receive_capture_host(tx_pk, tx_lp, cap, st.THR_LTF, stf=True)
    ref = st.sync_stf(cap, tx_lp[0, -64:])
    print(f"\nreceive_capture_host stf: start {out['start']}, cfo {out['cfo']}")
    assert np.array_equal(out["start"], ref["start"]) and np.all(out["start"] >= delay + 192)
    assert np.all(out["start"] <= delay + 197)
    assert float(np.max(np.abs(np.asarray(out["cfo"], LD) - ref["cfo"]))) <= st.TOL_CFO
    assert np.max(np.abs(out["cfo"] - 0.02)) < 1e-3
    assert float(np.max(np.abs(np.asarray(out["metric_stf"], LD) - ref["metric_stf"]))) <= st.TOL_MS
    for k in ("lt_ls", "ps_linear", "ps_mmse"):
        assert np.isfinite(out[k].view(np.float64)).all(), k
    old = ctx.receive_capture_host(tx_pk, tx_lp, cap, st.THR_LTF, cfo=True)
    assert np.all(old["start"] == -1) and "metric_stf" not in old
