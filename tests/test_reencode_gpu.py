"""wce_reencode on the device against the model of tests/reencode_model.py.  The
re-encoded symbols are held to the model's bits, the data-aided estimate to the
bound tests/test_reencode_abi.py derives (and checks the data for).  Batches of 1,
5 and 67 frames (77 with the impulse set); every stride padded, the padding
filled with sentinels that must survive; the frames' tx passed is a poisoned copy
that holds true pilots only."""
import ctypes
import functools

import numpy as np
import pytest

import cfo_model as cm
import demod_model as dm
import fec_model as fm
import reencode_model as rm

pytestmark = pytest.mark.gpu

N, NBLK = dm.N, dm.NBLK
HS = 56                              # estimates: row stride
FS, BS = 15 * 56 + 3, 56             # frames and x^: frame and block stride
SENT, SENT8 = 7.0 - 3.0j, 0xA5
BATCHES = (1, 5, 67)
P = list(dm.PILOTS)
H_SETS = [(m, fm.RATE_1_2) for m in fm.MODS] + [(dm.QAM64, fm.RATE_3_4)]


def _pad_frames(a, fill=SENT):
    out = np.full((a.shape[0], FS), fill, np.complex128)
    for b in range(NBLK):
        out[:, b * BS:b * BS + N] = a[:, b]
    return out


def _unpad_frames(flat):
    mask = np.zeros(FS, bool)
    for b in range(NBLK):
        mask[b * BS:b * BS + N] = True
    vals = np.stack([flat[:, b * BS:b * BS + N] for b in range(NBLK)], axis=1)
    return vals, bool(np.all(flat[:, ~mask] == SENT))


def _pack(u):
    """[B][T] -> [B][ceil(T/8) + 3] uint8: LSB first, the last byte's spare bits set, the padding a sentinel"""
    T = u.shape[1]
    nby = (T + 7) // 8
    out = np.full((u.shape[0], nby + 3), SENT8, np.uint8)
    out[:, :nby] = fm.pack(u)
    if T % 8:
        out[:, nby - 1] |= (0xFF << (T % 8)) & 0xFF
    return out


def _poisoned(pilots):
    """a frames' tx that holds nothing but pilots [B][15][4]: NaN wherever the call must not read"""
    tx = np.full((pilots.shape[0], NBLK, N), np.nan + 1j * np.nan, np.complex128)
    tx[:, :, P] = pilots
    return tx


@pytest.fixture(scope="module")
def ctx(gpu_wce):
    return gpu_wce.Context(empty=True)     # the ctx only selects the device


def reencode(wce, ctx, u, mod, rate, pilots=None, rx=None, theta=None, want=("tx", "h")):
    """one wce_reencode call on padded device buffers -> dict tx [B][15][53], h [B][53]"""
    B = u.shape[0]
    D = wce.DeviceArray.from_numpy
    packed = _pack(u)
    dbits = D(packed)
    fr = None
    keep = []
    if pilots is not None or rx is not None:
        dtx = D(_pad_frames(_poisoned(pilots), np.nan)) if pilots is not None else None
        drx = D(_pad_frames(rx, np.nan)) if rx is not None else None
        keep += [dtx, drx]
        fr = ctx.frames(dtx, drx, B, frame_stride=FS, block_stride=BS)
    dth = D(np.ascontiguousarray(theta, np.float64)) if theta is not None else None
    dtx_out = D(np.full((B, FS), SENT, np.complex128)) if "tx" in want else None
    dh = D(np.full((B, HS), SENT, np.complex128)) if "h" in want else None
    ctx.reencode(dbits, B, mod, rate, bits_stride=packed.shape[1], theta=dth, frames=fr, tx=dtx_out,
                 tx_frame_stride=FS, tx_block_stride=BS, h=dh, h_stride=HS)
    wce.synchronize()
    assert np.array_equal(dbits.numpy(), packed)
    out = {}
    if dtx_out is not None:
        out["tx"], ok = _unpad_frames(dtx_out.numpy())
        assert ok, "tx: padding overwritten"
    if dh is not None:
        raw = dh.numpy()
        assert np.all(raw[:, N:] == SENT), "h: padding overwritten"
        out["h"] = raw[:, :N]
    return out


def _same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))


@functools.lru_cache(maxsize=None)
def _x_set(mod, rate):
    """the clean set's information bits and the impulse set, [77][T], and the model's x^ with 802.11's pilots"""
    u = np.concatenate([fm.clean_set(mod, rate)["u"], rm.impulse_set(mod, rate)])
    return u, rm.xhat(u, mod, rate)


# ---------------------------------------------------------------- 1. x^ is exact
@pytest.mark.parametrize("mod,rate", fm.COMBOS)
def test_reencoded_symbols_are_exact(gpu_wce, ctx, mod, rate):
    u, x = _x_set(mod, rate)
    for B in BATCHES + (len(u),):
        sel = slice(len(u) - B, len(u)) if B == 5 else slice(0, B)       # the batch of 5: impulses from the end
        got = reencode(gpu_wce, ctx, u[sel], mod, rate, want=("tx",))
        assert set(got) == {"tx"} and _same_bits(got["tx"], x[sel]), B
    # pilots copied from a frames' tx that holds nothing else: only the four pilot entries are read
    pil = -0.5 * rm.standard_pilots(len(u))
    want = x.copy()
    want[:, :, P] = pil
    got = reencode(gpu_wce, ctx, u, mod, rate, pilots=pil, want=("tx",))
    assert _same_bits(got["tx"], want)
    assert not got["tx"][:, :, dm.DC].any()


# ---------------------------------------------------------------- 2. closed loop on the device, no model
@pytest.mark.parametrize("mod,rate", fm.COMBOS)
def test_closed_loop(gpu_wce, ctx, mod, rate):
    u = fm.clean_set(mod, rate)["u"][:5]
    x = reencode(gpu_wce, ctx, u, mod, rate, want=("tx",))["tx"]
    one = np.ones((5, N), np.complex128)
    dem = ctx.demodulate_host(x, x, one, None, modulation=mod, track=True, ref_tx=True)
    assert not dem["nerr"].any() and np.all(dem["evm"] == 0.0)
    out = ctx.decode_host(dem["eq"], one, None, modulation=mod, rate=rate, ref_bits=u)
    assert np.array_equal(out["bits"], u) and not out["nbiterr"].any()


# ---------------------------------------------------------------- 3. H_dd
def _within(h, ld, what):
    err = rm.relmax_rows(h, ld)
    print(f"{what}: worst |dH| = {err.max():.2e} of the frame's max |H_dd| (TOL_H {rm.TOL_H:.0e})")
    assert np.all(err <= rm.TOL_H), what
    assert not h[:, dm.DC].any(), what


@pytest.mark.parametrize("mod,rate", H_SETS)
def test_data_aided_estimate(gpu_wce, ctx, mod, rate):
    wce = gpu_wce
    s = fm.clean_set(mod, rate)
    u, rx, theta = s["u"], s["rx"], rm.clean_theta(mod, rate)
    x = rm.xhat(u, mod, rate)
    pil = x[:, :, P]
    ld = rm.h_dd(x, rx, theta)[0]
    both = reencode(wce, ctx, u, mod, rate, pilots=pil, rx=rx, theta=theta)
    assert _same_bits(both["tx"], x)
    _within(both["h"], ld, f"{mod} bits rate {rate}")
    # h alone: the bits of the call with both outputs; a frame alone and in smaller batches: its bits in the 67
    alone = reencode(wce, ctx, u, mod, rate, pilots=pil, rx=rx, theta=theta, want=("h",))
    assert set(alone) == {"h"} and _same_bits(alone["h"], both["h"])
    for B in (1, 5):
        sel = slice(60, 60 + B)
        part = reencode(wce, ctx, u[sel], mod, rate, pilots=pil[sel], rx=rx[sel], theta=theta[sel], want=("h",))
        assert _same_bits(part["h"], both["h"][sel]), B
    # 802.11's pilots are the set's own: no frames' tx, the same bits
    std = reencode(wce, ctx, u, mod, rate, rx=rx, theta=theta, want=("h",))
    assert _same_bits(std["h"], both["h"])
    # theta == NULL is theta = 0
    null = reencode(wce, ctx, u, mod, rate, pilots=pil, rx=rx, want=("h",))
    zero = reencode(wce, ctx, u, mod, rate, pilots=pil, rx=rx, theta=np.zeros_like(theta), want=("h",))
    assert _same_bits(null["h"], zero["h"])
    _within(null["h"], rm.h_dd(x, rx, None)[0], f"{mod} bits rate {rate}, no theta")
    # rx = H x^ exactly and no rotation: the estimate is H
    h = s["h"].copy()
    h[:, dm.DC] = 0
    exact = reencode(wce, ctx, u, mod, rate, pilots=pil, rx=s["h"][:, None, :] * x, want=("h",))
    _within(exact["h"], h, f"{mod} bits rate {rate}, rx = H x^")
    # a NaN in one frame's rx and in another frame's theta: no other frame changes by a bit
    rx2, th2 = rx.copy(), theta.copy()
    rx2[3, 7, 30] = np.nan
    th2[9, 4] = np.nan
    bad = reencode(wce, ctx, u, mod, rate, pilots=pil, rx=rx2, theta=th2, want=("h",))
    others = np.ones(67, bool)
    others[[3, 9]] = False
    assert _same_bits(bad["h"][others], both["h"][others])
    assert np.isnan(bad["h"][3, 30].real) and np.isnan(bad["h"][3, 30].imag)
    k = np.arange(N) != 30
    assert _same_bits(bad["h"][3, k], both["h"][3, k])
    nd = np.arange(N) != dm.DC
    assert np.all(np.isnan(bad["h"][9, nd].real)) and np.all(np.isnan(bad["h"][9, nd].imag)) and bad["h"][9, dm.DC] == 0


# ---------------------------------------------------------------- 4. the chain
@pytest.mark.parametrize("mod,rate,snr", rm.LOW_SNR)
def test_second_pass_on_the_device(gpu_wce, ctx, mod, rate, snr):
    """decode_host(dd_iterations=1) on the low-SNR sets: the device's second pass leaves at most 0.75 of its own
    first pass's bit errors (the model's <= 0.6, tests/test_reencode_abi.py, plus room for frames whose float
    metrics break differently); the first pass is what dd_iterations=0 returns"""
    s = rm.low_snr_set(mod, rate, snr)
    pilots_only = _poisoned(s["tx"][:, :, P])
    dem = ctx.demodulate_host(pilots_only, s["rx"], s["h0"], None, modulation=mod)
    plain = ctx.decode_host(dem["eq"], s["h0"], None, modulation=mod, rate=rate, ref_bits=s["u"])
    out = ctx.decode_host(dem["eq"], s["h0"], None, modulation=mod, rate=rate, ref_bits=s["u"], dd_iterations=1,
                          rx=s["rx"], tx_pilots=pilots_only)
    assert set(out) == set(plain) | {"h_dd", "decode_dd"} and set(out["decode_dd"]) == {"bits", "nbiterr"}
    for k in plain:
        assert np.array_equal(out[k].view(np.uint8), plain[k].view(np.uint8)), k
    assert out["h_dd"].shape == (67, N) and out["decode_dd"]["bits"].shape == s["u"].shape
    std = ctx.decode_host(dem["eq"], s["h0"], None, modulation=mod, rate=rate, ref_bits=s["u"], dd_iterations=1,
                          rx=s["rx"])                                      # 802.11's pilots are the set's own
    assert _same_bits(std["h_dd"], out["h_dd"]) and np.array_equal(std["decode_dd"]["bits"], out["decode_dd"]["bits"])
    n1, n2 = int(out["nbiterr"].sum()), int(out["decode_dd"]["nbiterr"].sum())
    assert np.array_equal(out["decode_dd"]["nbiterr"], np.sum(out["decode_dd"]["bits"] != s["u"], axis=1))
    print(f"{mod} bits rate {rate} at {snr} dB: device {n1} -> {n2} bit errors (ratio {n2 / max(n1, 1):.2f})")
    assert n1 > 0 and n2 <= 0.75 * n1
    two = ctx.decode_host(dem["eq"], s["h0"], None, modulation=mod, rate=rate, ref_bits=s["u"], dd_iterations=2,
                          rx=s["rx"])
    print(f"  a second round: {int(two['decode_dd']['nbiterr'].sum())} bit errors")
    assert np.array_equal(two["bits"], plain["bits"])
    with pytest.raises(ValueError):
        ctx.decode_host(dem["eq"], s["h0"], None, modulation=mod, rate=rate, dd_iterations=1)


def _ofdm(sym):
    """[B][n][53] -> [B][80 n]: the 64-point inverse DFT of each block behind its 16-sample cyclic prefix"""
    X = np.zeros(sym.shape[:2] + (64,), complex)
    X[:, :, (np.arange(N) - 26) % 64] = sym
    x = np.fft.ifft(X, axis=-1)
    return np.concatenate([x[:, :, -16:], x], axis=-1).reshape(sym.shape[0], -1)


def test_receive_chain_iterates(gpu_wce):
    """the packet tests/test_decode_gpu.py's receive_host test builds (a BPSK rate-1/2 packet, a 3-tap channel,
    white noise at 25 dB), through receive_iterated_host: the first pass's outputs are receive_host's, the
    second pass decodes no worse"""
    wce = gpu_wce
    B, mod, rate = 3, dm.BPSK, fm.RATE_1_2
    rng = np.random.default_rng(0x80211)
    u = fm.random_info(rng, B, mod, rate)
    tx, _ = fm.transmit(u, mod, rate)
    ltf = dm.SCALE * rng.choice([-1.0, 1.0], N)
    ltf[dm.DC] = 0
    taps = np.array([1.0, 0.4 - 0.3j, 0.2j])[None, :] * np.exp(2j * np.pi * rng.random((B, 1)))
    H = taps @ np.exp(-2j * np.pi * np.outer(np.arange(3), np.arange(N) - dm.DC) / 64)
    sigma = dm.SCALE * 10 ** (-25 / 20) / 8 / np.sqrt(2)            # per part of a time sample: 64 of them make a bin
    noise = lambda shape: sigma * (rng.standard_normal(shape) + 1j * rng.standard_normal(shape))
    field = lambda X: np.tile(_ofdm(X[:, None, :])[:, 16:], (1, 3))[:, -160:]
    tx_pk, tx_lp = _ofdm(tx), np.repeat(field(ltf[None]), B, axis=0)
    rx_pk = _ofdm(H[:, None, :] * tx)
    rx_pk, rx_lp = rx_pk + noise(rx_pk.shape), field(H * ltf[None]) + noise((B, 160))
    pre = np.asarray(cm.preamble(tx_lp, np.zeros(B))[0][0], np.complex128)
    c = wce.Context(pre, pre, 9.6172e-8, wce.MMSE_TEXTBOOK)
    plain = c.receive_host(tx_pk, tx_lp, rx_pk, rx_lp, demod_source=wce.PS_MMSE, decode_rate=wce.RATE_1_2, ref_bits=u)
    out = c.receive_iterated_host(tx_pk, tx_lp, rx_pk, rx_lp, wce.PS_MMSE, wce.RATE_1_2, dd_iterations=1, ref_bits=u)
    assert set(out) == set(plain) | {"h_dd", "decode_dd"}
    for k in plain:                                                 # what was there is unchanged
        if k in ("demod", "decode"):
            for n in plain[k]:
                assert np.array_equal(out[k][n].view(np.uint8), plain[k][n].view(np.uint8)), (k, n)
        else:
            assert np.array_equal(out[k].view(np.uint8), plain[k].view(np.uint8)), k
    d = out["decode_dd"]
    assert set(d) == {"bits", "nbiterr"} and d["bits"].shape == (B, 360) and out["h_dd"].shape == (B, N)
    print(f"bit errors: first pass {out['decode']['nbiterr']}, second pass {d['nbiterr']}")
    assert np.all(d["nbiterr"] <= out["decode"]["nbiterr"])
    same = c.receive_iterated_host(tx_pk, tx_lp, rx_pk, rx_lp, wce.PS_MMSE, wce.RATE_1_2, dd_iterations=0, ref_bits=u)
    assert set(same) == set(plain)
    with pytest.raises(TypeError):
        c.receive_iterated_host(tx_pk, tx_lp, rx_pk, rx_lp, wce.PS_MMSE, wce.RATE_1_2, threshold=0.5)


# ---------------------------------------------------------------- 5. arguments
def test_invalid_arguments(gpu_wce, ctx):
    wce = gpu_wce
    lib, W = wce.load(), wce.wce
    mod, rate, B = dm.QAM16, fm.RATE_3_4, 5
    nby = (fm.info_bits(mod, rate) + 7) // 8
    s = fm.clean_set(mod, rate)
    D = wce.DeviceArray.from_numpy
    dbits = D(_pack(s["u"][:B]))
    dtx, drx = D(_pad_frames(s["tx"][:B])), D(_pad_frames(s["rx"][:B]))
    dth = D(np.zeros((B, NBLK)))
    dxo, dho = D(np.full((B, FS), SENT, np.complex128)), D(np.full((B, HS), SENT, np.complex128))
    outs = (dxo, dho)
    before = [a.numpy() for a in outs]

    def call(ctx_=ctx.handle, p=None, null_p=False, fr=None, null_in=False, out=None, null_out=False, n=B):
        Pp = W.ReencodePar(dbits.addr, nby + 3, mod, rate, dm.SCALE, dth.addr)
        F = W.Frames(dtx.addr, drx.addr, None, None, FS, BS, 0, n, 0, 0)
        O = W.ReencodeOut(dxo.addr, FS, BS, dho.addr, HS)
        for st, kv in ((Pp, p), (F, fr), (O, out)):
            for k, v in (kv or {}).items():
                setattr(st, k, v)
        return lib.wce_reencode(ctx_, None if null_p else ctypes.byref(Pp), None if null_in else ctypes.byref(F), n,
                                None if null_out else ctypes.byref(O), None)

    cases = [("null ctx", dict(ctx_=None)), ("null p", dict(null_p=True)), ("null out", dict(null_out=True)),
             ("null bits", dict(p={"bits": None})), ("both outputs null", dict(out={"tx": None, "h": None})),
             ("h without in", dict(null_in=True)), ("h without rx", dict(fr={"rx": None})),
             ("n_frames of in", dict(fr={"n_frames": B + 1})), ("modulation 3", dict(p={"modulation": 3})),
             ("rate 3", dict(p={"rate": 3})), ("scale 0", dict(p={"scale": 0.0})),
             ("scale nan", dict(p={"scale": float("nan")})), ("bits_stride", dict(p={"bits_stride": nby - 1})),
             ("tx block stride", dict(out={"tx_block_stride": 52})),
             ("tx frame stride", dict(out={"tx_frame_stride": 14 * BS + 52})),
             ("in block stride", dict(fr={"block_stride": 52})),
             ("in frame stride", dict(fr={"frame_stride": 14 * BS + 52})), ("h_stride", dict(out={"h_stride": 52})),
             ("tx alignment", dict(out={"tx": dxo.addr + 8})), ("h alignment", dict(out={"h": dho.addr + 8})),
             ("rx alignment", dict(fr={"rx": drx.addr + 8})), ("theta alignment", dict(p={"theta": dth.addr + 4})),
             ("n_frames < 0", dict(n=-1)), ("n_frames 2^31", dict(n=2 ** 31))]
    for name, kw in cases:
        assert lib.wce_decode_info_bits(0, 0) == -1                            # leaves its own text behind
        marker = lib.wce_last_error()
        assert call(**kw) == -1, name
        text = lib.wce_last_error()
        assert text and text != marker, name
    assert call(n=0) == 0 and call(n=0, null_in=True, out={"h": None}) == 0
    wce.synchronize()
    for a, b in zip(outs, before):                                             # nothing was launched
        assert np.array_equal(a.numpy().view(np.uint8), b.view(np.uint8))
    assert call() == 0 and call(out={"tx": None}) == 0 and call(out={"h": None}, null_in=True) == 0
    assert call(out={"h": None}, fr={"rx": None}) == 0 and call(p={"theta": None}) == 0
    wce.synchronize()
    with pytest.raises(wce.WceError) as e:
        ctx.reencode(dbits, B, mod, 7, tx=dxo)
    assert e.value.code == -1
