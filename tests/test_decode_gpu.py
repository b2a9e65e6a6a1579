"""wce_soft_demap and wce_viterbi_decode on the device against the model of
tests/fec_model.py.  The soft bits are held to bound (c), the decoder's bits and
error counts to the model's exactly, on the data whose conditions
tests/test_decode_abi.py checks (and derives the bound for).  Batches of 1, 5 and
67 frames; every stride padded, the padding filled with sentinels that must
survive."""
import ctypes
import functools

import numpy as np
import pytest

import cfo_model as cm
import demod_model as dm
import fec_model as fm

pytestmark = pytest.mark.gpu

N, NBLK = dm.N, dm.NBLK
HS = 56                              # estimates: row stride
EFS, EBS = 15 * 56 + 3, 56           # eq: frame and block stride
SENT, SENTF, SENT8 = 7.0 - 3.0j, np.float32(-777.25), 0xA5
BATCHES = (1, 5, 67)


def _strides(mod):
    """llr block and frame stride"""
    lbs = 48 * mod + 5
    return lbs, 15 * lbs + 7


def _pad_eq(a):
    out = np.full((a.shape[0], EFS), SENT, np.complex128)
    for b in range(NBLK):
        out[:, b * EBS:b * EBS + N] = a[:, b]
    return out


def _pad_rows(a):
    out = np.full((a.shape[0], HS), SENT, np.complex128)
    out[:, :N] = a
    return out


def _pad_llr(L, mod):
    lbs, lfs = _strides(mod)
    out = np.full((L.shape[0], lfs), SENTF, np.float32)
    for b in range(NBLK):
        out[:, b * lbs:b * lbs + 48 * mod] = L[:, b]
    return out


def _unpad_llr(flat, mod):
    lbs, lfs = _strides(mod)
    mask = np.zeros(lfs, bool)
    for b in range(NBLK):
        mask[b * lbs:b * lbs + 48 * mod] = True
    vals = np.stack([flat[:, b * lbs:b * lbs + 48 * mod] for b in range(NBLK)], axis=1)
    return vals, bool(np.all(flat[:, ~mask] == SENTF))


@pytest.fixture(scope="module")
def ctx(gpu_wce):
    return gpu_wce.Context(empty=True)     # the ctx only selects the device


def demap(wce, ctx, eq, h, h_lt, mod):
    """one wce_soft_demap call on padded device buffers -> llr [B][15][48 mod]"""
    B = eq.shape[0]
    D = wce.DeviceArray.from_numpy
    lbs, lfs = _strides(mod)
    keep = [D(_pad_eq(eq)), D(_pad_rows(h)), D(_pad_rows(h_lt)) if h_lt is not None else None]
    dl = D(np.full((B, lfs), SENTF, np.float32))
    ctx.soft_demap(keep[0], keep[1], B, h_lt=keep[2], h_stride=HS, modulation=mod, llr=dl, eq_frame_stride=EFS,
                   eq_block_stride=EBS, llr_frame_stride=lfs, llr_block_stride=lbs)
    wce.synchronize()
    out, ok = _unpad_llr(dl.numpy(), mod)
    assert ok, "llr: padding overwritten"
    return out


def viterbi(wce, ctx, L, mod, rate, terminated, ref=None, want=("bits", "nbiterr")):
    """one wce_viterbi_decode call on padded device buffers -> dict bits [B][T] (unpacked), nbiterr [B]"""
    B, T = L.shape[0], fm.info_bits(mod, rate)
    nby = (T + 7) // 8
    D = wce.DeviceArray.from_numpy
    lbs, lfs = _strides(mod)
    dl = D(_pad_llr(L, mod))
    dbits = D(np.full((B, nby + 3), SENT8, np.uint8)) if "bits" in want else None
    dref = dn = None
    if ref is not None:
        r = np.full((B, nby + 2), 0xFF, np.uint8)           # the padding, and the last byte's spare bits, all set
        r[:, :nby] = fm.pack(ref)
        if T % 8:
            r[:, nby - 1] |= (0xFF << (T % 8)) & 0xFF
        dref = D(r)
    if "nbiterr" in want:
        dn = D(np.full(B + 1, 0xDEAD, np.uint32))
    ctx.viterbi_decode(dl, B, mod, rate, terminated=terminated, bits=dbits, bits_stride=nby + 3, ref_bits=dref,
                       ref_stride=nby + 2, nbiterr=dn, llr_frame_stride=lfs, llr_block_stride=lbs)
    wce.synchronize()
    assert np.array_equal(dl.numpy(), _pad_llr(L, mod), equal_nan=True)
    out = {}
    if dbits is not None:
        raw = dbits.numpy()
        assert np.all(raw[:, nby:] == SENT8), "bits: padding overwritten"
        out["bits"] = np.unpackbits(raw[:, :nby], axis=1, bitorder="little")
        assert not out["bits"][:, T:].any(), "bits: the last byte's spare bits are not 0"
        out["bits"] = out["bits"][:, :T]
    if dn is not None:
        raw = dn.numpy()
        assert raw[-1] == 0xDEAD, "nbiterr: written past the end"
        out["nbiterr"] = raw[:-1]
    return out


# ---------------------------------------------------------------- 1. the demapper
@functools.lru_cache(maxsize=None)
def _demap_ref(mod, bl):
    """the clean set's fp64 model eq (tracked; blended or not) and the long double soft bits of that eq"""
    s = fm.clean_set(mod, fm.RATE_1_2)
    h_lt = s["h_lt"] if bl else None
    e64 = np.asarray(dm.demodulate(s["tx"], s["rx"], s["h"], h_lt, mod, real=np.float64)["eq"], np.complex128)
    return e64, fm.llr(e64, dm.blend(s["h"], h_lt), mod)


def _within_bound(L, ld, what):
    ld = np.asarray(ld, np.longdouble)
    mx = np.max(np.abs(ld), axis=(1, 2), keepdims=True)
    err = np.abs(L.astype(np.longdouble) - ld)
    print(f"{what}: worst |dL| - 2^-23 |L| = {float(np.max((err - 2.0 ** -23 * np.abs(ld)) / mx)):.2e} of max |L| "
          f"(TOL_ABS {fm.TOL_ABS:.0e}), worst |dL| / |L| = {float(np.max(err / np.maximum(np.abs(ld), 1e-300))):.2e}")
    assert np.all(err <= 2.0 ** -23 * np.abs(ld) + fm.TOL_ABS * mx), what


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("mod", fm.MODS)
def test_soft_bits_within_the_bound(gpu_wce, ctx, mod, B):
    s = fm.clean_set(mod, fm.RATE_1_2)
    for bl in (True, False):
        e64, ld = _demap_ref(mod, bl)
        L = demap(gpu_wce, ctx, e64[:B], s["h"][:B], s["h_lt"][:B] if bl else None, mod)
        assert L.dtype == np.float32 and L.shape == (B, NBLK, 48 * mod)
        _within_bound(L, ld[:B], f"{mod} bits B={B} blend={bl}")


@pytest.mark.parametrize("mod", fm.MODS)
def test_soft_bits_of_non_finite_symbols_are_erasures(gpu_wce, ctx, mod):
    s = fm.clean_set(mod, fm.RATE_1_2)
    B = 5
    e64, _ = _demap_ref(mod, True)
    eq, h, h_lt = e64[:B].copy(), s["h"][:B].copy(), s["h_lt"][:B].copy()
    clean = demap(gpu_wce, ctx, eq, h, h_lt, mod)
    eq[2, 7, 30] = np.nan                       # one symbol
    h[2, 11] = np.inf                           # a data subcarrier of the estimate: its 15 symbols
    eq[3, 0, 5] = np.nan                        # a pilot: no soft bit comes from it
    got = demap(gpu_wce, ctx, eq, h, h_lt, mod)
    inv = np.argsort(fm.interleave_index(mod))  # transmitted bit j is coded bit inv[j]
    where = lambda k: inv[mod * int(np.searchsorted(dm.DATA, k)) + np.arange(mod)]
    zero = np.zeros(clean.shape, bool)
    zero[2, 7, where(30)] = True
    zero[2, :, where(11)] = True
    assert np.all(got[zero] == 0) and not np.any(np.signbit(got[zero]))
    assert np.array_equal(got[~zero].view(np.uint32), clean[~zero].view(np.uint32))
    assert np.all(clean[zero] != 0)
    assert np.array_equal(got[[0, 1, 3, 4]].view(np.uint32), clean[[0, 1, 3, 4]].view(np.uint32))


# ---------------------------------------------------------------- 2. the decoder
@pytest.mark.parametrize("mod,rate", fm.COMBOS)
def test_decoder_matches_the_model_exactly(gpu_wce, ctx, mod, rate):
    s = fm.integer_set(mod, rate)
    for terminated in (True, False):
        bits, nerr = fm.integer_model(mod, rate, terminated)
        for B in BATCHES:
            got = viterbi(gpu_wce, ctx, s["llr"][:B], mod, rate, terminated, s["u"][:B])
            assert np.array_equal(got["bits"], bits[:B]), (terminated, B)
            assert np.array_equal(got["nbiterr"], nerr[:B]), (terminated, B)
        one = viterbi(gpu_wce, ctx, s["llr"][:5], mod, rate, terminated, want=("bits",))
        assert set(one) == {"bits"} and np.array_equal(one["bits"], bits[:5])
        one = viterbi(gpu_wce, ctx, s["llr"][:5], mod, rate, terminated, s["u"][:5], want=("nbiterr",))
        assert set(one) == {"nbiterr"} and np.array_equal(one["nbiterr"], nerr[:5])


@pytest.mark.parametrize("mod,rate", fm.COMBOS)
def test_zero_and_non_finite_llrs(gpu_wce, ctx, mod, rate):
    s = fm.integer_set(mod, rate)
    rng = np.random.default_rng(7 + 16 * mod + rate)
    L = np.stack([s["llr"][0], np.zeros_like(s["llr"][0]), s["llr"][0], s["llr"][0], s["llr"][1]])
    hit = rng.random(L[0].shape) < 0.1
    L[2][hit] = rng.choice(np.array([np.nan, np.inf, -np.inf], np.float32), int(hit.sum()))
    L[3][hit] = 0
    u = s["u"][[0, 0, 0, 0, 1]]
    for terminated in (True, False):
        got = viterbi(gpu_wce, ctx, L, mod, rate, terminated, u)
        want = fm.decode(L[[0, 3, 4]], mod, rate, terminated)
        assert not got["bits"][1].any() and got["nbiterr"][1] == u[1].sum()
        assert np.array_equal(got["bits"][2], got["bits"][3]) and got["nbiterr"][2] == got["nbiterr"][3]
        assert np.array_equal(got["bits"][[0, 3, 4]], want)
        assert np.array_equal(got["nbiterr"][[0, 3, 4]], np.sum(want != u[[0, 3, 4]], axis=1))


# ---------------------------------------------------------------- 3. the chains
@pytest.mark.parametrize("mod,rate", fm.COMBOS)
def test_chain_decodes_the_clean_set(gpu_wce, ctx, mod, rate):
    """decode_host on the device's own wce_demodulate eq (tracked, blended): no bit error in any frame"""
    s = fm.clean_set(mod, rate)
    dem = ctx.demodulate_host(s["tx"], s["rx"], s["h"], s["h_lt"], modulation=mod)
    out = ctx.decode_host(dem["eq"], s["h"], s["h_lt"], modulation=mod, rate=rate, ref_bits=s["u"])
    T = fm.info_bits(mod, rate)
    assert set(out) == {"llr", "bits", "nbiterr"}
    assert out["llr"].shape == (67, NBLK, 48 * mod) and out["llr"].dtype == np.float32
    assert out["bits"].shape == (67, T) and out["bits"].dtype == np.uint8 and out["nbiterr"].shape == (67,)
    print(f"{mod} bits rate {rate}: {int(dem['nerr'].sum())} raw symbol errors, {int(out['nbiterr'].sum())} bit errors")
    assert not out["nbiterr"].any() and np.array_equal(out["bits"], s["u"])
    _within_bound(out["llr"], fm.llr(dem["eq"], dm.blend(s["h"], s["h_lt"]), mod), f"{mod} bits rate {rate} chain")
    assert set(ctx.decode_host(dem["eq"][:1], s["h"][:1], modulation=mod, rate=rate)) == {"llr", "bits"}


def _ofdm(sym):
    """[B][n][53] -> [B][80 n]: the 64-point inverse DFT of each block behind its 16-sample cyclic prefix"""
    X = np.zeros(sym.shape[:2] + (64,), complex)
    X[:, :, (np.arange(N) - 26) % 64] = sym
    x = np.fft.ifft(X, axis=-1)
    return np.concatenate([x[:, :, -16:], x], axis=-1).reshape(sym.shape[0], -1)


def test_receive_chain_decodes(gpu_wce):
    """a BPSK rate-1/2 packet through receive_host: time-domain field and packet of both sides, a 3-tap channel,
    white noise at 25 dB; PS_MMSE's estimate demodulates, the decoder returns the information bits"""
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
    z = np.zeros(B)
    assert cm.relmax(cm.blocks(tx_pk, z), tx) < 1e-14              # the synthesis is the front end's inverse
    pre = np.asarray(cm.preamble(tx_lp, z)[0][0], np.complex128)
    c = wce.Context(pre, pre, 9.6172e-8, wce.MMSE_TEXTBOOK)
    plain = c.receive_host(tx_pk, tx_lp, rx_pk, rx_lp, demod_source=wce.PS_MMSE)
    out = c.receive_host(tx_pk, tx_lp, rx_pk, rx_lp, demod_source=wce.PS_MMSE, decode_rate=wce.RATE_1_2, ref_bits=u)
    assert set(out) == set(plain) | {"decode"}
    for k in plain:                                                 # what was there is unchanged
        if k == "demod":
            for n in plain[k]:
                assert np.array_equal(out[k][n].view(np.uint8), plain[k][n].view(np.uint8)), n
        else:
            assert np.array_equal(out[k].view(np.uint8), plain[k].view(np.uint8)), k
    d = out["decode"]
    assert set(d) == {"llr", "bits", "nbiterr"}
    assert d["llr"].shape == (B, NBLK, 48) and d["bits"].shape == (B, 360) and d["nbiterr"].shape == (B,)
    print(f"evm {out['demod']['evm']}, raw symbol errors {out['demod']['nerr']}, bit errors {d['nbiterr']}")
    assert not d["nbiterr"].any() and np.array_equal(d["bits"], u)
    assert set(c.receive_host(tx_pk, tx_lp, rx_pk, rx_lp, demod_source=wce.PS_MMSE, decode_rate=wce.RATE_1_2,
                              terminated=False)["decode"]) == {"llr", "bits"}
    with pytest.raises(ValueError):
        c.receive_host(tx_pk, tx_lp, rx_pk, rx_lp, decode_rate=wce.RATE_1_2)
    # a frame of NaN symbols decodes from all-zero soft bits to all-zero bits
    bad = rx_pk.copy()
    bad[1, 100] = np.nan
    d = c.receive_host(tx_pk, tx_lp, bad, rx_lp, demod_source=wce.PS_MMSE, decode_rate=wce.RATE_1_2, ref_bits=u)["decode"]
    assert not d["llr"][1, 1].any() and not d["nbiterr"][[0, 2]].any()


# ---------------------------------------------------------------- 4. arguments
def test_invalid_arguments(gpu_wce, ctx):
    wce = gpu_wce
    lib, W = wce.load(), wce.wce
    mod, rate, B = dm.QAM16, fm.RATE_3_4, 5
    T = fm.info_bits(mod, rate)
    nby = (T + 7) // 8
    lbs, lfs = _strides(mod)
    s = fm.clean_set(mod, fm.RATE_1_2)
    D = wce.DeviceArray.from_numpy
    deq, dh, dhl = D(_pad_eq(_demap_ref(mod, True)[0][:B])), D(_pad_rows(s["h"][:B])), D(_pad_rows(s["h_lt"][:B]))
    dl = D(_pad_llr(fm.integer_set(mod, rate)["llr"][:B], mod))
    dbits, dref = D(np.full((B, nby), SENT8, np.uint8)), D(fm.pack(fm.integer_set(mod, rate)["u"][:B]))
    dn = D(np.full(B, 0xDEAD, np.uint32))
    outs = (dl, dbits, dn)
    before = [a.numpy() for a in outs]

    def demap_call(p=None, null_p=False, **kw):
        P = W.Demod(dh.addr, dhl.addr, HS, mod, 0, dm.SCALE)
        for k, v in (p or {}).items():
            setattr(P, k, v)
        a = dict(ctx=ctx.handle, eq=deq.addr, efs=EFS, ebs=EBS, p=None if null_p else ctypes.byref(P), n=B,
                 llr=dl.addr, lfs=lfs, lbs=lbs)
        a.update(kw)
        return lib.wce_soft_demap(a["ctx"], a["eq"], a["efs"], a["ebs"], a["p"], a["n"], a["llr"], a["lfs"], a["lbs"],
                                  None)

    def vit_call(**kw):
        a = dict(ctx=ctx.handle, llr=dl.addr, lfs=lfs, lbs=lbs, mod=mod, rate=rate, flags=1, n=B, bits=dbits.addr,
                 bs=nby, ref=dref.addr, rs=nby, nerr=dn.addr)
        a.update(kw)
        return lib.wce_viterbi_decode(a["ctx"], a["llr"], a["lfs"], a["lbs"], a["mod"], a["rate"], a["flags"], a["n"],
                                      a["bits"], a["bs"], a["ref"], a["rs"], a["nerr"], None)

    demap_cases = [("null ctx", dict(ctx=None)), ("null eq", dict(eq=None)), ("null p", dict(null_p=True)),
                   ("null llr", dict(llr=None)), ("null h", dict(p={"h": None})), ("h_stride", dict(p={"h_stride": 52})),
                   ("modulation 3", dict(p={"modulation": 3})), ("modulation 0", dict(p={"modulation": 0})),
                   ("scale 0", dict(p={"scale": 0.0})), ("scale nan", dict(p={"scale": float("nan")})),
                   ("eq block stride", dict(ebs=52)), ("eq frame stride", dict(efs=14 * EBS + 52)),
                   ("llr block stride", dict(lbs=48 * mod - 1)), ("llr frame stride", dict(lfs=14 * lbs + 48 * mod - 1)),
                   ("eq alignment", dict(eq=deq.addr + 8)), ("h alignment", dict(p={"h": dh.addr + 8})),
                   ("llr alignment", dict(llr=dl.addr + 2)), ("n_frames < 0", dict(n=-1)),
                   ("n_frames 2^31", dict(n=2 ** 31))]
    vit_cases = [("null ctx", dict(ctx=None)), ("null llr", dict(llr=None)), ("modulation 3", dict(mod=3)),
                 ("modulation 0", dict(mod=0)), ("rate 3", dict(rate=3)), ("rate -1", dict(rate=-1)),
                 ("flags", dict(flags=2)), ("llr block stride", dict(lbs=48 * mod - 1)),
                 ("llr frame stride", dict(lfs=14 * lbs + 48 * mod - 1)), ("bits_stride", dict(bs=nby - 1)),
                 ("ref_stride", dict(rs=nby - 1)), ("nbiterr without ref_bits", dict(ref=None)),
                 ("no output", dict(bits=None, nerr=None)), ("llr alignment", dict(llr=dl.addr + 2)),
                 ("nbiterr alignment", dict(nerr=dn.addr + 2)), ("n_frames < 0", dict(n=-1)),
                 ("n_frames 2^31", dict(n=2 ** 31))]
    for call, cases in ((demap_call, demap_cases), (vit_call, vit_cases)):
        for name, kw in cases:
            assert lib.wce_decode_info_bits(0, 0) == -1                        # leaves its own text behind
            marker = lib.wce_last_error()
            assert call(**kw) == -1, name
            text = lib.wce_last_error()
            assert text and text != marker, name
    wce.synchronize()
    for a, b in zip(outs, before):                                             # nothing was launched
        assert np.array_equal(a.numpy().view(np.uint8), b.view(np.uint8))
    assert demap_call(n=0) == 0 and vit_call(n=0) == 0
    assert demap_call(n=0, efs=0, lfs=0) == 0 and vit_call(n=0, lfs=0) == 0
    wce.synchronize()
    assert np.array_equal(dbits.numpy(), before[1])
    assert demap_call(p={"flags": 0xFFFF, "h_lt": None}) == 0                  # flags are ignored
    assert vit_call() == 0 and vit_call(flags=0, bits=None) == 0 and vit_call(ref=None, nerr=None) == 0
    wce.synchronize()
    with pytest.raises(wce.WceError) as e:
        ctx.viterbi_decode(dl, B, mod, 7, bits=dbits)
    assert e.value.code == -1
