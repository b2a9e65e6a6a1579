"""wce_track_demodulate and wce_soft_demap_blocks on the device against the long
double model of tests/track_model.py: eq within TOL_EQ_T of the frame's max |e|,
h_blocks and h_last within TOL_H_T of the frame's max |H|, theta within TOL_TH, evm
within TOL_EVM_T relative (set and checked in tests/test_track_abi.py, which also
holds the data to the conditions that make the exact comparisons of sym and nerr
legitimate).  Batches of 1, 5 and 67 frames; every stride padded, the padding
filled with a sentinel that must survive.

The chain: on the coded 16-QAM rate 1/2 set of track_model.coded_set (67 frames,
22 dB, rho = 0.995) the tracked chain (mu = 0.5, beta = 2) leaves 945 bit errors
and the static chain (wce_demodulate with h, wce_soft_demap, the same decoder)
3126, on the model and on the device."""
import ctypes
import functools

import numpy as np
import pytest

import cfo_model as cm
import demod_model as dm
import fec_model as fm
import track_model as tm

pytestmark = pytest.mark.gpu

N, NBLK = dm.N, dm.NBLK
FS, BS, HS = 830, 55, 56            # frames: frame and block stride; estimates: row stride
EFS, EBS = 15 * 56 + 3, 56          # eq, sym and h_blocks: frame and block stride
SENT, SENT8, SENTF = 7.0 - 3.0j, 0xA5, np.float32(-77.0)
BATCHES = (1, 5, 67)
ALL_OUT = ("eq", "sym", "theta", "evm", "nerr", "h_blocks", "h_last")
CHAIN_TOL_EVM, CHAIN_TOL_TH = dm.TOL_EVM + 1e-12, dm.TOL_TH + 1e-13    # tests/test_demod_gpu.py's


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def _pad_frames(a, fs=FS, bs=BS):
    out = np.full((a.shape[0], fs), SENT, np.complex128)
    for b in range(NBLK):
        out[:, b * bs:b * bs + N] = a[:, b]
    return out


def _pad_rows(a):
    out = np.full((a.shape[0], HS), SENT, np.complex128)
    out[:, :N] = a
    return out


def _unpad(flat, fill):
    """[B][EFS] -> ([B][15][53], the padding is intact)"""
    mask = np.zeros(EFS, bool)
    for b in range(NBLK):
        mask[b * EBS:b * EBS + N] = True
    vals = np.stack([flat[:, b * EBS:b * EBS + N] for b in range(NBLK)], axis=1)
    return vals, bool(np.all(flat[:, ~mask] == fill))


class Run:
    """one wce_track_demodulate call on padded device buffers; .out holds the requested outputs unpadded"""

    def __init__(self, wce, ctx, tx, rx, h, mod, mu, beta, phase=True, ref_tx=True, known_tx=False, outs=ALL_OUT,
                 scale=dm.SCALE):
        B = tx.shape[0]
        D = wce.DeviceArray.from_numpy
        self.keep = [D(_pad_frames(tx)), D(_pad_frames(rx)), D(_pad_rows(h))]
        self.fr = wce.Context.frames(self.keep[0], self.keep[1], B, frame_stride=FS, block_stride=BS)
        self.init = {"eq": np.full((B, EFS), SENT, np.complex128), "sym": np.full((B, EFS), SENT8, np.uint8),
                     "theta": np.full(B * NBLK + 1, 9.0), "evm": np.full(B + 1, 9.0),
                     "nerr": np.full(B + 1, 0xDEAD, np.uint32), "h_blocks": np.full((B, EFS), SENT, np.complex128),
                     "h_last": np.full((B, HS), SENT, np.complex128)}
        self.dev = {k: D(self.init[k]) for k in outs}
        self.kw = dict(h_stride=HS, modulation=mod, scale=scale, phase=phase, ref_tx=ref_tx, known_tx=known_tx,
                       eq_frame_stride=EFS, eq_block_stride=EBS, sym_frame_stride=EFS, sym_block_stride=EBS,
                       hb_frame_stride=EFS, hb_block_stride=EBS, h_last_stride=HS)
        ctx.track_demodulate(self.fr, self.keep[2], mu, beta, **self.kw, **self.dev)
        wce.synchronize()
        self.out = {}
        for k in outs:
            a = self.dev[k].numpy()
            if k in ("eq", "sym", "h_blocks"):
                self.out[k], ok = _unpad(a, SENT8 if k == "sym" else SENT)
                assert ok, f"{k}: padding overwritten"
            elif k == "h_last":
                assert np.all(a[:, N:] == SENT), "h_last: padding overwritten"
                self.out[k] = a[:, :N]
            else:
                assert a[-1] == self.init[k][-1], f"{k}: written past the end"
                self.out[k] = a[:-1].reshape(B, NBLK) if k == "theta" else a[:-1]


@pytest.fixture(scope="module")
def ctx(gpu_wce):
    return gpu_wce.Context(empty=True)     # the ctx only selects the device


def _compare(out, ref, sl, what):
    """the device's outputs against the model's frames `sl`"""
    e = dm.relmax_frames(out["eq"], ref["eq"][sl]).max()
    hb = dm.relmax_frames(out["h_blocks"], ref["h_blocks"][sl]).max()
    hl = dm.relmax_frames(out["h_last"], ref["h_last"][sl]).max()
    th = np.max(np.abs(out["theta"] - np.asarray(ref["theta"][sl], np.float64)))
    ev = np.max(np.abs(out["evm"] - ref["evm"][sl]) / ref["evm"][sl])
    print(f"{what}: eq {e:.2e} h_blocks {hb:.2e} h_last {hl:.2e} theta {th:.2e} evm {float(ev):.2e}")
    assert e <= tm.TOL_EQ_T, what
    assert hb <= tm.TOL_H_T and hl <= tm.TOL_H_T, what
    assert th <= tm.TOL_TH, what
    assert ev <= tm.TOL_EVM_T, what
    assert np.array_equal(out["sym"], ref["sym"][sl]), what
    assert np.array_equal(out["nerr"], ref["nerr"][sl]), what


# ---------------------------------------------------------------- 1. the long double model
@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("mod", dm.MODS)
def test_parity_with_the_model(gpu_wce, ctx, mod, B):
    tx, rx, h = (a[:B] for a in tm.drifting_set(mod))
    for mu, beta, phase, known in tm.COMBOS:
        r = Run(gpu_wce, ctx, tx, rx, h, mod, mu, beta, phase, True, known)
        _compare(r.out, tm.model(mod, mu, beta, phase, known), slice(0, B),
                 f"{mod} bits B={B} mu={mu} beta={beta} phase={phase} known={known}")
        if not phase:
            assert not np.any(r.out["theta"])
    # EVM against the decided points
    r = Run(gpu_wce, ctx, tx, rx, h, mod, tm.MU, tm.BETA, ref_tx=False)
    _compare(r.out, tm.model(mod, tm.MU, tm.BETA, ref_tx=False), slice(0, B), f"{mod} bits B={B} decided reference")


# ---------------------------------------------------------------- 2. mu = 0 is wce_demodulate
@pytest.mark.parametrize("mod", dm.MODS)
def test_mu_zero_against_demodulate(gpu_wce, ctx, mod):
    wce = gpu_wce
    tx, rx, h = tm.drifting_set(mod)
    for phase in (True, False):
        r = Run(wce, ctx, tx, rx, h, mod, 0.0, 3, phase)
        d = {"eq": wce.DeviceArray.from_numpy(np.full((67, EFS), SENT, np.complex128)),
             "sym": wce.DeviceArray.from_numpy(np.full((67, EFS), SENT8, np.uint8)),
             "theta": wce.DeviceArray((67, NBLK), np.float64, zero=True),
             "evm": wce.DeviceArray((67,), np.float64, zero=True), "nerr": wce.DeviceArray((67,), np.uint32, zero=True)}
        ctx.demodulate(r.fr, r.keep[2], h_stride=HS, modulation=mod, track=phase, eq_frame_stride=EFS,
                       eq_block_stride=EBS, sym_frame_stride=EFS, sym_block_stride=EBS, **d)
        wce.synchronize()
        ref = {k: a.numpy() for k, a in d.items()}
        ref["eq"], ref["sym"] = _unpad(ref["eq"], SENT)[0], _unpad(ref["sym"], SENT8)[0]
        assert np.array_equal(r.out["sym"], ref["sym"]) and np.array_equal(r.out["nerr"], ref["nerr"])
        e = dm.relmax_frames(r.out["eq"], ref["eq"]).max()
        th = np.max(np.abs(r.out["theta"] - ref["theta"]))
        ev = np.max(np.abs(r.out["evm"] - ref["evm"]) / ref["evm"])
        print(f"{mod} bits phase={phase}: eq {e:.2e} theta {th:.2e} evm {ev:.2e}")
        assert e <= tm.TOL_EQ_T and th <= tm.TOL_TH and ev <= tm.TOL_EVM_T
        want = np.repeat(h[:, None, :], NBLK, axis=1)
        assert np.array_equal(_bits(r.out["h_blocks"]), _bits(want))
        assert np.array_equal(_bits(r.out["h_last"]), _bits(h))


# ---------------------------------------------------------------- 3. the window's geometry
@pytest.mark.parametrize("beta", range(5))
def test_window_geometry(gpu_wce, ctx, beta):
    """known tx, mu = 1, no phase: with rx_b[k] = tx_b[k] (k + 1 + i b), H_{b+1}[k] is the window mean of the small
    integers j + 1 + i b over N_k: an off-by-one at DC, at either edge or in lanes 53..63 moves it by far more than
    4 ulp.  BPSK at scale 8: tx = +-8, so G is the integers themselves"""
    B = 5
    rng = np.random.default_rng(beta)
    tx = np.where(rng.integers(0, 2, (B, NBLK, N)) > 0, 8.0, -8.0).astype(np.complex128)
    tx[:, :, dm.DC] = 0
    g = (np.arange(N)[None, None, :] + 1) + 1j * np.arange(NBLK)[None, :, None]
    rx = tx * g
    rx[:, :, dm.DC] = 1e3 - 1e3j                       # whatever arrives at DC is never read
    h = np.full((B, N), 3.0 - 2.0j)
    h[:, dm.DC] = 0.5j
    out = Run(gpu_wce, ctx, tx, rx, h, dm.BPSK, 1.0, beta, phase=False, known_tx=True, scale=8.0).out
    W, cnt = tm.window(beta)
    got = np.concatenate([out["h_blocks"], out["h_last"][:, None]], axis=1)          # H_0 .. H_15
    assert np.array_equal(_bits(got[:, 0]), _bits(h))
    for b in range(NBLK):
        mean = (W[tm.V] @ np.broadcast_to(g[0, b], (N,)).astype(np.clongdouble)) / cnt[tm.V]
        err = np.abs(got[:, b + 1][:, tm.V] - mean[None, :])
        ulp = np.spacing(np.abs(np.asarray(mean, np.complex128)))
        assert np.all(err <= 4 * ulp[None, :]), (beta, b, float(np.max(err / ulp)))
    assert np.all(got[:, :, dm.DC] == 0.5j)
    assert not out["nerr"].any()                      # every H_b keeps Re e on tx's side of the BPSK boundary


# ---------------------------------------------------------------- 4. subsets of the outputs
@pytest.mark.parametrize("known", [False, True])
def test_output_subsets(gpu_wce, ctx, known):
    mod = dm.QAM64
    tx, rx, h = (a[:5] for a in tm.drifting_set(mod))
    full = Run(gpu_wce, ctx, tx, rx, h, mod, tm.MU, tm.BETA, known_tx=known).out
    dec = Run(gpu_wce, ctx, tx, rx, h, mod, tm.MU, tm.BETA, ref_tx=False, known_tx=known).out
    for k in ALL_OUT:
        if k != "evm":
            assert np.array_equal(_bits(dec[k]), _bits(full[k])), k
    subsets = [(k,) for k in ALL_OUT] + [("evm", "nerr"), ("eq", "h_blocks"), ("eq", "sym", "theta"),
                                         ("h_blocks", "h_last")]
    for outs in subsets:
        for ref_tx in ((True, False) if "evm" in outs else (True,)):
            part = Run(gpu_wce, ctx, tx, rx, h, mod, tm.MU, tm.BETA, ref_tx=ref_tx, known_tx=known, outs=outs).out
            assert set(part) == set(outs)           # Run checked that nothing else was written: it was never there
            for k in outs:
                assert np.array_equal(_bits(part[k]), _bits((full if ref_tx else dec)[k])), (outs, k, ref_tx)


# ---------------------------------------------------------------- 5. and 6. a frame depends on itself alone
def test_isolation_of_non_finite_frames(gpu_wce, ctx):
    mod = dm.QAM16
    tx, rx, h = (a.copy() for a in tm.drifting_set(mod))
    clean = Run(gpu_wce, ctx, tx, rx, h, mod, tm.MU, tm.BETA).out
    rx[40, 7, 30] = np.nan                  # one received data symbol
    h[9, 11] = np.inf + 0j                  # a data subcarrier of the starting estimate
    got = Run(gpu_wce, ctx, tx, rx, h, mod, tm.MU, tm.BETA).out
    bad = np.zeros(67, bool)
    bad[[9, 40]] = True
    assert np.isnan(got["evm"][bad]).all() and np.isfinite(got["evm"][~bad]).all()
    assert got["sym"][40, 7, 30] == 0xFF and got["nerr"][40] >= 1
    assert not np.any(got["sym"][~bad] == 0xFF)
    # before the poisoned symbol frame 40 is untouched; after it only subcarriers within beta of it may differ
    assert np.array_equal(_bits(got["eq"][40, :7]), _bits(clean["eq"][40, :7]))
    far = np.abs(np.arange(N) - 30) > tm.BETA * (NBLK - 8)
    assert np.all(np.isfinite(got["h_blocks"][40][:, far])) and not np.all(np.isfinite(got["h_blocks"][40]))
    for k in ALL_OUT:
        assert np.array_equal(_bits(got[k][~bad]), _bits(clean[k][~bad])), k


def test_position_independence(gpu_wce, ctx):
    mod = dm.QAM16
    tx, rx, h = (a.copy() for a in tm.drifting_set(mod))
    for a in (tx, rx, h):
        a[41] = a[0]
    big = Run(gpu_wce, ctx, tx, rx, h, mod, tm.MU, tm.BETA).out
    one = Run(gpu_wce, ctx, tx[:1], rx[:1], h[:1], mod, tm.MU, tm.BETA).out
    for k in ALL_OUT:
        assert np.array_equal(_bits(big[k][0]), _bits(one[k][0])), k
        assert np.array_equal(_bits(big[k][41]), _bits(one[k][0])), k


# ---------------------------------------------------------------- 7. arguments
def test_invalid_arguments(gpu_wce, ctx):
    wce = gpu_wce
    lib = wce.load()
    B = 5
    tx, rx, h = (a[:B] for a in tm.drifting_set(dm.BPSK))
    base = Run(wce, ctx, tx, rx, h, dm.BPSK, tm.MU, tm.BETA)
    W = wce.wce

    def call(fr=None, p=None, o=None, null=()):
        """the base request with fields replaced; -> status"""
        f = W.Frames.from_buffer_copy(base.fr)
        for k, v in (fr or {}).items():
            setattr(f, k, v)
        P = W.Track(base.keep[2].addr, HS, dm.BPSK, W.TRACK_PHASE | W.TRACK_REF_TX, dm.SCALE, tm.MU, tm.BETA)
        for k, v in (p or {}).items():
            setattr(P, k, v)
        d = base.dev
        O = W.TrackOut(d["eq"].addr, d["sym"].addr, d["theta"].addr, d["evm"].addr, d["nerr"].addr, EFS, EBS, EFS, EBS,
                       d["h_blocks"].addr, EFS, EBS, d["h_last"].addr, HS)
        for k, v in (o or {}).items():
            setattr(O, k, v)
        args = [None if "in" in null else ctypes.byref(f), None if "p" in null else ctypes.byref(P),
                None if "out" in null else ctypes.byref(O)]
        return lib.wce_track_demodulate(ctx.handle, *args, None)

    assert call() == 0                                                     # the base request itself is fine
    wce.synchronize()
    before = {k: base.dev[k].numpy() for k in ALL_OUT}
    addr = lambda k, off: base.dev[k].addr + off
    inf, nan = float("inf"), float("nan")
    cases = [("null in", dict(null=("in",))), ("null p", dict(null=("p",))), ("null out", dict(null=("out",))),
             ("null h", dict(p={"h": None})), ("null tx", dict(fr={"tx": None})), ("null rx", dict(fr={"rx": None})),
             ("no output", dict(o={k: None for k in ALL_OUT})),
             ("h_stride", dict(p={"h_stride": 52})),
             ("modulation 3", dict(p={"modulation": 3})), ("modulation 0", dict(p={"modulation": 0})),
             ("modulation 8", dict(p={"modulation": 8})), ("flags", dict(p={"flags": 8})),
             ("scale 0", dict(p={"scale": 0.0})), ("scale < 0", dict(p={"scale": -1.0})),
             ("scale inf", dict(p={"scale": inf})), ("scale nan", dict(p={"scale": nan})),
             ("mu < 0", dict(p={"mu": -0.125})), ("mu > 1", dict(p={"mu": 1.0000001})),
             ("mu inf", dict(p={"mu": inf})), ("mu nan", dict(p={"mu": nan})),
             ("beta < 0", dict(p={"beta": -1})), ("beta 5", dict(p={"beta": 5})),
             ("eq block stride", dict(o={"eq_block_stride": 52})),
             ("eq frame stride", dict(o={"eq_frame_stride": 14 * EBS + 52})),
             ("sym block stride", dict(o={"sym_block_stride": 52})),
             ("sym frame stride", dict(o={"sym_frame_stride": 14 * EBS + 52})),
             ("h_blocks block stride", dict(o={"hb_block_stride": 52})),
             ("h_blocks frame stride", dict(o={"hb_frame_stride": 14 * EBS + 52})),
             ("h_last stride", dict(o={"h_last_stride": 52})),
             ("theta alignment", dict(o={"theta": addr("theta", 4)})), ("evm alignment", dict(o={"evm": addr("evm", 4)})),
             ("nerr alignment", dict(o={"nerr": addr("nerr", 2)})),
             ("h alignment", dict(p={"h": base.keep[2].addr + 8})),
             ("eq alignment", dict(o={"eq": addr("eq", 8)})),
             ("h_blocks alignment", dict(o={"h_blocks": addr("h_blocks", 8)})),
             ("h_last alignment", dict(o={"h_last": addr("h_last", 8)})),
             ("n_frames < 0", dict(fr={"n_frames": -1})), ("block_stride", dict(fr={"block_stride": 52})),
             ("frame_stride", dict(fr={"frame_stride": 14 * BS + 52}))]
    for name, kw in cases:
        assert lib.wce_track_demodulate(None, None, None, None, None) == -1   # leaves "null ctx" behind
        marker = lib.wce_last_error()
        assert call(**kw) == -1, name
        text = lib.wce_last_error()
        assert text and text != marker, name
    wce.synchronize()
    for k in ALL_OUT:
        assert np.array_equal(_bits(base.dev[k].numpy()), _bits(before[k])), k
    # the ends of the ranges, what the call ignores, an empty batch
    assert call(p={"mu": 0.0, "beta": 0}) == 0 and call(p={"mu": 1.0, "beta": 4}) == 0
    assert call(fr={"block": 99, "semantics": 7, "pre_stride": 0}) == 0
    assert call(fr={"n_frames": 0}) == 0
    assert call(o={"h_blocks": None, "hb_block_stride": 0, "h_last": None, "h_last_stride": 0}) == 0
    wce.synchronize()
    with pytest.raises(wce.WceError) as e:
        ctx.track_demodulate(base.fr, base.keep[2], 0.5, 7, evm=base.dev["evm"])
    assert e.value.code == -1 and "beta" in str(e.value)


# ---------------------------------------------------------------- 8. soft bits with an estimate per block
def _pad_llr(B, mod):
    lbs = 48 * mod + 5
    return np.full((B, 15 * lbs + 7), SENTF, np.float32), lbs


def _unpad_llr(flat, mod, lbs):
    mask = np.zeros(flat.shape[1], bool)
    for b in range(NBLK):
        mask[b * lbs:b * lbs + 48 * mod] = True
    assert np.all(flat[:, ~mask] == SENTF), "llr: padding overwritten"
    return np.stack([flat[:, b * lbs:b * lbs + 48 * mod] for b in range(NBLK)], axis=1)


def demap_blocks(wce, ctx, eq, hb, mod):
    """one wce_soft_demap_blocks call on padded device buffers -> llr [B][15][48 mod]"""
    B = eq.shape[0]
    D = wce.DeviceArray.from_numpy
    flat, lbs = _pad_llr(B, mod)
    keep = [D(_pad_frames(eq, EFS, EBS)), D(_pad_frames(hb, FS, BS))]
    dl = D(flat)
    ctx.soft_demap_blocks(keep[0], keep[1], B, modulation=mod, llr=dl, eq_frame_stride=EFS, eq_block_stride=EBS,
                          hb_frame_stride=FS, hb_block_stride=BS, llr_frame_stride=flat.shape[1],
                          llr_block_stride=lbs)
    wce.synchronize()
    return _unpad_llr(dl.numpy(), mod, lbs)


@functools.lru_cache(maxsize=None)
def _tracked64(mod):
    """the fp64 model's eq and h_blocks on the drifting set, as complex128"""
    r = tm.model(mod, tm.MU, tm.BETA, real=np.float64)
    return np.asarray(r["eq"], np.complex128), np.asarray(r["h_blocks"], np.complex128)


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("mod", dm.MODS)
def test_soft_demap_blocks_on_constant_rows_is_soft_demap(gpu_wce, ctx, mod, B):
    wce = gpu_wce
    eq = _tracked64(mod)[0][:B]
    h = tm.drifting_set(mod)[2][:B].copy()
    h[B // 2, 17] = np.nan                                  # an erasure: the same bits there too
    got = demap_blocks(wce, ctx, eq, np.repeat(h[:, None, :], NBLK, axis=1), mod)
    D = wce.DeviceArray.from_numpy
    flat, lbs = _pad_llr(B, mod)
    keep, dl = [D(_pad_frames(eq, EFS, EBS)), D(_pad_rows(h))], D(flat)
    ctx.soft_demap(keep[0], keep[1], B, h_stride=HS, modulation=mod, llr=dl, eq_frame_stride=EFS,
                   eq_block_stride=EBS, llr_frame_stride=flat.shape[1], llr_block_stride=lbs)
    wce.synchronize()
    want = _unpad_llr(dl.numpy(), mod, lbs)
    assert np.any(want != 0) and np.array_equal(_bits(got), _bits(want))


@pytest.mark.parametrize("mod", [dm.QAM16, dm.QAM64])
def test_soft_demap_blocks_parity(gpu_wce, ctx, mod):
    """against fec_model's demapper fed H_b, at tests/test_decode_gpu.py's bound"""
    eq, hb = _tracked64(mod)
    ld = np.asarray(fm.llr(eq, hb, mod), np.longdouble)
    for B in BATCHES:
        L = demap_blocks(gpu_wce, ctx, eq[:B], hb[:B], mod)
        assert L.dtype == np.float32 and L.shape == (B, NBLK, 48 * mod)
        mx = np.max(np.abs(ld[:B]), axis=(1, 2), keepdims=True)
        err = np.abs(L.astype(np.longdouble) - ld[:B])
        print(f"{mod} bits B={B}: worst |dL| - 2^-23 |L| = "
              f"{float(np.max((err - 2.0 ** -23 * np.abs(ld[:B])) / mx)):.2e} of max |L|")
        assert np.all(err <= 2.0 ** -23 * np.abs(ld[:B]) + fm.TOL_ABS * mx)
    # the weights do differ from block to block: the constant-row call is another result
    const = demap_blocks(gpu_wce, ctx, eq[:5], np.repeat(hb[:5, :1], NBLK, axis=1), mod)
    assert not np.array_equal(const[:, 1:], demap_blocks(gpu_wce, ctx, eq[:5], hb[:5], mod)[:, 1:])


# ---------------------------------------------------------------- 9. the chains
def test_tracked_chain_decodes_better(gpu_wce, ctx):
    """track_decode_host on the coded 16-QAM rate 1/2 set: the bit errors of the model chain (track, fec_model's soft
    bits weighed by |H_b|^2, fec_model's decoder), 945, and fewer than decode_host leaves with the static h on the
    same frames, 3126."""
    mod, rate = dm.QAM16, fm.RATE_1_2
    s = tm.coded_set()
    out = ctx.track_decode_host(s["tx"], s["rx"], s["h"], mod, rate, tm.MU, tm.BETA, ref_bits=s["u"])
    assert set(out) == {"demod", "llr", "bits", "nbiterr"} and set(out["demod"]) == set(ALL_OUT)
    tracked, static = tm.decode_chain(s)
    # the device's own soft bits through the model's decoder, then the model's whole chain
    assert np.array_equal(out["nbiterr"], np.sum(fm.decode(out["llr"], mod, rate) != s["u"], axis=1))
    assert np.array_equal(out["nbiterr"], np.sum(out["bits"] != s["u"], axis=1))
    assert np.array_equal(out["nbiterr"], tracked)
    dem = ctx.demodulate_host(s["tx"], s["rx"], s["h"], None, mod)
    st = ctx.decode_host(dem["eq"], s["h"], None, mod, rate, ref_bits=s["u"])
    print(f"bit errors: tracked {int(out['nbiterr'].sum())} (model {int(tracked.sum())}), "
          f"static {int(st['nbiterr'].sum())} (model {int(static.sum())})")
    assert np.array_equal(st["nbiterr"], static)
    assert out["nbiterr"].sum() < st["nbiterr"].sum()
    # the demodulator inside the chain is the call itself
    alone = ctx.track_demodulate_host(s["tx"], s["rx"], s["h"], tm.MU, tm.BETA, mod)
    for k in ALL_OUT:
        assert np.array_equal(_bits(alone[k]), _bits(out["demod"][k])), k


def test_receive_chain_tracks(gpu_wce, golden):
    """receive_host(tracker=(0.5, 2), demod_source=PS_MMSE) on the recorded packet and its copy under the residual
    offset of tests/test_demod_abi.py: the demod dict against the model run on the model's front end and the
    device's own estimates; tracker=None is the call without the keyword"""
    wce, m = gpu_wce, golden["matlab"]
    lp, pk = dm.rotated_packet(m)
    rx_pk, rx_lp = np.stack([m["rx_packet"], pk]), np.stack([m["rx_lptot"], lp])
    tx_pk, tx_lp = np.repeat(m["tx_packet"][None], 2, 0), np.repeat(m["tx_lptot"][None], 2, 0)
    c = wce.Context(m["tx_preamble_fft"], m["rx_preamble_fft"], 9.6172e-8, wce.MMSE_TEXTBOOK)
    plain = c.receive_host(tx_pk, tx_lp, rx_pk, rx_lp, demod_source=wce.PS_MMSE, decode_rate=wce.RATE_1_2)
    none = c.receive_host(tx_pk, tx_lp, rx_pk, rx_lp, demod_source=wce.PS_MMSE, decode_rate=wce.RATE_1_2, tracker=None)
    assert set(plain["demod"]) == {"eq", "sym", "theta", "evm", "nerr"}
    for k in ("eq", "sym", "theta", "evm", "nerr"):
        assert np.array_equal(_bits(plain["demod"][k]), _bits(none["demod"][k])), k
    assert np.array_equal(plain["decode"]["llr"], none["decode"]["llr"])
    z = np.zeros(2)
    tx, rx = cm.blocks(tx_pk, z), cm.blocks(rx_pk, z)
    for track in (True, False):
        out = c.receive_host(tx_pk, tx_lp, rx_pk, rx_lp, demod_source=wce.PS_MMSE, track=track,
                             decode_rate=wce.RATE_1_2, tracker=(tm.MU, tm.BETA))
        assert set(out) == set(plain)
        for k in set(plain) - {"demod", "decode"}:
            assert np.array_equal(_bits(out[k]), _bits(plain[k])), k
        d = out["demod"]
        assert set(d) == set(ALL_OUT)
        ref = tm.track(tx, rx, out["ps_mmse"], dm.BPSK, tm.MU, tm.BETA, phase=track)
        assert float(np.min(ref["margin"])) > dm.MARGIN * dm.SCALE
        ev = np.abs(d["evm"] - ref["evm"]) / ref["evm"]
        th = np.abs(d["theta"] - np.asarray(ref["theta"], np.float64))
        print(f"track={track}: evm {d['evm']} (model off by {float(ev.max()):.2e}), theta off by "
              f"{float(th.max()):.2e}, nerr {d['nerr']}; static evm {plain['demod']['evm']}")
        assert ev.max() <= CHAIN_TOL_EVM and th.max() <= CHAIN_TOL_TH
        assert np.array_equal(d["nerr"], ref["nerr"]) and np.array_equal(d["sym"], ref["sym"])
        assert dm.relmax_frames(d["eq"], ref["eq"]).max() <= 1e-12
        assert dm.relmax_frames(d["h_blocks"], ref["h_blocks"]).max() <= 1e-12
        assert dm.relmax_frames(d["h_last"], ref["h_last"]).max() <= 1e-12
        assert np.array_equal(_bits(d["h_blocks"][:, 0]), _bits(out["ps_mmse"]))
        # the soft bits are weighed by the tracked estimates
        L = out["decode"]["llr"]
        ld = np.asarray(fm.llr(d["eq"], d["h_blocks"], dm.BPSK), np.longdouble)
        mx = np.max(np.abs(ld), axis=(1, 2), keepdims=True)
        assert np.all(np.abs(L.astype(np.longdouble) - ld) <= 2.0 ** -23 * np.abs(ld) + fm.TOL_ABS * mx)
    with pytest.raises(ValueError):
        c.receive_host(tx_pk, tx_lp, rx_pk, rx_lp, tracker=(tm.MU, tm.BETA))
