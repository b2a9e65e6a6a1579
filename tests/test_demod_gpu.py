"""wce_demodulate on the device against the long double model of
tests/demod_model.py: eq within TOL_EQ of the frame's max |e|, theta within
TOL_TH, evm within TOL_EVM relative (derived in tests/test_demod_abi.py, which
also holds the data to the conditions that make the exact comparisons of sym
and nerr legitimate).  Batches of 1, 5 and 67 frames; every stride padded, the
padding filled with a sentinel that must survive.

The chain tests compare with the model run on the model's own front end, whose
symbols the device's match to TOL_BINS = 2e-14 of their largest
(tests/test_cfo_gpu.py): that moves the EVM by at most 2 * 2e-14 * A / evm < 1e-12
(A / evm <= 22 on the recorded packet) and theta by about 1e-13, so the chain
holds evm to TOL_EVM + 1e-12 and theta to TOL_TH + 1e-13."""
import ctypes
import functools

import numpy as np
import pytest

import cfo_model as cm
import demod_model as dm
import sync_model as sm

pytestmark = pytest.mark.gpu

N, NBLK = dm.N, dm.NBLK
FS, BS, HS = 830, 55, 56            # frames: frame and block stride (15 blocks of stride 55 need 823: the 800 the
                                    # request for these tests names would not hold them); estimates: row stride
EFS, EBS = 15 * 56 + 3, 56          # eq and sym: frame and block stride
SENT, SENT8 = 7.0 - 3.0j, 0xA5
BATCHES = (1, 5, 67)
ALL_OUT = ("eq", "sym", "theta", "evm", "nerr")
CHAIN_TOL_EVM, CHAIN_TOL_TH = dm.TOL_EVM + 1e-12, dm.TOL_TH + 1e-13


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint8)


def _pad_frames(a):
    B = a.shape[0]
    out = np.full((B, FS), SENT, np.complex128)
    for b in range(NBLK):
        out[:, b * BS:b * BS + N] = a[:, b]
    return out


def _pad_rows(a):
    out = np.full((a.shape[0], HS), SENT, np.complex128)
    out[:, :N] = a
    return out


def _unpad(flat, fill):
    """[B][EFS] -> ([B][15][53], the padding is intact)"""
    B = flat.shape[0]
    mask = np.zeros(EFS, bool)
    for b in range(NBLK):
        mask[b * EBS:b * EBS + N] = True
    vals = np.stack([flat[:, b * EBS:b * EBS + N] for b in range(NBLK)], axis=1)
    return vals, bool(np.all(flat[:, ~mask] == fill))


class Run:
    """one wce_demodulate call on padded device buffers; .out holds the requested outputs unpadded"""

    def __init__(self, wce, ctx, tx, rx, h, h_lt, mod, track=True, ref_tx=True, outs=ALL_OUT, scale=dm.SCALE):
        B = tx.shape[0]
        self.B = B
        D = wce.DeviceArray.from_numpy
        self.keep = [D(_pad_frames(tx)), D(_pad_frames(rx)), D(_pad_rows(h)), D(_pad_rows(h_lt)) if h_lt is not None else None]
        self.fr = wce.Context.frames(self.keep[0], self.keep[1], B, frame_stride=FS, block_stride=BS)
        self.init = {"eq": np.full((B, EFS), SENT, np.complex128), "sym": np.full((B, EFS), SENT8, np.uint8),
                     "theta": np.full(B * NBLK + 1, 9.0), "evm": np.full(B + 1, 9.0),
                     "nerr": np.full(B + 1, 0xDEAD, np.uint32)}
        self.dev = {k: D(self.init[k]) for k in outs}
        self.kw = dict(h_lt=self.keep[3], h_stride=HS, modulation=mod, scale=scale, track=track, ref_tx=ref_tx,
                       eq_frame_stride=EFS, eq_block_stride=EBS, sym_frame_stride=EFS, sym_block_stride=EBS)
        ctx.demodulate(self.fr, self.keep[2], **self.kw, **self.dev)
        wce.synchronize()
        self.out = {}
        for k in outs:
            a = self.dev[k].numpy()
            if k in ("eq", "sym"):
                self.out[k], ok = _unpad(a, SENT if k == "eq" else SENT8)
                assert ok, f"{k}: padding overwritten"
            else:
                assert a[-1] == self.init[k][-1], f"{k}: written past the end"
                self.out[k] = a[:-1].reshape(B, NBLK) if k == "theta" else a[:-1]


@pytest.fixture(scope="module")
def ctx(gpu_wce):
    return gpu_wce.Context(empty=True)     # the ctx only selects the device


@functools.lru_cache(maxsize=None)
def _synthetic(mod):
    return dm.synthetic(mod)


@functools.lru_cache(maxsize=None)
def _model(mod, track, ref_tx, bl):
    tx, rx, h, h_lt = _synthetic(mod)
    return dm.demodulate(tx, rx, h, h_lt if bl else None, mod, track=track, ref_tx=ref_tx)


def _compare(out, ref, sl, what):
    """the device's outputs against the model's frames `sl`"""
    e = dm.relmax_frames(out["eq"], ref["eq"][sl])
    th = np.max(np.abs(out["theta"] - np.asarray(ref["theta"][sl], np.float64)))
    ev = np.max(np.abs(out["evm"] - ref["evm"][sl]) / ref["evm"][sl])
    print(f"{what}: eq {e.max():.2e} theta {th:.2e} evm {float(ev):.2e}")
    assert e.max() <= dm.TOL_EQ, what
    assert th <= dm.TOL_TH, what
    assert ev <= dm.TOL_EVM, what
    assert np.array_equal(out["sym"], ref["sym"][sl]), what
    assert np.array_equal(out["nerr"], ref["nerr"][sl]), what


# ---------------------------------------------------------------- 1. WCE_EQUALIZE's bits
@pytest.mark.parametrize("B", BATCHES)
def test_untracked_eq_is_equalize_bit_for_bit(gpu_wce, golden, B):
    wce, inp = gpu_wce, golden["inputs"]
    tx, rx, h, h_lt = (a[:B] for a in _synthetic(dm.BPSK))
    est = wce.Context(inp["tx_pre"], inp["rx_pre"], float(inp["ow2"]), wce.MMSE_REF)
    D = wce.DeviceArray.from_numpy
    dtx, drx = D(_pad_frames(tx)), D(_pad_frames(rx))
    dpre = D(_pad_rows(h_lt * inp["tx_pre"][None, :]))          # each frame's own preamble
    fr = wce.Context.frames(dtx, drx, B, frame_stride=FS, block_stride=BS, rx_pre=dpre, pre_stride=HS)
    names = ("lt_ls", "ps_linear", "ps_cubic", "ps_sinc")
    for src_name, src in (("ps_linear", wce.PS_LINEAR), ("ps_cubic", wce.PS_CUBIC), ("ps_sinc", wce.PS_SINC)):
        H = {n: D(np.full((B, HS), SENT, np.complex128)) for n in names}
        deq = D(np.full((B, EFS), SENT, np.complex128))
        o = wce.Outputs(H["lt_ls"].addr, H["ps_linear"].addr, H["ps_cubic"].addr, H["ps_sinc"].addr, None, deq.addr,
                        HS, EFS, EBS, src, 0)
        est.estimate(fr, o, wce.LS_ALL | wce.EQUALIZE)
        dem = D(np.full((B, EFS), SENT, np.complex128))
        est.demodulate(fr, H[src_name], h_lt=H["lt_ls"], h_stride=HS, track=False, eq=dem, eq_frame_stride=EFS,
                       eq_block_stride=EBS)
        wce.synchronize()
        a, b = deq.numpy(), dem.numpy()
        assert np.isfinite(_unpad(a, SENT)[0]).all() and _unpad(a, SENT)[1] and _unpad(b, SENT)[1]
        assert np.array_equal(_bits(a), _bits(b)), src_name


# ---------------------------------------------------------------- 2. the long double model
@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("mod", dm.MODS)
def test_parity_with_the_model(gpu_wce, ctx, mod, B):
    tx, rx, h, h_lt = (a[:B] for a in _synthetic(mod))
    for track in (True, False):
        for ref_tx in (True, False):
            for bl in (True, False):
                r = Run(gpu_wce, ctx, tx, rx, h, h_lt if bl else None, mod, track, ref_tx)
                _compare(r.out, _model(mod, track, ref_tx, bl), slice(0, B),
                         f"{mod} bits B={B} track={track} ref_tx={ref_tx} blend={bl}")
                if not track:
                    assert not np.any(r.out["theta"])


def test_parity_on_the_recorded_frames(gpu_wce, ctx, golden):
    for name, (tx, rx, h, h_lt) in dm.recorded(golden).items():
        for track in (True, False):
            for ref_tx in (True, False):
                r = Run(gpu_wce, ctx, tx, rx, h, h_lt, dm.BPSK, track, ref_tx)
                ref = dm.demodulate(tx, rx, h, h_lt, dm.BPSK, track=track, ref_tx=ref_tx)
                _compare(r.out, ref, slice(0, 1), f"{name} track={track} ref_tx={ref_tx}")
                assert r.out["nerr"][0] == 0


def test_matlab_eq_symbols_pin(gpu_wce, ctx, golden):
    """matlab.mat's eq_symbols from its own H_EST_LT_LS and H_EST_PS_Linear, no tracking: the tolerance of
    the existing pin (tests/test_matlab_gpu.py)"""
    m = golden["matlab"]
    tx, rx, h, h_lt = dm.recorded(golden)["matlab.mat"]
    got = Run(gpu_wce, ctx, tx, rx, h, h_lt, dm.BPSK, track=False, outs=("eq",)).out["eq"][0]
    ref = m["eq_symbols"].T
    assert np.max(np.abs(got - ref)) / np.max(np.abs(ref)) < 1e-13
    assert np.all(got[:, 26] == 0)


# ---------------------------------------------------------------- 3. what tracking promises
def test_phase_invariance_and_wrap(gpu_wce, ctx):
    tx, rx, h, h_lt, rot = dm.phase_set()
    a = Run(gpu_wce, ctx, tx, rx, h, h_lt, dm.QPSK).out
    b = Run(gpu_wce, ctx, tx, rot, h, h_lt, dm.QPSK).out
    assert dm.relmax_frames(b["eq"], a["eq"]).max() <= 2 * dm.TOL_EQ
    move = np.abs(dm.wrap(b["theta"] - a["theta"] - dm.PHI[None, :]))
    print(f"theta moves by phi to {float(move.max()):.2e}")
    assert move.max() <= dm.TOL_TH + 8 * 2.0 ** -53               # the rotation itself rounds rx and exp(i phi)
    assert np.all(np.abs(b["theta"]) <= np.pi) and np.any(b["theta"] > 3.0) and np.any(b["theta"] < -3.0)
    assert np.array_equal(a["sym"], b["sym"]) and np.array_equal(a["nerr"], b["nerr"])
    ref = dm.demodulate(tx, rot, h, h_lt, dm.QPSK)
    assert np.max(np.abs(dm.wrap(b["theta"] - ref["theta"]))) <= dm.TOL_TH
    assert np.array_equal(b["sym"], ref["sym"])


def test_zero_pilots(gpu_wce, ctx):
    tx, rx, h, h_lt = (a[:5].copy() for a in _synthetic(dm.QAM16))
    rx[3, 6, list(dm.PILOTS)] = 0
    rx[0, 14, list(dm.PILOTS)] = 0
    on = Run(gpu_wce, ctx, tx, rx, h, h_lt, dm.QAM16).out
    off = Run(gpu_wce, ctx, tx, rx, h, h_lt, dm.QAM16, track=False).out
    for f, b in ((3, 6), (0, 14)):
        assert on["theta"][f, b] == 0.0 and not np.signbit(on["theta"][f, b])
        assert np.array_equal(_bits(on["eq"][f, b]), _bits(off["eq"][f, b]))
        assert np.array_equal(on["sym"][f, b], off["sym"][f, b])
    assert np.count_nonzero(on["theta"]) == 5 * NBLK - 2
    assert not np.array_equal(on["eq"][3, 5], off["eq"][3, 5])


def test_isolation_of_non_finite_frames(gpu_wce, ctx):
    mod = dm.QAM64
    tx, rx, h, h_lt = (a.copy() for a in _synthetic(mod))
    clean = Run(gpu_wce, ctx, tx, rx, h, h_lt, mod).out
    h[9, 11] = np.nan                       # a data subcarrier of the estimate: its 15 symbols
    rx[40, 7, 30] = np.inf + 0j             # one received symbol
    got = Run(gpu_wce, ctx, tx, rx, h, h_lt, mod).out
    ref = dm.demodulate(tx, rx, h, h_lt, mod)
    bad = np.zeros(67, bool)
    bad[[9, 40]] = True
    assert np.all(got["sym"][9, :, 11] == 0xFF) and got["sym"][40, 7, 30] == 0xFF
    assert np.count_nonzero(got["sym"] == 0xFF) == 16
    assert np.isnan(got["evm"][bad]).all() and np.isfinite(got["evm"][~bad]).all()
    assert np.array_equal(got["sym"], ref["sym"]) and np.array_equal(got["nerr"], ref["nerr"])
    assert got["nerr"][9] >= 15 and got["nerr"][40] >= 1
    assert np.all(~np.isfinite(got["eq"][9, :, 11])) and not np.isfinite(got["eq"][40, 7, 30])
    for k in ALL_OUT:
        assert np.array_equal(_bits(got[k][~bad]), _bits(clean[k][~bad])), k


def test_position_independence(gpu_wce, ctx):
    mod = dm.QAM16
    tx, rx, h, h_lt = (a.copy() for a in _synthetic(mod))
    for a in (tx, rx, h, h_lt):
        a[66] = a[0]
    big = Run(gpu_wce, ctx, tx, rx, h, h_lt, mod).out
    one = Run(gpu_wce, ctx, tx[:1], rx[:1], h[:1], h_lt[:1], mod).out
    for k in ALL_OUT:
        assert np.array_equal(_bits(big[k][0]), _bits(one[k][0])), k
        assert np.array_equal(_bits(big[k][66]), _bits(one[k][0])), k


@pytest.mark.parametrize("track", [True, False])
def test_output_subsets(gpu_wce, ctx, track):
    mod = dm.QAM64
    tx, rx, h, h_lt = (a[:5] for a in _synthetic(mod))
    full = Run(gpu_wce, ctx, tx, rx, h, h_lt, mod, track).out
    for outs in (("eq",), ("evm", "nerr"), ("sym",), ("theta",), ("evm",), ("nerr",), ("eq", "sym", "theta")):
        for ref_tx in ((True, False) if "evm" in outs else (True,)):
            want = full if ref_tx else Run(gpu_wce, ctx, tx, rx, h, h_lt, mod, track, False).out
            part = Run(gpu_wce, ctx, tx, rx, h, h_lt, mod, track, ref_tx, outs=outs).out
            assert set(part) == set(outs)
            for k in outs:
                assert np.array_equal(_bits(part[k]), _bits(want[k])), (outs, k, ref_tx)


# ---------------------------------------------------------------- 4. arguments
def test_invalid_arguments(gpu_wce, ctx):
    wce = gpu_wce
    lib = wce.load()
    B = 5
    tx, rx, h, h_lt = (a[:B] for a in _synthetic(dm.BPSK))
    base = Run(wce, ctx, tx, rx, h, h_lt, dm.BPSK)
    before = {k: base.dev[k].numpy() for k in ALL_OUT}
    W = wce.wce

    def call(fr=None, p=None, o=None, null=()):
        """the base request with fields replaced; -> status"""
        f = W.Frames.from_buffer_copy(base.fr)
        for k, v in (fr or {}).items():
            setattr(f, k, v)
        P = W.Demod(base.keep[2].addr, base.keep[3].addr, HS, dm.BPSK, W.DEMOD_TRACK | W.DEMOD_REF_TX, dm.SCALE)
        for k, v in (p or {}).items():
            setattr(P, k, v)
        O = W.DemodOut(*[base.dev[k].addr for k in ALL_OUT], EFS, EBS, EFS, EBS)
        for k, v in (o or {}).items():
            setattr(O, k, v)
        args = [None if "in" in null else ctypes.byref(f), None if "p" in null else ctypes.byref(P),
                None if "out" in null else ctypes.byref(O)]
        return lib.wce_demodulate(ctx.handle, *args, None)

    assert call() == 0                                                     # the base request itself is fine
    wce.synchronize()
    before = {k: base.dev[k].numpy() for k in ALL_OUT}
    addr = lambda k, off: base.dev[k].addr + off
    cases = [("null in", dict(null=("in",))), ("null p", dict(null=("p",))), ("null out", dict(null=("out",))),
             ("null h", dict(p={"h": None})), ("null tx", dict(fr={"tx": None})), ("null rx", dict(fr={"rx": None})),
             ("no output", dict(o={k: None for k in ALL_OUT})),
             ("h_stride", dict(p={"h_stride": 52})),
             ("modulation 3", dict(p={"modulation": 3})), ("modulation 0", dict(p={"modulation": 0})),
             ("modulation 8", dict(p={"modulation": 8})), ("flags", dict(p={"flags": 4})),
             ("scale 0", dict(p={"scale": 0.0})), ("scale < 0", dict(p={"scale": -1.0})),
             ("scale inf", dict(p={"scale": float("inf")})), ("scale nan", dict(p={"scale": float("nan")})),
             ("eq block stride", dict(o={"eq_block_stride": 52})),
             ("eq frame stride", dict(o={"eq_frame_stride": 14 * EBS + 52})),
             ("sym block stride", dict(o={"sym_block_stride": 52})),
             ("sym frame stride", dict(o={"sym_frame_stride": 14 * EBS + 52})),
             ("theta alignment", dict(o={"theta": addr("theta", 4)})), ("evm alignment", dict(o={"evm": addr("evm", 4)})),
             ("nerr alignment", dict(o={"nerr": addr("nerr", 2)})),
             ("h alignment", dict(p={"h": base.keep[2].addr + 8})),
             ("h_lt alignment", dict(p={"h_lt": base.keep[3].addr + 8})),
             ("eq alignment", dict(o={"eq": addr("eq", 8)})),
             ("n_frames < 0", dict(fr={"n_frames": -1})), ("block_stride", dict(fr={"block_stride": 52})),
             ("frame_stride", dict(fr={"frame_stride": 14 * BS + 52}))]
    for name, kw in cases:
        assert lib.wce_demodulate(None, None, None, None, None) == -1      # leaves "null ctx" behind
        marker = lib.wce_last_error()
        assert call(**kw) == -1, name
        text = lib.wce_last_error()
        assert text and text != marker, name
    wce.synchronize()
    for k in ALL_OUT:
        assert np.array_equal(_bits(base.dev[k].numpy()), _bits(before[k])), k
    # what the call ignores is not checked, and an empty batch is fine whatever else it is given
    assert call(fr={"block": 99, "semantics": 7, "pre_stride": 0}) == 0
    assert call(fr={"n_frames": 0}) == 0
    assert call(p={"h_lt": None}, o={"sym": None, "sym_block_stride": 0}) == 0
    wce.synchronize()
    with pytest.raises(wce.WceError) as e:
        ctx.demodulate(base.fr, base.keep[2], modulation=5, evm=base.dev["evm"])
    assert e.value.code == -1 and "modulation" in str(e.value)


# ---------------------------------------------------------------- 5. the chains
def _chain_inputs(m):
    lp, pk = dm.rotated_packet(m)
    rx_pk, rx_lp = np.stack([m["rx_packet"], pk]), np.stack([m["rx_lptot"], lp])
    tx_pk, tx_lp = np.repeat(m["tx_packet"][None], 2, 0), np.repeat(m["tx_lptot"][None], 2, 0)
    return tx_pk, tx_lp, rx_pk, rx_lp


def test_receive_chain_demodulates(gpu_wce, golden):
    """receive_host on the recorded packet and its copy under the residual offset of tests/test_demod_abi.py:
    the demod dict against the model run on the model's front end and the device's own estimates"""
    wce, m = gpu_wce, golden["matlab"]
    tx_pk, tx_lp, rx_pk, rx_lp = _chain_inputs(m)
    c = wce.Context(m["tx_preamble_fft"], m["rx_preamble_fft"], 9.6172e-8, wce.MMSE_TEXTBOOK)
    plain = c.receive_host(tx_pk, tx_lp, rx_pk, rx_lp)
    assert "demod" not in plain
    assert set(plain) == {"lt_ls", "ps_linear", "ps_cubic", "ps_sinc", "ps_mmse", "eq", "ow2"}   # today's keys
    z = np.zeros(2)
    tx, rx = cm.blocks(tx_pk, z), cm.blocks(rx_pk, z)
    for src, name in ((wce.PS_MMSE, "ps_mmse"), (wce.PS_LINEAR, "ps_linear")):
        for track in (True, False):
            out = c.receive_host(tx_pk, tx_lp, rx_pk, rx_lp, demod_source=src, track=track)
            assert set(out) == set(plain) | {"demod"}
            for k in plain:
                assert np.array_equal(_bits(out[k]), _bits(plain[k])), k
            d = out["demod"]
            assert set(d) == set(ALL_OUT)
            ref = dm.demodulate(tx, rx, out[name], out["lt_ls"], dm.BPSK, track=track)
            assert float(np.min(ref["margin"])) > dm.MARGIN * dm.SCALE
            ev = np.abs(d["evm"] - ref["evm"]) / ref["evm"]
            th = np.abs(d["theta"] - np.asarray(ref["theta"], np.float64))
            print(f"{name} track={track}: evm {d['evm']} (model off by {float(ev.max()):.2e}), theta off by "
                  f"{float(th.max()):.2e}, nerr {d['nerr']}")
            assert ev.max() <= CHAIN_TOL_EVM and th.max() <= CHAIN_TOL_TH
            assert np.array_equal(d["nerr"], ref["nerr"]) and np.array_equal(d["sym"], ref["sym"])
            assert dm.relmax_frames(d["eq"], ref["eq"]).max() <= 1e-12
            if track:     # the residual is tracked out; untracked it costs what the CPU test says
                assert d["evm"][1] <= 1.1 * d["evm"][0]
            else:
                assert d["evm"][1] >= 2 * out["demod"]["evm"][0] and not np.any(d["theta"])
    with pytest.raises(ValueError):
        c.receive_host(tx_pk, tx_lp, rx_pk, rx_lp, mask=wce.LT_LS | wce.PS_MMSE, demod_source=wce.PS_LINEAR)


def test_receive_capture_chain_demodulates(gpu_wce, golden):
    """a window without a detected packet: NaN evm and 0xFF symbols for that frame only"""
    wce, m = gpu_wce, golden["matlab"]
    cap, ltf = sm.chain(m)
    B, P, f = len(cap), sm.CHAIN_PREFIX, sm.CHAIN_NOISE
    c = wce.Context(m["tx_preamble_fft"], m["rx_preamble_fft"], 9.6172e-8, wce.MMSE_TEXTBOOK)
    tx_pk, tx_lp = np.repeat(m["tx_packet"][None], B, 0), np.repeat(m["tx_lptot"][None], B, 0)
    plain = c.receive_capture_host(tx_pk, tx_lp, cap, 0.25, cfo=True)
    out = c.receive_capture_host(tx_pk, tx_lp, cap, 0.25, cfo=True, demod_source=wce.PS_MMSE)
    assert set(out) == set(plain) | {"demod"} and out["start"][f] == -1
    for k in plain:
        assert np.array_equal(_bits(out[k]), _bits(plain[k])), k
    d = out["demod"]
    det = np.arange(B) != f
    assert np.isnan(d["evm"][f]) and np.isfinite(d["evm"][det]).all() and np.all(d["evm"][det] < 0.1)
    data = np.zeros(N, bool)
    data[dm.DATA] = True
    assert np.all(d["sym"][f][:, data] == 0xFF) and d["nerr"][f] == 48 * NBLK
    assert not np.any(d["sym"][det] == 0xFF) and not np.any(d["nerr"][det])
    # the detected frames: the aligned inputs through receive_host, bit for bit
    ref = c.receive_host(tx_pk[det], tx_lp[det], cap[det][:, P + 160:], cap[det][:, P:P + 160], cfo=True,
                         demod_source=wce.PS_MMSE)["demod"]
    for k in ALL_OUT:
        assert np.array_equal(_bits(d[k][det]), _bits(ref[k])), k
