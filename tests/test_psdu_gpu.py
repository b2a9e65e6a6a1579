"""wce_psdu_frame and wce_psdu_deframe on the device against tests/psdu_model.py, bit for bit (there is no
arithmetic to round: every comparison is exact).

B = 131 where nothing else is said: prime, so ragged for 1, 2, 4 or 8 frames per wave, and >= 127, so that
every scrambler seed occurs.  Rows have odd strides and an odd base address; every buffer is sentinel-filled
and every byte the calls must not write is checked to be the sentinel still."""
import numpy as np
import pytest

import fec_model as fm
import psdu_model as pm
import tx_model as tm

pytestmark = pytest.mark.gpu

B = 131
SENT = 0xA5
GRID = 6                      # WCE_VARIANT_GRID


@pytest.fixture(scope="module")
def ctx(gpu_wce):
    return gpu_wce.Context(empty=True)     # the ctx only selects the device


def _case(mod, rate, n=B, seed=0):
    """n frames: seeds cover 1..127, lengths 4, 5, max - 1, max and random ones -> payloads (list), lengths, seeds"""
    rng = np.random.default_rng(1000 * mod + 10 * rate + seed)
    mx = pm.max_len(mod, rate)
    lengths = rng.integers(4, mx + 1, n).astype(np.int32)
    k = min(n, 8)
    lengths[:k] = [4, 5, mx - 1, mx, 6, 7, 8, 12][:k]
    seeds = (np.arange(n) % 127 + 1).astype(np.uint8)
    rng.shuffle(seeds)
    payloads = [rng.integers(0, 256, int(L) - 4).astype(np.uint8) for L in lengths]
    return payloads, lengths, seeds


class Rows:
    """a sentinel-filled device byte buffer of n rows of `stride` bytes from an odd base address"""

    def __init__(self, wce, n, stride, rows=None):
        self.wce, self.n, self.stride = wce, n, stride
        self.host = np.full(1 + n * stride + 8, SENT, np.uint8)
        if rows is not None:
            for f, r in enumerate(rows):
                self.host[1 + f * stride:1 + f * stride + len(r)] = r
        self.d = wce.DeviceArray.from_numpy(self.host)

    @property
    def addr(self):
        return self.d.addr + 1

    def get(self):
        """-> (rows [n][stride], the bytes in front of and behind them)"""
        a = self.d.numpy()
        return a[1:1 + self.n * self.stride].reshape(self.n, self.stride), np.concatenate([a[:1], a[1 + self.n * self.stride:]])


def _frame_device(wce, ctx, mod, rate, payloads, lengths, seeds, scalar=False, n=None):
    """-> (rows [n][bits_stride], guard bytes).  scalar: the length / seed form (all frames alike)"""
    n = len(payloads) if n is None else n
    mx, nby = pm.max_len(mod, rate), pm.nbytes(mod, rate)
    pay = Rows(wce, n, mx + 3, payloads)
    out = Rows(wce, n, nby + 3)
    if scalar:
        ctx.psdu_frame(pay.addr, n, mod, rate, length=int(lengths[0]), seed=int(seeds[0]), bits=out.addr,
                       payload_stride=mx + 3, bits_stride=nby + 3)
    else:
        dl, ds = wce.DeviceArray.from_numpy(np.asarray(lengths, np.int32)), wce.DeviceArray.from_numpy(np.asarray(seeds, np.uint8))
        ctx.psdu_frame(pay.addr, n, mod, rate, lengths=dl, seeds=ds, bits=out.addr, payload_stride=mx + 3,
                       bits_stride=nby + 3)
    wce.synchronize()
    return out.get()


# ---------------------------------------------------------------- 1. framing
@pytest.mark.parametrize("mod,rate", pm.PAIRS)
def test_framing_parity(gpu_wce, ctx, mod, rate):
    wce = gpu_wce
    nby, T = pm.nbytes(mod, rate), pm.info_bits(mod, rate)
    payloads, lengths, seeds = _case(mod, rate)
    assert set(seeds) == set(range(1, 128)) and {4, 5, pm.max_len(mod, rate) - 1, pm.max_len(mod, rate)} <= set(lengths)
    want = pm.pack(pm.frame(payloads, seeds, mod, rate))
    assert want.shape == (B, nby)
    rows, guard = _frame_device(wce, ctx, mod, rate, payloads, lengths, seeds)
    assert np.array_equal(rows[:, :nby], want)
    assert np.all(rows[:, nby:] == SENT) and np.all(guard == SENT)
    if T % 8:                                                  # the unused high bits of the last byte are 0
        assert not np.any(rows[:, nby - 1] >> (T % 8))
    # the scalar form is the constant arrays'
    for L, sd in ((int(lengths[3]), 127), (4, 1), (5, 93)):
        pl = [np.random.default_rng(f).integers(0, 256, L - 4).astype(np.uint8) for f in range(13)]
        a, ga = _frame_device(wce, ctx, mod, rate, pl, [L] * 13, [sd] * 13, scalar=True)
        b, gb = _frame_device(wce, ctx, mod, rate, pl, [L] * 13, [sd] * 13)
        assert np.array_equal(a, b) and np.array_equal(a[:, :nby], pm.pack(pm.frame(pl, [sd] * 13, mod, rate)))
        assert np.all(ga == SENT) and np.all(gb == SENT)


def test_framing_without_a_payload_and_out_of_range_entries(gpu_wce, ctx):
    wce = gpu_wce
    mod, rate = 2, fm.RATE_3_4
    nby, mx = pm.nbytes(mod, rate), pm.max_len(mod, rate)
    out = Rows(wce, 9, nby + 3)
    ctx.psdu_frame(None, 9, mod, rate, length=4, seed=11, bits=out.addr, bits_stride=nby + 3)
    wce.synchronize()
    rows, guard = out.get()
    assert np.array_equal(rows[:, :nby], pm.pack(pm.frame([np.zeros(0, np.uint8)] * 9, [11] * 9, mod, rate)))
    assert np.all(rows[:, nby:] == SENT) and np.all(guard == SENT)
    # a length or a seed out of range: that frame's row is zeros, its neighbours are what they were
    payloads, lengths, seeds = _case(mod, rate, 29)
    good = pm.pack(pm.frame(payloads, seeds, mod, rate))
    lengths, seeds = lengths.copy(), seeds.copy()
    lengths[[2, 9]] = [3, mx + 1]
    lengths[[20, 21]] = [-5, 2 ** 31 - 1]
    seeds[[5, 13]] = [0, 128]
    rows, guard = _frame_device(wce, ctx, mod, rate, [p[:mx - 4] for p in payloads], lengths, seeds)
    bad = [2, 5, 9, 13, 20, 21]
    ok = np.setdiff1d(np.arange(29), bad)
    assert not rows[bad, :nby].any() and np.array_equal(rows[ok, :nby], good[ok])
    assert np.all(rows[:, nby:] == SENT) and np.all(guard == SENT)


# ---------------------------------------------------------------- 2. deframing
def _deframe_device(wce, ctx, mod, rate, rows, lengths, which=("psdu", "seed", "fcs_ok", "n_good"), scalar=False):
    """rows [n][nbytes] packed -> dict of what `which` names: psdu [n][max + 3] (sentinel where unwritten), seed,
    fcs_ok, n_good (started at 5), and "guard", the bytes around the PSDU rows"""
    n = len(rows)
    mx, nby = pm.max_len(mod, rate), pm.nbytes(mod, rate)
    inp = Rows(wce, n, nby + 3, rows)
    ps = Rows(wce, n, mx + 3)
    D = wce.DeviceArray.from_numpy
    d = {"seed": D(np.full(n, SENT, np.uint8)), "fcs_ok": D(np.full(n, 0xA5A5A5A5, np.uint32)),
         "n_good": D(np.array([5], np.uint32))}
    kw = {k: (ps.addr if k == "psdu" else d[k]) for k in which}
    if scalar:
        ctx.psdu_deframe(inp.addr, n, mod, rate, length=int(lengths[0]), bits_stride=nby + 3, psdu_stride=mx + 3, **kw)
    else:
        ctx.psdu_deframe(inp.addr, n, mod, rate, lengths=D(np.asarray(lengths, np.int32)), bits_stride=nby + 3,
                         psdu_stride=mx + 3, **kw)
    wce.synchronize()
    res = {k: d[k].numpy() for k in which if k != "psdu"}
    res["psdu"], res["guard"] = ps.get()
    assert np.array_equal(inp.d.numpy(), inp.host)            # the input is read only
    return res


def _check_deframe(got, rows, lengths, mod, rate, which=("psdu", "seed", "fcs_ok", "n_good")):
    T = pm.info_bits(mod, rate)
    psdu, seed, ok = pm.deframe(pm.unpack(rows, T), lengths, mod, rate)
    if "psdu" in which:
        for f, p in enumerate(psdu):
            n = 0 if p is None else p.size
            assert np.array_equal(got["psdu"][f, :n], p if n else np.zeros(0, np.uint8)), f
            assert np.all(got["psdu"][f, n:] == SENT), f
    else:
        assert np.all(got["psdu"] == SENT)
    assert np.all(got["guard"] == SENT)
    if "seed" in which:
        assert np.array_equal(got["seed"], seed)
    if "fcs_ok" in which:
        assert got["fcs_ok"].dtype == np.uint32 and np.array_equal(got["fcs_ok"], ok)
    if "n_good" in which:
        assert int(got["n_good"][0]) == 5 + int(ok.sum())
    return ok


def _damaged(mod, rate):
    """model-framed rows with one thing wrong each -> rows [n][nbytes], lengths, the expected flags by frame"""
    T, mx = pm.info_bits(mod, rate), pm.max_len(mod, rate)
    payloads, lengths, seeds = _case(mod, rate, B, seed=1)
    bits = pm.frame(payloads, seeds, mod, rate)
    lengths = lengths.copy()
    want = {}
    rng = np.random.default_rng(17)
    f = 8
    for t in range(16):                                        # SERVICE 0..6: another seed, bad; 7..15: still good
        bits[f, t] ^= 1
        want[f] = int(t >= 7)
        f += 1
    for where in ("first", "middle", "last", "fcs0", "fcs3", "tail", "tail5", "pad", "padlast"):
        L = int(lengths[f])
        t = {"first": 16 + int(rng.integers(0, 8)), "middle": 16 + 8 * ((L - 4) // 2) + int(rng.integers(0, 8)),
             "last": 16 + 8 * max(L - 5, 0) + int(rng.integers(0, 8)), "fcs0": 16 + 8 * (L - 4) + int(rng.integers(0, 8)),
             "fcs3": 16 + 8 * (L - 1) + 7, "tail": 16 + 8 * L, "tail5": 16 + 8 * L + 5, "pad": 16 + 8 * L + 6,
             "padlast": T - 1}[where]
        bits[f, t] ^= 1
        want[f] = int(where in ("tail", "tail5", "pad", "padlast"))
        f += 1
    bits[f] = 0                                                # an undetected packet's decode
    want[f] = 0
    f += 1
    for _ in range(6):                                         # random rows
        bits[f] = rng.integers(0, 2, T)
        want[f] = 0
        f += 1
    lengths[f], lengths[f + 2] = 3, mx + 1                     # lengths out of range, a good frame between them
    want[f] = want[f + 2] = 0
    return pm.pack(bits), lengths, want


@pytest.mark.parametrize("mod,rate", [(1, fm.RATE_1_2), (1, fm.RATE_3_4), (2, fm.RATE_2_3), (4, fm.RATE_1_2),
                                      (6, fm.RATE_1_2), (6, fm.RATE_3_4)])
def test_deframing_parity(gpu_wce, ctx, mod, rate):
    """T = 360, 540 (four unused bits in the last byte), 960, 1440, 2160 and 3240: 8, 16, 16, 32, 64 and 64 lanes
    a frame"""
    wce = gpu_wce
    T = pm.info_bits(mod, rate)
    payloads, lengths, seeds = _case(mod, rate)
    clean = pm.pack(pm.frame(payloads, seeds, mod, rate))
    got = _deframe_device(wce, ctx, mod, rate, clean, lengths)
    ok = _check_deframe(got, clean, lengths, mod, rate)
    assert ok.all() and np.array_equal(got["seed"], seeds)
    for f, p in enumerate(payloads):
        assert np.array_equal(got["psdu"][f, :p.size + 4], pm.psdu_of(p))
    rows, lens, want = _damaged(mod, rate)
    got = _deframe_device(wce, ctx, mod, rate, rows, lens)
    ok = _check_deframe(got, rows, lens, mod, rate)
    for f, w in want.items():
        assert ok[f] == w, (f, w)
    assert ok[[f for f in range(B) if f not in want]].all()    # the neighbours are unaffected
    zero = [f for f in range(B) if not rows[f].any()][0]
    assert got["seed"][zero] == 0 and not got["psdu"][zero, :lens[zero]].any()
    # each output alone gives what all together give
    for k in ("psdu", "seed", "fcs_ok", "n_good"):
        one = _deframe_device(wce, ctx, mod, rate, rows, lens, which=(k,))
        _check_deframe(one, rows, lens, mod, rate, which=(k,))
        assert np.array_equal(one[k], got[k]) if k != "psdu" else np.array_equal(one["psdu"], got["psdu"])
    # the scalar length is the constant array
    L = int(lengths[3])
    same = [pm.pack(pm.frame_one(np.random.default_rng(f).integers(0, 256, L - 4).astype(np.uint8), int(seeds[f]), T))
            for f in range(9)]
    same[1][5] ^= 0x10
    a = _deframe_device(wce, ctx, mod, rate, same, [L] * len(same), scalar=True)
    b = _deframe_device(wce, ctx, mod, rate, same, [L] * len(same))
    _check_deframe(a, np.stack(same), [L] * len(same), mod, rate)
    assert all(np.array_equal(a[k], b[k]) for k in a) and a["fcs_ok"][1] == 0 and a["fcs_ok"].sum() == len(same) - 1


# ---------------------------------------------------------------- 3. through the existing coder
@pytest.mark.parametrize("mod,rate", [(1, fm.RATE_1_2), (4, fm.RATE_3_4), (6, fm.RATE_2_3)])
def test_through_the_coder(gpu_wce, ctx, mod, rate):
    """psdu_frame -> reencode -> a noiseless h = 1 channel -> demodulate -> soft_demap -> viterbi_decode, unterminated
    -> psdu_deframe: the byte and bit orders against the calls on either side"""
    wce, n = gpu_wce, 67
    Z = lambda shape, dt=np.complex128: wce.DeviceArray(shape, dt, zero=True)
    D = wce.DeviceArray.from_numpy
    nby, mx, T = pm.nbytes(mod, rate), pm.max_len(mod, rate), pm.info_bits(mod, rate)
    payloads, lengths, seeds = _case(mod, rate, n, seed=2)
    pay = np.zeros((n, mx - 4), np.uint8)
    for f, p in enumerate(payloads):
        pay[f, :p.size] = p
    dlen, dbits, dtx = D(lengths), Z((n, nby), np.uint8), Z((n, 15, 53))
    ctx.psdu_frame(D(pay), n, mod, rate, lengths=dlen, seeds=D(seeds), bits=dbits)
    ctx.reencode(dbits, n, mod, rate, tx=dtx)
    h = np.ones((n, 53), np.complex128)
    dh, deq, dllr, ddec = D(h), Z((n, 15, 53)), Z((n, 15, 48 * mod), np.float32), Z((n, nby), np.uint8)
    ctx.demodulate(ctx.frames(dtx, dtx, n), dh, None, 53, mod, eq=deq)
    ctx.soft_demap(deq, dh, n, None, 53, mod, llr=dllr)
    ctx.viterbi_decode(dllr, n, mod, rate, False, ddec)
    out = {"psdu": Z((n, mx), np.uint8), "seed": Z((n,), np.uint8), "fcs_ok": Z((n,), np.uint32), "n_good": Z((1,), np.uint32)}
    ctx.psdu_deframe(ddec, n, mod, rate, lengths=dlen, **out)
    wce.synchronize()
    framed = pm.unpack(dbits.numpy(), T)
    assert np.array_equal(framed, pm.frame(payloads, seeds, mod, rate))
    assert np.array_equal(pm.unpack(ddec.numpy(), T)[:, :16 + 8 * 4], framed[:, :16 + 8 * 4])
    assert np.all(out["fcs_ok"].numpy() == 1) and int(out["n_good"].numpy()[0]) == n
    assert np.array_equal(out["seed"].numpy(), seeds)
    psdu = out["psdu"].numpy()
    for f, p in enumerate(payloads):
        assert np.array_equal(psdu[f, :p.size + 4], pm.psdu_of(p)) and not psdu[f, p.size + 4:].any(), f


# ---------------------------------------------------------------- 4. the frame loop and big indices
@pytest.mark.parametrize("n", (67, 13))
@pytest.mark.parametrize("mod,rate", [(1, fm.RATE_1_2), (2, fm.RATE_3_4), (4, fm.RATE_3_4), (6, fm.RATE_3_4)])
def test_frame_loop(gpu_wce, ctx, mod, rate, n):
    """three workgroups of four waves: at 8, 4, 2 and 1 frames a wave a sweep is 96, 48, 24 and 12 frames, so 67
    frames are a ragged first sweep or up to five and a ragged one, 13 one group and a bit.  Long and short, good and
    bad frames alternate: a CRC, phase or length left over from the frame before would show"""
    wce, lib = gpu_wce, gpu_wce.load()
    T, mx = pm.info_bits(mod, rate), pm.max_len(mod, rate)
    rng = np.random.default_rng(n)
    lengths = np.where(np.arange(n) % 2 == 0, mx - rng.integers(0, 3, n), 4 + rng.integers(0, 4, n)).astype(np.int32)
    seeds = rng.integers(1, 128, n).astype(np.uint8)
    payloads = [rng.integers(0, 256, int(L) - 4).astype(np.uint8) for L in lengths]
    want = pm.pack(pm.frame(payloads, seeds, mod, rate))
    rx = want.copy()
    for f in range(1, n, 3):                                   # every third frame bad, in its PSDU
        rx[f, 2 + int(rng.integers(0, lengths[f]))] ^= 1 << int(rng.integers(0, 8))
    runs = []
    try:
        for v in (0, 1):
            assert lib.wce_debug_set_variant(GRID, v) == 0
            rows, guard = _frame_device(wce, ctx, mod, rate, payloads, lengths, seeds)
            runs.append((rows, guard, _deframe_device(wce, ctx, mod, rate, rx, lengths)))
    finally:
        assert lib.wce_debug_set_variant(GRID, 0) == 0
    (r0, g0, d0), (r1, g1, d1) = runs
    assert np.array_equal(r0, r1) and np.array_equal(g0, g1) and all(np.array_equal(d0[k], d1[k]) for k in d0)
    assert np.array_equal(r1[:, :want.shape[1]], want) and np.all(r1[:, want.shape[1]:] == SENT) and np.all(g1 == SENT)
    ok = _check_deframe(d1, rx, lengths, mod, rate)
    assert np.array_equal(ok == 0, np.arange(n) % 3 == 1)


def test_big_indices(gpu_wce, ctx):
    """five frames a 2^30 + 1 bytes apart in every buffer: the last lies beyond 2^32 bytes.  Sparse: only the rows are
    touched; skipped when the device refuses 3 x 4 GB"""
    wce, lib = gpu_wce, gpu_wce.load()
    mod, rate, n, S = 4, fm.RATE_1_2, 5, (1 << 30) + 1
    nby, mx, T = pm.nbytes(mod, rate), pm.max_len(mod, rate), pm.info_bits(mod, rate)
    assert (n - 1) * S > 2 ** 32
    payloads, lengths, seeds = _case(mod, rate, n, seed=4)
    lengths[:] = [mx, 4, mx - 1, 9, mx]
    payloads = [np.random.default_rng(f).integers(0, 256, int(L) - 4).astype(np.uint8) for f, L in enumerate(lengths)]
    try:
        big = [wce.DeviceArray(((n - 1) * S + 4096,), np.uint8) for _ in range(3)]
    except wce.WceError:
        pytest.skip("the device refuses three buffers of 4 GB")
    bpay, bbits, bpsdu = big
    D = wce.DeviceArray.from_numpy
    try:
        for f, p in enumerate(payloads):
            assert lib.wce_memset(bbits.addr + f * S, SENT, nby + 64) == 0 and lib.wce_memset(bpsdu.addr + f * S, SENT, mx + 64) == 0
            if p.size:
                assert lib.wce_memcpy_htod(bpay.addr + f * S, np.ascontiguousarray(p).ctypes.data, p.size) == 0
        dlen, dseeds = D(lengths), D(seeds)
        ctx.psdu_frame(bpay, n, mod, rate, lengths=dlen, seeds=dseeds, bits=bbits, payload_stride=S, bits_stride=S)
        out = {"seed": D(np.zeros(n, np.uint8)), "fcs_ok": D(np.zeros(n, np.uint32)), "n_good": D(np.zeros(1, np.uint32))}
        ctx.psdu_deframe(bbits, n, mod, rate, lengths=dlen, psdu=bpsdu, bits_stride=S, psdu_stride=S, **out)
        wce.synchronize()
        want = pm.pack(pm.frame(payloads, seeds, mod, rate))
        for f, p in enumerate(payloads):
            row, ps = np.empty(nby + 64, np.uint8), np.empty(mx + 64, np.uint8)
            assert lib.wce_memcpy_dtoh(row.ctypes.data, bbits.addr + f * S, row.size) == 0
            assert lib.wce_memcpy_dtoh(ps.ctypes.data, bpsdu.addr + f * S, ps.size) == 0
            assert np.array_equal(row[:nby], want[f]) and np.all(row[nby:] == SENT), f
            assert np.array_equal(ps[:p.size + 4], pm.psdu_of(p)) and np.all(ps[p.size + 4:] == SENT), f
        assert np.all(out["fcs_ok"].numpy() == 1) and int(out["n_good"].numpy()[0]) == n
        assert np.array_equal(out["seed"].numpy(), seeds)
    finally:
        wce.synchronize()
        for b in big:
            b.free()


# ---------------------------------------------------------------- 5. the link
@pytest.fixture(scope="module")
def link_ctx(gpu_wce):
    pre = tm.chain_pre()
    return gpu_wce.Context(pre, pre, 1e-6, gpu_wce.MMSE_TEXTBOOK)


def _link(wce, link_ctx, snr, **kw):
    c = pm.link_set()
    res = link_ctx.link_host(pm.LINK_MOD, pm.LINK_RATE, snr, pm.LINK_B, psdu_len=c["L"], taps=c["taps"],
                             capture_len=pm.LINK_LEN, threshold=pm.LINK_THRESHOLD, seed=pm.LINK_SEED, **kw)
    assert np.array_equal(res["payload"], c["payload"]) and np.array_equal(res["seeds"], c["seeds"])
    assert np.array_equal(res["bits"], c["bits"])              # the device framed what the model frames
    return c, res


def test_link_at_30_db(gpu_wce, link_ctx):
    wce = gpu_wce
    c, res = _link(wce, link_ctx, pm.LINK_SNR_HIGH, tracker=(0.5, 2))
    sent = np.stack([pm.psdu_of(p) for p in c["payload"]])
    for s in (wce.LT_LS, wce.PS_LINEAR, wce.PS_MMSE):
        print(f"source {s}: good {int(res['fcs_ok'][s].sum())} of {pm.LINK_B}, bit errors {int(res[s].sum())}, "
              f"tracked good {int(res['tracked_fcs_ok'][s].sum())}")
        assert res["fcs_ok"][s].dtype == np.uint32 and np.all(res["fcs_ok"][s] == 1), s
        assert np.all(res[s] == 0), s
        assert res["psdu_rx"][s].shape == (pm.LINK_B, c["L"]) and np.array_equal(res["psdu_rx"][s], sent), s
        assert np.array_equal(res["psdu_rx"][s][:, :-4], res["payload"]) and np.array_equal(res["seed_rx"][s], c["seeds"])
        assert res["tracked_fcs_ok"][s].shape == (pm.LINK_B,)


def test_link_at_a_low_snr(gpu_wce, link_ctx):
    """LINK_SNR_LOW was chosen on the numpy chain (tests/test_psdu_abi.py: 33 good, 34 bad there)"""
    wce = gpu_wce
    c, res = _link(wce, link_ctx, pm.LINK_SNR_LOW, dd_iterations=1)
    T = pm.info_bits(pm.LINK_MOD, pm.LINK_RATE)
    sent = np.stack([pm.psdu_of(p) for p in c["payload"]])
    ok = res["fcs_ok"][wce.LT_LS]
    # the condition holds without the decision-directed round too, on LT_LS's own first decode
    plain = _link(wce, link_ctx, pm.LINK_SNR_LOW, sources=(wce.LT_LS,))[1]
    print(f"LT_LS: good {int(plain['fcs_ok'][wce.LT_LS].sum())}, bad {pm.LINK_B - int(plain['fcs_ok'][wce.LT_LS].sum())}; "
          f"after one decision-directed round good {int(ok.sum())}")
    assert 5 <= int(plain["fcs_ok"][wce.LT_LS].sum()) <= pm.LINK_B - 5
    for r, sources in ((plain, (wce.LT_LS,)), (res, (wce.LT_LS, wce.PS_LINEAR, wce.PS_MMSE))):
        for s in sources:
            right = np.all(r["psdu_rx"][s] == sent, axis=1) & (r["seed_rx"][s] == c["seeds"])
            assert np.array_equal(r["fcs_ok"][s] == 1, right), s
            psdu, seed, mok = pm.deframe(r["bits_rx"][s], np.full(pm.LINK_B, c["L"]), pm.LINK_MOD, pm.LINK_RATE)
            assert np.array_equal(r["fcs_ok"][s], mok) and np.array_equal(r["seed_rx"][s], seed), s
            assert np.array_equal(r["psdu_rx"][s], np.stack(psdu)), s
            assert np.array_equal(r[s], np.sum(r["bits_rx"][s] != c["bits"], axis=1)), s      # nbiterr against the framed bits
            assert np.all(r[s][r["fcs_ok"][s] == 0] > 0)


def test_link_mrc_with_psdus(gpu_wce, link_ctx):
    wce = gpu_wce
    c = pm.link_set()
    import fading_model as fd
    taps = np.stack([c["taps"], fd.pdp_taps(np.random.default_rng(pm.LINK_TAPS_SEED + 1), pm.LINK_B, pm.LINK_POWER)])
    res = link_ctx.link_mrc_host(pm.LINK_MOD, pm.LINK_RATE, pm.LINK_SNR_LOW, pm.LINK_B, 2, taps, sources=(wce.LT_LS,),
                                 capture_len=pm.LINK_LEN, threshold=pm.LINK_THRESHOLD, seed=pm.LINK_SEED, psdu_len=c["L"])
    assert np.array_equal(res["payload"], c["payload"]) and np.array_equal(res["bits"], c["bits"])
    f = res["fcs_ok"][wce.LT_LS]
    n = res[wce.LT_LS]
    print(f"good packets: combined {int(f['combined'].sum())}, branches {f['branch'].sum(axis=1)}")
    assert f["combined"].shape == (pm.LINK_B,) and f["branch"].shape == (2, pm.LINK_B)
    assert f["combined"].sum() >= f["branch"].sum(axis=1).max()         # two antennas lose no more than the better one
    assert np.all(n["combined"][f["combined"] == 0] > 0) and np.all(n["branch"][f["branch"] == 0] > 0)
    sent = np.stack([pm.psdu_of(p) for p in c["payload"]])
    good = f["combined"] == 1
    assert np.array_equal(res["psdu_rx"][wce.LT_LS][good], sent[good])
