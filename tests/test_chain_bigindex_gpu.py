"""Element indices past 2^31 in the receive and transmit chain, as tests/test_bigindex_gpu.py has them
for the estimators: 600 frames whose buffers are laid out with a frame stride of 2^22 complex elements
(frame 599 starts at element 2.5e9, 40 GB in) or 2^23 floats / bytes (past 2^32 elements), and with block
strides of 2^16 (2^18 for the soft bits) inside a frame's slot.  Every chain call must index in 64 bits:
its outputs must equal those of the same frames packed densely, bit for bit, since a frame's outputs
depend on its own data alone.  Every stride argument of a call is large in its strided run: frame and block
strides, h_stride, the h_blocks and h_last strides, pre_stride, the taps' stride, bits_stride, ref_stride,
and the packet, field, wave and capture strides.

Three groups, each with its own big buffers, freed before the next: the front end and sync (two of 40 GB),
the receive chain behind the estimate (two of 40 GB, soft bits 20 GB, bytes 5 GB), the transmitter (three of
40 GB: the peak, 121 GB of device memory).  The time is the allocations' and the per-frame copies'."""
import numpy as np
import pytest

import cfo_model as cm
import demod_model as dm
import fec_model as fm
import tx_model as tm

pytestmark = pytest.mark.gpu

N, NBLK = dm.N, dm.NBLK
B = 600
S = 1 << 22             # frame stride of complex buffers, elements (64 MB)
SF = 1 << 23            # frame stride of float and uint8 buffers, elements
BS = 1 << 16            # block stride inside a complex slot: 15 blocks take 2^20 elements
LBS = 1 << 18           # block stride of the soft bits
# where a complex slot keeps what: four regions of 15 block rows, and 53-element rows in the gaps behind block 0's
R0, R1, R2, R3 = 0, 1 << 20, 1 << 21, 3 << 20
ROW_A, ROW_B, ROW_C = 64, 128, 192


class Slots:
    """a device buffer of B slots of `stride` elements"""

    def __init__(self, wce, dtype, stride):
        self.wce, self.lib = wce, wce.load()
        self.dtype, self.item, self.stride = np.dtype(dtype), np.dtype(dtype).itemsize, stride
        assert (B - 1) * stride > 2 ** 31
        self.d = wce.DeviceArray((B * stride,), dtype)

    def at(self, off=0):
        return self.d.addr + off * self.item

    def _copy(self, dense, off, bs, out):
        shape = dense.shape
        nb, row = (1, shape[1]) if len(shape) == 2 else (shape[1], shape[2])
        if bs is None or nb == 1:
            nb, row, bs = 1, nb * row, 0
        assert shape[0] == B and off + (nb - 1) * bs + row <= self.stride
        for f in range(B):
            for b in range(nb):
                big = self.at(f * self.stride + off + b * bs)
                small = dense.addr + (f * nb + b) * row * self.item
                dst, src = (small, big) if out else (big, small)
                assert self.lib.wce_memcpy_dtod(dst, src, row * self.item, None) == 0

    def put(self, dense, off=0, bs=None):
        """dense DeviceArray [B][row] or [B][nb][row] -> slot f at off (+ b * bs)"""
        assert dense.dtype == self.dtype
        self._copy(dense, off, bs, False)

    def get(self, shape, off=0, bs=None):
        """the same places -> a host array of `shape`"""
        dense = self.wce.DeviceArray(shape, self.dtype, zero=True)
        self._copy(dense, off, bs, True)
        self.wce.synchronize()
        return dense.numpy()

    def free(self):
        self.wce.synchronize()
        self.d.free()


def _same(got, want, what):
    for k in want:
        g, w = np.ascontiguousarray(got[k]), np.ascontiguousarray(want[k])
        assert g.shape == w.shape and g.dtype == w.dtype, (what, k)
        assert np.array_equal(g.view(np.uint8), w.view(np.uint8)), f"{what}: {k} differs with the big strides"
    assert any(np.any(np.ascontiguousarray(w).view(np.uint8)) for w in want.values()), what


@pytest.fixture(scope="module")
def ctx(gpu_wce):
    return gpu_wce.Context(empty=True)     # the ctx only selects the device


# ---------------------------------------------------------------- 1. front end and sync
def test_front_end_and_sync(gpu_wce, ctx):
    wce = gpu_wce
    D, Z = wce.DeviceArray.from_numpy, lambda shape, dt=np.complex128: wce.DeviceArray(shape, dt, zero=True)
    W, off = 1500, 7
    rng = np.random.default_rng(0xB161)
    cap = cm.random_packets(rng, B, W)
    field = np.tile(np.fft.ifft(rng.choice([-1.0, 1.0], 64)), 2)
    for f in range(B):                                       # a field somewhere in every window: sync finds it
        p = int(rng.integers(0, W - 128 - off - NBLK * 80))
        cap[f, p:p + 128] += field
    eps = cm.draw_eps(rng, B)
    start = rng.integers(0, W - 128 - off - NBLK * 80 + 1, B).astype(np.int32)
    start[17], start[599] = -1, W                             # no start, and one outside the window: NaN rows
    dcap, dltf, dcfo, dstart = D(cap), D(field[:64].copy()), D(eps), D(start)
    bigin, bigout = Slots(wce, np.complex128, S), Slots(wce, np.complex128, S)
    try:
        bigin.put(dcap)

        def blocks(kw):
            dsym = Z((B, NBLK, N))
            ctx.front_end_blocks(dcap, B, NBLK, dsym, packet_stride=W, **kw)
            ctx.front_end_blocks(bigin.at(), B, NBLK, bigout.at(R1), packet_stride=S, frame_stride=S, block_stride=BS,
                                 **kw)
            wce.synchronize()
            return {"sym": dsym.numpy()}, {"sym": bigout.get((B, NBLK, N), R1, BS)}

        for what, kw in (("blocks", {}), ("blocks_cfo", dict(cfo=dcfo, sample_offset=off)),
                         ("blocks_at", dict(cfo=dcfo, sample_offset=off, start=dstart, capture_len=W))):
            want, got = blocks(kw)
            _same(got, want, what)
        assert np.isnan(want["sym"][[17, 599]].view(np.float64)).all() and np.isfinite(want["sym"][:17]).all()

        def preamble(kw, est):
            outs = []
            for big in (False, True):
                dpre, dow2 = Z((B, N)), Z((B,), np.float64)
                de = Z((B,), np.float64) if est else None
                ckw = dict(kw, cfo=de, estimate_cfo=True) if est else kw
                if big:
                    ctx.front_end_preamble(bigin.at(), B, W if "start" in kw else 160, bigout.at(ROW_A), dow2,
                                           lptot_stride=S, pre_stride=S, **ckw)
                else:
                    ctx.front_end_preamble(dcap, B, W if "start" in kw else 160, dpre, dow2, lptot_stride=W, **ckw)
                wce.synchronize()
                o = {"pre": bigout.get((B, N), ROW_A) if big else dpre.numpy(), "ow2": dow2.numpy()}
                if est:
                    o["cfo"] = de.numpy()
                outs.append(o)
            return outs

        for what, kw, est in (("preamble", {}, False), ("preamble_cfo given", dict(cfo=dcfo, estimate_cfo=False), False),
                              ("preamble_cfo estimated", {}, True),
                              ("preamble_at", dict(start=dstart, capture_len=W), True)):
            want, got = preamble(kw, est)
            _same(got, want, what)

        outs = []
        for big in (False, True):
            ds, dm_ = D(np.full(B, -77, np.int32)), D(np.full(B, 9.0))
            ctx.front_end_sync(bigin.at() if big else dcap, B, W, dltf, 0.25, 0, ds, dm_, capture_stride=S if big else W)
            wce.synchronize()
            outs.append({"start": ds.numpy(), "metric": dm_.numpy()})
        _same(outs[1], outs[0], "sync")
        assert np.count_nonzero(outs[0]["start"] >= 0) > B // 2
    finally:
        bigin.free()
        bigout.free()


# ---------------------------------------------------------------- 2. the receive chain behind the estimate
def test_receive_chain(gpu_wce, ctx):
    wce = gpu_wce
    D, Z = wce.DeviceArray.from_numpy, lambda shape, dt=np.complex128: wce.DeviceArray(shape, dt, zero=True)
    mod, rate = dm.QAM16, fm.RATE_1_2
    T = fm.info_bits(mod, rate)
    nby = (T + 7) // 8
    s = fm.clean_set(mod, rate)
    idx = np.arange(B) % 67                                   # the 67-frame set, tiled
    tx, rx, h, h_lt, u = (np.ascontiguousarray(s[k][idx]) for k in ("tx", "rx", "h", "h_lt", "u"))
    h = h * (1.0 + 1e-6 * np.arange(B))[:, None]              # no two frames alike
    dtx, drx, dh, dhl = D(tx), D(rx), D(h), D(h_lt)
    dref = D(fm.pack(u))
    bigin, bigout = Slots(wce, np.complex128, S), Slots(wce, np.complex128, S)
    bigf, big8 = Slots(wce, np.float32, SF), Slots(wce, np.uint8, SF)
    try:
        bigin.put(dtx, R0, BS)
        bigin.put(drx, R1, BS)
        bigin.put(dh, ROW_A)
        bigin.put(dhl, ROW_B)
        dense_fr = ctx.frames(dtx, drx, B)
        big_fr = ctx.frames(bigin.at(R0), bigin.at(R1), B, frame_stride=S, block_stride=BS)

        # demodulate: the build with the frame's sums, and the capped one without
        def small_outs(names):
            mk = {"theta": lambda: Z((B, NBLK), np.float64), "evm": lambda: Z((B,), np.float64),
                  "nerr": lambda: Z((B,), np.uint32)}
            return {k: mk[k]() for k in names}

        dense_eq = None
        for names in (("theta", "evm", "nerr"), ("theta",)):
            so = small_outs(names)
            deq, dsym = Z((B, NBLK, N)), Z((B, NBLK, N), np.uint8)
            ctx.demodulate(dense_fr, dh, dhl, N, mod, eq=deq, sym=dsym, **so)
            wce.synchronize()
            want = dict({k: a.numpy() for k, a in so.items()}, eq=deq.numpy(), sym=dsym.numpy())
            so = small_outs(names)
            ctx.demodulate(big_fr, bigin.at(ROW_A), bigin.at(ROW_B), S, mod, eq=bigout.at(R0), sym=big8.at(),
                           eq_frame_stride=S, eq_block_stride=BS, sym_frame_stride=SF, sym_block_stride=LBS, **so)
            wce.synchronize()
            got = dict({k: a.numpy() for k, a in so.items()}, eq=bigout.get((B, NBLK, N), R0, BS),
                       sym=big8.get((B, NBLK, N), 0, LBS))
            _same(got, want, f"demodulate {names}")
            dense_eq = deq

        # track_demodulate
        so = small_outs(("theta", "evm", "nerr"))
        deq, dsym, dhb, dhlast = Z((B, NBLK, N)), Z((B, NBLK, N), np.uint8), Z((B, NBLK, N)), Z((B, N))
        ctx.track_demodulate(dense_fr, dh, 0.5, 2, N, mod, eq=deq, sym=dsym, h_blocks=dhb, h_last=dhlast, **so)
        wce.synchronize()
        want = dict({k: a.numpy() for k, a in so.items()}, eq=deq.numpy(), sym=dsym.numpy(), h_blocks=dhb.numpy(),
                    h_last=dhlast.numpy())
        so = small_outs(("theta", "evm", "nerr"))
        ctx.track_demodulate(big_fr, bigin.at(ROW_A), 0.5, 2, S, mod, eq=bigout.at(R0), sym=big8.at(),
                             h_blocks=bigout.at(R2), h_last=bigout.at(ROW_C), eq_frame_stride=S, eq_block_stride=BS,
                             sym_frame_stride=SF, sym_block_stride=LBS, hb_frame_stride=S, hb_block_stride=BS,
                             h_last_stride=S, **so)
        wce.synchronize()
        got = dict({k: a.numpy() for k, a in so.items()}, eq=bigout.get((B, NBLK, N), R0, BS),
                   sym=big8.get((B, NBLK, N), 0, LBS), h_blocks=bigout.get((B, NBLK, N), R2, BS),
                   h_last=bigout.get((B, N), ROW_C))
        _same(got, want, "track_demodulate")

        # soft_demap on demodulate's eq; soft_demap_blocks on the tracker's eq and h_blocks
        bigin.put(dense_eq, R2, BS)
        dllr = Z((B, NBLK, 48 * mod), np.float32)
        ctx.soft_demap(dense_eq, dh, B, dhl, N, mod, llr=dllr)
        ctx.soft_demap(bigin.at(R2), bigin.at(ROW_A), B, bigin.at(ROW_B), S, mod, llr=bigf.at(), eq_frame_stride=S,
                       eq_block_stride=BS, llr_frame_stride=SF, llr_block_stride=LBS)
        wce.synchronize()
        _same({"llr": bigf.get((B, NBLK, 48 * mod), 0, LBS)}, {"llr": dllr.numpy()}, "soft_demap")
        bigin.put(deq, R2, BS)
        bigin.put(dhb, R3, BS)
        dllr_b = Z((B, NBLK, 48 * mod), np.float32)
        ctx.soft_demap_blocks(deq, dhb, B, mod, llr=dllr_b)
        ctx.soft_demap_blocks(bigin.at(R2), bigin.at(R3), B, mod, llr=bigf.at(), eq_frame_stride=S, eq_block_stride=BS,
                              hb_frame_stride=S, hb_block_stride=BS, llr_frame_stride=SF, llr_block_stride=LBS)
        wce.synchronize()
        _same({"llr": bigf.get((B, NBLK, 48 * mod), 0, LBS)}, {"llr": dllr_b.numpy()}, "soft_demap_blocks")

        # viterbi_decode on soft_demap's bits; the reference bits in the byte slots' upper half
        bigf.put(dllr, 0, LBS)
        big8.put(dref, SF // 2)
        dbits, dn = Z((B, nby), np.uint8), Z((B,), np.uint32)
        ctx.viterbi_decode(dllr, B, mod, rate, bits=dbits, ref_bits=dref, nbiterr=dn)
        dn2 = Z((B,), np.uint32)
        ctx.viterbi_decode(bigf.at(), B, mod, rate, bits=big8.at(), bits_stride=SF, ref_bits=big8.at(SF // 2),
                           ref_stride=SF, nbiterr=dn2, llr_frame_stride=SF, llr_block_stride=LBS)
        wce.synchronize()
        want = {"bits": dbits.numpy(), "nbiterr": dn.numpy()}
        _same({"bits": big8.get((B, nby), 0), "nbiterr": dn2.numpy()}, want, "viterbi_decode")
        assert np.array_equal(want["bits"], fm.pack(u))          # the clean set decodes

        # reencode from the reference bits: x^ and H_dd, the frames' own pilots, theta of the demodulator
        dth = Z((B, NBLK), np.float64)
        ctx.demodulate(dense_fr, dh, dhl, N, mod, theta=dth)
        dx, dhd = Z((B, NBLK, N)), Z((B, N))
        ctx.reencode(dref, B, mod, rate, theta=dth, frames=dense_fr, tx=dx, h=dhd)
        ctx.reencode(big8.at(SF // 2), B, mod, rate, bits_stride=SF, theta=dth, frames=big_fr, tx=bigout.at(R0),
                     tx_frame_stride=S, tx_block_stride=BS, h=bigout.at(ROW_A), h_stride=S)
        wce.synchronize()
        _same({"tx": bigout.get((B, NBLK, N), R0, BS), "h": bigout.get((B, N), ROW_A)},
              {"tx": dx.numpy(), "h": dhd.numpy()}, "reencode")
    finally:
        for big in (bigin, bigout, bigf, big8):
            big.free()


# ---------------------------------------------------------------- 3. the transmitter
def test_transmitter(gpu_wce, ctx):
    wce = gpu_wce
    D, Z = wce.DeviceArray.from_numpy, lambda shape, dt=np.complex128: wce.DeviceArray(shape, dt, zero=True)
    rng = np.random.default_rng(0xB163)
    mod, rate = dm.QAM16, fm.RATE_1_2
    sym = np.ascontiguousarray(fm.clean_set(mod, rate)["tx"][np.arange(B) % 67])
    pre, taps = tm.preambles(rng, B), tm.random_taps(rng, B, 16)
    S_wave, L = 160 + 80 * NBLK, 1488
    dsym, dpre, dtaps = D(sym), D(pre), D(taps)
    chan = dict(n_taps=16, cfo=D(rng.uniform(-0.002, 0.002, B)), ow2=D(rng.uniform(0.5, 2.0, B) * 1e-4),
                delay=D(rng.integers(-20, 60, B).astype(np.int32)), seed=tm.SEED, first_frame=11)
    bigin, bigwave, bigcap = (Slots(wce, np.complex128, S) for _ in range(3))
    try:
        bigin.put(dsym, R0, BS)
        bigin.put(dpre, ROW_A)
        bigin.put(dtaps, ROW_B)
        dwave, dcap, dcap2 = Z((B, S_wave)), Z((B, L)), Z((B, L))
        ctx.modulate(dsym, B, dwave, NBLK, dpre, N)
        ctx.modulate(bigin.at(R0), B, bigwave.at(), NBLK, bigin.at(ROW_A), S, frame_stride=S, block_stride=BS,
                     wave_stride=S)
        wce.synchronize()
        _same({"wave": bigwave.get((B, S_wave))}, {"wave": dwave.numpy()}, "modulate")
        ctx.channel(dwave, B, S_wave, dcap, L, taps=dtaps, taps_stride=16, field=True, **chan)
        ctx.channel(bigwave.at(), B, S_wave, bigcap.at(), L, taps=bigin.at(ROW_B), taps_stride=S, field=True,
                    wave_stride=S, capture_stride=S, **chan)
        wce.synchronize()
        want = dcap.numpy()
        _same({"capture": bigcap.get((B, L))}, {"capture": want}, "channel")
        ctx.transmit(dsym, B, dcap2, L, NBLK, dpre, N, taps=dtaps, taps_stride=16, **chan)
        ctx.transmit(bigin.at(R0), B, bigcap.at(), L, NBLK, bigin.at(ROW_A), S, frame_stride=S, block_stride=BS,
                     taps=bigin.at(ROW_B), taps_stride=S, capture_stride=S, **chan)
        wce.synchronize()
        _same({"capture": bigcap.get((B, L))}, {"capture": dcap2.numpy()}, "transmit")
        assert np.array_equal(dcap2.numpy().view(np.uint8), want.view(np.uint8))     # the fused call is the pair
    finally:
        for big in (bigin, bigwave, bigcap):
            big.free()
