"""Every stream-taking call of the library on a stream the caller made (include/wce.h "Threading").

The chain calls promise to be asynchronous on `stream`, to read nothing back and to allocate nothing.  Every other
GPU test passes stream=None, where a launcher that dropped its stream argument, a wrapper that forgot to forward it,
a validation path that reads device memory or a synchronous memset would change nothing.  Here two scripted links,
lists of (name, call(stream), buffers written) in which each call reads what an earlier one wrote, between them
make every entry point whose prototype ends in a stream argument:

  link P, one antenna:  psdu_frame, reencode, modulate, transmit, front_end_sync, the _at front end with its own
    offset estimate, estimate_noise, demodulate, soft_demap, viterbi_decode, a decision-directed round (reencode
    with theta, demodulate, soft_demap, viterbi_decode), psdu_deframe, nonfinite_scan; beside it the unfused
    modulate and channel feeding the plain and _cfo front end, synth feeding mmse_solve / mmse_apply and a plan,
    the long double conversions, the device copy and the pinned copies in and out;
  link Q, two antennas, short field, fading:  short_field, modulate, channel_tv per antenna, transmit_tv feeding
    a front_end_sync of its own, front_end_sync_stf, sync_share, the _at front end with the given offset, estimate,
    combine, track_demodulate, soft_demap_blocks, viterbi_decode, psdu_deframe.

16-QAM rate 1/2, the suite's batches of 67 and 13 frames.  Every buffer is allocated and filled with the suite's
sentinels (7 - 3j, 9.0, 0xDEAD, 0xA5; NaN where the consumer flags it) before the first asynchronous call.  The
reference is the same list on the null stream with a synchronise after every step; tests/chain_streams_model.py
says on the CPU which packets it must find good.

1. test_every_call_is_ordered_behind_a_held_stream: one of the library's own kernels, a 64-QAM 3/4 Viterbi decode
   of all-zero soft bits on three workgroups, holds the stream; an event is recorded behind it; every step is
   enqueued; the event must still be pending (no call waited, allocated or read back), and after the synchronise
   every buffer must hold the reference's bytes, compared in step order, so that the first buffer that differs
   names the call that ran early: a call that escaped to another stream reads sentinels while the blocker holds
   its producer.  A recording wrapper around the library asserts that every stream-taking entry point of
   include/wce.h and wce.py's prototype table was called with that stream.
   Measured on an MI355X with events and the host clock: enqueueing link P's 32 steps on an idle stream takes the
   host 0.24 to 0.51 ms over five runs (link Q's 19 steps 0.18 to 0.49 ms), and the blocker runs for 7.8 ms at 150
   frames, 15.5 ms at 300, 31.8 ms at 600 and 64.0 ms at 1,200: the 600 frames used here hold the stream for 62
   times the slowest enqueue measured, where 20 times was asked for.
   The first run of this test found a call that waited: wce_estimate_noise took 31.9 ms to return behind the 32 ms
   blocker.  The context had wce_ctx_reserve(150) behind it and the stream wce_ctx_reserve_stream(67); the
   latter ignored the former's size, wce_estimate then applied it to the scratch that existed, and growing scratch
   drains the stream.  csrc/wce_api.cpp now gives new scratch the larger of the two sizes in both places and never
   re-sizes existing scratch to wce_ctx_reserve's, as include/wce.h words it; link P takes 0.48 ms to enqueue behind
   the blocker since.  The fixture keeps the two reservations in that order.
2. test_streams_that_overlap_give_the_serial_bytes: under WCE_VARIANT_GRID every looping kernel runs on three
   workgroups, long enough to overlap and small enough to be co-scheduled.  The 150 packets of link P are cut into
   shards of 67, 13, 41 and 29, one stream each, enqueued round-robin with no synchronisation, three times over;
   link Q's 20 packets into 13 and 7.  Every shard must give its own serial bytes, the shards together the bytes of
   the one-batch run, and the one word all psdu_deframe calls add their good packets to must hold them all.
3. test_host_threads_share_one_context: four threads, one stream and one shard each, one Context; thread 0 has
   refused calls between its steps and finds its own text in wce_last_error(), the others' never changes.

Shown by mutation on an MI355X, in a scratch build that was never committed: with launch_sync_share
(csrc/wce_combine.hip) launching on the null stream in place of its argument, test 1 fails with "LinkQ: step
sync_share left other bytes in start than the serial run" -- the call ran on the sentinels while the blocker held
front_end_sync_stf, which then overwrote what it shared, so five windows keep their own start -- while the eleven
other GPU tests of the call (tests/test_combine_gpu.py's sync_share and link_mrc tests, tests/test_psdu_gpu.py's
link_mrc test), all on the null stream, still pass."""
import contextlib
import ctypes
import os
import re
import threading
import time

import numpy as np
import pytest

import chain_streams_model as M
import stf_model as st
import tx_model as tm

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRID = 6                        # WCE_VARIANT_GRID
N, NBLK = 53, 15
MOD, RATE, T, NBY, L = M.MOD, M.RATE, M.T, M.NBY, M.PSDU_LEN
SENT, SENT_F, SENT_W, SENT_B, SENT_L = 7.0 - 3.0j, 9.0, 0xDEAD, 0xA5, np.float32(-77.5)
N_GOOD_START = 5
# the blocker: a 64-QAM 3/4 decode of all-zero soft bits on three workgroups
BLOCKER_MOD, BLOCKER_RATE, BLOCKER_FRAMES = 6, 2, 600
# wce.h prototypes that end in a stream but are no stream-ordered call of one device: the two collectives need a
# communicator over several devices (tests/test_multi_gpu.py runs them)
NOT_HERE = {"wce_ctx_broadcast_state", "wce_comm_max_f64"}


def stream_entry_points(wce):
    """the library functions that take work for a stream: include/wce.h's prototypes whose last of several
    parameters is `void *stream`, each of which wce.py's table must bind with a trailing pointer"""
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "wce.h")).read(), flags=re.S)
    names = {m.group(1) for m in re.finditer(r"\b(wce_\w+)\s*\(([^;{}()]*),\s*void\s*\*\s*stream\s*\)\s*;", src)}
    table = {n for n, a in wce.wce.ABI.items() if len(a) > 1 and a[-1] is ctypes.c_void_p}
    assert names and names <= table, sorted(names - table)
    return names - NOT_HERE


class Recorder:
    """stands in for the loaded library: every call of a stream-taking function is noted with its stream and code"""

    def __init__(self, lib, names):
        self._lib, self._names, self.calls = lib, names, []

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if name not in self._names:
            return fn

        def call(*args):
            rc = fn(*args)
            s = args[-1]
            self.calls.append((name, s.value if isinstance(s, ctypes.c_void_p) else s, rc))
            return rc
        return call


@contextlib.contextmanager
def recording(wce):
    real = wce.load()
    rec = Recorder(real, stream_entry_points(wce))
    wce.wce._lib = rec
    try:
        yield rec
    finally:
        wce.wce._lib = real


@contextlib.contextmanager
def _grid(wce, v):
    lib = wce.load()
    try:
        assert lib.wce_debug_set_variant(GRID, v) == 0
        yield
    finally:
        assert lib.wce_debug_set_variant(GRID, 0) == 0


def _u8(a):
    return np.ascontiguousarray(a).reshape(-1).view(np.uint8)


class Buf:
    """a device (or pinned host) buffer and the contents every run starts from"""

    def __init__(self, wce, init, pinned=False):
        self.wce, self.init, self.pinned = wce, np.ascontiguousarray(init), pinned
        if pinned:
            self.d = wce.PinnedArray(self.init.shape, self.init.dtype)
        else:
            self.d = wce.DeviceArray.from_numpy(self.init)

    @property
    def addr(self):
        return self.d.addr

    def __int__(self):              # the package's wrappers take an address where they take a DeviceArray
        return self.d.addr

    def fill(self):
        if self.pinned:
            self.d.array[...] = self.init
        else:
            assert self.wce.load().wce_memcpy_htod(self.d.ptr, self.init.ctypes.data_as(ctypes.c_void_p),
                                                   self.init.nbytes) == 0

    def get(self):
        return self.d.array.copy() if self.pinned else self.d.numpy()


class Link:
    """buffers by name in the order the steps write them, and the steps"""
    accumulators = ("n_good",)          # not overwritten but added to: they start from a count, not a sentinel

    def out(self, name, shape, dtype=np.complex128, value=None, pinned=False):
        if value is None:
            value = {np.dtype(np.complex128): SENT, np.dtype(np.float64): SENT_F, np.dtype(np.uint32): SENT_W,
                     np.dtype(np.int32): SENT_W, np.dtype(np.uint64): SENT_W, np.dtype(np.uint8): SENT_B,
                     np.dtype(np.float32): SENT_L}[np.dtype(dtype)]
        self.b[name] = Buf(self.wce, np.full(shape, value, dtype), pinned)
        return self.b[name]

    def fill(self):
        for b in self.b.values():
            b.fill()
        self.wce.synchronize()

    def snapshot(self):
        return {k: b.get() for k, b in self.b.items()}

    def reference(self):
        """the steps on the null stream, a synchronise behind each -> every buffer's contents (kept)"""
        if self.ref is None:
            self.fill()
            for name, call, outs in self.steps():
                call(None)
                self.wce.synchronize()
            self.ref = self.snapshot()
        return self.ref

    def enqueue(self, stream):
        """-> (host seconds, step name) of every enqueue, the slowest first"""
        took = []
        for name, call, outs in self.steps():
            t0 = time.perf_counter()
            call(stream)
            took.append((time.perf_counter() - t0, name))
        return sorted(took, reverse=True)

    def compare(self, got, ref, what, skip=()):
        """in step order: the first buffer that differs names the call that wrote it"""
        seen = set()
        for name, call, outs in self.steps():
            for k in outs:
                if k in seen or k in skip:
                    continue
                seen.add(k)
                assert np.array_equal(_u8(got[k]), _u8(ref[k])), \
                    f"{what}: step {name} left other bytes in {k} than the serial run: it, or the call that " \
                    f"wrote its input, did not wait for the work queued before it"
        assert seen | set(skip) >= set(self.b), sorted(set(self.b) - seen)      # every buffer belongs to a step

    def no_sentinel_rows(self, ref):
        for k, b in self.b.items():
            if k in self.accumulators:
                continue
            rows = ref[k].shape[0] if ref[k].ndim > 1 else 1
            got, init = _u8(ref[k]).reshape(rows, -1), _u8(b.init).reshape(rows, -1)
            assert not np.any(np.all(got == init, axis=1)), f"{k}: a row still holds its sentinel"


class LinkP(Link):
    A = 1                       # antennas
    branch_major = ()           # buffers laid out [A][n]: none

    def __init__(self, wce, ctx, first=0, n=67, n_good=None):
        self.wce, self.ctx, self.first, self.n, self.b, self.ref = wce, ctx, first, n, {}, None
        c, sl = M.link_p_set(), slice(first, first + n)
        D = wce.DeviceArray.from_numpy
        self.pay_host = wce.PinnedArray((n, L - 4), np.uint8)
        self.pay_host.array[...] = c["payload"][sl]
        self.seeds, self.pre, self.taps = D(c["seeds"][sl]), D(tm.chain_pre()), D(c["taps"][sl])
        self.cfo, self.ow2, self.delay = D(c["cfo"][sl]), D(c["ow2"][sl]), D(c["delay"][sl])
        o = self.out
        o("pay", (n, L - 4), np.uint8), o("bits_tx", (n, NBY), np.uint8), o("tx", (n, NBLK, N)), o("field", (160,))
        o("cap", (n, M.P_LEN)), o("start", (n,), np.int32), o("metric", (n,), np.float64)
        o("rxpre", (n, N)), o("ow2e", (n,), np.float64, np.nan), o("cfo_e", (n,), np.float64), o("rx", (n, NBLK, N))
        o("h_lt", (n, N)), o("h_mmse", (n, N), value=complex(np.nan, np.nan))
        for p in ("", "2"):
            o("eq" + p, (n, NBLK, N)), o("sym" + p, (n, NBLK, N), np.uint8), o("theta" + p, (n, NBLK), np.float64)
            o("evm" + p, (n,), np.float64), o("nerr" + p, (n,), np.uint32)
            o("llr" + p, (n, NBLK, 48 * MOD), np.float32), o("bits" + p, (n, NBY), np.uint8)
            o("nbiterr" + p, (n,), np.uint32)
            if not p:
                o("h_dd", (n, N))
        o("psdu", (n, L), np.uint8), o("seed_rx", (n,), np.uint8), o("fcs_ok", (n,), np.uint32)
        if n_good is None:
            o("n_good", (1,), np.uint32, N_GOOD_START)
        else:
            self.b["n_good"] = n_good
        o("bitmap", ((n + 31) // 32,), np.uint32), o("n_bad", (1,), np.uint64)
        o("fcs_host", (n,), np.uint32, pinned=True)
        # beside the link: the unfused transmitter into the plain and _cfo front end
        o("wave", (n, 1360)), o("pre_a", (n, N)), o("ow2_a", (n,), np.float64), o("sym_a", (n, NBLK, N))
        o("cap2", (n, 1360)), o("pre_b", (n, N)), o("ow2_b", (n,), np.float64), o("cfo_b", (n,), np.float64)
        o("sym_b", (n, NBLK, N))
        # synthetic frames into the two MMSE stages and a plan, the conversions and the device copy
        o("tx_s", (n, NBLK, N)), o("rx_s", (n, NBLK, N)), o("pre_s", (n, N)), o("W", (n, N)), o("H_s", (n, N))
        o("H_p", (n, N)), o("ld", (n * N * 32,), np.uint8), o("H_back", (n, N)), o("H_copy", (n, N))
        b = self.b
        self.fr = ctx.frames(b["tx"], b["rx"], n, rx_pre=b["rxpre"], tx_pre=self.pre)
        self.fr_s = ctx.frames(b["tx_s"], b["rx_s"], n, rx_pre=b["pre_s"])
        self.est_out = wce.Outputs(b["h_lt"].addr, None, None, None, b["h_mmse"].addr, None, N, NBLK * N, N,
                                   wce.PS_LINEAR, 0)
        self.plan = ctx.plan(self.fr_s, wce.Outputs(None, None, None, None, b["H_p"].addr, None, N, 0, 0, 0, 0),
                             wce.PS_MMSE | wce.FRAME_COV)

    def _pass(self, p, h):
        """demodulate (every output), soft_demap and viterbi_decode with the estimate h, into the buffers *p"""
        b, c, n = self.b, self.ctx, self.n
        return [
            ("demodulate" + p, lambda s: c.demodulate(self.fr, b[h], None, N, MOD, eq=b["eq" + p], sym=b["sym" + p],
                                                      theta=b["theta" + p], evm=b["evm" + p], nerr=b["nerr" + p],
                                                      stream=s),
             ["eq" + p, "sym" + p, "theta" + p, "evm" + p, "nerr" + p]),
            ("soft_demap" + p, lambda s: c.soft_demap(b["eq" + p], b[h], n, None, N, MOD, llr=b["llr" + p], stream=s),
             ["llr" + p]),
            ("viterbi_decode" + p, lambda s: c.viterbi_decode(b["llr" + p], n, MOD, RATE, False, b["bits" + p],
                                                              ref_bits=b["bits_tx"], nbiterr=b["nbiterr" + p],
                                                              stream=s), ["bits" + p, "nbiterr" + p]),
        ]

    def steps(self):
        wce, c, b, n, lib = self.wce, self.ctx, self.b, self.n, self.wce.load()
        ok = lambda rc, what: wce.wce._check(rc, what)
        chan = dict(cfo=self.cfo, ow2=self.ow2, seed=M.P_SEED)
        return [
            ("memcpy_htod_async", lambda s: ok(lib.wce_memcpy_htod_async(b["pay"].addr, self.pay_host.addr,
                                                                         n * (L - 4), s), "htod_async"), ["pay"]),
            ("psdu_frame", lambda s: c.psdu_frame(b["pay"], n, MOD, RATE, length=L, seeds=self.seeds,
                                                  bits=b["bits_tx"], stream=s), ["bits_tx"]),
            ("reencode tx", lambda s: c.reencode(b["bits_tx"], n, MOD, RATE, tx=b["tx"], stream=s), ["tx"]),
            ("modulate field", lambda s: c.modulate(None, 1, b["field"], 0, self.pre, stream=s), ["field"]),
            ("transmit", lambda s: c.transmit(b["tx"], n, b["cap"], M.P_LEN, NBLK, self.pre, 0, taps=self.taps,
                                              n_taps=6, taps_stride=6, delay=self.delay, first_frame=self.first,
                                              stream=s, **chan), ["cap"]),
            ("front_end_sync", lambda s: c.front_end_sync(b["cap"], n, M.P_LEN, b["field"].addr + 32 * 16,
                                                          M.THRESHOLD, 0, b["start"], b["metric"], stream=s),
             ["start", "metric"]),
            ("front_end_preamble at", lambda s: c.front_end_preamble(b["cap"], n, M.P_LEN, b["rxpre"], b["ow2e"],
                                                                      cfo=b["cfo_e"], start=b["start"], stream=s),
             ["rxpre", "ow2e", "cfo_e"]),
            ("front_end_blocks at", lambda s: c.front_end_blocks(b["cap"], n, NBLK, b["rx"], cfo=b["cfo_e"],
                                                                  start=b["start"], capture_len=M.P_LEN, stream=s),
             ["rx"]),
            ("estimate_noise", lambda s: c.estimate(self.fr, self.est_out, wce.LT_LS | wce.PS_MMSE | wce.FRAME_COV,
                                                    stream=s, ow2=b["ow2e"]), ["h_lt", "h_mmse"]),
            *self._pass("", "h_lt"),
            ("reencode h", lambda s: c.reencode(b["bits"], n, MOD, RATE, theta=b["theta"], frames=self.fr,
                                                h=b["h_dd"], stream=s), ["h_dd"]),
            *self._pass("2", "h_dd"),
            ("psdu_deframe", lambda s: c.psdu_deframe(b["bits2"], n, MOD, RATE, length=L, psdu=b["psdu"],
                                                      seed=b["seed_rx"], fcs_ok=b["fcs_ok"], n_good=b["n_good"],
                                                      stream=s), ["psdu", "seed_rx", "fcs_ok", "n_good"]),
            ("nonfinite_scan", lambda s: c.nonfinite_scan(b["h_mmse"], n, bitmap=b["bitmap"], n_bad=b["n_bad"],
                                                          stream=s), ["bitmap", "n_bad"]),
            ("memcpy_dtoh_async", lambda s: ok(lib.wce_memcpy_dtoh_async(b["fcs_host"].addr, b["fcs_ok"].addr, 4 * n,
                                                                         s), "dtoh_async"), ["fcs_host"]),
            ("modulate", lambda s: c.modulate(b["tx"], n, b["wave"], NBLK, self.pre, stream=s), ["wave"]),
            ("front_end_preamble", lambda s: c.front_end_preamble(b["wave"], n, 160, b["pre_a"], b["ow2_a"],
                                                                  lptot_stride=1360, stream=s), ["pre_a", "ow2_a"]),
            ("front_end_blocks", lambda s: c.front_end_blocks(b["wave"].addr + 160 * 16, n, NBLK, b["sym_a"],
                                                              packet_stride=1360, stream=s), ["sym_a"]),
            ("channel", lambda s: c.channel(b["wave"], n, 1360, b["cap2"], 1360, first_frame=1000 + self.first,
                                            stream=s, **chan), ["cap2"]),
            ("front_end_preamble_cfo", lambda s: c.front_end_preamble(b["cap2"], n, 160, b["pre_b"], b["ow2_b"],
                                                                      lptot_stride=1360, cfo=b["cfo_b"], stream=s),
             ["pre_b", "ow2_b", "cfo_b"]),
            ("front_end_blocks_cfo", lambda s: c.front_end_blocks(b["cap2"].addr + 160 * 16, n, NBLK, b["sym_b"],
                                                                  packet_stride=1360, cfo=b["cfo_b"], stream=s),
             ["sym_b"]),
            ("synth", lambda s: c.synth(b["tx_s"], b["rx_s"], b["pre_s"], n, first_frame=self.first, seed=M.P_SEED,
                                        stream=s), ["tx_s", "rx_s", "pre_s"]),
            ("mmse_solve", lambda s: c.mmse_solve(self.fr_s, b["W"], stream=s), ["W"]),
            ("mmse_apply", lambda s: c.mmse_apply(b["W"], b["H_s"], n, stream=s), ["H_s"]),
            ("plan launch", lambda s: self.plan.launch(s), ["H_p"]),
            ("complex_to_ldc", lambda s: wce.complex_to_ldc(b["H_s"], b["ld"], n * N, s), ["ld"]),
            ("ldc_to_complex", lambda s: wce.ldc_to_complex(b["ld"], b["H_back"], n * N, s), ["H_back"]),
            ("memcpy_dtod", lambda s: ok(lib.wce_memcpy_dtod(b["H_copy"].addr, b["H_back"].addr, n * N * 16, s),
                                         "dtod"), ["H_copy"]),
        ]

    def meaningful(self, ref):
        """the reference run found what the CPU chain finds"""
        m, sl = M.link_p_model(), slice(self.first, self.first + self.n)
        self.no_sentinel_rows(ref)
        assert m["detected"].all() and np.all(ref["start"] >= 0), "a packet was not detected"
        good = int(m["fcs_ok"][sl].sum())
        print(f"\nlink P frames {self.first}..{self.first + self.n - 1}: {int(ref['fcs_ok'].sum())} good of {self.n} "
              f"(the numpy chain: {good}; packets judged otherwise: "
              f"{int(np.sum(ref['fcs_ok'] != m['fcs_ok'][sl]))}), after the first decode "
              f"{int(np.sum(ref['nbiterr'] == 0))} without a bit error (the numpy chain: "
              f"{int(m['fcs_first'][sl].sum())})")
        assert int(ref["fcs_ok"].sum()) == good and 0 < good < self.n
        assert np.array_equal(ref["fcs_host"], ref["fcs_ok"]) and np.array_equal(ref["H_copy"], ref["H_s"])
        assert int(ref["n_bad"][0]) == 0 and not ref["bitmap"].any()
        return good


class LinkQ(Link):
    A = M.Q_A
    branch_major = ("cap", "start", "cfo_e")

    def __init__(self, wce, ctx, first=0, n=13, n_good=None):
        self.wce, self.ctx, self.first, self.n, self.b, self.ref = wce, ctx, first, n, {}, None
        c, sl, A = M.link_q_set(), slice(first, first + n), self.A
        D = wce.DeviceArray.from_numpy
        nn = self.nn = A * n
        self.pay, self.seeds = D(np.tile(c["payload"][sl], (A, 1))), D(np.tile(c["seeds"][sl], A))
        self.pre, self.knots = D(tm.chain_pre()), [D(c["knots"][a][sl]) for a in range(A)]
        self.cfo, self.ow2, self.delay = D(c["cfo"][sl]), D(c["ow2"][sl]), D(c["delay"][sl])
        o = self.out
        o("bits_tx", (nn, NBY), np.uint8), o("tx", (nn, NBLK, N)), o("field", (160,)), o("wave", (n, 1520))
        o("cap", (nn, M.Q_LEN)), o("cap_t", (n, M.P_LEN)), o("start_t", (n,), np.int32)
        o("metric_t", (n,), np.float64), o("start", (nn,), np.int32), o("cfo_e", (nn,), np.float64)
        o("metric_stf", (nn,), np.float64), o("metric_ltf", (nn,), np.float64)
        o("rxpre", (nn, N)), o("ow2e", (nn,), np.float64), o("rx", (nn, NBLK, N))
        o("h_lt", (nn, N)), o("h_lin", (nn, N)), o("rxc", (n, NBLK, N)), o("hc", (n, N))
        o("eq", (n, NBLK, N)), o("sym", (n, NBLK, N), np.uint8), o("theta", (n, NBLK), np.float64)
        o("evm", (n,), np.float64), o("nerr", (n,), np.uint32), o("h_blocks", (n, NBLK, N)), o("h_last", (n, N))
        o("llr", (n, NBLK, 48 * MOD), np.float32), o("bits", (n, NBY), np.uint8), o("nbiterr", (n,), np.uint32)
        o("psdu", (n, L), np.uint8), o("seed_rx", (n,), np.uint8), o("fcs_ok", (n,), np.uint32)
        if n_good is None:
            o("n_good", (1,), np.uint32, N_GOOD_START)
        else:
            self.b["n_good"] = n_good
        b = self.b
        self.fr = ctx.frames(b["tx"], b["rx"], nn, rx_pre=b["rxpre"], tx_pre=self.pre)
        self.fr_c = ctx.frames(b["tx"], b["rxc"], n)
        self.est_out = wce.Outputs(b["h_lt"].addr, b["h_lin"].addr, None, None, None, None, N, NBLK * N, N,
                                   wce.PS_LINEAR, 0)

    def steps(self):
        wce, c, b, n, nn, A = self.wce, self.ctx, self.b, self.n, self.nn, self.A
        chan = dict(cfo=self.cfo, ow2=self.ow2, delay=self.delay, seed=M.Q_SEED)
        tv = dict(n_knots=M.Q_KNOTS, knot_period=M.Q_PERIOD, n_taps=6, knots_frame_stride=M.Q_KNOTS * 6)

        def branch(a):
            return ("channel_tv %d" % a,
                    lambda s: c.channel_tv(b["wave"], n, 1520, b["cap"].addr + a * n * M.Q_LEN * 16, M.Q_LEN,
                                           self.knots[a], first_frame=a * M.Q_B + self.first, stream=s, **tv, **chan),
                    ["cap"])
        return [
            ("psdu_frame", lambda s: c.psdu_frame(self.pay, nn, MOD, RATE, length=L, seeds=self.seeds,
                                                  bits=b["bits_tx"], stream=s), ["bits_tx"]),
            ("reencode tx", lambda s: c.reencode(b["bits_tx"], nn, MOD, RATE, tx=b["tx"], stream=s), ["tx"]),
            ("modulate field", lambda s: c.modulate(None, 1, b["field"], 0, self.pre, stream=s), ["field"]),
            ("short_field", lambda s: c.short_field(b["wave"], n, c.stf_amplitude(), 1520, stream=s), ["wave"]),
            ("modulate", lambda s: c.modulate(b["tx"], n, b["wave"].addr + 160 * 16, NBLK, self.pre, 0,
                                              wave_stride=1520, stream=s), ["wave"]),
            *[branch(a) for a in range(A)],
            ("transmit_tv", lambda s: c.transmit_tv(b["tx"], n, b["cap_t"], M.P_LEN, self.knots[0], tx_pre=self.pre,
                                                    first_frame=A * M.Q_B + self.first, stream=s, **tv, **chan),
             ["cap_t"]),
            ("front_end_sync", lambda s: c.front_end_sync(b["cap_t"], n, M.P_LEN, b["field"].addr + 32 * 16,
                                                          M.THRESHOLD, 0, b["start_t"], b["metric_t"], stream=s),
             ["start_t", "metric_t"]),
            ("front_end_sync_stf", lambda s: c.front_end_sync_stf(b["cap"], nn, M.Q_LEN, b["field"].addr + 32 * 16,
                                                                  st.THR_STF, M.THRESHOLD, 0, b["start"], b["cfo_e"],
                                                                  b["metric_stf"], b["metric_ltf"], stream=s),
             ["metric_stf", "metric_ltf"]),
            ("sync_share", lambda s: c.sync_share(b["metric_ltf"], n, A, b["start"], b["cfo_e"], stream=s),
             ["start", "cfo_e"]),
            ("front_end_preamble at", lambda s: c.front_end_preamble(b["cap"], nn, M.Q_LEN, b["rxpre"], b["ow2e"],
                                                                      cfo=b["cfo_e"], estimate_cfo=False,
                                                                      start=b["start"], stream=s), ["rxpre", "ow2e"]),
            ("front_end_blocks at", lambda s: c.front_end_blocks(b["cap"], nn, NBLK, b["rx"], cfo=b["cfo_e"],
                                                                  start=b["start"], capture_len=M.Q_LEN, stream=s),
             ["rx"]),
            ("estimate", lambda s: c.estimate(self.fr, self.est_out, wce.LT_LS | wce.PS_LINEAR, stream=s),
             ["h_lt", "h_lin"]),
            ("combine", lambda s: c.combine(b["rx"], b["h_lt"], n, A, b["ow2e"], b["rxc"], b["hc"], stream=s),
             ["rxc", "hc"]),
            ("track_demodulate", lambda s: c.track_demodulate(
                self.fr_c, b["hc"], M.Q_MU, M.Q_BETA, N, MOD, eq=b["eq"], sym=b["sym"], theta=b["theta"],
                evm=b["evm"], nerr=b["nerr"], h_blocks=b["h_blocks"], h_last=b["h_last"], stream=s),
             ["eq", "sym", "theta", "evm", "nerr", "h_blocks", "h_last"]),
            ("soft_demap_blocks", lambda s: c.soft_demap_blocks(b["eq"], b["h_blocks"], n, MOD, llr=b["llr"], stream=s),
             ["llr"]),
            ("viterbi_decode", lambda s: c.viterbi_decode(b["llr"], n, MOD, RATE, False, b["bits"],
                                                          ref_bits=b["bits_tx"], nbiterr=b["nbiterr"], stream=s),
             ["bits", "nbiterr"]),
            ("psdu_deframe", lambda s: c.psdu_deframe(b["bits"], n, MOD, RATE, length=L, psdu=b["psdu"],
                                                      seed=b["seed_rx"], fcs_ok=b["fcs_ok"], n_good=b["n_good"],
                                                      stream=s), ["psdu", "seed_rx", "fcs_ok", "n_good"]),
        ]

    def meaningful(self, ref):
        m, sl = M.link_q_model(), slice(self.first, self.first + self.n)
        self.no_sentinel_rows(ref)
        assert m["detected"].all() and np.all(ref["start"] >= 0) and np.all(ref["start_t"] >= 0), \
            "a packet was not detected"
        good = int(m["fcs_ok"][sl].sum())
        print(f"\nlink Q packets {self.first}..{self.first + self.n - 1}: {int(ref['fcs_ok'].sum())} good of {self.n} "
              f"(the numpy chain: {good}; packets judged otherwise: {int(np.sum(ref['fcs_ok'] != m['fcs_ok'][sl]))})")
        assert int(ref["fcs_ok"].sum()) == good and 0 < good < self.n
        return good


class Blocker:
    """one of the library's own kernels on buffers no step touches, long enough to hold a stream while the host
    enqueues a whole link behind it.  The knob is read on the host when the kernel is launched and is back at 0
    before launch() returns"""

    def __init__(self, wce, ctx, frames=BLOCKER_FRAMES):
        self.wce, self.ctx, self.frames = wce, ctx, frames
        nby = (wce.info_bits(BLOCKER_MOD, BLOCKER_RATE) + 7) // 8
        self.llr = wce.DeviceArray((frames, NBLK, 48 * BLOCKER_MOD), np.float32, zero=True)
        self.bits = wce.DeviceArray((frames, nby), np.uint8, zero=True)

    def launch(self, stream):
        with _grid(self.wce, 1):
            self.ctx.viterbi_decode(self.llr, self.frames, BLOCKER_MOD, BLOCKER_RATE, True, self.bits, stream=stream)


@pytest.fixture(scope="module")
def ctx(gpu_wce):
    pre = tm.chain_pre()
    c = gpu_wce.Context(pre, pre, 1e-6, gpu_wce.MMSE_TEXTBOOK)
    c.reserve(M.P_B)
    return c


def held_run(wce, ctx, link, blocker):
    """link's steps behind the blocker on a new stream -> (every buffer, the recorded calls, the stream's handle,
    whether the event behind the blocker was still pending when the last enqueue had returned, host seconds)"""
    stream, ev = wce.Stream(), wce.Event()
    with recording(wce) as rec:
        wce.wce._check(wce.load().wce_ctx_reserve_stream(ctx.handle, link.n * link.A, stream.handle),
                       "wce_ctx_reserve_stream")
        link.fill()
        blocker.launch(stream.handle)
        ev.record(stream)
        took = link.enqueue(stream.handle)
        pending = not ev.query()
        stream.synchronize()
    return link.snapshot(), rec.calls, stream.handle.value, pending, took


def test_every_call_is_ordered_behind_a_held_stream(gpu_wce, ctx):
    wce = gpu_wce
    blocker = Blocker(wce, ctx)
    called = set()
    for link in (LinkP(wce, ctx, 0, 67), LinkQ(wce, ctx, 0, 13)):
        what = type(link).__name__
        ref = link.reference()
        link.meaningful(ref)
        got, calls, handle, pending, took = held_run(wce, ctx, link, blocker)
        slow = ", ".join(f"{name} {1e3 * dt:.2f} ms" for dt, name in took[:3])
        print(f"{what}: {len(took)} steps enqueued in {1e3 * sum(dt for dt, _ in took):.2f} ms of host time "
              f"(the slowest: {slow})")
        assert calls and all(rc == 0 for _, _, rc in calls), [c for c in calls if c[2] != 0]
        assert pending, f"{what}: the blocker had finished when the last enqueue returned: a call waited for the " \
                        f"stream, allocated or read back (the slowest enqueues: {slow})"
        link.compare(got, ref, what)
        astray = sorted({name for name, s, _ in calls if s != handle})
        assert not astray, f"{what}: called with another stream than the caller's: {astray}"
        called |= {name for name, _, _ in calls}
    missing = sorted(stream_entry_points(wce) - called)
    assert not missing, f"stream-taking entry points without a step in either link: {missing}"


def _round_robin(links, streams):
    lists = [l.steps() for l in links]
    for i in range(max(len(s) for s in lists)):
        for steps, s in zip(lists, streams):
            if i < len(steps):
                steps[i][1](s.handle)


def _overlap(wce, ctx, cls, shards, total, together):
    """cls's problem of `total` packets cut into `shards`, one stream each, under the knob"""
    n_good = Buf(wce, np.full(1, N_GOOD_START, np.uint32))
    links = [cls(wce, ctx, first, n, n_good) for first, n in shards]
    whole = cls(wce, ctx, 0, total)
    ref0 = whole.reference()                                    # every launcher's own grid
    whole.meaningful(ref0)
    whole.ref = None
    with _grid(wce, 1):
        ref1 = whole.reference()
        whole.compare(ref1, ref0, f"{cls.__name__} {total} packets on three workgroups")
        refs, counts = [], []
        for l in links:
            refs.append(l.reference())                          # refills the shared word: 5 + this shard's own count
            counts.append(int(refs[-1]["n_good"][0]) - N_GOOD_START)
            assert counts[-1] == int(refs[-1]["fcs_ok"].sum())
        for k in together:                                      # the shards are the batch, cut
            a = cls.A if k in cls.branch_major else 1
            rows = lambda x: x.reshape(a, -1, *x.shape[1:])
            cat = np.concatenate([rows(r[k]) for r in refs], axis=1)
            assert np.array_equal(_u8(cat), _u8(rows(ref1[k]))), f"{k}: the shards together are not the batch"
        assert sum(counts) == int(ref1["n_good"][0]) - N_GOOD_START
        streams = [wce.Stream() for _ in links]
        for l, s in zip(links, streams):
            wce.wce._check(wce.load().wce_ctx_reserve_stream(ctx.handle, l.n * l.A, s.handle), "reserve")
        for rep in range(3):
            for l in links:
                l.fill()
            _round_robin(links, streams)
            for s in streams:
                s.synchronize()
            for l, r, (first, n) in zip(links, refs, shards):
                l.compare(l.snapshot(), r, f"{cls.__name__} shard at {first} beside the others, round {rep}",
                          skip=("n_good",))
            assert int(n_good.get()[0]) == N_GOOD_START + sum(counts), "psdu_deframe ADDS to n_good"


def test_streams_that_overlap_give_the_serial_bytes(gpu_wce, ctx):
    _overlap(gpu_wce, ctx, LinkP, M.P_SHARDS, M.P_B, ("cap", "bits2", "fcs_ok", "psdu"))
    _overlap(gpu_wce, ctx, LinkQ, M.Q_SHARDS, M.Q_B, ("cap", "start", "cfo_e", "bits", "fcs_ok"))


def test_host_threads_share_one_context(gpu_wce, ctx):
    wce, lib = gpu_wce, gpu_wce.load()
    links = [LinkP(wce, ctx, first, n) for first, n in M.P_SHARDS]
    refs = [l.reference() for l in links]
    for l in links:
        l.fill()
    got, errors = {}, []

    def refused(l, s):
        """two calls test_psdu_abi.py lists as WCE_EINVAL before any launch -> the texts they leave"""
        b = l.b
        par = wce.PsduPar(MOD, RATE, L, 0, None, None)
        out = wce.PsduOut(b["psdu"].addr, L, b["seed_rx"].addr, b["fcs_ok"].addr, b["n_good"].addr)
        assert lib.wce_psdu_deframe(ctx.handle, ctypes.byref(par), b["bits2"].addr, NBY, -1, ctypes.byref(out), s) == -1
        first = lib.wce_last_error().decode()
        out.fcs_ok = b["fcs_ok"].addr + 2
        assert lib.wce_psdu_deframe(ctx.handle, ctypes.byref(par), b["bits2"].addr, NBY, l.n, ctypes.byref(out), s) == -1
        return first, lib.wce_last_error().decode()

    def worker(t):
        try:
            l, s = links[t], wce.Stream()
            wce.wce._check(lib.wce_ctx_reserve_stream(ctx.handle, l.n, s.handle), "reserve")
            before = lib.wce_last_error()
            for name, call, outs in l.steps():
                call(s.handle)
                if t == 0:
                    a, b = refused(l, s.handle)
                    assert "wce_psdu_deframe" in a and "n_frames" in a and "4-byte" in b, (a, b)
                else:
                    assert lib.wce_last_error() == before, (t, name, lib.wce_last_error())
            s.synchronize()
            got[t] = l.snapshot()
        except BaseException as e:  # reported below
            errors.append((t, repr(e)))

    th = [threading.Thread(target=worker, args=(t,)) for t in range(len(links))]
    for x in th:
        x.start()
    for x in th:
        x.join(timeout=60)
    assert not any(x.is_alive() for x in th), "a thread did not finish"
    assert not errors, errors
    for t, (l, r) in enumerate(zip(links, refs)):
        l.compare(got[t], r, f"thread {t}")
