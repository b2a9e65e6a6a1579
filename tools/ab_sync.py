"""What do packet detection and the per-frame-start front end cost?  One process,
HIP events (wce_event_*), interleaved series:

  sync                      wce_front_end_sync on 65,536 windows of 488 samples
  blocks_cfo / blocks_at    wce_front_end_blocks_cfo on aligned packets against
                            wce_front_end_blocks_at on the capture windows the
                            packets were copied from
  preamble_cfo / _at        the same for the long training field, offset estimated
                            and offset given; and both calls on one placement (the
                            field at sample 0 of every window, the existing call
                            striding over the windows), which leaves the kernels'
                            own difference

usage: python tools/ab_sync.py [DIR ...] [--frames 65536] [--rounds 7] [--reps 20] [--align 1]

DIR/libwce.so: a build (default: the package's own).  The first DIR runs every
series; each further DIR adds a sync series of its own (an A/B of two sync
kernels).  Each round times every series in turn (odd rounds in reverse order):
2 warm-up calls, then `reps` calls between two events; one untimed round comes
first.  After the last round each _at series' output is compared bit for bit
with its aligned twin's, and sync's starts with the positions the fields were
put at.  --align 8 puts every start on a 128-byte boundary of its window, as
the aligned copies are: what is left of the _at calls' extra time then is the
kernels', the rest the placement's.

sync is reported against both of its floors: the FP64 rate over the flops the
kernel executes (64 lanes x 8 lags x 64 taps x 8 flop per 448-lag tile, whatever
the window's length) and over the useful ones ((L - 63) x 64 complex MACs), and
the HBM rate over L x 16 B per frame.
"""
import argparse
import ctypes
import importlib.util
import os

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "80211parallelestimation_amd")
N, NB = 53, 15
L_SYNC = 488                 # sync's window
W, SLACK = 1424, 96          # the front end's window: 128 + 1200 + 96; starts in 0..96


def load(d):
    spec = importlib.util.spec_from_file_location("wce_" + os.path.basename(d.rstrip("/")), os.path.join(PKG, "wce.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    path = os.path.join(d, "libwce.so")
    probe = ctypes.CDLL(path)
    m.ABI = {k: v for k, v in m.ABI.items() if hasattr(probe, k)}
    m._lib = None
    m.load(path)
    return m


def tiled(m, host, B):
    """a device array [B][...] holding the host chunk over and over"""
    d = m.DeviceArray((B,) + host.shape[1:], host.dtype)
    row = host[0].nbytes
    for off in range(0, B, len(host)):
        k = min(len(host), B - off)
        assert m.load().wce_memcpy_htod(d.addr + off * row, host[:k].ctypes.data, k * row) == 0
    return d


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("dirs", nargs="*", default=[PKG])
    ap.add_argument("--frames", type=int, default=65536)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--align", type=int, default=1, help="starts are multiples of this many samples (8: 128 B)")
    args = ap.parse_args()
    B = args.frames
    rng = np.random.default_rng(0)
    chunk = min(4096, B)
    cplx = lambda *shape: (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)) * 0.01
    mods = [load(d) for d in args.dirs]
    m = mods[0]

    # sync: noise windows with a repeated clean symbol (amplitude 10 x the noise) at a known position
    ltf_h = cplx(64)
    pos_h = rng.integers(0, L_SYNC - 127, chunk).astype(np.int32)
    win_h = cplx(chunk, L_SYNC)
    for f in range(chunk):
        win_h[f, pos_h[f]:pos_h[f] + 128] += 10 * np.tile(ltf_h, 2)
    win, ltf = tiled(m, win_h, B), m.DeviceArray.from_numpy(ltf_h)
    start, metric = m.DeviceArray((B,), np.int32, zero=True), m.DeviceArray((B,), np.float64, zero=True)

    # the front end: capture windows, per-frame starts, and the aligned copies the existing calls need
    cap_h = cplx(chunk, W)
    st_h = (rng.integers(0, SLACK + 1, chunk) // args.align * args.align).astype(np.int32)
    idx = st_h[:, None] + np.arange(128 + NB * 80)[None, :]
    cut = np.take_along_axis(cap_h, idx, axis=1)
    lt_h, pk_h = np.ascontiguousarray(cut[:, :128]), np.ascontiguousarray(cut[:, 128:])
    cap, st, lt, pk = tiled(m, cap_h, B), tiled(m, st_h, B), tiled(m, lt_h, B), tiled(m, pk_h, B)
    sym, pre, ow2 = m.DeviceArray((B, NB, N)), m.DeviceArray((B, N)), m.DeviceArray((B,), np.float64)
    given = m.DeviceArray.from_numpy(rng.uniform(-1 / 128, 1 / 128, B))
    est = m.DeviceArray((B,), np.float64, zero=True)
    zero = m.DeviceArray((B,), np.int32, zero=True)

    series, keep = [], []
    for i, mod in enumerate(mods):
        ctx, stream = mod.Context(empty=True), mod.Stream()
        keep += [ctx, stream]
        s = stream.handle
        tag = "sync" if len(mods) == 1 else f"sync {os.path.basename(args.dirs[i].rstrip('/'))}"
        series.append((tag, "sync", mod, stream, lambda c=ctx, s=s: c.front_end_sync(
            win.addr, B, L_SYNC, ltf.addr, 0.25, 0, start.addr, metric.addr, stream=s)))
        if i:
            continue
        series.append(("blocks_cfo", "blocks", mod, stream, lambda c=ctx, s=s: c.front_end_blocks(
            pk.addr, B, NB, sym.addr, stream=s, cfo=given.addr)))
        series.append(("blocks_at", "blocks", mod, stream, lambda c=ctx, s=s: c.front_end_blocks(
            cap.addr, B, NB, sym.addr, stream=s, cfo=given.addr, start=st.addr, capture_len=W)))
        series.append(("preamble_cfo estimate", "preamble", mod, stream, lambda c=ctx, s=s: c.front_end_preamble(
            lt.addr, B, 128, pre.addr, ow2.addr, stream=s, cfo=est.addr)))
        series.append(("preamble_at estimate", "preamble", mod, stream, lambda c=ctx, s=s: c.front_end_preamble(
            cap.addr, B, W, pre.addr, ow2.addr, stream=s, cfo=est.addr, start=st.addr)))
        series.append(("preamble_cfo given", "preamble", mod, stream, lambda c=ctx, s=s: c.front_end_preamble(
            lt.addr, B, 128, pre.addr, ow2.addr, stream=s, cfo=given.addr, estimate_cfo=False)))
        series.append(("preamble_at given", "preamble", mod, stream, lambda c=ctx, s=s: c.front_end_preamble(
            cap.addr, B, W, pre.addr, ow2.addr, stream=s, cfo=given.addr, estimate_cfo=False, start=st.addr)))
        # the same placement for both: the field at sample 0 of every window, the existing call striding over them
        series.append(("preamble_cfo in windows", "preamble", mod, stream, lambda c=ctx, s=s: c.front_end_preamble(
            cap.addr, B, 128, pre.addr, ow2.addr, stream=s, cfo=given.addr, estimate_cfo=False, lptot_stride=W)))
        series.append(("preamble_at start 0", "preamble", mod, stream, lambda c=ctx, s=s: c.front_end_preamble(
            cap.addr, B, W, pre.addr, ow2.addr, stream=s, cfo=given.addr, estimate_cfo=False, start=zero.addr)))
    times = {s[0]: [] for s in series}
    outs = {}
    for rd in range(-1, args.rounds):   # round -1: untimed
        for name, kind, mod, stream, f in (series if rd % 2 == 0 else series[::-1]):
            for _ in range(2):
                f()
            e0, e1 = mod.Event(), mod.Event()
            e0.record(stream.handle)
            for _ in range(args.reps):
                f()
            e1.record(stream.handle)
            t = e0.elapsed_ms(e1) / args.reps * 1e3
            if rd >= 0:
                times[name].append(t)
            if rd == args.rounds - 1:
                outs[name] = {"sync": lambda: (start.numpy(), metric.numpy()), "blocks": lambda: (sym.numpy(),),
                              "preamble": lambda: (pre.numpy(), ow2.numpy(), est.numpy())}[kind]()
    tiles = -(-(L_SYNC - 127) // 448)
    executed, useful = B * tiles * 64 * 8 * 64 * 8, B * (L_SYNC - 63) * 64 * 8
    nbytes = {"sync": B * L_SYNC * 16, "blocks": B * NB * (1024 + 848), "preamble": B * (2048 + 848 + 8)}
    print(f"{B} frames, {args.rounds} rounds x {args.reps} calls, us per call (HIP events); sync on {L_SYNC}-sample "
          f"windows, the front end on {NB} blocks + a 128-sample field, starts 0..{SLACK} (multiples of {args.align}) in {W}-sample windows")
    for name, kind, *_ in series:
        t = times[name]
        med = np.median(t)
        line = f"{name:24s} median {med:8.2f}  min {min(t):8.2f}  max {max(t):8.2f}  {nbytes[kind] / med / 1e3:6.0f} GB/s"
        if kind == "sync":
            line += f"  {executed / med / 1e6:5.1f} TFLOP/s executed  {useful / med / 1e6:5.1f} TFLOP/s useful"
        print(line + "  runs " + " ".join(f"{x:.2f}" for x in t))
    want = np.tile(pos_h, -(-B // chunk))[:B]
    for name, kind, *_ in series:
        if kind == "sync":
            s_, m_ = outs[name]
            print(f"{name}: starts equal the fields' positions: {bool(np.array_equal(s_, want))}; "
                  f"metric {m_.min():.3f} .. {m_.max():.3f}; same bits as {series[0][0]}: "
                  f"{bool(np.array_equal(s_, outs[series[0][0]][0]) and np.array_equal(m_, outs[series[0][0]][1]))}")
    for a, b in (("blocks_at", "blocks_cfo"), ("preamble_at estimate", "preamble_cfo estimate"),
                 ("preamble_at given", "preamble_cfo given"), ("preamble_at start 0", "preamble_cfo in windows")):
        p = times[b]
        same = all(np.array_equal(x.view(np.uint8), y.view(np.uint8)) for x, y in zip(outs[a], outs[b]))
        print(f"{a} over {b}: {np.median(times[a]) / np.median(p) - 1.0:+.2%} (median over median; the aligned "
              f"call's spread {(max(p) - min(p)) / np.median(p):.2%}); same bits: {same}")


if __name__ == "__main__":
    main()
