"""What does detection on the short training field cost?  One process, HIP events
(wce_event_*), interleaved series, after tools/ab_sync.py:

  sync_stf L / sync L       wce_front_end_sync_stf against wce_front_end_sync, the
                            yardstick, on the same 65,536 windows of L = 488 and of
                            L = 1,648 samples
  short_field               wce_short_field into 65,536 rows of 160 samples

usage: python tools/ab_stf.py [--frames 65536] [--rounds 7] [--reps 10]

Every window holds noise and, at a known position, a short field, a long field
(32-sample prefix, two copies) and packet-like samples to the window's end, all
turned by 0.002 cycles per sample (20 kHz at 10 MHz), which both calls bear.
Each round times every series in turn (odd rounds in reverse order): 2 warm-up
calls, then `reps` calls between two events; one untimed round comes first.
After the last round the starts of both calls are compared with the positions
the packets were put at, and sync_stf's offset with the one applied.

Rates.  sync_stf does sync's correlation, one complex MAC per sample for q, and
a second visit of the window.  Executed flops per frame: per tile of its second
pass what sync executes (64 lanes x 8 lags x 64 taps x 8 flop) plus 576 complex
products of the derotation (6 flop); per tile of its first pass 576 + 64 x 16
products q (6 flop) and as many |x|^2 (3 flop), and 64 x 8 lags x 2 sums of 3
terms.  Useful: (L - 63) x 64 complex MACs and L - 16 products q.  Bytes: the
window once from HBM, L x 16 B; the second visit is served by the caches.
"""
import argparse
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
EPS = 0.002
LENGTHS = (488, 1648)
LAGS_STF, LAGS_LTF = 432, 448


def tiled(m, host, B):
    """a device array [B][...] holding the host chunk over and over"""
    d = m.DeviceArray((B,) + host.shape[1:], host.dtype)
    row = host[0].nbytes
    for off in range(0, B, len(host)):
        k = min(len(host), B - off)
        assert m.load().wce_memcpy_htod(d.addr + off * row, host[:k].ctypes.data, k * row) == 0
    return d


def windows(rng, chunk, L, ltf, stf):
    """noise at -20 dB around a packet head at a known position -> (windows [chunk][L], the long field's first
    copy's position [chunk])"""
    p0 = float(np.mean(np.abs(ltf) ** 2))
    cplx = lambda *shape: (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)) * np.sqrt(p0 / 2)
    win = 0.1 * cplx(chunk, L)
    pos = rng.integers(0, L - 320 + 1, chunk)
    head = np.concatenate([stf, ltf[32:], ltf, ltf])
    for f in range(chunk):
        pk = np.concatenate([head, cplx(L)])[:L - pos[f]]
        win[f, pos[f]:] += pk * np.exp(2j * np.pi * EPS * np.arange(len(pk)))
    return win, (pos + 192).astype(np.int32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=65536)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=10)
    args = ap.parse_args()
    B = args.frames
    import importlib
    m = importlib.import_module("80211parallelestimation_amd")
    m.load()
    import stf_model as st
    import sync_model as sm
    rng = np.random.default_rng(0)
    chunk = min(1024, B)
    ltf_h = sm.clean_ltf()
    stf_h = np.asarray(st.short_field(1.0), np.complex128)
    ctx, stream = m.Context(empty=True), m.Stream()
    s = stream.handle
    ltf = m.DeviceArray.from_numpy(ltf_h)
    start, metric = m.DeviceArray((B,), np.int32, zero=True), m.DeviceArray((B,), np.float64, zero=True)
    cfo, mstf = m.DeviceArray((B,), np.float64, zero=True), m.DeviceArray((B,), np.float64, zero=True)
    wave = m.DeviceArray((B, 160), zero=True)
    series, want = [], {}
    for L in LENGTHS:
        win_h, want[L] = windows(rng, chunk, L, ltf_h, stf_h)
        win = tiled(m, win_h, B)
        series.append((f"sync_stf {L}", "stf", L, lambda w=win, L=L: ctx.front_end_sync_stf(
            w.addr, B, L, ltf.addr, 0.25, 0.25, 0, start.addr, cfo.addr, mstf.addr, metric.addr, stream=s)))
        series.append((f"sync {L}", "sync", L, lambda w=win, L=L: ctx.front_end_sync(
            w.addr, B, L, ltf.addr, 0.25, 0, start.addr, metric.addr, stream=s)))
    series.append(("short_field", "field", 160, lambda: ctx.short_field(wave.addr, B, 1.0, 160, stream=s)))
    times = {x[0]: [] for x in series}
    outs = {}
    for rd in range(-1, args.rounds):   # round -1: untimed
        for name, kind, L, f in (series if rd % 2 == 0 else series[::-1]):
            for _ in range(2):
                f()
            e0, e1 = m.Event(), m.Event()
            e0.record(s)
            for _ in range(args.reps):
                f()
            e1.record(s)
            t = e0.elapsed_ms(e1) / args.reps * 1e3
            if rd >= 0:
                times[name].append(t)
            if rd == args.rounds - 1:
                outs[name] = (start.numpy(), metric.numpy(), cfo.numpy(), mstf.numpy()) if kind != "field" \
                    else (wave.numpy(),)
    print(f"{B} frames, {args.rounds} rounds x {args.reps} calls, us per call (HIP events); windows of "
          f"{' and '.join(str(L) for L in LENGTHS)} samples, offset {EPS} cycles per sample")
    for name, kind, L, _ in series:
        t = times[name]
        med = np.median(t)
        line = f"{name:14s} median {med:9.2f}  min {min(t):9.2f}  max {max(t):9.2f}"
        if kind == "field":
            line += f"  {B * 160 * 16 / med / 1e3:6.0f} GB/s written"
        else:
            t2 = -(-(L - 127) // LAGS_LTF)
            executed, useful = t2 * 64 * 8 * 64 * 8, (L - 63) * 64 * 8
            if kind == "stf":
                t1 = -(-(L - 143) // LAGS_STF)
                executed += t2 * 576 * 6 + t1 * ((576 + 64 * 16) * 9 + 64 * 8 * 2 * 3 * 2)
                useful += (L - 16) * 6
            line += (f"  {B * L * 16 / med / 1e3:6.0f} GB/s  {B * executed / med / 1e6:5.1f} TFLOP/s executed  "
                     f"{B * useful / med / 1e6:5.1f} TFLOP/s useful")
        print(line + "  runs " + " ".join(f"{x:.2f}" for x in t))
    for L in LENGTHS:
        a, b = np.median(times[f"sync_stf {L}"]), np.median(times[f"sync {L}"])
        w = np.tile(want[L], -(-B // chunk))[:B]
        s1, ml, e, ms = outs[f"sync_stf {L}"]
        s0 = outs[f"sync {L}"][0]
        print(f"L = {L}: sync_stf over sync {a / b:.2f}x; starts equal the placed positions: sync_stf "
              f"{bool(np.array_equal(s1, w))}, sync {bool(np.array_equal(s0, w))}; Ms {ms.min():.3f} .. {ms.max():.3f}, "
              f"Ml {ml.min():.3f} .. {ml.max():.3f}, |cfo - {EPS}| <= {np.max(np.abs(e - EPS)):.1e}")
    w = outs["short_field"][0]
    print(f"short_field: rows periodic and equal: {bool(np.array_equal(w[:, :144], w[:, 16:]) and np.all(w == w[0]))}")


if __name__ == "__main__":
    main()
