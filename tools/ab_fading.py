"""What do taps that move within the packet cost?  One process, one binary, HIP events
(wce_event_*), interleaved series, 65,536 frames by default: a 160-sample field and 15
blocks (1,360 clean samples) into 1,488-sample capture windows through 6 taps, with an
offset and noise on -- tools/ab_transmit.py's workload and method.

  transmit        wce_transmit with 6 static taps per frame: the yardstick
  tv constant     wce_transmit_tv, the same taps as 19 constant knots, P = 80 (the same
                  capture, bit for bit: what the per-lane taps cost and nothing else)
  tv moving       wce_transmit_tv, fading_taps' knots (rho = 0.995), P = 80
  tv shared       wce_transmit_tv, one moving trajectory for all frames (frame_stride 0)
  tv P=16         wce_transmit_tv, 87 moving knots 16 samples apart: the knots are staged
                  per tile, and most lane runs straddle a knot
  mod, chan_tv    wce_modulate then wce_channel_tv: the clean waveform goes through memory

usage: python tools/ab_fading.py [--frames 65536] [--rounds 7] [--reps 5] [--lib PATH]
                                 [--out profiles/fading_65536.txt]

Each round times every series in turn (odd rounds in reverse order): 2 warm-up calls,
then `reps` calls between two events; one untimed round comes first.  Reported: median,
minimum and maximum of the rounds, every round's figure, and each series' median over
wce_transmit's of the same run.  --lib times another build of the library (one compiled
with -DWCE_TX_KNOT_PAD=0 or -DWCE_TX_KNOT_ONCE=0, the A/B of the LDS layout and of the
staging); --out appends the report to a file."""
import argparse
import importlib
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
N, NB, S, L, NT = 53, 15, 1360, 1488, 6


def run(m, ctx, B, rounds, reps, emit):
    D = m.DeviceArray
    rng = np.random.default_rng(0xAB)
    sym, wave, cap = D((B, NB, N)), D((B, S)), D((B, L))
    ctx.reencode(D.from_numpy(rng.integers(0, 256, (B, (m.info_bits(6, 2) + 7) // 8), dtype=np.uint8)), B, 6, 2, tx=sym)
    pre = D.from_numpy(ctx.tx_pre)
    power = np.exp(-np.arange(NT))
    h = m.pdp_taps(rng, B, power)
    taps = D.from_numpy(h)
    const = D.from_numpy(np.ascontiguousarray(np.repeat(h[:, None, :], 19, axis=1)))
    moving = D.from_numpy(m.fading_taps(rng, B, power, 0.995, 19))
    k16 = (S + NT - 2) // 16 + 2
    fast = D.from_numpy(m.fading_taps(rng, B, power, 0.995 ** 0.2, k16))
    chan = dict(cfo=D.from_numpy(rng.uniform(-0.002, 0.002, B)), ow2=D.from_numpy(np.full(B, 1e-3)),
                delay=D.from_numpy(rng.integers(0, L - S - NT, B).astype(np.int32)))
    stream = m.Stream()
    s = stream.handle
    tv = lambda knots, K, P, fs: dict(knots=knots, n_knots=K, knot_period=P, n_taps=NT, knots_frame_stride=fs,
                                      stream=s, **chan)
    series = [
        ("transmit", lambda: ctx.transmit(sym, B, cap, L, tx_pre=pre, taps=taps, n_taps=NT, taps_stride=NT, stream=s,
                                          **chan)),
        ("tv constant", lambda: ctx.transmit_tv(sym, B, cap, L, tx_pre=pre, **tv(const, 19, 80, 19 * NT))),
        ("tv moving", lambda: ctx.transmit_tv(sym, B, cap, L, tx_pre=pre, **tv(moving, 19, 80, 19 * NT))),
        ("tv shared", lambda: ctx.transmit_tv(sym, B, cap, L, tx_pre=pre, **tv(moving, 19, 80, 0))),
        ("tv P=16", lambda: ctx.transmit_tv(sym, B, cap, L, tx_pre=pre, **tv(fast, k16, 16, k16 * NT))),
        ("mod, chan_tv", lambda: (ctx.modulate(sym, B, wave, tx_pre=pre, stream=s),
                                  ctx.channel_tv(wave, B, S, cap, L, **tv(moving, 19, 80, 19 * NT)))),
    ]
    for _, f in series:
        f()
    stream.synchronize()
    times = {name: [] for name, _ in series}
    for rd in range(-1, rounds):   # round -1: untimed
        for name, f in (series if rd % 2 == 0 else series[::-1]):
            for _ in range(2):
                f()
            e0, e1 = m.Event(), m.Event()
            e0.record(s)
            for _ in range(reps):
                f()
            e1.record(s)
            t = e0.elapsed_ms(e1) / reps * 1e3
            if rd >= 0:
                times[name].append(t)
    emit(f"{B} frames, {rounds} rounds x {reps} calls, us per call (HIP events)")
    med = {k: float(np.median(v)) for k, v in times.items()}
    for name, _ in series:
        t = times[name]
        emit(f"{name:13s} median {med[name]:9.2f}  min {min(t):9.2f}  max {max(t):9.2f}  "
             f"over transmit {med[name] / med['transmit']:5.3f}x  runs " + " ".join(f"{x:.2f}" for x in t))
    stream.synchronize()
    emit("")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, nargs="+", default=[65536])
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--lib", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    m = importlib.import_module("80211parallelestimation_amd")
    if args.lib:
        m.load(args.lib)
    lines = []

    def emit(line):
        print(line, flush=True)
        lines.append(line)
    emit(f"tools/ab_fading.py, library {os.path.relpath(args.lib, REPO) if args.lib else 'libwce.so'}")
    inp = np.load(os.path.join(REPO, "tests", "golden", "inputs_h.npz"))
    ctx = m.Context(inp["tx_pre"], inp["rx_pre"], float(inp["ow2"]), m.MMSE_TEXTBOOK)
    for B in args.frames:
        run(m, ctx, B, args.rounds, args.reps, emit)
    if args.out:
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
