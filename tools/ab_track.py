"""What does tracking the channel through the packet cost?  One process, HIP events
(wce_event_*), interleaved series, 65,536 frames of each modulation (the 67-frame
drifting sets of tests/track_model.py, repeated), mu = 0.5, beta = 2, phase on:

  demodulate     the yardstick: wce_demodulate, tracked, eq, sym, theta, evm and nerr,
                 EVM against tx, h with no h_lt
  track all      wce_track_demodulate with those five and h_blocks and h_last
  track eq       eq only
  track h_blocks h_blocks only

usage: python tools/ab_track.py [--frames 65536] [--rounds 7] [--reps 20]
                                [--out profiles/track_65536.txt] [--label TEXT]

Each round times every series in turn (odd rounds in reverse order): 2 warm-up
calls, then `reps` calls between two events; one untimed round comes first.  Each
series is reported with its HBM rate over its own algorithmic bytes per frame
(whole 64-byte sectors where a load touches single elements: the pilots) and the
spread of its rounds; "track all over demodulate" is median over median.  After
the last round the first and the last 67 frames, which hold the same data, are
compared bit for bit and the symbol errors are counted.  The report is printed
and appended to --out, so that repeated processes stand below each other.
"""
import argparse
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
N, NB = 53, 15
FRAME = NB * N * 16          # 12,720 B: one frame's rx, tx, eq or h_blocks
ROW = N * 16                 # one estimate row
PILOT_TX = NB * 4 * 64       # tx at the pilots, a sector each
SCORES = NB * N + NB * 8 + 8 + 4   # sym, theta, evm, nerr
BYTES = {"demodulate": 3 * FRAME + ROW + SCORES,                    # rx, tx, eq, h
         "track all": 4 * FRAME + 2 * ROW + SCORES,                 # + h_blocks, h_last
         "track eq": 2 * FRAME + ROW + PILOT_TX,
         "track h_blocks": 2 * FRAME + ROW + PILOT_TX}
TILE = 67 * 16               # frames uploaded; the rest are device copies of them


def repeated(m, a, B):
    """host [67][...] -> device [B][...]: the rows repeated"""
    lib = m.load()
    tile = np.ascontiguousarray(np.concatenate([a] * (TILE // 67)))
    d = m.DeviceArray((B,) + a.shape[1:], a.dtype)
    step = tile.nbytes
    first = m.DeviceArray.from_numpy(tile)
    for off in range(0, B, TILE):
        n = min(TILE, B - off)
        assert lib.wce_memcpy_dtod(d.addr + off * (step // TILE), first.addr, n * (step // TILE), None) == 0
    m.synchronize()
    return d


def run(m, ctx, tm, mod, B, rounds, reps, say):
    D = m.DeviceArray
    tx, rx, h = (repeated(m, np.ascontiguousarray(a, np.complex128), B) for a in tm.drifting_set(mod))
    eq, hb, hl = D((B, NB, N)), D((B, NB, N)), D((B, N))
    sym, theta = D((B, NB, N), np.uint8), D((B, NB), np.float64)
    evm, nerr = D((B,), np.float64), D((B,), np.uint32)
    fr = ctx.frames(tx, rx, B)
    stream = m.Stream()
    s = stream.handle
    five = dict(eq=eq, sym=sym, theta=theta, evm=evm, nerr=nerr)
    trk = lambda **o: ctx.track_demodulate(fr, h, tm.MU, tm.BETA, modulation=mod, stream=s, **o)
    series = [
        ("demodulate", lambda: ctx.demodulate(fr, h, modulation=mod, track=True, ref_tx=True, stream=s, **five)),
        ("track all", lambda: trk(h_blocks=hb, h_last=hl, **five)),
        ("track eq", lambda: trk(eq=eq)),
        ("track h_blocks", lambda: trk(h_blocks=hb)),
    ]
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
    say(f"{mod} bits per symbol, {B} frames, mu {tm.MU}, beta {tm.BETA}, {rounds} rounds x {reps} calls, "
        f"us per call (HIP events)")
    for name, _ in series:
        t = times[name]
        med = np.median(t)
        say(f"{name:14s} median {med:9.2f}  min {min(t):9.2f}  max {max(t):9.2f}  spread "
            f"{(max(t) - min(t)) / med:6.2%}  {BYTES[name]:6d} B/frame {B * BYTES[name] / med / 1e3:6.0f} GB/s  runs "
            + " ".join(f"{x:.2f}" for x in t))
    med = {k: np.median(v) for k, v in times.items()}
    say(f"track all over demodulate: {med['track all'] / med['demodulate']:.3f} in time, "
        f"{BYTES['track all'] / BYTES['demodulate']:.3f} in bytes; track eq over track all "
        f"{med['track eq'] / med['track all']:.3f}, track h_blocks over track all "
        f"{med['track h_blocks'] / med['track all']:.3f}")
    series[0][1]()
    stream.synchronize()
    static = int(nerr.numpy().sum())
    series[1][1]()
    stream.synchronize()
    last = (B - 67) // 67 * 67
    same = all(np.array_equal(a.rows(0, 67).view(np.uint8), a.rows(last, 67).view(np.uint8))
               for a in (eq, hb, hl, sym, theta, evm, nerr))
    say(f"frames 0..66 and {last}..{last + 66} agree bit for bit: {bool(same)}; symbol errors in {B * 48 * NB}: "
        f"static {static}, tracked {int(nerr.numpy().sum())}")
    say("")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=65536)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "track_65536.txt"))
    ap.add_argument("--label", default="process 1")
    args = ap.parse_args()
    import importlib
    m = importlib.import_module("80211parallelestimation_amd")
    import track_model as tm
    ctx = m.Context(empty=True)
    with open(args.out, "a") as out:
        def say(line):
            print(line, flush=True)
            out.write(line + "\n")
            out.flush()
        say(f"---- {args.label}")
        for mod, _ in tm.SETS:
            run(m, ctx, tm, mod, args.frames, args.rounds, args.reps, say)


if __name__ == "__main__":
    main()
