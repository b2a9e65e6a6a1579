"""What does demodulation cost?  One process, HIP events (wce_event_*), interleaved
series on synthetic BPSK frames (wce_synth_frames), for each batch size:

  ls pass        the yardstick: wce_estimate with LT_LS | PS_LINEAR | WCE_EQUALIZE
                 (shared preamble), which moves the same rx and eq bytes
  eq             wce_demodulate, eq only, untracked, h = that pass's ps_linear and
                 h_lt = its lt_ls: the same equalizer
  eq tracked     the same with WCE_DEMOD_TRACK (tx at the pilots)
  everything     eq, sym, theta, evm, nerr, tracked, EVM against tx

usage: python tools/ab_demod.py [--frames 65536 1048576] [--rounds 7] [--reps 20]

Each round times every series in turn (odd rounds in reverse order): 2 warm-up
calls, then `reps` calls between two events; one untimed round comes first.  Each
series is reported with its HBM rate over its own algorithmic bytes per frame
(whole 64-byte sectors where a load touches single elements: the pilots).  After
the last round the untracked eq is compared bit for bit with the pass's eq.
"""
import argparse
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
N, NB = 53, 15
FRAME = NB * N * 16          # 12,720 B: one frame's rx, tx or eq
ROW = N * 16                 # one estimate row
BYTES = {"ls pass": 2 * FRAME + 2 * ROW + 2 * 4 * 64,               # rx, eq, lt_ls and ps_linear out, 4 pilot pairs
         "eq": 2 * FRAME + 2 * ROW,                                 # rx, eq, h and h_lt in
         "eq tracked": 2 * FRAME + 2 * ROW + NB * 4 * 64,           # + tx at the pilots, a sector each
         "everything": 3 * FRAME + 2 * ROW + NB * N + NB * 8 + 8 + 4}   # + all of tx, sym, theta, evm, nerr


def run(m, ctx, B, rounds, reps):
    D = m.DeviceArray
    tx, rx = D((B, NB, N)), D((B, NB, N))
    ctx.synth(tx, rx, None, B)
    lt, lin, eq_ls, eq = D((B, N)), D((B, N)), D((B, NB, N)), D((B, NB, N))
    sym, theta = D((B, NB, N), np.uint8), D((B, NB), np.float64)
    evm, nerr = D((B,), np.float64), D((B,), np.uint32)
    fr = ctx.frames(tx, rx, B)
    o = m.Outputs(lt.addr, lin.addr, None, None, None, eq_ls.addr, N, NB * N, N, m.PS_LINEAR, 0)
    stream = m.Stream()
    s = stream.handle
    series = [
        ("ls pass", lambda: ctx.estimate(fr, o, m.LT_LS | m.PS_LINEAR | m.EQUALIZE, stream=s)),
        ("eq", lambda: ctx.demodulate(fr, lin, lt, track=False, eq=eq, stream=s)),
        ("eq tracked", lambda: ctx.demodulate(fr, lin, lt, track=True, eq=eq, stream=s)),
        ("everything", lambda: ctx.demodulate(fr, lin, lt, track=True, ref_tx=True, eq=eq, sym=sym, theta=theta,
                                              evm=evm, nerr=nerr, stream=s)),
    ]
    series[0][1]()               # the estimates the demodulation reads
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
    print(f"{B} frames, {rounds} rounds x {reps} calls, us per call (HIP events)")
    for name, _ in series:
        t = times[name]
        med = np.median(t)
        print(f"{name:12s} median {med:9.2f}  min {min(t):9.2f}  max {max(t):9.2f}  {BYTES[name]:6d} B/frame "
              f"{B * BYTES[name] / med / 1e3:6.0f} GB/s  runs " + " ".join(f"{x:.2f}" for x in t))
    ls, med = times["ls pass"], {k: np.median(v) for k, v in times.items()}
    print(f"eq over ls pass: {med['eq'] / med['ls pass'] - 1.0:+.2%} (median over median; the pass's spread "
          f"{(max(ls) - min(ls)) / med['ls pass']:.2%})")
    print(f"eq tracked over eq: {med['eq tracked'] / med['eq'] - 1.0:+.2%} in time, "
          f"{BYTES['eq tracked'] / BYTES['eq'] - 1.0:+.2%} in bytes")
    print(f"everything over eq: {med['everything'] / med['eq'] - 1.0:+.2%} in time, "
          f"{BYTES['everything'] / BYTES['eq'] - 1.0:+.2%} in bytes")
    series[1][1]()
    stream.synchronize()
    n = min(B, 4096)
    same = np.array_equal(eq.rows(0, n).view(np.uint8), eq_ls.rows(0, n).view(np.uint8)) and \
        np.array_equal(eq.rows(B - n, n).view(np.uint8), eq_ls.rows(B - n, n).view(np.uint8))
    series[3][1]()
    stream.synchronize()
    ev, ne = evm.numpy(), nerr.numpy()
    print(f"untracked eq has the pass's bits (first and last {n} frames): {bool(same)}; evm {ev.min():.4f} .. "
          f"{ev.max():.4f}, symbol errors {int(ne.sum())} in {B * 48 * NB}")
    print()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, nargs="+", default=[65536, 1048576])
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    import importlib
    m = importlib.import_module("80211parallelestimation_amd")
    inp = np.load(os.path.join(REPO, "tests", "golden", "inputs_h.npz"))
    ctx = m.Context(inp["tx_pre"], inp["rx_pre"], float(inp["ow2"]), m.MMSE_TEXTBOOK)
    for B in args.frames:
        run(m, ctx, B, args.rounds, args.reps)


if __name__ == "__main__":
    main()
