"""What does decision-directed estimation cost?  One process, HIP events
(wce_event_*), interleaved series on synthetic frames (wce_synth_frames), 65,536
frames by default:

  eq             the yardstick, tools/ab_demod.py's series: wce_demodulate, eq only,
                 untracked, h = the LS pass's ps_linear and h_lt = its lt_ls, on the
                 same rx.  It moves 27,136 B per frame
  tx  m r        wce_reencode, x^ only (802.11's pilots): ceil(T / 8) B of bits in,
                 12,720 B out; BPSK 1/2 and 64-QAM 3/4
  h   m r        wce_reencode, H_dd only, theta given: the bits, 120 B of theta and
                 12,720 B of rx in, 848 B out
  tx+h m r       one call with both outputs
  tx, h m r      the x^-only call and the H_dd-only call back to back: what "write
                 tx, then estimate" costs in launches, without even re-reading x^

usage: python tools/ab_reencode.py [--frames 65536] [--rounds 7] [--reps 10]

Each round times every series in turn (odd rounds in reverse order): 2 warm-up
calls, then `reps` calls between two events; one untimed round comes first.
Every series is reported with its HBM rate over its own algorithmic bytes.  The
kernel's time does not depend on the data: the bits are random bytes and theta
is what a tracked wce_demodulate of the synthetic frames gives.
"""
import argparse
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
N, NB = 53, 15
FRAME = NB * N * 16          # 12,720 B: one frame's rx, eq or x^
ROW = N * 16                 # one estimate row
THETA = NB * 8
MODS = {1: "BPSK", 2: "QPSK", 4: "16-QAM", 6: "64-QAM"}
RATES = {0: "1/2", 1: "2/3", 2: "3/4"}
CASES = ((1, 0), (6, 2))


def run(m, ctx, B, rounds, reps):
    D = m.DeviceArray
    tx, rx = D((B, NB, N)), D((B, NB, N))
    ctx.synth(tx, rx, None, B)
    lt, lin, eq, theta = D((B, N)), D((B, N)), D((B, NB, N)), D((B, NB), np.float64)
    fr = ctx.frames(tx, rx, B)
    fr_rx = ctx.frames(None, rx, B)          # no tx: 802.11's pilots, nothing of tx is read
    o = m.Outputs(lt.addr, lin.addr, None, None, None, None, N, NB * N, N, m.PS_LINEAR, 0)
    stream = m.Stream()
    s = stream.handle
    ctx.estimate(fr, o, m.LT_LS | m.PS_LINEAR, stream=s)
    ctx.demodulate(fr, lin, lt, track=True, theta=theta, stream=s)
    rng = np.random.default_rng(0xAB)
    xh, hdd = D((B, NB, N)), D((B, N))
    series = [("eq", lambda: ctx.demodulate(fr, lin, lt, track=False, eq=eq, stream=s))]
    nbytes = {"eq": 2 * FRAME + 2 * ROW}
    keep = []
    for c in CASES:
        nby = (m.info_bits(*c) + 7) // 8
        bits = D.from_numpy(rng.integers(0, 256, (B, nby), dtype=np.uint8))
        keep.append(bits)
        tag = f"{MODS[c[0]]} {RATES[c[1]]}"
        tx_only = lambda c=c, bits=bits: ctx.reencode(bits, B, c[0], c[1], tx=xh, stream=s)
        h_only = lambda c=c, bits=bits: ctx.reencode(bits, B, c[0], c[1], theta=theta, frames=fr_rx, h=hdd, stream=s)
        both = lambda c=c, bits=bits: ctx.reencode(bits, B, c[0], c[1], theta=theta, frames=fr_rx, tx=xh, h=hdd,
                                                  stream=s)
        series += [(f"tx {tag}", tx_only), (f"h {tag}", h_only), (f"tx+h {tag}", both),
                   (f"tx, h {tag}", lambda a=tx_only, b=h_only: (a(), b()))]
        nbytes[f"tx {tag}"] = nby + FRAME
        nbytes[f"h {tag}"] = nby + THETA + FRAME + ROW
        nbytes[f"tx+h {tag}"] = nby + THETA + 2 * FRAME + ROW
        nbytes[f"tx, h {tag}"] = nbytes[f"tx {tag}"] + nbytes[f"h {tag}"]
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
    print(f"{B} frames, {rounds} rounds x {reps} calls, us per call (HIP events)")
    med = {k: float(np.median(v)) for k, v in times.items()}
    for name, _ in series:
        t = times[name]
        print(f"{name:18s} median {med[name]:10.2f}  min {min(t):10.2f}  max {max(t):10.2f}  {nbytes[name]:6d} B/frame "
              f"{B * nbytes[name] / med[name] / 1e6:6.3f} TB/s  runs " + " ".join(f"{x:.2f}" for x in t))
    for c in CASES:
        tag = f"{MODS[c[0]]} {RATES[c[1]]}"
        print(f"h {tag} over eq: {med[f'h {tag}'] / med['eq'] - 1.0:+.2%} in time, "
              f"{nbytes[f'h {tag}'] / nbytes['eq'] - 1.0:+.2%} in bytes; over tx then h: "
              f"{med[f'h {tag}'] / med[f'tx, h {tag}'] - 1.0:+.2%} in time; tx+h over tx then h: "
              f"{med[f'tx+h {tag}'] / med[f'tx, h {tag}'] - 1.0:+.2%} in time")
    stream.synchronize()
    print()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, nargs="+", default=[65536])
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=10)
    args = ap.parse_args()
    import importlib
    m = importlib.import_module("80211parallelestimation_amd")
    inp = np.load(os.path.join(REPO, "tests", "golden", "inputs_h.npz"))
    ctx = m.Context(inp["tx_pre"], inp["rx_pre"], float(inp["ow2"]), m.MMSE_TEXTBOOK)
    for B in args.frames:
        run(m, ctx, B, args.rounds, args.reps)


if __name__ == "__main__":
    main()
