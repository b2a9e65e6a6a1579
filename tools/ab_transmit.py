"""What does transmitting on the device cost?  One process, HIP events
(wce_event_*), interleaved series, 65,536 frames by default: a 160-sample field and
15 blocks (1,360 clean samples) into 1,488-sample capture windows through 6 taps
per frame, with an offset and noise on.

  store          the yardstick, a pure store stream: wce_reencode, x^ only (64-QAM
                 3/4, 405 B of bits in, 12,720 B out per frame), reported as measured
                 and scaled by bytes to a capture window's 23,808 B
  modulate       wce_modulate: 12,720 B of symbols in (the preamble is shared),
                 21,760 B of clean waveform out
  channel        wce_channel: the waveform in (read twice, the guard's scan and the
                 tiles; counted once), 96 B of taps and 20 B of scalars, 23,808 B out
  mod, chan      the two back to back: the clean waveform goes through memory
  transmit       wce_transmit: symbols in, capture out, the waveform stays in LDS

usage: python tools/ab_transmit.py [--frames 65536] [--rounds 7] [--reps 5]

Each round times every series in turn (odd rounds in reverse order): 2 warm-up
calls, then `reps` calls between two events; one untimed round comes first.
Every series is reported with its HBM rate over its own algorithmic bytes, and
the calls that make noise with their FP64 rate over a count of 130 flops per
sample for 16 taps' worth of FIR (here 6: 48) plus about 260 for the rotor and
Box-Muller.  The kernels' time does not depend on the data.
"""
import argparse
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
N, NB, S, L, NT = 53, 15, 1360, 1488, 6
SYM = NB * N * 16            # 12,720 B: one frame's symbols
WAVE, CAP = S * 16, L * 16   # 21,760 B and 23,808 B
PAR = NT * 16 + 8 + 8 + 4
FLOPS = L * (8 * NT + 260)   # per frame, the channel's arithmetic


def run(m, ctx, B, rounds, reps):
    D = m.DeviceArray
    rng = np.random.default_rng(0xAB)
    nby = (m.info_bits(6, 2) + 7) // 8
    bits = D.from_numpy(rng.integers(0, 256, (B, nby), dtype=np.uint8))
    sym, wave, cap = D((B, NB, N)), D((B, S)), D((B, L))
    pre = D.from_numpy(ctx.tx_pre)
    taps = D.from_numpy(m.pdp_taps(rng, B, np.exp(-np.arange(NT))))
    cfo = D.from_numpy(rng.uniform(-0.002, 0.002, B))
    ow2 = D.from_numpy(np.full(B, 1e-3))
    delay = D.from_numpy(rng.integers(0, L - S - NT, B).astype(np.int32))
    stream = m.Stream()
    s = stream.handle
    chan = dict(taps=taps, n_taps=NT, taps_stride=NT, cfo=cfo, ow2=ow2, delay=delay, stream=s)
    store = lambda: ctx.reencode(bits, B, 6, 2, tx=sym, stream=s)
    mod = lambda: ctx.modulate(sym, B, wave, tx_pre=pre, stream=s)
    ch = lambda: ctx.channel(wave, B, S, cap, L, **chan)
    series = [("store", store), ("modulate", mod), ("channel", ch), ("mod, chan", lambda: (mod(), ch())),
              ("transmit", lambda: ctx.transmit(sym, B, cap, L, tx_pre=pre, **chan))]
    nbytes = {"store": nby + SYM, "modulate": SYM + WAVE, "channel": WAVE + PAR + CAP,
              "mod, chan": SYM + 2 * WAVE + PAR + CAP, "transmit": SYM + PAR + CAP}
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
        print(f"{name:10s} median {med[name]:10.2f}  min {min(t):10.2f}  max {max(t):10.2f}  {nbytes[name]:6d} B/frame "
              f"{B * nbytes[name] / med[name] / 1e6:6.3f} TB/s  runs " + " ".join(f"{x:.2f}" for x in t))
    scaled = med["store"] * CAP / SYM
    print(f"store scaled to {CAP} B/frame: {scaled:.2f} us; transmit over it: {med['transmit'] / scaled:.2f}x; "
          f"transmit over mod, chan: {med['transmit'] / med['mod, chan'] - 1.0:+.2%}; "
          f"channel arithmetic {B * FLOPS / med['transmit'] / 1e6:.2f} TFLOP/s (FP64, counted) in transmit, "
          f"{B * FLOPS / med['channel'] / 1e6:.2f} in channel")
    stream.synchronize()
    print()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, nargs="+", default=[65536])
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    import importlib
    m = importlib.import_module("80211parallelestimation_amd")
    inp = np.load(os.path.join(REPO, "tests", "golden", "inputs_h.npz"))
    ctx = m.Context(inp["tx_pre"], inp["rx_pre"], float(inp["ow2"]), m.MMSE_TEXTBOOK)
    for B in args.frames:
        run(m, ctx, B, args.rounds, args.reps)


if __name__ == "__main__":
    main()
