"""What does decoding cost?  One process, HIP events (wce_event_*), interleaved
series on synthetic frames (wce_synth_frames), 65,536 frames by default:

  eq             the yardstick, tools/ab_demod.py's series: wce_demodulate, eq only,
                 untracked, h = the LS pass's ps_linear and h_lt = its lt_ls.  It
                 moves the 12.7 KB per frame the demapper reads
  demap m bits   wce_soft_demap of that eq as BPSK, QPSK, 16-QAM, 64-QAM (same h and
                 h_lt): 12.7 KB in, 720 m floats out
  viterbi ...    wce_viterbi_decode of those soft bits, terminated, bits and error
                 count out: BPSK 1/2, 16-QAM 1/2, 64-QAM 3/4

usage: python tools/ab_decode.py [--frames 65536] [--rounds 7] [--reps 10]

Each round times every series in turn (odd rounds in reverse order): 2 warm-up
calls, then `reps` calls between two events; one untimed round comes first.  The
demapper is reported with its HBM rate over its own algorithmic bytes; the
decoder in frames/s, decoded Mbit/s and cycles per trellis step per wave,
    time x shader clock x resident waves / (frames x T),
with the clock sampled from amd-smi while the series runs back to back
(tools/energy_bound.py's sampler; 2,400 MHz where that gives nothing) and the
resident waves = CUs x the waves per CU that the survivor memory and the 32
wave slots allow.  The kernels' time does not depend on the data: the frames
are the synthetic BPSK ones whatever the series decodes them as.
"""
import argparse
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))
N, NB = 53, 15
FRAME = NB * N * 16          # 12,720 B: one frame's rx or eq
ROW = N * 16                 # one estimate row
CUS, LDS_CU, SLOTS = 256, 160 * 1024, 32     # MI355X
MODS = {1: "BPSK", 2: "QPSK", 4: "16-QAM", 6: "64-QAM"}
RATES = {0: "1/2", 1: "2/3", 2: "3/4"}
DECODES = ((1, 0), (4, 0), (6, 2))


def resident_waves(T):
    """waves per CU of wce_viterbi_decode: 256 B of survivor memory per 32 steps per wave, workgroups of 4, 2 or 1
    waves (within 64 KiB), whichever lets the CU hold the most (launch_viterbi's choice)"""
    per_wave = (T + 31) // 32 * 256
    return max(min(SLOTS, LDS_CU // (w * per_wave) * w) for w in (4, 2, 1) if w * per_wave <= 65536)


def run(m, ctx, B, rounds, reps):
    import energy_bound
    D = m.DeviceArray
    tx, rx = D((B, NB, N)), D((B, NB, N))
    ctx.synth(tx, rx, None, B)
    lt, lin, eq = D((B, N)), D((B, N)), D((B, NB, N))
    fr = ctx.frames(tx, rx, B)
    o = m.Outputs(lt.addr, lin.addr, None, None, None, None, N, NB * N, N, m.PS_LINEAR, 0)
    stream = m.Stream()
    s = stream.handle
    ctx.estimate(fr, o, m.LT_LS | m.PS_LINEAR, stream=s)
    ctx.demodulate(fr, lin, lt, track=False, eq=eq, stream=s)
    llr = {mod: D((B, NB, 48 * mod), np.float32) for mod in MODS}
    T = {c: m.info_bits(*c) for c in DECODES}
    bits = {c: D((B, (T[c] + 7) // 8), np.uint8) for c in DECODES}
    ref = {c: D((B, (T[c] + 7) // 8), np.uint8, zero=True) for c in DECODES}
    nerr = D((B,), np.uint32)
    series = [("eq", lambda: ctx.demodulate(fr, lin, lt, track=False, eq=eq, stream=s))]
    nbytes = {"eq": 2 * FRAME + 2 * ROW}
    for mod in MODS:
        name = f"demap {mod} bits"
        series.append((name, lambda mod=mod: ctx.soft_demap(eq, lin, B, h_lt=lt, modulation=mod, llr=llr[mod], stream=s)))
        nbytes[name] = FRAME + 2 * ROW + NB * 48 * mod * 4
    for c in DECODES:
        name = f"viterbi {MODS[c[0]]} {RATES[c[1]]}"
        series.append((name, lambda c=c: ctx.viterbi_decode(llr[c[0]], B, c[0], c[1], bits=bits[c], ref_bits=ref[c],
                                                            nbiterr=nerr, stream=s)))
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
    for name, _ in series[:1 + len(MODS)]:
        t = times[name]
        print(f"{name:20s} median {med[name]:10.2f}  min {min(t):10.2f}  max {max(t):10.2f}  {nbytes[name]:6d} B/frame "
              f"{B * nbytes[name] / med[name] / 1e6:6.3f} TB/s  runs " + " ".join(f"{x:.2f}" for x in t))
    for mod in MODS:
        name = f"demap {mod} bits"
        print(f"{name} over eq: {med[name] / med['eq'] - 1.0:+.2%} in time, {nbytes[name] / nbytes['eq'] - 1.0:+.2%} "
              f"in bytes")
    for (name, f), c in zip(series[1 + len(MODS):], DECODES):
        t = times[name]
        _, mhz, ns = energy_bound.measure(stream, f, 1.5)
        clock = mhz if mhz else 2400.0
        waves = resident_waves(T[c]) * CUS
        cyc = med[name] * clock * min(waves, B) / (B * T[c])
        print(f"{name:20s} median {med[name]:10.2f}  min {min(t):10.2f}  max {max(t):10.2f}  T {T[c]:4d}  "
              f"{B / med[name]:7.3f} Mframes/s  {B * T[c] / med[name]:9.1f} decoded Mbit/s  "
              f"{cyc:6.1f} cycles per step per wave ({resident_waves(T[c])} waves per CU, {clock:.0f} MHz"
              f"{'' if mhz else ' assumed'}, {ns} samples)  runs " + " ".join(f"{x:.2f}" for x in t))
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
