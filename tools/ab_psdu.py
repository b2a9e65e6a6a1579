"""What does framing the payload cost beside the decoder?  One process, HIP events
(wce_event_*), interleaved series, 65,536 frames at the longest PSDU, for BPSK 1/2 (the
decoder's cheapest case: 45-byte rows, 8 lanes a frame) and 64-QAM 3/4 (405-byte rows,
64 lanes a frame):

  viterbi          the yardstick: wce_viterbi_decode, unterminated, bits out
  copy             the floor: wce_memcpy_dtod of the frames' ceil(T / 8) bytes
  frame            wce_psdu_frame, one length and seed for all
  frame lengths    the same with per-frame lengths and seeds
  deframe          wce_psdu_deframe, every output, one length for all
  deframe lengths  the same with per-frame lengths
  deframe flags    psdu, seed and fcs_ok without the n_good counter, one length for all

usage: python tools/ab_psdu.py [--frames 65536] [--rounds 7] [--reps 20]
                               [--out profiles/psdu_65536.txt] [--label TEXT]

Each round times every series in turn (odd rounds in reverse order): 2 warm-up calls,
then `reps` calls between two events; one untimed round comes first.  Each series is
reported with the median, the spread of its rounds and its time over the decoder's and
over the copy's.  After the last round the deframed outputs are checked: every frame
good, every seed the one sent.  The report is printed and appended to --out.
"""
import argparse
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
TILE = 1024


def tiled(m, a, B):
    """host [TILE][...] -> device [B][...]: the rows repeated"""
    lib = m.load()
    d = m.DeviceArray((B,) + a.shape[1:], a.dtype)
    row = int(np.prod(a.shape[1:], dtype=np.int64)) * a.dtype.itemsize
    first = m.DeviceArray.from_numpy(np.ascontiguousarray(a))
    for off in range(0, B, TILE):
        n = min(TILE, B - off)
        assert lib.wce_memcpy_dtod(d.addr + off * row, first.addr, n * row, None) == 0
    m.synchronize()
    return d


def timing(m, ctx, mod, rate, B, rounds, reps, say):
    lib = m.load()
    D = m.DeviceArray
    rng = np.random.default_rng(0x5D0)
    T, mx = m.info_bits(mod, rate), m.psdu_max_len(mod, rate)
    nby = (T + 7) // 8
    stream = m.Stream()
    s = stream.handle
    llr = tiled(m, rng.standard_normal((TILE, 15, 48 * mod)).astype(np.float32), B)
    pay = tiled(m, rng.integers(0, 256, (TILE, mx - 4)).astype(np.uint8), B)
    seeds = (np.arange(B) % 127 + 1).astype(np.uint8)
    dlen, dseeds = D.from_numpy(np.full(B, mx, np.int32)), D.from_numpy(seeds)
    dec, bits, copy = D((B, nby), np.uint8), D((B, nby), np.uint8, zero=True), D((B, nby), np.uint8)
    out = {"psdu": D((B, mx), np.uint8), "seed": D((B,), np.uint8), "fcs_ok": D((B,), np.uint32),
           "n_good": D((1,), np.uint32, zero=True)}
    series = [
        ("viterbi", lambda: ctx.viterbi_decode(llr, B, mod, rate, False, dec, stream=s)),
        ("copy", lambda: lib.wce_memcpy_dtod(copy.addr, bits.addr, B * nby, s)),
        ("frame", lambda: ctx.psdu_frame(pay, B, mod, rate, length=mx, seed=93, bits=bits, stream=s)),
        ("frame lengths", lambda: ctx.psdu_frame(pay, B, mod, rate, lengths=dlen, seeds=dseeds, bits=bits, stream=s)),
        ("deframe", lambda: ctx.psdu_deframe(bits, B, mod, rate, length=mx, stream=s, **out)),
        ("deframe lengths", lambda: ctx.psdu_deframe(bits, B, mod, rate, lengths=dlen, stream=s, **out)),
        ("deframe flags", lambda: ctx.psdu_deframe(bits, B, mod, rate, length=mx, stream=s,
                                                   **{k: v for k, v in out.items() if k != "n_good"})),
    ]
    series[3][1]()          # the rows the deframer reads: per-frame seeds
    stream.synchronize()
    times = {name: [] for name, _ in series}
    for rd in range(-1, rounds):   # round -1: untimed
        for name, f in (series if rd % 2 == 0 else series[::-1]):
            if name.startswith("deframe"):
                series[3][1]()
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
    say(f"modulation {mod} rate {rate}: T = {T}, {nby} B a row, PSDU {mx} octets; {B} frames, {rounds} rounds x {reps} "
        f"calls, us per call (HIP events)")
    med = {name: float(np.median(t)) for name, t in times.items()}
    for name, _ in series:
        t = times[name]
        say(f"{name:16s} median {med[name]:9.2f}  min {min(t):9.2f}  max {max(t):9.2f}  spread "
            f"{(max(t) - min(t)) / med[name]:6.2%}  {med[name] / med['viterbi']:8.4f} of the decoder  "
            f"{med[name] / med['copy']:6.2f} x the copy")
    series[3][1]()
    lib.wce_memset(out["n_good"].addr, 0, 4)
    series[5][1]()
    stream.synchronize()
    ok = bool(np.all(out["fcs_ok"].numpy() == 1) and int(out["n_good"].numpy()[0]) == B and
              np.array_equal(out["seed"].numpy(), seeds))
    say(f"every frame deframed good, with the seed it was sent with: {ok}")
    say("")
    return med


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=65536)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "psdu_65536.txt"))
    ap.add_argument("--label", default="process 1")
    args = ap.parse_args()
    import importlib
    m = importlib.import_module("80211parallelestimation_amd")
    with open(args.out, "a") as out:
        def say(line):
            print(line, flush=True)
            out.write(line + "\n")
            out.flush()
        say(f"---- {args.label}")
        ctx = m.Context(empty=True)
        for mod, rate in ((m.MOD_BPSK, m.RATE_1_2), (m.MOD_QAM64, m.RATE_3_4)):
            med = timing(m, ctx, mod, rate, args.frames, args.rounds, args.reps, say)
            worst = max(med[k] for k in med if k not in ("viterbi", "copy")) / med["viterbi"]
            say(f"the dearest of the five calls takes {worst:.4f} of the decoder's time "
                f"({'above' if worst > 0.1 else 'within'} a tenth)")
            say("")


if __name__ == "__main__":
    main()
