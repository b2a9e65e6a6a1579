"""What does combining the antenna branches cost?  One process, HIP events
(wce_event_*), interleaved series, 65,536 packets (the 67-packet branch set of
tests/combine_model.py, repeated):

  demod eq        the yardstick: wce_demodulate's eq-only build (no tracking, no
                  blend): reads rx and h, writes eq -- 2 x 12.7 KB per frame
  A<n> [ow2] both wce_combine on n branches, both outputs -- (n + 1) x (12.7 + 0.8) KB
  A<n> [ow2] rx   the combined stream alone
  A<n> [ow2] h    the combined estimate alone (reads no rx)

usage: python tools/ab_combine.py [--frames 65536] [--rounds 7] [--reps 20] [--no-link]
                                  [--out profiles/combine_65536.txt] [--label TEXT]

Each round times every series in turn (odd rounds in reverse order): 2 warm-up
calls, then `reps` calls between two events; one untimed round comes first.  Each
series is reported with its HBM rate over its own algorithmic bytes per packet and
the spread of its rounds, and with its rate over the yardstick's.  After the last
round the first and the last 67 packets, which hold the same data, are compared
bit for bit.  Then (unless --no-link) the link experiment of tests/test_combine_gpu.py
runs once per case and its bit-error counts are printed beside the fp64 model's on
the same captures.  The report is printed and appended to --out, so that repeated
processes stand below each other.
"""
import argparse
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
N, NB = 53, 15
FRAME = NB * N * 16          # 12,720 B: one packet's rx of one branch, or rx_c
ROW = N * 16                 # one estimate row
TILE = 67 * 16               # packets uploaded per branch; the rest are device copies of them
AS = (1, 2, 4)


def nbytes(A, ow2, what):
    if what == "h":
        return A * ROW + ROW + (8 * A if ow2 else 0)
    return A * (FRAME + ROW) + FRAME + (ROW if what == "both" else 0) + (8 * A if ow2 else 0)


def repeated(m, a, B):
    """host [A][67][...] -> device [A][B][...]: each branch's rows repeated"""
    lib = m.load()
    A = a.shape[0]
    d = m.DeviceArray((A, B) + a.shape[2:], a.dtype)
    row = int(np.prod(a.shape[2:], dtype=np.int64)) * a.dtype.itemsize
    for q in range(A):
        first = m.DeviceArray.from_numpy(np.ascontiguousarray(np.concatenate([a[q]] * (TILE // 67))))
        for off in range(0, B, TILE):
            n = min(TILE, B - off)
            assert lib.wce_memcpy_dtod(d.addr + (q * B + off) * row, first.addr, n * row, None) == 0
        m.synchronize()
    return d


def timing(m, ctx, cb, B, rounds, reps, say):
    D = m.DeviceArray
    tx, rx, h, ow2 = cb.branches(max(AS), loss_db=3.0 * np.arange(max(AS)))
    stream = m.Stream()
    s = stream.handle
    series, keep = [], []
    dtx = repeated(m, np.ascontiguousarray(tx[None]), B)
    for A in AS:
        drx, dh, dow2 = (repeated(m, np.ascontiguousarray(a[:A]), B) for a in (rx, h, ow2))
        orx, oh = D((B, NB, N)), D((B, N))
        keep.append((drx, dh, dow2, orx, oh))
        if A == 1:
            fr = ctx.frames(dtx, drx, B)
            series.append(("demod eq", 2 * FRAME + ROW, (orx,),
                           lambda fr=fr, dh=dh, orx=orx: ctx.demodulate(fr, dh, modulation=m.MOD_QAM16, track=False,
                                                                         ref_tx=False, eq=orx, stream=s)))
        for w in (False, True):
            for what in ("both", "rx", "h"):
                outs = (orx if what != "h" else None, oh if what != "rx" else None)
                series.append((f"A{A} {'ow2 ' if w else '    '}{what}", nbytes(A, w, what),
                               tuple(o for o in outs if o is not None),
                               lambda drx=drx, dh=dh, o2=(dow2 if w else None), A=A, outs=outs:
                               ctx.combine(drx, dh, B, A, o2, outs[0], outs[1], stream=s)))
    times = {name: [] for name, _, _, _ in series}
    for rd in range(-1, rounds):   # round -1: untimed
        for name, _, _, f in (series if rd % 2 == 0 else series[::-1]):
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
    say(f"{B} packets, {rounds} rounds x {reps} calls, us per call (HIP events)")
    yard = None
    last = (B - 67) // 67 * 67
    for name, nb, outs, f in series:
        t = times[name]
        med = np.median(t)
        rate = B * nb / med / 1e6          # TB/s
        yard = rate if yard is None else yard
        f()
        stream.synchronize()
        same = all(np.array_equal(o.rows(0, 67).view(np.uint8), o.rows(last, 67).view(np.uint8)) for o in outs)
        say(f"{name:12s} median {med:8.2f}  min {min(t):8.2f}  max {max(t):8.2f}  spread {(max(t) - min(t)) / med:6.2%}  "
            f"{nb:6d} B/packet {rate:6.3f} TB/s  {rate / yard:5.2f} of the yardstick's rate  tiles agree {bool(same)}")
    say("")


def link(m, ctx, cb, say):
    say(f"link experiment: 16-QAM rate 1/2, nominal {cb.LINK_SNR} dB, {cb.LINK_B} packets, six static taps per branch, "
        f"seed {cb.LINK_SEED:#x}; bit errors in {cb.LINK_B * 1440}: combined / each branch alone")
    for A, unequal in ((2, False), (2, True), (4, False), (4, True)):
        c = cb.link_set(A, unequal)
        front = None
        for weighted in ((True, False) if unequal else (True,)):
            res = ctx.link_mrc_host(cb.LINK_MOD, cb.LINK_RATE, cb.LINK_SNR, cb.LINK_B, A, c["taps"],
                                    sources=(m.LT_LS, m.PS_MMSE), branch_loss_db=c["loss"], weighted=weighted,
                                    cfo=c["cfo"], delay=c["delay"], capture_len=cb.LINK_LEN,
                                    threshold=cb.LINK_THRESHOLD, seed=c["seed"], keep_capture=True)
            front = front if front is not None else cb.link_front(res["capture"])
            model = cb.link_model(res["capture"], c["bits"], weighted, front=front)
            tot = lambda r: f"{int(r['combined'].sum())} / {[int(x) for x in r['branch'].sum(axis=1)]}"
            say(f"A = {A}, {'6 dB steps' if unequal else 'equal noise'}, {'weighted' if weighted else 'unweighted'}: "
                f"LT_LS {tot(res[m.LT_LS])} (fp64 model {tot(model)}, "
                f"{int((model['marginal'] | model['branch_marginal'].any(axis=0)).sum())} marginal frames), "
                f"PS_MMSE {tot(res[m.PS_MMSE])}")
    say("")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=65536)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--no-link", action="store_true")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "combine_65536.txt"))
    ap.add_argument("--label", default="process 1")
    args = ap.parse_args()
    import importlib
    m = importlib.import_module("80211parallelestimation_amd")
    import combine_model as cb
    import tx_model as tm
    with open(args.out, "a") as out:
        def say(line):
            print(line, flush=True)
            out.write(line + "\n")
            out.flush()
        say(f"---- {args.label}")
        timing(m, m.Context(empty=True), cb, args.frames, args.rounds, args.reps, say)
        if not args.no_link:
            pre = tm.chain_pre()
            link(m, m.Context(pre, pre, 1e-6, m.MMSE_TEXTBOOK), cb, say)


if __name__ == "__main__":
    main()
