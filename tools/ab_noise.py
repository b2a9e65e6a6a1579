"""Does the headline pay for per-frame noise?  Interleaved A/B of two libwce.so
builds on wce_estimate(PS_MMSE), TEXTBOOK, one process, HIP events
(wce_event_*), plus wce_estimate_noise on the second build at the same size.

usage: python tools/ab_noise.py PARENT_DIR NEW_DIR [--frames 65536] [--rounds 7] [--reps 200]

PARENT_DIR/libwce.so: the parent commit's build (no wce_estimate_noise);
NEW_DIR/libwce.so: this tree's.  Each round times, in turn, the parent's
headline, the new build's headline and the new build's noise request (odd
rounds in the reverse order): 3 warm-up calls, then `reps` calls between two
events; one untimed round comes first.  The verdict line says whether the new
headline's median lies inside the spread (min..max) of the parent's runs.
Every series reads the same device buffers (one allocation, synthetic frames of
seed 0x80211) and writes the same H, so buffer placement is not part of the
comparison; each series' output is read back after its last round: the two
headlines are compared bit for bit, and the noise request with ow2[:] = the
context's ow2 against them too.
"""
import argparse
import ctypes
import importlib.util
import os

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, NB = 53, 15


def load(d):
    spec = importlib.util.spec_from_file_location("wce_" + os.path.basename(d.rstrip("/")),
                                                  os.path.join(REPO, "80211parallelestimation_amd", "wce.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    path = os.path.join(d, "libwce.so")
    probe = ctypes.CDLL(path)
    m.ABI = {k: v for k, v in m.ABI.items() if hasattr(probe, k)}   # an older build lacks the newer entry points
    m._lib = None
    m.load(path)
    return m


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("parent")
    ap.add_argument("new")
    ap.add_argument("--frames", type=int, default=65536)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=200)
    args = ap.parse_args()
    n = args.frames
    inp = dict(np.load(os.path.join(REPO, "tests", "golden", "inputs_h.npz")))
    series, outs, keep = [], {}, []
    tx = rx = H = ow2 = None
    for tag, d in (("new", args.new), ("parent", args.parent)):
        m = load(d)
        st = m.Stream()
        ctx = m.Context(inp["tx_pre"], inp["rx_pre"], inp["ow2"], m.MMSE_TEXTBOOK)
        if tx is None:   # one set of buffers for every series (device pointers are the process's, not a library's)
            tx, rx, H = m.DeviceArray((n, NB, N)), m.DeviceArray((n, NB, N)), m.DeviceArray((n, N), zero=True)
            ow2 = m.DeviceArray.from_numpy(np.full(n, float(inp["ow2"]), np.float64))
            ctx.synth(tx, rx, None, n, seed=0x80211)
            m.synchronize()
        fr = ctx.frames(tx.addr, rx.addr, n)
        o = m.Outputs(None, None, None, None, H.addr, None, N, 0, 0, 0, 0)
        keep += [ctx, fr, o, st]
        series.append((f"{tag} wce_estimate", m, st,
                       (lambda c, fr, o, st, m: lambda: c.estimate(fr, o, m.PS_MMSE, st.handle))(ctx, fr, o, st, m)))
        if tag == "new":
            series.append(("new wce_estimate_noise", m, st,
                           (lambda c, fr, o, st, m, w: lambda: c.estimate(fr, o, m.PS_MMSE, st.handle, ow2=w))(
                               ctx, fr, o, st, m, ow2.addr)))
    series = [series[2], series[0], series[1]]   # parent, new, new + noise
    times = {s[0]: [] for s in series}
    for rd in range(-1, args.rounds):   # round -1: untimed
        for name, m, st, f in (series if rd % 2 == 0 else series[::-1]):
            for _ in range(3):
                f()
            e0, e1 = m.Event(), m.Event()
            e0.record(st.handle)
            for _ in range(args.reps):
                f()
            e1.record(st.handle)
            t = e0.elapsed_ms(e1) / args.reps * 1e3
            if rd >= 0:
                times[name].append(t)
            if rd == args.rounds - 1:
                outs[name] = H.numpy()
    print(f"PS_MMSE TEXTBOOK, {n} frames, {args.rounds} rounds x {args.reps} calls, us per call (HIP events)")
    for name in times:
        t = times[name]
        print(f"{name:24s} median {np.median(t):8.2f}  min {min(t):8.2f}  max {max(t):8.2f}  runs " +
              " ".join(f"{x:.2f}" for x in t))
    p, q, z = times["parent wce_estimate"], times["new wce_estimate"], times["new wce_estimate_noise"]
    inside = min(p) <= np.median(q) <= max(p)
    print(f"new headline median {np.median(q):.2f} us inside the parent's spread [{min(p):.2f}, {max(p):.2f}]: {inside}"
          f" (below it: {bool(np.median(q) < min(p))})")
    print(f"wce_estimate_noise over the new headline: {np.median(z) / np.median(q) - 1.0:+.2%} (median over median)")
    ref = outs["parent wce_estimate"]
    for name in ("new wce_estimate", "new wce_estimate_noise"):
        print(f"{name}: same bits as the parent's headline: {bool(np.array_equal(outs[name], ref))}; "
              f"non-finite frames {int(np.sum(~np.isfinite(outs[name]).all(1)))}")


if __name__ == "__main__":
    main()
