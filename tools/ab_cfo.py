"""Does the front end pay for the CFO builds?  Interleaved A/B of two libwce.so
builds on wce_front_end_blocks and wce_front_end_preamble, one process, HIP
events (wce_event_*), plus the new build's wce_front_end_blocks_cfo and
wce_front_end_preamble_cfo (estimate, then given) at the same size.

usage: python tools/ab_cfo.py PARENT_DIR NEW_DIR [--frames 65536] [--rounds 7] [--reps 20]

PARENT_DIR/libwce.so: the parent commit's build (no CFO entry points);
NEW_DIR/libwce.so: this tree's.  Each round times every series in turn (odd
rounds with each parent / new pair swapped): 2 warm-up calls, then `reps` calls
between two events; one untimed round comes first.  PARENT_DIR given twice is
the null experiment: what the two slots differ by on one and the same build.  The verdict lines say whether the new
build's plain calls lie inside the spread (min..max) of the parent's runs.
Every series reads the same device buffers (random samples of seed 0, every
frame with an offset of its own in +-1/128 cycles per sample) and writes the
same outputs, so buffer placement is not part of the comparison.  Each series'
output is read back after its last round: the plain calls of the two builds are
compared bit for bit, and the CFO calls are checked for finite output.
"""
import argparse
import ctypes
import importlib.util
import os

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, NB, L = 53, 15, 160


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
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    B = args.frames
    rng = np.random.default_rng(0)
    chunk = min(4096, B)
    pk_h = (rng.standard_normal((chunk, NB * 80)) + 1j * rng.standard_normal((chunk, NB * 80))) * 0.01
    lt_h = (rng.standard_normal((chunk, L)) + 1j * rng.standard_normal((chunk, L))) * 0.01
    mods = {"parent": load(args.parent), "new": load(args.new)}
    m = mods["new"]
    pk, lt = m.DeviceArray((B, NB * 80)), m.DeviceArray((B, L))
    lib = m.load()
    for off in range(0, B, chunk):
        k = min(chunk, B - off)
        assert lib.wce_memcpy_htod(pk.addr + off * NB * 80 * 16, pk_h[:k].ctypes.data, k * NB * 80 * 16) == 0
        assert lib.wce_memcpy_htod(lt.addr + off * L * 16, lt_h[:k].ctypes.data, k * L * 16) == 0
    sym, pre, ow2 = m.DeviceArray((B, NB, N)), m.DeviceArray((B, N)), m.DeviceArray((B,), np.float64)
    given = m.DeviceArray.from_numpy(rng.uniform(-1 / 128, 1 / 128, B))
    est = m.DeviceArray((B,), np.float64, zero=True)
    series, keep = [], []
    for tag, mod in mods.items():
        ctx, st = mod.Context(empty=True), mod.Stream()
        keep += [ctx, st]
        s = st.handle
        series.append((f"{tag} blocks", "blocks", mod, st,
                       lambda c=ctx, s=s: c.front_end_blocks(pk.addr, B, NB, sym.addr, stream=s)))
        series.append((f"{tag} preamble", "preamble", mod, st,
                       lambda c=ctx, s=s: c.front_end_preamble(lt.addr, B, L, pre.addr, ow2.addr, stream=s)))
        if tag == "new" and "wce_front_end_blocks_cfo" in mod.ABI:   # absent: a null A/B of one build against itself
            series.append(("new blocks_cfo", "blocks", mod, st,
                           lambda c=ctx, s=s: c.front_end_blocks(pk.addr, B, NB, sym.addr, stream=s, cfo=given.addr)))
            series.append(("new preamble_cfo estimate", "preamble", mod, st,
                           lambda c=ctx, s=s: c.front_end_preamble(lt.addr, B, L, pre.addr, ow2.addr, stream=s,
                                                                   cfo=est.addr)))
            series.append(("new preamble_cfo given", "preamble", mod, st,
                           lambda c=ctx, s=s: c.front_end_preamble(lt.addr, B, L, pre.addr, ow2.addr, stream=s,
                                                                   cfo=given.addr, estimate_cfo=False)))
    # parent and new side by side for each plain call, the CFO calls last; odd rounds swap each pair and
    # reverse the CFO calls, so that neither build's series always follows the same neighbour
    by = {s[0]: s for s in series}
    pairs = [by[f"{t} {k}"] for k in ("blocks", "preamble") for t in ("parent", "new")]
    extra = [s for s in series if s not in pairs]
    even = pairs + extra
    odd = [pairs[1], pairs[0], pairs[3], pairs[2]] + extra[::-1]
    series = even
    times = {s[0]: [] for s in series}
    outs = {}
    for rd in range(-1, args.rounds):   # round -1: untimed
        for name, kind, mod, st, f in (even if rd % 2 == 0 else odd):
            for _ in range(2):
                f()
            e0, e1 = mod.Event(), mod.Event()
            e0.record(st.handle)
            for _ in range(args.reps):
                f()
            e1.record(st.handle)
            t = e0.elapsed_ms(e1) / args.reps * 1e3
            if rd >= 0:
                times[name].append(t)
            if rd == args.rounds - 1:
                outs[name] = (sym.numpy(),) if kind == "blocks" else (pre.numpy(), ow2.numpy())
    nbytes = {"blocks": B * NB * (1024 + 848), "preamble": B * (2048 + 848 + 8)}
    print(f"front end, {B} frames x {NB} blocks + {L}-sample LTF, {args.rounds} rounds x {args.reps} calls, "
          f"us per call (HIP events)")
    for name, kind, *_ in series:
        t = times[name]
        print(f"{name:26s} median {np.median(t):8.2f}  min {min(t):8.2f}  max {max(t):8.2f}  "
              f"{nbytes[kind] / np.median(t) / 1e3:6.0f} GB/s  runs " + " ".join(f"{x:.2f}" for x in t))
    for kind in ("blocks", "preamble"):
        p, q = times[f"parent {kind}"], times[f"new {kind}"]
        print(f"new {kind} median {np.median(q):.2f} us inside the parent's spread [{min(p):.2f}, {max(p):.2f}]: "
              f"{bool(min(p) <= np.median(q) <= max(p))} (below it: {bool(np.median(q) < min(p))}); "
              f"same bits as the parent's: "
              f"{all(np.array_equal(a, b) for a, b in zip(outs[f'new {kind}'], outs[f'parent {kind}']))}")
    for name, base in (("new blocks_cfo", "new blocks"), ("new preamble_cfo estimate", "new preamble"),
                       ("new preamble_cfo given", "new preamble")):
        if name not in times:
            continue
        p = times[base]
        z = np.median(times[name])
        print(f"{name} over {base}: {z / np.median(p) - 1.0:+.2%} (median over median; the plain call's spread "
              f"{(max(p) - min(p)) / np.median(p):.2%}); all finite: {all(bool(np.isfinite(a).all()) for a in outs[name])}")


if __name__ == "__main__":
    main()
