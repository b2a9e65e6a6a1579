"""tests/golden/mmse_routes.json: the kernels one wce_estimate call launches,
for every combination of the facts the dispatch consults.

Two steps, the first on an MI355X, the second anywhere:

    rocprofv3 --kernel-trace --output-format csv -d OUT -o run -- \
        python tests/golden/make_mmse_routes.py walk OUT/requests.json
    python tests/golden/make_mmse_routes.py cut OUT/requests.json OUT/**/run_kernel_trace.csv \
        --commit <hash of the walked tree> [--out tests/golden/mmse_routes.json]

`walk` makes one valid wce_estimate call per combination on 5 seeded frames
(20 units in MATLAB semantics: every chunk loop runs once and the size-dependent
choices inside the launchers sit on their small-batch side) and launches
wce_nonfinite_scan on a 1-frame buffer after each as a separator; no route
launches that kernel.  It writes the requests, in order, with the status each
call returned.  `cut` orders the trace's kernels by start time, drops the
runtime's own fill kernels, cuts at the separators and writes the fixture.

The walk uses the public API and the debug switches only, so it runs
unchanged on any commit: tests/test_route.py compares the planner
(wce_debug_route) with the recorded table, and two walks of two commits
compare row by row (`cut` of each, then `diff`).

Combinations that cannot differ are walked once: the border dot only on REF
and TEXTBOOK contexts, the modulus only on COV contexts, the fusion switch
only where a C-semantics request asks for LS outputs, WCE_OUT_LS_F32 only
where FRAME_COV meets LT_LS (the one place the output format decides a
launch), variant R1 only on TEXTBOOK or FRAME_COV, REF_FC only on FRAME_COV in
C semantics, REF_LS only on REF in C semantics.
"""
import argparse
import csv
import ctypes
import importlib
import itertools
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
N, NBLK, B = 53, 15, 5
A = 8.8753
SEPARATOR = "nonfinite_scan_kernel"
FACTS = ("mode", "bdot", "fuse", "cm", "lr_k0", "rank", "sem", "mask", "f32", "r1", "ref_fc", "ref_ls")
V_REF_LS, V_REF_FC, V_R1 = 2, 4, 5


def pdp_rhh(L, decay):
    p = np.exp(-decay * np.arange(L))
    R = np.zeros((N, N), np.complex128)
    R[np.arange(L), np.arange(L)] = p / p.sum() * 1.1e-4
    return R


def requests(wce):
    """every (context name, facts) to walk, in order"""
    PS, LT, FC = wce.PS_MMSE, wce.LT_LS, wce.FRAME_COV
    masks = [m | f for m in (PS, LT | PS, wce.LS_ALL | PS, wce.ALL) for f in (0, FC)]
    out = []
    for name in ("ref", "textbook", "cov_dense", "cov_lr4", "cov_lr16", "cov_dense_cm", "cov_lr4_cm", "cov_lr16_cm"):
        shared = name in ("ref", "textbook")
        for bdot, cm, sem, mask in itertools.product((1, 0) if shared else (1,), (1, 0) if name.endswith("_cm") else (0,),
                                                     (wce.SEM_C, wce.SEM_MATLAB), masks):
            ls = bool(mask & (wce.LS_ALL | wce.EQUALIZE))
            c_sem = sem == wce.SEM_C
            fuses = (1, 0) if ls and c_sem else (1,)
            f32s = (0, 1) if (mask & FC) and (mask & LT) else (0,)
            r1s = (0, 1, 2) if name == "textbook" or (mask & FC) else (0,)
            fcs = (0, 1) if (mask & FC) and c_sem else (0,)
            lss = (0, 1) if name == "ref" and c_sem else (0,)
            for fuse, f32, r1, rfc, rls in itertools.product(fuses, f32s, r1s, fcs, lss):
                out.append(dict(ctx=name, bdot=bdot, fuse=fuse, cm=cm, sem=sem, mask=mask, f32=f32, r1=r1, ref_fc=rfc,
                                ref_ls=rls))
    return out


def walk(path):
    sys.path.insert(0, REPO)
    wce = importlib.import_module("80211parallelestimation_amd")
    lib = wce.load()
    inp = dict(np.load(os.path.join(HERE, "inputs_h.npz")))
    tp, rp, ow2 = inp["tx_pre"], inp["rx_pre"], float(inp["ow2"])
    rng = np.random.default_rng(0x20075)
    tx = rng.choice([-A, A], (B, NBLK, N)).astype(np.complex128)   # BPSK: frames the constant-modulus operator takes
    tx[:, :, 26] = 0
    h = 0.01 * (rng.standard_normal((B, 1, N)) + 1j * rng.standard_normal((B, 1, N)))
    rx = h * tx + np.sqrt(ow2 / 2) * (rng.standard_normal(tx.shape) + 1j * rng.standard_normal(tx.shape))
    pre = h[:, 0] * tp + np.sqrt(ow2 / 2) * (rng.standard_normal((B, N)) + 1j * rng.standard_normal((B, N)))
    dev = wce.DeviceArray.from_numpy
    dtx, drx, dpre, dtp = dev(tx), dev(rx), dev(pre), dev(np.asarray(tp, np.complex128))

    rhh = {"cov_dense": pdp_rhh(53, 0.12), "cov_lr4": pdp_rhh(4, 0.5), "cov_lr16": pdp_rhh(16, 0.5)}
    ctxs, facts = {}, {}
    for name, mode in (("ref", wce.MMSE_REF), ("textbook", wce.MMSE_TEXTBOOK)):
        ctxs[name] = wce.Context(tp, rp, ow2, mode)
        facts[name] = dict(mode=mode, lr_k0=-1, rank=0)
    for name, R in rhh.items():
        _, rank, k0, _, _ = wce.cov_factor(wce.state_blob(tp, rp, ow2, Rhh=R))
        for suffix in ("", "_cm"):
            c = ctxs[name + suffix] = wce.Context(tp, rp, ow2, Rhh=R)
            assert c.cov_info()[:2] == (rank, k0 >= 0)
            if suffix:
                c.set_modulus(tx[0, 0])
            facts[name + suffix] = dict(mode=wce.MMSE_COV, lr_k0=k0, rank=rank)

    outs = {f32: {n: wce.DeviceArray((B, N), np.complex64 if f32 and n != "ps_mmse" else np.complex128, zero=True)
                  for n in ("lt_ls", "ps_linear", "ps_cubic", "ps_sinc", "ps_mmse")} for f32 in (0, 1)}
    eqs = {f32: wce.DeviceArray((B, NBLK, N), np.complex64 if f32 else np.complex128, zero=True) for f32 in (0, 1)}
    sep = wce.DeviceArray((1, N), zero=True)
    bitmap, n_bad = wce.DeviceArray((1,), np.uint32), wce.DeviceArray((1,), np.uint64)
    bits = (("lt_ls", wce.LT_LS), ("ps_linear", wce.PS_LINEAR), ("ps_cubic", wce.PS_CUBIC), ("ps_sinc", wce.PS_SINC),
            ("ps_mmse", wce.PS_MMSE))
    rows = []
    try:
        for q in requests(wce):
            c = ctxs[q["ctx"]]
            c.set_border_dot(bool(q["bdot"]))
            c.set_fusion(bool(q["fuse"]))
            if q["ctx"].endswith("_cm"):
                c.set_cm(bool(q["cm"]))
            for which, key in ((V_R1, "r1"), (V_REF_FC, "ref_fc"), (V_REF_LS, "ref_ls")):
                assert lib.wce_debug_set_variant(which, q[key]) == 0
            o = outs[q["f32"]]
            out = wce.Outputs(*[(o[n].addr if q["mask"] & bit else None) for n, bit in bits],
                              eqs[q["f32"]].addr if q["mask"] & wce.EQUALIZE else None, N, NBLK * N, N, wce.PS_LINEAR,
                              wce.OUT_LS_F32 if q["f32"] else 0)
            fr = c.frames(dtx, drx, B, rx_pre=dpre, tx_pre=dtp, semantics=q["sem"])
            rc = lib.wce_estimate(c.handle, ctypes.byref(fr), ctypes.byref(out), q["mask"], None)
            c.nonfinite_scan(sep, 1, bitmap=bitmap, n_bad=n_bad)
            wce.synchronize()
            rows.append([{**facts[q["ctx"]], **q}[k] for k in FACTS] + [rc])
    finally:
        for which in (V_R1, V_REF_FC, V_REF_LS):
            lib.wce_debug_set_variant(which, 0)
    with open(path, "w") as f:
        json.dump(rows, f)
    print(f"walked {len(rows)} requests, {sum(1 for r in rows if r[-1])} rejected")


def kernel_name(raw):
    """'void wce::k<true, 1>(wce::State const*, ...) [clone .kd]' -> 'k<true, 1>'"""
    s = raw.split(" [clone")[0].strip()
    if s.endswith(".kd"):
        s = s[:-3]
    depth, cut = 0, len(s)
    for i in range(len(s) - 1, -1, -1):   # drop the parameter list: the last top-level (...) group
        if s[i] == ")":
            depth += 1
        elif s[i] == "(":
            depth -= 1
            if depth == 0:
                cut = i
                break
    s = s[:cut] if s.endswith(")") else s
    depth, start = 0, 0
    for i, ch in enumerate(s):   # drop the return type: up to the last top-level space
        depth += ch in "<("
        depth -= ch in ">)"
        if ch == " " and depth == 0:
            start = i + 1
    s = s[start:]
    return s[5:] if s.startswith("wce::") else s


def cut(requests_path, trace_path, commit, out_path):
    rows = json.load(open(requests_path))
    with open(trace_path, newline="") as f:
        recs = sorted(csv.DictReader(f), key=lambda r: int(r["Start_Timestamp"]))
    names = [kernel_name(r["Kernel_Name"]) for r in recs]
    names = [n for n in names if not n.startswith("__amd_rocclr")]   # hipMemsetAsync of the separator's bitmap
    segs, cur = [], []
    for n in names:
        if n.split("<")[0] == SEPARATOR:
            segs.append(cur)
            cur = []
        else:
            cur.append(n)
    assert not cur, f"kernels after the last separator: {cur}"
    assert len(segs) == len(rows), (len(segs), len(rows))
    routes, table, seen = [], [], {}
    for row, seg in zip(rows, segs):
        facts, rc = tuple(row[:-1]), row[-1]
        assert (rc != 0) == (not seg), (row, seg)
        route = ";".join(seg)
        if facts in seen:   # two contexts with the same facts (a modulus loaded but switched off): one row
            assert seen[facts] == (route, rc), (facts, seen[facts], route)
            continue
        seen[facts] = (route, rc)
        if route not in routes:
            routes.append(route)
        table.append(list(facts) + [rc, routes.index(route)])
    doc = {
        "provenance": {
            "commit": commit,
            "how": "rocprofv3 --kernel-trace --output-format csv of `make_mmse_routes.py walk` on one MI355X; "
                   "kernel names ordered by start time, namespace and parameter list stripped, cut at " + SEPARATOR,
            "frames": B,
        },
        "columns": list(FACTS) + ["rc", "route"],
        "routes": routes,
        "rows": table,
    }
    with open(out_path, "w") as f:
        f.write("{\n")
        for k in ("provenance", "columns", "routes"):
            f.write(f' "{k}": {json.dumps(doc[k], indent=1 if k == "routes" else None)},\n')
        f.write(' "rows": [\n' + ",\n".join("  " + json.dumps(r, separators=(",", ":")) for r in table) + "\n ]\n}\n")
    print(f"{len(table)} rows, {len(routes)} distinct routes -> {out_path}")


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    sub = ap.add_subparsers(dest="cmd", required=True)
    w = sub.add_parser("walk")
    w.add_argument("requests")
    c = sub.add_parser("cut")
    c.add_argument("requests")
    c.add_argument("trace")
    c.add_argument("--commit", required=True)
    c.add_argument("--out", default=os.path.join(HERE, "mmse_routes.json"))
    a = ap.parse_args()
    if a.cmd == "walk":
        walk(a.requests)
    else:
        cut(a.requests, a.trace, a.commit, a.out)
