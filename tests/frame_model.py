"""The frame law of the library's batched calls: a frame's outputs depend on that
frame's inputs and the call's shared arguments, and on nothing else: not on its
position in the batch, not on the batch size, not on what its neighbours hold
(include/wce.h, "Frames").  Sharding, first_frame on the transmit side and the
rule that a NaN row changes no other frame all rest on it, and the kernels pack
several frames into a wave, a tile or a workgroup wherever they are fast.

ROWS is the table, one row per batched call.  A row names

    calls     the functions of include/wce.h it binds
    frame     name -> axis: the arguments that are per frame, and where the frames are
    shared    the arguments every frame sees
    outputs   name -> axis: the per-frame outputs
    indexed   the call's definition keys something on the global frame index first_frame + f
    totals    name -> per-frame output: batch-wide counts, equal to the sum of that output

UNBATCHED lists every other function of the header with a frame count, with the
reason it has no row; tests/test_frame_model.py checks that the two together
are complete.  Three transforms, each with the outputs it expects of the base run:

    ("moved", perm)       every per-frame argument indexed by perm -> base[perm].  An indexed row runs it with
                          the noise off (ow2 = 0, which the header defines as no noise)
    ("window", s, n)      frames [s, s + n) as a batch of their own (an indexed row's first_frame raised by s)
                          -> base[s:s + n]
    ("poisoned", which)   the frames in `which` get hostile contents in every per-frame argument (NaN, +-Inf,
                          zeros, 2^+-500, bytes 0x00 / 0xFF, lengths / seeds out of range) -> every other frame
                          as in the base, bit for bit

At most half a batch is poisoned at a time.  Every odd frame, frame 0 and a run
of 16 together would be more (at 67 frames: 33 + 8 + 1), so there are two sets:
every odd frame (every clean frame then shares its wave, quad and tile with a
poisoned one), and frame 0 with a run of consecutive frames (a whole tile of 16
lost)."""
import collections
import re

import numpy as np

import gain_model as gm

Row = collections.namedtuple("Row", "key calls frame shared outputs indexed totals")
EST = ("lt_ls", "ps_linear", "ps_cubic", "ps_sinc", "ps_mmse")


def _row(key, calls, frame, outputs, shared="", axis=0, out_axis=0, indexed=False, totals=None):
    return Row(key, tuple(calls.split()), {n: axis for n in frame.split()}, tuple(shared.split()),
               {n: out_axis for n in outputs.split()}, indexed, dict(totals or {}))


_DEM = "eq sym theta evm nerr"
_CHAN = "cfo ow2 delay"
ROWS = [
    # ---- front end
    _row("blocks", "wce_front_end_blocks wce_front_end_blocks_cfo wce_front_end_blocks_at", "samples eps start", "sym"),
    _row("preamble", "wce_front_end_preamble wce_front_end_preamble_cfo wce_front_end_preamble_at", "lptot start",
         "pre_fft ow2 cfo"),
    _row("sync", "wce_front_end_sync", "capture", "start metric", "ltf threshold"),
    _row("sync_stf", "wce_front_end_sync_stf", "capture", "start cfo metric_stf metric_ltf",
         "ltf threshold_stf threshold_ltf"),
    # ---- the estimators
    _row("estimate", "wce_estimate wce_estimate_noise", "tx rx rx_pre ow2", " ".join(EST) + " eq",
         "tx_pre ctx_tx_pre ctx_rx_pre ctx_ow2 Rhh x_ref"),
    _row("mmse_solve", "wce_mmse_solve", "tx rx", "w", "ctx_tx_pre ctx_rx_pre ctx_ow2 Rhh"),
    _row("mmse_apply", "wce_mmse_apply", "w", "h", "ctx_tx_pre ctx_rx_pre ctx_ow2 Rhh"),
    # ---- demodulators
    _row("demodulate", "wce_demodulate", "tx rx h h_lt", _DEM, "mod scale"),
    _row("track", "wce_track_demodulate", "tx rx h", _DEM + " h_blocks h_last", "mod scale"),
    # ---- soft bits, the decoder, the re-encoder, the PSDU
    _row("soft_demap", "wce_soft_demap", "eq h h_lt", "llr", "mod scale"),
    _row("soft_demap_blocks", "wce_soft_demap_blocks", "eq hb", "llr", "mod scale"),
    _row("viterbi", "wce_viterbi_decode", "llr u", "bits nbiterr", "mod rate terminated"),
    _row("reencode", "wce_reencode", "u rx theta pilots", "tx h", "mod rate scale"),
    _row("psdu_frame", "wce_psdu_frame", "payload lengths seeds", "bits", "mod rate"),
    _row("psdu_deframe", "wce_psdu_deframe", "bits lengths", "psdu seed fcs_ok", "mod rate",
         totals={"n_good": "fcs_ok"}),
    # ---- diversity: branch-major, the frames on axis 1
    _row("combine", "wce_combine", "rx h ow2", "rx_c h_c", axis=1),
    _row("sync_share", "wce_sync_share", "metric start cfo", "start cfo", axis=1, out_axis=1),
    # ---- the transmit side
    _row("modulate", "wce_modulate", "sym tx_pre", "wave"),
    _row("channel", "wce_channel", "wave taps " + _CHAN, "capture", "seed first_frame capture_len", indexed=True),
    _row("transmit", "wce_transmit", "sym tx_pre taps " + _CHAN, "capture", "seed first_frame capture_len",
         indexed=True),
    _row("channel_tv", "wce_channel_tv", "wave knots " + _CHAN, "capture", "seed first_frame capture_len",
         indexed=True),
    _row("transmit_tv", "wce_transmit_tv", "sym tx_pre knots " + _CHAN, "capture", "seed first_frame capture_len",
         indexed=True),
    _row("synth_frames", "wce_synth_frames", "", "tx rx rx_pre", "seed first_frame n_frames amplitude ow2",
         indexed=True),
    _row("short_field", "wce_short_field", "", "wave", "amplitude n_frames"),
    # ---- the guard
    _row("nonfinite_scan", "wce_nonfinite_scan", "H", "bad", totals={"n_bad": "bad"}),
]
BY_KEY = {r.key: r for r in ROWS}
assert len(BY_KEY) == len(ROWS)

UNBATCHED = {
    "wce_ctx_reserve": "computes nothing: it sizes the scratch of later calls",
    "wce_ctx_reserve_stream": "computes nothing: it sizes one stream's scratch",
    "wce_plan_create": "launches nothing: it captures one wce_estimate call, whose frames the estimate row holds",
}


def batched_calls():
    """the functions include/wce.h declares with a frame count: an n_frames or n_packets parameter, or a
    wce_frames argument"""
    with open(gm.HEADER) as f:
        text = f.read()
    decl = re.findall(r"^int (wce_\w+)\(([^;{]*)\);", text, re.M)
    return {name for name, par in decl if re.search(r"\bn_frames\b|\bn_packets\b|\bwce_frames\b", par)}


# ---------------------------------------------------------------- the transforms
def n_frames(row, args):
    for n, ax in row.frame.items():
        if args.get(n) is not None:
            return args[n].shape[ax]
    return int(args["n_frames"])


def rotation(B):
    """the rotation by one: every frame changes its lane slot, and the last frame of a ragged tail moves into a
    full wave"""
    return np.roll(np.arange(B), 1)


def derangement(B, seed=0x6A22):
    rng = np.random.default_rng(seed + B)
    while True:
        p = rng.permutation(B)
        if B < 2 or not np.any(p == np.arange(B)):
            return p


def permutations(B):
    ps = [rotation(B), derangement(B)]
    assert all(not np.any(p == np.arange(B)) and np.array_equal(np.sort(p), np.arange(B)) for p in ps)
    return [("moved", p) for p in ps]


def windows(B):
    """the first frame, the last, all but the last, and one that starts in the middle of a packing unit"""
    w = [(0, 1), (B - 1, 1), (0, B - 1), (B // 2 + 1, B // 2 - 1)]
    return [("window", s, n) for s, n in w if n >= 1]


def poison_sets(B):
    """-> two index sets, each at most half the batch: every odd frame; frame 0 and a run of consecutive frames
    (16 of them where the batch has 34 and more) that starts off a multiple of 4"""
    odd = np.arange(1, B, 2)
    run = min(16, B // 2 - 1)
    s = (B // 4) | 1
    both = np.unique(np.r_[0, np.arange(s, s + run)]).astype(np.int64)
    assert len(odd) <= B // 2 and len(both) <= B // 2 and both.max() < B
    return [("poisoned", odd), ("poisoned", both)]


def transforms(row, B, covered=False):
    """every transform of a row at B frames.  covered: the call's own test file already permutes a batch and
    runs frames alone, so the rotation and the poison are what it lacks.  A row without per-frame arguments has
    nothing to move or to poison"""
    row = BY_KEY[row] if isinstance(row, str) else row
    if not row.frame:
        return windows(B)
    if covered:
        return permutations(B)[:1] + poison_sets(B)
    return permutations(B) + windows(B) + poison_sets(B)


def label(t):
    if t[0] == "moved":
        return "moved:" + ("rotation" if np.array_equal(t[1], rotation(len(t[1]))) else "derangement")
    if t[0] == "window":
        return f"window:{t[1]}+{t[2]}"
    return "poisoned:" + ("odd" if t[1][0] == 1 else "run")


def _take(a, idx, axis):
    return np.ascontiguousarray(np.take(a, idx, axis=axis))


def quiet(row, args):
    """an indexed row with the noise off"""
    out = dict(args)
    if out.get("ow2") is not None:
        out["ow2"] = np.zeros_like(out["ow2"]) if np.ndim(out["ow2"]) else 0.0
    return out


def moved(row, args, perm):
    out = dict(args)
    for n, ax in row.frame.items():
        if out.get(n) is not None:
            out[n] = _take(out[n], perm, ax)
    return out


def window(row, args, s, n):
    out = dict(args)
    for k, ax in row.frame.items():
        if out.get(k) is not None:
            out[k] = _take(out[k], np.arange(s, s + n), ax)
    if "n_frames" in out:
        out["n_frames"] = n
    if row.indexed:
        out["first_frame"] = int(args.get("first_frame", 0)) + s
    return out


# what a poisoned frame holds, by type, one value per poisoned frame in turn
_BIG = {np.dtype(np.float64): 500, np.dtype(np.complex128): 500, np.dtype(np.float32): 100, np.dtype(np.complex64): 100}
POISON_NAMED = {"lengths": (3, -5, 2 ** 31 - 1, 0), "seeds": (0, 128, 255, 200)}     # each out of range


def poison_values(name, dtype):
    dtype = np.dtype(dtype)
    if name in POISON_NAMED:
        return POISON_NAMED[name]
    if dtype.kind in "fc":
        e = _BIG[dtype]
        v = (np.nan, np.inf, -np.inf, 0.0, 2.0 ** e, 2.0 ** -e)
        return tuple(complex(x, x) for x in v) if dtype.kind == "c" else v
    if dtype.kind == "u":
        return (0, np.iinfo(dtype).max)            # bytes 0x00 / 0xFF
    return (0, -1)                                 # signed: the same bytes


def poisoned(row, args, which):
    out = dict(args)
    for n, ax in row.frame.items():
        if out.get(n) is None:
            continue
        a = np.array(out[n])
        vals = poison_values(n, a.dtype)
        for j, f in enumerate(which):
            a[(slice(None),) * ax + (int(f),)] = vals[j % len(vals)]
        out[n] = a
    return out


def apply(row, args, t):
    return {"moved": moved, "window": window, "poisoned": poisoned}[t[0]](row, args, *t[1:])


def _equal(a, b):
    """gain_model.same_bits, element by element"""
    if a.dtype.kind == "c":
        return _equal(a.real, b.real) & _equal(a.imag, b.imag)
    if a.dtype.kind != "f":
        return a == b
    return ((a == b) & (np.signbit(a) == np.signbit(b))) | (np.isnan(a) & np.isnan(b))


def first_difference(got, want, axis=0):
    """-> the first frame whose bits differ, None where gain_model.same_bits holds (-1: another type or shape)"""
    got, want = np.asarray(got), np.asarray(want)
    if got.dtype != want.dtype or got.shape != want.shape:
        return -1
    if gm.same_bits(got, want):
        return None
    eq = np.moveaxis(_equal(got, want), axis, 0).reshape(got.shape[axis], -1).all(axis=1)
    return int(np.argmin(eq))


def check(row, run, args, t, base=None):
    """run(args) and run(the transform of args): every per-frame output the run returns as the transform expects
    it of the base run, by gain_model.same_bits (signs of zero count, a NaN matches a NaN), and every total the
    sum of its per-frame output.  base: the base run where the caller has it (an indexed row's `moved` makes its
    own, with the noise off).  -> a list of (output, first differing frame in the transformed batch); empty:
    the law holds"""
    if row.indexed and t[0] == "moved":
        args, base = quiet(row, args), None
    base = run(args) if base is None else base
    B = n_frames(row, args)
    got = run(apply(row, args, t))
    if t[0] == "moved":
        src = np.asarray(t[1])
    elif t[0] == "window":
        src = np.arange(t[1], t[1] + t[2])
    else:
        src = np.setdiff1d(np.arange(B), t[1])      # every clean frame, none skipped
    bad = []
    for name, ax in row.outputs.items():
        if name not in base:
            continue
        want = _take(base[name], src, ax)
        g = np.asarray(got[name])
        if t[0] == "poisoned":
            if g.shape != np.asarray(base[name]).shape:
                bad.append((name, -1))
                continue
            g = _take(g, src, ax)
        d = first_difference(g, want, ax)
        if d is not None:
            bad.append((name, int(src[d]) if t[0] == "poisoned" and d >= 0 else d))
    for name, per in row.totals.items():
        if name in got and int(np.asarray(got[name]).ravel()[0]) != int(np.sum(got[per], dtype=np.int64)):
            bad.append((name, -1))
    return bad


def hold(row, run, args, ts, base=None):
    """every transform of ts; -> the base run.  A failure names the call, the transform, the output and the
    first frame that differs"""
    row = BY_KEY[row] if isinstance(row, str) else row
    base = run(args) if base is None else base
    for t in ts:
        bad = check(row, run, args, t, base)
        assert not bad, f"{row.key}, {label(t)}: (output, first frame that differs) {bad}"
    return base


# ---------------------------------------------------------------- data the gain sets do not have
def vary_tx(args, seed=0x6A23):
    """the estimators' gain set sends one real BPSK tx to every frame, so a lane that took its neighbour's tx
    would pass, and so would anything wrong in the terms that Im tx switches on: every element of tx gets its own
    factor out of 1, -1, i, -i, and rx with it.  The products are exact, the channel stays, and so does every
    modulus, which the constant-modulus routes need"""
    k = np.random.default_rng(seed).integers(0, 4, args["tx"].shape)

    def turned(z):
        out = np.where(k % 2 == 0, z, z.imag * -1 + 1j * z.real)       # times i, part by part
        return np.where(k >= 2, -out, out)
    out = dict(args)
    out["tx"], out["rx"] = turned(args["tx"]), turned(args["rx"])
    return out


def psdu_frame_set(mod, rate, B):
    """payload [B][max - 4], lengths (4, 5, max - 1, max and random ones), seeds"""
    import psdu_model as pm
    rng = np.random.default_rng(0x6A24 + 16 * mod + rate)
    mx = pm.max_len(mod, rate)
    lengths = rng.integers(4, mx + 1, B).astype(np.int32)
    lengths[:4] = [4, 5, mx - 1, mx]
    return dict(payload=rng.integers(0, 256, (B, mx - 4)).astype(np.uint8), lengths=lengths,
                seeds=rng.integers(1, 128, B).astype(np.uint8), mod=mod, rate=rate)


def psdu_frame_model(a):
    import psdu_model as pm
    mx, T = pm.max_len(a["mod"], a["rate"]), pm.info_bits(a["mod"], a["rate"])
    rows = [pm.frame_one(p[:L - 4], int(s), T) if 4 <= L <= mx else np.zeros(T, np.uint8)
            for p, L, s in zip(a["payload"], a["lengths"], a["seeds"])]
    return {"bits": pm.pack(np.stack(rows))}


def psdu_deframe_set(mod, rate, B):
    """the model's framed rows of psdu_frame_set, every third with one bit of its PSDU flipped and every seventh
    starting with seven zeros (no seed), with their lengths"""
    a = psdu_frame_set(mod, rate, B)
    rows = psdu_frame_model(a)["bits"].copy()
    rows[::3, 2] ^= 0x10
    rows[::7, 0] &= 0x80
    return dict(bits=rows, lengths=a["lengths"], mod=mod, rate=rate)


PSDU_SENT = 0xA5


def psdu_deframe_model(a):
    """psdu [B][max] (PSDU_SENT where nothing is written), seed, fcs_ok, n_good"""
    import psdu_model as pm
    mx, T = pm.max_len(a["mod"], a["rate"]), pm.info_bits(a["mod"], a["rate"])
    psdu, seed, ok = pm.deframe(pm.unpack(a["bits"], T), a["lengths"], a["mod"], a["rate"])
    out = np.full((len(seed), mx), PSDU_SENT, np.uint8)
    for f, p in enumerate(psdu):
        if p is not None:
            out[f, :p.size] = p
    return {"psdu": out, "seed": seed, "fcs_ok": ok, "n_good": np.array([ok.sum()], np.uint32)}


def scan_set(B):
    """estimate rows H [B][53], every fifth frame with one non-finite part"""
    rng = np.random.default_rng(0x6A25)
    H = rng.standard_normal((B, 53)) + 1j * rng.standard_normal((B, 53))
    for j, f in enumerate(range(2, B, 5)):
        H[f, (7 * j) % 53] = complex(*((np.nan, 1.0), (2.0, np.inf), (-np.inf, 0.0))[j % 3])
    return dict(H=H)


def scan_model(a):
    bad = ~np.isfinite(a["H"].view(np.float64)).all(axis=1)
    return {"bad": bad.astype(np.uint8), "n_bad": np.array([bad.sum()], np.uint64)}
