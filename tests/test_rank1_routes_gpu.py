"""Every dispatch route into the rank-1 PS_MMSE solve (plan_route in
csrc/wce_route.cpp decides it, estimate_impl in csrc/wce_api.cpp runs it; which
kernels each request launches is pinned on the CPU by tests/test_route.py):
the closed form (mmse_rank1_kernel, WCE_VARIANT_R1 = 0, and its nontemporal
build, 2) and the retained 53 x 53 factorisation (variant 1: mmse_solve_fc_kernel,
and mmse_solve_ls_kernel<true, true, *> when the LS family rides along in C
semantics), each against a long double oracle at 1e-10 norm-relative.

    context    request                          semantics   variants   oracle
    TEXTBOOK   PS_MMSE | ALL | ALL + ls_f32     C, MATLAB   0, 1, 2    mmse_textbook_closed(c, ...)
    TEXTBOOK   the same + FRAME_COV             C, MATLAB   0, 1, 2    the same with c_f of the frame's preamble
    COV        PS_MMSE | ALL, + FRAME_COV       C, MATLAB   0, 1       the TEXTBOOK per-frame oracle (and the
                                                                       TEXTBOOK context's bits: the modifier
                                                                       replaces the model covariance)
    REF with   PS_MMSE | ALL, + FRAME_COV       C, MATLAB   0, 1       C: mmse_ref_repaired with the frame's LT_LS;
    bdot off                                                           MATLAB: mean over blocks 0..3 of mmse_unified
                                                                       (C_ref(h_f), pilots, 0, 2 ow2), h_f the
                                                                       MATLAB LT_LS (ls_kernel<*, ML>: proper conj)

REF with the border dot off is the one public route into rank1_s's `cwg`
branch (a given w, the complex division, State::xmask = the pilots); a = 0
there, so g = 0 -- the branch with g != 0 is pinned on the CPU model only
(tests/test_rank1_model.py against tests/golden/rank1_cw_mp.npz).

37 frames (3 workgroups of the closed form in C semantics, the last partial;
148 units in MATLAB semantics): BPSK, QPSK and 16-QAM, matched and unrelated
channels, a DC null, every block its own symbols, per-frame preambles drawn
independently of the data.  The split (MATLAB) closed form also runs at 1, 3,
4, 5 and 17 frames (4..68 units of 16 lanes, 16 units per workgroup), through a
plan replay, and with blocks 4..14 changed.

Measured on an MI355X, max norm-relative over the 37 frames; PS_MMSE alone, ALL
and ALL + ls_f32 give the same figures on every route:

    route                        variant 0 / 2    variant 1    variant 1 against 0
    TEXTBOOK shared     C        1.4e-12          3.2e-13      1.4e-12
    TEXTBOOK shared     MATLAB   6.4e-13          5.4e-13      6.4e-13
    TEXTBOOK FRAME_COV  C        3.0e-13          3.1e-13      1.7e-14
    TEXTBOOK FRAME_COV  MATLAB   4.6e-13          4.6e-13      1.7e-14
    COV FRAME_COV       C, MATLAB: the TEXTBOOK FRAME_COV bits and figures
    REF bdot off        C        3.0e-15          3.8e-15      1.6e-15   (border dot off against on 1.9e-15)
    REF bdot off        MATLAB   2.0e-13          6.2e-14      2.3e-13   (border dot off against on 2.3e-13)

so every route the project had not measured stays inside the 1e-11 between
the two forms.  The LS family and the equalized symbols are bit-identical
between variant 0 (LS pass, then the closed form) and variant 1 (in C
semantics the fused epilogue), in fp64 and in fp32 storage.  Small split
batches: at most 6.4e-13 (TEXTBOOK) and 2.0e-13 (REF).

Each of these breaks at least one test here (tried on scratch builds, not
committed): prep_frame_cov dropping cw; `closed` forced false for COV +
FRAME_COV; mmse_rank1_kernel ignoring State::xmask; mmse_rank1_kernel reading
block 0 for every split unit; mmse_solve_fc_kernel and mmse_solve_ls_kernel
multiplying s by frame 0's u.
"""
import contextlib

import numpy as np
import pytest

from oracle_py import N, NBLK, PILOTS, from_split, normrel
from test_rank1_gpu import _cvec, _mixed

pytestmark = pytest.mark.gpu

TOL = 1e-10        # GPU against the long double oracle
TOL_V1 = 1e-11     # the factorisation against the closed form (test_variant_factorisation_agrees)
TOL_BDOT = 1e-11   # REF: border dot off against on (test_border_dot_matches_backsolve_path)
TOL_F32 = 1e-6     # LS family stored as complex float (test_config5_gpu.py)
B0 = 37
OS = 61            # H row stride: columns 53..60 hold a sentinel that must survive
SENT = 7.0 - 3.0j
R1 = 5             # WCE_VARIANT_R1
LS_NAMES = ("lt_ls", "ps_linear", "ps_cubic", "ps_sinc")

ROUTES = {
    "textbook-shared": dict(ctx="textbook", fc=False, oracle="tb_shared", variants=(0, 1, 2),
                            requests=("mmse", "all", "all_f32")),
    "textbook-frame_cov": dict(ctx="textbook", fc=True, oracle="tb_fc", variants=(0, 1, 2),
                               requests=("mmse", "all", "all_f32")),
    "cov-frame_cov": dict(ctx="cov", fc=True, oracle="tb_fc", variants=(0, 1), requests=("mmse", "all")),
    "ref_bdot_off-frame_cov": dict(ctx="ref", fc=True, oracle="ref", variants=(0, 1), requests=("mmse", "all")),
}
CASES = [(r, q, s) for r, d in ROUTES.items() for q in d["requests"] for s in ("C", "MATLAB")]
SPLIT_ROUTES = ("textbook-shared", "textbook-frame_cov", "ref_bdot_off-frame_cov")


class Env:
    """Contexts, the 37 frames and preambles, and the long double answers, each computed once."""

    def __init__(self, wce, golden, oracle):
        self.wce, self.oracle = wce, oracle
        inp = self.inp = golden["inputs"]
        r = golden["ref"]
        self.F = oracle.fmatrix()
        self.Fr, self.invF = from_split(r["F"]), from_split(r["invF"])
        self.ow2 = inp["ow2"]
        pdp = np.exp(-0.05 * np.arange(N))   # 53 taps: a full-rank model covariance, nothing like c c'
        self.ctx = {
            "textbook": wce.Context(inp["tx_pre"], inp["rx_pre"], inp["ow2"], wce.MMSE_TEXTBOOK),
            "cov": wce.Context(inp["tx_pre"], inp["rx_pre"], inp["ow2"], Rhh=np.diag(pdp / pdp.sum() * 1.1e-4 + 0j)),
            "ref": wce.Context(inp["tx_pre"], inp["rx_pre"], inp["ow2"], wce.MMSE_REF),
        }
        assert self.ctx["cov"].cov_info()[0] == N, "a full-rank model covariance"
        self.hlt = np.asarray(oracle.lt_ls(inp["tx_pre"], inp["rx_pre"]), np.complex128)
        self.c = _cvec(oracle, self.F, inp["tx_pre"], inp["rx_pre"])
        rng = np.random.default_rng(0x707E5)
        self.tx, self.rx = _mixed(rng, self.hlt, inp["ow2"], B0)
        # REF's caller preamble: the context's with every third entry negated
        self.tpre = np.array(inp["tx_pre"], np.complex128)
        self.tpre[::3] *= -1.0
        amp = np.sqrt(np.mean(np.abs(self.hlt) ** 2) / 2.0)
        hp = amp * (rng.standard_normal((B0, N)) + 1j * rng.standard_normal((B0, N)))
        noise = np.sqrt(inp["ow2"] / 2.0) * (rng.standard_normal((2, B0, N)) + 1j * rng.standard_normal((2, B0, N)))
        self.pre = {"textbook": hp * inp["tx_pre"] + noise[0], "ref": hp * self.tpre + noise[1]}
        self.pre["cov"] = self.pre["textbook"]
        for a in (self.tx, self.rx, self.tpre, *self.pre.values()):
            a.setflags(write=False)
        self._ref, self._ls, self._runs = {}, {}, {}

    def blocks(self, name, sem):
        """the frame blocks a request estimates: MATLAB 0..3 (averaged), C the one asked for (REF: 2)"""
        return range(4) if sem == "MATLAB" else ((2,) if ROUTES[name]["ctx"] == "ref" else (0,))

    def run_args(self, name, sem):
        d = ROUTES[name]
        kw = dict(sem=self.wce.SEM_MATLAB if sem == "MATLAB" else self.wce.SEM_C, block=self.blocks(name, sem)[0])
        if d["ctx"] == "ref":
            kw["tx_pre"] = self.tpre
        return kw

    def expected(self, name, sem):
        """[37][53] long double PS_MMSE of a route (ROUTES[name]["oracle"]) in one semantics"""
        kind = ROUTES[name]["oracle"]
        if (kind, sem) in self._ref:
            return self._ref[kind, sem]
        o, ml, tx, rx = self.oracle, sem == "MATLAB", self.tx, self.rx
        out = []
        for f in range(B0):
            bl = self.blocks(name, sem)
            if kind == "tb_shared":
                per = [o.mmse_textbook_closed(self.c, tx[f, b], rx[f, b], self.ow2) for b in bl]
            elif kind == "tb_fc":
                cf = _cvec(o, self.F, self.inp["tx_pre"], self.pre["textbook"][f], matlab=ml)
                per = [o.mmse_textbook_closed(cf, tx[f, b], rx[f, b], self.ow2) for b in bl]
            elif not ml:
                hf = o.lt_ls(self.tpre, self.pre["ref"][f])
                per = [o.mmse_ref_repaired(tx[f, b], rx[f, b], self.Fr, self.ow2, hf, self.invF) for b in bl]
            else:   # ls_kernel<*, ML> feeds the factors: lt_ls_lane<true>, the proper conjugate
                C = o.mmse_ref_cmatrix(self.Fr, self.invF, o.matlab_lt_ls(self.tpre, self.pre["ref"][f]))
                per = [o.mmse_unified(C, o.pilot_mask(), 0, 2 * np.longdouble(self.ow2), tx[f, b], rx[f, b]) for b in bl]
            out.append(np.mean(np.stack(per), axis=0))
        self._ref[kind, sem] = np.stack(out)
        return self._ref[kind, sem]

    def ls_expected(self, sem):
        """the LS family and the equalized symbols of the TEXTBOOK rows (block 0 / blocks 0..3)"""
        if sem not in self._ls:
            o, tx, rx, pre, tp = self.oracle, self.tx, self.rx, self.pre["textbook"], self.inp["tx_pre"]
            if sem == "MATLAB":
                lt = [o.matlab_lt_ls(tp, pre[f]) for f in range(B0)]
                ps = {k: [o.matlab(k, tx[f], rx[f]) for f in range(B0)] for k in LS_NAMES[1:]}
            else:
                lt = [o.lt_ls(tp, pre[f]) for f in range(B0)]
                ps = {k: [getattr(o, k)(tx[f, 0], rx[f, 0]) for f in range(B0)] for k in LS_NAMES[1:]}
            e = dict(lt_ls=np.stack(lt), **{k: np.stack(v) for k, v in ps.items()})
            e["eq"] = np.stack([o.equalize(rx[f], e["lt_ls"][f], e["ps_linear"][f]) for f in range(B0)])
            self._ls[sem] = e
        return self._ls[sem]

    def split37(self, name):
        """PS_MMSE (+ FRAME_COV) of the 37 frames in MATLAB semantics, variant 0: the bits the small batches must repeat"""
        if name not in self._runs:
            self._runs[name] = _route_run(self, name, "mmse", "MATLAB", 0)["ps_mmse"]
            self._runs[name].setflags(write=False)
        return self._runs[name]


@pytest.fixture(scope="module")
def env(gpu_wce, golden, oracle):
    return Env(gpu_wce, golden, oracle)


@contextlib.contextmanager
def _knobs(wce, ctx, variant=0, bdot=True):
    """The process-global R1 variant and the context's border dot, both put back whatever happens."""
    lib = wce.load()
    try:
        assert lib.wce_debug_set_variant(R1, variant) == 0
        ctx.set_border_dot(bdot)
        yield
    finally:
        assert lib.wce_debug_set_variant(R1, 0) == 0
        ctx.set_border_dot(True)


def _run(wce, ctx, tx, rx, mask, sem, pre=None, tx_pre=None, block=0, f32=False, plan=False):
    """One wce_estimate (or a plan replay of it) on host frames: every H output in rows of stride OS filled with a
    sentinel beforehand; returns the 53 live columns after checking the rest."""
    B = tx.shape[0]
    dev = wce.DeviceArray.from_numpy
    dtx, drx = dev(np.asarray(tx, np.complex128)), dev(np.asarray(rx, np.complex128))
    dpre = dev(np.asarray(pre, np.complex128)) if pre is not None else None
    dtp = dev(np.asarray(tx_pre, np.complex128)) if tx_pre is not None else None
    lsdt = np.complex64 if f32 else np.complex128
    bits = (("lt_ls", wce.LT_LS), ("ps_linear", wce.PS_LINEAR), ("ps_cubic", wce.PS_CUBIC), ("ps_sinc", wce.PS_SINC),
            ("ps_mmse", wce.PS_MMSE))
    bufs = {n: dev(np.full((B, OS), SENT, np.complex128 if n == "ps_mmse" else lsdt)) for n, bit in bits if mask & bit}
    deq = wce.DeviceArray((B, NBLK, N), lsdt, zero=True) if mask & wce.EQUALIZE else None
    o = wce.Outputs(*[(bufs[n].addr if n in bufs else None) for n, _ in bits], deq.addr if deq is not None else None,
                    OS, NBLK * N, N, wce.PS_LINEAR, wce.OUT_LS_F32 if f32 else 0)
    fr = ctx.frames(dtx, drx, B, rx_pre=dpre, tx_pre=dtp, block=block, semantics=sem)
    if plan:
        p = ctx.plan(fr, o, mask)
        p.launch()
        wce.synchronize()
        p.close()
    else:
        ctx.estimate(fr, o, mask)
        wce.synchronize()
    res = {}
    for n, d in bufs.items():
        a = d.numpy()
        assert np.all(a[:, N:] == SENT), f"{n}: columns past 52 were written"
        res[n] = np.ascontiguousarray(a[:, :N])
    if deq is not None:
        res["eq"] = deq.numpy()
    return res


def _route_run(env, name, request, sem, variant, B=B0, tx=None, rx=None, plan=False, bdot=None):
    """A route's request on the first B frames, with its knobs set for the run only."""
    wce, d = env.wce, ROUTES[name]
    ctx = env.ctx[d["ctx"]]
    mask = (wce.PS_MMSE if request == "mmse" else wce.ALL) | (wce.FRAME_COV if d["fc"] else 0)
    pre = env.pre[d["ctx"]][:B] if d["fc"] or request != "mmse" else None
    tx, rx = env.tx if tx is None else tx, env.rx if rx is None else rx
    if bdot is None:
        bdot = d["ctx"] != "ref"
    with _knobs(wce, ctx, variant, bdot):
        return _run(wce, ctx, tx[:B], rx[:B], mask, pre=pre, f32=request == "all_f32", plan=plan,
                    **env.run_args(name, sem))


def _flat(a):
    return np.asarray(a).reshape(a.shape[0], -1)


@pytest.mark.parametrize("name,request_kind,sem", CASES, ids=["-".join(c) for c in CASES])
def test_route(env, name, request_kind, sem):
    """One row of the table, one request, one semantics, every variant of the row."""
    d = ROUTES[name]
    exp = env.expected(name, sem)
    got = {v: _route_run(env, name, request_kind, sem, v) for v in d["variants"]}
    errs = {v: normrel(got[v]["ps_mmse"], exp) for v in got}
    d10 = normrel(got[1]["ps_mmse"], got[0]["ps_mmse"])
    print(f"\n{name} {request_kind} {sem}: " + ", ".join(f"v{v} vs oracle {e.max():.2e}" for v, e in errs.items()) +
          f"; v1 vs v0 {d10.max():.2e}")
    for v, e in errs.items():
        assert np.isfinite(got[v]["ps_mmse"]).all(), v
        assert e.max() < TOL, (v, int(e.argmax()), e.max())
    if 2 in got:   # the nontemporal build of the closed form: the same bits, every output
        for k in got[0]:
            assert np.array_equal(got[0][k], got[2][k]), k
    assert d10.max() < TOL_V1, (int(d10.argmax()), d10.max())
    if request_kind != "mmse":
        # variant 0: the LS pass, then mmse_rank1_kernel; variant 1 in C semantics: the fused epilogue
        for k in LS_NAMES + ("eq",):
            assert np.array_equal(got[0][k], got[1][k]), k
    if request_kind == "all_f32":
        ls = env.ls_expected(sem)
        for v in got:
            assert got[v]["ps_mmse"].dtype == np.complex128
            for k in LS_NAMES:
                assert got[v][k].dtype == np.complex64
                assert normrel(got[v][k].astype(np.complex128), ls[k]).max() < TOL_F32, (v, k)
            assert normrel(_flat(got[v]["eq"].astype(np.complex128)), _flat(ls["eq"])).max() < TOL_F32, v
    if d["ctx"] == "cov":
        # FRAME_COV replaces a COV context's model covariance: the TEXTBOOK context's bits
        for v in got:
            tb = _route_run(env, "textbook-frame_cov", request_kind, sem, v)
            for k in tb:
                assert np.array_equal(got[v][k], tb[k]), (v, k)
    if d["ctx"] == "ref":
        on = _route_run(env, name, request_kind, sem, 0, bdot=True)   # ref_fc_kernel (C) / the pilot form (MATLAB)
        db = normrel(got[0]["ps_mmse"], on["ps_mmse"])
        print(f"  border dot off vs on {db.max():.2e}")
        assert db.max() < TOL_BDOT, (int(db.argmax()), db.max())
        # State::xmask hides tx off the four pilots: garbage there changes no bit
        rng = np.random.default_rng(0x6A)
        junk = np.array(env.tx)
        off = np.setdiff1d(np.arange(N), PILOTS)
        junk[:, :, off] = 1e200 * (rng.choice([-1.0, 1.0], (B0, NBLK, off.size)) +
                                   1j * rng.choice([-1.0, 1.0], (B0, NBLK, off.size)))
        for v in got:
            g2 = _route_run(env, name, request_kind, sem, v, tx=junk)
            for k in got[v]:
                assert np.array_equal(g2[k], got[v][k]), (v, k)


@pytest.mark.parametrize("B", [1, 3, 4, 5, 17])
@pytest.mark.parametrize("name", SPLIT_ROUTES)
def test_split_batch_edges(env, name, B):
    """The split closed form, unit g = 4 f + b: 4, 12, 16, 20 and 68 units -- a partial wave, a partial
    workgroup, exactly one, and a frame whose blocks straddle two.  Every frame against the oracle, and the
    bits of the same frames inside the 37-frame batch."""
    out = _route_run(env, name, "mmse", "MATLAB", 0, B=B)["ps_mmse"]
    err = normrel(out, env.expected(name, "MATLAB")[:B])
    print(f"\n{name} B={B}: max {err.max():.2e}")
    assert err.max() < TOL, (int(err.argmax()), err.max())
    assert np.array_equal(out, env.split37(name)[:B])


@pytest.mark.parametrize("name", SPLIT_ROUTES)
def test_split_plan_replay(env, name):
    """wce_plan_create sizes the plan's own workspace (dots, and the per-frame factors); the replay gives the direct call's bits."""
    out = _route_run(env, name, "mmse", "MATLAB", 0, plan=True)["ps_mmse"]
    assert np.array_equal(out, env.split37(name))
    assert normrel(out, env.expected(name, "MATLAB")).max() < TOL


@pytest.mark.parametrize("name", SPLIT_ROUTES)
def test_split_reads_blocks_0_to_3_only(env, name):
    tx, rx = np.array(env.tx), np.array(env.rx)
    tx[:, 4:] = tx[:, 4:] * (-0.5 + 2.0j) + 3.0
    rx[:, 4:] = rx[:, 4:] * (1.5 - 0.25j) - 1.0
    out = _route_run(env, name, "mmse", "MATLAB", 0, tx=tx, rx=rx)["ps_mmse"]
    assert np.array_equal(out, env.split37(name))
