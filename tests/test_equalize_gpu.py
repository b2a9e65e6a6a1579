"""The equalization epilogue ls_store_rv (csrc/wce_kernels.hip) per element, on every kernel family that carries
it, from every wce_outputs.eq_source, in fp64 and in fp32 storage (WCE_OUT_LS_F32):

    family                          context    semantics   request                               route (wce.debug_route)
    ls_kernel<true, false>          TEXTBOOK   C           EQUALIZE + LS bits                    ls
                                                           ALL                                   ls;mmse_rank1
    ls_kernel<true, true>           TEXTBOOK   MATLAB      the same two                          ls / ls;mmse_rank1;fc_finish
    ref_ls_elem_kernel<true>        REF        C           PS_MMSE | EQUALIZE ...                ref_ls_elem
                                                           the same + FRAME_COV                  ref_fc;ref_ls_elem_done
    mmse_solve_ls_kernel<.,.,true>  COV        C           PS_MMSE | EQUALIZE ...                fused_dense;apply
                                    (a full-rank diagonal Rhh)
    and, with ctx.set_fusion(False), REF and COV through ls_kernel<true, false> as a separate pass.

The reference is the long double WiFi_Equalization.m (oracle_py.equalize) on the long double LT_LS and PS estimate
of the same inputs, per element by complex modulus.  The bounds come from the host model alone
(tests/eq_model.py, measured in tests/test_eq_model.py; nothing is taken from a device run):

    fp32   twice the model's worst element on the set: 4.7e-7 .. 5.5e-7, under the 1e-6 gate
    fp64   kappa_b[k] x (the fp64 formula's worst element over kappa on the set) x 4: 7.6e-15 .. 9.0e-14 times
           kappa, kappa up to 2e6 on the fade set

Data (eq_model.Sets, fixed seed): 37 frames -- ls_kernel takes 4 per wave and 16 per workgroup, so the last group
is partial; ref_ls_elem_kernel takes 256 elements per workgroup and 53 per frame, so frames straddle workgroups;
mmse_solve_ls_kernel takes one frame per workgroup -- and their first 1 and 5.  plain: BPSK / QPSK / 16-QAM blocks on
per-frame 3-tap channels with per-frame preambles; fade: 15 elements whose blend at one block is -delta wps hps,
delta = 1e-2, 1e-4, 1e-6, one k of each linear segment and k = 52 at every delta; scale: the channel times 2^100
and 2^-100 (rx stays a normal fp32 number).  Every stride is padded (frame 15 * 56 + 3, block 56, H rows 61, eq
frame 15 * 57 + 5, eq block 57, preamble 55); input gaps hold NaN, output gaps and two rows past the batch a
sentinel; all six output pointers are set on every call, whatever the mask.

Measured on an MI355X: fp32, the worst element of every family equals the host model's worst on the set or lies
below it (2.43e-7 .. 2.77e-7 against bounds of 4.68e-7 .. 5.53e-7); fp64, the worst element stands at 0.25 .. 0.41
of its bound, PS_Cubic in MATLAB semantics at 0.86 (7.8e-14 on plain, 1.1e-9 at kappa = 2e6).  The whole file runs
in about two seconds.

Each of these breaks at least one test here (tried on scratch builds, not committed): ls_store_rv always taking
hlin (test_every_source, test_fp32_per_element, test_isolation); the fp32 blend formed from fp32-rounded hlt and
hps (test_fp32_per_element); ls_args without its `|= eq_src` line (test_mask_does_not_change_eq, PS_Cubic and
PS_Sinc).  ls_args as it was before it nulled the unrequested pointers fails test_unrequested_outputs_untouched
for every source, in fp64 and in fp32 storage, and nothing else.
"""
import hashlib

import numpy as np
import pytest

import eq_model as em
from eq_model import B0, DC, N, NBLK, PILOTS, TX_BLOCK

pytestmark = pytest.mark.gpu

OS, BS, FS, EBS, EFS, PS, PAD = 61, 56, 15 * 56 + 3, 57, 15 * 57 + 5, 55, 2
SENT = 7.0 - 3.0j
H_NAMES = ("lt_ls", "ps_linear", "ps_cubic", "ps_sinc", "ps_mmse")
SRC_IDS = ("default", "linear", "cubic", "sinc")
SRC_NAME = dict(default="ps_linear", linear="ps_linear", cubic="ps_cubic", sinc="ps_sinc")
KINDS = ("plain", "fade", "scale")


class Env:
    def __init__(self, wce, golden, oracle):
        self.wce = wce
        self.sets = em.datasets(oracle, golden)
        inp = golden["inputs"]
        pdp = np.exp(-0.05 * np.arange(N))   # 53 taps: a full-rank model covariance (test_rank1_routes_gpu.py's)
        self.ctx = {
            "textbook": wce.Context(inp["tx_pre"], inp["rx_pre"], inp["ow2"], wce.MMSE_TEXTBOOK),
            "ref": wce.Context(inp["tx_pre"], inp["rx_pre"], inp["ow2"], wce.MMSE_REF),
            "cov": wce.Context(inp["tx_pre"], inp["rx_pre"], inp["ow2"], Rhh=np.diag(pdp / pdp.sum() * 1.1e-4 + 0j)),
        }
        rank, lowrank = self.ctx["cov"].cov_info()[:2]
        assert rank == N and not lowrank, "a full-rank model covariance on the dense path"
        self.mode = dict(textbook=wce.MMSE_TEXTBOOK, ref=wce.MMSE_REF, cov=wce.MMSE_COV)
        self.bits = dict(lt_ls=wce.LT_LS, ps_linear=wce.PS_LINEAR, ps_cubic=wce.PS_CUBIC, ps_sinc=wce.PS_SINC,
                         ps_mmse=wce.PS_MMSE)
        self.src = dict(default=0, linear=wce.PS_LINEAR, cubic=wce.PS_CUBIC, sinc=wce.PS_SINC)
        self._dev, self._memo, self._pool = {}, {}, {}
        self.dtp = wce.DeviceArray.from_numpy(self.sets.tx_pre)
        self.dtx = self._frames_dev(self.sets.tx)

    # ---- inputs on the device, padded, gaps NaN
    def _frames_dev(self, a):
        p = np.full((B0, FS), np.nan + 1j * np.nan, np.complex128)
        p[:, :NBLK * BS].reshape(B0, NBLK, BS)[:, :, :N] = a
        return self.wce.DeviceArray.from_numpy(p)

    def _pre_dev(self, a):
        p = np.full((B0, PS), np.nan + 1j * np.nan, np.complex128)
        p[:, :N] = a
        return self.wce.DeviceArray.from_numpy(p)

    def inputs(self, kind, sem, name):
        rx, pre = self.sets.inputs[kind, sem, name]
        key = (id(rx), id(pre))
        if key not in self._dev:
            self._dev[key] = (self._frames_dev(rx), self._pre_dev(pre))
        return self._dev[key]

    # ---- the route planner on the facts of a call
    def route(self, ctxk, sem, mask, f32=False, fuse=True):
        wce = self.wce
        return wce.debug_route(self.mode[ctxk], True, fuse, False, -1, N if ctxk == "cov" else 0,
                               wce.SEM_MATLAB if sem == "MATLAB" else wce.SEM_C, mask, f32, 0, 0, 0)

    # ---- one call
    def call(self, ctxk, sem, mask, src, f32, drx, dpre, B=B0, fuse=True, plan=False, eq_source=None):
        """wce_estimate with all six output pointers set -> the live part of every buffer (None where it kept its
        sentinel throughout), `bad`: the buffers with a gap, a row past B or an unrequested element overwritten."""
        wce, ctx = self.wce, self.ctx[ctxk]
        lsdt = np.complex64 if f32 else np.complex128
        dev = wce.DeviceArray.from_numpy
        bufs = {n: dev(np.full((B + PAD, OS), SENT, np.complex128 if n == "ps_mmse" else lsdt)) for n in H_NAMES}
        deq = dev(np.full((B + PAD, EFS), SENT, lsdt))
        o = wce.Outputs(*[bufs[n].addr for n in H_NAMES], deq.addr, OS, EFS, EBS,
                        self.src[src] if eq_source is None else eq_source, wce.OUT_LS_F32 if f32 else 0)
        fr = ctx.frames(self.dtx, drx, B, frame_stride=FS, block_stride=BS, rx_pre=dpre, pre_stride=PS, tx_pre=self.dtp,
                        block=TX_BLOCK, semantics=wce.SEM_MATLAB if sem == "MATLAB" else wce.SEM_C)
        ctx.set_fusion(fuse)
        try:
            if plan:
                p = ctx.plan(fr, o, mask)
                p.launch()
                wce.synchronize()
                p.close()
            else:
                ctx.estimate(fr, o, mask)
        except wce.WceError:
            wce.synchronize()
            self.refused = self._collect(bufs, deq, 0, B)   # a refused call: what it left in the buffers
            raise
        finally:
            ctx.set_fusion(True)
        wce.synchronize()
        return self._collect(bufs, deq, mask, B)

    def _collect(self, bufs, deq, mask, B):
        res, bad = {}, []
        for n in H_NAMES:
            a = bufs[n].numpy()
            asked = bool(mask & self.bits[n])
            clean = np.all(a[:B, N:] == SENT) and np.all(a[B:] == SENT) and (asked or np.all(a[:B, :N] == SENT))
            if not clean:
                bad.append(n)
            res[n] = np.ascontiguousarray(a[:B, :N]) if asked else None
        a = deq.numpy()
        asked = bool(mask & self.wce.EQUALIZE)
        blocks = a[:B, :NBLK * EBS].reshape(B, NBLK, EBS)
        clean = (np.all(blocks[:, :, N:] == SENT) and np.all(a[:B, NBLK * EBS:] == SENT) and np.all(a[B:] == SENT)
                 and (asked or np.all(blocks[:, :, :N] == SENT)))
        if not clean:
            bad.append("eq")
        res["eq"] = np.ascontiguousarray(blocks[:, :, :N]) if asked else None
        return res, bad

    def run(self, ctxk, sem, mask, src, f32, kind, B=B0, fuse=True, plan=False):
        """call() on a set, once per distinct request"""
        key = (ctxk, sem, mask, src, f32, kind, B, fuse, plan)
        if key not in self._memo:
            drx, dpre = self.inputs(kind, sem, SRC_NAME[src])
            res, bad = self.call(ctxk, sem, mask, src, f32, drx, dpre, B, fuse, plan)
            self._memo[key] = ({n: self._intern(a) for n, a in res.items()}, bad)
        return self._memo[key]

    def _intern(self, a):
        """equal outputs of different requests are kept once (most of these runs repeat one another's bits)"""
        if a is None:
            return None
        a.setflags(write=False)
        return self._pool.setdefault((a.dtype.str, a.shape, hashlib.sha1(a.tobytes()).digest()), a)


@pytest.fixture(scope="module")
def env(gpu_wce, golden, oracle):
    return Env(gpu_wce, golden, oracle)


def _cases(wce):
    """(id, context, semantics, mask, the route the planner must name) of the table above"""
    full = wce.EQUALIZE | wce.LS_ALL
    return [
        ("ls_c", "textbook", "C", full, "ls"),
        ("ls_c-all", "textbook", "C", wce.ALL, "ls;mmse_rank1"),
        ("ls_matlab", "textbook", "MATLAB", full, "ls"),
        ("ls_matlab-all", "textbook", "MATLAB", wce.ALL, "ls;mmse_rank1;fc_finish"),
        ("ref_elem", "ref", "C", wce.ALL, "ref_ls_elem"),
        ("ref_elem-frame_cov", "ref", "C", wce.ALL | wce.FRAME_COV, "ref_fc;ref_ls_elem_done"),
        ("fused_dense", "cov", "C", wce.ALL, "fused_dense;apply"),
    ]


CASE_IDS = ("ls_c", "ls_c-all", "ls_matlab", "ls_matlab-all", "ref_elem", "ref_elem-frame_cov", "fused_dense")


def _case(env, cid):
    c = {c[0]: c for c in _cases(env.wce)}[cid]
    assert env.route(c[1], c[2], c[3]) == c[4], (cid, env.route(c[1], c[2], c[3]))
    assert env.route(c[1], c[2], c[3], f32=True) == c[4], cid
    return c[1:4]


def _off_dc(a):
    return np.delete(a, DC, axis=-1)


def _same(a, b):
    """the same bits, NaNs included (or neither requested)"""
    if a is None or b is None:
        return a is None and b is None
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def _rows(a, sel):
    return None if a is None else a[sel]


def test_case_ids_cover_the_table(env):
    assert tuple(c[0] for c in _cases(env.wce)) == CASE_IDS
    wce = env.wce
    # the separate-pass twins of the fused families
    assert env.route("ref", "C", wce.ALL, fuse=False) == "ls;ref_pilots"
    assert env.route("cov", "C", wce.ALL, fuse=False).startswith("ls;factor_dense")


@pytest.mark.parametrize("cid", CASE_IDS)
def test_every_source(env, cid):
    """fp64: every eq element of every source within kappa x the host figure x 4 of the long double value, on
    plain, fade and scale; 0 gives PS_Linear's bits; DC exactly 0; the three sources differ."""
    ctxk, sem, mask = _case(env, cid)
    eqs = {}
    for src in SRC_IDS:
        name = SRC_NAME[src]
        for kind in KINDS:
            res, bad = env.run(ctxk, sem, mask, src, False, kind)
            eq = res["eq"]
            assert bad == [] and eq.dtype == np.complex128
            assert np.all(eq[..., DC] == 0)
            err = em.relerr(eq, env.sets.exact(kind, sem, name)["eq"])
            lim = env.sets.bound_f64(kind, sem, name)
            worst = float(np.max(_off_dc(err / lim)))
            print(f"\n{cid} {src} {kind}: worst element at {worst:.2f} of its bound "
                  f"(max err {float(_off_dc(err).max()):.2e})")
            assert np.isfinite(_off_dc(eq)).all() and worst < 1.0, (src, kind, worst)
            if mask & env.wce.PS_MMSE and kind != "scale":
                assert np.isfinite(res["ps_mmse"]).all()
            eqs[src, kind] = eq
    for kind in KINDS:
        assert _same(eqs["default", kind], eqs["linear", kind]), kind
    for a, b in (("linear", "cubic"), ("linear", "sinc"), ("cubic", "sinc")):
        differ = _off_dc(eqs[a, "plain"]) != _off_dc(eqs[b, "plain"])
        assert differ.mean() > 0.9, (a, b, differ.mean())


@pytest.mark.parametrize("B", [1, 5])
@pytest.mark.parametrize("cid", CASE_IDS)
def test_small_batches(env, cid, B):
    """the first 1 and 5 frames alone: the bits of the same frames inside the 37, rows past B untouched"""
    ctxk, sem, mask = _case(env, cid)
    for src in SRC_IDS[1:]:
        for f32 in (False, True):
            for kind in ("plain", "fade"):
                res, bad = env.run(ctxk, sem, mask, src, f32, kind, B=B)
                big, _ = env.run(ctxk, sem, mask, src, f32, kind)
                assert bad == [], (src, f32, kind, bad)
                for k in H_NAMES[:4] + ("eq",):
                    assert _same(res[k], big[k][:B]), (src, f32, kind, k)


def _mask_runs(env):
    """(context, semantics, mask, fuse) of every request tests 2 and 3 compare"""
    wce = env.wce
    out = []
    for ctxk, sem in (("textbook", "C"), ("textbook", "MATLAB"), ("ref", "C"), ("cov", "C")):
        for mmse in (0, wce.PS_MMSE) + ((wce.PS_MMSE | wce.FRAME_COV,) if ctxk == "ref" else ()):
            for ls in ("none", "source", "all"):
                for fuse in (True, False) if (ctxk != "textbook" and mmse) else (True,):
                    out.append((ctxk, sem, mmse, ls, fuse))
    return out


def _ls_mask(wce, ls, src):
    return wce.EQUALIZE | (0 if ls == "none" else wce.LS_ALL if ls == "all" else (wce.PS_LINEAR if src == "default" else
                                                                                  {"linear": wce.PS_LINEAR, "cubic": wce.PS_CUBIC, "sinc": wce.PS_SINC}[src]))


@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
@pytest.mark.parametrize("src", SRC_IDS)
def test_mask_does_not_change_eq(env, src, f32):
    """EQUALIZE alone, with the source's bit, with every LS bit, with and without PS_MMSE (and FRAME_COV on REF),
    fused and as a separate pass: one set of eq bits per semantics -- so also the same across the four
    C-semantics families, as ref_ls_elem_kernel's comment promises."""
    wce = env.wce
    for kind in ("plain", "fade"):
        first = {}
        seen = set()
        for ctxk, sem, mmse, ls, fuse in _mask_runs(env):
            mask = _ls_mask(wce, ls, src) | mmse
            seen.add(env.route(ctxk, sem, mask, f32, fuse))
            res, _ = env.run(ctxk, sem, mask, src, f32, kind, fuse=fuse)
            ref = first.setdefault(sem, res["eq"])
            assert _same(res["eq"], ref), (kind, ctxk, sem, hex(mask), fuse)
        # every family was among them
        assert {"ls", "ls;mmse_rank1", "ref_ls_elem", "ref_fc;ref_ls_elem_done", "fused_dense;apply",
                "ls;ref_pilots"} <= seen, seen


@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
@pytest.mark.parametrize("src", SRC_IDS)
def test_unrequested_outputs_untouched(env, src, f32):
    """All six pointers set: a buffer whose bit is not in the mask keeps every sentinel -- the source's too, which
    the kernels compute for the blend -- and so do the gaps and the rows past the batch of those that are."""
    wce = env.wce
    for ctxk, sem, mmse, ls, fuse in _mask_runs(env):
        mask = _ls_mask(wce, ls, src) | mmse
        res, bad = env.run(ctxk, sem, mask, src, f32, "plain", fuse=fuse)
        assert bad == [], (ctxk, sem, hex(mask), fuse, bad)
        for n in H_NAMES:
            assert (res[n] is not None) == bool(mask & env.bits[n])
            if res[n] is not None:
                assert res[n].dtype == (np.complex64 if f32 and n != "ps_mmse" else np.complex128)
                assert not np.any(res[n] == SENT), n


@pytest.mark.parametrize("cid", CASE_IDS)
def test_fp32_per_element(env, cid):
    """WCE_OUT_LS_F32: every element within twice the host model's worst of the long double value, on plain, fade
    and scale; complex64; DC exactly 0; sentinels intact; the C families' bits agree."""
    ctxk, sem, mask = _case(env, cid)
    for src in SRC_IDS:
        name = SRC_NAME[src]
        for kind in KINDS:
            res, bad = env.run(ctxk, sem, mask, src, True, kind)
            eq = res["eq"]
            assert bad == [] and eq.dtype == np.complex64
            for n in H_NAMES[:4]:
                assert res[n].dtype == np.complex64
            assert res["ps_mmse"] is None or res["ps_mmse"].dtype == np.complex128
            assert np.all(eq[..., DC] == 0)
            err = _off_dc(em.relerr(eq, env.sets.exact(kind, sem, name)["eq"]))
            lim = env.sets.bound_f32(kind, sem, name)
            print(f"\n{cid} {src} {kind}: max {float(err.max()):.3e}, bound {lim:.3e}")
            assert lim < em.GATE_F32
            assert np.isfinite(_off_dc(eq)).all() and float(err.max()) <= lim, (src, kind, float(err.max()), lim)
            if sem == "C":
                base, _ = env.run("textbook", "C", env.wce.EQUALIZE | env.wce.LS_ALL, src, True, kind)
                assert _same(eq, base["eq"]), (src, kind)


@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
@pytest.mark.parametrize("cid", CASE_IDS)
def test_isolation(env, cid, f32):
    """A NaN in rx off the estimating block's pilots reaches its own eq element only; a NaN at a pilot of the
    estimating block reaches its own frame only; hlt = hps = 0 at one subcarrier makes that column of the frame
    non-finite and nothing else."""
    ctxk, sem, mask = _case(env, cid)
    rx, pre = env.sets.inputs["plain", sem, "ps_sinc"]
    f, b, k = 17, 5, 7
    est = range(4) if sem == "MATLAB" else (TX_BLOCK,)
    others = np.arange(B0) != f

    def go(src, rx2, pre2=pre):
        return env.call(ctxk, sem, mask, src, f32, env._frames_dev(rx2), env._pre_dev(pre2))

    for src in SRC_IDS[1:]:
        base, _ = env.run(ctxk, sem, mask, src, f32, "plain")
        # (a) one data element
        r2 = np.array(rx)
        r2[f, b, k] = np.nan
        res, bad = go(src, r2)
        assert bad == [] and not np.isfinite(res["eq"][f, b, k])
        patched = np.array(res["eq"])
        patched[f, b, k] = base["eq"][f, b, k]
        assert _same(patched, base["eq"]), src
        for n in H_NAMES:
            assert _same(res[n], base[n]), (src, n)
        # (b) a pilot of an estimating block
        r2 = np.array(rx)
        r2[f, est[-1], PILOTS[1]] = np.nan
        res, bad = go(src, r2)
        hit = np.ones(N, bool)
        hit[DC] = False
        if src == "linear":   # PS_Linear reads pilot 1 on the first two segments only
            hit[PILOTS[2]:] = False
        assert bad == [] and not np.isfinite(res["eq"][f][:, hit]).any(), src
        assert np.isfinite(res["eq"][f][:, ~hit]).all() and np.all(res["eq"][f][:, DC] == 0)
        assert _same(res["eq"][others], base["eq"][others]), src
        for n in H_NAMES:
            assert _same(_rows(res[n], others), _rows(base[n], others)), (src, n)
        # (c) hlt = hps = 0 at pilot 0 (PS_Sinc there is h0 + 3.9e-17 h1 + ...: never exactly 0)
        if src == "sinc":
            continue
        r2, p2 = np.array(rx), np.array(pre)
        r2[f, list(est), PILOTS[0]] = 0.0
        p2[f, PILOTS[0]] = 0.0
        res, bad = go(src, r2, p2)
        col = np.zeros(N, bool)
        col[PILOTS[0]] = True
        assert bad == [] and not np.isfinite(res["eq"][f][:, col]).any(), src
        assert np.isfinite(res["eq"][f][:, ~col]).all(), src
        assert _same(res["eq"][others], base["eq"][others]), src


@pytest.mark.parametrize("cid", CASE_IDS)
def test_plan_replay(env, cid):
    """one plan with eq_source = PS_Sinc: the direct call's bits in every output"""
    ctxk, sem, mask = _case(env, cid)
    for f32 in (False, True):
        direct, _ = env.run(ctxk, sem, mask, "sinc", f32, "fade")
        res, bad = env.run(ctxk, sem, mask, "sinc", f32, "fade", plan=True)
        assert bad == []
        for n in H_NAMES + ("eq",):
            assert _same(res[n], direct[n]), (f32, n)


@pytest.mark.parametrize("ctxk,sem", [("textbook", "C"), ("textbook", "MATLAB"), ("ref", "C"), ("cov", "C")])
def test_refusals(env, ctxk, sem):
    """With EQUALIZE: an eq_source that is no PS interpolation estimator is WCE_EINVAL with its own
    wce_last_error() text, and nothing is written.  Without EQUALIZE the field is not looked at."""
    wce, lib = env.wce, env.wce.load()
    drx, dpre = env.inputs("plain", sem, "ps_linear")
    for bad_src in (wce.LT_LS, wce.PS_MMSE, wce.PS_LINEAR | wce.PS_CUBIC, 0x80):
        for mask in (wce.EQUALIZE, wce.ALL):
            with pytest.raises(wce.WceError) as e0:   # another refusal first, so that the text below is this call's
                env.call(ctxk, sem, 0x80, "default", False, drx, dpre)
            assert e0.value.code == -1 and b"unknown estimator bits" in lib.wce_last_error()
            with pytest.raises(wce.WceError) as e1:
                env.call(ctxk, sem, mask, "default", False, drx, dpre, eq_source=bad_src)
            assert e1.value.code == -1 and b"eq_source" in lib.wce_last_error(), (hex(bad_src), hex(mask))
            res, bad = env.refused
            assert bad == [] and all(v is None for v in res.values())
    # ignored without EQUALIZE
    want, _ = env.call(ctxk, sem, wce.LS_ALL, "default", False, drx, dpre)
    for bad_src in (wce.LT_LS, wce.PS_MMSE, 0x80):
        res, bad = env.call(ctxk, sem, wce.LS_ALL, "default", False, drx, dpre, eq_source=bad_src)
        assert bad == [] and res["eq"] is None
        for n in H_NAMES[:4]:
            assert _same(res[n], want[n]), (hex(bad_src), n)
