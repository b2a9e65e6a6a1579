"""GPU checks of mmse_rank1_kernel's prologue and workgroup sizes (csrc/wce_rank1.hip): the first
unit's tx / rx loads are issued straight after the bounds test, ahead of the shared u, and the rows
per workgroup follow the launch's block size.

Launch shapes under test (WCE_VARIANT_R1): 0 = the default (256 threads, loads first), 8 = 64
threads (4 rows per workgroup), 9 = 128 threads (8 rows), 10 = the default grid with the previous
prologue (u and the State scalars before the first tx / rx load).  The bit reference is variant 4,
three looping workgroups: a different instantiation (the prefetching build where there is one), whose rows make
many trips.  A unit's bits depend on its own data only, so every shape must repeat them.  The
oracle is the long double closed form (oracle_py.mmse_textbook_closed) at the project's 1e-10
norm-relative; REF's given w has no TEXTBOOK closed form and is held to test_rank1_routes_gpu.py's
long double REF answer at the same 1e-10.  Frames, contexts and helpers are
test_rank1_persistent_gpu.py's.

Rows past the batch leave before any address is formed: the batch sizes below end inside a wave
(1, 3, 5, ...), inside a workgroup of each size and on their edges, and the strided case checks
that H rows past the batch keep a sentinel's bits."""
import numpy as np
import pytest

from oracle_py import N, NBLK, normrel
from test_rank1_gpu import _cvec
from test_rank1_persistent_gpu import THREE_WGS, TOL, _bits, _mmse, _swept_run, _variant, env, swept  # noqa: F401
from test_rank1_routes_gpu import Env, _route_run

pytestmark = pytest.mark.gpu

WG64, WG128, U_FIRST = 8, 9, 10
SHAPES = (0, WG64, WG128, U_FIRST)
B_ROUTES = 37


def _same_bits(got, ref, what):
    for v, a in got.items():
        assert np.array_equal(_bits(a), _bits(ref)), (what, v)


def _oracle_block(env, f, b, oracle, c=None, ow2=None):
    return oracle.mmse_textbook_closed(env["c"] if c is None else c, env["tx"][f, b], env["rx"][f, b],
                                  env["inp"]["ow2"] if ow2 is None else ow2)


@pytest.mark.parametrize("B", [1, 3, 4, 5, 15, 16, 17, 63, 64, 65, 255, 256, 257])
def test_batch_sizes(gpu_wce, env, B):
    """A lone row, part-filled waves (4 rows each), and part-filled and just-filled workgroups of 4, 8 and
    16 rows."""
    ref = _mmse(gpu_wce, env, B, THREE_WGS)
    _same_bits({v: _mmse(gpu_wce, env, B, v) for v in SHAPES}, ref, B)
    err = normrel(ref, env["ref"][:B])
    print(f"\nB={B}: max {err.max():.2e}")
    assert err.max() < TOL, (int(err.argmax()), err.max())


def test_strided_layout(gpu_wce, env, oracle):
    """Block 3 of strided frames (block stride 60, 17 block slots per frame) into H rows of stride 61 in a
    buffer of five rows more than the batch: columns 53..60 and the rows past the batch keep the sentinel."""
    wce, ctx = gpu_wce, env["ctx"]
    B, BS, FS, OS, EXTRA = 37, 60, 17 * 60, 61, 5
    tx = np.full((B, 17, BS), np.nan + 1j * np.nan, np.complex128)
    rx = np.full_like(tx, np.nan + 1j * np.nan)
    tx[:, :NBLK, :N], rx[:, :NBLK, :N] = env["tx"][:B], env["rx"][:B]
    dtx, drx = wce.DeviceArray.from_numpy(tx), wce.DeviceArray.from_numpy(rx)
    fr = ctx.frames(dtx, drx, B, frame_stride=FS, block_stride=BS, block=3)
    sent = np.full((B + EXTRA, OS), 7.0 - 3.0j, np.complex128)
    got = {}
    for v in (THREE_WGS,) + SHAPES:
        dH = wce.DeviceArray.from_numpy(sent)
        with _variant(wce, v):
            ctx.estimate(fr, wce.Outputs(None, None, None, None, dH.addr, None, OS, 0, 0, 0, 0), wce.PS_MMSE)
            wce.synchronize()
        got[v] = dH.numpy()
        assert np.array_equal(_bits(got[v][:B, N:]), _bits(sent[:B, N:])), v
        assert np.array_equal(_bits(got[v][B:]), _bits(sent[B:])), v
    ref = got.pop(THREE_WGS)
    _same_bits(got, ref, "strided")
    err = normrel(ref[:B, :N], np.stack([_oracle_block(env, f, 3, oracle) for f in range(B)]))
    assert err.max() < TOL, (int(err.argmax()), err.max())


def test_route_matlab_split(gpu_wce, env, oracle):
    """MATLAB semantics: 37 frames are 148 (frame, block) units, one dot each."""
    wce, B = gpu_wce, B_ROUTES
    ref = _mmse(wce, env, B, THREE_WGS, semantics=wce.SEM_MATLAB)
    _same_bits({v: _mmse(wce, env, B, v, semantics=wce.SEM_MATLAB) for v in SHAPES}, ref, "split")
    c = _cvec(oracle, env["F"], env["inp"]["tx_pre"], env["inp"]["rx_pre"], matlab=False)
    exp = np.stack([np.mean(np.stack([_oracle_block(env, f, b, oracle, c=c) for b in range(4)]), axis=0)
                    for f in range(B)])
    err = normrel(ref, exp)
    assert err.max() < TOL, (int(err.argmax()), err.max())


@pytest.mark.parametrize("sem", ["C", "MATLAB"])
def test_route_frame_cov(gpu_wce, env, oracle, sem):
    """WCE_MMSE_FRAME_COV: every unit loads its frame's own u behind its tx / rx loads."""
    wce, B, inp = gpu_wce, B_ROUTES, env["inp"]
    ml = sem == "MATLAB"
    kw = dict(rx_pre=env["pre"][:B], mask=wce.PS_MMSE | wce.FRAME_COV, semantics=wce.SEM_MATLAB if ml else wce.SEM_C)
    ref = _mmse(wce, env, B, THREE_WGS, **kw)
    _same_bits({v: _mmse(wce, env, B, v, **kw) for v in SHAPES}, ref, sem)
    exp = []
    for f in range(B):
        cf = _cvec(oracle, env["F"], inp["tx_pre"], env["pre"][f], matlab=ml)
        exp.append(np.mean(np.stack([_oracle_block(env, f, b, oracle, c=cf) for b in range(4 if ml else 1)]),
                           axis=0))
    err = normrel(ref, np.stack(exp))
    assert err.max() < TOL, (int(err.argmax()), err.max())


@pytest.mark.parametrize("fc", [False, True], ids=["shared", "frame_cov"])
def test_route_per_frame_noise(gpu_wce, env, oracle, fc):
    """wce_estimate_noise: ow2[f] is loaded with the unit's tx / rx.  A zero and an infinite entry make their
    rows NaN; every other row keeps the bits of the run without them."""
    wce, B, inp = gpu_wce, B_ROUTES, env["inp"]
    rng = np.random.default_rng(0x0E7)
    ow2 = inp["ow2"] * 10.0 ** rng.uniform(-1.0, 1.0, B)
    bad = ow2.copy()
    bad[13], bad[30] = 0.0, np.inf
    kw = dict(mask=wce.PS_MMSE | (wce.FRAME_COV if fc else 0))
    if fc:
        kw["rx_pre"] = env["pre"][:B]
    clean = _mmse(wce, env, B, THREE_WGS, ow2=ow2, **kw)
    ref = _mmse(wce, env, B, THREE_WGS, ow2=bad, **kw)
    _same_bits({v: _mmse(wce, env, B, v, ow2=bad, **kw) for v in SHAPES}, ref, "noise")
    _same_bits({v: _mmse(wce, env, B, v, ow2=ow2, **kw) for v in SHAPES}, clean, "noise, clean")
    assert np.isnan(ref[[13, 30]].real).all() and np.isnan(ref[[13, 30]].imag).all()
    good = np.setdiff1d(np.arange(B), [13, 30])
    assert np.array_equal(_bits(ref[good]), _bits(clean[good]))
    assert np.isfinite(clean).all()
    exp = []
    for f in good:
        cf = _cvec(oracle, env["F"], inp["tx_pre"], env["pre"][f]) if fc else env["c"]
        exp.append(_oracle_block(env, f, 0, oracle, c=cf, ow2=ow2[f]))
    err = normrel(ref[good], np.stack(exp))
    assert err.max() < TOL, err.max()


def test_route_ref_given_w(gpu_wce, golden, oracle):
    """REF with the border dot off under WCE_MMSE_FRAME_COV, C semantics: each unit's u and the given w are
    its own, loaded behind its tx / rx."""
    renv = Env(gpu_wce, golden, oracle)
    name = "ref_bdot_off-frame_cov"
    ref = _route_run(renv, name, "mmse", "C", THREE_WGS)["ps_mmse"]
    assert ref.shape == (B_ROUTES, N)
    _same_bits({v: _route_run(renv, name, "mmse", "C", v)["ps_mmse"] for v in SHAPES}, ref, name)
    err = normrel(ref, renv.expected(name, "C"))
    assert err.max() < TOL, (int(err.argmax()), err.max())


def test_plan_replay_default(gpu_wce, env, swept):
    """One replay of the default through a plan (captured graph): the direct call's bits."""
    direct = _swept_run(gpu_wce, env, swept, 0).numpy()
    replay = _swept_run(gpu_wce, env, swept, 0, plan=True).numpy()
    assert np.array_equal(_bits(direct), _bits(replay))
