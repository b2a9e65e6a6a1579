"""GPU checks of mmse_rank1_kernel's launch shapes (csrc/wce_rank1.hip): rows that loop over
units with the next unit's loads in flight, u kept in registers where it is shared.

The launch shapes are values of WCE_VARIANT_R1, read by launch_mmse_rank1 alone:
3 = one unit per 16-lane row (the grid covers the batch: no second trip, nothing
prefetched), 4 = three workgroups (48 rows per sweep: a few hundred frames make many
ragged trips), 5 / 6 = nontemporal stores / loads on the default grid, 7 = the
persistent grid (at most wce_debug_rank1_rows_per_sweep rows), 0 = the default, which
is 3's shape since the persistent grid measured no faster (DESIGN s6).  A unit's bits
depend on its own data only, so every shape must give the same bits; the oracle is the
long double closed form (oracle_py.mmse_textbook_closed) at the project's 1e-10
norm-relative.  Frames are test_rank1_model.make_frames' mixed classes, as in
test_rank1_gpu.py."""
import contextlib

import numpy as np
import pytest

from oracle_py import N, NBLK, normrel
from test_rank1_gpu import _cvec, _mixed

pytestmark = pytest.mark.gpu

TOL = 1e-10
NF = 261
R1 = 5   # WCE_VARIANT_R1
ONE_PER_ROW, THREE_WGS, NT_STORES, NT_LOADS, PERSISTENT = 3, 4, 5, 6, 7
SEED = 0x80211   # bench.py's


@contextlib.contextmanager
def _variant(wce, v):
    lib = wce.load()
    try:
        assert lib.wce_debug_set_variant(R1, v) == 0
        yield
    finally:
        assert lib.wce_debug_set_variant(R1, 0) == 0


def _bits(a):
    """complex128 -> the 64-bit patterns, so that NaN rows compare too"""
    return np.ascontiguousarray(a).view(np.uint64)


@pytest.fixture(scope="module")
def env(gpu_wce, golden, oracle):
    """One TEXTBOOK context, NF mixed frames, their preambles and the long double answers of block 0."""
    inp = golden["inputs"]
    F = oracle.fmatrix()
    ctx = gpu_wce.Context(inp["tx_pre"], inp["rx_pre"], inp["ow2"], gpu_wce.MMSE_TEXTBOOK)
    ctx.reserve(NF)
    hlt = np.asarray(oracle.lt_ls(inp["tx_pre"], inp["rx_pre"]), np.complex128)
    c = _cvec(oracle, F, inp["tx_pre"], inp["rx_pre"])
    rng = np.random.default_rng(0x9E2)
    tx, rx = _mixed(rng, hlt, inp["ow2"], NF)
    amp = np.sqrt(np.mean(np.abs(hlt) ** 2) / 2.0)
    hp = amp * (rng.standard_normal((NF, N)) + 1j * rng.standard_normal((NF, N)))
    pre = hp * inp["tx_pre"] + np.sqrt(inp["ow2"] / 2.0) * (rng.standard_normal((NF, N)) + 1j * rng.standard_normal((NF, N)))
    ref = np.stack([oracle.mmse_textbook_closed(c, tx[f, 0], rx[f, 0], inp["ow2"]) for f in range(NF)])
    for a in (tx, rx, pre, ref):
        a.setflags(write=False)
    return dict(inp=inp, F=F, ctx=ctx, hlt=hlt, c=c, tx=tx, rx=rx, pre=pre, ref=ref)


def _mmse(wce, env, B, variant, **kw):
    with _variant(wce, variant):
        return env["ctx"].estimate_host(env["tx"][:B], env["rx"][:B], mask=kw.pop("mask", wce.PS_MMSE), **kw)["ps_mmse"]


@pytest.mark.parametrize("B", [1, 15, 16, 17, 47, 48, 49, 96, 97, 261])
def test_ragged_trips(gpu_wce, env, B):
    """48 rows per sweep: 48 frames are one trip for every row, with no next unit to prefetch; 49 make one
    row of a wave take a second trip while its neighbours stop; 261 are five full sweeps and a part."""
    looped = _mmse(gpu_wce, env, B, THREE_WGS)
    single = _mmse(gpu_wce, env, B, ONE_PER_ROW)
    assert np.array_equal(_bits(looped), _bits(single))
    err = normrel(looped, env["ref"][:B])
    print(f"\nB={B}: max {err.max():.2e}")
    assert err.max() < TOL, (int(err.argmax()), err.max())


def test_route_matlab_split(gpu_wce, env, oracle):
    """MATLAB semantics: 37 frames are 148 (frame, block) units, one dot each, averaged by fc_finish_kernel."""
    wce, B = gpu_wce, 37
    looped = _mmse(wce, env, B, THREE_WGS, semantics=wce.SEM_MATLAB)
    single = _mmse(wce, env, B, ONE_PER_ROW, semantics=wce.SEM_MATLAB)
    assert np.array_equal(_bits(looped), _bits(single))
    c = _cvec(oracle, env["F"], env["inp"]["tx_pre"], env["inp"]["rx_pre"], matlab=False)
    exp = np.stack([np.mean(np.stack([oracle.mmse_textbook_closed(c, env["tx"][f, b], env["rx"][f, b], env["inp"]["ow2"])
                                      for b in range(4)]), axis=0) for f in range(B)])
    err = normrel(looped, exp)
    assert err.max() < TOL, (int(err.argmax()), err.max())


@pytest.mark.parametrize("sem", ["C", "MATLAB"])
def test_route_frame_cov(gpu_wce, env, oracle, sem):
    """WCE_MMSE_FRAME_COV: every unit loads its frame's own u in its own trip."""
    wce, B, inp = gpu_wce, 37, env["inp"]
    ml = sem == "MATLAB"
    kw = dict(rx_pre=env["pre"][:B], mask=wce.PS_MMSE | wce.FRAME_COV, semantics=wce.SEM_MATLAB if ml else wce.SEM_C)
    looped = _mmse(wce, env, B, THREE_WGS, **kw)
    single = _mmse(wce, env, B, ONE_PER_ROW, **kw)
    assert np.array_equal(_bits(looped), _bits(single))
    exp = []
    for f in range(B):
        cf = _cvec(oracle, env["F"], inp["tx_pre"], env["pre"][f], matlab=ml)
        exp.append(np.mean(np.stack([oracle.mmse_textbook_closed(cf, env["tx"][f, b], env["rx"][f, b], inp["ow2"])
                                     for b in range(4 if ml else 1)]), axis=0))
    err = normrel(looped, np.stack(exp))
    assert err.max() < TOL, (int(err.argmax()), err.max())


@pytest.mark.parametrize("fc", [False, True], ids=["shared", "frame_cov"])
def test_route_per_frame_noise(gpu_wce, env, oracle, fc):
    """wce_estimate_noise: ow2[f] is loaded per unit.  A non-positive and an infinite entry make their rows
    NaN and change no other row's bits."""
    wce, B, inp = gpu_wce, 97, env["inp"]
    rng = np.random.default_rng(0x0E6)
    ow2 = inp["ow2"] * 10.0 ** rng.uniform(-1.0, 1.0, B)
    bad = ow2.copy()
    bad[13], bad[60] = 0.0, np.inf
    kw = dict(mask=wce.PS_MMSE | (wce.FRAME_COV if fc else 0))
    if fc:
        kw["rx_pre"] = env["pre"][:B]
    clean = _mmse(wce, env, B, ONE_PER_ROW, ow2=ow2, **kw)
    looped = _mmse(wce, env, B, THREE_WGS, ow2=bad, **kw)
    single = _mmse(wce, env, B, ONE_PER_ROW, ow2=bad, **kw)
    assert np.array_equal(_bits(looped), _bits(single))
    assert np.isnan(looped[[13, 60]].real).all() and np.isnan(looped[[13, 60]].imag).all()
    good = np.setdiff1d(np.arange(B), [13, 60])
    assert np.array_equal(_bits(looped[good]), _bits(clean[good]))
    assert np.isfinite(clean).all()
    exp = []
    for f in good[::4]:
        cf = _cvec(oracle, env["F"], inp["tx_pre"], env["pre"][f]) if fc else env["c"]
        exp.append(oracle.mmse_textbook_closed(cf, env["tx"][f, 0], env["rx"][f, 0], ow2[f]))
    err = normrel(looped[good[::4]], np.stack(exp))
    assert err.max() < TOL, err.max()


def test_route_strided_layout(gpu_wce, env):
    """test_block3_strided_frames_and_out_stride_61's layout (block 3, block stride 60, 17 block slots per
    frame, H rows of stride 61) on looping rows: columns past 52 stay untouched."""
    wce, ctx = gpu_wce, env["ctx"]
    B, BS, FS, OS = 37, 60, 17 * 60, 61
    tx = np.full((B, 17, BS), np.nan + 1j * np.nan, np.complex128)
    rx = np.full_like(tx, np.nan + 1j * np.nan)
    tx[:, :NBLK, :N], rx[:, :NBLK, :N] = env["tx"][:B], env["rx"][:B]
    dtx, drx = wce.DeviceArray.from_numpy(tx), wce.DeviceArray.from_numpy(rx)
    fr = ctx.frames(dtx, drx, B, frame_stride=FS, block_stride=BS, block=3)
    got = {}
    for v in (THREE_WGS, ONE_PER_ROW):
        dH = wce.DeviceArray.from_numpy(np.full((B, OS), 7.0 - 3.0j, np.complex128))
        with _variant(wce, v):
            ctx.estimate(fr, wce.Outputs(None, None, None, None, dH.addr, None, OS, 0, 0, 0, 0), wce.PS_MMSE)
            wce.synchronize()
        got[v] = dH.numpy()
        assert np.all(got[v][:, N:] == 7.0 - 3.0j)
    assert np.array_equal(_bits(got[THREE_WGS]), _bits(got[ONE_PER_ROW]))
    assert np.array_equal(got[THREE_WGS][:, :N], _mmse(wce, env, B, ONE_PER_ROW, block=3))


@pytest.fixture(scope="module")
def swept(gpu_wce, env):
    """Two sweeps of the persistent grid and five frames, made on the device as bench.py makes its batch."""
    wce, ctx = gpu_wce, env["ctx"]
    rows = wce.load().wce_debug_rank1_rows_per_sweep(ctx.handle)
    assert rows > 0 and rows % 16 == 0, rows
    B = 2 * rows + 5
    hs = wce.DeviceArray.from_numpy(ctx.shared()[0])
    tx, rx = wce.DeviceArray((B, NBLK, N)), wce.DeviceArray((B, NBLK, N))
    ctx.synth(tx, rx, None, B, first_frame=0, seed=SEED, h_shared=hs)
    wce.synchronize()
    return dict(B=B, tx=tx, rx=rx, fr=ctx.frames(tx, rx, B))


def _swept_run(wce, env, swept, variant, plan=False):
    H = wce.DeviceArray((swept["B"], N), zero=True)
    o = wce.Outputs(None, None, None, None, H.addr, None, N, 0, 0, 0, 0)
    with _variant(wce, variant):
        if plan:
            p = env["ctx"].plan(swept["fr"], o, wce.PS_MMSE)
            p.launch()
            wce.synchronize()
            p.close()
        else:
            env["ctx"].estimate(swept["fr"], o, wce.PS_MMSE)
            wce.synchronize()
    return H


def test_launches_past_one_sweep(gpu_wce, env, swept, oracle):
    """Every row of the persistent grid makes two trips and five rows a third; its whole H, the default
    launch's and each cache policy's are what one unit per row gives, and 64 sampled frames match the oracle."""
    wce, B, inp = gpu_wce, swept["B"], env["inp"]
    H0 = _swept_run(wce, env, swept, 0)
    h0 = _bits(H0.numpy())
    for v in (ONE_PER_ROW, PERSISTENT, NT_STORES, NT_LOADS, 2):
        assert np.array_equal(h0, _bits(_swept_run(wce, env, swept, v).numpy())), v
    idx = np.unique(np.concatenate([[0, B - 1], np.linspace(1, B - 2, 62).astype(np.int64)]))
    assert len(idx) == 64
    errs = np.array([float(normrel(H0.rows(f)[0], oracle.mmse_textbook_closed(env["c"], swept["tx"].rows(f)[0, 0],
                                                                              swept["rx"].rows(f)[0, 0], inp["ow2"])))
                     for f in idx])
    print(f"\n{B} frames, 64 samples: max {errs.max():.2e}")
    assert errs.max() < TOL, errs.max()


@pytest.mark.parametrize("v", [NT_STORES, NT_LOADS, PERSISTENT])
def test_cache_policies_and_persistent_grid_same_bits(gpu_wce, env, v):
    """261 frames: below one sweep, so the persistent grid launches one unit per row of its prefetching build."""
    assert np.array_equal(_bits(_mmse(gpu_wce, env, NF, v)), _bits(_mmse(gpu_wce, env, NF, 0)))


@pytest.mark.parametrize("v", [0, PERSISTENT], ids=["default", "persistent"])
def test_plan_replay(gpu_wce, env, swept, v):
    """A plan replays the launch path: the persistent grid's size comes from the context, not from a device query."""
    direct = _swept_run(gpu_wce, env, swept, v).numpy()
    replay = _swept_run(gpu_wce, env, swept, v, plan=True).numpy()
    assert np.array_equal(_bits(direct), _bits(replay))
    assert np.array_equal(_bits(direct), _bits(_swept_run(gpu_wce, env, swept, ONE_PER_ROW).numpy()))
