"""GPU checks of mmse_rank1_head_kernel (csrc/wce_rank1_head.hip): the headline's launch of the closed-form
rank-1 PS_MMSE solve with preloaded scalar arguments, in workgroups of 64, 128 or 256 threads, with and
without the placement of neighbouring groups on one XCD.

WCE_VARIANT_R1: 14 / 15 / 16 = the head kernel in 64 / 128 / 256 threads in dispatch order, 17 / 18 / 19 = the
same with the remap, 13 = the head kernel off, 0 = whatever was adopted.  The arithmetic is
mmse_rank1_kernel's (csrc/wce_rank1_body.h) and a unit's bits depend on its own data only, so every shape
must repeat, bit for bit, variant 4 (three looping workgroups of mmse_rank1_kernel: the prefetching build)
and variant 10 (mmse_rank1_kernel's general build behind the previous prologue).  The oracle is the long
double closed form (oracle_py.mmse_textbook_closed) at the project's 1e-10 norm-relative.  Frames and
helpers are test_rank1_persistent_gpu.py's.

The remap is where a wrong index would write a row twice or never: the batch sizes put the number of groups
below the 8 XCD labels and at 8k - 1, 8k and 8k + 1 for each workgroup size, and end inside waves and
workgroups; the sentinel cases check every row of H and the rows and columns around it."""
import numpy as np
import pytest

from oracle_py import N, NBLK, normrel
from test_rank1_gpu import _cvec, _mixed
from test_rank1_persistent_gpu import THREE_WGS, TOL, _bits, _mmse, _variant

pytestmark = pytest.mark.gpu

NF = 1021
U_FIRST, HEAD_OFF = 10, 13
HEAD = (14, 15, 16, 17, 18, 19)
NEW = HEAD + (HEAD_OFF,)
RUNS = (0,) + NEW
SENT = 7.0 - 3.0j


@pytest.fixture(scope="module")
def henv(gpu_wce, golden, oracle):
    """One TEXTBOOK context, NF mixed frames, their preambles and the long double answers of block 0."""
    inp = golden["inputs"]
    F = oracle.fmatrix()
    ctx = gpu_wce.Context(inp["tx_pre"], inp["rx_pre"], inp["ow2"], gpu_wce.MMSE_TEXTBOOK)
    ctx.reserve(NF)
    hlt = np.asarray(oracle.lt_ls(inp["tx_pre"], inp["rx_pre"]), np.complex128)
    c = _cvec(oracle, F, inp["tx_pre"], inp["rx_pre"])
    rng = np.random.default_rng(0x4EAD)
    tx, rx = _mixed(rng, hlt, inp["ow2"], NF)
    amp = np.sqrt(np.mean(np.abs(hlt) ** 2) / 2.0)
    hp = amp * (rng.standard_normal((64, N)) + 1j * rng.standard_normal((64, N)))
    pre = hp * inp["tx_pre"] + np.sqrt(inp["ow2"] / 2.0) * (rng.standard_normal((64, N)) + 1j * rng.standard_normal((64, N)))
    ref = np.stack([oracle.mmse_textbook_closed(c, tx[f, 0], rx[f, 0], inp["ow2"]) for f in range(NF)])
    for a in (tx, rx, pre, ref):
        a.setflags(write=False)
    return dict(inp=inp, F=F, ctx=ctx, hlt=hlt, c=c, tx=tx, rx=rx, pre=pre, ref=ref)


def _device_run(wce, ctx, fr, B, v, rows, stride, offset=0, plan=False):
    """H of one launch under variant v into a sentinel-filled [rows][stride] buffer, written from element `offset`"""
    dH = wce.DeviceArray.from_numpy(np.full((rows, stride), SENT, np.complex128))
    o = wce.Outputs(None, None, None, None, dH.addr + 16 * offset, None, stride, 0, 0, 0, 0)
    with _variant(wce, v):
        if plan:
            p = ctx.plan(fr, o, wce.PS_MMSE)
            p.launch()
            wce.synchronize()
            p.close()
        else:
            ctx.estimate(fr, o, wce.PS_MMSE)
            wce.synchronize()
    return dH.numpy()


@pytest.mark.parametrize("B", [1, 3, 4, 5, 7, 8, 9, 28, 29, 31, 32, 33, 35, 36, 37, 63, 64, 65, 255, 256, 257, 1021])
def test_batch_sizes(gpu_wce, henv, B):
    looped = _mmse(gpu_wce, henv, B, THREE_WGS)
    general = _mmse(gpu_wce, henv, B, U_FIRST)
    assert np.array_equal(_bits(looped), _bits(general))
    for v in RUNS:
        assert np.array_equal(_bits(_mmse(gpu_wce, henv, B, v)), _bits(looped)), v
    err = normrel(looped, henv["ref"][:B])
    print(f"\nB={B}: max {err.max():.2e}")
    assert err.max() < TOL, (int(err.argmax()), err.max())


@pytest.mark.parametrize("B", [37, 257])
def test_sentinel_rows_and_columns(gpu_wce, henv, B):
    """H rows of stride 61 in a buffer five rows longer than the batch: every row of the batch is written with
    variant 4's bits, columns 53..60 and the rows past the batch keep the sentinel's."""
    wce, ctx = gpu_wce, henv["ctx"]
    OS, EXTRA = 61, 5
    dtx, drx = wce.DeviceArray.from_numpy(henv["tx"][:B]), wce.DeviceArray.from_numpy(henv["rx"][:B])
    fr = ctx.frames(dtx, drx, B)
    sent = np.full((B + EXTRA, OS), SENT, np.complex128)
    want = _mmse(wce, henv, B, THREE_WGS)
    assert not np.any(_bits(want) == _bits(sent[:B, :N]))   # so an unwritten entry shows
    for v in RUNS:
        got = _device_run(wce, ctx, fr, B, v, B + EXTRA, OS)
        assert np.array_equal(_bits(got[:B, :N]), _bits(want)), v
        assert np.array_equal(_bits(got[:B, N:]), _bits(sent[:B, N:])), v
        assert np.array_equal(_bits(got[B:]), _bits(sent[B:])), v


def test_strided_input(gpu_wce, henv):
    """Block 3 of frames with block stride 60 and 17 block slots (the host folds the block into tx and rx), H rows
    of stride 61; the slots and columns that are not frames hold NaN."""
    wce, ctx = gpu_wce, henv["ctx"]
    B, BS, FS, OS = 37, 60, 17 * 60, 61
    tx = np.full((B, 17, BS), np.nan + 1j * np.nan, np.complex128)
    rx = np.full_like(tx, np.nan + 1j * np.nan)
    tx[:, :NBLK, :N], rx[:, :NBLK, :N] = henv["tx"][:B], henv["rx"][:B]
    dtx, drx = wce.DeviceArray.from_numpy(tx), wce.DeviceArray.from_numpy(rx)
    fr = ctx.frames(dtx, drx, B, frame_stride=FS, block_stride=BS, block=3)
    want = _mmse(wce, henv, B, THREE_WGS, block=3)
    assert np.isfinite(want).all()
    for v in RUNS + (U_FIRST,):
        got = _device_run(wce, ctx, fr, B, v, B, OS)
        assert np.array_equal(_bits(got[:, :N]), _bits(want)), v
        assert np.all(got[:, N:] == SENT), v


def test_unaligned_h_base(gpu_wce, henv):
    """H starts one 848-B row into its buffer, 80 B past a 128-B line: the same bits, the row before and the
    row after untouched."""
    wce, ctx = gpu_wce, henv["ctx"]
    B = 37
    dtx, drx = wce.DeviceArray.from_numpy(henv["tx"][:B]), wce.DeviceArray.from_numpy(henv["rx"][:B])
    fr = ctx.frames(dtx, drx, B)
    want = _mmse(wce, henv, B, THREE_WGS)
    for v in RUNS:
        got = _device_run(wce, ctx, fr, B, v, B + 2, N, offset=N)
        assert np.array_equal(_bits(got[1:B + 1]), _bits(want)), v
        assert np.all(got[0] == SENT) and np.all(got[B + 1] == SENT), v


@pytest.mark.parametrize("nan_at,inf_at", [(("tx", 7), ("rx", 50)), (("rx", 52), ("tx", 48)), (("tx", 49), ("rx", 0))])
def test_nonfinite_input(gpu_wce, henv, nan_at, inf_at):
    """A NaN in frame 5 and an Inf in frame 20: the entries that are not finite are variant 10's, and every other
    frame keeps the bits of the run without them."""
    wce, B = gpu_wce, 37
    bad = dict(henv, tx=henv["tx"][:B].copy(), rx=henv["rx"][:B].copy())
    bad[nan_at[0]][5, 0, nan_at[1]] = np.nan
    bad[inf_at[0]][20, 0, inf_at[1]] = np.inf
    clean = _mmse(wce, henv, B, U_FIRST)
    want = _mmse(wce, bad, B, U_FIRST)
    fin = np.isfinite(want.real) & np.isfinite(want.imag)
    assert not fin[5].any() or not fin[20].any()
    other = np.setdiff1d(np.arange(B), [5, 20])
    assert np.array_equal(_bits(want[other]), _bits(clean[other]))
    for v in RUNS:
        got = _mmse(wce, bad, B, v)
        assert np.array_equal(np.isfinite(got.real) & np.isfinite(got.imag), fin), v
        assert np.array_equal(_bits(got[other]), _bits(clean[other])), v
        assert np.array_equal(_bits(got[fin]), _bits(want[fin])), v


@pytest.mark.parametrize("route", ["matlab_split", "frame_cov_c", "frame_cov_matlab", "noise", "ref"])
def test_other_routes_keep_the_old_kernel(gpu_wce, henv, route):
    """Launches the head kernel does not serve, at 37 frames: under every variant that names it, and under the
    default, the bits are those of the head kernel switched off."""
    wce, B, inp = gpu_wce, 37, henv["inp"]
    env, kw = henv, {}
    if route == "matlab_split":
        kw = dict(semantics=wce.SEM_MATLAB)
    elif route.startswith("frame_cov"):
        kw = dict(rx_pre=henv["pre"][:B], mask=wce.PS_MMSE | wce.FRAME_COV,
                  semantics=wce.SEM_MATLAB if route.endswith("matlab") else wce.SEM_C)
    elif route == "noise":
        kw = dict(ow2=inp["ow2"] * 10.0 ** np.random.default_rng(0x0E8).uniform(-1.0, 1.0, B))
    else:
        env = dict(henv, ctx=wce.Context(inp["tx_pre"], inp["rx_pre"], inp["ow2"], wce.MMSE_REF))
    want = _mmse(wce, env, B, HEAD_OFF, **kw)
    assert np.isfinite(want).all()
    for v in (0,) + HEAD:
        assert np.array_equal(_bits(_mmse(wce, env, B, v, **kw)), _bits(want)), v


def test_plan_replay_default(gpu_wce, henv):
    """One replay of the default through a plan (captured graph): the direct call's bits, and variant 4's."""
    wce, ctx = gpu_wce, henv["ctx"]
    dtx, drx = wce.DeviceArray.from_numpy(henv["tx"]), wce.DeviceArray.from_numpy(henv["rx"])
    fr = ctx.frames(dtx, drx, NF)
    direct = _device_run(wce, ctx, fr, NF, 0, NF, N)
    replay = _device_run(wce, ctx, fr, NF, 0, NF, N, plan=True)
    assert np.array_equal(_bits(direct), _bits(replay))
    assert np.array_equal(_bits(direct), _bits(_mmse(wce, henv, NF, THREE_WGS)))
