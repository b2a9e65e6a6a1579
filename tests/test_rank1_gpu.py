"""GPU checks of the closed-form rank-1 PS_MMSE (mmse_rank1_kernel, csrc/wce_rank1.hip):
the TEXTBOOK headline, WCE_MMSE_FRAME_COV in C and MATLAB semantics, the
factorising kernel as variant 1, bit stability under batching, and the
LS-family request that used to run fused.

Oracle: the long double closed form (oracle_py.mmse_textbook_closed) at the
project's 1e-10 norm-relative.  Frames are host-made (tests/test_rank1_model.py):
BPSK, QPSK and 16-QAM symbols at the inputs.h amplitude (cond(Ryy) = 4.3e6)
with a DC null, on the preamble's channel ("matched") and on per-frame random
channels; frame f of the shared batch is class f % 6.

Measured on an MI355X (max norm-relative error over the 261 shared frames):
BPSK matched 3.8e-13, unrelated 3.7e-13 (the oracle's own cancellation in
long double); QPSK matched 7.3e-12, unrelated 2.1e-15; 16-QAM matched 2.6e-12,
unrelated 2.9e-15; nulls and |x_k| down to 1e-150 on a matched channel
3.9e-11; FRAME_COV 4.9e-13 (C), 1.0e-12 (MATLAB).  The closed form against
the factorising kernel (variant 1): BPSK 9.6e-14, QPSK 3.5e-12, 16-QAM 5.2e-12."""
import numpy as np
import pytest

from oracle_py import N, NBLK, normrel
from test_rank1_model import make_frames

pytestmark = pytest.mark.gpu

TOL = 1e-10
KINDS = ("bpsk", "qpsk", "qam16")
NF = 261
R1 = 5   # WCE_VARIANT_R1


def _cvec(oracle, F, tx_pre, rx_pre, matlab=False):
    hls = oracle.matlab_lt_ls(tx_pre, rx_pre) if matlab else oracle.lt_ls(tx_pre, rx_pre)
    return F @ (F.conj() @ hls / N)


def _mixed(rng, hlt, ow2, n, classes=tuple((k, m) for k in KINDS for m in (True, False))):
    """[n][15][53] frames, every block its own symbols; frame f is class f % len(classes)."""
    tx = np.zeros((n, NBLK, N), np.complex128)
    rx = np.zeros_like(tx)
    for ci, (kind, matched) in enumerate(classes):
        idx = np.arange(ci, n, len(classes))
        if idx.size == 0:
            continue
        t, r = make_frames(rng, kind, matched, hlt, ow2, n=idx.size * NBLK)
        tx[idx], rx[idx] = t.reshape(idx.size, NBLK, N), r.reshape(idx.size, NBLK, N)
    return tx, rx


@pytest.fixture(scope="module")
def env(gpu_wce, golden, oracle):
    """One context, NF mixed frames and their long double answers (block 0), shared and left unchanged."""
    inp = golden["inputs"]
    F = oracle.fmatrix()
    ctx = gpu_wce.Context(inp["tx_pre"], inp["rx_pre"], inp["ow2"], gpu_wce.MMSE_TEXTBOOK)
    hlt = np.asarray(oracle.lt_ls(inp["tx_pre"], inp["rx_pre"]), np.complex128)
    c = _cvec(oracle, F, inp["tx_pre"], inp["rx_pre"])
    tx, rx = _mixed(np.random.default_rng(0xB1), hlt, inp["ow2"], NF)
    ref = np.stack([oracle.mmse_textbook_closed(c, tx[f, 0], rx[f, 0], inp["ow2"]) for f in range(NF)])
    for a in (tx, rx, ref):
        a.setflags(write=False)
    return dict(inp=inp, F=F, ctx=ctx, hlt=hlt, c=c, tx=tx, rx=rx, ref=ref)


def _mmse(wce, ctx, tx, rx, **kw):
    return ctx.estimate_host(tx, rx, mask=kw.pop("mask", wce.PS_MMSE), **kw)["ps_mmse"]


@pytest.mark.parametrize("B", [1, 3, 4, 5, 63, 64, 65, 257])
def test_batches_against_closed_form(gpu_wce, env, B):
    """Partial 16-lane rows of a wave (1, 3, 5), whole waves (4), partial and
    more than one workgroup (63..65: 16 units per workgroup; 257)."""
    out = _mmse(gpu_wce, env["ctx"], env["tx"][:B], env["rx"][:B])
    err = normrel(out, env["ref"][:B])
    print(f"\nB={B}: max {err.max():.2e} (frame {int(err.argmax())}, class {int(err.argmax()) % 6})")
    assert err.max() < TOL, (int(err.argmax()), err.max())


def test_per_class_maxima(gpu_wce, env):
    """The figure the record keeps: the worst frame of each class on the GPU."""
    out = _mmse(gpu_wce, env["ctx"], env["tx"], env["rx"])
    err = normrel(out, env["ref"])
    names = [f"{k} {'matched' if m else 'unrelated'}" for k in KINDS for m in (True, False)]
    for ci, nm in enumerate(names):
        print(f"\n{nm}: max {err[ci::6].max():.2e}", end="")
    assert err.max() < TOL, (int(err.argmax()), err.max())


def test_block3_strided_frames_and_out_stride_61(gpu_wce, env, oracle):
    """block = 3 of frames laid out with gaps (block stride 60, 17 block slots
    per frame) and H rows of stride 61: the columns past 52 stay untouched."""
    wce, ctx, inp = gpu_wce, env["ctx"], env["inp"]
    B, BS, FS, OS = 37, 60, 17 * 60, 61
    tx = np.full((B, 17, BS), np.nan + 1j * np.nan, np.complex128)
    rx = np.full_like(tx, np.nan + 1j * np.nan)
    tx[:, :NBLK, :N], rx[:, :NBLK, :N] = env["tx"][:B], env["rx"][:B]
    Hh = np.full((B, OS), 7.0 - 3.0j, np.complex128)
    dtx, drx, dH = wce.DeviceArray.from_numpy(tx), wce.DeviceArray.from_numpy(rx), wce.DeviceArray.from_numpy(Hh)
    fr = ctx.frames(dtx, drx, B, frame_stride=FS, block_stride=BS, block=3)
    ctx.estimate(fr, wce.Outputs(None, None, None, None, dH.addr, None, OS, 0, 0, 0, 0), wce.PS_MMSE)
    wce.synchronize()
    got = dH.numpy()
    assert np.all(got[:, N:] == 7.0 - 3.0j)
    exp = np.stack([oracle.mmse_textbook_closed(env["c"], env["tx"][f, 3], env["rx"][f, 3], inp["ow2"])
                    for f in range(B)])
    err = normrel(got[:, :N], exp)
    assert err.max() < TOL, err.max()
    # the same frames, densely laid out: the same bits
    assert np.array_equal(got[:, :N], _mmse(wce, ctx, env["tx"][:B], env["rx"][:B], block=3))


def test_nulls_zero_frame_and_tiny_symbols(gpu_wce, env, oracle):
    wce, ctx, inp, hlt = gpu_wce, env["ctx"], env["inp"], env["hlt"]
    rng = np.random.default_rng(0x52)
    n = 8
    tx, rx = _mixed(rng, hlt, inp["ow2"], n, classes=(("qpsk", True),))
    tx[1, :, ::5] = 0.0                        # more nulls than the DC bin
    tx[2], rx[2] = 0.0, 0.0                    # an all-zero frame
    scale = np.logspace(0, -150, N)            # |x_k| down to 1e-150 (x^2 stays normal)
    for f in range(3, n):
        tx[f, 0] *= rng.permutation(scale)
        rx[f, 0] = hlt * tx[f, 0] + np.sqrt(inp["ow2"] / 2.0) * (rng.standard_normal(N) + 1j * rng.standard_normal(N))
    out = _mmse(wce, ctx, tx, rx)
    assert np.isfinite(out).all()
    assert np.all(out[2] == 0.0), "all-zero frame: s = 0, H = 0"
    live = [0, 1, 3, 4, 5, 6, 7]
    exp = np.stack([oracle.mmse_textbook_closed(env["c"], tx[f, 0], rx[f, 0], inp["ow2"]) for f in live])
    err = normrel(out[live], exp)
    print(f"\nnulls / tiny symbols: max {err.max():.2e}")
    assert err.max() < TOL, err


@pytest.mark.parametrize("sem", ["C", "MATLAB"])
def test_frame_cov_textbook(gpu_wce, env, oracle, sem):
    """WCE_MMSE_FRAME_COV: u_f from each frame's own preamble, drawn
    independently of the frame's data.  C semantics: block 0; MATLAB semantics
    (split, 4 blocks): the mean of the 4 per-block closed forms."""
    wce, ctx, inp, F = gpu_wce, env["ctx"], env["inp"], env["F"]
    B = 37
    rng = np.random.default_rng(0xFC0)
    amp = np.sqrt(np.mean(np.abs(env["hlt"]) ** 2) / 2.0)
    hp = amp * (rng.standard_normal((B, N)) + 1j * rng.standard_normal((B, N)))
    pre = hp * inp["tx_pre"] + np.sqrt(inp["ow2"] / 2.0) * (rng.standard_normal((B, N)) + 1j * rng.standard_normal((B, N)))
    tx, rx = env["tx"][:B], env["rx"][:B]
    ml = sem == "MATLAB"
    ctx.reserve(B)
    out = _mmse(wce, ctx, tx, rx, rx_pre=pre, mask=wce.PS_MMSE | wce.FRAME_COV,
                semantics=wce.SEM_MATLAB if ml else wce.SEM_C)
    exp = []
    for f in range(B):
        cf = _cvec(oracle, F, inp["tx_pre"], pre[f], matlab=ml)
        per = [oracle.mmse_textbook_closed(cf, tx[f, b], rx[f, b], inp["ow2"]) for b in range(4 if ml else 1)]
        exp.append(np.mean(np.stack(per), axis=0))
    err = normrel(out, np.stack(exp))
    print(f"\nFRAME_COV {sem}: max {err.max():.2e}")
    assert err.max() < TOL, (int(err.argmax()), err.max())


@pytest.mark.parametrize("kind", KINDS)
def test_variant_factorisation_agrees(gpu_wce, env, kind):
    """WCE_VARIANT_R1 = 1 (mmse_solve_fc_kernel, the 53 x 53 factorisation)
    against the default on 257 frames of one modulation, matched and unrelated
    channels alternating: 1e-11, as test_border_dot_matches_backsolve_path."""
    wce, ctx, inp = gpu_wce, env["ctx"], env["inp"]
    lib = wce.load()
    rng = np.random.default_rng([0xAB, KINDS.index(kind)])
    tx, rx = _mixed(rng, env["hlt"], inp["ow2"], 257, classes=((kind, True), (kind, False)))
    got = {}
    try:
        for v in (0, 1, 2):
            assert lib.wce_debug_set_variant(R1, v) == 0
            got[v] = _mmse(wce, ctx, tx, rx)
    finally:
        assert lib.wce_debug_set_variant(R1, 0) == 0
    d = normrel(got[1], got[0])
    print(f"\n{kind}: closed form vs factorisation max {d.max():.2e}")
    assert np.array_equal(got[0], got[2]), "nontemporal build: the same bits"
    assert d.max() < 1e-11, (int(d.argmax()), d.max())


def _device_run(wce, ctx, tx, rx, plan=False):
    B = tx.shape[0]
    dtx, drx = wce.DeviceArray.from_numpy(tx), wce.DeviceArray.from_numpy(rx)
    dH = wce.DeviceArray((B, N), zero=True)
    fr = ctx.frames(dtx, drx, B)
    o = wce.Outputs(None, None, None, None, dH.addr, None, N, 0, 0, 0, 0)
    if plan:
        p = ctx.plan(fr, o, wce.PS_MMSE)
        p.launch()
        wce.synchronize()
        p.close()
    else:
        ctx.estimate(fr, o, wce.PS_MMSE)
        wce.synchronize()
    return dH.numpy()


def test_bits_do_not_depend_on_batching(gpu_wce, env):
    """A frame's output bits depend on its own data only: 261 frames at once =
    the same frames as 1 + 4 + 256, = frames [5:] estimated alone, = a plan replay."""
    wce, ctx = gpu_wce, env["ctx"]
    tx, rx = np.array(env["tx"]), np.array(env["rx"])
    whole = _device_run(wce, ctx, tx, rx)
    parts = np.concatenate([_device_run(wce, ctx, tx[a:b], rx[a:b]) for a, b in ((0, 1), (1, 5), (5, 261))])
    assert np.array_equal(whole, parts)
    assert np.array_equal(whole[5:], _device_run(wce, ctx, tx[5:], rx[5:]))
    assert np.array_equal(whole, _device_run(wce, ctx, tx, rx, plan=True))
    assert normrel(whole, env["ref"]).max() < TOL


@pytest.mark.parametrize("fc", [False, True], ids=["shared", "frame_cov"])
def test_ls_request_equals_mmse_alone(gpu_wce, env, fc):
    """mask = ALL used to run the fused solve; with the closed form it runs the
    LS pass, then mmse_rank1_kernel: PS_MMSE is bit for bit what PS_MMSE alone gives."""
    wce, ctx, inp = gpu_wce, env["ctx"], env["inp"]
    B = 130
    rng = np.random.default_rng(0x130)
    pre = env["hlt"] * inp["tx_pre"] + np.sqrt(inp["ow2"] / 2.0) * (rng.standard_normal((B, N)) + 1j * rng.standard_normal((B, N)))
    tx, rx = env["tx"][:B], env["rx"][:B]
    extra = wce.FRAME_COV if fc else 0
    ctx.reserve(B)
    alone = ctx.estimate_host(tx, rx, rx_pre=pre, mask=wce.PS_MMSE | extra)["ps_mmse"]
    fused = ctx.estimate_host(tx, rx, rx_pre=pre, mask=wce.ALL | extra)
    assert np.array_equal(fused["ps_mmse"], alone)
    assert np.isfinite(fused["ps_linear"]).all() and np.isfinite(fused["eq"]).all()
    if not fc:
        assert normrel(alone, env["ref"][:B]).max() < TOL
