"""BASELINE configs[4] as named, at full size on one GPU: 1,048,576 frames,
all 5 estimators + per-symbol equalization, mixed precision (fp64 solve;
LT_LS / PS_Linear / PS_Cubic / PS_Sinc and the equalized symbols stored as
complex float, WCE_OUT_LS_F32), per-frame preambles, frames with their own
channels.  Since the closed-form rank-1 solve this request runs the LS pass
(ls_kernel), then mmse_rank1_kernel; the fusion into the MMSE solve
(mmse_solve_ls_kernel) runs behind wce_debug_set_variant(5, 1) only and is
tested by tests/test_rank1_routes_gpu.py (the "all" and "all_f32" requests in
C semantics, variant 1), not here.

Checks (main.c:66-212, WiFi_Equalization.m:1-9):
  * every output of every frame is finite (wce_nonfinite_scan);
  * sampled frames against the CPU oracle -- the LS family and equalization
    at 1e-6 (fp32 storage), PS_MMSE at 1e-10 against the
    long double closed form;
  * the batch split into the 8 wce_shard ranges of the 8-GPU run, each shard
    generating its frames from the global index, reproduces the single batch
    bit for bit (the N>1 data path, size-independently)."""
import importlib

import numpy as np
import pytest

from oracle_py import normrel

pytestmark = pytest.mark.gpu

N, NBLK = 53, 15
TOTAL, WORLD = 1 << 20, 8
TOL_F32, TOL = 1e-6, 1e-10


def _run(wce, ctx, first, count):
    tx, rx, pre = wce.DeviceArray((count, NBLK, N)), wce.DeviceArray((count, NBLK, N)), wce.DeviceArray((count, N))
    ctx.synth(tx, rx, pre, count, first_frame=first, seed=0x80211)
    outs = [wce.DeviceArray((count, N), np.complex64) for _ in range(4)] + [wce.DeviceArray((count, N))]
    eq = wce.DeviceArray((count, NBLK, N), np.complex64)
    o = wce.Outputs(*(x.addr for x in outs), eq.addr, N, NBLK * N, N, 0, wce.OUT_LS_F32)
    ctx.estimate(ctx.frames(tx, rx, count, rx_pre=pre), o, wce.ALL)
    wce.synchronize()
    return (tx, rx, pre), outs, eq


def test_config5_full_size(gpu_wce, golden, oracle):
    wce = gpu_wce
    multi = importlib.import_module("80211parallelestimation_amd.multi")
    inp = golden["inputs"]
    ctx = wce.Context(inp["tx_pre"], inp["rx_pre"], inp["ow2"], wce.MMSE_TEXTBOOK, device=0)
    (tx, rx, pre), outs, eq = _run(wce, ctx, 0, TOTAL)
    # 1. finite everywhere: the 4 fp32 LS outputs, fp64 MMSE, fp32 eq (15 rows per frame)
    for i, h in enumerate(outs):
        assert ctx.nonfinite_scan(h, TOTAL, f32=(i < 4))[1] == 0, i
    assert ctx.nonfinite_scan(eq, TOTAL * NBLK, f32=True)[1] == 0
    # 2. sampled frames against the oracle
    F = oracle.fmatrix()
    c = F @ (F.conj() @ oracle.lt_ls(inp["tx_pre"], inp["rx_pre"]) / N)
    rng = np.random.default_rng(0xC4)
    sample = np.concatenate([[0, 1, TOTAL // 2, TOTAL - 1], rng.choice(TOTAL, 60, replace=False)])
    for f in sample:
        t, r, p = tx.rows(f)[0], rx.rows(f)[0], pre.rows(f)[0]
        hls = oracle.lt_ls(inp["tx_pre"], p)
        lin = oracle.ps_linear(t[0], r[0])
        want = [hls, lin, oracle.ps_cubic(t[0], r[0]), oracle.ps_sinc(t[0], r[0])]
        for i in range(4):
            assert normrel(outs[i].rows(f)[0].astype(np.complex128), want[i]) < TOL_F32, (f, i)
        got = outs[4].rows(f)[0]
        assert normrel(got, oracle.mmse_textbook_closed(c, t[0], r[0], inp["ow2"])) < TOL, f
        e = eq.rows(f)[0].astype(np.complex128).reshape(-1)
        assert normrel(e, oracle.equalize(r, hls, lin).reshape(-1)) < TOL_F32, f
    # 3. the 8 shards of the 8-GPU run reproduce the batch bit for bit
    whole = [h.numpy() for h in outs]
    whole_eq = eq.numpy()
    del tx, rx, pre, outs, eq
    for rank in range(WORLD):
        first, count = multi.native_shard(wce, TOTAL, WORLD, rank)
        _, souts, seq = _run(wce, ctx, first, count)
        for i in range(5):
            assert np.array_equal(souts[i].numpy(), whole[i][first:first + count]), (rank, i)
        assert np.array_equal(seq.numpy(), whole_eq[first:first + count]), rank
        del souts, seq
