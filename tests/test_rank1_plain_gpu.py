"""mmse_rank1_kernel's build without mask and scale (csrc/wce_rank1.hip, PLAIN) against the general build.

Every TEXTBOOK State has acoef = 1.0 and a full xmask; a context caches that fact when it takes its State
(wce_ctx_create, wce_ctx_load_state, wce_ctx_mark_ready) and the default launch then runs a build that
neither reads nor applies them, and with a shared u issues its loads row by row (tx, u, rx).
WCE_VARIANT_R1 = 11 runs the general build under the default cache policy, 12 the build without mask and
scale in the general build's load order (tx and rx alternating, u last): both must repeat the default's bits.
REF contexts (a = 0, the four pilots) keep the general build whatever the variant; there the mask hides
1e200 garbage off the pilots, which a wrongly cached fact would let through.

Frames, contexts and helpers are test_rank1_persistent_gpu.py's and test_rank1_routes_gpu.py's."""
import numpy as np
import pytest

from oracle_py import N, NBLK, PILOTS, normrel
from test_rank1_persistent_gpu import TOL, _bits, _mmse, _variant, env  # noqa: F401
from test_rank1_routes_gpu import Env, _route_run, _run

pytestmark = pytest.mark.gpu

GENERAL, ALTERNATING = 11, 12
BUILDS = (0, GENERAL, ALTERNATING)
B = 257   # 16 full workgroups and one row


def _strided(wce, env, tx, rx, variant, block=3):
    """Block `block` of strided frames (block stride 60, 17 block slots per frame) into H rows of stride 61 in a
    buffer five rows longer than the batch; returns the whole buffer."""
    n, BS, FS, OS, EXTRA = tx.shape[0], 60, 17 * 60, 61, 5
    ftx = np.full((n, 17, BS), np.nan + 1j * np.nan, np.complex128)
    frx = np.full_like(ftx, np.nan + 1j * np.nan)
    ftx[:, :NBLK, :N], frx[:, :NBLK, :N] = tx, rx
    dtx, drx = wce.DeviceArray.from_numpy(ftx), wce.DeviceArray.from_numpy(frx)
    fr = env["ctx"].frames(dtx, drx, n, frame_stride=FS, block_stride=BS, block=block)
    sent = np.full((n + EXTRA, OS), 7.0 - 3.0j, np.complex128)
    dH = wce.DeviceArray.from_numpy(sent)
    with _variant(wce, variant):
        env["ctx"].estimate(fr, wce.Outputs(None, None, None, None, dH.addr, None, OS, 0, 0, 0, 0), wce.PS_MMSE)
        wce.synchronize()
    out = dH.numpy()
    assert np.array_equal(_bits(out[:n, N:]), _bits(sent[:n, N:])), variant
    assert np.array_equal(_bits(out[n:]), _bits(sent[n:])), variant
    return out[:n, :N]


def test_plain_build_repeats_the_general_build(gpu_wce, env, oracle):
    """257 frames, block 3 of strided frames: the default (no mask, no scale, loads row by row), the general
    build and the build without mask and scale in its load order, bit for bit, and the long double closed form
    at 1e-10."""
    tx, rx = env["tx"][:B], env["rx"][:B]
    got = {v: _strided(gpu_wce, env, tx, rx, v) for v in BUILDS}
    assert np.isfinite(got[0]).all()
    for v in BUILDS[1:]:
        assert np.array_equal(_bits(got[v]), _bits(got[0])), v
    exp = np.stack([oracle.mmse_textbook_closed(env["c"], tx[f, 3], rx[f, 3], env["inp"]["ow2"]) for f in range(0, B, 8)])
    err = normrel(got[0][::8], exp)
    assert err.max() < TOL, (int(err.argmax()), err.max())


def test_nonfinite_inputs_mark_the_same_entries(gpu_wce, env):
    """A NaN or an Inf in one entry of tx or rx: every build leaves the same output entries non-finite, and
    every other frame keeps its bits."""
    tx, rx = np.array(env["tx"][:B]), np.array(env["rx"][:B])
    clean = _strided(gpu_wce, env, tx, rx, 0)
    hit = {5: (tx, np.nan), 16: (rx, np.inf), 100: (tx, -np.inf), 101: (rx, np.nan + 1j * np.nan), 256: (tx, np.inf * 1j)}
    for k, (f, (a, v)) in enumerate(hit.items()):
        a[f, 3, (7 * k + 3) % N] = v
    a = tx[200, 3]
    a[50] = np.nan   # subcarriers 48..52: the lane-masked loads
    got = {v: _strided(gpu_wce, env, tx, rx, v) for v in BUILDS}
    bad = sorted(list(hit) + [200])
    good = np.setdiff1d(np.arange(B), bad)
    for v in BUILDS:
        assert np.array_equal(np.isfinite(got[v].real), np.isfinite(got[0].real)), v
        assert np.array_equal(np.isfinite(got[v].imag), np.isfinite(got[0].imag)), v
        assert np.array_equal(_bits(got[v][good]), _bits(clean[good])), v
        assert not np.isfinite(got[v][bad]).all(axis=1).any(), v


def test_small_batches_and_routes(gpu_wce, env):
    """1, 4, 5, 17 and 37 frames on the shared-u route, and MATLAB split, FRAME_COV and per-frame noise (a zero
    and an infinite entry) at 37: the three builds agree bit for bit."""
    wce = gpu_wce
    for n in (1, 4, 5, 17, 37):
        ref = _mmse(wce, env, n, GENERAL)
        for v in (0, ALTERNATING):
            assert np.array_equal(_bits(_mmse(wce, env, n, v)), _bits(ref)), (n, v)
    rng = np.random.default_rng(0x0E8)
    ow2 = env["inp"]["ow2"] * 10.0 ** rng.uniform(-1.0, 1.0, 37)
    ow2[13], ow2[30] = 0.0, np.inf
    routes = {"split": dict(semantics=wce.SEM_MATLAB),
              "frame_cov": dict(rx_pre=env["pre"][:37], mask=wce.PS_MMSE | wce.FRAME_COV),
              "frame_cov split": dict(rx_pre=env["pre"][:37], mask=wce.PS_MMSE | wce.FRAME_COV, semantics=wce.SEM_MATLAB),
              "noise": dict(ow2=ow2),
              "noise frame_cov": dict(ow2=ow2, rx_pre=env["pre"][:37], mask=wce.PS_MMSE | wce.FRAME_COV)}
    for name, kw in routes.items():
        ref = _mmse(wce, env, 37, GENERAL, **dict(kw))
        assert np.isfinite(ref[0]).all(), name
        for v in (0, ALTERNATING):
            assert np.array_equal(_bits(_mmse(wce, env, 37, v, **dict(kw))), _bits(ref)), (name, v)
        if "ow2" in kw:
            assert np.isnan(ref[[13, 30]].real).all() and np.isfinite(np.delete(ref, [13, 30], axis=0)).all()


def test_loaded_state_carries_the_fact(gpu_wce, golden, oracle, env):
    """wce_ctx_load_state on an empty context (the multi-GPU broadcast path): a TEXTBOOK blob gives the bits of
    the directly built context, and so does a REF blob -- whose mask must still hide garbage off the pilots."""
    wce, inp = gpu_wce, golden["inputs"]
    # TEXTBOOK
    direct = _mmse(wce, env, 37, 0)
    loaded = wce.Context(empty=True)
    loaded.load_state(wce.state_blob(inp["tx_pre"], inp["rx_pre"], inp["ow2"], wce.MMSE_TEXTBOOK))
    for v in (0, GENERAL):
        with _variant(wce, v):
            got = loaded.estimate_host(env["tx"][:37], env["rx"][:37], mask=wce.PS_MMSE)["ps_mmse"]
        assert np.array_equal(_bits(got), _bits(direct)), v
    # REF, border dot off under FRAME_COV: rank1_s's given-w branch, a = 0, the four pilots
    renv = Env(wce, golden, oracle)
    name = "ref_bdot_off-frame_cov"
    rng = np.random.default_rng(0x6B)
    junk = np.array(renv.tx)
    off = np.setdiff1d(np.arange(N), PILOTS)
    junk[:, :, off] = 1e200 * (rng.choice([-1.0, 1.0], junk[:, :, off].shape) + 1j * rng.choice([-1.0, 1.0], junk[:, :, off].shape))
    want = _route_run(renv, name, "mmse", "C", 0)["ps_mmse"]
    assert np.isfinite(want).all()
    assert np.array_equal(_bits(_route_run(renv, name, "mmse", "C", 0, tx=junk)["ps_mmse"]), _bits(want))
    ref_loaded = wce.Context(empty=True)
    ref_loaded.load_state(wce.state_blob(inp["tx_pre"], inp["rx_pre"], inp["ow2"], wce.MMSE_REF))
    renv.ctx["ref"] = ref_loaded
    for v in BUILDS:
        for tx in (None, junk):
            got = _route_run(renv, name, "mmse", "C", v, tx=tx)["ps_mmse"]
            assert np.array_equal(_bits(got), _bits(want)), (v, tx is junk)
    # the same context, given the TEXTBOOK State afterwards, follows it
    ref_loaded.load_state(wce.state_blob(inp["tx_pre"], inp["rx_pre"], inp["ow2"], wce.MMSE_TEXTBOOK))
    got = ref_loaded.estimate_host(env["tx"][:37], env["rx"][:37], mask=wce.PS_MMSE)["ps_mmse"]
    assert np.array_equal(_bits(got), _bits(direct))


def test_plan_replay_default(gpu_wce, env):
    """One replay of the default through a plan (captured graph): the direct call's bits."""
    wce = gpu_wce
    direct = _run(wce, env["ctx"], env["tx"][:37], env["rx"][:37], wce.PS_MMSE, wce.SEM_C)["ps_mmse"]
    replay = _run(wce, env["ctx"], env["tx"][:37], env["rx"][:37], wce.PS_MMSE, wce.SEM_C, plan=True)["ps_mmse"]
    assert np.array_equal(_bits(direct), _bits(replay))
    assert np.array_equal(_bits(direct), _bits(_mmse(wce, env, 37, GENERAL)))
