"""bench.py --dump-outputs and the plain / --full split.

CPU: dump_outputs writes float64 (re, im) pairs of the whole H, or of a fixed
seeded sample of frames once the batch passes DUMP_LIMIT.  GPU: a plain run
times exactly --steps steps, carries none of the --full legs, and its dump is
the H an in-process wce_estimate(PS_MMSE) of the same seeded batch returns,
bit for bit (same kernel, same inputs, no atomics)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle_py import N, NBLK

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


class _HostArray:
    """the two DeviceArray methods dump_outputs uses, over a host array"""

    def __init__(self, a):
        self.a = a

    def numpy(self):
        return self.a.copy()

    def rows(self, first, count=1):
        return self.a[first:first + count].copy()


def _h(B):
    rng = np.random.default_rng(7)
    return rng.standard_normal((B, N)) + 1j * rng.standard_normal((B, N))


def test_dump_whole_batch(tmp_path):
    import bench
    h = _h(37)
    bench.dump_outputs(str(tmp_path / "d"), _HostArray(h), 37)
    assert os.listdir(tmp_path / "d") == ["ps_mmse.npy"]
    got = np.load(tmp_path / "d" / "ps_mmse.npy")
    assert got.dtype == np.float64 and got.shape == (37, N, 2)
    assert np.array_equal(got[..., 0], h.real) and np.array_equal(got[..., 1], h.imag)


def test_dump_samples_a_batch_over_the_limit(tmp_path, monkeypatch):
    import bench
    assert bench.DUMP_LIMIT <= 64_000_000
    assert 65536 * N * 16 <= bench.DUMP_LIMIT            # the default batch is dumped whole
    monkeypatch.setattr(bench, "DUMP_LIMIT", 4096 + 10 * (N * 16 + 8))
    h = _h(41)
    picks = []
    for name in ("a", "b"):
        bench.dump_outputs(str(tmp_path / name), _HostArray(h), 41)
        d = tmp_path / name
        idx = np.load(d / "ps_mmse_frames.npy")
        got = np.load(d / "ps_mmse.npy")
        assert idx.dtype == np.float64 and idx.shape == (10,) and np.all(np.diff(idx) > 0)
        assert got.dtype == np.float64 and got.shape == (10, N, 2)
        assert sum(os.path.getsize(d / f) for f in os.listdir(d)) <= 4096 + 10 * (N * 16 + 8)
        sel = h[idx.astype(np.int64)]
        assert np.array_equal(got[..., 0], sel.real) and np.array_equal(got[..., 1], sel.imag)
        picks.append(idx)
    assert np.array_equal(picks[0], picks[1])             # the same frames from run to run


def test_full_is_an_option_and_off_by_default(monkeypatch):
    import bench
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "4", "--warmup", "2"])
    a = bench.parse()
    assert a.full is False and a.dump_outputs is None and a.steps == 4 and a.warmup == 2
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "x"])
    a = bench.parse()
    assert a.full is True and a.dump_outputs == "x"


@pytest.mark.gpu
def test_plain_run_dumps_the_last_steps_h(gpu_wce, golden, tmp_path):
    wce, B = gpu_wce, 2048 + 37
    out = tmp_path / "dump"
    p = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--prewarm-s", "0.05", "--frames-per-gpu", str(B), "--dump-outputs", str(out)],
                       capture_output=True, text=True, timeout=120, cwd=str(tmp_path))
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1 and p.stdout.rstrip().endswith(lines[0])
    r = json.loads(lines[0])
    assert r["steps"] == 3 and r["warmup"] == 1 and r["ms_per_step"] > 0 and r["nonfinite_frames"] == 0
    assert abs(r["value"] - B / (r["ms_per_step"] * 1e-3)) / r["value"] < 1e-6
    assert r["unit"] == "frames/s" and r["higher_is_better"] is True and r["dtype"] == "f64"
    # none of the --full legs, no extras file
    assert "roofline" not in r and "cpu_baseline" not in r and not r["legs"] and r["extras_file"] is None
    assert os.listdir(tmp_path) == ["dump"]
    got = np.load(out / "ps_mmse.npy")
    assert got.dtype == np.float64 and got.shape == (B, N, 2)
    # the same seeded batch, estimated here
    inp = golden["inputs"]
    ctx = wce.Context(inp["tx_pre"], inp["rx_pre"], inp["ow2"], wce.MMSE_TEXTBOOK)
    hs = wce.DeviceArray.from_numpy(ctx.shared()[0])
    tx, rx = wce.DeviceArray((B, NBLK, N)), wce.DeviceArray((B, NBLK, N))
    ctx.synth(tx, rx, None, B, first_frame=0, seed=0x80211, h_shared=hs)
    H = wce.DeviceArray((B, N), zero=True)
    ctx.estimate(ctx.frames(tx, rx, B), wce.Outputs(None, None, None, None, H.addr, None, N, 0, 0, 0, 0), wce.PS_MMSE)
    wce.synchronize()
    want = H.numpy()
    assert np.isfinite(got).all()
    assert np.array_equal(got[..., 0], want.real) and np.array_equal(got[..., 1], want.imag)
