"""bench.py --dump-outputs: the last timed step's outputs as .npy files, next to the result line."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu


def test_dump_outputs_writes_the_last_step(cuda, tmp_path):
    """One plain 1-GPU run (a 1-layer model): ``--steps`` timed steps, ``ms_per_step`` in the result
    line, and the step's statistics, gradient norm and the sampled parameters / gradients on disk as
    float64 / float32 arrays of at most 64 MB in all."""
    out_dir = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
                        "--layers", "1", "--dump-outputs", str(out_dir)], capture_output=True, text=True, timeout=300,
                       cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr[-3000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["steps"] == 2 and out["warmup"] == 1 and out["unit"] == "s/step" and out["higher_is_better"] is False
    assert out["ms_per_step"] > 0 and abs(out["ms_per_step"] - out["value"] * 1000) < 2e-3

    sys.path.insert(0, ROOT)
    try:
        import bench
    finally:
        sys.path.remove(ROOT)
    got = {f: np.load(str(out_dir / f)) for f in sorted(os.listdir(str(out_dir)))}
    assert sorted(got) == ["grad_norm.npy", "grads.npy", "params.npy", "step_stats.npy"]
    assert sum(a.nbytes for a in got.values()) <= 64 << 20
    stats, gnorm = got["step_stats.npy"], got["grad_norm.npy"]
    assert stats.dtype == np.float64 and stats.shape == (4,) and np.isfinite(stats).all()
    loss, nll, ntokens, nsentences = stats
    # sample_size (and with it nsentences) is len(sample[0][0]) as in the reference: the sequence length
    assert nsentences == 128 and ntokens >= 0 and nll == loss
    # logged as batch loss / (sample_size ln 2); a random-init model's batch loss is about
    # ln 30522 + ln 2 = 11.0 nats (MLM over the vocabulary + NSP)
    assert 8.0 < loss * 128 * np.log(2.0) < 16.0
    assert gnorm.dtype == np.float64 and gnorm.shape == (1,) and np.isfinite(gnorm).all() and gnorm[0] > 0
    for name in ("params.npy", "grads.npy"):
        a = got[name]
        assert a.dtype == np.float32 and a.shape == (bench.DUMP_SAMPLE,) and np.isfinite(a).all()
        assert np.count_nonzero(a) > a.size // 100
    # grad_norm is the norm of the whole gradient buffer times 1 / sample_size: the sampled positions
    # (distinct ones) cannot hold more than that
    assert float(np.sqrt((got["grads.npy"].astype(np.float64) ** 2).sum())) <= gnorm[0] * 128 * (1 + 1e-3)
