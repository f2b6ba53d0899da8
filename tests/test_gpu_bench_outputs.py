"""bench.py as the driver runs it (``--gpus 1 --steps K --warmup W``), once, with --dump-outputs:
the plain run's result line carries the headline fields and none of the --full passes' figures,
--steps sets the number of timed steps, and the dumped arrays are what the last timed step left.

The fused step is deterministic (test_prepared_steps_equal_train_steps), so the dump is compared
bit for bit with W + K steps of an engine set up here the way bench.py sets its own up; W + K - 1
steps must differ, or the comparison would not see a miscounted step."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, S, D, Z, H = 1024, 100, 6, 8, 128
K, W = 3, 1


def _bench_state(steps):
    """(loss, params) after ``steps`` fused steps of bench.py's cfg2 set-up (its seeds)."""
    from cvae_amd import ConditionalTrajectoryVAE
    torch.manual_seed(0)
    model = ConditionalTrajectoryVAE(S, D, Z, H, 4, 4, n_classes=0, class_dim=16)
    eng = model.attach(dtype="bf16", max_batch=B, device="cuda:0", seed=4321)
    x = eng.as_input(torch.randn(B, S, D, generator=torch.Generator().manual_seed(1234)))
    eng.train_steps(x, steps, batch=B)
    torch.cuda.synchronize()
    return eng.loss.float().cpu().numpy(), eng.params.float().cpu().numpy()


def test_plain_run_line_and_dumped_outputs(tmp_path):
    out = tmp_path / "dump"
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(K),
                        "--warmup", str(W), "--dump-outputs", str(out)], capture_output=True, text=True, timeout=240)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = p.stdout.strip().splitlines()
    assert len(lines) == 1
    res = json.loads(lines[0])
    assert res["metric"] == "trajectories/sec per ELBO step, batch=1024 seq_len=100; 1/2/4/8 MI355X"
    assert res["unit"] == "trajectories/s" and res["higher_is_better"] is True and res["dtype"] == "bf16"
    assert res["steps"] == K and res["warmup"] == W and res["n_gpus"] == 1
    assert res["ms_per_step"] > 0
    # value and ms_per_step are the same measurement (both rounded in the line: 1e-5 ms, 0.1 traj/s)
    assert res["value"] == pytest.approx(B / (res["ms_per_step"] * 1e-3), rel=1e-5 / res["ms_per_step"] + 1e-6)
    for key in ("roofline", "cpu_baseline", "speedup_vs_cpu"):  # measured in passes of their own: --full only
        assert key not in res
    assert sorted(os.listdir(out)) == ["loss.npy", "params.npy"]
    loss, params = np.load(out / "loss.npy"), np.load(out / "params.npy")
    assert loss.dtype == np.float32 and params.dtype == np.float32
    assert loss.shape == (5,) and params.shape == (275432,)
    assert np.isfinite(loss).all() and np.isfinite(params).all()
    want_loss, want_params = _bench_state(W + K)
    np.testing.assert_array_equal(loss, want_loss)
    np.testing.assert_array_equal(params, want_params)
    short_loss, short_params = _bench_state(W + K - 1)
    assert not np.array_equal(loss, short_loss) and not np.array_equal(params, short_params)
