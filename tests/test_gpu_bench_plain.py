"""bench.py's plain run (no --full): the headline line alone, --steps timed steps, and --dump-outputs.

Two plain runs with the same arguments (started side by side) must print the headline fields without any
of the --full sub-records and dump identical arrays: the steps run before and inside the timed region
depend on the arguments alone, and the training step is deterministic."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FULL_ONLY = ("roofline", "kernels", "kernels_sum_ms", "optimizer_params", "dp1_overhead", "c2p", "c5", "c5_online", "e2e", "c3",
             "cpu_baseline")


def test_plain_run_line_and_dump(tmp_path):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    dirs = [str(tmp_path / d) for d in ("a", "b")]
    procs = [subprocess.Popen([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "4", "--warmup", "2",
                               "--dump-outputs", d], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, cwd=ROOT)
             for d in dirs]
    outs = [p.communicate(timeout=240) for p in procs]
    for p, (out, err) in zip(procs, outs):
        assert p.returncode == 0, err[-4000:]
        lines = [ln for ln in out.splitlines() if ln.startswith("{")]
        assert len(lines) == 1, out[-2000:]
        res = json.loads(lines[0])
        assert res["unit"] == "samples/s" and res["higher_is_better"] is True and res["dtype"] == "f16" and res["metric"]
        assert res["steps"] == 4 and res["warmup"] == 2 and res["full"] is False
        assert res["ms_per_step"] > 0
        assert res["value"] == pytest.approx((1 << 18) / (res["ms_per_step"] * 1e-3), rel=1e-9)
        assert not [k for k in FULL_ONLY if k in res]
    a, b = ({f: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))} for d in dirs)
    assert sorted(a) == sorted(b) == ["mlp_gradients.npy", "params.npy"]
    assert sum(os.path.getsize(os.path.join(dirs[0], f)) for f in a) <= 64e6
    n_matrix = a["mlp_gradients.npy"].size
    assert a["params.npy"].shape == (3302400,) and n_matrix == 9216  # C2: every parameter, nothing sampled
    for f in a:
        assert a[f].dtype == np.float32 and np.array_equal(a[f], b[f]), f
    assert all(np.all(np.isfinite(v)) for v in a.values())
    grid = a["params.npy"][n_matrix:]
    assert np.count_nonzero(grid) > grid.size // 2 and np.count_nonzero(a["mlp_gradients.npy"]) > n_matrix // 4  # not empty buffers
