"""The NerfNetwork training pass (k_nerf_mlp_train, mlp.hip) reproduces recorded results bit for bit.

tests/golden/mlp_train_bits/ holds, per (config, n), the fp16 MLP gradient bits of one forward_backward at seeded
inputs and the SHA-256 of the network output and of dL/d(encoding), recorded by tools/mlp_train_bits.py from the
commit named in manifest.json. The kernel's LDS layout, its split of the dW tiles over the waves and its barriers may
change; which products are summed, and in which order, may not: every array must match exactly.

n = 100: one block with a partial tile and empty tiles; 4,133: several blocks, ragged; 36,901: on a 256-CU part some
blocks run two iterations and some one."""
import json
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import mlp_train_bits as mtb  # noqa: E402


@pytest.fixture(scope="module")
def pkg():
    from __graft_entry__ import load_package
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return load_package()


@pytest.fixture(scope="module")
def manifest():
    with open(os.path.join(mtb.GOLDEN, "manifest.json")) as f:
        return json.load(f)


@pytest.mark.parametrize("cfg,n", mtb.CASES)
def test_training_pass_bits(pkg, manifest, cfg, n):
    name = mtb.case_name(cfg, n)
    rec = manifest["cases"][name]
    want = np.load(os.path.join(mtb.GOLDEN, name + "_grad.npy"))
    assert want.dtype == np.uint16 and want.size == rec["n_matrix"] and mtb.sha(want) == rec["grad_sha256"]
    grad, out, denc = mtb.run_case(pkg, cfg, n)
    grad2, out2, denc2 = mtb.run_case(pkg, cfg, n)
    # two runs in one process agree with each other
    assert np.array_equal(grad, grad2) and np.array_equal(out, out2) and np.array_equal(denc, denc2)
    # and with the recorded run
    diff = np.nonzero(grad != want)[0]
    print(f"{name}: {diff.size} of {want.size} gradient halves differ from commit {manifest['commit'][:7]}")
    assert np.array_equal(grad, want), f"{name}: MLP gradient bits differ at {diff[:8].tolist()}"
    assert mtb.sha(out) == rec["out_sha256"], f"{name}: network output bits differ"
    assert mtb.sha(denc) == rec["denc_sha256"], f"{name}: dL/d(encoding) bits differ"
