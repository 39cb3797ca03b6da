"""The two entries that run a whole training step share the tail that chooses the fused optimizer update, builds it and
finishes the step (ngp_trainer::step_tail / finish_step): ngp_trainer_training_step (forward, loss, backward,
optimizer in one call) and ngp_forward -> ngp_loss_evaluate -> ngp_trainer_train_step. From the same seed, targets and
loss scale they must leave the same bits, in either optimizer layout (NGP_LAZY_EMA, as test_gpu_lazy_ema.py selects
it): with the lazy layout the update runs fused in the backward, with the eager arrays as the separate launch."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

N = 4096
STEPS = 3
LOSS_SCALE = 128.0
ENCODING = {"otype": "HashGrid", "n_levels": 4, "n_features_per_level": 2, "log2_hashmap_size": 14, "base_resolution": 8,
            "per_level_scale": 2.0}
NETWORK = {"otype": "FullyFusedMLP", "activation": "ReLU", "output_activation": "None", "n_neurons": 64, "n_hidden_layers": 2}


@pytest.fixture(scope="module")
def pkg():
    from __graft_entry__ import load_package
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return load_package()


def make_trainer(pkg, lazy):
    old = os.environ.get("NGP_LAZY_EMA")
    os.environ["NGP_LAZY_EMA"] = "1" if lazy else "0"
    try:
        net = pkg.NetworkWithInputEncoding(3, 1, ENCODING, NETWORK)
        net.set_option("grid_backward_mode", 3)  # the bucketed backward's exact sums at this batch size
        tr = pkg.Trainer(net, pkg.SDF_BASE["optimizer"], seed=1337)
    finally:
        if old is None:
            del os.environ["NGP_LAZY_EMA"]
        else:
            os.environ["NGP_LAZY_EMA"] = old
    return net, tr


def batch(step):
    g = np.random.default_rng(500 + step)
    x = g.random((N, 3)).astype(np.float32)
    t = g.uniform(-1, 1, (N, 1)).astype(np.float32)
    return torch.from_numpy(x).cuda(), torch.from_numpy(t).cuda()


def state(tr):
    torch.cuda.synchronize()
    return (tr.params.cpu().numpy().view(np.uint16).copy(),
            tr.params_full_precision.cpu().numpy().view(np.uint32).copy(), tr.step)


@pytest.mark.parametrize("lazy", [False, True])
def test_training_step_and_train_step_agree_bitwise(pkg, lazy):
    net_a, tr_a = make_trainer(pkg, lazy)
    net_b, tr_b = make_trainer(pkg, lazy)
    for tr in (tr_a, tr_b):
        assert tr.fused_update_active(N) == lazy
    for step in range(STEPS):
        x, target = batch(step)
        tr_a.training_step(x, target, loss="L2", loss_scale=LOSS_SCALE, run_optimizer=True)
        out = torch.zeros((N, 16), dtype=torch.float16, device="cuda")
        ctx, _ = net_b.forward(x, output=out)
        dl, _, _ = pkg.loss_evaluate("L2", out, target, 1, loss_scale=LOSS_SCALE)
        tr_b.train_step(x, dl, loss_scale=LOSS_SCALE)
        del ctx
    p_a, w_a, s_a = state(tr_a)
    p_b, w_b, s_b = state(tr_b)
    assert s_a == s_b == STEPS
    np.testing.assert_array_equal(p_a, p_b)
    np.testing.assert_array_equal(w_a, w_b)
