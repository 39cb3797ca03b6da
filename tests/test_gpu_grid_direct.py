"""Direct levels and the inline plan of the bucketed grid backward (csrc/grid_scatter.hip).

A level of at most two buckets (ScatterPlan::direct_mask; C2's level 0, the 2D grid's levels 0-2) is not sorted
into items: direct part blocks of k_sc_accumulate, one per (direct bucket, range of grid_direct_part samples),
recompute the contributions, sum them in LDS and store slabs that k_sc_split_reduce adds (model option
grid_direct). Where the bucket list is small, k_sc_plan is not launched and every consumer derives the bucket
starts and the split lists from the bucket totals (model option grid_plan_inline). Both keep the contributions
and their exact fixed-point sums, so every comparison here is on the bit patterns: against the oracle's
contribution-exact backward, and against the same engine with both options off. The batches are small on
purpose (the bucketed threshold 4096, one more, a second direct part holding one sample, three ragged parts);
the positions are a concentrated cloud plus cell boundaries, the unit cube's upper faces and points outside it.
"""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

MLP2 = {"otype": "FullyFusedMLP", "activation": "ReLU", "output_activation": "None", "n_neurons": 64, "n_hidden_layers": 2}
ADAM = {"otype": "Adam", "learning_rate": 1e-2, "beta1": 0.9, "beta2": 0.99, "epsilon": 1e-15, "l2_reg": 1e-6}
ON = {"grid_direct": 1, "grid_plan_inline": 1}
OFF = {"grid_direct": 0, "grid_plan_inline": 0}


@pytest.fixture(scope="module")
def pkg():
    from __graft_entry__ import load_package
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return load_package()


def enc_cfg(L, F, T):
    return {"otype": "HashGrid", "n_levels": L, "n_features_per_level": F, "log2_hashmap_size": T, "base_resolution": 16,
            "per_level_scale": 2.0}


def encoding_width(L, F):
    return (L * F + 15) // 16 * 16


def positions(n, D, seed):
    """A concentrated cloud (hot coarse entries) with a uniform fifth, plus the edge cases of test_gpu_grid_exact.py."""
    g = np.random.default_rng(seed)
    x = np.clip(0.5 + 0.06 * g.standard_normal((n, D)), 0.0, 1.0).astype(np.float32)
    m = g.random(n) < 0.2
    x[m] = g.random((int(m.sum()), D), dtype=np.float32)
    x[:64] = np.round(x[:64] * 4) / 4      # exact cell boundaries
    x[64:72] = 1.0                         # the upper faces
    x[72:80] = np.float32(1.0 + 1e-3)      # outside the unit cube (tcnn wraps the index)
    x[80:88] = np.float32(-1e-2)
    return x


def dy_batch(n, L, F, seed, zero_levels=()):
    g = np.random.default_rng(seed)
    dy = np.zeros((n, encoding_width(L, F)), np.float16)
    dy[:, :L * F] = g.uniform(-1, 1, (n, L * F)).astype(np.float16)
    for l in zero_levels:
        dy[:, l * F:(l + 1) * F] = 0
    return dy


def direct_part(pkg, D=3, L=4, F=4, T=19):
    net = pkg.NetworkWithInputEncoding(D, 1, enc_cfg(L, F, T), MLP2)
    s = int(net.query("grid_direct_part"))
    assert s >= 4096
    return s


def sizes(S):
    return (4096, 4097, S + 1, 3 * S - 5)


def backward(pkg, D, L, F, T, x, dy, opts, grad_mode=None, init=None, ml=None, soa=False):
    """encoding_backward on a fresh model: (grid_direct_levels, grid_plan_inline, gradient bits of the grid)."""
    net = pkg.NetworkWithInputEncoding(D, 1, enc_cfg(L, F, T), MLP2)
    for k, v in opts.items():
        net.set_option(k, v)
    tr = pkg.Trainer(net, ADAM)
    nm = net.n_matrix_params
    if init is not None:
        tr.gradients[nm:] = torch.from_numpy(init.view(np.float16)).cuda()
    mlt = None
    if ml is not None:
        mlt = torch.from_numpy(ml).cuda()
        net.set_max_level(1.0, mlt)
    kw = {} if grad_mode is None else {"grad_mode": grad_mode}
    if soa:
        dyt = torch.from_numpy(np.ascontiguousarray(dy.T)).cuda()  # [W x n]
        kw["layout"] = pkg.LAYOUT_SOA
    else:
        dyt = torch.from_numpy(dy).cuda()
    net.encoding_backward(torch.from_numpy(x).cuda(), dyt, **kw)
    torch.cuda.synchronize()
    got = tr.gradients[nm:].cpu().numpy().view(np.uint16).copy()
    return int(net.query("grid_direct_levels")), int(net.query("grid_plan_inline")), got


def assert_same(got, ref, what):
    assert got.shape == ref.shape
    bad = np.nonzero(got != ref)[0]
    detail = [(int(i), hex(got[i]), hex(ref[i])) for i in bad[:6]]
    assert bad.size == 0, f"{what}: {bad.size} of {ref.size} gradient entries differ: {detail}"


# (D, L, F, T, direct levels, inline plan): C2, C2', F = 1 (level 0 is one 8192-entry bucket), the 2D grid (levels 0-2),
# F = 8 (level 0 spans 4 buckets). C2' has 1737 buckets, more than the inline plan takes; the others at most 402.
ORACLE_CASES = [(3, 4, 4, 19, 1, 1), (3, 16, 2, 19, 1, 0), (3, 8, 1, 16, 1, 1), (2, 4, 2, 14, 3, 1), (3, 4, 8, 14, 0, 1)]


@pytest.mark.parametrize("D,L,F,T,n_direct,inline", ORACLE_CASES)
def test_direct_levels_against_oracle(pkg, orc, D, L, F, T, n_direct, inline):
    grid = orc.make_grid(D, L, F, T)
    for n in sizes(direct_part(pkg, D, L, F, T)):
        x = positions(n, D, seed=n + L)
        dy = dy_batch(n, L, F, seed=n + F)
        ref = orc.grid_backward_exact(grid, x, dy)
        assert np.count_nonzero(ref) > 0
        for want_inline in (0, 1):  # grid_direct at its default (on), with k_sc_plan and with the inline plan
            nd, inl, got = backward(pkg, D, L, F, T, x, dy, {"grid_plan_inline": want_inline})
            assert nd == n_direct, f"n={n}: {nd} direct levels, expected {n_direct}"  # the old path must not pass silently
            assert inl == (inline if want_inline else 0)
            assert_same(got, ref, f"D{D} L{L} F{F} T{T} n={n} inline={want_inline}")


def both(pkg, D, L, F, T, x, dy, n_direct, **kw):
    nd1, inl1, g1 = backward(pkg, D, L, F, T, x, dy, ON, **kw)
    nd0, inl0, g0 = backward(pkg, D, L, F, T, x, dy, OFF, **kw)
    assert (nd1, inl1) == (n_direct, 1) and (nd0, inl0) == (0, 0)
    assert_same(g1, g0, "options on vs off")
    return g1


def test_max_level_per_sample_2d(pkg, orc):
    """Per-sample max_level on the 2D grid, whose direct levels 1-2 can be masked; values exactly on the level
    boundaries (the backward's test is l > max_level * L + 1e-3)."""
    D, L, F, T = 2, 4, 2, 14
    n = direct_part(pkg, D, L, F, T) + 1
    x = positions(n, D, seed=11)
    ml = np.random.default_rng(12).random(n).astype(np.float32)
    for j, v in enumerate((0.0, 0.25, 0.5, 0.75, 1.0)):
        ml[100 * j:100 * j + 100] = np.float32(v)
    dy = dy_batch(n, L, F, seed=13)
    got = both(pkg, D, L, F, T, x, dy, 3, ml=ml)
    assert_same(got, orc.grid_backward_exact(orc.make_grid(D, L, F, T), x, dy, 1.0, ml), "max_level vs oracle")


def test_accumulate_nonzero_initial_gradient(pkg, orc):
    D, L, F, T = 3, 4, 4, 19
    n = direct_part(pkg) + 1
    grid = orc.make_grid(D, L, F, T)
    x = positions(n, D, seed=21)
    dy = dy_batch(n, L, F, seed=22)
    init = np.random.default_rng(23).uniform(-0.5, 0.5, orc.grid_n_entries(grid) * F).astype(np.float16).view(np.uint16)
    got = both(pkg, D, L, F, T, x, dy, 1, grad_mode=pkg.GRAD_ACCUMULATE, init=init)
    assert_same(got, orc.grid_backward_exact(grid, x, dy, grad16=init), "accumulate vs oracle")


def test_zero_dy_on_direct_level(pkg, orc):
    """dL/dy all zero on the direct level's columns: overwrite mode stores 0 to every entry of the level (no item,
    no slab contribution), accumulate mode keeps the old values."""
    D, L, F, T = 3, 4, 4, 19
    n = 3 * direct_part(pkg) - 5
    grid = orc.make_grid(D, L, F, T)
    n0 = grid.offsets[1] * F  # level 0's parameters
    x = positions(n, D, seed=31)
    dy = dy_batch(n, L, F, seed=32, zero_levels=(0,))
    init = np.random.default_rng(33).uniform(-0.5, 0.5, orc.grid_n_entries(grid) * F).astype(np.float16).view(np.uint16)
    init[init == 0x8000] = 0
    over = both(pkg, D, L, F, T, x, dy, 1, init=init)
    assert not over[:n0].any() and over[n0:].any()
    acc = both(pkg, D, L, F, T, x, dy, 1, grad_mode=pkg.GRAD_ACCUMULATE, init=init)
    np.testing.assert_array_equal(acc[:n0], init[:n0])
    assert_same(acc, orc.grid_backward_exact(grid, x, dy, grad16=init), "zero dy, accumulate vs oracle")


@pytest.mark.parametrize("D,L,F,T,n_direct", [(3, 4, 4, 19, 1), (2, 4, 2, 14, 3)])
def test_soa_and_aos_dy(pkg, D, L, F, T, n_direct):
    n = direct_part(pkg, D, L, F, T) + 1
    x = positions(n, D, seed=41)
    dy = dy_batch(n, L, F, seed=42)
    aos = both(pkg, D, L, F, T, x, dy, n_direct)
    soa = both(pkg, D, L, F, T, x, dy, n_direct, soa=True)
    assert_same(soa, aos, "SoA vs AoS")


# ---- training: NerfNetwork steps, bitwise with the options on and off

def nerf_batch(n, seed, blob=0.8, scale=1e-2):
    g = np.random.default_rng(seed)
    c = np.zeros((n, 7), np.float32)
    c[:, :3] = g.random((n, 3), dtype=np.float32)
    cloud = np.clip(0.5 + 0.05 * g.standard_normal((n, 3)), 0.0, 1.0).astype(np.float32)
    keep = g.random(n) < blob
    c[keep, :3] = cloud[keep]
    c[:64, :3] = np.round(c[:64, :3] * 8) / 8
    c[64:72, :3] = 1.0
    c[72:80, :3] = np.float32(1.0 + 1e-3)
    c[80:88, :3] = np.float32(-1e-2)
    d = g.standard_normal((n, 3))
    c[:, 4:] = (d / np.linalg.norm(d, axis=1, keepdims=True) + 1) / 2
    dL = np.zeros((n, 16), np.float16)
    dL[:, :4] = g.uniform(-scale, scale, (n, 4))
    return torch.from_numpy(c).cuda(), torch.from_numpy(dL).cuda()


def make_nerf(pkg, variant, lazy, opts):
    old = os.environ.get("NGP_LAZY_EMA")
    os.environ["NGP_LAZY_EMA"] = "1" if lazy else "0"
    try:
        cfg = pkg.nerf_config(variant)
        net = pkg.create_nerf_network(cfg)
        tr = pkg.Trainer(net, cfg["optimizer"], seed=1337)
    finally:
        if old is None:
            del os.environ["NGP_LAZY_EMA"]
        else:
            os.environ["NGP_LAZY_EMA"] = old
    for k, v in opts.items():
        net.set_option(k, v)
    return net, tr


def result(tr):
    torch.cuda.synchronize()
    return tr.params.cpu().numpy().view(np.uint16).copy(), tr.params_full_precision.cpu().numpy().view(np.uint32).copy()


def train(pkg, variant, lazy, opts, n, steps=4, scale=1e-2):
    net, tr = make_nerf(pkg, variant, lazy, opts)
    net.reserve(n)
    assert tr.fused_update_active(n) == lazy
    for s in range(steps):
        x, dL = nerf_batch(n, 100 + s, scale=scale)
        tr.train_step(x, dL, 128.0)
    torch.cuda.synchronize()
    on = bool(opts["grid_direct"])
    assert net.query("grid_direct_levels") == (1 if on else 0)
    assert net.query("grid_plan_inline") == (1 if on and variant == "C2" else 0)  # C2': too many buckets
    return result(tr)


@pytest.mark.parametrize("lazy", [False, True], ids=["eager", "lazy_fused"])
@pytest.mark.parametrize("variant", ["C2", "C2p"])
def test_train_bitwise_like_items(pkg, variant, lazy):
    n = direct_part(pkg) + 1
    p1, w1 = train(pkg, variant, lazy, ON, n)
    p0, w0 = train(pkg, variant, lazy, OFF, n)
    assert np.isfinite(p1.view(np.float16).astype(np.float32)).all()
    np.testing.assert_array_equal(p1, p0)
    np.testing.assert_array_equal(w1, w0)


def test_train_zero_gradient_fused_update_skips(pkg):
    """dL/doutput = 0: every contribution is zero, and the fused update skips the direct level's entries as it skips
    the item buckets' (the same parameters as with the options off)."""
    n = direct_part(pkg) + 1
    p1, w1 = train(pkg, "C2", True, ON, n, steps=2, scale=0.0)
    p0, w0 = train(pkg, "C2", True, OFF, n, steps=2, scale=0.0)
    np.testing.assert_array_equal(p1, p0)
    np.testing.assert_array_equal(w1, w0)


def test_train_graph_like_eager(pkg):
    """3 steps captured into one HIP graph (the benchmark's form) against 3 eager steps, options on."""
    n = direct_part(pkg) + 1
    x, dL = nerf_batch(n, 7)
    net, tr = make_nerf(pkg, "C2", True, ON)
    net.reserve(n)
    s = torch.cuda.Stream()
    graph = tr.capture_training_step(x, dL, 128.0, n_steps=3, stream=s)
    graph.launch(stream=s)
    s.synchronize()
    assert net.query("grid_direct_levels") == 1 and net.query("grid_plan_inline") == 1
    pg, wg = result(tr)
    del graph
    net2, tr2 = make_nerf(pkg, "C2", True, ON)
    net2.reserve(n)
    for _ in range(3):
        tr2.train_step(x, dL, 128.0)
    pe, we = result(tr2)
    np.testing.assert_array_equal(pg, pe)
    np.testing.assert_array_equal(wg, we)


def test_split_buckets_with_inline_plan(pkg, orc):
    """n = 8192 with 90 % of the samples inside one level-2 cell (20, 20, 20), which lies inside one level-1 cell whose
    8 corners share one bucket: ~59 k items, above split_limit, so the inline plan derives split parts and a split
    bucket behind the direct level's static ones. Bitwise against grid_plan_inline = 0 and against the oracle."""
    D, L, F, T, n = 3, 4, 4, 19, 8192
    x = positions(n, D, seed=51)
    g = np.random.default_rng(52)
    hot = g.random(n) < 0.9
    hot[:88] = False
    lo, hi = (20 - 0.45) / 63, (20 + 0.45) / 63  # level 2: scale 63, cell = floor(63 x + 0.5)
    x[hot] = g.uniform(lo, hi, (int(hot.sum()), D)).astype(np.float32)
    dy = dy_batch(n, L, F, seed=53)
    nd1, inl1, g1 = backward(pkg, D, L, F, T, x, dy, ON)
    nd0, inl0, g0 = backward(pkg, D, L, F, T, x, dy, {"grid_direct": 1, "grid_plan_inline": 0})
    assert (nd1, inl1, nd0, inl0) == (1, 1, 1, 0)
    assert_same(g1, g0, "inline plan vs k_sc_plan")
    _, _, g00 = backward(pkg, D, L, F, T, x, dy, OFF)
    assert_same(g1, g00, "options on vs off")
    assert_same(g1, orc.grid_backward_exact(orc.make_grid(D, L, F, T), x, dy), "split buckets vs oracle")


@pytest.mark.parametrize("lazy", [False, True], ids=["eager", "lazy_fused"])
def test_replan_alternating_batches(pkg, lazy):
    """One model, the batch size alternating and both options toggled between the steps (every change re-plans in
    the reused workspace), against a model that ran with both off throughout."""
    schedule = ((8192, 1, 1), (4096, 0, 1), (12289, 1, 0), (8192, 0, 0), (8192, 1, 1))
    runs = []
    for toggled in (True, False):
        net, tr = make_nerf(pkg, "C2", lazy, OFF)
        net.reserve(12289)
        for s, (n, d, i) in enumerate(schedule):
            net.set_option("grid_direct", d if toggled else 0)
            net.set_option("grid_plan_inline", i if toggled else 0)
            x, dL = nerf_batch(n, 300 + s)
            tr.train_step(x, dL, 128.0)
        runs.append(result(tr))
        del net, tr
    np.testing.assert_array_equal(runs[0][0], runs[1][0])
    np.testing.assert_array_equal(runs[0][1], runs[1][1])
