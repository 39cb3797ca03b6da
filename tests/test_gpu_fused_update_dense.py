"""The fused optimizer update on DENSE item buckets of the bucketed grid backward (grid_scatter.hip, k_sc_accumulate:
a bucket with at least two items per entry updates its records in place, every thread its pairs round by round, with
the step, the hyperparameters and the scheduled learning rate derived once per block: optimizer.h FusedStep). The
tests hold whatever way the branch moves its records: DESIGN §10 (round 9) records a form that staged whole spans of
records through LDS, for which the ragged last spans and the skipped pairs inside a span below are the edge cases.

The yardstick is the project's own: the eager optimizer layout with a separate optimizer launch (NGP_LAZY_EMA=0) must
equal, bit for bit, the lazy layout with fuse_opt=0, the fused update with fuse_mlp_opt 1 and with fuse_mlp_opt 0, in
the fp32 master weights, the fp16 weights, the inference (EMA) parameters read mid-run and at the end, the serialized
optimizer state and the step count. The equality of the serialized state (m1, m2, ema, steps of every parameter) is
also the proof that skipped records and the skipped half of a mixed pair kept their bytes, and that nothing was
written past a bucket's last record.

Shapes are the smallest at which the dense branch can go wrong (base_resolution 12, per_level_scale 1.5: levels of
1,728, 5,832 and 16,384 entries): a level that is one partial bucket, a level whose last bucket is partial (1,736
entries: 54.25 spans of 64 pairs at F = 4), and hashed levels of full buckets; F = 4 (2,048-entry buckets, 1,024
threads, 4 rounds) and F = 2 (4,096-entry buckets, 512 threads, 8 rounds; 1,728 and 1,736 pairs are 27 and 27.125
spans). Which buckets take the dense branch is computed on the host from the positions with the plan's bucket size and
asserted, never assumed.

Batches are 8,192 samples: every item bucket then has t >= 2 n_e. The level that is a single bucket holds all of the
batch's 65,536 items of that level, more than the plan's split limit (49,152 items), so at 8,192 samples it is summed
in parts and updated by k_sc_split_reduce (or, with grid_direct 1, has no items at all). The runs therefore add steps
of 6,144 samples (49,152 items per level: not split, every item bucket still dense), at which the single partial
bucket does take the dense branch with grid_direct 0."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPLIT_LIMIT = 49152      # ScatterKnobs::limit: buckets with more items are summed in parts
TILE_ENTRY_FEATURES = 8192  # a bucket's int64 accumulators fill the 64-KB tile: 2^B entries = 8192 / F
VARIANTS = (("eager", False, 0, 1), ("lazy", True, 0, 1), ("fused", True, 1, 1), ("fused_mlp_launch", True, 1, 0))


@pytest.fixture(scope="module")
def pkg():
    from __graft_entry__ import load_package
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return load_package()


@pytest.fixture(scope="module")
def orc():
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import pyoracle
    return pyoracle


def encoding(F, n_levels, log2T):
    return {"n_levels": n_levels, "n_features_per_level": F, "log2_hashmap_size": log2T, "base_resolution": 12,
            "per_level_scale": 1.5}


def make_trainer(pkg, lazy, enc, direct):
    old = os.environ.get("NGP_LAZY_EMA")
    os.environ["NGP_LAZY_EMA"] = "1" if lazy else "0"
    try:
        cfg = pkg.nerf_config("C2")
        cfg["encoding"].update(enc)
        net = pkg.create_nerf_network(cfg)
        net.set_option("grid_direct", direct)
        tr = pkg.Trainer(net, cfg["optimizer"], seed=1337)
    finally:
        if old is None:
            del os.environ["NGP_LAZY_EMA"]
        else:
            os.environ["NGP_LAZY_EMA"] = old
    return net, tr


@functools.lru_cache(maxsize=None)
def host_batch(n, step):
    g = np.random.default_rng(7000 + step)
    c = np.zeros((n, 7), np.float32)
    c[:, :3] = g.random((n, 3))
    c[:, 3] = 0.01
    d = g.standard_normal((n, 3))
    c[:, 4:] = (d / np.linalg.norm(d, axis=1, keepdims=True) + 1) / 2
    dl = np.zeros((n, 16), np.float32)
    dl[:, :4] = g.uniform(-1, 1, (n, 4))
    return c, dl


def batch(n, step, scale=1.0):
    c, dl = host_batch(n, step)
    return torch.from_numpy(c).cuda(), torch.from_numpy((dl * np.float32(scale)).astype(np.float16)).cuda()


def dense_kinds(orc, enc, direct, n, step):
    """Which kinds of bucket the batch's plan updates in the dense branch of k_sc_accumulate (2 n_e <= t <= split
    limit, item levels only), and whether any item bucket below the split limit is sparse (t < 2 n_e)."""
    F, L = enc["n_features_per_level"], enc["n_levels"]
    g = orc.make_grid(3, L, F, enc["log2_hashmap_size"], Nmin=enc["base_resolution"], b=enc["per_level_scale"])
    NE = TILE_ENTRY_FEATURES // F
    pos = np.ascontiguousarray(host_batch(n, step)[0][:, :3])
    idx = orc.grid_indices(g, pos)
    sizes = [g.offsets[l + 1] - g.offsets[l] for l in range(L)]
    n_direct = 0  # the leading levels of at most two buckets have no items with grid_direct
    while direct and n_direct < L and sizes[n_direct] <= 2 * NE:
        n_direct += 1
    kinds, sparse = set(), 0
    for l in range(n_direct, L):
        nb = -(-sizes[l] // NE)
        t = np.bincount(((idx[:, l, :].astype(np.int64) - g.offsets[l]) // NE).ravel(), minlength=nb)
        assert t.sum() == 8 * n
        hashed = g.resolution[l] ** 3 > sizes[l]
        for b in range(nb):
            n_e = min(NE, sizes[l] - b * NE)
            if t[b] > SPLIT_LIMIT or t[b] == 0:
                continue
            if t[b] < 2 * n_e:
                sparse += 1
                continue
            if nb == 1 and n_e < NE:
                kinds.add("single_partial")
            elif b == nb - 1 and n_e < NE:
                kinds.add("last_partial")
            elif n_e == NE and hashed:
                kinds.add("full_hashed")
            elif n_e == NE:
                kinds.add("full_dense_level")
    return kinds, sparse


def train(pkg, enc, direct, sizes, scale=1.0, snap_at=(), keep_gradients=False):
    """The same steps under the four variants: name -> (w32 bits, w16 bits, inference snapshots, blob, step[, grads])."""
    runs = {}
    for name, lazy, fuse, mlp in VARIANTS:
        net, tr = make_trainer(pkg, lazy, enc, direct)
        net.set_option("fuse_opt", fuse)
        net.set_option("fuse_mlp_opt", mlp)
        assert tr.fused_update_active(sizes[0]) == bool(lazy and fuse)
        snaps = []
        for step, n in enumerate(sizes):
            x, dl = batch(n, step, scale)
            tr.train_step(x, dl, 128.0)
            if step in snap_at:  # reading the inference parameters mid-run completes the EMA; training continues
                torch.cuda.synchronize()
                snaps.append(tr.inference_params.cpu().numpy().view(np.uint16).copy())
        torch.cuda.synchronize()
        grads = None
        if keep_gradients and name == "lazy":
            grads = tr.gradients.cpu().numpy().view(np.uint16)[net.n_matrix_params:].copy()
        snaps.append(tr.inference_params.cpu().numpy().view(np.uint16).copy())
        runs[name] = (tr.params_full_precision.cpu().numpy().view(np.uint32).copy(),
                      tr.params.cpu().numpy().view(np.uint16).copy(), snaps, tr.serialize(), tr.step, grads)
        del net, tr
    return runs


def assert_all_equal_eager(runs, n_steps):
    w_e, p_e, s_e, b_e, st_e, _ = runs["eager"]
    assert st_e == n_steps
    for name in ("lazy", "fused", "fused_mlp_launch"):
        w, p, s, b, st, _ = runs[name]
        np.testing.assert_array_equal(w, w_e, err_msg=f"{name}: params_full_precision")
        np.testing.assert_array_equal(p, p_e, err_msg=f"{name}: params")
        assert len(s) == len(s_e)
        for i, (a, e) in enumerate(zip(s, s_e)):
            np.testing.assert_array_equal(a, e, err_msg=f"{name}: inference parameters, read {i}")
        assert b == b_e, f"{name}: serialized optimizer state (w32, m1, m2, ema32, steps) differs"
        assert st == st_e


RAGGED = {4: (encoding(4, 3, 14), (8192, 8192, 6144, 8192, 6144, 8192)),
          2: (encoding(2, 4, 14), (8192, 8192, 6144, 8192, 6144, 8192))}
# the kinds of bucket the dense branch must have updated in each run (with grid_direct the leading levels of at most
# two buckets have no items: level 0 at F = 4, levels 0 and 1 at F = 2)
RAGGED_KINDS = {(4, 0): {"single_partial", "last_partial", "full_hashed"}, (4, 1): {"last_partial", "full_hashed"},
                (2, 0): {"single_partial", "last_partial", "full_hashed"}, (2, 1): {"full_hashed"}}


@pytest.mark.parametrize("F,direct", [(4, 1), (4, 0), (2, 1), (2, 0)])
def test_ragged_dense_buckets_bitwise(pkg, orc, F, direct):
    enc, sizes = RAGGED[F]
    seen = set()
    for step, n in enumerate(sizes):
        kinds, sparse = dense_kinds(orc, enc, direct, n, step)
        assert sparse == 0, f"step {step}: {sparse} item buckets below 2 items per entry"
        if n == 8192:
            assert "single_partial" not in kinds  # 65,536 items: over the split limit, summed in parts
        seen |= kinds
    assert seen >= RAGGED_KINDS[(F, direct)], f"dense branch took {seen}"
    runs = train(pkg, enc, direct, sizes, snap_at=(2,))
    assert_all_equal_eager(runs, len(sizes))


def test_dense_and_compacted_branches_alternate_bitwise(pkg, orc):
    """8,192-sample steps alternate with 4,096-sample steps on a 2^16 table (level 2: 19,688 entries, 10 buckets): in the
    small steps the fine buckets fall below two items per entry and take the compacted path, on the records the dense
    path wrote the step before, and the other way round."""
    enc = encoding(4, 3, 16)
    sizes = tuple(8192 if s % 2 == 0 else 4096 for s in range(12))
    k_big, sparse_big = dense_kinds(orc, enc, 1, 8192, 0)
    k_small, sparse_small = dense_kinds(orc, enc, 1, 4096, 1)
    assert sparse_big == 0 and "full_dense_level" in k_big and "last_partial" in k_big
    assert sparse_small >= 8, "the fine level's buckets must take the compacted path in the small steps"
    assert k_small, "the coarse buckets stay dense in the small steps"
    runs = train(pkg, enc, 1, sizes, snap_at=(5,))
    assert_all_equal_eager(runs, 12)


SKIP_SCALE = 2.0 ** -19


def test_skipped_and_half_skipped_pairs_inside_dense_buckets_bitwise(pkg, orc):
    """dL/dout scaled by SKIP_SCALE = 2^-19: a contribution to_f16(w * dL/dy) then often rounds to fp16 zero, and an
    entry's gradient is exactly zero when all of its contributions do, while the buckets stay dense (t depends on the
    positions alone). The scale was chosen from the unfused arithmetic alone, by a host sweep with the oracle's
    contribution-exact backward at the initial weights (share of the grid's parameter pairs with exactly one zero half /
    with both halves zero: 2^-16 0.07 / 0.29, 2^-17 0.11 / 0.31, 2^-18 0.17 / 0.35, 2^-19 0.23 / 0.41, 2^-20 0.25 /
    0.55, 2^-21 0.19 / 0.72, 2^-22 0.10 / 0.87; about 0.28 of the pairs are zero at any scale, features behind inactive
    neurons). The test takes the shares from the fuse_opt=0 run's gradient buffer after the last step and asserts both
    in [0.05, 0.95]; on the GPU they read 0.2585 (one zero half) and 0.5075 (both halves zero)."""
    enc, _ = RAGGED[4]
    sizes = (8192, 8192, 8192, 8192)
    for step, n in enumerate(sizes):
        kinds, sparse = dense_kinds(orc, enc, 1, n, step)
        assert sparse == 0 and kinds >= {"last_partial", "full_hashed"}
    runs = train(pkg, enc, 1, sizes, scale=SKIP_SCALE, snap_at=(1,), keep_gradients=True)
    g = runs["lazy"][5].reshape(-1, 2)
    zero = (g & 0x7FFF) == 0
    one, both = float(np.mean(zero[:, 0] != zero[:, 1])), float(np.mean(zero[:, 0] & zero[:, 1]))
    print(f"scale {SKIP_SCALE}: pairs with exactly one zero half {one:.4f}, with both halves zero {both:.4f}")
    assert 0.05 <= one <= 0.95, f"share of pairs with exactly one zero half: {one}"
    assert 0.05 <= both <= 0.95, f"share of pairs with both halves zero: {both}"
    assert_all_equal_eager(runs, len(sizes))


def test_captured_steps_dense_buckets_bitwise(pkg, orc):
    """The ragged F = 4 shape through capture_training_step (n_steps = 2, three launches, the learning rate halved
    between launches): the block-uniform step, hyperparameters and scheduled learning rate come from the trainer's
    device block, read once per block."""
    enc, _ = RAGGED[4]
    kinds, sparse = dense_kinds(orc, enc, 1, 8192, 0)
    assert sparse == 0 and kinds >= {"last_partial", "full_hashed"}
    runs = {}
    for name, lazy, fuse, mlp in VARIANTS:
        net, tr = make_trainer(pkg, lazy, enc, 1)
        net.set_option("fuse_opt", fuse)
        net.set_option("fuse_mlp_opt", mlp)
        s = torch.cuda.Stream()
        x, dl = batch(8192, 0)
        with torch.cuda.stream(s):
            graph = tr.capture_training_step(x, dl, 128.0, n_steps=2, stream=s)
        snaps = []
        for it in range(3):
            graph.launch(s)
            s.synchronize()
            if it == 0:
                snaps.append(tr.inference_params.cpu().numpy().view(np.uint16).copy())
            tr.learning_rate = tr.learning_rate * 0.5
        snaps.append(tr.inference_params.cpu().numpy().view(np.uint16).copy())
        runs[name] = (tr.params_full_precision.cpu().numpy().view(np.uint32).copy(),
                      tr.params.cpu().numpy().view(np.uint16).copy(), snaps, tr.serialize(), tr.step, None)
        del graph, net, tr
    assert_all_equal_eager(runs, 6)
