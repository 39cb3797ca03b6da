"""The NeRF loss pass on the GPU (k_loss_pass1 / k_scan4 / k_loss_pass2) against the float64 restatement of
test_nerf_loss_host.py, on its hand-built batches: every loss, every activation pair, the three colour spaces, fixed and
random backgrounds, the regularisers on and off, every entry point (plain, error_map=, keep_state= with a full and a
short state), ray counts around the kernels' group sizes and the compaction's cases.

Integers (compacted counter, every {n, base}) and compacted coordinates are equal: the batches keep every ray away from
every decision (test_batch_has_every_shape_and_no_ray_near_a_decision), so no element is left out of any comparison.
Per-ray loss: |got - ref| <= 4 K32 2^-24 companion. Each fp16 gradient element: the same, plus half an fp16 ulp of the
reference, plus one fp16 ulp for a rounding that flips. K32 and the companions: test_nerf_loss_host.py's docstring."""
import ctypes as C

import numpy as np
import pytest
import torch

from test_nerf_loss_host import (ACT_LOGISTIC, ACT_NONE, ACT_RELU, GROUPS, K32, N_RAYS_TOTAL, RAY_COUNTS, batches, cfg_values,
                                 compaction_cases, compare, error_map_deposit, f16_ulp, make_cfg, planted_expectations)

pytestmark = pytest.mark.gpu
K_GPU = 4 * K32
MAX_C = 1 << 13


@pytest.fixture(scope="module")
def pkg():
    from __graft_entry__ import load_package
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return load_package()


@pytest.fixture(scope="module")
def world(pkg):
    groups, full, _, _ = batches(pkg)
    return groups, full, pkg.nerf.NerfDataset(full.images, full.pixels)


def to_device(samples):
    return {k: torch.from_numpy(v.view(np.int32) if v.dtype == np.uint32 else v).cuda() for k, v in samples.items()}


def run(pkg, ds, batch, cfg, mean=0.003, max_c=MAX_C, n_rays=None, counter=None, **kw):
    n = batch.n_rays if n_rays is None else n_rays
    s = to_device(batch.samples(n, counter))
    out = torch.from_numpy(batch.out(int(cfg.density_activation))).cuda()
    got = pkg.nerf.compute_loss(ds, cfg, n, batch.rng, max_c, s, out, torch.tensor([mean], device="cuda"),
                                n_rays_total=N_RAYS_TOTAL, **kw)
    torch.cuda.synchronize()
    res = {k: v.cpu().numpy() for k, v in got.items()}
    res["numsteps"] = s["numsteps"].cpu().numpy()
    return res


def check(ref, got, max_c=MAX_C):
    """compare() with the GPU bound, and what must stay as it was: columns 4..15 of dloss_doutput, the rows at and past
    the compacted total of both compacted arrays (the buffers start as zeros)."""
    worst = compare(ref, got["loss"], got["dloss_doutput"], got["numsteps"], got["compacted_counter"].view(np.uint32)[0],
                    got["coords_compacted"], K_GPU)
    used = ref["row"].size
    np.testing.assert_array_equal(ref["row"], np.arange(used))
    assert used == min(ref["compacted_counter"], max_c)
    assert not got["dloss_doutput"].view(np.uint16)[:, 4:].any()
    assert not got["dloss_doutput"].view(np.uint16)[used:].any() and not got["coords_compacted"].view(np.uint32)[used:].any()
    return worst


def bitwise_equal(a, b):
    for k in ("numsteps", "compacted_counter", "coords_compacted", "loss"):
        np.testing.assert_array_equal(a[k].view(np.uint32), b[k].view(np.uint32), err_msg=k)
    np.testing.assert_array_equal(a["dloss_doutput"].view(np.uint16), b["dloss_doutput"].view(np.uint16))


def check_planted(batch, ref, got, cfg, mean):
    """The planted exact-decision samples (+-0, -10 and its fp16 neighbours, the clamps) against hand-written values."""
    g = got["dloss_doutput"].astype(np.float64)
    n = 0
    for i, col, want, what in planted_expectations(batch, ref, cfg_values(cfg), mean):
        have = g[ref["row"][i], col]
        if what == "ReLU at +-0":
            assert have == 0.0, (what, have)
        else:
            bound = K_GPU * 2.0 ** -24 * ref["grad_companion"][i, col] + 1.5 * f16_ulp(want)
            assert abs(have - want) <= bound, (what, i, col, have, want, bound)
        n += 1
    assert n >= 11


@pytest.mark.parametrize("group", GROUPS)
def test_loss_pass_matches_float64(pkg, world, group):
    """The plain form, every configuration of the group, the 300-ray batch."""
    groups, full, ds = world
    worst = (0.0, 0.0)
    for label, cfg, mean in groups[group]:
        ref = full.reference(cfg, mean, max_compacted=MAX_C)
        got = run(pkg, ds, full, cfg, mean)
        ul, ug = check(ref, got)
        check_planted(full, ref, got, cfg, mean)
        assert ref["compacted_counter"] > 1000 and np.abs(ref["grad"]).max() > 0
        worst = (max(worst[0], ul), max(worst[1], ug))
    print(f"{group}: worst err / bound, loss {worst[0] / K_GPU:.3f}, gradient (beyond half an fp16 ulp) {worst[1] / K_GPU:.3f}"
          f" over {len(groups[group])} configurations")


@pytest.mark.parametrize("n_rays", RAY_COUNTS)
def test_ray_counts(pkg, world, n_rays):
    """The first n rays of the batch as a batch of their own: a scan group of 4, a block of 16 rays, an XCD group of 128,
    each with a ragged tail; the plain form and the wave-per-ray pass 2, which must give the same bits."""
    groups, full, ds = world
    worst = (0.0, 0.0)
    for cfg in (make_cfg(pkg), make_cfg(pkg, "L2", ACT_NONE, ACT_NONE)):
        ref = full.reference(cfg, max_compacted=MAX_C, n_rays=n_rays)
        plain = run(pkg, ds, full, cfg, n_rays=n_rays)
        ul, ug = check(ref, plain)
        worst = (max(worst[0], ul), max(worst[1], ug))
        kept = run(pkg, ds, full, cfg, n_rays=n_rays, keep_state=True)
        bitwise_equal(plain, kept)
    print(f"{n_rays} rays: worst err / bound, loss {worst[0] / K_GPU:.3f}, gradient {worst[1] / K_GPU:.3f}")


@pytest.mark.parametrize("case", range(5))
def test_compaction(pkg, world, case):
    """max_compacted above the total, inside a ray, exactly at a ray's end, and so small that later rays get {0, base}
    and loss 0; a ray counter below n_rays (those rays: loss 0, no count, their numsteps rows as they were)."""
    groups, full, ds = world
    cfg = make_cfg(pkg)
    max_c, counter = compaction_cases(full, cfg)[case]
    ref = full.reference(cfg, max_compacted=max_c, counter=counter)
    plain = run(pkg, ds, full, cfg, max_c=max_c, counter=counter)
    ul, ug = check(ref, plain, max_c)
    if counter is not None:
        np.testing.assert_array_equal(plain["numsteps"][counter:].view(np.uint32), full.samples()["numsteps"][counter:])
        assert not plain["loss"][counter:].any()
    for cap in (None, full.total // 3):
        kept = run(pkg, ds, full, cfg, max_c=max_c, counter=counter, keep_state=True, state_capacity=cap)
        bitwise_equal(plain, kept)
    print(f"compaction case {case} (max_compacted {max_c}, counter {counter}): worst err / bound, loss {ul / K_GPU:.3f}, "
          f"gradient {ug / K_GPU:.3f}")


KEPT_STATE_CONFIGS = [("Huber", 3, 3), ("L2", ACT_RELU, ACT_LOGISTIC), ("MAPE", 3, 3), ("LogL1", ACT_LOGISTIC, ACT_NONE),
                      ("RelativeL2", ACT_NONE, ACT_RELU)]


@pytest.mark.parametrize("loss,rgb,density", KEPT_STATE_CONFIGS)
def test_kept_state_forms(pkg, world, loss, rgb, density):
    """keep_state=True with a full and a short state_capacity (wave-per-ray pass 2; the 65- and 100-sample rays take a
    second round, the rays past a short state are composited again): against float64, and the same bits as the plain form."""
    groups, full, ds = world
    cfg = make_cfg(pkg, loss, rgb, density)
    ref = full.reference(cfg, max_compacted=MAX_C)
    plain = run(pkg, ds, full, cfg)
    assert (ref["cn"] > 64).any()
    for cap in (None, full.total // 3, 1):
        kept = run(pkg, ds, full, cfg, keep_state=True, state_capacity=cap)
        ul, ug = check(ref, kept)
        check_planted(full, ref, kept, cfg, 0.003)
        bitwise_equal(plain, kept)
    print(f"kept state {loss} rgb={rgb} density={density}: worst err / bound, loss {ul / K_GPU:.3f}, gradient {ug / K_GPU:.3f}")


@pytest.mark.parametrize("loss,width,height", [("Huber", 13, 11), ("SMAPE", 5, 4)])
def test_error_map_form(pkg, world, loss, width, height):
    """error_map=: the outputs as in the plain form, and the deposit is the restatement's mean loss split bilinearly
    (float atomics in any order: the tolerance of test_compute_loss). 13x11 is larger than every image, so the texel
    index is clamped with the image's resolution; rays cut off by max_compacted deposit nothing."""
    groups, full, ds = world
    cfg = make_cfg(pkg, loss)
    max_c = full.reference(cfg)["compacted_counter"] // 2
    ref = full.reference(cfg, max_compacted=max_c)
    assert (ref["cnum"][ref["cn"] > 0] == 0).any()
    em = torch.zeros((len(full.images), height, width), dtype=torch.float32, device="cuda")
    got = run(pkg, ds, full, cfg, max_c=max_c, error_map=em)
    check(ref, got, max_c)
    want = error_map_deposit(ref, full.pixels, width, height)
    assert want.sum() > 0
    np.testing.assert_allclose(em.cpu().numpy(), want, rtol=1e-4, atol=1e-6 * float(want.max()))


def test_plain_form_touches_nothing_else(pkg, world):
    """Through the C-ABI with buffers full of a sentinel: columns 4..15 of dloss_doutput, the rows at and past the
    compacted total and the loss of rays past the ray counter keep it; rays before the counter that compact nothing get
    no loss written either (the caller's zeros stay)."""
    from instant_ngp_amd._capi import check as check_rc
    from instant_ngp_amd.network import _ptr, _stream
    groups, full, ds = world
    cfg = make_cfg(pkg)
    counter, max_c = 250, 3000
    ref = full.reference(cfg, max_compacted=max_c, counter=counter)
    s = to_device(full.samples(counter=counter))
    out = torch.from_numpy(full.out(3)).cuda()
    mean = torch.tensor([0.003], device="cuda")
    coords_c = torch.full((max_c + 7, 7), -7.5, device="cuda")
    dl = torch.full((max_c + 7, 16), -3.25, dtype=torch.float16, device="cuda")
    loss = torch.full((full.n_rays,), -1.0, device="cuda")
    cc = torch.zeros(1, dtype=torch.int32, device="cuda")
    check_rc(pkg.lib().ngp_nerf_compute_loss(
        ds.handle, C.byref(cfg), _stream(None), full.n_rays, N_RAYS_TOTAL, full.rng, max_c, _ptr(s["counters"]), _ptr(out),
        _ptr(s["ray_indices"]), _ptr(s["rays"]), _ptr(s["numsteps"]), _ptr(s["coords"]), _ptr(coords_c), _ptr(dl), _ptr(loss),
        _ptr(cc), _ptr(mean), 128.0))
    torch.cuda.synchronize()
    used = ref["row"].size
    assert used == max_c < ref["compacted_counter"]
    dl, coords_c, loss = dl.cpu().numpy(), coords_c.cpu().numpy(), loss.cpu().numpy()
    assert (dl[:, 4:] == np.float16(-3.25)).all() and (dl[used:] == np.float16(-3.25)).all() and (coords_c[used:] == -7.5).all()
    assert (loss[ref["cnum"] == 0] == -1.0).all() and (ref["cnum"][:counter] == 0).any()
    got = {"loss": np.where(ref["cnum"] > 0, loss, 0.0), "dloss_doutput": dl, "coords_compacted": coords_c,
           "compacted_counter": cc.cpu().numpy(), "numsteps": s["numsteps"].cpu().numpy()}
    compare(ref, got["loss"], dl, got["numsteps"], got["compacted_counter"].view(np.uint32)[0], coords_c, K_GPU)
