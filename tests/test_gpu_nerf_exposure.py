"""Per-image exposure on the GPU (Training::optimize_exposure): k_loss_pass1's exposure instantiations and the per-image
sum of the rays' exposure gradients (k_exposure_image_sum) against the float64 restatement of test_nerf_exposure_host.py
on its 300-ray batch, determinism, the switch-off identities (bitwise), the trainer's update cadence, resets, snapshots
and refusals, an end-to-end run that recovers known exposures on the procedural scene, and pyngp.

Bounds (constants and companions: test_nerf_exposure_host.py's docstring). Integers and compacted coordinates equal.
Per-ray loss within 4 K32X 2^-24 companion; each fp16 gradient element the same plus half an fp16 ulp plus one ulp for a
rounding that flips; no element left out. A per-image exposure sum within the sum of its rays' bounds (4 K32E 2^-24
companion each) plus (n_i - 1) 2^-24 sum |term|, the worst case of any summation order of n_i float32 terms."""
import ctypes as C

import numpy as np
import pytest
import torch

from test_nerf_depth_host import DEPTH_LAMBDA, MARGIN_TARGET, depth_images, restate_loss_depth, stored_depth
from test_nerf_exposure_host import (HELD_IMAGE, K32E, K32X, exposure_configs, exposure_violations, exposure_world, pixel_margins_hold,
                                     restate_loss_exposure)
from test_nerf_loss_host import C as lit, F32, N_RAYS_TOTAL, RAY_COUNTS, cfg_values, compaction_cases, compare, make_cfg, srgb_to_linear

pytestmark = pytest.mark.gpu
K_GRAD, K_EXP = 4 * K32X, 4 * K32E
MAX_C = 1 << 13


@pytest.fixture(scope="module")
def pkg():
    from __graft_entry__ import load_package
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return load_package()


@pytest.fixture(scope="module")
def world(pkg):
    mine, exposure, _ = exposure_world(pkg)
    return mine, exposure, pkg.nerf.NerfDataset(mine.images, mine.pixels)


def to_device(samples):
    return {k: torch.from_numpy(v.view(np.int32) if v.dtype == np.uint32 else v).cuda() for k, v in samples.items()}


def run(pkg, ds, batch, cfg, exposure=None, gradient=None, mean=0.003, max_c=MAX_C, n_rays=None, counter=None, **kw):
    """compute_loss on the batch's first n rays. exposure: [3, 3] or None; gradient: None (no gradient), or the initial
    value of the accumulator the call adds onto (a scalar or [3, 3]); the accumulator comes back as "exposure_gradient"."""
    n = batch.n_rays if n_rays is None else n_rays
    s = to_device(batch.samples(n, counter))
    out = torch.from_numpy(batch.out(int(cfg.density_activation))).cuda()
    e = None if exposure is None else torch.from_numpy(np.ascontiguousarray(exposure, np.float32)).cuda()
    acc = None if gradient is None else torch.from_numpy(np.array(np.broadcast_to(np.asarray(gradient, np.float32), (3, 3)))).cuda()
    got = pkg.nerf.compute_loss(ds, cfg, n, batch.rng, max_c, s, out, torch.tensor([mean], device="cuda"), n_rays_total=N_RAYS_TOTAL,
                                exposure=e, exposure_gradient=acc, **kw)
    torch.cuda.synchronize()
    res = {k: v.cpu().numpy() for k, v in got.items()}
    res["numsteps"] = s["numsteps"].cpu().numpy()
    if acc is not None:
        res["exposure_gradient"] = acc.cpu().numpy()
    return res


def check(ref, got, max_c=MAX_C):
    """Loss, sample gradients, integers and coordinates (test_nerf_loss_host.compare with this file's constant), what must
    stay zero, and the per-image exposure sums when the call took them (onto zeros). Returns the worst error / bound of
    (loss, gradient, exposure sum)."""
    ul, ug = compare(ref, got["loss"], got["dloss_doutput"], got["numsteps"], got["compacted_counter"].view(np.uint32)[0],
                     got["coords_compacted"], K_GRAD)
    used = ref["row"].size
    assert used == min(ref["compacted_counter"], max_c)
    assert not got["dloss_doutput"].view(np.uint16)[:, 4:].any()
    assert not got["dloss_doutput"].view(np.uint16)[used:].any() and not got["coords_compacted"].view(np.uint32)[used:].any()
    ue = 0.0
    if "exposure_gradient" in got:
        g = got["exposure_gradient"].astype(np.float64)
        n_i = ref["exp_img_n"][:, None]
        bound = K_EXP * 2.0 ** -24 * ref["exp_img_c"] + np.maximum(n_i - 1, 0) * 2.0 ** -24 * ref["exp_img_abs"]
        err = np.abs(g - ref["exp_img"])
        assert (err <= bound).all(), (err, bound)
        assert not g[ref["exp_img_n"] == 0].any()
        ue = float((err[ref["exp_img_n"] > 0] / bound[ref["exp_img_n"] > 0]).max(initial=0.0))
    return ul / K_GRAD, ug / K_GRAD, ue


def bitwise_equal(a, b, keys=("numsteps", "compacted_counter", "coords_compacted", "loss", "dloss_doutput")):
    for k in keys:
        x, y = (a[k].view(np.uint16), b[k].view(np.uint16)) if k == "dloss_doutput" else (a[k].view(np.uint32), b[k].view(np.uint32))
        np.testing.assert_array_equal(x, y, err_msg=k)


# ---- the kernels against the yardstick ---------------------------------------------------------------------------------
@pytest.mark.parametrize("which", range(3))
def test_exposure_matches_float64(pkg, world, which):
    """Each colour space with its loss and activations, the 300-ray batch: everything the loss pass returns at the exposed
    target, and the per-image sums; the plain form and the kept state give the same bits; the exposures change the
    gradients, and the image held at 0 keeps its rays' gradients as they were without exposure."""
    mine, exposure, ds = world
    label, cfg = exposure_configs(pkg)[which]
    ref = restate_loss_exposure(mine, cfg, exposure, max_compacted=MAX_C)
    got = run(pkg, ds, mine, cfg, exposure, 0.0)
    worst = check(ref, got)
    assert ref["compacted_counter"] > 1000 and (ref["exp_img_n"] > 20).all() and np.abs(ref["exp_img"]).min() > 0
    bitwise_equal(got, run(pkg, ds, mine, cfg, exposure, 0.0, keep_state=True))
    bitwise_equal(got, run(pkg, ds, mine, cfg, exposure))         # without a gradient buffer: the same outputs
    off = run(pkg, ds, mine, cfg)
    rows_img = np.asarray(mine.px["img"])[ref["ray"]]
    moved = (got["dloss_doutput"][ref["row"], :4].view(np.uint16) != off["dloss_doutput"][ref["row"], :4].view(np.uint16)).any(axis=1)
    # (Huber's gradient is constant beyond its knee: there a moved target leaves the bits as they were)
    assert moved[rows_img != HELD_IMAGE].mean() > 0.05 and not moved[rows_img == HELD_IMAGE].any()
    print(f"{label}: worst err / bound: loss {worst[0]:.3f}, gradient (beyond half an fp16 ulp) {worst[1]:.3f}, exposure sums {worst[2]:.3f}")


@pytest.mark.parametrize("n_rays", RAY_COUNTS)
def test_ray_counts_with_exposure(pkg, world, n_rays):
    """The first n rays as a batch of their own (a scan group of 4, a block of 16 rays, an XCD group of 128, ragged tails;
    up to 129 rays image 2 has none, and up to 17 image 1 has none either): two configurations, all forms of pass 2."""
    mine, exposure, ds = world
    worst = (0.0, 0.0, 0.0)
    for label, cfg in exposure_configs(pkg)[:2]:
        ref = restate_loss_exposure(mine, cfg, exposure, max_compacted=MAX_C, n_rays=n_rays)
        got = run(pkg, ds, mine, cfg, exposure, 0.0, n_rays=n_rays)
        worst = tuple(max(a, b) for a, b in zip(worst, check(ref, got)))
        bitwise_equal(got, run(pkg, ds, mine, cfg, exposure, 0.0, n_rays=n_rays, keep_state=True))
        if n_rays <= 129:
            assert ref["exp_img_n"][2] == 0
    print(f"{n_rays} rays: worst err / bound: loss {worst[0]:.3f}, gradient {worst[1]:.3f}, exposure sums {worst[2]:.3f}")


@pytest.mark.parametrize("case", range(5))
def test_compaction_with_exposure(pkg, world, case):
    """max_compacted above the total; inside a ray (that ray is counted); at a ray's end; so small that most rays are cut
    to nothing (those are not counted); a ray counter below n_rays (the rays past it are not counted)."""
    mine, exposure, ds = world
    label, cfg = exposure_configs(pkg)[0]
    max_c, counter = compaction_cases(mine, make_cfg(pkg))[case]
    ref = restate_loss_exposure(mine, cfg, exposure, max_compacted=max_c, counter=counter)
    if case == 1:
        cut = np.nonzero((ref["cnum"] > 0) & (ref["cnum"] < ref["cn"]))[0]
        assert cut.size == 1 and ref["counted"][cut[0]]
    if case == 3:
        assert (ref["cn"][~ref["counted"]] > 0).sum() > 200
    got = run(pkg, ds, mine, cfg, exposure, 0.0, max_c=max_c, counter=counter)
    worst = check(ref, got, max_c)
    for cap in (None, mine.total // 3):
        bitwise_equal(got, run(pkg, ds, mine, cfg, exposure, 0.0, max_c=max_c, counter=counter, keep_state=True, state_capacity=cap))
    print(f"compaction case {case}: worst err / bound: loss {worst[0]:.3f}, gradient {worst[1]:.3f}, exposure sums {worst[2]:.3f}")


def position_cdfs(n_images, w, h, seed):
    """Error-map CDFs of the position in the image only (sample_focal_plane_proportional_to_error): the image choice
    stays uniform, so the images are monotone in the ray id, and uv_pdf is not 1."""
    g = np.random.default_rng(seed)
    pmf = g.random((n_images, h, w)) + 0.05
    rows = pmf.sum(axis=2)
    return {"cdf_x_cond_y": (np.cumsum(pmf, axis=2) / pmf.sum(axis=2, keepdims=True)).astype(np.float32),
            "cdf_y": (np.cumsum(rows, axis=1) / rows.sum(axis=1, keepdims=True)).astype(np.float32)}


def test_exposure_with_focal_plane_cdfs(pkg, world):
    """The CDF instantiation: pixels drawn from position CDFs (other texels, uv_pdf != 1), the gradient divided by uv_pdf
    and the loss by the pdf. The CDFs' seed is the first whose pixels keep every ray clear of every margin (found on the
    host, no exclusions). With an image CDF the per-image sum is refused."""
    mine, exposure, ds = world
    label, cfg = exposure_configs(pkg)[2]
    for seed in range(60):
        cd = position_cdfs(3, 5, 4, seed)
        px_all = pkg.nerf.training_pixels(mine.images, mine.cfg0, N_RAYS_TOTAL, mine.rng, cdfs=cd, host=True)
        px = {"img": px_all["img"][mine.ray_indices], "uv": px_all["uv"][mine.ray_indices]}
        if pixel_margins_hold(mine, [cfg], exposure, px=px) and exposure_violations(mine, cfg, exposure, px=px).size == 0:
            break
    else:
        raise AssertionError("no CDF seed keeps the rays clear of the margins")
    pdf = px_all["pdf"][mine.ray_indices].astype(np.float64)
    assert (px["img"] == mine.px["img"]).all() and np.abs(pdf[:, 1] - 1).max() > 0.3 and (pdf[:, 0] == 1).all()
    ref = restate_loss_exposure(mine, cfg, exposure, max_compacted=MAX_C, px=px, uv_pdf=pdf[:, 1])
    ref["loss"], ref["loss_companion"] = ref["loss"] / pdf[:, 1], ref["loss_companion"] / pdf[:, 1] + np.abs(ref["loss"] / pdf[:, 1])
    got = run(pkg, ds, mine, cfg, exposure, 0.0, cdfs=cd)
    worst = check(ref, got)
    flat = restate_loss_exposure(mine, cfg, exposure, max_compacted=MAX_C, px=px)
    assert np.abs(flat["exp_img"] - ref["exp_img"]).max() > 100 * (K_EXP * 2.0 ** -24 * ref["exp_img_c"]).max()   # uv_pdf is seen
    bitwise_equal(got, run(pkg, ds, mine, cfg, exposure, 0.0, cdfs=cd, keep_state=True))
    with pytest.raises(pkg.NgpError):
        run(pkg, ds, mine, cfg, exposure, 0.0, cdfs=dict(cd, cdf_img=np.array([0.2, 0.7, 1.0], np.float32)))
    run(pkg, ds, mine, cfg, exposure, cdfs=dict(cd, cdf_img=np.array([0.2, 0.7, 1.0], np.float32)))   # without the sum: allowed
    print(f"{label} with position CDFs (seed {seed}): worst err / bound: loss {worst[0]:.3f}, gradient {worst[1]:.3f}, "
          f"exposure sums {worst[2]:.3f}")


def constant_map_background(v, rgba):
    """cfg values whose fixed background, behind a map that holds `rgba` in every texel, is what the kernel composites
    (testbed_nerf.cu:1787-1792): linear map rgb + linear background * (1 - map alpha), as the sRGB colour the restatement
    takes its background in (the exact inverse of its srgb_to_linear, above that curve's knee)."""
    lin = rgba[:3].astype(np.float64) + srgb_to_linear(v["background_color"]) * (1.0 - float(rgba[3]))
    assert (lin > 0.01).all()
    back = lit(1.055) * lin ** (1.0 / lit(2.4)) - lit(0.055)     # the module's constants are the reference's float literals
    assert np.abs(srgb_to_linear(back) - lin).max() < 1e-14     # against bounds in units of 2^-24
    return dict(v, background_color=back)


def test_exposure_with_an_environment_map(pkg, world):
    """The ENV instantiation with a map that is not zero: every texel holds the same RGBA, so the bilinear read returns
    it whatever the ray's direction and the background behind the map is known in closed form; the restatement runs with
    that background. The exposure must scale the texel and not the map's share of the target. The map's value is the
    first of a seeded sequence that keeps every ray clear of the margins (found on the host, no exclusions). The map's
    gradient is bound and not zero; the kept state gives the same bits."""
    mine, exposure, ds = world
    label, cfg = exposure_configs(pkg)[0]
    g = np.random.default_rng(31)
    for attempt in range(40):
        rgba = g.uniform(0.1, 0.7, 4).astype(np.float32)
        v = constant_map_background(cfg_values(cfg), rgba)
        if pixel_margins_hold(mine, [v], exposure) and exposure_violations(mine, v, exposure).size == 0:
            break
    else:
        raise AssertionError("no map value keeps the rays clear of the margins")
    ref = restate_loss_exposure(mine, v, exposure, max_compacted=MAX_C)
    plain = restate_loss_exposure(mine, cfg, exposure, max_compacted=MAX_C)
    assert np.abs(ref["exp_img"] - plain["exp_img"]).max() > 100 * (K_EXP * 2.0 ** -24 * ref["exp_img_c"]).max()   # the map is seen
    env = torch.from_numpy(np.ascontiguousarray(np.broadcast_to(rgba, (4, 8, 4)))).cuda()
    g_env = torch.full((4, 8, 4), 7.0, device="cuda")
    got = run(pkg, ds, mine, cfg, exposure, 0.0, envmap=env, envmap_gradient=g_env)
    worst = check(ref, got)
    assert g_env[..., :3].abs().max() > 0 and not g_env[..., 3].any()
    g2 = torch.full((4, 8, 4), 7.0, device="cuda")
    kept = run(pkg, ds, mine, cfg, exposure, 0.0, envmap=env, envmap_gradient=g2, keep_state=True, state_capacity=mine.total // 3)
    bitwise_equal(got, kept)
    np.testing.assert_array_equal(kept["exposure_gradient"].view(np.uint32), got["exposure_gradient"].view(np.uint32))
    print(f"{label} with a constant environment map {rgba.tolist()} (attempt {attempt}): worst err / bound: loss {worst[0]:.3f}, "
          f"gradient {worst[1]:.3f}, exposure sums {worst[2]:.3f}")


def test_exposure_with_depth_supervision(pkg, world):
    """The DEPTH instantiation: depth images attached, lambda > 0, L2 depth loss (no decision of its own but target > 0,
    whose margin is asserted). The colour part is the exposed restatement, the depth term test_nerf_depth_host's."""
    mine, exposure, _ = world
    maps = depth_images(mine.images)
    stored = stored_depth(maps)
    ds = pkg.nerf.NerfDataset(mine.images, mine.pixels)
    for i, m in enumerate(maps):
        if m is not None:
            ds.set_depth(i, m[0], m[1])
    label, cfg = exposure_configs(pkg)[1]
    colour = restate_loss_exposure(mine, cfg, exposure, max_compacted=MAX_C)
    ref = restate_loss_depth(mine, cfg, stored, DEPTH_LAMBDA, "L2", max_compacted=MAX_C, extra={"ref": colour})
    assert ref["depth_margins"]["target"].min() >= MARGIN_TARGET and (ref["live"] & (ref["cnum"] > 0)).sum() > 30
    got = run(pkg, ds, mine, cfg, exposure, 0.0, depth_lambda=DEPTH_LAMBDA, depth_loss="L2")
    worst = check(ref, got)
    no_depth = run(pkg, ds, mine, cfg, exposure, 0.0)
    assert (got["dloss_doutput"].view(np.uint16) != no_depth["dloss_doutput"].view(np.uint16)).any()
    np.testing.assert_array_equal(got["exposure_gradient"].view(np.uint32), no_depth["exposure_gradient"].view(np.uint32))
    for cap in (None, mine.total // 3):
        bitwise_equal(got, run(pkg, ds, mine, cfg, exposure, 0.0, depth_lambda=DEPTH_LAMBDA, depth_loss="L2", keep_state=True,
                               state_capacity=cap))
    print(f"{label} with depth supervision: worst err / bound: loss {worst[0]:.3f}, gradient {worst[1]:.3f}, exposure sums {worst[2]:.3f}")


# ---- determinism -----------------------------------------------------------------------------------------------------------
def test_exposure_sums_are_deterministic_and_accumulate(pkg, world):
    """Two calls give the same bytes; a call onto its own output gives exactly twice it; an image without a counted ray
    keeps its accumulator's bits, whatever they are."""
    mine, exposure, ds = world
    label, cfg = exposure_configs(pkg)[0]
    a = run(pkg, ds, mine, cfg, exposure, 0.0)
    for _ in range(3):
        b = run(pkg, ds, mine, cfg, exposure, 0.0)
        np.testing.assert_array_equal(a["exposure_gradient"].view(np.uint32), b["exposure_gradient"].view(np.uint32))
    twice = run(pkg, ds, mine, cfg, exposure, a["exposure_gradient"])
    np.testing.assert_array_equal(twice["exposure_gradient"].view(np.uint32), (F32(2.0) * a["exposure_gradient"]).view(np.uint32))
    assert np.abs(a["exposure_gradient"]).min() > 0
    sentinel = np.array([[7.25, -0.0, 1e-30], [3.5, -2.0, 0.0], [-0.0, 5e-40, -7.75]], np.float32)   # a denormal and -0 among them
    part = run(pkg, ds, mine, cfg, exposure, sentinel, n_rays=129)
    ref = restate_loss_exposure(mine, cfg, exposure, max_compacted=MAX_C, n_rays=129)
    assert ref["exp_img_n"][2] == 0 and (ref["exp_img_n"][:2] > 0).all()
    np.testing.assert_array_equal(part["exposure_gradient"][2].view(np.uint32), sentinel[2].view(np.uint32))
    zero_based = run(pkg, ds, mine, cfg, exposure, 0.0, n_rays=129)["exposure_gradient"]
    np.testing.assert_array_equal(part["exposure_gradient"][:2].view(np.uint32), (sentinel[:2] + zero_based[:2]).view(np.uint32))
    none_counted = run(pkg, ds, mine, cfg, exposure, sentinel, counter=0)
    np.testing.assert_array_equal(none_counted["exposure_gradient"].view(np.uint32), sentinel.view(np.uint32))


# ---- switch-off identities ---------------------------------------------------------------------------------------------------
def test_switch_off_identities(pkg, world):
    """Bitwise: exposure=None through the new entry point, an all-zero exposure array (with and without the gradient)
    and the old entry points give the same dloss_doutput, loss, numsteps and coordinates: plain, kept state, error map,
    CDFs, with depth."""
    mine, exposure, ds = world
    zero = np.zeros((3, 3), np.float32)
    for label, cfg in exposure_configs(pkg):
        plain = run(pkg, ds, mine, cfg)
        on = run(pkg, ds, mine, cfg, exposure)
        assert (on["dloss_doutput"].view(np.uint16) != plain["dloss_doutput"].view(np.uint16)).any()
        for kw in ({}, {"keep_state": True}, {"keep_state": True, "state_capacity": mine.total // 3}, {"max_c": 700}, {"n_rays": 17}):
            old = run(pkg, ds, mine, cfg, **kw)
            bitwise_equal(old, run(pkg, ds, mine, cfg, exposure_entry=True, **kw))
            bitwise_equal(old, run(pkg, ds, mine, cfg, zero, **kw))
            z = run(pkg, ds, mine, cfg, zero, 0.0, **kw)
            bitwise_equal(old, z)
            assert np.abs(z["exposure_gradient"]).max() > 0
        cd = position_cdfs(3, 5, 4, 1)
        bitwise_equal(run(pkg, ds, mine, cfg, cdfs=cd), run(pkg, ds, mine, cfg, zero, cdfs=cd))
        em0, em1 = torch.zeros((3, 7, 9), device="cuda"), torch.zeros((3, 7, 9), device="cuda")
        bitwise_equal(run(pkg, ds, mine, cfg, error_map=em0), run(pkg, ds, mine, cfg, zero, error_map=em1))
        assert em0.sum() > 0
        bitwise_equal(run(pkg, ds, mine, cfg, depth_entry=True), run(pkg, ds, mine, cfg, exposure_entry=True))
    with pytest.raises(ValueError):
        run(pkg, ds, mine, cfg, None, 0.0)                      # a gradient without exposures


# ---- the trainer -------------------------------------------------------------------------------------------------------------
N_SMALL, W_SMALL = 8, 32


def small_scene(pkg, exposures=None, n=N_SMALL, res=W_SMALL, seed=3):
    S = pkg.synthetic
    ims, pix = [], []
    for i, c2w in enumerate(S.camera_poses(n, seed=seed)):
        ims.append(pkg.nerf.make_image(res, res, pkg.nerf.nerf_matrix_to_ngp(c2w), camera_angle_x=S.LEGO_CAMERA_ANGLE_X))
        pix.append(S.render(c2w, res, res, exposure=None if exposures is None else float(exposures[i])))
    return pkg.nerf.NerfDataset(ims, pix), ims, pix


def new_run(pkg, ds, seed=7, batch=1 << 14, log2_hashmap_size=14):
    ncfg = pkg.nerf_config("C2")
    ncfg["encoding"]["log2_hashmap_size"] = log2_hashmap_size
    net = pkg.create_nerf_network(ncfg)
    tr = pkg.Trainer(net, ncfg["optimizer"], seed=seed)
    cfg = pkg.nerf.default_config(1.0, target_batch_size=batch)
    return net, tr, pkg.nerf.NerfTraining(net, tr, ds, cfg, seed=1337), cfg


def exposures_of(run, n=N_SMALL):
    return np.array([run.camera_exposure(i) for i in range(n)], np.float32)


def test_trainer_with_the_switch_off_is_the_trainer_that_was_never_told(pkg):
    ds, _, _ = small_scene(pkg)
    outs = []
    for touch in (False, True):
        net, tr, run, _ = new_run(pkg, ds)
        assert run.exposure_training() == {"optimize_exposure": False, "exposure_l2_reg": 0.0}
        if touch:
            run.set_exposure_training(optimize=False, l2_reg=0.5)
            run.set_exposure_training(optimize=True)
            run.set_exposure_training(optimize=False)
            assert run.exposure_training() == {"optimize_exposure": False, "exposure_l2_reg": 0.5}
        stats = [run.train_step(get_loss=False) for _ in range(20)]
        torch.cuda.synchronize()
        assert not exposures_of(run).any()
        outs.append((stats, tr.params.cpu().numpy().view(np.uint16), run.density_grid.cpu().numpy()))
    assert outs[0][0] == outs[1][0]
    np.testing.assert_array_equal(outs[0][1], outs[1][1])
    np.testing.assert_array_equal(outs[0][2], outs[1][2])


def test_trainer_update_cadence_resets_and_bound_exposures(pkg):
    """With the switch on the exposures stay zero until step n_steps_between_cam_updates and are non-zero with zero mean
    after it; the optimisers' iteration counts follow; reset_camera_extrinsics zeroes them, set_camera_extrinsics(i) image
    i's; exposures that are not zero scale the targets with the switch off too, and do not train."""
    ds, ims, _ = small_scene(pkg)
    net, tr, run, _ = new_run(pkg, ds)
    run.set_camera_training(n_steps_between_cam_updates=4)
    run.set_exposure_training(optimize=True, l2_reg=1e-3)
    for _ in range(3):
        run.train_step(get_loss=False)
    assert not exposures_of(run).any() and run.exposure_optimizer_state(0)["iter"] == 0
    run.train_step(get_loss=False)
    e = exposures_of(run)
    assert (e != 0).all() and np.abs(e.astype(np.float64).mean(axis=0)).max() <= N_SMALL * 2.0 ** -24 * np.abs(e).max()
    st = run.exposure_optimizer_state(3)
    assert st["iter"] == 1 and st["learning_rate"] == pytest.approx(1e-2) and np.abs(e).max() <= 2.02e-2   # a first Adam step is lr, less the mean
    for _ in range(4):
        run.train_step(get_loss=False)
    assert run.exposure_optimizer_state(3)["iter"] == 2 and (exposures_of(run) != e).any()
    before = exposures_of(run)
    run.set_camera_extrinsics(2, np.array(ims[2].xform[:], np.float32))
    after = exposures_of(run)
    assert not after[2].any() and run.exposure_optimizer_state(2)["iter"] == 0
    np.testing.assert_array_equal(np.delete(after, 2, 0), np.delete(before, 2, 0))
    run.reset_camera_extrinsics()
    assert not exposures_of(run).any() and all(run.exposure_optimizer_state(i)["iter"] == 0 for i in range(N_SMALL))
    run.train_step(get_loss=False)
    # bound but off: the targets are scaled (the first step's loss, over the same rays and the same network, differs from
    # a plain trainer's, and so does the training), the exposures stay as set. Image 0: at the first steps the compacted
    # budget holds only the batch's first rays, which are image 0's
    results = []
    for value in (None, (0.5, -0.25, 0.0)):
        net2, tr2, run2, _ = new_run(pkg, ds)
        if value is not None:
            run2.set_camera_exposure(0, value)
            np.testing.assert_array_equal(run2.camera_exposure(0), np.array(value, np.float32))
            assert run2.exposure_optimizer_state(0)["iter"] == 0
        first = run2.train_step(get_loss=True)["loss"]
        for _ in range(5):
            run2.train_step(get_loss=False)
        torch.cuda.synchronize()
        results.append((first, tr2.params.cpu().numpy().view(np.uint16).copy()))
        if value is not None:
            np.testing.assert_array_equal(run2.camera_exposure(0), np.array(value, np.float32))
            assert not run2.camera_exposure(1).any()
    print(f"first step's loss: plain {results[0][0]:.6f}, image 0 exposed {results[1][0]:.6f}; parameters that differ after 6 steps: "
          f"{(results[0][1] != results[1][1]).mean():.4f}")
    assert results[0][0] != results[1][0]
    assert (results[0][1] != results[1][1]).any()
    with pytest.raises(pkg.NgpError):
        run.set_exposure_training(l2_reg=-1.0)
    with pytest.raises(pkg.NgpError):
        run.set_camera_exposure(N_SMALL, (0.0, 0.0, 0.0))
    with pytest.raises(pkg.NgpError):
        run.set_camera_exposure(0, (float("nan"), 0.0, 0.0))


def test_exposure_and_pose_refinement_share_the_update_counter(pkg):
    """Both switches on: both update at the same steps, every n_steps_between_cam_updates; pose refinement alone keeps
    its cadence with the exposure code present."""
    ds, _, _ = small_scene(pkg)
    net, tr, run, _ = new_run(pkg, ds)
    run.set_camera_training(optimize_extrinsics=1, n_steps_between_cam_updates=3)
    run.set_exposure_training(optimize=True)
    for k in range(1, 8):
        run.train_step(get_loss=False)
        assert run.exposure_optimizer_state(0)["iter"] == k // 3 and run.pose_optimizer_state(0)[0]["iter"] == k // 3
    assert exposures_of(run).any()


def test_snapshot_round_trip_and_continuation(pkg, tmp_path):
    """An untouched trainer's snapshot has no cam_exposure member; with the feature used, variables and moments come
    back bit for bit and training continues with the bits of the uninterrupted run. A snapshot holds no random number
    generator (as in the reference), so the loading trainer has taken the same number of steps before it loads; it took
    them with the switch off and is given other exposures, so everything compared comes from the file."""
    import gzip
    ds, _, _ = small_scene(pkg)
    net0, tr0, plain, _ = new_run(pkg, ds)
    plain.train_step(get_loss=False)
    p0 = str(tmp_path / "plain.ingp")
    plain.save_snapshot(p0)
    assert b"cam_exposure" not in gzip.open(p0).read() and b"cam_pos_offset" in gzip.open(p0).read()
    net, tr, run, _ = new_run(pkg, ds)
    run.set_camera_training(n_steps_between_cam_updates=4)
    run.set_exposure_training(optimize=True, l2_reg=1e-4)
    for _ in range(8):
        run.train_step(get_loss=False)
    path = str(tmp_path / "exposure.ingp")
    run.save_snapshot(path, include_optimizer_state=True)
    assert b"cam_exposure" in gzip.open(path).read()
    saved = [run.exposure_optimizer_state(i) for i in range(N_SMALL)]
    assert all(s["iter"] == 2 for s in saved)
    net2, tr2, run2, _ = new_run(pkg, ds)
    run2.set_camera_training(n_steps_between_cam_updates=4)
    for _ in range(8):
        run2.train_step(get_loss=False)
    run2.set_camera_exposure(5, (0.3, 0.2, 0.1))
    run2.load_snapshot(path)
    run2.set_exposure_training(optimize=True, l2_reg=1e-4)
    for i in range(N_SMALL):
        got = run2.exposure_optimizer_state(i)
        for k, v in saved[i].items():
            assert (got[k].tobytes() == v.tobytes()) if isinstance(v, np.ndarray) else got[k] == v, (i, k)
    for _ in range(8):
        run.train_step(get_loss=False)
        run2.train_step(get_loss=False)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(exposures_of(run2).view(np.uint32), exposures_of(run).view(np.uint32))
    assert run2.exposure_optimizer_state(0)["iter"] == 4
    np.testing.assert_array_equal(tr2.params.cpu().numpy().view(np.uint16), tr.params.cpu().numpy().view(np.uint16))
    # a snapshot without the member loads the exposures as zeros
    run2.load_snapshot(p0)
    assert not exposures_of(run2).any() and run2.exposure_optimizer_state(0)["iter"] == 0


def test_refusals(pkg):
    """sample_image_proportional_to_error and a data-parallel hook are refused with the switch on, either way round;
    the message names both switches; the state stays. sample_focal_plane_proportional_to_error is allowed and trains."""
    ds, _, _ = small_scene(pkg)
    net, tr, run, _ = new_run(pkg, ds)
    run.set_exposure_training(optimize=True)
    with pytest.raises(pkg.NgpError, match="optimize_exposure.*sample_image_proportional_to_error"):
        run.set_error_sampling(image=True)
    assert run.error_sampling() == {"focal_plane": False, "image": False}
    run.set_error_sampling(focal_plane=True)
    run.set_exposure_training(optimize=False)
    run.set_error_sampling(image=True)
    with pytest.raises(pkg.NgpError, match="optimize_exposure.*sample_image_proportional_to_error"):
        run.set_exposure_training(optimize=True)
    assert run.exposure_training()["optimize_exposure"] is False
    run.set_error_sampling(image=False)
    run.set_exposure_training(optimize=True)
    for _ in range(3):
        run.train_step(get_loss=False)
    # data parallel
    hook_t = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_uint64, C.c_int, C.c_int, C.c_void_p)
    hook = hook_t(lambda user, buf, count, dtype, op, stream: 0)
    lib = pkg.lib()
    assert lib.ngp_nerf_trainer_set_data_parallel(run.handle, 0, 1, C.cast(hook, C.c_void_p), None) != 0
    assert b"single-GPU" in lib.ngp_last_error() and b"optimize_exposure" in lib.ngp_last_error()
    net2, tr2, run2, _ = new_run(pkg, ds)
    assert lib.ngp_nerf_trainer_set_data_parallel(run2.handle, 0, 1, C.cast(hook, C.c_void_p), None) == 0
    with pytest.raises(pkg.NgpError, match="single-GPU"):
        run2.set_exposure_training(optimize=True)
    assert run2.exposure_training()["optimize_exposure"] is False
    assert run2.train_step(get_loss=False)["step"] == 1


# ---- end to end ------------------------------------------------------------------------------------------------------------
E2E_VIEWS, E2E_HELD, E2E_RES, E2E_STEPS, E2E_BETWEEN = 20, 4, 64, 6000, 4


def e2e_exposures(views=E2E_VIEWS):
    """Known log2 exposures, one per view, zero mean, spread about +-0.4."""
    e = np.random.default_rng(21).uniform(-0.4, 0.4, views)
    return (e - e.mean()).astype(np.float32)


def train_e2e(pkg, brighten, optimize, seed=7, steps=E2E_STEPS):
    """Train on E2E_VIEWS views brightened by `brighten` (or not); returns (learned exposures [views, 3], mean held-out
    PSNR against unbrightened ground truth)."""
    views = E2E_VIEWS if brighten is None else len(brighten)
    n = views + E2E_HELD
    ex = None if brighten is None else np.concatenate([brighten, np.zeros(E2E_HELD, np.float32)])
    _, ims, pix = small_scene(pkg, ex, n=n, res=E2E_RES, seed=9)
    ds = pkg.nerf.NerfDataset(ims[:views], pix[:views])
    net, tr, run, cfg = new_run(pkg, ds, seed=seed, batch=1 << 16)
    run.set_camera_training(n_steps_between_cam_updates=E2E_BETWEEN)
    run.set_exposure_training(optimize=optimize)
    for _ in range(steps):
        run.train_step(get_loss=False)
    learned = exposures_of(run, views)
    r = pkg.nerf.NerfRenderer()
    psnr = [pkg.nerf.psnr(r.render(net, cfg, ims[k], run.bitfield, spp=1).cpu(), pkg.nerf.ground_truth_linear(pix[k]))[0]
            for k in range(views, n)]
    return learned, float(np.mean(psnr))


def test_training_recovers_known_exposures(pkg):
    """E2E_VIEWS views of the 64 x 64 procedural scene, each brightened by a known e_i (zero mean, about +-0.4), batch
    2^16, E2E_STEPS steps, an exposure update every E2E_BETWEEN steps (at the default 16 the per-update step of at most
    the learning rate, 1e-2, needs more steps than a test may take). The learned exposures x_i should approach -e_i (only
    the mean-free part is identifiable, and both have zero mean). With the switch off the residual x_i + e_i is e_i by
    construction; with it on its RMS must be under half of that. The held-out PSNR against unbrightened ground truth is
    reported, one run each; it is asserted only if the gap exceeds the spread of two off runs with different seeds.
    Measured once on an MI355X (a run repeats itself): residual RMS 0.2457 off, 0.1178 on, ratio 0.480; PSNR 27.06 dB off
    (27.04 dB with the other seed), 28.27 dB on. The ratio is not far below one half; why, and what else was tried, is in
    DESIGN.md §8f, and the 40-view test below has the margin this one lacks."""
    e = e2e_exposures()
    assert abs(float(e.mean())) < 1e-6 and 0.3 < np.abs(e).max() <= 0.8
    x_off, psnr_off = train_e2e(pkg, e, False)
    assert not x_off.any()
    x_on, psnr_on = train_e2e(pkg, e, True)
    rms_off = float(np.sqrt(((x_off + e[:, None]) ** 2).mean()))
    rms_on = float(np.sqrt(((x_on.astype(np.float64) + e[:, None]) ** 2).mean()))
    _, psnr_off_b = train_e2e(pkg, e, False, seed=11)
    print(f"exposure recovery, {E2E_VIEWS} views, {E2E_STEPS} steps, update every {E2E_BETWEEN}: residual RMS off {rms_off:.4f}, on "
          f"{rms_on:.4f}, ratio {rms_on / rms_off:.3f}; held-out PSNR off {psnr_off:.2f} dB (other seed {psnr_off_b:.2f}), on "
          f"{psnr_on:.2f} dB (one run each)")
    assert rms_on < 0.5 * rms_off
    if abs(psnr_on - psnr_off) > abs(psnr_off - psnr_off_b):
        assert psnr_on > psnr_off


def test_training_recovers_known_exposures_from_more_views(pkg):
    """The same run from 40 views: with twice the views the network's view-dependent colour can absorb less of a per-view
    brightness, and the residual falls well below the bar, which the 20-view run only just clears. The
    same bar, one half; measured once on an MI355X: ratio 0.217, correlation 0.986, PSNR 29.13 dB."""
    e = e2e_exposures(40)
    x_on, psnr_on = train_e2e(pkg, e, True)
    ratio = float(np.sqrt(((x_on.astype(np.float64) + e[:, None]) ** 2).mean()) / np.sqrt((e.astype(np.float64) ** 2).mean()))
    corr = float(np.corrcoef(x_on.astype(np.float64).mean(axis=1), -e)[0, 1])
    print(f"exposure recovery, 40 views, {E2E_STEPS} steps, update every {E2E_BETWEEN}: ratio {ratio:.3f}, correlation of the learned "
          f"exposures with -e {corr:.3f}; held-out PSNR {psnr_on:.2f} dB (one run)")
    assert ratio < 0.5


# ---- pyngp -------------------------------------------------------------------------------------------------------------------
def test_pyngp_exposure(pkg, tmp_path):
    import json
    from PIL import Image
    S = pkg.synthetic
    ngp = pkg.pyngp()
    frames = []
    for i, c2w in enumerate(S.camera_poses(4, seed=4)):
        Image.fromarray(S.render(c2w, 16, 16, exposure=0.3 * (i - 1.5))).save(tmp_path / f"r_{i}.png")
        frames.append({"file_path": f"./r_{i}", "transform_matrix": np.asarray(c2w, np.float64).tolist()})
    (tmp_path / "transforms.json").write_text(json.dumps({"camera_angle_x": S.LEGO_CAMERA_ANGLE_X, "frames": frames}))
    tb = ngp.Testbed()
    tb.load_training_data(str(tmp_path))
    tr = tb.nerf.training
    tr.n_steps_between_cam_updates = 2
    tr.exposure_l2_reg = 1e-3
    tr.optimize_exposure = True
    assert tr.optimize_exposure and tr.exposure_l2_reg == pytest.approx(1e-3)
    with pytest.raises(RuntimeError, match="optimize_exposure.*sample_image_proportional_to_error"):
        tr.sample_image_proportional_to_error = True
    tb.shall_train = True
    tb.frame()
    assert not tr.get_camera_exposure(0).any()
    for _ in range(3):
        tb.frame()
    e = np.array([tr.get_camera_exposure(i) for i in range(4)])
    assert e.shape == (4, 3) and (e != 0).all() and np.abs(e.mean(axis=0)).max() < 1e-6
    assert not tr.get_camera_exposure(7).any()
    tr.reset_camera_extrinsics()
    assert not np.array([tr.get_camera_exposure(i) for i in range(4)]).any()
    tb.reset()                                    # the switch outlives reset_network; the exposures start over
    assert tr.optimize_exposure
    tb.frame()
