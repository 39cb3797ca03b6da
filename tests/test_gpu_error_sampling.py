"""Error-driven ray sampling on the GPU (sample_focal_plane_proportional_to_error / sample_image_proportional_to_error):
the device form of the shared pixel lookup against its host form, the sampler and the loss pass with CDFs against the
numpy restatement of tests/test_error_sampling_host.py, the trainer's use of its own CDFs, the refusals and pyngp.

Runs are only ever compared with their OWN error map: the map is summed with float atomics, so two runs' CDFs differ
in their last bits.
"""
import json

import numpy as np
import pytest
import torch

import test_error_sampling_host as H
from test_error_sampling_host import F, FLAGS, N_IMG, N_RAYS, IMG_W, IMG_H, bits

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pkg():
    from __graft_entry__ import load_package
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return load_package()


@pytest.fixture(scope="module")
def scene(pkg):
    """H's four pinhole 48 x 32 images with rendered pixels."""
    S = pkg.synthetic
    ims = H.make_images(pkg)
    pix = [S.render(c2w, IMG_W, IMG_H) for c2w in S.camera_poses(N_IMG, seed=3)]
    return pkg.nerf.NerfDataset(ims, pix), ims, pix


def np_(d):
    return {k: v.cpu().numpy() for k, v in d.items()}


# ---- 4. device against host -------------------------------------------------------------------------------------
@pytest.mark.parametrize("snap", [1, 0])
@pytest.mark.parametrize("focal_plane,image", FLAGS)
def test_device_lookup_equals_host_bitwise(pkg, orc, scene, focal_plane, image, snap):
    ds, ims, _ = scene
    cfg = pkg.nerf.default_config(1.0, snap_to_pixel_centers=snap)
    cd = H.select(H.make_cdfs(orc), focal_plane, image)
    r = H.batch_rng(pkg)
    host = pkg.nerf.training_pixels(ims, cfg, N_RAYS, r, cdfs=cd, host=True)
    dev = np_(pkg.nerf.training_pixels(ds, cfg, N_RAYS, r, cdfs=cd))
    for k in ("img", "uv", "pdf"):
        np.testing.assert_array_equal(bits(dev[k]), bits(host[k]), err_msg=k)
    if focal_plane and image and snap:
        part = np_(pkg.nerf.training_pixels(ds, cfg, 3000, r, cdfs=cd, ray_offset=1000, n_rays_total=N_RAYS))
        for k in ("img", "uv", "pdf"):
            np.testing.assert_array_equal(bits(part[k]), bits(host[k][1000:4000]), err_msg=k)


# ---- 5. the sampler with CDFs -----------------------------------------------------------------------------------
def numpy_rays(orc, ims, img, uv):
    """uv_to_ray of a pinhole camera in the engine's operation order (no contraction): origin, unnormalised dir."""
    m = np.stack([orc.camera_matrix(np.array(im.xform[:], F)) for im in ims]).astype(F)[img]
    w = np.array([im.width for im in ims], F)[img]
    h = np.array([im.height for im in ims], F)[img]
    fx = np.array([im.focal_length[0] for im in ims], F)[img]
    fy = np.array([im.focal_length[1] for im in ims], F)[img]
    cx = np.array([im.principal_point[0] for im in ims], F)[img]
    cy = np.array([im.principal_point[1] for im in ims], F)[img]
    dx = (uv[:, 0] - cx) * w / fx
    dy = (uv[:, 1] - cy) * h / fy
    d = np.stack([m[:, k] * dx + m[:, 3 + k] * dy + m[:, 6 + k] * F(1) for k in range(3)], 1)
    return np.concatenate([m[:, 9:12], d], 1).astype(F)


def occupancy(orc, seed=4, frac=0.02):
    g = np.random.default_rng(seed)
    grid = np.where(g.random(128 ** 3 * 8) < frac, 1.0, 0.0).astype(np.float32)
    return torch.from_numpy(orc.nerf_grid_bitfield(grid, 0, 0.005)).cuda()


def test_sampler_with_cdfs(pkg, orc, scene):
    ds, ims, _ = scene
    cfg = pkg.nerf.default_config(1.0)
    n, max_samples = 4096, 1 << 18
    bf = occupancy(orc)
    r = H.batch_rng(pkg)
    cd = H.select(H.make_cdfs(orc), True, True)
    got = np_(pkg.nerf.generate_training_samples(ds, cfg, n, r, max_samples, bf, n_rays_total=n, cdfs=cd))
    ref = H.restate(orc, r, n, n, [(IMG_W, IMG_H)] * N_IMG, 1, cd)
    kept = int(got["counters"][0])
    assert kept > n // 2 and int(got["counters"][1]) <= max_samples
    idx = got["ray_indices"][:kept].view(np.uint32).astype(np.int64)
    assert (np.diff(idx) > 0).all() and idx[-1] < n
    want = numpy_rays(orc, ims, ref["img"].astype(np.int64), ref["uv"])
    np.testing.assert_array_equal(bits(got["rays"][:kept]), bits(want[idx]))
    # the CDFs moved the rays: the uniform sampler's are different
    plain = np_(pkg.nerf.generate_training_samples(ds, cfg, n, r, max_samples, bf, n_rays_total=n))
    assert not np.array_equal(plain["rays"][:kept], got["rays"][:kept])
    # null pointers: the uniform kernels, every output bit for bit
    null = np_(pkg.nerf.generate_training_samples(ds, cfg, n, r, max_samples, bf, n_rays_total=n, cdfs={}))
    for k in plain:
        np.testing.assert_array_equal(bits(null[k]), bits(plain[k]), err_msg=k)
    # two shards concatenate to the unsharded sample set (the image sample uses the global ray index)
    shards = [np_(pkg.nerf.generate_training_samples(ds, cfg, n // 2, r, max_samples, bf, ray_offset=lo, n_rays_total=n, cdfs=cd))
              for lo in (0, n // 2)]
    cat = lambda k, c: np.concatenate([s[k][:int(s["counters"][c])] for s in shards])
    np.testing.assert_array_equal(cat("ray_indices", 0), got["ray_indices"][:kept])
    np.testing.assert_array_equal(bits(cat("rays", 0)), bits(got["rays"][:kept]))
    np.testing.assert_array_equal(cat("numsteps", 0)[:, 0], got["numsteps"][:kept, 0])
    np.testing.assert_array_equal(bits(cat("coords", 1)), bits(got["coords"][:int(got["counters"][1])]))


# ---- 6. the loss with CDFs --------------------------------------------------------------------------------------
def numpy_deposit(img, uv, ml, n_img, em_h, em_w):
    """deposit_error of csrc/nerf_loss.hip (testbed_nerf.cu:1869-1899): weights in float32, sums in float64."""
    rx, ry = F(em_w), F(em_h)
    px = np.minimum(np.maximum(uv[:, 0] * rx - F(0.5), F(0)), rx - F(1.0 + 1e-4)).astype(F)
    py = np.minimum(np.maximum(uv[:, 1] * ry - F(0.5), F(0)), ry - F(1.0 + 1e-4)).astype(F)
    ix, iy = px.astype(np.int64), py.astype(np.int64)
    wx, wy = (px - ix.astype(F)).astype(np.float64), (py - iy.astype(F)).astype(np.float64)
    em = np.zeros((n_img, em_h, em_w))
    ml = ml.astype(np.float64)
    np.add.at(em, (img, iy, ix), (1 - wx) * (1 - wy) * ml)
    np.add.at(em, (img, iy, ix + 1), wx * (1 - wy) * ml)
    np.add.at(em, (img, iy + 1, ix), (1 - wx) * wy * ml)
    np.add.at(em, (img, iy + 1, ix + 1), wx * wy * ml)
    return em


def test_loss_with_cdfs(pkg, orc):
    """Every image is the same opaque colour, so a ray's target does not depend on which pixel it reads: with and
    without CDFs the loss pass sees the same samples, network output and targets, and only the division by the
    pixel's pdf differs. ngp_nerf_compute_loss_cdf has no sample-state argument (keep_state): that combination runs
    in the trainer only (test_trainer_samples_from_its_own_cdfs)."""
    S = pkg.synthetic
    ims = H.make_images(pkg)
    px = np.zeros((IMG_H, IMG_W, 4), np.uint8)
    px[...] = (200, 120, 40, 255)
    ds = pkg.nerf.NerfDataset(ims, [px] * N_IMG)
    cfg = pkg.nerf.default_config(1.0)
    n, max_samples, max_c = 4096, 1 << 18, 1 << 16
    bf = occupancy(orc)
    r = H.batch_rng(pkg)
    cd = H.select(H.make_cdfs(orc), True, True)
    samples = pkg.nerf.generate_training_samples(ds, cfg, n, r, max_samples, bf, n_rays_total=n, cdfs=cd)
    g = np.random.default_rng(5)
    out = torch.from_numpy(g.uniform(-3.0, 2.0, (max_samples, 16)).astype(np.float16)).cuda()
    mean = torch.tensor([0.003], device="cuda")
    em_h, em_w = 11, 13
    em = torch.zeros((N_IMG, em_h, em_w), dtype=torch.float32, device="cuda")
    s_on, s_off = ({k: v.clone() for k, v in samples.items()} for _ in range(2))
    on = np_(pkg.nerf.compute_loss(ds, cfg, n, r, max_c, s_on, out, mean, error_map=em, cdfs=cd))
    off = np_(pkg.nerf.compute_loss(ds, cfg, n, r, max_c, s_off, out, mean))
    assert int(on["compacted_counter"][0]) > 0
    np.testing.assert_array_equal(on["compacted_counter"], off["compacted_counter"])
    np.testing.assert_array_equal(s_on["numsteps"].cpu().numpy(), s_off["numsteps"].cpu().numpy())
    np.testing.assert_array_equal(bits(on["coords_compacted"]), bits(off["coords_compacted"]))
    np.testing.assert_array_equal(on["dloss_doutput"].view(np.uint16), off["dloss_doutput"].view(np.uint16))
    kept = int(samples["counters"][0])
    idx = samples["ray_indices"].cpu().numpy()[:kept].view(np.uint32).astype(np.int64)
    ref = H.restate(orc, r, n, n, [(IMG_W, IMG_H)] * N_IMG, 1, cd)
    pdf = (ref["pdf"][idx, 0] * ref["pdf"][idx, 1]).astype(F)
    assert (pdf != 1).sum() > kept // 2 and (off["loss"][:kept] > 0).sum() > kept // 2
    # both sides are sums of non-negative terms that differ by at most about eight float32 roundings (4.8e-7)
    np.testing.assert_allclose(on["loss"][:kept], off["loss"][:kept] / pdf, rtol=1e-6, atol=0)
    assert (on["loss"][kept:] == 0).all()
    want = numpy_deposit(ref["img"][idx].astype(np.int64), ref["uv"][idx], on["loss"][:kept] * F(n), N_IMG, em_h, em_w)
    assert want.sum() > 0
    # float atomics in any order: the bar of test_training_error_map_window / test_compute_loss
    np.testing.assert_allclose(em.cpu().numpy(), want, rtol=1e-4, atol=1e-6 * float(want.max()))


# ---- 7. the trainer ---------------------------------------------------------------------------------------------
N_VIEWS, VIEW_W = 8, 96


def new_run(pkg, ds):
    cfg = pkg.nerf.default_config(1.0)
    net = pkg.create_nerf_network(pkg.nerf_config("C2"))
    tr = pkg.Trainer(net, pkg.nerf_config("C2")["optimizer"])
    return net, tr, pkg.nerf.NerfTraining(net, tr, ds, cfg, seed=1337)


@pytest.fixture(scope="module")
def views(pkg):
    return pkg.synthetic.lego_like_dataset(n_images=N_VIEWS, width=VIEW_W, height=VIEW_W, seed=5)


def check_last_samples(pkg, ds, run, cdfs, same_as_uniform):
    """The step's rays are the public sampler's for the step's rng, ray count and budget with `cdfs`."""
    ls = run.last_samples()
    kept = int(ls["counters"][0])
    assert kept > 0
    mine = (ls["ray_indices"][:kept].cpu().numpy(), ls["rays"][:kept].cpu().numpy())
    again = pkg.nerf.generate_training_samples(ds, run.cfg, ls["n_rays"], ls["rng"], ls["max_samples"], run.bitfield,
                                               n_rays_total=ls["n_rays"], cdfs=cdfs)
    assert int(again["counters"][0]) == kept
    np.testing.assert_array_equal(again["ray_indices"][:kept].cpu().numpy(), mine[0])
    np.testing.assert_array_equal(bits(again["rays"][:kept].cpu().numpy()), bits(mine[1]))
    plain = pkg.nerf.generate_training_samples(ds, run.cfg, ls["n_rays"], ls["rng"], ls["max_samples"], run.bitfield,
                                               n_rays_total=ls["n_rays"])
    k = min(kept, int(plain["counters"][0]))
    same = int(plain["counters"][0]) == kept and np.array_equal(plain["rays"][:k].cpu().numpy(), mine[1][:k])
    assert same == same_as_uniform


def test_flags_change_nothing_before_the_first_window_closes(pkg, views):
    params = []
    for on in (True, False):
        net, tr, run = new_run(pkg, views)
        if on:
            run.set_error_sampling(focal_plane=True, image=True)
        assert run.error_sampling() == {"focal_plane": on, "image": on}
        for _ in range(128):
            run.train_step(get_loss=False)
        torch.cuda.synchronize()
        params.append(tr.params.cpu().numpy().view(np.uint16).copy())
        assert run.error_map()["cdf_valid"] == 1
    np.testing.assert_array_equal(params[0], params[1])


def test_trainer_samples_from_its_own_cdfs(pkg, views):
    """Windows close at steps 128 and 320. Pipelining off: last_samples holds the step's rays; the steps around both
    closes draw from the CDFs that were current when they sampled (none before 128; step 320 still the first
    window's, step 321 the second's). The loss falls on the way."""
    net, tr, run = new_run(pkg, views)
    run.set_pipeline(False)
    run.set_error_sampling(focal_plane=True, image=True)
    losses = {}
    for step in range(1, 322):
        before = run.error_map() if step == 320 else None
        s = run.train_step(get_loss=step in (1, 200))
        if step in (1, 200):
            losses[step] = s["loss"]
        if step in (127, 128):
            check_last_samples(pkg, views, run, None, same_as_uniform=True)
        elif step in (129, 319, 321):
            check_last_samples(pkg, views, run, run.error_map(), same_as_uniform=False)
        elif step == 320:
            em = run.error_map()
            assert em["n_steps_since_update"] == 0 and em["n_steps_between_updates"] == 288
            assert not np.array_equal(em["cdf_x_cond_y"], before["cdf_x_cond_y"])
            check_last_samples(pkg, views, run, before, same_as_uniform=False)
    assert np.isfinite(losses[200]) and losses[200] < losses[1]


def test_trainer_pipelined_samples_from_its_own_cdfs(pkg, views):
    """Pipelining on: a step's rays survive in last_samples only when no sampler was prelaunched after it, which is
    the case after the steps that are followed by a density-grid update (multiples of 8 up to 255, of 16 after).
    Step 128's sampler was prelaunched before any CDF existed; the samplers of steps 136 and 336 were prelaunched
    under steps 135 and 335 and read the first and the second window's CDFs."""
    net, tr, run = new_run(pkg, views)
    run.set_error_sampling(focal_plane=True, image=True)
    for step in range(1, 337):
        s = run.train_step(get_loss=step == 336)
        if step == 128:
            check_last_samples(pkg, views, run, None, same_as_uniform=True)
        elif step in (136, 336):
            check_last_samples(pkg, views, run, run.error_map(), same_as_uniform=False)
    assert np.isfinite(s["loss"]) and s["loss"] > 0


def test_one_switch_at_a_time(pkg, views):
    net, tr, run = new_run(pkg, views)
    run.set_pipeline(False)
    for _ in range(128):
        run.train_step(get_loss=False)
    for kw in ({"focal_plane": True, "image": False}, {"focal_plane": False, "image": True}):
        run.set_error_sampling(**kw)
        run.train_step(get_loss=False)
        em = run.error_map()
        sel = H.select(em, kw["focal_plane"], kw["image"])
        check_last_samples(pkg, views, run, sel, same_as_uniform=False)
    run.set_error_sampling(focal_plane=False, image=False)
    run.train_step(get_loss=False)
    check_last_samples(pkg, views, run, None, same_as_uniform=True)


# ---- 8. refusals --------------------------------------------------------------------------------------------------
def test_refused_together_with_pose_refinement(pkg, views):
    net, tr, run = new_run(pkg, views)
    run.set_camera_training(optimize_extrinsics=1)
    for kw in ({"focal_plane": True}, {"image": True}):
        with pytest.raises(Exception, match="optimize_extrinsics.*sample_focal_plane"):
            run.set_error_sampling(**kw)
        assert run.error_sampling() == {"focal_plane": False, "image": False}
    run.set_camera_training(optimize_extrinsics=0)
    for kw in ({"focal_plane": True, "image": False}, {"focal_plane": False, "image": True}):
        run.set_error_sampling(**kw)
        with pytest.raises(Exception, match="optimize_extrinsics.*sample_image"):
            run.set_camera_training(optimize_extrinsics=1)
        assert run.camera_training()["optimize_extrinsics"] == 0
        assert run.error_sampling() == kw
    run.train_step(get_loss=False)


# ---- 9. pyngp -----------------------------------------------------------------------------------------------------
def test_pyngp_properties(pkg, tmp_path):
    from PIL import Image
    S = pkg.synthetic
    frames = []
    for i, c2w in enumerate(S.camera_poses(N_VIEWS, seed=4)):
        Image.fromarray(S.render(c2w, VIEW_W, VIEW_W)).save(tmp_path / f"r_{i}.png")
        frames.append({"file_path": f"./r_{i}", "transform_matrix": np.asarray(c2w, np.float64).tolist()})
    (tmp_path / "transforms.json").write_text(json.dumps({"camera_angle_x": S.LEGO_CAMERA_ANGLE_X, "frames": frames}))
    ngp = pkg.pyngp()
    tb = ngp.Testbed()
    tb.load_training_data(str(tmp_path))
    tr = tb.nerf.training
    assert tr.sample_focal_plane_proportional_to_error is False and tr.sample_image_proportional_to_error is False
    tr.sample_focal_plane_proportional_to_error = True  # before there is a trainer
    assert tr.sample_focal_plane_proportional_to_error is True and tr.sample_image_proportional_to_error is False
    with pytest.raises(Exception, match="optimize_extrinsics"):
        tr.optimize_extrinsics = True
    assert tr.optimize_extrinsics is False
    for _ in range(4):
        tb.train(1 << 18)
    tr.sample_image_proportional_to_error = True  # pushed to the live trainer
    assert tr.sample_focal_plane_proportional_to_error is True and tr.sample_image_proportional_to_error is True
    with pytest.raises(Exception, match="optimize_extrinsics"):
        tr.optimize_extrinsics = True
    assert tr.optimize_extrinsics is False
    while tb.training_step < 130:
        tb.train(1 << 18)
    assert tb.training_step == 130 and np.isfinite(tb.loss) and tb.loss > 0
