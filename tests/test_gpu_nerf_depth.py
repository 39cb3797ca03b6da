"""Depth supervision on the GPU: the dataset's depth images, the loss pass's DEPTH instantiations (k_loss_pass1 /
k_loss_pass2, all three forms of pass 2) against the float64 restatement of test_nerf_depth_host.py on its 300-ray batch
and depth images, the switch-off identities (bitwise), the combinations with error-map CDFs and an environment map, the
trainer, an end-to-end run on the procedural scene, and pyngp.

Bounds: integers and compacted coordinates equal; loss[] bitwise equal to the same call with lambda 0 (the depth term
does not enter it); each fp16 gradient element within 4 K32D 2^-24 companion + half an fp16 ulp + one ulp for a flipped
rounding (K32D and the companion: test_nerf_depth_host.py's docstring), no element left out."""
import json

import numpy as np
import pytest
import torch

from test_nerf_depth_host import COLOUR_CONFIGS, DEPTH_LAMBDA, DEPTH_LOSSES, K32D, MARGIN_TARGET, depth_world, restate_loss_depth
from test_nerf_loss_host import MARGIN_HUBER, MARGIN_SIGN, N_RAYS_TOTAL, RAY_COUNTS, compaction_cases, compare, make_cfg

pytestmark = pytest.mark.gpu
K_GPU = 4 * K32D
MAX_C = 1 << 13


@pytest.fixture(scope="module")
def pkg():
    from __graft_entry__ import load_package
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return load_package()


def attach(ds, maps):
    for i, m in enumerate(maps):
        if m is not None:
            ds.set_depth(i, m[0], m[1])
    return ds


@pytest.fixture(scope="module")
def world(pkg):
    mine, maps, stored = depth_world(pkg)
    return mine, maps, stored, attach(pkg.nerf.NerfDataset(mine.images, mine.pixels), maps)


def to_device(samples):
    return {k: torch.from_numpy(v.view(np.int32) if v.dtype == np.uint32 else v).cuda() for k, v in samples.items()}


def run(pkg, ds, batch, cfg, mean=0.003, max_c=MAX_C, n_rays=None, counter=None, px_total=N_RAYS_TOTAL, **kw):
    n = batch.n_rays if n_rays is None else n_rays
    s = to_device(batch.samples(n, counter))
    out = torch.from_numpy(batch.out(int(cfg.density_activation))).cuda()
    got = pkg.nerf.compute_loss(ds, cfg, n, batch.rng, max_c, s, out, torch.tensor([mean], device="cuda"),
                                n_rays_total=px_total, **kw)
    torch.cuda.synchronize()
    res = {k: v.cpu().numpy() for k, v in got.items()}
    res["numsteps"] = s["numsteps"].cpu().numpy()
    return res


def check(ref, got, max_c=MAX_C, loss=True):
    """test_nerf_loss_host.compare with the depth bound, and what must stay zero: columns 4..15 of dloss_doutput, the
    rows at and past the compacted total."""
    worst = compare(ref, got["loss"] if loss else ref["loss"], got["dloss_doutput"], got["numsteps"],
                    got["compacted_counter"].view(np.uint32)[0], got["coords_compacted"], K_GPU)
    used = ref["row"].size
    assert used == min(ref["compacted_counter"], max_c)
    assert not got["dloss_doutput"].view(np.uint16)[:, 4:].any()
    assert not got["dloss_doutput"].view(np.uint16)[used:].any() and not got["coords_compacted"].view(np.uint32)[used:].any()
    return worst


def bitwise_equal(a, b, keys=("numsteps", "compacted_counter", "coords_compacted", "loss", "dloss_doutput")):
    for k in keys:
        x, y = (a[k].view(np.uint16), b[k].view(np.uint16)) if k == "dloss_doutput" else (a[k].view(np.uint32), b[k].view(np.uint32))
        np.testing.assert_array_equal(x, y, err_msg=k)


# ---- the dataset -----------------------------------------------------------------------------------------------------------
def test_dataset_depth_round_trip(pkg, world):
    mine, maps, stored, _ = world
    ds = pkg.nerf.NerfDataset(mine.images, mine.pixels)
    assert all(ds.depth(i) is None for i in range(3))
    g = np.random.default_rng(2)
    h, w = mine.pixels[1].shape[:2]
    u16 = g.integers(0, 65536, (h, w)).astype(np.uint16)
    f32 = (g.random((h, w)) * 7.3).astype(np.float32)
    for arr, scale in ((u16, 1.0 / 3.0), (u16, 0.001), (f32, 0.37), (f32, 1.0)):
        ds.set_depth(1, arr, scale)
        got = ds.depth(1)
        np.testing.assert_array_equal(got.view(np.uint32), (arr.astype(np.float32) * np.float32(scale)).view(np.uint32))
        assert ds.depth(0) is None and ds.depth(2) is None
    ds.set_depth(1, u16, 0.0)                       # scale 0: zeros
    assert ds.depth(1) is not None and not ds.depth(1).any()
    ds.set_depth(1, u16, 0.5)
    ds.set_depth(1, None)                           # NULL: zeros
    assert ds.depth(1) is not None and not ds.depth(1).any()
    ds.set_depth(1, None, -1.0)                     # NULL and a negative scale: the image has no depth any more
    assert ds.depth(1) is None
    ds.set_depth(1, None, -1.0)                     # and again: nothing to remove
    L = pkg.lib()
    assert L.ngp_nerf_dataset_set_depth(ds.handle, 3, u16.ctypes.data, 0, 1.0) == -2       # image index
    assert L.ngp_nerf_dataset_set_depth(ds.handle, 1, u16.ctypes.data, 2, 1.0) == -2       # dtype
    assert L.ngp_nerf_dataset_set_depth(ds.handle, 1, u16.ctypes.data, 0, float("nan")) == -2
    assert L.ngp_nerf_dataset_depth(ds.handle, 3, None, 0, None) == -2
    assert ds.depth(1) is None
    with pytest.raises(ValueError):
        ds.set_depth(1, u16[:-1], 1.0)
    with pytest.raises(ValueError):
        ds.set_depth(1, u16.astype(np.float64), 1.0)
    # the batch's images as the tests attach them
    _, _, _, attached = world
    for i, st in enumerate(stored):
        if st is None:
            assert attached.depth(i) is None
        else:
            np.testing.assert_array_equal(attached.depth(i).view(np.uint32), st.view(np.uint32))


# ---- the loss pass ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("depth_loss", DEPTH_LOSSES)
def test_loss_pass_with_depth_matches_float64(pkg, world, depth_loss):
    """Every depth loss x {Huber, L2} colour loss x {Exp / Exp, None / None}, the plain form, the 300-ray batch."""
    mine, maps, stored, ds = world
    worst = 0.0
    for loss, r, d in COLOUR_CONFIGS:
        cfg = make_cfg(pkg, loss, r, d)
        ref = restate_loss_depth(mine, cfg, stored, DEPTH_LAMBDA, depth_loss, max_compacted=MAX_C)
        got = run(pkg, ds, mine, cfg, depth_lambda=DEPTH_LAMBDA, depth_loss=depth_loss)
        off = run(pkg, ds, mine, cfg)
        np.testing.assert_array_equal(got["loss"].view(np.uint32), off["loss"].view(np.uint32))
        ul, ug = check(ref, got)
        # the term is there: the density column moved on rays with a live target, and only there
        moved = (got["dloss_doutput"][:, 3] != off["dloss_doutput"][:, 3])[ref["row"]]
        live = ref["live"][ref["ray"]]
        assert moved[live].mean() > 0.5 and not moved[~live].any()
        np.testing.assert_array_equal(got["dloss_doutput"][:, :3].view(np.uint16), off["dloss_doutput"][:, :3].view(np.uint16))
        worst = max(worst, ug)
        print(f"depth {depth_loss}, colour {loss} rgb={r} density={d}: worst err / bound, gradient (beyond half an fp16 ulp) "
              f"{ug / K_GPU:.3f}, loss {ul / K_GPU:.3f}")
    assert ref["compacted_counter"] > 1000


@pytest.mark.parametrize("n_rays", RAY_COUNTS)
def test_ray_counts_with_depth(pkg, world, n_rays):
    """The first n rays as a batch of their own: the plain form (pass 2 composites again), keep_state (a wave per ray
    reads the six kept planes) and keep_state with a third of the capacity (the rays past it: the per-lane form) give the
    same bits, and the float64 values."""
    mine, maps, stored, ds = world
    for (loss, r, d), dl in zip(COLOUR_CONFIGS, ("L1", "Huber")):
        cfg = make_cfg(pkg, loss, r, d)
        ref = restate_loss_depth(mine, cfg, stored, DEPTH_LAMBDA, dl, max_compacted=MAX_C, n_rays=n_rays)
        kw = dict(n_rays=n_rays, depth_lambda=DEPTH_LAMBDA, depth_loss=dl)
        plain = run(pkg, ds, mine, cfg, **kw)
        ul, ug = check(ref, plain)
        kept = run(pkg, ds, mine, cfg, keep_state=True, **kw)
        bitwise_equal(plain, kept)
        short = run(pkg, ds, mine, cfg, keep_state=True, state_capacity=max(mine.total // 3, 1), **kw)
        bitwise_equal(plain, short)
    print(f"{n_rays} rays with depth: worst err / bound, gradient {ug / K_GPU:.3f}")


@pytest.mark.parametrize("case", range(5))
def test_compaction_with_depth(pkg, world, case):
    """The compaction cases of the colour tests with depth on: a ray cut by the budget uses the whole depth_ray of pass 1
    in its suffix, as the reference does; all three forms of pass 2."""
    mine, maps, stored, ds = world
    cfg = make_cfg(pkg)
    max_c, counter = compaction_cases(mine, cfg)[case]
    ref = restate_loss_depth(mine, cfg, stored, DEPTH_LAMBDA, "L2", max_compacted=max_c, counter=counter)
    if case == 1:
        cut = np.nonzero((ref["cnum"] > 0) & (ref["cnum"] < ref["cn"]))[0]
        assert cut.size == 1
    kw = dict(max_c=max_c, counter=counter, depth_lambda=DEPTH_LAMBDA, depth_loss="L2")
    plain = run(pkg, ds, mine, cfg, **kw)
    ul, ug = check(ref, plain, max_c)
    for cap in (None, mine.total // 3, 1):
        bitwise_equal(plain, run(pkg, ds, mine, cfg, keep_state=True, state_capacity=cap, **kw))
    print(f"compaction case {case} with depth: worst err / bound, gradient {ug / K_GPU:.3f}")


def test_switch_off_identities(pkg, world):
    """Bitwise: lambda 0 through the depth entry point with depth attached, lambda > 0 with all-zero depth images, and
    lambda > 0 on a dataset without depth, each equal to the plain entry points on a dataset without depth; with
    keep_state and with an error map too."""
    mine, maps, stored, ds = world
    bare = pkg.nerf.NerfDataset(mine.images, mine.pixels)
    zeros = pkg.nerf.NerfDataset(mine.images, mine.pixels)
    for i, m in enumerate(maps):
        if m is not None:
            zeros.set_depth(i, np.zeros_like(m[0]), m[1])
    for loss, r, d in COLOUR_CONFIGS:
        cfg = make_cfg(pkg, loss, r, d)
        plain = run(pkg, bare, mine, cfg)
        on = run(pkg, ds, mine, cfg, depth_lambda=DEPTH_LAMBDA)
        assert (on["dloss_doutput"].view(np.uint16) != plain["dloss_doutput"].view(np.uint16)).any()
        for dset, lam in ((ds, 0.0), (zeros, DEPTH_LAMBDA), (bare, DEPTH_LAMBDA)):
            for kw in ({}, {"keep_state": True}, {"keep_state": True, "state_capacity": mine.total // 3}):
                bitwise_equal(plain, run(pkg, dset, mine, cfg, depth_lambda=lam, depth_loss="L2", depth_entry=True, **kw))
        em0 = torch.zeros((3, 7, 9), device="cuda")
        em1 = torch.zeros((3, 7, 9), device="cuda")
        a = run(pkg, bare, mine, cfg, error_map=em0)
        b = run(pkg, ds, mine, cfg, error_map=em1, depth_lambda=DEPTH_LAMBDA)     # the depth term is not deposited
        bitwise_equal(a, b, keys=("numsteps", "compacted_counter", "coords_compacted", "loss"))
        np.testing.assert_allclose(em1.cpu().numpy(), em0.cpu().numpy(), rtol=1e-5, atol=1e-9)
        assert em0.sum() > 0


def make_training(pkg, ds, seed=1337, batch=1 << 14, **cfg_kw):
    ncfg = pkg.nerf_config("C2")
    ncfg["encoding"]["log2_hashmap_size"] = 14
    net = pkg.create_nerf_network(ncfg)
    tr = pkg.Trainer(net, ncfg["optimizer"], seed=seed)
    cfg = pkg.nerf.default_config(1.0, target_batch_size=batch, **cfg_kw)
    return pkg.nerf.NerfTraining(net, tr, ds, cfg, seed=seed), net, tr, cfg


def scene(pkg, n, res=64, seed=3, depth=True):
    """n views of the procedural scene with their z-depth attached (in the engine's units: scale 0.33)."""
    S = pkg.synthetic
    ims, pix, dep = [], [], []
    for c2w in S.camera_poses(n, seed=seed):
        ims.append(pkg.nerf.make_image(res, res, pkg.nerf.nerf_matrix_to_ngp(c2w), camera_angle_x=S.LEGO_CAMERA_ANGLE_X))
        p, d = S.render(c2w, res, res, return_depth=True)
        pix.append(p)
        dep.append(d)
    return ims, pix, dep


def test_trainer_with_lambda_zero_is_the_trainer_without_depth(pkg):
    """20 steps with depth attached and lambda 0 leave the parameters byte-identical to a trainer on a dataset without
    depth; with lambda > 0 they differ after the first step; the setter's values come back; bad values are refused."""
    ims, pix, dep = scene(pkg, 6)
    bare = pkg.nerf.NerfDataset(ims, pix)
    with_depth = pkg.nerf.NerfDataset(ims, pix)
    for i, d in enumerate(dep):
        with_depth.set_depth(i, d, 0.33)
    a, _, tra, _ = make_training(pkg, bare)
    b, _, trb, _ = make_training(pkg, with_depth)
    c, _, trc, _ = make_training(pkg, with_depth)
    e, _, tre, _ = make_training(pkg, bare)
    assert b.depth_supervision() == (0.0, "L1")
    c.set_depth_supervision(0.25, "Huber")
    assert c.depth_supervision() == (0.25, "Huber")
    e.set_depth_supervision(0.25, "Huber")         # no image has depth: the plain step
    for bad in ((-1.0, "L1"), (float("nan"), "L1"), (float("inf"), "L1"), (0.5, 9)):
        with pytest.raises(pkg.NgpError):
            c.set_depth_supervision(*bad)
    assert c.depth_supervision() == (0.25, "Huber")
    for run_ in (a, b, c, e):
        run_.train_step(get_loss=False)
    torch.cuda.synchronize()
    pa, pc = tra.params.cpu().numpy().view(np.uint16), trc.params.cpu().numpy().view(np.uint16)
    assert (pa != pc).mean() > 0.01
    for _ in range(19):
        for run_ in (a, b, e):
            run_.train_step(get_loss=False)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(tra.params.cpu().numpy().view(np.uint16), trb.params.cpu().numpy().view(np.uint16))
    np.testing.assert_array_equal(tra.params.cpu().numpy().view(np.uint16), tre.params.cpu().numpy().view(np.uint16))


# ---- combinations ------------------------------------------------------------------------------------------------------
def error_cdfs(n_images, w, h, seed):
    g = np.random.default_rng(seed)
    pmf = g.random((n_images, h, w)) + 0.05
    cdf_x = np.cumsum(pmf, axis=2) / pmf.sum(axis=2, keepdims=True)
    rows = pmf.sum(axis=2)
    cdf_y = np.cumsum(rows, axis=1) / rows.sum(axis=1, keepdims=True)
    tot = rows.sum(axis=1)
    return {"cdf_x_cond_y": cdf_x.astype(np.float32), "cdf_y": cdf_y.astype(np.float32),
            "cdf_img": (np.cumsum(tot) / tot.sum()).astype(np.float32)}


def test_depth_with_error_map_cdfs(pkg, world):
    """The CDF instantiation with depth: the rays' pixels come from error-map CDFs (so other texels, images and pdfs),
    against the float64 restatement at those pixels. The CDFs' seed is the first whose pixels keep every ray away from
    every decision margin, colour and depth (found on the host, no exclusions). loss[] equals the lambda-0 call's."""
    mine, maps, stored, ds = world
    cfg = make_cfg(pkg)
    for seed in range(40):
        cd = error_cdfs(3, 5, 4, seed)
        px_all = pkg.nerf.training_pixels(mine.images, mine.cfg0, N_RAYS_TOTAL, mine.rng, cdfs=cd, host=True)
        px = {"img": px_all["img"][mine.ray_indices], "uv": px_all["uv"][mine.ray_indices]}
        ref = restate_loss_depth(mine, cfg, stored, DEPTH_LAMBDA, "L1", max_compacted=MAX_C, px=px)
        m, dm = ref["margins"], ref["depth_margins"]
        alive = ref["cn"] > 0
        ok = (m["huber"][alive].min() >= MARGIN_HUBER and m["srgb_knee"][alive].min() >= 1e-6 and dm["sign"].min() >= MARGIN_SIGN
              and dm["target"].min() >= MARGIN_TARGET)
        if ok:
            break
    assert ok
    assert (px["img"] != mine.px["img"]).any() and (ref["live"] & (ref["cnum"] > 0)).sum() > 30
    got = run(pkg, ds, mine, cfg, cdfs=cd, depth_lambda=DEPTH_LAMBDA, depth_loss="L1")
    off = run(pkg, ds, mine, cfg, cdfs=cd)
    np.testing.assert_array_equal(got["loss"].view(np.uint32), off["loss"].view(np.uint32))
    assert (got["dloss_doutput"].view(np.uint16) != off["dloss_doutput"].view(np.uint16)).any()
    ul, ug = check(ref, got, loss=False)     # loss[] is divided by the pixels' pdf: checked against the lambda-0 call above
    kept = run(pkg, ds, mine, cfg, cdfs=cd, depth_lambda=DEPTH_LAMBDA, depth_loss="L1", keep_state=True)
    bitwise_equal(got, kept)
    print(f"depth with CDFs (seed {seed}): worst err / bound, gradient {ug / K_GPU:.3f}")


def test_depth_with_an_environment_map(pkg, world):
    """The ENV instantiations with depth, the map's gradient bound. The map is all zeros (rgb 0, alpha 0: the background
    behind it comes through exactly, so the float64 restatement holds as it stands); its gradient is what the lambda-0
    call deposits, bit for bit, since the depth term does not enter it, and it is not zero."""
    mine, maps, stored, ds = world
    cfg = make_cfg(pkg)
    ref = restate_loss_depth(mine, cfg, stored, DEPTH_LAMBDA, "SMAPE", max_compacted=MAX_C)
    env = torch.zeros((4, 8, 4), device="cuda")
    g_on, g_off = torch.full((4, 8, 4), 7.0, device="cuda"), torch.full((4, 8, 4), 7.0, device="cuda")
    got = run(pkg, ds, mine, cfg, envmap=env, envmap_gradient=g_on, depth_lambda=DEPTH_LAMBDA, depth_loss="SMAPE")
    off = run(pkg, ds, mine, cfg, envmap=env, envmap_gradient=g_off)
    ul, ug = check(ref, got)
    np.testing.assert_array_equal(got["loss"].view(np.uint32), off["loss"].view(np.uint32))
    np.testing.assert_array_equal(g_on.cpu().numpy().view(np.uint32), g_off.cpu().numpy().view(np.uint32))
    assert g_on[..., :3].abs().max() > 0 and not g_on[..., 3].any()
    assert (got["dloss_doutput"].view(np.uint16) != off["dloss_doutput"].view(np.uint16)).any()
    kept = run(pkg, ds, mine, cfg, envmap=env, envmap_gradient=g_off, depth_lambda=DEPTH_LAMBDA, depth_loss="SMAPE", keep_state=True,
               state_capacity=mine.total // 3)
    bitwise_equal(got, kept)
    print(f"depth with an environment map: worst err / bound, gradient {ug / K_GPU:.3f}, loss {ul / K_GPU:.3f}")


def test_depth_with_pose_refinement_and_data_parallel_are_not_refused(pkg):
    ims, pix, dep = scene(pkg, 4, res=32)
    ds = pkg.nerf.NerfDataset(ims, pix)
    for i, d in enumerate(dep):
        ds.set_depth(i, d, 0.33)
    run_, _, tr, _ = make_training(pkg, ds, batch=1 << 12)
    run_.set_depth_supervision(0.5)
    run_.set_camera_training(optimize_extrinsics=True)
    for _ in range(3):
        run_.train_step(get_loss=False)
    torch.cuda.synchronize()
    assert np.isfinite(tr.params.float().cpu().numpy()).all()
    # data parallelism: the term is per ray, so neither order of the two settings is refused
    dp, _, tr2, _ = make_training(pkg, ds, batch=1 << 12)
    dp.set_depth_supervision(0.5)
    assert pkg.lib().ngp_nerf_trainer_set_data_parallel(dp.handle, 0, 1, None, None) == 0
    dp.set_depth_supervision(0.25, "L2")
    assert dp.depth_supervision() == (0.25, "L2")
    for _ in range(3):
        dp.train_step(get_loss=False)
    torch.cuda.synchronize()
    assert np.isfinite(tr2.params.float().cpu().numpy()).all()


# ---- end to end ------------------------------------------------------------------------------------------------------------
E2E_VIEWS, E2E_HELD, E2E_STEPS, E2E_LAMBDA = 6, 4, 1000, 0.1


def depth_rmse(pkg, n_train, seed, lam, steps=E2E_STEPS, n_held=E2E_HELD):
    """Train on n_train views of the 64x64 procedural scene, render the held-out views in Depth mode (Blender units:
    depth_scale 1 / 0.33) and return (RMSE of the depth over pixels whose true alpha is 1, mean PSNR)."""
    S = pkg.synthetic
    ims, pix, dep = scene(pkg, n_train + n_held, seed=9)
    ds = pkg.nerf.NerfDataset(ims[:n_train], pix[:n_train])
    for i in range(n_train):
        ds.set_depth(i, dep[i], 0.33)
    run_, net, tr, cfg = make_training(pkg, ds, seed=seed, batch=1 << 16)
    run_.set_depth_supervision(lam, "L1")
    for _ in range(steps):
        run_.train_step(get_loss=False)
    r = pkg.nerf.NerfRenderer()
    se, cnt, psnr = 0.0, 0, []
    for k in range(n_train, n_train + n_held):
        img = r.render(net, cfg, ims[k], run_.bitfield, spp=1, render_mode="Depth", depth_scale=1.0 / 0.33).cpu().numpy()
        a = np.maximum(img[..., 3], 1e-3)
        z = np.where(img[..., 3] > 1e-3, img[..., 0] / a, 0.0)
        solid = pix[k][..., 3] == 255
        se += float(((z - dep[k])[solid] ** 2).sum())
        cnt += int(solid.sum())
        shade = r.render(net, cfg, ims[k], run_.bitfield, spp=1)
        psnr.append(pkg.nerf.psnr(shade.cpu(), pkg.nerf.ground_truth_linear(pix[k]))[0])
    return float(np.sqrt(se / cnt)), float(np.mean(psnr))


def test_depth_supervision_improves_held_out_depth(pkg):
    """E2E_VIEWS training views of the 64x64 procedural scene (so few that colour alone leaves the geometry loose),
    E2E_STEPS steps at a batch of 2^16, the same seed with lambda 0 and with lambda E2E_LAMBDA (L1), and the unsupervised
    run once more with another seed. Held-out depth RMSE over pixels whose true alpha is 1: the supervised run must be
    below the unsupervised one by more than the two unsupervised seeds differ. Measured once on an MI355X (a run repeats
    itself): 6 views, 1000 steps: RMSE 0.228 (the other seed: 0.182) without, 0.086 with depth, in Blender units, where
    the cameras stand 4.03 from the origin; PSNR 19.13 -> 22.68 dB. With 3, 4 and 10 views the same order holds (0.483 ->
    0.170, 0.391 -> 0.189, 0.108 -> 0.059); at 10 views colour alone already finds most of the geometry. lambda 1 gives
    the same RMSEs here (0.083), but over a few thousand steps at full resolution an L1 depth term of that weight
    outweighs the colour loss and empties the scene, so the test uses 0.1."""
    off_a, psnr_off = depth_rmse(pkg, E2E_VIEWS, 1337, 0.0)
    off_b, _ = depth_rmse(pkg, E2E_VIEWS, 7, 0.0)
    on_a, psnr_on = depth_rmse(pkg, E2E_VIEWS, 1337, E2E_LAMBDA)
    print(f"held-out depth RMSE (Blender units) with {E2E_VIEWS} views, {E2E_STEPS} steps: lambda 0 {off_a:.4f} (other seed "
          f"{off_b:.4f}), lambda {E2E_LAMBDA} {on_a:.4f}; PSNR {psnr_off:.2f} dB -> {psnr_on:.2f} dB")
    assert off_a - on_a > abs(off_a - off_b)


# ---- pyngp ---------------------------------------------------------------------------------------------------------------
def test_pyngp_depth(pkg, tmp_path):
    from PIL import Image
    S = pkg.synthetic
    ngp = pkg.pyngp()
    frames, depths = [], []
    for i, c2w in enumerate(S.camera_poses(3, seed=4)):
        rgba, z = S.render(c2w, 16, 16, return_depth=True)
        Image.fromarray(rgba).save(tmp_path / f"r_{i}.png")
        fr = {"file_path": f"./r_{i}", "transform_matrix": np.asarray(c2w, np.float64).tolist()}
        if i < 2:
            d16 = np.round(z * 1000).astype(np.uint16)          # millimetres
            Image.fromarray(d16).save(tmp_path / f"d_{i}.png")
            fr["depth_path"] = f"d_{i}.png"
            depths.append(d16)
        frames.append(fr)
    (tmp_path / "transforms.json").write_text(json.dumps({"camera_angle_x": S.LEGO_CAMERA_ANGLE_X, "integer_depth_scale": 0.001,
                                                          "frames": frames}))
    tb = ngp.Testbed()
    tb.load_training_data(str(tmp_path))
    tr = tb.nerf.training
    assert tr.depth_supervision_lambda == 0.0 and tr.depth_loss_type == ngp.LossType.L1
    tr.depth_supervision_lambda = 0.5
    tr.depth_loss_type = ngp.LossType.Huber
    assert tr.depth_supervision_lambda == 0.5 and tr.depth_loss_type == ngp.LossType.Huber
    with pytest.raises(RuntimeError):
        tr.depth_supervision_lambda = -1.0
    assert tr.depth_supervision_lambda == 0.5
    scale = np.float32(0.001) * np.float32(0.33)
    loaded = [tr.depth_image(i) for i in range(3)]
    assert loaded[2] is None
    for got, d16 in zip(loaded, depths):
        np.testing.assert_array_equal(got.view(np.uint32), (d16.astype(np.float32) * scale).view(np.uint32))
    # set_image's depth part gives the same dataset depth as the loader
    tb2 = ngp.Testbed()
    (tmp_path / "transforms.json").write_text(json.dumps({"camera_angle_x": S.LEGO_CAMERA_ANGLE_X, "frames": frames}))
    tb2.load_training_data(str(tmp_path))
    assert all(tb2.nerf.training.depth_image(i) is None for i in range(3))
    for i, d16 in enumerate(depths):
        tb2.nerf.training.set_image(i, None, d16, float(scale))
        np.testing.assert_array_equal(tb2.nerf.training.depth_image(i), loaded[i])
    tb2.nerf.training.set_image(0, None, depths[0].astype(np.float32), float(scale))
    np.testing.assert_array_equal(tb2.nerf.training.depth_image(0), loaded[0])
    with pytest.raises(RuntimeError):
        tb2.nerf.training.set_image(0, np.zeros((16, 16, 4), np.float32), depths[0], 1.0)     # colours: not supported
    with pytest.raises(RuntimeError):
        tb2.nerf.training.set_image(0, None, depths[0][:-1], 1.0)
    # it trains: the step runs with the depth term, and the setting outlives reset_network
    tb.shall_train = True
    for _ in range(3):
        tb.frame()
    tb.reset()
    tb.frame()
    assert tb.nerf.training.depth_supervision_lambda == 0.5 and tb.nerf.training.depth_image(0) is not None
