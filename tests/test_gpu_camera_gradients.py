"""GPU tests of the NeRF camera pose refinement: the per-image extrinsics gradient kernels
(ngp_nerf_camera_gradients), the input gradient inside the training step, and the trainer's refinement loop.

The float64 restatement of the gradient sums is written here from the kernel's definition: per kept ray with n > 0
samples, d = normalize(ray.d), o = ray.o, diag = aabb_max - aabb_min,
    g_pos_j = coords_grad[base + j].pos / diag,  pos = aabb_min + coords[base + j].pos * diag,
    go += g_pos_j,  gd += g_pos_j * |pos - o| + coords_grad[base + j].dir * 0.5,
    pos_grad[img] += go,  rot_grad[img] += cross(d, gd),  img = (ray_index * n_images) // n_rays_total % n_images.
"""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
# The issue asks for 3,000 kept rays of 4,096 with one image empty and one holding a single ray. The two do not fit:
# image_idx gives each of the 7 images 585 or 586 of the 4,096 ray ids, so with those two images out at most 2,927 rays
# can be kept. The empty and the single-ray image are the cases that matter; the count is 2,900.
N_IMAGES, N_TOTAL, N_KEPT = 7, 4096, 2900
EMPTY_IMAGE, SINGLE_IMAGE = 3, 5
BOX = ([-1.5] * 3, [2.5] * 3)


@pytest.fixture(scope="module")
def pkg():
    from __graft_entry__ import load_package
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return load_package()


def image_of(ray_idx, n_total, n_images):
    return (ray_idx.astype(np.int64) * n_images) // n_total % n_images


def hand_batch(seed=0):
    """2,900 kept rays of 4,096 over 7 images: one image without a kept ray, one with a single ray; sample counts
    mixed from {0, 1, 2, 63, 64, 65, 200}. Ray origins lie outside the box, so |pos - o| has no cancellation."""
    g = np.random.default_rng(seed)
    ids = np.arange(N_TOTAL)
    img = image_of(ids, N_TOTAL, N_IMAGES)
    single = g.choice(ids[img == SINGLE_IMAGE])
    pool = ids[(img != EMPTY_IMAGE) & (img != SINGLE_IMAGE)]
    kept = np.sort(np.concatenate([g.choice(pool, N_KEPT - 1, replace=False), [single]])).astype(np.uint32)
    n = g.choice(np.array([0, 1, 2, 63, 64, 65, 200], np.uint32), N_KEPT)
    n[kept == single] = 2
    base = np.concatenate([[0], np.cumsum(n)[:-1]]).astype(np.uint32)
    B = int(n.sum())
    rays = np.concatenate([g.uniform(3.0, 4.0, (N_KEPT, 3)), g.standard_normal((N_KEPT, 3)) * 2.0], 1).astype(np.float32)
    coords = g.random((B, 7)).astype(np.float32)
    grad = g.standard_normal((B, 7)).astype(np.float32)
    return {"kept": kept, "numsteps": np.stack([n, base], 1).astype(np.uint32), "rays": rays, "coords": coords,
            "grad": grad, "counters": np.array([N_KEPT, B], np.uint32)}


def restate(b, n_kept, n_total=N_TOTAL, n_images=N_IMAGES, box=BOX):
    """float64 sums, with each output component's number of terms and sum of |term|."""
    lo, hi = np.float64(np.float32(box[0])), np.float64(np.float32(box[1]))
    diag = hi - lo
    n = b["numsteps"][:n_kept, 0].astype(np.int64)
    base = b["numsteps"][:n_kept, 1].astype(np.int64)
    ray = np.repeat(np.arange(n_kept), n)
    row = np.concatenate([np.arange(bb, bb + nn) for bb, nn in zip(base, n)]) if n.sum() else np.zeros(0, np.int64)
    c, cg = b["coords"][row].astype(np.float64), b["grad"][row].astype(np.float64)
    o = b["rays"][:n_kept, :3].astype(np.float64)
    d = b["rays"][:n_kept, 3:].astype(np.float64)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    gp = cg[:, :3] / diag
    t = np.linalg.norm(lo + c[:, :3] * diag - o[ray], axis=1)
    gpt, gdd = gp * t[:, None], cg[:, 4:7] * 0.5
    img = image_of(b["kept"][:n_kept], n_total, n_images)[ray]
    out = {k: np.zeros((n_images, 3)) for k in ("pos", "rot", "pos_abs", "rot_abs", "pos_n", "rot_n")}
    for k in range(3):
        np.add.at(out["pos"][:, k], img, gp[:, k])
        np.add.at(out["pos_abs"][:, k], img, np.abs(gp[:, k]))
        np.add.at(out["pos_n"][:, k], img, 1)
        a, bb = (k + 1) % 3, (k + 2) % 3
        da, db = d[ray, a], d[ray, bb]
        np.add.at(out["rot"][:, k], img, da * (gpt[:, bb] + gdd[:, bb]) - db * (gpt[:, a] + gdd[:, a]))
        np.add.at(out["rot_abs"][:, k], img, np.abs(da) * (np.abs(gpt[:, bb]) + np.abs(gdd[:, bb])) +
                  np.abs(db) * (np.abs(gpt[:, a]) + np.abs(gdd[:, a])))
        np.add.at(out["rot_n"][:, k], img, 4)
    return out


def upload(pkg, b, counter=None, stride=7):
    dev = "cuda"
    grad = b["grad"]
    if stride != 7:
        grad = np.concatenate([grad, np.full((grad.shape[0], stride - 7), 1e30, np.float32)], 1)
    samples = {"counters": torch.tensor([b["counters"][0] if counter is None else counter, b["counters"][1]], dtype=torch.int32, device=dev),
               "ray_indices": torch.from_numpy(b["kept"].view(np.int32)).to(dev),
               "rays": torch.from_numpy(b["rays"]).to(dev),
               "numsteps": torch.from_numpy(b["numsteps"].view(np.int32)).to(dev)}
    return samples, torch.from_numpy(b["coords"]).to(dev), torch.from_numpy(np.ascontiguousarray(grad)).to(dev)


def box_cfg(pkg, box=BOX):
    return pkg.nerf.default_config(1.0, aabb_min=box[0], aabb_max=box[1])


def check_against(ref, pos, rot, label):
    for name, got in (("pos", pos), ("rot", rot)):
        d = np.abs(got.astype(np.float64) - ref[name])
        bound = (ref[name + "_n"] + 16) * U * ref[name + "_abs"]
        print(f"{label} {name}: max |delta| {d.max():.3e}, max delta / bound {np.max(d / np.maximum(bound, 1e-300)):.3f}")
        assert (d <= bound).all(), (name, d, bound)


@pytest.mark.parametrize("stride", [7, 8])
def test_hand_built_batch_matches_float64(pkg, stride):
    b = hand_batch()
    img = image_of(b["kept"], N_TOTAL, N_IMAGES)
    assert (img == EMPTY_IMAGE).sum() == 0 and (img == SINGLE_IMAGE).sum() == 1
    assert set(np.unique(b["numsteps"][:, 0])) == {0, 1, 2, 63, 64, 65, 200}
    samples, coords, grad = upload(pkg, b, stride=stride)
    pos = torch.zeros((N_IMAGES, 3), device="cuda")
    rot = torch.zeros((N_IMAGES, 3), device="cuda")
    pkg.nerf.camera_gradients(box_cfg(pkg), N_TOTAL, N_IMAGES, samples, coords, grad, pos, rot)
    ref = restate(b, N_KEPT)
    check_against(ref, pos.cpu().numpy(), rot.cpu().numpy(), f"stride {stride}")
    assert not pos[EMPTY_IMAGE].any() and not rot[EMPTY_IMAGE].any()
    assert pos[SINGLE_IMAGE].any() and rot[SINGLE_IMAGE].any()


def test_reproducible_and_accumulating(pkg):
    b = hand_batch(seed=1)
    samples, coords, grad = upload(pkg, b)
    cfg = box_cfg(pkg)
    outs = []
    for _ in range(2):
        pos = torch.zeros((N_IMAGES, 3), device="cuda")
        rot = torch.zeros((N_IMAGES, 3), device="cuda")
        pkg.nerf.camera_gradients(cfg, N_TOTAL, N_IMAGES, samples, coords, grad, pos, rot)
        outs.append((pos.cpu().numpy().tobytes(), rot.cpu().numpy().tobytes()))
    assert outs[0] == outs[1]
    once = (pos.cpu().numpy().copy(), rot.cpu().numpy().copy())
    pkg.nerf.camera_gradients(cfg, N_TOTAL, N_IMAGES, samples, coords, grad, pos, rot)  # onto the first call's sums
    np.testing.assert_array_equal(pos.cpu().numpy(), 2 * once[0])
    np.testing.assert_array_equal(rot.cpu().numpy(), 2 * once[1])


def test_edge_sizes(pkg):
    b = hand_batch(seed=2)
    cfg = box_cfg(pkg)
    # ray counter 0: the outputs are not touched
    samples, coords, grad = upload(pkg, b, counter=0)
    pos = torch.full((N_IMAGES, 3), 7.5, device="cuda")
    rot = torch.full((N_IMAGES, 3), -2.25, device="cuda")
    pkg.nerf.camera_gradients(cfg, N_TOTAL, N_IMAGES, samples, coords, grad, pos, rot)
    assert (pos == 7.5).all() and (rot == -2.25).all()
    # a ray counter smaller than the buffers: only the first 1000 kept rays count
    samples, coords, grad = upload(pkg, b, counter=1000)
    pos = torch.zeros((N_IMAGES, 3), device="cuda")
    rot = torch.zeros((N_IMAGES, 3), device="cuda")
    pkg.nerf.camera_gradients(cfg, N_TOTAL, N_IMAGES, samples, coords, grad, pos, rot)
    check_against(restate(b, 1000), pos.cpu().numpy(), rot.cpu().numpy(), "counter 1000")
    # one ray of one sample, one image
    one = {"kept": np.array([0], np.uint32), "numsteps": np.array([[1, 0]], np.uint32), "rays": b["rays"][:1],
           "coords": b["coords"][:1], "grad": b["grad"][:1], "counters": np.array([1, 1], np.uint32)}
    samples, coords, grad = upload(pkg, one)
    pos = torch.zeros((1, 3), device="cuda")
    rot = torch.zeros((1, 3), device="cuda")
    pkg.nerf.camera_gradients(cfg, 1, 1, samples, coords, grad, pos, rot)
    check_against(restate(one, 1, n_total=1, n_images=1), pos.cpu().numpy(), rot.cpu().numpy(), "one ray")
    assert pos.any() and rot.any()


def test_input_gradient_precedes_the_fused_update(pkg):
    """The training step's dL/dinput is taken with respect to the weights the forward used, although the grid's
    optimizer update is fused into the grid backward that runs in the same step."""
    cfg = pkg.nerf_config("C2")
    net = pkg.create_nerf_network(cfg)
    tr = pkg.Trainer(net, cfg["optimizer"], seed=11)
    n = next((k for k in range(256, 1 << 17, 256) if tr.fused_update_active(k)), None)
    assert n is not None and tr.fused_update_active(n) and not tr.fused_update_active(n - 256)
    g = np.random.default_rng(5)
    x = np.zeros((n, 7), np.float32)
    x[:, :3] = g.random((n, 3))
    x[:, 3] = 0.01
    d = g.standard_normal((n, 3))
    x[:, 4:] = (d / np.linalg.norm(d, axis=1, keepdims=True) + 1) / 2
    dL = np.zeros((n, 16), np.float16)
    dL[:, :4] = g.uniform(-1, 1, (n, 4))
    xt, dLt = torch.from_numpy(x).cuda(), torch.from_numpy(dL).cuda()
    saved = tr.params.clone()
    in_step = torch.zeros((n, 7), device="cuda")
    tr.train_step(xt, dLt, dL_dinput=in_step)
    torch.cuda.synchronize()
    layout = net.layout()
    grid = slice(int(layout.grid_offset), int(layout.grid_offset + layout.grid_params))
    assert not torch.equal(tr.params[grid], saved[grid])  # the fused update did change the table
    net2 = pkg.create_nerf_network(cfg)
    tr2 = pkg.Trainer(net2, cfg["optimizer"], seed=11)
    tr2.params.copy_(saved)
    ctx, _ = net2.forward(xt)
    plain = torch.zeros((n, 7), device="cuda")
    net2.backward(ctx, dLt, dL_dinput=plain)
    torch.cuda.synchronize()
    assert plain[:, :3].any() and plain[:, 4:].any()
    np.testing.assert_array_equal(in_step.cpu().numpy(), plain.cpu().numpy())


def ragged_scene(pkg):
    """The 6-image ragged scene of test_gpu_nerf.py's shape."""
    S = pkg.synthetic
    ims, pix = [], []
    for i, c2w in enumerate(S.camera_poses(6, seed=1)):
        w, h = 96 + 8 * i, 80 + 4 * i
        ims.append(pkg.nerf.make_image(w, h, pkg.nerf.nerf_matrix_to_ngp(c2w), camera_angle_x=S.LEGO_CAMERA_ANGLE_X))
        px = S.render(c2w, w, h)
        px[3:5, 7:40] = np.array([255, 0, 255, 0], np.uint8)
        pix.append(px)
    return pkg.nerf.NerfDataset(ims, pix), ims


def new_run(pkg, ds, seed=7):
    net = pkg.create_nerf_network(pkg.nerf_config("C2"))
    tr = pkg.Trainer(net, pkg.nerf_config("C2")["optimizer"], seed=seed)
    return net, tr, pkg.nerf.NerfTraining(net, tr, ds, pkg.nerf.default_config(1.0), seed=1337)


def test_feature_off_trains_bit_for_bit(pkg):
    ds, ims = ragged_scene(pkg)
    outs = []
    for touch in (False, True):
        net, tr, run = new_run(pkg, ds)
        if touch:
            run.set_camera_training(optimize_extrinsics=0)
        assert run.camera_training() == {"optimize_extrinsics": 0, "n_steps_between_cam_updates": 16,
                                         "extrinsic_l2_reg": pytest.approx(1e-4), "extrinsic_learning_rate": pytest.approx(1e-3)}
        stats = [run.train_step(get_loss=False) for _ in range(40)]
        torch.cuda.synchronize()
        for i, im in enumerate(ims):
            assert run.camera_extrinsics(i).tobytes() == np.array(im.xform[:], np.float32).tobytes()
        outs.append((stats, tr.params.cpu().numpy().view(np.uint16), run.density_grid.cpu().numpy()))
    assert outs[0][0] == outs[1][0]
    np.testing.assert_array_equal(outs[0][1], outs[1][1])
    np.testing.assert_array_equal(outs[0][2], outs[1][2])


N_SMALL, W_SMALL = 8, 64


def small_scene(pkg, displace=None):
    """8 images of 64 x 64 of the procedural scene; displace: [8 x 3] added to the NGP-space origins."""
    S = pkg.synthetic
    ims, pix, truth = [], [], []
    for i, c2w in enumerate(S.camera_poses(N_SMALL, seed=3)):
        x = pkg.nerf.nerf_matrix_to_ngp(c2w)
        truth.append(x.copy())
        if displace is not None:
            x[9:] += displace[i]
        ims.append(pkg.nerf.make_image(W_SMALL, W_SMALL, x, camera_angle_x=S.LEGO_CAMERA_ANGLE_X))
        pix.append(S.render(c2w, W_SMALL, W_SMALL))
    return pkg.nerf.NerfDataset(ims, pix), ims, pix, np.array(truth)


def test_refinement_moves_the_cameras_the_sampler_traces(pkg):
    S = pkg.synthetic
    ds, ims, pix, _ = small_scene(pkg)
    net, tr, run = new_run(pkg, ds)
    run.set_pipeline(False)  # last_samples then holds the step's rays until the next step
    run.set_camera_training(optimize_extrinsics=1, n_steps_between_cam_updates=4)
    first = [run.camera_extrinsics(i) for i in range(N_SMALL)]
    for i, im in enumerate(ims):
        assert first[i].tobytes() == np.array(im.xform[:], np.float32).tobytes()
    for _ in range(3):
        run.train_step(get_loss=False)
    assert all(run.camera_extrinsics(i).tobytes() == first[i].tobytes() for i in range(N_SMALL))
    assert run.pose_optimizer_state(0)[0]["iter"] == 0
    run.train_step(get_loss=False)
    ls = run.last_samples()
    kept = int(ls["counters"][0])
    with_rays = set(image_of(ls["ray_indices"][:kept].cpu().numpy().view(np.uint32), ls["n_rays"], N_SMALL).tolist())
    assert len(with_rays) >= 2
    moved = [run.camera_extrinsics(i) for i in range(N_SMALL)]
    for i in with_rays:
        assert moved[i][:9].tobytes() != first[i][:9].tobytes() and moved[i][9:].tobytes() != first[i][9:].tobytes()
        p, r = run.pose_optimizer_state(i)
        assert p["iter"] == 1 and r["iter"] == 1 and p["learning_rate"] == pytest.approx(1e-3)
    # step 5 traces the moved cameras: the public sampler over a dataset built from them gives the step's rays
    run.train_step(get_loss=False)
    ls = run.last_samples()
    ims2 = [pkg.nerf.make_image(W_SMALL, W_SMALL, moved[i], camera_angle_x=S.LEGO_CAMERA_ANGLE_X) for i in range(N_SMALL)]
    ds2 = pkg.nerf.NerfDataset(ims2, pix)
    again = pkg.nerf.generate_training_samples(ds2, run.cfg, ls["n_rays"], ls["rng"], ls["max_samples"], run.bitfield,
                                               n_rays_total=ls["n_rays"])
    kept = int(ls["counters"][0])
    assert kept > 0 and int(again["counters"][0]) == kept
    np.testing.assert_array_equal(again["ray_indices"][:kept].cpu().numpy(), ls["ray_indices"][:kept].cpu().numpy())
    np.testing.assert_array_equal(again["rays"][:kept].cpu().numpy(), ls["rays"][:kept].cpu().numpy())
    stale = pkg.nerf.generate_training_samples(ds, run.cfg, ls["n_rays"], ls["rng"], ls["max_samples"], run.bitfield,
                                               n_rays_total=ls["n_rays"])
    assert not np.array_equal(stale["rays"][:kept].cpu().numpy(), ls["rays"][:kept].cpu().numpy())
    run.reset_camera_extrinsics()
    assert all(run.camera_extrinsics(i).tobytes() == first[i].tobytes() for i in range(N_SMALL))
    assert run.pose_optimizer_state(0)[0]["iter"] == 0
    run.train_step(get_loss=False)  # and training goes on


RECOVERY_STEPS = 480  # 30 pose updates at the default 16 steps between them


def test_refinement_recovers_displaced_cameras(pkg):
    """Every camera's NGP-space origin displaced by 0.02 in its own direction; refinement at the defaults brings the
    mean distance to the true origins below 0.02, and without refinement it stays where it was.
    One measurement (one MI355X, 480 steps): 0.0200 -> 0.0156, ratio 0.78 (also in DESIGN.md §8b); no ratio is asserted."""
    g = np.random.default_rng(9)
    v = g.standard_normal((N_SMALL, 3))
    displace = (0.02 * v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)
    ds, ims, pix, truth = small_scene(pkg, displace)

    def mean_distance(run):
        o = np.array([run.camera_extrinsics(i)[9:] for i in range(N_SMALL)], np.float64)
        return float(np.linalg.norm(o - truth[:, 9:].astype(np.float64), axis=1).mean())

    results = {}
    for refine in (1, 0):
        net, tr, run = new_run(pkg, ds)
        start = mean_distance(run)
        assert start == pytest.approx(0.02, rel=1e-5)
        run.set_camera_training(optimize_extrinsics=refine)
        for _ in range(RECOVERY_STEPS):
            run.train_step(get_loss=False)
        results[refine] = (start, mean_distance(run))
    print(f"mean origin distance after {RECOVERY_STEPS} steps: refined {results[1][1]:.5f} (ratio {results[1][1] / 0.02:.3f}), "
          f"control {results[0][1]:.5f}")
    assert results[0][1] == results[0][0]
    assert results[1][1] < 0.02


def test_data_parallel_trainer_refuses_refinement(pkg):
    ds, _ = ragged_scene(pkg)
    net, tr, run = new_run(pkg, ds)
    hook_t = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_uint64, C.c_int, C.c_int, C.c_void_p)
    hook = hook_t(lambda user, buf, count, dtype, op, stream: 0)  # one rank: the sum is the buffer itself
    lib = pkg.lib()
    assert lib.ngp_nerf_trainer_set_data_parallel(run.handle, 0, 1, C.cast(hook, C.c_void_p), None) == 0
    with pytest.raises(pkg.NgpError, match="single-GPU"):
        run.set_camera_training(optimize_extrinsics=1)
    assert run.camera_training()["optimize_extrinsics"] == 0
    assert run.train_step(get_loss=False)["step"] == 1  # still trains, through the hook
    # and the other order: refinement on, then a hook
    assert lib.ngp_nerf_trainer_set_data_parallel(run.handle, 0, 1, None, None) == 0
    run.set_camera_training(optimize_extrinsics=1)
    assert lib.ngp_nerf_trainer_set_data_parallel(run.handle, 0, 1, C.cast(hook, C.c_void_p), None) != 0
    assert b"single-GPU" in lib.ngp_last_error()
    assert run.train_step(get_loss=False)["step"] == 2
