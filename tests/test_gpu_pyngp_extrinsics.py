"""Camera pose refinement through the pybind11 Testbed (`pyngp`): the nerf.training knobs and extrinsics methods of
the reference's scripting surface, and the per-camera optimisers in snapshots."""
import gzip
import json

import msgpack
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
N_IMAGES = 8


@pytest.fixture(scope="module")
def pkg():
    from __graft_entry__ import load_package
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return load_package()


@pytest.fixture(scope="module")
def scene(pkg, tmp_path_factory):
    from PIL import Image
    S = pkg.synthetic
    d = tmp_path_factory.mktemp("extrinsics_scene")
    poses = S.camera_poses(N_IMAGES, seed=6)
    frames = []
    for i, c2w in enumerate(poses):
        Image.fromarray(S.render(c2w, 64, 64)).save(d / f"r_{i}.png")
        frames.append({"file_path": f"./r_{i}", "transform_matrix": np.asarray(c2w, np.float64).tolist()})
    (d / "transforms.json").write_text(json.dumps({"camera_angle_x": S.LEGO_CAMERA_ANGLE_X, "frames": frames}))
    return str(d), [np.asarray(p, np.float64)[:3, :4] for p in poses]


def make_testbed(pkg, scene_dir):
    ngp = pkg.pyngp()
    tb = ngp.Testbed()
    tb.load_training_data(scene_dir)
    return tb


def extrinsics(tb):
    return [tb.nerf.training.get_camera_extrinsics(i) for i in range(N_IMAGES)]


def test_defaults_are_the_reference_values(pkg, scene):
    tr = make_testbed(pkg, scene[0]).nerf.training
    assert tr.optimize_extrinsics is False
    assert tr.n_steps_between_cam_updates == 16
    assert tr.extrinsic_l2_reg == pytest.approx(1e-4, rel=1e-6)
    assert tr.extrinsic_learning_rate == pytest.approx(1e-3, rel=1e-6)


def test_extrinsics_round_trip(pkg, scene):
    scene_dir, poses = scene
    tb = make_testbed(pkg, scene_dir)
    tr = tb.nerf.training
    for i, p in enumerate(poses):  # the dataset's poses come back through the inverse of nerf_matrix_to_ngp
        got = tr.get_camera_extrinsics(i)
        assert got.shape == (3, 4) and got.dtype == np.float32
        np.testing.assert_allclose(got, p, atol=4e-6)
    new = poses[2].copy()
    new[:, 3] += [0.05, -0.1, 0.2]
    tr.set_camera_extrinsics(2, new)  # convert_to_ngp defaults to True
    np.testing.assert_allclose(tr.get_camera_extrinsics(2), new, atol=4e-6)
    np.testing.assert_allclose(tr.get_camera_extrinsics(3), poses[3], atol=4e-6)
    # the same pose given in NGP space: what the package's nerf_matrix_to_ngp makes of it, as a [3 x 4]
    d = pkg.nerf_data.load_nerf(scene_dir)
    ngp_m = pkg.nerf.nerf_matrix_to_ngp(new.astype(np.float32), d.scale, d.offset).reshape(4, 3).T
    tr.set_camera_extrinsics(4, ngp_m, convert_to_ngp=False)
    np.testing.assert_allclose(tr.get_camera_extrinsics(4), new, atol=4e-6)
    tb.set_camera_to_training_view(4)  # the view follows the trainer's transform
    np.testing.assert_array_equal(tb.camera_matrix, ngp_m.astype(np.float32))
    np.testing.assert_array_equal(tr.get_camera_extrinsics(N_IMAGES), np.eye(3, 4, dtype=np.float32))  # out of range


def test_snapshot_keeps_the_refined_poses(pkg, scene, tmp_path):
    scene_dir, _ = scene
    tb = make_testbed(pkg, scene_dir)
    initial = extrinsics(tb)
    tb.nerf.training.optimize_extrinsics = True
    tb.nerf.training.n_steps_between_cam_updates = 4
    for _ in range(8):
        tb.train(1 << 18)
    refined = extrinsics(tb)
    assert any(not np.array_equal(a, b) for a, b in zip(refined, initial))
    states = [tb.nerf.training.camera_optimizer_state(i) for i in range(N_IMAGES)]
    assert all(p["iter"] == 2 and r["iter"] == 2 for p, r in states)
    path = tmp_path / "refined.ingp"
    tb.save_snapshot(str(path), False)
    raw = msgpack.unpackb(gzip.decompress(path.read_bytes()), raw=False)
    for name in ("cam_pos_offset", "cam_rot_offset"):
        members = raw["snapshot"]["nerf"][name]
        assert len(members) == N_IMAGES
        assert set(members[0]) == {"iter", "first_moment", "second_moment", "variable", "learning_rate", "epsilon", "beta1", "beta2"}
        assert members[0]["iter"] == 2 and len(members[0]["variable"]) == 3

    tb2 = make_testbed(pkg, scene_dir)
    tb2.load_snapshot(str(path))
    for a, b in zip(extrinsics(tb2), refined):
        np.testing.assert_array_equal(a, b)
    for i in range(N_IMAGES):
        p, r = tb2.nerf.training.camera_optimizer_state(i)
        assert p["iter"] == 2 and r["iter"] == 2
        assert p["variable"] == states[i][0]["variable"] and r["variable"] == states[i][1]["variable"]
        assert p["first_moment"] == states[i][0]["first_moment"] and r["second_moment"] == states[i][1]["second_moment"]

    # a snapshot without the members (one written before pose refinement existed): the dataset's poses
    del raw["snapshot"]["nerf"]["cam_pos_offset"], raw["snapshot"]["nerf"]["cam_rot_offset"]
    old = tmp_path / "old.ingp"
    old.write_bytes(gzip.compress(msgpack.packb(raw, use_bin_type=True)))
    tb3 = make_testbed(pkg, scene_dir)
    tb3.load_snapshot(str(old))
    for a, b in zip(extrinsics(tb3), initial):
        np.testing.assert_array_equal(a, b)
    assert tb3.nerf.training.camera_optimizer_state(0)[0]["iter"] == 0
