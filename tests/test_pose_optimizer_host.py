"""CPU tests of the camera pose refinement's host side: the per-camera Adam optimisers (ngp_pose_optimizer), the
transform update (ngp_pose_apply) and the argument check of ngp_nerf_camera_gradients. No GPU calls.

The float64 restatements below are written from the update rule (Adam with beta1 0.9, beta2 0.99, epsilon 1e-8,
bias-corrected step; rotation variable <- rotvec(rotmat(-step) rotmat(variable)); gradients scaled by
n_images / 128 / n_steps_between plus l2_reg * variable; learning rate max(extrinsic_lr 0.33^(iter // 128),
network_lr / 1000)). The hyperparameters are fp32 values, so the restatement widens those exact values."""
import ctypes as C

import numpy as np
import pytest

F = np.float32
U = 2.0 ** -24  # fp32 unit roundoff


@pytest.fixture(scope="module")
def pkg():
    from __graft_entry__ import load_package
    return load_package()


# ---- float64 restatement ------------------------------------------------------------------------
def rodrigues(v):
    v = np.asarray(v, np.float64)
    a = np.linalg.norm(v)
    if a == 0:
        return np.eye(3)
    k = v / a
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(a) * K + (1 - np.cos(a)) * (K @ K)


def rotvec64(R):
    """Rotation vector of a proper rotation (angle below pi), from the skew part and the trace."""
    s = 0.5 * np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    sn = np.linalg.norm(s)
    if sn == 0:
        return np.zeros(3)
    return s / sn * np.arctan2(sn, 0.5 * (np.trace(R) - 1.0))


class RefAdam:
    def __init__(self):
        self.iter = 0
        self.m1, self.m2, self.var = np.zeros(3), np.zeros(3), np.zeros(3)
        self.lr = float(F(1e-4))
        self.b1, self.b2, self.eps = float(F(0.9)), float(F(0.99)), float(F(1e-8))

    def increment(self, g):
        self.iter += 1
        lr = self.lr * np.sqrt(1.0 - self.b2 ** self.iter) / (1.0 - self.b1 ** self.iter)
        self.m1 = self.b1 * self.m1 + (1.0 - self.b1) * g
        self.m2 = self.b2 * self.m2 + (1.0 - self.b2) * g * g
        return lr * self.m1 / (np.sqrt(self.m2) + self.eps)


def ref_lr(extrinsic_lr, it, network_lr):
    return max(float(F(extrinsic_lr)) * float(F(0.33)) ** (it // 128), float(F(network_lr)) / 1000.0)


def test_twenty_steps_match_float64_restatement(pkg):
    n_img, steps, between = 3, 20, 16
    ext_lr, l2, net_lr = 1e-3, 1e-4, 1e-2
    g = np.random.default_rng(7)
    opt = pkg.nerf.PoseOptimizer(n_img)
    pos = [RefAdam() for _ in range(n_img)]
    rot = [RefAdam() for _ in range(n_img)]
    inc_sum = np.zeros((n_img, 3))
    scale = n_img / 128.0 / between
    for _ in range(steps):
        pg = (g.standard_normal((n_img, 3)) * 50).astype(F)
        rg = (g.standard_normal((n_img, 3)) * 50).astype(F)
        opt.step(pg, rg, between, ext_lr, l2, net_lr)
        for i in range(n_img):
            p, r = pos[i], rot[i]
            p.lr = ref_lr(ext_lr, p.iter, net_lr)
            r.lr = ref_lr(ext_lr, r.iter, net_lr)
            inc = p.increment(pg[i].astype(np.float64) * scale + p.var * float(F(l2)))
            p.var = p.var - inc
            inc_sum[i] += np.abs(inc)
            rinc = r.increment(rg[i].astype(np.float64) * scale + r.var * float(F(l2)))
            r.var = rotvec64(rodrigues(-rinc) @ rodrigues(r.var))
    for i in range(n_img):
        gp, gr = opt.get(i)
        assert gp["iter"] == steps and gr["iter"] == steps
        dp = np.abs(gp["variable"].astype(np.float64) - pos[i].var)
        print(f"camera {i}: position |delta| {dp} bound {64 * U * inc_sum[i]}")
        assert (dp <= 64 * U * inc_sum[i]).all()
        dr = np.abs(gr["variable"].astype(np.float64) - rot[i].var)
        print(f"camera {i}: rotation |delta| {dr} bound {steps * 16 * U}")
        assert (dr <= steps * 16 * U).all()
        assert np.abs(rot[i].var).max() > 1e-3  # the rotations did move


@pytest.mark.parametrize("it", [0, 127, 128, 256])
def test_learning_rate_schedule(pkg, it):
    opt = pkg.nerf.PoseOptimizer(1)
    p, r = opt.get(0)
    p["iter"] = r["iter"] = it
    opt.set_state(0, p, r)
    opt.step(np.ones((1, 3), F), np.ones((1, 3), F), 16, 1e-3, 1e-4, 1e-2)
    p, r = opt.get(0)
    want = F(1e-3) * F(0.33) ** (it // 128)
    assert p["iter"] == it + 1 and r["iter"] == it + 1
    assert p["learning_rate"] == pytest.approx(float(want), rel=4 * U)
    assert r["learning_rate"] == pytest.approx(float(want), rel=4 * U)


def test_learning_rate_floor(pkg):
    opt = pkg.nerf.PoseOptimizer(1)
    p, r = opt.get(0)
    p["iter"] = r["iter"] = 128 * 12  # 1e-3 * 0.33^12 = 1.7e-9, below 1e-2 / 1000
    opt.set_state(0, p, r)
    opt.step(np.ones((1, 3), F), np.ones((1, 3), F), 16, 1e-3, 1e-4, 1e-2)
    p, r = opt.get(0)
    assert p["learning_rate"] == pytest.approx(float(F(1e-2)) / 1000.0, rel=4 * U)
    assert r["learning_rate"] == pytest.approx(float(F(1e-2)) / 1000.0, rel=4 * U)


def some_rotation():
    return rodrigues([0.3, -0.9, 0.5]).astype(F)


def xform_of(R, t):
    return np.concatenate([np.asarray(R, F).T.reshape(9), np.asarray(t, F)])  # column-major mat4x3


def test_pose_apply_zero_offsets_is_identity_bit_for_bit(pkg):
    x = xform_of(some_rotation(), [0.25, -0.0, 1.5])
    assert pkg.nerf.pose_apply(x, [0, 0, 0], [0, 0, 0]).tobytes() == x.tobytes()
    x = xform_of(rodrigues([0, 0, 0.7]).astype(F), [0.25, -0.0, 1.5])
    assert x[2] == 0 and x[5] == 0
    x[2] = x[5] = F(-0.0)  # signed zeros survive too (a product with the identity would make them +0)
    assert pkg.nerf.pose_apply(x, [0, 0, 0], [0, 0, 0]).tobytes() == x.tobytes()


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_pose_apply_small_rotation_matches_rodrigues(pkg, axis):
    R = some_rotation()
    t = np.array([0.5, 0.25, -1.0], F)
    off = np.zeros(3, F)
    off[axis] = 0.01
    dpos = np.array([0.125, -0.5, 0.0625], F)
    out = pkg.nerf.pose_apply(xform_of(R, t), off, dpos)
    want_R = rodrigues(off.astype(np.float64)) @ R.astype(np.float64)
    got_R = out[:9].reshape(3, 3).T.astype(np.float64)
    assert np.abs(got_R - want_R).max() <= 8 * U
    assert np.abs(out[9:].astype(np.float64) - (t.astype(np.float64) + dpos)).max() <= 8 * U


def test_pose_apply_normalises_a_scaled_rotation(pkg):
    R = some_rotation().astype(np.float64) * 1.05 ** (1.0 / 3.0)
    assert np.linalg.det(R) == pytest.approx(1.05, abs=1e-6)
    out = pkg.nerf.pose_apply(xform_of(R, [0, 0, 0]), [0, 0, 0], [0, 0, 0])
    assert abs(np.linalg.det(out[:9].reshape(3, 3).T.astype(np.float64)) - 1.0) <= 1e-5
    # within the 0.01 tolerance the matrix is kept as it is
    R = some_rotation().astype(np.float64) * 1.005 ** (1.0 / 3.0)
    x = xform_of(R, [0, 0, 0])
    assert pkg.nerf.pose_apply(x, [0, 0, 0], [0, 0, 0]).tobytes() == x.tobytes()


def test_tiny_rotations_compose_without_loss(pkg):
    """1e-5 rad composed 100 times is 1e-3 rad to 1 %. With the angle taken as 2 acos(w) the quaternion's w rounds
    to 1 and the rotation vanishes."""
    d = np.array([1e-5, 0, 0], F)
    v = np.zeros(3, F)
    for _ in range(100):
        v = pkg.nerf.pose_compose_rotation(d, v)
    assert abs(float(v[0]) - 1e-3) <= 1e-5
    assert abs(float(v[1])) <= 1e-8 and abs(float(v[2])) <= 1e-8


def test_set_state_get_round_trip(pkg):
    opt = pkg.nerf.PoseOptimizer(2)
    p = {"iter": 37, "first_moment": F([1, 2, 3]), "second_moment": F([4, 5, 6]), "variable": F([0.1, -0.2, 0.3]),
         "learning_rate": 2.5e-4, "epsilon": 1e-7, "beta1": 0.8, "beta2": 0.95}
    r = dict(p, iter=5, variable=F([0.01, 0.02, -0.03]))
    opt.set_state(1, p, r)
    gp, gr = opt.get(1)
    for want, got in ((p, gp), (r, gr)):
        assert got["iter"] == want["iter"]
        for k in ("first_moment", "second_moment", "variable"):
            assert got[k].tobytes() == np.asarray(want[k], F).tobytes()
        for k in ("learning_rate", "epsilon", "beta1", "beta2"):
            assert got[k] == float(F(want[k]))
    gp0, gr0 = opt.get(0)  # the other camera is untouched: the defaults
    assert gp0["iter"] == 0 and not gp0["variable"].any()
    assert (gp0["learning_rate"], gp0["epsilon"], gp0["beta1"], gp0["beta2"]) == tuple(float(F(v)) for v in (1e-4, 1e-8, 0.9, 0.99))


def test_reset_one_clears_only_that_camera(pkg):
    opt = pkg.nerf.PoseOptimizer(3)
    for _ in range(3):
        opt.step(np.ones((3, 3), F), -np.ones((3, 3), F))
    before = [opt.get(i) for i in range(3)]
    assert all(p["variable"].any() and r["variable"].any() for p, r in before)
    opt.reset_one(1)
    for i in (0, 2):
        p, r = opt.get(i)
        assert p["iter"] == 3 and p["variable"].tobytes() == before[i][0]["variable"].tobytes()
        assert r["variable"].tobytes() == before[i][1]["variable"].tobytes()
    p, r = opt.get(1)
    for s in (p, r):
        assert s["iter"] == 0 and not s["variable"].any() and not s["first_moment"].any() and not s["second_moment"].any()
    opt.reset()
    assert all(opt.get(i)[0]["iter"] == 0 and not opt.get(i)[1]["variable"].any() for i in range(3))


def test_camera_gradients_null_pointer_is_invalid(pkg):
    lib = pkg.lib()
    cfg = pkg.nerf.default_config(1.0)
    one = C.c_void_p(16)  # never dereferenced: the null check comes first
    rc = lib.ngp_nerf_camera_gradients(C.byref(cfg), None, 16, 2, one, one, one, one, one, None, 7, one, one)
    assert rc == -2 and b"invalid argument" in lib.ngp_last_error()
    rc = lib.ngp_nerf_camera_gradients(None, None, 16, 2, one, one, one, one, one, one, 7, one, one)
    assert rc == -2
    rc = lib.ngp_nerf_camera_gradients(C.byref(cfg), None, 16, 0, one, one, one, one, one, one, 7, one, one)
    assert rc == -2
    assert lib.ngp_pose_apply(None, None, None, None) == -2
    assert lib.ngp_pose_optimizer_create(0, None) == -2
