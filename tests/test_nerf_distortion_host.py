"""CPU tests of the lens distortion map's host side: the lookup compiled for the host (csrc/distortion.h through
ngp_nerf_distortion_lookup_host) against a numpy float32 restatement of Buffer2DView::at_lerp (common.h:384-400), the
argument checks that precede any HIP call, and the network config's "distortion_map" section. No GPU call is made."""
import ctypes as C

import numpy as np
import pytest

SIZES = [(1, 1), (3, 2), (32, 32)]  # (width, height)
F = np.float32


@pytest.fixture(scope="module")
def pkg():
    from __graft_entry__ import load_package
    return load_package()


def uv_cases(width, height, n_random=1000, seed=0):
    """The issue's list: 0, k / res exactly, nextafter(1, 0), 1, 1 + 2 ulp, 2.5 (folded), -1e-3, NaN, random values."""
    one_2ulp = np.nextafter(np.nextafter(F(1), F(2)), F(2))
    special = [F(0), np.nextafter(F(1), F(0)), F(1), one_2ulp, F(2.5), F(-1e-3), F(np.nan)]
    special += [F(k) / F(width) for k in range(width + 1)] + [F(k) / F(height) for k in range(height + 1)]
    special = np.array(special, F)
    uu, vv = np.meshgrid(special, special, indexing="ij")
    rs = np.random.RandomState(seed)
    rnd = rs.uniform(-0.05, 1.05, (n_random, 2)).astype(F)
    return np.concatenate([np.stack([uu.ravel(), vv.ravel()], -1), rnd]).astype(F)


def restate_lookup(width, height, uv):
    """distortion_lookup in numpy float32, from the definition: fold into [0, 2] (NaN to 0), xy = (w, h) * uv, texel
    (int)xy, weights xy - texel, corners clamped into the map, the reference's products."""
    uv = np.asarray(uv, F)

    def fold(x):
        with np.errstate(invalid="ignore"):
            return np.where(x >= 0, np.where(x <= 2, x, F(2)), F(0)).astype(F)
    u, v = fold(uv[:, 0]), fold(uv[:, 1])
    fx, fy = (F(width) * u).astype(F), (F(height) * v).astype(F)
    ix, iy = fx.astype(np.int32), fy.astype(np.int32)  # truncation
    wx, wy = (fx - ix.astype(F)).astype(F), (fy - iy.astype(F)).astype(F)

    def tex(x, y):
        return np.clip(x, 0, width - 1).astype(np.int64) + np.clip(y, 0, height - 1).astype(np.int64) * width
    idx = np.stack([tex(ix, iy), tex(ix + 1, iy), tex(ix, iy + 1), tex(ix + 1, iy + 1)], -1)
    one = F(1)
    wt = np.stack([((one - wx) * (one - wy)), (wx * (one - wy)), ((one - wx) * wy), (wx * wy)], -1).astype(F)
    return idx, wt


def restate_mix(idx, wt, m):
    """distortion_mix per channel: the four products summed in the reference's order, every operation in float32."""
    t = m.reshape(-1, 2).astype(F)
    out = np.zeros((idx.shape[0], 2), F)
    for c in range(2):
        p = [(wt[:, k] * t[idx[:, k], c]).astype(F) for k in range(4)]
        out[:, c] = (((p[0] + p[1]).astype(F) + p[2]).astype(F) + p[3]).astype(F)
    return out


@pytest.mark.parametrize("width,height", SIZES)
def test_host_lookup_is_the_float32_restatement(pkg, width, height):
    uv = uv_cases(width, height)
    rs = np.random.RandomState(1)
    m = (rs.uniform(-0.05, 0.05, (height, width, 2))).astype(F)
    tex, wt, off = pkg.nerf.distortion_lookup(width, height, uv, map=m, host=True)
    idx_r, wt_r = restate_lookup(width, height, uv)
    assert tex.min() >= 0 and tex.max() < width * height
    np.testing.assert_array_equal(tex, idx_r)
    assert wt.view(np.uint32).tolist() == wt_r.view(np.uint32).tolist()
    assert off.view(np.uint32).tolist() == restate_mix(idx_r, wt_r, m).view(np.uint32).tolist()
    # the four weights sum to 1 within 2 ulp
    s = wt.astype(np.float64).sum(-1)
    err = np.abs(s - 1.0).max()
    print(f"distortion lookup {width}x{height}: max |sum of weights - 1| = {err:.3e} ({err / 2.0 ** -23:.2f} ulp)")
    assert err <= 2 * 2.0 ** -23
    # without a map the taps are the same
    tex2, wt2 = pkg.nerf.distortion_lookup(width, height, uv, host=True)
    np.testing.assert_array_equal(tex2, tex)
    assert wt2.tobytes() == wt.tobytes()


def test_invalid_arguments_fail_before_any_hip_call(pkg):
    lib = pkg.lib()
    uv = np.zeros((4, 2), F)
    tex, wt, off = np.zeros((4, 4), np.uint32), np.zeros((4, 4), F), np.zeros((4, 2), F)
    m = np.zeros((8, 8, 2), F)
    INVALID = -2
    p = lambda a: a.ctypes.data  # noqa: E731
    # a zero width or height, and sizes the envmap's check refuses
    for w, h in [(0, 4), (4, 0), (8193, 4), (4, 8193)]:
        assert lib.ngp_nerf_distortion_lookup_host(w, h, 4, p(uv), p(tex), p(wt), None, None) == INVALID
        assert lib.ngp_nerf_distortion_lookup(None, w, h, 4, p(uv), p(tex), p(wt), None, None) == INVALID
        assert lib.ngp_nerf_distortion_accumulator_words(w, h) == 0
        assert lib.ngp_nerf_distortion_gradient(None, w, h, p(uv), p(wt)) == INVALID
        assert lib.ngp_nerf_trainer_set_distortion_map(None, w, h, None) == INVALID
        assert lib.ngp_nerf_renderer_set_distortion_map(None, p(m), w, h) == INVALID
    # null pointers
    assert lib.ngp_nerf_distortion_lookup_host(8, 8, 4, None, p(tex), p(wt), None, None) == INVALID
    assert lib.ngp_nerf_distortion_lookup_host(8, 8, 4, p(uv), None, p(wt), None, None) == INVALID
    assert lib.ngp_nerf_distortion_lookup_host(8, 8, 4, p(uv), p(tex), None, None, None) == INVALID
    assert lib.ngp_nerf_distortion_lookup_host(8, 8, 4, p(uv), p(tex), p(wt), None, p(off)) == INVALID  # offsets need a map
    assert lib.ngp_nerf_distortion_lookup(None, 8, 8, 4, None, p(tex), p(wt), None, None) == INVALID
    assert lib.ngp_nerf_distortion_gradient(None, 8, 8, None, p(wt)) == INVALID
    assert lib.ngp_nerf_distortion_gradient(None, 8, 8, p(uv), None) == INVALID
    rng = pkg.nerf.pcg32(1)
    cfg = pkg.nerf.default_config()
    assert lib.ngp_nerf_distortion_deposit(None, C.byref(cfg), None, 16, rng, p(tex), p(tex), None, p(wt), 8, 8, p(tex)) == INVALID
    assert lib.ngp_nerf_distortion_ray_gradients(C.byref(cfg), None, 16, 2, None, None, None, None, None, None, 7, None, None,
                                                 None, None) == INVALID
    assert b"invalid argument" in lib.ngp_last_error()
    for fn in (lib.ngp_nerf_trainer_clear_distortion_map,):
        assert fn(None) == INVALID
    assert lib.ngp_nerf_trainer_set_optimize_distortion(None, 1) == INVALID
    assert lib.ngp_nerf_trainer_get_optimize_distortion(None, None) == INVALID
    assert lib.ngp_nerf_trainer_distortion_map(None, 0, None, 0, None, None) == INVALID
    assert lib.ngp_nerf_trainer_set_distortion_training(None, None, 32, 32) == INVALID
    assert lib.ngp_nerf_generate_training_samples_distortion(None, C.byref(cfg), None, 16, 0, 16, rng, 64, None, None, None, None,
                                                             None, None, None, p(m), 0, 8) == INVALID
    # a valid size has 3 channels of 16 bins per texel and the counter of dropped contributions
    assert lib.ngp_nerf_distortion_accumulator_words(32, 32) == 32 * 32 * 3 * 16 + 1
    assert lib.ngp_nerf_distortion_accumulator_words(32, 32) * 8 == 384 * 1024 + 8
    # the wrapper refuses a map of the wrong shape
    with pytest.raises(ValueError):
        pkg.nerf.distortion_lookup(8, 8, uv, map=np.zeros((4, 8, 2), F), host=True)


def test_config_distortion_map_section(pkg):
    from instant_ngp_amd import config
    base = config.nerf_config()
    sec = config.distortion_map_config(base)
    # the reference's defaults: 32 x 32, ExponentialDecay over Adam at 1e-4
    assert sec["resolution"] == [32, 32]
    assert sec["optimizer"]["otype"] == "ExponentialDecay" and sec["optimizer"]["decay_start"] == 10000
    assert sec["optimizer"]["decay_interval"] == 5000 and sec["optimizer"]["decay_base"] == 0.33
    adam = sec["optimizer"]["nested"]
    assert adam["otype"] == "Adam" and adam["learning_rate"] == 1e-4 and adam["epsilon"] == 1e-8
    assert adam["beta1"] == 0.9 and adam["beta2"] == 0.99
    # an explicit resolution or optimizer
    mine = dict(base, distortion_map={"resolution": [16, 8], "optimizer": {"otype": "Adam", "learning_rate": 3e-3}})
    sec = config.distortion_map_config(mine)
    assert sec["resolution"] == [16, 8] and sec["optimizer"] == {"otype": "Adam", "learning_rate": 3e-3}
    sec = config.distortion_map_config(dict(base, distortion_map={"resolution": [16, 8]}))
    assert sec["resolution"] == [16, 8] and sec["optimizer"] == base["optimizer"]  # falls back to the main optimizer
    # the section absent: the main optimizer, the default resolution
    bare = {k: v for k, v in base.items() if k != "distortion_map"}
    sec = config.distortion_map_config(bare)
    assert sec["resolution"] == [32, 32] and sec["optimizer"] == bare["optimizer"]
    assert sec["optimizer"] is not bare["optimizer"]  # a copy
    with pytest.raises(ValueError):
        config.distortion_map_config({"distortion_map": {"resolution": [0, 4]}, "optimizer": {"otype": "Adam"}})
    with pytest.raises(ValueError):
        config.distortion_map_config({})
