"""CPU tests of the environment map's host side: the lookup compiled for the host (csrc/envmap.h through
ngp_envmap_lookup_host) against a float64 numpy restatement of read_envmap (envmap.cuh:29-55), and the loader's
`"envmap"` key (nerf_loader.cu:516-528). No GPU call is made."""
import json

import numpy as np
import pytest

RESOLUTIONS = [(8, 4), (5, 3)]


@pytest.fixture(scope="module")
def pkg():
    from __graft_entry__ import load_package
    return load_package()


def reference_lookup(width, height, dirs):
    """read_envmap's coordinates in float64 (envmap.cuh:30-35, random_val.cuh:62-72): texel (ix, iy) and the
    fractions (wx, wy) of float32 directions."""
    d = np.asarray(dirs, np.float32).astype(np.float64)
    theta = np.arccos(np.clip(d[:, 1], -1.0, 1.0))          # dir_to_spherical({d.z, -d.x, d.y}).x
    phi = np.arctan2(-d[:, 0], d[:, 2])                      # .y
    fx = (phi / (2.0 * np.pi) + 0.5) * (width - 1)
    fy = theta / np.pi * (height - 1)
    ix, iy = np.trunc(fx).astype(np.int64), np.trunc(fy).astype(np.int64)
    return ix, iy, fx - ix, fy - iy


def reference_read(envmap, dirs):
    """read_envmap in float64: the four corners, x wrapped and y clamped per corner (envmap.cuh:37-52)."""
    h, w = envmap.shape[:2]
    ix, iy, wx, wy = reference_lookup(w, h, dirs)

    def at(x, y):
        x = np.where(x < 0, x + w, np.where(x >= w, x - w, x))
        y = np.clip(y, 0, h - 1)
        return envmap[y, x].astype(np.float64)
    wx, wy = wx[:, None], wy[:, None]
    return ((1 - wx) * (1 - wy) * at(ix, iy) + wx * (1 - wy) * at(ix + 1, iy) + (1 - wx) * wy * at(ix, iy + 1)
            + wx * wy * at(ix + 1, iy + 1))


def smooth_map(width, height):
    """A smooth RGBA map (not periodic in x: the seam is a real edge)."""
    y, x = np.mgrid[0:height, 0:width].astype(np.float64)
    m = np.stack([0.5 + 0.4 * np.sin(0.7 * x + 0.3 * y), 0.5 + 0.4 * np.cos(0.5 * x - 0.9 * y), 0.1 * x + 0.2 * y,
                  0.5 + 0.05 * x], axis=-1)
    return m.astype(np.float32)


def hard_directions():
    """Both poles; the seam d.z < 0 with d.x -> +-0, where x + 1 wraps to 0; the last row, where y + 1 clamps."""
    tiny = np.float32(1e-30)
    d = [(0, 1, 0), (0, -1, 0),
         (0.0, 0.0, -1.0), (-0.0, 0.0, -1.0), (tiny, 0.0, -1.0), (-tiny, 0.0, -1.0), (1e-7, 0.3, -0.95), (-1e-7, 0.3, -0.95),
         (1e-4, -0.5, -0.86), (-1e-4, -0.5, -0.86),
         (0.3, -1.0 + 1e-7, 0.0), (0.1, -0.99999, 0.1), (-0.2, -0.9999, -0.3), (0.0, -1.0, 1e-20),
         (1, 0, 0), (-1, 0, 0), (0, 0, 1)]
    d = np.asarray(d, np.float64)
    return (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)


def directions(n=4096, seed=0):
    g = np.random.default_rng(seed)
    d = g.standard_normal((n, 3))
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    return np.concatenate([hard_directions(), d])


def interpolation_bound(envmap):
    """How far the value interpolated with float32 coordinates may be from the float64 one. The bilinear interpolant is
    continuous (also across texel borders, the seam and the clamped row: a corner that changes does so with weight 0)
    and piecewise linear, so it moves by at most (largest difference of x-neighbours) per unit of fx plus the same in y.
    float32: acosf / atan2f within 4 ulp of a result of at most pi (4 * 2^-22), divided by pi or 2 pi: below
    4 * 2^-23 in the unorm coordinate; the division, the + 0.5 and the scale by the resolution round three more times,
    each at most 2^-24 of a value of at most 1: 11 * 2^-24 in all, times (resolution - 1) texels. The four weights are
    products of rounded factors (3 roundings each, 2^-24 relative): 12 * 2^-24 of the largest texel magnitude."""
    h, w = envmap.shape[:2]
    e = envmap.astype(np.float64)
    lx = np.abs(np.diff(e, axis=1)).max() if w > 1 else 0.0
    ly = np.abs(np.diff(e, axis=0)).max() if h > 1 else 0.0
    eps = 11 * 2.0 ** -24
    return lx * (w - 1) * eps + ly * (h - 1) * eps + 12 * 2.0 ** -24 * np.abs(e).max()


def check_lookup(width, height, dirs, texels, weights):
    """Shared by the host and the device test: structure of the four corners, weights, interpolated value."""
    texels, weights = np.asarray(texels, np.int64), np.asarray(weights, np.float64)
    n_tex = width * height
    assert texels.min() >= 0 and texels.max() < n_tex
    x, y = texels[:, 0] % width, texels[:, 0] // width
    # (x + 1, y) wraps, (x, y + 1) clamps, per corner
    np.testing.assert_array_equal(texels[:, 1], (x + 1) % width + y * width)
    np.testing.assert_array_equal(texels[:, 2], x + np.minimum(y + 1, height - 1) * width)
    np.testing.assert_array_equal(texels[:, 3], (x + 1) % width + np.minimum(y + 1, height - 1) * width)
    assert (weights >= 0).all() and (weights <= 1).all()
    # (1-wx)(1-wy) + wx(1-wy) + (1-wx)wy + wx wy = 1 up to the factors' and the products' roundings
    assert np.abs(weights.sum(axis=1) - 1.0).max() <= 4 * 2.0 ** -23
    # the texel agrees with the float64 one wherever the coordinate is not within the bound of a texel border
    ix, iy, wx, wy = reference_lookup(width, height, dirs)
    eps = 11 * 2.0 ** -24
    clear_x = (np.minimum(wx, 1 - wx) > eps * max(width - 1, 1))
    clear_y = (np.minimum(wy, 1 - wy) > eps * max(height - 1, 1))
    np.testing.assert_array_equal(x[clear_x], ix[clear_x])
    np.testing.assert_array_equal(y[clear_y], iy[clear_y])
    envmap = smooth_map(width, height)
    got = (weights[:, :, None] * envmap.reshape(-1, 4).astype(np.float64)[texels]).sum(axis=1)
    ref = reference_read(envmap, dirs)
    err, bound = np.abs(got - ref).max(), interpolation_bound(envmap)
    print(f"envmap lookup {width}x{height}: max |interpolated - float64| = {err:.3e}, bound {bound:.3e}")
    assert err <= bound


@pytest.mark.parametrize("width,height", RESOLUTIONS)
def test_host_lookup_matches_the_float64_restatement(pkg, width, height):
    d = directions()
    tex, wt = pkg.nerf.envmap_lookup(width, height, d, host=True)
    check_lookup(width, height, d, tex, wt)


def test_host_lookup_hard_directions(pkg):
    """The poles read row 0 / the last row with wy = 0; d.z < 0 with d.x = +-0 reads the last / first column."""
    w, h = 8, 4
    d = hard_directions()
    tex, wt = pkg.nerf.envmap_lookup(w, h, d, host=True)
    assert tex[0, 0] // w == 0 and tex[1, 0] // w == h - 1 and tex[1, 2] // w == h - 1   # (0, +-1, 0); y + 1 clamps
    assert wt[1, 2] + wt[1, 3] == 0.0                                                     # wy = 0 in the last row
    # d = (+0, 0, -1): atan2(-0, -1) = -pi, the first column; d = (-0, 0, -1): atan2(+0, -1) = +pi, the last column, wx = 0,
    # and its x + 1 neighbour is column 0
    assert tex[2, 0] % w == 0 and tex[3, 0] % w == w - 1 and tex[3, 1] % w == 0 and wt[3, 1] == 0.0


def test_lookup_rejects_bad_arguments(pkg):
    d = np.zeros((1, 3), np.float32)
    with pytest.raises(pkg.NgpError):
        pkg.nerf.envmap_lookup(0, 4, d, host=True)
    with pytest.raises(pkg.NgpError):
        pkg.nerf.envmap_lookup(8, 8193, d, host=True)


def _write_scene(pkg, tmp, envmap_key):
    from PIL import Image
    S = pkg.synthetic
    frames = []
    for i, c2w in enumerate(S.camera_poses(2, seed=1)):
        Image.fromarray(S.render(c2w, 16, 16)).save(tmp / f"r_{i}.png")
        frames.append({"file_path": f"./r_{i}", "transform_matrix": np.asarray(c2w, np.float64).tolist()})
    top = {"camera_angle_x": S.LEGO_CAMERA_ANGLE_X, "frames": frames}
    if envmap_key is not None:
        top["envmap"] = envmap_key
    (tmp / "transforms.json").write_text(json.dumps(top))
    return str(tmp)


def test_loader_reads_the_envmap_key(pkg, tmp_path):
    from PIL import Image
    g = np.random.default_rng(3)
    px = g.integers(0, 256, (3, 5, 4), dtype=np.uint8)
    Image.fromarray(px, "RGBA").save(tmp_path / "sky.png")
    d = pkg.nerf_data.load_nerf(_write_scene(pkg, tmp_path, "sky.png"))
    assert d.envmap_resolution == (5, 3) and d.envmap.shape == (3, 5, 4) and d.envmap.dtype == np.float32
    # from_rgba32 (common_device.cuh:771-798): sRGB decoded, premultiplied by alpha
    f = px.astype(np.float64) / 255.0
    lin = np.where(f[..., :3] <= 0.04045, f[..., :3] / 12.92, ((f[..., :3] + 0.055) / 1.055) ** 2.4) * f[..., 3:4]
    np.testing.assert_allclose(d.envmap[..., :3], lin, rtol=1e-6, atol=1e-7)
    np.testing.assert_allclose(d.envmap[..., 3], f[..., 3], rtol=1e-6)


def test_loader_reads_an_exr_envmap(pkg, tmp_path):
    g = np.random.default_rng(4)
    rgba = g.random((4, 8, 4)).astype(np.float32)
    pkg.exr.write_exr(str(tmp_path / "sky.exr"), rgba)
    d = pkg.nerf_data.load_nerf(_write_scene(pkg, tmp_path, "./sky.exr"))
    assert d.envmap_resolution == (8, 4)
    np.testing.assert_array_equal(d.envmap, rgba)


def test_loader_without_the_key_has_no_envmap(pkg, tmp_path):
    d = pkg.nerf_data.load_nerf(_write_scene(pkg, tmp_path, None))
    assert d.envmap is None and d.envmap_resolution == (0, 0)


def test_loader_raises_on_a_dangling_envmap(pkg, tmp_path):
    with pytest.raises(FileNotFoundError, match="Environment map"):
        pkg.nerf_data.load_nerf(_write_scene(pkg, tmp_path, "missing_sky.png"))
