"""The SDF renderer's C-ABI without a GPU: ngp_sdf_render_default_config returns the reference's defaults
(testbed.h:601-602, 798-835, 916; sdf.h:62-72; MARCH_ITER testbed_sdf.cu:37) and invalid calls are rejected with
NGP_INVALID before any HIP call."""
import ctypes as C

import numpy as np
import pytest

NGP_INVALID = -2


@pytest.fixture(scope="module")
def pkg():
    from __graft_entry__ import load_package
    return load_package()


def test_default_config_is_the_reference(pkg):
    cfg = pkg.sdf.default_render_config()
    f32 = np.float32
    assert cfg.zero_offset == 0.0
    assert f32(cfg.distance_scale) == f32(0.95)
    assert f32(cfg.maximum_distance) == f32(5e-5)
    assert f32(cfg.fd_normals_epsilon) == f32(5e-4)
    assert cfg.shadow_sharpness == 2048.0
    assert cfg.analytic_normals == 0 and cfg.floor_enable == 0
    assert cfg.max_iterations == 10000
    np.testing.assert_allclose(list(cfg.sun_dir), np.full(3, 1 / np.sqrt(3)), rtol=0, atol=1e-7)
    assert list(cfg.up_dir) == [0.0, 1.0, 0.0]
    assert [cfg.metallic, cfg.subsurface, cfg.specular, cfg.roughness, cfg.sheen, cfg.clearcoat, cfg.clearcoat_gloss] == \
        [0.0, 0.0, 1.0, 0.5, 0.0, 0.0, 0.0]
    assert [f32(v) for v in cfg.basecolor] == [f32(0.8)] * 3
    assert list(cfg.ambientcolor) == [0.0, 0.0, 0.0]
    assert list(cfg.aabb_min) == [0.0] * 3 and list(cfg.aabb_max) == [1.0] * 3
    assert pkg.lib().ngp_sdf_render_default_config(None) == NGP_INVALID


def test_overrides_reach_the_struct(pkg):
    cfg = pkg.sdf.default_render_config(max_iterations=512, floor_enable=1, aabb_min=(0.1, 0.2, 0.3), basecolor=(1, 0, 0))
    assert cfg.max_iterations == 512 and cfg.floor_enable == 1
    assert [np.float32(v) for v in cfg.aabb_min] == [np.float32(v) for v in (0.1, 0.2, 0.3)]
    assert list(cfg.basecolor) == [1.0, 0.0, 0.0]


def test_invalid_arguments_fail_without_gpu(pkg):
    lib = pkg.lib()
    assert lib.ngp_sdf_renderer_create(None) == NGP_INVALID
    r = C.c_void_p()
    assert lib.ngp_sdf_renderer_create(C.byref(r)) == 0  # a host object; no HIP call until the first render
    try:
        cfg = pkg.sdf.default_render_config()
        cam = pkg.nerf.make_image(8, 8, [1, 0, 0, 0, 1, 0, 0, 0, 1, 0.5, 0.5, -1.0], focal=(8, 8))
        fake = C.c_void_p(0x1000)  # never dereferenced: every call below is rejected first

        def render(rr=r, model=fake, gt=None, c=C.byref(cfg), camera=C.byref(cam), mode=1, spp=1, out=fake):
            return lib.ngp_sdf_render(rr, model, gt, c, None, camera, mode, spp, 0, None, 1, out, None)

        assert render(rr=None) == NGP_INVALID
        assert render(c=None) == NGP_INVALID
        assert render(camera=None) == NGP_INVALID
        assert render(out=None) == NGP_INVALID
        assert render(spp=0) == NGP_INVALID
        assert render(model=None, gt=None) == NGP_INVALID  # neither distance source
        assert render(model=fake, gt=fake) == NGP_INVALID  # both
        assert b"exactly one" in lib.ngp_last_error()
        for mode in (-1, 5, 7, 8, 9):  # Distortion, Slice, EncodingVis, ...
            assert render(mode=mode) == NGP_INVALID
            assert render(model=None, gt=fake, mode=mode) == NGP_INVALID
        assert lib.ngp_sdf_iou_accumulate(None, 4, fake, fake, 1.0, None) == NGP_INVALID
        assert lib.ngp_sdf_iou_accumulate(None, 4, None, fake, 1.0, fake) == NGP_INVALID
        assert lib.ngp_sdf_iou_accumulate(None, 4, fake, None, 1.0, fake) == NGP_INVALID
    finally:
        lib.ngp_sdf_renderer_destroy(r)
