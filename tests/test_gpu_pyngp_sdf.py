"""`pyngp.Testbed` in SDF mode on the GPU: render (the sphere tracer behind Testbed::render_sdf), the ground-truth view,
the new members with the reference's names (python_api.cu:438-443, 455-505, 569-580, 666-678) and calculate_iou.
The mesh is a 320-triangle bumped icosphere written to an .obj."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pkg():
    from __graft_entry__ import load_package
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return load_package()


@pytest.fixture(scope="module")
def verts(pkg):
    return pkg.synthetic.icosphere(2, bumps=0.15, seed=1)


@pytest.fixture(scope="module")
def obj_path(verts, tmp_path_factory):
    p = tmp_path_factory.mktemp("mesh") / "icosphere.obj"
    with open(p, "w") as f:
        for v in verts:
            f.write("v %r %r %r\n" % (float(v[0]), float(v[1]), float(v[2])))
        for t in range(len(verts) // 3):
            f.write("f %d %d %d\n" % (3 * t + 1, 3 * t + 2, 3 * t + 3))
    return str(p)


CAMERA = np.asarray([[1, 0, 0, 0.5], [0, 1, 0, 0.5], [0, 0, 1, -1.0]], np.float32)  # [3 x 4]: axes and origin


@pytest.fixture(scope="module")
def testbed(pkg, obj_path):
    ngp = pkg.pyngp()
    tb = ngp.Testbed()
    tb.load_training_data(obj_path)
    assert tb.mode == ngp.TestbedMode.Sdf
    tb.reload_network_from_json({**pkg.SDF_BASE, "encoding": {**pkg.SDF_BASE["encoding"], "log2_hashmap_size": 14}})
    tb.camera_matrix = CAMERA
    tb.sdf.max_iterations = 512
    tb.snap_to_pixel_centers = True
    tb.background_color = [0.0, 0.0, 0.0, 0.0]
    return tb


def test_iou_rises_with_training_and_render_shows_the_network(pkg, testbed):
    ngp, tb = pkg.pyngp(), testbed
    fresh = tb.calculate_iou(1 << 18)
    tb.training_batch_size = 1 << 14
    for _ in range(300):
        tb.train(1 << 14)
    assert tb.training_step == 300
    after = tb.calculate_iou(1 << 18)
    print(f"IoU fresh {fresh:.4f}, after 300 steps {after:.4f}")
    assert 0.0 < fresh <= 1.0 and 0.0 < after <= 1.0
    assert after > fresh
    # accumulation: factor 1 adds the samples onto the existing counters, non-blocking returns the previous ratio
    prev = tb.calculate_iou(1 << 12, 1.0, False)
    assert prev == after
    for mode in (ngp.RenderMode.Shade, ngp.RenderMode.Normals, ngp.RenderMode.Cost):
        tb.render_mode = mode
        img = tb.render(96, 64, 1, True)
        assert img.shape == (64, 96, 4) and img.dtype == np.float32
        assert np.isfinite(img).all()
        assert set(np.unique(img[..., 3])) <= {0.0, 1.0} and (img[..., 3] == 1.0).sum() > 100
    tb.render_mode = ngp.RenderMode.Slice
    with pytest.raises(RuntimeError):
        tb.render(96, 64, 1, True)
    tb.render_mode = ngp.RenderMode.Shade


def test_ground_truth_view_equals_the_renderer(pkg, testbed, verts):
    ngp, tb = pkg.pyngp(), testbed
    tb.render_ground_truth = True
    try:
        tris, amin, amax, _ = pkg.sdf.load_mesh(verts)
        lo, hi = tb.aabb
        assert np.array_equal(np.asarray(lo, np.float32), amin) and np.array_equal(np.asarray(hi, np.float32), amax)
        mesh = pkg.sdf.SdfMesh(tris)
        cfg = pkg.sdf.default_render_config(aabb_min=amin, aabb_max=amax, snap_to_pixel_centers=1, max_iterations=512)
        cam = pkg.nerf.make_image(96, 64, np.ascontiguousarray(CAMERA.T).reshape(12), focal=(64.0, 64.0))
        r = pkg.sdf.SdfRenderer()
        for name in ("Shade", "Depth"):
            tb.render_mode = getattr(ngp.RenderMode, name)
            img = tb.render(96, 64, 1, True)
            want = r.render(ground_truth=mesh, cfg=cfg, camera=cam, mode=name).cpu().numpy()
            assert (img[..., 3] == 1.0).mean() > 0.15
            assert np.array_equal(img, want)
        tb.floor_enable = True
        cfg.floor_enable = 1
        tb.render_mode = ngp.RenderMode.Shade
        assert np.array_equal(tb.render(96, 64, 1, True), r.render(ground_truth=mesh, cfg=cfg, camera=cam, mode="Shade").cpu().numpy())
    finally:
        tb.render_ground_truth = False
        tb.floor_enable = False
        tb.render_mode = ngp.RenderMode.Shade


def test_new_properties_round_trip(pkg):
    ngp = pkg.pyngp()
    tb = ngp.Testbed(ngp.TestbedMode.Sdf)
    f32 = np.float32
    # the reference's defaults
    assert tb.render_ground_truth is False and tb.render_groundtruth is False and tb.floor_enable is False
    assert tb.sdf.analytic_normals is False
    assert f32(tb.sdf.distance_scale) == f32(0.95) and tb.sdf.zero_offset == 0.0
    assert f32(tb.sdf.fd_normals_epsilon) == f32(5e-4) and tb.sdf.shadow_sharpness == 2048.0
    np.testing.assert_allclose(tb.sun_dir, np.full(3, 1 / np.sqrt(3)), atol=1e-7)
    assert list(tb.up_dir) == [0.0, 1.0, 0.0]
    b = tb.sdf.brdf
    assert [b.metallic, b.subsurface, b.specular, b.roughness, b.sheen, b.clearcoat, b.clearcoat_gloss] == [0, 0, 1, 0.5, 0, 0, 0]
    assert [f32(v) for v in b.basecolor] == [f32(0.8)] * 3 and list(b.ambientcolor) == [0.0, 0.0, 0.0]
    # every new member round-trips
    tb.render_ground_truth = True
    assert tb.render_groundtruth is True
    tb.render_groundtruth = False
    assert tb.render_ground_truth is False
    tb.floor_enable = True
    assert tb.floor_enable is True
    tb.sun_dir = [0.0, 0.5, 1.0]
    tb.up_dir = [0.0, 0.0, 1.0]
    assert list(tb.sun_dir) == [0.0, 0.5, 1.0] and list(tb.up_dir) == [0.0, 0.0, 1.0]
    tb.sdf.analytic_normals = True
    assert tb.sdf.analytic_normals is True
    for name, v in (("zero_offset", 0.25), ("distance_scale", 0.5), ("fd_normals_epsilon", 0.125), ("shadow_sharpness", 64.0)):
        setattr(tb.sdf, name, v)
        assert getattr(tb.sdf, name) == v
    for name, v in (("metallic", 0.5), ("subsurface", 0.25), ("specular", 0.75), ("roughness", 0.125), ("sheen", 0.5),
                    ("clearcoat", 0.25), ("clearcoat_gloss", 0.5)):
        setattr(tb.sdf.brdf, name, v)
        assert getattr(tb.sdf.brdf, name) == v
    tb.sdf.brdf.basecolor = [1.0, 0.5, 0.25]
    tb.sdf.brdf.ambientcolor = [0.5, 0.25, 0.125]
    assert list(tb.sdf.brdf.basecolor) == [1.0, 0.5, 0.25] and list(tb.sdf.brdf.ambientcolor) == [0.5, 0.25, 0.125]
    m = np.arange(12, dtype=np.float32).reshape(3, 4)
    tb.camera_matrix = m
    assert np.array_equal(tb.camera_matrix, m)
    assert isinstance(ngp.BRDFParams, type)
