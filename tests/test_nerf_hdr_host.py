"""HDR training images (EImageDataType Half and Float; read_rgba, common_device.cuh:885-913) on the host: the float64
restatement of the loss pass's target for Half and Float texels, the seeded HDR images test_gpu_nerf_hdr.py imports, and
the CPU tests: margins, the loader's EXR frames, the C-ABI's argument checks and pyngp's surface. No GPU call is made.

restate_loss (test_nerf_loss_host.py) decodes RGBA8 texels, so the target is restated here: a Half or Float texel is
linear and premultiplied as it stands, (rgb, alpha) = the stored values, exact in float64; the target is then formed in
each of the three colour spaces as for a decoded Byte texel. While restate_loss runs, its loss_channel and
loss_channel_companion are handed this target (test_nerf_exposure_host.py's loss_sees_target), so the prediction, the
stop and compaction decisions, the sample gradients and their companions are that module's code.

The target's companion is restate_loss' own, 8 (|target| + |texel| + |(1 - alpha) background|): it allows two powf behind
the target, and an HDR target has at most one (no sRGB decode of the texel), a division and two products. So K32, which
that module measured with float32 reference arithmetic for the Byte target, bounds the HDR target too, and the GPU test
allows the same 4 K32. Nothing here comes from the kernel's output.

The images: image 0 and 2 Half, image 1 Float (a float32 draw that is not representable in fp16). Per texel alpha is 0
(then rgb is 0), 1, or uniform in (0, 1); the straight colour is log-uniform in [0.02, 12], so premultiplied rgb passes
8; about one texel in twenty has a red < 0 (the sampler's mask, which the loss pass must take as a plain value). A texel
that puts one of its rays within a decision margin under a configuration the GPU test runs is drawn again.
"""
import ctypes as ct
import functools
import json

import numpy as np
import pytest

import test_nerf_loss_host as H
from test_nerf_exposure_host import loss_sees_target
from test_nerf_loss_host import (ACT_NONE, F32, LINEAR_KNEE, MARGIN_HUBER, MARGIN_KNEE, MARGIN_SIGN, SIGN_LOSSES, batches,
                                 cfg_values, linear_to_srgb, make_cfg, srgb_to_linear)

lit = H.C
IMAGE_BYTE, IMAGE_HALF, IMAGE_FLOAT = 1, 2, 3
HDR_DTYPES = (np.float16, np.float32, np.float16)      # image 0, 1, 2
NGP_INVALID = -2
NEW_SYMBOLS = ("ngp_nerf_dataset_create_typed", "ngp_nerf_dataset_set_image", "ngp_nerf_dataset_image")


def hdr_configs(pkg):
    """The configurations the GPU test compares with float64: every loss (Exp / Exp, the default colour space), the three
    colour spaces under L2 and RelativeL2, and the ray-count test's second configuration."""
    groups, _, _, _ = batches(pkg)
    return ([(label, cfg) for label, cfg, _ in groups["losses"]] + [(label, cfg) for label, cfg, _ in groups["colour_spaces"]]
            + [("L2 None/None", make_cfg(pkg, "L2", ACT_NONE, ACT_NONE))])


def draw_texel(image, y, x, attempt, dtype):
    """One texel from (image, y, x, attempt) alone, as `dtype`: premultiplied linear RGBA."""
    g = np.random.default_rng([77, image, y, x, attempt])
    kind = g.random()
    alpha = 0.0 if kind < 0.2 else 1.0 if kind < 0.5 else g.uniform(0.02, 0.98)
    straight = np.exp(g.uniform(np.log(0.02), np.log(12.0), 3))
    t = np.concatenate([straight * alpha, [alpha]])
    if g.random() < 0.05:
        t[0] = -g.uniform(0.05, 1.0)
    return t.astype(np.float32).astype(dtype)


def ray_pixels(images, px, n):
    """Every ray's image and pixel (read_rgba's index, as restate_loss takes it)."""
    img, uv = np.asarray(px["img"]).astype(np.int64)[:n], np.asarray(px["uv"], F32)[:n]
    yx = np.zeros((n, 2), np.int64)
    for i in range(n):
        h, w = images[img[i]].shape[:2]
        yx[i] = (min(max(int(F32(uv[i, 1]) * F32(h)), 0), h - 1), min(max(int(F32(uv[i, 0]) * F32(w)), 0), w - 1))
    return img, yx


def hdr_target(pixels, px, v, background, n):
    """The target of Half / Float texels in float64: {target, target_c, knee, tex [n, 4], img, yx}."""
    img, yx = ray_pixels(pixels, px, n)
    tex4 = np.stack([pixels[img[i]][yx[i, 0], yx[i, 1]].astype(np.float64) for i in range(n)]) if n else np.zeros((0, 4))
    tex, tex_a = tex4[:, :3], tex4[:, 3:4]
    bg_srgb = np.asarray(background, np.float64)[:n] if v["random_bg_color"] else np.broadcast_to(v["background_color"], (n, 3))
    bg = srgb_to_linear(bg_srgb)
    mag = np.abs(tex) + np.abs((1.0 - tex_a) * bg)
    knee = np.full(n, np.inf)

    def to_srgb(l):
        nonlocal knee
        knee = np.minimum(knee, np.abs(l - LINEAR_KNEE).min(axis=1))
        return linear_to_srgb(l)
    if v["linear_colors"]:
        target = tex + (1.0 - tex_a) * bg
    elif v["color_space_linear"]:
        target = to_srgb(tex + (1.0 - tex_a) * bg)
    else:
        bg = to_srgb(bg)
        pos = tex_a > 0
        straight = np.where(pos, tex / np.where(pos, tex_a, 1.0), 1.0)
        target = np.where(pos, to_srgb(straight) * tex_a + (1.0 - tex_a) * bg, bg)
    return {"target": target, "target_c": 8 * (np.abs(target) + mag), "knee": knee, "tex": tex4, "img": img, "yx": yx}


def restate_loss_hdr(batch, pixels, cfg, mean_density=0.003, max_compacted=1 << 14, n_rays=None, counter=None, **kw):
    """restate_loss with the HDR images `pixels` (float16 / float32 [h, w, 4] per image) as the targets."""
    v = cfg if isinstance(cfg, dict) else cfg_values(cfg)
    n = batch.n_rays if n_rays is None else n_rays
    t = hdr_target(pixels, batch.px, v, batch.background, n)
    with loss_sees_target(t["target"], t["target_c"]):
        ref = H.restate_loss(batch.samples(n, counter), batch.out(v["density_activation"]), batch.pixels, batch.px, v, mean_density,
                             128.0, max_compacted, n, background=batch.background, **kw)
    d = ref["pred"] - t["target"]
    ref.update(target=t["target"], tex=t["tex"], img=t["img"], yx=t["yx"],
               hdr_margins={"huber": np.abs(np.abs(d) - lit(0.1)).min(axis=1), "sign": np.abs(d).min(axis=1), "srgb_knee": t["knee"]})
    return ref


def hdr_violations(batch, pixels, cfg):
    """Rays with a sample that are within a margin of Huber's knee, of the sign of pred - target or of the sRGB curve's
    knee with the HDR target, or within one of the module's own margins."""
    ref = restate_loss_hdr(batch, pixels, cfg)
    m, lt = ref["hdr_margins"], cfg_values(cfg)["loss_type"]
    bad = m["srgb_knee"] < MARGIN_KNEE
    if lt == 4:
        bad |= m["huber"] < MARGIN_HUBER
    if lt in SIGN_LOSSES:
        bad |= m["sign"] < MARGIN_SIGN
    own = ref["margins"]
    bad |= (own["t_stop"] < H.MARGIN_T) | (own["near"] < H.MARGIN_NEAR)
    return np.nonzero(bad & (ref["cn"] > 0))[0], ref


@functools.lru_cache(maxsize=None)
def _hdr_world(pkg):
    _, full, _, _ = batches(pkg)
    shapes = [p.shape[:2] for p in full.pixels]
    attempt = [np.zeros(s, np.int64) for s in shapes]
    pixels = [np.zeros(s + (4,), dt) for s, dt in zip(shapes, HDR_DTYPES)]
    for i, (h, w) in enumerate(shapes):
        for y in range(h):
            for x in range(w):
                pixels[i][y, x] = draw_texel(i, y, x, 0, HDR_DTYPES[i])
    cfgs = hdr_configs(pkg)
    redrawn = 0
    for _ in range(20):
        bad = set()
        for _, cfg in cfgs:
            rays, ref = hdr_violations(full, pixels, cfg)
            bad |= set((int(ref["img"][r]), int(ref["yx"][r, 0]), int(ref["yx"][r, 1])) for r in rays)
        if not bad:
            return full, pixels, redrawn
        for i, y, x in sorted(bad):
            attempt[i][y, x] += 1
            pixels[i][y, x] = draw_texel(i, y, x, int(attempt[i][y, x]), HDR_DTYPES[i])
            redrawn += 1
    raise AssertionError("texels within a decision margin after every redraw")


def hdr_world(pkg):
    """(the 300-ray batch, the three HDR images [float16, float32, float16], texels redrawn): built once, left unchanged."""
    return _hdr_world(pkg)


def half_images(pixels):
    """Every image rounded to fp16, and the float32 images of exactly those values."""
    with np.errstate(over="ignore"):
        h = [np.ascontiguousarray(p.astype(np.float16)) for p in pixels]
    return h, [np.ascontiguousarray(p.astype(np.float32)) for p in h]


# ---- CPU tests -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pkg():
    from __graft_entry__ import load_package
    return load_package()


def test_hdr_images_and_margins(pkg):
    """The HDR images have every kind of alpha, premultiplied rgb past 8 and some red < 0; image 1's float32 values are
    not fp16 values; under every configuration the GPU test runs no ray with a sample is within a decision margin: zero
    violations, so no ray is left out of a comparison. The target goes through the three colour-space branches and, with
    texels above 1, differs from what a clipped Byte image could give."""
    full, pixels, redrawn = hdr_world(pkg)
    assert [p.dtype for p in pixels] == [np.dtype(d) for d in HDR_DTYPES]
    for p in pixels:
        a, rgb = p[..., 3].astype(np.float64), p[..., :3].astype(np.float64)
        assert (a == 0).any() and (a == 1).any() and ((a > 0) & (a < 1)).any()
        assert not rgb[a == 0][:, 1:].any() and rgb.max() >= 8.0 and (rgb[..., 0] < 0).any() and np.isfinite(rgb).all()
    assert (pixels[1] != pixels[1].astype(np.float16).astype(np.float32)).mean() > 0.5
    branches = set()
    for label, cfg in hdr_configs(pkg):
        rays, ref = hdr_violations(full, pixels, cfg)
        assert rays.size == 0, (label, rays)
        v = cfg_values(cfg)
        branches.add((v["linear_colors"], v["color_space_linear"]))
        alive = ref["cn"] > 0
        assert alive.sum() > 250 and np.isfinite(ref["grad"]).all() and np.isfinite(ref["loss"]).all()
        assert set(np.unique(ref["img"][alive])) == {0, 1, 2}
        assert (ref["tex"][alive, :3].max(axis=1) > 1.0).sum() > 50, label
        if v["linear_colors"]:   # the linear target is the texel over the background, exactly
            bg = srgb_to_linear(np.asarray(v["background_color"]))
            np.testing.assert_array_equal(ref["target"], ref["tex"][:, :3] + (1.0 - ref["tex"][:, 3:4]) * bg)
    assert branches == {(1, 0), (0, 1), (0, 0)}
    h16, f32 = half_images(pixels)
    assert all((a.astype(np.float64) == b.astype(np.float64)).all() for a, b in zip(h16, f32))
    print(f"HDR images: {redrawn} texels drawn again; {sum(p[..., 0].size for p in pixels)} texels")


def test_restatement_sees_the_hdr_target(pkg):
    """Negative control of the hook: the loss restated with the HDR target differs from the Byte one for nearly every ray,
    and a texel scaled by 2 moves the linear target by exactly the texel."""
    full, pixels, _ = hdr_world(pkg)
    cfg = make_cfg(pkg, "L2", linear_colors=1, color_space_linear=0)
    byte, hdr = full.reference(cfg), restate_loss_hdr(full, pixels, cfg)
    alive = hdr["cnum"] > 0
    # the two agree only where both texels have alpha 0 (the target is the background): 0.25 x 0.2 of the texels
    assert (byte["loss"][alive] != hdr["loss"][alive]).mean() > 0.85
    np.testing.assert_array_equal(byte["numsteps"], hdr["numsteps"])          # the compaction does not read texels
    twice = restate_loss_hdr(full, [(p.astype(np.float32) * 2).astype(np.float32) for p in pixels], cfg)
    np.testing.assert_allclose(twice["target"] - hdr["target"], hdr["tex"][:, :3] - hdr["tex"][:, 3:4] * srgb_to_linear(
        np.asarray(cfg_values(cfg)["background_color"])), rtol=0, atol=1e-12)


# ---- the loader ----------------------------------------------------------------------------------------------------------
def _write_hdr_scene(tmp_path, **top):
    from PIL import Image
    from instant_ngp_amd.exr import write_exr
    g = np.random.default_rng(5)
    frames, exr = [], []
    for k, pixel_type in enumerate((1, 2)):                 # a HALF file and a FLOAT file
        alpha = g.choice([0.0, 1.0, 0.37, 0.5], (4, 5, 1))
        rgba = np.concatenate([g.uniform(0.0, 9.0, (4, 5, 3)), alpha], axis=-1).astype(np.float32)
        rgba[0, 0, :3] = 1.0                                # white, which white_transparent would make transparent at 8 bits
        rgba[0, 0, 3] = 1.0
        write_exr(str(tmp_path / f"h{k}.exr"), rgba, pixel_type=pixel_type)
        exr.append(rgba if pixel_type == 2 else rgba.astype(np.float16).astype(np.float32))
        frames.append({"file_path": f"h{k}.exr"})
    png = g.integers(0, 256, (4, 5, 4), dtype=np.uint8)
    png[1, 1] = (255, 255, 255, 255)
    Image.fromarray(png, "RGBA").save(tmp_path / "p2.png")
    frames.append({"file_path": "p2.png"})
    for k, fr in enumerate(frames):
        m = np.eye(4)
        m[:3, 3] = (0.1 * k, 0.2, 3.0)
        fr["transform_matrix"] = m.tolist()
    j = {"camera_angle_x": 0.7, "frames": frames}
    j.update(top)
    (tmp_path / "transforms.json").write_text(json.dumps(j))
    return str(tmp_path / "transforms.json"), exr, png


def test_loader_reads_exr_frames(pkg, tmp_path):
    """Two EXR frames (a half and a float file) and a PNG frame: types, is_hdr, bit-exact half values with and without
    fix_premult; white_transparent leaves the EXR frames alone and changes the PNG as it does today; the PNG's bytes are
    those of a scene without the EXR frames."""
    for name in ("a", "b", "c", "d"):
        (tmp_path / name).mkdir()
    path, exr, png = _write_hdr_scene(tmp_path / "a")
    data = pkg.nerf_data.load_nerf(path)
    assert len(data) == 3 and data.is_hdr and data.image_types == [IMAGE_HALF, IMAGE_HALF, IMAGE_BYTE]
    assert [p.dtype for p in data.rgba8] == [np.float16, np.float16, np.uint8]
    for got, src in zip(data.rgba8[:2], exr):
        np.testing.assert_array_equal(got.view(np.uint16), src.astype(np.float16).view(np.uint16))
    np.testing.assert_array_equal(data.rgba8[2], png)
    assert (data.images[0].width, data.images[0].height) == (5, 4)
    # fix_premult: rgb = half(float(rgb) * alpha), alpha = half(alpha)
    fixed = pkg.nerf_data.load_nerf(_write_hdr_scene(tmp_path / "b", fix_premult=True)[0])
    for got, src in zip(fixed.rgba8[:2], exr):
        want = np.concatenate([src[..., :3] * src[..., 3:4], src[..., 3:4]], axis=-1).astype(np.float32).astype(np.float16)
        np.testing.assert_array_equal(got.view(np.uint16), want.view(np.uint16))
        assert (got.view(np.uint16) != src.astype(np.float16).view(np.uint16)).any()
    np.testing.assert_array_equal(fixed.rgba8[2], png)
    # white_transparent: 8-bit frames only
    white = pkg.nerf_data.load_nerf(_write_hdr_scene(tmp_path / "c", white_transparent=True)[0])
    for got, src in zip(white.rgba8[:2], exr):
        np.testing.assert_array_equal(got.view(np.uint16), src.astype(np.float16).view(np.uint16))
    assert white.rgba8[0][0, 0, 3] == 1.0 and white.rgba8[2][1, 1, 3] == 0 and png[1, 1, 3] == 255
    # the PNG frame alone: what today's loader gives, and an 8-bit dataset is not HDR
    _, _, _ = _write_hdr_scene(tmp_path / "d")
    j = json.loads((tmp_path / "d" / "transforms.json").read_text())
    j["frames"] = j["frames"][2:]
    (tmp_path / "d" / "transforms.json").write_text(json.dumps(j))
    only = pkg.nerf_data.load_nerf(str(tmp_path / "d" / "transforms.json"))
    assert not only.is_hdr and only.image_types == [IMAGE_BYTE] and only.rgba8[0].dtype == np.uint8
    np.testing.assert_array_equal(only.rgba8[0], data.rgba8[2])


# ---- the C-ABI -----------------------------------------------------------------------------------------------------------
def test_hdr_symbols_and_constants(pkg):
    L = pkg.lib()
    for name in NEW_SYMBOLS:
        assert getattr(L, name) is not None
    assert (pkg.nerf.IMAGE_BYTE, pkg.nerf.IMAGE_HALF, pkg.nerf.IMAGE_FLOAT) == (1, 2, 3)   # EImageDataType's values


def test_hdr_arguments_are_checked_before_any_gpu_call(pkg):
    """Null pointers, no images, a type of 0 or 4 and a null dataset return NGP_INVALID (this machine has no GPU: a HIP
    call would return NGP_ERROR instead). An image index out of range and a short capacity need a dataset, which needs
    a GPU: test_gpu_nerf_hdr.py checks them."""
    from instant_ngp_amd._capi import NerfImage
    L = pkg.lib()
    im = pkg.nerf.make_image(2, 2, np.eye(4)[:3].T.reshape(12), camera_angle_x=0.7)
    arr = (NerfImage * 1)(im)
    px = np.zeros((2, 2, 4), np.float32)
    ptrs = (ct.c_void_p * 1)(px.ctypes.data)
    nulls = (ct.c_void_p * 1)(None)
    h = ct.c_void_p()

    def types(t):
        return (ct.c_uint32 * 1)(t)
    for args in ((0, arr, ptrs, types(3), ct.byref(h)), (1, None, ptrs, types(3), ct.byref(h)), (1, arr, None, types(3), ct.byref(h)),
                 (1, arr, ptrs, None, ct.byref(h)), (1, arr, ptrs, types(3), None), (1, arr, ptrs, types(0), ct.byref(h)),
                 (1, arr, ptrs, types(4), ct.byref(h)), (1, arr, nulls, types(2), ct.byref(h))):
        assert L.ngp_nerf_dataset_create_typed(*args) == NGP_INVALID and not h.value
    for t in (0, 1, 2, 3, 4):
        assert L.ngp_nerf_dataset_set_image(None, 0, px.ctypes.data, t, 2, 2) == NGP_INVALID
    t = ct.c_uint32(7)
    assert L.ngp_nerf_dataset_image(None, 0, px.ctypes.data, px.nbytes, ct.byref(t)) == NGP_INVALID and t.value == 7
    assert L.ngp_nerf_dataset_image(None, 0, None, 0, None) == NGP_INVALID
    # the Python wrapper refuses other dtypes beside an HDR image, and wrong shapes, before it calls anything
    with pytest.raises(ValueError, match="uint8, float16 or float32"):
        pkg.nerf.NerfDataset([im, im], [np.zeros((2, 2, 4), np.float16), np.zeros((2, 2, 4), np.float64)])
    with pytest.raises(ValueError, match="shape"):
        pkg.nerf.NerfDataset([im], [np.zeros((2, 3, 4), np.float16)])


def test_pyngp_hdr_surface(pkg):
    """nerf.training.set_image_pixels / image and nerf.training.dataset.is_hdr exist in the built module; without
    training data the first two raise, and set_image with colours still refuses."""
    ngp = pkg.pyngp()
    tb = ngp.Testbed()
    tr = tb.nerf.training
    assert tr.dataset.is_hdr is False
    with pytest.raises(RuntimeError, match="no NeRF training data"):
        tr.set_image_pixels(0, np.zeros((2, 2, 4), np.float32))
    with pytest.raises(RuntimeError, match="float32"):
        tr.set_image_pixels(0, np.zeros((2, 2, 4), np.uint8))
    with pytest.raises(RuntimeError, match="no such training view"):
        tr.image(0)
    with pytest.raises(RuntimeError, match="colours is not supported"):
        tr.set_image(0, np.zeros((2, 2, 4), np.float32))
