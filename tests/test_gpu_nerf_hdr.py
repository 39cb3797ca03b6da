"""HDR training images on the GPU: the loss pass's TEX instantiations against the float64 restatement of
test_nerf_hdr_host.py (Half and Float texels, every loss, the three colour spaces, the plain and kept-state forms, ray
counts around the kernels' group sizes), bitwise identities where the operations are the same (Half against Float of
the same values, a Byte image inside a mixed dataset against the Byte dataset, create_typed against create, with every
combination of the loss pass's other switches), the sampler's mask, set_image and read-back, and an end-to-end run
through pyngp on EXR frames against clipped 8-bit frames.

The bound is test_gpu_nerf_loss.py's (K_GPU = 4 K32) with its compare; test_nerf_hdr_host.py's docstring says why K32
holds for the HDR target."""
import ctypes as C
import itertools
import json

import numpy as np
import pytest
import torch

from test_gpu_nerf_exposure import position_cdfs
from test_gpu_nerf_loss import K_GPU, MAX_C, bitwise_equal, check, run
from test_nerf_hdr_host import IMAGE_BYTE, IMAGE_FLOAT, IMAGE_HALF, NGP_INVALID, half_images, hdr_world, restate_loss_hdr
from test_nerf_loss_host import ACT_NONE, MASKED, RAY_COUNTS, batches, make_cfg

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pkg():
    from __graft_entry__ import load_package
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return load_package()


@pytest.fixture(scope="module")
def world(pkg):
    full, pixels, _ = hdr_world(pkg)
    return full, pixels, pkg.nerf.NerfDataset(full.images, pixels)


# ---- 1. the loss pass against float64 --------------------------------------------------------------------------------------
@pytest.mark.parametrize("group", ("losses", "colour_spaces"))
def test_hdr_loss_pass_matches_float64(pkg, world, group):
    """Image 0 and 2 Half, image 1 Float; every loss, the three colour spaces under L2 and RelativeL2; the plain form
    against float64 and the kept-state form with the plain form's bits."""
    full, pixels, ds = world
    assert ds.is_hdr and ds.image_types == [IMAGE_HALF, IMAGE_FLOAT, IMAGE_HALF]
    groups, _, _, _ = batches(pkg)
    worst = (0.0, 0.0)
    for label, cfg, mean in groups[group]:
        ref = restate_loss_hdr(full, pixels, cfg, mean, max_compacted=MAX_C)
        got = run(pkg, ds, full, cfg, mean)
        ul, ug = check(ref, got)
        assert ref["compacted_counter"] > 1000 and np.abs(ref["grad"]).max() > 0
        bitwise_equal(got, run(pkg, ds, full, cfg, mean, keep_state=True))
        worst = (max(worst[0], ul), max(worst[1], ug))
    print(f"HDR {group}: worst err / bound, loss {worst[0] / K_GPU:.3f}, gradient (beyond half an fp16 ulp) {worst[1] / K_GPU:.3f}"
          f" over {len(groups[group])} configurations")


@pytest.mark.parametrize("n_rays", RAY_COUNTS)
def test_hdr_ray_counts(pkg, world, n_rays):
    """The first n rays as a batch of their own: a scan group of 4, a block of 16 rays, an XCD group of 128, each with a
    ragged tail; the plain form against float64, the kept-state form with its bits."""
    full, pixels, ds = world
    worst = (0.0, 0.0)
    for cfg in (make_cfg(pkg), make_cfg(pkg, "L2", ACT_NONE, ACT_NONE)):
        ref = restate_loss_hdr(full, pixels, cfg, max_compacted=MAX_C, n_rays=n_rays)
        plain = run(pkg, ds, full, cfg, n_rays=n_rays)
        ul, ug = check(ref, plain)
        worst = (max(worst[0], ul), max(worst[1], ug))
        bitwise_equal(plain, run(pkg, ds, full, cfg, n_rays=n_rays, keep_state=True))
    print(f"HDR {n_rays} rays: worst err / bound, loss {worst[0] / K_GPU:.3f}, gradient {worst[1] / K_GPU:.3f}")


# ---- 2. the same bits where the operations are the same -------------------------------------------------------------------
SWITCHES = list(itertools.product((False, True), repeat=4))   # (cdfs, envmap, depth, exposure): every TEX instantiation


def switch_kwargs(pkg, datasets, full, cdfs, envmap, depth, exposure):
    """compute_loss' keywords for a combination of its other switches, through the entry point that takes them all;
    depth images go to every dataset of `datasets`."""
    kw = {"exposure_entry": True}
    if cdfs:
        kw["cdfs"] = position_cdfs(3, 5, 4, 1)
    if envmap:
        g = np.random.default_rng(8)
        kw["envmap"] = torch.from_numpy(g.uniform(0.0, 1.0, (6, 9, 4)).astype(np.float32)).cuda()
    if depth:
        for ds in datasets:
            for i, im in enumerate(full.images):
                ds.set_depth(i, np.random.default_rng(20 + i).uniform(0.5, 3.0, (im.height, im.width)).astype(np.float32), 0.33)
        kw.update(depth_lambda=0.5, depth_loss="L2")
    if exposure:
        kw["exposure"] = torch.from_numpy(np.random.default_rng(9).uniform(-1, 1, (3, 3)).astype(np.float32)).cuda()
    return kw


@pytest.mark.parametrize("cdfs,envmap,depth,exposure", SWITCHES)
def test_half_and_float_of_the_same_values_give_the_same_bits(pkg, world, cdfs, envmap, depth, exposure):
    """(a) A Float dataset whose values are all fp16 values and the Half dataset of those values: loss, dloss_doutput,
    numsteps, the compacted counter and the coordinates bit for bit, under every combination of the other switches."""
    full, pixels, _ = world
    h16, f32 = half_images(pixels)
    ds_h, ds_f = pkg.nerf.NerfDataset(full.images, h16), pkg.nerf.NerfDataset(full.images, f32)
    assert ds_h.image_types == [IMAGE_HALF] * 3 and ds_f.image_types == [IMAGE_FLOAT] * 3
    kw = switch_kwargs(pkg, (ds_h, ds_f), full, cdfs, envmap, depth, exposure)
    cfg = make_cfg(pkg)
    a, b = run(pkg, ds_h, full, cfg, **kw), run(pkg, ds_f, full, cfg, **kw)
    assert a["compacted_counter"].view(np.uint32)[0] > 1000 and a["loss"].any()
    bitwise_equal(a, b)


def rows_of(numsteps, rays):
    ns = numsteps.view(np.uint32).reshape(-1, 2)
    return np.concatenate([np.arange(ns[r, 1], ns[r, 1] + ns[r, 0]) for r in rays]).astype(np.int64)


@pytest.mark.parametrize("cdfs,envmap,depth,exposure", SWITCHES)
def test_byte_image_in_a_mixed_dataset_gives_the_byte_dataset_bits(pkg, world, cdfs, envmap, depth, exposure):
    """(b) Image 0 Byte, images 1 and 2 Float: every output of the rays of image 0 equals the all-Byte dataset's bit for
    bit (the compaction does not read texels, so all rows line up), and the rays of the other images do see other targets."""
    full, pixels, _ = world
    mixed = pkg.nerf.NerfDataset(full.images, [full.pixels[0], pixels[1].astype(np.float32), pixels[2].astype(np.float32)])
    byte = pkg.nerf.NerfDataset(full.images, full.pixels)
    assert mixed.image_types == [IMAGE_BYTE, IMAGE_FLOAT, IMAGE_FLOAT] and mixed.is_hdr and not byte.is_hdr
    kw = switch_kwargs(pkg, (mixed, byte), full, cdfs, envmap, depth, exposure)
    cfg = make_cfg(pkg)
    a, b = run(pkg, mixed, full, cfg, **kw), run(pkg, byte, full, cfg, **kw)
    for k in ("numsteps", "compacted_counter", "coords_compacted"):
        np.testing.assert_array_equal(a[k].view(np.uint32), b[k].view(np.uint32), err_msg=k)
    img = full.px["img"]     # position CDFs leave the image choice as it is
    ns = a["numsteps"].view(np.uint32).reshape(-1, 2)
    first = np.nonzero((img == 0) & (ns[:, 0] > 0))[0]
    other = np.nonzero((img != 0) & (ns[:, 0] > 0))[0]
    assert first.size > 50 and other.size > 100
    np.testing.assert_array_equal(a["loss"][first].view(np.uint32), b["loss"][first].view(np.uint32))
    rows = rows_of(a["numsteps"], first)
    np.testing.assert_array_equal(a["dloss_doutput"].view(np.uint16)[rows], b["dloss_doutput"].view(np.uint16)[rows])
    assert (a["loss"][other] != b["loss"][other]).mean() > 0.85


def test_create_typed_with_byte_types_is_create(pkg, world):
    """(c) ngp_nerf_dataset_create_typed with every type Byte: the bytes read back and the loss pass's output are
    ngp_nerf_dataset_create's."""
    from instant_ngp_amd._capi import NerfImage, check as check_rc
    full, _, _ = world
    byte = pkg.nerf.NerfDataset(full.images, full.pixels)
    arr = (NerfImage * 3)(*full.images)
    bufs = [np.ascontiguousarray(p) for p in full.pixels]
    h = C.c_void_p()
    check_rc(pkg.lib().ngp_nerf_dataset_create_typed(3, arr, (C.c_void_p * 3)(*[b.ctypes.data for b in bufs]),
                                                     (C.c_uint32 * 3)(IMAGE_BYTE, IMAGE_BYTE, IMAGE_BYTE), C.byref(h)))
    typed = pkg.nerf.NerfDataset.__new__(pkg.nerf.NerfDataset)
    typed.handle, typed.images, typed.image_types = h, list(full.images), [IMAGE_BYTE] * 3
    for i in range(3):
        assert typed.image(i).dtype == np.uint8
        np.testing.assert_array_equal(typed.image(i), full.pixels[i])
        np.testing.assert_array_equal(byte.image(i), full.pixels[i])
    cfg = make_cfg(pkg)
    bitwise_equal(run(pkg, typed, full, cfg), run(pkg, byte, full, cfg))


# ---- 3. the sampler's mask -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("aabb_scale,cdfs", [(1.0, False), (1.0, True), (2.0, False), (2.0, True)])
def test_sampler_drops_rays_whose_texel_has_a_negative_red(pkg, orc, aabb_scale, cdfs):
    """A Float and a Half image with red < 0 at seeded pixels (and a Byte image with 0x00FF00FF) against the Byte dataset
    with 0x00FF00FF at the same pixels: generate_training_samples gives the same bits, at cone 0 and with cone stepping,
    with uniform pixels and with pixels from CDFs (the four TEX instantiations of the count pass). -0.0 is not < 0."""
    S = pkg.synthetic
    g = np.random.default_rng(31)
    images, byte, hdr, masks = [], [], [], []
    for i, (c2w, (w, h)) in enumerate(zip(S.camera_poses(3, seed=5), ((16, 16), (24, 20), (32, 32)))):
        images.append(pkg.nerf.make_image(w, h, pkg.nerf.nerf_matrix_to_ngp(c2w), camera_angle_x=S.LEGO_CAMERA_ANGLE_X))
        mask = g.random((h, w)) < 0.3
        b = g.integers(0, 256, (h, w, 4), dtype=np.uint8)
        b[(b == np.array(MASKED, np.uint8)).all(axis=-1)] = 0
        b[mask] = np.array(MASKED, np.uint8)
        f = g.uniform(0.0, 9.0, (h, w, 4)).astype(np.float32)
        f[..., 0][g.random((h, w)) < 0.2] = -0.0
        f[..., 0][g.random((h, w)) < 0.1] = 0.0
        f[..., 0][mask] = -g.uniform(1e-3, 4.0, int(mask.sum())).astype(np.float32)
        hdr.append(f if i == 0 else f.astype(np.float16) if i == 1 else b)
        assert ((hdr[-1][..., 0] < 0) == mask).all() or i == 2
        byte.append(b)
        masks.append(mask)
    ds_b, ds_h = pkg.nerf.NerfDataset(images, byte), pkg.nerf.NerfDataset(images, hdr)
    assert ds_h.image_types == [IMAGE_FLOAT, IMAGE_HALF, IMAGE_BYTE]
    cfg = pkg.nerf.default_config(aabb_scale)
    grid = np.where(np.random.default_rng(3).random(128 ** 3 * 8) < 0.3, 1.0, 0.0).astype(np.float32)
    bf = torch.from_numpy(orc.nerf_grid_bitfield(grid, int(cfg.max_cascade), 0.005)).cuda()
    n, rng = 300, pkg.nerf.pcg32(77)
    cd = dict(position_cdfs(3, 5, 4, 2), cdf_img=np.array([0.3, 0.6, 1.0], np.float32)) if cdfs else None
    a = pkg.nerf.generate_training_samples(ds_b, cfg, n, rng, 1 << 16, bf, cdfs=cd)
    b = pkg.nerf.generate_training_samples(ds_h, cfg, n, rng, 1 << 16, bf, cdfs=cd)
    torch.cuda.synchronize()
    for k in a:
        np.testing.assert_array_equal(a[k].cpu().numpy(), b[k].cpu().numpy(), err_msg=k)
    px = pkg.nerf.training_pixels(images, cfg, n, rng, cdfs=cd, host=True)
    hit = np.zeros(n, bool)
    for r in range(n):
        m = masks[px["img"][r]]
        h, w = m.shape
        x = min(max(int(np.float32(px["uv"][r, 0]) * np.float32(w)), 0), w - 1)
        y = min(max(int(np.float32(px["uv"][r, 1]) * np.float32(h)), 0), h - 1)
        hit[r] = m[y, x]
    kept = int(a["counters"].cpu().numpy().view(np.uint32)[0])
    assert 30 < hit.sum() < n - 100 and set(np.unique(px["img"])) == {0, 1, 2}
    assert kept > 0 and not hit[a["ray_indices"].cpu().numpy().view(np.uint32)[:kept]].any()


# ---- 4. set_image and read-back --------------------------------------------------------------------------------------------
def test_set_image_replaces_an_image_and_reads_back(pkg, world):
    """Byte -> Float -> Half -> Byte on image 0 of a Byte dataset: read back exactly, the next compute_loss equals a fresh
    dataset of the same arrays bit for bit; a resolution mismatch, a bad index, an unknown type and a short capacity are
    refused and leave the image as it was."""
    full, pixels, _ = world
    cfg = make_cfg(pkg)
    L = pkg.lib()
    ds = pkg.nerf.NerfDataset(full.images, full.pixels)
    f0 = pixels[0].astype(np.float32) * np.float32(1.7)
    h0 = pixels[0].astype(np.float16)
    b0 = np.ascontiguousarray(full.pixels[0][::-1])
    for new in (f0, h0, b0):
        ds.set_image(0, new)
        back = ds.image(0)
        assert back.dtype == new.dtype
        np.testing.assert_array_equal(back.view(np.uint8), np.ascontiguousarray(new).view(np.uint8))
        fresh = pkg.nerf.NerfDataset(full.images, [new, full.pixels[1], full.pixels[2]])
        assert ds.image_types == fresh.image_types and ds.is_hdr == fresh.is_hdr == (new.dtype != np.uint8)
        bitwise_equal(run(pkg, ds, full, cfg), run(pkg, fresh, full, cfg))
        for i in (1, 2):
            np.testing.assert_array_equal(ds.image(i), full.pixels[i])
    im = full.images[0]
    with pytest.raises(ValueError, match="shape"):
        ds.set_image(0, np.zeros((im.height + 1, im.width, 4), np.float32))
    with pytest.raises(IndexError):
        ds.set_image(3, f0)
    big = np.zeros((im.height + 1, im.width + 1, 4), np.float32)
    for args in ((0, big.ctypes.data, IMAGE_FLOAT, im.width + 1, im.height), (0, big.ctypes.data, IMAGE_FLOAT, im.width, im.height + 1),
                 (3, big.ctypes.data, IMAGE_FLOAT, im.width, im.height), (0, big.ctypes.data, 0, im.width, im.height),
                 (0, big.ctypes.data, 4, im.width, im.height), (0, None, IMAGE_FLOAT, im.width, im.height)):
        assert L.ngp_nerf_dataset_set_image(ds.handle, *args) == NGP_INVALID
    t = C.c_uint32(0)
    out = np.zeros(b0.nbytes, np.uint8)
    assert L.ngp_nerf_dataset_image(ds.handle, 3, out.ctypes.data, out.nbytes, C.byref(t)) == NGP_INVALID
    assert L.ngp_nerf_dataset_image(ds.handle, 0, out.ctypes.data, out.nbytes - 1, C.byref(t)) == NGP_INVALID and not out.any()
    assert L.ngp_nerf_dataset_image(ds.handle, 0, None, 0, C.byref(t)) == 0 and t.value == IMAGE_BYTE
    np.testing.assert_array_equal(ds.image(0), b0)


def test_trainer_drops_the_sampler_it_launched_ahead_when_an_image_is_replaced(pkg):
    """Four Float views; after six steps image 0 is replaced by a Half image whose every red is < 0, so the sampler must
    drop its rays from then on (image 0: its rays come first in ray order, and in these early steps, with the whole grid
    still occupied, the sample budget cuts the batch before the later images' rays). With pipelining the seventh step's
    sampler has already run on the old image: the trainer discards it, and twelve steps give the parameters, bit for
    bit, of a trainer that never launches ahead (which differ from a run whose image was left alone)."""
    S = pkg.synthetic
    ims, views = [], []
    for c2w in S.camera_poses(4, seed=7):
        ims.append(pkg.nerf.make_image(32, 32, pkg.nerf.nerf_matrix_to_ngp(c2w), camera_angle_x=S.LEGO_CAMERA_ANGLE_X))
        px = S.render(c2w, 32, 32).astype(np.float32) / np.float32(255)
        views.append(np.concatenate([px[..., :3] ** 2.2 * px[..., 3:4] * 3.0, px[..., 3:4]], axis=-1).astype(np.float32))
    masked = views[0].astype(np.float16)
    masked[..., 0] = -1.0
    params = {}
    for name, pipeline, replace in (("pipelined", True, True), ("serial", False, True), ("untouched", True, False)):
        ds = pkg.nerf.NerfDataset(ims, views)
        ncfg = pkg.nerf_config("C2")
        ncfg["encoding"]["log2_hashmap_size"] = 14
        net = pkg.create_nerf_network(ncfg)
        tr = pkg.Trainer(net, ncfg["optimizer"], seed=7)
        run_ = pkg.nerf.NerfTraining(net, tr, ds, pkg.nerf.default_config(1.0, target_batch_size=1 << 14), seed=1337)
        run_.set_pipeline(pipeline)
        for step in range(12):
            if replace and step == 6:
                ds.set_image(0, masked)
                assert ds.image_types == [IMAGE_HALF, IMAGE_FLOAT, IMAGE_FLOAT, IMAGE_FLOAT]
            run_.train_step(get_loss=False)
        torch.cuda.synchronize()
        params[name] = tr.serialize()
    assert params["pipelined"] == params["serial"]
    assert params["pipelined"] != params["untouched"]


# ---- 5. end to end through pyngp -------------------------------------------------------------------------------------------
E2E_VIEWS, E2E_RES, E2E_STEPS, E2E_GAIN, E2E_BATCH = 8, 32, 300, 6.0, 1 << 16
E2E_RATIO = 0.72


def _srgb_to_linear(s):
    return np.where(s <= 0.04045, s / 12.92, ((s + 0.055) / 1.055) ** 2.4)


def _linear_to_srgb(l):
    return np.where(l < 0.0031308, 12.92 * l, 1.055 * np.maximum(l, 0) ** (1 / 2.4) - 0.055)


def _radiance(pkg, c2w):
    """The procedural scene's view as linear premultiplied RGBA float32, its radiance scaled by E2E_GAIN."""
    px = pkg.synthetic.render(c2w, E2E_RES, E2E_RES).astype(np.float64) / 255.0
    return np.concatenate([_srgb_to_linear(px[..., :3]) * px[..., 3:4] * E2E_GAIN, px[..., 3:4]], axis=-1).astype(np.float32)


def _train(pkg, folder, replace_frame=None):
    ngp = pkg.pyngp()
    tb = ngp.Testbed()
    tb.load_training_data(str(folder))
    tb.training_batch_size = E2E_BATCH
    tb.shall_train = True
    for step in range(E2E_STEPS):
        if replace_frame is not None and step == E2E_STEPS // 2:
            tr = tb.nerf.training
            own = tr.image(replace_frame)
            assert own.dtype == np.float16
            tr.set_image_pixels(replace_frame, own.astype(np.float32))
            back = tr.image(replace_frame)
            assert back.dtype == np.float32 and (back == own.astype(np.float32)).all()
        tb.frame()
        assert np.isfinite(tb.loss)
    assert tb.training_step == E2E_STEPS
    return tb


def test_training_on_exr_frames_recovers_radiance_above_one(pkg, tmp_path):
    """The procedural scene at 32 x 32 from 8 views, radiance scaled by 6 so that a substantial share of the covered pixels
    lies above 1. One run trains on 8-bit PNGs (clipped at 1), the other on EXR frames through load_training_data (Half,
    is_hdr, Exponential rgb activation), has frame 3 replaced through set_image_pixels with its own data as Float after
    150 steps and trains on; both take 300 steps and render a held-out view in linear colours. Over the pixels whose truth
    exceeds 1 the HDR model's RMS error must be below E2E_RATIO of the 8-bit model's.
    Measured once on an MI355X (353 of the held-out view's 452 covered pixels lie above 1): 8-bit RMS error 1.2964, HDR
    0.5812, ratio 0.448. The bar, 0.72, is that ratio plus half of the measured advantage (1 - 0.448) / 2 = 0.276, so the
    HDR run keeps at least half of it as margin against the run-to-run differences of pipelined training."""
    from PIL import Image
    from instant_ngp_amd.exr import write_exr
    S = pkg.synthetic
    poses = S.camera_poses(E2E_VIEWS + 1, seed=6)
    ldr, hdr = tmp_path / "ldr", tmp_path / "hdr"
    for folder in (ldr, hdr):
        folder.mkdir()
    frames = {"ldr": [], "hdr": []}
    for i, c2w in enumerate(poses[:E2E_VIEWS]):
        rad = _radiance(pkg, c2w)
        a = rad[..., 3:4]
        straight = np.clip(np.where(a > 0, rad[..., :3] / np.maximum(a, 1e-6), 0.0), 0.0, 1.0)       # what 8 bits can hold
        png = np.concatenate([_linear_to_srgb(straight), a], axis=-1)
        Image.fromarray((png * 255 + 0.5).clip(0, 255).astype(np.uint8), "RGBA").save(ldr / f"r_{i}.png")
        write_exr(str(hdr / f"r_{i}.exr"), rad, pixel_type=1)
        for name, ext in (("ldr", "png"), ("hdr", "exr")):
            frames[name].append({"file_path": f"r_{i}.{ext}", "transform_matrix": np.asarray(c2w, np.float64).tolist()})
    for name, folder in (("ldr", ldr), ("hdr", hdr)):
        (folder / "transforms.json").write_text(json.dumps({"camera_angle_x": S.LEGO_CAMERA_ANGLE_X, "frames": frames[name]}))
    truth = _radiance(pkg, poses[E2E_VIEWS])
    bright = (truth[..., :3].max(axis=-1) > 1.0) & (truth[..., 3] > 0)
    covered = truth[..., 3] > 0
    assert bright.sum() > 0.25 * covered.sum() > 20
    err = {}
    for name, folder in (("ldr", ldr), ("hdr", hdr)):
        tb = _train(pkg, folder, replace_frame=3 if name == "hdr" else None)
        assert tb.nerf.training.dataset.is_hdr == (name == "hdr")
        if name == "hdr":
            assert tb.nerf.rgb_activation == pkg.pyngp().NerfActivation.Exponential
        tb.set_camera_to_training_view(0)
        tb.camera_matrix = pkg.nerf.nerf_matrix_to_ngp(poses[E2E_VIEWS]).reshape(4, 3).T
        img = tb.render(E2E_RES, E2E_RES, 4, True)
        assert np.isfinite(img).all()
        err[name] = float(np.sqrt(((img[..., :3] - truth[..., :3])[bright] ** 2).mean()))
    ratio = err["hdr"] / err["ldr"]
    print(f"held-out RMS error over the {int(bright.sum())} pixels above 1 (of {int(covered.sum())} covered): 8-bit "
          f"{err['ldr']:.4f}, HDR {err['hdr']:.4f}, ratio {ratio:.3f} (bar {E2E_RATIO})")
    assert ratio < E2E_RATIO
