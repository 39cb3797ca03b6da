"""CPU tests of error-driven ray sampling: the engine's shared pixel lookup (csrc/nerf_pixel.h, compiled for the
host: training_pixels(host=True), no GPU call) against a float32 numpy restatement written from the description of
the reference's image_idx / nerf_random_image_pos_training / sample_cdf_2d / binary_search, and that restatement
against the distribution the CDFs describe.

Bitwise equality is the bar for the lookup: it uses only IEEE add, subtract, multiply, divide, compare and convert,
and the engine is built with -ffp-contract=off. tests/test_gpu_error_sampling.py imports the restatement and the
inputs from here.
"""
import functools

import numpy as np
import pytest

F = np.float32
N_IMG, IMG_W, IMG_H = 4, 48, 32   # non-square: catches swapped axes
CDF_W, CDF_H = 7, 5
N_RAYS = 1 << 16
SEED = 20
FLAGS = [(True, True), (True, False), (False, True), (False, False)]  # (focal_plane, image)


@pytest.fixture(scope="module")
def pkg():
    from __graft_entry__ import load_package
    return load_package()


def make_images(pkg, w=IMG_W, h=IMG_H, n=N_IMG):
    S = pkg.synthetic
    return [pkg.nerf.make_image(w, h, pkg.nerf.nerf_matrix_to_ngp(c2w), camera_angle_x=S.LEGO_CAMERA_ANGLE_X)
            for c2w in S.camera_poses(n, seed=3)]


@functools.lru_cache(maxsize=None)
def error_map():
    """A random non-negative map [N_IMG, CDF_H, CDF_W] with one all-zero row, one all-zero image and one cell 50
    times the rest."""
    g = np.random.default_rng(11)
    m = g.uniform(0.5, 1.5, (N_IMG, CDF_H, CDF_W)).astype(F)
    m[1, 3, :] = 0.0
    m[2] = 0.0
    m[3, 1, 4] = 50.0
    return m


def make_cdfs(orc, data=None):
    """The trainer's CDFs of a map: construct_cdf_2d / 1d and the host pass over the image totals (pyoracle)."""
    cx, cy, ci = orc.error_map_cdfs(error_map() if data is None else data)
    pmf_img, cdf_img = orc.error_map_image_pmf(ci)
    return {"cdf_x_cond_y": cx, "cdf_y": cy, "cdf_img": cdf_img, "pmf_img": pmf_img}


def select(cdfs, focal_plane, image):
    """The dict the engine takes for a pair of switches (an absent entry is a null pointer)."""
    d = {}
    if focal_plane:
        d["cdf_x_cond_y"], d["cdf_y"] = cdfs["cdf_x_cond_y"], cdfs["cdf_y"]
    if image:
        d["cdf_img"] = cdfs["cdf_img"]
    return d


_draws = {}


def draws(orc, rng, n_total):
    """Per global ray index of a batch: the two pcg floats of the ray's stream (advanced by 16 per ray) and the
    low-discrepancy image sample, from pyoracle's pcg32 and orc_ld_random_val."""
    key = (rng.state, rng.inc, n_total)
    if key not in _draws:
        L = orc.lib()
        x, y, ld = np.zeros(n_total, F), np.zeros(n_total, F), np.zeros(n_total, F)
        r = orc.Rng(0)
        for i in range(n_total):
            r.s.state, r.s.inc = rng.state, rng.inc
            r.advance(i * 16)
            x[i] = r.next_float()
            y[i] = r.next_float()
            ld[i] = L.orc_ld_random_val(i, 0xdeadbeef, 0)
        _draws[key] = (x, y, ld)
    return _draws[key]


def binary_search(val, rows):
    """common.h:268-292 per ray: rows [n, L] is each ray's CDF row, val [n]. First index whose entry is not below
    val, clamped to L - 1."""
    n, L = rows.shape
    ar = np.arange(n)
    first, count = np.zeros(n, np.int64), np.full(n, L, np.int64)
    while (count > 0).any():
        act = count > 0
        step = count // 2
        it = first + step
        lt = act & (rows[ar, np.minimum(it, L - 1)] < val)
        first = np.where(lt, it + 1, first)
        count = np.where(lt, count - step - 1, np.where(act, step, count))
    return np.minimum(first, L - 1)


def restate(orc, rng, n_rays, n_total, sizes, snap, cdfs, ray_offset=0):
    """The lookup in float32 numpy. sizes: [(w, h)] per image; cdfs: select(...)'s dict. Returns img, uv, pdf like
    training_pixels and, for the tests, half (True: the CDF half), col, row."""
    x, y, ld = (a[ray_offset:ray_offset + n_rays].copy() for a in draws(orc, rng, n_total))
    ig = np.arange(ray_offset, ray_offset + n_rays, dtype=np.uint64)
    n_images = len(sizes)
    img_pdf, uv_pdf = np.ones(n_rays, F), np.ones(n_rays, F)
    if "cdf_img" in cdfs:
        c = np.asarray(cdfs["cdf_img"], F)
        img = binary_search(ld, np.broadcast_to(c, (n_rays, n_images)))
        prev = np.where(img > 0, c[np.maximum(img - 1, 0)], F(0))
        img_pdf = ((c[img] - prev) * F(n_images)).astype(F)
    else:
        img = ((((ig * n_images) & 0xFFFFFFFF) // n_total) % n_images).astype(np.int64)
    half = np.zeros(n_rays, bool)
    col, row = np.zeros(n_rays, np.int64), np.zeros(n_rays, np.int64)
    if "cdf_x_cond_y" in cdfs:
        cx, cy = np.asarray(cdfs["cdf_x_cond_y"], F), np.asarray(cdfs["cdf_y"], F)
        h, w = cx.shape[1:]
        half = ~(x < F(0.5))
        xu = x / F(0.5)
        xs = (x - F(0.5)) / (F(1.0) - F(0.5))
        rows_y = cy[img]
        row = binary_search(y, rows_y)
        ar = np.arange(n_rays)
        prev = np.where(row > 0, rows_y[ar, np.maximum(row - 1, 0)], F(0))
        pmf_y = rows_y[ar, row] - prev
        ys = (y - prev) / pmf_y
        rows_x = cx[img, row]
        col = binary_search(xs, rows_x)
        prev = np.where(col > 0, rows_x[ar, np.maximum(col - 1, 0)], F(0))
        pmf_x = rows_x[ar, col] - prev
        xs = (xs - prev) / pmf_x
        pdf = pmf_x * pmf_y * F(w * h)
        xs = (col.astype(F) + xs) / F(w)
        ys = (row.astype(F) + ys) / F(h)
        x = np.where(half, xs, xu).astype(F)
        y = np.where(half, ys, y).astype(F)
        uv_pdf = np.where(half, pdf, F(1)).astype(F)
    if snap:
        W = np.array([s[0] for s in sizes], np.int64)[img]
        H = np.array([s[1] for s in sizes], np.int64)[img]
        px = np.clip((x * W.astype(F)).astype(np.int64), 0, W - 1)
        py = np.clip((y * H.astype(F)).astype(np.int64), 0, H - 1)
        x = (px.astype(F) + F(0.5)) / W.astype(F)
        y = (py.astype(F) + F(0.5)) / H.astype(F)
    return {"img": img.astype(np.uint32), "uv": np.stack([x, y], 1).astype(F), "pdf": np.stack([img_pdf, uv_pdf], 1).astype(F),
            "half": half, "col": col, "row": row}


def batch_rng(pkg):
    return pkg.nerf.pcg32(SEED)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize("snap", [1, 0])
@pytest.mark.parametrize("focal_plane,image", FLAGS)
def test_host_lookup_equals_restatement_bitwise(pkg, orc, focal_plane, image, snap):
    ims = make_images(pkg)
    cfg = pkg.nerf.default_config(1.0, snap_to_pixel_centers=snap)
    cd = select(make_cdfs(orc), focal_plane, image)
    r = batch_rng(pkg)
    got = pkg.nerf.training_pixels(ims, cfg, N_RAYS, r, cdfs=cd, host=True)
    ref = restate(orc, r, N_RAYS, N_RAYS, [(IMG_W, IMG_H)] * N_IMG, snap, cd)
    np.testing.assert_array_equal(got["img"], ref["img"])
    np.testing.assert_array_equal(bits(got["uv"]), bits(ref["uv"]))
    np.testing.assert_array_equal(bits(got["pdf"]), bits(ref["pdf"]))
    if focal_plane:
        assert ref["half"].sum() > N_RAYS // 3 and (~ref["half"]).sum() > N_RAYS // 3
        # the image shape is not the CDF's: a swapped axis would show
        assert len(np.unique(ref["col"][ref["half"]])) == CDF_W and len(np.unique(ref["row"][ref["half"]])) == CDF_H
    if not focal_plane and not image:
        # today's formulas: image from the ray index, position the two pcg floats, pdfs 1
        x, y, _ = draws(orc, r, N_RAYS)
        i = np.arange(N_RAYS, dtype=np.uint64)
        np.testing.assert_array_equal(got["img"], ((i * N_IMG) // N_RAYS) % N_IMG)
        if snap:
            x = ((x * F(IMG_W)).astype(np.int64).clip(0, IMG_W - 1).astype(F) + F(0.5)) / F(IMG_W)
            y = ((y * F(IMG_H)).astype(np.int64).clip(0, IMG_H - 1).astype(F) + F(0.5)) / F(IMG_H)
        np.testing.assert_array_equal(bits(got["uv"]), bits(np.stack([x, y], 1)))
        assert (got["pdf"] == 1.0).all()
        # and a null cdfs argument is the same as one with null pointers
        none = pkg.nerf.training_pixels(ims, cfg, N_RAYS, r, cdfs=None, host=True)
        for k in ("img", "uv", "pdf"):
            np.testing.assert_array_equal(bits(none[k]), bits(got[k]))


def test_host_lookup_of_a_shard_is_that_slice(pkg, orc):
    ims = make_images(pkg)
    cfg = pkg.nerf.default_config(1.0)
    cd = select(make_cdfs(orc), True, True)
    r = batch_rng(pkg)
    full = pkg.nerf.training_pixels(ims, cfg, N_RAYS, r, cdfs=cd, host=True)
    part = pkg.nerf.training_pixels(ims, cfg, 3000, r, cdfs=cd, ray_offset=1000, n_rays_total=N_RAYS, host=True)
    for k in ("img", "uv", "pdf"):
        np.testing.assert_array_equal(bits(part[k]), bits(full[k][1000:4000]))


def test_last_cdf_entry_below_one_stays_in_its_row(pkg, orc):
    """Rows whose last entry rounds to 0.99999994 with samples above it, and CDFs that are not CDFs at all (zeros,
    NaN): every search result is clamped to the row's last entry, so the lookup returns a valid image and a pixel
    inside it (a load past a row would read the neighbouring row and show as a different cell or pdf here)."""
    ims = make_images(pkg)
    cfg = pkg.nerf.default_config(1.0)
    cd = {k: np.array(v, F) for k, v in select(make_cdfs(orc), True, True).items()}
    below = np.nextafter(F(1), F(0))
    cd["cdf_x_cond_y"][:, :, -1] = below
    cd["cdf_y"][:, -1] = below
    cd["cdf_img"][-1] = below
    r = batch_rng(pkg)
    got = pkg.nerf.training_pixels(ims, cfg, N_RAYS, r, cdfs=cd, host=True)
    ref = restate(orc, r, N_RAYS, N_RAYS, [(IMG_W, IMG_H)] * N_IMG, 1, cd)
    for k in ("img", "uv", "pdf"):
        np.testing.assert_array_equal(bits(got[k]), bits(ref[k]))
    assert got["img"].max() == N_IMG - 1 and (got["uv"] > 0).all() and (got["uv"] < 1).all()
    for fill in (0.0, np.nan):
        bad = {k: np.full_like(v, fill) for k, v in cd.items()}
        got = pkg.nerf.training_pixels(ims, cfg, 4096, r, cdfs=bad, host=True)
        assert got["img"].max() < N_IMG and (got["uv"] > 0).all() and (got["uv"] < 1).all()


def test_restatement_samples_what_the_cdfs_say(pkg, orc):
    """Counts per CDF cell against the probabilities the CDFs describe, at 6 binomial standard deviations. The
    focal-plane switch alone keeps the images uniform (2^14 rays each), so every cell expects at least 0.5 / 35 *
    2^14 = 234 rays; with numpy's own generator in place of the pcg stream the worst cell of this map was at 4.2,
    with the pcg stream at SEED it is at 2.5. The image choice, low-discrepancy, is checked against pmf_img."""
    cdfs = make_cdfs(orc)
    r = batch_rng(pkg)
    sizes = [(IMG_W, IMG_H)] * N_IMG
    ref = restate(orc, r, N_RAYS, N_RAYS, sizes, 0, select(cdfs, True, False))
    cx, cy = cdfs["cdf_x_cond_y"].astype(np.float64), cdfs["cdf_y"].astype(np.float64)
    pmf_x = np.diff(np.concatenate([np.zeros((N_IMG, CDF_H, 1)), cx], axis=2), axis=2)
    pmf_y = np.diff(np.concatenate([np.zeros((N_IMG, 1)), cy], axis=1), axis=1)
    p = 0.5 / (CDF_W * CDF_H) + 0.5 * pmf_x * pmf_y[:, :, None]
    np.testing.assert_allclose(p.sum(axis=(1, 2)), 1.0, atol=1e-5)
    cu = np.clip((ref["uv"][:, 0].astype(np.float64) * CDF_W).astype(int), 0, CDF_W - 1)
    cv = np.clip((ref["uv"][:, 1].astype(np.float64) * CDF_H).astype(int), 0, CDF_H - 1)
    worst = 0.0
    for i in range(N_IMG):
        m = ref["img"] == i
        n = int(m.sum())
        assert n == N_RAYS // N_IMG
        cnt = np.zeros((CDF_H, CDF_W))
        np.add.at(cnt, (cv[m], cu[m]), 1)
        assert (n * p[i] >= 200).all()
        z = np.abs(cnt - n * p[i]) / np.sqrt(n * p[i] * (1 - p[i]))
        worst = max(worst, float(z.max()))
    print(f"worst cell: {worst:.2f} standard deviations")
    assert worst < 6.0
    # the heavy cell (50 against 34 cells of about 1) draws about 0.5 * 50 / 84 of image 3's rays, the checks above
    # are not about a flat map
    assert p[3, 1, 4] > 0.25
    ref = restate(orc, r, N_RAYS, N_RAYS, sizes, 0, select(cdfs, False, True))
    pm = cdfs["pmf_img"].astype(np.float64)
    cnt = np.bincount(ref["img"], minlength=N_IMG)
    z = np.abs(cnt - N_RAYS * pm) / np.sqrt(N_RAYS * pm * (1 - pm))
    print(f"image choice: {z.max():.2f} standard deviations; counts {cnt.tolist()}")
    assert z.max() < 6.0
    assert cnt[2] == cnt.min() and cnt[2] > 0  # the all-zero image keeps its floor share and no more


@pytest.mark.parametrize("snap", [1, 0])
def test_pdfs(pkg, orc, snap):
    """uv_pdf is exactly 1 on the uniform half and exactly pmf_x * pmf_y * 35 of the returned cell on the other;
    img_pdf is the image's CDF step times the image count."""
    ims = make_images(pkg)
    cfg = pkg.nerf.default_config(1.0, snap_to_pixel_centers=snap)
    cdfs = make_cdfs(orc)
    cd = select(cdfs, True, True)
    r = batch_rng(pkg)
    got = pkg.nerf.training_pixels(ims, cfg, N_RAYS, r, cdfs=cd, host=True)
    ref = restate(orc, r, N_RAYS, N_RAYS, [(IMG_W, IMG_H)] * N_IMG, snap, cd)
    x, _, _ = draws(orc, r, N_RAYS)
    uniform = x < F(0.5)
    np.testing.assert_array_equal(uniform, ~ref["half"])
    assert (got["pdf"][uniform, 1] == 1.0).all()
    img, row, col = got["img"].astype(np.int64), ref["row"], ref["col"]
    cx, cy, ci = cdfs["cdf_x_cond_y"], cdfs["cdf_y"], cdfs["cdf_img"]
    pmf_x = cx[img, row, col] - np.where(col > 0, cx[img, row, np.maximum(col - 1, 0)], F(0))
    pmf_y = cy[img, row] - np.where(row > 0, cy[img, np.maximum(row - 1, 0)], F(0))
    want = (pmf_x * pmf_y * F(35)).astype(F)
    np.testing.assert_array_equal(bits(got["pdf"][~uniform, 1]), bits(want[~uniform]))
    if not snap:  # the returned position lies in the returned cell
        u, v = got["uv"][~uniform, 0], got["uv"][~uniform, 1]
        assert (np.abs(u * CDF_W - (col[~uniform] + 0.5)) <= 0.5 + 1e-5).all()
        assert (np.abs(v * CDF_H - (row[~uniform] + 0.5)) <= 0.5 + 1e-5).all()
    want_img = ((ci[img] - np.where(img > 0, ci[np.maximum(img - 1, 0)], F(0))) * F(N_IMG)).astype(F)
    np.testing.assert_array_equal(bits(got["pdf"][:, 0]), bits(want_img))


def test_pyngp_properties_without_a_trainer(pkg):
    """nerf.training.sample_*_proportional_to_error (python_api.cu:624-625): default False, kept until there is a
    trainer, and refused together with optimize_extrinsics in either order, with the state left as it was."""
    ngp = pkg.pyngp()
    tr = ngp.Testbed().nerf.training
    assert tr.sample_focal_plane_proportional_to_error is False and tr.sample_image_proportional_to_error is False
    tr.sample_image_proportional_to_error = True
    assert tr.sample_focal_plane_proportional_to_error is False and tr.sample_image_proportional_to_error is True
    with pytest.raises(RuntimeError, match="optimize_extrinsics.*sample_image_proportional_to_error"):
        tr.optimize_extrinsics = True
    assert tr.optimize_extrinsics is False
    tr.sample_image_proportional_to_error = False
    tr.optimize_extrinsics = True
    with pytest.raises(RuntimeError, match="optimize_extrinsics.*sample_focal_plane_proportional_to_error"):
        tr.sample_focal_plane_proportional_to_error = True
    assert tr.sample_focal_plane_proportional_to_error is False and tr.optimize_extrinsics is True
