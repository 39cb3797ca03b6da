"""Per-image exposure (Training::optimize_exposure; testbed_nerf.cu:1794-1818, 1973-1986, 3831-3858) on the host: the
float64 restatement of the loss pass's target with exposure and of the exposure gradient, per ray and per image, which
test_gpu_nerf_exposure.py imports, and the CPU tests: margins, the zero-exposure identity, central differences (the
gradient's missing texel factor), a float32 restatement that measures K32E, the host optimisers, the C-ABI's argument
checks, pyngp's knobs and the synthetic scene's exposure. No GPU call is made.

restate_loss (test_nerf_loss_host.py) has no exposure argument, so the target is restated here: the premultiplied linear
texel times 2^exposure[img] per channel (exp(0.6931471805599453f * e), the reference's float literal), in each of the
three colour spaces. Everything else is that module's: while restate_loss runs, its loss_channel and
loss_channel_companion are handed this file's target (and its companion) in place of the one restate_loss made, so the
prediction, the stop and compaction decisions, the sample gradients and their companions are its own code, applied to
the exposed target.

The exposure gradient of a ray, per channel (the reference's expression, which is NOT the loss's derivative: it leaves
out the texel's own value, d target / d exposure = ln2 * 2^e * texel):
    loss_scale / n_rays * (-dL/dprediction / uv_pdf [/ srgb_to_linear_derivative(target)]) * 2^e * ln2
and per image the sum over its rays that compact to at least one sample. Its companion follows the module's rule (one
rounding per operation, first order): the loss gradient's companion, 5 roundings and the propagated target error for the
sRGB derivative's powf, 3 |ln2 e| + 2 for the exponential of a rounded product, 4 for the remaining products.

K32E: the float32 numpy restatement of the per-ray gradient (every operation in the kernel's order, numpy's float32 exp
and power) against float64 on the 300-ray batch, in units of 2^-24 companion, over exposure_configs(): measured 0.419
(sRGB 0.352, linear 0.296, color_space_linear 0.419), K32E = 0.45 (the measured worst rounded up to the next 0.05;
test_float32_restatement_measures_k32e prints it). K32X: the same run's float32 loss gradient dL/dprediction at the
exposed target against float64, in units of its own companion: measured 0.319 (0.250, 0.319, 0.250), K32X = 0.35. The
sample gradients' companion is a sum of non-negative terms of which the loss gradient's is one, so with that term off
by K32X and the others by the module's K32 (0.25, measured there without exposure) the sum is off by at most
max(K32, K32X) = K32X. The GPU test allows 4 K32E for the exposure gradient and 4 K32X for loss and sample gradients, as
the other loss tests allow 4 K32: the device's powf and expf are ocml's, a few ulp from numpy's. These tolerances come
from float32 reference arithmetic, never from the kernel's output.

One image is held at exposure 0 (image 1). The batch's 300 rays reach all three images; its first 129 and fewer (the
GPU test's smaller ray counts) leave image 2 without a ray, which is the case of an accumulator that must keep its bits.
"""
import contextlib
import copy
import ctypes as ct
import functools
import os

import numpy as np
import pytest

import test_nerf_loss_host as H
from test_nerf_depth_host import _geometry, _loss32
from test_nerf_loss_host import (ACT_EXP, ACT_NONE, DT_SPAN, F32, K32, LINEAR_KNEE, MARGIN_HUBER, MARGIN_KNEE, MARGIN_SIGN, MASKED,
                                 MIN_STEP, SIGN_LOSSES, SRGB_KNEE, batches, cfg_values, in_units, linear_to_srgb, make_cfg,
                                 srgb_to_linear)

lit = H.C
LN2 = lit(0.6931471805599453)
K32E = 0.45
K32X = 0.35
HELD_IMAGE = 1                                       # its exposure stays 0
DERIV_LOW = float(F32(1.0) / F32(12.92))             # 1.0f / 12.92f and 2.4f / 1.055f, as the compiler folds them
DERIV_GAIN = float(F32(2.4) / F32(1.055))
NGP_INVALID = -2


def exposure_configs(pkg):
    """The configurations the exposure tests run: the three colour spaces, the two losses and activation pairs."""
    return [("Huber Exp/Exp sRGB", make_cfg(pkg, "Huber", ACT_EXP, ACT_EXP, linear_colors=0, color_space_linear=0)),
            ("L2 None/None linear", make_cfg(pkg, "L2", ACT_NONE, ACT_NONE, linear_colors=1, color_space_linear=0)),
            ("Huber Exp/Exp color_space_linear", make_cfg(pkg, "Huber", ACT_EXP, ACT_EXP, linear_colors=0, color_space_linear=1))]


def draw_exposures(seed, n_images=3):
    """Seeded log2 exposures per image and channel from [-1, 1], image HELD_IMAGE at 0."""
    e = np.random.default_rng(4000 + seed).uniform(-1.0, 1.0, (n_images, 3)).astype(F32)
    e[HELD_IMAGE] = 0.0
    return e


def srgb_to_linear_derivative(s):
    with np.errstate(invalid="ignore"):
        return np.where(s <= SRGB_KNEE, DERIV_LOW, DERIV_GAIN * ((np.maximum(s, 0) + lit(0.055)) / lit(1.055)) ** lit(1.4))


def ray_texels(pixels, px, n):
    """Every ray's image and RGBA8 texel (read_rgba's index, as restate_loss takes it)."""
    img, uv = np.asarray(px["img"]).astype(np.int64)[:n], np.asarray(px["uv"], F32)[:n]
    texel = np.zeros((n, 4), np.int64)
    for i in range(n):
        h, w = pixels[img[i]].shape[:2]
        x = min(max(int(F32(uv[i, 0]) * F32(w)), 0), w - 1)
        y = min(max(int(F32(uv[i, 1]) * F32(h)), 0), h - 1)
        texel[i] = pixels[img[i]][y, x]
    return img, texel


def exposure_target(pixels, px, v, background, exposure, n):
    """The target with exposure in float64 (testbed_nerf.cu:1794-1818): {target, target_c (companion), knee (distance of
    every linear_to_srgb argument from its knee), tex (the premultiplied linear texel, unscaled), scale, img}."""
    img, texel = ray_texels(pixels, px, n)
    e = np.asarray(exposure, F32).astype(np.float64)[img]                                     # [n, 3]
    scale = np.exp(LN2 * e)
    masked = (texel == np.array(MASKED)).all(axis=1)
    a8 = texel[:, 3:4] / 255.0
    tex = np.where(masked[:, None], -1.0, srgb_to_linear(texel[:, :3] / 255.0) * a8)
    tex_a = np.where(masked[:, None], -1.0, a8)
    bg_srgb = np.asarray(background, np.float64)[:n] if v["random_bg_color"] else np.broadcast_to(v["background_color"], (n, 3))
    bg = srgb_to_linear(bg_srgb)
    lin = scale * tex
    mag = np.abs(lin) + np.abs((1.0 - tex_a) * bg)
    knee = np.full(n, np.inf)

    def to_srgb(l):
        nonlocal knee
        knee = np.minimum(knee, np.abs(l - LINEAR_KNEE).min(axis=1))
        return linear_to_srgb(l)
    if v["linear_colors"]:
        target = lin + (1.0 - tex_a) * bg
    elif v["color_space_linear"]:
        target = to_srgb(lin + (1.0 - tex_a) * bg)
    else:
        bg = to_srgb(bg)
        pos = tex_a > 0
        straight = np.where(pos, lin / np.where(pos, tex_a, 1.0), 1.0)
        target = np.where(pos, to_srgb(straight) * tex_a + (1.0 - tex_a) * bg, bg)
    # restate_loss allows 8 roundings for the two powf behind the target; the exponential of a rounded product and the
    # product with the texel add 3 |ln2 e| + 4
    target_c = (8 + 3 * np.abs(LN2 * e) + 4) * (np.abs(target) + mag)
    return {"target": target, "target_c": target_c, "knee": knee, "tex": tex, "scale": scale, "img": img, "e": e}


@contextlib.contextmanager
def loss_sees_target(target, target_c):
    """While this runs, restate_loss' loss and its companion are evaluated at `target` (module docstring). Yields a dict
    that receives the loss gradient's companion, which restate_loss does not return."""
    lc, lcc = H.loss_channel, H.loss_channel_companion
    seen = {}

    def loss_channel(_, pred, kind, den_pred=None):
        return lc(target, pred, kind, den_pred)

    def loss_channel_companion(_, pred, kind, d_c, pred_c, t_c):
        out = lcc(target, pred, kind, pred_c + target_c + np.abs(pred - target), pred_c, target_c)
        seen["gradient_c"] = out[1]
        return out
    H.loss_channel, H.loss_channel_companion = loss_channel, loss_channel_companion
    try:
        yield seen
    finally:
        H.loss_channel, H.loss_channel_companion = lc, lcc


def restate_loss_exposure(batch, cfg, exposure, mean_density=0.003, max_compacted=1 << 14, n_rays=None, counter=None, px=None,
                          uv_pdf=None, loss_scale=128.0, sign=-1.0, ln2=LN2, **kw):
    """restate_loss at the exposed target, plus the exposure gradient: exp_ray [n, 3] and its companion exp_ray_c, counted
    (the rays whose gradient enters a sum), and per image exp_img [n_images, 3], exp_img_abs (sum of |term|), exp_img_c
    (sum of companions) and exp_img_n (rays counted). uv_pdf [n]: the pixels' pdf under CDFs (default 1). sign, ln2: the
    expression's sign and its ln 2, for the negative controls."""
    v = cfg if isinstance(cfg, dict) else cfg_values(cfg)
    n = batch.n_rays if n_rays is None else n_rays
    px = batch.px if px is None else px
    t = exposure_target(batch.pixels, px, v, batch.background, exposure, n)
    target, target_c = t["target"], t["target_c"]
    with loss_sees_target(target, target_c) as seen:
        ref = H.restate_loss(batch.samples(n, counter), batch.out(v["density_activation"]), batch.pixels, px, v, mean_density,
                             loss_scale, max_compacted, n, background=batch.background, **kw)
    pred = ref["pred"]
    d = pred - target
    _, gc = H.loss_channel(target, pred, v["loss_type"])
    gc_c = seen["gradient_c"]
    uvp = np.ones(n) if uv_pdf is None else np.asarray(uv_pdf, F32).astype(np.float64)[:n]
    q = sign * gc / uvp[:, None]
    q_c = gc_c / uvp[:, None] + np.abs(q)
    deriv_knee = np.full(n, np.inf)
    if not v["linear_colors"]:
        sld = srgb_to_linear_derivative(target)
        curved = target > SRGB_KNEE
        sld_c = np.where(curved, sld * (lit(1.4) * target_c / (np.abs(target) + lit(0.055)) + 5), 0.0)
        q, q_c = q / sld, q_c / sld + np.abs(q / sld) * sld_c / sld + np.abs(q / sld)
        deriv_knee = np.abs(target - SRGB_KNEE).min(axis=1)
    ls = loss_scale / n
    scale = t["scale"]
    g = ls * q * scale * ln2
    g_c = ls * ln2 * (q_c * scale + np.abs(q) * scale * (3 * np.abs(LN2 * t["e"]) + 2)) + 4 * np.abs(g)
    counted = ref["cnum"] > 0
    n_images = len(batch.pixels)
    img_sum, img_abs, img_c = np.zeros((n_images, 3)), np.zeros((n_images, 3)), np.zeros((n_images, 3))
    np.add.at(img_sum, t["img"][counted], g[counted])
    np.add.at(img_abs, t["img"][counted], np.abs(g[counted]))
    np.add.at(img_c, t["img"][counted], g_c[counted])
    ref.update(target=target, exp_ray=g, exp_ray_c=g_c, counted=counted, exp_img=img_sum, exp_img_abs=img_abs, exp_img_c=img_c,
               exp_img_n=np.bincount(t["img"][counted], minlength=n_images), tex=t["tex"], exposure_scale=scale, loss_gradient=gc,
               loss_gradient_c=gc_c,
               exposure_margins={"huber": np.abs(np.abs(d) - lit(0.1)).min(axis=1), "sign": np.abs(d).min(axis=1),
                                 "srgb_knee": t["knee"], "deriv_knee": deriv_knee})
    return ref


def pixel_margins_hold(batch, cfgs, exposure, px=None):
    """The decisions that depend on the ray's pixel and exposure alone (redrawing a ray's samples cannot move them): the
    two knees of the sRGB curve, over the rays with a sample."""
    for cfg in cfgs:
        ref = restate_loss_exposure(batch, cfg, exposure, px=px)
        m, alive = ref["exposure_margins"], ref["cn"] > 0
        if min(m["srgb_knee"][alive].min(), m["deriv_knee"][alive].min()) < MARGIN_KNEE:
            return False
    return True


def exposure_violations(batch, cfg, exposure, px=None):
    """Rays within a margin of Huber's knee or of the sign of pred - target, with exposure applied."""
    ref = restate_loss_exposure(batch, cfg, exposure, px=px)
    m, lt = ref["exposure_margins"], (cfg if isinstance(cfg, dict) else cfg_values(cfg))["loss_type"]
    bad = np.zeros(ref["cn"].size, bool)
    if lt == 4:
        bad |= m["huber"] < MARGIN_HUBER
    if lt in SIGN_LOSSES:
        bad |= m["sign"] < MARGIN_SIGN
    return np.nonzero(bad & (ref["cn"] > 0))[0]


@functools.lru_cache(maxsize=None)
def _exposure_world(pkg):
    """A copy of the 300-ray batch (the other files' batch stays as it is) and the exposures: the first seed whose
    exposed targets keep clear of both sRGB knees, then every ray redrawn until it is clear of the other decisions, with
    exposure and without (the zero-exposure comparisons run on the same batch)."""
    _, full, _, _ = batches(pkg)
    mine = copy.copy(full)
    for name in ("attempt", "rays", "coords", "sigma_dt", "rgb_raw"):
        setattr(mine, name, getattr(full, name).copy())
    cfgs = [c for _, c in exposure_configs(pkg)]
    for seed in range(50):
        exposure = draw_exposures(seed)
        if pixel_margins_hold(mine, cfgs, exposure):
            break
    else:
        raise AssertionError("no exposure seed keeps the targets clear of the sRGB knees")
    for _ in range(20):
        bad = set()
        for cfg in cfgs:
            bad |= set(int(r) for r in exposure_violations(mine, cfg, exposure))
            bad |= set(int(r) for r in mine.violations(cfg))
        if not bad:
            return mine, exposure, seed
        for r in sorted(bad):
            mine.attempt[r] += 1
            mine._draw_ray(r)
    raise AssertionError("rays within a decision margin after every redraw")


def exposure_world(pkg):
    """(batch, exposures [3, 3] float32, the exposures' seed)."""
    return _exposure_world(pkg)


def exposure_gradient_f32(batch, cfg, exposure, ref):
    """The per-ray exposure gradient and the loss gradient in numpy float32, every operation in k_loss_pass1's order, for
    a fixed background and the None / Exponential activations; the stop decisions are ref's."""
    f = F32
    v = cfg_values(cfg)
    assert not v["random_bg_color"]
    n = batch.n_rays
    s = batch.samples()
    ns, base, M, valid, idx = _geometry(s, n)
    o = batch.out(v["density_activation"])[:, :4].astype(f)[idx]
    dt = s["coords"].astype(f)[idx, 3] * f(DT_SPAN) + f(MIN_STEP)
    ra, da = v["rgb_activation"], v["density_activation"]
    assert ra in (ACT_NONE, ACT_EXP) and da in (ACT_NONE, ACT_EXP)
    rgb = o[..., :3] if ra == ACT_NONE else np.exp(np.clip(o[..., :3], f(-10), f(10)))
    sigma = o[..., 3] if da == ACT_NONE else np.exp(o[..., 3])
    alpha = f(1.0) - np.exp(-sigma * dt)
    T, acc = np.ones(n, f), np.zeros((n, 3), f)
    for j in range(M):
        u = ref["upd"][:, j]
        w = alpha[:, j] * T
        new_acc, new_T = acc + w[:, None] * rgb[:, j], T * (f(1.0) - alpha[:, j])
        acc, T = np.where(u[:, None], new_acc, acc), np.where(u, new_T, T)
    assert acc.dtype == f and T.dtype == f
    img, texel = ray_texels(batch.pixels, batch.px, n)
    masked = (texel == np.array(MASKED)).all(axis=1)

    def to_linear(x):
        with np.errstate(invalid="ignore"):
            return np.where(x <= f(0.04045), x / f(12.92), np.power((x + f(0.055)) / f(1.055), f(2.4))).astype(f)

    def to_srgb(l):
        with np.errstate(invalid="ignore"):
            return np.where(l < f(0.0031308), f(12.92) * l, f(1.055) * np.power(l, f(0.41666)) - f(0.055)).astype(f)
    a8 = texel[:, 3:4].astype(f) * f(1.0 / 255.0)
    texc = np.where(masked[:, None], f(-1.0), to_linear(texel[:, :3].astype(f) * f(1.0 / 255.0)) * a8).astype(f)
    tex3 = np.where(masked[:, None], f(-1.0), a8).astype(f)
    bgc = to_linear(np.broadcast_to(v["background_color"].astype(f), (n, 3)))
    es = np.exp(f(LN2) * np.asarray(exposure, f)[img])
    assert es.dtype == f
    if v["linear_colors"] or v["color_space_linear"]:
        target = es * texc + (f(1.0) - tex3) * bgc
        if not v["linear_colors"]:
            target, bgc = to_srgb(target), to_srgb(bgc)
    else:
        bgc = to_srgb(bgc)
        pos = tex3 > 0
        with np.errstate(invalid="ignore", divide="ignore"):
            target = np.where(pos, to_srgb(es * texc / np.where(pos, tex3, f(1.0))) * tex3 + (f(1.0) - tex3) * bgc, bgc).astype(f)
    kept_all = ref["cn"] == ns
    pred = np.where(kept_all[:, None], acc + T[:, None] * bgc, acc).astype(f)
    _, gc = _loss32(target, pred, v["loss_type"])
    dgt = -gc
    if not v["linear_colors"]:
        with np.errstate(invalid="ignore"):
            sld = np.where(target <= f(0.04045), f(1.0) / f(12.92),
                           f(2.4) / f(1.055) * np.power((target + f(0.055)) / f(1.055), f(1.4))).astype(f)
        dgt = dgt / sld
    g = (f(128.0) / f(n)) * dgt * es * f(LN2)
    assert g.dtype == f and gc.dtype == f
    return g, gc


# ---- CPU tests -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pkg():
    from __graft_entry__ import load_package
    return load_package()


def test_batch_margins_hold_with_exposure_applied(pkg):
    """Under every configuration the exposure tests run, with the exposures applied: no ray with a sample within a margin
    of Huber's knee, of the sign of pred - target, or of either knee of the sRGB curve (the scaled target can cross one
    where the unscaled target does not), and none within the module's own margins; so no comparison leaves a ray out.
    The exposures are spread over about +-1, one image stays at 0, and image 2 has no ray among the first 129."""
    mine, exposure, seed = exposure_world(pkg)
    assert not exposure[HELD_IMAGE].any() and np.abs(exposure).max() > 0.5 and (exposure < 0).any() and (exposure > 0).any()
    moved = 0
    for label, cfg in exposure_configs(pkg):
        assert exposure_violations(mine, cfg, exposure).size == 0 and mine.violations(cfg).size == 0, label
        assert pixel_margins_hold(mine, [cfg], exposure), label
        ref = restate_loss_exposure(mine, cfg, exposure)
        base = mine.reference(cfg)
        moved += int((np.abs(ref["target"] - base["target"]).max(axis=1) > 1e-3).sum())
        assert (ref["exp_img_n"] > 20).all() and ref["counted"].sum() > 200
    assert moved > 300
    px_img = np.asarray(mine.px["img"])
    assert set(px_img[:129]) == {0, 1} and set(px_img) == {0, 1, 2}
    print(f"exposure seed {seed}: {exposure.tolist()}")


def test_zero_exposures_reproduce_restate_loss(pkg):
    mine, _, _ = exposure_world(pkg)
    zero = np.zeros((3, 3), F32)
    for label, cfg in exposure_configs(pkg):
        for kw in ({}, {"max_compacted": 40}, {"counter": 211}, {"n_rays": 17}):
            ref, base = restate_loss_exposure(mine, cfg, zero, **kw), mine.reference(cfg, **kw)
            for key in ("loss", "grad", "pred", "target", "numsteps", "cnum", "coords_compacted", "mean_loss"):
                np.testing.assert_array_equal(ref[key], base[key], err_msg=f"{label} {key}")
            assert ref["compacted_counter"] == base["compacted_counter"]


def test_counted_rays_follow_the_compaction(pkg):
    """A ray past the ray counter or cut to no sample by the compacted budget enters no sum; a ray cut to part of its
    samples does."""
    mine, exposure, _ = exposure_world(pkg)
    cfg = exposure_configs(pkg)[0][1]
    cases = H.compaction_cases(mine, make_cfg(pkg))
    r = restate_loss_exposure(mine, cfg, exposure, max_compacted=cases[1][0])
    cut = np.nonzero((r["cnum"] > 0) & (r["cnum"] < r["cn"]))[0]
    assert cut.size == 1 and r["counted"][cut[0]] and not r["counted"][cut[0] + 1:].any()
    r = restate_loss_exposure(mine, cfg, exposure, counter=211)
    assert not r["counted"][211:].any() and r["counted"][:211].sum() > 150
    full = restate_loss_exposure(mine, cfg, exposure)
    assert np.abs(r["exp_img"][2]).max() < np.abs(full["exp_img"][2]).max()


def _central_difference(pkg, mine, exposure, cfg, **kw):
    """max over rays of |3 loss_scale d(loss_i)/d(e[img_i, ch]) - gradient * texel| / the ray's largest |gradient * texel|."""
    Hs = 1e-6
    ref = restate_loss_exposure(mine, cfg, exposure, **kw)
    e64 = exposure.astype(np.float64)
    worst = 0.0
    for ch in range(3):
        lp, lm = [], []
        for s_, out in ((+1, lp), (-1, lm)):
            e = e64.copy()
            e[:, ch] += s_ * Hs
            t = _exposed_loss(mine, cfg, e)
            out.append(t)
        fd = 3 * 128.0 * (lp[0] - lm[0]) / (2 * Hs)
        analytic = ref["exp_ray"] * ref["tex"]
        scale = np.abs(analytic).max(axis=1)
        ok = ref["counted"] & (scale > 0)
        worst = max(worst, float((np.abs(fd - analytic[:, ch])[ok] / scale[ok]).max()))
    return worst


def _exposed_loss(mine, cfg, e64):
    """restate_loss' per-ray loss at float64 exposures (exposure_target with its float32 rounding bypassed)."""
    v = cfg_values(cfg)
    n = mine.n_rays
    img, texel = ray_texels(mine.pixels, mine.px, n)
    a8 = texel[:, 3:4] / 255.0
    masked = (texel == np.array(MASKED)).all(axis=1)
    tex = np.where(masked[:, None], -1.0, srgb_to_linear(texel[:, :3] / 255.0) * a8)
    tex_a = np.where(masked[:, None], -1.0, a8)
    bg = srgb_to_linear(np.broadcast_to(v["background_color"], (n, 3)))
    assert v["linear_colors"]
    target = np.exp(LN2 * e64[img]) * tex + (1.0 - tex_a) * bg
    with loss_sees_target(target, np.abs(target)):
        return H.restate_loss(mine.samples(), mine.out(v["density_activation"]), mine.pixels, mine.px, v, 0.003, 128.0, 1 << 14, n,
                              background=mine.background)["loss"]


def test_gradient_times_texel_is_the_derivative_of_the_loss(pkg):
    """The missing factor: in linear colours, gradient * (premultiplied linear) texel equals the central difference
    (step 1e-6) of 3 loss_scale loss_i with respect to the exposure of the ray's image, channel by channel (3 because
    the reference divides the loss by 3 and not the gradient; loss_i already holds 1 / n_rays). Every ray with a sample,
    whatever its texel's alpha (alpha 1 among them). Bound: 1e-6 of the ray's largest |gradient * texel|, as the module's
    own central-difference test sets it (the differences' truncation error is h^2 ~ 1e-12 relative, their rounding
    2^-53 / h ~ 1e-10); L2 and Huber (symmetric losses, the reference's assumption)."""
    mine, exposure, _ = exposure_world(pkg)
    alpha1 = 0
    for loss in ("L2", "Huber"):
        cfg = make_cfg(pkg, loss, ACT_NONE, ACT_NONE, linear_colors=1, color_space_linear=0)
        assert exposure_violations(mine, cfg, exposure).size == 0
        e = _central_difference(pkg, mine, exposure, cfg)
        print(f"{loss}: worst |fd - gradient * texel| / max = {e:.2e}")
        assert e <= 1e-6
    _, texel = ray_texels(mine.pixels, mine.px, mine.n_rays)
    alpha1 = int((texel[:, 3] == 255).sum())
    assert alpha1 > 30


def test_central_differences_see_a_wrong_sign_or_a_dropped_ln2(pkg):
    mine, exposure, _ = exposure_world(pkg)
    cfg = make_cfg(pkg, "L2", ACT_NONE, ACT_NONE, linear_colors=1, color_space_linear=0)
    for kw in ({"sign": 1.0}, {"ln2": 1.0}):
        e = _central_difference(pkg, mine, exposure, cfg, **kw)
        print(f"{kw}: {e:.2e}")
        assert e > 1e-1


def test_float32_restatement_measures_k32e(pkg):
    """K32E (module docstring): float32 against float64, the per-ray exposure gradient in units of 2^-24 companion over
    the rays that are counted, every configuration; and K32X, the loss gradient at the exposed target in units of its
    own companion, the constant the sample gradients' bound uses."""
    mine, exposure, _ = exposure_world(pkg)
    worst = worst_g = 0.0
    for label, cfg in exposure_configs(pkg):
        ref = restate_loss_exposure(mine, cfg, exposure)
        g32, gc32 = exposure_gradient_f32(mine, cfg, exposure, ref)
        c = ref["counted"]
        u = in_units(np.abs(g32.astype(np.float64) - ref["exp_ray"])[c], ref["exp_ray_c"][c])
        ug = in_units(np.abs(gc32.astype(np.float64) - ref["loss_gradient"])[c], ref["loss_gradient_c"][c])
        print(f"{label}: exposure gradient {u.max():.3f}, loss gradient {ug.max():.3f} units of 2^-24 companion")
        worst, worst_g = max(worst, float(u.max())), max(worst_g, float(ug.max()))
        assert np.isfinite(u).all() and u.max() <= K32E and ug.max() <= K32X, label
    print(f"K32E: float32 vs float64, exposure gradient {worst:.3f} (constant K32E = {K32E}); loss gradient {worst_g:.3f} (K32X = {K32X})")
    assert worst > K32E - 0.05 and worst_g > K32X - 0.05 and K32X >= K32   # the measured worst rounded up to the next 0.05


# ---- the host optimisers ---------------------------------------------------------------------------------------------------
def adam_reference(grads, n_between, l2, lrs, n_images):
    """Testbed::train_nerf's exposure update (testbed_nerf.cu:3831-3858) over AdamOptimizer<vec3> (adam_optimizer.h) in
    float64: beta1 0.9, beta2 0.99, epsilon 1e-8, the mean over the images removed after every step."""
    b1, b2, eps = lit(0.9), lit(0.99), lit(1e-8)
    m1, m2, var = np.zeros((n_images, 3)), np.zeros((n_images, 3)), np.zeros((n_images, 3))
    history = []
    for it, (g, lr) in enumerate(zip(grads, lrs), 1):
        grad = g.astype(np.float64) * (n_images / 128.0 / n_between) + l2 * var
        m1 = b1 * m1 + (1 - b1) * grad
        m2 = b2 * m2 + (1 - b2) * grad * grad
        var = var - lr * np.sqrt(1 - b2 ** it) / (1 - b1 ** it) * m1 / (np.sqrt(m2) + eps)
        var = var - var.mean(axis=0)
        history.append(var.copy())
    return history, m1, m2


def test_host_optimiser_matches_adam_with_the_mean_removed(pkg):
    """300 random steps of 7 images against the float64 restatement. Bound on a variable after k steps: 8 k 2^-24
    max(1, |variable|): a step rounds each of its ~8 float32 operations once, relative to values that stay below 1 here.
    After every step the per-channel mean is zero to the rounding of the subtraction, n 2^-24 max|variable|."""
    n, steps = 7, 300
    g = np.random.default_rng(12)
    opt = pkg.nerf.ExposureOptimizer(n)
    assert pkg.lib().ngp_exposure_optimizer_n_images(opt.handle) == n
    st0 = opt.get(3)
    assert st0["iter"] == 0 and st0["learning_rate"] == float(F32(1e-3)) and (st0["beta1"], st0["beta2"]) == (float(F32(0.9)), float(F32(0.99)))
    assert st0["epsilon"] == float(F32(1e-8)) and not any(st0["variable"]) and not any(st0["first_moment"])
    grads = [(g.standard_normal((n, 3)) * 10 ** g.uniform(-3, 1)).astype(F32) for _ in range(steps)]
    lrs = [float(F32(1e-2 * 0.99 ** k)) for k in range(steps)]
    want, m1, m2 = adam_reference(grads, 16, float(F32(1e-3)), lrs, n)
    for k in range(steps):
        opt.step(grads[k], n_steps_between=16, l2_reg=1e-3, network_lr=lrs[k])
        got = np.array([opt.get(i)["variable"] for i in range(n)], np.float64)
        assert np.abs(got.mean(axis=0)).max() <= n * 2.0 ** -24 * max(np.abs(got).max(), 1e-30)
        assert np.abs(got).max() < 1.0
        bound = 8 * (k + 1) * 2.0 ** -24 * np.maximum(1.0, np.abs(want[k]))
        assert (np.abs(got - want[k]) <= bound).all(), (k, np.abs(got - want[k]).max())
    st = opt.get(2)
    assert st["iter"] == steps and st["learning_rate"] == lrs[-1]
    np.testing.assert_allclose(st["first_moment"], m1[2], rtol=1e-4, atol=1e-9)
    np.testing.assert_allclose(st["second_moment"], m2[2], rtol=1e-4, atol=1e-12)
    # a wrong rule is seen: without the mean subtraction the first step already differs by more than the bound
    raw = -lrs[0] * np.sign(grads[0].astype(np.float64))
    assert np.abs(raw - want[0]).max() > 1e-4


def state_key(st):
    """An optimiser state dict as a comparable tuple (its vectors by their bits)."""
    return tuple((k, v.tobytes() if isinstance(v, np.ndarray) else v) for k, v in sorted(st.items()))


def test_host_optimiser_zero_gradient_reset_and_state(pkg):
    n = 5
    opt = pkg.nerf.ExposureOptimizer(n)
    for _ in range(3):
        opt.step(np.zeros((n, 3), F32), n_steps_between=4, l2_reg=0.0, network_lr=1e-2)
    for i in range(n):
        st = opt.get(i)
        assert st["iter"] == 3 and not any(st["variable"]) and not any(st["first_moment"]) and not any(st["second_moment"])
    g = np.random.default_rng(3).standard_normal((n, 3)).astype(F32)
    opt.step(g, n_steps_between=4, l2_reg=0.0, network_lr=1e-2)
    before = [opt.get(i) for i in range(n)]
    assert all(any(b["variable"]) for b in before)
    opt.reset_one(2)
    after = [opt.get(i) for i in range(n)]
    assert after[2]["iter"] == 0 and not any(after[2]["variable"]) and not any(after[2]["second_moment"])
    assert after[2]["learning_rate"] == before[2]["learning_rate"]       # reset_state keeps the hyperparameters
    assert all(state_key(after[i]) == state_key(before[i]) for i in range(n) if i != 2)
    # get / set_state round-trips every member
    other = pkg.nerf.ExposureOptimizer(n)
    for i in range(n):
        other.set_state(i, after[i])
    assert [state_key(other.get(i)) for i in range(n)] == [state_key(a) for a in after]
    opt.step(g, n_steps_between=4, l2_reg=0.5, network_lr=3e-3)
    other.step(g, n_steps_between=4, l2_reg=0.5, network_lr=3e-3)
    assert [state_key(other.get(i)) for i in range(n)] == [state_key(opt.get(i)) for i in range(n)]
    opt.reset()
    assert all(opt.get(i)["iter"] == 0 and not any(opt.get(i)["variable"]) for i in range(n))


# ---- the C-ABI without a GPU ---------------------------------------------------------------------------------------------
NEW_SYMBOLS = ("ngp_nerf_compute_loss_exposure", "ngp_exposure_optimizer_create", "ngp_exposure_optimizer_n_images",
               "ngp_exposure_optimizer_reset", "ngp_exposure_optimizer_reset_one", "ngp_exposure_optimizer_step",
               "ngp_exposure_optimizer_get", "ngp_exposure_optimizer_set_state", "ngp_nerf_trainer_set_exposure_training",
               "ngp_nerf_trainer_get_exposure_training", "ngp_nerf_trainer_camera_exposure", "ngp_nerf_trainer_set_camera_exposure",
               "ngp_nerf_trainer_exposure_optimizer_state")


def test_exposure_symbols_exist(pkg):
    L = pkg.lib()
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "ngp_engine.h")).read()
    for name in NEW_SYMBOLS:
        assert getattr(L, name) is not None
        assert f"{name}(" in header
    assert L.ngp_exposure_optimizer_destroy is not None


def test_exposure_arguments_are_checked_before_any_gpu_call(pkg):
    L = pkg.lib()
    three = np.zeros(3, np.float32)
    from instant_ngp_amd._capi import AdamState
    st = AdamState()
    # a NULL trainer, with good and with bad values
    for on, reg in ((1, 0.0), (0, -1.0), (1, float("nan")), (1, float("inf"))):
        assert L.ngp_nerf_trainer_set_exposure_training(None, on, reg) == NGP_INVALID
    assert L.ngp_nerf_trainer_get_exposure_training(None, None, None) == NGP_INVALID
    assert L.ngp_nerf_trainer_camera_exposure(None, 0, three.ctypes.data) == NGP_INVALID
    assert L.ngp_nerf_trainer_set_camera_exposure(None, 0, three.ctypes.data) == NGP_INVALID
    assert L.ngp_nerf_trainer_exposure_optimizer_state(None, 0, ct.byref(st)) == NGP_INVALID
    # the optimisers: no images, a NULL handle, an image index out of range, a negative l2, no steps between
    h = ct.c_void_p()
    assert L.ngp_exposure_optimizer_create(0, ct.byref(h)) == NGP_INVALID and L.ngp_exposure_optimizer_create(3, None) == NGP_INVALID
    assert L.ngp_exposure_optimizer_n_images(None) == 0 and L.ngp_exposure_optimizer_reset(None) == NGP_INVALID
    opt = pkg.nerf.ExposureOptimizer(3)
    assert L.ngp_exposure_optimizer_get(opt.handle, 3, ct.byref(st)) == NGP_INVALID
    assert L.ngp_exposure_optimizer_set_state(opt.handle, 3, ct.byref(st)) == NGP_INVALID
    assert L.ngp_exposure_optimizer_reset_one(opt.handle, 3) == NGP_INVALID
    g = np.zeros((3, 3), np.float32)
    assert L.ngp_exposure_optimizer_step(opt.handle, g.ctypes.data, 16, -1.0, 1e-2) == NGP_INVALID
    assert L.ngp_exposure_optimizer_step(opt.handle, g.ctypes.data, 0, 0.0, 1e-2) == NGP_INVALID
    assert L.ngp_exposure_optimizer_step(opt.handle, None, 16, 0.0, 1e-2) == NGP_INVALID
    assert "exposure optimizer" in pkg.lib().ngp_last_error().decode()
    assert opt.get(0)["iter"] == 0
    # the entry point with every pointer NULL
    cfg = pkg.nerf.default_config(1.0)
    rc = L.ngp_nerf_compute_loss_exposure(None, ct.byref(cfg), None, 4, 4, pkg.nerf.pcg32(1), 16, None, None, None, None, None, None,
                                          None, None, None, None, None, 128.0, None, 0, 0, None, None, 0, 0, 0, None, None, 0,
                                          0.0, 1, None, three.ctypes.data)
    assert rc == NGP_INVALID


def test_pyngp_exposure_knobs_without_a_trainer(pkg):
    """nerf.training.optimize_exposure / exposure_l2_reg are kept until there is a trainer; the pair with
    sample_image_proportional_to_error is refused either way round, the message names both switches and the state stays;
    sample_focal_plane_proportional_to_error is allowed."""
    tb = pkg.pyngp().Testbed()
    tr = tb.nerf.training
    assert tr.optimize_exposure is False and tr.exposure_l2_reg == 0.0
    tr.exposure_l2_reg = 0.25
    tr.optimize_exposure = True
    tr.sample_focal_plane_proportional_to_error = True
    assert tr.optimize_exposure is True and tr.exposure_l2_reg == 0.25 and tr.sample_focal_plane_proportional_to_error
    with pytest.raises(RuntimeError, match="optimize_exposure.*sample_image_proportional_to_error"):
        tr.sample_image_proportional_to_error = True
    assert not tr.sample_image_proportional_to_error
    tr.optimize_exposure = False
    tr.sample_image_proportional_to_error = True
    with pytest.raises(RuntimeError, match="optimize_exposure.*sample_image_proportional_to_error"):
        tr.optimize_exposure = True
    assert tr.optimize_exposure is False
    with pytest.raises(RuntimeError):
        tr.exposure_l2_reg = -1.0
    assert tr.exposure_l2_reg == 0.25
    np.testing.assert_array_equal(tr.get_camera_exposure(0), np.zeros(3, np.float32))


def test_synthetic_exposure_scales_the_linear_colours(pkg):
    """render(exposure=e): alpha and the empty pixels as without, exposure 0 within a byte of the plain image, and the
    linear colours of unclipped pixels 2^e times the plain ones to the bytes' quantisation."""
    S = pkg.synthetic
    c2w = S.camera_poses(3, seed=5)[1]
    plain = S.render(c2w, 32, 32)
    np.testing.assert_array_equal(plain, S.render(c2w, 32, 32, exposure=None))
    same = S.render(c2w, 32, 32, exposure=0.0)
    assert np.abs(same.astype(int) - plain.astype(int)).max() <= 1
    for e in (0.4, -0.4, (0.3, 0.0, -0.3)):
        img = S.render(c2w, 32, 32, exposure=e)
        np.testing.assert_array_equal(img[..., 3], plain[..., 3])
        lin0, lin1 = srgb_to_linear(plain[..., :3] / 255.0), srgb_to_linear(img[..., :3] / 255.0)
        ok = (plain[..., 3:] == 255) & (plain[..., :3] > 40) & (img[..., :3] < 250) & (plain[..., :3] < 250)
        ratio = (lin1 / np.where(ok, lin0, 1.0))
        want = np.broadcast_to(2.0 ** np.asarray(e, np.float64), ratio.shape)
        assert ok.sum() > 200 and np.abs(ratio / want - 1.0)[ok].max() < 0.05
