"""Depth supervision of the NeRF loss pass (testbed_nerf.cu:1725-1748, 1848-1856, 1912-1956) restated in float64 on top
of test_nerf_loss_host.py's restatement, the depth maps and margins the GPU test runs with (test_gpu_nerf_depth.py
imports them), and the CPU tests: margins, central differences, a float32 restatement, the C-ABI's argument checks
and the loader. No GPU call is made.

restate_loss_depth wraps restate_loss: the colour part is the existing restatement's; the depth part composites
depth_ray = sum weight * |pos - ray_o| under the colour pass's stop decisions, reads target_depth = |ray.d| * depth texel
(-|ray.d| for an image without depth), and adds lambda dL_depth/d(depth_ray) (T depth - depth suffix) inside dt (...) of
every compacted sample's density gradient where target_depth > 0. loss[] is untouched.

The companion (test_nerf_loss_host.py's rules: one rounding per operation, first-order propagation) is extended by the
depth term's running magnitude: a sample's distance carries its subtraction's cancellation (pos - ray_o), depth_ray and
its prefixes accumulate like the rgb prefix, target_depth counts 4 roundings (a length and a product), the depth loss goes
through loss_channel_companion, and brace = T depth - suffix and its product with the ray's gradient follow the colour
brace. The sum dot + depth term rounds once more.

K32D: the same arithmetic in numpy float32 (restate_density_gradient_f32: the compositing, the colour dot product of the
default colour space, the depth path, every operation rounded to float32 in the kernel's order) against the float64
restatement over every depth loss x {Huber Exp/Exp, L2 None/None} on the 300-ray batch is at most K32D = 0.20 units of
2^-24 companion: measured 0.165 on the density gradient before its rounding to fp16 (Huber Exp/Exp; 0.119 for L2
None/None), the same element with lambda 0 and with every depth loss, so the depth term's own error stays below the
colour part's. test_float32_restatement_measures_k32d prints it. The GPU test allows 4 K32D on top of half an fp16 ulp
and one flipped rounding, the form of test_gpu_nerf_loss.py.
"""
import copy
import ctypes as C
import functools
import json
import os

import numpy as np
import pytest

from test_nerf_loss_host import (ACT_EXP, ACT_NONE, DT_SPAN, F32, LOSS, MARGIN_HUBER, MARGIN_SIGN, MIN_STEP, SIGN_LOSSES,
                                 C as lit, batches, cfg_values, density_slope, density_value, in_units, loss_channel,
                                 loss_channel_companion, make_cfg, restate_loss, slope_companion)

K32D = 0.20
DEPTH_LAMBDA = 0.5
DEPTH_LOSSES = tuple(LOSS)
COLOUR_CONFIGS = (("Huber", ACT_EXP, ACT_EXP), ("L2", ACT_NONE, ACT_NONE))
MARGIN_TARGET = 5e-3       # a live target depth is at least this far above 0
U16_SCALE, F32_SCALE = 0.00005, 0.1


def depth_images(images, seed=77):
    """Per image (host pixels, scale) or None: image 0 uint16, image 1 float32, image 2 none. A pixel's value is a hash
    of (image, pixel index, seed): 35 % exactly 0 (no depth there), the rest 0.004 .. 0.124 after the scale (target depths 0.01 .. 0.31,
    around the batch's composited depths)."""
    out = []
    for m, im in enumerate(images):
        n = im.width * im.height
        h = (np.arange(n, dtype=np.uint64) * np.uint64(2654435761) + np.uint64(m * 40503 + seed) * np.uint64(97)) % np.uint64(1 << 32)
        h = (h ^ (h >> np.uint64(13))) * np.uint64(0x9E3779B1) % np.uint64(1 << 32)
        zero = (h >> np.uint64(8)) % np.uint64(100) < 35
        level = ((h >> np.uint64(12)) % np.uint64(2400)).astype(np.int64) + 80          # 80 .. 2479
        level = np.where(zero, 0, level).reshape(im.height, im.width)
        if m == 0:
            out.append((level.astype(np.uint16), U16_SCALE))
        elif m == 1:
            out.append(((level * 0.0005).astype(np.float32), F32_SCALE))
        else:
            out.append(None)
    return out


def stored_depth(maps):
    """What the dataset keeps: float32(pixel) * float32(scale), or None."""
    return [None if m is None else (m[0].astype(F32) * F32(m[1])).astype(F32) for m in maps]


def _geometry(s, n):
    ns_in = np.asarray(s["numsteps"]).astype(np.int64).reshape(-1, 2)[:n]
    active = np.arange(n) < min(int(s["counters"][0]), n)
    ns, base = np.where(active, ns_in[:, 0], 0), ns_in[:, 1]
    M = max(int(ns.max()) if n else 0, 1)
    valid = np.arange(M)[None, :] < ns[:, None]
    return ns, base, M, valid, np.where(valid, base[:, None] + np.arange(M)[None, :], 0)


def depth_targets(s, px, stored, lam, n):
    """target_depth per ray (float64 of the float32 inputs) and the texel's depth."""
    img, uv = np.asarray(px["img"]).astype(np.int64)[:n], np.asarray(px["uv"], F32)[:n]
    tex = np.full(n, -1.0)
    for i in range(n):
        d = stored[img[i]]
        if lam > 0 and d is not None:
            h, w = d.shape
            x = min(max(int(F32(uv[i, 0]) * F32(w)), 0), w - 1)
            y = min(max(int(F32(uv[i, 1]) * F32(h)), 0), h - 1)
            tex[i] = d[y, x]
    return np.linalg.norm(np.asarray(s["rays"]).astype(np.float64)[:n, 3:6], axis=1) * tex, tex


def composite_depth(s, out, v, upd, n):
    """depth_ray and what pass 2 needs of the compositing, in float64 with companions, under the stop decisions `upd`
    of the colour restatement. out: fp16 [N, >= 4] or float64 with leading axes (then only depth_ray is meaningful)."""
    ns, base, M, valid, idx = _geometry(s, n)
    o3 = np.asarray(out)[..., 3].astype(np.float64)[..., idx]
    coords = np.asarray(s["coords"]).astype(np.float64)
    dt = coords[idx, 3] * DT_SPAN + MIN_STEP
    sigma = density_value(o3, v["density_activation"])
    alpha = 1.0 - np.exp(-sigma * dt)
    box = v["aabb_max"] - v["aabb_min"]
    c3 = coords[idx, :3]
    pos = v["aabb_min"] + c3 * box
    diff = pos - np.asarray(s["rays"]).astype(np.float64)[:n, None, :3]
    depth = np.sqrt((diff * diff).sum(axis=-1))
    diff_c = np.abs(c3 * box) + np.abs(pos) + np.abs(diff)
    sq = (diff * diff).sum(axis=-1)
    depth_c = ((2 * np.abs(diff) * diff_c + diff * diff).sum(axis=-1) + 2 * sq) / (2 * np.maximum(depth, 1e-300)) + depth
    lead = o3.shape[:-2]
    T, T_c = np.ones(lead + (n,)), np.zeros(lead + (n,))
    acc, acc_c = np.zeros(lead + (n,)), np.zeros(lead + (n,))
    T_all, T_c_all = np.zeros(lead + (n, M)), np.zeros(lead + (n, M))
    pre_all, pre_c_all = np.zeros(lead + (n, M)), np.zeros(lead + (n, M))
    for j in range(M):
        u = np.broadcast_to(upd[:, j], T.shape)
        a = alpha[..., j]
        w = a * T
        x = sigma[..., j] * dt[:, j]
        a_c = np.exp(-x) * (3 * np.abs(x) + 2) + np.abs(a)
        w_c = a_c * np.abs(T) + np.abs(a) * T_c + np.abs(w)
        new_acc, new_T = acc + w * depth[:, j], T * (1.0 - a)
        new_acc_c = acc_c + w_c * depth[:, j] + np.abs(w) * depth_c[:, j] + np.abs(w * depth[:, j]) + np.abs(new_acc)
        new_T_c = T_c * np.abs(1.0 - a) + np.abs(T) * (a_c + np.abs(1.0 - a)) + np.abs(new_T)
        acc, acc_c = np.where(u, new_acc, acc), np.where(u, new_acc_c, acc_c)
        T, T_c = np.where(u, new_T, T), np.where(u, new_T_c, T_c)
        T_all[..., j], T_c_all[..., j], pre_all[..., j], pre_c_all[..., j] = T, T_c, acc, acc_c
    return {"depth_ray": acc, "depth_ray_c": acc_c, "T": T_all, "T_c": T_c_all, "prefix": pre_all, "prefix_c": pre_c_all,
            "depth": depth, "depth_c": depth_c, "dt": dt, "base": base}


def restate_loss_depth(batch, cfg, stored, lam, depth_loss, mean_density=0.003, max_compacted=1 << 14, n_rays=None, counter=None,
                       px=None, extra=None, **kw):
    """restate_loss plus the depth term. Returns restate_loss's dict with grad / grad_companion (density column) extended,
    and depth_ray, target_depth, depth_loss (per ray, where live), live, depth_margins. extra: keyword arguments of
    restate_loss's caller that change the colour part (the GPU test's CDF / environment map references pass a ready
    colour reference instead: extra={"ref": ...})."""
    v = cfg if isinstance(cfg, dict) else cfg_values(cfg)
    n = batch.n_rays if n_rays is None else n_rays
    s = batch.samples(n, counter)
    out = batch.out(v["density_activation"])
    px = batch.px if px is None else px
    if extra and "ref" in extra:
        ref = dict(extra["ref"])
    else:
        ref = restate_loss(s, out, batch.pixels, px, v, mean_density, 128.0, max_compacted, n, background=batch.background, **kw)
    kind = LOSS[depth_loss] if isinstance(depth_loss, str) else int(depth_loss)
    regularisers = kw.get("regularisers", True)
    c = composite_depth(s, out, v, ref["upd"], n)
    target, tex = depth_targets(s, px, stored, lam, n)
    dray, dray_c = c["depth_ray"], c["depth_ray_c"]
    target_c = 4 * np.abs(target)
    d_c = dray_c + target_c + np.abs(dray - target)
    ld, gd = loss_channel(target, dray, kind)
    _, gd_c = loss_channel_companion(target, dray, kind, d_c, dray_c, target_c)
    live = target > 0
    dlg = np.where(live, lam * gd, 0.0)
    dlg_c = np.where(live, lam * gd_c + np.abs(dlg), 0.0)
    ray, j = ref["ray"], ref["sample"]
    Tj, depj = c["T"][ray, j], c["depth"][ray, j]
    suffix = dray[ray] - c["prefix"][ray, j]
    suffix_c = dray_c[ray] + c["prefix_c"][ray, j] + np.abs(suffix)
    brace = Tj * depj - suffix
    brace_c = c["T_c"][ray, j] * depj + np.abs(Tj) * c["depth_c"][ray, j] + np.abs(Tj * depj) + suffix_c + np.abs(brace)
    dsup = dlg[ray] * brace
    dsup_c = dlg_c[ray] * np.abs(brace) + np.abs(dlg[ray]) * brace_c + np.abs(dsup)
    # the density column again: dot + dsup inside dt (...). What restate_loss put into its companion for the colour dot
    # product (ls dt slope dot_c) is recovered from its result; everything else is restated
    ls, dtj, oo = 128.0 / n, c["dt"][ray, j], ref["raw"]
    da = v["density_activation"]
    slope = density_slope(oo[:, 3], da)
    slope_c = slope_companion(oo[:, 3], da, slope)
    dot = ref["dmlp_unit"] / (ls * dtj)
    l1 = np.where(oo[:, 3] < 0, -lit(1e-4), 0.0) if (regularisers and float(F32(mean_density)) < lit(0.01)) else np.zeros(ray.size)
    near = np.where((oo[:, 3] > -10.0) & (ref["depth"] < v["near_distance"]), lit(1e-4), 0.0) if regularisers else np.zeros(ray.size)
    old3, old3_c = ref["grad"][:, 3], ref["grad_companion"][:, 3]
    colour_c = old3_c - ls * dtj * slope_c * np.abs(dot) - 5 * np.abs(ref["dmlp"]) - np.abs(l1) - np.abs(near) - 2 * np.abs(old3)
    tot = dot + dsup
    dmlp = slope * ls * dtj * tot
    grad, comp = ref["grad"].copy(), ref["grad_companion"].copy()
    grad[:, 3] = dmlp + l1 + near
    comp[:, 3] = (ls * dtj * (slope_c * np.abs(tot) + slope * (dsup_c + np.abs(tot))) + np.maximum(colour_c, 0.0) + 5 * np.abs(dmlp)
                  + np.abs(l1) + np.abs(near) + 2 * np.abs(grad[:, 3]))
    alive = live & (ref["cn"] > 0)
    dd = np.abs(dray - target)
    margins = {"target": np.where(alive, target, np.inf), "sign": np.where(alive, dd, np.inf),
               "huber": np.where(alive, np.abs(dd - lit(0.1)), np.inf)}
    ref.update(grad=grad, grad_companion=comp, dmlp=dmlp, depth_ray=dray, target_depth=target, depth_texel=tex, live=live,
               depth_loss=np.where(live, ld, 0.0), depth_term=slope * ls * dtj * dsup, depth_margins=margins,
               colour_grad=ref["grad"])
    return ref


def depth_violations(batch, cfg, stored, depth_loss):
    ref = restate_loss_depth(batch, cfg, stored, DEPTH_LAMBDA, depth_loss)
    m, kind = ref["depth_margins"], LOSS[depth_loss]
    bad = m["target"] < MARGIN_TARGET
    if kind == 4:
        bad |= m["huber"] < MARGIN_HUBER
    if kind in SIGN_LOSSES or kind == 4:   # Huber's outer branch takes d's sign
        bad |= m["sign"] < MARGIN_SIGN
    return np.nonzero(bad)[0]


def depth_configs(pkg):
    return [(dl, make_cfg(pkg, loss, r, d)) for dl in DEPTH_LOSSES for loss, r, d in COLOUR_CONFIGS]


@functools.lru_cache(maxsize=None)
def _depth_world(pkg):
    """The 300-ray batch (a copy: the other files' batch stays as it is) with every ray redrawn until it is away from
    the colour pass's decisions under every configuration those files run and from the depth decisions under
    depth_configs; the depth images; what the dataset stores of them."""
    groups, full, small, product = batches(pkg)
    mine = copy.copy(full)
    for name in ("attempt", "rays", "coords", "sigma_dt", "rgb_raw"):
        setattr(mine, name, getattr(full, name).copy())
    maps = depth_images(mine.images)
    stored = stored_depth(maps)
    every = [c for name in groups for _, c, _ in groups[name]]
    for _ in range(20):
        bad = set()
        for dl, cfg in depth_configs(pkg):
            bad |= set(int(r) for r in depth_violations(mine, cfg, stored, dl))
        for cfg in every:   # a redrawn ray must stay away from the colour pass's decisions too
            bad |= set(int(r) for r in mine.violations(cfg))
        if not bad:
            return mine, maps, stored
        for r in sorted(bad):
            mine.attempt[r] += 1
            mine._draw_ray(r)
    raise AssertionError("rays within a depth decision margin after every redraw")


def depth_world(pkg):
    return _depth_world(pkg)


# ---- the float32 restatement -------------------------------------------------------------------------------------------
def _loss32(target, pred, kind):
    """loss_channel of nerf_loss.hip in float32 arrays: (loss, gradient)."""
    f = F32
    d = pred - target
    one, ad = f(1.0), np.abs(d)
    sign = np.where(np.signbit(d), f(-1.0), f(1.0)).astype(f)
    if kind == 0:
        return d * d, f(2.0) * d
    if kind == 1:
        return ad, sign
    if kind == 2:
        den = np.abs(pred) + f(1e-2)
        return ad / den, sign * (one / den)
    if kind == 3:
        den = f(0.5) * (np.abs(pred) + np.abs(target)) + f(1e-2)
        return ad / den, sign * (one / den)
    if kind == 4:
        a = f(0.1)
        sq = f(0.5) / a * d * d
        return (np.where(ad > a, ad - f(0.5) * a, sq) / f(5.0)).astype(f), (np.where(ad > a, np.where(d > 0, one, -one), d / a) / f(5.0)).astype(f)
    if kind == 5:
        div = ad + one
        return np.log(div), sign * (one / div)
    den = pred * pred + f(1e-2)
    return d * d / den, f(2.0) * d / den


def restate_density_gradient_f32(batch, cfg, stored, lam, depth_loss, ref):
    """The density column of dloss_doutput in numpy float32, every operation in the kernel's order, for the default
    colour space (color_space_linear, not linear_colors), a fixed background and the Exponential / None activations;
    the stop decisions are ref's. Returns float32 [compacted rows] before the rounding to fp16."""
    f = F32
    v = cfg_values(cfg)
    assert v["color_space_linear"] and not v["linear_colors"] and not v["random_bg_color"]
    n = batch.n_rays
    s = batch.samples()
    ns, base, M, valid, idx = _geometry(s, n)
    o = batch.out(v["density_activation"])[:, :4].astype(f)[idx]          # [n, M, 4]
    coords = s["coords"].astype(f)
    dt = coords[idx, 3] * f(DT_SPAN) + f(MIN_STEP)
    ra, da = v["rgb_activation"], v["density_activation"]
    assert ra in (ACT_NONE, ACT_EXP) and da in (ACT_NONE, ACT_EXP)
    rgb = o[..., :3] if ra == ACT_NONE else np.exp(np.clip(o[..., :3], f(-10), f(10)))
    sigma = o[..., 3] if da == ACT_NONE else np.exp(o[..., 3])
    alpha = f(1.0) - np.exp(-sigma * dt)
    mn, mx = v["aabb_min"].astype(f), v["aabb_max"].astype(f)
    pos = mn + coords[idx, :3] * (mx - mn)
    diff = pos - s["rays"].astype(f)[:, None, :3]
    depth = np.sqrt(diff[..., 0] * diff[..., 0] + diff[..., 1] * diff[..., 1] + diff[..., 2] * diff[..., 2])
    T, acc, dd = np.ones(n, f), np.zeros((n, 3), f), np.zeros(n, f)
    w_all, T_all, pre_all, dpre_all = np.zeros((n, M), f), np.zeros((n, M), f), np.zeros((n, M, 3), f), np.zeros((n, M), f)
    for j in range(M):
        u = ref["upd"][:, j]
        w = alpha[:, j] * T
        new_acc, new_dd, new_T = acc + w[:, None] * rgb[:, j], dd + w * depth[:, j], T * (f(1.0) - alpha[:, j])
        acc, dd, T = np.where(u[:, None], new_acc, acc), np.where(u, new_dd, dd), np.where(u, new_T, T)
        w_all[:, j], T_all[:, j], pre_all[:, j], dpre_all[:, j] = w, T, acc, dd
    assert acc.dtype == f and dd.dtype == f and T.dtype == f
    # the target texel and the background (k_loss_pass1)
    img, uv = np.asarray(batch.px["img"]).astype(np.int64), np.asarray(batch.px["uv"], f)
    texel = np.zeros((n, 4), np.int64)
    for i in range(n):
        h, w_ = batch.pixels[img[i]].shape[:2]
        x = min(max(int(uv[i, 0] * f(w_)), 0), w_ - 1)
        y = min(max(int(uv[i, 1] * f(h)), 0), h - 1)
        texel[i] = batch.pixels[img[i]][y, x]
    masked = (texel == np.array((255, 0, 255, 0))).all(axis=1)

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
    target = to_srgb(texc + (f(1.0) - tex3) * bgc)
    bgc = to_srgb(bgc)
    kept_all = ref["cn"] == ns
    pred = np.where(kept_all[:, None], acc + T[:, None] * bgc, acc).astype(f)
    _, gc = _loss32(target, pred, v["loss_type"])
    # the depth path (k_loss_pass2)
    dirs = s["rays"].astype(f)[:, 3:6]
    length = np.sqrt(dirs[:, 0] * dirs[:, 0] + dirs[:, 1] * dirs[:, 1] + dirs[:, 2] * dirs[:, 2])
    tdepth = (length * ref["depth_texel"].astype(f)).astype(f)
    _, gd = _loss32(tdepth, dd, LOSS[depth_loss])
    dlg = np.where(tdepth > 0, f(lam) * gd, f(0.0)).astype(f)
    ray, j = ref["ray"], ref["sample"]
    my_t, c, dep = T_all[ray, j], rgb[ray, j], depth[ray, j]
    suffix = pred[ray] - pre_all[ray, j]
    g = gc[ray]
    dotv = g[:, 0] * (my_t * c[:, 0] - suffix[:, 0]) + g[:, 1] * (my_t * c[:, 1] - suffix[:, 1]) + g[:, 2] * (my_t * c[:, 2] - suffix[:, 2])
    dsup = dlg[ray] * (my_t * dep - (dd[ray] - dpre_all[ray, j]))
    o3 = o[ray, j, 3]
    slope = np.ones_like(o3) if da == ACT_NONE else np.exp(np.clip(o3, f(-15), f(15)))
    dmlp = slope * (dt[ray, j] * (dotv + dsup))
    l1 = np.where(o3 < 0, f(-1e-4), f(0.0)).astype(f)                     # mean density 0.003 < 0.01
    near = np.where((o3 > f(-10.0)) & (dep < f(v["near_distance"])), f(1e-4), f(0.0)).astype(f)
    out = (f(128.0) / f(n)) * dmlp + l1 + near
    assert out.dtype == f
    return out


# ---- CPU tests -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pkg():
    from __graft_entry__ import load_package
    return load_package()


def test_depth_images_and_margins(pkg):
    """The depth images: a function of (image, pixel), at least a quarter of the texels exactly 0, the rest clearly
    positive; what the dataset stores is float32(pixel) * float32(scale). The batch: under every configuration the tests
    run, no ray within a margin of target_depth > 0, of the sign of depth_ray - target_depth or of Huber's knee, so the
    comparisons exclude nothing (the count of excluded rays is asserted to be 0); at least a quarter of the compacted rays
    carry a live depth term and at least a quarter none; both signs and both sides of the knee occur."""
    mine, maps, stored = depth_world(pkg)
    assert maps[2] is None and maps[0][0].dtype == np.uint16 and maps[1][0].dtype == np.float32
    for m, st in zip(maps[:2], stored[:2]):
        assert (st == 0).mean() >= 0.25 and st[st > 0].min() >= 0.0039 and st.max() < 0.125 and st.dtype == F32
        np.testing.assert_array_equal(st, m[0].astype(F32) * F32(m[1]))
    again = depth_images(mine.images)
    assert all(np.array_equal(a[0], b[0]) for a, b in zip(maps[:2], again[:2]))
    assert not np.array_equal(maps[0][0].ravel()[:64], (maps[1][0].ravel()[:64] / 0.0005).round())   # the image matters
    excluded = 0
    for dl, cfg in depth_configs(pkg):
        excluded += depth_violations(mine, cfg, stored, dl).size + mine.violations(cfg).size
        ref = restate_loss_depth(mine, cfg, stored, DEPTH_LAMBDA, dl)
        compacted = ref["cnum"] > 0
        live = ref["live"] & compacted
        assert live.sum() >= compacted.sum() / 4 and (compacted & ~ref["live"]).sum() >= compacted.sum() / 4
        d = (ref["depth_ray"] - ref["target_depth"])[live]
        assert (d > 0).sum() > 10 and (d < 0).sum() > 10 and (np.abs(d) > 0.1).sum() > 10 and (np.abs(d) < 0.1).sum() > 10
        assert np.abs(ref["depth_term"]).max() > 0 and not ref["depth_term"][~ref["live"][ref["ray"]]].any()
        np.testing.assert_array_equal(ref["grad"][:, :3], ref["colour_grad"][:, :3])
    assert excluded == 0
    groups = batches(pkg)[0]
    for name in groups:   # the colour pass's own margins still hold on the redrawn batch
        for _, cfg, _ in groups[name]:
            assert mine.violations(cfg).size == 0
    # no fp16 gradient overflows
    for dl, cfg in depth_configs(pkg):
        assert np.abs(restate_loss_depth(mine, cfg, stored, DEPTH_LAMBDA, dl)["grad"]).max() < 3e4


def test_lambda_zero_and_missing_depth_are_the_colour_restatement(pkg):
    mine, maps, stored = depth_world(pkg)
    cfg = make_cfg(pkg)
    plain = mine.reference(cfg)
    for st, lam in ((stored, 0.0), ([None] * 3, DEPTH_LAMBDA), ([np.zeros_like(s) if s is not None else None for s in stored], DEPTH_LAMBDA)):
        ref = restate_loss_depth(mine, cfg, st, lam, "L2")
        assert not ref["live"].any()
        np.testing.assert_allclose(ref["grad"], plain["grad"], rtol=1e-13, atol=1e-300)
        np.testing.assert_array_equal(ref["loss"], plain["loss"])


def _central_difference_error(batch, cfg, stored, depth_loss):
    """As test_nerf_loss_host._central_difference_error, of 3 (colour loss) + lambda (depth loss) / n_rays per ray."""
    v = cfg_values(cfg)
    kind = LOSS[depth_loss]
    n = batch.n_rays
    out = batch.out(v["density_activation"])[:, :4].astype(np.float64)
    ref = restate_loss_depth(batch, v, stored, DEPTH_LAMBDA, depth_loss, regularisers=False)
    H = 1e-6
    M = int(batch.ns.max())
    plus = np.broadcast_to(out, (M, 4) + out.shape).copy()
    minus = plus.copy()
    for j in range(M):
        rows = batch.base[batch.ns > j] + j
        for k in range(4):
            plus[j, k, rows, k] += H
            minus[j, k, rows, k] -= H
    fz = {"upd": ref["upd"], "den_pred": ref["den_pred"]}
    s = batch.samples()
    args = (batch.pixels, batch.px, v, 0.003, 128.0, 1 << 14, n)

    def total(o):
        colour = restate_loss(s, o, *args, background=batch.background, freeze=fz, live_denominator=False)["loss"]
        dray = composite_depth(s, o, v, ref["upd"], n)["depth_ray"]
        ld, _ = loss_channel(ref["target_depth"], dray, kind, den_pred=ref["depth_ray"])
        return 3 * colour + DEPTH_LAMBDA * np.where(ref["live"] & (ref["cnum"] > 0), ld, 0.0) / n
    fd = 128.0 * (total(plus) - total(minus)) / (2 * H)
    worst = 0.0
    scale = np.zeros(n)
    np.maximum.at(scale, ref["ray"], np.abs(ref["grad"]).max(axis=1))
    for i in range(ref["ray"].size):
        r, j = ref["ray"][i], ref["sample"][i]
        for k in range(4):
            if scale[r] > 0:
                worst = max(worst, abs(fd[j, k, r] - ref["grad"][i, k]) / scale[r])
    return worst, ref


def test_gradient_matches_central_differences_with_depth(pkg):
    """The restated dL/doutput with the depth term (regularisers removed) against central differences (step 1e-6) of
    3 x colour loss + lambda x depth loss / n_rays, decisions frozen, the denominators of MAPE, SMAPE and RelativeL2
    frozen at the unperturbed depth_ray, as the colour check does: every depth loss on the 30-ray batch, Exp / Exp
    and None / None. Bound: the colour check's 1e-6 of the ray's largest gradient element."""
    _, _, small, _ = batches(pkg)
    _, _, stored = depth_world(pkg)
    worst = 0.0
    for dl in DEPTH_LOSSES:
        for loss, r, d in COLOUR_CONFIGS:
            e, ref = _central_difference_error(small, make_cfg(pkg, loss, r, d), stored, dl)
            m = ref["depth_margins"]
            assert min(m["sign"].min(), m["huber"].min()) > 1e-4 and (ref["live"] & (ref["cnum"] > 0)).sum() >= 5, (dl, loss)
            assert np.abs(ref["depth_term"]).max() > 1e-3 * np.abs(ref["grad"][:, 3]).max()
            worst = max(worst, e)
            assert e <= 1e-6, (dl, loss, e)
    print(f"central differences with depth: worst |fd - grad| / max|grad of the ray| = {worst:.2e}")


def test_central_differences_see_a_missing_depth_term(pkg):
    """The negative control: the colour gradient alone fails the same check."""
    _, _, small, _ = batches(pkg)
    _, _, stored = depth_world(pkg)
    cfg = make_cfg(pkg)
    e, ref = _central_difference_error(small, cfg, stored, "L2")
    assert e <= 1e-6
    err = np.abs(ref["grad"][:, 3] - ref["colour_grad"][:, 3]).max() / np.abs(ref["grad"]).max()
    assert err > 1e-3


def test_float32_restatement_measures_k32d(pkg):
    """K32D (module docstring): numpy float32 against float64, the density column of every compacted sample, in units of
    2^-24 companion; every depth loss x the two colour configurations."""
    mine, maps, stored = depth_world(pkg)
    worst = 0.0
    for dl, cfg in depth_configs(pkg):
        ref = restate_loss_depth(mine, cfg, stored, DEPTH_LAMBDA, dl)
        g32 = restate_density_gradient_f32(mine, cfg, stored, DEPTH_LAMBDA, dl, ref).astype(np.float64)
        u = in_units(np.abs(g32 - ref["grad"][:, 3]), ref["grad_companion"][:, 3])
        worst = max(worst, float(u.max()))
        assert u.max() <= K32D, (dl, int(cfg.loss_type), float(u.max()), int(u.argmax()))
    print(f"K32D: float32 vs float64 with depth, density gradient {worst:.3f} units of 2^-24 companion (constant K32D = {K32D})")
    assert worst > K32D - 0.05 or K32D == 0.05    # K32D is the measured worst rounded up to the next 0.05


# ---- the C-ABI without a GPU ---------------------------------------------------------------------------------------------
NEW_SYMBOLS = ("ngp_nerf_dataset_set_depth", "ngp_nerf_dataset_depth", "ngp_nerf_compute_loss_depth",
               "ngp_nerf_trainer_set_depth_supervision", "ngp_nerf_trainer_get_depth_supervision")
NGP_INVALID = -2


def test_depth_symbols_exist(pkg):
    L = pkg.lib()
    for name in NEW_SYMBOLS:
        assert getattr(L, name) is not None
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "ngp_engine.h")).read()
    for name in NEW_SYMBOLS:
        assert f"int {name}(" in header


def test_depth_arguments_are_checked_before_any_gpu_call(pkg):
    L = pkg.lib()
    px = np.zeros(16, np.uint16)
    has = C.c_int32(7)
    # a NULL dataset (and with it any image index), a dtype that is neither uint16 nor float32
    assert L.ngp_nerf_dataset_set_depth(None, 0, px.ctypes.data, 0, 1.0) == NGP_INVALID
    assert L.ngp_nerf_dataset_set_depth(None, 5, px.ctypes.data, 2, 1.0) == NGP_INVALID
    assert L.ngp_nerf_dataset_depth(None, 0, None, 0, C.byref(has)) == NGP_INVALID and has.value == 7
    # the trainer's setter: NULL, negative, NaN, infinite lambda, an unknown loss
    for lam, lt in ((0.5, 1), (-1.0, 1), (float("nan"), 1), (float("inf"), 1), (0.5, 7)):
        assert L.ngp_nerf_trainer_set_depth_supervision(None, lam, lt) == NGP_INVALID
    assert L.ngp_nerf_trainer_get_depth_supervision(None, None, None) == NGP_INVALID
    # the entry point: a bad lambda or loss is refused before the pointers are looked at (they are all NULL here)
    cfg = pkg.nerf.default_config(1.0)
    for lam, lt in ((-0.5, 1), (float("nan"), 1), (float("inf"), 0), (0.5, 7), (0.5, 1)):
        rc = L.ngp_nerf_compute_loss_depth(None, C.byref(cfg), None, 4, 4, pkg.nerf.pcg32(1), 16, None, None, None, None, None, None,
                                           None, None, None, None, None, 128.0, None, 0, 0, None, None, 0, 0, 0, None, None, 0,
                                           lam, lt)
        assert rc == NGP_INVALID
    with pytest.raises(KeyError):
        pkg.nerf.LOSS["Depth"]


# ---- the loader ----------------------------------------------------------------------------------------------------------
def _write_scene(tmp_path, depth_shape=(4, 4), **top):
    from PIL import Image
    g = np.random.default_rng(3)
    frames = []
    depth = (g.integers(0, 60000, depth_shape)).astype(np.uint16)
    depth[0, 1] = 0
    for k in range(2):
        Image.fromarray(g.integers(0, 256, (4, 4, 4), dtype=np.uint8), "RGBA").save(tmp_path / f"f{k}.png")
        m = np.eye(4)
        m[:3, 3] = (0.1 * k, 0.2, 3.0)
        frames.append({"file_path": f"f{k}.png", "transform_matrix": m.tolist(), "depth_path": f"d{k}.png"})
    Image.fromarray(depth).save(tmp_path / "d0.png")          # mode I;16; d1.png does not exist
    j = {"camera_angle_x": 0.7, "scale": 0.5, "integer_depth_scale": 0.001, "frames": frames}
    j.update(top)
    j = {k: v for k, v in j.items() if v is not None}
    (tmp_path / "transforms.json").write_text(json.dumps(j))
    return str(tmp_path / "transforms.json"), depth


def test_loader_reads_depth(pkg, tmp_path):
    path, depth = _write_scene(tmp_path)
    from PIL import Image
    assert Image.open(tmp_path / "d0.png").mode.startswith("I;16")
    data = pkg.nerf_data.load_nerf(path)
    assert len(data) == 2 and data.depth[1] is None            # the missing file is ignored
    assert data.depth[0].dtype == np.uint16 and data.depth[0].shape == (4, 4)
    np.testing.assert_array_equal(data.depth[0], depth)
    want = float(F32(0.001) * F32(0.5))                         # integer_depth_scale * the dataset's scale, in float
    assert data.depth_scale == [want, want]
    # enable_depth_loading: false, and no integer_depth_scale: no depth
    (tmp_path / "a").mkdir()
    (tmp_path / "b").mkdir()
    (tmp_path / "c").mkdir()
    off = pkg.nerf_data.load_nerf(_write_scene(tmp_path / "a", enable_depth_loading=False)[0])
    assert off.depth == [None, None]
    none = pkg.nerf_data.load_nerf(_write_scene(tmp_path / "b", integer_depth_scale=None)[0])
    assert none.depth == [None, None] and all(s < 0 for s in none.depth_scale)
    with pytest.raises(ValueError, match="wrong resolution"):
        pkg.nerf_data.load_nerf(_write_scene(tmp_path / "c", depth_shape=(4, 5))[0])


def test_synthetic_depth_is_the_scene_z_depth(pkg):
    """render(return_depth=True): the same RGBA as without, depth 0 exactly where alpha is 0, and for the camera on the z
    axis above the big sphere the centre pixel's depth is the distance to the sphere's top."""
    S = pkg.synthetic
    c2w = S.camera_poses(3, seed=5)[1]
    rgba = S.render(c2w, 32, 32)
    rgba2, depth = S.render(c2w, 32, 32, return_depth=True)
    np.testing.assert_array_equal(rgba, rgba2)
    assert depth.dtype == np.float32 and depth.shape == (32, 32)
    np.testing.assert_array_equal(depth == 0, rgba[..., 3] == 0)
    assert depth[rgba[..., 3] > 0].min() > 2.0 and depth.max() < 6.0
    top = S.look_at_c2w((0.0, 0.0, 4.0))
    _, d = S.render(top, 33, 33, return_depth=True)
    assert abs(d[16, 16] - (4.0 - 0.75)) < 1e-4                 # the sphere at (0, 0, 0.2), radius 0.55
