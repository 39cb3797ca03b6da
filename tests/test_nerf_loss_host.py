"""The NeRF loss pass (compute_loss_kernel_train_nerf, testbed_nerf.cu:1660-2012) restated in float64 numpy, the
hand-built batches the GPU test runs (test_gpu_nerf_loss.py imports both), and the CPU tests that validate the
restatement: central differences of its own loss against its analytic gradient, and the float32 C oracle against it.
No GPU call is made.

The restatement is written from the mathematics: a ray composites its samples front to back (weight alpha T, T the
transmittance left) until T < 1e-4, adds the background if no sample was left out, compares with the image's texel in
one of three colour spaces, and hands every composited sample dL/d(raw rgb) and dL/d(raw density), plus three
regularisers. It is vectorised over rays and loops over the sample index only.

Errors are measured in units of 2^-24 of a conditioning companion: the same expression with every term replaced by
its magnitude (as out_abs / grads_abs elsewhere in this suite), taken down to the innermost subtraction. That depth is
needed: float32 computes alpha = 1 - exp(-sigma dt) and T *= 1 - alpha, so a thin sample's weight and the
transmittance behind an opaque sample carry exp's absolute error, 2^-24 of 1, however small they are. With the
magnitudes of the outermost expression only (sigma' dt sum_c |g_c| (T |rgb_c| + |suffix_c|) for the density row) the
float32 oracle is 2.3e6 units from float64 on this batch, and a bound built on that checks nothing. So every
intermediate carries a companion that follows the first-order propagation of one rounding per operation: for
x = a op b, |x| plus the operands' companions times the magnitudes of the partial derivatives (restate_loss' loop,
loss_channel_companion, slope_companion); fp16 inputs are exact, exp, logistic and powf count 2 to 4 roundings.

K32: the float32 oracle (oracle/ngp_nerf_oracle.c, glibc powf) against the restatement on the 300-ray batch over every
configuration of config_groups(), in those units, is at most K32 = 0.25 (measured 0.203 for the loss and 0.244 for the
gradient after half an fp16 ulp of the float64 value is taken off; test_oracle_agrees_with_the_restatement prints
both). It is below 1 because the companion adds every rounding's worst case. The GPU test allows 4 * K32: the device's
powf is ocml's (a few ulp from glibc's) and ngp_expf_fast / ngp_expf_mid are within 1 ulp of exact. That tolerance
comes from float32 reference arithmetic, never from the kernel's output.
"""
import functools

import numpy as np
import pytest

F32 = np.float32
K32 = 0.25


def C(x):
    """A float literal of the reference (`0.1f`): the float32 value, as a Python float."""
    return float(F32(x))


MIN_STEP = float(F32(1.73205080757) / F32(1024))                       # STEPSIZE(): sqrt(3) / 1024
DT_SPAN = float(F32(F32(MIN_STEP) * F32(128)) - F32(MIN_STEP))         # unwarp_dt: dt = warped * span + MIN_STEP
T_STOP = C(1e-4)
MASKED = (255, 0, 255, 0)                                              # the texel 0x00FF00FF
LOSS = {"L2": 0, "L1": 1, "MAPE": 2, "SMAPE": 3, "Huber": 4, "LogL1": 5, "RelativeL2": 6}
SIGN_LOSSES = (1, 2, 3, 5)
ACT_NONE, ACT_RELU, ACT_LOGISTIC, ACT_EXP = 0, 1, 2, 3


# ---- the float64 restatement -----------------------------------------------------------------------------------------
def _logistic(v):
    return 1.0 / (1.0 + np.exp(-v))


def rgb_value(v, a):
    return [v, np.where(v > 0, v, 0.0), _logistic(v), np.exp(np.clip(v, -10.0, 10.0))][a]


def rgb_slope(v, a):
    s = _logistic(v)
    return [np.ones_like(v), np.where(v > 0, 1.0, 0.0), s * (1 - s), np.exp(np.clip(v, -10.0, 10.0))][a]


def density_value(v, a):
    return [v, np.where(v > 0, v, 0.0), _logistic(v), np.exp(v)][a]


def density_slope(v, a):
    s = _logistic(v)
    return [np.ones_like(v), np.where(v > 0, 1.0, 0.0), s * (1 - s), np.exp(np.clip(v, -15.0, 15.0))][a]


SRGB_KNEE, LINEAR_KNEE = C(0.04045), C(0.0031308)


def srgb_to_linear(s):
    with np.errstate(invalid="ignore"):
        return np.where(s <= SRGB_KNEE, s / C(12.92), ((np.maximum(s, 0) + C(0.055)) / C(1.055)) ** C(2.4))


def linear_to_srgb(l):
    """The reference's exponent is 0.41666, not 1 / 2.4 (common_device.cuh:102)."""
    return np.where(l < LINEAR_KNEE, C(12.92) * l, C(1.055) * np.maximum(l, 0) ** C(0.41666) - C(0.055))


def loss_channel(target, pred, kind, den_pred=None):
    """loss_and_gradient per channel (testbed_nerf.cu:1340-1355, loss.h). The gradients of MAPE, SMAPE and RelativeL2
    treat their denominator as a constant; den_pred: the prediction the denominator is evaluated at (default: pred)."""
    d = pred - target
    p = pred if den_pred is None else den_pred
    sign = np.where(np.signbit(d), -1.0, 1.0)
    if kind == 0:
        return d * d, 2 * d
    if kind == 1:
        return np.abs(d), sign
    if kind == 2:
        den = np.abs(p) + C(1e-2)
        return np.abs(d) / den, sign / den
    if kind == 3:
        den = 0.5 * (np.abs(p) + np.abs(target)) + C(1e-2)
        return np.abs(d) / den, sign / den
    if kind == 4:
        a, ad = C(0.1), np.abs(d)
        big = ad > a
        return np.where(big, ad - 0.5 * a, 0.5 / a * d * d) / 5.0, np.where(big, np.where(d > 0, 1.0, -1.0), d / a) / 5.0
    if kind == 5:
        return np.log(np.abs(d) + 1.0), sign / (np.abs(d) + 1.0)
    if kind == 6:
        den = p * p + C(1e-2)
        return d * d / den, 2 * d / den
    raise ValueError(kind)


def loss_channel_companion(target, pred, kind, d_c, pred_c, target_c):
    """First-order error companions of loss_channel's two results, given those of d = pred - target, pred and target."""
    d = pred - target
    l, g = loss_channel(target, pred, kind)
    l, g, ad = np.abs(l), np.abs(g), np.abs(d)
    if kind == 0:
        return 2 * ad * d_c + l, 2 * d_c + g
    if kind == 1:
        return d_c + l, np.zeros_like(g)
    if kind in (2, 3, 6):
        if kind == 2:
            den = np.abs(pred) + C(1e-2)
            den_c = pred_c + den
        elif kind == 3:
            den = 0.5 * (np.abs(pred) + np.abs(target)) + C(1e-2)
            den_c = 0.5 * (pred_c + target_c) + den
        else:
            den = pred * pred + C(1e-2)
            den_c = 2 * np.abs(pred) * pred_c + 2 * pred * pred + den
            return 2 * ad * d_c / den + l * den_c / den + 2 * l, 2 * d_c / den + g * den_c / den + 2 * g
        return d_c / den + l * den_c / den + l, g * den_c / den + g
    if kind == 4:
        a = C(0.1)
        big = ad > a
        return np.where(big, d_c / 5 + 2 * l, ad / a * d_c / 5 + 3 * l), np.where(big, g, d_c / (5 * a) + 2 * g)
    if kind == 5:   # log(|d| + 1): the sum rounds at 1, whatever |d| is
        rel = (d_c + ad + 1.0) / (ad + 1.0)
        return rel + 2 * l, g * rel + g
    raise ValueError(kind)


def slope_companion(v, a, slope):
    """Of rgb_slope / density_slope: nothing to round for None and ReLU; the logistic's d (1 - d) keeps d's absolute
    error in 1 - d; the exponential is one function of an exact fp16 argument."""
    d = _logistic(v)
    return [np.zeros_like(v), np.zeros_like(v), d * (1 + d) + 2 * d * (1 - d), 2 * slope][a]


def cfg_values(cfg):
    """The fields of an ngp_nerf_config the loss pass reads, as a plain dict."""
    return {"aabb_min": np.array(cfg.aabb_min[:], np.float64), "aabb_max": np.array(cfg.aabb_max[:], np.float64),
            "random_bg_color": int(cfg.random_bg_color), "linear_colors": int(cfg.linear_colors),
            "color_space_linear": int(cfg.color_space_linear), "background_color": np.array(cfg.background_color[:], np.float64),
            "rgb_activation": int(cfg.rgb_activation), "density_activation": int(cfg.density_activation),
            "loss_type": int(cfg.loss_type), "near_distance": float(cfg.near_distance)}


def restate_loss(samples, out, pixels, px, cfg, mean_density, loss_scale, max_compacted, n_rays, background=None,
                 regularisers=True, freeze=None, live_denominator=True):
    """compute_loss_kernel_train_nerf in float64. samples: {ray_indices, rays, numsteps [n, 2] = {n, base}, coords
    [N, 7], counters}; out: the network output, fp16 [N, >= 4] (or float64, for differencing: any leading axes before
    [N, 4] are carried through the loss and nothing else is returned in full); pixels: the dataset's RGBA8 images; px:
    every ray's {"img", "uv"}; cfg: cfg_values(); background [n_rays, 3]: the sRGB background per ray when
    random_bg_color is set (pcg32_backgrounds). freeze: {"upd", "den_pred"} of an earlier result, so that perturbed
    outputs take the same stop decisions (and, unless live_denominator, the same loss denominators)."""
    R = int(n_rays)
    ns_in = np.asarray(samples["numsteps"]).astype(np.int64).reshape(-1, 2)[:R]
    active = np.arange(R) < min(int(samples["counters"][0]), R)
    ns, base = np.where(active, ns_in[:, 0], 0), ns_in[:, 1]
    M = max(int(ns.max()) if R else 0, 1)
    jj = np.arange(M)
    valid = jj[None, :] < ns[:, None]
    idx = np.where(valid, base[:, None] + jj[None, :], 0)
    o = np.asarray(out)[..., :4].astype(np.float64)[..., idx, :]                     # [..., R, M, 4]
    coords = np.asarray(samples["coords"]).astype(np.float64)
    dt = coords[idx, 3] * DT_SPAN + MIN_STEP
    ra, da = cfg["rgb_activation"], cfg["density_activation"]
    rgb = rgb_value(o[..., :3], ra)
    sigma = density_value(o[..., 3], da)
    alpha = 1.0 - np.exp(-sigma * dt)
    lead = o.shape[:-3]
    T = np.ones(lead + (R,))
    acc, acc_c = np.zeros(lead + (R, 3)), np.zeros(lead + (R, 3))
    T_c = np.zeros(lead + (R,))
    stopped = np.zeros(lead + (R,), bool)
    upd_all = np.zeros(lead + (R, M), bool)
    w_all, T_all = np.zeros(lead + (R, M)), np.zeros(lead + (R, M))
    prefix_all = np.zeros(lead + (R, M, 3))
    w_c_all, T_c_all, prefix_c_all = np.zeros(lead + (R, M)), np.zeros(lead + (R, M)), np.zeros(lead + (R, M, 3))
    t_margin = np.full(lead + (R,), np.inf)
    for j in range(M):
        act = valid[:, j] & ~stopped
        if freeze is None:
            low = T < T_STOP
            t_margin = np.where(act, np.minimum(t_margin, np.abs(T - T_STOP) / T_STOP), t_margin)
            upd = act & ~low
            stopped = stopped | (act & low)
        else:
            upd = np.broadcast_to(freeze["upd"][:, j], act.shape)
        a, cj = alpha[..., j], rgb[..., j, :]
        w = a * T
        # the companions (module docstring): e = exp(-x) of a rounded x = sigma dt; alpha = 1 - e and 1 - alpha keep e's
        # absolute error however small they are
        x = sigma[..., j] * dt[:, j]
        e_c = np.exp(-x) * (3 * np.abs(x) + 2)
        a_c = e_c + np.abs(a)
        w_c = a_c * np.abs(T) + np.abs(a) * T_c + np.abs(w)
        new_acc, new_T = acc + w[..., None] * cj, T * (1.0 - a)
        new_acc_c = acc_c + w_c[..., None] * np.abs(cj) + 3 * np.abs(w[..., None] * cj) + np.abs(new_acc)
        new_T_c = T_c * np.abs(1.0 - a) + np.abs(T) * (a_c + np.abs(1.0 - a)) + np.abs(new_T)
        acc, acc_c = np.where(upd[..., None], new_acc, acc), np.where(upd[..., None], new_acc_c, acc_c)
        T, T_c = np.where(upd, new_T, T), np.where(upd, new_T_c, T_c)
        upd_all[..., j], w_all[..., j], T_all[..., j], prefix_all[..., j, :] = upd, w, T, acc
        w_c_all[..., j], T_c_all[..., j], prefix_c_all[..., j, :] = w_c, T_c, acc_c
    cn = upd_all.sum(axis=-1)
    kept_all = cn == ns
    # the target texel and the background
    img, uv = np.asarray(px["img"]).astype(np.int64)[:R], np.asarray(px["uv"], F32)[:R]
    texel = np.zeros((R, 4), np.int64)
    for i in range(R):
        h, w_ = pixels[img[i]].shape[:2]
        x = min(max(int(F32(uv[i, 0]) * F32(w_)), 0), w_ - 1)
        y = min(max(int(F32(uv[i, 1]) * F32(h)), 0), h - 1)
        texel[i] = pixels[img[i]][y, x]
    masked = (texel == np.array(MASKED)).all(axis=1)
    a8 = texel[:, 3:4] / 255.0
    tex_rgb = np.where(masked[:, None], -1.0, srgb_to_linear(texel[:, :3] / 255.0) * a8)      # premultiplied, linear
    tex_a = np.where(masked[:, None], -1.0, a8)
    bg_srgb = np.asarray(background, np.float64)[:R] if cfg["random_bg_color"] else np.broadcast_to(cfg["background_color"], (R, 3))
    bg = srgb_to_linear(bg_srgb)
    target_mag = np.abs(tex_rgb) + np.abs((1.0 - tex_a) * bg)
    knee = np.full(R, np.inf)

    def to_srgb(l):
        nonlocal knee
        knee = np.minimum(knee, np.abs(l - LINEAR_KNEE).min(axis=1))
        return linear_to_srgb(l)
    if cfg["linear_colors"]:
        target = tex_rgb + (1.0 - tex_a) * bg
    elif cfg["color_space_linear"]:
        target = to_srgb(tex_rgb + (1.0 - tex_a) * bg)
        bg = to_srgb(bg)
    else:   # un-premultiply, to sRGB, premultiply again; a texel without alpha is the background
        bg = to_srgb(bg)
        pos = tex_a > 0
        straight = np.where(pos, tex_rgb / np.where(pos, tex_a, 1.0), 1.0)
        target = np.where(pos, to_srgb(straight) * tex_a + (1.0 - tex_a) * bg, bg)
    pred = acc + np.where(kept_all[..., None], T[..., None] * bg, 0.0)
    # two powf behind the target, one behind the background: 8 and 4 roundings allowed
    target_c = 8 * (np.abs(target) + target_mag)
    pred_c = acc_c + np.where(kept_all[..., None], T_c[..., None] * np.abs(bg) + 6 * np.abs(T[..., None] * bg), 0.0) + np.abs(pred)
    d_c = pred_c + target_c + np.abs(pred - target)
    den_pred = None
    if freeze is not None and not live_denominator:
        den_pred = freeze["den_pred"]
    lc, gc = loss_channel(target, pred, cfg["loss_type"], den_pred)
    lc_c, gc_c = loss_channel_companion(target, pred, cfg["loss_type"], d_c, pred_c, target_c)
    mean_loss = lc.sum(axis=-1) / 3.0
    # compaction: a running total of the composited counts in ray order, cut at max_compacted
    cn_a = np.where(active, cn, 0)
    cbase = np.cumsum(cn_a, axis=-1) - cn_a
    cnum = np.minimum(max_compacted - np.minimum(max_compacted, cbase), cn_a)
    loss = np.where(cnum > 0, mean_loss / R, 0.0)
    if lead:
        return {"loss": loss}
    numsteps = np.asarray(samples["numsteps"]).astype(np.int64).reshape(-1, 2).copy()
    numsteps[:R][active] = np.stack([cnum, cbase], axis=1)[active]
    d = pred - target
    res = {"loss": loss, "mean_loss": mean_loss, "numsteps": numsteps.astype(np.uint32), "compacted_counter": int(cn_a.sum()),
           "cn": cn, "cnum": cnum, "cbase": cbase, "pred": pred, "target": target, "upd": upd_all, "den_pred": pred,
           "loss_companion": np.where(cnum > 0, (lc_c.sum(axis=-1) / 3.0 + 3 * mean_loss) / R, 0.0),
           "img": img, "uv": uv,
           "margins": {"t_stop": t_margin, "huber": np.abs(np.abs(d) - C(0.1)).min(axis=1), "sign": np.abs(d).min(axis=1),
                       "srgb_knee": knee}}
    # gradients of the compacted samples
    ray = np.repeat(np.arange(R), cnum)
    j = np.arange(ray.size) - np.repeat(np.cumsum(cnum) - cnum, cnum)
    row = np.repeat(cbase, cnum) + j
    assert (row < max_compacted).all()
    src = base[ray] + j
    ls = loss_scale / R
    oo, w, Tj, dtj = o[ray, j], w_all[ray, j], T_all[ray, j], dt[ray, j]
    g, c = gc[ray], rgb[ray, j]
    suffix = pred[ray] - prefix_all[ray, j]
    l2 = np.maximum(0.0, C(1e-4) * oo[:, :3]) if (ra == ACT_EXP and regularisers) else np.zeros_like(c)
    slope = rgb_slope(oo[:, :3], ra)
    slope_c = slope_companion(oo[:, :3], ra, slope)
    grad, comp = np.zeros((ray.size, 4)), np.zeros((ray.size, 4))
    wg = w[:, None] * g
    grad[:, :3] = ls * (wg * slope + l2)
    comp[:, :3] = (ls * ((w_c_all[ray, j][:, None] * np.abs(g) + np.abs(w)[:, None] * gc_c[ray]) * slope + np.abs(wg) * slope_c
                         + 2 * np.abs(wg * slope) + 2 * np.abs(l2)) + np.abs(grad[:, :3]))
    ds = density_slope(oo[:, 3], da)
    ds_c = slope_companion(oo[:, 3], da, ds)
    brace = Tj[:, None] * c - suffix
    dot = (g * brace).sum(axis=1)
    dmlp_unit = ls * dtj * dot                                           # per unit of the density's slope
    dmlp = ds * dmlp_unit
    suffix_c = pred_c[ray] + prefix_c_all[ray, j] + np.abs(suffix)
    brace_c = T_c_all[ray, j][:, None] * np.abs(c) + 3 * np.abs(Tj[:, None] * c) + suffix_c + np.abs(brace)
    dot_c = (gc_c[ray] * np.abs(brace) + np.abs(g) * brace_c + 3 * np.abs(g * brace)).sum(axis=1)
    box = cfg["aabb_max"] - cfg["aabb_min"]
    position = cfg["aabb_min"] + coords[src, :3] * box
    depth = np.linalg.norm(position - np.asarray(samples["rays"]).astype(np.float64)[ray, :3], axis=1)
    l1 = np.where(oo[:, 3] < 0, -C(1e-4), 0.0) if (regularisers and float(F32(mean_density)) < C(0.01)) else np.zeros(ray.size)
    near = np.where((oo[:, 3] > -10.0) & (depth < cfg["near_distance"]), C(1e-4), 0.0) if regularisers else np.zeros(ray.size)
    grad[:, 3] = dmlp + l1 + near
    comp[:, 3] = (ls * dtj * (ds_c * np.abs(dot) + ds * dot_c) + 5 * np.abs(dmlp) + np.abs(l1) + np.abs(near) + 2 * np.abs(grad[:, 3]))
    near_margin = np.full(R, np.inf)
    np.minimum.at(near_margin, ray, np.abs(depth - cfg["near_distance"]))
    res["margins"]["near"] = near_margin
    res.update(grad=grad, grad_companion=comp, coords_compacted=np.asarray(samples["coords"], F32)[src], row=row, ray=ray,
               sample=j, weight=w, ray_gradient=g, dmlp=dmlp, dmlp_unit=dmlp_unit, raw=oo, depth=depth)
    return res


def error_map_deposit(ref, pixels, width, height):
    """The error map deposit (testbed_nerf.cu:1869-1899): every compacted ray's mean loss split bilinearly over the four
    texels around uv * res - 0.5, the texel index clamped with the ray's image's resolution."""
    em = np.zeros((len(pixels), height, width))
    for i in np.nonzero(ref["cnum"] > 0)[0]:
        u, v = ref["uv"][i].astype(np.float64)
        x = min(max(u * width - 0.5, 0.0), width - (1.0 + C(1e-4)))
        y = min(max(v * height - 0.5, 0.0), height - (1.0 + C(1e-4)))
        wx, wy = x - int(x), y - int(y)
        ih, iw = pixels[ref["img"][i]].shape[:2]
        ix, iy = min(max(int(x), 0), iw - 2), min(max(int(y), 0), ih - 2)
        e, ml = em[ref["img"][i]], ref["mean_loss"][i]
        e[iy, ix] += (1 - wx) * (1 - wy) * ml
        e[iy, ix + 1] += wx * (1 - wy) * ml
        e[iy + 1, ix] += (1 - wx) * wy * ml
        e[iy + 1, ix + 1] += wx * wy * ml
    return em


# ---- pcg32 -------------------------------------------------------------------------------------------------------------
_M64, _PCG_MULT = (1 << 64) - 1, 0x5851F42D4C957F2D


class Pcg32:
    """tcnn::pcg32 (pcg32.h) in Python integers."""

    def __init__(self, state, inc):
        self.state, self.inc = int(state), int(inc)

    def next_uint(self):
        old = self.state
        self.state = (old * _PCG_MULT + self.inc) & _M64
        x = (((old >> 18) ^ old) >> 27) & 0xFFFFFFFF
        rot = old >> 59
        return ((x >> rot) | (x << ((-rot) & 31))) & 0xFFFFFFFF

    def next_float(self):
        return float(np.array([(self.next_uint() >> 9) | 0x3F800000], np.uint32).view(F32)[0] - F32(1.0))

    def advance(self, delta):
        cur_mult, cur_plus, acc_mult, acc_plus = _PCG_MULT, self.inc, 1, 0
        delta &= _M64
        while delta:
            if delta & 1:
                acc_mult = (acc_mult * cur_mult) & _M64
                acc_plus = (acc_plus * cur_mult + cur_plus) & _M64
            cur_plus = ((cur_mult + 1) * cur_plus) & _M64
            cur_mult = (cur_mult * cur_mult) & _M64
            delta >>= 1
        self.state = (acc_mult * self.state + acc_plus) & _M64


def pcg32_backgrounds(rng, ray_indices):
    """The random sRGB background of every ray: its stream advanced by ray_idx * 16, the pixel's two draws, one skipped
    draw (motion blur time), then three floats (testbed_nerf.cu:1763-1779)."""
    bg = np.zeros((len(ray_indices), 3))
    for i, r in enumerate(ray_indices):
        g = Pcg32(rng.state, rng.inc)
        g.advance(int(r) * 16)
        g.next_float(), g.next_float()
        g.advance(1)
        bg[i] = [g.next_float() for _ in range(3)]
    return bg


# ---- the batches ---------------------------------------------------------------------------------------------------------
RAY_COUNTS = (1, 3, 4, 5, 16, 17, 127, 128, 129, 300)
STEP_COUNTS = (0, 1, 15, 16, 17, 31, 32, 33, 47, 48, 63, 64, 65, 100)
STEP_PATTERN = (17, 0, 33, 1, 65, 16, 100, 15, 32, 31, 47, 48, 63, 64)
N_RAYS_TOTAL = 307   # the batch the rays' indices (and so their images) are drawn from
RNG_SEED = 11
# dense rays built around one opaque sample: ray -> (samples, index of the opaque sample)
STOPS = {20: (17, 5),     # transmittance gone inside the first chunk of 16
         21: (33, 15),    # sample 16 is the first one not composited: the stop is carried across the chunk boundary
         22: (48, 31),    # likewise sample 32: the prefetch ring wraps
         23: (33, 32),    # gone in the last sample: every sample is kept, the background gets T ~ 0
         24: (100, 63),   # sample 64: the second round of the wave-per-ray pass 2
         25: (100, 99)}
# values planted in one known sample (index 1 of a 4-sample ray, the last one for the opaque densities): (column, value),
# every value exact in fp16
F16_BELOW_M10, F16_ABOVE_M10 = -10.0078125, -9.9921875
PLANTED = [(0, 0.0), (1, -0.0), (2, 10.0), (0, -10.0), (1, 11.0), (2, -11.0), (0, 10.0078125), (1, -10.0078125),
           (3, 0.0), (3, -0.0), (3, -10.0), (3, F16_BELOW_M10), (3, F16_ABOVE_M10), (3, -15.0), (3, -16.0), (3, -15.0078125),
           (3, 15.0), (3, 16.0), (3, 15.0078125)]
PLANTED_FIRST = 200
MARGIN_T, MARGIN_HUBER, MARGIN_SIGN, MARGIN_NEAR, MARGIN_KNEE = 1e-3, 1e-4, 1e-5, 1e-4, 1e-6
NEAR = C(0.1)


def planted_row(batch, k):
    """(ray, sample) of PLANTED[k]."""
    return PLANTED_FIRST + k, (3 if PLANTED[k] in ((3, 15.0), (3, 16.0), (3, 15.0078125)) else 1)


class Batch:
    """A sampler's output made by hand, the network output for each density activation, the dataset and the pixels."""

    def __init__(self, pkg, n_rays=300, step_pattern=STEP_PATTERN, special=True, seed=0):
        self.pkg, self.n_rays, self.seed, self.special = pkg, n_rays, seed, special
        S = pkg.synthetic
        g = np.random.default_rng(1000 + seed)
        self.images, self.pixels = [], []
        for c2w, (w, h) in zip(S.camera_poses(3, seed=2), ((8, 8), (12, 10), (10, 9))):
            self.images.append(pkg.nerf.make_image(w, h, pkg.nerf.nerf_matrix_to_ngp(c2w), camera_angle_x=S.LEGO_CAMERA_ANGLE_X))
            px = g.integers(0, 256, (h, w, 4), dtype=np.uint8)
            kind = g.random((h, w))
            px[..., 3] = np.where(kind < 0.25, 0, np.where(kind < 0.55, 255, g.integers(1, 255, (h, w))))
            for y, x in ((1, 2), (h - 1, 0), (3, w - 1), (4, 4)):
                px[y, x] = MASKED
            self.pixels.append(px)
        self.rng = pkg.nerf.pcg32(RNG_SEED)
        self.cfg0 = pkg.nerf.default_config(2.0)   # aabb [-0.5, 1.5]: positions are not the coordinates themselves
        ns = np.array([step_pattern[i % len(step_pattern)] for i in range(n_rays)], np.int64)
        if special:
            for r, (n, _) in STOPS.items():
                ns[r] = n
            ns[PLANTED_FIRST:PLANTED_FIRST + len(PLANTED)] = 4
        self.ns = ns
        self.base = np.cumsum(ns) - ns
        self.total = int(ns.sum())
        self.ray_indices = np.sort(g.choice(N_RAYS_TOTAL, n_rays, replace=False)).astype(np.uint32)
        px_all = pkg.nerf.training_pixels(self.images, self.cfg0, N_RAYS_TOTAL, self.rng, host=True)
        self.px = {"img": px_all["img"][self.ray_indices], "uv": px_all["uv"][self.ray_indices]}
        self.background = pcg32_backgrounds(self.rng, self.ray_indices)
        self.attempt = np.zeros(n_rays, np.int64)
        self.rays = np.zeros((n_rays, 6), F32)
        self.coords = np.zeros((self.total, 7), F32)
        self.sigma_dt = np.zeros(self.total)
        self.rgb_raw = np.zeros((self.total, 3), np.float16)
        for r in range(n_rays):
            self._draw_ray(r)

    def _draw_ray(self, r):
        """Ray r's origin, samples and outputs, from (seed, r, attempt[r]) alone."""
        g = np.random.default_rng([self.seed, r, int(self.attempt[r])])
        n, b = int(self.ns[r]), int(self.base[r])
        o = g.uniform(0.3, 0.7, 3)
        d = g.standard_normal(3)
        d /= np.linalg.norm(d)
        self.rays[r] = np.concatenate([o, 2.5 * d])            # the direction is not normalised; the loss reads the origin
        planted = self.special and PLANTED_FIRST <= r < PLANTED_FIRST + len(PLANTED)
        # depths on both sides of near_distance, none within 3e-4 of it
        t = 0.02 + (0.01 if planted else g.uniform(0.004, 0.03)) * np.arange(n) + (0.0 if planted else g.uniform(0, 0.05))
        t = np.where(np.abs(t - NEAR) < 3e-4, NEAR + 3e-4 * np.where(t < NEAR, -1.0, 1.0), t)
        c = self.coords[b:b + n]
        c[:, :3] = ((o + t[:, None] * d) + 0.5) / 2.0
        c[:, 3] = 0.0 if planted else g.random(n)
        c[:, 4:] = (d + 1) / 2
        kind = r % 3
        sd = (g.uniform(0.2, 1.5, n) if kind == 0 else g.uniform(0.001, 0.05, n) if kind == 1 else g.uniform(0.02, 0.3, n))
        rgb = g.uniform(-3.0, 2.0, (n, 3))
        if self.special and r in STOPS:
            sd = g.uniform(0.02, 0.08, n)
            sd[STOPS[r][1]] = 12.0
        if planted:
            sd = np.full(n, 0.05)
            rgb = g.uniform(-3.0, 0.3, (n, 3))
            col, _ = PLANTED[r - PLANTED_FIRST]
            if col < 3:
                sd[1] = 1e-4   # exp(10) reaches the prediction through a small weight: fp16 gradients stay finite
        self.sigma_dt[b:b + n] = sd
        self.rgb_raw[b:b + n] = rgb

    def samples(self, n_rays=None, counter=None):
        """The samples dict (host arrays, fresh copies) of the first n_rays rays."""
        n = self.n_rays if n_rays is None else n_rays
        numsteps = np.stack([self.ns, self.base], axis=1).astype(np.uint32)[:n]
        return {"ray_indices": self.ray_indices[:n].copy(), "rays": self.rays[:n].copy(), "numsteps": numsteps.copy(),
                "coords": self.coords.copy(), "counters": np.array([n if counter is None else counter, self.total], np.uint32)}

    def out(self, density_activation):
        """The network output, fp16 [total, 16]: the raw density whose activation gives sigma_dt / dt (Logistic: what
        it can reach); columns 4..15 carry values the loss pass must not read."""
        dt = self.coords[:, 3].astype(np.float64) * DT_SPAN + MIN_STEP
        sigma = self.sigma_dt / dt
        if density_activation == ACT_EXP:
            raw = np.log(sigma)
        elif density_activation == ACT_LOGISTIC:
            s = np.clip(sigma, 0.02, 0.98)
            raw = np.log(s / (1 - s))
        else:   # None, ReLU: a few negative densities (alpha < 0 and T > 1 for None) in the thin rays
            ray = np.repeat(np.arange(self.n_rays), self.ns)
            raw = np.where((ray % 3 == 1) & (np.arange(self.total) % 11 == 0), -sigma, sigma)
        out = np.random.default_rng(5).uniform(-4, 4, (self.total, 16)).astype(np.float16)
        out[:, :3] = self.rgb_raw
        out[:, 3] = raw
        if self.special:
            for k, (col, value) in enumerate(PLANTED):
                r, j = planted_row(self, k)
                out[self.base[r] + j, col] = value
        return out

    def reference(self, cfg, mean_density=0.003, max_compacted=1 << 14, n_rays=None, counter=None, **kw):
        n = self.n_rays if n_rays is None else n_rays
        v = cfg if isinstance(cfg, dict) else cfg_values(cfg)
        return restate_loss(self.samples(n, counter), self.out(v["density_activation"]), self.pixels, self.px, v, mean_density,
                            128.0, max_compacted, n, background=self.background, **kw)

    def violations(self, cfg):
        ref = self.reference(cfg)
        m, lt = ref["margins"], cfg_values(cfg)["loss_type"]
        bad = (m["t_stop"] < MARGIN_T) | (m["near"] < MARGIN_NEAR) | (m["srgb_knee"] < MARGIN_KNEE)
        if lt == 4:
            bad |= m["huber"] < MARGIN_HUBER
        if lt in SIGN_LOSSES:
            bad |= m["sign"] < MARGIN_SIGN
        # a ray without a composited sample returns nothing that depends on a decision (no sample: prediction and target
        # can both be the background exactly)
        return np.nonzero(bad & (ref["cn"] > 0))[0]

    def enforce_margins(self, cfgs, rounds=20):
        """Draw again every ray that is within a margin of a decision under any of cfgs, until none is."""
        for _ in range(rounds):
            bad = sorted(set(int(r) for c in cfgs for r in self.violations(c)))
            if not bad:
                return self
            for r in bad:
                self.attempt[r] += 1
                self._draw_ray(r)
        raise AssertionError("rays within a decision margin after every redraw")


BACKGROUND = (0.9, 0.3, 0.1)   # not grey, no channel near a knee of the sRGB curve


def make_cfg(pkg, loss="Huber", rgb=ACT_EXP, density=ACT_EXP, near=0.1, **kw):
    base = dict(random_bg_color=0, background_color=BACKGROUND, loss_type=LOSS[loss] if isinstance(loss, str) else loss,
                rgb_activation=rgb, density_activation=density, near_distance=near)
    base.update(kw)
    return pkg.nerf.default_config(2.0, **base)


def config_groups(pkg):
    """The covering set of configurations, by group: name -> [(label, cfg, mean_density)]."""
    g = {"losses": [(name, make_cfg(pkg, name), 0.003) for name in LOSS],
         "activations": [(f"{loss} rgb={r} density={d}", make_cfg(pkg, loss, r, d), 0.003)
                         for loss in ("L2", "Huber") for r in range(4) for d in range(4)],
         "colour_spaces": [(f"{loss} {label}", make_cfg(pkg, loss, **kw), 0.003) for loss in ("L2", "RelativeL2")
                           for label, kw in (("linear_colors", dict(linear_colors=1, color_space_linear=0)),
                                             ("color_space_linear", dict(linear_colors=0, color_space_linear=1)),
                                             ("srgb", dict(linear_colors=0, color_space_linear=0)))],
         "regularisers": [("mean_density 0.02", make_cfg(pkg, "Huber"), 0.02), ("near_distance 0", make_cfg(pkg, "L2", near=0.0), 0.003),
                          ("mean_density 0.02 near 0", make_cfg(pkg, "L1", near=0.0), 0.02)],
         "random_background": [("random_bg_color", make_cfg(pkg, "Huber", random_bg_color=1), 0.003)]}
    return g


GROUPS = ("losses", "activations", "colour_spaces", "regularisers", "random_background")


@functools.lru_cache(maxsize=None)
def _batches(pkg):
    groups = config_groups(pkg)
    every = [c for name in GROUPS for _, c, _ in groups[name]]
    full = Batch(pkg).enforce_margins(every)
    # every loss x every activation pair, for the central differences: short rays, no planted rows
    product = [make_cfg(pkg, loss, r, d) for loss in range(7) for r in range(4) for d in range(4)]
    small = Batch(pkg, n_rays=30, step_pattern=(17, 0, 5, 1, 16, 15, 9), special=False, seed=1).enforce_margins(product)
    return groups, full, small, product


def batches(pkg):
    """(config groups, the 300-ray batch, the 30-ray batch of the central differences, its configurations): built once."""
    return _batches(pkg)


def f16_ulp(x):
    """The spacing of fp16 at |x| (float64 in, 2^-24 in the subnormal range)."""
    _, e = np.frexp(np.abs(np.asarray(x, np.float64)))
    return np.ldexp(1.0, np.maximum(e - 1, -14) - 10)


def in_units(err, companion):
    """err / (2^-24 companion); an error where the companion is zero is infinite."""
    err, companion = np.asarray(err, np.float64), np.asarray(companion, np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(companion > 0, err / (2.0 ** -24 * companion), np.where(err > 0, np.inf, 0.0))


# ---- CPU tests -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pkg():
    from __graft_entry__ import load_package
    return load_package()


def test_pcg32_restatement_matches_the_oracle_and_the_package(pkg, orc):
    r = pkg.nerf.pcg32(RNG_SEED)
    mine, theirs = Pcg32(r.state, r.inc), orc.Rng(RNG_SEED)
    assert (theirs.s.state, theirs.s.inc) == (r.state, r.inc)
    for delta in (0, 1, 16, 5 * 16, 12345678901):
        mine.advance(delta)
        theirs.advance(delta)
        assert [mine.next_uint() for _ in range(3)] == [theirs.next_uint() for _ in range(3)]
        assert [F32(mine.next_float()) for _ in range(3)] == [F32(theirs.next_float()) for _ in range(3)]
    # the pixel's two draws: the position training_pixels reports, before snapping
    cfg = pkg.nerf.default_config(2.0, snap_to_pixel_centers=0)
    b = batches(pkg)[1]
    px = pkg.nerf.training_pixels(b.images, cfg, N_RAYS_TOTAL, b.rng, host=True)
    for i in (0, 1, 150, 306):
        g = Pcg32(b.rng.state, b.rng.inc)
        g.advance(i * 16)
        assert [F32(g.next_float()), F32(g.next_float())] == list(px["uv"][i])


def test_batch_has_every_shape_and_no_ray_near_a_decision(pkg):
    """The builder's promises: the sample counts, the placed stops, the planted values, every alpha kind and masked
    texels among the rays' pixels, depths on both sides of near_distance; and, under every configuration the tests run,
    every ray's margins (the cap on exclusions in the comparisons is zero, which these margins make possible)."""
    groups, full, small, product = batches(pkg)
    assert full.n_rays == 300 and set(STEP_COUNTS) <= set(full.ns.tolist()) and max(RAY_COUNTS) == 300
    for batch, cfgs in ((full, [c for n in GROUPS for _, c, _ in groups[n]]), (small, product)):
        for cfg in cfgs:
            assert batch.violations(cfg).size == 0
    for da in (ACT_EXP, ACT_NONE, ACT_RELU):
        ref = full.reference(make_cfg(pkg, "L2", density=da))
        for r, (n, opaque) in STOPS.items():
            assert full.ns[r] == n and ref["cn"][r] == opaque + 1, (da, r, ref["cn"][r])
    ref = full.reference(make_cfg(pkg))
    kept, stopped = ref["cn"] == full.ns, ref["cn"] < full.ns
    assert kept[full.ns > 0].sum() > 50 and stopped.sum() > 50
    assert ref["margins"]["t_stop"][full.ns > 0].min() >= MARGIN_T
    texel = np.array([full.pixels[i][min(int(v * full.pixels[i].shape[0]), full.pixels[i].shape[0] - 1),
                                     min(int(u * full.pixels[i].shape[1]), full.pixels[i].shape[1] - 1)]
                      for i, (u, v) in zip(full.px["img"], full.px["uv"])])
    masked = (texel == np.array(MASKED)).all(axis=1)
    alpha = texel[~masked, 3]
    assert masked.sum() >= 2 and (alpha == 0).sum() > 10 and (alpha == 255).sum() > 10 and ((alpha > 0) & (alpha < 255)).sum() > 10
    assert (ref["depth"] < NEAR).sum() > 100 and (ref["depth"] > NEAR).sum() > 100 and np.abs(ref["depth"] - NEAR).min() >= MARGIN_NEAR
    out = full.out(ACT_EXP)
    for k, (col, value) in enumerate(PLANTED):
        r, j = planted_row(full, k)
        got = out[full.base[r] + j, col]
        assert got == np.float16(value) and np.signbit(got) == np.signbit(value) and float(np.float16(value)) == value
    assert float(np.nextafter(np.float16(-10), np.float16(-20))) == F16_BELOW_M10
    assert float(np.nextafter(np.float16(-10), np.float16(0))) == F16_ABOVE_M10
    neg = full.out(ACT_NONE)[:, 3] < 0
    assert 3 <= neg.sum()
    t_none = full.reference(make_cfg(pkg, "L2", density=ACT_NONE))
    assert (t_none["weight"] < 0).any()   # negative density: alpha < 0, and both sides must still agree
    # no fp16 gradient overflows, at any ray count the GPU test runs
    for n in RAY_COUNTS:
        for cfg in (make_cfg(pkg, "L2"), make_cfg(pkg, "Huber", ACT_NONE, ACT_NONE)):
            assert np.abs(full.reference(cfg, n_rays=n)["grad"]).max(initial=0.0) < 3e4


def planted_expectations(batch, ref, cfgv, mean_density):
    """Hand-written expectations for the planted samples, from the rules alone: yields (compacted row, column, expected
    gradient element in float64, what is checked)."""
    ls = 128.0 / ref["loss"].size
    l1_on = mean_density < 0.01
    for k, (col, value) in enumerate(PLANTED):
        r, j = planted_row(batch, k)
        hit = np.nonzero((ref["ray"] == r) & (ref["sample"] == j))[0]
        assert hit.size == 1
        i = hit[0]
        if col < 3:
            ra = cfgv["rgb_activation"]
            if ra == ACT_RELU and value == 0.0:       # +0 and -0 are not > 0: no gradient at all
                yield i, col, 0.0, "ReLU at +-0"
            elif ra == ACT_EXP:                       # the value's clamp: slope exp(+-10) beyond it; the l2 term is not clamped
                slope = np.exp(10.0) if value >= 10 else np.exp(-10.0) if value <= -10 else 1.0
                yield i, col, ls * (ref["weight"][i] * ref["ray_gradient"][i, col] * slope + max(0.0, C(1e-4) * value)), "Exponential clamp"
        else:
            da = cfgv["density_activation"]
            near = C(1e-4) if (value > -10.0 and ref["depth"][i] < cfgv["near_distance"]) else 0.0
            l1 = -C(1e-4) if (l1_on and value < 0) else 0.0      # -0.0 < 0 is false
            if da == ACT_RELU and value <= 0:
                yield i, 3, l1 + near, "ReLU density: regularisers only"
            elif da == ACT_EXP and abs(value) >= 15:             # the slope is clamped at exp(+-15), the value is not
                yield i, 3, ref["dmlp_unit"][i] * np.exp(15.0 if value > 0 else -15.0) + l1 + near, "Exponential density slope clamp"
            else:
                yield i, 3, ref["dmlp"][i] + l1 + near, "density regularisers"


def test_restatement_planted_rows(pkg):
    """The restatement itself against the hand-written expectations (the GPU test checks the kernel against the same)."""
    groups, full, _, _ = batches(pkg)
    seen = set()
    for name in ("losses", "activations", "regularisers"):
        for label, cfg, mean in groups[name]:
            v = cfg_values(cfg)
            ref = full.reference(cfg, mean)
            for i, col, want, what in planted_expectations(full, ref, v, mean):
                assert abs(ref["grad"][i, col] - want) <= 1e-12 * max(abs(want), 1e-4), (label, what, ref["grad"][i, col], want)
                seen.add(what)
    assert len(seen) == 5
    # near term at -10 and its two fp16 neighbours, l1 term at +-0, by their literal values (default configuration)
    ref = full.reference(make_cfg(pkg), 0.003)
    reg = {}
    for k, (col, value) in enumerate(PLANTED):
        if col == 3:
            r, j = planted_row(full, k)
            i = np.nonzero((ref["ray"] == r) & (ref["sample"] == j))[0][0]
            assert ref["depth"][i] < NEAR
            reg[value if value != 0 else ("-0" if np.signbit(value) else "+0")] = ref["grad"][i, 3] - ref["dmlp"][i]
    e = C(1e-4)
    want = {"+0": e, "-0": e, -10.0: -e, F16_BELOW_M10: -e, F16_ABOVE_M10: 0.0, -15.0: -e, 15.0: e}
    for key, val in want.items():
        assert abs(reg[key] - val) < 1e-15, (key, reg[key], val)


def _central_difference_error(batch, cfg, live_denominator=False):
    """max over rays of |3 loss_scale d(sum loss)/d(output) - analytic| / the ray's largest gradient element."""
    v = cfg_values(cfg)
    out = batch.out(v["density_activation"])[:, :4].astype(np.float64)
    ref = batch.reference(v, regularisers=False)
    H = 1e-6
    M = int(batch.ns.max())
    # one perturbation per (sample index, column), applied to that sample of every ray at once: rays are independent
    plus = np.broadcast_to(out, (M, 4) + out.shape).copy()
    minus = plus.copy()
    for j in range(M):
        rows = batch.base[batch.ns > j] + j
        for k in range(4):
            plus[j, k, rows, k] += H
            minus[j, k, rows, k] -= H
    fz = {"upd": ref["upd"], "den_pred": ref["den_pred"]}
    s = batch.samples()
    args = (batch.pixels, batch.px, v, 0.003, 128.0, 1 << 14, batch.n_rays)
    lp = restate_loss(s, plus, *args, background=batch.background, freeze=fz, live_denominator=live_denominator)["loss"]
    lm = restate_loss(s, minus, *args, background=batch.background, freeze=fz, live_denominator=live_denominator)["loss"]
    fd = 3 * 128.0 * (lp - lm) / (2 * H)                 # [M, 4, R]
    worst = 0.0
    scale = np.zeros(batch.n_rays)
    np.maximum.at(scale, ref["ray"], np.abs(ref["grad"]).max(axis=1))
    for i in range(ref["ray"].size):
        r, j = ref["ray"][i], ref["sample"][i]
        for k in range(4):
            act = v["rgb_activation"] if k < 3 else v["density_activation"]
            if act == ACT_RELU and abs(ref["raw"][i, k]) <= H:
                continue
            if scale[r] > 0:
                worst = max(worst, abs(fd[j, k, r] - ref["grad"][i, k]) / scale[r])
    return worst


def test_gradient_matches_central_differences_of_the_loss(pkg):
    """The restatement's analytic dL/doutput (regularisers removed) against central differences (step 1e-6) of its own
    float64 loss, every stop and compaction decision frozen: grad = 3 loss_scale d(sum loss)/d(output), since the
    reference divides the loss by 3 and not the gradient. All 7 losses x 16 activation pairs on a 30-ray batch. For
    MAPE, SMAPE and RelativeL2 the reference's gradient treats the denominator as a constant, so the differenced loss is
    evaluated with the denominator frozen at the unperturbed prediction. ReLU inputs within the step of 0 are skipped.
    Bound: 1e-6 of the ray's largest gradient element (measured: 2.5e-7)."""
    _, _, small, product = batches(pkg)
    worst = 0.0
    for cfg in product:
        e = _central_difference_error(small, cfg)
        worst = max(worst, e)
        assert e <= 1e-6, (cfg.loss_type, cfg.rgb_activation, cfg.density_activation, e)
    print(f"central differences: worst |fd - grad| / max|grad of the ray| = {worst:.2e} over {len(product)} configurations")


def test_central_differences_see_a_wrong_gradient(pkg):
    """The negative control: with the denominator of MAPE, SMAPE or RelativeL2 live, the differenced loss is not the
    loss the reference's gradient belongs to, and the same check fails."""
    _, _, small, _ = batches(pkg)
    for loss in ("MAPE", "SMAPE", "RelativeL2"):
        e = _central_difference_error(small, make_cfg(pkg, loss), live_denominator=True)
        print(f"live denominator, {loss}: {e:.2e}")
        assert e > 1e-3


def oracle_loss(orc, batch, cfg, mean_density, max_compacted=1 << 14, n_rays=None, counter=None):
    n = batch.n_rays if n_rays is None else n_rays
    s = batch.samples(n, counter)
    out = batch.out(int(cfg.density_activation))
    r = orc.nerf_compute_loss(cfg, batch.images, batch.pixels, n, orc.pcg(batch.rng.state, batch.rng.inc), max_compacted, s,
                              out.view(np.uint16), mean_density, n_div=N_RAYS_TOTAL)
    r["numsteps"] = s["numsteps"]
    return r


def compare(ref, got_loss, got_grad16, got_numsteps, got_counter, got_coords, k):
    """Everything a loss pass returns against the restatement `ref`: integers and coordinates equal; loss and fp16
    gradient in units of 2^-24 companion (half an fp16 ulp of the float64 value taken off the gradient's error).
    Returns the worst (loss, gradient) in those units; asserts them <= k when k is given, no element left out."""
    assert int(got_counter) == ref["compacted_counter"]
    np.testing.assert_array_equal(np.asarray(got_numsteps).view(np.uint32).reshape(-1, 2), ref["numsteps"])
    n = ref["row"].size
    np.testing.assert_array_equal(np.asarray(got_coords)[ref["row"]].view(np.uint32), ref["coords_compacted"].view(np.uint32))
    got_loss = np.asarray(got_loss, np.float64)
    assert not got_loss[ref["cnum"] == 0].any()
    ul = in_units(np.abs(got_loss - ref["loss"]), ref["loss_companion"])
    g = np.asarray(got_grad16)[ref["row"], :4].astype(np.float64)
    assert np.isfinite(g).all()
    err = np.maximum(np.abs(g - ref["grad"]) - 0.5 * f16_ulp(ref["grad"]), 0.0)
    ug = in_units(err, ref["grad_companion"]) if n else np.zeros(1)
    if k is not None:
        flip = f16_ulp(ref["grad"])   # one fp16 ulp for a rounding that flips
        bound = k * 2.0 ** -24 * ref["grad_companion"] + 0.5 * f16_ulp(ref["grad"]) + flip
        bad = np.abs(g - ref["grad"]) > bound
        assert not bad.any(), (int(bad.sum()), g[bad][:4], ref["grad"][bad][:4])
        assert (ul <= k).all(), (ul.max(), int(ul.argmax()))
    return float(ul.max(initial=0.0)), float(ug.max(initial=0.0))


def test_oracle_agrees_with_the_restatement(pkg, orc):
    """The float32 C oracle against the float64 restatement on the 300-ray batch, every configuration: compacted counts,
    {n, base} and coordinates equal; loss and gradient within K32 units of 2^-24 companion. This is float32 reference
    arithmetic against float64: the measurement the GPU tolerance (4 K32) is set from."""
    groups, full, _, _ = batches(pkg)
    worst_l = worst_g = 0.0
    for name in GROUPS:
        for label, cfg, mean in groups[name]:
            ref = full.reference(cfg, mean)
            o = oracle_loss(orc, full, cfg, mean)
            ul, ug = compare(ref, o["loss"], orc.f16_bits_to_f32(o["dloss_doutput"]), o["numsteps"], o["compacted_counter"][0],
                             o["coords_compacted"], None)
            worst_l, worst_g = max(worst_l, ul), max(worst_g, ug)
            assert max(ul, ug) <= K32, (label, ul, ug)
    print(f"K32: oracle vs float64, loss {worst_l:.2f}, gradient {worst_g:.2f} units of 2^-24 companion (constant K32 = {K32})")
    # compaction: cut inside a ray, at a ray boundary, long before the end, and a ray counter below n_rays
    cfg = make_cfg(pkg)
    for max_c, counter in compaction_cases(full, cfg):
        ref = full.reference(cfg, max_compacted=max_c, counter=counter)
        o = oracle_loss(orc, full, cfg, 0.003, max_compacted=max_c, counter=counter)
        compare(ref, o["loss"], orc.f16_bits_to_f32(o["dloss_doutput"]), o["numsteps"], o["compacted_counter"][0],
                o["coords_compacted"], K32)


def compaction_cases(batch, cfg):
    """(max_compacted, ray counter): larger than the total; cutting a ray in the middle; ending exactly at a ray's end;
    so small that later rays get {0, base}; a ray counter below n_rays."""
    ref = batch.reference(cfg)
    total, end = ref["compacted_counter"], ref["cbase"] + ref["cn"]
    mid = int(np.nonzero(ref["cn"] > 8)[0][40])
    return [(total + 100, None), (int(ref["cbase"][mid] + 3), None), (int(end[mid]), None), (40, None), (total + 100, 211)]


def test_compaction_cases_are_what_they_claim(pkg):
    _, full, _, _ = batches(pkg)
    cfg = make_cfg(pkg)
    cases = compaction_cases(full, cfg)
    full_ref = full.reference(cfg)
    r = full.reference(cfg, max_compacted=cases[1][0])
    cut = np.nonzero((r["cnum"] > 0) & (r["cnum"] < r["cn"]))[0]
    assert cut.size == 1 and (r["cnum"][cut[0] + 1:] == 0).all() and not r["loss"][cut[0] + 1:].any()
    r = full.reference(cfg, max_compacted=cases[2][0])
    assert ((r["cnum"] == r["cn"]) | (r["cnum"] == 0)).all() and (r["cnum"][r["cn"] > 0] == 0).any()
    assert r["grad"].shape[0] == cases[2][0]
    r = full.reference(cfg, max_compacted=cases[3][0])
    assert (r["cnum"] == 0).sum() > 250 and r["compacted_counter"] == full_ref["compacted_counter"]
    r = full.reference(cfg, counter=cases[4][1])
    assert not r["loss"][211:].any() and r["compacted_counter"] == full_ref["cn"][:211].sum()
    np.testing.assert_array_equal(r["numsteps"][211:], full.samples()["numsteps"][211:])


def test_config_switches_reach_the_engine(pkg):
    """default_config overrides for every switch of the loss pass are stored as given (none is rejected or folded)."""
    for r in range(4):
        for d in range(4):
            c = pkg.nerf.default_config(1.0, rgb_activation=r, density_activation=d)
            assert (c.rgb_activation, c.density_activation) == (r, d)
    for name, k in LOSS.items():
        assert pkg.nerf.LOSS[name] == k and pkg.nerf.default_config(1.0, loss_type=k).loss_type == k
    c = pkg.nerf.default_config(1.0, color_space_linear=0, linear_colors=0, random_bg_color=0, background_color=BACKGROUND)
    assert (c.color_space_linear, c.linear_colors, c.random_bg_color) == (0, 0, 0)
    assert list(c.background_color) == [F32(x) for x in BACKGROUND]
    assert pkg.nerf.ACT == {"None": 0, "ReLU": 1, "Logistic": 2, "Exponential": 3}
    # the pyngp setters (nerf.rgb_activation, nerf.density_activation, nerf.training.loss_type and the knobs) keep every value
    ngp = pkg.pyngp()
    tb = ngp.Testbed()
    for name, k in pkg.nerf.ACT.items():
        tb.nerf.rgb_activation = tb.nerf.density_activation = getattr(ngp.NerfActivation, name)
        assert (int(tb.nerf.rgb_activation), int(tb.nerf.density_activation)) == (k, k)
    for name, k in (("L2", 0), ("L1", 1), ("Mape", 2), ("Smape", 3), ("Huber", 4), ("LogL1", 5), ("RelativeL2", 6)):
        tb.nerf.training.loss_type = getattr(ngp.LossType, name)
        assert int(tb.nerf.training.loss_type) == k
    tb.nerf.training.random_bg_color, tb.nerf.training.linear_colors, tb.nerf.training.near_distance = False, True, 0.0
    assert (bool(tb.nerf.training.random_bg_color), bool(tb.nerf.training.linear_colors), tb.nerf.training.near_distance) == (False, True, 0.0)
