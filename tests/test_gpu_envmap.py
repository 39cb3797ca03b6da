"""The trainable environment map (train_envmap) on the GPU: the device lookup, the exact gradient deposit, the loss pass
with a map bound (value and gradient), the map's optimizer, reproducible training, rendering, snapshots, the
data-parallel refusal and the pyngp surface. The float64 restatement of read_envmap and its bound live in
test_envmap_host.py."""
import ctypes as C
import json

import numpy as np
import pytest
import torch

from test_envmap_host import RESOLUTIONS, check_lookup, directions, smooth_map

pytestmark = pytest.mark.gpu

ENVMAP_SECTION = {  # configs/nerf/base.json "envmap" (the keys this chain reads)
    "loss": {"otype": "RelativeL2"},
    "optimizer": {"otype": "Ema", "decay": 0.99, "nested": {
        "otype": "ExponentialDecay", "decay_start": 10000, "decay_interval": 5000, "decay_base": 0.33, "nested": {
            "otype": "Adam", "learning_rate": 1e-2, "beta1": 0.9, "beta2": 0.99, "epsilon": 1e-10, "l2_reg": 1e-10}}},
}


@pytest.fixture(scope="module")
def pkg():
    from __graft_entry__ import load_package
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return load_package()


# ---- lookup ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("width,height", RESOLUTIONS)
def test_device_lookup_matches_the_float64_restatement(pkg, width, height):
    d = directions()
    tex, wt = pkg.nerf.envmap_lookup(width, height, torch.from_numpy(d).cuda())
    check_lookup(width, height, d, tex.cpu().numpy(), wt.cpu().numpy())


# ---- deposit --------------------------------------------------------------------------------------------------------
def exact_deposit(width, height, texels, weights, values):
    """Every contribution fp16(value) * fp16(weight), rounded to fp16 (numpy float16 arithmetic: the product is exact in
    float32 and rounds once), summed exactly in integers of 2^-24 and rounded once to float32. The sums here stay far
    below 2^53, so the int64 -> float64 step is exact and float64 -> float32 is the one rounding."""
    v16 = values.astype(np.float16)                      # [n, 3]
    w16 = weights.astype(np.float16)                     # [n, 4]
    contrib = (v16[:, None, :] * w16[:, :, None]).astype(np.float16)  # [n, corner, channel]
    units = contrib.astype(np.float64) * 2.0 ** 24
    assert np.array_equal(units, np.rint(units))          # every fp16 value is a multiple of 2^-24
    acc = np.zeros(width * height * 4, np.int64)
    idx = texels[:, :, None] * 4 + np.arange(3)[None, None, :]
    np.add.at(acc, idx.reshape(-1), units.astype(np.int64).reshape(-1))
    assert np.abs(acc).max() < 2 ** 53
    return (acc.astype(np.float64) * 2.0 ** -24).astype(np.float32).reshape(height, width, 4)


@pytest.mark.parametrize("case,width,height", [("random", 16, 8), ("one_texel", 16, 8), ("random", 2, 2), ("random", 5, 3)])
def test_deposit_is_the_exact_sum(pkg, case, width, height):
    n = 4096
    g = np.random.default_rng(11)
    if case == "one_texel":  # every direction inside one texel's cell: 4096 contributions per corner channel
        base = np.array([0.3, 0.2, 0.93], np.float64)
        d = base[None] + 1e-3 * g.standard_normal((n, 3))
    else:
        d = g.standard_normal((n, 3))
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    values = (g.standard_normal((n, 3)) * np.array([50.0, 1.0, 1e-3])).astype(np.float16)  # large, moderate and tiny values
    values[::7, 1] = 0
    dt, vt = torch.from_numpy(d).cuda(), torch.from_numpy(values).cuda()
    tex, wt = pkg.nerf.envmap_lookup(width, height, dt)
    grad = pkg.nerf.envmap_deposit(width, height, dt, vt).cpu().numpy()
    ref = exact_deposit(width, height, tex.cpu().numpy(), wt.cpu().numpy(), values)
    if case == "one_texel":
        assert len(np.unique(tex.cpu().numpy()[:, 0])) == 1
    assert np.abs(ref).max() > 0
    np.testing.assert_array_equal(grad.view(np.uint32), ref.view(np.uint32))
    assert not grad[..., 3].any()                                  # alpha's gradient stays zero
    again = pkg.nerf.envmap_deposit(width, height, dt, vt).cpu().numpy()
    np.testing.assert_array_equal(again.view(np.uint32), grad.view(np.uint32))


def test_deposit_non_finite_value_poisons_its_channels_only(pkg):
    w, h = 8, 4
    d = directions(64, seed=5)[-64:]
    values = np.ones((64, 3), np.float16)
    values[3, 1] = np.inf
    values[9, 2] = np.nan
    dt = torch.from_numpy(d).cuda()
    tex, wt = pkg.nerf.envmap_lookup(w, h, dt)
    grad = pkg.nerf.envmap_deposit(w, h, dt, torch.from_numpy(values).cuda()).cpu().numpy().reshape(-1, 4)
    tex, wt = tex.cpu().numpy(), wt.cpu().numpy()
    bad = np.zeros((w * h, 4), bool)
    bad[tex[3], 1] = True   # inf * weight: inf, or NaN where the fp16 weight is 0
    bad[tex[9], 2] = True
    assert np.isnan(grad[bad]).all() and np.isfinite(grad[~bad]).all()


# ---- loss pass --------------------------------------------------------------------------------------------------------
def opaque_dataset(pkg, seed=0, n_images=2, res=8):
    g = np.random.default_rng(seed)
    S = pkg.synthetic
    ims, pix = [], []
    for c2w in S.camera_poses(n_images, seed=seed):
        ims.append(pkg.nerf.make_image(res, res, pkg.nerf.nerf_matrix_to_ngp(c2w), camera_angle_x=S.LEGO_CAMERA_ANGLE_X))
        px = g.integers(0, 256, (res, res, 4), dtype=np.uint8)
        px[..., 3] = 255  # opaque: the target does not depend on the background
        pix.append(px)
    return pkg.nerf.NerfDataset(ims, pix)


def crafted_samples(n_rays=256, max_steps=32, seed=0):
    """A sampler's output made by hand: n_rays rays of 0..max_steps samples (some with none), random directions, step
    sizes large enough that dense rays stop early. Returns the samples dict (host) and the network output: the first
    third of the rays is dense (they stop before their last sample), the rest is thin (transmittance left)."""
    g = np.random.default_rng(seed)
    numsteps = g.integers(3, max_steps + 1, n_rays).astype(np.uint32)
    numsteps[::17] = 0
    base = np.concatenate([[0], np.cumsum(numsteps)[:-1]]).astype(np.uint32)
    total = int(numsteps.sum())
    coords = g.random((total, 7)).astype(np.float32)
    coords[:, 3] = g.uniform(0.5, 1.0, total)   # warped dt: steps of 0.11 .. 0.22
    rays = np.concatenate([g.random((n_rays, 3)), 3.0 * g.standard_normal((n_rays, 3))], axis=1).astype(np.float32)  # unnormalized d
    out = np.zeros((total, 16), np.float16)
    out[:, :3] = g.uniform(-2.0, 2.0, (total, 3))
    dense = np.repeat(np.arange(n_rays) < n_rays // 3, numsteps)
    out[:, 3] = np.where(dense, g.uniform(4.0, 5.0, total), g.uniform(-6.0, -3.0, total))
    samples = {"ray_indices": np.arange(n_rays, dtype=np.uint32), "rays": rays,
               "numsteps": np.stack([numsteps, base], axis=1), "coords": coords,
               "counters": np.array([n_rays, total], np.uint32)}
    return samples, out


def to_device(samples):
    return {k: torch.from_numpy(v.view(np.int32) if v.dtype == np.uint32 else v).cuda() for k, v in samples.items()}


def run_loss(pkg, ds, cfg, samples, out, n_rays, **kw):
    s = to_device(samples)
    mean = torch.tensor([0.003], device="cuda")
    got = pkg.nerf.compute_loss(ds, cfg, n_rays, pkg.nerf.pcg32(3), 1 << 14, s, torch.from_numpy(out).cuda(), mean, **kw)
    torch.cuda.synchronize()
    return got, s


def test_loss_with_a_constant_map_equals_the_constant_background(pkg):
    """A constant-colour map with alpha 0 over background_color 0 against the existing path with that colour as
    background_color. The colours are chosen so that srgb_to_linear is exact arithmetic (1 -> 1; s <= 0.04045 -> s / 12.92).
    The map's background is sum_k w_k c: four products and three sums, each rounding by half an ulp, over weights whose
    own sum is 1 within 4 * 2^-23 (test_envmap_host): within 6 ulp (fp32) of c. Linear colours, L2: prediction and
    target move by at most that (times T <= 1, 1 - alpha <= 1), their difference d by DELTA = 6 ulp(c_max) + 2 ulp(2)
    (the roundings of two sums of magnitude <= 2). Loss per ray: (2 |d| DELTA + DELTA^2) / n_rays. dL/doutput: rgb rows
    scale * w * 2 DELTA * rgb' with w, rgb' <= 1; the density row scale * sigma' dt * sum_c 2 DELTA |T rgb_c - suffix_c|
    with the bracket <= 2: everything is below scale * max(1, sigma' dt) * 12 DELTA, plus one fp16 ulp for a rounding
    that flips."""
    n_rays = 256
    ds = opaque_dataset(pkg)
    samples, out = crafted_samples(n_rays)
    srgb = np.array([1.0, 0.04, 0.03], np.float32)
    lin = np.where(srgb <= 0.04045, srgb / np.float32(12.92), np.float32(1.0)).astype(np.float32)
    kw = dict(random_bg_color=0, linear_colors=1, loss_type=0, rgb_activation=2, density_activation=3)
    cfg_ref = pkg.nerf.default_config(1.0, background_color=list(srgb), **kw)
    cfg_env = pkg.nerf.default_config(1.0, background_color=[0.0, 0.0, 0.0], **kw)
    ref, s_ref = run_loss(pkg, ds, cfg_ref, samples, out, n_rays)
    envmap = torch.zeros((4, 8, 4), device="cuda")
    envmap[..., :3] = torch.from_numpy(lin).cuda()
    got, s_env = run_loss(pkg, ds, cfg_env, samples, out, n_rays, envmap=envmap)
    # compaction does not depend on the background
    assert int(ref["compacted_counter"][0]) == int(got["compacted_counter"][0]) > 0
    np.testing.assert_array_equal(s_ref["numsteps"].cpu().numpy(), s_env["numsteps"].cpu().numpy())
    np.testing.assert_array_equal(ref["coords_compacted"].cpu().numpy(), got["coords_compacted"].cpu().numpy())
    ns = s_env["numsteps"].cpu().numpy()[:, 0]
    assert (ns < samples["numsteps"][:, 0]).any() and (ns == samples["numsteps"][:, 0]).any()  # stopped early / kept all
    delta = 6 * np.spacing(np.float32(1.0)) + 2 * np.spacing(np.float32(2.0))
    d_max = 2.0
    l_ref, l_got = ref["loss"].cpu().numpy().astype(np.float64), got["loss"].cpu().numpy().astype(np.float64)
    print(f"constant map: max |loss - ref| = {np.abs(l_got - l_ref).max():.3e} (bound {(2 * d_max * delta + delta ** 2) / n_rays:.3e})")
    assert np.abs(l_got - l_ref).max() <= (2 * d_max * delta + delta ** 2) / n_rays
    assert l_ref.max() > 0
    dt = samples["coords"][:, 3].astype(np.float64) * (np.sqrt(3) / 1024 * 127) + np.sqrt(3) / 1024
    sig_dt = max(1.0, float((np.exp(out[:, 3].astype(np.float64)) * dt).max()))
    g_ref = ref["dloss_doutput"].cpu().numpy()
    g_got = got["dloss_doutput"].cpu().numpy().astype(np.float64)
    tol = (128.0 / n_rays) * sig_dt * 12 * delta + np.spacing(np.abs(g_ref)).astype(np.float64)
    err = np.abs(g_got - g_ref.astype(np.float64))
    print(f"constant map: max |dL/doutput - ref| = {err.max():.3e}, worst err / tol = {(err / tol).max():.3f}")
    assert (err <= tol).all() and np.abs(g_ref).max() > 0


def test_loss_gradient_matches_central_differences(pkg):
    """dL/d(envmap) of a 4x2 map against central differences of the summed loss, L2 for both losses, linear colours,
    opaque training pixels. The loss is a quadratic in the map, so central differences have no truncation error and the
    step can be large (H = 0.25). loss[i] = mean_c (pred - target)^2 / n_rays and the reference deposits
    loss_scale / n_rays * T * 2 (pred - target) per channel (no 1 / 3): gradient = 3 * loss_scale * d(sum loss)/d(texel).
    Bound per texel channel: three fp16 roundings per contribution (value, weight, product), 3 * 2^-11 relative, of
    contributions whose magnitudes sum to at most loss_scale / n_rays * 2 |d|max * sum_rays w_k (|d|max = 1 + the largest
    background, the map's value plus cfg's: rgb in (0, 1) through the logistic, target in [0, 1]), plus 3 * 2^-25 absolute per contribution where a
    product is subnormal in fp16, plus the differences' own noise: each loss[i] carries at most 8 fp32 roundings."""
    n_rays, w, h, H = 256, 4, 2, 0.25
    ds = opaque_dataset(pkg, seed=1)
    samples, out = crafted_samples(n_rays, seed=1)
    cfg = pkg.nerf.default_config(1.0, background_color=[1.0, 0.04, 0.03], random_bg_color=0, linear_colors=1, loss_type=0,
                                  rgb_activation=2, density_activation=3)  # a background behind the map: its alpha matters
    g = np.random.default_rng(2)
    env0 = g.uniform(0.2, 0.8, (h, w, 4)).astype(np.float32)
    env0[..., 3] = g.uniform(0.0, 0.5, (h, w))

    def total(env):
        got, _ = run_loss(pkg, ds, cfg, samples, out, n_rays, envmap=torch.from_numpy(env).cuda(), envmap_loss="L2")
        return got["loss"].cpu().numpy().astype(np.float64).sum()

    grad_t = torch.full((h, w, 4), 7.0, device="cuda")  # overwritten, not accumulated
    got, s = run_loss(pkg, ds, cfg, samples, out, n_rays, envmap=torch.from_numpy(env0).cuda(), envmap_gradient=grad_t,
                      envmap_loss="L2")
    grad = grad_t.cpu().numpy().astype(np.float64)
    assert not grad[..., 3].any()
    fd = np.zeros((h, w, 3))
    for y in range(h):
        for x in range(w):
            for c in range(3):
                ep, em = env0.copy(), env0.copy()
                ep[y, x, c] += H
                em[y, x, c] -= H
                fd[y, x, c] = (total(ep) - total(em)) / (2 * H)
    expect = 3 * 128.0 * fd
    # the bound, from the rays that may deposit (all of them, an upper bound) and the device's weights
    d = samples["rays"][:, 3:] / np.linalg.norm(samples["rays"][:, 3:], axis=1, keepdims=True)
    tex, wt = pkg.nerf.envmap_lookup(w, h, torch.from_numpy(d.astype(np.float32)).cuda())
    wsum, count = np.zeros(w * h), np.zeros(w * h)
    np.add.at(wsum, tex.cpu().numpy().reshape(-1), wt.cpu().numpy().astype(np.float64).reshape(-1))
    np.add.at(count, tex.cpu().numpy().reshape(-1), 1)
    d_max = 2.0 + float(env0.max()) + H   # prediction <= 1 + map + background (<= 1), target in [0, 1]
    loss_sum = got["loss"].cpu().numpy().astype(np.float64).sum()
    fd_noise = 3 * 128.0 * (2 * 8 * 2.0 ** -24 * 2 * loss_sum) / (2 * H)
    bound = (3 * 2.0 ** -11 * (128.0 / n_rays) * 2 * d_max * wsum + 3 * 2.0 ** -25 * count + fd_noise).reshape(h, w, 1)
    err = np.abs(grad[..., :3] - expect)
    print(f"envmap gradient: max |grad| = {np.abs(expect).max():.3e}, max err = {err.max():.3e}, worst err / bound = {(err / bound).max():.3f}")
    assert np.abs(expect).max() > 10 * bound.max()   # the check can see the gradient
    assert (err <= bound).all()
    # rays that stopped early, and rays without samples, deposit nothing: with every ray dense the gradient is zero
    out_dense = out.copy()
    out_dense[:, 3] = 5.0
    grad_t.fill_(7.0)
    got, s = run_loss(pkg, ds, cfg, samples, out_dense, n_rays, envmap=torch.from_numpy(env0).cuda(), envmap_gradient=grad_t,
                      envmap_loss="L2")
    ns = s["numsteps"].cpu().numpy()[:, 0]
    assert ((ns < samples["numsteps"][:, 0]) | (ns == 0)).all() and (ns > 0).any()
    assert not grad_t.cpu().numpy().any()


# ---- optimizer --------------------------------------------------------------------------------------------------------
def test_envmap_optimizer_follows_the_recurrence(pkg):
    """Five steps of the "envmap" chain on a 4x2 map against a float32 numpy restatement (same operations, same order).
    powf / sqrtf differ between the device and numpy by a few ulp: each step's update (at most ~lr in magnitude) is
    allowed 16 ulp relative, lr * 2^-20, plus the half ulp of the parameter it is subtracted from (|w| < 1: 2^-24)."""
    f32 = np.float32
    n, steps, ls = 32, 5, f32(128.0)
    opt = ENVMAP_SECTION["optimizer"]
    d, ad = f32(opt["decay"]), opt["nested"]["nested"]
    lr, b1, b2, eps = f32(ad["learning_rate"]), f32(ad["beta1"]), f32(ad["beta2"]), f32(ad["epsilon"])
    g = np.random.default_rng(5)
    w0 = g.uniform(0.1, 0.9, n).astype(np.float32)
    grads = (g.standard_normal((steps, n)) * 3.0).astype(np.float32)
    grads[:, 3::4] = 0      # alpha: never a gradient
    grads[:, 5] = 0         # a colour channel that never gets one
    grads[1:3, 8] = 0       # one that skips two steps
    st = {k: torch.zeros(n, device="cuda") for k in ("first_moments", "second_moments", "ema", "ema_params")}
    st["params"] = torch.from_numpy(w0).cuda()
    st["param_steps"] = torch.zeros(n, dtype=torch.int32, device="cuda")
    w, m1, m2, cnt, ema = w0.copy(), np.zeros(n, f32), np.zeros(n, f32), np.zeros(n, np.int32), np.zeros(n, f32)
    for k in range(steps):
        pkg.nerf.envmap_optimizer_step(opt, k, st, torch.from_numpy(grads[k]).cuda(), loss_scale=float(ls))
        torch.cuda.synchronize()
        w_dev = st["params"].cpu().numpy()
        gk = grads[k] / ls
        act = gk != 0
        m1 = np.where(act, b1 * m1 + (f32(1) - b1) * gk, m1).astype(f32)
        m2 = np.where(act, b2 * m2 + (f32(1) - b2) * (gk * gk), m2).astype(f32)
        cnt = cnt + act
        with np.errstate(divide="ignore", invalid="ignore"):
            lr_s = lr * np.sqrt(f32(1) - np.power(b2, cnt.astype(f32), dtype=f32)) / (f32(1) - np.power(b1, cnt.astype(f32), dtype=f32))
            w = np.where(act, w - lr_s / (np.sqrt(m2) + eps) * m1, w).astype(f32)
        np.testing.assert_array_equal(st["param_steps"].cpu().numpy(), cnt)
        np.testing.assert_allclose(st["first_moments"].cpu().numpy(), m1, rtol=4 * 2.0 ** -23, atol=0)
        np.testing.assert_allclose(st["second_moments"].cpu().numpy(), m2, rtol=4 * 2.0 ** -23, atol=0)
        assert np.abs(w_dev - w).max() <= (k + 1) * (float(lr) * 2.0 ** -20 + 2.0 ** -24)
        # the EMA follows ema_step over the device's own parameters, bit for bit; its debiased form within powf's ulps
        ema = (d * ema + (f32(1) - d) * w_dev).astype(f32)
        np.testing.assert_array_equal(st["ema"].cpu().numpy().view(np.uint32), ema.view(np.uint32))
        debias = f32(1) - np.power(d, f32(k + 1), dtype=f32)
        np.testing.assert_allclose(st["ema_params"].cpu().numpy(), ema / debias, rtol=8 * 2.0 ** -23, atol=0)
    w_dev = st["params"].cpu().numpy()
    never = np.zeros(n, bool)
    never[3::4] = True
    never[5] = True
    np.testing.assert_array_equal(w_dev[never].view(np.uint32), w0[never].view(np.uint32))  # did not move
    assert (st["param_steps"].cpu().numpy()[never] == 0).all() and st["param_steps"].cpu().numpy()[8] == steps - 2
    assert (w_dev[~never] != w0[~never]).all()


# ---- training -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small_scene(pkg):
    return pkg.synthetic.lego_like_dataset(n_images=6, width=64, height=64, seed=3)


def make_run(pkg, ds, envmap_res=(16, 8), train=True, batch=1 << 14, section=ENVMAP_SECTION, aabb_scale=1.0, **cfg_kw):
    ncfg = pkg.nerf_config("C2")
    ncfg["encoding"]["log2_hashmap_size"] = 14
    net = pkg.create_nerf_network(ncfg)
    tr = pkg.Trainer(net, ncfg["optimizer"], seed=1337)
    cfg = pkg.nerf.default_config(aabb_scale, target_batch_size=batch, **cfg_kw)
    run = pkg.nerf.NerfTraining(net, tr, ds, cfg, seed=1337)
    if envmap_res is not None:
        run.set_envmap(resolution=envmap_res, loss=section["loss"]["otype"], optimizer=section["optimizer"])
    run.train_envmap = train
    return run, net, tr, cfg


def test_training_with_train_envmap_is_reproducible(pkg, small_scene):
    """The same 20 steps twice: the map, its EMA and the network come out byte-identical; alpha never moves."""
    res = []
    for _ in range(2):
        run, net, tr, cfg = make_run(pkg, small_scene)
        assert run.train_envmap and run.envmap().shape == (8, 16, 4) and not run.envmap().any()
        for _ in range(20):
            run.train_step(get_loss=False)
        torch.cuda.synchronize()
        res.append((run.envmap("params"), run.envmap("ema"), run.envmap("gradient"), tr.params.cpu().numpy().copy(),
                    run.envmap("param_steps")))
    a, b = res
    for x, y in zip(a, b):
        np.testing.assert_array_equal(x.view(np.uint8), y.view(np.uint8))
    assert np.abs(a[0][..., :3]).max() > 0 and np.isfinite(a[0]).all() and np.isfinite(a[1]).all()
    assert not a[0][..., 3].any() and not a[4][..., 3].any()     # alpha: no gradient, no step
    assert a[4][..., :3].max() > 0 and a[4].max() <= 20
    assert not np.array_equal(a[0], a[1])                          # the EMA lags the raw parameters


def test_train_envmap_without_a_map_and_a_map_without_training(pkg, small_scene):
    """train_envmap without a map does nothing (the step is the plain one); a map without train_envmap stays as set."""
    plain, _, tr0, _ = make_run(pkg, small_scene, envmap_res=None, train=False)
    nomap, _, tr1, _ = make_run(pkg, small_scene, envmap_res=None, train=True)
    for _ in range(5):
        plain.train_step(get_loss=False)
        nomap.train_step(get_loss=False)
    torch.cuda.synchronize()
    assert nomap.envmap() is None
    np.testing.assert_array_equal(tr0.params.cpu().numpy().view(np.uint16), tr1.params.cpu().numpy().view(np.uint16))
    fixed, _, _, _ = make_run(pkg, small_scene, train=False)
    init = np.random.default_rng(0).random((8, 16, 4)).astype(np.float32)
    fixed.set_envmap(init)
    for _ in range(3):
        fixed.train_step(get_loss=False)
    np.testing.assert_array_equal(fixed.envmap(), init)
    np.testing.assert_array_equal(fixed.envmap("ema"), init)
    fixed.set_envmap()
    assert fixed.envmap() is None


def test_snapshot_round_trip_keeps_the_map_and_its_optimizer(pkg, small_scene, tmp_path):
    """The map, its EMA, moments and step counters come back bit for bit, and the step after loading is the step the
    saving trainer takes next. A snapshot holds neither random number generator (as in the reference), so the loading
    trainer has taken the same number of steps, from another map, before it loads."""
    run, net, tr, cfg = make_run(pkg, small_scene)
    for _ in range(6):
        run.train_step(get_loss=False)
    path = str(tmp_path / "env.ingp")
    run.save_snapshot(path, include_optimizer_state=True)
    saved = {k: run.envmap(k) for k in run.ENVMAP_ARRAYS if k != "gradient"}
    run2, net2, tr2, _ = make_run(pkg, small_scene, envmap_res=(4, 2))  # the "envmap" section's loss and optimizer: configuration
    run2.set_envmap(np.random.default_rng(9).random((2, 4, 4)).astype(np.float32))
    for _ in range(6):
        run2.train_step(get_loss=False)
    run2.load_snapshot(path)
    for k, v in saved.items():
        np.testing.assert_array_equal(run2.envmap(k).view(np.uint32), v.view(np.uint32), err_msg=k)
    run.train_step(get_loss=False)
    run2.train_step(get_loss=False)
    torch.cuda.synchronize()
    exact = all(np.array_equal(run2.envmap(k).view(np.uint32), run.envmap(k).view(np.uint32)) for k in run.ENVMAP_ARRAYS)
    print(f"snapshot: the step after loading equals the saving trainer's next step: {exact}")
    for k in run.ENVMAP_ARRAYS:
        np.testing.assert_array_equal(run2.envmap(k).view(np.uint32), run.envmap(k).view(np.uint32), err_msg=k)
    np.testing.assert_array_equal(tr2.params.cpu().numpy().view(np.uint16), tr.params.cpu().numpy().view(np.uint16))
    # a snapshot without the member loads as before and leaves no map behind
    plain, _, _, _ = make_run(pkg, small_scene, envmap_res=None, train=False)
    plain.train_step(get_loss=False)
    p2 = str(tmp_path / "plain.ingp")
    plain.save_snapshot(p2)
    fresh, _, _, _ = make_run(pkg, small_scene, envmap_res=None, train=False)
    fresh.load_snapshot(p2)
    assert fresh.envmap() is None


def test_train_envmap_is_refused_with_data_parallelism(pkg, small_scene):
    from instant_ngp_amd.dp import ALLREDUCE_FN
    hook = ALLREDUCE_FN(lambda *a: 1)   # never called: the step is not run
    lib = pkg.nerf.lib()
    run, _, _, _ = make_run(pkg, small_scene, train=True)
    assert lib.ngp_nerf_trainer_set_data_parallel(run.handle, 0, 2, C.cast(hook, C.c_void_p), None) != 0
    assert "train_envmap is single-GPU" in lib.ngp_last_error().decode()
    run2, _, _, _ = make_run(pkg, small_scene, train=False)
    assert lib.ngp_nerf_trainer_set_data_parallel(run2.handle, 0, 2, C.cast(hook, C.c_void_p), None) == 0
    with pytest.raises(pkg.NgpError, match="train_envmap is single-GPU"):
        run2.train_envmap = True
    assert not run2.train_envmap


# ---- rendering --------------------------------------------------------------------------------------------------------
def pixel_directions(im, W, H):
    """k_render_init's ray directions of a camera's pixels at sample 0 (pixel centres), float32, normalized."""
    f32 = np.float32
    m = np.array(im.xform[:], f32)
    y, x = np.mgrid[0:H, 0:W].astype(f32)
    u, v = (x + f32(0.5)) / f32(W), (y + f32(0.5)) / f32(H)
    dx = (u - f32(im.principal_point[0])) * f32(W) / f32(im.focal_length[0])
    dy = (v - f32(im.principal_point[1])) * f32(H) / f32(im.focal_length[1])
    d = np.stack([m[0] * dx + m[3] * dy + m[6], m[1] * dx + m[4] * dy + m[7], m[2] * dx + m[5] * dy + m[8]], -1).astype(f32)
    return (d / np.linalg.norm(d.astype(np.float64), axis=-1, keepdims=True)).astype(f32)


def test_render_reads_the_map_behind_an_empty_scene(pkg):
    """With an empty occupancy bitfield every pixel of a 32x16 frame is the map read in the pixel's ray direction. The
    directions are restated here in float32; the camera matrix goes through a quaternion and back in the engine
    (effective_camera_matrix) and the pixel offset through a low-discrepancy sample, a few dozen float operations:
    64 * 2^-24 in the direction, on top of the lookup's own 11 * 2^-24 (test_envmap_host), through the map's largest
    neighbour differences times its resolution, amplified by at most 1 / sin(theta) >= 1 / 0.5 for this camera's
    rays (phi's sensitivity to the direction)."""
    W, H, ew, eh = 32, 16, 16, 8
    S = pkg.synthetic
    c2w = S.camera_poses(1, seed=7)[0]
    f = 0.5 * W / np.tan(0.5 * S.LEGO_CAMERA_ANGLE_X)
    cam = pkg.nerf.make_image(W, H, pkg.nerf.nerf_matrix_to_ngp(c2w), focal=(f, f))
    ncfg = pkg.nerf_config("C2")
    ncfg["encoding"]["log2_hashmap_size"] = 14
    net = pkg.create_nerf_network(ncfg)
    tr = pkg.Trainer(net, ncfg["optimizer"], seed=1)  # owns the parameters
    cfg = pkg.nerf.default_config(1.0)
    bitfield = torch.zeros(pkg.nerf.BITFIELD_BYTES, dtype=torch.uint8, device="cuda")
    envmap = smooth_map(ew, eh)
    r = pkg.nerf.NerfRenderer()
    r.set_envmap(torch.from_numpy(envmap).cuda())
    img = r.render(net, cfg, cam, bitfield, spp=1, background=(0.25, 0.5, 0.75, 1.0), use_inference_params=False).cpu().numpy()
    d = pixel_directions(cam, W, H).reshape(-1, 3)
    assert np.abs(d[:, 1]).max() < np.cos(np.pi / 6)   # sin(theta) > 0.5
    tex, wt = pkg.nerf.envmap_lookup(ew, eh, torch.from_numpy(d).cuda())
    expect = (wt.cpu().numpy().astype(np.float64)[:, :, None] * envmap.reshape(-1, 4).astype(np.float64)[tex.cpu().numpy()]).sum(1)
    e64 = envmap.astype(np.float64)
    lx, ly = np.abs(np.diff(e64, axis=1)).max(), np.abs(np.diff(e64, axis=0)).max()
    bound = (lx * (ew - 1) + ly * (eh - 1)) * (64 + 11) * 2.0 ** -24 * 2 + 12 * 2.0 ** -24 * np.abs(e64).max()
    err = np.abs(img.reshape(-1, 4) - expect).max()
    print(f"render over the map: max err = {err:.3e} (bound {bound:.3e})")
    assert err <= bound and np.ptp(img[..., 0]) > 0.01
    # unbound: the constant, as before
    r.set_envmap(None)
    img = r.render(net, cfg, cam, bitfield, spp=1, background=(0.25, 0.5, 0.75, 1.0), use_inference_params=False).cpu().numpy()
    np.testing.assert_array_equal(img, np.broadcast_to(np.array([0.25, 0.5, 0.75, 1.0], np.float32), img.shape))
    del tr


def environment(d):
    """A smooth known environment (linear colours) by NGP-space direction."""
    return np.clip(0.5 + 0.45 * np.stack([d[..., 0], d[..., 1], d[..., 2]], -1) * np.array([1.0, -1.0, 1.0]), 0.0, 1.0)


def composited_scene(pkg, n_images, res, seed):
    """The procedural scene's images composited on the host over `environment`, alpha 1 (sRGB bytes)."""
    S = pkg.synthetic
    to_srgb = lambda l: np.where(l < 0.0031308, 12.92 * l, 1.055 * np.power(np.maximum(l, 0), 0.41666) - 0.055)  # noqa: E731
    to_lin = lambda s: np.where(s <= 0.04045, s / 12.92, ((s + 0.055) / 1.055) ** 2.4)  # noqa: E731
    ims, pix, lin = [], [], []
    for c2w in S.camera_poses(n_images, seed=seed):
        im = pkg.nerf.make_image(res, res, pkg.nerf.nerf_matrix_to_ngp(c2w), camera_angle_x=S.LEGO_CAMERA_ANGLE_X)
        px = S.render(c2w, res, res).astype(np.float64) / 255.0
        a = px[..., 3:4]
        full = to_lin(px[..., :3]) * a + environment(pixel_directions(im, res, res).astype(np.float64)) * (1 - a)
        out = np.concatenate([to_srgb(full), np.ones_like(a)], -1)
        ims.append(im)
        pix.append((out * 255 + 0.5).clip(0, 255).astype(np.uint8))
        lin.append(full)
    return ims, pix, lin


PSNR_ON, PSNR_OFF = 25.62, 17.96   # measured on an MI355X, one run each (training is reproducible: a run repeats itself)
MEASURED_GAP_DB = PSNR_ON - PSNR_OFF


def test_train_envmap_learns_a_background(pkg):
    """The procedural scene composited on the host over a smooth known environment, alpha 1: 40 views of 64x64 for
    training and 4 held out; 1000 steps at a batch of 2^18 with no random background (every pixel is opaque),
    train_envmap on from a zero 16x8 map against off, which is the parent commit's behaviour rendered over black: there
    the far field has to be baked into the box. Mean held-out PSNR measured once on an MI355X: 25.62 dB on, 17.96 dB
    off (a 32x16 map: 23.48 dB). The test asserts half of that gap, so that seed and run-to-run variation fit inside."""
    n_train, n_held = 40, 4
    ims, pix, lin = composited_scene(pkg, n_train + n_held, 64, seed=5)
    ds = pkg.nerf.NerfDataset(ims[:n_train], pix[:n_train])
    psnr = {}
    for on in (True, False):
        # no random background: every training pixel is opaque, and a random colour behind the rays would only teach
        # the network to let none through
        run, net, tr, cfg = make_run(pkg, ds, envmap_res=(16, 8) if on else None, train=on, batch=1 << 18, random_bg_color=0)
        for _ in range(1000):
            run.train_step(get_loss=False)
        r = pkg.nerf.NerfRenderer()
        if on:
            r.set_envmap(run)
        vals = []
        for k in range(n_train, n_train + n_held):
            img = r.render(net, cfg, ims[k], run.bitfield, spp=1, background=(0.0, 0.0, 0.0, 1.0))
            vals.append(pkg.nerf.psnr(img.cpu(), torch.from_numpy(lin[k]).float())[0])
        psnr[on] = float(np.mean(vals))
    print(f"held-out PSNR: train_envmap on {psnr[True]:.2f} dB, off {psnr[False]:.2f} dB")
    assert psnr[True] - psnr[False] >= 0.5 * MEASURED_GAP_DB


# ---- pyngp --------------------------------------------------------------------------------------------------------
def test_pyngp_trains_the_datasets_envmap(pkg, tmp_path):
    from PIL import Image
    S = pkg.synthetic
    frames = []
    for i, c2w in enumerate(S.camera_poses(6, seed=4)):
        Image.fromarray(S.render(c2w, 48, 48)).save(tmp_path / f"r_{i}.png")
        frames.append({"file_path": f"./r_{i}", "transform_matrix": np.asarray(c2w, np.float64).tolist()})
    sky = np.random.default_rng(1).random((4, 8, 4)).astype(np.float32)
    pkg.exr.write_exr(str(tmp_path / "sky.exr"), sky)
    (tmp_path / "transforms.json").write_text(json.dumps({"camera_angle_x": S.LEGO_CAMERA_ANGLE_X, "envmap": "sky.exr",
                                                          "frames": frames}))
    ngp = pkg.pyngp()
    tb = ngp.Testbed()
    tb.load_training_data(str(tmp_path))
    assert not tb.nerf.training.train_envmap
    tb.nerf.training.train_envmap = True
    assert tb.nerf.training.train_envmap
    tb.shall_train = True
    tb.frame()
    first = tb.nerf.training.envmap()
    assert first.shape == (4, 8, 4)
    for _ in range(9):
        tb.frame()
    after = tb.nerf.training.envmap()
    assert np.isfinite(after).all() and np.abs(after[..., :3] - sky[..., :3]).max() > 1e-3   # it trained
    np.testing.assert_array_equal(after[..., 3], sky[..., 3])                                  # alpha stays
    assert tb.nerf.training.envmap(ema=True).shape == (4, 8, 4)
    img = tb.render(32, 24, spp=1, linear=True)
    assert np.isfinite(img).all()
    # a dataset without the key: no map until one is created; then it trains from zero
    (tmp_path / "transforms.json").write_text(json.dumps({"camera_angle_x": S.LEGO_CAMERA_ANGLE_X, "frames": frames}))
    tb2 = ngp.Testbed()
    tb2.load_training_data(str(tmp_path))
    tb2.nerf.training.train_envmap = True
    tb2.shall_train = True
    tb2.frame()
    assert tb2.nerf.training.envmap() is None
    tb2.nerf.training.create_envmap(16, 8)
    for _ in range(5):
        tb2.frame()
    m = tb2.nerf.training.envmap()
    assert m.shape == (8, 16, 4) and np.abs(m[..., :3]).max() > 0
