"""Smoothstep interpolation of the grid encoding ("interpolation": "Smoothstep") on the GPU, through every kernel
that turns a cell fraction into a corner weight: the two forward kernels, the atomic backward, the bucketed
backward's item, direct and brick paths, the input-gradient kernel and the encoding fused into the NeRF inference
MLP. The yardstick is tests/grid_reference.py (anchored to the CPU oracle by tests/test_grid_reference_host.py):
forward and bucketed backward bit for bit, input gradient within the Linear test's bar."""
import numpy as np
import pytest
import torch

import grid_reference as gr

pytestmark = pytest.mark.gpu

MLP1 = {"otype": "FullyFusedMLP", "activation": "ReLU", "output_activation": "None", "n_neurons": 64, "n_hidden_layers": 1}
MLP2 = {**MLP1, "n_hidden_layers": 2}
ADAM = {"otype": "Adam", "learning_rate": 1e-2, "beta1": 0.9, "beta2": 0.99, "epsilon": 1e-15, "l2_reg": 1e-6}
N = 4099  # above the bucketed backward's threshold (4096), ragged


@pytest.fixture(scope="module")
def pkg():
    from __graft_entry__ import load_package
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return load_package()


def enc_cfg(L, F, T, interp="Smoothstep", Nmin=16):
    cfg = {"otype": "HashGrid", "n_levels": L, "n_features_per_level": F, "log2_hashmap_size": T, "base_resolution": Nmin,
           "per_level_scale": 2.0}
    if interp is not None:
        cfg["interpolation"] = interp
    return cfg


def make(pkg, D, L, F, T, interp="Smoothstep", seed=1, opts=None, Nmin=16, mlp=MLP2):
    """(network, trainer, desc, fp16 bits of a U(-1, 1) grid table planted in the trainer's parameters)."""
    net = pkg.NetworkWithInputEncoding(D, 1, enc_cfg(L, F, T, interp, Nmin), mlp)
    for k, v in (opts or {}).items():
        net.set_option(k, v)
    tr = pkg.Trainer(net, ADAM)
    nm = net.n_matrix_params
    table = (np.random.default_rng(seed).random(net.n_params - nm, dtype=np.float32) * 2 - 1).astype(np.float16)
    tr.params[nm:] = torch.from_numpy(table).cuda()
    torch.cuda.synchronize()
    return net, tr, gr.Desc(net.layout()), table.view(np.uint16)


def dy_batch(net, g, n, seed):
    dy = np.zeros((n, net.layout().encoding_width), np.float16)
    dy[:, :g.L * g.F] = np.random.default_rng(seed).uniform(-1, 1, (n, g.L * g.F)).astype(np.float16)
    return dy


def grid_grad(net, tr, x, dy, soa=False, init=None, **kw):
    nm = net.n_matrix_params
    if init is not None:
        tr.gradients[nm:] = torch.from_numpy(init.view(np.float16)).cuda()
    if soa:
        dyt, kw["layout"] = torch.from_numpy(np.ascontiguousarray(dy.T)).cuda(), 1
    else:
        dyt = torch.from_numpy(dy).cuda()
    net.encoding_backward(torch.from_numpy(x).cuda(), dyt, **kw)
    torch.cuda.synchronize()
    return tr.gradients[nm:].cpu().numpy().view(np.uint16).copy()


def assert_bits(got, ref, what):
    assert got.shape == ref.shape, what
    bad = np.argwhere(got != ref)
    assert len(bad) == 0, f"{what}: {len(bad)} of {ref.size} differ, first {[(tuple(i), hex(got[tuple(i)]), hex(ref[tuple(i)])) for i in bad[:4]]}"


# ---- 1. config surface --------------------------------------------------------------------------------------------

def test_config_surface(pkg):
    for name in ("Smoothstep", "smoothstep", "SMOOTHSTEP"):
        net = pkg.NetworkWithInputEncoding(3, 1, enc_cfg(4, 2, 14, name), MLP1)
        assert net.query("grid_interpolation") == 1 and net.interpolation == "Smoothstep"
    for name in (None, "Linear", "linear"):
        net = pkg.NetworkWithInputEncoding(2, 3, enc_cfg(4, 2, 14, name), MLP1)
        assert net.query("grid_interpolation") == 0 and net.interpolation == "Linear"
    cfg = pkg.nerf_config("C2")
    assert pkg.create_nerf_network(cfg).query("grid_interpolation") == 0
    cfg["encoding"]["interpolation"] = "Smoothstep"
    assert pkg.create_nerf_network(cfg).interpolation == "Smoothstep"
    dense = {"otype": "DenseGrid", "n_levels": 3, "n_features_per_level": 8, "base_resolution": 8, "interpolation": "Smoothstep"}
    assert pkg.NetworkWithInputEncoding(3, 1, dense, MLP1).query("grid_interpolation") == 1
    with pytest.raises(RuntimeError, match="(?s)Linear.*Smoothstep"):
        pkg.NetworkWithInputEncoding(3, 1, enc_cfg(4, 2, 14, "Nearest"), MLP1)
    with pytest.raises(AttributeError):
        net.interpolation = "Smoothstep"  # read-only


# ---- 2. forward ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("D,L,F,T", gr.SHAPES)
def test_forward_bits(pkg, D, L, F, T):
    """AoS (the row kernel) and SoA (the per-level kernel) against the helper; a lowered max level on the L16 shape
    and a per-sample max level on the 2D shape."""
    net, tr, g, table = make(pkg, D, L, F, T, seed=L + F)
    x = gr.positions(g, N, seed=T)
    xt = torch.from_numpy(x).cuda()
    variants = [{}]
    if L == 16:
        variants.append({"max_level": 0.6})
    if D == 2:
        variants.append({"max_level_per_sample": np.random.default_rng(5).uniform(0, 1.2, N).astype(np.float32)})
    for kw in variants:
        per = kw.get("max_level_per_sample")
        net.set_max_level(kw.get("max_level", 1.0), None if per is None else torch.from_numpy(per).cuda())
        ref = gr.forward(g, x, table, gr.SMOOTHSTEP, **kw)
        assert (ref != gr.forward(g, x, table, gr.LINEAR, **kw)).mean() > 0.5  # the two modes are told apart
        aos = net.encode(xt).cpu().numpy().view(np.uint16)
        assert_bits(aos[:, :L * F], ref, f"AoS {kw.keys()}")
        assert not aos[:, L * F:].any()
        soa = net.encode(xt, layout=pkg.LAYOUT_SOA).cpu().numpy().view(np.uint16)
        assert_bits(np.ascontiguousarray(soa[:L * F].T), ref, f"SoA {kw.keys()}")


# ---- 3. bucketed backward -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("D,L,F,T", gr.SHAPES)
def test_backward_items_bits(pkg, D, L, F, T):
    """Every level through items (grid_direct 0; no bricks at this size): overwrite, then accumulate onto a nonzero
    gradient, then an SoA dL/dy."""
    net, tr, g, _ = make(pkg, D, L, F, T, opts={"grid_direct": 0, "grid_backward_mode": 3})
    x = gr.positions(g, N, seed=T + 1)
    dy = dy_batch(net, g, N, seed=2)
    ref = gr.backward(g, x, dy.view(np.uint16), gr.SMOOTHSTEP)
    assert (ref != gr.backward(g, x, dy.view(np.uint16), gr.LINEAR)).mean() > 0.05
    assert_bits(grid_grad(net, tr, x, dy), ref, "overwrite")
    assert net.query("grid_direct_levels") == 0 and net.query("grid_brick_levels") == 0
    init = np.random.default_rng(3).uniform(-0.5, 0.5, g.n_params).astype(np.float16).view(np.uint16)
    ref_acc = gr.backward(g, x, dy.view(np.uint16), gr.SMOOTHSTEP, grad16=init)
    assert_bits(grid_grad(net, tr, x, dy, init=init, grad_mode=pkg.GRAD_ACCUMULATE), ref_acc, "accumulate")
    assert_bits(grid_grad(net, tr, x, dy, soa=True), ref, "SoA dL/dy")


@pytest.mark.parametrize("D,L,F,T,n_direct", [(3, 4, 4, 15, 1), (2, 4, 2, 14, 3), (3, 8, 1, 12, 8)])
def test_backward_direct_bits(pkg, D, L, F, T, n_direct):
    """Direct levels (no items; grid_direct_part + 1 samples so that a second part holds one sample), with a
    per-sample max level on the 2D shape whose direct levels it can mask; the same bits with the option off. At
    T = 2^12 every level of the F = 1 shape has at most two buckets: all eight are direct and no item is staged."""
    probe = pkg.NetworkWithInputEncoding(D, 1, enc_cfg(L, F, T), MLP2)
    n = int(probe.query("grid_direct_part")) + 1
    net, tr, g, _ = make(pkg, D, L, F, T)
    x = gr.positions(g, n, seed=7)
    dy = dy_batch(net, g, n, seed=8)
    ml = np.random.default_rng(9).uniform(0, 1.2, n).astype(np.float32) if D == 2 else None
    if ml is not None:
        mlt = torch.from_numpy(ml).cuda()
        net.set_max_level(1.0, mlt)
    ref = gr.backward(g, x, dy.view(np.uint16), gr.SMOOTHSTEP, max_level_per_sample=ml)
    assert_bits(grid_grad(net, tr, x, dy), ref, "direct")
    assert net.query("grid_direct_levels") == n_direct
    assert_bits(grid_grad(net, tr, x, dy, soa=True), ref, "direct, SoA dL/dy")
    net.set_option("grid_direct", 0)
    assert_bits(grid_grad(net, tr, x, dy), ref, "items")
    assert net.query("grid_direct_levels") == 0


def test_backward_bricks_bits(pkg):
    """Brick-summed dense levels: C2's grid at 2^18 samples, the smallest batch at which the plan takes bricks.
    Positions include cell faces and points outside the cube (the global fallback table). With bricks, without them
    and with every level through items the engine gives the helper's bits, hence the forms give one another's (direct
    levels against items at their own batch sizes: test_backward_direct_bits)."""
    D, L, F, T, n = 3, 4, 4, 19, 1 << 18
    net, tr, g, _ = make(pkg, D, L, F, T, opts={"grid_bricks": 1})
    x = gr.positions(g, n, seed=11)
    blob = np.random.default_rng(12).random(n) < 0.5  # a concentrated cloud: bricks of thousands of samples split into parts
    x[blob] = np.clip(0.5 + 0.05 * np.random.default_rng(13).standard_normal((int(blob.sum()), D)), 0, 1).astype(np.float32)
    dy = dy_batch(net, g, n, seed=14)
    ref = gr.backward(g, x, dy.view(np.uint16), gr.SMOOTHSTEP)
    assert_bits(grid_grad(net, tr, x, dy), ref, "bricks")
    assert net.query("grid_brick_levels") > 0
    net.set_option("grid_bricks", 0)
    assert_bits(grid_grad(net, tr, x, dy), ref, "no bricks (the plan's own choice of direct levels)")
    assert net.query("grid_brick_levels") == 0
    net.set_option("grid_direct", 0)
    assert_bits(grid_grad(net, tr, x, dy), ref, "items")
    assert net.query("grid_brick_levels") == 0 and net.query("grid_direct_levels") == 0
    net.set_option("grid_bricks", 1)
    assert_bits(grid_grad(net, tr, x, dy), ref, "bricks + items")
    assert net.query("grid_brick_levels") > 0


# ---- 4. small-batch atomic backward -------------------------------------------------------------------------------

@pytest.mark.parametrize("D,L,F,T", gr.SHAPES)
def test_backward_atomics(pkg, D, L, F, T):
    """n = 1000 takes the packed-fp16 atomics. The bar is test_gpu_parity.py::test_encoding_backward's for the Linear
    kernel, 3e-2 max|ref| + 1e-3: each add rounds the running sum to fp16 in arrival order, which is the only
    difference from the helper's exact sums and does not depend on the interpolation."""
    net, tr, g, _ = make(pkg, D, L, F, T)
    n = 1000
    x = gr.positions(g, n, seed=21)
    dy = dy_batch(net, g, n, seed=22)
    got = grid_grad(net, tr, x, dy).view(np.float16).astype(np.float64)
    ref = gr.backward(g, x, dy.view(np.uint16), gr.SMOOTHSTEP).view(np.float16).astype(np.float64)
    lin = gr.backward(g, x, dy.view(np.uint16), gr.LINEAR).view(np.float16).astype(np.float64)
    tol = 3e-2 * np.abs(ref).max() + 1e-3
    print("atomic backward: max err %.3g, bar %.3g, Linear's distance %.3g" % (np.abs(got - ref).max(), tol, np.abs(lin - ref).max()))
    assert np.abs(got - ref).max() <= tol
    assert np.all(got[ref == 0] == 0)


# ---- 5. identities with Linear ------------------------------------------------------------------------------------

def test_identities_with_linear(pkg):
    """One level of scale 16 (base_resolution 17) and positions k / 32: every fraction is 0 or 0.5, where
    s(f) = f, so forward and backward equal the Linear model's bits; s'(0) = 0 and s'(0.5) = 1.5 give the input
    gradient from the Linear one."""
    D, L, F, T = 3, 1, 2, 15
    nets = {m: make(pkg, D, L, F, T, interp=m, Nmin=17, seed=4, opts={"grid_backward_mode": 3}) for m in ("Linear", "Smoothstep")}
    g = nets["Linear"][2]
    assert float(g.scale[0]) == 16.0
    k = np.random.default_rng(31).integers(0, 33, (N, D))
    x = (k / 32).astype(np.float32)
    half = (k % 2 == 0)  # p = k / 2 + 0.5: fraction 0.5 for even k, 0 for odd k
    dy = dy_batch(nets["Linear"][0], g, N, seed=32)
    out = {}
    for m, (net, tr, _, _) in nets.items():
        xt = torch.from_numpy(x).cuda()
        enc = net.encode(xt).cpu().numpy().view(np.uint16)
        din = torch.full((N, D + 1), 7.0, device="cuda")
        net.encoding_backward(xt, torch.from_numpy(dy).cuda(), dL_dinput=din)
        torch.cuda.synchronize()
        out[m] = (enc, tr.gradients[net.n_matrix_params:].cpu().numpy().view(np.uint16).copy(), din.cpu().numpy())
    assert out["Linear"][0].any() and out["Linear"][1].any()
    assert_bits(out["Smoothstep"][0], out["Linear"][0], "forward")
    assert_bits(out["Smoothstep"][1], out["Linear"][1], "backward")
    lin, sm = out["Linear"][2][:, :D], out["Smoothstep"][2][:, :D]
    assert np.all(sm[~half] == 0.0)
    want = np.float32(1.5) * lin[half]
    assert np.abs(lin[half]).max() > 1.0
    assert np.all(np.abs(sm[half] - want) <= 4 * np.spacing(np.abs(want)))


# ---- 6. input gradient --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("D,L,F,T,max_level", [(3, 4, 4, 19, 1.0), (3, 16, 2, 19, 1.0), (2, 4, 2, 14, 1.0), (3, 8, 1, 12, 0.6),
                                                (3, 4, 8, 10, 1.0), (3, 16, 2, 22, 1.0)])
def test_input_gradient(pkg, D, L, F, T, max_level):
    """The shapes and the bar of test_gpu_input_grad.py::test_encoding_input_gradient_vs_oracle,
    |gpu - ref| <= 1e-5 (|ref| + cond), cond multiplied by 1.5 = max s'; the batch ends with face-straddling pairs."""
    net, tr, g, table = make(pkg, D, L, F, T, seed=L * F + D, mlp=MLP1)
    net.set_max_level(max_level)
    xm, xp, _, _, _ = gr.face_pairs(g, 48, seed=6)
    x = np.concatenate([gr.positions(g, N - 96, seed=41), xm, xp])
    W = net.layout().encoding_width
    dy = np.zeros((N, W), np.float16)
    dy[:, :L * F] = np.random.default_rng(42).standard_normal((N, L * F)).astype(np.float16)
    tr.gradients.zero_()
    out = torch.full((N, D + 1), 7.0, device="cuda")
    net.encoding_backward(torch.from_numpy(x).cuda(), torch.from_numpy(dy).cuda(), grad_mode=pkg.GRAD_IGNORE, dL_dinput=out)
    got = out.cpu().numpy()
    assert np.all(got[:, D] == 7.0)
    ref = gr.input_grad(g, x, table, dy.astype(np.float32), gr.SMOOTHSTEP, max_level=max_level)
    scales = np.array([float(s) for s in g.scale])
    active = np.arange(L) < max_level * L + 1e-3
    cond = (np.abs(dy[:, :L * F].astype(np.float64)).reshape(N, L, F).sum(2) * (scales * active)).sum(1) * 2 ** D * 1.5
    bar = 1e-5 * (np.abs(ref) + cond[:, None])
    err = np.abs(got[:, :D] - ref)
    lin = gr.input_grad(g, x, table, dy.astype(np.float32), gr.LINEAR, max_level=max_level)
    print("input gradient: max err / bar %.3g; Linear's distance / bar, median %.3g" % ((err / bar).max(), np.median(np.abs(lin - ref) / bar)))
    assert np.all(err <= bar), (err.max(), np.unravel_index(np.argmax(err / bar), err.shape))
    assert np.median(np.abs(lin - ref) / bar) > 10  # the bar tells the modes apart
    assert int(torch.count_nonzero(tr.gradients).item()) == 0  # GRAD_IGNORE: no parameter gradient written


# ---- 7. fused inference -------------------------------------------------------------------------------------------

def test_fused_inference_bits(pkg):
    """A C2-shaped NeRF model: inference with the encoding inside the MLP kernel (the Smoothstep instantiation) equals
    encode-then-MLP bit for bit, the fused path is the one that runs, and both differ from the Linear model's."""
    outs = {}
    n = 1000
    r = np.random.default_rng(51)
    x = np.zeros((n, 7), np.float32)
    x[:, :3] = r.uniform(-0.1, 1.1, (n, 3))
    x[:, 4:] = r.standard_normal((n, 3))
    x[:, 4:] /= np.linalg.norm(x[:, 4:], axis=1, keepdims=True)
    xt = torch.from_numpy(x).cuda()
    for interp in ("Smoothstep", "Linear"):
        cfg = pkg.nerf_config("C2")
        cfg["encoding"].update({"log2_hashmap_size": 15, "interpolation": interp})
        net = pkg.create_nerf_network(cfg)
        params = torch.from_numpy((np.random.default_rng(52).standard_normal(net.n_params) * 0.3).astype(np.float16)).cuda()
        net.set_params(params, params)
        for fuse in (1, 0):
            net.set_option("fuse_infer", fuse)
            assert net.query("fused_inference") == fuse
            outs[interp, fuse, "rgbd"] = net.inference(xt, layout=pkg.LAYOUT_AOS_RGBD).cpu().numpy().view(np.uint16)
            outs[interp, fuse, "soa"] = net.inference(xt, layout=pkg.LAYOUT_SOA).cpu().numpy().view(np.uint16)
            outs[interp, fuse, "density"] = net.density(xt).cpu().numpy().view(np.uint16)
    for what in ("rgbd", "soa", "density"):
        assert_bits(outs["Smoothstep", 1, what], outs["Smoothstep", 0, what], what)
    assert np.isfinite(outs["Smoothstep", 1, "rgbd"].view(np.float16).astype(np.float32)).all()
    assert (outs["Smoothstep", 1, "rgbd"] != outs["Linear", 1, "rgbd"]).mean() > 0.5


# ---- 8. end to end through the network ----------------------------------------------------------------------------

def test_network_input_gradient(pkg, orc):
    """ngp_input_gradient (dim 0) of a Smoothstep NetworkWithInputEncoding against the helper's encoding, the
    oracle's MLP backward on it and the helper's input gradient of the resulting dL/d(encoding). Tolerances of
    test_gpu_input_grad.py::test_nerf_backward_input_gradients: per element 1e-2 relative + 1e-3 of the column's
    largest value, fewer than 2e-3 of the elements outside (fp16 dL/d(encoding) against the oracle's float)."""
    D, L, F, T = 3, 4, 4, 15
    net = pkg.NetworkWithInputEncoding(D, 1, enc_cfg(L, F, T), MLP2)
    tr = pkg.Trainer(net, ADAM)
    nm = net.n_matrix_params
    p = net.initialize_params(1337)
    p[nm:] = np.random.default_rng(61).uniform(-0.5, 0.5, net.n_params - nm)
    tr.set_params_full_precision(p)
    torch.cuda.synchronize()
    p16 = tr.params.cpu().numpy().view(np.uint16).copy()
    g = gr.Desc(net.layout())
    x = gr.positions(g, N, seed=62)
    got = net.input_gradient(0, torch.from_numpy(x).cuda()).cpu().numpy()[:, :D]
    mlp = orc.make_mlp(16, 64, 2, 16)
    assert orc.mlp_n_params(mlp) == nm
    enc = gr.forward(g, x, p16[nm:], gr.SMOOTHSTEP).view(np.float16).astype(np.float32)
    dout = np.zeros((N, 16), np.float32)
    dout[:, 0] = 1.0
    _, denc = orc.mlp_backward(mlp, p16[:nm], enc, dout)
    ref = gr.input_grad(g, x, p16[nm:], denc, gr.SMOOTHSTEP)
    bad = np.abs(got - ref) > 1e-2 * np.abs(ref) + 1e-3 * np.abs(ref).max(axis=0)
    print("network input gradient: fraction outside %.3g" % bad.mean())
    assert np.abs(ref).max() > 1e-3
    assert bad.mean() < 2e-3, bad.mean()


# ---- 9. training and round trip -----------------------------------------------------------------------------------

def test_training_falls_and_is_deterministic(pkg):
    """An SDF-shaped Smoothstep model on the distance to a sphere, 50 steps at batch 4096: the loss falls, and the
    parameters after the run are the same bits in a second run (the bucketed backward is deterministic)."""
    r = np.random.default_rng(71)
    xs = [torch.from_numpy(r.random((4096, 3), dtype=np.float32)).cuda() for _ in range(50)]
    ts = [(torch.linalg.norm(x - 0.5, dim=1, keepdim=True) - 0.3).contiguous() for x in xs]
    runs = []
    for fused_hist in (1, 1, 0):  # the third run counts the buckets in a pass of its own instead of in the forward
        net = pkg.NetworkWithInputEncoding(3, 1, enc_cfg(8, 2, 15), MLP2)
        net.set_option("fused_hist", fused_hist)
        tr = pkg.Trainer(net, ADAM, seed=1337)
        losses = [tr.training_step(x, t, loss="L2") for x, t in zip(xs, ts)]
        torch.cuda.synchronize()
        runs.append((losses, tr.params.cpu().numpy().view(np.uint16).copy()))
    losses = runs[0][0]
    print("loss: first %.4g, last %.4g" % (losses[0], losses[-1]))
    assert np.isfinite(losses).all() and np.mean(losses[-5:]) < 0.5 * np.mean(losses[:5])
    np.testing.assert_array_equal(runs[0][1], runs[1][1])
    np.testing.assert_array_equal(runs[0][1], runs[2][1])


def test_pyngp_snapshot_round_trip(pkg, tmp_path):
    """pyngp.Testbed takes the mode from its network config, and a snapshot carries it: the loaded model reports
    Smoothstep and renders the frame that the saving testbed renders after loading its own snapshot."""
    ngp = pkg.pyngp()
    verts = pkg.synthetic.icosphere(2, bumps=0.15, seed=1)
    obj = tmp_path / "icosphere.obj"
    with open(obj, "w") as f:
        for v in verts:
            f.write("v %r %r %r\n" % (float(v[0]), float(v[1]), float(v[2])))
        for t in range(len(verts) // 3):
            f.write("f %d %d %d\n" % (3 * t + 1, 3 * t + 2, 3 * t + 3))
    cam = np.asarray([[1, 0, 0, 0.5], [0, 1, 0, 0.5], [0, 0, 1, -1.0]], np.float32)

    def testbed():
        tb = ngp.Testbed()
        tb.load_training_data(str(obj))
        return tb

    def frame(tb):
        tb.camera_matrix = cam
        tb.sdf.max_iterations = 256
        tb.snap_to_pixel_centers = True
        tb.background_color = [0.0, 0.0, 0.0, 0.0]
        tb.render_mode = ngp.RenderMode.Normals
        return tb.render(32, 32, 1, True)

    tb = testbed()
    tb.reload_network_from_json({**pkg.SDF_BASE, "encoding": {**pkg.SDF_BASE["encoding"], "log2_hashmap_size": 14,
                                                              "interpolation": "Smoothstep"}})
    for _ in range(30):
        tb.train(1 << 14)
    assert tb.grid_interpolation == "Smoothstep"
    snap = str(tmp_path / "smooth.ingp")
    tb.save_snapshot(snap, False, False)
    tb.load_snapshot(snap)
    tb2 = testbed()
    tb2.load_snapshot(snap)
    assert tb2.grid_interpolation == "Smoothstep"
    a, b = frame(tb), frame(tb2)
    assert (a[..., 3] == 1.0).sum() > 50
    np.testing.assert_array_equal(a.view(np.uint32), b.view(np.uint32))
    lin = testbed()
    lin.reload_network_from_json({**pkg.SDF_BASE, "encoding": {**pkg.SDF_BASE["encoding"], "log2_hashmap_size": 14}})
    lin.train(1 << 14)
    assert lin.grid_interpolation == "Linear"
