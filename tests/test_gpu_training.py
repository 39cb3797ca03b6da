"""GPU parity for tcnn's training_step, the image primitive (C1) and the SDF primitive (C5), through
the C-ABI, against the CPU oracle on identical seeded inputs.

Bars: loss gradients bit-exact (same fp32 formula, one RNE rounding); image positions bit-exact,
targets within 2e-6 (powf of the sRGB curve may differ by an ulp); SDF surface/uniform sample
positions within 1e-6, perturbed ones within 1e-5 (logf), signed distances within 1e-5 (sign equal
away from the surface); training_step gradients equal forward_backward given the same dL/doutput.
"""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARMADILLO = os.path.join(ROOT, "data", "sdf", "armadillo.obj")


@pytest.fixture(scope="module")
def pkg():
    from __graft_entry__ import load_package
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return load_package()


MLP = {"otype": "FullyFusedMLP", "activation": "ReLU", "output_activation": "None", "n_neurons": 64, "n_hidden_layers": 2}
ADAM = {"otype": "Adam", "learning_rate": 1e-2, "beta1": 0.9, "beta2": 0.99, "epsilon": 1e-15, "l2_reg": 1e-6}


def enc(D, L, F, T):
    return {"otype": "HashGrid", "n_levels": L, "n_features_per_level": F, "log2_hashmap_size": T, "base_resolution": 16,
            "per_level_scale": 2.0}


@pytest.mark.parametrize("loss", ["L2", "L1", "MAPE", "SMAPE", "RelativeL2"])
def test_loss_bitexact(pkg, orc, loss):
    g = np.random.default_rng(3)
    n, dims = 4099, 3
    out = torch.from_numpy(g.uniform(-2, 2, (n, 16)).astype(np.float16)).cuda()
    tgt = torch.from_numpy(g.uniform(-2, 2, (n, dims)).astype(np.float32)).cuda()
    dl, vals, tot = pkg.loss_evaluate(loss, out, tgt, dims)
    rtot, rdl, rvals = orc.loss(loss, out.cpu().numpy().view(np.uint16), tgt.cpu().numpy(), dims)
    assert np.array_equal(dl.cpu().numpy().view(np.uint16), rdl)
    np.testing.assert_array_equal(vals.cpu().numpy(), rvals)
    assert abs(tot - rtot) <= 1e-5 * abs(rtot)


def test_training_step_equals_forward_backward(pkg):
    net = pkg.NetworkWithInputEncoding(2, 3, enc(2, 4, 2, 14), MLP)
    tr = pkg.Trainer(net, ADAM, seed=5)
    g = np.random.default_rng(0)
    n = 5000
    x = torch.from_numpy(g.random((n, 2), dtype=np.float32)).cuda()
    tgt = torch.from_numpy(g.random((n, 3), dtype=np.float32)).cuda()
    loss = tr.training_step(x, tgt, "L2", run_optimizer=False)
    torch.cuda.synchronize()
    g1 = tr.gradients.clone()
    out = net.inference(x, use_inference_params=False)
    dl, vals, tot = pkg.loss_evaluate("L2", out, tgt, 3)
    net.forward_backward(x, dl)
    torch.cuda.synchronize()
    assert torch.equal(g1, tr.gradients)
    assert abs(loss - tot) <= 1e-5 * abs(tot)
    step0 = tr.step
    tr.training_step(x, tgt, "L2", run_optimizer=True)
    assert tr.step == step0 + 1


@pytest.mark.parametrize("snap,mode,n", [(True, 3, 1 << 12), (False, 3, 1 << 12), (False, 0, 3001), (True, 3, 1 << 11)])
def test_image_samples_match_oracle(pkg, orc, snap, mode, n):
    tex = pkg.synthetic.synthetic_image(96, 64)
    img = pkg.image.Image(tex)
    net = pkg.NetworkWithInputEncoding(2, 3, enc(2, 4, 2, 14), MLP)
    tr = pkg.Trainer(net, ADAM)
    it = pkg.image.ImageTraining(net, tr, img, cfg=pkg.image.default_config(random_mode=mode, snap_to_pixel_centers=snap))
    pos, tgt = it.generate_training_samples(n)
    r = orc.Rng(1337)
    rpos, rtgt = orc.image_samples(n, r, tex, random_mode=mode, snap=snap)
    assert np.array_equal(pos.cpu().numpy(), rpos)
    np.testing.assert_allclose(tgt.cpu().numpy(), rtgt, rtol=2e-6, atol=2e-7)
    assert it.rng.state == r.s.state


def test_image_training_converges(pkg):
    tex = pkg.synthetic.synthetic_image(128, 128)
    img = pkg.image.Image(tex)
    net = pkg.NetworkWithInputEncoding(2, 3, enc(2, 8, 2, 16), MLP)
    tr = pkg.Trainer(net, ADAM)
    it = pkg.image.ImageTraining(net, tr, img, batch_size=1 << 14)
    losses = [it.train_step() for _ in range(60)]
    assert all(np.isfinite(losses))
    assert np.mean(losses[-5:]) < 0.3 * np.mean(losses[:3]), losses[::10]
    assert tr.step == 60


def test_image_c1_albert(pkg, orc):
    """BASELINE configs[0] on the GPU: albert.exr (staged by tools/stage_image.sh; without it rows 384..639 of
    the same file, tests/golden/albert_rows384_639.exr) through the EXR reader, the 2D L=4 F=2 T=2^14 grid and
    a 2x16 FullyFusedMLP; the first batch's positions and targets match the oracle, and training converges."""
    path, height = os.path.join(ROOT, "data", "image", "albert.exr"), 1024
    if not os.path.exists(path):
        path, height = os.path.join(ROOT, "tests", "golden", "albert_rows384_639.exr"), 256
    img = pkg.image.Image.load(path)
    tex = pkg.exr.read_exr(path)
    assert (img.width, img.height) == (1024, height)
    net = pkg.NetworkWithInputEncoding(2, 3, enc(2, 4, 2, 14), dict(MLP, n_neurons=16, n_hidden_layers=2))
    assert net.n_matrix_params == 16 * 16 * 3  # 768 MLP params
    tr = pkg.Trainer(net, ADAM)
    it = pkg.image.ImageTraining(net, tr, img, batch_size=1 << 16)
    pos, tgt = it.generate_training_samples(4096)
    r = orc.Rng(1337)
    rpos, rtgt = orc.image_samples(4096, r, tex)
    assert np.array_equal(pos.cpu().numpy(), rpos)
    np.testing.assert_allclose(tgt.cpu().numpy(), rtgt, rtol=2e-6, atol=2e-7)
    losses = [it.train_step() for _ in range(150)]
    assert all(np.isfinite(losses))
    assert np.mean(losses[-10:]) < 0.5 * np.mean(losses[:3]), losses[::15]


def test_sdf_samples_match_oracle(pkg, orc):
    verts = pkg.synthetic.icosphere(2, radius=0.3, bumps=0.3)
    tris, amin, amax, brad = pkg.sdf.load_mesh(verts)
    mesh = pkg.sdf.SdfMesh(tris)
    net = pkg.NetworkWithInputEncoding(3, 1, enc(3, 4, 2, 14), MLP)
    tr = pkg.Trainer(net, ADAM)
    st = pkg.sdf.SdfTraining(net, tr, mesh, amin, amax, brad, seed=11, batch_size=2048)
    pos, dist = st.generate_training_samples(2048)
    r = orc.Rng(11)
    tris = mesh.triangles  # BVH order: the surface CDF follows it (testbed_sdf.cu:1157-1172)
    rpos, rdist = orc.sdf_samples(2048, r, tris, amin, amax, st.stddev)
    base = 2048 // 8
    gp, gd = pos.cpu().numpy(), dist.cpu().numpy()
    np.testing.assert_allclose(gp[:4 * base], rpos[:4 * base], rtol=0, atol=1e-6)
    np.testing.assert_allclose(gp[7 * base:], rpos[7 * base:], rtol=0, atol=1e-6)
    np.testing.assert_allclose(gp[4 * base:7 * base], rpos[4 * base:7 * base], rtol=0, atol=1e-5)
    assert np.all(gd[:4 * base] == 0)
    ref_sd = orc.sdf_signed_distance(gp[4 * base:], tris)
    np.testing.assert_allclose(gd[4 * base:], ref_sd, rtol=0, atol=1e-5)
    assert st.rng.state == r.s.state


def test_sdf_shuffle_is_permutation(pkg):
    import ctypes as C
    from instant_ngp_amd._capi import lib
    n = 10007
    p = torch.arange(3 * n, dtype=torch.float32, device="cuda").reshape(n, 3)
    d = torch.arange(n, dtype=torch.float32, device="cuda")
    po, do = torch.empty_like(p), torch.empty_like(d)
    assert lib().ngp_sdf_shuffle(None, n, 42, C.c_void_p(p.data_ptr()), C.c_void_p(d.data_ptr()), C.c_void_p(po.data_ptr()),
                                 C.c_void_p(do.data_ptr())) == 0
    torch.cuda.synchronize()
    assert torch.equal(torch.sort(do).values, d)
    assert torch.equal(po[:, 0] / 3, do)  # rows moved together


def test_sdf_training_converges(pkg):
    verts = pkg.synthetic.icosphere(2, radius=0.3, bumps=0.2)
    tris, amin, amax, brad = pkg.sdf.load_mesh(verts)
    mesh = pkg.sdf.SdfMesh(tris)
    net = pkg.NetworkWithInputEncoding(3, 1, enc(3, 8, 2, 16), MLP)
    tr = pkg.Trainer(net, ADAM)
    st = pkg.sdf.SdfTraining(net, tr, mesh, amin, amax, brad, batch_size=1 << 13)
    losses = [st.train_step() for _ in range(120)]
    assert all(np.isfinite(losses))
    # MAPE is dominated by the on-surface samples (target 0, scale 1/0.01); it drops after an early spike
    assert np.mean(losses[-10:]) < 0.7 * max(losses[:10]), losses[::12]
    assert np.mean(losses[-10:]) < np.mean(losses[10:20]), losses[::12]


def test_sdf_bvh_signed_distance_matches_bruteforce(pkg, orc):
    """BVH raystab signed distance (csrc/bvh.hip) == the oracle's brute force over every triangle
    (closest distance and the 32-stab-ray sign with per-sample offsets), on a 20k-triangle mesh."""
    verts = pkg.synthetic.icosphere(5, radius=0.3, bumps=0.3)
    tris, amin, amax, brad = pkg.sdf.load_mesh(verts)
    mesh = pkg.sdf.SdfMesh(tris)
    assert mesh.triangles.shape[0] >= 20000
    g = np.random.default_rng(3)
    pts = np.concatenate([g.uniform(0.0, 1.0, (256, 3)),  # uniform in the cube (mostly outside)
                          (0.5 + g.normal(0.0, 0.12, (256, 3)))]).astype(np.float32)  # near the surface / inside
    got = mesh.signed_distance(torch.from_numpy(pts).cuda()).cpu().numpy()
    ref = orc.sdf_signed_distance(pts, mesh.triangles)
    assert np.mean(ref < 0) > 0.1 and np.mean(ref > 0) > 0.1
    np.testing.assert_allclose(got, ref, rtol=0, atol=1e-5)


@pytest.mark.skipif(not os.path.isfile(ARMADILLO), reason="data/sdf not staged (tools/stage_sdf.sh)")
def test_sdf_armadillo_signed_distance_matches_bruteforce(pkg, orc):
    """C5's mesh (armadillo, ~100k triangles): the online ground truth of the training batch — perturbed
    surface samples (the hard case for the stab rays: they start next to the surface) and uniform
    samples — equals the oracle's brute force over every triangle, sign and distance."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import sdf_train
    tris, amin, amax, brad = pkg.sdf.load_mesh(sdf_train.load_obj_triangles(ARMADILLO))
    mesh = pkg.sdf.SdfMesh(tris)
    net = pkg.NetworkWithInputEncoding(3, 1, enc(3, 4, 2, 14), MLP)
    tr = pkg.Trainer(net, ADAM)
    st = pkg.sdf.SdfTraining(net, tr, mesh, amin, amax, brad, seed=5, batch_size=1 << 12)
    pos, dist = st.generate_training_samples(1 << 12)
    base = (1 << 12) // 8
    pts = pos.cpu().numpy()[4 * base:]
    idx = np.concatenate([np.arange(0, 3 * base, 3 * base // 96), np.arange(3 * base, 4 * base, base // 32)])
    got = mesh.signed_distance(torch.from_numpy(np.ascontiguousarray(pts[idx])).cuda()).cpu().numpy()
    ref = orc.sdf_signed_distance(pts[idx], mesh.triangles)
    assert np.mean(ref < 0) > 0.2 and np.mean(ref > 0) > 0.2
    np.testing.assert_array_equal(np.sign(got), np.sign(ref))
    np.testing.assert_allclose(got, ref, rtol=0, atol=1e-6)
