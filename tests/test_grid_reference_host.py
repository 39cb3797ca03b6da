"""tests/grid_reference.py against the CPU oracle (Linear: bit for bit) and against itself (Smoothstep: the analytic
input gradient is the derivative of the forward, and is continuous across cell faces where the Linear one jumps)."""
import numpy as np
import pytest

import grid_reference as gr

N = 4096


@pytest.fixture(scope="module", params=gr.SHAPES, ids=lambda s: "D%d-L%d-F%d-T%d" % s)
def case(request, orc):
    D, L, F, log2T = request.param
    og = orc.make_grid(D, L, F, log2T)
    g = gr.Desc(og)
    r = np.random.default_rng(L * 100 + F)
    table = r.uniform(-1, 1, g.n_params).astype(np.float16).view(np.uint16)
    pos = gr.positions(g, N, seed=F)
    dy = r.uniform(-1, 1, (N, L * F)).astype(np.float16)
    return og, g, table, pos, dy


def test_fma32_rounds_once():
    """An fp32 FMA whose exact result lies 2^-31 below an fp32 tie: a b = 32 (1 - 2^-36), c = 2^29 + 64 (ulp 64, odd
    mantissa). One rounding gives c; rounding to float64 first lands on the tie, which then rounds to even, c + 64."""
    a = np.array([32 * (1 - 2.0 ** -18)], np.float32)
    b = np.array([1 + 2.0 ** -18], np.float32)
    c = np.array([2.0 ** 29 + 64], np.float32)
    assert float(a[0]) * float(b[0]) == 32 - 2.0 ** -31
    twice = np.float32(float(a[0]) * float(b[0]) + float(c[0]))
    assert twice == np.float32(2.0 ** 29 + 128)
    assert gr.fma32(a, b, c)[0] == c[0]
    assert gr.fma32(a, b, -c)[0] == -c[0]  # -(2^29 + 32 + 2^-31): just beyond the tie with -2^29, which two roundings give
    assert np.float32(float(a[0]) * float(b[0]) - float(c[0])) == np.float32(-(2.0 ** 29))
    # exact ties still go to even, and exact results stay
    one = np.array([1.0], np.float32)
    assert gr.fma32(np.array([2.0 ** -24], np.float32), one, one)[0] == np.float32(1.0)
    assert gr.fma32(np.array([3 * 2.0 ** -24], np.float32), one, one)[0] == np.float32(1 + 2.0 ** -22)
    assert gr.fma32(np.array([0.5], np.float32), np.array([0.25], np.float32), one)[0] == np.float32(1.125)


def test_linear_forward_bits(case, orc):
    og, g, table, pos, _ = case
    for kw in ({}, {"max_level": 0.6}, {"max_level_per_sample": np.random.default_rng(1).uniform(0, 1.2, N).astype(np.float32)}):
        ref = orc.grid_forward(og, pos, table, **kw).astype(np.float16).view(np.uint16)
        np.testing.assert_array_equal(gr.forward(g, pos, table, gr.LINEAR, **kw), ref)


def test_linear_backward_bits(case, orc):
    og, g, _, pos, dy = case
    dy16 = dy.view(np.uint16)
    g0 = np.random.default_rng(2).uniform(-1, 1, g.n_params).astype(np.float16).view(np.uint16)
    for kw in ({}, {"max_level": 0.6}, {"grad16": g0},
               {"max_level_per_sample": np.random.default_rng(1).uniform(0, 1.2, N).astype(np.float32)}):
        np.testing.assert_array_equal(gr.backward(g, pos, dy16, gr.LINEAR, **kw), orc.grid_backward_exact(og, pos, dy16, **kw))


def test_linear_input_grad(case, orc):
    og, g, table, pos, dy = case
    for ml in (1.0, 0.6):
        ref = orc.grid_input_grad(og, pos, table, dy.astype(np.float32), max_level=ml)
        got = gr.input_grad(g, pos, table, dy.astype(np.float32), gr.LINEAR, max_level=ml)
        assert (np.abs(got - ref) <= 1e-12 * np.abs(ref)).all()


def _corner_sums(g, table, dy, pos64):
    """A_l = sum_c |sum_f dL/dy T[e_c]| per sample and level [n, L]. The Smoothstep weight s and its derivatives obey
    |s| <= 1, |s1| <= 1.5, |s2| <= 6, |s3| = 12, so every second partial derivative of the level's sum_f dL/dy y is
    at most 6 scale_l^2 A_l and every third one at most 12 scale_l^3 A_l."""
    tab = np.asarray(table).view(np.float16).reshape(-1, g.F)
    out = np.zeros((pos64.shape[0], g.L))
    for l in range(g.L):
        base, _, _ = gr.level_setup(g, l, pos64, gr.LINEAR)
        for c in range(1 << g.D):
            out[:, l] += np.abs((dy[:, l * g.F:(l + 1) * g.F] * tab[gr.corner_index(g, l, base, c)].astype(np.float64)).sum(axis=1))
    return out


def _second_derivative_bound(g, table, dy, pos64):
    return (_corner_sums(g, table, dy, pos64) * np.array([float(s) ** 2 for s in g.scale])).sum(axis=1)


def test_smoothstep_gradient_is_the_derivative(case):
    """Central differences of the float64 forward, step h, against the analytic gradient at float64 positions. Per
    level, inside a cell the forward is a polynomial and the central difference is off by at most h^2 / 6 times the
    third derivative, <= 2 h^2 scale^3 A; where the stencil crosses a face the forward is only C1 and the error is at
    most h times the second derivative, <= 6 h scale^2 A. Rounding of the two float64 forwards adds about
    eps |terms| / h."""
    _, g, table, pos, dy = case
    x = pos.astype(np.float64)
    dyd = dy.astype(np.float64)
    h = 2.0 ** -30
    an = gr.input_grad(g, x, table, dyd, gr.SMOOTHSTEP)
    lin = gr.input_grad(g, x, table, dyd, gr.LINEAR)
    A = _corner_sums(g, table, dyd, x)
    sc = np.array([float(s) for s in g.scale])
    missed = np.zeros(x.shape[0], bool)
    for d in range(g.D):
        e = np.zeros(g.D)
        e[d] = h
        crosses = np.stack([gr.level_setup(g, l, x + e, gr.LINEAR)[0][:, d] != gr.level_setup(g, l, x - e, gr.LINEAR)[0][:, d]
                            for l in range(g.L)], axis=1)
        tol = (np.where(crosses, 6 * h * sc ** 2, 2 * h * h * sc ** 3) * A).sum(axis=1) + 2.0 ** -52 * 8 * (A.sum(axis=1) + 1) / h
        fd = ((gr.forward64(g, x + e, table, gr.SMOOTHSTEP) - gr.forward64(g, x - e, table, gr.SMOOTHSTEP)) * dyd).sum(axis=1) / (2 * h)
        assert (np.abs(fd - an[:, d]) <= tol).all(), (d, (np.abs(fd - an[:, d]) / tol).max())
        missed |= np.abs(fd - lin[:, d]) > tol
    # the bar notices a wrong derivative: the Linear gradient of the same table misses it almost everywhere
    assert missed.mean() > 0.9


def test_smoothstep_gradient_is_continuous_across_faces(case):
    """Pairs of float32 positions a few ulps either side of a cell face (different `base` in the fp32 setup), the
    levels finer than the face's switched off. The Smoothstep gradient is Lipschitz: a level's second derivatives are
    at most 6 scale^2 A, so across the pair it moves by at most 6 D sum_l scale_l^2 A_l (dx + r), r the two positions'
    fp32 rounding of p = fma(scale, x, 0.5) expressed as a shift of x, ulp(scale + 1) / scale at its largest. The
    Linear gradient jumps by the difference of two cells' slopes instead."""
    _, g, table, _, _ = case
    n = 96
    xm, xp, dim, lev, ml = gr.face_pairs(g, n, seed=3)
    dy = np.random.default_rng(4).uniform(-1, 1, (n, g.L * g.F))
    for j in range(n):  # the pair really straddles the face of its level
        bm, _, _ = gr.level_setup(g, lev[j], xm[j:j + 1], gr.LINEAR)
        bp, _, _ = gr.level_setup(g, lev[j], xp[j:j + 1], gr.LINEAR)
        assert bp[0, dim[j]] == bm[0, dim[j]] + 1
    dx = (xp.astype(np.float64) - xm.astype(np.float64)).max(axis=1)
    active = np.arange(g.L)[None, :] <= lev[:, None]
    sc2 = np.array([float(s) ** 2 for s in g.scale])
    B = np.maximum((_corner_sums(g, table, dy, xm.astype(np.float64)) * sc2 * active).sum(axis=1),
                   (_corner_sums(g, table, dy, xp.astype(np.float64)) * sc2 * active).sum(axis=1))
    round_p = max(float(np.spacing(np.float32(float(g.scale[l]) + 1))) / float(g.scale[l]) for l in range(lev.max() + 1))
    bound = 6 * B * g.D * (dx + round_p)
    jump = {}
    for mode in (gr.LINEAR, gr.SMOOTHSTEP):
        gp = gr.input_grad(g, xp, table, dy, mode, max_level_per_sample=ml)
        gm = gr.input_grad(g, xm, table, dy, mode, max_level_per_sample=ml)
        jump[mode] = np.abs(gp - gm)[np.arange(n), dim]
    print("jump / bound: smoothstep max %.3g, linear median %.3g" % ((jump[gr.SMOOTHSTEP] / bound).max(),
                                                                   np.median(jump[gr.LINEAR] / bound)))
    assert (jump[gr.SMOOTHSTEP] <= bound).all()
    # a random table makes two neighbouring cells' slopes agree to within the bound only by accident
    assert (jump[gr.LINEAR] > bound).mean() >= 0.9
