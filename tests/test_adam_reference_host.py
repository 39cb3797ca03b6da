"""The float64 optimizer reference (tests/adam_reference.py) checked on the host, and the fp32 oracle against it.

* The reference against torch.optim.Adam in float64 (an implementation nobody here wrote): 50 steps, 1,000 parameters,
  eps = 0 (torch bias-corrects sqrt(v) before adding eps and this chain does not, so they coincide only there),
  weight_decay = l2 with every parameter a matrix parameter, the learning rate set per step from the reference's
  schedule. 1e-12 relative on w, m1 and m2.
* Skip semantics worked by hand on one grid and one matrix parameter.
* The oracle's orc_adam_step (fp32, oracle/ngp_oracle.c) free-running for 40 steps on the three configs and the
  gradient patterns the GPU tests use (adam_reference.gradient_patterns on the GPU tests' model size), against the
  reference running alongside. This closes the oracle's own gap (tests/test_oracle.py checks it at step 0 only) and
  MEASURES what an honest fp32 evaluation of the recurrence loses over 40 steps. Worst over steps, parameters and
  the loss scales 1, 128 and 2^15; w, m1, m2 and ema32 in units of 2^-24 x the quantity's magnitude scale (the
  recurrence on absolute values, adam_reference module docstring), the fp16 inference parameters in ulp16:

      config   w       m1      m2      ema32   inference
      stock    7.99    11.57   16.12   9.53    1
      sharp    11.32   10.72   18.48   11.37   1
      plain    7.99    11.57   16.12   -       1    (the weights' own fp16 rounding)

  These figures are adam_reference.ORACLE_FP32_LOSS (rounded up). The oracle is asserted against 2x them, so a
  later oracle change cannot drift silently; the free-running GPU bar of tests/test_gpu_adam_float64.py is 4x them
  (the device's powf and division sequence differ from the host's by an ulp here and there, and the error feeds
  forward through w -> l2).
* The bars bite: each of seven deliberate changes to the reference (test_bar_bites; the bias-correction step in both
  directions) puts the oracle-vs-reference comparison beyond the 4x bar on at least one config.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import adam_reference as ar  # noqa: E402

LOSS_SCALES = (1.0, 128.0, 32768.0)
N, NM = ar.TEST_N, ar.TEST_N_MATRIX


def test_reference_matches_torch_adam_float64():
    opt = ar._chain({"learning_rate": 3e-3, "beta1": 0.8, "beta2": 0.95, "epsilon": 0.0, "l2_reg": 1e-2}, (3, 2, 0.5), 0.9)
    n, steps, ls = 1000, 50, 128.0
    ref = ar.Reference(opt, n_matrix=n)
    h = ref.h
    r = np.random.default_rng(11)
    w0 = r.uniform(-0.2, 0.2, n).astype(np.float32)
    G = (r.standard_normal((steps, n)) * 10.0 ** r.uniform(-1, 3, n)).astype(np.float16)
    G[G == 0] = np.float16(1.0)
    st = ar.State(w0)
    p = torch.nn.Parameter(torch.from_numpy(w0.astype(np.float64)))
    topt = torch.optim.Adam([p], lr=h.lr, betas=(h.beta1, h.beta2), eps=0.0, weight_decay=h.l2, foreach=False)
    lrs = []
    for t in range(steps):
        ref.step(st, G[t], t, ls)
        topt.param_groups[0]["lr"] = ref.lr_at(t)
        lrs.append(ref.lr_at(t))
        p.grad = torch.from_numpy(G[t].astype(np.float64) / ls)
        topt.step()
    assert lrs[2] == h.lr and lrs[3] == h.lr * h.base and lrs[5] == h.lr * h.base * h.base  # the schedule was crossed
    assert len(set(lrs)) > 10
    s = topt.state[p]
    np.testing.assert_allclose(st.w, p.detach().numpy(), rtol=1e-12, atol=0)
    np.testing.assert_allclose(st.m1, s["exp_avg"].numpy(), rtol=1e-12, atol=0)
    np.testing.assert_allclose(st.m2, s["exp_avg_sq"].numpy(), rtol=1e-12, atol=0)
    assert np.all(st.steps == steps)


def test_skip_semantics_by_hand():
    """Parameter 0 is a matrix parameter, parameter 1 a grid parameter; both get the gradients [x, 0, 0, -0.0, y]."""
    ref = ar.Reference(ar.CONFIGS["stock"], n_matrix=1)
    h = ref.h
    x, y = np.float16(0.75), np.float16(-1.5)
    seq = [x, np.float16(0), np.float16(0), np.float16(-0.0), y]
    assert np.signbit(seq[3])
    st = ar.State(np.array([0.25, 0.25]))
    hist = [st.copy()]
    infs = []
    for t, g in enumerate(seq):
        infs.append(ref.step(st, np.array([g, g], np.float16), t, 1.0))
        hist.append(st.copy())
    assert st.steps.tolist() == [5, 2]
    for t in (1, 2, 3):  # the three middle steps: the grid parameter keeps everything but its EMA
        a, b = hist[t], hist[t + 1]
        assert b.w[1] == a.w[1] and b.m1[1] == a.m1[1] and b.m2[1] == a.m2[1] and b.steps[1] == a.steps[1]
        assert b.w[0] != a.w[0] and b.steps[0] == a.steps[0] + 1  # the matrix parameter moves by l2 alone
        assert b.ema[1] == h.decay * a.ema[1] + (1 - h.decay) * a.w[1] and b.ema[1] != a.ema[1]
    # the grid parameter by hand: two Adam steps with counters 1 and 2, five EMA steps
    w, m1, m2, e = 0.25, 0.0, 0.0, 0.0
    s = 0
    for t, g in enumerate(seq):
        g = float(g)
        if g != 0.0:
            m1 = h.beta1 * m1 + (1 - h.beta1) * g
            m2 = h.beta2 * m2 + (1 - h.beta2) * g * g
            s += 1
            w -= h.lr * np.sqrt(1 - h.beta2 ** s) / (1 - h.beta1 ** s) / (np.sqrt(m2) + h.eps) * m1
        e = h.decay * e + (1 - h.decay) * w
        assert infs[t][1] == np.float16(e / (1 - h.decay ** (t + 1)))
    assert s == 2
    assert st.w[1] == pytest.approx(w, rel=1e-15) and st.m1[1] == pytest.approx(m1, rel=1e-15)
    assert st.m2[1] == pytest.approx(m2, rel=1e-15) and st.ema[1] == pytest.approx(e, rel=1e-15)
    # first step of both: |dw| = lr (bias-corrected m1 / sqrt(m2) = sign g), the matrix one shifted by l2 w
    assert hist[1].w[1] == pytest.approx(0.25 - h.lr, rel=1e-12)
    assert hist[1].w[0] == pytest.approx(0.25 - h.lr, rel=1e-12)


# ---- the fp32 oracle, free-running, against the reference -------------------------------------------------------------

_ORACLE_RUNS = {}


def oracle_run(orc, name, ls):
    """orc_adam_step for N_STEPS steps; the fp32 state after every step (computed once per config and loss scale)"""
    key = (name, ls)
    if key not in _ORACLE_RUNS:
        h = ar.Hyper(ar.CONFIGS[name])
        cfg = orc.AdamCfg(h.lr, h.beta1, h.beta2, h.eps, h.l2, h.decay, h.start, h.interval, h.base)
        G, _ = ar.gradient_patterns(N, NM, ls)
        w32 = ar.initial_weights(N, NM)
        w16 = orc.f32_to_f16_bits(w32)
        m1, m2, e32 = np.zeros(N, np.float32), np.zeros(N, np.float32), np.zeros(N, np.float32)
        steps, e16 = np.zeros(N, np.uint32), np.zeros(N, np.uint16)
        hist = []
        for t in range(ar.N_STEPS):
            orc.adam_step(cfg, t, NM, ls, w32, w16, np.ascontiguousarray(G[t]).view(np.uint16), m1, m2, steps, e32, e16)
            inf = (e16 if h.decay > 0 else w16).copy().view(np.float16)
            hist.append((w32.copy(), m1.copy(), m2.copy(), e32.copy(), steps.copy(), inf))
        _ORACLE_RUNS[key] = (G, hist)
    return _ORACLE_RUNS[key]


def oracle_loss(orc, name, ref_cls=ar.Reference):
    """worst oracle-vs-reference error per quantity over steps, parameters and loss scales"""
    worst = {}
    for ls in LOSS_SCALES:
        G, hist = oracle_run(orc, name, ls)
        ref = ref_cls(ar.CONFIGS[name], NM)
        st = ar.State(ar.initial_weights(N, NM))
        for t in range(ar.N_STEPS):
            inf = ref.step(st, G[t], t, ls)
            w, m1, m2, e, steps, inf16 = hist[t]
            for q, v in ar.loss_against(st, inf, w, m1, m2, e, steps, inf16, has_ema=ref.h.decay > 0).items():
                worst[q] = max(worst.get(q, 0.0), v)
    return worst


@pytest.mark.parametrize("name", list(ar.CONFIGS))
def test_oracle_free_running_vs_reference(orc, name, record_property):
    got = oracle_loss(orc, name)
    rec = ar.ORACLE_FP32_LOSS[name]
    print(f"oracle vs float64 over {ar.N_STEPS} steps, {name}: " + ", ".join(f"{q} {v:.3f}" for q, v in got.items()))
    for q, v in got.items():
        record_property(f"oracle_loss_{name}_{q}", v)
    assert set(got) == set(rec)
    for q, v in got.items():
        assert v <= 2 * rec[q], f"{name} {q}: the oracle is {v:.3f} from the reference, recorded {rec[q]}"
        assert v >= rec[q] / 4 or q == "inf", f"{name} {q}: recorded {rec[q]} but the oracle loses only {v:.3f}: re-measure"


def test_gradient_patterns_cover_the_lanes():
    G, lanes = ar.gradient_patterns(N, NM, 128.0)
    nz = G != 0
    for name in ("masks", "masks_end"):
        idx = lanes[name]
        assert idx[0] % 4 == 0 and idx[0] >= NM
        m = nz[:, idx].reshape(ar.N_STEPS, -1, 4)
        codes = (m * np.array([1, 2, 4, 8])).sum(-1)
        assert set(np.unique(codes)) == set(range(16))
        assert all(len(set(codes[:, j])) == 16 for j in range(codes.shape[1]))  # every group sees every mask
    assert lanes["masks_end"][-1] == N - 1
    assert not nz[:, lanes["never"]].any() and nz[:, lanes["always"]].all()
    assert nz[:, lanes["skip20"]].sum(0).tolist() == [2] * 16 and nz[:, lanes["skip5"]].sum(0).tolist() == [7] * 16
    b = G.view(np.uint16)
    assert (b[1, lanes["negzero"]] == 0x8000).all() and (b[:, lanes["mat_negzero"]] == 0x8000).all()
    assert lanes["mat_zero"].max() < NM and lanes["huge_m"].max() < NM and lanes["huge_g"].min() >= NM
    assert set(np.unique(b[:, lanes["huge_g"]])) == {0x7BFF, 0xFBFF} and set(np.unique(b[:, lanes["tiny_m"]])) == {0x0001, 0x8001}
    G15, _ = ar.gradient_patterns(N, NM, 32768.0)
    assert np.abs(G15[:, lanes["huge_g"]].astype(np.float32)).max() < 65504


# ---- the bars bite -------------------------------------------------------------------------------------------------------

class BiasStepPlus(ar.Reference):
    def bias_step(self, s, t):
        return s + 1


class BiasStepMinus(ar.Reference):
    def bias_step(self, s, t):
        return s - 1


class BiasGlobalStep(ar.Reference):
    def bias_step(self, s, t):
        return np.full_like(s, t + 1)


class L2Everywhere(ar.Reference):
    def l2_mask(self, n):
        return np.ones(n, bool)


class EpsUnderRootScaling(ar.Reference):  # torch's placement: sqrt(m2) / sqrt(1 - b2^s) + eps
    def denominator(self, m2, s):
        return np.sqrt(m2) + self.h.eps * np.sqrt(1.0 - self.h.beta2 ** s)


class ScheduleOneStepLate(ar.Reference):
    def schedule_products(self, t):
        return super().schedule_products(t - 1) if t > 0 else 0


class DebiasExponentT(ar.Reference):
    def debias_exponent(self, t):
        return t


class ZeroGradientUpdated(ar.Reference):
    def active(self, g):
        return np.ones(g.size, bool)


MUTANTS = [BiasStepPlus, BiasStepMinus, BiasGlobalStep, L2Everywhere, EpsUnderRootScaling, ScheduleOneStepLate, DebiasExponentT,
           ZeroGradientUpdated]


@pytest.mark.parametrize("mutant", MUTANTS, ids=lambda c: c.__name__)
def test_bar_bites(orc, mutant):
    """The oracle against a deliberately changed reference must exceed the free-running GPU bar (4x the recorded
    loss, the widest bar in use) in some quantity on at least one config."""
    beyond = {}
    for name in ar.CONFIGS:
        got = oracle_loss(orc, name, mutant)
        beyond[name] = {q: v / (4 * ar.ORACLE_FP32_LOSS[name][q]) for q, v in got.items() if v > 4 * ar.ORACLE_FP32_LOSS[name][q]}
    print(mutant.__name__, beyond)
    assert any(beyond.values()), f"{mutant.__name__} stays within the bars on every config: the inputs are too tame"
