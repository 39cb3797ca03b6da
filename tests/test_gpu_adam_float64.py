"""The optimizer's kernels against the float64 reference (tests/adam_reference.py): multi-step Adam, skips, the
schedule, planted deep state.

The other optimizer tests show one implementation equal to another (eager == lazy == fused == captured); the Adam
arithmetic they share is compared with something outside the engine only for one step from a zero state. Here
gradients are written straight into Trainer.gradients and optimizer_step is called, so the kernels under test are
k_adam_ema4 (eager arrays, NGP_LAZY_EMA=0) and k_adam_lazy4 (records, NGP_LAZY_EMA=1) on inputs controlled to the
bit (adam_reference.gradient_patterns: all 16 activity masks of a group of four, skip lengths 1, 5, 20 and forever,
-0.0, zero-gradient matrix parameters, +-2^-24 and +-65504), on the smallest model that has both kinds of parameter
(adam_reference.TEST_ENCODING / TEST_NETWORK, 38,912 parameters). State is read after every step from
Trainer.serialize(): a 32-byte header (u64 magic, version, n, step) and w32, m1, m2, ema32, steps, each [n].

Odd group count: k_adam_lazy4's unpaired last group needs n / 4 odd. No supported model has it: every grid level holds
a multiple of 8 entries (grid_desc_init) and every MLP matrix a multiple of 256 weights, so n is a multiple of 8.

(a) ONE STEP AHEAD. For each step the reference starts from the engine's own state before the step; nothing
accumulates, so the bars are derived from the kernel text (u = 2^-24, one rounding of fp32; |.| = the sum of the
absolute values of a recurrence's terms, with |g| + l2 |w| for the gradient of a matrix parameter):

* m1: C_M1 = 7 roundings: g16 / loss_scale, l2 * w, g + l2 w, 1 - b1, (1 - b1) * g, b1 * m1, the sum.
      |m1 - ref| <= 7 u (b1 |m1| + (1 - b1) |g|)
* m2: C_M2 = 11: the three of g twice over in g * g, the product, 1 - b2, (1 - b2) * g^2, b2 * m2, the sum.
      |m2 - ref| <= 11 u (b2 m2 + (1 - b2) |g|^2)
* dw = w_after - w_before: C_W = 9 roundings relative to the step: 1 - b2^s, its sqrtf, 1 - b1^s, lr * q0, / q1,
  sqrtf(m2), + eps, lr_s / that, * m1; the k roundings of the schedule's k products; the device pow's error P in the
  cancellation A(s) = b2^s / (2 (1 - b2^s)) + b1^s / (1 - b1^s); m2's own error through the root, (C_M2 / 2) |m2| / m2.
  Two terms are not relative to dw and are carried as they are: m1's bar times the step factor f (m1's terms may
  cancel), and the one rounding of the subtraction w - f m1, u |w_after| (a weight cannot be stored more finely):
      |dw - ref| <= u (C_W + (C_M2 / 2) |m2| / m2 + k + P A(s)) |dw_ref| + f bar_m1 + u |w_after|
  P is measured once per session, outside the engine: torch.pow on float32 GPU tensors over the (beta, s) used
  here against float64, in units of 2^-24 relative (a correctly rounded result is <= 1); P = max(2, 2 x worst).
* ema32: C_E = 4: 1 - d, (1 - d) * w, d * e, the sum; the new weight's own bar enters with 1 - d.
      |e - ref| <= 4 u (d |e| + (1 - d) |w_after|) + (1 - d) bar_w
* exact: every counter, the header step; a skipped grid parameter's w, m1, m2 and counter bit for bit; w16 = fp16 of
  the engine's w32; the inference parameter within 1 ulp16 of the reference's.

(b) FREE-RUNNING. The reference runs alongside from the initial state for the same 40 steps; the bar is 4 x what the
fp32 oracle loses on the same inputs (adam_reference.ORACLE_FP32_LOSS, measured in test_adam_reference_host.py).
On the record layout the 40 steps are then repeated without reading the state in between (reading completes
every parameter's EMA, so only this run leaves skipped parameters owing EMA steps at their next update): the final
state must equal the step-by-step run's bit for bit.

DEEP STATE is planted through deserialize (header step and arrays patched) and gets check (a): the schedule's
boundaries at 20,000 and 30,000 with per-parameter counters drawn from [0, step]; the bias table's end (counters
2^20-3 .. 2^20+1: the table is read below 2^20, powf from there on, and both bias factors are 1 to the last bit, so the
step factor times the denominator is lr itself); the EMA debias, 1 at that depth. The fused and the captured
updates take no hand-made gradient, so at the same depths (C2 network, 2^14-entry table, 4,096 samples) they are
tied bit for bit to forward_backward + optimizer_step on the eager arrays, each step of which gets check (a).

Measured on an MI355X (reported per test through record_property): P = 3.05 (torch.pow is at most 1.52 x 2^-24 off);
one step ahead the engine uses at most 0.36 of the m1 bar, 0.44 of m2's, 0.48 of ema32's and 0.998 of dw's (that
one is the rounding of the stored weight: half an ulp is u |w| when |w| sits just above a power of two); free-running
it stays within 0.46 of the 4 x bar, that is within twice the oracle's own loss. Eager and lazy agree to the digit.
"""
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import adam_reference as ar  # noqa: E402

pytestmark = pytest.mark.gpu

U = ar.U
TINY = 2.0 ** -149  # the smallest fp32 subnormal: no fp32 result is closer to its exact value than it can be stored
C_M1, C_M2, C_W, C_E = 7, 11, 9, 4
HDR = 32
DEEP = (1 << 20) + 8


@pytest.fixture(scope="module")
def pkg():
    from __graft_entry__ import load_package
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return load_package()


@pytest.fixture(scope="module")
def pow_error(pkg):
    """P: the error of single-precision device pow over the (beta, s) of these tests, in units of 2^-24 relative."""
    betas = set()
    for opt in list(ar.CONFIGS.values()) + [ar.PLAIN_EMA]:
        h = ar.Hyper(opt)
        betas |= {h.beta1, h.beta2, h.decay}
    betas.discard(0.0)
    r = np.random.default_rng(5)
    s = np.unique(np.concatenate([np.arange(1, 65), r.integers(1, DEEP + 8, 4096), np.arange(19990, 20010),
                                  np.arange(29990, 30010), np.arange((1 << 20) - 8, DEEP + 8)])).astype(np.float64)
    worst = 0.0
    for b in sorted(betas):
        got = torch.pow(torch.full((s.size,), b, dtype=torch.float32, device="cuda"),
                        torch.from_numpy(s.astype(np.float32)).cuda()).cpu().numpy().astype(np.float64)
        want = b ** s
        ok = want >= 2.0 ** -100  # below, b^s vanishes against the 1 it is subtracted from
        assert np.all(got[~ok] <= 2.0 ** -99)
        worst = max(worst, float(np.max(np.abs(got[ok] - want[ok]) / (U * want[ok]))))
    return max(2.0, 2.0 * worst)


def make_trainer(pkg, opt, lazy, nerf=False):
    old = os.environ.get("NGP_LAZY_EMA")
    os.environ["NGP_LAZY_EMA"] = "1" if lazy else "0"
    try:
        if nerf:  # the C2 network of test_gpu_ema_gaps.py
            cfg = pkg.nerf_config("C2")
            cfg["encoding"]["log2_hashmap_size"] = 14
            net = pkg.create_nerf_network(cfg)
        else:
            net = pkg.NetworkWithInputEncoding(3, 1, ar.TEST_ENCODING, ar.TEST_NETWORK)
        tr = pkg.Trainer(net, opt, seed=1337)
    finally:
        if old is None:
            del os.environ["NGP_LAZY_EMA"]
        else:
            os.environ["NGP_LAZY_EMA"] = old
    return net, tr


def parse(blob):
    hdr = np.frombuffer(blob, np.uint64, 4)
    n = int(hdr[2])
    assert len(blob) == HDR + 20 * n
    a = lambda k, dt=np.float32: np.frombuffer(blob, dt, n, HDR + 4 * n * k)
    return SimpleNamespace(step=int(hdr[3]), w=a(0), m1=a(1), m2=a(2), ema=a(3), steps=a(4, np.uint32))


def planted(blob, step, w=None, m1=None, m2=None, ema=None, steps=None):
    """the blob with its header step and the given arrays replaced"""
    b = bytearray(blob)
    n = int(np.frombuffer(blob, np.uint64, 4)[2])
    b[24:32] = np.uint64(step).tobytes()
    for k, (a, dt) in enumerate(((w, np.float32), (m1, np.float32), (m2, np.float32), (ema, np.float32), (steps, np.uint32))):
        if a is not None:
            assert a.size == n
            b[HDR + 4 * n * k:HDR + 4 * n * (k + 1)] = np.ascontiguousarray(a, dt).tobytes()
    return bytes(b)


def read(tr):
    torch.cuda.synchronize()
    st = parse(tr.serialize())
    inf16 = tr.inference_params.cpu().numpy().copy()
    w16 = tr.params.cpu().numpy().copy()
    return st, inf16, w16


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype.itemsize == 4 else np.uint16)


def worst_of(name, diff, bar, out):
    ratio = np.where(diff == 0, 0.0, diff / bar)
    i = int(np.argmax(np.where(np.isfinite(ratio), ratio, np.inf)))
    out[name] = max(out.get(name, 0.0), float(ratio[i]) if np.isfinite(ratio[i]) else float("inf"))
    assert np.isfinite(ratio[i]) and ratio[i] <= 1.0, f"{name}: parameter {i} is {diff[i]:.6g} from the reference, bar {bar[i]:.6g}"


def check_one_step(ref, P, before, g16, ls, after, inf16, w16, worst):
    """check (a) of the module docstring for the step before.step: `before` and `after` are the engine's states"""
    h, t, nm = ref.h, before.step, ref.n_matrix
    f64 = lambda a: a.astype(np.float64)
    r = ar.State(before.w, before.m1, before.m2, before.ema, before.steps)
    ref_inf = ref.step(r, g16, t, ls)
    act = r.steps != before.steps
    # exact: counters, header, skipped parameters, w16
    assert after.step == t + 1
    np.testing.assert_array_equal(after.steps, r.steps)
    skipped = ~act
    assert not skipped[:nm].any(), "a matrix parameter was skipped by the reference"
    for name in ("w", "m1", "m2"):
        np.testing.assert_array_equal(bits(getattr(after, name))[skipped], bits(getattr(before, name))[skipped],
                                      err_msg=f"a skipped grid parameter's {name} changed")
    np.testing.assert_array_equal(bits(w16), bits(after.w.astype(np.float16)), err_msg="w16 is not the fp16 of w32")
    # the bars
    w0, m10, m20 = f64(before.w), f64(before.m1), f64(before.m2)
    l2 = np.where(np.arange(w0.size) < nm, h.l2, 0.0)
    ga = np.abs(f64(g16)) / ls + l2 * np.abs(w0)
    t1 = h.beta1 * np.abs(m10) + (1.0 - h.beta1) * ga
    t2 = h.beta2 * m20 + (1.0 - h.beta2) * ga * ga
    bar_m1 = C_M1 * U * t1 + TINY
    bar_m2 = C_M2 * U * t2 + TINY
    with np.errstate(all="ignore"):
        s = f64(r.steps)
        b1s, b2s = h.beta1 ** s, h.beta2 ** s
        A = np.where(act, b2s / (2.0 * (1.0 - b2s)) + b1s / (1.0 - b1s), 0.0)
        f = np.where(act, np.abs(ref.step_factor(r.steps, t, r.m2)), 0.0)
        via_m2 = np.where(act, 0.5 * C_M2 * t2 / r.m2, 0.0)
    k = ref.schedule_products(t)
    dw_ref = r.w - w0
    bar_w = np.where(act, U * (C_W + via_m2 + k + P * A) * np.abs(dw_ref) + f * bar_m1 + U * np.abs(r.w) + TINY, TINY)
    worst_of("m1", np.abs(f64(after.m1) - r.m1), bar_m1, worst)
    worst_of("m2", np.abs(f64(after.m2) - r.m2), bar_m2, worst)
    worst_of("dw", np.abs((f64(after.w) - w0) - dw_ref), bar_w, worst)
    if h.decay > 0.0:
        te = h.decay * np.abs(f64(before.ema)) + (1.0 - h.decay) * np.abs(r.w)
        bar_e = C_E * U * te + (1.0 - h.decay) * np.where(act, bar_w, 0.0) + TINY
        worst_of("ema", np.abs(f64(after.ema) - r.ema), bar_e, worst)
    else:
        np.testing.assert_array_equal(bits(inf16), bits(w16), err_msg="no Ema wrapper: the inference parameters are the weights")
    worst_of("inf_ulp16", np.abs(f64(inf16) - f64(ref_inf)), ar.ulp16(ref_inf), worst)
    return r


def record(record_property, prefix, worst):
    for q, v in worst.items():
        record_property(f"{prefix}_{q}", round(v, 4))


@pytest.mark.parametrize("ls", [1.0, 128.0, 32768.0])
@pytest.mark.parametrize("lazy", [False, True], ids=["eager", "lazy"])
@pytest.mark.parametrize("name", list(ar.CONFIGS))
def test_forty_steps_vs_float64(pkg, pow_error, record_property, name, lazy, ls):
    opt = ar.CONFIGS[name]
    net, tr = make_trainer(pkg, opt, lazy)
    n, nm = net.n_params, net.n_matrix_params
    assert (n, nm) == (ar.TEST_N, ar.TEST_N_MATRIX) and (n // 4) % 2 == 0
    ref = ar.Reference(opt, nm)
    G, lanes = ar.gradient_patterns(n, nm, ls)
    Gd = torch.from_numpy(G).cuda()
    before, _, _ = read(tr)
    blob0 = tr.serialize()
    assert before.step == 0 and not before.m1.any() and not before.steps.any()
    free = ar.State(before.w)
    one, run = {}, {}
    rec = ar.ORACLE_FP32_LOSS[name]
    for t in range(ar.N_STEPS):
        tr.gradients.copy_(Gd[t])
        tr.optimizer_step(ls)
        after, inf16, w16 = read(tr)
        check_one_step(ref, pow_error, before, G[t], ls, after, inf16, w16, one)
        free_inf = ref.step(free, G[t], t, ls)
        got = ar.loss_against(free, free_inf, after.w, after.m1, after.m2, after.ema, after.steps, inf16, has_ema=ref.h.decay > 0)
        for q, v in got.items():
            run[q] = max(run.get(q, 0.0), v / (4.0 * rec[q]))
        before = after
    record_property("P", pow_error)
    record(record_property, "one_step_ratio", one)
    record(record_property, "free_running_ratio", run)
    print(f"{name} {'lazy' if lazy else 'eager'} ls={ls}: P={pow_error}, one step ahead {one}, free-running {run}")
    # the lanes did what they are there for
    assert not after.steps[lanes["never"]].any() and (after.steps[lanes["always"]] == ar.N_STEPS).all()
    assert (after.steps[lanes["skip20"]] == 2).all() and (after.steps[lanes["negzero"]] == 6).all()
    assert (after.steps[:nm] == ar.N_STEPS).all(), "zero-gradient matrix parameters count too"
    grp = after.steps[lanes["masks"]].reshape(-1, 2)
    assert (grp[:, 0] != grp[:, 1]).any(), "the counters within a pair never diverged"
    assert all(v <= 1.0 for v in run.values()), f"free-running beyond 4 x the oracle's loss: {run}"
    if lazy:
        # the same steps without reading in between: skipped parameters owe EMA steps when they are next updated
        final = tr.serialize()
        final_inf = inf16
        tr.deserialize(blob0)
        for t in range(ar.N_STEPS):
            tr.gradients.copy_(Gd[t])
            tr.optimizer_step(ls)
        torch.cuda.synchronize()
        assert tr.serialize() == final, "owed EMA steps: the unread run differs from the step-by-step run"
        np.testing.assert_array_equal(bits(tr.inference_params.cpu().numpy()), bits(final_inf))


def deep_arrays(n, nm, step, w, seed, counters=None):
    """random non-zero moments, an EMA near the weights, counters drawn from [0, step] (or given)"""
    r = np.random.default_rng(seed)
    m1 = (r.standard_normal(n) * 10.0 ** r.uniform(-5, -1, n)).astype(np.float32)
    m1[m1 == 0] = np.float32(1e-3)
    m2 = ((np.abs(m1) * r.uniform(1.0, 3.0, n)) ** 2).astype(np.float32)
    ema = (w * r.uniform(0.9, 1.1, n)).astype(np.float32)
    steps = r.integers(0, step + 1, n).astype(np.uint32) if counters is None else counters
    steps[:nm] = step  # a matrix parameter is updated every step
    return m1, m2, ema, steps


@pytest.mark.parametrize("lazy", [False, True], ids=["eager", "lazy"])
@pytest.mark.parametrize("start,n_steps", [(19998, 4), (29999, 2)])
def test_schedule_boundaries_deep(pkg, pow_error, record_property, start, n_steps, lazy):
    opt = ar.CONFIGS["stock"]
    net, tr = make_trainer(pkg, opt, lazy)
    n, nm = net.n_params, net.n_matrix_params
    ref = ar.Reference(opt, nm)
    h = ref.h
    ls = 128.0
    G, _ = ar.gradient_patterns(n, nm, ls, n_steps=n_steps, seed=start)
    blob = tr.serialize()
    m1, m2, ema, steps = deep_arrays(n, nm, start, parse(blob).w, start)
    steps[nm:nm + 64] = np.arange(64)  # small counters too: bias factors far from 1
    tr.deserialize(planted(blob, start, m1=m1, m2=m2, ema=ema, steps=steps))
    before, _, _ = read(tr)
    assert before.step == start and np.array_equal(before.steps, steps) and np.array_equal(bits(before.m2), bits(m2))
    want_lr = {19998: [h.lr, h.lr, h.lr * h.base, h.lr * h.base], 29999: [h.lr * h.base, h.lr * h.base * h.base]}[start]
    worst = {}
    for k in range(n_steps):
        assert ref.lr_at(start + k) == want_lr[k]
        assert tr.learning_rate == pytest.approx(want_lr[k], rel=1e-6)
        tr.gradients.copy_(torch.from_numpy(G[k]).cuda())
        tr.optimizer_step(ls)
        after, inf16, w16 = read(tr)
        check_one_step(ref, pow_error, before, G[k], ls, after, inf16, w16, worst)
        before = after
    record_property("P", pow_error)
    record(record_property, "one_step_ratio", worst)


@pytest.mark.parametrize("lazy", [False, True], ids=["eager", "lazy"])
def test_bias_table_boundary_and_deep_ema(pkg, pow_error, record_property, lazy):
    opt = ar.PLAIN_EMA
    net, tr = make_trainer(pkg, opt, lazy)
    n, nm = net.n_params, net.n_matrix_params
    ref = ar.Reference(opt, nm)
    h = ref.h
    ls = 128.0
    G, _ = ar.gradient_patterns(n, nm, ls, n_steps=1, seed=3)
    blob = tr.serialize()
    r = np.random.default_rng(9)
    counters = ((1 << 20) - 3 + r.integers(0, 5, n)).astype(np.uint32)
    i = np.arange(n)
    counters[i % 16 < 5] = ((1 << 20) - 3 + i % 16)[i % 16 < 5]  # all five within two pairs, at every 16th parameter
    m1, m2, ema, _ = deep_arrays(n, nm, DEEP, parse(blob).w, 9, counters=counters.copy())  # matrix counters as drawn
    tr.deserialize(planted(blob, DEEP, m1=m1, m2=m2, ema=ema, steps=counters))
    before, _, _ = read(tr)
    assert before.step == DEEP and np.array_equal(before.steps, counters)
    tr.gradients.copy_(torch.from_numpy(G[0]).cuda())
    tr.optimizer_step(ls)
    after, inf16, w16 = read(tr)
    worst = {}
    ref_after = check_one_step(ref, pow_error, before, G[0], ls, after, inf16, w16, worst)
    act = after.steps != before.steps
    new = after.steps[act]
    for s in range((1 << 20) - 2, (1 << 20) + 3):  # table entries 2^20-2 and 2^20-1, powf from 2^20 on
        assert (new[: nm] == s).any() and (after.steps[nm:][act[nm:]] == s).any(), f"no matrix or no grid parameter at counter {s}"
    # both bias factors are 1 to the last bit: the reference's step is lr itself
    s = ref_after.steps[act].astype(np.float64)
    assert np.all(ref.lr_at(DEEP) * np.sqrt(1.0 - h.beta2 ** s) / (1.0 - h.beta1 ** s) == h.lr)
    # the EMA debias is 1 at this depth: the inference parameter is the plain fp16 of the advanced ema32
    assert 1.0 - h.decay ** (DEEP + 1) == 1.0
    np.testing.assert_array_equal(bits(inf16), bits(after.ema.astype(np.float16)))
    assert (bits(after.ema) != bits(before.ema)).mean() > 0.9, "the planted EMA did not advance"
    record_property("P", pow_error)
    record(record_property, "one_step_ratio", worst)


def nerf_batch(n, seed):
    g = np.random.default_rng(seed)
    c = np.zeros((n, 7), np.float32)
    c[:, :3] = g.random((n, 3))
    c[:, 3] = 0.01
    d = g.standard_normal((n, 3))
    c[:, 4:] = (d / np.linalg.norm(d, axis=1, keepdims=True) + 1) / 2
    dl = np.zeros((n, 16), np.float16)
    dl[:, :4] = g.uniform(-1, 1, (n, 4))
    return torch.from_numpy(c).cuda(), torch.from_numpy(dl).cuda()


@pytest.mark.parametrize("depth", ["schedule", "bias_table"])
def test_fused_and_captured_updates_deep(pkg, pow_error, record_property, depth):
    """The fused update in the grid backward and the captured two-step graph, from a planted deep state, against
    forward_backward + optimizer_step on the eager arrays (whose gradients are readable: check (a) per step)."""
    opt, start = (ar.CONFIGS["stock"], 19999) if depth == "schedule" else (ar.PLAIN_EMA, DEEP)
    N, ls = 4096, 128.0
    x, dl = nerf_batch(N, 21)
    blob = None
    results = {}
    for mode, lazy in (("eager", False), ("fused", True), ("graph", True)):
        net, tr = make_trainer(pkg, opt, lazy, nerf=True)
        n, nm = net.n_params, net.n_matrix_params
        assert tr.fused_update_active(N) == lazy
        if blob is None:
            b0 = tr.serialize()
            if depth == "schedule":
                m1, m2, ema, steps = deep_arrays(n, nm, start, parse(b0).w, 31)
            else:
                counters = ((1 << 20) - 3 + np.random.default_rng(32).integers(0, 5, n)).astype(np.uint32)
                m1, m2, ema, _ = deep_arrays(n, nm, start, parse(b0).w, 32, counters=counters.copy())
                steps = counters
            blob = planted(b0, start, m1=m1, m2=m2, ema=ema, steps=steps)
        tr.deserialize(blob)
        if mode == "eager":
            ref = ar.Reference(opt, nm)
            worst = {}
            before, _, _ = read(tr)
            assert before.step == start
            for k in range(2):
                net.forward_backward(x, dl)
                torch.cuda.synchronize()
                g16 = tr.gradients.cpu().numpy().copy()
                assert np.isfinite(g16.astype(np.float32)).all()
                nz = np.count_nonzero(g16[nm:])
                assert 0 < nz < n - nm, "the batch must leave some grid parameters with and some without a gradient"
                tr.optimizer_step(ls)
                after, inf16, w16 = read(tr)
                check_one_step(ref, pow_error, before, g16, ls, after, inf16, w16, worst)
                before = after
            record_property("P", pow_error)
            record(record_property, "one_step_ratio", worst)
        elif mode == "fused":
            for k in range(2):
                tr.train_step(x, dl, ls)
        else:
            s = torch.cuda.Stream()
            with torch.cuda.stream(s):
                graph = tr.capture_training_step(x, dl, ls, n_steps=2, stream=s)
                graph.launch(s)
            s.synchronize()
            del graph
        torch.cuda.synchronize()
        assert tr.step == start + 2
        results[mode] = (tr.serialize(), bits(tr.inference_params.cpu().numpy()).copy(), bits(tr.params.cpu().numpy()).copy())
        del net, tr
    for mode in ("fused", "graph"):
        assert results[mode][0] == results["eager"][0], f"{mode}: serialized optimizer state differs from the eager run"
        np.testing.assert_array_equal(results[mode][1], results["eager"][1])
        np.testing.assert_array_equal(results[mode][2], results["eager"][2])
