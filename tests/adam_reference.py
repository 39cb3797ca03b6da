"""Float64 reference of the optimizer chain Ema(ExponentialDecay(Adam)), and the inputs the optimizer tests share.

Plain module (numpy only), written from the chain's definition rather than from any implementation in this
repository. Per parameter i at optimizer step t (0-based), all arithmetic in float64, the hyperparameters first
rounded to float32 (as the engine parses them), the fp16 gradient widened exactly:

    g = g16 / loss_scale
    a non-matrix parameter (i >= n_matrix) with g == 0 (-0.0 included) keeps w, m1, m2 and its counter; otherwise
        g  += l2 w                      (matrix parameters only)
        m1  = b1 m1 + (1 - b1) g
        m2  = b2 m2 + (1 - b2) g^2
        s   = ++steps[i]
        w  -= lr_t sqrt(1 - b2^s) / (1 - b1^s) / (sqrt(m2) + eps) m1
    lr_t = lr base^k, k = (t - start) / interval + 1 once t >= start and interval > 0, formed as k successive
    products (the definition the engine follows)
    decay > 0: e = d e + (1 - d) w for every parameter every step; inference parameter = fp16(e / (1 - d^(t+1)));
    no Ema wrapper: the inference parameters are the weights, fp16(w).

Reference(optimizer, n_matrix).step(state, g16, t, loss_scale) advances a State in place and returns the fp16
inference parameters. `optimizer` is the nested dict that Trainer takes. The small methods of Reference (bias_step,
l2_mask, active, denominator, schedule_products, debias_exponent) are the places where an implementation can be
subtly wrong; the host tests override them one at a time to show that the tests' bars notice.

Next to w, m1, m2 and ema a State carries each quantity's MAGNITUDE SCALE: the same recurrence evaluated on the
absolute values of its terms (s1 = b1 s1 + (1 - b1) (|g| + l2 |w|), s2 likewise with the square, sw = |w0| + the
sum over steps of step_factor * s1, se = d se + (1 - d) sw). Every rounding of an fp32 evaluation is relative to a
partial result no larger than that scale, so errors of free-running fp32 implementations are quoted in units of
2^-24 * scale (ORACLE_FP32_LOSS below, tests/test_adam_reference_host.py).
"""
import numpy as np

U = 2.0 ** -24  # unit roundoff of float32


def _f32(x):
    return float(np.float32(x))


class Hyper:
    """The nested optimizer dict flattened, with the engine's defaults for absent keys, rounded to float32."""

    def __init__(self, optimizer):
        self.decay = 0.0
        self.start, self.interval, self.base = 0, 0, 1.0
        j = optimizer
        while True:
            ot = j.get("otype", "Adam").lower()
            if ot == "ema":
                self.decay = _f32(j.get("decay", 0.99))
            elif ot == "exponentialdecay":
                self.start = int(j.get("decay_start", 0))
                self.interval = int(j.get("decay_interval", 10000))
                self.base = _f32(j.get("decay_base", 0.1))
            elif ot == "adam":
                self.lr = _f32(j.get("learning_rate", 1e-3))
                self.beta1 = _f32(j.get("beta1", 0.9))
                self.beta2 = _f32(j.get("beta2", 0.999))
                self.eps = _f32(j.get("epsilon", 1e-8))
                self.l2 = _f32(j.get("l2_reg", 1e-8))
                return
            else:
                raise ValueError(f"optimizer otype {j.get('otype')!r}")
            j = j["nested"]


class State:
    """w, m1, m2, ema (float64 [n]), steps (int64 [n]) and the magnitude scales sw, s1, s2, se (module docstring)."""

    def __init__(self, w, m1=None, m2=None, ema=None, steps=None):
        f = lambda a: np.zeros(len(w), np.float64) if a is None else np.asarray(a).astype(np.float64)
        self.w, self.m1, self.m2, self.ema = f(w), f(m1), f(m2), f(ema)
        self.steps = np.zeros(len(w), np.int64) if steps is None else np.asarray(steps).astype(np.int64)
        self.sw, self.s1, self.s2, self.se = np.abs(self.w), np.abs(self.m1), np.abs(self.m2), np.abs(self.ema)

    def copy(self):
        c = State.__new__(State)
        for k in ("w", "m1", "m2", "ema", "steps", "sw", "s1", "s2", "se"):
            setattr(c, k, getattr(self, k).copy())
        return c


class Reference:
    def __init__(self, optimizer, n_matrix):
        self.h = Hyper(optimizer)
        self.n_matrix = int(n_matrix)

    # ---- the places where an implementation can be subtly wrong -------------------------------------------------
    def schedule_products(self, t):
        """k of lr_t = lr base^k"""
        h = self.h
        if h.interval == 0 or t < h.start:
            return 0
        return (t - h.start) // h.interval + 1

    def bias_step(self, s, t):
        """the exponent of the bias correction: the parameter's own counter after the increment"""
        return s

    def l2_mask(self, n):
        return np.arange(n) < self.n_matrix

    def active(self, g):
        """False where the parameter is skipped: a non-matrix parameter whose gradient is zero of either sign"""
        return ~((np.arange(g.size) >= self.n_matrix) & (g == 0.0))

    def denominator(self, m2, s):
        return np.sqrt(m2) + self.h.eps

    def debias_exponent(self, t):
        return t + 1

    # --------------------------------------------------------------------------------------------------------------
    def lr_at(self, t):
        r = self.h.lr
        for _ in range(self.schedule_products(t)):
            r *= self.h.base
        return r

    def step_factor(self, s, t, m2):
        """lr_t sqrt(1 - b2^s) / (1 - b1^s) / (sqrt(m2) + eps): what multiplies m1"""
        h = self.h
        sb = np.asarray(self.bias_step(s, t), np.float64)
        return self.lr_at(t) * np.sqrt(1.0 - h.beta2 ** sb) / (1.0 - h.beta1 ** sb) / self.denominator(m2, sb)

    def step(self, st, g16, t, loss_scale):
        h = self.h
        g16 = np.asarray(g16)
        assert g16.dtype == np.float16 and g16.size == st.w.size
        g = g16.astype(np.float64) / _f32(loss_scale)
        act = self.active(g)
        l2 = np.where(self.l2_mask(g.size), h.l2, 0.0)
        ga = np.abs(g) + l2 * np.abs(st.w)
        g = g + l2 * st.w
        with np.errstate(all="ignore"):
            m1 = h.beta1 * st.m1 + (1.0 - h.beta1) * g
            m2 = h.beta2 * st.m2 + (1.0 - h.beta2) * g * g
            s1 = h.beta1 * st.s1 + (1.0 - h.beta1) * ga
            s2 = h.beta2 * st.s2 + (1.0 - h.beta2) * ga * ga
            s = st.steps + 1
            f = self.step_factor(s, t, m2)
            w = st.w - f * m1
            sw = st.sw + np.abs(f) * s1
        st.m1 = np.where(act, m1, st.m1)
        st.m2 = np.where(act, m2, st.m2)
        st.s1 = np.where(act, s1, st.s1)
        st.s2 = np.where(act, s2, st.s2)
        st.steps = np.where(act, s, st.steps)
        st.w = np.where(act, w, st.w)
        st.sw = np.where(act, sw, st.sw)
        with np.errstate(all="ignore"):
            if h.decay > 0.0:
                st.ema = h.decay * st.ema + (1.0 - h.decay) * st.w
                st.se = h.decay * st.se + (1.0 - h.decay) * st.sw
                return (st.ema / (1.0 - h.decay ** float(self.debias_exponent(t)))).astype(np.float16)
            return st.w.astype(np.float16)


# ---- the configs and inputs that the host tests and the GPU tests share ---------------------------------------------

def _chain(adam, decay=None, ema=None):
    o = dict(adam, otype="Adam")
    if decay is not None:
        o = {"otype": "ExponentialDecay", "decay_start": decay[0], "decay_interval": decay[1], "decay_base": decay[2], "nested": o}
    if ema is not None:
        o = {"otype": "Ema", "decay": ema, "nested": o}
    return o


_STOCK_ADAM = {"learning_rate": 1e-2, "beta1": 0.9, "beta2": 0.99, "epsilon": 1e-15, "l2_reg": 1e-6}
CONFIGS = {
    # the NeRF base optimizer
    "stock": _chain(_STOCK_ADAM, (20000, 10000, 0.33), 0.95),
    # every term large enough to be seen; the schedule is crossed several times within 12 steps
    "sharp": _chain({"learning_rate": 3e-3, "beta1": 0.8, "beta2": 0.95, "epsilon": 1e-3, "l2_reg": 1e-2}, (3, 2, 0.5), 0.9),
    # Adam alone: the inference parameters are the weights
    "plain": _chain(_STOCK_ADAM),
}
# the deep bias-table case: plain plus an Ema (the stock schedule would have driven the learning rate to zero)
PLAIN_EMA = _chain(_STOCK_ADAM, None, 0.95)

N_STEPS = 40
# the test model: NetworkWithInputEncoding(3, 1, HashGrid L=4 F=2 T=2^12 base 16, 64 x 2 MLP)
TEST_ENCODING = {"otype": "HashGrid", "n_levels": 4, "n_features_per_level": 2, "log2_hashmap_size": 12, "base_resolution": 16,
                 "per_level_scale": 2.0}
TEST_NETWORK = {"otype": "FullyFusedMLP", "activation": "ReLU", "output_activation": "None", "n_neurons": 64, "n_hidden_layers": 2}
TEST_N_MATRIX = 16 * 64 + 64 * 64 + 64 * 16  # input and output padded to 16
TEST_N = TEST_N_MATRIX + 4 * 4096 * 2       # 38,912: four levels of 2^12 entries (16^3 = 2^12 fills level 0), 2 features

F16_MAX, F16_TINY = 0x7BFF, 0x0001  # 65504 and the smallest subnormal 2^-24, as bit patterns
NEG = 0x8000


def gradient_patterns(n, n_matrix, loss_scale, n_steps=N_STEPS, seed=20240607):
    """fp16 gradients [n_steps, n] (as the backward leaves them: scaled by loss_scale) and the lanes placed on purpose.

    Normal values at per-parameter scales from 1e-3 to 10; every other grid parameter zero with probability 0.7 per
    step; and, in lanes (dict name -> indices):
    * "masks" and "masks_end": grid groups of four aligned to a multiple of 4, at the start of the grid and as its
      last groups (the lazy kernel's second group per thread), run through all 16 zero/non-zero masks; group j has
      mask (j + 5 t) % 16 at step t, so the counters within a pair diverge;
    * "never", "always", "skip1", "skip5", "skip20": grid parameters never touched, touched every step, and touched
      every 2nd, 6th and 21st step; "negzero": touched every 7th step and given -0.0 in between;
    * "mat_zero", "mat_negzero": matrix parameters whose gradient is always +0.0 / -0.0 (they move by l2 and count);
      "mat_some": matrix parameters zero on two steps out of three;
    * "tiny_m", "tiny_g", "huge_m", "huge_g": +-2^-24 and +-65504 (signs alternate by lane and step) on matrix and
      grid parameters; the 65504 lanes only at loss scale 1 or 128.
    """
    assert n_matrix % 4 == 0 and n % 4 == 0 and n_matrix >= 256 and n - n_matrix >= 1024
    r = np.random.default_rng(seed)
    scale = 10.0 ** r.uniform(-3, 1, n)
    G = (r.standard_normal((n_steps, n)) * scale).astype(np.float16)
    zero = r.random((n_steps, n)) < 0.7
    zero[:, :n_matrix] = False
    G[zero] = 0
    bits = G.view(np.uint16)
    t = np.arange(n_steps)
    lanes = {}
    nm = n_matrix

    def take(name, lo, cnt):
        lanes[name] = np.arange(lo, lo + cnt)
        return lanes[name]

    vals = (r.standard_normal((n_steps, 512)) * 10.0 ** r.uniform(-3, 1, 512)).astype(np.float16)
    vals[vals == 0] = np.float16(0.5)
    for name, lo in (("masks", nm), ("masks_end", n - 256)):
        idx = take(name, lo, 256)
        grp, bit = np.arange(256) // 4, np.arange(256) % 4
        on = (((grp[None, :] + 5 * t[:, None]) % 16) >> bit[None, :]) & 1
        G[:, idx] = np.where(on == 1, vals[:, :256], np.float16(0))
    lo = nm + 256
    G[:, take("never", lo, 16)] = 0
    G[:, take("always", lo + 16, 16)] = vals[:, 256:272]
    for name, off, period in (("skip1", 32, 2), ("skip5", 48, 6), ("skip20", 64, 21)):
        G[:, take(name, lo + off, 16)] = np.where((t % period == 0)[:, None], vals[:, 272:288], np.float16(0))
    idx = take("negzero", lo + 80, 16)
    G[:, idx] = vals[:, 288:304]
    bits[np.ix_(t % 7 != 0, idx)] = NEG
    G[:, take("mat_zero", 64, 16)] = 0
    bits[:, take("mat_negzero", 80, 16)] = NEG
    G[:, take("mat_some", 96, 16)] = np.where((t % 3 == 0)[:, None], vals[:, 304:320], np.float16(0))
    sign = (((np.arange(16)[None, :] + t[:, None]) % 2) * NEG).astype(np.uint16)
    bits[:, take("tiny_m", 112, 16)] = F16_TINY | sign
    bits[:, take("tiny_g", lo + 96, 16)] = F16_TINY | sign
    take("huge_m", 128, 16)
    take("huge_g", lo + 112, 16)
    if loss_scale in (1.0, 128.0):
        bits[:, lanes["huge_m"]] = F16_MAX | sign
        bits[:, lanes["huge_g"]] = F16_MAX | sign
    return G, lanes


def initial_weights(n, n_matrix, seed=7):
    """Host stand-in for a fresh trainer's weights: matrices uniform in +-0.2, grid entries uniform in +-1e-4."""
    r = np.random.default_rng(seed)
    w = r.uniform(-1e-4, 1e-4, n)
    w[:n_matrix] = r.uniform(-0.2, 0.2, n_matrix)
    return w.astype(np.float32)


def ulp16(x):
    """the spacing of fp16 at |x| (2^-24 below the normal range)"""
    x = np.abs(np.asarray(x, np.float64))
    return 2.0 ** (np.floor(np.log2(np.maximum(x, 2.0 ** -14))) - 10)


QUANTITIES = ("w", "m1", "m2", "ema", "inf")


def loss_against(ref_state, ref_inf, w, m1, m2, ema, steps, inf16, has_ema=True):
    """Worst error of an fp32 implementation's state against the reference's: w, m1, m2 and ema in units of
    2^-24 * the quantity's magnitude scale, the fp16 inference parameters in ulp16 of the reference's value. A counter
    that differs, a value that is not finite, or a difference where the scale is zero counts as infinite."""
    out = {}
    pairs = [("w", w, ref_state.w, ref_state.sw), ("m1", m1, ref_state.m1, ref_state.s1), ("m2", m2, ref_state.m2, ref_state.s2)]
    if has_ema:
        pairs.append(("ema", ema, ref_state.ema, ref_state.se))
    with np.errstate(all="ignore"):
        for name, got, want, scale in pairs:
            d = np.abs(np.asarray(got, np.float64) - want)
            ratio = np.where(d == 0, 0.0, d / (U * scale))
            out[name] = float(np.max(np.where(np.isfinite(ratio), ratio, np.inf)))
        ri = np.asarray(ref_inf).astype(np.float64)
        d = np.abs(np.asarray(inf16).astype(np.float64) - ri) / ulp16(ri)
        out["inf"] = float(np.max(np.where(np.isfinite(d), d, np.inf)))
    if not np.array_equal(np.asarray(steps).astype(np.int64), ref_state.steps):
        out["w"] = float("inf")
    return out


# What an honest fp32 evaluation of the recurrence (the oracle's orc_adam_step, free-running for N_STEPS steps from
# initial_weights on gradient_patterns, worst over steps, parameters and the loss scales 1, 128 and 2^15) loses
# against this reference, in the units of loss_against. Measured by tests/test_adam_reference_host.py, which
# asserts the oracle against 2x these; the free-running GPU bar (tests/test_gpu_adam_float64.py) is 4x these.
ORACLE_FP32_LOSS = {
    "stock": {"w": 8.0, "m1": 12.0, "m2": 17.0, "ema": 10.0, "inf": 1.0},
    "sharp": {"w": 12.0, "m1": 11.0, "m2": 19.0, "ema": 12.0, "inf": 1.0},
    "plain": {"w": 8.0, "m1": 12.0, "m2": 17.0, "inf": 1.0},
}
