"""NumPy restatement of the multiresolution grid encoding with a selectable interpolation mode.

Plain module (numpy only). The CPU oracle knows Linear interpolation alone, so the Smoothstep tests measure against
this restatement, and tests/test_grid_reference_host.py anchors it: in Linear mode it equals the oracle's forward
and exact backward bit for bit and its input gradient to 1e-12, so the only text the oracle does not vouch for is
`interp()` below.

Per level l and dimension d (tcnn GridEncoding):

    p = fma(scale_l, x_d, 0.5)      base_d = floor(p)      frac_d = p - base_d            (fp32)
    Smoothstep:  deriv_d = 6 frac_d (1 - frac_d)   then   frac_d = frac_d frac_d (3 - 2 frac_d)   (fp32)
    w_c = prod_d (bit d of c ? frac_d : 1 - frac_d), starting from 1, in dimension order     (fp32)

forward       y[l, f] = fp16( fma(w_c, T[e_c, f], acc) over c = 0 .. 2^D - 1 from acc = 0 )     fp32, one RNE rounding
backward      grad[e_c, f] = fp16( fp32(sum over samples of fp16(fp32(w_c * dL/dy[l, f])) ) [+ fp32(grad0)] )
              the fp16 contributions are summed exactly as integers in units of 2^-24 and rounded once
input grad    dL/dx_d = sum_l scale_l deriv_d sum_c (+-) prod_{e != d} w_e(c) sum_f dL/dy[l, f] T[e_c, f]    float64
              (deriv_d = 1 for Linear)

The forward zeroes the levels with float(l) >= max_level L + 1e-3; the backward skips those with > (tcnn's two
comparisons); max_level may be given per sample.

Positions given as float64 select the ideal evaluation instead (setup, transform and sums in float64): a smooth
function of the position whose central differences the host test compares with the analytic gradient.
"""
import numpy as np

LINEAR, SMOOTHSTEP = 0, 1
F32, F64 = np.float32, np.float64


class Desc:
    """The level table of a grid, from the oracle's Grid (pyoracle.make_grid) or a model's ParamLayout."""

    def __init__(self, g):
        lay = hasattr(g, "grid_levels")
        self.D = int(g.grid_dims if lay else g.n_dims)
        self.L = int(g.grid_levels if lay else g.n_levels)
        self.F = int(g.grid_features if lay else g.n_features)
        self.offsets = [int(v) for v in (g.grid_level_offsets if lay else g.offsets)][: self.L + 1]
        self.scale = [F32(v) for v in (g.grid_scale if lay else g.scale)][: self.L]
        self.resolution = [int(v) for v in (g.grid_resolution if lay else g.resolution)][: self.L]

    @property
    def n_params(self):
        return self.offsets[self.L] * self.F


def fma32(a, b, c):
    """fp32 fused multiply-add of float32 arrays, one rounding. The product of two fp32 is exact in float64; the
    sum with c is formed with its exact error (TwoSum) and, where inexact, moved to the neighbouring double with an
    odd last bit (round to odd), so that the final rounding to fp32 sees on which side of every fp32 tie the exact
    value lies: no double rounding."""
    p = np.asarray(a, F32).astype(F64) * np.asarray(b, F32).astype(F64)
    c = np.asarray(c, F32).astype(F64)
    p, c = np.broadcast_arrays(p, c)
    s = p + c
    t = s - p
    e = (p - (s - t)) + (c - t)
    even = (s.view(np.int64) & 1) == 0
    fix = (e != 0) & even
    s = np.where(fix, np.nextafter(s, np.where(e > 0, np.inf, -np.inf)), s)
    return s.astype(F32)


def interp(frac, mode):
    """(frac, deriv) of the mode, in frac's own precision, the products left to right as written above."""
    one, two, three, six = (frac.dtype.type(v) for v in (1, 2, 3, 6))
    if mode == LINEAR:
        return frac, np.ones_like(frac)
    deriv = six * frac * (one - frac)
    return frac * frac * (three - two * frac), deriv


def level_setup(g, l, x, mode):
    """base (int64 [n, D], the kernel's uint32 before wrap-around), transformed frac and deriv [n, D]."""
    if x.dtype == F64:
        p = F64(g.scale[l]) * x[:, : g.D] + 0.5
    else:
        p = fma32(g.scale[l], x[:, : g.D], F32(0.5))
    t = np.floor(p)
    frac, deriv = interp(p - t, mode)
    return t.astype(np.int64), frac, deriv


def corner_index(g, l, base, c):
    """tcnn grid_index of corner c, uint32 arithmetic: dense while the stride fits, else the coherent prime hash."""
    primes = (1, 2654435761, 805459861)
    M = 0xFFFFFFFF
    T, res = g.offsets[l + 1] - g.offsets[l], g.resolution[l]
    pd = [(base[:, d] + ((c >> d) & 1)) & M for d in range(g.D)]
    stride, index = 1, np.zeros(base.shape[0], np.int64)
    for d in range(g.D):
        if stride > T:
            break
        index = (index + pd[d] * stride) & M
        stride = (stride * res) & M
    if T < stride:
        index = np.zeros(base.shape[0], np.int64)
        for d in range(g.D):
            index ^= (pd[d] * primes[d]) & M
    return g.offsets[l] + index % T


def corner_weight(g, frac, c, skip=None):
    w = np.ones(frac.shape[0], frac.dtype)
    for d in range(g.D):
        if d != skip:
            w = w * (frac[:, d] if (c >> d) & 1 else frac.dtype.type(1) - frac[:, d])
    return w


def _limit(g, n, max_level, per_sample):
    ml = np.full(n, max_level, F32) if per_sample is None else np.asarray(per_sample, F32)
    return ml * F32(g.L) + F32(1e-3)  # fp32, as the kernels form it


def forward(g, pos, table16, mode=LINEAR, max_level=1.0, max_level_per_sample=None):
    """fp16 bits [n, L F] of the encoding. table16: uint16 [entries F]."""
    g = g if isinstance(g, Desc) else Desc(g)
    x = np.ascontiguousarray(pos, F32)
    n = x.shape[0]
    tab = np.asarray(table16).view(np.float16).reshape(-1, g.F)  # widened after the gather: the table may be large
    lim = _limit(g, n, max_level, max_level_per_sample)
    out = np.zeros((n, g.L * g.F), np.uint16)
    for l in range(g.L):
        base, frac, _ = level_setup(g, l, x, mode)
        acc = np.zeros((n, g.F), F32)
        for c in range(1 << g.D):
            acc = fma32(corner_weight(g, frac, c)[:, None], tab[corner_index(g, l, base, c)].astype(F32), acc)
        acc[F32(l) >= lim] = 0
        out[:, l * g.F:(l + 1) * g.F] = acc.astype(np.float16).view(np.uint16)
    return out


def forward64(g, pos64, table16, mode=LINEAR):
    """The ideal encoding in float64 [n, L F] at float64 positions (no fp16 rounding of the result)."""
    g = g if isinstance(g, Desc) else Desc(g)
    x = np.ascontiguousarray(pos64, F64)
    tab = np.asarray(table16).view(np.float16).reshape(-1, g.F)
    out = np.zeros((x.shape[0], g.L * g.F), F64)
    for l in range(g.L):
        base, frac, _ = level_setup(g, l, x, mode)
        for c in range(1 << g.D):
            out[:, l * g.F:(l + 1) * g.F] += corner_weight(g, frac, c)[:, None] * tab[corner_index(g, l, base, c)].astype(F64)
    return out


def _exact_bincount(idx, q, size):
    """sum of the int64 values q per index, exactly: two float64 bincounts of 20-bit halves (each sum < 2^53)."""
    lo = q & 0xFFFFF
    hi = q >> 20
    s_lo = np.bincount(idx, lo.astype(F64), size).astype(np.int64)
    s_hi = np.bincount(idx, hi.astype(F64), size).astype(np.int64)
    return (s_hi << 20) + s_lo


def backward(g, pos, dL_dy16, mode=LINEAR, max_level=1.0, max_level_per_sample=None, grad16=None):
    """fp16 bits [entries F] of the exact parameter gradient. dL_dy16: uint16 [n, >= L F] (AoS). grad16: the initial
    gradient to accumulate onto (None: overwrite)."""
    g = g if isinstance(g, Desc) else Desc(g)
    x = np.ascontiguousarray(pos, F32)
    n = x.shape[0]
    dy = np.asarray(dL_dy16).view(np.float16).astype(F32)
    lim = _limit(g, n, max_level, max_level_per_sample)
    acc = np.zeros(g.n_params, np.int64)
    feat = np.arange(g.F, dtype=np.int64)
    for l in range(g.L):
        keep = ~(F32(l) > lim)
        if not keep.any():
            continue
        base, frac, _ = level_setup(g, l, x[keep], mode)
        gy = dy[keep, l * g.F:(l + 1) * g.F]
        for c in range(1 << g.D):
            w = corner_weight(g, frac, c)
            contrib = (w[:, None] * gy).astype(np.float16).astype(F64)  # fp32 product, RNE to fp16
            q = (contrib * 16777216.0).astype(np.int64)                  # exact: fp16 values are multiples of 2^-24
            idx = (corner_index(g, l, base, c) - g.offsets[l])[:, None] * g.F + feat
            acc[g.offsets[l] * g.F:g.offsets[l + 1] * g.F] += _exact_bincount(idx.ravel(), q.ravel(), (g.offsets[l + 1] - g.offsets[l]) * g.F)
    s = (acc.astype(F64) * (1.0 / 16777216.0)).astype(F32)
    if grad16 is not None:
        s = s + np.asarray(grad16).view(np.float16).astype(F32)
    return s.astype(np.float16).view(np.uint16)


def input_grad(g, pos, table16, dL_dy, mode=LINEAR, max_level=1.0, max_level_per_sample=None, with_cond=False):
    """dL/dposition, float64 [n, D]. dL_dy: float [n, >= L F]. float32 positions: the kernels' fp32 setup and
    transform, widened; float64 positions: the ideal evaluation. with_cond: also sum_l scale_l sum_c |prod w| |gs|,
    the magnitude of the summed terms before the factor deriv (the conditioning of the result)."""
    g = g if isinstance(g, Desc) else Desc(g)
    x = np.ascontiguousarray(pos, F64 if np.asarray(pos).dtype == F64 else F32)
    n = x.shape[0]
    tab = np.asarray(table16).view(np.float16).reshape(-1, g.F)
    dy = np.asarray(dL_dy, F64)
    lim = _limit(g, n, max_level, max_level_per_sample)
    out = np.zeros((n, g.D), F64)
    cond = np.zeros((n, g.D), F64)
    for l in range(g.L):
        active = ~(F32(l) >= lim)
        base, frac, deriv = level_setup(g, l, x, mode)
        frac, deriv = frac.astype(F64), deriv.astype(F64)
        for c in range(1 << g.D):
            tc = tab[corner_index(g, l, base, c)].astype(F64)
            gs = np.zeros(n, F64)
            for f in range(g.F):  # the oracle's order of operations throughout, so that Linear reproduces its bits
                gs += dy[:, l * g.F + f] * tc[:, f]
            for d in range(g.D):
                wo = corner_weight(g, frac, c, skip=d)
                t = F64(g.scale[l]) * deriv[:, d] * (wo if (c >> d) & 1 else -wo) * gs
                out[:, d] += np.where(active, t, 0.0)
                cond[:, d] += np.where(active, F64(g.scale[l]) * wo * np.abs(gs), 0.0)
    return (out, cond) if with_cond else out


# ---- shared test inputs -------------------------------------------------------------------------------------------
SHAPES = [(3, 4, 4, 15), (3, 16, 2, 15), (2, 4, 2, 14), (3, 8, 1, 12), (3, 4, 8, 10)]  # (D, L, F, log2 T)


def positions(g, n, seed):
    """n float32 positions [n, D]: uniform in the unit cube, then points on cell faces of several levels, points at
    0 and 1, and points slightly outside the cube (each kind about n / 16 rows)."""
    g = g if isinstance(g, Desc) else Desc(g)
    r = np.random.default_rng(seed)
    x = r.random((n, g.D)).astype(F32)
    k = max(n // 16, 1)
    for j in range(k):  # on a face of level l in one dimension: scale x + 0.5 is an integer up to rounding
        l = j % g.L
        d = j % g.D
        cell = r.integers(1, max(g.resolution[l] - 1, 2))
        x[j, d] = F32((cell - 0.5) / float(g.scale[l]))
    x[k:2 * k] = r.integers(0, 2, (k, g.D)).astype(F32)                       # corners of the cube
    x[2 * k:3 * k, 0] = r.integers(0, 2, k).astype(F32)                       # one coordinate at 0 or 1
    x[3 * k:4 * k] = r.uniform(-0.05, 1.05, (k, g.D)).astype(F32)             # slightly outside
    x[3 * k:3 * k + k // 2, 1] = r.choice([-0.03, 1.03], k // 2).astype(F32)
    return x


def face_pairs(g, n_pairs, seed, ulps=4):
    """(x_minus, x_plus, dim, level, max_level): float32 positions that differ in one coordinate only, `ulps` float32
    steps either side of a cell face of `level` in dimension `dim`, so that the fp32 level setup gives them different
    cells. Only levels with scale < 2^12 are used, where those few ulps are under 2^-9 of a cell, and max_level (per
    pair) switches off the levels finer than `level`, for which the same step is no small part of a cell."""
    g = g if isinstance(g, Desc) else Desc(g)
    r = np.random.default_rng(seed)
    levels = [l for l in range(g.L) if g.scale[l] < 4096]
    xm = r.uniform(0.1, 0.9, (n_pairs, g.D)).astype(F32)
    xp = xm.copy()
    dim = np.arange(n_pairs) % g.D
    lev = np.array([levels[(j // g.D) % len(levels)] for j in range(n_pairs)])
    for j in range(n_pairs):
        l, d = lev[j], dim[j]
        cell = r.integers(2, g.resolution[l] - 2)
        a = b = F32((cell - 0.5) / float(g.scale[l]))
        for _ in range(ulps):
            a = np.nextafter(a, F32(-1))
            b = np.nextafter(b, F32(2))
        xm[j, d], xp[j, d] = a, b
    return xm, xp, dim, lev, ((lev + 0.5) / g.L).astype(F32)
