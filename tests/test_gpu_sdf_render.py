"""The SDF sphere tracer (csrc/sdf_render.hip: SphereTracer + render_sdf, testbed_sdf.cu:47-434, 508-613, 629-1063) on
the GPU, on a 320-triangle bumped icosphere seen from outside its box at 96 x 64:

1. ground-truth depth against exact ray-mesh intersection (Moeller-Trumbore, float64);
2. finite-difference normals of the mesh's distance against the face normals;
3. the whole pipeline (trace, FD normals, shadow rays, evaluate_shading) against a float32 numpy restatement of the
   reference's arithmetic, uncompacted with an alive mask and one row per pixel (the tracer seeds the mesh's sign test
   with the ray's pixel, ngp_sdf_signed_distance_rows): positions and step counts bit for bit, colours to 1e-4;
4. the network path: the same restatement with the engine's inference as the distance, analytic normals;
5. frame semantics (determinism under compaction, spp averaging, inference parameters, odd frame sizes);
6. the IoU counters.
The library is built with -ffp-contract=off and the kernels keep the reference's operation order, which is what
makes the bit-for-bit comparisons possible."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

f32 = np.float32
W, H = 96, 64
XFORM = [1, 0, 0, 0, 1, 0, 0, 0, 1, 0.5, 0.5, -1.0]  # identity axes, origin outside the box
MAX_ITER = 512
FMAX = f32(3.402823466e+38)
MAX_DEPTH = f32(16384.0)


@pytest.fixture(scope="module")
def pkg():
    from __graft_entry__ import load_package
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return load_package()


class Scene:
    pass


@pytest.fixture(scope="module")
def scene(pkg):
    s = Scene()
    verts = pkg.synthetic.icosphere(2, bumps=0.15, seed=1)
    s.tris, s.amin, s.amax, s.brad = pkg.sdf.load_mesh(verts)
    assert s.tris.shape == (320, 9)
    s.mesh = pkg.sdf.SdfMesh(s.tris)
    s.renderer = pkg.sdf.SdfRenderer()
    s.cam = camera(pkg, W, H)
    return s


def camera(pkg, w, h):
    return pkg.nerf.make_image(w, h, XFORM, focal=(64.0, 64.0), principal=(0.5, 0.5))


def config(pkg, scene, **kw):
    return pkg.sdf.default_render_config(aabb_min=scene.amin, aabb_max=scene.amax, snap_to_pixel_centers=1, max_iterations=MAX_ITER, **kw)


# ---- the reference's arithmetic in numpy float32 -----------------------------------------------------------------
M32 = 0xFFFFFFFF


def _rev(x):
    return int("{:032b}".format(x)[::-1], 2)


def _laine_karras(x, seed):
    x = (x + seed) & M32
    for c in (0x6c50b47c, 0xb82f1e52, 0xc7afe638, 0x8d22f6e6):
        x ^= (x * c) & M32
    return x


def _nus(x, seed):
    return _rev(_laine_karras(_rev(x), seed))


def _hash_combine(seed, v):
    return (seed ^ ((v + ((seed << 6) & M32) + (seed >> 2)) & M32)) & M32


def _sobol(index, dim):
    X, v = 0, 0x80000000
    for bit in range(32):
        if dim == 0:
            X ^= ((index >> bit) & 1) * (0x80000000 >> bit)
        else:
            X ^= ((index >> bit) & 1) * v
            v ^= v >> 1
    return X


def _ld_val_2d(index, seed):
    S = f32(1.0 / 4294967296.0)
    index = _nus(index, seed)
    return tuple(f32(_nus(_sobol(index, d), _hash_combine(seed, d))) * S for d in (0, 1))


def pixel_offset(spp):
    """ld_random_pixel_offset (random_val.cuh:320-326)"""
    ax, ay = _ld_val_2d(0, 0xdeadbeef)
    bx, by = _ld_val_2d(spp, 0xdeadbeef)
    fx, fy = f32(0.5) - ax + bx, f32(0.5) - ay + by
    return fx - np.floor(fx), fy - np.floor(fy)


def dot(a, b):
    return a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1] + a[:, 2] * b[:, 2]


def normalize(v):
    inv = f32(1.0) / np.sqrt(dot(v, v))
    return v * inv[:, None]


def contains(lo, hi, p):
    return np.all((p >= lo) & (p <= hi), axis=1)


def ray_intersect(lo, hi, o, d):
    """BoundingBox::ray_intersect (bounding_box.cuh:163-216): tmin, FMAX where the ray misses"""
    with np.errstate(all="ignore"):
        tmin, tmax = (lo[0] - o[:, 0]) / d[:, 0], (hi[0] - o[:, 0]) / d[:, 0]
        sw = tmin > tmax
        tmin, tmax = np.where(sw, tmax, tmin), np.where(sw, tmin, tmax)
        miss = np.zeros(len(o), bool)
        for k in (1, 2):
            a, b = (lo[k] - o[:, k]) / d[:, k], (hi[k] - o[:, k]) / d[:, k]
            sw = a > b
            a, b = np.where(sw, b, a), np.where(sw, a, b)
            miss |= (tmin > b) | (a > tmax)
            tmin = np.where(a > tmin, a, tmin)
            tmax = np.where(b < tmax, b, tmax)
    return np.where(miss, FMAX, tmin).astype(f32)


def camera_rays(w, h):
    """init_rays_with_payload_kernel_sdf's pixel_to_ray for the fixture's camera, pixels snapped (sample 0)"""
    ox, oy = pixel_offset(0)
    i = np.arange(w * h, dtype=np.uint32)
    x, y = (i % w).astype(f32), (i // w).astype(f32)
    u, v = (x + ox) / f32(w), (y + oy) / f32(h)
    dx = (u - f32(0.5)) * f32(w) / f32(64.0)
    dy = (v - f32(0.5)) * f32(h) / f32(64.0)
    m = np.asarray(XFORM, f32)
    d = np.stack([m[0] * dx + m[3] * dy + m[6], m[1] * dx + m[4] * dy + m[7], m[2] * dx + m[5] * dy + m[8]], axis=1).astype(f32)
    o = (m[9:12][None, :] + d * f32(0.0)).astype(f32)
    return o, normalize(d)


class Trace:
    """SphereTracer::trace (:707-799) without compaction: every ray keeps its slot, `alive` masks the updates. Hits and
    finished shadow rays are taken where the reference compacts, so rays that end after the last compaction are left
    out exactly as there."""

    def __init__(self, cfg, distance):
        self.zero_offset, self.scale, self.maxd = f32(cfg.zero_offset), f32(cfg.distance_scale), f32(cfg.maximum_distance)
        self.k = f32(cfg.shadow_sharpness)
        self.lo = np.asarray(list(cfg.aabb_min), f32) - self.zero_offset
        self.hi = np.asarray(list(cfg.aabb_max), f32) + self.zero_offset
        self.floor_y = f32(cfg.aabb_min[1]) + f32(0.001) if cfg.floor_enable else f32(-10000.0)
        self.max_iter = cfg.max_iterations
        self.distance = distance

    def init_camera(self, o, d):
        tmin = ray_intersect(self.lo, self.hi, o, d)
        with np.errstate(all="ignore"):
            adv = np.fmax(tmin, f32(0.0)) + f32(1e-6)
            pos = np.where((tmin < FMAX)[:, None], o + adv[:, None] * d, o).astype(f32)
        return pos, (tmin < FMAX) & contains(self.lo, self.hi, pos)

    def run(self, pos, dirs, alive, shadow=False):
        n = len(pos)
        pos, alive = pos.copy(), alive.copy()
        steps = np.zeros(n, np.uint32)
        prev, total, min_vis = np.full(n, f32(1e20)), np.zeros(n, f32), np.ones(n, f32)
        retired, hit, factor = np.zeros(n, bool), np.zeros(n, bool), np.ones(n, f32)
        i = 1
        with np.errstate(all="ignore"):
            while i < self.max_iter:
                step_size = min(i, 4)
                new = ~alive & ~retired  # the compaction
                inside = contains(self.lo, self.hi, pos)
                hit |= new & inside
                factor = np.where(new, np.where(inside, f32(0.0), min_vis), factor)
                retired |= new
                if not alive.any():
                    break
                for _ in range(step_size):
                    dist = (self.distance(pos) - self.zero_offset) * self.scale
                    p = pos + dist[:, None] * dirs
                    fl = (p[:, 1] < self.floor_y) & (dirs[:, 1] < 0)
                    fd = np.where(fl, -(p[:, 1] - self.floor_y) / dirs[:, 1], f32(0.0)).astype(f32)
                    dist = np.where(fl, dist + fd, dist)
                    p = np.where(fl[:, None], p + fd[:, None] * dirs, p)
                    a = alive
                    pos = np.where(a[:, None], p, pos).astype(f32)
                    if shadow:
                        upd = a & (dist > 0)
                        yy = dist * dist / (f32(2.0) * prev)
                        dd = np.sqrt(dist * dist - yy * yy)
                        mv = np.fmin(min_vis, self.k * dd / np.fmax(f32(0.0), total - yy))
                        min_vis = np.where(upd, mv, min_vis)
                        prev = np.where(upd, dist, prev)
                        total = np.where(upd, total + dist, total)
                    stay = (dist > self.maxd) & (np.abs(dist / f32(2.0)) > f32(3.0) * self.maxd) & contains(self.lo, self.hi, p)
                    steps = steps + (a & stay).astype(np.uint32)
                    alive = a & stay & ~fl
                i += step_size
        self.pos, self.steps, self.hit, self.factor = pos, steps, hit, factor
        return self


def fd_normals(distance, pos, eps):
    """FiniteDifferenceNormalsApproximator::normal (:853-881)"""
    out = np.zeros_like(pos)
    for k in range(3):
        e = np.zeros(3, f32)
        e[k] = eps
        out[:, k] = distance((pos + e).astype(f32)) - distance((pos - e).astype(f32))
    return out


def shadow_factors(tr, cfg, pos, dirs, normals, sun1, hit):
    """prepare_shadow_rays + the shadow trace + write_shadow_ray_result (:233-296); one row per pixel, `hit` marks the
    rows that hold a camera hit"""
    ff = np.where((dot(normals, dirs) < 0)[:, None], normals, -normals)
    with np.errstate(all="ignore"):
        p = (pos + normalize(ff) * f32(1e-3)).astype(f32)
    sd = np.repeat(normalize(sun1[None, :]), len(pos), axis=0)
    tmin = ray_intersect(tr.lo, tr.hi, p, sd)
    with np.errstate(all="ignore"):
        adv = np.fmax(tmin + f32(1e-6), f32(0.0))
        p2 = (p + adv[:, None] * sd).astype(f32)
    alive = hit & (tmin < FMAX) & contains(tr.lo, tr.hi, p2)
    p2 = np.where(alive[:, None], p2, tr.hi + f32(1.0)).astype(f32)
    t = Trace(cfg, tr.distance).run(p2, sd, alive, shadow=True)
    return t.factor


def schlick(u):
    m = np.clip((1.0 - u.astype(np.float64)).astype(f32), f32(0), f32(1))
    return (m * m) * (m * m) * m


PI = f32(3.14159265358979323846)


def g1(ndh, a):
    a = f32(a)
    if a >= 1.0:
        return np.full_like(ndh, f32(1.0 / np.float64(PI)))
    a2 = a * a
    t = (1.0 + (np.float64(a2) - 1.0) * ndh.astype(np.float64) * ndh.astype(np.float64)).astype(f32)
    return ((np.float64(a2) - 1.0) / (PI * np.log(a2) * t).astype(np.float64)).astype(f32)


def smith(ndv, alpha):
    a = f32(alpha) * f32(alpha)
    b = ndv * ndv
    return (1.0 / (ndv + np.sqrt(a + b - a * b)).astype(np.float64)).astype(f32)


def mix(a, b, t):
    return a + (b - a) * t


def evaluate_shading(base, ambient, light, metallic, subsurface, specular, roughness, sheen, clearcoat, clearcoat_gloss, L, V, N):
    """evaluate_shading (:78-147); specular_tint = sheen_tint = 0 as shade_kernel_sdf passes them. Per-ray arrays:
    base [n,3], ambient [n,3], light [n,3], metallic .. clearcoat [n]; L [3]; V, N [n,3]."""
    Lb = np.broadcast_to(L, N.shape)
    ndl, ndv = dot(N, Lb), dot(N, V)
    Hv = normalize((Lb + V).astype(f32))
    ndh, ldh = dot(N, Hv), dot(Lb, Hv)
    FL, FV = schlick(ndl), schlick(ndv)
    amb = ambient * mix(f32(0.2), FV, metallic)[:, None]
    amb = amb * base
    lum = base[:, 0] * f32(0.3) + base[:, 1] * f32(0.6) + base[:, 2] * f32(0.1)
    ctint = base * (f32(1.0) / (lum + f32(0.00001)))[:, None]
    one = np.ones_like(base)
    c0 = mix(one, ctint, f32(0.0)) * specular[:, None] * f32(0.08)
    cspec0 = mix(c0, base, metallic[:, None])
    csheen = mix(one, ctint, f32(0.0))
    fd90 = f32(0.5) + f32(2.0) * ldh * ldh * roughness
    fd = mix(f32(1.0), fd90, FL) * mix(f32(1.0), fd90, FV)
    fss90 = ldh * ldh * roughness
    fss = mix(f32(1.0), fss90, FL) * mix(f32(1.0), fss90, FV)
    ss = f32(1.25) * (fss * (f32(1.0) / (ndl + ndv) - f32(0.5)) + f32(0.5))
    a = np.fmax(f32(0.001), roughness * roughness)
    # G2 and SmithG_GGX with a per-ray roughness: the floor's differs from the mesh's
    a2 = a * a
    t = (1.0 + (a2.astype(np.float64) - 1.0) * ndh.astype(np.float64) * ndh.astype(np.float64)).astype(f32)
    Ds = a2 / (PI * t * t)
    FH = schlick(ldh)
    Fs = mix(cspec0, one, FH[:, None])

    def smith_v(x, al):
        aa = al * al
        b = x * x
        return (1.0 / (x + np.sqrt(aa + b - aa * b)).astype(np.float64)).astype(f32)
    Gs = smith_v(ndl, a) * smith_v(ndv, a)
    fsheen = (FH * sheen)[:, None] * csheen
    Dr = g1(ndh, mix(f32(0.1), f32(0.001), f32(clearcoat_gloss)))
    Fr = mix(f32(0.04), f32(1.0), FH)
    Gr = smith(ndl, 0.25) * smith(ndv, 0.25)
    ccs = f32(0.25) * clearcoat * Gr * Fr * Dr
    diff = (f32(f32(1.0) / PI) * mix(fd, ss, subsurface))
    brdf = (diff[:, None] * base + fsheen) * (f32(1.0) - metallic)[:, None] + Gs[:, None] * Fs * Ds[:, None] + ccs[:, None]
    out = brdf * light * ndl[:, None] + amb
    back = (ndl < 0) | (ndv < 0)
    return np.where(back[:, None], amb, out).astype(f32)


def shade(cfg, pos, dirs, normals, factor):
    """shade_kernel_sdf's Shade branch (:317-361) for hits"""
    lo, hi = np.asarray(list(cfg.aabb_min), f32), np.asarray(list(cfg.aabb_max), f32)
    n = len(pos)
    floor_y = f32(cfg.aabb_min[1]) + f32(0.001) if cfg.floor_enable else f32(-10000.0)
    nrm = normalize(normals)
    floor = (pos[:, 1] < floor_y + f32(0.001)) & (dirs[:, 1] < 0)
    nrm = np.where(floor[:, None], np.asarray([0, 1, 0], f32), nrm).astype(f32)
    sun = np.asarray(list(cfg.sun_dir), f32)
    sun = sun * (f32(1.0) / np.sqrt(sun[0] * sun[0] + sun[1] * sun[1] + sun[2] * sun[2]))
    up = np.asarray(list(cfg.up_dir), f32)
    up = up * (f32(1.0) / np.sqrt(up[0] * up[0] + up[1] * up[1] + up[2] * up[2]))
    skyam = -(nrm[:, 0] * up[0] + nrm[:, 1] * up[1] + nrm[:, 2] * up[2]) * f32(0.5) + f32(0.5)
    suncol = (np.asarray([255.0 / 255.0, 225.0 / 255.0, 195.0 / 255.0], f32) * f32(4.0))[None, :] * factor[:, None]
    skycol = (np.asarray([195.0 / 255.0, 215.0 / 255.0, 255.0 / 255.0], f32) * f32(4.0))[None, :] * skyam[:, None]
    check_size = f32(8.0) / (hi[0] - lo[0])
    cx = np.floor(check_size * (pos[:, 0] - lo[0])).astype(np.int32)
    cz = np.floor(check_size * (pos[:, 2] - lo[2])).astype(np.int32)
    check = np.where((cx ^ cz) & 1, f32(0.8), f32(0.2)).astype(f32)
    floorcol = np.stack([check * check * check, check * check, check], axis=1)
    bc = np.asarray(list(cfg.basecolor), f32)
    base = np.where(floor[:, None], floorcol, (bc * bc)[None, :]).astype(f32)
    ambient = np.asarray(list(cfg.ambientcolor), f32)[None, :] * skycol

    def sel(floor_v, v):
        return np.where(floor, f32(floor_v), f32(v)).astype(f32)
    V = -normalize(dirs)
    return evaluate_shading(base, ambient, suncol, sel(0, cfg.metallic), sel(0, cfg.subsurface), sel(1, cfg.specular),
                            sel(0.5, cfg.roughness), sel(0, cfg.sheen), sel(0, cfg.clearcoat), cfg.clearcoat_gloss, sun, V, nrm), sun


def mesh_distance(scene):
    def fn(pos):
        return scene.mesh.signed_distance(torch.from_numpy(np.ascontiguousarray(pos, f32)).cuda()).cpu().numpy()
    return fn


def positions_colour(pos):
    return (pos - f32(0.5)) / f32(2.0) + f32(0.5)


def render(scene, cfg, mode, network=None, camera=None, **kw):
    """the network's distance, or the mesh's own when no network is given"""
    out = scene.renderer.render(network=network, ground_truth=None if network is not None else scene.mesh, cfg=cfg,
                                camera=camera if camera is not None else scene.cam, mode=mode, **kw)
    if isinstance(out, tuple):
        return tuple(o.cpu().numpy() for o in out)
    return out.cpu().numpy()


# ---- exact intersection (float64) ---------------------------------------------------------------------------------
def moller_trumbore(o, d, tris):
    """nearest hit of every ray: t (inf: none), triangle index, barycentrics (u, v, 1 - u - v), float64"""
    o, d, T = o.astype(np.float64), d.astype(np.float64), tris.reshape(-1, 3, 3).astype(np.float64)
    v0, e1, e2 = T[:, 0], T[:, 1] - T[:, 0], T[:, 2] - T[:, 0]
    p = np.cross(d[:, None, :], e2[None, :, :])
    det = np.einsum("tk,rtk->rt", e1, p)
    with np.errstate(all="ignore"):
        inv = 1.0 / det
        s = o[:, None, :] - v0[None, :, :]
        u = np.einsum("rtk,rtk->rt", s, p) * inv
        q = np.cross(s, e1[None, :, :])
        v = np.einsum("rk,rtk->rt", d, q) * inv
        t = np.einsum("tk,rtk->rt", e2, q) * inv
    ok = (np.abs(det) > 1e-14) & (u >= 0) & (v >= 0) & (u + v <= 1) & (t > 0)
    t = np.where(ok, t, np.inf)
    k = np.argmin(t, axis=1)
    r = np.arange(len(o))
    nrm = np.cross(e1, e2)
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    return t[r, k], k, np.stack([u[r, k], v[r, k], 1 - u[r, k] - v[r, k]], axis=1), nrm[k]


@pytest.fixture(scope="module")
def exact(scene):
    e = Scene()
    e.o, e.d = camera_rays(W, H)
    e.t, e.tri, e.bary, e.nrm = moller_trumbore(e.o, e.d, scene.mesh.triangles)
    e.hit = np.isfinite(e.t)
    e.cos = np.abs(np.einsum("rk,rk->r", e.d.astype(np.float64), e.nrm))
    h2 = np.pad(e.hit.reshape(H, W), 1, mode="edge")
    nb = sum(h2[1 + dy:1 + dy + H, 1 + dx:1 + dx + W].astype(int) for dy in (-1, 0, 1) for dx in (-1, 0, 1)).reshape(-1)
    e.excluded = ((nb != 0) & (nb != 9)) | (e.hit & (e.cos < 0.25))
    return e


# ---- 1, 2: the mesh's own distance ----------------------------------------------------------------------------------
def test_ground_truth_depth_matches_exact_intersection(pkg, scene, exact):
    cfg = config(pkg, scene)
    bg = (0.25, 0.5, 0.75, 0.125)
    rgba, depth = render(scene, cfg, "Depth", background=bg, return_depth=True)
    rgba, depth = rgba.reshape(-1, 4), depth.reshape(-1)
    share = exact.excluded.mean()
    print(f"excluded share {share:.4f}, hit share {exact.hit.mean():.4f}")
    assert share <= 0.08
    keep = ~exact.excluded
    got_hit = rgba[:, 3] == 1.0
    assert np.array_equal(got_hit[keep], exact.hit[keep])
    miss = ~got_hit
    assert np.array_equal(rgba[miss], np.broadcast_to(np.asarray(bg, f32), (miss.sum(), 4)))
    assert np.all(depth[miss] == MAX_DEPTH)
    m = keep & exact.hit
    depth_exact = exact.t[m] * exact.d[m, 2].astype(np.float64)  # dot(camera forward = +z, pos - origin)
    diff = depth_exact - depth[m].astype(np.float64)
    bound = (3 * float(cfg.maximum_distance) * 2 / float(cfg.distance_scale)) / exact.cos[m] + 1e-5
    print(f"depth_exact - depth: min {diff.min():.3e} max {diff.max():.3e}, max of diff / bound {np.max(diff / bound):.3f}")
    assert np.all(diff >= 0) and np.all(diff <= bound)
    assert np.array_equal(rgba[m, 0], depth[m]) and np.array_equal(rgba[m, 1], depth[m])  # Depth mode's colour


def test_ground_truth_normals_match_the_faces(pkg, scene, exact):
    cfg = config(pkg, scene)
    rgba = render(scene, cfg, "Normals").reshape(-1, 4)
    m = ~exact.excluded & exact.hit & np.all(exact.bary >= 0.1, axis=1)
    assert m.sum() > 300
    want = 0.5 * exact.nrm[m] + 0.5
    per = np.abs(rgba[m, :3] - want).max(axis=1)
    err = per.max()
    print(f"normals: {m.sum()} pixels, max error {err:.3e}, {int((per > 1e-2).sum())} above 1e-2")
    for k in np.flatnonzero(per > 1e-2)[:5]:
        px = np.flatnonzero(m)[k]
        print(f"  pixel {px}: got {rgba[px, :3]}, want {want[k]}, bary {exact.bary[px]}, cos {exact.cos[px]:.3f}, alpha {rgba[px, 3]}")
    assert err <= 1e-2


def test_seeded_mesh_distance_follows_the_point(pkg, scene):
    """ngp_sdf_signed_distance_rows: a point keeps its distance, sign included, wherever it stands in the batch, when
    its seed goes with it; rows = 0..n-1 is the plain call. Points 2e-4 inside the surface, where the finite-difference
    taps land and where a stab ray slipping between two triangles flips the sign of about one point in a million."""
    g = np.random.default_rng(5)
    T = scene.mesh.triangles.reshape(-1, 3, 3)
    k = g.integers(0, len(T), 1 << 16)
    w = g.dirichlet(np.ones(3), len(k)).astype(f32)
    nrm = np.cross(T[:, 1] - T[:, 0], T[:, 2] - T[:, 0])
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    pts = (np.einsum("nk,nkd->nd", w, T[k]) - f32(2e-4) * nrm[k]).astype(f32)
    x = torch.from_numpy(pts).cuda()
    rows = torch.arange(len(pts), dtype=torch.int32, device="cuda")
    base = scene.mesh.signed_distance(x)
    assert torch.equal(scene.mesh.signed_distance(x, rows=rows), base)
    assert (base < 0).float().mean() > 0.9
    for _ in range(4):
        perm = torch.from_numpy(g.permutation(len(pts))).cuda()
        got = scene.mesh.signed_distance(x[perm].contiguous(), rows=rows[perm].contiguous())
        assert torch.equal(got, base[perm])


# ---- 3: the float32 restatement ---------------------------------------------------------------------------------------
def restate(cfg, distance, w=W, h=H, shade_too=True):
    o, d = camera_rays(w, h)
    tr = Trace(cfg, distance)
    pos0, alive0 = tr.init_camera(o, d)
    tr.run(pos0, d, alive0)
    r = Scene()
    r.hit, r.pos, r.steps, r.dirs = tr.hit, tr.pos, tr.steps, d
    if shade_too:
        # one row per pixel in every distance evaluation: the tracer seeds the mesh's sign test with the ray's pixel
        # (ngp_sdf_signed_distance_rows), and a plain signed_distance call seeds it with the row
        full = np.where(tr.hit[:, None], tr.pos, f32(0.5)).astype(f32)
        normals = fd_normals(distance, full, f32(cfg.fd_normals_epsilon))
        sun = np.asarray(list(cfg.sun_dir), f32)
        sun1 = sun * (f32(1.0) / np.sqrt(sun[0] * sun[0] + sun[1] * sun[1] + sun[2] * sun[2]))
        factor = shadow_factors(tr, cfg, full, d, normals, sun1, tr.hit)
        r.normals, r.factor = normals[tr.hit], factor[tr.hit]
        r.colour, _ = shade(cfg, tr.pos[tr.hit], d[tr.hit], r.normals, r.factor)
    return r


def check_positions_and_steps(scene, cfg, r, camera_=None, **kw):
    inside = contains(np.asarray(list(cfg.aabb_min), f32), np.asarray(list(cfg.aabb_max), f32), r.pos)
    shaded = r.hit & inside  # shade_kernel_sdf tests m_aabb again
    cam = camera_ if camera_ is not None else scene.cam
    p = render(scene, cfg, "Positions", camera=cam, **kw).reshape(-1, 4)
    c = render(scene, cfg, "Cost", camera=cam, **kw).reshape(-1, 4)
    assert np.array_equal(p[:, 3] == 1.0, shaded)
    assert shaded.sum() > 0.1 * len(shaded)
    assert np.array_equal(p[shaded, :3], positions_colour(r.pos[shaded]))
    assert np.array_equal(c[shaded, 0], r.steps[shaded].astype(f32) / f32(30))
    assert np.all(p[~shaded] == 0) and np.all(c[~shaded] == 0)
    return shaded


@pytest.mark.parametrize("floor", [0, 1])
def test_shade_pipeline_matches_the_float32_restatement(pkg, scene, floor):
    cfg = config(pkg, scene, floor_enable=floor)
    r = restate(cfg, mesh_distance(scene))
    shaded = check_positions_and_steps(scene, cfg, r)
    img = render(scene, cfg, "Shade").reshape(-1, 4)
    sel = shaded[r.hit]
    got, want = img[shaded, :3], r.colour[sel]
    assert np.isfinite(want).all()
    err = np.abs(got - want) / np.maximum(1.0, np.abs(want))
    print(f"floor {floor}: {shaded.sum()} shaded pixels, max colour error {err.max():.3e}, shadowed share {(r.factor[sel] < 0.5).mean():.3f}")
    assert err.max() <= 1e-4
    if floor:
        fl = (r.pos[shaded, 1] < f32(cfg.aabb_min[1]) + f32(0.001) + f32(0.001)) & (r.dirs[shaded, 1] < 0)
        assert fl.sum() > 50  # the floor is in view
    assert (r.factor[sel] < 0.5).sum() > 20 and (r.factor[sel] == 1.0).sum() > 20  # lit and shadowed pixels both


# ---- 4, 5: the network --------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def trained(pkg, scene):
    import copy
    c = copy.deepcopy(pkg.SDF_BASE)
    c["encoding"]["log2_hashmap_size"] = 14
    net = pkg.NetworkWithInputEncoding(3, 1, c["encoding"], c["network"])
    tr = pkg.Trainer(net, c["optimizer"], seed=1337)
    st = pkg.sdf.SdfTraining(net, tr, scene.mesh, scene.amin, scene.amax, scene.brad, batch_size=1 << 14)
    for _ in range(300):
        st.train_step(get_loss=False)
    torch.cuda.synchronize()
    t = Scene()
    t.net, t.trainer = net, tr
    return t


def network_distance(net, use_inference_params=True):
    def fn(pos):
        n = len(pos)
        x = np.full(((n + 255) // 256 * 256, 3), 0.5, f32)
        x[:n] = pos
        out = net.inference(torch.from_numpy(x).cuda(), layout=1, use_inference_params=use_inference_params)
        return out[0, :n].float().cpu().numpy()
    return fn


def test_network_path_matches_the_restatement(pkg, scene, trained):
    net = trained.net
    # precondition: a position's inference output does not depend on its row
    g = np.random.default_rng(3)
    x = (np.asarray(scene.amin) + g.random((4096, 3)) * (np.asarray(scene.amax) - np.asarray(scene.amin))).astype(f32)
    perm = g.permutation(len(x))
    fn = network_distance(net)
    a, b = fn(x), fn(x[perm])
    assert np.array_equal(a[perm].view(np.uint32), b.view(np.uint32)), "inference depends on the row order"
    cfg = config(pkg, scene)
    r = restate(cfg, fn, shade_too=False)
    shaded = check_positions_and_steps(scene, cfg, r, network=net)
    # analytic normals: Network::input_gradient(dim 0) on the hit positions
    cfg_a = config(pkg, scene, analytic_normals=1)
    img = render(scene, cfg_a, "Normals", network=net).reshape(-1, 4)
    hp = np.ascontiguousarray(r.pos[shaded])
    grad = net.input_gradient(0, torch.from_numpy(hp).cuda()).cpu().numpy()[:, :3]
    assert np.array_equal(img[shaded, :3], (f32(0.5) * normalize(grad) + f32(0.5)).astype(f32))
    # and a frame whose pixel count is no multiple of 64
    cam2 = camera(pkg, 50, 30)
    r2 = restate(cfg, fn, 50, 30, shade_too=False)
    check_positions_and_steps(scene, cfg, r2, camera_=cam2, network=net)


def test_frame_semantics(pkg, scene, trained):
    net = trained.net
    cfg = config(pkg, scene)
    kw = dict(network=net)
    a = render(scene, cfg, "Shade", **kw)
    b = render(scene, cfg, "Shade", **kw)
    assert np.array_equal(a, b)  # compaction order does not leak
    assert np.array_equal(render(scene, cfg, "Shade"), render(scene, cfg, "Shade"))
    # spp: the mean of the sample_index renders (pixels jittered)
    cfg_j = pkg.sdf.default_render_config(aabb_min=scene.amin, aabb_max=scene.amax, snap_to_pixel_centers=0, max_iterations=MAX_ITER)
    bg = (0.1, 0.2, 0.3, 0.4)
    four = render(scene, cfg_j, "Shade", spp=4, sample_index=3, background=bg)
    singles = [render(scene, cfg_j, "Shade", spp=1, sample_index=3 + k, background=bg) for k in range(4)]
    assert not np.array_equal(singles[0], singles[1])
    assert np.abs(four - np.mean(singles, axis=0)).max() <= 1e-6
    # the inference (EMA) parameters differ from the training ones after training
    p0 = render(scene, cfg, "Positions", use_inference_params=False, **kw)
    p1 = render(scene, cfg, "Positions", use_inference_params=True, **kw)
    assert not np.array_equal(p0, p1)
    # 50 x 30 with the mesh's distance, against the restatement
    cam2 = camera(pkg, 50, 30)
    r2 = restate(cfg, mesh_distance(scene), 50, 30, shade_too=False)
    check_positions_and_steps(scene, cfg, r2, camera_=cam2)


# ---- 6: IoU ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [65, 1000])
def test_iou_counters(pkg, n):
    g = np.random.default_rng(n)
    ref, model = g.standard_normal(n).astype(f32), g.standard_normal(n).astype(f32)
    ref[::7] = 0.0
    model[::5] = 0.0
    model[3] = -0.0

    def count(r, m):
        i1, i2 = r <= 0, m <= 0
        return np.asarray([i1.sum(), (~i1).sum(), i2.sum(), (~i2).sum(), (i1 & i2).sum(), (i1 | i2).sum(), 0, len(r)], np.int64)
    counters = pkg.sdf.iou_accumulate(torch.from_numpy(ref).cuda(), torch.from_numpy(model).cuda())
    c1 = count(ref, model)
    assert np.array_equal(counters.cpu().numpy().astype(np.int64), c1)
    ref2, model2 = g.standard_normal(n).astype(f32), g.standard_normal(n).astype(f32)
    pkg.sdf.iou_accumulate(torch.from_numpy(ref2).cuda(), torch.from_numpy(model2).cuda(), counters, scale_existing=0.5)
    scaled = np.floor(c1.astype(f32) * f32(0.5) + f32(0.5)).astype(np.int64)  # roundf: halves away from zero
    assert np.array_equal(counters.cpu().numpy().astype(np.int64), scaled + count(ref2, model2))


def test_iou_of_a_trained_network(pkg, scene, trained):
    rng = pkg.nerf.pcg32(7)
    before = rng.state
    v = pkg.sdf.iou(scene.mesh, trained.net, 1 << 16, rng, scene.amin, scene.amax)
    print(f"IoU after 300 steps: {v:.4f}")
    assert 0.0 < v <= 1.0 and rng.state != before
