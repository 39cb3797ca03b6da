"""Mesh extraction on the GPU (csrc/marching_cubes.hip): marching cubes against a numpy restatement that reads the
engine's own case table, vertex normals, the model sampled on a grid, and the two pyngp calls.

The engine's vertex and triangle order is a function of the grid (block by block), the reference's is point by point,
so meshes are compared as sets: vertices by their bytes, triangles as rotation-normalised triples of vertex keys
(axis, x, y, z of the grid edge the vertex lies on)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
f32 = np.float32

CORNERS = [(0, 0, 0), (1, 0, 0), (1, 1, 0), (0, 1, 0), (0, 0, 1), (1, 0, 1), (1, 1, 1), (0, 1, 1)]
EDGES = [(0, 1), (1, 2), (2, 3), (3, 0), (4, 5), (5, 6), (6, 7), (7, 4), (0, 4), (1, 5), (2, 6), (3, 7)]
UNIT = (np.zeros(3, f32), np.ones(3, f32))


@pytest.fixture(scope="module")
def pkg():
    from __graft_entry__ import load_package
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return load_package()


@pytest.fixture(scope="module")
def cases(pkg):
    tri, _ = pkg.mesh.mc_tables()
    out = []
    for row in tri:
        row = [int(v) for v in row]
        n = row.index(-1)
        out.append([tuple(row[k:k + 3]) for k in range(0, n, 3)])
    return out


# ---- the numpy reference -----------------------------------------------------------------------------------------
def cube_cases(f, thresh):
    rz, ry, rx = f.shape
    inside = f > f32(thresh)
    c = np.zeros((rz - 1, ry - 1, rx - 1), np.int32)
    for i, (dx, dy, dz) in enumerate(CORNERS):
        c |= inside[dz:rz - 1 + dz, dy:ry - 1 + dy, dx:rx - 1 + dx].astype(np.int32) << i
    return c


def reference_mesh(f, aabb, thresh, cases):
    """({vertex key: float32 position}, [triangle = 3 vertex keys]) of the float32 field f [rz, ry, rx]."""
    lo, hi = np.asarray(aabb[0], f32), np.asarray(aabb[1], f32)
    rz, ry, rx = f.shape
    scale = (hi - lo) / (np.asarray([rx, ry, rz]) - 1).astype(f32)
    assert scale.dtype == f32
    verts = {}
    for axis in range(3):
        na = 2 - axis  # the numpy axis of x / y / z
        a0 = np.take(f, np.arange(0, f.shape[na] - 1), axis=na)
        a1 = np.take(f, np.arange(1, f.shape[na]), axis=na)
        cross = (a0 > f32(thresh)) != (a1 > f32(thresh))
        zz, yy, xx = np.nonzero(cross)
        f0, f1 = a0[cross], a1[cross]
        dt = (f32(thresh) - f0) / (f1 - f0)
        coord = np.stack([xx, yy, zz], 1).astype(f32)
        coord[:, axis] = coord[:, axis] + dt
        pos = coord * scale + lo
        assert pos.dtype == f32
        for k in range(len(xx)):
            verts[(axis, int(xx[k]), int(yy[k]), int(zz[k]))] = pos[k]
    c = cube_cases(f, thresh)
    tris = []
    for z, y, x in zip(*np.nonzero((c != 0) & (c != 255))):
        for t in cases[c[z, y, x]]:
            tri = []
            for e in t:
                a, b = CORNERS[EDGES[e][0]], CORNERS[EDGES[e][1]]
                axis = next(k for k in range(3) if a[k] != b[k])
                p = (min(a[0], b[0]) + x, min(a[1], b[1]) + y, min(a[2], b[2]) + z)
                tri.append((axis, int(p[0]), int(p[1]), int(p[2])))
            tris.append(tuple(tri))
    return verts, tris


def rot_norm(t):
    k = t.index(min(t))
    return t[k:] + t[:k]


def compare_with_reference(V, F, ref):
    """V equals the reference's vertices byte for byte as a set; F through that map equals its triangle set."""
    verts, tris = ref
    by_bytes = {p.tobytes(): key for key, p in verts.items()}
    assert len(by_bytes) == len(verts), "the reference's vertex positions are not distinct"
    assert V.shape == (len(verts), 3) and F.shape == (len(tris), 3)
    keys = []
    for row in V:
        assert row.tobytes() in by_bytes, "a vertex that the reference does not have"
        keys.append(by_bytes[row.tobytes()])
    assert len(set(keys)) == len(keys)
    got = sorted(rot_norm(tuple(keys[i] for i in t)) for t in F)
    want = sorted(rot_norm(t) for t in tris)
    assert got == want
    return keys


def directed_edges(F):
    e = np.concatenate([F[:, [0, 1]], F[:, [1, 2]], F[:, [2, 0]]]).astype(np.int64)
    return e


def open_edges(F, n_verts):
    """directed edges without their reverse; asserts that no directed edge occurs twice"""
    e = directed_edges(F)
    code = e[:, 0] * n_verts + e[:, 1]
    assert len(np.unique(code)) == len(code), "a directed edge occurs twice"
    rev = e[:, 1] * n_verts + e[:, 0]
    return e[~np.isin(code, rev)]


def euler(V, F):
    e = np.sort(directed_edges(F), axis=1)
    return len(V) - len(np.unique(e, axis=0)) + len(F)


def volume(V, F):
    p = V.astype(np.float64)
    a, b, c = p[F[:, 0]], p[F[:, 1]], p[F[:, 2]]
    return float(np.einsum("ij,ij->i", a, np.cross(b, c)).sum() / 6.0)


def grid_points(res, aabb=UNIT):
    """float32 grid positions [rz, ry, rx, 3], built as the engine builds them"""
    lo, hi = np.asarray(aabb[0], f32), np.asarray(aabb[1], f32)
    scale = (hi - lo) / (np.asarray(res) - 1).astype(f32)
    z, y, x = np.meshgrid(*(np.arange(r, dtype=f32) for r in res[::-1]), indexing="ij")
    return lo + np.stack([x, y, z], -1) * scale


def run_mc(pkg, f, aabb, thresh, rot=None):
    rz, ry, rx = f.shape
    d = torch.from_numpy(np.ascontiguousarray(f, f32)).cuda()
    return pkg.mesh.marching_cubes(d, (rx, ry, rz), aabb, thresh, rot)


def sphere_field(res=(48, 48, 48)):
    p = grid_points(res).astype(np.float64) - 0.5
    return (0.3 - np.linalg.norm(p, axis=-1)).astype(f32)


def torus_field(res=(48, 48, 48)):
    p = grid_points(res).astype(np.float64) - 0.5
    return (0.1 - np.sqrt((np.sqrt(p[..., 0] ** 2 + p[..., 1] ** 2) - 0.28) ** 2 + p[..., 2] ** 2)).astype(f32)


@pytest.fixture(scope="module")
def shapes(pkg, cases):
    """name -> (field, engine (V, N, F), reference, analytic volume), computed once"""
    out = {}
    for name, f, vol in (("sphere", sphere_field(), 4 / 3 * np.pi * 0.3 ** 3), ("torus", torus_field(), 2 * np.pi ** 2 * 0.28 * 0.1 ** 2)):
        out[name] = (f, run_mc(pkg, f, UNIT, 0.0), reference_mesh(f, UNIT, 0.0, cases), vol)
    return out


# ---- 1: exact match ------------------------------------------------------------------------------------------------
def test_exact_match_on_a_smooth_field(pkg, cases):
    res = (20, 17, 13)
    aabb = (np.asarray([-0.3, 0.1, 0.2], f32), np.asarray([0.9, 0.7, 1.4], f32))
    p = grid_points(res, aabb).astype(np.float64)
    f = (np.sin(5 * p[..., 0]) * np.cos(4 * p[..., 1]) + np.sin(3 * p[..., 2] + 0.5) + 0.3 * p[..., 0] * p[..., 1]).astype(f32)
    thresh = 0.25
    V, N, F = run_mc(pkg, f, aabb, thresh)
    assert V.dtype == f32 and N.dtype == f32 and F.dtype == np.int32
    assert len(V) > 300 and len(F) > 300
    compare_with_reference(V, F, reference_mesh(f, aabb, thresh, cases))
    # a rotation: the same vertices and triangles in the same order, positions through transpose(aabb_to_local)
    a, b = 0.4, -0.7
    rx = np.asarray([[1, 0, 0], [0, np.cos(a), -np.sin(a)], [0, np.sin(a), np.cos(a)]])
    rz = np.asarray([[np.cos(b), -np.sin(b), 0], [np.sin(b), np.cos(b), 0], [0, 0, 1]])
    R = (rx @ rz).astype(f32)
    Vr, Nr, Fr = run_mc(pkg, f, aabb, thresh, R)
    assert np.array_equal(Fr, F)
    want = V.astype(np.float64) @ R.astype(np.float64)  # transpose(R) v as a row vector times R
    err = np.abs(Vr - want).max()
    print(f"rotated vertices: max |err| {err:.3e}")
    assert err <= 1e-6


# ---- 2: all cases --------------------------------------------------------------------------------------------------
def test_all_cases_on_a_random_field(pkg, cases):
    R = 24
    f = np.zeros((R, R, R), f32)
    f[1:-1, 1:-1, 1:-1] = np.random.default_rng(0).random((R - 2, R - 2, R - 2)).astype(f32)
    assert len(np.unique(cube_cases(f, 0.5))) == 256, "the field does not cover all 256 cases"
    V, N, F = run_mc(pkg, f, UNIT, 0.5)
    assert len(open_edges(F, len(V))) == 0  # every directed edge once, its reverse once
    compare_with_reference(V, F, reference_mesh(f, UNIT, 0.5, cases))


# ---- 3: shapes -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,chi,tol", [("sphere", 2, 0.01), ("torus", 0, 0.02)])
def test_shapes_are_closed_with_the_right_topology_and_volume(shapes, name, chi, tol):
    f, (V, N, F), (rverts, rtris), analytic = shapes[name]
    assert len(open_edges(F, len(V))) == 0
    assert euler(V, F) == chi
    vol = volume(V, F)
    keys = list(rverts)
    index = {k: i for i, k in enumerate(keys)}
    rV = np.stack([rverts[k] for k in keys])
    rF = np.asarray([[index[k] for k in t] for t in rtris])
    ref_vol = volume(rV, rF)
    print(f"{name}: volume {vol:.6f}, analytic {analytic:.6f} ({(vol / analytic - 1) * 100:+.2f} %), reference {ref_vol:.6f}")
    assert vol > 0
    assert abs(vol - analytic) <= tol * analytic
    assert abs(vol - ref_vol) <= 1e-5 * ref_vol


# ---- 4: more than one scan chunk, counts, determinism ------------------------------------------------------------------
def test_gyroid_counts_and_determinism(pkg, cases):
    res = (70, 66, 34)  # 9 x 9 x 9 = 729 blocks: more than one chunk of the block-count scan
    aabb = (np.zeros(3, f32), np.asarray([1.0, 0.9, 0.5], f32))
    p = grid_points(res, aabb).astype(np.float64) * 14.0 + 0.3  # no grid point on the surface itself
    f = (np.sin(p[..., 0]) * np.cos(p[..., 1]) + np.sin(p[..., 1]) * np.cos(p[..., 2]) + np.sin(p[..., 2]) * np.cos(p[..., 0])).astype(f32)
    V, N, F = run_mc(pkg, f, aabb, 0.0)
    inside = f > 0
    n_verts = sum(int((np.take(inside, np.arange(0, inside.shape[a] - 1), axis=a) !=
                       np.take(inside, np.arange(1, inside.shape[a]), axis=a)).sum()) for a in range(3))
    n_tris = int(np.asarray([len(t) for t in cases])[cube_cases(f, 0.0)].sum())
    assert n_verts > 10000
    assert (len(V), len(F)) == (n_verts, n_tris)
    assert F.min() == 0 and F.max() == n_verts - 1 and len(np.unique(F)) == n_verts
    # open edges only in the boundary layer: both ends on one face of the box
    lo, hi = aabb
    top = (np.asarray(res) - 1).astype(f32) * ((hi - lo) / (np.asarray(res) - 1).astype(f32)) + lo
    for a, b in open_edges(F, len(V)):
        assert any((V[a, k] == lo[k] and V[b, k] == lo[k]) or (V[a, k] == top[k] and V[b, k] == top[k]) for k in range(3))
    V2, N2, F2 = run_mc(pkg, f, aabb, 0.0)
    assert V.tobytes() == V2.tobytes() and N.tobytes() == N2.tobytes() and F.tobytes() == F2.tobytes()
    assert np.isfinite(N).all() and (np.linalg.norm(N, axis=1) > 0).all()


# ---- 5: the edges of the domain ----------------------------------------------------------------------------------------
def test_empty_fields(pkg):
    for value in (-1.0, 1.0):
        V, N, F = run_mc(pkg, np.full((9, 10, 11), value, f32), UNIT, 0.0)
        assert V.shape == (0, 3) and N.shape == (0, 3) and F.shape == (0, 3)
        assert V.dtype == f32 and F.dtype == np.int32


def test_small_and_flat_grids(pkg, cases):
    one = np.zeros((2, 2, 2), f32)
    one[0, 0, 0] = 1.0
    V, N, F = run_mc(pkg, one, UNIT, 0.5)
    assert V.shape == (3, 3) and F.shape == (1, 3)
    compare_with_reference(V, F, reference_mesh(one, UNIT, 0.5, cases))
    n = np.cross(V[F[0, 1]] - V[F[0, 0]], V[F[0, 2]] - V[F[0, 0]])
    assert (n > 0).all()  # away from the inside corner at the origin
    np.testing.assert_allclose(N, np.tile(n, (3, 1)), rtol=1e-6)

    res = (33, 2, 5)
    g = np.random.default_rng(3).random((res[2], res[1], res[0])).astype(f32)
    V, N, F = run_mc(pkg, g, UNIT, 0.5)
    compare_with_reference(V, F, reference_mesh(g, UNIT, 0.5, cases))

    # a plane cut by the boundary: open edges occur once, and only on the box
    res = (19, 21, 10)
    p = grid_points(res).astype(np.float64)
    plane = (p[..., 0] * 0.7 + p[..., 1] * 0.5 + p[..., 2] * 0.3 - 0.71).astype(f32)
    V, N, F = run_mc(pkg, plane, UNIT, 0.0)
    compare_with_reference(V, F, reference_mesh(plane, UNIT, 0.0, cases))
    border = open_edges(F, len(V))
    assert len(border) > 10
    for a, b in border:
        assert any((V[a, k] == 0.0 and V[b, k] == 0.0) or (V[a, k] == 1.0 and V[b, k] == 1.0) for k in range(3))
    assert euler(V, F) == 1  # a disc
    nn = N / np.linalg.norm(N, axis=1, keepdims=True)
    want = -np.asarray([0.7, 0.5, 0.3]) / np.linalg.norm([0.7, 0.5, 0.3])  # towards f <= 0
    assert np.abs(nn - want).max() < 1e-4


# ---- 6: normals --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["sphere", "torus"])
def test_normals_are_the_area_weighted_sums(shapes, name):
    f, (V, N, F), _, _ = shapes[name]
    p = V.astype(np.float64)
    fn = np.cross(p[F[:, 1]] - p[F[:, 0]], p[F[:, 2]] - p[F[:, 0]])
    want = np.zeros_like(p)
    for k in range(3):
        np.add.at(want, F[:, k], fn)
    want /= np.linalg.norm(want, axis=1, keepdims=True)
    got = N.astype(np.float64) / np.linalg.norm(N.astype(np.float64), axis=1, keepdims=True)
    err = np.abs(got - want).max()
    print(f"{name}: normals max |err| {err:.3e}")
    assert err <= 1e-5
    if name == "sphere":
        assert (np.einsum("ij,ij->i", N, V - f32(0.5)) > 0).all()


# ---- 7: sampling -------------------------------------------------------------------------------------------------------
def test_sampling_a_three_input_network(pkg):
    cfg = pkg.SDF_BASE
    enc = {**cfg["encoding"], "log2_hashmap_size": 12}
    net = pkg.NetworkWithInputEncoding(3, 1, enc, cfg["network"])
    tr = pkg.Trainer(net, cfg["optimizer"], seed=7)
    g = torch.Generator(device="cpu").manual_seed(0)
    x = torch.rand((1024, 3), generator=g).cuda()
    tr.learning_rate = 1e-2
    for _ in range(8):  # the EMA (inference) parameters leave the training parameters
        tr.training_step(x, (x[:, :1] - 0.5).contiguous(), loss="L2", get_loss=False)
    res = (9, 8, 7)
    aabb = (np.asarray([0.1, 0.2, 0.05], f32), np.asarray([0.9, 0.85, 0.95], f32))
    pos = torch.from_numpy(grid_points(res, aabb).reshape(-1, 3)).cuda()
    n = pos.shape[0]
    padded = torch.cat([pos, pos[-1:].expand(512 - n, 3)]).contiguous()
    grids = {}
    for inf in (True, False):
        want = net.inference(padded, use_inference_params=inf)[:n, 0].float().cpu().numpy()
        raw = pkg.mesh.density_on_grid(net, "raw", res, aabb, use_inference_params=inf)
        assert raw.shape == (7, 8, 9) and raw.dtype == torch.float32
        raw = raw.cpu().numpy().reshape(-1)
        assert raw.tobytes() == want.tobytes()
        sdf = pkg.mesh.density_on_grid(net, "sdf", res, aabb, use_inference_params=inf).cpu().numpy().reshape(-1)
        assert sdf.tobytes() == (-want).tobytes()
        ragged = pkg.mesh.density_on_grid(net, "raw", res, aabb, use_inference_params=inf, batch=128).cpu().numpy().reshape(-1)
        assert ragged.tobytes() == raw.tobytes()
        grids[inf] = raw
    assert not np.array_equal(grids[True], grids[False])
    with pytest.raises(pkg.NgpError):
        pkg.mesh.density_on_grid(net, "nerf", res, aabb)


def test_sampling_a_nerf_network(pkg):
    ncfg = pkg.nerf_config("C2")
    ncfg["encoding"]["log2_hashmap_size"] = 14
    net = pkg.create_nerf_network(ncfg)
    tr = pkg.Trainer(net, ncfg["optimizer"], seed=11)  # noqa: F841 (owns the parameters)
    res = (9, 8, 7)
    aabb = (np.asarray([-0.5, 0.0, 0.25], f32), np.asarray([1.5, 1.0, 0.75], f32))
    warp = (np.asarray([-0.5, -0.5, -0.5], f32), np.asarray([1.5, 1.5, 1.5], f32))
    p = grid_points(res, aabb).reshape(-1, 3)
    n = p.shape[0]
    coords = np.zeros((512, 7), f32)
    coords[:n, :3] = (p - warp[0]) / (warp[1] - warp[0])
    coords[n:, :3] = coords[n - 1, :3]
    coords[:, 4:] = 0.5
    want = net.density(torch.from_numpy(coords).cuda())[:n, 0].float().cpu().numpy()
    raw = pkg.mesh.density_on_grid(net, "raw", res, aabb, warp_aabb=warp).cpu().numpy().reshape(-1)
    assert raw.tobytes() == want.tobytes()
    ragged = pkg.mesh.density_on_grid(net, "raw", res, aabb, warp_aabb=warp, batch=128).cpu().numpy().reshape(-1)
    assert ragged.tobytes() == raw.tobytes()
    unwarped = pkg.mesh.density_on_grid(net, "raw", res, aabb).cpu().numpy().reshape(-1)
    assert not np.array_equal(unwarped, raw)
    for act, fn in (("Exponential", np.exp), ("None", lambda v: v), ("ReLU", lambda v: np.maximum(v, 0))):
        got = pkg.mesh.density_on_grid(net, "nerf", res, aabb, warp_aabb=warp, density_activation=act).cpu().numpy().reshape(-1)
        np.testing.assert_allclose(got, fn(want.astype(f32)), rtol=1e-5, atol=0)
    with pytest.raises(pkg.NgpError):
        pkg.mesh.density_on_grid(net, "sdf", res, aabb)


# ---- 8, 9: pyngp -------------------------------------------------------------------------------------------------------
def parse_counts(path):
    text = open(path).read().split("\n")
    if str(path).lower().endswith(".ply"):
        nv = int(next(ln for ln in text if ln.startswith("element vertex")).split()[-1])
        nf = int(next(ln for ln in text if ln.startswith("element face")).split()[-1])
        body = text[text.index("end_header") + 1:]
        assert len([ln for ln in body if ln]) == nv + nf
        return nv, nf
    return (sum(ln.startswith("v ") for ln in text), sum(ln.startswith("f ") for ln in text))


def check_mesh_dict(m):
    assert set(m) == {"V", "N", "C", "F"}
    nv, nt = len(m["V"]), len(m["F"])
    for k in "VNC":
        assert m[k].dtype == np.float32 and m[k].shape == (nv, 3)
    assert m["F"].dtype == np.int32 and m["F"].shape == (nt, 3)
    return nv, nt


def test_pyngp_sdf_mesh(pkg, tmp_path):
    ngp = pkg.pyngp()
    verts = pkg.synthetic.icosphere(2, bumps=0.15, seed=1)
    obj = tmp_path / "icosphere.obj"
    with open(obj, "w") as fh:
        for v in verts:
            fh.write("v %r %r %r\n" % (float(v[0]), float(v[1]), float(v[2])))
        for t in range(len(verts) // 3):
            fh.write("f %d %d %d\n" % (3 * t + 1, 3 * t + 2, 3 * t + 3))
    net_cfg = {**pkg.SDF_BASE, "encoding": {**pkg.SDF_BASE["encoding"], "log2_hashmap_size": 14}}
    tb = ngp.Testbed()
    tb.load_training_data(str(obj))
    tb.reload_network_from_json(net_cfg)
    for _ in range(300):
        tb.train(1 << 14)
    # through a snapshot both sides hold the same parameters (after a load the inference parameters are the loaded ones)
    snap = str(tmp_path / "sdf.msgpack")
    tb.save_snapshot(snap, False, False)
    tb.load_snapshot(snap)
    res = [32, 32, 32]
    m = tb.compute_marching_cubes_mesh(resolution=res, thresh=2.5)  # the SDF threshold is forced to 0
    nv, nt = check_mesh_dict(m)
    assert nv > 500 and nt > 1000
    assert len(open_edges(m["F"], nv)) == 0 and euler(m["V"], m["F"]) == 2
    np.testing.assert_allclose(np.linalg.norm(m["N"], axis=1), 1.0, atol=1e-5)

    net = pkg.NetworkWithInputEncoding(3, 1, net_cfg["encoding"], net_cfg["network"])
    tr = pkg.Trainer(net, net_cfg["optimizer"], seed=1337)
    pkg._capi.check(pkg.lib().ngp_load_snapshot(tr.handle, None, snap.encode(), None, None, None, None, None))
    aabb = tb.aabb
    d = pkg.mesh.density_on_grid(net, "sdf", res, aabb)
    mesh = pkg.mesh.extract(d, res, aabb, 0.0)
    V, N, F = mesh.read()
    Cc = pkg.mesh.vertex_colors(mesh, kind="sdf")
    assert np.array_equal(m["V"], V) and np.array_equal(m["F"], F)
    unit = N / np.linalg.norm(N, axis=1, keepdims=True)
    np.testing.assert_allclose(m["N"], unit, atol=1e-6)
    assert np.array_equal(m["C"], Cc)
    np.testing.assert_allclose(Cc, 0.5 * unit + 0.5, atol=1e-6)
    # a given box
    half = tb.compute_marching_cubes_mesh(resolution=[16, 24, 32], aabb=([0.0, 0.0, 0.0], [0.5, 1.0, 1.0]))
    hv, ht = check_mesh_dict(half)
    assert 0 < hv < nv and half["V"][:, 0].max() <= 0.5

    for name in ("mesh.obj", "mesh.ply"):
        path = tmp_path / name
        tb.compute_and_save_marching_cubes_mesh(str(path), resolution=res)
        assert parse_counts(path) == (nv, nt)
    with pytest.raises(RuntimeError, match="generate_uvs_for_obj_file"):
        tb.compute_and_save_marching_cubes_mesh(str(tmp_path / "uv.obj"), resolution=res, generate_uvs_for_obj_file=True)


def test_pyngp_nerf_mesh_colors(pkg, tmp_path):
    import json

    from PIL import Image
    ngp, S = pkg.pyngp(), pkg.synthetic
    scene = tmp_path / "scene"
    scene.mkdir()
    frames = []
    for i, c2w in enumerate(S.camera_poses(8, seed=4)):
        Image.fromarray(S.render(c2w, 64, 64)).save(scene / f"r_{i}.png")
        frames.append({"file_path": f"./r_{i}", "transform_matrix": np.asarray(c2w, np.float64).tolist()})
    (scene / "transforms.json").write_text(json.dumps({"camera_angle_x": S.LEGO_CAMERA_ANGLE_X, "frames": frames}))
    ncfg = pkg.nerf_config("C2")
    ncfg["encoding"]["log2_hashmap_size"] = 14
    tb = ngp.Testbed()
    tb.load_training_data(str(scene))
    tb.reload_network_from_json(ncfg)
    for _ in range(40):
        tb.train(1 << 15)
    snap = str(tmp_path / "nerf.ingp")
    tb.save_snapshot(snap, False, False)
    tb.load_snapshot(snap)

    d = pkg.nerf_data.load_nerf(str(scene))
    ds = pkg.nerf.NerfDataset(d.images, d.rgba8)
    cfg = pkg.nerf.default_config(d.aabb_scale)
    net = pkg.create_nerf_network(ncfg)
    tr = pkg.Trainer(net, ncfg["optimizer"], seed=1337)
    run = pkg.nerf.NerfTraining(net, tr, ds, cfg, seed=1337)
    run.load_snapshot(snap)
    box = (np.asarray(list(cfg.aabb_min), f32), np.asarray(list(cfg.aabb_max), f32))
    res = [24, 24, 24]
    grid = pkg.mesh.density_on_grid(net, "nerf", res, box, warp_aabb=box, density_activation=int(cfg.density_activation))
    flat = np.sort(grid.cpu().numpy().reshape(-1))
    assert np.isfinite(flat).all() and flat[0] < flat[-1]
    lo_v, hi_v = flat[int(0.6 * len(flat))], flat[int(0.95 * len(flat))]
    assert lo_v < hi_v, "the trained density is flat"
    thresh = float(0.5 * (float(lo_v) + float(hi_v)))
    m = tb.compute_marching_cubes_mesh(resolution=res, thresh=thresh)
    nv, nt = check_mesh_dict(m)
    assert nv > 0 and nt > 0, "the mesh is empty"
    V, N, F = pkg.mesh.marching_cubes(grid.reshape(-1), res, box, thresh)
    assert np.array_equal(m["V"], V) and np.array_equal(m["F"], F)

    # the test's own colours: inference at (V, -N), rgb activation, linear -> sRGB
    coords = np.zeros(((nv + 255) // 256 * 256, 7), f32)
    coords[:nv, :3] = (m["V"] - box[0]) / (box[1] - box[0])
    coords[:nv, 4:] = (-m["N"] + 1.0) * 0.5
    coords[nv:] = coords[nv - 1]
    out = net.inference(torch.from_numpy(coords).cuda())[:nv, :3].float().cpu().numpy().astype(np.float64)
    act = int(cfg.rgb_activation)
    rgb = {0: lambda v: v, 1: lambda v: np.maximum(v, 0), 2: lambda v: 1 / (1 + np.exp(-v)), 3: lambda v: np.exp(np.clip(v, -10, 10))}[act](out)
    want = np.where(rgb < 0.0031308, 12.92 * rgb, 1.055 * np.power(np.maximum(rgb, 0), 0.41666) - 0.055)
    err = np.abs(m["C"] - want).max()
    print(f"NeRF mesh: {nv} vertices, thresh {thresh:.3f}, colours max |err| {err:.3e}")
    assert err <= 1e-4
    path = tmp_path / "nerf.ply"
    tb.compute_and_save_marching_cubes_mesh(str(path), resolution=res, thresh=thresh)
    assert parse_counts(path) == (nv, nt)
    # vertices go back to the dataset's units: (p - offset) / scale
    rows = open(path).read().split("end_header\n")[1].split("\n")[:nv]
    saved = np.asarray([[float(t) for t in r.split()[:3]] for r in rows])
    np.testing.assert_allclose(saved, (m["V"] - np.asarray(d.offset, f32)) / f32(d.scale), atol=2e-5)
