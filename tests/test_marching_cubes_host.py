"""The host side of the mesh extraction, without a GPU: the generated marching-cubes case table (ngp_mc_tables), the
grid resolution of a box (ngp_marching_cubes_res, marching_cubes.cu:42-49), the .obj / .ply writer (ngp_mesh_save,
marching_cubes.cu:806-956), argument checks that return NGP_INVALID before any HIP call, and the pyngp methods."""
import ctypes as C
import itertools

import numpy as np
import pytest

NGP_INVALID = -2

CORNERS = [(0, 0, 0), (1, 0, 0), (1, 1, 0), (0, 1, 0), (0, 0, 1), (1, 0, 1), (1, 1, 1), (0, 1, 1)]
EDGES = [(0, 1), (1, 2), (2, 3), (3, 0), (4, 5), (5, 6), (6, 7), (7, 4), (0, 4), (1, 5), (2, 6), (3, 7)]


@pytest.fixture(scope="module")
def pkg():
    from __graft_entry__ import load_package
    return load_package()


@pytest.fixture(scope="module")
def table(pkg):
    """(list of triangle lists per case, edge masks)"""
    tri, masks = pkg.mesh.mc_tables()
    cases = []
    for row in tri:
        row = [int(v) for v in row]
        n = row.index(-1)
        assert n % 3 == 0 and n <= 15, "rows are -1 terminated and hold at most 5 triangles"
        assert all(v == -1 for v in row[n:])
        assert all(0 <= v < 12 for v in row[:n])
        cases.append([tuple(row[k:k + 3]) for k in range(0, n, 3)])
    return cases, masks


def edges_on_one_face(a, b):
    """both cube edges lie in one face of the cube: some coordinate is constant over their four corners"""
    pts = [CORNERS[c] for c in EDGES[a] + EDGES[b]]
    return any(len({p[ax] for p in pts}) == 1 for ax in range(3))


def crossing_edges(case):
    return {e for e, (a, b) in enumerate(EDGES) if ((case >> a) & 1) != ((case >> b) & 1)}


def test_table_rows(table):
    cases, masks = table
    assert sum(len(t) for t in cases) == 820
    assert max(len(t) for t in cases) == 5
    for case, tris in enumerate(cases):
        cross = crossing_edges(case)
        assert {e for t in tris for e in t} == cross, case
        assert int(masks[case]) == sum(1 << e for e in cross), case
        directed = [(t[k], t[(k + 1) % 3]) for t in tris for k in range(3)]
        assert len(set(directed)) == len(directed), f"case {case}: a directed edge occurs twice"
        have = set(directed)
        for a, b in directed:
            if (b, a) in have:  # an inner diagonal of a fan: never in a face of the cube
                assert not edges_on_one_face(a, b), (case, a, b)
            else:               # a boundary segment: lies in a face, where the neighbouring cell continues it
                assert edges_on_one_face(a, b), (case, a, b)


def face_segments(tris, axis, side):
    """the directed boundary segments of a case that lie in the face `axis` = `side`"""
    face_edges = {e for e, (a, b) in enumerate(EDGES) if CORNERS[a][axis] == side and CORNERS[b][axis] == side}
    directed = {(t[k], t[(k + 1) % 3]) for t in tris for k in range(3)}
    return {(a, b) for a, b in directed if (b, a) not in directed and a in face_edges and b in face_edges}


def test_table_neighbours_agree(table):
    """Two cells sharing a face see the same four signs there; their segments on it must be equal and opposite. The
    segments depend on the four signs alone, so it is enough to compare, per axis and per face pattern, every case's
    high face with every case's low face after moving the edges across the cell."""
    cases, _ = table
    for axis in range(3):
        lo_c = [c for c in range(8) if CORNERS[c][axis] == 0]
        partner = {}  # corner on the low face -> the corner opposite on the high face
        for c in lo_c:
            p = list(CORNERS[c])
            p[axis] = 1
            partner[c] = CORNERS.index(tuple(p))
        edge_up = {}  # edge in the low face -> the same edge seen from the cell below, in its high face
        for e, (a, b) in enumerate(EDGES):
            if a in partner and b in partner:
                edge_up[e] = next(k for k, (u, v) in enumerate(EDGES) if {u, v} == {partner[a], partner[b]})
        by_pattern_lo, by_pattern_hi = {}, {}
        for case in range(256):
            pat_lo = tuple((case >> c) & 1 for c in lo_c)
            pat_hi = tuple((case >> partner[c]) & 1 for c in lo_c)
            seg_lo = frozenset((edge_up[a], edge_up[b]) for a, b in face_segments(cases[case], axis, 0))
            seg_hi = frozenset(face_segments(cases[case], axis, 1))
            by_pattern_lo.setdefault(pat_lo, set()).add(seg_lo)
            by_pattern_hi.setdefault(pat_hi, set()).add(seg_hi)
        assert len(by_pattern_lo) == 16 and len(by_pattern_hi) == 16
        for pat in by_pattern_lo:
            assert len(by_pattern_lo[pat]) == 1 and len(by_pattern_hi[pat]) == 1, (axis, pat)
            (lo,), (hi,) = by_pattern_lo[pat], by_pattern_hi[pat]
            # the cell above (its low face) and the cell below (its high face) run the segments in opposite directions
            assert lo == frozenset((b, a) for a, b in hi), (axis, pat)


def test_table_orientation(table):
    cases, _ = table
    mid = [(np.asarray(CORNERS[a], float) + np.asarray(CORNERS[b], float)) / 2 for a, b in EDGES]
    for c in range(8):
        (t,) = cases[1 << c]
        p = [mid[e] for e in t]
        n = np.cross(p[1] - p[0], p[2] - p[0])
        assert np.dot(n, np.mean(p, axis=0) - np.asarray(CORNERS[c], float)) > 0, c  # away from the inside corner


def test_table_is_manifold_on_a_random_field(table):
    cases, _ = table
    R = 12
    f = np.zeros((R, R, R))
    f[1:-1, 1:-1, 1:-1] = np.random.default_rng(0).random((R - 2, R - 2, R - 2))
    inside = f > 0.5
    count = {}
    for x, y, z in itertools.product(range(R - 1), repeat=3):
        case = sum(1 << i for i, c in enumerate(CORNERS) if inside[x + c[0], y + c[1], z + c[2]])
        for t in cases[case]:
            v = []
            for e in t:
                a = tuple(np.add((x, y, z), CORNERS[EDGES[e][0]]))
                b = tuple(np.add((x, y, z), CORNERS[EDGES[e][1]]))
                v.append((min(a, b), max(a, b)))
            for k in range(3):
                key = (v[k], v[(k + 1) % 3])
                count[key] = count.get(key, 0) + 1
    assert count
    assert all(n == 1 and count.get((k[1], k[0]), 0) == 1 for k, n in count.items())


def reference_res(res_1d, lo, hi):
    f32 = np.float32
    d = np.asarray(hi, f32) - np.asarray(lo, f32)
    scale = f32(res_1d) / d.max()
    r = (d * scale + f32(0.5)).astype(np.int32)
    return tuple(int((v + 15) // 16 * 16) for v in r)


@pytest.mark.parametrize("res_1d,lo,hi", [
    (128, (0, 0, 0), (1, 1, 1)),
    (100, (0, 0, 0), (1, 1, 1)),
    (256, (-0.3, 0.1, 0.2), (0.9, 0.7, 1.4)),
    (77, (0.25, 0.0, 0.4), (0.75, 1.0, 0.6)),
    (1, (0, 0, 0), (1, 2, 4)),
])
def test_marching_cubes_res(pkg, res_1d, lo, hi):
    got = pkg.mesh.marching_cubes_res(res_1d, (lo, hi))
    assert got == reference_res(res_1d, lo, hi)
    assert all(v % 16 == 0 for v in got)


def parse_obj(path):
    v, c, vn, f = [], [], [], []
    for line in open(path):
        tok = line.split()
        if tok[0] == "v":
            v.append([float(t) for t in tok[1:4]])
            c.append([float(t) for t in tok[4:7]])
        elif tok[0] == "vn":
            vn.append([float(t) for t in tok[1:4]])
        elif tok[0] == "f":
            idx = [t.split("//") for t in tok[1:]]
            assert all(a == b for a, b in idx)
            f.append([int(a) for a, _ in idx])
    return np.asarray(v), np.asarray(c), np.asarray(vn), np.asarray(f)


def parse_ply(path):
    lines = open(path).read().split("\n")
    assert lines[0] == "ply" and lines[1] == "format ascii 1.0"
    end = lines.index("end_header")
    nv = int(next(ln for ln in lines[:end] if ln.startswith("element vertex")).split()[-1])
    nf = int(next(ln for ln in lines[:end] if ln.startswith("element face")).split()[-1])
    rows = [[float(t) for t in ln.split()] for ln in lines[end + 1:end + 1 + nv]]
    faces = [[int(t) for t in ln.split()] for ln in lines[end + 1 + nv:end + 1 + nv + nf]]
    assert all(r[0] == 3 for r in faces)
    rows = np.asarray(rows)
    return rows[:, :3], rows[:, 6:9], rows[:, 3:6], np.asarray(faces)[:, 1:]


def test_mesh_save_round_trip(pkg, tmp_path):
    V = np.asarray([[0.5, 0.5, 0.5], [1.5, 0.5, 0.5], [0.5, 1.5, 0.5], [np.nan, 0.5, 1.5]], np.float32)
    N = np.asarray([[0, 0, 3.0], [2.0, 0, 0], [0, np.inf, 0], [1, 1, 1]], np.float32)
    Cc = np.asarray([[0.25, 0.5, 0.75], [1.5, -0.5, 0.5], [np.nan, 0, 0], [0, 1, 0]], np.float32)
    F = np.asarray([[0, 2, 1], [0, 1, 3], [1, 2, 3], [2, 0, 3]], np.int32)
    scale, offset = 0.5, (0.5, 0.25, 0.0)
    want_v = (np.where(np.isfinite(V).all(1, keepdims=True), V, 0.0) - np.asarray(offset)) / scale
    want_n = np.asarray([[0, 0, 1], [1, 0, 0], [0, 1, 0], [3 ** -0.5] * 3])
    want_c = np.asarray([[0.25, 0.5, 0.75], [1.0, 0.0, 0.5], [0, 0, 0], [0, 1, 0]])

    obj = tmp_path / "tet.obj"
    pkg.mesh.save_mesh(obj, V, N, Cc, F, scale=scale, offset=offset)
    v, c, vn, f = parse_obj(obj)
    assert v.shape == (4, 3) and vn.shape == (4, 3) and f.shape == (4, 3)
    np.testing.assert_allclose(v, want_v, atol=1e-5)
    np.testing.assert_allclose(c, want_c, atol=1e-3)
    np.testing.assert_allclose(vn, want_n, atol=1e-5)
    assert np.array_equal(f, F + 1)  # 1-based, winding kept

    ply = tmp_path / "tet.PLY"  # the extension is matched without case
    pkg.mesh.save_mesh(ply, V, N, Cc, F, scale=scale, offset=offset)
    v, c, vn, f = parse_ply(ply)
    assert v.shape == (4, 3) and f.shape == (4, 3)
    np.testing.assert_allclose(v, want_v, atol=1e-5)
    np.testing.assert_allclose(vn, want_n, atol=1e-3)
    assert np.array_equal(c, np.floor(want_c * 255.0))  # uchar, clamped to [0, 255]
    assert np.array_equal(f, F)

    # without normals and colours: +y and black
    bare = tmp_path / "bare.obj"
    pkg.mesh.save_mesh(bare, V, F=F)
    v, c, vn, f = parse_obj(bare)
    assert np.array_equal(vn, np.tile([0.0, 1.0, 0.0], (4, 1))) and not c.any() and np.array_equal(f, F + 1)


def test_invalid_arguments_fail_without_gpu(pkg, tmp_path):
    lib = pkg.lib()
    fake = C.c_void_p(0x1000)  # never dereferenced: every call below is rejected first
    f3 = lambda *v: np.asarray(v, np.float32)  # noqa: E731
    lo, hi = f3(0, 0, 0), f3(1, 1, 1)
    good = np.asarray([8, 8, 8], np.uint32)
    out = C.c_void_p()

    def mc(density=fake, res=good, a=lo, b=hi, thresh=0.0, o=C.byref(out)):
        return lib.ngp_marching_cubes(None, density, res.ctypes.data if res is not None else None, a.ctypes.data, b.ctypes.data,
                                      None, thresh, o)

    def grid(model=fake, res=good, a=lo, b=hi, kind=2, batch=1 << 20, o=fake):
        return lib.ngp_density_on_grid(model, None, kind, res.ctypes.data if res is not None else None, a.ctypes.data,
                                       b.ctypes.data, None, None, None, 3, batch, 1, o)

    assert mc(o=None) == NGP_INVALID and mc(density=None) == NGP_INVALID and mc(res=None) == NGP_INVALID
    assert grid(o=None) == NGP_INVALID and grid(model=None) == NGP_INVALID and grid(res=None) == NGP_INVALID
    assert grid(kind=3) == NGP_INVALID and grid(batch=0) == NGP_INVALID
    for bad in ([1, 8, 8], [8, 0, 8], [8, 8, 1]):
        r = np.asarray(bad, np.uint32)
        assert mc(res=r) == NGP_INVALID and grid(res=r) == NGP_INVALID
        assert b"at least 2" in lib.ngp_last_error()
    for big in ([1 << 16, 1 << 16, 2], [1 << 11, 1 << 11, 1 << 10], [0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF]):
        r = np.asarray(big, np.uint32)  # 2^33, 2^32, and a product that overflows 64 bits
        assert mc(res=r) == NGP_INVALID and grid(res=r) == NGP_INVALID
        assert b"2^32" in lib.ngp_last_error()
    for a, b in ((lo, lo), (hi, lo), (lo, f3(1, 0, 1)), (lo, f3(1, np.nan, 1)), (lo, f3(1, np.inf, 1))):
        assert mc(a=a, b=b) == NGP_INVALID and grid(a=a, b=b) == NGP_INVALID
        assert b"box" in lib.ngp_last_error()
    assert mc(thresh=float("nan")) == NGP_INVALID
    assert out.value is None

    assert lib.ngp_mc_tables(None, fake) == NGP_INVALID and lib.ngp_mc_tables(fake, None) == NGP_INVALID
    r3 = np.zeros(3, np.uint32)
    assert lib.ngp_marching_cubes_res(16, lo.ctypes.data, hi.ctypes.data, None) == NGP_INVALID
    assert lib.ngp_marching_cubes_res(16, None, hi.ctypes.data, r3.ctypes.data) == NGP_INVALID
    assert lib.ngp_marching_cubes_res(0, lo.ctypes.data, hi.ctypes.data, r3.ctypes.data) == NGP_INVALID
    assert lib.ngp_marching_cubes_res(16, hi.ctypes.data, lo.ctypes.data, r3.ctypes.data) == NGP_INVALID
    assert lib.ngp_mesh_counts(None, None, None) == NGP_INVALID
    assert lib.ngp_mesh_read(None, None, None, None, None, None) == NGP_INVALID
    assert lib.ngp_mesh_vertex_colors(None, fake, None, 0, None, None, 2, 1) == NGP_INVALID
    assert lib.ngp_mesh_vertex_colors(fake, fake, None, 2, None, None, 2, 1) == NGP_INVALID  # RAW has no colours
    assert lib.ngp_mesh_vertex_colors(fake, None, None, 0, None, None, 2, 1) == NGP_INVALID  # NeRF colours need the model
    lib.ngp_mesh_destroy(None)

    V = np.zeros((3, 3), np.float32)
    F = np.asarray([[0, 1, 2]], np.int32)
    path = str(tmp_path / "x.obj").encode()
    assert lib.ngp_mesh_save(None, 3, V.ctypes.data, None, None, 1, F.ctypes.data, 1.0, None) == NGP_INVALID
    assert lib.ngp_mesh_save(path, 3, None, None, None, 1, F.ctypes.data, 1.0, None) == NGP_INVALID
    assert lib.ngp_mesh_save(path, 3, V.ctypes.data, None, None, 1, None, 1.0, None) == NGP_INVALID
    assert lib.ngp_mesh_save(path, 3, V.ctypes.data, None, None, 1, F.ctypes.data, 0.0, None) == NGP_INVALID
    Fbad = np.asarray([[0, 1, 3]], np.int32)
    assert lib.ngp_mesh_save(path, 3, V.ctypes.data, None, None, 1, Fbad.ctypes.data, 1.0, None) == NGP_INVALID
    assert lib.ngp_mesh_save(path, 3, V.ctypes.data, None, None, 1, F.ctypes.data, 1.0, None) == 0


def test_pyngp_methods_raise_without_a_model(pkg, tmp_path):
    ngp = pkg.pyngp()
    for mode in (ngp.TestbedMode.Sdf, ngp.TestbedMode.Nerf):
        tb = ngp.Testbed(mode)
        with pytest.raises(RuntimeError, match="no network"):
            tb.compute_marching_cubes_mesh()
        with pytest.raises(RuntimeError, match="no network"):
            tb.compute_and_save_marching_cubes_mesh(str(tmp_path / "m.obj"), resolution=[16, 16, 16])
        with pytest.raises(RuntimeError, match="generate_uvs_for_obj_file"):
            tb.compute_and_save_marching_cubes_mesh(str(tmp_path / "m.obj"), generate_uvs_for_obj_file=True)
    for mode in (ngp.TestbedMode.Image, ngp.TestbedMode.Volume, getattr(ngp.TestbedMode, "None")):
        tb = ngp.Testbed(mode)
        with pytest.raises(RuntimeError, match="only NeRF and SDF"):
            tb.compute_marching_cubes_mesh(resolution=[16, 16, 16], aabb=([0, 0, 0], [1, 1, 1]), thresh=1.0)
        with pytest.raises(RuntimeError, match="only NeRF and SDF"):
            tb.compute_and_save_marching_cubes_mesh(str(tmp_path / "m.ply"))
    assert not list(tmp_path.iterdir())  # nothing was written
