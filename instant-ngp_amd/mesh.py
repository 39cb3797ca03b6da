"""Mesh extraction from a trained model (Testbed::marching_cubes, src/marching_cubes.cu) over the C-ABI:
the model sampled on a regular grid (`density_on_grid`), marching cubes with normals (`marching_cubes`),
vertex colours (`vertex_colors`) and the .obj / .ply writer (`save_mesh`). Kernels: csrc/marching_cubes.hip.

Vertex and triangle order are a function of the grid alone, so two runs return byte-identical arrays.
"""
import ctypes as C

import numpy as np
import torch

from ._capi import check, lib
from .network import _ptr, _stream

KINDS = {"nerf": 0, "sdf": 1, "raw": 2}  # NGP_MC_NERF / NGP_MC_SDF / NGP_MC_RAW
ACTIVATIONS = {"None": 0, "ReLU": 1, "Logistic": 2, "Exponential": 3}  # ENerfActivation


def _f3(v):
    return np.ascontiguousarray(np.asarray(v, dtype=np.float32).reshape(3))


def _res(res):
    r = np.asarray([res] * 3 if np.isscalar(res) else res, dtype=np.int64).reshape(3)
    if (r < 0).any() or (r >= 1 << 32).any():
        raise ValueError("resolution out of range")
    return np.ascontiguousarray(r.astype(np.uint32))


def _mat(m):
    return None if m is None else np.ascontiguousarray(np.asarray(m, dtype=np.float32).reshape(3, 3))


def _np_ptr(a):
    return a.ctypes.data if a is not None else None


def _act(a):
    return ACTIVATIONS[a] if isinstance(a, str) else int(a)


def mc_tables():
    """The engine's generated case table: (triangles int8 [256, 16] of edge ids, -1 terminated; edge masks uint16 [256])."""
    tri = np.zeros((256, 16), np.int8)
    edges = np.zeros(256, np.uint16)
    check(lib().ngp_mc_tables(tri.ctypes.data, edges.ctypes.data))
    return tri, edges


def marching_cubes_res(res_1d, aabb):
    """get_marching_cubes_res: `res_1d` points along the longest side of aabb = (min, max), each axis a multiple of 16."""
    lo, hi = _f3(aabb[0]), _f3(aabb[1])
    out = np.zeros(3, np.uint32)
    check(lib().ngp_marching_cubes_res(int(res_1d), lo.ctypes.data, hi.ctypes.data, out.ctypes.data))
    return tuple(int(v) for v in out)


def density_on_grid(network, kind, res, aabb, aabb_to_local=None, warp_aabb=None, density_activation="Exponential",
                    use_inference_params=True, batch=1 << 20, stream=None):
    """The model on the grid: a CUDA float32 tensor [res_z, res_y, res_x] (x fastest). kind "nerf": the NerfNetwork's
    activated density at positions warped into warp_aabb (the training box); "sdf": minus the distance (inside > 0);
    "raw": float(output row 0). aabb_to_local (3x3) is applied to the positions as its transpose."""
    r, lo, hi, rot = _res(res), _f3(aabb[0]), _f3(aabb[1]), _mat(aabb_to_local)
    wlo = _f3(warp_aabb[0]) if warp_aabb is not None else None
    whi = _f3(warp_aabb[1]) if warp_aabb is not None else None
    n = int(r[0]) * int(r[1]) * int(r[2])
    # an invalid grid is rejected by the engine before the output is touched
    out = torch.empty(n if 0 < n < 1 << 32 and r.min() >= 2 else 1, dtype=torch.float32, device="cuda")
    check(lib().ngp_density_on_grid(network.handle, _stream(stream), KINDS[kind] if isinstance(kind, str) else int(kind),
                                    r.ctypes.data, lo.ctypes.data, hi.ctypes.data, _np_ptr(rot), _np_ptr(wlo), _np_ptr(whi),
                                    _act(density_activation), int(batch), int(use_inference_params), _ptr(out)))
    return out.view(int(r[2]), int(r[1]), int(r[0]))


class Mesh:
    """An extracted mesh on the device (ngp_mesh)."""

    def __init__(self, handle):
        self.handle = handle

    @property
    def counts(self):
        nv, nt = C.c_uint32(0), C.c_uint32(0)
        check(lib().ngp_mesh_counts(self.handle, C.byref(nv), C.byref(nt)))
        return nv.value, nt.value

    def read(self, colors=False, stream=None):
        """(V, N, F) or (V, N, C, F) as numpy arrays: float32 [n, 3] and int32 [m, 3]."""
        nv, nt = self.counts
        V, N, F = np.zeros((nv, 3), np.float32), np.zeros((nv, 3), np.float32), np.zeros((nt, 3), np.int32)
        Cc = np.zeros((nv, 3), np.float32) if colors else None
        check(lib().ngp_mesh_read(self.handle, _stream(stream), V.ctypes.data, N.ctypes.data, _np_ptr(Cc), F.ctypes.data))
        return (V, N, Cc, F) if colors else (V, N, F)

    def __del__(self):
        h = getattr(self, "handle", None)
        if h:
            try:
                lib().ngp_mesh_destroy(h)
            except Exception:
                pass
            self.handle = None


def extract(density, res, aabb, thresh, aabb_to_local=None, stream=None):
    """ngp_marching_cubes: the Mesh of a device density grid (float32, res_x * res_y * res_z values, x fastest)."""
    r, lo, hi, rot = _res(res), _f3(aabb[0]), _f3(aabb[1]), _mat(aabb_to_local)
    if not (density.is_cuda and density.dtype == torch.float32 and density.is_contiguous()):
        raise ValueError("density must be a contiguous CUDA float32 tensor")
    if density.numel() != int(r[0]) * int(r[1]) * int(r[2]):
        raise ValueError("density does not hold res_x * res_y * res_z values")
    h = C.c_void_p()
    check(lib().ngp_marching_cubes(_stream(stream), _ptr(density), r.ctypes.data, lo.ctypes.data, hi.ctypes.data, _np_ptr(rot),
                                   float(thresh), C.byref(h)))
    return Mesh(h)


def marching_cubes(density, res, aabb, thresh, aabb_to_local=None, stream=None):
    """V float32 [n, 3], N float32 [n, 3] (area-weighted outward normals, not normalised), F int32 [m, 3] (counter-clockwise
    seen from the side where density <= thresh)."""
    return extract(density, res, aabb, thresh, aabb_to_local, stream).read(stream=stream)


def vertex_colors(mesh, network=None, kind="sdf", warp_aabb=None, rgb_activation="Logistic", use_inference_params=True,
                  stream=None):
    """Vertex colours of a Mesh, float32 [n, 3]. "nerf": the network at the vertices seen along minus the normal, rgb
    activation, linear -> sRGB; "sdf": 0.5 n + 0.5."""
    wlo = _f3(warp_aabb[0]) if warp_aabb is not None else None
    whi = _f3(warp_aabb[1]) if warp_aabb is not None else None
    check(lib().ngp_mesh_vertex_colors(mesh.handle, network.handle if network is not None else None, _stream(stream),
                                       KINDS[kind] if isinstance(kind, str) else int(kind), _np_ptr(wlo), _np_ptr(whi),
                                       _act(rgb_activation), int(use_inference_params)))
    return mesh.read(colors=True, stream=stream)[2]


def save_mesh(path, V, N=None, colors=None, F=None, scale=1.0, offset=(0.0, 0.0, 0.0)):
    """save_mesh: host arrays to .obj, or ASCII .ply when the extension says so; vertices written as (p - offset) / scale."""
    V = np.ascontiguousarray(V, dtype=np.float32).reshape(-1, 3)
    N = None if N is None else np.ascontiguousarray(N, dtype=np.float32).reshape(-1, 3)
    colors = None if colors is None else np.ascontiguousarray(colors, dtype=np.float32).reshape(-1, 3)
    F = np.zeros((0, 3), np.int32) if F is None else np.ascontiguousarray(F, dtype=np.int32).reshape(-1, 3)
    for a in (N, colors):
        if a is not None and a.shape != V.shape:
            raise ValueError("normals and colours need one row per vertex")
    off = _f3(offset)
    check(lib().ngp_mesh_save(str(path).encode(), V.shape[0], V.ctypes.data, _np_ptr(N), _np_ptr(colors), F.shape[0], F.ctypes.data,
                              float(scale), off.ctypes.data))
