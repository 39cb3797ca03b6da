"""Host mirror of the Testbed's SDF primitive (BASELINE config C5, src/testbed_sdf.cu) over the C-ABI.

`load_mesh` restates Testbed::load_mesh's normalisation (testbed_sdf.cu:1120-1165); `SdfTraining` is
training_prep_sdf + train_sdf (:1289-1330): every step regenerates the batch online
(generate_training_samples_sdf, :1187-1275, non-octree branch), shuffles it and runs tcnn
training_step with the MAPE loss (configs/sdf/base.json) and the optimizer. Signed distances come
from a 4-ary triangle BVH (TriangleBvh4, src/triangle_bvh.cu; csrc/bvh.hip) traversed on the GPU.
`SdfRenderer` is the SphereTracer and render_sdf (:629-1063; csrc/sdf_render.hip), `iou` calculate_iou (:1329-1364).
"""
import ctypes as C

import numpy as np
import torch

from ._capi import SdfRenderConfig, check, lib
from .nerf import pcg32
from .network import _ptr, _stream


def load_mesh(vertices):
    """Normalise triangle-soup vertices [3T, 3] into the unit cube as Testbed::load_mesh does.
    Returns (triangles [T, 9] float32, aabb_min, aabb_max, bounding_radius)."""
    v = np.asarray(vertices, dtype=np.float32).reshape(-1, 3)
    if v.shape[0] % 3 != 0 or v.shape[0] == 0:
        raise ValueError("vertices must hold whole triangles")
    inflation = np.float32(0.005)
    lo, hi = v.min(axis=0), v.max(axis=0)
    amount = np.float32(np.linalg.norm(hi - lo)) * inflation
    lo, hi = lo - amount, hi + amount
    diag = hi - lo
    scale = np.float32(diag.max())
    v = (v - lo - np.float32(0.5) * diag) / scale + np.float32(0.5)
    alo, ahi = v.min(axis=0), v.max(axis=0)
    amount = np.float32(np.linalg.norm(ahi - alo)) * inflation
    alo, ahi = np.maximum(alo - amount, 0.0), np.minimum(ahi + amount, 1.0)  # intersection with [0,1]^3
    bounding_radius = float(np.linalg.norm(np.full(3, 0.5, np.float32)))
    return (np.ascontiguousarray(v.reshape(-1, 9), dtype=np.float32), alo.astype(np.float32), ahi.astype(np.float32),
            bounding_radius)


BVH_NODE = np.dtype([("lo", np.float32, 3), ("hi", np.float32, 3), ("left", np.int32), ("right", np.int32)])


def build_bvh(triangles, n_primitives_per_leaf=8):
    """TriangleBvh4::build on the host (no GPU): (triangles in BVH order, nodes structured array)."""
    tris = np.array(triangles, dtype=np.float32).reshape(-1, 9)
    n = C.c_uint32(0)
    check(lib().ngp_sdf_bvh_build(tris.ctypes.data, tris.shape[0], n_primitives_per_leaf, None, C.byref(n)))
    nodes = np.zeros(n.value, dtype=BVH_NODE)
    check(lib().ngp_sdf_bvh_build(tris.ctypes.data, tris.shape[0], n_primitives_per_leaf, nodes.ctypes.data, C.byref(n)))
    return tris, nodes


class SdfMesh:
    """The mesh on the device with its BVH. `triangles` is the BVH order (the build reorders them, as
    TriangleBvh4::build reorders m_sdf.triangles_cpu; surface sampling draws from that order)."""

    def __init__(self, triangles):
        tris = np.ascontiguousarray(triangles, dtype=np.float32).reshape(-1, 9)
        h = C.c_void_p()
        check(lib().ngp_sdf_mesh_create(tris.shape[0], tris.ctypes.data, C.byref(h)))
        self.handle = h
        self.triangles = np.empty_like(tris)
        check(lib().ngp_sdf_mesh_triangles(h, self.triangles.ctypes.data))

    def signed_distance(self, positions, rows=None, stream=None):
        """rows (int32 [n], optional): the index seeding each point's stab rays (ngp_sdf_signed_distance_rows); default:
        the point's place in the batch."""
        out = torch.empty(positions.shape[0], dtype=torch.float32, device=positions.device)
        if rows is None:
            check(lib().ngp_sdf_signed_distance(self.handle, _stream(stream), positions.shape[0], _ptr(positions), _ptr(out)))
        else:
            assert rows.dtype == torch.int32 and rows.numel() == positions.shape[0] and rows.is_cuda
            check(lib().ngp_sdf_signed_distance_rows(self.handle, _stream(stream), positions.shape[0], _ptr(positions),
                                                     _ptr(rows), _ptr(out)))
        return out

    def __del__(self):
        h = getattr(self, "handle", None)
        if h:
            try:
                lib().ngp_sdf_mesh_destroy(h)
            except Exception:
                pass
            self.handle = None


RENDER_MODES = {"AO": 0, "Shade": 1, "Normals": 2, "Positions": 3, "Depth": 4, "Cost": 6}  # ERenderMode (common.h:110-119)
MAX_DEPTH = 16384.0  # common_device.cuh:33: the depth of a pixel whose ray hits nothing


def default_render_config(**overrides):
    """Testbed::Sdf's render defaults, sun / up direction and BRDFParams (testbed.h:601-602, 798-835, sdf.h:62-72)."""
    cfg = SdfRenderConfig()
    check(lib().ngp_sdf_render_default_config(C.byref(cfg)))
    for k, v in overrides.items():
        if isinstance(getattr(cfg, k), C.Array):
            getattr(cfg, k)[:] = [float(x) for x in v]
        else:
            setattr(cfg, k, v)
    return cfg


class SdfRenderer:
    """SphereTracer + Testbed::render_sdf (testbed_sdf.cu:629-1063): sphere-traces the network's distance, or the
    mesh's own signed distance (render_ground_truth), from a camera. Output: linear RGBA [H, W, 4] float32, alpha 1 on
    hits and `background` elsewhere."""

    def __init__(self):
        h = C.c_void_p()
        check(lib().ngp_sdf_renderer_create(C.byref(h)))
        self.handle = h

    def render(self, network=None, ground_truth=None, cfg=None, camera=None, mode="Shade", spp=1, sample_index=0,
               background=(0.0, 0.0, 0.0, 0.0), use_inference_params=True, return_depth=False, stream=None):
        """Exactly one of network (a NetworkWithInputEncoding 3 -> 1) / ground_truth (an SdfMesh). camera: a NerfImage
        (nerf.make_image). mode: an ERenderMode name. return_depth: also dot(camera forward, pos - origin) [H, W]."""
        cfg = cfg if cfg is not None else default_render_config()
        out = torch.empty((camera.height, camera.width, 4), dtype=torch.float32, device="cuda")
        depth = torch.empty((camera.height, camera.width), dtype=torch.float32, device="cuda") if return_depth else None
        bg = (C.c_float * 4)(*[float(v) for v in background])
        check(lib().ngp_sdf_render(self.handle, network.handle if network is not None else None,
                                   ground_truth.handle if ground_truth is not None else None, C.byref(cfg), _stream(stream),
                                   C.byref(camera), RENDER_MODES[mode] if isinstance(mode, str) else int(mode), spp, sample_index, bg,
                                   int(use_inference_params), _ptr(out), _ptr(depth)))
        return (out, depth) if return_depth else out

    def __del__(self):
        h = getattr(self, "handle", None)
        if h:
            try:
                lib().ngp_sdf_renderer_destroy(h)
            except Exception:
                pass
            self.handle = None


def iou_accumulate(distances_ref, distances_model, counters=None, scale_existing=1.0, stream=None):
    """compare_signs_kernel + scale_iou_counters_kernel (testbed_sdf.cu:474-499) on fp32 distances: the eight uint32
    counters (as int32 storage) scaled by scale_existing (if < 1), then the samples added. Returns the counters."""
    if counters is None:
        counters = torch.zeros(8, dtype=torch.int32, device=distances_ref.device)
    n = distances_ref.numel()
    assert distances_model.numel() == n and distances_ref.dtype == distances_model.dtype == torch.float32
    check(lib().ngp_sdf_iou_accumulate(_stream(stream), n, _ptr(distances_ref), _ptr(distances_model), float(scale_existing),
                                       _ptr(counters)))
    return counters


def iou(mesh, network, n_samples, rng, aabb_min=(0.0, 0.0, 0.0), aabb_max=(1.0, 1.0, 1.0), batch=1 << 18,
        use_inference_params=True, stream=None):
    """Testbed::calculate_iou (testbed_sdf.cu:1329-1364) without the octree: uniform positions in the aabb drawn from
    `rng` (a pcg32, advanced), the mesh's and the network's distance at each, intersection over union of the two
    insides = counters[4] / counters[5]. The positions are the uniform eighth of generate_training_samples_sdf's
    batch (:1187-1275), which also carries their signed distances."""
    lo, hi = np.asarray(aabb_min, np.float32), np.asarray(aabb_max, np.float32)
    counters = torch.zeros(8, dtype=torch.int32, device="cuda")
    left = int(n_samples)
    while left > 0:
        m = min(left, batch)
        left -= m
        pos = torch.empty((8 * m, 3), dtype=torch.float32, device="cuda")
        dist = torch.empty(8 * m, dtype=torch.float32, device="cuda")
        check(lib().ngp_sdf_generate_training_samples(mesh.handle, _stream(stream), 8 * m, C.byref(rng), lo.ctypes.data,
                                                      hi.ctypes.data, 0.0, _ptr(pos), _ptr(dist)))
        p, ref = pos[7 * m:], dist[7 * m:]
        model = network.inference(p, layout=1, use_inference_params=use_inference_params, stream=stream)[0].float()
        iou_accumulate(ref, model, counters, stream=stream)
    c = counters.cpu().numpy().view(np.uint32)
    return float(c[4]) / float(c[5]) if c[5] else 0.0


class SdfTraining:
    """Testbed SDF training (training_prep_sdf + train_sdf) over a NetworkWithInputEncoding (3 -> 1)."""

    def __init__(self, network, trainer, mesh, aabb_min, aabb_max, bounding_radius=float(np.sqrt(0.75)), seed=1337,
                 batch_size=1 << 18, surface_offset_scale=1.0, zero_offset=0.0):
        self.network, self.trainer, self.mesh = network, trainer, mesh
        self.rng = pcg32(seed)
        self.batch_size = batch_size
        # sdf_aabb = m_aabb inflated by zero_offset (testbed_sdf.cu:1238-1239)
        self.aabb_min = (np.asarray(aabb_min, np.float32) - np.float32(zero_offset)).astype(np.float32)
        self.aabb_max = (np.asarray(aabb_max, np.float32) + np.float32(zero_offset)).astype(np.float32)
        self.stddev = float(np.float32(bounding_radius) / np.float32(1024.0) * np.float32(surface_offset_scale))
        self.training_step = 0
        n = batch_size
        self.positions = torch.empty((n, 3), dtype=torch.float32, device="cuda")
        self.distances = torch.empty(n, dtype=torch.float32, device="cuda")
        self.positions_shuffled = torch.empty_like(self.positions)
        self.distances_shuffled = torch.empty_like(self.distances)
        self._loss = torch.zeros(1, dtype=torch.float32, device="cuda")

    def generate_training_samples(self, n=None, positions=None, distances=None, stream=None):
        n = n or self.batch_size
        pos = positions if positions is not None else torch.empty((n, 3), dtype=torch.float32, device="cuda")
        dist = distances if distances is not None else torch.empty(n, dtype=torch.float32, device="cuda")
        check(lib().ngp_sdf_generate_training_samples(self.mesh.handle, _stream(stream), n, C.byref(self.rng),
                                                      self.aabb_min.ctypes.data, self.aabb_max.ctypes.data, self.stddev,
                                                      _ptr(pos), _ptr(dist)))
        return pos, dist

    def train_step(self, get_loss=True, regenerate=True, stream=None):
        if regenerate:  # generate_sdf_data_online (training_prep_sdf)
            self.generate_training_samples(self.batch_size, self.positions, self.distances, stream=stream)
        if get_loss:
            self._loss.zero_()
        check(lib().ngp_sdf_train_step(self.trainer.handle, _stream(stream), self.batch_size, _ptr(self.positions),
                                       _ptr(self.distances), self.training_step, _ptr(self.positions_shuffled),
                                       _ptr(self.distances_shuffled), _ptr(self._loss) if get_loss else None))
        self.training_step += 1
        return float(self._loss.item()) if get_loss else None
