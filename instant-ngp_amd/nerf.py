"""Host mirror of the Testbed's NeRF training path (src/testbed_nerf.cu) over the C-ABI.

`NerfTraining` is Testbed::train for a NeRF testbed (training_prep_nerf + train_nerf,
testbed_nerf.cu:3611-3862, 4137-4152); the free functions expose the individual kernels
(generate_training_samples_nerf, compute_loss_kernel_train_nerf, the density-grid update) with
the reference's argument meaning so they can be tested one by one. Every call runs HIP.
"""
import ctypes as C
import json
import math
import os

import numpy as np
import torch

from ._capi import (AdamState, NerfCameraTraining, NerfConfig, NerfErrorCdfs, NerfErrorMapInfo, NerfImage, NerfStats, Rng, check,
                    lib)
from .network import _ptr, _stream, wrap_device

NERF_GRIDSIZE = 128
NERF_CASCADES = 8
N_CELLS = NERF_GRIDSIZE ** 3
BITFIELD_BYTES = N_CELLS // 8 * NERF_CASCADES
ACT = {"None": 0, "ReLU": 1, "Logistic": 2, "Exponential": 3}
LOSS = {"L2": 0, "L1": 1, "MAPE": 2, "SMAPE": 3, "Huber": 4, "LogL1": 5, "RelativeL2": 6}


def default_config(aabb_scale=1.0, **overrides):
    """Testbed NeRF defaults after load_nerf_post (testbed_nerf.cu:3093-3109, testbed.h:716-785)."""
    cfg = NerfConfig()
    check(lib().ngp_nerf_default_config(float(aabb_scale), C.byref(cfg)))
    for k, v in overrides.items():
        if isinstance(getattr(cfg, k), C.Array):
            getattr(cfg, k)[:] = list(v)
        else:
            setattr(cfg, k, v)
    return cfg


def rng_state(state, inc):
    return Rng(state, inc)


def pcg32(seed, seq=1):
    """tcnn::pcg32(initstate, initseq) seeding (pcg32.h), host side."""
    mask = (1 << 64) - 1
    mult = 0x5851F42D4C957F2D
    inc = ((seq << 1) | 1) & mask
    state = 0
    state = (state * mult + inc) & mask
    state = (state + seed) & mask
    state = (state * mult + inc) & mask
    return Rng(state, inc)


def nerf_matrix_to_ngp(m, scale=0.33, offset=(0.5, 0.5, 0.5)):
    """NerfDataset::nerf_matrix_to_ngp (nerf_loader.h:120-140), non-mitsuba branch.
    m: 3x4 (or 4x4) camera-to-world in the NeRF/Blender convention. Returns the 12 floats of the
    column-major mat4x3 the engine takes."""
    m = np.asarray(m, dtype=np.float32)[:3, :4].copy()
    m[:, 1] *= -1.0
    m[:, 2] *= -1.0
    m[:, 3] = m[:, 3] * np.float32(scale) + np.asarray(offset, np.float32)
    m = m[[1, 2, 0], :]  # cycle axes xyz <- yzx
    return np.ascontiguousarray(m.T).reshape(12)


LENS_PERSPECTIVE, LENS_OPENCV, LENS_OPENCV_FISHEYE = 0, 1, 2


def make_image(width, height, xform12, focal=None, camera_angle_x=None, principal=(0.5, 0.5), lens_mode=LENS_PERSPECTIVE,
               lens_params=(0.0, 0.0, 0.0, 0.0)):
    im = NerfImage()
    im.width, im.height = width, height
    if focal is None:
        f = 0.5 * width / math.tan(0.5 * camera_angle_x)  # nerf_loader.cu: fl from camera_angle_x
        focal = (f, f)
    im.focal_length[:] = list(focal)
    im.principal_point[:] = list(principal)
    im.xform[:] = [float(v) for v in xform12]
    im.lens_mode = int(lens_mode)
    im.lens_params[:] = [float(v) for v in lens_params]
    return im


IMAGE_BYTE, IMAGE_HALF, IMAGE_FLOAT = 1, 2, 3  # EImageDataType (NGP_IMAGE_*)
_IMAGE_TYPE = {np.dtype(np.uint8): IMAGE_BYTE, np.dtype(np.float16): IMAGE_HALF, np.dtype(np.float32): IMAGE_FLOAT}
_IMAGE_DTYPE = {IMAGE_BYTE: np.uint8, IMAGE_HALF: np.float16, IMAGE_FLOAT: np.float32}


def _image_array(im, px):
    """px as a contiguous [h, w, 4] array of one of the three texel types, and that type."""
    px = np.asarray(px)
    if px.dtype not in _IMAGE_TYPE:
        raise ValueError(f"training image: uint8, float16 or float32, not {px.dtype}")
    if px.shape != (im.height, im.width, 4):
        raise ValueError(f"image buffer shape {px.shape} != {(im.height, im.width, 4)}")
    return np.ascontiguousarray(px), _IMAGE_TYPE[px.dtype]


class NerfDataset:
    """Training images + cameras on the device. Each image is a [h, w, 4] array: uint8 is RGBA8 sRGB with straight alpha
    (EImageDataType::Byte), float16 and float32 are linear premultiplied RGBA (Half, Float) which the loss pass uses as
    they are; the three may be mixed. A red < 0 in a Half or Float texel masks the pixel, as 0x00FF00FF does in a Byte
    one."""

    def __init__(self, images, pixels):
        if len(images) != len(pixels) or not images:
            raise ValueError("need one RGBA array per image")
        arr = (NerfImage * len(images))(*images)
        self.images = list(images)
        if all(np.asarray(px).dtype not in (np.float16, np.float32) for px in pixels):
            pixels = [np.ascontiguousarray(px, dtype=np.uint8) for px in pixels]  # as before: anything castable to bytes
        bufs, types = [], []
        for im, px in zip(images, pixels):
            px, t = _image_array(im, px)
            bufs.append(px)
            types.append(t)
        ptrs = (C.c_void_p * len(bufs))(*[b.ctypes.data for b in bufs])
        h = C.c_void_p()
        if all(t == IMAGE_BYTE for t in types):
            check(lib().ngp_nerf_dataset_create(len(images), arr, ptrs, C.byref(h)))
        else:
            check(lib().ngp_nerf_dataset_create_typed(len(images), arr, ptrs, (C.c_uint32 * len(types))(*types), C.byref(h)))
        self.handle = h
        self.image_types = types

    @property
    def is_hdr(self):
        """NerfDataset::is_hdr: an image is Half or Float."""
        return any(t != IMAGE_BYTE for t in self.image_types)

    def set_image(self, i, array):
        """Replaces image i's colours (NerfDataset::set_training_image's colour part) by a uint8, float16 or float32
        [h, w, 4] array at the image's resolution; the type may change. Waits for the device; a trainer of this dataset
        discards the sampler it launched ahead."""
        if not 0 <= int(i) < len(self.images):
            raise IndexError(f"image {i} of {len(self.images)}")
        im = self.images[i]
        px, t = _image_array(im, array)
        check(lib().ngp_nerf_dataset_set_image(self.handle, int(i), px.ctypes.data, t, im.width, im.height))
        self.image_types[i] = t

    def image(self, i):
        """Image i's texels as stored: [h, w, 4] uint8, float16 or float32."""
        if not 0 <= int(i) < len(self.images):
            raise IndexError(f"image {i} of {len(self.images)}")
        im, t = self.images[i], C.c_uint32(0)
        check(lib().ngp_nerf_dataset_image(self.handle, int(i), None, 0, C.byref(t)))
        out = np.zeros((im.height, im.width, 4), _IMAGE_DTYPE[t.value])
        check(lib().ngp_nerf_dataset_image(self.handle, int(i), out.ctypes.data, out.nbytes, C.byref(t)))
        return out

    def __len__(self):
        return len(self.images)

    def set_depth(self, i, array, scale=1.0):
        """Image i's depth image (NerfDataset::set_training_image's depth part): a uint16 or float32 array [h, w]; the
        device keeps float32(pixel) * float32(scale). None or scale <= 0 stores zeros (no depth anywhere in the image);
        None with a negative scale removes the image's depth."""
        im = self.images[i]
        if array is None:
            check(lib().ngp_nerf_dataset_set_depth(self.handle, int(i), None, 0, float(scale)))
            return
        a = np.asarray(array)
        if a.dtype not in (np.uint16, np.float32):
            raise ValueError(f"depth image: uint16 or float32, not {a.dtype}")
        if a.shape != (im.height, im.width):
            raise ValueError(f"depth image shape {a.shape} != {(im.height, im.width)}")
        a = np.ascontiguousarray(a)
        check(lib().ngp_nerf_dataset_set_depth(self.handle, int(i), a.ctypes.data, 0 if a.dtype == np.uint16 else 1, float(scale)))

    def depth(self, i):
        """Image i's depth as stored, float32 [h, w], or None when the image has none."""
        im = self.images[i]
        out, has = np.zeros((im.height, im.width), np.float32), C.c_int32(0)
        check(lib().ngp_nerf_dataset_depth(self.handle, int(i), out.ctypes.data, out.size, C.byref(has)))
        return out if has.value else None

    def __del__(self):
        h = getattr(self, "handle", None)
        if h:
            try:
                lib().ngp_nerf_dataset_destroy(h)
            except Exception:
                pass
            self.handle = None


# ---- kernel-level entry points ------------------------------------------------------------------
def _error_cdfs(cdfs, device, n_images):
    """ngp_nerf_error_cdfs from a dict with any of "cdf_x_cond_y" [n_images, h, w], "cdf_y" [n_images, h] and "cdf_img"
    [n_images] (other keys ignored, so NerfTraining.error_map()'s dict can be passed as it is): float32 numpy arrays
    or tensors, copied to `device` (None: kept on the host, for training_pixels(host=True)). A missing, None or empty
    entry is a null pointer; a first dimension other than n_images is refused (the kernels index by image). Returns
    (struct or None, the arrays it points into)."""
    if cdfs is None:
        return None, ()
    keep, e = [], NerfErrorCdfs()

    def one(name):
        a = cdfs.get(name)
        if a is None or (a.numel() if torch.is_tensor(a) else np.asarray(a).size) == 0:
            return None
        if device is None:
            a = np.ascontiguousarray(a.cpu().numpy() if torch.is_tensor(a) else a, dtype=np.float32)
            keep.append(a)
            return a, a.ctypes.data
        a = torch.as_tensor(a, dtype=torch.float32).to(device).contiguous()
        keep.append(a)
        return a, a.data_ptr()

    x, img = one("cdf_x_cond_y"), one("cdf_img")
    if x is not None:
        y = one("cdf_y")
        if y is None or x[0].ndim != 3 or tuple(y[0].shape) != tuple(x[0].shape[:2]) or x[0].shape[0] != n_images:
            raise ValueError("cdfs: cdf_x_cond_y [n_images, h, w] needs cdf_y [n_images, h]")
        e.cdf_x_cond_y, e.cdf_y, e.width, e.height = x[1], y[1], x[0].shape[2], x[0].shape[1]
    if img is not None:
        if tuple(img[0].shape) != (n_images,):
            raise ValueError("cdfs: cdf_img [n_images]")
        e.cdf_img = img[1]
    return e, keep


def generate_training_samples(ds, cfg, n_rays, rng, max_samples, bitfield, ray_offset=0, n_rays_total=None,
                              stream=None, cdfs=None, distortion=None):
    """generate_training_samples_nerf (testbed_nerf.cu:1382-1658). cdfs: draw the rays' pixels from the error map's
    CDFs (a dict, see _error_cdfs; ngp_nerf_generate_training_samples_cdf). distortion: a lens distortion map, a
    contiguous float32 device tensor [h, w, 2], whose offset at the ray's uv is added to dir.xy after the lens
    (ngp_nerf_generate_training_samples_distortion)."""
    dev = bitfield.device
    out = {
        "ray_indices": torch.zeros(n_rays, dtype=torch.int32, device=dev),
        "rays": torch.zeros((n_rays, 6), dtype=torch.float32, device=dev),
        "numsteps": torch.zeros((n_rays, 2), dtype=torch.int32, device=dev),
        "coords": torch.zeros((max_samples, 7), dtype=torch.float32, device=dev),
        "counters": torch.zeros(2, dtype=torch.int32, device=dev),
    }
    args = (ds.handle, C.byref(cfg), _stream(stream), n_rays, ray_offset, n_rays_total or n_rays, rng, max_samples,
            _ptr(bitfield), _ptr(out["ray_indices"]), _ptr(out["rays"]), _ptr(out["numsteps"]), _ptr(out["coords"]),
            _ptr(out["counters"]))
    if distortion is not None:
        _check_distortion_map(distortion, dev, "generate_training_samples")
        e, keep = _error_cdfs(cdfs, dev, len(ds))
        check(lib().ngp_nerf_generate_training_samples_distortion(*args, C.byref(e) if e is not None else None,
                                                                  _ptr(distortion), distortion.shape[1], distortion.shape[0]))
        torch.cuda.synchronize(dev)  # the kernels read `keep`
    elif cdfs is None:
        check(lib().ngp_nerf_generate_training_samples(*args))
    else:
        e, keep = _error_cdfs(cdfs, dev, len(ds))
        check(lib().ngp_nerf_generate_training_samples_cdf(*args, C.byref(e)))
        torch.cuda.synchronize(dev)  # the kernels read `keep`
    return out


def training_pixels(ds, cfg, n_rays, rng, cdfs=None, ray_offset=0, n_rays_total=None, host=False, stream=None):
    """The training pixel of rays [ray_offset, ray_offset + n_rays) of a batch of n_rays_total, as the sampler and the
    loss pass draw it: {"img" [n], "uv" [n, 2] after snapping, "pdf" [n, 2] = (img_pdf, uv_pdf)}. Device tensors from
    ngp_nerf_training_pixels; host=True: numpy arrays from ngp_nerf_training_pixels_host, the same function compiled
    for the host (no GPU call; ds may then be a list of NerfImage instead of a NerfDataset)."""
    if host:
        images = list(ds.images if isinstance(ds, NerfDataset) else ds)
        arr = (NerfImage * len(images))(*images)
        e, keep = _error_cdfs(cdfs, None, len(images))
        out = {"img": np.zeros(n_rays, np.uint32), "uv": np.zeros((n_rays, 2), np.float32),
               "pdf": np.zeros((n_rays, 2), np.float32)}
        check(lib().ngp_nerf_training_pixels_host(len(images), arr, C.byref(cfg), n_rays, ray_offset, n_rays_total or n_rays,
                                                  rng, C.byref(e) if e is not None else None, out["img"].ctypes.data,
                                                  out["uv"].ctypes.data, out["pdf"].ctypes.data))
        del keep
        return out
    dev = torch.device("cuda")
    e, keep = _error_cdfs(cdfs, dev, len(ds))
    out = {"img": torch.zeros(n_rays, dtype=torch.int32, device=dev),
           "uv": torch.zeros((n_rays, 2), dtype=torch.float32, device=dev),
           "pdf": torch.zeros((n_rays, 2), dtype=torch.float32, device=dev)}
    check(lib().ngp_nerf_training_pixels(ds.handle, C.byref(cfg), _stream(stream), n_rays, ray_offset, n_rays_total or n_rays,
                                         rng, C.byref(e) if e is not None else None, _ptr(out["img"]), _ptr(out["uv"]),
                                         _ptr(out["pdf"])))
    torch.cuda.synchronize(dev)  # the kernel reads `keep`
    return out


def compute_loss(ds, cfg, n_rays, rng, max_compacted, samples, network_output, mean_density, loss_scale=128.0,
                 n_rays_total=None, stream=None, error_map=None, keep_state=False, state_capacity=None, cdfs=None,
                 envmap=None, envmap_gradient=None, envmap_loss=None, depth_lambda=0.0, depth_loss="L1", depth_entry=None,
                 exposure=None, exposure_gradient=None, exposure_entry=None):
    """compute_loss_kernel_train_nerf (testbed_nerf.cu:1660-2012). `samples` is the dict returned by
    generate_training_samples (its numsteps is rewritten to the compacted {n, base}). error_map: a
    float32 device tensor [n_images, h, w] the compacted rays' losses are added into (:1869-1899).
    keep_state: pass 1 keeps each composited sample's state for pass 2 (ngp_nerf_compute_loss_state, the
    training step's form; same outputs bit for bit). state_capacity: samples the kept state holds (default: every
    sample slot); rays reaching past it are composited again by pass 2, with the same result. cdfs: the CDFs the
    samples' pixels were drawn from (generate_training_samples(cdfs=)): loss and the error map deposit are divided by
    the pixels' pdf, dL/doutput is not (ngp_nerf_compute_loss_cdf; that entry point has no keep_state form).
    envmap: a contiguous float32 device tensor [h, w, 4], the environment map behind every ray (testbed_nerf.cu:1781-1792;
    ngp_nerf_compute_loss_envmap, on its own: no error_map, keep_state or cdfs). envmap_gradient: a tensor of the same
    shape that is overwritten with the map's gradient (:1988-2011, an exact sum: the same bits in every run);
    envmap_loss: the gradient's loss name or number (default: cfg.loss_type).
    depth_lambda, depth_loss: depth supervision (testbed_nerf.cu:1848-1856, 1952-1956) against the dataset's depth images
    (NerfDataset.set_depth) with the loss of that name or number. With depth_lambda > 0 (or depth_entry=True) the call
    goes through ngp_nerf_compute_loss_depth, which takes error_map, cdfs, envmap and keep_state in any combination
    (the kept state then has six planes); with depth_lambda 0 that entry point gives the others' bits.
    exposure: a contiguous float32 device tensor [n_images, 3], the images' log2 exposures per channel: the target's
    texel is scaled by 2^exposure (testbed_nerf.cu:1794-1818). exposure_gradient: a tensor of the same shape the
    per-image sums of the rays' dloss_by_dexposure (:1973-1986) are ADDED onto, without atomics (the same bits in every
    run). With exposure given (or exposure_entry=True) the call goes through ngp_nerf_compute_loss_exposure, which takes
    everything the depth entry point takes; with exposure None it gives that entry point's bits."""
    dev = network_output.device
    # the kernel reads one output row per sample; samples never exceed the sampler's coords buffer
    if network_output.shape[0] < samples["coords"].shape[0]:
        raise ValueError(f"network_output has {network_output.shape[0]} rows, fewer than the {samples['coords'].shape[0]} "
                         "sample slots of generate_training_samples")
    out = {
        "coords_compacted": torch.zeros((max_compacted, 7), dtype=torch.float32, device=dev),
        "dloss_doutput": torch.zeros((max_compacted, 16), dtype=torch.float16, device=dev),
        "loss": torch.zeros(n_rays, dtype=torch.float32, device=dev),
        "compacted_counter": torch.zeros(1, dtype=torch.int32, device=dev),
    }
    args = (ds.handle, C.byref(cfg), _stream(stream), n_rays, n_rays_total or n_rays, rng, max_compacted,
            _ptr(samples["counters"]), _ptr(network_output), _ptr(samples["ray_indices"]), _ptr(samples["rays"]),
            _ptr(samples["numsteps"]), _ptr(samples["coords"]), _ptr(out["coords_compacted"]), _ptr(out["dloss_doutput"]),
            _ptr(out["loss"]), _ptr(out["compacted_counter"]), _ptr(mean_density), float(loss_scale))
    if error_map is not None and (error_map.dtype != torch.float32 or error_map.dim() != 3 or not error_map.is_contiguous()):
        raise ValueError("error_map: a contiguous float32 tensor [n_images, h, w]")
    if envmap is None and envmap_gradient is not None:
        raise ValueError("envmap_gradient: needs envmap")
    if exposure is None and exposure_gradient is not None:
        raise ValueError("exposure_gradient: needs exposure")
    for t in (exposure, exposure_gradient):
        if t is not None and (t.dtype != torch.float32 or tuple(t.shape) != (len(ds), 3) or not t.is_contiguous() or t.device != dev):
            raise ValueError("exposure / exposure_gradient: contiguous float32 device tensors [n_images, 3]")
    through_exposure = exposure is not None if exposure_entry is None else bool(exposure_entry)
    if exposure is not None and not through_exposure:
        raise ValueError("exposure: only ngp_nerf_compute_loss_exposure takes it (exposure_entry=False)")
    if through_exposure or ((depth_lambda > 0) if depth_entry is None else depth_entry):
        for t in (envmap, envmap_gradient):
            if t is not None and (t.dtype != torch.float32 or t.dim() != 3 or t.shape[2] != 4 or not t.is_contiguous()
                                  or t.shape != envmap.shape or t.device != dev):
                raise ValueError("envmap / envmap_gradient: contiguous float32 device tensors [h, w, 4] of one shape")
        e, keep = _error_cdfs(cdfs, dev, len(ds))
        em = (_ptr(error_map), error_map.shape[2], error_map.shape[1]) if error_map is not None else (None, 0, 0)
        lt = cfg.loss_type if envmap_loss is None else (LOSS[envmap_loss] if isinstance(envmap_loss, str) else int(envmap_loss))
        env = (_ptr(envmap), envmap.shape[1], envmap.shape[0], lt, _ptr(envmap_gradient)) if envmap is not None else (None, 0, 0, 0, None)
        cap = (samples["coords"].shape[0] if state_capacity is None else int(state_capacity)) if keep_state else 0
        state = torch.empty((6, cap), dtype=torch.float32, device=dev) if keep_state else None
        dl = LOSS[depth_loss] if isinstance(depth_loss, str) else int(depth_loss)
        if through_exposure:
            check(lib().ngp_nerf_compute_loss_exposure(*args, *em, C.byref(e) if e is not None else None, *env, _ptr(state),
                                                       cap, float(depth_lambda), dl, _ptr(exposure), _ptr(exposure_gradient)))
        else:
            check(lib().ngp_nerf_compute_loss_depth(*args, *em, C.byref(e) if e is not None else None, *env, _ptr(state), cap,
                                                    float(depth_lambda), dl))
        torch.cuda.synchronize(dev)  # the kernels read `keep` and `state`
    elif envmap is not None:
        if error_map is not None or keep_state or cdfs is not None:
            raise ValueError("envmap: without error_map, keep_state and cdfs (the C-ABI form takes none of them)")
        for t in (envmap, envmap_gradient):
            if t is not None and (t.dtype != torch.float32 or t.dim() != 3 or t.shape[2] != 4 or not t.is_contiguous()
                                  or t.shape != envmap.shape or t.device != dev):
                raise ValueError("envmap / envmap_gradient: contiguous float32 device tensors [h, w, 4] of one shape")
        lt = cfg.loss_type if envmap_loss is None else (LOSS[envmap_loss] if isinstance(envmap_loss, str) else int(envmap_loss))
        check(lib().ngp_nerf_compute_loss_envmap(*args, _ptr(envmap), envmap.shape[1], envmap.shape[0], lt,
                                                 _ptr(envmap_gradient)))
    elif cdfs is not None:
        if keep_state:
            raise ValueError("cdfs: without keep_state (the C-ABI form has no sample-state argument)")
        e, keep = _error_cdfs(cdfs, dev, len(ds))
        em = (_ptr(error_map), error_map.shape[2], error_map.shape[1]) if error_map is not None else (None, 0, 0)
        check(lib().ngp_nerf_compute_loss_cdf(*args, *em, C.byref(e)))
        torch.cuda.synchronize(dev)  # the kernels read `keep`
    elif keep_state:
        if error_map is not None:
            raise ValueError("keep_state: without error_map (the C-ABI form has no error-map argument)")
        cap = samples["coords"].shape[0] if state_capacity is None else int(state_capacity)
        state = torch.empty((5, cap), dtype=torch.float32, device=dev)
        check(lib().ngp_nerf_compute_loss_state(*args, _ptr(state), cap))
    elif error_map is None:
        check(lib().ngp_nerf_compute_loss(*args))
    else:
        check(lib().ngp_nerf_compute_loss_error_map(*args, _ptr(error_map), error_map.shape[2], error_map.shape[1]))
    return out


# ---- environment map ----------------------------------------------------------------------------
def envmap_lookup(width, height, dirs, host=False, stream=None):
    """The four texels and bilinear weights of normalized directions in a width x height environment map, as the read
    and the gradient deposit derive them (envmap.cuh:29-35, 59-64): (texels [n, 4] int64 indices x + y * width in the
    order (x, y), (x+1, y), (x, y+1), (x+1, y+1), weights [n, 4] float32). dirs: [n, 3] float32; a device tensor
    (ngp_envmap_lookup) or, host=True, a numpy array (ngp_envmap_lookup_host: the same function compiled for the host,
    no GPU call). The two agree to the rounding of acos / atan2, not to the bit."""
    if host:
        d = np.ascontiguousarray(dirs, dtype=np.float32).reshape(-1, 3)
        tex, wt = np.zeros((d.shape[0], 4), np.uint32), np.zeros((d.shape[0], 4), np.float32)
        check(lib().ngp_envmap_lookup_host(int(width), int(height), d.shape[0], d.ctypes.data, tex.ctypes.data, wt.ctypes.data))
        return tex.astype(np.int64), wt
    d = dirs.to(torch.float32).contiguous().view(-1, 3)
    tex = torch.zeros((d.shape[0], 4), dtype=torch.int32, device=d.device)
    wt = torch.zeros((d.shape[0], 4), dtype=torch.float32, device=d.device)
    check(lib().ngp_envmap_lookup(_stream(stream), int(width), int(height), d.shape[0], _ptr(d), _ptr(tex), _ptr(wt)))
    return tex.to(torch.int64), wt


def envmap_deposit(width, height, dirs, values, stream=None):
    """deposit_envmap_gradient (envmap.cuh:57-94) of fp16 rgb values [n, 3] along directions [n, 3], as the loss pass
    does it (ngp_envmap_deposit): the gradient image [height, width, 4] float32, each channel the exact sum of its
    fp16 contributions rounded once; alpha stays zero. Device tensors."""
    d = dirs.to(torch.float32).contiguous().view(-1, 3)
    v = values.to(torch.float16).contiguous().view(-1, 3)
    if v.shape[0] != d.shape[0] or v.device != d.device:
        raise ValueError("envmap_deposit: one fp16 rgb value per direction, on the directions' device")
    g = torch.empty((int(height), int(width), 4), dtype=torch.float32, device=d.device)
    check(lib().ngp_envmap_deposit(_stream(stream), int(width), int(height), d.shape[0], _ptr(d), _ptr(v), _ptr(g)))
    return g


def envmap_optimizer_step(optimizer, step, state, gradient, loss_scale=128.0, stream=None):
    """One step of the map's optimizer chain (ngp_envmap_optimizer_step; tcnn Trainer<float, float, float>): optimizer
    is the chain's config dict, step the steps taken before, state a dict of float32 device tensors of one size
    ("params", "first_moments", "second_moments", "ema", "ema_params") and "param_steps" (int32), updated in place."""
    n = state["params"].numel()
    for k in ("params", "first_moments", "second_moments", "ema", "ema_params", "param_steps"):
        t = state[k]
        want = torch.int32 if k == "param_steps" else torch.float32
        if t.dtype != want or t.numel() != n or not t.is_contiguous():
            raise ValueError(f"envmap_optimizer_step: state[{k!r}] is a contiguous {want} tensor of {n} elements")
    g = gradient.to(torch.float32).contiguous()
    if g.numel() != n:
        raise ValueError("envmap_optimizer_step: one gradient per parameter")
    check(lib().ngp_envmap_optimizer_step(_stream(stream), json.dumps(optimizer).encode(), int(step), float(loss_scale), n,
                                          _ptr(state["params"]), _ptr(g), _ptr(state["first_moments"]),
                                          _ptr(state["second_moments"]), _ptr(state["param_steps"]), _ptr(state["ema"]),
                                          _ptr(state["ema_params"])))


def fill_rollover(data, n_input, rescale=False, stream=None):
    """tcnn fill_rollover / fill_rollover_and_rescale over the rows of a 2D tensor (testbed_nerf.cu:4061-4069)."""
    dtype = {torch.float32: 0, torch.float16: 1}[data.dtype]
    check(lib().ngp_nerf_fill_rollover(_stream(stream), data.shape[0], data.shape[1], _ptr(n_input), _ptr(data), dtype,
                                       int(rescale)))


def grid_generate_samples(cfg, n, rng, step, grid, n_cascades, thresh, stream=None):
    """generate_grid_samples_nerf_nonuniform (testbed_nerf.cu:635-676)."""
    pos = torch.zeros((n, 3), dtype=torch.float32, device=grid.device)
    idx = torch.zeros(n, dtype=torch.int32, device=grid.device)
    check(lib().ngp_nerf_grid_generate_samples(_stream(stream), C.byref(cfg), n, rng, step, _ptr(grid), n_cascades,
                                               float(thresh), _ptr(pos), _ptr(idx)))
    return pos, idx


def grid_splat_max(indices, density_out, density_activation, grid_tmp, stream=None, binned=False):
    """splat_grid_samples_nerf_max_nearest_neighbor (testbed_nerf.cu:678-702). density_out: the density
    network's fp16 output, row-major [16 x n] (feature-major), density in row 0. binned: the memset of grid_tmp
    and the splat in one call (ngp_nerf_grid_splat_max_cells, a counting sort by cell bin): grid_tmp is
    overwritten, every cell of it."""
    if binned:
        check(lib().ngp_nerf_grid_splat_max_cells(_stream(stream), indices.shape[0], _ptr(indices), _ptr(density_out),
                                                  density_activation, _ptr(grid_tmp), grid_tmp.numel()))
        return
    check(lib().ngp_nerf_grid_splat_max(_stream(stream), indices.shape[0], _ptr(indices), _ptr(density_out),
                                        density_activation, _ptr(grid_tmp)))


def grid_ema(decay, grid, grid_tmp, stream=None):
    """ema_grid_samples_nerf (testbed_nerf.cu:731-754)."""
    check(lib().ngp_nerf_grid_ema(_stream(stream), grid.numel(), float(decay), _ptr(grid), _ptr(grid_tmp)))


def grid_mean_and_bitfield(grid, max_cascade, stream=None):
    """update_density_grid_mean_and_bitfield (testbed_nerf.cu:3538-3567)."""
    mean = torch.zeros(1 + 512, dtype=torch.float32, device=grid.device)
    bf = torch.zeros(BITFIELD_BYTES, dtype=torch.uint8, device=grid.device)
    check(lib().ngp_nerf_grid_mean_and_bitfield(_stream(stream), _ptr(grid), max_cascade, _ptr(mean), _ptr(bf)))
    return mean, bf


# ---- lens distortion map ------------------------------------------------------------------------
def _check_distortion_map(m, device, who):
    if not torch.is_tensor(m) or m.dtype != torch.float32 or m.dim() != 3 or m.shape[2] != 2 or not m.is_contiguous() \
            or (device is not None and m.device != device):
        raise ValueError(f"{who}: the distortion map is a contiguous float32 device tensor [h, w, 2]")


def distortion_lookup(width, height, uv, map=None, host=False, stream=None):
    """The four texels and bilinear weights of positions uv [n, 2] in a width x height lens distortion map, as
    Buffer2DView::at_lerp (common.h:384-400) and deposit_image_gradient (common_device.cuh:124-156) both derive them:
    (texels [n, 4] int64 indices x + y * width in the order (x, y), (x+1, y), (x, y+1), (x+1, y+1), each clamped into the
    map, weights [n, 4] float32); with map ([height, width, 2] float32) also the mixed offsets [n, 2]. uv is folded into
    [0, 2] with NaN to 0 first. Device tensors (ngp_nerf_distortion_lookup) or, host=True, numpy arrays
    (ngp_nerf_distortion_lookup_host: the same function compiled for the host, no GPU call); the two agree bit for bit."""
    if host:
        u = np.ascontiguousarray(uv, dtype=np.float32).reshape(-1, 2)
        tex, wt = np.zeros((u.shape[0], 4), np.uint32), np.zeros((u.shape[0], 4), np.float32)
        m = off = None
        if map is not None:
            m = np.ascontiguousarray(map, dtype=np.float32)
            if m.shape != (int(height), int(width), 2):
                raise ValueError("distortion_lookup: map is [height, width, 2]")
            off = np.zeros((u.shape[0], 2), np.float32)
        check(lib().ngp_nerf_distortion_lookup_host(int(width), int(height), u.shape[0], u.ctypes.data, tex.ctypes.data,
                                                    wt.ctypes.data, m.ctypes.data if m is not None else None,
                                                    off.ctypes.data if off is not None else None))
        return (tex.astype(np.int64), wt) if map is None else (tex.astype(np.int64), wt, off)
    u = uv.to(torch.float32).contiguous().view(-1, 2)
    tex = torch.zeros((u.shape[0], 4), dtype=torch.int32, device=u.device)
    wt = torch.zeros((u.shape[0], 4), dtype=torch.float32, device=u.device)
    off = None
    if map is not None:
        _check_distortion_map(map, u.device, "distortion_lookup")
        if tuple(map.shape) != (int(height), int(width), 2):
            raise ValueError("distortion_lookup: map is [height, width, 2]")
        off = torch.zeros((u.shape[0], 2), dtype=torch.float32, device=u.device)
    check(lib().ngp_nerf_distortion_lookup(_stream(stream), int(width), int(height), u.shape[0], _ptr(u), _ptr(tex), _ptr(wt),
                                           _ptr(map) if map is not None else None, _ptr(off) if off is not None else None))
    return (tex.to(torch.int64), wt) if map is None else (tex.to(torch.int64), wt, off)


def distortion_ray_gradients(cfg, n_rays_total, n_images, samples, coords_compacted, coords_gradient, camera_matrices,
                             pos_gradient=None, rot_gradient=None, stream=None):
    """compute_cam_gradient_train_nerf's distortion branch per ray (testbed_nerf.cu:2088-2099;
    ngp_nerf_distortion_ray_gradients): camera_gradients' arguments plus camera_matrices, float32 [n_images, 3, 3] with
    [i, c, r] the column-major element (column c, row r) of image i's rotation. Returns float32 [n_rays_total, 2]: row r
    of a kept ray r holds (inverse(mat3(xform_img)) * (gd - d dot(gd, d))).xy, zeros for a ray without samples.
    pos_gradient / rot_gradient (both or neither): the per-image pose sums are added onto them as camera_gradients does."""
    for t in (coords_compacted, coords_gradient, camera_matrices) + ((pos_gradient, rot_gradient) if pos_gradient is not None else ()):
        if t is None or t.dtype != torch.float32 or not t.is_contiguous():
            raise ValueError("distortion_ray_gradients: contiguous float32 tensors")
    if (pos_gradient is None) != (rot_gradient is None):
        raise ValueError("distortion_ray_gradients: pos_gradient and rot_gradient, both or neither")
    if camera_matrices.numel() != 9 * n_images:
        raise ValueError("distortion_ray_gradients: camera_matrices are [n_images, 3, 3]")
    if coords_gradient.shape[0] < coords_compacted.shape[0] or coords_compacted.shape[1] != 7:
        raise ValueError("distortion_ray_gradients: one gradient row per compacted coordinate")
    out = torch.zeros((int(n_rays_total), 2), dtype=torch.float32, device=coords_compacted.device)
    check(lib().ngp_nerf_distortion_ray_gradients(
        C.byref(cfg), _stream(stream), int(n_rays_total), int(n_images), _ptr(samples["counters"]),
        _ptr(samples["ray_indices"]), _ptr(samples["rays"]), _ptr(samples["numsteps"]), _ptr(coords_compacted),
        _ptr(coords_gradient), coords_gradient.shape[1], _ptr(pos_gradient) if pos_gradient is not None else None,
        _ptr(rot_gradient) if rot_gradient is not None else None, _ptr(camera_matrices), _ptr(out)))
    return out


DISTORTION_BINS = 16  # 64-bit bins per channel of the distortion map's gradient accumulator; bin b's unit is 2^(16 b - 149)


def distortion_accumulator(width, height, device="cuda"):
    """A zeroed gradient accumulator for a width x height map (ngp_nerf_distortion_accumulator_words int64 words):
    [height * width * 3 * 16] bins, channels sum g.x w, sum g.y w and sum w per texel, then the count of rays dropped
    for a non-finite gradient."""
    n = int(lib().ngp_nerf_distortion_accumulator_words(int(width), int(height)))
    if n == 0:
        raise ValueError("distortion_accumulator: width and height in 1..8192")
    return torch.zeros(n, dtype=torch.int64, device=device)


def distortion_deposit(ds, cfg, n_rays_total, rng, ray_counter, ray_indices, ray_gradients, width, height, accumulator,
                       numsteps=None, stream=None):
    """deposit_image_gradient (common_device.cuh:124-156) of every kept ray's image-plane gradient (ray_gradients,
    float32 [R, 2]) into `accumulator` (distortion_accumulator(); added to its content) at the ray's uv, recomputed from
    its id (ray_indices int32 [R], *ray_counter of them) and rng as the sampler and the loss pass draw it. numsteps
    (int32 [R, 2], optional): rays whose count is 0 deposit nothing. Exact integer sums: independent of arrival order."""
    if accumulator.dtype != torch.int64 or not accumulator.is_contiguous() or \
            accumulator.numel() != int(lib().ngp_nerf_distortion_accumulator_words(int(width), int(height))):
        raise ValueError("distortion_deposit: accumulator from distortion_accumulator(width, height)")
    g = ray_gradients.to(torch.float32).contiguous()
    if g.dim() != 2 or g.shape[1] != 2 or g.shape[0] < ray_indices.numel():
        raise ValueError("distortion_deposit: ray_gradients are [R, 2], one row per ray index")
    if ray_indices.numel() < min(int(n_rays_total), int(ray_counter.reshape(-1)[0])):
        raise ValueError("distortion_deposit: fewer ray indices than the ray counter says")
    if numsteps is not None and numsteps.numel() < 2 * ray_indices.numel():
        raise ValueError("distortion_deposit: numsteps are [R, 2]")
    check(lib().ngp_nerf_distortion_deposit(ds.handle, C.byref(cfg), _stream(stream), int(n_rays_total), rng, _ptr(ray_counter),
                                            _ptr(ray_indices), _ptr(numsteps) if numsteps is not None else None, _ptr(g),
                                            int(width), int(height), _ptr(accumulator)))
    torch.cuda.synchronize(accumulator.device)  # the kernel reads `g`


def distortion_gradient(width, height, accumulator, stream=None):
    """safe_divide of the accumulated gradient by the accumulated weight (testbed_nerf.cu:3811-3816;
    ngp_nerf_distortion_gradient): float32 [height, width, 2], 0 where no weight arrived."""
    if accumulator.dtype != torch.int64 or not accumulator.is_contiguous() or \
            accumulator.numel() != int(lib().ngp_nerf_distortion_accumulator_words(int(width), int(height))):
        raise ValueError("distortion_gradient: accumulator from distortion_accumulator(width, height)")
    g = torch.empty((int(height), int(width), 2), dtype=torch.float32, device=accumulator.device)
    check(lib().ngp_nerf_distortion_gradient(_stream(stream), int(width), int(height), _ptr(accumulator), _ptr(g)))
    return g


# ---- camera pose refinement ---------------------------------------------------------------------
def camera_gradients(cfg, n_rays_total, n_images, samples, coords_compacted, coords_gradient, pos_gradient, rot_gradient,
                     stream=None):
    """compute_cam_gradient_train_nerf (testbed_nerf.cu:2014-2123), extrinsics only, without float atomics: the per-image
    sums of the compacted batch's input gradient are ADDED onto pos_gradient / rot_gradient (float32 [n_images, 3]).
    samples: the dict of generate_training_samples after compute_loss rewrote its numsteps (counters[0]: rays kept);
    coords_gradient: float32 [B, stride >= 7] (rows 0..2 position, 4..6 direction)."""
    for t in (coords_compacted, coords_gradient, pos_gradient, rot_gradient):
        if t.dtype != torch.float32 or not t.is_contiguous():
            raise ValueError("camera_gradients: contiguous float32 tensors")
    if pos_gradient.numel() != 3 * n_images or rot_gradient.numel() != 3 * n_images:
        raise ValueError("camera_gradients: pos_gradient / rot_gradient are [n_images, 3]")
    if coords_gradient.shape[0] < coords_compacted.shape[0] or coords_compacted.shape[1] != 7:
        raise ValueError("camera_gradients: one gradient row per compacted coordinate")
    check(lib().ngp_nerf_camera_gradients(
        C.byref(cfg), _stream(stream), int(n_rays_total), int(n_images), _ptr(samples["counters"]),
        _ptr(samples["ray_indices"]), _ptr(samples["rays"]), _ptr(samples["numsteps"]), _ptr(coords_compacted),
        _ptr(coords_gradient), coords_gradient.shape[1], _ptr(pos_gradient), _ptr(rot_gradient)))


def _adam_dict(s):
    return {"iter": int(s.iter), "first_moment": np.array(s.first_moment[:], np.float32),
            "second_moment": np.array(s.second_moment[:], np.float32), "variable": np.array(s.variable[:], np.float32),
            "learning_rate": float(s.learning_rate), "epsilon": float(s.epsilon), "beta1": float(s.beta1),
            "beta2": float(s.beta2)}


def _adam_struct(d):
    s = AdamState()
    s.iter = int(d["iter"])
    for k in ("first_moment", "second_moment", "variable"):
        getattr(s, k)[:] = [float(v) for v in d[k]]
    for k in ("learning_rate", "epsilon", "beta1", "beta2"):
        setattr(s, k, float(d[k]))
    return s


def _f3(v):
    return np.ascontiguousarray(np.asarray(v, np.float32).reshape(3))


def pose_apply(xform12, rot_offset, pos_offset):
    """Training::update_transforms for one image (testbed_nerf.cu:2998-3019). Host only."""
    x = np.ascontiguousarray(np.asarray(xform12, np.float32).reshape(12))
    r, p, out = _f3(rot_offset), _f3(pos_offset), np.zeros(12, np.float32)
    check(lib().ngp_pose_apply(x.ctypes.data, r.ctypes.data, p.ctypes.data, out.ctypes.data))
    return out


def pose_compose_rotation(a, b):
    """rotvec(rotmat(a) * rotmat(b)) (common_device.cuh:698-722). Host only."""
    a, b, out = _f3(a), _f3(b), np.zeros(3, np.float32)
    check(lib().ngp_pose_compose_rotation(a.ctypes.data, b.ctypes.data, out.ctypes.data))
    return out


class PoseOptimizer:
    """n_images pairs of (AdamOptimizer<vec3>, RotationAdamOptimizer) (adam_optimizer.h:128-309) with the update rule
    of Testbed::train_nerf (testbed_nerf.cu:3784-3805). Host only: no GPU call."""

    def __init__(self, n_images):
        h = C.c_void_p()
        check(lib().ngp_pose_optimizer_create(int(n_images), C.byref(h)))
        self.handle, self.n_images = h, int(n_images)

    def step(self, pos_grad, rot_grad, n_steps_between=16, extrinsic_lr=1e-3, l2_reg=1e-4, network_lr=1e-2):
        pg = np.ascontiguousarray(np.asarray(pos_grad, np.float32).reshape(self.n_images, 3))
        rg = np.ascontiguousarray(np.asarray(rot_grad, np.float32).reshape(self.n_images, 3))
        check(lib().ngp_pose_optimizer_step(self.handle, pg.ctypes.data, rg.ctypes.data, int(n_steps_between),
                                            float(extrinsic_lr), float(l2_reg), float(network_lr)))

    def get(self, i):
        """(position state, rotation state) of camera i as dicts."""
        p, r = AdamState(), AdamState()
        check(lib().ngp_pose_optimizer_get(self.handle, int(i), C.byref(p), C.byref(r)))
        return _adam_dict(p), _adam_dict(r)

    def set_state(self, i, pos=None, rot=None):
        ps = _adam_struct(pos) if pos is not None else None
        rs = _adam_struct(rot) if rot is not None else None
        check(lib().ngp_pose_optimizer_set_state(self.handle, int(i), C.byref(ps) if ps else None,
                                                 C.byref(rs) if rs else None))

    def reset(self):
        check(lib().ngp_pose_optimizer_reset(self.handle))

    def reset_one(self, i):
        check(lib().ngp_pose_optimizer_reset_one(self.handle, int(i)))

    def __del__(self):
        h = getattr(self, "handle", None)
        if h:
            try:
                lib().ngp_pose_optimizer_destroy(h)
            except Exception:
                pass
            self.handle = None


class ExposureOptimizer:
    """n_images AdamOptimizer<vec3> (Training::cam_exposure) with the update rule of Testbed::train_nerf
    (testbed_nerf.cu:3831-3858), the mean subtraction included. Host only: no GPU call."""

    def __init__(self, n_images):
        h = C.c_void_p()
        check(lib().ngp_exposure_optimizer_create(int(n_images), C.byref(h)))
        self.handle, self.n_images = h, int(n_images)

    def step(self, grad, n_steps_between=16, l2_reg=0.0, network_lr=1e-2):
        g = np.ascontiguousarray(np.asarray(grad, np.float32).reshape(self.n_images, 3))
        check(lib().ngp_exposure_optimizer_step(self.handle, g.ctypes.data, int(n_steps_between), float(l2_reg), float(network_lr)))

    def get(self, i):
        e = AdamState()
        check(lib().ngp_exposure_optimizer_get(self.handle, int(i), C.byref(e)))
        return _adam_dict(e)

    def set_state(self, i, state):
        st = _adam_struct(state)
        check(lib().ngp_exposure_optimizer_set_state(self.handle, int(i), C.byref(st)))

    def reset(self):
        check(lib().ngp_exposure_optimizer_reset(self.handle))

    def reset_one(self, i):
        check(lib().ngp_exposure_optimizer_reset_one(self.handle, int(i)))

    def __del__(self):
        h = getattr(self, "handle", None)
        if h:
            try:
                lib().ngp_exposure_optimizer_destroy(h)
            except Exception:
                pass
            self.handle = None


# ---- Testbed-level training -------------------------------------------------------------------
class NerfTraining:
    """Testbed::train for NeRF: density-grid update + one training step per call (testbed.cu:4285-4370)."""

    def __init__(self, network, trainer, dataset, cfg=None, seed=1337):
        self.network, self.trainer, self.dataset = network, trainer, dataset
        self.cfg = cfg if cfg is not None else default_config()
        h = C.c_void_p()
        check(lib().ngp_nerf_trainer_create(network.handle, trainer.handle, dataset.handle, C.byref(self.cfg), seed,
                                            C.byref(h)))
        self.handle = h

    def _buffers(self, write=False):
        # reads keep a prelaunched (pipelined) sampler: it reads only the bitfield and writes none of the
        # three buffers. ngp_nerf_trainer_buffers (write=True) discards it, so writes through the returned
        # views are seen by the next step's sampling
        g, b, m = C.c_void_p(), C.c_void_p(), C.c_void_p()
        fn = lib().ngp_nerf_trainer_buffers if write else lib().ngp_nerf_trainer_buffers_read
        check(fn(self.handle, C.byref(g), C.byref(b), C.byref(m)))
        return g.value, b.value, m.value

    def _views(self, write):
        g, b, m = self._buffers(write)
        return (wrap_device(g, N_CELLS * (self.cfg.max_cascade + 1), torch.float32),
                wrap_device(b, BITFIELD_BYTES // 4, torch.float32).view(torch.uint8),
                wrap_device(m, 1, torch.float32))

    @property
    def density_grid(self):
        """fp32 [128^3 x (max_cascade + 1)] (testbed_nerf.cu:3412-3420), Morton order per cascade. For
        reading (logging, snapshots); modify through writable_buffers()."""
        return self._views(False)[0]

    @property
    def mean_density(self):
        return self._views(False)[2]

    @property
    def bitfield(self):
        return self._views(False)[1]

    def writable_buffers(self):
        """(density_grid, bitfield, mean_density) views for MODIFYING the occupancy state between steps:
        discards a prelaunched sampler so the next step samples with the caller's writes."""
        return self._views(True)

    def set_data_parallel(self, rank, world, group=None, exchange_at_world_1=False):
        """Shard the rays (global ids kept), the compacted batch and the density-grid evaluation over
        `world` ranks; gradients, density-grid maxima and counters are all-reduced by the engine's RCCL
        communicator (nccl backend) or through torch.distributed (gloo: dp.make_allreduce_callback).
        exchange_at_world_1: run the data-parallel step (exchanges included) with one rank too — on a
        one-GPU box, the way to exercise the RCCL path (it must then train bitwise like the plain step)."""
        import torch.distributed as dist
        from .dp import EngineComm, make_allreduce_callback
        self._allreduce = None
        if (world > 1 or exchange_at_world_1) and dist.get_backend(group) == "nccl":
            # one GPU per rank: the engine's RCCL communicator, enqueued on the training stream
            self._allreduce = EngineComm(rank, world, group)
            fn, user = self._allreduce.fn, self._allreduce.handle
        elif world > 1:
            # gloo (CPU tests, ranks sharing a GPU): host round trip through torch.distributed
            self._allreduce = make_allreduce_callback(group)
            fn, user = C.cast(self._allreduce, C.c_void_p), None
        else:
            fn, user = None, None
        check(lib().ngp_nerf_trainer_set_data_parallel(self.handle, rank, world, fn, user))

    def set_pipeline(self, enable):
        """Launch the next step's ray sampling under this step's training pass (default on; identical
        samples). Reading density_grid / bitfield / mean_density keeps it; writable_buffers() discards it,
        so writes through those views reach the next step."""
        check(lib().ngp_nerf_trainer_set_pipeline(self.handle, int(enable)))

    def save_snapshot(self, path, network_config=None, include_optimizer_state=False, compress=True, stream=None):
        """Testbed::save_snapshot (testbed.cu:4873-4937): .ingp = gzip'd msgpack of the network config
        (dict, the Testbed's m_network_config) with the "snapshot" member."""
        cfg = json.dumps(network_config) if network_config is not None else None
        check(lib().ngp_nerf_save_snapshot(self.handle, _stream(stream), os.fsencode(path),
                                           cfg.encode() if cfg else None, int(include_optimizer_state), int(compress)))

    def load_snapshot(self, path, stream=None):
        """Testbed::load_snapshot (testbed.cu:4939-5057) into this trainer's network/optimizer/grid."""
        check(lib().ngp_nerf_load_snapshot(self.handle, _stream(stream), os.fsencode(path)))

    ERROR_MAP_ARRAYS = ("data", "cdf_x_cond_y", "cdf_y", "cdf_img", "pmf_img")

    def error_map(self):
        """The training error map (Testbed::Nerf::Training::ErrorMap, testbed.h:668-677): the rays' losses
        deposited since the current window started ("data", [n_images, h, w]) and, once a window has closed,
        its CDFs ("cdf_x_cond_y" [n_images, cdf_h, cdf_w], "cdf_y" [n_images, cdf_h], "cdf_img", "pmf_img"
        [n_images]), plus the window state (testbed_nerf.cu:3659-3666, 3700-3748)."""
        info = NerfErrorMapInfo()
        check(lib().ngp_nerf_trainer_error_map(self.handle, 0, None, 0, C.byref(info)))
        out = {k: getattr(info, k) for k, _ in NerfErrorMapInfo._fields_ if k != "size"}
        shapes = {"data": (info.n_images, info.height, info.width),
                  "cdf_x_cond_y": (info.n_images, info.cdf_height, info.cdf_width),
                  "cdf_y": (info.n_images, info.cdf_height), "cdf_img": (info.n_images,), "pmf_img": (info.n_images,)}
        for which, name in enumerate(self.ERROR_MAP_ARRAYS):
            check(lib().ngp_nerf_trainer_error_map(self.handle, which, None, 0, C.byref(info)))
            a = np.zeros(int(info.size), np.float32)
            if a.size:
                check(lib().ngp_nerf_trainer_error_map(self.handle, which, a.ctypes.data, a.size, C.byref(info)))
                a = a.reshape(shapes[name])
            out[name] = a
        return out

    # ---- camera pose refinement (nerf.training.optimize_extrinsics, python_api.cu:618-653) ----
    def camera_training(self):
        """The camera optimisation knobs as a dict (ngp_nerf_camera_training)."""
        c = NerfCameraTraining()
        check(lib().ngp_nerf_trainer_get_camera_training(self.handle, C.byref(c)))
        return {k: getattr(c, k) for k, _ in NerfCameraTraining._fields_}

    def set_camera_training(self, **kw):
        """optimize_extrinsics (default 0), n_steps_between_cam_updates (16), extrinsic_l2_reg (1e-4),
        extrinsic_learning_rate (1e-3); knobs not named keep their value. Single GPU only."""
        c = NerfCameraTraining()
        check(lib().ngp_nerf_trainer_get_camera_training(self.handle, C.byref(c)))
        for k, v in kw.items():
            if k not in dict(NerfCameraTraining._fields_):
                raise TypeError(f"set_camera_training: unknown knob {k!r}")
            setattr(c, k, int(v) if k in ("optimize_extrinsics", "n_steps_between_cam_updates") else float(v))
        check(lib().ngp_nerf_trainer_set_camera_training(self.handle, C.byref(c)))

    def camera_extrinsics(self, i):
        """Image i's refined camera-to-world transform in NGP space: the 12 floats of the column-major mat4x3."""
        out = np.zeros(12, np.float32)
        check(lib().ngp_nerf_trainer_camera_extrinsics(self.handle, int(i), out.ctypes.data))
        return out

    def set_camera_extrinsics(self, i, m):
        """Replace image i's transform (12 floats, NGP space, as nerf_matrix_to_ngp returns) in this trainer and reset
        its optimiser state (set_camera_extrinsics, testbed_nerf.cu:2896-2919)."""
        m = np.ascontiguousarray(np.asarray(m, np.float32).reshape(12))
        check(lib().ngp_nerf_trainer_set_camera_extrinsics(self.handle, int(i), m.ctypes.data))

    def reset_camera_extrinsics(self):
        check(lib().ngp_nerf_trainer_reset_camera_extrinsics(self.handle))

    # ---- per-image exposure (nerf.training.optimize_exposure / exposure_l2_reg, python_api.cu:620, 634) ----
    def set_exposure_training(self, optimize=None, l2_reg=None):
        """Training::optimize_exposure (default off) and exposure_l2_reg (0); an argument not named keeps its value. One
        log2 exposure per image and channel is learned with the scene, updated every n_steps_between_cam_updates steps
        with the mean removed. Single GPU; cannot be combined with sample_image_proportional_to_error."""
        cur = self.exposure_training()
        o = cur["optimize_exposure"] if optimize is None else bool(optimize)
        r = cur["exposure_l2_reg"] if l2_reg is None else float(l2_reg)
        check(lib().ngp_nerf_trainer_set_exposure_training(self.handle, int(o), r))

    def exposure_training(self):
        o, r = C.c_int(), C.c_float()
        check(lib().ngp_nerf_trainer_get_exposure_training(self.handle, C.byref(o), C.byref(r)))
        return {"optimize_exposure": bool(o.value), "exposure_l2_reg": r.value}

    def camera_exposure(self, i):
        """Image i's log2 exposure per channel (cam_exposure[i].variable())."""
        out = np.zeros(3, np.float32)
        check(lib().ngp_nerf_trainer_camera_exposure(self.handle, int(i), out.ctypes.data))
        return out

    def set_camera_exposure(self, i, rgb):
        """Set image i's exposure and reset its optimiser's moments (an engine extension)."""
        v = np.ascontiguousarray(np.broadcast_to(np.asarray(rgb, np.float32), (3,)))
        check(lib().ngp_nerf_trainer_set_camera_exposure(self.handle, int(i), v.ctypes.data))

    def exposure_optimizer_state(self, i):
        """cam_exposure[i] as a dict with the reference's member names."""
        e = AdamState()
        check(lib().ngp_nerf_trainer_exposure_optimizer_state(self.handle, int(i), C.byref(e)))
        return _adam_dict(e)

    # ---- error-driven sampling (nerf.training.sample_*_proportional_to_error, python_api.cu:624-625) ----
    def set_error_sampling(self, focal_plane=None, image=None):
        """Draw the rays' pixels in proportion to the error map once its first window has closed: focal_plane (the
        position in the image) and image (which image); a switch not named keeps its value. Both default off. With a
        switch on, training is not reproducible from run to run (the map is summed with float atomics). Cannot be
        combined with optimize_extrinsics."""
        cur = self.error_sampling()
        f = cur["focal_plane"] if focal_plane is None else bool(focal_plane)
        i = cur["image"] if image is None else bool(image)
        check(lib().ngp_nerf_trainer_set_error_sampling(self.handle, int(f), int(i)))

    def error_sampling(self):
        f, i = C.c_int(), C.c_int()
        check(lib().ngp_nerf_trainer_get_error_sampling(self.handle, C.byref(f), C.byref(i)))
        return {"focal_plane": bool(f.value), "image": bool(i.value)}

    # ---- depth supervision (nerf.training.depth_supervision_lambda / depth_loss_type, python_api.cu:616, 635) ----
    def set_depth_supervision(self, lambda_, loss="L1"):
        """Training::depth_supervision_lambda and depth_loss_type (defaults 0 and L1): the steps' loss pass adds the
        depth term for rays whose training pixel has a depth > 0 (NerfDataset.set_depth). Only the loss pass reads them."""
        check(lib().ngp_nerf_trainer_set_depth_supervision(self.handle, float(lambda_),
                                                           LOSS[loss] if isinstance(loss, str) else int(loss)))

    def depth_supervision(self):
        """(lambda, loss name)."""
        lam, lt = C.c_float(0), C.c_uint32(0)
        check(lib().ngp_nerf_trainer_get_depth_supervision(self.handle, C.byref(lam), C.byref(lt)))
        return lam.value, {v: k for k, v in LOSS.items()}[lt.value]

    # ---- environment map (nerf.training.train_envmap, python_api.cu:618-653; testbed.cu:4133-4147) ----
    ENVMAP_ARRAYS = {"params": 0, "ema": 1, "gradient": 2, "first_moments": 3, "second_moments": 4, "param_steps": 5}

    def set_envmap(self, rgba=None, resolution=None, loss=None, optimizer=None):
        """Give the trainer an environment map: rgba, linear RGBA float32 [h, w, 4] (e.g. LoadedNerf.envmap), or zeros of
        resolution = (width, height). rgba=None and resolution=None: remove the map. Every training ray is then
        composited over the map; it trains only with train_envmap on. loss / optimizer: the network config's "envmap"
        section ({"loss": {"otype": ...}, "optimizer": {...}}); not given: the training loss and the main optimizer."""
        if rgba is None and resolution is None:
            check(lib().ngp_nerf_trainer_clear_envmap(self.handle))
            return
        if rgba is not None:
            a = np.ascontiguousarray(rgba.detach().cpu().numpy() if torch.is_tensor(rgba) else rgba, dtype=np.float32)
            if a.ndim != 3 or a.shape[2] != 4 or (resolution is not None and tuple(resolution) != (a.shape[1], a.shape[0])):
                raise ValueError("set_envmap: rgba is [h, w, 4] (and resolution, if given, its (width, height))")
            check(lib().ngp_nerf_trainer_set_envmap(self.handle, a.shape[1], a.shape[0], a.ctypes.data))
        else:
            check(lib().ngp_nerf_trainer_set_envmap(self.handle, int(resolution[0]), int(resolution[1]), None))
        if loss is not None or optimizer is not None:
            lt = -1 if loss is None else (LOSS[loss] if isinstance(loss, str) else int(loss))
            check(lib().ngp_nerf_trainer_set_envmap_training(self.handle, lt,
                                                             json.dumps(optimizer).encode() if optimizer is not None else None))

    def envmap(self, which="params"):
        """The map as a numpy array [h, w, 4] (None without one): "params" (what training reads), "ema" (what rendering
        reads: the debiased EMA parameters once a step ran under an Ema wrapper), "gradient" (the last step's, scaled
        by LOSS_SCALE = 128), "first_moments", "second_moments" or "param_steps" (int32)."""
        w, h = C.c_uint32(), C.c_uint32()
        k = self.ENVMAP_ARRAYS[which]
        check(lib().ngp_nerf_trainer_envmap(self.handle, k, None, 0, C.byref(w), C.byref(h)))
        if w.value == 0:
            return None
        a = np.zeros((h.value, w.value, 4), np.float32)
        check(lib().ngp_nerf_trainer_envmap(self.handle, k, a.ctypes.data, a.size, C.byref(w), C.byref(h)))
        return a.view(np.int32) if which == "param_steps" else a

    def envmap_device(self, ema=True):
        """(device pointer, width, height) of the raw or EMA parameters for NerfRenderer.set_envmap; (None, 0, 0) without
        a map. Ask again after training: the array holding the EMA parameters changes with the first step."""
        p, w, h = C.c_void_p(), C.c_uint32(), C.c_uint32()
        check(lib().ngp_nerf_trainer_envmap_device(self.handle, 1 if ema else 0, C.byref(p), C.byref(w), C.byref(h)))
        return p.value, w.value, h.value

    @property
    def train_envmap(self):
        """Training::train_envmap: every step also trains the environment map (default off; nothing without a map)."""
        v = C.c_int()
        check(lib().ngp_nerf_trainer_get_train_envmap(self.handle, C.byref(v)))
        return bool(v.value)

    @train_envmap.setter
    def train_envmap(self, on):
        check(lib().ngp_nerf_trainer_set_train_envmap(self.handle, int(bool(on))))

    # ---- lens distortion map (nerf.training.optimize_distortion, python_api.cu:618-653; testbed.cu:4066-4076) ----
    DISTORTION_ARRAYS = {"params": 0, "gradient": 1, "first_moments": 2, "second_moments": 3, "param_steps": 4, "inference": 5}

    def set_distortion_map(self, params=None, resolution=None, optimizer=None, default_resolution=(32, 32)):
        """Give the trainer a lens distortion map: params, float32 [h, w, 2] offsets of dir.xy, or zeros of resolution =
        (width, height). params=None and resolution=None: remove the map (and turn optimize_distortion off). A bound
        map is added to every training ray, whether optimize_distortion is on or off. optimizer: the network config's
        "distortion_map" optimizer section (not given: the main optimizer); default_resolution: the section's
        resolution, the size of the map optimize_distortion creates when none is bound."""
        if optimizer is not None or tuple(default_resolution) != (32, 32):
            check(lib().ngp_nerf_trainer_set_distortion_training(
                self.handle, json.dumps(optimizer).encode() if optimizer is not None else None, int(default_resolution[0]),
                int(default_resolution[1])))
        if params is None and resolution is None:
            if optimizer is None:
                check(lib().ngp_nerf_trainer_clear_distortion_map(self.handle))
            return
        if params is not None:
            a = np.ascontiguousarray(params.detach().cpu().numpy() if torch.is_tensor(params) else params, dtype=np.float32)
            if a.ndim != 3 or a.shape[2] != 2 or (resolution is not None and tuple(resolution) != (a.shape[1], a.shape[0])):
                raise ValueError("set_distortion_map: params are [h, w, 2] (and resolution, if given, their (width, height))")
            check(lib().ngp_nerf_trainer_set_distortion_map(self.handle, a.shape[1], a.shape[0], a.ctypes.data))
        else:
            check(lib().ngp_nerf_trainer_set_distortion_map(self.handle, int(resolution[0]), int(resolution[1]), None))

    def set_distortion_training(self, network_config):
        """The "distortion_map" section of a network config dict (testbed.cu:4068-4076): its optimizer, falling back to
        the config's main "optimizer", and its resolution (default 32 x 32)."""
        from .config import distortion_map_config
        sec = distortion_map_config(network_config)
        check(lib().ngp_nerf_trainer_set_distortion_training(self.handle, json.dumps(sec["optimizer"]).encode(),
                                                             int(sec["resolution"][0]), int(sec["resolution"][1])))

    def distortion_map(self, which="params"):
        """The map as a numpy array [h, w, 2] (None without one): "params", "gradient" (the last update's, sum g w / sum w,
        scaled by 128 * n_steps_between_cam_updates), "first_moments", "second_moments", "param_steps" (int32) or
        "inference" (the parameters; the debiased EMA under an optimizer with an Ema wrapper)."""
        w, h = C.c_uint32(), C.c_uint32()
        k = self.DISTORTION_ARRAYS[which]
        check(lib().ngp_nerf_trainer_distortion_map(self.handle, k, None, 0, C.byref(w), C.byref(h)))
        if w.value == 0:
            return None
        a = np.zeros((h.value, w.value, 2), np.float32)
        check(lib().ngp_nerf_trainer_distortion_map(self.handle, k, a.ctypes.data, a.size, C.byref(w), C.byref(h)))
        return a.view(np.int32) if which == "param_steps" else a

    def distortion_map_device(self, inference=True):
        """(device pointer, width, height) of the parameters for NerfRenderer.set_distortion_map; (None, 0, 0) without a map."""
        p, w, h = C.c_void_p(), C.c_uint32(), C.c_uint32()
        check(lib().ngp_nerf_trainer_distortion_map_device(self.handle, 5 if inference else 0, C.byref(p), C.byref(w), C.byref(h)))
        return p.value, w.value, h.value

    def distortion_accumulator(self):
        """The trainer's gradient accumulator as it is: numpy int64 (layout: distortion_accumulator()); None without a map."""
        n = C.c_uint64()
        check(lib().ngp_nerf_trainer_distortion_accumulator(self.handle, None, 0, C.byref(n)))
        if n.value == 0:
            return None
        a = np.zeros(n.value, np.int64)
        check(lib().ngp_nerf_trainer_distortion_accumulator(self.handle, a.ctypes.data, a.size, C.byref(n)))
        return a

    @property
    def optimize_distortion(self):
        """Training::optimize_distortion: train the lens distortion map with the scene (default off). Turning it on
        without a map creates a zero map of the configured resolution. Single GPU; cannot be combined with error-driven
        sampling."""
        v = C.c_int()
        check(lib().ngp_nerf_trainer_get_optimize_distortion(self.handle, C.byref(v)))
        return bool(v.value)

    @optimize_distortion.setter
    def optimize_distortion(self, on):
        check(lib().ngp_nerf_trainer_set_optimize_distortion(self.handle, int(bool(on))))

    def last_samples(self):
        """The last step's sampler call (ngp_nerf_trainer_last_samples): {"rng", "n_rays", "max_samples"} and views of
        the "ray_indices", "rays" and "counters" it wrote (valid until a later sampler runs: turn pipelining off)."""
        rng, n, ms = Rng(), C.c_uint32(), C.c_uint32()
        ri, ry, ct = C.c_void_p(), C.c_void_p(), C.c_void_p()
        check(lib().ngp_nerf_trainer_last_samples(self.handle, C.byref(rng), C.byref(n), C.byref(ms), C.byref(ri),
                                                  C.byref(ry), C.byref(ct)))
        return {"rng": rng, "n_rays": n.value, "max_samples": ms.value,
                "ray_indices": wrap_device(ri.value, n.value, torch.float32).view(torch.int32),
                "rays": wrap_device(ry.value, n.value * 6, torch.float32).view(n.value, 6),
                "counters": wrap_device(ct.value, 2, torch.float32).view(torch.int32)}

    def pose_optimizer_state(self, i):
        """(cam_pos_offset[i], cam_rot_offset[i]) as dicts with the reference's member names."""
        p, r = AdamState(), AdamState()
        check(lib().ngp_nerf_trainer_pose_optimizer_state(self.handle, int(i), C.byref(p), C.byref(r)))
        return _adam_dict(p), _adam_dict(r)

    def train_step(self, get_loss=True, stream=None):
        st = NerfStats()
        check(lib().ngp_nerf_train_step(self.handle, _stream(stream), int(get_loss), C.byref(st)))
        return {k: getattr(st, k) for k, _ in NerfStats._fields_}

    def __del__(self):
        h = getattr(self, "handle", None)
        if h:
            try:
                lib().ngp_nerf_trainer_destroy(h)
            except Exception:
                pass
            self.handle = None


def snapshot_network_config(path):
    """Testbed::load_network_config (testbed.cu:246) of a snapshot: the network config dict without its
    "snapshot" member, e.g. to build the network before NerfTraining.load_snapshot."""
    size = C.c_uint64(0)
    check(lib().ngp_snapshot_network_config(os.fsencode(path), None, C.byref(size)))
    buf = C.create_string_buffer(size.value)
    check(lib().ngp_snapshot_network_config(os.fsencode(path), buf, C.byref(size)))
    return json.loads(buf.value.decode())


# ---- rendering / evaluation -------------------------------------------------------------------
class NerfRenderer:
    """NerfTracer (testbed_nerf.cu:2229-2659): renders a camera view with the network, marching the
    occupancy bitfield. Output: linear RGBA [H, W, 4] float32 composited over `background` (linear)."""

    def __init__(self):
        h = C.c_void_p()
        check(lib().ngp_nerf_renderer_create(C.byref(h)))
        self.handle = h

    RENDER_MODES = {"AO": 0, "Shade": 1, "Normals": 2, "Positions": 3, "Depth": 4, "Distortion": 5,
                    "EncodingVis": 9}  # ERenderMode (common.h:110-121)

    def render(self, network, cfg, camera, bitfield=None, spp=1, sample_index=0, min_transmittance=0.01,
               background=(0.0, 0.0, 0.0, 0.0), use_inference_params=True, stream=None, render_mode="Shade",
               depth_scale=1.0, show_accel=-1):
        """render_mode: an ERenderMode name; depth_scale (Depth): 1 / the dataset's scale (testbed_nerf.cu:2822);
        show_accel: Testbed::Nerf::show_accel (-1 off; 0..7: the march's minimum mip, opaque steps, Positions by cell)."""
        check(lib().ngp_nerf_renderer_set_mode(self.handle, self.RENDER_MODES[render_mode]))
        check(lib().ngp_nerf_renderer_set_show_accel(self.handle, int(show_accel)))
        check(lib().ngp_nerf_renderer_set_depth_scale(self.handle, float(depth_scale)))
        out = torch.empty((camera.height, camera.width, 4), dtype=torch.float32, device="cuda")
        bg = (C.c_float * 4)(*[float(v) for v in background])
        check(lib().ngp_nerf_render(self.handle, network.handle, C.byref(cfg), _stream(stream), C.byref(camera),
                                    _ptr(bitfield), spp, sample_index, float(min_transmittance), bg,
                                    int(use_inference_params), _ptr(out)))
        return out

    def set_envmap(self, envmap=None):
        """Render over an environment map instead of `background` (testbed_nerf.cu:2315-2319): a contiguous float32
        device tensor [h, w, 4] (kept alive by the renderer), a NerfTraining (its EMA parameters, inference_view();
        bind again after further training or after the trainer's map changes), or None to unbind."""
        if envmap is None:
            self._envmap = None
            check(lib().ngp_nerf_renderer_set_envmap(self.handle, None, 0, 0))
        elif isinstance(envmap, NerfTraining):
            p, w, h = envmap.envmap_device(ema=True)
            self._envmap = envmap
            check(lib().ngp_nerf_renderer_set_envmap(self.handle, p, w, h))
        else:
            if envmap.dtype != torch.float32 or envmap.dim() != 3 or envmap.shape[2] != 4 or not envmap.is_contiguous() \
                    or not envmap.is_cuda:
                raise ValueError("set_envmap: a contiguous float32 device tensor [h, w, 4]")
            self._envmap = envmap
            check(lib().ngp_nerf_renderer_set_envmap(self.handle, _ptr(envmap), envmap.shape[1], envmap.shape[0]))

    def set_distortion_map(self, distortion=None):
        """Render through a lens distortion map (render_with_lens_distortion; testbed_nerf.cu:2229-2344), which render
        mode "Distortion" also shows: a contiguous float32 device tensor [h, w, 2] (kept alive by the renderer), a
        NerfTraining (its map; bind again after the trainer's map is set or cleared), or None to unbind."""
        if distortion is None:
            self._distortion = None
            check(lib().ngp_nerf_renderer_set_distortion_map(self.handle, None, 0, 0))
        elif isinstance(distortion, NerfTraining):
            p, w, h = distortion.distortion_map_device(inference=True)
            self._distortion = distortion
            check(lib().ngp_nerf_renderer_set_distortion_map(self.handle, p, w, h))
        else:
            _check_distortion_map(distortion, None, "set_distortion_map")
            if not distortion.is_cuda:
                raise ValueError("set_distortion_map: a device tensor")
            self._distortion = distortion
            check(lib().ngp_nerf_renderer_set_distortion_map(self.handle, _ptr(distortion), distortion.shape[1], distortion.shape[0]))

    def __del__(self):
        h = getattr(self, "handle", None)
        if h:
            try:
                lib().ngp_nerf_renderer_destroy(h)
            except Exception:
                pass
            self.handle = None


def linear_to_srgb(x):
    return torch.where(x < 0.0031308, 12.92 * x, 1.055 * torch.pow(torch.clamp(x, min=0), 0.41666) - 0.055)


def srgb_to_linear(x):
    return torch.where(x <= 0.04045, x / 12.92, torch.pow((x + 0.055) / 1.055, 2.4))


def ground_truth_linear(rgba8, background=(0.0, 0.0, 0.0)):
    """The reference's render_ground_truth of a training/test image (sRGB RGBA8, premultiplied by
    alpha in linear space, composited over the linear background), as a float [H, W, 4] tensor."""
    px = torch.as_tensor(rgba8).float() / 255.0
    a = px[..., 3:4]
    rgb = srgb_to_linear(px[..., :3]) * a + torch.tensor(background, dtype=torch.float32, device=px.device) * (1 - a)
    return torch.cat([rgb, torch.ones_like(a)], dim=-1)


def psnr(image, ref):
    """scripts/run.py:245-252: MSE of clip(linear_to_srgb(rgb), 0, 1), PSNR = -10 log10(MSE)."""
    A = torch.clamp(linear_to_srgb(image[..., :3].float()), 0.0, 1.0)
    R = torch.clamp(linear_to_srgb(ref[..., :3].float().to(A.device)), 0.0, 1.0)
    mse = float(torch.mean((A - R) ** 2))
    return -10.0 * math.log10(max(mse, 1e-12)), mse
