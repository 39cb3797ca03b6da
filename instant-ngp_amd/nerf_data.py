"""NeRF dataset ingest: transforms.json + images -> NerfDataset.

Host-side restatement of the reference loader `load_nerf` (src/nerf_loader.cu:260-726) for the
formats the training path consumes: the original NeRF/instant-ngp `transforms.json` (one or more
files), 8-bit images (PNG/JPEG/BMP... decoded to RGBA8 sRGB, EImageDataType::Byte), `.exr` frames (HDR: linear
premultiplied RGBA stored as fp16, EImageDataType::Half, with `fix_premult`; nerf_loader.cu:429-430, 549-553; the two kinds
may be mixed, and the `.alpha.` companion, the dynamic masks and `white_transparent` / `black_transparent` apply to
the 8-bit frames only, as in the reference), perspective and
OpenCV / OpenCV-fisheye lenses, per-frame intrinsics overrides, `scale` / `offset` / `aabb` /
`aabb_scale`, the sharpness filter, `n_frames`, `white_transparent` / `black_transparent`,
`<file>.alpha.<ext>` alpha images, `dynamic_mask_<name>.png` masks, the `envmap` image, and depth supervision:
`integer_depth_scale`, `enable_depth_loading` and per-frame `depth_path` 16-bit images (nerf_loader.cu:404-422, 471,
609-621, 711). Not handled (the loader raises): per-pixel ray files, rolling shutter, FTheta /
LatLong / equirectangular lenses, Mitsuba scenes — none of the in-scope datasets use them.
Image decoding is PIL's (the reference uses stb_image) or, for EXR, the package's reader (exr.py; the reference uses
tinyexr); the pixels then travel to the device
unchanged, as `set_training_image` does with `convert_rgba32` (nerf_loader.cu:49-71).
"""
import json
import math
import os
import re

import numpy as np

from .nerf import LENS_OPENCV, LENS_OPENCV_FISHEYE, LENS_PERSPECTIVE, NerfDataset, make_image, nerf_matrix_to_ngp

NERF_SCALE = 0.33  # nerf_loader.h:29
IMAGE_FORMATS = ("png", "jpg", "jpeg", "bmp", "gif", "tga", "pic", "pnm", "psd", "exr")  # nerf_loader.cu:303-305
MASK_COLOR = 0x00FF00FF  # hot pink (nerf_loader.cu:580)


def _natural_key(s):
    """SI::natural::compare order (nerf_loader.cu:339-341): digit runs compare as numbers."""
    return [(0, int(t), "") if t.isdigit() else (1, 0, t) for t in re.split(r"(\d+)", s) if t != ""]


def _resolve(base, local):
    """resolve_path (nerf_loader.cu:307-318): try the known extensions when none is given."""
    path = local if os.path.isabs(local) else os.path.join(base, local)
    if not os.path.splitext(path)[1] and not os.path.exists(path):
        for ext in IMAGE_FORMATS:
            if os.path.exists(path + "." + ext):
                return path + "." + ext
    return path


def _load_json(path):
    with open(path, "r") as f:
        text = f.read()
    # nlohmann::json::parse(..., ignore_comments = true): strip // and /* */ comments outside strings
    out, i, n, in_str = [], 0, len(text), False
    while i < n:
        c = text[i]
        if in_str:
            out.append(c)
            if c == "\\" and i + 1 < n:
                out.append(text[i + 1])
                i += 1
            elif c == '"':
                in_str = False
        elif c == '"':
            in_str = True
            out.append(c)
        elif text.startswith("//", i):
            while i < n and text[i] != "\n":
                i += 1
            continue
        elif text.startswith("/*", i):
            j = text.find("*/", i + 2)
            i = n if j < 0 else j + 2
            continue
        else:
            out.append(c)
        i += 1
    return json.loads("".join(out))


def _read_lens(j, lens):
    """read_lens (nerf_loader.cu:160-224) into lens = {mode, params[4], principal[2]}."""
    opencv_mode = LENS_OPENCV_FISHEYE if j.get("is_fisheye", False) else LENS_OPENCV
    mode = LENS_PERSPECTIVE
    for name, idx in (("k1", 0), ("k2", 1), ("k3", 2), ("k4", 3), ("p1", 2), ("p2", 3)):
        if name in j:
            lens["params"][idx] = float(j[name])
            if lens["params"][idx] != 0.0:
                mode = opencv_mode
    if "cx" in j:
        lens["principal"][0] = float(np.float32(j["cx"]) / np.float32(j["w"]))
    if "cy" in j:
        lens["principal"][1] = float(np.float32(j["cy"]) / np.float32(j["h"]))
    if "rolling_shutter" in j:
        raise NotImplementedError("rolling_shutter datasets are not supported by this loader")
    for k in ("ftheta_p0", "latlong", "equirectangular"):
        if k in j:
            raise NotImplementedError(f"lens '{k}' is not supported (perspective / OpenCV / OpenCV fisheye only)")
    if mode != LENS_PERSPECTIVE:
        lens["mode"] = mode


def _fov_to_focal(res, degrees):
    """fov_to_focal_length (common.h), float arithmetic."""
    f32 = np.float32
    return float(f32(0.5) * f32(res) / np.tan(f32(0.5) * f32(degrees) * f32(math.pi) / f32(180)))


def _read_focal(j, res):
    """read_focal_length (nerf_loader.cu:226-258); returns (fx, fy) or None."""
    def axis(r, a):
        if a + "_fov" in j:
            return _fov_to_focal(r, j[a + "_fov"])
        if "fl_" + a in j:
            return float(np.float32(j["fl_" + a]))
        if "camera_angle_" + a in j:
            return _fov_to_focal(r, np.float32(j["camera_angle_" + a]) * np.float32(180) / np.float32(math.pi))
        return 0.0
    x, y = axis(res[0], "x"), axis(res[1], "y")
    if x != 0.0:
        return (x, y if y != 0.0 else x)
    if y != 0.0:
        return (y, y)
    return None


def _decode(path):
    from PIL import Image  # image decoding only (the reference uses stb_image)
    with Image.open(path) as im:
        return np.array(im.convert("RGBA"), dtype=np.uint8)


def _decode_8bit(base, fr, p, white, black):
    """An 8-bit frame as RGBA8 [h, w, 4]: the image, its `.alpha.` companion and dynamic mask if present, then
    convert_rgba32."""
    px = _decode(p)
    h, w = px.shape[:2]
    ap = _resolve(base, f"{fr['file_path']}.alpha.{os.path.splitext(p)[1]}")
    if os.path.exists(ap):
        a = _decode(ap)
        if a.shape[:2] != (h, w):
            raise ValueError(f"Alpha image {ap} has wrong resolution.")
        px[..., 3] = (255.0 * _srgb_to_linear(a[..., 0].astype(np.float32) / 255.0)).astype(np.uint8)
    mp = os.path.join(os.path.dirname(p), f"dynamic_mask_{os.path.splitext(os.path.basename(p))[0]}.png")
    mask_color = 0
    if os.path.exists(mp):
        m = _decode(mp)
        if m.shape[:2] != (h, w):
            raise ValueError(f"Dynamic mask {mp} has wrong resolution.")
        mask_color = MASK_COLOR
        px.view(np.uint32)[..., 0][np.any(m[..., :3] != 0, axis=-1)] = MASK_COLOR
    # convert_rgba32 (nerf_loader.cu:49-71)
    if white:
        px[..., 3][np.all(px[..., :3] == 255, axis=-1)] = 0
    if black:
        px[..., 3][np.all(px[..., :3] == 0, axis=-1)] = 0
    if mask_color:
        px.view(np.uint32)[..., 0][px.view(np.uint32)[..., 0] == mask_color] = 0x00FF00FF
    return px


def _decode_exr(path, fix_premult):
    """load_exr_to_gpu (tinyexr_wrapper.cu:41-55, interleave_and_cast_kernel): float16 [h, w, 4], rgb = half(float(rgb) *
    (alpha if fix_premult else 1)), alpha = half(alpha)."""
    from .exr import read_exr
    px = np.asarray(read_exr(path), np.float32)
    if fix_premult:
        px = np.concatenate([px[..., :3] * px[..., 3:4], px[..., 3:4]], axis=-1)
    with np.errstate(over="ignore"):  # beyond fp16's range: infinity, as the device conversion gives
        return np.ascontiguousarray(px.astype(np.float16))


def _decode_depth(path):
    """load_stbi_16(path, 1 channel): a single-channel 16-bit image as uint16 [h, w] (8-bit files widen as stb does,
    v * 257)."""
    from PIL import Image
    with Image.open(path) as im:
        if im.mode in ("I;16", "I;16L", "I;16B", "I"):
            return np.ascontiguousarray(np.array(im).astype(np.uint16))
        return np.ascontiguousarray(np.array(im.convert("L"), dtype=np.uint16) * np.uint16(257))


def _srgb_to_linear(x):
    return np.where(x <= 0.04045, x / 12.92, ((x + 0.055) / 1.055) ** 2.4)


def _load_envmap(path):
    """The transforms file's "envmap" image (nerf_loader.cu:516-528) as linear RGBA float32 [h, w, 4]: load_exr_gpu for
    .exr (the package's EXR reader), else load_stbi_gpu's from_rgba32 (common_device.cuh:771-798): sRGB decoded and
    premultiplied by alpha."""
    if not os.path.exists(path):
        raise FileNotFoundError(f"Environment map {path} does not exist.")
    if path.lower().endswith(".exr"):
        from .exr import read_exr
        return np.ascontiguousarray(read_exr(path), dtype=np.float32)
    px = _decode(path).astype(np.float32) * np.float32(1.0 / 255.0)
    alpha = px[..., 3:4]
    rgb = _srgb_to_linear(px[..., :3]).astype(np.float32) * alpha
    return np.ascontiguousarray(np.concatenate([rgb, alpha], axis=-1), dtype=np.float32)


class LoadedNerf:
    """Result of load_nerf: cameras + pixels (host) and the dataset-level settings. rgba8 holds one array per image:
    uint8 RGBA8 for an 8-bit frame, float16 linear premultiplied RGBA for an EXR frame."""

    def __init__(self):
        self.images, self.rgba8, self.paths = [], [], []
        self.scale, self.offset, self.aabb_scale = NERF_SCALE, [0.5, 0.5, 0.5], 1.0
        self.up = [0.0, 1.0, 0.0]
        self.envmap = None  # the "envmap" image: linear RGBA float32 [h, w, 4] (NerfTraining.set_envmap takes it)
        # depth supervision: per image the uint16 pixels of its depth_path [h, w], or None (no depth_path, a missing
        # file, enable_depth_loading false or no integer_depth_scale), and per image the scale the dataset multiplies
        # them by: integer_depth_scale * scale (nerf_loader.cu:711)
        self.depth, self.depth_scale = [], []

    @property
    def image_types(self):
        """EImageDataType per image: 1 Byte, 2 Half."""
        return [2 if px.dtype == np.float16 else 1 for px in self.rgba8]

    @property
    def is_hdr(self):
        """NerfDataset::is_hdr: a frame was an EXR file (the Testbed then trains with the exponential rgb activation)."""
        return any(px.dtype == np.float16 for px in self.rgba8)

    @property
    def envmap_resolution(self):
        """(width, height) of the dataset's environment map, (0, 0) without one (NerfDataset::envmap_resolution)."""
        return (0, 0) if self.envmap is None else (self.envmap.shape[1], self.envmap.shape[0])

    def __len__(self):
        return len(self.images)

    def to_device(self):
        """NerfDataset (pixels and cameras uploaded: set_training_image)."""
        ds = NerfDataset(self.images, self.rgba8)
        for i, (d, s) in enumerate(zip(self.depth, self.depth_scale)):
            if d is not None:   # an image without depth pixels stays without depth: the same loss as the zeros the
                ds.set_depth(i, d, s)   # reference stores for it, at no cost
        return ds


def load_nerf(jsonpaths, max_images=None):
    """load_nerf (nerf_loader.cu:260-726). jsonpaths: a transforms.json, a directory holding
    transforms*.json, or a list of json files."""
    if isinstance(jsonpaths, (str, os.PathLike)):
        p = os.fspath(jsonpaths)
        if os.path.isdir(p):
            jsonpaths = sorted(os.path.join(p, f) for f in os.listdir(p) if f.startswith("transforms") and f.endswith(".json"))
        else:
            jsonpaths = [p]
    if not jsonpaths:
        raise ValueError("Cannot load NeRF data from an empty set of paths.")
    res = LoadedNerf()
    jsons = [_load_json(p) for p in jsonpaths]
    per_json_frames = []
    enable_depth_loading = True
    fix_premult = False
    for path, j in zip(jsonpaths, jsons):
        base = os.path.dirname(path)
        if not isinstance(j.get("frames"), list):
            per_json_frames.append([])
            continue
        frames = sorted(j["frames"], key=lambda fr: _natural_key(fr["file_path"]))
        for fr in frames:
            fr["file_path"] = fr["file_path"].replace("\\", "/")
        if "n_frames" in j:
            frames = frames[:min(len(frames), int(j["n_frames"]))]
        thresh = float(j.get("sharpness_discard_threshold", 0.0))
        if frames and "sharpness" in frames[0]:
            # kill frames blurrier than their neighbours (:349-372); also drops missing files
            kept = []
            for i in range(len(frames)):
                s0, s1 = max(0, i - 3), min(i + 3, len(frames) - 1)
                mean = sum(float(frames[k].get("sharpness", 1.0)) for k in range(s0, s1))
                mean = mean / (s1 - s0) if s1 > s0 else float("nan")
                if os.path.exists(_resolve(base, frames[i]["file_path"])) and float(frames[i].get("sharpness", 1.0)) > thresh * mean:
                    kept.append(frames[i])
            frames = kept
        per_json_frames.append(frames)
    for path, j, frames in zip(jsonpaths, jsons, per_json_frames):
        base = os.path.dirname(path)
        if j.get("normal_mts_args") is not None:
            raise NotImplementedError("Mitsuba scenes are not supported")
        if "camera" in j and isinstance(j["camera"], list):
            raise ValueError("hdf5 is no longer supported. please use the hdf52nerf.py conversion script")
        white = bool(j.get("white_transparent", False))
        black = bool(j.get("black_transparent", False))
        if "scale" in j:
            res.scale = float(j["scale"])
        if "aabb_scale" in j:
            res.aabb_scale = float(j["aabb_scale"])
        if "offset" in j:
            o = j["offset"]
            res.offset = [float(v) for v in o] if isinstance(o, list) else [float(o)] * 3
        if "aabb" in j:
            a = j["aabb"]
            length = max(1e-6, max(abs(float(a[1][k]) - float(a[0][k])) for k in range(3)))
            res.scale = 1.0 / length
            res.offset = [(float(a[1][k]) + float(a[0][k])) * 0.5 * -res.scale + 0.5 for k in range(3)]
        if "up" in j:
            res.up = [float(j["up"][1]), float(j["up"][2]), float(j["up"][0])]
        if "envmap" in j:  # the initial environment map; its resolution is the map's (nerf_loader.cu:516-528)
            res.envmap = _load_envmap(_resolve(base, j["envmap"]))
        if "enable_depth_loading" in j:   # like the reference's flag, it carries over to the files after this one
            enable_depth_loading = bool(j["enable_depth_loading"])
        if "fix_premult" in j:   # carries over likewise (nerf_loader.cu:402, 429-430)
            fix_premult = bool(j["fix_premult"])
        integer_depth_scale = np.float32(j["integer_depth_scale"]) if "integer_depth_scale" in j else np.float32(-1.0)
        lens0 = {"mode": LENS_PERSPECTIVE, "params": [0.0] * 4, "principal": [0.5, 0.5]}
        _read_lens(j, lens0)
        for fr in frames:
            if max_images is not None and len(res.images) >= max_images:
                break
            p = _resolve(base, fr["file_path"] or "")
            if not os.path.exists(p):
                raise FileNotFoundError(f"Could not find image file '{p}'.")
            if p.lower().endswith(".exr"):
                px = _decode_exr(p, fix_premult)
            else:
                px = _decode_8bit(base, fr, p, white, black)
            h, w = px.shape[:2]
            focal = _read_focal(fr, (w, h)) or _read_focal(j, (w, h))
            if focal is None:
                raise ValueError("Couldn't read fov.")
            if "transform_matrix_end" in fr and fr.get("transform_matrix_end") != fr.get("transform_matrix_start", fr.get("transform_matrix")):
                pass  # only the start transform is used without a rolling shutter (t = 0)
            mat = fr.get("transform_matrix_start", fr["transform_matrix"])
            lens = {"mode": lens0["mode"], "params": list(lens0["params"]), "principal": list(lens0["principal"])}
            _read_lens(fr, lens)  # per-frame override (:676)
            xf = nerf_matrix_to_ngp(np.asarray(mat, np.float32), res.scale, res.offset)
            res.images.append(make_image(w, h, xf, focal=focal, principal=lens["principal"], lens_mode=lens["mode"],
                                         lens_params=lens["params"]))
            res.rgba8.append(px)
            res.paths.append(p)
            depth = None
            if enable_depth_loading and integer_depth_scale > 0 and "depth_path" in fr:
                dp = _resolve(base, fr["depth_path"])
                if os.path.exists(dp):   # a missing depth file is ignored
                    depth = _decode_depth(dp)
                    if depth.shape != (h, w):
                        raise ValueError(f"Depth image {dp} has wrong resolution.")
            res.depth.append(depth)
            res.depth_scale.append(integer_depth_scale)
    if not res.images:
        raise ValueError("No training images were found for NeRF training!")
    # m.depth_scale * result.scale, in float, with the scale every file has had its say on (nerf_loader.cu:711)
    res.depth_scale = [float(s * np.float32(res.scale)) for s in res.depth_scale]
    return res
