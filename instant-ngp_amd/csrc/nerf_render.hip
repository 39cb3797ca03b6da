// nerf_render.hip — the NeRF renderer for gfx950 (see nerf.h): NerfTracer's kernels and render_frame.
#include <algorithm>
#include <cmath>
#include <functional>

#include "nerf_device.h"
#include "rng.h"
#include "envmap.h"
#include "distortion.h"

namespace ngp {
namespace nerf {

// ------------------------------------------------------------------------------------------------
// Rendering: NerfTracer (testbed_nerf.cu:2229-2503 init/advance, 2504-2659 trace, 948-1196
// generate_next_nerf_network_inputs / composite_kernel_nerf, 2164-2226 shade / compact), pinhole
// cameras, ERenderMode::Shade. Compaction uses atomic slots like the reference: rays are independent,
// so the image does not depend on their order.
// ------------------------------------------------------------------------------------------------

// if_unoccupied_advance_to_next_occupied_voxel<MIP_FROM_DT = false> (testbed_nerf.cu:811-842)
__device__ float advance_to_occupied(float t, const Cone& cone, V3 o, V3 d, V3 idir, const uint8_t* bitfield, uint32_t min_mip,
                                     uint32_t max_mip, const Aabb& box) {
	while (true) {
		const V3 pos = v3(o.x + t * d.x, o.y + t * d.y, o.z + t * d.z);
		if (t >= 16384.0f || !aabb_contains(box, pos)) return 16384.0f;
		uint32_t mip = min(max(mip_from_pos(pos, CASCADES - 1), min_mip), max_mip);
		if (!bitfield || density_grid_occupied_at(pos, bitfield, mip)) return t;
		while (mip < max_mip && !density_grid_occupied_at(pos, bitfield, mip + 1)) ++mip;
		t = advance_to_next_voxel(t, cone, pos, d, idir, mip);
	}
}

struct Payload {  // NerfPayload (nerf.h:32-40)
	float o[3], d[3];
	float t, max_weight;
	uint32_t idx, n_steps, alive;
};

// DIST: the distortion map of the arguments adds its offset at the pixel's uv to dir.xy after the lens (render_with_lens_distortion)
template <bool DIST> using RenderArgsK = std::conditional_t<DIST, RenderArgsDist, RenderArgs>;
__device__ __forceinline__ DistMap dist_of(const RenderArgs&) { return DistMap{}; }
__device__ __forceinline__ DistMap dist_of(const RenderArgsDist& a) { return a.dist; }

template <bool DIST>
__global__ void k_render_init(RenderArgsK<DIST> a, Payload* __restrict__ pay, float* __restrict__ rgba) {
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	const uint32_t W = a.width, H = a.height;
	if (i >= W * H) return;
	const uint32_t x = i % W, y = i / W;
	float ox, oy;
	ld_random_pixel_offset(a.snap_to_pixel_centers ? 0u : a.sample_index, &ox, &oy);
	const float u = ((float)x + ox) / (float)W, v = ((float)y + oy) / (float)H;
	// uv_to_ray (common_device.cuh:443-510), screen_center = render_screen_center(1 - principal point)
	// (testbed.cu:852, 4376-4379, 4541) = the principal point, with
	// the training view's lens (render_with_lens_distortion, testbed.cu:845-846)
	float dx = (u - a.screen_center[0]) * (float)W / a.focal[0];
	float dy = (v - a.screen_center[1]) * (float)H / a.focal[1];
	lens_undistort(a.lens_mode, a.lens, &dx, &dy);
	if (DIST) {
		const DistMap dm = dist_of(a);
		float fx, fy;
		distortion_offset(dm.data, dm.w, dm.h, u, v, &fx, &fy);
		dx += fx;
		dy += fy;
	}
	const float* m = a.cam;
	V3 d = v3(m[0] * dx + m[3] * dy + m[6], m[1] * dx + m[4] * dy + m[7], m[2] * dx + m[5] * dy + m[8]);
	V3 o = v3(m[9] + d.x * a.near_distance, m[10] + d.y * a.near_distance, m[11] + d.z * a.near_distance);
	Payload p;
	p.max_weight = 0.f;
	p.idx = i;
	p.n_steps = 0;
	p.alive = 0;
	rgba[4 * (size_t)i] = rgba[4 * (size_t)i + 1] = rgba[4 * (size_t)i + 2] = rgba[4 * (size_t)i + 3] = 0.f;
	const float inv = 1.0f / sqrtf(d.x * d.x + d.y * d.y + d.z * d.z);
	d = v3(d.x * inv, d.y * inv, d.z * inv);
	p.o[0] = o.x; p.o[1] = o.y; p.o[2] = o.z;
	p.d[0] = d.x; p.d[1] = d.y; p.d[2] = d.z;
	const Aabb box{v3(a.aabb_min[0], a.aabb_min[1], a.aabb_min[2]), v3(a.aabb_max[0], a.aabb_max[1], a.aabb_max[2])};
	float tmin, tmax;
	aabb_ray_intersect(box, o, d, &tmin, &tmax);
	float t = fmaxf(tmin, 0.0f) + 1e-6f;
	if (aabb_contains(box, v3(o.x + t * d.x, o.y + t * d.y, o.z + t * d.z))) {
		// advance_pos_nerf (:844-900): jitter the start by a scrambled-Sobol fraction of a step
		const V3 idir = v3(1.0f / d.x, 1.0f / d.y, 1.0f / d.z);
		const Cone cone = make_cone(a.cone_angle_constant);
		t = advance_n_steps(t, cone, ld_random_val(a.sample_index, i * 786433u));
		// min_mip = show_accel >= 0 ? show_accel : 0 (testbed_nerf.cu:2497)
		t = advance_to_occupied(t, cone, o, d, idir, a.bitfield, a.show_accel >= 0 ? (uint32_t)a.show_accel : 0u, a.max_mip, box);
		if (t < 16384.0f) p.alive = 1;
	}
	p.t = t;
	pay[i] = p;
}

// compact_kernel_nerf (:2198-2226)
__global__ void k_render_compact(uint32_t n, const Payload* __restrict__ src, const float* __restrict__ src_rgba,
                                 Payload* __restrict__ dst, float* __restrict__ dst_rgba, Payload* __restrict__ hit,
                                 float* __restrict__ hit_rgba, uint32_t* __restrict__ counters) {
	// One atomic per wave and list (the reference takes one per ray: ~2 M same-address atomics per
	// compaction at 1080p serialise in L2, ~10 ms). Slot order differs run to run, as with per-ray
	// atomics; every later pass is per ray (the frame is written through the payload's pixel index).
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	const bool in = i < n;
	Payload p{};
	f32x4 c{0.f, 0.f, 0.f, 0.f};
	if (in) {
		p = src[i];
		c = *(const f32x4*)(src_rgba + 4 * (size_t)i);
	}
	const bool alive = in && p.alive, hitp = in && !p.alive && c[3] > 0.001f;
	const uint64_t ma = __ballot(alive), mh = __ballot(hitp);
	const uint32_t lane = __lane_id();
	const uint64_t below = (1ull << lane) - 1ull;
	uint32_t ba = 0, bh = 0;
	if (lane == 0) {
		if (ma) ba = atomicAdd(&counters[0], (uint32_t)__popcll(ma));
		if (mh) bh = atomicAdd(&counters[1], (uint32_t)__popcll(mh));
	}
	ba = (uint32_t)__shfl((int)ba, 0);
	bh = (uint32_t)__shfl((int)bh, 0);
	if (alive) {
		const uint32_t k = ba + (uint32_t)__popcll(ma & below);
		dst[k] = p;
		*(f32x4*)(dst_rgba + 4 * (size_t)k) = c;
	} else if (hitp) {
		const uint32_t k = bh + (uint32_t)__popcll(mh & below);
		hit[k] = p;
		*(f32x4*)(hit_rgba + 4 * (size_t)k) = c;
	}
}

// generate_next_nerf_network_inputs (:948-1014): coordinate (i, j) at row i + j * n
__global__ void k_render_inputs(RenderArgs a, uint32_t n, uint32_t n_steps, Payload* __restrict__ pay, float* __restrict__ coords) {
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n) return;
	Payload& p = pay[i];
	if (!p.alive) return;
	const V3 o = v3(p.o[0], p.o[1], p.o[2]), d = v3(p.d[0], p.d[1], p.d[2]);
	const V3 idir = v3(1.0f / d.x, 1.0f / d.y, 1.0f / d.z);
	const Aabb box{v3(a.aabb_min[0], a.aabb_min[1], a.aabb_min[2]), v3(a.aabb_max[0], a.aabb_max[1], a.aabb_max[2])};
	const V3 diag = v3(box.mx.x - box.mn.x, box.mx.y - box.mn.y, box.mx.z - box.mn.z);
	const Cone cone = make_cone(a.cone_angle_constant);
	float t = p.t;
	for (uint32_t j = 0; j < n_steps; ++j) {
		t = advance_to_occupied(t, cone, o, d, idir, a.bitfield, a.show_accel >= 0 ? (uint32_t)a.show_accel : 0u, a.max_mip, box);
		if (t >= 16384.0f) {
			p.n_steps = j;
			return;
		}
		const float dt = calc_dt(t, cone);
		const V3 pos = v3(o.x + d.x * t, o.y + d.y * t, o.z + d.z * t);
		float* c = coords + (size_t)(i + j * n) * 7;
		c[0] = (pos.x - box.mn.x) / diag.x; c[1] = (pos.y - box.mn.y) / diag.y; c[2] = (pos.z - box.mn.z) / diag.z;
		c[3] = warp_dt(dt);
		c[4] = (d.x + 1.0f) * 0.5f; c[5] = (d.y + 1.0f) * 0.5f; c[6] = (d.z + 1.0f) * 0.5f;
		t += dt;
	}
	p.t = t;
	p.n_steps = n_steps;
}

// composite_kernel_nerf (:1016-1196); network output RM [16 x stride]. The colour of a step by ERenderMode
// (:1183-1208): Shade the network's rgb; Normals normalize(-density'(raw) * d(raw density)/d(position)), the
// gradient in the coordinates' position rows (render_frame's grad); Positions (pos - 0.5) / 2 + 0.5, or with
// show_accel >= 0 the step's occupancy cell (mip = max(show_accel, mip_from_pos), red 1 - mip / 7, green and blue
// two pcg32 draws seeded by the cell); EncodingVis the warped position (the network's input); Depth dot(camera
// forward, pos - ray origin) * depth_scale; AO the step's alpha. pos = unwarp_position of the step's coordinate over
// the aabb the inputs were warped with. show_accel >= 0 also makes every step opaque (alpha 1, :1078-1080).
__global__ void k_render_composite(RenderArgs a, uint32_t n, uint32_t stride, uint32_t current_step, uint32_t n_steps,
                                   Payload* __restrict__ pay, float* __restrict__ rgba, const float* __restrict__ coords,
                                   const f16* __restrict__ out) {
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n) return;
	Payload& p = pay[i];
	if (!p.alive) return;
	f32x4 c = *(const f32x4*)(rgba + 4 * (size_t)i);
	const uint32_t actual = p.n_steps;
	uint32_t j = 0;
	for (; j < actual; ++j) {
		const size_t r = i + (size_t)j * n;
		const float o0 = (float)out[r], o1 = (float)out[r + stride], o2 = (float)out[r + 2 * (size_t)stride];
		const float o3 = (float)out[r + 3 * (size_t)stride];
		const float T = 1.f - c[3];
		const float dt = unwarp_dt(coords[r * 7 + 3]);
		const float alpha = a.show_accel >= 0 ? 1.f : 1.f - ngp_expf_fast(-network_to_density(o3, a.density_activation) * dt);
		const float weight = alpha * T;
		float rgb[3];
		if (a.render_mode == RENDER_NORMALS) {
			const float dd = -network_to_density_derivative(o3, a.density_activation);
			const float nx = dd * coords[r * 7 + 0], ny = dd * coords[r * 7 + 1], nz = dd * coords[r * 7 + 2];
			const float inv = 1.0f / sqrtf(nx * nx + ny * ny + nz * nz);  // glm normalize (0 -> NaN, as the reference)
			rgb[0] = nx * inv; rgb[1] = ny * inv; rgb[2] = nz * inv;
		} else if (a.render_mode == RENDER_POSITIONS || a.render_mode == RENDER_DEPTH) {
			float pos[3];
#pragma unroll
			for (int k = 0; k < 3; ++k) pos[k] = coords[r * 7 + k] * (a.aabb_max[k] - a.aabb_min[k]) + a.aabb_min[k];
			if (a.render_mode == RENDER_POSITIONS && a.show_accel >= 0) {
				// :1190-1199: the cell of the cascade the march tested, coloured by its mip and a seeded pcg32
				const uint32_t mip = max((uint32_t)a.show_accel, mip_from_pos(v3(pos[0], pos[1], pos[2]), CASCADES - 1));
				const uint32_t res = GRIDSIZE >> mip;
				const int ix = (int)(pos[0] * (float)res), iy = (int)(pos[1] * (float)res), iz = (int)(pos[2] * (float)res);
				Pcg32Dev rng{0u, (1ull << 1u) | 1u};  // pcg32(initstate, initseq = 1)
				pcg_next(rng);
				rng.state += (uint64_t)(int64_t)(ix + iy * 232323 + iz * 727272);
				pcg_next(rng);
				rgb[0] = 1.f - (float)mip * (1.f / (float)(CASCADES - 1));
				rgb[1] = pcg_float(rng);
				rgb[2] = pcg_float(rng);
			} else if (a.render_mode == RENDER_POSITIONS) {
#pragma unroll
				for (int k = 0; k < 3; ++k) rgb[k] = (pos[k] - 0.5f) / 2.0f + 0.5f;
			} else {
				const float z = (a.cam[6] * (pos[0] - p.o[0]) + a.cam[7] * (pos[1] - p.o[1]) + a.cam[8] * (pos[2] - p.o[2])) * a.depth_scale;
				rgb[0] = rgb[1] = rgb[2] = z;
			}
		} else if (a.render_mode == RENDER_AO) {
			rgb[0] = rgb[1] = rgb[2] = alpha;
		} else if (a.render_mode == RENDER_ENCODING_VIS) {
#pragma unroll
			for (int k = 0; k < 3; ++k) rgb[k] = coords[r * 7 + k];  // warped_pos
		} else {
			rgb[0] = network_to_rgb(o0, a.rgb_activation);
			rgb[1] = network_to_rgb(o1, a.rgb_activation);
			rgb[2] = network_to_rgb(o2, a.rgb_activation);
		}
		c[0] += rgb[0] * weight;
		c[1] += rgb[1] * weight;
		c[2] += rgb[2] * weight;
		c[3] += weight;
		if (weight > p.max_weight) p.max_weight = weight;
		if (c[3] > (1.0f - a.min_transmittance)) {
			const float inv = 1.0f / c[3];
			c[0] *= inv; c[1] *= inv; c[2] *= inv; c[3] *= inv;
			break;
		}
	}
	if (j < n_steps) {
		p.alive = 0;
		p.n_steps = j + current_step;
	}
	*(f32x4*)(rgba + 4 * (size_t)i) = c;
}

// shade_kernel_nerf (:2164-2196) into the frame (pre-filled with the linear background), then the
// spp average (the render buffer's accumulation)
__global__ void k_render_shade(uint32_t n_hit, uint32_t linear_colors, uint32_t mode, const Payload* __restrict__ hit,
                               const float* __restrict__ hit_rgba, float* __restrict__ frame) {
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n_hit) return;
	f32x4 c = *(const f32x4*)(hit_rgba + 4 * (size_t)i);
	if (mode == RENDER_NORMALS) {  // (0.5 n + 0.5) * a with n = normalize(rgb)
		const float inv = 1.0f / sqrtf(c[0] * c[0] + c[1] * c[1] + c[2] * c[2]);
		for (int k = 0; k < 3; ++k) c[k] = (0.5f * (c[k] * inv) + 0.5f) * c[3];
	} else if (!linear_colors && mode == RENDER_SHADE) {  // only Shade (and Slice) accumulate in linear colours
		c[0] = srgb_to_linear(c[0]); c[1] = srgb_to_linear(c[1]); c[2] = srgb_to_linear(c[2]);
	}
	float* f = frame + 4 * (size_t)hit[i].idx;
	for (int k = 0; k < 4; ++k) f[k] = c[k] + f[k] * (1.0f - c[3]);
}
__global__ void k_render_fill(uint32_t n, f32x4 bg, float* __restrict__ frame) {
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i < n) *(f32x4*)(frame + 4 * (size_t)i) = bg;
}
// The frame pre-filled with the environment map in each pixel's ray direction (testbed_nerf.cu:2315-2319); the
// direction is the one k_render_init gives the pixel's payload (same operations)
template <bool DIST>
__global__ void k_render_fill_envmap(RenderArgsK<DIST> a, float* __restrict__ frame) {
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	const uint32_t W = a.width, H = a.height;
	if (i >= W * H) return;
	const uint32_t x = i % W, y = i / W;
	float ox, oy;
	ld_random_pixel_offset(a.snap_to_pixel_centers ? 0u : a.sample_index, &ox, &oy);
	const float u = ((float)x + ox) / (float)W, v = ((float)y + oy) / (float)H;
	float dx = (u - a.screen_center[0]) * (float)W / a.focal[0];
	float dy = (v - a.screen_center[1]) * (float)H / a.focal[1];
	lens_undistort(a.lens_mode, a.lens, &dx, &dy);
	if (DIST) {
		const DistMap dm = dist_of(a);
		float fx, fy;
		distortion_offset(dm.data, dm.w, dm.h, u, v, &fx, &fy);
		dx += fx;
		dy += fy;
	}
	const float* m = a.cam;
	const V3 d = v3(m[0] * dx + m[3] * dy + m[6], m[1] * dx + m[4] * dy + m[7], m[2] * dx + m[5] * dy + m[8]);
	const float inv = 1.0f / sqrtf(d.x * d.x + d.y * d.y + d.z * d.z);
	const EnvmapTap t = envmap_lookup(a.env_w, a.env_h, d.x * inv, d.y * inv, d.z * inv);
	const f32x4* em = (const f32x4*)a.envmap;
	const f32x4 e0 = em[t.idx[0]], e1 = em[t.idx[1]], e2 = em[t.idx[2]], e3 = em[t.idx[3]];
	f32x4 c;
	for (int k = 0; k < 4; ++k) c[k] = envmap_mix(t, e0[k], e1[k], e2[k], e3[k]);
	*(f32x4*)(frame + 4 * (size_t)i) = c;
}

// hsv_to_rgb and to_rgb (common_device.cuh:802-827)
__device__ inline void hsv_to_rgb(float h, float s, float v, float rgb[3]) {
	if (s == 0.0f) {
		rgb[0] = rgb[1] = rgb[2] = v;
		return;
	}
	h = fmodf(h, 1.0f) * 6.0f;
	const int i = (int)h;
	const float f = h - (float)i;
	const float p = v * (1.0f - s), q = v * (1.0f - s * f), t = v * (1.0f - s * (1.0f - f));
	switch (i) {
		case 0: rgb[0] = v; rgb[1] = t; rgb[2] = p; break;
		case 1: rgb[0] = q; rgb[1] = v; rgb[2] = p; break;
		case 2: rgb[0] = p; rgb[1] = v; rgb[2] = t; break;
		case 3: rgb[0] = p; rgb[1] = q; rgb[2] = v; break;
		case 4: rgb[0] = t; rgb[1] = p; rgb[2] = v; break;
		default: rgb[0] = v; rgb[1] = p; rgb[2] = q; break;
	}
}
__device__ inline void to_rgb(float x, float y, float rgb[3]) {
	const float PI = 3.14159265358979323846f;
	hsv_to_rgb(atan2f(y, x) / (2.0f * PI) + 0.5f, 1.0f, sqrtf(x * x + y * y), rgb);
}
// ERenderMode::Distortion (testbed_nerf.cu:2331-2344): every pixel to_rgb(offset * 50) with alpha 1, the offset read at
// the pixel's centre; no ray is marched. dm.data null: the offset is zero.
__global__ void k_render_distortion(uint32_t W, uint32_t H, DistMap dm, float* __restrict__ out) {
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= W * H) return;
	const uint32_t x = i % W, y = i / W;
	float ox = 0.0f, oy = 0.0f;
	if (dm.data) distortion_offset(dm.data, dm.w, dm.h, ((float)x + 0.5f) / (float)W, ((float)y + 0.5f) / (float)H, &ox, &oy);
	float rgb[3];
	to_rgb(ox * 50.0f, oy * 50.0f, rgb);
	*(f32x4*)(out + 4 * (size_t)i) = f32x4{rgb[0], rgb[1], rgb[2], 1.0f};
}
__global__ void k_render_accumulate(uint32_t n4, float w, const float* __restrict__ frame, float* __restrict__ acc, bool first) {
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i < n4) acc[i] = (first ? 0.f : acc[i]) + frame[i] * w;
}

void render_frame(const RenderArgs& a, uint32_t spp, RenderWorkspace& ws, const std::function<void(uint32_t, const float*, f16*)>& infer,
                  float* out, hipStream_t s, const std::function<void(uint32_t, float*)>& grad, const DistMap* dist) {
	NGP_CHECK((a.render_mode <= RENDER_DISTORTION || a.render_mode == RENDER_ENCODING_VIS) && (a.render_mode != RENDER_NORMALS || grad),
	          "render: AO, Shade, Normals, Positions, Depth, Distortion and EncodingVis are implemented");
	const uint32_t n_px = a.width * a.height;
	if (n_px == 0) return;
	const DistMap dm = dist && dist->data ? *dist : DistMap{};
	if (a.render_mode == RENDER_DISTORTION) {  // the same frame for every sample: written once
		k_render_distortion<<<div_round_up(n_px, 256), 256, 0, s>>>(a.width, a.height, dm, out);
		NGP_HIP(hipGetLastError());
		return;
	}
	const uint32_t MARCH_ITER = 10000, MIN_STEPS = 1, MAX_STEPS = 8, TARGET_QUERIES = 2 * 1024 * 1024;
	Payload* pay[2] = {(Payload*)ws.payload[0], (Payload*)ws.payload[1]};
	float* rgba[2] = {ws.rgba[0], ws.rgba[1]};
	Payload* hit = (Payload*)ws.payload_hit;
	for (uint32_t sidx = 0; sidx < spp; ++sidx) {
		RenderArgs r = a;
		r.sample_index = a.sample_index + sidx;
		RenderArgsDist rd;  // the DIST forms' arguments
		(RenderArgs&)rd = r;
		rd.dist = dm;
		if (a.envmap && dm.data) k_render_fill_envmap<true><<<div_round_up(n_px, 256), 256, 0, s>>>(rd, ws.frame);
		else if (a.envmap) k_render_fill_envmap<false><<<div_round_up(n_px, 256), 256, 0, s>>>(r, ws.frame);
		else k_render_fill<<<div_round_up(n_px, 256), 256, 0, s>>>(n_px, f32x4{a.background[0], a.background[1], a.background[2],
		                                                                         a.background[3]}, ws.frame);
		if (dm.data) k_render_init<true><<<div_round_up(n_px, 128), 128, 0, s>>>(rd, pay[0], rgba[0]);
		else k_render_init<false><<<div_round_up(n_px, 128), 128, 0, s>>>(r, pay[0], rgba[0]);
		NGP_HIP(hipGetLastError());
		NGP_HIP(hipMemsetAsync(ws.counters, 0, 8, s));  // counters[1]: hits (whole trace)
		uint32_t n_alive = n_px, it = 1, db = 0;
		while (it < MARCH_ITER) {
			Payload* src = pay[db % 2];
			float* src_c = rgba[db % 2];
			Payload* dst = pay[(db + 1) % 2];
			float* dst_c = rgba[(db + 1) % 2];
			++db;
			NGP_HIP(hipMemsetAsync(ws.counters, 0, 4, s));
			k_render_compact<<<div_round_up(n_alive, 256), 256, 0, s>>>(n_alive, src, src_c, dst, dst_c, hit, ws.rgba_hit, ws.counters);
			NGP_HIP(hipGetLastError());
			NGP_HIP(hipMemcpyAsync(ws.host_counters, ws.counters, 8, hipMemcpyDeviceToHost, s));
			NGP_HIP(hipStreamSynchronize(s));
			n_alive = ws.host_counters[0];
			if (n_alive == 0) break;
			const uint32_t n_steps = std::min(std::max(TARGET_QUERIES / n_alive, MIN_STEPS), MAX_STEPS);
			k_render_inputs<<<div_round_up(n_alive, 128), 128, 0, s>>>(r, n_alive, n_steps, dst, ws.coords);
			NGP_HIP(hipGetLastError());
			const uint32_t n_el = next_multiple(n_alive * n_steps, 256);
			infer(n_el, ws.coords, ws.out);
			if (a.render_mode == RENDER_NORMALS) grad(n_el, ws.coords);
			k_render_composite<<<div_round_up(n_alive, 128), 128, 0, s>>>(r, n_alive, n_el, it, n_steps, dst, dst_c, ws.coords, ws.out);
			NGP_HIP(hipGetLastError());
			it += n_steps;
		}
		const uint32_t n_hit = ws.host_counters[1];
		if (n_hit) k_render_shade<<<div_round_up(n_hit, 256), 256, 0, s>>>(n_hit, a.linear_colors, a.render_mode, hit, ws.rgba_hit, ws.frame);
		k_render_accumulate<<<div_round_up(4 * n_px, 256), 256, 0, s>>>(4 * n_px, 1.0f / (float)spp, ws.frame, out, sidx == 0);
		NGP_HIP(hipGetLastError());
	}
}

size_t render_payload_bytes() { return sizeof(Payload); }

}  // namespace nerf
}  // namespace ngp
