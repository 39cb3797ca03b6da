// sdf_render.hip — the SDF sphere tracer, its shading and the IoU counters (see sdf_render.h), and their C-ABI
// (ngp_sdf_render*, ngp_sdf_iou_accumulate). Each kernel cites the reference kernel it re-implements; glm vector
// operations are written out per component in glm's order (dot = x + y + z of the products, normalize = v * (1 / sqrt(dot)),
// double-typed literals of the reference keep their double arithmetic).
#include <algorithm>
#include <cmath>
#include <cstring>

#include "abi_guard.h"
#include "lens.h"
#include "nerf.h"
#include "render_common.h"
#include "sdf_render.h"

namespace ngp {
namespace sdf {

using nerf::Aabb;
using nerf::V3;
using nerf::v3;
using nerf::aabb_contains;
using nerf::aabb_ray_intersect;

namespace {

constexpr float FMAX = 3.402823466e+38f;  // aabb_ray_intersect's "no intersection"

__device__ __forceinline__ float dot3(V3 a, V3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
__device__ __forceinline__ V3 normalize3(V3 v) {
	const float inv = 1.0f / sqrtf(dot3(v, v));
	return v3(v.x * inv, v.y * inv, v.z * inv);
}
__device__ __forceinline__ V3 load3(const float* p, uint32_t i) { return v3(p[3 * (size_t)i], p[3 * (size_t)i + 1], p[3 * (size_t)i + 2]); }
__device__ __forceinline__ void store3(float* p, uint32_t i, V3 v) {
	p[3 * (size_t)i] = v.x; p[3 * (size_t)i + 1] = v.y; p[3 * (size_t)i + 2] = v.z;
}

struct TraceArgs {  // what the trace kernels share
	Aabb box;        // m_aabb inflated by zero_offset
	float zero_offset, distance_scale, maximum_distance, shadow_sharpness, floor_y;
	V3 sun_dir;      // normalize(m_sun_dir) from the host; shadow rays run along shadow_dir(t)
};
// prepare_shadow_rays normalises the (already normalised) sun direction once more for the payload (:253, 274)
__device__ __forceinline__ V3 shadow_dir(const TraceArgs& t) { return normalize3(t.sun_dir); }

// init_rays_with_payload_kernel_sdf (:508-613) with pixel_to_ray as k_render_init does it (nerf_render.hip): no slice
// plane, aperture, foveation, envmap, hidden-area mask or octree. Also clears the frame and the depth buffer.
__global__ void k_sdf_init_rays(FrameArgs a, TraceArgs t, Rays r, float* __restrict__ frame, float* __restrict__ depth) {
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	const uint32_t W = a.width, H = a.height;
	if (i >= W * H) return;
	const uint32_t x = i % W, y = i / W;
	float ox, oy;
	nerf::ld_random_pixel_offset(a.snap_to_pixel_centers ? 0u : a.sample_index, &ox, &oy);
	const float u = ((float)x + ox) / (float)W, v = ((float)y + oy) / (float)H;
	float dx = (u - a.screen_center[0]) * (float)W / a.focal[0];
	float dy = (v - a.screen_center[1]) * (float)H / a.focal[1];
	lens_undistort(a.lens_mode, a.lens, &dx, &dy);
	const float* m = a.cam;
	V3 d = v3(m[0] * dx + m[3] * dy + m[6], m[1] * dx + m[4] * dy + m[7], m[2] * dx + m[5] * dy + m[8]);
	V3 o = v3(m[9] + d.x * 0.0f, m[10] + d.y * 0.0f, m[11] + d.z * 0.0f);  // m_render_near_distance = 0
	*(f32x4*)(frame + 4 * (size_t)i) = f32x4{a.background[0], a.background[1], a.background[2], a.background[3]};
	depth[i] = MAX_DEPTH;
	d = normalize3(d);
	float tmin, tmax;
	aabb_ray_intersect(t.box, o, d, &tmin, &tmax);
	if (tmin < FMAX) {  // ray.advance(max(tmin, 0) + 1e-6); a ray that misses the box stays at its origin (outside: dead)
		const float adv = fmaxf(tmin, 0.0f) + 1e-6f;
		o = v3(o.x + adv * d.x, o.y + adv * d.y, o.z + adv * d.z);
	}
	store3(r.pos, i, o);
	store3(r.dir, i, d);
	r.idx[i] = i;
	r.n_steps[i] = 0;
	r.alive[i] = tmin < FMAX && aabb_contains(t.box, o) ? 1u : 0u;
}

// compact_kernel_sdf / compact_kernel_shadow_sdf (:376-434). One atomic per wave and list from a 64-lane ballot
// (the reference: one same-address atomic per ray). Camera rays that ended inside the box go to the hit list with
// shadow factor 1; finished shadow rays write min_visibility (0 inside the box) to the hit they started from.
template <bool SHADOW>
__global__ void __launch_bounds__(256) k_sdf_compact(uint32_t n, Rays src, Rays dst, Rays hit, float* __restrict__ hit_shadow, Aabb box,
                                                     uint32_t* __restrict__ counters) {
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	const bool in = i < n;
	V3 p = v3(0.f, 0.f, 0.f);
	bool alive = false;
	if (in) {
		p = load3(src.pos, i);
		alive = src.alive[i] != 0;
	}
	const bool inside = in && !alive && aabb_contains(box, p);
	const bool hitp = !SHADOW && inside;
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
		store3(dst.pos, k, p);
		dst.idx[k] = src.idx[i];
		dst.alive[k] = 1u;
		if (SHADOW) {
			dst.prev[k] = src.prev[i];
			dst.total[k] = src.total[i];
			dst.min_vis[k] = src.min_vis[i];
		} else {
			store3(dst.dir, k, load3(src.dir, i));
			dst.n_steps[k] = src.n_steps[i];
		}
	} else if (SHADOW) {
		if (in) hit_shadow[src.idx[i]] = inside ? 0.0f : src.min_vis[i];  // by pixel
	} else if (hitp) {
		const uint32_t k = bh + (uint32_t)__popcll(mh & below);
		store3(hit.pos, k, p);
		store3(hit.dir, k, load3(src.dir, i));
		hit.idx[k] = src.idx[i];
		hit.n_steps[k] = src.n_steps[i];
		hit_shadow[src.idx[i]] = 1.0f;  // by pixel; distances encode the shadowing factor when shading (:432)
	}
}

// advance_pos_kernel_sdf (:149-220) without the octree. T: f16 (the network's SoA row 0) or float (the mesh)
template <typename T, bool SHADOW>
__global__ void k_sdf_advance(uint32_t n, const T* __restrict__ distances, Rays r, TraceArgs t) {
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n) return;
	if (!r.alive[i]) return;
	float distance = (float)distances[i] - t.zero_offset;
	distance *= t.distance_scale;
	const V3 dir = SHADOW ? shadow_dir(t) : load3(r.dir, i);
	V3 pos = load3(r.pos, i);
	pos = v3(pos.x + distance * dir.x, pos.y + distance * dir.y, pos.z + distance * dir.z);
	bool alive = true;
	if (pos.y < t.floor_y && dir.y < 0.f) {
		const float floor_dist = -(pos.y - t.floor_y) / dir.y;
		distance += floor_dist;
		pos = v3(pos.x + floor_dist * dir.x, pos.y + floor_dist * dir.y, pos.z + floor_dist * dir.z);
		alive = false;
	}
	store3(r.pos, i, pos);
	if (SHADOW && distance > 0.0f) {
		// https://www.iquilezles.org/www/articles/rmshadows/rmshadows.htm
		const float total_distance = r.total[i];
		const float y = distance * distance / (2.0f * r.prev[i]);
		const float d = sqrtf(distance * distance - y * y);
		r.min_vis[i] = fminf(r.min_vis[i], t.shadow_sharpness * d / fmaxf(0.0f, total_distance - y));
		r.prev[i] = distance;
		r.total[i] = total_distance + distance;
	}
	const bool stay_alive = distance > t.maximum_distance && fabsf(distance / 2) > 3 * t.maximum_distance;
	if (!stay_alive || !aabb_contains(t.box, pos)) {
		r.alive[i] = 0u;
		return;
	}
	if (!alive) r.alive[i] = 0u;  // the floor ends the ray, yet the step below still counts (:188-193, 219)
	if (!SHADOW) r.n_steps[i] += 1u;
}

// FiniteDifferenceNormalsApproximator::normal (:853-881): the six taps in one launch, the differences in another
__global__ void k_sdf_fd_taps(uint32_t n, uint32_t n_cap, const float* __restrict__ pos, float eps, float* __restrict__ taps) {
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n) return;
	const V3 p = load3(pos, i);
	const size_t S = 3 * (size_t)n_cap;
	store3(taps, i, v3(p.x + eps, p.y, p.z));
	store3(taps + S, i, v3(p.x, p.y + eps, p.z));
	store3(taps + 2 * S, i, v3(p.x, p.y, p.z + eps));
	store3(taps + 3 * S, i, v3(p.x - eps, p.y, p.z));
	store3(taps + 4 * S, i, v3(p.x, p.y - eps, p.z));
	store3(taps + 5 * S, i, v3(p.x, p.y, p.z - eps));
}
template <typename T>
__global__ void k_sdf_fd_normals(uint32_t n, uint32_t n_cap, const T* __restrict__ d, float* __restrict__ normal) {
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n) return;
	const size_t S = n_cap;
	store3(normal, i, v3((float)d[i] - (float)d[3 * S + i], (float)d[S + i] - (float)d[4 * S + i], (float)d[2 * S + i] - (float)d[5 * S + i]));
}

// prepare_shadow_rays (:233-296): one shadow ray per camera hit, its index the hit's pixel. A ray that starts
// outside the box is parked at a finite point outside it (the reference leaves it wherever FLT_MAX took it).
__global__ void k_sdf_prepare_shadow(uint32_t n, Rays hit, const float* __restrict__ normals, Rays r, TraceArgs t) {
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n) return;
	const V3 nrm = load3(normals, i), rd = load3(hit.dir, i);
	// step back a little along the ray to prevent self-intersection: faceforward(N, I, Nref) = dot(Nref, I) < 0 ? N : -N
	V3 ff = dot3(nrm, rd) < 0.f ? nrm : v3(-nrm.x, -nrm.y, -nrm.z);
	ff = normalize3(ff);
	V3 p = load3(hit.pos, i);
	p = v3(p.x + ff.x * 1e-3f, p.y + ff.y * 1e-3f, p.z + ff.z * 1e-3f);
	const V3 dir = shadow_dir(t);
	float tmin, tmax;
	aabb_ray_intersect(t.box, p, dir, &tmin, &tmax);
	bool alive = tmin < FMAX;
	if (alive) {
		const float adv = fmaxf(tmin + 1e-6f, 0.0f);
		p = v3(p.x + adv * dir.x, p.y + adv * dir.y, p.z + adv * dir.z);
		alive = aabb_contains(t.box, p);
	}
	if (!alive) p = v3(t.box.mx.x + 1.0f, t.box.mx.y + 1.0f, t.box.mx.z + 1.0f);
	store3(r.pos, i, p);
	r.idx[i] = hit.idx[i];
	r.alive[i] = alive ? 1u : 0u;
	r.prev[i] = 1e20f;
	r.total[i] = 0.0f;
	r.min_vis[i] = 1.0f;
}

// ---- shading (:47-147) --------------------------------------------------------------------------
constexpr float PI_F = 3.14159265358979323846f;
__device__ __forceinline__ float square(float x) { return x * x; }
__device__ __forceinline__ float mixf(float a, float b, float t) { return a + (b - a) * t; }
__device__ __forceinline__ V3 mix3(V3 a, V3 b, float t) { return v3(a.x + (b.x - a.x) * t, a.y + (b.y - a.y) * t, a.z + (b.z - a.z) * t); }
__device__ __forceinline__ float saturate(float x) { return fminf(fmaxf(x, 0.0f), 1.0f); }
__device__ __forceinline__ float schlick_fresnel(float u) {
	const float m = saturate((float)(1.0 - (double)u));
	return square(square(m)) * m;
}
__device__ __forceinline__ float g1(float NdotH, float a) {
	if (a >= 1.0) return (float)(1.0 / (double)PI_F);
	const float a2 = square(a);
	const float t = (float)(1.0 + ((double)a2 - 1.0) * (double)NdotH * (double)NdotH);
	return (float)(((double)a2 - 1.0) / (double)(PI_F * logf(a2) * t));
}
__device__ __forceinline__ float g2(float NdotH, float a) {
	const float a2 = square(a);
	const float t = (float)(1.0 + ((double)a2 - 1.0) * (double)NdotH * (double)NdotH);
	return a2 / (PI_F * t * t);
}
__device__ __forceinline__ float smith_g_ggx(float NdotV, float alphaG) {
	const float a = alphaG * alphaG;
	const float b = NdotV * NdotV;
	return (float)(1.0 / (double)(NdotV + sqrtf(a + b - a * b)));
}
// evaluate_shading (:78-147), after the Disney BRDF
__device__ V3 evaluate_shading(V3 base_color, V3 ambient_color, V3 light_color, float metallic, float subsurface, float specular,
                               float roughness, float specular_tint, float sheen, float sheen_tint, float clearcoat,
                               float clearcoat_gloss, V3 L, V3 V, V3 N) {
	const float NdotL = dot3(N, L);
	const float NdotV = dot3(N, V);
	const V3 H = normalize3(v3(L.x + V.x, L.y + V.y, L.z + V.z));
	const float NdotH = dot3(N, H);
	const float LdotH = dot3(L, H);
	const float FL = schlick_fresnel(NdotL), FV = schlick_fresnel(NdotV);
	const float am = mixf(0.2f, FV, metallic);
	V3 amb = v3(ambient_color.x * am, ambient_color.y * am, ambient_color.z * am);
	amb = v3(amb.x * base_color.x, amb.y * base_color.y, amb.z * base_color.z);
	if (NdotL < 0.f || NdotV < 0.f) return amb;
	const float luminance = dot3(base_color, v3(0.3f, 0.6f, 0.1f));
	const float il = 1.f / (luminance + 0.00001f);
	const V3 Ctint = v3(base_color.x * il, base_color.y * il, base_color.z * il);
	const V3 one = v3(1.0f, 1.0f, 1.0f);
	V3 c0 = mix3(one, Ctint, specular_tint);
	c0 = v3(c0.x * specular * 0.08f, c0.y * specular * 0.08f, c0.z * specular * 0.08f);
	const V3 Cspec0 = mix3(c0, base_color, metallic);
	const V3 Csheen = mix3(one, Ctint, sheen_tint);
	const float Fd90 = 0.5f + 2.0f * LdotH * LdotH * roughness;
	const float Fd = mixf(1, Fd90, FL) * mixf(1.f, Fd90, FV);
	const float Fss90 = LdotH * LdotH * roughness;
	const float Fss = mixf(1.0f, Fss90, FL) * mixf(1.0f, Fss90, FV);
	const float ss = 1.25f * (Fss * (1.f / (NdotL + NdotV) - 0.5f) + 0.5f);
	const float a = fmaxf(0.001f, square(roughness));
	const float Ds = g2(NdotH, a);
	const float FH = schlick_fresnel(LdotH);
	const V3 Fs = mix3(Cspec0, one, FH);
	const float Gs = smith_g_ggx(NdotL, a) * smith_g_ggx(NdotV, a);
	const float fs = FH * sheen;
	const V3 Fsheen = v3(fs * Csheen.x, fs * Csheen.y, fs * Csheen.z);
	const float Dr = g1(NdotH, mixf(0.1f, 0.001f, clearcoat_gloss));
	const float Fr = mixf(0.04f, 1.0f, FH);
	const float Gr = smith_g_ggx(NdotL, 0.25f) * smith_g_ggx(NdotV, 0.25f);
	const float CCs = 0.25f * clearcoat * Gr * Fr * Dr;
	const float diff = (float)(1.0f / PI_F) * mixf(Fd, ss, subsurface);
	const float om = 1.0f - metallic;
	const float brdf[3] = {(diff * base_color.x + Fsheen.x) * om + Gs * Fs.x * Ds + CCs, (diff * base_color.y + Fsheen.y) * om + Gs * Fs.y * Ds + CCs,
	                       (diff * base_color.z + Fsheen.z) * om + Gs * Fs.z * Ds + CCs};
	return v3(brdf[0] * light_color.x * NdotL + amb.x, brdf[1] * light_color.y * NdotL + amb.y, brdf[2] * light_color.z * NdotL + amb.z);
}

// shade_kernel_sdf (:298-374): AO, Shade, Normals, Positions, Depth, Cost. The box is m_aabb, not the inflated one.
__global__ void k_sdf_shade(uint32_t n, FrameArgs a, Rays hit, const float* __restrict__ normals, const float* __restrict__ shadow,
                            float* __restrict__ frame, float* __restrict__ depth) {
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n) return;
	const Aabb box{v3(a.aabb_min[0], a.aabb_min[1], a.aabb_min[2]), v3(a.aabb_max[0], a.aabb_max[1], a.aabb_max[2])};
	const V3 pos = load3(hit.pos, i);
	if (!aabb_contains(box, pos)) return;
	const V3 dir = load3(hit.dir, i);
	const uint32_t n_steps = hit.n_steps[i];
	const uint32_t mode = a.render_mode;
	V3 normal = v3(0.f, 0.f, 0.f);
	if (mode == MODE_SHADE || mode == MODE_NORMALS) normal = normalize3(load3(normals, i));  // not normalised in memory
	bool floor = false;
	if (pos.y < a.floor_y + 0.001f && dir.y < 0.f) {
		normal = v3(0.f, 1.f, 0.f);
		floor = true;
	}
	const V3 cam_pos = v3(a.cam[9], a.cam[10], a.cam[11]), cam_fwd = v3(a.cam[6], a.cam[7], a.cam[8]);
	const float z = dot3(cam_fwd, v3(pos.x - cam_pos.x, pos.y - cam_pos.y, pos.z - cam_pos.z));
	V3 color = v3(0.f, 0.f, 0.f);
	switch (mode) {
	case MODE_AO: {
		const float c = powf(0.92f, (float)n_steps);
		color = v3(c, c, c);
	} break;
	case MODE_SHADE: {
		const V3 sun = v3(a.sun_dir[0], a.sun_dir[1], a.sun_dir[2]), up = v3(a.up_dir[0], a.up_dir[1], a.up_dir[2]);
		const float skyam = -dot3(normal, up) * 0.5f + 0.5f;
		const float sh = shadow[hit.idx[i]];  // 0 = occluded, 1 = no shadow
		const V3 suncol = v3(255.f / 255.0f * 4.f * sh, 225.f / 255.0f * 4.f * sh, 195.f / 255.0f * 4.f * sh);
		const V3 skycol = v3(195.f / 255.0f * 4.f * skyam, 215.f / 255.0f * 4.f * skyam, 255.f / 255.0f * 4.f * skyam);
		const float check_size = 8.f / (box.mx.x - box.mn.x);
		const float check = (((int)floorf(check_size * (pos.x - box.mn.x)) ^ (int)floorf(check_size * (pos.z - box.mn.z))) & 1) ? 0.8f : 0.2f;
		const V3 floorcol = v3(check * check * check, check * check, check);
		const float* b = a.brdf;
		const V3 base = v3(b[7] * b[7], b[8] * b[8], b[9] * b[9]);
		const V3 ambient = v3(b[10] * skycol.x, b[11] * skycol.y, b[12] * skycol.z);
		const V3 nd = normalize3(dir);
		color = evaluate_shading(floor ? floorcol : base, ambient, suncol, floor ? 0.f : b[0], floor ? 0.f : b[1], floor ? 1.f : b[2],
		                         floor ? 0.5f : b[3], 0.f, floor ? 0.f : b[4], 0.f, floor ? 0.f : b[5], b[6], sun, v3(-nd.x, -nd.y, -nd.z),
		                         normal);
	} break;
	case MODE_DEPTH: color = v3(z, z, z); break;
	case MODE_POSITIONS: color = v3((pos.x - 0.5f) / 2.0f + 0.5f, (pos.y - 0.5f) / 2.0f + 0.5f, (pos.z - 0.5f) / 2.0f + 0.5f); break;
	case MODE_NORMALS: color = v3(0.5f * normal.x + 0.5f, 0.5f * normal.y + 0.5f, 0.5f * normal.z + 0.5f); break;
	case MODE_COST: {
		const float c = (float)n_steps / 30;
		color = v3(c, c, c);
	} break;
	default: break;
	}
	const uint32_t px = hit.idx[i];
	*(f32x4*)(frame + 4 * (size_t)px) = f32x4{color.x, color.y, color.z, 1.0f};
	depth[px] = z;
}

__global__ void k_sdf_accumulate(uint32_t n, float w, const float* __restrict__ src, float* __restrict__ acc, bool first) {
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i < n) acc[i] = (first ? 0.f : acc[i]) + src[i] * w;
}

// compare_signs_kernel (:474-492) without the octree: [0]/[1] reference inside/outside, [2]/[3] model inside/outside,
// [4] both inside, [5] either inside, [6] outside the octree (none), [7] samples. Ballots count per wave, lanes 0..7
// of each wave add one counter each at the end of the wave's grid-stride loop.
__global__ void __launch_bounds__(256) k_sdf_iou(uint32_t n, const float* __restrict__ ref, const float* __restrict__ model,
                                                 uint32_t* __restrict__ counters) {
	uint32_t c[8] = {0, 0, 0, 0, 0, 0, 0, 0};
	for (uint64_t base = (uint64_t)blockIdx.x * blockDim.x; base < n; base += (uint64_t)gridDim.x * blockDim.x) {
		const uint64_t i = base + threadIdx.x;
		const bool in = i < n;
		const bool inside1 = in && ref[i] <= 0.f, inside2 = in && model[i] <= 0.f;
		const uint64_t mv = __ballot(in), m1 = __ballot(inside1), m2 = __ballot(inside2);
		c[0] += (uint32_t)__popcll(m1);
		c[1] += (uint32_t)__popcll(mv & ~m1);
		c[2] += (uint32_t)__popcll(m2);
		c[3] += (uint32_t)__popcll(mv & ~m2);
		c[4] += (uint32_t)__popcll(m1 & m2);
		c[5] += (uint32_t)__popcll(m1 | m2);
		c[7] += (uint32_t)__popcll(mv);
	}
	const uint32_t lane = __lane_id();
	uint32_t mine = 0;
#pragma unroll
	for (uint32_t k = 0; k < 8; ++k) mine = lane == k ? c[k] : mine;
	if (lane < 8 && mine) atomicAdd(&counters[lane], mine);
}
// scale_iou_counters_kernel (:494-499)
__global__ void k_sdf_iou_scale(uint32_t* __restrict__ counters, float scale) {
	const uint32_t i = threadIdx.x;
	if (i < 8) counters[i] = (uint32_t)roundf(counters[i] * scale);
}

uint32_t blocks(uint32_t n, uint32_t b = 256) { return div_round_up(n, b); }

// SphereTracer::trace (:707-799): compact, min(i, 4) rounds of {distance, advance}, until nothing is alive or the
// iteration cap. Returns the hits the compactions collected (camera rays). Rays start in ws.rays[0].
template <bool SHADOW>
uint32_t trace(uint32_t n_rays, const TraceArgs& t, uint32_t max_iterations, Workspace& ws, const DistanceFn& fn, hipStream_t s) {
	if (n_rays == 0) return 0;
	NGP_HIP(hipMemsetAsync(ws.counters, 0, 8, s));
	ws.host_counters[1] = 0;
	const uint32_t STEPS_INBETWEEN_COMPACTION = 4;
	uint32_t n_alive = n_rays, i = 1, db = 0;
	while (i < max_iterations) {
		const uint32_t step_size = std::min(i, STEPS_INBETWEEN_COMPACTION);
		Rays& cur = ws.rays[(db + 1) % 2];
		Rays& tmp = ws.rays[db % 2];
		++db;
		NGP_HIP(hipMemsetAsync(ws.counters, 0, 4, s));
		k_sdf_compact<SHADOW><<<blocks(n_alive), 256, 0, s>>>(n_alive, tmp, cur, ws.hit, ws.hit_shadow, t.box, ws.counters);
		NGP_HIP(hipGetLastError());
		NGP_HIP(hipMemcpyAsync(ws.host_counters, ws.counters, 8, hipMemcpyDeviceToHost, s));
		NGP_HIP(hipStreamSynchronize(s));
		n_alive = ws.host_counters[0];
		if (n_alive == 0) break;
		NGP_CHECK(n_alive <= n_rays, "sdf trace: more rays alive than were started");
		const uint32_t n_pad = next_multiple(n_alive, BATCH_GRANULARITY);
		for (uint32_t j = 0; j < step_size; ++j) {
			fn.eval(n_alive, n_pad, cur.pos, cur.idx, ws.dist32);
			if (fn.half_out) k_sdf_advance<f16, SHADOW><<<blocks(n_alive), 256, 0, s>>>(n_alive, ws.out16, cur, t);
			else k_sdf_advance<float, SHADOW><<<blocks(n_alive), 256, 0, s>>>(n_alive, ws.dist32, cur, t);
			NGP_HIP(hipGetLastError());
		}
		i += step_size;
	}
	return ws.host_counters[1];
}

}  // namespace

void render_frame(const FrameArgs& a, uint32_t spp, Workspace& ws, const DistanceFn& fn, float* out_rgba, float* out_depth,
                  hipStream_t s) {
	const uint32_t n_px = a.width * a.height;
	if (n_px == 0) return;
	NGP_CHECK(n_px <= ws.n_cap, "sdf render: workspace too small");
	TraceArgs t{};
	t.box = Aabb{V3{a.aabb_min[0] - a.zero_offset, a.aabb_min[1] - a.zero_offset, a.aabb_min[2] - a.zero_offset},
	             V3{a.aabb_max[0] + a.zero_offset, a.aabb_max[1] + a.zero_offset, a.aabb_max[2] + a.zero_offset}};
	t.zero_offset = a.zero_offset;
	t.distance_scale = a.distance_scale;
	t.maximum_distance = a.maximum_distance;
	t.shadow_sharpness = a.shadow_sharpness;
	t.floor_y = a.floor_y;
	t.sun_dir = V3{a.sun_dir[0], a.sun_dir[1], a.sun_dir[2]};
	for (uint32_t sidx = 0; sidx < spp; ++sidx) {
		FrameArgs r = a;
		r.sample_index = a.sample_index + sidx;
		k_sdf_init_rays<<<blocks(n_px, 128), 128, 0, s>>>(r, t, ws.rays[0], ws.frame, ws.depth);
		NGP_HIP(hipGetLastError());
		const uint32_t n_hit = trace<false>(n_px, t, a.max_iterations, ws, fn, s);
		if (n_hit) {
			NGP_CHECK(n_hit <= n_px, "sdf render: more hits than pixels");
			const uint32_t n_pad = next_multiple(n_hit, BATCH_GRANULARITY);
			if (a.render_mode == MODE_SHADE || a.render_mode == MODE_NORMALS) {
				if (a.analytic_normals && fn.gradient) {
					fn.gradient(n_pad, ws.hit.pos, ws.hit_normal);
				} else {
					k_sdf_fd_taps<<<blocks(n_hit), 256, 0, s>>>(n_hit, ws.n_cap, ws.hit.pos, a.fd_normals_epsilon, ws.fd_pos);
					NGP_HIP(hipGetLastError());
					for (uint32_t k = 0; k < 6; ++k) {
						const float* taps = ws.fd_pos + 3 * (size_t)ws.n_cap * k;
						if (fn.half_out) {
							fn.eval(n_hit, n_pad, taps, ws.hit.idx, nullptr);
							NGP_HIP(hipMemcpyAsync((f16*)ws.fd_dist + (size_t)ws.n_cap * k, ws.out16, (size_t)n_hit * sizeof(f16),
							                       hipMemcpyDeviceToDevice, s));
						} else {
							fn.eval(n_hit, n_pad, taps, ws.hit.idx, (float*)ws.fd_dist + (size_t)ws.n_cap * k);
						}
					}
					if (fn.half_out) k_sdf_fd_normals<f16><<<blocks(n_hit), 256, 0, s>>>(n_hit, ws.n_cap, (const f16*)ws.fd_dist, ws.hit_normal);
					else k_sdf_fd_normals<float><<<blocks(n_hit), 256, 0, s>>>(n_hit, ws.n_cap, (const float*)ws.fd_dist, ws.hit_normal);
					NGP_HIP(hipGetLastError());
				}
				if (a.render_mode == MODE_SHADE) {
					// shadow rays towards the sun (:989-1022): a second trace with the shadow recurrence
					k_sdf_prepare_shadow<<<blocks(n_hit), 256, 0, s>>>(n_hit, ws.hit, ws.hit_normal, ws.rays[0], t);
					NGP_HIP(hipGetLastError());
					trace<true>(n_hit, t, a.max_iterations, ws, fn, s);
				}
			}
			k_sdf_shade<<<blocks(n_hit), 256, 0, s>>>(n_hit, r, ws.hit, ws.hit_normal, ws.hit_shadow, ws.frame, ws.depth);
			NGP_HIP(hipGetLastError());
		}
		k_sdf_accumulate<<<blocks(4 * n_px), 256, 0, s>>>(4 * n_px, 1.0f / (float)spp, ws.frame, out_rgba, sidx == 0);
		if (out_depth) k_sdf_accumulate<<<blocks(n_px), 256, 0, s>>>(n_px, 1.0f / (float)spp, ws.depth, out_depth, sidx == 0);
		NGP_HIP(hipGetLastError());
	}
}

void iou_accumulate(uint32_t n, const float* distances_ref, const float* distances_model, float scale_existing, uint32_t* counters,
                    hipStream_t s) {
	if (scale_existing < 1.f) k_sdf_iou_scale<<<1, 64, 0, s>>>(counters, scale_existing);
	if (n) k_sdf_iou<<<std::min(blocks(n), 2048u), 256, 0, s>>>(n, distances_ref, distances_model, counters);
	NGP_HIP(hipGetLastError());
}

}  // namespace sdf
}  // namespace ngp

// ---- C-ABI ------------------------------------------------------------------------------------------
using namespace ngp;

namespace {
struct Buf {  // grows on demand; new memory is zeroed so that padded batch rows hold finite positions
	void* p = nullptr;
	size_t n = 0;
	template <typename T> T* get(size_t count) {
		const size_t need = std::max<size_t>(count * sizeof(T), 16);
		if (need > n) {
			if (p) NGP_HIP(hipFree(p));
			p = nullptr;
			n = 0;
			NGP_HIP(hipMalloc(&p, need));
			n = need;
			NGP_HIP(hipMemset(p, 0, need));
		}
		return (T*)p;
	}
	~Buf() { if (p) (void)hipFree(p); }
};
int invalid(const char* what) {
	ngp::set_last_error(what);
	return NGP_INVALID;
}
void normalize_host(const float* v, float* out) {  // glm::normalize on the host (render_sdf :1041-1042)
	const float inv = 1.0f / std::sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
	for (int k = 0; k < 3; ++k) out[k] = v[k] * inv;
}
}  // namespace

struct ngp_sdf_renderer {
	Buf f32, u32, out16;
	uint32_t* host_counters = nullptr;
	~ngp_sdf_renderer() { if (host_counters) (void)hipHostFree(host_counters); }
};

extern "C" {

int ngp_sdf_render_default_config(ngp_sdf_render_config* out) {
	if (!out) return invalid("ngp_sdf_render_default_config: null config");
	std::memset(out, 0, sizeof(*out));
	for (int k = 0; k < 3; ++k) { out->aabb_min[k] = 0.f; out->aabb_max[k] = 1.f; }
	out->zero_offset = 0.f;              // testbed.h:830
	out->distance_scale = 0.95f;         // :831
	out->maximum_distance = 0.00005f;    // :800
	out->fd_normals_epsilon = 0.0005f;   // :801
	out->shadow_sharpness = 2048.0f;     // :799
	out->analytic_normals = 0;           // :829
	out->floor_enable = 0;               // :916
	out->snap_to_pixel_centers = 0;      // m_snap_to_pixel_centers (testbed.h)
	out->max_iterations = 10000;         // MARCH_ITER (testbed_sdf.cu:37)
	const float one[3] = {1.f, 1.f, 1.f};
	normalize_host(one, out->sun_dir);   // testbed.h:602
	out->up_dir[0] = 0.f; out->up_dir[1] = 1.f; out->up_dir[2] = 0.f;  // :601
	out->metallic = 0.f; out->subsurface = 0.f; out->specular = 1.f; out->roughness = 0.5f;  // BRDFParams (sdf.h:62-72)
	out->sheen = 0.f; out->clearcoat = 0.f; out->clearcoat_gloss = 0.f;
	for (int k = 0; k < 3; ++k) { out->basecolor[k] = 0.8f; out->ambientcolor[k] = 0.f; }
	return NGP_OK;
}

int ngp_sdf_renderer_create(ngp_sdf_renderer** out) {
	if (!out) return invalid("ngp_sdf_renderer_create: null output");
	NGP_TRY({
		*out = new ngp_sdf_renderer();
	});
}
void ngp_sdf_renderer_destroy(ngp_sdf_renderer* r) { delete r; }

int ngp_sdf_render(ngp_sdf_renderer* r, ngp_model* model, ngp_sdf_mesh* ground_truth, const ngp_sdf_render_config* cfg, void* stream,
                   const ngp_nerf_image* camera, int render_mode, uint32_t spp, uint32_t sample_index, const float* background_rgba,
                   int use_inference_params, float* out_rgba, float* out_depth) {
	if (!r || !cfg || !camera || !out_rgba) return invalid("ngp_sdf_render: null argument");
	if ((model != nullptr) == (ground_truth != nullptr)) return invalid("ngp_sdf_render: exactly one of model / ground_truth");
	if (!sdf::mode_supported(render_mode)) return invalid("ngp_sdf_render: AO, Shade, Normals, Positions, Depth and Cost are implemented");
	if (spp == 0 || camera->width == 0 || camera->height == 0 || (uint64_t)camera->width * camera->height > (1u << 28))
		return invalid("ngp_sdf_render: empty or oversized frame");
	if (camera->lens_mode > LENS_OPENCV_FISHEYE) return invalid("ngp_sdf_render: unsupported lens mode");
	NGP_TRY({
		hipStream_t s = (hipStream_t)stream;
		sdf::FrameArgs a{};
		a.width = camera->width; a.height = camera->height;
		a.focal[0] = camera->focal_length[0]; a.focal[1] = camera->focal_length[1];
		// the screen centre as ngp_nerf_render derives it: render_screen_center(1 - principal point) = the principal point
		for (int k = 0; k < 2; ++k) a.screen_center[k] = (0.5f - (1.0f - camera->principal_point[k])) * 1.0f + 0.5f;
		nerf::effective_camera_matrix(camera->xform, a.cam);
		a.lens_mode = camera->lens_mode;
		for (int k = 0; k < 4; ++k) a.lens[k] = camera->lens_params[k];
		a.sample_index = sample_index;
		a.snap_to_pixel_centers = cfg->snap_to_pixel_centers;
		for (int k = 0; k < 3; ++k) { a.aabb_min[k] = cfg->aabb_min[k]; a.aabb_max[k] = cfg->aabb_max[k]; }
		a.zero_offset = cfg->zero_offset;
		a.distance_scale = cfg->distance_scale;
		a.maximum_distance = cfg->maximum_distance;
		a.fd_normals_epsilon = cfg->fd_normals_epsilon;
		a.shadow_sharpness = cfg->shadow_sharpness;
		a.analytic_normals = cfg->analytic_normals;
		a.max_iterations = cfg->max_iterations;
		a.floor_y = cfg->floor_enable ? cfg->aabb_min[1] + 0.001f : -10000.f;  // get_floor_y (testbed.h:917)
		normalize_host(cfg->sun_dir, a.sun_dir);
		normalize_host(cfg->up_dir, a.up_dir);
		const float brdf[13] = {cfg->metallic, cfg->subsurface, cfg->specular, cfg->roughness, cfg->sheen, cfg->clearcoat,
		                        cfg->clearcoat_gloss, cfg->basecolor[0], cfg->basecolor[1], cfg->basecolor[2], cfg->ambientcolor[0],
		                        cfg->ambientcolor[1], cfg->ambientcolor[2]};
		std::memcpy(a.brdf, brdf, sizeof(brdf));
		for (int k = 0; k < 4; ++k) a.background[k] = background_rgba ? background_rgba[k] : 0.f;
		a.render_mode = (uint32_t)render_mode;

		const uint32_t n_px = a.width * a.height;
		const size_t N = next_multiple(n_px, sdf::BATCH_GRANULARITY);
		sdf::Workspace ws{};
		ws.n_cap = (uint32_t)N;
		// floats: 2 x {pos 3, dir 3, prev, total, min_vis} + hit {pos 3, dir 3} + shadow 1 + normal 3 + taps 18 + tap distances 6
		// + distances 1 + frame 4 + depth 1
		float* f = r->f32.get<float>(N * (2 * 9 + 6 + 1 + 3 + 18 + 6 + 1 + 4 + 1));
		uint32_t* u = r->u32.get<uint32_t>(N * (2 * 3 + 2) + 2);
		for (int k = 0; k < 2; ++k) {
			sdf::Rays& q = ws.rays[k];
			q.pos = f; f += 3 * N;
			q.dir = f; f += 3 * N;
			q.prev = f; f += N;
			q.total = f; f += N;
			q.min_vis = f; f += N;
			q.idx = u; u += N;
			q.n_steps = u; u += N;
			q.alive = u; u += N;
		}
		ws.hit.pos = f; f += 3 * N;
		ws.hit.dir = f; f += 3 * N;
		ws.hit.idx = u; u += N;
		ws.hit.n_steps = u; u += N;
		ws.counters = u;
		ws.hit_shadow = f; f += N;
		ws.hit_normal = f; f += 3 * N;
		ws.fd_pos = f; f += 18 * N;
		ws.fd_dist = f; f += 6 * N;
		ws.dist32 = f; f += N;
		ws.frame = f; f += 4 * N;
		ws.depth = f;
		ws.out16 = model ? r->out16.get<f16>(16 * N) : nullptr;
		if (!r->host_counters) NGP_HIP(hipHostMalloc(&r->host_counters, 16));
		ws.host_counters = r->host_counters;

		sdf::DistanceFn fn;
		fn.half_out = model != nullptr;
		if (model) {
			// SoA: output row 0, the distance, is n contiguous halves that the kernels read in place
			fn.eval = [&](uint32_t, uint32_t n_pad, const float* pos, const uint32_t*, float*) {
				check_rc(ngp_inference(model, s, n_pad, pos, 3, ws.out16, n_pad, NGP_LAYOUT_SOA, use_inference_params));
			};
			// Network::input_gradient(stream, 0, positions, normals) (testbed.cu:4621), tcnn's default backprop_scale
			fn.gradient = [&](uint32_t n_pad, const float* pos, float* normals) {
				check_rc(ngp_input_gradient(model, s, 0, n_pad, pos, 3, normals, 3, 128.0f));
			};
		} else {
			fn.eval = [&](uint32_t n, uint32_t, const float* pos, const uint32_t* pixel, float* out32) {
				check_rc(ngp_sdf_signed_distance_rows(ground_truth, s, n, pos, pixel, out32));
			};
		}
		sdf::render_frame(a, spp, ws, fn, out_rgba, out_depth, s);
	});
}

int ngp_sdf_iou_accumulate(void* stream, uint32_t n, const float* distances_ref, const float* distances_model, float scale_existing,
                           uint32_t* counters) {
	if (!counters || (n > 0 && (!distances_ref || !distances_model))) return invalid("ngp_sdf_iou_accumulate: null argument");
	NGP_TRY({
		sdf::iou_accumulate(n, distances_ref, distances_model, scale_existing, counters, (hipStream_t)stream);
	});
}

}  // extern "C"
