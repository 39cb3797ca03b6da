// nerf_device.h — device code shared by the NeRF kernel files (nerf_sampler.hip, nerf_loss.hip, nerf_density_grid.hip,
// nerf_render.hip) and by marching_cubes.hip: cone-angle stepping, voxel advance, mip selection, Morton codes, the
// occupancy test, the network's activations, and the one-block scan the sampler and the loss pass share. A family of
// helpers is here when two of those files use it; a helper with one user stays beside that user. The sRGB curves are in
// ngp_math.h (the image trainer uses them too). Include inside a .hip file only.
//
// Each function cites the reference code it re-implements; float formulas follow the reference line by line (glm vector
// ops written out per component, -ffp-contract=off). Every exp/log whose result decides an integer (cone-angle
// stepping, compositing termination and compaction) is ngp_expf/ngp_logf from ngp_math.h, the same
// instruction sequence the oracle runs, so sample indices, coordinates and compacted counts match the
// oracle bit for bit at every cone angle (the reference's libdevice logf/expf/__expf are <= 2-ulp
// approximations of the same functions).
#pragma once
#include "nerf.h"
#include "ngp_math.h"
#include "render_common.h"

namespace ngp {
namespace nerf {

// ------------------------------------------------------------------------------------------------
// device math
// ------------------------------------------------------------------------------------------------

// t / MIN_CONE_STEPSIZE, correctly rounded, in three instructions: q = t * RN(1/c) and one residual
// correction. Checked exhaustively against the IEEE quotient for every float t >= 0
// (tools/microbench/div_check.c): equal for 1.5e-31 <= t <= 5.7e35; outside that the IEEE divide runs.
// Both the quotient and the residual step are odd in t, so the same holds for -t (the linear segment
// below `at` divides t - at <= 0).
__device__ __forceinline__ float div_min_stepsize(float t) {
	constexpr float c = MIN_CONE_STEPSIZE;
	const float r = 1.0f / c;  // folded to RN(1/c) at compile time
	const float at = fabsf(t);
	if (__builtin_expect(at >= 1e-30f && at <= 1e35f, 1)) {
		const float q = t * r;
		return __builtin_fmaf(__builtin_fmaf(-q, c, t), r, q);
	}
	return t / c;
}
// x / MAX_CONE_STEPSIZE: MAX = MIN * 2^10 exactly, so (barring subnormals, excluded by the range test)
// RN(x / MAX) = RN(x / MIN) * 2^-10.
static_assert(MAX_CONE_STEPSIZE == MIN_CONE_STEPSIZE * 1024.0f, "MAX_CONE_STEPSIZE = MIN * 2^10");
__device__ __forceinline__ float div_max_stepsize(float t) {
	const float at = fabsf(t);
	if (__builtin_expect(at >= 1e-30f && at <= 1e35f, 1)) return div_min_stepsize(t) * (1.0f / 1024.0f);
	return t / MAX_CONE_STEPSIZE;
}

// testbed_nerf.cu:114-184. The constants of a cone angle (log(1 + cone), the two linear segments'
// bounds) are computed once per ray or thread (make_cone), not at every step: with the shared
// software logf/expf (ngp_math.h) they are ~10 transcendental evaluations per call. Same operations
// and values as evaluating them inline.
struct Cone {
	float c, log1p_c, a, b, at, bt, rl;  // rl = RN(1 / log1p_c)
};
// host and device: the sampler computes it once per launch on the host (same ngp_math.h operations)
__host__ __device__ inline Cone make_cone(float c) {
	Cone k{c, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
	if (c <= 1e-5f) return k;
	k.log1p_c = ngp_logf(1.0f + c);
	k.rl = 1.0f / k.log1p_c;
	k.a = (ngp_logf(MIN_CONE_STEPSIZE) - ngp_logf(k.log1p_c)) / k.log1p_c;
	k.b = (ngp_logf(MAX_CONE_STEPSIZE) - ngp_logf(k.log1p_c)) / k.log1p_c;
	k.at = ngp_expf(k.a * k.log1p_c);
	k.bt = ngp_expf(k.b * k.log1p_c);
	return k;
}
__device__ inline float to_stepping_space(float t, const Cone& k) {
	if (k.c <= 1e-5f) return div_min_stepsize(t);
	if (t <= k.at) return div_min_stepsize(t - k.at) + k.a;
	if (t <= k.bt) return ngp_div_rc(ngp_logf_pos(t), k.log1p_c, k.rl);  // at < t <= bt: positive, normal
	return div_max_stepsize(t - k.bt) + k.b;
}
__device__ inline float from_stepping_space(float n, const Cone& k) {
	if (k.c <= 1e-5f) return n * MIN_CONE_STEPSIZE;
	if (n <= k.a) return (n - k.a) * MIN_CONE_STEPSIZE + k.at;
	if (n <= k.b) return ngp_expf_mid(n * k.log1p_c);  // a l < n l <= b l, i.e. log(at) .. log(bt): |.| << 80
	return (n - k.b) * MAX_CONE_STEPSIZE + k.bt;
}
__device__ __forceinline__ float advance_n_steps(float t, const Cone& k, float n) { return from_stepping_space(to_stepping_space(t, k) + n, k); }
__device__ __forceinline__ float calc_dt(float t, const Cone& k) { return advance_n_steps(t, k, 1.0f) - t; }

__device__ __forceinline__ float signf_(float v) { return v > 0.f ? 1.f : (v < 0.f ? -1.f : 0.f); }  // glm::sign

// testbed_nerf.cu:272-315
__device__ inline float distance_to_next_voxel(V3 pos, V3 dir, V3 idir, float res) {
	const V3 p = v3(res * (pos.x - 0.5f), res * (pos.y - 0.5f), res * (pos.z - 0.5f));
	const float tx = (floorf(p.x + 0.5f + 0.5f * signf_(dir.x)) - p.x) * idir.x;
	const float ty = (floorf(p.y + 0.5f + 0.5f * signf_(dir.y)) - p.y) * idir.y;
	const float tz = (floorf(p.z + 0.5f + 0.5f * signf_(dir.z)) - p.z) * idir.z;
	const float t = fminf(fminf(tx, ty), tz);
	return fmaxf(t * (1.0f / res), 0.0f);  // res is a power of two: same rounding as t / res, no IEEE divide
}
// n_t = to_stepping_space(t): callers that already hold it (the sampler's empty-space march, which
// also needs it for calc_dt) pass it in.
__device__ __forceinline__ float advance_to_next_voxel_n(float t, float n_t, const Cone& cone, V3 pos, V3 dir, V3 idir, uint32_t mip) {
	const float res = scalbnf((float)GRIDSIZE, -(int)mip);
	const float t_target = to_stepping_space(t + distance_to_next_voxel(pos, dir, idir, res), cone);
	return from_stepping_space(n_t + ceilf(fmaxf(t_target - n_t, 0.5f)), cone);
}
__device__ inline float advance_to_next_voxel(float t, const Cone& cone, V3 pos, V3 dir, V3 idir, uint32_t mip) {
	return advance_to_next_voxel_n(t, to_stepping_space(t, cone), cone, pos, dir, idir, mip);
}

// testbed_nerf.cu:614-633
__device__ inline uint32_t mip_from_pos(V3 pos, uint32_t max_cascade) {
	int exponent;
	const float maxval = fmaxf(fmaxf(fabsf(pos.x - 0.5f), fabsf(pos.y - 0.5f)), fabsf(pos.z - 0.5f));
	frexpf(maxval, &exponent);
	const int e = exponent + 1;
	return (uint32_t)(e < 0 ? 0 : (e > (int)max_cascade ? (int)max_cascade : e));
}
__device__ inline uint32_t mip_from_dt(float dt, V3 pos, uint32_t max_cascade) {
	const uint32_t mip = mip_from_pos(pos, max_cascade);
	dt *= 2 * GRIDSIZE;
	if (dt < 1.0f) return mip;
	int exponent;
	frexpf(dt, &exponent);
	int v = (int)mip > exponent ? (int)mip : exponent;  // tcnn::clamp(mip, exponent, max_cascade)
	return (uint32_t)(v < (int)max_cascade ? v : (int)max_cascade);
}

__device__ __forceinline__ uint32_t expand_bits(uint32_t v) {
	v = (v * 0x00010001u) & 0xFF0000FFu;
	v = (v * 0x00000101u) & 0x0F00F00Fu;
	v = (v * 0x00000011u) & 0xC30C30C3u;
	v = (v * 0x00000005u) & 0x49249249u;
	return v;
}
// tcnn morton3D: x in bit 0 (consistent with morton3D_invert(idx >> 0) = x, testbed_nerf.cu:518-520)
__device__ __forceinline__ uint32_t morton3D(uint32_t x, uint32_t y, uint32_t z) {
	return expand_bits(x) | (expand_bits(y) << 1) | (expand_bits(z) << 2);
}
__device__ __forceinline__ uint32_t morton3D_invert(uint32_t x) {
	x = x & 0x49249249u;
	x = (x | (x >> 2)) & 0xc30c30c3u;
	x = (x | (x >> 4)) & 0x0f00f00fu;
	x = (x | (x >> 8)) & 0xff0000ffu;
	x = (x | (x >> 16)) & 0x0000ffffu;
	return x;
}

// testbed_nerf.cu:433-457
__device__ inline uint32_t cascaded_grid_idx_at(V3 pos, uint32_t mip) {
	const float mip_scale = scalbnf(1.0f, -(int)mip);
	pos = v3((pos.x - 0.5f) * mip_scale + 0.5f, (pos.y - 0.5f) * mip_scale + 0.5f, (pos.z - 0.5f) * mip_scale + 0.5f);
	const int ix = (int)(pos.x * (float)GRIDSIZE), iy = (int)(pos.y * (float)GRIDSIZE), iz = (int)(pos.z * (float)GRIDSIZE);
	if (ix < 0 || ix >= (int)GRIDSIZE || iy < 0 || iy >= (int)GRIDSIZE || iz < 0 || iz >= (int)GRIDSIZE) return 0xFFFFFFFFu;
	return morton3D((uint32_t)ix, (uint32_t)iy, (uint32_t)iz);
}
__device__ inline bool density_grid_occupied_at(V3 pos, const uint8_t* bitfield, uint32_t mip) {
	const uint32_t idx = cascaded_grid_idx_at(pos, mip);
	if (idx == 0xFFFFFFFFu) return false;
	return bitfield[idx / 8 + GRID_N_CELLS * mip / 8] & (1 << (idx % 8));
}

__device__ __forceinline__ float warp_dt(float dt) {  // :413-416
	const float max_stepsize = MIN_CONE_STEPSIZE * (1 << (CASCADES - 1));
	return (dt - MIN_CONE_STEPSIZE) / (max_stepsize - MIN_CONE_STEPSIZE);
}
__device__ __forceinline__ float unwarp_dt(float dt) {  // :418-421
	const float max_stepsize = MIN_CONE_STEPSIZE * (1 << (CASCADES - 1));
	return dt * (max_stepsize - MIN_CONE_STEPSIZE) + MIN_CONE_STEPSIZE;
}

__device__ __forceinline__ float logistic(float x) { return 1.0f / (1.0f + ngp_expf_fast(-x)); }  // tcnn::logistic
// testbed_nerf.cu:317-378 (the reference's __expf; ngp_expf here and in the oracle)
__device__ inline float network_to_rgb(float v, uint32_t act) {
	switch (act) {
		case ACT_NONE: return v;
		case ACT_RELU: return v > 0.0f ? v : 0.0f;
		case ACT_LOGISTIC: return logistic(v);
		case ACT_EXP: return ngp_expf_mid(fminf(fmaxf(v, -10.0f), 10.0f));
	}
	return 0.0f;
}
__device__ inline float network_to_rgb_derivative(float v, uint32_t act) {
	switch (act) {
		case ACT_NONE: return 1.0f;
		case ACT_RELU: return v > 0.0f ? 1.0f : 0.0f;
		case ACT_LOGISTIC: { const float d = logistic(v); return d * (1 - d); }
		case ACT_EXP: return ngp_expf_mid(fminf(fmaxf(v, -10.0f), 10.0f));
	}
	return 0.0f;
}
__device__ inline float network_to_density(float v, uint32_t act) {
	switch (act) {
		case ACT_NONE: return v;
		case ACT_RELU: return v > 0.0f ? v : 0.0f;
		case ACT_LOGISTIC: return logistic(v);
		case ACT_EXP: return ngp_expf_fast(v);
	}
	return 0.0f;
}
__device__ inline float network_to_density_derivative(float v, uint32_t act) {
	switch (act) {
		case ACT_NONE: return 1.0f;
		case ACT_RELU: return v > 0.0f ? 1.0f : 0.0f;
		case ACT_LOGISTIC: { const float d = logistic(v); return d * (1 - d); }
		case ACT_EXP: return ngp_expf_mid(fminf(fmaxf(v, -15.0f), 15.0f));
	}
	return 0.0f;
}

__device__ __forceinline__ Aabb cfg_aabb(const ngp_nerf_config& c) {
	return Aabb{v3(c.aabb_min[0], c.aabb_min[1], c.aabb_min[2]), v3(c.aabb_max[0], c.aabb_max[1], c.aabb_max[2])};
}

// image_idx and nerf_random_image_pos_training (testbed_nerf.cu:1292-1338): training_pixel (nerf_pixel.h)

__device__ __forceinline__ uint64_t pixel_index(float u, float v, uint32_t w, uint32_t h) {  // image_pos + pixel_idx
	int px = (int)(u * (float)w), py = (int)(v * (float)h);
	px = px < 0 ? 0 : (px > (int)w - 1 ? (int)w - 1 : px);
	py = py < 0 ? 0 : (py > (int)h - 1 ? (int)h - 1 : py);
	return (uint64_t)px + (uint64_t)py * w;
}

// read_rgba's Half and Float branches (common_device.cuh:905-912): the texel as it is stored, one 8-byte load and four
// conversions, or one 16-byte load
__device__ __forceinline__ f32x4 read_hdr_texel(const ImageRef& im, uint64_t idx) {
	if (im.type == IMAGE_FLOAT) return ((const f32x4*)im.data)[idx];
	const f16x4 h = ((const f16x4*)im.data)[idx];
	return f32x4{(float)h[0], (float)h[1], (float)h[2], (float)h[3]};
}

// Single-workgroup scans of one step's per-wave / per-group sums (the sampler's count waves, the loss's groups of
// 4 rays: ~2-8 K values at ~32 K rays): one launch of 1024 threads, tiles of 4096 values, 4 consecutive ones per
// thread (16-B coalesced loads and stores), one block scan per tile. Round 6: they replaced scans over every
// ray (one single-block scan of up to 8 tiles, or above 32 K rays a device-wide hipcub scan: 2 launches per
// scan, and 3 scans per step).
constexpr uint32_t SCAN1_THREADS = 1024, SCAN1_TILE = 4 * SCAN1_THREADS;
// exclusive sum of one value per thread over the block, and the block total; lds: 32 words
__device__ __forceinline__ uint32_t block_exclusive_sum(uint32_t v, uint32_t* lds, uint32_t* total) {
	constexpr uint32_t NW = SCAN1_THREADS / 64;
	const uint32_t lane = threadIdx.x & 63, w = threadIdx.x >> 6;
	uint32_t x = v;
#pragma unroll
	for (uint32_t d = 1; d < 64; d <<= 1) {
		const uint32_t y = __shfl_up(x, d, 64);
		if (lane >= d) x += y;
	}
	if (lane == 63) lds[w] = x;
	__syncthreads();
	if (w == 0) {
		uint32_t y = lane < NW ? lds[lane] : 0u;
#pragma unroll
		for (uint32_t d = 1; d < NW; d <<= 1) {
			const uint32_t z = __shfl_up(y, d, 64);
			if (lane >= d) y += z;
		}
		if (lane < NW) lds[NW + lane] = y;  // inclusive
	}
	__syncthreads();
	const uint32_t r = (w ? lds[NW + w - 1] : 0u) + x - v;
	*total = lds[2 * NW - 1];
	__syncthreads();
	return r;
}
__device__ __forceinline__ void scan1_load(const uint32_t* in, uint32_t n, uint32_t i, uint32_t v[4]) {
	if (i + 3 < n && ((uintptr_t)in & 15) == 0) {
		const uint4 q = *(const uint4*)(in + i);
		v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
	} else {
#pragma unroll
		for (uint32_t k = 0; k < 4; ++k) v[k] = i + k < n ? in[i + k] : 0u;
	}
}
__device__ __forceinline__ void scan1_store(uint32_t* out, uint32_t n, uint32_t i, const uint32_t v[4]) {
	if (i + 3 < n && ((uintptr_t)out & 15) == 0) {
		*(uint4*)(out + i) = uint4{v[0], v[1], v[2], v[3]};
	} else {
#pragma unroll
		for (uint32_t k = 0; k < 4; ++k)
			if (i + k < n) out[i + k] = v[k];
	}
}

}  // namespace nerf
}  // namespace ngp
