// nerf_sampler.hip — the NeRF training sampler for gfx950 (see nerf.h): the ray-parallel march of the count pass, the
// scan over its waves, the write pass, and the training pixels' stand-alone form. The NGP_SAMPLER_DIAG instrumentation
// lives here whole (its __device__ counters and their reader must share one translation unit).
#include <cmath>
#include <cstring>
#include <utility>

#include "nerf_device.h"
#include "profiler.h"
#include "rng.h"
#include "nerf_pixel.h"
#include "distortion.h"

namespace ngp {
namespace nerf {

// Ray setup shared by the sampler's two passes (testbed_nerf.cu:1415-1493).
struct RaySetup {
	bool valid;
	V3 o, d, dn, idir;
	float startt, cone;
};

// CDF: the ray's pixel comes from the error map's CDFs `e` (a separate instantiation: the uniform one carries none of it)
// TEX: the dataset holds a Half or Float image (Dataset::tex): `pixels` is then the image table, ImageRef [n_images],
// and the texel is read by its image's type; otherwise it is the packed RGBA8 buffer
// DIST: the distortion map `dm` adds its offset at the ray's (u, v) to dir.xy after the lens (uv_to_ray,
// common_device.cuh:443-510); the rng draws and the pixel choice are those of the form without it
template <bool CDF, bool TEX, bool DIST>
__device__ RaySetup setup_ray(const Camera* cams, const void* pixels, uint32_t n_images, const ngp_nerf_config& cfg,
                              uint32_t ig, uint32_t n_rays_div, Rng rng, const Cone& cone, const ErrorCdfs& e, const DistMap& dm) {
	RaySetup r;
	r.valid = false;
	pcg_advance(rng, (uint64_t)ig * N_MAX_RANDOM_SAMPLES_PER_RAY);
	const TrainPixel px = training_pixel<CDF>(cams, n_images, cfg.snap_to_pixel_centers != 0, e, ig, n_rays_div, rng);
	const Camera& cam = cams[px.img];
	const float u = px.u, v = px.v;
	if (TEX) {  // a texel whose red is < 0 is masked (testbed_nerf.cu:1430-1435); a Byte one decodes to that at 0x00FF00FF
		const ImageRef im = ((const ImageRef*)pixels)[px.img];
		const uint64_t idx = pixel_index(u, v, cam.width, cam.height);
		if (im.type == IMAGE_BYTE) {
			if (((const uint32_t*)im.data)[idx] == 0x00FF00FFu) return r;
		} else if (read_hdr_texel(im, idx)[0] < 0.0f) {
			return r;
		}
	} else {
		const uint32_t raw = ((const uint32_t*)pixels)[cam.pixel_offset + pixel_index(u, v, cam.width, cam.height)];
		if (raw == 0x00FF00FFu) return r;  // masked (read_rgba returns -1)
	}
	(void)pcg_float(rng);              // motionblur_time
	// uv_to_ray (common_device.cuh:443-510): pinhole, then the lens undistortion
	float dx = (u - cam.principal[0]) * (float)cam.width / cam.focal[0];
	float dy = (v - cam.principal[1]) * (float)cam.height / cam.focal[1];
	lens_undistort(cam.lens_mode, cam.lens, &dx, &dy);
	if (DIST) {
		float ox, oy;
		distortion_offset(dm.data, dm.w, dm.h, u, v, &ox, &oy);
		dx += ox;
		dy += oy;
	}
	const float dz = 1.0f;
	const float* m = cam.m;
	r.d = v3(m[0] * dx + m[3] * dy + m[6] * dz, m[1] * dx + m[4] * dy + m[7] * dz, m[2] * dx + m[5] * dy + m[8] * dz);
	r.o = v3(m[9], m[10], m[11]);
	const float inv = 1.0f / sqrtf(r.d.x * r.d.x + r.d.y * r.d.y + r.d.z * r.d.z);
	r.dn = v3(r.d.x * inv, r.d.y * inv, r.d.z * inv);
	float tmin, tmax;
	aabb_ray_intersect(cfg_aabb(cfg), r.o, r.dn, &tmin, &tmax);
	r.cone = cfg.cone_angle_constant;
	tmin = fmaxf(tmin, 0.0f);
	r.startt = advance_n_steps(tmin, cone, pcg_float(rng));
	r.idir = v3(1.0f / r.dn.x, 1.0f / r.dn.y, 1.0f / r.dn.z);
	r.valid = true;
	return r;
}

// Conservative end of sampling along a ray: for t > sampling_end no occupancy test of the sampler can
// succeed, so the count pass stops there with the same result (no exact skip positions are needed
// after the last occupied cell). Found by marching BACKWARD from the aabb exit through the pooled
// bitfield mips: a cell empty at mip m >= the mip the sampler would use there (mip_from_dt) is empty
// at every finer mip (bitfield_max_pool ORs children into parents, testbed_nerf.cu:788-809), and that
// mip never grows as t decreases. The forward march through the trailing empty space (one skip per
// mip-0 voxel, ~70 % of the pass at Lego scale) is replaced by a handful of coarse backward jumps.
// Occupancy of the mip-m cell containing p in the DDA frame (cell boundaries where res*(p - 0.5) is
// an integer, the frame advance_to_next_voxel / the backward jump use), OR-ed with the sampler's own
// classification of p (cascaded_grid_idx_at rounds (p - 0.5) * 2^-m + 0.5, which can land in the
// neighbouring cell within a few ulps of a face): the scan only jumps over cells empty in both.
// Row-cooperative: lane L probes mip mu + L, so the climb to the coarsest empty mip is one parallel
// load round trip instead of up to 7 dependent ones; both classifications are loaded unconditionally.
__device__ __forceinline__ bool scan_occupied_2load(V3 p, const uint8_t* bitfield, uint32_t m) {
	const uint32_t i0 = cascaded_grid_idx_at(p, m);
	const float res = scalbnf((float)GRIDSIZE, -(int)m);
	const int ix = (int)floorf(res * (p.x - 0.5f)) + (int)GRIDSIZE / 2;
	const int iy = (int)floorf(res * (p.y - 0.5f)) + (int)GRIDSIZE / 2;
	const int iz = (int)floorf(res * (p.z - 0.5f)) + (int)GRIDSIZE / 2;
	const bool in1 = !(ix < 0 || ix >= (int)GRIDSIZE || iy < 0 || iy >= (int)GRIDSIZE || iz < 0 || iz >= (int)GRIDSIZE);
	const uint32_t i1 = in1 ? morton3D((uint32_t)ix, (uint32_t)iy, (uint32_t)iz) : 0u;
	const uint32_t j0 = i0 == 0xFFFFFFFFu ? 0u : i0;
	const uint8_t b0 = bitfield[j0 / 8 + GRID_N_CELLS * m / 8], b1 = bitfield[i1 / 8 + GRID_N_CELLS * m / 8];
	return (i0 != 0xFFFFFFFFu && (b0 & (1 << (j0 % 8)))) || (in1 && (b1 & (1 << (i1 % 8))));
}

template <uint32_t G>
__device__ float sampling_end_row(V3 o, V3 d, V3 idir, float t_start, const Cone& cone, const Aabb& box, const uint8_t* bitfield,
                                  uint32_t max_cascade, uint32_t L) {
	static_assert(G >= CASCADES || 2 * G == CASCADES, "one lane per mip, or two");
	float tmin, tmax;
	aabb_ray_intersect(box, o, d, &tmin, &tmax);
	if (!(tmax < 3.0e38f)) return t_start;
	const V3 nd = v3(-d.x, -d.y, -d.z), nidir = v3(-idir.x, -idir.y, -idir.z);
	const uint32_t shift = __lane_id() & (64u - G);
	float t = tmax;
	for (int it = 0; it < 8192; ++it) {
		if (t <= t_start) return t_start;
		const V3 p = v3(o.x + t * d.x, o.y + t * d.y, o.z + t * d.z);
		const uint32_t mu = mip_from_dt(calc_dt(t, cone), p, max_cascade);
		const uint32_t mL = mu + L;
		const bool probe = mL < CASCADES;
		const bool occ = probe && scan_occupied_2load(p, bitfield, probe ? mL : 0u);
		uint32_t bits = (uint32_t)(__ballot(occ) >> shift) & ((1u << G) - 1u);
		if (G < CASCADES) {  // lanes probe mips mu + L and mu + L + G
			const bool probe2 = mL + G < CASCADES;
			const bool occ2 = probe2 && scan_occupied_2load(p, bitfield, probe2 ? mL + G : 0u);
			bits |= ((uint32_t)(__ballot(occ2) >> shift) & ((1u << G) - 1u)) << G;
		}
		if (bits & 1u) return t + 2.0f * SQRT3 / scalbnf((float)GRIDSIZE, -(int)mu);
		const uint32_t m = bits ? mu + __builtin_ctz(bits) - 1u : CASCADES - 1u;
		const float res = scalbnf((float)GRIDSIZE, -(int)m);
		t -= distance_to_next_voxel(p, nd, nidir, res);
		t -= fmaxf(fabsf(t), 1.0f) * 2.5e-7f;
	}
	return 3.402823466e38f;
}

// ------------------------------------------------------------------------------------------------
// Ray-parallel marching. The reference marches one ray per thread (testbed_nerf.cu:1432-1480); at
// ~23 K rays per step that is ~1.4 waves per CU and every step of a long ray waits on one dependent
// bitfield load. Here a ray owns a lane group (RG = 8 lanes, half a DPP row): the group speculates the next RG states
// of the reference's sequential march (all occupied: t += calc_dt(t); or all empty:
// advance_to_next_voxel), tests their occupancy in parallel (one load latency per RG states) and
// keeps the prefix that the sequential march would take, switching speculation mode at the first
// lane that disagrees. The t chain itself is evaluated with the reference's float ops in order (every
// lane of the row evaluates it redundantly), so sample positions stay bit-exact with the sequential
// algorithm. The count pass stores the t of every occupied step (tbuf, STEPS floats per ray) and the
// ray geometry, so the write pass is a flat copy instead of a second march.
// ------------------------------------------------------------------------------------------------
#ifndef NGP_SAMPLER_RG
#define NGP_SAMPLER_RG 8
#endif
constexpr uint32_t RG = NGP_SAMPLER_RG;  // lanes per ray (16 = one DPP row)
#ifndef NGP_SAMPLER_EMPTY_SPEC
#define NGP_SAMPLER_EMPTY_SPEC 1  // cone stepping: one guess-and-verify loop for both modes (0: occupied guess-and-verify, empty chain in every lane)
#endif
#ifndef NGP_SAMPLER_ROUND_CAP
#define NGP_SAMPLER_ROUND_CAP 1  // verify rounds per march iteration (0: until every lane is verified)
#endif
#ifndef NGP_SAMPLER_PRIO
#define NGP_SAMPLER_PRIO 3  // s_setprio of the cone-stepping count pass (it shares the SIMDs with the training pass and
                            // is the fox step's critical path): neutral in round 4, fox -1 % since the early counter
                            // publish starts it under the training pass (gpurun_out/r06bl, r06bm)
#endif
#ifndef NGP_SAMPLER_END_CONE
#define NGP_SAMPLER_END_CONE 0  // sampling_end under cone stepping (off: measured slower with the speculative march)
#endif
#ifndef NGP_SAMPLER_UNIFIED0
#define NGP_SAMPLER_UNIFIED0 1  // the same for cone 0 (0: occupied guess-and-verify, empty chain)
#endif
static_assert(RG >= 4 && RG <= 16 && (RG & (RG - 1)) == 0, "sampler group: 4, 8 or 16 lanes");
#ifndef NGP_SAMPLER_RG0
#define NGP_SAMPLER_RG0 4  // lanes per ray at cone 0 (k_sample_count<true>, the Lego stand-in): 8 -> 4 measured
                           // Lego 0.451-0.453 -> 0.443-0.446 ms per step; the cone-stepping march (fox) stays at
                           // RG (4 there: 0.546 -> 0.605 ms, gpurun_out/r05zzg)
#endif
static_assert(NGP_SAMPLER_RG0 >= 4 && NGP_SAMPLER_RG0 <= 16 && (NGP_SAMPLER_RG0 & (NGP_SAMPLER_RG0 - 1)) == 0,
              "sampler group: 4, 8 or 16 lanes");
template <bool CONE0> constexpr uint32_t sampler_rg() { return CONE0 ? NGP_SAMPLER_RG0 : RG; }
#ifndef NGP_SAMPLER_BLOCK
#define NGP_SAMPLER_BLOCK 256
#endif

template <uint32_t G>
__device__ __forceinline__ uint32_t row_ballot(bool p) {  // this ray's G lanes of a wave ballot
	const unsigned long long b = __ballot(p);
	return (uint32_t)(b >> (__lane_id() & (64u - G))) & ((1u << G) - 1u);
}
__device__ __forceinline__ float dpp_shr1(float v) {  // lane l - 1 of the same DPP row (lane 0 of a row: 0)
	return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x111, 0xF, 0xF, false));
}

struct RayGeo {  // per ray, count pass -> write pass
	float o[3], d[3], dn[3];
	float pad[3];
};

// The march's state transitions. CONE0: cone_angle <= 1e-5 (every aabb_scale 1 scene), where
// to/from_stepping_space are t / MIN_CONE_STEPSIZE and back, calc_dt(t) stays within a few ulps of
// MIN_CONE_STEPSIZE (dt * 2 * GRIDSIZE ~ 0.43 < 1), so mip_from_dt(dt, pos) == mip_from_pos(pos);
// with max_cascade 0 that is mip 0. Same values as the generic path, fewer instructions per state.
template <bool CONE0>
struct Marcher {
	V3 o, dn, idir;
	Cone cone;
	uint32_t max_cascade;
	__device__ __forceinline__ V3 pos(float t) const { return v3(o.x + t * dn.x, o.y + t * dn.y, o.z + t * dn.z); }
	__device__ __forceinline__ Cone k() const { return CONE0 ? Cone{} : cone; }
	__device__ __forceinline__ float dt_at(float t) const { return calc_dt(t, k()); }
	__device__ __forceinline__ uint32_t mip_at(float dt, V3 p) const {
		if (CONE0) return max_cascade == 0 ? 0u : mip_from_pos(p, max_cascade);
		return mip_from_dt(dt, p, max_cascade);
	}
	__device__ __forceinline__ float step_occupied(float t) const { return t + dt_at(t); }
	// advance_to_next_voxel from t, sharing to_stepping_space(t) with calc_dt(t) (same values as
	// evaluating both separately); *mip_out: the mip the sampler tests t's occupancy at.
	// In the exponential segment of the stepping space two of the step's four transcendentals only
	// decide integers: the mip (the binary exponent of calc_dt(t) * 2 GRIDSIZE) and the number of
	// stepping-space steps to the next voxel (a ceil). Both are first taken from hardware exp/log
	// (relative error ~1e-6, bound below) and recomputed exactly only when the approximate value lies
	// within a margin (>= 10x that error) of a decision boundary: same integers as the exact evaluation.
	// Both errors grow like 1 / log(1 + cone) (= cone.rl): the margins scale with it, so a small cone
	// (cone_angle_constant down to 1e-5) simply takes the exact path more often, never a wrong integer.
	__device__ __forceinline__ float step_empty(float t, uint32_t* mip_out = nullptr) const {
		return step_empty_n(t, to_stepping_space(t, k()), mip_out);
	}
	// step_empty given n = to(t) (the verify step has it for every candidate)
	__device__ __forceinline__ float step_empty_n(float t, float n, uint32_t* mip_out = nullptr) const {
		const V3 p = pos(t);
		uint32_t mip;
		if (CONE0) {
			mip = mip_at(0.0f, p);
			if (mip_out) *mip_out = mip;
			return advance_to_next_voxel_n(t, n, k(), p, dn, idir, mip);
		}
		const float c = empty_steps(t, n, p, &mip);
		if (mip_out) *mip_out = mip;
		return from_stepping_space(n + c, cone);
	}
	// Cone stepping: the number of stepping-space steps advance_to_next_voxel takes from t (n = to(t),
	// p = pos(t)), ceil(max(to(target) - n, 0.5)), and t's mip.
	__device__ __forceinline__ float empty_steps(float t, float n, V3 p, uint32_t* mip_out) const {
		const float n1 = n + 1.0f;
		float dt;
		if (n1 > cone.a && n1 <= cone.b) {
			// from_stepping_space(n1) = ngp_expf(n1 * log1p_c); __expf: v_exp_f32 (~2 ulp) of
			// the same argument, so dt * 2 GRIDSIZE is off by <= ~3e-7 * t / dt ~ 3e-7 * rl relative
			// (~8e-5 at cone 1/256). Margin: 13x that, relative to the boundary (mantissa 0.5 = powers of two)
			dt = __expf(n1 * cone.log1p_c) - t;
			int e;
			const float mant = frexpf(dt * (2 * GRIDSIZE), &e);
			const float mm = 3.9e-6f * cone.rl;  // 1e-3 at cone 1/256
			if (mant < 0.5f + 0.5f * mm || mant > 1.0f - mm) dt = from_stepping_space(n1, cone) - t;
		} else {
			dt = from_stepping_space(n1, cone) - t;
		}
		const uint32_t mip = mip_at(dt, p);
		*mip_out = mip;
		const float res = scalbnf((float)GRIDSIZE, -(int)mip);
		const float target = t + distance_to_next_voxel(p, dn, idir, res);
		float x;
		if (target > cone.at && target <= cone.bt) {
			// to_stepping_space(target) = ngp_logf(target) / log1p_c; __logf (v_log_f32) is within
			// ~1e-6 absolute for target in (at, bt], i.e. ~1e-6 * rl stepping-space units (~3e-4 at cone
			// 1/256); margin 15x that (4e-3 at cone 1/256; >= 0.5 below cone ~3e-5: always exact)
			x = __logf(target) * cone.rl - n;
			if (fabsf(x - rintf(x)) < 1.5625e-5f * cone.rl) x = to_stepping_space(target, cone) - n;
		} else {
			x = to_stepping_space(target, cone) - n;
		}
		return ceilf(fmaxf(x, 0.5f));
	}
	// Either mode: the state after t and t's mip. occ: t + calc_dt(t) (calc_dt = from(n + 1)
	// - t); empty: advance_to_next_voxel = from(n + empty_steps). One to() and one from() either way, so
	// a wave whose rays are in different modes evaluates the two software transcendentals once.
	__device__ __forceinline__ float step_any(float t, bool occ, uint32_t* mip_out, float* n_out = nullptr) const {
		const V3 p = pos(t);
		const float n = to_stepping_space(t, k());
		if (n_out) *n_out = n;
		uint32_t mip = CONE0 ? mip_at(0.0f, p) : 0u;
		float c = 1.0f;
		if (!occ) c = CONE0 ? empty_steps0(t, n, p, mip) : empty_steps(t, n, p, &mip);
		const float e = from_stepping_space(n + c, k());
		if (!occ) {
			*mip_out = mip;
			return e;
		}
		const float dt = e - t;
		*mip_out = CONE0 ? mip : mip_at(dt, p);
		return t + dt;
	}
	// cone 0: the steps of advance_to_next_voxel_n (mip: mip_at(0, p))
	__device__ __forceinline__ float empty_steps0(float t, float n, V3 p, uint32_t mip) const {
		const float target = t + distance_to_next_voxel(p, dn, idir, scalbnf((float)GRIDSIZE, -(int)mip));
		return ceilf(fmaxf(to_stepping_space(target, Cone{}) - n, 0.5f));
	}
	// Guesses only (the speculative empty-space march verifies every state they lead to): the
	// stepping-space conversions with hardware exp/log in the exponential segment.
	__device__ __forceinline__ float to_fast(float t) const {
		if (t <= cone.at) return div_min_stepsize(t - cone.at) + cone.a;
		if (t <= cone.bt) return __logf(t) * cone.rl;
		return div_max_stepsize(t - cone.bt) + cone.b;
	}
	__device__ __forceinline__ float from_fast(float n) const {
		if (n <= cone.a) return (n - cone.a) * MIN_CONE_STEPSIZE + cone.at;
		if (n <= cone.b) return __expf(n * cone.log1p_c);
		return (n - cone.b) * MAX_CONE_STEPSIZE + cone.bt;
	}
	// Guess of the state j >= 1 empty-space steps after the exact state (tb, nb = to(tb)), assuming each
	// step crosses one voxel boundary at tb's mip: b_j, the j-th boundary crossing of the ray's DDA from
	// pos(tb), then state j = from(nb + ceil(to(b_j) - nb)); returns that ceil (advance_to_next_voxel from inside the cell
	// before b_j lands on the first lattice point past it; nb plus an integer is exact). No dependency
	// between the lanes' guesses; wrong ones (a mip change, two crossings in one step, a tie at a cell
	// corner) only cost a verify round.
	__device__ __forceinline__ float guess_empty_steps(float tb, float nb, uint32_t j) const {
		const V3 p = pos(tb);
		const float res = scalbnf((float)GRIDSIZE, -(int)mip_at(CONE0 ? 0.0f : from_fast(nb + 1.0f) - tb, p));
		const float qx = res * (p.x - 0.5f), qy = res * (p.y - 0.5f), qz = res * (p.z - 0.5f);
		float sx = (floorf(qx + 0.5f + 0.5f * signf_(dn.x)) - qx) * idir.x;
		float sy = (floorf(qy + 0.5f + 0.5f * signf_(dn.y)) - qy) * idir.y;
		float sz = (floorf(qz + 0.5f + 0.5f * signf_(dn.z)) - qz) * idir.z;
		const float ax = fabsf(idir.x), ay = fabsf(idir.y), az = fabsf(idir.z);
		float s = 0.0f;
#pragma unroll
		for (uint32_t k = 0; k + 1 < sampler_rg<CONE0>(); ++k) {
			if (k < j) {
				s = fminf(fminf(sx, sy), sz);
				if (sx == s) sx += ax;
				else if (sy == s) sy += ay;
				else sz += az;
			}
		}
		const float b = tb + fmaxf(s, 0.0f) * (1.0f / res);
		return ceilf(fmaxf((CONE0 ? to_stepping_space(b, Cone{}) : to_fast(b)) - nb, 0.5f));
	}
};

#if NGP_SAMPLER_DIAG == 4  // instrumentation aid: per-ray march statistics (tools/nerf_step_profile.py --sampler-stats)
// [0] empty iterations [1] occupied iterations [2] occupied verify rounds [3] rays [4] occupied states
// [5] max iterations of one ray [6] empty-mode exits (mode switches) [7] empty verify rounds
// [8 + b] rays with 2^b <= iterations < 2^(b+1); wall_clock64 ticks summed over rays: [40] setup_ray
// [41] sampling_end [42] guess + verify [43] occupancy test [44] whole march loop; [45] max ticks of one ray;
// [46] the initial guesses of the unified loop (part of [42])
__device__ unsigned long long g_sampler_stats[48];
extern "C" __attribute__((visibility("default"))) int ngp_debug_sampler_stats(unsigned long long* out, int n) {
	if (!out) {
		static const unsigned long long z[48] = {};
		return hipMemcpyToSymbol(HIP_SYMBOL(g_sampler_stats), z, sizeof(z)) == hipSuccess ? 0 : -1;
	}
	return hipMemcpyFromSymbol(out, HIP_SYMBOL(g_sampler_stats), sizeof(unsigned long long) * (n < 48 ? n : 48)) == hipSuccess ? 0 : -1;
}
#define SAMPLER_STAT(...) __VA_ARGS__
// a timestamp the scheduler keeps in program order
__device__ __forceinline__ unsigned long long sampler_clock() {
	__builtin_amdgcn_sched_barrier(0);
	const unsigned long long t = wall_clock64();
	__builtin_amdgcn_sched_barrier(0);
	return t;
}
#else
#define SAMPLER_STAT(...)
#endif

// generate_training_samples_nerf pass 1: count the occupied steps of ray i (lane L of its group), keep their t;
// returns the count (uniform over the group).
template <bool CONE0, bool CDF, bool TEX, bool DIST>
__device__ __forceinline__ uint32_t count_ray(const Camera* __restrict__ cams, const void* __restrict__ pixels, uint32_t n_images,
                                              const ngp_nerf_config& cfg, const SampleArgs& a, uint32_t* __restrict__ nsteps,
                                              float* __restrict__ tbuf, RayGeo* __restrict__ geo, const Cone& cone, uint32_t i,
                                              uint32_t L, const DistMap& dm) {
	constexpr uint32_t RGk = sampler_rg<CONE0>();
	if (!CONE0 && NGP_SAMPLER_PRIO) __builtin_amdgcn_s_setprio(NGP_SAMPLER_PRIO);
	SAMPLER_STAT(const unsigned long long ck0 = sampler_clock();)
	const RaySetup r = setup_ray<CDF, TEX, DIST>(cams, pixels, n_images, cfg, i + a.ray_offset, a.n_rays_total_for_image_idx, a.rng, cone,
	                                             a.cdfs, dm);
	SAMPLER_STAT(const unsigned long long ck1 = sampler_clock(); unsigned long long ck2 = ck1, ck_g = 0, ck_o = 0, ck_q = 0;)
	uint32_t j = 0;
	if (r.valid) {
		const Aabb box = cfg_aabb(cfg);
		const Marcher<CONE0> m{r.o, r.dn, r.idir, cone, cfg.max_cascade};
		float t = r.startt;
#if NGP_SAMPLER_DIAG == 2
		const float t_end = 3.0e38f;
#else
		// Under cone stepping the speculative march crosses trailing empty space faster than the backward
		// scan finds its start (fox: 0.356 ms with it, 0.334 without, profiles/r03ak); at cone 0 it pays.
		const float t_end = (CONE0 || NGP_SAMPLER_END_CONE)
		                        ? sampling_end_row<RGk>(r.o, r.dn, r.idir, t, m.cone, box, a.bitfield, cfg.max_cascade, L)
		                        : 3.0e38f;
#endif
#if NGP_SAMPLER_DIAG == 1  // timing aid: sampling_end twice (cost of one = difference to the default build)
		const float t_end2 = sampling_end_row<RGk>(r.o, r.dn, r.idir, t + 0.0f * t_end, m.cone, box, a.bitfield, cfg.max_cascade, L);
		if (t_end2 != t_end) t = t_end2;
#endif
		float* tout = tbuf + (size_t)i * STEPS;
		bool occ_mode = false;  // rays enter the aabb in empty space far more often than not
		bool have_n0 = false;   // unified loop: n0_next = to(t) is known (the verify step computed it for the new state)
		float n0_next = 0.f;
		SAMPLER_STAT(ck2 = sampler_clock();)
		SAMPLER_STAT(uint32_t st_e = 0; uint32_t st_o = 0; uint32_t st_r = 0; uint32_t st_x = 0; uint32_t st_q = 0;)
		for (;;) {
			SAMPLER_STAT(if (occ_mode) ++st_o; else ++st_e; const unsigned long long cka = sampler_clock();)
			// lanes [0, nvalid) take the next nvalid states of the sequential march, assuming it stays in
			// the current mode (all occupied / all empty)
			float tl, last;  // last: the state after lane nvalid-1's (the march continues there if every lane stays in the mode)
			uint32_t mipl;   // the mip lane L's state is tested at
			float nk = 0.f;  // unified loop: to(tl), from its verify step (reused when the ray leaves an occupied run at this lane)
			uint32_t nvalid = RGk;  // lanes holding verified states
			if (CONE0 ? NGP_SAMPLER_UNIFIED0 : NGP_SAMPLER_EMPTY_SPEC) {
				// Both modes in one guess-and-verify loop. Every state is from(n + c) with n =
				// to(previous state): c = 1 in an occupied run (t + calc_dt(t)), c = the ceil of
				// advance_to_next_voxel in an empty one. Lane L guesses state L as from(to(t) + C_L): C_L = L
				// when occupied (to(from(n)) == n nearly always), the voxel DDA's estimate when empty
				// (guess_empty_steps). All lanes verify at once: lane L redoes the exact step from lane L-1's
				// guess. The verified prefix is exact; the first lane that fails takes the exact state from its
				// predecessor and the lanes after it are re-guessed from there. The rays of a wave sit in
				// different modes most of the time; sharing the loop (and its exact to()/from() per lane and
				// round) means the wave no longer runs one mode's loop after the other's.
				const float n0 = have_n0 ? n0_next : to_stepping_space(t, m.k());
				have_n0 = false;
				const float c0 = occ_mode ? (float)L : m.guess_empty_steps(t, n0, L);
				float cand = L == 0 ? t : from_stepping_space(n0 + c0, m.k());
				SAMPLER_STAT(ck_q += sampler_clock() - cka;)
				uint32_t v0 = 1, mk = 0, rounds = 0;
				float nxt, tcap = 0.0f;
				for (;;) {
					SAMPLER_STAT(if (occ_mode) ++st_r; else ++st_q;)
					nxt = m.step_any(cand, occ_mode, &mk, &nk);
					const float expct = dpp_shr1(nxt);
					const uint32_t v = __builtin_ctz(row_ballot<RGk>(L >= v0 && __float_as_uint(expct) != __float_as_uint(cand)) | (1u << RGk));
					if (v >= RGk) break;
					const float tv = __shfl(expct, (int)v, (int)RGk);
					// The wave runs the loop until its slowest ray is verified. After NGP_SAMPLER_ROUND_CAP rounds a
					// ray keeps its verified prefix (lanes < v) and continues from tv (the exact state after it)
					// in the next iteration.
					if (NGP_SAMPLER_ROUND_CAP && ++rounds >= NGP_SAMPLER_ROUND_CAP) {
						nvalid = v;
						tcap = tv;
						break;
					}
					const float nv = to_stepping_space(tv, m.k());
					const float cv = occ_mode ? (float)(L - v) : m.guess_empty_steps(tv, nv, L - v);
					cand = L < v ? cand : (L == v ? tv : from_stepping_space(nv + cv, m.k()));
					v0 = v + 1;
				}
				tl = cand;
				mipl = mk;
				last = __shfl(nxt, (int)(RGk - 1), (int)RGk);
				if (nvalid < RGk) last = tcap;
			} else if (occ_mode) {
				// Occupied run: t_{k+1} = t_k + calc_dt(t_k) = from(to(t_k) + 1) in stepping space, and
				// to(from(n)) == n nearly always. Guess state L as from(to(t) + L) and verify every guess at
				// once (lane L redoes the exact step from lane L-1's state): the verified prefix is exact; the
				// first lane that fails takes the exact state from its verified predecessor and the lanes
				// after it are re-guessed from there. Each round verifies at least one more lane, most runs
				// take one round instead of a chain of RGk dependent steps.
				const float n0 = to_stepping_space(t, m.k());
				float cand = L == 0 ? t : from_stepping_space(n0 + (float)L, m.k());
				uint32_t v0 = 1;
				float dt, nxt;
				for (;;) {
					SAMPLER_STAT(++st_r;)
					dt = m.dt_at(cand);
					nxt = cand + dt;  // step_occupied(cand)
					const float expct = dpp_shr1(nxt);
					const uint32_t v = __builtin_ctz(row_ballot<RGk>(L >= v0 && __float_as_uint(expct) != __float_as_uint(cand)) | (1u << RGk));
					if (v >= RGk) break;
					const float tv = __shfl(expct, (int)v, (int)RGk);
					cand = L < v ? cand : (L == v ? tv : from_stepping_space(to_stepping_space(tv, m.k()) + (float)(L - v), m.k()));
					v0 = v + 1;
				}
				tl = cand;
				mipl = m.mip_at(CONE0 ? 0.0f : dt, m.pos(tl));
				last = __shfl(nxt, (int)(RGk - 1), (int)RGk);
			} else {
				// empty space: the chain evaluated in order by every lane of the group; lane L keeps state L
				float tk = t;
				tl = t;
				mipl = 0;
#pragma unroll 1  // rolled: the unrolled chain (8 inlined steps) overflowed the instruction cache
				for (uint32_t kk = 0; kk < RGk; ++kk) {
					uint32_t mk;
					const float tn = m.step_empty(tk, &mk);
					if (L == kk) { tl = tk; mipl = mk; }
					tk = tn;
				}
				last = tk;
			}
			SAMPLER_STAT(const unsigned long long ckb = sampler_clock(); ck_g += ckb - cka;)
			const V3 pos = m.pos(tl);
			const uint32_t mip = mipl;
			const bool inside = L < nvalid && tl <= t_end && aabb_contains(box, pos) && (occ_mode ? j + L : j) < STEPS;
			const bool occ = inside && density_grid_occupied_at(pos, a.bitfield, mip);
			const uint32_t cont = row_ballot<RGk>(inside && occ == occ_mode);
			const uint32_t f = __builtin_ctz(~cont | (1u << RGk));  // first lane the sequential march leaves the mode at
			SAMPLER_STAT(ck_o += sampler_clock() - ckb;)
			if (occ_mode) {
#if NGP_SAMPLER_DIAG == 5  // timing aid: every occupied state stored twice (mirrored copy; cost of the stores)
				if (L < f) { tout[j + L] = tl; tout[STEPS - 1 - (j + L)] = tl; }
#else
				if (L < f) tout[j + L] = tl;
#endif
				j += f;
			}
			if (f >= nvalid) {  // every state taken stayed in the mode: continue after the last one
				t = last;
				continue;
			}
			if (!((row_ballot<RGk>(inside) >> f) & 1u)) break;  // left the aabb / sampling range / step budget
			const float tf = __shfl(tl, (int)f, (int)RGk);
			if (occ_mode) {  // empty cell at lane f: advance_to_next_voxel
				// cone stepping: lane f's to() from its verify step (at cone 0 to() is a multiply, cheaper than the shuffle)
				if (!CONE0 && NGP_SAMPLER_EMPTY_SPEC) t = m.step_empty_n(tf, __shfl(nk, (int)f, (int)RGk));
				else t = m.step_empty(tf);
			}
			else {  // occupied cell at lane f: sample it next
				t = tf;
				if (!CONE0 && NGP_SAMPLER_EMPTY_SPEC) {
					n0_next = __shfl(nk, (int)f, (int)RGk);
					have_n0 = true;
				}
			}
			SAMPLER_STAT(st_x += occ_mode ? 0u : 1u;)
			occ_mode = !occ_mode;
		}
		SAMPLER_STAT(if (L == 0) {
			atomicAdd(&g_sampler_stats[0], (unsigned long long)st_e);
			atomicAdd(&g_sampler_stats[1], (unsigned long long)st_o);
			atomicAdd(&g_sampler_stats[2], (unsigned long long)st_r);
			atomicAdd(&g_sampler_stats[3], 1ull);
			atomicAdd(&g_sampler_stats[4], (unsigned long long)j);
			atomicMax(&g_sampler_stats[5], (unsigned long long)(st_e + st_o));
			atomicAdd(&g_sampler_stats[6], (unsigned long long)st_x);
			atomicAdd(&g_sampler_stats[7], (unsigned long long)st_q);
			atomicAdd(&g_sampler_stats[8 + (31 - __builtin_clz(st_e + st_o))], 1ull);
			const unsigned long long ck3 = sampler_clock();
			atomicAdd(&g_sampler_stats[40], ck1 - ck0);
			atomicAdd(&g_sampler_stats[41], ck2 - ck1);
			atomicAdd(&g_sampler_stats[42], ck_g);
			atomicAdd(&g_sampler_stats[43], ck_o);
			atomicAdd(&g_sampler_stats[44], ck3 - ck2);
			atomicMax(&g_sampler_stats[45], ck3 - ck0);
			atomicAdd(&g_sampler_stats[46], ck_q);
		})
	}
	if (L == 0) {
		nsteps[i] = j;
		RayGeo g;
		g.o[0] = r.o.x; g.o[1] = r.o.y; g.o[2] = r.o.z;
		g.d[0] = r.d.x; g.d[1] = r.d.y; g.d[2] = r.d.z;
		g.dn[0] = r.dn.x; g.dn[1] = r.dn.y; g.dn[2] = r.dn.z;
		g.pad[0] = r.cone; g.pad[1] = g.pad[2] = 0.f;
		geo[i] = g;
	}
	return j;
}

__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
#pragma unroll
	for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
	return v;
}

// The count pass, and per wave the sum of its rays' counts and the number of its rays with samples (wsum[2 w],
// wsum[2 w + 1]): the sampler's prefix sums over rays become a scan over waves (k_sample_bscan, ~2 K values at
// the Lego stand-in's ~32 K rays) plus an in-wave prefix in k_sample_write, instead of a scan over the rays.
// DIST: the launch's arguments carry a distortion map (SampleArgsDist), which setup_ray adds to the rays
template <bool DIST> using SampleArgsK = std::conditional_t<DIST, SampleArgsDist, SampleArgs>;
__device__ __forceinline__ DistMap dist_of(const SampleArgs&) { return DistMap{}; }
__device__ __forceinline__ DistMap dist_of(const SampleArgsDist& a) { return a.dist; }

template <bool CONE0, bool CDF, bool TEX, bool DIST>
__global__ void __launch_bounds__(256) k_sample_count(const Camera* __restrict__ cams, const void* __restrict__ pixels,
                                                      uint32_t n_images, const ngp_nerf_config cfg, SampleArgsK<DIST> a,
                                                      uint32_t* __restrict__ nsteps, float* __restrict__ tbuf,
                                                      RayGeo* __restrict__ geo, const Cone cone, uint32_t* __restrict__ wsum) {
	constexpr uint32_t RGk = sampler_rg<CONE0>();
	const uint32_t gid = blockIdx.x * blockDim.x + threadIdx.x;
	const uint32_t i = gid / RGk, L = gid % RGk;
	const bool live = i < a.n_rays;  // whole rows
	uint32_t j = 0;
	if (live) j = count_ray<CONE0, CDF, TEX, DIST>(cams, pixels, n_images, cfg, a, nsteps, tbuf, geo, cone, i, L, dist_of(a));
	const bool head = live && L == 0;
	const uint32_t sum = wave_sum(head ? j : 0u);
	const uint32_t nz = (uint32_t)__popcll(__ballot(head && j > 0));
	if ((threadIdx.x & 63) == 0) {
		const uint32_t w = gid / 64;
		wsum[2 * w] = sum;
		wsum[2 * w + 1] = nz;
	}
}

// pass 2: write the ray records and the NerfCoordinates of kept rays from the stored t values; one
// wave per ray (most rays take one or two iterations, consecutive lanes write consecutive samples).
constexpr uint32_t WG = 64;
#ifndef NGP_SW_STAGE
#define NGP_SW_STAGE 1  // records staged in LDS, written as contiguous wave stores
#endif
// pass 2: write the ray records and the NerfCoordinates of kept rays from the stored t values.
// The ray's sample base (exclusive prefix of the counts, the reference's atomicAdd on numsteps_counter in ray order)
// and its slot among the kept rays: bpre (the count wave's prefixes, k_sample_bscan) plus the prefix over the
// rays of its count wave before it (rpw rays per count wave). A ray is kept when it has samples and they fit
// under max_samples (testbed_nerf.cu:1616-1619); the inclusive prefix grows with the ray index, so the kept
// rays are the rays with samples before the first that does not fit, and a kept ray's slot counts every ray
// with samples before it.
__global__ void __launch_bounds__(256) k_sample_write(const ngp_nerf_config cfg, SampleArgs a, const uint32_t* __restrict__ nsteps,
                                                      const uint32_t* __restrict__ bpre, uint32_t rpw, const float* __restrict__ tbuf,
                                                      const RayGeo* __restrict__ geo, const Cone cone) {
	const uint32_t gid = blockIdx.x * blockDim.x + threadIdx.x;
	const uint32_t i = gid / WG, L = gid % WG;
	if (i >= a.n_rays) return;  // whole waves
	const uint32_t w = i / rpw, r0 = w * rpw;
	const uint32_t nl = (r0 + L < i) ? nsteps[r0 + L] : 0u;  // the count wave's rays before ray i
	const uint32_t before = wave_sum(nl);
	const uint32_t nz_before = (uint32_t)__popcll(__ballot(nl > 0));
	const uint32_t numsteps = nsteps[i], b = bpre[2 * w] + before;
	if (numsteps == 0 || b + numsteps > a.max_samples) return;
	const uint32_t s = bpre[2 * w + 1] + nz_before;
	const RayGeo g = geo[i];
	if (L == 0) {
		a.ray_indices[s] = i + a.ray_offset;
		float* ro = a.rays + (size_t)s * 6;
		ro[0] = g.o[0]; ro[1] = g.o[1]; ro[2] = g.o[2]; ro[3] = g.d[0]; ro[4] = g.d[1]; ro[5] = g.d[2];
		a.numsteps[2 * s] = numsteps;
		a.numsteps[2 * s + 1] = b;
	}
	const Aabb box = cfg_aabb(cfg);
	const V3 diag = v3(box.mx.x - box.mn.x, box.mx.y - box.mn.y, box.mx.z - box.mn.z);
	const V3 wdir = v3((g.dn[0] + 1.0f) * 0.5f, (g.dn[1] + 1.0f) * 0.5f, (g.dn[2] + 1.0f) * 0.5f);
	const float* tin = tbuf + (size_t)i * STEPS;
#if NGP_SW_STAGE
	// a wave's 64 records (7 floats each, 28-B stride) are staged in LDS and written back as 7 contiguous
	// 256-B wave stores instead of 7 stores that each touch 14 lines
	__shared__ float stage[256 / WG][WG * 7];
	float* st = stage[threadIdx.x / WG];
	for (uint32_t j0 = 0; j0 < numsteps; j0 += WG) {
		const uint32_t jj = j0 + L;
		if (jj < numsteps) {
			const float t = tin[jj];
			const V3 pos = v3(g.o[0] + t * g.dn[0], g.o[1] + t * g.dn[1], g.o[2] + t * g.dn[2]);
			const float dt = calc_dt(t, cone);
			float* c = st + L * 7;  // stride 7 words: conflict-free
			c[0] = (pos.x - box.mn.x) / diag.x; c[1] = (pos.y - box.mn.y) / diag.y; c[2] = (pos.z - box.mn.z) / diag.z;
			c[3] = warp_dt(dt);
			c[4] = wdir.x; c[5] = wdir.y; c[6] = wdir.z;
		}
		__builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
		__builtin_amdgcn_wave_barrier();
		__builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
		const uint32_t nf = min(WG, numsteps - j0) * 7;
		float* dst = a.coords + (size_t)(b + j0) * 7;
#pragma unroll
		for (uint32_t k = 0; k < 7; ++k)
			if (L + k * WG < nf) dst[L + k * WG] = st[L + k * WG];
		__builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
		__builtin_amdgcn_wave_barrier();
		__builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
	}
#else
	for (uint32_t jj = L; jj < numsteps; jj += WG) {
		const float t = tin[jj];
		const V3 pos = v3(g.o[0] + t * g.dn[0], g.o[1] + t * g.dn[1], g.o[2] + t * g.dn[2]);
		const float dt = calc_dt(t, cone);
		float* c = a.coords + (size_t)(b + jj) * 7;
		c[0] = (pos.x - box.mn.x) / diag.x; c[1] = (pos.y - box.mn.y) / diag.y; c[2] = (pos.z - box.mn.z) / diag.z;
		c[3] = warp_dt(dt);
		c[4] = wdir.x; c[5] = wdir.y; c[6] = wdir.z;
	}
#endif
}

// The count waves' exclusive prefixes (bpre[2 w]: samples before wave w, bpre[2 w + 1]: rays with samples
// before it) from their sums, one block; and the counters: rays kept, and the total count of every ray (the
// reference's numsteps_counter, dropped rays included). The one wave whose rays cross max_samples is found
// here and its rays counted in order.
__global__ void __launch_bounds__(SCAN1_THREADS) k_sample_bscan(uint32_t nw, const uint32_t* __restrict__ wsum, uint32_t* __restrict__ bpre,
                                                                const uint32_t* __restrict__ nsteps, uint32_t n_rays, uint32_t rpw,
                                                                uint32_t max_samples, uint32_t* __restrict__ counters) {
	__shared__ uint32_t lds[32];
	__shared__ uint32_t cross[3];  // the crossing wave, its prefixes
	if (threadIdx.x == 0) cross[0] = nw;
	uint32_t run_s = 0, run_z = 0;
	for (uint32_t t0 = 0; t0 < nw; t0 += SCAN1_TILE) {
		uint32_t sv[4], zv[4];
#pragma unroll
		for (uint32_t k = 0; k < 4; ++k) {
			const uint32_t w = t0 + 4 * threadIdx.x + k;
			sv[k] = w < nw ? wsum[2 * w] : 0u;
			zv[k] = w < nw ? wsum[2 * w + 1] : 0u;
		}
		uint32_t ts, tz;
		uint32_t bs = run_s + block_exclusive_sum(sv[0] + sv[1] + sv[2] + sv[3], lds, &ts);
		uint32_t bz = run_z + block_exclusive_sum(zv[0] + zv[1] + zv[2] + zv[3], lds, &tz);
#pragma unroll
		for (uint32_t k = 0; k < 4; ++k) {
			const uint32_t w = t0 + 4 * threadIdx.x + k;
			if (w < nw) {
				bpre[2 * w] = bs;
				bpre[2 * w + 1] = bz;
				if (bs <= max_samples && bs + sv[k] > max_samples) {  // at most one wave
					cross[0] = w; cross[1] = bs; cross[2] = bz;
				}
			}
			bs += sv[k];
			bz += zv[k];
		}
		run_s += ts;
		run_z += tz;
	}
	__syncthreads();
	if (threadIdx.x == 0) {
		uint32_t kept = run_z;
		if (cross[0] < nw) {
			uint32_t b = cross[1];
			kept = cross[2];
			for (uint32_t r = cross[0] * rpw; r < min(n_rays, (cross[0] + 1) * rpw); ++r) {
				const uint32_t n = nsteps[r];
				if (b + n > max_samples) break;
				kept += n > 0 ? 1u : 0u;
				b += n;
			}
		}
		counters[0] = kept;
		counters[1] = run_s;
	}
}

size_t sample_tmp_f32(uint32_t n_rays) { return (size_t)n_rays * (STEPS + sizeof(RayGeo) / 4); }

// count waves of the sampler's count pass: whole blocks of NGP_SAMPLER_BLOCK threads, RGk lanes per ray
static uint32_t sample_count_waves(uint32_t n_rays, uint32_t rgk) {
	return (uint32_t)(div_round_up((size_t)n_rays * rgk, NGP_SAMPLER_BLOCK) * (NGP_SAMPLER_BLOCK / 64));
}
size_t sample_tmp_u32(uint32_t n_rays) { return n_rays + 4 * (size_t)sample_count_waves(n_rays, std::max(RG, sampler_rg<true>())); }

// k_sample_count's 8 instantiations by their switches, without and with a distortion map. Bit 0: cone stepping (CONE0 = false), bit 1: CDF, bit 2: TEX.
// The order is the order the kernels are instantiated in, and their machine code depends on it: each CONE0 = true form
// before the cone-stepping form it shares setup_ray<CDF, TEX> with, as the launch code listed them before there was a
// table. With CONE0 as a plain bit 0 the four cone-stepping kernels come out scheduled differently (60 VGPRs for 62,
// one or two instructions more); tools/kernel_asm_diff.py against the commit before shows it.
template <bool DIST>
using SampleCount = void (*)(const Camera*, const void*, uint32_t, const ngp_nerf_config, SampleArgsK<DIST>, uint32_t*, float*, RayGeo*,
                             const Cone, uint32_t*);
template <bool DIST, size_t... I>
static SampleCount<DIST> sample_count_kernel(uint32_t i, std::index_sequence<I...>) {
	static const SampleCount<DIST> k[] = {k_sample_count<(I & 1) == 0, (I & 2) != 0, (I & 4) != 0, DIST>...};
	return k[i];
}
// DIST is no bit of the index: the 8 forms without a map first, in their order, then the 8 with one
template <bool DIST>
static SampleCount<DIST> sample_count_kernel(bool cone0, bool cdf, bool tex) {
	return sample_count_kernel<DIST>((cone0 ? 0u : 1u) | (cdf ? 2u : 0u) | (tex ? 4u : 0u), std::make_index_sequence<8>{});
}

void sample_rays(const Dataset& ds, const ngp_nerf_config& cfg, const SampleArgs& a, uint32_t* tmp, float* tmpf, hipStream_t s,
                 const Camera* cams, const DistMap* dist) {
	if (a.n_rays == 0) return;
	if (!cams) cams = ds.d_cams;
	NGP_CHECK(tmpf != nullptr, "sample_rays: float scratch of sample_tmp_f32(n_rays) floats required");
	const bool cone0 = cfg.cone_angle_constant <= 1e-5f;
	const uint32_t rgk = cone0 ? sampler_rg<true>() : RG;
	const uint32_t nw = sample_count_waves(a.n_rays, rgk);
	uint32_t* nsteps = tmp;
	uint32_t* wsum = tmp + a.n_rays;    // 2 per count wave
	uint32_t* bpre = wsum + 2 * (size_t)nw;
	float* tbuf = tmpf;
	RayGeo* geo = (RayGeo*)(tmpf + (size_t)a.n_rays * STEPS);
	const uint32_t blocks = div_round_up((size_t)a.n_rays * RG, NGP_SAMPLER_BLOCK);
	const uint32_t blocks0 = div_round_up((size_t)a.n_rays * sampler_rg<true>(), NGP_SAMPLER_BLOCK);
	const Cone cone = make_cone(cfg.cone_angle_constant);  // every ray's cone (setup_ray: r.cone)
	{
		ProfScope ps("sample_count", s);
		// pixels from the error map's CDFs, or a Half or Float image in the dataset (the TEX forms read the image table): the
		// count pass's other instantiations (the write pass copies what it stored)
		const bool tex = ds.tex();
		const void* pixels = tex ? (const void*)ds.d_images : (const void*)ds.d_pixels;
		const SampleCount<false> count = sample_count_kernel<false>(cone0, a.cdfs.any(), tex);
		if (dist && dist->data) {  // a distortion map: the DIST forms
			SampleArgsDist ad;
			(SampleArgs&)ad = a;
			ad.dist = *dist;
			sample_count_kernel<true>(cone0, a.cdfs.any(), tex)<<<cone0 ? blocks0 : blocks, NGP_SAMPLER_BLOCK, 0, s>>>(
			    cams, pixels, ds.n_images, cfg, ad, nsteps, tbuf, geo, cone, wsum);
		} else {
			count<<<cone0 ? blocks0 : blocks, NGP_SAMPLER_BLOCK, 0, s>>>(cams, pixels, ds.n_images, cfg, a, nsteps, tbuf, geo, cone, wsum);
		}
		NGP_HIP(hipGetLastError());
	}
	NGP_CHECK(nw == (cone0 ? blocks0 : blocks) * (NGP_SAMPLER_BLOCK / 64) && 64 % rgk == 0, "sampler: count waves");
	{
		ProfScope ps("sample_scans", s);
		k_sample_bscan<<<1, SCAN1_THREADS, 0, s>>>(nw, wsum, bpre, nsteps, a.n_rays, 64 / rgk, a.max_samples, a.counters);
		NGP_HIP(hipGetLastError());
	}
	ProfScope ps("sample_write", s);
	k_sample_write<<<div_round_up((size_t)a.n_rays * WG, 256), 256, 0, s>>>(cfg, a, nsteps, bpre, 64 / rgk, tbuf, geo, cone);
	NGP_HIP(hipGetLastError());
}

// Every ray's training pixel, as the sampler and loss pass 1 draw it (nerf_pixel.h): for inspection and tests
__global__ void __launch_bounds__(256) k_training_pixels(const Camera* __restrict__ cams, uint32_t n_images, bool snap, ErrorCdfs e,
                                                         uint32_t n_rays, uint32_t ray_offset, uint32_t n_rays_div, Rng rng,
                                                         uint32_t* __restrict__ img, float* __restrict__ uv, float* __restrict__ pdf) {
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n_rays) return;
	const uint32_t ig = i + ray_offset;
	pcg_advance(rng, (uint64_t)ig * N_MAX_RANDOM_SAMPLES_PER_RAY);
	const TrainPixel p = training_pixel<true>(cams, n_images, snap, e, ig, n_rays_div, rng);
	img[i] = p.img;
	uv[2 * (size_t)i] = p.u; uv[2 * (size_t)i + 1] = p.v;
	pdf[2 * (size_t)i] = p.img_pdf; pdf[2 * (size_t)i + 1] = p.uv_pdf;
}
void training_pixels(const Dataset& ds, const ngp_nerf_config& cfg, uint32_t n_rays, uint32_t ray_offset, uint32_t n_rays_total, Rng rng,
                     const ErrorCdfs& cdfs, uint32_t* img, float* uv, float* pdf, hipStream_t s) {
	if (n_rays == 0) return;
	k_training_pixels<<<div_round_up(n_rays, 256u), 256, 0, s>>>(ds.d_cams, ds.n_images, cfg.snap_to_pixel_centers != 0, cdfs, n_rays,
	                                                             ray_offset, n_rays_total, rng, img, uv, pdf);
	NGP_HIP(hipGetLastError());
}
void training_pixels_host(const Camera* cams, uint32_t n_images, const ngp_nerf_config& cfg, uint32_t n_rays, uint32_t ray_offset,
                          uint32_t n_rays_total, Rng rng, const ErrorCdfs& cdfs, uint32_t* img, float* uv, float* pdf) {
	for (uint32_t i = 0; i < n_rays; ++i) {
		const uint32_t ig = i + ray_offset;
		HostPcg32 r{rng.state, rng.inc};
		r.advance((uint64_t)ig * N_MAX_RANDOM_SAMPLES_PER_RAY);
		const TrainPixel p = training_pixel<true>(cams, n_images, cfg.snap_to_pixel_centers != 0, cdfs, ig, n_rays_total, r);
		img[i] = p.img;
		uv[2 * (size_t)i] = p.u; uv[2 * (size_t)i + 1] = p.v;
		pdf[2 * (size_t)i] = p.img_pdf; pdf[2 * (size_t)i + 1] = p.uv_pdf;
	}
}

}  // namespace nerf
}  // namespace ngp
