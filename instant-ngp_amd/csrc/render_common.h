// render_common.h — device helpers shared by the ray tracers (nerf_render.hip's NerfTracer, sdf_render.hip's SphereTracer):
// the vector type, the bounding box tests (bounding_box.cuh) and the scrambled-Sobol pixel jitter (random_val.cuh).
// Float arithmetic in the reference's operation order (-ffp-contract=off). Include inside a .hip file only.
#pragma once
#include <cstdint>

#include "common.h"

namespace ngp {
namespace nerf {

struct V3 { float x, y, z; };
__device__ __forceinline__ V3 v3(float x, float y, float z) { return V3{x, y, z}; }

struct Aabb { V3 mn, mx; };
__device__ __forceinline__ bool aabb_contains(const Aabb& b, V3 p) {
	return p.x >= b.mn.x && p.x <= b.mx.x && p.y >= b.mn.y && p.y <= b.mx.y && p.z >= b.mn.z && p.z <= b.mx.z;
}
// bounding_box.cuh:163-216
__device__ void aabb_ray_intersect(const Aabb& b, V3 pos, V3 dir, float* out_min, float* out_max) {
	const float FMAX = 3.402823466e+38f;
	float tmin = (b.mn.x - pos.x) / dir.x, tmax = (b.mx.x - pos.x) / dir.x;
	if (tmin > tmax) { float t = tmin; tmin = tmax; tmax = t; }
	float tymin = (b.mn.y - pos.y) / dir.y, tymax = (b.mx.y - pos.y) / dir.y;
	if (tymin > tymax) { float t = tymin; tymin = tymax; tymax = t; }
	if (tmin > tymax || tymin > tmax) { *out_min = FMAX; *out_max = FMAX; return; }
	if (tymin > tmin) tmin = tymin;
	if (tymax < tmax) tmax = tymax;
	float tzmin = (b.mn.z - pos.z) / dir.z, tzmax = (b.mx.z - pos.z) / dir.z;
	if (tzmin > tzmax) { float t = tzmin; tzmin = tzmax; tzmax = t; }
	if (tmin > tzmax || tzmin > tmax) { *out_min = FMAX; *out_max = FMAX; return; }
	if (tzmin > tmin) tmin = tzmin;
	if (tzmax < tmax) tmax = tzmax;
	*out_min = tmin; *out_max = tmax;
}

// random_val.cuh:162-291 (Burley 2019 scrambled Sobol); ld_random_val also runs on the host (nerf_pixel.h)
__host__ __device__ inline uint32_t sobol_dim(uint32_t index, uint32_t dim) {
	// direction numbers of dims 0 and 1 (random_val.cuh:163-181)
	uint32_t X = 0;
	if (dim == 0) {
		X = 0;
#pragma unroll
		for (uint32_t bit = 0; bit < 32; ++bit) X ^= ((index >> bit) & 1u) * (0x80000000u >> bit);
	} else {
		uint32_t v = 0x80000000u;  // dim 1: v_k = v_{k-1} ^ (v_{k-1} >> 1)
#pragma unroll
		for (uint32_t bit = 0; bit < 32; ++bit) {
			X ^= ((index >> bit) & 1u) * v;
			v ^= v >> 1;
		}
	}
	return X;
}
__host__ __device__ __forceinline__ uint32_t hash_combine(uint32_t seed, uint32_t v) { return seed ^ (v + (seed << 6) + (seed >> 2)); }
__host__ __device__ __forceinline__ uint32_t reverse_bits32(uint32_t x) { return __builtin_bitreverse32(x); }
__host__ __device__ __forceinline__ uint32_t laine_karras(uint32_t x, uint32_t seed) {
	x += seed;
	x ^= x * 0x6c50b47cu;
	x ^= x * 0xb82f1e52u;
	x ^= x * 0xc7afe638u;
	x ^= x * 0x8d22f6e6u;
	return x;
}
__host__ __device__ __forceinline__ uint32_t nus_base2(uint32_t x, uint32_t seed) { return reverse_bits32(laine_karras(reverse_bits32(x), seed)); }
__host__ __device__ inline float ld_random_val(uint32_t index, uint32_t seed, uint32_t dim = 0) {
	const float S = (float)(1.0 / 4294967296.0);
	index = nus_base2(index, seed);
	return (float)nus_base2(sobol_dim(index, dim), hash_combine(seed, dim)) * S;
}
__device__ void ld_random_val_2d(uint32_t index, uint32_t seed, float* x, float* y) {
	const float S = (float)(1.0 / 4294967296.0);
	index = nus_base2(index, seed);
	*x = (float)nus_base2(sobol_dim(index, 0), hash_combine(seed, 0)) * S;
	*y = (float)nus_base2(sobol_dim(index, 1), hash_combine(seed, 1)) * S;
}
__device__ __forceinline__ float fractf_(float x) { return x - floorf(x); }
__device__ void ld_random_pixel_offset(uint32_t spp, float* ox, float* oy) {  // random_val.cuh:320-326
	float ax, ay, bx, by;
	ld_random_val_2d(0, 0xdeadbeefu, &ax, &ay);
	ld_random_val_2d(spp, 0xdeadbeefu, &bx, &by);
	*ox = fractf_(0.5f - ax + bx);
	*oy = fractf_(0.5f - ay + by);
}

}  // namespace nerf
}  // namespace ngp
