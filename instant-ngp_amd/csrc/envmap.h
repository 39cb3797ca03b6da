// envmap.h — the environment map: a small trainable equirectangular RGBA image read by ray direction as the
// background at infinity (read_envmap / deposit_envmap_gradient, envmap.cuh:29-94; dir_to_spherical_unorm,
// random_val.cuh:62-72; restated).
//
// One text for the device and the host, in nerf_pixel.h's manner: the loss pass's read, its gradient deposit, the
// renderer's frame fill, the stand-alone kernels and the host export all take the four texels and weights of a
// direction from envmap_lookup(). acosf and atan2f are not the same function on the host and on the device, so the
// two do NOT agree to the last bit and nothing relies on that. Include inside a .hip file only.
#pragma once
#include <cmath>
#include <cstdint>

#include <hip/hip_runtime.h>

namespace ngp {
namespace nerf {

#define NGP_ENVMAP_FN __host__ __device__ __forceinline__

struct EnvmapTap {
	uint32_t idx[4];  // texel index x + y * width of (x, y), (x + 1, y), (x, y + 1), (x + 1, y + 1): x wraps, y clamps
	float w[4];       // (1-wx)(1-wy), wx(1-wy), (1-wx)wy, wx wy
};

// dir: normalized. width, height >= 1.
NGP_ENVMAP_FN EnvmapTap envmap_lookup(uint32_t width, uint32_t height, float dx, float dy, float dz) {
	const float PI = 3.14159265358979323846f;
	// dir_to_spherical_unorm({d.z, -d.x, d.y}): theta from the y axis, phi around it
	const float cos_theta = fminf(fmaxf(dy, -1.0f), 1.0f);
	const float theta_unorm = acosf(cos_theta) / PI;
	const float phi_unorm = atan2f(-dx, dz) / (2.0f * PI) + 0.5f;
	const float fx = phi_unorm * (float)((int)width - 1), fy = theta_unorm * (float)((int)height - 1);
	const int ix = (int)fx, iy = (int)fy;  // truncation, as ivec2(vec2)
	const float wx = fx - (float)ix, wy = fy - (float)iy;
	const int W = (int)width, H = (int)height;
	auto texel = [&](int x, int y) {
		if (x < 0) x += W;
		else if (x >= W) x -= W;
		// one wrap is the reference's; the clamp after it keeps every index inside the map whatever the direction holds
		x = x < 0 ? 0 : (x > W - 1 ? W - 1 : x);
		y = y > H - 1 ? H - 1 : y;
		y = y < 0 ? 0 : y;
		return (uint32_t)x + (uint32_t)y * width;
	};
	EnvmapTap t;
	t.idx[0] = texel(ix, iy); t.idx[1] = texel(ix + 1, iy); t.idx[2] = texel(ix, iy + 1); t.idx[3] = texel(ix + 1, iy + 1);
	t.w[0] = (1.0f - wx) * (1.0f - wy); t.w[1] = wx * (1.0f - wy); t.w[2] = (1.0f - wx) * wy; t.w[3] = wx * wy;
	return t;
}

// One channel of read_envmap: the four products summed in the reference's order
NGP_ENVMAP_FN float envmap_mix(const EnvmapTap& t, float a, float b, float c, float d) {
	return t.w[0] * a + t.w[1] * b + t.w[2] * c + t.w[3] * d;
}

// The gradient accumulator of a map of n = width * height * 4 channels: n 64-bit integers, each the exact sum of its
// channel's fp16 contributions in units of 2^-24 (every fp16 value is an integer multiple of 2^-24, and 2^20
// contributions of fp16's maximum stay below 2^61), then one bit per channel, set by a non-finite contribution.
// Integer addition and OR do not depend on the order of arrival, so the gradient is the same bits in every run.
constexpr float ENVMAP_ACC_UNIT = 5.9604644775390625e-08f;  // 2^-24
size_t envmap_acc_words64(uint32_t width, uint32_t height);  // n, then the bits rounded up to whole words

// One ray's deposit (deposit_envmap_gradient with T = half, envmap.cuh:57-94): value[c] holds the fp16 gradient of
// channel c (alpha's is zero in the reference, testbed_nerf.cu:2007-2008, and is not deposited); each corner
// receives fp16(value) * fp16(weight), the product rounded to fp16. A zero product adds nothing and is skipped.
// idx < width * height by envmap_lookup, so every access is inside the accumulator.
__device__ __forceinline__ void envmap_deposit(unsigned long long* __restrict__ acc, size_t n_channels, const EnvmapTap& t,
                                               _Float16 v0, _Float16 v1, _Float16 v2) {
	uint32_t* poison = (uint32_t*)(acc + n_channels);
	const _Float16 v[3] = {v0, v1, v2};
#pragma unroll
	for (int k = 0; k < 4; ++k) {
		// fp16(weight) of the fp32 weight envmap_lookup returns, as the reference's `T weight` argument rounds it. The
		// empty asm pins the fp32 product: without it the compiler folds the weight's multiplication and this
		// conversion into one mixed-precision instruction that rounds the exact product once, and a weight that
		// is a tie in fp32 then lands on the other fp16 neighbour (seen on gfx950 against numpy's float16).
		float wf = t.w[k];
		asm volatile("" : "+v"(wf));
		const _Float16 wk = (_Float16)wf;
#pragma unroll
		for (int c = 0; c < 3; ++c) {
			const _Float16 p = v[c] * wk;
			const float pf = (float)p;
			const size_t ch = (size_t)t.idx[k] * 4 + c;
			if (!(fabsf(pf) <= 65504.0f)) atomicOr(poison + ch / 32, 1u << (ch % 32));  // inf or NaN: the channel's gradient is NaN
			else if (pf != 0.0f) atomicAdd(acc + ch, (unsigned long long)(long long)(pf * 16777216.0f));
		}
	}
}

}  // namespace nerf
}  // namespace ngp
