// distortion.h — the lens distortion map: a small trainable 2-D image of ray-direction offsets that absorbs what the
// declared lens model does not explain (Testbed::m_distortion; uv_to_ray adds distortion.at_lerp(uv) to dir.xy,
// common_device.cuh:443-510; Buffer2DView::at_lerp, common.h:384-400; deposit_image_gradient, common_device.cuh:124-156;
// restated).
//
// One text for the device and the host, in nerf_pixel.h's manner: the sampler's setup_ray, the renderer's ray setup and
// its Distortion mode, the gradient deposit, the stand-alone kernels and the host export all take the four texels and
// weights of a uv from distortion_lookup(). It uses IEEE add, subtract, multiply, compare and convert only and the build
// has -ffp-contract=off, so the host and the device return the same bits. Include inside a .hip file only.
#pragma once
#include <cmath>
#include <cstdint>

#include <hip/hip_runtime.h>

namespace ngp {
namespace nerf {

#define NGP_DISTORTION_FN __host__ __device__ __forceinline__

struct DistortionTap {
	uint32_t idx[4];  // texel index x + y * width of (x, y), (x + 1, y), (x, y + 1), (x + 1, y + 1), each clamped into the map
	float w[4];       // (1-wx)(1-wy), wx(1-wy), (1-wx)wy, wx wy
};

// width, height >= 1. uv is folded into [0, 2] with NaN to 0 before the conversion to int, as training_pixel folds its
// coordinates, so every index is inside the map whatever uv holds (the reference converts as it comes).
NGP_DISTORTION_FN DistortionTap distortion_lookup(uint32_t width, uint32_t height, float u, float v) {
	u = u >= 0.0f ? (u <= 2.0f ? u : 2.0f) : 0.0f;
	v = v >= 0.0f ? (v <= 2.0f ? v : 2.0f) : 0.0f;
	const float fx = (float)(int)width * u, fy = (float)(int)height * v;
	const int ix = (int)fx, iy = (int)fy;  // truncation, as ivec2(vec2)
	const float wx = fx - (float)ix, wy = fy - (float)iy;
	const int W = (int)width, H = (int)height;
	auto texel = [&](int x, int y) {
		x = x > W - 1 ? W - 1 : x;
		x = x < 0 ? 0 : x;
		y = y > H - 1 ? H - 1 : y;
		y = y < 0 ? 0 : y;
		return (uint32_t)x + (uint32_t)y * width;
	};
	DistortionTap t;
	t.idx[0] = texel(ix, iy); t.idx[1] = texel(ix + 1, iy); t.idx[2] = texel(ix, iy + 1); t.idx[3] = texel(ix + 1, iy + 1);
	t.w[0] = (1.0f - wx) * (1.0f - wy); t.w[1] = wx * (1.0f - wy); t.w[2] = (1.0f - wx) * wy; t.w[3] = wx * wy;
	return t;
}

// One channel of at_lerp: the four products summed in the reference's order
NGP_DISTORTION_FN float distortion_mix(const DistortionTap& t, float a, float b, float c, float d) {
	return t.w[0] * a + t.w[1] * b + t.w[2] * c + t.w[3] * d;
}

// The offset of a map [height][width][2] at uv
NGP_DISTORTION_FN void distortion_offset(const float* __restrict__ map, uint32_t width, uint32_t height, float u, float v, float* ox,
                                         float* oy) {
	const DistortionTap t = distortion_lookup(width, height, u, v);
	const float* a = map + 2 * (size_t)t.idx[0];
	const float* b = map + 2 * (size_t)t.idx[1];
	const float* c = map + 2 * (size_t)t.idx[2];
	const float* d = map + 2 * (size_t)t.idx[3];
	*ox = distortion_mix(t, a[0], b[0], c[0], d[0]);
	*oy = distortion_mix(t, a[1], b[1], c[1], d[1]);
}

// ---- the gradient accumulator ----------------------------------------------------------------------------------------
// Exact and independent of the order of arrival, at any magnitude. A finite fp32 value is M * 2^(e - 149) with a signed
// 24-bit integer M and e = max(biased exponent, 1) - 1 in [0, 253]. It is added as the integer M << (e % 16) into bin
// e / 16 of its channel, whose unit is 2^(16 bin - 149): an addend is below 2^40 in magnitude, so 2^22 contributions to
// one bin cannot overflow its 64 bits. A texel has three channels, sum g.x w, sum g.y w and sum w (the reference keeps
// one weight per gradient channel; the two are equal), of DISTORTION_BINS 64-bit integers each. A product of a finite
// gradient and a weight in [0, 1] is finite, so a non-finite product comes from a non-finite gradient alone: such a ray
// is dropped whole, weights included, and counted in one more word behind the bins (the reference would turn the texel
// NaN for good).
constexpr uint32_t DISTORTION_BINS = 16, DISTORTION_CHANNELS = 3;
constexpr int DISTORTION_BIAS = 149;
// words of the accumulator of a width x height map: the bins, then the counter
NGP_DISTORTION_FN size_t distortion_acc_words64(uint32_t width, uint32_t height) {
	return (size_t)width * height * DISTORTION_CHANNELS * DISTORTION_BINS + 1;
}

__device__ __forceinline__ void distortion_acc_add(unsigned long long* __restrict__ acc, size_t n_bins, size_t channel, float p) {
	const uint32_t bits = __float_as_uint(p);
	const uint32_t E = (bits >> 23) & 0xffu, frac = bits & 0x7fffffu;
	if (E == 0xffu || (E == 0 && frac == 0)) return;  // a zero adds nothing (inf and NaN: dropped by distortion_deposit)
	const uint32_t e = (E ? E : 1u) - 1u;
	const long long M = (long long)(E ? (frac | 0x800000u) : frac) << (e % DISTORTION_BINS);
	atomicAdd(acc + channel * DISTORTION_BINS + e / DISTORTION_BINS, (unsigned long long)((bits >> 31) ? -M : M));
}

// One ray's deposit (deposit_image_gradient): corner k receives g.x * w_k, g.y * w_k and w_k, each product one fp32
// multiply. idx < width * height by distortion_lookup, so every access is inside the accumulator.
__device__ __forceinline__ void distortion_deposit(unsigned long long* __restrict__ acc, size_t n_bins, const DistortionTap& t, float gx,
                                                   float gy) {
	if (!(fabsf(gx) <= 3.402823466e38f) || !(fabsf(gy) <= 3.402823466e38f)) {  // inf or NaN: the ray is dropped and counted
		atomicAdd(acc + n_bins, 1ull);
		return;
	}
#pragma unroll
	for (int k = 0; k < 4; ++k) {
		const size_t ch = (size_t)t.idx[k] * DISTORTION_CHANNELS;
		distortion_acc_add(acc, n_bins, ch, gx * t.w[k]);
		distortion_acc_add(acc, n_bins, ch + 1, gy * t.w[k]);
		distortion_acc_add(acc, n_bins, ch + 2, t.w[k]);
	}
}

}  // namespace nerf
}  // namespace ngp
