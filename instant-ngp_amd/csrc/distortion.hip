// distortion.hip — the lens distortion map's stand-alone kernels: the lookup for inspection and tests (device and host),
// the per-ray gradient deposit into the exact accumulator, and the accumulator's conversion to the fp32 gradient
// (distortion.h). The per-ray image-plane gradient itself is k_cam_ray_grad's DIST form (nerf_camera.hip).
#include "distortion.h"
#include "nerf.h"
#include "nerf_pixel.h"

namespace ngp {
namespace nerf {

__global__ void __launch_bounds__(256) k_distortion_lookup(uint32_t w, uint32_t h, uint32_t n, const float* __restrict__ uv,
                                                           uint32_t* __restrict__ texels, float* __restrict__ weights,
                                                           const float* __restrict__ map, float* __restrict__ offsets) {
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n) return;
	const float u = uv[2 * (size_t)i], v = uv[2 * (size_t)i + 1];
	const DistortionTap t = distortion_lookup(w, h, u, v);
	for (int k = 0; k < 4; ++k) { texels[4 * (size_t)i + k] = t.idx[k]; weights[4 * (size_t)i + k] = t.w[k]; }
	if (map && offsets) distortion_offset(map, w, h, u, v, offsets + 2 * (size_t)i, offsets + 2 * (size_t)i + 1);
}

void distortion_lookup_device(uint32_t w, uint32_t h, uint32_t n, const float* uv, uint32_t* texels, float* weights, const float* map,
                              float* offsets, hipStream_t s) {
	if (n == 0) return;
	k_distortion_lookup<<<div_round_up(n, 256), 256, 0, s>>>(w, h, n, uv, texels, weights, map, offsets);
	NGP_HIP(hipGetLastError());
}

void distortion_lookup_host(uint32_t w, uint32_t h, uint32_t n, const float* uv, uint32_t* texels, float* weights, const float* map,
                            float* offsets) {
	for (size_t i = 0; i < n; ++i) {
		const DistortionTap t = distortion_lookup(w, h, uv[2 * i], uv[2 * i + 1]);
		for (int k = 0; k < 4; ++k) { texels[4 * i + k] = t.idx[k]; weights[4 * i + k] = t.w[k]; }
		if (map && offsets) distortion_offset(map, w, h, uv[2 * i], uv[2 * i + 1], offsets + 2 * i, offsets + 2 * i + 1);
	}
}

// One thread per kept ray: its uv as the sampler and loss pass 1 drew it (uniform pixels: uv_pdf 1), the taps, the adds
__global__ void __launch_bounds__(256) k_distortion_deposit(DistDepositArgs a) {
	const uint32_t n_kept = min(*a.ray_counter, a.n_rays_cap);
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n_kept) return;
	if (a.numsteps && a.numsteps[2 * (size_t)i] == 0) return;  // the ray does not matter (testbed_nerf.cu:2044-2048)
	const uint32_t ig = a.ray_indices[i];
	Rng rng = a.rng;
	pcg_advance(rng, (uint64_t)ig * N_MAX_RANDOM_SAMPLES_PER_RAY);
	const TrainPixel px = training_pixel<false>(a.cams, a.n_images, a.snap, ErrorCdfs{}, ig, a.n_rays_total, rng);
	const DistortionTap t = distortion_lookup(a.w, a.h, px.u, px.v);
	distortion_deposit(a.acc, (size_t)a.w * a.h * DISTORTION_CHANNELS * DISTORTION_BINS, t, a.ray_grad[2 * (size_t)i],
	                   a.ray_grad[2 * (size_t)i + 1]);
}

void distortion_deposit_rays(const DistDepositArgs& a, hipStream_t s) {
	if (a.n_rays_cap == 0) return;
	k_distortion_deposit<<<div_round_up(a.n_rays_cap, 256u), 256, 0, s>>>(a);
	NGP_HIP(hipGetLastError());
}

// A channel's value: its bins from the highest down, each converted to double and scaled by its unit (exact), summed
__device__ __forceinline__ double distortion_channel_sum(const unsigned long long* __restrict__ bins) {
	double s = 0.0;
#pragma unroll
	for (int b = (int)DISTORTION_BINS - 1; b >= 0; --b)
		s += (double)(long long)bins[b] * __builtin_scalbn(1.0, 16 * b - DISTORTION_BIAS);
	return s;
}

// safe_divide(gradient, weight) per texel (testbed_nerf.cu:3811-3816). The quotient of the two exact sums is taken in
// double and rounded to fp32 once: within 2^-24 of the exact quotient, relatively (dividing the two sums after rounding
// each to fp32, as the reference's float arrays would, rounds three times: up to 1.5 * 2^-23)
__global__ void __launch_bounds__(256) k_distortion_gradient(uint32_t n_texels, const unsigned long long* __restrict__ acc,
                                                             float* __restrict__ grad) {
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n_texels) return;
	const unsigned long long* t = acc + (size_t)i * DISTORTION_CHANNELS * DISTORTION_BINS;
	const double sw = distortion_channel_sum(t + 2 * DISTORTION_BINS);
	float gx = 0.0f, gy = 0.0f;
	if (sw != 0.0) {
		gx = (float)(distortion_channel_sum(t) / sw);
		gy = (float)(distortion_channel_sum(t + DISTORTION_BINS) / sw);
	}
	grad[2 * (size_t)i] = gx;
	grad[2 * (size_t)i + 1] = gy;
}

void distortion_gradient_f32(uint32_t w, uint32_t h, const unsigned long long* acc, float* grad, hipStream_t s) {
	const uint32_t n = w * h;
	if (n == 0) return;
	k_distortion_gradient<<<div_round_up(n, 256u), 256, 0, s>>>(n, acc, grad);
	NGP_HIP(hipGetLastError());
}

}  // namespace nerf
}  // namespace ngp
