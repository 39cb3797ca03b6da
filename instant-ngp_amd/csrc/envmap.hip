// envmap.hip — the environment map's stand-alone kernels: the lookup for inspection and tests (device and host), the
// gradient deposit outside the loss pass, and the accumulator's conversion to the fp32 gradient (envmap.h).
#include "envmap.h"
#include "nerf.h"

namespace ngp {
namespace nerf {

size_t envmap_acc_words64(uint32_t width, uint32_t height) {
	const size_t n = (size_t)width * height * 4;
	return n + (n / 32 + 2) / 2;
}

__global__ void __launch_bounds__(256) k_envmap_lookup(uint32_t w, uint32_t h, uint32_t n, const float* __restrict__ dirs,
                                                       uint32_t* __restrict__ texels, float* __restrict__ weights) {
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n) return;
	const EnvmapTap t = envmap_lookup(w, h, dirs[3 * (size_t)i], dirs[3 * (size_t)i + 1], dirs[3 * (size_t)i + 2]);
	for (int k = 0; k < 4; ++k) { texels[4 * (size_t)i + k] = t.idx[k]; weights[4 * (size_t)i + k] = t.w[k]; }
}

void envmap_lookup_device(uint32_t w, uint32_t h, uint32_t n, const float* dirs, uint32_t* texels, float* weights, hipStream_t s) {
	if (n == 0) return;
	k_envmap_lookup<<<div_round_up(n, 256), 256, 0, s>>>(w, h, n, dirs, texels, weights);
	NGP_HIP(hipGetLastError());
}

void envmap_lookup_host(uint32_t w, uint32_t h, uint32_t n, const float* dirs, uint32_t* texels, float* weights) {
	for (size_t i = 0; i < n; ++i) {
		const EnvmapTap t = envmap_lookup(w, h, dirs[3 * i], dirs[3 * i + 1], dirs[3 * i + 2]);
		for (int k = 0; k < 4; ++k) { texels[4 * i + k] = t.idx[k]; weights[4 * i + k] = t.w[k]; }
	}
}

__global__ void __launch_bounds__(256) k_envmap_deposit(uint32_t w, uint32_t h, uint32_t n, const float* __restrict__ dirs,
                                                        const f16* __restrict__ values, unsigned long long* __restrict__ acc) {
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n) return;
	const EnvmapTap t = envmap_lookup(w, h, dirs[3 * (size_t)i], dirs[3 * (size_t)i + 1], dirs[3 * (size_t)i + 2]);
	envmap_deposit(acc, (size_t)w * h * 4, t, values[3 * (size_t)i], values[3 * (size_t)i + 1], values[3 * (size_t)i + 2]);
}

void envmap_deposit_values(uint32_t w, uint32_t h, uint32_t n, const float* dirs, const f16* values, unsigned long long* acc,
                           hipStream_t s) {
	if (n == 0) return;
	k_envmap_deposit<<<div_round_up(n, 256), 256, 0, s>>>(w, h, n, dirs, values, acc);
	NGP_HIP(hipGetLastError());
}

// One rounding: the integer sum converts to fp32 (round to nearest) and the scale by 2^-24 is exact
__global__ void __launch_bounds__(256) k_envmap_gradient(uint32_t n, const unsigned long long* __restrict__ acc,
                                                         float* __restrict__ grad) {
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n) return;
	const uint32_t* poison = (const uint32_t*)(acc + n);
	const bool bad = (poison[i / 32] >> (i % 32)) & 1u;
	grad[i] = bad ? __uint_as_float(0x7fc00000u) : (float)(long long)acc[i] * ENVMAP_ACC_UNIT;
}

void envmap_gradient_f32(uint32_t w, uint32_t h, const unsigned long long* acc, float* grad, hipStream_t s) {
	const uint32_t n = w * h * 4;
	if (n == 0) return;
	k_envmap_gradient<<<div_round_up(n, 256), 256, 0, s>>>(n, acc, grad);
	NGP_HIP(hipGetLastError());
}

}  // namespace nerf
}  // namespace ngp
