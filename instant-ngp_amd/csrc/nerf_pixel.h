// nerf_pixel.h — which training pixel a ray looks at: its image, its position in the image and the probability
// densities of both choices (image_idx and nerf_random_image_pos_training with sample_cdf_2d,
// testbed_nerf.cu:1232-1338; binary_search, common.h:268-292; restated).
//
// One text for the device and the host, in ngp_math.h's manner: the sampler's count pass (setup_ray), loss pass 1,
// k_training_pixels and training_pixels_host all call training_pixel(). It uses IEEE add, subtract, multiply,
// divide, compare and convert only and the build has -ffp-contract=off, so the host and the device return the same
// bits. Include inside a .hip file only, after nerf.h, render_common.h and rng.h.
#pragma once
#include "nerf.h"
#include "ngp_math.h"
#include "render_common.h"
#include "rng.h"

namespace ngp {
namespace nerf {

#define NGP_PIXEL_FN __host__ __device__ __forceinline__

constexpr float UNIFORM_SAMPLING_FRACTION = 0.5f;  // testbed_nerf.cu:1232

// binary_search: the first index whose entry is not below val, at most length - 1. Every load is at an index below
// length, whatever the entries are: `it` stays under first + count <= length.
NGP_PIXEL_FN uint32_t cdf_search(float val, const float* __restrict__ data, uint32_t length) {
	if (length == 0) return 0;
	uint32_t first = 0, count = length;
	while (count > 0) {
		const uint32_t step = count / 2, it = first + step;
		if (data[it] < val) {
			first = it + 1;
			count -= step + 1;
		} else {
			count = step;
		}
	}
	return first < length - 1 ? first : length - 1;
}

// next_float of tcnn::pcg32 (pcg_float of rng.h, with a bit cast the host has too)
template <typename R>
NGP_PIXEL_FN float pixel_pcg_float(R& r) { return ngp_math_u2f((pcg_next(r) >> 9) | 0x3f800000u) - 1.0f; }

struct TrainPixel {
	uint32_t img;
	float u, v;             // after snapping
	float img_pdf, uv_pdf;  // 1 where the choice was uniform
};

// Ray ig (global index) of a batch whose image choice divides by n_rays_div; rng is the ray's stream, already
// advanced to the ray (ig * N_MAX_RANDOM_SAMPLES_PER_RAY): two floats are drawn, with or without CDFs.
// CDF false: the uniform formulas and nothing else (the kernels' flag-off instantiations). CDF true: e.cdf_img
// non-null picks the image by the low-discrepancy sample of ig; e.cdf_x_cond_y non-null (with e.cdf_y) spends half
// of the position samples on the error map's CDFs. cams: width and height of every image (host or device memory).
template <bool CDF, typename R>
NGP_PIXEL_FN TrainPixel training_pixel(const Camera* __restrict__ cams, uint32_t n_images, bool snap, const ErrorCdfs& e, uint32_t ig,
                                       uint32_t n_rays_div, R& rng) {
	TrainPixel p;
	p.img_pdf = 1.0f;
	p.uv_pdf = 1.0f;
	if (CDF && e.cdf_img) {
		p.img = cdf_search(ld_random_val(ig, 0xdeadbeefu), e.cdf_img, n_images);
		const float prev = p.img > 0 ? e.cdf_img[p.img - 1] : 0.0f;
		p.img_pdf = (e.cdf_img[p.img] - prev) * (float)n_images;
	} else {
		p.img = ((ig * n_images) / n_rays_div) % n_images;  // neighbouring rays share an image
	}
	const uint32_t w = cams[p.img].width, h = cams[p.img].height;
	float x = pixel_pcg_float(rng);
	float y = pixel_pcg_float(rng);
	if (CDF && e.cdf_x_cond_y) {
		if (x < UNIFORM_SAMPLING_FRACTION) {
			x = x / UNIFORM_SAMPLING_FRACTION;
		} else {
			x = (x - UNIFORM_SAMPLING_FRACTION) / (1.0f - UNIFORM_SAMPLING_FRACTION);
			// the row by cdf_y, then the column by that row's cdf_x_cond_y; a sample above a row's last entry
			// (0.99999994 after rounding) lands in the last cell, with the rescaled coordinate a little above 1
			const float* __restrict__ cy = e.cdf_y + (size_t)p.img * e.h;
			const uint32_t row = cdf_search(y, cy, e.h);
			float prev = row > 0 ? cy[row - 1] : 0.0f;
			const float pmf_y = cy[row] - prev;
			y = (y - prev) / pmf_y;
			const float* __restrict__ cx = e.cdf_x_cond_y + ((size_t)p.img * e.h + row) * e.w;
			const uint32_t col = cdf_search(x, cx, e.w);
			prev = col > 0 ? cx[col - 1] : 0.0f;
			const float pmf_x = cx[col] - prev;
			x = (x - prev) / pmf_x;
			p.uv_pdf = pmf_x * pmf_y * (float)(e.w * e.h);
			x = ((float)col + x) / (float)e.w;
			y = ((float)row + y) / (float)e.h;
			// CDFs keep both within [0, 1 + a few ulp]. Arrays that are not CDFs (a zero or NaN step) give inf or NaN
			// here, which the conversions to int that follow (snapping, pixel_index) must not see: folded into [0, 2],
			// NaN to 0, the same on the host and the device
			x = x >= 0.0f ? (x <= 2.0f ? x : 2.0f) : 0.0f;
			y = y >= 0.0f ? (y <= 2.0f ? y : 2.0f) : 0.0f;
		}
	}
	if (snap) {
		int px = (int)(x * (float)w), py = (int)(y * (float)h);
		px = px < 0 ? 0 : (px > (int)w - 1 ? (int)w - 1 : px);
		py = py < 0 ? 0 : (py > (int)h - 1 ? (int)h - 1 : py);
		x = ((float)px + 0.5f) / (float)w;
		y = ((float)py + 0.5f) / (float)h;
	}
	p.u = x;
	p.v = y;
	return p;
}

}  // namespace nerf
}  // namespace ngp
