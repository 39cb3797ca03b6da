// nerf_camera.h — camera pose refinement for NeRF training: the per-image extrinsics gradient kernels
// (compute_cam_gradient_train_nerf, testbed_nerf.cu:2014-2123, restated without float atomics) and the host side
// (per-camera Adam states, adam_optimizer.h:128-309; update_transforms, testbed_nerf.cu:2980-3024).
#pragma once
#include <type_traits>

#include "common.h"

namespace ngp {
namespace nerf {

// ---- device: per-image camera gradients ------------------------------------------------------------------------
// Two passes, no atomics (the reference adds every ray into 6 x n_images floats: every adder on a handful of rows,
// and a sum that depends on arrival order):
//   1. k_cam_ray_grad<L>: L lanes per kept ray stride its samples (rows of 28 B, consecutive lanes on consecutive
//      rows), then an xor butterfly over the L lanes; lane 0 stores the ray's six floats {go, cross(d, gd)} (zeros
//      for a ray without samples). Lane l adds samples l, l + L, ... in order, so the summation tree is a function
//      of (n, L) alone.
//   2. k_cam_image_sum: one block per image. Kept rays keep their ray order and image_idx is monotone in the ray id,
//      so the image's rays are one contiguous segment of ray_grad, found by binary search on ray_indices; thread t
//      adds rows lo + t, lo + t + 256, ... in order, then a fixed tree over the block. The six sums are added onto
//      pos_grad / rot_grad by one thread.
struct CamGradArgs {
	uint32_t n_rays_cap;        // rows of ray_grad: an upper bound of *ray_counter known on the host
	uint32_t n_rays_total, n_images;
	const uint32_t* ray_counter;
	const uint32_t* ray_indices;
	const float* rays;          // [R x 6] {o, d} (d unnormalised)
	const uint32_t* numsteps;   // [R x 2] {n, base} after the loss pass
	const float* coords;        // [B x 7]
	const float* coords_grad;   // [B x grad_stride] fp32, rows 0..2 position, 4..6 direction
	uint32_t grad_stride;
	float aabb_min[3], aabb_max[3];
	float* ray_grad;            // [n_rays_cap x 6] workspace
	float* pos_grad;            // [n_images x 3], accumulated
	float* rot_grad;            // [n_images x 3], accumulated
};
// The distortion map's share of pass 1 (compute_cam_gradient_train_nerf's distortion branch, testbed_nerf.cu:2088-2099):
// k_cam_ray_grad's DIST forms take these behind their arguments (CamGradArgsDist) and lane 0, which holds the ray's summed gd and
// d = normalize(ray.d), also stores (inverse(mat3(xform_img)) * (gd - d * dot(gd, d))).xy, the image-plane gradient, into
// dist_grad [n_rays_cap x 2] (zeros for a ray without samples). inverse is the general 3x3 inverse by the adjugate
// (glm::inverse), not the transpose. mats: image i's column-major 3x3 at mats + i * mat_stride floats (a Camera's m, or
// packed matrices). The six pose floats are computed by the same text as without DIST.
struct CamDistArgs {
	const float* mats;
	uint32_t mat_stride;
	float* dist_grad;
};
struct CamGradArgsDist : CamGradArgs {
	CamDistArgs dist;
};
// lanes per ray of pass 1: 1, 8, 16 or 64 (camera pose refinement, has the measurement behind the choice;
// a build with -DNGP_CAM_GRAD_LANES=n repeats it)
#ifndef NGP_CAM_GRAD_LANES
#define NGP_CAM_GRAD_LANES 64
#endif
constexpr uint32_t CAM_GRAD_LANES = NGP_CAM_GRAD_LANES;
constexpr uint32_t CAM_SUM_THREADS = 256;

// Both passes on `s`. lanes (per ray, pass 1): 1, 8, 16 or 64.
void camera_gradients(const CamGradArgs& a, uint32_t lanes, hipStream_t s);
// Pass 1's DIST form; pass 2 only with image_sums (optimize_extrinsics on): with the distortion map alone no per-image
// sum is wanted and k_cam_image_sum is not launched
void camera_gradients_distortion(const CamGradArgs& a, const CamDistArgs& d, uint32_t lanes, bool image_sums, hipStream_t s);

}  // namespace nerf

// ---- host: per-camera optimisers -------------------------------------------------------------------------------
// rotvec / rotmat (common_device.cuh:698-722) go through tcnn's quaternion helpers, which are absent here. The
// rotation vector of a matrix is taken from its quaternion (glm quat_cast) as axis * angle with
//   angle = 2 atan2(|xyz|, w)
// which is well conditioned at the 1e-4 rad rotations this optimiser makes; 2 acos(w) is not: w rounds to 1 there
// and the angle to 0, or to a multiple of ~4.9e-4.
namespace pose {

struct AdamState {  // AdamOptimizer<vec3> / RotationAdamOptimizer state + hyperparameters (adam_optimizer.h:196-209, 287-300)
	uint32_t iter = 0;
	float first_moment[3] = {0.f, 0.f, 0.f}, second_moment[3] = {0.f, 0.f, 0.f}, variable[3] = {0.f, 0.f, 0.f};
	float learning_rate = 1e-4f, epsilon = 1e-8f, beta1 = 0.9f, beta2 = 0.99f;
};

void rotmat(const float v[3], float m[9]);      // column-major 3x3, m[3c + r]
void rotvec(const float m[9], float v[3]);
void compose_rotation(const float a[3], const float b[3], float out[3]);  // rotvec(rotmat(a) * rotmat(b))
void adam_step_position(AdamState& s, const float grad[3]);
void adam_step_rotation(AdamState& s, const float grad[3]);
// update_transforms for one image (testbed_nerf.cu:2998-3019)
void apply(const float xform[12], const float rot_offset[3], const float pos_offset[3], float out[12]);

}  // namespace pose
}  // namespace ngp
