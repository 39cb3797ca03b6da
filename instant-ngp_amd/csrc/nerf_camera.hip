// nerf_camera.hip — camera pose refinement: the per-image gradient kernels with their C-ABI
// (ngp_nerf_camera_gradients) and the host-only per-camera optimisers (ngp_pose_optimizer_*, ngp_pose_apply); and the
// per-image exposure's share of the same machinery: the per-image sum of the loss pass's per-ray exposure gradients
// (exposure_gradients, nerf.h) and the host-only per-image optimisers (ngp_exposure_optimizer_*).
#include <cmath>
#include <cstring>
#include <memory>
#include <vector>

#include "abi_guard.h"
#include "nerf.h"
#include "nerf_camera.h"

using namespace ngp;

// ---- device: per-image camera gradients (the two passes are described in nerf_camera.h) ----------------------------
namespace ngp {
namespace nerf {

// image_idx (testbed_nerf.cu:1317-1338), uniform branch: monotone in the ray id
__device__ __forceinline__ uint32_t cam_image_idx(uint32_t ray_idx, uint32_t n_rays_total, uint32_t n_images) {
	return ((ray_idx * n_images) / n_rays_total) % n_images;
}

template <bool DIST> using CamGradArgsK = std::conditional_t<DIST, CamGradArgsDist, CamGradArgs>;
__device__ __forceinline__ CamDistArgs dist_of(const CamGradArgs&) { return CamDistArgs{}; }
__device__ __forceinline__ CamDistArgs dist_of(const CamGradArgsDist& a) { return a.dist; }

template <uint32_t L, bool DIST>
__global__ void __launch_bounds__(256) k_cam_ray_grad(CamGradArgsK<DIST> a) {
	const uint32_t n_kept = min(*a.ray_counter, a.n_rays_cap);
	const uint32_t lane = threadIdx.x % L;
	const float diag[3] = {a.aabb_max[0] - a.aabb_min[0], a.aabb_max[1] - a.aabb_min[1], a.aabb_max[2] - a.aabb_min[2]};
	const uint32_t groups = gridDim.x * (256 / L);
	// whole groups enter and leave the loop together: the shuffles below see all their lanes
	for (uint32_t i = blockIdx.x * (256 / L) + threadIdx.x / L; i < n_kept; i += groups) {
		const uint32_t n = a.numsteps[2 * i], base = a.numsteps[2 * i + 1];
		const float* ray = a.rays + 6 * (size_t)i;
		const float o[3] = {ray[0], ray[1], ray[2]};
		float g[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};  // go, gd
		for (uint32_t j = lane; j < n; j += L) {
			const float* c = a.coords + 7 * (size_t)(base + j);
			const float* cg = a.coords_grad + (size_t)a.grad_stride * (base + j);
			float dist2 = 0.f, gp[3];
			for (int k = 0; k < 3; ++k) {
				gp[k] = cg[k] / diag[k];                             // warp_position_derivative
				const float p = a.aabb_min[k] + c[k] * diag[k];     // unwarp_position
				dist2 += (p - o[k]) * (p - o[k]);
			}
			const float t = sqrtf(dist2);
			for (int k = 0; k < 3; ++k) {
				g[k] += gp[k];
				g[3 + k] += gp[k] * t + cg[4 + k] * 0.5f;            // warp_direction_derivative = 0.5
			}
		}
		for (uint32_t off = L / 2; off > 0; off >>= 1)
			for (int k = 0; k < 6; ++k) g[k] += __shfl_xor(g[k], (int)off);
		if (lane == 0) {
			float d[3] = {ray[3], ray[4], ray[5]};
			const float il = 1.0f / sqrtf(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
			for (int k = 0; k < 3; ++k) d[k] *= il;
			float* out = a.ray_grad + 6 * (size_t)i;
			out[0] = g[0]; out[1] = g[1]; out[2] = g[2];
			out[3] = d[1] * g[5] - d[2] * g[4];
			out[4] = d[2] * g[3] - d[0] * g[5];
			out[5] = d[0] * g[4] - d[1] * g[3];
			if (DIST) {
				const CamDistArgs dm = dist_of(a);
				float* dg = dm.dist_grad + 2 * (size_t)i;
				if (n == 0) {
					dg[0] = dg[1] = 0.f;
				} else {
					const float dt = g[3] * d[0] + g[4] * d[1] + g[5] * d[2];
					const float ox = g[3] - d[0] * dt, oy = g[4] - d[1] * dt, oz = g[5] - d[2] * dt;
					const float* m = dm.mats + (size_t)dm.mat_stride * cam_image_idx(a.ray_indices[i], a.n_rays_total, a.n_images);
					// the first two rows of inverse(mat3(m)) via the adjugate (glm::inverse), as k_mark_untrained takes it
					const float a00 = m[0], a01 = m[1], a02 = m[2], a10 = m[3], a11 = m[4], a12 = m[5], a20 = m[6], a21 = m[7], a22 = m[8];
					const float det = a00 * (a11 * a22 - a21 * a12) - a10 * (a01 * a22 - a21 * a02) + a20 * (a01 * a12 - a11 * a02);
					const float id = 1.0f / det;
					const float I0 = (a11 * a22 - a21 * a12) * id, I3 = -(a10 * a22 - a20 * a12) * id, I6 = (a10 * a21 - a20 * a11) * id;
					const float I1 = -(a01 * a22 - a21 * a02) * id, I4 = (a00 * a22 - a20 * a02) * id, I7 = -(a00 * a21 - a20 * a01) * id;
					dg[0] = I0 * ox + I3 * oy + I6 * oz;
					dg[1] = I1 * ox + I4 * oy + I7 * oz;
				}
			}
		}
	}
}


__global__ void __launch_bounds__(CAM_SUM_THREADS) k_cam_image_sum(CamGradArgs a) {
	const uint32_t n_kept = min(*a.ray_counter, a.n_rays_cap);
	const uint32_t img = blockIdx.x;
	// first kept ray whose image is >= img, and >= img + 1
	auto lower = [&](uint32_t target) {
		uint32_t lo = 0, hi = n_kept;
		while (lo < hi) {
			const uint32_t mid = lo + (hi - lo) / 2;
			if (cam_image_idx(a.ray_indices[mid], a.n_rays_total, a.n_images) < target) lo = mid + 1;
			else hi = mid;
		}
		return lo;
	};
	const uint32_t lo = lower(img), hi = img + 1 == a.n_images ? n_kept : lower(img + 1);
	if (lo >= hi) return;  // no kept ray of this image: the sums stay as they are
	float g[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
	for (uint32_t r = lo + threadIdx.x; r < hi; r += CAM_SUM_THREADS) {
		const float* row = a.ray_grad + 6 * (size_t)r;
		for (int k = 0; k < 6; ++k) g[k] += row[k];
	}
	for (int off = 32; off > 0; off >>= 1)
		for (int k = 0; k < 6; ++k) g[k] += __shfl_xor(g[k], off);
	__shared__ float part[CAM_SUM_THREADS / 64][6];
	if ((threadIdx.x & 63) == 0)
		for (int k = 0; k < 6; ++k) part[threadIdx.x >> 6][k] = g[k];
	__syncthreads();
	if (threadIdx.x < 6) {
		float s = 0.f;
		for (uint32_t w = 0; w < CAM_SUM_THREADS / 64; ++w) s += part[w][threadIdx.x];
		float* dst = threadIdx.x < 3 ? a.pos_grad + 3 * (size_t)img + threadIdx.x : a.rot_grad + 3 * (size_t)img + (threadIdx.x - 3);
		*dst += s;
	}
}

void camera_gradients(const CamGradArgs& a, uint32_t lanes, hipStream_t s) {
	if (a.n_rays_cap == 0 || a.n_images == 0) return;
	const uint32_t blocks = std::min(div_round_up((uint64_t)a.n_rays_cap * lanes, 256), 8u * 256u);
	switch (lanes) {
		case 1: k_cam_ray_grad<1, false><<<blocks, 256, 0, s>>>(a); break;
		case 8: k_cam_ray_grad<8, false><<<blocks, 256, 0, s>>>(a); break;
		case 16: k_cam_ray_grad<16, false><<<blocks, 256, 0, s>>>(a); break;
		case 64: k_cam_ray_grad<64, false><<<blocks, 256, 0, s>>>(a); break;
		default: throw Error("camera_gradients: lanes per ray must be 1, 8, 16 or 64");
	}
	NGP_HIP(hipGetLastError());
	k_cam_image_sum<<<a.n_images, CAM_SUM_THREADS, 0, s>>>(a);
	NGP_HIP(hipGetLastError());
}

void camera_gradients_distortion(const CamGradArgs& a, const CamDistArgs& d, uint32_t lanes, bool image_sums, hipStream_t s) {
	if (a.n_rays_cap == 0 || a.n_images == 0) return;
	const uint32_t blocks = std::min(div_round_up((uint64_t)a.n_rays_cap * lanes, 256), 8u * 256u);
	CamGradArgsDist ad;
	(CamGradArgs&)ad = a;
	ad.dist = d;
	switch (lanes) {
		case 1: k_cam_ray_grad<1, true><<<blocks, 256, 0, s>>>(ad); break;
		case 8: k_cam_ray_grad<8, true><<<blocks, 256, 0, s>>>(ad); break;
		case 16: k_cam_ray_grad<16, true><<<blocks, 256, 0, s>>>(ad); break;
		case 64: k_cam_ray_grad<64, true><<<blocks, 256, 0, s>>>(ad); break;
		default: throw Error("camera_gradients: lanes per ray must be 1, 8, 16 or 64");
	}
	NGP_HIP(hipGetLastError());
	if (!image_sums) return;
	k_cam_image_sum<<<a.n_images, CAM_SUM_THREADS, 0, s>>>(a);
	NGP_HIP(hipGetLastError());
}

// The exposure gradient per image (nerf.h): k_cam_image_sum's segment search and summation tree over three floats a
// ray, counting the rays the loss pass compacted to at least one sample
__global__ void __launch_bounds__(CAM_SUM_THREADS) k_exposure_image_sum(ExposureGradArgs a) {
	const uint32_t n_kept = min(*a.ray_counter, a.n_rays_cap);
	const uint32_t img = blockIdx.x;
	auto lower = [&](uint32_t target) {
		uint32_t lo = 0, hi = n_kept;
		while (lo < hi) {
			const uint32_t mid = lo + (hi - lo) / 2;
			if (cam_image_idx(a.ray_indices[mid], a.n_rays_total, a.n_images) < target) lo = mid + 1;
			else hi = mid;
		}
		return lo;
	};
	const uint32_t lo = lower(img), hi = img + 1 == a.n_images ? n_kept : lower(img + 1);
	float g[3] = {0.f, 0.f, 0.f};
	uint32_t counted = 0;
	for (uint32_t r = lo + threadIdx.x; r < hi; r += CAM_SUM_THREADS) {
		if (a.numsteps[2 * (size_t)r] == 0) continue;  // cut to no sample by the compacted budget, or without samples
		const float* row = a.ray_grad + 3 * (size_t)r;
		for (int k = 0; k < 3; ++k) g[k] += row[k];
		++counted;
	}
	for (int off = 32; off > 0; off >>= 1) {
		for (int k = 0; k < 3; ++k) g[k] += __shfl_xor(g[k], off);
		counted += __shfl_xor(counted, off);
	}
	__shared__ float part[CAM_SUM_THREADS / 64][3];
	__shared__ uint32_t part_n[CAM_SUM_THREADS / 64];
	if ((threadIdx.x & 63) == 0) {
		for (int k = 0; k < 3; ++k) part[threadIdx.x >> 6][k] = g[k];
		part_n[threadIdx.x >> 6] = counted;
	}
	__syncthreads();
	if (threadIdx.x < 3) {
		float s = 0.f;
		uint32_t n = 0;
		for (uint32_t w = 0; w < CAM_SUM_THREADS / 64; ++w) { s += part[w][threadIdx.x]; n += part_n[w]; }
		if (n) a.image_grad[3 * (size_t)img + threadIdx.x] += s;  // no counted ray: the accumulator keeps its bits
	}
}

void exposure_gradients(const ExposureGradArgs& a, hipStream_t s) {
	if (a.n_rays_cap == 0 || a.n_images == 0) return;
	k_exposure_image_sum<<<a.n_images, CAM_SUM_THREADS, 0, s>>>(a);
	NGP_HIP(hipGetLastError());
}

}  // namespace nerf
}  // namespace ngp

// ---- host pose math --------------------------------------------------------------------------------------------
namespace ngp {
namespace pose {

void rotmat(const float v[3], float m[9]) {
	const float angle = sqrtf(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
	if (angle == 0.0f) {
		for (int k = 0; k < 9; ++k) m[k] = k % 4 == 0 ? 1.f : 0.f;
		return;
	}
	const float x = v[0] / angle, y = v[1] / angle, z = v[2] / angle;
	const float s = sinf(angle), c = cosf(angle), oc = 1.0f - c;
	m[0] = oc * x * x + c;     m[1] = oc * x * y + z * s; m[2] = oc * z * x - y * s;
	m[3] = oc * x * y - z * s; m[4] = oc * y * y + c;     m[5] = oc * y * z + x * s;
	m[6] = oc * z * x + y * s; m[7] = oc * y * z - x * s; m[8] = oc * z * z + c;
}

void rotvec(const float m[9], float v[3]) {
	// glm quat_cast: the largest of w, x, y, z first
	auto M = [&](int c, int r) { return m[3 * c + r]; };
	const float fx = M(0, 0) - M(1, 1) - M(2, 2), fy = M(1, 1) - M(0, 0) - M(2, 2), fz = M(2, 2) - M(0, 0) - M(1, 1);
	const float fw = M(0, 0) + M(1, 1) + M(2, 2);
	int bi = 0;
	float big = fw;
	if (fx > big) { big = fx; bi = 1; }
	if (fy > big) { big = fy; bi = 2; }
	if (fz > big) { big = fz; bi = 3; }
	const float bv = sqrtf(big + 1.0f) * 0.5f, mult = 0.25f / bv;
	float w, x, y, z;
	switch (bi) {
		case 0: w = bv; x = (M(1, 2) - M(2, 1)) * mult; y = (M(2, 0) - M(0, 2)) * mult; z = (M(0, 1) - M(1, 0)) * mult; break;
		case 1: w = (M(1, 2) - M(2, 1)) * mult; x = bv; y = (M(0, 1) + M(1, 0)) * mult; z = (M(2, 0) + M(0, 2)) * mult; break;
		case 2: w = (M(2, 0) - M(0, 2)) * mult; x = (M(0, 1) + M(1, 0)) * mult; y = bv; z = (M(1, 2) + M(2, 1)) * mult; break;
		default: w = (M(0, 1) - M(1, 0)) * mult; x = (M(2, 0) + M(0, 2)) * mult; y = (M(1, 2) + M(2, 1)) * mult; z = bv; break;
	}
	const float sn = sqrtf(x * x + y * y + z * z);
	if (sn == 0.0f) { v[0] = v[1] = v[2] = 0.f; return; }
	const float k = 2.0f * atan2f(sn, w) / sn;  // axis * angle; not 2 acos(w) (nerf_camera.h)
	v[0] = x * k; v[1] = y * k; v[2] = z * k;
}

static void matmul3(const float a[9], const float b[9], float out[9]) {  // column-major a * b
	for (int c = 0; c < 3; ++c)
		for (int r = 0; r < 3; ++r) out[3 * c + r] = a[r] * b[3 * c] + a[3 + r] * b[3 * c + 1] + a[6 + r] * b[3 * c + 2];
}

void compose_rotation(const float a[3], const float b[3], float out[3]) {
	float ma[9], mb[9], p[9];
	rotmat(a, ma);
	rotmat(b, mb);
	matmul3(ma, mb, p);
	rotvec(p, out);
}

// the bias-corrected step both optimisers share (adam_optimizer.h:145-152, 238-247): returns lr_t * m1 / (sqrt(m2) + eps)
static void adam_moments(AdamState& s, const float g[3], float step[3]) {
	++s.iter;
	const float lr = s.learning_rate * std::sqrt(1.0f - std::pow(s.beta2, (float)s.iter)) / (1.0f - std::pow(s.beta1, (float)s.iter));
	for (int k = 0; k < 3; ++k) {
		s.first_moment[k] = s.beta1 * s.first_moment[k] + (1.0f - s.beta1) * g[k];
		s.second_moment[k] = s.beta2 * s.second_moment[k] + (1.0f - s.beta2) * g[k] * g[k];
		step[k] = lr * s.first_moment[k] / (std::sqrt(s.second_moment[k]) + s.epsilon);
	}
}

void adam_step_position(AdamState& s, const float grad[3]) {
	float step[3];
	adam_moments(s, grad, step);
	for (int k = 0; k < 3; ++k) s.variable[k] -= step[k];
}

void adam_step_rotation(AdamState& s, const float grad[3]) {
	float step[3];
	adam_moments(s, grad, step);
	const float neg[3] = {-step[0], -step[1], -step[2]};
	float out[3];
	compose_rotation(neg, s.variable, out);
	memcpy(s.variable, out, sizeof out);
}

void apply(const float xform[12], const float rot_offset[3], const float pos_offset[3], float out[12]) {
	float x[12];
	memcpy(x, xform, sizeof x);
	const float det = x[0] * (x[4] * x[8] - x[7] * x[5]) - x[3] * (x[1] * x[8] - x[7] * x[2]) + x[6] * (x[1] * x[5] - x[4] * x[2]);
	if (std::fabs(det - 1.0f) > 0.01f) {  // a scaling component: normalised (testbed_nerf.cu:3002-3009)
		const float c = std::cbrt(det);
		for (int k = 0; k < 9; ++k) x[k] /= c;
	}
	// zero offsets leave the matrix as it is, bit for bit (a product with the identity would turn -0 into +0)
	if (rot_offset[0] != 0.f || rot_offset[1] != 0.f || rot_offset[2] != 0.f) {
		float r[9], p[9];
		rotmat(rot_offset, r);
		matmul3(r, x, p);
		memcpy(x, p, sizeof p);
	}
	for (int k = 0; k < 3; ++k)
		if (pos_offset[k] != 0.f) x[9 + k] += pos_offset[k];
	memcpy(out, x, sizeof x);
}

}  // namespace pose
}  // namespace ngp

struct ngp_pose_optimizer {
	std::vector<pose::AdamState> pos, rot;
};

struct ngp_exposure_optimizer {
	std::vector<pose::AdamState> v;
};

static void to_c(const pose::AdamState& s, ngp_adam_state* o) {
	o->iter = s.iter;
	memcpy(o->first_moment, s.first_moment, 12);
	memcpy(o->second_moment, s.second_moment, 12);
	memcpy(o->variable, s.variable, 12);
	o->learning_rate = s.learning_rate; o->epsilon = s.epsilon; o->beta1 = s.beta1; o->beta2 = s.beta2;
}
static void from_c(const ngp_adam_state& o, pose::AdamState* s) {
	s->iter = o.iter;
	memcpy(s->first_moment, o.first_moment, 12);
	memcpy(s->second_moment, o.second_moment, 12);
	memcpy(s->variable, o.variable, 12);
	s->learning_rate = o.learning_rate; s->epsilon = o.epsilon; s->beta1 = o.beta1; s->beta2 = o.beta2;
}

static int invalid(const char* what) {
	ngp::set_last_error(what);
	return NGP_INVALID;
}

extern "C" {

int ngp_pose_optimizer_create(uint32_t n_images, ngp_pose_optimizer** out) {
	if (!out || n_images == 0) return invalid("invalid argument: pose optimizer: n_images > 0 and an out pointer");
	auto o = new ngp_pose_optimizer();
	o->pos.resize(n_images);
	o->rot.resize(n_images);
	*out = o;
	return NGP_OK;
}
void ngp_pose_optimizer_destroy(ngp_pose_optimizer* o) { delete o; }
uint32_t ngp_pose_optimizer_n_images(const ngp_pose_optimizer* o) { return o ? (uint32_t)o->pos.size() : 0; }

int ngp_pose_optimizer_reset(ngp_pose_optimizer* o) {
	if (!o) return invalid("invalid argument: pose optimizer");
	// reset_state keeps the hyperparameters (adam_optimizer.h:170-172, 261-263)
	for (auto* v : {&o->pos, &o->rot})
		for (auto& s : *v) { pose::AdamState z; z.learning_rate = s.learning_rate; z.epsilon = s.epsilon; z.beta1 = s.beta1; z.beta2 = s.beta2; s = z; }
	return NGP_OK;
}
int ngp_pose_optimizer_reset_one(ngp_pose_optimizer* o, uint32_t i) {
	if (!o || i >= o->pos.size()) return invalid("invalid argument: pose optimizer: image index");
	for (auto* v : {&o->pos, &o->rot}) {
		pose::AdamState& s = (*v)[i];
		pose::AdamState z; z.learning_rate = s.learning_rate; z.epsilon = s.epsilon; z.beta1 = s.beta1; z.beta2 = s.beta2;
		s = z;
	}
	return NGP_OK;
}

int ngp_pose_optimizer_step(ngp_pose_optimizer* o, const float* pos_grad, const float* rot_grad, uint32_t n_steps_between,
                            float extrinsic_lr, float l2_reg, float network_lr) {
	if (!o || !pos_grad || !rot_grad || n_steps_between == 0) return invalid("invalid argument: pose optimizer step");
	const uint32_t n = (uint32_t)o->pos.size();
	const float scale = (float)n / 128.0f / (float)n_steps_between;  // per_camera_loss_scale (testbed_nerf.cu:3784)
	for (uint32_t i = 0; i < n; ++i) {
		pose::AdamState &p = o->pos[i], &r = o->rot[i];
		float gp[3], gr[3];
		for (int k = 0; k < 3; ++k) {
			gp[k] = pos_grad[3 * i + k] * scale + p.variable[k] * l2_reg;
			gr[k] = rot_grad[3 * i + k] * scale + r.variable[k] * l2_reg;
		}
		p.learning_rate = std::max(extrinsic_lr * std::pow(0.33f, (float)(p.iter / 128)), network_lr / 1000.0f);
		r.learning_rate = std::max(extrinsic_lr * std::pow(0.33f, (float)(r.iter / 128)), network_lr / 1000.0f);
		pose::adam_step_position(p, gp);
		pose::adam_step_rotation(r, gr);
	}
	return NGP_OK;
}

int ngp_pose_optimizer_get(const ngp_pose_optimizer* o, uint32_t i, ngp_adam_state* pos, ngp_adam_state* rot) {
	if (!o || i >= o->pos.size()) return invalid("invalid argument: pose optimizer: image index");
	if (pos) to_c(o->pos[i], pos);
	if (rot) to_c(o->rot[i], rot);
	return NGP_OK;
}
int ngp_pose_optimizer_set_state(ngp_pose_optimizer* o, uint32_t i, const ngp_adam_state* pos, const ngp_adam_state* rot) {
	if (!o || i >= o->pos.size()) return invalid("invalid argument: pose optimizer: image index");
	if (pos) from_c(*pos, &o->pos[i]);
	if (rot) from_c(*rot, &o->rot[i]);
	return NGP_OK;
}

// ---- per-image exposure optimisers (testbed_nerf.cu:3831-3858) ----------------------------------------------------
int ngp_exposure_optimizer_create(uint32_t n_images, ngp_exposure_optimizer** out) {
	if (!out || n_images == 0) return invalid("invalid argument: exposure optimizer: n_images > 0 and an out pointer");
	auto o = new ngp_exposure_optimizer();
	o->v.resize(n_images);
	for (auto& s : o->v) s.learning_rate = 1e-3f;  // testbed_nerf.cu:3036; overwritten before every step
	*out = o;
	return NGP_OK;
}
void ngp_exposure_optimizer_destroy(ngp_exposure_optimizer* o) { delete o; }
uint32_t ngp_exposure_optimizer_n_images(const ngp_exposure_optimizer* o) { return o ? (uint32_t)o->v.size() : 0; }

static void exposure_reset_state(pose::AdamState& s) {  // reset_state keeps the hyperparameters
	pose::AdamState z;
	z.learning_rate = s.learning_rate; z.epsilon = s.epsilon; z.beta1 = s.beta1; z.beta2 = s.beta2;
	s = z;
}
int ngp_exposure_optimizer_reset(ngp_exposure_optimizer* o) {
	if (!o) return invalid("invalid argument: exposure optimizer");
	for (auto& s : o->v) exposure_reset_state(s);
	return NGP_OK;
}
int ngp_exposure_optimizer_reset_one(ngp_exposure_optimizer* o, uint32_t i) {
	if (!o || i >= o->v.size()) return invalid("invalid argument: exposure optimizer: image index");
	exposure_reset_state(o->v[i]);
	return NGP_OK;
}

int ngp_exposure_optimizer_step(ngp_exposure_optimizer* o, const float* grad, uint32_t n_steps_between, float l2_reg, float network_lr) {
	if (!o || !grad || n_steps_between == 0 || !(l2_reg >= 0.0f)) return invalid("invalid argument: exposure optimizer step");
	const uint32_t n = (uint32_t)o->v.size();
	const float scale = (float)n / 128.0f / (float)n_steps_between;  // per_camera_loss_scale (testbed_nerf.cu:3784)
	float mean[3] = {0.f, 0.f, 0.f};
	for (uint32_t i = 0; i < n; ++i) {
		pose::AdamState& e = o->v[i];
		float g[3];
		for (int k = 0; k < 3; ++k) g[k] = grad[3 * i + k] * scale + e.variable[k] * l2_reg;
		e.learning_rate = network_lr;
		pose::adam_step_position(e, g);
		for (int k = 0; k < 3; ++k) mean[k] += e.variable[k];
	}
	for (int k = 0; k < 3; ++k) mean[k] /= (float)n;
	for (auto& e : o->v)  // renormalise: only the exposures' differences are identifiable
		for (int k = 0; k < 3; ++k) e.variable[k] -= mean[k];
	return NGP_OK;
}

int ngp_exposure_optimizer_get(const ngp_exposure_optimizer* o, uint32_t i, ngp_adam_state* out) {
	if (!o || !out || i >= o->v.size()) return invalid("invalid argument: exposure optimizer: image index");
	to_c(o->v[i], out);
	return NGP_OK;
}
int ngp_exposure_optimizer_set_state(ngp_exposure_optimizer* o, uint32_t i, const ngp_adam_state* state) {
	if (!o || !state || i >= o->v.size()) return invalid("invalid argument: exposure optimizer: image index");
	from_c(*state, &o->v[i]);
	return NGP_OK;
}

int ngp_pose_compose_rotation(const float* a, const float* b, float* out) {
	if (!a || !b || !out) return invalid("invalid argument: pose compose: null pointer");
	float r[3];
	pose::compose_rotation(a, b, r);
	memcpy(out, r, sizeof r);
	return NGP_OK;
}

int ngp_pose_apply(const float* xform, const float* rot_offset, const float* pos_offset, float* out) {
	if (!xform || !rot_offset || !pos_offset || !out) return invalid("invalid argument: pose apply: null pointer");
	pose::apply(xform, rot_offset, pos_offset, out);
	return NGP_OK;
}

// ngp_nerf_camera_gradients and ngp_nerf_distortion_ray_gradients (mats null: the former)
static int camera_gradients_abi(const ngp_nerf_config* cfg, void* stream, uint32_t n_rays_total, uint32_t n_images,
                                const uint32_t* ray_counter, const uint32_t* ray_indices, const float* rays, const uint32_t* numsteps,
                                const float* coords, const float* coords_gradient, uint32_t gradient_stride, float* pos_gradient,
                                float* rot_gradient, const float* mats, float* dist_grad) {
	NGP_TRY({
		nerf::CamGradArgs a{};
		// kept rays are distinct ids below n_rays_total: at most that many rows
		a.n_rays_cap = n_rays_total; a.n_rays_total = n_rays_total; a.n_images = n_images;
		a.ray_counter = ray_counter; a.ray_indices = ray_indices; a.rays = rays; a.numsteps = numsteps;
		a.coords = coords; a.coords_grad = coords_gradient; a.grad_stride = gradient_stride;
		for (int k = 0; k < 3; ++k) { a.aabb_min[k] = cfg->aabb_min[k]; a.aabb_max[k] = cfg->aabb_max[k]; }
		static thread_local struct Ws {
			float* p = nullptr; size_t n = 0;
			~Ws() { if (p) (void)hipFree(p); }
		} ws;
		const size_t need = (size_t)n_rays_total * 6 * sizeof(float);
		if (need > ws.n) {
			if (ws.p) NGP_HIP(hipFree(ws.p));
			ws.p = nullptr; ws.n = 0;
			NGP_HIP(hipMalloc((void**)&ws.p, need));
			ws.n = need;
		}
		a.ray_grad = ws.p; a.pos_grad = pos_gradient; a.rot_grad = rot_gradient;
		if (mats) nerf::camera_gradients_distortion(a, nerf::CamDistArgs{mats, 9, dist_grad}, nerf::CAM_GRAD_LANES, pos_gradient != nullptr,
		                                            (hipStream_t)stream);
		else nerf::camera_gradients(a, nerf::CAM_GRAD_LANES, (hipStream_t)stream);
	});
}

int ngp_nerf_camera_gradients(const ngp_nerf_config* cfg, void* stream, uint32_t n_rays_total, uint32_t n_images,
                              const uint32_t* ray_counter, const uint32_t* ray_indices, const float* rays,
                              const uint32_t* numsteps, const float* coords, const float* coords_gradient,
                              uint32_t gradient_stride, float* pos_gradient, float* rot_gradient) {
	if (!cfg || !ray_counter || !ray_indices || !rays || !numsteps || !coords || !coords_gradient || !pos_gradient || !rot_gradient ||
	    n_rays_total == 0 || n_images == 0 || gradient_stride < 7 || (uint64_t)n_rays_total * n_images > 0xffffffffull)
		return invalid("invalid argument: camera gradients: null pointer, no rays or images, gradient stride < 7 or n_rays_total * n_images >= 2^32");
	for (int k = 0; k < 3; ++k)
		if (!(cfg->aabb_max[k] > cfg->aabb_min[k])) return invalid("invalid argument: camera gradients: empty training box");
	return camera_gradients_abi(cfg, stream, n_rays_total, n_images, ray_counter, ray_indices, rays, numsteps, coords, coords_gradient,
	                            gradient_stride, pos_gradient, rot_gradient, nullptr, nullptr);
}

int ngp_nerf_distortion_ray_gradients(const ngp_nerf_config* cfg, void* stream, uint32_t n_rays_total, uint32_t n_images,
                                      const uint32_t* ray_counter, const uint32_t* ray_indices, const float* rays,
                                      const uint32_t* numsteps, const float* coords, const float* coords_gradient,
                                      uint32_t gradient_stride, float* pos_gradient, float* rot_gradient, const float* camera_matrices,
                                      float* ray_gradients) {
	if (!cfg || !ray_counter || !ray_indices || !rays || !numsteps || !coords || !coords_gradient || !camera_matrices || !ray_gradients ||
	    (pos_gradient == nullptr) != (rot_gradient == nullptr) || n_rays_total == 0 || n_images == 0 || gradient_stride < 7 ||
	    (uint64_t)n_rays_total * n_images > 0xffffffffull)
		return invalid("invalid argument: distortion ray gradients: null pointer, one pose gradient without the other, no rays or images, gradient stride < 7 or n_rays_total * n_images >= 2^32");
	for (int k = 0; k < 3; ++k)
		if (!(cfg->aabb_max[k] > cfg->aabb_min[k])) return invalid("invalid argument: distortion ray gradients: empty training box");
	return camera_gradients_abi(cfg, stream, n_rays_total, n_images, ray_counter, ray_indices, rays, numsteps, coords, coords_gradient,
	                            gradient_stride, pos_gradient, rot_gradient, camera_matrices, ray_gradients);
}

}  // extern "C"
