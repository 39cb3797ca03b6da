// nerf_trainer.hip — the Testbed-level NeRF trainer: create / destroy, its setters and getters, the density-grid
// update and the training step in its stages. The trainer object itself is in nerf_host.h; the sampler and loss
// wrappers the step calls (run_sampler, run_compute_loss) are in nerf_abi.hip, snapshots in nerf_snapshot.hip.
//
// ngp_nerf_train_step mirrors Testbed::train for NeRF (src/testbed.cu:4285-4370): training_prep_nerf
// (occupancy-grid update every clamp(step/16, 1, 16) steps, testbed_nerf.cu:4137-4152) then
// train_nerf (testbed_nerf.cu:3611-3862): sample -> inference over every sample -> loss/compaction
// -> rollover -> forward/backward on the compacted batch -> optimizer step -> counters (host sync) ->
// rays_per_batch adaptation.
#include <chrono>

#include <cstddef>

#include "distortion.h"
#include "nerf_host.h"
#include "profiler.h"

// mark_untrained_density_grid (testbed_nerf.cu:503-592) for perspective and OpenCV(-fisheye) cameras
__global__ void k_mark_untrained(uint32_t n_elements, float* __restrict__ grid, uint32_t n_images, const Camera* __restrict__ cams,
                                 const float* __restrict__ raw_xforms, bool clear_visible) {
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n_elements) return;
	if (grid[i] == -1.0f) return;
	const uint32_t level = i / GRID_N_CELLS, pos_idx = i % GRID_N_CELLS;
	auto inv = [](uint32_t x) {
		x = x & 0x49249249u; x = (x | (x >> 2)) & 0xc30c30c3u; x = (x | (x >> 4)) & 0x0f00f00fu;
		x = (x | (x >> 8)) & 0xff0000ffu; x = (x | (x >> 16)) & 0x0000ffffu; return x;
	};
	const uint32_t x = inv(pos_idx >> 0), y = inv(pos_idx >> 1), z = inv(pos_idx >> 2);
	const float vs = scalbnf(1.0f / GRIDSIZE, (int)level), sc = scalbnf(1.0f, (int)level);
	const float px = ((float)x / (float)GRIDSIZE - 0.5f) * sc + 0.5f;
	const float py = ((float)y / (float)GRIDSIZE - 0.5f) * sc + 0.5f;
	const float pz = ((float)z / (float)GRIDSIZE - 0.5f) * sc + 0.5f;
	uint32_t count = 0;
	for (uint32_t j = 0; j < n_images && count < 1; ++j) {
		const float* m = raw_xforms + 12 * j;  // training_xforms[j].start
		const Camera& cam = cams[j];
		// inverse(mat3(m)) via the adjugate (glm::inverse)
		const float a00 = m[0], a01 = m[1], a02 = m[2], a10 = m[3], a11 = m[4], a12 = m[5], a20 = m[6], a21 = m[7], a22 = m[8];
		const float det = a00 * (a11 * a22 - a21 * a12) - a10 * (a01 * a22 - a21 * a02) + a20 * (a01 * a12 - a11 * a02);
		const float id = 1.0f / det;
		float I[9];
		I[0] = (a11 * a22 - a21 * a12) * id; I[3] = -(a10 * a22 - a20 * a12) * id; I[6] = (a10 * a21 - a20 * a11) * id;
		I[1] = -(a01 * a22 - a21 * a02) * id; I[4] = (a00 * a22 - a20 * a02) * id; I[7] = -(a00 * a21 - a20 * a01) * id;
		I[2] = (a01 * a12 - a11 * a02) * id; I[5] = -(a00 * a12 - a10 * a02) * id; I[8] = (a00 * a11 - a10 * a01) * id;
		for (uint32_t k = 0; k < 8; ++k) {
			const float cx = px + ((k & 1) ? vs : 0.f), cy = py + ((k & 2) ? vs : 0.f), cz = pz + ((k & 4) ? vs : 0.f);
			float dx = cx - m[9], dy = cy - m[10], dz = cz - m[11];
			const float il = 1.0f / sqrtf(dx * dx + dy * dy + dz * dz);
			const float nx = dx * il, ny = dy * il, nz = dz * il;
			if (nx * m[6] + ny * m[7] + nz * m[8] < 1e-4f) continue;
			// pos_to_uv (common_device.cuh:547-585): perspective projection + forward lens distortion
			float ex = I[0] * dx + I[3] * dy + I[6] * dz, ey = I[1] * dx + I[4] * dy + I[7] * dz, ez = I[2] * dx + I[5] * dy + I[8] * dz;
			ex /= ez; ey /= ez;
			float du, dv;
			lens_delta(cam.lens_mode, cam.lens, ex, ey, &du, &dv);
			ex += du; ey += dv;
			const float u = ex * cam.focal[0] / (float)cam.width + cam.principal[0];
			const float v = ey * cam.focal[1] / (float)cam.height + cam.principal[1];
			// uv_to_ray with the raw xform (pos_to_uv is not injective under distortion), compare directions
			float rx = (u - cam.principal[0]) * (float)cam.width / cam.focal[0];
			float ry = (v - cam.principal[1]) * (float)cam.height / cam.focal[1];
			lens_undistort(cam.lens_mode, cam.lens, &rx, &ry);
			const float ddx = m[0] * rx + m[3] * ry + m[6], ddy = m[1] * rx + m[4] * ry + m[7], ddz = m[2] * rx + m[5] * ry + m[8];
			const float rl = 1.0f / sqrtf(ddx * ddx + ddy * ddy + ddz * ddz);
			const float qx = ddx * rl - nx, qy = ddy * rl - ny, qz = ddz * rl - nz;
			if (u > 0.0f && v > 0.0f && u < 1.0f && v < 1.0f && sqrtf(qx * qx + qy * qy + qz * qz) < 1e-3f) { ++count; break; }
		}
	}
	if (clear_visible || (grid[i] < 0) != (count < 1)) grid[i] = count >= 1 ? 1.f : -1.f;
	else grid[i] = 1.0f;
}

extern "C" {

// ---- Testbed-level ---------------------------------------------------------------------------
int ngp_nerf_trainer_create(ngp_model* model, ngp_trainer* trainer, const ngp_nerf_dataset* ds, const ngp_nerf_config* cfg,
                            uint64_t seed, ngp_nerf_trainer** out) {
	if (!model || !trainer || !ds || !cfg || !out) return NGP_INVALID;
	NGP_TRY({
		auto t = std::make_unique<ngp_nerf_trainer>();
		t->model = model; t->trainer = trainer; t->data = ds; t->cfg = *cfg;
		t->rng = HostPcg(seed);                          // m_rng = default_rng_t{m_seed} (testbed.cu:3906)
		t->grid_rng = HostPcg(t->rng.next_uint());       // density_grid_rng (testbed.cu:3919)
		const uint32_t n_el = GRID_N_CELLS * (cfg->max_cascade + 1);
		NGP_HIP(hipMemset(t->grid.get<float>(n_el), 0, (size_t)n_el * 4));
		NGP_HIP(hipMemset(t->bitfield.get<uint8_t>(BITFIELD_BYTES), 0, BITFIELD_BYTES));
		NGP_HIP(hipMemset(t->mean.get<float>(1 + 512), 0, (1 + 512) * 4));
		// the trainer's cameras: the dataset's, verbatim
		const Dataset& d = ds->ds;
		t->cams = d.cams;
		t->xforms = d.xforms;
		NGP_HIP(hipMalloc((void**)&t->d_cams, d.n_images * sizeof(Camera)));
		NGP_HIP(hipMemcpy(t->d_cams, d.d_cams, d.n_images * sizeof(Camera), hipMemcpyDeviceToDevice));
		NGP_HIP(hipMalloc((void**)&t->d_raw, (size_t)d.n_images * 12 * sizeof(float)));
		NGP_HIP(hipMemcpy(t->d_raw, d.xforms.data(), (size_t)d.n_images * 12 * sizeof(float), hipMemcpyHostToDevice));
		if (ngp_pose_optimizer_create(d.n_images, &t->pose) != NGP_OK) throw Error(ngp_last_error());
		if (ngp_exposure_optimizer_create(d.n_images, &t->expo) != NGP_OK) throw Error(ngp_last_error());
		*out = t.release();
	});
}

void ngp_nerf_trainer_destroy(ngp_nerf_trainer* t) { delete t; }

int ngp_nerf_trainer_get_config(const ngp_nerf_trainer* t, ngp_nerf_config* out) {
	if (!t || !out) return NGP_INVALID;
	*out = t->cfg;
	return NGP_OK;
}

int ngp_nerf_trainer_set_config(ngp_nerf_trainer* t, const ngp_nerf_config* cfg) {
	if (!t || !cfg) return NGP_INVALID;
	NGP_TRY({
		NGP_CHECK(cfg->max_cascade == t->cfg.max_cascade, "set_config: max_cascade sizes the density grid (reset the trainer)");
		for (int k = 0; k < 3; ++k)
			NGP_CHECK(cfg->aabb_min[k] == t->cfg.aabb_min[k] && cfg->aabb_max[k] == t->cfg.aabb_max[k],
			          "set_config: the aabb is fixed for the trainer's lifetime (reset the trainer)");
		NGP_CHECK(cfg->target_batch_size > 0 && cfg->target_batch_size % 256 == 0, "set_config: target_batch_size");
		t->drain();  // a prelaunched sampler ran with the old knobs
		const bool early_was = t->early();
		t->cfg = *cfg;
		// the sample-set choice changes with the cone (ngp_nerf_trainer::early): let the last step's passes finish
		// reading their set first
		if (t->early() != early_was) NGP_HIP(hipDeviceSynchronize());
	});
}

// ---- camera pose refinement: the trainer's cameras -----------------------------------------------------------------
// Training::update_transforms (testbed_nerf.cu:2980-3024) for image i: its transform with the optimisers' offsets
void ngp_nerf_trainer::refined_xform(uint32_t i, float out[12]) const {
	ngp_adam_state p, r;
	check_rc(ngp_pose_optimizer_get(pose, i, &p, &r));
	ngp::pose::apply(&xforms[(size_t)12 * i], r.variable, p.variable, out);
}
// ... for every image, into the cameras the sampler traces and the raw transforms mark_untrained_density_grid reads.
// Uploaded on `s` and waited for: the caller launches the next sampler afterwards, on any stream.
void ngp_nerf_trainer::rebuild_cameras(hipStream_t s) {
	const uint32_t n = (uint32_t)cams.size();
	std::vector<float> raw((size_t)12 * n);
	for (uint32_t i = 0; i < n; ++i) {
		refined_xform(i, &raw[(size_t)12 * i]);
		effective_camera_matrix(&raw[(size_t)12 * i], cams[i].m);
	}
	NGP_HIP(hipMemcpyAsync(d_cams, cams.data(), n * sizeof(Camera), hipMemcpyHostToDevice, s));
	NGP_HIP(hipMemcpyAsync(d_raw, raw.data(), raw.size() * sizeof(float), hipMemcpyHostToDevice, s));
	NGP_HIP(hipStreamSynchronize(s));
}
// the poses are about to change outside a step: nothing may still trace, or be launched to trace, the old ones
static void cameras_quiesce(ngp_nerf_trainer* t) {
	t->drain();
	NGP_HIP(hipDeviceSynchronize());
}

// The per-image gradient sums rely on an image's rays being one contiguous run of the batch (k_cam_image_sum), which
// the image CDF breaks, and the reference divides the ray gradients by uv_pdf: neither is implemented
static const char* const ERROR_SAMPLING_VS_EXTRINSICS =
	"optimize_extrinsics cannot be combined with sample_focal_plane_proportional_to_error / "
	"sample_image_proportional_to_error: turn one of them off first";
// The exposure gradient's per-image sum relies on the same contiguous runs; it does divide by uv_pdf, so drawing the
// position in the image from the error map is allowed
static const char* const IMAGE_SAMPLING_VS_EXPOSURE =
	"optimize_exposure cannot be combined with sample_image_proportional_to_error: turn one of them off first";
static const char* const EXPOSURE_VS_DATA_PARALLEL =
	"exposure optimisation is single-GPU: the per-image gradient sums of a data-parallel trainer would need their own "
	"all-reduce";

// The deposit recomputes a ray's uv by the uniform draw and takes uv_pdf as 1
static const char* const ERROR_SAMPLING_VS_DISTORTION =
	"optimize_distortion cannot be combined with sample_focal_plane_proportional_to_error / "
	"sample_image_proportional_to_error: turn one of them off first";
static const char* const DISTORTION_VS_DATA_PARALLEL =
	"optimize_distortion is single-GPU (the distortion map's gradient is not all-reduced): it cannot be combined with a "
	"data-parallel exchange hook; turn one of them off first";

int ngp_nerf_trainer_set_error_sampling(ngp_nerf_trainer* t, int focal_plane, int image) {
	if (!t) return NGP_INVALID;
	NGP_TRY({
		NGP_CHECK(!(focal_plane || image) || !t->cam.optimize_extrinsics, ERROR_SAMPLING_VS_EXTRINSICS);
		NGP_CHECK(!(focal_plane || image) || !t->dist.optimize, ERROR_SAMPLING_VS_DISTORTION);
		NGP_CHECK(!image || !t->optimize_exposure, IMAGE_SAMPLING_VS_EXPOSURE);
		t->drain();  // a prelaunched sampler drew its pixels under the old switches
		t->sample_focal_plane_by_error = focal_plane != 0;
		t->sample_image_by_error = image != 0;
	});
}
int ngp_nerf_trainer_get_error_sampling(const ngp_nerf_trainer* t, int* focal_plane, int* image) {
	if (!t) return NGP_INVALID;
	if (focal_plane) *focal_plane = t->sample_focal_plane_by_error ? 1 : 0;
	if (image) *image = t->sample_image_by_error ? 1 : 0;
	return NGP_OK;
}

// ---- depth supervision -------------------------------------------------------------------------------------------
// Training::depth_supervision_lambda / depth_loss_type (testbed.h:719, 745). Only the loss pass reads them: the sampler,
// and so a prelaunched one, does not depend on them, and nothing is discarded.
int ngp_nerf_trainer_set_depth_supervision(ngp_nerf_trainer* t, float lambda, uint32_t loss_type) {
	if (!t || !(lambda >= 0.0f) || std::isinf(lambda) || loss_type > LOSS_RELL2) return NGP_INVALID;
	t->depth_lambda = lambda;
	t->depth_loss_type = loss_type;
	return NGP_OK;
}
int ngp_nerf_trainer_get_depth_supervision(const ngp_nerf_trainer* t, float* lambda, uint32_t* loss_type) {
	if (!t) return NGP_INVALID;
	if (lambda) *lambda = t->depth_lambda;
	if (loss_type) *loss_type = t->depth_loss_type;
	return NGP_OK;
}

// ---- environment map ---------------------------------------------------------------------------------------------
// The map's gradient is summed on one GPU and stepped there; all-reducing it is not implemented
static const char* const TRAIN_ENVMAP_VS_DATA_PARALLEL =
	"train_envmap is single-GPU (the environment map's gradient is not all-reduced): it cannot be combined with a "
	"data-parallel exchange hook; turn one of them off first";

int ngp_nerf_trainer_set_envmap(ngp_nerf_trainer* t, uint32_t width, uint32_t height, const float* rgba) {
	if (!t || !envmap_dims_ok(width, height)) return NGP_INVALID;
	NGP_TRY({
		NGP_HIP(hipDeviceSynchronize());  // the last step may still read the old map (the prelaunched sampler reads none)
		ngp_nerf_trainer::Envmap& e = t->env;
		e.w = width; e.h = height; e.step = 0; e.ema_valid = false;
		const size_t n = e.n(), b = n * sizeof(float);
		float* p = e.params.get<float>(n);
		if (rgba) NGP_HIP(hipMemcpy(p, rgba, b, hipMemcpyHostToDevice));
		else NGP_HIP(hipMemset(p, 0, b));
		for (Buf* q : {&e.ema, &e.ema_out, &e.m1, &e.m2, &e.steps, &e.grad}) NGP_HIP(hipMemset(q->get<float>(n), 0, b));
		(void)e.acc.get<unsigned long long>(envmap_acc_words64(width, height));
	});
}

int ngp_nerf_trainer_clear_envmap(ngp_nerf_trainer* t) {
	if (!t) return NGP_INVALID;
	NGP_TRY({
		NGP_HIP(hipDeviceSynchronize());
		t->env.w = t->env.h = 0;
		t->env.step = 0;
		t->env.ema_valid = false;
	});
}

static const float* envmap_array(const ngp_nerf_trainer* t, int which) {
	const ngp_nerf_trainer::Envmap& e = t->env;
	switch (which) {
		case NGP_ENVMAP_PARAMS: return (const float*)e.params.p;
		case NGP_ENVMAP_INFERENCE_PARAMS: return t->envmap_inference();
		case NGP_ENVMAP_GRADIENT: return (const float*)e.grad.p;
		case NGP_ENVMAP_FIRST_MOMENTS: return (const float*)e.m1.p;
		case NGP_ENVMAP_SECOND_MOMENTS: return (const float*)e.m2.p;
		case NGP_ENVMAP_PARAM_STEPS: return (const float*)e.steps.p;
	}
	return nullptr;
}

int ngp_nerf_trainer_envmap(const ngp_nerf_trainer* t, int which, float* out, uint64_t cap, uint32_t* width, uint32_t* height) {
	if (!t || which < NGP_ENVMAP_PARAMS || which > NGP_ENVMAP_PARAM_STEPS) return NGP_INVALID;
	if (width) *width = t->env.w;
	if (height) *height = t->env.h;
	if (!out || !t->env.bound()) return NGP_OK;
	if (cap < t->env.n()) return NGP_INVALID;
	NGP_TRY({
		NGP_HIP(hipDeviceSynchronize());
		NGP_HIP(hipMemcpy(out, envmap_array(t, which), t->env.n() * sizeof(float), hipMemcpyDeviceToHost));
	});
}

int ngp_nerf_trainer_envmap_device(const ngp_nerf_trainer* t, int which, const float** data, uint32_t* width, uint32_t* height) {
	if (!t || !data || (which != NGP_ENVMAP_PARAMS && which != NGP_ENVMAP_INFERENCE_PARAMS)) return NGP_INVALID;
	*data = t->env.bound() ? envmap_array(t, which) : nullptr;
	if (width) *width = t->env.w;
	if (height) *height = t->env.h;
	return NGP_OK;
}

int ngp_nerf_trainer_set_train_envmap(ngp_nerf_trainer* t, int train) {
	if (!t) return NGP_INVALID;
	NGP_TRY({
		NGP_CHECK(!train || !t->dp(), TRAIN_ENVMAP_VS_DATA_PARALLEL);
		t->env.train = train != 0;
	});
}

int ngp_nerf_trainer_get_train_envmap(const ngp_nerf_trainer* t, int* train) {
	if (!t || !train) return NGP_INVALID;
	*train = t->env.train ? 1 : 0;
	return NGP_OK;
}

int ngp_nerf_trainer_set_envmap_training(ngp_nerf_trainer* t, int loss_type, const char* optimizer_json) {
	if (!t || loss_type < -1 || loss_type > (int)LOSS_RELL2) return NGP_INVALID;
	NGP_TRY({
		AdamConfig c;
		if (optimizer_json) parse_optimizer_json(optimizer_json, c);
		t->env.loss_type = loss_type;
		t->env.opt_set = optimizer_json != nullptr;
		if (optimizer_json) t->env.opt = c;
	});
}

// ---- lens distortion map -----------------------------------------------------------------------------------------
// the map is about to change outside a step: nothing may still trace through, or be launched to trace through, the old one
int ngp_nerf_trainer_set_distortion_map(ngp_nerf_trainer* t, uint32_t width, uint32_t height, const float* params) {
	if (!t || !distortion_dims_ok(width, height)) return NGP_INVALID;
	NGP_TRY({
		cameras_quiesce(t);
		ngp_nerf_trainer::Distortion& d = t->dist;
		d.w = width; d.h = height; d.step = 0; d.ema_valid = false;
		const size_t n = d.n(), b = n * sizeof(float);
		float* p = d.params.get<float>(n);
		if (params) NGP_HIP(hipMemcpy(p, params, b, hipMemcpyHostToDevice));
		else NGP_HIP(hipMemset(p, 0, b));  // TrainableBuffer::initialize_params
		for (Buf* q : {&d.ema, &d.ema_out, &d.m1, &d.m2, &d.steps, &d.grad}) NGP_HIP(hipMemset(q->get<float>(n), 0, b));
		const size_t words = distortion_acc_words64(width, height);
		NGP_HIP(hipMemset(d.acc.get<unsigned long long>(words), 0, words * 8));
		if (d.optimize && !t->cam.optimize_extrinsics && !t->optimize_exposure) t->n_steps_since_cam_update = 0;
	});
}

int ngp_nerf_trainer_clear_distortion_map(ngp_nerf_trainer* t) {
	if (!t) return NGP_INVALID;
	NGP_TRY({
		cameras_quiesce(t);
		t->dist.w = t->dist.h = 0;
		t->dist.step = 0;
		t->dist.ema_valid = false;
		t->dist.optimize = false;  // nothing left to optimise
	});
}

static const void* distortion_array(const ngp_nerf_trainer* t, int which) {
	const ngp_nerf_trainer::Distortion& d = t->dist;
	switch (which) {
		case NGP_DISTORTION_PARAMS: return d.params.p;
		case NGP_DISTORTION_GRADIENT: return d.grad.p;
		case NGP_DISTORTION_FIRST_MOMENTS: return d.m1.p;
		case NGP_DISTORTION_SECOND_MOMENTS: return d.m2.p;
		case NGP_DISTORTION_PARAM_STEPS: return d.steps.p;
		case NGP_DISTORTION_INFERENCE_PARAMS: return t->distortion_inference();
	}
	return nullptr;
}

int ngp_nerf_trainer_distortion_map(const ngp_nerf_trainer* t, int which, float* out, uint64_t cap, uint32_t* width, uint32_t* height) {
	if (!t || which < NGP_DISTORTION_PARAMS || which > NGP_DISTORTION_INFERENCE_PARAMS) return NGP_INVALID;
	if (width) *width = t->dist.w;
	if (height) *height = t->dist.h;
	if (!out || !t->dist.bound()) return NGP_OK;
	if (cap < t->dist.n()) return NGP_INVALID;
	NGP_TRY({
		NGP_HIP(hipDeviceSynchronize());
		NGP_HIP(hipMemcpy(out, distortion_array(t, which), t->dist.n() * sizeof(float), hipMemcpyDeviceToHost));
	});
}

int ngp_nerf_trainer_distortion_map_device(const ngp_nerf_trainer* t, int which, const float** data, uint32_t* width, uint32_t* height) {
	if (!t || !data || (which != NGP_DISTORTION_PARAMS && which != NGP_DISTORTION_INFERENCE_PARAMS)) return NGP_INVALID;
	*data = t->dist.bound() ? (const float*)distortion_array(t, which) : nullptr;
	if (width) *width = t->dist.w;
	if (height) *height = t->dist.h;
	return NGP_OK;
}

int ngp_nerf_trainer_distortion_accumulator(const ngp_nerf_trainer* t, uint64_t* out, uint64_t cap, uint64_t* words) {
	if (!t) return NGP_INVALID;
	const uint64_t n = t->dist.bound() ? (uint64_t)distortion_acc_words64(t->dist.w, t->dist.h) : 0;
	if (words) *words = n;
	if (!out || n == 0) return NGP_OK;
	if (cap < n) return NGP_INVALID;
	NGP_TRY({
		NGP_HIP(hipDeviceSynchronize());
		NGP_HIP(hipMemcpy(out, t->dist.acc.p, n * 8, hipMemcpyDeviceToHost));
	});
}

int ngp_nerf_trainer_set_distortion_training(ngp_nerf_trainer* t, const char* optimizer_json, uint32_t width, uint32_t height) {
	if (!t || !distortion_dims_ok(width, height)) return NGP_INVALID;
	NGP_TRY({
		AdamConfig c;
		if (optimizer_json) parse_optimizer_json(optimizer_json, c);
		t->dist.opt_set = optimizer_json != nullptr;
		if (optimizer_json) t->dist.opt = c;
		t->dist.def_w = width; t->dist.def_h = height;
	});
}

int ngp_nerf_trainer_set_optimize_distortion(ngp_nerf_trainer* t, int optimize) {
	if (!t) return NGP_INVALID;
	NGP_TRY({
		const bool on = optimize != 0;
		NGP_CHECK(!on || !t->dp(), DISTORTION_VS_DATA_PARALLEL);
		NGP_CHECK(!on || !t->error_sampling(), ERROR_SAMPLING_VS_DISTORTION);
		if (on == t->dist.optimize) return NGP_OK;
		// the training pass is re-captured with (or without) the input gradient; a prelaunched sampler was released under
		// the other rule (step_release_samples), and traced without the map this creates
		cameras_quiesce(t);
		if (on && !t->dist.bound()) check_rc(ngp_nerf_trainer_set_distortion_map(t, t->dist.def_w, t->dist.def_h, nullptr));
		t->dist.optimize = on;
		if (on) {
			// a window of its own unless pose refinement's or the exposures' is running: the sums start from zero either way
			if (!t->cam.optimize_extrinsics && !t->optimize_exposure) t->n_steps_since_cam_update = 0;
			NGP_HIP(hipMemset(t->dist.acc.p, 0, distortion_acc_words64(t->dist.w, t->dist.h) * 8));
		}
	});
}

int ngp_nerf_trainer_get_optimize_distortion(const ngp_nerf_trainer* t, int* optimize) {
	if (!t || !optimize) return NGP_INVALID;
	*optimize = t->dist.optimize ? 1 : 0;
	return NGP_OK;
}

int ngp_nerf_trainer_get_camera_training(const ngp_nerf_trainer* t, ngp_nerf_camera_training* out) {
	if (!t || !out) return NGP_INVALID;
	*out = t->cam;
	return NGP_OK;
}

int ngp_nerf_trainer_set_camera_training(ngp_nerf_trainer* t, const ngp_nerf_camera_training* c) {
	if (!t || !c || c->n_steps_between_cam_updates == 0 || !(c->extrinsic_learning_rate >= 0.f) || !(c->extrinsic_l2_reg >= 0.f))
		return NGP_INVALID;
	NGP_TRY({
		NGP_CHECK(!c->optimize_extrinsics || !t->dp(),
		          "camera pose refinement is single-GPU: the per-image gradient sums of a data-parallel trainer would need "
		          "their own all-reduce");
		NGP_CHECK(!c->optimize_extrinsics || !t->error_sampling(), ERROR_SAMPLING_VS_EXTRINSICS);
		const bool toggled = (c->optimize_extrinsics != 0) != (t->cam.optimize_extrinsics != 0);
		if (toggled) {
			// the training pass is re-captured with (or without) the input gradient; a prelaunched sampler was
			// released under the other rule (step_release_samples)
			cameras_quiesce(t);
			t->n_steps_since_cam_update = 0;
		}
		t->cam = *c;
	});
}

// ---- per-image exposure ------------------------------------------------------------------------------------------
// The optimisers' variables to the device array the loss pass reads, on `s`; binds the array once a variable is not
// zero (with the switch off and every exposure zero the loss pass runs without it)
void ngp_nerf_trainer::upload_exposures(hipStream_t s) {
	const uint32_t n = (uint32_t)cams.size();
	expo_host.resize((size_t)3 * n);
	bool any = false;
	for (uint32_t i = 0; i < n; ++i) {
		ngp_adam_state e;
		check_rc(ngp_exposure_optimizer_get(expo, i, &e));
		for (int k = 0; k < 3; ++k) { expo_host[(size_t)3 * i + k] = e.variable[k]; any = any || e.variable[k] != 0.0f; }
	}
	expo_bound = any || optimize_exposure;
	if (!expo_bound) return;
	NGP_HIP(hipMemcpyAsync(expo_dev.get<float>((size_t)3 * n), expo_host.data(), expo_host.size() * sizeof(float), hipMemcpyHostToDevice, s));
}
// the exposures are about to change outside a step: no loss pass may still read the old ones (the sampler reads none,
// so a prelaunched one stays)
static void exposures_changed(ngp_nerf_trainer* t) {
	NGP_HIP(hipDeviceSynchronize());
	t->upload_exposures(nullptr);
	NGP_HIP(hipDeviceSynchronize());
}

int ngp_nerf_trainer_set_exposure_training(ngp_nerf_trainer* t, int optimize_exposure, float exposure_l2_reg) {
	if (!t || !(exposure_l2_reg >= 0.0f) || std::isinf(exposure_l2_reg)) return NGP_INVALID;
	NGP_TRY({
		NGP_CHECK(!optimize_exposure || !t->dp(), EXPOSURE_VS_DATA_PARALLEL);
		NGP_CHECK(!optimize_exposure || !t->sample_image_by_error, IMAGE_SAMPLING_VS_EXPOSURE);
		const bool on = optimize_exposure != 0;
		t->exposure_l2_reg = exposure_l2_reg;
		if (on == t->optimize_exposure) return NGP_OK;
		t->optimize_exposure = on;
		exposures_changed(t);  // binds (or, with every exposure zero, unbinds) the device array
		if (on) {
			// a window of its own unless pose refinement's is running: the sums start from zero either way
			if (!t->cam.optimize_extrinsics) t->n_steps_since_cam_update = 0;
			const size_t n = (size_t)3 * t->cams.size();
			NGP_HIP(hipMemset(t->expo_grad.get<float>(n), 0, n * sizeof(float)));
		}
	});
}
int ngp_nerf_trainer_get_exposure_training(const ngp_nerf_trainer* t, int* optimize_exposure, float* exposure_l2_reg) {
	if (!t) return NGP_INVALID;
	if (optimize_exposure) *optimize_exposure = t->optimize_exposure ? 1 : 0;
	if (exposure_l2_reg) *exposure_l2_reg = t->exposure_l2_reg;
	return NGP_OK;
}
int ngp_nerf_trainer_camera_exposure(const ngp_nerf_trainer* t, uint32_t i, float* out) {
	if (!t || !out || i >= t->cams.size()) return NGP_INVALID;
	ngp_adam_state e;
	const int rc = ngp_exposure_optimizer_get(t->expo, i, &e);
	if (rc == NGP_OK) memcpy(out, e.variable, 12);
	return rc;
}
int ngp_nerf_trainer_set_camera_exposure(ngp_nerf_trainer* t, uint32_t i, const float* rgb) {
	if (!t || !rgb || i >= t->cams.size()) return NGP_INVALID;
	for (int k = 0; k < 3; ++k)
		if (!std::isfinite(rgb[k])) return NGP_INVALID;
	NGP_TRY({
		check_rc(ngp_exposure_optimizer_reset_one(t->expo, i));
		ngp_adam_state e;
		check_rc(ngp_exposure_optimizer_get(t->expo, i, &e));
		memcpy(e.variable, rgb, 12);
		check_rc(ngp_exposure_optimizer_set_state(t->expo, i, &e));
		exposures_changed(t);
	});
}
int ngp_nerf_trainer_exposure_optimizer_state(const ngp_nerf_trainer* t, uint32_t i, ngp_adam_state* out) {
	if (!t || !out || i >= t->cams.size()) return NGP_INVALID;
	return ngp_exposure_optimizer_get(t->expo, i, out);
}

int ngp_nerf_trainer_camera_extrinsics(const ngp_nerf_trainer* t, uint32_t i, float* out) {
	if (!t || !out || i >= t->cams.size()) return NGP_INVALID;
	NGP_TRY(t->refined_xform(i, out));
}

int ngp_nerf_trainer_set_camera_extrinsics(ngp_nerf_trainer* t, uint32_t i, const float* xform) {
	if (!t || !xform || i >= t->cams.size()) return NGP_INVALID;
	NGP_TRY({
		cameras_quiesce(t);
		memcpy(&t->xforms[(size_t)12 * i], xform, 48);
		check_rc(ngp_pose_optimizer_reset_one(t->pose, i));
		check_rc(ngp_exposure_optimizer_reset_one(t->expo, i));  // cam_exposure[frame_idx].reset_state() (:2913)
		t->rebuild_cameras(nullptr);
		exposures_changed(t);
	});
}

int ngp_nerf_trainer_reset_camera_extrinsics(ngp_nerf_trainer* t) {
	if (!t) return NGP_INVALID;
	NGP_TRY({
		cameras_quiesce(t);
		check_rc(ngp_pose_optimizer_reset(t->pose));
		check_rc(ngp_exposure_optimizer_reset(t->expo));  // :2930-2932
		t->n_steps_since_cam_update = 0;
		t->rebuild_cameras(nullptr);
		exposures_changed(t);
	});
}

int ngp_nerf_trainer_last_samples(const ngp_nerf_trainer* t, ngp_rng* rng, uint32_t* n_rays, uint32_t* max_samples,
                                  const uint32_t** ray_indices, const float** rays, const uint32_t** counters) {
	if (!t || !t->last_ray_indices || t->world != 1) return NGP_INVALID;
	if (rng) *rng = t->last_rng;
	if (n_rays) *n_rays = t->last_n_rays;
	if (max_samples) *max_samples = t->last_max_samples;
	if (ray_indices) *ray_indices = t->last_ray_indices;
	if (rays) *rays = t->last_rays;
	if (counters) *counters = t->last_counters;
	return NGP_OK;
}

int ngp_nerf_trainer_pose_optimizer_state(const ngp_nerf_trainer* t, uint32_t i, ngp_adam_state* pos, ngp_adam_state* rot) {
	if (!t || i >= t->cams.size()) return NGP_INVALID;
	return ngp_pose_optimizer_get(t->pose, i, pos, rot);
}

int ngp_nerf_trainer_set_data_parallel(ngp_nerf_trainer* t, uint32_t rank, uint32_t world, ngp_allreduce_fn allreduce, void* user) {
	if (!t || world == 0 || rank >= world || (world > 1 && !allreduce)) return NGP_INVALID;
	if (allreduce && t->cam.optimize_extrinsics) {
		set_last_error("camera pose refinement is single-GPU: turn optimize_extrinsics off before setting an exchange hook");
		return NGP_ERROR;
	}
	if (allreduce && t->optimize_exposure) {
		set_last_error("exposure optimisation is single-GPU: turn optimize_exposure off before setting an exchange hook");
		return NGP_ERROR;
	}
	if (allreduce && t->env.train) {
		set_last_error(TRAIN_ENVMAP_VS_DATA_PARALLEL);
		return NGP_ERROR;
	}
	if (allreduce && t->dist.optimize) {
		set_last_error(DISTORTION_VS_DATA_PARALLEL);
		return NGP_ERROR;
	}
	t->drain();
	// the sample-set choice (ngp_nerf_trainer::early) depends on the exchange: the last step's passes finish first
	if (hipDeviceSynchronize() != hipSuccess) return NGP_ERROR;
	t->rank = rank;
	t->world = world;
	t->allreduce = allreduce;
	t->allreduce_user = user;
	// an RCCL hook is stream-ordered and graph-capturable; a host callback (gloo) is not
	t->dp_capturable = allreduce == ngp_dp_comm_allreduce;
	if (t->dp_capturable && user && ngp_dp_comm_reserve((ngp_dp_comm*)user, ngp_model_n_params(t->model)) != NGP_OK) return NGP_ERROR;
	// the trainer's exchange with this rank: large tables shard the optimizer (reduce-scatter, slice update,
	// all-gather of the weights; trainer option shard_opt)
	const int rc = ngp_trainer_set_data_parallel(t->trainer, allreduce ? rank : 0, allreduce ? world : 1, allreduce, user);
	if (rc != NGP_OK) return rc;
	if (t->train_graph) ngp_graph_destroy(t->train_graph);  // re-captured with (or without) the exchange
	t->train_graph = nullptr;
	return NGP_OK;
}

int ngp_nerf_trainer_buffers_read(const ngp_nerf_trainer* t, const float** grid, const uint8_t** bitfield, const float** mean) {
	if (!t) return NGP_INVALID;
	if (grid) *grid = (const float*)t->grid.p;
	if (bitfield) *bitfield = (const uint8_t*)t->bitfield.p;
	if (mean) *mean = (const float*)t->mean.p;
	return NGP_OK;
}

int ngp_nerf_trainer_buffers(ngp_nerf_trainer* t, float** grid, uint8_t** bitfield, float** mean) {
	if (!t) return NGP_INVALID;
	// the caller may write these: a prelaunched sampler (pipelining) read the bitfield before any such
	// write, so discard it and let the next step sample serially after the caller's writes
	t->drain();
	if (grid) *grid = (float*)t->grid.p;
	if (bitfield) *bitfield = (uint8_t*)t->bitfield.p;
	if (mean) *mean = (float*)t->mean.p;
	return NGP_OK;
}


// update_density_grid_nerf (testbed_nerf.cu:3412-3536), in two parts: the samples (generation and, on one GPU, the
// sort by cell bin: they read only the grid and the grid rng), then their density, splat, EMA, mean and bitfield.
// One GPU: the samples sorted by cell bin before the density evaluation, and the splat from the sorted order, which
// writes every cell. Data parallel: the order within a bin is not deterministic, so the ranks' shards of it would not
// partition the samples; there each rank evaluates its shard of the generated order and splats it by the binned
// counting sort (every cell too). A/B knob NGP_SPLAT_SORT=0: memset, generated order, atomics.
static void grid_update_samples(ngp_nerf_trainer* t, hipStream_t s, uint32_t n_uniform, uint32_t n_nonuniform) {
	const ngp_nerf_config& cfg = t->cfg;
	const uint32_t n_cascades = cfg.max_cascade + 1;
	const uint32_t n_el = GRID_N_CELLS * n_cascades;
	const uint32_t n = n_uniform + n_nonuniform;
	const float* grid = (const float*)t->grid.p;
	// every rank generates the same sample set (same density rng); each evaluates its 1/N shard
	float* pos = t->gpos.get<float>((size_t)n * 3);
	uint32_t* idx = t->gidx.get<uint32_t>(n);
	uint32_t* mask = t->grid_mask.get<uint32_t>(grid_mask_words(n_cascades));
	grid_generate_samples(n_uniform, t->grid_rng.dev(), t->ema_step, cfg, grid, n_cascades, -0.01f, pos, idx, mask, s);
	t->grid_rng.advance();
	grid_generate_samples(n_nonuniform, t->grid_rng.dev(), t->ema_step, cfg, grid, n_cascades, MIN_OPTICAL_THICKNESS,
	                      pos + (size_t)n_uniform * 3, idx + n_uniform, mask, s);
	t->grid_rng.advance();
	if (t->knobs.splat_sort != 0 && t->world == 1)
		grid_sort_samples(n, pos, idx, n_el, t->splat_scratch.get<uint32_t>(grid_sort_scratch_u32(n, n_el)),
		                  t->gpos_sorted.get<float>((size_t)n * 4), s);
}
static void grid_update_finish(ngp_nerf_trainer* t, hipStream_t s, float decay, uint32_t n_uniform, uint32_t n_nonuniform) {
	const ngp_nerf_config& cfg = t->cfg;
	const uint32_t n_cascades = cfg.max_cascade + 1;
	const uint32_t n_el = GRID_N_CELLS * n_cascades;
	const uint32_t n = n_uniform + n_nonuniform;
	float* grid = (float*)t->grid.p;
	float* tmp = t->grid_tmp.get<float>(n_el);
	const int splat_sort = t->knobs.splat_sort;
	const bool sorted = splat_sort != 0 && t->world == 1, binned = splat_sort != 0 && t->world > 1;
	if (splat_sort == 0) NGP_HIP(hipMemsetAsync(tmp, 0, (size_t)n_el * 4, s));
	const uint32_t* idx = t->gidx.get<uint32_t>(n);
	const uint32_t lo = (uint32_t)((uint64_t)n * t->rank / t->world), hi = (uint32_t)((uint64_t)n * (t->rank + 1) / t->world);
	const uint32_t ns = hi - lo;
	f16* dens = t->gdens.get<f16>((size_t)std::max(ns, 1u) * 16);
	const float* dpos = sorted ? t->gpos_sorted.get<float>((size_t)n * 4) : t->gpos.get<float>((size_t)n * 3);
	const uint32_t dstride = sorted ? 4 : 3;
	if (ns) {
		// row 0 (raw density) only: the other 15 rows of the density network's output are not read
		check_rc(ngp::density_impl(t->model, s, ns, dpos + (size_t)lo * dstride, dstride, dens, ns, ngp::DENSITY_LAYOUT_ROW0, 0));
		if (splat_sort == 0) grid_splat_max(ns, idx + lo, dens, cfg.density_activation, tmp, s);
	}
	if (sorted)
		grid_splat_sorted(n_el, t->splat_scratch.get<uint32_t>(grid_sort_scratch_u32(n, n_el)), dpos, dens, lo, hi,
		                  cfg.density_activation, tmp, s);
	if (binned)
		grid_splat_max_binned(ns, idx + lo, dens, cfg.density_activation, tmp, n_el,
		                      t->splat_scratch.get<uint32_t>(grid_splat_scratch_u32(ns, n_el)), s);
	if (t->world > 1) {
		// splatted maxima of all shards (values are >= 0: float max == max of the shards' atomicMax)
		NGP_CHECK(t->allreduce(t->allreduce_user, tmp, n_el, NGP_DTYPE_F32, NGP_REDUCE_MAX, s) == 0,
		          "data parallel: density-grid all-reduce failed");
	}
	if (t->knobs.grid_final_fused) {  // A/B knob
		grid_ema_mean_bitfield(n_el, decay, grid, tmp, cfg.max_cascade, (float*)t->mean.p, (uint8_t*)t->bitfield.p, s);
	} else {
		grid_ema(n_el, decay, grid, tmp, s);
		grid_mean_bitfield(grid, cfg.max_cascade, (float*)t->mean.p, (uint8_t*)t->bitfield.p, s);
	}
	++t->ema_step;
}
static void update_density_grid(ngp_nerf_trainer* t, hipStream_t s, float decay, uint32_t n_uniform, uint32_t n_nonuniform) {
	if (t->training_step == 0) {
		t->ema_step = 0;
		const Dataset& ds = t->data->ds;
		const uint32_t n_el = GRID_N_CELLS * (t->cfg.max_cascade + 1);
		k_mark_untrained<<<div_round_up(n_el, 128), 128, 0, s>>>(n_el, (float*)t->grid.p, ds.n_images, t->d_cams, t->d_raw, true);
		NGP_HIP(hipGetLastError());
	}
	grid_update_samples(t, s, n_uniform, n_nonuniform);
	grid_update_finish(t, s, decay, n_uniform, n_nonuniform);
}
// the update's sample counts at a step (training_prep_nerf, testbed_nerf.cu:3622-3630)
static void grid_update_counts(const ngp_nerf_trainer* t, uint32_t step, uint32_t* nu, uint32_t* nn) {
	const uint32_t nc = t->cfg.max_cascade + 1;
	*nu = step < 256 ? GRID_N_CELLS * nc : GRID_N_CELLS / 4 * nc;
	*nn = step < 256 ? 0u : GRID_N_CELLS / 4 * nc;
}

// Data parallel: this shard's counters and loss as five floats for one all-reduce (sum). The u32
// counters travel as 16-bit halves so their sums stay exact in fp32 for up to 256 ranks; the per-ray
// losses are normalised by the shard's ray count (compute_loss), rescaled here to 1 / R_global.
__global__ void k_dp_pack(const uint32_t* __restrict__ ctr, const float* __restrict__ loss, uint32_t n_loss, float loss_rescale,
                          float* __restrict__ out) {
	__shared__ float part[16];
	float sum = 0.f;
	for (uint32_t i = threadIdx.x; i < n_loss; i += blockDim.x) sum += loss[i];
	for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o);
	if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = sum;
	__syncthreads();
	if (threadIdx.x == 0) {
		float t = 0.f;
		for (uint32_t w = 0; w < blockDim.x / 64; ++w) t += part[w];
		out[0] = (float)(ctr[1] >> 16); out[1] = (float)(ctr[1] & 0xffffu);
		out[2] = (float)(ctr[2] >> 16); out[3] = (float)(ctr[2] & 0xffffu);
		out[4] = t * loss_rescale;
	}
}
// the all-reduced counters -> host-coherent memory (host[1] steps, host[2] compacted, host[5] loss bits;
// host[6] this shard's own step count, which sizes its next inference)
__global__ void k_dp_publish(const float* __restrict__ red, const uint32_t* __restrict__ ctr, volatile uint32_t* host, uint32_t seq) {
	if (threadIdx.x == 0) {
		host[6] = ctr[1];
		host[1] = ((uint32_t)red[0] << 16) + (uint32_t)red[1];
		host[2] = ((uint32_t)red[2] << 16) + (uint32_t)red[3];
		host[5] = __float_as_uint(red[4]);
		__threadfence_system();
		host[4] = seq;
	}
}

// Wait until the step's counters are published (k_rollover_pair_publish, or k_dp_publish; or the stream failed /
// stalled for a minute).
static void wait_published(volatile uint32_t* host, uint32_t seq, hipStream_t s) {
	const auto t0 = std::chrono::steady_clock::now();
	for (uint64_t spin = 0;; ++spin) {
		if (__atomic_load_n(&host[4], __ATOMIC_ACQUIRE) == seq) return;
		if ((spin & 1023) == 1023) {
			const hipError_t q = hipStreamQuery(s);
			if (q != hipSuccess && q != hipErrorNotReady) NGP_HIP(q);
			if (q == hipSuccess) {  // the stream drained: the publishing kernel ran, so its write is visible
				if (__atomic_load_n(&host[4], __ATOMIC_ACQUIRE) == seq) return;
				const hipError_t e = hipGetLastError();
				throw Error(std::string("nerf train step: stream idle but counters not published (") + hipGetErrorString(e) + ")");
			}
			NGP_CHECK(std::chrono::steady_clock::now() - t0 < std::chrono::seconds(60), "nerf train step: counters not published");
		}
		__builtin_ia32_pause();
	}
}

// Sizes and buffers of one step's sampling (train_nerf_step, testbed_nerf.cu:3867-3953), from the
// trainer's current rays-per-batch and measured counts.
struct SamplePlan {
	uint32_t R, Rl, r_lo, Bl, max_samples, max_inference, Ra;
	uint32_t* ray_indices;
	float* rays;
	uint32_t* numsteps;
	float* coords;
	uint32_t* ctr;
};
static SamplePlan sample_plan(ngp_nerf_trainer* t) {
	SamplePlan p;
	const uint32_t B = t->cfg.target_batch_size, W = t->world, rk = t->rank;
	p.R = t->rays_per_batch;
	p.r_lo = (uint32_t)((uint64_t)p.R * rk / W);
	p.Rl = (uint32_t)((uint64_t)p.R * (rk + 1) / W) - p.r_lo;
	p.Bl = (uint32_t)((uint64_t)B * (rk + 1) / W - (uint64_t)B * rk / W);
	p.max_samples = p.Bl * 16;
	if (t->measured_before_compaction_local == 0) p.max_inference = p.max_samples;
	else p.max_inference = next_multiple(std::min(t->measured_before_compaction_local, p.max_samples), 256);
	p.Ra = std::max(p.Rl, 1u);
	auto& set = t->sets[t->two_sets() && (t->training_step & 1u)];  // the step's sample set (ngp_nerf_trainer::two_sets)
	p.ray_indices = set.ray_indices.get<uint32_t>(p.Ra);
	p.rays = set.rays.get<float>((size_t)p.Ra * 6);
	p.numsteps = set.numsteps.get<uint32_t>((size_t)p.Ra * 2);
	p.coords = set.coords.get<float>((size_t)p.max_samples * 7);
	p.ctr = set.counters.get<uint32_t>(4);  // rays kept, steps, compacted steps
	return p;
}
static void launch_sampler(ngp_nerf_trainer* t, const SamplePlan& p, hipStream_t s) {
	ProfScope ps("nerf_sample", s);
	SampleArgs a{};
	a.n_rays = p.Rl; a.ray_offset = p.r_lo; a.n_rays_total_for_image_idx = p.R; a.cdfs = t->sampling_cdfs();
	a.max_samples = p.max_inference; a.rng = t->rng.dev(); a.bitfield = (const uint8_t*)t->bitfield.p;
	a.ray_indices = p.ray_indices; a.rays = p.rays; a.numsteps = p.numsteps; a.coords = p.coords; a.counters = p.ctr;
	const DistMap dm = t->dist.view();  // a bound map is always traced through, whether it is being optimised or not
	check_rc(run_sampler(t->data, &t->cfg, s, a, t->d_cams, dm.data ? &dm : nullptr));
}
static bool density_grid_update_due(uint32_t step) {
	const uint32_t skip = std::min(std::max(step / 16u, 1u), 16u);
	return step % skip == 0;
}

// Testbed::train_nerf's error map window (testbed_nerf.cu:3659-3666): at its first step the map is
// resized to min(3.5 (n_steps_between * rays_per_batch / n_images)^(1/4), image 0's size) per image and
// zeroed (uint32 arithmetic as in the reference). Returns the map the step's loss pass deposits into.
static float* error_map_window(ngp_nerf_trainer* t, hipStream_t s) {
	const Dataset& ds = t->data->ds;
	if (ds.n_images == 0 || ds.cams.empty()) return nullptr;
	if (t->em_steps_since == 0) {
		const uint32_t n_samples_per_image = (t->em_steps_between * t->rays_per_batch) / ds.n_images;
		const int k = (int)(std::sqrt(std::sqrt((float)n_samples_per_image)) * 3.5f);
		t->em_w = (uint32_t)std::min(k, (int)ds.cams[0].width);
		t->em_h = (uint32_t)std::min(k, (int)ds.cams[0].height);
		const size_t n = (size_t)t->em_w * t->em_h * ds.n_images;
		NGP_HIP(hipMemsetAsync(t->em_data.get<float>(std::max<size_t>(n, 1)), 0, n * sizeof(float), s));
	}
	return t->em_w >= 2 && t->em_h >= 2 ? (float*)t->em_data.p : nullptr;
}

// After the step (testbed_nerf.cu:3700-3748): when the window is full, the CDFs of the map
// (construct_cdf_2d/1d on the stream; with data parallelism the ranks' maps are summed first), the
// host pass over the per-image totals, then a 1.5x longer window.
// Returns whether it rebuilt the CDFs.
static bool error_map_step_done(ngp_nerf_trainer* t, hipStream_t s) {
	const Dataset& ds = t->data->ds;
	if (ds.n_images == 0 || ds.cams.empty()) return false;
	t->em_steps_since += 1;
	if (t->em_steps_since < t->em_steps_between) return false;
	t->em_cdf_w = t->em_w;
	t->em_cdf_h = t->em_h;
	const uint32_t n_img = ds.n_images, w = t->em_cdf_w, h = t->em_cdf_h;
	float* data = (float*)t->em_data.p;
	if (t->dp() && data && w && h)
		NGP_CHECK(t->allreduce(t->allreduce_user, data, (uint64_t)w * h * n_img, NGP_DTYPE_F32, NGP_REDUCE_SUM, s) == 0,
		          "data parallel: error map all-reduce failed");
	float* cdf_x = t->em_cdf_x.get<float>(std::max<size_t>((size_t)w * h * n_img, 1));
	float* cdf_y = t->em_cdf_y.get<float>(std::max<size_t>((size_t)h * n_img, 1));
	float* cdf_img = t->em_cdf_img.get<float>(n_img);
	error_map_cdfs(n_img, w, h, data, cdf_x, cdf_y, cdf_img, s);
	// the image CDF on the host (single-threaded in the reference too)
	std::vector<float> pmf(n_img), cdf(n_img);
	NGP_HIP(hipMemcpyAsync(pmf.data(), cdf_img, n_img * sizeof(float), hipMemcpyDeviceToHost, s));
	NGP_HIP(hipStreamSynchronize(s));
	float cum = 0.f;
	for (uint32_t i = 0; i < n_img; ++i) cdf[i] = cum += pmf[i];
	const float norm = 1.0f / cum;
	constexpr float MIN_PMF = 0.1f;
	for (uint32_t i = 0; i < n_img; ++i) {
		pmf[i] = (1.0f - MIN_PMF) * pmf[i] * norm + MIN_PMF / (float)n_img;
		cdf[i] = (1.0f - MIN_PMF) * cdf[i] * norm + MIN_PMF * (float)(i + 1) / (float)n_img;
	}
	NGP_HIP(hipMemcpyAsync(cdf_img, cdf.data(), n_img * sizeof(float), hipMemcpyHostToDevice, s));
	NGP_HIP(hipStreamSynchronize(s));
	t->em_pmf_img = std::move(pmf);
	t->em_steps_since = 0;
	t->em_cdf_valid = true;
	t->em_steps_between = (uint32_t)(t->em_steps_between * 1.5f);
	return true;
}

int ngp_nerf_trainer_error_map(ngp_nerf_trainer* t, int which, float* out, uint64_t cap, ngp_nerf_error_map_info* info) {
	if (!t || which < 0 || which > 4) return NGP_INVALID;
	NGP_TRY({
		const uint32_t n_img = t->data->ds.n_images;
		const uint64_t sizes[5] = {(uint64_t)t->em_w * t->em_h * n_img, (uint64_t)t->em_cdf_w * t->em_cdf_h * n_img,
		                           (uint64_t)t->em_cdf_h * n_img, t->em_cdf_valid ? n_img : 0u, t->em_pmf_img.size()};
		const void* src[5] = {t->em_data.p, t->em_cdf_x.p, t->em_cdf_y.p, t->em_cdf_img.p, t->em_pmf_img.data()};
		if (info) {
			info->width = t->em_w; info->height = t->em_h;
			info->cdf_width = t->em_cdf_w; info->cdf_height = t->em_cdf_h;
			info->n_images = n_img;
			info->cdf_valid = t->em_cdf_valid ? 1u : 0u;
			info->n_steps_since_update = t->em_steps_since;
			info->n_steps_between_updates = t->em_steps_between;
			info->size = sizes[which];
		}
		const uint64_t n = std::min(cap, sizes[which]);
		if (out && n) {
			if (which == 4) {
				memcpy(out, src[4], n * sizeof(float));
			} else {
				NGP_HIP(hipDeviceSynchronize());
				NGP_HIP(hipMemcpy(out, src[which], n * sizeof(float), hipMemcpyDeviceToHost));
			}
		}
	});
}

int ngp_nerf_trainer_set_pipeline(ngp_nerf_trainer* t, int enable) {
	if (!t) return NGP_INVALID;
	NGP_TRY({
		t->drain();
		t->pipeline = enable != 0;
	});
}

// The trainer's streams. Experiment knobs (A/B): NGP_SAMPLER_PRIO / NGP_MAIN_PRIO -1 low,
// 1 high (HSA queue priority: which queue's workgroups the dispatcher places first); NGP_SAMPLER_CU_KEEP k in 1..7:
// the sampler's queue may use k of every 8 CUs (CU mask), so the training pass's one-block-per-CU MLP kernel
// finds whole CUs free on the rest.
static int stream_prio(int knob) {
	if (!knob) return 0;
	int least = 0, greatest = 0;
	NGP_HIP(hipDeviceGetStreamPriorityRange(&least, &greatest));
	return knob < 0 ? least : greatest;  // lower number = higher priority
}
static hipStream_t make_sampler_stream(const NerfKnobs& knobs) {
	hipStream_t s = nullptr;
	const int k = knobs.sampler_cu_keep;
	if (k > 0 && k < 8) {
		int dev = 0, n_cu = 0;
		NGP_HIP(hipGetDevice(&dev));
		NGP_HIP(hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, dev));
		std::vector<uint32_t> mask((n_cu + 31) / 32, 0u);
		for (int c = 0; c < n_cu; ++c)
			if (c % 8 < k) mask[c / 32] |= 1u << (c % 32);
		NGP_HIP(hipExtStreamCreateWithCUMask(&s, (uint32_t)mask.size(), mask.data()));
		return s;
	}
	const int prio = stream_prio(knobs.sampler_prio);
	if (prio) NGP_HIP(hipStreamCreateWithPriority(&s, hipStreamNonBlocking, prio));
	else NGP_HIP(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
	return s;
}
// the step's stream: the caller's, or a private blocking one (ordered after the null stream's earlier work)
static hipStream_t step_stream(ngp_nerf_trainer* t, void* stream) {
	if (stream) return S(stream);
	if (!t->own_stream) {
		const int prio = stream_prio(t->knobs.main_prio);
		if (prio) NGP_HIP(hipStreamCreateWithPriority(&t->own_stream, hipStreamDefault, prio));
		else NGP_HIP(hipStreamCreate(&t->own_stream));
	}
	return t->own_stream;
}

// ---- the stages of ngp_nerf_train_step, in the order they run ---------------------------------------------------
// What the stages of one step share: its sampling plan, its workspaces and its mode.
struct Step {
	bool pre = false;       // the sampler was launched under the last step's training pass
	bool get_loss = false;
	SamplePlan sp;
	f16 *mlp_out = nullptr, *dloss = nullptr;
	float *coords_c = nullptr, *loss = nullptr;
	ngp_rng rng;            // the step's rays (the training pass advances the trainer's)
	bool dp = false;
	bool early_pub = false;     // the loss's scan publishes the counters (ngp_nerf_trainer::early)
	bool can_pipeline = false;  // the next step's sampler may run under this step's training pass: the exchange is
	                            // stream-ordered (single GPU, or the engine's RCCL communicator)
	bool cam = false;           // camera pose refinement: the training pass also writes dL/dinput
	float* dinput = nullptr;    // [Bl x 7]
	bool dist = false;          // optimize_distortion: likewise, for the map's gradient
	bool cam_updated = false;   // this step ended with a pose or distortion map update (step_camera_update)
	bool expo = false;          // optimize_exposure: the loss pass also takes the rays' exposure gradients
	const float* expo_ray_grad = nullptr;  // ... kept here for step_exposure_gradients
	bool expo_due = false;      // an exposure-only update is due at the end of this step (step_exposure_update)
	bool em_closed = false;     // this step closed an error map window: the CDFs were rebuilt (error_map_step_done)
};

// training_prep_nerf (a prelaunched sampler implies no update was due at this step)
static void step_density_grid(ngp_nerf_trainer* t, hipStream_t s, const Step& c) {
	if (c.pre || !density_grid_update_due(t->training_step)) return;
	{
		ProfScope ps("nerf_density_grid", s);
		uint32_t nu, nn;
		grid_update_counts(t, t->training_step, &nu, &nn);
		if (t->grid_pregen) {  // the samples were generated (and sorted) under the last step's training pass
			NGP_CHECK(nu == t->pregen_nu && nn == t->pregen_nn, "nerf: pregenerated density-grid samples are stale");
			t->grid_pregen = false;
			t->pregenerated.wait(s);
			grid_update_finish(t, s, 0.95f, nu, nn);
		} else {
			update_density_grid(t, s, 0.95f, nu, nn);
		}
	}
	t->grid_updated.signal(s);
}

// train_nerf_step's sizes and workspaces (testbed_nerf.cu:3867-3953)
static void step_plan(ngp_nerf_trainer* t, Step& c) {
	c.sp = sample_plan(t);
	const SamplePlan& sp = c.sp;
	if (t->training_step == 0) t->n_rays_total = 0;
	t->n_rays_total += sp.R;
	c.mlp_out = t->mlp_out.get<f16>((size_t)std::max(sp.Bl, sp.max_samples) * 16);
	c.dloss = t->dloss.get<f16>((size_t)sp.Bl * 16);
	c.coords_c = t->coords_c.get<float>((size_t)sp.Bl * 7);
	c.loss = t->loss.get<float>(sp.Ra);
	c.rng = ngp_rng{t->rng.state, t->rng.inc};
	c.dp = t->dp();
	c.early_pub = t->early() && sp.Rl > 0;
	c.can_pipeline = t->pipeline && (!c.dp || t->dp_capturable);
	c.cam = t->cam.optimize_extrinsics != 0;
	c.expo = t->optimize_exposure && sp.Rl > 0;
	t->last_rng = c.rng; t->last_n_rays = sp.R; t->last_max_samples = sp.max_inference;
	t->last_ray_indices = sp.ray_indices; t->last_rays = sp.rays; t->last_counters = sp.ctr;
	c.dist = t->dist.optimize && t->dist.bound() && !c.dp && sp.Rl > 0;
	c.dinput = c.cam || c.dist ? t->dinput.get<float>((size_t)sp.Bl * 7) : nullptr;
}

// The step's samples (launched here, or awaited from the prelaunch) and the network's output for every one of them.
// Global ray ids (rng.advance(i * 16), image_idx(i, R)) so the shards draw the 1-GPU rays.
static void step_sample_and_infer(ngp_nerf_trainer* t, hipStream_t s, const Step& c) {
	const SamplePlan& sp = c.sp;
	if (c.pre) {
		NGP_CHECK(sp.R == t->pre_R && sp.max_inference == t->pre_max_inference, "nerf: prelaunched sampler is stale");
		t->sampled.wait(s);
	} else {
		launch_sampler(t, sp, s);
	}
	ProfScope ps("nerf_inference", s);
	// only the 4 live outputs (raw rgb, raw density): compute_loss reads nothing else
	check_rc(ngp_inference(t->model, s, sp.max_inference, sp.coords, 7, c.mlp_out, 4, NGP_LAYOUT_AOS_RGBD, 0));
}

// Loss and compaction, rollover, and the step's counters to the host. The counters are final here (the training
// pass does not touch them): published before the training pass, the host can size the next step while it runs.
static void step_loss_and_publish(ngp_nerf_trainer* t, hipStream_t s, Step& c) {
	const SamplePlan& sp = c.sp;
	const uint32_t R = sp.R, Rl = sp.Rl, Bl = sp.Bl;
	uint32_t* ctr = sp.ctr;
	// dL/doutput is scaled by 128 / R (global), so the shards' summed gradient is the 1-GPU gradient
	const float loss_scale_local = 128.0f * (float)Rl / (float)R;
	float* error_map = error_map_window(t, s);
	if (!t->host_ctr) {
		void* p = nullptr;
		NGP_HIP(hipHostMalloc(&p, 64, hipHostMallocCoherent | hipHostMallocMapped));
		t->host_ctr = (volatile uint32_t*)p;
		memset(p, 0, 64);
	}
	const uint32_t pub_seq = c.dp ? 0u : ++t->publish_seq;
	// environment map: the raw parameters behind every ray (m_envmap.view()), and with train_envmap the gradient
	// accumulator, cleared for this step's deposit
	const ngp_nerf_trainer::Envmap& env = t->env;
	unsigned long long* env_acc = env.bound() && env.train ? (unsigned long long*)env.acc.p : nullptr;
	if (env_acc) NGP_HIP(hipMemsetAsync(env_acc, 0, envmap_acc_words64(env.w, env.h) * 8, s));
	{
		ProfScope ps("nerf_loss", s);
		// pass 1 keeps each composited sample's state for pass 2 (indexed like the sampler's samples, at most max_samples)
		// (a sixth plane, the depth prefix, with depth supervision on)
		LossArgs a{};
		a.depth_lambda = t->depth_lambda; a.depth_loss_type = t->depth_loss_type;
		const size_t planes = loss_depth_on(t->data->ds, a) ? 6 : 5;
		float* lstate = t->knobs.loss_state ? t->loss_state.get<float>(planes * sp.max_samples) : nullptr;
		a.n_rays = Rl; a.n_rays_total_for_image_idx = R; a.rng = Rng{c.rng.state, c.rng.inc};
		a.max_samples_compacted = Bl; a.ray_counter = ctr; a.network_output = c.mlp_out; a.out_stride = 4;
		a.ray_indices = sp.ray_indices; a.rays = sp.rays; a.numsteps = sp.numsteps; a.coords_in = sp.coords; a.coords_out = c.coords_c;
		a.dloss_doutput = c.dloss; a.loss = c.loss; a.compacted_counter = ctr + 2;
		a.mean_density = (const float*)t->mean.p; a.loss_scale = c.dp ? loss_scale_local : 128.0f; a.zero_loss = true;
		a.error_map = error_map; a.em_w = t->em_w; a.em_h = t->em_h;
		a.state = lstate; a.state_cap = sp.max_samples;
		a.pub_host = c.early_pub ? t->host_ctr : nullptr; a.pub_seq = pub_seq; a.cdfs = t->sampling_cdfs();
		a.envmap = env.bound() ? (const float*)env.params.p : nullptr; a.env_w = env.w; a.env_h = env.h;
		a.env_loss_type = t->envmap_loss_type(); a.env_acc = env_acc;
		// per-image exposures (bound once one is not zero, or with optimize_exposure, which also takes their gradient)
		a.exposure = t->expo_bound ? (const float*)t->expo_dev.p : nullptr;
		check_rc(run_compute_loss(t->data, &t->cfg, s, a, c.expo, &c.expo_ray_grad));
	}
	if (!c.dp) {
		// single GPU: the rollover launch (fill_rollover_and_rescale + fill_rollover) also publishes the counters
		// (early_pub: already published) and writes the optimizer control block the training graph reads (a separate
		// publish kernel and ngp_graph_launch's k_set_ctl before: two launches less per step)
		StepPublish pub{};
		pub.ctr = ctr;
		pub.host = c.early_pub ? nullptr : t->host_ctr;
		pub.seq = pub_seq;
		trainer_ctl_values(t->trainer, &pub.ctl, &pub.step, &pub.cfg_off, &pub.cfg_words, pub.cfg);
		fill_rollover_pair_publish(Bl, ctr + 2, c.dloss, 16, c.coords_c, 7, pub, s);
	} else {
		fill_rollover_pair(Bl, ctr + 2, c.dloss, 16, c.coords_c, 7, s);  // fill_rollover_and_rescale + fill_rollover
		// NerfCounters::update_after_training on the global batch: this shard's counters and loss
		// all-reduced on the stream, then published like the single-GPU counters (no copies, no sync)
		ProfScope ps("nerf_dp_counters", s);
		float* d = t->dp_scalars.get<float>(8);
		k_dp_pack<<<1, 1024, 0, s>>>(ctr, c.loss, c.get_loss ? Rl : 0u, (float)Rl / (float)R, d);
		NGP_HIP(hipGetLastError());
		NGP_CHECK(t->allreduce(t->allreduce_user, d, 5, NGP_DTYPE_F32, NGP_REDUCE_SUM, s) == 0,
		          "data parallel: counter all-reduce failed");
		k_dp_publish<<<1, 64, 0, s>>>(d, ctr, t->host_ctr, ++t->publish_seq);
	}
	NGP_HIP(hipGetLastError());
}

// optimize_exposure, device part (testbed_nerf.cu:3641-3644, 1973-1986): the rays' exposure gradients summed per image
// into the trainer's accumulators, which start from zero after every update. Before the sample buffers are released:
// the sum reads the ray indices and the compacted sample counts.
static void step_exposure_gradients(ngp_nerf_trainer* t, hipStream_t s, const Step& c) {
	if (!t->optimize_exposure) return;
	ProfScope ps("nerf_exposure_gradients", s);
	const uint32_t n_images = t->data->ds.n_images;
	float* acc = t->expo_grad.get<float>((size_t)3 * n_images);
	// a window's first step clears the sums, also when it has no ray of its own (the counter advances all the same)
	if (t->n_steps_since_cam_update == 0) NGP_HIP(hipMemsetAsync(acc, 0, (size_t)3 * n_images * sizeof(float), s));
	if (!c.expo) return;
	NGP_CHECK(c.expo_ray_grad, "nerf: the loss pass took no exposure gradient");
	const SamplePlan& sp = c.sp;
	ExposureGradArgs a{};
	a.n_rays_cap = sp.Rl; a.n_rays_total = sp.R; a.n_images = n_images;
	a.ray_counter = sp.ctr; a.ray_indices = sp.ray_indices; a.numsteps = sp.numsteps;
	a.ray_grad = c.expo_ray_grad; a.image_grad = acc;
	exposure_gradients(a, s);
}

// The sample buffers and counters are free for the next step's sampler (early(): nothing to release, that sampler
// writes the other sample set)
static void step_release_samples(ngp_nerf_trainer* t, hipStream_t s, const Step& c) {
	if (!c.can_pipeline) return;
	if (!t->sample_stream) t->sample_stream = make_sampler_stream(t->knobs);
	if (!t->two_sets()) t->released.signal(s);
}

static void step_train_pass(ngp_nerf_trainer* t, hipStream_t s, const Step& c) {
	const uint32_t Bl = c.sp.Bl;
	ProfScope ps("nerf_train_pass", s);
	StepBatch batch;
	batch.n = Bl; batch.input = c.coords_c; batch.input_stride = 7; batch.dL_doutput = c.dloss; batch.dL_stride = 16;
	batch.loss_scale = 128.0f;
	if (!c.dp || t->dp_capturable) {
		// one HIP graph per step: forward_backward [+ the gradient all-reduce, RCCL] + optimizer. Re-record
		// when the graph's buffers moved: the sample buffers, or any model workspace (a density-grid
		// update through ngp_density can grow the encoding workspace after a snapshot load)
		if (!t->train_graph || t->graph_in != c.coords_c || t->graph_dl != c.dloss || t->graph_n != Bl ||
		    t->graph_dinput != c.dinput || t->graph_epoch != ngp_model_workspace_epoch(t->model)) {
			if (t->train_graph) ngp_graph_destroy(t->train_graph);
			t->train_graph = nullptr;
			// data parallel: the shards' dL/doutput is scaled by 128 / R_global, so the summed gradient is the
			// 1-GPU gradient: world factor 1 in the optimizer
			batch.dL_dinput = c.dinput; batch.dL_dinput_stride = 7;
			check_rc(capture_training_step_with(t->trainer, s, batch, 1, 1, t->exchange(), &t->train_graph));
			t->graph_in = c.coords_c;
			t->graph_dinput = c.dinput;
			t->graph_dl = c.dloss;
			t->graph_n = Bl;
			t->graph_epoch = ngp_model_workspace_epoch(t->model);
		}
		if (c.dp) check_rc(ngp_graph_launch(t->train_graph, s));
		else graph_launch_ctl_written(t->train_graph, s);  // the control block was written by the rollover launch
	} else {
		// host-callback exchange (gloo): not capturable; the same step body, launched eagerly
		check_rc(train_step_with(t->trainer, s, batch, t->exchange()));
	}
	t->rng.advance();  // m_rng.advance() (testbed_nerf.cu:4127)
}

// train_envmap (testbed_nerf.cu:3683-3685): the loss pass's exact gradient sum to fp32, then the map's own optimizer
// step with LOSS_SCALE, eager on the step's stream after the training graph. The next step's loss pass reads the
// parameters on the same stream; the prelaunched sampler never does.
static void step_envmap_update(ngp_nerf_trainer* t, hipStream_t s, const Step& c) {
	ngp_nerf_trainer::Envmap& e = t->env;
	if (!e.bound() || !e.train || c.sp.Rl == 0) return;
	ProfScope ps("nerf_envmap_update", s);
	envmap_gradient_f32(e.w, e.h, (const unsigned long long*)e.acc.p, (float*)e.grad.p, s);
	AdamState st{};
	st.w32 = (float*)e.params.p; st.g32 = (const float*)e.grad.p;
	st.m1 = (float*)e.m1.p; st.m2 = (float*)e.m2.p; st.steps = (uint32_t*)e.steps.p;
	st.ema32 = (float*)e.ema.p; st.ema_f32 = (float*)e.ema_out.p;
	st.step_add = e.step;
	const AdamConfig& oc = t->envmap_optimizer();
	adam_ema_update_f32(oc, (uint32_t)e.n(), 128.0f, st, s);
	++e.step;
	e.ema_valid = oc.ema_decay > 0.f;
}

// Camera pose refinement, device part (testbed_nerf.cu:3641-3644, 4071-4125): the compacted batch's input gradient summed per
// image into the trainer's accumulators, which start from zero after every pose update.
// optimize_distortion (:2088-2099): pass 1's DIST form also stores every kept ray's image-plane gradient, which
// k_distortion_deposit adds into the map's exact accumulator; with the map alone pass 2 is not launched.
static void step_camera_gradients(ngp_nerf_trainer* t, hipStream_t s, const Step& c) {
	if (!c.cam && !c.dist) return;
	ProfScope ps("nerf_camera_gradients", s);
	const uint32_t n_images = t->data->ds.n_images;
	float* acc = c.cam ? t->cam_grad.get<float>((size_t)6 * n_images) : nullptr;
	if (c.cam && t->n_steps_since_cam_update == 0) NGP_HIP(hipMemsetAsync(acc, 0, (size_t)6 * n_images * sizeof(float), s));
	const SamplePlan& sp = c.sp;
	CamGradArgs a{};
	a.n_rays_cap = sp.Rl; a.n_rays_total = sp.R; a.n_images = n_images;
	a.ray_counter = sp.ctr; a.ray_indices = sp.ray_indices; a.rays = sp.rays; a.numsteps = sp.numsteps;
	a.coords = c.coords_c; a.coords_grad = c.dinput; a.grad_stride = 7;
	for (int k = 0; k < 3; ++k) { a.aabb_min[k] = t->cfg.aabb_min[k]; a.aabb_max[k] = t->cfg.aabb_max[k]; }
	a.ray_grad = t->cam_ray_grad.get<float>((size_t)sp.Ra * 6);
	a.pos_grad = acc; a.rot_grad = acc ? acc + (size_t)3 * n_images : nullptr;
	if (!c.dist) {
		camera_gradients(a, CAM_GRAD_LANES, s);
		return;
	}
	ngp_nerf_trainer::Distortion& d = t->dist;
	const size_t words = distortion_acc_words64(d.w, d.h);
	if (t->n_steps_since_cam_update == 0) NGP_HIP(hipMemsetAsync(d.acc.p, 0, words * 8, s));
	float* ray_g = d.ray_grad.get<float>((size_t)sp.Ra * 2);
	// xform_img: the camera the sampler traced the image through (the refined one)
	static_assert(sizeof(Camera) % sizeof(float) == 0 && offsetof(Camera, m) % sizeof(float) == 0, "Camera::m as a strided float array");
	const CamDistArgs da{(const float*)((const char*)t->d_cams + offsetof(Camera, m)), (uint32_t)(sizeof(Camera) / sizeof(float)), ray_g};
	camera_gradients_distortion(a, da, CAM_GRAD_LANES, c.cam, s);
	DistDepositArgs dep{};
	dep.n_rays_cap = sp.Rl; dep.n_rays_total = sp.R; dep.n_images = n_images;
	dep.snap = t->cfg.snap_to_pixel_centers != 0; dep.rng = Rng{c.rng.state, c.rng.inc}; dep.cams = t->d_cams;
	dep.ray_counter = sp.ctr; dep.ray_indices = sp.ray_indices; dep.numsteps = sp.numsteps; dep.ray_grad = ray_g;
	dep.w = d.w; dep.h = d.h; dep.acc = (unsigned long long*)d.acc.p;
	distortion_deposit_rays(dep, s);
}

// optimize_distortion's update (testbed_nerf.cu:3811-3818): safe_divide of the summed gradient by the summed weight, then
// the map's optimizer step with LOSS_SCALE * n_steps_between_cam_updates, on the step's stream: no host round trip. The
// next sampler runs behind it on the same stream (Step::cam_updated).
static void distortion_update(ngp_nerf_trainer* t, hipStream_t s, uint32_t between) {
	ngp_nerf_trainer::Distortion& d = t->dist;
	ProfScope ps("nerf_distortion_update", s);
	distortion_gradient_f32(d.w, d.h, (const unsigned long long*)d.acc.p, (float*)d.grad.p, s);
	AdamState st{};
	st.w32 = (float*)d.params.p; st.g32 = (const float*)d.grad.p;
	st.m1 = (float*)d.m1.p; st.m2 = (float*)d.m2.p; st.steps = (uint32_t*)d.steps.p;
	st.ema32 = (float*)d.ema.p; st.ema_f32 = (float*)d.ema_out.p;
	st.step_add = d.step;
	const AdamConfig& oc = t->distortion_optimizer();
	adam_ema_update_f32(oc, (uint32_t)d.n(), 128.0f * (float)between, st, s);
	++d.step;
	d.ema_valid = oc.ema_decay > 0.f;
}

// Camera pose refinement, host part (testbed_nerf.cu:3754-3809): every n_steps_between_cam_updates steps the sums come
// back, every camera's optimisers step and the cameras are rebuilt and uploaded before any later sampler is launched.
// optimize_exposure shares the counter and the update (:3831-3858): its sums come back, every image's optimiser steps
// with the network optimiser's learning rate, the mean is removed and the exposures are uploaded on the step's stream,
// where the next loss pass reads them. The sampler reads none of it: an exposure-only update keeps the prelaunch, and
// its round trip is put off until the next sampler is under way (step_exposure_update); with pose refinement on as
// well, which has to wait for the stream before the sampler anyway, both sums come back behind one synchronisation.
static void exposure_update_host(ngp_nerf_trainer* t, hipStream_t s, const std::vector<float>& g, uint32_t between) {
	check_rc(ngp_exposure_optimizer_step(t->expo, g.data(), between, t->exposure_l2_reg, ngp_trainer_learning_rate(t->trainer)));
	t->upload_exposures(s);
}
static void step_camera_update(ngp_nerf_trainer* t, hipStream_t s, Step& c) {
	const bool expo = t->optimize_exposure;  // also on a step without rays, as the counter is
	if (!c.cam && !expo && !c.dist) return;
	const uint32_t between = std::max(t->cam.n_steps_between_cam_updates, 1u);
	if (++t->n_steps_since_cam_update < between) return;
	t->n_steps_since_cam_update = 0;
	if (c.dist) {
		distortion_update(t, s, between);
		c.cam_updated = true;
	}
	if (!c.cam) { c.expo_due = expo; return; }
	const uint32_t n_images = t->data->ds.n_images;
	std::vector<float> g((size_t)6 * n_images), ge(expo ? (size_t)3 * n_images : 0);
	NGP_HIP(hipMemcpyAsync(g.data(), t->cam_grad.p, g.size() * sizeof(float), hipMemcpyDeviceToHost, s));
	if (expo) NGP_HIP(hipMemcpyAsync(ge.data(), t->expo_grad.get<float>(ge.size()), ge.size() * sizeof(float), hipMemcpyDeviceToHost, s));
	NGP_HIP(hipStreamSynchronize(s));
	check_rc(ngp_pose_optimizer_step(t->pose, g.data(), g.data() + (size_t)3 * n_images, between, t->cam.extrinsic_learning_rate,
	                                 t->cam.extrinsic_l2_reg, ngp_trainer_learning_rate(t->trainer)));
	t->rebuild_cameras(s);
	c.cam_updated = true;
	if (expo) exposure_update_host(t, s, ge, between);
}
// the exposure-only update's round trip, after the next step's sampler (and density-grid samples) have been launched
static void step_exposure_update(ngp_nerf_trainer* t, hipStream_t s, const Step& c) {
	if (!c.expo_due) return;
	std::vector<float> g((size_t)3 * t->data->ds.n_images);
	NGP_HIP(hipMemcpyAsync(g.data(), t->expo_grad.get<float>(g.size()), g.size() * sizeof(float), hipMemcpyDeviceToHost, s));
	NGP_HIP(hipStreamSynchronize(s));
	exposure_update_host(t, s, g, std::max(t->cam.n_steps_between_cam_updates, 1u));
}

// NerfCounters::update_after_training (testbed_nerf.cu:3583-3609): the host reads the step's counters and adapts
// rays_per_batch to the measured batch. Returns the step's loss (get_loss).
static float step_read_counters(ngp_nerf_trainer* t, hipStream_t s, const Step& c) {
	const uint32_t B = t->cfg.target_batch_size, Rl = c.sp.Rl;
	uint32_t h[4];
	double loss_sum = 0;
	if (c.get_loss && Rl && !c.dp) {
		std::vector<float> hl(Rl);
		NGP_HIP(hipMemcpyAsync(hl.data(), c.loss, (size_t)Rl * 4, hipMemcpyDeviceToHost, s));
		NGP_HIP(hipStreamSynchronize(s));
		for (float v : hl) loss_sum += v;
	} else {
		wait_published(t->host_ctr, t->publish_seq, s);
	}
	for (int k = 0; k < 4; ++k) h[k] = t->host_ctr[k];
	if (c.dp) {
		const uint32_t lb = t->host_ctr[5];
		float lv;
		memcpy(&lv, &lb, 4);
		loss_sum = lv;
		t->measured_before_compaction_local = t->host_ctr[6];
	} else {
		t->measured_before_compaction_local = h[1];
	}
	float loss_scalar = 0.f;
	t->measured_batch_size = 0;
	t->measured_before_compaction = 0;
	if (h[1] != 0 && h[2] != 0) {
		t->measured_before_compaction = h[1];
		t->measured_batch_size = h[2];
		if (c.get_loss) t->loss_scalar = loss_scalar = (float)(loss_sum * (double)t->measured_batch_size / (double)B);
		uint32_t r = (uint32_t)((float)t->rays_per_batch * (float)B / (float)t->measured_batch_size);
		t->rays_per_batch = std::min(next_multiple(r, 256), 1u << 18);
	}
	return loss_scalar;
}

// next step's sampler, concurrent with this step's training pass (no density-grid update due first)
static void step_prelaunch_sampler(ngp_nerf_trainer* t, const Step& c) {
	// (nor a pose update: that step's cameras are uploaded on the step's stream, where the next sampler then runs; nor,
	// with error-driven sampling, a rebuild of the CDFs the sampler reads, possibly into reallocated buffers: the
	// next step launches its sampler itself, on the stream that rebuilt them)
	if (!c.can_pipeline || t->measured_batch_size == 0 || density_grid_update_due(t->training_step) || c.cam_updated ||
	    (c.em_closed && t->error_sampling()))
		return;
	const SamplePlan np = sample_plan(t);
	// early(): the sampler writes the other sample set, which the step before last read (complete: this step's
	// counters are published), so it waits on nothing
	if (!t->two_sets()) t->released.wait(t->sample_stream);
	launch_sampler(t, np, t->sample_stream);
	t->sampled.signal(t->sample_stream);
	t->pre_R = np.R;
	t->pre_max_inference = np.max_inference;
	t->prelaunched = true;
}

// next step's density-grid update: its samples now, under this step's training pass (one GPU)
static void step_pregenerate_grid_samples(ngp_nerf_trainer* t, const Step& c) {
	if (!t->knobs.grid_pregen || !c.can_pipeline || c.dp || t->training_step == 0 || !density_grid_update_due(t->training_step)) return;
	grid_update_counts(t, t->training_step, &t->pregen_nu, &t->pregen_nn);
	t->pregen_rng = t->grid_rng;
	// complete by now (the host has read this step's counters, published after the update)
	t->grid_updated.wait(t->sample_stream);
	grid_update_samples(t, t->sample_stream, t->pregen_nu, t->pregen_nn);
	t->pregenerated.signal(t->sample_stream);
	t->grid_pregen = true;
}

int ngp_nerf_train_step(ngp_nerf_trainer* t, void* stream, int get_loss, ngp_nerf_stats* st) {
	if (!t) return NGP_INVALID;
	NGP_TRY({
		hipStream_t s = step_stream(t, stream);
		Step c;
		if (t->data_epoch != t->data->ds.image_epoch) {  // an image was replaced (ngp_nerf_dataset_set_image)
			t->drain();
			t->data_epoch = t->data->ds.image_epoch;
		}
		c.pre = t->prelaunched;
		c.get_loss = get_loss != 0;
		t->prelaunched = false;
		step_density_grid(t, s, c);
		step_plan(t, c);
		step_sample_and_infer(t, s, c);
		step_loss_and_publish(t, s, c);
		step_exposure_gradients(t, s, c);
		step_release_samples(t, s, c);
		step_train_pass(t, s, c);
		step_envmap_update(t, s, c);
		step_camera_gradients(t, s, c);
		++t->training_step;
		const float loss_scalar = step_read_counters(t, s, c);
		step_camera_update(t, s, c);
		c.em_closed = error_map_step_done(t, s);
		step_prelaunch_sampler(t, c);
		step_pregenerate_grid_samples(t, c);
		step_exposure_update(t, s, c);
		if (st) {
			st->step = t->training_step;
			st->rays_per_batch = t->rays_per_batch;
			st->measured_batch_size = t->measured_batch_size;
			st->measured_batch_size_before_compaction = t->measured_before_compaction;
			st->loss = loss_scalar;
		}
		NGP_CHECK(t->measured_batch_size > 0, "Nerf training generated 0 samples (testbed_nerf.cu:3693-3697)");
	});
}
}  // extern "C"
