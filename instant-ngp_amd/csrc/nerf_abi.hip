// nerf_abi.hip — the C-ABI that needs no trainer: the NeRF dataset (with its cameras' effective matrices), the default
// config, stateless wrappers around the kernels of nerf_sampler.hip, nerf_loss.hip, nerf_density_grid.hip and envmap.hip
// (sampler, training pixels, loss, environment map, rollover, density grid), the renderer (nerf_render.hip) and
// ngp_debug_math_check. run_sampler and run_compute_loss are the wrappers' common part, which the training step
// (nerf_trainer.hip) calls too.
#include "nerf_host.h"
#include "ngp_math.h"
#include "distortion.h"

namespace ngp {
namespace nerf {

// ------------------------------------------------------------------------------------------------
// host: effective camera matrix (glm quat_cast -> slerp(t=0, start == end) -> normalize -> mat3_cast)
// ------------------------------------------------------------------------------------------------
void effective_camera_matrix(const float xf[12], float out[12]) {
	// glm column-major m[c][r] = xf[3c + r]
	auto M = [&](int c, int r) { return xf[3 * c + r]; };
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
	// slerp(q, q, 0) takes the linear branch: q * 1 + q * 0 = q; then normalize
	const float len = sqrtf(w * w + x * x + y * y + z * z);
	if (len <= 0.f) { w = 1.f; x = y = z = 0.f; }
	else { const float inv = 1.0f / len; w *= inv; x *= inv; y *= inv; z *= inv; }
	const float qxx = x * x, qyy = y * y, qzz = z * z, qxz = x * z, qxy = x * y, qyz = y * z, qwx = w * x, qwy = w * y, qwz = w * z;
	out[0] = 1.f - 2.f * (qyy + qzz); out[1] = 2.f * (qxy + qwz); out[2] = 2.f * (qxz - qwy);
	out[3] = 2.f * (qxy - qwz); out[4] = 1.f - 2.f * (qxx + qzz); out[5] = 2.f * (qyz + qwx);
	out[6] = 2.f * (qxz + qwy); out[7] = 2.f * (qyz - qwx); out[8] = 1.f - 2.f * (qxx + qyy);
	out[9] = xf[9]; out[10] = xf[10]; out[11] = xf[11];
}

Dataset::~Dataset() {
	for (float* d : depth) if (d) (void)hipFree(d);
	for (void* d : hdr) if (d) (void)hipFree(d);
	if (d_images) (void)hipFree(d_images);
	if (d_depth) (void)hipFree(d_depth);
	if (d_cams) (void)hipFree(d_cams);
	if (d_pixels) (void)hipFree(d_pixels);
}

// ngp_debug_math_check: the device forms of the shared math against their reference operations, over whole
// input ranges. which 0: ngp_div_2pf(f) vs the IEEE f / (2 + f) for all 2^23 reduced logf arguments f.
__global__ void k_check_div_2pf(unsigned long long* bad) {
	const uint32_t m = blockIdx.x * blockDim.x + threadIdx.x;
	if (m >= (1u << 23)) return;
	const float f = __uint_as_float(m + 0x3f3504f3u) - 1.0f;
	const float want = f / (2.0f + f);
	if (__float_as_uint(ngp_div_2pf(f)) != __float_as_uint(want)) atomicAdd(bad, 1ull);
}
extern "C" __attribute__((visibility("default"))) int ngp_debug_math_check(int which, void* stream, uint64_t* mismatches) {
	if (!mismatches || which != 0) return NGP_INVALID;
	hipStream_t s = (hipStream_t)stream;
	unsigned long long* d = nullptr;
	if (hipMallocAsync((void**)&d, 8, s) != hipSuccess) return NGP_ERROR;
	int rc = NGP_OK;
	if (hipMemsetAsync(d, 0, 8, s) != hipSuccess) rc = NGP_ERROR;
	if (rc == NGP_OK) {
		k_check_div_2pf<<<(1u << 23) / 256, 256, 0, s>>>(d);
		if (hipGetLastError() != hipSuccess) rc = NGP_ERROR;
	}
	unsigned long long h = 0;
	if (rc == NGP_OK && hipMemcpyAsync(&h, d, 8, hipMemcpyDeviceToHost, s) != hipSuccess) rc = NGP_ERROR;
	if (hipStreamSynchronize(s) != hipSuccess) rc = NGP_ERROR;
	(void)hipFreeAsync(d, s);
	(void)hipStreamSynchronize(s);
	*mismatches = h;
	return rc;
}

// sample_rays, optionally tracing `cams` instead of the dataset's cameras
int run_sampler(const ngp_nerf_dataset* ds, const ngp_nerf_config* cfg, void* stream, SampleArgs a, const Camera* cams,
                const DistMap* dist) {
	if (!ds || !cfg || !a.bitfield || !a.ray_indices || !a.rays || !a.numsteps || !a.coords || !a.counters) return NGP_INVALID;
	NGP_TRY({
		if (!a.n_rays_total_for_image_idx) a.n_rays_total_for_image_idx = a.n_rays;
		static thread_local Buf tmp, tmpf;
		if (a.n_rays == 0) { NGP_HIP(hipMemsetAsync(a.counters, 0, 8, S(stream))); return NGP_OK; }
		sample_rays(ds->ds, *cfg, a, tmp.get<uint32_t>(sample_tmp_u32(a.n_rays)), tmpf.get<float>(sample_tmp_f32(a.n_rays)), S(stream), cams,
		            dist);
	});
}

int run_compute_loss(const ngp_nerf_dataset* ds, const ngp_nerf_config* cfg, void* stream, LossArgs a, bool exposure_grad,
                     const float** exposure_ray_grad) {
	if (!ds || !cfg || !a.ray_counter || !a.network_output || !a.numsteps || !a.coords_in || !a.coords_out || !a.dloss_doutput ||
	    !a.compacted_counter || !a.mean_density)
		return NGP_INVALID;
	NGP_TRY({
		if (!a.n_rays_total_for_image_idx) a.n_rays_total_for_image_idx = a.n_rays;
		if (!a.state) a.state_cap = 0;
		if (!a.envmap) a.env_acc = nullptr;
		if (exposure_ray_grad) *exposure_ray_grad = nullptr;
		NGP_CHECK(!exposure_grad || (a.exposure && a.ray_indices), "compute_loss: an exposure gradient needs the exposures and the ray indices");
		NGP_CHECK(a.n_rays > 0 || !a.pub_host, "compute_loss: the counters are published by the scan, which needs rays");
		if (a.n_rays == 0) { NGP_HIP(hipMemsetAsync(a.compacted_counter, 0, 4, S(stream))); return NGP_OK; }
		static thread_local Buf tmp, tmpf;
		const size_t nf = loss_depth_on(ds->ds, a) ? loss_tmp_f32_depth(a.n_rays) : loss_tmp_f32(a.n_rays);
		float* f = tmpf.get<float>(nf + (exposure_grad ? loss_tmp_f32_exposure(a.n_rays) : 0));
		if (exposure_grad) {  // the rays' exposure gradients behind the per-ray scratch, as depth_ray is
			a.exposure_ray_grad = f + nf;
			if (exposure_ray_grad) *exposure_ray_grad = a.exposure_ray_grad;
		}
		compute_loss(ds->ds, *cfg, a, tmp.get<uint32_t>(2 * (size_t)a.n_rays), f, S(stream));
	});
}

}  // namespace nerf
}  // namespace ngp

// The parameters every ngp_nerf_compute_loss* entry shares, in the order of their signature
static LossArgs public_loss_args(uint32_t n_rays, uint32_t n_rays_total, ngp_rng rng, uint32_t max_samples_compacted,
                                 const uint32_t* ray_counter, const void* network_output, const uint32_t* ray_indices,
                                 const float* rays, uint32_t* numsteps, const float* coords_in, float* coords_out,
                                 void* dloss_doutput, float* loss, uint32_t* compacted_counter, const float* mean_density,
                                 float loss_scale) {
	LossArgs a{};
	a.n_rays = n_rays; a.n_rays_total_for_image_idx = n_rays_total; a.rng = Rng{rng.state, rng.inc};
	a.max_samples_compacted = max_samples_compacted; a.ray_counter = ray_counter;
	a.network_output = (const f16*)network_output; a.out_stride = 16;
	a.ray_indices = ray_indices; a.rays = rays; a.numsteps = numsteps; a.coords_in = coords_in; a.coords_out = coords_out;
	a.dloss_doutput = (f16*)dloss_doutput; a.loss = loss; a.compacted_counter = compacted_counter;
	a.mean_density = mean_density; a.loss_scale = loss_scale;
	return a;
}

// The dataset's image table after an image's type or pointer changed: {pointer, type} per image, a Byte image's pointer
// being its slot of the packed buffer. Allocated once an image is Half or Float.
static void upload_image_table(Dataset& ds) {
	if (!ds.d_images && ds.n_hdr == 0) return;
	std::vector<ImageRef> refs(ds.n_images);
	for (uint32_t i = 0; i < ds.n_images; ++i) {
		const bool byte = ds.types[i] == IMAGE_BYTE;
		refs[i] = ImageRef{byte ? (const void*)(ds.d_pixels + ds.cams[i].pixel_offset) : (const void*)ds.hdr[i], ds.types[i], 0u};
	}
	if (!ds.d_images) NGP_HIP(hipMalloc(&ds.d_images, ds.n_images * sizeof(ImageRef)));
	NGP_HIP(hipMemcpy(ds.d_images, refs.data(), ds.n_images * sizeof(ImageRef), hipMemcpyHostToDevice));
}

// Image i's texels from host memory, as `type`: into its slot of the packed buffer, or into an allocation of its own
static void store_image(Dataset& ds, uint32_t i, const void* host, uint32_t type) {
	const size_t n = (size_t)ds.cams[i].width * ds.cams[i].height, bytes = n * image_texel_bytes(type);
	if (type == IMAGE_BYTE) {
		NGP_HIP(hipMemcpy(ds.d_pixels + ds.cams[i].pixel_offset, host, bytes, hipMemcpyHostToDevice));
		if (ds.hdr[i]) { NGP_HIP(hipFree(ds.hdr[i])); ds.hdr[i] = nullptr; --ds.n_hdr; }
	} else {
		void* p = nullptr;
		NGP_HIP(hipMalloc(&p, bytes));
		if (hipMemcpy(p, host, bytes, hipMemcpyHostToDevice) != hipSuccess) { (void)hipFree(p); throw Error("nerf dataset: image upload failed"); }
		if (ds.hdr[i]) NGP_HIP(hipFree(ds.hdr[i]));
		else ++ds.n_hdr;
		ds.hdr[i] = p;
	}
	ds.types[i] = type;
}

// ngp_nerf_dataset_create and _create_typed (types null: every image Byte)
static int ngp_nerf_dataset_create_typed_impl(uint32_t n_images, const ngp_nerf_image* images, const void* const* pixels,
                                              const uint32_t* types, ngp_nerf_dataset** out) {
	if (!out || !images || !pixels || n_images == 0) return NGP_INVALID;
	NGP_TRY({
		auto d = std::make_unique<ngp_nerf_dataset>();
		d->ds.n_images = n_images;
		uint64_t total = 0;
		std::vector<Camera> cams(n_images);
		for (uint32_t i = 0; i < n_images; ++i) {
			const ngp_nerf_image& im = images[i];
			Camera& c = cams[i];
			c.width = im.width; c.height = im.height;
			c.focal[0] = im.focal_length[0]; c.focal[1] = im.focal_length[1];
			c.principal[0] = im.principal_point[0]; c.principal[1] = im.principal_point[1];
			NGP_CHECK(im.lens_mode <= LENS_OPENCV_FISHEYE, "nerf dataset: unsupported lens mode");
			c.lens_mode = im.lens_mode;
			for (int k = 0; k < 4; ++k) c.lens[k] = im.lens_params[k];
			effective_camera_matrix(im.xform, c.m);
			c.pixel_offset = total;
			total += (uint64_t)im.width * im.height;
		}
		NGP_HIP(hipMalloc(&d->ds.d_pixels, total * 4 + 12 * 4 * n_images));
		d->ds.cams = cams;
		d->ds.types.assign(n_images, IMAGE_BYTE);
		d->ds.hdr.assign(n_images, nullptr);
		for (uint32_t i = 0; i < n_images; ++i) {
			NGP_CHECK(pixels[i] != nullptr, "nerf dataset: an image without pixels");
			const uint32_t type = types ? types[i] : (uint32_t)IMAGE_BYTE;
			// a Half or Float image's slot of the packed buffer is never read; zeroed, so that its bytes are defined
			if (type != IMAGE_BYTE) NGP_HIP(hipMemset(d->ds.d_pixels + cams[i].pixel_offset, 0, (size_t)images[i].width * images[i].height * 4));
			store_image(d->ds, i, pixels[i], type);
		}
		upload_image_table(d->ds);
		// raw (start) transforms after the pixels, for mark_untrained_density_grid
		std::vector<float> raw(12 * n_images);
		for (uint32_t i = 0; i < n_images; ++i) memcpy(&raw[12 * i], images[i].xform, 48);
		NGP_HIP(hipMemcpy(d->ds.d_pixels + total, raw.data(), raw.size() * 4, hipMemcpyHostToDevice));
		d->ds.xforms = raw;
		NGP_HIP(hipMalloc(&d->ds.d_cams, n_images * sizeof(Camera)));
		NGP_HIP(hipMemcpy(d->ds.d_cams, cams.data(), n_images * sizeof(Camera), hipMemcpyHostToDevice));
		*out = d.release();
	});
}

struct ngp_nerf_renderer {
	Buf pay0, pay1, payh, rgba0, rgba1, rgbah, coords, out, frame, counters;
	DistMap dist{nullptr, 0, 0};          // ngp_nerf_renderer_set_distortion_map (the caller's device memory)
	const float* envmap = nullptr;        // ngp_nerf_renderer_set_envmap (the caller's device memory)
	uint32_t env_w = 0, env_h = 0;
	uint32_t* host_counters = nullptr;
	uint32_t render_mode = RENDER_SHADE;  // ngp_nerf_renderer_set_mode
	int32_t show_accel = -1;             // ngp_nerf_renderer_set_show_accel
	float depth_scale = 1.0f;             // ngp_nerf_renderer_set_depth_scale
	~ngp_nerf_renderer() { if (host_counters) (void)hipHostFree(host_counters); }
};

extern "C" {

int ngp_nerf_default_config(float aabb_scale, ngp_nerf_config* o) {
	if (!o || !(aabb_scale >= 1.0f)) return NGP_INVALID;
	memset(o, 0, sizeof(*o));
	const float inflate = 0.5f * std::min((float)(1 << (CASCADES - 1)), aabb_scale);  // testbed_nerf.cu:3093-3094
	for (int k = 0; k < 3; ++k) { o->aabb_min[k] = 0.5f - inflate; o->aabb_max[k] = 0.5f + inflate; }
	uint32_t mc = 0;
	while ((float)(1u << mc) < aabb_scale) ++mc;  // :3102-3105
	o->max_cascade = mc;
	o->cone_angle_constant = aabb_scale <= 1.0f ? 0.0f : 1.0f / 256.0f;  // :3109
	o->snap_to_pixel_centers = 1;
	o->random_bg_color = 1;
	o->linear_colors = 0;
	o->color_space_linear = 1;
	o->rgb_activation = ACT_EXP;
	o->density_activation = ACT_EXP;
	o->loss_type = LOSS_HUBER;  // configs/nerf/base.json "loss": Huber
	o->near_distance = 0.1f;
	o->target_batch_size = 1u << 18;
	return NGP_OK;
}

int ngp_nerf_dataset_create(uint32_t n_images, const ngp_nerf_image* images, const void* const* rgba8, ngp_nerf_dataset** out) {
	return ngp_nerf_dataset_create_typed_impl(n_images, images, rgba8, nullptr, out);
}

int ngp_nerf_dataset_create_typed(uint32_t n_images, const ngp_nerf_image* images, const void* const* pixels_host,
                                  const uint32_t* image_types, ngp_nerf_dataset** out) {
	if (!image_types || !pixels_host) return NGP_INVALID;
	for (uint32_t i = 0; i < n_images; ++i)
		if (!image_type_ok(image_types[i]) || !pixels_host[i]) return NGP_INVALID;
	return ngp_nerf_dataset_create_typed_impl(n_images, images, pixels_host, image_types, out);
}

int ngp_nerf_dataset_set_image(ngp_nerf_dataset* d, uint32_t image, const void* pixels_host, uint32_t image_type, uint32_t width,
                               uint32_t height) {
	if (!d || !pixels_host || image >= d->ds.n_images || !image_type_ok(image_type)) return NGP_INVALID;
	if (width != d->ds.cams[image].width || height != d->ds.cams[image].height) return NGP_INVALID;  // resizing is not built
	NGP_TRY({
		Dataset& ds = d->ds;
		NGP_HIP(hipDeviceSynchronize());  // no sampler or loss pass may still be reading the image or the table
		const bool table_changes = image_type != IMAGE_BYTE || ds.types[image] != IMAGE_BYTE;
		store_image(ds, image, pixels_host, image_type);
		if (table_changes) upload_image_table(ds);  // Byte over Byte rewrites the packed buffer in place
		++ds.image_epoch;
	});
}

int ngp_nerf_dataset_image(const ngp_nerf_dataset* d, uint32_t image, void* out_host, uint64_t cap, uint32_t* image_type) {
	if (!d || image >= d->ds.n_images) return NGP_INVALID;
	const Dataset& ds = d->ds;
	const uint32_t type = ds.types[image];
	const size_t bytes = (size_t)ds.cams[image].width * ds.cams[image].height * image_texel_bytes(type);
	if (out_host && cap < bytes) return NGP_INVALID;
	if (image_type) *image_type = type;
	if (!out_host) return NGP_OK;
	const void* src = type == IMAGE_BYTE ? (const void*)(ds.d_pixels + ds.cams[image].pixel_offset) : (const void*)ds.hdr[image];
	NGP_TRY(NGP_HIP(hipMemcpy(out_host, src, bytes, hipMemcpyDeviceToHost)));
}

void ngp_nerf_dataset_destroy(ngp_nerf_dataset* d) { delete d; }

// NerfDataset::set_training_image's depth part (nerf_loader.cu:943-960) with copy_depth (:81-90): one fp32 multiply
// per pixel, done on the host, so the stored value is (float)pixel * depth_scale bit for bit
int ngp_nerf_dataset_set_depth(ngp_nerf_dataset* d, uint32_t image, const void* depth_host, int dtype, float depth_scale) {
	if (!d || image >= d->ds.n_images || (dtype != 0 && dtype != 1) || std::isnan(depth_scale)) return NGP_INVALID;
	NGP_TRY({
		Dataset& ds = d->ds;
		NGP_HIP(hipDeviceSynchronize());  // no loss pass may still be reading the pointers or the image
		if (ds.depth.empty()) ds.depth.assign(ds.n_images, nullptr);
		const size_t n = (size_t)ds.cams[image].width * ds.cams[image].height;
		if (!depth_host && depth_scale < 0.f) {
			if (ds.depth[image]) { NGP_HIP(hipFree(ds.depth[image])); ds.depth[image] = nullptr; --ds.n_depth; }
		} else {
			std::vector<float> v(n, 0.0f);  // no depth data for this image: zeros
			if (depth_host && depth_scale > 0.f) {
				if (dtype == 0) for (size_t k = 0; k < n; ++k) v[k] = (float)((const uint16_t*)depth_host)[k] * depth_scale;
				else for (size_t k = 0; k < n; ++k) v[k] = ((const float*)depth_host)[k] * depth_scale;
			}
			if (!ds.depth[image]) { NGP_HIP(hipMalloc(&ds.depth[image], n * 4)); ++ds.n_depth; }
			NGP_HIP(hipMemcpy(ds.depth[image], v.data(), n * 4, hipMemcpyHostToDevice));
		}
		if (!ds.d_depth) NGP_HIP(hipMalloc(&ds.d_depth, ds.n_images * sizeof(float*)));
		NGP_HIP(hipMemcpy(ds.d_depth, ds.depth.data(), ds.n_images * sizeof(float*), hipMemcpyHostToDevice));
	});
}

int ngp_nerf_dataset_depth(const ngp_nerf_dataset* d, uint32_t image, float* out_host, uint64_t cap, int* has_depth) {
	if (!d || image >= d->ds.n_images) return NGP_INVALID;
	const Dataset& ds = d->ds;
	const float* src = ds.depth.empty() ? nullptr : ds.depth[image];
	const size_t n = (size_t)ds.cams[image].width * ds.cams[image].height;
	if (src && out_host && cap < n) return NGP_INVALID;
	if (has_depth) *has_depth = src ? 1 : 0;
	if (!src || !out_host) return NGP_OK;
	NGP_TRY(NGP_HIP(hipMemcpy(out_host, src, n * 4, hipMemcpyDeviceToHost)));
}

int ngp_nerf_generate_training_samples(const ngp_nerf_dataset* ds, const ngp_nerf_config* cfg, void* stream, uint32_t n_rays,
                                       uint32_t ray_offset, uint32_t n_rays_total, ngp_rng rng, uint32_t max_samples,
                                       const uint8_t* bitfield, uint32_t* ray_indices, float* rays, uint32_t* numsteps,
                                       float* coords, uint32_t* counters) {
	SampleArgs a{};
	a.n_rays = n_rays; a.ray_offset = ray_offset; a.n_rays_total_for_image_idx = n_rays_total;
	a.max_samples = max_samples; a.rng = Rng{rng.state, rng.inc}; a.bitfield = bitfield;
	a.ray_indices = ray_indices; a.rays = rays; a.numsteps = numsteps; a.coords = coords; a.counters = counters;
	return run_sampler(ds, cfg, stream, a, nullptr);
}
int ngp_nerf_generate_training_samples_cdf(const ngp_nerf_dataset* ds, const ngp_nerf_config* cfg, void* stream, uint32_t n_rays,
                                           uint32_t ray_offset, uint32_t n_rays_total, ngp_rng rng, uint32_t max_samples,
                                           const uint8_t* bitfield, uint32_t* ray_indices, float* rays, uint32_t* numsteps,
                                           float* coords, uint32_t* counters, const ngp_nerf_error_cdfs* cdfs) {
	SampleArgs a{};
	if (!error_cdfs_arg(cdfs, &a.cdfs)) return NGP_INVALID;
	a.n_rays = n_rays; a.ray_offset = ray_offset; a.n_rays_total_for_image_idx = n_rays_total;
	a.max_samples = max_samples; a.rng = Rng{rng.state, rng.inc}; a.bitfield = bitfield;
	a.ray_indices = ray_indices; a.rays = rays; a.numsteps = numsteps; a.coords = coords; a.counters = counters;
	return run_sampler(ds, cfg, stream, a, nullptr);
}

int ngp_nerf_generate_training_samples_distortion(const ngp_nerf_dataset* ds, const ngp_nerf_config* cfg, void* stream, uint32_t n_rays,
                                                  uint32_t ray_offset, uint32_t n_rays_total, ngp_rng rng, uint32_t max_samples,
                                                  const uint8_t* bitfield, uint32_t* ray_indices, float* rays, uint32_t* numsteps,
                                                  float* coords, uint32_t* counters, const ngp_nerf_error_cdfs* cdfs,
                                                  const float* distortion_map, uint32_t map_width, uint32_t map_height) {
	SampleArgs a{};
	if (!error_cdfs_arg(cdfs, &a.cdfs)) return NGP_INVALID;
	if (distortion_map && !distortion_dims_ok(map_width, map_height)) return NGP_INVALID;
	a.n_rays = n_rays; a.ray_offset = ray_offset; a.n_rays_total_for_image_idx = n_rays_total;
	a.max_samples = max_samples; a.rng = Rng{rng.state, rng.inc}; a.bitfield = bitfield;
	a.ray_indices = ray_indices; a.rays = rays; a.numsteps = numsteps; a.coords = coords; a.counters = counters;
	const DistMap dm{distortion_map, map_width, map_height};
	return run_sampler(ds, cfg, stream, a, nullptr, distortion_map ? &dm : nullptr);
}

int ngp_nerf_training_pixels(const ngp_nerf_dataset* ds, const ngp_nerf_config* cfg, void* stream, uint32_t n_rays, uint32_t ray_offset,
                             uint32_t n_rays_total, ngp_rng rng, const ngp_nerf_error_cdfs* cdfs, uint32_t* img, float* uv, float* pdf) {
	ErrorCdfs e;
	if (!ds || !cfg || !img || !uv || !pdf || !error_cdfs_arg(cdfs, &e)) return NGP_INVALID;
	NGP_TRY(training_pixels(ds->ds, *cfg, n_rays, ray_offset, n_rays_total ? n_rays_total : n_rays, Rng{rng.state, rng.inc}, e, img, uv,
	                        pdf, S(stream)));
}
int ngp_nerf_training_pixels_host(uint32_t n_images, const ngp_nerf_image* images, const ngp_nerf_config* cfg, uint32_t n_rays,
                                  uint32_t ray_offset, uint32_t n_rays_total, ngp_rng rng, const ngp_nerf_error_cdfs* cdfs,
                                  uint32_t* img, float* uv, float* pdf) {
	ErrorCdfs e;
	if (!images || n_images == 0 || !cfg || !img || !uv || !pdf || !error_cdfs_arg(cdfs, &e)) return NGP_INVALID;
	NGP_TRY({
		std::vector<Camera> cams(n_images);
		for (uint32_t i = 0; i < n_images; ++i) {
			if (images[i].width == 0 || images[i].height == 0) return NGP_INVALID;
			cams[i] = Camera{};
			cams[i].width = images[i].width; cams[i].height = images[i].height;
		}
		training_pixels_host(cams.data(), n_images, *cfg, n_rays, ray_offset, n_rays_total ? n_rays_total : n_rays,
		                     Rng{rng.state, rng.inc}, e, img, uv, pdf);
	});
}

int ngp_nerf_compute_loss(const ngp_nerf_dataset* ds, const ngp_nerf_config* cfg, void* stream, uint32_t n_rays,
                          uint32_t n_rays_total, ngp_rng rng, uint32_t max_samples_compacted, const uint32_t* ray_counter,
                          const void* network_output, const uint32_t* ray_indices, const float* rays, uint32_t* numsteps,
                          const float* coords_in, float* coords_out, void* dloss_doutput, float* loss,
                          uint32_t* compacted_counter, const float* mean_density, float loss_scale) {
	const LossArgs a = public_loss_args(n_rays, n_rays_total, rng, max_samples_compacted, ray_counter, network_output, ray_indices, rays,
	                                    numsteps, coords_in, coords_out, dloss_doutput, loss, compacted_counter, mean_density, loss_scale);
	return run_compute_loss(ds, cfg, stream, a);
}

int ngp_nerf_compute_loss_error_map(const ngp_nerf_dataset* ds, const ngp_nerf_config* cfg, void* stream, uint32_t n_rays,
                                    uint32_t n_rays_total, ngp_rng rng, uint32_t max_samples_compacted,
                                    const uint32_t* ray_counter, const void* network_output, const uint32_t* ray_indices,
                                    const float* rays, uint32_t* numsteps, const float* coords_in, float* coords_out,
                                    void* dloss_doutput, float* loss, uint32_t* compacted_counter, const float* mean_density,
                                    float loss_scale, float* error_map, uint32_t em_width, uint32_t em_height) {
	if (error_map && (em_width < 2 || em_height < 2)) return NGP_INVALID;  // the bilinear deposit needs a 2x2 texel block
	LossArgs a = public_loss_args(n_rays, n_rays_total, rng, max_samples_compacted, ray_counter, network_output, ray_indices, rays,
	                              numsteps, coords_in, coords_out, dloss_doutput, loss, compacted_counter, mean_density, loss_scale);
	a.error_map = error_map; a.em_w = em_width; a.em_h = em_height;
	return run_compute_loss(ds, cfg, stream, a);
}

int ngp_nerf_compute_loss_state(const ngp_nerf_dataset* ds, const ngp_nerf_config* cfg, void* stream, uint32_t n_rays,
                                uint32_t n_rays_total, ngp_rng rng, uint32_t max_samples_compacted, const uint32_t* ray_counter,
                                const void* network_output, const uint32_t* ray_indices, const float* rays, uint32_t* numsteps,
                                const float* coords_in, float* coords_out, void* dloss_doutput, float* loss,
                                uint32_t* compacted_counter, const float* mean_density, float loss_scale, float* sample_state,
                                uint64_t state_capacity) {
	if (!sample_state || state_capacity == 0) return NGP_INVALID;
	LossArgs a = public_loss_args(n_rays, n_rays_total, rng, max_samples_compacted, ray_counter, network_output, ray_indices, rays,
	                              numsteps, coords_in, coords_out, dloss_doutput, loss, compacted_counter, mean_density, loss_scale);
	a.state = sample_state; a.state_cap = state_capacity;
	return run_compute_loss(ds, cfg, stream, a);
}

int ngp_nerf_compute_loss_cdf(const ngp_nerf_dataset* ds, const ngp_nerf_config* cfg, void* stream, uint32_t n_rays,
                              uint32_t n_rays_total, ngp_rng rng, uint32_t max_samples_compacted, const uint32_t* ray_counter,
                              const void* network_output, const uint32_t* ray_indices, const float* rays, uint32_t* numsteps,
                              const float* coords_in, float* coords_out, void* dloss_doutput, float* loss,
                              uint32_t* compacted_counter, const float* mean_density, float loss_scale, float* error_map,
                              uint32_t em_width, uint32_t em_height, const ngp_nerf_error_cdfs* cdfs) {
	LossArgs a = public_loss_args(n_rays, n_rays_total, rng, max_samples_compacted, ray_counter, network_output, ray_indices, rays,
	                              numsteps, coords_in, coords_out, dloss_doutput, loss, compacted_counter, mean_density, loss_scale);
	if (!error_cdfs_arg(cdfs, &a.cdfs)) return NGP_INVALID;
	if (error_map && (em_width < 2 || em_height < 2)) return NGP_INVALID;
	a.error_map = error_map; a.em_w = em_width; a.em_h = em_height;
	return run_compute_loss(ds, cfg, stream, a);
}

int ngp_nerf_compute_loss_envmap(const ngp_nerf_dataset* ds, const ngp_nerf_config* cfg, void* stream, uint32_t n_rays,
                                 uint32_t n_rays_total, ngp_rng rng, uint32_t max_samples_compacted, const uint32_t* ray_counter,
                                 const void* network_output, const uint32_t* ray_indices, const float* rays, uint32_t* numsteps,
                                 const float* coords_in, float* coords_out, void* dloss_doutput, float* loss,
                                 uint32_t* compacted_counter, const float* mean_density, float loss_scale, const float* envmap,
                                 uint32_t env_width, uint32_t env_height, uint32_t envmap_loss_type, float* envmap_gradient) {
	if (!envmap || !rays || !envmap_dims_ok(env_width, env_height) || envmap_loss_type > LOSS_RELL2) return NGP_INVALID;
	NGP_TRY({
		static thread_local Buf acc;
		LossArgs a = public_loss_args(n_rays, n_rays_total, rng, max_samples_compacted, ray_counter, network_output, ray_indices, rays,
		                              numsteps, coords_in, coords_out, dloss_doutput, loss, compacted_counter, mean_density, loss_scale);
		a.envmap = envmap; a.env_w = env_width; a.env_h = env_height; a.env_loss_type = envmap_loss_type;
		if (envmap_gradient) {
			const size_t words = envmap_acc_words64(env_width, env_height);
			a.env_acc = acc.get<unsigned long long>(words);
			NGP_HIP(hipMemsetAsync(a.env_acc, 0, words * 8, S(stream)));
		}
		const int rc = run_compute_loss(ds, cfg, stream, a);
		if (rc != NGP_OK) return rc;  // the error string is set
		if (envmap_gradient) envmap_gradient_f32(env_width, env_height, a.env_acc, envmap_gradient, S(stream));
	});
}

int ngp_nerf_compute_loss_depth(const ngp_nerf_dataset* ds, const ngp_nerf_config* cfg, void* stream, uint32_t n_rays,
                                uint32_t n_rays_total, ngp_rng rng, uint32_t max_samples_compacted, const uint32_t* ray_counter,
                                const void* network_output, const uint32_t* ray_indices, const float* rays, uint32_t* numsteps,
                                const float* coords_in, float* coords_out, void* dloss_doutput, float* loss,
                                uint32_t* compacted_counter, const float* mean_density, float loss_scale, float* error_map,
                                uint32_t em_width, uint32_t em_height, const ngp_nerf_error_cdfs* cdfs, const float* envmap,
                                uint32_t env_width, uint32_t env_height, uint32_t envmap_loss_type, float* envmap_gradient,
                                float* sample_state, uint64_t state_capacity, float depth_supervision_lambda,
                                uint32_t depth_loss_type) {
	// the same call without exposures: one set of checks and one setup for both
	return ngp_nerf_compute_loss_exposure(ds, cfg, stream, n_rays, n_rays_total, rng, max_samples_compacted, ray_counter, network_output,
	                                      ray_indices, rays, numsteps, coords_in, coords_out, dloss_doutput, loss, compacted_counter,
	                                      mean_density, loss_scale, error_map, em_width, em_height, cdfs, envmap, env_width, env_height,
	                                      envmap_loss_type, envmap_gradient, sample_state, state_capacity, depth_supervision_lambda,
	                                      depth_loss_type, nullptr, nullptr);
}

int ngp_nerf_compute_loss_exposure(const ngp_nerf_dataset* ds, const ngp_nerf_config* cfg, void* stream, uint32_t n_rays,
                                   uint32_t n_rays_total, ngp_rng rng, uint32_t max_samples_compacted, const uint32_t* ray_counter,
                                   const void* network_output, const uint32_t* ray_indices, const float* rays, uint32_t* numsteps,
                                   const float* coords_in, float* coords_out, void* dloss_doutput, float* loss,
                                   uint32_t* compacted_counter, const float* mean_density, float loss_scale, float* error_map,
                                   uint32_t em_width, uint32_t em_height, const ngp_nerf_error_cdfs* cdfs, const float* envmap,
                                   uint32_t env_width, uint32_t env_height, uint32_t envmap_loss_type, float* envmap_gradient,
                                   float* sample_state, uint64_t state_capacity, float depth_supervision_lambda,
                                   uint32_t depth_loss_type, const float* exposure, float* exposure_gradient) {
	if (!ds) return NGP_INVALID;
	if (!(depth_supervision_lambda >= 0.0f) || std::isinf(depth_supervision_lambda) || depth_loss_type > LOSS_RELL2) return NGP_INVALID;
	if (depth_supervision_lambda > 0.0f && !rays) return NGP_INVALID;
	if (envmap ? (!rays || !envmap_dims_ok(env_width, env_height) || envmap_loss_type > LOSS_RELL2) : envmap_gradient != nullptr)
		return NGP_INVALID;
	if (sample_state && state_capacity == 0) return NGP_INVALID;
	if (error_map && (em_width < 2 || em_height < 2)) return NGP_INVALID;
	if (exposure && !ray_indices) return NGP_INVALID;
	// the per-image sum needs the exposures, and an image's rays in one run: no image CDF
	if (exposure_gradient && (!exposure || (cdfs && cdfs->cdf_img))) return NGP_INVALID;
	const uint32_t total = n_rays_total ? n_rays_total : n_rays;
	if (exposure_gradient && (uint64_t)total * ds->ds.n_images > 0xffffffffull) return NGP_INVALID;
	NGP_TRY({
		static thread_local Buf acc;
		LossArgs a = public_loss_args(n_rays, n_rays_total, rng, max_samples_compacted, ray_counter, network_output, ray_indices, rays,
		                              numsteps, coords_in, coords_out, dloss_doutput, loss, compacted_counter, mean_density, loss_scale);
		if (!error_cdfs_arg(cdfs, &a.cdfs)) return NGP_INVALID;
		a.error_map = error_map; a.em_w = em_width; a.em_h = em_height;
		a.state = sample_state; a.state_cap = state_capacity;
		a.depth_lambda = depth_supervision_lambda; a.depth_loss_type = depth_loss_type;
		a.exposure = exposure;
		if (envmap) {
			a.envmap = envmap; a.env_w = env_width; a.env_h = env_height; a.env_loss_type = envmap_loss_type;
			if (envmap_gradient) {
				const size_t words = envmap_acc_words64(env_width, env_height);
				a.env_acc = acc.get<unsigned long long>(words);
				NGP_HIP(hipMemsetAsync(a.env_acc, 0, words * 8, S(stream)));
			}
		}
		const float* ray_grad = nullptr;
		const int rc = run_compute_loss(ds, cfg, stream, a, exposure_gradient != nullptr, &ray_grad);
		if (rc != NGP_OK) return rc;  // the error string is set
		if (a.env_acc) envmap_gradient_f32(env_width, env_height, a.env_acc, envmap_gradient, S(stream));
		if (ray_grad) {
			ExposureGradArgs g{};
			g.n_rays_cap = n_rays; g.n_rays_total = total; g.n_images = ds->ds.n_images;
			g.ray_counter = ray_counter; g.ray_indices = ray_indices; g.numsteps = numsteps;
			g.ray_grad = ray_grad; g.image_grad = exposure_gradient;
			exposure_gradients(g, S(stream));
		}
	});
}

int ngp_envmap_lookup(void* stream, uint32_t width, uint32_t height, uint32_t n, const float* dirs, uint32_t* texels, float* weights) {
	if (!envmap_dims_ok(width, height) || (n && (!dirs || !texels || !weights))) return NGP_INVALID;
	NGP_TRY({ envmap_lookup_device(width, height, n, dirs, texels, weights, S(stream)); });
}

int ngp_envmap_lookup_host(uint32_t width, uint32_t height, uint32_t n, const float* dirs, uint32_t* texels, float* weights) {
	if (!envmap_dims_ok(width, height) || (n && (!dirs || !texels || !weights))) return NGP_INVALID;
	envmap_lookup_host(width, height, n, dirs, texels, weights);
	return NGP_OK;
}

int ngp_envmap_deposit(void* stream, uint32_t width, uint32_t height, uint32_t n, const float* dirs, const void* values_f16,
                       float* gradient) {
	if (!envmap_dims_ok(width, height) || !gradient || (n && (!dirs || !values_f16))) return NGP_INVALID;
	NGP_TRY({
		static thread_local Buf acc;
		const size_t words = envmap_acc_words64(width, height);
		unsigned long long* a = acc.get<unsigned long long>(words);
		NGP_HIP(hipMemsetAsync(a, 0, words * 8, S(stream)));
		envmap_deposit_values(width, height, n, dirs, (const f16*)values_f16, a, S(stream));
		envmap_gradient_f32(width, height, a, gradient, S(stream));
	});
}

// ---- lens distortion map: the stand-alone forms (distortion.h, distortion.hip) ----------------------------------------
int ngp_nerf_distortion_lookup(void* stream, uint32_t width, uint32_t height, uint32_t n, const float* uv, uint32_t* texels,
                               float* weights, const float* map, float* offsets) {
	if (!distortion_dims_ok(width, height) || (n && (!uv || !texels || !weights)) || (offsets && !map)) return NGP_INVALID;
	NGP_TRY({ distortion_lookup_device(width, height, n, uv, texels, weights, map, offsets, S(stream)); });
}

int ngp_nerf_distortion_lookup_host(uint32_t width, uint32_t height, uint32_t n, const float* uv, uint32_t* texels, float* weights,
                                    const float* map, float* offsets) {
	if (!distortion_dims_ok(width, height) || (n && (!uv || !texels || !weights)) || (offsets && !map)) return NGP_INVALID;
	distortion_lookup_host(width, height, n, uv, texels, weights, map, offsets);
	return NGP_OK;
}

uint64_t ngp_nerf_distortion_accumulator_words(uint32_t width, uint32_t height) {
	return distortion_dims_ok(width, height) ? (uint64_t)distortion_acc_words64(width, height) : 0;
}

int ngp_nerf_distortion_deposit(const ngp_nerf_dataset* ds, const ngp_nerf_config* cfg, void* stream, uint32_t n_rays_total, ngp_rng rng,
                                const uint32_t* ray_counter, const uint32_t* ray_indices, const uint32_t* numsteps,
                                const float* ray_gradients, uint32_t width, uint32_t height, uint64_t* accumulator) {
	if (!ds || !cfg || !ray_counter || !ray_indices || !ray_gradients || !accumulator || n_rays_total == 0 ||
	    !distortion_dims_ok(width, height) || (uint64_t)n_rays_total * ds->ds.n_images > 0xffffffffull)
		return NGP_INVALID;
	NGP_TRY({
		DistDepositArgs a{};
		// kept rays are distinct ids below n_rays_total: at most that many rows
		a.n_rays_cap = n_rays_total; a.n_rays_total = n_rays_total; a.n_images = ds->ds.n_images;
		a.snap = cfg->snap_to_pixel_centers != 0; a.rng = Rng{rng.state, rng.inc}; a.cams = ds->ds.d_cams;
		a.ray_counter = ray_counter; a.ray_indices = ray_indices; a.numsteps = numsteps; a.ray_grad = ray_gradients;
		a.w = width; a.h = height; a.acc = (unsigned long long*)accumulator;
		distortion_deposit_rays(a, S(stream));
	});
}

int ngp_nerf_distortion_gradient(void* stream, uint32_t width, uint32_t height, const uint64_t* accumulator, float* gradient) {
	if (!distortion_dims_ok(width, height) || !accumulator || !gradient) return NGP_INVALID;
	NGP_TRY({ distortion_gradient_f32(width, height, (const unsigned long long*)accumulator, gradient, S(stream)); });
}

int ngp_envmap_optimizer_step(void* stream, const char* optimizer_json, uint32_t step, float loss_scale, uint32_t n, float* params,
                              const float* gradient, float* first_moments, float* second_moments, uint32_t* param_steps, float* ema,
                              float* ema_params) {
	if (!optimizer_json || !params || !gradient || !first_moments || !second_moments || !param_steps || !(loss_scale > 0.f))
		return NGP_INVALID;
	NGP_TRY({
		AdamConfig c;
		parse_optimizer_json(optimizer_json, c);
		AdamState st{};
		st.w32 = params; st.g32 = gradient; st.m1 = first_moments; st.m2 = second_moments; st.steps = param_steps;
		st.ema32 = ema; st.ema_f32 = ema_params; st.step_add = step;
		adam_ema_update_f32(c, n, loss_scale, st, S(stream));
	});
}

int ngp_nerf_fill_rollover(void* stream, uint32_t n_elements, uint32_t stride, const uint32_t* n_input, void* data, int dtype,
                           int rescale) {
	if (!n_input || !data) return NGP_INVALID;
	NGP_TRY({
		if (dtype == 1) fill_rollover_f16(n_elements, stride, n_input, (f16*)data, rescale != 0, S(stream));
		else fill_rollover_f32(n_elements, stride, n_input, (float*)data, S(stream));
	});
}

int ngp_nerf_grid_generate_samples(void* stream, const ngp_nerf_config* cfg, uint32_t n, ngp_rng rng, uint32_t step,
                                   const float* grid, uint32_t n_cascades, float thresh, float* positions, uint32_t* indices) {
	if (!cfg || !grid || !positions || !indices) return NGP_INVALID;
	NGP_TRY({
		static thread_local Buf mask;
		grid_generate_samples(n, Rng{rng.state, rng.inc}, step, *cfg, grid, n_cascades, thresh, positions, indices,
		                      mask.get<uint32_t>(grid_mask_words(n_cascades)), S(stream));
	});
}
int ngp_nerf_grid_splat_max(void* stream, uint32_t n, const uint32_t* indices, const void* density_rm, uint32_t act, float* tmp) {
	if (!indices || !density_rm || !tmp) return NGP_INVALID;
	NGP_TRY(grid_splat_max(n, indices, (const f16*)density_rm, act, tmp, S(stream)));
}
int ngp_nerf_grid_splat_max_cells(void* stream, uint32_t n, const uint32_t* indices, const void* density_rm, uint32_t act,
                                  float* tmp, uint32_t n_cells) {
	if ((n && (!indices || !density_rm)) || !tmp || n_cells == 0 || n_cells % 8192 || n_cells > 8 * GRID_N_CELLS) return NGP_INVALID;
	NGP_TRY({
		static thread_local Buf scratch;
		grid_splat_max_binned(n, indices, (const f16*)density_rm, act, tmp, n_cells,
		                      scratch.get<uint32_t>(grid_splat_scratch_u32(n, n_cells)), S(stream));
	});
}
int ngp_nerf_grid_ema(void* stream, uint32_t n, float decay, float* grid, const float* tmp) {
	if (!grid || !tmp) return NGP_INVALID;
	NGP_TRY(grid_ema(n, decay, grid, tmp, S(stream)));
}
int ngp_nerf_grid_mean_and_bitfield(void* stream, const float* grid, uint32_t max_cascade, float* mean, uint8_t* bitfield) {
	if (!grid || !mean || !bitfield || max_cascade >= CASCADES) return NGP_INVALID;
	NGP_TRY(grid_mean_bitfield(grid, max_cascade, mean, bitfield, S(stream)));
}

// ---- rendering ---------------------------------------------------------------------------------
int ngp_nerf_renderer_create(ngp_nerf_renderer** out) {
	if (!out) return NGP_INVALID;
	NGP_TRY({ *out = new ngp_nerf_renderer(); });
}
void ngp_nerf_renderer_destroy(ngp_nerf_renderer* r) { delete r; }
int ngp_nerf_renderer_set_mode(ngp_nerf_renderer* r, int render_mode) {
	if (!r || render_mode < (int)RENDER_AO || (render_mode > (int)RENDER_DISTORTION && render_mode != (int)RENDER_ENCODING_VIS))
		return NGP_INVALID;
	r->render_mode = (uint32_t)render_mode;
	return NGP_OK;
}
int ngp_nerf_renderer_set_show_accel(ngp_nerf_renderer* r, int show_accel) {
	if (!r || show_accel < -1 || show_accel >= (int)CASCADES) return NGP_INVALID;
	r->show_accel = show_accel;
	return NGP_OK;
}
int ngp_nerf_renderer_set_depth_scale(ngp_nerf_renderer* r, float depth_scale) {
	if (!r) return NGP_INVALID;
	r->depth_scale = depth_scale;
	return NGP_OK;
}
int ngp_nerf_renderer_set_envmap(ngp_nerf_renderer* r, const float* envmap, uint32_t width, uint32_t height) {
	if (!r || (envmap && !envmap_dims_ok(width, height))) return NGP_INVALID;
	r->envmap = envmap;
	r->env_w = envmap ? width : 0;
	r->env_h = envmap ? height : 0;
	return NGP_OK;
}

int ngp_nerf_renderer_set_distortion_map(ngp_nerf_renderer* r, const float* map, uint32_t width, uint32_t height) {
	if (!r || (map && !distortion_dims_ok(width, height))) return NGP_INVALID;
	r->dist = DistMap{map, map ? width : 0, map ? height : 0};
	return NGP_OK;
}

int ngp_nerf_render(ngp_nerf_renderer* r, ngp_model* model, const ngp_nerf_config* cfg, void* stream, const ngp_nerf_image* camera,
                    const uint8_t* bitfield, uint32_t spp, uint32_t sample_index, float min_transmittance, const float* background_rgba,
                    int use_inference_params, float* out_rgba) {
	if (!r || !model || !cfg || !camera || !out_rgba || spp == 0) return NGP_INVALID;
	NGP_TRY({
		hipStream_t s = S(stream);
		RenderArgs a{};
		a.width = camera->width; a.height = camera->height;
		a.focal[0] = camera->focal_length[0]; a.focal[1] = camera->focal_length[1];
		// m_screen_center = 1 - principal point (set_camera_to_training_view, testbed.cu:852), then
		// render_screen_center (testbed.cu:4376-4379, zoom 1): (0.5 - m_screen_center) + 0.5 = principal point
		for (int k = 0; k < 2; ++k) a.screen_center[k] = (0.5f - (1.0f - camera->principal_point[k])) * 1.0f + 0.5f;
		effective_camera_matrix(camera->xform, a.cam);
		NGP_CHECK(camera->lens_mode <= LENS_OPENCV_FISHEYE, "render: unsupported lens mode");
		a.lens_mode = camera->lens_mode;
		for (int k = 0; k < 4; ++k) a.lens[k] = camera->lens_params[k];
		a.near_distance = 0.0f;  // m_render_near_distance (testbed.h:914)
		for (int k = 0; k < 3; ++k) { a.aabb_min[k] = cfg->aabb_min[k]; a.aabb_max[k] = cfg->aabb_max[k]; }
		a.cone_angle_constant = cfg->cone_angle_constant;
		a.max_mip = cfg->max_cascade;
		a.bitfield = bitfield;
		a.sample_index = sample_index;
		a.snap_to_pixel_centers = cfg->snap_to_pixel_centers;
		a.linear_colors = cfg->linear_colors;
		a.rgb_activation = cfg->rgb_activation;
		a.density_activation = cfg->density_activation;
		a.min_transmittance = min_transmittance;
		for (int k = 0; k < 4; ++k) a.background[k] = background_rgba ? background_rgba[k] : 0.f;
		const uint32_t n_px = a.width * a.height;
		const size_t max_q = (size_t)std::max(n_px, 2u * 1024 * 1024) + 256;
		RenderWorkspace ws{};
		const size_t pb = render_payload_bytes();
		ws.payload[0] = r->pay0.get<char>(pb * n_px);
		ws.payload[1] = r->pay1.get<char>(pb * n_px);
		ws.payload_hit = r->payh.get<char>(pb * n_px);
		ws.rgba[0] = r->rgba0.get<float>(4 * (size_t)n_px);
		ws.rgba[1] = r->rgba1.get<float>(4 * (size_t)n_px);
		ws.rgba_hit = r->rgbah.get<float>(4 * (size_t)n_px);
		ws.coords = r->coords.get<float>(7 * max_q);
		ws.out = r->out.get<f16>(16 * max_q);
		ws.frame = r->frame.get<float>(4 * (size_t)n_px);
		ws.counters = r->counters.get<uint32_t>(2);
		if (!r->host_counters) NGP_HIP(hipHostMalloc(&r->host_counters, 16));
		ws.host_counters = r->host_counters;
		a.render_mode = r->render_mode;
		a.depth_scale = r->depth_scale;
		a.show_accel = r->show_accel;
		a.envmap = r->envmap; a.env_w = r->env_w; a.env_h = r->env_h;
		auto infer =[&](uint32_t n, const float* coords, f16* out) {
			check_rc(ngp_inference(model, s, n, coords, 7, out, n, NGP_LAYOUT_SOA, use_inference_params));
		};
		// Normals: tcnn input_gradient's default backprop_scale (128); it reads the inference parameters
		auto grad = [&](uint32_t n, float* coords) {
			check_rc(ngp_input_gradient(model, s, 3, n, coords, 7, coords, 7, 128.0f));
		};
		render_frame(a, spp, ws, infer, out_rgba, s, grad, &r->dist);
	});
}

}  // extern "C"
