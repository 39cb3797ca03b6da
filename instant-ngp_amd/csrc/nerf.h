// nerf.h — NeRF training kernels (sampling, loss + compaction, rollover, occupancy grid) for gfx950.
//
// Re-implements src/testbed_nerf.cu's training kernels without OptiX.
// Difference by design: the reference assigns sample / ray / compacted slots with
// atomicAdd counters, so its sample order is nondeterministic; here slots come from exclusive
// prefix scans in ray order, so the output is deterministic and equal to the reference's as a
// multiset keyed by (ray, step). Counters keep the reference's meaning (totals include rays that
// were dropped for exceeding the sample budget).
#pragma once
#include "../../include/ngp_engine.h"
#include "common.h"
#include "lens.h"

#include <functional>
#include <type_traits>

namespace ngp {
namespace nerf {

constexpr uint32_t GRIDSIZE = 128;                         // NERF_GRIDSIZE (nerf.h:24-30)
constexpr uint32_t GRID_N_CELLS = GRIDSIZE * GRIDSIZE * GRIDSIZE;
constexpr uint32_t CASCADES = 8;                           // NERF_CASCADES (testbed_nerf.cu:59)
constexpr uint32_t STEPS = 1024;                           // NERF_STEPS (:58)
constexpr float SQRT3 = 1.73205080757f;
constexpr float MIN_CONE_STEPSIZE = SQRT3 / STEPS;         // STEPSIZE() (:65-71)
constexpr float MAX_CONE_STEPSIZE = MIN_CONE_STEPSIZE * (1 << (CASCADES - 1)) * STEPS / GRIDSIZE;  // (:76-79)
constexpr uint32_t N_MAX_RANDOM_SAMPLES_PER_RAY = 16;      // (:85-87)
constexpr float MIN_OPTICAL_THICKNESS = 0.01f;             // (:92-94)
constexpr uint32_t BITFIELD_BYTES = GRID_N_CELLS * CASCADES / 8;  // grid_mip_offset(NERF_CASCADES)/8

enum Activation : uint32_t { ACT_NONE = 0, ACT_RELU = 1, ACT_LOGISTIC = 2, ACT_EXP = 3 };
enum LossType : uint32_t { LOSS_L2 = 0, LOSS_L1 = 1, LOSS_MAPE = 2, LOSS_SMAPE = 3, LOSS_HUBER = 4, LOSS_LOGL1 = 5, LOSS_RELL2 = 6 };

struct Camera {          // per image, device side
	uint32_t width, height;
	float focal[2], principal[2];
	float m[12];         // effective camera matrix (rolling-shutter slerp at t=0 applied on the host)
	uint64_t pixel_offset;  // first RGBA8 pixel of this image in the packed image buffer
	uint32_t lens_mode;  // LensMode (lens.h)
	float lens[4];
};

struct Rng { uint64_t state, inc; };  // tcnn::pcg32 state

// EImageDataType (common.h:123-128) with the reference's values: Byte is RGBA8 sRGB with straight alpha (4 bytes a
// texel), Half four fp16 and Float four fp32 (8 and 16 bytes), both linear, premultiplied RGBA
enum ImageType : uint32_t { IMAGE_BYTE = NGP_IMAGE_BYTE, IMAGE_HALF = NGP_IMAGE_HALF, IMAGE_FLOAT = NGP_IMAGE_FLOAT };
inline bool image_type_ok(uint32_t t) { return t >= IMAGE_BYTE && t <= IMAGE_FLOAT; }
inline size_t image_texel_bytes(uint32_t t) { return t == IMAGE_FLOAT ? 16 : t == IMAGE_HALF ? 8 : 4; }
// One image's texels as the kernels' TEX instantiations find them: [height][width] texels of `type` on the device
struct ImageRef {
	const void* data;
	uint32_t type, pad;
};

// Host: effective camera matrix = get_xform_given_rolling_shutter(start == end, t = 0)
// (common_device.cuh:401-408): rotation goes through glm quat_cast / slerp / normalize / mat3_cast. In nerf_abi.hip, as
// is ~Dataset: the dataset is created there.
void effective_camera_matrix(const float xform[12], float out[12]);

struct Dataset {
	uint32_t n_images = 0;
	Camera* d_cams = nullptr;
	uint32_t* d_pixels = nullptr;  // RGBA8 packed, sRGB
	std::vector<Camera> cams;
	std::vector<float> xforms;  // [n_images x 12] the raw (start) transforms, as uploaded after the pixels
	// Depth images (NerfDataset::depthmemory, nerf_loader.cu:943-960): per image fp32 [height][width] on the device or
	// null. The loss pass reads the device array of these pointers, d_depth [n_images], which exists once an image
	// has had depth set; Camera, which is also compiled for the host, keeps its layout.
	std::vector<float*> depth;
	float** d_depth = nullptr;
	uint32_t n_depth = 0;  // images with depth
	// Image types (NerfDataset::pixelmemory / image_data_type per image, nerf_loader.cu:907-1005). A Byte image's texels
	// are its slot of d_pixels, which every image keeps (Camera::pixel_offset stays valid whatever the image's type
	// becomes); a Half or Float image's are an allocation of its own, hdr[i]. d_images [n_images] {pointer, type} exists
	// once an image has been Half or Float; while one is (n_hdr > 0) the sampler and the loss pass run their TEX
	// instantiations, which read it. With n_hdr == 0 nothing of this is read.
	std::vector<uint32_t> types;  // ImageType per image
	std::vector<void*> hdr;       // per image: the Half / Float texels, or null
	ImageRef* d_images = nullptr;
	uint32_t n_hdr = 0;
	uint64_t image_epoch = 0;     // bumped whenever an image's texels change: a trainer discards its prelaunched sampler
	bool tex() const { return n_hdr > 0 && d_images != nullptr; }
	~Dataset();
};

// The error map's CDFs a sampler draws training pixels from (ngp_nerf_error_cdfs; nerf_pixel.h): device floats
// cdf_x_cond_y [n_images][h][w], cdf_y [n_images][h], cdf_img [n_images]. cdf_img null: the image choice stays
// uniform; cdf_x_cond_y null: the position in the image does. All null: the kernels' uniform instantiations run.
struct ErrorCdfs {
	const float* cdf_x_cond_y;
	const float* cdf_y;
	const float* cdf_img;
	uint32_t w, h;
	bool any() const { return cdf_img != nullptr || cdf_x_cond_y != nullptr; }
};

// The lens distortion map a sampler or renderer adds to its rays (distortion.h): device floats [h][w][2], the offset
// of dir.xy at the ray's uv after the lens. data null: none, and the kernels' instantiations without it run.
struct DistMap {
	const float* data;
	uint32_t w, h;
};

struct SampleArgs {
	uint32_t n_rays, ray_offset, n_rays_total_for_image_idx;  // image_idx uses the global ray id
	uint32_t max_samples;
	Rng rng;
	const uint8_t* bitfield;
	uint32_t* ray_indices;     // [n_rays] compacted
	float* rays;               // [n_rays x 6] {o, d} (unnormalized d)
	uint32_t* numsteps;        // [n_rays x 2] {numsteps, base}
	float* coords;             // [max_samples x 7] NerfCoordinate
	uint32_t* counters;        // [2]: rays kept, numsteps total (incl. dropped)
	ErrorCdfs cdfs;            // all null: uniform pixels
};

// the arguments of the count pass's DIST forms
struct SampleArgsDist : SampleArgs {
	DistMap dist;
};

struct LossArgs {
	uint32_t n_rays;           // rays_per_batch (kernel grid); rays kept are counters[0]
	uint32_t n_rays_total_for_image_idx;
	Rng rng;
	uint32_t max_samples_compacted;
	const uint32_t* ray_counter;
	const f16* network_output;  // [n x out_stride] rows 0..2 raw rgb, 3 raw density
	uint32_t out_stride;       // 16 (padded_output_width) or 4 (NGP_LAYOUT_AOS_RGBD)
	const uint32_t* ray_indices;
	const float* rays;
	uint32_t* numsteps;        // in: {numsteps, base}; out: {compacted numsteps, compacted base}
	const float* coords_in;
	float* coords_out;         // [max_samples_compacted x 7]
	f16* dloss_doutput;        // [max_samples_compacted x 16]
	float* loss;               // [n_rays]
	bool zero_loss;            // pass 1 zeroes loss[0, n_rays) (the Testbed step's memset, testbed_nerf.cu:3579)
	uint32_t* compacted_counter;  // [1]
	const float* mean_density;    // [1]
	float loss_scale;
	float bg[3];
	// training error map (testbed_nerf.cu:1869-1899): each compacted ray adds its mean loss, bilinearly
	// split, into [n_images][em_h][em_w] floats; null: off
	float* error_map;
	uint32_t em_w, em_h;
	// optional (null: off): pass 1 stores, per sample it composites, the weight, the transmittance after it and
	// the rgb prefix through it ([5][state_cap] floats, indexed by the pre-compaction sample), and pass 2 reads
	// them instead of compositing each ray again. Same float operations, so the same bits either way.
	float* state;
	uint64_t state_cap;
	// optional (null: off): the loss's compaction scan also publishes the step's counters to host-mapped memory
	// ({ray_counter[0], ray_counter[1], compacted total, 0}, then pub_seq at [4] after a system-scope fence), as soon
	// as they are final: the host sizes the next step while pass 2, the rollover and the training pass run
	volatile uint32_t* pub_host;
	uint32_t pub_seq;
	// the CDFs the rays' pixels were drawn from (the sampler's): pass 1 repeats the draw and divides the loss by its pdf
	ErrorCdfs cdfs;
	// environment map (testbed_nerf.cu:1781-1792, 1988-2011; envmap.h): [env_h][env_w] RGBA floats read by the ray's
	// direction as the background behind cfg's; null: off, and the kernels' instantiations without it run.
	// env_acc (optional): the gradient accumulator (envmap_acc_words64 words, zeroed by the caller) pass 2 deposits
	// into for every ray that kept all of its samples; the gradient's loss is env_loss_type.
	const float* envmap;
	uint32_t env_w, env_h, env_loss_type;
	unsigned long long* env_acc;
	// depth supervision (testbed_nerf.cu:1725-1748, 1848-1856, 1912-1956): with depth_lambda > 0 and a dataset in which
	// an image has depth, the kernels' depth instantiations run: pass 1 also composites the samples' distances from the
	// ray origin, pass 2 adds depth_lambda * dL_depth/d(depth_ray) * (T depth - depth suffix) to the density gradient of
	// rays whose texel has a depth > 0, with the gradient of depth_loss_type. The kept state then has a sixth plane,
	// the depth prefix through the sample ([6][state_cap]). Otherwise nothing of this is read.
	float depth_lambda;
	uint32_t depth_loss_type;
	// per-image exposure (testbed_nerf.cu:1794-1818, 1973-1986): exposure [n_images x 3] log2 exposures,
	// the target's premultiplied linear texel is scaled by 2^exposure per channel; null: off, and the kernels'
	// instantiations without it run. exposure_ray_grad (optional, [n_rays x 3]): pass 1 stores every kept ray's
	// dloss_by_dexposure there, and exposure_gradients (below) sums per image those of the rays that compact to at least
	// one sample; null: the scale is applied but no gradient is taken.
	const float* exposure;
	float* exposure_ray_grad;
};

// The per-image sum of the loss pass's per-ray exposure gradients, without atomics, by k_cam_image_sum's method
// (nerf_camera.h): image_idx is monotone in the ray id under a uniform image choice, so an image's kept rays are one
// contiguous run, found by two binary searches on ray_indices; one block per image adds, in a fixed tree, the rows of
// the rays whose compacted sample count (numsteps[2 r] after the loss pass) is not zero, and one thread per channel adds
// the sum onto image_grad. An image without such rays keeps its accumulator as it is.
struct ExposureGradArgs {
	uint32_t n_rays_cap;        // rows of ray_grad: an upper bound of *ray_counter known on the host
	uint32_t n_rays_total, n_images;
	const uint32_t* ray_counter;
	const uint32_t* ray_indices;
	const uint32_t* numsteps;   // [R x 2] after the loss pass: {compacted numsteps, compacted base}
	const float* ray_grad;      // [n_rays_cap x 3] LossArgs::exposure_ray_grad
	float* image_grad;          // [n_images x 3], accumulated
};
void exposure_gradients(const ExposureGradArgs& a, hipStream_t s);

// The environment map's stand-alone forms (envmap.hip): dirs [n x 3] normalized; texels, weights [n x 4] as
// envmap_lookup returns them; values [n x 3] fp16 rgb gradients added into acc (envmap_acc_words64 words, zeroed by
// the caller); envmap_gradient_f32 converts an accumulator to the fp32 gradient [h x w x 4].
size_t envmap_acc_words64(uint32_t width, uint32_t height);
void envmap_lookup_device(uint32_t w, uint32_t h, uint32_t n, const float* dirs, uint32_t* texels, float* weights, hipStream_t s);
void envmap_lookup_host(uint32_t w, uint32_t h, uint32_t n, const float* dirs, uint32_t* texels, float* weights);
void envmap_deposit_values(uint32_t w, uint32_t h, uint32_t n, const float* dirs, const f16* values, unsigned long long* acc,
                           hipStream_t s);
void envmap_gradient_f32(uint32_t w, uint32_t h, const unsigned long long* acc, float* grad, hipStream_t s);

// The lens distortion map's stand-alone forms (distortion.hip; distortion.h has the lookup and the accumulator): uv
// [n x 2]; texels, weights [n x 4] as distortion_lookup returns them; offsets (optional, with map [h][w][2]) [n x 2] the
// mixed offset. distortion_deposit_rays: one thread per kept ray (at most n_rays_cap, the device counter's value)
// recomputes the ray's uv by training_pixel<false> from its id and the rng, as loss pass 1 does, and adds ray_grad
// [R x 2] by the lookup's weights into acc (distortion_acc_words64 words, zeroed by the caller); numsteps (optional,
// [R x 2]): a ray whose count is 0 deposits nothing, as the reference returns before its deposit. cams: device cameras
// of which width and height are read. distortion_gradient_f32 turns an accumulator into the fp32 gradient [h][w][2]:
// per channel the bins summed in double from the highest down, then (float)(sum g / sum w), 0 where no weight came.
void distortion_lookup_device(uint32_t w, uint32_t h, uint32_t n, const float* uv, uint32_t* texels, float* weights, const float* map,
                              float* offsets, hipStream_t s);
void distortion_lookup_host(uint32_t w, uint32_t h, uint32_t n, const float* uv, uint32_t* texels, float* weights, const float* map,
                            float* offsets);
struct DistDepositArgs {
	uint32_t n_rays_cap, n_rays_total, n_images;
	bool snap;
	Rng rng;
	const Camera* cams;
	const uint32_t* ray_counter;
	const uint32_t* ray_indices;
	const uint32_t* numsteps;   // nullable
	const float* ray_grad;      // [R x 2]
	uint32_t w, h;
	unsigned long long* acc;
};
void distortion_deposit_rays(const DistDepositArgs& a, hipStream_t s);
void distortion_gradient_f32(uint32_t w, uint32_t h, const unsigned long long* acc, float* grad, hipStream_t s);

// The kernels' entry points, by the file that holds them; each kernel there cites the reference kernel it re-implements.

// ---- nerf_sampler.hip ------------------------------------------------------------------------
// Every ray's training pixel (nerf_pixel.h): img [n_rays], uv [n_rays x 2] after snapping, pdf [n_rays x 2] =
// {img_pdf, uv_pdf}. The device form reads the dataset's cameras and device CDFs; the host form makes no GPU call
// (cams: host cameras of which width and height are read, CDFs and outputs in host memory).
void training_pixels(const Dataset& ds, const ngp_nerf_config& cfg, uint32_t n_rays, uint32_t ray_offset, uint32_t n_rays_total, Rng rng,
                     const ErrorCdfs& cdfs, uint32_t* img, float* uv, float* pdf, hipStream_t s);
void training_pixels_host(const Camera* cams, uint32_t n_images, const ngp_nerf_config& cfg, uint32_t n_rays, uint32_t ray_offset,
                          uint32_t n_rays_total, Rng rng, const ErrorCdfs& cdfs, uint32_t* img, float* uv, float* pdf);
// cams (optional): the device cameras to trace instead of the dataset's (a trainer's refined poses)
// dist (optional, data non-null): the distortion map added to every ray's direction (the count pass's DIST forms)
void sample_rays(const Dataset& ds, const ngp_nerf_config& cfg, const SampleArgs& a, uint32_t* tmp_u32, float* tmp_f32, hipStream_t s,
                 const Camera* cams = nullptr, const DistMap* dist = nullptr);
size_t sample_tmp_u32(uint32_t n_rays);  // u32 of sample_rays' tmp_u32 (counts, count-wave sums and prefixes)
size_t sample_tmp_f32(uint32_t n_rays);  // floats of sample_rays' tmp_f32 (stored t per step + ray geometry)

// ---- nerf_loss.hip ---------------------------------------------------------------------------
void compute_loss(const Dataset& ds, const ngp_nerf_config& cfg, const LossArgs& a, uint32_t* tmp_u32, float* tmp_f32, hipStream_t s);
size_t loss_tmp_f32(uint32_t n_rays);    // floats of compute_loss' tmp_f32 (per-ray pass-1 results)
// whether compute_loss runs its depth instantiations, and the floats of tmp_f32 they need (one more per ray)
bool loss_depth_on(const Dataset& ds, const LossArgs& a);
size_t loss_tmp_f32_depth(uint32_t n_rays);
// the floats of the per-ray exposure gradients, which a caller may keep behind those (LossArgs::exposure_ray_grad)
size_t loss_tmp_f32_exposure(uint32_t n_rays);
// construct_cdf_2d / construct_cdf_1d (testbed_nerf.cu:2356-2410) over the error map
void error_map_cdfs(uint32_t n_images, uint32_t w, uint32_t h, const float* data, float* cdf_x_cond_y, float* cdf_y,
                    float* cdf_img, hipStream_t s);
void fill_rollover_f16(uint32_t n_elements, uint32_t stride, const uint32_t* n_input, f16* data, bool rescale, hipStream_t s);
void fill_rollover_f32(uint32_t n_elements, uint32_t stride, const uint32_t* n_input, float* data, hipStream_t s);
void fill_rollover_pair(uint32_t n_elements, const uint32_t* n_input, f16* dloss, uint32_t stride16, float* coords,
                        uint32_t stride32, hipStream_t s);
// What the single-GPU NeRF step does right after the rollover, in the same launch (block 0, thread 0): publish the
// step's counters ctr[0..3] to host-mapped memory (then seq, after a system-scope fence; host null: published
// earlier, by the loss's scan), and write the optimizer control block the training graph reads ({ctl[0] = step,
// ctl[CTL_CFG..] = cfg}, set_device_ctl). bytes: cfg.
struct StepPublish {
	const uint32_t* ctr; volatile uint32_t* host; uint32_t seq;
	uint32_t* ctl; uint32_t step; uint32_t cfg_off, cfg_words; uint32_t cfg[32];  // cfg at ctl + cfg_off (words)
};
void fill_rollover_pair_publish(uint32_t n_elements, const uint32_t* n_input, f16* dloss, uint32_t stride16, float* coords,
                                uint32_t stride32, const StepPublish& pub, hipStream_t s);

// ---- nerf_density_grid.hip -------------------------------------------------------------------
void grid_generate_samples(uint32_t n, Rng rng, uint32_t step, const ngp_nerf_config& cfg, const float* grid_in,
                           uint32_t n_cascades, float thresh, float* positions, uint32_t* indices, uint32_t* mask, hipStream_t s);
size_t grid_mask_words(uint32_t n_cascades);  // u32 of grid_generate_samples' cell mask
void grid_splat_max(uint32_t n, const uint32_t* indices, const f16* density_rm, uint32_t density_activation, float* grid_tmp,
                    hipStream_t s);
// memset(grid_tmp, 0) + grid_splat_max as a counting sort by cell bin: writes all n_cells of grid_tmp; scratch holds
// grid_splat_scratch_u32(n, n_cells) words
size_t grid_splat_scratch_u32(uint32_t n, uint32_t n_cells);
void grid_splat_max_binned(uint32_t n, const uint32_t* indices, const f16* density_rm, uint32_t density_activation,
                           float* grid_tmp, uint32_t n_cells, uint32_t* scratch, hipStream_t s);
// The update's samples in bin order before the density evaluation (which then runs ~1.8x faster on grouped positions):
// grid_sort_samples writes 16-B records (x, y, z, cell within the bin) sorted by 8192-cell bin (order within a bin
// arbitrary; recs: 4 n floats) and keeps the bins' offsets in scratch (grid_sort_scratch_u32 words); the density reads
// the records with stride 4; grid_splat_sorted then writes every cell of grid_tmp from the densities of the sorted
// samples [lo, hi) (density_rm[k - lo]) = memset + splat of those samples.
size_t grid_sort_scratch_u32(uint32_t n, uint32_t n_cells);
void grid_sort_samples(uint32_t n, const float* positions, const uint32_t* indices, uint32_t n_cells, uint32_t* scratch,
                       float* recs, hipStream_t s);
void grid_splat_sorted(uint32_t n_cells, const uint32_t* scratch, const float* recs, const f16* density_rm, uint32_t lo, uint32_t hi,
                       uint32_t density_activation, float* grid_tmp, hipStream_t s);
void grid_ema(uint32_t n, float decay, float* grid, const float* grid_tmp, hipStream_t s);
void grid_mean_bitfield(const float* grid, uint32_t max_cascade, float* mean_out, uint8_t* bitfield, hipStream_t s);
// grid_ema then grid_mean_bitfield in three launches (the density grid update's finalization; n_el >= GRID_N_CELLS)
void grid_ema_mean_bitfield(uint32_t n_el, float decay, float* grid, const float* tmp, uint32_t max_cascade, float* mean_out,
                            uint8_t* bitfield, hipStream_t s);

// ---- nerf_render.hip: rendering (NerfTracer) -------------------------------------------------
struct RenderArgs {
	uint32_t width, height;
	float focal[2], screen_center[2];
	float cam[12];                 // camera-to-world mat4x3 (column-major)
	uint32_t lens_mode;            // render_lens of the training view (testbed.cu:846)
	float lens[4];
	float near_distance;
	float aabb_min[3], aabb_max[3];
	float cone_angle_constant;
	uint32_t max_mip;              // max_cascade
	const uint8_t* bitfield;
	uint32_t sample_index, snap_to_pixel_centers, linear_colors;
	uint32_t rgb_activation, density_activation;
	float min_transmittance;
	float background[4];           // linear rgba
	uint32_t render_mode;          // ERenderMode (common.h:110-121): 0 AO, 1 Shade, 2 Normals, 3 Positions, 4 Depth, 5 Distortion, 9 EncodingVis
	float depth_scale;             // ERenderMode::Depth: 1 / dataset scale (testbed_nerf.cu:2822)
	int32_t show_accel;            // Testbed::Nerf::show_accel (-1 off): the march's minimum mip, alpha 1, Positions by cell
	// environment map (testbed_nerf.cu:2315-2319): the frame is pre-filled per pixel with the map's value in the
	// pixel's ray direction instead of `background`; device [env_h][env_w] RGBA floats, null: off
	const float* envmap;
	uint32_t env_w, env_h;
};
struct RenderArgsDist : RenderArgs {  // the arguments of the DIST forms of k_render_init and k_render_fill_envmap
	DistMap dist;
};
enum : uint32_t { RENDER_AO = 0, RENDER_SHADE = 1, RENDER_NORMALS = 2, RENDER_POSITIONS = 3, RENDER_DEPTH = 4, RENDER_DISTORTION = 5,
                  RENDER_ENCODING_VIS = 9 };
struct RenderWorkspace {
	void* payload[2]; void* payload_hit;
	float* rgba[2]; float* rgba_hit;
	float* coords;                 // [2^21 + 256 x 7]
	f16* out;                      // [16 x (2^21 + 256)] RM
	float* frame;                  // [W*H x 4]
	uint32_t* counters;            // device [2]
	uint32_t* host_counters;       // pinned [2]
};
size_t render_payload_bytes();
// spp samples of one view, averaged into out (linear RGBA [H x W x 4]); infer(n, coords, out_rm)
// evaluates the network on n NerfCoordinates (output RM, row stride n). Normals: grad(n, coords) then
// overwrites the coordinates' position rows with d(density output)/d(position) (Network::input_gradient,
// testbed_nerf.cu:2615-2617). dist (optional, data non-null): the distortion map added to every pixel's ray direction
// after the lens (render_with_lens_distortion), and what ERenderMode::Distortion shows (:2331-2344; without one, zero).
void render_frame(const RenderArgs& a, uint32_t spp, RenderWorkspace& ws,
                  const std::function<void(uint32_t, const float*, f16*)>& infer, float* out, hipStream_t s,
                  const std::function<void(uint32_t, float*)>& grad = nullptr, const DistMap* dist = nullptr);

}  // namespace nerf
}  // namespace ngp
