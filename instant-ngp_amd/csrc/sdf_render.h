// sdf_render.h — sphere tracing, shading and the IoU counters of the SDF primitive for gfx950.
//
// Re-designs the reference's SphereTracer and Testbed::render_sdf (src/testbed_sdf.cu:47-434, 508-613, 629-1063)
// and compare_signs_kernel / scale_iou_counters_kernel (:474-499). Float arithmetic keeps the reference's
// operation order (-ffp-contract=off), so positions and step counts are reproducible bit for bit from a float32
// restatement given the same distances.
//
// Ray state is a structure of arrays: positions [n x 3] fp32 are the distance function's input with stride 3
// (ngp_inference / ngp_sdf_signed_distance read them in place); direction, pixel index, step count and alive flag
// live in their own arrays; shadow rays carry prev / total / min-visibility arrays and share one direction.
// The network's distance is read straight from the fp16 inference output (NGP_LAYOUT_SOA: row 0 is n contiguous
// halves); the ground-truth path reads fp32 distances.
//
// Differences by design:
//  - compaction takes one atomic per wave and list (64-lane ballot) instead of one per ray; slot order may differ
//    from run to run, every later pass writes through the pixel index, so the image does not;
//  - finished shadow rays write their visibility to the pixel they belong to in the compaction itself
//    (the reference collects them into a third list and scatters afterwards, :291-296, 398-406);
//  - the mesh's signed distance is seeded by the ray's pixel instead of its slot (see DistanceFn);
//  - a ray that misses the box stays where it is (dead) instead of moving FLT_MAX along its direction: no
//    non-finite position ever reaches a distance function. Such rays are dead in the reference as well.
// Not built: octree skipping, slice plane, depth of field, foveation, envmap, hidden-area mask, the ray-traced
// mesh ground truth (ESDFGroundTruthMode::RaytracedMesh) and SDF bricks, EncodingVis.
#pragma once
#include "../../include/ngp_engine.h"
#include "common.h"

#include <functional>

namespace ngp {
namespace sdf {

constexpr float MAX_DEPTH = 16384.0f;  // common_device.cuh:33
enum : uint32_t { MODE_AO = 0, MODE_SHADE = 1, MODE_NORMALS = 2, MODE_POSITIONS = 3, MODE_DEPTH = 4, MODE_COST = 6 };  // ERenderMode
inline bool mode_supported(int m) { return (m >= (int)MODE_AO && m <= (int)MODE_DEPTH) || m == (int)MODE_COST; }

struct Rays {  // one ray list, n_cap entries each
	float* pos;         // [n x 3]
	float* dir;         // [n x 3] (camera rays; shadow rays share FrameArgs::sun_dir)
	uint32_t* idx;      // the ray's pixel (a shadow ray's: the pixel of the camera hit it starts from)
	uint32_t* n_steps;  // camera rays
	uint32_t* alive;
	float* prev;        // shadow rays: previous distance, distance travelled, minimum visibility
	float* total;
	float* min_vis;
};

struct Workspace {
	uint32_t n_cap;      // entries per array (pixels rounded up to the batch granularity)
	Rays rays[2];        // double buffer of the trace
	Rays hit;            // camera rays that ended inside the box (pos, dir, idx, n_steps)
	float* hit_shadow;   // [n_px] by pixel: shadow factor of its hit, 0 occluded .. 1 lit (the reference's rays_hit.distance)
	float* hit_normal;   // [n x 3], unnormalised
	float* fd_pos;       // [6][n_cap x 3] finite-difference taps: +x +y +z -x -y -z
	void* fd_dist;       // [6][n_cap] distances at the taps: f16 (network) or fp32 (ground truth)
	float* dist32;       // [n_cap] ground-truth distances of the current batch
	f16* out16;          // [16 x n_cap] network output, SoA
	float* frame;        // [n_px x 4]
	float* depth;        // [n_px]
	uint32_t* counters;  // device [2]: alive, hits
	uint32_t* host_counters;  // pinned [2]
};

struct FrameArgs {
	uint32_t width, height;
	float focal[2], screen_center[2];
	float cam[12];  // camera-to-world mat4x3 (column-major)
	uint32_t lens_mode;
	float lens[4];
	uint32_t sample_index, snap_to_pixel_centers;
	float aabb_min[3], aabb_max[3];  // m_aabb; the tracer's box is this inflated by zero_offset
	float zero_offset, distance_scale, maximum_distance, fd_normals_epsilon, shadow_sharpness;
	uint32_t analytic_normals, max_iterations;
	float floor_y;                   // get_floor_y() (testbed.h:917)
	float sun_dir[3], up_dir[3];     // normalised on the host, as render_sdf passes them (:1041-1042)
	float brdf[13];                  // BRDFParams (sdf.h:62-72): metallic, subsurface, specular, roughness, sheen,
	                                 // clearcoat, clearcoat_gloss, basecolor[3], ambientcolor[3]
	float background[4];
	uint32_t render_mode;
};

// A distance function writes the distances of n positions (stride 3; n_pad >= n rows are readable): the network's
// into ws.out16 row 0 (fp16), the mesh's into `out32`. `half_out` tells the kernels which one to read. `pixel` [n]
// is each position's pixel: the mesh's sign test is seeded by it (ngp_sdf_signed_distance_rows), so that the distance
// of a ray does not depend on the slot compaction gave it; the network's output does not depend on the row at all.
struct DistanceFn {
	bool half_out;
	std::function<void(uint32_t n, uint32_t n_pad, const float* pos, const uint32_t* pixel, float* out32)> eval;
	// analytic normals (Network::input_gradient, testbed.cu:4621): [n x 3] gradients for n positions; null: none
	std::function<void(uint32_t n_pad, const float* pos, float* normals)> gradient;
};

constexpr uint32_t BATCH_GRANULARITY = 256;  // tcnn::batch_size_granularity, as render_frame pads its batches

// spp samples of one view averaged into out_rgba [h x w x 4] (and out_depth [h x w], nullable)
void render_frame(const FrameArgs& a, uint32_t spp, Workspace& ws, const DistanceFn& fn, float* out_rgba, float* out_depth,
                  hipStream_t s);

// compare_signs_kernel without the octree + scale_iou_counters_kernel (testbed_sdf.cu:474-499)
void iou_accumulate(uint32_t n, const float* distances_ref, const float* distances_model, float scale_existing, uint32_t* counters,
                    hipStream_t s);

}  // namespace sdf
}  // namespace ngp
