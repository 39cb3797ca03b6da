/*
 * ngp_engine.h — C-ABI of the MI355X (gfx950) instant-ngp hot-path engine.
 *
 * The engine is a drop-in for the tiny-cuda-nn model/trainer objects the reference's Testbed drives:
 *   tcnn::NetworkWithInputEncoding  (src/testbed.cu:4110, image/SDF primitives)
 *   ngp::NerfNetwork                (include/neural-graphics-primitives/nerf_network.h:77-578)
 *   tcnn::Trainer + Optimizer chain (src/testbed.cu:4129; configs/nerf/base.json:5-22)
 * plus the NeRF training kernels of src/testbed_nerf.cu (ngp_nerf_* below).
 *
 * Conventions
 *  - Plain C types only; half-precision buffers are `void*` holding IEEE binary16.
 *  - Device pointers unless a name says _host. `stream` is a hipStream_t (NULL = default stream).
 *  - Matrices follow tcnn's naming: input  element (i, d) at input[i * input_stride + d] ("CM"/AoS,
 *    the NerfCoordinate layout, nerf.h:85-128); outputs AoS (layout 0: out[i * stride + f]) or
 *    SoA (layout 1: out[f * stride + i], tcnn "RM").
 *  - Errors: every int-returning function returns 0 on success and a negative code on failure;
 *    ngp_last_error() gives the message (the reference throws std::runtime_error /
 *    CUDA_CHECK_THROW, e.g. nerf_network.h:338-340). Handles are not internally synchronised:
 *    one host thread per (device, stream) handle, as the reference's one-stream-per-device Testbed
 *    (testbed.h:989).
 */
#ifndef NGP_ENGINE_H
#define NGP_ENGINE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
#pragma GCC visibility push(default)

typedef struct ngp_model ngp_model;     /* a network: NerfNetwork or NetworkWithInputEncoding */
typedef struct ngp_ctx ngp_ctx;         /* forward context (tcnn::Context, nerf_network.h:566-577) */
typedef struct ngp_trainer ngp_trainer; /* params + gradients + optimizer state (tcnn::Trainer) */

enum { NGP_OK = 0, NGP_ERROR = -1, NGP_INVALID = -2 };
enum { NGP_LAYOUT_AOS = 0, NGP_LAYOUT_SOA = 1 };
/* Engine extension for NerfNetwork inference outputs: only the 4 live rows (raw rgb, raw density) as
 * AoS [n x stride >= 4], skipping the 12 padded outputs of padded_output_width 16 (nerf_network.h:463). */
enum { NGP_LAYOUT_AOS_RGBD = 2 };
enum { NGP_GRAD_OVERWRITE = 0, NGP_GRAD_ACCUMULATE = 1, NGP_GRAD_IGNORE = 2 }; /* tcnn::EGradientMode */

/* ---- library ------------------------------------------------------------------------------ */
const char* ngp_last_error(void);
const char* ngp_version(void);
/* device name and CU count of the current HIP device */
int ngp_device_info(int* cu_count, char* name, size_t name_len);
/* device memory helpers for FFI callers without their own allocator */
int ngp_malloc(void** ptr, size_t bytes);
int ngp_free(void* ptr);
int ngp_memcpy(void* dst, const void* src, size_t bytes, int kind /* hipMemcpyKind */);
int ngp_stream_synchronize(void* stream);
/* per-kernel HIP-event timing on each kernel's launch stream (off by default). read() fills a JSON
 * object {"phase": {"calls": n, "ms": total}} and returns the length needed (incl. NUL). */
int ngp_profiler_enable(int enable);
int ngp_profiler_reset(void);
int ngp_profiler_read(char* json_buf, size_t len);
/* Verification (engine extension): the device forms of the shared math (csrc/ngp_math.h) against the reference
 * operations they replace, over the whole input range, on the GPU. which 0: ngp_div_2pf (the logf's f / (2 + f),
 * reciprocal + Newton + residual step) against the IEEE quotient for all 2^23 reduced arguments. *mismatches =
 * the number of inputs whose results differ in any bit (0 is the contract the sampler's bit-exactness rests on). */
int ngp_debug_math_check(int which, void* stream, uint64_t* mismatches);

/* ---- models (tcnn::Network<float, __half> surface) ------------------------------------------ */
/* NerfNetwork ctor (nerf_network.h:81-112); JSON strings are the config sections the Testbed passes
 * (src/testbed.cu:4029-4042: "encoding", "dir_encoding", "network", "rgb_network").
 * The position encoding is tcnn's grid: "otype" HashGrid | DenseGrid | Grid (with "type" Hash | Dense), "n_levels",
 * "n_features_per_level" (1, 2, 4, 8), "log2_hashmap_size", "base_resolution", "per_level_scale", and
 * "interpolation": "Linear" (default) or "Smoothstep" (tcnn InterpolationType; matched without case). Smoothstep
 * forms every corner weight from s(f) = f^2 (3 - 2f) of the cell fraction f and multiplies the input gradient's
 * term of dimension d by s'(f_d) = 6 f_d (1 - f_d), which makes the encoding C1 across cell faces. "Nearest" is
 * refused. ngp_model_query "grid_interpolation" reads the mode back (0 Linear, 1 Smoothstep). */
int ngp_nerf_network_create(uint32_t n_pos_dims, uint32_t n_dir_dims, uint32_t n_extra_dims, uint32_t dir_offset,
                            const char* pos_encoding_json, const char* dir_encoding_json,
                            const char* density_network_json, const char* rgb_network_json, ngp_model** out);
/* tcnn::NetworkWithInputEncoding(n_input_dims, n_output_dims, encoding, network) (src/testbed.cu:4101-4110) */
int ngp_network_with_input_encoding_create(uint32_t n_input_dims, uint32_t n_output_dims, const char* encoding_json,
                                           const char* network_json, ngp_model** out);
void ngp_model_destroy(ngp_model* m);

uint64_t ngp_model_n_params(const ngp_model* m);           /* n_params()            nerf_network.h:459 */
uint64_t ngp_model_n_matrix_params(const ngp_model* m);    /* sum of layer_sizes()  nerf_network.h:483, testbed.cu:3834-3846 */
uint32_t ngp_model_input_width(const ngp_model* m);        /* input_width()         nerf_network.h:467 */
uint32_t ngp_model_padded_output_width(const ngp_model* m);/* padded_output_width() nerf_network.h:463 */
uint32_t ngp_model_output_width(const ngp_model* m);       /* output_width()        nerf_network.h:471 */

/* Parameter layout: [density MLP | rgb MLP | position grid | dir encoding] (nerf_network.h:430-443);
 * NetworkWithInputEncoding: [MLP | grid]. Grid level offsets in entries (GridEncoding
 * level_params_offset / level_n_params, src/testbed.cu:4849-4856). */
typedef struct {
	uint64_t density_mlp_offset, density_mlp_params;
	uint64_t rgb_mlp_offset, rgb_mlp_params;
	uint64_t grid_offset, grid_params;
	uint32_t grid_dims, grid_levels, grid_features, grid_log2_hashmap, grid_base_resolution;
	float grid_per_level_scale;
	uint32_t grid_level_offsets[33]; /* entries; params = entries * grid_features */
	uint32_t grid_resolution[32];
	float grid_scale[32];
	uint32_t encoding_width;         /* padded encoding output width (density MLP input) */
} ngp_param_layout;
int ngp_model_param_layout(const ngp_model* m, ngp_param_layout* out);

/* set_params(params, inference_params, gradients) (nerf_network.h:430): fp16 device buffers of n_params */
int ngp_model_set_params(ngp_model* m, void* params, void* inference_params, void* gradients);
/* initialize_params(rnd, params_full_precision, scale) (nerf_network.h:445-457), host fp32 buffer */
int ngp_model_initialize_params(const ngp_model* m, uint64_t seed, float* params_full_precision_host, float scale);
/* GridEncoding::set_max_level / set_max_level_gpu (src/testbed.cu:3856-3864; testbed_nerf.cu:3996,4004) */
int ngp_model_set_max_level(ngp_model* m, float max_level, const float* max_level_per_sample);
/* engine knobs: "grid_backward_mode" = 0 auto, 1 direct packed-f16 atomics (tcnn-style),
 * 3 destination-bucketed exact sums (auto picks 3 for n >= 4096); "grid_bricks" (bucketed backward: dense
 * levels summed per brick where that moves fewer bytes, default 0); "fuse_infer", "fused_hist",
 * "fuse_slabs", "fuse_opt", "fuse_mlp_opt", "overlap", "win_debug"  */
int ngp_model_set_option(ngp_model* m, const char* key, double value);
/* engine state for tests and tools: "grid_brick_levels" = how many dense levels the bucketed backward sums
 * per brick in its plan for the last batch size (0: all levels through items); "grid_direct_levels",
 * "grid_direct_part", "grid_plan_inline" likewise describe that plan; "grid_interpolation" = the encoding's
 * interpolation (0 Linear, 1 Smoothstep); "fused_inference" = 1 when ngp_inference encodes inside the MLP kernel */
int ngp_model_query(const ngp_model* m, const char* key, double* value);
/* pre-size internal workspaces for batches up to n (lets callers capture steps into HIP graphs) */
int ngp_model_reserve(ngp_model* m, uint32_t n);
/* Inspection of the last training pass's intermediates (the role of tcnn's forward_activations(ctx),
 * nerf_network.h:502-507): "encoding" = fp16 AoS [n x encoding_width] grid output of the last unfused
 * forward, "dL_dencoding" = fp16 AoS [n x encoding_width] input of the grid backward, "dL_dsh" = fp16
 * [n x 16] dL/d(SH encoding) of the last backward with input gradients, "dw_slabs" = the fp32 per-block
 * MLP weight-gradient partial sums. Device pointer
 * valid until the next call that grows the workspace. */
int ngp_model_workspace(ngp_model* m, const char* name, void** ptr, uint64_t* bytes);
/* Counts workspace reallocations. A graph from ngp_trainer_capture_training_step holds workspace
 * pointers: ngp_graph_launch fails (instead of touching freed memory) once the epoch moved past the
 * capture's; callers re-capture when it changes. */
uint64_t ngp_model_workspace_epoch(const ngp_model* m);

/* inference_mixed_precision (nerf_network.h:116-174): output fp16 [n x padded_output_width] */
int ngp_inference(ngp_model* m, void* stream, uint32_t n, const float* input, uint32_t input_stride, void* output,
                  uint32_t output_stride, uint32_t output_layout, int use_inference_params);
/* NerfNetwork::density (nerf_network.h:337-353): density MLP output fp16 [n x 16] */
int ngp_density(ngp_model* m, void* stream, uint32_t n, const float* input, uint32_t input_stride, void* output,
                uint32_t output_stride, uint32_t output_layout, int use_inference_params);
/* forward_impl (nerf_network.h:179-254) -> context; output may be NULL */
int ngp_forward(ngp_model* m, void* stream, uint32_t n, const float* input, uint32_t input_stride, void* output,
                uint32_t output_stride, int use_inference_params, ngp_ctx** ctx);
/* backward_impl (nerf_network.h:256-335): param gradients into the gradient buffer given to set_params
 * (grad_mode NGP_GRAD_IGNORE: untouched). dL_dinput (nullable, the reference's `GPUMatrixDynamic<float>*
 * dL_dinput`): fp32 AoS [n x dL_dinput_stride]; rows 0..n_pos_dims-1 receive dL/dposition through the
 * grid encoding, a NerfNetwork's rows dir_offset..+2 dL/ddirection through the SH encoding
 * (nerf_network.h:282-299, 317-333); other rows are not written. A context from a forward with
 * use_inference_params runs the backward on the inference (EMA) parameters too (backward_impl's
 * use_inference_params, nerf_network.h:256-335). */
int ngp_backward(ngp_model* m, void* stream, ngp_ctx* ctx, const void* dL_doutput, uint32_t dL_stride, float* dL_dinput,
                 uint32_t dL_dinput_stride, int grad_mode);
void ngp_ctx_destroy(ngp_ctx* ctx);
/* NerfNetwork::density_forward (nerf_network.h:355-382) -> context; output (nullable): the density
 * network's fp16 output AoS [n x output_stride] (16 rows) */
int ngp_density_forward(ngp_model* m, void* stream, uint32_t n, const float* input, uint32_t input_stride, void* output,
                        uint32_t output_stride, int use_inference_params, ngp_ctx** ctx);
/* NerfNetwork::density_backward (nerf_network.h:384-428): dL_doutput = dL/d(density network output),
 * fp16 AoS [n x dL_stride] (16 rows, stride a multiple of 4). Gradients of the density MLP and the grid
 * (the rgb MLP's are left as they are); dL_dinput as in ngp_backward (position rows only). */
int ngp_density_backward(ngp_model* m, void* stream, ngp_ctx* ctx, const void* dL_doutput, uint32_t dL_stride, float* dL_dinput,
                         uint32_t dL_dinput_stride, int grad_mode);
/* tcnn Network::input_gradient(stream, dim, input, d_dinput, backprop_scale) — the reference's normals
 * (testbed_nerf.cu:2616, dim 3 = density; testbed.cu:4621, SDF dim 0): forward, backward of a one-hot
 * dL/doutput (row `dim` = backprop_scale) with parameter gradients ignored, result / backprop_scale.
 * d_dinput fp32 AoS [n x d_dinput_stride] (may alias `input` with the same stride, as the reference
 * passes positions_matrix for both: only the position/direction rows are written, after every read). */
int ngp_input_gradient(ngp_model* m, void* stream, uint32_t dim, uint32_t n, const float* input, uint32_t input_stride,
                       float* d_dinput, uint32_t d_dinput_stride, float backprop_scale);
/* fused training pass = forward_impl + backward_impl (src/testbed_nerf.cu:4077-4078) in one call */
int ngp_forward_backward(ngp_model* m, void* stream, uint32_t n, const float* input, uint32_t input_stride, void* output,
                         uint32_t output_stride, const void* dL_doutput, uint32_t dL_stride, int grad_mode);

/* Raw position-encoding access (tcnn GridEncoding forward / backward). out fp16 [n x encoding_width]. */
int ngp_encoding_forward(ngp_model* m, void* stream, uint32_t n, const float* input, uint32_t input_stride, void* output,
                         uint32_t output_stride, uint32_t output_layout, int use_inference_params);
/* dL_dinput (nullable; needs dL_layout AoS): fp32 [n x dL_dinput_stride], rows 0..n_pos_dims-1 */
int ngp_encoding_backward(ngp_model* m, void* stream, uint32_t n, const float* input, uint32_t input_stride,
                          const void* dL_doutput, uint32_t dL_stride, uint32_t dL_layout, float* dL_dinput,
                          uint32_t dL_dinput_stride, int grad_mode);

/* ---- trainer (tcnn::Trainer<float, __half, __half>, src/testbed.cu:4129) -------------------- */
/* optimizer_json: the "optimizer" config section (Ema / ExponentialDecay / Adam nesting).
 * Allocates fp32 master params, fp16 params / inference(EMA) params / gradients and Adam state,
 * initialises parameters from `seed` (default_rng_t, src/testbed.cu:3906) and calls set_params. */
int ngp_trainer_create(ngp_model* m, const char* optimizer_json, uint64_t seed, ngp_trainer** out);
void ngp_trainer_destroy(ngp_trainer* t);
/* Trainer::optimizer_step(stream, loss_scale) (src/testbed_nerf.cu:3678) */
int ngp_trainer_optimizer_step(ngp_trainer* t, void* stream, float loss_scale);
void* ngp_trainer_gradients(ngp_trainer* t);               /* fp16 [n_params], the DP all-reduce buffer */
/* 1 when the gradient buffer holds the last training pass's whole gradient. 0 after a step whose backward did
 * not write it: the grid's optimizer update fused into the backward (ngp_trainer_fused_update_active, captured
 * or training_step steps on the lazy layout) or the sharded data-parallel step, whose backward stores the
 * gradient as fp32 for the reduce-scatter. The buffer then holds an older gradient. ngp_forward_backward and
 * steps without the fused update write it again (engine extension; tcnn's gradients() is always current) */
int ngp_trainer_gradients_valid(const ngp_trainer* t);
void* ngp_trainer_params(ngp_trainer* t);                  /* fp16 [n_params] */
void* ngp_trainer_inference_params(ngp_trainer* t);        /* fp16 [n_params] (EMA when configured) */
/* fp32 [n_params]; large-table trainers keep the master weights in their optimizer records and refresh this
   mirror on each call (synchronizes the device; NULL + ngp_last_error on failure). For those trainers the
   buffer is read-only: writes into it never reach training or serialize (which reads the records); change
   weights with ngp_trainer_set_params_full_precision. For eager-layout trainers it is the live master copy. */
float* ngp_trainer_params_full_precision(ngp_trainer* t);
uint32_t ngp_trainer_step(const ngp_trainer* t);
uint64_t ngp_trainer_n_params(const ngp_trainer* t);
float ngp_trainer_learning_rate(const ngp_trainer* t);     /* optimizer->learning_rate() (testbed_nerf.cu:3771) */
int ngp_trainer_set_learning_rate(ngp_trainer* t, float lr);
/* Engine extension: trainer options. "ema_closed_form" 0 (default) / 1: how the large-table (lazy-EMA) layout
 * applies the EMA steps a skipped parameter owes: exact replay to the recurrence's fixed point, bit for bit the
 * per-step Ema of tcnn's chain (configs/nerf/base.json:5-8), or a closed form past 32 steps (within 1 fp16 ulp).
 * "shard_opt" 1 (default) / 0: the sharded optimizer under ngp_trainer_set_data_parallel (see there). */
int ngp_trainer_set_option(ngp_trainer* t, const char* key, double value);
/* set_params_full_precision (src/testbed.cu:4146): host fp32 -> master, fp16 params and inference params */
int ngp_trainer_set_params_full_precision(ngp_trainer* t, const float* params_host, uint64_t n);
/* serialize / deserialize (src/testbed.cu:4874,5040): flat little-endian blob, size query with buf=NULL */
int ngp_trainer_serialize(ngp_trainer* t, void* buf_host, uint64_t* size);
int ngp_trainer_deserialize(ngp_trainer* t, const void* buf_host, uint64_t size);

/* Engine extension (no reference counterpart): capture n_steps of {forward_backward(input, dL/doutput)
 * [+ optimizer_step(loss_scale) if with_optimizer]} on `stream` (not the null stream) into one HIP
 * graph, replayed by ngp_graph_launch. Inputs are read from the captured device pointers at every
 * launch. The optimizer step counter lives on the device, so replays follow the same learning-rate/EMA
 * schedule as eager steps. For launch-bound training loops (one launch instead of ~15 per step). */
typedef struct ngp_graph ngp_graph;
int ngp_trainer_capture_training_step(ngp_trainer* t, void* stream, uint32_t n, const float* input, uint32_t input_stride,
                                      const void* dL_doutput, uint32_t dL_stride, float loss_scale, uint32_t n_steps,
                                      int with_optimizer, ngp_graph** out);
/* Engine extension: ONE step of exactly what a captured step runs, launched eagerly: forward_backward
 * (with the grid's lazy update fused into the backward when ngp_trainer_fused_update_active), the
 * trainer's gradient exchange hook if set (ngp_trainer_set_allreduce), then optimizer_step(loss_scale x
 * world). The per-kernel profile of this call is the profile of a replayed graph step. */
int ngp_trainer_train_step(ngp_trainer* t, void* stream, uint32_t n, const float* input, uint32_t input_stride,
                           const void* dL_doutput, uint32_t dL_stride, float loss_scale);
/* 1 when a training step of n_batch samples runs the grid's optimizer update inside the backward (lazy-EMA
 * layout, model option fuse_opt, no exchange hook): the grid part of the gradient buffer is then not written. */
int ngp_trainer_fused_update_active(const ngp_trainer* t, uint32_t n_batch);
int ngp_graph_launch(ngp_graph* g, void* stream);
void ngp_graph_destroy(ngp_graph* g);

typedef struct { uint64_t state, inc; } ngp_rng; /* tcnn::pcg32 state (default_rng_t) */

/* ---- losses and the generic training step (tcnn::Trainer::training_step) ------------------- */
/* tcnn Loss otypes as named in the configs (configs/image/base.json:2-4 "L2", configs/sdf/base.json
 * "MAPE"): value = l(pred, target) / (n * dims), gradient = loss_scale * dl/dpred / (n * dims) rounded
 * to fp16; output columns >= dims get a zero gradient. */
enum { NGP_LOSS_L2 = 0, NGP_LOSS_L1 = 1, NGP_LOSS_MAPE = 2, NGP_LOSS_SMAPE = 3, NGP_LOSS_RELATIVE_L2 = 4 };
/* output fp16 AoS [n x output_stride], target fp32 AoS [n x target_stride], dL_doutput fp16 AoS;
 * values (optional, device [n]): per-sample loss; loss_sum (optional, device scalar): += total */
int ngp_loss_evaluate(int loss_type, void* stream, uint32_t n, uint32_t dims, const void* output, uint32_t output_stride,
                      const float* target, uint32_t target_stride, float loss_scale, void* dL_doutput, uint32_t dL_stride,
                      float* values, float* loss_sum);
/* tcnn::Trainer::training_step(stream, input, target, data_pdf = nullptr, run_optimizer)
 * (src/testbed_image.cu:276, src/testbed_sdf.cu:1304): forward, loss over the model's output_width
 * columns, backward into the gradient buffer (overwrite) and, if run_optimizer, optimizer_step. With
 * run_optimizer on the lazy-EMA layout and model option "fuse_opt" (default), the grid's update runs
 * inside the backward (bit-identical) and the grid part of the gradient buffer is not written. */
int ngp_trainer_training_step(ngp_trainer* t, void* stream, uint32_t n, const float* input, uint32_t input_stride,
                              const float* target, uint32_t target_stride, int loss_type, float loss_scale, int run_optimizer,
                              float* loss_sum);

/* ---- image primitive (BASELINE C1; src/testbed_image.cu) -------------------------------------- */
typedef struct ngp_image ngp_image;
enum { NGP_IMAGE_RANDOM = 0, NGP_IMAGE_STRATIFIED = 3 };  /* ERandomMode (common.h:124-130) */
typedef struct {
	uint32_t random_mode;            /* Stratified (testbed.h:875) */
	uint32_t snap_to_pixel_centers;  /* 1 (testbed.h:871) */
	uint32_t linear_colors;          /* 0 (testbed.h:872): targets are sRGB-encoded */
} ngp_image_config;
int ngp_image_default_config(ngp_image_config* out);
/* texture: RGBA fp32 [height x width x 4] in linear colours (EDataType::Float, e.g. albert.exr) */
int ngp_image_create(uint32_t width, uint32_t height, const float* rgba_host, ngp_image** out);
void ngp_image_destroy(ngp_image* img);
/* generate_training_data of Testbed::train_image (testbed_image.cu:223-265): generate_random_uniform
 * (advances *rng by 2n), stratify2_kernel (:62-76), eval_image_kernel_and_snap<float, 3> (:167-212).
 * positions [n x 2], targets [n x 3] (device). */
int ngp_image_generate_training_samples(const ngp_image* img, void* stream, uint32_t n, ngp_rng* rng, const ngp_image_config* cfg,
                                        float* positions, float* targets);
/* Testbed::train_image (testbed_image.cu:214-285): samples, training_step (L2, no optimizer), optimizer_step(128) */
int ngp_image_train_step(ngp_image* img, ngp_trainer* t, void* stream, uint32_t batch, ngp_rng* rng, const ngp_image_config* cfg,
                         float* loss_sum);

/* ---- SDF primitive (BASELINE C5; src/testbed_sdf.cu) ------------------------------------------ */
typedef struct ngp_sdf_mesh ngp_sdf_mesh;
/* triangles [n x 9] already normalised to the unit cube (Testbed::load_mesh, testbed_sdf.cu:1120-1150);
 * builds the surface-area CDF (triangle_distribution, :1167-1175) */
int ngp_sdf_mesh_create(uint32_t n_triangles, const float* tris_host, ngp_sdf_mesh** out);
void ngp_sdf_mesh_destroy(ngp_sdf_mesh* m);
/* the mesh's triangles in the order the BVH build left them (TriangleBvh4::build reorders
 * m_sdf.triangles_cpu, testbed_sdf.cu:1157; the surface CDF follows that order): [n x 9] host floats */
int ngp_sdf_mesh_triangles(const ngp_sdf_mesh* m, float* tris_out);
/* host-only TriangleBvh4::build (triangle_bvh.cu:540-617) for inspection: reorders tris [n x 9] in place
 * and writes the nodes, 32 bytes each {float lo[3], hi[3]; int32 left, right} (negative = leaf
 * triangle range [-left-1, -right-1)). nodes_out = NULL: *n_nodes = the node count, tris untouched. */
int ngp_sdf_bvh_build(float* tris, uint32_t n_triangles, uint32_t n_primitives_per_leaf, void* nodes_out, uint32_t* n_nodes);
/* generate_training_samples_sdf (testbed_sdf.cu:1187-1275), non-octree branch: n/8 * {4 on the surface,
 * 3 surface + logistic offset, 1 uniform in aabb}; n must be a multiple of 8; advances *rng by
 * 3n + 3 * (3n/8). Signed distances by brute force over the triangles (the BVH is SURVEY §8f). */
int ngp_sdf_generate_training_samples(ngp_sdf_mesh* m, void* stream, uint32_t n, ngp_rng* rng, const float* aabb_min,
                                      const float* aabb_max, float stddev, float* positions, float* distances);
/* signed_distance_raystab semantics (triangle_bvh.cu:415-433) over every triangle */
int ngp_sdf_signed_distance(ngp_sdf_mesh* m, void* stream, uint32_t n, const float* positions, float* distances);
/* The same with the index that seeds each point's stab rays given in rows (device [n]) instead of taken from the
 * point's place in the batch (the reference jitters the 32 rays of point i by rng.advance(2 i), triangle_bvh.cu:691-695;
 * a ray can slip between two triangles, so the sign of a point close inside the surface depends on that index about
 * once in a million). ngp_sdf_signed_distance(positions) == ngp_sdf_signed_distance_rows(positions, rows = 0..n-1).
 * The sphere tracer passes each ray's pixel, so its ground-truth view does not depend on how rays are compacted. */
int ngp_sdf_signed_distance_rows(ngp_sdf_mesh* m, void* stream, uint32_t n, const float* positions, const uint32_t* rows,
                                 float* distances);
/* shuffle<vec3> / shuffle<float> (testbed_sdf.cu:1295-1296): a bijection seeded by the training step */
int ngp_sdf_shuffle(void* stream, uint32_t n, uint32_t seed, const float* positions, const float* distances,
                    float* positions_shuffled, float* distances_shuffled);
/* Testbed::train_sdf (testbed_sdf.cu:1289-1312): shuffle, training_step (MAPE, loss scale 128, optimizer) */
int ngp_sdf_train_step(ngp_trainer* t, void* stream, uint32_t n, const float* positions, const float* distances, uint32_t step,
                       float* positions_shuffled, float* distances_shuffled, float* loss_sum);

/* ---- NeRF training kernels (src/testbed_nerf.cu), without OptiX --------------------------- */
typedef struct ngp_nerf_dataset ngp_nerf_dataset;  /* training images on device + cameras */
typedef struct ngp_nerf_trainer ngp_nerf_trainer;  /* Testbed NeRF training state (grid, counters, rng) */

/* One training image (TrainingImageMetadata, nerf_loader.h; xform after nerf_matrix_to_ngp):
 * camera-to-world mat4x3, column-major {x axis, y axis, z axis, origin}. */
typedef struct {
	uint32_t width, height;
	float focal_length[2];
	float principal_point[2];
	float xform[12];
	uint32_t lens_mode;      /* Lens (common_device.cuh:288-378, nerf_loader.cu:160-224): 0 perspective,
	                            1 OpenCV {k1, k2, p1, p2}, 2 OpenCV fisheye {k1, k2, k3, k4} */
	float lens_params[4];
} ngp_nerf_image;

/* Training knobs with the reference defaults (testbed.h:716-785; load_nerf_post testbed_nerf.cu:3093-3109). */
typedef struct {
	float aabb_min[3], aabb_max[3];   /* m_aabb */
	float cone_angle_constant;        /* 0 when aabb_scale <= 1, else 1/256 */
	uint32_t max_cascade;             /* ceil(log2(aabb_scale)) */
	uint32_t snap_to_pixel_centers;   /* 1 */
	uint32_t random_bg_color;         /* 1 */
	uint32_t linear_colors;           /* 0 */
	uint32_t color_space_linear;      /* 1 (m_color_space = Linear) */
	float background_color[3];        /* 0 */
	uint32_t rgb_activation;          /* 0 None, 1 ReLU, 2 Logistic, 3 Exponential; default 3 */
	uint32_t density_activation;      /* default 3 */
	uint32_t loss_type;               /* 0 L2, 1 L1, 2 MAPE, 3 SMAPE, 4 Huber, 5 LogL1, 6 RelativeL2; base.json: Huber */
	float near_distance;              /* 0.1 */
	uint32_t target_batch_size;       /* 2^18 */
} ngp_nerf_config;


typedef struct {
	uint32_t step, rays_per_batch, measured_batch_size, measured_batch_size_before_compaction;
	float loss;
} ngp_nerf_stats;

int ngp_nerf_default_config(float aabb_scale, ngp_nerf_config* out);
/* images: RGBA8 sRGB (EImageDataType::Byte; 0x00FF00FF marks masked pixels, common_device.cuh:893) */
int ngp_nerf_dataset_create(uint32_t n_images, const ngp_nerf_image* images, const void* const* rgba8_host,
                            ngp_nerf_dataset** out);
void ngp_nerf_dataset_destroy(ngp_nerf_dataset* ds);

/* generate_training_samples_nerf (testbed_nerf.cu:1382-1658); deterministic slots (prefix scans).
 * rays: [n_rays x 6] {o, d}; numsteps: [n_rays x 2] {n, base}; coords: [max_samples x 7];
 * counters: [2] = {rays kept, total steps incl. dropped rays}. */
int ngp_nerf_generate_training_samples(const ngp_nerf_dataset* ds, const ngp_nerf_config* cfg, void* stream,
                                       uint32_t n_rays, uint32_t ray_offset, uint32_t n_rays_total, ngp_rng rng,
                                       uint32_t max_samples, const uint8_t* bitfield, uint32_t* ray_indices, float* rays,
                                       uint32_t* numsteps, float* coords, uint32_t* counters);
/* compute_loss_kernel_train_nerf (testbed_nerf.cu:1660-2012): composite, loss, compaction, dL/doutput */
int ngp_nerf_compute_loss(const ngp_nerf_dataset* ds, const ngp_nerf_config* cfg, void* stream, uint32_t n_rays,
                          uint32_t n_rays_total, ngp_rng rng, uint32_t max_samples_compacted, const uint32_t* ray_counter,
                          const void* network_output, const uint32_t* ray_indices, const float* rays, uint32_t* numsteps,
                          const float* coords_in, float* coords_out, void* dloss_doutput, float* loss,
                          uint32_t* compacted_counter, const float* mean_density, float loss_scale);
/* The same with the training error map (testbed_nerf.cu:1869-1899, the kernel's error_map argument): every
 * compacted ray adds its mean loss, split bilinearly around uv * res - 0.5, into error_map
 * [n_images][em_height][em_width] (device floats, float atomics as in the reference). */
/* Engine extension: ngp_nerf_compute_loss with pass 1 keeping each composited sample's state (weight, transmittance
 * after it, rgb prefix through it) in sample_state ([5][state_capacity] floats, indexed like the samples: state_capacity
 * at least the sample buffer's length) for pass 2, which then does not composite each ray again. The same float
 * operations: outputs equal ngp_nerf_compute_loss's bit for bit. The training step uses this form. */
int ngp_nerf_compute_loss_state(const ngp_nerf_dataset* ds, const ngp_nerf_config* cfg, void* stream, uint32_t n_rays,
                                uint32_t n_rays_total, ngp_rng rng, uint32_t max_samples_compacted, const uint32_t* ray_counter,
                                const void* network_output, const uint32_t* ray_indices, const float* rays, uint32_t* numsteps,
                                const float* coords_in, float* coords_out, void* dloss_doutput, float* loss,
                                uint32_t* compacted_counter, const float* mean_density, float loss_scale, float* sample_state,
                                uint64_t state_capacity);
int ngp_nerf_compute_loss_error_map(const ngp_nerf_dataset* ds, const ngp_nerf_config* cfg, void* stream, uint32_t n_rays,
                                    uint32_t n_rays_total, ngp_rng rng, uint32_t max_samples_compacted,
                                    const uint32_t* ray_counter, const void* network_output, const uint32_t* ray_indices,
                                    const float* rays, uint32_t* numsteps, const float* coords_in, float* coords_out,
                                    void* dloss_doutput, float* loss, uint32_t* compacted_counter, const float* mean_density,
                                    float loss_scale, float* error_map, uint32_t em_width, uint32_t em_height);
/* Error-driven ray sampling (Training::sample_focal_plane_proportional_to_error / sample_image_proportional_to_error,
 * testbed.h:733-734; sample_cdf_2d and image_idx, testbed_nerf.cu:1232-1338). The CDFs of a closed error map window
 * as the trainer builds them (ngp_nerf_trainer_error_map): DEVICE floats cdf_x_cond_y [n_images][height][width], cdf_y
 * [n_images][height], cdf_img [n_images]. cdf_img NULL leaves the image choice uniform; cdf_x_cond_y NULL leaves the
 * position in the image uniform (cdf_y, width and height are then not looked at; with it they are required). A ray's
 * image is the first entry of cdf_img not below ld_random_val(global ray index, 0xdeadbeef); half of the positions
 * (first pcg float below 0.5) stay uniform, the other half pick a cell by cdf_y then cdf_x_cond_y and a uniform point
 * in it. img_pdf = pmf_img * n_images, uv_pdf = pmf_x * pmf_y * width * height, both 1 where the choice was uniform.
 * Every search result is clamped to the last entry, so no load leaves its CDF row whatever the entries are. */
typedef struct {
	const float* cdf_x_cond_y;
	const float* cdf_y;
	const float* cdf_img;
	uint32_t width, height;
} ngp_nerf_error_cdfs;
/* ngp_nerf_generate_training_samples with the rays' pixels drawn from cdfs. cdfs NULL, or with every pointer NULL:
 * the same kernels and the same bytes as ngp_nerf_generate_training_samples. */
int ngp_nerf_generate_training_samples_cdf(const ngp_nerf_dataset* ds, const ngp_nerf_config* cfg, void* stream,
                                           uint32_t n_rays, uint32_t ray_offset, uint32_t n_rays_total, ngp_rng rng,
                                           uint32_t max_samples, const uint8_t* bitfield, uint32_t* ray_indices, float* rays,
                                           uint32_t* numsteps, float* coords, uint32_t* counters,
                                           const ngp_nerf_error_cdfs* cdfs);
/* ngp_nerf_compute_loss_error_map (error_map nullable) for rays sampled with cdfs: every channel's loss is divided by
 * img_pdf * uv_pdf before the mean (testbed_nerf.cu:1846), so loss[] and the error map deposit are; dL/doutput is not
 * (the reference keeps that line commented out, :1858-1862: importance sampling is meant to reweight the loss). */
int ngp_nerf_compute_loss_cdf(const ngp_nerf_dataset* ds, const ngp_nerf_config* cfg, void* stream, uint32_t n_rays,
                              uint32_t n_rays_total, ngp_rng rng, uint32_t max_samples_compacted, const uint32_t* ray_counter,
                              const void* network_output, const uint32_t* ray_indices, const float* rays, uint32_t* numsteps,
                              const float* coords_in, float* coords_out, void* dloss_doutput, float* loss,
                              uint32_t* compacted_counter, const float* mean_density, float loss_scale, float* error_map,
                              uint32_t em_width, uint32_t em_height, const ngp_nerf_error_cdfs* cdfs);
/* Engine extension (inspection): the training pixel of rays [ray_offset, ray_offset + n_rays) of a batch of
 * n_rays_total, as the sampler and the loss pass draw it (one shared function): img [n_rays], uv [n_rays x 2] after
 * snapping, pdf [n_rays x 2] = {img_pdf, uv_pdf}; device memory. */
int ngp_nerf_training_pixels(const ngp_nerf_dataset* ds, const ngp_nerf_config* cfg, void* stream, uint32_t n_rays,
                             uint32_t ray_offset, uint32_t n_rays_total, ngp_rng rng, const ngp_nerf_error_cdfs* cdfs,
                             uint32_t* img, float* uv, float* pdf);
/* The same function compiled for the host: the CDFs and the outputs are HOST memory and no GPU call is made. A dataset
 * lives on the device, so the images (of which width and height are read) come as the array a dataset is made from.
 * Bit for bit what ngp_nerf_training_pixels writes. */
int ngp_nerf_training_pixels_host(uint32_t n_images, const ngp_nerf_image* images, const ngp_nerf_config* cfg, uint32_t n_rays,
                                  uint32_t ray_offset, uint32_t n_rays_total, ngp_rng rng, const ngp_nerf_error_cdfs* cdfs,
                                  uint32_t* img, float* uv, float* pdf);
/* tcnn fill_rollover / fill_rollover_and_rescale (testbed_nerf.cu:4061-4069); dtype 0 f32, 1 f16 */
int ngp_nerf_fill_rollover(void* stream, uint32_t n_elements, uint32_t stride, const uint32_t* n_input, void* data,
                           int dtype, int rescale);
/* occupancy grid (testbed_nerf.cu:635-809, 3412-3567) */
int ngp_nerf_grid_generate_samples(void* stream, const ngp_nerf_config* cfg, uint32_t n, ngp_rng rng, uint32_t step,
                                   const float* grid, uint32_t n_cascades, float thresh, float* positions,
                                   uint32_t* indices);
int ngp_nerf_grid_splat_max(void* stream, uint32_t n, const uint32_t* indices, const void* density_rm,
                            uint32_t density_activation, float* grid_tmp);
// The reference's memset(grid_tmp, 0) + splat_grid_samples_nerf_max_nearest_neighbor (testbed_nerf.cu:3476, :678-702)
// in one call: grid_tmp[c] = the max over the samples in cell c (0 where none) for all n_cells cells (a multiple of
// 8192), computed as a counting sort by cell bin instead of scattered atomics; bit-identical.
int ngp_nerf_grid_splat_max_cells(void* stream, uint32_t n, const uint32_t* indices, const void* density_rm,
                                  uint32_t density_activation, float* grid_tmp, uint32_t n_cells);
int ngp_nerf_grid_ema(void* stream, uint32_t n, float decay, float* grid, const float* grid_tmp);
int ngp_nerf_grid_mean_and_bitfield(void* stream, const float* grid, uint32_t max_cascade, float* mean, uint8_t* bitfield);

/* Testbed-level NeRF training (Testbed::train -> training_prep_nerf + train_nerf, src/testbed.cu:4285-4370,
 * testbed_nerf.cu:3611-3862, 4137-4152). The model/trainer must be a NerfNetwork and its Trainer. */
int ngp_nerf_trainer_create(ngp_model* model, ngp_trainer* trainer, const ngp_nerf_dataset* ds,
                            const ngp_nerf_config* cfg, uint64_t seed, ngp_nerf_trainer** out);
void ngp_nerf_trainer_destroy(ngp_nerf_trainer* t);
/* The training knobs of a live trainer (Testbed::Nerf::Training members the pybind surface writes, e.g.
 * random_bg_color, loss_type, near_distance, target batch size). max_cascade and the aabb size the density
 * grid and cannot change (recreate the trainer). */
int ngp_nerf_trainer_get_config(const ngp_nerf_trainer* t, ngp_nerf_config* out);
int ngp_nerf_trainer_set_config(ngp_nerf_trainer* t, const ngp_nerf_config* cfg);
int ngp_nerf_train_step(ngp_nerf_trainer* t, void* stream, int get_loss, ngp_nerf_stats* out);
int ngp_nerf_trainer_buffers(ngp_nerf_trainer* t, float** density_grid, uint8_t** bitfield, float** mean_density);
/* The same pointers for READING only: keeps a prelaunched (pipelined) sampler, which reads the bitfield
 * and writes none of the three. Writes through these pointers are not seen by an already prelaunched
 * sampler: use ngp_nerf_trainer_buffers to modify them. */
int ngp_nerf_trainer_buffers_read(const ngp_nerf_trainer* t, const float** density_grid, const uint8_t** bitfield,
                                  const float** mean_density);

/* Rendering (NerfTracer::init_rays_from_camera + trace + shade, testbed_nerf.cu:2229-2659,
 * 948-1196, 2164-2226; ERenderMode::Shade, pinhole). camera: the view (xform after
 * nerf_matrix_to_ngp, focal length in pixels, principal point); the screen centre is
 * render_screen_center(1 - principal point) = the principal point (set_camera_to_training_view,
 * testbed.cu:852, 4376-4379). spp samples starting at sample_index are averaged;
 * out_rgba: device float [height x width x 4], linear colours composited over background_rgba
 * (host, linear; NULL = transparent black). bitfield: the occupancy bitfield (NULL = march everywhere). */
typedef struct ngp_nerf_renderer ngp_nerf_renderer;
int ngp_nerf_renderer_create(ngp_nerf_renderer** out);
void ngp_nerf_renderer_destroy(ngp_nerf_renderer* r);
/* ERenderMode of the following renders (common.h:110-119): 1 Shade (default), 2 Normals (testbed_nerf.cu:
 * 1183-1188, 2179-2181, 2615-2617: the density output's input gradient per step, ngp_input_gradient with
 * backprop_scale 128, composited as normalize(-density'(raw) * gradient), shaded as (0.5 n + 0.5) * alpha),
 * 0 AO (each step's alpha), 3 Positions ((pos - 0.5) / 2 + 0.5, show_accel off), 4 Depth (dot(camera forward,
 * pos - ray origin) * depth_scale): :1189-1208, composited like Shade, no sRGB decoding in the shade step (:2183).
 * 5 Distortion: see ngp_nerf_renderer_set_distortion_map.
 * depth_scale: 1 / the dataset's scale (render_nerf, testbed_nerf.cu:2822); default 1. */
int ngp_nerf_renderer_set_mode(ngp_nerf_renderer* r, int render_mode);
int ngp_nerf_renderer_set_depth_scale(ngp_nerf_renderer* r, float depth_scale);
/* render_mode 9 = ERenderMode::EncodingVis (common.h:120): each step's warped position, the network's input
 * (testbed_nerf.cu:1202-1203). show_accel (Testbed::Nerf::show_accel, testbed.cu:1678; -1 = off, else 0..7): the
 * march tests the occupancy grid from that mip up (:2497, 2594), every step is opaque (:1078-1080), and Positions
 * colours the step's occupancy cell (:1190-1199) */
int ngp_nerf_renderer_set_show_accel(ngp_nerf_renderer* r, int show_accel);
int ngp_nerf_render(ngp_nerf_renderer* r, ngp_model* model, const ngp_nerf_config* cfg, void* stream, const ngp_nerf_image* camera,
                    const uint8_t* bitfield, uint32_t spp, uint32_t sample_index, float min_transmittance,
                    const float* background_rgba, int use_inference_params, float* out_rgba);

/* ---- SDF rendering (src/testbed_sdf.cu) --------------------------------------------------------- */
/* SphereTracer + Testbed::render_sdf (testbed_sdf.cu:47-434, 508-613, 629-1063): sphere tracing of a
 * distance function from a camera, finite-difference (FiniteDifferenceNormalsApproximator, :853-881) or analytic
 * (Network::input_gradient dim 0, testbed.cu:4621) normals, soft shadow rays towards the sun (:233-296) and the
 * Disney-style shading of shade_kernel_sdf (:298-374). Octree skipping, the slice plane, depth of field, foveation,
 * the envmap and the hidden-area mask are not built. */
typedef struct ngp_sdf_renderer ngp_sdf_renderer;
typedef struct {   /* Testbed::Sdf (testbed.h:798-835), BRDFParams, m_sun_dir/m_up_dir (:601-602), floor (:916-917) */
	float aabb_min[3], aabb_max[3];   /* m_aabb; the tracer's box is this inflated by zero_offset */
	float zero_offset, distance_scale, maximum_distance, fd_normals_epsilon, shadow_sharpness;
	uint32_t analytic_normals;        /* network path only; the mesh distance always takes finite differences */
	uint32_t floor_enable, snap_to_pixel_centers;
	uint32_t max_iterations;          /* MARCH_ITER (testbed_sdf.cu:37) */
	float sun_dir[3], up_dir[3];      /* normalised by the renderer, as render_sdf does (:1041-1042) */
	/* BRDFParams (sdf.h:62-72) */
	float metallic, subsurface, specular, roughness, sheen, clearcoat, clearcoat_gloss;
	float basecolor[3], ambientcolor[3];
} ngp_sdf_render_config;
/* the reference's defaults (aabb: the unit cube); no GPU call */
int ngp_sdf_render_default_config(ngp_sdf_render_config* out);
int ngp_sdf_renderer_create(ngp_sdf_renderer** out);
void ngp_sdf_renderer_destroy(ngp_sdf_renderer* r);
/* One view (render_sdf, :883-1063). Exactly one of model / ground_truth non-NULL: the network's distance, or the
 * mesh's BVH signed distance (m_render_ground_truth with ESDFGroundTruthMode::SignedDistance, testbed.cu:4596-4607).
 * camera as in ngp_nerf_render (near distance 0, the principal point as screen centre). render_mode (ERenderMode,
 * common.h:110-119): 0 AO, 1 Shade, 2 Normals, 3 Positions, 4 Depth, 6 Cost; others return NGP_INVALID. spp samples
 * starting at sample_index are averaged. out_rgba: device float [height x width x 4]: hits get alpha 1, misses
 * background_rgba (host; NULL = transparent black). out_depth (nullable): device float [height x width], dot(camera
 * forward, pos - origin), MAX_DEPTH() = 16384 on misses. Null and invalid arguments return NGP_INVALID before any
 * HIP call. */
int ngp_sdf_render(ngp_sdf_renderer* r, ngp_model* model, ngp_sdf_mesh* ground_truth, const ngp_sdf_render_config* cfg,
                   void* stream, const ngp_nerf_image* camera, int render_mode, uint32_t spp, uint32_t sample_index,
                   const float* background_rgba, int use_inference_params, float* out_rgba, float* out_depth);
/* compare_signs_kernel without the octree and scale_iou_counters_kernel (testbed_sdf.cu:474-499), the kernels of
 * Testbed::calculate_iou (:1329-1364): if scale_existing < 1 the eight counters become round(counter * scale_existing),
 * then the n samples are added (distance <= 0 is inside): [0]/[1] reference inside/outside, [2]/[3] model inside/outside,
 * [4] both inside, [5] either inside, [6] 0, [7] n. IoU = counters[4] / counters[5]. */
int ngp_sdf_iou_accumulate(void* stream, uint32_t n, const float* distances_ref, const float* distances_model,
                           float scale_existing, uint32_t* counters /* device [8] */);

/* ---- mesh extraction (src/marching_cubes.cu; Testbed::marching_cubes, testbed.h:472) ---------------------- */
/* Marching cubes over the model sampled on a regular grid. Unlike marching_cubes_gpu (marching_cubes.cu:776-804),
 * which appends through global atomic counters, the output order is a function of the grid alone: two runs give
 * byte-identical buffers. Grid arguments: res[3] points per axis (each >= 2, fewer than 2^32 in all), the box
 * aabb_min / aabb_max (host float[3], positive sides); grid point (x, y, z) lies at aabb_min + (x, y, z) *
 * (aabb_max - aabb_min) / (res - 1), x fastest in memory. aabb_to_local (nullable host float[9], row-major 3x3) is
 * applied to positions as its transpose (gen_vertices, :283); NULL skips the multiply. Null and invalid arguments
 * return NGP_INVALID before any HIP call. */
typedef struct ngp_mesh ngp_mesh;
enum { NGP_MC_NERF = 0, NGP_MC_SDF = 1, NGP_MC_RAW = 2 };
/* The case table (engine extension; gen_faces embeds its own, marching_cubes.cu:363-684), generated on the host at
 * first use: triangle_table [256][16] edge ids, three per triangle, -1 terminated, at most 5 triangles, wound
 * counter-clockwise seen from the outside (f <= thresh); edge_masks [256]: bit e set when edge e changes sign. Bit c of
 * a case: corner c inside (f > thresh); corners 0-3 counter-clockwise on z = 0, 4-7 above them; edges 0-3 bottom, 4-7
 * top, 8-11 vertical (:225-261). Host only. */
int ngp_mc_tables(int8_t* triangle_table, uint16_t* edge_masks);
/* get_marching_cubes_res (marching_cubes.cu:42-49): res_1d points along the box's longest side, every axis rounded up
 * to a multiple of 16. res_out: host uint32[3]. Host only. */
int ngp_marching_cubes_res(uint32_t res_1d, const float* aabb_min, const float* aabb_max, uint32_t* res_out);
/* Testbed::get_density_on_grid (testbed.h:472 marching_cubes' first step): density_out (device float [res.z][res.y][res.x])
 * = the model at every grid point, evaluated in batches of `batch` points. kind NGP_MC_NERF: a NerfNetwork's
 * network_to_density(float(density row 0), density_activation) at positions warped into warp_aabb (the training box;
 * NULL: positions as they are) like the renderer's inputs; NGP_MC_SDF: minus a 3-input network's output row 0, so that
 * inside is f > 0; NGP_MC_RAW: float(row 0) of ngp_density (NerfNetwork) or ngp_inference (3 inputs). */
int ngp_density_on_grid(ngp_model* model, void* stream, int kind, const uint32_t* res, const float* aabb_min, const float* aabb_max,
                        const float* aabb_to_local, const float* warp_aabb_min, const float* warp_aabb_max,
                        uint32_t density_activation, uint32_t batch, int use_inference_params, float* density_out);
/* marching_cubes_gpu (marching_cubes.cu:776-804) and compute_mesh_1ring's normals (:313-348, 702-708): density (device,
 * as ngp_density_on_grid writes it), inside where density > thresh. The mesh holds exact counts (no padding to 128):
 * vertices (coord + dt) * scale + offset with dt = (thresh - f0) / (f1 - f0) (:282-283), area-weighted outward vertex
 * normals (not normalised) and int32 triangles. More than 2^29 vertices fail. */
int ngp_marching_cubes(void* stream, const float* density, const uint32_t* res, const float* aabb_min, const float* aabb_max,
                       const float* aabb_to_local, float thresh, ngp_mesh** out);
/* Testbed::compute_mesh_vertex_colors (testbed.h:472 marching_cubes' last step): NGP_MC_NERF: the NerfNetwork at the
 * vertices (warped into warp_aabb, nullable) seen along minus the normal, network_to_rgb(rgb_activation), then
 * linear_to_srgb; NGP_MC_SDF: 0.5 n + 0.5 of the normalised normal (model unused). */
int ngp_mesh_vertex_colors(ngp_mesh* mesh, ngp_model* model, void* stream, int kind, const float* warp_aabb_min,
                           const float* warp_aabb_max, uint32_t rgb_activation, int use_inference_params);
int ngp_mesh_counts(const ngp_mesh* mesh, uint32_t* n_verts, uint32_t* n_tris);
/* copies to host arrays (each nullable): float [n_verts x 3] vertices, normals, colours; int32 [n_tris x 3] */
int ngp_mesh_read(const ngp_mesh* mesh, void* stream, float* verts_host, float* normals_host, float* colors_host, int32_t* faces_host);
/* save_mesh (marching_cubes.cu:806-956) without the UV unwrap, from host arrays (normals / colours nullable): vertices
 * as (p - offset) / scale (offset NULL = 0), non-finite positions and colours replaced by 0 and normals by +y, normals
 * normalised, colours clamped. A path ending in .ply (any case) gives ASCII PLY, anything else OBJ; faces keep the
 * outward winding of the triangle array. Host only. */
int ngp_mesh_save(const char* path, uint32_t n_verts, const float* verts_host, const float* normals_host, const float* colors_host,
                  uint32_t n_tris, const int32_t* faces_host, float scale, const float* offset);
void ngp_mesh_destroy(ngp_mesh* mesh);

/* Data-parallel NeRF training (no counterpart in the reference, which trains on one GPU: SURVEY F7,
 * §8e). `allreduce` reduces a device buffer in place across the ranks, ordered on `stream` (the
 * caller's RCCL/torch.distributed binding); it is called for the fp16 gradient buffer (sum, before
 * the optimizer), the density-grid splat (max) and three f32 counters (sum). Rank r traces the global
 * rays [R r / N, R (r+1) / N) with their global ids and compacts to B / N samples. */
enum { NGP_DTYPE_F32 = 0, NGP_DTYPE_F16 = 1 };
enum { NGP_REDUCE_SUM = 0, NGP_REDUCE_MAX = 1 };
/* Collectives of the sharded optimizer (ngp_trainer_set_data_parallel), passed in `op` of the same hook. `count`
 * is the whole buffer, a multiple of world; rank r's slice is [r count / world, (r + 1) count / world).
 * NGP_REDUCE_SCATTER_SUM: every rank's buffer summed, the sum of rank r's slice left in rank r's slice (other
 * slices undefined afterwards). NGP_ALL_GATHER: every rank's slice copied into that slice of every rank. */
enum { NGP_REDUCE_SCATTER_SUM = 2, NGP_ALL_GATHER = 3 };
typedef int (*ngp_allreduce_fn)(void* user, void* device_buf, uint64_t count, int dtype, int op, void* stream);
int ngp_nerf_trainer_set_data_parallel(ngp_nerf_trainer* t, uint32_t rank, uint32_t world, ngp_allreduce_fn allreduce, void* user);
// Sampler pipelining (default on, single GPU): when no density-grid update is due before the next
// step, ngp_nerf_train_step launches the next step's ray sampling on an internal stream right after
// this step's loss pass, so it runs under this step's training pass (identical samples: the sampler
// reads only the occupancy bitfield, the rng and the ray count). Disable before modifying the density
// grid or bitfield between steps (ngp_nerf_trainer_buffers discards a prelaunched sampler). No reference counterpart (the
// Testbed runs the step serially, testbed_nerf.cu:3867-4132).
int ngp_nerf_trainer_set_pipeline(ngp_nerf_trainer* t, int enable);

/* The training error map (Testbed::Nerf::Training::ErrorMap, testbed.h:668-677, 736-738). Every step
 * deposits the compacted rays' losses into it (accumulate_error, testbed_nerf.cu:3951-3953, 4044); it is
 * zeroed and resized to min(3.5 (n_steps_between * rays_per_batch / n_images)^(1/4), image size) when a
 * window starts (:3659-3666), and after n_steps_between steps its CDFs are built (construct_cdf_2d/1d and
 * the host pass over the per-image totals, :3700-3748) and the window grows by 1.5x. which: 0 data
 * [n_images][height][width], 1 cdf_x_cond_y (cdf resolution), 2 cdf_y [n_images][cdf_height], 3 cdf_img
 * [n_images] (the normalised image CDF), 4 pmf_img [n_images] (host). Copies min(cap, size) floats to
 * host memory `out` (NULL: only *info) after the trainer's stream work. */
typedef struct {
	uint32_t width, height;          /* error_map.resolution */
	uint32_t cdf_width, cdf_height;  /* error_map.cdf_resolution */
	uint32_t n_images;
	uint32_t cdf_valid;              /* error_map.is_cdf_valid */
	uint32_t n_steps_since_update, n_steps_between_updates;
	uint64_t size;                   /* floats held by the requested array */
} ngp_nerf_error_map_info;
int ngp_nerf_trainer_error_map(ngp_nerf_trainer* t, int which, float* out, uint64_t cap, ngp_nerf_error_map_info* info);

/* Snapshots (Testbed::save_snapshot / load_snapshot, src/testbed.cu:4873-5057; python_api.cu:446-447):
 * msgpack of the network config (network_config_json, the Testbed's m_network_config; NULL = {}) with
 * a "snapshot" member holding tcnn Trainer::serialize (n_params, params_type "__half", params_binary),
 * [optimizer state], version 1, mode "nerf", density_grid_size, density_grid_binary (fp16), nerf.aabb_scale,
 * nerf.rgb counters, training_step, loss, aabb. Paths ending in .ingp are gzip streams (zstr; level 0
 * unless compress), others raw msgpack; loading accepts gzip, zlib or raw. Loading restores the params
 * (and the optimizer state if present), the density grid (mean and bitfield recomputed), the
 * rays-per-batch counters and the training step; the network must have the snapshot's n_params.
 * Engine extension (the reference does not save m_envmap): with an environment map set, a member "envmap" holds
 * width, height, params_binary and ema_params_binary (fp32) and, with the optimizer state, "optimizer" {current_step,
 * ema_valid, ema_binary, first_moments_binary, second_moments_binary, param_steps_binary}. Loading sets the trainer's
 * map from it; a snapshot without the member leaves the trainer's map as it is. Likewise with a lens distortion map
 * bound: a member "distortion_map" holds width, height and params_binary ([height][width][2] fp32) and, with the
 * optimizer state, "optimizer" {current_step, ema_valid, ema_binary, ema_params_binary, first_moments_binary,
 * second_moments_binary, param_steps_binary}. Loading binds the map; a snapshot without the member leaves the
 * trainer's map as it is. */
int ngp_nerf_save_snapshot(ngp_nerf_trainer* t, void* stream, const char* path, const char* network_config_json,
                           int include_optimizer_state, int compress);
int ngp_nerf_load_snapshot(ngp_nerf_trainer* t, void* stream, const char* path);
/* Testbed::save_snapshot / load_snapshot for the image and SDF testbeds (testbed.cu:4873-5057): the trainer's
 * Trainer::serialize members (as in the NeRF snapshot), version, mode (e.g. "sdf", "image"), training_step, loss,
 * aabb {min, max} and bounding_radius. Loading restores the parameters (and the optimizer state if present; an
 * optimizer member lacking some arrays fills them from the parameters / zeros) and returns the scalars (each output
 * nullable; bounding_radius keeps its value when the snapshot has none). ngp_snapshot_mode: the snapshot's mode
 * (a NeRF snapshot without one: "nerf"), for a Testbed to switch mode before reset_network. */
int ngp_save_snapshot(ngp_trainer* t, void* stream, const char* path, const char* network_config_json, const char* mode,
                      const float* aabb_min, const float* aabb_max, float bounding_radius, uint32_t training_step, float loss,
                      int include_optimizer_state, int compress);
int ngp_load_snapshot(ngp_trainer* t, void* stream, const char* path, uint32_t* training_step, float* loss, float* aabb_min,
                      float* aabb_max, float* bounding_radius);
int ngp_snapshot_mode(const char* path, char* mode_buf, uint64_t cap);
/* Testbed::load_network_config (testbed.cu:246) of a snapshot: the config as JSON text without the
 * "snapshot" member (binaries as {"binary_bytes": n}); size query with json_buf = NULL. */
int ngp_snapshot_network_config(const char* path, char* json_buf, uint64_t* size);

/* The engine's own RCCL communicator (engine extension; SURVEY §8e exchange step). Rank 0 makes the
 * id, every rank passes the same bytes (any host channel) to ngp_dp_comm_create, which blocks until
 * all `world` ranks have joined; call it with the rank's HIP device current. ngp_dp_comm_allreduce
 * is an ngp_allreduce_fn (user = the communicator): ncclAllReduce in place on `stream`, graph-capturable. */
#define NGP_DP_UNIQUE_ID_BYTES 128
typedef struct ngp_dp_comm ngp_dp_comm;
int ngp_dp_comm_unique_id(uint8_t* id_out);
int ngp_dp_comm_create(uint32_t rank, uint32_t world, const uint8_t* id_in, ngp_dp_comm** out);
void ngp_dp_comm_destroy(ngp_dp_comm* c);
int ngp_dp_comm_allreduce(void* user, void* device_buf, uint64_t count, int dtype, int op, void* stream);
/* Wire type of fp16 sums (default NGP_DTYPE_F32: widened to fp32, all-reduced, rounded to fp16 once —
 * RCCL's fp16 ring rounds at every hop, so its sum depends on N and ring order; NGP_DTYPE_F16: half the
 * bytes). ngp_dp_comm_reserve sizes the fp32 staging buffer for `count` elements; it must run outside
 * graph capture (the trainers call it when the communicator is bound). */
int ngp_dp_comm_set_wire(ngp_dp_comm* c, int dtype);
int ngp_dp_comm_reserve(ngp_dp_comm* c, uint64_t count);
/* Gradient exchange inside the trainer's step (network-level data parallelism, bench.py --gpus N):
 * after every forward_backward captured by ngp_trainer_capture_training_step, and before the
 * optimizer, the fp16 gradient buffer is all-reduced (sum) with `allreduce`; the optimizer divides
 * by `world` (mean gradient) on top of its loss scale. allreduce = NULL turns it off. */
int ngp_trainer_set_allreduce(ngp_trainer* t, uint32_t world, ngp_allreduce_fn allreduce, void* user);
/* The same exchange with this process's rank, so that large-table (lazy-EMA) trainers shard the optimizer
 * (trainer option "shard_opt", default 1): the fp16 gradients, widened to fp32, are reduce-scattered; rank r
 * updates the optimizer records of its 1/world slice of the parameters from the fp32 sums rounded to fp16
 * once (bit for bit the all-reduce path's update) and the fp16 weights are all-gathered: half the wire bytes
 * of an fp32 all-reduce and 1/world of the update per rank. Other trainers, and shard_opt 0, all-reduce.
 * With world > 1 the records of other ranks' slices are stale on this rank after a sharded step: the EMA
 * (inference) parameters, the full-precision weights and serialize need ngp_trainer_gather_shards first,
 * called on every rank (they fail otherwise); the fp16 training parameters are always complete. */
int ngp_trainer_set_data_parallel(ngp_trainer* t, uint32_t rank, uint32_t world, ngp_allreduce_fn fn, void* user);
/* Collective (every rank, same order): all-gather the sharded optimizer records so that every rank holds the
 * whole optimizer state again. A no-op unless a sharded step left them partial. */
int ngp_trainer_gather_shards(ngp_trainer* t, void* stream);

/* ---- NeRF camera pose refinement (nerf.training.optimize_extrinsics) ------------------------------------------ */
/* ngp_trainer_train_step that also writes dL/dinput (fp32 AoS [n x dL_dinput_stride]: the position rows through the
 * grid and, for a NerfNetwork, the direction rows through SH, as ngp_backward does; NerfNetwork::backward's dL_dinput,
 * nerf_network.h). The gradient is taken with respect to the weights the forward used: it runs before the grid's
 * fused optimizer update (ngp_trainer_fused_update_active). dL_dinput must not alias input. */
int ngp_trainer_train_step_input_gradient(ngp_trainer* t, void* stream, uint32_t n, const float* input, uint32_t input_stride,
                                          const void* dL_doutput, uint32_t dL_stride, float loss_scale, float* dL_dinput,
                                          uint32_t dL_dinput_stride);
/* compute_cam_gradient_train_nerf (testbed_nerf.cu:2014-2123), extrinsics only (uv_pdf 1; no distortion map, no focal
 * length). Inputs: the compacted batch after the loss pass (numsteps [R x 2] = {n, base}, coords [B x 7]), its input
 * gradient (fp32 rows of gradient_stride >= 7 floats: 0..2 position, 4..6 direction), the kept rays' ids (ascending)
 * and unnormalised rays [R x 6], the device ray counter and the training box of cfg. Per kept ray with n > 0 the
 * samples' position gradients (divided by the box's sides) sum to the origin gradient, and position gradient x
 * distance to the origin + 0.5 x direction gradient to the direction gradient gd; pos_gradient[img] += origin gradient,
 * rot_gradient[img] += cross(normalize(d), gd), both device float [n_images x 3], accumulated onto their content.
 * Unlike the reference, which adds every ray with float atomics, each ray's six floats are stored and every image's
 * rays (one contiguous run of the kept rays) are summed in ray order: two calls on the same inputs give the same
 * bytes. n_rays_total * n_images must stay below 2^32. Null and invalid arguments return NGP_INVALID before any HIP
 * call. */
int ngp_nerf_camera_gradients(const ngp_nerf_config* cfg, void* stream, uint32_t n_rays_total, uint32_t n_images,
                              const uint32_t* ray_counter, const uint32_t* ray_indices, const float* rays,
                              const uint32_t* numsteps, const float* coords, const float* coords_gradient,
                              uint32_t gradient_stride, float* pos_gradient, float* rot_gradient);
/* The per-camera optimisers of Testbed::Nerf::Training (cam_pos_offset: AdamOptimizer<vec3>, cam_rot_offset:
 * RotationAdamOptimizer; adam_optimizer.h:128-309): n_images pairs of Adam states, beta1 0.9, beta2 0.99, epsilon 1e-8,
 * initial learning rate 1e-4 (testbed_nerf.cu:3037-3038). Host only: no GPU call. The rotation variable is updated as
 * rotvec(rotmat(-step) * rotmat(variable)) (common_device.cuh:698-722) with the angle taken as 2 atan2(|xyz|, w) of
 * the product's quaternion, not 2 acos(w), which loses the 1e-4 rad rotations this optimiser makes. */
typedef struct ngp_pose_optimizer ngp_pose_optimizer;
typedef struct {   /* the members VarAdamOptimizer::to_json writes (adam_optimizer.h:174-183) */
	uint32_t iter;
	float first_moment[3], second_moment[3], variable[3];
	float learning_rate, epsilon, beta1, beta2;
} ngp_adam_state;
int ngp_pose_optimizer_create(uint32_t n_images, ngp_pose_optimizer** out);
void ngp_pose_optimizer_destroy(ngp_pose_optimizer* o);
uint32_t ngp_pose_optimizer_n_images(const ngp_pose_optimizer* o);
/* reset_state of every camera / of one (testbed_nerf.cu:2921-2933, 2911-2912): moments, variable and iter to 0 */
int ngp_pose_optimizer_reset(ngp_pose_optimizer* o);
int ngp_pose_optimizer_reset_one(ngp_pose_optimizer* o, uint32_t i);
/* One update of every camera (testbed_nerf.cu:3784-3805) from the accumulated gradients (host float [n_images x 3]
 * each): gradient * n_images / 128 / n_steps_between + l2_reg * variable, learning rate max(extrinsic_lr *
 * 0.33^(iter / 128), network_lr / 1000) with the integer quotient of the camera's iter before the step. */
int ngp_pose_optimizer_step(ngp_pose_optimizer* o, const float* pos_grad, const float* rot_grad, uint32_t n_steps_between,
                            float extrinsic_lr, float l2_reg, float network_lr);
int ngp_pose_optimizer_get(const ngp_pose_optimizer* o, uint32_t i, ngp_adam_state* pos, ngp_adam_state* rot);  /* each nullable */
int ngp_pose_optimizer_set_state(ngp_pose_optimizer* o, uint32_t i, const ngp_adam_state* pos, const ngp_adam_state* rot);
/* rotvec(rotmat(a) * rotmat(b)): the composition the rotation optimiser applies. float[3] each, host only. */
int ngp_pose_compose_rotation(const float* a, const float* b, float* out);
/* Training::update_transforms for one image (testbed_nerf.cu:2998-3019): xform (camera-to-world mat4x3, column-major
 * float[12]) with its rotation divided by cbrt(det) when |det - 1| > 0.01, then rotmat(rot_offset) * rotation and
 * translation + pos_offset. Zero offsets return a proper rotation's xform bit for bit. Host only. */
int ngp_pose_apply(const float* xform, const float* rot_offset, const float* pos_offset, float* out);
/* Testbed::Nerf::Training's camera optimisation knobs (testbed.h:716-785; python_api.cu:618-653) and their defaults. */
typedef struct {
	uint32_t optimize_extrinsics;           /* 0 */
	uint32_t n_steps_between_cam_updates;   /* 16 */
	float extrinsic_l2_reg;                 /* 1e-4 */
	float extrinsic_learning_rate;          /* 1e-3 */
} ngp_nerf_camera_training;
/* With optimize_extrinsics the training step also takes the compacted batch's input gradient (with respect to the
 * forward's weights), sums it per image (ngp_nerf_camera_gradients; testbed_nerf.cu:3641-3644, 4071-4125) and, every
 * n_steps_between_cam_updates steps, steps the per-camera optimisers and rebuilds the cameras the sampler traces
 * (:3754-3809, update_transforms :2980-3024); the next step's rays come from the new poses. Off (default): the step
 * issues exactly the launches it would without this call. Single GPU: enabling it on a trainer with an exchange hook,
 * or setting a hook while it is on, fails (the per-image sums would need their own all-reduce). */
int ngp_nerf_trainer_set_camera_training(ngp_nerf_trainer* t, const ngp_nerf_camera_training* c);
int ngp_nerf_trainer_get_camera_training(const ngp_nerf_trainer* t, ngp_nerf_camera_training* out);
/* Training::transforms[i].start (get_camera_extrinsics, :2973-2978, before ngp_matrix_to_nerf): image i's refined
 * camera-to-world transform in NGP space, float[12] column-major; the dataset's own, bit for bit, while the offsets
 * are zero. */
int ngp_nerf_trainer_camera_extrinsics(const ngp_nerf_trainer* t, uint32_t i, float* out);
/* set_camera_extrinsics (:2896-2919) with an NGP-space transform: replaces image i's transform in this trainer (the
 * dataset is not modified) and resets that image's optimiser state, its exposure optimiser included (:2911-2913).
 * Discards a prelaunched sampler. */
int ngp_nerf_trainer_set_camera_extrinsics(ngp_nerf_trainer* t, uint32_t i, const float* xform);
/* reset_camera_extrinsics (:2921-2933): every camera's optimiser state to zero (pose and exposure), cameras rebuilt. */
int ngp_nerf_trainer_reset_camera_extrinsics(ngp_nerf_trainer* t);
/* Engine extension (inspection): the last step's sampler call on a single-GPU trainer: its rng, ray count and sample
 * budget (the arguments ngp_nerf_generate_training_samples would take, with the trainer's bitfield) and the device
 * buffers it wrote: ray_indices [n_rays], rays [n_rays x 6], counters [>= 2]. They hold that step's rays until a
 * later sampler writes them: with pipelining on, that may be as soon as the step returns. Outputs nullable. */
int ngp_nerf_trainer_last_samples(const ngp_nerf_trainer* t, ngp_rng* rng, uint32_t* n_rays, uint32_t* max_samples,
                                  const uint32_t** ray_indices, const float** rays, const uint32_t** counters);
/* Training::sample_focal_plane_proportional_to_error / sample_image_proportional_to_error (both off by default, as in
 * the reference). With a switch on, once the first error map window has closed (ngp_nerf_trainer_error_map: cdf_valid),
 * every step's sampler and loss pass draw the rays' pixels from the CDFs of the last closed window; before that, and
 * with both off, the step issues exactly the launches and writes exactly the bytes it would without this call. The
 * step that closes a window prelaunches no sampler: the next step's rays come from the new CDFs. The map is summed
 * with float atomics, whose last bits feed the CDFs: with a switch on, training is not reproducible from run to run.
 * Discards a prelaunched sampler. Cannot be combined with optimize_extrinsics (either call fails, state unchanged). */
int ngp_nerf_trainer_set_error_sampling(ngp_nerf_trainer* t, int focal_plane, int image);
int ngp_nerf_trainer_get_error_sampling(const ngp_nerf_trainer* t, int* focal_plane, int* image);  /* each nullable */
/* cam_pos_offset[i] / cam_rot_offset[i] (each nullable) */
int ngp_nerf_trainer_pose_optimizer_state(const ngp_nerf_trainer* t, uint32_t i, ngp_adam_state* pos, ngp_adam_state* rot);

/* ---- environment map (Testbed::m_envmap, Training::train_envmap) --------------------------------- */
/* A small trainable equirectangular RGBA image read by ray direction as the background at infinity (envmap.cuh:29-94,
 * dir_to_spherical_unorm random_val.cuh:62-72). A map is [height][width][4] fp32, texel index x + y * width.
 * ngp_envmap_lookup: the four texels and bilinear weights of n normalized directions (dirs [n x 3]) as read_envmap and
 * deposit_envmap_gradient both derive them (envmap.cuh:30-35, 59-64): texels [n x 4] in the order (x, y), (x+1, y),
 * (x, y+1), (x+1, y+1) with x wrapped and y clamped, weights [n x 4] = (1-wx)(1-wy), wx(1-wy), (1-wx)wy, wx wy.
 * Device memory. _host: the same function compiled for the host, host memory, no GPU call; acosf / atan2f differ
 * between the two, so they agree to rounding, not to the bit. Width and height in 1..8192. */
int ngp_envmap_lookup(void* stream, uint32_t width, uint32_t height, uint32_t n, const float* dirs, uint32_t* texels,
                      float* weights);
int ngp_envmap_lookup_host(uint32_t width, uint32_t height, uint32_t n, const float* dirs, uint32_t* texels, float* weights);
/* Engine extension (inspection): deposit_envmap_gradient (envmap.cuh:57-94, T = half) of n fp16 rgb values
 * (values_f16 [n x 3]; alpha's gradient is zero in the reference, testbed_nerf.cu:2007-2008) along n directions, as
 * the loss pass does it: each corner receives fp16(value) * fp16(weight) rounded to fp16, and gradient
 * [height][width][4] fp32 is WRITTEN with the exact sum of a channel's contributions rounded once to fp32 (64-bit
 * integer atomics in units of 2^-24: no dependence on the order of arrival). A non-finite contribution makes its
 * channel NaN. */
int ngp_envmap_deposit(void* stream, uint32_t width, uint32_t height, uint32_t n, const float* dirs, const void* values_f16,
                       float* gradient);
/* tcnn Trainer<float, float, float>::optimizer_step over a TrainableBuffer (testbed.cu:4133-4147, testbed_nerf.cu:
 * 3683-3685): one step of the Ema / ExponentialDecay / Adam chain of optimizer_json over n fp32 parameters with an
 * fp32 gradient, no matrix weights (a parameter whose gradient is exactly zero is skipped: no l2 term, its entry of
 * param_steps stays). `step`: the chain's steps taken before this one (schedule, EMA debias). ema / ema_params (both
 * required under an Ema wrapper): the running EMA and its debiased value. Device memory, caller-owned state. */
int ngp_envmap_optimizer_step(void* stream, const char* optimizer_json, uint32_t step, float loss_scale, uint32_t n, float* params,
                              const float* gradient, float* first_moments, float* second_moments, uint32_t* param_steps,
                              float* ema, float* ema_params);
/* ngp_nerf_compute_loss with an environment map bound (testbed_nerf.cu:1781-1792): every ray's background becomes
 * envmap.rgb + srgb_to_linear(background) * (1 - envmap.a) in the ray's normalized direction, before the target and
 * the prediction use it. envmap_gradient (nullable; [env_height][env_width][4], WRITTEN): the loss's gradient with
 * respect to the map (:1988-2011): rays that kept all of their samples (and at least one) deposit
 * fp16(loss_scale / n_rays * T * dL/drgb [/ srgb_to_linear_derivative(background)]) as ngp_envmap_deposit does, with
 * the gradient of envmap_loss_type (ELossType) where that differs from cfg's loss; alpha's gradient stays zero. */
int ngp_nerf_compute_loss_envmap(const ngp_nerf_dataset* ds, const ngp_nerf_config* cfg, void* stream, uint32_t n_rays,
                                 uint32_t n_rays_total, ngp_rng rng, uint32_t max_samples_compacted,
                                 const uint32_t* ray_counter, const void* network_output, const uint32_t* ray_indices,
                                 const float* rays, uint32_t* numsteps, const float* coords_in, float* coords_out,
                                 void* dloss_doutput, float* loss, uint32_t* compacted_counter, const float* mean_density,
                                 float loss_scale, const float* envmap, uint32_t env_width, uint32_t env_height,
                                 uint32_t envmap_loss_type, float* envmap_gradient);
/* The trainer's map (m_envmap; reset_network / load_nerf_post, testbed.cu:4133-4147, nerf_loader.cu:516-528): rgba
 * (nullable: zeros) are the [height][width][4] initial values in HOST memory. Setting a map resets its optimizer.
 * With a map set every training ray is composited over it (the raw parameters, m_envmap.view()); without one the step
 * issues exactly the launches it would have. */
int ngp_nerf_trainer_set_envmap(ngp_nerf_trainer* t, uint32_t width, uint32_t height, const float* rgba);
int ngp_nerf_trainer_clear_envmap(ngp_nerf_trainer* t);
enum {
	NGP_ENVMAP_PARAMS = 0,            /* the raw parameters (training reads these) */
	NGP_ENVMAP_INFERENCE_PARAMS = 1,  /* inference_view(): the debiased EMA once a step ran under an Ema wrapper */
	NGP_ENVMAP_GRADIENT = 2,          /* the last step's gradient (still scaled by LOSS_SCALE = 128) */
	NGP_ENVMAP_FIRST_MOMENTS = 3,
	NGP_ENVMAP_SECOND_MOMENTS = 4,
	NGP_ENVMAP_PARAM_STEPS = 5        /* per-parameter Adam step counters: uint32 in the float slots */
};
/* Copies array `which` ([height][width][4]) to HOST memory (out nullable: only the resolution; 0 x 0: no map). */
int ngp_nerf_trainer_envmap(const ngp_nerf_trainer* t, int which, float* out, uint64_t capacity, uint32_t* width,
                            uint32_t* height);
/* The device array (NGP_ENVMAP_PARAMS or NGP_ENVMAP_INFERENCE_PARAMS; NULL without a map), e.g. for
 * ngp_nerf_renderer_set_envmap. Valid until the map is set or cleared; which array holds the inference parameters
 * changes with the first training step, so ask again after training. */
int ngp_nerf_trainer_envmap_device(const ngp_nerf_trainer* t, int which, const float** data, uint32_t* width, uint32_t* height);
/* Training::train_envmap (testbed.h:716-785, python_api.cu:618-653; default off): every step sums the map's gradient
 * (bitwise reproducible, see ngp_envmap_deposit) and takes one step of the map's optimizer with LOSS_SCALE after the
 * loss pass (testbed_nerf.cu:3668-3685). Without a map it does nothing, as in the reference. Single GPU: refused with
 * a data-parallel exchange hook set, and so is setting a hook while it is on. */
int ngp_nerf_trainer_set_train_envmap(ngp_nerf_trainer* t, int train);
int ngp_nerf_trainer_get_train_envmap(const ngp_nerf_trainer* t, int* train);
/* The network config's "envmap" section (testbed.cu:4135-4136): the map's loss (ELossType; -1: the training loss)
 * and its optimizer chain (JSON as ngp_trainer_create takes it; NULL: the main trainer's). base.json trains the map
 * with RelativeL2 and its own Ema / ExponentialDecay / Adam. */
int ngp_nerf_trainer_set_envmap_training(ngp_nerf_trainer* t, int loss_type, const char* optimizer_json);
/* render_nerf with an environment map (testbed_nerf.cu:2315-2319): the frame is pre-filled per pixel with the map's
 * value in the pixel's normalized ray direction instead of background_rgba. envmap: DEVICE [height][width][4] fp32,
 * owned by the caller and read by every later ngp_nerf_render; NULL unbinds. */
int ngp_nerf_renderer_set_envmap(ngp_nerf_renderer* r, const float* envmap, uint32_t width, uint32_t height);

/* ---- lens distortion map (Testbed::m_distortion, Training::optimize_distortion) ----------------------------------- */
/* A small trainable 2-D map of ray-direction offsets that absorbs what the declared lens model does not explain:
 * uv_to_ray adds distortion.at_lerp(uv) to dir.xy after the lens (common_device.cuh:443-510), and
 * compute_cam_gradient_train_nerf splats every ray's image-plane gradient into it (testbed_nerf.cu:2088-2099). A map
 * is [height][width][2] fp32, texel index x + y * width; width and height in 1..8192.
 * ngp_nerf_distortion_lookup: the four texels and bilinear weights of n positions uv [n x 2] as Buffer2DView::at_lerp
 * (common.h:384-400) and deposit_image_gradient (common_device.cuh:124-156) both derive them: xy = (width, height) * uv,
 * texel (int)xy, weights xy - texel; texels [n x 4] in the order (x, y), (x+1, y), (x, y+1), (x+1, y+1), each clamped
 * into the map, weights [n x 4] = (1-wx)(1-wy), wx(1-wy), (1-wx)wy, wx wy. Deviation: uv is first folded into [0, 2]
 * with NaN to 0, so every index is inside the map whatever uv holds. map (nullable) with offsets (nullable, [n x 2]):
 * also the mixed offset, the four products summed in that order. Device memory. _host: the same function compiled for
 * the host, host memory, no GPU call; only IEEE add, subtract, multiply, compare and convert are used, so the two agree
 * bit for bit. */
int ngp_nerf_distortion_lookup(void* stream, uint32_t width, uint32_t height, uint32_t n, const float* uv, uint32_t* texels,
                               float* weights, const float* map, float* offsets);
int ngp_nerf_distortion_lookup_host(uint32_t width, uint32_t height, uint32_t n, const float* uv, uint32_t* texels, float* weights,
                                    const float* map, float* offsets);
/* ngp_nerf_generate_training_samples_cdf with a distortion map (DEVICE, nullable) added to every ray's dir.xy at the
 * ray's (u, v), after the lens; the rng draws and the pixel choice are unchanged. distortion_map NULL: the same
 * kernels and the same bytes as without it. */
int ngp_nerf_generate_training_samples_distortion(const ngp_nerf_dataset* ds, const ngp_nerf_config* cfg, void* stream,
                                                  uint32_t n_rays, uint32_t ray_offset, uint32_t n_rays_total, ngp_rng rng,
                                                  uint32_t max_samples, const uint8_t* bitfield, uint32_t* ray_indices,
                                                  float* rays, uint32_t* numsteps, float* coords, uint32_t* counters,
                                                  const ngp_nerf_error_cdfs* cdfs, const float* distortion_map,
                                                  uint32_t map_width, uint32_t map_height);
/* compute_cam_gradient_train_nerf's distortion branch, per ray (testbed_nerf.cu:2088-2099): ngp_nerf_camera_gradients'
 * arguments and first pass, which additionally writes, for every kept ray, ray_gradients[r] = (inverse(mat3(xform_img))
 * * (gd - d * dot(gd, d))).xy with d = normalize(ray.d) and gd the ray's summed direction gradient; zeros for a ray
 * without samples. camera_matrices: DEVICE [n_images x 9], each image's column-major 3x3; the inverse is the general
 * one (adjugate / determinant), not the transpose. ray_gradients: DEVICE, room for n_rays_total x 2 floats.
 * pos_gradient / rot_gradient: both given, the per-image sums are added onto them exactly as ngp_nerf_camera_gradients
 * does (the same bytes); both NULL, the second pass is not launched. */
int ngp_nerf_distortion_ray_gradients(const ngp_nerf_config* cfg, void* stream, uint32_t n_rays_total, uint32_t n_images,
                                      const uint32_t* ray_counter, const uint32_t* ray_indices, const float* rays,
                                      const uint32_t* numsteps, const float* coords, const float* coords_gradient,
                                      uint32_t gradient_stride, float* pos_gradient, float* rot_gradient,
                                      const float* camera_matrices, float* ray_gradients);
/* The map's gradient accumulator: exact and independent of the order of arrival at any magnitude (the reference adds
 * floats atomically). A finite fp32 contribution is M * 2^(e - 149) with a signed 24-bit integer M and e = max(biased
 * exponent, 1) - 1; it is added as the 64-bit integer M << (e % 16) into bin e / 16 of its channel, so bin b's unit is
 * 2^(16 b - 149) and 2^22 contributions to one bin cannot overflow it. Layout: [height][width][3 channels][16 bins]
 * signed 64-bit words, the channels sum g.x w, sum g.y w and sum w (the reference keeps one weight per gradient
 * channel; they are equal), then one word counting the rays whose gradient was not finite, which are dropped whole
 * (deviation: the reference would turn the texel NaN for good). _accumulator_words: the word count of a map (0: invalid size). The
 * accumulator is the caller's DEVICE memory, zeroed by the caller, and may be read as it is.
 * ngp_nerf_distortion_deposit (deposit_image_gradient): one thread per kept ray (*ray_counter of them, ids in
 * ray_indices) recomputes the ray's uv from its id and rng by the uniform training pixel draw, as the loss pass does,
 * and adds g.x * w_k, g.y * w_k and w_k for the four corners, each product one fp32 multiply, zero products skipped.
 * ray_gradients [R x 2]; numsteps (nullable, [R x 2]): a ray whose count is 0 deposits nothing (:2044-2048). Calls
 * accumulate. ngp_nerf_distortion_gradient (safe_divide, :3811-3816): gradient [height][width][2] is WRITTEN with
 * (float)(S_g / S_w) per channel, S the bins summed in double from the highest down and the quotient rounded to fp32
 * once, or 0 where S_w == 0. */
uint64_t ngp_nerf_distortion_accumulator_words(uint32_t width, uint32_t height);
int ngp_nerf_distortion_deposit(const ngp_nerf_dataset* ds, const ngp_nerf_config* cfg, void* stream, uint32_t n_rays_total,
                                ngp_rng rng, const uint32_t* ray_counter, const uint32_t* ray_indices, const uint32_t* numsteps,
                                const float* ray_gradients, uint32_t width, uint32_t height, uint64_t* accumulator);
int ngp_nerf_distortion_gradient(void* stream, uint32_t width, uint32_t height, const uint64_t* accumulator, float* gradient);
/* The trainer's map (m_distortion.map, a TrainableBuffer<2, 2, float>; testbed.cu:4066-4076): params (nullable: zeros,
 * TrainableBuffer::initialize_params) are the [height][width][2] initial values in HOST memory. Setting a map resets
 * its optimizer and discards a prelaunched sampler. A bound map is read by every sampler the trainer launches,
 * whether optimize_distortion is on or off, as in the reference, which always owns a 32 x 32 zero map; a trainer here
 * has none until asked, and then issues exactly the launches it would have. _clear also turns the switch off. */
int ngp_nerf_trainer_set_distortion_map(ngp_nerf_trainer* t, uint32_t width, uint32_t height, const float* params);
int ngp_nerf_trainer_clear_distortion_map(ngp_nerf_trainer* t);
enum {
	NGP_DISTORTION_PARAMS = 0,           /* the raw parameters (the sampler reads these) */
	NGP_DISTORTION_GRADIENT = 1,         /* the last update's gradient, sum g w / sum w (scaled by 128 * n_steps_between) */
	NGP_DISTORTION_FIRST_MOMENTS = 2,
	NGP_DISTORTION_SECOND_MOMENTS = 3,
	NGP_DISTORTION_PARAM_STEPS = 4,      /* per-parameter Adam step counters: uint32 in the float slots */
	NGP_DISTORTION_INFERENCE_PARAMS = 5  /* the parameters; the debiased EMA once a step ran under an Ema wrapper (the
	                                        default chain has none) */
};
/* Copies array `which` ([height][width][2]) to HOST memory (out nullable: only the resolution; 0 x 0: no map). */
int ngp_nerf_trainer_distortion_map(const ngp_nerf_trainer* t, int which, float* out, uint64_t capacity, uint32_t* width,
                                    uint32_t* height);
/* The device array (NGP_DISTORTION_PARAMS or NGP_DISTORTION_INFERENCE_PARAMS; NULL without a map), e.g. for
 * ngp_nerf_renderer_set_distortion_map. Valid until the map is set or cleared. */
int ngp_nerf_trainer_distortion_map_device(const ngp_nerf_trainer* t, int which, const float** data, uint32_t* width,
                                           uint32_t* height);
/* The trainer's accumulator copied to HOST memory as it is (out nullable: only the word count; 0: no map). */
int ngp_nerf_trainer_distortion_accumulator(const ngp_nerf_trainer* t, uint64_t* out, uint64_t capacity, uint64_t* words);
/* The network config's "distortion_map" section (testbed.cu:4068-4076): the map's optimizer chain (JSON as
 * ngp_trainer_create takes it; NULL: the main trainer's) and the resolution of the map that turning
 * optimize_distortion on creates when none is bound (the reference's default: 32 x 32). */
int ngp_nerf_trainer_set_distortion_training(ngp_nerf_trainer* t, const char* optimizer_json, uint32_t width, uint32_t height);
/* Training::optimize_distortion (testbed.h:716-785; default off). On: the training step takes the compacted batch's
 * input gradient as optimize_extrinsics does, stores every kept ray's image-plane gradient
 * (ngp_nerf_distortion_ray_gradients with the trainer's current cameras) and deposits it (ngp_nerf_distortion_deposit)
 * into the trainer's accumulator, which starts from zero after every update; every n_steps_between_cam_updates steps
 * (the counter shared with poses and exposure) it takes the gradient (ngp_nerf_distortion_gradient) and one step of
 * the map's optimizer with loss scale 128 * n_steps_between_cam_updates (testbed_nerf.cu:3811-3818) on the step's
 * stream, and the next step's sampler runs behind that update. Every step of this is bitwise reproducible. Without a
 * map, turning it on creates a zero map of the configured resolution. Refused, with the state unchanged: together
 * with either error-sampling switch (uv_pdf is taken as 1), and with a data-parallel exchange hook (the gradient is
 * not all-reduced), in either order of setting. */
int ngp_nerf_trainer_set_optimize_distortion(ngp_nerf_trainer* t, int optimize);
int ngp_nerf_trainer_get_optimize_distortion(const ngp_nerf_trainer* t, int* optimize);
/* render_nerf through a distortion map (Testbed::Nerf::render_with_lens_distortion; testbed_nerf.cu:2229-2344): every
 * pixel's ray gets the map's offset at the pixel's uv added to dir.xy after the lens, and render mode 5
 * (ERenderMode::Distortion, :2331-2344) shows to_rgb(offset * 50) with alpha 1 for every pixel, the offset read at
 * (x + 0.5, y + 0.5) / resolution, without marching a ray (hsv_to_rgb / to_rgb, common_device.cuh:802-827; without a
 * map the offset is zero). map: DEVICE [height][width][2] fp32, owned by the caller and read by every later
 * ngp_nerf_render; NULL unbinds. */
int ngp_nerf_renderer_set_distortion_map(ngp_nerf_renderer* r, const float* map, uint32_t width, uint32_t height);

/* ---- depth supervision (Training::depth_supervision_lambda, depth_loss_type; NerfDataset depth images) ---------- */
/* NerfDataset::set_training_image's depth part (nerf_loader.cu:943-960, copy_depth :81-90): image `image` gets an fp32
 * depth image [height][width] on the device, depth[i] = (float)pixel[i] * depth_scale (one fp32 multiply) from HOST
 * pixels of dtype 0 (uint16) or 1 (float32). depth_host NULL or depth_scale <= 0 stores zeros (a depth of 0 means "no
 * depth at this pixel"); depth_host NULL with depth_scale < 0 removes the image's depth. Images without depth keep a
 * null pointer and cost nothing. A NULL dataset, an image index out of range, another dtype or a NaN scale return
 * NGP_INVALID before any HIP call. Waits for the device: no loss pass may be reading the image. */
int ngp_nerf_dataset_set_depth(ngp_nerf_dataset* ds, uint32_t image, const void* depth_host, int dtype, float depth_scale);
/* Copies the image's depth to HOST memory (out_host nullable: only has_depth; capacity in floats, at least width *
 * height when the image has depth). has_depth (nullable): 1 when the image has a depth image, else 0 and out_host is
 * left alone. */
int ngp_nerf_dataset_depth(const ngp_nerf_dataset* ds, uint32_t image, float* out_host, uint64_t capacity, int* has_depth);
/* ngp_nerf_compute_loss with every optional input at once and the depth term (testbed_nerf.cu:1725-1748, 1848-1856,
 * 1912-1956): error_map / cdfs as in _cdf, envmap / envmap_gradient as in _envmap (envmap NULL: none), sample_state /
 * state_capacity as in _state (NULL: none) but with SIX planes, [6][state_capacity] floats: the sixth keeps the depth
 * prefix. depth_supervision_lambda > 0 on a dataset in which an image has depth: each ray also composites its samples'
 * distances from the ray origin (depth_ray), target_depth = |ray.d| * depth of the target texel (-|ray.d| for an image
 * without depth), and where target_depth > 0 the density gradient of every compacted sample takes lambda *
 * dL(target_depth, depth_ray)/d(depth_ray) * (T depth - depth suffix), the loss being depth_loss_type (ELossType). The
 * term enters neither loss[] nor the error map. With lambda 0, or no image with depth, this is the entry point without
 * it, bit for bit, and launches the same kernels. A negative or non-finite lambda or an unknown loss: NGP_INVALID. */
int ngp_nerf_compute_loss_depth(const ngp_nerf_dataset* ds, const ngp_nerf_config* cfg, void* stream, uint32_t n_rays,
                                uint32_t n_rays_total, ngp_rng rng, uint32_t max_samples_compacted,
                                const uint32_t* ray_counter, const void* network_output, const uint32_t* ray_indices,
                                const float* rays, uint32_t* numsteps, const float* coords_in, float* coords_out,
                                void* dloss_doutput, float* loss, uint32_t* compacted_counter, const float* mean_density,
                                float loss_scale, float* error_map, uint32_t em_width, uint32_t em_height,
                                const ngp_nerf_error_cdfs* cdfs, const float* envmap, uint32_t env_width,
                                uint32_t env_height, uint32_t envmap_loss_type, float* envmap_gradient, float* sample_state,
                                uint64_t state_capacity, float depth_supervision_lambda, uint32_t depth_loss_type);
/* Training::depth_supervision_lambda (default 0: off) and depth_loss_type (ELossType, default L1) of the trainer's
 * steps (testbed.h:719, 745). Only the loss pass reads them: nothing is discarded, and with lambda 0 or a dataset
 * without depth the step issues exactly the launches it would have. Works with the error-map CDFs, an environment
 * map, optimize_extrinsics and data-parallel training (the term is per ray). Sharpness stays unimplemented; an
 * image's colours are replaced with ngp_nerf_dataset_set_image. */
int ngp_nerf_trainer_set_depth_supervision(ngp_nerf_trainer* t, float lambda, uint32_t loss_type);
int ngp_nerf_trainer_get_depth_supervision(const ngp_nerf_trainer* t, float* lambda, uint32_t* loss_type);

/* ---- per-image exposure (Training::optimize_exposure, exposure_l2_reg; cam_exposure) ---------------------------- */
/* ngp_nerf_compute_loss_depth with per-image exposures (testbed_nerf.cu:1794-1818, 1973-1986). exposure (DEVICE,
 * [n_images x 3] log2 exposures; NULL: none): the target's premultiplied linear texel is multiplied by 2^exposure per
 * channel, in both colour-space branches; nothing else changes. exposure_gradient (DEVICE, [n_images x 3], nullable,
 * ADDED ONTO): for every ray that compacts to at least one sample, also one cut short by the budget,
 *   loss_scale / n_rays * (-dL/dprediction / uv_pdf [/ srgb_to_linear_derivative(target)]) * 2^exposure * ln 2
 * summed per image without atomics: the same bytes from run to run, and a second call onto the first's output gives
 * exactly twice it; an image without such a ray keeps its values. This is the reference's expression, which leaves out
 * the texel's own value (d target / d exposure = ln 2 * 2^exposure * texel). The per-image sum relies on image_idx
 * being monotone in the ray id: a gradient with cdfs->cdf_img set is NGP_INVALID, and so is one without exposures.
 * With exposure NULL this is ngp_nerf_compute_loss_depth, bit for bit, and launches the same kernels; an all-zero
 * exposure array gives the same bits too. */
int ngp_nerf_compute_loss_exposure(const ngp_nerf_dataset* ds, const ngp_nerf_config* cfg, void* stream, uint32_t n_rays,
                                   uint32_t n_rays_total, ngp_rng rng, uint32_t max_samples_compacted,
                                   const uint32_t* ray_counter, const void* network_output, const uint32_t* ray_indices,
                                   const float* rays, uint32_t* numsteps, const float* coords_in, float* coords_out,
                                   void* dloss_doutput, float* loss, uint32_t* compacted_counter, const float* mean_density,
                                   float loss_scale, float* error_map, uint32_t em_width, uint32_t em_height,
                                   const ngp_nerf_error_cdfs* cdfs, const float* envmap, uint32_t env_width,
                                   uint32_t env_height, uint32_t envmap_loss_type, float* envmap_gradient, float* sample_state,
                                   uint64_t state_capacity, float depth_supervision_lambda, uint32_t depth_loss_type,
                                   const float* exposure, float* exposure_gradient);
/* The per-image exposure optimisers (Training::cam_exposure: AdamOptimizer<vec3>, adam_optimizer.h:128-209): n_images
 * Adam states, beta1 0.9, beta2 0.99, epsilon 1e-8, initial learning rate 1e-3, which every step overwrites. Host
 * only: no GPU call. */
typedef struct ngp_exposure_optimizer ngp_exposure_optimizer;
int ngp_exposure_optimizer_create(uint32_t n_images, ngp_exposure_optimizer** out);
void ngp_exposure_optimizer_destroy(ngp_exposure_optimizer* o);
uint32_t ngp_exposure_optimizer_n_images(const ngp_exposure_optimizer* o);
int ngp_exposure_optimizer_reset(ngp_exposure_optimizer* o);
int ngp_exposure_optimizer_reset_one(ngp_exposure_optimizer* o, uint32_t i);
/* One update of every image (testbed_nerf.cu:3831-3858) from the accumulated gradients (host float [n_images x 3]):
 * gradient * n_images / 128 / n_steps_between + l2_reg * variable, an Adam step with learning rate network_lr, then
 * the mean of all variables (summed in image order, divided by n_images) subtracted from each. */
int ngp_exposure_optimizer_step(ngp_exposure_optimizer* o, const float* grad, uint32_t n_steps_between, float l2_reg,
                                float network_lr);
int ngp_exposure_optimizer_get(const ngp_exposure_optimizer* o, uint32_t i, ngp_adam_state* out);
int ngp_exposure_optimizer_set_state(ngp_exposure_optimizer* o, uint32_t i, const ngp_adam_state* state);
/* Training::optimize_exposure (default 0) and exposure_l2_reg (default 0) (testbed.h:716-785, python_api.cu:620, 634).
 * With the switch on, every step's loss pass scales the targets by the images' exposures and sums the exposure
 * gradient per image; every n_steps_between_cam_updates steps (the counter is shared with optimize_extrinsics) the
 * sums come back, the optimisers step with the network optimiser's learning rate, the mean is removed and the new
 * exposures are uploaded. Nothing the sampler reads changes: a prelaunched sampler stays. Exposures that are not zero
 * (after a snapshot or ngp_nerf_trainer_set_camera_exposure) scale the targets with the switch off too; with all of
 * them zero and the switch off the step issues exactly the launches it would without this call.
 * sample_focal_plane_proportional_to_error is allowed (the gradient is divided by uv_pdf);
 * sample_image_proportional_to_error is not (either call fails, state unchanged), and neither is a data-parallel
 * exchange hook. A negative or non-finite l2_reg: NGP_INVALID. */
int ngp_nerf_trainer_set_exposure_training(ngp_nerf_trainer* t, int optimize_exposure, float exposure_l2_reg);
int ngp_nerf_trainer_get_exposure_training(const ngp_nerf_trainer* t, int* optimize_exposure, float* exposure_l2_reg);
/* cam_exposure[i].variable(): image i's log2 exposure per channel, float[3]. */
int ngp_nerf_trainer_camera_exposure(const ngp_nerf_trainer* t, uint32_t i, float* out);
/* Engine extension: sets image i's exposure and resets that image's moments and iteration count. */
int ngp_nerf_trainer_set_camera_exposure(ngp_nerf_trainer* t, uint32_t i, const float* rgb);
int ngp_nerf_trainer_exposure_optimizer_state(const ngp_nerf_trainer* t, uint32_t i, ngp_adam_state* out);

/* ---- HDR training images (EImageDataType: image_data_type per image, read_rgba) ------------------- */
/* The reference's values (common.h:123-128). BYTE: RGBA8, sRGB with straight alpha, 4 bytes a texel, what
 * ngp_nerf_dataset_create takes. HALF: four fp16, 8 bytes. FLOAT: four fp32, 16 bytes. Half and Float texels are
 * linear, premultiplied RGBA in image order, and the loss pass uses them as they are (no sRGB decode, no alpha
 * multiply, so radiance above 1 survives); the sampler drops a ray whose texel's red is < 0, which for Byte is the
 * 0x00FF00FF texel. */
#define NGP_IMAGE_BYTE 1
#define NGP_IMAGE_HALF 2
#define NGP_IMAGE_FLOAT 3
/* ngp_nerf_dataset_create with a type per image: pixels_host[i] is HOST memory [height][width] texels of
 * image_types[i]. With every type BYTE this is ngp_nerf_dataset_create (the same bytes on the device, the same
 * kernels). ngp_nerf_generate_training_samples* and ngp_nerf_compute_loss* read the types from the dataset; with a
 * Half or Float image in it they launch their TEX instantiations, for which each ray's texel type is a run-time
 * value. NULL arguments, n_images 0 or a type other than the three: NGP_INVALID before any HIP call. */
int ngp_nerf_dataset_create_typed(uint32_t n_images, const ngp_nerf_image* images, const void* const* pixels_host,
                                  const uint32_t* image_types, ngp_nerf_dataset** out);
/* NerfDataset::set_training_image's colour part (nerf_loader.cu:907-1005): replaces image `image`'s texels by HOST
 * pixels [height][width] of image_type, at the image's existing resolution, which the call cannot change (the caller
 * passes it for checking: a width or height other than the image's is NGP_INVALID and leaves the image alone). The
 * type may change. Waits for the device first, as ngp_nerf_dataset_set_depth does, and a trainer of this dataset
 * discards the sampler it launched ahead (its mask decisions may have changed) before its next step. NULL arguments,
 * an image index out of range or an unknown type: NGP_INVALID before any HIP call. */
int ngp_nerf_dataset_set_image(ngp_nerf_dataset* ds, uint32_t image, const void* pixels_host, uint32_t image_type,
                               uint32_t width, uint32_t height);
/* Copies image `image`'s texels as stored to HOST memory and reports their type (image_type nullable; out_host
 * nullable: only the type; capacity in bytes, at least width * height * the type's texel size, else NGP_INVALID). */
int ngp_nerf_dataset_image(const ngp_nerf_dataset* ds, uint32_t image, void* out_host, uint64_t capacity, uint32_t* image_type);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif

#endif /* NGP_ENGINE_H */
