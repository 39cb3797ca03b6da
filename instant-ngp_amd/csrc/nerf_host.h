// nerf_host.h — host-side NeRF state shared between nerf_abi.hip, nerf_trainer.hip and nerf_snapshot.hip (not part of
// the C-ABI): the dataset and trainer objects behind the opaque handles, the helper types they are made of, and the
// small helpers every ngp_nerf_* entry point uses.
#pragma once
#include <cmath>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "abi_guard.h"
#include "engine_internal.h"
#include "knobs.h"
#include "nerf.h"
#include "nerf_camera.h"
#include "optimizer.h"

// private to the three sources above, which all work in these namespaces
using namespace ngp;
using namespace ngp::nerf;

struct ngp_nerf_dataset {
	Dataset ds;
};

namespace ngp {
namespace nerf {

struct HostPcg {  // tcnn::pcg32 (host) for the Testbed's m_rng / density_grid_rng
	uint64_t state, inc;
	explicit HostPcg(uint64_t initstate, uint64_t initseq = 1u) {
		state = 0u; inc = (initseq << 1u) | 1u; next_uint(); state += initstate; next_uint();
	}
	uint32_t next_uint() {
		const uint64_t old = state;
		state = old * 0x5851f42d4c957f2dULL + inc;
		const uint32_t xs = (uint32_t)(((old >> 18u) ^ old) >> 27u), rot = (uint32_t)(old >> 59u);
		return (xs >> rot) | (xs << ((~rot + 1u) & 31));
	}
	void advance(uint64_t delta = (1ull << 32)) {
		uint64_t cm = 0x5851f42d4c957f2dULL, cp = inc, am = 1u, ap = 0u;
		while (delta > 0) {
			if (delta & 1) { am *= cm; ap = ap * cm + cp; }
			cp = (cm + 1) * cp; cm *= cm; delta /= 2;
		}
		state = am * state + ap;
	}
	Rng dev() const { return Rng{state, inc}; }
};

struct Buf {
	void* p = nullptr;
	size_t n = 0;
	template <typename T> T* get(size_t count) {
		const size_t need = count * sizeof(T);
		if (need > n) {
			if (p) NGP_HIP(hipFree(p));
			NGP_HIP(hipMalloc(&p, need));
			n = need;
		}
		return (T*)p;
	}
	~Buf() { if (p) (void)hipFree(p); }
};

// One cross-queue handoff: the producer's stream signals, the consumer's stream waits for the latest signal. By
// event, or by value (hipStreamWriteValue32 / hipStreamWaitValue32 on signal memory): a queue idling on a pending
// event wait starts its next kernel ~10 us after the event's work ends, on a pending value wait ~6 us; a wait that
// finds its signal complete costs ~1.3 us by event against ~3.6 by value (tools/microbench/queue_handoff.hip,
// profiles/r06s_queue_handoff.jsonl; sampler -> inference by value: Lego step 0.433 -> 0.428 ms, fox 0.542 -> 0.535).
struct Handoff {
	bool by_value = false;
	hipEvent_t ev = nullptr;
	uint32_t* sig = nullptr;  // signal memory: only a by-value handoff allocates it
	uint32_t seq = 0;
	void signal(hipStream_t producer) {
		if (by_value) {
			if (!sig) {
				NGP_HIP(hipExtMallocWithFlags((void**)&sig, 8, hipMallocSignalMemory));
				NGP_HIP(hipMemset(sig, 0, 8));
			}
			NGP_HIP(hipStreamWriteValue32(producer, sig, ++seq, 0));
		} else {
			if (!ev) NGP_HIP(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
			NGP_HIP(hipEventRecord(ev, producer));
		}
	}
	void wait(hipStream_t consumer) const {
		if (!sig && !ev) return;  // never signalled: nothing to wait for
		if (by_value) NGP_HIP(hipStreamWaitValue32(consumer, sig, seq, hipStreamWaitValueGte, 0xFFFFFFFFu));
		else NGP_HIP(hipStreamWaitEvent(consumer, ev, 0));
	}
	~Handoff() {
		if (ev) (void)hipEventDestroy(ev);
		if (sig) (void)hipFree(sig);
	}
};

inline bool envmap_dims_ok(uint32_t w, uint32_t h) { return w >= 1 && h >= 1 && w <= 8192 && h <= 8192; }
inline bool distortion_dims_ok(uint32_t w, uint32_t h) { return envmap_dims_ok(w, h); }  // the same bounds

// ngp_nerf_error_cdfs -> ErrorCdfs (null: none). The position CDFs come as a pair with a resolution; without
// cdf_x_cond_y the other two members are not looked at.
inline bool error_cdfs_arg(const ngp_nerf_error_cdfs* c, ErrorCdfs* out) {
	*out = ErrorCdfs{};
	if (!c) return true;
	out->cdf_img = c->cdf_img;
	if (c->cdf_x_cond_y) {
		if (!c->cdf_y || c->width == 0 || c->height == 0) return false;
		out->cdf_x_cond_y = c->cdf_x_cond_y; out->cdf_y = c->cdf_y; out->w = c->width; out->h = c->height;
	}
	return true;
}

// The loss pass (compute_loss, nerf.h) and the sampler (sample_rays) behind the C-ABI's null checks, with their
// scratch buffers; the caller fills the arguments by field name. n_rays_total_for_image_idx 0 means n_rays.
// cams (optional): the device cameras to trace instead of the dataset's.
// exposure_grad: also take the rays' exposure gradients (a.exposure bound), kept behind the per-ray scratch: the pointer
// comes back in *exposure_ray_grad for exposure_gradients, and holds until the thread's next loss pass.
int run_compute_loss(const ngp_nerf_dataset* ds, const ngp_nerf_config* cfg, void* stream, LossArgs a, bool exposure_grad = false,
                     const float** exposure_ray_grad = nullptr);
// dist (optional): the distortion map the rays are traced through
int run_sampler(const ngp_nerf_dataset* ds, const ngp_nerf_config* cfg, void* stream, SampleArgs a, const Camera* cams,
                const DistMap* dist = nullptr);

}  // namespace nerf
}  // namespace ngp

struct ngp_nerf_trainer {
	const NerfKnobs knobs = NerfKnobs::read();  // at creation (knobs.h)
	ngp_model* model;
	ngp_trainer* trainer;
	const ngp_nerf_dataset* data;
	ngp_nerf_config cfg;
	HostPcg rng{1337}, grid_rng{1};
	uint32_t training_step = 0, ema_step = 0;
	uint32_t rays_per_batch = 1u << 12;  // testbed.h:440
	uint32_t n_rays_total = 0;
	uint32_t measured_batch_size = 0, measured_before_compaction = 0;
	uint32_t measured_before_compaction_local = 0;  // this rank's pre-compaction count (inference sizing)
	float loss_scalar = 0.f;  // m_loss_scalar (last step that computed the loss)
	// the training pass (forward_backward + optimizer over the fixed compacted batch) replayed as one
	// HIP graph per step; re-captured if its buffers move
	ngp_graph* train_graph = nullptr;
	const void* graph_in = nullptr;
	const void* graph_dl = nullptr;
	uint32_t graph_n = 0;
	uint64_t graph_epoch = 0;  // model workspace epoch at capture (ngp_model_workspace_epoch)
	hipStream_t own_stream = nullptr;  // used when the caller passes the null stream (graphs need a stream)
	// per-step counters published by the step's last kernel into host-coherent pinned memory, read by
	// spinning on a sequence number (no copy-engine transfer, no blocking stream synchronize)
	volatile uint32_t* host_ctr = nullptr;
	uint32_t publish_seq = 0;
	// Sampler pipelining: the next step's ray sampling depends on the occupancy bitfield, the rng and the
	// rays-per-batch count, not on the network, so (when no density-grid update is due before it) it is
	// launched on `sample_stream` as soon as this step's loss pass has released the sample buffers and
	// runs concurrently with this step's training pass. Same kernels, same inputs: same samples.
	bool pipeline = true;                // ngp_nerf_trainer_set_pipeline
	bool prelaunched = false;
	uint32_t pre_R = 0, pre_max_inference = 0;
	// Dataset::image_epoch the last step saw: ngp_nerf_dataset_set_image may have changed which texels are masked, so
	// the next step discards a sampler launched before it. (The captured training pass holds no dataset pointer.)
	uint64_t data_epoch = 0;
	hipStream_t sample_stream = nullptr;
	// prelaunched sampler -> this step's inference (the consumer is usually already waiting: by value), and the step's
	// release of the sample buffers -> the next sampler (long done when the host launches that sampler: by event; the
	// release by value too: Lego 0.427, fox 0.538 ms; not used under early())
	Handoff sampled{knobs.waitval != 0}, released{knobs.waitval == 2};
	// Density-grid update pipelining: when the next step is due an update, its sample generation and bin sort read
	// only the grid (unchanged until that update) and the grid rng, so they run on `sample_stream` under this step's
	// training pass, after the update before it (grid_updated: that one wrote the grid they read and read the buffers
	// they write); the update then starts at the density evaluation (pregenerated). Discarding them restores the rng.
	bool grid_pregen = false;
	uint32_t pregen_nu = 0, pregen_nn = 0;
	Handoff pregenerated, grid_updated;
	HostPcg pregen_rng{1};  // grid_rng before the pregenerated samples
	void drain() {  // the prelaunched sampler finished and discarded (state is about to change)
		if (sample_stream) (void)hipStreamSynchronize(sample_stream);
		prelaunched = false;
		if (grid_pregen) grid_rng = pregen_rng;
		grid_pregen = false;
	}
	~ngp_nerf_trainer() {
		drain();
		if (train_graph) ngp_graph_destroy(train_graph);
		if (own_stream) (void)hipStreamDestroy(own_stream);
		if (sample_stream) (void)hipStreamDestroy(sample_stream);
		if (host_ctr) (void)hipHostFree((void*)host_ctr);
		if (d_cams) (void)hipFree(d_cams);
		if (d_raw) (void)hipFree(d_raw);
		ngp_pose_optimizer_destroy(pose);
		ngp_exposure_optimizer_destroy(expo);
	}
	// data parallelism: rank r traces global rays [R r / N, R (r+1) / N), compacts to B / N,
	// evaluates 1/N of the density-grid samples; the exchange steps go through `allreduce`
	uint32_t rank = 0, world = 1;
	ngp_allreduce_fn allreduce = nullptr;
	void* allreduce_user = nullptr;
	bool dp_capturable = false;  // the hook is the engine's RCCL communicator: the DP training pass is a graph
	Buf dp_scalars;
	bool dp() const { return allreduce != nullptr; }
	// the training pass's exchange: the shards' dL/doutput is already scaled by 128 / R_global, so the summed
	// gradient is the 1-GPU gradient (world factor 1)
	ngp::Exchange exchange() const {
		ngp::Exchange e;
		e.fn = allreduce; e.user = allreduce_user; e.rank = rank; e.world = world; e.world_factor = 1.f;
		e.rank_known = allreduce != nullptr;
		return e;
	}
	// occupancy grid
	Buf grid, grid_tmp, bitfield, mean, gpos, gidx, gdens, grid_mask, splat_scratch, gpos_sorted;
	// training workspaces
	Buf mlp_out, dloss, coords_c, loss, scan_tmp, tmp_u32, tmp_f32;
	struct SampleSet { Buf ray_indices, rays, numsteps, coords, counters; } sets[2];  // the second one: early()
	// Early publish (one GPU): the counters are published by the loss's scan, so the host launches the next step's
	// sampler while this step's loss pass 2, rollover and training pass still run; the sampler's outputs then
	// alternate between two sets by step parity (the set it writes was last read two steps before), so it waits on
	// nothing. Default under cone stepping only (aabb_scale > 1: the count pass, ~1.5x the training pass, is the
	// step's critical path; fox 0.517 -> 0.499 ms); at cone 0 the two are balanced and a count pass already resident
	// when the training pass starts keeps its one-wave-per-SIMD MLP kernel off the SIMDs (Lego 0.421 -> 0.440 ms,
	// gpurun_out/r06bd). NGP_NERF_EARLY=1: always, 0: never (publish in the rollover, one set, the sampler waits
	// for this step's release).
	bool early() const {
		const bool on = knobs.early < 0 ? cfg.cone_angle_constant > 1e-5f : knobs.early != 0;
		return on && !dp();
	}
	// The sampler's outputs alternate between the two sets: under early publish, and with camera pose refinement, whose
	// gradient kernels read the ray buffers after the training pass: the next sampler, prelaunched under that pass,
	// then writes the other set (last read by the step before this one, complete once this step's counters are
	// published) instead of waiting for this step's release
	bool two_sets() const { return early() || ((cam.optimize_extrinsics != 0 || dist.optimize) && !dp()); }
	Buf loss_state;  // compute_loss: pass 1's per-sample compositing state for pass 2 (LossArgs::state)
	// depth supervision (ngp_nerf_trainer_set_depth_supervision): off at 0, or while no image of the dataset has depth
	float depth_lambda = 0.0f;
	uint32_t depth_loss_type = LOSS_L1;
	// Camera pose refinement (Testbed::Nerf::Training::optimize_extrinsics and its neighbours, testbed.h:716-785). The
	// trainer traces its own device copy of the cameras: the dataset's array to begin with (bit for bit), rebuilt from
	// `xforms` and the per-camera offsets (ngp_pose_apply, then effective_camera_matrix) whenever those change; d_raw
	// is the raw-transform array mark_untrained_density_grid reads, refreshed the same way.
	ngp_nerf_camera_training cam{0, 16, 1e-4f, 1e-3f};
	ngp_pose_optimizer* pose = nullptr;
	std::vector<float> xforms;   // [n_images x 12] the transforms the offsets apply to (set_camera_extrinsics writes them)
	std::vector<Camera> cams;    // host mirror of d_cams
	Camera* d_cams = nullptr;
	float* d_raw = nullptr;
	uint32_t n_steps_since_cam_update = 0;
	Buf cam_grad, cam_ray_grad, dinput;  // [2][n_images x 3] accumulators {pos, rot}; per-ray workspace; dL/dinput [B x 7]
	const float* graph_dinput = nullptr;  // the gradient pointer the training graph was captured with
	// Per-image exposure (Training::optimize_exposure, exposure_l2_reg, cam_exposure; testbed_nerf.cu:3831-3858): the
	// optimisers' variables are mirrored in expo_dev [n_images x 3] once an exposure is not zero or the switch is on
	// (expo_bound), and the loss pass then runs its exposure form; with the switch on it also takes the gradient, summed
	// per image into expo_grad, which starts from zero after every update. The update shares n_steps_since_cam_update
	// with pose refinement. The sampler reads none of this.
	bool optimize_exposure = false;
	float exposure_l2_reg = 0.0f;
	ngp_exposure_optimizer* expo = nullptr;
	Buf expo_dev, expo_grad;
	bool expo_bound = false;
	std::vector<float> expo_host;  // the upload's source: written only after the stream that read it was waited for
	void upload_exposures(hipStream_t s);
	// the last step's sampler call, for ngp_nerf_trainer_last_samples
	ngp_rng last_rng{0, 0};
	uint32_t last_n_rays = 0, last_max_samples = 0;
	const uint32_t* last_ray_indices = nullptr;
	const float* last_rays = nullptr;
	const uint32_t* last_counters = nullptr;
	void refined_xform(uint32_t i, float out[12]) const;
	void rebuild_cameras(hipStream_t s);
	// training error map (Testbed::Nerf::Training::ErrorMap and its update window, testbed.h:668-677, 736-738)
	Buf em_data, em_cdf_x, em_cdf_y, em_cdf_img;
	uint32_t em_w = 0, em_h = 0, em_cdf_w = 0, em_cdf_h = 0;
	uint32_t em_steps_since = 0, em_steps_between = 128;
	bool em_cdf_valid = false;
	std::vector<float> em_pmf_img;  // pmf_img_cpu
	// Error-driven sampling (Training::sample_focal_plane_proportional_to_error / sample_image_proportional_to_error,
	// testbed.h:733-734): once a window has closed, a step's sampler and its loss pass draw the rays' pixels from the
	// CDFs of the last closed window (testbed_nerf.cu:3948-3949). Both off: the uniform kernels, nothing else changes.
	bool sample_focal_plane_by_error = false, sample_image_by_error = false;
	bool error_sampling() const { return sample_focal_plane_by_error || sample_image_by_error; }
	// Environment map (Testbed::m_envmap and Training::train_envmap; testbed.cu:4133-4147, testbed_nerf.cu:3668-3685):
	// fp32 RGBA parameters [h][w][4] behind every training ray, their EMA for rendering, and with `train` on a
	// gradient summed exactly per step (envmap.h) and an optimizer step of their own after every loss pass. Not set:
	// the step issues exactly the launches it would without any of this.
	struct Envmap {
		uint32_t w = 0, h = 0;
		Buf params, ema, ema_out, m1, m2, steps, grad, acc;
		uint32_t step = 0;         // optimizer steps taken
		bool ema_valid = false;    // ema_out holds the debiased EMA of a step under an Ema wrapper (or a snapshot's)
		AdamConfig opt;            // the "envmap" section's optimizer; opt_set false: the main trainer's
		bool opt_set = false;
		int32_t loss_type = -1;    // the "envmap" section's loss; -1: cfg.loss_type
		bool train = false;
		size_t n() const { return (size_t)w * h * 4; }
		bool bound() const { return w != 0; }
	} env;
	const AdamConfig& envmap_optimizer() const { return env.opt_set ? env.opt : trainer_adam_config(trainer); }
	uint32_t envmap_loss_type() const { return env.loss_type < 0 ? cfg.loss_type : (uint32_t)env.loss_type; }
	// what rendering reads (inference_view): the debiased EMA once a step has been taken under an Ema wrapper
	const float* envmap_inference() const {
		return (const float*)(env.ema_valid ? env.ema_out.p : env.params.p);
	}
	// Lens distortion map (Testbed::m_distortion and Training::optimize_distortion; testbed.cu:4066-4076,
	// testbed_nerf.cu:2088-2099, 3811-3818; distortion.h): fp32 parameters [h][w][2], the offset the trainer's sampler adds
	// to every ray's dir.xy whenever a map is bound, whether `optimize` is on or off. With `optimize` on the step takes the
	// input gradient as pose refinement does, deposits every kept ray's image-plane gradient into the exact accumulator
	// `acc`, which starts from zero after every update, and every n_steps_between_cam_updates steps (the counter shared
	// with poses and exposure) turns it into `grad` and steps the map's optimizer on the step's stream. Not bound: the
	// step issues exactly the launches it would without any of this.
	struct Distortion {
		uint32_t w = 0, h = 0;
		Buf params, ema, ema_out, m1, m2, steps, grad, acc, ray_grad;
		uint32_t step = 0;          // optimizer steps taken
		bool ema_valid = false;     // ema_out holds the debiased EMA (an optimizer with an Ema wrapper has stepped)
		AdamConfig opt;             // the "distortion_map" section's optimizer; opt_set false: the main trainer's
		bool opt_set = false;
		uint32_t def_w = 32, def_h = 32;  // the section's resolution: the map `optimize` creates when none is bound
		bool optimize = false;
		size_t n() const { return (size_t)w * h * 2; }
		bool bound() const { return w != 0; }
		DistMap view() const { return DistMap{bound() ? (const float*)params.p : nullptr, w, h}; }
	} dist;
	const AdamConfig& distortion_optimizer() const { return dist.opt_set ? dist.opt : trainer_adam_config(trainer); }
	const float* distortion_inference() const { return (const float*)(dist.ema_valid ? dist.ema_out.p : dist.params.p); }
	ErrorCdfs sampling_cdfs() const {
		ErrorCdfs e{};
		if (!em_cdf_valid || !em_cdf_w || !em_cdf_h) return e;
		if (sample_image_by_error) e.cdf_img = (const float*)em_cdf_img.p;
		if (sample_focal_plane_by_error) {
			e.cdf_x_cond_y = (const float*)em_cdf_x.p; e.cdf_y = (const float*)em_cdf_y.p;
			e.w = em_cdf_w; e.h = em_cdf_h;
		}
		return e;
	}
};
