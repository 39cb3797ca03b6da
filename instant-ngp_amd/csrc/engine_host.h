// engine_host.h — the model / trainer objects behind the opaque handles of the C-ABI (include/ngp_engine.h), shared
// between engine_model.hip, engine_trainer.hip and engine_shard.hip and private to them (the other units see
// engine_internal.h). Data members, one-line predicates and accessors; every member that launches, allocates or
// records events is defined in one of the three units.
//
// Mirrors the tcnn object graph the reference's Testbed builds in reset_network
// (src/testbed.cu:3903-4151): NerfNetwork = position GridEncoding -> density FullyFusedMLP ->
// [density out | SH(dir)] -> rgb FullyFusedMLP; NetworkWithInputEncoding = encoding -> MLP;
// Trainer = fp32 master weights + fp16 params/inference params/gradients + optimizer state.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstring>
#include <memory>
#include <string>

#include "abi_guard.h"
#include "engine_internal.h"
#include "grid_scatter.h"
#include "grid.h"
#include "json.h"
#include "mlp.h"
#include "optimizer.h"
#include "profiler.h"
#include "training.h"

namespace ngp {

// Growable device buffer (grows outside the hot loop; ngp_model_reserve pre-sizes it).
// Every reallocation bumps *epoch (the owning model's workspace epoch): a captured HIP graph holds raw
// workspace pointers, so graph launches check the epoch they were captured at.
struct DevBuf {
	void* p = nullptr;
	size_t bytes = 0;
	uint64_t* epoch = nullptr;
	void* get(size_t need) {
		if (need > bytes) {
			if (p) NGP_HIP(hipFree(p));
			p = nullptr;
			NGP_HIP(hipMalloc(&p, need));
			NGP_HIP(hipMemset(p, 0, need));  // workspaces that must start zeroed (the grid backward's brick fallback table)
			bytes = need;
			if (epoch) ++*epoch;
		}
		return p;
	}
	~DevBuf() { if (p) (void)hipFree(p); }
};

// Optional parts of a backward pass (ngp_model::train_pass)
struct BwdExtra {
	float* dL_dinput = nullptr;     // fp32 AoS [n x dinput_stride]: rows 0..D-1 (+ the direction rows of a NerfNetwork)
	uint32_t dinput_stride = 0;
	float dinput_scale = 1.f;
	bool density_only = false;      // NerfNetwork::density_backward: the density network alone
	const f16* ddens = nullptr;     // its dL/d(density output), fp16 AoS [n x ddens_stride]
	uint32_t ddens_stride = 0;
	bool inference = false;         // the forward context ran on the inference (EMA) parameters: so does the backward
};

// One launch of the MLP (ngp_model::run_mlp); a caller sets the fields its mode reads. ngp_model::train_pass takes
// the batch in the same fields (n, coords, enc, out, dL_dout and their strides) and fills in the rest itself.
struct MlpCall {
	MlpMode mode = MLP_INFER;
	uint32_t n = 0;
	const float* coords = nullptr;  // fp32 AoS [n x coord_stride]
	uint32_t coord_stride = 0;
	const f16* enc = nullptr;       // the encoding, AoS [n x enc_width] (MLP_INFER_ENC: none, the kernel encodes)
	f16* out = nullptr;
	uint32_t out_stride = 0, out_layout = AoS;
	const f16* dL_dout = nullptr;
	uint32_t dL_stride = 0;
	f16* dL_denc = nullptr;
	float* slab = nullptr;          // the training blocks' dW slabs
	f16* dL_dsh = nullptr;
	bool inference = false;         // run on the inference (EMA) parameters
	const BwdExtra* ex = nullptr;
};

}  // namespace ngp

using namespace ngp;

struct ngp_ctx {
	uint32_t n;
	const float* input;
	uint32_t input_stride;
	bool use_inference_params;
	uint64_t generation;  // the model workspace generation the encoding lives in
	bool density_only = false;  // from ngp_density_forward: only ngp_density_backward may consume it
};

struct ngp_model {
	bool nerf = true;
	GridDesc grid;
	uint32_t n_pos_dims = 3, n_dir_dims = 3, n_extra_dims = 0, dir_offset = 4, n_input_dims = 3, n_output_dims = 4;
	uint32_t enc_width = 16;
	NerfMlpPlan nplan;
	MlpPlan mplan;
	uint64_t mlp0_params = 0, mlp1_params = 0, grid_params = 0, n_params = 0;
	FragDesc* d_descs = nullptr;
	uint32_t* d_fragmap = nullptr;  // [n_matrix x 2] fragment slot (f16 index) of each matrix param: fwd, bwd
	bool frags_current = false;     // `frags` holds the fragments of the current `params` (kept by the optimizer)
	uint32_t n_all_frags = 0;
	DevBuf frags, frags_inf, enc, denc, slabs, scatter_ws, out_ws, dl_ws, dsh_ws, dl1_ws;
	int grid_backward_mode = 0;  // 0 auto, 1 direct (tcnn-style), 3 bucketed (grid_scatter.h)
	uint32_t win_debug = 0;      // timing experiments only (see grid_scatter.h)
	ScatterPlan sc_plan;
	uint32_t sc_plan_n = 0;
	bool sc_prepared = false;               // phase 1 of the bucketed backward already enqueued (side stream)
	bool sc_hist_done = false;              // the training forward produced the bucket histogram
	bool frags_async = false;               // training fragments already enqueued on the side stream
	// side-stream overlap (bitmask): 1 bucket histogram under forward + MLP, 2 weight fragments,
	// 4 dW slab reduction under the grid backward, 8 optimizer step advance. Each costs a cross-queue
	// dependency edge, which in a HIP graph is not free.
	uint32_t overlap = 0;
	bool fused_hist = true;                 // option "fused_hist": bucket histogram inside the training forward
	bool fuse_infer = true;                 // option "fuse_infer": NerfNetwork inference encodes inside the MLP kernel
	bool fuse_slabs = true;                 // option "fuse_slabs": dW slab reduction inside the grid backward's last kernel
	bool fuse_opt = true;                   // option "fuse_opt": lazy-layout optimizer update inside the grid backward (training_step)
	bool fuse_mlp_opt = true;               // option "fuse_mlp_opt": ... and the MLP section's update in its dW slab blocks (no optimizer launch)
	bool grid_bricks = false;               // option "grid_bricks": dense levels of the bucketed backward summed per brick (off: measured slower)
	bool grid_direct = true;                // option "grid_direct": levels of at most two buckets summed without items (ScatterPlan::direct_mask)
	bool grid_plan_inline = false;          // option "grid_plan_inline": no k_sc_plan launch where the bucket list is small (ScatterPlan::plan_inline; off: measured slower)
	const ScatterKnobs sc_knobs = ScatterKnobs::read();  // NGP_SC_*: a set switch overrides the three options above
	ScatterOpts scatter_opts(bool bricks) const { return ScatterOpts{bricks, grid_direct, grid_plan_inline, sc_knobs}; }
	hipStream_t side = nullptr;             // overlaps fragments + bucket histogram with forward + MLP,
	                                        // and the dW slab reduction with the grid backward
	hipEvent_t ev_fork = nullptr, ev_join = nullptr, ev_frags = nullptr, ev_mlp = nullptr, ev_red = nullptr;
	f16 *params = nullptr, *inference_params = nullptr, *gradients = nullptr;
	// lazy-EMA trainer: brings the inference (EMA) parameters up to date before they are read
	void (*inference_hook)(void*, hipStream_t) = nullptr;
	void* inference_hook_ctx = nullptr;
	void sync_inference(hipStream_t s) { if (inference_hook) inference_hook(inference_hook_ctx, s); }
	float max_level = 1.0f;
	const float* max_level_per_sample = nullptr;
	// false: the last training pass did not write the fp16 gradient buffer (the grid's update ran inside the
	// backward, or the backward stored the gradient as fp32 for the sharded exchange): ngp_trainer_gradients_valid
	bool grads_valid = true;
	// the sharded exchange's consumer of the grid backward's parts (BwdParts): set by the trainer around one
	// training pass, used when the bucketed backward runs without bricks or the fused update
	const BwdParts* bwd_parts = nullptr;
	bool parts_ok(uint32_t n) const {
		return use_sorted(n) && fuse_slabs && !(overlap & 4) && !grid_bricks && grid.n_features >= 2;
	}
	uint64_t generation = 0;
	uint64_t ws_epoch = 0;  // bumped by every workspace reallocation (DevBuf::epoch)
	std::unique_ptr<ngp_ctx> last_ctx;

	ngp_model() {
		for (DevBuf* b : {&frags, &frags_inf, &enc, &denc, &slabs, &scatter_ws, &out_ws, &dl_ws, &dsh_ws, &dl1_ws}) b->epoch = &ws_epoch;
	}

	~ngp_model() {
		if (d_descs) (void)hipFree(d_descs);
		if (d_fragmap) (void)hipFree(d_fragmap);
		for (hipEvent_t e : {ev_fork, ev_join, ev_frags, ev_mlp, ev_red})
			if (e) (void)hipEventDestroy(e);
		if (side) (void)hipStreamDestroy(side);
	}
	// allocate every buffer a training pass over n samples touches (nothing may allocate during graph capture)
	void reserve(uint32_t n);
	void ensure_side_stream();
	bool use_sorted(uint32_t n) const { return grid_backward_mode == 3 || (grid_backward_mode == 0 && n >= 4096); }
	// the backward can store the whole gradient as fp32 itself (FusedAdam::g32): bucketed grid backward with the
	// dW slab reduction in its last kernel
	bool grad32_ok(uint32_t n) const { return use_sorted(n) && fuse_slabs && !(overlap & 4) && grid.n_features >= 2; }
	bool side_prepare(uint32_t n) const { return use_sorted(n) && (overlap & 1); }
	const ScatterPlan& sc_plan_for(uint32_t n);
	// The brick levels' fallback table must be zero when a backward adds into it (each finalize clears the
	// entries it reads, so it stays zero between steps of one plan). A new plan moves it (its offset follows
	// the item regions, sized by the batch): zero it once on the stream before the plan's first backward.
	bool fb_dirty = true;
	void clear_brick_fallback(hipStream_t s, void* ws);
	void* sorted_workspace(uint32_t n) { return scatter_ws.get(sc_plan_for(n).total); }
	// Phase 1 of the bucketed grid backward on a side stream: it only needs the positions, so it runs
	// concurrently with the forward encoding and the MLP; train_pass joins before the scatter.
	void prepare_grid_backward_async(hipStream_t s, uint32_t n, const float* in, uint32_t stride);

	const std::vector<FragDesc>& descs() const { return nerf ? nplan.descs : mplan.descs; }
	uint64_t grid_offset() const { return mlp0_params + mlp1_params; }
	uint64_t n_matrix() const { return mlp0_params + mlp1_params; }

	void finalize();
	void require_params(bool inference) const {
		NGP_CHECK(inference ? inference_params != nullptr : params != nullptr,
		          "model has no parameters: call ngp_model_set_params or create a trainer first");
	}
	const f16* pick(bool inference) const { return inference ? inference_params : params; }
	bool fused_encoding_ok() const {
		return nerf && !max_level_per_sample && nerf_mlp_fused_encoding_ok(grid, enc_width) && nplan.enc_steps == 1 &&
		       nplan.d_hidden == 1 && nplan.r_hidden >= 1 && nplan.r_hidden <= 3;
	}
	bool fused_inference_ok() const { return fuse_infer && fused_encoding_ok(); }
	f16x8* prep(hipStream_t s, bool inference);
	// want_hist: a training forward whose backward follows on the same positions — count the sorted
	// backward's bucket histogram in the forward kernel (its corner indices are computed anyway).
	void encode(hipStream_t s, uint32_t n, const float* in, uint32_t stride, f16* out, uint32_t out_stride, uint32_t layout, bool inference,
	            bool want_hist = false);
	void run_mlp(hipStream_t s, const MlpCall& c);
	// backward given the encoding already in `b.enc`: MLP fwd+bwd (+output), dW slabs, grid scatter.
	// ex (optional): input gradients and the density-only backward (BwdExtra); grad_mode NGP_GRAD_IGNORE
	// leaves the parameter gradients untouched (tcnn EGradientMode::Ignore, input_gradient).
	void train_pass(hipStream_t s, const MlpCall& b, int grad_mode, const BwdExtra& ex = BwdExtra{}, const FusedAdam* fopt = nullptr);
	// Hash-grid backward: destination-bucketed exact sums (n >= 4096, or mode 3), else tcnn-style direct
	// packed-f16 atomics (small batches, where the bucket plan costs more than the atomics).
	void scatter_grid_grad(hipStream_t s, GridBwdArgs b, bool overwrite, const SlabJob* slab = nullptr, const FusedAdam* fopt = nullptr);
};

struct ngp_trainer {
	ngp_model* model = nullptr;
	const TrainerKnobs knobs = TrainerKnobs::read();  // at every creation (knobs.h)
	AdamConfig cfg;
	uint32_t step = 0;
	uint64_t n = 0;
	void* arena = nullptr;
	float *w32 = nullptr, *m1 = nullptr, *m2 = nullptr, *ema32 = nullptr;
	f16 *w16 = nullptr, *inf16 = nullptr, *g16 = nullptr;
	uint32_t* steps = nullptr;
	float* bias_tab = nullptr;  // adam_bias_table for cfg.beta1/beta2 (built at creation)
	// lazy-EMA layout (optimizer.h AdamRec), chosen for large tables: a step touches only the state of
	// updated parameters; the inference (EMA) parameters are brought up to date when read
	AdamRec* rec = nullptr;
	bool inf_stale = false;
	// lazy layout: the fp32 weights live in the records (AdamRec::w); w32 is their mirror, stale after a step
	bool w32_stale = false;
	void sync_w32();
	void materialize(hipStream_t s, bool force = false);
	static void materialize_hook(void* self, hipStream_t s) { ((ngp_trainer*)self)->materialize(s); }
	void bind_model();
	uint32_t* ctl = nullptr;  // device {optimizer step, block counter, .., AdamConfig at ctl + CTL_CFG}; `step` mirrors ctl[0]
	ngp_allreduce_fn allreduce = nullptr;  // gradient exchange inside captured steps (ngp_trainer_set_allreduce)
	void* allreduce_user = nullptr;
	uint32_t world = 1;
	// sharded optimizer (ngp_trainer_set_data_parallel): this rank, the fp32 gradient staging of the
	// reduce-scatter [n_pad] and the parameter count padded to a multiple of 8 world (w16 and the records
	// are allocated with SHARD_PAD spare parameters for it)
	static constexpr uint64_t SHARD_PAD = 2048;
	uint32_t dp_rank = 0;
	bool dp_rank_known = false;
	bool shard_opt = true;       // trainer option "shard_opt"
	bool shards_valid = true;    // false: a sharded step left other ranks' records stale here (gather_shards)
	float* g32 = nullptr;
	uint64_t g32_count = 0;
	uint64_t n_pad = 0;
	// The exchange in parameter parts (trainer option "dp_parts"): part j = parameters [pb[j], pb[j + 1]), multiples
	// of 8 world; rank r owns the r-th of the world equal slices of every part. Each part is reduce-scattered,
	// its slice updated and all-gathered as soon as the backward has summed it (BwdParts), on the exchange
	// stream xs, while the backward sums the next part. Default 1 part: measured at world 1 the parted
	// step costs 35-40 us more (the bucket ranges' own launches, and the step's graph runs the two streams' work in
	// sequence), more than the overlap could hide at N = 8 under DESIGN §7's bandwidth model.
	uint32_t dp_parts = 1;
	bool dp_wire16 = false;      // option "dp_wire16": reduce-scatter the fp16 gradient (half the bytes; rounded per hop)
	std::vector<uint64_t> pb;
	hipStream_t xs = nullptr;
	hipEvent_t ev_part[BwdParts::MAX] = {}, ev_xs = nullptr;
	struct PartStep {  // one sharded step's exchange state (issue_part)
		hipStream_t s = nullptr;
		ngp::Exchange e;
		float loss_scale = 1.f;
		const uint32_t* step_base = nullptr;
		uint32_t step_add = 0;
		bool wire16 = false, overlap = false;
		uint32_t issued = 0;
		int rc = NGP_OK;
	} ps_;
	BwdParts bparts;
	~ngp_trainer() {
		if (arena) (void)hipFree(arena);
		if (bias_tab) (void)hipFree(bias_tab);
		if (g32) (void)hipFree(g32);
		for (hipEvent_t ev : ev_part)
			if (ev) (void)hipEventDestroy(ev);
		if (ev_xs) (void)hipEventDestroy(ev_xs);
		if (xs) (void)hipStreamDestroy(xs);
	}
	ngp::Exchange exchange() const {
		ngp::Exchange e;
		e.fn = allreduce; e.user = allreduce_user; e.rank = dp_rank; e.world = world; e.world_factor = (float)world;
		e.rank_known = dp_rank_known;
		return e;
	}
	// the sharded optimizer applies to this exchange: the lazy layout owning the model's buffers, rank known
	bool sharded(const ngp::Exchange& e) const {
		return e.fn && e.rank_known && shard_opt && rec && g32 && e.world == world && model->params == w16 &&
		       model->gradients == g16 && !pb.empty();
	}
	void require_full_state(const char* what) const {
		if (!shards_valid)
			throw Error(std::string(what) + ": the optimizer state is sharded over the data-parallel ranks; call "
			            "ngp_trainer_gather_shards on every rank first");
	}
	// part bounds for `world` ranks: dp_parts parts of about n_pad / dp_parts, multiples of 8 world
	void make_part_bounds(uint32_t w);
	void ensure_exchange_stream();
	// this rank's slice of part j, clamped to the parameters
	void part_slice(uint32_t j, uint64_t& lo, uint64_t& hi) const {
		const uint64_t c = (pb[j + 1] - pb[j]) / world;
		lo = std::min<uint64_t>(pb[j] + (uint64_t)dp_rank * c, n);
		hi = std::min<uint64_t>(lo + c, n);
	}
	// the MLP section lies in this rank's slice of part 0: the update keeps its weight fragments current
	bool mlp_owned() const {
		uint64_t lo, hi;
		part_slice(0, lo, hi);
		return lo == 0 && hi >= model->n_matrix();
	}
	// Exchange + update of part j (sharded step): reduce-scatter of the summed gradient, this rank's slice of the
	// records updated from the sums (fp32 wire: rounded to fp16 once, as the all-reduce path narrows; fp16 wire:
	// RCCL's per-hop fp16 sum), all-gather of the slice's fp16 weights. On xs behind an event when the backward
	// hands the parts over while it runs, else on the step's stream.
	void issue_part(uint32_t j);
	static void part_done(void* self, uint32_t j, hipStream_t) { ((ngp_trainer*)self)->issue_part(j); }
	// Before a sharded step's training pass: the exchange state, and the backward's parts when it can hand them
	// over (bucketed backward storing the fp32 gradient, or the fp16 one for the fp16 wire): returns them for
	// ngp_model::bwd_parts, or nullptr (then every part is exchanged after the backward).
	// stores_input: the backward writes the wire's input itself (fp32 wire: the fp32 store, FusedAdam::g32).
	const BwdParts* begin_shard_step(hipStream_t s, float loss_scale, const ngp::Exchange& e, const uint32_t* step_base,
	                                 uint32_t step_add, uint32_t n_batch, bool stores_input);
	// After the training pass: the parts the backward did not hand over, the join of the exchange stream, the MLP's
	// fragments from the gathered weights where another rank updated them.
	int shard_step(bool stored);
	void sync_device_step() { NGP_HIP(hipMemcpy(ctl, &step, sizeof(uint32_t), hipMemcpyHostToDevice)); }
	// One optimizer step on stream s. step_base/step_add: see AdamState (optimizer.h).
	// n_first: parameters [0, n_first) only (the MLP, when the grid's update ran fused in the backward)
	void run_step(hipStream_t s, float loss_scale, const uint32_t* step_base, uint32_t step_add, uint64_t n_first = 0);
	// The grid's lazy update fused into the backward (model option fuse_opt): lazy layout, no gradient
	// exchange (the all-reduce needs the stored gradients), the sorted backward, F >= 2, and an MLP
	// section that is a whole number of 4-parameter groups (k_adam_lazy4 then runs on it alone).
	bool fused_update_ok(uint32_t n_batch) const {
		const ngp_model* m = model;
		return rec && !allreduce && m->fuse_opt && m->use_sorted(n_batch) && m->grid.n_features >= 2 && m->n_matrix() % 4 == 0 &&
		       m->grid_offset() % 2 == 0 && m->params == w16 && m->gradients == g16;
	}
	FusedAdam fused_update(float loss_scale, uint32_t n_batch) const;
	// With the grid's update fused (fused_update_ok), the MLP section's update runs in the dW slab blocks of
	// the grid backward's last kernel when the slab reduction is fused there (model options fuse_slabs,
	// fuse_mlp_opt; not under the side-stream reduction, overlap bit 4): no optimizer launch.
	bool mlp_opt_in_backward(uint32_t n_batch) const {
		const ngp_model* m = model;
		return m->fuse_mlp_opt && m->fuse_slabs && !(m->overlap & 4) && m->use_sorted(n_batch) && m->n_matrix() > 0;
	}
	void mlp_step_done() {  // run_step's bookkeeping when the update ran in the backward
		if (rec) inf_stale = w32_stale = true;
	}
	// The optimizer's share of one training step over n_batch samples (ngp_trainer_training_step, train_step_body),
	// on both sides of its backward. step_tail: the grid's update runs inside the backward where possible (may_fuse:
	// the optimizer runs and no exchange needs the stored gradients; fused_update_ok), its gradient is then not
	// stored. step_base = the ctl block (captured: the step is the device base + k, hyperparameters read from the
	// ctl block) or nullptr (eager: host step + k). finish_step: the optimizer launch, over the MLP section alone
	// after a fused grid update, or none where the backward updated that section too.
	struct StepTail {
		bool fuse = false;
		FusedAdam fa;  // fuse: the update the backward runs
		float loss_scale = 1.f;
		const uint32_t* step_base = nullptr;
		uint32_t step_add = 0;
	};
	StepTail step_tail(bool may_fuse, float loss_scale, const uint32_t* step_base, uint32_t k, uint32_t n_batch) const;
	void finish_step(hipStream_t s, const StepTail& q);
};

// A captured training step (forward_backward + optimizer) replayed as one HIP graph launch.
struct ngp_graph {
	hipGraph_t graph = nullptr;
	hipGraphExec_t exec = nullptr;
	ngp_trainer* trainer = nullptr;
	uint32_t steps_per_launch = 1;
	uint64_t ws_epoch = 0;  // the model's workspace epoch at capture
	// the graph holds a sharded exchange over world > 1 ranks: every launch leaves the other ranks' optimizer
	// records stale on this rank again (ngp_trainer_gather_shards)
	bool shards_stale = false;
	// the graph's backward writes the gradient for the sharded exchange as fp32 only: g16 is not written
	bool g16_stale = false;
	void launched() {
		trainer->step += steps_per_launch;
		if (steps_per_launch && trainer->rec) trainer->inf_stale = trainer->w32_stale = true;
		if (shards_stale) trainer->shards_valid = false;
		if (g16_stale) trainer->model->grads_valid = false;
	}
	~ngp_graph() {
		if (exec) (void)hipGraphExecDestroy(exec);
		if (graph) (void)hipGraphDestroy(graph);
	}
};
