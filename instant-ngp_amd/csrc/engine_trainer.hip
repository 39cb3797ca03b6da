// engine_trainer.hip — the trainer behind the C-ABI (include/ngp_engine.h): the optimizer's JSON, creation, the
// optimizer step and its fused forms, training_step and the eager and captured train steps, the accessors, options
// and the serialized state. The sharded exchange of a data-parallel step is engine_shard.hip.
#include "engine_host.h"

static void parse_optimizer(const Json& j, AdamConfig& c) {
	const std::string ot = j.string_or("otype", "Adam");
	if (iequals(ot, "Ema")) {
		c.ema_decay = (float)j.number_or("decay", 0.99);
		parse_optimizer(j["nested"], c);
	} else if (iequals(ot, "ExponentialDecay")) {
		c.decay_start = (uint32_t)j.number_or("decay_start", 0);
		c.decay_interval = (uint32_t)j.number_or("decay_interval", 10000);
		c.decay_base = (float)j.number_or("decay_base", 0.1);
		parse_optimizer(j["nested"], c);
	} else if (iequals(ot, "Adam")) {
		c.lr = (float)j.number_or("learning_rate", 1e-3);
		c.beta1 = (float)j.number_or("beta1", 0.9);
		c.beta2 = (float)j.number_or("beta2", 0.999);
		c.eps = (float)j.number_or("epsilon", 1e-8);
		c.l2 = (float)j.number_or("l2_reg", 1e-8);
	} else {
		throw Error("optimizer: unsupported otype " + ot + " (Ema / ExponentialDecay / Adam implemented)");
	}
}

void ngp::parse_optimizer_json(const char* json, AdamConfig& c) { parse_optimizer(Json::parse(json), c); }
const AdamConfig& ngp::trainer_adam_config(const ngp_trainer* t) { return t->cfg; }

void ngp_trainer::sync_w32() {
	if (!rec || !w32_stale) return;
	require_full_state("full-precision weights");
	NGP_HIP(hipDeviceSynchronize());  // the optimizer may still run on a caller's non-blocking stream
	adam_rec_weights((uint32_t)n, rec, w32, false, nullptr);
	NGP_HIP(hipDeviceSynchronize());
	w32_stale = false;
}
void ngp_trainer::materialize(hipStream_t s, bool force) {
	if (!rec || (!inf_stale && !force)) return;
	require_full_state("inference (EMA) parameters");
	AdamState st{w32, w16, g16, nullptr, nullptr, nullptr, nullptr, inf16, nullptr, nullptr, nullptr, 0, nullptr, rec};
	ema_materialize(cfg, (uint32_t)n, step, st, s);
	inf_stale = false;
}
void ngp_trainer::bind_model() {
	ngp_model_set_params(model, w16, cfg.ema_decay > 0.f ? inf16 : w16, g16);
	if (rec) { model->inference_hook = materialize_hook; model->inference_hook_ctx = this; }
}
void ngp_trainer::run_step(hipStream_t s, float loss_scale, const uint32_t* step_base, uint32_t step_add, uint64_t n_first) {
	ngp_model* m = model;
	const bool own = m->params == w16;
	// captured steps (step_base = ctl) read the hyperparameters from the ctl block, which every graph
	// launch refreshes with the step: set_learning_rate / set_option reach replayed steps too
	AdamState st{w32, w16, g16, m1, m2, steps, ema32, inf16,
	             own && m->frags_current ? (f16*)m->frags.p : nullptr, m->d_fragmap, step_base, step_add,
	             step_base ? (const AdamConfig*)(ctl + CTL_CFG) : nullptr, rec, bias_tab};
	ProfScope ps("optimizer", s);
	adam_ema_update(cfg, (uint32_t)(n_first ? n_first : n), (uint32_t)m->n_matrix(), loss_scale, st, s);
	if (rec) inf_stale = w32_stale = true;
}
FusedAdam ngp_trainer::fused_update(float loss_scale, uint32_t n_batch) const {
	FusedAdam fa;
	const uint64_t go = model->grid_offset();
	fa.w16 = w16 + go; fa.rec = rec + go / 2;
	fa.loss_scale = loss_scale; fa.cfg = cfg; fa.step_add = step;
	fa.bias_tab = bias_tab;
	if (mlp_opt_in_backward(n_batch)) {
		fa.mlp_n = (uint32_t)model->n_matrix();
		fa.mlp_w16 = w16;
		fa.mlp_rec = rec;
	}
	return fa;
}
ngp_trainer::StepTail ngp_trainer::step_tail(bool may_fuse, float loss_scale, const uint32_t* step_base, uint32_t k,
                                             uint32_t n_batch) const {
	StepTail q;
	q.fuse = may_fuse && fused_update_ok(n_batch);
	q.loss_scale = loss_scale; q.step_base = step_base; q.step_add = step_base ? k : step + k;
	if (q.fuse) {
		q.fa = fused_update(loss_scale, n_batch);
		q.fa.step_base = step_base;
		q.fa.step_add = q.step_add;
		if (step_base) q.fa.cfg_dev = (const AdamConfig*)(ctl + CTL_CFG);
	}
	return q;
}
void ngp_trainer::finish_step(hipStream_t s, const StepTail& q) {
	if (q.fa.mlp_n) mlp_step_done();
	else run_step(s, q.loss_scale, q.step_base, q.step_add, q.fuse ? model->n_matrix() : 0);
}

// One training step as the captured graph runs it: forward_backward (the grid's lazy update fused into the
// backward where possible, ngp_trainer::step_tail), [gradient exchange: one all-reduce, or the sharded
// reduce-scatter / slice update / all-gather], optimizer. step_base = the trainer's ctl block (captured: the step
// is the device base + k, hyperparameters read from the ctl block) or nullptr (eager: host step + k).
static int train_step_body(ngp_trainer* t, void* stream, const StepBatch& b, int with_optimizer, const Exchange& ex,
                           const uint32_t* step_base, uint32_t k) {
	ngp_model* m = t->model;
	// the grid's update inside the backward where possible (lazy layout, no exchange): as training_step
	ngp_trainer::StepTail q = t->step_tail(with_optimizer && !ex.fn, b.loss_scale * ex.world_factor, step_base, k, b.n);
	const bool shard = with_optimizer && t->sharded(ex);
	// sharded: the backward writes the fp32 reduce-scatter input itself where it can (no widening pass); with the
	// fp16 wire it stores the fp16 gradient as usual
	const bool direct32 = shard && !t->dp_wire16 && m->grad32_ok(b.n);
	if (direct32) q.fa.g32 = t->g32;
	int rc = NGP_OK;
	if (shard) {
		try {
			// the exchange of each part starts as soon as the backward has summed it (BwdParts)
			m->bwd_parts = t->begin_shard_step(S(stream), q.loss_scale, ex, step_base, q.step_add, b.n, direct32);
		} catch (const std::exception& e) {
			set_last_error(e.what());
			rc = NGP_ERROR;
		}
	}
	if (rc == NGP_OK)
		rc = forward_backward_with(m, stream, b.n, b.input, b.input_stride, nullptr, 0, b.dL_doutput, b.dL_stride, NGP_GRAD_OVERWRITE,
		                           q.fuse || direct32 ? &q.fa : nullptr, b.dL_dinput, b.dL_dinput_stride);
	m->bwd_parts = nullptr;
	if (rc == NGP_OK && ex.fn) {
		try {
			// the summed gradient of the ranks: the mean (or, NeRF, the 1-GPU gradient) via the loss scale
			rc = shard ? t->shard_step(direct32) : ex.fn(ex.user, t->g16, t->n, NGP_DTYPE_F16, NGP_REDUCE_SUM, stream);
		} catch (const std::exception& e) {
			set_last_error(e.what());
			rc = NGP_ERROR;
		}
		if (rc != NGP_OK && !*ngp_last_error()) set_last_error("gradient exchange failed");
	}
	if (rc == NGP_OK && with_optimizer && !shard) {
		try {
			t->finish_step(S(stream), q);
		} catch (const std::exception& e) {
			set_last_error(e.what());
			rc = NGP_ERROR;
		}
	}
	return rc;
}

int ngp::train_step_with(ngp_trainer* t, void* stream, const StepBatch& batch, const Exchange& ex) {
	const auto& [n, input, input_stride, dL_doutput, dL_stride, loss_scale, dL_dinput, dL_dinput_stride] = batch;
	NGP_ARG(t && n > 0 && input && dL_doutput && loss_scale > 0.f && (const float*)dL_dinput != input);
	NGP_TRY({
		ngp_model* m = t->model;
		m->require_params(false);
		NGP_CHECK(m->gradients == t->g16, "train_step: the model's gradient buffer must be this trainer's");
		if (train_step_body(t, stream, batch, 1, ex, nullptr, 0) != NGP_OK) throw Error(ngp_last_error());
		t->step++;
	});
}

// The capture with an explicit gradient exchange hook and world factor (ngp_trainer_capture_training_step
// passes the trainer's own; the data-parallel NeRF trainer passes its communicator with world factor 1,
// because its shards' dL/doutput is already scaled by 128 / R_global, so the summed gradient is the
// 1-GPU gradient).
int ngp::capture_training_step_with(ngp_trainer* t, void* stream, const StepBatch& batch, uint32_t n_steps, int with_optimizer,
                                    const Exchange& ex, ngp_graph** out) {
	const auto& [n, input, input_stride, dL_doutput, dL_stride, loss_scale, dL_dinput, dL_dinput_stride] = batch;
	NGP_ARG(t && out && stream && n > 0 && input && dL_doutput && loss_scale > 0.f && n_steps >= 1 && ex.world >= 1 &&
	        (const float*)dL_dinput != input);
	NGP_TRY({
		ngp_model* m = t->model;
		m->require_params(false);
		NGP_CHECK(m->gradients == t->g16, "capture: the model's gradient buffer must be this trainer's");
		m->reserve(n);
		if (dL_dinput && m->nerf) m->dsh_ws.get((size_t)n * 16 * sizeof(f16));  // train_pass: dL/d(SH) of the input gradient
		hipStream_t s = S(stream);
		auto g = std::make_unique<ngp_graph>();
		g->trainer = t;
		g->steps_per_launch = with_optimizer ? n_steps : 0;
		NGP_HIP(hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal));
		int rc = NGP_OK;
		for (uint32_t k = 0; k < n_steps && rc == NGP_OK; ++k)
			rc = train_step_body(t, stream, batch, with_optimizer, ex, t->ctl, k);  // step = device base (set per launch) + k
		hipGraph_t graph = nullptr;
		const hipError_t end = hipStreamEndCapture(s, &graph);
		g->ws_epoch = m->ws_epoch;
		g->shards_stale = with_optimizer && t->sharded(ex) && ex.world > 1;
		g->g16_stale = !m->grads_valid;
		if (rc != NGP_OK) {
			if (graph) (void)hipGraphDestroy(graph);
			throw Error(ngp_last_error());
		}
		NGP_HIP(end);
		g->graph = graph;
		NGP_HIP(hipGraphInstantiate(&g->exec, g->graph, nullptr, nullptr, 0));
		*out = g.release();
	});
}
void ngp::trainer_ctl_values(const ngp_trainer* t, uint32_t** ctl, uint32_t* step, uint32_t* cfg_off, uint32_t* cfg_words, uint32_t* cfg) {
	static_assert(sizeof(AdamConfig) % 4 == 0 && sizeof(AdamConfig) <= 32 * 4, "AdamConfig as at most 32 words");
	*ctl = t->ctl;
	*step = t->step;
	*cfg_off = CTL_CFG;
	*cfg_words = sizeof(AdamConfig) / 4;
	memcpy(cfg, &t->cfg, sizeof(AdamConfig));
}
void ngp::graph_launch_ctl_written(ngp_graph* g, void* stream) {
	NGP_CHECK(g && g->exec, "graph launch: no graph");
	NGP_CHECK(g->ws_epoch == g->trainer->model->ws_epoch, "graph launch: the model's workspaces were reallocated (or its options changed) since capture");
	NGP_HIP(hipGraphLaunch(g->exec, S(stream)));
	g->launched();
}

__global__ static void k_f32_to_f16(const float* a, f16* b, f16* c, uint64_t n) {
	const uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
	if (i < n) { b[i] = (f16)a[i]; c[i] = (f16)a[i]; }
}

extern "C" {

int ngp_trainer_create(ngp_model* m, const char* optimizer_json, uint64_t seed, ngp_trainer** out) {
	NGP_ARG(m && out);
	NGP_TRY({
		auto t = std::make_unique<ngp_trainer>();
		t->model = m;
		if (optimizer_json) parse_optimizer(Json::parse(optimizer_json), t->cfg);
		if (t->knobs.ema_closed_form != KNOB_UNSET) t->cfg.ema_closed_form = t->knobs.ema_closed_form != 0;  // A/B runs
		// the betas are fixed for the trainer's lifetime (only the learning rate has a setter)
		NGP_HIP(hipMalloc(&t->bias_tab, (size_t)BIAS_TAB_CAP * 2 * sizeof(float)));
		adam_bias_table(t->bias_tab, t->cfg.beta1, t->cfg.beta2, nullptr);
		NGP_HIP(hipDeviceSynchronize());
		const uint64_t n = m->n_params;
		t->n = n;
		auto al = [](size_t b) { return (b + 255) / 256 * 256; };
		// w16 and the records carry SHARD_PAD spare parameters: the sharded optimizer pads to a multiple of 8 world
		const size_t b32 = al(n * 4), b16 = al((n + ngp_trainer::SHARD_PAD) * 2);
		// lazy-EMA records from 2^20 parameters (C5: 105 M parameters, ~28 % updated per step; C2' 13 M: captured
		// step 351 -> 330 us with the fused update, profiles/r03bw; C2, 3.3 M parameters, ~96 % updated: pass
		// 147.5 us with both updates in the backward, against 163.0 us on the eager arrays and 183.3 us with the
		// lazy layout's separate launch, one box and session, profiles/r09a_bench_c2_ab.json; round 4's 140.6-142.8
		// -> 136.0 us was measured while the bench's gradients were zero); the eager arrays for small
		// models. NGP_LAZY_EMA=0/1 forces the choice.
		bool lazy = n >= (1ull << 20);
		if (t->knobs.lazy_ema != KNOB_UNSET) lazy = t->knobs.lazy_ema != 0;
		lazy = lazy && n % 4 == 0;
		const size_t brec = al((n + ngp_trainer::SHARD_PAD) / 2 * sizeof(AdamRec));
		const size_t total = b32 + (lazy ? brec : 4 * b32) + 3 * b16 + 256 /*ctl*/;
		NGP_HIP(hipMalloc(&t->arena, total));
		char* p = (char*)t->arena;
		t->w32 = (float*)p; p += b32;
		if (lazy) {
			t->rec = (AdamRec*)p; p += brec;
		} else {
			t->m1 = (float*)p; p += b32;
			t->m2 = (float*)p; p += b32;
			t->ema32 = (float*)p; p += b32;
			t->steps = (uint32_t*)p; p += b32;
		}
		t->w16 = (f16*)p; p += b16;
		t->inf16 = (f16*)p; p += b16;
		t->g16 = (f16*)p; p += b16;
		t->ctl = (uint32_t*)p; p += 256;
		NGP_HIP(hipMemset(t->arena, 0, total));
		std::vector<float> host(n);
		check_rc(ngp_model_initialize_params(m, seed, host.data(), 1.0f));
		*out = t.release();
		check_rc(ngp_trainer_set_params_full_precision(*out, host.data(), n));
	});
}

void ngp_trainer_destroy(ngp_trainer* t) {
	if (!t) return;
	if (t->model && t->model->params == t->w16) ngp_model_set_params(t->model, nullptr, nullptr, nullptr);
	delete t;
}

int ngp_trainer_optimizer_step(ngp_trainer* t, void* stream, float loss_scale) {
	NGP_ARG(t && loss_scale > 0.f);
	NGP_TRY({
		t->run_step(S(stream), loss_scale, nullptr, t->step);
		t->step++;
	});
}

int ngp_loss_evaluate(int loss_type, void* stream, uint32_t n, uint32_t dims, const void* output, uint32_t output_stride,
                      const float* target, uint32_t target_stride, float loss_scale, void* dL_doutput, uint32_t dL_stride,
                      float* values, float* loss_sum) {
	NGP_ARG(loss_type >= 0 && (n == 0 || (output && target && dL_doutput)));
	NGP_TRY({
		LossEvalArgs a{n, dims, (const f16*)output, output_stride, target, target_stride, loss_scale, (f16*)dL_doutput, dL_stride,
		               values, loss_sum};
		loss_evaluate((uint32_t)loss_type, a, S(stream));
	});
}

// tcnn::Trainer::training_step(stream, input, target, data_pdf = nullptr, run_optimizer)
// (src/testbed_image.cu:276, src/testbed_sdf.cu:1304): forward -> loss -> backward [-> optimizer].
// The fused MLP kernel needs dL/doutput up front, so the forward runs once as inference (output for
// the loss) and once more inside the backward (recompute instead of stored activations).
int ngp_trainer_training_step(ngp_trainer* t, void* stream, uint32_t n, const float* input, uint32_t input_stride,
                              const float* target, uint32_t target_stride, int loss_type, float loss_scale, int run_optimizer,
                              float* loss_sum) {
	NGP_ARG(t && (n == 0 || (input && target)) && loss_scale > 0.f && loss_type >= 0);
	NGP_TRY({
		if (n == 0) return NGP_OK;
		ngp_model* m = t->model;
		m->require_params(false);
		NGP_CHECK(m->gradients == t->g16, "training_step: the model's gradient buffer must be this trainer's");
		hipStream_t s = S(stream);
		const uint32_t W = 16;  // padded_output_width (nerf_network.h:463-465; FullyFusedMLP pads to 16)
		f16* e = (f16*)m->enc.get((size_t)n * m->enc_width * sizeof(f16));
		f16* out = (f16*)m->out_ws.get((size_t)n * W * sizeof(f16));
		f16* dl = (f16*)m->dl_ws.get((size_t)n * W * sizeof(f16));
		m->generation++;
		m->encode(s, n, input, input_stride, e, m->enc_width, AoS, false, true);
		MlpCall c;
		c.mode = MLP_INFER; c.n = n; c.coords = input; c.coord_stride = input_stride; c.enc = e; c.out = out; c.out_stride = W;
		m->run_mlp(s, c);
		LossEvalArgs la{n, m->n_output_dims, out, W, target, target_stride, loss_scale, dl, W, nullptr, loss_sum};
		{
			ProfScope ps("loss", s);
			loss_evaluate((uint32_t)loss_type, la, s);
		}
		// the grid's optimizer update runs inside the backward where possible (fused_update_ok): its
		// gradient is then not stored, and the optimizer launch covers the MLP section alone
		const ngp_trainer::StepTail q = t->step_tail(run_optimizer, loss_scale, nullptr, 0, n);
		MlpCall b;
		b.n = n; b.coords = input; b.coord_stride = input_stride; b.enc = e; b.dL_dout = dl; b.dL_stride = W;
		m->train_pass(s, b, NGP_GRAD_OVERWRITE, BwdExtra{}, q.fuse ? &q.fa : nullptr);
		if (run_optimizer) {
			t->finish_step(s, q);
			t->step++;
		}
	});
}

int ngp_trainer_capture_training_step(ngp_trainer* t, void* stream, uint32_t n, const float* input, uint32_t input_stride,
                                      const void* dL_doutput, uint32_t dL_stride, float loss_scale, uint32_t n_steps,
                                      int with_optimizer, ngp_graph** out) {
	NGP_ARG(t);
	StepBatch b;
	b.n = n; b.input = input; b.input_stride = input_stride; b.dL_doutput = dL_doutput; b.dL_stride = dL_stride; b.loss_scale = loss_scale;
	return ngp::capture_training_step_with(t, stream, b, n_steps, with_optimizer, t->exchange(), out);
}

int ngp_trainer_train_step(ngp_trainer* t, void* stream, uint32_t n, const float* input, uint32_t input_stride,
                           const void* dL_doutput, uint32_t dL_stride, float loss_scale) {
	NGP_ARG(t);
	StepBatch b;
	b.n = n; b.input = input; b.input_stride = input_stride; b.dL_doutput = dL_doutput; b.dL_stride = dL_stride; b.loss_scale = loss_scale;
	return ngp::train_step_with(t, stream, b, t->exchange());
}

int ngp_trainer_train_step_input_gradient(ngp_trainer* t, void* stream, uint32_t n, const float* input, uint32_t input_stride,
                                          const void* dL_doutput, uint32_t dL_stride, float loss_scale, float* dL_dinput,
                                          uint32_t dL_dinput_stride) {
	NGP_ARG(t && dL_dinput);
	StepBatch b;
	b.n = n; b.input = input; b.input_stride = input_stride; b.dL_doutput = dL_doutput; b.dL_stride = dL_stride; b.loss_scale = loss_scale;
	b.dL_dinput = dL_dinput; b.dL_dinput_stride = dL_dinput_stride;
	return ngp::train_step_with(t, stream, b, t->exchange());
}

int ngp_trainer_fused_update_active(const ngp_trainer* t, uint32_t n_batch) {
	return t && !t->allreduce && t->fused_update_ok(n_batch) ? 1 : 0;
}

int ngp_graph_launch(ngp_graph* g, void* stream) {
	NGP_ARG(g && g->exec);
	NGP_TRY({
		NGP_CHECK(g->ws_epoch == g->trainer->model->ws_epoch,
		          "graph launch: the model's workspaces were reallocated since capture (a larger batch or a density "
		          "pass grew them); capture again (ngp_model_workspace_epoch tells when)");
		if (g->steps_per_launch) set_device_ctl(g->trainer->ctl, g->trainer->step, g->trainer->cfg, S(stream));
		NGP_HIP(hipGraphLaunch(g->exec, S(stream)));
		g->launched();
	});
}

void ngp_graph_destroy(ngp_graph* g) { delete g; }

void* ngp_trainer_gradients(ngp_trainer* t) { return t ? t->g16 : nullptr; }
int ngp_trainer_gradients_valid(const ngp_trainer* t) {
	return t && t->model->gradients == t->g16 && t->model->grads_valid ? 1 : 0;
}
void* ngp_trainer_params(ngp_trainer* t) { return t ? t->w16 : nullptr; }
void* ngp_trainer_inference_params(ngp_trainer* t) {
	if (!t) return nullptr;
	if (t->rec && t->inf_stale) {  // lazy EMA: bring the inference parameters up to date before handing them out
		try {
			NGP_HIP(hipDeviceSynchronize());  // the optimizer may still run on a caller's non-blocking stream
			t->materialize(nullptr);
			NGP_HIP(hipDeviceSynchronize());
		} catch (const std::exception& e) {
			set_last_error(e.what());
			return nullptr;
		}
	}
	return t->cfg.ema_decay > 0.f ? t->inf16 : t->w16;
}
// Lazy layout: the mirror of the records' weights, refreshed here (a read accessor: writes into it do not reach
// the records; set_params_full_precision does, as in tcnn).
float* ngp_trainer_params_full_precision(ngp_trainer* t) {
	if (!t) return nullptr;
	try {
		t->sync_w32();
		// the caller may write into the mirror: it is not the master copy, so the next reader (serialize, this
		// accessor) refreshes it from the records again instead of trusting it
		if (t->rec) t->w32_stale = true;
	} catch (const std::exception& e) {
		set_last_error(e.what());
		return nullptr;
	}
	return t->w32;
}
uint32_t ngp_trainer_step(const ngp_trainer* t) { return t ? t->step : 0; }
uint64_t ngp_trainer_n_params(const ngp_trainer* t) { return t ? t->n : 0; }
float ngp_trainer_learning_rate(const ngp_trainer* t) { return t ? t->cfg.lr_at(t->step) : 0.f; }
int ngp_trainer_set_learning_rate(ngp_trainer* t, float lr) {
	NGP_ARG(t && lr >= 0.f);
	NGP_TRY({ t->cfg.lr = lr; });
}
// Trainer options (engine extension). "ema_closed_form": 0 (default) = the lazy layout's owed EMA steps are
// replayed exactly (optimizer.h ema_catch_up: bit for bit the eager layout), 1 = closed form for gaps of more
// than 32 steps (A/B and the tolerance test only).
int ngp_trainer_set_option(ngp_trainer* t, const char* key, double value) {
	NGP_ARG(t && key);
	NGP_TRY({
		const std::string k = key;
		if (k == "ema_closed_form") {
			t->cfg.ema_closed_form = value != 0 ? 1u : 0u;
		} else if (k == "shard_opt") {
			NGP_CHECK(t->shards_valid, "shard_opt: gather the sharded optimizer state first (ngp_trainer_gather_shards)");
			t->shard_opt = value != 0;
		} else if (k == "dp_parts") {
			NGP_CHECK(t->shards_valid, "dp_parts: gather the sharded optimizer state first (ngp_trainer_gather_shards)");
			NGP_CHECK(value >= 1 && value <= BwdParts::MAX, "dp_parts: 1 to 8");
			t->dp_parts = (uint32_t)value;
			if (t->n_pad) t->make_part_bounds(t->world);
		} else if (k == "dp_wire16") {
			t->dp_wire16 = value != 0;
		} else {
			throw Error("ngp_trainer_set_option: unknown option " + k);
		}
	});
}

int ngp_trainer_set_params_full_precision(ngp_trainer* t, const float* params_host, uint64_t n) {
	NGP_ARG(t && params_host && n == t->n);
	NGP_TRY({
		t->require_full_state("set_params_full_precision");
		if (t->rec && t->step > 0) {
			// lazy EMA: entries skipped since their last update still owe EMA steps on the OLD weight (the eager
			// layout applied them every step). Replay them before the weights change; the records are then
			// current (done = step), as every eager EMA is.
			NGP_HIP(hipDeviceSynchronize());
			t->materialize(nullptr, true);
			NGP_HIP(hipDeviceSynchronize());
		}
		NGP_HIP(hipMemcpy(t->w32, params_host, n * 4, hipMemcpyHostToDevice));
		k_f32_to_f16<<<div_round_up(n, 256), 256>>>(t->w32, t->w16, t->inf16, n);
		NGP_HIP(hipGetLastError());
		if (t->rec) adam_rec_weights((uint32_t)n, t->rec, t->w32, true, nullptr);
		NGP_HIP(hipDeviceSynchronize());
		t->inf_stale = t->w32_stale = false;  // inference parameters = the new weights, as in the eager layout
		t->bind_model();
	});
}

// Blob: magic, version, n, step, then w32, m1, m2, ema32 (f32), steps (u32)
int ngp_trainer_serialize(ngp_trainer* t, void* buf, uint64_t* size) {
	NGP_ARG(t && size);
	NGP_TRY({
		const uint64_t need = 32 + t->n * 4 * 5;
		if (!buf) { *size = need; return NGP_OK; }
		t->require_full_state("serialize");
		NGP_CHECK(*size >= need, "serialize: buffer too small");
		char* p = (char*)buf;
		const uint64_t hdr[4] = {0x4e47504d49333535ULL /* "NGPMI355" */, 1, t->n, t->step};
		memcpy(p, hdr, 32); p += 32;
		NGP_HIP(hipDeviceSynchronize());
		if (t->rec) t->w32_stale = true;  // lazy layout: the blob's weights always come from the records
		t->sync_w32();
		DevBuf soa;
		float *m1 = t->m1, *m2 = t->m2, *ema32 = t->ema32;
		uint32_t* steps = t->steps;
		if (t->rec) {  // lazy layout: every EMA brought up to date, then the eager arrays of the blob
			t->materialize(nullptr);
			char* q = (char*)soa.get(t->n * 16);
			m1 = (float*)q; m2 = (float*)(q + t->n * 4); ema32 = (float*)(q + t->n * 8); steps = (uint32_t*)(q + t->n * 12);
			adam_rec_to_soa((uint32_t)t->n, t->rec, m1, m2, ema32, steps, nullptr);
			NGP_HIP(hipDeviceSynchronize());
		}
		for (void* src : {(void*)t->w32, (void*)m1, (void*)m2, (void*)ema32, (void*)steps}) {
			NGP_HIP(hipMemcpy(p, src, t->n * 4, hipMemcpyDeviceToHost));
			p += t->n * 4;
		}
		*size = need;
	});
}

int ngp_trainer_deserialize(ngp_trainer* t, const void* buf, uint64_t size) {
	NGP_ARG(t && buf);
	NGP_TRY({
		const char* p = (const char*)buf;
		uint64_t hdr[4];
		NGP_CHECK(size >= 32, "deserialize: truncated");
		memcpy(hdr, p, 32); p += 32;
		NGP_CHECK(hdr[0] == 0x4e47504d49333535ULL && hdr[1] == 1, "deserialize: bad magic/version");
		NGP_CHECK(hdr[2] == t->n && size >= 32 + t->n * 20, "deserialize: parameter count mismatch");
		t->step = (uint32_t)hdr[3];
		t->sync_device_step();
		DevBuf soa;
		float *m1 = t->m1, *m2 = t->m2, *ema32 = t->ema32;
		uint32_t* steps = t->steps;
		if (t->rec) {
			char* q = (char*)soa.get(t->n * 16);
			m1 = (float*)q; m2 = (float*)(q + t->n * 4); ema32 = (float*)(q + t->n * 8); steps = (uint32_t*)(q + t->n * 12);
		}
		for (void* dst : {(void*)t->w32, (void*)m1, (void*)m2, (void*)ema32, (void*)steps}) {
			NGP_HIP(hipMemcpy(dst, p, t->n * 4, hipMemcpyHostToDevice));
			p += t->n * 4;
		}
		if (t->rec) {
			adam_soa_to_rec((uint32_t)t->n, m1, m2, ema32, steps, t->step, t->rec, nullptr);
			adam_rec_weights((uint32_t)t->n, t->rec, t->w32, true, nullptr);
		}
		t->inf_stale = t->w32_stale = false;  // inference parameters = the restored weights (below), as in the eager layout
		t->shards_valid = true;              // every record restored on every rank
		k_f32_to_f16<<<div_round_up(t->n, 256), 256>>>(t->w32, t->w16, t->inf16, t->n);
		NGP_HIP(hipGetLastError());
		NGP_HIP(hipDeviceSynchronize());
		t->model->frags_current = false;
	});
}

}  // extern "C"
