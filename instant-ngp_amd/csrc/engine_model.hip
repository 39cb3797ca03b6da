// engine_model.hip — the model behind the C-ABI (include/ngp_engine.h): parameter initialisation and the JSON of its
// encoding and networks, ngp_model's passes (encode, run_mlp, train_pass, the grid backward), the ngp_model_* /
// ngp_forward* / ngp_backward* entry points, and the library's error string and device wrappers.
#include "engine_host.h"

static_assert(ngp::DENSITY_LAYOUT_ROW0 == ngp::MLP_LAYOUT_ROW0, "the row-0 density layout of mlp.h and engine_internal.h");

namespace ngp {

int device_cu_count() {
	static int cached = -1;
	if (cached < 0) {
		int dev = 0;
		NGP_HIP(hipGetDevice(&dev));
		NGP_HIP(hipDeviceGetAttribute(&cached, hipDeviceAttributeMultiprocessorCount, dev));
	}
	return cached;
}

// ---- pcg32 (tcnn::pcg32, random_val.cuh:26-43) used for parameter initialisation -------------
struct Pcg32 {
	uint64_t state = 0x853c49e6748fea9bULL, inc = 0xda3e39cb94b95bdbULL;
	static constexpr uint64_t MULT = 0x5851f42d4c957f2dULL;
	Pcg32(uint64_t initstate, uint64_t initseq = 1u) {
		state = 0u; inc = (initseq << 1u) | 1u; next_uint(); state += initstate; next_uint();
	}
	uint32_t next_uint() {
		uint64_t old = state;
		state = old * MULT + inc;
		uint32_t xs = (uint32_t)(((old >> 18u) ^ old) >> 27u), rot = (uint32_t)(old >> 59u);
		return (xs >> rot) | (xs << ((~rot + 1u) & 31));
	}
	float next_float() { uint32_t u = (next_uint() >> 9) | 0x3f800000u; float f; memcpy(&f, &u, 4); return f - 1.0f; }
	void advance(uint64_t delta) {
		uint64_t cm = MULT, cp = inc, am = 1u, ap = 0u;
		while (delta > 0) {
			if (delta & 1) { am *= cm; ap = ap * cm + cp; }
			cp = (cm + 1) * cp; cm *= cm; delta /= 2;
		}
		state = am * state + ap;
	}
	// tcnn generate_random_uniform: element k takes draw k of the stream; the caller advances by n
	void uniform(size_t n, float* out, float lo, float hi) {
		Pcg32 r = *this;
		for (size_t k = 0; k < n; ++k) out[k] = r.next_float() * (hi - lo) + lo;
		advance(n);
	}
};

static void init_mlp(const MlpDims& d, Pcg32& rng, float* p, float scale) {
	for (uint32_t l = 0; l <= d.n_hidden; ++l) {
		const uint32_t in = d.layer_in(l), out = d.layer_out(l);
		const float s = sqrtf(6.0f / (float)(in + out)) * scale;  // Xavier-uniform
		rng.uniform((size_t)in * out, p + d.layer_off(l), -s, s);
	}
}

// tcnn's GridEncoding otypes: HashGrid (= Grid with type Hash) and DenseGrid (= Grid with type Dense, e.g.
// configs/nerf/densegrid.json). A dense level holds res^D entries (rounded to 8) with no hashmap cap, so its
// stride never exceeds its size and grid_index never hashes: the hash-grid kernels run it unchanged with the
// cap lifted (GRID_LOG2_DENSE). TiledGrid is not implemented.
static GridDesc parse_grid(uint32_t n_dims, const Json& j) {
	const std::string ot = j.string_or("otype", "HashGrid");
	NGP_CHECK(iequals(ot, "HashGrid") || iequals(ot, "DenseGrid") || iequals(ot, "Grid"),
	          "encoding: HashGrid and DenseGrid are implemented (got " + ot + ")");
	const std::string type = j.string_or("type", iequals(ot, "DenseGrid") ? "Dense" : "Hash");
	NGP_CHECK(iequals(type, "Hash") || iequals(type, "Dense"), "encoding: grid type Hash or Dense (got " + type + ")");
	const std::string interp = j.string_or("interpolation", "Linear");
	NGP_CHECK(iequals(interp, "Linear") || iequals(interp, "Smoothstep"),
	          "encoding: interpolation Linear or Smoothstep (got " + interp + ")");
	GridDesc g;
	grid_desc_init(g, n_dims, (uint32_t)j.number_or("n_levels", 16), (uint32_t)j.number_or("n_features_per_level", 2),
	               iequals(type, "Dense") ? GRID_LOG2_DENSE : (uint32_t)j.number_or("log2_hashmap_size", 19),
	               (uint32_t)j.number_or("base_resolution", 16), (float)j.number_or("per_level_scale", 2.0));
	g.interpolation = iequals(interp, "Smoothstep") ? GRID_SMOOTHSTEP : GRID_LINEAR;  // after grid_desc_init, which resets g
	return g;
}

static uint32_t parse_mlp_hidden(const Json& j, uint32_t* width) {
	const std::string ot = j.string_or("otype", "FullyFusedMLP");
	NGP_CHECK(iequals(ot, "FullyFusedMLP") || iequals(ot, "CutlassMLP") || iequals(ot, "MegakernelMLP"),
	          "network: only FullyFusedMLP-shaped networks are implemented (got " + ot + ")");
	NGP_CHECK(iequals(j.string_or("activation", "ReLU"), "ReLU"), "network: only ReLU hidden activation is implemented");
	NGP_CHECK(iequals(j.string_or("output_activation", "None"), "None"), "network: only output_activation None is implemented");
	*width = (uint32_t)j.number_or("n_neurons", 64);
	return (uint32_t)j.number_or("n_hidden_layers", 2);
}

}  // namespace ngp

void ngp_model::reserve(uint32_t n) {
	enc.get((size_t)n * enc_width * sizeof(f16));
	denc.get((size_t)n * enc_width * sizeof(f16));
	const uint32_t blocks = nerf ? nerf_mlp_train_blocks(n) : mlp_train_blocks(n);
	slabs.get((size_t)blocks * n_matrix() * sizeof(float));
	frags.get((size_t)n_all_frags * 1024);
	frags_inf.get((size_t)n_all_frags * 1024);
	if (use_sorted(n)) {
		sorted_workspace(n);
		ensure_side_stream();
	}
}
void ngp_model::ensure_side_stream() {
	if (side) return;
	NGP_HIP(hipStreamCreateWithFlags(&side, hipStreamNonBlocking));
	NGP_HIP(hipEventCreateWithFlags(&ev_fork, hipEventDisableTiming));
	NGP_HIP(hipEventCreateWithFlags(&ev_join, hipEventDisableTiming));
	NGP_HIP(hipEventCreateWithFlags(&ev_frags, hipEventDisableTiming));
	NGP_HIP(hipEventCreateWithFlags(&ev_mlp, hipEventDisableTiming));
	NGP_HIP(hipEventCreateWithFlags(&ev_red, hipEventDisableTiming));
}
const ScatterPlan& ngp_model::sc_plan_for(uint32_t n) {
	if (sc_plan_n != n) {
		sc_plan = make_scatter_plan(grid, n, scatter_opts(grid_bricks));
		sc_plan_n = n;
		fb_dirty = true;  // the brick fallback table may now lie over bytes the previous plan used (items)
	}
	return sc_plan;
}
void ngp_model::clear_brick_fallback(hipStream_t s, void* ws) {
	if (!fb_dirty) return;
	if (sc_plan.bk.LD) NGP_HIP(hipMemsetAsync((char*)ws + sc_plan.off_fb, 0, sc_plan.total - sc_plan.off_fb, s));
	fb_dirty = false;
}
void ngp_model::prepare_grid_backward_async(hipStream_t s, uint32_t n, const float* in, uint32_t stride) {
	if (!side_prepare(n)) return;
	ensure_side_stream();
	void* ws = sorted_workspace(n);
	clear_brick_fallback(s, ws);  // on s, before the fork: the side stream's plan kernel writes the flag after it
	GridBwdArgs b{n, in, stride, nullptr, 0, AoS, nullptr, max_level, max_level_per_sample};
	NGP_HIP(hipEventRecord(ev_fork, s));
	NGP_HIP(hipStreamWaitEvent(side, ev_fork, 0));
	// the training MLP's weight fragments depend only on the parameters: build them here, off the
	// critical path (run_mlp waits on ev_frags instead of launching k_prepare_frags itself)
	if ((overlap & 2) && !frags_current) {
		prep(side, false);
		NGP_HIP(hipEventRecord(ev_frags, side));
		frags_async = true;
	}
	{
		ProfScope ps("grid_bwd_prepare", side);
		grid_scatter_prepare(grid, b, sc_plan, ws, side);
	}
	NGP_HIP(hipEventRecord(ev_join, side));
	sc_prepared = true;
}

void ngp_model::finalize() {
	grid_params = grid.n_params();
	n_params = mlp0_params + mlp1_params + grid_params;
	const auto& d = descs();
	n_all_frags = (uint32_t)d.size();
	NGP_HIP(hipMalloc(&d_descs, d.size() * sizeof(FragDesc)));
	NGP_HIP(hipMemcpy(d_descs, d.data(), d.size() * sizeof(FragDesc), hipMemcpyHostToDevice));
	// inverse of k_prepare_frags: where each matrix parameter lives in the fragment buffer
	std::vector<uint32_t> map(2 * n_matrix(), ~0u);
	for (uint32_t f = 0; f < n_all_frags; ++f)
		for (uint32_t lane = 0; lane < 64; ++lane)
			for (uint32_t j = 0; j < 8; ++j) {
				const FragDesc& q = d[f];
				const uint32_t h = lane >> 5, r = 32 * q.tile + (lane & 31);
				const uint32_t k = q.perm ? 16 * q.step + 8 * (j >> 2) + 4 * h + (j & 3) : 16 * q.step + 8 * h + j;
				uint64_t pi;
				if (!q.transposed) {
					if (!(r < q.out_dim && k < q.in_dim)) continue;
					pi = q.woff + (uint64_t)r * q.in_dim + k;
				} else {
					if (!(r < q.in_dim && k < q.out_dim)) continue;
					pi = q.woff + (uint64_t)k * q.in_dim + r;
				}
				NGP_CHECK(pi < n_matrix() && map[2 * pi + q.transposed] == ~0u, "fragment map: parameter mapped twice");
				map[2 * pi + q.transposed] = (f * 64 + lane) * 8 + j;
			}
	NGP_HIP(hipMalloc(&d_fragmap, map.size() * sizeof(uint32_t)));
	NGP_HIP(hipMemcpy(d_fragmap, map.data(), map.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
}
f16x8* ngp_model::prep(hipStream_t s, bool inference) {
	f16x8* f = (f16x8*)(inference ? frags_inf : frags).get((size_t)n_all_frags * 1024);
	if (inference) sync_inference(s);
	ProfScope ps("prepare_frags", s);
	prepare_frags(d_descs, n_all_frags, pick(inference), f, s);
	if (!inference) frags_current = true;
	return f;
}
void ngp_model::encode(hipStream_t s, uint32_t n, const float* in, uint32_t stride, f16* out, uint32_t out_stride, uint32_t layout,
                       bool inference, bool want_hist) {
	if (inference) sync_inference(s);
	GridFwdArgs a{n, in, stride, pick(inference) + grid_offset(), out, out_stride, layout, max_level, max_level_per_sample};
	if (enc_width > grid.n_levels * grid.n_features && layout == AoS && !grid_forward_rows_ok(grid, a)) {
		// zero the padding columns (tcnn pads the encoding output with zeros); the row kernel writes them
		NGP_HIP(hipMemsetAsync(out, 0, (size_t)n * out_stride * sizeof(f16), s));
	}
	sc_hist_done = false;
	GridHist h;
	const bool fuse = want_hist && fused_hist && use_sorted(n) && !sc_prepared && grid_forward_rows_ok(grid, a) &&
	                  scatter_hist(grid, sc_plan_for(n), sorted_workspace(n), h);
	ProfScope ps("grid_forward", s);
	grid_forward(grid, a, s, fuse ? &h : nullptr);
	sc_hist_done = fuse;
}
void ngp_model::run_mlp(hipStream_t s, const MlpCall& c) {
	const MlpMode mode = c.mode;
	f16x8* f;
	if (frags_async && !c.inference) {
		f = (f16x8*)frags.p;
		NGP_HIP(hipStreamWaitEvent(s, ev_frags, 0));
		frags_async = false;
	} else if (!c.inference && frags_current && frags.p) {
		f = (f16x8*)frags.p;  // kept current by the optimizer (k_adam_ema writes the fragment slots)
	} else {
		f = prep(s, c.inference);
	}
	if (nerf) {
		NerfMlpArgs a{};
		a.n = c.n; a.enc = c.enc; a.enc_stride = enc_width; a.coords = c.coords; a.coord_stride = c.coord_stride; a.dir_offset = dir_offset;
		a.frags = f; a.n_frags = n_all_frags; a.out = c.out; a.out_stride = c.out_stride; a.out_layout = c.out_layout;
		a.dL_dout = c.dL_dout; a.dL_stride = c.dL_stride; a.dL_denc = c.dL_denc; a.denc_stride = enc_width; a.dw_slab = c.slab;
		a.n_matrix = (uint32_t)n_matrix(); a.density_woff = 0; a.rgb_woff = (uint32_t)mlp0_params;
		a.dL_dsh = c.dL_dsh;
		if (c.ex) { a.dL_ddens = c.ex->ddens; a.ddens_stride = c.ex->ddens_stride; }
		if (mode == MLP_INFER_ENC || mode == MLP_INFER_ENC_SMOOTH) {
			if (c.inference) sync_inference(s);
			a.table = pick(c.inference) + grid_offset(); a.max_level = max_level; a.gc = make_grid_const(grid);
		}
		ProfScope ps(mode == MLP_TRAIN ? "mlp_train" : mode == MLP_DENSITY ? "mlp_density"
		             : (mode == MLP_INFER_ENC || mode == MLP_INFER_ENC_SMOOTH) ? "mlp_infer_enc"
		             : mode == MLP_DENSITY_TRAIN ? "mlp_density_train" : "mlp_infer", s);
		nerf_mlp_run(nplan, mode, a, s);
	} else {
		MlpArgs a{};
		a.n = c.n; a.enc = c.enc; a.enc_stride = enc_width; a.frags = f; a.n_frags = n_all_frags;
		a.out = c.out; a.out_stride = c.out_stride; a.out_layout = c.out_layout; a.dL_dout = c.dL_dout; a.dL_stride = c.dL_stride;
		a.dL_denc = c.dL_denc; a.denc_stride = enc_width; a.dw_slab = c.slab; a.n_matrix = (uint32_t)n_matrix();
		ProfScope ps(mode == MLP_TRAIN ? "mlp_train" : "mlp_infer", s);
		mlp_run(mplan, mode == MLP_DENSITY ? MLP_INFER : mode, a, s);
	}
}
void ngp_model::train_pass(hipStream_t s, const MlpCall& b, int grad_mode, const BwdExtra& ex, const FusedAdam* fopt) {
	const uint32_t n = b.n, stride = b.coord_stride;
	const float* in = b.coords;
	NGP_CHECK(gradients || grad_mode == NGP_GRAD_IGNORE, "model has no gradient buffer: call ngp_model_set_params");
	NGP_CHECK(!ex.density_only || (nerf && b.enc), "density backward: a NerfNetwork with its encoding");
	f16* dL_denc = (f16*)denc.get((size_t)n * enc_width * sizeof(f16));
	const uint32_t blocks = nerf ? nerf_mlp_train_blocks(n) : mlp_train_blocks(n);
	float* slab = (float*)slabs.get((size_t)blocks * n_matrix() * sizeof(float));
	f16* dsh = ex.dL_dinput && nerf && !ex.density_only ? (f16*)dsh_ws.get((size_t)n * 16 * sizeof(f16)) : nullptr;
	NGP_CHECK(b.enc, "train_pass: the encoding buffer");
	MlpCall c = b;
	c.mode = ex.density_only ? MLP_DENSITY_TRAIN : MLP_TRAIN;
	c.out_layout = AoS; c.dL_denc = dL_denc; c.slab = slab; c.dL_dsh = dsh; c.inference = ex.inference; c.ex = &ex;
	run_mlp(s, c);
	// dL/dinput through the grid (position rows) and the SH encoding (direction rows, NerfNetwork). Where
	// dL_dinput aliases the input (the reference passes positions_matrix for both, testbed_nerf.cu:2616) it runs
	// last, because the grid backward still reads the input. Otherwise it runs before the grid backward: with the
	// optimizer update fused into that backward (fopt->rec) the table holds the next step's weights afterwards,
	// and the gradient is with respect to the forward's
	const bool dinput_aliases = (const float*)ex.dL_dinput == in;
	auto input_gradient = [&]() {
		if (!ex.dL_dinput) return;
		ProfScope ps("input_gradient", s);
		if (ex.inference) sync_inference(s);
		InputGradArgs ia{n, in, stride, pick(ex.inference) + grid_offset(), dL_denc, enc_width, max_level, max_level_per_sample, dsh,
		                 dir_offset, ex.dL_dinput, ex.dinput_stride, ex.dinput_scale};
		grid_input_gradient(grid, ia, s);
	};
	if (grad_mode == NGP_GRAD_IGNORE) {
		input_gradient();
		return;
	}
	grads_valid = !(fopt && (fopt->rec || fopt->g32));
	// the dW slab reduction (MLP section of the gradient) and the grid backward (grid section) are
	// independent: for large batches the reduction runs in extra blocks of the grid backward's last
	// kernel (fuse_slabs, default), or on the side stream under it (overlap bit 4). The density-only
	// backward reduces the density MLP's leading slice of each slab (the rgb gradients stay untouched).
	const bool ovl = use_sorted(n) && (overlap & 4);
	const bool fused = use_sorted(n) && !ovl && fuse_slabs && !ex.density_only;
	const uint32_t n_red = ex.density_only ? (uint32_t)mlp0_params : (uint32_t)n_matrix();
	SlabJob sj;
	sj.slabs = slab; sj.n_slabs = blocks; sj.n = n_red; sj.grad = gradients; sj.stride = (uint32_t)n_matrix();
	sj.accumulate = grad_mode == NGP_GRAD_ACCUMULATE;
	FusedAdam f32store;
	if (fopt && fopt->g32) {
		// the sharded optimizer's input: the whole gradient stored widened to fp32 by the backward itself
		NGP_CHECK(fused && grad_mode == NGP_GRAD_OVERWRITE && !fopt->rec, "fp32 gradient store: fused slab reduction");
		sj.grad32 = fopt->g32;
		f32store.g32 = fopt->g32 + grid_offset();
		fopt = &f32store;
	}
	hipStream_t rs = s;
	if (ovl) {
		ensure_side_stream();
		NGP_HIP(hipEventRecord(ev_mlp, s));
		NGP_HIP(hipStreamWaitEvent(side, ev_mlp, 0));
		rs = side;
	}
	if (!fused) {
		ProfScope ps("reduce_slabs", rs);
		reduce_slabs(slab, blocks, n_red, gradients, grad_mode == NGP_GRAD_ACCUMULATE, rs, (uint32_t)n_matrix());
	}
	if (ovl) NGP_HIP(hipEventRecord(ev_red, side));
	GridBwdArgs gb{n, in, stride, dL_denc, enc_width, AoS, gradients + grid_offset(), max_level, max_level_per_sample};
	FusedAdam fmlp;
	if (fopt && fopt->mlp_n) {
		// the MLP's update in the slab blocks (trainer: mlp_opt_in_backward): the fragment slots are written
		// in place when they hold the current parameters, as the optimizer launch would (run_step)
		NGP_CHECK(fused && grad_mode == NGP_GRAD_OVERWRITE && fopt->mlp_n == n_matrix(), "fused MLP update: slab reduction not fused");
		fmlp = *fopt;
		fmlp.frags = frags_current ? (f16*)frags.p : nullptr;
		fmlp.fragmap = d_fragmap;
		fopt = &fmlp;
	}
	if (!dinput_aliases) input_gradient();
	scatter_grid_grad(s, gb, grad_mode != NGP_GRAD_ACCUMULATE, fused ? &sj : nullptr, fopt);
	if (ovl) NGP_HIP(hipStreamWaitEvent(s, ev_red, 0));
	if (dinput_aliases) input_gradient();
}
void ngp_model::scatter_grid_grad(hipStream_t s, GridBwdArgs b, bool overwrite, const SlabJob* slab, const FusedAdam* fopt) {
	if (use_sorted(b.n)) {
		void* ws = sorted_workspace(b.n);
		clear_brick_fallback(s, ws);
		if (sc_prepared) {
			NGP_HIP(hipStreamWaitEvent(s, ev_join, 0));
			sc_prepared = false;
		} else {
			ProfScope ps("grid_bwd_prepare", s);
			grid_scatter_prepare(grid, b, sc_plan, ws, s, sc_hist_done);
		}
		sc_hist_done = false;
		// _adam: with the grid's optimizer update
		ProfScope ps(fopt && fopt->rec ? "grid_backward_adam" : "grid_backward_sorted", s);
		grid_backward_sorted(grid, b, sc_plan, ws, s, overwrite, win_debug, slab, fopt,
		                     bwd_parts && !sc_plan.bk.LD && !(fopt && fopt->rec) ? bwd_parts : nullptr);
		return;
	}
	NGP_CHECK(!slab && !fopt, "fused slab reduction / optimizer need the sorted grid backward");
	if (overwrite) {
		ProfScope ps("grid_grad_zero", s);
		NGP_HIP(hipMemsetAsync(b.grad, 0, grid_params * sizeof(f16), s));
	}
	ProfScope ps("grid_backward", s);
	grid_backward(grid, b, s);
}

// dL/doutput of tcnn's input_gradient: row `dim` of every sample = scale, every other row 0
__global__ static void k_one_hot_f16(f16* out, uint32_t n, uint32_t width, uint32_t dim, f16 v) {
	const uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
	if (i < (uint64_t)n * width) out[i] = (i % width) == dim ? v : (f16)0.f;
}
static void fill_one_hot_f16(f16* out, uint32_t n, uint32_t width, uint32_t dim, float v, hipStream_t s) {
	k_one_hot_f16<<<div_round_up((uint64_t)n * width, 256), 256, 0, s>>>(out, n, width, dim, (f16)v);
	NGP_HIP(hipGetLastError());
}

static thread_local std::string g_last_error;

namespace ngp {
void set_last_error(const char* msg) { g_last_error = msg; }
}  // namespace ngp

// NGP_MODEL_OPTS="key=value,key=value": engine options applied to every model at creation (A/B runs of whole
// programs, tools/ab.sh); an unknown key or a bad value fails the creation
static void apply_env_options(ngp_model* m) {
	const char* env = knob_model_opts();
	if (!env || !*env) return;
	std::string all = env;
	size_t pos = 0;
	while (pos < all.size()) {
		size_t end = all.find(',', pos);
		if (end == std::string::npos) end = all.size();
		const std::string kv = all.substr(pos, end - pos);
		pos = end + 1;
		if (kv.empty()) continue;
		const size_t eq = kv.find('=');
		NGP_CHECK(eq != std::string::npos, "NGP_MODEL_OPTS: expected key=value, got " + kv);
		if (ngp_model_set_option(m, kv.substr(0, eq).c_str(), atof(kv.c_str() + eq + 1)) != NGP_OK) throw Error(g_last_error);
	}
}

static int check_dinput(const ngp_model* m, float* dL_dinput, uint32_t stride) {
	if (!dL_dinput) return NGP_OK;
	const uint32_t need = m->nerf ? m->dir_offset + 3 : m->n_pos_dims;
	if (stride < need) {
		g_last_error = "dL_dinput: stride smaller than the rows the input gradient writes";
		return NGP_INVALID;
	}
	return NGP_OK;
}

// NerfNetwork::density (ngp_density's body): the density network's output rows in `output_layout` (AoS, SoA, or
// MLP_LAYOUT_ROW0 for the density grid update, which reads row 0 only).
int ngp::density_impl(ngp_model* m, void* stream, uint32_t n, const float* input, uint32_t input_stride, void* output,
                      uint32_t output_stride, uint32_t output_layout, int use_inference_params) {
	NGP_TRY({
		NGP_CHECK(m->nerf, "density() is a NerfNetwork method");
		if (n == 0) return NGP_OK;
		m->require_params(use_inference_params);
		f16* e = (f16*)m->enc.get((size_t)n * m->enc_width * sizeof(f16));
		m->encode(S(stream), n, input, input_stride, e, m->enc_width, AoS, use_inference_params);
		MlpCall c;
		c.mode = MLP_DENSITY; c.n = n; c.coords = input; c.coord_stride = input_stride; c.enc = e;
		c.out = (f16*)output; c.out_stride = output_stride; c.out_layout = output_layout; c.inference = use_inference_params;
		m->run_mlp(S(stream), c);
		m->generation++;
	});
}

// ngp_forward_backward, optionally with the grid's lazy optimizer update fused into the backward (fopt:
// captured training steps, ngp_trainer_fused_update)
int ngp::forward_backward_with(ngp_model* m, void* stream, uint32_t n, const float* input, uint32_t input_stride, void* output,
                               uint32_t output_stride, const void* dL_doutput, uint32_t dL_stride, int grad_mode,
                               const FusedAdam* fopt, float* dL_dinput, uint32_t dL_dinput_stride) {
	NGP_ARG(m && (n == 0 || (input && dL_doutput)));
	if (check_dinput(m, dL_dinput, dL_dinput_stride) != NGP_OK) return NGP_INVALID;
	NGP_TRY({
		if (n == 0) return NGP_OK;
		m->require_params(false);
		f16* e = (f16*)m->enc.get((size_t)n * m->enc_width * sizeof(f16));
		m->generation++;
		m->prepare_grid_backward_async(S(stream), n, input, input_stride);
		m->encode(S(stream), n, input, input_stride, e, m->enc_width, AoS, false, true);
		BwdExtra ex;
		ex.dL_dinput = dL_dinput; ex.dinput_stride = dL_dinput_stride;
		MlpCall b;
		b.n = n; b.coords = input; b.coord_stride = input_stride; b.enc = e; b.out = (f16*)output; b.out_stride = output_stride;
		b.dL_dout = (const f16*)dL_doutput; b.dL_stride = dL_stride;
		m->train_pass(S(stream), b, grad_mode, ex, fopt);
	});
}

// ------------------------------------------------------------------------------------------------
// C-ABI
// ------------------------------------------------------------------------------------------------
extern "C" {

const char* ngp_last_error(void) { return g_last_error.c_str(); }
const char* ngp_version(void) { return "ngp-mi355x 0.1 (gfx950)"; }

int ngp_device_info(int* cu_count, char* name, size_t name_len) {
	NGP_TRY({
		int dev = 0;
		NGP_HIP(hipGetDevice(&dev));
		hipDeviceProp_t p;
		NGP_HIP(hipGetDeviceProperties(&p, dev));
		if (cu_count) *cu_count = p.multiProcessorCount;
		if (name && name_len) { strncpy(name, p.gcnArchName, name_len - 1); name[name_len - 1] = 0; }
	});
}

int ngp_malloc(void** ptr, size_t bytes) { NGP_ARG(ptr); NGP_TRY(NGP_HIP(hipMalloc(ptr, bytes))); }
int ngp_free(void* ptr) { NGP_TRY(NGP_HIP(hipFree(ptr))); }
int ngp_memcpy(void* dst, const void* src, size_t bytes, int kind) { NGP_TRY(NGP_HIP(hipMemcpy(dst, src, bytes, (hipMemcpyKind)kind))); }
int ngp_stream_synchronize(void* stream) { NGP_TRY(NGP_HIP(hipStreamSynchronize(S(stream)))); }

int ngp_nerf_network_create(uint32_t n_pos_dims, uint32_t n_dir_dims, uint32_t n_extra_dims, uint32_t dir_offset,
                            const char* pos_encoding_json, const char* dir_encoding_json, const char* density_network_json,
                            const char* rgb_network_json, ngp_model** out) {
	NGP_ARG(out && pos_encoding_json && density_network_json && rgb_network_json);
	NGP_TRY({
		auto m = std::make_unique<ngp_model>();
		m->nerf = true;
		NGP_CHECK(n_pos_dims == 3, "NerfNetwork: n_pos_dims must be 3");
		NGP_CHECK(n_dir_dims == 3, "NerfNetwork: n_dir_dims must be 3");
		NGP_CHECK(n_extra_dims == 0, "NerfNetwork: extra dims (latent codes) are not implemented");
		m->n_pos_dims = n_pos_dims; m->n_dir_dims = n_dir_dims; m->n_extra_dims = n_extra_dims; m->dir_offset = dir_offset;
		m->grid = parse_grid(3, Json::parse(pos_encoding_json));
		if (dir_encoding_json) {
			Json d = Json::parse(dir_encoding_json);
			const Json* sh = &d;
			if (iequals(d.string_or("otype", ""), "Composite")) sh = &d["nested"].arr.at(0);
			NGP_CHECK(iequals(sh->string_or("otype", ""), "SphericalHarmonics") && (int)sh->number_or("degree", 4) == 4,
			          "NerfNetwork: dir_encoding must be SphericalHarmonics of degree 4");
		}
		uint32_t wd, wr;
		const uint32_t dh = parse_mlp_hidden(Json::parse(density_network_json), &wd);
		const uint32_t rh = parse_mlp_hidden(Json::parse(rgb_network_json), &wr);
		NGP_CHECK(wd == wr, "NerfNetwork: density and rgb networks must share n_neurons");
		m->enc_width = next_multiple(m->grid.n_levels * m->grid.n_features, 16);
		m->nplan = make_nerf_mlp_plan(m->enc_width, wd, dh, rh);
		m->mlp0_params = m->nplan.density.n_params();
		m->mlp1_params = m->nplan.rgb.n_params();
		m->n_input_dims = dir_offset + n_dir_dims + n_extra_dims;
		m->n_output_dims = 4;
		m->finalize();
		apply_env_options(m.get());
		*out = m.release();
	});
}

int ngp_network_with_input_encoding_create(uint32_t n_input_dims, uint32_t n_output_dims, const char* encoding_json,
                                           const char* network_json, ngp_model** out) {
	NGP_ARG(out && encoding_json && network_json);
	NGP_TRY({
		auto m = std::make_unique<ngp_model>();
		m->nerf = false;
		NGP_CHECK(n_input_dims == 2 || n_input_dims == 3, "NetworkWithInputEncoding: 2 or 3 input dims");
		NGP_CHECK(n_output_dims >= 1 && n_output_dims <= 16, "NetworkWithInputEncoding: 1..16 outputs");
		m->n_pos_dims = n_input_dims; m->n_input_dims = n_input_dims; m->n_output_dims = n_output_dims;
		m->grid = parse_grid(n_input_dims, Json::parse(encoding_json));
		uint32_t w;
		const uint32_t hid = parse_mlp_hidden(Json::parse(network_json), &w);
		m->enc_width = next_multiple(m->grid.n_levels * m->grid.n_features, 16);
		m->mplan = make_mlp_plan(m->enc_width, w, hid, 16);
		m->mlp0_params = m->mplan.mlp.n_params();
		m->mlp1_params = 0;
		m->finalize();
		apply_env_options(m.get());
		*out = m.release();
	});
}

void ngp_model_destroy(ngp_model* m) { delete m; }
uint64_t ngp_model_n_params(const ngp_model* m) { return m ? m->n_params : 0; }
uint64_t ngp_model_n_matrix_params(const ngp_model* m) { return m ? m->n_matrix() : 0; }
uint32_t ngp_model_input_width(const ngp_model* m) { return m ? m->n_input_dims : 0; }
uint32_t ngp_model_padded_output_width(const ngp_model* m) { return m ? 16 : 0; }
uint32_t ngp_model_output_width(const ngp_model* m) { return m ? m->n_output_dims : 0; }

int ngp_model_param_layout(const ngp_model* m, ngp_param_layout* o) {
	NGP_ARG(m && o);
	NGP_TRY({
		memset(o, 0, sizeof(*o));
		o->density_mlp_offset = 0; o->density_mlp_params = m->mlp0_params;
		o->rgb_mlp_offset = m->mlp0_params; o->rgb_mlp_params = m->mlp1_params;
		o->grid_offset = m->grid_offset(); o->grid_params = m->grid_params;
		o->grid_dims = m->grid.n_dims; o->grid_levels = m->grid.n_levels; o->grid_features = m->grid.n_features;
		o->grid_log2_hashmap = m->grid.log2_hashmap; o->grid_base_resolution = m->grid.base_resolution;
		o->grid_per_level_scale = m->grid.per_level_scale;
		memcpy(o->grid_level_offsets, m->grid.offsets, sizeof(o->grid_level_offsets));
		memcpy(o->grid_resolution, m->grid.resolution, sizeof(o->grid_resolution));
		memcpy(o->grid_scale, m->grid.scale, sizeof(o->grid_scale));
		o->encoding_width = m->enc_width;
	});
}

int ngp_model_set_params(ngp_model* m, void* params, void* inference_params, void* gradients) {
	NGP_ARG(m);
	NGP_TRY({
		m->inference_hook = nullptr;  // a trainer that binds its own buffers installs its hook afterwards
		m->inference_hook_ctx = nullptr;
		m->params = (f16*)params;
		m->frags_current = false;
		m->inference_params = (f16*)(inference_params ? inference_params : params);
		m->gradients = (f16*)gradients;
	});
}

int ngp_model_initialize_params(const ngp_model* m, uint64_t seed, float* p, float scale) {
	NGP_ARG(m && p);
	NGP_TRY({
		Pcg32 rng(seed);
		if (m->nerf) {
			init_mlp(m->nplan.density, rng, p, scale);
			init_mlp(m->nplan.rgb, rng, p + m->mlp0_params, scale);
		} else {
			init_mlp(m->mplan.mlp, rng, p, scale);
		}
		rng.uniform(m->grid_params, p + m->grid_offset(), -1e-4f * scale, 1e-4f * scale);
	});
}

int ngp_model_set_max_level(ngp_model* m, float max_level, const float* per_sample) {
	NGP_ARG(m);
	NGP_TRY({ m->max_level = max_level; m->max_level_per_sample = per_sample; });
}

int ngp_model_set_option(ngp_model* m, const char* key, double value) {
	NGP_ARG(m && key);
	NGP_TRY({
		const std::string k = key;
		if (k == "grid_backward_mode") {
			NGP_CHECK(value == 0 || value == 1 || value == 3, "grid_backward_mode must be 0 (auto), 1 (direct), 3 (bucketed)");
			m->grid_backward_mode = (int)value;
		} else if (k == "overlap") {
			NGP_CHECK(value >= 0 && value <= 15, "overlap is a bitmask in [0, 15]");
			m->overlap = (uint32_t)value;
		} else if (k == "fused_hist") {
			m->fused_hist = value != 0;
		} else if (k == "fuse_infer") {
			m->fuse_infer = value != 0;
		} else if (k == "fuse_slabs") {
			m->fuse_slabs = value != 0;
		} else if (k == "fuse_opt") {
			m->fuse_opt = value != 0;
		} else if (k == "fuse_mlp_opt") {
			m->fuse_mlp_opt = value != 0;
		} else if (k == "grid_bricks") {
			m->grid_bricks = value != 0;
			m->sc_plan_n = 0;  // re-plan at the next batch
		} else if (k == "grid_direct") {
			m->grid_direct = value != 0;
			m->sc_plan_n = 0;
		} else if (k == "grid_plan_inline") {
			m->grid_plan_inline = value != 0;
			m->sc_plan_n = 0;
		} else if (k == "win_debug") {
			m->win_debug = (uint32_t)value;
		} else {
			throw Error("unknown model option: " + k);
		}
		// a graph captured before the change launches the old kernels: mark it stale (the NeRF trainer re-captures,
		// ngp_graph_launch of a caller's graph fails loudly)
		++m->ws_epoch;
	});
}

int ngp_model_query(const ngp_model* m, const char* key, double* value) {
	NGP_ARG(m && key && value);
	NGP_TRY({
		const std::string k = key;
		if (k == "grid_brick_levels") *value = m->sc_plan_n ? (double)(m->sc_plan.bk.LD - m->sc_plan.bk.LB) : 0.0;
		else if (k == "grid_direct_levels") *value = m->sc_plan_n ? (double)m->sc_plan.direct_levels : 0.0;
		else if (k == "grid_direct_part") *value = (double)make_scatter_plan(m->grid, 4096, m->scatter_opts(false)).direct_part;
		else if (k == "grid_plan_inline") *value = m->sc_plan_n && m->sc_plan.plan_inline ? 1.0 : 0.0;
		else if (k == "grid_interpolation") *value = (double)m->grid.interpolation;  // GridInterp: 0 Linear, 1 Smoothstep
		else if (k == "fused_inference") *value = m->fused_inference_ok() ? 1.0 : 0.0;  // ngp_inference encodes in the MLP kernel
		else throw Error("unknown model query: " + k);
	});
}

int ngp_model_reserve(ngp_model* m, uint32_t n) {
	NGP_ARG(m);
	NGP_TRY({ m->reserve(n); });
}

uint64_t ngp_model_workspace_epoch(const ngp_model* m) { return m ? m->ws_epoch : 0; }

int ngp_model_workspace(ngp_model* m, const char* name, void** ptr, uint64_t* bytes) {
	NGP_ARG(m && name && ptr);
	NGP_TRY({
		const std::string k(name);
		DevBuf* b = k == "encoding" ? &m->enc : k == "dL_dencoding" ? &m->denc : k == "dw_slabs" ? &m->slabs
		          : k == "dL_dsh" ? &m->dsh_ws : nullptr;
		NGP_CHECK(b, "ngp_model_workspace: unknown workspace '" + k + "' (encoding, dL_dencoding, dL_dsh, dw_slabs)");
		*ptr = b->p;
		if (bytes) *bytes = b->bytes;
	});
}

int ngp_encoding_forward(ngp_model* m, void* stream, uint32_t n, const float* input, uint32_t input_stride, void* output,
                         uint32_t output_stride, uint32_t output_layout, int use_inference_params) {
	NGP_ARG(m && (n == 0 || (input && output)) && output_layout <= 1);
	NGP_TRY({
		m->require_params(use_inference_params);
		m->encode(S(stream), n, input, input_stride, (f16*)output, output_stride, output_layout, use_inference_params);
	});
}

int ngp_encoding_backward(ngp_model* m, void* stream, uint32_t n, const float* input, uint32_t input_stride,
                          const void* dL_doutput, uint32_t dL_stride, uint32_t dL_layout, float* dL_dinput,
                          uint32_t dL_dinput_stride, int grad_mode) {
	NGP_ARG(m && (n == 0 || (input && dL_doutput)) && dL_layout <= 1 && grad_mode >= 0 && grad_mode <= NGP_GRAD_IGNORE);
	NGP_ARG(!dL_dinput || (dL_layout == NGP_LAYOUT_AOS && dL_dinput_stride >= m->grid.n_dims));
	NGP_TRY({
		if (n == 0) return NGP_OK;
		m->require_params(false);
		if (grad_mode != NGP_GRAD_IGNORE) {
			NGP_CHECK(m->gradients, "model has no gradient buffer");
			GridBwdArgs b{n, input, input_stride, (const f16*)dL_doutput, dL_stride, dL_layout, m->gradients + m->grid_offset(),
			              m->max_level, m->max_level_per_sample};
			m->scatter_grid_grad(S(stream), b, grad_mode != NGP_GRAD_ACCUMULATE);
		}
		// last: dL_dinput may alias the input, which the parameter backward above still reads
		if (dL_dinput) {
			ProfScope ps("input_gradient", S(stream));
			InputGradArgs ia{n, input, input_stride, m->params + m->grid_offset(), (const f16*)dL_doutput, dL_stride, m->max_level,
			                 m->max_level_per_sample, nullptr, 0, dL_dinput, dL_dinput_stride, 1.f};
			grid_input_gradient(m->grid, ia, S(stream));
		}
	});
}

int ngp_inference(ngp_model* m, void* stream, uint32_t n, const float* input, uint32_t input_stride, void* output,
                  uint32_t output_stride, uint32_t output_layout, int use_inference_params) {
	NGP_ARG(m && (n == 0 || (input && output)) && (output_layout <= 1 || (output_layout == NGP_LAYOUT_AOS_RGBD && m->nerf &&
	                                                                        output_stride >= 4)));
	NGP_TRY({
		if (n == 0) return NGP_OK;
		m->require_params(use_inference_params);
		MlpCall c;
		c.n = n; c.coords = input; c.coord_stride = input_stride;
		c.out = (f16*)output; c.out_stride = output_stride; c.out_layout = output_layout; c.inference = use_inference_params;
		if (m->fused_inference_ok()) {
			// the encoding never reaches HBM: the MLP kernel gathers and blends the grid levels itself
			c.mode = m->grid.interpolation == GRID_SMOOTHSTEP ? MLP_INFER_ENC_SMOOTH : MLP_INFER_ENC;
		} else {
			f16* e = (f16*)m->enc.get((size_t)n * m->enc_width * sizeof(f16));
			m->encode(S(stream), n, input, input_stride, e, m->enc_width, AoS, use_inference_params);
			c.mode = MLP_INFER; c.enc = e;
		}
		m->run_mlp(S(stream), c);
		m->generation++;
	});
}

int ngp_density(ngp_model* m, void* stream, uint32_t n, const float* input, uint32_t input_stride, void* output,
                uint32_t output_stride, uint32_t output_layout, int use_inference_params) {
	NGP_ARG(m && (n == 0 || (input && output)) && output_layout <= 1);
	return ngp::density_impl(m, stream, n, input, input_stride, output, output_stride, output_layout, use_inference_params);
}

int ngp_forward(ngp_model* m, void* stream, uint32_t n, const float* input, uint32_t input_stride, void* output,
                uint32_t output_stride, int use_inference_params, ngp_ctx** ctx) {
	NGP_ARG(m && ctx && (n == 0 || input));
	NGP_TRY({
		m->require_params(use_inference_params);
		f16* e = (f16*)m->enc.get((size_t)(n ? n : 1) * m->enc_width * sizeof(f16));
		m->generation++;
		if (n) {
			m->encode(S(stream), n, input, input_stride, e, m->enc_width, AoS, use_inference_params);
			if (output) {
				MlpCall c;
				c.mode = MLP_INFER; c.n = n; c.coords = input; c.coord_stride = input_stride; c.enc = e;
				c.out = (f16*)output; c.out_stride = output_stride; c.inference = use_inference_params;
				m->run_mlp(S(stream), c);
			}
		}
		*ctx = new ngp_ctx{n, input, input_stride, (bool)use_inference_params, m->generation};
	});
}

int ngp_backward(ngp_model* m, void* stream, ngp_ctx* ctx, const void* dL_doutput, uint32_t dL_stride, float* dL_dinput,
                 uint32_t dL_dinput_stride, int grad_mode) {
	NGP_ARG(m && ctx && (ctx->n == 0 || dL_doutput) && grad_mode >= 0 && grad_mode <= NGP_GRAD_IGNORE);
	if (check_dinput(m, dL_dinput, dL_dinput_stride) != NGP_OK) return NGP_INVALID;
	NGP_TRY({
		NGP_CHECK(ctx->generation == m->generation,
		          "backward: the forward context is stale (another forward/inference ran on this model since)");
		NGP_CHECK(!ctx->density_only, "backward: this context is from density_forward (use density_backward)");
		if (ctx->n == 0) return NGP_OK;
		BwdExtra ex;
		ex.dL_dinput = dL_dinput; ex.dinput_stride = dL_dinput_stride;
		ex.inference = ctx->use_inference_params;  // backward_impl passes use_inference_params to every sub-backward
		MlpCall b;
		b.n = ctx->n; b.coords = ctx->input; b.coord_stride = ctx->input_stride; b.enc = (const f16*)m->enc.p;
		b.dL_dout = (const f16*)dL_doutput; b.dL_stride = dL_stride;
		m->train_pass(S(stream), b, grad_mode, ex);
	});
}

int ngp_density_forward(ngp_model* m, void* stream, uint32_t n, const float* input, uint32_t input_stride, void* output,
                        uint32_t output_stride, int use_inference_params, ngp_ctx** ctx) {
	NGP_ARG(m && ctx && (n == 0 || input) && (!output || output_stride >= 16));
	NGP_TRY({
		NGP_CHECK(m->nerf, "density_forward is a NerfNetwork method");
		m->require_params(use_inference_params);
		f16* e = (f16*)m->enc.get((size_t)(n ? n : 1) * m->enc_width * sizeof(f16));
		m->generation++;
		if (n) {
			m->encode(S(stream), n, input, input_stride, e, m->enc_width, AoS, use_inference_params);
			if (output) {
				MlpCall c;
				c.mode = MLP_DENSITY; c.n = n; c.coords = input; c.coord_stride = input_stride; c.enc = e;
				c.out = (f16*)output; c.out_stride = output_stride; c.inference = use_inference_params;
				m->run_mlp(S(stream), c);
			}
		}
		*ctx = new ngp_ctx{n, input, input_stride, (bool)use_inference_params, m->generation, true};
	});
}

int ngp_density_backward(ngp_model* m, void* stream, ngp_ctx* ctx, const void* dL_doutput, uint32_t dL_stride, float* dL_dinput,
                         uint32_t dL_dinput_stride, int grad_mode) {
	NGP_ARG(m && ctx && (ctx->n == 0 || dL_doutput) && dL_stride >= 16 && dL_stride % 4 == 0 && grad_mode >= 0 &&
	        grad_mode <= NGP_GRAD_IGNORE && (!dL_dinput || dL_dinput_stride >= 3));
	NGP_TRY({
		NGP_CHECK(m->nerf, "density_backward is a NerfNetwork method");
		NGP_CHECK(ctx->generation == m->generation,
		          "density_backward: the forward context is stale (another forward/inference ran on this model since)");
		NGP_CHECK(ctx->density_only, "density_backward: this context is from forward (use backward)");
		if (ctx->n == 0) return NGP_OK;
		BwdExtra ex;
		ex.dL_dinput = dL_dinput; ex.dinput_stride = dL_dinput_stride;
		ex.density_only = true; ex.ddens = (const f16*)dL_doutput; ex.ddens_stride = dL_stride;
		ex.inference = ctx->use_inference_params;
		MlpCall b;
		b.n = ctx->n; b.coords = ctx->input; b.coord_stride = ctx->input_stride; b.enc = (const f16*)m->enc.p;
		m->train_pass(S(stream), b, grad_mode, ex);
	});
}

int ngp_input_gradient(ngp_model* m, void* stream, uint32_t dim, uint32_t n, const float* input, uint32_t input_stride,
                       float* d_dinput, uint32_t d_dinput_stride, float backprop_scale) {
	NGP_ARG(m && (n == 0 || (input && d_dinput)) && dim < 16 && backprop_scale != 0.f);
	if (check_dinput(m, d_dinput, d_dinput_stride) != NGP_OK) return NGP_INVALID;
	NGP_TRY({
		if (n == 0) return NGP_OK;
		m->require_params(false);
		hipStream_t s = S(stream);
		f16* e = (f16*)m->enc.get((size_t)n * m->enc_width * sizeof(f16));
		f16* dl = (f16*)m->dl1_ws.get((size_t)n * 16 * sizeof(f16));
		m->generation++;
		m->encode(s, n, input, input_stride, e, m->enc_width, AoS, false);
		// one-hot dL/doutput: row `dim` = backprop_scale (fp16), every other row 0
		fill_one_hot_f16(dl, n, 16, dim, backprop_scale, s);
		BwdExtra ex;
		ex.dL_dinput = d_dinput; ex.dinput_stride = d_dinput_stride; ex.dinput_scale = 1.f / backprop_scale;
		MlpCall b;
		b.n = n; b.coords = input; b.coord_stride = input_stride; b.enc = e; b.dL_dout = dl; b.dL_stride = 16;
		m->train_pass(s, b, NGP_GRAD_IGNORE, ex);
	});
}

void ngp_ctx_destroy(ngp_ctx* ctx) { delete ctx; }

int ngp_forward_backward(ngp_model* m, void* stream, uint32_t n, const float* input, uint32_t input_stride, void* output,
                         uint32_t output_stride, const void* dL_doutput, uint32_t dL_stride, int grad_mode) {
	return ngp::forward_backward_with(m, stream, n, input, input_stride, output, output_stride, dL_doutput, dL_stride, grad_mode,
	                                  nullptr);
}

}  // extern "C"
