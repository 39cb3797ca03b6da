// nerf_snapshot.hip — snapshots (.ingp): msgpack, zlib and file I/O; no kernel. A NeRF trainer's
// (ngp_nerf_save_snapshot / ngp_nerf_load_snapshot) and the generic ones of the image and SDF testbeds.
//
// Testbed::save_snapshot / load_snapshot (src/testbed.cu:4873-5057) for a NeRF testbed: msgpack of the
// network config with a "snapshot" member; .ingp files are gzip streams (zstr), others raw msgpack.
// tcnn Trainer::serialize writes n_params / params_type / params_binary (fp16 params); the optimizer
// member (include_optimizer_state) is this engine's own layout (tcnn absent: parity unpinned).
#include <fstream>
#include <sstream>

#include <zlib.h>

#include "json.h"
#include "msgpack.h"
#include "nerf_host.h"

namespace {
using ngp::mp::Value;

constexpr uint32_t SNAPSHOT_FORMAT_VERSION = 1;  // testbed.cu:80

bool ends_with_ci(const std::string& s, const std::string& suf) {
	return s.size() >= suf.size() && ngp::iequals(s.substr(s.size() - suf.size()), suf);
}

std::string gzip_bytes(const std::string& in, int level) {
	z_stream z{};
	NGP_CHECK(deflateInit2(&z, level, Z_DEFLATED, 15 + 16, 8, Z_DEFAULT_STRATEGY) == Z_OK, "snapshot: deflateInit2 failed");
	std::string out(deflateBound(&z, in.size()) + 64, '\0');
	z.next_in = (Bytef*)in.data();
	z.avail_in = (uInt)in.size();
	z.next_out = (Bytef*)out.data();
	z.avail_out = (uInt)out.size();
	const int rc = deflate(&z, Z_FINISH);
	const size_t n = out.size() - z.avail_out;
	deflateEnd(&z);
	NGP_CHECK(rc == Z_STREAM_END, "snapshot: deflate failed");
	out.resize(n);
	return out;
}

std::string maybe_inflate(const std::string& in) {
	const bool gz = in.size() >= 2 && (uint8_t)in[0] == 0x1f && (uint8_t)in[1] == 0x8b;
	const bool zl = in.size() >= 2 && ((uint8_t)in[0] & 0x0f) == 8 && (((uint8_t)in[0] << 8) | (uint8_t)in[1]) % 31 == 0;
	if (!gz && !zl) return in;  // raw msgpack
	z_stream z{};
	NGP_CHECK(inflateInit2(&z, 15 + 32) == Z_OK, "snapshot: inflateInit2 failed");
	z.next_in = (Bytef*)in.data();
	z.avail_in = (uInt)in.size();
	std::string out;
	char buf[1 << 16];
	int rc;
	do {
		z.next_out = (Bytef*)buf;
		z.avail_out = sizeof buf;
		rc = inflate(&z, Z_NO_FLUSH);
		NGP_CHECK(rc == Z_OK || rc == Z_STREAM_END, "snapshot: corrupt compressed stream");
		out.append(buf, sizeof buf - z.avail_out);
	} while (rc != Z_STREAM_END);
	inflateEnd(&z);
	return out;
}

std::string read_file(const char* path) {
	std::ifstream f(path, std::ios::binary);
	NGP_CHECK(f.good(), std::string("snapshot: cannot open '") + path + "'");
	std::stringstream ss;
	ss << f.rdbuf();
	return ss.str();
}

Value load_network_config(const char* path) {  // Testbed::load_network_config (testbed.cu:246): msgpack branch
	return ngp::mp::decode(maybe_inflate(read_file(path)));
}

Value vec3(const float* v) {
	Value a = Value::array();
	for (int k = 0; k < 3; ++k) a.arr.push_back(Value::real(v[k]));
	return a;
}

// one per-camera optimiser with the reference's member names (adam_optimizer.h:174-194)
Value adam_to_value(const ngp_adam_state& a) {
	Value v = Value::object();
	v["iter"] = Value::uint(a.iter);
	v["first_moment"] = vec3(a.first_moment);
	v["second_moment"] = vec3(a.second_moment);
	v["variable"] = vec3(a.variable);
	v["learning_rate"] = Value::real(a.learning_rate);
	v["epsilon"] = Value::real(a.epsilon);
	v["beta1"] = Value::real(a.beta1);
	v["beta2"] = Value::real(a.beta2);
	return v;
}
ngp_adam_state adam_from_value(const Value& v) {
	ngp_adam_state a;
	a.iter = (uint32_t)v.at("iter").number();
	const char* names[3] = {"first_moment", "second_moment", "variable"};
	float* dst[3] = {a.first_moment, a.second_moment, a.variable};
	for (int m = 0; m < 3; ++m) {
		const Value& x = v.at(names[m]);
		NGP_CHECK(x.type == Value::Array && x.arr.size() == 3, "snapshot: a camera optimiser's vectors hold three numbers");
		for (int k = 0; k < 3; ++k) dst[m][k] = (float)x.arr[k].number();
	}
	a.learning_rate = (float)v.at("learning_rate").number();
	a.epsilon = (float)v.at("epsilon").number();
	a.beta1 = (float)v.at("beta1").number();
	a.beta2 = (float)v.at("beta2").number();
	return a;
}

template <typename T> std::vector<T> device_to_host(const void* d, size_t n) {
	std::vector<T> h(n);
	if (n) NGP_HIP(hipMemcpy(h.data(), d, n * sizeof(T), hipMemcpyDeviceToHost));
	return h;
}

const char* const OPT_NAMES[5] = {"full_precision_params_binary", "first_moments_binary", "second_moments_binary",
                                  "ema_params_binary", "param_steps_binary"};

// tcnn Trainer::serialize(include_optimizer_state) (testbed.cu:4874): n_params, params_type, params_binary (the fp16
// parameters) and, with the optimizer state, an "optimizer" member: the Adam moments and per-parameter steps, the
// EMA weights and the fp32 master weights under tcnn-style names (tcnn absent: the member names are a restatement,
// parity unpinned)
void trainer_to_snapshot(ngp_trainer* tr, uint64_t n, bool include_optimizer_state, Value& snap) {
	snap["n_params"] = Value::uint(n);
	snap["params_type"] = Value::str("__half");
	{
		auto p = device_to_host<uint16_t>(ngp_trainer_params(tr), n);
		snap["params_binary"] = Value::bin(p.data(), p.size() * 2);
	}
	if (!include_optimizer_state) return;
	uint64_t bytes = 0;
	check_rc(ngp_trainer_serialize(tr, nullptr, &bytes));
	std::string blob(bytes, '\0');
	check_rc(ngp_trainer_serialize(tr, blob.data(), &bytes));
	uint64_t hdr[4];
	memcpy(hdr, blob.data(), 32);
	Value opt = Value::object();
	opt["otype"] = Value::str("Ema(ExponentialDecay(Adam))");
	opt["current_step"] = Value::uint(hdr[3]);
	for (int k = 0; k < 5; ++k) opt[OPT_NAMES[k]] = Value::bin(blob.data() + 32 + (size_t)k * n * 4, (size_t)n * 4);
	snap["optimizer"] = opt;
}

// tcnn Trainer::deserialize (testbed.cu:5040): the parameters, then the optimizer state when the snapshot has one.
// An optimizer member without some of this engine's arrays (one written by another implementation of the chain)
// fills them from what is there: fp32 master weights and EMA from the parameters, moments and steps from 0.
void trainer_from_snapshot(ngp_trainer* tr, uint64_t n, const Value& snap) {
	NGP_CHECK((uint64_t)snap.at("n_params").number() == n, "snapshot: parameter count differs from this network");
	const Value& pb = snap.at("params_binary");
	const std::string type = snap.find("params_type") ? snap.at("params_type").s : std::string("__half");
	std::vector<float> w(n);
	if (type == "float") {
		NGP_CHECK(pb.s.size() == n * 4, "snapshot: params_binary size");
		memcpy(w.data(), pb.s.data(), n * 4);
	} else {
		NGP_CHECK(type == "__half" && pb.s.size() == n * 2, "snapshot: params_binary size/type");
		const ngp::f16* h = (const ngp::f16*)pb.s.data();
		for (uint64_t k = 0; k < n; ++k) w[k] = (float)h[k];
	}
	check_rc(ngp_trainer_set_params_full_precision(tr, w.data(), n));
	const Value* opt = snap.find("optimizer");
	if (!opt) return;
	std::string blob(32 + (size_t)n * 20, '\0');
	const uint64_t hdr[4] = {0x4e47504d49333535ULL, 1, n, (uint64_t)opt->number_or("current_step", 0.0)};
	memcpy(blob.data(), hdr, 32);
	for (int k = 0; k < 5; ++k) {
		char* dst = blob.data() + 32 + (size_t)k * n * 4;
		if (const Value* b = opt->find(OPT_NAMES[k])) {
			NGP_CHECK(b->s.size() == n * 4, std::string("snapshot: optimizer ") + OPT_NAMES[k] + " size");
			memcpy(dst, b->s.data(), n * 4);
		} else if (k == 0 || k == 3) {
			memcpy(dst, w.data(), n * 4);  // master weights / EMA: the parameters
		}  // moments, steps: 0
	}
	check_rc(ngp_trainer_deserialize(tr, blob.data(), blob.size()));
}

void write_snapshot(const char* path, Value& root, Value& snap, int compress) {
	root["snapshot"] = snap;
	std::string bytes;
	ngp::mp::encode(root, bytes);
	if (ends_with_ci(path, ".ingp")) bytes = gzip_bytes(bytes, compress ? Z_DEFAULT_COMPRESSION : Z_NO_COMPRESSION);
	std::ofstream f(path, std::ios::binary);
	NGP_CHECK(f.good(), std::string("snapshot: cannot write '") + path + "'");
	f.write(bytes.data(), (std::streamsize)bytes.size());
	NGP_CHECK(f.good(), "snapshot: write failed");
}

Value snapshot_root(const char* network_config_json) {
	Value root = network_config_json && *network_config_json ? ngp::mp::from_json(ngp::Json::parse(network_config_json))
	                                                          : Value::object();
	root.erase("snapshot");
	return root;
}
}  // namespace

extern "C" {

int ngp_nerf_save_snapshot(ngp_nerf_trainer* t, void* stream, const char* path, const char* network_config_json,
                           int include_optimizer_state, int compress) {
	if (!t || !path) return NGP_INVALID;
	NGP_TRY({
		NGP_HIP(hipStreamSynchronize(S(stream)));
		Value root = snapshot_root(network_config_json);
		Value snap = Value::object();
		trainer_to_snapshot(t->trainer, ngp_model_n_params(t->model), include_optimizer_state != 0, snap);
		snap["version"] = Value::uint(SNAPSHOT_FORMAT_VERSION);
		snap["mode"] = Value::str("nerf");
		snap["density_grid_size"] = Value::uint(GRIDSIZE);
		{
			const uint32_t n_el = GRID_N_CELLS * (t->cfg.max_cascade + 1);
			auto g = device_to_host<float>(t->grid.p, n_el);
			std::vector<f16> h(n_el);
			for (uint32_t k = 0; k < n_el; ++k) h[k] = (f16)g[k];  // (__half)density_grid[i]
			snap["density_grid_binary"] = Value::bin(h.data(), h.size() * 2);
		}
		Value& nerf = snap["nerf"];
		nerf["aabb_scale"] = Value::real(t->cfg.aabb_max[0] - t->cfg.aabb_min[0]);
		nerf["rgb"]["rays_per_batch"] = Value::uint(t->rays_per_batch);
		nerf["rgb"]["measured_batch_size"] = Value::uint(t->measured_batch_size);
		nerf["rgb"]["measured_batch_size_before_compaction"] = Value::uint(t->measured_before_compaction);
		// the per-camera optimisers, as VarAdamOptimizer::to_json writes them (testbed.cu:4891-4892)
		{
			Value pos = Value::array(), rot = Value::array();
			for (uint32_t i = 0; i < t->cams.size(); ++i) {
				ngp_adam_state p, r;
				check_rc(ngp_pose_optimizer_get(t->pose, i, &p, &r));
				pos.arr.push_back(adam_to_value(p));
				rot.arr.push_back(adam_to_value(r));
			}
			nerf["cam_pos_offset"] = pos;
			nerf["cam_rot_offset"] = rot;
		}
		// engine extension (the reference does not save cam_exposure): the per-image exposure optimisers in the same
		// form, once one of them has left its initial state; a trainer that never used them writes the bytes it wrote
		// before they existed
		{
			Value ex = Value::array();
			bool used = false;
			for (uint32_t i = 0; i < t->cams.size(); ++i) {
				ngp_adam_state e;
				check_rc(ngp_nerf_trainer_exposure_optimizer_state(t, i, &e));
				used = used || e.iter != 0;
				for (int k = 0; k < 3; ++k) used = used || e.variable[k] != 0.f || e.first_moment[k] != 0.f || e.second_moment[k] != 0.f;
				ex.arr.push_back(adam_to_value(e));
			}
			if (used) nerf["cam_exposure"] = ex;
		}
		snap["training_step"] = Value::uint(t->training_step);
		snap["loss"] = Value::real(t->loss_scalar);
		snap["aabb"]["min"] = vec3(t->cfg.aabb_min);
		snap["aabb"]["max"] = vec3(t->cfg.aabb_max);
		snap["density_grid_ema_step"] = Value::uint(t->ema_step);
		// engine extension (the reference does not save m_envmap): the environment map and its optimizer
		if (t->env.bound()) {
			NGP_HIP(hipDeviceSynchronize());
			const ngp_nerf_trainer::Envmap& e = t->env;
			const size_t n = e.n();
			auto put = [&](Value& to, const char* name, const void* d) {
				auto h = device_to_host<float>(d, n);
				to[name] = Value::bin(h.data(), n * 4);
			};
			Value em = Value::object();
			em["width"] = Value::uint(e.w);
			em["height"] = Value::uint(e.h);
			put(em, "params_binary", e.params.p);
			put(em, "ema_params_binary", t->envmap_inference());
			if (include_optimizer_state) {
				Value opt = Value::object();
				opt["current_step"] = Value::uint(e.step);
				opt["ema_valid"] = Value::uint(e.ema_valid ? 1 : 0);
				put(opt, "ema_binary", e.ema.p);
				put(opt, "first_moments_binary", e.m1.p);
				put(opt, "second_moments_binary", e.m2.p);
				put(opt, "param_steps_binary", e.steps.p);
				em["optimizer"] = opt;
			}
			snap["envmap"] = em;
		}
		// engine extension (the reference does not save m_distortion): the lens distortion map and its optimizer
		if (t->dist.bound()) {
			NGP_HIP(hipDeviceSynchronize());
			const ngp_nerf_trainer::Distortion& d = t->dist;
			const size_t n = d.n();
			auto put = [&](Value& to, const char* name, const void* p) {
				auto h = device_to_host<float>(p, n);
				to[name] = Value::bin(h.data(), n * 4);
			};
			Value dm = Value::object();
			dm["width"] = Value::uint(d.w);
			dm["height"] = Value::uint(d.h);
			put(dm, "params_binary", d.params.p);
			if (include_optimizer_state) {
				Value opt = Value::object();
				opt["current_step"] = Value::uint(d.step);
				opt["ema_valid"] = Value::uint(d.ema_valid ? 1 : 0);
				put(opt, "ema_binary", d.ema.p);
				put(opt, "ema_params_binary", d.ema_out.p);
				put(opt, "first_moments_binary", d.m1.p);
				put(opt, "second_moments_binary", d.m2.p);
				put(opt, "param_steps_binary", d.steps.p);
				dm["optimizer"] = opt;
			}
			snap["distortion_map"] = dm;
		}
		write_snapshot(path, root, snap, compress);
	});
}

int ngp_nerf_load_snapshot(ngp_nerf_trainer* t, void* stream, const char* path) {
	if (!t || !path) return NGP_INVALID;
	NGP_TRY({
		t->drain();
		hipStream_t s = S(stream);
		NGP_HIP(hipStreamSynchronize(s));
		const Value root = load_network_config(path);
		NGP_CHECK(root.find("snapshot"), std::string("File '") + path + "' does not contain a snapshot.");
		const Value& snap = root.at("snapshot");
		NGP_CHECK(snap.number_or("version", 0) >= SNAPSHOT_FORMAT_VERSION, "Snapshot uses an old format and can not be loaded.");
		if (const Value* m = snap.find("mode")) NGP_CHECK(m->type == Value::Str && m->s == "nerf", "snapshot: not a NeRF snapshot");
		NGP_CHECK((uint32_t)snap.at("density_grid_size").number() == GRIDSIZE, "Incompatible grid size.");
		trainer_from_snapshot(t->trainer, ngp_model_n_params(t->model), snap);  // tcnn Trainer::deserialize
		// density grid (fp16 in the file)
		const Value& gb = snap.at("density_grid_binary");
		const uint32_t n_el = GRID_N_CELLS * (t->cfg.max_cascade + 1);
		const size_t n_file = gb.s.size() / 2;
		if (n_file == n_el) {
			std::vector<float> g(n_el);
			const f16* h = (const f16*)gb.s.data();
			for (uint32_t k = 0; k < n_el; ++k) g[k] = (float)h[k];
			NGP_HIP(hipMemcpy(t->grid.p, g.data(), (size_t)n_el * 4, hipMemcpyHostToDevice));
			grid_mean_bitfield((const float*)t->grid.p, t->cfg.max_cascade, (float*)t->mean.p, (uint8_t*)t->bitfield.p, s);
		} else {
			// a size of 0 is a never-populated grid (testbed.cu:5000-5005)
			NGP_CHECK(n_file == 0, "Incompatible number of grid cascades.");
		}
		const Value& rgb = snap.at("nerf").at("rgb");
		t->rays_per_batch = (uint32_t)rgb.at("rays_per_batch").number();
		t->measured_batch_size = (uint32_t)rgb.at("measured_batch_size").number();
		t->measured_before_compaction = (uint32_t)rgb.at("measured_batch_size_before_compaction").number();
		t->measured_before_compaction_local = t->measured_before_compaction / t->world;
		t->training_step = (uint32_t)snap.at("training_step").number();
		t->loss_scalar = (float)snap.number_or("loss", 0.0);
		t->ema_step = (uint32_t)snap.number_or("density_grid_ema_step", (double)t->training_step);
		// the refined poses (testbed.cu:5048-5051): the optimisers where the snapshot has them for this many images,
		// zero offsets otherwise; then the cameras from them
		{
			const Value& nerf = snap.at("nerf");
			const Value* pos = nerf.find("cam_pos_offset");
			const Value* rot = nerf.find("cam_rot_offset");
			const size_t n = t->cams.size();
			check_rc(ngp_pose_optimizer_reset(t->pose));
			if (pos && pos->type == Value::Array && pos->arr.size() == n)
				for (uint32_t i = 0; i < n; ++i) {
					const ngp_adam_state st = adam_from_value(pos->arr[i]);
					check_rc(ngp_pose_optimizer_set_state(t->pose, i, &st, nullptr));
				}
			if (rot && rot->type == Value::Array && rot->arr.size() == n)
				for (uint32_t i = 0; i < n; ++i) {
					const ngp_adam_state st = adam_from_value(rot->arr[i]);
					check_rc(ngp_pose_optimizer_set_state(t->pose, i, nullptr, &st));
				}
			// the exposures likewise (engine extension; key absent: zeros)
			const Value* ex = nerf.find("cam_exposure");
			check_rc(ngp_exposure_optimizer_reset(t->expo));
			if (ex && ex->type == Value::Array && ex->arr.size() == n)
				for (uint32_t i = 0; i < n; ++i) {
					const ngp_adam_state st = adam_from_value(ex->arr[i]);
					check_rc(ngp_exposure_optimizer_set_state(t->expo, i, &st));
				}
			t->n_steps_since_cam_update = 0;
			NGP_HIP(hipDeviceSynchronize());
			t->rebuild_cameras(s);
			t->upload_exposures(s);
			NGP_HIP(hipStreamSynchronize(s));
		}
		// the environment map, where the snapshot has one (a snapshot without it leaves this trainer's as it is)
		if (const Value* em = snap.find("envmap")) {
			const uint32_t w = (uint32_t)em->at("width").number(), h = (uint32_t)em->at("height").number();
			NGP_CHECK(envmap_dims_ok(w, h), "snapshot: envmap resolution");
			const size_t n = (size_t)w * h * 4;
			auto bin = [&](const Value& v, const char* name) -> const float* {
				const Value* b = v.find(name);
				if (!b) return nullptr;
				NGP_CHECK(b->s.size() == n * 4, std::string("snapshot: envmap ") + name + " size");
				return (const float*)b->s.data();
			};
			const float* params = bin(*em, "params_binary");
			NGP_CHECK(params, "snapshot: envmap without params_binary");
			check_rc(ngp_nerf_trainer_set_envmap(t, w, h, params));
			ngp_nerf_trainer::Envmap& e = t->env;
			auto up = [&](Buf& dst, const float* src) {
				if (src) NGP_HIP(hipMemcpy(dst.p, src, n * 4, hipMemcpyHostToDevice));
			};
			if (const float* ema = bin(*em, "ema_params_binary")) {
				up(e.ema_out, ema);
				e.ema_valid = true;
			}
			if (const Value* opt = em->find("optimizer")) {
				e.step = (uint32_t)opt->number_or("current_step", 0.0);
				e.ema_valid = opt->number_or("ema_valid", 1.0) != 0.0;
				up(e.ema, bin(*opt, "ema_binary"));
				up(e.m1, bin(*opt, "first_moments_binary"));
				up(e.m2, bin(*opt, "second_moments_binary"));
				up(e.steps, bin(*opt, "param_steps_binary"));
			}
		}
		// the lens distortion map likewise
		if (const Value* dm = snap.find("distortion_map")) {
			const uint32_t w = (uint32_t)dm->at("width").number(), h = (uint32_t)dm->at("height").number();
			NGP_CHECK(distortion_dims_ok(w, h), "snapshot: distortion_map resolution");
			const size_t n = (size_t)w * h * 2;
			auto bin = [&](const Value& v, const char* name) -> const float* {
				const Value* b = v.find(name);
				if (!b) return nullptr;
				NGP_CHECK(b->s.size() == n * 4, std::string("snapshot: distortion_map ") + name + " size");
				return (const float*)b->s.data();
			};
			const float* params = bin(*dm, "params_binary");
			NGP_CHECK(params, "snapshot: distortion_map without params_binary");
			check_rc(ngp_nerf_trainer_set_distortion_map(t, w, h, params));
			ngp_nerf_trainer::Distortion& d = t->dist;
			auto up = [&](Buf& dst, const float* src) {
				if (src) NGP_HIP(hipMemcpy(dst.p, src, n * 4, hipMemcpyHostToDevice));
			};
			if (const Value* opt = dm->find("optimizer")) {
				d.step = (uint32_t)opt->number_or("current_step", 0.0);
				d.ema_valid = opt->number_or("ema_valid", 0.0) != 0.0;
				up(d.ema, bin(*opt, "ema_binary"));
				up(d.ema_out, bin(*opt, "ema_params_binary"));
				up(d.m1, bin(*opt, "first_moments_binary"));
				up(d.m2, bin(*opt, "second_moments_binary"));
				up(d.steps, bin(*opt, "param_steps_binary"));
			}
		}
		NGP_HIP(hipStreamSynchronize(s));
	});
}

// Testbed::save_snapshot / load_snapshot for the image and SDF testbeds (testbed.cu:4873-4937, 4939-5057): the
// mode-independent members (Trainer::serialize, version, mode, training_step, loss, aabb, bounding_radius).
int ngp_save_snapshot(ngp_trainer* t, void* stream, const char* path, const char* network_config_json, const char* mode,
                      const float* aabb_min, const float* aabb_max, float bounding_radius, uint32_t training_step, float loss,
                      int include_optimizer_state, int compress) {
	if (!t || !path || !mode) return NGP_INVALID;
	NGP_TRY({
		NGP_HIP(hipStreamSynchronize(S(stream)));
		Value root = snapshot_root(network_config_json);
		Value snap = Value::object();
		trainer_to_snapshot(t, ngp_trainer_n_params(t), include_optimizer_state != 0, snap);
		snap["version"] = Value::uint(SNAPSHOT_FORMAT_VERSION);
		snap["mode"] = Value::str(mode);
		snap["training_step"] = Value::uint(training_step);
		snap["loss"] = Value::real(loss);
		const float zero[3] = {0.f, 0.f, 0.f}, one[3] = {1.f, 1.f, 1.f};
		snap["aabb"]["min"] = vec3(aabb_min ? aabb_min : zero);
		snap["aabb"]["max"] = vec3(aabb_max ? aabb_max : one);
		snap["bounding_radius"] = Value::real(bounding_radius);
		write_snapshot(path, root, snap, compress);
	});
}

int ngp_load_snapshot(ngp_trainer* t, void* stream, const char* path, uint32_t* training_step, float* loss, float* aabb_min,
                      float* aabb_max, float* bounding_radius) {
	if (!t || !path) return NGP_INVALID;
	NGP_TRY({
		NGP_HIP(hipStreamSynchronize(S(stream)));
		const Value root = load_network_config(path);
		NGP_CHECK(root.find("snapshot"), std::string("File '") + path + "' does not contain a snapshot.");
		const Value& snap = root.at("snapshot");
		NGP_CHECK(snap.number_or("version", 0) >= SNAPSHOT_FORMAT_VERSION, "Snapshot uses an old format and can not be loaded.");
		trainer_from_snapshot(t, ngp_trainer_n_params(t), snap);
		if (training_step) *training_step = (uint32_t)snap.number_or("training_step", 0.0);
		if (loss) *loss = (float)snap.number_or("loss", 0.0);
		if (bounding_radius) *bounding_radius = (float)snap.number_or("bounding_radius", (double)*bounding_radius);
		if (const Value* a = snap.find("aabb")) {
			for (int d = 0; d < 3; ++d) {
				if (aabb_min) aabb_min[d] = (float)a->at("min").arr.at(d).number();
				if (aabb_max) aabb_max[d] = (float)a->at("max").arr.at(d).number();
			}
		}
	});
}

// The snapshot's mode ("nerf", "sdf", "image", ...; testbed.cu:4950-4957: a snapshot without one but with a "nerf"
// member is a NeRF snapshot), so that a Testbed can switch mode before reset_network
int ngp_snapshot_mode(const char* path, char* mode_buf, uint64_t cap) {
	if (!path || !mode_buf || cap == 0) return NGP_INVALID;
	NGP_TRY({
		const Value root = load_network_config(path);
		NGP_CHECK(root.find("snapshot"), std::string("File '") + path + "' does not contain a snapshot.");
		const Value& snap = root.at("snapshot");
		std::string m;
		if (const Value* v = snap.find("mode")) m = v->s;
		else if (snap.find("nerf")) m = "nerf";
		NGP_CHECK(!m.empty(), "Unknown snapshot mode. Snapshot must be regenerated with a new version of instant-ngp.");
		NGP_CHECK(m.size() + 1 <= cap, "snapshot mode: buffer too small");
		memcpy(mode_buf, m.c_str(), m.size() + 1);
	});
}

int ngp_snapshot_network_config(const char* path, char* json_buf, uint64_t* size) {
	if (!path || !size) return NGP_INVALID;
	NGP_TRY({
		Value root = load_network_config(path);
		NGP_CHECK(root.is_map(), "snapshot: top level is not a map");
		root.erase("snapshot");
		std::string text;
		ngp::mp::to_json_text(root, text);
		if (!json_buf) { *size = text.size() + 1; return NGP_OK; }
		NGP_CHECK(*size >= text.size() + 1, "snapshot: buffer too small");
		memcpy(json_buf, text.c_str(), text.size() + 1);
		*size = text.size() + 1;
	});
}

}  // extern "C"
