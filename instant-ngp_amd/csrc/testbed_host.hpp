// testbed_host.hpp — the Testbed host (include/neural-graphics-primitives/testbed.h, src/testbed.cu) in plain
// C++17 over the engine's C-ABI (include/ngp_engine.h): mode dispatch, network (re)construction from the
// JSON config, Testbed::train / frame (headless), snapshots and the NeRF render of a camera. It holds no HIP
// code and no HIP headers: device buffers come from ngp_malloc, every kernel runs behind the C-ABI.
//
// Reference surface mirrored (names and argument meaning):
//   Testbed(mode) / load_training_data(path) / clear_training_data      testbed.cu:139-176
//   reload_network_from_file / reload_network_from_json                 testbed.cu:228-314 (parent merge)
//   reset_network(clear_density_grid)                                    testbed.cu:3903-4151
//   train(batch_size)                                                    testbed.cu:4285-4370
//   frame() (headless: train when shall_train)                           testbed.cu:3595-3761
//   n_params / n_encoding_params                                         testbed.cu:4843-4856
//   save_snapshot / load_snapshot                                        testbed.cu:4873-5057
//   set_camera_to_training_view / render_to_cpu                          testbed.cu:848-856, python_api.cu:418-427
//   render_sdf (through ngp_sdf_render) / calculate_iou                  testbed_sdf.cu:883-1063, 1329-1364
//   compute_marching_cubes_mesh / compute_and_save_marching_cubes_mesh   testbed.h:472, python_api.cu:101-125
// What lives elsewhere: decoding image files (JPEG/PNG/EXR) is the binding's job (python_api.cpp hands the
// decoded pixels to load_nerf / load_image), as the reference delegates it to stb_image / tinyexr.
#pragma once

#include <algorithm>
#include <cctype>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <fstream>
#include <sstream>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/ngp_engine.h"
#include "json.h"

namespace ngp_host {

using ngp::Json;

enum class ETestbedMode : int { Nerf, Sdf, Image, Volume, None };  // common.h:186-192
enum class ERenderMode : int { AO, Shade, Normals, Positions, Depth, Distortion, Cost, Slice };  // common.h:110-119

inline void check(int rc, const char* what) {
	if (rc != NGP_OK) throw std::runtime_error(std::string(what) + ": " + ngp_last_error());
}

inline bool iends_with(const std::string& s, const std::string& suffix) {
	if (s.size() < suffix.size()) return false;
	return ngp::iequals(s.substr(s.size() - suffix.size()), suffix);
}

inline bool is_directory(const std::string& p) {
	std::ifstream f(p + "/.");
	return f.good();
}

// mode_from_scene (common.cu:144-159): directories and .json are NeRF, .obj/.stl SDF, .nvdb volume, else an image
inline ETestbedMode mode_from_scene(const std::string& scene) {
	std::ifstream probe(scene);
	if (!probe.good() && !is_directory(scene)) return ETestbedMode::None;
	if (is_directory(scene) || iends_with(scene, ".json")) return ETestbedMode::Nerf;
	if (iends_with(scene, ".obj") || iends_with(scene, ".stl")) return ETestbedMode::Sdf;
	if (iends_with(scene, ".nvdb")) return ETestbedMode::Volume;
	return ETestbedMode::Image;
}

// to_string(ETestbedMode) (common.cu:175-184)
inline const char* mode_name(ETestbedMode m) {
	switch (m) {
	case ETestbedMode::Nerf: return "nerf";
	case ETestbedMode::Sdf: return "sdf";
	case ETestbedMode::Image: return "image";
	case ETestbedMode::Volume: return "volume";
	default: return "none";
	}
}

// mode_from_string (common.cu:161-173)
inline ETestbedMode mode_from_string(const std::string& s) {
	if (ngp::iequals(s, "nerf")) return ETestbedMode::Nerf;
	if (ngp::iequals(s, "sdf")) return ETestbedMode::Sdf;
	if (ngp::iequals(s, "image")) return ETestbedMode::Image;
	if (ngp::iequals(s, "volume")) return ETestbedMode::Volume;
	return ETestbedMode::None;
}

// RFC 7386 merge patch (nlohmann::json::merge_patch, the config `parent` merge of testbed.cu:95-106)
inline Json merge_patch(const Json& base, const Json& patch) {
	if (patch.type != Json::Object) return patch;
	Json out = base.type == Json::Object ? base : Json{};
	out.type = Json::Object;
	for (const auto& kv : patch.obj) {
		if (kv.second.type == Json::Null) out.obj.erase(kv.first);
		else out.obj[kv.first] = merge_patch(out.contains(kv.first) ? out.obj[kv.first] : Json{}, kv.second);
	}
	return out;
}

inline std::string read_text(const std::string& path) {
	std::ifstream f(path, std::ios::binary);
	if (!f) throw std::runtime_error("cannot open " + path);
	std::stringstream ss;
	ss << f.rdbuf();
	return ss.str();
}

// Testbed::load_network_config (testbed.cu:228-314): a config file, its "parent" merged underneath
inline Json load_network_config(const std::string& path) {
	Json cfg = Json::parse(read_text(path));
	if (cfg.contains("parent")) {
		const std::string dir = path.find('/') == std::string::npos ? "." : path.substr(0, path.rfind('/'));
		Json parent = load_network_config(dir + "/" + cfg["parent"].str);
		cfg.obj.erase("parent");
		cfg = merge_patch(parent, cfg);
	}
	return cfg;
}

// configs/<mode>/base.json of the reference fork, restated as data (nothing under the reference tree is read
// at run time); instant-ngp_amd/config.py holds the same dicts (tests/test_pyngp.py checks they agree)
inline std::string default_network_config(ETestbedMode mode) {
	switch (mode) {
	case ETestbedMode::Nerf:  // configs/nerf/base.json (fork: L=4, F=4, T=2^19)
		return R"({"loss": {"otype": "Huber"},
 "optimizer": {"otype": "Ema", "decay": 0.95, "nested": {"otype": "ExponentialDecay", "decay_start": 20000,
   "decay_interval": 10000, "decay_base": 0.33, "nested": {"otype": "Adam", "learning_rate": 1e-2, "beta1": 0.9,
   "beta2": 0.99, "epsilon": 1e-15, "l2_reg": 1e-6}}},
 "encoding": {"otype": "HashGrid", "n_levels": 4, "n_features_per_level": 4, "log2_hashmap_size": 19, "base_resolution": 16},
 "network": {"otype": "FullyFusedMLP", "activation": "ReLU", "output_activation": "None", "n_neurons": 64, "n_hidden_layers": 1},
 "dir_encoding": {"otype": "Composite", "nested": [{"n_dims_to_encode": 3, "otype": "SphericalHarmonics", "degree": 4},
   {"otype": "Identity"}]},
 "rgb_network": {"otype": "FullyFusedMLP", "activation": "ReLU", "output_activation": "None", "n_neurons": 64, "n_hidden_layers": 2},
 "distortion_map": {"resolution": [32, 32], "optimizer": {"otype": "ExponentialDecay", "decay_start": 10000,
   "decay_interval": 5000, "decay_end": 25000, "decay_base": 0.33, "nested": {"otype": "Adam", "learning_rate": 1e-4, "beta1": 0.9,
   "beta2": 0.99, "epsilon": 1e-8}}}})";
	case ETestbedMode::Sdf:  // configs/sdf/base.json
		return R"({"loss": {"otype": "MAPE"},
 "optimizer": {"otype": "Ema", "decay": 0.95, "nested": {"otype": "ExponentialDecay", "decay_start": 10000,
   "decay_interval": 5000, "decay_base": 0.33, "nested": {"otype": "Adam", "learning_rate": 1e-4, "beta1": 0.9,
   "beta2": 0.99, "epsilon": 1e-15, "l2_reg": 1e-6}}},
 "encoding": {"otype": "HashGrid", "n_levels": 16, "n_features_per_level": 2, "log2_hashmap_size": 19, "base_resolution": 16},
 "network": {"otype": "FullyFusedMLP", "activation": "ReLU", "output_activation": "None", "n_neurons": 64, "n_hidden_layers": 2}})";
	case ETestbedMode::Image:  // configs/image/base.json
		return R"({"loss": {"otype": "L2"},
 "optimizer": {"otype": "ExponentialDecay", "decay_start": 20000, "decay_interval": 10000, "decay_base": 0.33,
   "nested": {"otype": "Adam", "learning_rate": 1e-2, "beta1": 0.9, "beta2": 0.99, "epsilon": 1e-15, "l2_reg": 1e-6}},
 "encoding": {"otype": "HashGrid", "n_levels": 16, "n_features_per_level": 2, "log2_hashmap_size": 24, "base_resolution": 16},
 "network": {"otype": "FullyFusedMLP", "activation": "ReLU", "output_activation": "None", "n_neurons": 64, "n_hidden_layers": 2}})";
	default:
		throw std::runtime_error("no network config for this mode (volume rendering is out of scope, SURVEY §2)");
	}
}

// OBJ triangle soup (tinyobjloader's role in Testbed::load_mesh, testbed_sdf.cu:1120): vertices of every
// face, fans triangulated; returns [3T x 3] floats
inline std::vector<float> read_obj_triangles(const std::string& path) {
	std::ifstream f(path);
	if (!f) throw std::runtime_error("cannot open " + path);
	std::vector<float> v, out;
	std::string line;
	while (std::getline(f, line)) {
		std::istringstream ls(line);
		std::string tag;
		ls >> tag;
		if (tag == "v") {
			float x, y, z;
			ls >> x >> y >> z;
			v.insert(v.end(), {x, y, z});
		} else if (tag == "f") {
			std::vector<long> idx;
			std::string tok;
			while (ls >> tok) {
				long i = std::stol(tok.substr(0, tok.find('/')));
				idx.push_back(i < 0 ? (long)(v.size() / 3) + i : i - 1);
			}
			for (size_t k = 2; k < idx.size(); ++k)
				for (long i : {idx[0], idx[k - 1], idx[k]}) {
					if (i < 0 || (size_t)i * 3 + 2 >= v.size()) throw std::runtime_error("obj: face index out of range");
					out.insert(out.end(), {v[i * 3], v[i * 3 + 1], v[i * 3 + 2]});
				}
		}
	}
	if (out.empty()) throw std::runtime_error("obj: no triangles in " + path);
	return out;
}

inline float half_to_float(uint16_t h) {
	const uint32_t s = (h >> 15) & 1, e = (h >> 10) & 31, m = h & 1023;
	float v;
	if (e == 0) v = std::ldexp((float)m, -24);
	else if (e == 31) v = m ? NAN : INFINITY;
	else v = std::ldexp((float)(m | 1024), (int)e - 25);
	return s ? -v : v;
}
inline float linear_to_srgb(float x) { return x < 0.0031308f ? 12.92f * x : 1.055f * std::pow(std::max(x, 0.f), 0.41666f) - 0.055f; }
inline float srgb_to_linear(float x) { return x <= 0.04045f ? x / 12.92f : std::pow((x + 0.055f) / 1.055f, 2.4f); }

struct DeviceBuffer {
	void* p = nullptr;
	size_t bytes = 0;
	DeviceBuffer() = default;
	DeviceBuffer(const DeviceBuffer&) = delete;
	DeviceBuffer& operator=(const DeviceBuffer&) = delete;
	~DeviceBuffer() { if (p) ngp_free(p); }
	template <typename T> T* get(size_t n) {
		const size_t b = n * sizeof(T);
		if (b > bytes) {
			if (p) ngp_free(p);
			p = nullptr;
			check(ngp_malloc(&p, b), "ngp_malloc");
			bytes = b;
		}
		return (T*)p;
	}
};

class Testbed {
public:
	explicit Testbed(ETestbedMode mode = ETestbedMode::None) {
		check(ngp_sdf_render_default_config(&m_sdf_render_cfg), "ngp_sdf_render_default_config");  // no GPU call
		std::memcpy(m_sun_dir, m_sdf_render_cfg.sun_dir, sizeof(m_sun_dir));
		std::memcpy(m_up_dir, m_sdf_render_cfg.up_dir, sizeof(m_up_dir));
		set_mode(mode);
	}
	~Testbed() { free_network(); free_data(); }
	Testbed(const Testbed&) = delete;
	Testbed& operator=(const Testbed&) = delete;

	// ---- mode and configuration -------------------------------------------------------------------
	ETestbedMode mode() const { return m_testbed_mode; }
	// Testbed::set_mode (testbed.cu:178-226): a new mode drops the network, the data and the config
	void set_mode(ETestbedMode mode) {
		if (mode == m_testbed_mode && m_mode_set) return;
		free_network();
		free_data();
		m_testbed_mode = mode;
		m_mode_set = true;
		m_training_step = 0;
		m_network_config = mode == ETestbedMode::None || mode == ETestbedMode::Volume ? Json{}
		                                                                                 : Json::parse(default_network_config(mode));
	}
	void reload_network_from_json(const std::string& json_text) {
		m_network_config = Json::parse(json_text);
		reset_network();
	}
	void reload_network_from_file(const std::string& path) {
		if (!path.empty()) m_network_config = load_network_config(path);
		else if (m_network_config.type != Json::Object) m_network_config = Json::parse(default_network_config(m_testbed_mode));
		reset_network();
	}
	std::string network_config() const { return m_network_config.dump(); }

	// ---- training data ------------------------------------------------------------------------------
	// Testbed::load_nerf + load_nerf_post (testbed_nerf.cu:3093-3109): decoded images (RGBA8 sRGB, or with `types` an
	// NGP_IMAGE_* type per image: EXR frames come as Half) with their metadata after nerf_matrix_to_ngp, and the
	// dataset's aabb_scale
	void load_nerf(const std::vector<ngp_nerf_image>& images, const std::vector<const void*>& rgba8, float aabb_scale,
	               float dataset_scale = 1.0f, const float* dataset_offset = nullptr, const std::vector<uint32_t>* types = nullptr) {
		set_mode(ETestbedMode::Nerf);
		if (images.empty() || images.size() != rgba8.size()) throw std::runtime_error("load_nerf: one RGBA8 buffer per image");
		if (types && types->size() != images.size()) throw std::runtime_error("load_nerf: one image type per image");
		free_network();
		free_data();
		bool hdr = false;
		if (types) for (uint32_t t : *types) hdr = hdr || t != NGP_IMAGE_BYTE;
		if (hdr)
			check(ngp_nerf_dataset_create_typed((uint32_t)images.size(), images.data(), rgba8.data(), types->data(), &m_nerf_dataset),
			      "ngp_nerf_dataset_create_typed");
		else
			check(ngp_nerf_dataset_create((uint32_t)images.size(), images.data(), rgba8.data(), &m_nerf_dataset), "ngp_nerf_dataset_create");
		m_nerf_is_hdr = hdr;  // NerfDataset::is_hdr: set by the loader, not changed by set_image_pixels (nerf_loader.cu:553)
		m_nerf_images = images;
		m_aabb_scale = aabb_scale;
		m_dataset_scale = dataset_scale;  // NerfDataset::scale (nerf_loader.cu:388): Depth renders in its units
		for (int d = 0; d < 3; ++d) m_dataset_offset[d] = dataset_offset ? dataset_offset[d] : 0.5f;  // NerfDataset::offset
		check(ngp_nerf_default_config(aabb_scale, &m_nerf_cfg), "ngp_nerf_default_config");
		if (m_nerf_is_hdr) m_nerf_cfg.rgb_activation = 3;  // load_nerf_post (testbed_nerf.cu:3027): Exponential for an HDR dataset
		m_training_data_available = true;
		set_camera_to_training_view(0);
	}
	// Testbed::load_image (testbed_image.cu:372-402): RGBA float [h x w x 4], linear colours
	void load_image(uint32_t width, uint32_t height, const float* rgba) {
		set_mode(ETestbedMode::Image);
		free_network();
		free_data();
		check(ngp_image_create(width, height, rgba, &m_image), "ngp_image_create");
		check(ngp_image_default_config(&m_image_cfg), "ngp_image_default_config");
		m_image_res[0] = width;
		m_image_res[1] = height;
		m_training_data_available = true;
	}
	// Testbed::load_mesh (testbed_sdf.cu:1120-1165): triangle soup [3T x 3] normalised into the unit cube
	void load_mesh(const std::vector<float>& vertices) {
		set_mode(ETestbedMode::Sdf);
		free_network();
		free_data();
		const size_t nv = vertices.size() / 3;
		if (nv == 0 || nv % 3 != 0) throw std::runtime_error("load_mesh: vertices must hold whole triangles");
		float lo[3], hi[3];
		for (int d = 0; d < 3; ++d) { lo[d] = INFINITY; hi[d] = -INFINITY; }
		for (size_t i = 0; i < nv; ++i)
			for (int d = 0; d < 3; ++d) { lo[d] = std::min(lo[d], vertices[i * 3 + d]); hi[d] = std::max(hi[d], vertices[i * 3 + d]); }
		const float inflation = 0.005f;
		auto norm = [](const float* a, const float* b) {
			float s = 0.f;
			for (int d = 0; d < 3; ++d) s += (b[d] - a[d]) * (b[d] - a[d]);
			return std::sqrt(s);
		};
		float amount = norm(lo, hi) * inflation;
		for (int d = 0; d < 3; ++d) { lo[d] -= amount; hi[d] += amount; }
		float diag[3], scale = 0.f;
		for (int d = 0; d < 3; ++d) { diag[d] = hi[d] - lo[d]; scale = std::max(scale, diag[d]); }
		std::vector<float> tris(vertices.size());
		float alo[3], ahi[3];
		for (int d = 0; d < 3; ++d) { alo[d] = INFINITY; ahi[d] = -INFINITY; }
		for (size_t i = 0; i < nv; ++i)
			for (int d = 0; d < 3; ++d) {
				const float v = (vertices[i * 3 + d] - lo[d] - 0.5f * diag[d]) / scale + 0.5f;
				tris[i * 3 + d] = v;
				alo[d] = std::min(alo[d], v);
				ahi[d] = std::max(ahi[d], v);
			}
		amount = norm(alo, ahi) * inflation;
		for (int d = 0; d < 3; ++d) {
			m_sdf_aabb_min[d] = std::max(alo[d] - amount, 0.f);
			m_sdf_aabb_max[d] = std::min(ahi[d] + amount, 1.f);
		}
		m_bounding_radius = std::sqrt(0.75f);
		check(ngp_sdf_mesh_create((uint32_t)(nv / 3), tris.data(), &m_sdf_mesh), "ngp_sdf_mesh_create");
		m_training_data_available = true;
	}
	void load_mesh_file(const std::string& path) { load_mesh(read_obj_triangles(path)); }
	void clear_training_data() {
		free_network();
		free_data();
	}
	bool training_data_available() const { return m_training_data_available; }

	// ---- network ------------------------------------------------------------------------------------
	// Testbed::reset_network (testbed.cu:3903-4151): the model from the config sections, a trainer seeded
	// from m_seed, and for NeRF the training state (density grid, counters, rng). reset_density_grid = false
	// keeps the occupancy grid of the previous network.
	void reset_network(bool reset_density_grid = true) {
		if (m_testbed_mode == ETestbedMode::None) throw std::runtime_error("reset_network: no mode");
		if (m_testbed_mode == ETestbedMode::Volume) throw std::runtime_error("the volume primitive is out of scope (SURVEY §2)");
		std::vector<float> kept_grid;
		if (!reset_density_grid && m_nerf_trainer) {
			const float* g = nullptr;
			const uint8_t* b = nullptr;
			const float* m = nullptr;
			check(ngp_nerf_trainer_buffers_read(m_nerf_trainer, &g, &b, &m), "ngp_nerf_trainer_buffers_read");
			kept_grid.resize((size_t)128 * 128 * 128 * (m_nerf_cfg.max_cascade + 1));
			check(ngp_memcpy(kept_grid.data(), g, kept_grid.size() * 4, 2 /* device to host */), "ngp_memcpy");
		}
		free_network();
		m_training_step = 0;
		m_loss_scalar = 0.f;
		// testbed.cu:3975-3997: a missing base_resolution becomes 2^(log2_hashmap_size / n_pos) and is written
		// into the config. per_level_scale: the fork sets only its log member to 2.0 (:3991), so the auto-scale
		// branch never runs and the encoding config reaches the network unchanged (:4037): a config's own value
		// stays (configs/nerf/densegrid.json 1.405), an absent key is tcnn's default 2.0 (parse_grid)
		Json enc = m_network_config["encoding"];
		const uint32_t n_pos = m_testbed_mode == ETestbedMode::Image ? 2u : 3u;
		if (enc.number_or("base_resolution", 0.0) == 0.0) {
			enc.obj["base_resolution"].type = Json::Number;
			enc.obj["base_resolution"].num = (double)(1u << ((uint32_t)enc.number_or("log2_hashmap_size", 15.0) / n_pos));
		}
		const std::string opt = m_network_config["optimizer"].dump();
		switch (m_testbed_mode) {
		case ETestbedMode::Nerf: {
			const Json& c = m_network_config;
			check(ngp_nerf_network_create(3, 3, 0, 4, enc.dump().c_str(), c.contains("dir_encoding") ? c["dir_encoding"].dump().c_str() : nullptr,
			                              c["network"].dump().c_str(), c["rgb_network"].dump().c_str(), &m_model),
			      "ngp_nerf_network_create");
			break;
		}
		case ETestbedMode::Image:
			check(ngp_network_with_input_encoding_create(2, 3, enc.dump().c_str(), m_network_config["network"].dump().c_str(), &m_model),
			      "ngp_network_with_input_encoding_create");
			break;
		case ETestbedMode::Sdf:
			check(ngp_network_with_input_encoding_create(3, 1, enc.dump().c_str(), m_network_config["network"].dump().c_str(), &m_model),
			      "ngp_network_with_input_encoding_create");
			break;
		default: break;
		}
		check(ngp_trainer_create(m_model, opt.c_str(), m_seed, &m_trainer), "ngp_trainer_create");
		m_rng = host_pcg32(m_seed);
		if (m_testbed_mode == ETestbedMode::Nerf && m_nerf_dataset) {
			check(ngp_nerf_trainer_create(m_model, m_trainer, m_nerf_dataset, &m_nerf_cfg, m_seed, &m_nerf_trainer),
			      "ngp_nerf_trainer_create");
			if (!kept_grid.empty()) {
				float* g = nullptr;
				uint8_t* b = nullptr;
				float* m = nullptr;
				check(ngp_nerf_trainer_buffers(m_nerf_trainer, &g, &b, &m), "ngp_nerf_trainer_buffers");
				check(ngp_memcpy(g, kept_grid.data(), kept_grid.size() * 4, 1 /* host to device */), "ngp_memcpy");
			}
			push_camera_training();
			push_error_sampling();
			push_envmap();
			push_depth_supervision();
			push_exposure_training();
			push_distortion_training();
		}
	}
	uint64_t n_params() const { return m_model ? ngp_model_n_params(m_model) : 0; }
	uint64_t n_encoding_params() const {
		if (!m_model) return 0;
		ngp_param_layout lo;
		check(ngp_model_param_layout(m_model, &lo), "ngp_model_param_layout");
		return lo.grid_params;
	}
	// the encoding's "interpolation" as the model parsed it from the network config ("" before reset_network)
	std::string grid_interpolation() const {
		if (!m_model) return "";
		double v = 0.0;
		check(ngp_model_query(m_model, "grid_interpolation", &v), "ngp_model_query");
		return v == 1.0 ? "Smoothstep" : "Linear";
	}

	// ---- training -----------------------------------------------------------------------------------
	// Testbed::train (testbed.cu:4285-4370); the loss is read back every 16 steps, as the reference does
	void train(uint32_t batch_size) {
		if (!m_training_data_available) {
			m_train = false;
			return;
		}
		if (m_testbed_mode == ETestbedMode::None) throw std::runtime_error("Cannot train without a mode.");
		if (!m_trainer) reset_network();
		const bool get_loss = m_training_step % 16 == 0;
		switch (m_testbed_mode) {
		case ETestbedMode::Nerf: {
			if (batch_size != m_nerf_cfg.target_batch_size) {
				m_nerf_cfg.target_batch_size = batch_size;
				push_nerf_config();
			}
			ngp_nerf_stats st;
			check(ngp_nerf_train_step(m_nerf_trainer, nullptr, get_loss ? 1 : 0, &st), "ngp_nerf_train_step");
			if (get_loss) m_loss_scalar = st.loss;
			m_training_step = st.step;
			return;
		}
		case ETestbedMode::Image: {
			float* loss = m_loss_dev.get<float>(1);
			if (get_loss) check(ngp_memcpy(loss, &ZERO, 4, 1), "ngp_memcpy");
			check(ngp_image_train_step(m_image, m_trainer, nullptr, batch_size, &m_rng, &m_image_cfg, get_loss ? loss : nullptr),
			      "ngp_image_train_step");
			break;
		}
		case ETestbedMode::Sdf: {
			const uint32_t n = batch_size / 8 * 8;
			float* pos = m_sdf_pos.get<float>((size_t)n * 3);
			float* dist = m_sdf_dist.get<float>(n);
			float* pos_s = m_sdf_pos_s.get<float>((size_t)n * 3);
			float* dist_s = m_sdf_dist_s.get<float>(n);
			float* loss = m_loss_dev.get<float>(1);
			if (get_loss) check(ngp_memcpy(loss, &ZERO, 4, 1), "ngp_memcpy");
			// generate_sdf_data_online (testbed.h:842): the batch is regenerated every step
			if (m_sdf_generate_online || m_training_step == 0) {
				const float stddev = m_bounding_radius / 1024.0f * m_sdf_surface_offset_scale;
				check(ngp_sdf_generate_training_samples(m_sdf_mesh, nullptr, n, &m_rng, m_sdf_aabb_min, m_sdf_aabb_max, stddev, pos, dist),
				      "ngp_sdf_generate_training_samples");
			}
			check(ngp_sdf_train_step(m_trainer, nullptr, n, pos, dist, m_training_step, pos_s, dist_s, get_loss ? loss : nullptr),
			      "ngp_sdf_train_step");
			break;
		}
		default: throw std::runtime_error("Invalid training mode.");
		}
		check(ngp_stream_synchronize(nullptr), "ngp_stream_synchronize");
		if (get_loss) {
			float l = 0.f;
			check(ngp_memcpy(&l, m_loss_dev.p, 4, 2), "ngp_memcpy");
			m_loss_scalar = l;
		}
		++m_training_step;
	}
	// Testbed::frame (testbed.cu:3595-3761) without a window: train_and_render trains when shall_train
	bool frame() {
		if (m_train) train(m_training_batch_size);
		return true;
	}
	float loss() const { return m_loss_scalar; }
	uint32_t training_step() const { return m_training_step; }

	// ---- snapshots (the .ingp / msgpack format of testbed.cu:4873-5057, every mode) -----------------------
	void save_snapshot(const std::string& path, bool include_optimizer_state, bool compress) {
		if (m_testbed_mode == ETestbedMode::Nerf) {
			require_nerf_trainer("save_snapshot");
			check(ngp_nerf_save_snapshot(m_nerf_trainer, nullptr, path.c_str(), m_network_config.dump().c_str(),
			                             include_optimizer_state ? 1 : 0, compress ? 1 : 0),
			      "ngp_nerf_save_snapshot");
			return;
		}
		if (!m_trainer) throw std::runtime_error("save_snapshot: no network (train first)");
		const float img_min[3] = {0.f, 0.f, 0.f}, img_max[3] = {1.f, 1.f, 1.f};
		const bool sdf = m_testbed_mode == ETestbedMode::Sdf;
		check(ngp_save_snapshot(m_trainer, nullptr, path.c_str(), m_network_config.dump().c_str(), mode_name(m_testbed_mode),
		                        sdf ? m_sdf_aabb_min : img_min, sdf ? m_sdf_aabb_max : img_max, m_bounding_radius, m_training_step,
		                        m_loss_scalar, include_optimizer_state ? 1 : 0, compress ? 1 : 0),
		      "ngp_save_snapshot");
	}
	// Testbed::load_snapshot (testbed.cu:4939-5057): the snapshot's mode (a different one drops the loaded data, as
	// set_mode does), its network config, then the trainer state and the mode's members
	void load_snapshot(const std::string& path) {
		char mode[32];
		check(ngp_snapshot_mode(path.c_str(), mode, sizeof mode), "ngp_snapshot_mode");
		const ETestbedMode m = mode_from_string(mode);
		if (m == ETestbedMode::None || m == ETestbedMode::Volume)
			throw std::runtime_error(std::string("load_snapshot: unsupported snapshot mode '") + mode + "'");
		set_mode(m);
		if (m == ETestbedMode::Nerf && !m_nerf_dataset)
			throw std::runtime_error("load_snapshot: load the NeRF training data first (the snapshot's dataset member is not read)");
		uint64_t size = 0;
		check(ngp_snapshot_network_config(path.c_str(), nullptr, &size), "ngp_snapshot_network_config");
		std::string cfg(size, '\0');
		check(ngp_snapshot_network_config(path.c_str(), &cfg[0], &size), "ngp_snapshot_network_config");
		cfg.resize(strlen(cfg.c_str()));
		m_network_config = Json::parse(cfg);
		reset_network();
		if (m == ETestbedMode::Nerf) {
			check(ngp_nerf_load_snapshot(m_nerf_trainer, nullptr, path.c_str()), "ngp_nerf_load_snapshot");
			m_training_step = ngp_trainer_step(m_trainer);  // one optimizer step per training step
			return;
		}
		float amin[3], amax[3];
		check(ngp_load_snapshot(m_trainer, nullptr, path.c_str(), &m_training_step, &m_loss_scalar, amin, amax, &m_bounding_radius),
		      "ngp_load_snapshot");
		if (m == ETestbedMode::Sdf) {
			std::memcpy(m_sdf_aabb_min, amin, sizeof amin);
			std::memcpy(m_sdf_aabb_max, amax, sizeof amax);
		}
	}

	// ---- camera and rendering -----------------------------------------------------------------------
	// set_camera_to_training_view (testbed.cu:848-856): the view's camera, relative focal length and screen centre
	void set_camera_to_training_view(uint32_t i) {
		if (i >= m_nerf_images.size()) throw std::runtime_error("set_camera_to_training_view: no such training view");
		const ngp_nerf_image& im = m_nerf_images[i];
		training_view_xform(i, m_camera);  // m_nerf.training.transforms[i].start: the refined pose
		const float res_axis = (float)(m_fov_axis == 0 ? im.width : im.height);
		m_relative_focal_length[0] = im.focal_length[0] / res_axis;
		m_relative_focal_length[1] = im.focal_length[1] / res_axis;
		m_screen_center[0] = 1.0f - im.principal_point[0];
		m_screen_center[1] = 1.0f - im.principal_point[1];
		m_lens_mode = im.lens_mode;
		std::memcpy(m_lens_params, im.lens_params, sizeof(m_lens_params));
		m_training_view = i;
	}
	uint32_t n_training_views() const { return (uint32_t)m_nerf_images.size(); }
	// render_to_cpu (python_api.cu:418-427): an RGBA float image [height x width x 4], linear colours or sRGB.
	// NeRF: the NerfTracer over the occupancy bitfield with the inference (EMA) parameters, spp samples
	// averaged; Image: the network evaluated at the pixel centres.
	std::vector<float> render(uint32_t width, uint32_t height, uint32_t spp, bool linear) {
		if (width == 0 || height == 0 || spp == 0) throw std::runtime_error("render: empty image");
		if (!m_model && m_testbed_mode == ETestbedMode::Sdf && m_sdf_mesh) reset_network();  // as train() does
		if (!m_model) throw std::runtime_error("render: no network (train or load a snapshot first)");
		std::vector<float> out((size_t)width * height * 4);
		if (m_testbed_mode == ETestbedMode::Nerf) {
			if ((int)m_render_mode > (int)ERenderMode::Distortion)
				throw std::runtime_error("render: ERenderMode AO, Shade, Normals, Positions, Depth and Distortion are implemented");
			require_nerf_trainer("render");
			if (!m_renderer) check(ngp_nerf_renderer_create(&m_renderer), "ngp_nerf_renderer_create");
			check(ngp_nerf_renderer_set_mode(m_renderer, (int)m_render_mode), "ngp_nerf_renderer_set_mode");
			// depth_scale = 1 / m_nerf.training.dataset.scale (render_nerf, testbed_nerf.cu:2822)
			check(ngp_nerf_renderer_set_depth_scale(m_renderer, 1.0f / m_dataset_scale), "ngp_nerf_renderer_set_depth_scale");
			const ngp_nerf_image cam = render_camera(width, height);
			const float* g = nullptr;
			const uint8_t* bf = nullptr;
			const float* mean = nullptr;
			check(ngp_nerf_trainer_buffers_read(m_nerf_trainer, &g, &bf, &mean), "ngp_nerf_trainer_buffers_read");
			{  // the environment map's EMA parameters behind the frame (inference_view, testbed_nerf.cu:2315-2319); none: unbound
				const float* env = nullptr;
				uint32_t ew = 0, eh = 0;
				check(ngp_nerf_trainer_envmap_device(m_nerf_trainer, NGP_ENVMAP_INFERENCE_PARAMS, &env, &ew, &eh), "ngp_nerf_trainer_envmap_device");
				check(ngp_nerf_renderer_set_envmap(m_renderer, env, ew, eh), "ngp_nerf_renderer_set_envmap");
			}
			{  // the trainer's lens distortion map under render_with_lens_distortion (testbed_nerf.cu:2229-2344), which
			   // ERenderMode::Distortion shows; none, or the switch off: unbound
				const float* dm = nullptr;
				uint32_t dw = 0, dh = 0;
				if (m_render_with_lens_distortion)
					check(ngp_nerf_trainer_distortion_map_device(m_nerf_trainer, NGP_DISTORTION_INFERENCE_PARAMS, &dm, &dw, &dh),
					      "ngp_nerf_trainer_distortion_map_device");
				check(ngp_nerf_renderer_set_distortion_map(m_renderer, dm, dw, dh), "ngp_nerf_renderer_set_distortion_map");
			}
			float* dev = m_render_buf.get<float>(out.size());
			ngp_nerf_config cfg = m_nerf_cfg;
			check(ngp_nerf_render(m_renderer, m_model, &cfg, nullptr, &cam, bf, spp, m_render_sample_index, m_render_min_transmittance,
			                      m_background_color, 1, dev),
			      "ngp_nerf_render");
			check(ngp_memcpy(out.data(), dev, out.size() * 4, 2), "ngp_memcpy");
		} else if (m_testbed_mode == ETestbedMode::Image) {
			const size_t n = (size_t)width * height;
			std::vector<float> pos(n * 2);
			for (uint32_t y = 0; y < height; ++y)
				for (uint32_t x = 0; x < width; ++x) {
					pos[((size_t)y * width + x) * 2] = (x + 0.5f) / width;
					pos[((size_t)y * width + x) * 2 + 1] = (y + 0.5f) / height;
				}
			float* dpos = m_render_buf.get<float>(n * 2);
			check(ngp_memcpy(dpos, pos.data(), n * 8, 1), "ngp_memcpy");
			uint16_t* dout = m_render_out.get<uint16_t>(n * 16);
			check(ngp_inference(m_model, nullptr, (uint32_t)n, dpos, 2, dout, 16, NGP_LAYOUT_AOS, 1), "ngp_inference");
			std::vector<uint16_t> h(n * 16);
			check(ngp_memcpy(h.data(), dout, n * 32, 2), "ngp_memcpy");
			for (size_t i = 0; i < n; ++i) {
				for (int c = 0; c < 3; ++c) {
					float v = half_to_float(h[i * 16 + c]);
					// the network regresses sRGB targets unless linear_colors (testbed_image.cu:167-212)
					out[i * 4 + c] = m_image_cfg.linear_colors ? v : srgb_to_linear(v);
				}
				out[i * 4 + 3] = 1.0f;
			}
		} else if (m_testbed_mode == ETestbedMode::Sdf) {
			// Testbed::render_frame_main's SDF branch (testbed.cu:4590-4640): the network's distance with the inference
			// (EMA) parameters, or the mesh's own signed distance when render_ground_truth
			if (m_render_ground_truth && !m_sdf_mesh) throw std::runtime_error("render: render_ground_truth needs a loaded mesh");
			if (!m_sdf_renderer) check(ngp_sdf_renderer_create(&m_sdf_renderer), "ngp_sdf_renderer_create");
			const ngp_sdf_render_config cfg = sdf_render_config();
			const ngp_nerf_image cam = render_camera(width, height);
			float* dev = m_render_buf.get<float>(out.size());
			check(ngp_sdf_render(m_sdf_renderer, m_render_ground_truth ? nullptr : m_model, m_render_ground_truth ? m_sdf_mesh : nullptr, &cfg,
			                     nullptr, &cam, (int)m_render_mode, spp, m_render_sample_index, m_background_color, 1, dev, nullptr),
			      "ngp_sdf_render");
			check(ngp_memcpy(out.data(), dev, out.size() * 4, 2), "ngp_memcpy");
		} else {
			throw std::runtime_error("render: volume rendering is out of scope (SURVEY §2)");
		}
		if (!linear)
			for (size_t i = 0; i < out.size(); i += 4)
				for (int c = 0; c < 3; ++c) out[i + c] = linear_to_srgb(out[i + c]);
		return out;
	}

	// Testbed::calculate_iou (testbed_sdf.cu:1329-1364) without the octree (force_use_octree is accepted and ignored):
	// batches of 128^3 uniform positions in the aabb from m_rng (generate_training_samples_sdf's uniform_only branch:
	// generate_random_uniform then scale_to_aabb), the mesh's and the network's distance at each, the sign counters
	// accumulated on the device. blocking = false returns the ratio of the counters before this call's samples.
	double calculate_iou(uint32_t n_samples, float scale_existing_results_factor, bool blocking, bool /*force_use_octree*/) {
		if (m_testbed_mode != ETestbedMode::Sdf || !m_sdf_mesh) throw std::runtime_error("calculate_iou: no SDF mesh loaded");
		if (!m_model) reset_network();
		uint32_t host[8] = {0, 0, 0, 0, 0, 0, 0, 0};
		const bool fresh = m_iou_counters.p == nullptr;
		uint32_t* counters = m_iou_counters.get<uint32_t>(8);
		if (fresh) check(ngp_memcpy(counters, host, sizeof host, 1), "ngp_memcpy");
		if (!blocking) check(ngp_memcpy(host, counters, sizeof host, 2), "ngp_memcpy");
		float lo[3], hi[3];
		for (int d = 0; d < 3; ++d) {
			lo[d] = m_sdf_aabb_min[d] - m_sdf_render_cfg.zero_offset;
			hi[d] = m_sdf_aabb_max[d] + m_sdf_render_cfg.zero_offset;
		}
		bool scaled = false;
		std::vector<float> pos, dist;
		std::vector<uint16_t> half;
		do {
			const uint32_t n = std::min(128u * 128u * 128u, n_samples);
			n_samples -= n;
			const uint32_t n_pad = (n + 255u) / 256u * 256u;
			pos.assign((size_t)n_pad * 3, 0.5f);
			for (size_t i = 0; i < (size_t)n; ++i)
				for (int d = 0; d < 3; ++d) pos[i * 3 + d] = lo[d] + pcg32_next_float(m_rng) * (hi[d] - lo[d]);
			float* dpos = m_iou_pos.get<float>((size_t)n_pad * 3);
			float* dref = m_iou_ref.get<float>(n_pad);
			float* dmodel = m_iou_model.get<float>(n_pad);
			uint16_t* dout = m_render_out.get<uint16_t>((size_t)n_pad * 16);
			check(ngp_memcpy(dpos, pos.data(), pos.size() * 4, 1), "ngp_memcpy");
			if (n) {
				check(ngp_sdf_signed_distance(m_sdf_mesh, nullptr, n, dpos, dref), "ngp_sdf_signed_distance");
				// m_network->inference (:1350): SoA, so the distance is the first n_pad halves; widened to fp32 on the host
				check(ngp_inference(m_model, nullptr, n_pad, dpos, 3, dout, n_pad, NGP_LAYOUT_SOA, 1), "ngp_inference");
				half.resize(n);
				dist.resize(n);
				check(ngp_memcpy(half.data(), dout, (size_t)n * 2, 2), "ngp_memcpy");
				for (uint32_t i = 0; i < n; ++i) dist[i] = half_to_float(half[i]);
				check(ngp_memcpy(dmodel, dist.data(), (size_t)n * 4, 1), "ngp_memcpy");
			}
			check(ngp_sdf_iou_accumulate(nullptr, n, dref, dmodel, scaled ? 1.0f : scale_existing_results_factor, counters),
			      "ngp_sdf_iou_accumulate");
			scaled = true;
		} while (n_samples > 0);
		if (blocking) {
			check(ngp_stream_synchronize(nullptr), "ngp_stream_synchronize");
			check(ngp_memcpy(host, counters, sizeof host, 2), "ngp_memcpy");
		}
		return (double)host[4] / (double)host[5];
	}
	// ---- mesh extraction (Testbed::marching_cubes, testbed.h:472; python_api.cu:101-125) -----------------------------
	struct Mesh {
		std::vector<float> V, N, C;  // [n x 3] each; N normalised
		std::vector<int32_t> F;      // [m x 3], counter-clockwise seen from outside
	};
	// The model sampled on res3d points over the box (null: the model's own), marching cubes at thresh (SDF: 0, as
	// testbed_sdf.cu:1146 sets it), vertex normals and colours, with the inference (EMA) parameters as render() uses.
	Mesh compute_marching_cubes_mesh(const uint32_t* res3d, const float* aabb_min, const float* aabb_max, float thresh) {
		if (m_testbed_mode != ETestbedMode::Nerf && m_testbed_mode != ETestbedMode::Sdf)
			throw std::runtime_error("compute_marching_cubes_mesh: only NeRF and SDF models have a mesh");
		if (!m_model || !m_trainer) throw std::runtime_error("compute_marching_cubes_mesh: no network (train or load a snapshot first)");
		const bool nerf = m_testbed_mode == ETestbedMode::Nerf;
		if ((aabb_min == nullptr) != (aabb_max == nullptr)) throw std::runtime_error("compute_marching_cubes_mesh: half a box");
		if (!aabb_min) {
			aabb_min = nerf ? m_nerf_cfg.aabb_min : m_sdf_aabb_min;
			aabb_max = nerf ? m_nerf_cfg.aabb_max : m_sdf_aabb_max;
		}
		if (!nerf) thresh = 0.f;
		uint64_t n = 1;
		for (int d = 0; d < 3; ++d) {
			if (res3d[d] < 2) throw std::runtime_error("compute_marching_cubes_mesh: every resolution must be at least 2");
			n *= res3d[d];
			if (n >= (1ull << 32)) throw std::runtime_error("compute_marching_cubes_mesh: grids of 2^32 points or more are not supported");
		}
		float* density = m_mc_density.get<float>(n);
		check(ngp_density_on_grid(m_model, nullptr, nerf ? NGP_MC_NERF : NGP_MC_SDF, res3d, aabb_min, aabb_max, nullptr,
		                          nerf ? m_nerf_cfg.aabb_min : nullptr, nerf ? m_nerf_cfg.aabb_max : nullptr,
		                          nerf ? m_nerf_cfg.density_activation : 0u, 1u << 20, 1, density),
		      "ngp_density_on_grid");
		ngp_mesh* mesh = nullptr;
		check(ngp_marching_cubes(nullptr, density, res3d, aabb_min, aabb_max, nullptr, thresh, &mesh), "ngp_marching_cubes");
		struct Guard { ngp_mesh* m; ~Guard() { ngp_mesh_destroy(m); } } guard{mesh};
		check(ngp_mesh_vertex_colors(mesh, m_model, nullptr, nerf ? NGP_MC_NERF : NGP_MC_SDF, nerf ? m_nerf_cfg.aabb_min : nullptr,
		                             nerf ? m_nerf_cfg.aabb_max : nullptr, nerf ? m_nerf_cfg.rgb_activation : 0u, 1),
		      "ngp_mesh_vertex_colors");
		uint32_t nv = 0, nt = 0;
		check(ngp_mesh_counts(mesh, &nv, &nt), "ngp_mesh_counts");
		Mesh out;
		out.V.resize((size_t)nv * 3); out.N.resize((size_t)nv * 3); out.C.resize((size_t)nv * 3); out.F.resize((size_t)nt * 3);
		check(ngp_mesh_read(mesh, nullptr, out.V.data(), out.N.data(), out.C.data(), out.F.data()), "ngp_mesh_read");
		for (size_t i = 0; i < nv; ++i) {  // python_api.cu:119-122
			float* v = &out.N[i * 3];
			const float len = std::sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
			if (len > 0.f) for (int d = 0; d < 3; ++d) v[d] /= len;
		}
		return out;
	}
	// Testbed::compute_and_save_marching_cubes_mesh: a NeRF's vertices go back to the dataset's units through its scale
	// and offset (save_mesh's nerf_scale / nerf_offset, marching_cubes.cu:895, 912). The UV unwrap is not built.
	void compute_and_save_marching_cubes_mesh(const std::string& path, const uint32_t* res3d, const float* aabb_min, const float* aabb_max,
	                                          float thresh, bool unwrap_it) {
		if (unwrap_it) throw std::runtime_error("compute_and_save_marching_cubes_mesh: generate_uvs_for_obj_file is not supported (no UV unwrap)");
		const Mesh m = compute_marching_cubes_mesh(res3d, aabb_min, aabb_max, thresh);
		const bool nerf = m_testbed_mode == ETestbedMode::Nerf;
		const float zero[3] = {0.f, 0.f, 0.f};
		check(ngp_mesh_save(path.c_str(), (uint32_t)(m.V.size() / 3), m.V.data(), m.N.data(), m.C.data(), (uint32_t)(m.F.size() / 3),
		                    m.F.data(), nerf ? m_dataset_scale : 1.0f, nerf ? m_dataset_offset : zero),
		      "ngp_mesh_save");
	}

	// the SDF render configuration in use: Testbed::Sdf's knobs with the aabb, floor, sun and up of the Testbed
	ngp_sdf_render_config sdf_render_config() const {
		ngp_sdf_render_config cfg = m_sdf_render_cfg;
		std::memcpy(cfg.aabb_min, m_sdf_aabb_min, sizeof(cfg.aabb_min));
		std::memcpy(cfg.aabb_max, m_sdf_aabb_max, sizeof(cfg.aabb_max));
		cfg.floor_enable = m_floor_enable ? 1 : 0;
		cfg.snap_to_pixel_centers = m_snap_to_pixel_centers ? 1 : 0;
		std::memcpy(cfg.sun_dir, m_sun_dir, sizeof(cfg.sun_dir));
		std::memcpy(cfg.up_dir, m_up_dir, sizeof(cfg.up_dir));
		return cfg;
	}
	const float* sdf_aabb_min() const { return m_sdf_aabb_min; }
	const float* sdf_aabb_max() const { return m_sdf_aabb_max; }

	// NeRF training knobs (Testbed::Nerf::Training, testbed.h:716-785) reach a live trainer here
	ngp_nerf_config& nerf_config() { return m_nerf_cfg; }
	void push_nerf_config() {
		if (m_nerf_trainer) check(ngp_nerf_trainer_set_config(m_nerf_trainer, &m_nerf_cfg), "ngp_nerf_trainer_set_config");
	}
	// ---- camera pose refinement (Testbed::Nerf::Training, python_api.cu:618-653) -----------------------------
	ngp_nerf_camera_training& camera_training() { return m_cam_training; }
	void push_camera_training() {
		if (m_nerf_trainer) check(ngp_nerf_trainer_set_camera_training(m_nerf_trainer, &m_cam_training), "ngp_nerf_trainer_set_camera_training");
	}
	// ---- error-driven sampling (sample_focal_plane_proportional_to_error / sample_image_proportional_to_error,
	// python_api.cu:624-625): kept here until there is a trainer, pushed to a live one
	bool sample_focal_plane_by_error() const { return m_sample_focal_plane_by_error; }
	bool sample_image_by_error() const { return m_sample_image_by_error; }
	void set_error_sampling(bool focal_plane, bool image) {
		const bool was_f = m_sample_focal_plane_by_error, was_i = m_sample_image_by_error;
		m_sample_focal_plane_by_error = focal_plane;
		m_sample_image_by_error = image;
		try {
			check_error_sampling_vs_extrinsics();
			check_image_sampling_vs_exposure();
			check_error_sampling_vs_distortion();
			push_error_sampling();
		} catch (...) {
			m_sample_focal_plane_by_error = was_f;
			m_sample_image_by_error = was_i;
			throw;
		}
	}
	void push_error_sampling() {
		if (m_nerf_trainer)
			check(ngp_nerf_trainer_set_error_sampling(m_nerf_trainer, m_sample_focal_plane_by_error, m_sample_image_by_error),
			      "ngp_nerf_trainer_set_error_sampling");
	}
	// ---- depth supervision (nerf.training.depth_supervision_lambda / depth_loss_type, python_api.cu:616, 635; the depth
	// part of set_image, :657): kept here until there is a trainer, pushed to a live one. The depth images live in the
	// dataset (NerfDataset::set_training_image, nerf_loader.cu:943-960), so they outlast reset_network.
	float depth_supervision_lambda() const { return m_depth_lambda; }
	uint32_t depth_loss_type() const { return m_depth_loss_type; }
	void set_depth_supervision(float lambda, uint32_t loss_type) {
		if (!(lambda >= 0.f) || std::isinf(lambda)) throw std::runtime_error("depth_supervision_lambda: a finite value >= 0");
		if (loss_type > 6) throw std::runtime_error("depth_loss_type: unknown loss");
		m_depth_lambda = lambda;
		m_depth_loss_type = loss_type;
		push_depth_supervision();
	}
	void push_depth_supervision() {
		if (m_nerf_trainer)
			check(ngp_nerf_trainer_set_depth_supervision(m_nerf_trainer, m_depth_lambda, m_depth_loss_type),
			      "ngp_nerf_trainer_set_depth_supervision");
	}
	// ---- per-image exposure (nerf.training.optimize_exposure / exposure_l2_reg, python_api.cu:620, 634): kept here until
	// there is a trainer, pushed to a live one; the exposures themselves belong to the trainer (reset_network zeroes them)
	bool optimize_exposure() const { return m_optimize_exposure; }
	float exposure_l2_reg() const { return m_exposure_l2_reg; }
	void set_exposure_training(bool optimize, float l2_reg) {
		if (!(l2_reg >= 0.f) || std::isinf(l2_reg)) throw std::runtime_error("exposure_l2_reg: a finite value >= 0");
		const bool was = m_optimize_exposure;
		const float was_reg = m_exposure_l2_reg;
		m_optimize_exposure = optimize;
		m_exposure_l2_reg = l2_reg;
		try {
			check_image_sampling_vs_exposure();
			push_exposure_training();
		} catch (...) {
			m_optimize_exposure = was;
			m_exposure_l2_reg = was_reg;
			throw;
		}
	}
	void push_exposure_training() {
		if (m_nerf_trainer)
			check(ngp_nerf_trainer_set_exposure_training(m_nerf_trainer, m_optimize_exposure ? 1 : 0, m_exposure_l2_reg),
			      "ngp_nerf_trainer_set_exposure_training");
	}
	// ---- lens distortion map (nerf.training.optimize_distortion, python_api.cu:618-653; m_distortion, testbed.cu:4066-4076):
	// the switch is kept here until there is a trainer and pushed to a live one with the config's "distortion_map"
	// section (its optimizer, falling back to the main one, and its resolution); the map itself belongs to the trainer,
	// which creates it, zero, when the switch first goes on (reset_network starts over)
	bool optimize_distortion() const { return m_optimize_distortion; }
	void set_optimize_distortion(bool on) {
		const bool was = m_optimize_distortion;
		m_optimize_distortion = on;
		try {
			check_error_sampling_vs_distortion();
			push_distortion_training();
		} catch (...) {
			m_optimize_distortion = was;
			throw;
		}
	}
	void push_distortion_training() {
		if (!m_nerf_trainer) return;
		uint32_t w = 32, h = 32;
		std::string opt;
		if (m_network_config.contains("distortion_map")) {
			const Json& d = m_network_config["distortion_map"];
			if (d.contains("resolution")) {
				const Json& r = d["resolution"];
				if (r.type == Json::Array && r.arr.size() == 2) { w = (uint32_t)r.arr[0].num; h = (uint32_t)r.arr[1].num; }
				else if (r.type == Json::Number) w = h = (uint32_t)r.num;
				else throw std::runtime_error("distortion_map: resolution is [width, height]");
			}
			if (d.contains("optimizer")) opt = d["optimizer"].dump();
		}
		// no section, or none with an optimizer: the main optimizer (testbed.cu:4068)
		if (opt.empty() && m_network_config.contains("optimizer")) opt = m_network_config["optimizer"].dump();
		check(ngp_nerf_trainer_set_distortion_training(m_nerf_trainer, opt.empty() ? nullptr : opt.c_str(), w, h),
		      "ngp_nerf_trainer_set_distortion_training");
		check(ngp_nerf_trainer_set_optimize_distortion(m_nerf_trainer, m_optimize_distortion ? 1 : 0), "ngp_nerf_trainer_set_optimize_distortion");
	}
	// the trainer's map on the host: [height x width x 2] offsets of dir.xy; empty without a map
	std::vector<float> distortion_map(uint32_t* width, uint32_t* height) {
		*width = *height = 0;
		if (!m_nerf_trainer) return {};
		check(ngp_nerf_trainer_distortion_map(m_nerf_trainer, NGP_DISTORTION_PARAMS, nullptr, 0, width, height), "ngp_nerf_trainer_distortion_map");
		std::vector<float> out((size_t)*width * *height * 2);
		if (!out.empty())
			check(ngp_nerf_trainer_distortion_map(m_nerf_trainer, NGP_DISTORTION_PARAMS, out.data(), out.size(), width, height),
			      "ngp_nerf_trainer_distortion_map");
		return out;
	}
	// cam_exposure[i].variable(): zeros before there is a trainer, and for a frame out of range
	void get_camera_exposure(int frame_idx, float out[3]) const {
		out[0] = out[1] = out[2] = 0.f;
		if (frame_idx < 0 || (size_t)frame_idx >= m_nerf_images.size() || !m_nerf_trainer) return;
		check(ngp_nerf_trainer_camera_exposure(m_nerf_trainer, (uint32_t)frame_idx, out), "ngp_nerf_trainer_camera_exposure");
	}
	// dtype 0 uint16, 1 float32; pixels null: zeros (or, with a negative scale, no depth)
	void set_image_depth(uint32_t frame_idx, const void* pixels, int dtype, float depth_scale) {
		if (!m_nerf_dataset) throw std::runtime_error("set_image: no NeRF training data loaded");
		if (frame_idx >= m_nerf_images.size()) throw std::runtime_error("set_image: no such training view");
		check(ngp_nerf_dataset_set_depth(m_nerf_dataset, frame_idx, pixels, dtype, depth_scale), "ngp_nerf_dataset_set_depth");
	}
	bool nerf_is_hdr() const { return m_nerf_is_hdr; }
	// Engine extension: a training view's colours replaced by a float32 RGBA image [height][width][4] (linear,
	// premultiplied; stored as Float) at the view's resolution
	void set_image_pixels(uint32_t frame_idx, const float* rgba, uint32_t width, uint32_t height) {
		if (!m_nerf_dataset) throw std::runtime_error("set_image_pixels: no NeRF training data loaded");
		if (frame_idx >= m_nerf_images.size()) throw std::runtime_error("set_image_pixels: no such training view");
		if (width != m_nerf_images[frame_idx].width || height != m_nerf_images[frame_idx].height)
			throw std::runtime_error("set_image_pixels: the image has the wrong resolution (resizing a training view is not supported)");
		check(ngp_nerf_dataset_set_image(m_nerf_dataset, frame_idx, rgba, NGP_IMAGE_FLOAT, width, height), "ngp_nerf_dataset_set_image");
	}
	// a training view's texels as stored, and their NGP_IMAGE_* type
	std::vector<uint8_t> image_pixels(uint32_t frame_idx, uint32_t* type) const {
		if (!m_nerf_dataset || frame_idx >= m_nerf_images.size()) throw std::runtime_error("image: no such training view");
		check(ngp_nerf_dataset_image(m_nerf_dataset, frame_idx, nullptr, 0, type), "ngp_nerf_dataset_image");
		const size_t texel = *type == NGP_IMAGE_FLOAT ? 16 : *type == NGP_IMAGE_HALF ? 8 : 4;
		std::vector<uint8_t> out((size_t)m_nerf_images[frame_idx].width * m_nerf_images[frame_idx].height * texel);
		check(ngp_nerf_dataset_image(m_nerf_dataset, frame_idx, out.data(), out.size(), type), "ngp_nerf_dataset_image");
		return out;
	}
	// the stored depth image of a training view (empty: none)
	std::vector<float> image_depth(uint32_t frame_idx) const {
		if (!m_nerf_dataset || frame_idx >= m_nerf_images.size()) throw std::runtime_error("depth: no such training view");
		std::vector<float> out((size_t)m_nerf_images[frame_idx].width * m_nerf_images[frame_idx].height);
		int has = 0;
		check(ngp_nerf_dataset_depth(m_nerf_dataset, frame_idx, out.data(), out.size(), &has), "ngp_nerf_dataset_depth");
		if (!has) out.clear();
		return out;
	}
	// ---- environment map (Testbed::m_envmap, Training::train_envmap; testbed.cu:4133-4147, python_api.cu:618-653) ----
	// The dataset's "envmap" image (nerf_loader.cu:516-528), or zeros of a resolution asked for with create_envmap
	// when the dataset brings none: the trainer's map after every reset_network. Without either, train_envmap does
	// nothing, as in the reference.
	void set_dataset_envmap(uint32_t width, uint32_t height, const float* rgba) {
		if (width == 0 || height == 0) throw std::runtime_error("envmap: empty resolution");
		m_envmap_res[0] = width;
		m_envmap_res[1] = height;
		if (rgba) m_envmap_init.assign(rgba, rgba + (size_t)width * height * 4);
		else m_envmap_init.clear();
		push_envmap();
	}
	void create_envmap(uint32_t width, uint32_t height) { set_dataset_envmap(width, height, nullptr); }
	bool train_envmap() const { return m_train_envmap; }
	void set_train_envmap(bool on) {
		const bool was = m_train_envmap;
		m_train_envmap = on;
		try {
			if (m_nerf_trainer) check(ngp_nerf_trainer_set_train_envmap(m_nerf_trainer, on ? 1 : 0), "ngp_nerf_trainer_set_train_envmap");
		} catch (...) {
			m_train_envmap = was;
			throw;
		}
	}
	// the map, its "envmap" config section (loss and optimizer, each falling back to the main one, testbed.cu:4135-4136)
	// and the switch, to a live trainer
	void push_envmap() {
		if (!m_nerf_trainer) return;
		if (m_envmap_res[0] == 0) {
			check(ngp_nerf_trainer_clear_envmap(m_nerf_trainer), "ngp_nerf_trainer_clear_envmap");
		} else {
			check(ngp_nerf_trainer_set_envmap(m_nerf_trainer, m_envmap_res[0], m_envmap_res[1], m_envmap_init.empty() ? nullptr : m_envmap_init.data()),
			      "ngp_nerf_trainer_set_envmap");
			int loss = -1;
			std::string opt;
			if (m_network_config.contains("envmap")) {
				const Json& e = m_network_config["envmap"];
				if (e.contains("loss")) loss = loss_type_from_name(e["loss"].string_or("otype", "L2"));
				if (e.contains("optimizer")) opt = e["optimizer"].dump();
			}
			check(ngp_nerf_trainer_set_envmap_training(m_nerf_trainer, loss, opt.empty() ? nullptr : opt.c_str()),
			      "ngp_nerf_trainer_set_envmap_training");
		}
		check(ngp_nerf_trainer_set_train_envmap(m_nerf_trainer, m_train_envmap ? 1 : 0), "ngp_nerf_trainer_set_train_envmap");
	}
	static int loss_type_from_name(const std::string& name) {  // string_to_loss_type (common.cu), ELossType's order
		static const char* const names[] = {"L2", "L1", "Mape", "Smape", "Huber", "LogL1", "RelativeL2"};
		for (int k = 0; k < 7; ++k) {
			const std::string n = names[k];
			if (n.size() == name.size() && std::equal(n.begin(), n.end(), name.begin(), [](char a, char b) { return std::tolower(a) == std::tolower(b); }))
				return k;
		}
		throw std::runtime_error("envmap: unknown loss type '" + name + "'");
	}
	// the trainer's map on the host: [height x width x 4], the raw or the EMA (rendering) parameters; empty without a map
	std::vector<float> envmap(bool ema, uint32_t* width, uint32_t* height) {
		*width = *height = 0;
		if (!m_nerf_trainer) return {};
		const int which = ema ? NGP_ENVMAP_INFERENCE_PARAMS : NGP_ENVMAP_PARAMS;
		check(ngp_nerf_trainer_envmap(m_nerf_trainer, which, nullptr, 0, width, height), "ngp_nerf_trainer_envmap");
		std::vector<float> out((size_t)*width * *height * 4);
		if (!out.empty()) check(ngp_nerf_trainer_envmap(m_nerf_trainer, which, out.data(), out.size(), width, height), "ngp_nerf_trainer_envmap");
		return out;
	}
	// the trainer refuses the pair; refused here as well, so that it cannot build up before there is a trainer
	void check_error_sampling_vs_extrinsics() const {
		if (m_cam_training.optimize_extrinsics && (m_sample_focal_plane_by_error || m_sample_image_by_error))
			throw std::runtime_error("optimize_extrinsics cannot be combined with sample_focal_plane_proportional_to_error / "
			                         "sample_image_proportional_to_error: turn one of them off first");
	}
	void check_error_sampling_vs_distortion() const {
		if (m_optimize_distortion && (m_sample_focal_plane_by_error || m_sample_image_by_error))
			throw std::runtime_error("optimize_distortion cannot be combined with sample_focal_plane_proportional_to_error / "
			                         "sample_image_proportional_to_error: turn one of them off first");
	}
	void check_image_sampling_vs_exposure() const {
		if (m_optimize_exposure && m_sample_image_by_error)
			throw std::runtime_error("optimize_exposure cannot be combined with sample_image_proportional_to_error: turn one of "
			                         "them off first");
	}
	// Training::transforms[i].start: the trainer's refined transform, or the dataset's before there is a trainer
	void training_view_xform(uint32_t i, float out[12]) const {
		if (i >= m_nerf_images.size()) throw std::runtime_error("no such training view");
		if (m_nerf_trainer) check(ngp_nerf_trainer_camera_extrinsics(m_nerf_trainer, i, out), "ngp_nerf_trainer_camera_extrinsics");
		else std::memcpy(out, m_nerf_images[i].xform, 12 * sizeof(float));
	}
	// NerfDataset::nerf_matrix_to_ngp (nerf_loader.h:120-140, non-mitsuba branch) and its inverse ngp_matrix_to_nerf
	// (:142) with the dataset's scale and offset; m: [3 x 4] row-major, x: mat4x3 column-major
	void nerf_matrix_to_ngp(const float m[12], float x[12]) const {
		for (int c = 0; c < 4; ++c)
			for (int k = 0; k < 3; ++k) {
				float v = m[k * 4 + c];
				if (c == 1 || c == 2) v = -v;
				if (c == 3) v = v * m_dataset_scale + m_dataset_offset[k];
				x[c * 3 + (k + 2) % 3] = v;  // cycle axes xyz <- yzx
			}
	}
	void ngp_matrix_to_nerf(const float x[12], float m[12]) const {
		for (int c = 0; c < 4; ++c)
			for (int k = 0; k < 3; ++k) {
				float v = x[c * 3 + (k + 2) % 3];
				if (c == 1 || c == 2) v = -v;
				if (c == 3) v = (v - m_dataset_offset[k]) / m_dataset_scale;
				m[k * 4 + c] = v;
			}
	}
	// get_camera_extrinsics (testbed_nerf.cu:2973-2978): [3 x 4] row-major, NeRF convention
	void get_camera_extrinsics(int frame_idx, float m[12]) const {
		if (frame_idx < 0 || (size_t)frame_idx >= m_nerf_images.size()) {  // mat4x3(1.0f)
			for (int k = 0; k < 12; ++k) m[k] = k % 5 == 0 ? 1.f : 0.f;
			return;
		}
		float x[12];
		training_view_xform((uint32_t)frame_idx, x);
		ngp_matrix_to_nerf(x, m);
	}
	// set_camera_extrinsics (:2896-2919): m [3 x 4] row-major; out-of-range frames are ignored, as there
	void set_camera_extrinsics(int frame_idx, const float m[12], bool convert_to_ngp) {
		if (frame_idx < 0 || (size_t)frame_idx >= m_nerf_images.size()) return;
		require_nerf_trainer("set_camera_extrinsics");
		float x[12];
		if (convert_to_ngp) nerf_matrix_to_ngp(m, x);
		else
			for (int c = 0; c < 4; ++c)
				for (int k = 0; k < 3; ++k) x[c * 3 + k] = m[k * 4 + c];
		check(ngp_nerf_trainer_set_camera_extrinsics(m_nerf_trainer, (uint32_t)frame_idx, x), "ngp_nerf_trainer_set_camera_extrinsics");
	}
	void reset_camera_extrinsics() {
		if (m_nerf_trainer) check(ngp_nerf_trainer_reset_camera_extrinsics(m_nerf_trainer), "ngp_nerf_trainer_reset_camera_extrinsics");
	}
	// cam_pos_offset[i] / cam_rot_offset[i]
	void camera_optimizer_state(int frame_idx, ngp_adam_state* pos, ngp_adam_state* rot) {
		require_nerf_trainer("camera_optimizer_state");
		check(ngp_nerf_trainer_pose_optimizer_state(m_nerf_trainer, (uint32_t)frame_idx, pos, rot), "ngp_nerf_trainer_pose_optimizer_state");
	}
	ngp_image_config& image_config() { return m_image_cfg; }
	const std::vector<ngp_nerf_image>& nerf_images() const { return m_nerf_images; }
	float aabb_scale() const { return m_aabb_scale; }
	ngp_trainer* trainer() const { return m_trainer; }
	ngp_model* model() const { return m_model; }

	// public members with the reference's names (testbed.h)
	bool m_train = false;
	uint32_t m_training_batch_size = 1u << 18;
	uint32_t m_seed = 1337;
	float m_background_color[4] = {0.f, 0.f, 0.f, 1.f};
	ERenderMode m_render_mode = ERenderMode::Shade;
	float m_camera[12] = {1, 0, 0, 0, 1, 0, 0, 0, 1, 0.5f, 0.5f, -1.5f};  // mat4x3, column-major
	float m_relative_focal_length[2] = {1.0f, 1.0f};
	float m_screen_center[2] = {0.5f, 0.5f};
	uint32_t m_fov_axis = 1;
	float m_zoom = 1.0f;
	uint32_t m_render_sample_index = 0;
	float m_render_min_transmittance = 0.01f;   // Nerf::render_min_transmittance (testbed.h)
	bool m_render_with_lens_distortion = false;  // Nerf::render_with_lens_distortion
	bool m_sdf_generate_online = true;           // Sdf::Training::generate_sdf_data_online (testbed.h:842)
	float m_sdf_surface_offset_scale = 1.0f;     // Sdf::Training::surface_offset_scale
	float m_bounding_radius = 1.0f;
	uint32_t m_training_view = 0;
	bool m_render_ground_truth = false;          // testbed.h:564
	bool m_floor_enable = false;                 // testbed.h:916
	bool m_snap_to_pixel_centers = false;        // testbed.h:984 (the SDF render; NeRF renders follow the training config)
	float m_sun_dir[3], m_up_dir[3];             // testbed.h:601-602
	// Testbed::Sdf's render members and its BRDFParams (testbed.h:798-835); aabb, floor, sun and up are filled in by
	// sdf_render_config()
	ngp_sdf_render_config m_sdf_render_cfg{};

private:
	static constexpr float ZERO = 0.f;
	static ngp_rng host_pcg32(uint64_t seed) {  // tcnn::pcg32(initstate, initseq = 1)
		const uint64_t mult = 0x5851F42D4C957F2DULL;
		ngp_rng r;
		r.inc = (1ull << 1) | 1u;
		r.state = 0;
		r.state = r.state * mult + r.inc;
		r.state += seed;
		r.state = r.state * mult + r.inc;
		return r;
	}
	// tcnn::pcg32::next_float (pcg32.h): 23 random mantissa bits in [1, 2) minus 1
	static float pcg32_next_float(ngp_rng& r) {
		const uint64_t old = r.state;
		r.state = old * 0x5851F42D4C957F2DULL + r.inc;
		const uint32_t xs = (uint32_t)(((old >> 18u) ^ old) >> 27u), rot = (uint32_t)(old >> 59u);
		const uint32_t v = ((xs >> rot) | (xs << ((~rot + 1u) & 31))) >> 9 | 0x3f800000u;
		float f;
		std::memcpy(&f, &v, 4);
		return f - 1.0f;
	}
	// the view of render(): the Testbed's camera, relative focal length, zoom and screen centre at a resolution
	ngp_nerf_image render_camera(uint32_t width, uint32_t height) const {
		ngp_nerf_image cam{};
		cam.width = width;
		cam.height = height;
		const float res_axis = (float)(m_fov_axis == 0 ? width : height);
		cam.focal_length[0] = m_relative_focal_length[0] * res_axis * m_zoom;
		cam.focal_length[1] = m_relative_focal_length[1] * res_axis * m_zoom;
		cam.principal_point[0] = 1.0f - m_screen_center[0];
		cam.principal_point[1] = 1.0f - m_screen_center[1];
		std::memcpy(cam.xform, m_camera, sizeof(m_camera));
		cam.lens_mode = m_render_with_lens_distortion ? m_lens_mode : 0;
		std::memcpy(cam.lens_params, m_lens_params, sizeof(m_lens_params));
		return cam;
	}
	void require_nerf_trainer(const char* what) {
		if (m_testbed_mode != ETestbedMode::Nerf) throw std::runtime_error(std::string(what) + ": not a NeRF testbed");
		if (!m_nerf_trainer) {
			if (!m_nerf_dataset) throw std::runtime_error(std::string(what) + ": no NeRF training data loaded");
			reset_network();
		}
	}
	void free_network() {
		if (m_nerf_trainer) ngp_nerf_trainer_destroy(m_nerf_trainer);
		if (m_trainer) ngp_trainer_destroy(m_trainer);
		if (m_model) ngp_model_destroy(m_model);
		m_nerf_trainer = nullptr;
		m_trainer = nullptr;
		m_model = nullptr;
	}
	void free_data() {
		if (m_renderer) ngp_nerf_renderer_destroy(m_renderer);
		if (m_sdf_renderer) ngp_sdf_renderer_destroy(m_sdf_renderer);
		m_sdf_renderer = nullptr;
		if (m_nerf_dataset) ngp_nerf_dataset_destroy(m_nerf_dataset);
		if (m_image) ngp_image_destroy(m_image);
		if (m_sdf_mesh) ngp_sdf_mesh_destroy(m_sdf_mesh);
		m_renderer = nullptr;
		m_nerf_dataset = nullptr;
		m_image = nullptr;
		m_sdf_mesh = nullptr;
		m_nerf_images.clear();
		m_envmap_init.clear();
		m_envmap_res[0] = m_envmap_res[1] = 0;
		m_training_data_available = false;
	}

	ETestbedMode m_testbed_mode = ETestbedMode::None;
	bool m_mode_set = false;
	Json m_network_config;
	bool m_training_data_available = false;
	uint32_t m_training_step = 0;
	float m_loss_scalar = 0.f;
	ngp_rng m_rng{};
	ngp_model* m_model = nullptr;
	ngp_trainer* m_trainer = nullptr;
	// NeRF
	ngp_nerf_dataset* m_nerf_dataset = nullptr;
	bool m_nerf_is_hdr = false;
	ngp_nerf_trainer* m_nerf_trainer = nullptr;
	ngp_nerf_camera_training m_cam_training{0, 16, 1e-4f, 1e-3f};  // testbed.h:716-785 defaults
	bool m_sample_focal_plane_by_error = false, m_sample_image_by_error = false;  // testbed.h:733-734
	bool m_train_envmap = false;            // Training::train_envmap
	bool m_optimize_exposure = false;       // Training::optimize_exposure
	bool m_optimize_distortion = false;     // Training::optimize_distortion
	float m_exposure_l2_reg = 0.f;          // Training::exposure_l2_reg
	float m_depth_lambda = 0.f;             // Training::depth_supervision_lambda (testbed.h:719)
	uint32_t m_depth_loss_type = 1;         // Training::depth_loss_type: L1 (testbed.h:745)
	uint32_t m_envmap_res[2] = {0, 0};      // NerfDataset::envmap_resolution, or create_envmap's; 0: no map
	std::vector<float> m_envmap_init;       // NerfDataset::envmap_data; empty: zeros
	ngp_nerf_renderer* m_renderer = nullptr;
	ngp_nerf_config m_nerf_cfg{};
	std::vector<ngp_nerf_image> m_nerf_images;
	float m_aabb_scale = 1.f;
	float m_dataset_scale = 1.f;
	float m_dataset_offset[3] = {0.5f, 0.5f, 0.5f};
	uint32_t m_lens_mode = 0;
	float m_lens_params[4] = {0, 0, 0, 0};
	// image
	ngp_image* m_image = nullptr;
	ngp_image_config m_image_cfg{};
	uint32_t m_image_res[2] = {0, 0};
	// SDF
	ngp_sdf_mesh* m_sdf_mesh = nullptr;
	ngp_sdf_renderer* m_sdf_renderer = nullptr;
	DeviceBuffer m_iou_counters, m_iou_pos, m_iou_ref, m_iou_model;  // the training batch buffers stay as they are
	float m_sdf_aabb_min[3] = {0, 0, 0}, m_sdf_aabb_max[3] = {1, 1, 1};
	DeviceBuffer m_sdf_pos, m_sdf_dist, m_sdf_pos_s, m_sdf_dist_s;
	DeviceBuffer m_loss_dev, m_render_buf, m_render_out, m_mc_density;
};

}  // namespace ngp_host
