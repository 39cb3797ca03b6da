// python_api.cpp — the `pyngp` pybind11 module (src/python_api.cpp of the reference, :258-698): the Testbed
// host of testbed_host.hpp with the reference's Python names and argument meaning, over the engine's C-ABI.
// Built by g++ against libngp_engine.so (no HIP headers); scripts use it as the reference's do
// (`import pyngp as ngp`, scripts/run.py:25): ngp.Testbed(), load_training_data, shall_train, frame / train,
// training_step, loss, save_snapshot / load_snapshot, render.
//
// Headless: no window, GUI, DLSS or VR members (SURVEY §2 out of scope). Image files are decoded by the
// package's Python readers (nerf_data.load_nerf: PIL for JPEG/PNG; exr.read_exr), the way the reference
// hands decoding to stb_image / tinyexr; everything after decoding runs in C++ and on the GPU.
#include <pybind11/eval.h>
#include <pybind11/numpy.h>
#include <pybind11/pybind11.h>
#include <pybind11/stl.h>

#include "testbed_host.hpp"

namespace py = pybind11;
using namespace ngp_host;

namespace {

enum class ELossType : int { L2, L1, Mape, Smape, Huber, LogL1, RelativeL2 };  // common.h (python_api.cu:306-315)
enum class ENerfActivation : int { None, ReLU, Logistic, Exponential };       // nerf.h (python_api.cu:323-328)
enum class ERandomMode : int { Random = 0, Stratified = 3 };                   // common.h:124-130 (engine's subset)

std::string g_module_file;

// instant-ngp_amd/ as the Python package `instant_ngp_amd` (its directory name is not an identifier); this
// module lives in instant-ngp_amd/lib/
py::object package() {
	py::object modules = py::module_::import("sys").attr("modules");
	if (modules.contains("instant_ngp_amd")) return modules["instant_ngp_amd"];
	py::dict scope;
	scope["module_file"] = g_module_file;
	py::exec(R"(
import importlib.util, os, sys
pkg_dir = os.path.dirname(os.path.dirname(os.path.abspath(module_file)))
spec = importlib.util.spec_from_file_location("instant_ngp_amd", os.path.join(pkg_dir, "__init__.py"),
                                              submodule_search_locations=[pkg_dir])
mod = importlib.util.module_from_spec(spec)
sys.modules["instant_ngp_amd"] = mod
spec.loader.exec_module(mod)
)", scope);
	return modules["instant_ngp_amd"];
}

// Testbed::load_training_data (testbed.cu:139-165): the mode follows the scene (mode_from_scene)
void load_training_data(Testbed& tb, const std::string& path) {
	const ETestbedMode mode = mode_from_scene(path);
	switch (mode) {
	case ETestbedMode::Nerf: {
		py::object d = package().attr("nerf_data").attr("load_nerf")(path);
		py::list images = d.attr("images"), pixels = d.attr("rgba8");
		py::object ctypes = py::module_::import("ctypes");
		std::vector<ngp_nerf_image> meta(py::len(images));
		// an EXR frame's pixels come as float16 (Half), every other frame's as RGBA8
		std::vector<py::array> keep;
		std::vector<const void*> ptrs;
		std::vector<uint32_t> types;
		for (size_t i = 0; i < meta.size(); ++i) {
			py::object im = images[i];
			if (ctypes.attr("sizeof")(im).cast<size_t>() != sizeof(ngp_nerf_image))
				throw std::runtime_error("load_training_data: NerfImage layout differs from ngp_nerf_image");
			std::memcpy(&meta[i], (const void*)ctypes.attr("addressof")(im).cast<uintptr_t>(), sizeof(ngp_nerf_image));
			py::array px = py::array::ensure(pixels[i]);
			const bool half = px && px.dtype().kind() == 'f' && px.dtype().itemsize() == 2;
			if (half) keep.emplace_back(py::array::ensure(px, py::array::c_style));
			else keep.emplace_back(py::array_t<uint8_t, py::array::c_style | py::array::forcecast>(pixels[i]));
			types.push_back(half ? NGP_IMAGE_HALF : NGP_IMAGE_BYTE);
			if (keep.back().ndim() != 3 || (uint32_t)keep.back().shape(0) != meta[i].height ||
			    (uint32_t)keep.back().shape(1) != meta[i].width || keep.back().shape(2) != 4)
				throw std::runtime_error("load_training_data: image buffer shape does not match its metadata");
			ptrs.push_back(keep.back().data());
		}
		const float aabb_scale = d.attr("aabb_scale").cast<float>();
		const float scale = py::hasattr(d, "scale") ? d.attr("scale").cast<float>() : 1.0f;
		float offset[3] = {0.5f, 0.5f, 0.5f};
		if (py::hasattr(d, "offset")) {
			const std::vector<float> o = d.attr("offset").cast<std::vector<float>>();
			if (o.size() == 3) std::copy(o.begin(), o.end(), offset);
		}
		// the transforms file's "envmap" image: the initial environment map and its resolution (nerf_loader.cu:516-528)
		py::array_t<float, py::array::c_style | py::array::forcecast> envmap;
		const bool has_envmap = py::hasattr(d, "envmap") && !d.attr("envmap").is_none();
		if (has_envmap) {
			envmap = py::array_t<float, py::array::c_style | py::array::forcecast>(d.attr("envmap"));
			if (envmap.ndim() != 3 || envmap.shape(2) != 4) throw std::runtime_error("load_training_data: the envmap is an [H, W, 4] RGBA image");
		}
		// the frames' depth images (uint16) and the scale the dataset multiplies them by (nerf_loader.cu:609-621, 711)
		std::vector<py::array_t<uint16_t, py::array::c_style | py::array::forcecast>> depth(meta.size());
		std::vector<float> depth_scale(meta.size(), -1.0f);
		std::vector<bool> has_depth(meta.size(), false);
		if (py::hasattr(d, "depth") && py::hasattr(d, "depth_scale")) {
			py::list dl = d.attr("depth"), sl = d.attr("depth_scale");
			for (size_t i = 0; i < meta.size() && i < py::len(dl) && i < py::len(sl); ++i) {
				if (py::object(dl[i]).is_none()) continue;
				depth[i] = py::array_t<uint16_t, py::array::c_style | py::array::forcecast>(dl[i]);
				if (depth[i].ndim() != 2 || (uint32_t)depth[i].shape(0) != meta[i].height || (uint32_t)depth[i].shape(1) != meta[i].width)
					throw std::runtime_error("load_training_data: depth image shape does not match its image");
				depth_scale[i] = py::object(sl[i]).cast<float>();
				has_depth[i] = true;
			}
		}
		py::gil_scoped_release nogil;
		tb.load_nerf(meta, ptrs, aabb_scale, scale, offset, &types);
		if (has_envmap) tb.set_dataset_envmap((uint32_t)envmap.shape(1), (uint32_t)envmap.shape(0), envmap.data());
		for (size_t i = 0; i < meta.size(); ++i)
			if (has_depth[i]) tb.set_image_depth((uint32_t)i, depth[i].data(), 0, depth_scale[i]);
		break;
	}
	case ETestbedMode::Image: {
		py::object arr;
		if (iends_with(path, ".exr")) arr = package().attr("exr").attr("read_exr")(path);
		else if (iends_with(path, ".npy")) arr = py::module_::import("numpy").attr("load")(path);
		else throw std::runtime_error("load_training_data: images are read from .exr or .npy [H, W, 4] float files");
		py::array_t<float, py::array::c_style | py::array::forcecast> a(arr);
		if (a.ndim() != 3 || a.shape(2) != 4) throw std::runtime_error("load_training_data: expected an [H, W, 4] RGBA image");
		tb.load_image((uint32_t)a.shape(1), (uint32_t)a.shape(0), a.data());
		break;
	}
	case ETestbedMode::Sdf: {
		py::gil_scoped_release nogil;
		tb.load_mesh_file(path);
		break;
	}
	case ETestbedMode::Volume: throw std::runtime_error("the volume primitive is out of scope (SURVEY §2)");
	default: throw std::runtime_error("Unknown scene format for path '" + path + "'.");
	}
}

// Testbed::load_file (testbed.cu:316-375): snapshots, network configs, else training data
void load_file(Testbed& tb, const std::string& path) {
	if (iends_with(path, ".ingp") || iends_with(path, ".msgpack")) {
		tb.load_snapshot(path);
		return;
	}
	if (iends_with(path, ".json") && !is_directory(path)) {
		const Json j = Json::parse(read_text(path));
		if (j.contains("encoding") || j.contains("network") || j.contains("parent")) {
			tb.reload_network_from_file(path);
			return;
		}
	}
	const bool had_data = tb.training_data_available();
	load_training_data(tb, path);
	if (!had_data) tb.m_train = true;  // testbed.cu:363-371
}

// the (min, max) pair of a box argument; None: the model's own box
struct BoxArg {
	bool given = false;
	float lo[3], hi[3];
	explicit BoxArg(const py::object& aabb) {
		if (aabb.is_none()) return;
		const auto pair = aabb.cast<std::pair<std::vector<float>, std::vector<float>>>();
		if (pair.first.size() != 3 || pair.second.size() != 3) throw std::runtime_error("aabb: a (min, max) pair of 3 values each");
		std::copy(pair.first.begin(), pair.first.end(), lo);
		std::copy(pair.second.begin(), pair.second.end(), hi);
		given = true;
	}
};
std::vector<uint32_t> resolution_arg(const std::vector<int>& res) {
	if (res.size() != 3) throw std::runtime_error("resolution: 3 values");
	for (int r : res)
		if (r < 0) throw std::runtime_error("resolution: negative value");
	return std::vector<uint32_t>(res.begin(), res.end());
}

// views of the Testbed's nested members (Testbed::Nerf, ::Sdf, ::Image and their ::Training)
struct NerfView { Testbed* t; };
struct NerfTrainingView { Testbed* t; };
struct NerfDatasetView { Testbed* t; };
struct SdfView { Testbed* t; };
struct SdfTrainingView { Testbed* t; };
struct BrdfView { Testbed* t; };  // Testbed::Sdf::brdf (BRDFParams, sdf.h:62-72), a view into the Testbed's render config
struct ImageView { Testbed* t; };
struct ImageTrainingView { Testbed* t; };

// a Testbed::Nerf::Training knob: written into the trainer's live configuration (ngp_nerf_trainer_set_config)
template <typename V, typename T>
void nerf_knob(py::class_<V>& c, const char* name, T ngp_nerf_config::*field) {
	c.def_property(name, [field](const V& v) { return v.t->nerf_config().*field; },
	               [field](V& v, T x) {
		               v.t->nerf_config().*field = x;
		               v.t->push_nerf_config();
	               });
}

// a float member of the SDF render configuration (Testbed::Sdf, BRDFParams)
template <typename V>
void sdf_knob(py::class_<V>& c, const char* name, float ngp_sdf_render_config::*field) {
	c.def_property(name, [field](const V& v) { return v.t->m_sdf_render_cfg.*field; },
	               [field](V& v, float x) { v.t->m_sdf_render_cfg.*field = x; });
}
template <typename V>
void sdf_vec3(py::class_<V>& c, const char* name, float (ngp_sdf_render_config::*field)[3]) {
	c.def_property(name, [field](const V& v) { const float* p = v.t->m_sdf_render_cfg.*field; return std::vector<float>(p, p + 3); },
	               [field, name](V& v, const std::vector<float>& x) {
		               if (x.size() != 3) throw std::runtime_error(std::string(name) + ": 3 values");
		               std::copy(x.begin(), x.end(), v.t->m_sdf_render_cfg.*field);
	               });
}
// a vec3 member of the Testbed (m_sun_dir, m_up_dir)
void testbed_vec3(py::class_<Testbed>& c, const char* name, float (Testbed::*field)[3]) {
	c.def_property(name, [field](const Testbed& t) { const float* p = t.*field; return std::vector<float>(p, p + 3); },
	               [field, name](Testbed& t, const std::vector<float>& x) {
		               if (x.size() != 3) throw std::runtime_error(std::string(name) + ": 3 values");
		               std::copy(x.begin(), x.end(), t.*field);
	               });
}

}  // namespace

PYBIND11_MODULE(pyngp, m) {
	m.doc() = "instant-ngp Testbed on MI355X (gfx950): the reference's pyngp surface over the engine's C-ABI";
	g_module_file = m.attr("__file__").cast<std::string>();

	py::enum_<ETestbedMode>(m, "TestbedMode")
		.value("Nerf", ETestbedMode::Nerf).value("Sdf", ETestbedMode::Sdf).value("Image", ETestbedMode::Image)
		.value("Volume", ETestbedMode::Volume).value("None", ETestbedMode::None).export_values();
	m.def("mode_from_scene", &mode_from_scene);
	m.def("mode_from_string", &mode_from_string);
	py::enum_<ERenderMode>(m, "RenderMode")
		.value("AO", ERenderMode::AO).value("Shade", ERenderMode::Shade).value("Normals", ERenderMode::Normals)
		.value("Positions", ERenderMode::Positions).value("Depth", ERenderMode::Depth).value("Distortion", ERenderMode::Distortion)
		.value("Cost", ERenderMode::Cost).value("Slice", ERenderMode::Slice).export_values();
	py::enum_<ELossType>(m, "LossType")
		.value("L2", ELossType::L2).value("L1", ELossType::L1).value("Mape", ELossType::Mape).value("Smape", ELossType::Smape)
		.value("Huber", ELossType::Huber).value("SmoothL1", ELossType::Huber).value("LogL1", ELossType::LogL1)
		.value("RelativeL2", ELossType::RelativeL2);
	py::enum_<ENerfActivation>(m, "NerfActivation")
		.value("None", ENerfActivation::None).value("ReLU", ENerfActivation::ReLU).value("Logistic", ENerfActivation::Logistic)
		.value("Exponential", ENerfActivation::Exponential);
	py::enum_<ERandomMode>(m, "RandomMode").value("Random", ERandomMode::Random).value("Stratified", ERandomMode::Stratified);

	py::class_<Testbed> testbed(m, "Testbed");
	testbed
		.def(py::init<ETestbedMode>(), py::arg("mode") = ETestbedMode::None)
		.def(py::init([](ETestbedMode mode, const std::string& data_path, const std::string& network_config_path) {
			     auto t = std::make_unique<Testbed>(mode);
			     if (!data_path.empty()) load_training_data(*t, data_path);
			     if (!network_config_path.empty()) t->reload_network_from_file(network_config_path);
			     return t;
		     }),
		     py::arg("mode"), py::arg("data_path"), py::arg("network_config_path"))
		.def_property_readonly("mode", &Testbed::mode)
		.def("load_training_data", &load_training_data, "Load training data from a given path.")
		.def("clear_training_data", &Testbed::clear_training_data, "Clears training data to free up GPU memory.")
		.def("frame", &Testbed::frame, py::call_guard<py::gil_scoped_release>(),
		     "Process a single frame (headless: one training step when shall_train).")
		.def("train", &Testbed::train, py::call_guard<py::gil_scoped_release>(), py::arg("batch_size"),
		     "Perform a single training step with a specified batch size.")
		.def("reset", &Testbed::reset_network, py::arg("reset_density_grid") = true, "Reset training.")
		.def("reload_network_from_file", &Testbed::reload_network_from_file, py::arg("path") = "",
		     "Reload the network from a config file.")
		.def("reload_network_from_json",
		     [](Testbed& t, py::object json, const std::string&) {
			     t.reload_network_from_json(py::module_::import("json").attr("dumps")(json).cast<std::string>());
		     },
		     py::arg("json"), py::arg("config_base_path") = "", "Reload the network from a json object.")
		.def("n_params", &Testbed::n_params, "Number of trainable parameters")
		.def("n_encoding_params", &Testbed::n_encoding_params, "Number of trainable parameters in the encoding")
		.def_property_readonly("grid_interpolation", &Testbed::grid_interpolation,
		                       "The grid encoding's interpolation, from the network config: \"Linear\" or \"Smoothstep\"")
		.def("save_snapshot", &Testbed::save_snapshot, py::arg("path"), py::arg("include_optimizer_state") = false,
		     py::arg("compress") = true, py::call_guard<py::gil_scoped_release>(),
		     "Save a snapshot of the currently trained model (.ingp: gzip'd msgpack).")
		.def("load_snapshot", &Testbed::load_snapshot, py::arg("path"), py::call_guard<py::gil_scoped_release>(),
		     "Load a previously saved snapshot")
		.def("load_file", &load_file, py::arg("path"),
		     "Load a file and automatically determine how to handle it: a snapshot, a network config or training data.")
		.def("render",
		     [](Testbed& t, uint32_t width, uint32_t height, uint32_t spp, bool linear, float, float, float, float) {
			     std::vector<float> img;
			     {
				     py::gil_scoped_release nogil;
				     img = t.render(width, height, spp, linear);
			     }
			     py::array_t<float> a({(py::ssize_t)height, (py::ssize_t)width, (py::ssize_t)4});
			     std::memcpy(a.mutable_data(), img.data(), img.size() * sizeof(float));
			     return a;
		     },
		     py::arg("width") = 1920, py::arg("height") = 1080, py::arg("spp") = 1, py::arg("linear") = true,
		     py::arg("start_t") = -1.f, py::arg("end_t") = -1.f, py::arg("fps") = 30.f, py::arg("shutter_fraction") = 1.0f,
		     "Renders an image at the requested resolution. Does not require a window.")
		.def_readwrite("shall_train", &Testbed::m_train)
		.def_readwrite("training_batch_size", &Testbed::m_training_batch_size)
		.def_readwrite("render_mode", &Testbed::m_render_mode)
		.def_readwrite("render_groundtruth", &Testbed::m_render_ground_truth)
		.def_readwrite("render_ground_truth", &Testbed::m_render_ground_truth)
		.def_readwrite("floor_enable", &Testbed::m_floor_enable)
		.def_readwrite("snap_to_pixel_centers", &Testbed::m_snap_to_pixel_centers)
		.def("calculate_iou", &Testbed::calculate_iou, py::call_guard<py::gil_scoped_release>(),
		     "Calculate the intersection over union error value", py::arg("n_samples") = 128 * 1024 * 1024,
		     py::arg("scale_existing_results_factor") = 0.0f, py::arg("blocking") = true, py::arg("force_use_octree") = true)
		.def("compute_marching_cubes_mesh",
		     [](Testbed& t, const std::vector<int>& resolution, py::object aabb, float thresh) {
			     const std::vector<uint32_t> res = resolution_arg(resolution);
			     const BoxArg box(aabb);
			     Testbed::Mesh mesh;
			     {
				     py::gil_scoped_release nogil;
				     mesh = t.compute_marching_cubes_mesh(res.data(), box.given ? box.lo : nullptr, box.given ? box.hi : nullptr, thresh);
			     }
			     const py::ssize_t nv = (py::ssize_t)(mesh.V.size() / 3), nt = (py::ssize_t)(mesh.F.size() / 3);
			     py::array_t<float> V({nv, (py::ssize_t)3}), N({nv, (py::ssize_t)3}), C({nv, (py::ssize_t)3});
			     py::array_t<int32_t> F({nt, (py::ssize_t)3});
			     if (nv) {
				     std::memcpy(V.mutable_data(), mesh.V.data(), mesh.V.size() * sizeof(float));
				     std::memcpy(N.mutable_data(), mesh.N.data(), mesh.N.size() * sizeof(float));
				     std::memcpy(C.mutable_data(), mesh.C.data(), mesh.C.size() * sizeof(float));
			     }
			     if (nt) std::memcpy(F.mutable_data(), mesh.F.data(), mesh.F.size() * sizeof(int32_t));
			     py::dict d;
			     d["V"] = V; d["N"] = N; d["C"] = C; d["F"] = F;
			     return d;
		     },
		     py::arg("resolution") = std::vector<int>{128, 128, 128}, py::arg("aabb") = py::none(), py::arg("thresh") = 2.5f,
		     "Compute a marching cubes mesh from the current SDF or NeRF model. Returns a python dict with numpy arrays V "
		     "(vertices), N (vertex normals), C (vertex colors), and F (triangular faces).")
		.def("compute_and_save_marching_cubes_mesh",
		     [](Testbed& t, const std::string& filename, const std::vector<int>& resolution, py::object aabb, float thresh,
		        bool generate_uvs_for_obj_file) {
			     const std::vector<uint32_t> res = resolution_arg(resolution);
			     const BoxArg box(aabb);
			     py::gil_scoped_release nogil;
			     t.compute_and_save_marching_cubes_mesh(filename, res.data(), box.given ? box.lo : nullptr, box.given ? box.hi : nullptr, thresh,
			                                            generate_uvs_for_obj_file);
		     },
		     py::arg("filename"), py::arg("resolution") = std::vector<int>{128, 128, 128}, py::arg("aabb") = py::none(),
		     py::arg("thresh") = 2.5f, py::arg("generate_uvs_for_obj_file") = false,
		     "Compute a marching cubes mesh from the current SDF or NeRF model and save it to an .obj or .ply file. "
		     "UV generation is not supported.")
		.def_property_readonly("aabb", [](const Testbed& t) {  // m_aabb of an SDF testbed: (min, max)
			return py::make_tuple(std::vector<float>(t.sdf_aabb_min(), t.sdf_aabb_min() + 3),
			                      std::vector<float>(t.sdf_aabb_max(), t.sdf_aabb_max() + 3));
		})
		.def_readwrite("fov_axis", &Testbed::m_fov_axis)
		.def_readwrite("zoom", &Testbed::m_zoom)
		.def_property(
			"background_color", [](const Testbed& t) { return std::vector<float>(t.m_background_color, t.m_background_color + 4); },
			[](Testbed& t, const std::vector<float>& c) {
				if (c.size() != 4) throw std::runtime_error("background_color: 4 values (RGBA, linear)");
				std::copy(c.begin(), c.end(), t.m_background_color);
			})
		// m_camera: mat4x3 (columns = the camera's x, y, z axes and its position), as a [3 x 4] array
		.def_property(
			"camera_matrix",
			[](const Testbed& t) {
				py::array_t<float> a({3, 4});
				auto r = a.mutable_unchecked<2>();
				for (int c = 0; c < 4; ++c)
					for (int k = 0; k < 3; ++k) r(k, c) = t.m_camera[c * 3 + k];
				return a;
			},
			[](Testbed& t, py::array_t<float, py::array::c_style | py::array::forcecast> a) {
				if (a.ndim() != 2 || a.shape(0) != 3 || a.shape(1) != 4) throw std::runtime_error("camera_matrix: a [3 x 4] array");
				auto r = a.unchecked<2>();
				for (int c = 0; c < 4; ++c)
					for (int k = 0; k < 3; ++k) t.m_camera[c * 3 + k] = r(k, c);
			})
		.def("set_camera_to_training_view", &Testbed::set_camera_to_training_view, py::arg("view"))
		.def("first_training_view", [](Testbed& t) { t.set_camera_to_training_view(0); })
		.def("last_training_view", [](Testbed& t) { t.set_camera_to_training_view(t.n_training_views() - 1); })
		.def("previous_training_view",
		     [](Testbed& t) { t.set_camera_to_training_view(t.m_training_view == 0 ? t.n_training_views() - 1 : t.m_training_view - 1); })
		.def("next_training_view", [](Testbed& t) { t.set_camera_to_training_view((t.m_training_view + 1) % t.n_training_views()); })
		.def_property_readonly("loss", &Testbed::loss)
		.def_property_readonly("training_step", &Testbed::training_step)
		.def_readonly("bounding_radius", &Testbed::m_bounding_radius)
		.def_property_readonly("nerf", py::cpp_function([](Testbed& t) { return NerfView{&t}; }, py::keep_alive<0, 1>()))
		.def_property_readonly("sdf", py::cpp_function([](Testbed& t) { return SdfView{&t}; }, py::keep_alive<0, 1>()))
		.def_property_readonly("image", py::cpp_function([](Testbed& t) { return ImageView{&t}; }, py::keep_alive<0, 1>()));

	testbed_vec3(testbed, "sun_dir", &Testbed::m_sun_dir);
	testbed_vec3(testbed, "up_dir", &Testbed::m_up_dir);

	py::class_<NerfView> nerf(testbed, "Nerf");
	nerf.def_property_readonly("training", py::cpp_function([](NerfView& v) { return NerfTrainingView{v.t}; }, py::keep_alive<0, 1>()))
		.def_property("rgb_activation", [](NerfView& v) { return (ENerfActivation)v.t->nerf_config().rgb_activation; },
		              [](NerfView& v, ENerfActivation a) { v.t->nerf_config().rgb_activation = (uint32_t)a; v.t->push_nerf_config(); })
		.def_property("density_activation", [](NerfView& v) { return (ENerfActivation)v.t->nerf_config().density_activation; },
		              [](NerfView& v, ENerfActivation a) { v.t->nerf_config().density_activation = (uint32_t)a; v.t->push_nerf_config(); })
		.def_property("render_min_transmittance", [](NerfView& v) { return v.t->m_render_min_transmittance; },
		              [](NerfView& v, float x) { v.t->m_render_min_transmittance = x; })
		.def_property("rendering_min_transmittance", [](NerfView& v) { return v.t->m_render_min_transmittance; },
		              [](NerfView& v, float x) { v.t->m_render_min_transmittance = x; })
		.def_property("render_with_lens_distortion", [](NerfView& v) { return v.t->m_render_with_lens_distortion; },
		              [](NerfView& v, bool x) { v.t->m_render_with_lens_distortion = x; });
	nerf_knob(nerf, "cone_angle_constant", &ngp_nerf_config::cone_angle_constant);

	py::class_<NerfTrainingView> ntr(nerf, "Training");
	nerf_knob(ntr, "random_bg_color", &ngp_nerf_config::random_bg_color);
	nerf_knob(ntr, "linear_colors", &ngp_nerf_config::linear_colors);
	nerf_knob(ntr, "snap_to_pixel_centers", &ngp_nerf_config::snap_to_pixel_centers);
	nerf_knob(ntr, "near_distance", &ngp_nerf_config::near_distance);
	ntr.def_property("loss_type", [](NerfTrainingView& v) { return (ELossType)v.t->nerf_config().loss_type; },
	                 [](NerfTrainingView& v, ELossType l) { v.t->nerf_config().loss_type = (uint32_t)l; v.t->push_nerf_config(); })
		.def_property_readonly("n_images_for_training", [](NerfTrainingView& v) { return v.t->n_training_views(); })
		// camera pose refinement (python_api.cu:618-653)
		.def_property("optimize_extrinsics", [](NerfTrainingView& v) { return v.t->camera_training().optimize_extrinsics != 0; },
		              [](NerfTrainingView& v, bool x) {
			              const uint32_t was = v.t->camera_training().optimize_extrinsics;
			              v.t->camera_training().optimize_extrinsics = x ? 1u : 0u;
			              try {
				              v.t->check_error_sampling_vs_extrinsics();
				              v.t->push_camera_training();
			              } catch (...) { v.t->camera_training().optimize_extrinsics = was; throw; }
		              })
		// the environment map (python_api.cu:618-653): trains the dataset's "envmap" image, or the zero map of create_envmap
		.def_property("train_envmap", [](NerfTrainingView& v) { return v.t->train_envmap(); },
		              [](NerfTrainingView& v, bool x) { v.t->set_train_envmap(x); })
		.def("create_envmap", [](NerfTrainingView& v, uint32_t width, uint32_t height) { v.t->create_envmap(width, height); },
		     py::arg("width"), py::arg("height"),
		     "Engine extension: a zero environment map of this resolution (for a dataset without an \"envmap\" image).")
		.def("envmap", [](NerfTrainingView& v, bool ema) -> py::object {
			     uint32_t w = 0, h = 0;
			     const std::vector<float> a = v.t->envmap(ema, &w, &h);
			     if (a.empty()) return py::none();
			     py::array_t<float> out({(py::ssize_t)h, (py::ssize_t)w, (py::ssize_t)4});
			     std::memcpy(out.mutable_data(), a.data(), a.size() * sizeof(float));
			     return std::move(out);
		     }, py::arg("ema") = false,
		     "Engine extension: the environment map [H, W, 4] (the raw parameters, or the EMA parameters rendering reads); None without one.")
		// the lens distortion map (python_api.cu:618-653; testbed.cu:4066-4076)
		.def_property("optimize_distortion", [](NerfTrainingView& v) { return v.t->optimize_distortion(); },
		              [](NerfTrainingView& v, bool x) { v.t->set_optimize_distortion(x); })
		.def_property_readonly("distortion_map", [](NerfTrainingView& v) -> py::object {
			     uint32_t w = 0, h = 0;
			     const std::vector<float> a = v.t->distortion_map(&w, &h);
			     if (a.empty()) return py::none();
			     py::array_t<float> out({(py::ssize_t)h, (py::ssize_t)w, (py::ssize_t)2});
			     std::memcpy(out.mutable_data(), a.data(), a.size() * sizeof(float));
			     return std::move(out);
		     }, "Engine extension: the lens distortion map [H, W, 2], the offsets added to the rays' dir.xy; None without one.")
		// depth supervision (python_api.cu:616, 635, 657)
		.def_property("depth_supervision_lambda", [](NerfTrainingView& v) { return v.t->depth_supervision_lambda(); },
		              [](NerfTrainingView& v, float x) { v.t->set_depth_supervision(x, v.t->depth_loss_type()); })
		.def_property("depth_loss_type", [](NerfTrainingView& v) { return (ELossType)v.t->depth_loss_type(); },
		              [](NerfTrainingView& v, ELossType l) { v.t->set_depth_supervision(v.t->depth_supervision_lambda(), (uint32_t)l); })
		.def("set_image",
		     [](NerfTrainingView& v, int frame_idx, py::object img, py::object depth_img, float depth_scale) {
			     if (!img.is_none() && py::len(img) != 0)
				     throw std::runtime_error("set_image: replacing a training image's colours is not supported; pass img=None "
				                              "(or an empty array) to set only its depth image");
			     if (frame_idx < 0) throw std::runtime_error("set_image: no such training view");
			     if (depth_img.is_none()) { v.t->set_image_depth((uint32_t)frame_idx, nullptr, 0, depth_scale); return; }
			     py::array a = py::array::ensure(depth_img);
			     if (!a || a.ndim() != 2) throw std::runtime_error("set_image: depth_img is a [H, W] uint16 or float32 array");
			     const ngp_nerf_image& im = v.t->nerf_images().at((size_t)frame_idx);
			     if ((uint32_t)a.shape(0) != im.height || (uint32_t)a.shape(1) != im.width)
				     throw std::runtime_error("set_image: depth_img has the wrong resolution");
			     const float s = depth_scale;  // as given, as in the reference (the loader's is integer_depth_scale * dataset scale)
			     if (a.dtype().is(py::dtype::of<uint16_t>())) {
				     py::array_t<uint16_t, py::array::c_style | py::array::forcecast> u(a);
				     v.t->set_image_depth((uint32_t)frame_idx, u.data(), 0, s);
			     } else {
				     py::array_t<float, py::array::c_style | py::array::forcecast> f(a);
				     v.t->set_image_depth((uint32_t)frame_idx, f.data(), 1, s);
			     }
		     },
		     py::arg("frame_idx"), py::arg("img") = py::none(), py::arg("depth_img") = py::none(), py::arg("depth_scale") = 1.0f,
		     "The depth part of Testbed.nerf.training.set_image: depth_img [H, W] (uint16 or float32) times depth_scale "
		     "becomes the image's depth; None: zeros (with a negative depth_scale: no depth). img must be None.")
		.def("set_image_pixels",
		     [](NerfTrainingView& v, int frame_idx, py::array img) {
			     if (frame_idx < 0) throw std::runtime_error("set_image_pixels: no such training view");
			     if (!img.dtype().is(py::dtype::of<float>()) || img.ndim() != 3 || img.shape(2) != 4)
				     throw std::runtime_error("set_image_pixels: img is a float32 [H, W, 4] array");
			     py::array_t<float, py::array::c_style | py::array::forcecast> f(img);
			     v.t->set_image_pixels((uint32_t)frame_idx, f.data(), (uint32_t)f.shape(1), (uint32_t)f.shape(0));
		     },
		     py::arg("frame_idx"), py::arg("img"),
		     "Engine extension: replaces a training view's colours by a float32 [H, W, 4] image (linear, premultiplied RGBA, "
		     "stored as it is) of the view's resolution.")
		.def("image", [](NerfTrainingView& v, int frame_idx) -> py::object {
			     if (frame_idx < 0) throw std::runtime_error("image: no such training view");
			     uint32_t type = 0;
			     const std::vector<uint8_t> d = v.t->image_pixels((uint32_t)frame_idx, &type);
			     const ngp_nerf_image& im = v.t->nerf_images().at((size_t)frame_idx);
			     const char* dt = type == NGP_IMAGE_FLOAT ? "float32" : type == NGP_IMAGE_HALF ? "float16" : "uint8";
			     py::array out(py::dtype(dt), std::vector<py::ssize_t>{(py::ssize_t)im.height, (py::ssize_t)im.width, 4});
			     std::memcpy(out.mutable_data(), d.data(), d.size());
			     return std::move(out);
		     }, py::arg("frame_idx"), "Engine extension: a training view's texels as stored: [H, W, 4] uint8, float16 or float32.")
		.def("depth_image", [](NerfTrainingView& v, int frame_idx) -> py::object {
			     if (frame_idx < 0) throw std::runtime_error("depth_image: no such training view");
			     const std::vector<float> d = v.t->image_depth((uint32_t)frame_idx);
			     if (d.empty()) return py::none();
			     const ngp_nerf_image& im = v.t->nerf_images().at((size_t)frame_idx);
			     py::array_t<float> out({(py::ssize_t)im.height, (py::ssize_t)im.width});
			     std::memcpy(out.mutable_data(), d.data(), d.size() * sizeof(float));
			     return std::move(out);
		     }, py::arg("frame_idx"), "Engine extension: the stored depth image [H, W] of a training view; None without one.")
		// per-image exposure (python_api.cu:620, 634)
		.def_property("optimize_exposure", [](NerfTrainingView& v) { return v.t->optimize_exposure(); },
		              [](NerfTrainingView& v, bool x) { v.t->set_exposure_training(x, v.t->exposure_l2_reg()); })
		.def_property("exposure_l2_reg", [](NerfTrainingView& v) { return v.t->exposure_l2_reg(); },
		              [](NerfTrainingView& v, float x) { v.t->set_exposure_training(v.t->optimize_exposure(), x); })
		.def("get_camera_exposure",
		     [](NerfTrainingView& v, int frame_idx) {
			     py::array_t<float> a(3);
			     v.t->get_camera_exposure(frame_idx, a.mutable_data());
			     return a;
		     },
		     py::arg("frame_idx"), "Engine extension: a training image's learned log2 exposure per channel.")
		// error-driven sampling (python_api.cu:624-625); not reproducible from run to run while on
		.def_property("sample_focal_plane_proportional_to_error", [](NerfTrainingView& v) { return v.t->sample_focal_plane_by_error(); },
		              [](NerfTrainingView& v, bool x) { v.t->set_error_sampling(x, v.t->sample_image_by_error()); })
		.def_property("sample_image_proportional_to_error", [](NerfTrainingView& v) { return v.t->sample_image_by_error(); },
		              [](NerfTrainingView& v, bool x) { v.t->set_error_sampling(v.t->sample_focal_plane_by_error(), x); })
		.def_property("n_steps_between_cam_updates", [](NerfTrainingView& v) { return v.t->camera_training().n_steps_between_cam_updates; },
		              [](NerfTrainingView& v, uint32_t x) {
			              if (x == 0) throw std::runtime_error("n_steps_between_cam_updates: at least 1");
			              v.t->camera_training().n_steps_between_cam_updates = x;
			              v.t->push_camera_training();
		              })
		.def_property("extrinsic_l2_reg", [](NerfTrainingView& v) { return v.t->camera_training().extrinsic_l2_reg; },
		              [](NerfTrainingView& v, float x) { v.t->camera_training().extrinsic_l2_reg = x; v.t->push_camera_training(); })
		.def_property("extrinsic_learning_rate", [](NerfTrainingView& v) { return v.t->camera_training().extrinsic_learning_rate; },
		              [](NerfTrainingView& v, float x) { v.t->camera_training().extrinsic_learning_rate = x; v.t->push_camera_training(); })
		.def("get_camera_extrinsics",
		     [](NerfTrainingView& v, int frame_idx) {
			     float m[12];
			     v.t->get_camera_extrinsics(frame_idx, m);
			     py::array_t<float> a({3, 4});
			     std::memcpy(a.mutable_data(), m, sizeof m);
			     return a;
		     },
		     py::arg("frame_idx"), "The refined camera-to-world [3 x 4] of a training image, in the dataset's (NeRF) convention.")
		.def("set_camera_extrinsics",
		     [](NerfTrainingView& v, int frame_idx, py::array_t<float, py::array::c_style | py::array::forcecast> m, bool convert_to_ngp) {
			     if (m.ndim() != 2 || m.shape(0) < 3 || m.shape(1) != 4) throw std::runtime_error("set_camera_extrinsics: a [3 x 4] camera_to_world");
			     v.t->set_camera_extrinsics(frame_idx, m.data(), convert_to_ngp);
		     },
		     py::arg("frame_idx"), py::arg("camera_to_world"), py::arg("convert_to_ngp") = true,
		     "Replace a training image's camera-to-world [3 x 4] and reset its pose optimiser; convert_to_ngp: given in the NeRF convention.")
		.def("reset_camera_extrinsics", [](NerfTrainingView& v) { v.t->reset_camera_extrinsics(); })
		// engine extension: cam_pos_offset[frame_idx] / cam_rot_offset[frame_idx] as dicts with the snapshot's member names
		.def("camera_optimizer_state",
		     [](NerfTrainingView& v, int frame_idx) {
			     ngp_adam_state st[2];
			     v.t->camera_optimizer_state(frame_idx, &st[0], &st[1]);
			     py::list out;
			     for (const ngp_adam_state& a : st) {
				     py::dict d;
				     d["iter"] = a.iter;
				     d["first_moment"] = std::vector<float>(a.first_moment, a.first_moment + 3);
				     d["second_moment"] = std::vector<float>(a.second_moment, a.second_moment + 3);
				     d["variable"] = std::vector<float>(a.variable, a.variable + 3);
				     d["learning_rate"] = a.learning_rate;
				     d["epsilon"] = a.epsilon;
				     d["beta1"] = a.beta1;
				     d["beta2"] = a.beta2;
				     out.append(d);
			     }
			     return py::make_tuple(out[0], out[1]);
		     },
		     py::arg("frame_idx"))
		.def_property_readonly("dataset", py::cpp_function([](NerfTrainingView& v) { return NerfDatasetView{v.t}; }, py::keep_alive<0, 1>()));

	py::class_<NerfDatasetView>(m, "NerfDataset")
		.def_property_readonly("n_images", [](NerfDatasetView& v) { return v.t->n_training_views(); })
		.def_property_readonly("aabb_scale", [](NerfDatasetView& v) { return v.t->aabb_scale(); })
		.def_property_readonly("is_hdr", [](NerfDatasetView& v) { return v.t->nerf_is_hdr(); })
		.def_property_readonly("metadata", [](NerfDatasetView& v) {
			py::list out;
			for (const ngp_nerf_image& im : v.t->nerf_images()) {
				py::dict d;
				d["resolution"] = std::vector<uint32_t>{im.width, im.height};
				d["focal_length"] = std::vector<float>{im.focal_length[0], im.focal_length[1]};
				d["principal_point"] = std::vector<float>{im.principal_point[0], im.principal_point[1]};
				d["lens"] = py::make_tuple(im.lens_mode, std::vector<float>(im.lens_params, im.lens_params + 4));
				out.append(d);
			}
			return out;
		})
		.def_property_readonly("transforms", [](NerfDatasetView& v) {
			py::list out;
			for (const ngp_nerf_image& im : v.t->nerf_images()) {
				py::array_t<float> a({3, 4});
				auto r = a.mutable_unchecked<2>();
				for (int c = 0; c < 4; ++c)
					for (int k = 0; k < 3; ++k) r(k, c) = im.xform[c * 3 + k];
				out.append(a);
			}
			return out;
		});

	py::class_<SdfView> sdf(testbed, "Sdf");
	sdf.def_property_readonly("training", py::cpp_function([](SdfView& v) { return SdfTrainingView{v.t}; }, py::keep_alive<0, 1>()))
		.def_property("analytic_normals", [](SdfView& v) { return v.t->m_sdf_render_cfg.analytic_normals != 0; },
		              [](SdfView& v, bool x) { v.t->m_sdf_render_cfg.analytic_normals = x ? 1 : 0; })
		.def_property_readonly("brdf", py::cpp_function([](SdfView& v) { return BrdfView{v.t}; }, py::keep_alive<0, 1>()));
	sdf_knob(sdf, "zero_offset", &ngp_sdf_render_config::zero_offset);
	sdf_knob(sdf, "distance_scale", &ngp_sdf_render_config::distance_scale);
	sdf_knob(sdf, "fd_normals_epsilon", &ngp_sdf_render_config::fd_normals_epsilon);
	sdf_knob(sdf, "shadow_sharpness", &ngp_sdf_render_config::shadow_sharpness);
	sdf.def_property("max_iterations", [](SdfView& v) { return v.t->m_sdf_render_cfg.max_iterations; },
	                 [](SdfView& v, uint32_t x) { v.t->m_sdf_render_cfg.max_iterations = x; });  // engine extension: MARCH_ITER
	py::class_<BrdfView> brdf(m, "BRDFParams");  // python_api.cu:569-580
	sdf_knob(brdf, "metallic", &ngp_sdf_render_config::metallic);
	sdf_knob(brdf, "subsurface", &ngp_sdf_render_config::subsurface);
	sdf_knob(brdf, "specular", &ngp_sdf_render_config::specular);
	sdf_knob(brdf, "roughness", &ngp_sdf_render_config::roughness);
	sdf_knob(brdf, "sheen", &ngp_sdf_render_config::sheen);
	sdf_knob(brdf, "clearcoat", &ngp_sdf_render_config::clearcoat);
	sdf_knob(brdf, "clearcoat_gloss", &ngp_sdf_render_config::clearcoat_gloss);
	sdf_vec3(brdf, "basecolor", &ngp_sdf_render_config::basecolor);
	sdf_vec3(brdf, "ambientcolor", &ngp_sdf_render_config::ambientcolor);
	py::class_<SdfTrainingView>(sdf, "Training")
		.def_property("generate_sdf_data_online", [](SdfTrainingView& v) { return v.t->m_sdf_generate_online; },
		              [](SdfTrainingView& v, bool x) { v.t->m_sdf_generate_online = x; })
		.def_property("surface_offset_scale", [](SdfTrainingView& v) { return v.t->m_sdf_surface_offset_scale; },
		              [](SdfTrainingView& v, float x) { v.t->m_sdf_surface_offset_scale = x; });

	py::class_<ImageView> image(testbed, "Image");
	image.def_property_readonly("training", py::cpp_function([](ImageView& v) { return ImageTrainingView{v.t}; }, py::keep_alive<0, 1>()))
		.def_property("random_mode", [](ImageView& v) { return (ERandomMode)v.t->image_config().random_mode; },
		              [](ImageView& v, ERandomMode r) { v.t->image_config().random_mode = (uint32_t)r; });
	py::class_<ImageTrainingView>(image, "Training")
		.def_property("snap_to_pixel_centers", [](ImageTrainingView& v) { return (bool)v.t->image_config().snap_to_pixel_centers; },
		              [](ImageTrainingView& v, bool x) { v.t->image_config().snap_to_pixel_centers = x; })
		.def_property("linear_colors", [](ImageTrainingView& v) { return (bool)v.t->image_config().linear_colors; },
		              [](ImageTrainingView& v, bool x) { v.t->image_config().linear_colors = x; });

	// engine extension for tests and tools: the network config in use (JSON text) and the default of a mode
	m.def("default_network_config", [](ETestbedMode mode) { return default_network_config(mode); });
	testbed.def_property_readonly("network_config", &Testbed::network_config);
}
