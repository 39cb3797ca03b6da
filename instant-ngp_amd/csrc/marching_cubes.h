// marching_cubes.h — host parts of the mesh extraction (csrc/marching_cubes.hip): the generated case table, the
// grid resolution of a box and the .obj / .ply writer. No HIP calls in this file.
//
// Re-designs src/marching_cubes.cu of the reference: get_marching_cubes_res (:42-49), the tables gen_faces reads
// (:359-700) and save_mesh (:806-956). The reference embeds a 256 x 16 triangle table; this one is built at first use:
//
//  - corners 0-3 counter-clockwise on z = 0, 4-7 above them; edges 0-3 on the bottom, 4-7 on the top, 8-11 the verticals;
//  - for each sign pattern (bit c set: corner c inside, f > thresh) every cube face joins its crossing edges into
//    directed segments with the inside on the left seen from outside the cube. A face with four crossings cuts off each
//    inside corner on its own: the choice depends on the face's four signs only, so the two cells sharing it agree;
//  - the segments chain into closed loops; each loop is fan-triangulated from the apex that puts no fan diagonal
//    between two edges of one cube face (such an apex exists for every loop of every case), so that no triangle edge
//    lies in a face except the segments themselves;
//  - at most 5 triangles per case, 820 in all, wound counter-clockwise seen from the outside (f <= thresh) side.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

namespace ngp {
namespace mc {

constexpr int CORNER[8][3] = {{0, 0, 0}, {1, 0, 0}, {1, 1, 0}, {0, 1, 0}, {0, 0, 1}, {1, 0, 1}, {1, 1, 1}, {0, 1, 1}};
constexpr int EDGE[12][2] = {{0, 1}, {1, 2}, {2, 3}, {3, 0}, {4, 5}, {5, 6}, {6, 7}, {7, 4}, {0, 4}, {1, 5}, {2, 6}, {3, 7}};
// the corner cycle of each cube face, counter-clockwise seen from outside: x = 0, x = 1, y = 0, y = 1, z = 0, z = 1
constexpr int FACE[6][4] = {{0, 4, 7, 3}, {1, 2, 6, 5}, {0, 1, 5, 4}, {3, 7, 6, 2}, {0, 3, 2, 1}, {4, 5, 6, 7}};

struct Tables {
	int8_t tri[256][16];     // edge ids, three per triangle, -1 terminated
	uint16_t edge_mask[256]; // bit e set: edge e changes sign
	uint8_t n_tris[256];
};

inline int edge_between(int a, int b) {
	for (int e = 0; e < 12; ++e)
		if ((EDGE[e][0] == a && EDGE[e][1] == b) || (EDGE[e][0] == b && EDGE[e][1] == a)) return e;
	return -1;
}
inline bool edges_share_face(int a, int b) {
	for (int f = 0; f < 6; ++f) {
		int hit = 0;
		for (int k = 0; k < 4; ++k)
			for (int e : {a, b})
				for (int c = 0; c < 2; ++c) hit += FACE[f][k] == EDGE[e][c];
		if (hit == 4) return true;
	}
	return false;
}

inline Tables build_tables() {
	Tables T;
	std::memset(T.tri, -1, sizeof(T.tri));
	for (int mask = 0; mask < 256; ++mask) {
		uint16_t em = 0;
		for (int e = 0; e < 12; ++e)
			if (((mask >> EDGE[e][0]) & 1) != ((mask >> EDGE[e][1]) & 1)) em |= (uint16_t)(1u << e);
		T.edge_mask[mask] = em;
		int next[12];
		for (int e = 0; e < 12; ++e) next[e] = -1;
		for (int f = 0; f < 6; ++f) {
			const int* cyc = FACE[f];
			int in[4];
			for (int k = 0; k < 4; ++k) in[k] = (mask >> cyc[k]) & 1;
			for (int k = 0; k < 4; ++k) {
				if (in[k] || !in[(k + 1) % 4]) continue;  // walking the cycle, the inside run starts behind edge k ...
				int j = k;
				do j = (j + 1) % 4; while (!(in[j] && !in[(j + 1) % 4]));  // ... and ends at edge j
				next[edge_between(cyc[j], cyc[(j + 1) % 4])] = edge_between(cyc[k], cyc[(k + 1) % 4]);
			}
		}
		bool seen[12] = {};
		int n = 0;
		for (int s = 0; s < 12; ++s) {
			if (next[s] < 0 || seen[s]) continue;
			int loop[12], len = 0;
			for (int c = s; !seen[c]; c = next[c]) { loop[len++] = c; seen[c] = true; }
			int best_r = 0, best_bad = 1 << 30;
			for (int r = 0; r < len; ++r) {
				int bad = 0;
				for (int k = 2; k < len - 1; ++k) bad += edges_share_face(loop[r], loop[(r + k) % len]);
				if (bad < best_bad) { best_bad = bad; best_r = r; }
			}
			for (int k = 1; k < len - 1; ++k) {
				T.tri[mask][n++] = (int8_t)loop[best_r];
				T.tri[mask][n++] = (int8_t)loop[(best_r + k + 1) % len];
				T.tri[mask][n++] = (int8_t)loop[(best_r + k) % len];
			}
		}
		T.n_tris[mask] = (uint8_t)(n / 3);
	}
	return T;
}
inline const Tables& tables() {
	static const Tables T = build_tables();
	return T;
}

// get_marching_cubes_res (marching_cubes.cu:42-49): the longest side gets res_1d points, every axis rounded up to 16
inline bool grid_res(uint32_t res_1d, const float* aabb_min, const float* aabb_max, uint32_t* out) {
	float diag[3], longest = 0.f;
	for (int k = 0; k < 3; ++k) {
		diag[k] = aabb_max[k] - aabb_min[k];
		if (!(diag[k] > 0.f) || !std::isfinite(diag[k])) return false;
		longest = std::fmax(longest, diag[k]);
	}
	const float scale = (float)res_1d / longest;
	for (int k = 0; k < 3; ++k) {
		const float r = diag[k] * scale + 0.5f;
		if (!(r < 2147483648.f)) return false;
		out[k] = ((uint32_t)(int)r + 15u) / 16u * 16u;
	}
	return true;
}

inline bool ends_with_nocase(const std::string& s, const char* suffix) {
	const size_t n = std::strlen(suffix);
	if (s.size() < n) return false;
	for (size_t i = 0; i < n; ++i) {
		char c = s[s.size() - n + i];
		if (c >= 'A' && c <= 'Z') c = (char)(c - 'A' + 'a');
		if (c != suffix[i]) return false;
	}
	return true;
}
inline float clamp01(float v, float hi) { return v < 0.f ? 0.f : v > hi ? hi : v; }

// save_mesh's records (marching_cubes.cu:806-956) without the UV unwrap: vertices as (p - offset) / scale, non-finite
// positions and colours replaced by 0 and non-finite normals by +y (:826-830), normals normalised, colours clamped.
// A .ply extension gives ASCII PLY, anything else OBJ. Faces keep the winding of F (counter-clockwise from outside).
inline bool save_mesh(const char* path, uint32_t n_verts, const float* V, const float* N, const float* C, uint32_t n_tris,
                      const int32_t* F, float scale, const float* offset, std::string* err) {
	FILE* f = std::fopen(path, "wb");
	if (!f) {
		*err = std::string("ngp_mesh_save: cannot open '") + path + "' for writing";
		return false;
	}
	auto finite3 = [](const float* v) { return std::isfinite(v[0]) && std::isfinite(v[1]) && std::isfinite(v[2]); };
	std::vector<float> p(3 * (size_t)n_verts), n(3 * (size_t)n_verts), c(3 * (size_t)n_verts);
	for (size_t i = 0; i < n_verts; ++i) {
		const float zero[3] = {0.f, 0.f, 0.f}, up[3] = {0.f, 1.f, 0.f};
		const float* v = finite3(V + 3 * i) ? V + 3 * i : zero;
		const float* nn = N && finite3(N + 3 * i) ? N + 3 * i : up;
		const float* cc = C && finite3(C + 3 * i) ? C + 3 * i : zero;
		const float inv = 1.0f / std::sqrt(nn[0] * nn[0] + nn[1] * nn[1] + nn[2] * nn[2]);
		for (int k = 0; k < 3; ++k) {
			p[3 * i + k] = (v[k] - offset[k]) / scale;
			n[3 * i + k] = nn[k] * inv;
			c[3 * i + k] = cc[k];
		}
		if (!finite3(&n[3 * i])) std::memcpy(&n[3 * i], up, sizeof(up));  // a zero-length normal
	}
	if (ends_with_nocase(path, ".ply")) {
		std::fprintf(f,
		             "ply\nformat ascii 1.0\nelement vertex %u\nproperty float x\nproperty float y\nproperty float z\n"
		             "property float nx\nproperty float ny\nproperty float nz\nproperty uchar red\nproperty uchar green\n"
		             "property uchar blue\nelement face %u\nproperty list uchar int vertex_index\nend_header\n",
		             n_verts, n_tris);
		for (size_t i = 0; i < n_verts; ++i)
			std::fprintf(f, "%0.5f %0.5f %0.5f %0.3f %0.3f %0.3f %d %d %d\n", p[3 * i], p[3 * i + 1], p[3 * i + 2], n[3 * i], n[3 * i + 1],
			             n[3 * i + 2], (int)(unsigned char)clamp01(c[3 * i] * 255.f, 255.f), (int)(unsigned char)clamp01(c[3 * i + 1] * 255.f, 255.f),
			             (int)(unsigned char)clamp01(c[3 * i + 2] * 255.f, 255.f));
		for (size_t t = 0; t < n_tris; ++t) std::fprintf(f, "3 %d %d %d\n", F[3 * t], F[3 * t + 1], F[3 * t + 2]);
	} else {
		for (size_t i = 0; i < n_verts; ++i)
			std::fprintf(f, "v %0.5f %0.5f %0.5f %0.3f %0.3f %0.3f\n", p[3 * i], p[3 * i + 1], p[3 * i + 2], clamp01(c[3 * i], 1.f),
			             clamp01(c[3 * i + 1], 1.f), clamp01(c[3 * i + 2], 1.f));
		for (size_t i = 0; i < n_verts; ++i) std::fprintf(f, "vn %0.5f %0.5f %0.5f\n", n[3 * i], n[3 * i + 1], n[3 * i + 2]);
		for (size_t t = 0; t < n_tris; ++t) {
			const unsigned a = (unsigned)F[3 * t] + 1, b = (unsigned)F[3 * t + 1] + 1, cc = (unsigned)F[3 * t + 2] + 1;
			std::fprintf(f, "f %u//%u %u//%u %u//%u\n", a, a, b, b, cc, cc);
		}
	}
	const bool ok = std::ferror(f) == 0;
	if (std::fclose(f) != 0 || !ok) {
		*err = std::string("ngp_mesh_save: write to '") + path + "' failed";
		return false;
	}
	return true;
}

}  // namespace mc
}  // namespace ngp
