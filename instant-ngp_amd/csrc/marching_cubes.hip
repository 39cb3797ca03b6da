// marching_cubes.hip — mesh extraction from a trained NeRF or SDF: the model sampled on a regular grid, marching cubes
// over that grid, vertex normals and vertex colours, and their C-ABI (ngp_density_on_grid, ngp_marching_cubes,
// ngp_mesh_*). The host parts (generated case table, grid resolution, file writer) are in marching_cubes.h.
//
// Re-designs marching_cubes_gpu (src/marching_cubes.cu:263-311, 359-700, 776-804). The reference appends vertices and
// triangles through global atomic counters and sums normals with float atomics, so its output order changes from run
// to run. Here the order is a function of the grid alone:
//   count  every block of 8 x 8 x 4 grid points stages its densities plus a one-point halo in LDS and counts the
//          vertices (sign-changing edges leaving a point's low corner) and triangles (of the point's cube) it owns;
//   scan   one block turns the per-block counts into exclusive bases;
//   emit   vertices, then triangles: a point's slot is its block's base plus the wave prefix (64-lane ballots of the
//          count's bits, mbcnt) plus the totals of the block's earlier waves. Blocks that own nothing return at once.
// Each grid point keeps one u32: 29 bits of its first vertex's index and a 3-bit mask of the edges it owns (the
// reference keeps three ints per point); a point's vertices are consecutive in x, y, z order.
// Normals are gathered, not scattered: a vertex lies on one grid edge, only the four cubes around that edge touch it,
// and they are visited in a fixed order.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <memory>
#include <mutex>
#include <string>

#include "abi_guard.h"
#include "marching_cubes.h"
#include "nerf_device.h"
#include "profiler.h"

namespace ngp {
namespace mc {
namespace {

constexpr uint32_t TX = 8, TY = 8, TZ = 4, THREADS = TX * TY * TZ;  // one wave per z slice of the tile
constexpr uint32_t HX = TX + 1, HY = TY + 1, HZ = TZ + 1, HALO = HX * HY * HZ;
constexpr uint32_t SCAN_THREADS = 512;
constexpr uint32_t BASE_BITS = 29, BASE_MASK = (1u << BASE_BITS) - 1;

__device__ int8_t d_tri[256 * 16];
__device__ uint8_t d_ntris[256];

struct Grid {
	uint32_t rx, ry, rz;     // grid points per axis
	uint32_t nbx, nby, nbz;  // blocks per axis
	float scale[3], offset[3];
	float rot[9];            // row-major aabb_to_local, applied as its transpose
	uint32_t has_rot;
	float thresh;
};

// (owner dx | dy << 1 | dz << 2 | axis << 3) of cube edge e, 5 bits each
constexpr uint64_t pack_owner() {
	const uint64_t code[12] = {0, 9, 2, 8, 4, 13, 6, 12, 16, 17, 19, 18};
	uint64_t v = 0;
	for (int e = 0; e < 12; ++e) v |= code[e] << (5 * e);
	return v;
}
constexpr uint64_t EDGE_OWNER = pack_owner();

__device__ __forceinline__ uint32_t mbcnt(uint64_t m) {
	return __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
}
__device__ __forceinline__ size_t point_index(const Grid& g, uint32_t x, uint32_t y, uint32_t z) {
	return (size_t)x + (size_t)g.rx * ((size_t)y + (size_t)g.ry * z);
}

struct Cell {
	uint32_t x, y, z;
	bool valid;      // inside the grid
	uint32_t edges;  // bit a: the edge leaving this point along axis a changes sign (the vertices it owns)
	uint32_t n_tris; // triangles of the cube at this point (0 on the last layer of each axis)
	uint32_t cube;   // its case
	uint32_t l;      // index into the LDS tile
};

// Stage the block's densities plus halo (coordinates clamped to the grid; clamped values are never used) and
// classify this thread's grid point.
__device__ __forceinline__ Cell load_cell(const Grid& g, const float* __restrict__ density, float* tile) {
	const uint32_t b = blockIdx.x;
	const uint32_t bx = b % g.nbx, by = (b / g.nbx) % g.nby, bz = b / (g.nbx * g.nby);
	for (uint32_t i = threadIdx.x; i < HALO; i += THREADS) {
		const uint32_t hx = i % HX, hy = (i / HX) % HY, hz = i / (HX * HY);
		const uint32_t x = min(bx * TX + hx, g.rx - 1), y = min(by * TY + hy, g.ry - 1), z = min(bz * TZ + hz, g.rz - 1);
		tile[i] = density[point_index(g, x, y, z)];
	}
	__syncthreads();
	const uint32_t t = threadIdx.x, lx = t % TX, ly = (t / TX) % TY, lz = t / (TX * TY);
	Cell c;
	c.x = bx * TX + lx; c.y = by * TY + ly; c.z = bz * TZ + lz;
	c.valid = c.x < g.rx && c.y < g.ry && c.z < g.rz;
	c.l = lx + HX * (ly + HY * lz);
	c.edges = 0; c.n_tris = 0; c.cube = 0;
	if (!c.valid) return c;
	const bool in0 = tile[c.l] > g.thresh;
	const bool hx = c.x + 1 < g.rx, hy = c.y + 1 < g.ry, hz = c.z + 1 < g.rz;
	if (hx && in0 != (tile[c.l + 1] > g.thresh)) c.edges |= 1u;
	if (hy && in0 != (tile[c.l + HX] > g.thresh)) c.edges |= 2u;
	if (hz && in0 != (tile[c.l + HX * HY] > g.thresh)) c.edges |= 4u;
	if (hx && hy && hz) {
#pragma unroll
		for (uint32_t k = 0; k < 8; ++k) {
			const uint32_t dx = (k == 1 || k == 2 || k == 5 || k == 6), dy = (k == 2 || k == 3 || k == 6 || k == 7), dz = k >> 2;
			if (tile[c.l + dx + HX * (dy + HY * dz)] > g.thresh) c.cube |= 1u << k;
		}
		c.n_tris = d_ntris[c.cube];
	}
	return c;
}

// exclusive prefix of `count` (< 8) over the block's threads in thread order, and the block's total
__device__ __forceinline__ uint32_t block_prefix(uint32_t count, uint32_t* wave_tot, uint32_t* total) {
	const uint64_t b0 = __ballot(count & 1u), b1 = __ballot(count & 2u), b2 = __ballot(count & 4u);
	const uint32_t lane_prefix = mbcnt(b0) + 2u * mbcnt(b1) + 4u * mbcnt(b2);
	const uint32_t w = threadIdx.x / WAVE;
	if (threadIdx.x % WAVE == 0) wave_tot[w] = (uint32_t)__popcll(b0) + 2u * (uint32_t)__popcll(b1) + 4u * (uint32_t)__popcll(b2);
	__syncthreads();
	uint32_t base = 0, sum = 0;
	for (uint32_t k = 0; k < THREADS / WAVE; ++k) {
		if (k < w) base += wave_tot[k];
		sum += wave_tot[k];
	}
	__syncthreads();
	*total = sum;
	return base + lane_prefix;
}

__global__ void __launch_bounds__(THREADS) k_mc_count(Grid g, const float* __restrict__ density, uint2* __restrict__ counts) {
	__shared__ float tile[HALO];
	__shared__ uint32_t wave_tot[THREADS / WAVE];
	const Cell c = load_cell(g, density, tile);
	uint32_t nv, nt;
	block_prefix(__popc(c.edges), wave_tot, &nv);
	block_prefix(c.n_tris, wave_tot, &nt);
	if (threadIdx.x == 0) counts[blockIdx.x] = make_uint2(nv, nt);
}

// exclusive scan of the per-block counts in chunks of SCAN_THREADS with a running carry; bases[n] = the totals
__global__ void __launch_bounds__(SCAN_THREADS) k_mc_scan(uint32_t n, const uint2* __restrict__ counts, uint2* __restrict__ bases) {
	__shared__ uint2 wave_tot[SCAN_THREADS / WAVE];
	uint2 carry = make_uint2(0, 0);
	const uint32_t lane = threadIdx.x % WAVE, w = threadIdx.x / WAVE;
	for (uint32_t start = 0; start < n; start += SCAN_THREADS) {
		const uint32_t i = start + threadIdx.x;
		const uint2 own = i < n ? counts[i] : make_uint2(0, 0);
		uint2 v = own;
		for (uint32_t d = 1; d < WAVE; d <<= 1) {
			const uint32_t ax = __shfl_up(v.x, d, WAVE), ay = __shfl_up(v.y, d, WAVE);
			if (lane >= d) { v.x += ax; v.y += ay; }
		}
		if (lane == WAVE - 1) wave_tot[w] = v;
		__syncthreads();
		uint2 before = carry, all = carry;
		for (uint32_t k = 0; k < SCAN_THREADS / WAVE; ++k) {
			if (k < w) { before.x += wave_tot[k].x; before.y += wave_tot[k].y; }
			all.x += wave_tot[k].x; all.y += wave_tot[k].y;
		}
		if (i < n) bases[i] = make_uint2(before.x + v.x - own.x, before.y + v.y - own.y);
		carry = all;
		__syncthreads();
	}
	if (threadIdx.x == 0) bases[n] = carry;
}

__device__ __forceinline__ void store_vertex(const Grid& g, float* __restrict__ verts, uint32_t vi, float cx, float cy, float cz) {
	float p[3] = {cx * g.scale[0] + g.offset[0], cy * g.scale[1] + g.offset[1], cz * g.scale[2] + g.offset[2]};
	if (g.has_rot) {  // transpose(aabb_to_local) * p (gen_vertices, marching_cubes.cu:283)
		const float q[3] = {g.rot[0] * p[0] + g.rot[3] * p[1] + g.rot[6] * p[2], g.rot[1] * p[0] + g.rot[4] * p[1] + g.rot[7] * p[2],
		                    g.rot[2] * p[0] + g.rot[5] * p[1] + g.rot[8] * p[2]};
		p[0] = q[0]; p[1] = q[1]; p[2] = q[2];
	}
	verts[3 * (size_t)vi] = p[0]; verts[3 * (size_t)vi + 1] = p[1]; verts[3 * (size_t)vi + 2] = p[2];
}

__global__ void __launch_bounds__(THREADS) k_mc_emit_vertices(Grid g, const float* __restrict__ density, const uint2* __restrict__ counts,
                                                              const uint2* __restrict__ bases, uint32_t* __restrict__ vertmap,
                                                              float* __restrict__ verts) {
	if (counts[blockIdx.x].x == 0) return;
	__shared__ float tile[HALO];
	__shared__ uint32_t wave_tot[THREADS / WAVE];
	const Cell c = load_cell(g, density, tile);
	uint32_t total;
	uint32_t vi = bases[blockIdx.x].x + block_prefix(__popc(c.edges), wave_tot, &total);
	if (!c.edges) return;
	vertmap[point_index(g, c.x, c.y, c.z)] = vi | (c.edges << BASE_BITS);
	const float f0 = tile[c.l], x = (float)c.x, y = (float)c.y, z = (float)c.z;
	if (c.edges & 1u) store_vertex(g, verts, vi++, x + (g.thresh - f0) / (tile[c.l + 1] - f0), y, z);
	if (c.edges & 2u) store_vertex(g, verts, vi++, x, y + (g.thresh - f0) / (tile[c.l + HX] - f0), z);
	if (c.edges & 4u) store_vertex(g, verts, vi++, x, y, z + (g.thresh - f0) / (tile[c.l + HX * HY] - f0));
}

// the vertex on edge e of the cube at (x, y, z): its owner's base plus the rank of the edge's axis in the owner's mask
__device__ __forceinline__ uint32_t edge_vertex(const Grid& g, const uint32_t* __restrict__ vertmap, uint32_t x, uint32_t y, uint32_t z,
                                                uint32_t e) {
	const uint32_t code = (uint32_t)(EDGE_OWNER >> (5 * e)) & 31u, axis = code >> 3;
	const uint32_t m = vertmap[point_index(g, x + (code & 1u), y + ((code >> 1) & 1u), z + ((code >> 2) & 1u))];
	return (m & BASE_MASK) + __popc((m >> BASE_BITS) & ((1u << axis) - 1u));
}

__global__ void __launch_bounds__(THREADS) k_mc_emit_faces(Grid g, const float* __restrict__ density, const uint2* __restrict__ counts,
                                                           const uint2* __restrict__ bases, const uint32_t* __restrict__ vertmap,
                                                           int32_t* __restrict__ faces) {
	if (counts[blockIdx.x].y == 0) return;
	__shared__ float tile[HALO];
	__shared__ uint32_t wave_tot[THREADS / WAVE];
	const Cell c = load_cell(g, density, tile);
	uint32_t total;
	const uint32_t ti = bases[blockIdx.x].y + block_prefix(c.n_tris, wave_tot, &total);
	for (uint32_t k = 0; k < 3 * c.n_tris; ++k)
		faces[3 * (size_t)ti + k] = (int32_t)edge_vertex(g, vertmap, c.x, c.y, c.z, (uint32_t)d_tri[c.cube * 16 + k]);
}

// Area-weighted vertex normals: the sum of (p1 - p0) x (p2 - p0) over the triangles at the vertex, which points to the
// outside (f <= thresh) by the table's winding. A vertex on the edge leaving (x, y, z) along `axis` belongs to the
// cubes at (x, y, z) - {0, 1} in the two other axes; they are visited in that order, their triangles in table order.
__global__ void __launch_bounds__(256) k_mc_normals(Grid g, uint64_t n_points, const float* __restrict__ density,
                                                    const uint32_t* __restrict__ vertmap, const float* __restrict__ verts,
                                                    float* __restrict__ normals) {
	const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n_points) return;
	const uint32_t m = vertmap[i];
	const uint32_t edges = m >> BASE_BITS;
	if (!edges) return;
	const uint32_t x = (uint32_t)(i % g.rx), y = (uint32_t)((i / g.rx) % g.ry), z = (uint32_t)(i / ((uint64_t)g.rx * g.ry));
	uint32_t vi = m & BASE_MASK;
	for (uint32_t axis = 0; axis < 3; ++axis) {
		if (!(edges & (1u << axis))) continue;
		const uint32_t u = (axis + 1) % 3, v = (axis + 2) % 3;  // the two other axes
		float acc[3] = {0.f, 0.f, 0.f};
		for (uint32_t q = 0; q < 4; ++q) {
			uint32_t d[3] = {0, 0, 0};
			d[u] = q & 1u; d[v] = q >> 1;
			if (x < d[0] || y < d[1] || z < d[2]) continue;
			const uint32_t cx = x - d[0], cy = y - d[1], cz = z - d[2];
			if (cx + 1 >= g.rx || cy + 1 >= g.ry || cz + 1 >= g.rz) continue;
			// this edge's id in that cube: x edges 0 2 4 6, y edges 3 1 7 5, z edges 8 9 11 10 by the cube-local offset
			const uint32_t le = axis == 0 ? 2u * d[1] + 4u * d[2]
			                  : axis == 1 ? (d[0] ? 1u : 3u) + 4u * d[2]
			                              : (d[1] ? (d[0] ? 10u : 11u) : (d[0] ? 9u : 8u));
			uint32_t cube = 0;
			for (uint32_t k = 0; k < 8; ++k) {
				const uint32_t dx = (k == 1 || k == 2 || k == 5 || k == 6), dy = (k == 2 || k == 3 || k == 6 || k == 7), dz = k >> 2;
				if (density[point_index(g, cx + dx, cy + dy, cz + dz)] > g.thresh) cube |= 1u << k;
			}
			const uint32_t nt = d_ntris[cube];
			for (uint32_t t = 0; t < nt; ++t) {
				const int8_t* tri = d_tri + cube * 16 + 3 * t;
				if ((uint32_t)tri[0] != le && (uint32_t)tri[1] != le && (uint32_t)tri[2] != le) continue;
				float p[3][3];
				for (uint32_t k = 0; k < 3; ++k) {
					const uint32_t w = edge_vertex(g, vertmap, cx, cy, cz, (uint32_t)tri[k]);
					for (uint32_t j = 0; j < 3; ++j) p[k][j] = verts[3 * (size_t)w + j];
				}
				const float a[3] = {p[1][0] - p[0][0], p[1][1] - p[0][1], p[1][2] - p[0][2]};
				const float b[3] = {p[2][0] - p[0][0], p[2][1] - p[0][1], p[2][2] - p[0][2]};
				acc[0] += a[1] * b[2] - a[2] * b[1];
				acc[1] += a[2] * b[0] - a[0] * b[2];
				acc[2] += a[0] * b[1] - a[1] * b[0];
			}
		}
		for (uint32_t j = 0; j < 3; ++j) normals[3 * (size_t)vi + j] = acc[j];
		++vi;
	}
}

// ---- sampling the model on the grid ---------------------------------------------------------------------------------
struct SampleArgs {
	uint32_t rx, ry;
	uint64_t n_points;
	float scale[3], offset[3], rot[9];
	uint32_t has_rot, has_warp;
	float warp_min[3], warp_diag[3];
	uint32_t stride;  // 3, or 7 for a NerfNetwork (NerfCoordinate: position, dt, direction)
};

// Grid point p = aabb_min + (x, y, z) * (aabb_max - aabb_min) / (res - 1) (gen_vertices' vec * scale + offset), through
// transpose(aabb_to_local), then warped into the model's box as the renderer's inputs are (k_render_inputs, nerf_render.hip).
// Rows past the grid's end repeat its last point: the batch is padded to the inference granularity.
__global__ void __launch_bounds__(256) k_mc_positions(SampleArgs a, uint64_t start, uint32_t n_pad, float* __restrict__ out) {
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n_pad) return;
	const uint64_t idx = start + i < a.n_points ? start + i : a.n_points - 1;
	const uint32_t x = (uint32_t)(idx % a.rx), y = (uint32_t)((idx / a.rx) % a.ry), z = (uint32_t)(idx / ((uint64_t)a.rx * a.ry));
	float p[3] = {a.offset[0] + (float)x * a.scale[0], a.offset[1] + (float)y * a.scale[1], a.offset[2] + (float)z * a.scale[2]};
	if (a.has_rot) {
		const float q[3] = {a.rot[0] * p[0] + a.rot[3] * p[1] + a.rot[6] * p[2], a.rot[1] * p[0] + a.rot[4] * p[1] + a.rot[7] * p[2],
		                    a.rot[2] * p[0] + a.rot[5] * p[1] + a.rot[8] * p[2]};
		p[0] = q[0]; p[1] = q[1]; p[2] = q[2];
	}
	if (a.has_warp)
		for (int k = 0; k < 3; ++k) p[k] = (p[k] - a.warp_min[k]) / a.warp_diag[k];
	float* o = out + (size_t)i * a.stride;
	o[0] = p[0]; o[1] = p[1]; o[2] = p[2];
	if (a.stride == 7) {  // dt = warp_dt(MIN_CONE_STEPSIZE) = 0; the density does not depend on the direction
		o[3] = 0.f; o[4] = 0.5f; o[5] = 0.5f; o[6] = 0.5f;
	}
}

// row 0 of the model's fp16 output (SoA: n contiguous halves) -> the grid's float; the density as the renderer and the
// density grid update activate it (nerf_device.h)
__global__ void __launch_bounds__(256) k_mc_values(uint32_t n, const f16* __restrict__ row0, int kind, uint32_t act, float* __restrict__ out) {
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n) return;
	const float v = (float)row0[i];
	out[i] = kind == NGP_MC_NERF ? nerf::network_to_density(v, act) : kind == NGP_MC_SDF ? -v : v;
}

// NerfCoordinate rows at the vertices: warped position, dt 0, direction normalize(-normal) as (d + 1) / 2
__global__ void __launch_bounds__(256) k_mc_color_inputs(uint32_t n, uint32_t n_pad, const float* __restrict__ verts,
                                                         const float* __restrict__ normals, SampleArgs a, float* __restrict__ out) {
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n_pad) return;
	const uint32_t r = min(i, n - 1);
	float* o = out + (size_t)i * 7;
	float d[3] = {-normals[3 * (size_t)r], -normals[3 * (size_t)r + 1], -normals[3 * (size_t)r + 2]};
	const float len = sqrtf(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
	for (int k = 0; k < 3; ++k) {
		float p = verts[3 * (size_t)r + k];
		if (a.has_warp) p = (p - a.warp_min[k]) / a.warp_diag[k];
		o[k] = p;
		o[4 + k] = ((len > 0.f ? d[k] / len : 0.f) + 1.0f) * 0.5f;
	}
	o[3] = 0.f;
}
// NeRF: linear_to_srgb(network_to_rgb(raw)) of the inference's AoS {r, g, b, density} rows
__global__ void __launch_bounds__(256) k_mc_colors_nerf(uint32_t n, const f16* __restrict__ rgbd, uint32_t act, float* __restrict__ colors) {
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n) return;
	for (int k = 0; k < 3; ++k) colors[3 * (size_t)i + k] = linear_to_srgb(nerf::network_to_rgb((float)rgbd[4 * (size_t)i + k], act));
}
// SDF: 0.5 n + 0.5 of the normalised normal
__global__ void __launch_bounds__(256) k_mc_colors_normal(uint32_t n, const float* __restrict__ normals, float* __restrict__ colors) {
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n) return;
	const float* v = normals + 3 * (size_t)i;
	const float inv = 1.0f / sqrtf(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
	for (int k = 0; k < 3; ++k) colors[3 * (size_t)i + k] = 0.5f * (v[k] * inv) + 0.5f;
}

struct Buf {  // device memory released at scope exit
	void* p = nullptr;
	Buf() = default;
	Buf(const Buf&) = delete;
	Buf& operator=(const Buf&) = delete;
	template <typename T> T* alloc(size_t count) {
		NGP_HIP(hipMalloc(&p, std::max<size_t>(count * sizeof(T), 16)));
		return (T*)p;
	}
	void* release() { void* q = p; p = nullptr; return q; }
	~Buf() { if (p) (void)hipFree(p); }
};

int invalid(const char* what) {
	ngp::set_last_error(what);
	return NGP_INVALID;
}

// the generated table, uploaded once per device
void upload_tables() {
	static std::mutex mu;
	static bool done[64] = {};
	int dev = 0;
	NGP_HIP(hipGetDevice(&dev));
	std::lock_guard<std::mutex> lock(mu);
	if (dev < 0 || dev >= 64) throw Error("marching cubes: device index out of range");
	if (done[dev]) return;
	const Tables& T = tables();
	NGP_HIP(hipMemcpyToSymbol(HIP_SYMBOL(d_tri), T.tri, sizeof(T.tri)));
	NGP_HIP(hipMemcpyToSymbol(HIP_SYMBOL(d_ntris), T.n_tris, sizeof(T.n_tris)));
	done[dev] = true;
}

// res >= 2 per axis, fewer than 2^32 points, a box with positive finite sides
const char* check_grid(const uint32_t* res, const float* aabb_min, const float* aabb_max) {
	if (!res || !aabb_min || !aabb_max) return "null grid argument";
	uint64_t n = 1;
	for (int k = 0; k < 3; ++k) {
		if (res[k] < 2) return "every resolution must be at least 2";
		if (n > UINT64_MAX / res[k]) return "grids of 2^32 points or more are not supported";
		n *= res[k];
		const float d = aabb_max[k] - aabb_min[k];
		if (!(d > 0.f) || !std::isfinite(d)) return "empty or non-finite box";
	}
	if (n >= (1ull << 32)) return "grids of 2^32 points or more are not supported";
	return nullptr;
}

void fill_transform(const uint32_t* res, const float* aabb_min, const float* aabb_max, const float* aabb_to_local, float* scale,
                    float* offset, float* rot, uint32_t* has_rot) {
	for (int k = 0; k < 3; ++k) {
		scale[k] = (aabb_max[k] - aabb_min[k]) / (float)(res[k] - 1);
		offset[k] = aabb_min[k];
	}
	*has_rot = aabb_to_local != nullptr;
	for (int k = 0; k < 9; ++k) rot[k] = aabb_to_local ? aabb_to_local[k] : (k % 4 == 0 ? 1.f : 0.f);
}

}  // namespace
}  // namespace mc
}  // namespace ngp

using namespace ngp;

struct ngp_mesh {
	uint32_t n_verts = 0, n_tris = 0;
	float *verts = nullptr, *normals = nullptr, *colors = nullptr;
	int32_t* faces = nullptr;
	~ngp_mesh() {
		if (verts) (void)hipFree(verts);
		if (normals) (void)hipFree(normals);
		if (colors) (void)hipFree(colors);
		if (faces) (void)hipFree(faces);
	}
};

extern "C" {

int ngp_mc_tables(int8_t* triangle_table, uint16_t* edge_masks) {
	if (!triangle_table || !edge_masks) return mc::invalid("ngp_mc_tables: null output");
	const mc::Tables& T = mc::tables();
	std::memcpy(triangle_table, T.tri, sizeof(T.tri));
	std::memcpy(edge_masks, T.edge_mask, sizeof(T.edge_mask));
	return NGP_OK;
}

int ngp_marching_cubes_res(uint32_t res_1d, const float* aabb_min, const float* aabb_max, uint32_t* res_out) {
	if (!aabb_min || !aabb_max || !res_out) return mc::invalid("ngp_marching_cubes_res: null argument");
	if (res_1d == 0) return mc::invalid("ngp_marching_cubes_res: resolution 0");
	if (!mc::grid_res(res_1d, aabb_min, aabb_max, res_out)) return mc::invalid("ngp_marching_cubes_res: empty or non-finite box");
	return NGP_OK;
}

int ngp_density_on_grid(ngp_model* model, void* stream, int kind, const uint32_t* res, const float* aabb_min, const float* aabb_max,
                        const float* aabb_to_local, const float* warp_aabb_min, const float* warp_aabb_max,
                        uint32_t density_activation, uint32_t batch, int use_inference_params, float* density_out) {
	if (!model || !density_out) return mc::invalid("ngp_density_on_grid: null argument");
	if (kind < NGP_MC_NERF || kind > NGP_MC_RAW) return mc::invalid("ngp_density_on_grid: kind must be NGP_MC_NERF, NGP_MC_SDF or NGP_MC_RAW");
	if (const char* why = mc::check_grid(res, aabb_min, aabb_max)) return mc::invalid((std::string("ngp_density_on_grid: ") + why).c_str());
	if ((warp_aabb_min != nullptr) != (warp_aabb_max != nullptr)) return mc::invalid("ngp_density_on_grid: half a warp box");
	if (warp_aabb_min)
		for (int k = 0; k < 3; ++k)
			if (!(warp_aabb_max[k] - warp_aabb_min[k] > 0.f)) return mc::invalid("ngp_density_on_grid: empty warp box");
	if (batch == 0 || batch > (1u << 28)) return mc::invalid("ngp_density_on_grid: batch must be in [1, 2^28]");
	if (density_activation > nerf::ACT_EXP) return mc::invalid("ngp_density_on_grid: unknown density activation");
	const uint32_t width = ngp_model_input_width(model);
	if (width != 3 && width != 7) return mc::invalid("ngp_density_on_grid: the model must take 3 inputs or be a NerfNetwork (7)");
	if (kind == NGP_MC_NERF && width != 7) return mc::invalid("ngp_density_on_grid: NGP_MC_NERF needs a NerfNetwork");
	if (kind == NGP_MC_SDF && width != 3) return mc::invalid("ngp_density_on_grid: NGP_MC_SDF needs a 3-input network");
	NGP_TRY({
		hipStream_t s = (hipStream_t)stream;
		mc::SampleArgs a{};
		a.rx = res[0]; a.ry = res[1];
		a.n_points = (uint64_t)res[0] * res[1] * res[2];
		mc::fill_transform(res, aabb_min, aabb_max, aabb_to_local, a.scale, a.offset, a.rot, &a.has_rot);
		a.has_warp = warp_aabb_min != nullptr;
		for (int k = 0; k < 3; ++k) {
			a.warp_min[k] = a.has_warp ? warp_aabb_min[k] : 0.f;
			a.warp_diag[k] = a.has_warp ? warp_aabb_max[k] - warp_aabb_min[k] : 1.f;
		}
		a.stride = width;
		// one workspace for every batch: positions and the fp16 output, padded to the inference granularity
		const uint32_t per = (uint32_t)std::min<uint64_t>(batch, a.n_points);
		const uint32_t cap = next_multiple(per, 256u);
		mc::Buf pos_buf, out_buf;
		float* pos = pos_buf.alloc<float>((size_t)cap * width);
		f16* out16 = out_buf.alloc<f16>((size_t)cap * 16);
		check_rc(ngp_model_reserve(model, cap));
		for (uint64_t start = 0; start < a.n_points; start += per) {
			const uint32_t n = (uint32_t)std::min<uint64_t>(per, a.n_points - start);
			const uint32_t n_pad = next_multiple(n, 256u);
			{
				ProfScope ps("mc_positions", s);
				hipLaunchKernelGGL(mc::k_mc_positions, dim3(n_pad / 256), dim3(256), 0, s, a, start, n_pad, pos);
			}
			// SoA: output row 0 is n_pad contiguous halves
			if (width == 7) check_rc(ngp_density(model, s, n_pad, pos, 7, out16, n_pad, NGP_LAYOUT_SOA, use_inference_params));
			else check_rc(ngp_inference(model, s, n_pad, pos, 3, out16, n_pad, NGP_LAYOUT_SOA, use_inference_params));
			{
				ProfScope ps("mc_values", s);
				hipLaunchKernelGGL(mc::k_mc_values, dim3(n_pad / 256), dim3(256), 0, s, n, out16, kind, density_activation, density_out + start);
			}
		}
		NGP_HIP(hipGetLastError());
		NGP_HIP(hipStreamSynchronize(s));  // the workspace is released on return
	});
}

int ngp_marching_cubes(void* stream, const float* density, const uint32_t* res, const float* aabb_min, const float* aabb_max,
                       const float* aabb_to_local, float thresh, ngp_mesh** out) {
	if (!density || !out) return mc::invalid("ngp_marching_cubes: null argument");
	if (const char* why = mc::check_grid(res, aabb_min, aabb_max)) return mc::invalid((std::string("ngp_marching_cubes: ") + why).c_str());
	if (!std::isfinite(thresh)) return mc::invalid("ngp_marching_cubes: non-finite threshold");
	NGP_TRY({
		hipStream_t s = (hipStream_t)stream;
		mc::upload_tables();
		mc::Grid g{};
		g.rx = res[0]; g.ry = res[1]; g.rz = res[2];
		g.nbx = div_round_up(g.rx, mc::TX); g.nby = div_round_up(g.ry, mc::TY); g.nbz = div_round_up(g.rz, mc::TZ);
		mc::fill_transform(res, aabb_min, aabb_max, aabb_to_local, g.scale, g.offset, g.rot, &g.has_rot);
		g.thresh = thresh;
		const uint64_t n_points = (uint64_t)g.rx * g.ry * g.rz;
		const uint64_t n_blocks64 = (uint64_t)g.nbx * g.nby * g.nbz;
		NGP_CHECK(n_blocks64 < (1ull << 31), "ngp_marching_cubes: too many blocks");
		const uint32_t n_blocks = (uint32_t)n_blocks64;

		mc::Buf counts_buf, bases_buf, map_buf;
		uint2* counts = counts_buf.alloc<uint2>(n_blocks);
		uint2* bases = bases_buf.alloc<uint2>((size_t)n_blocks + 1);
		{
			ProfScope ps("mc_count", s);
			hipLaunchKernelGGL(mc::k_mc_count, dim3(n_blocks), dim3(mc::THREADS), 0, s, g, density, counts);
			hipLaunchKernelGGL(mc::k_mc_scan, dim3(1), dim3(mc::SCAN_THREADS), 0, s, n_blocks, counts, bases);
		}
		uint2 totals;
		NGP_HIP(hipMemcpyAsync(&totals, bases + n_blocks, sizeof(totals), hipMemcpyDeviceToHost, s));
		NGP_HIP(hipStreamSynchronize(s));
		NGP_CHECK(totals.x <= mc::BASE_MASK, "ngp_marching_cubes: more than 2^29 vertices");

		std::unique_ptr<ngp_mesh> mesh(new ngp_mesh());
		mesh->n_verts = totals.x;
		mesh->n_tris = totals.y;
		if (totals.x) {
			NGP_HIP(hipMalloc((void**)&mesh->verts, (size_t)totals.x * 12));
			NGP_HIP(hipMalloc((void**)&mesh->normals, (size_t)totals.x * 12));
			NGP_HIP(hipMemsetAsync(mesh->normals, 0, (size_t)totals.x * 12, s));
			uint32_t* vertmap = map_buf.alloc<uint32_t>(n_points);
			NGP_HIP(hipMemsetAsync(vertmap, 0, n_points * 4, s));
			{
				ProfScope ps("mc_vertices", s);
				hipLaunchKernelGGL(mc::k_mc_emit_vertices, dim3(n_blocks), dim3(mc::THREADS), 0, s, g, density, counts, bases, vertmap, mesh->verts);
			}
			if (totals.y) {
				NGP_HIP(hipMalloc((void**)&mesh->faces, (size_t)totals.y * 12));
				{
					ProfScope ps("mc_faces", s);
					hipLaunchKernelGGL(mc::k_mc_emit_faces, dim3(n_blocks), dim3(mc::THREADS), 0, s, g, density, counts, bases, vertmap, mesh->faces);
				}
				{
					ProfScope ps("mc_normals", s);
					hipLaunchKernelGGL(mc::k_mc_normals, dim3(div_round_up(n_points, 256)), dim3(256), 0, s, g, n_points, density, vertmap,
					                   mesh->verts, mesh->normals);
				}
			}
			NGP_HIP(hipGetLastError());
			NGP_HIP(hipStreamSynchronize(s));  // the vertex map is released on return
		}
		*out = mesh.release();
	});
}

int ngp_mesh_vertex_colors(ngp_mesh* mesh, ngp_model* model, void* stream, int kind, const float* warp_aabb_min,
                           const float* warp_aabb_max, uint32_t rgb_activation, int use_inference_params) {
	if (!mesh) return mc::invalid("ngp_mesh_vertex_colors: null mesh");
	if (kind != NGP_MC_NERF && kind != NGP_MC_SDF) return mc::invalid("ngp_mesh_vertex_colors: kind must be NGP_MC_NERF or NGP_MC_SDF");
	if (kind == NGP_MC_NERF) {
		if (!model || ngp_model_input_width(model) != 7) return mc::invalid("ngp_mesh_vertex_colors: NGP_MC_NERF needs a NerfNetwork");
		if ((warp_aabb_min != nullptr) != (warp_aabb_max != nullptr)) return mc::invalid("ngp_mesh_vertex_colors: half a warp box");
		if (warp_aabb_min)
			for (int k = 0; k < 3; ++k)
				if (!(warp_aabb_max[k] - warp_aabb_min[k] > 0.f)) return mc::invalid("ngp_mesh_vertex_colors: empty warp box");
		if (rgb_activation > nerf::ACT_EXP) return mc::invalid("ngp_mesh_vertex_colors: unknown rgb activation");
	}
	NGP_TRY({
		hipStream_t s = (hipStream_t)stream;
		const uint32_t n = mesh->n_verts;
		if (n == 0) return NGP_OK;
		if (!mesh->colors) NGP_HIP(hipMalloc((void**)&mesh->colors, (size_t)n * 12));
		if (kind == NGP_MC_SDF) {
			ProfScope ps("mc_colors", s);
			hipLaunchKernelGGL(mc::k_mc_colors_normal, dim3(div_round_up(n, 256)), dim3(256), 0, s, n, mesh->normals, mesh->colors);
			NGP_HIP(hipGetLastError());
			return NGP_OK;
		}
		mc::SampleArgs a{};
		a.has_warp = warp_aabb_min != nullptr;
		for (int k = 0; k < 3; ++k) {
			a.warp_min[k] = a.has_warp ? warp_aabb_min[k] : 0.f;
			a.warp_diag[k] = a.has_warp ? warp_aabb_max[k] - warp_aabb_min[k] : 1.f;
		}
		const uint32_t batch = 1u << 20;
		const uint32_t cap = next_multiple(std::min(n, batch), 256u);
		mc::Buf in_buf, out_buf;
		float* in = in_buf.alloc<float>((size_t)cap * 7);
		f16* rgbd = out_buf.alloc<f16>((size_t)cap * 4);
		check_rc(ngp_model_reserve(model, cap));
		for (uint32_t start = 0; start < n; start += batch) {
			const uint32_t m = std::min(batch, n - start), m_pad = next_multiple(m, 256u);
			{
				ProfScope ps("mc_colors", s);
				hipLaunchKernelGGL(mc::k_mc_color_inputs, dim3(m_pad / 256), dim3(256), 0, s, m, m_pad, mesh->verts + 3 * (size_t)start,
				                   mesh->normals + 3 * (size_t)start, a, in);
			}
			check_rc(ngp_inference(model, s, m_pad, in, 7, rgbd, 4, NGP_LAYOUT_AOS_RGBD, use_inference_params));
			{
				ProfScope ps("mc_colors", s);
				hipLaunchKernelGGL(mc::k_mc_colors_nerf, dim3(m_pad / 256), dim3(256), 0, s, m, rgbd, rgb_activation,
				                   mesh->colors + 3 * (size_t)start);
			}
		}
		NGP_HIP(hipGetLastError());
		NGP_HIP(hipStreamSynchronize(s));  // the workspace is released on return
	});
}

int ngp_mesh_counts(const ngp_mesh* mesh, uint32_t* n_verts, uint32_t* n_tris) {
	if (!mesh) return mc::invalid("ngp_mesh_counts: null mesh");
	if (n_verts) *n_verts = mesh->n_verts;
	if (n_tris) *n_tris = mesh->n_tris;
	return NGP_OK;
}

int ngp_mesh_read(const ngp_mesh* mesh, void* stream, float* verts_host, float* normals_host, float* colors_host, int32_t* faces_host) {
	if (!mesh) return mc::invalid("ngp_mesh_read: null mesh");
	if (colors_host && mesh->n_verts && !mesh->colors) return mc::invalid("ngp_mesh_read: no colours (ngp_mesh_vertex_colors first)");
	NGP_TRY({
		hipStream_t s = (hipStream_t)stream;
		const size_t vb = (size_t)mesh->n_verts * 12, fb = (size_t)mesh->n_tris * 12;
		if (vb && verts_host) NGP_HIP(hipMemcpyAsync(verts_host, mesh->verts, vb, hipMemcpyDeviceToHost, s));
		if (vb && normals_host) NGP_HIP(hipMemcpyAsync(normals_host, mesh->normals, vb, hipMemcpyDeviceToHost, s));
		if (vb && colors_host) NGP_HIP(hipMemcpyAsync(colors_host, mesh->colors, vb, hipMemcpyDeviceToHost, s));
		if (fb && faces_host) NGP_HIP(hipMemcpyAsync(faces_host, mesh->faces, fb, hipMemcpyDeviceToHost, s));
		if (vb || fb) NGP_HIP(hipStreamSynchronize(s));
	});
}

int ngp_mesh_save(const char* path, uint32_t n_verts, const float* verts_host, const float* normals_host, const float* colors_host,
                  uint32_t n_tris, const int32_t* faces_host, float scale, const float* offset) {
	if (!path || !*path) return mc::invalid("ngp_mesh_save: no path");
	if ((n_verts && !verts_host) || (n_tris && !faces_host)) return mc::invalid("ngp_mesh_save: null vertex or face array");
	if (!(scale != 0.f) || !std::isfinite(scale)) return mc::invalid("ngp_mesh_save: scale must be finite and not 0");
	for (size_t i = 0; i < 3 * (size_t)n_tris; ++i)
		if (faces_host[i] < 0 || (uint32_t)faces_host[i] >= n_verts) return mc::invalid("ngp_mesh_save: face index out of range");
	const float zero[3] = {0.f, 0.f, 0.f};
	std::string err;
	if (!mc::save_mesh(path, n_verts, verts_host, normals_host, colors_host, n_tris, faces_host, scale, offset ? offset : zero, &err)) {
		ngp::set_last_error(err.c_str());
		return NGP_ERROR;
	}
	return NGP_OK;
}

void ngp_mesh_destroy(ngp_mesh* mesh) { delete mesh; }

}  // extern "C"
