// nerf_density_grid.hip — the NeRF occupancy grid's update for gfx950 (see nerf.h): sample generation, the splat in its
// direct, binned and sorted forms, the EMA, the mean and the bitfield with its mips, fused and in the reference's order.
#include <algorithm>
#include <cmath>

#include "nerf_device.h"
#include "rng.h"

namespace ngp {
namespace nerf {

// ------------------------------------------------------------------------------------------------
// occupancy grid
// ------------------------------------------------------------------------------------------------
// generate_grid_samples_nerf_nonuniform (testbed_nerf.cu:635-676)
// The candidate test of generate_grid_samples_nerf_nonuniform (grid_in[idx] > thresh) for every cell of the
// sampled cascades as one bit per cell: a linear pass over the grid (32 cells -> one word, 128-B coalesced reads),
// so the samples' up-to-10 candidates are tested against a 256-KB-per-cascade mask that stays in L2 instead of
// one scattered 4-B grid read (a 64-B transaction) per candidate, in a chain.
__global__ void k_grid_mask(uint32_t n_words, const float* __restrict__ grid, float thresh, uint32_t* __restrict__ mask) {
	const uint32_t w = blockIdx.x * blockDim.x + threadIdx.x;
	if (w >= n_words) return;
	const float4* g = (const float4*)(grid + (size_t)w * 32);
	uint32_t bits = 0;
#pragma unroll
	for (uint32_t q = 0; q < 8; ++q) {
		const float4 v = g[q];
		bits |= (v.x > thresh ? 1u : 0u) << (4 * q) | (v.y > thresh ? 1u : 0u) << (4 * q + 1) |
		        (v.z > thresh ? 1u : 0u) << (4 * q + 2) | (v.w > thresh ? 1u : 0u) << (4 * q + 3);
	}
	mask[w] = bits;
}

#ifndef NGP_GRID_CAND_FIRST
#define NGP_GRID_CAND_FIRST 2  // k_grid_samples: candidates whose mask words every lane loads (10: all at once)
#endif
static_assert(NGP_GRID_CAND_FIRST >= 1 && NGP_GRID_CAND_FIRST <= 10, "grid sample candidates");
__global__ void k_grid_samples(uint32_t n, Rng rng, uint32_t step, const ngp_nerf_config cfg, const uint32_t* __restrict__ mask,
                               uint32_t n_cascades, float* __restrict__ out, uint32_t* __restrict__ indices) {
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n) return;
	pcg_advance(rng, (uint64_t)i * 4);
	const uint32_t level = (uint32_t)(pcg_float(rng) * n_cascades) % n_cascades;
	// the candidates' mask words (L2 hits) in batches of GRID_CAND_FIRST and the rest, the second batch only for the
	// lanes whose first batch has no passing cell: the first candidate that passes, as the reference's loop takes it
	// (its last candidate when none passes). The kernel is bound by the L2 request rate, and in the uniform pass nearly
	// every first candidate passes.
	constexpr uint32_t NA = NGP_GRID_CAND_FIRST;
	uint32_t cand[10], word[10];
	const uint32_t base = (i + step * n) * 56924617u + 96925573u;
#pragma unroll
	for (uint32_t j = 0; j < 10; ++j) cand[j] = (base + j * 19349663u) % GRID_N_CELLS + level * GRID_N_CELLS;
#pragma unroll
	for (uint32_t j = 0; j < NA; ++j) word[j] = mask[cand[j] >> 5];
	uint32_t idx = ~0u;
#pragma unroll
	for (int j = (int)NA - 1; j >= 0; --j)
		if ((word[j] >> (cand[j] & 31u)) & 1u) idx = cand[j];
	if (idx == ~0u) {
#pragma unroll
		for (uint32_t j = NA; j < 10; ++j) word[j] = mask[cand[j] >> 5];
		idx = cand[9];
#pragma unroll
		for (int j = 9; j >= (int)NA; --j)
			if ((word[j] >> (cand[j] & 31u)) & 1u) idx = cand[j];
	}
	const uint32_t pos_idx = idx % GRID_N_CELLS;
	const uint32_t x = morton3D_invert(pos_idx >> 0), y = morton3D_invert(pos_idx >> 1), z = morton3D_invert(pos_idx >> 2);
	const float r0 = pcg_float(rng), r1 = pcg_float(rng), r2 = pcg_float(rng);
	const float sc = scalbnf(1.0f, (int)level);
	const float px = (((float)x + r0) / (float)GRIDSIZE - 0.5f) * sc + 0.5f;
	const float py = (((float)y + r1) / (float)GRIDSIZE - 0.5f) * sc + 0.5f;
	const float pz = (((float)z + r2) / (float)GRIDSIZE - 0.5f) * sc + 0.5f;
	out[(size_t)i * 3 + 0] = (px - cfg.aabb_min[0]) / (cfg.aabb_max[0] - cfg.aabb_min[0]);
	out[(size_t)i * 3 + 1] = (py - cfg.aabb_min[1]) / (cfg.aabb_max[1] - cfg.aabb_min[1]);
	out[(size_t)i * 3 + 2] = (pz - cfg.aabb_min[2]) / (cfg.aabb_max[2] - cfg.aabb_min[2]);
	indices[i] = idx;
}

// splat_grid_samples_nerf_max_nearest_neighbor (:678-702); density_rm = density MLP output row 0 (RM)
__global__ void k_grid_splat(uint32_t n, const uint32_t* __restrict__ indices, const f16* __restrict__ density, uint32_t act,
                             float* __restrict__ grid_out) {
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n) return;
	const float mlp = network_to_density((float)density[i], act);
	const float thickness = mlp * scalbnf(MIN_CONE_STEPSIZE, 0);
	atomicMax((uint32_t*)&grid_out[indices[i]], __float_as_uint(thickness));
}

// ema_grid_samples_nerf (:731-754): max-filter
__global__ void k_grid_ema(uint32_t n, float decay, float* __restrict__ grid, const float* __restrict__ tmp) {
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n) return;
	const float prev = grid[i];
	grid[i] = prev < 0.f ? prev : fmaxf(prev * decay, tmp[i]);
}

// reduce_sum(max(v,0)/N) over cascade 0 (:3544-3551), fixed order: 512 blocks x 256 threads, then one block.
__global__ void __launch_bounds__(256) k_grid_mean_partial(const float* __restrict__ grid, float* __restrict__ partial) {
	__shared__ float s[256];
	const uint32_t per_block = GRID_N_CELLS / 512;
	const uint32_t base = blockIdx.x * per_block;
	float acc = 0.f;
	for (uint32_t k = threadIdx.x; k < per_block; k += 256) acc += fmaxf(grid[base + k], 0.f) / (float)GRID_N_CELLS;
	s[threadIdx.x] = acc;
	__syncthreads();
	for (uint32_t off = 128; off > 0; off >>= 1) {
		if (threadIdx.x < off) s[threadIdx.x] += s[threadIdx.x + off];
		__syncthreads();
	}
	if (threadIdx.x == 0) partial[blockIdx.x] = s[0];
}
__global__ void __launch_bounds__(512) k_grid_mean_final(const float* __restrict__ partial, float* __restrict__ mean) {
	__shared__ float s[512];
	s[threadIdx.x] = partial[threadIdx.x];
	__syncthreads();
	for (uint32_t off = 256; off > 0; off >>= 1) {
		if (threadIdx.x < off) s[threadIdx.x] += s[threadIdx.x + off];
		__syncthreads();
	}
	if (threadIdx.x == 0) *mean = s[0];
}

// grid_to_bitfield (:762-786)
__global__ void k_grid_to_bitfield(uint32_t n_elements, uint32_t n_nonzero, const float* __restrict__ grid,
                                   uint8_t* __restrict__ bitfield, const float* __restrict__ mean) {
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n_elements) return;
	if (i >= n_nonzero) { bitfield[i] = 0; return; }
	const float thresh = fminf(MIN_OPTICAL_THICKNESS, *mean);
	uint8_t bits = 0;
#pragma unroll
	for (uint8_t j = 0; j < 8; ++j) bits |= grid[i * 8 + j] > thresh ? ((uint8_t)1 << j) : 0;
	bitfield[i] = bits;
}

// bitfield_max_pool (:788-809)
__global__ void k_bitfield_max_pool(uint32_t n, const uint8_t* __restrict__ prev, uint8_t* __restrict__ next) {
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n) return;
	uint8_t bits = 0;
#pragma unroll
	for (uint8_t j = 0; j < 8; ++j) bits |= prev[i * 8 + j] > 0 ? ((uint8_t)1 << j) : 0;
	const uint32_t x = morton3D_invert(i >> 0) + GRIDSIZE / 8;
	const uint32_t y = morton3D_invert(i >> 1) + GRIDSIZE / 8;
	const uint32_t z = morton3D_invert(i >> 2) + GRIDSIZE / 8;
	next[morton3D(x, y, z)] |= bits;
}

size_t grid_mask_words(uint32_t n_cascades) { return (size_t)n_cascades * GRID_N_CELLS / 32; }
void grid_generate_samples(uint32_t n, Rng rng, uint32_t step, const ngp_nerf_config& cfg, const float* grid_in,
                           uint32_t n_cascades, float thresh, float* positions, uint32_t* indices, uint32_t* mask, hipStream_t s) {
	if (n == 0) return;
	const uint32_t nw = (uint32_t)grid_mask_words(n_cascades);
	k_grid_mask<<<div_round_up(nw, 256), 256, 0, s>>>(nw, grid_in, thresh, mask);
	k_grid_samples<<<div_round_up(n, 128), 128, 0, s>>>(n, rng, step, cfg, mask, n_cascades, positions, indices);
	NGP_HIP(hipGetLastError());
}
// The splat as a counting sort by cell bin (fox: 5.2 M samples into 10.5 M cells). The direct splat's atomics are
// scattered over the whole grid and run at ~32 G/s whatever their locality (an XCD-sliced variant that kept each
// XCD's cells L2-resident measured no faster): here each sample costs two LDS atomics and 8 B of
// coalesced-ish traffic instead. Bins of 8192 cells (32 KB of LDS):
//   k_splat_hist: per-block LDS histogram of the samples' bins, added to the global counts (one atomic per bin and
//     block);
//   k_splat_scan: the bins' offsets (one block);
//   k_splat_scatter: each block reserves its range in every bin (cursor atomics), ranks its samples in LDS and writes
//     (cell in bin << 16 | density bits) there;
//   k_splat_bins: a block per bin takes the max of its samples in LDS with the same uint compare as the atomics, then
//     writes all 8192 cells (so no memset of grid_tmp).
// Max does not depend on the order, so grid_tmp is bit-identical to memset(0) + k_grid_splat.
#ifndef NGP_SPLAT_THREADS
#define NGP_SPLAT_THREADS 1024
#endif
constexpr uint32_t SPLAT_THREADS = NGP_SPLAT_THREADS;  // k_splat_hist / k_splat_scatter block size
constexpr uint32_t SPLAT_BIN_SHIFT = 13, SPLAT_BIN = 1u << SPLAT_BIN_SHIFT, SPLAT_MAX_BINS = 8 * GRID_N_CELLS / SPLAT_BIN;
#ifndef NGP_SPLAT_MAX_BLOCKS
#define NGP_SPLAT_MAX_BLOCKS 256  // 128 -> 256: fox scatter 88.5 -> 63.5 us (gpurun_out/r06as_256)
#endif
#ifndef NGP_SPLAT_CHUNK
#define NGP_SPLAT_CHUNK 4096  // samples per k_splat_hist / k_splat_scatter block at least (Lego: 256 blocks, not 64)
#endif
static uint32_t splat_blocks(uint32_t n) {
	return std::max(1u, std::min((uint32_t)NGP_SPLAT_MAX_BLOCKS, div_round_up(n, NGP_SPLAT_CHUNK)));
}
__device__ __forceinline__ void splat_chunk(uint32_t n, uint32_t nb, uint32_t* s0, uint32_t* s1) {
	*s0 = (uint32_t)((uint64_t)n * blockIdx.x / nb);
	*s1 = (uint32_t)((uint64_t)n * (blockIdx.x + 1) / nb);
}
__global__ void __launch_bounds__(SPLAT_THREADS) k_splat_hist(uint32_t n, const uint32_t* __restrict__ indices, uint32_t n_bins,
                                                   uint32_t* __restrict__ counts) {
	__shared__ uint32_t h[SPLAT_MAX_BINS];
	for (uint32_t b = threadIdx.x; b < n_bins; b += SPLAT_THREADS) h[b] = 0;
	__syncthreads();
	uint32_t s0, s1;
	splat_chunk(n, gridDim.x, &s0, &s1);
	for (uint32_t i = s0 + threadIdx.x; i < s1; i += 4 * SPLAT_THREADS) {
		uint32_t k[4];
#pragma unroll
		for (uint32_t u = 0; u < 4; ++u) k[u] = i + u * SPLAT_THREADS < s1 ? indices[i + u * SPLAT_THREADS] : ~0u;
#pragma unroll
		for (uint32_t u = 0; u < 4; ++u)
			if (k[u] != ~0u) atomicAdd(&h[k[u] >> SPLAT_BIN_SHIFT], 1u);
	}
	__syncthreads();
	for (uint32_t b = threadIdx.x; b < n_bins; b += SPLAT_THREADS)
		if (h[b]) atomicAdd(&counts[b], h[b]);
}
__global__ void __launch_bounds__(1024) k_splat_scan(uint32_t n_bins, const uint32_t* __restrict__ counts,
                                                    uint32_t* __restrict__ offsets, uint32_t* __restrict__ cursor) {
	__shared__ uint32_t sh[1024];
	const uint32_t b0 = 2 * threadIdx.x;  // two bins per thread (n_bins <= 2048)
	const uint32_t c0 = b0 < n_bins ? counts[b0] : 0u, c1 = b0 + 1 < n_bins ? counts[b0 + 1] : 0u;
	sh[threadIdx.x] = c0 + c1;
	__syncthreads();
	for (uint32_t off = 1; off < 1024; off <<= 1) {  // inclusive scan (Hillis-Steele)
		const uint32_t v = threadIdx.x >= off ? sh[threadIdx.x - off] : 0u;
		__syncthreads();
		sh[threadIdx.x] += v;
		__syncthreads();
	}
	const uint32_t ex = sh[threadIdx.x] - c0 - c1;
	if (b0 < n_bins) { offsets[b0] = ex; cursor[b0] = ex; }
	if (b0 + 1 < n_bins) { offsets[b0 + 1] = ex + c0; cursor[b0 + 1] = ex + c0; }
	if (threadIdx.x == 1023) offsets[n_bins] = sh[1023];
}
// SORT: the samples themselves into bin order before the density evaluation, one 16-B record per sample (x, y, z and
// the cell within the bin as the 4th word: one store request per sample); else the (cell in bin, density bits) pairs
// after it.
template <bool SORT>
__global__ void __launch_bounds__(SPLAT_THREADS) k_splat_scatter(uint32_t n, const uint32_t* __restrict__ indices,
                                                                const f16* __restrict__ density,
                                                                const float* __restrict__ positions, uint32_t n_bins,
                                                                uint32_t* __restrict__ cursor, uint32_t* __restrict__ packed,
                                                                float4* __restrict__ pos_out) {
	__shared__ uint32_t h[SPLAT_MAX_BINS], base[SPLAT_MAX_BINS];
	for (uint32_t b = threadIdx.x; b < n_bins; b += SPLAT_THREADS) h[b] = 0;
	__syncthreads();
	uint32_t s0, s1;
	splat_chunk(n, gridDim.x, &s0, &s1);
	for (uint32_t i = s0 + threadIdx.x; i < s1; i += 4 * SPLAT_THREADS) {
		uint32_t k[4];
#pragma unroll
		for (uint32_t u = 0; u < 4; ++u) k[u] = i + u * SPLAT_THREADS < s1 ? indices[i + u * SPLAT_THREADS] : ~0u;
#pragma unroll
		for (uint32_t u = 0; u < 4; ++u)
			if (k[u] != ~0u) atomicAdd(&h[k[u] >> SPLAT_BIN_SHIFT], 1u);
	}
	__syncthreads();
	for (uint32_t b = threadIdx.x; b < n_bins; b += SPLAT_THREADS) {
		if (h[b]) base[b] = atomicAdd(&cursor[b], h[b]);
		h[b] = 0;
	}
	__syncthreads();
	for (uint32_t i = s0 + threadIdx.x; i < s1; i += 4 * SPLAT_THREADS) {
		uint32_t k[4];
		uint16_t d[4];
		float px[4], py[4], pz[4];
#pragma unroll
		for (uint32_t u = 0; u < 4; ++u) {
			const bool ok = i + u * SPLAT_THREADS < s1;
			const uint32_t j = i + u * SPLAT_THREADS;
			k[u] = ok ? indices[j] : ~0u;
			if (SORT) {
				px[u] = ok ? positions[(size_t)j * 3 + 0] : 0.f;
				py[u] = ok ? positions[(size_t)j * 3 + 1] : 0.f;
				pz[u] = ok ? positions[(size_t)j * 3 + 2] : 0.f;
			} else {
				d[u] = ok ? __builtin_bit_cast(uint16_t, density[j]) : (uint16_t)0;
			}
		}
#pragma unroll
		for (uint32_t u = 0; u < 4; ++u) {
			if (k[u] == ~0u) continue;
			const uint32_t b = k[u] >> SPLAT_BIN_SHIFT;
			const uint32_t slot = base[b] + atomicAdd(&h[b], 1u);
			if (SORT) {
				pos_out[slot] = make_float4(px[u], py[u], pz[u], __uint_as_float(k[u] & (SPLAT_BIN - 1)));
			} else {
				packed[slot] = (k[u] & (SPLAT_BIN - 1)) << 16 | d[u];
			}
		}
	}
}
// SORT: bin b's samples are [offsets[b], offsets[b + 1]) of the sorted records (cell in the 4th word), their densities
// density[k - lo] for the shard [lo, hi) this rank evaluated
template <bool SORT>
__global__ void __launch_bounds__(1024) k_splat_bins(const uint32_t* __restrict__ offsets, const uint32_t* __restrict__ packed,
                                                    const float4* __restrict__ recs, const f16* __restrict__ density,
                                                    uint32_t lo, uint32_t hi, uint32_t act, float* __restrict__ grid_out) {
	__shared__ uint32_t m[SPLAT_BIN];
	for (uint32_t c = threadIdx.x; c < SPLAT_BIN; c += 1024) m[c] = 0;
	__syncthreads();
	const uint32_t b = blockIdx.x;
	const uint32_t k0 = SORT ? std::max(offsets[b], lo) : offsets[b], e = SORT ? std::min(offsets[b + 1], hi) : offsets[b + 1];
	for (uint32_t k = k0 + threadIdx.x; k < e; k += 1024) {
		uint32_t c;
		f16 d;
		if (SORT) {
			c = __float_as_uint(recs[k].w);
			d = density[k - lo];
		} else {
			const uint32_t v = packed[k];
			c = v >> 16;
			d = __builtin_bit_cast(f16, (uint16_t)(v & 0xffffu));
		}
		const float mlp = network_to_density((float)d, act);
		const float thickness = mlp * scalbnf(MIN_CONE_STEPSIZE, 0);
		atomicMax(&m[c], __float_as_uint(thickness));
	}
	__syncthreads();
	uint4* out = (uint4*)(grid_out + (size_t)b * SPLAT_BIN);
	for (uint32_t q = threadIdx.x; q < SPLAT_BIN / 4; q += 1024) out[q] = make_uint4(m[4 * q], m[4 * q + 1], m[4 * q + 2], m[4 * q + 3]);
}

size_t grid_splat_scratch_u32(uint32_t n, uint32_t n_cells) { return 3 * ((size_t)(n_cells >> SPLAT_BIN_SHIFT) + 1) + n; }

void grid_splat_max(uint32_t n, const uint32_t* indices, const f16* density_rm, uint32_t act, float* grid_tmp, hipStream_t s) {
	if (n == 0) return;
	k_grid_splat<<<div_round_up(n, 128), 128, 0, s>>>(n, indices, density_rm, act, grid_tmp);
	NGP_HIP(hipGetLastError());
}
// the histogram, offsets and cursors of n samples' bins (scratch: counts, offsets, cursor of n_bins + 1 words each)
static uint32_t splat_bin_offsets(uint32_t n, const uint32_t* indices, uint32_t n_cells, uint32_t* scratch, hipStream_t s) {
	const uint32_t n_bins = n_cells >> SPLAT_BIN_SHIFT;
	NGP_CHECK(n_cells % SPLAT_BIN == 0 && n_bins <= SPLAT_MAX_BINS, "grid splat: bad cell count");
	uint32_t* counts = scratch;
	NGP_HIP(hipMemsetAsync(counts, 0, (size_t)n_bins * 4, s));
	if (n) k_splat_hist<<<splat_blocks(n), SPLAT_THREADS, 0, s>>>(n, indices, n_bins, counts);
	k_splat_scan<<<1, 1024, 0, s>>>(n_bins, counts, counts + n_bins + 1, counts + 2 * (n_bins + 1));
	return n_bins;
}
void grid_splat_max_binned(uint32_t n, const uint32_t* indices, const f16* density_rm, uint32_t act, float* grid_tmp,
                           uint32_t n_cells, uint32_t* scratch, hipStream_t s) {
	const uint32_t n_bins = splat_bin_offsets(n, indices, n_cells, scratch, s);
	const uint32_t* offsets = scratch + n_bins + 1;
	uint32_t* cursor = scratch + 2 * (n_bins + 1);
	uint32_t* packed = cursor + n_bins + 1;
	if (n) k_splat_scatter<false><<<splat_blocks(n), SPLAT_THREADS, 0, s>>>(n, indices, density_rm, nullptr, n_bins, cursor, packed,
	                                                                       nullptr);
	k_splat_bins<false><<<n_bins, 1024, 0, s>>>(offsets, packed, nullptr, nullptr, 0, 0, act, grid_tmp);
	NGP_HIP(hipGetLastError());
}
size_t grid_sort_scratch_u32(uint32_t n, uint32_t n_cells) { return 3 * ((size_t)(n_cells >> SPLAT_BIN_SHIFT) + 1); }
void grid_sort_samples(uint32_t n, const float* positions, const uint32_t* indices, uint32_t n_cells, uint32_t* scratch,
                       float* recs, hipStream_t s) {
	const uint32_t n_bins = splat_bin_offsets(n, indices, n_cells, scratch, s);
	uint32_t* cursor = scratch + 2 * (n_bins + 1);
	if (n) k_splat_scatter<true><<<splat_blocks(n), SPLAT_THREADS, 0, s>>>(n, indices, nullptr, positions, n_bins, cursor, nullptr,
	                                                                      (float4*)recs);
	NGP_HIP(hipGetLastError());
}
void grid_splat_sorted(uint32_t n_cells, const uint32_t* scratch, const float* recs, const f16* density_rm, uint32_t lo,
                       uint32_t hi, uint32_t act, float* grid_tmp, hipStream_t s) {
	const uint32_t n_bins = n_cells >> SPLAT_BIN_SHIFT;
	const uint32_t* offsets = scratch + n_bins + 1;
	k_splat_bins<true><<<n_bins, 1024, 0, s>>>(offsets, nullptr, (const float4*)recs, density_rm, lo, hi, act, grid_tmp);
	NGP_HIP(hipGetLastError());
}
// The update step's finalization in three launches instead of ten (the reference's ema_grid_samples_nerf,
// update_density_grid_mean_and_bitfield and 7 bitfield_max_pool launches), the same float operations in the same
// order, so the same bits:
//   k_grid_ema_mean: the EMA of every cell; blocks [0, 512) take cascade 0 in k_grid_mean_partial's mapping and
//     accumulate its mean partials from the values they just wrote;
//   k_grid_bitfield: every block reduces the 512 partials in k_grid_mean_final's tree (block 0 stores the mean),
//     then writes 8 bitfield bytes per thread;
//   the pools into mips 1 .. max_cascade + 1 (full grids), then k_bitfield_pool_tail: one block for the mips above,
//     whose sources are zero outside a central region that halves per mip (max_cascade + 1: 64^3 cells, ...).
__global__ void __launch_bounds__(256) k_grid_ema_mean(uint32_t n, float decay, float* __restrict__ grid, const float* __restrict__ tmp,
                                                       float* __restrict__ partial) {
	__shared__ float sh[256];
	if (blockIdx.x >= 512) {
		const uint32_t i = GRID_N_CELLS + (blockIdx.x - 512) * 256 + threadIdx.x;
		if (i >= n) return;
		const float prev = grid[i];
		grid[i] = prev < 0.f ? prev : fmaxf(prev * decay, tmp[i]);
		return;
	}
	const uint32_t per_block = GRID_N_CELLS / 512;
	const uint32_t base = blockIdx.x * per_block;
	float acc = 0.f;
	for (uint32_t k = threadIdx.x; k < per_block; k += 256) {
		const float prev = grid[base + k];
		const float v = prev < 0.f ? prev : fmaxf(prev * decay, tmp[base + k]);
		grid[base + k] = v;
		acc += fmaxf(v, 0.f) / (float)GRID_N_CELLS;
	}
	sh[threadIdx.x] = acc;
	__syncthreads();
	for (uint32_t off = 128; off > 0; off >>= 1) {
		if (threadIdx.x < off) sh[threadIdx.x] += sh[threadIdx.x + off];
		__syncthreads();
	}
	if (threadIdx.x == 0) partial[blockIdx.x] = sh[0];
}
__global__ void __launch_bounds__(512) k_grid_bitfield(uint32_t n_bytes, uint32_t n_nonzero, const float* __restrict__ grid,
                                                       uint8_t* __restrict__ bitfield, const float* __restrict__ partial,
                                                       float* __restrict__ mean_out) {
	__shared__ float sh[512];
	sh[threadIdx.x] = partial[threadIdx.x];
	__syncthreads();
	for (uint32_t off = 256; off > 0; off >>= 1) {
		if (threadIdx.x < off) sh[threadIdx.x] += sh[threadIdx.x + off];
		__syncthreads();
	}
	const float mean = sh[0];
	if (blockIdx.x == 0 && threadIdx.x == 0) *mean_out = mean;
	const float thresh = fminf(MIN_OPTICAL_THICKNESS, mean);
#pragma unroll
	for (uint32_t q = 0; q < 8; ++q) {
		const uint32_t i = (blockIdx.x * 8 + q) * 512 + threadIdx.x;
		if (i >= n_bytes) return;
		if (i >= n_nonzero) { bitfield[i] = 0; continue; }
		uint8_t bits = 0;
#pragma unroll
		for (uint8_t j = 0; j < 8; ++j) bits |= grid[i * 8 + j] > thresh ? ((uint8_t)1 << j) : 0;
		bitfield[i] = bits;
	}
}
__global__ void __launch_bounds__(1024) k_bitfield_pool_tail(uint32_t first, uint8_t* __restrict__ bitfield) {
	for (uint32_t m = first; m + 1 < CASCADES; ++m) {
		// mip m is zero outside cells [64 - h, 64 + h): h = 32 at m = first, halving per mip; in 4-cell blocks [lo, hi)
		const uint32_t h = 32u >> (m - first);
		const uint32_t lo = (64 - h) / 4, hi = (64 + h + 3) / 4, w = hi - lo;
		const uint8_t* prev = bitfield + (size_t)m * GRID_N_CELLS / 8;
		uint8_t* next = bitfield + (size_t)(m + 1) * GRID_N_CELLS / 8;
		for (uint32_t t = threadIdx.x; t < w * w * w; t += blockDim.x) {
			const uint32_t x = lo + t % w, y = lo + (t / w) % w, z = lo + t / (w * w);
			const uint32_t i = morton3D(x, y, z);
			uint8_t bits = 0;
#pragma unroll
			for (uint8_t j = 0; j < 8; ++j) bits |= prev[i * 8 + j] > 0 ? ((uint8_t)1 << j) : 0;
			next[morton3D(x + GRIDSIZE / 8, y + GRIDSIZE / 8, z + GRIDSIZE / 8)] |= bits;
		}
		__syncthreads();
	}
}
void grid_ema_mean_bitfield(uint32_t n_el, float decay, float* grid, const float* tmp, uint32_t max_cascade, float* mean_out,
                            uint8_t* bitfield, hipStream_t s) {
	float* partial = mean_out + 1;  // [1 + 512] floats
	k_grid_ema_mean<<<512 + div_round_up(n_el - GRID_N_CELLS, 256), 256, 0, s>>>(n_el, decay, grid, tmp, partial);
	const uint32_t n_bytes = GRID_N_CELLS / 8 * CASCADES;
	k_grid_bitfield<<<div_round_up(n_bytes, 8 * 512), 512, 0, s>>>(n_bytes, GRID_N_CELLS / 8 * (max_cascade + 1), grid, bitfield, partial,
	                                                              mean_out);
	const uint32_t full = std::min(max_cascade + 1, CASCADES - 1);  // mips 1 .. full from whole grids
	for (uint32_t level = 1; level <= full; ++level) {
		const uint32_t n = GRID_N_CELLS / 64;
		k_bitfield_max_pool<<<div_round_up(n, 256), 256, 0, s>>>(n, bitfield + (size_t)(level - 1) * GRID_N_CELLS / 8,
		                                                          bitfield + (size_t)level * GRID_N_CELLS / 8);
	}
	if (full + 1 < CASCADES) k_bitfield_pool_tail<<<1, 1024, 0, s>>>(full, bitfield);
	NGP_HIP(hipGetLastError());
}
void grid_ema(uint32_t n, float decay, float* grid, const float* tmp, hipStream_t s) {
	k_grid_ema<<<div_round_up(n, 256), 256, 0, s>>>(n, decay, grid, tmp);
	NGP_HIP(hipGetLastError());
}
void grid_mean_bitfield(const float* grid, uint32_t max_cascade, float* mean_out, uint8_t* bitfield, hipStream_t s) {
	float* partial = mean_out + 1;  // caller provides [1 + 512] floats
	k_grid_mean_partial<<<512, 256, 0, s>>>(grid, partial);
	k_grid_mean_final<<<1, 512, 0, s>>>(partial, mean_out);
	const uint32_t n_bytes = GRID_N_CELLS / 8 * CASCADES;
	k_grid_to_bitfield<<<div_round_up(n_bytes, 256), 256, 0, s>>>(n_bytes, GRID_N_CELLS / 8 * (max_cascade + 1), grid, bitfield, mean_out);
	for (uint32_t level = 1; level < CASCADES; ++level) {
		const uint32_t n = GRID_N_CELLS / 64;
		k_bitfield_max_pool<<<div_round_up(n, 256), 256, 0, s>>>(n, bitfield + (size_t)(level - 1) * GRID_N_CELLS / 8,
		                                                          bitfield + (size_t)level * GRID_N_CELLS / 8);
	}
	NGP_HIP(hipGetLastError());
}

}  // namespace nerf
}  // namespace ngp
