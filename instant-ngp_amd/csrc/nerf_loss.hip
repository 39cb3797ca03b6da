// nerf_loss.hip — the NeRF training loss for gfx950 (see nerf.h): compute_loss_kernel_train_nerf as two passes around
// a prefix scan, the error map's CDFs, and tcnn's fill_rollover.
#include <cmath>
#include <cstring>
#include <utility>

#include "nerf_device.h"
#include "profiler.h"
#include "rng.h"
#include "nerf_pixel.h"
#include "envmap.h"

namespace ngp {
namespace nerf {

constexpr uint32_t LG = 16;  // lanes per ray in the loss passes: one DPP row
#ifndef NGP_LOSS_PF
#define NGP_LOSS_PF 2  // loss pass 1: chunks of 16 samples whose loads are in flight ahead of the compositing
#endif
#ifndef NGP_LOSS_XCD
#define NGP_LOSS_XCD 1  // loss pass 1 reads its rays on the XCD that wrote their samples (k_loss_pass1)
#endif
#ifndef NGP_LOSS2_LANES
#define NGP_LOSS2_LANES 64  // loss pass 2 with pass 1's kept state: lanes per ray (k_loss_pass2)
#endif
// a ray's lanes must be one wave: lane 0 overwrites numsteps[2i + 1] after every lane has read it in the same
// wave instruction (128 or 256 lanes per ray let a second wave read the overwritten value: wrong samples)
static_assert(NGP_LOSS2_LANES >= 16 && NGP_LOSS2_LANES <= 64, "loss pass 2: at most one wave per ray");
#ifndef NGP_LOSS_SELECT
#define NGP_LOSS_SELECT 1  // loss pass 1: compositing steps committed with selects instead of branches (pass 2
                           // measured slower that way: its steps already run under a per-lane mask)
#endif
#ifndef NGP_LOSS2_PF
#define NGP_LOSS2_PF 1  // loss pass 2: depth 2 takes 86 VGPRs (5 waves/SIMD) and measured 41 -> 45 us (Lego stand-in)
#endif
template <int K> __device__ __forceinline__ float row_bcast(float v) {  // v of lane K of this row (row_newbcast)
	return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x150 + K, 0xF, 0xF, false));
}

// ------------------------------------------------------------------------------------------------
// compute_loss_kernel_train_nerf (testbed_nerf.cu:1660-2012), split at its atomicAdd into two passes
// around a prefix scan. The error map deposit (:1869-1899, always on in the reference's training) is
// done in pass 2 after the compaction early-out, as there, and so is the environment map's gradient
// deposit (:1988-2011; envmap.h), and depth supervision (:1725-1748, 1848-1856, 1912-1956;
// DESIGN.md §8e) is the kernels' DEPTH instantiation, and the per-image exposure (:1794-1818, 1973-1986)
// pass 1's EXPO instantiation, whose per-ray gradients exposure_gradients sums per image; sharpness is off in the
// reference's default training and not implemented.
// A ray owns one DPP row: lanes load and activate 16 samples at once (network output, dt, exp), and
// the compositing recurrence (T *= 1 - alpha, rgb += alpha T c) runs over the row in sample order
// with row_newbcast broadcasts, i.e. with the reference's float ops in the reference's order.
// ------------------------------------------------------------------------------------------------
struct LossRay {  // pass-1 results kept for pass 2
	float grad[3];
	float rgb_ray[3];
	float mean_loss;
	float u, v;    // the ray's image position and image (the error map deposit)
	uint32_t img;
	// with an environment map's gradient bound: the ray's fp16 dL/d(envmap rgb) (bits of halves 0|1, 2|-), valid when
	// the ray kept all of its samples; zero otherwise
	uint32_t env[2];
};

__device__ __forceinline__ V3 unwarp_pos(const float* c, const Aabb& b) {
	return v3(b.mn.x + c[0] * (b.mx.x - b.mn.x), b.mn.y + c[1] * (b.mx.y - b.mn.y), b.mn.z + c[2] * (b.mx.z - b.mn.z));
}

// distance(unwarp_position(c), ray_o): a sample's depth along its ray, one expression for both passes
__device__ __forceinline__ float sample_depth(const float* c, const Aabb& b, float ox, float oy, float oz) {
	const V3 pos = unwarp_pos(c, b);
	const float dx = pos.x - ox, dy = pos.y - oy, dz = pos.z - oz;
	return sqrtf(dx * dx + dy * dy + dz * dz);
}

// loss_and_gradient (testbed_nerf.cu:1340-1355) per channel
__device__ void loss_channel(float target, float pred, uint32_t type, float* loss, float* grad) {
	const float d = pred - target;
	switch (type) {
		case LOSS_RELL2: { const float den = pred * pred + 1e-2f; *loss = d * d / den; *grad = 2.0f * d / den; return; }
		case LOSS_L1: *loss = fabsf(d); *grad = copysignf(1.0f, d); return;
		case LOSS_MAPE: { const float den = fabsf(pred) + 1e-2f; *loss = fabsf(d) / den; *grad = copysignf(1.0f / den, d); return; }
		case LOSS_SMAPE: { const float den = 0.5f * (fabsf(pred) + fabsf(target)) + 1e-2f; *loss = fabsf(d) / den; *grad = copysignf(1.0f / den, d); return; }
		case LOSS_HUBER: {
			const float alpha = 0.1f, ad = fabsf(d), sq = 0.5f / alpha * d * d;
			*loss = (ad > alpha ? (ad - 0.5f * alpha) : sq) / 5.0f;
			*grad = (ad > alpha ? (d > 0 ? 1.0f : -1.0f) : (d / alpha)) / 5.0f;
			return;
		}
		case LOSS_LOGL1: { const float div = fabsf(d) + 1.0f; *loss = ngp_logf(div); *grad = copysignf(1.0f / div, d); return; }
		default: *loss = d * d; *grad = 2.0f * d; return;
	}
}

#define NGP_ROW_UNROLL16(M) M(0) M(1) M(2) M(3) M(4) M(5) M(6) M(7) M(8) M(9) M(10) M(11) M(12) M(13) M(14) M(15)

// ENV: an environment map is bound (LossArgs::envmap): a separate instantiation, as CDF is
// DEPTH: depth supervision is on (loss_depth_on): the lanes also load their sample's position, and the row recurrence
// carries depth_ray += weight * distance(pos, ray_o) under rgb's stop rule; the ray's sum goes to depth_ray[i]
// EXPO: per-image exposures are bound (LossArgs::exposure): lane ch scales the texel by 2^exposure[img][ch] and, with
// exposure_ray_grad bound, stores the ray's dloss_by_dexposure[ch]
// TEX: the dataset holds a Half or Float image (Dataset::tex): `pixels` is the image table, and a Half or Float texel
// is the target as it stands, linear and premultiplied: no sRGB decode, no alpha multiply (read_rgba)
template <bool CDF, bool ENV, bool DEPTH, bool EXPO, bool TEX>
__global__ void __launch_bounds__(256) k_loss_pass1(const Camera* __restrict__ cams, const void* __restrict__ pixels,
                                                    uint32_t n_images, const ngp_nerf_config cfg, LossArgs a,
                                                    uint32_t* __restrict__ craw, LossRay* __restrict__ lr,
                                                    float* __restrict__ depth_ray) {
	// XCD-aware ray order (NGP_LOSS_XCD): the block on XCD x = blockIdx % 8 takes the rays whose samples
	// k_sample_write wrote from XCD x (a wave per ray there: ray i on XCD (i / 4) % 8), so their coordinates
	// can still be in that XCD's L2: rays 128 m + 32 q + 4 x + j (q, j in 0..3) for block 8 m + x
	static_assert(!DEPTH || NGP_LOSS_SELECT, "the depth recurrence is written in the select form only");
	uint32_t i;
	const uint32_t L = threadIdx.x % LG;
	if (NGP_LOSS_XCD) {
		const uint32_t m = blockIdx.x / 8, x = blockIdx.x % 8, r = threadIdx.x / LG;
		i = 128 * m + 32 * (r / 4) + 4 * x + (r % 4);
	} else {
		i = (blockIdx.x * blockDim.x + threadIdx.x) / LG;
	}
	if (i >= a.n_rays) return;
	if (L == 0 && a.zero_loss && a.loss) a.loss[i] = 0.0f;  // pass 2 writes the compacted rays' loss after it
	if (i >= *a.ray_counter) { if (L == 0) craw[i] = 0; return; }
	const uint32_t numsteps = a.numsteps[2 * i], base = a.numsteps[2 * i + 1];
	const f16* out = a.network_output + (size_t)base * a.out_stride;
	const float* ci = a.coords_in + (size_t)base * 7;
	// target texel first (same random stream as the sampler for the same ray): its dependent chain of
	// loads (ray index -> camera -> pixel) overlaps the compositing loop instead of following it
	const uint32_t ray_idx = a.ray_indices[i];
	Rng rng = a.rng;
	pcg_advance(rng, (uint64_t)ray_idx * N_MAX_RANDOM_SAMPLES_PER_RAY);
	const TrainPixel px = training_pixel<CDF>(cams, n_images, cfg.snap_to_pixel_centers != 0, a.cdfs, ray_idx, a.n_rays_total_for_image_idx, rng);
	const uint32_t img = px.img;
	const Camera& cam = cams[img];
	const float u = px.u, v = px.v;
	pcg_advance(rng, 1);  // motionblur_time
	// The per-ray colour work (12 powf in the default configuration) is split over the row: lane ch < 3
	// finishes colour channel ch with the reference's per-channel operations, and lane 0 gathers the
	// three results (the other lanes repeat channel 2).
	const uint32_t ch = L < 3 ? L : 2;
	float bg[3] = {cfg.background_color[0], cfg.background_color[1], cfg.background_color[2]};
	if (cfg.random_bg_color) { bg[0] = pcg_float(rng); bg[1] = pcg_float(rng); bg[2] = pcg_float(rng); }
	float bgc = srgb_to_linear(ch == 0 ? bg[0] : ch == 1 ? bg[1] : bg[2]);
	// read_rgba (common_device.cuh:885-913): Byte images, or with TEX the image's own type
	uint32_t raw = 0, tex_type = IMAGE_BYTE;
	f32x4 hdr = {0.f, 0.f, 0.f, 0.f};
	if (TEX) {
		const ImageRef im = ((const ImageRef*)pixels)[img];
		const uint64_t idx = pixel_index(u, v, cam.width, cam.height);
		tex_type = im.type;
		if (tex_type == IMAGE_BYTE) raw = ((const uint32_t*)im.data)[idx];
		else hdr = read_hdr_texel(im, idx);
	} else {
		raw = ((const uint32_t*)pixels)[cam.pixel_offset + pixel_index(u, v, cam.width, cam.height)];
	}
	// the environment map's four texels in the ray's direction, loaded here for the same reason
	EnvmapTap tap;
	f32x4 e0, e1, e2, e3;
	if (ENV) {
		const float* rd = a.rays + (size_t)i * 6 + 3;
		const float dx = rd[0], dy = rd[1], dz = rd[2];
		const float inv = 1.0f / sqrtf(dx * dx + dy * dy + dz * dz);
		tap = envmap_lookup(a.env_w, a.env_h, dx * inv, dy * inv, dz * inv);
		const f32x4* em = (const f32x4*)a.envmap;
		e0 = em[tap.idx[0]]; e1 = em[tap.idx[1]]; e2 = em[tap.idx[2]]; e3 = em[tap.idx[3]];
	}
	float t = 1.f;
	const float eps = 1e-4f;
	float rr = 0.f, rg = 0.f, rb = 0.f;
	float dd = 0.f;  // DEPTH: depth_ray
	uint32_t cn = 0;
	bool stop = false;
	const bool keep_state = NGP_LOSS_SELECT && a.state != nullptr;
	Aabb box;
	float ro0 = 0.f, ro1 = 0.f, ro2 = 0.f;
	float pb[NGP_LOSS_PF][3];
	if (DEPTH) {
		box = cfg_aabb(cfg);
		const float* ro = a.rays + (size_t)i * 6;
		ro0 = ro[0]; ro1 = ro[1]; ro2 = ro[2];
	}
	// software pipelining: the loads of the next NGP_LOSS_PF chunks are in flight while a chunk's
	// compositing chain runs (the chunk loop is unrolled by the depth, so every buffer keeps its registers)
	f16x4 ob[NGP_LOSS_PF];
	float db[NGP_LOSS_PF];
#pragma unroll
	for (uint32_t d = 0; d < NGP_LOSS_PF; ++d) {
		ob[d] = f16x4{(f16)0.f, (f16)0.f, (f16)0.f, (f16)0.f};
		db[d] = 0.f;
		if (DEPTH) pb[d][0] = pb[d][1] = pb[d][2] = 0.f;
		if (L + d * LG < numsteps) {
			ob[d] = *(const f16x4*)(out + (size_t)(L + d * LG) * a.out_stride);
			db[d] = ci[(size_t)(L + d * LG) * 7 + 3];
			if (DEPTH) {
#pragma unroll
				for (int k = 0; k < 3; ++k) pb[d][k] = ci[(size_t)(L + d * LG) * 7 + k];
			}
		}
	}
	for (uint32_t c0 = 0; c0 < numsteps && !stop; c0 += NGP_LOSS_PF * LG)
#pragma unroll
	for (uint32_t d = 0; d < NGP_LOSS_PF; ++d) {
		const uint32_t c = c0 + d * LG;
		if (c >= numsteps || stop) break;
		const uint32_t jj = c + L;
		const f16x4 o = ob[d];
		const float dtw = db[d];
		float pc[3] = {0.f, 0.f, 0.f};
		if (DEPTH) { pc[0] = pb[d][0]; pc[1] = pb[d][1]; pc[2] = pb[d][2]; }
		if (jj + NGP_LOSS_PF * LG < numsteps) {
			ob[d] = *(const f16x4*)(out + (size_t)(jj + NGP_LOSS_PF * LG) * a.out_stride);
			db[d] = ci[(size_t)(jj + NGP_LOSS_PF * LG) * 7 + 3];
			if (DEPTH) {
#pragma unroll
				for (int k = 0; k < 3; ++k) pb[d][k] = ci[(size_t)(jj + NGP_LOSS_PF * LG) * 7 + k];
			}
		}
		float alpha = 0.f, cr = 0.f, cg = 0.f, cb = 0.f, cd = 0.f;
		if (DEPTH && jj < numsteps) cd = sample_depth(pc, box, ro0, ro1, ro2);
		if (jj < numsteps) {
			const float dt = unwarp_dt(dtw);
			const float density = network_to_density((float)o[3], cfg.density_activation);
			alpha = 1.f - ngp_expf_fast(-density * dt);
			cr = network_to_rgb((float)o[0], cfg.rgb_activation);
			cg = network_to_rgb((float)o[1], cfg.rgb_activation);
			cb = network_to_rgb((float)o[2], cfg.rgb_activation);
		}
#if NGP_LOSS_SELECT
		// branch-free step: the same operations, committed with selects (no exec-mask branch per sample)
#define NGP_LOSS1_STEP(K)                                                                              \
		{                                                                                              \
			const float ak = row_bcast<K>(alpha), rk = row_bcast<K>(cr), gk = row_bcast<K>(cg), bk = row_bcast<K>(cb); \
			const bool act = !stop && c + K < numsteps;                                                \
			const bool low = t < eps;                                                                  \
			stop = stop || (act && low);                                                               \
			const bool upd = act && !low;                                                              \
			const float weight = ak * t;                                                               \
			const float nr = rr + weight * rk, ng = rg + weight * gk, nb = rb + weight * bk;           \
			const float nt = t * (1.f - ak);                                                           \
			rr = upd ? nr : rr; rg = upd ? ng : rg; rb = upd ? nb : rb; t = upd ? nt : t;              \
			cn += upd ? 1u : 0u;                                                                       \
			if (keep_state && L == K) { sw = weight; sT = nt; sr = nr; sg = ng; sb = nb; su = upd; }   \
			if (DEPTH) {                                                                               \
				const float nd = dd + weight * row_bcast<K>(cd);                                       \
				dd = upd ? nd : dd;                                                                    \
				if (keep_state && L == K) sd = nd;                                                     \
			}                                                                                          \
		}
#else
#define NGP_LOSS1_STEP(K)                                                                              \
		{                                                                                              \
			const float ak = row_bcast<K>(alpha), rk = row_bcast<K>(cr), gk = row_bcast<K>(cg), bk = row_bcast<K>(cb); \
			if (!stop && c + K < numsteps) {                                                           \
				if (t < eps) stop = true;                                                              \
				else {                                                                                 \
					const float weight = ak * t;                                                       \
					rr += weight * rk; rg += weight * gk; rb += weight * bk;                           \
					t *= (1.f - ak);                                                                   \
					++cn;                                                                              \
				}                                                                                      \
			}                                                                                          \
		}
#endif
		float sw = 0.f, sT = 0.f, sr = 0.f, sg = 0.f, sb = 0.f, sd = 0.f;
		bool su = false;
		NGP_ROW_UNROLL16(NGP_LOSS1_STEP)
#undef NGP_LOSS1_STEP
		if (keep_state && su && (size_t)base + jj < a.state_cap) {  // composited: pass 2 reads its state instead of compositing again
			const size_t si = (size_t)base + jj;
			a.state[si] = sw; a.state[a.state_cap + si] = sT;
			a.state[2 * a.state_cap + si] = sr; a.state[3 * a.state_cap + si] = sg; a.state[4 * a.state_cap + si] = sb;
			if (DEPTH) a.state[5 * a.state_cap + si] = sd;
		}
	}
	// channel ch of the target, the background and the loss (every lane of the row holds rr, rg, rb, t, cn)
	float texc, tex3;
	if (TEX && tex_type != IMAGE_BYTE) { texc = ch == 0 ? hdr[0] : ch == 1 ? hdr[1] : hdr[2]; tex3 = hdr[3]; }
	else if (raw == 0x00FF00FFu) { texc = tex3 = -1.0f; }
	else {
		const float alpha = (float)(raw >> 24) * (1.0f / 255.0f);
		texc = srgb_to_linear((float)((raw >> (8 * ch)) & 0xff) * (1.0f / 255.0f)) * alpha;
		tex3 = alpha;
	}
	if (ENV) {  // the background behind the map's (testbed_nerf.cu:1787-1792), before the target and the prediction use it
		const float ec = envmap_mix(tap, e0[ch], e1[ch], e2[ch], e3[ch]), ea = envmap_mix(tap, e0[3], e1[3], e2[3], e3[3]);
		bgc = ec + bgc * (1.0f - ea);
	}
	const float exposure_scale = expf(0.6931471805599453f * (EXPO ? a.exposure[3 * (size_t)img + ch] : 0.0f));
	float target;
	if (cfg.linear_colors || cfg.color_space_linear) {
		target = exposure_scale * texc + (1.0f - tex3) * bgc;
		if (!cfg.linear_colors) { target = linear_to_srgb(target); bgc = linear_to_srgb(bgc); }
	} else {
		bgc = linear_to_srgb(bgc);
		target = tex3 > 0 ? linear_to_srgb(exposure_scale * texc / tex3) * tex3 + (1.0f - tex3) * bgc : bgc;
	}
	float pred = ch == 0 ? rr : ch == 1 ? rg : rb;
	if (cn == numsteps) pred += t * bgc;
	float lc, gc;
	loss_channel(target, pred, cfg.loss_type, &lc, &gc);
	// lg.loss /= img_pdf * uv_pdf (testbed_nerf.cu:1846): the reported loss and the error map deposit. The gradient is
	// NOT divided: the reference leaves that line commented out on purpose (:1858-1862). Dividing it would make the
	// loss estimate unbiased, the same optimisation with less variance; importance sampling is meant to change the
	// weighting of the loss instead.
	if (CDF) lc = lc / (px.img_pdf * px.uv_pdf);
	// dloss_by_dexposure of channel ch (testbed_nerf.cu:1973-1986): -gradient / uv_pdf, through the sRGB curve at the
	// target when not training in linear colours, times loss_scale * 2^exposure * ln 2. It lacks the texel's own value
	// (d target / d exposure = ln 2 * 2^exposure * texel), as there. Which rays count is decided after the compaction
	// (exposure_gradients).
	if (EXPO && a.exposure_ray_grad && L < 3) {
		float dgt = -gc;
		if (CDF) dgt = dgt / px.uv_pdf;
		if (!cfg.linear_colors) dgt = dgt / srgb_to_linear_derivative(target);
		a.exposure_ray_grad[3 * (size_t)i + L] = (a.loss_scale / (float)a.n_rays) * dgt * exposure_scale * 0.6931471805599453f;
	}
	const float l1 = row_bcast<1>(lc), l2 = row_bcast<2>(lc), g1 = row_bcast<1>(gc), g2 = row_bcast<2>(gc);
	const float p1 = row_bcast<1>(pred), p2 = row_bcast<2>(pred);
	// dL/d(envmap) of channel ch (testbed_nerf.cu:1988-2002): the map's own loss where it differs, times the
	// transmittance left, through the sRGB curve when not training in linear colours, rounded to fp16
	uint32_t eh0 = 0, eh1 = 0, eh2 = 0;
	if (ENV) {
		if (a.env_acc && cn == numsteps) {
			float ge = gc;
			if (a.env_loss_type != cfg.loss_type) { float le; loss_channel(target, pred, a.env_loss_type, &le, &ge); }
			float dbg = t * ge;
			if (!cfg.linear_colors) dbg = dbg / srgb_to_linear_derivative(bgc);
			const f16 hv = (f16)((a.loss_scale / (float)a.n_rays) * dbg);
			eh0 = (uint32_t)__builtin_bit_cast(uint16_t, hv);
		}
		eh1 = __float_as_uint(row_bcast<1>(__uint_as_float(eh0)));
		eh2 = __float_as_uint(row_bcast<2>(__uint_as_float(eh0)));
	}
	if (L != 0) return;
	craw[i] = cn;
	LossRay q;
	q.mean_loss = (lc + l1 + l2) / 3.0f;
	q.grad[0] = gc; q.grad[1] = g1; q.grad[2] = g2;
	q.rgb_ray[0] = pred; q.rgb_ray[1] = p1; q.rgb_ray[2] = p2;
	q.u = u; q.v = v; q.img = img;
	q.env[0] = eh0 | (eh1 << 16); q.env[1] = eh2;
	lr[i] = q;
	if (DEPTH) depth_ray[i] = dd;  // the background adds nothing to it
}

// error map deposit of one compacted ray (testbed_nerf.cu:1869-1899 without the sharpness factor,
// include_sharpness_in_error is off by default): mean loss split bilinearly over the 4 texels around
// uv * res - 0.5, float atomics as in the reference (the map only steers importance sampling)
__device__ __forceinline__ void deposit_error(const LossArgs& a, const Camera* __restrict__ cams, const LossRay& q) {
	const float rx = (float)a.em_w, ry = (float)a.em_h;
	const float px = fminf(fmaxf(q.u * rx - 0.5f, 0.0f), rx - (1.0f + 1e-4f));
	const float py = fminf(fmaxf(q.v * ry - 0.5f, 0.0f), ry - (1.0f + 1e-4f));
	const int ix0 = (int)px, iy0 = (int)py;
	const float wx = px - (float)ix0, wy = py - (float)iy0;
	// clamp(pos_int, 0, resolution - 2) with the image's resolution, as the reference writes it
	const int ix = min(max(ix0, 0), (int)cams[q.img].width - 2), iy = min(max(iy0, 0), (int)cams[q.img].height - 2);
	float* em = a.error_map + (size_t)q.img * a.em_w * a.em_h;
	const float ml = q.mean_loss;
	atomicAdd(em + (size_t)iy * a.em_w + ix, (1 - wx) * (1 - wy) * ml);
	atomicAdd(em + (size_t)iy * a.em_w + ix + 1, wx * (1 - wy) * ml);
	atomicAdd(em + (size_t)(iy + 1) * a.em_w + ix, (1 - wx) * wy * ml);
	atomicAdd(em + (size_t)(iy + 1) * a.em_w + ix + 1, wx * wy * ml);
}

// LANES per ray: LG (one DPP row) when pass 2 composites again; a whole wave when it reads pass 1's kept state,
// where the samples are independent: a ray's samples then take ceil(cn / 64) rounds of loads instead of
// ceil(cn / 16), and the long rays, each round a memory latency, set the kernel's time (fox: up to ~26 rounds)
// ENV: an environment map's gradient accumulator is bound (LossArgs::env_acc): lane 0 deposits the ray's gradient
// DEPTH: depth supervision (loss_depth_on): every lane works out the ray's depth_loss_gradient from pass 1's depth_ray
// and the target texel's depth (depth_imgs: the dataset's per-image pointers), after the compaction early-out as in the
// reference, and each sample's density gradient takes depth_loss_gradient * (T depth - depth suffix) in all three forms
template <uint32_t LANES, bool ENV, bool DEPTH>
__global__ void __launch_bounds__(256) k_loss_pass2(const Camera* __restrict__ cams, const ngp_nerf_config cfg, LossArgs a,
                                                    const uint32_t* __restrict__ craw, const uint32_t* __restrict__ gpre,
                                                    const LossRay* __restrict__ lr, const float* __restrict__ depth_ray_in,
                                                    const float* const* __restrict__ depth_imgs) {
	const uint32_t gid = blockIdx.x * blockDim.x + threadIdx.x;
	const uint32_t i = gid / LANES, L = gid % LANES;
	if (i >= a.n_rays || i >= *a.ray_counter) return;
	const uint32_t base = a.numsteps[2 * i + 1];
	uint32_t numsteps = 0;  // the sampler's count, read by every lane before lane 0 overwrites it below
	if (ENV) numsteps = a.numsteps[2 * i];
	// the exclusive prefix of the compacted counts: the ray's group of 4 (k_scan4) plus the rays of the group before it
	uint32_t compacted_base = gpre[i / 4];
	for (uint32_t r = i & ~3u; r < i; ++r) compacted_base += craw[r];
	const uint32_t mx = a.max_samples_compacted;
	const uint32_t cn = min(mx - min(mx, compacted_base), craw[i]);
	if (L == 0) {  // every lane of the row has read numsteps[2i + 1] above (one wave instruction)
		a.numsteps[2 * i] = cn;
		a.numsteps[2 * i + 1] = compacted_base;
	}
	if (cn == 0) return;
	const LossRay q = lr[i];
	if (L == 0 && a.loss) a.loss[i] = q.mean_loss / (float)a.n_rays;  // written after the compaction early-out (:1836-1866)
	if (L == 0 && a.error_map) deposit_error(a, cams, q);
	// the map's gradient, after the compaction early-out and only from rays that kept every sample (:1836, :1988):
	// a ray cut short by the compacted budget deposits nothing, as there
	if (ENV && L == 0 && cn == numsteps) {
		const float* rd = a.rays + (size_t)i * 6 + 3;
		const float dx = rd[0], dy = rd[1], dz = rd[2];
		const float inv = 1.0f / sqrtf(dx * dx + dy * dy + dz * dz);
		const EnvmapTap tap = envmap_lookup(a.env_w, a.env_h, dx * inv, dy * inv, dz * inv);
		envmap_deposit(a.env_acc, (size_t)a.env_w * a.env_h * 4, tap, __builtin_bit_cast(f16, (uint16_t)(q.env[0] & 0xffffu)),
		               __builtin_bit_cast(f16, (uint16_t)(q.env[0] >> 16)), __builtin_bit_cast(f16, (uint16_t)(q.env[1] & 0xffffu)));
	}
	const float loss_scale = a.loss_scale / (float)a.n_rays;
	const float output_l2_reg = cfg.rgb_activation == ACT_EXP ? 1e-4f : 0.0f;
	const float output_l1_reg_density = *a.mean_density < MIN_OPTICAL_THICKNESS ? 1e-4f : 0.0f;
	const Aabb box = cfg_aabb(cfg);
	const float* ray = a.rays + (size_t)i * 6;
	const float ro0 = ray[0], ro1 = ray[1], ro2 = ray[2];
	const f16* out = a.network_output + (size_t)base * a.out_stride;
	const float* ci = a.coords_in + (size_t)base * 7;
	float* co = a.coords_out + (size_t)compacted_base * 7;
	f16* dl = a.dloss_doutput + (size_t)compacted_base * 16;
	// target_depth, lg_depth and depth_loss_gradient (testbed_nerf.cu:1848-1856); the depth term enters neither loss[]
	// nor the error map deposit
	float depth_ray = 0.f, depth_loss_gradient = 0.f;
	if (DEPTH) {
		depth_ray = depth_ray_in[i];
		const float d0 = ray[3], d1 = ray[4], d2 = ray[5];
		const float* dimg = depth_imgs[q.img];
		const Camera& cam = cams[q.img];
		const float target_depth = sqrtf(d0 * d0 + d1 * d1 + d2 * d2) *
		                           (a.depth_lambda > 0.0f && dimg ? dimg[pixel_index(q.u, q.v, cam.width, cam.height)] : -1.0f);
		float ld, gd;
		loss_channel(target_depth, depth_ray, a.depth_loss_type, &ld, &gd);
		depth_loss_gradient = target_depth > 0.0f ? a.depth_lambda * gd : 0.0f;
	}
	// the gradient of compacted sample jj (cc its coordinates, o its network output, its weight my_w, the
	// transmittance after it my_t and the rgb prefix through it my_r2), written with its coordinates
	// my_d2 (DEPTH): the depth prefix through the sample
	auto emit = [&](uint32_t jj, const float (&cc)[7], const f16x4& o, const float (&rgb)[3], float dt, float my_w, float my_t,
	                const float (&my_r2)[3], float my_d2) __attribute__((always_inline)) {
#pragma unroll
		for (int k = 0; k < 7; ++k) co[(size_t)jj * 7 + k] = cc[k];
		const V3 pos = unwarp_pos(cc, box);
		const float ddx = pos.x - ro0, ddy = pos.y - ro1, ddz = pos.z - ro2;
		const float depth = sqrtf(ddx * ddx + ddy * ddy + ddz * ddz);
		float depth_supervision = 0.0f;
		if (DEPTH) {
			const float depth_suffix = depth_ray - my_d2;
			depth_supervision = depth_loss_gradient * (my_t * depth - depth_suffix);
		}
		float suffix[3];
		for (int k = 0; k < 3; ++k) suffix[k] = q.rgb_ray[k] - my_r2[k];
		f16x4 g;
		for (int k = 0; k < 3; ++k) {
			const float dloss_by_drgb = my_w * q.grad[k];
			g[k] = (f16)(loss_scale * (dloss_by_drgb * network_to_rgb_derivative((float)o[k], cfg.rgb_activation) +
			                           fmaxf(0.0f, output_l2_reg * (float)o[k])));
		}
		const float density_derivative = network_to_density_derivative((float)o[3], cfg.density_activation);
		const float dotv = q.grad[0] * (my_t * rgb[0] - suffix[0]) + q.grad[1] * (my_t * rgb[1] - suffix[1]) +
		                   q.grad[2] * (my_t * rgb[2] - suffix[2]);
		const float dloss_by_dmlp = density_derivative * (dt * (dotv + depth_supervision));
		const float o3 = (float)o[3];
		g[3] = (f16)(loss_scale * dloss_by_dmlp + (o3 < 0.0f ? -output_l1_reg_density : 0.0f) +
		             (o3 > -10.0f && depth < cfg.near_distance ? 1e-4f : 0.0f));
		*(f16x4*)(dl + (size_t)jj * 16) = g;
	};
	if (LANES != LG || a.state) {  // pass 1 kept every composited sample's state: no sequential compositing here
		if ((size_t)base + cn <= a.state_cap) {
			for (uint32_t jj = L; jj < cn; jj += LANES) {
				float cc[7];
#pragma unroll
				for (int k = 0; k < 7; ++k) cc[k] = ci[(size_t)jj * 7 + k];
				const f16x4 o = *(const f16x4*)(out + (size_t)jj * a.out_stride);
				const size_t si = (size_t)base + jj;
				const float my_w = a.state[si], my_t = a.state[a.state_cap + si];
				const float my_r2[3] = {a.state[2 * a.state_cap + si], a.state[3 * a.state_cap + si], a.state[4 * a.state_cap + si]};
				float rgb[3];
				for (int k = 0; k < 3; ++k) rgb[k] = network_to_rgb((float)o[k], cfg.rgb_activation);
				emit(jj, cc, o, rgb, unwarp_dt(cc[3]), my_w, my_t, my_r2, DEPTH ? a.state[5 * a.state_cap + si] : 0.0f);
			}
			return;
		}
		// the ray's samples reach past the caller's state capacity (pass 1 kept no state there): every lane
		// composites the ray in sample order itself, with pass 1's operations, and emits its own samples
		float t = 1.f, r2[3] = {0.f, 0.f, 0.f}, d2 = 0.f;
		for (uint32_t jj = 0; jj < cn; ++jj) {
			float cc[7];
#pragma unroll
			for (int k = 0; k < 7; ++k) cc[k] = ci[(size_t)jj * 7 + k];
			const f16x4 o = *(const f16x4*)(out + (size_t)jj * a.out_stride);
			float rgb[3];
			for (int k = 0; k < 3; ++k) rgb[k] = network_to_rgb((float)o[k], cfg.rgb_activation);
			const float dt = unwarp_dt(cc[3]);
			const float alpha = 1.f - ngp_expf_fast(-network_to_density((float)o[3], cfg.density_activation) * dt);
			const float weight = alpha * t;
			r2[0] = r2[0] + weight * rgb[0]; r2[1] = r2[1] + weight * rgb[1]; r2[2] = r2[2] + weight * rgb[2];
			if (DEPTH) d2 = d2 + weight * sample_depth(cc, box, ro0, ro1, ro2);
			t = t * (1.f - alpha);
			if (jj % LANES == L) emit(jj, cc, o, rgb, dt, weight, t, r2, d2);
		}
		return;
	}
	if constexpr (LANES == LG) {
	float r2[3] = {0.f, 0.f, 0.f}, d2 = 0.f;
	float t = 1.0f;
	// software pipelining as in pass 1: NGP_LOSS2_PF chunks' loads in flight ahead of the compositing
	float cb[NGP_LOSS2_PF][7];
	f16x4 ob[NGP_LOSS2_PF];
#pragma unroll
	for (uint32_t d = 0; d < NGP_LOSS2_PF; ++d) {
		ob[d] = f16x4{(f16)0.f, (f16)0.f, (f16)0.f, (f16)0.f};
#pragma unroll
		for (int k = 0; k < 7; ++k) cb[d][k] = 0.f;
		if (L + d * LG < cn) {
#pragma unroll
			for (int k = 0; k < 7; ++k) cb[d][k] = ci[(size_t)(L + d * LG) * 7 + k];
			ob[d] = *(const f16x4*)(out + (size_t)(L + d * LG) * a.out_stride);
		}
	}
	for (uint32_t cq = 0; cq < cn; cq += NGP_LOSS2_PF * LG)
#pragma unroll
	for (uint32_t d = 0; d < NGP_LOSS2_PF; ++d) {
		const uint32_t c0 = cq + d * LG;
		if (c0 >= cn) break;
		const uint32_t jj = c0 + L;
		const bool valid = jj < cn;
		float cc[7];
#pragma unroll
		for (int k = 0; k < 7; ++k) cc[k] = cb[d][k];
		const f16x4 o = ob[d];
		if (jj + NGP_LOSS2_PF * LG < cn) {
#pragma unroll
			for (int k = 0; k < 7; ++k) cb[d][k] = ci[(size_t)(jj + NGP_LOSS2_PF * LG) * 7 + k];
			ob[d] = *(const f16x4*)(out + (size_t)(jj + NGP_LOSS2_PF * LG) * a.out_stride);
		}
		float rgb[3] = {0.f, 0.f, 0.f}, alpha = 0.f, dt = 0.f, cd = 0.f;
		if (DEPTH && valid) cd = sample_depth(cc, box, ro0, ro1, ro2);
		if (valid) {
			for (int k = 0; k < 3; ++k) rgb[k] = network_to_rgb((float)o[k], cfg.rgb_activation);
			dt = unwarp_dt(cc[3]);
			const float density = network_to_density((float)o[3], cfg.density_activation);
			alpha = 1.f - ngp_expf_fast(-density * dt);
		}
		// compositing in sample order; lane L stops after its own sample, so it ends with its weight, the
		// transmittance after it and the rgb prefix through it; the chunk's totals come from lane 15
		float my_w = 0.f;
#define NGP_LOSS2_STEP(K)                                                                              \
		{                                                                                              \
			const float ak = row_bcast<K>(alpha), rk = row_bcast<K>(rgb[0]), gk = row_bcast<K>(rgb[1]), bk = row_bcast<K>(rgb[2]); \
			const float dk = DEPTH ? row_bcast<K>(cd) : 0.0f;                                              \
			if (c0 + K < cn && K <= L) {                                                               \
				const float weight = ak * t;                                                           \
				r2[0] += weight * rk; r2[1] += weight * gk; r2[2] += weight * bk;                      \
				if (DEPTH) d2 += weight * dk;                                                          \
				t *= (1.0f - ak);                                                                      \
				my_w = weight;                                                                         \
			}                                                                                          \
		}
		NGP_ROW_UNROLL16(NGP_LOSS2_STEP)
#undef NGP_LOSS2_STEP
		const float my_t = t, my_r2[3] = {r2[0], r2[1], r2[2]}, my_d2 = d2;
		t = row_bcast<15>(t);  // a next chunk exists only if this one is full: lane 15 then took all 16 samples
		r2[0] = row_bcast<15>(r2[0]); r2[1] = row_bcast<15>(r2[1]); r2[2] = row_bcast<15>(r2[2]);
		if (DEPTH) d2 = row_bcast<15>(d2);
		if (!valid) continue;
		emit(jj, cc, o, rgb, dt, my_w, my_t, my_r2, my_d2);
	}
	}
}

// Exclusive prefix sums of the sums of groups of 4 consecutive values (gpre[g] = in[0] + .. + in[4 g - 1]) and the
// total, one block: a quarter of the block scans of a per-element scan (the loss's compaction: ~32 K rays, two
// tiles instead of eight); a consumer adds the at most 3 values of its group before it.
__global__ void __launch_bounds__(SCAN1_THREADS) k_scan4(uint32_t n, const uint32_t* __restrict__ in, uint32_t* __restrict__ gpre,
                                                         uint32_t* __restrict__ total, const uint32_t* __restrict__ ray_counter,
                                                         volatile uint32_t* pub_host, uint32_t pub_seq) {
	__shared__ uint32_t lds[32];
	const uint32_t ng = (n + 3) / 4;
	uint32_t run = 0;
	for (uint32_t g0 = 0; g0 < ng; g0 += SCAN1_TILE) {
		uint32_t gs[4];
#pragma unroll
		for (uint32_t k = 0; k < 4; ++k) {
			uint32_t v[4];
			scan1_load(in, n, 4 * (g0 + 4 * threadIdx.x + k), v);
			gs[k] = v[0] + v[1] + v[2] + v[3];
		}
		uint32_t tot;
		uint32_t b = run + block_exclusive_sum(gs[0] + gs[1] + gs[2] + gs[3], lds, &tot);
		uint32_t o[4];
#pragma unroll
		for (uint32_t k = 0; k < 4; ++k) {
			o[k] = b;
			b += gs[k];
		}
		scan1_store(gpre, ng, g0 + 4 * threadIdx.x, o);
		run += tot;
	}
	if (threadIdx.x == 0) {
		*total = run;
		if (pub_host) {  // LossArgs::pub_host: the step's counters are final here
			pub_host[0] = ray_counter[0]; pub_host[1] = ray_counter[1]; pub_host[2] = run; pub_host[3] = 0u;
			__threadfence_system();
			pub_host[4] = pub_seq;
		}
	}
}

size_t loss_tmp_f32(uint32_t n_rays) { return (size_t)n_rays * (sizeof(LossRay) / 4); }
// depth_ray, one float per ray after the LossRay array: LossRay and the default path's scratch keep their size
size_t loss_tmp_f32_depth(uint32_t n_rays) { return loss_tmp_f32(n_rays) + n_rays; }
size_t loss_tmp_f32_exposure(uint32_t n_rays) { return (size_t)n_rays * 3; }

// k_loss_pass1's 32 instantiations by their switches. Bit 0: CDF (a.cdfs.any()), bit 1: ENV (a.envmap), bit 2: DEPTH
// (loss_depth_on), bit 3: EXPO (a.exposure), bit 4: TEX (Dataset::tex: the image table instead of the packed buffer).
using LossPass1 = void (*)(const Camera*, const void*, uint32_t, const ngp_nerf_config, LossArgs, uint32_t*, LossRay*, float*);
template <size_t... I>
static LossPass1 loss_pass1_kernel(uint32_t i, std::index_sequence<I...>) {
	static const LossPass1 k[] = {k_loss_pass1<(I & 1) != 0, (I & 2) != 0, (I & 4) != 0, (I & 8) != 0, (I & 16) != 0>...};
	return k[i];
}
static LossPass1 loss_pass1_kernel(bool cdf, bool env, bool depth, bool expo, bool tex) {
	return loss_pass1_kernel((cdf ? 1u : 0u) | (env ? 2u : 0u) | (depth ? 4u : 0u) | (expo ? 8u : 0u) | (tex ? 16u : 0u),
	                         std::make_index_sequence<32>{});
}
// k_loss_pass2's 8 instantiations. Bit 0: ENV (a.env_acc: the gradient accumulator, not the map), bit 1: DEPTH, bit 2:
// pass 1's kept state is bound (a.state): NGP_LOSS2_LANES lanes per ray, a wave; otherwise LG.
using LossPass2 = void (*)(const Camera*, const ngp_nerf_config, LossArgs, const uint32_t*, const uint32_t*, const LossRay*, const float*,
                           const float* const*);
template <size_t... I>
static LossPass2 loss_pass2_kernel(uint32_t i, std::index_sequence<I...>) {
	static const LossPass2 k[] = {k_loss_pass2<(I & 4) ? NGP_LOSS2_LANES : LG, (I & 1) != 0, (I & 2) != 0>...};
	return k[i];
}
static LossPass2 loss_pass2_kernel(bool env_acc, bool depth, bool state) {
	return loss_pass2_kernel((env_acc ? 1u : 0u) | (depth ? 2u : 0u) | (state ? 4u : 0u), std::make_index_sequence<8>{});
}

bool loss_depth_on(const Dataset& ds, const LossArgs& a) { return a.depth_lambda > 0.0f && ds.n_depth > 0 && ds.d_depth != nullptr; }

void compute_loss(const Dataset& ds, const ngp_nerf_config& cfg, const LossArgs& a, uint32_t* tmp, float* tmpf, hipStream_t s) {
	if (a.n_rays == 0) return;
	uint32_t* craw = tmp;
	uint32_t* gpre = tmp + a.n_rays;  // per group of 4 rays
	LossRay* lr = (LossRay*)tmpf;
	// depth supervision: the kernels' DEPTH instantiations, and one more float per ray behind the LossRay array (tmpf
	// then holds loss_tmp_f32_depth floats); off: the launches and bytes written are those of a build without it
	const bool depth_on = loss_depth_on(ds, a);
	float* depth_ray = depth_on ? tmpf + loss_tmp_f32(a.n_rays) : nullptr;
	const float* const* dimgs = depth_on ? ds.d_depth : nullptr;
	const uint32_t blocks = div_round_up((size_t)a.n_rays * LG, 256);
	{
		ProfScope ps("loss_pass1", s);
		static_assert(256 / LG == 16, "k_loss_pass1's XCD-aware order assumes 16 rays per block");
		const uint32_t b1 = NGP_LOSS_XCD ? 8 * div_round_up(a.n_rays, 128) : blocks;
		NGP_CHECK(!a.envmap || (a.env_w > 0 && a.env_h > 0 && a.rays), "compute_loss: environment map without a resolution or rays");
		NGP_CHECK(!a.env_acc || a.envmap, "compute_loss: an environment map gradient needs the map");
		NGP_CHECK(!a.exposure_ray_grad || a.exposure, "compute_loss: an exposure gradient needs the exposures");
		if (depth_on) {
			NGP_CHECK(a.rays, "compute_loss: depth supervision needs the rays");
			NGP_CHECK(a.depth_loss_type <= LOSS_RELL2, "compute_loss: unknown depth loss");
		}
		// a Half or Float image in the dataset: the TEX forms read the image table instead of the packed buffer
		const bool tex = ds.tex();
		const LossPass1 pass1 = loss_pass1_kernel(a.cdfs.any(), a.envmap != nullptr, depth_on, a.exposure != nullptr, tex);
		const void* pixels = tex ? (const void*)ds.d_images : (const void*)ds.d_pixels;
		pass1<<<b1, 256, 0, s>>>(ds.d_cams, pixels, ds.n_images, cfg, a, craw, lr, depth_ray);
		NGP_HIP(hipGetLastError());
	}
	{
		ProfScope ps("loss_scan", s);
		k_scan4<<<1, SCAN1_THREADS, 0, s>>>(a.n_rays, craw, gpre, a.compacted_counter, a.ray_counter, a.pub_host, a.pub_seq);
		NGP_HIP(hipGetLastError());
	}
	ProfScope ps("loss_pass2", s);
	static_assert(NGP_LOSS_SELECT, "pass 1 keeps the compositing state pass 2 reads only in its select form");
	const uint32_t lanes = a.state ? NGP_LOSS2_LANES : LG;  // a wave per ray with pass 1's kept state: see k_loss_pass2
	const LossPass2 pass2 = loss_pass2_kernel(a.env_acc != nullptr, depth_on, a.state != nullptr);
	pass2<<<div_round_up((size_t)a.n_rays * lanes, 256), 256, 0, s>>>(ds.d_cams, cfg, a, craw, gpre, lr, depth_ray, dimgs);
	NGP_HIP(hipGetLastError());
}

// construct_cdf_2d (testbed_nerf.cu:2356-2382): one thread per (image, row), running sums along x
constexpr float ERROR_MAP_MIN_PDF = 0.01f;
__global__ void k_cdf_2d(uint32_t n_images, uint32_t h, uint32_t w, const float* __restrict__ data, float* __restrict__ cdf_x_cond_y,
                         float* __restrict__ cdf_y) {
	const uint32_t y = blockIdx.x * blockDim.x + threadIdx.x, img = blockIdx.y;
	if (y >= h || img >= n_images) return;
	const size_t off = ((size_t)img * h + y) * w;
	float cum = 0.f;
	for (uint32_t x = 0; x < w; ++x) {
		cum += data[off + x] + 1e-10f;
		cdf_x_cond_y[off + x] = cum;
	}
	cdf_y[(size_t)img * h + y] = cum;
	const float norm = 1.0f / cum;  // __frcp_rn: the correctly rounded reciprocal
	for (uint32_t x = 0; x < w; ++x)
		cdf_x_cond_y[off + x] = (1.0f - ERROR_MAP_MIN_PDF) * cdf_x_cond_y[off + x] * norm + ERROR_MAP_MIN_PDF * (float)(x + 1) / (float)w;
}
// construct_cdf_1d (:2384-2410): one thread per image, running sums over the rows' totals
__global__ void k_cdf_1d(uint32_t n_images, uint32_t h, float* __restrict__ cdf_y, float* __restrict__ cdf_img) {
	const uint32_t img = blockIdx.x * blockDim.x + threadIdx.x;
	if (img >= n_images) return;
	float* c = cdf_y + (size_t)img * h;
	float cum = 0.f;
	for (uint32_t y = 0; y < h; ++y) {
		cum += c[y];
		c[y] = cum;
	}
	cdf_img[img] = cum;
	const float norm = 1.0f / cum;
	for (uint32_t y = 0; y < h; ++y) c[y] = (1.0f - ERROR_MAP_MIN_PDF) * c[y] * norm + ERROR_MAP_MIN_PDF * (float)(y + 1) / (float)h;
}

void error_map_cdfs(uint32_t n_images, uint32_t w, uint32_t h, const float* data, float* cdf_x_cond_y, float* cdf_y,
                    float* cdf_img, hipStream_t s) {
	if (!n_images || !w || !h) return;
	ProfScope ps("nerf_error_map_cdf", s);
	k_cdf_2d<<<dim3(div_round_up(h, 64u), n_images), 64, 0, s>>>(n_images, h, w, data, cdf_x_cond_y, cdf_y);
	NGP_HIP(hipGetLastError());
	k_cdf_1d<<<div_round_up(n_images, 64u), 64, 0, s>>>(n_images, h, cdf_y, cdf_img);
	NGP_HIP(hipGetLastError());
}


// ------------------------------------------------------------------------------------------------
// tcnn fill_rollover / fill_rollover_and_rescale
// ------------------------------------------------------------------------------------------------
__global__ void k_rollover_f16(uint32_t n_elements, uint32_t stride, const uint32_t* n_input_ptr, f16* data, bool rescale) {
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	const uint32_t n_in = *n_input_ptr;
	if (i < n_in * stride || i >= n_elements * stride || n_in == 0) return;
	f16 r = data[i % (n_in * stride)];
	if (rescale) r = (f16)((float)r * n_in / n_elements);
	data[i] = r;
}
__global__ void k_rollover_f32(uint32_t n_elements, uint32_t stride, const uint32_t* n_input_ptr, float* data) {
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	const uint32_t n_in = *n_input_ptr;
	if (i < n_in * stride || i >= n_elements * stride || n_in == 0) return;
	data[i] = data[i % (n_in * stride)];
}
// both rollovers of the training batch in one launch (dL/doutput rescaled, coordinates copied)
// Grid-stride over the rollover range only (a full batch leaves nothing to fill; launching one thread per
// element cost ~16 K empty blocks per step).
__global__ void k_rollover_pair(uint32_t n_elements, uint32_t stride16, uint32_t stride32, const uint32_t* n_input_ptr, f16* d16,
                                float* d32) {
	const uint32_t n_in = *n_input_ptr;
	if (n_in == 0 || n_in >= n_elements) return;
	const uint32_t lo = n_in * (stride16 < stride32 ? stride16 : stride32);
	const uint32_t hi = n_elements * (stride16 > stride32 ? stride16 : stride32);
	for (uint32_t i = lo + blockIdx.x * blockDim.x + threadIdx.x; i < hi; i += gridDim.x * blockDim.x) {
		if (i >= n_in * stride16 && i < n_elements * stride16) {
			f16 r = d16[i % (n_in * stride16)];
			r = (f16)((float)r * n_in / n_elements);
			d16[i] = r;
		}
		if (i >= n_in * stride32 && i < n_elements * stride32) d32[i] = d32[i % (n_in * stride32)];
	}
}
// k_rollover_pair plus the step's publish and control-block writes (StepPublish): two launches less per NeRF step
__global__ void k_rollover_pair_publish(uint32_t n_elements, uint32_t stride16, uint32_t stride32, const uint32_t* n_input_ptr, f16* d16,
                                        float* d32, const StepPublish pub) {
	if (blockIdx.x == 0 && threadIdx.x == 0) {
		volatile uint32_t* host = pub.host;
		if (host) {
			host[0] = pub.ctr[0]; host[1] = pub.ctr[1]; host[2] = pub.ctr[2]; host[3] = pub.ctr[3];
			__threadfence_system();
			host[4] = pub.seq;
		}
		pub.ctl[0] = pub.step;
		for (uint32_t k = 0; k < pub.cfg_words; ++k) pub.ctl[pub.cfg_off + k] = pub.cfg[k];
	}
	const uint32_t n_in = *n_input_ptr;
	if (n_in == 0 || n_in >= n_elements) return;
	const uint32_t lo = n_in * (stride16 < stride32 ? stride16 : stride32);
	const uint32_t hi = n_elements * (stride16 > stride32 ? stride16 : stride32);
	for (uint32_t i = lo + blockIdx.x * blockDim.x + threadIdx.x; i < hi; i += gridDim.x * blockDim.x) {
		if (i >= n_in * stride16 && i < n_elements * stride16) {
			f16 r = d16[i % (n_in * stride16)];
			r = (f16)((float)r * n_in / n_elements);
			d16[i] = r;
		}
		if (i >= n_in * stride32 && i < n_elements * stride32) d32[i] = d32[i % (n_in * stride32)];
	}
}
void fill_rollover_pair_publish(uint32_t n_elements, const uint32_t* n_input, f16* dloss, uint32_t stride16, float* coords,
                                uint32_t stride32, const StepPublish& pub, hipStream_t s) {
	NGP_CHECK(pub.ctl && pub.cfg_words <= 32, "rollover publish: control block and config required");
	const uint64_t n = (uint64_t)n_elements * (stride16 > stride32 ? stride16 : stride32);
	const uint32_t blocks = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(div_round_up(n, 256), 1024));
	k_rollover_pair_publish<<<blocks, 256, 0, s>>>(n_elements, stride16, stride32, n_input, dloss, coords, pub);
	NGP_HIP(hipGetLastError());
}
void fill_rollover_pair(uint32_t n_elements, const uint32_t* n_input, f16* dloss, uint32_t stride16, float* coords,
                        uint32_t stride32, hipStream_t s) {
	const uint64_t n = (uint64_t)n_elements * (stride16 > stride32 ? stride16 : stride32);
	const uint32_t blocks = (uint32_t)std::min<uint64_t>(div_round_up(n, 256), 1024);
	k_rollover_pair<<<blocks, 256, 0, s>>>(n_elements, stride16, stride32, n_input, dloss, coords);
	NGP_HIP(hipGetLastError());
}
void fill_rollover_f16(uint32_t n_elements, uint32_t stride, const uint32_t* n_input, f16* data, bool rescale, hipStream_t s) {
	k_rollover_f16<<<div_round_up((uint64_t)n_elements * stride, 256), 256, 0, s>>>(n_elements, stride, n_input, data, rescale);
	NGP_HIP(hipGetLastError());
}
void fill_rollover_f32(uint32_t n_elements, uint32_t stride, const uint32_t* n_input, float* data, hipStream_t s) {
	k_rollover_f32<<<div_round_up((uint64_t)n_elements * stride, 256), 256, 0, s>>>(n_elements, stride, n_input, data);
	NGP_HIP(hipGetLastError());
}

}  // namespace nerf
}  // namespace ngp
