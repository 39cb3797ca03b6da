// mlp_image.h — the LDS image layout of the MLP training kernels: [32 samples][W features] fp16, W = 16, 32 or 64,
// written per sample by img_store_acc / img_store_std and read back transposed (K = samples) by img_frag's two
// ds_read_b64_tr_b16 (mlp.hip). One definition for writers and readers; plain C++ (host and device), constexpr.
//
// Banking (ds_read_b64_tr_b16: bank = dword address mod 64, lanes 0-31 and 32-63 are served as two groups, 8 B per
// lane, one LDS cycle per group when no two distinct addresses share a bank): lane (g = lane >> 4, q, p) of img_frag
// reads the four features 4p.. of sample row 8g + q, then of row 8g + q + 4, in one 16-feature block. A group's 32
// lanes therefore touch 8 rows, 8 dwords each: conflict-free needs the 8 rows on 8 disjoint 8-bank windows, i.e.
// row starts that are distinct multiples of 8 dwords mod 64 (plus one common phase). No single row stride does that
// for both reads of both groups, so the image is stored by 16-feature column blocks, rows permuted:
//   sample row r = 16c + 8a + 4b + q   (c, a, b bits; q = 0..3)
//   dword offset = block * BLOCK_DWORDS + (2c + b) * OCT_DWORDS + 8 * (4a + q)  [+ feature-in-block / 2]
// The 8 rows of one read share (c, b) and run over (a, q): one octet of 8 consecutive 8-dword rows = exactly the 64
// banks.
// Stores (ds_write_b64: four groups of 16 consecutive lanes, bank = dword mod 32): the 16 lanes of a group hold the
// rows of one c and write the same 4 features of each. Octets are padded by 4 dwords, which puts the b = 1 rows 4
// banks beside the b = 0 rows, and the four 4-feature quads of a row's block are stored in the order quad ^ a,
// which separates rows a = 0 and a = 1 (32 banks apart, i.e. on the same bank for a store): 16 distinct bank pairs.
// The swap stays inside a row's 8-dword window, so the reads' banking is unchanged.
#pragma once

namespace ngp {
namespace mlp_image {

constexpr int ROWS = 32;
constexpr int OCT_DWORDS = 8 * 8 + 4;                 // 8 rows x 16 halves, + 4 dwords of padding
constexpr int BLOCK_DWORDS = 4 * OCT_DWORDS;          // one 16-feature block of all 32 rows
constexpr int BLOCK_HALVES = 2 * BLOCK_DWORDS;

// width class: an image of W halves per sample is W / 16 column blocks
constexpr bool width_ok(int w) { return w == 16 || w == 32 || w == 64; }
constexpr int image_halves(int w) { return (w / 16) * BLOCK_HALVES; }

// slot of a logical sample row inside a block (a bijection on 0..31): octet 2c + b, row 4a + q of the octet
constexpr int row_slot(int r) {
	const int c = (r >> 4) & 1, a = (r >> 3) & 1, b = (r >> 2) & 1, q = r & 3;
	return 8 * (2 * c + b) + 4 * a + q;
}
// half offset of a row's first feature within a block
constexpr int row_halves(int r) {
	const int s = row_slot(r);
	return 2 * ((s >> 3) * OCT_DWORDS + 8 * (s & 7));
}
// rows with a = 1 keep their block's quads pairwise swapped (0 <-> 1, 2 <-> 3)
constexpr bool quads_swapped(int r) {
	return (r >> 3) & 1;
}
// half offset of (sample row, feature) in an image
constexpr int offset(int r, int feat) {
	return (feat >> 4) * BLOCK_HALVES + row_halves(r) + ((feat & 15) ^ (quads_swapped(r) ? 4 : 0));
}
// half offset of the 16-byte unit that holds features feat8 .. feat8 + 7 (feat8 a multiple of 8): its two quads are
// features feat8, feat8 + 4 in this order, or the reverse where quads_swapped(r)
constexpr int offset16(int r, int feat8) { return (feat8 >> 4) * BLOCK_HALVES + row_halves(r) + (feat8 & 8); }

// img_frag's per-lane addresses: read rd (0, 1) of lane `lane`, fragment starting at feature feat0 (multiple of 16)
constexpr int frag_row(int lane, int rd) { return 8 * (lane >> 4) + ((lane & 15) >> 2) + 4 * rd; }
constexpr int frag_offset(int lane, int rd, int feat0) { return offset(frag_row(lane, rd), feat0 + 4 * (lane & 3)); }
// the second read sits at one fixed distance from the first, in every lane
constexpr int FRAG_RD1_HALVES = frag_offset(0, 1, 0) - frag_offset(0, 0, 0);
constexpr bool frag_rd1_uniform() {
	for (int lane = 0; lane < 64; ++lane)
		if (frag_offset(lane, 1, 0) - frag_offset(lane, 0, 0) != FRAG_RD1_HALVES) return false;
	return true;
}
static_assert(frag_rd1_uniform(), "img_frag adds one constant to reach its second read");

// Largest number of distinct addresses on one bank among `n` lanes accessing `dwords` dwords each at half offsets
// off[0..n), banks taken mod `banks` (1 = conflict-free).
constexpr int conflict_degree(const int* off, int n, int dwords, int banks) {
	int worst = 0;
	for (int bank = 0; bank < banks; ++bank) {
		int seen[64] = {};
		int n_seen = 0;
		for (int i = 0; i < n; ++i)
			for (int d = 0; d < dwords; ++d) {
				const int dw = off[i] / 2 + d;
				if (dw % banks != bank) continue;
				bool dup = false;
				for (int k = 0; k < n_seen; ++k) dup = dup || seen[k] == dw;
				if (!dup) seen[n_seen++] = dw;
			}
		if (n_seen > worst) worst = n_seen;
	}
	return worst;
}

// worst conflict degree of img_frag's reads over both reads, both lane groups and every fragment of a W-wide image
constexpr int read_degree(int w) {
	int worst = 0;
	for (int feat0 = 0; feat0 < w; feat0 += 16)
		for (int rd = 0; rd < 2; ++rd)
			for (int grp = 0; grp < 2; ++grp) {
				int off[32] = {};
				for (int l = 0; l < 32; ++l) off[l] = frag_offset(32 * grp + l, rd, feat0);
				const int d = conflict_degree(off, 32, 2, 64);
				if (d > worst) worst = d;
			}
	return worst;
}
// img_store_acc: lane (sample = lane & 31, h = lane >> 5) stores 8 B at features 4h and 4h + 8 of a block;
// ds_write_b64 is served in four groups of 16 consecutive lanes, bank = dword mod 32
constexpr int store_acc_degree() {
	int worst = 0;
	for (int grp = 0; grp < 4; ++grp)
		for (int k = 0; k < 2; ++k) {
			int off[16] = {};
			for (int l = 0; l < 16; ++l) off[l] = offset((16 * grp + l) & 31, 4 * (grp >> 1) + 8 * k);
			const int d = conflict_degree(off, 16, 2, 32);
			if (d > worst) worst = d;
		}
	return worst;
}
// img_store_std: 16 B at features 8h .. 8h + 7 of a block; ds_write_b128 is served in eight groups of 8 consecutive lanes
constexpr int store_std_degree() {
	int worst = 0;
	for (int grp = 0; grp < 8; ++grp) {
		int off[8] = {};
		for (int l = 0; l < 8; ++l) off[l] = offset16((8 * grp + l) & 31, 8 * (grp >> 2));
		const int d = conflict_degree(off, 8, 4, 32);
		if (d > worst) worst = d;
	}
	return worst;
}

static_assert(read_degree(16) == 1 && read_degree(32) == 1 && read_degree(64) == 1,
              "img_frag: both transposed reads of both lane groups must be bank-conflict-free at every image width");
static_assert(store_acc_degree() == 1, "img_store_acc: 8-byte stores are conflict-free");
static_assert(store_std_degree() == 1, "img_store_std: 16-byte stores are conflict-free");
static_assert(row_halves(0) % 8 == 0 && BLOCK_HALVES % 8 == 0 && OCT_DWORDS % 4 == 0, "16-byte stores stay aligned");

}  // namespace mlp_image
}  // namespace ngp
