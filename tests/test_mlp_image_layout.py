"""The LDS image layout of the MLP training kernels (csrc/mlp_image.h), checked on the host: a small program compiled
with g++ against the header prints the offsets the kernels use; the checks below re-derive everything from those
numbers by brute force over the lanes, independently of the header's own static_asserts.

Bank rule (gfx950 LDS): ds_read_b64_tr_b16 is served in two groups, lanes 0-31 and 32-63, bank = dword address
mod 64, 8 bytes per lane; a group costs one cycle per distinct dword address on its busiest bank."""
import json
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "instant-ngp_amd", "csrc")
WIDTHS = [16, 32, 64]          # image widths in halves; the encoding image is 16 ES = 16 or 32

PROGRAM = r"""
#include "mlp_image.h"
#include <cstdio>
using namespace ngp::mlp_image;
int main() {
	const int widths[3] = {16, 32, 64};
	std::printf("{\"rd1\": %d, \"images\": {", FRAG_RD1_HALVES);
	for (int wi = 0; wi < 3; ++wi) {
		const int w = widths[wi];
		std::printf("%s\"%d\": {\"halves\": %d, \"slot\": [", wi ? ", " : "", w, image_halves(w));
		for (int r = 0; r < 32; ++r) std::printf("%s%d", r ? ", " : "", row_slot(r));
		std::printf("], \"offset\": [");
		for (int r = 0; r < 32; ++r) {
			std::printf("%s[", r ? ", " : "");
			for (int f = 0; f < w; ++f) std::printf("%s%d", f ? ", " : "", offset(r, f));
			std::printf("]");
		}
		std::printf("], \"frag\": [");
		for (int f0 = 0; f0 < w; f0 += 16)
			for (int rd = 0; rd < 2; ++rd) {
				std::printf("%s[", (f0 || rd) ? ", " : "");
				for (int lane = 0; lane < 64; ++lane) std::printf("%s%d", lane ? ", " : "", frag_offset(lane, rd, f0));
				std::printf("]");
			}
		std::printf("]}");
	}
	std::printf("}}\n");
	return 0;
}
"""


@pytest.fixture(scope="module")
def layout(tmp_path_factory):
    d = tmp_path_factory.mktemp("mlp_image")
    src, exe = os.path.join(d, "layout.cpp"), os.path.join(d, "layout")
    with open(src, "w") as f:
        f.write(PROGRAM)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", CSRC, "-o", exe, src])
    return json.loads(subprocess.check_output([exe], text=True))


def degree(offsets_halves, dwords, banks):
    """Most distinct dword addresses on one bank among the lanes of one group."""
    per_bank = {}
    for o in offsets_halves:
        assert o % 2 == 0
        for d in range(dwords):
            dw = o // 2 + d
            per_bank.setdefault(dw % banks, set()).add(dw)
    return max(len(v) for v in per_bank.values())


def frag_lane(lane):
    g, i = lane >> 4, lane & 15
    return g, i >> 2, i & 3


@pytest.mark.parametrize("w", WIDTHS)
def test_rows_are_a_bijection_and_do_not_overlap(layout, w):
    im = layout["images"][str(w)]
    assert sorted(im["slot"]) == list(range(32))
    seen = {}
    for r in range(32):
        for f in range(w):
            o = im["offset"][r][f]
            assert 0 <= o < im["halves"], (r, f, o)
            assert o not in seen, f"row {r} feature {f} shares half {o} with {seen[o]}"
            seen[o] = (r, f)
        for f0 in range(0, w, 16):
            blk = [im["offset"][r][f0 + k] for k in range(16)]
            # a block's 16 features fill one 16-byte-aligned window of 32 bytes (the 8 dwords a read takes of a row) ...
            assert min(blk) % 8 == 0 and max(blk) == min(blk) + 15
            for q in range(0, 16, 4):
                # ... in contiguous, 8-byte-aligned quads (one lane's share of a transposed read; an 8-byte store)
                assert blk[q] % 4 == 0 and blk[q:q + 4] == list(range(blk[q], blk[q] + 4))
            for q in range(0, 16, 8):
                # ... and each aligned pair of quads in one 16-byte unit (img_store_std)
                assert min(blk[q:q + 8]) % 8 == 0 and max(blk[q:q + 8]) == min(blk[q:q + 8]) + 7
    assert len(seen) == 32 * w


@pytest.mark.parametrize("w", WIDTHS)
def test_fragment_reads_address_the_rows_the_mfma_needs(layout, w):
    """Lane (g, q, p) reads features f0 + 4p.. of sample 8g + q, then of sample 8g + q + 4: which sample sits at which
    K index is unchanged, only where its row lies."""
    im = layout["images"][str(w)]
    for fi, f0 in enumerate(range(0, w, 16)):
        for rd in range(2):
            for lane in range(64):
                g, q, p = frag_lane(lane)
                assert im["frag"][2 * fi + rd][lane] == im["offset"][8 * g + q + 4 * rd][f0 + 4 * p]
            if rd:
                assert all(b - a == layout["rd1"] for a, b in zip(im["frag"][2 * fi], im["frag"][2 * fi + 1]))


@pytest.mark.parametrize("w", WIDTHS)
def test_transposed_reads_are_conflict_free(layout, w):
    im = layout["images"][str(w)]
    for addrs in im["frag"]:
        for grp in range(2):
            assert degree(addrs[32 * grp:32 * grp + 32], 2, 64) == 1


@pytest.mark.parametrize("w,stride", [(16, 20), (32, 36), (64, 68)])
def test_the_former_padded_strides_were_two_way(w, stride):
    """The layout this one replaces: row r at r * stride halves (stride = width + 4). Every read group took 2 cycles."""
    for f0 in range(0, w, 16):
        for rd in range(2):
            addrs = []
            for lane in range(64):
                g, q, p = frag_lane(lane)
                addrs.append((8 * g + q + 4 * rd) * stride + f0 + 4 * p)
            for grp in range(2):
                assert degree(addrs[32 * grp:32 * grp + 32], 2, 64) == 2


@pytest.mark.parametrize("w", WIDTHS)
def test_store_conflicts_are_as_documented(layout, w):
    """img_store_acc: lane (sample = lane & 31, h = lane >> 5) writes 8 B at features 4h and 4h + 8 of a block
    (ds_write_b64: four groups of 16 consecutive lanes, bank = dword mod 32). img_store_std: the 16-byte unit of
    features 8h .. 8h + 7 (ds_write_b128: eight groups of 8 lanes). Both conflict-free."""
    im = layout["images"][str(w)]
    for f0 in range(0, w, 16):
        for k in range(2):
            for grp in range(4):
                lanes = range(16 * grp, 16 * grp + 16)
                assert degree([im["offset"][l & 31][f0 + 4 * (l >> 5) + 8 * k] for l in lanes], 2, 32) == 1
        for grp in range(8):
            lanes = range(8 * grp, 8 * grp + 8)
            assert degree([min(im["offset"][l & 31][f0 + 8 * (l >> 5):][:8]) for l in lanes], 4, 32) == 1
