// knobs.h — every environment switch of the engine, and the only place in csrc/ that reads the environment.
//
// One rule: a switch is read when the object it configures is created (ngp_model, ngp_trainer,
// ngp_nerf_trainer) and kept on that object; the two process-wide ones are read at their first use. Where a
// switch and a model option cover the same setting, the environment wins. Each read() below is the table of its
// group: name, default, meaning. INTEGRATION.md §4 lists the same switches for users (tests/test_knobs.py).
#pragma once
#include <algorithm>
#include <climits>
#include <cstdint>
#include <cstdlib>

namespace ngp {

constexpr int KNOB_UNSET = INT_MIN;  // the switch is not in the environment: the owner's own choice (auto) holds

inline int knob_int(const char* name, int unset) {
	const char* v = getenv(name);
	return v ? atoi(v) : unset;
}

// The bucketed grid backward's plan (make_scatter_plan, grid_scatter.hip). Read when an ngp_model is created.
struct ScatterKnobs {
	int bricks = KNOB_UNSET;        // 0: no brick levels whatever option "grid_bricks" says
	double brick_min_cells = 3.0;   // a level joins the bricks only if a brick spans this many of its cells per dimension
	int brick_part = 1024;          // samples per brick part
	int lds_kb = KNOB_UNSET;        // LDS budget of a bucket's accumulators in KB (at most the 64 KB tile)
	int direct = KNOB_UNSET;        // 0/1: overrides option "grid_direct"
	int direct_part = KNOB_UNSET;   // samples per direct part (auto: 16384)
	int plan_inline = KNOB_UNSET;   // 0/1: overrides option "grid_plan_inline"
	int chunk = KNOB_UNSET;         // samples per scatter block, 512 or 1024 (auto: 512, or 1024 for sparse tables)
	int part = 49152;               // items per part of a split bucket
	int limit = 49152;              // buckets with more items are summed in parts
	int xcd = 2;                    // scatter block order: 0 plain, 1 a chunk's levels on one XCD, 2 that plus chunk ranges per XCD
	int bt = KNOB_UNSET;            // accumulation block threads, a multiple of 64 up to 1024 (auto: 512 for F = 2, else 1024)
	static ScatterKnobs read() {
		ScatterKnobs k;
		k.bricks = knob_int("NGP_SC_BRICKS", KNOB_UNSET);
		if (const char* e = getenv("NGP_SC_BRICK_MIN_CELLS")) k.brick_min_cells = atof(e);
		if (const char* e = getenv("NGP_SC_BRICK_PART")) k.brick_part = std::max(1, atoi(e));
		k.lds_kb = knob_int("NGP_SC_LDS_KB", KNOB_UNSET);
		k.direct = knob_int("NGP_SC_DIRECT", KNOB_UNSET);
		k.direct_part = knob_int("NGP_SC_DIRECT_PART", KNOB_UNSET);
		k.plan_inline = knob_int("NGP_SC_PLAN_INLINE", KNOB_UNSET);
		k.chunk = knob_int("NGP_SC_CHUNK", KNOB_UNSET);
		k.part = knob_int("NGP_SC_PART", k.part);
		k.limit = knob_int("NGP_SC_LIMIT", k.limit);
		k.xcd = knob_int("NGP_SC_XCD", k.xcd);
		k.bt = knob_int("NGP_SC_BT", KNOB_UNSET);
		return k;
	}
};

// The optimizer's layout and exchange stream. Read in ngp_trainer_create (every creation: tests flip NGP_LAZY_EMA
// between trainers of one process).
struct TrainerKnobs {
	int lazy_ema = KNOB_UNSET;         // 0/1: eager arrays / lazy-EMA records (auto: records from 2^20 parameters)
	int ema_closed_form = KNOB_UNSET;  // 0/1: trainer option "ema_closed_form" at creation
	bool xs_high_priority = true;      // 0: the sharded exchange's second stream at the default priority
	static TrainerKnobs read() {
		TrainerKnobs k;
		k.lazy_ema = knob_int("NGP_LAZY_EMA", KNOB_UNSET);
		k.ema_closed_form = knob_int("NGP_EMA_CLOSED_FORM", KNOB_UNSET);
		k.xs_high_priority = knob_int("NGP_XS_PRIORITY", 1) != 0;
		return k;
	}
};

// The NeRF training step (nerf_trainer.hip). Read in ngp_nerf_trainer_create.
struct NerfKnobs {
	int early = KNOB_UNSET;        // early counter publish + two sample sets: 1 always, 0 never (negative or unset: under cone stepping)
	int waitval = 1;               // queue handoffs by value: 1 sampler -> inference, 2 the buffer release too, 0 events only
	int splat_sort = 1;            // density-grid update: 1 sorted / binned splat, 0 memset + scattered atomics
	bool grid_final_fused = true;  // density-grid update's EMA, mean and bitfield fused (0: the 11-launch form)
	bool loss_state = true;        // loss pass 2 reads pass 1's per-sample state (0: composites each ray again)
	bool grid_pregen = true;       // the next update's samples generated under this step's training pass
	int sampler_prio = 0;          // the sampler stream's queue priority: -1 low, 1 high, 0 default
	int main_prio = 0;             // the trainer's own stream (null-stream callers), likewise
	int sampler_cu_keep = 0;       // k in 1..7: the sampler's queue may use k of every 8 CUs
	static NerfKnobs read() {
		NerfKnobs k;
		k.early = knob_int("NGP_NERF_EARLY", KNOB_UNSET);
		k.waitval = knob_int("NGP_NERF_WAITVAL", k.waitval);
		k.splat_sort = knob_int("NGP_SPLAT_SORT", k.splat_sort);
		k.grid_final_fused = knob_int("NGP_GRID_FINAL_FUSED", 1) != 0;
		k.loss_state = knob_int("NGP_LOSS_STATE", 1) != 0;
		k.grid_pregen = knob_int("NGP_GRID_PREGEN", 1) != 0;
		k.sampler_prio = knob_int("NGP_SAMPLER_PRIO", 0);
		k.main_prio = knob_int("NGP_MAIN_PRIO", 0);
		k.sampler_cu_keep = knob_int("NGP_SAMPLER_CU_KEEP", 0);
		return k;
	}
};

// Process-wide, read once at first use.
struct ProcessKnobs {
	uint32_t mlp_train_blocks = 100;  // training MLP blocks per CU x 100, 25..1600 (else 100)
	bool sdf_stats = false;           // set: the SDF ground truth prints its stab-ray traversal statistics (synchronises)
};
inline const ProcessKnobs& process_knobs() {
	static const ProcessKnobs k = [] {
		ProcessKnobs p;
		const int x = knob_int("NGP_MLP_TRAIN_BLOCKS", 100);
		p.mlp_train_blocks = (uint32_t)(x >= 25 && x <= 1600 ? x : 100);
		p.sdf_stats = getenv("NGP_SDF_STATS") != nullptr;
		return p;
	}();
	return k;
}

// "key=value,key=value": engine options set on every model at its creation (nullptr: unset)
inline const char* knob_model_opts() { return getenv("NGP_MODEL_OPTS"); }

}  // namespace ngp
