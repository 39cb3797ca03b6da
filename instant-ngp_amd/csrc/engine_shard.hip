// engine_shard.hip — the sharded and parted gradient exchange of a data-parallel training step (ngp_trainer's
// issue_part / begin_shard_step / shard_step) and the entry points that attach an exchange to a trainer.
#include "engine_host.h"

void ngp_trainer::make_part_bounds(uint32_t w) {
	const uint64_t q = 8ull * w;
	pb.assign(1, 0);
	for (uint32_t j = 1; j < dp_parts; ++j) {
		const uint64_t b = (n_pad * j / dp_parts) / q * q;
		if (b > pb.back() && b < n_pad) pb.push_back(b);
	}
	pb.push_back(n_pad);
}
void ngp_trainer::ensure_exchange_stream() {
	if (xs) return;
	// the exchange stream at the highest priority: a stream of the default priority may share a hardware queue
	// with the step's stream (GPU_MAX_HW_QUEUES), which would run its work in submission order, after the step's
	// next launches. NGP_XS_PRIORITY=0: the default priority (A/B)
	int lo = 0, hi = 0;
	NGP_HIP(hipDeviceGetStreamPriorityRange(&lo, &hi));
	NGP_HIP(hipStreamCreateWithPriority(&xs, hipStreamNonBlocking, knobs.xs_high_priority ? hi : 0));
	for (hipEvent_t& ev : ev_part) NGP_HIP(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
	NGP_HIP(hipEventCreateWithFlags(&ev_xs, hipEventDisableTiming));
}
void ngp_trainer::issue_part(uint32_t j) {
	PartStep& q = ps_;
	// parts go out from the last to the first (the order the parted backward finishes them), on every rank
	if (q.rc != NGP_OK || j + 1 >= pb.size() || j + 2 + q.issued != pb.size()) { q.rc = NGP_ERROR; return; }
	hipStream_t x = q.s;
	if (q.overlap) {
		NGP_HIP(hipEventRecord(ev_part[j], q.s));
		NGP_HIP(hipStreamWaitEvent(xs, ev_part[j], 0));
		x = xs;
	}
	const uint64_t a = pb[j], len = pb[j + 1] - pb[j];
	const ngp::Exchange& e = q.e;
	if (e.fn(e.user, q.wire16 ? (void*)(g16 + a) : (void*)(g32 + a), len, q.wire16 ? NGP_DTYPE_F16 : NGP_DTYPE_F32,
	         NGP_REDUCE_SCATTER_SUM, x) != NGP_OK) { q.rc = NGP_ERROR; return; }
	uint64_t lo, hi;
	part_slice(j, lo, hi);
	ngp_model* m = model;
	const bool mlp_here = lo == 0 && hi >= m->n_matrix();
	AdamState st{w32, w16, g16, nullptr, nullptr, nullptr, nullptr, inf16,
	             mlp_here && m->frags_current ? (f16*)m->frags.p : nullptr, m->d_fragmap, q.step_base, q.step_add,
	             q.step_base ? (const AdamConfig*)(ctl + CTL_CFG) : nullptr, rec, bias_tab, q.wire16 ? nullptr : g32};
	{
		ProfScope ps("optimizer", x);
		adam_lazy_range(cfg, (uint32_t)lo, (uint32_t)hi, (uint32_t)m->n_matrix(), q.loss_scale, st, x);
	}
	if (e.fn(e.user, w16 + a, len, NGP_DTYPE_F16, NGP_ALL_GATHER, x) != NGP_OK) { q.rc = NGP_ERROR; return; }
	++q.issued;
}
const BwdParts* ngp_trainer::begin_shard_step(hipStream_t s, float loss_scale, const ngp::Exchange& e, const uint32_t* step_base,
                                              uint32_t step_add, uint32_t n_batch, bool stores_input) {
	ps_ = PartStep{};
	ps_.s = s; ps_.e = e; ps_.loss_scale = loss_scale; ps_.step_base = step_base; ps_.step_add = step_add;
	ps_.wire16 = dp_wire16;
	ngp_model* m = model;
	if (pb.size() < 3 || !m->parts_ok(n_batch) || !(stores_input || dp_wire16)) return nullptr;
	ensure_exchange_stream();
	ps_.overlap = true;
	const ScatterPlan& p = m->sc_plan_for(n_batch);
	// the MLP's gradient (slab reduction with bucket range 0) must lie in part 0
	if (p.bk.LD || pb[1] < m->grid_offset()) { ps_.overlap = false; return nullptr; }
	bparts = BwdParts{};
	bparts.k = (uint32_t)pb.size() - 1;
	const uint64_t go = m->grid_offset();
	// range j ends at the bucket holding part j + 1's first parameter: that bucket is summed with range j + 1,
	// before part j + 1 goes out, so every part is final when its exchange starts
	for (uint32_t j = 0; j < bparts.k; ++j)
		bparts.vb_end[j] = j + 1 == bparts.k ? p.n_buckets : scatter_bucket_at_param(m->grid, p, pb[j + 1] > go ? pb[j + 1] - go : 0);
	bparts.after = part_done;
	bparts.user = this;
	return &bparts;
}
int ngp_trainer::shard_step(bool stored) {
	PartStep& q = ps_;
	hipStream_t s = q.s;
	ngp_model* m = model;
	if (q.issued == 0) {
		q.overlap = false;  // nothing handed over (not the bucketed backward): every part here, on s
		if (!stored && !q.wire16) widen_f16(g16, g32, n, s);  // the backward did not write the fp32 input itself
	}
	while (q.rc == NGP_OK && q.issued + 1 < pb.size()) issue_part((uint32_t)pb.size() - 2 - q.issued);
	if (q.rc != NGP_OK) return NGP_ERROR;
	if (q.overlap) {
		NGP_HIP(hipEventRecord(ev_xs, xs));
		NGP_HIP(hipStreamWaitEvent(s, ev_xs, 0));
	}
	if (!mlp_owned() && m->n_matrix() > 0) m->prep(s, false);  // fragments of the gathered MLP weights
	inf_stale = w32_stale = true;
	if (q.e.world > 1) shards_valid = false;
	return NGP_OK;
}

// The sharded optimizer's buffers for `world` ranks: the fp32 gradient staging of the reduce-scatter, sized
// outside any capture (the records and w16 carry SHARD_PAD spare parameters for the padding)
static void trainer_prepare_shards(ngp_trainer* t, uint32_t world) {
	if (!t->rec) return;
	const uint64_t q = 8ull * world, n_pad = (t->n + q - 1) / q * q;
	NGP_CHECK(n_pad - t->n <= ngp_trainer::SHARD_PAD, "sharded optimizer: too many ranks for the parameter padding");
	t->n_pad = n_pad;
	t->make_part_bounds(world);
	if (t->g32 && t->g32_count == n_pad) return;
	if (t->g32) NGP_HIP(hipFree(t->g32));
	t->g32 = nullptr;
	NGP_HIP(hipMalloc(&t->g32, n_pad * sizeof(float)));
	NGP_HIP(hipMemset(t->g32, 0, n_pad * sizeof(float)));  // the padding stays 0: it sums to 0 in the reduce-scatter
	t->g32_count = n_pad;
}

extern "C" {

int ngp_trainer_set_data_parallel(ngp_trainer* t, uint32_t rank, uint32_t world, ngp_allreduce_fn fn, void* user) {
	NGP_ARG(t && world >= 1 && rank < world && (fn || world == 1));
	NGP_TRY({
		NGP_CHECK(t->shards_valid, "set_data_parallel: gather the sharded optimizer state first (ngp_trainer_gather_shards)");
		t->allreduce = fn;
		t->allreduce_user = user;
		t->world = fn ? world : 1;
		t->dp_rank = fn ? rank : 0;
		t->dp_rank_known = fn != nullptr;
		if (fn) trainer_prepare_shards(t, world);
		// the engine's communicator widens fp16 all-reduces to fp32 (the unsharded path): staging sized now
		if (fn == ngp_dp_comm_allreduce && user)
			NGP_CHECK(ngp_dp_comm_reserve((ngp_dp_comm*)user, t->n) == NGP_OK, "ngp_dp_comm_reserve failed");
	});
}

int ngp_trainer_gather_shards(ngp_trainer* t, void* stream) {
	NGP_ARG(t);
	NGP_TRY({
		if (t->shards_valid) return NGP_OK;
		NGP_CHECK(t->allreduce && t->rec && t->n_pad && t->pb.size() >= 2, "gather_shards: no sharded exchange attached");
		// records of each part's parameter pairs, 12 floats each: rank r's slice of the part holds the pairs of its
		// parameter slice
		static_assert(sizeof(AdamRec) == 12 * sizeof(float), "AdamRec: 12 floats");
		for (size_t j = 0; j + 1 < t->pb.size(); ++j)
			if (t->allreduce(t->allreduce_user, t->rec + t->pb[j] / 2, (t->pb[j + 1] - t->pb[j]) / 2 * 12, NGP_DTYPE_F32, NGP_ALL_GATHER,
			                 stream) != NGP_OK)
				throw Error(*ngp_last_error() ? ngp_last_error() : "gather_shards: all-gather failed");
		NGP_HIP(hipStreamSynchronize(S(stream)));
		t->shards_valid = true;
	});
}

int ngp_trainer_set_allreduce(ngp_trainer* t, uint32_t world, ngp_allreduce_fn allreduce, void* user) {
	NGP_ARG(t && world >= 1);
	NGP_TRY({
		NGP_CHECK(t->shards_valid, "set_allreduce: gather the sharded optimizer state first (ngp_trainer_gather_shards)");
		t->allreduce = allreduce;
		t->allreduce_user = user;
		t->world = allreduce ? world : 1;
		t->dp_rank = 0;
		t->dp_rank_known = false;
		// the engine's communicator widens the fp16 sum to fp32: size its staging now, outside any capture
		if (allreduce == ngp_dp_comm_allreduce && user)
			NGP_CHECK(ngp_dp_comm_reserve((ngp_dp_comm*)user, t->n) == NGP_OK, "ngp_dp_comm_reserve failed");
	});
}

}  // extern "C"
