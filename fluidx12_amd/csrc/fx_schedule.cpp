// fx_schedule.cpp -- Fluid::Simulate (/root/reference/FluidX12/Content/Fluid.cpp:348-410) as a schedule of kernel launches and halo
// exchanges over a group of z-slab contexts: one code path serves the single-GPU case, the RCCL slabs and the in-process loop-back
// slabs.  The C ABI entry points that drive it are in fx_api.cpp and fx_stage_api.cpp; contexts, fields and options in fx_context.cpp.
#include "fx_host.h"
#include <memory>

using namespace fx;

namespace fxh {

// ---- the simulation step, phase by phase, over a group of slab contexts ----------------------------
// (Fluid::Simulate, Fluid.cpp:348-410; the phase structure is what lets one code path serve the
// single-GPU case, the RCCL slabs and the in-process loop-back slabs)
//
// Multi-rank schedule of one step (k = sweeps per pressure exchange, Ha = advect halo):
//   1  [comm] exchange Ha planes of velocity + colour      || [compute] advect the planes >= Ha away from a slab face
//      then advect the 2 x Ha face planes
//   2  exchange 1 plane of the advected uz ; divergence on the owned planes
//   3  exchange k-1 planes of b and k planes of p (one message group)
//   4  per round of k sweeps: the k planes next to each face are brought to the round's last level first
//      (thin single-sweep launches over both face zones, from the exchanged halo), [comm] they travel to the
//      neighbour || [compute] the interior follows with the fused-sweep kernels (see jacobi_overlapped)
//   5  projection (reads the 1st halo plane of the last exchange)
// Every cell is computed with the arithmetic of the single-domain run, so results are bit-identical.
int for_members(fx_ctx* ctx, std::vector<fx_ctx*>& out)
{
	out.clear();
	if (ctx->group && ctx->group->transport->is_local() && !ctx->group->broken) out = ctx->group->members;
	else out.push_back(ctx);                           // (a broken loop-back group: only this context, and only for teardown)
	return FX_OK;
}


// ---- lanes (fx_context.h): where a member's work is enqueued.  One lane serves a whole shared-stream loop-back group and an RCCL rank;
// a peer group has a lane per member, each with the member's own compute stream.
static inline bool peer_group(const fx_ctx* c) { return c->group && c->group->per_member; }
// the compute stream of member m in a step driven on stream s
static inline hipStream_t CS(const fx_ctx* m, hipStream_t s) { return peer_group(m) ? m->group->lane_of(m).compute : s; }
struct LaneRef { fx_lane* lane; hipStream_t compute; };
static std::vector<LaneRef> lanes_of(fx_ctx* lead, const std::vector<fx_ctx*>& M, hipStream_t s)
{
	std::vector<LaneRef> out;
	if (!lead->group) return out;
	if (lead->group->per_member) for (fx_ctx* m : M) out.push_back(LaneRef{ &lead->group->lane_of(m), lead->group->lane_of(m).compute });
	else out.push_back(LaneRef{ &lead->group->lanes[0], s });
	return out;
}
enum StreamKind { ON_COMPUTE = 0, ON_COMM = 1 };

// 0 = no side stream, 1 = advection halo overlapped, 2 = pressure rounds overlapped as well, 3 = and the colour half of the
// next step's advection halo travels behind this step's pressure phase (fx_set_option)
int overlap_level(const fx_ctx* lead)
{
	if (!multi_rank(lead) || lead->group->lanes.empty() || !lead->group->lanes[0].comm) return 0;
	return lead->opt_overlap;
}

struct ExchSpec { int set, k, pidx; };

// one exchange of the chain, ordered on every lane's compute or comm stream
static int do_exchange(fx_ctx* ctx, const std::vector<fx_ctx*>& M, const ExchSpec* specs, int nspec, StreamKind kind, hipStream_t s, int channel = 0)
{
	if (!multi_rank(ctx)) return FX_OK;
	DeviceGuard dg(ctx->device);
	std::vector<hipStream_t> streams;
	for (const LaneRef& L : lanes_of(ctx, M, s)) streams.push_back(kind == ON_COMM ? L.lane->comm : L.compute);
	ScopedMark mk(ctx, peer_group(ctx) ? streams[(size_t)ctx->rank] : streams[0], MK_EXCH);
	std::vector<std::vector<Seg>> segs(M.size());
	size_t total = 0;
	for (size_t i = 0; i < M.size(); ++i) {
		for (int j = 0; j < nspec; ++j) {
			if (specs[j].k <= 0) continue;
			ExchItem it[4];
			const int n = exchange_items(M[i], specs[j].set, specs[j].k, specs[j].pidx, it);
			halo_segments(M[i], it, n, segs[i]);
		}
		total += segs[i].size();
		if (M[i]->timing_on) for (const Seg& sg : segs[i]) M[i]->acc.exchange_bytes += sg.bytes;     // what this rank sends
	}
	if (!total) return FX_OK;
	for (fx_ctx* m : M) if (m->timing_on) m->acc.exchange_calls += 1;  // one group call (ncclGroupStart .. End) per exchange
	return ctx->group->transport->exchange(ctx->group, segs, streams, channel);
}

// on every lane: `to` picks up after everything queued on `from` so far
#define FX_LANES(body) do { for (const LaneRef& L : lanes_of(ctx, M, s)) { DeviceGuard dgl_(L.lane->device); body } } while (0)
// comm stream picks up after everything queued on the compute stream so far
static int comm_fork(fx_ctx* ctx, const std::vector<fx_ctx*>& M, hipStream_t s)
{
	FX_LANES(FX_HIP(hipEventRecord(L.lane->ev_ready, L.compute)); FX_HIP(hipStreamWaitEvent(L.lane->comm, L.lane->ev_ready, 0)););
	return FX_OK;
}
static int comm_mark_done(fx_ctx* ctx, const std::vector<fx_ctx*>& M, hipStream_t s) { FX_LANES(FX_HIP(hipEventRecord(L.lane->ev_done, L.lane->comm));); return FX_OK; }
static int comm_join(fx_ctx* ctx, const std::vector<fx_ctx*>& M, hipStream_t s) { FX_LANES(FX_HIP(hipStreamWaitEvent(L.compute, L.lane->ev_done, 0));); return FX_OK; }


// advect planes [r.lo, r.hi); own_only: back-traces must stay inside the owned planes (the halo is still in flight)
int advect_range(fx_ctx* ctx, hipStream_t s, Range r, bool own_only)
{
	if (r.hi <= r.lo) return FX_OK;
	DeviceGuard dg(ctx->device);
	const SimParams sp{ ctx->time_step, (int)ctx->desc.advect_address, ctx->g.Zg > 1 ? 1 : 0, ctx->impulse_on ? 1 : 0 };
	const int par = ctx->frame_parity;
	if (ctx->adv_scheme == FX_ADVECT_MACCORMACK) {
		// the predictor and the corrector (fx_maccormack.hip) over the whole grid -- fx_set_advection_scheme refuses slab ranks, so the range is
		// all of it -- from the same inputs into the same outputs as the launch below; the render's alpha side volume on that launch's terms.
		// Everything behind reads velocity[0] / velocity[1] / colour[parity] per call (the confinement's pointer swap included): the scratch is
		// the scheme's own and dead once the corrector has run
		if (!ctx->mc_vel || !ctx->mc_col || r.lo != 0 || r.hi != ctx->g.Zg) { ctx->last_error = "MacCormack advection of a partial plane range"; return FX_E_STATE; }
		const bool was_rendered = ctx->rendered_since_step && ctx->rendered_on == s;
		ctx->rendered_since_step = false;
		float* alpha = was_rendered && ctx->accel_ok && ctx->opt_render_accel && FX_KNOB_INT("ADVECT_ALPHA", 1) ? ctx->accel.alpha : nullptr;
		if (ctx->accel_alpha_of == ctx->col[par]) ctx->accel_alpha_of = nullptr;      // that buffer is about to change
		FX_HIP(launch_maccormack(ctx->g, sp, ctx->half, ctx->vel[0], ctx->col[1 - par], ctx->vel[1], ctx->col[par], ctx->mc_vel, ctx->mc_col, alpha, s));
		if (alpha) ctx->accel_alpha_of = ctx->col[par];
		return FX_OK;
	}
	Geom g = ctx->g;
	// only halo_advect planes per side were refreshed by EX_ADVECT_IN; the allocation may be wider (max with halo_jacobi), and
	// a tap into those stale planes must count as "left the exchanged halo", not as present data
	// (with FX_OPT_ADAPTIVE_HALO: only the planes this step's exchange carried, adv_w_lo / adv_w_hi <= halo_advect)
	g.zlo = std::max(g.zlo, g.z0 - ctx->adv_w_lo); g.zhi = std::min(g.zhi, g.z0 + g.nz - 1 + ctx->adv_w_hi);
	if (own_only) { g.zlo = std::max(g.zlo, g.z0); g.zhi = std::min(g.zhi, g.z0 + g.nz - 1); }
	// the context lends the staged kernel scratch to put far-tracing voxels aside (allocated by fx_create for its owned planes -- the lazy
	// branch below only serves contexts made before that; every advection of a context runs on its compute stream, one after the other,
	// so one scratch serves all its ranges)
	if (!ctx->adv_far && !ctx->adv_far_tried) {
		ctx->adv_far_tried = true;
		const size_t words = advect_far_words(g, g.nz);
		if (words) {
			if (hipMalloc((void**)&ctx->adv_far, words * sizeof(uint32_t)) == hipSuccess) {
				FX_HIP(hipMemsetAsync(ctx->adv_far, 0, 2 * sizeof(uint32_t), s));   // the two alternating totals
				ctx->adv_far_words = words;
			} else {                                         // no room for the scratch: the staged kernel gathers far-tracing voxels itself
				(void)hipGetLastError();
				ctx->adv_far = nullptr;
			}
		}
	}
	const bool lend = ctx->adv_far != nullptr;
	bool far_used = false;
	// the render's alpha-only side volume (fx_render_accel.hip) is written by the launch that makes the colour field, where that is one
	// staged launch over the whole grid: the render's build pass then reads 4 bytes per voxel instead of the whole texel
	const bool frame_was_rendered = ctx->rendered_since_step && ctx->rendered_on == s;
	ctx->rendered_since_step = false;
	AdvectAlpha aa{ frame_was_rendered && ctx->accel_ok && ctx->opt_render_accel && FX_KNOB_INT("ADVECT_ALPHA", 1) ? ctx->accel.alpha : nullptr, false };
	if (ctx->accel_alpha_of == ctx->col[par]) ctx->accel_alpha_of = nullptr;          // that buffer is about to change
	FX_HIP(launch_advect(g, sp, ctx->half, ctx->vel[0], ctx->col[1 - par], ctx->vel[1], ctx->col[par],
		r.lo, r.hi, ctx->halo_overflow, s, lend ? ctx->adv_far : nullptr, lend ? ctx->adv_far_words : 0, (int)(ctx->adv_far_turn & 1u), &far_used, &aa));
	if (aa.written) ctx->accel_alpha_of = ctx->col[par];
	if (far_used) ++ctx->adv_far_turn;
	return FX_OK;
}

// ---- the per-step record (fx_context.h): written behind the projection, read by the next step ------------------------------
int options_digest(const fx_ctx* c)
{
	uint32_t h = 2166136261u;
	uint32_t dt_bits;
	std::memcpy(&dt_bits, &c->time_step, 4);               // the time step the record's needs were measured with: the ranks must agree on it too
	for (uint32_t v : { (uint32_t)c->opt_overlap, (uint32_t)c->opt_round, (uint32_t)c->opt_adaptive, dt_bits }) h = (h ^ v) * 16777619u;
	return (int)(h & 0x3FFFFFFFu);
}

static int record_step(fx_ctx* ctx, std::vector<fx_ctx*>& M, hipStream_t s)
{
	if (!multi_rank(ctx) || !ctx->step_rec) return FX_OK;
	for (fx_ctx* m : M) {
		if (m->rec_in_project) { m->rec_in_project = false; continue; }       // k_project_v4 has already written it
		DeviceGuard dg(m->device);
		FX_HIP(launch_face_need(m->g, m->half, m->vel[0], m->time_step, (int)m->desc.advect_address, options_digest(m), m->halo_overflow, m->step_rec, CS(m, s)));
	}
	DeviceGuard dg(ctx->device);
	if (ctx->group->transport->is_local()) {
		for (fx_ctx* m : M) {                                                  // every member's record on its own stream, behind its own event
			DeviceGuard dgm(m->device);
			FX_HIP(hipMemcpyAsync(m->rec_host, m->step_rec, 4 * sizeof(int), hipMemcpyDeviceToHost, CS(m, s)));
			FX_HIP(hipEventRecord(m->rec_ev, CS(m, s)));
		}
	} else {
		// off the compute stream when there is a side stream: the next step's interior advection need not wait for the gather
		hipStream_t cs = s;
		if (overlap_level(ctx) >= 1) { int rc = comm_fork(ctx, M, s); if (rc) return rc; cs = ctx->group->lanes[0].comm; }
		if (ctx->group->transport->allgather(ctx->step_rec, 4, ctx->gath_dev, cs) != FX_OK) { ctx->last_error = "rccl: all-gather of the step record failed"; return FX_E_COMM; }
		FX_HIP(hipMemcpyAsync(ctx->rec_host, ctx->gath_dev, 4 * sizeof(int) * (size_t)ctx->nranks, hipMemcpyDeviceToHost, cs));
		FX_HIP(hipEventRecord(ctx->rec_ev, cs));
	}
	for (fx_ctx* m : M) { m->rec_pending = true; m->need_valid = true; m->rec_dt = m->time_step; }
	return FX_OK;
}

// Waits for the previous step's record and takes the step's decisions from it -- every rank holds the same records and therefore
// decides alike: FX_E_HALO if ANY rank's advection left its exchanged planes (or the next one would need more than halo_advect),
// FX_E_STATE if the ranks disagree about the schedule options; else the planes this step's advection exchange carries per face
// (FX_OPT_ADAPTIVE_HALO: the measured need of the two slabs that share the face; otherwise, or when the measurement does not
// cover this step -- first step, velocity uploaded since, larger dt -- the whole halo_advect).
static int consume_record(fx_ctx* ctx, std::vector<fx_ctx*>& M)
{
	const int Ha = (int)ctx->desc.halo_advect;
	for (fx_ctx* m : M) { m->adv_w_lo = has_lower(m) ? Ha : 0; m->adv_w_hi = has_upper(m) ? Ha : 0; }
	if (!multi_rank(ctx) || !ctx->rec_pending) return FX_OK;
	const bool local = ctx->group->transport->is_local();
	for (fx_ctx* m : M) {                                  // (in-process groups: every member's record; an RCCL rank: the gathered one)
		DeviceGuard dg(m->device);
		FX_HIP(hipEventSynchronize(m->rec_ev));
		if (!local) break;
	}
	const int n = ctx->nranks;
	auto rec = [&](int r) -> const int* { return local ? M[(size_t)r]->rec_host : ctx->rec_host + 4 * r; };
	bool fault = false, mismatch = false, usable = ctx->opt_adaptive != 0;
	for (int r = 0; r < n; ++r) { fault = fault || rec(r)[3] != 0; mismatch = mismatch || rec(r)[2] != rec(0)[2]; }
	for (fx_ctx* m : M) { usable = usable && m->need_valid && m->time_step <= m->rec_dt; m->rec_pending = false; }
	if (fault) {
		// This return IS the chain-wide notice of the fault: every rank gets it once, from the same gathered record, and the step
		// after it starts clean -- on every rank, whether or not anybody calls fx_synchronize in between: a rank whose own flag is
		// still up takes it down here (nothing of the previous step is in flight any more: its record has arrived) and remembers the
		// fault on the host instead, so that its read-back and checkpoints keep refusing until fx_synchronize acknowledges it.
		// Left up, the flag would be copied into the record of every later step and the chain would alternate between one executed and
		// one refused step for ever.
		for (fx_ctx* m : M) {
			if (!rec(m->rank)[3] || !m->halo_overflow) continue;
			DeviceGuard dg(m->device);
			FX_HIP(hipDeviceSynchronize());                            // (the overlapped schedule has enqueued this step's interior advection already: it may raise the flag again)
			unsigned flag = 0;
			FX_HIP(hipMemcpy(&flag, m->halo_overflow, sizeof flag, hipMemcpyDeviceToHost));
			if (!flag) continue;                                       // acknowledged by an fx_synchronize since
			FX_HIP(hipMemset(m->halo_overflow, 0, sizeof(unsigned)));
			FX_HIP(hipDeviceSynchronize());                            // the context's streams do not order against the NULL stream
			m->halo_fault = true;
		}
		ctx->last_error = "the previous step's advection left the exchanged halo on at least one rank";
		return FX_E_HALO;
	}
	if (mismatch) { ctx->last_error = "the ranks of the chain run with different schedule options (fx_set_option) or time steps"; return FX_E_STATE; }
	if (!usable) return FX_OK;
	for (int r = 0; r + 1 < n; ++r)
		if (std::max(rec(r)[1], rec(r + 1)[0]) > Ha) {
			ctx->last_error = "the next advection needs more planes across a slab face than halo_advect provides";
			return FX_E_HALO;                            // the step is abandoned; its INPUTS (velocity[0], colour[!parity], pressure) are untouched -- in the
			                                             // overlapped schedule the interior advection has already written part of its outputs (velocity[1], colour[parity])
		}
	for (fx_ctx* m : M) {
		const int r = m->rank;
		m->adv_w_lo = r > 0 ? std::max(rec(r - 1)[1], rec(r)[0]) : 0;
		m->adv_w_hi = r + 1 < n ? std::max(rec(r)[1], rec(r + 1)[0]) : 0;
	}
	return FX_OK;
}

int advect_all(fx_ctx* ctx, std::vector<fx_ctx*>& M, hipStream_t s)
{
	int rc;
	const int Ha = (int)ctx->desc.halo_advect;
	// FX_OPT_OVERLAP 3: the previous step already sent the colour planes this advection gathers from (simulate_impl); only
	// the velocity, which the projection has just finished, travels now.  Every rank of a chain takes the same branch: the
	// flag follows from the option level and the step history alone (a colour upload in between is refused, fx_upload).
	bool col_ready = multi_rank(ctx);
	for (fx_ctx* m : M) col_ready = col_ready && m->col_halo_buf == 1 - (int)m->frame_parity;
	for (fx_ctx* m : M) m->col_halo_buf = -1;
	bool ov = overlap_level(ctx) >= 1;
	if (ov && ctx->group->min_nz <= 2 * Ha) ov = false;        // decided on the thinnest slab of the chain: the same on every rank
	if (!ov) {
		if ((rc = consume_record(ctx, M))) return rc;
		if (col_ready) FX_LANES(FX_HIP(hipStreamWaitEvent(L.compute, L.lane->ev_col_done, 0)););
		const ExchSpec spec{ col_ready ? EX_ADVECT_VEL : EX_ADVECT_IN, Ha, 0 };
		if ((rc = do_exchange(ctx, M, &spec, 1, ON_COMPUTE, s))) return rc;
		for (fx_ctx* m : M) {
			ScopedMark mk(m, CS(m, s), MK_ADVECT);
			if (m->timing_on) m->acc.advect_halo_planes += (uint64_t)(m->adv_w_lo + m->adv_w_hi);
			if ((rc = advect_range(m, CS(m, s), owned(m), false))) return rc;
		}
		return FX_OK;
	}
	// the interior first (it reads owned planes only, whatever the exchange will carry): the device is busy while the host waits
	// for the previous step's record, which sizes the exchange
	if ((rc = comm_fork(ctx, M, s))) return rc;                // the comm stream picks up behind the previous step
	for (fx_ctx* m : M) {
		ScopedMark mk(m, CS(m, s), MK_ADVECT);
		const Range o = owned(m);
		if ((rc = advect_range(m, CS(m, s), Range{ o.lo + (has_lower(m) ? Ha : 0), o.hi - (has_upper(m) ? Ha : 0) }, true))) return rc;
	}
	if ((rc = consume_record(ctx, M))) return rc;
	if (col_ready) FX_LANES(FX_HIP(hipStreamWaitEvent(L.lane->comm, L.lane->ev_col_done, 0)););
	const ExchSpec spec{ col_ready ? EX_ADVECT_VEL : EX_ADVECT_IN, Ha, 0 };
	if ((rc = do_exchange(ctx, M, &spec, 1, ON_COMM, s))) return rc;
	if ((rc = comm_mark_done(ctx, M, s))) return rc;
	if ((rc = comm_join(ctx, M, s))) return rc;
	for (fx_ctx* m : M) {
		ScopedMark mk(m, CS(m, s), MK_ADVECT);
		if (m->timing_on) m->acc.advect_halo_planes += (uint64_t)(m->adv_w_lo + m->adv_w_hi);
		const Range o = owned(m);
		if (has_lower(m) && (rc = advect_range(m, CS(m, s), Range{ o.lo, o.lo + Ha }, false))) return rc;
		if (has_upper(m) && (rc = advect_range(m, CS(m, s), Range{ o.hi - Ha, o.hi }, false))) return rc;
	}
	return FX_OK;
}

// The render's alpha side volume (fx_render_accel.hip) if this step's advection left the alpha of colour[parity] in it, else null: a pass that
// changes that colour field in place stores the alpha there too, so the volume stays true.
static float* alpha_mirror(const fx_ctx* ctx) { return ctx->accel_alpha_of == ctx->col[ctx->frame_parity] ? ctx->accel.alpha : nullptr; }

// Vorticity confinement (fx_vorticity.hip) finishes the advected velocity, so its time is booked with the advection.  The pass cannot run
// in place; velocity[0] is dead between the advection and the projection of a single domain, so the result goes there and the two
// pointers swap: velocity[1] then names the confined field, the projection overwrites the other buffer as always.  Everybody who holds
// these pointers reads them per call (fx_upload / fx_download / fx_field_digest and through them the checkpoint, the exchange items and
// launch_face_need of slab ranks -- which never get here, fx_set_vorticity_confinement refuses them -- and the dt = 0 copy, which the
// pass does not precede: it is a no-op then).
int confine_phase(fx_ctx* ctx, hipStream_t s)
{
	if (!(ctx->vort_eps > 0.0f) || !(ctx->time_step > 0.0f)) return FX_OK;
	DeviceGuard dg(ctx->device);
	ScopedMark mk(ctx, s, MK_ADVECT);
	FX_HIP(launch_confine_vorticity(ctx->g, ctx->half, ctx->vel[1], ctx->vel[0], ctx->vort_eps, ctx->time_step, s));
	std::swap(ctx->vel[0], ctx->vel[1]);
	return FX_OK;
}

// Open walls (fx_open.hip): directly behind the advection and in front of the emitters, the advected colour is scaled by the share of its
// back-traced sample that lies inside the box -- the cells beyond an open face hold clear air.  The trace is the advection's: velocity[0].
// One launch over the grid, in place on colour[parity], booked with the advection; it keeps the render's alpha side volume true on the
// emitters' condition.
int open_inflow_phase(fx_ctx* ctx, hipStream_t s)
{
	if (!ctx->open_faces || !(ctx->time_step > 0.0f)) return FX_OK;
	DeviceGuard dg(ctx->device);
	ScopedMark mk(ctx, s, MK_ADVECT);
	FX_HIP(launch_open_inflow(ctx->g, ctx->half, ctx->vel[0], ctx->col[ctx->frame_parity], alpha_mirror(ctx), ctx->open_faces, ctx->time_step, s));
	return FX_OK;
}

// The settable emitters (fx_emit.hip) add to the advected velocity and colour in place, in front of the confinement and of the divergence
// (the sparse solver's fused one included: it reads velocity[1] behind this launch), booked with the advection like the confinement.
// When this step's advection left the alpha of colour[parity] in the render's side volume, the pass keeps that volume true as well.
int emit_phase(fx_ctx* ctx, hipStream_t s)
{
	if (ctx->emitters.empty() || !(ctx->time_step > 0.0f)) return FX_OK;
	DeviceGuard dg(ctx->device);
	ScopedMark mk(ctx, s, MK_ADVECT);
	FX_HIP(launch_emit(ctx->g, ctx->half, ctx->vel[1], ctx->col[ctx->frame_parity], alpha_mirror(ctx), ctx->emitters.data(), (int)ctx->emitters.size(), ctx->time_step, s));
	return FX_OK;
}

// Buoyancy (fx_heat.hip): behind the emitters -- the force reads the alpha they have added to --, in front of the enforce pass (the pass skips
// solid cells itself, the enforce pass clears their velocity as always) and of the confinement, which leaves velocity[0] unspecified: the
// temperature is traced with velocity[0], the field this step's advection traced with.  One launch over the grid, temp[temp_cur] -> the
// other buffer, then the two swap; the force goes into velocity[1] in place.  Booked with the advection like its neighbours.
int heat_phase(fx_ctx* ctx, hipStream_t s)
{
	if (!ctx->buoy_on || !ctx->temp[0] || !(ctx->time_step > 0.0f)) return FX_OK;
	DeviceGuard dg(ctx->device);
	ScopedMark mk(ctx, s, MK_ADVECT);
	const int cur = ctx->temp_cur;
	FX_HIP(launch_heat(ctx->g, ctx->half, ctx->buoy, ctx->heat_sources.data(), (int)ctx->heat_sources.size(), ctx->vel[0], ctx->vel[1],
		ctx->col[ctx->frame_parity], ctx->temp[cur], ctx->temp[1 - cur], ctx->obst_code, ctx->time_step, (int)ctx->desc.advect_address, s, ctx->open_faces));
	ctx->temp_cur = 1 - cur;
	return FX_OK;
}

// The particle trail (fx_particle_trail.hip): behind buoyancy, in front of the enforce pass.  Colour and temperature are final for the step
// here -- the deposit does not enter this step's buoyancy force: heat left now lifts from the next step on --, and the enforce pass behind it
// has nothing to clear that the pass's own solid test did not keep out.  The positions are the ones the buffer holds now: moved at the end of
// the previous step, or set by the caller.  Two launches, the scatter over the records and the apply over the grid, booked with the advection
// like the neighbours; the temperature is the current buffer (heat_phase has swapped already), in place.  Nothing is allocated, copied or
// waited for (fx_set_particle_trail did that); it keeps the render's alpha side volume true on the emitters' condition.
int trail_phase(fx_ctx* ctx, hipStream_t s)
{
	if (!ctx->trail_acc || !ctx->part || !(ctx->time_step > 0.0f)) return FX_OK;
	DeviceGuard dg(ctx->device);
	ScopedMark mk(ctx, s, MK_ADVECT);
	FX_HIP(launch_trail_splat(ctx->g, ctx->part, ctx->part_count, ctx->trail_acc, s));
	float* temp = ctx->buoy_on && ctx->temp[0] && ctx->trail.heat != 0.0f ? ctx->temp[ctx->temp_cur] : nullptr;
	FX_HIP(launch_trail_apply(ctx->g, ctx->half, ctx->trail, ctx->time_step, ctx->trail_acc, ctx->col[ctx->frame_parity], temp, alpha_mirror(ctx),
		ctx->obst_code, s));
	return FX_OK;
}

// The scatter alone, for fx_particle_density: the accumulator is left holding the set's weights (the caller copies and clears it).  Booked like
// the stage, so that tools/particle_trail_bench.py can time the scatter apart from the apply.
int trail_splat_phase(fx_ctx* ctx, hipStream_t s)
{
	if (!ctx->trail_acc) return FX_E_STATE;
	if (!ctx->part) return FX_OK;
	DeviceGuard dg(ctx->device);
	ScopedMark mk(ctx, s, MK_ADVECT);
	FX_HIP(launch_trail_splat(ctx->g, ctx->part, ctx->part_count, ctx->trail_acc, s));
	return FX_OK;
}

// Solid obstacles (fx_obstacle.hip): behind the advection and the emitters, in front of the confinement, the solid cells of the advected velocity
// and colour become +0, in place -- one launch over the solids' bounding box, booked with the advection like the two passes around it.  When this
// step's advection left the alpha of colour[parity] in the render's side volume, the pass keeps that volume true as well (the emitters' condition).
// While the solids have bodies (fx_set_obstacle_bodies) this pass, the divergence and the projection get the list: the velocity of a solid cell
// is its body's, not +0.  An empty list: the launches below are the ones they were.
int enforce_phase(fx_ctx* ctx, hipStream_t s)
{
	if (!ctx->obst_code || !ctx->obst_cells || !(ctx->time_step > 0.0f)) return FX_OK;
	DeviceGuard dg(ctx->device);
	ScopedMark mk(ctx, s, MK_ADVECT);
	FX_HIP(launch_obstacle_enforce(ctx->g, ctx->half, ctx->obst_code, ctx->obst_lo, ctx->obst_hi, ctx->obst_bodies.data(), (int)ctx->obst_bodies.size(),
		ctx->vel[1], ctx->col[ctx->frame_parity], alpha_mirror(ctx), s));
	return FX_OK;
}

int divergence_phase(fx_ctx* ctx, hipStream_t s)
{
	DeviceGuard dg(ctx->device);
	ScopedMark mk(ctx, s, MK_DIV);
	const Range r = owned(ctx);
	if (ctx->obst_code) {
		FX_HIP(launch_divergence_obs(ctx->g, ctx->half, ctx->vel[1], ctx->obst_code, ctx->obst_bodies.data(), (int)ctx->obst_bodies.size(), ctx->b, r.lo, r.hi, s));
		return FX_OK;
	}
	FX_HIP(launch_divergence(ctx->g, ctx->half, ctx->vel[1], ctx->b, r.lo, r.hi, s));
	return FX_OK;
}

// what this context's rounds run (fx_jacobi_plan.cpp); asks whether a second mask buffer EXISTS, not which of the two is current (jacobi_launch swaps them)
static JacobiPolicy policy_of(const fx_ctx* c)
{
	return jacobi_policy(c->g, (int)(c->desc.flags & FX_FLAG_JACOBI_FUSE_MASK), c->frozen != nullptr, c->frozen_alt != nullptr);
}

// one planned launch: l.sweeps lock-step sweeps p[src] -> p[src ^ 1] on planes [r.lo, r.hi)
static int jacobi_launch(fx_ctx* ctx, hipStream_t s, int src, JacobiLaunch l, Range r, ScopedMark* mk)
{
	r.lo = std::max(r.lo, 0); r.hi = std::min(r.hi, ctx->g.Zg);
	if (r.hi <= r.lo) return FX_OK;
	DeviceGuard dg(ctx->device);
	FX_HIP(launch_jacobi(ctx->g, l, ctx->p[src], ctx->b, ctx->p[src ^ 1], ctx->frozen, ctx->frozen ? ctx->frozen_alt : nullptr, r.lo, r.hi, s));
	if (l.family == JF_TILE2D && ctx->frozen) std::swap(ctx->frozen, ctx->frozen_alt);       // the mask ping-pongs with the pressure
	if (mk) { mk->launches += 1; mk->sweeps += l.sweeps; }
	return FX_OK;
}

// `count` lock-step sweeps whose first one may read `count` exchanged halo planes; the planes swept shrink by
// one per sweep towards the owned range (redundant halo work instead of an exchange per sweep)
static int jacobi_round(fx_ctx* ctx, hipStream_t s, int count, ScopedMark* mk)
{
	std::vector<JacobiLaunch> plan(count);
	plan.resize(jacobi_plan(policy_of(ctx), count, plan.data()));
	int left = count;
	for (const JacobiLaunch& l : plan) {
		const int t = l.sweeps;
		if (mk && mk->kind == MK_JACOBI && mk->launches && t * mk->launches < mk->sweeps) mk->split(MK_JACOBI_TAIL);   // shorter launches from here on
		left -= t;
		const int rc = jacobi_launch(ctx, s, ctx->p_cur, l, grown(ctx, multi_rank(ctx) ? left : 0), mk);
		if (rc) return rc;
		ctx->p_cur ^= 1;
	}
	return FX_OK;
}

static int clear_freeze_masks(std::vector<fx_ctx*>& M, hipStream_t s)
{
	for (fx_ctx* m : M)
		if (m->frozen) { DeviceGuard dg(m->device); if (hipMemsetAsync(m->frozen, 0, m->g.cells_local(), s) != hipSuccess) return FX_E_DEVICE; }
	return FX_OK;
}

// FX_JACOBI_FAITHFUL: the sparse solver of fx_jacobi_freeze.hip, as fx_jacobi_plan.cpp plans it (freeze_plan): level 1 everywhere, then
// masked strip launches for every cell while most tiles relax, then launches over the tiles that still do, all enqueued; the result is in
// the last launch's output buffer (settled tiles agree in both).  Bit-identical to `iters` generic sweeps with the byte mask
// (tests/test_gpu_freeze.py).  A slab rank (round 4) runs it on the view of the planes it holds (jacobi_freeze_view): the dense sweep
// over its owned planes, the tile cones reaching into the halo, and kFreezeHalo planes of pressure + mask travelling to the
// neighbours behind every launch -- every rank enqueues the same launches and exchanges whatever its tiles do.
// (The dense sweep in front of tile launches writes level 1 to BOTH buffers they alternate between.  Writing one and letting the first
// tile launch carry the unlisted tiles' border cells across was built and measured level: the dense sweep 75 -> 46 us at 256^3, the
// first tile launch slower by as much -- the shell of a 4-deep cone around ~3000 listed tiles is more bytes than the second copy.)
// Whole steps (simulate_impl) leave the divergence to the dense sweep: it computes b from the advected velocity and stores it for the
// launches behind it, instead of reading it back from a launch of its own.
// fx_timing books the dense sweep as the "main" launch and the launches behind it beside it.  A single domain keeps ONE mark open over
// all of them (an event record between two launches is a 2-3 us gap, 17 of them a solve); slab ranks close it at every exchange.
static bool takes_sparse_solver(const fx_ctx* c, uint32_t iters) { return freeze_takes_sparse_solver(c->g, iters, c->frozen && c->fz_tile_next, multi_rank(c), multi_rank(c) ? c->group->min_nz : 0); }

// the buffers behind a launch that read `a`: a tile launch left its last level in d; a strip launch in d AND the spare, and the buffer it
// read is the spare now
template <class T> static void freeze_rotate(T*& a, T*& d, T*& spare, bool strip) { std::swap(a, d); if (strip) std::swap(d, spare); }

static int jacobi_freeze(fx_ctx* lead, std::vector<fx_ctx*>& M, hipStream_t s, uint32_t iters)
{
	fx_ctx* ctx = lead;                                                 // FX_HIP reports through `ctx`
	const bool multi = multi_rank(lead);
	struct Run { Geom v; size_t off, moff; int own0; FreezeWork w; float *src, *a, *d; uint8_t *ma, *md, *mx; uint32_t* stat; uint32_t stat_hi; };
	std::vector<Run> R(M.size());
	std::vector<std::unique_ptr<ScopedMark>> mk(M.size());
	const bool fuse = lead->fz_fuse_div;
	lead->fz_fuse_div = false;
	FreezeLaunch plan[kFreezeSlots];                                    // (the same on every rank of a chain: no strips there, and the tile launches follow from iters alone)
	int launches = 0;
	for (size_t i = 0; i < M.size(); ++i) {
		fx_ctx* m = M[i];
		DeviceGuard dg(m->device);
		hipStream_t ms = CS(m, s);
		if (++m->fz_gen >= (1u << 23)) {                                // the tag (gen << 8 | level) of the stat words stays below 2^32: start over
			FX_HIP(hipMemsetAsync(m->fz_tile_next, 0, (size_t)jacobi_freeze_tiles(m->g) * sizeof(uint32_t), ms));
			FX_HIP(hipMemsetAsync(m->fz_stat, 0, kFreezeStatRing * sizeof(uint32_t), ms));
			FX_HIP(hipMemsetAsync(m->fz_counts, 0, 2 * jacobi_freeze_count_words() * sizeof(uint32_t), ms));
			m->fz_gen = 2; m->fz_gen_mark = 0;
		}
		Run& r = R[i];
		int first = 0;
		r.v = jacobi_freeze_view(m->g, &first, &r.own0);
		r.off = (size_t)first * m->g.plane();
		r.moff = (size_t)first * (size_t)((m->g.X + 3) / 4) * m->g.Y;
		const uint32_t gen = m->fz_gen;
		r.stat_hi = gen << 8;
		r.stat = m->fz_stat + gen % kFreezeStatRing;
		m->fz_iters[gen % kFreezeStatRing] = iters;
		const size_t cw = jacobi_freeze_count_words(), es = elem_size(m);
		r.w = FreezeWork{ m->fz_tile_next, gen, { m->fz_list[0], m->fz_list[1] }, jacobi_freeze_tiles(m->g),
			m->fz_counts + (gen & 1u) * cw, m->fz_counts + ((gen & 1u) ^ 1u) * cw };
		r.src = m->p[m->p_cur]; r.a = m->p[m->p_cur ^ 1]; r.d = m->p_aux;
		r.ma = m->fz_mask[0]; r.md = m->fz_mask[1]; r.mx = m->fz_mask[2];
		// the strip launches in use follow the count k_count_marks put into a host-visible word behind an earlier solve's dense sweep;
		// decided HERE because the dense sweep itself depends on what follows it
		int forced;
		const int width = freeze_strip_width(m->g, multi, m->fz_mask[2] != nullptr, &forced);
		const bool adaptive = width && forced < 0 && m->fz_active_dev;      // the count of relaxing tiles decides how many strip launches
		const FreezeCadence cadence = freeze_cadence(gen);
		if (adaptive && cadence.take_over && m->fz_active_pending) {
			FX_HIP(hipEventSynchronize(m->fz_active_ev));
			m->fz_active_pending = false;
			m->fz_dense_n = freeze_strip_hysteresis(m->fz_dense_n, *(volatile uint32_t*)m->fz_active_host, (uint32_t)jacobi_freeze_tiles(m->g), width == 4);
		}
		launches = freeze_plan(m->g, iters, multi, m->fz_mask[2] != nullptr, adaptive ? m->fz_dense_n : 0, plan);
		if (!launches) return FX_E_STATE;                               // (takes_sparse_solver admits no solve whose launches outnumber the counters)
		const bool one_copy = plan[0].kind == FZ_DENSE_ONE;
		mk[i].reset(new ScopedMark(m, ms, MK_JACOBI));
		FX_HIP(launch_freeze_dense(r.v, r.src + r.off, m->b + r.off, r.a + r.off, one_copy ? nullptr : r.d + r.off, r.ma + r.moff, one_copy ? nullptr : r.md + r.moff, r.w, ms,
			fuse ? (const char*)m->vel[1] + r.off * es : nullptr, m->half, r.own0, m->g.nz, m->g.cells_local()));
		mk[i]->launches = 1; mk[i]->sweeps = 1;
		if (multi || iters == 1) mk[i].reset(); else mk[i]->split(MK_JACOBI_TAIL);
		if (adaptive && cadence.count) {                                   // (single domain: no exchange stands between the dense sweep and this)
			FX_HIP(launch_count_marks(r.w.tile_mark, gen, jacobi_freeze_tiles(m->g), m->fz_active_dev, ms));
			if (!m->fz_active_ev) FX_HIP(hipEventCreateWithFlags(&m->fz_active_ev, hipEventDisableTiming));
			FX_HIP(hipEventRecord(m->fz_active_ev, ms));
			m->fz_active_pending = true;
		}
	}
	auto exchange = [&](bool with_b) -> int {
		if (!multi) return FX_OK;
		for (size_t i = 0; i < M.size(); ++i) { M[i]->fz_x_p = R[i].a; M[i]->fz_x_m = R[i].ma; }
		const ExchSpec specs[2] = { { EX_FREEZE, kFreezeHalo, 0 }, { EX_DIV, kFreezeHalo, 0 } };
		return do_exchange(lead, M, specs, with_b ? 2 : 1, ON_COMPUTE, s);
	};
	int rc = exchange(true);                                            // level 1 and the divergence across the faces
	if (rc) return rc;
	uint32_t flag_tag = 0;                                              // what the last strip launch wrote into the tile marks, for the first tile launch
	for (int j = 1, n = 0; j < launches; ++j) {
		const FreezeLaunch& l = plan[j];
		const bool strip = l.kind == FZ_STRIP;
		if (strip) flag_tag = R[0].w.gen | ((uint32_t)j << 24);
		for (size_t i = 0; i < M.size(); ++i) {
			fx_ctx* m = M[i];
			Run& r = R[i];
			DeviceGuard dg(m->device);
			if (!mk[i]) mk[i].reset(new ScopedMark(m, CS(m, s), MK_JACOBI_TAIL));
			if (strip)                                                      // reads (a, ma), leaves level base + levels in (d, src) and (md, mx)
				FX_HIP((l.levels == 4 ? launch_freeze_strip4 : launch_freeze_strip3)(r.v, r.a, m->b, r.d, r.src, r.ma, r.md, r.mx, r.w.tile_mark, flag_tag, r.stat, r.stat_hi, l.base, CS(m, s)));
			else
				FX_HIP(launch_freeze_tiles(r.v, r.a + r.off, m->b + r.off, r.d + r.off, r.ma + r.moff, r.md + r.moff, r.w, n, l.levels, l.base, r.stat, r.stat_hi, CS(m, s), r.own0, m->g.nz, n == 0 ? flag_tag : 0u));
			m->acc.freeze_strip_launches += strip;                          // (counted like the solves: with or without the timing marks)
			mk[i]->launches += 1; mk[i]->sweeps += (uint64_t)l.levels;
			if (multi) mk[i].reset();
			freeze_rotate(r.a, r.d, r.src, strip);
			freeze_rotate(r.ma, r.md, r.mx, strip);
		}
		if (!strip) ++n;
		if ((rc = exchange(false))) return rc;                          // the levels just made, kFreezeHalo planes deep (the last one serves the projection)
	}
	mk.clear();
	for (size_t i = 0; i < M.size(); ++i) { fx_ctx* m = M[i]; m->p[0] = R[i].a; m->p[1] = R[i].d; m->p_aux = R[i].src; m->fz_mask[0] = R[i].ma; m->fz_mask[1] = R[i].md; m->fz_mask[2] = R[i].mx; m->p_cur = 0; }
	return FX_OK;
}

// exchange, then k sweeps, exchange, ... on one stream
static int jacobi_serial(fx_ctx* lead, std::vector<fx_ctx*>& M, hipStream_t s, uint32_t iters)
{
	const bool multi = multi_rank(lead);
	const int k = multi ? lead->opt_round : (int)iters;
	int rc;
	if (takes_sparse_solver(lead, iters)) return jacobi_freeze(lead, M, s, iters);
	for (fx_ctx* m : M) { std::vector<fx_ctx*> one{ m }; if ((rc = clear_freeze_masks(one, CS(m, s)))) return rc; }
	const ExchSpec bspec{ EX_DIV, k - 1, 0 };
	if ((rc = do_exchange(lead, M, &bspec, 1, ON_COMPUTE, s))) return rc;
	uint32_t done = 0;
	while (done < iters) {
		const int cnt = (int)std::min<uint32_t>(k, iters - done);
		const ExchSpec pspec{ EX_PRESSURE, cnt, lead->p_cur };
		if ((rc = do_exchange(lead, M, &pspec, 1, ON_COMPUTE, s))) return rc;
		for (fx_ctx* m : M) {
			ScopedMark mk(m, CS(m, s), MK_JACOBI);
			if ((rc = jacobi_round(m, CS(m, s), cnt, &mk))) return rc;
		}
		done += cnt;
	}
	const ExchSpec last{ EX_PRESSURE, 1, lead->p_cur };          // the projection's z-gradient reads one plane across the face
	return do_exchange(lead, M, &last, 1, ON_COMPUTE, s);
}

// Rounds of up to k sweeps with the pressure exchange of a round hidden behind its interior sweeps, on three streams.
// With lo/hi = the owned planes, src = the buffer holding the round's level 0 (k halo planes valid), cnt <= k sweeps in the
// round, done as m launches of t_1 <= t_2 = ... = t_m fused sweeps (c_j = t_1 + ... + t_j, rem_j = cnt - c_j):
//   face stream   the FACE CHAIN: cnt single sweeps over both face zones per launch, level s on [lo - (cnt - s), lo + k + (cnt - s))
//                 (mirrored at hi), entirely in two scratch buffers (only its first sweep reads src): thin, latency-bound
//                 launches that run BESIDE the interior instead of in front of it.  Its last level holds the k planes the
//                 neighbour needs.
//   comm stream   after the chain: those k planes leave from the scratch buffer, the neighbour's land in the halo of the
//                 round's last buffer (which no interior launch touches)
//   compute       the INTERIOR, self-sufficient: launch j brings [lo + k - rem_j, hi - k + rem_j) from level c_(j-1) to c_j,
//                 i.e. it recomputes the rem_j planes per side the chain also computes instead of waiting for them (it never
//                 reads below lo + k - cnt >= lo, so it needs no halo).  Launch 2 overwrites src and therefore waits until
//                 the chain's first sweep has read it; after the last launch the chain's k final planes are copied from the
//                 scratch buffer into [lo, lo + k) of the round's last buffer, which completes the owned planes.
// Per round the critical path is max(interior, chain + link) instead of chain + max(interior, link).  Every cell gets the
// arithmetic of the single-domain sweep; (cell, level) pairs of the zone borders are computed twice, which is why the
// faithful mode (its freeze mask is a side effect) takes the serial schedule instead.
// pol: the lead's policy, then every member's; t = jacobi_group_sweeps of them
static int jacobi_overlapped(fx_ctx* lead, std::vector<fx_ctx*>& M, hipStream_t s, uint32_t iters, const std::vector<JacobiPolicy>& pol, int t, int k)
{
	fx_comm_group* grp = lead->group;
	int rc;
	fx_ctx* ctx = lead;                                    // FX_HIP / FX_LANES report through `ctx`
	// The face chain runs one single-sweep launch (k_jacobi_v4: 60 registers, both faces) per level.  Groups of fused sweeps with the
	// interior's register-strip kernels were built and measured slower (loop-back N = 4, 256^3 per rank, rounds of 9: 6.30 against 5.67 ms
	// per step; docs/LAB.md): on a 9..27-plane zone the strips have 64..192 waves whose 310 registers shut
	// the interior's waves out of their SIMDs for a whole 14-step pipeline -- removed in round 3.
	const ExchSpec first[2] = { { EX_DIV, k - 1, 0 }, { EX_PRESSURE, k, lead->p_cur } };
	if ((rc = do_exchange(lead, M, first, 2, ON_COMPUTE, s))) return rc;
	FX_LANES(FX_HIP(hipEventRecord(L.lane->ev_int, L.compute)););
	bool in_flight = false;
	uint32_t done = 0;
	while (done < iters) {
		const int cnt = (int)std::min<uint32_t>(k, iters - done);
		// the interior's launches: the remainder first, then whole t's (jacobi_group_parts: the same list on every member)
		std::vector<int> parts(cnt);
		const int m = jacobi_group_parts(pol[0], t, cnt, parts.data());
		// (every member from ITS OWN current buffer: members that ran serial rounds before -- the schedule is an option at run time -- may
		// hold their pressure in different buffers; SRC / FIN below are per member)
		const int flip = m & 1;
#define FX_SRC(c_) ((c_)->p_cur)
#define FX_FIN(c_) ((c_)->p_cur ^ flip)
		int fbuf = 0;                                      // which scratch buffer holds the chain's last level (set below)
		// ---- face stream: the chain (needs the previous round's interior + face copy, and its exchange)
		FX_LANES(FX_HIP(hipStreamWaitEvent(L.lane->face, L.lane->ev_int, 0)); if (in_flight) FX_HIP(hipStreamWaitEvent(L.lane->face, L.lane->ev_done, 0)););
		ScopedMark chain_mark(lead, grp->lane_of(lead).face, MK_CHAIN);         // one mark per chain (shared stream: all members' chains, booked on the first)
		{
			// the chain: one sweep per launch over the two thin face zones
			int grp_i = 0;
			for (int c = 1; c <= cnt; ++c, ++grp_i) {
				const int rem = cnt - c, ob = (grp_i + 1) & 1;
				for (fx_ctx* mctx : M) {
					if (!has_lower(mctx) && !has_upper(mctx)) continue;
					DeviceGuard dg(mctx->device);
					const Range o = owned(mctx);
					const float* in = grp_i == 0 ? mctx->p[FX_SRC(mctx)] : mctx->p_face[grp_i & 1];
					const Range lo{ o.lo - rem, has_lower(mctx) ? o.lo + k + rem : o.lo - rem };
					const Range hi{ has_upper(mctx) ? o.hi - k - rem : o.hi + rem, o.hi + rem };
					FX_HIP(launch_jacobi_sweep2(mctx->g, in, mctx->b, mctx->p_face[ob], nullptr, lo.lo, lo.hi, hi.lo, hi.hi, grp->lane_of(mctx).face));
				}
				if (grp_i == 0) FX_LANES(FX_HIP(hipEventRecord(L.lane->ev_face1, L.lane->face)););
			}
			fbuf = grp_i & 1;                                  // the buffer the last group wrote
		}
		// ---- comm stream: the k final planes of the chain travel, the neighbour's land in the halo of p[fin]
		FX_LANES(FX_HIP(hipEventRecord(L.lane->ev_ready, L.lane->face)); FX_HIP(hipStreamWaitEvent(L.lane->comm, L.lane->ev_ready, 0)););
		const ExchSpec pspec{ EX_PRESSURE_FACE, k, (fbuf << 1) | flip };      // (bit 0: the receiving buffer relative to the member's current one)
		if ((rc = do_exchange(lead, M, &pspec, 1, ON_COMM, s))) return rc;
		if ((rc = comm_mark_done(lead, M, s))) return rc;
		in_flight = true;
		// ---- compute stream: the interior
		for (size_t i = 0; i < M.size(); ++i) {
			fx_ctx* mctx = M[i];
			ScopedMark mk(mctx, CS(mctx, s), MK_JACOBI);
			const Range o = owned(mctx);
			int lvl = 0, cur = FX_SRC(mctx);
			for (int j = 0; j < m; ++j) {
				const int tj = parts[j];
				lvl += tj;
				const int rem = cnt - lvl;
				const Range in{ has_lower(mctx) ? o.lo + k - rem : o.lo, has_upper(mctx) ? o.hi - k + rem : o.hi };
				if (j == 1 && (grp->per_member || mctx == M.front())) {      // launch 2 overwrites the chain's input
					DeviceGuard dg(mctx->device);
					FX_HIP(hipStreamWaitEvent(CS(mctx, s), grp->lane_of(mctx).ev_face1, 0));
				}
				if ((rc = jacobi_launch(mctx, CS(mctx, s), cur, JacobiLaunch{ pol[i + 1].fam[std::min(tj, 4)], tj }, in, &mk))) return rc;
				cur ^= 1;
			}
		}
		// the chain's final planes complete the owned range of p[fin]
		FX_LANES(FX_HIP(hipStreamWaitEvent(L.compute, L.lane->ev_ready, 0)););
		for (fx_ctx* mctx : M) {
			DeviceGuard dg(mctx->device);
			const size_t pl = mctx->g.plane(), kb = (size_t)k * pl * 4;
			const Range o = owned(mctx);
			if (has_lower(mctx))
				FX_HIP(launch_copy_bytes(mctx->p[FX_FIN(mctx)] + (size_t)mctx->g.lz(o.lo) * pl, mctx->p_face[fbuf] + (size_t)mctx->g.lz(o.lo) * pl, kb, CS(mctx, s)));
			if (has_upper(mctx))
				FX_HIP(launch_copy_bytes(mctx->p[FX_FIN(mctx)] + (size_t)mctx->g.lz(o.hi - k) * pl, mctx->p_face[fbuf] + (size_t)mctx->g.lz(o.hi - k) * pl, kb, CS(mctx, s)));
			mctx->p_cur = FX_FIN(mctx);
		}
		FX_LANES(FX_HIP(hipEventRecord(L.lane->ev_int, L.compute)););
		done += cnt;
	}
	if (in_flight) rc = comm_join(lead, M, s);
	return rc;
#undef FX_SRC
#undef FX_FIN
}

// With obstacles set or a wall open (a whole-grid context in fixed mode: fx_set_obstacles and fx_set_open_walls refuse the others) the solve is
// `iters` single-sweep launches of the boundary-aware kernel (fx_obstacle.hip), the wide one where it applies; FX_FLAG_JACOBI_FUSE_MASK is
// ignored and the planner is not asked.  (Several such sweeps per launch, in the manner of the strip and block families, do not exist yet.)
static int jacobi_obstacle(fx_ctx* lead, hipStream_t s, uint32_t iters)
{
	fx_ctx* ctx = lead;                                                 // FX_HIP reports through `ctx`
	DeviceGuard dg(ctx->device);
	ScopedMark mk(ctx, s, MK_JACOBI);
	const Range r = owned(ctx);
	for (uint32_t i = 0; i < iters; ++i) {
		FX_HIP(launch_jacobi_bnd(ctx->g, ctx->p[ctx->p_cur], ctx->b, ctx->obst_code, ctx->p[ctx->p_cur ^ 1], ctx->open_faces, r.lo, r.hi, s));
		ctx->p_cur ^= 1;
		mk.launches += 1; mk.sweeps += 1;
	}
	return FX_OK;
}

int jacobi_all(fx_ctx* lead, std::vector<fx_ctx*>& M, hipStream_t s, uint32_t iters)
{
	if (lead->obst_code || lead->open_faces) return jacobi_obstacle(lead, s, iters);
	if (overlap_level(lead) >= 2) {
		std::vector<JacobiPolicy> pol{ policy_of(lead) };
		for (fx_ctx* m : M) pol.push_back(policy_of(m));
		const int k = lead->opt_round;
		// two face zones (<= 2k - 1 planes each) and an interior; decided on the thinnest slab of the chain and on the (chain-wide)
		// Jacobi mode, so that every rank takes the same branch -- the two schedules exchange different things
		const bool ok = lead->group->lanes[0].face != nullptr && lead->group->min_nz >= 4 * k && lead->p_face[0] && !lead->frozen;
		if (ok) return jacobi_overlapped(lead, M, s, iters, pol, jacobi_group_sweeps(pol.data(), (int)pol.size()), k);
	}
	return jacobi_serial(lead, M, s, iters);
}


// FX_PRESSURE_MULTIGRID (a whole-grid context in fixed mode with closed walls and no obstacles: fx_set_pressure_solver refuses the others):
// `cycles` V-cycles on the pyramid of ctx->mg, level 0 = p[] / b.  A sweep flips a level's ping-pong; the first sweep on a coarse level reads
// no input (all +0), and with no pre-sweeps there the correction is cleared by a memset instead.  From level mg.tail down one launch runs the
// rest of the cycle (fx_multigrid.hip: k_mg_tail) unless FX_MG_NO_TAIL asks for the launches per level.  One mark over the whole solve:
// launches counts everything enqueued, sweeps the level-0 sweeps
namespace {
struct MgRun {
	fx_ctx* ctx; hipStream_t s; ScopedMark* mk; int is3d, tail;
	float* cur(int l) const { return l ? ctx->mg_e[l][ctx->mg_cur[l]] : ctx->p[ctx->p_cur]; }
	float* other(int l) const { return l ? ctx->mg_e[l][ctx->mg_cur[l] ^ 1] : ctx->p[ctx->p_cur ^ 1]; }
	float* rhs(int l) const { return l ? ctx->mg_b[l] : ctx->b; }
	void flip(int l) const { if (l) ctx->mg_cur[l] ^= 1; else ctx->p_cur ^= 1; }
	// `n` sweeps on level l; fresh: the level's correction is all +0 and stored nowhere yet
	int smooth(int l, uint32_t n, bool fresh) const
	{
		const fx::MgDims& d = ctx->mg.lv[l];
		for (uint32_t i = 0; i < n; ++i) {
			FX_HIP(fx::launch_mg_smooth(d, is3d, fresh && !i ? nullptr : cur(l), rhs(l), other(l), ctx->solver.omega, s));
			flip(l);
			mk->launches += 1;
			if (!l) mk->sweeps += 1;
		}
		if (fresh && !n) { FX_HIP(hipMemsetAsync(cur(l), 0, d.cells() * sizeof(float), s)); mk->launches += 1; }
		return FX_OK;
	}
	int cycle(int l) const
	{
		const fx_pressure_solver& ps = ctx->solver;
		int rc;
		if (l == ctx->mg.levels - 1) return smooth(l, ps.coarse_sweeps, l > 0);
		if ((rc = smooth(l, ps.pre_sweeps, l > 0))) return rc;
		FX_HIP(fx::launch_mg_residual_restrict(ctx->mg.lv[l], is3d, cur(l), rhs(l), rhs(l + 1), s));
		mk->launches += 1;
		if (l + 1 == tail) {
			fx::MgTailArgs a = {};
			a.first = tail; a.levels = ctx->mg.levels; a.is3d = is3d;
			a.pre = (int)ps.pre_sweeps; a.post = (int)ps.post_sweeps; a.coarse = (int)ps.coarse_sweeps; a.omega = ps.omega;
			for (int k = tail; k < ctx->mg.levels; ++k) { a.lv[k] = ctx->mg.lv[k]; ctx->mg_cur[k] = 0; a.e[k] = ctx->mg_e[k][0]; a.b[k] = ctx->mg_b[k]; }
			FX_HIP(fx::launch_mg_tail(a, ctx->mg.tail_floats, s));
			mk->launches += 1;
		} else if ((rc = cycle(l + 1))) return rc;
		FX_HIP(fx::launch_mg_prolong_correct(ctx->mg.lv[l], is3d, cur(l), cur(l + 1), s));
		mk->launches += 1;
		return smooth(l, ps.post_sweeps, false);
	}
};
}  // namespace

static int multigrid_solve(fx_ctx* ctx, hipStream_t s)
{
	if (!ctx->mg_mem && ctx->mg.levels > 1) { ctx->last_error = "multigrid solve without its pyramid"; return FX_E_STATE; }
	DeviceGuard dg(ctx->device);
	ScopedMark mk(ctx, s, MK_JACOBI);
	const MgRun run{ ctx, s, &mk, ctx->g.Zg > 1 ? 1 : 0, (ctx->solver.flags & FX_MG_NO_TAIL) ? 0 : ctx->mg.tail };
	for (uint32_t c = 0; c < ctx->solver.cycles; ++c)
		if (const int rc = run.cycle(0)) return rc;
	return FX_OK;
}

int pressure_solve_all(fx_ctx* lead, std::vector<fx_ctx*>& M, hipStream_t s)
{
	if (lead->solver.kind == FX_PRESSURE_MULTIGRID) return multigrid_solve(lead, s);
	return jacobi_all(lead, M, s, lead->desc.jacobi_iters);
}


int project_phase(fx_ctx* ctx, hipStream_t s)
{
	DeviceGuard dg(ctx->device);
	const SimParams sp{ ctx->time_step, (int)ctx->desc.advect_address, ctx->g.Zg > 1 ? 1 : 0, 1 };
	ScopedMark mk(ctx, s, MK_PROJECT);
	const Range r = owned(ctx);
	int* rec = multi_rank(ctx) ? ctx->step_rec : nullptr;           // slab ranks: the projection also measures the next advection's need
	ctx->rec_in_project = false;
	if (ctx->obst_code || ctx->open_faces) {                        // obstacles (resting or moving), open walls or both: the boundary-aware projection
		const int bodies = ctx->obst_code ? (int)ctx->obst_bodies.size() : 0;       // without a mask the list is idle
		FX_HIP(launch_project_bnd(ctx->g, sp, ctx->half, ctx->vel[1], ctx->p[ctx->p_cur], ctx->obst_code, ctx->obst_bodies.data(), bodies,
			ctx->vel[0], ctx->open_faces, r.lo, r.hi, s));
		return FX_OK;
	}
	FX_HIP(launch_project(ctx->g, sp, ctx->half, ctx->vel[1], ctx->p[ctx->p_cur], ctx->vel[0], r.lo, r.hi, s,
		rec, rec ? options_digest(ctx) : 0, ctx->halo_overflow, &ctx->rec_in_project));
	return FX_OK;
}

// Tracer particles (fx_particles.hip): behind the projection, every live record takes one step through velocity[0], the field the projection has
// just written; while spawners are set (fx_particle_spawn.hip) the births follow.  The move is one launch over the records, in place; it reads the velocity, the obstacle code and the open-wall bits and writes the particle
// buffer alone, so no field of the step knows of it.  Nothing is allocated, copied or waited for here (fx_set_particles did all of that).  Booked
// with the projection: fx_timing has no mark of its own for it.
int particles_phase(fx_ctx* ctx, hipStream_t s)
{
	if (!ctx->part || !(ctx->time_step > 0.0f)) return FX_OK;
	DeviceGuard dg(ctx->device);
	ScopedMark mk(ctx, s, MK_PROJECT);
	// the sort, when this run is due one (fx_set_particle_sort's `every`: the 1st, (n+1)th ... run of this stage), in front of the move: the step
	// that pays for it gets the coherent gathers.  Decided here, at enqueue time: a captured step replays what was captured
	if (ctx->psort_mem && ctx->psort_cfg.every) {
		const bool due = ctx->psort_runs % ctx->psort_cfg.every == 0;
		++ctx->psort_runs;
		if (due) {
			FX_HIP(launch_particle_sort(ctx->g, ctx->psort, ctx->part, ctx->psort_mem, s));
			++ctx->psort_sorts;
		}
	}
	FX_HIP(launch_move_particles(ctx->g, ctx->half, ctx->part_prm, ctx->vel[0], ctx->obst_code, ctx->open_faces, ctx->time_step, ctx->part, ctx->part_count, s));
	// the births behind the move: a record born now sits on its spawn point when the step ends and moves from the next step on
	if (ctx->spawn_mem) FX_HIP(launch_spawn_particles(ctx->g, ctx->spawn, (uint32_t)ctx->spawners.size(), ctx->time_step, ctx->part, ctx->obst_code, ctx->spawn_mem, s));
	return FX_OK;
}

// The particle spawners alone (fx_particle_spawn.hip): the dead counted per workgroup and scanned, the rates ticked, the births placed into
// dead slots in index order.  dt is the kernel argument taken here, at enqueue, like every other stage's; how many records a run bears is
// decided on the device, so a captured run replayed keeps the rate.  Enqueues only (fx_set_particle_spawners and fx_set_particles did the
// allocating); booked with the projection like the move.
int spawn_phase(fx_ctx* ctx, hipStream_t s)
{
	if (!ctx->spawn_mem) return FX_E_STATE;
	if (!ctx->part || !(ctx->time_step > 0.0f)) return FX_OK;
	DeviceGuard dg(ctx->device);
	ScopedMark mk(ctx, s, MK_PROJECT);
	FX_HIP(launch_spawn_particles(ctx->g, ctx->spawn, (uint32_t)ctx->spawners.size(), ctx->time_step, ctx->part, ctx->obst_code, ctx->spawn_mem, s));
	return FX_OK;
}

// The particle sort alone (fx_particle_sort.hip): the records by cell, the dead last, order and live left in the scratch block.  Enqueues only.
int sort_particles_phase(fx_ctx* ctx, hipStream_t s)
{
	if (!ctx->psort_mem) return FX_E_STATE;
	if (!ctx->part) return FX_OK;
	DeviceGuard dg(ctx->device);
	ScopedMark mk(ctx, s, MK_PROJECT);
	FX_HIP(launch_particle_sort(ctx->g, ctx->psort, ctx->part, ctx->psort_mem, s));
	++ctx->psort_sorts;
	return FX_OK;
}

// The optional stages between the advection and the divergence, each a no-op unless its feature is set (whole-grid contexts only: the setters
// refuse slab ranks).  The order is the contract, every phase's own comment gives its half of it: the inflow pass scales what the advection
// sampled, before the emitters add to it; buoyancy reads the alpha the emitters added; the enforce pass clears the solid cells of everything
// added so far; the confinement comes last because it writes into velocity[0], the field the inflow pass and buoyancy trace with.  The
// particle trail stands behind buoyancy, whose force it does not enter, and in front of the enforce pass.
static int (*const kOptionalStages[])(fx_ctx*, hipStream_t) = { open_inflow_phase, emit_phase, heat_phase, trail_phase, enforce_phase, confine_phase };

int simulate_impl(fx_ctx* ctx, hipStream_t s)
{
	std::vector<fx_ctx*> M;
	for_members(ctx, M);
	int rc;
	if ((rc = advect_all(ctx, M, s))) return rc;
	if (overlap_level(ctx) >= 3) {
		// colour[parity] is final for this step: its halo planes -- four of the seven plane-units the next advection needs --
		// leave now on the side stream, behind divergence / pressure / projection
		FX_LANES(FX_HIP(hipEventRecord(L.lane->ev_col_ready, L.compute)); FX_HIP(hipStreamWaitEvent(L.lane->comm, L.lane->ev_col_ready, 0)););
		const ExchSpec cs{ EX_COLOR_CUR, (int)ctx->desc.halo_advect, 0 };
		if ((rc = do_exchange(ctx, M, &cs, 1, ON_COMM, s, 1))) return rc;           // side channel: not queued with the step's own exchanges
		FX_LANES(FX_HIP(hipEventRecord(L.lane->ev_col_done, L.lane->comm)););
		for (fx_ctx* m : M) m->col_halo_buf = (int)m->frame_parity;
	}
	if (ctx->time_step > 0.0f) {                       // CSProject3D.hlsl:88
		for (const auto stage : kOptionalStages)
			for (fx_ctx* m : M) if ((rc = stage(m, CS(m, s)))) return rc;
		const ExchSpec uz{ EX_UZ1, 1, 0 };
		if ((rc = do_exchange(ctx, M, &uz, 1, ON_COMPUTE, s))) return rc;
		if (takes_sparse_solver(ctx, ctx->desc.jacobi_iters) && jacobi_freeze_can_fuse_divergence(ctx->g)) ctx->fz_fuse_div = true;   // k_freeze_dense computes it
		else for (fx_ctx* m : M) if ((rc = divergence_phase(m, CS(m, s)))) return rc;
		rc = pressure_solve_all(ctx, M, s);
		ctx->fz_fuse_div = false;                      // (consumed by the dense sweep; never left standing for a later stage call)
		if (rc) return rc;
		for (fx_ctx* m : M) if ((rc = project_phase(m, CS(m, s)))) return rc;
		for (fx_ctx* m : M) if ((rc = particles_phase(m, CS(m, s)))) return rc;    // (one null test per member while no set exists)
	} else {
		for (fx_ctx* m : M) {
			DeviceGuard dg(m->device);
			m->rec_in_project = false;
			if (launch_copy_velocity(m->g, m->half, m->vel[1], m->vel[0], CS(m, s)) != hipSuccess) return FX_E_DEVICE;
		}
	}
	if ((rc = record_step(ctx, M, s))) return rc;
	for (fx_ctx* m : M) { if (m->timing_on) m->acc.steps += 1; if (ctx->time_step > 0.0f) m->steps_simulated += 1; }
	return FX_OK;
}

}  // namespace fxh
