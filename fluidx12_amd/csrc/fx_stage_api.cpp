// fx_stage_api.cpp -- the entry points of the step's optional stages (include/fluidx_hip.h): vorticity confinement, emitters, obstacles with
// their bodies and meshes, open walls, buoyancy, tracer particles with their sort, trail, spawners and draw, the obstacle draw, the advection scheme and the pressure solver --
// each stage's setter, getter and its phase of the step (fx_schedule.cpp) on its own.  A setter that owns device memory builds the new
// buffers beside the ones in force (DevBuf, fx_host.h) and commits in its last lines.  The per-frame calls: fx_api.cpp.
#include "fx_host.h"
#include "fx_mesh_args.h"

using namespace fx;
using namespace fxh;

// Their calls want a context that simulates and, unless `whole` is false (the getters), holds the whole grid: FX_E_INVALID for null, FX_E_STATE for a render-only one,
// FX_E_INVALID for a slab or a rank of a chain -- each stage would need halo planes of its own there (the confinement two of velocity[1] across
// each face, the temperature a field's worth; the colour halos leave right behind the advection, in front of the passes that change it).
// A context never fails both of the last two tests: fx_create refuses a render-only slab, check_slab_chain a whole grid in a chain.
static int sim_guard(const fx_ctx* ctx, bool whole = true)
{
	if (!ctx) return FX_E_INVALID;
	if (ctx->desc.flags & FX_FLAG_RENDER_ONLY) return FX_E_STATE;
	if (whole && (ctx->g.nz != ctx->g.Zg || ctx->nranks > 1)) return FX_E_INVALID;
	return FX_OK;
}

// fx_<stage>(ctx, stream): the stage's phase of the step (fx_schedule.cpp) on its own
static int run_stage(fx_ctx* ctx, void* stream, int (*phase)(fx_ctx*, hipStream_t))
{
	const int rc = sim_guard(ctx);
	return rc ? rc : phase(ctx, pick_stream(ctx, stream));
}

// The host-side lists (emitters, heat sources, bodies): at most `limit` records, each passing `status` (FX_OK / FX_E_INVALID), replace `v`;
// the getter hands out the first `capacity` of them and the count
template <class T, class Status> static int set_list(std::vector<T>& v, const T* list, uint32_t count, uint32_t limit, Status status)
{
	if (count > limit || (count && !list)) return FX_E_INVALID;
	for (uint32_t k = 0; k < count; ++k) if (const int rc = status(list[k])) return rc;
	v.assign(list, list + count);
	return FX_OK;
}

template <class T> static int get_list(const std::vector<T>& v, T* out, uint32_t capacity, uint32_t* count)
{
	if (!count || (capacity && !out)) return FX_E_INVALID;
	*count = (uint32_t)v.size();
	for (uint32_t k = 0; k < capacity && k < *count; ++k) out[k] = v[k];
	return FX_OK;
}

// a setting held in the context as the struct the getter hands out (slab ranks may ask: the default there)
template <class T> static int get_setting(const fx_ctx* ctx, T fx_ctx::*setting, T* out)
{
	if (const int rc = sim_guard(ctx, false)) return rc;
	if (!out) return FX_E_INVALID;
	*out = ctx->*setting;
	return FX_OK;
}

extern "C" {

int fx_set_vorticity_confinement(fx_ctx* ctx, float epsilon)
{
	if (!std::isfinite(epsilon) || epsilon < 0.0f) return FX_E_INVALID;
	if (const int rc = sim_guard(ctx)) return rc;
	ctx->vort_eps = epsilon;
	return FX_OK;
}

int fx_confine_vorticity(fx_ctx* ctx, void* stream) { return run_stage(ctx, stream, confine_phase); }

int fx_set_emitters(fx_ctx* ctx, const fx_emitter* list, uint32_t count)
{
	if (const int rc = sim_guard(ctx)) return rc;
	return set_list(ctx->emitters, list, count, FX_MAX_EMITTERS, [](const fx_emitter& e) -> int {
		if (e.struct_size != sizeof(fx_emitter) || e.flags != 0) return FX_E_INVALID;
		if (!std::isfinite(e.radius) || !(e.radius > 0.0f) || !std::isfinite(e.swirl)) return FX_E_INVALID;
		for (int a = 0; a < 3; ++a) if (!std::isfinite(e.center[a]) || !std::isfinite(e.force[a])) return FX_E_INVALID;
		for (int a = 0; a < 4; ++a) if (!std::isfinite(e.color_rate[a]) || e.color_rate[a] < 0.0f) return FX_E_INVALID;
		return FX_OK;
	});
}

int fx_get_emitters(fx_ctx* ctx, fx_emitter* out, uint32_t capacity, uint32_t* count)
{
	if (const int rc = sim_guard(ctx, false)) return rc;             // (slab ranks may ask: the list is empty there)
	return get_list(ctx->emitters, out, capacity, count);
}

int fx_set_impulse(fx_ctx* ctx, int enabled)
{
	if (const int rc = sim_guard(ctx, !enabled)) return rc;           // off: on the emitters' footing -- without it a slab rank has no source
	ctx->impulse_on = enabled != 0;
	return FX_OK;
}

int fx_emit(fx_ctx* ctx, void* stream) { return run_stage(ctx, stream, emit_phase); }

// ---- solid obstacles (fx_obstacle.hip) ------------------------------------------------------------------
// the tail the two mask setters share: the 0 / 1 bytes at `src` (device memory) become the code volume in obst_spare, the count and the box come
// back, and the new volume takes the place of the one in force.  obst_spare and obst_stats are allocated; blocks until `src` has been read
static int install_obstacle_mask(fx_ctx* ctx, const uint8_t* src, hipStream_t s)
{
	FX_HIP(launch_obstacle_codes(ctx->g, src, ctx->obst_spare, ctx->obst_stats, s));
	unsigned st[8];
	FX_HIP(hipMemcpyAsync(st, ctx->obst_stats, sizeof st, hipMemcpyDeviceToHost, s));
	FX_HIP(hipStreamSynchronize(s));                                        // the count and the box size the enforce launch; `solid` is free again
	std::swap(ctx->obst_code, ctx->obst_spare);
	++ctx->obst_gen;                                                        // (the obstacle draw packs its bricks anew)
	ctx->obst_cells = (uint64_t)st[0] | ((uint64_t)st[1] << 32);
	for (int a = 0; a < 3; ++a) {
		ctx->obst_lo[a] = ctx->obst_cells ? (int)st[2 + a] : 0;
		ctx->obst_hi[a] = ctx->obst_cells ? (int)st[5 + a] + 1 : 0;
	}
	return FX_OK;
}

int fx_set_obstacles(fx_ctx* ctx, void* stream, const uint8_t* solid, size_t bytes, uint32_t flags)
{
	if (const int rc = sim_guard(ctx)) return rc;
	if (flags & ~(uint32_t)FX_OBSTACLES_DEVICE) return FX_E_INVALID;
	if (ctx->desc.jacobi_mode == FX_JACOBI_FAITHFUL) return FX_E_INVALID;  // the per-cell freeze solve has no obstacle-aware kernels
	DeviceGuard dg(ctx->device);
	if (!solid) {                                                           // detach: every launch is the plain one again
		if (ctx->obst_code) {
			if (const int rc = dev_free(ctx, &ctx->obst_spare)) return rc;      // (waits for the device: nothing reads the volume any more)
			std::swap(ctx->obst_spare, ctx->obst_code);
		}
		ctx->obst_cells = 0;
		++ctx->obst_gen;
		return FX_OK;
	}
	if (ctx->solver.kind == FX_PRESSURE_MULTIGRID) return FX_E_STATE;          // the multigrid solve has no coarse code volumes
	const size_t n = ctx->g.plane() * (size_t)ctx->g.Zg;
	if (bytes != n) return FX_E_INVALID;
	hipStream_t s = pick_stream(ctx, stream);
	// the new code volume is built beside the one in force, which stays in force if anything below fails
	if (const int rc = dev_keep(ctx, &ctx->obst_spare, n)) return rc;
	if (const int rc = dev_keep(ctx, &ctx->obst_stats, 8 * sizeof(unsigned))) return rc;
	const uint8_t* src = solid;
	if (!(flags & FX_OBSTACLES_DEVICE)) {
		if (const int rc = ensure_stage(ctx, n)) return rc;
		FX_HIP(hipMemcpyAsync(ctx->stage, solid, n, hipMemcpyHostToDevice, s));
		src = reinterpret_cast<const uint8_t*>(ctx->stage);
	}
	return install_obstacle_mask(ctx, src, s);
}

int fx_get_obstacles(fx_ctx* ctx, uint8_t* solid_out, size_t bytes, uint64_t* solid_cells)
{
	if (const int rc = sim_guard(ctx, false)) return rc;
	const size_t n = ctx->g.plane() * (size_t)ctx->g.Zg;
	if (solid_out && bytes != n) return FX_E_INVALID;
	if (solid_cells) *solid_cells = ctx->obst_code ? ctx->obst_cells : 0;
	if (!solid_out) return FX_OK;
	if (!ctx->obst_code) { std::memset(solid_out, 0, n); return FX_OK; }
	DeviceGuard dg(ctx->device);
	FX_HIP(hipDeviceSynchronize());
	if (const int rc = ensure_stage(ctx, n)) return rc;
	FX_HIP(launch_obstacle_mask(ctx->obst_code, reinterpret_cast<uint8_t*>(ctx->stage), n, ctx->stream));
	FX_HIP(hipMemcpyAsync(solid_out, ctx->stage, n, hipMemcpyDeviceToHost, ctx->stream));
	FX_HIP(hipStreamSynchronize(ctx->stream));
	return FX_OK;
}

int fx_enforce_obstacles(fx_ctx* ctx, void* stream) { return run_stage(ctx, stream, enforce_phase); }

// ---- the solids' rigid-body velocities (fx_obstacle.hip): a host-side list like the emitters ---------------------------------
int fx_set_obstacle_bodies(fx_ctx* ctx, const fx_obstacle_body* list, uint32_t count)
{
	if (const int rc = sim_guard(ctx)) return rc;
	if (ctx->desc.jacobi_mode == FX_JACOBI_FAITHFUL) return FX_E_INVALID;  // on the obstacles' footing: fx_set_obstacles refuses these contexts
	return set_list(ctx->obst_bodies, list, count, FX_MAX_OBSTACLE_BODIES, [](const fx_obstacle_body& b) -> int {
		if (b.struct_size != sizeof(fx_obstacle_body) || b.flags != 0) return FX_E_INVALID;
		for (int a = 0; a < 3; ++a) {
			if (!std::isfinite(b.box_lo[a]) || !std::isfinite(b.box_hi[a]) || !std::isfinite(b.linear[a]) || !std::isfinite(b.angular[a]) ||
				!std::isfinite(b.pivot[a])) return FX_E_INVALID;
			if (b.box_lo[a] > b.box_hi[a]) return FX_E_INVALID;
		}
		return FX_OK;
	});
}

int fx_get_obstacle_bodies(fx_ctx* ctx, fx_obstacle_body* out, uint32_t capacity, uint32_t* count)
{
	if (const int rc = sim_guard(ctx, false)) return rc;             // (slab ranks may ask: the list is empty there)
	return get_list(ctx->obst_bodies, out, capacity, count);
}

// ---- the mask from triangle meshes (fx_voxelize.hip): scatter and fill per mesh into the staging buffer, then fx_set_obstacles' own tail --------
int fx_set_obstacle_meshes(fx_ctx* ctx, void* stream, const fx_obstacle_mesh* meshes, uint32_t count, fx_mesh_report* report)
{
	if (const int rc = sim_guard(ctx)) return rc;
	if (const int rc = mesh_args_status(meshes, count)) return rc;
	if (ctx->g.Zg <= 1) return FX_E_INVALID;                                // a 2-D grid has no columns to fill
	if (ctx->desc.jacobi_mode == FX_JACOBI_FAITHFUL) return FX_E_INVALID;  // as fx_set_obstacles
	if (ctx->solver.kind == FX_PRESSURE_MULTIGRID) return FX_E_STATE;
	DeviceGuard dg(ctx->device);
	const Geom& g = ctx->g;
	const size_t n = g.plane() * (size_t)g.Zg;
	hipStream_t s = pick_stream(ctx, stream);
	// everything is allocated before anything is enqueued: the mask in force stays in force if one of these fails
	if (const int rc = dev_keep(ctx, &ctx->obst_spare, n)) return rc;
	if (const int rc = dev_keep(ctx, &ctx->obst_stats, 8 * sizeof(unsigned))) return rc;
	if (const int rc = dev_keep(ctx, &ctx->vox_report, kVoxReportWords * sizeof(unsigned))) return rc;
	if (!ctx->vox_bits)                                                     // zeroed once: the fill kernel leaves it all zero
		if (const int rc = dev_alloc_zeroed(ctx, &ctx->vox_bits, (size_t)g.Y * g.Zg * voxel_row_words(g) * sizeof(unsigned), s)) return rc;
	if (const int rc = dev_grow(ctx, &ctx->vox_work, &ctx->vox_work_bytes, mesh_work_bytes(meshes, count))) return rc;
	if (const int rc = ensure_stage(ctx, n)) return rc;
	uint8_t* mask = reinterpret_cast<uint8_t*>(ctx->stage);
	FX_HIP(hipMemsetAsync(ctx->vox_report, 0, kVoxReportWords * sizeof(unsigned), s));
	for (uint32_t k = 0; k < count; ++k) {
		const fx_obstacle_mesh& m = meshes[k];
		VoxMesh vm = { m.positions, m.indices, m.transform, m.vertex_count, m.triangle_count };
		if (m.triangle_count && !(m.flags & FX_MESH_DEVICE)) {               // a host mesh: its copy lies behind the list of large triangles
			char* at = static_cast<char*>(ctx->vox_work) + (size_t)16 * m.triangle_count;
			const size_t ib = (size_t)12 * m.triangle_count, pb = (size_t)12 * m.vertex_count;
			FX_HIP(hipMemcpyAsync(at, m.indices, ib, hipMemcpyHostToDevice, s));
			vm.idx = reinterpret_cast<const uint32_t*>(at);
			if (pb) FX_HIP(hipMemcpyAsync(at + ib, m.positions, pb, hipMemcpyHostToDevice, s));
			vm.pos = reinterpret_cast<const float*>(at + ib);
			if (m.transform) {
				FX_HIP(hipMemcpyAsync(at + ib + pb, m.transform, 48, hipMemcpyHostToDevice, s));
				vm.xf = reinterpret_cast<const float*>(at + ib + pb);
			}
		}
		FX_HIP(launch_voxel_scatter(g, vm, ctx->vox_bits, ctx->vox_report, ctx->vox_report + 2 + k, static_cast<uint4*>(ctx->vox_work), s));
		if (k == 0 || m.triangle_count) FX_HIP(launch_voxel_fill(g, ctx->vox_bits, mask, k == 0, ctx->vox_report, s));
	}
	unsigned rep[2];
	FX_HIP(hipMemcpyAsync(rep, ctx->vox_report, sizeof rep, hipMemcpyDeviceToHost, s));
	if (const int rc = install_obstacle_mask(ctx, mask, s)) return rc;        // (synchronises: rep is there, the meshes are free again)
	if (report) {
		report->solid_cells = ctx->obst_cells;
		report->open_columns = rep[0];
		report->skipped_triangles = rep[1];
	}
	return FX_OK;
}

// ---- open walls (fx_open.hip) ---------------------------------------------------------------------------
int fx_set_open_walls(fx_ctx* ctx, uint32_t faces)
{
	if (const int rc = sim_guard(ctx)) return rc;
	if (!open_faces_ok(ctx->g, faces)) return FX_E_INVALID;                 // (a 2-D grid has no z faces)
	if (ctx->desc.jacobi_mode == FX_JACOBI_FAITHFUL) return FX_E_INVALID;  // the per-cell freeze solve has no open-wall kernels
	if (faces && ctx->solver.kind == FX_PRESSURE_MULTIGRID) return FX_E_STATE; // the multigrid solve knows closed walls only
	ctx->open_faces = faces;
	return FX_OK;
}

int fx_get_open_walls(fx_ctx* ctx, uint32_t* faces)
{
	if (!faces) return FX_E_INVALID;
	if (const int rc = sim_guard(ctx, false)) return rc;
	*faces = ctx->open_faces;
	return FX_OK;
}

int fx_open_inflow(fx_ctx* ctx, void* stream) { return run_stage(ctx, stream, open_inflow_phase); }

// ---- buoyancy (fx_heat.hip) -------------------------------------------------------------------------------
int fx_set_buoyancy(fx_ctx* ctx, const fx_buoyancy* b)
{
	if (const int rc = sim_guard(ctx)) return rc;
	DeviceGuard dg(ctx->device);
	if (!b) {                                                               // off: every call behaves as without this function, the field goes
		const int r0 = dev_free(ctx, &ctx->temp[0]), r1 = dev_free(ctx, &ctx->temp[1]);   // (waits for the device: nothing reads the volume any more)
		ctx->temp_cur = 0;
		ctx->buoy_on = false;
		const fx_buoyancy off = { (uint32_t)sizeof(fx_buoyancy), 0u, 0.0f, 0.0f, 0.0f, 0.0f, { 0.0f, 1.0f, 0.0f } };
		ctx->buoy = off;
		return r0 ? r0 : r1;
	}
	if (b->struct_size != sizeof(fx_buoyancy) || b->flags != 0) return FX_E_INVALID;
	if (!std::isfinite(b->ambient) || !std::isfinite(b->density_weight) || !std::isfinite(b->lift) || !std::isfinite(b->cooling)) return FX_E_INVALID;
	if (b->density_weight < 0.0f || b->cooling < 0.0f) return FX_E_INVALID;
	for (int a = 0; a < 3; ++a) if (!std::isfinite(b->up[a])) return FX_E_INVALID;
	if (b->up[0] == 0.0f && b->up[1] == 0.0f && b->up[2] == 0.0f) return FX_E_INVALID;
	if (!ctx->temp[0]) {                                                    // the first successful call: the ping-pong pair, both at the ambient value
		const size_t n = ctx->g.cells_owned();
		DevBuf t[2];
		uint32_t bits;
		std::memcpy(&bits, &b->ambient, sizeof bits);
		for (int i = 0; i < 2; ++i) {
			if (const int rc = t[i].alloc(ctx, n * sizeof(float))) return rc;
			FX_HIP(hipMemsetD32Async((hipDeviceptr_t)t[i].get(), (int)bits, n, ctx->stream));
		}
		FX_HIP(hipStreamSynchronize(ctx->stream));
		for (int i = 0; i < 2; ++i) ctx->temp[i] = t[i].release<float>();
		ctx->temp_cur = 0;
	}
	ctx->buoy = *b;
	ctx->buoy_on = true;
	return FX_OK;
}

int fx_get_buoyancy(fx_ctx* ctx, fx_buoyancy* out, int* enabled)
{
	if (const int rc = sim_guard(ctx, false)) return rc;
	if (out) *out = ctx->buoy;
	if (enabled) *enabled = ctx->buoy_on ? 1 : 0;
	return FX_OK;
}

int fx_set_heat_sources(fx_ctx* ctx, const fx_heat_source* list, uint32_t count)
{
	if (const int rc = sim_guard(ctx)) return rc;
	return set_list(ctx->heat_sources, list, count, FX_MAX_HEAT_SOURCES, [](const fx_heat_source& e) -> int {
		if (e.struct_size != sizeof(fx_heat_source) || e.flags != 0) return FX_E_INVALID;
		if (!std::isfinite(e.radius) || !(e.radius > 0.0f) || !std::isfinite(e.rate)) return FX_E_INVALID;
		for (int a = 0; a < 3; ++a) if (!std::isfinite(e.center[a])) return FX_E_INVALID;
		return FX_OK;
	});
}

int fx_get_heat_sources(fx_ctx* ctx, fx_heat_source* out, uint32_t capacity, uint32_t* count)
{
	if (const int rc = sim_guard(ctx, false)) return rc;
	return get_list(ctx->heat_sources, out, capacity, count);
}

int fx_heat(fx_ctx* ctx, void* stream) { return run_stage(ctx, stream, heat_phase); }

// ---- tracer particles and the point query (fx_particles.hip) ---------------------------------------------------
// The sort's scratch block for `count` records of this grid (fx_particle_sort_plan.cpp lays it out), its live word zeroed; blocks.  FX_E_INVALID
// for a grid the 32-bit key cannot number, FX_E_NOMEM; nothing of the context changes
static int psort_alloc(fx_ctx* ctx, uint32_t count, fx::PsortPlan* plan, DevBuf* mem)
{
	const uint64_t cells = (uint64_t)ctx->g.X * (uint64_t)ctx->g.Y * (uint64_t)ctx->g.Zg;
	if (fx::psort_plan(cells, count, FX_KNOB_INT("PSORT_KEY_BITS", 0), plan) != 0) return FX_E_INVALID;
	if (const int rc = mem->alloc(ctx, plan->scratch_bytes)) return rc;
	FX_HIP(hipMemset(mem->get<char>() + plan->off_live, 0, 4));
	FX_HIP(hipDeviceSynchronize());
	return FX_OK;
}

// The set lives in a buffer of its own that only this call allocates and frees: the new one is filled beside the one in force, which stays in
// force if anything fails.  Blocks until the caller's records have been read.
int fx_set_particles(fx_ctx* ctx, void* stream, const float* records, uint32_t count, uint32_t flags)
{
	if (const int rc = sim_guard(ctx)) return rc;
	if (flags & ~(uint32_t)FX_PARTICLES_DEVICE) return FX_E_INVALID;
	if (count > FX_MAX_PARTICLES || (count && !records)) return FX_E_INVALID;
	DeviceGuard dg(ctx->device);
	DevBuf fresh, sort_mem;                                                 // while sorting is enabled: the scratch of the new count, on the same terms
	fx::PsortPlan sort_plan = {};
	const bool sorting = ctx->psort_mem != nullptr;
	if (const int rc = sorting ? psort_alloc(ctx, count, &sort_plan, &sort_mem) : FX_OK) return rc;
	DevBuf spawn_mem;                                                       // while spawners are set: their block for the new count, the state carried over
	const fx::SpawnPlan spawn_plan = fx::spawn_plan(count);
	if (ctx->spawn_mem) {
		if (const int rc = spawn_mem.alloc(ctx, spawn_plan.bytes)) return rc;
		FX_HIP(hipDeviceSynchronize());                                     // (no run of the stage is in flight any more: the state is final)
		FX_HIP(hipMemcpy(spawn_mem.get(), ctx->spawn_mem, sizeof(fx::SpawnState), hipMemcpyDeviceToDevice));
		FX_HIP(hipDeviceSynchronize());
	}
	if (count) {
		const size_t bytes = (size_t)count * 16;
		if (const int rc = fresh.alloc(ctx, bytes)) return rc;
		hipStream_t s = pick_stream(ctx, stream);
		FX_HIP(hipMemcpyAsync(fresh.get(), records, bytes, (flags & FX_PARTICLES_DEVICE) ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, s));
		FX_HIP(hipStreamSynchronize(s));
	}
	// the commit: the owners take the old set and the old scratch and free them (hipFree waits for the device: nothing moves the old set any more)
	fresh.swap(&ctx->part);
	ctx->part_count = count;
	if (sorting) {
		sort_mem.swap(&ctx->psort_mem);
		ctx->psort = sort_plan;
	}
	ctx->psort_runs = ctx->psort_sorts = 0;
	if (spawn_mem.get()) {
		spawn_mem.swap(&ctx->spawn_mem);
		ctx->spawn = spawn_plan;
	}
	return fresh.free(ctx);
}

int fx_get_particles(fx_ctx* ctx, float* out, uint32_t capacity, uint32_t* count)
{
	if (const int rc = sim_guard(ctx, false)) return rc;             // (slab ranks may ask: the set is empty there)
	if (!count || (capacity && !out)) return FX_E_INVALID;
	*count = ctx->part_count;
	const uint32_t n = std::min(capacity, ctx->part_count);
	if (!n) return FX_OK;
	DeviceGuard dg(ctx->device);
	FX_HIP(hipDeviceSynchronize());
	FX_HIP(hipMemcpy(out, ctx->part, (size_t)n * 16, hipMemcpyDeviceToHost));
	return FX_OK;
}

int fx_particles_device(fx_ctx* ctx, void** records, uint32_t* count)
{
	if (const int rc = sim_guard(ctx, false)) return rc;
	if (records) *records = ctx->part;
	if (count) *count = ctx->part_count;
	return FX_OK;
}

int fx_set_particle_params(fx_ctx* ctx, const fx_particle_params* p)
{
	if (const int rc = sim_guard(ctx)) return rc;
	const fx_particle_params def = { (uint32_t)sizeof(fx_particle_params), 0u, FX_PARTICLE_MIDPOINT, { 0.0f, 0.0f, 0.0f }, 0.0f };
	if (!p) { ctx->part_prm = def; return FX_OK; }
	if (p->struct_size != sizeof(fx_particle_params) || p->flags != 0) return FX_E_INVALID;
	if (p->scheme != FX_PARTICLE_EULER && p->scheme != FX_PARTICLE_MIDPOINT) return FX_E_INVALID;
	for (int a = 0; a < 3; ++a) if (!std::isfinite(p->drift[a])) return FX_E_INVALID;
	if (!std::isfinite(p->lifetime) || p->lifetime < 0.0f) return FX_E_INVALID;
	ctx->part_prm = *p;
	return FX_OK;
}

int fx_get_particle_params(fx_ctx* ctx, fx_particle_params* out) { return get_setting(ctx, &fx_ctx::part_prm, out); }

int fx_move_particles(fx_ctx* ctx, void* stream) { return run_stage(ctx, stream, particles_phase); }

// ---- the particle sort (fx_particle_sort.hip) -------------------------------------------------------------------
// Enabling allocates the scratch of the set in force (fx_set_particles resizes it from then on), disabling frees it; either way the stage's run
// counter and the sort counter start again.  Blocks.
int fx_set_particle_sort(fx_ctx* ctx, const fx_particle_sort* p)
{
	if (const int rc = sim_guard(ctx)) return rc;
	const fx_particle_sort def = { (uint32_t)sizeof(fx_particle_sort), 0u, 0u, 0u };
	if (!p) p = &def;
	if (p->struct_size != sizeof(fx_particle_sort) || p->flags != 0 || p->enabled > 1u || (p->every && !p->enabled)) return FX_E_INVALID;
	DeviceGuard dg(ctx->device);
	int freed = FX_OK;
	if (p->enabled && !ctx->psort_mem) {
		DevBuf mem;
		fx::PsortPlan plan = {};
		if (const int rc = psort_alloc(ctx, ctx->part_count, &plan, &mem)) return rc;
		ctx->psort_mem = mem.release();
		ctx->psort = plan;
	} else if (!p->enabled && ctx->psort_mem) {
		freed = dev_free(ctx, &ctx->psort_mem);                             // (waits for the device: no sort is in flight any more)
		ctx->psort = fx::PsortPlan{};
	}
	ctx->psort_cfg = *p;
	ctx->psort_runs = ctx->psort_sorts = 0;
	return freed;
}

int fx_get_particle_sort(fx_ctx* ctx, fx_particle_sort* out) { return get_setting(ctx, &fx_ctx::psort_cfg, out); }

int fx_sort_particles(fx_ctx* ctx, void* stream) { return run_stage(ctx, stream, sort_particles_phase); }

int fx_particle_sort_info(fx_ctx* ctx, void* stream, struct fx_particle_sort_info* out)
{
	if (const int rc = sim_guard(ctx, false)) return rc;
	if (!out) return FX_E_INVALID;
	struct fx_particle_sort_info r = { (uint32_t)sizeof(struct fx_particle_sort_info), 0u, ctx->psort_sorts, 0u };
	if (ctx->psort_mem) {
		DeviceGuard dg(ctx->device);
		hipStream_t s = pick_stream(ctx, stream);
		FX_HIP(hipMemcpyAsync(&r.live, static_cast<char*>(ctx->psort_mem) + ctx->psort.off_live, 4, hipMemcpyDeviceToHost, s));
		FX_HIP(hipStreamSynchronize(s));
	}
	*out = r;
	return FX_OK;
}

int fx_particle_order_device(fx_ctx* ctx, void** order_u32, void** live_u32)
{
	if (const int rc = sim_guard(ctx)) return rc;
	if (!order_u32 || !live_u32) return FX_E_INVALID;
	if (!ctx->psort_mem) return FX_E_STATE;
	char* m = static_cast<char*>(ctx->psort_mem);
	*order_u32 = ctx->part_count ? m + ctx->psort.off_order : nullptr;
	*live_u32 = m + ctx->psort.off_live;
	return FX_OK;
}

// ---- the particle trail (fx_particle_trail.hip) -----------------------------------------------------------------
// The accumulator is allocated, zeroed, by the first call that sets a trail and freed by NULL; a later call replaces the rates and keeps it (it is
// all zero between calls).  Blocks.
int fx_set_particle_trail(fx_ctx* ctx, const fx_particle_trail* t)
{
	if (const int rc = sim_guard(ctx)) return rc;
	DeviceGuard dg(ctx->device);
	if (!t) {
		const int freed = dev_free(ctx, &ctx->trail_acc);                    // (waits for the device: no deposit is in flight any more)
		const fx_particle_trail off = { (uint32_t)sizeof(fx_particle_trail), 0u, 0.0f, { 0.0f, 0.0f, 0.0f, 0.0f }, 0.0f };
		ctx->trail = off;
		return freed;
	}
	if (t->struct_size != sizeof(fx_particle_trail) || t->flags != 0) return FX_E_INVALID;
	if (!std::isfinite(t->rate) || t->rate < 0.0f || !std::isfinite(t->heat)) return FX_E_INVALID;
	for (int a = 0; a < 4; ++a) if (!std::isfinite(t->tint[a])) return FX_E_INVALID;
	if (!ctx->trail_acc) {
		const size_t bytes = ctx->g.cells_owned() * sizeof(unsigned long long);
		DevBuf acc;
		if (const int rc = acc.alloc(ctx, bytes)) return rc;
		FX_HIP(hipMemsetAsync(acc.get(), 0, bytes, ctx->stream));
		FX_HIP(hipStreamSynchronize(ctx->stream));
		ctx->trail_acc = acc.release<unsigned long long>();
	}
	ctx->trail = *t;
	return FX_OK;
}

int fx_get_particle_trail(fx_ctx* ctx, fx_particle_trail* out) { return get_setting(ctx, &fx_ctx::trail, out); }

int fx_deposit_particles(fx_ctx* ctx, void* stream)
{
	if (const int rc = sim_guard(ctx)) return rc;
	if (!ctx->trail_acc) return FX_E_STATE;
	return trail_phase(ctx, pick_stream(ctx, stream));
}

// The scatter alone, the accumulator copied out and cleared again; blocks.  (The stage buffer is not used: the copy goes straight to the caller.)
int fx_particle_density(fx_ctx* ctx, void* stream, uint64_t* out, size_t bytes)
{
	if (const int rc = sim_guard(ctx)) return rc;
	if (!out || bytes != ctx->g.cells_owned() * sizeof(uint64_t)) return FX_E_INVALID;
	if (!ctx->trail_acc) return FX_E_STATE;
	hipStream_t s = pick_stream(ctx, stream);
	if (const int rc = trail_splat_phase(ctx, s)) return rc;
	DeviceGuard dg(ctx->device);
	FX_HIP(hipMemcpyAsync(out, ctx->trail_acc, bytes, hipMemcpyDeviceToHost, s));
	FX_HIP(hipMemsetAsync(ctx->trail_acc, 0, bytes, s));
	FX_HIP(hipStreamSynchronize(s));
	return FX_OK;
}

// ---- the particle spawners (fx_particle_spawn.hip) --------------------------------------------------------------
// A list allocates the device block of the set in force (fx_set_particles resizes it from then on) and fills it: the sites, and zeroes for the
// fractions, the serials and the counters; an empty list frees it.  The new block is built beside the one in force.  Blocks.
int fx_set_particle_spawners(fx_ctx* ctx, const fx_particle_spawner* list, uint32_t count)
{
	if (const int rc = sim_guard(ctx)) return rc;
	if (count > FX_MAX_PARTICLE_SPAWNERS || (count && !list)) return FX_E_INVALID;
	if (!list) count = 0;
	for (uint32_t k = 0; k < count; ++k) {
		const fx_particle_spawner& p = list[k];
		if (p.struct_size != sizeof(fx_particle_spawner) || p.flags != 0) return FX_E_INVALID;
		if (p.shape != FX_SPAWN_BOX && p.shape != FX_SPAWN_BALL) return FX_E_INVALID;
		for (int a = 0; a < 3; ++a) if (!std::isfinite(p.center[a]) || !std::isfinite(p.half_extent[a]) || p.half_extent[a] < 0.0f) return FX_E_INVALID;
		if (!std::isfinite(p.rate) || p.rate < 0.0f || !std::isfinite(p.age_spread) || p.age_spread < 0.0f) return FX_E_INVALID;
	}
	DeviceGuard dg(ctx->device);
	DevBuf mem;
	const fx::SpawnPlan plan = fx::spawn_plan(ctx->part_count);
	if (count) {
		fx::SpawnState st = {};
		for (uint32_t k = 0; k < count; ++k) {
			const fx_particle_spawner& p = list[k];
			st.site[k] = fx::SpawnSite{ p.shape, p.seed, { p.center[0], p.center[1], p.center[2] }, { p.half_extent[0], p.half_extent[1], p.half_extent[2] }, p.rate, p.age_spread };
		}
		if (const int rc = mem.alloc(ctx, plan.bytes)) return rc;
		FX_HIP(hipMemcpy(mem.get(), &st, sizeof st, hipMemcpyHostToDevice));
		FX_HIP(hipDeviceSynchronize());
	}
	// the commit: the owner takes the old block and frees it (hipFree waits for the device: no run of the stage is in flight any more)
	mem.swap(&ctx->spawn_mem);
	ctx->spawn = count ? plan : fx::SpawnPlan{};
	ctx->spawners.assign(list, list + count);
	return mem.free(ctx);
}

int fx_get_particle_spawners(fx_ctx* ctx, fx_particle_spawner* out, uint32_t capacity, uint32_t* count)
{
	if (const int rc = sim_guard(ctx, false)) return rc;             // (slab ranks may ask: the list is empty there)
	return get_list(ctx->spawners, out, capacity, count);
}

int fx_spawn_particles(fx_ctx* ctx, void* stream) { return run_stage(ctx, stream, spawn_phase); }

int fx_particle_spawn_info(fx_ctx* ctx, void* stream, struct fx_particle_spawn_info* out)
{
	if (const int rc = sim_guard(ctx, false)) return rc;
	if (!out) return FX_E_INVALID;
	struct fx_particle_spawn_info r = {};
	r.struct_size = (uint32_t)sizeof r;
	if (ctx->spawn_mem) {                                                   // born, dropped, blocked, serial[]: the head of the block, in this order
		static_assert(sizeof r - offsetof(struct fx_particle_spawn_info, born) == offsetof(fx::SpawnState, acc), "the info struct mirrors the state's head");
		DeviceGuard dg(ctx->device);
		hipStream_t s = pick_stream(ctx, stream);
		FX_HIP(hipMemcpyAsync(&r.born, ctx->spawn_mem, offsetof(fx::SpawnState, acc), hipMemcpyDeviceToHost, s));
		FX_HIP(hipStreamSynchronize(s));
	}
	*out = r;
	return FX_OK;
}

// ---- the particle draw (fx_particle_draw.hip) --------------------------------------------------------------------
// what its calls want beside sim_guard: a 3-D grid with a viewport to project it onto
static int draw_guard(const fx_ctx* ctx)
{
	if (const int rc = sim_guard(ctx)) return rc;
	if (ctx->g.Zg <= 1 || !ctx->desc.viewport_w || !ctx->desc.viewport_h) return FX_E_INVALID;
	// (fx_render's limits: tap indices are 32 bits wide and put together by 24-bit multiplies, fx_march.h make_taps)
	if ((uint64_t)ctx->g.Y * ((uint64_t)ctx->g.Zg + 1) >= (1u << 24) || ctx->g.cells_owned() >= ((size_t)1 << 32)) return FX_E_INVALID;
	return FX_OK;
}

// The accumulator is allocated, zeroed, by the first call that sets a draw and freed by NULL; a later call replaces the colours and keeps it (it is
// all zero between calls).  The render target too, where no render has allocated it yet.  Blocks.
int fx_set_particle_draw(fx_ctx* ctx, const fx_particle_draw* d)
{
	if (const int rc = draw_guard(ctx)) return rc;
	DeviceGuard dg(ctx->device);
	if (!d) {
		const int freed = dev_free(ctx, &ctx->draw_acc);                     // (waits for the device: no draw is in flight any more)
		const fx_particle_draw off = { (uint32_t)sizeof(fx_particle_draw), 0u, { 0.0f, 0.0f, 0.0f, 0.0f }, { 0.0f, 0.0f, 0.0f, 0.0f } };
		ctx->draw = off;
		return freed;
	}
	if (d->struct_size != sizeof(fx_particle_draw) || d->flags != 0) return FX_E_INVALID;
	for (int a = 0; a < 4; ++a)
		if (!std::isfinite(d->color[a]) || d->color[a] < 0.0f || !std::isfinite(d->end_color[a]) || d->end_color[a] < 0.0f) return FX_E_INVALID;
	DevBuf acc;
	if (!ctx->draw_acc) {
		const size_t bytes = (size_t)ctx->desc.viewport_w * ctx->desc.viewport_h * 2 * sizeof(unsigned long long);
		if (const int rc = acc.alloc(ctx, bytes)) return rc;
		FX_HIP(hipMemsetAsync(acc.get(), 0, bytes, ctx->stream));
	}
	if (const int rc = ensure_target(ctx, ctx->stream)) return rc;
	FX_HIP(hipStreamSynchronize(ctx->stream));
	if (acc.get()) ctx->draw_acc = acc.release<unsigned long long>();
	ctx->draw = *d;
	return FX_OK;
}

int fx_get_particle_draw(fx_ctx* ctx, fx_particle_draw* out) { return get_setting(ctx, &fx_ctx::draw, out); }

// the splat of the set in force through the colour field fx_render marches; nothing with no set
static int draw_splat(fx_ctx* ctx, hipStream_t s)
{
	if (!ctx->part || !ctx->part_count) return FX_OK;
	FX_HIP(launch_draw_splat(ctx->g, ctx->half, ctx->col[ctx->frame_parity], ctx->fc, ctx->wvp, ctx->depth, (int)ctx->desc.viewport_w,
		(int)ctx->desc.viewport_h, ctx->max_ray_samples, ctx->part_prm.lifetime, ctx->part, ctx->part_count, ctx->draw_acc, s));
	return FX_OK;
}

int fx_draw_particles(fx_ctx* ctx, void* stream, uint8_t frame_index)
{
	if (const int rc = draw_guard(ctx)) return rc;
	if (frame_index >= FX_FRAME_COUNT) return FX_E_INVALID;
	if (!ctx->draw_acc || !ctx->view_valid) return FX_E_STATE;
	DeviceGuard dg(ctx->device);
	hipStream_t s = pick_stream(ctx, stream);
	ScopedMark mk(ctx, s, MK_RESOLVE);
	if (const int rc = draw_splat(ctx, s)) return rc;
	FX_HIP(launch_draw_resolve(ctx->draw, (int)ctx->desc.viewport_w, (int)ctx->desc.viewport_h, ctx->draw_acc, ctx->target, ctx->target_float, s));
	return FX_OK;
}

// The splat alone, the accumulator copied out and cleared again; blocks.  (The stage buffer is not used: the copy goes straight to the caller.)
int fx_particle_splats(fx_ctx* ctx, void* stream, uint64_t* out, size_t bytes)
{
	if (const int rc = draw_guard(ctx)) return rc;
	if (!out || bytes != (size_t)ctx->desc.viewport_w * ctx->desc.viewport_h * 2 * sizeof(uint64_t)) return FX_E_INVALID;
	if (!ctx->draw_acc || !ctx->view_valid) return FX_E_STATE;
	DeviceGuard dg(ctx->device);
	hipStream_t s = pick_stream(ctx, stream);
	{
		ScopedMark mk(ctx, s, MK_RESOLVE);                                  // (the splat's time apart from the resolve's: tools/particle_draw_bench.py)
		if (const int rc = draw_splat(ctx, s)) return rc;
	}
	FX_HIP(hipMemcpyAsync(out, ctx->draw_acc, bytes, hipMemcpyDeviceToHost, s));
	FX_HIP(hipMemsetAsync(ctx->draw_acc, 0, bytes, s));
	FX_HIP(hipStreamSynchronize(s));
	return FX_OK;
}

// ---- the obstacle draw (fx_obstacle_draw.hip) --------------------------------------------------------------------
// what its calls want beside sim_guard: a 3-D grid whose cell index fits the hits word, and a viewport to cast it onto
static int odraw_guard(const fx_ctx* ctx)
{
	if (const int rc = sim_guard(ctx)) return rc;
	if (ctx->g.Zg <= 1 || !ctx->desc.viewport_w || !ctx->desc.viewport_h) return FX_E_INVALID;
	if (ctx->g.cells_owned() >= ((size_t)1 << 32)) return FX_E_INVALID;
	return FX_OK;
}

// The depth-out buffer, filled with 1.0, and the brick volume are allocated by the first call that sets a draw and freed by NULL; a later call
// replaces the albedo and keeps them.  The render target too, where no render has allocated it yet.  Blocks.
int fx_set_obstacle_draw(fx_ctx* ctx, const fx_obstacle_draw* d)
{
	if (const int rc = odraw_guard(ctx)) return rc;
	DeviceGuard dg(ctx->device);
	if (!d) {
		const int freed = dev_free(ctx, &ctx->odraw_depth);                  // (waits for the device: no draw is in flight any more)
		const int freed2 = dev_free(ctx, &ctx->odraw_bricks);
		const fx_obstacle_draw off = { (uint32_t)sizeof(fx_obstacle_draw), 0u, { 0.0f, 0.0f, 0.0f, 0.0f } };
		ctx->odraw = off;
		return freed ? freed : freed2;
	}
	if (d->struct_size != sizeof(fx_obstacle_draw) || d->flags != 0) return FX_E_INVALID;
	for (int a = 0; a < 4; ++a) if (!std::isfinite(d->albedo[a]) || d->albedo[a] < 0.0f) return FX_E_INVALID;
	DevBuf depth, bricks;
	if (!ctx->odraw_depth) {
		const size_t pixels = (size_t)ctx->desc.viewport_w * ctx->desc.viewport_h;
		if (const int rc = depth.alloc(ctx, pixels * sizeof(float))) return rc;
		if (const int rc = bricks.alloc(ctx, obstacle_brick_count(ctx->g) * sizeof(unsigned long long))) return rc;
		FX_HIP(hipMemsetD32Async((hipDeviceptr_t)depth.get(), 0x3F800000, pixels, ctx->stream));   // 1.0f: nothing there
	}
	if (const int rc = ensure_target(ctx, ctx->stream)) return rc;
	FX_HIP(hipStreamSynchronize(ctx->stream));
	if (depth.get()) {
		ctx->odraw_depth = depth.release<float>();
		ctx->odraw_bricks = bricks.release<unsigned long long>();
		ctx->odraw_packed = ctx->obst_gen - 1;                               // nothing is packed yet: the first draw packs
	}
	ctx->odraw = *d;
	return FX_OK;
}

int fx_get_obstacle_draw(fx_ctx* ctx, fx_obstacle_draw* out) { return get_setting(ctx, &fx_ctx::odraw, out); }

int fx_obstacle_depth_device(fx_ctx* ctx, void** depth)
{
	if (const int rc = sim_guard(ctx, false)) return rc;
	if (!depth) return FX_E_INVALID;
	*depth = ctx->odraw_depth;
	return FX_OK;
}

// what fx_draw_obstacles and fx_obstacle_hits share: the arguments' status ...
static int odraw_status(const fx_ctx* ctx, uint8_t frame_index, const float* scene)
{
	if (const int rc = odraw_guard(ctx)) return rc;
	if (frame_index >= FX_FRAME_COUNT) return FX_E_INVALID;
	if (!ctx->odraw_depth || !ctx->view_valid) return FX_E_STATE;
	if (scene && scene == ctx->odraw_depth) return FX_E_INVALID;
	return FX_OK;
}

// ... and the launches: the pack where the mask has changed since the last one, then the cast
static int odraw_cast(fx_ctx* ctx, hipStream_t s, const float* scene, uint8_t* target, float* out_float, float* depth_out, unsigned long long* hits)
{
	const uint8_t* code = ctx->obst_code;
	if (code && ctx->odraw_packed != ctx->obst_gen) {
		FX_HIP(launch_obstacle_pack(ctx->g, code, ctx->odraw_bricks, s));
		ctx->odraw_packed = ctx->obst_gen;
	}
	FX_HIP(launch_obstacle_cast(ctx->g, code, ctx->odraw_bricks, ctx->obst_lo, ctx->obst_hi, ctx->fc, ctx->wvp, ctx->light_kind == FX_LIGHT_POINT,
		ctx->odraw, scene, (int)ctx->desc.viewport_w, (int)ctx->desc.viewport_h, target, out_float, depth_out, hits, s));
	return FX_OK;
}

int fx_draw_obstacles(fx_ctx* ctx, void* stream, uint8_t frame_index, const float* scene_depth_device)
{
	if (const int rc = odraw_status(ctx, frame_index, scene_depth_device)) return rc;
	DeviceGuard dg(ctx->device);
	hipStream_t s = pick_stream(ctx, stream);
	ScopedMark mk(ctx, s, MK_RESOLVE);
	return odraw_cast(ctx, s, scene_depth_device, ctx->target, ctx->target_float, ctx->odraw_depth, nullptr);
}

// The cast alone into the staging buffer, hits words and depths copied out; blocks
int fx_obstacle_hits(fx_ctx* ctx, void* stream, uint8_t frame_index, const float* scene_depth_device, uint64_t* hits_out, float* depth_out, size_t pixels)
{
	if (const int rc = odraw_guard(ctx)) return rc;
	if (pixels != (size_t)ctx->desc.viewport_w * ctx->desc.viewport_h) return FX_E_INVALID;
	if (const int rc = odraw_status(ctx, frame_index, scene_depth_device)) return rc;
	DeviceGuard dg(ctx->device);
	hipStream_t s = pick_stream(ctx, stream);
	FX_HIP(hipDeviceSynchronize());                                          // (the staging buffer is shared with the context's other blocking calls)
	if (const int rc = ensure_stage(ctx, pixels * (sizeof(uint64_t) + sizeof(float)))) return rc;
	unsigned long long* hits = reinterpret_cast<unsigned long long*>(ctx->stage);
	float* depth = reinterpret_cast<float*>(hits + pixels);
	if (const int rc = odraw_cast(ctx, s, scene_depth_device, nullptr, nullptr, depth, hits)) return rc;
	if (hits_out) FX_HIP(hipMemcpyAsync(hits_out, hits, pixels * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
	if (depth_out) FX_HIP(hipMemcpyAsync(depth_out, depth, pixels * sizeof(float), hipMemcpyDeviceToHost, s));
	FX_HIP(hipStreamSynchronize(s));
	return FX_OK;
}

int fx_sample_velocity(fx_ctx* ctx, void* stream, const float* points, uint32_t count, float* out, uint32_t flags)
{
	if (const int rc = sim_guard(ctx)) return rc;
	if (flags & ~(uint32_t)FX_PARTICLES_DEVICE) return FX_E_INVALID;
	if (count > FX_MAX_PARTICLES) return FX_E_INVALID;
	if (count == 0) return FX_OK;
	if (!points || !out) return FX_E_INVALID;
	DeviceGuard dg(ctx->device);
	hipStream_t s = pick_stream(ctx, stream);
	if (flags & FX_PARTICLES_DEVICE) {                                      // enqueue only: the kernel loads a point as one 16-byte vector
		if (((uintptr_t)points & 15u) || ((uintptr_t)out & 3u)) return FX_E_INVALID;
		FX_HIP(launch_sample_velocity(ctx->g, ctx->half, ctx->vel[0], points, out, count, s));
		return FX_OK;
	}
	const size_t in_bytes = (size_t)count * 16, out_bytes = (size_t)count * 12;
	if (const int rc = ensure_stage(ctx, in_bytes + out_bytes)) return rc;
	float* pts = ctx->stage;
	float* res = ctx->stage + (size_t)count * 4;
	FX_HIP(hipMemcpyAsync(pts, points, in_bytes, hipMemcpyHostToDevice, s));
	FX_HIP(launch_sample_velocity(ctx->g, ctx->half, ctx->vel[0], pts, res, count, s));
	FX_HIP(hipMemcpyAsync(out, res, out_bytes, hipMemcpyDeviceToHost, s));
	FX_HIP(hipStreamSynchronize(s));
	return FX_OK;
}

// ---- the advection scheme (fx_maccormack.hip) ---------------------------------------------------------------
int fx_set_advection_scheme(fx_ctx* ctx, uint32_t scheme)
{
	if (const int rc = sim_guard(ctx)) return rc;
	if (scheme != FX_ADVECT_SEMI_LAGRANGIAN && scheme != FX_ADVECT_MACCORMACK) return FX_E_INVALID;
	DeviceGuard dg(ctx->device);
	if (scheme == FX_ADVECT_SEMI_LAGRANGIAN) {                                // the default: every launch is the plain one again, the scratch goes
		const int rv = dev_free(ctx, &ctx->mc_vel), rc = dev_free(ctx, &ctx->mc_col);   // (waits for the device: nothing reads the scratch any more)
		ctx->adv_scheme = scheme;
		return rv ? rv : rc;
	}
	if (!ctx->mc_vel) {                                                       // the first successful switch: seven fp32 values per cell
		const size_t n = ctx->g.cells_owned();
		DevBuf v, c;
		if (const int rc = v.alloc(ctx, 3 * n * sizeof(float))) return rc;
		if (const int rc = c.alloc(ctx, 4 * n * sizeof(float))) return rc;
		ctx->mc_vel = v.release<float>(); ctx->mc_col = c.release<float>();
	}
	ctx->adv_scheme = scheme;
	return FX_OK;
}

int fx_get_advection_scheme(fx_ctx* ctx, uint32_t* scheme)
{
	if (!scheme) return FX_E_INVALID;
	if (const int rc = sim_guard(ctx, false)) return rc;                     // (slab ranks may ask: semi-Lagrangian there)
	*scheme = ctx->adv_scheme;
	return FX_OK;
}

// ---- the pressure solver (fx_multigrid.hip, fx_multigrid_plan.cpp) ---------------------------------------------
static void mg_release(fx_ctx* ctx)
{
	(void)dev_free(ctx, &ctx->mg_mem);                                        // (waits for the device: nothing reads the pyramid any more)
	ctx->mg = MgPlan{};
	for (int l = 0; l < kMgMaxLevels; ++l) { ctx->mg_e[l][0] = ctx->mg_e[l][1] = ctx->mg_b[l] = nullptr; ctx->mg_cur[l] = 0; }
}

int fx_set_pressure_solver(fx_ctx* ctx, const fx_pressure_solver* solver)
{
	if (const int rc = sim_guard(ctx)) return rc;
	if (solver && solver->kind != FX_PRESSURE_JACOBI && solver->kind != FX_PRESSURE_MULTIGRID) return FX_E_INVALID;
	DeviceGuard dg(ctx->device);
	if (!solver || solver->kind == FX_PRESSURE_JACOBI) {                      // the default: every launch is the plain one again, the pyramid goes
		mg_release(ctx);
		ctx->solver = fx_pressure_solver{ FX_PRESSURE_JACOBI, 0u, 0u, 0u, 0u, 0u, 0u, 0.0f };
		return FX_OK;
	}
	const fx_pressure_solver& ps = *solver;
	if ((ps.flags & ~(uint32_t)FX_MG_NO_TAIL) || ps.cycles < 1 || ps.cycles > 64 || ps.pre_sweeps > 64 || ps.post_sweeps > 64 ||
		ps.coarse_sweeps < 1 || ps.coarse_sweeps > 256 || ps.max_levels > FX_MG_MAX_LEVELS || !std::isfinite(ps.omega) || !(ps.omega > 0.0f) || ps.omega > 1.0f)
		return FX_E_INVALID;
	if (ctx->desc.jacobi_mode == FX_JACOBI_FAITHFUL) return FX_E_INVALID;  // the per-cell freeze solve has no coarse levels
	if (ctx->obst_code || ctx->open_faces) return FX_E_STATE;               // their boundary rules have no coarse counterpart yet
	MgPlan plan;
	mg_plan(ctx->g, ps.max_levels, &plan);
	// the pyramid of the new plan is built beside the one in force, which stays in force if the allocation fails
	const size_t align = 64;                                                  // floats: every buffer starts on a 256-byte boundary
	size_t total = 0;
	for (int l = 1; l < plan.levels; ++l) total += 3 * ((plan.lv[l].cells() + align - 1) / align * align);
	DevBuf pyramid;
	if (total) {
		if (const int rc = pyramid.alloc(ctx, total * sizeof(float))) return rc;
		FX_HIP(hipMemset(pyramid.get(), 0, total * sizeof(float)));
	}
	mg_release(ctx);
	float* mem = ctx->mg_mem = pyramid.release<float>();
	ctx->mg = plan;
	for (int l = 1; l < plan.levels; ++l) {
		const size_t n = (plan.lv[l].cells() + align - 1) / align * align;
		ctx->mg_e[l][0] = mem; ctx->mg_e[l][1] = mem + n; ctx->mg_b[l] = mem + 2 * n;
		mem += 3 * n;
	}
	ctx->solver = ps;
	return FX_OK;
}

int fx_get_pressure_solver(fx_ctx* ctx, fx_pressure_solver* out)
{
	if (!out) return FX_E_INVALID;
	if (const int rc = sim_guard(ctx, false)) return rc;                     // (slab ranks may ask: Jacobi there)
	*out = ctx->solver;
	out->max_levels = ctx->solver.kind == FX_PRESSURE_MULTIGRID ? (uint32_t)ctx->mg.levels : 1u;
	return FX_OK;
}

int fx_pressure_solve(fx_ctx* ctx, void* stream)
{
	if (!ctx || ctx->nranks > 1) return FX_E_INVALID;
	if (ctx->desc.flags & FX_FLAG_RENDER_ONLY) return FX_E_STATE;
	std::vector<fx_ctx*> M{ ctx };
	return pressure_solve_all(ctx, M, pick_stream(ctx, stream));
}

int fx_download_pressure_level(fx_ctx* ctx, uint32_t level, int what, void* host, size_t bytes)
{
	if (!host || (what != 0 && what != 1)) return FX_E_INVALID;
	if (const int rc = sim_guard(ctx)) return rc;
	if (level == 0) return fx_download(ctx, what ? FX_FIELD_DIVERGENCE : FX_FIELD_PRESSURE, host, bytes);
	if (ctx->solver.kind != FX_PRESSURE_MULTIGRID || level >= (uint32_t)ctx->mg.levels) return FX_E_INVALID;
	if (bytes != ctx->mg.lv[level].cells() * sizeof(float)) return FX_E_INVALID;
	DeviceGuard dg(ctx->device);
	FX_HIP(hipDeviceSynchronize());
	FX_HIP(hipMemcpy(host, what ? ctx->mg_b[level] : ctx->mg_e[level][ctx->mg_cur[level]], bytes, hipMemcpyDeviceToHost));
	return FX_OK;
}

}  // extern "C"
