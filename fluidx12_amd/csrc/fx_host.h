// fx_host.h -- what the four host-side units of the C ABI share (fx_context.cpp: contexts, fields, timing, options;
// fx_schedule.cpp: the simulation step over a group of slab contexts; fx_api.cpp: frame constants, rendering, light probe, slab
// groups; fx_stage_api.cpp: the optional stages' setters, getters and stage calls): status macro, device guard, the owners of
// device memory, timing marks, plane ranges.  Product code: nothing from oracle/.
#pragma once
#include "fx_context.h"
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>

// A failed HIP call also leaves its code in the runtime's sticky "last error": the launch helpers end in hipGetLastError(), and a
// stale out-of-memory from one context's failed fx_create would otherwise surface as the status of the next, unrelated launch
// (found by the descriptor fuzz).  Reading the last error here clears it.
#define FX_HIP(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) { (void)hipGetLastError(); \
	ctx->last_error = std::string(#call) + ": " + hipGetErrorString(e_); return e_ == hipErrorOutOfMemory ? FX_E_NOMEM : FX_E_DEVICE; } } while (0)

namespace fxh {

const uint32_t kNumMips = 5;            // Fluid.cpp:229
const uint32_t kDefaultAdvectHalo = 6;  // measured z back-trace reach at 256^3: <= 3.5 cells over 400 steps (tools/reach_probe.py)
const uint32_t kFreezeStatRing = 1024;   // per-step statistics words of the sparse faithful solver kept on the device
const uint32_t kDefaultJacobiHalo = 8;   // sweeps per pressure exchange: 5 messages per 40 sweeps, +11% halo sweeps at 64 planes/rank

inline hipStream_t pick_stream(fx_ctx* ctx, void* s) { return s ? (hipStream_t)s : ctx->stream; }
inline size_t elem_size(const fx_ctx* c) { return c->half ? 2 : 4; }
// the reference's light (Fluid.cpp:169-173): what a context starts with and fx_set_light(ctx, NULL) returns to
inline void default_light(fx_ctx* c)
{
	const float pi = 3.141592654f;
	const float lp[3] = { 75.0f, 75.0f, -75.0f };
	const float lc[4] = { 1.0f, 0.7f, 0.3f, pi * 3.0f }, am[4] = { 1.0f, 1.0f, 1.0f, pi * 1.5f };
	for (int a = 0; a < 3; ++a) c->fc.light_pt[a] = lp[a];
	for (int a = 0; a < 4; ++a) { c->fc.light_color[a] = lc[a]; c->fc.ambient[a] = am[a]; }
	c->light_kind = FX_LIGHT_DIRECTIONAL;
}

struct DeviceGuard {
	int prev = -1;
	bool ok = true, changed = false;
	explicit DeviceGuard(int dev) { if (hipGetDevice(&prev) != hipSuccess) prev = -1; if (prev != dev) { ok = hipSetDevice(dev) == hipSuccess; changed = true; } }
	~DeviceGuard() { if (changed && prev >= 0) (void)hipSetDevice(prev); }     // (nothing to restore on the usual one-device path: a guard per launch costs one hipGetDevice)
};

// ---- device memory ----------------------------------------------------------------------------
// Every allocation and free of the host units outside free_all goes through these.  One failure mapping, FX_HIP's: last_error is
// written, HIP's sticky error cleared, hipErrorOutOfMemory gives FX_E_NOMEM and anything else FX_E_DEVICE; the pointer is null behind
// a failure.  The try_ forms are for what a context can do without (fx_create's best-effort scratch): they report to nobody.
namespace {   // (each unit gets its own copies, and the library exports no symbol for them)
template <class T> hipError_t try_dev_alloc(T** p, size_t bytes)
{
	void* q = nullptr;
	const hipError_t e = hipMalloc(&q, bytes);
	if (e != hipSuccess) { (void)hipGetLastError(); q = nullptr; }
	*p = static_cast<T*>(q);
	return e;
}
template <class T> hipError_t try_host_alloc(T** p, size_t bytes, unsigned flags)       // pinned host memory (free_all: hipHostFree)
{
	void* q = nullptr;
	const hipError_t e = hipHostMalloc(&q, bytes, flags);
	if (e != hipSuccess) { (void)hipGetLastError(); q = nullptr; }
	*p = static_cast<T*>(q);
	return e;
}
template <class T> int dev_alloc(fx_ctx* ctx, T** p, size_t bytes) { FX_HIP(try_dev_alloc(p, bytes)); return FX_OK; }
template <class T> int dev_keep(fx_ctx* ctx, T** p, size_t bytes) { return *p ? FX_OK : dev_alloc(ctx, p, bytes); }   // allocated by the first call that needs it, and kept
// frees if set, nulls always, and reports a failed hipFree afterwards (hipFree waits for the device: nothing uses the memory any more)
template <class T> int dev_free(fx_ctx* ctx, T** p)
{
	T* q = *p;
	*p = nullptr;
	if (q) FX_HIP(hipFree((void*)q));
	return FX_OK;
}
// dev_alloc with the buffer zeroed on `s` (default: the context's stream); null behind a failed fill too
template <class T> int dev_alloc_zeroed(fx_ctx* ctx, T** p, size_t bytes, hipStream_t s = nullptr)
{
	if (const int rc = dev_alloc(ctx, p, bytes)) return rc;
	const hipError_t e = hipMemsetAsync(*p, 0, bytes, s ? s : ctx->stream);
	if (e != hipSuccess) (void)dev_free(ctx, p);
	FX_HIP(e);
	return FX_OK;
}
// a kept buffer that grows: a request beyond the *have bytes of *p frees it and allocates anew (the contents go); *have stays true on every path
template <class T> int dev_grow(fx_ctx* ctx, T** p, size_t* have, size_t bytes)
{
	if (*have >= bytes) return FX_OK;
	*have = 0;
	if (const int rc = dev_free(ctx, p)) return rc;
	if (const int rc = dev_alloc(ctx, p, bytes)) return rc;
	*have = bytes;
	return FX_OK;
}

// One device allocation owned by a scope: a setter builds the new buffers beside the ones in force in owners on its stack, every early
// return frees them, and its last lines -- which cannot fail -- swap them into the context, so that the owner then frees the old ones.
class DevBuf {
	void* p_ = nullptr;
public:
	DevBuf() = default;
	DevBuf(DevBuf&& o) noexcept : p_(o.p_) { o.p_ = nullptr; }
	DevBuf& operator=(DevBuf&& o) noexcept { std::swap(p_, o.p_); return *this; }
	~DevBuf() { if (p_ && hipFree(p_) != hipSuccess) (void)hipGetLastError(); }
	int alloc(fx_ctx* ctx, size_t bytes) { if (const int rc = dev_free(ctx, &p_)) return rc; return dev_alloc(ctx, &p_, bytes); }
	template <class T = void> T* get() const { return static_cast<T*>(p_); }
	template <class T = void> T* release() { void* q = p_; p_ = nullptr; return static_cast<T*>(q); }
	template <class T> void swap(T** slot) { void* q = (void*)*slot; *slot = static_cast<T*>(p_); p_ = q; }   // the commit: *slot's old buffer is this owner's now
	int free(fx_ctx* ctx) { return dev_free(ctx, &p_); }                  // now, reporting a failure, where the destructor cannot
};
}  // namespace

// ---- timing ---------------------------------------------------------------------------------
enum MarkKind { MK_ADVECT, MK_DIV, MK_JACOBI, MK_PROJECT, MK_LIGHT, MK_VIEW, MK_EXCH, MK_RESOLVE, MK_JACOBI_TAIL, MK_CHAIN };

size_t ev_record(fx_ctx* c, hipStream_t s);          // fx_context.cpp

struct ScopedMark {
	fx_ctx* c; hipStream_t s; int kind; size_t e0; uint64_t launches, sweeps;
	ScopedMark(fx_ctx* c_, hipStream_t s_, int kind_) : c(c_), s(s_), kind(kind_), e0((size_t)-1), launches(0), sweeps(0)
	{
		if (c->timing_on) e0 = ev_record(c, s);
	}
	// close the mark here and continue as `new_kind` from the same event (one event more, no gap)
	void split(int new_kind)
	{
		if (c->timing_on && e0 != (size_t)-1) {
			const size_t e1 = ev_record(c, s);
			if (e1 != (size_t)-1) { c->marks.push_back(fx_ctx::Mark{ kind, e0, e1, launches, sweeps }); e0 = e1; }
		}
		kind = new_kind; launches = 0; sweeps = 0;
	}
	~ScopedMark()
	{
		if (c->timing_on && e0 != (size_t)-1) {
			const size_t e1 = ev_record(c, s);
			if (e1 != (size_t)-1) c->marks.push_back(fx_ctx::Mark{ kind, e0, e1, launches, sweeps });
		}
	}
};

int drain_timing(fx_ctx* c);
int ensure_stage(fx_ctx* ctx, size_t bytes);
int ensure_target(fx_ctx* ctx, hipStream_t s);   // fx_api.cpp: the render target and its float twin, zeroed on `s`, where no call has allocated them yet
void free_all(fx_ctx* c);
void destroy_lanes(fx_comm_group* g);
void group_release(fx_comm_group* g);

// planes of the local array a stage may compute / read, as global z ranges
struct Range { int lo, hi; };   // [lo, hi)
inline Range owned(const fx_ctx* c) { return Range{ c->g.z0, c->g.z0 + c->g.nz }; }
inline Range grown(const fx_ctx* c, int by)
{
	return Range{ std::max(c->g.z0 - by, 0), std::min(c->g.z0 + c->g.nz + by, c->g.Zg) };
}

inline bool multi_rank(const fx_ctx* c) { return c->group && c->nranks > 1; }
inline bool has_lower(const fx_ctx* c) { return c->nranks > 1 && c->rank > 0; }
inline bool has_upper(const fx_ctx* c) { return c->nranks > 1 && c->rank + 1 < c->nranks; }
inline bool is_driver(const fx_ctx* c) { return !c->group || !c->group->transport->is_local() || c->group->members[0] == c; }
inline bool group_broken(const fx_ctx* c) { return c->group && c->group->transport->is_local() && c->group->broken; }

// ---- fx_schedule.cpp: the step, phase by phase ------------------------------------------------------
int for_members(fx_ctx* ctx, std::vector<fx_ctx*>& out);
int overlap_level(const fx_ctx* lead);
int options_digest(const fx_ctx* c);
int advect_range(fx_ctx* ctx, hipStream_t s, Range r, bool own_only);   // planes [r.lo, r.hi); own_only: back-traces must stay inside the owned planes
int advect_all(fx_ctx* ctx, std::vector<fx_ctx*>& M, hipStream_t s);
int open_inflow_phase(fx_ctx* ctx, hipStream_t s);   // colour[parity] scaled by the inside share of its back-trace; nothing with all walls closed or dt <= 0
int emit_phase(fx_ctx* ctx, hipStream_t s);          // the settable emitters on velocity[1] / colour[parity]; nothing with an empty list or dt <= 0
int heat_phase(fx_ctx* ctx, hipStream_t s);          // buoyancy: the temperature advected / cooled / heated, the force on velocity[1]; nothing while it is off or with dt <= 0
int enforce_phase(fx_ctx* ctx, hipStream_t s);       // the solid cells of velocity[1] / colour[parity] become +0; nothing without solid cells or with dt <= 0
int confine_phase(fx_ctx* ctx, hipStream_t s);       // vorticity confinement of velocity[1]; nothing with epsilon = 0 or dt <= 0
int divergence_phase(fx_ctx* ctx, hipStream_t s);
int jacobi_all(fx_ctx* lead, std::vector<fx_ctx*>& M, hipStream_t s, uint32_t iters);
int pressure_solve_all(fx_ctx* lead, std::vector<fx_ctx*>& M, hipStream_t s);   // the solver stage of the step: jacobi_all(jacobi_iters), or the multigrid V-cycles (fx_set_pressure_solver)
int project_phase(fx_ctx* ctx, hipStream_t s);
int particles_phase(fx_ctx* ctx, hipStream_t s);     // the tracer particles one step through velocity[0], behind the projection; nothing with no set or dt <= 0
int sort_particles_phase(fx_ctx* ctx, hipStream_t s);   // the particle sort alone (fx_sort_particles); nothing with no set; counts into psort_sorts
int trail_phase(fx_ctx* ctx, hipStream_t s);         // the particle trail (fx_deposit_particles): scatter and apply; nothing with no trail, no set or dt <= 0
int trail_splat_phase(fx_ctx* ctx, hipStream_t s);   // the scatter alone (fx_particle_density); FX_E_STATE with no trail, nothing with no set
int spawn_phase(fx_ctx* ctx, hipStream_t s);         // the particle spawners alone (fx_spawn_particles); FX_E_STATE with no spawners, nothing with no set or dt <= 0
int simulate_impl(fx_ctx* ctx, hipStream_t s);

}  // namespace fxh
