// fx_emit.hip -- the settable smoke emitters (fx_set_emitters), gfx950.
//
//   k_emit   the impulse of CSAdvect.hlsl:59-68 / Impulse.hlsli with its constants made arguments, as a pass of its own behind the advection
//
// Per cell (x, y, z) of a whole grid, for each emitter e in list order (the operation order of k_advect's impulse block, fx_sim.hip):
//   px = ((float)x + 0.5f) / (float)X  (py, pz alike)      dx = px - e.cx, dy = py - e.cy, dz = 3-D ? pz - e.cz : 0
//   d2 = fmaf(dz, dz, fmaf(dy, dy, dx * dx))               basis = exp2f(((d2 * -4.0f) / (e.r * e.r)) * 1.44269502f)
//   if (basis >= e^-4) {
//       F = 3-D: (fmaf(basis, e.fx, dz * -e.swirl), fmaf(basis, e.fy, 0), fmaf(basis, e.fz, dx * e.swirl))      2-D: (basis * e.fx, basis * e.fy, 0)
//       u[a] = fmaf(F[a], dt, u[a])        c[i] = saturate(fmaf(basis * dt, e.rate[i], c[i]))
//   }
// in place on velocity[1] and colour[parity].  An emitter with the built-in impulse's constants forms the same basis bits as the advection
// kernels (tests/test_gpu_emitters.py holds the pass against k_advect, k_advect_fast and k_advect_lds bit for bit, from zero fields);
// unlike the built-in it adds BEHIND the step's attenuation.
// fp16 storage widens on load and rounds each stored value once (RNE) behind the last emitter; a cell in no emitter's support is not stored.
//
// One launch, the emitters travel as kernel arguments (no device memory, no copy, no synchronisation: a new list every frame is free).
// The host (emit_plan, fx_emit_plan.cpp: plain host code, tests/test_emitter_ref.py links it into a small program) clips each
// emitter's bounding box to the grid, drops the emitters whose box is empty and lays 64 x 4 x 1 tiles (one wave64 = 64 consecutive x of a row), aligned to the grid's own
// 64 x 4 raster, over the union box: the work follows the covered volume, not the grid.  A workgroup whose tile meets no box exits on a
// uniform test; a cell is owned by exactly one thread, which walks the emitters whose box holds it in list order, so overlapping emitters
// cannot race.  exp2(ex) >= e^-4 needs ex >= -5.77: a wave whose lanes are all below -6.5 skips the transcendental (the test advect_finish
// uses, fx_advect_lds.hip); the decision itself still uses the computed basis.
// When the step's advection wrote the render's alpha side volume (fx_render_accel.hip), the pass stores the stored alpha of every cell it
// changes there too, so the volume stays true to the colour field.
#include "fx_internal.h"
#include "fx_store.h"

namespace fx {

using namespace sto;

namespace {

const int ET_X = kEmitTileX, ET_Y = kEmitTileY;  // tile: one wave a row

__device__ __forceinline__ float saturatef(float x) { return fminf(fmaxf(x, 0.0f), 1.0f); }

}  // namespace

template <bool HALF, bool WIDE>
__global__ __launch_bounds__(256) void k_emit(const Geom g, const EmitArgs a, void* __restrict__ vel, void* __restrict__ col,
	float* __restrict__ alpha, float dt, int is3d)
{
	typedef Cell<HALF> Ce;
	typedef typename Off<WIDE>::T O;
	int bid = (int)blockIdx.x;
	const int tile_x = bid % a.tiles_x; bid /= a.tiles_x;
	const int tile_y = bid % a.tiles_y;
	const int bx0 = a.x0 + tile_x * ET_X, by0 = a.y0 + tile_y * ET_Y, z = a.z0 + bid / a.tiles_y;

	// ---- the tile against every box: uniform over the workgroup (scalar compares on kernel arguments)
	bool hit = false;
	for (int i = 0; i < a.n; ++i) {
		const EmitBall& e = a.e[i];
		hit = hit || (bx0 < e.hi[0] && bx0 + ET_X > e.lo[0] && by0 < e.hi[1] && by0 + ET_Y > e.lo[1] && z >= e.lo[2] && z < e.hi[2]);
	}
	if (!hit) return;

	// ---- the cell against every box (the boxes are clipped to the grid: a cell inside one is a cell of the grid)
	const int x = bx0 + (int)threadIdx.x, y = by0 + (int)threadIdx.y;
	bool mine = false;
	for (int i = 0; i < a.n; ++i) {
		const EmitBall& e = a.e[i];
		mine = mine || (x >= e.lo[0] && x < e.hi[0] && y >= e.lo[1] && y < e.hi[1] && z >= e.lo[2] && z < e.hi[2]);
	}
	if (!mine) return;

	const O stride = (O)g.cells_local();                        // cells between velocity component planes
	const O id = (O)g.lz(z) * (O)g.plane() + (O)y * (O)g.X + (O)x;
	char* v0 = static_cast<char*>(vel);
	char* co = static_cast<char*>(col);
	float u[3] = { Ce::ld1(v0, id), Ce::ld1(v0, stride + id), Ce::ld1(v0, (O)2 * stride + id) };
	const float4 c4 = Ce::ld4(co, id);
	float c[4] = { c4.x, c4.y, c4.z, c4.w };

	const float px = ((float)x + 0.5f) / (float)g.X;            // Simulation.hlsli:10, as k_advect
	const float py = ((float)y + 0.5f) / (float)g.Y;
	const float pz = ((float)z + 0.5f) / (float)g.Zg;
	bool changed = false;
	for (int i = 0; i < a.n; ++i) {
		const EmitBall& e = a.e[i];
		const bool in = x >= e.lo[0] && x < e.hi[0] && y >= e.lo[1] && y < e.hi[1] && z >= e.lo[2] && z < e.hi[2];
		const float dx = px - e.c[0], dy = py - e.c[1], dz = is3d ? pz - e.c[2] : 0.0f;
		const float d2 = fmaf(dz, dz, fmaf(dy, dy, dx * dx));
		const float ex = ((d2 * -4.0f) / e.rr) * 1.44269502f;
		if (__builtin_amdgcn_ballot_w64(in && ex > -6.5f) == 0) continue;
		const float basis = exp2f(ex);
		if (in && basis >= 0.0183156393f) {
			float Fx, Fy, Fz;
			if (is3d) {
				Fx = fmaf(basis, e.force[0], dz * -e.swirl);
				Fy = fmaf(basis, e.force[1], 0.0f);
				Fz = fmaf(basis, e.force[2], dx * e.swirl);
			} else {
				Fx = basis * e.force[0]; Fy = basis * e.force[1]; Fz = 0.0f;
			}
			u[0] = fmaf(Fx, dt, u[0]); u[1] = fmaf(Fy, dt, u[1]); u[2] = fmaf(Fz, dt, u[2]);
			const float bdt = basis * dt;
			c[0] = saturatef(fmaf(bdt, e.rate[0], c[0]));
			c[1] = saturatef(fmaf(bdt, e.rate[1], c[1]));
			c[2] = saturatef(fmaf(bdt, e.rate[2], c[2]));
			c[3] = saturatef(fmaf(bdt, e.rate[3], c[3]));
			changed = true;
		}
	}
	if (!changed) return;                                       // outside every support: the cell keeps its bits
	Ce::st1(v0, id, u[0]);
	Ce::st1(v0, stride + id, u[1]);
	Ce::st1(v0, (O)2 * stride + id, u[2]);
	const float stored_alpha = Ce::st4(co, id, c);
	if (alpha) *reinterpret_cast<float*>(reinterpret_cast<char*>(alpha) + id * (O)4) = stored_alpha;
}

hipError_t launch_emit(const Geom& g, int half_store, void* vel, void* col, float* alpha, const fx_emitter* list, int count, float dt, hipStream_t s)
{
	if (!whole_grid(g)) return hipErrorNotSupported;                            // (fx_set_emitters refuses slab ranks)
	EmitArgs a;
	const int wgs = emit_plan(g, list, count, &a);
	if (wgs < 0) return hipErrorInvalidValue;
	if (wgs == 0) return hipSuccess;                                            // every box clipped away: nothing to launch
	const dim3 grid((unsigned)wgs, 1, 1), block(ET_X, ET_Y, 1);
	const int is3d = g.Zg > 1 ? 1 : 0;
	const bool wide = colour_wants_wide_offsets(g);
	if (half_store) {
		if (wide) hipLaunchKernelGGL((k_emit<true, true>), grid, block, 0, s, g, a, vel, col, alpha, dt, is3d);
		else hipLaunchKernelGGL((k_emit<true, false>), grid, block, 0, s, g, a, vel, col, alpha, dt, is3d);
	} else {
		if (wide) hipLaunchKernelGGL((k_emit<false, true>), grid, block, 0, s, g, a, vel, col, alpha, dt, is3d);
		else hipLaunchKernelGGL((k_emit<false, false>), grid, block, 0, s, g, a, vel, col, alpha, dt, is3d);
	}
	return hipGetLastError();
}

}  // namespace fx
