// fx_heat.hip -- buoyancy (fx_set_buoyancy): an advected temperature that lifts the smoke, gfx950.  No reference counterpart (the reference's
// only lift is the constant force inside its impulse ball); Fedkiw, Stam, Jensen 2001, eq. 8 is the force.
//
//   k_heat   T advected with the velocity the step's advection traced with, cooled, heated by the sources; f = (-alpha rho + beta (T - Ta)) up
//
// Per cell (x, y, z) of a whole grid, fp32, every operation rounded as written (tests/buoyancy_ref.py restates it in numpy):
//   px = ((float)x + 0.5f) / (float)X (py, pz alike)      a = fmaf(-u0, dt, p)         u0 = velocity[0], the field k_advect traces with
//   t = a * N - 0.5f, i0 = floorf(t), f = t - i0          taps i0, i0 + 1 through the address mode (clamp / mirror)
//   Ts = lerp_z(lerp_y(lerp_x ...)), lerp(a, b, f) = fmaf(f, b - a, a)                 k_advect's colour sample (fx_sim.hip FX_TRI), restated here
//   open walls (faces != 0, fx_open.hip): Ts = fmaf(w, Ts - Ta, Ta), w = (wx * wy) * wz (2-D: no wz) of open_wall_weight(i0, f) -- a ghost at Ta
//   T1 = fmaf(Ts - Ta, fmaxf(fmaf(-dt, cooling, 1), 0), Ta)
//   for each source e in list order: basis as k_emit forms it; if (basis >= e^-4) T1 = fmaf(basis * dt, e.rate, T1)
//   a solid cell (code bit 6, fx_obstacle.hip): T1 = Ta, nothing else
//   t_out = T1;   s = fmaf(lift, T1 - Ta, -(weight * rho)), rho = colour[parity].w as stored;   for each axis a of `axes`:
//   velocity[1][a] = fmaf(up[a] * s, dt, velocity[1][a]), in place (fp16 storage: widened on load, rounded once, RNE, on store)
// A 2-D grid's two z taps are both plane 0: the four taps of the plane are loaded once and the z lerp runs on equal operands.
//
// One launch over the grid, 64 x 4 x 1 tiles (one wave64 = 64 consecutive x of a row).  A near-cell gather bound by memory traffic: the
// eight taps of T come through the L1 / L2 (neighbouring cells share them), nothing is staged in the LDS.  Every field is addressed with
// 32-bit byte offsets from uniform bases (saddr + voffset accesses) while the largest one is under 4 GiB, with 64-bit ones above (WIDE).
// The sources travel as kernel arguments with their clipped boxes (heat_plan, fx_heat_plan.cpp); a tile tests each box with scalar
// compares, and a wave whose lanes are all far below the threshold skips the transcendental, as k_emit does.  The axes the force acts on
// are a launch-uniform argument: a component with up[a] == 0 is neither read nor written.
#include "fx_internal.h"
#include "fx_store.h"

namespace fx {

using namespace sto;

namespace {

const int HT_X = kHeatTileX, HT_Y = kHeatTileY;

// the temperature, fp32 in every context
template <typename O> __device__ __forceinline__ float ldt(const char* b, O cell) { return *reinterpret_cast<const float*>(b + cell * (O)4); }

__device__ __forceinline__ float lerpf(float a, float b, float f) { return fmaf(f, b - a, a); }

// D3D addressing of an integer tap (CLAMP / MIRROR), as the advection kernels address theirs
__device__ __forceinline__ int addr_tap(int i, int n, int mode)
{
	if (mode == FX_ADDRESS_MIRROR) {
		const int period = 2 * n;
		int m = i % period;
		if (m < 0) m += period;
		return m < n ? m : period - 1 - m;
	}
	return min(max(i, 0), n - 1);
}

}  // namespace

template <bool HALF, bool IS3D, bool WIDE>
__global__ __launch_bounds__(256) void k_heat(const Geom g, const HeatArgs a, const void* __restrict__ vel0, void* __restrict__ vel1,
	const void* __restrict__ col, const float* __restrict__ t_in, float* __restrict__ t_out, const uint8_t* __restrict__ code, float dt, int address,
	unsigned faces)
{
	typedef Cell<HALF> Ce;
	typedef typename Off<WIDE>::T O;
	int bid = (int)blockIdx.x;
	const int tile_x = bid % a.tiles_x; bid /= a.tiles_x;
	const int tile_y = bid % a.tiles_y;
	const int bx0 = tile_x * HT_X, by0 = tile_y * HT_Y, z = bid / a.tiles_y;

	// ---- the tile against every source's box: uniform over the workgroup (scalar compares on kernel arguments)
	unsigned reach = 0;
	for (int i = 0; i < a.n; ++i) {
		const HeatBall& e = a.s[i];
		if (bx0 < e.hi[0] && bx0 + HT_X > e.lo[0] && by0 < e.hi[1] && by0 + HT_Y > e.lo[1] && z >= e.lo[2] && z < e.hi[2]) reach |= 1u << i;
	}

	const int x = bx0 + (int)threadIdx.x, y = by0 + (int)threadIdx.y;
	if (x >= g.X || y >= g.Y) return;

	const O X = (O)g.X, plane = (O)g.X * (O)g.Y;
	const O stride = plane * (O)g.Zg;                           // cells between velocity component planes (a whole grid: no halo)
	const O id = (O)z * plane + (O)y * X + (O)x;
	const char* v0 = static_cast<const char*>(vel0);
	char* v1 = static_cast<char*>(vel1);
	const char* ti = reinterpret_cast<const char*>(t_in);
	const float Ta = a.ambient;

	// ---- 1: the back-trace and the taps of k_advect
	const float px = ((float)x + 0.5f) / (float)g.X;
	const float py = ((float)y + 0.5f) / (float)g.Y;
	const float pz = ((float)z + 0.5f) / (float)g.Zg;
	// (2-D grids load u0z and form fz too, on purpose: the z lerp on equal operands below is k_advect's, with its NaN / inf / -0 behaviour -- one
	// load per cell more than the bytes-per-cell floor of the 3-D pass counts)
	const float u0x = Ce::ld1(v0, id), u0y = Ce::ld1(v0, stride + id), u0z = Ce::ld1(v0, (O)2 * stride + id);
	const float ax = fmaf(-u0x, dt, px), ay = fmaf(-u0y, dt, py), az = fmaf(-u0z, dt, pz);
	const float tx = ax * (float)g.X - 0.5f, ty = ay * (float)g.Y - 0.5f, tz = az * (float)g.Zg - 0.5f;
	const float flx = floorf(tx), fly = floorf(ty), flz = floorf(tz);
	const float fx = tx - flx, fy = ty - fly, fz = tz - flz;
	const int ix = (int)flx, iy = (int)fly, iz = (int)flz;
	const O x0 = (O)addr_tap(ix, g.X, address), x1 = (O)addr_tap(ix + 1, g.X, address);
	const O r0 = (O)addr_tap(iy, g.Y, address) * X, r1 = (O)addr_tap(iy + 1, g.Y, address) * X;
	float Ts;
	if (IS3D) {
		const O p0 = (O)addr_tap(iz, g.Zg, address) * plane, p1 = (O)addr_tap(iz + 1, g.Zg, address) * plane;
		const float t000 = ldt(ti, p0 + r0 + x0), t100 = ldt(ti, p0 + r0 + x1), t010 = ldt(ti, p0 + r1 + x0), t110 = ldt(ti, p0 + r1 + x1);
		const float t001 = ldt(ti, p1 + r0 + x0), t101 = ldt(ti, p1 + r0 + x1), t011 = ldt(ti, p1 + r1 + x0), t111 = ldt(ti, p1 + r1 + x1);
		Ts = lerpf(lerpf(lerpf(t000, t100, fx), lerpf(t010, t110, fx), fy), lerpf(lerpf(t001, t101, fx), lerpf(t011, t111, fx), fy), fz);
	} else {
		const float t00 = ldt(ti, r0 + x0), t10 = ldt(ti, r0 + x1), t01 = ldt(ti, r1 + x0), t11 = ldt(ti, r1 + x1);
		const float c = lerpf(lerpf(t00, t10, fx), lerpf(t01, t11, fx), fy);
		Ts = lerpf(c, c, fz);
	}

	// ---- 1b: open walls (fx_open.hip; launch-uniform, 0 = none): the cells beyond an open face are at the ambient value
	if (faces) {
		float w = open_wall_weight(flx, fx, g.X, faces & 1u, faces & 2u) * open_wall_weight(fly, fy, g.Y, faces & 4u, faces & 8u);
		if (IS3D) w = w * open_wall_weight(flz, fz, g.Zg, faces & 16u, faces & 32u);
		Ts = fmaf(w, Ts - Ta, Ta);
	}

	// ---- 2: cooling towards the ambient value
	float T1 = fmaf(Ts - Ta, fmaxf(fmaf(-dt, a.cooling, 1.0f), 0.0f), Ta);

	// ---- 3: the heat sources whose box meets the tile, in list order (the basis of k_emit)
	for (int i = 0; i < a.n; ++i) {
		if (!((reach >> i) & 1u)) continue;
		const HeatBall& e = a.s[i];
		const bool in = x >= e.lo[0] && x < e.hi[0] && y >= e.lo[1] && y < e.hi[1] && z >= e.lo[2] && z < e.hi[2];
		const float dx = px - e.c[0], dy = py - e.c[1], dz = IS3D ? pz - e.c[2] : 0.0f;
		const float d2 = fmaf(dz, dz, fmaf(dy, dy, dx * dx));
		const float ex = ((d2 * -4.0f) / e.rr) * 1.44269502f;
		if (__builtin_amdgcn_ballot_w64(in && ex > -6.5f) == 0) continue;        // exp2(ex) >= e^-4 needs ex >= -5.77
		const float basis = exp2f(ex);
		if (in && basis >= 0.0183156393f) T1 = fmaf(basis * dt, e.rate, T1);
	}

	// ---- 4, 5: a solid cell holds the ambient value and keeps its velocity bits
	const bool solid = code != nullptr && (code[id] & OB_SELF) != 0;
	if (solid) T1 = Ta;
	*reinterpret_cast<float*>(reinterpret_cast<char*>(t_out) + id * (O)4) = T1;
	if (solid) return;

	// ---- 6: the force, on the axes with up != 0
	const float rho = Ce::alpha(static_cast<const char*>(col), id);
	const float s = fmaf(a.lift, T1 - Ta, -(a.weight * rho));
	if (a.axes & 1) Ce::st1(v1, id, fmaf(a.up[0] * s, dt, Ce::ld1(v1, id)));
	if (a.axes & 2) Ce::st1(v1, stride + id, fmaf(a.up[1] * s, dt, Ce::ld1(v1, stride + id)));
	if (IS3D && (a.axes & 4)) Ce::st1(v1, (O)2 * stride + id, fmaf(a.up[2] * s, dt, Ce::ld1(v1, (O)2 * stride + id)));
}

template <bool HALF, bool IS3D>
static hipError_t launch_heat_t(bool wide, dim3 grid, dim3 block, hipStream_t s, const Geom& g, const HeatArgs& a, const void* vel0, void* vel1,
	const void* col, const float* t_in, float* t_out, const uint8_t* code, float dt, int address, unsigned faces)
{
	if (wide) hipLaunchKernelGGL((k_heat<HALF, IS3D, true>), grid, block, 0, s, g, a, vel0, vel1, col, t_in, t_out, code, dt, address, faces);
	else hipLaunchKernelGGL((k_heat<HALF, IS3D, false>), grid, block, 0, s, g, a, vel0, vel1, col, t_in, t_out, code, dt, address, faces);
	return hipGetLastError();
}

hipError_t launch_heat(const Geom& g, int half_store, const fx_buoyancy& b, const fx_heat_source* list, int count, const void* vel0, void* vel1,
	const void* col, const float* t_in, float* t_out, const uint8_t* code, float dt, int address, hipStream_t s, unsigned faces)
{
	if (!whole_grid(g)) return hipErrorNotSupported;                            // (fx_set_buoyancy refuses slab ranks)
	if (!vel0 || !vel1 || !col || !t_in || !t_out || t_in == t_out) return hipErrorInvalidValue;
	if (!open_faces_ok(g, faces)) return hipErrorInvalidValue;
	HeatArgs a;
	const int wgs = heat_plan(g, b, list, count, &a);
	if (wgs <= 0) return hipErrorInvalidValue;
	const dim3 grid((unsigned)wgs, 1, 1), block(HT_X, HT_Y, 1);
	const bool wide = colour_wants_wide_offsets(g);
	const bool is3d = g.Zg > 1;
	if (half_store) return is3d ? launch_heat_t<true, true>(wide, grid, block, s, g, a, vel0, vel1, col, t_in, t_out, code, dt, address, faces)
	                            : launch_heat_t<true, false>(wide, grid, block, s, g, a, vel0, vel1, col, t_in, t_out, code, dt, address, faces);
	return is3d ? launch_heat_t<false, true>(wide, grid, block, s, g, a, vel0, vel1, col, t_in, t_out, code, dt, address, faces)
	            : launch_heat_t<false, false>(wide, grid, block, s, g, a, vel0, vel1, col, t_in, t_out, code, dt, address, faces);
}

}  // namespace fx
