// fx_obstacle_moving.hip -- the obstacle kernels for solids that move (fx_set_obstacle_bodies), gfx950.  No reference counterpart; the
// other half of the Harris / Crane et al. scheme (GPU Gems 3, ch. 30) that fx_obstacle.hip cites: the velocity of the solid enters the
// divergence and the boundary rule of the projection.
//
//   k_obstacle_enforce_mov  k_obstacle_enforce with a solid cell's VELOCITY1 = w(c) instead of +0
//   k_divergence_obs_mov    k_divergence_obs with  v_a(n) -> S(n) ? w_a(n) : v_a(n)
//   k_project_bnd_mov       k_project_bnd (CODE = 1) with u[a] = the wall's w_a beside a solid along a (both sides solid: their mean) and
//                           w(c) in a solid cell
//
// w(n) of a solid cell n: B(n) = the first body of the list whose closed box holds the cell centre pos(n) = ((float)i + 0.5f) / (float)N per
// axis (a 2-D grid ignores z); r = pos(n) - pivot;
//   w_x = fmaf(angular_y, r_z, fmaf(-angular_z, r_y, linear_x))
//   w_y = fmaf(angular_z, r_x, fmaf(-angular_x, r_z, linear_y))
//   w_z = fmaf(angular_x, r_y, fmaf(-angular_y, r_x, linear_z))
// 2-D grids: w_x = fmaf(-angular_z, r_y, linear_x), w_y = fmaf(angular_z, r_x, linear_y), w_z = +0.  No box holds the cell: w = +0.
// The relaxation is not here: the pressure ghost of a moving wall is still the cell's own pressure (k_jacobi_bnd / _v4 serve).
//
// The kernels are launched only while a mask is in force AND the list is not empty (fx_schedule.cpp); otherwise fx_obstacle.hip's run.  The
// bodies travel as a kernel argument (no device memory, no copy: a new list every frame is free).  Nothing reads the mask: the code byte of a
// cell (fx_obstacle.hip) says which clamped neighbours are solid, and a lane evaluates w only for those -- the body lookup is one loop over
// the list (uniform loads of the argument, a compare per axis and position) behind a wave-uniform test of the byte's bits, so a wave none of
// whose cells has a solid neighbour executes k_divergence_obs' / k_project_bnd's arithmetic and nothing else.  With w = +0 everywhere (no box
// holds a solid) every kernel is, operation for operation, its resting counterpart.  tests/test_gpu_moving_obstacles.py holds them bit for
// bit against the numpy model tests/moving_obstacle_ref.py.
// fp32 arithmetic in the resting kernels' association order; fp16 storage widens on load and rounds once (RNE) on store -- w too, where it
// is stored; where it is read by the divergence and the projection it is the fp32 value.
// Whole grids only (fx_set_obstacle_bodies refuses slab ranks): local plane = global plane.
#include "fx_internal.h"
#include "fx_store.h"

namespace fx {

using namespace sto;

namespace {

// the code byte's bits, the tile order and the open-face test of fx_obstacle.hip, restated: that file's kernels stay as they are
enum { OB_XM = 1, OB_XP = 2, OB_YM = 4, OB_YP = 8, OB_ZM = 16, OB_ZP = 32, OB_SELF = 64 };

struct Tile3 { int x, y, z; };
__device__ __forceinline__ Tile3 tile_of(int gx, int gy, int gz, int remap)
{
	int t = (int)blockIdx.x;
	if (remap == 1) {
		const int n = gx * gy * gz, q = n >> 3, r = n & 7;
		const int xcd = t & 7, j = t >> 3;
		t = xcd * q + min(xcd, r) + j;
	}
	Tile3 o;
	o.x = t % gx;
	const int u = t / gx;
	o.y = u % gy;
	o.z = u / gy;
	return o;
}

__device__ __forceinline__ unsigned beyond_of(const Geom& g, unsigned faces, int x, int y, int z)
{
	unsigned on = 0;
	if (x == 0) on |= OB_XM;
	if (x == g.X - 1) on |= OB_XP;
	if (y == 0) on |= OB_YM;
	if (y == g.Y - 1) on |= OB_YP;
	if (z == 0) on |= OB_ZM;
	if (z == g.Zg - 1) on |= OB_ZP;
	return faces & on;
}

// cell index -> the advection's cell centre
__device__ __forceinline__ float centre(int i, int n) { return ((float)i + 0.5f) / (float)n; }

// What the walls around cell (px, py, pz) give it, in ONE pass over the list.  need: the code byte's bits of the positions asked for (a
// neighbour bit: the clamped neighbour on that side, at pxl / pxr, pyu / pyd, pzf / pzb; OB_SELF: the cell itself).  Each position goes to
// the first body whose box holds it and stays +0 if none does.  w_a does not depend on r_a (w_x = linear_x + angular_y r_z - angular_z r_y),
// so the normal component of both x neighbours and of the cell itself is, per body, the same value formed from the cell's own (py, pz) --
// three values a body, shared by the positions it claims.  The list index is uniform (the loop runs on the argument's count): the bodies
// are read with scalar loads and nothing is indexed per lane.
struct Walls { float xm, xp, ym, yp, zm, zp, cx, cy, cz; };
__device__ __forceinline__ Walls walls_of(const BodyArgs& a, unsigned need, float pxl, float px, float pxr, float pyu, float py, float pyd,
	float pzf, float pz, float pzb)
{
	Walls w = { 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f };
	unsigned open = need;                                                  // positions no body has claimed yet
	for (int i = 0; i < a.n; ++i) {
		const BodyArg& b = a.b[i];
		const bool xl = pxl >= b.lo[0] && pxl <= b.hi[0], xc = px >= b.lo[0] && px <= b.hi[0], xr = pxr >= b.lo[0] && pxr <= b.hi[0];
		const bool yu = pyu >= b.lo[1] && pyu <= b.hi[1], yc = py >= b.lo[1] && py <= b.hi[1], yd = pyd >= b.lo[1] && pyd <= b.hi[1];
		bool zf = true, zc = true, zb = true;                               // a 2-D grid ignores z
		if (a.is3d) {
			zf = pzf >= b.lo[2] && pzf <= b.hi[2]; zc = pz >= b.lo[2] && pz <= b.hi[2]; zb = pzb >= b.lo[2] && pzb <= b.hi[2];
		}
		unsigned hit = 0;
		if (xl && yc && zc) hit |= OB_XM;
		if (xr && yc && zc) hit |= OB_XP;
		if (xc && yu && zc) hit |= OB_YM;
		if (xc && yd && zc) hit |= OB_YP;
		if (xc && yc && zf) hit |= OB_ZM;
		if (xc && yc && zb) hit |= OB_ZP;
		if (xc && yc && zc) hit |= OB_SELF;
		hit &= open;
		if (hit) {
			const float rx = px - b.piv[0], ry = py - b.piv[1], rz = pz - b.piv[2];
			float wx, wy, wz;
			if (a.is3d) {
				wx = fmaf(b.ang[1], rz, fmaf(-b.ang[2], ry, b.lin[0]));
				wy = fmaf(b.ang[2], rx, fmaf(-b.ang[0], rz, b.lin[1]));
				wz = fmaf(b.ang[0], ry, fmaf(-b.ang[1], rx, b.lin[2]));
			} else {
				wx = fmaf(-b.ang[2], ry, b.lin[0]);
				wy = fmaf(b.ang[2], rx, b.lin[1]);
				wz = 0.0f;
			}
			if (hit & OB_XM) w.xm = wx;
			if (hit & OB_XP) w.xp = wx;
			if (hit & OB_YM) w.ym = wy;
			if (hit & OB_YP) w.yp = wy;
			if (hit & OB_ZM) w.zm = wz;
			if (hit & OB_ZP) w.zp = wz;
			if (hit & OB_SELF) { w.cx = wx; w.cy = wy; w.cz = wz; }
			open &= ~hit;
		}
	}
	return w;
}

}  // namespace

// ---------------------------------------------------------------------------------------------
// enforce: the tiles of k_obstacle_enforce over the solids' bounding box
// ---------------------------------------------------------------------------------------------
template <bool HALF>
__global__ __launch_bounds__(256) void k_obstacle_enforce_mov(const Geom g, const BodyArgs a, const uint8_t* __restrict__ code,
	typename Sto<HALF>::S* __restrict__ vel, typename Sto<HALF>::S4* __restrict__ col, float* __restrict__ alpha, int x0, int y0, int z0, int tiles_x, int tiles_y)
{
	typedef Sto<HALF> St;
	int t = (int)blockIdx.x;
	const int x = x0 + (t % tiles_x) * 64 + (int)threadIdx.x; t /= tiles_x;
	const int y = y0 + (t % tiles_y) * 4 + (int)threadIdx.y, z = z0 + t / tiles_y;
	if (x >= g.X || y >= g.Y) return;
	const size_t stride = g.cells_local();
	const size_t id = (size_t)g.lz(z) * g.plane() + (size_t)y * g.X + x;
	if (!(code[id] & OB_SELF)) return;                       // fluid cells keep their bits
	const float px = centre(x, g.X), py = centre(y, g.Y), pz = centre(z, g.Zg);
	const Walls w = walls_of(a, OB_SELF, px, px, px, py, py, py, pz, pz, pz);
	St::st(vel, id, w.cx);
	St::st(vel, stride + id, w.cy);
	St::st(vel, 2 * stride + id, w.cz);
	St::zero4(col, id);
	if (alpha) alpha[id] = 0.0f;
}

// ---------------------------------------------------------------------------------------------
// divergence  b = 0.5 * (ddz + (ddy + ddx)), dd = -v(n-) + v(n+), a neighbour inside a solid reads as the solid's velocity there
// ---------------------------------------------------------------------------------------------
template <bool HALF>
__global__ __launch_bounds__(256) void k_divergence_obs_mov(const Geom g, const BodyArgs a, const typename Sto<HALF>::S* __restrict__ vel,
	const uint8_t* __restrict__ code, float* __restrict__ b, int z_begin, int nzp, int remap)
{
	typedef Sto<HALF> St;
	const Tile3 tile = tile_of((g.X + 63) >> 6, (g.Y + 3) >> 2, nzp, remap);
	const int x = tile.x * 64 + threadIdx.x;
	const int y = tile.y * 4 + threadIdx.y;
	const int z = z_begin + tile.z;
	if (x >= g.X || y >= g.Y) return;
	const size_t plane = g.plane(), stride = g.cells_local();
	const size_t zrow = (size_t)g.lz(z) * plane, row = zrow + (size_t)y * g.X;
	const unsigned k = code[row + x];
	const int xl = max(x, 1) - 1, xr = min(x + 1, g.X - 1);
	const int yu = max(y, 1) - 1, yd = min(y + 1, g.Y - 1);
	const int zf = max(z, 1) - 1, zb = min(z + 1, g.Zg - 1);
	// (every load is issued in front of the test of the code byte below: the wave waits for memory once, as k_divergence_obs does)
	const float vl = St::ld(vel, row + xl), vr = St::ld(vel, row + xr);
	const float vu = St::ld(vel, stride + zrow + (size_t)yu * g.X + x), vd = St::ld(vel, stride + zrow + (size_t)yd * g.X + x);
	float vf = 0.0f, vb = 0.0f;
	if (g.Zg > 1) {
		vf = St::ld(vel, 2 * stride + (size_t)g.lz(zf) * plane + (size_t)y * g.X + x);
		vb = St::ld(vel, 2 * stride + (size_t)g.lz(zb) * plane + (size_t)y * g.X + x);
	}
	// the walls' velocities, only in a wave that has a fluid cell beside a wall and only for the neighbours that are one (a solid cell's
	// b is 0 whatever it would have summed: the inside of a solid costs nothing)
	const unsigned kn = (k & OB_SELF) ? 0u : k;
	Walls w = { 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f };
	if (__builtin_amdgcn_ballot_w64(kn != 0) != 0)
		w = walls_of(a, kn, centre(xl, g.X), centre(x, g.X), centre(xr, g.X), centre(yu, g.Y), centre(y, g.Y), centre(yd, g.Y),
			centre(zf, g.Zg), centre(z, g.Zg), centre(zb, g.Zg));
	const float wl = w.xm, wr = w.xp, wu = w.ym, wd = w.yp, wf = w.zm, wb = w.zp;
	const float ddx = -((k & OB_XM) ? wl : vl) + ((k & OB_XP) ? wr : vr);
	const float ddy = -((k & OB_YM) ? wu : vu) + ((k & OB_YP) ? wd : vd);
	float S;
	if (g.Zg > 1) {
		const float ddz = -((k & OB_ZM) ? wf : vf) + ((k & OB_ZP) ? wb : vb);
		S = ddz + (ddy + ddx);
	} else {
		S = ddx + ddy;
	}
	b[row + x] = (k & OB_SELF) ? 0.0f : 0.5f * S;
}

// ---------------------------------------------------------------------------------------------
// projection + free slip against the moving solids + wall damping, none of it towards an open face
// ---------------------------------------------------------------------------------------------
template <bool HALF, bool OPEN>
__global__ __launch_bounds__(256) void k_project_bnd_mov(const Geom g, const SimParams sp, const BodyArgs a,
	const typename Sto<HALF>::S* __restrict__ vel_in, const float* __restrict__ p, const uint8_t* __restrict__ code,
	typename Sto<HALF>::S* __restrict__ vel_out, unsigned faces_arg, int z_begin, int nzp, int remap)
{
	const unsigned faces = OPEN ? faces_arg : 0u;
	typedef Sto<HALF> St;
	const Tile3 tile = tile_of((g.X + 63) >> 6, (g.Y + 3) >> 2, nzp, remap);
	const int x = tile.x * 64 + threadIdx.x;
	const int y = tile.y * 4 + threadIdx.y;
	const int z = z_begin + tile.z;
	if (x >= g.X || y >= g.Y) return;
	const size_t plane = g.plane(), stride = g.cells_local();
	const size_t zrow = (size_t)g.lz(z) * plane;
	const size_t id = zrow + (size_t)y * g.X + x;
	const unsigned k = (unsigned)code[id];
	const unsigned o = beyond_of(g, faces, x, y, z);
	const int xl = max(x, 1) - 1, xr = min(x + 1, g.X - 1);
	const int yu = max(y, 1) - 1, yd = min(y + 1, g.Y - 1);
	const int zf = max(z, 1) - 1, zb = min(z + 1, g.Zg - 1);
	// (every load is issued in front of the test of the code byte below: the wave waits for memory once, as k_project_bnd does)
	float u[3] = { St::ld(vel_in, id), St::ld(vel_in, stride + id), St::ld(vel_in, 2 * stride + id) };
	const float c = p[id];
	const float L = p[zrow + (size_t)y * g.X + xl], R = p[zrow + (size_t)y * g.X + xr];
	const float U = p[zrow + (size_t)yu * g.X + x], D = p[zrow + (size_t)yd * g.X + x];
	float F = 0.0f, B = 0.0f;
	if (sp.is3d) {
		F = p[(size_t)g.lz(zf) * plane + (size_t)y * g.X + x];
		B = p[(size_t)g.lz(zb) * plane + (size_t)y * g.X + x];
	}
	// what the walls give: slip[a] = u[a] of a fluid cell beside a solid along a, own[a] = the cell's own velocity where it is solid; only
	// in a wave that has either, only for the neighbours that are solid (a solid cell takes own[] whatever its neighbours are)
	const unsigned kn = (k & OB_SELF) ? 0u : k;
	float slip[3] = { 0.0f, 0.0f, 0.0f }, own[3] = { 0.0f, 0.0f, 0.0f };
	if (__builtin_amdgcn_ballot_w64(k != 0) != 0) {
		const Walls w = walls_of(a, kn | (k & OB_SELF), centre(xl, g.X), centre(x, g.X), centre(xr, g.X), centre(yu, g.Y), centre(y, g.Y), centre(yd, g.Y),
			centre(zf, g.Zg), centre(z, g.Zg), centre(zb, g.Zg));
		slip[0] = (kn & OB_XM) ? ((kn & OB_XP) ? 0.5f * (w.xm + w.xp) : w.xm) : w.xp;
		slip[1] = (kn & OB_YM) ? ((kn & OB_YP) ? 0.5f * (w.ym + w.yp) : w.ym) : w.yp;
		slip[2] = (kn & OB_ZM) ? ((kn & OB_ZP) ? 0.5f * (w.zm + w.zp) : w.zm) : w.zp;
		own[0] = w.cx; own[1] = w.cy; own[2] = w.cz;
	}
	float grad[3];
	grad[0] = -((o & OB_XM) ? 0.0f : (k & OB_XM) ? c : L) + ((o & OB_XP) ? 0.0f : (k & OB_XP) ? c : R);
	grad[1] = -((o & OB_YM) ? 0.0f : (k & OB_YM) ? c : U) + ((o & OB_YP) ? 0.0f : (k & OB_YP) ? c : D);
	grad[2] = 0.0f;
	float kd = 0.5f;
	if (sp.is3d) {
		grad[2] = -((o & OB_ZM) ? 0.0f : (k & OB_ZM) ? c : F) + ((o & OB_ZP) ? 0.0f : (k & OB_ZP) ? c : B);
		kd = __uint_as_float(0x3f855556u);                                 // 0.5f / 0.48f, as k_project
		u[2] = fmaf(-grad[2], kd, u[2]);
	}
	u[0] = fmaf(-grad[0], kd, u[0]);
	u[1] = fmaf(-grad[1], kd, u[1]);
	// free slip against a moving solid: along an axis on which a neighbour is solid the flow is the wall's (the z bits are 0 on 2-D grids)
	if (k & (OB_XM | OB_XP)) u[0] = slip[0];
	if (k & (OB_YM | OB_YP)) u[1] = slip[1];
	if (k & (OB_ZM | OB_ZP)) u[2] = slip[2];
	const int cell[3] = { x, y, z };
	const float dims[3] = { (float)g.X, (float)g.Y, (float)g.Zg };
#pragma unroll
	for (int ax = 0; ax < 3; ++ax) {                                       // the wall damping of k_project, except towards an open face
		float pos = ((float)cell[ax] + 0.5f) / dims[ax];
		if (sp.is3d || ax < 2) pos = fmaf(pos, 2.0f, -1.0f);
		float f = (-fabsf(pos) + 0.970000029f) * 33.3333359f;
		f = fminf(fmaxf(f, -1.0f), 1.0f);
		const bool open = (pos < 0.0f && ((faces >> (2 * ax)) & 1u)) || (pos > 0.0f && ((faces >> (2 * ax + 1)) & 1u));
		const float w = (0.0f < u[ax] * pos && !open) ? f : 1.0f;
		St::st(vel_out, ax * stride + id, (k & OB_SELF) ? own[ax] : u[ax] * w);
	}
}

// ---------------------------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------------------------
static inline dim3 grid_cells(const Geom& g, int nzp) { return dim3(((g.X + 63) / 64) * ((g.Y + 3) / 4) * nzp, 1, 1); }
// fx_obstacle.hip's remap_small: divergence and projection take the contiguous-eighth order on the small 3-D grids that live in L2
static inline int remap_small(const Geom& g) { return g.Zg > 1 && g.plane() <= 32768 && g.cells_local() < (size_t)6 << 20 ? 1 : 0; }

// the list as the kernels take it; false: no list, or more bodies than the argument holds
static bool body_args(const Geom& g, const fx_obstacle_body* list, int count, BodyArgs* out)
{
	if (!list || count <= 0 || count > (int)FX_MAX_OBSTACLE_BODIES) return false;
	out->n = count;
	out->is3d = g.Zg > 1 ? 1 : 0;
	for (int i = 0; i < count; ++i)
		for (int c = 0; c < 3; ++c) {
			out->b[i].lo[c] = list[i].box_lo[c]; out->b[i].hi[c] = list[i].box_hi[c];
			out->b[i].lin[c] = list[i].linear[c]; out->b[i].ang[c] = list[i].angular[c]; out->b[i].piv[c] = list[i].pivot[c];
		}
	return true;
}

hipError_t launch_obstacle_enforce_mov(const Geom& g, int half_store, const uint8_t* code, const int lo[3], const int hi[3],
	const fx_obstacle_body* list, int count, void* vel, void* col, float* alpha, hipStream_t s)
{
	if (!whole_grid(g)) return hipErrorNotSupported;
	BodyArgs a;
	if (!code || !body_args(g, list, count, &a)) return hipErrorInvalidValue;
	int x0, y0, tx, ty;
	const long long wgs = obstacle_enforce_tiles(lo, hi, &x0, &y0, &tx, &ty);
	if (wgs <= 0) return hipSuccess;                                          // no solid cell: nothing to launch
	if (wgs > 0x7fffffffLL || hi[0] > g.X || hi[1] > g.Y || hi[2] > g.Zg || lo[0] < 0 || lo[1] < 0 || lo[2] < 0) return hipErrorInvalidValue;
	const dim3 grid((unsigned)wgs, 1, 1), block(64, 4, 1);
	if (half_store) hipLaunchKernelGGL(k_obstacle_enforce_mov<true>, grid, block, 0, s, g, a, code, (h16*)vel, (h16x4*)col, alpha, x0, y0, lo[2], tx, ty);
	else hipLaunchKernelGGL(k_obstacle_enforce_mov<false>, grid, block, 0, s, g, a, code, (float*)vel, (float4*)col, alpha, x0, y0, lo[2], tx, ty);
	return hipGetLastError();
}

hipError_t launch_divergence_obs_mov(const Geom& g, int half_store, const void* vel, const uint8_t* code, const fx_obstacle_body* list, int count,
	float* b, int z_begin, int z_end, hipStream_t s)
{
	if (!whole_grid(g)) return hipErrorNotSupported;
	BodyArgs a;
	if (!code || !body_args(g, list, count, &a) || z_begin < 0 || z_end > g.Zg) return hipErrorInvalidValue;
	if (z_end <= z_begin) return hipSuccess;
	const dim3 grid = grid_cells(g, z_end - z_begin), block(64, 4, 1);
	if (half_store) hipLaunchKernelGGL(k_divergence_obs_mov<true>, grid, block, 0, s, g, a, (const h16*)vel, code, b, z_begin, z_end - z_begin, remap_small(g));
	else hipLaunchKernelGGL(k_divergence_obs_mov<false>, grid, block, 0, s, g, a, (const float*)vel, code, b, z_begin, z_end - z_begin, remap_small(g));
	return hipGetLastError();
}

template <bool HALF>
static hipError_t launch_project_bnd_mov_t(const Geom& g, const SimParams& sp, const BodyArgs& a, const void* vel_in, const float* p, const uint8_t* code,
	void* vel_out, unsigned faces, int z_begin, int nzp, hipStream_t s)
{
	typedef typename Sto<HALF>::S S;
	const auto k = faces ? k_project_bnd_mov<HALF, true> : k_project_bnd_mov<HALF, false>;
	hipLaunchKernelGGL(k, grid_cells(g, nzp), dim3(64, 4, 1), 0, s, g, sp, a, (const S*)vel_in, p, code, (S*)vel_out, faces, z_begin, nzp, remap_small(g));
	return hipGetLastError();
}

hipError_t launch_project_bnd_mov(const Geom& g, const SimParams& sp, int half_store, const void* vel_in, const float* p, const uint8_t* code,
	const fx_obstacle_body* list, int count, void* vel_out, unsigned faces, int z_begin, int z_end, hipStream_t s)
{
	if (!whole_grid(g)) return hipErrorNotSupported;
	BodyArgs a;
	if (!code || !body_args(g, list, count, &a) || !open_faces_ok(g, faces) || z_begin < 0 || z_end > g.Zg) return hipErrorInvalidValue;
	if (z_end <= z_begin) return hipSuccess;
	return half_store ? launch_project_bnd_mov_t<true>(g, sp, a, vel_in, p, code, vel_out, faces, z_begin, z_end - z_begin, s)
	                  : launch_project_bnd_mov_t<false>(g, sp, a, vel_in, p, code, vel_out, faces, z_begin, z_end - z_begin, s);
}

}  // namespace fx
