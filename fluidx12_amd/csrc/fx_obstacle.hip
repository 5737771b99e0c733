// fx_obstacle.hip -- the boundary-aware pressure kernels, gfx950: voxelised solid obstacles inside the box (fx_set_obstacles) and open walls
// (fx_set_open_walls; their inflow pass is fx_open.hip).  No reference counterpart: the reference's only boundaries are six closed walls (the
// clamped neighbour indices of its projection shaders); Harris / Crane et al. (GPU Gems 3, ch. 30) is the scheme of the solids, whose
// velocity w (fx_set_obstacle_bodies; +0 at rest) enters the enforce pass, the divergence and the boundary rule of the projection.
//
//   k_obstacle_codes    mask uint8[Z][Y][X] -> one code byte per cell (+ the count of solid cells and their bounding box)
//   k_obstacle_enforce  solid cells: VELOCITY1 = w(c), COLOR (and the render's alpha side volume) +0; over the solids' bounding box only
//   k_divergence_obs    k_divergence with  v_a(n) -> S(n) ? w_a(n) : v_a(n),  b = 0 in a solid cell
//   k_jacobi_bnd(_v4)   one lock-step sweep with  p(n) -> q(n) = beyond an open face ? +0 : S(n) ? p(c) : p(n),  p_out = 0 in a solid cell
//   k_project_bnd       k_project with the same q, u[a] = the wall's w_a beside a solid along a (free slip; both sides solid: their mean),
//                       w(c) in a solid cell, and no wall damping of axis a towards an open face of a
//
// w(n) of a solid cell n: B(n) = the first body of the list whose closed box holds the cell centre pos(n) = ((float)i + 0.5f) / (float)N per
// axis (a 2-D grid ignores z); r = pos(n) - pivot;
//   w_x = fmaf(angular_y, r_z, fmaf(-angular_z, r_y, linear_x))
//   w_y = fmaf(angular_z, r_x, fmaf(-angular_x, r_z, linear_y))
//   w_z = fmaf(angular_x, r_y, fmaf(-angular_y, r_x, linear_z))
// 2-D grids: w_x = fmaf(-angular_z, r_y, linear_x), w_y = fmaf(angular_z, r_x, linear_y), w_z = +0.  No box holds the cell: w = +0.
// The three kernels that see w are templated on MOV.  MOV = 0 (an empty list: the solids rest) has w = +0 as a compile-time constant and no
// list in its argument block.  MOV = 1 gets the bodies as a kernel argument (no device memory, no copy: a new list every frame is free) and
// evaluates w only for the neighbours the code byte calls solid -- one loop over the list (uniform loads of the argument, a compare per
// axis and position) behind a wave-uniform test of the byte's bits, with every field load issued in front of that test, so a wave none of
// whose cells has a solid neighbour executes the resting arithmetic and nothing else.  The relaxation never sees w: the pressure ghost of a
// moving wall is still the cell's own pressure.  Bodies all of whose velocities are +0 give the resting kernels' bits
// (tests/test_gpu_moving_obstacles.py, which also holds MOV = 1 bit for bit against the numpy model tests/moving_obstacle_ref.py).
//
// The wall rule of the plain kernels is "a neighbour that is not there reads as the cell itself" (clamped indices); a solid extends it to
// neighbours inside an obstacle.  The stencil kernels never read the mask: the code byte of a cell holds S of its six CLAMPED neighbours
// (bit 0..5: x-1, x+1, y-1, y+1, z-1, z+1; the z bits are 0 on 2-D grids) and of the cell itself (bit 6), built once per fx_set_obstacles.
// "Beyond an open face" = a stencil neighbour whose unclamped index is -1 or N on an axis whose face there is open (FX_WALL_*: the code
// byte's bit order), a Dirichlet ghost p = 0.  The divergence has no open rule: its clamped neighbour is the zero-gradient velocity ghost
// already.  The open rule costs no bytes: it replaces the clamped replica of a cell by +0 at the ends of a row and in the rows / planes on a
// face, which are then not loaded at all.
// The bnd kernels are templated on CODE (a code volume is present) and OPEN (a face is open), and three combinations exist: (1, 0) obstacles
// in a closed box, (1, 1) both, (0, 1) open walls alone, which read no code byte (12 bytes per cell and sweep; 13 with).  Without either the
// plain kernels of fx_sim.hip run.  With OPEN = 0 the faces are a compile-time zero and nothing of the open rule is left in the kernel.
// Every substitution is a select on a loaded value -- no branch, no divergence -- and with an all-zero mask and no open face each kernel is,
// operation for operation, its plain counterpart of fx_sim.hip (tests/test_gpu_obstacles.py holds them bit for bit against each other and
// against tests/obstacle_ref/, tests/test_gpu_open_walls.py against the numpy model tests/open_ref.py).  fp32 arithmetic in the plain
// kernels' association order; fp16 storage widens on load and rounds once (RNE) on store -- w too, where it is stored; where the divergence
// and the projection read it, it is the fp32 value.
// Whole grids only (fx_set_obstacles, fx_set_obstacle_bodies and fx_set_open_walls refuse slab ranks): local plane = global plane.
#include <type_traits>
#include "fx_internal.h"
#include "fx_store.h"

namespace fx {

using namespace sto;

// what the MOV kernels get as their last argument: the list by value and whether the grid is 3-D (MOV = 1), nothing (MOV = 0)
struct BodyArg { float lo[3], hi[3], lin[3], ang[3], piv[3]; };
struct BodyArgs { int n, is3d; BodyArg b[FX_MAX_OBSTACLE_BODIES]; };
struct NoBodies {};
template <bool MOV> using Bodies = typename std::conditional<MOV, BodyArgs, NoBodies>::type;

namespace {

// workgroup -> tile, the mapping of the plain kernels (fx_sim.hip xcd_tile): remap 1 = XCD k walks the k-th contiguous eighth of the
// (x, y, z)-ordered tile sequence, 0 = natural order.  Speed only.
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

// the faces a cell's neighbours lie beyond: bit a of `faces` survives where the cell sits on that face (the z bits never on a 2-D grid:
// fx_set_open_walls refuses them)
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
// code bytes.  stats: { solid cells (two words, low first), min x, y, z, max x, y, z } -- zeroed / set to (INT_MAX, 0) by the launcher
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_obstacle_codes(const Geom g, const uint8_t* __restrict__ solid, uint8_t* __restrict__ code,
	unsigned* __restrict__ stats)
{
	const int gx = (g.X + 63) >> 6, gy = (g.Y + 3) >> 2;
	int t = (int)blockIdx.x;
	const int tx = t % gx; t /= gx;
	const int x = tx * 64 + (int)threadIdx.x, y = (t % gy) * 4 + (int)threadIdx.y, z = t / gy;
	const bool in = x < g.X && y < g.Y;
	unsigned self = 0;
	if (in) {
		const size_t plane = g.plane();
		const int xl = max(x, 1) - 1, xr = min(x + 1, g.X - 1);
		const int yu = max(y, 1) - 1, yd = min(y + 1, g.Y - 1);
		const size_t zrow = (size_t)z * plane, row = zrow + (size_t)y * g.X;
		unsigned k = 0;
		self = solid[row + x] ? 1u : 0u;
		k |= solid[row + xl] ? OB_XM : 0;
		k |= solid[row + xr] ? OB_XP : 0;
		k |= solid[zrow + (size_t)yu * g.X + x] ? OB_YM : 0;
		k |= solid[zrow + (size_t)yd * g.X + x] ? OB_YP : 0;
		if (g.Zg > 1) {
			const int zf = max(z, 1) - 1, zb = min(z + 1, g.Zg - 1);
			k |= solid[(size_t)zf * plane + (size_t)y * g.X + x] ? OB_ZM : 0;
			k |= solid[(size_t)zb * plane + (size_t)y * g.X + x] ? OB_ZP : 0;
		}
		k |= self ? OB_SELF : 0;
		code[row + x] = (uint8_t)k;
	}
	// one wave = one row of the tile: its solid cells share y and z
	const unsigned long long m = __builtin_amdgcn_ballot_w64(self != 0);
	if (m == 0 || (threadIdx.x & 63) != 0) return;
	const int x0 = tx * 64;
	const unsigned n = (unsigned)__builtin_popcountll(m);
	if (atomicAdd(stats, n) + n < n) atomicAdd(stats + 1, 1u);              // carry into the high word
	atomicMin(reinterpret_cast<int*>(stats) + 2, x0 + (int)__builtin_ctzll(m));
	atomicMax(reinterpret_cast<int*>(stats) + 5, x0 + 63 - (int)__builtin_clzll(m));
	atomicMin(reinterpret_cast<int*>(stats) + 3, y); atomicMax(reinterpret_cast<int*>(stats) + 6, y);
	atomicMin(reinterpret_cast<int*>(stats) + 4, z); atomicMax(reinterpret_cast<int*>(stats) + 7, z);
}

// the mask back out of the code bytes (fx_get_obstacles): 0 / 1 per cell
__global__ __launch_bounds__(256) void k_obstacle_mask(const uint8_t* __restrict__ code, uint8_t* __restrict__ solid, size_t n)
{
	for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) solid[i] = (code[i] >> 6) & 1u;
}

// ---------------------------------------------------------------------------------------------
// enforce: 64 x 4 x 1 tiles on the grid's own raster over the solids' bounding box, first tile at (x0, y0, z0)
// ---------------------------------------------------------------------------------------------
template <bool HALF, bool MOV>
__global__ __launch_bounds__(256) void k_obstacle_enforce(const Geom g, const uint8_t* __restrict__ code, typename Sto<HALF>::S* __restrict__ vel,
	typename Sto<HALF>::S4* __restrict__ col, float* __restrict__ alpha, int x0, int y0, int z0, int tiles_x, int tiles_y, const Bodies<MOV> a)
{
	typedef Sto<HALF> St;
	int t = (int)blockIdx.x;
	const int x = x0 + (t % tiles_x) * 64 + (int)threadIdx.x; t /= tiles_x;
	const int y = y0 + (t % tiles_y) * 4 + (int)threadIdx.y, z = z0 + t / tiles_y;
	if (x >= g.X || y >= g.Y) return;
	const size_t stride = g.cells_local();
	const size_t id = (size_t)g.lz(z) * g.plane() + (size_t)y * g.X + x;
	if (!(code[id] & OB_SELF)) return;                       // fluid cells keep their bits
	Walls w = { 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f };
	if constexpr (MOV) {
		const float px = centre(x, g.X), py = centre(y, g.Y), pz = centre(z, g.Zg);
		w = walls_of(a, OB_SELF, px, px, px, py, py, py, pz, pz, pz);
	}
	St::st(vel, id, w.cx);
	St::st(vel, stride + id, w.cy);
	St::st(vel, 2 * stride + id, w.cz);
	St::zero4(col, id);
	if (alpha) alpha[id] = 0.0f;
}

// ---------------------------------------------------------------------------------------------
// divergence  b = 0.5 * (ddz + (ddy + ddx)), dd = -v(n-) + v(n+), a neighbour inside a solid reads as the solid's velocity there
// ---------------------------------------------------------------------------------------------
template <bool HALF, bool MOV>
__global__ __launch_bounds__(256) void k_divergence_obs(const Geom g, const typename Sto<HALF>::S* __restrict__ vel, const uint8_t* __restrict__ code,
	float* __restrict__ b, int z_begin, int nzp, int remap, const Bodies<MOV> a)
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
	const float vl = St::ld(vel, row + xl), vr = St::ld(vel, row + xr);
	const float vu = St::ld(vel, stride + zrow + (size_t)yu * g.X + x), vd = St::ld(vel, stride + zrow + (size_t)yd * g.X + x);
	float vf = 0.0f, vb = 0.0f;
	Walls w = { 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f };
	if constexpr (MOV) {
		// every load is issued in front of the test of the code byte below: the wave waits for memory once, as at rest (MOV = 0 loads z
		// where it sums it, which is what keeps that kernel's registers and control flow)
		if (g.Zg > 1) {
			vf = St::ld(vel, 2 * stride + (size_t)g.lz(zf) * plane + (size_t)y * g.X + x);
			vb = St::ld(vel, 2 * stride + (size_t)g.lz(zb) * plane + (size_t)y * g.X + x);
		}
		// the walls' velocities, only in a wave that has a fluid cell beside a wall and only for the neighbours that are one (a solid cell's
		// b is 0 whatever it would have summed: the inside of a solid costs nothing)
		const unsigned kn = (k & OB_SELF) ? 0u : k;
		if (__builtin_amdgcn_ballot_w64(kn != 0) != 0)
			w = walls_of(a, kn, centre(xl, g.X), centre(x, g.X), centre(xr, g.X), centre(yu, g.Y), centre(y, g.Y), centre(yd, g.Y),
				centre(zf, g.Zg), centre(z, g.Zg), centre(zb, g.Zg));
	}
	const float ddx = -((k & OB_XM) ? w.xm : vl) + ((k & OB_XP) ? w.xp : vr);
	const float ddy = -((k & OB_YM) ? w.ym : vu) + ((k & OB_YP) ? w.yp : vd);
	float S;
	if (g.Zg > 1) {
		if constexpr (!MOV) {
			vf = St::ld(vel, 2 * stride + (size_t)g.lz(zf) * plane + (size_t)y * g.X + x);
			vb = St::ld(vel, 2 * stride + (size_t)g.lz(zb) * plane + (size_t)y * g.X + x);
		}
		const float ddz = -((k & OB_ZM) ? w.zm : vf) + ((k & OB_ZP) ? w.zp : vb);
		S = ddz + (ddy + ddx);
	} else {
		S = ddx + ddy;
	}
	b[row + x] = (k & OB_SELF) ? 0.0f : 0.5f * S;
}

// ---------------------------------------------------------------------------------------------
// Jacobi sweep, scalar: any extent, 2-D / 3-D
//   x = ((((((qL - b) + qR) + qU) + qD) + qF) + qB) * (1/6)     2-D: ((((qL - b) + qR) + qU) + qD) * 1/4
// ---------------------------------------------------------------------------------------------
template <bool CODE, bool OPEN>
__global__ __launch_bounds__(256) void k_jacobi_bnd(const Geom g, const float* __restrict__ p_in, const float* __restrict__ b,
	const uint8_t* __restrict__ code, float* __restrict__ p_out, unsigned faces_arg, int z_begin, int nzp, int remap)
{
	const unsigned faces = OPEN ? faces_arg : 0u;
	const Tile3 tile = tile_of((g.X + 63) >> 6, (g.Y + 3) >> 2, nzp, remap);
	const int x = tile.x * 64 + threadIdx.x;
	const int y = tile.y * 4 + threadIdx.y;
	const int z = z_begin + tile.z;
	if (x >= g.X || y >= g.Y) return;
	const size_t plane = g.plane();
	const size_t zrow = (size_t)g.lz(z) * plane;
	const size_t id = zrow + (size_t)y * g.X + x;
	const unsigned k = CODE ? (unsigned)code[id] : 0u;
	const unsigned o = beyond_of(g, faces, x, y, z);
	const float c = p_in[id];
	const int xl = max(x, 1) - 1, xr = min(x + 1, g.X - 1);
	const int yu = max(y, 1) - 1, yd = min(y + 1, g.Y - 1);
	const float L = p_in[zrow + (size_t)y * g.X + xl], R = p_in[zrow + (size_t)y * g.X + xr];
	const float U = p_in[zrow + (size_t)yu * g.X + x], D = p_in[zrow + (size_t)yd * g.X + x];
	float s = ((o & OB_XM) ? 0.0f : (k & OB_XM) ? c : L) - b[id];
	s = ((o & OB_XP) ? 0.0f : (k & OB_XP) ? c : R) + s;
	s = ((o & OB_YM) ? 0.0f : (k & OB_YM) ? c : U) + s;
	s = ((o & OB_YP) ? 0.0f : (k & OB_YP) ? c : D) + s;
	float inv = 0.25f;
	if (g.Zg > 1) {
		const int zf = max(z, 1) - 1, zb = min(z + 1, g.Zg - 1);
		const float F = p_in[(size_t)g.lz(zf) * plane + (size_t)y * g.X + x], B = p_in[(size_t)g.lz(zb) * plane + (size_t)y * g.X + x];
		s = ((o & OB_ZM) ? 0.0f : (k & OB_ZM) ? c : F) + s;
		s = ((o & OB_ZP) ? 0.0f : (k & OB_ZP) ? c : B) + s;
		inv = __uint_as_float(0x3e2aaaabu);
	}
	p_out[id] = (k & OB_SELF) ? 0.0f : s * inv;
}

// ---------------------------------------------------------------------------------------------
// Jacobi sweep, 3-D, X % 4 == 0: k_jacobi_v4's scheme (one thread = 4 consecutive x: 16-byte loads of the five p rows and of b, a 16-byte
// store, the x neighbours of the row's ends through DPP lane shifts) + with CODE one 4-byte load for the four cells' codes: 13 bytes per
// cell and sweep against 12, twenty-four selects and four for the solid cells themselves.  With OPEN the clamped replica becomes +0 at
// x4 == 0 / X4 - 1 and in the rows and planes on an open face, whose row beyond is not loaded.  A cell on a face is its own clamped
// neighbour there, so its code bit for that side is its own solid bit: the select behind the +0 only ever changes a solid cell, whose
// result is 0 whatever it summed.  Bit-identical to k_jacobi_bnd.
// ---------------------------------------------------------------------------------------------
template <bool CODE, bool OPEN>
__global__ __launch_bounds__(256) void k_jacobi_bnd_v4(const Geom g, const float* __restrict__ p_in, const float* __restrict__ b,
	const uint8_t* __restrict__ code, float* __restrict__ p_out, unsigned faces_arg, int z_begin, int nzp, int remap, int rows_per_block)
{
	const unsigned faces = OPEN ? faces_arg : 0u;
	const int X4 = g.X >> 2;
	const int lane = threadIdx.x;                       // float4 column
	const Tile3 tile = tile_of((X4 + (int)blockDim.x - 1) / (int)blockDim.x, (g.Y + rows_per_block - 1) / rows_per_block, nzp, remap);
	const int x4 = tile.x * blockDim.x + lane;
	const int y = tile.y * rows_per_block + threadIdx.y;
	const int z = z_begin + tile.z;
	if (x4 >= X4 || y >= g.Y) return;
	const size_t plane = g.plane();
	const int yu = max(y, 1) - 1, yd = min(y + 1, g.Y - 1);
	const int zf = max(z, 1) - 1, zb = min(z + 1, g.Zg - 1);
	const size_t zrow = (size_t)g.lz(z) * plane;
	const size_t c_off = zrow + (size_t)y * g.X + 4 * x4;
	const float4 zero4 = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
	const bool oU = (faces & OB_YM) && y == 0, oD = (faces & OB_YP) && y == g.Y - 1;
	const bool oF = (faces & OB_ZM) && z == 0, oB = (faces & OB_ZP) && z == g.Zg - 1;
	const float4 c = *reinterpret_cast<const float4*>(p_in + c_off);
	float4 U = zero4, D = zero4, F = zero4, B = zero4;                         // (a row or plane beyond an open face is not loaded)
	if (!oU) U = *reinterpret_cast<const float4*>(p_in + zrow + (size_t)yu * g.X + 4 * x4);
	if (!oD) D = *reinterpret_cast<const float4*>(p_in + zrow + (size_t)yd * g.X + 4 * x4);
	if (!oF) F = *reinterpret_cast<const float4*>(p_in + (size_t)g.lz(zf) * plane + (size_t)y * g.X + 4 * x4);
	if (!oB) B = *reinterpret_cast<const float4*>(p_in + (size_t)g.lz(zb) * plane + (size_t)y * g.X + 4 * x4);
	const float4 bb = *reinterpret_cast<const float4*>(b + c_off);
	uint32_t kk = 0;
	if (CODE) kk = *reinterpret_cast<const uint32_t*>(code + c_off);           // (X % 4 == 0: every group of four cells is 4-byte aligned)
	// x neighbours: the adjacent float4 column sits in the adjacent lane (DPP wave_shr:1 / wave_shl:1, as k_jacobi_v4); only a wave's
	// first / last lane inside a row still loads them
	const int wl = (int)((threadIdx.y * blockDim.x + threadIdx.x) & 63);
	float L = __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, c.w), 0x138, 0xf, 0xf, false));
	float R = __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, c.x), 0x130, 0xf, 0xf, false));
	if (x4 == 0) L = (faces & OB_XM) ? 0.0f : c.x; else if (wl == 0 || lane == 0) L = p_in[c_off - 1];
	if (x4 == X4 - 1) R = (faces & OB_XP) ? 0.0f : c.w; else if (wl == 63 || lane == (int)blockDim.x - 1) R = p_in[c_off + 4];
	const float inv = __uint_as_float(0x3e2aaaabu);
	const float pc[4] = { c.x, c.y, c.z, c.w };
	const float pl[4] = { L, c.x, c.y, c.z }, pr[4] = { c.y, c.z, c.w, R };
	const float pu[4] = { U.x, U.y, U.z, U.w }, pd[4] = { D.x, D.y, D.z, D.w };
	const float pf[4] = { F.x, F.y, F.z, F.w }, pb[4] = { B.x, B.y, B.z, B.w };
	const float bv[4] = { bb.x, bb.y, bb.z, bb.w };
	float o[4];
#pragma unroll
	for (int i = 0; i < 4; ++i) {
		if (CODE) {
			const unsigned k = kk >> (8 * i);
			float s = ((k & OB_XM) ? pc[i] : pl[i]) - bv[i];
			s = ((k & OB_XP) ? pc[i] : pr[i]) + s;
			s = ((k & OB_YM) ? pc[i] : pu[i]) + s;
			s = ((k & OB_YP) ? pc[i] : pd[i]) + s;
			s = ((k & OB_ZM) ? pc[i] : pf[i]) + s;
			s = ((k & OB_ZP) ? pc[i] : pb[i]) + s;
			o[i] = (k & OB_SELF) ? 0.0f : s * inv;
		} else {
			float s = pl[i] - bv[i];
			s = pr[i] + s;
			s = pu[i] + s;
			s = pd[i] + s;
			s = pf[i] + s;
			s = pb[i] + s;
			o[i] = s * inv;
		}
	}
	*reinterpret_cast<float4*>(p_out + c_off) = make_float4(o[0], o[1], o[2], o[3]);
}

// ---------------------------------------------------------------------------------------------
// projection + free slip against the solids + wall damping, none of it towards an open face
// ---------------------------------------------------------------------------------------------
template <bool HALF, bool CODE, bool OPEN, bool MOV>
__global__ __launch_bounds__(256) void k_project_bnd(const Geom g, const SimParams sp,
	const typename Sto<HALF>::S* __restrict__ vel_in, const float* __restrict__ p, const uint8_t* __restrict__ code,
	typename Sto<HALF>::S* __restrict__ vel_out, unsigned faces_arg, int z_begin, int nzp, int remap, const Bodies<MOV> a)
{
	static_assert(CODE || !MOV, "the solids' velocities need the code byte");
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
	const unsigned k = CODE ? (unsigned)code[id] : 0u;
	const unsigned o = beyond_of(g, faces, x, y, z);
	const int xl = max(x, 1) - 1, xr = min(x + 1, g.X - 1);
	const int yu = max(y, 1) - 1, yd = min(y + 1, g.Y - 1);
	const int zf = max(z, 1) - 1, zb = min(z + 1, g.Zg - 1);
	float u[3] = { St::ld(vel_in, id), St::ld(vel_in, stride + id), St::ld(vel_in, 2 * stride + id) };
	const float c = p[id];
	const float L = p[zrow + (size_t)y * g.X + xl], R = p[zrow + (size_t)y * g.X + xr];
	const float U = p[zrow + (size_t)yu * g.X + x], D = p[zrow + (size_t)yd * g.X + x];
	float F = 0.0f, B = 0.0f;
	// what the walls give: slip[a] = u[a] of a fluid cell beside a solid along a, own[a] = the cell's own velocity where it is solid; +0 at rest
	float slip[3] = { 0.0f, 0.0f, 0.0f }, own[3] = { 0.0f, 0.0f, 0.0f };
	if constexpr (MOV) {
		// every load is issued in front of the test of the code byte below: the wave waits for memory once, as at rest (MOV = 0 loads z
		// where it forms grad[2], which is what keeps those kernels' registers and control flow)
		if (sp.is3d) {
			F = p[(size_t)g.lz(zf) * plane + (size_t)y * g.X + x];
			B = p[(size_t)g.lz(zb) * plane + (size_t)y * g.X + x];
		}
		// only in a wave that has either, only for the neighbours that are solid (a solid cell takes own[] whatever its neighbours are)
		const unsigned kn = (k & OB_SELF) ? 0u : k;
		if (__builtin_amdgcn_ballot_w64(k != 0) != 0) {
			const Walls w = walls_of(a, kn | (k & OB_SELF), centre(xl, g.X), centre(x, g.X), centre(xr, g.X), centre(yu, g.Y), centre(y, g.Y), centre(yd, g.Y),
				centre(zf, g.Zg), centre(z, g.Zg), centre(zb, g.Zg));
			slip[0] = (kn & OB_XM) ? ((kn & OB_XP) ? 0.5f * (w.xm + w.xp) : w.xm) : w.xp;
			slip[1] = (kn & OB_YM) ? ((kn & OB_YP) ? 0.5f * (w.ym + w.yp) : w.ym) : w.yp;
			slip[2] = (kn & OB_ZM) ? ((kn & OB_ZP) ? 0.5f * (w.zm + w.zp) : w.zm) : w.zp;
			own[0] = w.cx; own[1] = w.cy; own[2] = w.cz;
		}
	}
	float grad[3];
	grad[0] = -((o & OB_XM) ? 0.0f : (k & OB_XM) ? c : L) + ((o & OB_XP) ? 0.0f : (k & OB_XP) ? c : R);
	grad[1] = -((o & OB_YM) ? 0.0f : (k & OB_YM) ? c : U) + ((o & OB_YP) ? 0.0f : (k & OB_YP) ? c : D);
	grad[2] = 0.0f;
	float kd = 0.5f;
	if (sp.is3d) {
		if constexpr (!MOV) {
			F = p[(size_t)g.lz(zf) * plane + (size_t)y * g.X + x];
			B = p[(size_t)g.lz(zb) * plane + (size_t)y * g.X + x];
		}
		grad[2] = -((o & OB_ZM) ? 0.0f : (k & OB_ZM) ? c : F) + ((o & OB_ZP) ? 0.0f : (k & OB_ZP) ? c : B);
		kd = __uint_as_float(0x3f855556u);                                 // 0.5f / 0.48f, as k_project
		u[2] = fmaf(-grad[2], kd, u[2]);
	}
	u[0] = fmaf(-grad[0], kd, u[0]);
	u[1] = fmaf(-grad[1], kd, u[1]);
	// free slip against a solid: along an axis on which a neighbour is solid the flow is the wall's (the z bits are 0 on 2-D grids)
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
// the plain kernels' defaults (fx_sim.hip xcd_remap_for): the sweeps always take the contiguous-eighth order, divergence and projection on
// the small 3-D grids that live in L2
static inline int remap_small(const Geom& g) { return g.Zg > 1 && g.plane() <= 32768 && g.cells_local() < (size_t)6 << 20 ? 1 : 0; }

hipError_t launch_obstacle_codes(const Geom& g, const uint8_t* solid_dev, uint8_t* code, unsigned* stats_dev, hipStream_t s)
{
	if (!whole_grid(g)) return hipErrorNotSupported;
	const unsigned init[8] = { 0u, 0u, 0x7fffffffu, 0x7fffffffu, 0x7fffffffu, 0u, 0u, 0u };
	hipError_t e = hipMemcpyAsync(stats_dev, init, sizeof init, hipMemcpyHostToDevice, s);     // (pageable source: copied out before the call returns)
	if (e != hipSuccess) return e;
	hipLaunchKernelGGL(k_obstacle_codes, grid_cells(g, g.Zg), dim3(64, 4, 1), 0, s, g, solid_dev, code, stats_dev);
	return hipGetLastError();
}

hipError_t launch_obstacle_mask(const uint8_t* code, uint8_t* solid_dev, size_t n, hipStream_t s)
{
	if (!n) return hipSuccess;
	const unsigned grid = (unsigned)((n + 255) / 256 < 4096 ? (n + 255) / 256 : 4096);
	hipLaunchKernelGGL(k_obstacle_mask, dim3(grid), dim3(256), 0, s, code, solid_dev, n);
	return hipGetLastError();
}

// the tiles of the enforce launch: the box [lo, hi) on the grid's 64 x 4 raster -> workgroups (host code, no device needed)
long long obstacle_enforce_tiles(const int lo[3], const int hi[3], int* x0, int* y0, int* tiles_x, int* tiles_y)
{
	if (hi[0] <= lo[0] || hi[1] <= lo[1] || hi[2] <= lo[2]) return 0;
	*x0 = lo[0] & ~63; *y0 = lo[1] & ~3;
	*tiles_x = (hi[0] - *x0 + 63) / 64; *tiles_y = (hi[1] - *y0 + 3) / 4;
	return (long long)*tiles_x * *tiles_y * (hi[2] - lo[2]);
}

// the list as the MOV kernels take it.  count 0: the solids rest and *out is not written; a list needs a code volume and fits the argument
static hipError_t body_args(const Geom& g, const uint8_t* code, const fx_obstacle_body* list, int count, BodyArgs* out)
{
	if (count == 0) return hipSuccess;
	if (!code || !list || count < 0 || count > (int)FX_MAX_OBSTACLE_BODIES) return hipErrorInvalidValue;
	out->n = count;
	out->is3d = g.Zg > 1 ? 1 : 0;
	for (int i = 0; i < count; ++i)
		for (int c = 0; c < 3; ++c) {
			out->b[i].lo[c] = list[i].box_lo[c]; out->b[i].hi[c] = list[i].box_hi[c];
			out->b[i].lin[c] = list[i].linear[c]; out->b[i].ang[c] = list[i].angular[c]; out->b[i].piv[c] = list[i].pivot[c];
		}
	return hipSuccess;
}

// (in the three launches below the list travels only when there is one: count 0 is the MOV = 0 kernel)
template <bool HALF>
static hipError_t launch_obstacle_enforce_t(const Geom& g, const uint8_t* code, int x0, int y0, int z0, int tx, int ty, unsigned wgs, int count,
	const BodyArgs& a, void* vel, void* col, float* alpha, hipStream_t s)
{
	typedef typename Sto<HALF>::S S;
	typedef typename Sto<HALF>::S4 S4;
	const dim3 grid(wgs, 1, 1), block(64, 4, 1);
	if (count) hipLaunchKernelGGL((k_obstacle_enforce<HALF, true>), grid, block, 0, s, g, code, (S*)vel, (S4*)col, alpha, x0, y0, z0, tx, ty, a);
	else hipLaunchKernelGGL((k_obstacle_enforce<HALF, false>), grid, block, 0, s, g, code, (S*)vel, (S4*)col, alpha, x0, y0, z0, tx, ty, NoBodies());
	return hipGetLastError();
}

hipError_t launch_obstacle_enforce(const Geom& g, int half_store, const uint8_t* code, const int lo[3], const int hi[3],
	const fx_obstacle_body* list, int count, void* vel, void* col, float* alpha, hipStream_t s)
{
	if (!whole_grid(g)) return hipErrorNotSupported;
	BodyArgs a;
	const hipError_t e = body_args(g, code, list, count, &a);
	if (e != hipSuccess) return e;
	int x0, y0, tx, ty;
	const long long wgs = obstacle_enforce_tiles(lo, hi, &x0, &y0, &tx, &ty);
	if (wgs <= 0) return hipSuccess;                                          // no solid cell: nothing to launch
	if (wgs > 0x7fffffffLL || hi[0] > g.X || hi[1] > g.Y || hi[2] > g.Zg || lo[0] < 0 || lo[1] < 0 || lo[2] < 0) return hipErrorInvalidValue;
	return half_store ? launch_obstacle_enforce_t<true>(g, code, x0, y0, lo[2], tx, ty, (unsigned)wgs, count, a, vel, col, alpha, s)
	                  : launch_obstacle_enforce_t<false>(g, code, x0, y0, lo[2], tx, ty, (unsigned)wgs, count, a, vel, col, alpha, s);
}

template <bool HALF>
static hipError_t launch_divergence_obs_t(const Geom& g, const void* vel, const uint8_t* code, int count, const BodyArgs& a, float* b,
	int z_begin, int nzp, hipStream_t s)
{
	typedef typename Sto<HALF>::S S;
	const dim3 grid = grid_cells(g, nzp), block(64, 4, 1);
	if (count) hipLaunchKernelGGL((k_divergence_obs<HALF, true>), grid, block, 0, s, g, (const S*)vel, code, b, z_begin, nzp, remap_small(g), a);
	else hipLaunchKernelGGL((k_divergence_obs<HALF, false>), grid, block, 0, s, g, (const S*)vel, code, b, z_begin, nzp, remap_small(g), NoBodies());
	return hipGetLastError();
}

hipError_t launch_divergence_obs(const Geom& g, int half_store, const void* vel, const uint8_t* code, const fx_obstacle_body* list, int count,
	float* b, int z_begin, int z_end, hipStream_t s)
{
	if (!whole_grid(g)) return hipErrorNotSupported;
	BodyArgs a;
	const hipError_t e = body_args(g, code, list, count, &a);
	if (e != hipSuccess) return e;
	if (!code || z_begin < 0 || z_end > g.Zg) return hipErrorInvalidValue;
	if (z_end <= z_begin) return hipSuccess;
	return half_store ? launch_divergence_obs_t<true>(g, vel, code, count, a, b, z_begin, z_end - z_begin, s)
	                  : launch_divergence_obs_t<false>(g, vel, code, count, a, b, z_begin, z_end - z_begin, s);
}

// ---- the bnd family.  code may be null (open walls alone), faces may be 0 (obstacles in a closed box); not both: those are the plain kernels
static inline hipError_t bnd_args(const Geom& g, const uint8_t* code, unsigned faces, int z_begin, int z_end)
{
	if (!whole_grid(g)) return hipErrorNotSupported;
	return open_faces_ok(g, faces) && (code || faces) && z_begin >= 0 && z_end <= g.Zg ? hipSuccess : hipErrorInvalidValue;
}
// the wide sweep.  OBSTACLE_V4 = 0 (lab builds): the scalar kernel on every geometry -- what tests/test_gpu_obstacles.py and
// tests/test_gpu_open_walls.py hold the wide one against
static bool jacobi_bnd_takes_v4(const Geom& g) { return g.Zg > 1 && (g.X & 3) == 0 && FX_KNOB_INT("OBSTACLE_V4", 1) != 0; }

hipError_t launch_jacobi_bnd(const Geom& g, const float* p_in, const float* b, const uint8_t* code, float* p_out, unsigned faces,
	int z_begin, int z_end, hipStream_t s)
{
	const hipError_t e = bnd_args(g, code, faces, z_begin, z_end);
	if (e != hipSuccess) return e;
	const int nzp = z_end - z_begin;
	if (nzp <= 0) return hipSuccess;
	if (jacobi_bnd_takes_v4(g)) {
		const int X4 = g.X >> 2;                         // the block shape of k_jacobi_v4's launch
		const int bx = X4 < 64 ? X4 : 64;
		int by = 256 / bx; if (by < 1) by = 1; if (by > g.Y) by = g.Y;
		const dim3 block(bx, by, 1), grid(((X4 + bx - 1) / bx) * ((g.Y + by - 1) / by) * nzp, 1, 1);
		const auto k = !faces ? k_jacobi_bnd_v4<true, false> : code ? k_jacobi_bnd_v4<true, true> : k_jacobi_bnd_v4<false, true>;
		hipLaunchKernelGGL(k, grid, block, 0, s, g, p_in, b, code, p_out, faces, z_begin, nzp, 1, by);
	} else {
		const auto k = !faces ? k_jacobi_bnd<true, false> : code ? k_jacobi_bnd<true, true> : k_jacobi_bnd<false, true>;
		hipLaunchKernelGGL(k, grid_cells(g, nzp), dim3(64, 4, 1), 0, s, g, p_in, b, code, p_out, faces, z_begin, nzp, 1);
	}
	return hipGetLastError();
}

template <bool HALF>
static hipError_t launch_project_bnd_t(const Geom& g, const SimParams& sp, const void* vel_in, const float* p, const uint8_t* code, int count,
	const BodyArgs& a, void* vel_out, unsigned faces, int z_begin, int nzp, hipStream_t s)
{
	typedef typename Sto<HALF>::S S;
	const dim3 grid = grid_cells(g, nzp), block(64, 4, 1);
	if (count) {
		const auto k = faces ? k_project_bnd<HALF, true, true, true> : k_project_bnd<HALF, true, false, true>;
		hipLaunchKernelGGL(k, grid, block, 0, s, g, sp, (const S*)vel_in, p, code, (S*)vel_out, faces, z_begin, nzp, remap_small(g), a);
	} else {
		const auto k = !faces ? k_project_bnd<HALF, true, false, false> : code ? k_project_bnd<HALF, true, true, false> : k_project_bnd<HALF, false, true, false>;
		hipLaunchKernelGGL(k, grid, block, 0, s, g, sp, (const S*)vel_in, p, code, (S*)vel_out, faces, z_begin, nzp, remap_small(g), NoBodies());
	}
	return hipGetLastError();
}

hipError_t launch_project_bnd(const Geom& g, const SimParams& sp, int half_store, const void* vel_in, const float* p, const uint8_t* code,
	const fx_obstacle_body* list, int count, void* vel_out, unsigned faces, int z_begin, int z_end, hipStream_t s)
{
	hipError_t e = bnd_args(g, code, faces, z_begin, z_end);
	if (e != hipSuccess) return e;
	BodyArgs a;
	e = body_args(g, code, list, count, &a);
	if (e != hipSuccess) return e;
	if (z_end <= z_begin) return hipSuccess;
	return half_store ? launch_project_bnd_t<true>(g, sp, vel_in, p, code, count, a, vel_out, faces, z_begin, z_end - z_begin, s)
	                  : launch_project_bnd_t<false>(g, sp, vel_in, p, code, count, a, vel_out, faces, z_begin, z_end - z_begin, s);
}

}  // namespace fx
