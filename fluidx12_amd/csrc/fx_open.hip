// fx_open.hip -- open walls (fx_set_open_walls): faces of the box through which the smoke leaves, gfx950.  No reference counterpart: the
// reference's six walls are closed (the clamped neighbour indices of its projection shaders and the wall damping of its projection).
//
//   k_jacobi_open(_v4)  one lock-step sweep of k_jacobi_obs with  q(n) = beyond an open face ? +0 : S(n) ? p(c) : p(n)   (a Dirichlet ghost p = 0)
//   k_project_open      k_project_obs with the same q, and no wall damping of axis a towards an open face of a
//   k_open_inflow       COLOR *= w: the share of the back-traced sample that lies inside the box, the ghost cells beyond an open face holding clear air
//
// "Beyond an open face" = a stencil neighbour whose unclamped index is -1 or N on an axis whose face there is open (FX_WALL_*: the code
// byte's bit order x-, x+, y-, y+, z-, z+).  The divergence is unchanged: its clamped neighbour is the zero-gradient velocity ghost already.
// The open rule costs no bytes: it replaces the clamped replica of a cell by +0 at the ends of a row and in the rows / planes on a face, which
// are then not loaded at all.  The sweeps and the projection are templated on whether a code volume (fx_obstacle.hip) is present: open walls
// without obstacles read no code byte (12 bytes per cell and sweep; 13 with).  With faces = 0 each kernel is, operation for operation,
// its obstacle counterpart (tests/open_ref.py restates the rules in numpy, tests/test_gpu_open_walls.py holds the kernels against it bit for
// bit).  fp32 arithmetic in the plain kernels' association order; fp16 storage widens on load and rounds once (RNE) on store.
// Whole grids only (fx_set_open_walls refuses slab ranks): local plane = global plane.
#include "fx_internal.h"

namespace fx {

namespace {

typedef _Float16 h16;
typedef _Float16 h16x4 __attribute__((ext_vector_type(4)));

enum { OB_XM = 1, OB_XP = 2, OB_YM = 4, OB_YP = 8, OB_ZM = 16, OB_ZP = 32, OB_SELF = 64 };      // fx_obstacle.hip's code byte; FX_WALL_* = bits 0..5

// velocity storage (Sto of fx_obstacle.hip, restated): fp32, or binary16 rounded from the fp32 result in a step of its own
template <bool HALF> struct Sto;
template <> struct Sto<false> {
	typedef float S;
	static __device__ __forceinline__ float ld(const S* p, size_t i) { return p[i]; }
	static __device__ __forceinline__ void st(S* p, size_t i, float v) { p[i] = v; }
};
template <> struct Sto<true> {
	typedef h16 S;
	static __device__ __forceinline__ float ld(const S* p, size_t i) { return (float)p[i]; }
	static __device__ __forceinline__ void st(S* p, size_t i, float v) { asm("" : "+v"(v)); p[i] = (h16)v; }
};

__device__ __forceinline__ h16 to_h16(float v) { asm("" : "+v"(v)); return (h16)v; }

// the inflow pass addresses its fields as k_heat does: 32-bit byte offsets from uniform bases while the colour field is under 4 GiB
template <bool WIDE> struct Off { typedef uint32_t T; };
template <> struct Off<true> { typedef size_t T; };

template <bool HALF> struct Cell;
template <> struct Cell<false> {
	template <typename O> static __device__ __forceinline__ float lds(const char* b, O cell) { return *reinterpret_cast<const float*>(b + cell * (O)4); }
	template <typename O> static __device__ __forceinline__ float4 ldv(const char* b, O cell) { return *reinterpret_cast<const float4*>(b + cell * (O)16); }
	// stores the texel, returns the alpha a later load of it yields
	template <typename O> static __device__ __forceinline__ float stv(char* b, O cell, const float (&c)[4])
	{
		*reinterpret_cast<float4*>(b + cell * (O)16) = make_float4(c[0], c[1], c[2], c[3]);
		return c[3];
	}
};
template <> struct Cell<true> {
	template <typename O> static __device__ __forceinline__ float lds(const char* b, O cell) { return (float)*reinterpret_cast<const h16*>(b + cell * (O)2); }
	template <typename O> static __device__ __forceinline__ float4 ldv(const char* b, O cell)
	{
		const h16x4 h = *reinterpret_cast<const h16x4*>(b + cell * (O)8);
		return make_float4((float)h.x, (float)h.y, (float)h.z, (float)h.w);
	}
	template <typename O> static __device__ __forceinline__ float stv(char* b, O cell, const float (&c)[4])
	{
		h16x4 h;
		h.x = to_h16(c[0]); h.y = to_h16(c[1]); h.z = to_h16(c[2]); h.w = to_h16(c[3]);
		*reinterpret_cast<h16x4*>(b + cell * (O)8) = h;
		return (float)h.w;
	}
};

// workgroup -> tile, the mapping of the plain kernels (tile_of of fx_obstacle.hip, restated).  Speed only.
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

}  // namespace

// ---------------------------------------------------------------------------------------------
// Jacobi sweep, scalar: any extent, 2-D / 3-D
//   x = ((((((qL - b) + qR) + qU) + qD) + qF) + qB) * (1/6)     2-D: ((((qL - b) + qR) + qU) + qD) * 1/4
// ---------------------------------------------------------------------------------------------
template <bool CODE>
__global__ __launch_bounds__(256) void k_jacobi_open(const Geom g, const float* __restrict__ p_in, const float* __restrict__ b,
	const uint8_t* __restrict__ code, float* __restrict__ p_out, unsigned faces, int z_begin, int nzp, int remap)
{
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
// Jacobi sweep, 3-D, X % 4 == 0: k_jacobi_obs_v4's scheme (one thread = 4 consecutive x: 16-byte loads of the five p rows and of b, a 16-byte
// store, the x neighbours of the row's ends through DPP lane shifts; with CODE one 4-byte load for the four cells' codes).  The clamped
// replica becomes +0 at x4 == 0 / X4 - 1 and in the rows and planes on an open face, whose row beyond is not loaded.  A cell on a face is
// its own clamped neighbour there, so its code bit for that side is its own solid bit: the select behind the +0 only ever changes a solid
// cell, whose result is 0 whatever it summed.  Bit-identical to k_jacobi_open.
// ---------------------------------------------------------------------------------------------
template <bool CODE>
__global__ __launch_bounds__(256) void k_jacobi_open_v4(const Geom g, const float* __restrict__ p_in, const float* __restrict__ b,
	const uint8_t* __restrict__ code, float* __restrict__ p_out, unsigned faces, int z_begin, int nzp, int remap, int rows_per_block)
{
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
template <bool HALF, bool CODE>
__global__ __launch_bounds__(256) void k_project_open(const Geom g, const SimParams sp,
	const typename Sto<HALF>::S* __restrict__ vel_in, const float* __restrict__ p, const uint8_t* __restrict__ code,
	typename Sto<HALF>::S* __restrict__ vel_out, unsigned faces, int z_begin, int nzp, int remap)
{
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
	float u[3] = { St::ld(vel_in, id), St::ld(vel_in, stride + id), St::ld(vel_in, 2 * stride + id) };
	const float c = p[id];
	const float L = p[zrow + (size_t)y * g.X + xl], R = p[zrow + (size_t)y * g.X + xr];
	const float U = p[zrow + (size_t)yu * g.X + x], D = p[zrow + (size_t)yd * g.X + x];
	float grad[3];
	grad[0] = -((o & OB_XM) ? 0.0f : (k & OB_XM) ? c : L) + ((o & OB_XP) ? 0.0f : (k & OB_XP) ? c : R);
	grad[1] = -((o & OB_YM) ? 0.0f : (k & OB_YM) ? c : U) + ((o & OB_YP) ? 0.0f : (k & OB_YP) ? c : D);
	grad[2] = 0.0f;
	float kd = 0.5f;
	if (sp.is3d) {
		const int zf = max(z, 1) - 1, zb = min(z + 1, g.Zg - 1);
		const float F = p[(size_t)g.lz(zf) * plane + (size_t)y * g.X + x], B = p[(size_t)g.lz(zb) * plane + (size_t)y * g.X + x];
		grad[2] = -((o & OB_ZM) ? 0.0f : (k & OB_ZM) ? c : F) + ((o & OB_ZP) ? 0.0f : (k & OB_ZP) ? c : B);
		kd = __uint_as_float(0x3f855556u);                                 // 0.5f / 0.48f, as k_project
		u[2] = fmaf(-grad[2], kd, u[2]);
	}
	u[0] = fmaf(-grad[0], kd, u[0]);
	u[1] = fmaf(-grad[1], kd, u[1]);
	// free slip against a resting solid: no flow along an axis on which a neighbour is solid (the z bits are 0 on 2-D grids)
	if (k & (OB_XM | OB_XP)) u[0] = 0.0f;
	if (k & (OB_YM | OB_YP)) u[1] = 0.0f;
	if (k & (OB_ZM | OB_ZP)) u[2] = 0.0f;
	const int cell[3] = { x, y, z };
	const float dims[3] = { (float)g.X, (float)g.Y, (float)g.Zg };
#pragma unroll
	for (int a = 0; a < 3; ++a) {                                          // the wall damping of k_project, except towards an open face
		float pos = ((float)cell[a] + 0.5f) / dims[a];
		if (sp.is3d || a < 2) pos = fmaf(pos, 2.0f, -1.0f);
		float f = (-fabsf(pos) + 0.970000029f) * 33.3333359f;
		f = fminf(fmaxf(f, -1.0f), 1.0f);
		const bool open = (pos < 0.0f && ((faces >> (2 * a)) & 1u)) || (pos > 0.0f && ((faces >> (2 * a + 1)) & 1u));
		const float w = (0.0f < u[a] * pos && !open) ? f : 1.0f;
		St::st(vel_out, a * stride + id, (k & OB_SELF) ? 0.0f : u[a] * w);
	}
}

// ---------------------------------------------------------------------------------------------
// inflow: 64 x 4 x 1 tiles over the grid, one wave a row.  Only the velocity components of axes with an open face are read; a cell whose
// trace stays inside (w == 1) reads and writes no colour.
// ---------------------------------------------------------------------------------------------
template <bool HALF, bool IS3D, bool WIDE>
__global__ __launch_bounds__(256) void k_open_inflow(const Geom g, const void* __restrict__ vel0, void* __restrict__ col, float* __restrict__ alpha,
	unsigned faces, float dt, int tiles_x, int tiles_y)
{
	typedef Cell<HALF> Ce;
	typedef typename Off<WIDE>::T O;
	int bid = (int)blockIdx.x;
	const int x = (bid % tiles_x) * kOpenTileX + (int)threadIdx.x; bid /= tiles_x;
	const int y = (bid % tiles_y) * kOpenTileY + (int)threadIdx.y, z = bid / tiles_y;
	if (x >= g.X || y >= g.Y) return;
	const O plane = (O)g.X * (O)g.Y;
	const O stride = plane * (O)g.Zg;                           // cells between velocity component planes (a whole grid: no halo)
	const O id = (O)z * plane + (O)y * (O)g.X + (O)x;
	const char* v0 = static_cast<const char*>(vel0);
	float wx = 1.0f, wy = 1.0f, wz = 1.0f;
	if (faces & (OB_XM | OB_XP)) wx = open_wall_trace(Ce::lds(v0, id), dt, x, g.X, faces & OB_XM, faces & OB_XP);
	if (faces & (OB_YM | OB_YP)) wy = open_wall_trace(Ce::lds(v0, stride + id), dt, y, g.Y, faces & OB_YM, faces & OB_YP);
	if (IS3D && (faces & (OB_ZM | OB_ZP))) wz = open_wall_trace(Ce::lds(v0, (O)2 * stride + id), dt, z, g.Zg, faces & OB_ZM, faces & OB_ZP);
	float w = wx * wy;
	if (IS3D) w = w * wz;
	if (w == 1.0f) return;                                      // the texel times one: its own bits
	char* co = static_cast<char*>(col);
	const float4 t = Ce::ldv(co, id);
	const float c[4] = { t.x * w, t.y * w, t.z * w, t.w * w };
	const float stored_alpha = Ce::stv(co, id, c);
	if (alpha) *reinterpret_cast<float*>(reinterpret_cast<char*>(alpha) + id * (O)4) = stored_alpha;
}

// ---------------------------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------------------------
static inline bool whole_grid(const Geom& g) { return g.nz == g.Zg && g.H == 0; }
static inline dim3 grid_cells(const Geom& g, int nzp) { return dim3(((g.X + 63) / 64) * ((g.Y + 3) / 4) * nzp, 1, 1); }
// (fx_obstacle.hip remap_small: divergence and projection take the contiguous-eighth order on the small 3-D grids that live in L2)
static inline int remap_small(const Geom& g) { return g.Zg > 1 && g.plane() <= 32768 && g.cells_local() < (size_t)6 << 20 ? 1 : 0; }
static inline bool faces_ok(const Geom& g, unsigned faces) { return !(faces & ~0x3Fu) && !(g.Zg <= 1 && (faces & (OB_ZM | OB_ZP))); }

bool jacobi_open_takes_v4(const Geom& g) { return g.Zg > 1 && (g.X & 3) == 0; }

hipError_t launch_jacobi_open(const Geom& g, const float* p_in, const float* b, const uint8_t* code, float* p_out, unsigned faces,
	int z_begin, int z_end, hipStream_t s)
{
	if (!whole_grid(g)) return hipErrorNotSupported;
	if (!faces_ok(g, faces) || z_begin < 0 || z_end > g.Zg) return hipErrorInvalidValue;
	const int nzp = z_end - z_begin;
	if (nzp <= 0) return hipSuccess;
	if (jacobi_open_takes_v4(g)) {
		const int X4 = g.X >> 2;                         // the block shape of k_jacobi_v4's launch
		const int bx = X4 < 64 ? X4 : 64;
		int by = 256 / bx; if (by < 1) by = 1; if (by > g.Y) by = g.Y;
		const dim3 block(bx, by, 1), grid(((X4 + bx - 1) / bx) * ((g.Y + by - 1) / by) * nzp, 1, 1);
		if (code) hipLaunchKernelGGL(k_jacobi_open_v4<true>, grid, block, 0, s, g, p_in, b, code, p_out, faces, z_begin, nzp, 1, by);
		else hipLaunchKernelGGL(k_jacobi_open_v4<false>, grid, block, 0, s, g, p_in, b, code, p_out, faces, z_begin, nzp, 1, by);
	} else {
		if (code) hipLaunchKernelGGL(k_jacobi_open<true>, grid_cells(g, nzp), dim3(64, 4, 1), 0, s, g, p_in, b, code, p_out, faces, z_begin, nzp, 1);
		else hipLaunchKernelGGL(k_jacobi_open<false>, grid_cells(g, nzp), dim3(64, 4, 1), 0, s, g, p_in, b, code, p_out, faces, z_begin, nzp, 1);
	}
	return hipGetLastError();
}

template <bool HALF>
static hipError_t launch_project_open_t(const Geom& g, const SimParams& sp, const void* vel_in, const float* p, const uint8_t* code, void* vel_out,
	unsigned faces, int z_begin, int nzp, hipStream_t s)
{
	typedef typename Sto<HALF>::S S;
	const dim3 grid = grid_cells(g, nzp), block(64, 4, 1);
	if (code) hipLaunchKernelGGL((k_project_open<HALF, true>), grid, block, 0, s, g, sp, (const S*)vel_in, p, code, (S*)vel_out, faces, z_begin, nzp, remap_small(g));
	else hipLaunchKernelGGL((k_project_open<HALF, false>), grid, block, 0, s, g, sp, (const S*)vel_in, p, code, (S*)vel_out, faces, z_begin, nzp, remap_small(g));
	return hipGetLastError();
}

hipError_t launch_project_open(const Geom& g, const SimParams& sp, int half_store, const void* vel_in, const float* p, const uint8_t* code,
	void* vel_out, unsigned faces, int z_begin, int z_end, hipStream_t s)
{
	if (!whole_grid(g)) return hipErrorNotSupported;
	if (!faces_ok(g, faces) || z_begin < 0 || z_end > g.Zg) return hipErrorInvalidValue;
	if (z_end <= z_begin) return hipSuccess;
	return half_store ? launch_project_open_t<true>(g, sp, vel_in, p, code, vel_out, faces, z_begin, z_end - z_begin, s)
	                  : launch_project_open_t<false>(g, sp, vel_in, p, code, vel_out, faces, z_begin, z_end - z_begin, s);
}

template <bool HALF, bool IS3D>
static hipError_t launch_open_inflow_t(bool wide, dim3 grid, dim3 block, hipStream_t s, const Geom& g, const void* vel0, void* col, float* alpha,
	unsigned faces, float dt, int tx, int ty)
{
	if (wide) hipLaunchKernelGGL((k_open_inflow<HALF, IS3D, true>), grid, block, 0, s, g, vel0, col, alpha, faces, dt, tx, ty);
	else hipLaunchKernelGGL((k_open_inflow<HALF, IS3D, false>), grid, block, 0, s, g, vel0, col, alpha, faces, dt, tx, ty);
	return hipGetLastError();
}

hipError_t launch_open_inflow(const Geom& g, int half_store, const void* vel0, void* col, float* alpha, unsigned faces, float dt, hipStream_t s)
{
	if (!whole_grid(g)) return hipErrorNotSupported;
	if (!vel0 || !col || !faces_ok(g, faces)) return hipErrorInvalidValue;
	if (!faces) return hipSuccess;
	const int tx = (g.X + kOpenTileX - 1) / kOpenTileX, ty = (g.Y + kOpenTileY - 1) / kOpenTileY;
	const long long wgs = (long long)tx * ty * g.Zg;
	if (wgs <= 0 || wgs > 0x7fffffffLL) return hipErrorInvalidValue;
	const dim3 grid((unsigned)wgs, 1, 1), block(kOpenTileX, kOpenTileY, 1);
	const bool wide = g.cells_local() * 16 >= ((size_t)1 << 32);                // the colour field, the largest one, in fp32
	const bool is3d = g.Zg > 1;
	if (half_store) return is3d ? launch_open_inflow_t<true, true>(wide, grid, block, s, g, vel0, col, alpha, faces, dt, tx, ty)
	                            : launch_open_inflow_t<true, false>(wide, grid, block, s, g, vel0, col, alpha, faces, dt, tx, ty);
	return is3d ? launch_open_inflow_t<false, true>(wide, grid, block, s, g, vel0, col, alpha, faces, dt, tx, ty)
	            : launch_open_inflow_t<false, false>(wide, grid, block, s, g, vel0, col, alpha, faces, dt, tx, ty);
}

}  // namespace fx
