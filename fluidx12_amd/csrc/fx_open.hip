// fx_open.hip -- open walls (fx_set_open_walls): the inflow pass of the faces of the box through which the smoke leaves, gfx950.  No reference
// counterpart: the reference's six walls are closed.
//
//   k_open_inflow       COLOR *= w: the share of the back-traced sample that lies inside the box, the ghost cells beyond an open face holding clear air
//
// The pressure side of an open face (the Dirichlet ghost p = 0 of the sweeps, the projection without wall damping towards the face) lives with
// the obstacle rule in the boundary-aware kernels of fx_obstacle.hip (k_jacobi_bnd, k_project_bnd); the temperature's ghost at the ambient
// value in k_heat (fx_heat.hip).  tests/open_ref.py restates the rules in numpy, tests/test_gpu_open_walls.py holds the kernels against it bit
// for bit.  fp16 storage widens on load and rounds once (RNE) on store.
// Whole grids only (fx_set_open_walls refuses slab ranks): local plane = global plane.
#include "fx_internal.h"

namespace fx {

namespace {

typedef _Float16 h16;
typedef _Float16 h16x4 __attribute__((ext_vector_type(4)));

// binary16 rounded from the fp32 result in a step of its own (the empty asm keeps the producing multiply and the conversion apart)
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

}  // namespace

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
	if (faces & (FX_WALL_X_LO | FX_WALL_X_HI)) wx = open_wall_trace(Ce::lds(v0, id), dt, x, g.X, faces & FX_WALL_X_LO, faces & FX_WALL_X_HI);
	if (faces & (FX_WALL_Y_LO | FX_WALL_Y_HI)) wy = open_wall_trace(Ce::lds(v0, stride + id), dt, y, g.Y, faces & FX_WALL_Y_LO, faces & FX_WALL_Y_HI);
	if (IS3D && (faces & (FX_WALL_Z_LO | FX_WALL_Z_HI))) wz = open_wall_trace(Ce::lds(v0, (O)2 * stride + id), dt, z, g.Zg, faces & FX_WALL_Z_LO, faces & FX_WALL_Z_HI);
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
static inline bool faces_ok(const Geom& g, unsigned faces) { return !(faces & ~0x3Fu) && !(g.Zg <= 1 && (faces & (FX_WALL_Z_LO | FX_WALL_Z_HI))); }

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
