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
#include "fx_store.h"

namespace fx {

using namespace sto;

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
	if (faces & (FX_WALL_X_LO | FX_WALL_X_HI)) wx = open_wall_trace(Ce::ld1(v0, id), dt, x, g.X, faces & FX_WALL_X_LO, faces & FX_WALL_X_HI);
	if (faces & (FX_WALL_Y_LO | FX_WALL_Y_HI)) wy = open_wall_trace(Ce::ld1(v0, stride + id), dt, y, g.Y, faces & FX_WALL_Y_LO, faces & FX_WALL_Y_HI);
	if (IS3D && (faces & (FX_WALL_Z_LO | FX_WALL_Z_HI))) wz = open_wall_trace(Ce::ld1(v0, (O)2 * stride + id), dt, z, g.Zg, faces & FX_WALL_Z_LO, faces & FX_WALL_Z_HI);
	float w = wx * wy;
	if (IS3D) w = w * wz;
	if (w == 1.0f) return;                                      // the texel times one: its own bits
	char* co = static_cast<char*>(col);
	const float4 t = Ce::ld4(co, id);
	const float c[4] = { t.x * w, t.y * w, t.z * w, t.w * w };
	const float stored_alpha = Ce::st4(co, id, c);
	if (alpha) *reinterpret_cast<float*>(reinterpret_cast<char*>(alpha) + id * (O)4) = stored_alpha;
}

// ---------------------------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------------------------
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
	if (!vel0 || !col || !open_faces_ok(g, faces)) return hipErrorInvalidValue;
	if (!faces) return hipSuccess;
	const int tx = (g.X + kOpenTileX - 1) / kOpenTileX, ty = (g.Y + kOpenTileY - 1) / kOpenTileY;
	const long long wgs = (long long)tx * ty * g.Zg;
	if (wgs <= 0 || wgs > 0x7fffffffLL) return hipErrorInvalidValue;
	const dim3 grid((unsigned)wgs, 1, 1), block(kOpenTileX, kOpenTileY, 1);
	const bool wide = colour_wants_wide_offsets(g);
	const bool is3d = g.Zg > 1;
	if (half_store) return is3d ? launch_open_inflow_t<true, true>(wide, grid, block, s, g, vel0, col, alpha, faces, dt, tx, ty)
	                            : launch_open_inflow_t<true, false>(wide, grid, block, s, g, vel0, col, alpha, faces, dt, tx, ty);
	return is3d ? launch_open_inflow_t<false, true>(wide, grid, block, s, g, vel0, col, alpha, faces, dt, tx, ty)
	            : launch_open_inflow_t<false, false>(wide, grid, block, s, g, vel0, col, alpha, faces, dt, tx, ty);
}

}  // namespace fx
