// fx_multigrid.hip -- the geometric multigrid V-cycle of the pressure solve (fx_set_pressure_solver: FX_PRESSURE_MULTIGRID), gfx950.  No
// reference counterpart (the reference's CSProject relaxes with Jacobi sweeps only).  Nothing is shared with fx_sim.hip / fx_obstacle.hip.
//
//   k_mg_smooth            one damped lock-step sweep on a level, scalar: any extent, 2-D and 3-D, 64 x 4 tiles
//   k_mg_smooth_v4         the same sweep, 3-D with X % 4 == 0: k_jacobi_bnd_v4's scheme (16-byte loads of the five rows and of b, the x
//                          neighbours by DPP lane shifts, 12 bytes per cell); bit-identical to the scalar one
//   k_mg_residual_restrict r = fma(6, p, b - S) of eight (2-D: four) fine cells summed into one coarse right-hand side; no fine-size residual
//                          exists anywhere.  One thread = one fine x of a 2 x 2 (y, z) column, the pair sums along x by DPP
//   k_mg_prolong_correct   p += the tri- (bi-)linear prolongation of the coarse correction, in place; the coarse taps come through L1 / L2
//   k_mg_tail              from the first level with <= 4096 cells down, the rest of the cycle in one workgroup in the LDS (those levels are
//                          bound by launch latency): smooth, restrict, recurse, prolong, smooth, through the same device functions as the
//                          launches per level, so the same bits
//
// The arithmetic (include/fluidx_hip.h states it, tests/multigrid_ref.py restates it in numpy), fp32, every operation rounded as written,
// neighbours by clamped index:
//   sweep     J = ((((((L - b) + R) + U) + D) + F) + B) * INV6 (2-D: ((((L - b) + R) + U) + D) * 0.25f)      p' = fmaf(omega, J - p, p)
//   residual  S = (((((L + R) + U) + D) + F) + B)      r = fmaf(6.0f, p, b - S)  (2-D: four neighbours, 4.0f)
//   restrict  b_c = 0.5f * (((r000 + r100) + (r010 + r110)) + ((r001 + r101) + (r011 + r111)))      2-D: (r00 + r10) + (r01 + r11)
//   prolong   per axis: parent j = i >> 1, other o = clamp(j + (i odd ? 1 : -1)), v = fmaf(0.25f, e[o] - e[j], e[j]); x, then y, then z
// A sweep whose input is all +0 (the first one on a coarse level) evaluates the same expressions on constant zeros instead of loads.
// Fields are addressed with 32-bit byte offsets while a level is below 4 GiB (WIDE above), as k_heat.
#include "fx_internal.h"
#include "fx_store.h"

namespace fx {

using namespace sto;

namespace {

const int MG_X = 64, MG_Y = 4;
typedef Cell<false> Ce;

__device__ __forceinline__ float mg_inv6() { return __uint_as_float(0x3e2aaaabu); }

// the sweep's new value of a cell
__device__ __forceinline__ float mg_relax(float p, float b, float L, float R, float U, float D, float F, float B, float omega, bool is3d)
{
	float s = L - b;
	s = s + R;
	s = s + U;
	s = s + D;
	float J;
	if (is3d) {
		s = s + F;
		s = s + B;
		J = s * mg_inv6();
	} else {
		J = s * 0.25f;
	}
	return fmaf(omega, J - p, p);
}

__device__ __forceinline__ float mg_resid(float p, float b, float L, float R, float U, float D, float F, float B, bool is3d)
{
	float S = L + R;
	S = S + U;
	S = S + D;
	if (is3d) {
		S = S + F;
		S = S + B;
		return fmaf(6.0f, p, b - S);
	}
	return fmaf(4.0f, p, b - S);
}

__device__ __forceinline__ float mg_lerp(float ej, float eo) { return fmaf(0.25f, eo - ej, ej); }

// the other coarse index of fine index i along an axis of nc coarse cells
__device__ __forceinline__ int mg_other(int i, int nc) { return min(max((i >> 1) + ((i & 1) ? 1 : -1), 0), nc - 1); }

// workgroup -> (tile x, tile y, plane) of a raster of tiles_x x tiles_y tiles per plane
__device__ __forceinline__ void tile_of(int tiles_x, int tiles_y, int& tx, int& ty, int& z)
{
	int bid = (int)blockIdx.x;
	tx = bid % tiles_x; bid /= tiles_x;
	ty = bid % tiles_y;
	z = bid / tiles_y;
}

}  // namespace

// ---------------------------------------------------------------------------------------------
// the sweep, scalar
// ---------------------------------------------------------------------------------------------
template <bool ZERO, bool WIDE>
__global__ __launch_bounds__(256) void k_mg_smooth(const MgDims d, int is3d, int tiles_x, int tiles_y, const float* __restrict__ e_in,
	const float* __restrict__ b, float* __restrict__ e_out, float omega)
{
	typedef typename Off<WIDE>::T O;
	int tx, ty, z;
	tile_of(tiles_x, tiles_y, tx, ty, z);
	const int x = tx * MG_X + (int)threadIdx.x, y = ty * MG_Y + (int)threadIdx.y;
	if (x >= d.X || y >= d.Y || z >= d.Z) return;
	const O X = (O)d.X, plane = (O)d.X * (O)d.Y;
	const O zrow = (O)z * plane, row = zrow + (O)y * X;
	const O id = row + (O)x;
	const char* pi = reinterpret_cast<const char*>(e_in);
	const float bb = Ce::ld1(reinterpret_cast<const char*>(b), id);
	float c = 0.0f, L = 0.0f, R = 0.0f, U = 0.0f, D = 0.0f, F = 0.0f, B = 0.0f;
	if (!ZERO) {
		const int xl = max(x, 1) - 1, xr = min(x + 1, d.X - 1);
		const int yu = max(y, 1) - 1, yd = min(y + 1, d.Y - 1);
		c = Ce::ld1(pi, id);
		L = Ce::ld1(pi, row + (O)xl); R = Ce::ld1(pi, row + (O)xr);
		U = Ce::ld1(pi, zrow + (O)yu * X + (O)x); D = Ce::ld1(pi, zrow + (O)yd * X + (O)x);
		if (is3d) {
			const int zf = max(z, 1) - 1, zb = min(z + 1, d.Z - 1);
			F = Ce::ld1(pi, (O)zf * plane + (O)y * X + (O)x); B = Ce::ld1(pi, (O)zb * plane + (O)y * X + (O)x);
		}
	}
	Ce::st1(reinterpret_cast<char*>(e_out), id, mg_relax(c, bb, L, R, U, D, F, B, omega, is3d != 0));
}

// ---------------------------------------------------------------------------------------------
// the sweep, 3-D, X % 4 == 0: one thread = four consecutive x.  The adjacent float4 column sits in the adjacent lane (DPP wave_shr:1 /
// wave_shl:1); only a wave's first / last lane inside a row still loads its x neighbour, a row's ends take the clamped replica
// ---------------------------------------------------------------------------------------------
template <bool ZERO, bool WIDE>
__global__ __launch_bounds__(256) void k_mg_smooth_v4(const MgDims d, int tiles_x, int tiles_y, int rows_per_block, const float* __restrict__ e_in,
	const float* __restrict__ b, float* __restrict__ e_out, float omega)
{
	typedef typename Off<WIDE>::T O;
	const int X4 = d.X >> 2;
	const int lane = (int)threadIdx.x;                  // float4 column
	int tx, ty, z;
	tile_of(tiles_x, tiles_y, tx, ty, z);
	const int x4 = tx * (int)blockDim.x + lane;
	const int y = ty * rows_per_block + (int)threadIdx.y;
	if (x4 >= X4 || y >= d.Y || z >= d.Z) return;
	const O X = (O)d.X, plane = (O)d.X * (O)d.Y;
	const O c_off = (O)z * plane + (O)y * X + (O)(4 * x4);
	const float4 bb = *reinterpret_cast<const float4*>(reinterpret_cast<const char*>(b) + c_off * (O)4);
	const float4 zero4 = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
	float4 c = zero4, U = zero4, D = zero4, F = zero4, B = zero4;
	float L = 0.0f, R = 0.0f;
	if (!ZERO) {
		const char* pi = reinterpret_cast<const char*>(e_in);
		const int yu = max(y, 1) - 1, yd = min(y + 1, d.Y - 1);
		const int zf = max(z, 1) - 1, zb = min(z + 1, d.Z - 1);
		c = *reinterpret_cast<const float4*>(pi + c_off * (O)4);
		U = *reinterpret_cast<const float4*>(pi + ((O)z * plane + (O)yu * X + (O)(4 * x4)) * (O)4);
		D = *reinterpret_cast<const float4*>(pi + ((O)z * plane + (O)yd * X + (O)(4 * x4)) * (O)4);
		F = *reinterpret_cast<const float4*>(pi + ((O)zf * plane + (O)y * X + (O)(4 * x4)) * (O)4);
		B = *reinterpret_cast<const float4*>(pi + ((O)zb * plane + (O)y * X + (O)(4 * x4)) * (O)4);
		const int wl = (int)((threadIdx.y * blockDim.x + threadIdx.x) & 63);
		L = __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, c.w), 0x138, 0xf, 0xf, false));
		R = __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, c.x), 0x130, 0xf, 0xf, false));
		if (x4 == 0) L = c.x; else if (wl == 0 || lane == 0) L = Ce::ld1(pi, c_off - (O)1);
		if (x4 == X4 - 1) R = c.w; else if (wl == 63 || lane == (int)blockDim.x - 1) R = Ce::ld1(pi, c_off + (O)4);
	}
	const float pc[4] = { c.x, c.y, c.z, c.w };
	const float pl[4] = { L, c.x, c.y, c.z }, pr[4] = { c.y, c.z, c.w, R };
	const float pu[4] = { U.x, U.y, U.z, U.w }, pd[4] = { D.x, D.y, D.z, D.w };
	const float pf[4] = { F.x, F.y, F.z, F.w }, pb[4] = { B.x, B.y, B.z, B.w };
	const float bv[4] = { bb.x, bb.y, bb.z, bb.w };
	float o[4];
#pragma unroll
	for (int i = 0; i < 4; ++i) o[i] = mg_relax(pc[i], bv[i], pl[i], pr[i], pu[i], pd[i], pf[i], pb[i], omega, true);
	*reinterpret_cast<float4*>(reinterpret_cast<char*>(e_out) + c_off * (O)4) = make_float4(o[0], o[1], o[2], o[3]);
}

// ---------------------------------------------------------------------------------------------
// residual + restriction.  Thread (x, yc, zc) holds the fine cells (x, 2 yc + i, 2 zc + k), i, k = 0, 1 (2-D: k = 0); the fine extents are
// even, so lanes x and x ^ 1 of a pair are both inside or both outside.  The even lane of a pair forms r0ik + r1ik with the odd lane's
// residual (DPP quad_perm [1, 1, 3, 3]) and stores the coarse cell x >> 1
// ---------------------------------------------------------------------------------------------
template <bool WIDE>
__global__ __launch_bounds__(256) void k_mg_residual_restrict(const MgDims d, int is3d, int tiles_x, int tiles_y, const float* __restrict__ p,
	const float* __restrict__ b, float* __restrict__ b_coarse)
{
	typedef typename Off<WIDE>::T O;
	int tx, ty, zc;
	tile_of(tiles_x, tiles_y, tx, ty, zc);
	const int x = tx * MG_X + (int)threadIdx.x, yc = ty * MG_Y + (int)threadIdx.y;
	const int Xc = d.X >> 1, Yc = d.Y >> 1, Zc = is3d ? d.Z >> 1 : 1;
	if (x >= d.X || yc >= Yc || zc >= Zc) return;
	const O X = (O)d.X, plane = (O)d.X * (O)d.Y;
	const char* pp = reinterpret_cast<const char*>(p);
	const char* bp = reinterpret_cast<const char*>(b);
	const int xl = max(x, 1) - 1, xr = min(x + 1, d.X - 1);
	const int nk = is3d ? 2 : 1;
	float r[2][2];                                      // [k][i]
#pragma unroll
	for (int k = 0; k < 2; ++k) {
		if (k >= nk) { r[k][0] = r[k][1] = 0.0f; continue; }
		const int z = is3d ? 2 * zc + k : 0;
		const int zf = max(z, 1) - 1, zb = min(z + 1, d.Z - 1);
#pragma unroll
		for (int i = 0; i < 2; ++i) {
			const int y = 2 * yc + i;
			const int yu = max(y, 1) - 1, yd = min(y + 1, d.Y - 1);
			const O row = (O)z * plane + (O)y * X;
			const float c = Ce::ld1(pp, row + (O)x);
			const float L = Ce::ld1(pp, row + (O)xl), R = Ce::ld1(pp, row + (O)xr);
			const float U = Ce::ld1(pp, (O)z * plane + (O)yu * X + (O)x), D = Ce::ld1(pp, (O)z * plane + (O)yd * X + (O)x);
			float F = 0.0f, B = 0.0f;
			if (is3d) { F = Ce::ld1(pp, (O)zf * plane + (O)y * X + (O)x); B = Ce::ld1(pp, (O)zb * plane + (O)y * X + (O)x); }
			r[k][i] = mg_resid(c, Ce::ld1(bp, row + (O)x), L, R, U, D, F, B, is3d != 0);
		}
	}
	float s[2][2];                                      // r0ik + r1ik, valid in the even lane
#pragma unroll
	for (int k = 0; k < 2; ++k)
#pragma unroll
		for (int i = 0; i < 2; ++i) {
			const float other = __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, r[k][i]), 0xF5, 0xf, 0xf, false));
			s[k][i] = r[k][i] + other;
		}
	if (x & 1) return;
	const O cid = ((O)zc * (O)Yc + (O)yc) * (O)Xc + (O)(x >> 1);
	const float v = is3d ? 0.5f * ((s[0][0] + s[0][1]) + (s[1][0] + s[1][1])) : s[0][0] + s[0][1];
	Ce::st1(reinterpret_cast<char*>(b_coarse), cid, v);
}

// ---------------------------------------------------------------------------------------------
// prolongation + correction, in place
// ---------------------------------------------------------------------------------------------
template <bool WIDE>
__global__ __launch_bounds__(256) void k_mg_prolong_correct(const MgDims d, int is3d, int tiles_x, int tiles_y, float* __restrict__ p,
	const float* __restrict__ e)
{
	typedef typename Off<WIDE>::T O;
	int tx, ty, z;
	tile_of(tiles_x, tiles_y, tx, ty, z);
	const int x = tx * MG_X + (int)threadIdx.x, y = ty * MG_Y + (int)threadIdx.y;
	if (x >= d.X || y >= d.Y || z >= d.Z) return;
	const int Xc = d.X >> 1, Yc = d.Y >> 1, Zc = is3d ? d.Z >> 1 : 1;
	const char* ep = reinterpret_cast<const char*>(e);
	const O jx = (O)(x >> 1), ox = (O)mg_other(x, Xc);
	const O rj = (O)(y >> 1) * (O)Xc, ro = (O)mg_other(y, Yc) * (O)Xc;
	const O cplane = (O)Xc * (O)Yc;
	const O pj = is3d ? (O)(z >> 1) * cplane : (O)0;
	const float xjj = mg_lerp(Ce::ld1(ep, pj + rj + jx), Ce::ld1(ep, pj + rj + ox));       // (z parent, y parent)
	const float xoj = mg_lerp(Ce::ld1(ep, pj + ro + jx), Ce::ld1(ep, pj + ro + ox));       // (z parent, y other)
	float v = mg_lerp(xjj, xoj);
	if (is3d) {
		const O po = (O)mg_other(z, Zc) * cplane;
		const float xjo = mg_lerp(Ce::ld1(ep, po + rj + jx), Ce::ld1(ep, po + rj + ox));   // (z other, y parent)
		const float xoo = mg_lerp(Ce::ld1(ep, po + ro + jx), Ce::ld1(ep, po + ro + ox));
		v = mg_lerp(v, mg_lerp(xjo, xoo));
	}
	const O id = ((O)z * (O)d.Y + (O)y) * (O)d.X + (O)x;
	char* pp = reinterpret_cast<char*>(p);
	Ce::st1(pp, id, Ce::ld1(pp, id) + v);
}

// ---------------------------------------------------------------------------------------------
// the tail: one workgroup, every level from a.first down in the LDS -- a ping-pong partner S shared by all levels (a sweep writes S, then
// copies it back), then correction and right-hand side per level
// ---------------------------------------------------------------------------------------------
namespace {

const int MG_TAIL_THREADS = 1024;

__device__ __forceinline__ void tail_smooth(const MgDims d, bool is3d, float* e, const float* b, float* S, float omega, int sweeps)
{
	const int n = (int)d.cells(), XY = d.X * d.Y;
	for (int k = 0; k < sweeps; ++k) {
		for (int i = (int)threadIdx.x; i < n; i += MG_TAIL_THREADS) {
			const int z = i / XY, rem = i - z * XY, y = rem / d.X, x = rem - y * d.X;
			const int xl = max(x, 1) - 1, xr = min(x + 1, d.X - 1);
			const int yu = max(y, 1) - 1, yd = min(y + 1, d.Y - 1);
			const int zf = max(z, 1) - 1, zb = min(z + 1, d.Z - 1);
			const int row = z * XY + y * d.X;
			float F = 0.0f, B = 0.0f;
			if (is3d) { F = e[zf * XY + y * d.X + x]; B = e[zb * XY + y * d.X + x]; }
			S[i] = mg_relax(e[i], b[i], e[row + xl], e[row + xr], e[z * XY + yu * d.X + x], e[z * XY + yd * d.X + x], F, B, omega, is3d);
		}
		__syncthreads();
		for (int i = (int)threadIdx.x; i < n; i += MG_TAIL_THREADS) e[i] = S[i];
		__syncthreads();
	}
}

__device__ __forceinline__ float tail_resid(const MgDims d, bool is3d, const float* e, const float* b, int x, int y, int z)
{
	const int XY = d.X * d.Y;
	const int xl = max(x, 1) - 1, xr = min(x + 1, d.X - 1);
	const int yu = max(y, 1) - 1, yd = min(y + 1, d.Y - 1);
	const int zf = max(z, 1) - 1, zb = min(z + 1, d.Z - 1);
	const int row = z * XY + y * d.X;
	float F = 0.0f, B = 0.0f;
	if (is3d) { F = e[zf * XY + y * d.X + x]; B = e[zb * XY + y * d.X + x]; }
	return mg_resid(e[row + x], b[row + x], e[row + xl], e[row + xr], e[z * XY + yu * d.X + x], e[z * XY + yd * d.X + x], F, B, is3d);
}

}  // namespace

__global__ __launch_bounds__(MG_TAIL_THREADS) void k_mg_tail(const MgTailArgs a)
{
	extern __shared__ __attribute__((aligned(16))) float mg_lds[];
	const bool is3d = a.is3d != 0;
	float* S = mg_lds;
	// level l's correction, with its right-hand side behind it (offsets summed from the kernel arguments: no indexed private array)
	const auto le = [&](int l) { size_t o = a.lv[a.first].cells(); for (int k = a.first; k < l; ++k) o += 2 * a.lv[k].cells(); return mg_lds + o; };
	const auto lb = [&](int l) { return le(l) + a.lv[l].cells(); };
	const int last = a.levels - 1;
	{
		float* b0 = lb(a.first);
		for (int i = (int)threadIdx.x, n = (int)a.lv[a.first].cells(); i < n; i += MG_TAIL_THREADS) b0[i] = a.b[a.first][i];
	}
	for (int l = a.first; l <= last; ++l) {
		const MgDims d = a.lv[l];
		const int n = (int)d.cells();
		float* el = le(l);
		float* bl = el + n;
		for (int i = (int)threadIdx.x; i < n; i += MG_TAIL_THREADS) el[i] = 0.0f;
		__syncthreads();                                 // the zeros, and the right-hand side the level above (or the load) left
		if (l == last) { tail_smooth(d, is3d, el, bl, S, a.omega, a.coarse); break; }
		tail_smooth(d, is3d, el, bl, S, a.omega, a.pre);
		const MgDims c = a.lv[l + 1];
		const int nc = (int)c.cells(), cXY = c.X * c.Y;
		float* bc = bl + n + nc;                         // the next level's right-hand side, behind its correction
		for (int i = (int)threadIdx.x; i < nc; i += MG_TAIL_THREADS) {
			const int zc = i / cXY, rem = i - zc * cXY, yc = rem / c.X, xc = rem - yc * c.X;
			const int x = 2 * xc, y = 2 * yc, z = is3d ? 2 * zc : 0;
			const float s00 = tail_resid(d, is3d, el, bl, x, y, z) + tail_resid(d, is3d, el, bl, x + 1, y, z);
			const float s10 = tail_resid(d, is3d, el, bl, x, y + 1, z) + tail_resid(d, is3d, el, bl, x + 1, y + 1, z);
			float v = s00 + s10;
			if (is3d) {
				const float s01 = tail_resid(d, is3d, el, bl, x, y, z + 1) + tail_resid(d, is3d, el, bl, x + 1, y, z + 1);
				const float s11 = tail_resid(d, is3d, el, bl, x, y + 1, z + 1) + tail_resid(d, is3d, el, bl, x + 1, y + 1, z + 1);
				v = 0.5f * (v + (s01 + s11));
			}
			bc[i] = v;
		}
	}
	for (int l = last - 1; l >= a.first; --l) {
		const MgDims d = a.lv[l], c = a.lv[l + 1];
		const int n = (int)d.cells(), XY = d.X * d.Y, cXY = c.X * c.Y;
		float* el = le(l);
		float* bl = el + n;
		const float* e = bl + n;                         // the level below's correction
		for (int i = (int)threadIdx.x; i < n; i += MG_TAIL_THREADS) {
			const int z = i / XY, rem = i - z * XY, y = rem / d.X, x = rem - y * d.X;
			const int jx = x >> 1, ox = mg_other(x, c.X);
			const int rj = (y >> 1) * c.X, ro = mg_other(y, c.Y) * c.X;
			const int pj = is3d ? (z >> 1) * cXY : 0;
			const float xjj = mg_lerp(e[pj + rj + jx], e[pj + rj + ox]);
			const float xoj = mg_lerp(e[pj + ro + jx], e[pj + ro + ox]);
			float v = mg_lerp(xjj, xoj);
			if (is3d) {
				const int po = mg_other(z, c.Z) * cXY;
				const float xjo = mg_lerp(e[po + rj + jx], e[po + rj + ox]);
				const float xoo = mg_lerp(e[po + ro + jx], e[po + ro + ox]);
				v = mg_lerp(v, mg_lerp(xjo, xoo));
			}
			el[i] = el[i] + v;
		}
		__syncthreads();
		tail_smooth(d, is3d, el, bl, S, a.omega, a.post);
	}
	__syncthreads();
	for (int l = a.first; l <= last; ++l) {
		const int n = (int)a.lv[l].cells();
		const float* el = le(l);
		const float* bl = el + n;
		float* eo = a.e[l];
		float* bo = a.b[l];
		for (int i = (int)threadIdx.x; i < n; i += MG_TAIL_THREADS) {
			eo[i] = el[i];
			if (l > a.first) bo[i] = bl[i];
		}
	}
}

// ---------------------------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------------------------
static bool mg_dims_ok(const MgDims& d, int is3d) { return d.X > 0 && d.Y > 0 && d.Z > 0 && (is3d || d.Z == 1); }
static bool mg_wide(const MgDims& d) { return d.cells() * 4 >= ((size_t)1 << 32) || lab_wide_offsets(); }      // (WIDE_OFFSETS: fx_internal.h)
static bool mg_halves(const MgDims& d, int is3d) { return !(d.X & 1) && !(d.Y & 1) && (!is3d || !(d.Z & 1)); }

hipError_t launch_mg_smooth(const MgDims& d, int is3d, const float* e_in, const float* b, float* e_out, float omega, hipStream_t s)
{
	if (!mg_dims_ok(d, is3d) || !b || !e_out || e_in == e_out) return hipErrorInvalidValue;
	const bool wide = mg_wide(d), zero = e_in == nullptr;
	if (is3d && (d.X & 3) == 0) {
		const int X4 = d.X >> 2;
		const int bx = X4 < 64 ? X4 : 64;
		int by = 256 / bx; if (by < 1) by = 1; if (by > d.Y) by = d.Y;
		const int tiles_x = (X4 + bx - 1) / bx, tiles_y = (d.Y + by - 1) / by;
		const long long wgs = (long long)tiles_x * tiles_y * d.Z;
		if (wgs > 0x7FFFFFFFll) return hipErrorInvalidValue;
		const auto k = zero ? (wide ? k_mg_smooth_v4<true, true> : k_mg_smooth_v4<true, false>) : (wide ? k_mg_smooth_v4<false, true> : k_mg_smooth_v4<false, false>);
		hipLaunchKernelGGL(k, dim3((unsigned)wgs, 1, 1), dim3(bx, by, 1), 0, s, d, tiles_x, tiles_y, by, e_in, b, e_out, omega);
		return hipGetLastError();
	}
	const int tiles_x = (d.X + MG_X - 1) / MG_X, tiles_y = (d.Y + MG_Y - 1) / MG_Y;
	const long long wgs = (long long)tiles_x * tiles_y * d.Z;
	if (wgs > 0x7FFFFFFFll) return hipErrorInvalidValue;
	const auto k = zero ? (wide ? k_mg_smooth<true, true> : k_mg_smooth<true, false>) : (wide ? k_mg_smooth<false, true> : k_mg_smooth<false, false>);
	hipLaunchKernelGGL(k, dim3((unsigned)wgs, 1, 1), dim3(MG_X, MG_Y, 1), 0, s, d, is3d, tiles_x, tiles_y, e_in, b, e_out, omega);
	return hipGetLastError();
}

hipError_t launch_mg_residual_restrict(const MgDims& fine, int is3d, const float* p, const float* b, float* b_coarse, hipStream_t s)
{
	if (!mg_dims_ok(fine, is3d) || !mg_halves(fine, is3d) || !p || !b || !b_coarse) return hipErrorInvalidValue;
	const int tiles_x = (fine.X + MG_X - 1) / MG_X, tiles_y = ((fine.Y >> 1) + MG_Y - 1) / MG_Y;
	const long long wgs = (long long)tiles_x * tiles_y * (is3d ? fine.Z >> 1 : 1);
	if (wgs > 0x7FFFFFFFll) return hipErrorInvalidValue;
	const auto k = mg_wide(fine) ? k_mg_residual_restrict<true> : k_mg_residual_restrict<false>;
	hipLaunchKernelGGL(k, dim3((unsigned)wgs, 1, 1), dim3(MG_X, MG_Y, 1), 0, s, fine, is3d, tiles_x, tiles_y, p, b, b_coarse);
	return hipGetLastError();
}

hipError_t launch_mg_prolong_correct(const MgDims& fine, int is3d, float* p, const float* e_coarse, hipStream_t s)
{
	if (!mg_dims_ok(fine, is3d) || !mg_halves(fine, is3d) || !p || !e_coarse) return hipErrorInvalidValue;
	const int tiles_x = (fine.X + MG_X - 1) / MG_X, tiles_y = (fine.Y + MG_Y - 1) / MG_Y;
	const long long wgs = (long long)tiles_x * tiles_y * fine.Z;
	if (wgs > 0x7FFFFFFFll) return hipErrorInvalidValue;
	const auto k = mg_wide(fine) ? k_mg_prolong_correct<true> : k_mg_prolong_correct<false>;
	hipLaunchKernelGGL(k, dim3((unsigned)wgs, 1, 1), dim3(MG_X, MG_Y, 1), 0, s, fine, is3d, tiles_x, tiles_y, p, e_coarse);
	return hipGetLastError();
}

hipError_t launch_mg_tail(const MgTailArgs& a, int lds_floats, hipStream_t s)
{
	if (a.first < 1 || a.first >= a.levels || a.levels > kMgMaxLevels || lds_floats <= 0 || (size_t)lds_floats * sizeof(float) > (size_t)kMgTailLdsBytes)
		return hipErrorInvalidValue;
	size_t need = a.lv[a.first].cells();
	for (int l = a.first; l < a.levels; ++l) {
		if (!mg_dims_ok(a.lv[l], a.is3d) || !a.e[l] || !a.b[l] || a.lv[l].cells() > (size_t)kMgTailCells) return hipErrorInvalidValue;
		if (l + 1 < a.levels && (!mg_halves(a.lv[l], a.is3d) || a.lv[l + 1].X != a.lv[l].X >> 1 || a.lv[l + 1].Y != a.lv[l].Y >> 1 ||
			a.lv[l + 1].Z != (a.is3d ? a.lv[l].Z >> 1 : 1))) return hipErrorInvalidValue;
		need += 2 * a.lv[l].cells();
	}
	if (need > (size_t)lds_floats) return hipErrorInvalidValue;
	hipLaunchKernelGGL(k_mg_tail, dim3(1, 1, 1), dim3(MG_TAIL_THREADS, 1, 1), (size_t)lds_floats * sizeof(float), s, a);
	return hipGetLastError();
}

}  // namespace fx
