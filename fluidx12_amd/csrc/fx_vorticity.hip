// fx_vorticity.hip -- vorticity confinement (Fedkiw, Stam, Jensen 2001) of the advected velocity, gfx950.
//
//   k_vorticity   no reference counterpart (the reference's only swirl is the fixed term inside its impulse, CSAdvect.hlsl:63-65)
//
// Index space like k_divergence / k_project: unit cell spacing, neighbour indices clamped to the grid (xl = max(x,1)-1, xr = min(x+1,X-1)).
// With D_a f = 0.5f * (f[upper clamped neighbour along a] - f[lower clamped neighbour along a]):
//   w  = (Dy(uz) - Dz(uy), Dz(ux) - Dx(uz), Dx(uy) - Dy(ux))        m = sqrtf((wx*wx + wy*wy) + wz*wz)      of THIS cell
//   g  = (Dx(m), Dy(m), Dz(m))      l = sqrtf((gx*gx + gy*gy) + gz*gz)      s = (eps * dt) / (l + 1e-6f)
//   u' = u + (g x w) * s            stored in the context's format (fp16: RNE, in a step of its own)
// 2-D grids: every z difference is 0 (wx = wy = gz = 0, m = |wz|) and uz is copied.
// Numerics contract: fp32, every operation separately rounded -- NO fmaf in this file (the build's -ffp-contract=off keeps a*b + c as
// two roundings), sqrtf and / correctly rounded: tests/vorticity_ref.py restates the pass in numpy float32 and the kernel matches it
// bit for bit (tests/test_gpu_vorticity.py).
//
// The cell stencil has radius 2 (m at the six neighbours, each from ITS neighbours), so the pass is out of place: vel_in -> vel_out.
// One launch.  A workgroup of 256 owns a 64 x 16 tile in x-y (wave64 lanes along x) and marches +z through a chunk of planes with
//   su   a ring of three velocity planes, tile + 2-cell rim, 3 components      (48960 B)
//   sm   a ring of three planes of m, tile + 1-cell rim                        (14256 B)
// and w / u of its own four cells of the centre plane in registers.  Per z step it stores the prefetched plane zm + 1 into the ring,
// issues the loads of plane zm + 2 (they land behind the arithmetic), forms w and m of plane zm on the rimmed tile and emits plane
// zm - 1: two barriers a plane.  Walls are index clamps while filling and reading the ring, never ghost cells in memory: ring position
// (i, j) holds the velocity of cell (clamp(x0 - 2 + i), clamp(y0 - 2 + j)), and a rim position outside the grid computes the m of the
// wall cell it clamps to (read by nobody).  Every velocity component is read from HBM once (+ rim and chunk overlap, mostly L2) and
// written once.  Rows of any length: lanes beyond the row clamp their reads and store nothing.
#include "fx_internal.h"
#include "fx_store.h"

namespace fx {

using namespace sto;

namespace {

const int VT_X = 64, VT_Y = 16;                 // tile
const int VU_W = VT_X + 4, VU_H = VT_Y + 4;     // velocity planes of the ring: 2-cell rim
const int VM_W = VT_X + 2, VM_H = VT_Y + 2;     // m planes: 1-cell rim
const int VU_N = VU_W * VU_H;                   // 1360 positions a plane and component
const int VLD = (VU_N + 255) / 256;             // ring positions a thread fills per component (6)
const int VROWS = VT_Y / 4;                     // own cells per thread (rows ty, ty + 4, ...)
const int VRIM = VM_W * VM_H - VT_X * VT_Y;     // rim positions of an m plane (164)

__device__ __forceinline__ int clampi(int v, int hi) { return min(max(v, 0), hi); }

struct Vec3 { float x, y, z; };

}  // namespace

template <bool HALF, bool IS3D>
__global__ __launch_bounds__(256) void k_vorticity(const Geom g, const typename Sto<HALF>::S* __restrict__ vin,
	typename Sto<HALF>::S* __restrict__ vout, float eps, float dt, int zchunk, int tiles_x, int tiles_y)
{
	typedef Sto<HALF> St;
	constexpr int NC = IS3D ? 3 : 2;            // components the stencil reads (2-D: uz is only copied)
	constexpr int NP = IS3D ? 3 : 1;            // planes of the rings
	__shared__ float su[NP][NC][VU_N];
	__shared__ float sm[NP][VM_W * VM_H];

	const int t = (int)threadIdx.x, tx = t & 63, ty = t >> 6;
	int bid = (int)blockIdx.x;
	const int tile_x = bid % tiles_x; bid /= tiles_x;
	const int tile_y = bid % tiles_y;
	const int chunk = bid / tiles_y;
	const int x0 = tile_x * VT_X, y0 = tile_y * VT_Y;
	const int X = g.X, Y = g.Y, Z = g.Zg;
	const int za = chunk * zchunk, zb = min(za + zchunk, Z);
	const size_t plane = g.plane(), stride = g.cells_local();

	// ---- filling the ring: position idx = j * VU_W + i <- cell (clamp(x0 - 2 + i), clamp(y0 - 2 + j)); the same for every plane and component
	uint32_t goff[VLD];
#pragma unroll
	for (int r = 0; r < VLD; ++r) {
		const int idx = min(t + 256 * r, VU_N - 1);
		const int j = idx / VU_W, i = idx - j * VU_W;
		goff[r] = (uint32_t)clampi(y0 - 2 + j, Y - 1) * (uint32_t)X + (uint32_t)clampi(x0 - 2 + i, X - 1);
	}
	float pre[NC][VLD];
	auto issue = [&](int z) {
		const typename St::S* base = vin + (size_t)g.lz(z) * plane;
#pragma unroll
		for (int c = 0; c < NC; ++c)
#pragma unroll
			for (int r = 0; r < VLD; ++r)
				if (t + 256 * r < VU_N) pre[c][r] = St::ld(base + (size_t)c * stride, goff[r]);
	};
	auto commit = [&](int z) {
		const int sl = IS3D ? z % 3 : 0;
#pragma unroll
		for (int c = 0; c < NC; ++c)
#pragma unroll
			for (int r = 0; r < VLD; ++r)
				if (t + 256 * r < VU_N) su[sl][c][t + 256 * r] = pre[c][r];
	};

	// w and m of the cell that m-plane position (i, j) stands for (a position outside the grid: the wall cell it clamps to), plane z
	// -> sm; returns w, and the cell's own velocity in *uc
	auto vort_at = [&](int i, int j, int z, Vec3* uc) -> Vec3 {
		const int cx = clampi(x0 - 1 + i, X - 1), cy = clampi(y0 - 1 + j, Y - 1);
		const int bx = 2 - x0, by = 2 - y0;                                     // cell -> ring position
		const int xl = max(cx, 1) - 1 + bx, xr = min(cx + 1, X - 1) + bx, xc = cx + bx;
		const int yu = (max(cy, 1) - 1 + by) * VU_W, yd = (min(cy + 1, Y - 1) + by) * VU_W, yc = (cy + by) * VU_W;
		const int sc = IS3D ? z % 3 : 0;
		Vec3 w;
		// Dx(uy) - Dy(ux)
		w.z = 0.5f * (su[sc][1][yc + xr] - su[sc][1][yc + xl]) - 0.5f * (su[sc][0][yd + xc] - su[sc][0][yu + xc]);
		float m;
		if constexpr (IS3D) {
			const int sf = (max(z, 1) - 1) % 3, sb = min(z + 1, Z - 1) % 3;
			// Dy(uz) - Dz(uy),  Dz(ux) - Dx(uz)
			w.x = 0.5f * (su[sc][2][yd + xc] - su[sc][2][yu + xc]) - 0.5f * (su[sb][1][yc + xc] - su[sf][1][yc + xc]);
			w.y = 0.5f * (su[sb][0][yc + xc] - su[sf][0][yc + xc]) - 0.5f * (su[sc][2][yc + xr] - su[sc][2][yc + xl]);
			m = sqrtf((w.x * w.x + w.y * w.y) + w.z * w.z);
			uc->z = su[sc][2][yc + xc];
		} else {
			w.x = 0.0f; w.y = 0.0f;
			m = fabsf(w.z);
			uc->z = 0.0f;
		}
		uc->x = su[sc][0][yc + xc]; uc->y = su[sc][1][yc + xc];
		sm[sc][j * VM_W + i] = m;
		return w;
	};

	Vec3 w_cur[VROWS], u_cur[VROWS], w_new[VROWS], u_new[VROWS];
#pragma unroll
	for (int r = 0; r < VROWS; ++r) { w_cur[r] = Vec3{ 0.0f, 0.0f, 0.0f }; u_cur[r] = w_cur[r]; w_new[r] = w_cur[r]; u_new[r] = w_cur[r]; }

	// m of plane z on the rimmed tile: a thread's own four cells (kept), then the 164 rim positions
	auto plane_m = [&](int z) {
#pragma unroll
		for (int r = 0; r < VROWS; ++r) w_new[r] = vort_at(tx + 1, ty + 4 * r + 1, z, &u_new[r]);
		if (t < VRIM) {
			int i, j;
			if (t < VM_W) { i = t; j = 0; }
			else if (t < 2 * VM_W) { i = t - VM_W; j = VM_H - 1; }
			else { const int q = t - 2 * VM_W; i = (q & 1) ? VM_W - 1 : 0; j = 1 + (q >> 1); }
			Vec3 dummy;
			(void)vort_at(i, j, z, &dummy);
		}
	};

	// plane k from w / u of the own cells and the three m planes around it
	const float ed = eps * dt;
	auto emit = [&](int k) {
		const int x = x0 + tx;
		if (x >= X) return;
		const int mb = 1 - x0;                                                  // cell -> m-plane position
		const int xl = max(x, 1) - 1 + mb, xr = min(x + 1, X - 1) + mb, xc = x + mb;
		const int sc = IS3D ? k % 3 : 0;
#pragma unroll
		for (int r = 0; r < VROWS; ++r) {
			const int y = y0 + ty + 4 * r;
			if (y >= Y) continue;
			const int my = 1 - y0;
			const int yu = (max(y, 1) - 1 + my) * VM_W, yd = (min(y + 1, Y - 1) + my) * VM_W, yc = (y + my) * VM_W;
			const float gx = 0.5f * (sm[sc][yc + xr] - sm[sc][yc + xl]);
			const float gy = 0.5f * (sm[sc][yd + xc] - sm[sc][yu + xc]);
			float gz = 0.0f;
			if constexpr (IS3D) gz = 0.5f * (sm[min(k + 1, Z - 1) % 3][yc + xc] - sm[(max(k, 1) - 1) % 3][yc + xc]);
			// 2-D: the +0 stays a register value.  As a constant it leaves Fy = +0 - gx * wz, which the backend folds into the multiply as
			// -(gx * wz) * s: -0 where gx * wz is +0 and the expression as written gives +0 (a -0 velocity then stays -0 instead of
			// becoming +0; tests/test_gpu_store_edges.py found it)
			else asm("" : "+v"(gz));
			const float l = sqrtf((gx * gx + gy * gy) + gz * gz);
			const float s = ed / (l + 1e-6f);
			const Vec3 w = w_cur[r], u = u_cur[r];
			const float Fx = gy * w.z - gz * w.y, Fy = gz * w.x - gx * w.z, Fz = gx * w.y - gy * w.x;
			const size_t id = (size_t)g.lz(k) * plane + (size_t)y * X + x;
			St::st(vout, id, u.x + Fx * s);
			St::st(vout + stride, id, u.y + Fy * s);
			if constexpr (IS3D) St::st(vout + 2 * stride, id, u.z + Fz * s);
			else vout[2 * stride + id] = vin[2 * stride + id];                  // 2-D: uz comes back unchanged
		}
	};

	if constexpr (!IS3D) {
		issue(0); commit(0);
		__syncthreads();
		plane_m(0);
#pragma unroll
		for (int r = 0; r < VROWS; ++r) { w_cur[r] = w_new[r]; u_cur[r] = u_new[r]; }
		__syncthreads();
		emit(0);
		return;
	}

	// planes whose m this chunk needs: zlo .. min(zb, Z - 1); m of plane zm reads the velocity planes zm - 1 .. zm + 1 (clamped)
	const int zlo = max(za - 1, 0);
	if (zlo >= 1) { issue(zlo - 1); commit(zlo - 1); }
	issue(zlo); commit(zlo);
	if (zlo + 1 <= Z - 1) issue(zlo + 1);
	for (int zm = zlo; zm <= zb; ++zm) {
		// (no barrier here: the slot plane zm + 1 goes to held plane zm - 2, last read by plane_m(zm - 1) in front of the previous
		// step's second barrier; emit reads sm and registers only)
		if (zm + 1 <= Z - 1) commit(zm + 1);
		if (zm + 2 <= Z - 1 && zm + 1 <= zb) issue(zm + 2);
		__syncthreads();                    // the ring holds zm - 1 .. zm + 1; the previous step's emit has read sm[(zm - 3) % 3]
		if (zm <= Z - 1) plane_m(zm);
		__syncthreads();                    // m of plane zm is complete
		if (zm - 1 >= za) emit(zm - 1);
#pragma unroll
		for (int r = 0; r < VROWS; ++r) { w_cur[r] = w_new[r]; u_cur[r] = u_new[r]; }
	}
}

hipError_t launch_confine_vorticity(const Geom& g, int half_store, const void* vel_in, void* vel_out, float eps, float dt, hipStream_t s)
{
	if (!whole_grid(g)) return hipErrorNotSupported;                            // a slab would need two planes across each face
	const int tiles_x = (g.X + VT_X - 1) / VT_X, tiles_y = (g.Y + VT_Y - 1) / VT_Y;
	const long long tiles = (long long)tiles_x * tiles_y;
	const bool is3d = g.Zg > 1;
	// z chunks: enough workgroups for two rounds of the 2 x 256 resident ones, at least 8 planes each (a chunk re-reads 3 planes)
	int zchunk = 1, nchunks = 1;
	if (is3d) {
		const long long want = std::max<long long>(1, 1024 / tiles);
		zchunk = (int)std::max<long long>(8, (g.Zg + want - 1) / want);
		if (const char* k = FX_KNOB("VORT_ZCHUNK")) { const int v = atoi(k); if (v > 0) zchunk = v; }
		nchunks = (g.Zg + zchunk - 1) / zchunk;
	}
	if (tiles * nchunks > 0x7fffffffLL) return hipErrorInvalidValue;
	const dim3 grid((unsigned)(tiles * nchunks), 1, 1), block(256, 1, 1);
	if (is3d) {
		if (half_store) hipLaunchKernelGGL((k_vorticity<true, true>), grid, block, 0, s, g, (const h16*)vel_in, (h16*)vel_out, eps, dt, zchunk, tiles_x, tiles_y);
		else hipLaunchKernelGGL((k_vorticity<false, true>), grid, block, 0, s, g, (const float*)vel_in, (float*)vel_out, eps, dt, zchunk, tiles_x, tiles_y);
	} else {
		if (half_store) hipLaunchKernelGGL((k_vorticity<true, false>), grid, block, 0, s, g, (const h16*)vel_in, (h16*)vel_out, eps, dt, zchunk, tiles_x, tiles_y);
		else hipLaunchKernelGGL((k_vorticity<false, false>), grid, block, 0, s, g, (const float*)vel_in, (float*)vel_out, eps, dt, zchunk, tiles_x, tiles_y);
	}
	return hipGetLastError();
}

}  // namespace fx
