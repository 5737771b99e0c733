// fx_voxelize.hip -- the solid voxeliser of fx_set_obstacle_meshes, gfx950: closed triangle meshes -> the 0 / 1 byte mask that
// launch_obstacle_codes (fx_obstacle.hip) turns into the code volume.  No reference counterpart (the reference has no solids).
//
//   k_vox_scatter      one wave per triangle: its covered (y, z) columns each toggle one bit of the bitmap [Z][Y][X / 32 + 1] at the cell the
//                      triangle's plane crosses the column in; triangles whose clipped box is larger than kVoxBig columns go onto a list
//   k_vox_scatter_big  the list: one workgroup per (triangle, 16 x 16 patch of the grid's columns), so that a wall-sized triangle is spread
//                      over the chip instead of being walked by one wave
//   k_vox_fill         one wave per row of X cells: the prefix XOR of the row's toggles is the solid set (a cell is inside where the toggles
//                      at or below it are odd in number); written, or ORed for the second mesh on, as bytes; clears the words it read
//
// The rule (include/fluidx_hip.h) is exact: one fp32 rounding per operation of the transform and one of the quantisation to 1 / 256 of a cell,
// int64 from there.  A column's sample point is its cell centre shifted by (-eps^2, +eps) in (y, z), which is what the tie rule of the edge
// functions says: an edge or vertex shared by two triangles counts for exactly one of them, whatever their order or winding.  XOR commutes, so
// the atomic scatter gives the same bits in every order.
// |q| <= 2^18, so the edge functions stay below 2^41, the projected area A and the normal's components below 2^40 and T below 2^61.
#include "fx_internal.h"

namespace fx {

namespace {

enum { kVoxBig = 1024 };             // columns of a clipped box one wave still walks itself (16 rounds of 64)
constexpr float kVoxClamp = 262144.0f;

struct VoxTri {
	int ax, ay, az, bx, by, bz, cx, cy, cz;
	long long A, ny, nz;             // A > 0: the x component of the normal (b - a) x (c - a), and its y and z components
	int j0, j1, k0, k1;              // the columns whose centre lies in the triangle's (y, z) box, clipped to the grid; inclusive
};

// one position, transformed and quantised; false: a transformed coordinate is not finite
__device__ __forceinline__ bool vox_vertex(const Geom& g, const VoxMesh& m, uint32_t v, int& qx, int& qy, int& qz)
{
	const float x = m.pos[3 * (size_t)v], y = m.pos[3 * (size_t)v + 1], z = m.pos[3 * (size_t)v + 2];
	float p[3] = { x, y, z };
	if (m.xf) {
		for (int a = 0; a < 3; ++a) {
			const float* r = m.xf + 4 * a;
			p[a] = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(r[0], x), __fmul_rn(r[1], y)), __fmul_rn(r[2], z)), r[3]);
		}
	}
	const float n[3] = { (float)(256 * g.X), (float)(256 * g.Y), (float)(256 * g.Zg) };
	int q[3];
	bool ok = true;
	for (int a = 0; a < 3; ++a) {
		ok = ok && isfinite(p[a]);
		const float t = fminf(fmaxf(__fmul_rn(p[a], n[a]), -kVoxClamp), kVoxClamp);
		q[a] = (int)rintf(t);
	}
	qx = q[0]; qy = q[1]; qz = q[2];
	return ok;
}

enum { VOX_OK = 0, VOX_SKIPPED = 1, VOX_NOTHING = 2 };

__device__ __forceinline__ int vox_triangle(const Geom& g, const VoxMesh& m, uint32_t t, VoxTri& o)
{
	const uint32_t ia = m.idx[3 * (size_t)t], ib = m.idx[3 * (size_t)t + 1], ic = m.idx[3 * (size_t)t + 2];
	if (ia >= m.nv || ib >= m.nv || ic >= m.nv) return VOX_SKIPPED;
	bool ok = vox_vertex(g, m, ia, o.ax, o.ay, o.az);
	ok = vox_vertex(g, m, ib, o.bx, o.by, o.bz) && ok;
	ok = vox_vertex(g, m, ic, o.cx, o.cy, o.cz) && ok;
	if (!ok) return VOX_SKIPPED;
	long long A = (long long)(o.by - o.ay) * (o.cz - o.az) - (long long)(o.bz - o.az) * (o.cy - o.ay);
	if (A == 0) return VOX_NOTHING;                                   // edge-on: covers no column
	if (A < 0) {
		int s;
		s = o.bx; o.bx = o.cx; o.cx = s;
		s = o.by; o.by = o.cy; o.cy = s;
		s = o.bz; o.bz = o.cz; o.cz = s;
		A = -A;
	}
	o.A = A;
	const long long e1x = o.bx - o.ax, e1y = o.by - o.ay, e1z = o.bz - o.az, e2x = o.cx - o.ax, e2y = o.cy - o.ay, e2z = o.cz - o.az;
	o.ny = e1z * e2x - e1x * e2z;
	o.nz = e1x * e2y - e1y * e2x;
	// centre 256 j + 128 inside [min, max]: j from ceil((min - 128) / 256) to floor((max - 128) / 256) (>> of a negative int floors)
	const int ylo = min(o.ay, min(o.by, o.cy)), yhi = max(o.ay, max(o.by, o.cy));
	const int zlo = min(o.az, min(o.bz, o.cz)), zhi = max(o.az, max(o.bz, o.cz));
	o.j0 = max((ylo + 127) >> 8, 0); o.j1 = min((yhi - 128) >> 8, g.Y - 1);
	o.k0 = max((zlo + 127) >> 8, 0); o.k1 = min((zhi - 128) >> 8, g.Zg - 1);
	return (o.j0 > o.j1 || o.k0 > o.k1) ? VOX_NOTHING : VOX_OK;
}

// the directed edge p -> r holds the sample: on its left, or on it and the edge points up (or level and towards +z)
__device__ __forceinline__ bool vox_edge(int py, int pz, int ry, int rz, int Py, int Pz)
{
	const long long dy = ry - py, dz = rz - pz;
	const long long E = dy * (Pz - pz) - dz * (Py - py);
	return E > 0 || (E == 0 && (dy > 0 || (dy == 0 && dz > 0)));
}

// column (j, k) of triangle t: if covered, toggle the first cell whose centre is at or beyond the plane
__device__ __forceinline__ void vox_column(const Geom& g, const VoxTri& t, int W, unsigned* __restrict__ bits, int j, int k)
{
	const int Py = 256 * j + 128, Pz = 256 * k + 128;
	if (!(vox_edge(t.ay, t.az, t.by, t.bz, Py, Pz) && vox_edge(t.by, t.bz, t.cy, t.cz, Py, Pz) && vox_edge(t.cy, t.cz, t.ay, t.az, Py, Pz))) return;
	const long long T = (long long)(t.ax - 128) * t.A - (t.ny * (Py - t.ay) + t.nz * (Pz - t.az));
	const long long D = t.A << 8;
	// i0 = clamp(ceil(T / D), 0, X): the smallest i with i * D >= T.  An fp32 estimate of the quotient (which lies below X, so the estimate is
	// within a step of it), then corrected against the exact products: no 64-bit division
	int i0;
	if (T <= 0) i0 = 0;
	else if (T >= (long long)g.X * D) i0 = g.X;
	else {
		i0 = (int)((float)T / (float)D);
		i0 = min(max(i0, 0), g.X);
		while ((long long)i0 * D < T) ++i0;
		while (i0 > 0 && (long long)(i0 - 1) * D >= T) --i0;
	}
	atomicXor(bits + ((size_t)k * g.Y + j) * W + (i0 >> 5), 1u << (i0 & 31));             // the result is not used: a no-return atomic
}

}  // namespace

__global__ __launch_bounds__(256) void k_vox_scatter(const Geom g, const VoxMesh m, int W, unsigned* __restrict__ bits, unsigned* __restrict__ report,
	unsigned* __restrict__ nbig, uint4* __restrict__ list)
{
	const uint32_t t = blockIdx.x * 4u + (threadIdx.x >> 6);
	const int lane = (int)(threadIdx.x & 63);
	if (t >= m.nt) return;
	VoxTri tr;
	const int st = vox_triangle(g, m, t, tr);                          // wave-uniform: every lane reads the same nine floats
	if (st == VOX_SKIPPED && lane == 0) atomicAdd(report + 1, 1u);
	if (st != VOX_OK) return;
	const int by = tr.j1 - tr.j0 + 1, n = by * (tr.k1 - tr.k0 + 1);     // each extent <= 2^10 (|q| <= 2^18)
	if (n > kVoxBig) {
		if (lane == 0) list[atomicAdd(nbig, 1u)] = make_uint4(t, (unsigned)tr.j0 | ((unsigned)tr.j1 << 16), (unsigned)tr.k0 | ((unsigned)tr.k1 << 16), 0u);
		return;
	}
	for (int c = lane; c < n; c += 64) vox_column(g, tr, W, bits, tr.j0 + c % by, tr.k0 + c / by);
}

// items = (list entry, 16 x 16 patch of the grid); a patch off the triangle's box costs its workgroup one 16-byte load
__global__ __launch_bounds__(256) void k_vox_scatter_big(const Geom g, const VoxMesh m, int W, unsigned* __restrict__ bits, const unsigned* __restrict__ nbig,
	const uint4* __restrict__ list)
{
	const unsigned py = (unsigned)(g.Y + 15) >> 4, pz = (unsigned)(g.Zg + 15) >> 4, P = py * pz;
	const unsigned long long items = (unsigned long long)min(*nbig, m.nt) * P;
	const int jl = (int)(threadIdx.x & 15), kl = (int)(threadIdx.x >> 4);
	for (unsigned long long it = blockIdx.x; it < items; it += gridDim.x) {
		const unsigned p = (unsigned)(it % P);
		const uint4 e = list[it / P];
		const int j = (int)(p % py) * 16, k = (int)(p / py) * 16;
		const int j0 = (int)(e.y & 0xFFFFu), j1 = (int)(e.y >> 16), k0 = (int)(e.z & 0xFFFFu), k1 = (int)(e.z >> 16);
		if (j + 15 < j0 || j > j1 || k + 15 < k0 || k > k1) continue;
		VoxTri tr;
		if (vox_triangle(g, m, e.x, tr) != VOX_OK) continue;
		if (j + jl >= tr.j0 && j + jl <= tr.j1 && k + kl >= tr.k0 && k + kl <= tr.k1) vox_column(g, tr, W, bits, j + jl, k + kl);
	}
}

// 4 mask bits -> 4 bytes of 0 / 1
__device__ __forceinline__ unsigned vox_spread(unsigned nib) { return ((nib & 15u) * 0x00204081u) & 0x01010101u; }

__global__ __launch_bounds__(256) void k_vox_fill(const Geom g, int W, unsigned* __restrict__ bits, uint8_t* __restrict__ mask, int first,
	unsigned* __restrict__ report)
{
	const size_t row = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6);
	const int lane = (int)(threadIdx.x & 63);
	if (row >= (size_t)g.Y * g.Zg) return;
	unsigned* rb = bits + row * W;
	uint8_t* ro = mask + row * g.X;
	const bool wide = (g.X & 15) == 0;                                 // every row then starts on a 16-byte boundary
	unsigned carry = 0;                                                // parity of the toggles below this round's words
	for (int base = 0; base < W; base += 64) {
		const int w = base + lane;
		unsigned t = 0;
		if (w < W) {
			t = rb[w];
			if (t) rb[w] = 0;
		}
		unsigned p = t;                                                // bit b: parity of the word's toggles at or below b
		p ^= p << 1; p ^= p << 2; p ^= p << 4; p ^= p << 8; p ^= p << 16;
		const unsigned long long odd = __builtin_amdgcn_ballot_w64((p >> 31) != 0);
		const unsigned below = (unsigned)__builtin_popcountll(odd & ((1ull << lane) - 1ull)) & 1u;
		if (carry ^ below) p = ~p;
		carry ^= (unsigned)__builtin_popcountll(odd) & 1u;
		const int x0 = w * 32;
		if (w >= W || x0 >= g.X) continue;
		const int n = min(32, g.X - x0);
		if (wide) {                                                    // n is 16 or 32
			for (int h = 0; h < n; h += 16) {
				const unsigned q = p >> h;
				uint4 v = make_uint4(vox_spread(q), vox_spread(q >> 4), vox_spread(q >> 8), vox_spread(q >> 12));
				uint4* dst = reinterpret_cast<uint4*>(ro + x0 + h);
				if (!first) { const uint4 u = *dst; v.x |= u.x; v.y |= u.y; v.z |= u.z; v.w |= u.w; }
				*dst = v;
			}
		} else {
			for (int b = 0; b < n; ++b) {
				const uint8_t v = (uint8_t)((p >> b) & 1u);
				if (first) ro[x0 + b] = v;
				else if (v) ro[x0 + b] = 1;
			}
		}
	}
	if (lane == 0 && carry) atomicAdd(report, 1u);                     // odd with bit X counted: the column is open
}

hipError_t launch_voxel_scatter(const Geom& g, const VoxMesh& m, unsigned* bits, unsigned* report, unsigned* nbig, uint4* list, hipStream_t s)
{
	if (!whole_grid(g) || g.Zg <= 1 || g.Y > 65535 || g.Zg > 65535) return hipErrorNotSupported;
	if (!m.nt) return hipSuccess;
	const int W = voxel_row_words(g);
	hipLaunchKernelGGL(k_vox_scatter, dim3((m.nt + 3u) / 4u), dim3(256), 0, s, g, m, W, bits, report, nbig, list);
	hipError_t e = hipGetLastError();
	if (e != hipSuccess) return e;
	const unsigned long long items = (unsigned long long)m.nt * (unsigned)((g.Y + 15) >> 4) * (unsigned)((g.Zg + 15) >> 4);
	hipLaunchKernelGGL(k_vox_scatter_big, dim3((unsigned)(items < 2048 ? items : 2048)), dim3(256), 0, s, g, m, W, bits, nbig, list);
	return hipGetLastError();
}

hipError_t launch_voxel_fill(const Geom& g, unsigned* bits, uint8_t* mask, bool first, unsigned* report, hipStream_t s)
{
	if (!whole_grid(g) || g.Zg <= 1) return hipErrorNotSupported;
	const size_t rows = (size_t)g.Y * g.Zg;
	hipLaunchKernelGGL(k_vox_fill, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, s, g, voxel_row_words(g), bits, mask, first ? 1 : 0, report);
	return hipGetLastError();
}

}  // namespace fx
