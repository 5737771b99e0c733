// fx_obstacle_draw.hip -- the obstacle draw (fx_set_obstacle_draw): the solid cells of the code volume ray-cast into the render target and a
// depth buffer, gfx950.  No reference counterpart.
//
//   k_obstacle_pack   bit 6 of the code volume folded into one uint64 per 4 x 4 x 4 brick
//   k_obstacle_cast   per pixel the view ray walked through the bricks to the first solid cell, its face shaded, colour and D3D depth stored
//
// The rule, fp32, every operation rounded as written (include/fluidx_hip.h states it, tests/obstacle_draw_ref.py restates it in numpy);
// N = (X, Y, Z), S(i) = code bit 6, M = the forward WorldViewProj rows:
//   ray      (o, d) = pixel_ray (fx_march.h), e = the entry axis of compute_ray_origin (-1: the eye is inside the box); a discard is a miss
//   start    s_a = fma(o_a, .5, .5);  i_a = min(max((int)floorf(s_a * N_a), 0), N_a - 1);  st_a = (d_a > 0) - (d_a < 0);  r_a = 1 / d_a;
//            S(i): a hit at t = 0, p = o, face = e >= 0 ? 2e + (d_e > 0) : 6
//   walk     t_a = st_a ? (fma((float)(i_a + (st_a > 0)) / (float)N_a, 2, -1) - o_a) * r_a : FLT_MAX;
//            a* = (t_0 <= t_1 && t_0 <= t_2) ? 0 : (t_1 <= t_2) ? 1 : 2;  st_a* == 0: miss;  i_a* += st_a*;  off the grid: miss;
//            S(i): hit, t_hit = t_a*, face = 2 a* + (st_a* > 0), p_a = fma(d_a, t_hit, o_a);  X + Y + Z advances at most
//   visible  h_r = fma(1, M[4r+3], fma(p_2, M[4r+2], fma(p_1, M[4r+1], p_0 * M[4r+0])));  cz = h_2 / h_3;
//            drawn iff h_3 > 0 && 0 <= cz && cz < 1 && (no scene depth || cz <= scene[py][px])
//   shade    L = light_dir_local or point_light_ray(light_point_local, p);  st = face & 1 ? +1 : -1, a = face >> 1;
//            ndl = face < 6 ? fmaxf(0, (float)(-st) * L_a) : 0;  src_c = (k_c * fma(ndl, lc_c, am_c)) * 0.159154937f with k_c = albedo_c * albedo_w,
//            lc_c = color_w * color_c, am_c = ambient_w * ambient_c
//   store    drawn: target = unorm8(src) | 255 << 24, out_float = (src, 1), depth_out = cz;  else the target is not stored, out_float = 0,
//            depth_out = scene depth or 1;  hits = a hit ? 1 << 63 | drawn << 62 | face << 32 | (z Y + y) X + x : 0
//
// Every t of the walk is a function of an integer plane index; nothing accumulates.  So the walk may leave out every load and test whose answer it
// knows -- a cell outside the solids' bounding box, a cell of a brick whose word is 0 -- and may end as a miss once it is outside the box on an
// axis it does not move back on: the cells it visits, the t it reports and so every stored bit are those of the plain walk.  It keeps the current
// brick's word in registers, loads when the brick index changes, and only t of the stepped axis is recomputed.
// k_obstacle_cast: one lane per pixel, a wave = an 8 x 8 pixel tile as in k_raycast_direct.  No atomics, no lane writes another's pixel; every
// index is clamped or tested before use; the only loop is bounded by the rule's cap.
// FX_ODRAW_FLAT (a timing build, docs/LAB.md; not a shipped knob): the plain walk -- one code byte per cell, no box, no bricks.
#include "fx_march.h"
#include <algorithm>

namespace fx {

namespace {

typedef unsigned long long u64;

struct ObstCastArgs {
	float wvp[16];
	const float* scene;     // the caller's scene depth float[H][W], or null
	int W, H;
	int lo[3], hi[3];       // the solids' bounding box [lo, hi)
	float k[3], lc[3], am[3];
};

__device__ __forceinline__ int sel3(bool a0, bool a1, int v0, int v1, int v2) { return a0 ? v0 : a1 ? v1 : v2; }
__device__ __forceinline__ float sel3(bool a0, bool a1, float v0, float v1, float v2) { return a0 ? v0 : a1 ? v1 : v2; }

// t of the plane in front of cell index i on an axis of n cells
__device__ __forceinline__ float plane_t(int i, int st, int n, float o, float r)
{
	if (!st) return 3.40282347e+38f;
	const float P = fmaf((float)(i + (st > 0)) / (float)n, 2.0f, -1.0f);
	return (P - o) * r;
}

}  // namespace

// one thread per brick; rows of four code bytes, bounds tested per cell
__global__ __launch_bounds__(256) void k_obstacle_pack(const Geom g, const uint8_t* __restrict__ code, u64* __restrict__ bricks, int BX, int BY, int BZ)
{
	const unsigned b = blockIdx.x * 256u + threadIdx.x;
	if (b >= (unsigned)BX * (unsigned)BY * (unsigned)BZ) return;
	const int bx = (int)(b % (unsigned)BX), by = (int)((b / (unsigned)BX) % (unsigned)BY), bz = (int)(b / ((unsigned)BX * (unsigned)BY));
	u64 w = 0;
	for (int dz = 0; dz < 4; ++dz) {
		const int z = bz * 4 + dz;
		if (z >= g.Zg) break;
		for (int dy = 0; dy < 4; ++dy) {
			const int y = by * 4 + dy;
			if (y >= g.Y) break;
			const uint8_t* row = code + ((size_t)z * (size_t)g.Y + (size_t)y) * (size_t)g.X;
#pragma unroll
			for (int dx = 0; dx < 4; ++dx) {
				const int x = bx * 4 + dx;
				if (x < g.X && (row[x] & 0x40u)) w |= (u64)1 << (dz * 16 + dy * 4 + dx);
			}
		}
	}
	bricks[b] = w;
}

template <bool FLAT>
__global__ __launch_bounds__(64) void k_obstacle_cast(const Geom g, const uint8_t* __restrict__ code, const u64* __restrict__ bricks, const FrameConsts fc,
	const ObstCastArgs a, int point_light, uint32_t* __restrict__ target, float4* __restrict__ out_float, float* __restrict__ depth_out, u64* __restrict__ hits)
{
	const int px = blockIdx.x * 8 + threadIdx.x, py = blockIdx.y * 8 + threadIdx.y;
	if (px >= a.W || py >= a.H) return;
	const size_t pix = (size_t)py * (size_t)a.W + (size_t)px;
	const float behind = a.scene ? a.scene[pix] : 1.0f;
	const int N0 = g.X, N1 = g.Y, N2 = g.Zg;
	float o[3], d[3];
	int e;
	bool hit = false, start = false;
	int face = 6, i0 = 0, i1 = 0, i2 = 0;
	float th = 0.0f;
	if (code != nullptr && pixel_ray(fc, px, py, a.W, a.H, o, d, e)) {
		// ---- start
		i0 = min(max((int)floorf(fmaf(o[0], 0.5f, 0.5f) * (float)N0), 0), N0 - 1);
		i1 = min(max((int)floorf(fmaf(o[1], 0.5f, 0.5f) * (float)N1), 0), N1 - 1);
		i2 = min(max((int)floorf(fmaf(o[2], 0.5f, 0.5f) * (float)N2), 0), N2 - 1);
		const int st0 = (d[0] > 0.0f) - (d[0] < 0.0f), st1 = (d[1] > 0.0f) - (d[1] < 0.0f), st2 = (d[2] > 0.0f) - (d[2] < 0.0f);
		const float r0 = 1.0f / d[0], r1 = 1.0f / d[1], r2 = 1.0f / d[2];
		const int BX = (N0 + 3) >> 2, BY = (N1 + 3) >> 2;
		unsigned cur = 0xFFFFFFFFu;                                                     // the brick whose word is held
		u64 word = 0;
		// S(i) of the current cell.  Bricks: nothing is loaded or tested outside the box or while the word is 0
		auto solid = [&]() -> bool {
			if (FLAT) return (code[((size_t)i2 * (size_t)N1 + (size_t)i1) * (size_t)N0 + (size_t)i0] & 0x40u) != 0;
			if (i0 < a.lo[0] || i0 >= a.hi[0] || i1 < a.lo[1] || i1 >= a.hi[1] || i2 < a.lo[2] || i2 >= a.hi[2]) return false;
			const unsigned b = ((unsigned)(i2 >> 2) * (unsigned)BY + (unsigned)(i1 >> 2)) * (unsigned)BX + (unsigned)(i0 >> 2);
			if (b != cur) { cur = b; word = bricks[b]; }
			return word != 0 && ((word >> ((i2 & 3) * 16 + (i1 & 3) * 4 + (i0 & 3))) & 1) != 0;
		};
		// outside the box on an axis the walk does not come back on: no solid cell lies ahead
		auto gone = [&](int i, int st, int lo, int hi) -> bool { return (i >= hi && st >= 0) || (i < lo && st <= 0); };
		if (solid()) {
			hit = start = true;
			face = e >= 0 ? 2 * e + ((e == 0 ? d[0] : e == 1 ? d[1] : d[2]) > 0.0f ? 1 : 0) : 6;
		}
		else {
			// ---- walk
			float t0 = plane_t(i0, st0, N0, o[0], r0), t1 = plane_t(i1, st1, N1, o[1], r1), t2 = plane_t(i2, st2, N2, o[2], r2);
			const int cap = N0 + N1 + N2;
			for (int n = 0; n < cap; ++n) {
				if (!FLAT && (gone(i0, st0, a.lo[0], a.hi[0]) || gone(i1, st1, a.lo[1], a.hi[1]) || gone(i2, st2, a.lo[2], a.hi[2]))) break;
				const bool a0 = t0 <= t1 && t0 <= t2, a1 = !a0 && t1 <= t2;
				const int st = sel3(a0, a1, st0, st1, st2);
				if (!st) break;                                                             // the walk cannot move
				const int ia = sel3(a0, a1, i0, i1, i2) + st, Na = sel3(a0, a1, N0, N1, N2);
				if ((unsigned)ia >= (unsigned)Na) break;                                    // off the grid
				const float tn = sel3(a0, a1, t0, t1, t2);
				const float ta = plane_t(ia, st, Na, sel3(a0, a1, o[0], o[1], o[2]), sel3(a0, a1, r0, r1, r2));
				i0 = a0 ? ia : i0; i1 = a1 ? ia : i1; i2 = (a0 || a1) ? i2 : ia;
				t0 = a0 ? ta : t0; t1 = a1 ? ta : t1; t2 = (a0 || a1) ? t2 : ta;
				if (solid()) {
					hit = true;
					th = tn;
					face = 2 * sel3(a0, a1, 0, 1, 2) + (st > 0 ? 1 : 0);
					break;
				}
			}
		}
	}
	bool drawn = false;
	float cz = 0.0f, src[3] = { 0.0f, 0.0f, 0.0f };
	if (hit) {
		const float p0 = start ? o[0] : fmaf(d[0], th, o[0]), p1 = start ? o[1] : fmaf(d[1], th, o[1]), p2 = start ? o[2] : fmaf(d[2], th, o[2]);
		// ---- visible
		const float* M = a.wvp;
		const float h2 = fmaf(1.0f, M[11], fmaf(p2, M[10], fmaf(p1, M[9], p0 * M[8])));
		const float h3 = fmaf(1.0f, M[15], fmaf(p2, M[14], fmaf(p1, M[13], p0 * M[12])));
		cz = h2 / h3;
		drawn = h3 > 0.0f && 0.0f <= cz && cz < 1.0f && (a.scene == nullptr || cz <= behind);
		if (drawn) {
			// ---- shade
			float lx, ly, lz;
			if (point_light) {
				float qx, qy, qz, tEnd;
				light_point_local(fc, qx, qy, qz);
				point_light_ray(qx, qy, qz, p0, p1, p2, lx, ly, lz, tEnd);
			}
			else light_dir_local(fc, lx, ly, lz);
			const int ax = face >> 1;
			const float La = ax == 0 ? lx : ax == 1 ? ly : lz;
			const float ndl = face < 6 ? fmaxf(0.0f, ((face & 1) ? -1.0f : 1.0f) * La) : 0.0f;
#pragma unroll
			for (int c = 0; c < 3; ++c) src[c] = (a.k[c] * fmaf(ndl, a.lc[c], a.am[c])) * 0.159154937f;
		}
	}
	if (drawn) {
		if (target) target[pix] = to_unorm8(src[0]) | (to_unorm8(src[1]) << 8) | (to_unorm8(src[2]) << 16) | (255u << 24);
		if (out_float) out_float[pix] = make_float4(src[0], src[1], src[2], 1.0f);
	}
	else if (out_float) out_float[pix] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
	if (depth_out) depth_out[pix] = drawn ? cz : behind;
	if (hits) {
		const u64 cell = (u64)(((size_t)i2 * (size_t)N1 + (size_t)i1) * (size_t)N0 + (size_t)i0);
		hits[pix] = hit ? ((u64)1 << 63) | ((u64)(drawn ? 1 : 0) << 62) | ((u64)face << 32) | cell : 0;
	}
}

hipError_t launch_obstacle_pack(const Geom& g, const uint8_t* code, unsigned long long* bricks, hipStream_t s)
{
	if (!whole_grid(g)) return hipErrorNotSupported;                            // (fx_set_obstacle_draw refuses slab ranks)
	if (!code || !bricks || g.Zg <= 1 || g.cells_owned() >= ((size_t)1 << 32)) return hipErrorInvalidValue;
	const int BX = (g.X + 3) / 4, BY = (g.Y + 3) / 4, BZ = (g.Zg + 3) / 4;
	const size_t n = obstacle_brick_count(g);
	hipLaunchKernelGGL(k_obstacle_pack, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, g, code, bricks, BX, BY, BZ);
	return hipGetLastError();
}

hipError_t launch_obstacle_cast(const Geom& g, const uint8_t* code, const unsigned long long* bricks, const int lo[3], const int hi[3],
	const FrameConsts& fc, const float wvp[16], int point_light, const fx_obstacle_draw& dr, const float* scene, int W, int H,
	uint8_t* target, float* out_float, float* depth_out, unsigned long long* hits, hipStream_t s)
{
	if (!whole_grid(g)) return hipErrorNotSupported;
	if (g.Zg <= 1 || g.cells_owned() >= ((size_t)1 << 32) || W <= 0 || H <= 0 || (code && !bricks)) return hipErrorInvalidValue;
	if (scene != nullptr && scene == depth_out) return hipErrorInvalidValue;    // a lane would read what another has written
	ObstCastArgs a;
	for (int k = 0; k < 16; ++k) a.wvp[k] = wvp[k];
	a.scene = scene; a.W = W; a.H = H;
	for (int c = 0; c < 3; ++c) {
		// (the box is clamped to the grid: whatever the caller passes, the brick index stays inside the volume)
		a.lo[c] = std::max(lo[c], 0);
		a.hi[c] = std::min(hi[c], c == 0 ? g.X : c == 1 ? g.Y : g.Zg);
		a.k[c] = dr.albedo[c] * dr.albedo[3];
		a.lc[c] = fc.light_color[3] * fc.light_color[c];
		a.am[c] = fc.ambient[3] * fc.ambient[c];
	}
	const dim3 grid((W + 7) / 8, (H + 7) / 8, 1), block(8, 8, 1);
#ifdef FX_ODRAW_FLAT
	const bool flat = true;
#else
	const bool flat = false;
	if (a.hi[0] <= a.lo[0] || a.hi[1] <= a.lo[1] || a.hi[2] <= a.lo[2]) code = nullptr;   // an empty box -- a mask without a solid cell -- casts like no mask
#endif
	if (flat) hipLaunchKernelGGL(k_obstacle_cast<true>, grid, block, 0, s, g, code, bricks, fc, a, point_light, reinterpret_cast<uint32_t*>(target),
		reinterpret_cast<float4*>(out_float), depth_out, hits);
	else hipLaunchKernelGGL(k_obstacle_cast<false>, grid, block, 0, s, g, code, bricks, fc, a, point_light, reinterpret_cast<uint32_t*>(target),
		reinterpret_cast<float4*>(out_float), depth_out, hits);
	return hipGetLastError();
}

}  // namespace fx
