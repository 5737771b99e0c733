// fx_maccormack.hip -- MacCormack advection (fx_set_advection_scheme: FX_ADVECT_MACCORMACK), gfx950.  No reference counterpart (the reference's
// CSAdvect is the semi-Lagrangian step of fx_sim.hip); Selle, Fedkiw, Kim, Liu, Rossignac 2008, with the limiter of its section 3.
//
//   k_mc_predict   hat_q = the semi-Lagrangian sample of q at the back-traced place, all seven quantities, fp32, into the scratch
//   k_mc_correct   bar_q = the sample of hat at the forward-traced place; r = hat + (q - bar) / 2, limited to the back-trace's eight taps; then
//                  k_advect's tail: impulse, attenuation, stores
//
// Per cell (x, y, z) of a whole grid, fp32, every operation rounded as written (tests/maccormack_ref.py restates it in numpy); q = VELOCITY x, y, z
// and COLOR r, g, b, a; u0 = velocity[0] at the cell:
//   1  px = ((float)x + 0.5f) / (float)X (py, pz alike)      a = fmaf(-u0, dt, p)      t = a * N - 0.5f, i0 = floorf(t), f = t - i0
//      taps i0, i0 + 1 through the address mode (clamp / mirror)      hat_q = lerp_z(lerp_y(lerp_x ...)), lerp(a, b, f) = fmaf(f, b - a, a)
//      k_advect's trace and sampler (fx_sim.hip), restated here.  lo = hi = tap 000, then over the taps v in the order 000, 100, 010, 110, 001, 101,
//      011, 111:   lo = v < lo ? v : lo      hi = v > hi ? v : hi      (selects: the earlier of +0 / -0 stays, a NaN tap never replaces a bound)
//   2  k_mc_predict stores hat_q into the scratch (three planes + one float4 volume, fp32 whatever the storage)
//   3  b = fmaf(u0, dt, p), taps and fractions as in 1;   bar_q = the same sample of the scratch
//   4  r = fmaf(0.5f, q - bar_q, hat_q), q as stored at the cell;   r = r < lo ? lo : (r > hi ? hi : r)
//   5  k_advect's impulse block under sp.impulse (CSAdvect.hlsl:60-67), atten = fmaxf(fmaf(-dt, 0.2f, 1), 0), velocity[1] = r * atten,
//      colour[parity] = r * atten (fp16 storage: rounded once, RNE), the render's alpha side volume where the launch is given one
// A 2-D grid goes through the same code: its two z taps are both plane 0 and the z lerp runs on equal operands.
//
// Two launches over the grid, 64 x 4 x 1 tiles (one wave64 = 64 consecutive x of a row), modelled on k_heat.  Near-cell gathers bound by the
// texture path and memory traffic: the taps come through the L1 / L2 (neighbouring cells share them), nothing is staged in the LDS.  Every
// field is addressed with 32-bit byte offsets from uniform bases (saddr + voffset accesses) while the largest one is under 4 GiB, with 64-bit
// ones above (WIDE).  The corrector recomputes hat_q from the taps it loads for the bounds (the same bits as the predictor stored) and works
// quantity by quantity -- a velocity component, then the next, then the colour texel -- so that only one set of { taps, lo, hi, hat, bar }
// is live at a time.
#include "fx_internal.h"
#include "fx_store.h"

namespace fx {

using namespace sto;

namespace {

const int MC_X = kMcTileX, MC_Y = kMcTileY;

__device__ __forceinline__ float lerpf(float a, float b, float f) { return fmaf(f, b - a, a); }
__device__ __forceinline__ float saturatef(float x) { return fminf(fmaxf(x, 0.0f), 1.0f); }

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

// the eight taps of a trace as cell offsets (in the order 000, 100, 010, 110, 001, 101, 011, 111) and the three fractions
template <typename O> struct Taps { O c[8]; float fx, fy, fz; };

// the trace from cell centre p along sign * u0 (rules 1 and 3)
template <typename O>
__device__ __forceinline__ Taps<O> trace(const Geom& g, float px, float py, float pz, float ux, float uy, float uz, float dt, int address)
{
	const float ax = fmaf(ux, dt, px), ay = fmaf(uy, dt, py), az = fmaf(uz, dt, pz);
	const float tx = ax * (float)g.X - 0.5f, ty = ay * (float)g.Y - 0.5f, tz = az * (float)g.Zg - 0.5f;
	const float flx = floorf(tx), fly = floorf(ty), flz = floorf(tz);
	Taps<O> t;
	t.fx = tx - flx; t.fy = ty - fly; t.fz = tz - flz;
	const int ix = (int)flx, iy = (int)fly, iz = (int)flz;
	const O X = (O)g.X, plane = (O)g.X * (O)g.Y;
	const O x0 = (O)addr_tap(ix, g.X, address), x1 = (O)addr_tap(ix + 1, g.X, address);
	const O r0 = (O)addr_tap(iy, g.Y, address) * X, r1 = (O)addr_tap(iy + 1, g.Y, address) * X;
	const O p0 = (O)addr_tap(iz, g.Zg, address) * plane, p1 = (O)addr_tap(iz + 1, g.Zg, address) * plane;
	t.c[0] = p0 + r0 + x0; t.c[1] = p0 + r0 + x1; t.c[2] = p0 + r1 + x0; t.c[3] = p0 + r1 + x1;
	t.c[4] = p1 + r0 + x0; t.c[5] = p1 + r0 + x1; t.c[6] = p1 + r1 + x0; t.c[7] = p1 + r1 + x1;
	return t;
}

__device__ __forceinline__ float tri(const float (&v)[8], float fx, float fy, float fz)
{
	return lerpf(lerpf(lerpf(v[0], v[1], fx), lerpf(v[2], v[3], fx), fy), lerpf(lerpf(v[4], v[5], fx), lerpf(v[6], v[7], fx), fy), fz);
}

// rule 4 for one quantity: v = the back-trace's taps (hat and the bounds come from them), bar = the forward sample of the scratch
__device__ __forceinline__ float correct(const float (&v)[8], float fx, float fy, float fz, float q, float bar)
{
	const float hat = tri(v, fx, fy, fz);
	float lo = v[0], hi = v[0];
#pragma unroll
	for (int k = 0; k < 8; ++k) {
		lo = v[k] < lo ? v[k] : lo;
		hi = v[k] > hi ? v[k] : hi;
	}
	const float r = fmaf(0.5f, q - bar, hat);
	return r < lo ? lo : (r > hi ? hi : r);
}

// workgroup -> (tile x, tile y, plane) on the grid's 64 x 4 raster -> the cell, or false outside the grid
__device__ __forceinline__ bool cell_of(const Geom& g, int tiles_x, int tiles_y, int& x, int& y, int& z)
{
	int bid = (int)blockIdx.x;
	const int tile_x = bid % tiles_x; bid /= tiles_x;
	const int tile_y = bid % tiles_y;
	z = bid / tiles_y;
	x = tile_x * MC_X + (int)threadIdx.x;
	y = tile_y * MC_Y + (int)threadIdx.y;
	return x < g.X && y < g.Y && z < g.Zg;
}

}  // namespace

template <bool HALF, bool WIDE>
__global__ __launch_bounds__(256) void k_mc_predict(const Geom g, int tiles_x, int tiles_y, const void* __restrict__ vel_in, const void* __restrict__ col_in,
	float* __restrict__ hat_vel, float* __restrict__ hat_col, float dt, int address)
{
	typedef Cell<HALF> Ce;
	typedef Cell<false> Sc;                                     // the scratch
	typedef typename Off<WIDE>::T O;
	int x, y, z;
	if (!cell_of(g, tiles_x, tiles_y, x, y, z)) return;

	const O plane = (O)g.X * (O)g.Y;
	const O stride = plane * (O)g.Zg;                           // cells between velocity component planes (a whole grid: no halo)
	const O id = (O)z * plane + (O)y * (O)g.X + (O)x;
	const char* vi = static_cast<const char*>(vel_in);
	const char* ci = static_cast<const char*>(col_in);
	char* hv = reinterpret_cast<char*>(hat_vel);
	char* hc = reinterpret_cast<char*>(hat_col);

	// ---- 1: the back-trace and the taps of k_advect
	const float px = ((float)x + 0.5f) / (float)g.X;
	const float py = ((float)y + 0.5f) / (float)g.Y;
	const float pz = ((float)z + 0.5f) / (float)g.Zg;
	const float u0x = Ce::ld1(vi, id), u0y = Ce::ld1(vi, stride + id), u0z = Ce::ld1(vi, (O)2 * stride + id);
	const Taps<O> t = trace<O>(g, px, py, pz, -u0x, -u0y, -u0z, dt, address);

	// ---- 2: hat_q into the scratch, quantity by quantity
#pragma unroll
	for (int a = 0; a < 3; ++a) {
		float v[8];
#pragma unroll
		for (int k = 0; k < 8; ++k) v[k] = Ce::ld1(vi, (O)a * stride + t.c[k]);
		Sc::st1(hv, (O)a * stride + id, tri(v, t.fx, t.fy, t.fz));
	}
	{
		float4 c[8];
#pragma unroll
		for (int k = 0; k < 8; ++k) c[k] = Ce::ld4(ci, t.c[k]);
		float h[4];
#define FX_MC_TRI(m, i) { const float v[8] = { c[0].m, c[1].m, c[2].m, c[3].m, c[4].m, c[5].m, c[6].m, c[7].m }; h[i] = tri(v, t.fx, t.fy, t.fz); }
		FX_MC_TRI(x, 0) FX_MC_TRI(y, 1) FX_MC_TRI(z, 2) FX_MC_TRI(w, 3)
#undef FX_MC_TRI
		(void)Sc::st4(hc, id, h);
	}
}

template <bool HALF, bool WIDE>
__global__ __launch_bounds__(256) void k_mc_correct(const Geom g, int tiles_x, int tiles_y, const SimParams sp, const void* __restrict__ vel_in,
	const void* __restrict__ col_in, const float* __restrict__ hat_vel, const float* __restrict__ hat_col, void* __restrict__ vel_out, void* __restrict__ col_out,
	float* __restrict__ alpha_out)
{
	typedef Cell<HALF> Ce;
	typedef Cell<false> Sc;                                     // the scratch
	typedef typename Off<WIDE>::T O;
	int x, y, z;
	if (!cell_of(g, tiles_x, tiles_y, x, y, z)) return;

	const O plane = (O)g.X * (O)g.Y;
	const O stride = plane * (O)g.Zg;
	const O id = (O)z * plane + (O)y * (O)g.X + (O)x;
	const char* vi = static_cast<const char*>(vel_in);
	const char* ci = static_cast<const char*>(col_in);
	const char* hv = reinterpret_cast<const char*>(hat_vel);
	const char* hc = reinterpret_cast<const char*>(hat_col);
	char* vo = static_cast<char*>(vel_out);
	char* co = static_cast<char*>(col_out);
	const float dt = sp.dt;

	// ---- 1, 3: the back-trace and the forward trace from the same cell with the same u0
	const float px = ((float)x + 0.5f) / (float)g.X;
	const float py = ((float)y + 0.5f) / (float)g.Y;
	const float pz = ((float)z + 0.5f) / (float)g.Zg;
	const float u0[3] = { Ce::ld1(vi, id), Ce::ld1(vi, stride + id), Ce::ld1(vi, (O)2 * stride + id) };
	const Taps<O> tb = trace<O>(g, px, py, pz, -u0[0], -u0[1], -u0[2], dt, sp.address);
	const Taps<O> tf = trace<O>(g, px, py, pz, u0[0], u0[1], u0[2], dt, sp.address);

	// ---- 4: correction and limiter, quantity by quantity (a velocity component's own value is u0)
	float u[3], c[4];
#pragma unroll
	for (int a = 0; a < 3; ++a) {
		float v[8], w[8];
#pragma unroll
		for (int k = 0; k < 8; ++k) v[k] = Ce::ld1(vi, (O)a * stride + tb.c[k]);
#pragma unroll
		for (int k = 0; k < 8; ++k) w[k] = Sc::ld1(hv, (O)a * stride + tf.c[k]);
		u[a] = correct(v, tb.fx, tb.fy, tb.fz, u0[a], tri(w, tf.fx, tf.fy, tf.fz));
	}
	{
		float4 b[8], f[8];
#pragma unroll
		for (int k = 0; k < 8; ++k) b[k] = Ce::ld4(ci, tb.c[k]);
#pragma unroll
		for (int k = 0; k < 8; ++k) f[k] = Sc::ld4(hc, tf.c[k]);
		const float4 q = Ce::ld4(ci, id);
#define FX_MC_COR(m, i) { const float v[8] = { b[0].m, b[1].m, b[2].m, b[3].m, b[4].m, b[5].m, b[6].m, b[7].m }; \
		const float w[8] = { f[0].m, f[1].m, f[2].m, f[3].m, f[4].m, f[5].m, f[6].m, f[7].m }; \
		c[i] = correct(v, tb.fx, tb.fy, tb.fz, q.m, tri(w, tf.fx, tf.fy, tf.fz)); }
		FX_MC_COR(x, 0) FX_MC_COR(y, 1) FX_MC_COR(z, 2) FX_MC_COR(w, 3)
#undef FX_MC_COR
	}

	// ---- 5: the tail of k_advect -- the built-in impulse (CSAdvect.hlsl:59-68, Impulse.hlsli:14), the attenuation (:74), the stores (:77-78)
	if (sp.impulse) {                                                        // (fx_set_impulse: a uniform flag)
		const float dx = px + -0.5f, dy = py + -0.100000001f, dz = pz + -0.5f;
		const float d2 = fmaf(dz, dz, fmaf(dy, dy, dx * dx));
		const float rr = sp.is3d ? 0.00390625f : 0.0009765625f;
		const float basis = exp2f(((d2 * -4.0f) / rr) * 1.44269502f);
		if (basis >= 0.0183156393f) {                                        // :60
			float Fx, Fy, Fz;
			if (sp.is3d) {                                                   // :63-65
				Fx = fmaf(basis, 0.0f, dz * -200.0f);
				Fy = fmaf(basis, 192.0f, 0.0f);
				Fz = fmaf(basis, 0.0f, dx * 200.0f);
			} else {
				Fx = 0.0f; Fy = basis * 48.0f; Fz = 0.0f;
			}
			u[0] = fmaf(Fx, dt, u[0]); u[1] = fmaf(Fy, dt, u[1]); u[2] = fmaf(Fz, dt, u[2]);   // :66
			const float bdt = basis * dt;
			c[0] = saturatef(fmaf(bdt, 8.0f, c[0]));                         // :67, g_impulse = (.2,.4,1,1)*40
			c[1] = saturatef(fmaf(bdt, 16.0f, c[1]));
			c[2] = saturatef(fmaf(bdt, 40.0f, c[2]));
			c[3] = saturatef(fmaf(bdt, 40.0f, c[3]));
		}
	}
	const float atten = fmaxf(fmaf(-dt, 0.200000003f, 1.0f), 0.0f);
	Ce::st1(vo, id, u[0] * atten);
	Ce::st1(vo, stride + id, u[1] * atten);
	Ce::st1(vo, (O)2 * stride + id, u[2] * atten);
	const float out[4] = { c[0] * atten, c[1] * atten, c[2] * atten, c[3] * atten };
	const float alpha = Ce::st4(co, id, out);
	if (alpha_out) *reinterpret_cast<float*>(reinterpret_cast<char*>(alpha_out) + id * (O)4) = alpha;   // the render's alpha side volume (fx_render_accel.hip)
}

template <bool HALF, bool WIDE>
static hipError_t launch_mc_t(dim3 grid, dim3 block, hipStream_t s, const Geom& g, int tiles_x, int tiles_y, const SimParams& sp, const void* vel_in,
	const void* col_in, void* vel_out, void* col_out, float* hat_vel, float* hat_col, float* alpha_out)
{
	hipLaunchKernelGGL((k_mc_predict<HALF, WIDE>), grid, block, 0, s, g, tiles_x, tiles_y, vel_in, col_in, hat_vel, hat_col, sp.dt, sp.address);
	const hipError_t e = hipGetLastError();
	if (e != hipSuccess) return e;
	hipLaunchKernelGGL((k_mc_correct<HALF, WIDE>), grid, block, 0, s, g, tiles_x, tiles_y, sp, vel_in, col_in, hat_vel, hat_col, vel_out, col_out, alpha_out);
	return hipGetLastError();
}

hipError_t launch_maccormack(const Geom& g, const SimParams& sp, int half_store, const void* vel_in, const void* col_in, void* vel_out, void* col_out,
	float* hat_vel, float* hat_col, float* alpha_out, hipStream_t s)
{
	if (!whole_grid(g)) return hipErrorNotSupported;                            // (fx_set_advection_scheme refuses slab ranks)
	if (!vel_in || !col_in || !vel_out || !col_out || !hat_vel || !hat_col || vel_in == vel_out || col_in == col_out) return hipErrorInvalidValue;
	if (g.X <= 0 || g.Y <= 0 || g.Zg <= 0) return hipErrorInvalidValue;
	const int tiles_x = (g.X + MC_X - 1) / MC_X, tiles_y = (g.Y + MC_Y - 1) / MC_Y;
	const long long wgs = (long long)tiles_x * tiles_y * g.Zg;
	if (wgs > 0x7FFFFFFFll) return hipErrorInvalidValue;
	const dim3 grid((unsigned)wgs, 1, 1), block(MC_X, MC_Y, 1);
	const bool wide = colour_wants_wide_offsets(g);
	if (half_store) return wide ? launch_mc_t<true, true>(grid, block, s, g, tiles_x, tiles_y, sp, vel_in, col_in, vel_out, col_out, hat_vel, hat_col, alpha_out)
	                            : launch_mc_t<true, false>(grid, block, s, g, tiles_x, tiles_y, sp, vel_in, col_in, vel_out, col_out, hat_vel, hat_col, alpha_out);
	return wide ? launch_mc_t<false, true>(grid, block, s, g, tiles_x, tiles_y, sp, vel_in, col_in, vel_out, col_out, hat_vel, hat_col, alpha_out)
	            : launch_mc_t<false, false>(grid, block, s, g, tiles_x, tiles_y, sp, vel_in, col_in, vel_out, col_out, hat_vel, hat_col, alpha_out);
}

}  // namespace fx
