// fx_particles.hip -- tracer particles carried by the flow (fx_set_particles) and the point query (fx_sample_velocity), gfx950.  No reference
// counterpart: the reference carries nothing but its grid fields.
//
//   k_move_particles   every live record (x, y, z, age) takes one Euler or midpoint step through the stored velocity
//   k_sample_velocity  the velocity at a list of points
//
// The rule, fp32, every operation rounded as written (include/fluidx_hip.h states it, tests/particle_ref.py restates it in numpy), N = (X, Y, Z),
// c(v) = fminf(fmaxf(v, 0), 1) (a NaN becomes 0, -0 becomes +0):
//   U(p), per axis:  s = c(p_a), t = s * N_a - 0.5f, fl = floorf(t), f = t - fl, taps (int)fl and (int)fl + 1 clamped to [0, N_a - 1]; each
//         component plane through k_advect's colour sampler (fx_sim.hip FX_TRI, restated in fx_heat.hip): lerp(a, b, f) = fmaf(f, b - a, a),
//         x, then y, then z.  A 2-D grid's two z taps are both plane 0: the plane's taps are loaded once, the z lerp runs on equal operands.
//   move, per live record (age >= 0; every bit of any other record stays):
//         k1 = U(p) + drift;   midpoint: m_a = c(fmaf(k1_a, 0.5f * dt, p_a)), k = U(m) + drift;   Euler: k = k1
//         q_a = fmaf(k_a, dt, p_a);   an open face the record crosses (q_a < 0 / q_a > 1) kills it;   q_a = c(q_a)
//         a mask is set and the cell min((int)(q_a * N_a), N_a - 1) is solid (code bit 6): the position stays p, bits kept
//         age1 = age + dt;  lifetime > 0 && age1 >= lifetime kills it;   stored: (position, dead ? -1 : age1)
//         a 2-D grid leaves z alone altogether: q_z = p_z, bits kept, no wall, no clamp, cell plane 0
// No value reaches an index computation unclamped, so a record the caller wrote on the device, whatever it holds, is safe to read.
//
// One lane per record, 256-thread workgroups, no LDS; the record is one 16-byte load and one 16-byte store (the 2-D kernels never change z: the
// compiler reads the age first and leaves z out of the store).  The kernel is a scattered gather:
// the midpoint scheme samples three planes twice, 48 taps, and what bounds it is how many of them a CU keeps in flight.  So (a) the two x taps
// of a row come as ONE load of two adjacent cells (8 bytes in fp32, 4 in fp16, at the alignment of one cell): the pair starts at
// min(max(i0, 0), X - 2), and the two taps are selected from it by index compare, which also serves the rows where both taps clamp onto
// the same wall cell -- 24 loads, not 48; (b) the four pairs of a component are issued before its first lerp and nothing but the
// sampler's own dependency (the midpoint needs k1) orders the three components, and (c) the register count stays at or below 64, i.e. eight waves
// per SIMD.  A dead lane leaves before its first tap.  Fields are addressed as fx_store.h has it: 32-bit cell offsets while the colour
// field is under 4 GiB, 64-bit ones above (WIDE).
#include "fx_internal.h"
#include "fx_store.h"
#include "fx_particle_cell.h"

namespace fx {

using namespace sto;

namespace {

const int PT_WG = 256;

__device__ __forceinline__ float lerpf(float a, float b, float f) { return fmaf(f, b - a, a); }

// two adjacent cells of a plane in one load, at the alignment of one cell
struct __attribute__((packed, aligned(4))) PairF { float a, b; };
struct __attribute__((packed, aligned(2))) PairH { h16 a, b; };
template <bool HALF> struct Pair;
template <> struct Pair<false> {
	template <typename O> static __device__ __forceinline__ float2 ld(const char* b, O cell)
	{
		const PairF p = *reinterpret_cast<const PairF*>(b + cell * (O)4);
		return make_float2(p.a, p.b);
	}
};
template <> struct Pair<true> {
	template <typename O> static __device__ __forceinline__ float2 ld(const char* b, O cell)
	{
		const PairH p = *reinterpret_cast<const PairH*>(b + cell * (O)2);
		return make_float2((float)p.a, (float)p.b);
	}
};

// what the sampler needs of the grid: extents, and cells between the component planes / in the whole velocity field less two (the last pair)
template <typename O> struct Grid { int X, Y, Z; O plane, stride, last_pair; };

// one axis of U: fraction and the two clamped taps
__device__ __forceinline__ void axis_taps(float p, int n, float* f, int* i0, int* t0, int* t1)
{
	const float s = clamp01(p);
	const float t = s * (float)n - 0.5f;
	const float fl = floorf(t);
	*f = t - fl;
	*i0 = (int)fl;                                                      // -1 .. n - 1
	*t0 = min(max(*i0, 0), n - 1);
	*t1 = min(max(*i0 + 1, 0), n - 1);
}

// U(p): the three components of the stored velocity at a point of texture space
template <bool HALF, bool IS3D, typename O>
__device__ __forceinline__ void sample_u(const char* __restrict__ vel, const Grid<O>& g, float px, float py, float pz, float (&u)[3])
{
	float fx, fy, fz;
	int ix, iy, iz, x0, x1, y0, y1, z0, z1;
	axis_taps(px, g.X, &fx, &ix, &x0, &x1);
	axis_taps(py, g.Y, &fy, &iy, &y0, &y1);
	axis_taps(pz, g.Z, &fz, &iz, &z0, &z1);
	const O X = (O)g.X;
	const O r0 = (O)y0 * X, r1 = (O)y1 * X;
	const O p0 = IS3D ? (O)z0 * g.plane : (O)0, p1 = IS3D ? (O)z1 * g.plane : (O)0;
	const O xb = (O)min(max(ix, 0), max(g.X - 2, 0));                   // where the pair starts in its row
	const O xa = (O)x0, xc = (O)x1;
#pragma unroll
	for (int a = 0; a < 3; ++a) {
		const O base = (O)a * g.stride;
		// (the pair of the field's very last cell starts one cell early: a row of one cell, X = 1, has no second cell of its own)
		const O c00 = base + p0 + r0, c01 = base + p0 + r1, c10 = base + p1 + r0, c11 = base + p1 + r1;
		const O b00 = min(c00 + xb, g.last_pair), b01 = min(c01 + xb, g.last_pair);
		const float2 v00 = Pair<HALF>::ld(vel, b00), v01 = Pair<HALF>::ld(vel, b01);
		const float t000 = c00 + xa == b00 ? v00.x : v00.y, t100 = c00 + xc == b00 ? v00.x : v00.y;
		const float t010 = c01 + xa == b01 ? v01.x : v01.y, t110 = c01 + xc == b01 ? v01.x : v01.y;
		if (IS3D) {
			const O b10 = min(c10 + xb, g.last_pair), b11 = min(c11 + xb, g.last_pair);
			const float2 v10 = Pair<HALF>::ld(vel, b10), v11 = Pair<HALF>::ld(vel, b11);
			const float t001 = c10 + xa == b10 ? v10.x : v10.y, t101 = c10 + xc == b10 ? v10.x : v10.y;
			const float t011 = c11 + xa == b11 ? v11.x : v11.y, t111 = c11 + xc == b11 ? v11.x : v11.y;
			u[a] = lerpf(lerpf(lerpf(t000, t100, fx), lerpf(t010, t110, fx), fy), lerpf(lerpf(t001, t101, fx), lerpf(t011, t111, fx), fy), fz);
		} else {
			const float c = lerpf(lerpf(t000, t100, fx), lerpf(t010, t110, fx), fy);
			u[a] = lerpf(c, c, fz);
		}
	}
}

template <typename O> __device__ __forceinline__ Grid<O> grid_of(const Geom& g)
{
	Grid<O> r;
	r.X = g.X; r.Y = g.Y; r.Z = g.Zg;
	r.plane = (O)g.X * (O)g.Y;
	r.stride = r.plane * (O)g.Zg;                                       // a whole grid: no halo planes
	r.last_pair = (O)3 * r.stride - (O)2;
	return r;
}

}  // namespace

struct ParticleArgs { float drift[3], lifetime, dt; unsigned faces; };

template <bool HALF, bool IS3D, bool WIDE, int SCHEME>
__global__ __launch_bounds__(256) void k_move_particles(const Geom geo, const ParticleArgs a, const void* __restrict__ vel0, const uint8_t* __restrict__ code,
	float4* __restrict__ rec, unsigned count)
{
	typedef typename Off<WIDE>::T O;
	const unsigned i = blockIdx.x * (unsigned)PT_WG + threadIdx.x;
	if (i >= count) return;
	const float4 r = rec[i];
	if (!(r.w >= 0.0f)) return;                                         // dead (negative or NaN age): not a bit of it changes
	const Grid<O> g = grid_of<O>(geo);
	const char* v = static_cast<const char*>(vel0);
	const float dt = a.dt;

	float k[3];
	sample_u<HALF, IS3D, O>(v, g, r.x, r.y, r.z, k);
	k[0] = k[0] + a.drift[0]; k[1] = k[1] + a.drift[1]; k[2] = k[2] + a.drift[2];
	if (SCHEME == (int)FX_PARTICLE_MIDPOINT) {
		const float h = 0.5f * dt;
		const float mx = clamp01(fmaf(k[0], h, r.x)), my = clamp01(fmaf(k[1], h, r.y)), mz = clamp01(fmaf(k[2], h, r.z));
		sample_u<HALF, IS3D, O>(v, g, mx, my, mz, k);
		k[0] = k[0] + a.drift[0]; k[1] = k[1] + a.drift[1]; k[2] = k[2] + a.drift[2];
	}
	float qx = fmaf(k[0], dt, r.x), qy = fmaf(k[1], dt, r.y), qz = IS3D ? fmaf(k[2], dt, r.z) : r.z;

	// open walls (launch-uniform bits, the code byte's order): a record that crosses one leaves the box
	// (| and &, not || and &&: six compares and no branch)
	bool dead = ((qx < 0.0f) & ((a.faces & FX_WALL_X_LO) != 0)) | ((qx > 1.0f) & ((a.faces & FX_WALL_X_HI) != 0)) |
	            ((qy < 0.0f) & ((a.faces & FX_WALL_Y_LO) != 0)) | ((qy > 1.0f) & ((a.faces & FX_WALL_Y_HI) != 0));
	if (IS3D) dead = dead | ((qz < 0.0f) & ((a.faces & FX_WALL_Z_LO) != 0)) | ((qz > 1.0f) & ((a.faces & FX_WALL_Z_HI) != 0));
	// a closed wall holds it (+ 0.0f: whichever zero fmaxf picks of -0 and +0, +0 is stored)
	qx = clamp01(qx) + 0.0f; qy = clamp01(qy) + 0.0f;
	if (IS3D) qz = clamp01(qz) + 0.0f;

	if (code) {                                                         // a record does not enter a solid
		const int cx = cell_axis(qx, g.X), cy = cell_axis(qy, g.Y);
		const int cz = IS3D ? cell_axis(qz, g.Z) : 0;
		const size_t cell = ((size_t)cz * (size_t)g.Y + (size_t)cy) * (size_t)g.X + (size_t)cx;
		if (code[cell] & OB_SELF) { qx = r.x; qy = r.y; qz = r.z; }
	}
	const float age1 = r.w + dt;
	if (a.lifetime > 0.0f && age1 >= a.lifetime) dead = true;
	rec[i] = make_float4(qx, qy, qz, dead ? -1.0f : age1);
}

template <bool HALF, bool IS3D, bool WIDE>
__global__ __launch_bounds__(256) void k_sample_velocity(const Geom geo, const void* __restrict__ vel0, const float4* __restrict__ pts, float* __restrict__ out,
	unsigned count)
{
	typedef typename Off<WIDE>::T O;
	const unsigned i = blockIdx.x * (unsigned)PT_WG + threadIdx.x;
	if (i >= count) return;
	const float4 p = pts[i];                                            // (w is not looked at: a particle buffer serves as it is)
	const Grid<O> g = grid_of<O>(geo);
	float u[3];
	sample_u<HALF, IS3D, O>(static_cast<const char*>(vel0), g, p.x, p.y, p.z, u);
	float* o = out + (size_t)i * 3;
	o[0] = u[0]; o[1] = u[1]; o[2] = u[2];
}

template <bool HALF, bool IS3D, bool WIDE>
static hipError_t launch_move_t(int scheme, dim3 grid, hipStream_t s, const Geom& g, const ParticleArgs& a, const void* vel0, const uint8_t* code,
	float4* rec, unsigned count)
{
	if (scheme == (int)FX_PARTICLE_MIDPOINT)
		hipLaunchKernelGGL((k_move_particles<HALF, IS3D, WIDE, (int)FX_PARTICLE_MIDPOINT>), grid, dim3(PT_WG), 0, s, g, a, vel0, code, rec, count);
	else
		hipLaunchKernelGGL((k_move_particles<HALF, IS3D, WIDE, (int)FX_PARTICLE_EULER>), grid, dim3(PT_WG), 0, s, g, a, vel0, code, rec, count);
	return hipGetLastError();
}

template <bool HALF, bool IS3D>
static hipError_t launch_move_w(bool wide, int scheme, dim3 grid, hipStream_t s, const Geom& g, const ParticleArgs& a, const void* vel0,
	const uint8_t* code, float4* rec, unsigned count)
{
	return wide ? launch_move_t<HALF, IS3D, true>(scheme, grid, s, g, a, vel0, code, rec, count)
	            : launch_move_t<HALF, IS3D, false>(scheme, grid, s, g, a, vel0, code, rec, count);
}

hipError_t launch_move_particles(const Geom& g, int half_store, const fx_particle_params& prm, const void* vel0, const uint8_t* code, unsigned faces,
	float dt, float* records, uint32_t count, hipStream_t s)
{
	if (!whole_grid(g)) return hipErrorNotSupported;                            // (fx_set_particles refuses slab ranks)
	if (!vel0 || !records || count > FX_MAX_PARTICLES) return hipErrorInvalidValue;
	if (prm.scheme != FX_PARTICLE_EULER && prm.scheme != FX_PARTICLE_MIDPOINT) return hipErrorInvalidValue;
	if (!open_faces_ok(g, faces)) return hipErrorInvalidValue;
	if (count == 0) return hipSuccess;
	const ParticleArgs a = { { prm.drift[0], prm.drift[1], prm.drift[2] }, prm.lifetime, dt, faces };
	const dim3 grid((count + PT_WG - 1) / PT_WG, 1, 1);
	const bool wide = colour_wants_wide_offsets(g);
	const bool is3d = g.Zg > 1;
	float4* rec = reinterpret_cast<float4*>(records);
	if (half_store) return is3d ? launch_move_w<true, true>(wide, (int)prm.scheme, grid, s, g, a, vel0, code, rec, count)
	                            : launch_move_w<true, false>(wide, (int)prm.scheme, grid, s, g, a, vel0, code, rec, count);
	return is3d ? launch_move_w<false, true>(wide, (int)prm.scheme, grid, s, g, a, vel0, code, rec, count)
	            : launch_move_w<false, false>(wide, (int)prm.scheme, grid, s, g, a, vel0, code, rec, count);
}

template <bool HALF, bool IS3D>
static hipError_t launch_sample_t(bool wide, dim3 grid, hipStream_t s, const Geom& g, const void* vel0, const float4* pts, float* out, unsigned count)
{
	if (wide) hipLaunchKernelGGL((k_sample_velocity<HALF, IS3D, true>), grid, dim3(PT_WG), 0, s, g, vel0, pts, out, count);
	else hipLaunchKernelGGL((k_sample_velocity<HALF, IS3D, false>), grid, dim3(PT_WG), 0, s, g, vel0, pts, out, count);
	return hipGetLastError();
}

hipError_t launch_sample_velocity(const Geom& g, int half_store, const void* vel0, const float* points, float* out, uint32_t count, hipStream_t s)
{
	if (!whole_grid(g)) return hipErrorNotSupported;
	if (!vel0 || !points || !out || count > FX_MAX_PARTICLES) return hipErrorInvalidValue;
	if (count == 0) return hipSuccess;
	const dim3 grid((count + PT_WG - 1) / PT_WG, 1, 1);
	const bool wide = colour_wants_wide_offsets(g);
	const bool is3d = g.Zg > 1;
	const float4* pts = reinterpret_cast<const float4*>(points);
	if (half_store) return is3d ? launch_sample_t<true, true>(wide, grid, s, g, vel0, pts, out, count) : launch_sample_t<true, false>(wide, grid, s, g, vel0, pts, out, count);
	return is3d ? launch_sample_t<false, true>(wide, grid, s, g, vel0, pts, out, count) : launch_sample_t<false, false>(wide, grid, s, g, vel0, pts, out, count);
}

}  // namespace fx
