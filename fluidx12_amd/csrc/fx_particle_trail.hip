// fx_particle_trail.hip -- the particle trail (fx_set_particle_trail): the tracer particles as a source of smoke and heat, gfx950.  No reference
// counterpart.
//
//   k_trail_splat   every live record adds its 2^24 of integer weights to the uint64 accumulators of the eight cells around it
//   k_trail_apply   every cell with a non-zero accumulator adds to the colour (and the temperature) and clears its word
//
// A scatter from points into the grid, made reproducible the way fx_voxelize.hip makes its own: the scattered operation is an integer add,
// commutative and exact, so any order of arrival and any grouping gives the same words; the integers become floats once per cell.
//
// The rule, fp32, every operation rounded as written (include/fluidx_hip.h states it, tests/particle_trail_ref.py restates it in numpy),
// N = (X, Y, Z), c(v) = fminf(fmaxf(v, 0), 1) (fx_particle_cell.h):
//   scatter, per live record (age >= 0, the move's test) and axis a:  s = c(p_a), t = s * N_a - 0.5f, fl = floorf(t), f = t - fl;
//         q = (int)rintf(f * 256) in 0 .. 256; taps (int)fl and (int)fl + 1 clamped to [0, N_a - 1] -- the cells U(p) of fx_particles.hip reads --
//         with the weights 256 - q and q.  A 2-D grid does not look at z: one tap, plane 0, weight 256.
//         acc[cell] += w_x * w_y * w_z for the eight (four) tap combinations; adds of 0 are skipped; two taps that clamp onto one wall cell both add
//         to it: 2^24 per live record in total.  No value reaches an index unclamped
//   apply, per cell with acc != 0:  the word goes back to 0;  a solid cell (code bit 6) takes nothing;  otherwise A = (float)acc * 0x1p-24f,
//         g = rate * dt, colour_ch = fmaf(A, tint_ch * g, colour_ch), and with a temperature T = fmaf(A, heat * dt, T), in place
//         (fp16 storage: widened on load, rounded once, RNE, on store).  A cell with acc == 0 is not stored
//
// k_trail_splat: one lane per record, 256-thread workgroups, the record one 16-byte load, no LDS, no scratch; the adds are no-return 64-bit
// integer atomics (global_atomic_add_x2).  Atomics with one lane per row or with every adder on one address run an order of magnitude below
// the chip's rate, and a shuffled set and a nozzle are those two cases.  So the kernel merges before it adds: adjacent lanes of a wave that are
// live and have the same base cell -- the same (int)fl triple -- address the same eight cells; their weights are summed in the wave by a
// segmented scan (32-bit sums: 64 * 2^24 < 2^32) and the last lane of the run issues the eight atomics.  The scan stops at the first distance
// no run reaches, so a wave without runs pays one ballot.  A set sorted by cell (fx_particle_sort.hip) makes the runs long.  MERGE = false (the
// lab switch TRAIL_MERGE = 0): every lane adds its own eight weights.
// k_trail_apply: one launch over the grid, k_heat's 64 x 4 x 1 tiles; 8 bytes read per cell, everything else only where acc != 0.
// Fields are addressed as fx_store.h has it: 32-bit byte offsets while the colour field is under 4 GiB, 64-bit ones above (WIDE).
#include "fx_internal.h"
#include "fx_store.h"
#include "fx_particle_cell.h"

namespace fx {

using namespace sto;

namespace {

const int TR_WG = 256;
const int TR_X = kHeatTileX, TR_Y = kHeatTileY;

typedef unsigned long long u64;

// one axis of the scatter: the first tap before the clamp (-1 .. n - 1) and the weight of the second tap (0 .. 256)
__device__ __forceinline__ void axis_split(float p, int n, int* i0, int* q)
{
	const float s = clamp01(p);
	const float t = s * (float)n - 0.5f;
	const float fl = floorf(t);
	const float f = t - fl;
	*i0 = (int)fl;
	*q = (int)rintf(f * 256.0f);
}

__device__ __forceinline__ int clamp_tap(int i, int n) { return min(max(i, 0), n - 1); }

template <typename O> __device__ __forceinline__ void add_word(u64* acc, O cell, unsigned w)
{
	if (w) atomicAdd(reinterpret_cast<u64*>(reinterpret_cast<char*>(acc) + cell * (O)8), (u64)w);      // (the result is not used: no-return)
}

struct TrailArgs { float rate, dt, tint[4], heat; int tiles_x, tiles_y; };

}  // namespace

template <bool IS3D, bool WIDE, bool MERGE>
__global__ __launch_bounds__(256) void k_trail_splat(const Geom g, const float4* __restrict__ rec, unsigned count, u64* __restrict__ acc)
{
	typedef typename Off<WIDE>::T O;
	const int NW = IS3D ? 8 : 4;
	const unsigned i = blockIdx.x * (unsigned)TR_WG + threadIdx.x;
	const bool in = i < count;
	const float4 r = in ? rec[i] : make_float4(0.0f, 0.0f, 0.0f, -1.0f);
	const bool live = r.w >= 0.0f;                                      // (a lane beyond the set is a dead record)
	if (!MERGE && !live) return;

	int ix, iy, iz = 0, qx, qy, qz = 0;
	axis_split(r.x, g.X, &ix, &qx);
	axis_split(r.y, g.Y, &iy, &qy);
	if (IS3D) axis_split(r.z, g.Zg, &iz, &qz);
	unsigned w[NW];
	{
		const unsigned x0 = live ? 256u - (unsigned)qx : 0u, x1 = live ? (unsigned)qx : 0u;
		const unsigned y0 = 256u - (unsigned)qy, y1 = (unsigned)qy;
		w[0] = x0 * y0; w[1] = x1 * y0; w[2] = x0 * y1; w[3] = x1 * y1;
		if (IS3D) {
			const unsigned z0 = 256u - (unsigned)qz, z1 = (unsigned)qz;
#pragma unroll
			for (int k = 0; k < 4; ++k) { w[4 + k] = w[k] * z1; w[k] = w[k] * z0; }
		} else {
#pragma unroll
			for (int k = 0; k < 4; ++k) w[k] = w[k] * 256u;
		}
	}

	if (MERGE) {
		// ---- runs of adjacent live lanes with one base cell: the weights summed in the wave, the run's last lane adds
		const int lane = (int)(threadIdx.x & 63u);
		const int px = __shfl_up(ix, 1), py = __shfl_up(iy, 1), pz = __shfl_up(iz, 1);
		const int pl = __shfl_up((int)live, 1);
		const bool head = lane == 0 || !live || !pl || px != ix || py != iy || pz != iz;
		const u64 heads = __builtin_amdgcn_ballot_w64(head);                // (every lane of the wave is here: bit 0 is set)
		const int first = 63 - __builtin_clzll(heads & (~0ull >> (63 - lane)));
		const int dist = lane - first;                                      // lanes between this one and its run's head
		for (int d = 1; d < 64; d <<= 1) {
			if (__builtin_amdgcn_ballot_w64(dist >= d) == 0) break;         // no run reaches this far: uniform over the wave
#pragma unroll
			for (int k = 0; k < NW; ++k) {
				const unsigned u = (unsigned)__shfl_up((int)w[k], d);
				if (dist >= d) w[k] += u;
			}
		}
		const bool tail = lane == 63 || ((heads >> (lane + 1)) & 1ull) != 0;
		if (!live || !tail) return;
	}

	const O X = (O)g.X, plane = (O)g.X * (O)g.Y;
	const O x0 = (O)clamp_tap(ix, g.X), x1 = (O)clamp_tap(ix + 1, g.X);
	const O r0 = (O)clamp_tap(iy, g.Y) * X, r1 = (O)clamp_tap(iy + 1, g.Y) * X;
	const O p0 = IS3D ? (O)clamp_tap(iz, g.Zg) * plane : (O)0;
	add_word<O>(acc, p0 + r0 + x0, w[0]);
	add_word<O>(acc, p0 + r0 + x1, w[1]);
	add_word<O>(acc, p0 + r1 + x0, w[2]);
	add_word<O>(acc, p0 + r1 + x1, w[3]);
	if (IS3D) {
		const O p1 = (O)clamp_tap(iz + 1, g.Zg) * plane;
		add_word<O>(acc, p1 + r0 + x0, w[4]);
		add_word<O>(acc, p1 + r0 + x1, w[5]);
		add_word<O>(acc, p1 + r1 + x0, w[6]);
		add_word<O>(acc, p1 + r1 + x1, w[7]);
	}
}

template <bool HALF, bool WIDE>
__global__ __launch_bounds__(256) void k_trail_apply(const Geom g, const TrailArgs a, u64* __restrict__ acc, void* __restrict__ col, float* __restrict__ temp,
	float* __restrict__ alpha, const uint8_t* __restrict__ code)
{
	typedef Cell<HALF> Ce;
	typedef typename Off<WIDE>::T O;
	int bid = (int)blockIdx.x;
	const int tile_x = bid % a.tiles_x; bid /= a.tiles_x;
	const int tile_y = bid % a.tiles_y;
	const int x = tile_x * TR_X + (int)threadIdx.x, y = tile_y * TR_Y + (int)threadIdx.y, z = bid / a.tiles_y;
	if (x >= g.X || y >= g.Y) return;
	const O id = (O)z * ((O)g.X * (O)g.Y) + (O)y * (O)g.X + (O)x;
	u64* word = reinterpret_cast<u64*>(reinterpret_cast<char*>(acc) + id * (O)8);
	const u64 v = *word;
	if (v == 0) return;                                                 // no particle near: the cell keeps its bits
	*word = 0;
	if (code != nullptr && (code[id] & OB_SELF) != 0) return;               // a solid cell takes nothing
	const float A = (float)v * 0x1p-24f;
	const float gdt = a.rate * a.dt;
	char* co = static_cast<char*>(col);
	const float4 c4 = Ce::ld4(co, id);
	const float c[4] = { fmaf(A, a.tint[0] * gdt, c4.x), fmaf(A, a.tint[1] * gdt, c4.y), fmaf(A, a.tint[2] * gdt, c4.z), fmaf(A, a.tint[3] * gdt, c4.w) };
	const float stored_alpha = Ce::st4(co, id, c);
	if (alpha) *reinterpret_cast<float*>(reinterpret_cast<char*>(alpha) + id * (O)4) = stored_alpha;
	if (temp) {
		float* t = reinterpret_cast<float*>(reinterpret_cast<char*>(temp) + id * (O)4);
		*t = fmaf(A, a.heat * a.dt, *t);
	}
}

template <bool IS3D, bool WIDE>
static hipError_t launch_splat_t(bool merge, dim3 grid, hipStream_t s, const Geom& g, const float4* rec, unsigned count, u64* acc)
{
	if (merge) hipLaunchKernelGGL((k_trail_splat<IS3D, WIDE, true>), grid, dim3(TR_WG), 0, s, g, rec, count, acc);
	else hipLaunchKernelGGL((k_trail_splat<IS3D, WIDE, false>), grid, dim3(TR_WG), 0, s, g, rec, count, acc);
	return hipGetLastError();
}

hipError_t launch_trail_splat(const Geom& g, const float* records, uint32_t count, unsigned long long* acc, hipStream_t s)
{
	if (!whole_grid(g)) return hipErrorNotSupported;                            // (fx_set_particle_trail refuses slab ranks)
	if (!records || !acc || count > FX_MAX_PARTICLES) return hipErrorInvalidValue;
	if (count == 0) return hipSuccess;
	const dim3 grid((count + TR_WG - 1) / TR_WG, 1, 1);
	const bool wide = colour_wants_wide_offsets(g);
	const bool merge = FX_KNOB_INT("TRAIL_MERGE", 1) != 0;                      // (a lab switch: the shipped library always merges)
	const float4* rec = reinterpret_cast<const float4*>(records);
	if (g.Zg > 1) return wide ? launch_splat_t<true, true>(merge, grid, s, g, rec, count, acc) : launch_splat_t<true, false>(merge, grid, s, g, rec, count, acc);
	return wide ? launch_splat_t<false, true>(merge, grid, s, g, rec, count, acc) : launch_splat_t<false, false>(merge, grid, s, g, rec, count, acc);
}

template <bool HALF>
static hipError_t launch_apply_t(bool wide, dim3 grid, dim3 block, hipStream_t s, const Geom& g, const TrailArgs& a, u64* acc, void* col, float* temp,
	float* alpha, const uint8_t* code)
{
	if (wide) hipLaunchKernelGGL((k_trail_apply<HALF, true>), grid, block, 0, s, g, a, acc, col, temp, alpha, code);
	else hipLaunchKernelGGL((k_trail_apply<HALF, false>), grid, block, 0, s, g, a, acc, col, temp, alpha, code);
	return hipGetLastError();
}

hipError_t launch_trail_apply(const Geom& g, int half_store, const fx_particle_trail& t, float dt, unsigned long long* acc, void* col, float* temp,
	float* alpha, const uint8_t* code, hipStream_t s)
{
	if (!whole_grid(g)) return hipErrorNotSupported;
	if (!acc || !col) return hipErrorInvalidValue;
	TrailArgs a = { t.rate, dt, { t.tint[0], t.tint[1], t.tint[2], t.tint[3] }, t.heat, (g.X + TR_X - 1) / TR_X, (g.Y + TR_Y - 1) / TR_Y };
	const size_t wgs = (size_t)a.tiles_x * (size_t)a.tiles_y * (size_t)g.Zg;
	if (wgs == 0 || wgs > 0x7FFFFFFFu) return hipErrorInvalidValue;
	const dim3 grid((unsigned)wgs, 1, 1), block(TR_X, TR_Y, 1);
	const bool wide = colour_wants_wide_offsets(g);
	return half_store ? launch_apply_t<true>(wide, grid, block, s, g, a, acc, col, temp, alpha, code)
	                  : launch_apply_t<false>(wide, grid, block, s, g, a, acc, col, temp, alpha, code);
}

}  // namespace fx
