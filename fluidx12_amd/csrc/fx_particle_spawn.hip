// fx_particle_spawn.hip -- tracer particles born on the device (fx_set_particle_spawners, fx_spawn_particles), gfx950.  No reference counterpart.
// Up to FX_MAX_PARTICLE_SPAWNERS boxes and ellipsoids bear records at a rate; a birth takes a dead record's slot, so the set is a closed loop
// on the device: spawn -> move -> deposit -> die -> slot reused.
//
// The rule (include/fluidx_hip.h states it, tests/particle_spawn_ref.py restates it in numpy): per spawner a 2^-16 fraction accumulates
// rate * dt and its whole part is the step's births n_s; the births of a step are numbered j = 0 .. n - 1, spawner 0's first; birth j takes
// the j-th dead record (!(age >= 0), the move's test) of the buffer in index order, births beyond the D dead records are dropped; birth j of
// spawner s has the serial k = serial_s + (j - first_s), and its record is a function of (seed, s, k) alone: hashed words, no state.
//
//   k_spawn_count   a workgroup counts the dead among its kSpawnRecords consecutive records (ages only) -> counts[workgroup]
//   k_spawn_scan_*  the exclusive scan of counts in place and the total D: one launch while they fit one tile, else reduce / scan of the
//                   block sums / apply (the shape of fx_particle_sort.hip's scan)
//   k_spawn_tick    one wave: the accumulators tick, n_s, first_s, n, the serial bases of the step and min(n, D) are written, `dropped` and
//                   the serials advance
//   k_spawn_place   a workgroup whose exclusive base is >= min(n, D) returns before it loads a record; any other ranks its dead records in
//                   index order (a ballot per round of 256 records, the counts of the lower rounds and waves from LDS, as k_psort_scatter
//                   ranks equal digits), and every dead record of rank j < min(n, D) finds its spawner among the first_s, forms its record,
//                   looks up the obstacle code and stores 16 bytes
//
// Determinism is structural: no atomic decides a slot, no kernel waits for another workgroup.  The only atomics add to the `born` and
// `blocked` counters, once per wave; integer sums do not depend on order.  Bounds: a slot is an index this launch formed from blockIdx and
// threadIdx and tested against `count`; the obstacle cell comes from clamped coordinates; the spawner index is a count of at most 15 compares.
// A caller's kernel that changes ages between the count and the place can only make births land on other dead-or-alive slots below `count`.
// No scratch: the ball's eight tries are a loop over hashed words, no array.
#include "fx_internal.h"
#include "fx_particle_cell.h"

namespace fx {

namespace {

typedef unsigned long long u64;

const unsigned SP_WAVES = kSpawnThreads / 64u;
const unsigned SP_AGE_WORD = 24u;                                       // words 0 .. 23: eight tries of three offsets; 24: the age

__device__ __forceinline__ unsigned mix32(unsigned x)
{
	x ^= x >> 16; x *= 0x7feb352du;
	x ^= x >> 15; x *= 0x846ca68bu;
	x ^= x >> 16;
	return x;
}

// u(d) in [0, 1) and a(d) = fmaf(2, u(d), -1) in [-1, 1) of a birth whose (seed, s, k) are hashed into h2; both exact
__device__ __forceinline__ float unit_of(unsigned h2, unsigned d) { return (float)(mix32(h2 + 0x85ebca6bu * (d + 1u)) >> 8) * 0x1p-24f; }
__device__ __forceinline__ float sym_of(unsigned h2, unsigned d) { return fmaf(2.0f, unit_of(h2, d), -1.0f); }

// exclusive scan of one value per thread over the 256 threads of a workgroup; *total = the sum.  sh: 256 words, free again on return
__device__ __forceinline__ unsigned block_scan(unsigned v, unsigned* sh, unsigned* total)
{
	const unsigned t = threadIdx.x;
	sh[t] = v;
	__syncthreads();
#pragma unroll
	for (unsigned off = 1; off < kSpawnThreads; off <<= 1) {
		const unsigned a = t >= off ? sh[t - off] : 0u;
		__syncthreads();
		sh[t] += a;
		__syncthreads();
	}
	const unsigned incl = sh[t];
	*total = sh[kSpawnThreads - 1];
	__syncthreads();
	return incl - v;
}

__device__ __forceinline__ bool dead_at(const float4* __restrict__ rec, unsigned i, unsigned count)
{
	return i < count && !(reinterpret_cast<const float*>(rec)[(size_t)i * 4u + 3u] >= 0.0f);    // (the age alone: 4 of the record's 16 bytes)
}

struct SpawnGrid { int X, Y, Z; };

}  // namespace

__global__ __launch_bounds__(256) void k_spawn_count(const float4* __restrict__ rec, unsigned count, unsigned* __restrict__ counts)
{
	__shared__ unsigned wsum[SP_WAVES];
	const unsigned t = threadIdx.x, wg = blockIdx.x;
	unsigned n = 0u;
#pragma unroll
	for (unsigned c = 0; c < kSpawnItems; ++c)
		n += (unsigned)__popcll(__ballot(dead_at(rec, wg * kSpawnRecords + c * kSpawnThreads + t, count)));      // (wave-uniform)
	if ((t & 63u) == 0u) wsum[t >> 6] = n;
	__syncthreads();
	if (t == 0u) {
		unsigned sum = 0u;
#pragma unroll
		for (unsigned w = 0; w < SP_WAVES; ++w) sum += wsum[w];
		counts[wg] = sum;
	}
}

// the three kernels of the scan over the n workgroup counts, tiles of kSpawnScanTile: eight consecutive entries per thread
__global__ __launch_bounds__(256) void k_spawn_scan_reduce(const unsigned* __restrict__ a, unsigned n, unsigned* __restrict__ sums)
{
	__shared__ unsigned sh[kSpawnThreads];
	const unsigned base = blockIdx.x * kSpawnScanTile + threadIdx.x * 8u;
	unsigned v = 0u;
#pragma unroll
	for (unsigned j = 0; j < 8; ++j) if (base + j < n) v += a[base + j];
	unsigned total;
	(void)block_scan(v, sh, &total);
	if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

__global__ __launch_bounds__(256) void k_spawn_scan_sums(unsigned* __restrict__ sums, unsigned n, SpawnState* __restrict__ st)
{
	__shared__ unsigned sh[kSpawnThreads];
	unsigned carry = 0u;
	for (unsigned base = 0; base < n; base += kSpawnThreads) {          // (n is launch-uniform: every thread takes every round)
		const unsigned i = base + threadIdx.x;
		const unsigned v = i < n ? sums[i] : 0u;
		unsigned total;
		const unsigned ex = block_scan(v, sh, &total);
		if (i < n) sums[i] = carry + ex;
		carry += total;
	}
	if (threadIdx.x == 0) st->dead = carry;
}

// sums: the scanned block sums, or null when one tile holds the whole array -- its total is D then
__global__ __launch_bounds__(256) void k_spawn_scan_apply(unsigned* __restrict__ a, unsigned n, const unsigned* __restrict__ sums, SpawnState* __restrict__ st)
{
	__shared__ unsigned sh[kSpawnThreads];
	const unsigned base = blockIdx.x * kSpawnScanTile + threadIdx.x * 8u;
	unsigned e[8], v = 0u;
#pragma unroll
	for (unsigned j = 0; j < 8; ++j) { e[j] = base + j < n ? a[base + j] : 0u; v += e[j]; }
	unsigned total;
	unsigned run = block_scan(v, sh, &total) + (sums ? sums[blockIdx.x] : 0u);
#pragma unroll
	for (unsigned j = 0; j < 8; ++j) {
		if (base + j < n) a[base + j] = run;
		run += e[j];
	}
	if (!sums && threadIdx.x == 0) st->dead = total;
}

__global__ __launch_bounds__(64) void k_spawn_tick(SpawnState* __restrict__ st, unsigned nsp, float dt)
{
	__shared__ unsigned ns[FX_MAX_PARTICLE_SPAWNERS];
	const unsigned lane = threadIdx.x;
	if (lane < FX_MAX_PARTICLE_SPAWNERS) {
		unsigned n = 0u;
		if (lane < nsp) {
			const float w = fminf(st->site[lane].rate * dt, 67108864.0f);
			const u64 inc = (u64)llrintf(w * 65536.0f);
			const u64 acc = st->acc[lane] + inc;
			n = (unsigned)(acc >> 16);                                  // <= 2^26 + 1
			st->acc[lane] = acc & 0xFFFFull;
			const u64 serial = st->serial[lane];
			st->base[lane] = serial;
			st->serial[lane] = serial + (u64)n;                         // whether or not a birth finds a slot
		}
		ns[lane] = n;
	}
	__syncthreads();
	if (lane == 0u) {
		unsigned run = 0u;                                              // <= 16 (2^26 + 1)
		for (unsigned s = 0; s < FX_MAX_PARTICLE_SPAWNERS; ++s) { st->first[s] = run; run += ns[s]; }
		st->first[FX_MAX_PARTICLE_SPAWNERS] = run;
		const unsigned take = min(run, st->dead);
		st->take = take;
		st->dropped += (u64)(run - take);
	}
}

template <bool IS3D>
__global__ __launch_bounds__(256) void k_spawn_place(const SpawnGrid g, float4* __restrict__ rec, unsigned count, const unsigned* __restrict__ offs,
	SpawnState* __restrict__ st, const uint8_t* __restrict__ code)
{
	__shared__ unsigned wcnt[kSpawnItems][SP_WAVES];
	__shared__ unsigned first[FX_MAX_PARTICLE_SPAWNERS + 1];
	const unsigned t = threadIdx.x, wg = blockIdx.x, lane = t & 63u, w = t >> 6;
	const unsigned take = st->take, base = offs[wg];
	if (base >= take) return;                                           // (uniform over the workgroup: nobody is left at a barrier)
	if (t <= FX_MAX_PARTICLE_SPAWNERS) first[t] = st->first[t];
	u64 b[kSpawnItems];
#pragma unroll
	for (unsigned c = 0; c < kSpawnItems; ++c) {
		b[c] = __ballot(dead_at(rec, wg * kSpawnRecords + c * kSpawnThreads + t, count));
		if (lane == 0u) wcnt[c][w] = (unsigned)__popcll(b[c]);
	}
	__syncthreads();
	const u64 below = (1ull << lane) - 1ull;
	unsigned run = base, born = 0u, blocked = 0u;
#pragma unroll
	for (unsigned c = 0; c < kSpawnItems; ++c) {
		unsigned j = run + (unsigned)__popcll(b[c] & below);            // buffer order: rounds, then waves, then lanes
#pragma unroll
		for (unsigned ww = 0; ww < SP_WAVES; ++ww) { if (ww < w) j += wcnt[c][ww]; run += wcnt[c][ww]; }
		const unsigned i = wg * kSpawnRecords + c * kSpawnThreads + t;
		const bool mine = ((b[c] >> lane) & 1ull) != 0ull && j < take && i < count;
		bool stored = false, solid = false;
		if (mine) {
			unsigned s = 0u;
#pragma unroll
			for (unsigned q = 1; q < FX_MAX_PARTICLE_SPAWNERS; ++q) s += j >= first[q] ? 1u : 0u;     // (first_q = n > j behind the last spawner)
			const SpawnSite site = st->site[s];
			const u64 k = st->base[s] + (u64)(j - first[s]);
			const unsigned h0 = mix32(site.seed + 0x9e3779b9u * (s + 1u));
			const unsigned h1 = mix32(h0 ^ (unsigned)k);
			const unsigned h2 = mix32(h1 ^ (unsigned)(k >> 32));
			float ax, ay, az;
			if (site.shape == FX_SPAWN_BALL) {
				ax = 0.0f; ay = 0.0f; az = 0.0f;
				for (unsigned tr = 0; tr < 8u; ++tr) {
					const float tx = sym_of(h2, 3u * tr), ty = sym_of(h2, 3u * tr + 1u), tz = IS3D ? sym_of(h2, 3u * tr + 2u) : 0.0f;
					if (fmaf(tz, tz, fmaf(ty, ty, tx * tx)) <= 1.0f) { ax = tx; ay = ty; az = tz; break; }
				}
			} else {
				ax = sym_of(h2, 0u); ay = sym_of(h2, 1u); az = IS3D ? sym_of(h2, 2u) : 0.0f;
			}
			const float px = clamp01(fmaf(ax, site.half[0], site.center[0])) + 0.0f;
			const float py = clamp01(fmaf(ay, site.half[1], site.center[1])) + 0.0f;
			const float pz = clamp01(fmaf(az, site.half[2], site.center[2])) + 0.0f;
			const float age = unit_of(h2, SP_AGE_WORD) * site.age_spread;
			if (code) {
				const int cx = cell_axis(px, g.X), cy = cell_axis(py, g.Y);
				const int cz = IS3D ? cell_axis(pz, g.Z) : 0;
				const size_t cell = ((size_t)cz * (size_t)g.Y + (size_t)cy) * (size_t)g.X + (size_t)cx;
				solid = (code[cell] & OB_SELF) != 0;
			}
			if (!solid) { rec[i] = make_float4(px, py, pz, age); stored = true; }
		}
		born += (unsigned)__popcll(__ballot(stored));
		blocked += (unsigned)__popcll(__ballot(solid));
	}
	if (lane == 0u) {                                                   // (integer adds: the sums are the same in any order)
		if (born) atomicAdd(&st->born, (u64)born);
		if (blocked) atomicAdd(&st->blocked, (u64)blocked);
	}
}

SpawnPlan spawn_plan(uint32_t count)
{
	SpawnPlan p = {};
	p.count = count;
	p.wgs = (count + kSpawnRecords - 1) / kSpawnRecords;                // (count <= 2^26: 65 536 at the most)
	p.scan_blocks = (p.wgs + kSpawnScanTile - 1) / kSpawnScanTile;
	const size_t al = 256;
	size_t off = (sizeof(SpawnState) + al - 1) / al * al;
	p.off_counts = off; off += ((size_t)p.wgs * 4 + al - 1) / al * al;
	p.off_sums = off;   off += ((size_t)p.scan_blocks * 4 + al - 1) / al * al;
	p.bytes = off;
	return p;
}

hipError_t launch_spawn_particles(const Geom& g, const SpawnPlan& p, uint32_t spawners, float dt, float* records, const uint8_t* code, void* mem, hipStream_t s)
{
	if (!whole_grid(g)) return hipErrorNotSupported;                            // (fx_set_particle_spawners refuses slab ranks)
	if (!records || !mem || p.count == 0 || p.count > FX_MAX_PARTICLES || spawners == 0 || spawners > FX_MAX_PARTICLE_SPAWNERS) return hipErrorInvalidValue;
	if (p.wgs != (p.count + kSpawnRecords - 1) / kSpawnRecords || p.scan_blocks != (p.wgs + kSpawnScanTile - 1) / kSpawnScanTile) return hipErrorInvalidValue;
	char* m = static_cast<char*>(mem);
	SpawnState* st = reinterpret_cast<SpawnState*>(m);
	unsigned* counts = reinterpret_cast<unsigned*>(m + p.off_counts);
	unsigned* sums = reinterpret_cast<unsigned*>(m + p.off_sums);
	float4* rec = reinterpret_cast<float4*>(records);
	const dim3 wg(kSpawnThreads), grid(p.wgs);
	hipLaunchKernelGGL(k_spawn_count, grid, wg, 0, s, (const float4*)rec, p.count, counts);
	if (p.scan_blocks > 1) {
		hipLaunchKernelGGL(k_spawn_scan_reduce, dim3(p.scan_blocks), wg, 0, s, (const unsigned*)counts, p.wgs, sums);
		hipLaunchKernelGGL(k_spawn_scan_sums, dim3(1), wg, 0, s, sums, p.scan_blocks, st);
		hipLaunchKernelGGL(k_spawn_scan_apply, dim3(p.scan_blocks), wg, 0, s, counts, p.wgs, (const unsigned*)sums, st);
	} else {
		hipLaunchKernelGGL(k_spawn_scan_apply, dim3(1), wg, 0, s, counts, p.wgs, (const unsigned*)nullptr, st);
	}
	hipLaunchKernelGGL(k_spawn_tick, dim3(1), dim3(64), 0, s, st, spawners, dt);
	const SpawnGrid sg = { g.X, g.Y, g.Zg };
	if (g.Zg > 1) hipLaunchKernelGGL((k_spawn_place<true>), grid, wg, 0, s, sg, rec, p.count, (const unsigned*)counts, st, code);
	else hipLaunchKernelGGL((k_spawn_place<false>), grid, wg, 0, s, sg, rec, p.count, (const unsigned*)counts, st, code);
	return hipGetLastError();
}

}  // namespace fx
