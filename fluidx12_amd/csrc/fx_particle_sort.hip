// fx_particle_sort.hip -- the tracer particles sorted by cell, dead records last (fx_set_particle_sort, fx_sort_particles), gfx950.  No reference
// counterpart.  A stable least-significant-digit radix sort of (key, index) pairs, written with the HIP runtime alone; the 16-byte records are
// gathered once at the end.
//
// The rule (include/fluidx_hip.h states it, tests/particle_sort_ref.py restates it in numpy): a record (x, y, z, age) is live iff age >= 0, the
// move kernel's own test; its cell per axis is min((int)(c(p_a) * (float)N_a), N_a - 1), c and the formula being fx_particle_cell.h's, shared
// with k_move_particles' solid lookup (a 2-D grid's z cell is 0 by the same formula: (int)c(z) is 0 or 1, and N_z - 1 = 0); its key is
// (c_z Y + c_y) X + c_x, or X Y Z when it is dead.  The buffer becomes rec[order], order = the stable ascending permutation of the keys.
//
// Per pass (fx_particle_sort_plan.cpp decides digits, workgroups and the scan's shape):
//   k_psort_hist     every workgroup counts the digits of its kPsortRecords consecutive records in LDS -> hist[digit][workgroup]
//   k_psort_scan_*   the exclusive scan of that array in place: one launch while it fits one tile, else reduce / scan of block sums / apply
//   k_psort_scatter  every workgroup places its records: four rounds of 256 consecutive records, one per thread; a record's rank among the
//                    round's equal digits is its lane's count of lower lanes with the same digit (eight ballots) plus the counts of the
//                    lower waves (LDS, one writer per wave and digit); the workgroup's running base per digit is carried from round to round
// The first pass forms keys from the records (twice: in the histogram and in the scatter; a key is a few instructions, a key array written and
// read back is 8 bytes per record) and indices from positions.  The last pass writes its indices into `order`.
//   k_psort_gather   scratch[i] = rec[order[i]], and `live` = the position behind the last live key (one thread finds the boundary)
// and a device-to-device copy puts the sorted set back where the caller's pointer looks for it.
//
// Determinism is structural: no atomic decides a position.  The only atomics are the LDS counters of k_psort_hist, whose sums do not depend on
// arrival order.  Bounds: keys come from clamped values alone, so every digit is below the histogram's extent; a position is a sum of counts of
// the same keys, below `count` whenever the buffer held still between the histogram and the scatter -- and tested against `count` before the
// store in case a caller's kernel raced with the sort; an index read back from scratch is clamped before it addresses a record.
//
// Bytes per record, P passes: first pass 2 x 16 read, 8 written; every later pass 4 + 8 read, 8 written; gather 8 + 16 read, 16 written; copy
// 16 + 16.  P = 4 (256^3): 172 bytes per record, of which only the gather's 16-byte read is scattered.
#include "fx_internal.h"
#include "fx_particle_cell.h"

namespace fx {

namespace {

struct KeyGrid { int X, Y, Z; unsigned cells; };

__device__ __forceinline__ unsigned key_of(const float4 r, const KeyGrid g)
{
	if (!(r.w >= 0.0f)) return g.cells;                                 // dead (negative or NaN age): behind every live key
	const unsigned cx = (unsigned)cell_axis(clamp01(r.x), g.X), cy = (unsigned)cell_axis(clamp01(r.y), g.Y), cz = (unsigned)cell_axis(clamp01(r.z), g.Z);
	return (cz * (unsigned)g.Y + cy) * (unsigned)g.X + cx;
}

// exclusive scan of one value per thread over the 256 threads of a workgroup; *total = the sum.  sh: 256 words, free again on return
__device__ __forceinline__ unsigned block_scan(unsigned v, unsigned* sh, unsigned* total)
{
	const unsigned t = threadIdx.x;
	sh[t] = v;
	__syncthreads();
#pragma unroll
	for (unsigned off = 1; off < kPsortThreads; off <<= 1) {
		const unsigned a = t >= off ? sh[t - off] : 0u;
		__syncthreads();
		sh[t] += a;
		__syncthreads();
	}
	const unsigned incl = sh[t];
	*total = sh[kPsortThreads - 1];
	__syncthreads();
	return incl - v;
}

}  // namespace

template <bool FIRST>
__global__ __launch_bounds__(256) void k_psort_hist(const float4* __restrict__ rec, const unsigned* __restrict__ keys, const KeyGrid g, unsigned count,
	unsigned shift, unsigned dbits, unsigned nwg, unsigned* __restrict__ hist)
{
	__shared__ unsigned cnt[1u << kPsortDigitBits];
	const unsigned t = threadIdx.x, wg = blockIdx.x, nb = 1u << dbits, mask = nb - 1u;
	cnt[t] = 0u;
	__syncthreads();
#pragma unroll
	for (unsigned c = 0; c < kPsortItems; ++c) {
		const unsigned i = wg * kPsortRecords + c * kPsortThreads + t;
		if (i < count) {
			const unsigned k = FIRST ? key_of(rec[i], g) : keys[i];
			atomicAdd(&cnt[(k >> shift) & mask], 1u);                   // (LDS, integer: the sum is the same in any order)
		}
	}
	__syncthreads();
	if (t < nb) hist[t * nwg + wg] = cnt[t];
}

// the three kernels of the scan over n = (1 << dbits) * nwg entries, tiles of kPsortScanTile: eight consecutive entries per thread
__global__ __launch_bounds__(256) void k_psort_scan_reduce(const unsigned* __restrict__ a, unsigned n, unsigned* __restrict__ sums)
{
	__shared__ unsigned sh[kPsortThreads];
	const unsigned base = blockIdx.x * kPsortScanTile + threadIdx.x * 8u;
	unsigned v = 0u;
#pragma unroll
	for (unsigned j = 0; j < 8; ++j) if (base + j < n) v += a[base + j];
	unsigned total;
	(void)block_scan(v, sh, &total);
	if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

__global__ __launch_bounds__(256) void k_psort_scan_sums(unsigned* __restrict__ sums, unsigned n)
{
	__shared__ unsigned sh[kPsortThreads];
	unsigned carry = 0u;
	for (unsigned base = 0; base < n; base += kPsortThreads) {          // (n is launch-uniform: every thread takes every round)
		const unsigned i = base + threadIdx.x;
		const unsigned v = i < n ? sums[i] : 0u;
		unsigned total;
		const unsigned ex = block_scan(v, sh, &total);
		if (i < n) sums[i] = carry + ex;
		carry += total;
	}
}

// sums: the scanned block sums, or null when one tile holds the whole array
__global__ __launch_bounds__(256) void k_psort_scan_apply(unsigned* __restrict__ a, unsigned n, const unsigned* __restrict__ sums)
{
	__shared__ unsigned sh[kPsortThreads];
	const unsigned base = blockIdx.x * kPsortScanTile + threadIdx.x * 8u;
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
}

template <bool FIRST>
__global__ __launch_bounds__(256) void k_psort_scatter(const float4* __restrict__ rec, const unsigned* __restrict__ keys_in, const unsigned* __restrict__ idx_in,
	const KeyGrid g, unsigned count, unsigned shift, unsigned dbits, unsigned nwg, const unsigned* __restrict__ offs,
	unsigned* __restrict__ keys_out, unsigned* __restrict__ idx_out)
{
	const unsigned WAVES = kPsortThreads / 64u;
	__shared__ unsigned base[1u << kPsortDigitBits];                    // where the workgroup's next record of each digit goes
	__shared__ unsigned wcnt[WAVES][1u << kPsortDigitBits];             // this round's count per wave and digit
	const unsigned t = threadIdx.x, wg = blockIdx.x, lane = t & 63u, w = t >> 6, nb = 1u << dbits, mask = nb - 1u;
	base[t] = t < nb ? offs[t * nwg + wg] : 0u;
#pragma unroll
	for (unsigned ww = 0; ww < WAVES; ++ww) wcnt[ww][t] = 0u;
	unsigned k[kPsortItems], v[kPsortItems];
#pragma unroll
	for (unsigned c = 0; c < kPsortItems; ++c) {                        // all loads of the workgroup's records up front
		const unsigned i = wg * kPsortRecords + c * kPsortThreads + t;
		k[c] = 0u; v[c] = 0u;
		if (i < count) {
			k[c] = FIRST ? key_of(rec[i], g) : keys_in[i];
			v[c] = FIRST ? i : idx_in[i];
		}
	}
	__syncthreads();
	const unsigned long long below = (1ull << lane) - 1ull;
#pragma unroll
	for (unsigned c = 0; c < kPsortItems; ++c) {                        // (no thread leaves early: every wave takes every ballot and barrier)
		const bool valid = wg * kPsortRecords + c * kPsortThreads + t < count;
		const unsigned d = (k[c] >> shift) & mask;
		unsigned long long same = __ballot(valid);                      // the lanes of this wave that hold a record with the digit d
#pragma unroll
		for (unsigned b = 0; b < kPsortDigitBits; ++b) {
			const bool bit = (d >> b) & 1u;
			const unsigned long long has = __ballot(bit);
			same &= bit ? has : ~has;
		}
		const unsigned rank = (unsigned)__popcll(same & below);         // buffer order inside the wave is lane order
		if (valid && rank == 0u) wcnt[w][d] = (unsigned)__popcll(same); // one writer per wave and digit
		__syncthreads();
		if (valid) {
			unsigned pos = base[d] + rank;
#pragma unroll
			for (unsigned ww = 0; ww + 1 < WAVES; ++ww) if (ww < w) pos += wcnt[ww][d];
			if (pos < count) { keys_out[pos] = k[c]; idx_out[pos] = v[c]; }
		}
		__syncthreads();
		unsigned sum = 0u;
#pragma unroll
		for (unsigned ww = 0; ww < WAVES; ++ww) { sum += wcnt[ww][t]; wcnt[ww][t] = 0u; }
		base[t] += sum;
		__syncthreads();
	}
}

__global__ __launch_bounds__(256) void k_psort_gather(const float4* __restrict__ rec, const unsigned* __restrict__ order, const unsigned* __restrict__ keys,
	unsigned cells, unsigned count, float4* __restrict__ out, unsigned* __restrict__ live)
{
	const unsigned i = blockIdx.x * kPsortThreads + threadIdx.x;
	if (i >= count) return;
	out[i] = rec[min(order[i], count - 1u)];
	// the keys are sorted: the live ones end where the first key `cells` stands
	if (keys[i] < cells) {
		if (i + 1u == count || keys[i + 1u] >= cells) *live = i + 1u;
	} else if (i == 0u) {
		*live = 0u;
	}
}

hipError_t launch_particle_sort(const Geom& g, const PsortPlan& p, float* records, void* scratch, hipStream_t s)
{
	if (!whole_grid(g)) return hipErrorNotSupported;
	if (!records || !scratch || p.count == 0 || p.count > kPsortMaxCount || p.passes == 0 || p.passes > kPsortMaxPasses) return hipErrorInvalidValue;
	if ((uint64_t)g.X * (uint64_t)g.Y * (uint64_t)g.Zg != (uint64_t)p.cells || p.wgs != (p.count + kPsortRecords - 1) / kPsortRecords) return hipErrorInvalidValue;
	char* m = static_cast<char*>(scratch);
	unsigned* live = reinterpret_cast<unsigned*>(m + p.off_live);
	unsigned* idx[2] = { reinterpret_cast<unsigned*>(m + p.off_order), reinterpret_cast<unsigned*>(m + p.off_index) };
	unsigned* keys[2] = { reinterpret_cast<unsigned*>(m + p.off_keys[0]), reinterpret_cast<unsigned*>(m + p.off_keys[1]) };
	float4* tmp = reinterpret_cast<float4*>(m + p.off_records);
	unsigned* hist = reinterpret_cast<unsigned*>(m + p.off_hist);
	unsigned* sums = reinterpret_cast<unsigned*>(m + p.off_sums);
	const float4* rec = reinterpret_cast<const float4*>(records);
	const KeyGrid kg = { g.X, g.Y, g.Zg, p.cells };
	const dim3 wg(kPsortThreads), grid(p.wgs);
	for (uint32_t i = 0; i < p.passes; ++i) {
		const unsigned shift = p.shift[i], dbits = p.digit_bits[i], n = p.scan_entries[i], blocks = p.scan_blocks[i];
		if (dbits == 0 || dbits > kPsortDigitBits || n != (p.wgs << dbits) || blocks != (n + kPsortScanTile - 1) / kPsortScanTile) return hipErrorInvalidValue;
		const unsigned* kin = keys[(i + 1) & 1];                        // what pass i - 1 wrote
		unsigned* kout = keys[i & 1];
		unsigned* iout = idx[(p.passes - 1 - i) & 1];                   // the last pass writes `order`
		const unsigned* iin = idx[(p.passes - i) & 1];
		if (i == 0) hipLaunchKernelGGL((k_psort_hist<true>), grid, wg, 0, s, rec, kin, kg, p.count, shift, dbits, p.wgs, hist);
		else hipLaunchKernelGGL((k_psort_hist<false>), grid, wg, 0, s, rec, kin, kg, p.count, shift, dbits, p.wgs, hist);
		if (blocks > 1) {
			hipLaunchKernelGGL(k_psort_scan_reduce, dim3(blocks), wg, 0, s, hist, n, sums);
			hipLaunchKernelGGL(k_psort_scan_sums, dim3(1), wg, 0, s, sums, blocks);
			hipLaunchKernelGGL(k_psort_scan_apply, dim3(blocks), wg, 0, s, hist, n, (const unsigned*)sums);
		} else {
			hipLaunchKernelGGL(k_psort_scan_apply, dim3(1), wg, 0, s, hist, n, (const unsigned*)nullptr);
		}
		if (i == 0) hipLaunchKernelGGL((k_psort_scatter<true>), grid, wg, 0, s, rec, kin, iin, kg, p.count, shift, dbits, p.wgs, (const unsigned*)hist, kout, iout);
		else hipLaunchKernelGGL((k_psort_scatter<false>), grid, wg, 0, s, rec, kin, iin, kg, p.count, shift, dbits, p.wgs, (const unsigned*)hist, kout, iout);
		const hipError_t e = hipGetLastError();
		if (e != hipSuccess) return e;
	}
	hipLaunchKernelGGL(k_psort_gather, dim3((p.count + kPsortThreads - 1) / kPsortThreads), wg, 0, s, rec, (const unsigned*)idx[0],
		(const unsigned*)keys[(p.passes - 1) & 1], p.cells, p.count, tmp, live);
	hipError_t e = hipGetLastError();
	if (e != hipSuccess) return e;
	return hipMemcpyAsync(records, tmp, (size_t)p.count * 16, hipMemcpyDeviceToDevice, s);
}

}  // namespace fx
