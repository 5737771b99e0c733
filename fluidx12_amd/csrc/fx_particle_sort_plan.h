// fx_particle_sort_plan.h -- the shape of one particle sort (fx_particle_sort.hip), decided on the host by fx_particle_sort_plan.cpp: key width,
// digits, launches and the layout of the scratch block.  Plain C++, no HIP: the kernels, the entry points (fx_stage_api.cpp) and the stand-alone
// planner test (tests/test_particle_sort_ref.py) all include it.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace fx {

const uint32_t kPsortThreads = 256;                           // threads of a histogram / scatter workgroup
const uint32_t kPsortItems = 4;                               // records each of them takes
const uint32_t kPsortRecords = kPsortThreads * kPsortItems;   // records per workgroup
const uint32_t kPsortDigitBits = 8;                           // the widest digit: the kernels hold a histogram of 1 << 8 counters
const uint32_t kPsortMaxPasses = 4;                           // 32 key bits at most
const uint32_t kPsortScanTile = 2048;                         // histogram entries one scan workgroup takes (256 threads x 8)
const uint32_t kPsortMaxCount = 1u << 26;                     // FX_MAX_PARTICLES
const size_t kPsortAlign = 256;                               // every array of the scratch block starts on a multiple of this

struct PsortPlan {
	uint32_t cells;                          // X * Y * Z: the key of a dead record, one above the largest live key
	uint32_t count;                          // records
	uint32_t bits;                           // key bits sorted: bit_length(cells), or more when forced
	uint32_t passes;                         // 1 .. kPsortMaxPasses
	uint32_t digit_bits[kPsortMaxPasses];    // per pass, least significant digit first; sum = bits, each 1 .. kPsortDigitBits
	uint32_t shift[kPsortMaxPasses];         // where the digit of a pass starts in the key
	uint32_t wgs;                            // workgroups of every histogram and scatter launch
	uint32_t records_per_wg;                 // kPsortRecords
	uint32_t scan_entries[kPsortMaxPasses];  // (1 << digit_bits) * wgs: the histogram a pass scans, laid out [digit][workgroup]
	uint32_t scan_blocks[kPsortMaxPasses];   // workgroups of its scan; 1: one launch, more: reduce, scan of the block sums, apply
	// the scratch block, byte offsets: live (one word), order and its ping-pong twin (count words each), two key arrays (count words each),
	// a record array (count x 16 bytes), the histogram (the largest scan_entries) and the scan's block sums (the largest scan_blocks)
	size_t off_live, off_order, off_index, off_keys[2], off_records, off_hist, off_sums;
	size_t scratch_bytes;
};

// 0, or -1 for what fx_set_particle_sort refuses: cells == 0, cells >= 2^32 - 1, count > kPsortMaxCount.  force_bits > bits of the grid (the lab
// switch PSORT_KEY_BITS): plan for that many key bits, 32 at the most.  count 0 plans the live word alone.
int psort_plan(uint64_t cells, uint32_t count, int force_bits, PsortPlan* out);

}  // namespace fx
