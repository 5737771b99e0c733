// fx_particle_sort_plan.cpp -- the host side of the particle sort (fx_particle_sort.hip): how many key bits a grid needs, how they split into
// digits, how many workgroups a pass launches, the shape of its scan and where each array lies in the scratch block.  Plain host code: no device,
// no HIP call (tests/test_particle_sort_ref.py links it into a small program, also under the address and undefined-behaviour sanitizers).
#include "fx_particle_sort_plan.h"

namespace fx {

namespace {
size_t align_up(size_t v) { return (v + kPsortAlign - 1) / kPsortAlign * kPsortAlign; }
}  // namespace

int psort_plan(uint64_t cells, uint32_t count, int force_bits, PsortPlan* out)
{
	if (!out || cells == 0 || cells >= 0xFFFFFFFFull || count > kPsortMaxCount) return -1;
	PsortPlan p = {};
	p.cells = (uint32_t)cells;
	p.count = count;
	uint32_t bits = 0;
	while (bits < 32 && (cells >> bits)) ++bits;                    // bit_length: the dead key, `cells` itself, has to fit
	if (force_bits > (int)bits) bits = force_bits > 32 ? 32u : (uint32_t)force_bits;
	p.bits = bits;
	// as few passes as the widest digit allows, the bits spread evenly over them (25 bits: 7 + 6 + 6 + 6): narrower digits scan less
	p.passes = (bits + kPsortDigitBits - 1) / kPsortDigitBits;
	uint32_t at = 0;
	for (uint32_t i = 0; i < p.passes; ++i) {
		p.digit_bits[i] = bits / p.passes + (i < bits % p.passes ? 1u : 0u);
		p.shift[i] = at;
		at += p.digit_bits[i];
	}
	p.records_per_wg = kPsortRecords;
	p.wgs = (count + kPsortRecords - 1) / kPsortRecords;            // (count <= 2^26: 65 536 at the most)
	uint32_t entries = 0, blocks = 0;
	for (uint32_t i = 0; i < p.passes; ++i) {
		p.scan_entries[i] = p.wgs << p.digit_bits[i];               // <= 2^24
		p.scan_blocks[i] = (p.scan_entries[i] + kPsortScanTile - 1) / kPsortScanTile;
		if (p.scan_entries[i] > entries) entries = p.scan_entries[i];
		if (p.scan_blocks[i] > blocks) blocks = p.scan_blocks[i];
	}
	size_t off = 0;
	const size_t words = align_up((size_t)count * 4);
	p.off_live = off;       off += kPsortAlign;
	p.off_order = off;      off += words;
	p.off_index = off;      off += words;
	p.off_keys[0] = off;    off += words;
	p.off_keys[1] = off;    off += words;
	p.off_records = off;    off += align_up((size_t)count * 16);
	p.off_hist = off;       off += align_up((size_t)entries * 4);
	p.off_sums = off;       off += align_up((size_t)blocks * 4);
	p.scratch_bytes = off;
	*out = p;
	return 0;
}

}  // namespace fx
