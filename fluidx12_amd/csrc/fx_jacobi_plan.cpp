// fx_jacobi_plan.cpp -- which kernel family runs a round of the fixed-count pressure solve, and with how many sweeps per launch.
// The ONE place that holds this policy: jacobi_policy is the table (geometry class x request -> families, sweeps per launch),
// jacobi_plan turns it into the launches of a round, launch_jacobi hands a planned launch to its family's launcher, jacobi_group_* is the form
// the overlapped slab schedule uses.  The families' own predicates (jacobi_*_supported) and launchers stay with their kernels.
// tests/test_jacobi_plan.py pins the schedule of some five thousand (geometry, request, switch, count) cases (tests/golden/jacobi_plan.json).
// The faithful solve's policy is here too (freeze_*, at the end): whether the sparse solver runs, how many strip launches follow the dense
// sweep, the launches of a solve and the cadence of the activity count; tests/test_freeze_plan.py pins it (tests/golden/freeze_plan.json).
#include "fx_internal.h"
#include <algorithm>

namespace fx {

// Precedence of what asks for a launch length: the context's jacobi_fuse flag > the JACOBI_T switch > the measured thresholds below
// (want == 0).  An explicit request is honoured as given: the preferences (three / four) apply to want == 0 only.
JacobiPolicy jacobi_policy(const Geom& g, int fuse, bool frozen, bool second_mask)
{
	JacobiPolicy p{ { JF_NONE, JF_SWEEP1, JF_NONE, JF_NONE, JF_NONE }, 1, 0, 0 };
	// 2-D grids relax on LDS tiles (fx_jacobi2d.hip), freeze bytes included where the mask has a second buffer to ping-pong with, unless the
	// caller asked for one sweep per launch (jacobi_fuse = 1: the plainest kernels, what the kernel-against-kernel parity tests compare with)
	if (jacobi2d_max_sweeps(g) > 0 && fuse != 1 && (!frozen || second_mask)) {
		for (int k = 1; k <= 4; ++k) p.fam[k] = JF_TILE2D;
		p.unit = jacobi2d_max_sweeps(g);
		return p;
	}
	if (frozen) return p;                                               // a byte mask: the generic kernel, one sweep per launch
	const int forced = FX_KNOB_INT("JACOBI_T", 0), want = std::min(fuse > 0 ? fuse : forced, 4), nzp = g.nz;
	const size_t cells = (size_t)g.X * g.Y * (size_t)nzp;
	const bool s3 = jacobi_strip3_supported(g), s4 = jacobi_strip4_supported(g);
	const bool wide = jacobi_strip_supported(g) && jacobi_strip_wide(g);   // X = 512, an even number of rows
	const bool narrow = g.Zg > 1 && (g.X == 64 || g.X == 128 || g.X == 256) && g.Y >= 16;
	if (s4) p.fam[4] = JF_STRIP4;                                       // fx_jacobi_strip4.hip: k_jacobi_strip4o (X = 256), 4x (512), 4t (x tiles: any other row of whole quads from 68 cells)
	const int four_asked = want >= 4 && s4 && nzp >= 2 ? 4 : 0;
	if (wide || narrow) {
		// ---- X = 512 | X = 64, 128, 256: the register strips (fx_jacobi_strip.hip: twos, X = 512 the wide kernel; threes in registers where the
		// lab asks for them), threes through the LDS (fx_jacobi_strip3.hip: X = 256, 512), X = 128 a 4 x 4-row block per wave (fx_jacobi_block.hip)
		// -- the strips have too few waves there.  (Round 6 built FOUR sweeps per launch on 8 x 8-row tiles for X = 128, a workgroup each with
		// the 16 x 16-row cone in its waves' registers and the planes handed over through the LDS: bit-exact, 24.9 us per launch against
		// 2 x 6.8 -- eight barrier phases on one workgroup per CU; docs/LAB.md section 12.  The LDS tile kernel k_jacobi_tb<T> of round 1 lost
		// to the register strips in every shape measured, profiles/archive/r01_jacobi_tile_sweep.txt, and was removed in round 3.)
		const bool block = narrow && jacobi_block2_supported(g);
		p.fam[2] = block ? JF_BLOCK2 : JF_STRIP;
		if (s3) p.fam[3] = narrow && FX_KNOB_INT("STRIP3_OFF", 0) ? JF_STRIP : JF_STRIP3;      // (STRIP3_OFF = 1: the all-register three-sweep strips)
		// where two sweeps per launch (register strips) beat one: measured on MI355X with the DPP lane shifts in place
		// (us per sweep, one / two sweeps per launch): 256^3 30 / 17.8, 512x512x64 41 / 18.9, 512x512x32 21.8 / 12.0, 512x512x16
		// 12.5 / 9.9, 256x256x64 10.0 / 9.0 -- but 256x256x32 6.2 / 8.2, 128^3 5.7 / 7.6, 128x128x32 3.3 / 7.8, 64^3 2.8 / 7.3: below
		// ~4 M cells a launch is too short for 8-plane z chunks to fill the chip.  The block kernel of X = 128 pays from two planes.
		const bool twos = block ? nzp >= 2 : cells >= ((size_t)7 << 19);                        // 3.5 M cells
		p.unit = four_asked ? 4 : want >= 3 && s3 ? 3 : want >= 2 ? 2 : want == 1 ? 1 : twos ? 2 : 1;
	} else {
		// ---- every other row: the general block-per-wave kernel, two sweeps per launch (fx_jacobi_block.hip; 150^3, the reference's GI preset:
		// 19.3 us per single-sweep launch before), as the default and for jacobi_fuse = 2 (the slab rounds).  A request this class has no kernel
		// for (3; 4 without the x tiles) runs ones, and so does everything under JACOBI_T (the ones are what that switch measures against).
		if (jacobi_blockg_supported(g) && !forced && nzp >= 2) p.fam[2] = JF_BLOCKG;
		p.unit = four_asked ? 4 : (fuse == 0 || fuse == 2) && p.fam[2] ? 2 : 1;
	}
	if (want) return p;
	// ---- the measured defaults of the serial rounds (single domain, and slab ranks thick enough)
	// THREE sweeps per launch (k_jacobi_strip3c / 3h) where that kernel exists and the grid is large enough, the remainder as two-sweep launches
	// (40 = 12 x 3 + 2 x 2).  Measured 256^3: Jacobi stage of the bench 0.664 ms against 0.714 ms in twos (15.0 against 14.3 G voxel-updates/s).
	// X = 256 (k_jacobi_strip3c): wherever the strips pay at all -- round 5, us per sweep in twos / threes / fours: 256 x 256 x 64 8.1 / 7.2 / 7.5,
	// x 96 9.0 / 7.8 / 7.9, x 128 10.8 / 8.9 / 8.9, x 192 14.2 / 11.3 / 11.1 (the 12.6 M-cell threshold dated from the kernel before the
	// cooperative pairs).  X = 512 (k_jacobi_strip3h): from 16.8 M cells since the round-2 hand-over order -- 512x512x64 (a rank of
	// BASELINE configs[3]) 18.7 against 19.5 us per sweep, 512x512x128 36.2 against 43.7, 512^3 117.6 against 152 (before: 20.3 / 39.6 / 129).
	// JACOBI_PREFER3=0 keeps two sweeps per launch throughout.
	p.three = FX_KNOB_INT("JACOBI_PREFER3", 1) && !FX_KNOB_INT("STRIP3_OFF", 0) && s3 && cells >= (g.X == 512 ? (size_t)1 << 24 : (size_t)7 << 19);
	// FOUR sweeps per launch where the kernels exist: 40 sweeps = 10 launches.  JACOBI_PREFER4=0 keeps the threes.
	size_t from;
	if (g.X == 512)
		// k_jacobi_strip4x from 96 planes; below, three x tiles of the octet (k_jacobi_strip4t) from SIX planes -- us per sweep at 512 x 512 x D,
		// the round-5 schedule (ones below 16 planes, twos) / fours: 4 6.9 / 9.6, 6 7.0 / 4.9, 8 7.7 / 4.9, 12 10.1 / 5.5, 16 10.2 / 6.3,
		// 32 12.2 / 9.3, 48 15.8 / 12.3 (rows the octet's bands cannot be placed on, Y = 15, 16: from 64 planes, k_jacobi_strip4x)
		from = g.Y >= 17 ? (size_t)3 << 19 : (size_t)1 << 24;
	else if (g.X == 256)
		// the octet kernel (k_jacobi_strip4o, the default) -- round 5, us per sweep at 256 x 256 x D in ones / twos / threes / fours: D = 24
		// 5.7 / 7.4 / 6.8 / 5.3, 32 6.2 / 7.7 / 6.9 / 5.2, 64 9.6 / 8.1 / 7.3 / 5.6, 96 - / - / 7.7 / 6.1, 128 8.8 (threes) / 7.1, 192 11.3 / 9.6,
		// 256 14.0 / 12.1, 400 23.3 / 19.0 -- from SIX planes since its z chunks may be four planes short -- round 6, us per sweep in ones / fours:
		// D = 6 3.88 / 3.33, 8 4.30 / 3.48, 12 4.79 / 3.90, 16 5.33 / 3.96, 20 5.58 / 3.87 (with chunks of eight or more the fours started at 24
		// planes); the quad kernel (STRIP4_OCTET=0) from 144 planes
		from = FX_KNOB_INT("STRIP4_OCTET", 1) ? (size_t)3 << 17 : (size_t)9 << 20;
	else if (g.X > 256)
		from = (size_t)FX_KNOB_INT("STRIP4T_FROM", 1 << 20);            // k_jacobi_strip4t, x tiles of the octet
	else
		// rows below 256 cells: a tile with its upper lanes switched off -- from 160 cells a row and 3.1 M cells; us per sweep, the block kernel's
		// twos / fours: 132^3 4.9 / 5.5, 160^3 7.7 / 6.2, 192^3 9.8 / 7.7, 224^3 15.2 / 9.6, 252^3 20.3 / 11.8; 192 x 192 x 48 4.0 / 5.5,
		// x 80 5.2 / 5.3, x 100 6.5 / 5.8; 224 x 224 x 48 4.1 / 5.6, x 64 5.8 / 5.2; 240 x 240 x 48 4.6 / 5.0, x 64 6.2 / 5.4; 160 x 160 x 100
		// 5.1 / 5.3, x 128 6.1 / 5.9
		from = g.X >= FX_KNOB_INT("STRIP4T_NARROW", 160) ? (size_t)FX_KNOB_INT("STRIP4T_NARROW_FROM", 3 << 20) : (size_t)-1;
	p.four = FX_KNOB_INT("JACOBI_PREFER4", 1) && s4 && cells >= from;
	return p;
}

// the longest launch of at most t sweeps the geometry has a kernel for (threes exist for X = 256 / 512 only, twos wherever a fused kernel
// serves the rows; a single sweep always)
static JacobiLaunch legal_launch(const JacobiPolicy& p, int t)
{
	while (p.fam[std::min(t, 4)] == JF_NONE) --t;
	return JacobiLaunch{ p.fam[std::min(t, 4)], t };
}

// the next launch of a serial round with `left` sweeps to go
static JacobiLaunch jacobi_next(const JacobiPolicy& p, int left)
{
	if (p.four)                                                         // fours; with threes, a remainder of 5 / 6 as 3 + 2 / 3 + 3 (x tiles: no threes -- 4 + 2, 4 + 1)
		return legal_launch(p, p.fam[3] ? (left >= 7 || left == 4 ? 4 : std::min(left, 3)) : std::min(left, 4));
	if (p.three) return legal_launch(p, left == 4 ? 2 : std::min(left, 3));     // threes, and a remainder of 4 as 2 + 2 rather than 3 + 1
	return legal_launch(p, std::min(left, p.unit));
}

int jacobi_plan(const JacobiPolicy& p, int n, JacobiLaunch* out)
{
	int m = 0;
	for (int left = n; left > 0; left -= out[m++].sweeps) out[m] = jacobi_next(p, left);
	return m;
}

hipError_t launch_jacobi(const Geom& g, JacobiLaunch l, const float* p_in, const float* b, float* p_out, uint8_t* frozen, uint8_t* frozen_out,
	int z_begin, int z_end, hipStream_t s)
{
	switch (l.family) {
	case JF_SWEEP1: return launch_jacobi_sweep(g, p_in, b, p_out, frozen, z_begin, z_end, s);
	case JF_TILE2D: return launch_jacobi2d(g, p_in, b, p_out, frozen, frozen_out, l.sweeps, s);
	case JF_STRIP: return launch_jacobi_strip(g, p_in, b, p_out, l.sweeps, z_begin, z_end, s);
	case JF_STRIP3: return launch_jacobi_strip3(g, p_in, b, p_out, z_begin, z_end, s);
	case JF_STRIP4: return launch_jacobi_strip4(g, p_in, b, p_out, z_begin, z_end, s);
	case JF_BLOCK2: return launch_jacobi_block2(g, p_in, b, p_out, z_begin, z_end, s);
	case JF_BLOCKG: return launch_jacobi_blockg(g, p_in, b, p_out, z_begin, z_end, s);
	default: return hipErrorInvalidValue;
	}
}

// ---- the group form: the interior launches of an overlapped round (fx_schedule.cpp: jacobi_overlapped) of n slab ranks
// sweeps per interior launch: what every member's policy agrees to -- fours / threes where all prefer them (a local choice, the exchanges do
// not depend on it), else the shortest unit
int jacobi_group_sweeps(const JacobiPolicy* p, int n)
{
	int t = p[0].unit;
	bool three = true, four = true;
	for (int i = 0; i < n; ++i) { t = std::min(t, p[i].unit); three = three && p[i].three; four = four && p[i].four; }
	return four ? 4 : three ? 3 : t;
}

// the sweeps of a round's interior launches, cnt in all: the remainder first (in launches the lead has a kernel for), then whole t's.
// Taken from the LEAD for every member, which launches each part with its own family of that length: sound because the schedule is
// only used on slabs of at least 4 k >= 2 planes, where which lengths have a kernel (fam[] != JF_NONE) depends on X and Y alone -- the
// chain's -- apart from the block kernels' limit of 2^30 cells a rank, halo included, which a chain must not straddle.
int jacobi_group_parts(const JacobiPolicy& lead, int t, int cnt, int* parts)
{
	int m = 0;
	for (int left = cnt % t; left > 0; left -= parts[m++]) parts[m] = legal_launch(lead, left).sweeps;
	for (int j = 0; j < cnt / t; ++j) parts[m++] = t;
	return m;
}

// ---- the faithful solve (FX_JACOBI_FAITHFUL: the sparse solver of fx_jacobi_freeze.hip; fx_schedule.cpp: jacobi_freeze runs what is planned here)
// Whether it runs at all: the context holds the byte mask and the tile marks, the kernels serve the geometry, a level fits the stat word's low
// byte and every launch has its counters.  On a slab rank chain-wide facts only -- every rank must take the same branch: the grid, the halo,
// the thinnest slab.
bool freeze_takes_sparse_solver(const Geom& g, uint32_t iters, bool masks, bool slab, int min_nz)
{
	if (!(masks && jacobi_freeze_supported(g) && iters <= 255 && (int)iters / jacobi_freeze_levels_per_launch() + 3 < kFreezeSlots)) return false;
	const uint64_t planes = (uint64_t)g.Zg + 2 * (uint64_t)g.H;
	return !slab || (g.H >= kFreezeHalo && min_nz >= kFreezeHalo && (uint64_t)g.X * g.Y * planes < (1u << 30));
}

// the levels a masked strip launch takes behind the dense sweep: 4 where the octet serves the grid (k_freeze_strip4o, fx_jacobi_strip4.hip;
// FREEZE_STRIP4=0: never), else 3 (k_freeze_strip3, fx_jacobi_stripm.hip); 0: no strip pipeline -- single domain, X = 256 and a third mask
// buffer to rotate through.  *forced = FREEZE_DENSE_LEVELS: how many levels go through the strip pipelines (0, 3, 4, 6, 7, 8 ...); default
// -1 = by what the dense sweeps of the last steps left relaxing (freeze_strip_hysteresis)
int freeze_strip_width(const Geom& g, bool slab, bool third_mask, int* forced)
{
	*forced = FX_KNOB_INT("FREEZE_DENSE_LEVELS", -1);
	if (slab || !third_mask || !jacobi_freeze_strip_supported(g)) return 0;
	return FX_KNOB_INT("FREEZE_STRIP4", 1) && jacobi_freeze_strip4_supported(g) ? 4 : 3;
}

// Every fourth solve counts the tiles its dense sweep left relaxing (the plume changes slowly, the count is a 5-us launch); the solve TWO
// after it takes the count over, behind the event recorded with it -- by then it has long arrived, so nothing waits, and which solve switches
// is a function of the step sequence, not of when the host happened to look (the unsynchronised read made launch sequences, step
// times and kernel statistics vary from run to run around the threshold)
FreezeCadence freeze_cadence(uint32_t gen) { return FreezeCadence{ (gen & 3u) == 0u, (gen & 3u) == 2u }; }

// How many strip launches a solve takes (n in use -> n'), from the relaxing tiles among all, with hysteresis.  Young plumes stay on the tile
// launches, where a masked launch would cost 0.08 ms for nothing.
int freeze_strip_hysteresis(int n, uint32_t active, uint32_t tiles, bool four)
{
	if (four) {
		// four levels per launch (k_freeze_strip4o behind a one-copy dense sweep): one launch pays from a fifth of the tiles (256^3 plume: frame
		// ~70, 0.600 -> 0.585 ms per step; at a half, frame 110: 0.747 -> 0.671), a second one from two thirds (frame ~140; frame 190: 0.790 -> 0.759)
		if (n == 0 && 5u * active >= tiles) n = 1;
		else if (n >= 1 && 6u * active < tiles) n = 0;
		if (n == 1 && 16u * active >= 11u * tiles) n = 2;
		else if (n == 2 && 8u * active < 5u * tiles) n = 1;
	} else                                                              // three levels per launch (k_freeze_strip3, 30 us per level): one launch from
		n = n == 0 ? 2u * active >= tiles : 5u * active >= 2u * tiles;      // half of the tiles, none again below two fifths
	return n;
}

// The launches of one solve of `iters` levels, in order: the dense sweep (level 1 everywhere), strip launches of four or three levels
// (7 = 4 + 3, 11 = 4 + 4 + 3; a strip launch needs a level left behind it for the tile launches), then tile launches of up to FREEZE_T levels
// over the tiles that still relax.  While most tiles relax the tile launches are dense sweeps in all but name (43 us per level at 256^3, a cone
// five times the core per tile) against 22 (fours) / 30 (threes) us per level on the strips.  A strip launch reads ONE copy of level 1, so
// the dense sweep in front of one leaves its second copy away (FZ_DENSE_ONE; FREEZE_DENSE_ONE=0: writes both as in front of tile launches).
// strips_in_use: the context's hysteresis state.  -> how many launches (<= kFreezeSlots wherever freeze_takes_sparse_solver holds)
int freeze_plan(const Geom& g, uint32_t iters, bool slab, bool third_mask, int strips_in_use, FreezeLaunch* out)
{
	int forced, level = 1, left = (int)iters - 1, m = 1;
	const int width = freeze_strip_width(g, slab, third_mask, &forced), T = jacobi_freeze_levels_per_launch();
	for (int want = !width ? 0 : forced < 0 ? strips_in_use * width : forced; left > 0 && m < kFreezeSlots; ++m) {
		const bool strip = want >= 3 && left > 3;                           // (never again once it fails: want and left only fall)
		const int lv = !strip ? std::min(T, left) : width == 4 && want >= 4 && left > 4 ? 4 : 3;
		out[m] = FreezeLaunch{ strip ? FZ_STRIP : FZ_TILES, lv, level };
		level += lv; left -= lv; want -= lv;
	}
	out[0] = FreezeLaunch{ m > 1 && out[1].kind == FZ_STRIP && FX_KNOB_INT("FREEZE_DENSE_ONE", 1) ? FZ_DENSE_ONE : FZ_DENSE, 1, 0 };
	return left > 0 ? 0 : m;                                            // (0: more launches than a solve has counters for -- freeze_takes_sparse_solver refuses those)
}

}  // namespace fx
