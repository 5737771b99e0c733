// fx_multigrid_plan.cpp -- the host side of the multigrid pressure solver (fx_multigrid.hip; fx_set_pressure_solver): the levels of a grid and
// where the LDS tail starts.  Plain host code: no device, no HIP call (tests/test_multigrid_ref.py links it into a small program).
#include "fx_internal.h"

namespace fx {

// Level 0 is the grid; level l + 1 halves X, Y and (3-D) Z of level l.  It is added only while every extent that would be halved is even and
// at least 4 (no half-covered coarse cell: an odd extent is not coarsened), below max_levels (0: no cap of the caller's) and below kMgMaxLevels.
// The tail: the first level >= 1 with at most kMgTailCells cells that the LDS holds with everything below it (one shared ping-pong partner of
// that level's size + correction and right-hand side per level); 0: no such level.
int mg_plan(const Geom& g, unsigned max_levels, MgPlan* out)
{
	const bool is3d = g.Zg > 1;
	const int cap = max_levels && max_levels < (unsigned)kMgMaxLevels ? (int)max_levels : kMgMaxLevels;
	int n = 0;
	MgDims d{ g.X, g.Y, g.Zg };
	out->lv[n++] = d;
	while (n < cap) {
		const bool ok = !(d.X & 1) && d.X >= 4 && !(d.Y & 1) && d.Y >= 4 && (!is3d || (!(d.Z & 1) && d.Z >= 4));
		if (!ok) break;
		d = MgDims{ d.X >> 1, d.Y >> 1, is3d ? d.Z >> 1 : 1 };
		out->lv[n++] = d;
	}
	out->levels = n;
	out->tail = 0;
	out->tail_floats = 0;
	for (int l = 1; l < n; ++l) {
		if (out->lv[l].cells() > (size_t)kMgTailCells) continue;
		size_t floats = out->lv[l].cells();                            // the shared ping-pong partner
		for (int k = l; k < n; ++k) floats += 2 * out->lv[k].cells();
		if (floats * sizeof(float) > (size_t)kMgTailLdsBytes) continue;  // (no grid gets here today: the largest tail, from 64 x 64, takes 60 KB)
		out->tail = l; out->tail_floats = (int)floats;
		break;
	}
	return n;
}

}  // namespace fx
