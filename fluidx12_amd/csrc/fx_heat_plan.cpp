// fx_heat_plan.cpp -- the host side of the buoyancy pass (fx_heat.hip: k_heat): the coefficients, the axes the force acts on, the grid's
// tiles and the heat sources that reach the kernel with their clipped bounding boxes.  Plain host code: no device, no HIP call
// (tests/test_buoyancy_ref.py links it, with fx_emit_plan.cpp, into a small program).
#include "fx_internal.h"

namespace fx {

// A heat source has an emitter's support, so its box is an emitter's box: each source goes through emit_plan as a one-entry list (which also
// drops the sources no cell can lie in).  The launch itself covers the grid -- every cell is advected --, on its own 64 x 4 raster.
int heat_plan(const Geom& g, const fx_buoyancy& b, const fx_heat_source* list, int count, HeatArgs* out)
{
	out->ambient = b.ambient; out->weight = b.density_weight; out->lift = b.lift; out->cooling = b.cooling;
	out->axes = 0;
	for (int a = 0; a < 3; ++a) {
		out->up[a] = b.up[a];
		if (b.up[a] != 0.0f && (a < 2 || g.Zg > 1)) out->axes |= 1 << a;        // a 2-D grid has no z component to push
	}
	int n = 0;
	for (int k = 0; k < count && k < (int)FX_MAX_HEAT_SOURCES; ++k) {
		fx_emitter e = {};
		e.struct_size = sizeof e;
		for (int a = 0; a < 3; ++a) e.center[a] = list[k].center[a];
		e.radius = list[k].radius;
		EmitArgs one;
		emit_plan(g, &e, 1, &one);
		if (one.n != 1) continue;
		HeatBall& h = out->s[n++];
		for (int a = 0; a < 3; ++a) { h.c[a] = one.e[0].c[a]; h.lo[a] = one.e[0].lo[a]; h.hi[a] = one.e[0].hi[a]; }
		h.rr = one.e[0].rr;
		h.rate = list[k].rate;
	}
	out->n = n;
	out->tiles_x = (g.X + kHeatTileX - 1) / kHeatTileX;
	out->tiles_y = (g.Y + kHeatTileY - 1) / kHeatTileY;
	const long long wgs = (long long)out->tiles_x * out->tiles_y * g.Zg;
	return wgs > 0x7fffffffLL ? -1 : (int)wgs;
}

}  // namespace fx
