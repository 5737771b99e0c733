// fx_emit_plan.cpp -- the host side of the emitter pass (fx_emit.hip: k_emit): which emitters reach the kernel, with which clipped bounding
// boxes, and the tiles of the launch.  Plain host code: no device, no HIP call (tests/test_emitter_ref.py links it into a small program).
#include "fx_internal.h"
#include <algorithm>
#include <cmath>
#include <climits>

namespace fx {

// The boxes and the tiling, in double: cell x lies in the box of an emitter when |(x + 0.5) / X - cx| <= r + margin.  The support is
// d2 <= r^2 up to the rounding of the fp32 chain (a few ulp of d2 and of px, py, pz); the margin -- r / 10^4 + 10^-6 max(1, |cx|) -- is
// orders of magnitude above that, so the box can only be too large, never cut a cell of the support off.
int emit_plan(const Geom& g, const fx_emitter* list, int count, EmitArgs* out)
{
	const int N[3] = { g.X, g.Y, g.Zg };
	const bool is3d = g.Zg > 1;
	int n = 0, ulo[3] = { INT_MAX, INT_MAX, INT_MAX }, uhi[3] = { 0, 0, 0 };
	for (int k = 0; k < count && k < (int)FX_MAX_EMITTERS; ++k) {
		const fx_emitter& src = list[k];
		EmitBall b;
		bool empty = false;
		for (int ax = 0; ax < 3; ++ax) {
			if (ax == 2 && !is3d) { b.lo[2] = 0; b.hi[2] = 1; continue; }
			const double c = (double)src.center[ax], r = (double)src.radius;
			const double m = r * (1.0 + 1e-4) + 1e-6 * std::max(1.0, std::fabs(c));
			const double lo = std::ceil((c - m) * N[ax] - 0.5), hi = std::floor((c + m) * N[ax] - 0.5) + 1.0;
			b.lo[ax] = (int)std::min(std::max(lo, 0.0), (double)N[ax]);
			b.hi[ax] = (int)std::min(std::max(hi, 0.0), (double)N[ax]);
			empty = empty || b.hi[ax] <= b.lo[ax];
		}
		if (empty || !(src.radius * src.radius > 0.0f)) continue;   // (a radius below 1e-23 squares to 0 in fp32 -- the exponent would be -0 / 0 on a cell centre: such a ball has no cell)
		for (int ax = 0; ax < 3; ++ax) { b.c[ax] = src.center[ax]; b.force[ax] = src.force[ax]; ulo[ax] = std::min(ulo[ax], b.lo[ax]); uhi[ax] = std::max(uhi[ax], b.hi[ax]); }
		for (int i = 0; i < 4; ++i) b.rate[i] = src.color_rate[i];
		b.rr = src.radius * src.radius;                           // fp32, one rounding
		b.swirl = src.swirl;
		out->e[n++] = b;
	}
	out->n = n;
	if (!n) { out->x0 = out->y0 = out->z0 = out->tiles_x = out->tiles_y = out->tiles_z = 0; return 0; }
	out->x0 = ulo[0] / kEmitTileX * kEmitTileX; out->y0 = ulo[1] / kEmitTileY * kEmitTileY; out->z0 = ulo[2];
	out->tiles_x = (uhi[0] - out->x0 + kEmitTileX - 1) / kEmitTileX;
	out->tiles_y = (uhi[1] - out->y0 + kEmitTileY - 1) / kEmitTileY;
	out->tiles_z = uhi[2] - ulo[2];
	const long long wgs = (long long)out->tiles_x * out->tiles_y * out->tiles_z;
	return wgs > 0x7fffffffLL ? -1 : (int)wgs;
}

}  // namespace fx
