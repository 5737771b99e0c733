// fx_advect_plan.cpp -- the host side of the staged advection (fx_advect_lds.hip: k_advect_lds, k_advect_far): whether a launch takes the staged
// path at all, which instantiation <HALF, TY, DEFER, P2, ALPHA> serves it, the tiles, the chunks along z and the scratch the deferred voxels
// need.  Plain host code: no device, no HIP call, the launcher's switches come in as arguments (tests/test_advect_edges.py links it into a
// small program).
#include "fx_internal.h"
#include <algorithm>
#include <cstdlib>

namespace fx {

AdvectLdsPlan advect_lds_plan(const Geom& g, int half_store, int z_begin, int z_end, bool force, bool has_scratch, size_t far_words, bool alpha_offered,
	const AdvectLdsKnobs& k)
{
	AdvectLdsPlan p = {};
	auto pow2 = [](int v) { return v > 0 && (v & (v - 1)) == 0; };
	const int TX = kAdvectTileX;
	const int nzp = z_end - z_begin;
	// rows per workgroup tile.  16 (one 1024-thread workgroup per CU, 1.16 x instead of 1.29 x border) measured 0.228 / 0.269 ms against
	// 0.223 / 0.263 for 8 (256^3, states of step 25 / 110): the bytes it saves it loses to the single workgroup's barrier stalls
	const bool p2 = pow2(g.X) && pow2(g.Y) && pow2(g.Zg);
	const int TY = p2 && k.tile_rows == 16 ? 16 : 8;
	// where it pays: from 4 M voxels per launch.  128^3 measured 0.032-0.040 ms against 0.030 for k_advect_fast, 150^3 0.049-0.053 against
	// 0.057 for k_advect -- and inside whole steps, with the second launch for the far-tracing voxels, 0.0586 against 0.0555: too few
	// workgroups either way
	const size_t min_voxels = (size_t)1 << 22;
	if (g.Zg <= 1 || g.X < TX || g.Y < TY || nzp < 12 || (!force && (size_t)g.X * g.Y * (size_t)nzp < min_voxels) ||
		g.cells_local() * 16 >= ((size_t)1 << 32))
		return p;
	if (half_store && !k.lds_half) return p;
	auto lg = [](int v) { int n = 0; while ((1 << n) < v) ++n; return n; };
	const int ntx = (g.X + TX - 1) / TX, nty = (g.Y + TY - 1) / TY;
	const int tiles_xy = ntx * nty;
	// planes per workgroup.  Every chunk re-reads two planes.  While the far-tracing voxels were gathered inside this kernel the
	// workgroups over the plume took several times longer than the rest and short chunks (2048 workgroups of 16 planes at 256^3)
	// balanced that: 0.216 ms with 16, 0.219 with 8, 0.241 with 32, 0.258 with 64.  With those voxels deferred every workgroup costs
	// the same: 16 / 32 / 64 planes measure 0.211 / 0.203 / 0.212 ms (fp32), 0.147 / 0.143 / 0.144 (fp16), within the noise -- 32.
	const bool want_defer = has_scratch && k.defer != 0;
	int zchunk = k.zchunk && *k.zchunk ? atoi(k.zchunk) : (want_defer ? 32 : 16);
	// grids of a few million voxels (150^3: 57 tiles per plane) have too few workgroups for 32-plane chunks to fill the chip and too many
	// with short ones for one resident round (two workgroups per CU): as many chunks as keep them all resident at once.  150^3, us per
	// launch by planes per chunk: 6 49.8, 8 51.4, 12 51.2, 15 54.8, 19 49.0, 25 57.5, 32 67.5, 64 122 (k_advect: 57.3)
	if (!p2 && !k.zchunk) {
		const int chunks = std::max(1, 512 / tiles_xy);
		zchunk = std::max(8, (nzp + chunks - 1) / chunks);
	}
	if (zchunk < 4) zchunk = 4;
	if (zchunk > nzp) zchunk = nzp;
	const int nchunks = (nzp + zchunk - 1) / zchunk;
	// far-tracing voxels deferred to k_advect_far when the caller lent scratch: [two alternating totals][the common list: an id per voxel]
	// [a segment of 64 * TY * zchunk ids per workgroup] (ADVECT_DEFER = 0: gathered inside the staged kernel, as before)
	const uint32_t nwg = (uint32_t)(tiles_xy * nchunks), far_cap = (uint32_t)(TX * TY * zchunk);
	const size_t flat_words = (size_t)g.X * g.Y * (size_t)nzp;
	const bool defer = want_defer && far_words >= 2 + flat_words + (size_t)nwg * far_cap &&
		((uint64_t)g.Zg << (lg(g.X) + lg(g.Y))) <= ((uint64_t)1 << 32);          // (a note = x | y << lgX | z << lgP, or the voxel's index in the whole grid)
	p.staged = true;
	p.p2 = p2;
	p.tile_rows = TY;
	p.tiles_x = ntx; p.tiles_y = nty;
	p.zchunk = zchunk; p.nchunks = nchunks;
	p.defer = defer;
	// the render's alpha side volume rides along on the default path (8-row tiles, far voxels deferred) of a context whose local planes
	// are the whole grid (the side volume is indexed by global voxel)
	p.alpha = alpha_offered && defer && TY == 8 && g.nzl() == g.Zg && z_begin == 0 && z_end == g.Zg;
	return p;
}

// scratch words launch_advect_lds needs to defer far-tracing voxels for planes [z_begin, z_end) of `g` (0: no staged path there)
size_t advect_far_words(const Geom& g, int nzp)
{
	const int TX = kAdvectTileX;
	if (g.Zg <= 1 || g.X < TX || g.Y < 16 || nzp < 12) return 0;
	const size_t tiled = (size_t)((g.X + TX - 1) / TX * TX) * (size_t)((g.Y + 7) / 8 * 8);             // a plane as the 64 x 8 tiles cover it
	return 2 + (size_t)g.X * g.Y * (size_t)nzp + tiled * (size_t)(nzp + 32);   // two totals, the common list, the workgroups' segments (whole chunks)
}

}  // namespace fx
