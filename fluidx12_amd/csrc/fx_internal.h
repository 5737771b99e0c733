// fx_internal.h -- context layout and kernel launcher declarations shared by the C-ABI
// implementation (fx_api.cpp) and the HIP kernels (fx_sim.hip, fx_render.hip, fx_sh.hip).
// Product code: never includes or links anything from oracle/.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>
#include "../../include/fluidx_hip.h"
#include "fx_knobs.h"
#include "fx_particle_sort_plan.h"

namespace fx {

// Geometry of one z-slab as the kernels see it.  Local plane l <-> global z = z0 - H + l.
struct Geom {
	int X, Y;        // plane extent
	int Zg;          // global depth
	int z0;          // first owned global plane
	int nz;          // owned planes
	int H;           // allocated halo planes on each side (0 for a single-GPU context)
	int zlo, zhi;    // inclusive range of global planes whose data is present locally
	__host__ __device__ size_t plane() const { return (size_t)X * Y; }
	__host__ __device__ int nzl() const { return nz + 2 * H; }
	__host__ __device__ size_t cells_local() const { return plane() * (size_t)nzl(); }
	__host__ __device__ size_t cells_owned() const { return plane() * (size_t)nz; }
	// local plane index of global plane z (must be present)
	__host__ __device__ int lz(int z) const { return z - z0 + H; }
};
// ---- what the launchers of the step's optional stages (vorticity, emitters, obstacles, buoyancy, open walls) test, host side
// the geometry is a whole grid, no slab of one: those stages refuse anything else with hipErrorNotSupported (local plane = global plane)
inline bool whole_grid(const Geom& g) { return g.nz == g.Zg && g.H == 0; }
// faces holds FX_WALL_* bits only, and no z face on a 2-D grid
inline bool open_faces_ok(const Geom& g, unsigned faces) { return !(faces & ~0x3Fu) && !(g.Zg <= 1 && (faces & (FX_WALL_Z_LO | FX_WALL_Z_HI))); }
// the colour field, the largest one, takes 4 GiB or more in fp32: the kernels that address by byte offset need 64-bit ones (WIDE, fx_store.h).
// WIDE_OFFSETS = 1 (lab builds): on every grid, so that tests/test_gpu_store_edges.py can run the WIDE instantiations at all
inline bool lab_wide_offsets() { return FX_KNOB_INT("WIDE_OFFSETS", 0) != 0; }
inline bool colour_wants_wide_offsets(const Geom& g) { return g.cells_local() * 16 >= ((size_t)1 << 32) || lab_wide_offsets(); }

// frame constants of the ray-march kernels (Common.hlsli:15-30 cbPerObject/cbPerFrame)
struct FrameConsts {
	float world_i[12];     // XMFLOAT3X4: rows of the transposed inverse world
	float world[12];
	float eye_pt[3];
	float light_pt[3];
	float light_color[4];
	float ambient[4];
	float wvp_i[16];       // CBPerObject.WorldViewProjI as its four constant-buffer rows (Fluid.cpp:318)
	float s2w[16];         // LightProbe's ScreenToWorld = transpose(inverse(view * proj)) rows (LightProbe.cpp:70-76)
};

// scene depth of the view-ray kernels (the reference's _HAS_DEPTH_MAP_ variants; fx_set_scene_depth).  A kernel argument of its own, passed
// only to the depth instantiations (a trailing parameter pack that is empty in the others), never part of FrameConsts.
struct DepthArgs {
	const float* depth;    // float[H][W] of the viewport, D3D depth: 0 = near plane, 1 = far plane (nothing there)
	int W, H;
	float wvp[16];         // CBPerObject.WorldViewProj (Fluid.cpp:315-318: world * view * proj) as its four constant-buffer rows
	float z_near, z_far;   // the projection's planes (UnprojectZ of the cube resolve)
	float* cube_depth;     // the cube map's depth at the mip being marched (written) or resolved (read): float[6][S][S]
};

struct SimParams {
	float dt;
	int address;           // fx_address
	int is3d;
	int impulse = 1;       // the reference's built-in source (CSAdvect.hlsl:59-68) is on; 0: fx_set_impulse switched it off
};

// ---- simulation launchers (fx_sim.hip); `half_store` selects __half storage of velocity/colour
// z_begin/z_end: global plane range to compute (within the locally present range)
// alpha: when the launch writes every voxel of an unsliced grid on the staged path it also writes the stored alpha, as fp32, to `out`
// (the render's side volume, fx_render_accel.hip) and says so in `written`
struct AdvectAlpha { float* out; bool written; };
hipError_t launch_advect(const Geom& g, const SimParams& sp, int half_store, const void* vel_in, const void* col_in,
	void* vel_out, void* col_out, int z_begin, int z_end, unsigned* halo_overflow, hipStream_t s, uint32_t* far_scratch = nullptr, size_t far_words = 0, int far_parity = 0, bool* far_used = nullptr,
	AdvectAlpha* alpha = nullptr);
// LDS-staged variant (fx_advect_lds.hip); hipErrorNotSupported when the geometry has no such path (force: also below the size where it pays)
hipError_t launch_advect_lds(const Geom& g, const SimParams& sp, int half_store, const void* vel_in, const void* col_in,
	void* vel_out, void* col_out, int z_begin, int z_end, unsigned* halo_overflow, uint32_t* far_scratch, size_t far_words, int far_parity, bool* far_used, hipStream_t s, bool force,
	AdvectAlpha* alpha = nullptr);
// far_scratch: advect_far_words(g, planes) words lent by the caller (its first two words ZEROED once; far_parity alternates over the launches that report *far_used) let the staged kernel
// defer far-tracing voxels to a second, small launch
size_t advect_far_words(const Geom& g, int nzp);
// What launch_advect_lds decides before it launches (fx_advect_plan.cpp; host code, no device needed).  staged = false: the geometry has no
// staged path.  Otherwise k_advect_lds<half_store, tile_rows, defer, p2, alpha> runs on tiles_x * tiles_y * nchunks workgroups, each a tile of
// 64 x tile_rows voxels over zchunk planes (the last chunk: what is left), and with defer k_advect_far<half_store, p2, alpha> behind it.
// AdvectLdsKnobs: the launcher's switches as it reads them per launch (zchunk: the ADVECT_ZCHUNK string, null while unset)
const int kAdvectTileX = 64;
struct AdvectLdsKnobs { int tile_rows = 8, lds_half = 1, defer = 1; const char* zchunk = nullptr; };
struct AdvectLdsPlan { bool staged, p2; int tile_rows, tiles_x, tiles_y, zchunk, nchunks; bool defer, alpha; };
AdvectLdsPlan advect_lds_plan(const Geom& g, int half_store, int z_begin, int z_end, bool force, bool has_scratch, size_t far_words, bool alpha_offered,
	const AdvectLdsKnobs& k);
// vorticity confinement of a whole-grid velocity (fx_vorticity.hip), vel_in -> vel_out (never in place: the cell stencil has radius 2);
// hipErrorNotSupported for a slab geometry
hipError_t launch_confine_vorticity(const Geom& g, int half_store, const void* vel_in, void* vel_out, float eps, float dt, hipStream_t s);
// the settable emitters (fx_emit.hip), in place on a whole-grid velocity and colour; hipErrorNotSupported for a slab geometry.
// EmitArgs is what the kernel gets: the emitters whose clipped bounding box [lo, hi) holds a cell, in list order, and the 64 x 4 x 1 tiles
// over the union of the boxes (first tile at (x0, y0, z0), on the grid's own 64 x 4 raster).  emit_plan (fx_emit_plan.cpp) fills it -> workgroups to launch
// (0: nothing, below 0: too many); host code, no device needed.  alpha: the render's side volume when it holds this colour field's alpha, else null
const int kEmitTileX = 64, kEmitTileY = 4;
struct EmitBall { float c[3], rr, rate[4], force[3], swirl; int lo[3], hi[3]; };
struct EmitArgs { int n, x0, y0, z0, tiles_x, tiles_y, tiles_z; EmitBall e[FX_MAX_EMITTERS]; };
int emit_plan(const Geom& g, const fx_emitter* list, int count, EmitArgs* out);
hipError_t launch_emit(const Geom& g, int half_store, void* vel, void* col, float* alpha, const fx_emitter* list, int count, float dt, hipStream_t s);
// buoyancy (fx_heat.hip), one launch over a whole grid: the temperature t_in is advected with vel0, cooled, heated by the sources and stored
// to t_out; VELOCITY1 (vel1) gets the force, in place, on the axes with up != 0; hipErrorNotSupported for a slab geometry.  code: the
// obstacle bytes (fx_obstacle.hip) or null.  HeatArgs is what the kernel gets: the coefficients, the axes the force acts on (bit a: up[a] != 0,
// never z on a 2-D grid), the grid's 64 x 4 raster and the sources whose clipped bounding box [lo, hi) holds a cell, in list order.
// heat_plan (fx_heat_plan.cpp; host code, no device needed: it takes the boxes from emit_plan) fills it -> workgroups to launch (below 0: too many)
const int kHeatTileX = 64, kHeatTileY = 4;
struct HeatBall { float c[3], rr, rate; int lo[3], hi[3]; };
struct HeatArgs { float ambient, weight, lift, cooling, up[3]; int axes, n, tiles_x, tiles_y; HeatBall s[FX_MAX_HEAT_SOURCES]; };
int heat_plan(const Geom& g, const fx_buoyancy& b, const fx_heat_source* list, int count, HeatArgs* out);
// faces: the open walls (FX_WALL_* bits, 0 = none): the sample is blended towards the ambient value by open_wall_weight of each axis
hipError_t launch_heat(const Geom& g, int half_store, const fx_buoyancy& b, const fx_heat_source* list, int count, const void* vel0, void* vel1,
	const void* col, const float* t_in, float* t_out, const uint8_t* code, float dt, int address, hipStream_t s, unsigned faces = 0);
// MacCormack advection (fx_maccormack.hip; fx_set_advection_scheme), two launches over a whole grid: the predictor samples vel_in / col_in at the
// back-traced place into the scratch (hat_vel: three fp32 planes of X * Y * Z, hat_col: one float4 per cell, fp32 whatever the storage), the
// corrector samples the scratch at the forward-traced place, corrects, limits to the back-trace's eight taps and finishes like k_advect (impulse,
// attenuation) into vel_out / col_out.  alpha_out: the render's side volume (it then gets the stored alpha of every cell), or null.
// hipErrorNotSupported for a slab geometry
const int kMcTileX = 64, kMcTileY = 4;
hipError_t launch_maccormack(const Geom& g, const SimParams& sp, int half_store, const void* vel_in, const void* col_in, void* vel_out, void* col_out,
	float* hat_vel, float* hat_col, float* alpha_out, hipStream_t s);
// ---- the multigrid pressure solver (fx_multigrid.hip, fx_multigrid_plan.cpp; fx_set_pressure_solver), whole grids with closed walls and no
// obstacles only.  mg_plan (host code, no device needed): the levels of a grid under a cap (0: none) and the level the LDS tail starts at
// (0: no tail) with the floats of LDS it takes -> the level count
const int kMgMaxLevels = (int)FX_MG_MAX_LEVELS, kMgTailCells = 4096, kMgTailLdsBytes = 64 * 1024;
struct MgDims { int X, Y, Z; __host__ __device__ size_t cells() const { return (size_t)X * Y * Z; } };
struct MgPlan { int levels, tail, tail_floats; MgDims lv[kMgMaxLevels]; };
int mg_plan(const Geom& g, unsigned max_levels, MgPlan* out);
// one damped lock-step sweep e_in -> e_out (p' = fma(omega, J - p, p)); e_in null: the input is all +0 and is not read (the same bits)
hipError_t launch_mg_smooth(const MgDims& d, int is3d, const float* e_in, const float* b, float* e_out, float omega, hipStream_t s);
// the residual of (p, b) on the fine level, restricted: one value of b_coarse per 2 x 2 (x 2) fine cells; no fine-size residual is stored
hipError_t launch_mg_residual_restrict(const MgDims& fine, int is3d, const float* p, const float* b, float* b_coarse, hipStream_t s);
// p += the (bi-, tri-)linear prolongation of the coarse correction e, in place
hipError_t launch_mg_prolong_correct(const MgDims& fine, int is3d, float* p, const float* e_coarse, hipStream_t s);
// the rest of a cycle from level plan.tail down in one workgroup: reads b[plan.tail], leaves every level's correction in e[l] and the lower
// levels' right-hand sides in b[l] (arrays indexed by level; entries below plan.tail unused)
struct MgTailArgs { int first, levels, is3d, pre, post, coarse; float omega; MgDims lv[kMgMaxLevels]; float* e[kMgMaxLevels]; float* b[kMgMaxLevels]; };
hipError_t launch_mg_tail(const MgTailArgs& a, int lds_floats, hipStream_t s);
// ---- open walls (the inflow pass: fx_open.hip; the sweeps and the projection: the bnd launchers below), whole grids only (hipErrorNotSupported
// for a slab geometry).  faces: FX_WALL_* bits, the code byte's bit order (x-, x+, y-, y+, z-, z+; no z bit on a 2-D grid: hipErrorInvalidValue)
// The share of a linear sample at t = i0 + f (i0 = fl = floor(t), taps i0 and i0 + 1 of an axis of n cells) that lies inside the box when the
// cells beyond an open face are empty: low face open: 0 for i0 < -1, f for i0 == -1; high face open: 0 for i0 >= n, 1 - f for i0 == n - 1; else 1
__host__ __device__ inline float open_wall_weight(float fl, float f, int n, unsigned lo_open, unsigned hi_open)
{
	float w = 1.0f;
	if (lo_open && fl < 0.0f) w = fl == -1.0f ? f : 0.0f;
	if (hi_open && fl >= (float)(n - 1)) w = fl == (float)(n - 1) ? 1.0f - f : 0.0f;
	return w;
}
// ... of cell i's back-trace with velocity u0 along that axis, t formed as k_heat (fx_heat.hip) step 1 forms it
__host__ __device__ inline float open_wall_trace(float u0, float dt, int i, int n, unsigned lo_open, unsigned hi_open)
{
	const float p = ((float)i + 0.5f) / (float)n;
	const float a = fmaf(-u0, dt, p);
	const float t = a * (float)n - 0.5f;
	const float fl = floorf(t);
	return open_wall_weight(fl, t - fl, n, lo_open, hi_open);
}
const int kOpenTileX = 64, kOpenTileY = 4;
// the inflow pass, in place on a whole-grid colour: COLOR *= w of the back-trace with vel0; alpha: the render's side volume when it holds this
// colour field's alpha, else null
hipError_t launch_open_inflow(const Geom& g, int half_store, const void* vel0, void* col, float* alpha, unsigned faces, float dt, hipStream_t s);
hipError_t launch_divergence(const Geom& g, int half_store, const void* vel, float* b, int z_begin, int z_end, hipStream_t s);
// ---- solid obstacles (fx_obstacle.hip), whole grids only (hipErrorNotSupported for a slab geometry).  code: one byte per cell, bits 0..5 = the
// clamped neighbour at x-1, x+1, y-1, y+1, z-1, z+1 is solid (z bits 0 on 2-D grids), bit 6 = the cell is; the stencil launchers read it, never the mask
enum { OB_XM = 1, OB_XP = 2, OB_YM = 4, OB_YP = 8, OB_ZM = 16, OB_ZP = 32, OB_SELF = 64 };
// launch_obstacle_codes: solid_dev uint8[Z][Y][X] (device) -> code; stats_dev (8 device words) gets { solid cells (2 words, low first), min x, y, z, max x, y, z }
hipError_t launch_obstacle_codes(const Geom& g, const uint8_t* solid_dev, uint8_t* code, unsigned* stats_dev, hipStream_t s);
hipError_t launch_obstacle_mask(const uint8_t* code, uint8_t* solid_dev, size_t n, hipStream_t s);      // the 0 / 1 mask back out of the codes
// the enforce launch's tiles: the solids' box [lo, hi) on the grid's 64 x 4 raster, first tile at (*x0, *y0, lo[2]) -> workgroups (host code)
long long obstacle_enforce_tiles(const int lo[3], const int hi[3], int* x0, int* y0, int* tiles_x, int* tiles_y);
// The three launches whose rule sees the solid's velocity take the bodies of fx_set_obstacle_bodies: (list, count) with count == 0 = the solids
// rest, count >= 1 = a solid cell moves with the first body whose box holds its centre (then code must not be null and count no more than
// FX_MAX_OBSTACLE_BODIES: else hipErrorInvalidValue).  The sweeps never see the bodies.
// solid cells of vel (3 components) become their body's velocity (+0 at rest), those of col +0, in place; alpha: the render's side volume when it
// holds this colour field's alpha, else null
hipError_t launch_obstacle_enforce(const Geom& g, int half_store, const uint8_t* code, const int lo[3], const int hi[3],
	const fx_obstacle_body* list, int count, void* vel, void* col, float* alpha, hipStream_t s);
hipError_t launch_divergence_obs(const Geom& g, int half_store, const void* vel, const uint8_t* code, const fx_obstacle_body* list, int count,
	float* b, int z_begin, int z_end, hipStream_t s);
// the boundary-aware sweep (one per launch; 3-D, X % 4 == 0: four cells per thread, else the scalar kernel) and projection, for obstacles,
// open walls or both.  code: the obstacle bytes, or null (then no code byte is read); faces: the open walls' FX_WALL_* bits, or 0 (all closed);
// neither: hipErrorInvalidValue, that is the plain kernels' case
hipError_t launch_jacobi_bnd(const Geom& g, const float* p_in, const float* b, const uint8_t* code, float* p_out, unsigned faces,
	int z_begin, int z_end, hipStream_t s);
hipError_t launch_project_bnd(const Geom& g, const SimParams& sp, int half_store, const void* vel_in, const float* p, const uint8_t* code,
	const fx_obstacle_body* list, int count, void* vel_out, unsigned faces, int z_begin, int z_end, hipStream_t s);
// ---- the mesh voxeliser (fx_voxelize.hip; fx_set_obstacle_meshes), whole 3-D grids only: closed triangle meshes -> the 0 / 1 byte mask
// launch_obstacle_codes reads.  The rule is integer arithmetic on coordinates quantised to 1 / 256 of a cell (include/fluidx_hip.h).
// VoxMesh: one mesh, every pointer device memory; xf null = no transform.  bits: the toggle bitmap, [Z][Y][voxel_row_words] words, all zero on
// entry to the scatter and again behind the fill.  report: word 0 open columns, word 1 skipped triangles (both added to).  nbig / list: a
// zeroed word and room for nt entries -- the triangles whose clipped (y, z) box is too large for one wave go through them.
struct VoxMesh { const float* pos; const uint32_t* idx; const float* xf; uint32_t nv, nt; };
enum { kVoxReportWords = 2 + FX_MAX_OBSTACLE_MESHES };
inline int voxel_row_words(const Geom& g) { return g.X / 32 + 1; }                   // bit X: the virtual cell beyond the +x wall
hipError_t launch_voxel_scatter(const Geom& g, const VoxMesh& m, unsigned* bits, unsigned* report, unsigned* nbig, uint4* list, hipStream_t s);
// the prefix XOR along x of one mesh's toggles, written (first) or ORed into mask[Z][Y][X]; clears the bitmap
hipError_t launch_voxel_fill(const Geom& g, unsigned* bits, uint8_t* mask, bool first, unsigned* report, hipStream_t s);
// ---- tracer particles and the point query (fx_particles.hip; fx_set_particles, fx_sample_velocity), whole grids only (hipErrorNotSupported for a
// slab geometry).  records: count x (x, y, z, age), device memory, 16-byte aligned, moved in place one step of dt through vel0; code: the obstacle
// bytes or null; faces: the open walls' FX_WALL_* bits or 0.  Reads vel0 and code, writes the records: no field of the simulation is touched
hipError_t launch_move_particles(const Geom& g, int half_store, const fx_particle_params& prm, const void* vel0, const uint8_t* code, unsigned faces,
	float dt, float* records, uint32_t count, hipStream_t s);
// points: count x float4 (w ignored), out: count x 3 floats, both device memory; out = the stored velocity vel0 sampled as the particles sample it
hipError_t launch_sample_velocity(const Geom& g, int half_store, const void* vel0, const float* points, float* out, uint32_t count, hipStream_t s);
// ---- the particle sort (fx_particle_sort.hip; fx_set_particle_sort, fx_sort_particles): records sorted in place by cell, dead ones last, stable;
// p: psort_plan of this grid and count (fx_particle_sort_plan.cpp), scratch: p.scratch_bytes of device memory laid out as p says -- order and
// live are read there.  Enqueues only; reads and writes the records and the scratch, nothing else.  count 0 is the caller's to skip
hipError_t launch_particle_sort(const Geom& g, const PsortPlan& p, float* records, void* scratch, hipStream_t s);
// ---- the particle trail (fx_particle_trail.hip; fx_set_particle_trail, fx_deposit_particles, fx_particle_density).  acc: one uint64 per cell,
// all zero between calls.  splat: every live record adds its 2^24 of integer weights to the cells around it (count 0 is the caller's to skip);
// apply: the cells with acc != 0 add to col (and to temp unless it is null), store their alpha to `alpha` unless it is null, and clear their
// word; code: the obstacle code or null.  Both enqueue only
hipError_t launch_trail_splat(const Geom& g, const float* records, uint32_t count, unsigned long long* acc, hipStream_t s);
hipError_t launch_trail_apply(const Geom& g, int half_store, const fx_particle_trail& t, float dt, unsigned long long* acc, void* col, float* temp,
	float* alpha, const uint8_t* code, hipStream_t s);
// ---- the particle draw (fx_particle_draw.hip; fx_set_particle_draw, fx_draw_particles, fx_particle_splats).  acc: two uint64 per pixel of the
// W x H viewport, all zero between calls.  splat: every live record that projects onto the viewport adds its amounts, dimmed by the alpha of the
// direct view march of its pixel through `color` (wvp: the forward WorldViewProj rows, depth: the scene depth float[H][W] or null, ns: the merged
// direct march's sample count); hipErrorInvalidValue for a 2-D grid or one beyond fx_render's limits; count 0 is the caller's to skip.
// resolve: the pixels with a non-zero pair blend into target, every pixel stores out_float, the pairs are cleared.  Both enqueue only
hipError_t launch_draw_splat(const Geom& g, int half_store, const void* color, const FrameConsts& fc, const float wvp[16], const float* depth, int W, int H,
	uint32_t ns, float lifetime, const float* records, uint32_t count, unsigned long long* acc, hipStream_t s);
hipError_t launch_draw_resolve(const fx_particle_draw& dr, int W, int H, unsigned long long* acc, uint8_t* target, float* out_float, hipStream_t s);
// ---- the obstacle draw (fx_obstacle_draw.hip; fx_set_obstacle_draw, fx_draw_obstacles, fx_obstacle_hits).  bricks: one uint64 per 4 x 4 x 4
// cells, bit (z & 3) * 16 + (y & 3) * 4 + (x & 3) = the cell is solid (code bit 6), cells beyond the grid 0; brick (bx, by, bz) at
// (bz * BY + by) * BX + bx with B_a = (N_a + 3) / 4.  pack: the brick volume of `code`.  cast: per pixel of the W x H viewport the view ray walked
// to the first solid cell of `code` (null: every pixel misses) within the box [lo, hi); target, out_float, depth_out (float[H][W]) and hits
// (uint64[H][W]) are each stored unless null; scene: the caller's depth float[H][W] or null, never depth_out.  hipErrorInvalidValue for a 2-D grid
// or one of 2^32 cells or more.  Both enqueue only
inline size_t obstacle_brick_count(const Geom& g) { return (size_t)((g.X + 3) / 4) * (size_t)((g.Y + 3) / 4) * (size_t)((g.Zg + 3) / 4); }
hipError_t launch_obstacle_pack(const Geom& g, const uint8_t* code, unsigned long long* bricks, hipStream_t s);
hipError_t launch_obstacle_cast(const Geom& g, const uint8_t* code, const unsigned long long* bricks, const int lo[3], const int hi[3],
	const FrameConsts& fc, const float wvp[16], int point_light, const fx_obstacle_draw& dr, const float* scene, int W, int H,
	uint8_t* target, float* out_float, float* depth_out, unsigned long long* hits, hipStream_t s);
// ---- the particle spawners (fx_particle_spawn.hip;fx_set_particle_spawners, fx_spawn_particles).  One device block: SpawnState at its head,
// then one count of dead records per workgroup of kSpawnRecords records and the scan's block sums, laid out by spawn_plan(count).  The setter
// fills `site` and zeroes the rest; born .. serial are what fx_particle_spawn_info copies out in one piece
const uint32_t kSpawnThreads = 256;                           // threads of a count / place workgroup
const uint32_t kSpawnItems = 4;                               // records each of them takes
const uint32_t kSpawnRecords = kSpawnThreads * kSpawnItems;   // records per workgroup
const uint32_t kSpawnScanTile = 2048;                         // workgroup counts one scan workgroup takes (256 threads x 8)
struct SpawnSite { uint32_t shape, seed; float center[3], half[3], rate, age_spread; };
struct SpawnState {
	unsigned long long born, dropped, blocked, serial[FX_MAX_PARTICLE_SPAWNERS];      // the counters and the births each spawner has attempted
	unsigned long long acc[FX_MAX_PARTICLE_SPAWNERS];                                 // the fractions, units of 2^-16 births
	unsigned long long base[FX_MAX_PARTICLE_SPAWNERS];                                // of the run in flight: the serial of each spawner's first birth,
	uint32_t first[FX_MAX_PARTICLE_SPAWNERS + 1];                                     // ... its first birth's number j (the last entry: n),
	uint32_t dead, take, pad;                                                         // ... D and min(n, D)
	SpawnSite site[FX_MAX_PARTICLE_SPAWNERS];
};
struct SpawnPlan { uint32_t count, wgs, scan_blocks; size_t off_counts, off_sums, bytes; };
SpawnPlan spawn_plan(uint32_t count);                         // count 0 plans the state alone
// records: count x (x, y, z, age) as the move has them, code: the obstacle bytes or null, mem: p.bytes of device memory holding `spawners`
// sites.  Four launches (six when the counts need more than one scan tile); enqueues only; writes dead records and the block, nothing else.
// count 0 is the caller's to skip
hipError_t launch_spawn_particles(const Geom& g, const SpawnPlan& p, uint32_t spawners, float dt, float* records, const uint8_t* code, void* mem, hipStream_t s);
// ---- which kernel of a stage's family serves a geometry and a storage type (fx_sim.hip: the one place that decides; host code, no device needed):
// cells per thread along the row -- the scalar kernel (any extent, 2-D), 16-byte vectors, or the 4-byte-aligned pairs / triples of the vW kernels
enum SimStage { SIM_DIVERGENCE = 0, SIM_PROJECT = 1 };
enum SimRowKernel { ROW_SCALAR = 0, ROW_V4 = 4, ROW_VW2 = 2, ROW_VW3 = 3 };
int sim_row_kernel(const Geom& g, int half_store, int stage, int is3d);       // is3d: SimParams::is3d (the projection's own 2-D / 3-D switch)
// fx_field_digest's range rule: the planes [z_begin, z_begin + z_count) lie inside the owned planes (z_count = 0 stands for all of them)
bool digest_range_ok(const Geom& g, uint32_t z_begin, uint32_t z_count);
// one lock-step sweep p_in -> p_out on planes [z_begin, z_end); frozen may be null
hipError_t launch_jacobi_sweep(const Geom& g, const float* p_in, const float* b, float* p_out, uint8_t* frozen,
	int z_begin, int z_end, hipStream_t s);
// the same sweep over two disjoint plane ranges in one launch (the two face zones of a slab)
hipError_t launch_jacobi_sweep2(const Geom& g, const float* p_in, const float* b, float* p_out, uint8_t* frozen,
	int z_begin, int z_end, int z_begin2, int z_end2, hipStream_t s);
// two or three sweeps per launch, register-resident strips (fx_jacobi_strip.hip)
bool jacobi_strip_supported(const Geom& g);
bool jacobi_strip_wide(const Geom& g);       // X = 512: only the two-sweep wide kernel exists
hipError_t launch_jacobi_strip(const Geom& g, const float* p_in, const float* b, float* p_out, int sweeps, int z_begin, int z_end, hipStream_t s);
// three sweeps per launch, register strips + the LDS as a second register file (fx_jacobi_strip3.hip; X = 256)
bool jacobi_strip3_supported(const Geom& g);
hipError_t launch_jacobi_strip3(const Geom& g, const float* p_in, const float* b, float* p_out, int z_begin, int z_end, hipStream_t s);
// four sweeps per launch, a workgroup's four waves as a quad over 16 rows (fx_jacobi_strip4.hip; X = 256, Y % 16 == 0)
bool jacobi_strip4_supported(const Geom& g);
hipError_t launch_jacobi_strip4(const Geom& g, const float* p_in, const float* b, float* p_out, int z_begin, int z_end, hipStream_t s);
// two sweeps per launch, one 4 x 4-row block per wave (fx_jacobi_block.hip; X = 128)
bool jacobi_block2_supported(const Geom& g);
hipError_t launch_jacobi_block2(const Geom& g, const float* p_in, const float* b, float* p_out, int z_begin, int z_end, hipStream_t s);
// the same scheme for any X = CPL x (<= 64 lanes), CPL <= 4: rows that are no multiple of four cells (150^3, the reference's GI preset)
bool jacobi_blockg_supported(const Geom& g);
hipError_t launch_jacobi_blockg(const Geom& g, const float* p_in, const float* b, float* p_out, int z_begin, int z_end, hipStream_t s);
// the reference's own solve (cap N + per-cell early-out) as a sparse solver (fx_jacobi_freeze.hip): a dense first sweep that writes
// level 1 to TWO buffers and marks the 32 x 8 x 8 tiles that still relax, then launches of <= 4 levels over the marked tiles only.
// stat: device word raised to stat_hi | level for every level that leaves a cell relaxing.
bool jacobi_freeze_supported(const Geom& g);
int jacobi_freeze_tiles(const Geom& g);
size_t jacobi_freeze_mask_bytes(const Geom& g);
size_t jacobi_freeze_list_bytes(const Geom& g);     // one work list (eight per-XCD sub-lists of { tile, box } entries)
const int kFreezeSlots = 128;                       // launches a solve may enqueue
size_t jacobi_freeze_count_words();                 // list-length counters of one solve: kFreezeSlots launches x 8 sub-lists
int jacobi_freeze_levels_per_launch();
// the device-side work state of one solve: tile_mark[tile] == gen <=> the tile is on the first list already; the dense sweep fills
// list[0] and counts[0][8] (zero on entry); tile launch n reads list[n & 1] / counts[n] and appends its surviving tiles to
// list[(n + 1) & 1] / counts[n + 1]; counts_next = the next solve's counters, cleared by this solve's dense launch
struct FreezeWork { uint32_t* tile_mark; uint32_t gen; void* list[2]; int cap; uint32_t* counts; uint32_t* counts_next; };
// a slab rank runs the solver on a view of the planes it holds (jacobi_freeze_view): `g` = the view, the field pointers advanced to its plane 0,
// [z_begin, z_begin + nzp) = the owned planes in view coordinates (nzp = 0: all), vel_comp_cells = cells between velocity components (0: the view's)
Geom jacobi_freeze_view(const Geom& g, int* first_plane, int* own_begin);
hipError_t launch_freeze_dense(const Geom& g, const float* p_in, const float* b, float* pA, float* pB, uint8_t* mA, uint8_t* mB,
	const FreezeWork& w, hipStream_t s, const void* vel = nullptr, int vel_half = 0, int z_begin = 0, int nzp = 0, size_t vel_comp_cells = 0);   // vel: compute (and store) the divergence of this velocity instead of reading b
bool jacobi_freeze_can_fuse_divergence(const Geom& g);
// flag_tag (first tile launch only, n == 0): the value a tile's mark must hold to be taken -- w.gen as k_freeze_dense writes it, or the tag the
// last masked strip launch wrote (0: w.gen)
hipError_t launch_freeze_tiles(const Geom& g, const float* p_src, const float* b, float* p_dst, const uint8_t* m_src, uint8_t* m_dst,
	const FreezeWork& w, int n, int levels, int level_base, uint32_t* stat, uint32_t stat_hi, hipStream_t s, int z_begin = 0, int nzp = 0, uint32_t flag_tag = 0);
// three more levels for EVERY cell on the streaming strip pipeline (fx_jacobi_stripm.hip; X = 256, single domain): level_in in p_in / m_in ->
// level_in + 3 in p_outA = p_outB, nibbles in m_outA = m_outB; tiles that still relax get `tag` in tile_mark
bool jacobi_freeze_strip_supported(const Geom& g);
hipError_t launch_count_marks(const uint32_t* tile_mark, uint32_t gen, int ntiles, uint32_t* out, hipStream_t s);   // tiles with tile_mark == gen, into *out (a host-visible word)
hipError_t launch_freeze_strip3(const Geom& g, const float* p_in, const float* b, float* p_outA, float* p_outB, const uint8_t* m_in, uint8_t* m_outA, uint8_t* m_outB,
	uint32_t* tile_mark, uint32_t tag, uint32_t* stat, uint32_t stat_hi, int level_in, hipStream_t s);
bool jacobi_freeze_strip4_supported(const Geom& g);
hipError_t launch_freeze_strip4(const Geom& g, const float* p_in, const float* b, float* p_outA, float* p_outB, const uint8_t* m_in, uint8_t* m_outA, uint8_t* m_outB,
	uint32_t* tile_mark, uint32_t tag, uint32_t* stat, uint32_t stat_hi, int level_in, hipStream_t s);
// 2-D grids (fx_jacobi2d.hip): up to jacobi2d_max_sweeps (0: not a 2-D grid / switched off) lock-step sweeps per launch on LDS tiles, with or without the freeze bytes
int jacobi2d_max_sweeps(const Geom& g);
hipError_t launch_jacobi2d(const Geom& g, const float* p_in, const float* b, float* p_out, const uint8_t* frozen_in, uint8_t* frozen_out, int sweeps, hipStream_t s);
// ---- which family runs a round of the fixed-count solve, and with how many sweeps per launch (fx_jacobi_plan.cpp: the one place that decides)
enum JacobiFamily { JF_NONE = 0, JF_SWEEP1, JF_TILE2D, JF_STRIP, JF_STRIP3, JF_STRIP4, JF_BLOCK2, JF_BLOCKG };    // one per launcher above
struct JacobiLaunch { int family, sweeps; };
// what a geometry runs under a jacobi_fuse request (0: none), the launcher switches, a freeze byte mask and (2-D) a second buffer for it:
// fam[k] = the family of a launch of k sweeps, k = 1 .. 4 (JF_NONE: no such kernel; 2-D tiles: every length up to `unit`), unit = sweeps per
// launch unless three / four (the measured preferences of the default schedule) say otherwise
struct JacobiPolicy { int fam[5]; int unit, three, four; };
JacobiPolicy jacobi_policy(const Geom& g, int fuse, bool frozen, bool second_mask);
int jacobi_plan(const JacobiPolicy& p, int n, JacobiLaunch* out);        // the launches of a serial round of n sweeps, in order (at most n) -> how many
// one planned launch, p_in -> p_out on planes [z_begin, z_end): valid provided p_in / b are valid `sweeps` planes beyond the range (or up to the
// global boundary).  frozen: the byte mask (or null); frozen_out: where the 2-D tiles leave it
hipError_t launch_jacobi(const Geom& g, JacobiLaunch l, const float* p_in, const float* b, float* p_out, uint8_t* frozen, uint8_t* frozen_out,
	int z_begin, int z_end, hipStream_t s);
// the interior launches of an overlapped round of n slab ranks: sweeps per launch, and the lengths of a round of cnt sweeps (at most cnt)
int jacobi_group_sweeps(const JacobiPolicy* p, int n);
int jacobi_group_parts(const JacobiPolicy& lead, int t, int cnt, int* parts);
// ---- the launches of the faithful solve (fx_jacobi_plan.cpp decides, fx_schedule.cpp: jacobi_freeze runs them)
const int kFreezeHalo = 4;                          // planes a slab rank exchanges behind every launch = the most levels a tile launch takes (jacobi_freeze_levels_per_launch)
// masks: the context holds the byte mask and the tile-mark buffer; slab: it is a rank of a chain whose thinnest slab has min_nz planes
bool freeze_takes_sparse_solver(const Geom& g, uint32_t iters, bool masks, bool slab, int min_nz);
// FZ_DENSE: the dense sweep writing both copies of level 1, FZ_DENSE_ONE: one (a strip launch follows); FZ_STRIP: a masked strip launch of
// 4 or 3 levels for every cell; FZ_TILES: a launch of up to 4 levels over the tiles that still relax.  base: the level the launch starts from
enum FreezeKind { FZ_DENSE = 0, FZ_DENSE_ONE, FZ_STRIP, FZ_TILES };
struct FreezeLaunch { int kind, levels, base; };
// the launches of a solve in order (the levels sum to iters) -> how many, at most kFreezeSlots (0: they do not fit); strips_in_use: the context's fz_dense_n
int freeze_plan(const Geom& g, uint32_t iters, bool slab, bool third_mask, int strips_in_use, FreezeLaunch* out);
// levels per strip launch (4 / 3; 0: no strip pipeline); *forced: FREEZE_DENSE_LEVELS -- the levels the strip pipelines take, below 0: as many
// launches as the count of relaxing tiles asks for (the two functions below)
int freeze_strip_width(const Geom& g, bool slab, bool third_mask, int* forced);
// what the solve of generation gen does about that count -- count: launch k_count_marks behind its dense sweep, take_over: read the count
// launched two solves ago
struct FreezeCadence { bool count, take_over; };
FreezeCadence freeze_cadence(uint32_t gen);
// strip launches in use, n -> n', once a count is taken over: `active` of `tiles` tiles relax; four: a strip launch takes four levels, not three
int freeze_strip_hysteresis(int n, uint32_t active, uint32_t tiles, bool four);
// The LDS hand-overs of the strip kernels wait in bounded loops; a wait that runs out raises a device word (per translation unit) instead
// of hanging the device or continuing silently.  Read-and-clear on the current device; fx_synchronize turns a raised word into FX_E_DEVICE.
// fx_field_digest's kernel: two wrapping sums of 64-bit mixes of (stored bits, key0 + element index) over `count` elements, added to out[0..1]
hipError_t launch_digest(const void* v, size_t count, int elem_bytes, unsigned long long key0, unsigned long long* out, hipStream_t s);
hipError_t strip3_fault_take(unsigned* out);
hipError_t strip4_fault_take(unsigned* out);
// rec (optional, slab ranks): the step record of launch_face_need is produced by this launch when it can be (fp32 3-D kernel
// over exactly the owned planes); *rec_done tells whether it was
hipError_t launch_project(const Geom& g, const SimParams& sp, int half_store, const void* vel_in, const float* p,
	void* vel_out, int z_begin, int z_end, hipStream_t s, int* rec = nullptr, int digest = 0, const unsigned* halo_overflow = nullptr,
	bool* rec_done = nullptr);
// multi-GPU: what the next advection will need from the z-neighbours (rec[0] planes below, rec[1] above; exact for time steps
// <= dt), closed with the options digest (rec[2]) and this step's halo-overflow flag (rec[3]); rec = 4 device ints
hipError_t launch_face_need(const Geom& g, int half_store, const void* vel, float dt, int address, int digest, const unsigned* halo_overflow, int* rec, hipStream_t s);
hipError_t launch_copy_bytes(void* dst, const void* src, size_t bytes, hipStream_t s);   // device-to-device, as a kernel
hipError_t launch_copy_velocity(const Geom& g, int half_store, const void* vel_in, void* vel_out, hipStream_t s);

// ---- layout conversion between dense fp32 host layouts and device storage (fx_sim.hip)
// scalar planes: nplanes x cells fp32 <-> T ; colour: cells x 4
hipError_t launch_to_storage(const float* src, void* dst, size_t n, int half_store, hipStream_t s);
hipError_t launch_from_storage(const void* src, float* dst, size_t n, int half_store, hipStream_t s);

// ---- ray march launchers
// counters (FX_OPT_COUNT_SAMPLES, else null): 64 shards x { colour samples of view rays, density samples of light / AO rays, light-map
// fetches }, added to by every thread that took one
const int kSampleShards = 64;
// plain path (fx_render.hip): every sample gathers its taps
hipError_t launch_raymarch_light(const Geom& g, int half_store, const void* color, uint32_t* lightmap,
	const FrameConsts& fc, const float* sh, uint32_t num_samples, hipStream_t s, unsigned long long* counters = nullptr, int point_light = 0);
// (point_light, here and below: the FX_LIGHT_POINT instantiations of the kernels that cast light rays -- fx_march.h point_light_ray)
hipError_t launch_raymarch_view(const Geom& g, int half_store, const void* color, const uint32_t* lightmap,
	const FrameConsts& fc, const float* sh, int cube_size, uint32_t mask, uint32_t num_samples,
	uint32_t num_light_samples, int separate, uint8_t* cube, hipStream_t s, unsigned long long* counters = nullptr, const DepthArgs* depth = nullptr, int point_light = 0);
// direct screen-space march (row f-2): one ray per pixel, blended into the RGBA8 target (and/or kept as float4)
hipError_t launch_raycast_direct(const Geom& g, int half_store, const void* color, const uint32_t* lightmap,
	const FrameConsts& fc, const float* sh, int W, int H, uint32_t num_samples, uint32_t num_light_samples, int separate,
	uint8_t* target, float* out_float, hipStream_t s, unsigned long long* counters = nullptr, const DepthArgs* depth = nullptr, int point_light = 0);
// accelerated path (fx_render_accel.hip; the default, bit-identical to the plain one).  Device scratch, owned by the context:
struct RenderAccel {
	float* occ;          // per 4^3 block: max alpha over everything a sample based in the block can touch (n cells) + the maxima it is dilated from (n cells)
	float* alpha;        // alpha-only fp32 copy of the colour volume, X * Y * Zg
	uint32_t* bits;      // { pos, vis } masks of the fine level (fine_words each) [+ { pos, vis } of the LDS level (mask_words each) when msh > 0]
	uint32_t* list;      // ids of the light-map voxels that cast rays, a segment of X * Y entries per z plane
	float* gi;           // light probe only (allocated by fx_set_sh): direction of each listed voxel's occlusion ray, 3 floats per list entry
	uint32_t* cells;     // ids of the 4^3 cells that may hold a lit voxel, a segment of CX * CY entries per cell layer
	uint32_t* ctr;       // counters, a cache line apart: list lengths per z plane, work heads of the view march, cell-list lengths per layer
	int CX, CY, CZ;      // fine level: 4^3 blocks
	int msh, MX, MY, MZ; // level held in the LDS: (4 << msh)^3 blocks, at most 262144 of them
	uint32_t fine_words, mask_words;
	uint32_t frame;      // renders built so far: the counters are double-buffered (set frame & 1), every build pass clears the list lengths of the NEXT render's set
	uint32_t fill_frame; // filling build passes so far: each leaves a bit per cell "holds a lit voxel" (in `cells`, two sets) for the next one
};
void render_accel_layout(const Geom& g, RenderAccel* a);       // fills the dimensions
size_t render_accel_bits_words(const RenderAccel& a);
size_t render_accel_ctr_words(const Geom& g);
// alpha_current: a.alpha holds this colour field's alpha already (AdvectAlpha)
// fill (with alpha_current, on grids whose extents are powers of two -- a voxel's centre sample is then its own alpha): the pass also writes the
// unlit voxels' light-map constant and lists the lit voxels, i.e. it does k_light_cells' and k_light_classify's work in the same sweep over
// the side volume; *filled says whether it did (launch_accel_light is then told so)
// incremental: the light map still holds what the previous filling pass and its ray kernels left, and the unlit value is the same -- only
// the cells that held a lit voxel then need the constant again
struct LightFill { uint32_t* lightmap; const FrameConsts* fc; int has_sh; bool incremental; };
hipError_t launch_accel_build(const Geom& g, int half_store, const void* color, const RenderAccel& a, hipStream_t s, bool alpha_current = false,
	const LightFill* fill = nullptr, bool* filled = nullptr);
hipError_t launch_accel_light(const Geom& g, const RenderAccel& a, uint32_t* lightmap, const FrameConsts& fc, const float* sh,
	uint32_t num_samples, hipStream_t s, unsigned long long* counters = nullptr, bool filled = false, int point_light = 0);
hipError_t launch_accel_view(const Geom& g, int half_store, const void* color, const uint32_t* lightmap, const FrameConsts& fc, const float* sh,
	int cube_size, uint32_t mask, uint32_t num_samples, uint32_t num_light_samples, int separate, uint8_t* cube, const RenderAccel& a, hipStream_t s,
	unsigned long long* counters = nullptr, const DepthArgs* depth = nullptr, int point_light = 0);
hipError_t launch_accel_direct(const Geom& g, int half_store, const void* color, const uint32_t* lightmap, const FrameConsts& fc, const float* sh,
	int W, int H, uint32_t num_samples, uint32_t num_light_samples, int separate, uint8_t* target, float* out_float, const RenderAccel& a, hipStream_t s,
	unsigned long long* counters = nullptr, const DepthArgs* depth = nullptr, int point_light = 0);
// 2-D visualiser (PSVisualizeColor): colour[parity] of a Z = 1 grid onto the render target
hipError_t launch_visualize_color(const Geom& g, int half_store, const void* color, int W, int H, uint8_t* target, float* out_float, hipStream_t s);
hipError_t launch_lightmap_decode(const uint32_t* lightmap, float* out, size_t n, hipStream_t s);

// ---- cube map -> screen resolve (fx_resolve.hip; row f-1)
// depth (optional): the depth-aware CubeCast (PSCube.hlsli:82-113), for a cube map that was marched with the same scene depth attached
hipError_t launch_resolve_cube(const uint8_t* cube_mip, int N, const FrameConsts& fc, int W, int H, uint8_t* target,
	float* out_float, hipStream_t s, const DepthArgs* depth = nullptr);
hipError_t launch_clear_target(uint8_t* target, int W, int H, const float rgba[4], hipStream_t s);
// sky pass (PSEnvironment): float radiance cube [6][n][n][3] on the device -> target (opaque write) and/or float4
hipError_t launch_environment(const float* cube, int n, const FrameConsts& fc, int W, int H, uint8_t* target, float* out_float, hipStream_t s);

// ---- BC6H_UF16 / DDS cube (fx_bc6h.hip; row f-4)
hipError_t launch_bc6h_decode(const void* blocks_dev, int nbx, int nby, int n, float* out_dev, hipStream_t s);
enum { DDS_BC6H_UF16 = 0, DDS_RGBA32F = 1, DDS_RGB32F = 2, DDS_RGBA16F = 3, DDS_RGBA8 = 4 };
struct DdsCube { uint32_t size, mips; int kind; size_t face_offset[6], mip_offset[16]; };
bool dds_cube_layout(const void* dds, size_t bytes, DdsCube* out);
void dds_linear_face_to_rgb(const void* texels, int kind, size_t n, float* out);

// ---- SH light probe (fx_sh.hip): cube float[6][n][n][3] (device) -> out float[27] (device)
hipError_t launch_sh_transform(const float* cube, int n, float* scratch0, float* scratch1, float* w0, float* w1,
	float* out27, hipStream_t s);
size_t sh_scratch_floats(int n, int which);

}  // namespace fx
