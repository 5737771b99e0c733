/* fluidx_hip.h -- C ABI of the MI355X-native smoke solver + cube-map-space ray marcher.
 *
 * Drop-in boundary for the reference's `class Fluid` operator (StarsX/FluidX12,
 * FluidX12/Content/Fluid.h:20-35) and the SH side of `LightProbe` (Content/LightProbe.h:16-26):
 * every entry point below names the reference interface it replaces.  Plain C types only
 * (pointers + sizes); `void* stream` is a `hipStream_t` (the reference's `XUSG::CommandList*`
 * becomes the HIP stream work is enqueued on; NULL = the context's own stream).
 *
 * All functions return 0 (FX_OK) or a negative FX_E_* code and never throw across the ABI.
 * A context is not thread-safe (single caller thread, like the reference's UI thread).
 * There is no CPU fallback: without a HIP device fx_create fails with FX_E_DEVICE.
 */
#ifndef FLUIDX_HIP_H
#define FLUIDX_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FX_ABI_VERSION 7   /* 7: fx_field_digest, fx_last_error; 6: fx_comm_init_peer, fx_set_knob / fx_knob_name, FX_OPT_RENDER_ACCEL, fx_timing.freeze_strip_launches; the launcher switches no longer come from FLUIDX_* environment variables */

enum fx_status {
	FX_OK = 0,
	FX_E_INVALID = -1,      /* bad argument / unsupported combination          */
	FX_E_DEVICE = -2,       /* HIP runtime error (no device, launch failure)   */
	FX_E_NOMEM = -3,        /* device or host allocation failed                */
	FX_E_STATE = -4,        /* call order violation (e.g. render before update) */
	FX_E_COMM = -5,         /* RCCL error / library unavailable                */
	FX_E_HALO = -6          /* back-trace left the exchanged halo (multi-GPU)  */
};

/* Fluid::RenderFlags (Fluid.h:12-18) */
enum fx_render_flags {
	FX_RAY_MARCH_DIRECT = 0,
	FX_RAY_MARCH_CUBEMAP = 1,
	FX_SEPARATE_LIGHT_PASS = 2,
	FX_OPTIMIZED = 3
};
#define FX_FRAME_COUNT 3            /* Fluid::FrameCount (Fluid.h:35) */

enum fx_storage { FX_STORAGE_FP32 = 0, FX_STORAGE_FP16 = 1 };   /* velocity/colour texel storage; the
                                                                  reference is RGBA16F (Fluid.cpp:207,213) */
enum fx_jacobi_mode { FX_JACOBI_FIXED = 0,      /* N lock-step sweeps, no early-out (BASELINE configs)     */
                      FX_JACOBI_FAITHFUL = 1 }; /* cap N (reference: 64) + per-cell freeze at |dx| < 1e-3
                                                   (CSPoisson.hlsli:11,24)                                  */
enum fx_address { FX_ADDRESS_CLAMP = 0,         /* FluidEZ.cpp:406 (default path of the reference)          */
                  FX_ADDRESS_MIRROR = 1 };      /* Fluid.cpp:452                                            */

/* fields for fx_upload / fx_download; host layouts are dense fp32 regardless of device storage:
 *   VELOCITY  float[3][Z][Y][X]  (component planes; the texture advect reads = m_velocities[0])
 *   VELOCITY1 float[3][Z][Y][X]  (m_velocities[1], advect output / project input)
 *   COLOR     float[Z][Y][X][4]  (m_colors[parity], the one every renderer reads)
 *   COLOR_PREV float[Z][Y][X][4] (m_colors[!parity])
 *   PRESSURE  float[Z][Y][X]     (m_incompress)      DIVERGENCE float[Z][Y][X] (scratch b)
 *   LIGHTMAP  float[Z][Y][X][3]  (m_lightMap decoded from R11G11B10F)
 *   CUBEMAP   uint8[6][S][S][4]  (mip `lod` of m_cubeMap, S = X >> lod, R8G8B8A8_UNORM)
 *   CUBE_DEPTH float[6][S][S]    (mip `lod` of the cube depth: the scene depth each texel's ray saw when the last cube-path fx_render ran
 *                                with a depth attached, CSRayMarch.hlsl:124; 1.0 where no such ray was cast; download only)
 *   TEMPERATURE float[Z][Y][X]   (the buoyancy's temperature, fp32 on the device too; only while fx_set_buoyancy has it on, FX_E_STATE otherwise)
 * Z = the context's own slab (slab_nz planes), never the halo. */
enum fx_field {
	FX_FIELD_VELOCITY = 0, FX_FIELD_VELOCITY1 = 1, FX_FIELD_COLOR = 2, FX_FIELD_COLOR_PREV = 3,
	FX_FIELD_PRESSURE = 4, FX_FIELD_DIVERGENCE = 5, FX_FIELD_LIGHTMAP = 6, FX_FIELD_CUBEMAP = 7,
	FX_FIELD_TARGET = 8,        /* render target of fx_render_cube: uint8 [viewport_h][viewport_w][4] (download only) */
	FX_FIELD_TARGET_FLOAT = 9,  /* the resolve's output before the blend: float [h][w][4], zeros where discarded     */
	FX_FIELD_CUBE_DEPTH = 10,   /* see above (3-D contexts with a viewport)                                          */
	FX_FIELD_TEMPERATURE = 11   /* see above and fx_set_buoyancy                                                     */
};

typedef struct fx_ctx fx_ctx;

/* replaces the arguments of Fluid::Init (Fluid.cpp:189-270) */
typedef struct fx_desc {
	uint32_t struct_size;       /* = sizeof(fx_desc)                                        */
	uint32_t grid_x, grid_y, grid_z;    /* global grid; grid_x == grid_y (Fluid.cpp:201); grid_z == 1 -> 2D */
	uint32_t viewport_w, viewport_h;    /* Init(width, height); 0 x 0 = a context that only simulates (fx_render: FX_E_INVALID) */
	uint32_t storage;           /* fx_storage                                               */
	uint32_t jacobi_iters;      /* N (BASELINE: 20/40/80; reference faithful: 64)           */
	uint32_t jacobi_mode;       /* fx_jacobi_mode                                           */
	uint32_t advect_address;    /* fx_address                                               */
	int32_t  device;            /* HIP device ordinal, -1 = current                         */
	uint32_t slab_z0, slab_nz;  /* z-slab owned by this context; {0, 0} = whole grid        */
	uint32_t halo_advect;       /* planes allocated (and at most exchanged) per face for the advection (0 = default 6) */
	uint32_t halo_jacobi;       /* sweeps per pressure halo exchange (0 = default)          */
	uint32_t flags;             /* FX_FLAG_*                                                */
} fx_desc;

/* fx_desc.flags: bits 0-3 = Jacobi sweeps fused per launch (temporal blocking), 0 = library default,
 * 1 = one launch per sweep; results are bit-identical for every setting */
#define FX_FLAG_JACOBI_FUSE_MASK 0xFu
/* multi-rank contexts: keep every halo exchange on the compute stream (no side comm stream, no face-first
 * ordering); results are bit-identical either way -- the switch exists to measure what the overlap buys */
#define FX_FLAG_NO_OVERLAP 0x10u
/* a context that only renders: one colour buffer + light map / cube map / target, no velocity, pressure or divergence.
 * It receives its colour from fx_upload or fx_comm_gather_color; fx_simulate and the stage calls return FX_E_STATE. */
#define FX_FLAG_RENDER_ONLY 0x20u

/* values Fluid::UpdateFrame derives (Fluid.cpp:324-333) */
typedef struct fx_frame_info {
	uint32_t cube_lod;          /* m_cubeMapLOD                         */
	uint32_t cube_size;         /* grid_x >> cube_lod                   */
	uint32_t ray_samples;       /* m_raySampleCount                     */
	uint32_t visibility_mask;   /* m_visibilityMask                     */
	uint32_t frame_parity;      /* m_frameParity                        */
	float    edge_pixels;       /* EstimateCubeEdgePixelSize            */
	float    time_step;
	float    world_view_proj_i[16];  /* CBPerObject.WorldViewProjI as its 4 constant-buffer rows (Fluid.cpp:318; ABI 2) */
	float    screen_to_world[16];    /* LightProbe CBPerFrame.ScreenToWorld rows (LightProbe.cpp:70-76; ABI 2)        */
} fx_frame_info;

/* HIP-event timings accumulated by fx_simulate / fx_render while enabled (milliseconds, launch counts) */
typedef struct fx_timing {
	double   advect_ms, divergence_ms, jacobi_ms, project_ms, light_ms, view_ms, exchange_ms;
	uint64_t steps, jacobi_launches, jacobi_sweeps, renders;
	double   resolve_ms;        /* fx_render_cube (ABI 2) */
	/* ABI 3: when a step mixes launch shapes (40 sweeps = 12 launches of three + 2 of two), the launches with the most
	 * sweeps each -- the dominant kernel -- are also booked on their own; otherwise these equal the jacobi_* totals */
	double   jacobi_main_ms;
	uint64_t jacobi_main_launches, jacobi_main_sweeps;
	/* ABI 4 (slab ranks): bytes this rank SENT in halo exchanges, and planes its advection exchange carried across its lower +
	 * upper face (summed over the timed steps; halo_advect per face without FX_OPT_ADAPTIVE_HALO) */
	uint64_t exchange_bytes, advect_halo_planes;
	double   chain_ms;          /* face chains of the overlapped pressure rounds (their own stream, beside the interior sweeps) */
	/* ABI 5 (FX_JACOBI_FAITHFUL, single-domain contexts): pressure solves since the last reset, and the sweeps the reference's
	 * loop (CSPoisson.hlsli:11-25) executes in them -- per solve 1 + the last sweep that left a cell relaxing, at most N.
	 * jacobi_sweeps above counts the levels ENQUEUED (always N: the sparse solver needs no read-back to stop early). */
	uint64_t freeze_solves, freeze_sweeps;
	uint64_t exchange_calls;    /* slab ranks: halo exchanges issued (one RCCL group call each) over the timed steps */
	/* FX_OPT_COUNT_SAMPLES: trilinear colour fetches of the view rays, density fetches of the light / AO rays (the light pass's one
	 * fetch per voxel included), light-map fetches -- summed over the renders since the last reset */
	uint64_t view_samples, light_samples, lightmap_fetches;
	/* ABI 6 (FX_JACOBI_FAITHFUL, single domain, X = 256): launches of the masked strip pipeline among jacobi_launches -- which of the two
	 * launch sequences the solves took (decided per solve from a tile count measured two solves earlier: a function of the step sequence) */
	uint64_t freeze_strip_launches;
} fx_timing;

int fx_abi_version(void);
const char* fx_error_string(int status);

/* Fluid::Fluid + Fluid::Init (Fluid.cpp:168-270): allocates all fields zero-initialised */
int fx_create(fx_ctx** out, const fx_desc* desc);
/* Fluid::~Fluid */
int fx_destroy(fx_ctx* ctx);
/* Fluid::SetMaxSamples (Fluid.cpp:272-276) */
int fx_set_max_samples(fx_ctx* ctx, uint32_t max_ray_samples, uint32_t max_light_samples);
/* Fluid::SetSH (Fluid.cpp:278-281): 9 x float3 host coefficients, NULL detaches the probe */
int fx_set_sh(fx_ctx* ctx, const float* coeffs27);
/* Fluid::UpdateFrame (Fluid.cpp:283-346); matrices row-major, row-vector convention (DirectXMath).
 * view/proj/eye may be NULL for a pure simulation context (no rendering state is updated).
 * A call with time_step > 0 flips the colour parity (Fluid.cpp:345): from then on FX_FIELD_COLOR names the buffer the coming fx_simulate
 * writes, and FX_FIELD_COLOR_PREV the buffer FX_FIELD_COLOR named before the call, which is the one that step's advection samples.
 * frame_index picks one of the FX_FRAME_COUNT per-frame constant slots and enters no arithmetic of the step. */
int fx_update_frame(fx_ctx* ctx, float time_step, uint8_t frame_index,
	const float view[16], const float proj[16], const float eye[3]);
/* Fluid::Simulate (Fluid.cpp:348-410): enqueues advect + divergence + N sweeps + project.  Asynchronous like the reference's call, with one
 * exception: with FX_JACOBI_FAITHFUL on a single 256-wide domain every fourth solve takes over a tile count that a launch two solves earlier
 * left in host-visible memory and waits for THAT launch's event first (hipEventSynchronize; long past in practice) -- so the host runs at
 * most about two steps ahead of the device there, and such a context must not be stepped inside a stream capture.  The wait is what makes
 * the launch sequence a function of (the last uploaded state, the steps since) instead of when the host happened to look; fx_upload of a
 * simulation field starts that adaptation over.
 * The whole step with every optional stage, in order, and what each stage reads at its point of the step (each block below gives its own
 * rule; time_step > 0, tests/step_ref.py composes the per-stage models in exactly this order and tests/test_gpu_step_model.py holds
 * fx_simulate to it):
 *   advect (either scheme)   traces with VELOCITY, samples VELOCITY and COLOR_PREV                          -> VELOCITY1, COLOR
 *   inflow                   the advection's back-trace again: VELOCITY                                     -> COLOR in place
 *   emit                                                                                                    -> VELOCITY1, COLOR in place
 *   heat                     traces TEMPERATURE with VELOCITY; rho = COLOR.w as the stages above left it    -> TEMPERATURE (the two buffers
 *                            swap: every later stage and the next step see the new field), VELOCITY1 in place
 *   trail                    the particle positions as the buffer holds them now                            -> COLOR, TEMPERATURE in place
 *   enforce                                                                                                 -> VELOCITY1, COLOR in place
 *   confine                  VELOCITY1                                                                      -> VELOCITY1 (the names swap)
 *   divergence               VELOCITY1                                                                      -> DIVERGENCE
 *   solve                    DIVERGENCE, PRESSURE as the previous step (or an upload) left it               -> PRESSURE
 *   project                  VELOCITY1, PRESSURE                                                            -> VELOCITY
 *   particles                the sort when this run of the stage is due one, then the move through the VELOCITY just projected, then the
 *                            births while spawners are set (fx_set_particle_spawners)
 * Behind the step FX_FIELD_VELOCITY1 holds what the divergence read, FX_FIELD_COLOR_PREV what the advection sampled. */
int fx_simulate(fx_ctx* ctx, void* stream, uint8_t frame_index);
/* Fluid::Render (Fluid.cpp:412-446), all four flag combinations:
 *   flags & FX_RAY_MARCH_CUBEMAP   cube-map-space march (merged, or light volume + view pass with FX_SEPARATE_LIGHT_PASS):
 *                                  writes the cube map (and light map); fx_render_cube below puts it on the screen
 *   otherwise                      direct screen-space march, one ray per pixel of the viewport (PSRayCast / PSRayCastV,
 *                                  Fluid.cpp:932-972), blended straight into the render target (PREMULTIPLIED) */
/* (FX_E_INVALID also for a 3-D grid with grid_y * (grid_z + 1) >= 2^24 or 2^32 voxels: tap indices are 32 bits wide.) */
int fx_render(fx_ctx* ctx, void* stream, uint8_t frame_index, uint8_t flags);
/* The caller-side half of the cube path (row f-1 of SURVEY.md 8): the render target the reference's caller binds.
 * fx_clear_render_target = ClearRenderTargetView (FluidX12.cpp:471-472; the demo clears to (0.2, 0.2, 0.2, 0));
 * fx_render_cube = Fluid::renderCube (Fluid.cpp:910-931) in its raster-free per-pixel form (PSRayCastCube.hlsl):
 * resolves mip `cube_lod` of the cube map the last fx_render wrote onto the viewport_w x viewport_h RGBA8 target with
 * the PREMULTIPLIED blend (Fluid.cpp:653).  Read the result with fx_download(FX_FIELD_TARGET). */
int fx_clear_render_target(fx_ctx* ctx, void* stream, const float rgba[4]);
int fx_render_cube(fx_ctx* ctx, void* stream, uint8_t frame_index);

/* Scene depth for the following renders (the reference's _HAS_DEPTH_MAP_ variants): the volume is occluded by the scene it stands in.
 * depth = float[viewport_h][viewport_w], D3D convention: 0 = near plane, 1 = far plane = "nothing here" (the demo's clear value,
 * FluidX12.cpp:473), under the projection passed to fx_update_frame.  z_near / z_far: that projection's planes (SharedConsts.h:8-9: 1, 1000),
 * used by the cube resolve's UnprojectZ.  flags & FX_DEPTH_DEVICE: `depth` is device memory of the context's device, read in place by every
 * later render (the caller keeps it alive and orders its writes on `stream`); otherwise it is copied, enqueued on `stream`, and the call
 * returns once the copy is made.  NULL detaches: renders are then exactly what they are without this call.
 *   direct march (PSRayCast.hlsl:52-56)   every ray ends at its pixel's scene point (GetTMax, RayMarch.hlsli:99-110)
 *   cube-map march (CSRayMarch.hlsl:121-126)  each texel's ray point-samples the depth (nearest texel, clamped to the edge) where a point just
 *                                         inside its entry projects, ends there, and keeps the value in FX_FIELD_CUBE_DEPTH
 *   fx_render_cube (PSCube.hlsli:82-113)   weights the four cube taps by view-space depth agreement with the pixel, when the cube map
 *                                         resolved was marched with depth attached
 * Depth is render state: kept across fx_update_frame, not checkpointed, not digested; FX_FLAG_RENDER_ONLY contexts take it too.
 * FX_E_INVALID: size is not the viewport, 2-D grid, 0 x 0 viewport, slab context, !(0 < z_near < z_far), unknown flag bits. */
#define FX_DEPTH_DEVICE 0x1u
int fx_set_scene_depth(fx_ctx* ctx, void* stream, const float* depth, uint32_t width, uint32_t height,
	float z_near, float z_far, uint32_t flags);

/* The scene light of the following renders.  A context starts with the reference's constants (Fluid.cpp:169-173: position (75, 75, -75),
 * colour (1, .7, .3) x 3 pi, ambient (1, 1, 1) x 1.5 pi, directional); fx_set_light(ctx, NULL) returns to them.
 *   position  world space of fx_update_frame's view matrix; the volume is the cube [-10, 10]^3 there (its world matrix is a scale by 10)
 *   FX_LIGHT_DIRECTIONAL  only the direction of `position` matters: every shadow ray runs along normalize(position) (CSRayMarchL.hlsl:52-53)
 *   FX_LIGHT_POINT        `position` is the light's place (the reference's compiled-out _POINT_LIGHT_ variants): the shadow ray of a light-map
 *                         voxel (CSRayMarchL.hlsl:49-50) and the nested light ray of each visible sample of the merged marches
 *                         (CSRayMarch.hlsl:165, PSRayCast.hlsl:93) run from there towards the light.  Two deviations from that variant text:
 *                         (A) the ray ENDS at the light -- a sample is taken only while t < |light - origin| -- so smoke behind a lamp does
 *                         not shadow what is in front of it (the variant marches on through the light); (B) where the light sits exactly
 *                         on a ray's origin (a light vector of length zero, or not finite) no shadow ray is cast: shadow = 1.
 *                         No distance attenuation (the reference has none).
 *   color, ambient        rgb x intensity (w); ambient is unused while a light probe is set (fx_set_sh), as in the reference
 * GI / occlusion rays, the unlit constant `light colour + ambient`, step rule and thresholds are the same for both kinds.
 * The light is render state like the scene depth: per context, kept across fx_update_frame, in force at the next fx_render, not checkpointed,
 * not digested; FX_FLAG_RENDER_ONLY contexts take it too.
 * FX_E_INVALID (the previous light stays in force): null context, wrong struct_size, unknown kind, a component that is not finite, a negative
 * colour or ambient component (the light map is unsigned R11G11B10_FLOAT), a directional light at (0, 0, 0), 2-D grid, slab context. */
#define FX_LIGHT_DIRECTIONAL 0u
#define FX_LIGHT_POINT       1u
typedef struct fx_light {
	uint32_t struct_size, kind;
	float position[3];
	float color[4];
	float ambient[4];
} fx_light;
int fx_set_light(fx_ctx* ctx, const fx_light* light);
int fx_get_light(fx_ctx* ctx, fx_light* out);

/* The light probe's sky pass (LightProbe::RenderEnvironment, LightProbe.cpp:85-97; PSEnvironment.hlsl), which the demo draws
 * before the volume (FluidX12.cpp:483): fx_set_environment keeps a copy of the radiance cube float[6][n][n][3] on the device
 * (NULL releases it), fx_render_environment writes it onto the render target as seen by the camera of the last
 * fx_update_frame (no blending: rgb, alpha 0). */
int fx_set_environment(fx_ctx* ctx, const float* cube, uint32_t n);
int fx_render_environment(fx_ctx* ctx, void* stream, uint8_t frame_index);

int fx_get_frame_info(fx_ctx* ctx, fx_frame_info* out);

/* blocks until everything enqueued by this context has finished; reports FX_E_HALO if the advection back-trace of a multi-GPU
 * step left the exchanged halo ON THIS RANK, and thereby acknowledges it.  Until then fx_download of a simulation field,
 * fx_checkpoint_save and fx_comm_gather_color of this rank return FX_E_HALO as well.  Independently the fault travels with the
 * per-step record: the next fx_simulate returns FX_E_HALO on EVERY rank of the chain, once, without stepping (its inputs are
 * untouched) -- the chain-wide notice, whichever of the two calls comes first; the fx_simulate after that starts clean on every
 * rank, with or without an fx_synchronize in between (the notice takes the faulting rank's device flag down and keeps the fault on
 * the host: that rank's read-back and checkpoints go on refusing until its fx_synchronize).  No rank runs on, or stores, fields that
 * differ from the single-domain run without having been told. */
int fx_synchronize(fx_ctx* ctx);
/* Also FX_E_DEVICE from fx_synchronize: a strip kernel's LDS hand-over wait ran out (a protocol error or a lost wave; the waits are bounded,
 * ~10 ms) -- the pressure field that launch wrote is not the solver's; the report clears the fault.  fx_last_error: what the last failed
 * call of this context had to say beyond its status (a HIP error string, which kernel family timed out, ...); "" if nothing; the pointer is
 * valid until the context's next call. */
const char* fx_last_error(fx_ctx* ctx);

/* checkpoint / parity access (no reference counterpart; the reference cannot read fields back) */
int fx_upload(fx_ctx* ctx, int field, const void* host, size_t bytes);
int fx_download(fx_ctx* ctx, int field, void* host, size_t bytes);
size_t fx_field_bytes(fx_ctx* ctx, int field);
/* A 128-bit digest of global planes [z_begin, z_begin + z_count) of a simulation field (VELOCITY .. DIVERGENCE), computed ON THE DEVICE
 * from the stored bits (fp16 storage: the fp16 bits) and each element's GLOBAL position: a sum over the elements of a 64-bit mix of
 * (bits, global element index), twice with different seeds.  The sum does not depend on how the planes are spread over contexts, so
 * a slab rank's digest of its owned planes equals the single-domain context's digest of the same planes if and only if (to 2^-128)
 * the fields agree bit for bit -- what `bench.py --gpus N` certifies its timed steps with, without reading 0.5 GB per rank back.
 * The planes must be owned by this context (FX_E_INVALID otherwise); z_count = 0 = all owned planes from z_begin = the first.
 * Blocks like fx_download; FX_E_HALO while a halo fault is pending. */
int fx_field_digest(fx_ctx* ctx, int field, uint32_t z_begin, uint32_t z_count, uint64_t out[2]);

/* Checkpoint / resume (the reference keeps no state across runs).  One file holds what a later
 * fx_simulate depends on -- velocity[0], colour[parity], pressure (Fluid.cpp:360-384) -- for the WHOLE grid, dense fp32 in the
 * layouts above behind a 64-byte header ("FXCKPT01", X, Y, Z, storage, step count).  Every slab context stores / loads its own
 * planes at their offsets, so the ranks of a chain call these on the same path and a run may resume under another
 * decomposition.  fp16-storage contexts round-trip exactly.  Resuming continues bit-identically to the uninterrupted run. */
int fx_checkpoint_save(fx_ctx* ctx, const char* path);
int fx_checkpoint_load(fx_ctx* ctx, const char* path);

/* individual stages of Simulate, exposed for per-kernel parity tests and micro-benchmarks */
int fx_advect(fx_ctx* ctx, void* stream);
int fx_divergence(fx_ctx* ctx, void* stream);
int fx_jacobi(fx_ctx* ctx, void* stream, uint32_t iters);
int fx_project(fx_ctx* ctx, void* stream);

/* Vorticity confinement (Fedkiw, Stam, Jensen 2001; no reference counterpart -- the reference's only swirl is the fixed term inside its
 * impulse, CSAdvect.hlsl:63-65).  The semi-Lagrangian step wears the small eddies down; with epsilon > 0 fx_simulate runs one more pass
 * between the advection and the divergence, on the advected velocity u = VELOCITY1, in index space like the divergence and the projection
 * (unit cell spacing, neighbour indices clamped to the grid; D = half the difference of the two clamped neighbours):
 *   w = curl u      m = |w|      g = grad m      u' = u + (g x w) * (epsilon * dt) / (|g| + 1e-6)
 * fp32, every operation rounded on its own (tests/vorticity_ref.py restates it in numpy, bit for bit); fp16 storage widens on load and rounds
 * u' once (RNE).  2-D grids: w = (0, 0, wz), uz is left alone.  epsilon multiplies N x w per cell: on a cubic grid Fedkiw's eps * h * (N x w);
 * non-cubic grids are treated in index space like the divergence.  The pass is explicit: keeping epsilon * dt small enough for the flow at
 * hand is the caller's business.
 * fx_set_vorticity_confinement: 0 = off (default): every call behaves exactly as without this function.  Configuration like the scene depth:
 * kept across fx_update_frame, not checkpointed (set it again after fx_checkpoint_load), not part of fx_field_digest.  FX_E_INVALID for a
 * negative or non-finite epsilon and for a context that owns fewer planes than the grid (slab ranks, over RCCL or in-process groups, are
 * out of scope: the pass would need two planes of all three VELOCITY1 components across each face); FX_E_STATE for FX_FLAG_RENDER_ONLY.
 * fx_confine_vorticity: the stage alone, beside fx_advect / fx_divergence / fx_jacobi / fx_project (parity tests, micro-benchmarks), with
 * the context's epsilon and the time step of the last fx_update_frame; nothing (FX_OK) while either is 0.  The pass cannot run in place:
 * it writes the buffer behind FX_FIELD_VELOCITY and the two names swap, so afterwards FX_FIELD_VELOCITY1 is the confined field and
 * FX_FIELD_VELOCITY is unspecified until the next fx_project (or fx_simulate) has written it.
 * Timing: the pass finishes the advected velocity, its time is booked into fx_timing.advect_ms. */
int fx_set_vorticity_confinement(fx_ctx* ctx, float epsilon);
int fx_confine_vorticity(fx_ctx* ctx, void* stream);

/* Smoke sources (no reference counterpart: the reference's only source is the impulse compiled into its advection, CSAdvect.hlsl:59-68 /
 * Impulse.hlsli -- a Gaussian ball at (0.5, 0.1, 0.5), radius 1/16 (2-D: 1/32), colour rate (8, 16, 40, 40), lift 192 (2-D: 48), swirl 200).
 * fx_set_emitters gives the context a list of such balls with every constant an argument; with a non-empty list fx_simulate runs one more
 * pass (one launch, over the cells the balls cover, not over the grid) between the advection and the vorticity confinement / divergence,
 * in place on VELOCITY1 and COLOR.  Per cell (x, y, z) and emitter e, in list order, fp32 in the built-in's own operation order:
 *   p = ((x + .5) / X, (y + .5) / Y, (z + .5) / Z)      d = p - e.center (2-D grids: dz = 0)      d2 = fma(dz, dz, fma(dy, dy, dx * dx))
 *   basis = exp2(((d2 * -4) / (radius * radius)) * 1.44269502)
 *   if (basis >= e^-4) {      -- i.e. within `radius` of the centre
 *       F = 3-D: (fma(basis, fx, dz * -swirl), fma(basis, fy, 0), fma(basis, fz, dx * swirl))      2-D: (basis * fx, basis * fy, 0)
 *       u = fma(F, dt, u)      c[i] = saturate(fma(basis * dt, color_rate[i], c[i]))
 *   }
 * (tests/emitter_ref.py restates it in numpy.)  An emitter with the built-in's constants forms the built-in's basis bit for bit.  One
 * documented difference: the built-in adds in front of the step's attenuation max(1 - 0.2 dt, 0), an emitter behind it -- what an emitter
 * injects is not attenuated in the step that injects it.  fp16 storage widens on load and rounds each stored value once (RNE) behind the
 * last emitter; a cell in no emitter's support keeps its bits.  The list travels with the launch (no device memory, no copy, no
 * synchronisation): a moving source is a new fx_set_emitters per frame and costs nothing on the device.
 * fx_set_emitters: count 0 (list may be NULL) = none, the default: every call behaves exactly as without this function.  FX_E_INVALID,
 * the previous list staying in force, for a wrong struct_size, count > FX_MAX_EMITTERS, a non-finite member, radius <= 0, a negative
 * color_rate and unknown flag bits.  fx_get_emitters: the list in force -- *count gets its length, out (may be NULL with capacity 0) the
 * first min(capacity, length) entries.
 * fx_set_impulse: 0 switches the reference's built-in source off (a uniform flag in the advection kernels), so that the emitters are the
 * only sources; default 1.
 * Configuration like the vorticity confinement: per context, kept across fx_update_frame, not checkpointed (set it again after
 * fx_checkpoint_load), not part of fx_field_digest.  fx_set_emitters and fx_set_impulse(0) return FX_E_INVALID for a context that owns
 * fewer planes than the grid (slab ranks, over RCCL or in-process groups, on the same footing as the confinement: the overlapped schedule
 * sends the colour halos right behind the advection, and ordering an in-place pass against that exchange is work of its own); all four
 * calls return FX_E_STATE for FX_FLAG_RENDER_ONLY contexts.
 * fx_emit: the stage alone, beside fx_advect / fx_confine_vorticity (fx_advect does not include it), with the time step of the last
 * fx_update_frame; nothing (FX_OK) with an empty list or dt <= 0.  Timing: booked into fx_timing.advect_ms. */
#define FX_MAX_EMITTERS 16u
typedef struct fx_emitter {
	uint32_t struct_size, flags;   /* flags: 0 (unknown bits: FX_E_INVALID) */
	float center[3];               /* the simulation's texture space [0,1]^3: cell (x,y,z) sits at ((x+.5)/X, (y+.5)/Y, (z+.5)/Z); may lie outside the volume */
	float radius;                  /* same space; support = cells with basis >= e^-4, i.e. within `radius` of the centre */
	float color_rate[4];           /* rgba added per unit time at the centre (built-in: 8, 16, 40, 40); >= 0 */
	float force[3];                /* acceleration at the centre, scaled by basis (built-in: 0, 192, 0; 2-D: 0, 48, 0) */
	float swirl;                   /* adds swirl * (-dz, 0, dx), NOT scaled by basis, inside the support (built-in: 200; ignored on 2-D grids) */
} fx_emitter;
int fx_set_emitters(fx_ctx* ctx, const fx_emitter* list, uint32_t count);
int fx_get_emitters(fx_ctx* ctx, fx_emitter* out, uint32_t capacity, uint32_t* count);
int fx_set_impulse(fx_ctx* ctx, int enabled);
int fx_emit(fx_ctx* ctx, void* stream);

/* Solid obstacles inside the box (no reference counterpart: the reference's only boundaries are the six walls -- the clamped neighbour indices
 * of its divergence, relaxation and projection; voxelised solids after Harris / Crane et al., GPU Gems 3 ch. 30).  fx_set_obstacles gives the
 * context a mask S = uint8[Z][Y][X], non-zero = solid, resting (velocity 0).  The wall rule is "a neighbour that is not there reads as the cell
 * itself"; a solid extends it to neighbours inside an obstacle.  In index space, n-a / n+a = the neighbours of cell c along axis a with the
 * index clamped to the grid exactly as without obstacles, every operation rounded as in the plain stages:
 *   enforce     (a pass of its own behind the advection and the emitters, in front of the confinement; dt > 0 only) a solid cell's VELOCITY1 and
 *               COLOR components become +0; fluid cells keep their bits
 *   divergence  b = 0.5 * (ddz + (ddy + ddx)) (2-D: ddx + ddy), dd = -v(n-) + v(n+) with v(n) read as S(n) ? 0 : v(n); b = 0 in a solid cell
 *   relaxation  ((((((L - b) + R) + U) + D) + F) + B) * (1/6) (2-D: four terms, * 0.25), each neighbour S(n) ? p(c) : p(n); 0 in a solid cell
 *   projection  grad_a = -(S(n-) ? p(c) : p(n-)) + (S(n+) ? p(c) : p(n+)), u[a] = fma(-grad_a, k, u[a]); then u[a] = 0 where S(n-a) | S(n+a)
 *               (free slip against a resting solid); then the wall damping; 0 in all three components of a solid cell
 * With an all-zero mask the three stages are, operation for operation, the plain ones (tests/obstacle_ref/ restates all four in C++).
 * The stages read one code byte per cell, built on the device once per call (one upload + one launch: a moving obstacle is a new call per
 * frame); the pressure solve then runs one obstacle-aware sweep per launch and ignores FX_FLAG_JACOBI_FUSE_MASK.
 * The marches are unchanged: a solid cell holds no smoke.  The solids themselves are drawn by fx_set_obstacle_draw / fx_draw_obstacles below, which
 * ray-cast the mask into the render target and a depth buffer for fx_set_scene_depth; a caller with a rasteriser of its own may still draw the
 * object itself and pass its depth.
 * fx_set_obstacles: replaces the previous mask; NULL detaches (`bytes` is ignored): every call behaves exactly as without this function.  An
 * all-zero mask is legal and keeps the obstacle kernels in force.  flags & FX_OBSTACLES_DEVICE: `solid` is device memory of the context's
 * device, read by work enqueued on `stream` during this call only; otherwise host memory.  The call returns once the mask has been read;
 * set it on the stream the steps run on (or synchronise in between).  FX_E_INVALID, the previous mask staying in force, for bytes != X * Y * Z,
 * unknown flag bits, a context that owns fewer planes than the grid (slab ranks of every transport, on the same footing as the confinement)
 * and FX_JACOBI_FAITHFUL contexts (the per-cell freeze solve with obstacles is out of scope: its sparse solver has no obstacle-aware kernels);
 * FX_E_STATE for FX_FLAG_RENDER_ONLY; FX_E_NOMEM if the code volume cannot be allocated.
 * fx_get_obstacles: the mask in force as 0 / 1 per cell (all 0 when none) and the count of solid cells; either out may be NULL; blocks like
 * fx_download.  FX_E_INVALID for bytes != X * Y * Z with solid_out set.
 * Configuration like the confinement and the emitters: per context, kept across fx_update_frame, not checkpointed (set it again after
 * fx_checkpoint_load), not part of fx_field_digest.
 * fx_enforce_obstacles: the enforce stage alone, beside fx_emit, with the time step of the last fx_update_frame; nothing (FX_OK) with no
 * obstacles or dt <= 0.  fx_divergence / fx_jacobi / fx_project take the obstacle kernels while a mask is set.
 * Timing: the enforce pass is booked into fx_timing.advect_ms; jacobi_launches = jacobi_sweeps with a mask. */
#define FX_OBSTACLES_DEVICE 0x1u
int fx_set_obstacles(fx_ctx* ctx, void* stream, const uint8_t* solid, size_t bytes, uint32_t flags);
int fx_get_obstacles(fx_ctx* ctx, uint8_t* solid_out, size_t bytes, uint64_t* solid_cells);
int fx_enforce_obstacles(fx_ctx* ctx, void* stream);

/* Solids that move: rigid-body velocities for the voxel mask (the other half of the Harris / Crane et al. scheme: the solid's velocity enters
 * the divergence and the boundary rule of the projection).  The mask stays what it is -- any non-zero byte is solid, and a moving object is a
 * new fx_set_obstacles per frame --; fx_set_obstacle_bodies says how fast the solids under it move, so that they push the air in front of
 * them and drag it behind them.  A body claims solid cells by a box: with pos_a(n) = ((float)i_a + 0.5f) / (float)N_a, the advection's cell
 * centre, B(n) = the first body of the list with box_lo[a] <= pos_a(n) && pos_a(n) <= box_hi[a] on every axis (a 2-D grid ignores z); none if
 * no box holds the cell.  With r = pos(n) - pivot the velocity of solid cell n is w(n) = linear + angular x r, in this order:
 *   w_x = fmaf(angular_y, r_z, fmaf(-angular_z, r_y, linear_x))
 *   w_y = fmaf(angular_z, r_x, fmaf(-angular_x, r_z, linear_y))
 *   w_z = fmaf(angular_x, r_y, fmaf(-angular_y, r_x, linear_z))
 *   2-D grids: only angular_z acts: w_x = fmaf(-angular_z, r_y, linear_x), w_y = fmaf(angular_z, r_x, linear_y), w_z = +0
 *   w(n) = +0 where B(n) is none: a solid in no box rests
 * S and the clamped neighbours n-a / n+a are those of the obstacle block above, and so is every operation not named here:
 *   enforce     a solid cell's VELOCITY1 becomes w(c), rounded once to the storage; its COLOR (and the render's alpha) become +0 as before
 *   divergence  v_a(n) read as S(n) ? w_a(n) : v_a(n) (w in fp32, not as stored); b = 0 in a solid cell
 *   relaxation  unchanged: the pressure ghost of a moving wall is still the cell's own pressure
 *   projection  the gradient as before; then, where S(n-a) | S(n+a): u[a] = 0.5f * (w_a(n-a) + w_a(n+a)) if both are solid, otherwise the one
 *               solid neighbour's w_a (free slip against a moving wall: the normal component is the wall's); then the wall damping, with the
 *               open-face exception of fx_set_open_walls; a solid cell's three components become w(c)
 *   the other stages (heat, inflow, emitters, confinement, both advection schemes) are unchanged: they see the bodies only through the
 *               velocity the enforce pass and the projection leave in solid cells -- the advection's taps into a solid drag the air with it
 * (tests/moving_obstacle_ref.py restates the rules in numpy.)  Velocities are in texture units per unit time, the unit of FX_FIELD_VELOCITY
 * (the advection traces pos - v * dt).  A rotation given in texture space is rigid in world space only on axes of equal extent: on a grid
 * whose box is no cube the caller scales angular and pivot per axis pair, or accepts the shear.
 * The list is configuration on the emitters' terms: a host-side list per context (it travels with the launches: no device memory, no copy),
 * kept across fx_update_frame, not checkpointed, not part of fx_field_digest.  count 0 (list may be NULL) is the default, "every solid
 * rests": every call then runs exactly the launches it runs without this function.  The list may be set with or without a mask in force and
 * takes effect once one is (as heat sources wait for buoyancy); it does not depend on the order of the two calls.  A cell inside several
 * boxes belongs to the first body in list order.  The library does not move the mask (fx_set_obstacle_meshes below rasterises it from meshes,
 * where the caller's transform says), and no force acts on the body.
 * fx_set_obstacle_bodies: FX_E_INVALID, the previous list staying in force, for count > FX_MAX_OBSTACLE_BODIES, count with a NULL list, a wrong
 * struct_size, non-zero flags, a non-finite member, box_lo[a] > box_hi[a], a context that owns fewer planes than the grid (slab ranks of every
 * transport) and FX_JACOBI_FAITHFUL contexts (fx_set_obstacles refuses them too); FX_E_STATE for FX_FLAG_RENDER_ONLY.
 * fx_get_obstacle_bodies: as fx_get_emitters (slab ranks may ask: the list is empty there). */
#define FX_MAX_OBSTACLE_BODIES 16u
typedef struct fx_obstacle_body {
	uint32_t struct_size, flags;   /* sizeof(fx_obstacle_body) = 68; flags must be 0 */
	float box_lo[3], box_hi[3];    /* texture space: the solid cells whose CENTRE lies in this closed box belong to the body */
	float linear[3];               /* velocity of the pivot, texture units per unit time */
	float angular[3];              /* angular velocity about the pivot, radians per unit time, texture space */
	float pivot[3];                /* texture space */
} fx_obstacle_body;
int fx_set_obstacle_bodies(fx_ctx* ctx, const fx_obstacle_body* list, uint32_t count);
int fx_get_obstacle_bodies(fx_ctx* ctx, fx_obstacle_body* out, uint32_t capacity, uint32_t* count);

/* The mask from triangle meshes: a solid voxeliser on the device (fx_voxelize.hip).  fx_set_obstacle_meshes voxelises up to
 * FX_MAX_OBSTACLE_MESHES closed triangle meshes into solid sets, ORs them into one mask and installs it exactly as
 * fx_set_obstacles(ctx, stream, mask, X * Y * Z, FX_OBSTACLES_DEVICE) would: the same code volume, count and bounding box, the same "returns
 * once the inputs have been read" (it blocks like fx_set_obstacles), the same configuration terms.  fx_get_obstacles then returns the
 * voxelised mask, fx_set_obstacles(NULL) detaches it, fx_set_obstacle_bodies acts on it unchanged.  A rigidly animated object costs its
 * 48-byte transform per frame: with FX_MESH_DEVICE the positions and indices stay where they are.
 * The rule is exact integer arithmetic behind one rounding per coordinate (tests/voxelize_ref.py restates it in numpy).  With N = (X, Y, Z),
 * per position v and axis a:
 *   1 transform   with a transform m: p_a = ((m[4a] * v_x + m[4a+1] * v_y) + m[4a+2] * v_z) + m[4a+3], every multiply and add rounded to fp32
 *                 on its own (no fused multiply-add); without one p_a = v_a, bits untouched
 *   2 quantise    to 1 / 256 of a cell: t = p_a * (float)(256 * N_a) rounded to fp32, clamped to [-262144, 262144]; q_a = (int)rintf(t)
 *                 (ties to even).  Cell i's centre is 256 i + 128.  A triangle is SKIPPED (skipped_triangles += 1) if one of its indices is
 *                 >= vertex_count or a transformed coordinate p_a of one of its vertices is not finite
 *   3 triangle    (a, b, c) quantised, int64 from here: A = (b_y - a_y)(c_z - a_z) - (b_z - a_z)(c_y - a_y).  A = 0: the triangle is edge-on,
 *                 covers no column and contributes nothing (this is not "skipped").  A < 0: swap b and c and negate A
 *   4 column      (j, k) with P = (256 j + 128, 256 k + 128) is COVERED iff for each directed edge p -> r of a -> b, b -> c, c -> a, with
 *                 dy = r_y - p_y, dz = r_z - p_z, E = dy (P_z - p_z) - dz (P_y - p_y):  E > 0, or E == 0 and (dy > 0 or (dy == 0 and dz > 0)).
 *                 The tie rule is the sample shifted by (-eps^2, +eps): a shared edge or vertex counts exactly once, whatever the triangle
 *                 order or winding
 *   5 toggle      with e1 = b - a, e2 = c - a: n_y = e1_z e2_x - e1_x e2_z, n_z = e1_x e2_y - e1_y e2_x,
 *                 T = (a_x - 128) A - (n_y (P_y - a_y) + n_z (P_z - a_z)), i0 = clamp(ceil(T / (256 A)), 0, X) with the ceiling of the exact
 *                 quotient.  The triangle toggles covered column (j, k) at i0; index X is a virtual cell beyond the +x wall
 *   6 fill        per mesh, solid(i, j, k) = XOR over t <= i of toggles(t, j, k), for i < X.  open_columns counts, summed over the meshes,
 *                 the columns whose number of toggles INCLUDING index X is odd: 0 for a watertight mesh wherever it lies, also across a wall
 *   7 union       mask = OR over the meshes; solid_cells = what fx_set_obstacles counts
 * The result does not depend on the order of the triangles, of the vertices within one, or on the winding.  Bad geometry is never an error
 * (device meshes cannot be looked at up front): it is defined by the rule and counted in the report.  Magnitudes: |q| <= 2^18, |A|, |n| < 2^40,
 * |T| < 2^61.
 * positions: texture space, cell (x, y, z)'s centre = ((x + .5) / X, (y + .5) / Y, (z + .5) / Z).  A mesh with triangle_count == 0 is legal
 * and contributes nothing (positions and indices may then be NULL); meshes that leave every cell empty install an all-zero mask, which keeps
 * the obstacle kernels in force.  flags & FX_MESH_DEVICE: positions, indices and transform are device memory of the context's device, read
 * by work enqueued on `stream` during this call only; otherwise host memory.  report may be NULL.
 * FX_E_INVALID, the previous mask staying in force, for count == 0 (detaching stays fx_set_obstacles(NULL)) or > FX_MAX_OBSTACLE_MESHES, a
 * NULL list, a wrong struct_size, unknown flag bits, NULL positions or indices with triangle_count > 0, 2-D grids, and the contexts
 * fx_set_obstacles refuses (slab ranks, FX_JACOBI_FAITHFUL); FX_E_STATE for FX_FLAG_RENDER_ONLY and while the multigrid solver is selected;
 * FX_E_NOMEM if the code volume or the voxeliser's scratch (a bitmap of X / 32 + 1 words per row, 16 bytes per triangle, a host mesh's copy)
 * cannot be allocated.  The scratch is allocated by the first call and freed with the context. */
#define FX_MAX_OBSTACLE_MESHES 16u
#define FX_MESH_DEVICE 0x1u          /* positions / indices / transform are device memory of the context's device */
typedef struct fx_obstacle_mesh {
	uint32_t struct_size, flags;     /* sizeof(fx_obstacle_mesh); FX_MESH_DEVICE or 0 */
	const float* positions;          /* float[vertex_count][3], texture space */
	const uint32_t* indices;         /* uint32[triangle_count][3] */
	uint32_t vertex_count, triangle_count;
	const float* transform;          /* float[12], row-major 3x4 applied to every position; NULL = none */
} fx_obstacle_mesh;
typedef struct fx_mesh_report { uint64_t solid_cells; uint32_t open_columns, skipped_triangles; } fx_mesh_report;
int fx_set_obstacle_meshes(fx_ctx* ctx, void* stream, const fx_obstacle_mesh* meshes, uint32_t count, fx_mesh_report* report);

/* Open walls (no reference counterpart: the reference's box is closed on all six faces -- the clamped neighbour indices of its stages and the
 * wall damping of its projection).  fx_set_open_walls names the faces through which the smoke may leave; the step is then
 *   advect -> inflow -> emit -> heat -> enforce -> confine -> divergence -> relaxation -> projection.
 * "Beyond an open face" = a stencil neighbour whose UNCLAMPED index is -1 or N on an axis whose face there is open.  Rule by rule, every
 * operation rounded as written, S = the obstacle mask (all 0 without one), n-a / n+a as in the obstacle block above:
 *   divergence  unchanged (the plain or the obstacle one): the clamped neighbour is the zero-gradient velocity ghost already
 *   relaxation  ((((((L - b) + R) + U) + D) + F) + B) * (1/6) (the constant 0x3e2aaaab; 2-D: four terms, * 0.25), each neighbour read as
 *               beyond an open face ? +0 : S(n) ? p(c) : p(n)   -- a Dirichlet ghost p = 0; 0 in a solid cell
 *   projection  grad_a = -q(n-) + q(n+) with the same q, u[a] = fma(-grad_a, k, u[a]); then the free-slip rule of the obstacles; then the wall
 *               damping, which is skipped for axis a (factor 1) when pos < 0 and the low face of a is open or pos > 0 and the high face is
 *               (pos = the cell centre in [-1, 1], as the plain projection forms it); 0 in all three components of a solid cell
 *   inflow      a pass of its own directly behind the advection and in front of the emitters, dt > 0 only: the ghost cells beyond an open face
 *               hold clear air.  Per axis with u0 = VELOCITY (the field the advection traced with), exactly as the buoyancy's step 1:
 *                 p = (i + .5) / N      a = fma(-u0, dt, p)      t = a * N - 0.5      i0 = floor(t)      f = t - i0
 *                 low face open:   w_a = 0 if i0 < -1,   f if i0 == -1,        else 1
 *                 high face open:  w_a = 0 if i0 >= N,   1 - f if i0 == N - 1, else 1          (an axis with no open face: w_a = 1)
 *                 w = (w_x * w_y) * w_z (2-D grids: w_x * w_y)      COLOR[c] = COLOR[c] * w, all four channels
 *               an fp32 multiply; fp16 storage widens on load and rounds each channel once (RNE); a cell with w == 1 keeps its bits.
 *               In real arithmetic this IS the advection's sample with zero ghost taps wherever both taps of an axis clamp onto the edge
 *               cell (weights 1 - f and f on one value), and the same holds under mirror addressing (-1 -> 0, N -> N - 1).  The velocity
 *               keeps its clamped (zero-gradient) sample.  The built-in impulse adds inside the advection, in front of this pass: what it
 *               adds to a cell is scaled with the cell (an emitter's contribution, added behind the pass, is not).
 *   temperature (fx_set_buoyancy) the ghost is at ambient: between its steps 1 and 2 the buoyancy pass forms Ts = fma(w, Ts - Ta, Ta) with w
 *               from the i0 and f it already holds.  With all faces closed its arithmetic is unchanged.
 * fx_set_open_walls: faces = a set of FX_WALL_* bits; 0 = all closed, the default: every call behaves exactly as without this function.
 * FX_E_INVALID, the previous setting staying in force, for bits above 0x3F, a z bit on a 2-D grid, a context that owns fewer planes than
 * the grid (slab ranks of every transport, on the obstacles' footing) and FX_JACOBI_FAITHFUL contexts (the freeze solve has no such
 * kernels); FX_E_STATE for FX_FLAG_RENDER_ONLY (all three calls).  Obstacles, emitters, buoyancy, confinement, 2-D grids, both storages and
 * both address modes are served together with open walls; without a mask the open kernels read no code byte.
 * As with obstacles the pressure solve then runs one sweep per launch and ignores FX_FLAG_JACOBI_FUSE_MASK (jacobi_launches = jacobi_sweeps).
 * Configuration like the confinement: per context, kept across fx_update_frame, not checkpointed (set it again after fx_checkpoint_load),
 * not part of fx_field_digest.
 * fx_open_inflow: the inflow stage alone, beside fx_emit / fx_heat (fx_advect does not include it), with the time step of the last
 * fx_update_frame; nothing (FX_OK) with all faces closed or dt <= 0.  fx_jacobi / fx_project / fx_heat follow the setting.
 * Timing: the inflow pass is booked into fx_timing.advect_ms.
 * Out of scope: open walls on slab ranks; open walls in faithful mode; several open-wall sweeps per launch; velocity ghosts other than
 * zero-gradient; checkpointing the setting. */
#define FX_WALL_X_LO 0x01u   /* the code byte's order: x-, x+, y-, y+, z-, z+ */
#define FX_WALL_X_HI 0x02u
#define FX_WALL_Y_LO 0x04u
#define FX_WALL_Y_HI 0x08u   /* "up" for the built-in impulse and fx_buoyancy's default */
#define FX_WALL_Z_LO 0x10u
#define FX_WALL_Z_HI 0x20u
int fx_set_open_walls(fx_ctx* ctx, uint32_t faces);
int fx_get_open_walls(fx_ctx* ctx, uint32_t* faces);
int fx_open_inflow(fx_ctx* ctx, void* stream);

/* Buoyancy (Fedkiw, Stam, Jensen 2001, eq. 8; no reference counterpart -- the reference's only lift is the constant force inside its impulse
 * ball): a temperature T that is advected with the flow, cools towards an ambient value and, with the smoke density rho = COLOR.w, pushes
 * the velocity along `up`:   f = (-density_weight * rho + lift * (T - ambient)) * up.   With buoyancy on, fx_simulate runs one more pass
 * (one launch over the grid) behind the emitters and in front of the obstacle enforce pass, the confinement and the divergence:
 * advect -> emit -> heat -> enforce -> confine -> divergence ...   Per cell (x, y, z), fp32, every operation rounded as written
 * (tests/buoyancy_ref.py restates it in numpy), u0 = VELOCITY (the velocity the step's advection traced with), Ta = ambient:
 *   1  p = ((x + .5) / X, (y + .5) / Y, (z + .5) / Z)      a = fma(-u0, dt, p)      t = a * N - 0.5, i0 = floor(t), f = t - i0 per axis;
 *      the eight taps i0, i0 + 1 go through the context's address mode (clamp / mirror), Ts = lerp_z(lerp_y(lerp_x ...)) with
 *      lerp(a, b, f) = fma(f, b - a, a): the back-trace and the sampler of the colour advection, tap for tap (2-D grids: both z taps are plane 0)
 *   2  T1 = fma(Ts - Ta, max(fma(-dt, cooling, 1), 0), Ta)
 *   3  for every heat source e in list order: basis as an emitter forms it (d = p - e.center, 2-D grids: dz = 0,
 *      basis = exp2(((d2 * -4) / (radius * radius)) * 1.44269502));   if (basis >= e^-4) T1 = fma(basis * dt, e.rate, T1)      -- no clamp
 *   4  a solid cell (fx_set_obstacles) gets T1 = Ta and its velocity is left alone (the enforce pass behind clears it)
 *   5  T1 is stored into the second temperature buffer and the two swap
 *   6  fluid cells: s = fma(lift, T1 - Ta, -(density_weight * rho)), rho = COLOR.w as stored (what the emitters added included), and for
 *      each axis a with up[a] != 0 (2-D grids: never z):   VELOCITY1[a] = fma(up[a] * s, dt, VELOCITY1[a]);   a component with up[a] == 0
 *      is neither read nor written.  fp16 storage widens on load and rounds the stored component once (RNE).
 * The field: the first successful fx_set_buoyancy allocates two fp32 volumes of X * Y * Z (fp32 whatever fx_desc.storage is), both filled
 * with `ambient`; FX_E_NOMEM if that fails.  A later call replaces the coefficients and keeps the field; NULL switches the feature off (the
 * default: every call behaves exactly as without this function) and frees the field.  While buoyancy is on, fx_upload / fx_download /
 * fx_field_bytes serve FX_FIELD_TEMPERATURE; while it is off they return FX_E_STATE (fx_field_bytes: 0).  fx_field_digest does not take it.
 * Configuration like the emitters: per context, kept across fx_update_frame, not part of fx_field_digest.  The checkpoint file does not hold
 * the temperature: a caller who resumes calls fx_set_buoyancy (and fx_set_heat_sources) again behind fx_checkpoint_load and uploads the
 * FX_FIELD_TEMPERATURE they downloaded when they saved; the run then continues bit-identically.
 * fx_set_heat_sources: count 0 (list may be NULL) = none, the default.  The list may be set while buoyancy is off and takes effect once it
 * is on.  It travels with the launch like the emitters (no device memory, no copy).  A cold source (rate < 0) is legal.
 * FX_E_INVALID, the previous setting staying in force: a wrong struct_size, unknown flag bits, a non-finite member, a negative
 * density_weight or cooling, `up` all zero, radius <= 0, count > FX_MAX_HEAT_SOURCES, and (both setters, fx_heat) a context that owns fewer
 * planes than the grid -- slab ranks of every transport, on the same footing as the confinement: the field would need halo planes of its
 * own.  FX_E_STATE (all five calls): FX_FLAG_RENDER_ONLY contexts.  Both Jacobi modes, 2-D grids, both address modes and obstacles are served.
 * fx_get_buoyancy: *enabled gets 0 / 1 and *out the coefficients in force (the defaults while off); either may be NULL.
 * fx_get_heat_sources: as fx_get_emitters.
 * fx_heat: the stage alone, beside fx_emit, with the time step of the last fx_update_frame; nothing (FX_OK) while buoyancy is off or
 * dt <= 0.  It reads FX_FIELD_VELOCITY, so it must run BEFORE fx_confine_vorticity, which leaves that field unspecified.
 * Timing: booked into fx_timing.advect_ms. */
#define FX_MAX_HEAT_SOURCES 16u
typedef struct fx_buoyancy {
	uint32_t struct_size, flags;   /* flags: 0 (unknown bits: FX_E_INVALID) */
	float ambient;                 /* T_amb; the field starts at this value everywhere */
	float density_weight;          /* alpha >= 0: pulls smoke (COLOR.w) down along -up */
	float lift;                    /* beta: pushes (T - T_amb) along up; any finite value */
	float cooling;                 /* >= 0, per unit time: T relaxes to ambient by max(1 - cooling * dt, 0) per step */
	float up[3];                   /* direction of "up" in grid axes, used as given (not normalised); default (0, 1, 0) */
} fx_buoyancy;
typedef struct fx_heat_source {
	uint32_t struct_size, flags;   /* flags: 0 (unknown bits: FX_E_INVALID) */
	float center[3];               /* texture space, as fx_emitter.center */
	float radius;                  /* > 0, as fx_emitter.radius */
	float rate;                    /* temperature per unit time at the centre; any finite value */
} fx_heat_source;
int fx_set_buoyancy(fx_ctx* ctx, const fx_buoyancy* buoyancy);
int fx_get_buoyancy(fx_ctx* ctx, fx_buoyancy* out, int* enabled);
int fx_set_heat_sources(fx_ctx* ctx, const fx_heat_source* list, uint32_t count);
int fx_get_heat_sources(fx_ctx* ctx, fx_heat_source* out, uint32_t capacity, uint32_t* count);
int fx_heat(fx_ctx* ctx, void* stream);

/* Tracer particles and point queries (no reference counterpart: the reference carries nothing but its grid fields with the flow).  Embers, ash,
 * debris: points that ride the velocity field, moved on the device by one gather kernel (fx_particles.hip), and their smaller sibling, "what
 * is the wind at these points?" (fx_sample_velocity).  Particles are passive: the stage reads VELOCITY and the obstacle code and writes the
 * particle buffer only; no field of the simulation changes by a bit because particles exist.
 * A record is float[4] = (x, y, z, age).  x, y, z lie in texture space [0,1]^3, the space of fx_emitter.center: cell (i, j, k)'s centre is
 * ((i + .5) / X, (j + .5) / Y, (k + .5) / Z).  age >= 0 is a live particle, in seconds; a record whose age is not >= 0 (negative or NaN) is
 * DEAD: the stage leaves every bit of it alone.  The caller respawns by writing records, with fx_set_particles or through the pointer of
 * fx_particles_device on the stream the steps run on.
 * The rule, fp32, every operation rounded as written (tests/particle_ref.py restates it in numpy).  N = (X, Y, Z), dt = the time step of the
 * last fx_update_frame, c(v) = fminf(fmaxf(v, 0), 1): a NaN becomes 0 (and -0 becomes +0), so no value, however wild, reaches an index
 * computation unclamped -- that is what makes a record the caller wrote safe to read.
 *   sampler U(p)  per axis a: s = c(p_a), t = s * N_a - 0.5, fl = floor(t), f = t - fl; the taps (int)fl and (int)fl + 1 are CLAMPED to
 *                 [0, N_a - 1] whatever fx_desc.advect_address is (with s in [0,1] clamp and mirror address the same cells).  Each of the
 *                 three component planes of VELOCITY is read with the advection's colour sampler, lerp(a, b, f) = fma(f, b - a, a), in
 *                 the order x, then y, then z; fp16 storage widens each tap on load.  2-D grids: both z taps are plane 0, the z lerp runs
 *                 on equal operands; all three components are returned
 *   move, per live record (p, age):
 *   1  k1 = U(p) + drift
 *   2  FX_PARTICLE_MIDPOINT: m_a = c(fma(k1_a, 0.5 * dt, p_a)), k = U(m) + drift;   FX_PARTICLE_EULER: k = k1
 *   3  q_a = fma(k_a, dt, p_a).  On a 2-D grid z is left alone altogether: q_z = p_z, bits kept, and rules 4 to 6 pass it by
 *   4  open walls (fx_set_open_walls): q_a < 0 with the low face of a open, or q_a > 1 with the high face open: the record dies
 *   5  q_a = c(q_a): a closed wall holds the particle on it
 *   6  with a mask set (fx_set_obstacles): the cell i_a = min((int)(q_a * N_a), N_a - 1); if it is solid the position stays p, bits kept --
 *      a particle does not enter a solid, and one that a moving solid has run over stays put until the solid has passed
 *   7  age1 = age + dt;  lifetime > 0 and age1 >= lifetime: the record dies
 *   8  stored: (the position of rule 5 or 6, a dying record's age = -1, a surviving one's = age1)
 * fx_simulate runs the stage behind the projection, on the projected VELOCITY, when the time step is > 0 and a set exists; the step then
 * never allocates, copies or synchronises for it (a captured fx_simulate stays capturable).  fx_move_particles is that stage alone: nothing
 * (FX_OK) with no set or dt <= 0.  Timing: booked into fx_timing.project_ms.
 * fx_set_particles replaces the set: records = float[count][4], host memory, or with FX_PARTICLES_DEVICE device memory of the context's device
 * read by a copy enqueued on `stream`.  All allocation happens here; it returns once the records have been read.  count 0 (records may be
 * NULL) frees the buffer and restores the default: every call then behaves exactly as without this function.
 * fx_get_particles blocks like fx_download: *count gets the set's size, out (may be NULL with capacity 0) the first min(capacity, *count) records.
 * fx_particles_device: the context's own buffer and count, for zero-copy drawing and respawning; valid until the next fx_set_particles or
 * fx_destroy; (NULL, 0) with no set.  Either out-pointer may be NULL.
 * fx_set_particle_params: NULL restores the defaults (midpoint, no drift, immortal).  fx_get_particle_params: the setting in force.
 * fx_sample_velocity: points = float[count][4] (w is ignored: a particle buffer can be passed as it is), out = float[count][3] = U(point),
 * read from FX_FIELD_VELOCITY (behind fx_simulate: the projected field).  Host pointers: copy in, launch, copy out, block.  With
 * FX_PARTICLES_DEVICE both are device memory (points 16-byte aligned, out 4-byte): the launch is enqueued on `stream`, nothing else.
 * count 0 returns FX_OK.
 * Particles are caller data and configuration on the emitters' terms: per context, kept across fx_update_frame, not checkpointed (a caller
 * saves them with fx_get_particles), not part of fx_field_digest.
 * FX_E_INVALID, the previous state staying in force: a NULL ctx, a wrong struct_size, unknown flag bits, an unknown scheme, a non-finite
 * drift, a non-finite or negative lifetime, count > FX_MAX_PARTICLES, count with a NULL pointer, a misaligned device pointer, and (every
 * call but the three getters) a context that owns fewer planes than the grid -- slab ranks of every transport, on the confinement's footing;
 * the getters succeed there and report the empty default, as fx_get_emitters does.  FX_E_STATE: FX_FLAG_RENDER_ONLY contexts.  FX_E_NOMEM:
 * the buffer cannot be allocated.
 * Out of scope (drawing the particles: fx_set_particle_draw below; births on the device: fx_set_particle_spawners below): momentum deposit, i.e. drag back on the flow (smoke and heat the particles do leave behind:
 * fx_set_particle_trail below); sampling colour or temperature at points. */
#define FX_MAX_PARTICLES      (1u << 26)
#define FX_PARTICLES_DEVICE   0x1u      /* the pointer(s) are device memory of the context's device */
#define FX_PARTICLE_EULER     0u
#define FX_PARTICLE_MIDPOINT  1u        /* default */
typedef struct fx_particle_params {
	uint32_t struct_size, flags;   /* sizeof(fx_particle_params) = 28; flags: 0 */
	uint32_t scheme;               /* FX_PARTICLE_* */
	float drift[3];                /* added to the sampled velocity, texture space per second (settling ash: negative y); default 0 */
	float lifetime;                /* seconds; 0 = immortal (default); finite, >= 0 */
} fx_particle_params;
int fx_set_particles(fx_ctx* ctx, void* stream, const float* records, uint32_t count, uint32_t flags);
int fx_get_particles(fx_ctx* ctx, float* out, uint32_t capacity, uint32_t* count);
int fx_particles_device(fx_ctx* ctx, void** records, uint32_t* count);
int fx_set_particle_params(fx_ctx* ctx, const fx_particle_params* params);
int fx_get_particle_params(fx_ctx* ctx, fx_particle_params* out);
int fx_move_particles(fx_ctx* ctx, void* stream);
int fx_sample_velocity(fx_ctx* ctx, void* stream, const float* points, uint32_t count, float* out, uint32_t flags);

/* The particle sort (no reference counterpart).  The move above is a scattered gather: how fast it runs depends on the order of the buffer,
 * and a set in cell order moves many times faster than a shuffled one.  This stage sorts the buffer on the device: a
 * stable sort by cell with the dead records last, which also leaves the number of live records in device memory, so that respawning is an
 * append.  One stable radix sort of (key, index) pairs and one gather of the records (fx_particle_sort.hip); no atomic decides a position, the
 * result is the same bit for bit on every run.
 * The rule (tests/particle_sort_ref.py restates it in numpy), for a record r = (x, y, z, age) on a grid N = (X, Y, Z):
 *   live   iff age >= 0 -- the move's own test: a negative or NaN age is dead, -0.0 is live
 *   cell   per axis, fp32, each operation rounded as written: c_a = min((int)(c(p_a) * (float)N_a), N_a - 1), c(v) = fminf(fmaxf(v, 0), 1):
 *          the formula of the move's solid lookup (rule 6).  A NaN position lands in cell 0, 1.0 in N_a - 1.  A 2-D grid does not look at
 *          z: c_z = 0
 *   key    (c_z * Y + c_y) * X + c_x for a live record, X * Y * Z for a dead one; a uint32
 *   sort   the buffer becomes rec[order], order = the stable ascending permutation of the keys (numpy: argsort(key, kind="stable")).  Every
 *          record moves with all 128 bits intact: dead records keep their bits, NaN payloads included, and their relative order; live
 *          records of one cell keep theirs
 *   live   = the number of live records: behind a sort they occupy [0, live), the dead [live, count)
 * The buffer stays where it is: fx_particles_device returns the same pointer before and behind a sort, and it holds the sorted set.
 * fx_set_particle_sort: NULL = the default (off).  enabled = 1 allocates the sort's scratch for the set in force, and fx_set_particles
 * resizes it with every later set (FX_E_NOMEM there leaves the previous set and scratch in force); enabled = 0 frees it.  All allocation and
 * waiting happens in these two calls: fx_sort_particles and the step only enqueue (a captured fx_simulate stays capturable).  every = n > 0:
 * the particle stage (fx_simulate, fx_move_particles) sorts in front of the move on its 1st, (n+1)th, (2n+1)th ... run, counted from the last
 * fx_set_particles / fx_set_particle_sort, so the step that pays for the sort also gets the coherent gathers; every = 0: only
 * fx_sort_particles sorts.  Whether a run sorts is decided on the host when it is enqueued: a captured step replays what was captured,
 * with or without the sort, however often it is replayed.  Timing: booked into fx_timing.project_ms, like the move.
 * fx_sort_particles: the stage alone.  FX_OK and nothing done while no set exists.
 * fx_particle_sort_info waits for `stream`: live = what the last sort counted (0 before the first), sorts = sorts enqueued since the last
 * fx_set_particles / fx_set_particle_sort.  With sorting off both are 0.
 * fx_particle_order_device: the context's own device arrays.  order_u32[i] = the index the record now at i had before the last sort -- what
 * a caller needs to carry per-particle arrays of its own (colour, size, id) along, with a gather kernel on the same stream; valid once
 * sorts > 0, until the next sort or fx_set_particles (NULL while no set exists).  live_u32 = one uint32, rewritten by every sort.  Respawning:
 * a caller's kernel on the steps' stream reads *live_u32 and writes its new records to [live, count).
 * The sort reads and writes the particle buffer and its own scratch, nothing else: no field, no obstacle code.  Configuration on the
 * particles' terms: per context, kept across fx_update_frame, not checkpointed, not part of fx_field_digest.
 * FX_E_INVALID, the previous state staying in force: a NULL ctx, a wrong struct_size, unknown flag bits, enabled > 1, every > 0 with
 * enabled = 0, a NULL out-pointer, a grid of 2^32 - 1 cells or more, and (all but fx_get_particle_sort and fx_particle_sort_info, which
 * report the default there) slab ranks.  FX_E_STATE: FX_FLAG_RENDER_ONLY contexts; fx_sort_particles and fx_particle_order_device while
 * sorting is not enabled.  FX_E_NOMEM: the scratch cannot be allocated.
 * (struct fx_particle_sort_info has no typedef: C keeps a typedef and the function of that name in one name space.)
 * Out of scope: other orders (Morton, tiles) (births on the device: fx_set_particle_spawners below); sorting by anything but cell; slab contexts. */
typedef struct fx_particle_sort {
	uint32_t struct_size, flags;   /* sizeof(fx_particle_sort) = 16; flags: 0 */
	uint32_t enabled;              /* 0 (default): no scratch, no sort anywhere; 1: scratch allocated for the current and every later set */
	uint32_t every;                /* with enabled: 0 = only fx_sort_particles sorts; n > 0 = the particle stage sorts on every nth run */
} fx_particle_sort;
struct fx_particle_sort_info { uint32_t struct_size, live, sorts, reserved; };   /* 16 bytes */
int fx_set_particle_sort(fx_ctx* ctx, const fx_particle_sort* sort);
int fx_get_particle_sort(fx_ctx* ctx, fx_particle_sort* out);
int fx_sort_particles(fx_ctx* ctx, void* stream);
int fx_particle_sort_info(fx_ctx* ctx, void* stream, struct fx_particle_sort_info* out);
int fx_particle_order_device(fx_ctx* ctx, void** order_u32, void** live_u32);

/* The particle trail (no reference counterpart): the particles as a source of smoke and heat.  While a trail is set, every live record spreads
 * one unit of "amount" tri-linearly over the eight cells around it, and COLOR (and TEMPERATURE while fx_set_buoyancy is on) grow by that amount
 * times the rates below: an ember leaves a smoke trail and warms the air it flies through.  A scatter from points into the grid, made
 * reproducible the way the voxeliser is (fx_voxelize.hip): the scattered operation is an integer add, commutative and exact, so any order
 * gives the same bits; the integers become floats once per cell.  Two launches (fx_particle_trail.hip): k_trail_splat over the records,
 * k_trail_apply over the grid.  Off by default: a context that never calls the setter launches, computes and counts what it did before.
 * The rule, fp32, every operation rounded as written (tests/particle_trail_ref.py restates it in numpy); N = (X, Y, Z),
 * c(v) = fminf(fmaxf(v, 0), 1), dt = the time step of the last fx_update_frame:
 *   scatter  a record deposits iff age >= 0 (the move's test: -0.0 is live, a NaN is dead).  Per axis a of a live record:
 *            s = c(p_a), t = s * N_a - 0.5, fl = floor(t), f = t - fl;  q = (int)rintf(f * 256), in 0 ... 256;
 *            the taps are (int)fl and (int)fl + 1, both clamped to [0, N_a - 1] -- the two cells the sampler U(p) reads -- with the integer
 *            weights 256 - q and q.  A 2-D grid does not look at z: one tap, plane 0, weight 256.
 *            The cell of each of the eight tap combinations grows by w_x * w_y * w_z in a uint64 accumulator (adds of 0 may be skipped; two
 *            taps that clamp onto the same wall cell both add to it).  So every live record adds exactly 2^24 in total, wherever it is and
 *            whatever its coordinates hold: a NaN or an infinity lands where the clamp says, no value reaches an index unclamped
 *   apply    for a cell with acc != 0: if the obstacle code says the cell itself is solid (bit 6, the bit the move tests) nothing is added;
 *            otherwise A = (float)acc * 0x1p-24f (one round-to-nearest-even conversion of the 64-bit integer, then an exact scaling),
 *            g = rate * dt, colour_ch = fma(A, tint_ch * g, colour_ch) on the current colour field for each of the four channels, and, while
 *            buoyancy is on and heat != 0, T = fma(A, heat * dt, T) on the current temperature, in place.  fp16 storage widens on load and
 *            rounds once on store.  Either way the accumulator word goes back to 0: the volume is all zero between calls.  A cell with
 *            acc == 0 is not stored: its bits, a -0 included, stay
 * fx_set_particle_trail with a struct allocates the accumulator, one uint64 per cell (X * Y * Z * 8 bytes), zeroed; FX_E_NOMEM if that fails,
 * the previous state staying in force.  NULL = off (the default), which frees it.  All allocation and waiting happens here:
 * fx_deposit_particles and the step only enqueue (a captured fx_simulate stays capturable).
 * fx_simulate runs the stage between the buoyancy pass and the obstacles' enforce pass when a trail is set, a set of particles exists and the
 * time step is > 0, on the positions as they are then (moved at the end of the previous step, or set by the caller): colour and temperature
 * are final for the step there, and heat left now lifts from the next step on.  Timing: booked into fx_timing.advect_ms, like its
 * neighbours.  fx_deposit_particles is that stage alone; FX_OK and nothing done with no set or dt <= 0.
 * fx_particle_density is the inspection call (as fx_download_pressure_level is for the multigrid): it runs the scatter alone on the set in
 * force, copies the accumulator to out = uint64[Z][Y][X], clears it and blocks.  With no set: zeros.  It is also the particle density for a
 * caller's own use: out / 2^24 = particles per cell, tri-linearly spread.
 * fx_get_particle_trail: the setting in force; off reports rate 0, tint 0, heat 0.
 * Configuration on the emitters' terms: per context, kept across fx_update_frame, not checkpointed, not part of fx_field_digest.
 * FX_E_INVALID, the previous state staying in force: a NULL ctx or out-pointer, a wrong struct_size, unknown flag bits, a non-finite member,
 * rate < 0, bytes != X * Y * Z * 8, and (all but fx_get_particle_trail, which reports the default there) slab ranks.  FX_E_STATE:
 * FX_FLAG_RENDER_ONLY contexts; fx_deposit_particles and fx_particle_density while no trail is set.  FX_E_NOMEM: the accumulator cannot be
 * allocated.
 * Out of scope: per-particle strength or fading by age (the record has no room for it); momentum deposit; slab contexts (births: fx_set_particle_spawners,
 * drawing: fx_set_particle_draw, both below);
 * restricting the apply pass to the set's bounding box; checkpointing. */
typedef struct fx_particle_trail {
	uint32_t struct_size, flags;   /* sizeof(fx_particle_trail) = 32; flags: 0 */
	float rate;                    /* amount per second and particle; finite, >= 0 */
	float tint[4];                 /* rgba added per unit amount; finite */
	float heat;                    /* temperature added per unit amount and second; finite, either sign */
} fx_particle_trail;
int fx_set_particle_trail(fx_ctx* ctx, const fx_particle_trail* trail);
int fx_get_particle_trail(fx_ctx* ctx, fx_particle_trail* out);
int fx_deposit_particles(fx_ctx* ctx, void* stream);
int fx_particle_density(fx_ctx* ctx, void* stream, uint64_t* out, size_t bytes);

/* Particle spawners (no reference counterpart): tracer particles born on the device.  The set above ages and dies -- by lifetime, through open
 * walls, and, once sorted, into the tail [live, count) --; while spawners are set, up to FX_MAX_PARTICLE_SPAWNERS boxes and ellipsoids bear
 * new records at a rate, each birth taking a dead record's slot: spawn -> move -> deposit -> die -> slot reused, with no upload and no kernel
 * of the caller's.  The count per step lives in device memory, so a replayed graph keeps spawning at the right rate.  Four launches
 * (fx_particle_spawn.hip): a count of the dead per workgroup, its scan, the tick of the rates, the placement; no atomic decides a slot, the
 * result is the same bit for bit on every run.  Off by default: a context that never calls the setter launches what it did before.
 * The rule (tests/particle_spawn_ref.py restates it in numpy).  All integer arithmetic is unsigned and wraps; all floating point is fp32,
 * every operation rounded as written; c(v) = fminf(fmaxf(v, 0), 1); dt = the time step of the last fx_update_frame, taken at enqueue.
 *   state    in device memory, per spawner s: acc_s, a uint64 fraction in units of 2^-16 births, and serial_s, a uint64 count of the births
 *            the spawner has attempted; and the three uint64 counters born, dropped, blocked
 *   count    w = fminf(rate_s * dt, 67108864.0f);  inc = (uint64)llrintf(w * 65536.0f);  acc_s += inc;  n_s = acc_s >> 16;  acc_s &= 0xFFFF.
 *            The step's births are numbered j = 0 ... n - 1, n = sum of n_s: spawner 0's first, in serial order, then spawner 1's, and so
 *            on; first_s = the number of spawner s's first birth.  Birth j of spawner s has the serial k = serial_s + (j - first_s); behind
 *            the step serial_s += n_s, whether or not a birth found a slot: a record is a function of (seed, s, k) and nothing else
 *   slots    a record is dead iff !(age >= 0), the move's own test (-0.0 is live, a NaN is dead); D = the number of dead records.  Birth j
 *            takes the j-th dead record of the buffer in index order.  Births j >= D are dropped and `dropped` grows by n - D: the last
 *            spawners starve first.  A live record never changes by a bit.  Behind a sort the dead are the tail, so births append;
 *            *live_u32 and order stay those of the last sort, as they do when records die between sorts
 *   words    mix(x):  x ^= x >> 16;  x *= 0x7feb352d;  x ^= x >> 15;  x *= 0x846ca68b;  x ^= x >> 16
 *            h0 = mix(seed + 0x9e3779b9 * (s + 1));  h1 = mix(h0 ^ (uint32)k);  h2 = mix(h1 ^ (uint32)(k >> 32))
 *            word(d) = mix(h2 + 0x85ebca6b * (d + 1));  u(d) = (float)(word(d) >> 8) * 0x1p-24f, exact, in [0, 1);
 *            a(d) = fmaf(2, u(d), -1), exact, in [-1, 1)
 *   place    FX_SPAWN_BOX: (ax, ay, az) = (a(0), a(1), a(2)).  FX_SPAWN_BALL: tries t = 0 ... 7 with (a(3t), a(3t + 1), a(3t + 2)), taking
 *            the first with fmaf(az, az, fmaf(ay, ay, ax * ax)) <= 1, and (0, 0, 0) if none passes (0.476^8, about one birth in 400).  On a
 *            2-D grid az is 0 for either shape, before the test.  p_a = c(fmaf(a_a, half_extent_a, center_a)) + 0.0f
 *   age      u(24) * age_spread, which is >= 0: the record is live
 *   solids   with a mask set (fx_set_obstacles): the cell min((int)(p_a * N_a), N_a - 1) per axis, z cell 0 on a 2-D grid; if it is solid
 *            (code bit 6, the bit the move tests) the birth is blocked: its slot is not stored and stays dead with every bit kept, and
 *            `blocked` grows by one.  `born` counts the records stored
 * fx_set_particle_spawners replaces the list and zeroes the state and the three counters; count 0 or NULL = off (the default), which frees
 * the device block.  The block (one word per 1024 records, the state) is allocated here for the set in force and resized by every later
 * fx_set_particles, which keeps fractions, serials and counters (FX_E_NOMEM there leaves the previous set and block in force).  All
 * allocation and waiting happens in these two calls: fx_spawn_particles and the step only enqueue (a captured fx_simulate stays capturable).
 * fx_simulate runs the stage inside the particle stage, behind the move (sort if due, move, spawn), when the time step is > 0, a set exists
 * and spawners are set: a record born in a step sits on its spawn point with its spawn age when the step ends, is drawn there, deposits
 * there in the next step's trail and moves from the next step on.  fx_move_particles does the same.  Timing: booked into
 * fx_timing.project_ms, like the move.  fx_spawn_particles is the stage alone: FX_OK and nothing done -- the state does not tick -- while no
 * set exists or dt <= 0.
 * fx_get_particle_spawners: the list in force, as fx_get_emitters reports its own.
 * fx_particle_spawn_info waits for `stream`: the three counters and the serials since the last fx_set_particle_spawners (all 0 while off).
 * A set that is only ever spawned into starts as `count` records (0, 0, 0, -1).
 * Configuration on the particles' terms: per context, kept across fx_update_frame, not checkpointed, not part of fx_field_digest.
 * FX_E_INVALID, the previous state staying in force: a NULL ctx or out-pointer, a wrong struct_size, unknown flag bits, an unknown shape,
 * count > FX_MAX_PARTICLE_SPAWNERS, a count with a NULL list, a non-finite member, a negative rate, half_extent or age_spread, and (all but
 * fx_get_particle_spawners and fx_particle_spawn_info, which report the empty default there) slab ranks.  FX_E_STATE: FX_FLAG_RENDER_ONLY
 * contexts; fx_spawn_particles while no spawners are set.  FX_E_NOMEM: the block cannot be allocated.
 * (struct fx_particle_spawn_info has no typedef, as fx_particle_sort_info has none.)
 * Out of scope: initial velocities (the record has no room for them); per-spawner lifetimes; Gaussian shapes; slab contexts (drawing:
 * fx_set_particle_draw below). */
#define FX_MAX_PARTICLE_SPAWNERS 16u
#define FX_SPAWN_BOX  0u
#define FX_SPAWN_BALL 1u     /* an ellipsoid with the half extents as semi-axes */
typedef struct fx_particle_spawner {
	uint32_t struct_size, flags;      /* sizeof(fx_particle_spawner) = 48; flags: 0 */
	uint32_t shape, seed;             /* FX_SPAWN_*; any seed */
	float center[3], half_extent[3];  /* texture space, as fx_emitter.center; finite, half_extent >= 0 */
	float rate;                       /* births per second; finite, >= 0 */
	float age_spread;                 /* finite, >= 0: a new record's age is u * age_spread, so that a burst does not die in one frame */
} fx_particle_spawner;
struct fx_particle_spawn_info { uint32_t struct_size, reserved; uint64_t born, dropped, blocked; uint64_t serial[FX_MAX_PARTICLE_SPAWNERS]; };   /* 160 bytes */
int fx_set_particle_spawners(fx_ctx* ctx, const fx_particle_spawner* list, uint32_t count);
int fx_get_particle_spawners(fx_ctx* ctx, fx_particle_spawner* out, uint32_t capacity, uint32_t* count);
int fx_spawn_particles(fx_ctx* ctx, void* stream);
int fx_particle_spawn_info(fx_ctx* ctx, void* stream, struct fx_particle_spawn_info* out);

/* The particle draw (no reference counterpart): the tracer particles as emissive points on the render target, each dimmed by the smoke between
 * the eye and it.  A scene depth buffer hides an ember behind a wall; it does not dim one behind the plume -- that dimming is the alpha the view
 * march accumulates in front of the particle, and the march, the colour field and the camera live here.  While a draw is set,
 * fx_draw_particles splats every live record onto the render target, on top of what fx_render and fx_render_cube put there, attenuated by
 * exactly the opacity the direct view march shows in front of a scene point at the particle's place.  The trail's recipe: an integer scatter,
 * exact and independent of order, then one pass that turns integers into floats -- the same bits on every run.  Two launches
 * (fx_particle_draw.hip): k_draw_splat over the records, k_draw_resolve over the pixels.  Off by default: a context that never calls the setter
 * launches, computes and counts what it did before.
 * The rule, fp32, every operation rounded as written, fma only where it says so (tests/particle_draw_ref.py restates it in numpy); (W, H) = the
 * viewport, M = the forward WorldViewProj rows of the last fx_update_frame that carried matrices, ns = max_ray of fx_set_max_samples (the
 * merged direct march's sample count), c(v) = fminf(fmaxf(v, 0), 1).  A record (p, age) is drawn iff age >= 0 (the move's test: -0.0 is live,
 * a NaN is dead).
 *   project    q_a = fma(c(p_a), 2, -1);  h_r = fma(1, M[4r+3], fma(q_z, M[4r+2], fma(q_y, M[4r+1], q_x * M[4r+0])));  culled unless h_3 > 0;
 *              cx = h_0 / h_3, cy = h_1 / h_3, cz = h_2 / h_3;  culled unless 0 <= cz && cz < 1;  u = fma(cx, .5, .5), v = -fma(cy, .5, .5) + 1;
 *              X = u * W, Y = v * H;  culled unless 0 <= X && X < W && 0 <= Y && Y < H -- every test is written so that a NaN culls;
 *              the host pixel (px, py) = ((int)X, (int)Y)
 *   depth      with a scene depth attached (fx_set_scene_depth): culled unless cz <= depth[py][px]
 *   occlusion  the alpha sa of the direct view march of the host pixel, ended at the particle: the pixel's ray as fx_render casts it (sa = 0
 *              where that discards), tMax = the ray parameter of the clip-space point (pixel centre, cz) as the depth-aware march forms it, and
 *              the march's loop over ns samples with what alpha does not depend on left out: no light map, no light rays, no colour channels.
 *              T = c(-sa + 1).  By construction sa is what the merged direct march returns as alpha with a depth buffer holding cz at that pixel
 *   amounts    qb = (uint32)(T * 32768.0f + 0.5f);  s = lifetime > 0 ? c(age / lifetime) : 0 (fx_particle_params.lifetime);
 *              qs = (uint32)(s * 256.0f + 0.5f);  young = qb * (256 - qs), old = qb * qs
 *   footprint  bilinear over the four pixels whose centres surround (X, Y).  Per axis: t = X - 0.5, fl = floorf(t), w1 = (int)rintf((t - fl) * 128),
 *              w0 = 128 - w1 on the pixels (int)fl and (int)fl + 1.  A footprint pixel outside the viewport is dropped, not clamped: light that
 *              leaves the screen is lost.  acc[iy][ix][0] += young * wx * wy, acc[iy][ix][1] += old * wx * wy in uint64 (adds of 0 may be
 *              skipped): qb << 22 in total for a footprint on screen, at most 2^37 a word, so FX_MAX_PARTICLES records cannot overflow one
 *   resolve    per pixel:  Yv = (float)acc0 * 0x1p-37f, Ov = (float)acc1 * 0x1p-37f (one round-to-nearest-even conversion, then an exact scaling);
 *              k0_c = color[c] * color[3], k1_c = end_color[c] * end_color[3];  src_c = fma(Ov, k1_c, Yv * k0_c) for c = r, g, b.  Where
 *              acc0 | acc1 is non-zero the target takes the premultiplied blend of (src, alpha 0) -- additive, the target's alpha stays --,
 *              FX_FIELD_TARGET_FLOAT = (src, 0) and both words go back to 0; elsewhere the target is not stored and FX_FIELD_TARGET_FLOAT = 0
 * No value reaches an index unclamped or untested: whatever the caller wrote into the record buffer is safe to draw.
 * fx_set_particle_draw with a struct allocates the accumulator, two uint64 per pixel (W * H * 16 bytes), zeroed, and the render target where
 * no render has allocated it yet; FX_E_NOMEM if that fails, the previous state staying in force.  NULL = off (the default), which frees the
 * accumulator.  All allocation and waiting happens here: fx_draw_particles only enqueues its two launches and stays capturable.
 * fx_draw_particles draws the set in force with the camera of the last fx_update_frame that carried matrices, through the colour field
 * fx_render marches (every sample gathers: FX_OPT_RENDER_ACCEL does not change a bit of it).  With no set of particles: FX_OK, the target
 * untouched, FX_FIELD_TARGET_FLOAT all zero.  Timing: booked into fx_timing.resolve_ms; it does not count as a render.
 * fx_particle_splats is the inspection call, the counterpart of fx_particle_density: it runs the splat alone on the set in force, copies the
 * accumulator to out = uint64[H][W][2], clears it and blocks.  With no set: zeros.
 * fx_get_particle_draw: the setting in force; off reports both colours 0.
 * Configuration on the emitters' terms: per context, kept across fx_update_frame, not checkpointed, not part of fx_field_digest.
 * FX_E_INVALID, the previous state staying in force: a NULL ctx or out-pointer, a wrong struct_size, unknown flag bits, a non-finite or
 * negative member, bytes != W * H * 16, a frame_index >= FX_FRAME_COUNT, and (all but fx_get_particle_draw, which reports the default there) a
 * 2-D grid, a context without a viewport, a slab rank.  FX_E_STATE: FX_FLAG_RENDER_ONLY contexts, which have no particles; fx_draw_particles
 * and fx_particle_splats while no draw is set or before an fx_update_frame gave a camera (as fx_render).  FX_E_NOMEM: the accumulator or the
 * target cannot be allocated.
 * Out of scope: sprites larger than the bilinear footprint; per-particle colour or strength (the record has no room for them); absorbing
 * particles; lighting the particles from the light map; motion blur; drawing into the cube map; slab and render-only contexts; checkpointing. */
typedef struct fx_particle_draw {
	uint32_t struct_size, flags;   /* sizeof(fx_particle_draw) = 40; flags: 0 */
	float color[4];                /* rgb x intensity (w) of a particle of age 0; finite, >= 0 */
	float end_color[4];            /* ... of a particle of age >= lifetime (fx_particle_params); finite, >= 0 */
} fx_particle_draw;
int fx_set_particle_draw(fx_ctx* ctx, const fx_particle_draw* draw);
int fx_get_particle_draw(fx_ctx* ctx, fx_particle_draw* out);
int fx_draw_particles(fx_ctx* ctx, void* stream, uint8_t frame_index);
int fx_particle_splats(fx_ctx* ctx, void* stream, uint64_t* out, size_t bytes);

/* The obstacle draw (no reference counterpart): the solid cells of the mask in force -- whichever of fx_set_obstacles and fx_set_obstacle_meshes
 * put it there, resting or moving (fx_set_obstacle_bodies) -- ray-cast into the render target and into a depth buffer.  Per pixel the view ray walks the
 * voxel mask to the first solid cell; the face it entered through is shaded with the light of fx_set_light and written, opaque, with its D3D
 * depth.  With that depth attached (fx_set_scene_depth, FX_DEPTH_DEVICE) the marches end at the solid: smoke in front of it blends over it,
 * smoke behind it is hidden, fx_draw_particles culls what lies behind it.  No march kernel knows of it.  The frame order becomes: clear,
 * environment, fx_draw_obstacles, fx_render (with the obstacle depth attached), fx_draw_particles.  Off by default: a context that never
 * calls the setter launches, computes and counts what it did before.
 * The rule, fp32, every operation rounded as written, fma only where it says so (tests/obstacle_draw_ref.py restates it in numpy).
 * N = (X, Y, Z) the grid, S(i) = bit 6 of the code byte of cell i = (i_0, i_1, i_2) = (x, y, z), (W, H) = the viewport.
 *   ray      (o, d) = what fx_render's direct march casts for the pixel: the pixel's ray and its origin moved onto the volume's box
 *            (PSRayCast.hlsl:17-26,47-50, ComputeRayOrigin); a pixel that discards is a miss.  e = the entry axis of ComputeRayOrigin, the axis
 *            whose quotient became U (the lowest on a tie); none when the eye lies inside the box
 *   start    s_a = fma(o_a, .5, .5);  i_a = min(max((int)floorf(s_a * N_a), 0), N_a - 1);  st_a = +1 / -1 / 0 for d_a > 0 / d_a < 0 / otherwise
 *            (a -0 or a NaN gives 0);  r_a = 1.0f / d_a.  If S(i): a hit at t = 0, p = o, face = 2e + (d_e > 0) with an entry axis, 6 without
 *   walk     per axis n_a = i_a + (st_a > 0);  P_a = fma((float)n_a / (float)N_a, 2, -1);  t_a = st_a ? (P_a - o_a) * r_a : FLT_MAX.
 *            The step axis a* = (t_0 <= t_1 && t_0 <= t_2) ? 0 : (t_1 <= t_2) ? 1 : 2 (the smallest t, ties to the lowest axis, a NaN loses).
 *            st_a* == 0: a miss (the walk cannot move).  i_a* += st_a*;  off the grid on that axis: a miss;  S(i): a hit with t_hit = t_a*
 *            (taken before the advance), face = 2 a* + (st_a* > 0), normal = -st_a* e_a*, p_a = fma(d_a, t_hit, o_a).  After X + Y + Z advances
 *            without a hit: a miss.  Every t is a function of an integer plane index and nothing accumulates, so a walk that skips what it knows
 *            to be empty reproduces this one bit for bit, and the cap ends it whatever the matrices held
 *   visible  h_r = fma(1, M[4r+3], fma(p_2, M[4r+2], fma(p_1, M[4r+1], p_0 * M[4r+0]))), M = the forward WorldViewProj rows (the chain of the
 *            particle draw's project, on p itself);  cz = h_2 / h_3.  Drawn iff h_3 > 0 && 0 <= cz && cz < 1 && (no scene depth ||
 *            cz <= scene[py][px]), written so that a NaN is not drawn: a hit in front of the near plane is clipped away, as a rasteriser would
 *   shade    L = the unit vector the shadow rays run along: the local light direction (FX_LIGHT_DIRECTIONAL) or the direction from p to the
 *            local light point, 0 where the marches cast no ray (FX_LIGHT_POINT).  With st = +1 for an odd face, -1 for an even one and
 *            a = face / 2:  ndl = face < 6 ? fmaxf(0, (float)(-st) * L_a) : 0;  k_c = albedo[c] * albedo[3];
 *            src_c = (k_c * fma(ndl, color[3] * color[c], ambient[3] * ambient[c])) * 0.159154937f for c = r, g, b (the light's colour and
 *            ambient of fx_set_light; the ambient term also while a light probe is set)
 *   store    a drawn pixel: target = (unorm8(src_r), unorm8(src_g), unorm8(src_b), 255) -- an opaque overwrite, no blend --,
 *            FX_FIELD_TARGET_FLOAT = (src, 1), depth-out = cz.  Every other pixel: the target keeps its bytes, FX_FIELD_TARGET_FLOAT = 0,
 *            depth-out = the scene depth, or 1.0 without one.  The hits word (fx_obstacle_hits) of a pixel whose walk hit, drawn or not:
 *            bit 63 set, bit 62 = drawn, bits 32-34 = face, bits 0-31 = (z * Y + y) * X + x of the cell; a miss is 0
 * No value reaches an index unclamped or untested, and the only loop is bounded by the cap.
 * fx_set_obstacle_draw with a struct does all the allocation: the depth-out buffer (W * H floats, filled with 1.0), the brick volume the cast
 * walks through (one uint64 per 4 x 4 x 4 cells: bit (z & 3) * 16 + (y & 3) * 4 + (x & 3) = S, cells beyond the grid 0) and the render
 * target where no render has allocated it yet; FX_E_NOMEM if that fails, the previous state staying in force.  NULL = off (the default), which
 * frees the first two.  fx_get_obstacle_draw: the setting in force; off reports albedo 0.
 * fx_draw_obstacles only enqueues -- it never allocates, copies to the host or waits, and stays capturable: the cast (fx_obstacle_draw.hip
 * k_obstacle_cast), and in front of it the pack of the brick volume (k_obstacle_pack) when the mask has changed since the last pack, so that a
 * mask set between two draws is seen by the second.  It uses the camera of the last fx_update_frame that carried matrices and the light of
 * fx_set_light.  scene_depth_device is optional: the caller's own scene, float[H][W] on the context's device, D3D convention; a hit behind it
 * is not drawn.  It must not be the depth-out buffer.  With no mask in force, or one without a solid cell: FX_OK, the target untouched,
 * depth-out = the scene depth (1.0 without one), FX_FIELD_TARGET_FLOAT all zero.  Timing: booked into fx_timing.resolve_ms; not a render.
 * fx_obstacle_depth_device: the depth-out buffer, float[H][W] on the device; NULL while the draw is off.  One call attaches it:
 * fx_set_scene_depth(ctx, stream, depth, W, H, z_near, z_far, FX_DEPTH_DEVICE).  The renders read it in place and fx_draw_obstacles rewrites
 * it each frame on the same stream.  The pointer is valid until the next fx_set_obstacle_draw or fx_destroy; switching the draw off while it
 * is attached is the caller's error (detach first: fx_set_scene_depth(ctx, stream, NULL, ...)).
 * fx_obstacle_hits is the inspection call: the same cast, storing neither target nor depth-out, its hits words and depths copied to the host
 * pointers hits_out and depth_out (either may be NULL), pixels = W * H each; blocks.
 * Configuration on the particle draw's terms: per context, kept across fx_update_frame, not checkpointed, not part of fx_field_digest.
 * FX_E_INVALID, the previous state staying in force: a NULL ctx or out-pointer, a wrong struct_size, unknown flag bits, a non-finite or
 * negative albedo member, pixels != W * H, a frame_index >= FX_FRAME_COUNT, scene_depth_device = the depth-out buffer, and (all but
 * fx_get_obstacle_draw and fx_obstacle_depth_device, which report the default there) a 2-D grid, a context without a viewport, a slab rank, a
 * grid of 2^32 cells or more.  FX_E_STATE: FX_FLAG_RENDER_ONLY contexts, which have no obstacles; fx_draw_obstacles and fx_obstacle_hits while
 * the draw is off or before an fx_update_frame gave a camera (as fx_render).  FX_E_NOMEM: a buffer cannot be allocated.
 * Out of scope: solids casting shadows into the smoke (the light marches do not see the mask -- the obvious next step); smoke shadowing the
 * solids (a light-map fetch at the hit); SH irradiance on solids; per-body or per-mesh colours (the code byte carries no body); smooth normals;
 * drawing into the cube map; slab, render-only and 2-D contexts; checkpointing. */
typedef struct fx_obstacle_draw {
	uint32_t struct_size, flags;   /* sizeof(fx_obstacle_draw) = 24; flags: 0 */
	float albedo[4];               /* rgb x intensity (w); finite, >= 0 */
} fx_obstacle_draw;
int fx_set_obstacle_draw(fx_ctx* ctx, const fx_obstacle_draw* draw);
int fx_get_obstacle_draw(fx_ctx* ctx, fx_obstacle_draw* out);
int fx_draw_obstacles(fx_ctx* ctx, void* stream, uint8_t frame_index, const float* scene_depth_device);
int fx_obstacle_depth_device(fx_ctx* ctx, void** depth);
int fx_obstacle_hits(fx_ctx* ctx, void* stream, uint8_t frame_index, const float* scene_depth_device,
	uint64_t* hits_out, float* depth_out, size_t pixels);

/* The advection scheme (no reference counterpart: the reference's CSAdvect is a first-order semi-Lagrangian step, the main source of the blur
 * the confinement fights).  FX_ADVECT_MACCORMACK is the scheme of Selle, Fedkiw, Kim, Liu, Rossignac 2008 (also Crane et al., GPU Gems 3
 * ch. 30): second order, unconditionally stable with its limiter, two more gathers per cell.  While it is set, the advection of fx_simulate
 * and the stage call fx_advect run two launches, a predictor and a corrector, in place of the semi-Lagrangian one; the step around them is
 * unchanged (advect -> inflow -> emit -> heat -> enforce -> confine -> divergence ...).  Per cell (x, y, z), fp32, every operation rounded as
 * written (tests/maccormack_ref.py restates it in numpy); q ranges over the seven advected quantities VELOCITY x, y, z and COLOR r, g, b, a;
 * u0 = VELOCITY at the cell, dt = the time step of the last fx_update_frame; fp16 storage widens on load:
 *   1  the back-trace, tap for tap as the semi-Lagrangian step does it:  p = ((x + .5) / X, (y + .5) / Y, (z + .5) / Z)      a = fma(-u0, dt, p)
 *      t = a * N - 0.5, i0 = floor(t), f = t - i0 per axis; the eight taps i0, i0 + 1 go through the context's address mode (clamp / mirror);
 *      hat_q = lerp_z(lerp_y(lerp_x ...)) with lerp(a, b, f) = fma(f, b - a, a).  The bounds go over the eight taps v in the order 000, 100,
 *      010, 110, 001, 101, 011, 111 (x fastest), starting at the first tap:   lo = v < lo ? v : lo      hi = v > hi ? v : hi
 *      -- selects, not fmin / fmax: of +0 and -0 the earlier tap stays, a NaN tap never replaces a bound
 *   2  the predictor stores hat_q (fp32) for all seven quantities into a scratch
 *   3  the forward trace from the same cell with the same u0:  b = fma(u0, dt, p), taps and fractions as in 1 through the same address mode;
 *      bar_q = the same trilinear sample, taken from the scratch
 *   4  r_q = fma(0.5, q - bar_q, hat_q), q the cell's own stored value;   then the limiter  r_q = r_q < lo ? lo : (r_q > hi ? hi : r_q)
 *   5  the tail of the semi-Lagrangian step, unchanged, on r: the built-in impulse unless fx_set_impulse switched it off, the attenuation
 *      max(fma(-dt, 0.2, 1), 0), the stores into VELOCITY1 and COLOR, each rounded once, and the render's alpha side volume on the
 *      semi-Lagrangian step's own condition
 * No special cases: dt <= 0 and 2-D grids go through the same rules (a 2-D grid: both z taps are plane 0, the z lerp runs on equal operands).
 * The temperature of fx_set_buoyancy stays semi-Lagrangian under either scheme.
 * fx_set_advection_scheme: FX_ADVECT_SEMI_LAGRANGIAN is the default: every call behaves exactly as without this function.  The first
 * successful switch to FX_ADVECT_MACCORMACK allocates the scratch, seven fp32 values per cell (three planes of X * Y * Z and one float4
 * volume) whatever fx_desc.storage is -- FX_E_NOMEM if that fails, the scheme staying as it was; the switch back frees it.  The scratch
 * carries nothing from step to step.  Configuration like the emitters: per context, kept across fx_update_frame, not checkpointed (a resumed
 * run only has to set the scheme again behind fx_checkpoint_load), not part of fx_field_digest.  FX_E_INVALID, the previous setting staying
 * in force: an unknown scheme, a NULL ctx or out-pointer, and (the setter) a context that owns fewer planes than the grid -- slab ranks of
 * every transport: the corrector would need halo planes of the predicted fields.  FX_E_STATE (both calls): FX_FLAG_RENDER_ONLY contexts.
 * Both Jacobi modes, both address modes, both storages, 2-D grids and every optional stage are served.
 * Timing: both launches are booked into fx_timing.advect_ms. */
#define FX_ADVECT_SEMI_LAGRANGIAN 0u   /* the reference's CSAdvect; the default */
#define FX_ADVECT_MACCORMACK      1u
int fx_set_advection_scheme(fx_ctx* ctx, uint32_t scheme);
int fx_get_advection_scheme(fx_ctx* ctx, uint32_t* scheme);

/* The pressure solver (no reference counterpart: the reference's CSProject relaxes with Jacobi sweeps only).  FX_PRESSURE_JACOBI, the default,
 * is fx_desc.jacobi_iters lock-step sweeps, every launch the one it is without this function.  FX_PRESSURE_MULTIGRID runs `cycles` geometric
 * V-cycles of damped Jacobi on the same operator (clamped walls, sum(q) - 6 p = b; 2-D: 4 p) from the same warm start: fx_simulate and
 * fx_pressure_solve then ignore jacobi_iters; fx_jacobi(iters) stays plain Jacobi whatever is set.
 * Levels: level 0 is the grid; level l + 1 halves X, Y and (3-D) Z of level l, and exists only while every extent to be halved is even and
 * >= 4 -- an odd extent is not coarsened: a half-covered last coarse cell has no consistent coarse operator here yet, and the V-cycle slowly
 * diverges with either naive one --, below max_levels and below 12 levels.  256^3 has 8 levels (down to 2^3), 150^3 two (75^3), 37 x 37 one;
 * with one level a solve is cycles x coarse_sweeps damped sweeps.
 * Arithmetic, fp32, every operation rounded as written, fma only where it says so (tests/multigrid_ref.py restates it in numpy); neighbours
 * L, R (x -+ 1), U, D (y -+ 1), F, B (z -+ 1) by clamped index:
 *   sweep      J = ((((((L - b) + R) + U) + D) + F) + B) * (1/6 as 0x3e2aaaab)    2-D: ((((L - b) + R) + U) + D) * 0.25
 *              p' = fma(omega, J - p, p)            lock step, out of place: the pressure ping-pong flips as in the Jacobi solve
 *   residual   S = (((((L + R) + U) + D) + F) + B)      r = fma(6, p, b - S)      2-D: four neighbours and 4
 *   restrict   b_c = 0.5 * (((r000 + r100) + (r010 + r110)) + ((r001 + r101) + (r011 + r111)))  (index order x, y, z)
 *              2-D: b_c = (r00 + r10) + (r01 + r11).  The coarse operator is the same unscaled stencil (hence 4 x the mean); the coarse
 *              correction starts at +0
 *   prolong    per axis, fine index i: parent j = i >> 1, other o = clamp(j + (i odd ? 1 : -1), 0, n_c - 1), v = fma(0.25, e[o] - e[j], e[j]);
 *              x, then y, then z (3-D); p += v, in place on the current buffer
 *   cycle(l)   last level: coarse_sweeps sweeps.  Otherwise pre_sweeps sweeps; restrict the residual into level l + 1; cycle(l + 1) from +0;
 *              prolong and correct; post_sweeps sweeps
 * From the first level >= 1 with at most 4096 cells down, the rest of the cycle runs as one launch of one workgroup in the LDS (the "tail":
 * those levels are bound by launch latency); FX_MG_NO_TAIL runs them as launches of their own instead -- the same bits, a diagnostic.
 * fx_set_pressure_solver: NULL or kind FX_PRESSURE_JACOBI returns to the default and frees the pyramid (per coarse level two correction buffers
 * and a right-hand side, about 1.7 bytes per fine cell in all), which the first switch to multigrid allocates: FX_E_NOMEM if that fails, the
 * state as it was.  Configuration like the emitters: per context, kept across fx_update_frame, not checkpointed (the pressure itself is: a
 * resumed run that sets the solver again continues bit for bit), not part of fx_field_digest.
 * FX_E_INVALID: a NULL ctx or out-pointer, an unknown kind or flag, cycles outside 1..64, pre_sweeps / post_sweeps above 64, coarse_sweeps
 * outside 1..256, max_levels above 12, omega not finite or outside (0, 1], slab ranks, FX_JACOBI_FAITHFUL contexts.  FX_E_STATE:
 * FX_FLAG_RENDER_ONLY contexts; multigrid requested while obstacles or an open wall are set, and fx_set_obstacles (non-NULL) /
 * fx_set_open_walls (non-zero) while multigrid is set -- their boundary rules have no coarse counterpart yet.
 * fx_get_pressure_solver: the setting in force; max_levels = the levels in use (1 under FX_PRESSURE_JACOBI; the other fields are then 0).
 * fx_pressure_solve: the stage fx_simulate runs between fx_divergence and fx_project, under either kind.
 * fx_download_pressure_level: what = 0 the solution (level 0: FX_FIELD_PRESSURE) or the correction the last solve left on a level >= 1,
 * what = 1 the right-hand side (level 0: FX_FIELD_DIVERGENCE); float[Z_l][Y_l][X_l], bytes exact; FX_E_INVALID for a level not in use.
 * Timing: booked under the Jacobi mark; `launches` counts every launch of a solve, `sweeps` the level-0 smoothing sweeps. */
#define FX_PRESSURE_JACOBI    0u   /* default: fx_desc.jacobi_iters sweeps, every launch the one it is without fx_set_pressure_solver */
#define FX_PRESSURE_MULTIGRID 1u
#define FX_MG_NO_TAIL         0x1u /* diagnostic: every level runs as launches of its own */
#define FX_MG_MAX_LEVELS      12u
typedef struct fx_pressure_solver {      /* 32 bytes */
	uint32_t kind, flags;
	uint32_t cycles;         /* V-cycles per solve, 1..64 */
	uint32_t pre_sweeps;     /* 0..64 */
	uint32_t post_sweeps;    /* 0..64 */
	uint32_t coarse_sweeps;  /* sweeps on the coarsest level, 1..256 */
	uint32_t max_levels;     /* set: cap, 0 = as many as the grid allows; get: the levels in use */
	float    omega;          /* damping, finite, 0 < omega <= 1 */
} fx_pressure_solver;
int fx_set_pressure_solver(fx_ctx* ctx, const fx_pressure_solver* solver);
int fx_get_pressure_solver(fx_ctx* ctx, fx_pressure_solver* out);
int fx_pressure_solve(fx_ctx* ctx, void* stream);
int fx_download_pressure_level(fx_ctx* ctx, uint32_t level, int what, void* host, size_t bytes);

/* LightProbe::TransformSH + GetSH (LightProbe.h:22,26; LightProbeEZ.cpp:117-123,183-278):
 * order-3 SH of a radiance cube float[6][N][N][3] (host), coefficients to out27 (host) */
int fx_sh_transform(fx_ctx* ctx, const float* cube, uint32_t n, float* out27);

/* LightProbe::Init's asset path (LightProbe.cpp:41-46 hands a DDS file to XUSG's loader, row f-4): a DDS cube map to linear float
 * radiance.  Accepted: DX10-header files in DXGI_FORMAT_BC6H_UF16 (the reference's Bin/Assets/rnl_cross.dds; decoded on the device),
 * R32G32B32A32_FLOAT, R32G32B32_FLOAT, R16G16B16A16_FLOAT, R8G8B8A8_UNORM, and legacy headers with FourCC 113 / 116
 * (D3DFMT_A16B16G16R16F / A32B32G32R32F); every face carries its whole mip chain.  fx_dds_cube_info: edge of mip 0 and mip count
 * (FX_E_INVALID for any other container / format); fx_dds_decode_cube: mip `mip` of all six faces (order +X -X +Y -Y +Z -Z) as
 * out_cube float[6][n][n][3] (n = max(size >> mip, 1); out_floats must be 18 n^2; alpha is dropped). */
int fx_dds_cube_info(const void* dds, size_t bytes, uint32_t* size, uint32_t* mips);
int fx_dds_decode_cube(fx_ctx* ctx, const void* dds, size_t bytes, uint32_t mip, float* out_cube, size_t out_floats);

/* timing */
int fx_timing_enable(fx_ctx* ctx, int enable);
int fx_timing_read(fx_ctx* ctx, fx_timing* out, int reset);

/* ---- multi-GPU z-slabs (no reference counterpart) --------------------------------
 * One context per rank.  RCCL transport: fx_comm_id_bytes/fx_comm_get_unique_id on rank 0, broadcast
 * the bytes out of band, fx_comm_init_rank on every rank (rank r owns slab r).  In-process groups (one process, several slab
 * contexts, rank 0 drives them all): fx_comm_init_local -- one device, every member on ONE compute stream (the decomposition's
 * arithmetic on a 1-GPU box) -- and fx_comm_init_peer -- every member keeps its own streams and may live on its own device
 * (fx_desc.device): a rank pulls its halo planes straight out of its neighbour's memory (hipDeviceEnablePeerAccess +
 * hipMemcpyPeerAsync; no IPC handles, no RCCL), the members run concurrently, ordered by events per exchange.  With a peer group
 * fx_simulate ignores its stream argument: each member's work goes to the member's own stream.
 * The id is TWO ncclUniqueIds (256 bytes): the communicator of the step's exchanges and a second one for traffic that must not
 * queue with them (FX_OPT_OVERLAP 3).  Passing only the first 128 bytes gives one communicator serving both. */
size_t fx_comm_id_bytes(void);
int fx_comm_get_unique_id(void* id_out, size_t bytes);
int fx_comm_init_rank(fx_ctx* ctx, const void* id, size_t bytes, int rank, int nranks);
int fx_comm_init_local(fx_ctx** ctxs, int nranks);
int fx_comm_init_peer(fx_ctx** ctxs, int nranks);

/* Multi-GPU rendering (row f-3 of SURVEY.md 8), the exact way: rays cross slabs, so the colour field is gathered.  Every
 * rank of the slab group sends its owned planes of colour[parity] to rank `root`, where they land in `full`, a whole-grid
 * context on the root's device (same grid and storage; FX_FLAG_RENDER_ONLY keeps it small) that then runs
 * fx_update_frame(dt = 0, camera) + fx_render like any single-GPU context -- the picture is bit-identical to the
 * single-domain one.  Call on every rank; `full` is read on the root only (NULL elsewhere).  slab_z0 / slab_nz list the
 * nranks slabs (the root places the planes by them; a loop-back group knows its members and accepts NULL). */
int fx_comm_gather_color(fx_ctx* ctx, void* stream, fx_ctx* full, int root, const uint32_t* slab_z0, const uint32_t* slab_nz);

/* How the slab schedule hides the exchanges; results are bit-identical for every setting, and every rank of a
 * group must use the same values (a loop-back group reads those of its first context).
 *   FX_OPT_OVERLAP       0 = every exchange on the compute stream;
 *                        1 = the advection halo travels on a side stream behind the interior advection;
 *                        2 = (default) additionally each pressure exchange travels behind the interior sweeps
 *                            of its round (the face planes are swept first)
 *                        3 = additionally the colour half of the NEXT step's advection halo (4 of its 7 plane-units)
 *                            leaves as soon as this step's advection has written it and travels behind the pressure
 *                            phase; the next step only exchanges the velocity.  While such a halo is out, fx_upload of a
 *                            colour field into an RCCL rank returns FX_E_STATE (its neighbours could not know; a
 *                            loop-back group simply exchanges the colour again)
 *   FX_OPT_JACOBI_ROUND  sweeps per pressure exchange, 1 .. fx_desc.halo_jacobi (default = halo_jacobi)
 *   FX_OPT_ADAPTIVE_HALO 1 = (default) the advection exchange carries, per slab face, exactly the planes the coming advection
 *                        will touch: behind every projection a kernel measures them on the velocity just written (the z taps
 *                        of every voxel's back-trace, computed with the advection's own arithmetic), the ranks all-gather the
 *                        two numbers, and the next step exchanges max(need of the two slabs sharing the face) planes instead of
 *                        fx_desc.halo_advect -- which remains the allocation and the limit: a need beyond it stops the step with
 *                        FX_E_HALO on EVERY rank before a field is touched.  The measurement holds for time steps up to the one
 *                        it was taken with; a larger one, the first step, or a velocity upload fall back to halo_advect planes.
 *                        0 = always halo_advect planes.
 *   FX_OPT_COUNT_SAMPLES 1 = fx_render counts the samples its marches take (fx_timing.view_samples / light_samples / lightmap_fetches): every
 *                        thread adds its counts with atomics, so a counted render is for statistics, not for timing.  Local to the context.
 *   FX_OPT_RENDER_ACCEL  1 = (default) fx_render runs the accelerated marches: occupancy masks of the colour field held in the LDS, an
 *                        alpha-only side volume for the density taps, the lit light-map voxels compacted into a list.  0 = the plain
 *                        kernels, where every sample gathers its taps like the reference's shaders.  Bit-identical pictures either
 *                        way (the accelerated path only skips fetches whose result is known); local to the context.  Grids of more
 *                        than 2^28 voxels always take the plain kernels (the accelerated ones address by 32-bit byte offsets).  While
 *                        it is on, a context that renders its frames has the advection of the NEXT fx_simulate -- when that runs on
 *                        the stream the render ran on -- store the side volume along with the colour field (one more 4-byte store
 *                        per voxel), so that the render does not read the field a second time to extract it.
 * On an RCCL chain fx_set_option (of the three schedule options) is COLLECTIVE: every rank calls it with the same arguments between two steps; the values are
 * compared across the chain and a disagreement returns FX_E_INVALID everywhere with nothing changed.  While FX_OPT_ADAPTIVE_HALO
 * is on and a step has run, fx_upload(FX_FIELD_VELOCITY) into an RCCL rank returns FX_E_STATE (its neighbours have sized the next
 * exchange from the old field); switch the option off first. */
enum fx_option { FX_OPT_OVERLAP = 1, FX_OPT_JACOBI_ROUND = 2, FX_OPT_ADAPTIVE_HALO = 3, FX_OPT_COUNT_SAMPLES = 4, FX_OPT_RENDER_ACCEL = 5 };
int fx_set_option(fx_ctx* ctx, uint32_t option, uint32_t value);

/* Measurement switches of the kernel launchers (no reference counterpart; docs/LAB.md lists them): which kernel serves a geometry,
 * chunk sizes, tile orders -- A/B runs and the parity tests that pit one kernel of the library against another.  Process-wide,
 * none changes a result.  name: e.g. "ADVECT_LDS", "JACOBI_T" (fx_knob_name enumerates them, NULL behind the last); value: the
 * text the switch parses, NULL = back to the default.  FX_E_INVALID for an unknown name.  The library reads no environment variable
 * for them (the one it reads: FLUIDX_RCCL_LIB, the path of librccl.so). */
int fx_set_knob(const char* name, const char* value);
const char* fx_knob_name(uint32_t index);

#ifdef __cplusplus
}
#endif
#endif /* FLUIDX_HIP_H */
