// Fluid.hpp -- C++ host-side mirror of the reference's operator classes over the C ABI
// (include/fluidx_hip.h).  Same method names, argument meaning and error behaviour as
// /root/reference/FluidX12/Content/Fluid.h:20-35 and Content/LightProbe.h:16-26, so a caller written
// against the reference (FluidX12/FluidX12.cpp:197-201, 277, 465, 484-500) ports by dropping the XUSG
// arguments: CommandList* -> hipStream_t (void*), descriptor-table lib / uploaders / formats -> gone.
// Header-only; links against libfluidx_hip.so.
#pragma once
#include "../../include/fluidx_hip.h"
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

namespace fluidx {

struct XMUINT3 { uint32_t x, y, z; };
struct XMFLOAT3 { float x, y, z; };
struct XMFLOAT4X4 { float m[4][4]; };      // row-major, row-vector convention (DirectXMath)

struct FluidOptions {                       // knobs the reference fixes at compile time / in FluidX12.cpp
	uint32_t storage = FX_STORAGE_FP16;            // the reference stores RGBA16F (Fluid.cpp:207,213)
	uint32_t jacobiIters = 64;                     // ITER (CSProject3D.hlsl:13)
	uint32_t jacobiMode = FX_JACOBI_FAITHFUL;      // per-cell early-out (CSPoisson.hlsli:24)
	uint32_t advectAddress = FX_ADDRESS_CLAMP;     // FluidEZ.cpp:406 (Fluid.cpp:452 uses MIRROR)
	int32_t device = -1;
};

class Fluid {
public:
	typedef FluidOptions Options;
	enum RenderFlags : uint8_t {           // Fluid.h:12-18
		RAY_MARCH_DIRECT = 0,
		RAY_MARCH_CUBEMAP = (1 << 0),
		SEPARATE_LIGHT_PASS = (1 << 1),
		OPTIMIZED = RAY_MARCH_CUBEMAP | SEPARATE_LIGHT_PASS
	};
	static const uint8_t FrameCount = FX_FRAME_COUNT;   // Fluid.h:35

	Fluid() : m_ctx(nullptr) {}
	virtual ~Fluid() { if (m_ctx) fx_destroy(m_ctx); }
	Fluid(const Fluid&) = delete;
	Fluid& operator=(const Fluid&) = delete;

	// Fluid::Init (Fluid.cpp:189-270): false on failure, like XUSG_N_RETURN(..., false)
	bool Init(void* /*pCommandList*/, uint32_t width, uint32_t height, const XMUINT3& gridSize, const Options& opt = Options())
	{
		if (m_ctx) { fx_destroy(m_ctx); m_ctx = nullptr; }
		fx_desc d;
		std::memset(&d, 0, sizeof d);
		d.struct_size = sizeof d;
		d.grid_x = gridSize.x; d.grid_y = gridSize.y; d.grid_z = gridSize.z;
		d.viewport_w = width; d.viewport_h = height;
		d.storage = opt.storage; d.jacobi_iters = opt.jacobiIters; d.jacobi_mode = opt.jacobiMode;
		d.advect_address = opt.advectAddress; d.device = opt.device;
		m_status = fx_create(&m_ctx, &d);
		m_width = width; m_height = height;
		return m_status == FX_OK;
	}
	void SetMaxSamples(uint32_t maxRaySamples, uint32_t maxLightSamples) { m_status = fx_set_max_samples(m_ctx, maxRaySamples, maxLightSamples); }
	void SetSH(const float* coeffSH /* 9 x float3, or nullptr */) { m_status = fx_set_sh(m_ctx, coeffSH); }
	void UpdateFrame(float timeStep, uint8_t frameIndex, const XMFLOAT4X4& view, const XMFLOAT4X4& proj, const XMFLOAT3& eyePt)
	{
		const float eye[3] = { eyePt.x, eyePt.y, eyePt.z };
		m_status = fx_update_frame(m_ctx, timeStep, frameIndex, &view.m[0][0], &proj.m[0][0], eye);
	}
	void Simulate(void* pCommandList /* hipStream_t */, uint8_t frameIndex) { m_status = fx_simulate(m_ctx, pCommandList, frameIndex); }
	// Fluid::Render (Fluid.cpp:412-446).  With a render target in use (ClearRenderTarget called at least once) the
	// cube path ends in renderCube like the reference's (Fluid.cpp:430); without one only the cube map is produced.
	void Render(void* pCommandList /* hipStream_t */, uint8_t frameIndex, uint8_t flags)
	{
		m_status = fx_render(m_ctx, pCommandList, frameIndex, flags);
		if (m_status == FX_OK && m_hasTarget && (flags & RAY_MARCH_CUBEMAP)) m_status = fx_render_cube(m_ctx, pCommandList, frameIndex);
	}
	// the caller's ClearRenderTargetView on the swap-chain target (FluidX12.cpp:471-472)
	void ClearRenderTarget(void* pCommandList, const float clearColor[4])
	{
		m_status = fx_clear_render_target(m_ctx, pCommandList, clearColor);
		m_hasTarget = m_status == FX_OK;
	}
	void UseRenderTarget() { m_hasTarget = true; }
	// the scene's depth buffer for the following renders (the reference's _HAS_DEPTH_MAP_ variants; fx_set_scene_depth): float[height][width]
	// of the Init viewport, 0 = near, 1 = far plane, under UpdateFrame's projection with planes zNear / zFar.  onDevice: `depth` is device
	// memory read in place by every later Render (keep it alive); otherwise it is copied.  nullptr detaches.
	bool SetSceneDepth(const float* depth, float zNear, float zFar, bool onDevice = false)
	{
		m_status = fx_set_scene_depth(m_ctx, nullptr, depth, m_width, m_height, zNear, zFar, onDevice ? FX_DEPTH_DEVICE : 0u);
		return m_status == FX_OK;
	}       // something (the sky pass) has drawn on the target: Render resolves onto it
	// read the RGBA8 target back (the reference's screen-shot path reads the back buffer, FluidX12.cpp:640-660)
	bool ReadRenderTarget(std::vector<uint8_t>& rgba)
	{
		rgba.resize(fx_field_bytes(m_ctx, FX_FIELD_TARGET));
		if (rgba.empty()) return false;
		m_status = fx_download(m_ctx, FX_FIELD_TARGET, rgba.data(), rgba.size());
		return m_status == FX_OK;
	}

	// not in the reference (its light is three constants, Fluid.cpp:169-173): the scene light of the following renders (fx_set_light).
	// position: world space of UpdateFrame's view matrix (the volume is [-10, 10]^3 there); point = false: only its direction matters,
	// true: the light's place -- shadow rays run to it and end there.  color / ambient: rgb x intensity (w).  nullptr: the reference's constants
	bool SetLight(const fx_light* light) { m_status = fx_set_light(m_ctx, light); return m_status == FX_OK; }
	bool SetLight(const float position[3], bool point, const float color[4] = nullptr, const float ambient[4] = nullptr)
	{
		fx_light l;
		if ((m_status = fx_get_light(m_ctx, &l)) != FX_OK) return false;
		l.kind = point ? FX_LIGHT_POINT : FX_LIGHT_DIRECTIONAL;
		for (int a = 0; a < 3; ++a) l.position[a] = position[a];
		for (int a = 0; a < 4; ++a) { if (color) l.color[a] = color[a]; if (ambient) l.ambient[a] = ambient[a]; }
		return SetLight(&l);
	}
	bool GetLight(fx_light* out) { m_status = fx_get_light(m_ctx, out); return m_status == FX_OK; }

	// not in the reference: vorticity confinement between advection and divergence (fx_set_vorticity_confinement); 0 = off (default)
	bool SetVorticityConfinement(float epsilon) { m_status = fx_set_vorticity_confinement(m_ctx, epsilon); return m_status == FX_OK; }

	// not in the reference (its only source is the impulse compiled into its advection): smoke emitters applied behind every advection
	// (fx_set_emitters; count 0 = none, the default), and the switch of that built-in impulse (fx_set_impulse; default on)
	bool SetEmitters(const fx_emitter* list, uint32_t count) { m_status = fx_set_emitters(m_ctx, list, count); return m_status == FX_OK; }
	bool SetEmitters(const std::vector<fx_emitter>& list) { return SetEmitters(list.data(), (uint32_t)list.size()); }
	bool GetEmitters(std::vector<fx_emitter>& out)
	{
		uint32_t n = 0;
		out.resize(FX_MAX_EMITTERS);
		m_status = fx_get_emitters(m_ctx, out.data(), FX_MAX_EMITTERS, &n);
		out.resize(m_status == FX_OK ? n : 0);
		return m_status == FX_OK;
	}
	bool SetImpulse(bool enabled) { m_status = fx_set_impulse(m_ctx, enabled ? 1 : 0); return m_status == FX_OK; }
	// the emitter stage alone (fx_emit), beside the stage calls of the C interface
	bool Emit(void* stream = nullptr) { m_status = fx_emit(m_ctx, stream); return m_status == FX_OK; }

	// not in the reference (its only boundaries are the box's walls): voxelised solid obstacles the smoke flows around (fx_set_obstacles;
	// mask uint8[Z][Y][X], non-zero = solid; nullptr detaches).  Drawing the solids: SetObstacleDraw below
	bool SetObstacles(const uint8_t* solid, size_t bytes, void* stream = nullptr, bool deviceMemory = false)
	{
		m_status = fx_set_obstacles(m_ctx, stream, solid, bytes, deviceMemory ? FX_OBSTACLES_DEVICE : 0u);
		return m_status == FX_OK;
	}
	bool SetObstacles(const std::vector<uint8_t>& solid) { return SetObstacles(solid.data(), solid.size()); }
	bool GetObstacles(std::vector<uint8_t>& out, uint64_t* solidCells = nullptr)
	{
		out.assign(fx_field_bytes(m_ctx, FX_FIELD_PRESSURE) / sizeof(float), 0);        // one byte per cell
		m_status = fx_get_obstacles(m_ctx, out.data(), out.size(), solidCells);
		return m_status == FX_OK;
	}
	// the enforce stage alone (fx_enforce_obstacles), beside Emit
	bool EnforceObstacles(void* stream = nullptr) { m_status = fx_enforce_obstacles(m_ctx, stream); return m_status == FX_OK; }

	// the rigid-body velocities of the solids under the mask (fx_set_obstacle_bodies; count 0 = every solid rests, the default): a moving
	// object is a new mask and a new list per frame, and then pushes the smoke in front of it and drags it behind
	bool SetObstacleBodies(const fx_obstacle_body* list, uint32_t count) { m_status = fx_set_obstacle_bodies(m_ctx, list, count); return m_status == FX_OK; }
	bool SetObstacleBodies(const std::vector<fx_obstacle_body>& list) { return SetObstacleBodies(list.data(), (uint32_t)list.size()); }
	bool GetObstacleBodies(std::vector<fx_obstacle_body>& out)
	{
		uint32_t n = 0;
		out.resize(FX_MAX_OBSTACLE_BODIES);
		m_status = fx_get_obstacle_bodies(m_ctx, out.data(), FX_MAX_OBSTACLE_BODIES, &n);
		out.resize(m_status == FX_OK ? n : 0);
		return m_status == FX_OK;
	}
	// the mask from closed triangle meshes, voxelised on the device (fx_set_obstacle_meshes): the union of the meshes' solid sets replaces
	// the previous mask as SetObstacles would; a rigidly moving object is a new call with a new transform.  report may be null
	bool SetObstacleMeshes(const fx_obstacle_mesh* meshes, uint32_t count, fx_mesh_report* report = nullptr, void* stream = nullptr)
	{
		m_status = fx_set_obstacle_meshes(m_ctx, stream, meshes, count, report);
		return m_status == FX_OK;
	}
	// one host mesh: positions float[n][3] in texture space, indices uint32[m][3], transform float[12] (row-major 3 x 4) or null
	bool SetObstacleMesh(const std::vector<float>& positions, const std::vector<uint32_t>& indices, const float* transform = nullptr,
		fx_mesh_report* report = nullptr, void* stream = nullptr)
	{
		fx_obstacle_mesh m = {};
		m.struct_size = (uint32_t)sizeof m;
		m.positions = positions.data(); m.indices = indices.data();
		m.vertex_count = (uint32_t)(positions.size() / 3); m.triangle_count = (uint32_t)(indices.size() / 3);
		m.transform = transform;
		return SetObstacleMeshes(&m, 1, report, stream);
	}

	// not in the reference: the obstacle draw -- the solid cells of the mask ray-cast into the render target, lit by the scene light, and into a
	// depth buffer (fx_set_obstacle_draw: albedo rgb x intensity; nullptr = off, the default), the draw itself in front of Render
	// (fx_draw_obstacles; sceneDepthDevice: the caller's own scene or nullptr), its depth buffer attached as the scene depth of the following
	// renders (fx_obstacle_depth_device + fx_set_scene_depth) and the cast alone copied to the host (fx_obstacle_hits: uint64[H][W], float[H][W])
	bool SetObstacleDraw(const fx_obstacle_draw* draw) { m_status = fx_set_obstacle_draw(m_ctx, draw); return m_status == FX_OK; }
	bool SetObstacleDraw(const float albedo[4])
	{
		const fx_obstacle_draw d = { (uint32_t)sizeof(fx_obstacle_draw), 0u, { albedo[0], albedo[1], albedo[2], albedo[3] } };
		return SetObstacleDraw(&d);
	}
	bool GetObstacleDraw(fx_obstacle_draw& out) { m_status = fx_get_obstacle_draw(m_ctx, &out); return m_status == FX_OK; }
	bool DrawObstacles(uint8_t frameIndex = 0, const float* sceneDepthDevice = nullptr, void* stream = nullptr)
	{
		m_status = fx_draw_obstacles(m_ctx, stream, frameIndex, sceneDepthDevice);
		return m_status == FX_OK;
	}
	bool AttachObstacleDepth(float zNear = 1.0f, float zFar = 1000.0f, void* stream = nullptr)
	{
		void* depth = nullptr;
		m_status = fx_obstacle_depth_device(m_ctx, &depth);
		if (m_status == FX_OK && !depth) m_status = FX_E_STATE;
		if (m_status == FX_OK) m_status = fx_set_scene_depth(m_ctx, stream, static_cast<const float*>(depth), m_width, m_height, zNear, zFar, FX_DEPTH_DEVICE);
		return m_status == FX_OK;
	}
	bool ObstacleHits(uint64_t* hits, float* depth, size_t pixels, uint8_t frameIndex = 0, const float* sceneDepthDevice = nullptr, void* stream = nullptr)
	{
		m_status = fx_obstacle_hits(m_ctx, stream, frameIndex, sceneDepthDevice, hits, depth, pixels);
		return m_status == FX_OK;
	}

	// not in the reference (its box is closed): the faces through which the smoke leaves (fx_set_open_walls; FX_WALL_* bits, 0 = all closed,
	// the default) and the inflow stage alone (fx_open_inflow), directly behind the advection, beside Emit
	bool SetOpenWalls(uint32_t faces) { m_status = fx_set_open_walls(m_ctx, faces); return m_status == FX_OK; }
	bool GetOpenWalls(uint32_t& faces) { m_status = fx_get_open_walls(m_ctx, &faces); return m_status == FX_OK; }
	bool OpenInflow(void* stream = nullptr) { m_status = fx_open_inflow(m_ctx, stream); return m_status == FX_OK; }

	// not in the reference (it carries nothing but its grid fields): tracer particles that ride the flow -- records float[4] = (x, y, z, age) in
	// texture space, age >= 0 alive (fx_set_particles; count 0 frees the set, the default) --, moved by Simulate behind the projection; the
	// context's own buffer for zero-copy drawing (fx_particles_device), how they move (fx_set_particle_params; nullptr = the defaults), the
	// stage alone (fx_move_particles) and the velocity at points (fx_sample_velocity: points float[n][4], out float[n][3])
	bool SetParticles(const float* records, uint32_t count, void* stream = nullptr, bool deviceMemory = false)
	{
		m_status = fx_set_particles(m_ctx, stream, records, count, deviceMemory ? FX_PARTICLES_DEVICE : 0u);
		return m_status == FX_OK;
	}
	bool SetParticles(const std::vector<float>& records) { return SetParticles(records.data(), (uint32_t)(records.size() / 4)); }
	bool GetParticles(std::vector<float>& out)
	{
		uint32_t n = 0;
		if ((m_status = fx_get_particles(m_ctx, nullptr, 0, &n)) != FX_OK) { out.clear(); return false; }
		out.resize((size_t)n * 4);
		m_status = fx_get_particles(m_ctx, out.data(), n, &n);
		out.resize(m_status == FX_OK ? (size_t)n * 4 : 0);
		return m_status == FX_OK;
	}
	bool ParticlesDevice(void*& records, uint32_t& count) { m_status = fx_particles_device(m_ctx, &records, &count); return m_status == FX_OK; }
	bool SetParticleParams(const fx_particle_params* params) { m_status = fx_set_particle_params(m_ctx, params); return m_status == FX_OK; }
	bool SetParticleParams(uint32_t scheme, float driftX = 0.0f, float driftY = 0.0f, float driftZ = 0.0f, float lifetime = 0.0f)
	{
		const fx_particle_params p = { (uint32_t)sizeof(fx_particle_params), 0u, scheme, { driftX, driftY, driftZ }, lifetime };
		return SetParticleParams(&p);
	}
	bool GetParticleParams(fx_particle_params& out) { m_status = fx_get_particle_params(m_ctx, &out); return m_status == FX_OK; }
	bool MoveParticles(void* stream = nullptr) { m_status = fx_move_particles(m_ctx, stream); return m_status == FX_OK; }
	bool SampleVelocity(const float* points, uint32_t count, float* out, void* stream = nullptr, bool deviceMemory = false)
	{
		m_status = fx_sample_velocity(m_ctx, stream, points, count, out, deviceMemory ? FX_PARTICLES_DEVICE : 0u);
		return m_status == FX_OK;
	}

	// not in the reference: the particle sort -- the buffer of ParticlesDevice sorted on the device by cell, stable, dead records last
	// (fx_set_particle_sort: enabled allocates the scratch, every = n > 0 sorts in front of the move on every nth run of the particle stage;
	// nullptr = off, the default), the stage alone (fx_sort_particles), what the last sort counted (fx_particle_sort_info: the live records
	// occupy [0, live)) and the context's device arrays (fx_particle_order_device: order[i] = where the record now at i came from, and live)
	bool SetParticleSort(const fx_particle_sort* sort) { m_status = fx_set_particle_sort(m_ctx, sort); return m_status == FX_OK; }
	bool SetParticleSort(bool enabled, uint32_t every = 0)
	{
		const fx_particle_sort p = { (uint32_t)sizeof(fx_particle_sort), 0u, enabled ? 1u : 0u, every };
		return SetParticleSort(&p);
	}
	bool GetParticleSort(fx_particle_sort& out) { m_status = fx_get_particle_sort(m_ctx, &out); return m_status == FX_OK; }
	bool SortParticles(void* stream = nullptr) { m_status = fx_sort_particles(m_ctx, stream); return m_status == FX_OK; }
	bool ParticleSortInfo(uint32_t& live, uint32_t& sorts, void* stream = nullptr)
	{
		struct fx_particle_sort_info r = { (uint32_t)sizeof(struct fx_particle_sort_info), 0u, 0u, 0u };
		m_status = fx_particle_sort_info(m_ctx, stream, &r);
		live = r.live; sorts = r.sorts;
		return m_status == FX_OK;
	}
	bool ParticleOrderDevice(void*& order, void*& live) { m_status = fx_particle_order_device(m_ctx, &order, &live); return m_status == FX_OK; }
	// (a host copy of order is the caller's own device-to-host copy: this header does not include the HIP runtime)

	// not in the reference: the particle trail -- the particles as a source of smoke and heat (fx_set_particle_trail: every live particle
	// spreads `rate` per second over the eight cells around it, COLOR grows by tint and TEMPERATURE by heat per unit; nullptr = off, the
	// default), the stage alone (fx_deposit_particles) and the scatter alone copied to the host (fx_particle_density: uint64[Z][Y][X])
	bool SetParticleTrail(const fx_particle_trail* trail) { m_status = fx_set_particle_trail(m_ctx, trail); return m_status == FX_OK; }
	bool SetParticleTrail(float rate, const float tint[4], float heat = 0.0f)
	{
		const fx_particle_trail t = { (uint32_t)sizeof(fx_particle_trail), 0u, rate, { tint[0], tint[1], tint[2], tint[3] }, heat };
		return SetParticleTrail(&t);
	}
	bool GetParticleTrail(fx_particle_trail& out) { m_status = fx_get_particle_trail(m_ctx, &out); return m_status == FX_OK; }
	bool DepositParticles(void* stream = nullptr) { m_status = fx_deposit_particles(m_ctx, stream); return m_status == FX_OK; }
	bool ParticleDensity(uint64_t* out, size_t bytes, void* stream = nullptr)
	{
		m_status = fx_particle_density(m_ctx, stream, out, bytes);
		return m_status == FX_OK;
	}

	// not in the reference: the particle spawners -- records born on the device into dead slots of the set (fx_set_particle_spawners: up to
	// FX_MAX_PARTICLE_SPAWNERS boxes and ellipsoids with a rate; nullptr or count 0 = off, the default), the stage alone (fx_spawn_particles),
	// its counters and serials (fx_particle_spawn_info) and a set of `count` dead records to spawn into (SetParticlePool)
	bool SetParticleSpawners(const fx_particle_spawner* list, uint32_t count) { m_status = fx_set_particle_spawners(m_ctx, list, count); return m_status == FX_OK; }
	bool GetParticleSpawners(fx_particle_spawner* out, uint32_t capacity, uint32_t& count)
	{
		m_status = fx_get_particle_spawners(m_ctx, out, capacity, &count);
		return m_status == FX_OK;
	}
	bool SpawnParticles(void* stream = nullptr) { m_status = fx_spawn_particles(m_ctx, stream); return m_status == FX_OK; }
	bool ParticleSpawnInfo(struct fx_particle_spawn_info& out, void* stream = nullptr)
	{
		m_status = fx_particle_spawn_info(m_ctx, stream, &out);
		return m_status == FX_OK;
	}
	bool SetParticlePool(uint32_t count, void* stream = nullptr)
	{
		std::vector<float> dead((size_t)count * 4, 0.0f);
		for (uint32_t i = 0; i < count; ++i) dead[(size_t)i * 4 + 3] = -1.0f;
		m_status = fx_set_particles(m_ctx, stream, count ? dead.data() : nullptr, count, 0u);
		return m_status == FX_OK;
	}

	// not in the reference: the particle draw -- the live particles as emissive points on the render target, each dimmed by the smoke the
	// direct view march shows in front of it (fx_set_particle_draw: colour x intensity at age 0 and at the lifetime; nullptr = off, the
	// default), the draw itself on top of Render / RenderCube (fx_draw_particles) and the splat alone copied to the host
	// (fx_particle_splats: uint64[H][W][2])
	bool SetParticleDraw(const fx_particle_draw* draw) { m_status = fx_set_particle_draw(m_ctx, draw); return m_status == FX_OK; }
	bool SetParticleDraw(const float color[4], const float endColor[4])
	{
		const fx_particle_draw d = { (uint32_t)sizeof(fx_particle_draw), 0u, { color[0], color[1], color[2], color[3] },
			{ endColor[0], endColor[1], endColor[2], endColor[3] } };
		return SetParticleDraw(&d);
	}
	bool GetParticleDraw(fx_particle_draw& out) { m_status = fx_get_particle_draw(m_ctx, &out); return m_status == FX_OK; }
	bool DrawParticles(uint8_t frameIndex = 0, void* stream = nullptr) { m_status = fx_draw_particles(m_ctx, stream, frameIndex); return m_status == FX_OK; }
	bool ParticleSplats(uint64_t* out, size_t bytes, void* stream = nullptr)
	{
		m_status = fx_particle_splats(m_ctx, stream, out, bytes);
		return m_status == FX_OK;
	}

	// not in the reference (its advection is semi-Lagrangian): the advection scheme of Simulate and Advect (fx_set_advection_scheme;
	// FX_ADVECT_SEMI_LAGRANGIAN, the default, or FX_ADVECT_MACCORMACK)
	bool SetAdvectionScheme(uint32_t scheme) { m_status = fx_set_advection_scheme(m_ctx, scheme); return m_status == FX_OK; }
	bool GetAdvectionScheme(uint32_t& scheme) { m_status = fx_get_advection_scheme(m_ctx, &scheme); return m_status == FX_OK; }

	// not in the reference (its pressure solve is Jacobi sweeps only): the pressure solver of Simulate and PressureSolve (fx_set_pressure_solver;
	// nullptr or kind FX_PRESSURE_JACOBI = the default, FX_PRESSURE_MULTIGRID = geometric V-cycles), the stage alone (fx_pressure_solve) and a
	// level of the last solve (fx_download_pressure_level).  MultigridDefaults: 2 V(2,2) cycles, 16 coarse sweeps, omega 6/7 (3-D) or 4/5 (2-D)
	static fx_pressure_solver MultigridDefaults(bool is3d) { return fx_pressure_solver{ FX_PRESSURE_MULTIGRID, 0u, 2u, 2u, 2u, 16u, 0u, is3d ? 6.0f / 7.0f : 4.0f / 5.0f }; }
	bool SetPressureSolver(const fx_pressure_solver* solver) { m_status = fx_set_pressure_solver(m_ctx, solver); return m_status == FX_OK; }
	bool GetPressureSolver(fx_pressure_solver& solver) { m_status = fx_get_pressure_solver(m_ctx, &solver); return m_status == FX_OK; }
	bool PressureSolve(void* stream = nullptr) { m_status = fx_pressure_solve(m_ctx, stream); return m_status == FX_OK; }
	bool DownloadPressureLevel(uint32_t level, int what, float* host, size_t bytes) { m_status = fx_download_pressure_level(m_ctx, level, what, host, bytes); return m_status == FX_OK; }

	// not in the reference (its only lift is the constant force inside its impulse ball): buoyancy -- a temperature advected with the flow that
	// lifts the smoke, and the smoke's weight (fx_set_buoyancy; nullptr = off, the default) --, its heat sources (fx_set_heat_sources) and the
	// stage alone (fx_heat), beside Emit.  The field is FX_FIELD_TEMPERATURE while buoyancy is on
	bool SetBuoyancy(const fx_buoyancy* buoyancy) { m_status = fx_set_buoyancy(m_ctx, buoyancy); return m_status == FX_OK; }
	bool SetBuoyancy(float ambient, float densityWeight, float lift, float cooling, float upX = 0.0f, float upY = 1.0f, float upZ = 0.0f)
	{
		const fx_buoyancy b = { (uint32_t)sizeof(fx_buoyancy), 0u, ambient, densityWeight, lift, cooling, { upX, upY, upZ } };
		return SetBuoyancy(&b);
	}
	bool GetBuoyancy(fx_buoyancy& out, bool& enabled)
	{
		int on = 0;
		m_status = fx_get_buoyancy(m_ctx, &out, &on);
		enabled = on != 0;
		return m_status == FX_OK;
	}
	bool SetHeatSources(const fx_heat_source* list, uint32_t count) { m_status = fx_set_heat_sources(m_ctx, list, count); return m_status == FX_OK; }
	bool SetHeatSources(const std::vector<fx_heat_source>& list) { return SetHeatSources(list.data(), (uint32_t)list.size()); }
	bool GetHeatSources(std::vector<fx_heat_source>& out)
	{
		uint32_t n = 0;
		out.resize(FX_MAX_HEAT_SOURCES);
		m_status = fx_get_heat_sources(m_ctx, out.data(), FX_MAX_HEAT_SOURCES, &n);
		out.resize(m_status == FX_OK ? n : 0);
		return m_status == FX_OK;
	}
	bool Heat(void* stream = nullptr) { m_status = fx_heat(m_ctx, stream); return m_status == FX_OK; }

	// not in the reference (its state dies with the window): whole-grid state files, see fx_checkpoint_save
	bool SaveCheckpoint(const char* path) { m_status = fx_checkpoint_save(m_ctx, path); return m_status == FX_OK; }
	bool LoadCheckpoint(const char* path) { m_status = fx_checkpoint_load(m_ctx, path); return m_status == FX_OK; }

	// not in the reference: the void methods above cannot report failure there either (debug layer only)
	// waits for everything this object enqueued; false (LastStatus() == FX_E_HALO) if a multi-GPU step's advection left its halo:
	// the reference's void methods cannot report that, so a caller that renders or stores fields checks here (or LastStatus())
	bool Synchronize() { m_status = fx_synchronize(m_ctx); return m_status == FX_OK; }
	int LastStatus() const { return m_status; }
	fx_ctx* Handle() const { return m_ctx; }

protected:
	fx_ctx* m_ctx;
	int m_status = FX_OK;
	bool m_hasTarget = false;
	uint32_t m_width = 0, m_height = 0;
};

// SH side of class LightProbe (LightProbe.h:16-26); the DDS loader and the sky pass are out of scope
class LightProbe {
public:
	bool Init(const float* radianceCube /* float[6][n][n][3] */, uint32_t n)
	{
		if (!radianceCube || !n) return false;
		m_cube.assign(radianceCube, radianceCube + (size_t)6 * n * n * 3);
		m_n = n;
		return true;
	}
	// LightProbe::Init(..., fileName) (LightProbe.cpp:41-46): a DDS cube map in BC6H_UF16 such as Bin/Assets/rnl_cross.dds
	bool Init(Fluid& fluid, const char* fileName, uint32_t mip = 0)
	{
		FILE* fp = std::fopen(fileName, "rb");
		if (!fp) return false;
		std::vector<uint8_t> dds;
		uint8_t buf[65536];
		for (size_t got; (got = std::fread(buf, 1, sizeof buf, fp)) > 0;) dds.insert(dds.end(), buf, buf + got);
		std::fclose(fp);
		uint32_t size = 0, mips = 0;
		m_status = fx_dds_cube_info(dds.data(), dds.size(), &size, &mips);
		if (m_status != FX_OK || mip >= mips) return false;
		m_n = (size >> mip) ? size >> mip : 1;
		m_cube.resize((size_t)6 * m_n * m_n * 3);
		m_status = fx_dds_decode_cube(fluid.Handle(), dds.data(), dds.size(), mip, m_cube.data(), m_cube.size());
		return m_status == FX_OK;
	}
	// LightProbe::RenderEnvironment (LightProbe.cpp:85-97): the radiance cube as the sky behind the volume.  The first call
	// uploads the cube; draw it BEFORE Fluid::Render like the demo does (FluidX12.cpp:483)
	void RenderEnvironment(Fluid& fluid, void* pCommandList, uint8_t frameIndex)
	{
		if (!m_envSet) { m_status = fx_set_environment(fluid.Handle(), m_cube.data(), m_n); m_envSet = m_status == FX_OK; }
		if (m_envSet) m_status = fx_render_environment(fluid.Handle(), pCommandList, frameIndex);
		fluid.UseRenderTarget();
	}
	void TransformSH(Fluid& fluid) { m_status = fx_sh_transform(fluid.Handle(), m_cube.data(), m_n, m_sh); }   // LightProbeEZ.cpp:117-123
	const float* GetSH() const { return m_sh; }
	int LastStatus() const { return m_status; }
private:
	std::vector<float> m_cube;
	uint32_t m_n = 0;
	float m_sh[27] = {};
	int m_status = FX_OK;
	bool m_envSet = false;
};

}  // namespace fluidx
