// fluidx_demo.cpp -- the frame loop of the reference's demo driver (FluidX12/FluidX12.cpp) on the C++ shim:
// OnUpdate's time-step rule (:266) and default camera (:243-253), PopulateCommandList's Simulate + Render
// (:465,489-490), minus the window.  Build (after `python -m fluidx12_amd.build`):
//   hipcc -std=c++17 examples/fluidx_demo.cpp -o fluidx_demo -Lfluidx12_amd -lfluidx_hip -Wl,-rpath,$PWD/fluidx12_amd
// Usage: fluidx_demo [-gridSize X Y Z] [-maxRaySamples N] [-maxLightSamples N] [-radiance cube.dds] [-frames N] [-screenshot out.png|out.ppm] [-resume in.fxck] [-checkpoint out.fxck] [-vorticity E]
//        [-emitter CX CY CZ R]... [-noimpulse]     (smoke sources, fx_set_emitters: texture space [0,1]^3, with the built-in's colour and lift; -noimpulse: without the reference's own source)
//        [-obstacle CX CY CZ R]     (a solid ball the smoke flows around, fx_set_obstacles: texture space [0,1]^3; drawn only with -drawObstacle)
//        [-obstacleVelocity VX VY VZ]     (the ball moves: each frame it is voxelised anew at c + v * t, stopping at the walls, under one body with that velocity,
//                                          fx_set_obstacle_bodies: texture units per unit time; it then pushes the smoke in front of it and drags a wake)
//        [-obstacleMesh]     (the ball is handed over as a triangle mesh, fx_set_obstacle_meshes: a UV sphere of 16 x 32 segments built once and voxelised on the
//                             device; a moving ball is then moved by the mesh's transform alone, with no mask filled or uploaded per frame; 3-D grids)
//        [-openWalls BITS]     (faces through which the smoke leaves, fx_set_open_walls: 1 x-, 2 x+, 4 y-, 8 y+ (up), 16 z-, 32 z+; accepts 0x.. too)
//        [-advection maccormack|semi-lagrangian]     (the advection scheme, fx_set_advection_scheme; default: the reference's semi-Lagrangian step)
//        [-multigrid]     (the pressure solve as two multigrid V(2,2) cycles instead of the Jacobi sweeps, fx_set_pressure_solver)
//        [-light X Y Z] [-pointLight] [-lightColor R G B I] [-ambient R G B I]     (the scene light, fx_set_light: world space, the volume is [-10, 10]^3)
//        [-drawObstacle [R G B]]     (the ball itself, ray-cast from the voxel mask and lit by the scene light before the volume is rendered, its depth
//                                     attached so that the plume wraps around it, fx_set_obstacle_draw; albedo default 0.8 0.8 0.8, times 0.4; 3-D grids)
//        [-embers N]     (N tracer particles born at the built-in impulse, fx_set_particle_spawners, and drawn on top of the volume as glowing points that
//                         the smoke in front of them dims, fx_set_particle_draw; 3-D grids)
// (FluidX12.cpp:398-433; the screen shot is a PNG like the reference's (FluidX12.cpp:640-660), written without a compression library, or a binary PPM by extension)
#include "../fluidx12_amd/csrc/Fluid.hpp"
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include <algorithm>

using namespace fluidx;

static XMFLOAT4X4 LookAtLH(const float eye[3], const float at[3], const float up[3])
{
	float z[3] = { at[0] - eye[0], at[1] - eye[1], at[2] - eye[2] };
	float l = std::sqrt(z[0] * z[0] + z[1] * z[1] + z[2] * z[2]);
	for (float& v : z) v /= l;
	float x[3] = { up[1] * z[2] - up[2] * z[1], up[2] * z[0] - up[0] * z[2], up[0] * z[1] - up[1] * z[0] };
	l = std::sqrt(x[0] * x[0] + x[1] * x[1] + x[2] * x[2]);
	for (float& v : x) v /= l;
	const float y[3] = { z[1] * x[2] - z[2] * x[1], z[2] * x[0] - z[0] * x[2], z[0] * x[1] - z[1] * x[0] };
	auto dot = [&](const float* a) { return a[0] * eye[0] + a[1] * eye[1] + a[2] * eye[2]; };
	XMFLOAT4X4 m = { { { x[0], y[0], z[0], 0 }, { x[1], y[1], z[1], 0 }, { x[2], y[2], z[2], 0 }, { -dot(x), -dot(y), -dot(z), 1 } } };
	return m;
}

static XMFLOAT4X4 PerspectiveFovLH(float fovy, float aspect, float zn, float zf)
{
	const float h = std::cos(0.5f * fovy) / std::sin(0.5f * fovy), w = h / aspect, q = zf / (zf - zn);
	XMFLOAT4X4 m = { { { w, 0, 0, 0 }, { 0, h, 0, 0 }, { 0, 0, q, 1 }, { 0, 0, -q * zn, 0 } } };
	return m;
}

// A PNG of the RGBA8 render target, as FluidX12.cpp:640-660 saves one (8-bit RGBA, no interlace).  The pixel rows go into the zlib
// stream as STORED deflate blocks: every PNG reader takes that, and the demo needs no compression library.
static uint32_t crc32_of(const uint8_t* d, size_t n, uint32_t c = 0)
{
	static uint32_t table[256];
	if (!table[1]) for (uint32_t i = 0; i < 256; ++i) { uint32_t v = i; for (int k = 0; k < 8; ++k) v = (v & 1u) ? 0xEDB88320u ^ (v >> 1) : v >> 1; table[i] = v; }
	c = ~c;
	for (size_t i = 0; i < n; ++i) c = table[(c ^ d[i]) & 255u] ^ (c >> 8);
	return ~c;
}
static void png_chunk(FILE* fp, const char type[5], const std::vector<uint8_t>& body)
{
	std::vector<uint8_t> b(4 + body.size());
	std::memcpy(b.data(), type, 4);
	if (!body.empty()) std::memcpy(b.data() + 4, body.data(), body.size());
	const uint32_t len = (uint32_t)body.size(), crc = crc32_of(b.data(), b.size());
	const uint8_t l[4] = { (uint8_t)(len >> 24), (uint8_t)(len >> 16), (uint8_t)(len >> 8), (uint8_t)len };
	const uint8_t c[4] = { (uint8_t)(crc >> 24), (uint8_t)(crc >> 16), (uint8_t)(crc >> 8), (uint8_t)crc };
	std::fwrite(l, 1, 4, fp); std::fwrite(b.data(), 1, b.size(), fp); std::fwrite(c, 1, 4, fp);
}
static void write_png(FILE* fp, const uint8_t* rgba, uint32_t w, uint32_t h)
{
	static const uint8_t sig[8] = { 0x89, 'P', 'N', 'G', 0x0D, 0x0A, 0x1A, 0x0A };
	std::fwrite(sig, 1, 8, fp);
	std::vector<uint8_t> ihdr = { (uint8_t)(w >> 24), (uint8_t)(w >> 16), (uint8_t)(w >> 8), (uint8_t)w, (uint8_t)(h >> 24), (uint8_t)(h >> 16), (uint8_t)(h >> 8), (uint8_t)h, 8, 6, 0, 0, 0 };
	png_chunk(fp, "IHDR", ihdr);
	std::vector<uint8_t> raw;                                            // filter byte 0 + the row
	raw.reserve((size_t)h * (1 + 4 * (size_t)w));
	for (uint32_t y = 0; y < h; ++y) { raw.push_back(0); raw.insert(raw.end(), rgba + (size_t)y * w * 4, rgba + (size_t)(y + 1) * w * 4); }
	std::vector<uint8_t> z = { 0x78, 0x01 };
	uint32_t a = 1, b = 0;                                               // Adler-32 of the raw bytes
	for (size_t pos = 0; pos < raw.size() || pos == 0;) {
		const size_t n = std::min<size_t>(65535, raw.size() - pos);
		z.push_back(pos + n >= raw.size() ? 1 : 0);                       // BFINAL, BTYPE = 00 (stored)
		z.push_back((uint8_t)n); z.push_back((uint8_t)(n >> 8)); z.push_back((uint8_t)~n); z.push_back((uint8_t)(~n >> 8));
		z.insert(z.end(), raw.begin() + (ptrdiff_t)pos, raw.begin() + (ptrdiff_t)(pos + n));
		for (size_t i = pos; i < pos + n; ++i) { a = (a + raw[i]) % 65521u; b = (b + a) % 65521u; }
		pos += n;
		if (!n) break;
	}
	const uint32_t ad = (b << 16) | a;
	z.push_back((uint8_t)(ad >> 24)); z.push_back((uint8_t)(ad >> 16)); z.push_back((uint8_t)(ad >> 8)); z.push_back((uint8_t)ad);
	png_chunk(fp, "IDAT", z);
	png_chunk(fp, "IEND", {});
}

int main(int argc, char** argv)
{
	XMUINT3 grid = { 128, 128, 128 };                  // FluidX12.cpp:44
	uint32_t maxRay = 192, maxLight = 64, frames = 100; // FluidX12.cpp:38-39
	const uint32_t width = 800, height = 800;           // Main.cpp:17
	const char* screenshot = nullptr;
	const char* radiance = nullptr;                     // FluidGI.bat: -radiance Assets/rnl_cross.dds
	const char* resume = nullptr;                       // not in the reference: continue from / leave behind a state file
	const char* checkpoint = nullptr;
	float vorticity = 0.0f;                             // not in the reference: strength of the vorticity confinement, 0 = off
	std::vector<fx_emitter> emitters;                   // not in the reference: its only source is the impulse inside its advection
	bool noImpulse = false;
	bool obstacleSet = false;                           // not in the reference: its only boundaries are the box's walls
	float obstacle[4] = {};
	bool obstacleMoves = false;
	bool obstacleMesh = false;
	bool drawObstacle = false;                          // not in the reference: nothing but the volume is drawn there
	float obstacleAlbedo[4] = { 0.8f, 0.8f, 0.8f, 0.4f };   // (x 0.4: the reference's light is 3 pi + 1.5 pi strong)
	float obstacleVelocity[3] = {};
	uint32_t openWalls = 0;                             // not in the reference: its box is closed on all six faces
	uint32_t advection = FX_ADVECT_SEMI_LAGRANGIAN;     // not in the reference: its advection is semi-Lagrangian
	bool multigrid = false;                             // not in the reference: its pressure solve is Jacobi sweeps
	uint32_t embers = 0;                                // not in the reference: it has no particles
	bool lightSet = false, pointLight = false, colorSet = false, ambientSet = false;   // not in the reference: its light is three constants (Fluid.cpp:169-173)
	float lightPos[3] = { 75.0f, 75.0f, -75.0f }, lightColor[4] = {}, ambient[4] = {};
	for (int i = 1; i < argc; ++i) {
		if (!std::strcmp(argv[i], "-gridSize") && i + 3 < argc) { grid.x = atoi(argv[++i]); grid.y = atoi(argv[++i]); grid.z = atoi(argv[++i]); }
		else if (!std::strcmp(argv[i], "-maxRaySamples") && i + 1 < argc) maxRay = atoi(argv[++i]);
		else if (!std::strcmp(argv[i], "-maxLightSamples") && i + 1 < argc) maxLight = atoi(argv[++i]);
		else if (!std::strcmp(argv[i], "-frames") && i + 1 < argc) frames = atoi(argv[++i]);
		else if (!std::strcmp(argv[i], "-screenshot") && i + 1 < argc) screenshot = argv[++i];
		else if (!std::strcmp(argv[i], "-radiance") && i + 1 < argc) radiance = argv[++i];
		else if (!std::strcmp(argv[i], "-resume") && i + 1 < argc) resume = argv[++i];
		else if (!std::strcmp(argv[i], "-checkpoint") && i + 1 < argc) checkpoint = argv[++i];
		else if (!std::strcmp(argv[i], "-vorticity") && i + 1 < argc) vorticity = (float)atof(argv[++i]);
		else if (!std::strcmp(argv[i], "-emitter") && i + 4 < argc) {
			fx_emitter e = {};
			e.struct_size = sizeof e;
			for (float& v : e.center) v = (float)atof(argv[++i]);
			e.radius = (float)atof(argv[++i]);
			emitters.push_back(e);
		}
		else if (!std::strcmp(argv[i], "-noimpulse")) noImpulse = true;
		else if (!std::strcmp(argv[i], "-obstacle") && i + 4 < argc) { for (float& v : obstacle) v = (float)atof(argv[++i]); obstacleSet = true; }
		else if (!std::strcmp(argv[i], "-obstacleVelocity") && i + 3 < argc) { for (float& v : obstacleVelocity) v = (float)atof(argv[++i]); obstacleMoves = true; }
		else if (!std::strcmp(argv[i], "-obstacleMesh")) obstacleMesh = true;
		else if (!std::strcmp(argv[i], "-drawObstacle")) {
			drawObstacle = true;
			char* end = nullptr;                            // three numbers may follow
			if (i + 3 < argc && (std::strtod(argv[i + 1], &end), end != argv[i + 1] && !*end))
				for (int c = 0; c < 3; ++c) obstacleAlbedo[c] = (float)atof(argv[++i]);
		}
		else if (!std::strcmp(argv[i], "-openWalls") && i + 1 < argc) openWalls = (uint32_t)std::strtoul(argv[++i], nullptr, 0);
		else if (!std::strcmp(argv[i], "-advection") && i + 1 < argc) {
			const char* v = argv[++i];
			if (!std::strcmp(v, "maccormack")) advection = FX_ADVECT_MACCORMACK;
			else if (!std::strcmp(v, "semi-lagrangian")) advection = FX_ADVECT_SEMI_LAGRANGIAN;
			else { std::fprintf(stderr, "-advection %s: maccormack or semi-lagrangian\n", v); return 1; }
		}
		else if (!std::strcmp(argv[i], "-multigrid")) multigrid = true;
		else if (!std::strcmp(argv[i], "-embers") && i + 1 < argc) embers = (uint32_t)std::strtoul(argv[++i], nullptr, 0);
		else if (!std::strcmp(argv[i], "-light") && i + 3 < argc) { for (float& v : lightPos) v = (float)atof(argv[++i]); lightSet = true; }
		else if (!std::strcmp(argv[i], "-pointLight")) { pointLight = true; lightSet = true; }
		else if (!std::strcmp(argv[i], "-lightColor") && i + 4 < argc) { for (float& v : lightColor) v = (float)atof(argv[++i]); colorSet = lightSet = true; }
		else if (!std::strcmp(argv[i], "-ambient") && i + 4 < argc) { for (float& v : ambient) v = (float)atof(argv[++i]); ambientSet = lightSet = true; }
	}
	Fluid fluid;
	Fluid::Options options;
	if (obstacleSet) options.jacobiMode = FX_JACOBI_FIXED;   // obstacles are served by the fixed-count solve only (fx_set_obstacles refuses the per-cell early-out)
	if (!fluid.Init(nullptr, width, height, grid, options)) {   // ThrowIfFailed(E_FAIL) in the reference (FluidX12.cpp:198-200)
		std::fprintf(stderr, "Fluid::Init failed: %s\n", fx_error_string(fluid.LastStatus()));
		return 1;
	}
	fluid.SetMaxSamples(maxRay, maxLight);
	if (vorticity != 0.0f && !fluid.SetVorticityConfinement(vorticity)) { std::fprintf(stderr, "-vorticity %g: %s\n", vorticity, fx_error_string(fluid.LastStatus())); return 1; }
	for (fx_emitter& e : emitters) {                    // the built-in's colour, lift and swirl (Impulse.hlsli; 2-D: CSAdvect.hlsl's 48)
		const float rate[4] = { 8.0f, 16.0f, 40.0f, 40.0f };
		std::memcpy(e.color_rate, rate, sizeof rate);
		e.force[1] = grid.z > 1 ? 192.0f : 48.0f;
		e.swirl = 200.0f;
	}
	if (!emitters.empty() && !fluid.SetEmitters(emitters)) { std::fprintf(stderr, "-emitter: %s\n", fx_error_string(fluid.LastStatus())); return 1; }
	if (noImpulse && !fluid.SetImpulse(false)) { std::fprintf(stderr, "-noimpulse: %s\n", fx_error_string(fluid.LastStatus())); return 1; }
	// -obstacleMesh: the unit UV sphere about the origin, 16 stacks of 32 slices with the poles on y, built once; the ball is its image under
	// scale r, translate c
	std::vector<float> ballPositions;
	std::vector<uint32_t> ballIndices;
	if (obstacleMesh) {
		const uint32_t stacks = 16, slices = 32, south = 1 + (stacks - 1) * slices;
		const float pi = 3.14159265358979f;
		auto push = [&](float x, float y, float z) { ballPositions.push_back(x); ballPositions.push_back(y); ballPositions.push_back(z); };
		auto ring = [&](uint32_t i, uint32_t j) { return 1 + (i - 1) * slices + j % slices; };
		auto tri = [&](uint32_t a, uint32_t b, uint32_t c) { ballIndices.push_back(a); ballIndices.push_back(b); ballIndices.push_back(c); };
		push(0.0f, 1.0f, 0.0f);
		for (uint32_t i = 1; i < stacks; ++i)
			for (uint32_t j = 0; j < slices; ++j) {
				const float th = pi * i / stacks, ph = 2.0f * pi * j / slices;
				push(std::sin(th) * std::cos(ph), std::cos(th), std::sin(th) * std::sin(ph));
			}
		push(0.0f, -1.0f, 0.0f);
		for (uint32_t j = 0; j < slices; ++j) {
			tri(0, ring(1, j), ring(1, j + 1));
			tri(south, ring(stacks - 1, j + 1), ring(stacks - 1, j));
			for (uint32_t i = 1; i + 1 < stacks; ++i) {
				tri(ring(i, j), ring(i + 1, j), ring(i + 1, j + 1));
				tri(ring(i, j), ring(i + 1, j + 1), ring(i, j + 1));
			}
		}
	}
	// voxelise: the cells whose centre lies inside the ball at c + v * t, t clamped per axis where the ball meets a wall; with a velocity also the
	// one body whose box encloses the ball (an axis on which the ball has stopped no longer moves)
	auto placeObstacle = [&](float t) {
		float c[3], v[3];
		for (int a = 0; a < 3; ++a) {
			const float lo = std::min(obstacle[3], 0.5f), hi = 1.0f - lo, at = obstacle[a] + obstacleVelocity[a] * t;
			c[a] = std::min(std::max(at, std::min(lo, obstacle[a])), std::max(hi, obstacle[a]));
			v[a] = c[a] == at ? obstacleVelocity[a] : 0.0f;
		}
		if (obstacleMesh) {                                 // the library voxelises: 48 bytes of transform say where the ball is
			const float m[12] = { obstacle[3], 0, 0, c[0], 0, obstacle[3], 0, c[1], 0, 0, obstacle[3], c[2] };
			fx_mesh_report report = {};
			if (!fluid.SetObstacleMesh(ballPositions, ballIndices, m, &report)) return false;
			if (report.open_columns || report.skipped_triangles) std::fprintf(stderr, "-obstacleMesh: %u open columns, %u skipped triangles\n", report.open_columns, report.skipped_triangles);
		}
		std::vector<uint8_t> solid(obstacleMesh ? 0 : (size_t)grid.x * grid.y * grid.z, 0);
		for (uint32_t z = 0; z < grid.z && !obstacleMesh; ++z)
			for (uint32_t y = 0; y < grid.y; ++y)
				for (uint32_t x = 0; x < grid.x; ++x) {
					const float dx = (x + 0.5f) / grid.x - c[0], dy = (y + 0.5f) / grid.y - c[1];
					const float dz = grid.z > 1 ? (z + 0.5f) / grid.z - c[2] : 0.0f;
					solid[((size_t)z * grid.y + y) * grid.x + x] = dx * dx + dy * dy + dz * dz <= obstacle[3] * obstacle[3] ? 1 : 0;
				}
		if (!obstacleMesh && !fluid.SetObstacles(solid)) return false;
		if (!obstacleMoves) return true;
		fx_obstacle_body body = {};
		body.struct_size = sizeof body;
		for (int a = 0; a < 3; ++a) {
			body.box_lo[a] = c[a] - obstacle[3]; body.box_hi[a] = c[a] + obstacle[3];
			body.linear[a] = v[a]; body.pivot[a] = c[a];
		}
		return fluid.SetObstacleBodies(&body, 1);
	};
	if (obstacleMesh && !obstacleSet) { std::fprintf(stderr, "-obstacleMesh: there is no -obstacle to hand over\n"); return 1; }
	if (obstacleMoves && !obstacleSet) { std::fprintf(stderr, "-obstacleVelocity: there is no -obstacle to move\n"); return 1; }
	if (obstacleSet && !placeObstacle(0.0f)) { std::fprintf(stderr, "-obstacle: %s\n", fx_error_string(fluid.LastStatus())); return 1; }
	if (drawObstacle && (!obstacleSet || grid.z <= 1)) { std::fprintf(stderr, "-drawObstacle: there is no -obstacle on a 3-D grid to draw\n"); return 1; }
	if (drawObstacle && (!fluid.SetObstacleDraw(obstacleAlbedo) || !fluid.AttachObstacleDepth(1.0f, 1000.0f))) {   // (the projection's planes below)
		std::fprintf(stderr, "-drawObstacle: %s\n", fx_error_string(fluid.LastStatus()));
		return 1;
	}
	if (openWalls && !fluid.SetOpenWalls(openWalls)) { std::fprintf(stderr, "-openWalls 0x%x: %s\n", (unsigned)openWalls, fx_error_string(fluid.LastStatus())); return 1; }
	if (advection != FX_ADVECT_SEMI_LAGRANGIAN && !fluid.SetAdvectionScheme(advection)) { std::fprintf(stderr, "-advection: %s\n", fx_error_string(fluid.LastStatus())); return 1; }
	if (multigrid) {
		const fx_pressure_solver mg = Fluid::MultigridDefaults(grid.z > 1);
		if (!fluid.SetPressureSolver(&mg)) { std::fprintf(stderr, "-multigrid: %s\n", fx_error_string(fluid.LastStatus())); return 1; }
	}
	if (embers) {                                       // a pool of dead records, one ball spawner at the impulse that refills it over a lifetime, the draw
		const float lifetime = 2.0f, young[4] = { 1.0f, 0.6f, 0.2f, 4.0f }, old[4] = { 0.6f, 0.1f, 0.0f, 1.0f };
		fx_particle_params prm = { (uint32_t)sizeof(fx_particle_params), 0u, FX_PARTICLE_MIDPOINT, { 0.0f, 0.0f, 0.0f }, lifetime };
		const fx_particle_spawner ball = { (uint32_t)sizeof(fx_particle_spawner), 0u, FX_SPAWN_BALL, 1u, { 0.5f, 0.1f, 0.5f }, { 0.05f, 0.05f, 0.05f }, embers / lifetime, 0.0f };
		if (!fluid.SetParticlePool(embers) || !fluid.SetParticleParams(&prm) || !fluid.SetParticleSpawners(&ball, 1) || !fluid.SetParticleDraw(young, old)) {
			std::fprintf(stderr, "-embers %u: %s\n", (unsigned)embers, fx_error_string(fluid.LastStatus()));
			return 1;
		}
	}
	if (lightSet && grid.z <= 1) std::fprintf(stderr, "-light / -pointLight / -lightColor / -ambient: a 2-D grid has no light; ignored\n");
	if (lightSet && grid.z > 1 && !fluid.SetLight(lightPos, pointLight, colorSet ? lightColor : nullptr, ambientSet ? ambient : nullptr)) {
		std::fprintf(stderr, "-light / -pointLight / -lightColor / -ambient: %s\n", fx_error_string(fluid.LastStatus()));
		return 1;
	}
	if (resume && !fluid.LoadCheckpoint(resume)) { std::fprintf(stderr, "cannot resume from %s: %s\n", resume, fx_error_string(fluid.LastStatus())); return 1; }
	LightProbe probe;                                   // FluidX12.cpp:189-195, 205-210: load, TransformSH, SetSH
	if (radiance) {
		if (!probe.Init(fluid, radiance)) { std::fprintf(stderr, "cannot load %s as a BC6H_UF16 DDS cube map\n", radiance); return 1; }
		probe.TransformSH(fluid);
		fluid.SetSH(probe.GetSH());
		std::printf("light probe %s: SH L00 = (%.3f, %.3f, %.3f)\n", radiance, probe.GetSH()[0], probe.GetSH()[1], probe.GetSH()[2]);
	}
	const float eye[3] = { 4.0f, 16.0f, -40.0f }, at[3] = { 0, 0, 0 }, up[3] = { 0, 1, 0 };
	const XMFLOAT4X4 view = LookAtLH(eye, at, up);
	const XMFLOAT4X4 proj = PerspectiveFovLH(3.141592654f / 4.0f, width / (float)height, 1.0f, 1000.0f);
	const XMFLOAT3 eyePt = { eye[0], eye[1], eye[2] };
	const float timeStep = (grid.z > 1 ? 2.0f : 1.0f) / grid.y;    // FluidX12.cpp:266

	const auto t0 = std::chrono::steady_clock::now();
	for (uint32_t f = 0; f < frames; ++f) {
		const uint8_t frameIndex = f % Fluid::FrameCount;
		if (obstacleMoves && f > 0 && !placeObstacle(f * timeStep)) { std::fprintf(stderr, "frame %u, -obstacleVelocity: %s\n", f, fx_error_string(fluid.LastStatus())); return 1; }
		fluid.UpdateFrame(timeStep, frameIndex, view, proj, eyePt);
		fluid.Simulate(nullptr, frameIndex);
		const float clearColor[4] = { 0.2f, 0.2f, 0.2f, 0.0f };                    // FluidX12.cpp:471-472
		if (grid.z > 1) {
			fluid.ClearRenderTarget(nullptr, clearColor);
			if (radiance) probe.RenderEnvironment(fluid, nullptr, frameIndex);      // FluidX12.cpp:483: the sky first
			if (drawObstacle) fluid.DrawObstacles(frameIndex);                      // the ball, and its depth for the marches that follow
			fluid.Render(nullptr, frameIndex, Fluid::OPTIMIZED);                    // marches + renderCube onto the target
			if (embers) fluid.DrawParticles(frameIndex);                            // the embers on top, dimmed by the smoke in front of them
		}
		if (fluid.LastStatus() != FX_OK) { std::fprintf(stderr, "frame %u: %s\n", f, fx_error_string(fluid.LastStatus())); return 1; }
	}
	if (fx_synchronize(fluid.Handle()) != FX_OK) return 1;
	if (checkpoint && !fluid.SaveCheckpoint(checkpoint)) { std::fprintf(stderr, "cannot write %s: %s\n", checkpoint, fx_error_string(fluid.LastStatus())); return 1; }
	if (screenshot && grid.z > 1) {
		std::vector<uint8_t> rgba;
		if (!fluid.ReadRenderTarget(rgba)) { std::fprintf(stderr, "read-back failed\n"); return 1; }
		FILE* fp = std::fopen(screenshot, "wb");
		if (!fp) { std::perror(screenshot); return 1; }
		const size_t nl = std::strlen(screenshot);
		if (nl > 4 && !std::strcmp(screenshot + nl - 4, ".png")) write_png(fp, rgba.data(), width, height);      // FluidX12.cpp:640-660 writes a PNG (stbi_write_png)
		else {
			std::fprintf(fp, "P6\n%u %u\n255\n", width, height);
			for (size_t p = 0; p < (size_t)width * height; ++p) std::fwrite(&rgba[4 * p], 1, 3, fp);
		}
		std::fclose(fp);
	}
	const double s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
	fx_frame_info fi;
	fx_get_frame_info(fluid.Handle(), &fi);
	std::printf("%u frames of %ux%ux%u in %.3f s (%.1f fps); cube LOD %u (%u^2), %u ray samples, mask 0x%x\n",
		frames, grid.x, grid.y, grid.z, s, frames / s, fi.cube_lod, fi.cube_size, fi.ray_samples, fi.visibility_mask);
	return 0;
}
