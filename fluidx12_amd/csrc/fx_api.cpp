// fx_api.cpp -- the per-frame entry points of the C ABI declared in include/fluidx_hip.h: the HIP re-statement of class Fluid's
// host side (/root/reference/FluidX12/Content/Fluid.cpp): UpdateFrame, Simulate, Render, the caller-side cube resolve, the SH probe,
// and the slab-group set-up.  The command list becomes a HIP stream; the 3-slot upload constant buffers (Fluid.cpp:239-252) become
// kernel arguments passed by value (no host/device hazard, so `frame_index` only needs range-checking).  Contexts and fields:
// fx_context.cpp; the step's schedule: fx_schedule.cpp.
//
// No CPU fallback and nothing from oracle/: every field operation is a HIP kernel.
#include "fx_host.h"
#include <cstring>
#include "fx_hostmath.h"
#include "fx_mesh_args.h"

using namespace fx;
using namespace fxh;

// ===================================================================================================
extern "C" {

int fx_abi_version(void) { return FX_ABI_VERSION; }

int fx_set_max_samples(fx_ctx* ctx, uint32_t max_ray, uint32_t max_light)
{
	if (!ctx || !max_ray || !max_light) return FX_E_INVALID;
	ctx->max_ray_samples = max_ray;
	ctx->max_light_samples = max_light;
	return FX_OK;
}

int fx_set_sh(fx_ctx* ctx, const float* coeffs27)
{
	if (!ctx) return FX_E_INVALID;
	if (!ctx->sh_dev) return FX_E_STATE;
	if (!coeffs27) { ctx->has_sh = false; return FX_OK; }
	DeviceGuard dg(ctx->device);
	FX_HIP(hipMemcpy(ctx->sh_dev, coeffs27, 27 * sizeof(float), hipMemcpyHostToDevice));
	if (ctx->accel_ok && !ctx->accel.gi)               // scratch of the occlusion rays (fx_render_accel.hip); without it the render takes the chunked march
		if (hipMalloc((void**)&ctx->accel.gi, 3 * ctx->g.cells_owned() * sizeof(float)) != hipSuccess) { ctx->accel.gi = nullptr; (void)hipGetLastError(); }
	ctx->has_sh = true;
	return FX_OK;
}

int fx_update_frame(fx_ctx* ctx, float time_step, uint8_t frame_index,
	const float view[16], const float proj[16], const float eye[3])
{
	if (!ctx || frame_index >= FX_FRAME_COUNT) return FX_E_INVALID;
	std::vector<fx_ctx*> M;
	for_members(ctx, M);
	if (!is_driver(ctx) || group_broken(ctx)) return FX_E_STATE;
	for (fx_ctx* c : M) {
		if (c->g.Zg > 1 && view && proj && eye && c->desc.viewport_w && c->desc.viewport_h) {   // a context without a viewport only simulates
			// Fluid.cpp:296-334
			const Mat4 world = Mat4::scaling(10.0f, 10.0f, 10.0f);              // m_volumeWorld, Fluid.cpp:182
			const Mat4 worldI = world.inverse();
			const Mat4 wvp = world * (Mat4::from(view) * Mat4::from(proj));
			worldI.store3x4(c->fc.world_i);
			world.store3x4(c->fc.world);
			const Mat4 vpI = (Mat4::from(view) * Mat4::from(proj)).inverse();   // LightProbe::UpdateFrame (LightProbe.cpp:70-76)
			for (int r = 0; r < 4; ++r)
				for (int q = 0; q < 4; ++q) c->fc.s2w[r * 4 + q] = vpI.m[q][r];
			const Mat4 wvpI = wvp.inverse();                                    // stored transposed (Fluid.cpp:318)
			for (int r = 0; r < 4; ++r)
				for (int q = 0; q < 4; ++q) { c->fc.wvp_i[r * 4 + q] = wvpI.m[q][r]; c->wvp[r * 4 + q] = wvp.m[q][r]; }   // (the forward one: scene depth)
			for (int a = 0; a < 3; ++a) c->fc.eye_pt[a] = eye[a];
			// (light point, light colour and ambient -- Fluid.cpp:169-173 -- belong to the context: fx_create, fx_set_light)

			// EstimateCubeMapLOD (Fluid.cpp:141-166)
			static const Vec3 corners[8] = { {1,1,1},{-1,1,1},{1,-1,1},{-1,-1,1},{-1,1,-1},{1,1,-1},{-1,-1,-1},{1,-1,-1} };
			static const uint8_t edges[12][2] = { {0,1},{3,2},{1,3},{2,0},{4,5},{7,6},{5,7},{6,4},{1,4},{6,3},{5,0},{2,7} };
			float sx[8], sy[8];
			for (int i = 0; i < 8; ++i) {
				const Vec3 q = wvp.transform_coord(corners[i]);
				sx[i] = (q.x * 0.5f + 0.5f) * (float)c->desc.viewport_w;
				sy[i] = (q.y * -0.5f + 0.5f) * (float)c->desc.viewport_h;
			}
			float edge = 0.0f;
			for (const auto& e : edges) {
				const float ex = sx[e[1]] - sx[e[0]], ey = sy[e[1]] - sy[e[0]];
				edge = std::max(std::sqrt(ex * ex + ey * ey), edge);
			}
			c->edge_pixels = edge;
			float s = edge / 2.0f;
			float amount = 2.0f * s / std::sqrt(3.0f);
			const uint32_t wanted = (uint32_t)std::ceil(amount);
			c->ray_samples = std::min(wanted, c->max_ray_samples);
			amount = std::min(amount, (float)c->ray_samples);
			s = amount / 2.0f * std::sqrt(3.0f);
			const uint8_t level = (uint8_t)std::max(std::log2((float)c->g.X / s), 0.0f);
			c->cube_lod = std::min<uint32_t>(level, kNumMips - 1);

			// GenVisibilityMask (Fluid.cpp:49-61)
			uint32_t mask = 0;
			for (uint32_t f = 0; f < 6; ++f) {
				const float v = worldI.transform_comp(eye, (int)(f >> 1));
				mask |= ((f & 1u) ? v > -1.0f : v < 1.0f) ? 1u << f : 0u;
			}
			c->visibility_mask = mask;
			c->view_valid = true;
		}
		c->time_step = time_step;
		if (time_step > 0.0f && !(c->desc.flags & FX_FLAG_RENDER_ONLY)) c->frame_parity ^= 1;   // Fluid.cpp:345
		c->frame_valid = true;
	}
	return FX_OK;
}

int fx_simulate(fx_ctx* ctx, void* stream, uint8_t frame_index)
{
	if (!ctx || frame_index >= FX_FRAME_COUNT) return FX_E_INVALID;
	if (!ctx->frame_valid || (ctx->desc.flags & FX_FLAG_RENDER_ONLY) || group_broken(ctx)) return FX_E_STATE;
	if (!is_driver(ctx)) return FX_OK;             // loop-back group: rank 0 drives every member
	ctx->last_step_stream = pick_stream(ctx, stream);
	return simulate_impl(ctx, ctx->last_step_stream);
}

// the zero fill is ordered on the stream the target is about to be used on (the context's streams do not synchronise
// with the NULL stream)
static int ensure_target(fx_ctx* ctx, hipStream_t s)
{
	if (ctx->target) return FX_OK;
	const size_t n = (size_t)ctx->desc.viewport_w * ctx->desc.viewport_h;
	if (!n) return FX_E_INVALID;
	FX_HIP(hipMalloc((void**)&ctx->target, n * 4));
	FX_HIP(hipMemsetAsync(ctx->target, 0, n * 4, s));
	FX_HIP(hipMalloc((void**)&ctx->target_float, n * 16));
	FX_HIP(hipMemsetAsync(ctx->target_float, 0, n * 16, s));
	return FX_OK;
}

// the scene depth's kernel argument (fx_set_scene_depth) for the cube mip `lod` (fx_render, fx_render_cube); false when none is attached
static bool depth_args(const fx_ctx* c, uint32_t lod, DepthArgs* da)
{
	if (!c->depth) return false;
	da->depth = c->depth;
	da->W = (int)c->desc.viewport_w; da->H = (int)c->desc.viewport_h;
	std::memcpy(da->wvp, c->wvp, sizeof da->wvp);
	da->z_near = c->depth_zn; da->z_far = c->depth_zf;
	da->cube_depth = reinterpret_cast<float*>(reinterpret_cast<char*>(c->cube_depth) + c->cube_mip_offset[lod]);
	return true;
}

// The marches of one fx_render.  FX_OPT_RENDER_ACCEL (default): the acceleration structures of this frame's colour field are built
// first, inside the first pass's timing mark -- their cost belongs to the frame.
struct Marches {
	fx_ctx* c; const void* color; hipStream_t s; unsigned long long* cnt; bool accel, built, filled;
	DepthArgs da; const DepthArgs* dep;             // the scene depth of the view marches (null: none attached)
	Marches(fx_ctx* ctx, const void* col, hipStream_t st, unsigned long long* counters)
		: c(ctx), color(col), s(st), cnt(counters), accel(ctx->opt_render_accel && ctx->accel_ok), built(false), filled(false)
	{
		dep = depth_args(ctx, ctx->cube_lod, &da) ? &da : nullptr;
	}
	const float* sh() const { return c->has_sh ? c->sh_dev : nullptr; }
	int point() const { return c->light_kind == FX_LIGHT_POINT ? 1 : 0; }     // which instantiation of the light-ray kernels (fx_set_light)
	hipError_t build(bool for_light = false)
	{
		if (!accel || built) return hipSuccess;
		built = true;
		// (the side volume counts as current only when the advection that made this field wrote it: a full build also leaves it current,
		// but a render loop over a paused field would then time a cheaper build than a frame behind its own step gets -- not worth the ambiguity)
		const bool current = c->accel_alpha_of == color;
		if (!current) c->accel_alpha_of = nullptr;                   // the build overwrites the side volume with this field's alpha
		c->rendered_since_step = true; c->rendered_on = s;
		c->accel.frame += 1;                                         // this render's set of counters
		// the filling pass may skip the cells whose light-map words nobody has touched since the last one wrote the same constant there
		float key[9];
		for (int i = 0; i < 4; ++i) { key[i] = c->fc.light_color[i]; key[4 + i] = c->fc.ambient[i]; }
		key[8] = c->has_sh ? 1.0f : 0.0f;
		const bool same = c->lightmap_filled && std::memcmp(key, c->lightmap_key, sizeof key) == 0;
		const LightFill lf{ c->lightmap, &c->fc, c->has_sh ? 1 : 0, same };
		if (for_light) c->accel.fill_frame += 1;
		const hipError_t e = launch_accel_build(c->g, c->half, color, c->accel, s, current, for_light ? &lf : nullptr, &filled);
		if (for_light) {
			if (!filled) c->accel.fill_frame -= 1;
			c->lightmap_filled = filled && e == hipSuccess;          // (another light path writes every word: no record)
			std::memcpy(c->lightmap_key, key, sizeof key);
		}
		return e;
	}
	hipError_t light()                                  // Fluid.cpp:857-878
	{
		hipError_t e = build(true);
		if (e != hipSuccess) return e;
		if (accel) return launch_accel_light(c->g, c->accel, c->lightmap, c->fc, sh(), c->max_light_samples, s, cnt, filled, point());
		c->lightmap_filled = false;
		return launch_raymarch_light(c->g, c->half, color, c->lightmap, c->fc, sh(), c->max_light_samples, s, cnt, point());
	}
	hipError_t view(int size, uint8_t* cube, bool separate)   // Fluid.cpp:880-908 (separate) / :825-855 (merged)
	{
		hipError_t e = build();
		if (e != hipSuccess) return e;
		const uint32_t ns = c->ray_samples;
		if (accel) return launch_accel_view(c->g, c->half, color, separate ? c->lightmap : nullptr, c->fc, separate ? nullptr : sh(), size,
			c->visibility_mask, ns, c->max_light_samples, separate, cube, c->accel, s, cnt, dep, point());
		return launch_raymarch_view(c->g, c->half, color, separate ? c->lightmap : nullptr, c->fc, separate ? nullptr : sh(), size,
			c->visibility_mask, ns, c->max_light_samples, separate, cube, s, cnt, dep, point());
	}
	hipError_t direct(int W, int H, bool separate)      // rayCastVDirect Fluid.cpp:953-972 / rayCastDirect :932-951
	{
		hipError_t e = build();
		if (e != hipSuccess) return e;
		const uint32_t ns = separate ? c->ray_samples : c->max_ray_samples;
		if (accel) return launch_accel_direct(c->g, c->half, color, separate ? c->lightmap : nullptr, c->fc, separate ? nullptr : sh(), W, H,
			ns, c->max_light_samples, separate, c->target, c->target_float, c->accel, s, cnt, dep, point());
		return launch_raycast_direct(c->g, c->half, color, separate ? c->lightmap : nullptr, c->fc, separate ? nullptr : sh(), W, H,
			ns, c->max_light_samples, separate, c->target, c->target_float, s, cnt, dep, point());
	}
};

int fx_render(fx_ctx* ctx, void* stream, uint8_t frame_index, uint8_t flags)
{
	if (!ctx || frame_index >= FX_FRAME_COUNT) return FX_E_INVALID;
	if (ctx->g.Zg <= 1) {                          // Fluid.cpp:445: else visualizeColor(pCommandList)
		if (!ctx->frame_valid) return FX_E_STATE;
		DeviceGuard dg2(ctx->device);
		hipStream_t s2 = pick_stream(ctx, stream);
		int rc = ensure_target(ctx, s2);
		if (rc) return rc;
		ScopedMark mk(ctx, s2, MK_VIEW);
		FX_HIP(launch_visualize_color(ctx->g, ctx->half, ctx->col[ctx->frame_parity], (int)ctx->desc.viewport_w,
			(int)ctx->desc.viewport_h, ctx->target, ctx->target_float, s2));
		if (ctx->timing_on) ctx->acc.renders += 1;
		return FX_OK;
	}
	if (!ctx->desc.viewport_w || !ctx->desc.viewport_h) return FX_E_INVALID;   // created without a viewport: nothing to project the cube onto
	if (!ctx->view_valid) return FX_E_STATE;
	if (ctx->g.nz != ctx->g.Zg) return FX_E_INVALID;            // rays cross slabs: multi-GPU rendering is row f-3
	// (tap indices are 32 bits wide and put together by 24-bit multiplies, fx_march.h make_taps)
	if ((uint64_t)ctx->g.Y * ((uint64_t)ctx->g.Zg + 1) >= (1u << 24) || ctx->g.cells_owned() >= ((size_t)1 << 32)) return FX_E_INVALID;
	unsigned long long* cnt = ctx->opt_count_samples ? ctx->sample_counters : nullptr;
	if (cnt && (flags & FX_SEPARATE_LIGHT_PASS)) ctx->acc.light_samples += (uint64_t)ctx->g.cells_owned();   // the light pass's own fetch per voxel
	DeviceGuard dg(ctx->device);
	hipStream_t s = pick_stream(ctx, stream);
	Marches m(ctx, ctx->col[ctx->frame_parity], s, cnt);
	const bool separate = (flags & FX_SEPARATE_LIGHT_PASS) != 0;
	if (!(flags & FX_RAY_MARCH_CUBEMAP)) {
		// direct screen-space marching (Fluid.cpp:432-443): one ray per pixel, straight onto the render target
		int rc = ensure_target(ctx, s);
		if (rc) return rc;
		if (separate) {
			ScopedMark mk(ctx, s, MK_LIGHT);
			FX_HIP(m.light());
		}
		ScopedMark mk(ctx, s, MK_VIEW);
		FX_HIP(m.direct((int)ctx->desc.viewport_w, (int)ctx->desc.viewport_h, separate));
		if (ctx->timing_on) ctx->acc.renders += 1;
		return FX_OK;
	}
	const int size = ctx->g.X >> ctx->cube_lod;
	uint8_t* cube = ctx->cube + ctx->cube_mip_offset[ctx->cube_lod];
	if (separate) {
		ScopedMark mk(ctx, s, MK_LIGHT);
		FX_HIP(m.light());
	}
	{
		ScopedMark mk(ctx, s, MK_VIEW);
		FX_HIP(m.view(size, cube, separate));
	}
	ctx->cube_depth_on[ctx->cube_lod] = m.dep != nullptr;          // what fx_render_cube resolves this mip with
	if (ctx->timing_on) ctx->acc.renders += 1;
	return FX_OK;
}

int fx_clear_render_target(fx_ctx* ctx, void* stream, const float rgba[4])
{
	if (!ctx || !rgba) return FX_E_INVALID;
	DeviceGuard dg(ctx->device);
	int rc = ensure_target(ctx, pick_stream(ctx, stream));
	if (rc) return rc;
	FX_HIP(launch_clear_target(ctx->target, (int)ctx->desc.viewport_w, (int)ctx->desc.viewport_h, rgba, pick_stream(ctx, stream)));
	return FX_OK;
}

int fx_render_cube(fx_ctx* ctx, void* stream, uint8_t frame_index)
{
	if (!ctx || frame_index >= FX_FRAME_COUNT) return FX_E_INVALID;
	if (ctx->g.Zg <= 1 || !ctx->cube) return FX_E_INVALID;
	if (!ctx->view_valid) return FX_E_STATE;
	if (ctx->g.nz != ctx->g.Zg) return FX_E_INVALID;
	DeviceGuard dg(ctx->device);
	hipStream_t s = pick_stream(ctx, stream);
	int rc = ensure_target(ctx, s);
	if (rc) return rc;
	// the depth-aware CubeCast only for a cube map that was marched with depth, and while depth is attached
	DepthArgs da;
	const bool dep = ctx->cube_depth_on[ctx->cube_lod] && depth_args(ctx, ctx->cube_lod, &da);
	ScopedMark mk(ctx, s, MK_RESOLVE);
	FX_HIP(launch_resolve_cube(ctx->cube + ctx->cube_mip_offset[ctx->cube_lod], ctx->g.X >> ctx->cube_lod, ctx->fc,
		(int)ctx->desc.viewport_w, (int)ctx->desc.viewport_h, ctx->target, ctx->target_float, s, dep ? &da : nullptr));
	return FX_OK;
}

int fx_set_scene_depth(fx_ctx* ctx, void* stream, const float* depth, uint32_t width, uint32_t height, float z_near, float z_far, uint32_t flags)
{
	if (!ctx || (flags & ~FX_DEPTH_DEVICE)) return FX_E_INVALID;
	// 2-D grids have no depth variant (PSVisualizeColor); a context without a viewport or a slab of a group does not march view rays
	if (ctx->g.Zg <= 1 || !ctx->cube_depth || ctx->g.nz != ctx->g.Zg) return FX_E_INVALID;
	if (!depth) { ctx->depth = nullptr; return FX_OK; }
	if (width != ctx->desc.viewport_w || height != ctx->desc.viewport_h || !(0.0f < z_near && z_near < z_far)) return FX_E_INVALID;
	DeviceGuard dg(ctx->device);
	if (flags & FX_DEPTH_DEVICE) {
		// read in place by the kernels: it must be memory this device can address (a host pointer here would fault the first render)
		hipPointerAttribute_t at;
		if (hipPointerGetAttributes(&at, depth) != hipSuccess) { (void)hipGetLastError(); return FX_E_INVALID; }
		if (at.type != hipMemoryTypeDevice && at.type != hipMemoryTypeManaged) return FX_E_INVALID;
		if (at.type == hipMemoryTypeDevice && at.device != ctx->device) return FX_E_INVALID;
		ctx->depth = depth;
	} else {
		const size_t bytes = (size_t)width * height * sizeof(float);
		if (!ctx->depth_own) FX_HIP(hipMalloc((void**)&ctx->depth_own, bytes));
		hipStream_t s = pick_stream(ctx, stream);
		FX_HIP(hipMemcpyAsync(ctx->depth_own, depth, bytes, hipMemcpyHostToDevice, s));   // behind the renders that read the previous copy
		FX_HIP(hipStreamSynchronize(s));                                                    // the caller's buffer may go when this returns
		ctx->depth = ctx->depth_own;
	}
	ctx->depth_zn = z_near;
	ctx->depth_zf = z_far;
	return FX_OK;
}

int fx_set_light(fx_ctx* ctx, const fx_light* light)
{
	if (!ctx) return FX_E_INVALID;
	if (ctx->g.Zg <= 1 || ctx->g.nz != ctx->g.Zg) return FX_E_INVALID;       // 2-D grids have no light; a slab of a group does not march rays
	if (!light) { default_light(ctx); return FX_OK; }
	if (light->struct_size != sizeof(fx_light)) return FX_E_INVALID;
	if (light->kind != FX_LIGHT_DIRECTIONAL && light->kind != FX_LIGHT_POINT) return FX_E_INVALID;
	for (int a = 0; a < 3; ++a) if (!std::isfinite(light->position[a])) return FX_E_INVALID;
	for (int a = 0; a < 4; ++a)                                              // (the light map is unsigned: R11G11B10_FLOAT)
		if (!std::isfinite(light->color[a]) || !std::isfinite(light->ambient[a]) || light->color[a] < 0.0f || light->ambient[a] < 0.0f) return FX_E_INVALID;
	if (light->kind == FX_LIGHT_DIRECTIONAL && light->position[0] == 0.0f && light->position[1] == 0.0f && light->position[2] == 0.0f) return FX_E_INVALID;
	std::memcpy(ctx->fc.light_pt, light->position, sizeof ctx->fc.light_pt);
	std::memcpy(ctx->fc.light_color, light->color, sizeof ctx->fc.light_color);
	std::memcpy(ctx->fc.ambient, light->ambient, sizeof ctx->fc.ambient);
	ctx->light_kind = light->kind;
	return FX_OK;
}

int fx_get_light(fx_ctx* ctx, fx_light* out)
{
	if (!ctx || !out) return FX_E_INVALID;
	out->struct_size = sizeof(fx_light);
	out->kind = ctx->light_kind;
	std::memcpy(out->position, ctx->fc.light_pt, sizeof out->position);
	std::memcpy(out->color, ctx->fc.light_color, sizeof out->color);
	std::memcpy(out->ambient, ctx->fc.ambient, sizeof out->ambient);
	return FX_OK;
}

int fx_set_environment(fx_ctx* ctx, const float* cube, uint32_t n)
{
	if (!ctx || (cube && (!n || n > 8192))) return FX_E_INVALID;
	DeviceGuard dg(ctx->device);
	FX_HIP(hipDeviceSynchronize());
	if (ctx->env) { FX_HIP(hipFree(ctx->env)); ctx->env = nullptr; ctx->env_n = 0; }
	if (!cube) return FX_OK;
	const size_t bytes = (size_t)6 * n * n * 3 * sizeof(float);
	FX_HIP(hipMalloc((void**)&ctx->env, bytes));
	FX_HIP(hipMemcpy(ctx->env, cube, bytes, hipMemcpyHostToDevice));
	ctx->env_n = n;
	return FX_OK;
}

int fx_render_environment(fx_ctx* ctx, void* stream, uint8_t frame_index)
{
	if (!ctx || frame_index >= FX_FRAME_COUNT) return FX_E_INVALID;
	if (!ctx->env || !ctx->view_valid) return FX_E_STATE;
	DeviceGuard dg(ctx->device);
	hipStream_t s = pick_stream(ctx, stream);
	int rc = ensure_target(ctx, s);
	if (rc) return rc;
	ScopedMark mk(ctx, s, MK_RESOLVE);
	FX_HIP(launch_environment(ctx->env, (int)ctx->env_n, ctx->fc, (int)ctx->desc.viewport_w, (int)ctx->desc.viewport_h,
		ctx->target, ctx->target_float, s));
	return FX_OK;
}

int fx_get_frame_info(fx_ctx* ctx, fx_frame_info* out)
{
	if (!ctx || !out) return FX_E_INVALID;
	out->cube_lod = ctx->cube_lod;
	out->cube_size = (uint32_t)ctx->g.X >> ctx->cube_lod;
	out->ray_samples = ctx->ray_samples;
	out->visibility_mask = ctx->visibility_mask;
	out->frame_parity = ctx->frame_parity;
	out->edge_pixels = ctx->edge_pixels;
	out->time_step = ctx->time_step;
	std::memcpy(out->world_view_proj_i, ctx->fc.wvp_i, sizeof out->world_view_proj_i);
	std::memcpy(out->screen_to_world, ctx->fc.s2w, sizeof out->screen_to_world);
	return FX_OK;
}

// ---- individual stages (parity tests, micro-benchmarks) ---------------------------------------------
int fx_advect(fx_ctx* ctx, void* stream)
{
	if (!ctx) return FX_E_INVALID;
	if (ctx->desc.flags & FX_FLAG_RENDER_ONLY) return FX_E_STATE;
	if (!ctx->frame_valid) return FX_E_STATE;
	if (ctx->nranks > 1) return FX_E_INVALID;
	hipStream_t s = pick_stream(ctx, stream);
	ScopedMark mk(ctx, s, MK_ADVECT);
	return advect_range(ctx, s, owned(ctx), false);
}

// ---- the optional stages of the step: vorticity confinement, emitters, obstacles, open walls, buoyancy ------------------------------
// Their calls want a context that simulates and, unless `whole` is false (the getters), holds the whole grid: FX_E_INVALID for null, FX_E_STATE for a render-only one,
// FX_E_INVALID for a slab or a rank of a chain -- each stage would need halo planes of its own there (the confinement two of velocity[1] across
// each face, the temperature a field's worth; the colour halos leave right behind the advection, in front of the passes that change it).
// A context never fails both of the last two tests: fx_create refuses a render-only slab, check_slab_chain a whole grid in a chain.
static int sim_guard(const fx_ctx* ctx, bool whole = true)
{
	if (!ctx) return FX_E_INVALID;
	if (ctx->desc.flags & FX_FLAG_RENDER_ONLY) return FX_E_STATE;
	if (whole && (ctx->g.nz != ctx->g.Zg || ctx->nranks > 1)) return FX_E_INVALID;
	return FX_OK;
}

// fx_<stage>(ctx, stream): the stage's phase of the step (fx_schedule.cpp) on its own
static int run_stage(fx_ctx* ctx, void* stream, int (*phase)(fx_ctx*, hipStream_t))
{
	const int rc = sim_guard(ctx);
	return rc ? rc : phase(ctx, pick_stream(ctx, stream));
}

int fx_set_vorticity_confinement(fx_ctx* ctx, float epsilon)
{
	if (!std::isfinite(epsilon) || epsilon < 0.0f) return FX_E_INVALID;
	if (const int rc = sim_guard(ctx)) return rc;
	ctx->vort_eps = epsilon;
	return FX_OK;
}

int fx_confine_vorticity(fx_ctx* ctx, void* stream) { return run_stage(ctx, stream, confine_phase); }

int fx_set_emitters(fx_ctx* ctx, const fx_emitter* list, uint32_t count)
{
	if (const int rc = sim_guard(ctx)) return rc;
	if (count > FX_MAX_EMITTERS || (count && !list)) return FX_E_INVALID;
	for (uint32_t k = 0; k < count; ++k) {
		const fx_emitter& e = list[k];
		if (e.struct_size != sizeof(fx_emitter) || e.flags != 0) return FX_E_INVALID;
		if (!std::isfinite(e.radius) || !(e.radius > 0.0f) || !std::isfinite(e.swirl)) return FX_E_INVALID;
		for (int a = 0; a < 3; ++a) if (!std::isfinite(e.center[a]) || !std::isfinite(e.force[a])) return FX_E_INVALID;
		for (int a = 0; a < 4; ++a) if (!std::isfinite(e.color_rate[a]) || e.color_rate[a] < 0.0f) return FX_E_INVALID;
	}
	ctx->emitters.assign(list, list + count);
	return FX_OK;
}

int fx_get_emitters(fx_ctx* ctx, fx_emitter* out, uint32_t capacity, uint32_t* count)
{
	if (const int rc = sim_guard(ctx, false)) return rc;             // (slab ranks may ask: the list is empty there)
	if (!count || (capacity && !out)) return FX_E_INVALID;
	*count = (uint32_t)ctx->emitters.size();
	for (uint32_t k = 0; k < capacity && k < *count; ++k) out[k] = ctx->emitters[k];
	return FX_OK;
}

int fx_set_impulse(fx_ctx* ctx, int enabled)
{
	if (const int rc = sim_guard(ctx, !enabled)) return rc;           // off: on the emitters' footing -- without it a slab rank has no source
	ctx->impulse_on = enabled != 0;
	return FX_OK;
}

int fx_emit(fx_ctx* ctx, void* stream) { return run_stage(ctx, stream, emit_phase); }

// ---- solid obstacles (fx_obstacle.hip) ------------------------------------------------------------------
// the tail the two mask setters share: the 0 / 1 bytes at `src` (device memory) become the code volume in obst_spare, the count and the box come
// back, and the new volume takes the place of the one in force.  obst_spare and obst_stats are allocated; blocks until `src` has been read
static int install_obstacle_mask(fx_ctx* ctx, const uint8_t* src, hipStream_t s)
{
	FX_HIP(launch_obstacle_codes(ctx->g, src, ctx->obst_spare, ctx->obst_stats, s));
	unsigned st[8];
	FX_HIP(hipMemcpyAsync(st, ctx->obst_stats, sizeof st, hipMemcpyDeviceToHost, s));
	FX_HIP(hipStreamSynchronize(s));                                        // the count and the box size the enforce launch; `solid` is free again
	std::swap(ctx->obst_code, ctx->obst_spare);
	ctx->obst_cells = (uint64_t)st[0] | ((uint64_t)st[1] << 32);
	for (int a = 0; a < 3; ++a) {
		ctx->obst_lo[a] = ctx->obst_cells ? (int)st[2 + a] : 0;
		ctx->obst_hi[a] = ctx->obst_cells ? (int)st[5 + a] + 1 : 0;
	}
	return FX_OK;
}

int fx_set_obstacles(fx_ctx* ctx, void* stream, const uint8_t* solid, size_t bytes, uint32_t flags)
{
	if (const int rc = sim_guard(ctx)) return rc;
	if (flags & ~(uint32_t)FX_OBSTACLES_DEVICE) return FX_E_INVALID;
	if (ctx->desc.jacobi_mode == FX_JACOBI_FAITHFUL) return FX_E_INVALID;  // the per-cell freeze solve has no obstacle-aware kernels
	DeviceGuard dg(ctx->device);
	if (!solid) {                                                           // detach: every launch is the plain one again
		if (ctx->obst_code) {
			if (ctx->obst_spare) FX_HIP(hipFree(ctx->obst_spare));          // (hipFree waits for the device: nothing reads the volume any more)
			ctx->obst_spare = ctx->obst_code;
			ctx->obst_code = nullptr;
		}
		ctx->obst_cells = 0;
		return FX_OK;
	}
	if (ctx->solver.kind == FX_PRESSURE_MULTIGRID) return FX_E_STATE;          // the multigrid solve has no coarse code volumes
	const size_t n = ctx->g.plane() * (size_t)ctx->g.Zg;
	if (bytes != n) return FX_E_INVALID;
	hipStream_t s = pick_stream(ctx, stream);
	// the new code volume is built beside the one in force, which stays in force if anything below fails
	if (!ctx->obst_spare && hipMalloc((void**)&ctx->obst_spare, n) != hipSuccess) { (void)hipGetLastError(); ctx->obst_spare = nullptr; return FX_E_NOMEM; }
	if (!ctx->obst_stats && hipMalloc((void**)&ctx->obst_stats, 8 * sizeof(unsigned)) != hipSuccess) { (void)hipGetLastError(); ctx->obst_stats = nullptr; return FX_E_NOMEM; }
	const uint8_t* src = solid;
	if (!(flags & FX_OBSTACLES_DEVICE)) {
		const int rc = ensure_stage(ctx, n);
		if (rc) return rc;
		FX_HIP(hipMemcpyAsync(ctx->stage, solid, n, hipMemcpyHostToDevice, s));
		src = reinterpret_cast<const uint8_t*>(ctx->stage);
	}
	return install_obstacle_mask(ctx, src, s);
}

int fx_get_obstacles(fx_ctx* ctx, uint8_t* solid_out, size_t bytes, uint64_t* solid_cells)
{
	if (const int rc = sim_guard(ctx, false)) return rc;
	const size_t n = ctx->g.plane() * (size_t)ctx->g.Zg;
	if (solid_out && bytes != n) return FX_E_INVALID;
	if (solid_cells) *solid_cells = ctx->obst_code ? ctx->obst_cells : 0;
	if (!solid_out) return FX_OK;
	if (!ctx->obst_code) { std::memset(solid_out, 0, n); return FX_OK; }
	DeviceGuard dg(ctx->device);
	FX_HIP(hipDeviceSynchronize());
	const int rc = ensure_stage(ctx, n);
	if (rc) return rc;
	FX_HIP(launch_obstacle_mask(ctx->obst_code, reinterpret_cast<uint8_t*>(ctx->stage), n, ctx->stream));
	FX_HIP(hipMemcpyAsync(solid_out, ctx->stage, n, hipMemcpyDeviceToHost, ctx->stream));
	FX_HIP(hipStreamSynchronize(ctx->stream));
	return FX_OK;
}

int fx_enforce_obstacles(fx_ctx* ctx, void* stream) { return run_stage(ctx, stream, enforce_phase); }

// ---- the solids' rigid-body velocities (fx_obstacle.hip): a host-side list like the emitters ---------------------------------
int fx_set_obstacle_bodies(fx_ctx* ctx, const fx_obstacle_body* list, uint32_t count)
{
	if (const int rc = sim_guard(ctx)) return rc;
	if (ctx->desc.jacobi_mode == FX_JACOBI_FAITHFUL) return FX_E_INVALID;  // on the obstacles' footing: fx_set_obstacles refuses these contexts
	if (count > FX_MAX_OBSTACLE_BODIES || (count && !list)) return FX_E_INVALID;
	for (uint32_t k = 0; k < count; ++k) {
		const fx_obstacle_body& b = list[k];
		if (b.struct_size != sizeof(fx_obstacle_body) || b.flags != 0) return FX_E_INVALID;
		for (int a = 0; a < 3; ++a) {
			if (!std::isfinite(b.box_lo[a]) || !std::isfinite(b.box_hi[a]) || !std::isfinite(b.linear[a]) || !std::isfinite(b.angular[a]) ||
				!std::isfinite(b.pivot[a])) return FX_E_INVALID;
			if (b.box_lo[a] > b.box_hi[a]) return FX_E_INVALID;
		}
	}
	ctx->obst_bodies.assign(list, list + count);
	return FX_OK;
}

int fx_get_obstacle_bodies(fx_ctx* ctx, fx_obstacle_body* out, uint32_t capacity, uint32_t* count)
{
	if (const int rc = sim_guard(ctx, false)) return rc;             // (slab ranks may ask: the list is empty there)
	if (!count || (capacity && !out)) return FX_E_INVALID;
	*count = (uint32_t)ctx->obst_bodies.size();
	for (uint32_t k = 0; k < capacity && k < *count; ++k) out[k] = ctx->obst_bodies[k];
	return FX_OK;
}

// ---- the mask from triangle meshes (fx_voxelize.hip): scatter and fill per mesh into the staging buffer, then fx_set_obstacles' own tail --------
int fx_set_obstacle_meshes(fx_ctx* ctx, void* stream, const fx_obstacle_mesh* meshes, uint32_t count, fx_mesh_report* report)
{
	if (const int rc = sim_guard(ctx)) return rc;
	if (const int rc = mesh_args_status(meshes, count)) return rc;
	if (ctx->g.Zg <= 1) return FX_E_INVALID;                                // a 2-D grid has no columns to fill
	if (ctx->desc.jacobi_mode == FX_JACOBI_FAITHFUL) return FX_E_INVALID;  // as fx_set_obstacles
	if (ctx->solver.kind == FX_PRESSURE_MULTIGRID) return FX_E_STATE;
	DeviceGuard dg(ctx->device);
	const Geom& g = ctx->g;
	const size_t n = g.plane() * (size_t)g.Zg;
	hipStream_t s = pick_stream(ctx, stream);
	// everything is allocated before anything is enqueued: the mask in force stays in force if one of these fails
	if (!ctx->obst_spare && hipMalloc((void**)&ctx->obst_spare, n) != hipSuccess) { (void)hipGetLastError(); ctx->obst_spare = nullptr; return FX_E_NOMEM; }
	if (!ctx->obst_stats && hipMalloc((void**)&ctx->obst_stats, 8 * sizeof(unsigned)) != hipSuccess) { (void)hipGetLastError(); ctx->obst_stats = nullptr; return FX_E_NOMEM; }
	if (!ctx->vox_report && hipMalloc((void**)&ctx->vox_report, kVoxReportWords * sizeof(unsigned)) != hipSuccess) { (void)hipGetLastError(); ctx->vox_report = nullptr; return FX_E_NOMEM; }
	if (!ctx->vox_bits) {
		const size_t bytes = (size_t)g.Y * g.Zg * voxel_row_words(g) * sizeof(unsigned);
		if (hipMalloc((void**)&ctx->vox_bits, bytes) != hipSuccess) { (void)hipGetLastError(); ctx->vox_bits = nullptr; return FX_E_NOMEM; }
		FX_HIP(hipMemsetAsync(ctx->vox_bits, 0, bytes, s));                 // once: the fill kernel leaves it all zero
	}
	const size_t work = mesh_work_bytes(meshes, count);
	if (ctx->vox_work_bytes < work) {
		if (ctx->vox_work) { FX_HIP(hipFree(ctx->vox_work)); ctx->vox_work = nullptr; ctx->vox_work_bytes = 0; }
		if (hipMalloc(&ctx->vox_work, work) != hipSuccess) { (void)hipGetLastError(); ctx->vox_work = nullptr; return FX_E_NOMEM; }
		ctx->vox_work_bytes = work;
	}
	if (const int rc = ensure_stage(ctx, n)) return rc;
	uint8_t* mask = reinterpret_cast<uint8_t*>(ctx->stage);
	FX_HIP(hipMemsetAsync(ctx->vox_report, 0, kVoxReportWords * sizeof(unsigned), s));
	for (uint32_t k = 0; k < count; ++k) {
		const fx_obstacle_mesh& m = meshes[k];
		VoxMesh vm = { m.positions, m.indices, m.transform, m.vertex_count, m.triangle_count };
		if (m.triangle_count && !(m.flags & FX_MESH_DEVICE)) {               // a host mesh: its copy lies behind the list of large triangles
			char* at = static_cast<char*>(ctx->vox_work) + (size_t)16 * m.triangle_count;
			const size_t ib = (size_t)12 * m.triangle_count, pb = (size_t)12 * m.vertex_count;
			FX_HIP(hipMemcpyAsync(at, m.indices, ib, hipMemcpyHostToDevice, s));
			vm.idx = reinterpret_cast<const uint32_t*>(at);
			if (pb) FX_HIP(hipMemcpyAsync(at + ib, m.positions, pb, hipMemcpyHostToDevice, s));
			vm.pos = reinterpret_cast<const float*>(at + ib);
			if (m.transform) {
				FX_HIP(hipMemcpyAsync(at + ib + pb, m.transform, 48, hipMemcpyHostToDevice, s));
				vm.xf = reinterpret_cast<const float*>(at + ib + pb);
			}
		}
		FX_HIP(launch_voxel_scatter(g, vm, ctx->vox_bits, ctx->vox_report, ctx->vox_report + 2 + k, static_cast<uint4*>(ctx->vox_work), s));
		if (k == 0 || m.triangle_count) FX_HIP(launch_voxel_fill(g, ctx->vox_bits, mask, k == 0, ctx->vox_report, s));
	}
	unsigned rep[2];
	FX_HIP(hipMemcpyAsync(rep, ctx->vox_report, sizeof rep, hipMemcpyDeviceToHost, s));
	if (const int rc = install_obstacle_mask(ctx, mask, s)) return rc;        // (synchronises: rep is there, the meshes are free again)
	if (report) {
		report->solid_cells = ctx->obst_cells;
		report->open_columns = rep[0];
		report->skipped_triangles = rep[1];
	}
	return FX_OK;
}

// ---- open walls (fx_open.hip) ---------------------------------------------------------------------------
int fx_set_open_walls(fx_ctx* ctx, uint32_t faces)
{
	if (const int rc = sim_guard(ctx)) return rc;
	if (!open_faces_ok(ctx->g, faces)) return FX_E_INVALID;                 // (a 2-D grid has no z faces)
	if (ctx->desc.jacobi_mode == FX_JACOBI_FAITHFUL) return FX_E_INVALID;  // the per-cell freeze solve has no open-wall kernels
	if (faces && ctx->solver.kind == FX_PRESSURE_MULTIGRID) return FX_E_STATE; // the multigrid solve knows closed walls only
	ctx->open_faces = faces;
	return FX_OK;
}

int fx_get_open_walls(fx_ctx* ctx, uint32_t* faces)
{
	if (!faces) return FX_E_INVALID;
	if (const int rc = sim_guard(ctx, false)) return rc;
	*faces = ctx->open_faces;
	return FX_OK;
}

int fx_open_inflow(fx_ctx* ctx, void* stream) { return run_stage(ctx, stream, open_inflow_phase); }

// ---- buoyancy (fx_heat.hip) -------------------------------------------------------------------------------
int fx_set_buoyancy(fx_ctx* ctx, const fx_buoyancy* b)
{
	if (const int rc = sim_guard(ctx)) return rc;
	DeviceGuard dg(ctx->device);
	if (!b) {                                                               // off: every call behaves as without this function, the field goes
		for (int i = 0; i < 2; ++i) {
			if (ctx->temp[i]) FX_HIP(hipFree(ctx->temp[i]));                // (hipFree waits for the device: nothing reads the volume any more)
			ctx->temp[i] = nullptr;
		}
		ctx->temp_cur = 0;
		ctx->buoy_on = false;
		const fx_buoyancy off = { (uint32_t)sizeof(fx_buoyancy), 0u, 0.0f, 0.0f, 0.0f, 0.0f, { 0.0f, 1.0f, 0.0f } };
		ctx->buoy = off;
		return FX_OK;
	}
	if (b->struct_size != sizeof(fx_buoyancy) || b->flags != 0) return FX_E_INVALID;
	if (!std::isfinite(b->ambient) || !std::isfinite(b->density_weight) || !std::isfinite(b->lift) || !std::isfinite(b->cooling)) return FX_E_INVALID;
	if (b->density_weight < 0.0f || b->cooling < 0.0f) return FX_E_INVALID;
	for (int a = 0; a < 3; ++a) if (!std::isfinite(b->up[a])) return FX_E_INVALID;
	if (b->up[0] == 0.0f && b->up[1] == 0.0f && b->up[2] == 0.0f) return FX_E_INVALID;
	if (!ctx->temp[0]) {                                                    // the first successful call: the ping-pong pair, both at the ambient value
		const size_t n = ctx->g.cells_owned();
		float* t[2] = { nullptr, nullptr };
		for (int i = 0; i < 2; ++i)
			if (hipMalloc((void**)&t[i], n * sizeof(float)) != hipSuccess) {
				(void)hipGetLastError();
				if (t[0]) (void)hipFree(t[0]);
				return FX_E_NOMEM;
			}
		uint32_t bits;
		std::memcpy(&bits, &b->ambient, sizeof bits);
		hipError_t e = hipMemsetD32Async((hipDeviceptr_t)t[0], (int)bits, n, ctx->stream);
		if (e == hipSuccess) e = hipMemsetD32Async((hipDeviceptr_t)t[1], (int)bits, n, ctx->stream);
		if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
		if (e != hipSuccess) { (void)hipGetLastError(); (void)hipFree(t[0]); (void)hipFree(t[1]); return FX_E_DEVICE; }
		ctx->temp[0] = t[0]; ctx->temp[1] = t[1];
		ctx->temp_cur = 0;
	}
	ctx->buoy = *b;
	ctx->buoy_on = true;
	return FX_OK;
}

int fx_get_buoyancy(fx_ctx* ctx, fx_buoyancy* out, int* enabled)
{
	if (const int rc = sim_guard(ctx, false)) return rc;
	if (out) *out = ctx->buoy;
	if (enabled) *enabled = ctx->buoy_on ? 1 : 0;
	return FX_OK;
}

int fx_set_heat_sources(fx_ctx* ctx, const fx_heat_source* list, uint32_t count)
{
	if (const int rc = sim_guard(ctx)) return rc;
	if (count > FX_MAX_HEAT_SOURCES || (count && !list)) return FX_E_INVALID;
	for (uint32_t k = 0; k < count; ++k) {
		const fx_heat_source& e = list[k];
		if (e.struct_size != sizeof(fx_heat_source) || e.flags != 0) return FX_E_INVALID;
		if (!std::isfinite(e.radius) || !(e.radius > 0.0f) || !std::isfinite(e.rate)) return FX_E_INVALID;
		for (int a = 0; a < 3; ++a) if (!std::isfinite(e.center[a])) return FX_E_INVALID;
	}
	ctx->heat_sources.assign(list, list + count);
	return FX_OK;
}

int fx_get_heat_sources(fx_ctx* ctx, fx_heat_source* out, uint32_t capacity, uint32_t* count)
{
	if (const int rc = sim_guard(ctx, false)) return rc;
	if (!count || (capacity && !out)) return FX_E_INVALID;
	*count = (uint32_t)ctx->heat_sources.size();
	for (uint32_t k = 0; k < capacity && k < *count; ++k) out[k] = ctx->heat_sources[k];
	return FX_OK;
}

int fx_heat(fx_ctx* ctx, void* stream) { return run_stage(ctx, stream, heat_phase); }

// ---- tracer particles and the point query (fx_particles.hip) ---------------------------------------------------
// The sort's scratch block for `count` records of this grid (fx_particle_sort_plan.cpp lays it out), its live word zeroed; blocks.  FX_E_INVALID
// for a grid the 32-bit key cannot number, FX_E_NOMEM; nothing of the context changes
static int psort_alloc(fx_ctx* ctx, uint32_t count, fx::PsortPlan* plan, void** mem)
{
	const uint64_t cells = (uint64_t)ctx->g.X * (uint64_t)ctx->g.Y * (uint64_t)ctx->g.Zg;
	if (fx::psort_plan(cells, count, FX_KNOB_INT("PSORT_KEY_BITS", 0), plan) != 0) return FX_E_INVALID;
	*mem = nullptr;
	if (hipMalloc(mem, plan->scratch_bytes) != hipSuccess) { (void)hipGetLastError(); *mem = nullptr; return FX_E_NOMEM; }
	if (hipMemset(static_cast<char*>(*mem) + plan->off_live, 0, 4) != hipSuccess || hipDeviceSynchronize() != hipSuccess) {
		(void)hipGetLastError(); (void)hipFree(*mem); *mem = nullptr;
		return FX_E_DEVICE;
	}
	return FX_OK;
}

// The set lives in a buffer of its own that only this call allocates and frees: the new one is filled beside the one in force, which stays in
// force if anything fails.  Blocks until the caller's records have been read.
int fx_set_particles(fx_ctx* ctx, void* stream, const float* records, uint32_t count, uint32_t flags)
{
	if (const int rc = sim_guard(ctx)) return rc;
	if (flags & ~(uint32_t)FX_PARTICLES_DEVICE) return FX_E_INVALID;
	if (count > FX_MAX_PARTICLES || (count && !records)) return FX_E_INVALID;
	DeviceGuard dg(ctx->device);
	float* fresh = nullptr;
	void* sort_mem = nullptr;                                               // while sorting is enabled: the scratch of the new count, on the same terms
	fx::PsortPlan sort_plan = {};
	if (ctx->psort_mem)
		if (const int rc = psort_alloc(ctx, count, &sort_plan, &sort_mem)) return rc;
	if (count) {
		const size_t bytes = (size_t)count * 16;
		if (hipMalloc((void**)&fresh, bytes) != hipSuccess) { (void)hipGetLastError(); if (sort_mem) (void)hipFree(sort_mem); return FX_E_NOMEM; }
		hipStream_t s = pick_stream(ctx, stream);
		hipError_t e = hipMemcpyAsync(fresh, records, bytes, (flags & FX_PARTICLES_DEVICE) ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, s);
		if (e == hipSuccess) e = hipStreamSynchronize(s);
		if (e != hipSuccess) {
			(void)hipGetLastError(); (void)hipFree(fresh);
			if (sort_mem) (void)hipFree(sort_mem);
			ctx->last_error = std::string("fx_set_particles: ") + hipGetErrorString(e);
			return FX_E_DEVICE;
		}
	}
	if (ctx->part) FX_HIP(hipFree(ctx->part));                              // (hipFree waits for the device: nothing moves the old set any more)
	ctx->part = fresh;
	ctx->part_count = count;
	if (sort_mem) {
		(void)hipFree(ctx->psort_mem);
		ctx->psort_mem = sort_mem;
		ctx->psort = sort_plan;
	}
	ctx->psort_runs = ctx->psort_sorts = 0;
	return FX_OK;
}

int fx_get_particles(fx_ctx* ctx, float* out, uint32_t capacity, uint32_t* count)
{
	if (const int rc = sim_guard(ctx, false)) return rc;             // (slab ranks may ask: the set is empty there)
	if (!count || (capacity && !out)) return FX_E_INVALID;
	*count = ctx->part_count;
	const uint32_t n = std::min(capacity, ctx->part_count);
	if (!n) return FX_OK;
	DeviceGuard dg(ctx->device);
	FX_HIP(hipDeviceSynchronize());
	FX_HIP(hipMemcpy(out, ctx->part, (size_t)n * 16, hipMemcpyDeviceToHost));
	return FX_OK;
}

int fx_particles_device(fx_ctx* ctx, void** records, uint32_t* count)
{
	if (const int rc = sim_guard(ctx, false)) return rc;
	if (records) *records = ctx->part;
	if (count) *count = ctx->part_count;
	return FX_OK;
}

int fx_set_particle_params(fx_ctx* ctx, const fx_particle_params* p)
{
	if (const int rc = sim_guard(ctx)) return rc;
	const fx_particle_params def = { (uint32_t)sizeof(fx_particle_params), 0u, FX_PARTICLE_MIDPOINT, { 0.0f, 0.0f, 0.0f }, 0.0f };
	if (!p) { ctx->part_prm = def; return FX_OK; }
	if (p->struct_size != sizeof(fx_particle_params) || p->flags != 0) return FX_E_INVALID;
	if (p->scheme != FX_PARTICLE_EULER && p->scheme != FX_PARTICLE_MIDPOINT) return FX_E_INVALID;
	for (int a = 0; a < 3; ++a) if (!std::isfinite(p->drift[a])) return FX_E_INVALID;
	if (!std::isfinite(p->lifetime) || p->lifetime < 0.0f) return FX_E_INVALID;
	ctx->part_prm = *p;
	return FX_OK;
}

int fx_get_particle_params(fx_ctx* ctx, fx_particle_params* out)
{
	if (const int rc = sim_guard(ctx, false)) return rc;
	if (!out) return FX_E_INVALID;
	*out = ctx->part_prm;
	return FX_OK;
}

int fx_move_particles(fx_ctx* ctx, void* stream) { return run_stage(ctx, stream, particles_phase); }

// ---- the particle sort (fx_particle_sort.hip) -------------------------------------------------------------------
// Enabling allocates the scratch of the set in force (fx_set_particles resizes it from then on), disabling frees it; either way the stage's run
// counter and the sort counter start again.  Blocks.
int fx_set_particle_sort(fx_ctx* ctx, const fx_particle_sort* p)
{
	if (const int rc = sim_guard(ctx)) return rc;
	const fx_particle_sort def = { (uint32_t)sizeof(fx_particle_sort), 0u, 0u, 0u };
	if (!p) p = &def;
	if (p->struct_size != sizeof(fx_particle_sort) || p->flags != 0 || p->enabled > 1u || (p->every && !p->enabled)) return FX_E_INVALID;
	DeviceGuard dg(ctx->device);
	if (p->enabled && !ctx->psort_mem) {
		void* mem = nullptr;
		fx::PsortPlan plan = {};
		if (const int rc = psort_alloc(ctx, ctx->part_count, &plan, &mem)) return rc;
		ctx->psort_mem = mem;
		ctx->psort = plan;
	} else if (!p->enabled && ctx->psort_mem) {
		FX_HIP(hipFree(ctx->psort_mem));                                    // (waits for the device: no sort is in flight any more)
		ctx->psort_mem = nullptr;
		ctx->psort = fx::PsortPlan{};
	}
	ctx->psort_cfg = *p;
	ctx->psort_runs = ctx->psort_sorts = 0;
	return FX_OK;
}

int fx_get_particle_sort(fx_ctx* ctx, fx_particle_sort* out)
{
	if (const int rc = sim_guard(ctx, false)) return rc;
	if (!out) return FX_E_INVALID;
	*out = ctx->psort_cfg;
	return FX_OK;
}

int fx_sort_particles(fx_ctx* ctx, void* stream) { return run_stage(ctx, stream, sort_particles_phase); }

int fx_particle_sort_info(fx_ctx* ctx, void* stream, struct fx_particle_sort_info* out)
{
	if (const int rc = sim_guard(ctx, false)) return rc;
	if (!out) return FX_E_INVALID;
	struct fx_particle_sort_info r = { (uint32_t)sizeof(struct fx_particle_sort_info), 0u, ctx->psort_sorts, 0u };
	if (ctx->psort_mem) {
		DeviceGuard dg(ctx->device);
		hipStream_t s = pick_stream(ctx, stream);
		FX_HIP(hipMemcpyAsync(&r.live, static_cast<char*>(ctx->psort_mem) + ctx->psort.off_live, 4, hipMemcpyDeviceToHost, s));
		FX_HIP(hipStreamSynchronize(s));
	}
	*out = r;
	return FX_OK;
}

int fx_particle_order_device(fx_ctx* ctx, void** order_u32, void** live_u32)
{
	if (const int rc = sim_guard(ctx)) return rc;
	if (!order_u32 || !live_u32) return FX_E_INVALID;
	if (!ctx->psort_mem) return FX_E_STATE;
	char* m = static_cast<char*>(ctx->psort_mem);
	*order_u32 = ctx->part_count ? m + ctx->psort.off_order : nullptr;
	*live_u32 = m + ctx->psort.off_live;
	return FX_OK;
}

// ---- the particle trail (fx_particle_trail.hip) -----------------------------------------------------------------
// The accumulator is allocated, zeroed, by the first call that sets a trail and freed by NULL; a later call replaces the rates and keeps it (it is
// all zero between calls).  Blocks.
int fx_set_particle_trail(fx_ctx* ctx, const fx_particle_trail* t)
{
	if (const int rc = sim_guard(ctx)) return rc;
	DeviceGuard dg(ctx->device);
	if (!t) {
		if (ctx->trail_acc) FX_HIP(hipFree(ctx->trail_acc));                // (hipFree waits for the device: no deposit is in flight any more)
		ctx->trail_acc = nullptr;
		const fx_particle_trail off = { (uint32_t)sizeof(fx_particle_trail), 0u, 0.0f, { 0.0f, 0.0f, 0.0f, 0.0f }, 0.0f };
		ctx->trail = off;
		return FX_OK;
	}
	if (t->struct_size != sizeof(fx_particle_trail) || t->flags != 0) return FX_E_INVALID;
	if (!std::isfinite(t->rate) || t->rate < 0.0f || !std::isfinite(t->heat)) return FX_E_INVALID;
	for (int a = 0; a < 4; ++a) if (!std::isfinite(t->tint[a])) return FX_E_INVALID;
	if (!ctx->trail_acc) {
		const size_t bytes = ctx->g.cells_owned() * sizeof(unsigned long long);
		unsigned long long* acc = nullptr;
		if (hipMalloc((void**)&acc, bytes) != hipSuccess) { (void)hipGetLastError(); return FX_E_NOMEM; }
		hipError_t e = hipMemsetAsync(acc, 0, bytes, ctx->stream);
		if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
		if (e != hipSuccess) { (void)hipGetLastError(); (void)hipFree(acc); return FX_E_DEVICE; }
		ctx->trail_acc = acc;
	}
	ctx->trail = *t;
	return FX_OK;
}

int fx_get_particle_trail(fx_ctx* ctx, fx_particle_trail* out)
{
	if (const int rc = sim_guard(ctx, false)) return rc;
	if (!out) return FX_E_INVALID;
	*out = ctx->trail;
	return FX_OK;
}

int fx_deposit_particles(fx_ctx* ctx, void* stream)
{
	if (const int rc = sim_guard(ctx)) return rc;
	if (!ctx->trail_acc) return FX_E_STATE;
	return trail_phase(ctx, pick_stream(ctx, stream));
}

// The scatter alone, the accumulator copied out and cleared again; blocks.  (The stage buffer is not used: the copy goes straight to the caller.)
int fx_particle_density(fx_ctx* ctx, void* stream, uint64_t* out, size_t bytes)
{
	if (const int rc = sim_guard(ctx)) return rc;
	if (!out || bytes != ctx->g.cells_owned() * sizeof(uint64_t)) return FX_E_INVALID;
	if (!ctx->trail_acc) return FX_E_STATE;
	hipStream_t s = pick_stream(ctx, stream);
	if (const int rc = trail_splat_phase(ctx, s)) return rc;
	DeviceGuard dg(ctx->device);
	FX_HIP(hipMemcpyAsync(out, ctx->trail_acc, bytes, hipMemcpyDeviceToHost, s));
	FX_HIP(hipMemsetAsync(ctx->trail_acc, 0, bytes, s));
	FX_HIP(hipStreamSynchronize(s));
	return FX_OK;
}

int fx_sample_velocity(fx_ctx* ctx, void* stream, const float* points, uint32_t count, float* out, uint32_t flags)
{
	if (const int rc = sim_guard(ctx)) return rc;
	if (flags & ~(uint32_t)FX_PARTICLES_DEVICE) return FX_E_INVALID;
	if (count > FX_MAX_PARTICLES) return FX_E_INVALID;
	if (count == 0) return FX_OK;
	if (!points || !out) return FX_E_INVALID;
	DeviceGuard dg(ctx->device);
	hipStream_t s = pick_stream(ctx, stream);
	if (flags & FX_PARTICLES_DEVICE) {                                      // enqueue only: the kernel loads a point as one 16-byte vector
		if (((uintptr_t)points & 15u) || ((uintptr_t)out & 3u)) return FX_E_INVALID;
		FX_HIP(launch_sample_velocity(ctx->g, ctx->half, ctx->vel[0], points, out, count, s));
		return FX_OK;
	}
	const size_t in_bytes = (size_t)count * 16, out_bytes = (size_t)count * 12;
	if (const int rc = ensure_stage(ctx, in_bytes + out_bytes)) return rc;
	float* pts = ctx->stage;
	float* res = ctx->stage + (size_t)count * 4;
	FX_HIP(hipMemcpyAsync(pts, points, in_bytes, hipMemcpyHostToDevice, s));
	FX_HIP(launch_sample_velocity(ctx->g, ctx->half, ctx->vel[0], pts, res, count, s));
	FX_HIP(hipMemcpyAsync(out, res, out_bytes, hipMemcpyDeviceToHost, s));
	FX_HIP(hipStreamSynchronize(s));
	return FX_OK;
}

// ---- the advection scheme (fx_maccormack.hip) ---------------------------------------------------------------
int fx_set_advection_scheme(fx_ctx* ctx, uint32_t scheme)
{
	if (const int rc = sim_guard(ctx)) return rc;
	if (scheme != FX_ADVECT_SEMI_LAGRANGIAN && scheme != FX_ADVECT_MACCORMACK) return FX_E_INVALID;
	DeviceGuard dg(ctx->device);
	if (scheme == FX_ADVECT_SEMI_LAGRANGIAN) {                                // the default: every launch is the plain one again, the scratch goes
		if (ctx->mc_vel) FX_HIP(hipFree(ctx->mc_vel));                        // (hipFree waits for the device: nothing reads the scratch any more)
		ctx->mc_vel = nullptr;
		if (ctx->mc_col) FX_HIP(hipFree(ctx->mc_col));
		ctx->mc_col = nullptr;
		ctx->adv_scheme = scheme;
		return FX_OK;
	}
	if (!ctx->mc_vel) {                                                       // the first successful switch: seven fp32 values per cell
		const size_t n = ctx->g.cells_owned();
		float *v = nullptr, *c = nullptr;
		if (hipMalloc((void**)&v, 3 * n * sizeof(float)) != hipSuccess || hipMalloc((void**)&c, 4 * n * sizeof(float)) != hipSuccess) {
			(void)hipGetLastError();
			if (v) (void)hipFree(v);
			return FX_E_NOMEM;
		}
		ctx->mc_vel = v; ctx->mc_col = c;
	}
	ctx->adv_scheme = scheme;
	return FX_OK;
}

int fx_get_advection_scheme(fx_ctx* ctx, uint32_t* scheme)
{
	if (!scheme) return FX_E_INVALID;
	if (const int rc = sim_guard(ctx, false)) return rc;                     // (slab ranks may ask: semi-Lagrangian there)
	*scheme = ctx->adv_scheme;
	return FX_OK;
}

// ---- the pressure solver (fx_multigrid.hip, fx_multigrid_plan.cpp) ---------------------------------------------
static void mg_release(fx_ctx* ctx)
{
	if (ctx->mg_mem) (void)hipFree(ctx->mg_mem);                              // (hipFree waits for the device: nothing reads the pyramid any more)
	ctx->mg_mem = nullptr;
	ctx->mg = MgPlan{};
	for (int l = 0; l < kMgMaxLevels; ++l) { ctx->mg_e[l][0] = ctx->mg_e[l][1] = ctx->mg_b[l] = nullptr; ctx->mg_cur[l] = 0; }
}

int fx_set_pressure_solver(fx_ctx* ctx, const fx_pressure_solver* solver)
{
	if (const int rc = sim_guard(ctx)) return rc;
	if (solver && solver->kind != FX_PRESSURE_JACOBI && solver->kind != FX_PRESSURE_MULTIGRID) return FX_E_INVALID;
	DeviceGuard dg(ctx->device);
	if (!solver || solver->kind == FX_PRESSURE_JACOBI) {                      // the default: every launch is the plain one again, the pyramid goes
		mg_release(ctx);
		ctx->solver = fx_pressure_solver{ FX_PRESSURE_JACOBI, 0u, 0u, 0u, 0u, 0u, 0u, 0.0f };
		return FX_OK;
	}
	const fx_pressure_solver& ps = *solver;
	if ((ps.flags & ~(uint32_t)FX_MG_NO_TAIL) || ps.cycles < 1 || ps.cycles > 64 || ps.pre_sweeps > 64 || ps.post_sweeps > 64 ||
		ps.coarse_sweeps < 1 || ps.coarse_sweeps > 256 || ps.max_levels > FX_MG_MAX_LEVELS || !std::isfinite(ps.omega) || !(ps.omega > 0.0f) || ps.omega > 1.0f)
		return FX_E_INVALID;
	if (ctx->desc.jacobi_mode == FX_JACOBI_FAITHFUL) return FX_E_INVALID;  // the per-cell freeze solve has no coarse levels
	if (ctx->obst_code || ctx->open_faces) return FX_E_STATE;               // their boundary rules have no coarse counterpart yet
	MgPlan plan;
	mg_plan(ctx->g, ps.max_levels, &plan);
	// the pyramid of the new plan is built beside the one in force, which stays in force if the allocation fails
	const size_t align = 64;                                                  // floats: every buffer starts on a 256-byte boundary
	size_t total = 0;
	for (int l = 1; l < plan.levels; ++l) total += 3 * ((plan.lv[l].cells() + align - 1) / align * align);
	float* mem = nullptr;
	if (total && hipMalloc((void**)&mem, total * sizeof(float)) != hipSuccess) { (void)hipGetLastError(); return FX_E_NOMEM; }
	if (mem && hipMemset(mem, 0, total * sizeof(float)) != hipSuccess) { (void)hipGetLastError(); (void)hipFree(mem); return FX_E_DEVICE; }
	mg_release(ctx);
	ctx->mg_mem = mem;
	ctx->mg = plan;
	for (int l = 1; l < plan.levels; ++l) {
		const size_t n = (plan.lv[l].cells() + align - 1) / align * align;
		ctx->mg_e[l][0] = mem; ctx->mg_e[l][1] = mem + n; ctx->mg_b[l] = mem + 2 * n;
		mem += 3 * n;
	}
	ctx->solver = ps;
	return FX_OK;
}

int fx_get_pressure_solver(fx_ctx* ctx, fx_pressure_solver* out)
{
	if (!out) return FX_E_INVALID;
	if (const int rc = sim_guard(ctx, false)) return rc;                     // (slab ranks may ask: Jacobi there)
	*out = ctx->solver;
	out->max_levels = ctx->solver.kind == FX_PRESSURE_MULTIGRID ? (uint32_t)ctx->mg.levels : 1u;
	return FX_OK;
}

int fx_pressure_solve(fx_ctx* ctx, void* stream)
{
	if (!ctx || ctx->nranks > 1) return FX_E_INVALID;
	if (ctx->desc.flags & FX_FLAG_RENDER_ONLY) return FX_E_STATE;
	std::vector<fx_ctx*> M{ ctx };
	return pressure_solve_all(ctx, M, pick_stream(ctx, stream));
}

int fx_download_pressure_level(fx_ctx* ctx, uint32_t level, int what, void* host, size_t bytes)
{
	if (!host || (what != 0 && what != 1)) return FX_E_INVALID;
	if (const int rc = sim_guard(ctx)) return rc;
	if (level == 0) return fx_download(ctx, what ? FX_FIELD_DIVERGENCE : FX_FIELD_PRESSURE, host, bytes);
	if (ctx->solver.kind != FX_PRESSURE_MULTIGRID || level >= (uint32_t)ctx->mg.levels) return FX_E_INVALID;
	if (bytes != ctx->mg.lv[level].cells() * sizeof(float)) return FX_E_INVALID;
	DeviceGuard dg(ctx->device);
	FX_HIP(hipDeviceSynchronize());
	FX_HIP(hipMemcpy(host, what ? ctx->mg_b[level] : ctx->mg_e[level][ctx->mg_cur[level]], bytes, hipMemcpyDeviceToHost));
	return FX_OK;
}

int fx_divergence(fx_ctx* ctx, void* stream)
{
	if (!ctx || ctx->nranks > 1) return FX_E_INVALID;
	if (ctx->desc.flags & FX_FLAG_RENDER_ONLY) return FX_E_STATE;
	return divergence_phase(ctx, pick_stream(ctx, stream));
}

int fx_jacobi(fx_ctx* ctx, void* stream, uint32_t iters)
{
	if (!ctx || !iters || ctx->nranks > 1) return FX_E_INVALID;
	if (ctx->desc.flags & FX_FLAG_RENDER_ONLY) return FX_E_STATE;
	std::vector<fx_ctx*> M{ ctx };
	return jacobi_all(ctx, M, pick_stream(ctx, stream), iters);
}

int fx_project(fx_ctx* ctx, void* stream)
{
	if (!ctx || ctx->nranks > 1) return FX_E_INVALID;
	if (!ctx->frame_valid || (ctx->desc.flags & FX_FLAG_RENDER_ONLY)) return FX_E_STATE;
	return project_phase(ctx, pick_stream(ctx, stream));
}

// ---- SH light probe -----------------------------------------------------------------------------------
int fx_sh_transform(fx_ctx* ctx, const float* cube, uint32_t n, float* out27)
{
	if (!ctx || !cube || !out27 || !n || n > 4096) return FX_E_INVALID;
	DeviceGuard dg(ctx->device);
	FX_HIP(hipDeviceSynchronize());
	const size_t cubeBytes = (size_t)6 * n * n * 3 * sizeof(float);
	int rc = ensure_stage(ctx, cubeBytes);
	if (rc) return rc;
	if (ctx->sh_scratch_n != n) {
		for (int i = 0; i < 4; ++i) {
			if (ctx->sh_scratch[i]) { FX_HIP(hipFree(ctx->sh_scratch[i])); ctx->sh_scratch[i] = nullptr; }
			FX_HIP(hipMalloc((void**)&ctx->sh_scratch[i], sh_scratch_floats((int)n, i) * sizeof(float)));
		}
		ctx->sh_scratch_n = n;
	}
	float* d_out = nullptr;
	FX_HIP(hipMalloc((void**)&d_out, 27 * sizeof(float)));
	FX_HIP(hipMemcpy(ctx->stage, cube, cubeBytes, hipMemcpyHostToDevice));
	hipError_t e = launch_sh_transform(ctx->stage, (int)n, ctx->sh_scratch[0], ctx->sh_scratch[1], ctx->sh_scratch[2],
		ctx->sh_scratch[3], d_out, ctx->stream);
	if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
	if (e == hipSuccess) e = hipMemcpy(out27, d_out, 27 * sizeof(float), hipMemcpyDeviceToHost);
	(void)hipFree(d_out);
	if (e != hipSuccess) { ctx->last_error = hipGetErrorString(e); return FX_E_DEVICE; }
	return FX_OK;
}

// ---- timing ---------------------------------------------------------------------------------------------
int fx_dds_cube_info(const void* dds, size_t bytes, uint32_t* size, uint32_t* mips)
{
	DdsCube d;
	if (!dds_cube_layout(dds, bytes, &d)) return FX_E_INVALID;
	if (size) *size = d.size;
	if (mips) *mips = d.mips;
	return FX_OK;
}

int fx_dds_decode_cube(fx_ctx* ctx, const void* dds, size_t bytes, uint32_t mip, float* out_cube, size_t out_floats)
{
	if (!ctx || !out_cube) return FX_E_INVALID;
	DdsCube d;
	if (!dds_cube_layout(dds, bytes, &d) || mip >= d.mips) return FX_E_INVALID;
	const size_t* fo = d.face_offset; const size_t* mo = d.mip_offset;
	const uint32_t n = std::max<uint32_t>(d.size >> mip, 1), nb = (n + 3) / 4;
	const size_t face_floats = (size_t)n * n * 3, face_blocks = (size_t)nb * nb * 16;
	if (out_floats != 6 * face_floats) return FX_E_INVALID;
	if (d.kind != DDS_BC6H_UF16) {                                          // uncompressed: a host-side format conversion
		for (int f = 0; f < 6; ++f) dds_linear_face_to_rgb(static_cast<const char*>(dds) + fo[f] + mo[mip], d.kind, n, out_cube + f * face_floats);
		return FX_OK;
	}
	DeviceGuard dg(ctx->device);
	const size_t float_bytes = (6 * face_floats * 4 + 15) & ~(size_t)15;     // the blocks are read as 16-byte words
	int rc = ensure_stage(ctx, float_bytes + 6 * face_blocks);
	if (rc) return rc;
	char* blocks_dev = reinterpret_cast<char*>(ctx->stage) + float_bytes;
	for (int f = 0; f < 6; ++f)
		FX_HIP(hipMemcpyAsync(blocks_dev + f * face_blocks, static_cast<const char*>(dds) + fo[f] + mo[mip], face_blocks, hipMemcpyHostToDevice, ctx->stream));
	for (int f = 0; f < 6; ++f)
		FX_HIP(launch_bc6h_decode(blocks_dev + f * face_blocks, (int)nb, (int)nb, (int)n, ctx->stage + f * face_floats, ctx->stream));
	FX_HIP(hipMemcpyAsync(out_cube, ctx->stage, 6 * face_floats * 4, hipMemcpyDeviceToHost, ctx->stream));
	FX_HIP(hipStreamSynchronize(ctx->stream));
	return FX_OK;
}

// ---- multi-GPU ---------------------------------------------------------------------------------------------
size_t fx_comm_id_bytes(void) { return rccl_id_bytes(); }

int fx_comm_get_unique_id(void* id_out, size_t bytes)
{
	if (!id_out) return FX_E_INVALID;
	std::string err;
	const int rc = rccl_get_unique_id(id_out, bytes, &err);
	if (rc) std::fprintf(stderr, "fluidx: %s\n", err.c_str());
	return rc;
}

static int check_slab_chain(fx_ctx* c, int rank, int nranks)
{
	if (nranks < 1 || rank < 0 || rank >= nranks) return FX_E_INVALID;
	if (c->group) return FX_E_STATE;
	if (nranks > 1 && c->g.nz == c->g.Zg) return FX_E_INVALID;     // a slab context is required
	if (rank == 0 && c->g.z0 != 0) return FX_E_INVALID;
	if (rank == nranks - 1 && c->g.z0 + c->g.nz != c->g.Zg) return FX_E_INVALID;
	return FX_OK;
}

// a lane: side streams + ordering events of one rank (fx_context.h); `compute` = the member's own stream in peer groups, else null
static int make_lane(fx_comm_group* g, int device, hipStream_t compute)
{
	fx_lane l{};
	l.device = device;
	l.compute = compute;
	DeviceGuard dg(device);
	// DEFAULT priority.  A high-priority side stream made every dependency between it and the compute stream cost about a
	// millisecond for the first group of a process (18 ms per step instead of 7.7, docs/LAB.md); the switch COMM_PRIORITY = 1
	// asks for the highest priority anyway (measurement).
	int lo = 0, hi = 0, prio = 0;
	const char* pe = FX_KNOB("COMM_PRIORITY");
	if (pe && pe[0] == '1' && hipDeviceGetStreamPriorityRange(&lo, &hi) == hipSuccess) prio = hi;
	bool ok = hipStreamCreateWithPriority(&l.comm, hipStreamNonBlocking, prio) == hipSuccess;
	ok = ok && hipStreamCreateWithFlags(&l.face, hipStreamNonBlocking) == hipSuccess;
	for (hipEvent_t* e : { &l.ev_ready, &l.ev_done, &l.ev_col_ready, &l.ev_col_done, &l.ev_int, &l.ev_face1, &l.x_ready, &l.x_done })
		ok = ok && hipEventCreateWithFlags(e, hipEventDisableTiming) == hipSuccess;
	g->lanes.push_back(l);                             // (pushed even when incomplete: the group's teardown frees what exists)
	return ok ? FX_OK : FX_E_DEVICE;
}

// buffers of the per-step record (fx_context.h); nrec = records the host copy holds (RCCL: every rank's; loop-back member: its own)
static int make_step_record(fx_ctx* ctx, int nrec, bool gathered)
{
	DeviceGuard dg(ctx->device);
	if (ctx->step_rec) return FX_OK;
	FX_HIP(hipMalloc((void**)&ctx->step_rec, 4 * sizeof(int)));
	FX_HIP(hipMemset(ctx->step_rec, 0, 4 * sizeof(int)));
	if (gathered) FX_HIP(hipMalloc((void**)&ctx->gath_dev, 4 * sizeof(int) * (size_t)nrec));
	FX_HIP(hipHostMalloc((void**)&ctx->rec_host, 4 * sizeof(int) * (size_t)nrec, hipHostMallocDefault));
	std::memset(ctx->rec_host, 0, 4 * sizeof(int) * (size_t)nrec);
	FX_HIP(hipEventCreateWithFlags(&ctx->rec_ev, hipEventDisableTiming));
	return FX_OK;
}

int fx_comm_init_rank(fx_ctx* ctx, const void* id, size_t bytes, int rank, int nranks)
{
	if (!ctx || !id) return FX_E_INVALID;
	int rc = check_slab_chain(ctx, rank, nranks);
	if (rc) return rc;
	Transport* t = make_rccl_transport(id, bytes, rank, nranks, ctx->device, &ctx->last_error);
	if (!t) { std::fprintf(stderr, "fluidx: %s\n", ctx->last_error.c_str()); return FX_E_COMM; }
	fx_comm_group* g = new fx_comm_group();
	g->members.push_back(ctx);
	g->transport = t;
	g->refs = 1;
	g->per_member = false; g->shared_stream = nullptr; g->broken = false;
	if ((rc = make_lane(g, ctx->device, nullptr))) { destroy_lanes(g); delete t; delete g; return rc; }
	if ((rc = t->min_over_ranks(ctx->g.nz, ctx->stream, &g->min_nz))) { destroy_lanes(g); delete t; delete g; return rc; }
	{	// every rank must run the same schedule: same grid, halos, sweep count, Jacobi mode and storage (min == max of a digest)
		const fx_desc& d = ctx->desc;
		uint32_t h = 2166136261u;
		// ... and the same schedule: what selects the exchange sequence (FX_FLAG_NO_OVERLAP / FX_OPT_OVERLAP, FX_OPT_JACOBI_ROUND,
		// FX_OPT_ADAPTIVE_HALO) is part of the digest; later changes go through fx_set_option, which checks them across the chain
		for (uint32_t v : { d.grid_x, d.grid_y, d.grid_z, d.halo_advect, d.halo_jacobi, d.jacobi_iters, d.jacobi_mode, d.storage, d.advect_address, (uint32_t)nranks,
				d.flags & (FX_FLAG_NO_OVERLAP | FX_FLAG_JACOBI_FUSE_MASK), (uint32_t)ctx->opt_overlap, (uint32_t)ctx->opt_round, (uint32_t)ctx->opt_adaptive })
			h = (h ^ v) * 16777619u;
		const int digest = (int)(h & 0x3FFFFFFFu);
		int lo = 0, hi = 0;
		if ((rc = t->min_over_ranks(digest, ctx->stream, &lo)) || (rc = t->min_over_ranks(-digest, ctx->stream, &hi))) { destroy_lanes(g); delete t; delete g; return rc; }
		if (lo != digest || -hi != digest) {
			ctx->last_error = "fx_comm_init_rank: the ranks were created with different descriptors";
			std::fprintf(stderr, "fluidx: %s\n", ctx->last_error.c_str());
			destroy_lanes(g); delete t; delete g;
			return FX_E_INVALID;
		}
	}
	if (!ctx->step_rec && (rc = make_step_record(ctx, nranks, true))) { destroy_lanes(g); delete t; delete g; return rc; }   // (kept from a refused earlier attempt)
	{	// the slabs must tile the grid in rank order: rank 0 starts at plane 0, the last ends at Zg (check_slab_chain), and every
		// slab starts where its lower neighbour ends -- gaps or overlaps between middle slabs would exchange the wrong planes
		DeviceGuard dg(ctx->device);
		const int mine[4] = { ctx->g.z0, ctx->g.nz, 0, 0 };
		bool ok = hipMemcpy(ctx->step_rec, mine, sizeof mine, hipMemcpyHostToDevice) == hipSuccess &&
			t->allgather(ctx->step_rec, 4, ctx->gath_dev, ctx->stream) == FX_OK &&
			hipMemcpyAsync(ctx->rec_host, ctx->gath_dev, 4 * sizeof(int) * (size_t)nranks, hipMemcpyDeviceToHost, ctx->stream) == hipSuccess &&
			hipStreamSynchronize(ctx->stream) == hipSuccess;
		bool tiles = ok;
		for (int r = 0; ok && r + 1 < nranks; ++r) tiles = tiles && ctx->rec_host[4 * r] + ctx->rec_host[4 * r + 1] == ctx->rec_host[4 * (r + 1)];
		if (ok) ok = hipMemset(ctx->step_rec, 0, 4 * sizeof(int)) == hipSuccess;
		if (!ok || !tiles) {
			ctx->last_error = ok ? "fx_comm_init_rank: the slabs of the ranks do not tile the grid in rank order" : "fx_comm_init_rank: exchanging the slab ranges failed";
			std::fprintf(stderr, "fluidx: %s\n", ctx->last_error.c_str());
			destroy_lanes(g); delete t; delete g;
			return ok ? FX_E_INVALID : FX_E_COMM;
		}
	}
	ctx->group = g; ctx->rank = rank; ctx->nranks = nranks;
	return FX_OK;
}

int fx_comm_gather_color(fx_ctx* ctx, void* stream, fx_ctx* full, int root, const uint32_t* slab_z0, const uint32_t* slab_nz)
{
	if (!ctx || !ctx->group || root < 0 || root >= ctx->nranks) return FX_E_INVALID;
	if (group_broken(ctx)) return FX_E_STATE;
	if (!is_driver(ctx)) return FX_OK;
	const bool local = ctx->group->transport->is_local();
	const bool am_root = local || ctx->rank == root;
	if (am_root) {
		if (!full || full->g.X != ctx->g.X || full->g.Y != ctx->g.Y || full->g.Zg != ctx->g.Zg || full->g.nz != full->g.Zg ||
			full->half != ctx->half) return FX_E_INVALID;
		if (!local && full->device != ctx->device) return FX_E_INVALID;
		if (local && full->device != ctx->group->members[(size_t)root]->device) return FX_E_INVALID;   // the whole-grid context lives where the root does
	}
	if (!local && (!slab_z0 || !slab_nz)) return FX_E_INVALID;
	const size_t plane_bytes = ctx->g.plane() * 4 * elem_size(ctx);
	std::vector<GatherPart> parts((size_t)ctx->nranks);
	for (int r = 0; r < ctx->nranks; ++r) {
		const fx_ctx* m = local ? ctx->group->members[r] : (r == ctx->rank ? ctx : nullptr);
		const uint32_t z0 = local ? (uint32_t)m->g.z0 : slab_z0[r], nz = local ? (uint32_t)m->g.nz : slab_nz[r];
		if (z0 > (uint32_t)ctx->g.Zg || nz > (uint32_t)ctx->g.Zg - z0) return FX_E_INVALID;   // (z0 + nz would wrap for absurd input)
		if (!local && r == ctx->rank && (z0 != (uint32_t)ctx->g.z0 || nz != (uint32_t)ctx->g.nz)) return FX_E_INVALID;   // what this rank sends is its own slab
		parts[r].rank = r;
		parts[r].bytes = (size_t)nz * plane_bytes;
		parts[r].src = m ? (const char*)m->col[m->frame_parity] + (size_t)m->g.H * plane_bytes : nullptr;
		parts[r].dst = am_root ? (char*)full->col[full->frame_parity] + (size_t)z0 * plane_bytes : nullptr;
		if (am_root) full->accel_alpha_of = nullptr;
	}
	DeviceGuard dg(ctx->device);
	hipStream_t s = pick_stream(ctx, stream);
	if (ctx->halo_fault) return FX_E_HALO;             // a colour field that is known to be off is not gathered into a picture
	std::vector<hipStream_t> streams;                  // one; a peer group: every member's own, the copies ordered on the root's
	if (ctx->group->per_member) for (fx_ctx* m : ctx->group->members) streams.push_back(m->stream);
	else streams.push_back(s);
	hipStream_t done_on = ctx->group->per_member ? streams[(size_t)root] : s;
	ScopedMark mk(ctx, s, MK_EXCH);
	int rc = ctx->group->transport->gather(ctx->group, parts, root, streams);
	if (rc) return rc;
	if (am_root && full->stream != done_on) {          // the render context's own stream must see the planes
		fx_lane& L = ctx->group->per_member ? ctx->group->lanes[(size_t)root] : ctx->group->lanes[0];
		DeviceGuard dgr(L.device);
		FX_HIP(hipEventRecord(L.ev_done, done_on));
		DeviceGuard dgf(full->device);
		FX_HIP(hipStreamWaitEvent(full->stream, L.ev_done, 0));
	}
	return FX_OK;
}

// the checks both kinds of in-process group share; one_device: every member must live on the first one's device
static int check_local_members(fx_ctx** ctxs, int nranks, bool one_device)
{
	if (!ctxs || nranks < 1) return FX_E_INVALID;
	int zexp = 0;
	for (int r = 0; r < nranks; ++r) {
		if (!ctxs[r]) return FX_E_INVALID;
		int rc = check_slab_chain(ctxs[r], r, nranks);
		if (rc) return rc;
		if (ctxs[r]->g.z0 != zexp || (one_device && ctxs[r]->device != ctxs[0]->device)) return FX_E_INVALID;   // contiguous chain
		// every member must describe the same run (the RCCL path checks a digest of the same fields across the ranks): members
		// of different grids would exchange planes of different sizes
		const fx_desc &a = ctxs[r]->desc, &b = ctxs[0]->desc;
		if (a.grid_x != b.grid_x || a.grid_y != b.grid_y || a.grid_z != b.grid_z || a.halo_advect != b.halo_advect ||
			a.halo_jacobi != b.halo_jacobi || a.jacobi_iters != b.jacobi_iters || a.jacobi_mode != b.jacobi_mode ||
			a.storage != b.storage || a.advect_address != b.advect_address)
			return FX_E_INVALID;
		for (int q = 0; q < r; ++q) if (ctxs[q] == ctxs[r]) return FX_E_INVALID;
		zexp += ctxs[r]->g.nz;
	}
	return FX_OK;
}

static int init_in_process_group(fx_ctx** ctxs, int nranks, bool peer)
{
	int rc = check_local_members(ctxs, nranks, !peer);
	if (rc) return rc;
	if (peer) {
		// a receiver copies out of its neighbour's memory: across devices that needs peer access (one process owns them all: no IPC
		// handles, which this pool's driver does not give out between processes)
		for (int r = 0; r + 1 < nranks; ++r) {
			const int a = ctxs[r]->device, b = ctxs[r + 1]->device;
			if (a == b) continue;
			int ab = 0, ba = 0;
			if (hipDeviceCanAccessPeer(&ab, a, b) != hipSuccess || hipDeviceCanAccessPeer(&ba, b, a) != hipSuccess || !ab || !ba) {
				ctxs[0]->last_error = "fx_comm_init_peer: two neighbouring slabs live on devices without peer access";
				return FX_E_DEVICE;
			}
			for (int k = 0; k < 2; ++k) {
				DeviceGuard dg(k ? b : a);
				const hipError_t e = hipDeviceEnablePeerAccess(k ? a : b, 0);
				if (e != hipSuccess && e != hipErrorPeerAccessAlreadyEnabled) { (void)hipGetLastError(); return FX_E_DEVICE; }
				(void)hipGetLastError();
			}
		}
	}
	for (int r = 0; r < nranks; ++r)
		if (!ctxs[r]->step_rec) { if ((rc = make_step_record(ctxs[r], 1, false))) return rc; }
	fx_comm_group* g = new fx_comm_group();
	g->transport = make_local_transport();
	g->refs = nranks;
	g->per_member = peer; g->shared_stream = nullptr; g->broken = false;
	for (int r = 0; r < (peer ? nranks : 1); ++r)
		if ((rc = make_lane(g, ctxs[r]->device, peer ? ctxs[r]->stream : nullptr))) { destroy_lanes(g); delete g->transport; delete g; return rc; }
	g->min_nz = ctxs[0]->g.nz;
	for (int r = 1; r < nranks; ++r) g->min_nz = std::min(g->min_nz, ctxs[r]->g.nz);
	for (int r = 0; r < nranks; ++r) {
		g->members.push_back(ctxs[r]);
		ctxs[r]->group = g; ctxs[r]->rank = r; ctxs[r]->nranks = nranks;
		if (peer) continue;                                // every member keeps (and owns) its stream
		// one stream for the whole shared-stream group: phases of different members are ordered by it.  The group owns it, so
		// that the members can be destroyed in any order.
		if (r > 0) {
			if (ctxs[r]->owns_stream) (void)hipStreamDestroy(ctxs[r]->stream);
			ctxs[r]->stream = ctxs[0]->stream;
		}
		ctxs[r]->owns_stream = false;
		g->shared_stream = ctxs[0]->stream;
	}
	return FX_OK;
}

int fx_comm_init_local(fx_ctx** ctxs, int nranks) { return init_in_process_group(ctxs, nranks, false); }
int fx_comm_init_peer(fx_ctx** ctxs, int nranks) { return init_in_process_group(ctxs, nranks, true); }

}  // extern "C"

