// orc_point_light.cpp -- TEST INFRASTRUCTURE: the settable scene light of the CPU reference (fx_set_light; the reference's _POINT_LIGHT_
// shader variants), never linked into the product.  It compiles oracle/orc_render.cpp into this translation unit and reuses its pinned
// helpers unchanged (make_taps, sample_chan, step_factor, gi_term, compute_ray_origin, cube_texel_to_local, store_light, normalize3, ...);
// what it restates, each with a `kind` argument (0 directional, 1 point), are the loops that use the light:
//   the light volume      CSRayMarchL.hlsl:15-80, with :49-50     rayDir = normalize(localSpaceLightPt - rayOrigin)
//   the view march        CSRayMarch.hlsl:140-190, with :134,165  lightDir = normalize(localSpaceLightPt - pos)
//   the direct march      PSRayCast.hlsl:72-122, with :64,95
//   CastLightRay          RayMarch.hlsli:215-247
// (paths relative to FluidX12/Content/Shaders/ of the reference).  No shipped binary of the point-light variants exists, so their
// arithmetic cannot be pinned to DXBC; it follows the conventions of the pinned shaders (mul(float4(p, 1), M) = mul then fma chain as
// for the eye point, normalize = v * rsq(dot(v, v)), dot = mul then fma chain).
// Two deliberate additions to the variant text:
//   A  a ray to a point light ends at the light: a sample is taken only while t < |localSpaceLightPt - origin| (the variant marches
//      on through the light, so that smoke behind a lamp would shadow what is in front of it).  orcl_set_end_rule(0) switches the
//      rule off -- the variant as written -- for the test that shows what the rule is for.
//   B  a light vector of length zero (the light sits on the ray's origin) or not finite casts no ray: shadow stays 1.
//      orcl_zero_vectors() counts how often that happened.
// Anchor: with kind = 0 every function below equals its oracle counterpart byte for byte (tests/test_light_ref.py).
#include "../../oracle/orc_render.cpp"
#include <atomic>

namespace {

enum { LIGHT_DIRECTIONAL = 0, LIGHT_POINT = 1 };

std::atomic<int> g_end_rule{ 1 };
std::atomic<long long> g_zero_vectors{ 0 };

// what the loops carry for the light: the unit direction (directional) or the light's place in the volume's space (point)
void light_source_local(float out[3], const orc_frame* fc, int kind)
{
	if (kind != LIGHT_POINT) { light_dir_local(out, fc); return; }                 // mul(g_lightPt, (float3x3)g_worldI), normalised
	for (int a = 0; a < 3; ++a) {                                                  // mul(float4(g_lightPt, 1), g_worldI)  (dp4)
		const float* r = fc->world_i + 4 * a;
		out[a] = std::fmaf(r[3], 1.0f, std::fmaf(fc->light_pt[2], r[2], std::fmaf(fc->light_pt[1], r[1], fc->light_pt[0] * r[0])));
	}
}

// the light ray of `origin`: direction and the parameter at which it ends; false = no ray is cast (addition B)
bool light_ray(float dir[3], float& tEnd, const float src[3], const float origin[3], int kind)
{
	if (kind != LIGHT_POINT) {
		for (int a = 0; a < 3; ++a) dir[a] = src[a];
		tEnd = 3.40282347e+38f;
		return true;
	}
	float v[3];
	for (int a = 0; a < 3; ++a) v[a] = src[a] - origin[a];
	const float l2 = dp3(v, v);
	if (!(l2 > 0.0f && l2 <= 3.40282347e+38f)) { ++g_zero_vectors; return false; }
	const float r = 1.0f / std::sqrt(l2);                                          // normalize = v * rsq(dot(v, v))
	for (int a = 0; a < 3; ++a) dir[a] = v[a] * r;
	tEnd = std::sqrt(l2);
	return true;
}

// CastLightRay (RayMarch.hlsli:215-247) as oracle/orc_render.cpp restates it, + addition A
void cast_light_ray_k(float& transm, const Vol& v, const float origin[3], const float dir[3], float stepScale, uint32_t numSamples,
	int kind, float tEnd)
{
	const bool ends = kind == LIGHT_POINT && g_end_rule.load(std::memory_order_relaxed) != 0;
	float t = stepScale, prevDensity = 0.0f;
	for (uint32_t i = 0; i < numSamples; ++i) {
		if (ends && !(t < tEnd)) break;                                            // addition A
		float pos[3], uvw[3];
		for (int a = 0; a < 3; ++a) pos[a] = std::fmaf(dir[a], t, origin[a]);
		if (outside(pos)) break;
		for (int a = 0; a < 3; ++a) uvw[a] = std::fmaf(pos[a], 0.5f, 0.5f);
		const Taps tp = make_taps(uvw, v.dims, ADDR_CLAMP);
		const float density = sample_chan(v.color, 4, 3, v.dims, tp);
		const float nt = std::fmaf(-density, 0.800000012f, 1.0f) * transm;
		if (nt < 0.00999999978f) { transm = nt; break; }
		const float fac = step_factor(-prevDensity + density, transm, density);
		t = std::fmaf(stepScale, fac, t);
		transm = nt;
		prevDensity = density;
	}
}

// the shadow term of a point of the volume
float shadow_at(const Vol& v, const float pos[3], const float src[3], float stepScale, uint32_t numSamples, int kind)
{
	float shadow = 1.0f, dir[3], tEnd;
	if (light_ray(dir, tEnd, src, pos, kind)) cast_light_ray_k(shadow, v, pos, dir, stepScale, numSamples, kind, tEnd);
	return shadow;
}

// the march of one view ray (CSRayMarch.hlsl:140-190 == PSRayCast.hlsl:72-122) as oracle/orc_render.cpp restates it; src = the
// light's direction or place (light_source_local)
void march_k(float scatter[4], const Vol& v, const orc_frame* fc, const float o[3], const float d[3], float tMax,
	const float src[3], const float lightColor[3], const float ambient[3], float stepScale, float lightStep,
	uint32_t numSamples, uint32_t numLightSamples, int hasSH, int separate, int kind)
{
	scatter[0] = scatter[1] = scatter[2] = scatter[3] = 0.0f;
	float t = 0.0f, prevDensity = 0.0f;
	for (uint32_t i = 0; i < numSamples; ++i) {
		float pos[3], uvw[3];
		for (int a = 0; a < 3; ++a) pos[a] = std::fmaf(d[a], t, o[a]);
		if (outside(pos)) break;
		for (int a = 0; a < 3; ++a) uvw[a] = std::fmaf(pos[a], 0.5f, 0.5f);
		const Taps tp = make_taps(uvw, v.dims, ADDR_CLAMP);
		float c[4];
		for (int a = 0; a < 4; ++a) c[a] = sample_chan(v.color, 4, a, v.dims, tp);
		float newStep = stepScale;
		if (0.00999999978f < c[3]) {
			float light[3];
			if (separate) {
				for (int a = 0; a < 3; ++a) light[a] = sample_chan(v.light, 3, a, v.dims, tp);
			} else {
				float ao = 1.0f, irr[3] = { 0, 0, 0 };
				const float shadow = shadow_at(v, pos, src, lightStep, numLightSamples, kind);   // CSRayMarch.hlsl:165 / PSRayCast.hlsl:95
				if (hasSH) gi_term(irr, ao, v, fc, pos, uvw, lightStep, numLightSamples);
				for (int a = 0; a < 3; ++a) {
					const float amb = hasSH ? ao * irr[a] : ambient[a];
					light[a] = std::fmaf(lightColor[a], shadow, amb);
				}
			}
			const float transm = -scatter[3] + 1.0f;
			newStep = step_factor(-prevDensity + c[3], transm, c[3]) * stepScale;
			for (int a = 0; a < 3; ++a)
				scatter[a] = std::fmaf(transm * (light[a] * c[a]), 0.800000012f, scatter[a]);
			scatter[3] = std::fmaf(0.800000012f * c[3], transm, scatter[3]);
			if (transm < 0.00999999978f) break;
			prevDensity = c[3];
		}
		t = t + newStep;
		if (tMax < t) break;
	}
}

}  // namespace

extern "C" {

void orcl_set_end_rule(int on) { g_end_rule.store(on ? 1 : 0); }
long long orcl_zero_vectors(void) { return g_zero_vectors.load(); }
void orcl_reset_zero_vectors(void) { g_zero_vectors.store(0); }

// orc_raymarch_light with a light of `kind`
void orcl_raymarch_light(const float* color, float* lightmap, int X, int Y, int Z, const orc_frame* fc,
	uint32_t numSamples, int hasSH, int light_fmt, int kind)
{
	const Vol v{ color, nullptr, { X, Y, Z } };
	const float fdims[3] = { (float)X, (float)Y, (float)Z };
	float src[3];
	light_source_local(src, fc, kind);
	float lightColor[3], ambient[3];
	for (int a = 0; a < 3; ++a) { lightColor[a] = fc->light_color[3] * fc->light_color[a]; ambient[a] = fc->ambient[3] * fc->ambient[a]; }
	const float stepScale = 3.46410155f / (float)numSamples;

#pragma omp parallel for schedule(dynamic, 1) collapse(2)
	for (int z = 0; z < Z; ++z)
		for (int y = 0; y < Y; ++y)
			for (int x = 0; x < X; ++x) {
				const int cell[3] = { x, y, z };
				float o[3], uvw[3];
				for (int a = 0; a < 3; ++a) {
					o[a] = std::fmaf(((float)cell[a] + 0.5f) / fdims[a], 2.0f, -1.0f);
					uvw[a] = std::fmaf(o[a], 0.5f, 0.5f);
				}
				const Taps tp = make_taps(uvw, v.dims, ADDR_CLAMP);
				const float density = sample_chan(color, 4, 3, v.dims, tp);
				float shadow = 1.0f, ao = 1.0f, irr[3] = { 0.0f, 0.0f, 0.0f };
				if (density >= 0.00999999978f) {
					shadow = shadow_at(v, o, src, stepScale, numSamples, kind);                 // CSRayMarchL.hlsl:49-55
					if (hasSH) gi_term(irr, ao, v, fc, o, uvw, stepScale, numSamples);
				}
				float* out = lightmap + (((size_t)z * Y + y) * X + x) * 3;
				for (int a = 0; a < 3; ++a) {
					const float amb = hasSH ? ao * irr[a] : ambient[a];
					out[a] = store_light(std::fmaf(shadow, lightColor[a], amb), light_fmt, a);
				}
			}
}

// orc_raymarch_view with a light of `kind`
void orcl_raymarch_view(const float* color, const float* lightmap, int X, int Y, int Z, const orc_frame* fc,
	int size, uint32_t mask, uint32_t numSamples, uint32_t numLightSamples, int hasSH, int separate, int kind,
	float* cube_f32, uint8_t* cube_u8)
{
	const Vol v{ color, lightmap, { X, Y, Z } };
	float eye[3];
	for (int a = 0; a < 3; ++a) {
		const float* r = fc->world_i + 4 * a;
		eye[a] = std::fmaf(r[3], 1.0f, std::fmaf(fc->eye_pt[2], r[2], std::fmaf(fc->eye_pt[1], r[1], fc->eye_pt[0] * r[0])));
	}
	float src[3];
	light_source_local(src, fc, kind);
	float lightColor[3], ambient[3];
	for (int a = 0; a < 3; ++a) { lightColor[a] = fc->light_color[3] * fc->light_color[a]; ambient[a] = fc->ambient[3] * fc->ambient[a]; }
	const float stepScale = 3.46410155f / (float)numSamples;
	const float lightStep = 3.46410155f / (float)numLightSamples;

#pragma omp parallel for schedule(dynamic, 1) collapse(2)
	for (int face = 0; face < 6; ++face)
		for (int y = 0; y < size; ++y) {
			if (!(mask >> face & 1u)) continue;
			for (int x = 0; x < size; ++x) {
				float target[3], o[3] = { eye[0], eye[1], eye[2] }, d[3];
				cube_texel_to_local(target, x, y, face, size);
				for (int a = 0; a < 3; ++a) d[a] = -o[a] + target[a];
				normalize3(d);
				if (!compute_ray_origin(o, d)) continue;
				float tq[3];
				for (int a = 0; a < 3; ++a) tq[a] = (target[a] + -o[a]) / d[a];
				const float tMax = std::fmax(tq[2], std::fmax(tq[1], tq[0]));
				float scatter[4];
				march_k(scatter, v, fc, o, d, tMax, src, lightColor, ambient, stepScale, lightStep, numSamples, numLightSamples, hasSH, separate, kind);
				const size_t o4 = (((size_t)face * size + y) * size + x) * 4;
				for (int a = 0; a < 3; ++a) scatter[a] *= 0.159154937f;
				for (int a = 0; a < 4; ++a) {
					if (cube_f32) cube_f32[o4 + a] = scatter[a];
					if (cube_u8) cube_u8[o4 + a] = to_unorm8(scatter[a]);
				}
			}
		}
}

// orc_raycast_direct with a light of `kind`
void orcl_raycast_direct(const float* color, const float* lightmap, int X, int Y, int Z, const orc_frame* fc,
	const float* wvp_i, int W, int H, uint32_t numSamples, uint32_t numLightSamples, int hasSH, int separate, int kind,
	float* out_rgba, uint8_t* covered)
{
	const Vol v{ color, lightmap, { X, Y, Z } };
	float eye[3];
	for (int a = 0; a < 3; ++a) {
		const float* r = fc->world_i + 4 * a;
		eye[a] = std::fmaf(r[3], 1.0f, std::fmaf(fc->eye_pt[2], r[2], std::fmaf(fc->eye_pt[1], r[1], fc->eye_pt[0] * r[0])));
	}
	float src[3];
	light_source_local(src, fc, kind);
	float lightColor[3], ambient[3];
	for (int a = 0; a < 3; ++a) { lightColor[a] = fc->light_color[3] * fc->light_color[a]; ambient[a] = fc->ambient[3] * fc->ambient[a]; }
	const float stepScale = 3.46410155f / (float)numSamples;
	const float lightStep = 3.46410155f / (float)numLightSamples;
#pragma omp parallel for schedule(dynamic, 1)
	for (int py = 0; py < H; ++py)
		for (int px = 0; px < W; ++px) {
			float* out = out_rgba + ((size_t)py * W + px) * 4;
			out[0] = out[1] = out[2] = out[3] = 0.0f;
			covered[(size_t)py * W + px] = 0;
			const float u = ((float)px + 0.5f) / (float)W, vv = ((float)py + 0.5f) / (float)H;
			const float q[3] = { std::fmaf(u, 2.0f, -1.0f), std::fmaf(vv, -2.0f, 1.0f), 1.0f };
			float h[4];
			for (int r = 0; r < 4; ++r) {
				const float col[3] = { wvp_i[4 * r + 0], wvp_i[4 * r + 1], wvp_i[4 * r + 3] };
				h[r] = dp3(q, col);
			}
			float o[3] = { h[0] / h[3], h[1] / h[3], h[2] / h[3] }, d[3];
			for (int a = 0; a < 3; ++a) d[a] = o[a] + -eye[a];
			normalize3(d);
			if (!compute_ray_origin(o, d)) continue;
			float scatter[4];
			march_k(scatter, v, fc, o, d, 3.40282347e+38f, src, lightColor, ambient, stepScale, lightStep, numSamples,
				numLightSamples, hasSH, separate, kind);
			for (int a = 0; a < 3; ++a) out[a] = scatter[a] * 0.159154937f;
			out[3] = scatter[3];
			covered[(size_t)py * W + px] = 1;
		}
}

}  // extern "C"
