// orc_depth_render.cpp -- TEST INFRASTRUCTURE: the depth-aware view marches of the CPU reference (the reference's _HAS_DEPTH_MAP_ shader
// variants), never linked into the product.  It compiles oracle/orc_render.cpp into this translation unit and reuses its pinned
// march(), compute_ray_origin(), cube_texel_to_local() and frame arithmetic unchanged; what it adds are the restated depth functions:
//   GetClipPos (direct)   PSRayCast.hlsl:30-39        the pixel's own depth texel at its screen-quad position
//   GetClipPos (cube)     CSRayMarch.hlsl:80-92       project o + 0.01 d with the forward WorldViewProj, point-sample the depth
//   GetTMax               RayMarch.hlsli:99-115       unproject through WorldViewProjI, max over (p - o) / d; FLT_MAX at z >= 1
// (paths relative to FluidX12/Content/Shaders/ of the reference).  No shipped binary of these variants exists, so the arithmetic cannot
// be pinned to DXBC; it follows the conventions of the pinned shaders (mad = fmaf, dp4 = mul then fma chain).  The point sampler of
// CSRayMarch.hlsl:89 is never created by the reference: nearest texel, clamped to the edge, NaN -> texel 0.
// Anchor: with a depth buffer of 1.0 everywhere, every function below equals its oracle counterpart byte for byte
// (tests/test_depth_ref.py).
#include "../../oracle/orc_render.cpp"

namespace {

// GetTMax (RayMarch.hlsli:99-110)
float get_tmax(const float* wvp_i, float x, float y, float z, const float o[3], const float d[3])
{
	if (z >= 1.0f) return 3.40282347e+38f;                                          // :102
	float h[4];
	for (int r = 0; r < 4; ++r)                                                    // :104
		h[r] = std::fmaf(1.0f, wvp_i[4 * r + 3], std::fmaf(z, wvp_i[4 * r + 2], std::fmaf(y, wvp_i[4 * r + 1], x * wvp_i[4 * r + 0])));
	float t[3];
	for (int a = 0; a < 3; ++a) t[a] = (h[a] / h[3] + -o[a]) / d[a];               // :105-107
	return std::fmax(std::fmax(t[0], t[1]), t[2]);                                 // :109
}

int depth_texel(float u, int n)
{
	const float f = u * (float)n;
	return !(f >= 0.0f) ? 0 : f >= (float)n ? n - 1 : (int)f;
}

}  // namespace

extern "C" {

// orc_raycast_direct + PSRayCast.hlsl:52-56,119-120: depth float[H][W]
void orcd_raycast_direct(const float* color, const float* lightmap, int X, int Y, int Z, const orc_frame* fc,
	const float* wvp_i, int W, int H, uint32_t numSamples, uint32_t numLightSamples, int hasSH, int separate,
	const float* depth, float* out_rgba, uint8_t* covered)
{
	const Vol v{ color, lightmap, { X, Y, Z } };
	float eye[3];
	for (int a = 0; a < 3; ++a) {
		const float* r = fc->world_i + 4 * a;
		eye[a] = std::fmaf(r[3], 1.0f, std::fmaf(fc->eye_pt[2], r[2], std::fmaf(fc->eye_pt[1], r[1], fc->eye_pt[0] * r[0])));
	}
	float ldir[3];
	light_dir_local(ldir, fc);
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
			// GetClipPos (PSRayCast.hlsl:30-39): xy = uv * 2 - 1, y flipped; z = the pixel's depth texel
			const float tMax = get_tmax(wvp_i, q[0], q[1], depth[(size_t)py * W + px], o, d);   // :55
			float scatter[4];
			march(scatter, v, fc, o, d, tMax, ldir, lightColor, ambient, stepScale, lightStep, numSamples, numLightSamples, hasSH, separate);
			for (int a = 0; a < 3; ++a) out[a] = scatter[a] * 0.159154937f;
			out[3] = scatter[3];
			covered[(size_t)py * W + px] = 1;
		}
}

// orc_raymarch_view + CSRayMarch.hlsl:121-126: depth float[H][W]; wvp = the forward WorldViewProj as its four constant-buffer rows,
// wvp_i the inverse; cube_depth float[6][size][size] receives each texel's depth where a ray was cast (other texels are left alone)
void orcd_raymarch_view(const float* color, const float* lightmap, int X, int Y, int Z, const orc_frame* fc,
	int size, uint32_t mask, uint32_t numSamples, uint32_t numLightSamples, int hasSH, int separate,
	const float* depth, int W, int H, const float* wvp, const float* wvp_i, float* cube_f32, uint8_t* cube_u8, float* cube_depth)
{
	const Vol v{ color, lightmap, { X, Y, Z } };
	float eye[3];
	for (int a = 0; a < 3; ++a) {
		const float* r = fc->world_i + 4 * a;
		eye[a] = std::fmaf(r[3], 1.0f, std::fmaf(fc->eye_pt[2], r[2], std::fmaf(fc->eye_pt[1], r[1], fc->eye_pt[0] * r[0])));
	}
	float ldir[3];
	light_dir_local(ldir, fc);
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
				float tMax = std::fmax(tq[2], std::fmax(tq[1], tq[0]));
				// GetClipPos (CSRayMarch.hlsl:80-92)
				float p[3], h[4];
				for (int a = 0; a < 3; ++a) p[a] = std::fmaf(d[a], 0.01f, o[a]);                 // :82
				for (int r = 0; r < 4; ++r)                                                     // :83
					h[r] = std::fmaf(1.0f, wvp[4 * r + 3], std::fmaf(p[2], wvp[4 * r + 2], std::fmaf(p[1], wvp[4 * r + 1], p[0] * wvp[4 * r + 0])));
				const float cx = h[0] / h[3], cy = h[1] / h[3];                                   // :85
				const float u = std::fmaf(cx, 0.5f, 0.5f), vv = -std::fmaf(cy, 0.5f, 0.5f) + 1.0f;  // :86-87
				const float z = depth[(size_t)depth_texel(vv, H) * W + depth_texel(u, W)];       // :89
				cube_depth[((size_t)face * size + y) * size + x] = z;                            // :124
				tMax = std::fmin(get_tmax(wvp_i, cx, cy, z, o, d), tMax);                       // :125
				float scatter[4];
				march(scatter, v, fc, o, d, tMax, ldir, lightColor, ambient, stepScale, lightStep, numSamples, numLightSamples, hasSH, separate);
				const size_t o4 = (((size_t)face * size + y) * size + x) * 4;
				for (int a = 0; a < 3; ++a) scatter[a] *= 0.159154937f;
				for (int a = 0; a < 4; ++a) {
					if (cube_f32) cube_f32[o4 + a] = scatter[a];
					if (cube_u8) cube_u8[o4 + a] = to_unorm8(scatter[a]);
				}
			}
		}
}

}  // extern "C"
