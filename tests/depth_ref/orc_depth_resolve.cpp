// orc_depth_resolve.cpp -- TEST INFRASTRUCTURE: the depth-aware cube resolve of the CPU reference (PSCube.hlsli:82-113 under
// _HAS_DEPTH_MAP_), never linked into the product.  It compiles oracle/orc_resolve.cpp into this translation unit and reuses its pinned
// footprint(), face tables and frame arithmetic; it adds the restated depth pieces:
//   UnprojectZ      PSCube.hlsli:31-36     view-space z of a D3D depth: zn zf / (d (zn - zf) + zf)
//   CubeCast        PSCube.hlsli:82-113    cube-depth taps at the colour's footprint (same across-edge / missing-corner rules),
//                                          w_i = max(1 - 0.5 |z_pixel - z_i|, 0) wb_i, result = sum(w_i s_i) / sum(w_i), fallback when
//                                          the sum is not positive
// The weights multiply the plain CubeCast's wb in an order that reduces to the oracle's exactly when every depth weight is 1 (the
// anchor: a far-plane depth buffer reproduces orc_resolve_cube byte for byte).
#include "../../oracle/orc_resolve.cpp"

namespace {

inline float unproject_z(float z, float zn, float zf) { return (zn * zf) / std::fmaf(z, zn - zf, zf); }   // :33-35

// the cube-depth texels of the footprint of direction d, gather order as footprint()
void depth_footprint(const float* cd, int N, const float d[3], float z[4])
{
	const int f = major_face(d);
	float sc, tc;
	face_coords(d, f, sc, tc);
	const float ma = std::fabs(d[f >> 1]);
	const float tu = std::fmaf(0.5f * (sc / ma) + 0.5f, (float)N, -0.5f);
	const float tv = std::fmaf(0.5f * (tc / ma) + 0.5f, (float)N, -0.5f);
	const int i0 = (int)std::floor(tu), j0 = (int)std::floor(tv);
	const int ii[4] = { i0, i0 + 1, i0 + 1, i0 }, jj[4] = { j0 + 1, j0 + 1, j0, j0 };
	int missing = -1;
	for (int k = 0; k < 4; ++k) {
		const bool oi = ii[k] < 0 || ii[k] >= N, oj = jj[k] < 0 || jj[k] >= N;
		if (oi && oj) { missing = k; continue; }
		int g = f, i2 = ii[k], j2 = jj[k];
		if (oi || oj) {                                     // texel_across_edge's index rule
			const float se = ii[k] < 0 ? -1.0f : ii[k] >= N ? 1.0f : texel_centre(ii[k], N);
			const float te = jj[k] < 0 ? -1.0f : jj[k] >= N ? 1.0f : texel_centre(jj[k], N);
			float P[3];
			face_point(P, f, se, te);
			for (int a = 0; a < 3; ++a)
				if (a != (f >> 1) && std::fabs(P[a]) == 1.0f) g = 2 * a + (P[a] < 0.0f ? 1 : 0);
			float s2, t2;
			face_coords(P, g, s2, t2);
			i2 = std::min(std::max((int)std::floor((0.5f * s2 + 0.5f) * (float)N), 0), N - 1);
			j2 = std::min(std::max((int)std::floor((0.5f * t2 + 0.5f) * (float)N), 0), N - 1);
		}
		z[k] = cd[((size_t)g * N + j2) * N + i2];
	}
	if (missing >= 0) {
		float acc = 0.0f;
		for (int k = 0; k < 4; ++k) if (k != missing) acc += z[k];
		z[missing] = acc / 3.0f;
	}
}

}  // namespace

extern "C" {

// orc_resolve_cube with the depth-aware CubeCast: cube_depth float[6][N][N] (what the depth march left), depth float[H][W]
void orcd_resolve_cube(const uint8_t* cube, const float* cube_depth, int N, const orc_frame* fc, const float* wvp_i,
	int W, int H, const float* depth, float zn, float zf, float* out_rgba, uint8_t* covered)
{
	const CubeTex ct{ cube, N };
#pragma omp parallel for schedule(static)
	for (int py = 0; py < H; ++py)
		for (int px = 0; px < W; ++px) {
			float* o = out_rgba + ((size_t)py * W + px) * 4;
			o[0] = o[1] = o[2] = o[3] = 0.0f;
			covered[(size_t)py * W + px] = 0;
			const float u = ((float)px + 0.5f) / (float)W, v = ((float)py + 0.5f) / (float)H;
			const float q[3] = { std::fmaf(u, 2.0f, -1.0f), std::fmaf(v, -2.0f, 1.0f), 1.0f };
			float h[4];
			for (int r = 0; r < 4; ++r) {
				const float col[3] = { wvp_i[4 * r + 0], wvp_i[4 * r + 1], wvp_i[4 * r + 3] };
				h[r] = dp3(q, col);
			}
			float pos[3] = { h[0] / h[3], h[1] / h[3], h[2] / h[3] };
			const float e4[4] = { fc->eye_pt[0], fc->eye_pt[1], fc->eye_pt[2], 1.0f };
			float dir[3];
			for (int a = 0; a < 3; ++a) dir[a] = pos[a] + -dp4(e4, fc->world_i + 4 * a);
			const float inv = 1.0f / std::sqrt(dp3(dir, dir));
			for (int a = 0; a < 3; ++a) dir[a] = inv * dir[a];
			float t[3];
			for (int a = 0; a < 3; ++a) {
				const float sgn = (float)((int)(0.0f < dir[a]) - (int)(dir[a] < 0.0f));
				t[a] = (-pos[a] + sgn) / dir[a];
			}
			float U = 3.40282347e+38f;
			int hit = -1;
			for (int i = 0; i < 3; ++i) {
				const int j = (i + 1) % 3, k = (i + 2) % 3;
				if (!(t[i] >= 0.0f)) continue;
				if (!(1.0f >= std::fabs(std::fmaf(dir[j], t[i], pos[j])))) continue;
				if (1.0f < std::fabs(std::fmaf(dir[k], t[i], pos[k]))) continue;
				if (t[i] < U) { U = t[i]; hit = i; }
			}
			if (hit < 0) continue;
			float P[3];
			for (int a = 0; a < 3; ++a) P[a] = std::fmaf(dir[a], U, pos[a]);
			float uvx, uvy;
			if (hit == 0) { uvx = P[2] * -P[0]; uvy = P[1]; }
			else if (hit == 1) { uvx = P[0]; uvy = P[2] * -P[1]; }
			else { uvx = P[0] * P[2]; uvy = P[1]; }
			uvx = std::fmaf(uvx, 0.5f, 0.5f);
			uvy = std::fmaf(uvy, 0.5f, 0.5f);
			float s[4][4], fu, fv, z[4];
			footprint(ct, P, s, fu, fv);
			depth_footprint(cube_depth, N, P, z);                                          // :83
			const float zp = unproject_z(depth[(size_t)py * W + px], zn, zf);               // :84,99
			float dw[4];
			for (int k = 0; k < 4; ++k) dw[k] = std::fmax(std::fmaf(-0.5f, std::fabs(zp - unproject_z(z[k], zn, zf)), 1.0f), 0.0f);   // :107-108
			const float g = (float)N;
			const float vf = -uvy + 1.0f;
			const float vN = vf * g, uN = uvx * g;
			float dv = std::fmaf(vf, g, 0.5f), du = std::fmaf(uvx, g, 0.5f);
			dv = dv - std::floor(dv); du = du - std::floor(du);
			const float bound = g + -1.0f;
			bool ext = false;
			for (int a = 0; a < 3; ++a) {
				const float ax = P[a] * g;
				ext = ext || ((bound < std::fabs(ax)) && (dir[a] * ax < 0.0f));
			}
			if (ext) {
				dv = std::fmin(vN, g + -0.5f) < 0.5f ? 1.0f : 0.0f;
				du = std::fmin(uN, g + -0.5f) < 0.5f ? 1.0f : 0.0f;
			}
			const float idu = -du + 1.0f, idv = -dv + 1.0f;
			// w_i = dw_i wb_i (:109), association chosen so that dw = 1 gives the plain CubeCast's products and sum exactly
			const float a0 = dv * dw[0], a2 = du * dw[2], a3 = idv * dw[3];
			const float wy = dv * du * dw[1], wx = a0 * idu, wz = a2 * idv, ww = a3 * idu;
			float ws = std::fmaf(idu, a0, wy);
			ws = std::fmaf(idv, a2, ws);
			ws = std::fmaf(idu, a3, ws);
			float res[4];
			for (int ch = 0; ch < 4; ++ch) {
				float r = wy * s[1][ch];
				r = std::fmaf(s[0][ch], wx, r);
				r = std::fmaf(s[2][ch], wz, r);
				r = std::fmaf(s[3][ch], ww, r);
				res[ch] = r / ws;
			}
			if (!(0.0f < ws)) {                                                              // :119
				for (int ch = 0; ch < 4; ++ch)
					res[ch] = lerpf(lerpf(s[3][ch], s[2][ch], fu), lerpf(s[0][ch], s[1][ch], fu), fv);
			}
			if (0.0f >= res[3]) continue;
			for (int ch = 0; ch < 4; ++ch) o[ch] = res[ch];
			covered[(size_t)py * W + px] = 1;
		}
}

}  // extern "C"
