// fx_particle_draw.hip -- the particle draw (fx_set_particle_draw): the tracer particles as emissive points on the render target, each dimmed by the
// smoke between the eye and it, gfx950.  No reference counterpart.
//
//   k_draw_splat     every live record that projects onto the viewport adds its integer amounts to the uint64 pairs of the four pixels around it
//   k_draw_resolve   every pixel with a non-zero pair adds its light to the render target and clears the pair
//
// The trail's recipe (fx_particle_trail.hip): the scattered operation is an integer add, commutative and exact, so any order of arrival gives the
// same words; the integers become floats once per pixel.
//
// The rule, fp32, every operation rounded as written (include/fluidx_hip.h states it, tests/particle_draw_ref.py restates it in numpy);
// M = the forward WorldViewProj rows, (W, H) = the viewport, c(v) = fminf(fmaxf(v, 0), 1) (fx_particle_cell.h):
//   project    per live record (age >= 0, the move's test):  q_a = fma(c(p_a), 2, -1);  h_r = the dp4 chain of cube_tmax (fx_march.h) on (q, 1);
//              culled unless h_3 > 0;  (cx, cy, cz) = h_012 / h_3;  culled unless 0 <= cz < 1;  u = fma(cx, .5, .5), v = -fma(cy, .5, .5) + 1;
//              X = u * W, Y = v * H;  culled unless 0 <= X < W and 0 <= Y < H (a NaN fails every test);  the host pixel (px, py) = ((int)X, (int)Y)
//   depth      with a scene depth attached: culled unless cz <= depth[py][px]
//   occlusion  sa = the alpha of the direct view march of the host pixel (pixel_ray; 0 where it discards) ended at the particle:
//              tMax = depth_tmax at the pixel's centre with cz, march_alpha over max_ray_samples samples;  T = c(-sa + 1)
//   amounts    qb = (uint)(T * 32768 + 0.5);  s = lifetime > 0 ? c(age / lifetime) : 0;  qs = (uint)(s * 256 + 0.5);  young = qb (256 - qs), old = qb qs
//   footprint  per axis t = X - 0.5, fl = floorf(t), w1 = (int)rintf((t - fl) * 128), w0 = 128 - w1 on the pixels (int)fl and (int)fl + 1; a pixel
//              off the viewport is dropped;  acc[iy][ix] += (young, old) * wx * wy: at most 2^37 a word and record, 2^63 for 2^26 records
//   resolve    per pixel with acc0 | acc1 != 0:  Yv = (float)acc0 * 2^-37, Ov = (float)acc1 * 2^-37;  src_c = fma(Ov, k1_c, Yv * k0_c) with
//              k0_c = color_c * color_w, k1_c = end_color_c * end_color_w;  target = blend_premultiplied(target, src, 0) (alpha 0: additive, the
//              target's alpha stays);  target_float = (src, 0);  the pair goes back to 0.  Elsewhere the target is not stored, target_float = 0
//
// k_draw_splat: one lane per record, 256-thread workgroups, the record one 16-byte load.  A dead or culled lane has read its record and at most one
// depth texel when it leaves.  The march is the view march's chain of dependent gathers (march_alpha, fx_march.h: every sample gathers, the plain
// policy -- the occupancy masks of the accelerated render live in the LDS of its own kernels); a wave lasts as long as its longest ray.  The adds
// are no-return 64-bit integer atomics, up to eight a record.
// k_draw_resolve: one lane per pixel, one 16-byte load of the pair; everything else only where the pair is not zero.
#include "fx_march.h"
#include "fx_particle_cell.h"

namespace fx {

namespace {

const int DR_WG = 256;

typedef unsigned long long u64;

struct DrawSplatArgs { float wvp[16]; const float* depth; int W, H; uint32_t ns; float lifetime; };
struct DrawResolveArgs { float k0[3], k1[3]; uint32_t pixels; };

// one axis of the footprint: the first pixel (-1 .. n - 1) and the weights of the two
__device__ __forceinline__ void foot_axis(float x, int* i0, unsigned* w0, unsigned* w1)
{
	const float t = x - 0.5f;
	const float fl = floorf(t);
	const int q = (int)rintf((t - fl) * 128.0f);
	*i0 = (int)fl;
	*w1 = (unsigned)q;
	*w0 = 128u - (unsigned)q;
}

__device__ __forceinline__ void add_pair(u64* acc, int W, int H, int ix, int iy, unsigned young, unsigned old, unsigned w)
{
	if ((unsigned)ix >= (unsigned)W || (unsigned)iy >= (unsigned)H || !w) return;      // light that leaves the screen is lost
	u64* p = acc + 2 * ((size_t)iy * (size_t)W + (size_t)ix);
	const u64 a0 = (u64)young * (u64)w, a1 = (u64)old * (u64)w;
	if (a0) atomicAdd(p, a0);                                                          // (the results are not used: no-return)
	if (a1) atomicAdd(p + 1, a1);
}

}  // namespace

template <bool HALF>
__global__ __launch_bounds__(256) void k_draw_splat(const Geom g, const typename ColTex<HALF>::T* __restrict__ col, const FrameConsts fc,
	const DrawSplatArgs a, const float4* __restrict__ rec, unsigned count, u64* __restrict__ acc)
{
	const unsigned i = blockIdx.x * (unsigned)DR_WG + threadIdx.x;
	if (i >= count) return;
	const float4 r = rec[i];
	if (!(r.w >= 0.0f)) return;                                                         // dead: the move's test
	// ---- project
	const float qx = fmaf(clamp01(r.x), 2.0f, -1.0f), qy = fmaf(clamp01(r.y), 2.0f, -1.0f), qz = fmaf(clamp01(r.z), 2.0f, -1.0f);
	float h[4];
#pragma unroll
	for (int k = 0; k < 4; ++k) h[k] = fmaf(1.0f, a.wvp[4 * k + 3], fmaf(qz, a.wvp[4 * k + 2], fmaf(qy, a.wvp[4 * k + 1], qx * a.wvp[4 * k + 0])));
	if (!(h[3] > 0.0f)) return;
	const float cx = h[0] / h[3], cy = h[1] / h[3], cz = h[2] / h[3];
	if (!(0.0f <= cz && cz < 1.0f)) return;
	const float u = fmaf(cx, 0.5f, 0.5f), v = -fmaf(cy, 0.5f, 0.5f) + 1.0f;
	const float X = u * (float)a.W, Y = v * (float)a.H;
	if (!(0.0f <= X && X < (float)a.W && 0.0f <= Y && Y < (float)a.H)) return;
	const int px = (int)X, py = (int)Y;                                                 // in [0, W) x [0, H): tested above
	// ---- scene depth
	if (a.depth != nullptr && !(cz <= a.depth[(size_t)py * (size_t)a.W + (size_t)px])) return;
	// ---- occlusion: the direct march of the host pixel, ended at the particle
	float o[3], d[3];
	float sa = 0.0f;
	if (pixel_ray(fc, px, py, a.W, a.H, o, d)) {
		const float upc = ((float)px + 0.5f) / (float)a.W, vpc = ((float)py + 0.5f) / (float)a.H;
		const float tMax = depth_tmax(fc, fmaf(upc, 2.0f, -1.0f), fmaf(vpc, -2.0f, 1.0f), cz, o, d);
		const PlainVol<HALF> vol{ col };
		sa = march_alpha(g, vol, o, d, tMax, a.ns, true);
	}
	const float T = clamp01(-sa + 1.0f);
	// ---- amounts
	const unsigned qb = (unsigned)(T * 32768.0f + 0.5f);
	const float s = a.lifetime > 0.0f ? clamp01(r.w / a.lifetime) : 0.0f;
	const unsigned qs = (unsigned)(s * 256.0f + 0.5f);
	const unsigned young = qb * (256u - qs), old = qb * qs;
	if (!qb) return;
	// ---- footprint
	int ix, iy;
	unsigned wx0, wx1, wy0, wy1;
	foot_axis(X, &ix, &wx0, &wx1);
	foot_axis(Y, &iy, &wy0, &wy1);
	add_pair(acc, a.W, a.H, ix, iy, young, old, wx0 * wy0);
	add_pair(acc, a.W, a.H, ix + 1, iy, young, old, wx1 * wy0);
	add_pair(acc, a.W, a.H, ix, iy + 1, young, old, wx0 * wy1);
	add_pair(acc, a.W, a.H, ix + 1, iy + 1, young, old, wx1 * wy1);
}

__global__ __launch_bounds__(256) void k_draw_resolve(const DrawResolveArgs a, u64* __restrict__ acc, uint32_t* __restrict__ target, float4* __restrict__ out_float)
{
	const unsigned pix = blockIdx.x * (unsigned)DR_WG + threadIdx.x;
	if (pix >= a.pixels) return;
	ulonglong2* word = reinterpret_cast<ulonglong2*>(acc) + pix;
	const ulonglong2 v = *word;
	if ((v.x | v.y) == 0) { out_float[pix] = make_float4(0.0f, 0.0f, 0.0f, 0.0f); return; }   // no particle near: the target keeps its bytes
	*word = make_ulonglong2(0, 0);
	const float Yv = (float)v.x * 0x1p-37f, Ov = (float)v.y * 0x1p-37f;
	float src[3];
#pragma unroll
	for (int c = 0; c < 3; ++c) src[c] = fmaf(Ov, a.k1[c], Yv * a.k0[c]);
	target[pix] = blend_premultiplied(target[pix], src[0], src[1], src[2], 0.0f);
	out_float[pix] = make_float4(src[0], src[1], src[2], 0.0f);
}

// wvp: the forward WorldViewProj rows; depth: the scene depth float[H][W] or null; ns: the merged direct march's sample count
hipError_t launch_draw_splat(const Geom& g, int half_store, const void* color, const FrameConsts& fc, const float wvp[16], const float* depth, int W, int H,
	uint32_t ns, float lifetime, const float* records, uint32_t count, unsigned long long* acc, hipStream_t s)
{
	if (!whole_grid(g)) return hipErrorNotSupported;                            // (fx_set_particle_draw refuses slab ranks)
	if (!records || !acc || !color || count > FX_MAX_PARTICLES || W <= 0 || H <= 0 || !ns) return hipErrorInvalidValue;
	// (tap indices are 32 bits wide and put together by 24-bit multiplies, fx_march.h make_taps: fx_render's own limits)
	if (g.Zg <= 1 || (uint64_t)g.Y * ((uint64_t)g.Zg + 1) >= (1u << 24) || g.cells_owned() >= ((size_t)1 << 32)) return hipErrorInvalidValue;
	if (count == 0) return hipSuccess;
	DrawSplatArgs a;
	for (int k = 0; k < 16; ++k) a.wvp[k] = wvp[k];
	a.depth = depth; a.W = W; a.H = H; a.ns = ns; a.lifetime = lifetime;
	const dim3 grid((count + DR_WG - 1) / DR_WG, 1, 1);
	const float4* rec = reinterpret_cast<const float4*>(records);
	if (half_store) hipLaunchKernelGGL(k_draw_splat<true>, grid, dim3(DR_WG), 0, s, g, (const h16x4*)color, fc, a, rec, count, acc);
	else hipLaunchKernelGGL(k_draw_splat<false>, grid, dim3(DR_WG), 0, s, g, (const float4*)color, fc, a, rec, count, acc);
	return hipGetLastError();
}

hipError_t launch_draw_resolve(const fx_particle_draw& dr, int W, int H, unsigned long long* acc, uint8_t* target, float* out_float, hipStream_t s)
{
	if (!acc || !target || !out_float || W <= 0 || H <= 0 || (uint64_t)W * (uint64_t)H > 0x7FFFFFFFu) return hipErrorInvalidValue;
	DrawResolveArgs a;
	for (int c = 0; c < 3; ++c) { a.k0[c] = dr.color[c] * dr.color[3]; a.k1[c] = dr.end_color[c] * dr.end_color[3]; }
	a.pixels = (uint32_t)W * (uint32_t)H;
	hipLaunchKernelGGL(k_draw_resolve, dim3((a.pixels + DR_WG - 1) / DR_WG), dim3(DR_WG), 0, s, a, acc, reinterpret_cast<uint32_t*>(target),
		reinterpret_cast<float4*>(out_float));
	return hipGetLastError();
}

}  // namespace fx
