// tests/obstacle_ref/obstacle_ref.cpp -- CPU reference of the solid obstacles (include/fluidx_hip.h fx_set_obstacles), TEST INFRASTRUCTURE ONLY.
// A plain restatement of the header's four rules -- enforce, divergence, relaxation, projection -- with a mask S = uint8[Z][Y][X], in the
// layouts and the operation order of the oracle (oracle/orc_sim.cpp: velocity float[3][Z][Y][X], colour float[Z][Y][X][4], scalars
// float[Z][Y][X]; -ffp-contract=off, a fused multiply-add only where the text says fmaf), and a whole step composed with the oracle's advection.
// Unlike the kernels it reads the MASK at the clamped neighbour, never a code byte: obr_codes restates the code byte on its own, for the
// test of k_obstacle_codes.  fp16 storage: the caller hands in values that are binary16 already (widen on load), stored values are rounded
// once (RNE).  Built on demand by tests/test_obstacle_ref.py with the oracle's flags, together with oracle/orc_sim.cpp.
#include "../../oracle/orc_common.h"
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

extern "C" void orc_advect(const float* vel_in, const float* col_in, float* vel_out, float* col_out, int X, int Y, int Z, float dt, int address_mode,
	int half_storage);

namespace {

struct Box {
	int X, Y, Z;
	const uint8_t* S;
	size_t n() const { return (size_t)X * Y * Z; }
	size_t at(int x, int y, int z) const { return ((size_t)z * Y + y) * X + x; }
	bool solid(int x, int y, int z) const { return S[at(x, y, z)] != 0; }
	// the neighbour along axis a, direction d = -1 / +1, index clamped to the grid
	void nb(int x, int y, int z, int a, int d, int& nx, int& ny, int& nz) const
	{
		nx = x; ny = y; nz = z;
		int& c = a == 0 ? nx : a == 1 ? ny : nz;
		const int hi = (a == 0 ? X : a == 1 ? Y : Z) - 1;
		c = std::min(std::max(c + d, 0), hi);
	}
};

inline float stored(float v, int half) { return half ? orc::quant_half(v) : v; }

// field f at the neighbour of (x, y, z) along a / d; `inside` is what a neighbour in a solid reads as
inline float tap(const Box& g, const float* f, int x, int y, int z, int a, int d, float inside)
{
	int nx, ny, nz;
	g.nb(x, y, z, a, d, nx, ny, nz);
	return g.solid(nx, ny, nz) ? inside : f[g.at(nx, ny, nz)];
}

}  // namespace

extern "C" {

// bits 0..5: S of the clamped neighbour at x-1, x+1, y-1, y+1, z-1, z+1 (z bits 0 on 2-D grids); bit 6: S of the cell
void obr_codes(const uint8_t* S, uint8_t* code, int X, int Y, int Z)
{
	const Box g{ X, Y, Z, S };
	for (int z = 0; z < Z; ++z)
		for (int y = 0; y < Y; ++y)
			for (int x = 0; x < X; ++x) {
				unsigned k = 0;
				for (int a = 0; a < (Z > 1 ? 3 : 2); ++a)
					for (int s = 0; s < 2; ++s) {
						int nx, ny, nz;
						g.nb(x, y, z, a, s ? 1 : -1, nx, ny, nz);
						if (g.solid(nx, ny, nz)) k |= 1u << (2 * a + s);
					}
				if (g.solid(x, y, z)) k |= 64u;
				code[g.at(x, y, z)] = (uint8_t)k;
			}
}

// in place: a solid cell's three velocity and four colour components become +0
void obr_enforce(float* vel, float* col, const uint8_t* S, int X, int Y, int Z)
{
	const size_t N = (size_t)X * Y * Z;
	for (size_t i = 0; i < N; ++i) {
		if (!S[i]) continue;
		for (int a = 0; a < 3; ++a) vel[a * N + i] = 0.0f;
		for (int a = 0; a < 4; ++a) col[4 * i + a] = 0.0f;
	}
}

void obr_divergence(const float* vel, const uint8_t* S, float* b, int X, int Y, int Z)
{
	const Box g{ X, Y, Z, S };
	const size_t N = g.n();
	for (int z = 0; z < Z; ++z)
		for (int y = 0; y < Y; ++y)
			for (int x = 0; x < X; ++x) {
				float dd[3] = { 0.0f, 0.0f, 0.0f };
				for (int a = 0; a < (Z > 1 ? 3 : 2); ++a)
					dd[a] = -tap(g, vel + a * N, x, y, z, a, -1, 0.0f) + tap(g, vel + a * N, x, y, z, a, 1, 0.0f);
				const float sum = Z > 1 ? dd[2] + (dd[1] + dd[0]) : dd[0] + dd[1];
				b[g.at(x, y, z)] = g.solid(x, y, z) ? 0.0f : 0.5f * sum;
			}
}

void obr_sweep(const float* p_in, const float* b, const uint8_t* S, float* p_out, int X, int Y, int Z)
{
	const Box g{ X, Y, Z, S };
	const float inv = Z > 1 ? orc::bits2f(0x3e2aaaabu) : 0.25f;
	for (int z = 0; z < Z; ++z)
		for (int y = 0; y < Y; ++y)
			for (int x = 0; x < X; ++x) {
				const size_t id = g.at(x, y, z);
				const float c = p_in[id];
				float s = tap(g, p_in, x, y, z, 0, -1, c) - b[id];
				s = tap(g, p_in, x, y, z, 0, 1, c) + s;
				s = tap(g, p_in, x, y, z, 1, -1, c) + s;
				s = tap(g, p_in, x, y, z, 1, 1, c) + s;
				if (Z > 1) {
					s = tap(g, p_in, x, y, z, 2, -1, c) + s;
					s = tap(g, p_in, x, y, z, 2, 1, c) + s;
				}
				p_out[id] = g.solid(x, y, z) ? 0.0f : s * inv;
			}
}

// n sweeps from p (in / out); tmp: scratch of the same size
void obr_jacobi(float* p, const float* b, const uint8_t* S, float* tmp, int X, int Y, int Z, int n)
{
	float* src = p; float* dst = tmp;
	for (int k = 0; k < n; ++k) { obr_sweep(src, b, S, dst, X, Y, Z); std::swap(src, dst); }
	if (src != p) std::memcpy(p, src, (size_t)X * Y * Z * sizeof(float));
}

void obr_project(const float* vel_in, const float* p, const uint8_t* S, float* vel_out, int X, int Y, int Z, int half)
{
	const Box g{ X, Y, Z, S };
	const size_t N = g.n();
	const bool is3d = Z > 1;
	const float k = is3d ? orc::bits2f(0x3f855556u) : 0.5f;
	const float dims[3] = { (float)X, (float)Y, (float)Z };
	for (int z = 0; z < Z; ++z)
		for (int y = 0; y < Y; ++y)
			for (int x = 0; x < X; ++x) {
				const size_t id = g.at(x, y, z);
				const int cell[3] = { x, y, z };
				const float c = p[id];
				float u[3] = { vel_in[id], vel_in[N + id], vel_in[2 * N + id] };
				for (int a = 0; a < (is3d ? 3 : 2); ++a) {
					const float grad = -tap(g, p, x, y, z, a, -1, c) + tap(g, p, x, y, z, a, 1, c);
					u[a] = std::fmaf(-grad, k, u[a]);
					int nx, ny, nz;
					g.nb(x, y, z, a, -1, nx, ny, nz);
					bool beside = g.solid(nx, ny, nz);
					g.nb(x, y, z, a, 1, nx, ny, nz);
					beside = beside || g.solid(nx, ny, nz);
					if (beside) u[a] = 0.0f;                            // free slip against a resting solid
				}
				for (int a = 0; a < 3; ++a) {                           // the wall damping, as without obstacles
					float pos = ((float)cell[a] + 0.5f) / dims[a];
					if (is3d || a < 2) pos = std::fmaf(pos, 2.0f, -1.0f);
					float f = (-std::fabs(pos) + 0.970000029f) * 33.3333359f;
					f = std::fmin(std::fmax(f, -1.0f), 1.0f);
					const float w = (0.0f < u[a] * pos) ? f : 1.0f;
					vel_out[a * N + id] = g.solid(x, y, z) ? 0.0f : stored(u[a] * w, half);
				}
			}
}

// one step: the oracle's advection, then enforce, divergence, `iters` sweeps, projection (dt <= 0: the advected velocity is copied, as in the oracle).
// vel0 / vel1: the two velocity fields (advect 0 -> 1, project 1 -> 0); col_src / col_dst: colour[!parity] / colour[parity]; p: warm start
void obr_step(float* vel0, float* vel1, const float* col_src, float* col_dst, float* p, float* b, float* tmp, const uint8_t* S,
	int X, int Y, int Z, float dt, int iters, int address, int half)
{
	orc_advect(vel0, col_src, vel1, col_dst, X, Y, Z, dt, address, half);
	if (dt > 0.0f) {
		obr_enforce(vel1, col_dst, S, X, Y, Z);
		obr_divergence(vel1, S, b, X, Y, Z);
		obr_jacobi(p, b, S, tmp, X, Y, Z, iters);
		obr_project(vel1, p, S, vel0, X, Y, Z, half);
	} else {
		std::memcpy(vel0, vel1, 3 * (size_t)X * Y * Z * sizeof(float));
	}
}

}  // extern "C"
