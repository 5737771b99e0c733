// fx_store.h -- how the optional stages of the step (fx_vorticity.hip, fx_emit.hip, fx_obstacle.hip, fx_heat.hip, fx_open.hip) the MacCormack
// advection (fx_maccormack.hip), the multigrid pressure solver (fx_multigrid.hip), the tracer particles (fx_particles.hip) and their trail (fx_particle_trail.hip) read and write a
// stored field: fp32, or binary16 widened on load and rounded once (RNE) on store.  Device code only: included by those files, never by
// fx_internal.h (host-only programs include that one).  The kernels of fx_sim.hip keep their own Store<HALF>, the original of the device below.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>

namespace fx {
namespace sto {

typedef _Float16 h16;
typedef _Float16 h16x4 __attribute__((ext_vector_type(4)));

// the fp32 value is rounded to binary16 in a step of its own (RNE): the empty asm keeps the compiler from folding the producing FMA (add,
// multiply) and the conversion into one mixed-precision instruction that rounds once (the same device as Store<true> of fx_sim.hip)
__device__ __forceinline__ h16 to_h16(float v) { asm("" : "+v"(v)); return (h16)v; }

// WIDE: fields of 4 GiB and more -- 64-bit byte offsets; otherwise 32-bit ones from uniform bases (saddr + voffset accesses)
template <bool WIDE> struct Off { typedef uint32_t T; };
template <> struct Off<true> { typedef size_t T; };

// by cell index from a byte base: one value of a scalar plane (ld1 / st1), the colour texel (ld4 / st4) and its alpha
template <bool HALF> struct Cell;
template <> struct Cell<false> {
	template <typename O> static __device__ __forceinline__ float ld1(const char* b, O cell) { return *reinterpret_cast<const float*>(b + cell * (O)4); }
	template <typename O> static __device__ __forceinline__ void st1(char* b, O cell, float v) { *reinterpret_cast<float*>(b + cell * (O)4) = v; }
	template <typename O> static __device__ __forceinline__ float alpha(const char* b, O cell) { return *reinterpret_cast<const float*>(b + cell * (O)16 + (O)12); }
	template <typename O> static __device__ __forceinline__ float4 ld4(const char* b, O cell) { return *reinterpret_cast<const float4*>(b + cell * (O)16); }
	// stores the texel, returns the alpha a later load of it yields
	template <typename O> static __device__ __forceinline__ float st4(char* b, O cell, const float (&c)[4])
	{
		*reinterpret_cast<float4*>(b + cell * (O)16) = make_float4(c[0], c[1], c[2], c[3]);
		return c[3];
	}
};
template <> struct Cell<true> {
	template <typename O> static __device__ __forceinline__ float ld1(const char* b, O cell) { return (float)*reinterpret_cast<const h16*>(b + cell * (O)2); }
	template <typename O> static __device__ __forceinline__ void st1(char* b, O cell, float v) { *reinterpret_cast<h16*>(b + cell * (O)2) = to_h16(v); }
	template <typename O> static __device__ __forceinline__ float alpha(const char* b, O cell) { return (float)*reinterpret_cast<const h16*>(b + cell * (O)8 + (O)6); }
	template <typename O> static __device__ __forceinline__ float4 ld4(const char* b, O cell)
	{
		const h16x4 h = *reinterpret_cast<const h16x4*>(b + cell * (O)8);
		return make_float4((float)h.x, (float)h.y, (float)h.z, (float)h.w);
	}
	template <typename O> static __device__ __forceinline__ float st4(char* b, O cell, const float (&c)[4])
	{
		h16x4 h;
		h.x = to_h16(c[0]); h.y = to_h16(c[1]); h.z = to_h16(c[2]); h.w = to_h16(c[3]);
		*reinterpret_cast<h16x4*>(b + cell * (O)8) = h;
		return (float)h.w;
	}
};

// the same by element index from a typed pointer (S: a velocity component or scalar, S4: the colour texel)
template <bool HALF> struct Sto;
template <> struct Sto<false> {
	typedef float S;
	typedef float4 S4;
	static __device__ __forceinline__ float ld(const S* p, size_t i) { return p[i]; }
	static __device__ __forceinline__ void st(S* p, size_t i, float v) { p[i] = v; }
	static __device__ __forceinline__ void zero4(S4* p, size_t i) { p[i] = make_float4(0.0f, 0.0f, 0.0f, 0.0f); }
};
template <> struct Sto<true> {
	typedef h16 S;
	typedef h16x4 S4;
	static __device__ __forceinline__ float ld(const S* p, size_t i) { return (float)p[i]; }
	static __device__ __forceinline__ void st(S* p, size_t i, float v) { p[i] = to_h16(v); }
	static __device__ __forceinline__ void zero4(S4* p, size_t i) { h16x4 h; h.x = h.y = h.z = h.w = (h16)0.0f; p[i] = h; }
};

}  // namespace sto
}  // namespace fx
