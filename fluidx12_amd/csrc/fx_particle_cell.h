// fx_particle_cell.h -- the two primitives the particle kernels share (fx_particles.hip: the move and the point query; fx_particle_sort.hip:
// the sort key; fx_particle_trail.hip: the scatter's taps): the clamp that stands in front of every index a record's position forms, and the cell of a clamped coordinate.  Device code only.
#pragma once

namespace fx {

// c(v): a NaN becomes 0, -0 becomes either zero (the product with an extent is 0 whichever it is)
__device__ __forceinline__ float clamp01(float v) { return fminf(fmaxf(v, 0.0f), 1.0f); }

// the cell of a coordinate s = c(v) along an axis of n cells: 1.0 lands in the last one
__device__ __forceinline__ int cell_axis(float s, int n) { return min((int)(s * (float)n), n - 1); }

}  // namespace fx
