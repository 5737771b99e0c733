// fx_mesh_args.h -- what fx_set_obstacle_meshes can tell about its list without looking at the geometry (a device mesh cannot be read up
// front, and bad geometry is defined behaviour anyway).  Host code with no HIP in it: a stand-alone program can call it.
#pragma once
#include "../../include/fluidx_hip.h"

namespace fx {

// FX_OK or FX_E_INVALID; reads count entries of the list and nothing they point to
inline int mesh_args_status(const fx_obstacle_mesh* meshes, uint32_t count)
{
	if (!meshes || count == 0 || count > FX_MAX_OBSTACLE_MESHES) return FX_E_INVALID;
	for (uint32_t k = 0; k < count; ++k) {
		const fx_obstacle_mesh& m = meshes[k];
		if (m.struct_size != sizeof(fx_obstacle_mesh) || (m.flags & ~(uint32_t)FX_MESH_DEVICE)) return FX_E_INVALID;
		if (m.triangle_count && (!m.positions || !m.indices)) return FX_E_INVALID;
	}
	return FX_OK;
}

// bytes of the voxeliser's work buffer a list needs: per mesh the list of large triangles (16 bytes a triangle) and, for a host mesh, its copy
// behind it (indices, positions, transform); the largest over the list
inline size_t mesh_work_bytes(const fx_obstacle_mesh* meshes, uint32_t count)
{
	size_t need = 16;
	for (uint32_t k = 0; k < count; ++k) {
		const fx_obstacle_mesh& m = meshes[k];
		if (!m.triangle_count) continue;
		size_t b = (size_t)16 * m.triangle_count;
		if (!(m.flags & FX_MESH_DEVICE)) b += (size_t)12 * m.triangle_count + (size_t)12 * m.vertex_count + 48;
		if (b > need) need = b;
	}
	return need;
}

}  // namespace fx
