"""ctypes declarations of the C ABI in include/fluidx_hip.h (libfluidx_hip.so).

The library is the product: there is no Python/CPU fallback.  `load()` raises if the HIP
extension cannot be built or loaded.
"""
import ctypes as C
import os

from . import build as _build

FX_OK = 0
FX_E_INVALID, FX_E_DEVICE, FX_E_NOMEM, FX_E_STATE, FX_E_COMM, FX_E_HALO = -1, -2, -3, -4, -5, -6

RAY_MARCH_DIRECT, RAY_MARCH_CUBEMAP, SEPARATE_LIGHT_PASS, OPTIMIZED = 0, 1, 2, 3
FRAME_COUNT = 3
STORAGE_FP32, STORAGE_FP16 = 0, 1
JACOBI_FIXED, JACOBI_FAITHFUL = 0, 1
ADDRESS_CLAMP, ADDRESS_MIRROR = 0, 1
FLAG_JACOBI_FUSE_MASK, FLAG_NO_OVERLAP, FLAG_RENDER_ONLY = 0xF, 0x10, 0x20
OPT_OVERLAP, OPT_JACOBI_ROUND, OPT_ADAPTIVE_HALO, OPT_COUNT_SAMPLES, OPT_RENDER_ACCEL = 1, 2, 3, 4, 5
ABI_VERSION = 7                      # FX_ABI_VERSION of include/fluidx_hip.h
(FIELD_VELOCITY, FIELD_VELOCITY1, FIELD_COLOR, FIELD_COLOR_PREV, FIELD_PRESSURE, FIELD_DIVERGENCE,
 FIELD_LIGHTMAP, FIELD_CUBEMAP, FIELD_TARGET, FIELD_TARGET_FLOAT, FIELD_CUBE_DEPTH) = range(11)
FIELD_TEMPERATURE = 11               # FX_FIELD_TEMPERATURE: float[Z][Y][X], only while fx_set_buoyancy has it on
DEPTH_DEVICE = 0x1                   # fx_set_scene_depth: the depth buffer is device memory, read in place
LIGHT_DIRECTIONAL, LIGHT_POINT = 0, 1   # fx_light.kind
MAX_EMITTERS = 16                    # FX_MAX_EMITTERS
OBSTACLES_DEVICE = 0x1               # fx_set_obstacles: the mask is device memory
MAX_OBSTACLE_BODIES = 16             # FX_MAX_OBSTACLE_BODIES
MAX_OBSTACLE_MESHES = 16             # FX_MAX_OBSTACLE_MESHES
MESH_DEVICE = 0x1                    # FX_MESH_DEVICE: fx_obstacle_mesh's positions / indices / transform are device memory
MAX_HEAT_SOURCES = 16                # FX_MAX_HEAT_SOURCES
WALL_X_LO, WALL_X_HI, WALL_Y_LO, WALL_Y_HI, WALL_Z_LO, WALL_Z_HI = 0x01, 0x02, 0x04, 0x08, 0x10, 0x20   # FX_WALL_*: fx_set_open_walls
WALL_ALL = 0x3F
ADVECT_SEMI_LAGRANGIAN, ADVECT_MACCORMACK = 0, 1   # FX_ADVECT_*: fx_set_advection_scheme
PRESSURE_JACOBI, PRESSURE_MULTIGRID = 0, 1         # FX_PRESSURE_*: fx_set_pressure_solver
MG_NO_TAIL = 0x1                                   # FX_MG_NO_TAIL
MG_MAX_LEVELS = 12                                 # FX_MG_MAX_LEVELS
MAX_PARTICLES = 1 << 26                            # FX_MAX_PARTICLES
PARTICLES_DEVICE = 0x1                             # FX_PARTICLES_DEVICE: fx_set_particles / fx_sample_velocity take device pointers
PARTICLE_EULER, PARTICLE_MIDPOINT = 0, 1           # FX_PARTICLE_*: fx_particle_params.scheme
MAX_PARTICLE_SPAWNERS = 16                         # FX_MAX_PARTICLE_SPAWNERS
SPAWN_BOX, SPAWN_BALL = 0, 1                       # FX_SPAWN_*: fx_particle_spawner.shape
DRAW_AMOUNT_ONE = 1 << 37                          # fx_particle_splats: what an unoccluded particle whose footprint is on screen adds to a pixel pair in total


class Desc(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("grid_x", C.c_uint32), ("grid_y", C.c_uint32), ("grid_z", C.c_uint32),
                ("viewport_w", C.c_uint32), ("viewport_h", C.c_uint32), ("storage", C.c_uint32),
                ("jacobi_iters", C.c_uint32), ("jacobi_mode", C.c_uint32), ("advect_address", C.c_uint32),
                ("device", C.c_int32), ("slab_z0", C.c_uint32), ("slab_nz", C.c_uint32),
                ("halo_advect", C.c_uint32), ("halo_jacobi", C.c_uint32), ("flags", C.c_uint32)]


class FrameInfo(C.Structure):
    _fields_ = [("cube_lod", C.c_uint32), ("cube_size", C.c_uint32), ("ray_samples", C.c_uint32),
                ("visibility_mask", C.c_uint32), ("frame_parity", C.c_uint32), ("edge_pixels", C.c_float),
                ("time_step", C.c_float), ("world_view_proj_i", C.c_float * 16), ("screen_to_world", C.c_float * 16)]


class Light(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("kind", C.c_uint32), ("position", C.c_float * 3), ("color", C.c_float * 4),
                ("ambient", C.c_float * 4)]


class Emitter(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("flags", C.c_uint32), ("center", C.c_float * 3), ("radius", C.c_float),
                ("color_rate", C.c_float * 4), ("force", C.c_float * 3), ("swirl", C.c_float)]


class ObstacleBody(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("flags", C.c_uint32), ("box_lo", C.c_float * 3), ("box_hi", C.c_float * 3),
                ("linear", C.c_float * 3), ("angular", C.c_float * 3), ("pivot", C.c_float * 3)]


class ObstacleMesh(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("flags", C.c_uint32), ("positions", C.c_void_p), ("indices", C.c_void_p),
                ("vertex_count", C.c_uint32), ("triangle_count", C.c_uint32), ("transform", C.c_void_p)]


class MeshReport(C.Structure):
    _fields_ = [("solid_cells", C.c_uint64), ("open_columns", C.c_uint32), ("skipped_triangles", C.c_uint32)]


class Buoyancy(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("flags", C.c_uint32), ("ambient", C.c_float), ("density_weight", C.c_float),
                ("lift", C.c_float), ("cooling", C.c_float), ("up", C.c_float * 3)]


class HeatSource(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("flags", C.c_uint32), ("center", C.c_float * 3), ("radius", C.c_float), ("rate", C.c_float)]


class PressureSolver(C.Structure):
    _fields_ = [("kind", C.c_uint32), ("flags", C.c_uint32), ("cycles", C.c_uint32), ("pre_sweeps", C.c_uint32), ("post_sweeps", C.c_uint32),
                ("coarse_sweeps", C.c_uint32), ("max_levels", C.c_uint32), ("omega", C.c_float)]


class ParticleParams(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("flags", C.c_uint32), ("scheme", C.c_uint32), ("drift", C.c_float * 3), ("lifetime", C.c_float)]


class ParticleSort(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("flags", C.c_uint32), ("enabled", C.c_uint32), ("every", C.c_uint32)]


class ParticleSortInfo(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("live", C.c_uint32), ("sorts", C.c_uint32), ("reserved", C.c_uint32)]


class ParticleTrail(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("flags", C.c_uint32), ("rate", C.c_float), ("tint", C.c_float * 4), ("heat", C.c_float)]


class ParticleSpawner(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("flags", C.c_uint32), ("shape", C.c_uint32), ("seed", C.c_uint32), ("center", C.c_float * 3),
                ("half_extent", C.c_float * 3), ("rate", C.c_float), ("age_spread", C.c_float)]


class ParticleDraw(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("flags", C.c_uint32), ("color", C.c_float * 4), ("end_color", C.c_float * 4)]


class ObstacleDraw(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("flags", C.c_uint32), ("albedo", C.c_float * 4)]


class ParticleSpawnInfo(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("reserved", C.c_uint32), ("born", C.c_uint64), ("dropped", C.c_uint64), ("blocked", C.c_uint64),
                ("serial", C.c_uint64 * 16)]


class Timing(C.Structure):
    _fields_ = [("advect_ms", C.c_double), ("divergence_ms", C.c_double), ("jacobi_ms", C.c_double),
                ("project_ms", C.c_double), ("light_ms", C.c_double), ("view_ms", C.c_double),
                ("exchange_ms", C.c_double), ("steps", C.c_uint64), ("jacobi_launches", C.c_uint64),
                ("jacobi_sweeps", C.c_uint64), ("renders", C.c_uint64), ("resolve_ms", C.c_double),
                ("jacobi_main_ms", C.c_double), ("jacobi_main_launches", C.c_uint64), ("jacobi_main_sweeps", C.c_uint64),
                ("exchange_bytes", C.c_uint64), ("advect_halo_planes", C.c_uint64), ("chain_ms", C.c_double),
                ("freeze_solves", C.c_uint64), ("freeze_sweeps", C.c_uint64), ("exchange_calls", C.c_uint64),
                ("view_samples", C.c_uint64), ("light_samples", C.c_uint64), ("lightmap_fetches", C.c_uint64),
                ("freeze_strip_launches", C.c_uint64)]


# every symbol include/fluidx_hip.h declares: name -> (restype, argtypes)
_vp, _fp = C.c_void_p, C.POINTER(C.c_float)
SYMBOLS = {
    "fx_abi_version": (C.c_int, []),
    "fx_error_string": (C.c_char_p, [C.c_int]),
    "fx_create": (C.c_int, [C.POINTER(_vp), C.POINTER(Desc)]),
    "fx_destroy": (C.c_int, [_vp]),
    "fx_set_max_samples": (C.c_int, [_vp, C.c_uint32, C.c_uint32]),
    "fx_set_sh": (C.c_int, [_vp, _fp]),
    "fx_update_frame": (C.c_int, [_vp, C.c_float, C.c_uint8, _fp, _fp, _fp]),
    "fx_simulate": (C.c_int, [_vp, _vp, C.c_uint8]),
    "fx_render": (C.c_int, [_vp, _vp, C.c_uint8, C.c_uint8]),
    "fx_get_frame_info": (C.c_int, [_vp, C.POINTER(FrameInfo)]),
    "fx_synchronize": (C.c_int, [_vp]),
    "fx_last_error": (C.c_char_p, [_vp]),
    "fx_upload": (C.c_int, [_vp, C.c_int, _vp, C.c_size_t]),
    "fx_download": (C.c_int, [_vp, C.c_int, _vp, C.c_size_t]),
    "fx_field_bytes": (C.c_size_t, [_vp, C.c_int]),
    "fx_field_digest": (C.c_int, [_vp, C.c_int, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint64)]),
    "fx_checkpoint_save": (C.c_int, [_vp, C.c_char_p]),
    "fx_checkpoint_load": (C.c_int, [_vp, C.c_char_p]),
    "fx_advect": (C.c_int, [_vp, _vp]),
    "fx_divergence": (C.c_int, [_vp, _vp]),
    "fx_jacobi": (C.c_int, [_vp, _vp, C.c_uint32]),
    "fx_project": (C.c_int, [_vp, _vp]),
    "fx_set_vorticity_confinement": (C.c_int, [_vp, C.c_float]),
    "fx_confine_vorticity": (C.c_int, [_vp, _vp]),
    "fx_set_emitters": (C.c_int, [_vp, C.POINTER(Emitter), C.c_uint32]),
    "fx_get_emitters": (C.c_int, [_vp, C.POINTER(Emitter), C.c_uint32, C.POINTER(C.c_uint32)]),
    "fx_set_impulse": (C.c_int, [_vp, C.c_int]),
    "fx_emit": (C.c_int, [_vp, _vp]),
    "fx_set_obstacles": (C.c_int, [_vp, _vp, _vp, C.c_size_t, C.c_uint32]),
    "fx_get_obstacles": (C.c_int, [_vp, _vp, C.c_size_t, C.POINTER(C.c_uint64)]),
    "fx_enforce_obstacles": (C.c_int, [_vp, _vp]),
    "fx_set_obstacle_bodies": (C.c_int, [_vp, C.POINTER(ObstacleBody), C.c_uint32]),
    "fx_get_obstacle_bodies": (C.c_int, [_vp, C.POINTER(ObstacleBody), C.c_uint32, C.POINTER(C.c_uint32)]),
    "fx_set_obstacle_meshes": (C.c_int, [_vp, _vp, C.POINTER(ObstacleMesh), C.c_uint32, C.POINTER(MeshReport)]),
    "fx_set_buoyancy": (C.c_int, [_vp, C.POINTER(Buoyancy)]),
    "fx_get_buoyancy": (C.c_int, [_vp, C.POINTER(Buoyancy), C.POINTER(C.c_int)]),
    "fx_set_heat_sources": (C.c_int, [_vp, C.POINTER(HeatSource), C.c_uint32]),
    "fx_get_heat_sources": (C.c_int, [_vp, C.POINTER(HeatSource), C.c_uint32, C.POINTER(C.c_uint32)]),
    "fx_heat": (C.c_int, [_vp, _vp]),
    "fx_set_particles": (C.c_int, [_vp, _vp, _fp, C.c_uint32, C.c_uint32]),
    "fx_get_particles": (C.c_int, [_vp, _fp, C.c_uint32, C.POINTER(C.c_uint32)]),
    "fx_particles_device": (C.c_int, [_vp, C.POINTER(_vp), C.POINTER(C.c_uint32)]),
    "fx_set_particle_params": (C.c_int, [_vp, C.POINTER(ParticleParams)]),
    "fx_get_particle_params": (C.c_int, [_vp, C.POINTER(ParticleParams)]),
    "fx_move_particles": (C.c_int, [_vp, _vp]),
    "fx_sample_velocity": (C.c_int, [_vp, _vp, _fp, C.c_uint32, _fp, C.c_uint32]),
    "fx_set_particle_sort": (C.c_int, [_vp, C.POINTER(ParticleSort)]),
    "fx_get_particle_sort": (C.c_int, [_vp, C.POINTER(ParticleSort)]),
    "fx_sort_particles": (C.c_int, [_vp, _vp]),
    "fx_particle_sort_info": (C.c_int, [_vp, _vp, C.POINTER(ParticleSortInfo)]),
    "fx_particle_order_device": (C.c_int, [_vp, C.POINTER(_vp), C.POINTER(_vp)]),
    "fx_set_particle_trail": (C.c_int, [_vp, C.POINTER(ParticleTrail)]),
    "fx_get_particle_trail": (C.c_int, [_vp, C.POINTER(ParticleTrail)]),
    "fx_deposit_particles": (C.c_int, [_vp, _vp]),
    "fx_particle_density": (C.c_int, [_vp, _vp, C.POINTER(C.c_uint64), C.c_size_t]),
    "fx_set_particle_spawners": (C.c_int, [_vp, C.POINTER(ParticleSpawner), C.c_uint32]),
    "fx_get_particle_spawners": (C.c_int, [_vp, C.POINTER(ParticleSpawner), C.c_uint32, C.POINTER(C.c_uint32)]),
    "fx_spawn_particles": (C.c_int, [_vp, _vp]),
    "fx_particle_spawn_info": (C.c_int, [_vp, _vp, C.POINTER(ParticleSpawnInfo)]),
    "fx_set_particle_draw": (C.c_int, [_vp, C.POINTER(ParticleDraw)]),
    "fx_get_particle_draw": (C.c_int, [_vp, C.POINTER(ParticleDraw)]),
    "fx_draw_particles": (C.c_int, [_vp, _vp, C.c_uint8]),
    "fx_particle_splats": (C.c_int, [_vp, _vp, C.POINTER(C.c_uint64), C.c_size_t]),
    "fx_set_obstacle_draw": (C.c_int, [_vp, C.POINTER(ObstacleDraw)]),
    "fx_get_obstacle_draw": (C.c_int, [_vp, C.POINTER(ObstacleDraw)]),
    "fx_draw_obstacles": (C.c_int, [_vp, _vp, C.c_uint8, _vp]),
    "fx_obstacle_depth_device": (C.c_int, [_vp, C.POINTER(C.c_void_p)]),
    "fx_obstacle_hits": (C.c_int, [_vp, _vp, C.c_uint8, _vp, C.POINTER(C.c_uint64), C.POINTER(C.c_float), C.c_size_t]),
    "fx_set_open_walls": (C.c_int, [_vp, C.c_uint32]),
    "fx_get_open_walls": (C.c_int, [_vp, C.POINTER(C.c_uint32)]),
    "fx_open_inflow": (C.c_int, [_vp, _vp]),
    "fx_set_advection_scheme": (C.c_int, [_vp, C.c_uint32]),
    "fx_get_advection_scheme": (C.c_int, [_vp, C.POINTER(C.c_uint32)]),
    "fx_set_pressure_solver": (C.c_int, [_vp, C.POINTER(PressureSolver)]),
    "fx_get_pressure_solver": (C.c_int, [_vp, C.POINTER(PressureSolver)]),
    "fx_pressure_solve": (C.c_int, [_vp, _vp]),
    "fx_download_pressure_level": (C.c_int, [_vp, C.c_uint32, C.c_int, _vp, C.c_size_t]),
    "fx_sh_transform": (C.c_int, [_vp, _fp, C.c_uint32, _fp]),
    "fx_set_environment": (C.c_int, [_vp, _fp, C.c_uint32]),
    "fx_render_environment": (C.c_int, [_vp, _vp, C.c_uint8]),
    "fx_clear_render_target": (C.c_int, [_vp, _vp, _fp]),
    "fx_render_cube": (C.c_int, [_vp, _vp, C.c_uint8]),
    "fx_set_scene_depth": (C.c_int, [_vp, _vp, _vp, C.c_uint32, C.c_uint32, C.c_float, C.c_float, C.c_uint32]),
    "fx_set_light": (C.c_int, [_vp, C.POINTER(Light)]),
    "fx_get_light": (C.c_int, [_vp, C.POINTER(Light)]),
    "fx_dds_cube_info": (C.c_int, [_vp, C.c_size_t, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    "fx_dds_decode_cube": (C.c_int, [_vp, _vp, C.c_size_t, C.c_uint32, _fp, C.c_size_t]),
    "fx_timing_enable": (C.c_int, [_vp, C.c_int]),
    "fx_set_option": (C.c_int, [_vp, C.c_uint32, C.c_uint32]),
    "fx_set_knob": (C.c_int, [C.c_char_p, C.c_char_p]),
    "fx_knob_name": (C.c_char_p, [C.c_uint32]),
    "fx_comm_gather_color": (C.c_int, [_vp, _vp, _vp, C.c_int, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    "fx_timing_read": (C.c_int, [_vp, C.POINTER(Timing), C.c_int]),
    "fx_comm_id_bytes": (C.c_size_t, []),
    "fx_comm_get_unique_id": (C.c_int, [_vp, C.c_size_t]),
    "fx_comm_init_rank": (C.c_int, [_vp, _vp, C.c_size_t, C.c_int, C.c_int]),
    "fx_comm_init_local": (C.c_int, [C.POINTER(_vp), C.c_int]),
    "fx_comm_init_peer": (C.c_int, [C.POINTER(_vp), C.c_int]),
}

_lib = None
# the launcher switches that exist in lab builds only (fx_knobs.cpp, -DFX_LAB)
LAB_KNOBS = {"ADVECT_BLOCK", "ADVECT_FAST", "ADVECT_LDS_HALF", "ADVECT_TILE_ROWS", "ADVECT_ZCHUNK", "BLOCK_REMAP", "BLOCK_SHAPE", "DEBUG_NO_COPY",
             "FREEZE_DENSE_LEVELS", "FREEZE_DENSE_ONE", "FREEZE_FAST", "FREEZE_FUSE_DIV", "FREEZE_NT", "FREEZE_SHRINK", "FREEZE_T", "FREEZE_WGS",
             "JACOBI2D_TILE", "JACOBI_BLOCK", "JACOBI_BLOCKG", "LIGHT_FILL_DIRTY", "LIGHT_RAY_NT", "LIGHT_RAY_WGS", "OBSTACLE_V4", "PROJECT_V4", "PSORT_KEY_BITS", "ROW_VW",
             "STRIP3H_PAIRS", "STRIP3_COOP", "STRIP3_NO512", "STRIP3_OFF", "STRIP3_ZCHUNK", "STRIP4T", "STRIP4T_256", "STRIP4T_512", "STRIP4T_FROM", "STRIP4T_GRID", "STRIP4T_NARROW", "STRIP4T_NARROW_FROM", "STRIP4T_PIECES", "STRIP4X", "STRIP4X_MINP", "STRIP4X_NT", "STRIP4X_ORDER", "STRIP4X_WGS",
             "STRIP4_OCTET", "STRIP4_ZCHUNK", "STRIP4_ZFLOOR", "STRIP_GENERIC", "STRIP_R", "STRIP_REMAP", "STRIP_WGS", "STRIP_WIDE", "STRIP_ZCHUNK", "TRAIL_MERGE", "VIEW_ORDER", "VIEW_WGS", "VORT_ZCHUNK", "WIDE_OFFSETS", "XCD_REMAP"}


def lib_path():
    return _build.LIB


def load():
    """Load libfluidx_hip.so (building it first if a source is newer).  Raises on failure."""
    global _lib
    if _lib is not None:
        return _lib
    try:
        # A process that also uses torch must share ONE HIP runtime: torch bundles its own
        # libamdhip64 and must be imported before this library resolves the same soname.
        import torch  # noqa: F401
    except Exception:  # torch is plumbing, not a requirement
        pass
    path = _build.ensure_built()
    if os.environ.get("FLUIDX_LIB_PATH"):          # a lab build of the library (build.build_variant): tools, and tests/conftest.py `knob` while a test runs on the lab build; bench.py never sets it
        path = os.environ["FLUIDX_LIB_PATH"]
    if not os.path.exists(path):
        raise RuntimeError("libfluidx_hip.so is missing and could not be built")
    lib = C.CDLL(path, mode=C.RTLD_GLOBAL)
    # the version first: an older library lacks symbols, and "ABI version 5, this harness speaks 6" says more than an AttributeError
    lib.fx_abi_version.restype, lib.fx_abi_version.argtypes = C.c_int, []
    have = lib.fx_abi_version()
    if have != ABI_VERSION:
        raise RuntimeError("fluidx ABI version mismatch: %s speaks version %d, this harness version %d" % (path, have, ABI_VERSION))
    for name, (res, args) in SYMBOLS.items():
        fn = getattr(lib, name)          # AttributeError if the ABI lost a symbol
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    # the launcher switches (fx_set_knob) are process-wide values inside the library, which reads no environment for them; the tools'
    # habit of `FLUIDX_<NAME>=... python tools/...` is served here, once, by the harness
    offered = knob_names()
    for name in offered:
        v = os.environ.get("FLUIDX_" + name)
        if v is not None:
            set_knob(name, v)
    # ... and a tool that asks for a lab switch on the shipped library is told so instead of measuring the default twice
    import sys
    for k in os.environ:
        if k.startswith("FLUIDX_") and k[7:] in LAB_KNOBS and k[7:] not in offered:
            sys.stderr.write("fluidx12_amd: %s is a lab-build switch (FLUIDX_BUILD_LAB=1 python -m fluidx12_amd.build); this library ignores it\n" % k)
    return lib


def knob_names():
    lib, out, i = load(), [], 0
    while True:
        n = lib.fx_knob_name(i)
        if n is None:
            return out
        out.append(n.decode())
        i += 1


def set_knob(name, value):
    """a measurement switch of the kernel launchers (include/fluidx_hip.h fx_set_knob); value None = back to the default"""
    check(load().fx_set_knob(name.encode(), None if value is None else str(value).encode()), "set_knob(%s)" % name)


class FluidxError(RuntimeError):
    def __init__(self, status, where):
        self.status = status
        msg = load().fx_error_string(status).decode()
        super().__init__("%s failed: %s (%d)" % (where, msg, status))


def check(status, where):
    if status != FX_OK:
        raise FluidxError(status, where)
