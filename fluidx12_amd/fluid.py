"""Host-side mirror of the reference's operator surface for the hot path, over the C ABI.

`Fluid` keeps the method names, argument meaning and error behaviour of
/root/reference/FluidX12/Content/Fluid.h:20-35 (Init returns bool, the rest return None and
raise only on ABI failure); `LightProbe` mirrors the SH side of Content/LightProbe.h:16-26.
The XUSG arguments that have no HIP meaning (descriptor-table lib, uploaders, RT/DS formats)
are dropped; `CommandList*` becomes an optional HIP stream handle (int / None).

This module only marshals: all arithmetic happens in libfluidx_hip.so.
"""
import ctypes as C
import os

import numpy as np

from . import capi


def look_at_lh(eye, focus, up):
    """XMMatrixLookAtLH (row-vector convention), as used at FluidX12/FluidX12.cpp:252."""
    eye, focus, up = (np.asarray(v, np.float32) for v in (eye, focus, up))
    z = focus - eye
    z = z / np.float32(np.sqrt(np.dot(z, z)))
    x = np.cross(up, z).astype(np.float32)
    x = x / np.float32(np.sqrt(np.dot(x, x)))
    y = np.cross(z, x).astype(np.float32)
    m = np.zeros((4, 4), np.float32)
    m[:3, 0], m[:3, 1], m[:3, 2] = x, y, z
    m[3, :3] = [-np.dot(x, eye), -np.dot(y, eye), -np.dot(z, eye)]
    m[3, 3] = 1.0
    return m


def perspective_fov_lh(fovy, aspect, zn, zf):
    """XMMatrixPerspectiveFovLH, as used at FluidX12/FluidX12.cpp:244."""
    h = np.float32(np.cos(0.5 * fovy) / np.sin(0.5 * fovy))
    w = np.float32(h / np.float32(aspect))
    q = np.float32(zf / (zf - zn))
    m = np.zeros((4, 4), np.float32)
    m[0, 0], m[1, 1], m[2, 2], m[2, 3], m[3, 2] = w, h, q, 1.0, -q * np.float32(zn)
    return m


def default_camera(width, height):
    """The demo driver's camera (FluidX12.cpp:243-253): eye (4,16,-40) -> origin, FOV pi/4, z 1..1000."""
    eye = np.array([4.0, 16.0, -40.0], np.float32)
    view = look_at_lh(eye, [0, 0, 0], [0, 1, 0])
    proj = perspective_fov_lh(np.float32(np.pi) / np.float32(4.0), width / float(height), 1.0, 1000.0)
    return view, proj, eye


def _fp(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


class Fluid:
    """class Fluid (Content/Fluid.h:9-128) on HIP."""

    RAY_MARCH_DIRECT = capi.RAY_MARCH_DIRECT
    RAY_MARCH_CUBEMAP = capi.RAY_MARCH_CUBEMAP
    SEPARATE_LIGHT_PASS = capi.SEPARATE_LIGHT_PASS
    OPTIMIZED = capi.OPTIMIZED
    FrameCount = capi.FRAME_COUNT

    def __init__(self):
        self._lib = capi.load()
        self._ctx = C.c_void_p()
        self.grid = None
        self.slab = None
        self.last_status = capi.FX_OK

    # ---- Fluid::Init (Fluid.cpp:189-270) ----------------------------------------------------------
    def Init(self, width, height, gridSize, *, storage="fp32", jacobi_iters=40, jacobi_mode="fixed",
             advect_address="clamp", device=-1, slab=None, halo_advect=0, halo_jacobi=0, jacobi_fuse=0, overlap=2,
             render_only=False):
        if self._ctx:
            self.Release()
        X, Y, Z = (int(v) for v in gridSize)
        d = capi.Desc()
        d.struct_size = C.sizeof(capi.Desc)
        d.grid_x, d.grid_y, d.grid_z = X, Y, Z
        d.viewport_w, d.viewport_h = int(width), int(height)
        d.storage = {"fp32": capi.STORAGE_FP32, "fp16": capi.STORAGE_FP16}[storage]
        d.jacobi_iters = int(jacobi_iters)
        d.jacobi_mode = {"fixed": capi.JACOBI_FIXED, "faithful": capi.JACOBI_FAITHFUL}[jacobi_mode]
        d.advect_address = {"clamp": capi.ADDRESS_CLAMP, "mirror": capi.ADDRESS_MIRROR}[advect_address]
        d.device = int(device)
        if slab is not None:
            d.slab_z0, d.slab_nz = int(slab[0]), int(slab[1])
        d.halo_advect, d.halo_jacobi = int(halo_advect), int(halo_jacobi)
        level = 2 if overlap is True else int(overlap)        # 0 none, 1 advection halo only, 2 (default) + pressure rounds, 3 + early colour halo
        d.flags = (int(jacobi_fuse) & 0xF) | (0 if level else capi.FLAG_NO_OVERLAP) | (capi.FLAG_RENDER_ONLY if render_only else 0)
        self.last_status = self._lib.fx_create(C.byref(self._ctx), C.byref(d))
        if self.last_status != capi.FX_OK:      # the reference's Init returns false (XUSG_N_RETURN)
            self._ctx = C.c_void_p()
            return False
        self.grid = (X, Y, Z)
        self.viewport = (int(width), int(height))
        self.slab = (d.slab_z0, d.slab_nz if d.slab_nz else Z)
        if level in (1, 3):
            self.set_option(capi.OPT_OVERLAP, level)
        return True

    def Release(self):
        if self._ctx:
            self._lib.fx_destroy(self._ctx)
            self._ctx = C.c_void_p()

    def __del__(self):
        try:
            self.Release()
        except Exception:
            pass

    def _need(self):
        if not self._ctx:
            raise capi.FluidxError(capi.FX_E_STATE, "Fluid (Init not called)")

    # ---- Fluid.h:28-33 ----------------------------------------------------------------------------
    def SetMaxSamples(self, maxRaySamples, maxLightSamples):
        self._need()
        capi.check(self._lib.fx_set_max_samples(self._ctx, maxRaySamples, maxLightSamples), "SetMaxSamples")

    def SetSH(self, coeffSH):
        self._need()
        if coeffSH is None:
            capi.check(self._lib.fx_set_sh(self._ctx, None), "SetSH")
            return
        c = np.ascontiguousarray(coeffSH, np.float32).reshape(27)
        capi.check(self._lib.fx_set_sh(self._ctx, _fp(c)), "SetSH")

    def UpdateFrame(self, timeStep, frameIndex, view=None, proj=None, eyePt=None):
        self._need()
        if view is None:
            capi.check(self._lib.fx_update_frame(self._ctx, timeStep, frameIndex, None, None, None), "UpdateFrame")
            return
        v = np.ascontiguousarray(view, np.float32).reshape(16)
        p = np.ascontiguousarray(proj, np.float32).reshape(16)
        e = np.ascontiguousarray(eyePt, np.float32).reshape(3)
        capi.check(self._lib.fx_update_frame(self._ctx, timeStep, frameIndex, _fp(v), _fp(p), _fp(e)), "UpdateFrame")

    def Simulate(self, frameIndex=0, stream=None):
        self._need()
        capi.check(self._lib.fx_simulate(self._ctx, stream, frameIndex), "Simulate")

    def Render(self, frameIndex=0, flags=capi.OPTIMIZED, stream=None, to_target=False):
        """Fluid::Render (Fluid.cpp:412-446).  to_target=True also runs renderCube (Fluid.cpp:430), which the reference
        always does: the cube map is resolved onto the render target (ClearRenderTarget first, as the caller does)."""
        self._need()
        capi.check(self._lib.fx_render(self._ctx, stream, frameIndex, flags), "Render")
        if to_target and (flags & capi.RAY_MARCH_CUBEMAP):     # the direct modes write the target themselves
            self.RenderCube(frameIndex, stream)

    def ClearRenderTarget(self, rgba=(0.2, 0.2, 0.2, 0.0), stream=None):
        """ClearRenderTargetView with the demo's clear colour (FluidX12.cpp:471-472)"""
        self._need()
        c = (C.c_float * 4)(*[float(v) for v in rgba])
        capi.check(self._lib.fx_clear_render_target(self._ctx, stream, c), "ClearRenderTarget")

    def SetEnvironment(self, radiance_cube):
        """the radiance cube float[6][n][n][3] the sky pass draws (None releases it)"""
        self._need()
        if radiance_cube is None:
            capi.check(self._lib.fx_set_environment(self._ctx, None, 0), "SetEnvironment")
            return
        a = np.ascontiguousarray(radiance_cube, np.float32)
        if a.ndim != 4 or a.shape[0] != 6 or a.shape[1] != a.shape[2] or a.shape[3] != 3:
            raise ValueError("radiance cube must be float[6][n][n][3]")
        capi.check(self._lib.fx_set_environment(self._ctx, _fp(a), a.shape[1]), "SetEnvironment")

    def RenderEnvironment(self, frameIndex=0, stream=None):
        """LightProbe::RenderEnvironment (LightProbe.cpp:85-97): the sky onto the render target, before the volume"""
        self._need()
        capi.check(self._lib.fx_render_environment(self._ctx, stream, frameIndex), "RenderEnvironment")

    def RenderCube(self, frameIndex=0, stream=None):
        """Fluid::renderCube (Fluid.cpp:910-931), raster-free: PSRayCastCube per pixel + PREMULTIPLIED blend"""
        self._need()
        capi.check(self._lib.fx_render_cube(self._ctx, stream, frameIndex), "RenderCube")

    def SetSceneDepth(self, depth, z_near=1.0, z_far=1000.0, stream=None):
        """the scene's depth buffer for the following renders (the reference's _HAS_DEPTH_MAP_ variants, fx_set_scene_depth):
        float32[viewport_h][viewport_w], 0 = near plane, 1 = far plane, under the projection given to UpdateFrame, whose planes are
        z_near / z_far.  A numpy array is copied; an object with data_ptr() on the device (a torch tensor) is read in place by every
        later render -- this object keeps a reference to it.  None detaches."""
        self._need()
        if depth is None:
            self._depth_ref = None
            capi.check(self._lib.fx_set_scene_depth(self._ctx, stream, None, 0, 0, 0.0, 0.0, 0), "SetSceneDepth")
            return
        w, h = self.viewport
        if hasattr(depth, "data_ptr") and getattr(getattr(depth, "device", None), "type", "cpu") != "cpu":
            if tuple(depth.shape) != (h, w) or str(depth.dtype) != "torch.float32" or not depth.is_contiguous():
                raise ValueError("device depth must be a contiguous float32[%d][%d]" % (h, w))
            capi.check(self._lib.fx_set_scene_depth(self._ctx, stream, C.c_void_p(depth.data_ptr()), w, h, float(z_near), float(z_far),
                                                     capi.DEPTH_DEVICE), "SetSceneDepth")
            self._depth_ref = depth
            return
        a = np.ascontiguousarray(depth, np.float32)
        if a.shape != (h, w):
            raise ValueError("depth must be float32[%d][%d], got %s" % (h, w, a.shape))
        capi.check(self._lib.fx_set_scene_depth(self._ctx, stream, a.ctypes.data_as(C.c_void_p), w, h, float(z_near), float(z_far), 0),
                   "SetSceneDepth")
        self._depth_ref = None

    def SetLight(self, position, kind="directional", color=None, ambient=None):
        """the scene light of the following renders (fx_set_light).  position: world space of UpdateFrame's view matrix (the volume is
        [-10, 10]^3 there); kind "directional": only its direction matters, "point": the light's place -- shadow rays run to it and end
        there.  color / ambient: (r, g, b, intensity); None keeps the current one.  SetLight(None): the reference's constants again.
        Render state: kept across UpdateFrame, not stored in checkpoints."""
        self._need()
        if position is None:
            capi.check(self._lib.fx_set_light(self._ctx, None), "SetLight")
            return
        l = capi.Light()
        capi.check(self._lib.fx_get_light(self._ctx, C.byref(l)), "SetLight")
        l.struct_size = C.sizeof(capi.Light)
        l.kind = {"directional": capi.LIGHT_DIRECTIONAL, "point": capi.LIGHT_POINT}[kind]
        l.position = (C.c_float * 3)(*[float(v) for v in position])
        if color is not None:
            l.color = (C.c_float * 4)(*[float(v) for v in color])
        if ambient is not None:
            l.ambient = (C.c_float * 4)(*[float(v) for v in ambient])
        capi.check(self._lib.fx_set_light(self._ctx, C.byref(l)), "SetLight")

    def GetLight(self):
        """the light in force (fx_get_light): {"kind", "position", "color", "ambient"}"""
        self._need()
        l = capi.Light()
        capi.check(self._lib.fx_get_light(self._ctx, C.byref(l)), "GetLight")
        return {"kind": "point" if l.kind == capi.LIGHT_POINT else "directional", "position": tuple(l.position), "color": tuple(l.color),
                "ambient": tuple(l.ambient)}

    # ---- the demo driver's time-step rule (FluidX12.cpp:266) ---------------------------------------
    def default_time_step(self):
        X, Y, Z = self.grid
        return (2.0 if Z > 1 else 1.0) / Y

    # ---- stages / access (no reference counterpart) ---------------------------------------------------
    def Synchronize(self):
        self._need()
        rc = self._lib.fx_synchronize(self._ctx)
        if rc != capi.FX_OK:                       # what the library had to say beyond the status (fx_last_error)
            note = self.last_error
            capi.check(rc, "Synchronize" + (" [%s]" % note if note else ""))

    @property
    def last_error(self):
        self._need()
        e = self._lib.fx_last_error(self._ctx)
        return e.decode() if e else ""

    def Advect(self, stream=None):
        capi.check(self._lib.fx_advect(self._ctx, stream), "Advect")

    def SetVorticityConfinement(self, eps):
        """strength of the vorticity confinement pass between advection and divergence (fx_set_vorticity_confinement); 0 = off (default).
        Configuration: kept across UpdateFrame, not stored in checkpoints.  Whole-grid contexts only."""
        self._need()
        capi.check(self._lib.fx_set_vorticity_confinement(self._ctx, float(eps)), "SetVorticityConfinement")

    def ConfineVorticity(self, stream=None):
        """the confinement stage alone, on VELOCITY1 (fx_confine_vorticity); VELOCITY is unspecified afterwards until the next Project"""
        self._need()
        capi.check(self._lib.fx_confine_vorticity(self._ctx, stream), "ConfineVorticity")

    def SetEmitters(self, emitters):
        """the smoke sources applied behind every advection (fx_set_emitters): a sequence of dicts (or capi.Emitter) with "center" (x, y, z) and
        "radius" in the simulation's texture space [0, 1]^3, and optionally "color_rate" (r, g, b, a per unit time; default the built-in's
        8, 16, 40, 40), "force" (default the built-in's lift: (0, 192, 0), 2-D grids (0, 48, 0)) and "swirl" (default 200; ignored in 2-D).
        None or () = none (default).  Configuration: kept across UpdateFrame, not stored in checkpoints.  Whole-grid contexts only."""
        self._need()
        items = list(emitters or ())
        arr = (capi.Emitter * max(len(items), 1))()
        is3d = self.grid[2] > 1
        for k, e in enumerate(items):
            if isinstance(e, capi.Emitter):
                arr[k] = e
                continue
            arr[k].struct_size, arr[k].flags = C.sizeof(capi.Emitter), int(e.get("flags", 0))
            arr[k].center = (C.c_float * 3)(*[float(v) for v in e["center"]])
            arr[k].radius = float(e["radius"])
            arr[k].color_rate = (C.c_float * 4)(*[float(v) for v in e.get("color_rate", (8.0, 16.0, 40.0, 40.0))])
            arr[k].force = (C.c_float * 3)(*[float(v) for v in e.get("force", (0.0, 192.0 if is3d else 48.0, 0.0))])
            arr[k].swirl = float(e.get("swirl", 200.0))
        capi.check(self._lib.fx_set_emitters(self._ctx, arr if items else None, len(items)), "SetEmitters")

    def GetEmitters(self):
        """the list in force (fx_get_emitters), as dicts with the keys SetEmitters takes"""
        self._need()
        n = C.c_uint32(0)
        arr = (capi.Emitter * capi.MAX_EMITTERS)()
        capi.check(self._lib.fx_get_emitters(self._ctx, arr, capi.MAX_EMITTERS, C.byref(n)), "GetEmitters")
        return [{"center": tuple(e.center), "radius": e.radius, "color_rate": tuple(e.color_rate), "force": tuple(e.force), "swirl": e.swirl,
                 "flags": e.flags} for e in arr[:n.value]]

    def SetImpulse(self, enabled):
        """the reference's built-in source inside the advection (fx_set_impulse); default on.  Off: the emitters are the only sources"""
        self._need()
        capi.check(self._lib.fx_set_impulse(self._ctx, 1 if enabled else 0), "SetImpulse")

    def Emit(self, stream=None):
        """the emitter stage alone, in place on VELOCITY1 and COLOR (fx_emit); Advect does not include it"""
        self._need()
        capi.check(self._lib.fx_emit(self._ctx, stream), "Emit")

    def SetObstacles(self, mask, stream=None):
        """voxelised solid obstacles the smoke flows around (fx_set_obstacles): `mask` is anything numpy takes as an array of grid shape
        (Z, Y, X) -- or X * Y * Z values in that order --, non-zero = solid; a torch tensor on the context's device is read in place; None
        detaches.  Replaces the previous mask.  Configuration: kept across UpdateFrame, not stored in checkpoints.  Whole-grid, fixed-mode contexts only."""
        self._need()
        if mask is None:
            capi.check(self._lib.fx_set_obstacles(self._ctx, stream, None, 0, 0), "SetObstacles")
            return
        if hasattr(mask, "data_ptr") and getattr(mask, "is_cuda", False):
            import torch
            t = (mask != 0).to(dtype=torch.uint8).contiguous()
            torch.cuda.current_stream(t.device).synchronize()      # the tensor was made on torch's stream, the library reads it on its own
            capi.check(self._lib.fx_set_obstacles(self._ctx, stream, t.data_ptr(), t.numel(), capi.OBSTACLES_DEVICE), "SetObstacles")
            return
        m = np.ascontiguousarray(np.asarray(mask) != 0, dtype=np.uint8)
        capi.check(self._lib.fx_set_obstacles(self._ctx, stream, m.ctypes.data, m.size, 0), "SetObstacles")

    def GetObstacles(self):
        """(mask uint8 (Z, Y, X) of 0 / 1, solid cells) in force (fx_get_obstacles); all 0 when none"""
        self._need()
        X, Y, Z = self.grid
        m = np.empty((Z, Y, X), np.uint8)
        n = C.c_uint64(0)
        capi.check(self._lib.fx_get_obstacles(self._ctx, m.ctypes.data, m.size, C.byref(n)), "GetObstacles")
        return m, int(n.value)

    def EnforceObstacles(self, stream=None):
        """the enforce stage alone, in place on VELOCITY1 and COLOR (fx_enforce_obstacles); Advect does not include it"""
        self._need()
        capi.check(self._lib.fx_enforce_obstacles(self._ctx, stream), "EnforceObstacles")

    def SetObstacleBodies(self, bodies):
        """the rigid-body velocities of the solids under the mask (fx_set_obstacle_bodies): a sequence of dicts (or capi.ObstacleBody) with
        "box_lo" and "box_hi" (x, y, z) in texture space [0, 1]^3 -- the solid cells whose centre lies in the closed box belong to the body,
        the first body in list order wins -- and optionally "linear" (the pivot's velocity, texture units per unit time), "angular" (radians
        per unit time about the pivot) and "pivot" (default: the box's centre); a missing vector is zero.  None or () = every solid rests
        (default).  Takes effect while a mask is set (SetObstacles), in either order.  Configuration: kept across UpdateFrame, not stored
        in checkpoints.  Whole-grid, fixed-mode contexts only."""
        self._need()
        items = list(bodies or ())
        arr = (capi.ObstacleBody * max(len(items), 1))()
        for k, b in enumerate(items):
            if isinstance(b, capi.ObstacleBody):
                arr[k] = b
                continue
            lo, hi = [float(v) for v in b["box_lo"]], [float(v) for v in b["box_hi"]]
            arr[k].struct_size, arr[k].flags = C.sizeof(capi.ObstacleBody), int(b.get("flags", 0))
            arr[k].box_lo, arr[k].box_hi = (C.c_float * 3)(*lo), (C.c_float * 3)(*hi)
            arr[k].linear = (C.c_float * 3)(*[float(v) for v in b.get("linear", (0.0, 0.0, 0.0))])
            arr[k].angular = (C.c_float * 3)(*[float(v) for v in b.get("angular", (0.0, 0.0, 0.0))])
            arr[k].pivot = (C.c_float * 3)(*[float(v) for v in b.get("pivot", [0.5 * (l + h) for l, h in zip(lo, hi)])])
        capi.check(self._lib.fx_set_obstacle_bodies(self._ctx, arr if items else None, len(items)), "SetObstacleBodies")

    def SetObstacleMeshes(self, meshes, stream=None):
        """the obstacle mask from closed triangle meshes, voxelised on the device (fx_set_obstacle_meshes): a sequence of
        (positions, indices, transform or None) -- positions (n, 3) float32 in texture space, indices (m, 3) uint32, transform 12 floats
        (row-major 3 x 4) -- as anything numpy takes as an array, or, all three of a mesh, as torch tensors on the context's device (float32 /
        int32 or uint32 / float32), which are read in place.  The mask is the union of the meshes' solid sets and replaces the previous mask as
        SetObstacles would; a rigidly moving object is a new call with a new transform.  -> {"solid_cells", "open_columns" (0 for watertight
        meshes), "skipped_triangles" (an index out of range, a non-finite position)}.  Whole-grid, fixed-mode 3-D contexts only."""
        self._need()
        items = list(meshes)
        arr = (capi.ObstacleMesh * max(len(items), 1))()
        keep = []                                                       # the arrays behind the pointers, alive until the call returns
        for k, (pos, idx, xf) in enumerate(items):
            arr[k].struct_size = C.sizeof(capi.ObstacleMesh)
            if hasattr(pos, "data_ptr") and getattr(pos, "is_cuda", False):
                import torch
                p = pos.to(torch.float32).contiguous().reshape(-1, 3)
                if idx.dtype not in (torch.int32, getattr(torch, "uint32", torch.int32)) or not idx.is_cuda:
                    raise TypeError("SetObstacleMeshes: a device mesh takes its indices as an int32 or uint32 tensor on the same device")
                i = idx.contiguous().reshape(-1, 3)
                x = None if xf is None else xf.to(torch.float32).contiguous().reshape(12)
                if x is not None and not x.is_cuda:
                    raise TypeError("SetObstacleMeshes: a device mesh takes its transform as a tensor on the same device")
                keep.append((p, i, x))
                arr[k].flags = capi.MESH_DEVICE
                arr[k].positions, arr[k].indices = p.data_ptr() or None, i.data_ptr() or None
                arr[k].vertex_count, arr[k].triangle_count = p.shape[0], i.shape[0]
                arr[k].transform = None if x is None else x.data_ptr()
                continue
            p = np.ascontiguousarray(np.asarray(pos, np.float32).reshape(-1, 3))
            i = np.ascontiguousarray(np.asarray(idx).astype(np.uint32, copy=False).reshape(-1, 3))
            x = None if xf is None else np.ascontiguousarray(np.asarray(xf, np.float32).reshape(12))
            keep.append((p, i, x))
            arr[k].flags = 0
            arr[k].positions, arr[k].indices = (p.ctypes.data if p.size else None), (i.ctypes.data if i.size else None)
            arr[k].vertex_count, arr[k].triangle_count = p.shape[0], i.shape[0]
            arr[k].transform = None if x is None else x.ctypes.data
        rep = capi.MeshReport()
        capi.check(self._lib.fx_set_obstacle_meshes(self._ctx, stream, arr if items else None, len(items), C.byref(rep)), "SetObstacleMeshes")
        return {"solid_cells": int(rep.solid_cells), "open_columns": int(rep.open_columns), "skipped_triangles": int(rep.skipped_triangles)}

    def GetObstacleBodies(self):
        """the list in force (fx_get_obstacle_bodies), as dicts with the keys SetObstacleBodies takes"""
        self._need()
        n = C.c_uint32(0)
        arr = (capi.ObstacleBody * capi.MAX_OBSTACLE_BODIES)()
        capi.check(self._lib.fx_get_obstacle_bodies(self._ctx, arr, capi.MAX_OBSTACLE_BODIES, C.byref(n)), "GetObstacleBodies")
        return [{"box_lo": tuple(b.box_lo), "box_hi": tuple(b.box_hi), "linear": tuple(b.linear), "angular": tuple(b.angular),
                 "pivot": tuple(b.pivot), "flags": b.flags} for b in arr[:n.value]]

    def SetObstacleDraw(self, albedo, flags=0):
        """the obstacle draw (fx_set_obstacle_draw): DrawObstacles then ray-casts the solid cells of the mask in force into the render target,
        each visible face lit by the light of SetLight and coloured `albedo` (r, g, b, intensity), and into a depth buffer for
        AttachObstacleDepth.  Allocates that buffer and one uint64 per 4 x 4 x 4 cells.  SetObstacleDraw(None) switches it off (the default)
        and frees both -- detach the depth first.  Configuration: kept across UpdateFrame, not stored in checkpoints.  Whole 3-D grids with
        a viewport only."""
        self._need()
        if albedo is None:
            capi.check(self._lib.fx_set_obstacle_draw(self._ctx, None), "SetObstacleDraw")
            return
        d = capi.ObstacleDraw()
        d.struct_size, d.flags = C.sizeof(capi.ObstacleDraw), int(flags)
        d.albedo = (C.c_float * 4)(*[float(v) for v in albedo])
        capi.check(self._lib.fx_set_obstacle_draw(self._ctx, C.byref(d)), "SetObstacleDraw")

    def GetObstacleDraw(self):
        """the setting in force (fx_get_obstacle_draw): {"albedo", "flags"}; off: albedo 0"""
        self._need()
        d = capi.ObstacleDraw()
        capi.check(self._lib.fx_get_obstacle_draw(self._ctx, C.byref(d)), "GetObstacleDraw")
        return {"albedo": tuple(d.albedo), "flags": d.flags}

    @staticmethod
    def _device_depth(scene_depth, w, h):
        """the device pointer of an optional caller's scene depth: None, an integer address, or a contiguous float32[h][w] torch tensor"""
        if scene_depth is None:
            return None
        if hasattr(scene_depth, "data_ptr"):
            if tuple(scene_depth.shape) != (h, w) or str(scene_depth.dtype) != "torch.float32" or not scene_depth.is_contiguous():
                raise ValueError("device depth must be a contiguous float32[%d][%d]" % (h, w))
            return C.c_void_p(scene_depth.data_ptr())
        return C.c_void_p(int(scene_depth))

    def ObstacleDepthPointer(self):
        """the device address of the draw's depth buffer, float32[H][W] (fx_obstacle_depth_device); None while the draw is off"""
        self._need()
        p = C.c_void_p()
        capi.check(self._lib.fx_obstacle_depth_device(self._ctx, C.byref(p)), "ObstacleDepthPointer")
        return p.value

    def DrawObstacles(self, frameIndex=0, scene_depth=None, stream=None):
        """the solids onto the render target and into the draw's depth buffer (fx_draw_obstacles), before Render, with the camera of the last
        UpdateFrame; FIELD_TARGET_FLOAT then holds (colour, 1) per drawn pixel.  scene_depth: the caller's own scene, a float32[H][W] torch
        tensor on the context's device (or its address); a solid behind it is not drawn.  Enqueues only"""
        self._need()
        w, h = self.viewport
        capi.check(self._lib.fx_draw_obstacles(self._ctx, stream, frameIndex, self._device_depth(scene_depth, w, h)), "DrawObstacles")

    def AttachObstacleDepth(self, z_near=1.0, z_far=1000.0, stream=None):
        """the draw's depth buffer as the scene depth of the following renders (fx_set_scene_depth, FX_DEPTH_DEVICE): the marches end at
        the solids, DrawParticles culls what lies behind them.  Read in place: every DrawObstacles on the same stream refreshes it.
        SetSceneDepth(None) detaches"""
        self._need()
        p = self.ObstacleDepthPointer()
        if not p:
            raise capi.FluidxError(capi.FX_E_STATE, "AttachObstacleDepth")
        w, h = self.viewport
        capi.check(self._lib.fx_set_scene_depth(self._ctx, stream, C.c_void_p(p), w, h, float(z_near), float(z_far), capi.DEPTH_DEVICE),
                   "AttachObstacleDepth")
        self._depth_ref = None

    def ObstacleHits(self, frameIndex=0, scene_depth=None, stream=None):
        """the cast alone (fx_obstacle_hits; blocks) -> (uint64[H][W], float32[H][W]): per pixel the hits word -- bit 63 = the walk hit,
        bit 62 = drawn, bits 32-34 = the face (2 axis + (step > 0); 6 = the eye's own cell), bits 0-31 = the cell (z Y + y) X + x -- and
        the depth DrawObstacles would store"""
        self._need()
        w, h = self.viewport
        hits, depth = np.empty((h, w), np.uint64), np.empty((h, w), np.float32)
        capi.check(self._lib.fx_obstacle_hits(self._ctx, stream, frameIndex, self._device_depth(scene_depth, w, h),
                                              hits.ctypes.data_as(C.POINTER(C.c_uint64)), _fp(depth), hits.size), "ObstacleHits")
        return hits, depth

    def SetOpenWalls(self, faces):
        """the faces of the box through which the smoke leaves (fx_set_open_walls): a set of capi.WALL_* bits, 0 = all closed (default).  Beyond
        an open face the pressure is 0, the smoke is clear air and the temperature ambient; the projection does not damp flow towards it.
        Configuration: kept across UpdateFrame, not stored in checkpoints.  Whole-grid, fixed-mode contexts only; no z face on a 2-D grid."""
        self._need()
        capi.check(self._lib.fx_set_open_walls(self._ctx, int(faces)), "SetOpenWalls")

    def GetOpenWalls(self):
        """the setting in force (fx_get_open_walls)"""
        self._need()
        faces = C.c_uint32(0)
        capi.check(self._lib.fx_get_open_walls(self._ctx, C.byref(faces)), "GetOpenWalls")
        return int(faces.value)

    def OpenInflow(self, stream=None):
        """the inflow stage alone, in place on COLOR (fx_open_inflow): run it directly behind Advect; Advect does not include it"""
        self._need()
        capi.check(self._lib.fx_open_inflow(self._ctx, stream), "OpenInflow")

    def SetAdvectionScheme(self, scheme):
        """the advection scheme (fx_set_advection_scheme): "semi-lagrangian" (the reference's, default) or "maccormack" (Selle et al. 2008: a
        predictor and a corrector launch, second order, limited to the back-trace's taps), or the capi.ADVECT_* value.  Simulate and Advect follow
        it; the temperature of SetBuoyancy stays semi-Lagrangian.  Configuration: kept across UpdateFrame, not stored in checkpoints (set it
        again after LoadCheckpoint).  Whole-grid contexts only."""
        self._need()
        if isinstance(scheme, str):
            names = {"semi-lagrangian": capi.ADVECT_SEMI_LAGRANGIAN, "maccormack": capi.ADVECT_MACCORMACK}
            if scheme.lower() not in names:
                raise ValueError("unknown advection scheme %r" % (scheme,))
            scheme = names[scheme.lower()]
        capi.check(self._lib.fx_set_advection_scheme(self._ctx, int(scheme)), "SetAdvectionScheme")

    def GetAdvectionScheme(self):
        """the capi.ADVECT_* value in force (fx_get_advection_scheme)"""
        self._need()
        scheme = C.c_uint32(0)
        capi.check(self._lib.fx_get_advection_scheme(self._ctx, C.byref(scheme)), "GetAdvectionScheme")
        return int(scheme.value)

    def SetPressureSolver(self, kind="multigrid", cycles=2, pre_sweeps=2, post_sweeps=2, coarse_sweeps=16, max_levels=0, omega=None, flags=0):
        """the pressure solver of Simulate and PressureSolve (fx_set_pressure_solver): "jacobi" (the default: jacobi_iters sweeps) or "multigrid"
        (`cycles` V(pre_sweeps, post_sweeps) cycles of damped Jacobi, coarse_sweeps on the coarsest level, at most max_levels levels, 0 = as many
        as the grid allows), or the capi.PRESSURE_* value.  omega: the damping, default 6/7 in 3-D and 4/5 in 2-D.  flags: capi.MG_NO_TAIL.
        Jacobi(iters) stays plain Jacobi.  Configuration: kept across UpdateFrame, not stored in checkpoints (set it again after LoadCheckpoint).
        Whole-grid contexts in fixed mode with closed walls and no obstacles only."""
        self._need()
        if isinstance(kind, str):
            names = {"jacobi": capi.PRESSURE_JACOBI, "multigrid": capi.PRESSURE_MULTIGRID}
            if kind.lower() not in names:
                raise ValueError("unknown pressure solver %r" % (kind,))
            kind = names[kind.lower()]
        if int(kind) == capi.PRESSURE_JACOBI:
            capi.check(self._lib.fx_set_pressure_solver(self._ctx, None), "SetPressureSolver")
            return
        if omega is None:
            omega = 6.0 / 7.0 if self.grid[2] > 1 else 4.0 / 5.0
        ps = capi.PressureSolver(int(kind), int(flags), int(cycles), int(pre_sweeps), int(post_sweeps), int(coarse_sweeps), int(max_levels), float(omega))
        capi.check(self._lib.fx_set_pressure_solver(self._ctx, C.byref(ps)), "SetPressureSolver")

    def GetPressureSolver(self):
        """the setting in force as a dict (fx_get_pressure_solver); "max_levels" holds the levels in use"""
        self._need()
        ps = capi.PressureSolver()
        capi.check(self._lib.fx_get_pressure_solver(self._ctx, C.byref(ps)), "GetPressureSolver")
        return {name: getattr(ps, name) for name, _ in capi.PressureSolver._fields_}

    def PressureSolve(self, stream=None):
        """the solver stage alone, between Divergence and Project (fx_pressure_solve): jacobi_iters Jacobi sweeps or the multigrid cycles"""
        self._need()
        capi.check(self._lib.fx_pressure_solve(self._ctx, stream), "PressureSolve")

    def _pressure_level_shape(self, level):
        """(Z, Y, X) of a level the solver in force has"""
        level = int(level)
        if not 0 <= level < self.GetPressureSolver()["max_levels"]:
            raise ValueError("pressure level %d: the solver in force has %d" % (level, self.GetPressureSolver()["max_levels"]))
        X, Y, Z = self.grid
        for _ in range(level):
            X, Y, Z = X // 2, Y // 2, (Z // 2 if self.grid[2] > 1 else 1)
        return (Z, Y, X)

    def DownloadPressureLevel(self, level, what=0):
        """what = 0: the solution (level 0) or the correction the last solve left on `level`; 1: its right-hand side (fx_download_pressure_level)"""
        self._need()
        out = np.empty(self._pressure_level_shape(level), np.float32)
        capi.check(self._lib.fx_download_pressure_level(self._ctx, int(level), int(what), out.ctypes.data_as(C.c_void_p), out.nbytes), "DownloadPressureLevel")
        return out

    def SetBuoyancy(self, ambient=0.0, density_weight=0.0, lift=0.0, cooling=0.0, up=(0.0, 1.0, 0.0), flags=0):
        """buoyancy (fx_set_buoyancy): a temperature field advected with the flow, cooling towards `ambient` by max(1 - cooling * dt, 0) per step,
        and the force (-density_weight * COLOR.w + lift * (T - ambient)) * up on VELOCITY1, one pass behind the emitters.  `up` is used as given.
        SetBuoyancy(None) switches it off (default) and frees the field; the first call that switches it on fills the field with `ambient`, a
        later one replaces the coefficients and keeps it.  The field is FIELD_TEMPERATURE (upload / download while on).  Configuration: kept
        across UpdateFrame, not stored in checkpoints (set it again and upload the temperature after LoadCheckpoint).  Whole-grid contexts only."""
        self._need()
        if ambient is None:
            capi.check(self._lib.fx_set_buoyancy(self._ctx, None), "SetBuoyancy")
            return
        b = capi.Buoyancy()
        b.struct_size, b.flags = C.sizeof(capi.Buoyancy), int(flags)
        b.ambient, b.density_weight, b.lift, b.cooling = float(ambient), float(density_weight), float(lift), float(cooling)
        b.up = (C.c_float * 3)(*[float(v) for v in up])
        capi.check(self._lib.fx_set_buoyancy(self._ctx, C.byref(b)), "SetBuoyancy")

    def GetBuoyancy(self):
        """the coefficients in force (fx_get_buoyancy) as a dict with SetBuoyancy's keys, or None while buoyancy is off"""
        self._need()
        b, on = capi.Buoyancy(), C.c_int(0)
        capi.check(self._lib.fx_get_buoyancy(self._ctx, C.byref(b), C.byref(on)), "GetBuoyancy")
        if not on.value:
            return None
        return {"ambient": b.ambient, "density_weight": b.density_weight, "lift": b.lift, "cooling": b.cooling, "up": tuple(b.up), "flags": b.flags}

    def SetHeatSources(self, sources):
        """the heat sources of the buoyancy pass (fx_set_heat_sources): a sequence of dicts (or capi.HeatSource) with "center" (x, y, z) and "radius"
        as an emitter's, and "rate" (temperature per unit time at the centre; negative = a cold source).  None or () = none (default).  May be
        set while buoyancy is off.  Configuration: kept across UpdateFrame, not stored in checkpoints.  Whole-grid contexts only."""
        self._need()
        items = list(sources or ())
        arr = (capi.HeatSource * max(len(items), 1))()
        for k, e in enumerate(items):
            if isinstance(e, capi.HeatSource):
                arr[k] = e
                continue
            arr[k].struct_size, arr[k].flags = C.sizeof(capi.HeatSource), int(e.get("flags", 0))
            arr[k].center = (C.c_float * 3)(*[float(v) for v in e["center"]])
            arr[k].radius = float(e["radius"])
            arr[k].rate = float(e["rate"])
        capi.check(self._lib.fx_set_heat_sources(self._ctx, arr if items else None, len(items)), "SetHeatSources")

    def GetHeatSources(self):
        """the list in force (fx_get_heat_sources), as dicts with the keys SetHeatSources takes"""
        self._need()
        n = C.c_uint32(0)
        arr = (capi.HeatSource * capi.MAX_HEAT_SOURCES)()
        capi.check(self._lib.fx_get_heat_sources(self._ctx, arr, capi.MAX_HEAT_SOURCES, C.byref(n)), "GetHeatSources")
        return [{"center": tuple(e.center), "radius": e.radius, "rate": e.rate, "flags": e.flags} for e in arr[:n.value]]

    def Heat(self, stream=None):
        """the buoyancy stage alone (fx_heat): TEMPERATURE advected with VELOCITY, the force in place on VELOCITY1; run it before ConfineVorticity"""
        self._need()
        capi.check(self._lib.fx_heat(self._ctx, stream), "Heat")

    def SetParticles(self, records, stream=None):
        """tracer particles carried by the flow (fx_set_particles): `records` is anything numpy takes as an array of shape (n, 4) = (x, y, z, age)
        -- positions in texture space [0, 1]^3, age >= 0 alive, anything else dead -- or a float32 torch tensor of that shape on the context's
        device, which is copied on the device.  Replaces the set; None or an empty array frees it (default).  Simulate then moves the live
        records behind the projection.  Caller data: kept across UpdateFrame, not stored in checkpoints.  Whole-grid contexts only."""
        self._need()
        if records is None:
            capi.check(self._lib.fx_set_particles(self._ctx, stream, None, 0, 0), "SetParticles")
            return
        if hasattr(records, "data_ptr") and getattr(records, "is_cuda", False):
            import torch
            t = records.to(dtype=torch.float32).contiguous().reshape(-1, 4)
            torch.cuda.current_stream(t.device).synchronize()      # the tensor was made on torch's stream, the library reads it on its own
            capi.check(self._lib.fx_set_particles(self._ctx, stream, C.cast(t.data_ptr() or None, C.POINTER(C.c_float)), t.shape[0], capi.PARTICLES_DEVICE), "SetParticles")
            return
        r = np.ascontiguousarray(np.asarray(records, np.float32).reshape(-1, 4))
        capi.check(self._lib.fx_set_particles(self._ctx, stream, _fp(r) if r.size else None, r.shape[0], 0), "SetParticles")

    def GetParticles(self):
        """the set as it stands (fx_get_particles; blocks like download): float32 (n, 4)"""
        self._need()
        dev, n = self.ParticlesDevice()
        out = np.empty((n, 4), np.float32)
        got = C.c_uint32(0)
        capi.check(self._lib.fx_get_particles(self._ctx, _fp(out) if n else None, n, C.byref(got)), "GetParticles")
        return out[:got.value]

    def ParticlesDevice(self):
        """(device address of the context's record buffer, count) for zero-copy drawing and respawning (fx_particles_device); (0, 0) with no
        set.  Valid until the next SetParticles or Release"""
        self._need()
        p, n = C.c_void_p(None), C.c_uint32(0)
        capi.check(self._lib.fx_particles_device(self._ctx, C.byref(p), C.byref(n)), "ParticlesDevice")
        return int(p.value or 0), int(n.value)

    def SetParticleParams(self, scheme="midpoint", drift=(0.0, 0.0, 0.0), lifetime=0.0, flags=0):
        """how the particles move (fx_set_particle_params): scheme "midpoint" (default) or "euler" (or a capi.PARTICLE_* value), `drift` added to
        the sampled velocity (texture space per second; settling ash: negative y), `lifetime` in seconds (0 = immortal).  SetParticleParams(None)
        restores the defaults."""
        self._need()
        if scheme is None:
            capi.check(self._lib.fx_set_particle_params(self._ctx, None), "SetParticleParams")
            return
        p = capi.ParticleParams()
        p.struct_size, p.flags = C.sizeof(capi.ParticleParams), int(flags)
        p.scheme = {"euler": capi.PARTICLE_EULER, "midpoint": capi.PARTICLE_MIDPOINT}.get(scheme, scheme)
        p.drift = (C.c_float * 3)(*[float(v) for v in drift])
        p.lifetime = float(lifetime)
        capi.check(self._lib.fx_set_particle_params(self._ctx, C.byref(p)), "SetParticleParams")

    def GetParticleParams(self):
        """the setting in force (fx_get_particle_params) as a dict with SetParticleParams' keys"""
        self._need()
        p = capi.ParticleParams()
        capi.check(self._lib.fx_get_particle_params(self._ctx, C.byref(p)), "GetParticleParams")
        return {"scheme": {capi.PARTICLE_EULER: "euler", capi.PARTICLE_MIDPOINT: "midpoint"}.get(p.scheme, p.scheme), "drift": tuple(p.drift),
                "lifetime": p.lifetime, "flags": p.flags}

    def MoveParticles(self, stream=None):
        """the particle stage alone (fx_move_particles): every live record one step through VELOCITY; Project does not include it"""
        self._need()
        capi.check(self._lib.fx_move_particles(self._ctx, stream), "MoveParticles")

    def SetParticleSort(self, enabled, every=0, flags=0):
        """the particle sort (fx_set_particle_sort): `enabled` allocates the sort's scratch for the set in force and every later one (False
        frees it, the default); `every` = n > 0 lets the particle stage sort in front of the move on its 1st, (n+1)th ... run, 0 leaves
        sorting to SortParticles.  The sort is stable, by cell, dead records last.  SetParticleSort(None) restores the default."""
        self._need()
        if enabled is None:
            capi.check(self._lib.fx_set_particle_sort(self._ctx, None), "SetParticleSort")
            return
        p = capi.ParticleSort()
        p.struct_size, p.flags, p.enabled, p.every = C.sizeof(capi.ParticleSort), int(flags), int(enabled), int(every)
        capi.check(self._lib.fx_set_particle_sort(self._ctx, C.byref(p)), "SetParticleSort")

    def GetParticleSort(self):
        """the setting in force (fx_get_particle_sort) as a dict with SetParticleSort's keys"""
        self._need()
        p = capi.ParticleSort()
        capi.check(self._lib.fx_get_particle_sort(self._ctx, C.byref(p)), "GetParticleSort")
        return {"enabled": bool(p.enabled), "every": p.every, "flags": p.flags}

    def SortParticles(self, stream=None):
        """the sort alone (fx_sort_particles): the buffer of ParticlesDevice() by cell, the dead last; enqueues only"""
        self._need()
        capi.check(self._lib.fx_sort_particles(self._ctx, stream), "SortParticles")

    def ParticleSortInfo(self, stream=None):
        """(live, sorts) (fx_particle_sort_info; waits for the stream): the live records the last sort counted -- they occupy [0, live) --
        and the sorts enqueued since the last SetParticles / SetParticleSort"""
        self._need()
        r = capi.ParticleSortInfo()
        r.struct_size = C.sizeof(capi.ParticleSortInfo)
        capi.check(self._lib.fx_particle_sort_info(self._ctx, stream, C.byref(r)), "ParticleSortInfo")
        return int(r.live), int(r.sorts)

    def ParticleOrderDevice(self):
        """(device address of order, device address of live) (fx_particle_order_device): order[i] = the index the record now at i had before
        the last sort, uint32 per record (0 with no set); live = one uint32.  Valid until the next SetParticles / SetParticleSort"""
        self._need()
        o, l = C.c_void_p(None), C.c_void_p(None)
        capi.check(self._lib.fx_particle_order_device(self._ctx, C.byref(o), C.byref(l)), "ParticleOrderDevice")
        return int(o.value or 0), int(l.value or 0)

    def ParticleOrder(self):
        """a host copy of order (numpy uint32, one per record), for tests and host callers; blocks like download"""
        self._need()
        o, _ = self.ParticleOrderDevice()
        _, n = self.ParticlesDevice()
        out = np.empty(n, np.uint32)
        if n and o:
            lib = self._lib                                  # the HIP runtime the library itself is linked against
            lib.hipDeviceSynchronize.restype, lib.hipDeviceSynchronize.argtypes = C.c_int, []
            lib.hipMemcpy.restype, lib.hipMemcpy.argtypes = C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
            if lib.hipDeviceSynchronize() != 0 or lib.hipMemcpy(out.ctypes.data, o, out.nbytes, 2) != 0:      # 2: hipMemcpyDeviceToHost
                raise RuntimeError("ParticleOrder: the copy from the device failed")
        return out

    def SetParticleTrail(self, rate, tint=(0.0, 0.0, 0.0, 0.0), heat=0.0, flags=0):
        """the particle trail (fx_set_particle_trail): every live particle spreads `rate` units of amount per second tri-linearly over the eight
        cells around it; COLOR grows by `tint` (r, g, b, a) per unit amount and, while buoyancy is on, TEMPERATURE by `heat` per unit amount.
        Simulate then deposits between the buoyancy pass and the obstacles' enforce pass.  Allocates one uint64 per cell.  SetParticleTrail(None)
        switches it off (the default) and frees that.  Configuration: kept across UpdateFrame, not stored in checkpoints.  Whole-grid contexts only."""
        self._need()
        if rate is None:
            capi.check(self._lib.fx_set_particle_trail(self._ctx, None), "SetParticleTrail")
            return
        t = capi.ParticleTrail()
        t.struct_size, t.flags, t.rate, t.heat = C.sizeof(capi.ParticleTrail), int(flags), float(rate), float(heat)
        t.tint = (C.c_float * 4)(*[float(v) for v in tint])
        capi.check(self._lib.fx_set_particle_trail(self._ctx, C.byref(t)), "SetParticleTrail")

    def GetParticleTrail(self):
        """the setting in force (fx_get_particle_trail) as a dict with SetParticleTrail's keys; off: rate 0, tint 0, heat 0"""
        self._need()
        t = capi.ParticleTrail()
        capi.check(self._lib.fx_get_particle_trail(self._ctx, C.byref(t)), "GetParticleTrail")
        return {"rate": t.rate, "tint": tuple(t.tint), "heat": t.heat, "flags": t.flags}

    def DepositParticles(self, stream=None):
        """the trail stage alone (fx_deposit_particles): the particles where they are now add to COLOR and TEMPERATURE; enqueues only"""
        self._need()
        capi.check(self._lib.fx_deposit_particles(self._ctx, stream), "DepositParticles")

    def ParticleDensity(self, stream=None):
        """the scatter alone (fx_particle_density; blocks): numpy uint64 [Z][Y][X], 2^24 per live particle spread tri-linearly"""
        self._need()
        X, Y, Z = self.grid
        out = np.empty((Z, Y, X), np.uint64)
        capi.check(self._lib.fx_particle_density(self._ctx, stream, out.ctypes.data_as(C.POINTER(C.c_uint64)), out.nbytes), "ParticleDensity")
        return out

    def SetParticleSpawners(self, spawners):
        """particles born on the device (fx_set_particle_spawners): a list of up to 16 dicts with the keys "shape" ("box", "ball" or a
        capi.SPAWN_* value; a ball is the ellipsoid with the half extents as semi-axes), "seed", "center" and "half_extent" (texture space),
        "rate" (births per second), "age_spread" (a new record's age is u * age_spread) and optionally "flags".  While set, the particle stage
        of Simulate and MoveParticles bears records into dead slots of the set behind the move.  Replaces the list and zeroes the serials and
        counters; None or an empty list switches it off (the default).  Configuration: kept across UpdateFrame, not stored in checkpoints.
        Whole-grid contexts only."""
        self._need()
        spawners = list(spawners or [])
        arr = (capi.ParticleSpawner * max(len(spawners), 1))()
        for e, d in zip(arr, spawners):
            e.struct_size, e.flags = C.sizeof(capi.ParticleSpawner), int(d.get("flags", 0))
            shape = d.get("shape", "box")
            e.shape = {"box": capi.SPAWN_BOX, "ball": capi.SPAWN_BALL}.get(shape, shape)
            e.seed = int(d.get("seed", 0)) & 0xFFFFFFFF
            e.center = (C.c_float * 3)(*[float(v) for v in d["center"]])
            e.half_extent = (C.c_float * 3)(*[float(v) for v in d["half_extent"]])
            e.rate, e.age_spread = float(d["rate"]), float(d.get("age_spread", 0.0))
        capi.check(self._lib.fx_set_particle_spawners(self._ctx, arr if spawners else None, len(spawners)), "SetParticleSpawners")

    def GetParticleSpawners(self):
        """the list in force (fx_get_particle_spawners), as dicts with the keys SetParticleSpawners takes"""
        self._need()
        n = C.c_uint32(0)
        arr = (capi.ParticleSpawner * capi.MAX_PARTICLE_SPAWNERS)()
        capi.check(self._lib.fx_get_particle_spawners(self._ctx, arr, capi.MAX_PARTICLE_SPAWNERS, C.byref(n)), "GetParticleSpawners")
        return [{"shape": {capi.SPAWN_BOX: "box", capi.SPAWN_BALL: "ball"}.get(e.shape, e.shape), "seed": e.seed, "center": tuple(e.center),
                 "half_extent": tuple(e.half_extent), "rate": e.rate, "age_spread": e.age_spread, "flags": e.flags} for e in arr[:n.value]]

    def SpawnParticles(self, stream=None):
        """the spawn stage alone (fx_spawn_particles): one step's births into the dead slots of the set; enqueues only"""
        self._need()
        capi.check(self._lib.fx_spawn_particles(self._ctx, stream), "SpawnParticles")

    def ParticleSpawnInfo(self, stream=None):
        """the counters since the last SetParticleSpawners (fx_particle_spawn_info; waits for the stream) as a dict: "born" (records stored),
        "dropped" (births that found no dead slot), "blocked" (births inside a solid) and "serial" (per spawner, the births attempted)"""
        self._need()
        r = capi.ParticleSpawnInfo()
        r.struct_size = C.sizeof(capi.ParticleSpawnInfo)
        capi.check(self._lib.fx_particle_spawn_info(self._ctx, stream, C.byref(r)), "ParticleSpawnInfo")
        return {"born": int(r.born), "dropped": int(r.dropped), "blocked": int(r.blocked), "serial": [int(v) for v in r.serial]}

    def SetParticleDraw(self, color, end_color=None, flags=0):
        """the particle draw (fx_set_particle_draw): DrawParticles then splats every live particle onto the render target as an emissive point of
        `color` (r, g, b, intensity), fading linearly to `end_color` (default: `color`) as its age reaches the lifetime of SetParticleParams,
        dimmed by the smoke the direct view march shows in front of it.  Allocates two uint64 per pixel.  SetParticleDraw(None) switches it off
        (the default) and frees that.  Configuration: kept across UpdateFrame, not stored in checkpoints.  Whole 3-D grids with a viewport only."""
        self._need()
        if color is None:
            capi.check(self._lib.fx_set_particle_draw(self._ctx, None), "SetParticleDraw")
            return
        d = capi.ParticleDraw()
        d.struct_size, d.flags = C.sizeof(capi.ParticleDraw), int(flags)
        d.color = (C.c_float * 4)(*[float(v) for v in color])
        d.end_color = (C.c_float * 4)(*[float(v) for v in (color if end_color is None else end_color)])
        capi.check(self._lib.fx_set_particle_draw(self._ctx, C.byref(d)), "SetParticleDraw")

    def GetParticleDraw(self):
        """the setting in force (fx_get_particle_draw) as a dict with SetParticleDraw's keys; off: both colours 0"""
        self._need()
        d = capi.ParticleDraw()
        capi.check(self._lib.fx_get_particle_draw(self._ctx, C.byref(d)), "GetParticleDraw")
        return {"color": tuple(d.color), "end_color": tuple(d.end_color), "flags": d.flags}

    def DrawParticles(self, frameIndex=0, stream=None):
        """the particles onto the render target (fx_draw_particles), on top of what Render and RenderCube put there, with the camera of the
        last UpdateFrame; FIELD_TARGET_FLOAT then holds the light added per pixel.  Enqueues only"""
        self._need()
        capi.check(self._lib.fx_draw_particles(self._ctx, stream, frameIndex), "DrawParticles")

    def ParticleSplats(self, stream=None):
        """the splat alone (fx_particle_splats; blocks): numpy uint64 [H][W][2], the young and the old amounts per pixel, 2^37 in total per
        unoccluded particle whose footprint is on screen"""
        self._need()
        W, H = self.viewport
        out = np.empty((H, W, 2), np.uint64)
        capi.check(self._lib.fx_particle_splats(self._ctx, stream, out.ctypes.data_as(C.POINTER(C.c_uint64)), out.nbytes), "ParticleSplats")
        return out

    def SetParticlePool(self, n, stream=None):
        """a set of `n` dead records (0, 0, 0, -1) (SetParticles): how a set that is only ever spawned into starts"""
        rec = np.zeros((int(n), 4), np.float32)
        rec[:, 3] = -1.0
        self.SetParticles(rec, stream)

    def SampleVelocity(self, points, stream=None, out=None):
        """the velocity at points of texture space (fx_sample_velocity): `points` (n, 3) or (n, 4) (a fourth column is ignored) as anything numpy
        takes -> float32 (n, 3), blocking; or a float32 torch tensor (n, 4) on the context's device with `out` a float32 tensor (n, 3) there:
        enqueued on `stream`, returns `out`."""
        self._need()
        if hasattr(points, "data_ptr") and getattr(points, "is_cuda", False):
            if out is None or tuple(out.shape) != (points.shape[0], 3) or tuple(points.shape[1:]) != (4,) or not points.is_contiguous() or not out.is_contiguous():
                raise TypeError("SampleVelocity: device points are a contiguous float32 (n, 4) tensor and take a contiguous float32 (n, 3) `out`")
            fp = C.POINTER(C.c_float)
            capi.check(self._lib.fx_sample_velocity(self._ctx, stream, C.cast(points.data_ptr() or None, fp), points.shape[0],
                                                    C.cast(out.data_ptr() or None, fp), capi.PARTICLES_DEVICE), "SampleVelocity")
            return out
        p = np.asarray(points, np.float32)
        p = p.reshape(-1, p.shape[-1] if p.ndim > 1 else 3)
        if p.shape[1] == 3:
            p = np.concatenate([p, np.zeros((p.shape[0], 1), np.float32)], axis=1)
        p = np.ascontiguousarray(p.reshape(-1, 4))
        res = np.empty((p.shape[0], 3), np.float32)
        capi.check(self._lib.fx_sample_velocity(self._ctx, stream, _fp(p) if p.size else None, p.shape[0], _fp(res) if p.size else None, 0), "SampleVelocity")
        return res

    def Divergence(self, stream=None):
        capi.check(self._lib.fx_divergence(self._ctx, stream), "Divergence")

    def Jacobi(self, iters, stream=None):
        capi.check(self._lib.fx_jacobi(self._ctx, stream, iters), "Jacobi")

    def Project(self, stream=None):
        capi.check(self._lib.fx_project(self._ctx, stream), "Project")

    def frame_info(self):
        self._need()
        fi = capi.FrameInfo()
        capi.check(self._lib.fx_get_frame_info(self._ctx, C.byref(fi)), "frame_info")
        return fi

    def _shape(self, field):
        X, Y, _ = self.grid
        nz = self.slab[1]
        if field in (capi.FIELD_VELOCITY, capi.FIELD_VELOCITY1):
            return (3, nz, Y, X), np.float32
        if field in (capi.FIELD_COLOR, capi.FIELD_COLOR_PREV):
            return (nz, Y, X, 4), np.float32
        if field in (capi.FIELD_PRESSURE, capi.FIELD_DIVERGENCE, capi.FIELD_TEMPERATURE):
            return (nz, Y, X), np.float32
        if field == capi.FIELD_LIGHTMAP:
            return (nz, Y, X, 3), np.float32
        if field == capi.FIELD_TARGET:
            return (self.viewport[1], self.viewport[0], 4), np.uint8
        if field == capi.FIELD_TARGET_FLOAT:
            return (self.viewport[1], self.viewport[0], 4), np.float32
        s = self.frame_info().cube_size
        if field == capi.FIELD_CUBE_DEPTH:
            return (6, s, s), np.float32
        return (6, s, s, 4), np.uint8

    def download(self, field):
        self._need()
        shape, dt = self._shape(field)
        out = np.empty(shape, dt)
        capi.check(self._lib.fx_download(self._ctx, field, out.ctypes.data_as(C.c_void_p), out.nbytes), "download")
        return out

    def digest(self, field, z_begin=0, z_count=0):
        """128-bit device-side digest (an int) of global planes [z_begin, z_begin + z_count) of a simulation field -- equal between a
        slab context and a single-domain context iff the planes agree bit for bit (fx_field_digest); z_count = 0: all owned planes"""
        z_begin, z_count = int(z_begin), int(z_count)
        if not (0 <= z_begin < 1 << 32 and 0 <= z_count < 1 << 32):     # ctypes would truncate to 32 bits without a word
            raise ValueError("digest: z_begin and z_count must be in 0 .. 2^32 - 1, got %d, %d" % (z_begin, z_count))
        self._need()
        out = (C.c_uint64 * 2)()
        capi.check(self._lib.fx_field_digest(self._ctx, field, z_begin, z_count, out), "digest")
        return (int(out[1]) << 64) | int(out[0])

    def upload(self, field, array):
        self._need()
        shape, dt = self._shape(field)
        a = np.ascontiguousarray(array, dt)
        if a.shape != shape:
            raise ValueError("field %d expects shape %s, got %s" % (field, shape, a.shape))
        capi.check(self._lib.fx_upload(self._ctx, field, a.ctypes.data_as(C.c_void_p), a.nbytes), "upload")

    def SaveCheckpoint(self, path):
        """velocity[0], colour[parity] and pressure of this context's planes into the whole-grid file `path` (every slab
        context of a chain saves to the same path); resuming from it continues bit-identically"""
        self._need()
        capi.check(self._lib.fx_checkpoint_save(self._ctx, os.fsencode(path)), "SaveCheckpoint")

    def LoadCheckpoint(self, path):
        self._need()
        capi.check(self._lib.fx_checkpoint_load(self._ctx, os.fsencode(path)), "LoadCheckpoint")

    def timing_enable(self, on=True):
        capi.check(self._lib.fx_timing_enable(self._ctx, int(on)), "timing_enable")

    def timing_read(self, reset=True):
        t = capi.Timing()
        capi.check(self._lib.fx_timing_read(self._ctx, C.byref(t), int(reset)), "timing_read")
        return t

    def set_option(self, option, value):
        """slab schedule knobs (capi.OPT_OVERLAP 0..3, capi.OPT_JACOBI_ROUND 1..halo_jacobi); same on every rank"""
        self._need()
        capi.check(self._lib.fx_set_option(self._ctx, int(option), int(value)), "set_option")

    def gather_color(self, full=None, root=0, slabs=None, stream=None):
        """multi-GPU rendering, exact: every rank's colour planes travel to `root`'s whole-grid context `full` (pass it on
        the root, None elsewhere); slabs = [(z0, nz)] * nranks for RCCL groups (a loop-back group knows its members)."""
        self._need()
        z0 = nz = None
        if slabs is not None:
            z0 = (C.c_uint32 * len(slabs))(*[int(a) for a, _ in slabs])
            nz = (C.c_uint32 * len(slabs))(*[int(b) for _, b in slabs])
        capi.check(self._lib.fx_comm_gather_color(self._ctx, stream, full._ctx if full is not None else None, int(root), z0, nz),
                   "gather_color")

    # ---- multi-GPU slabs ---------------------------------------------------------------------------------
    def comm_init_rank(self, unique_id, rank, nranks):
        buf = (C.c_char * len(unique_id)).from_buffer_copy(unique_id)
        capi.check(self._lib.fx_comm_init_rank(self._ctx, buf, len(unique_id), rank, nranks), "comm_init_rank")


def comm_unique_id():
    lib = capi.load()
    n = lib.fx_comm_id_bytes()
    buf = (C.c_char * n)()
    capi.check(lib.fx_comm_get_unique_id(buf, n), "comm_get_unique_id")
    return bytes(buf)


#: what `comm_init_local` builds when the caller does not say: the shared-stream group, or (tests re-running the slab suite with
#: real concurrency) the peer group
default_local_group = "shared"


def comm_init_local(fluids, peer=None):
    """In-process slab group of several `Fluid` slab contexts, driven through the first.  peer=False: one device, every member on one
    compute stream (fx_comm_init_local); peer=True: every member on its own streams and, if created so, its own device -- halo planes
    are pulled out of the neighbour's memory (fx_comm_init_peer)."""
    lib = capi.load()
    arr = (C.c_void_p * len(fluids))(*[f._ctx for f in fluids])
    if peer is None:
        peer = default_local_group == "peer"
    if peer:
        capi.check(lib.fx_comm_init_peer(arr, len(fluids)), "comm_init_peer")
    else:
        capi.check(lib.fx_comm_init_local(arr, len(fluids)), "comm_init_local")


def comm_init_peer(fluids):
    comm_init_local(fluids, peer=True)


class LightProbe:
    """SH side of class LightProbe (Content/LightProbe.h:16-26): TransformSH + GetSH."""

    def __init__(self, fluid):
        self._fluid = fluid
        self._radiance = None
        self._sh = None

    def Init(self, radiance_cube, mip=0):
        """radiance: a float cube [6][N][N][3], or -- like the reference (LightProbe.cpp:41-46) -- a DDS cube map in
        BC6H_UF16 given as a file name or its bytes (mip `mip` is decoded on the device)."""
        if isinstance(radiance_cube, (str, bytes, bytearray)):
            data = open(radiance_cube, "rb").read() if isinstance(radiance_cube, str) else bytes(radiance_cube)
            radiance_cube = self.decode_dds(data, mip)
            if radiance_cube is None:
                return False
        a = np.ascontiguousarray(radiance_cube, np.float32)
        if a.ndim != 4 or a.shape[0] != 6 or a.shape[1] != a.shape[2] or a.shape[3] != 3:
            return False
        self._radiance = a
        return True

    def decode_dds(self, data, mip=0):
        """DDS (BC6H_UF16 cube) bytes -> float32[6][n][n][3], or None if the container is something else"""
        f = self._fluid
        f._need()
        size, mips = C.c_uint32(), C.c_uint32()
        buf = (C.c_char * len(data)).from_buffer_copy(data)
        if f._lib.fx_dds_cube_info(buf, len(data), C.byref(size), C.byref(mips)) != capi.FX_OK or mip >= mips.value:
            return None
        n = max(size.value >> mip, 1)
        out = np.empty((6, n, n, 3), np.float32)
        capi.check(f._lib.fx_dds_decode_cube(f._ctx, buf, len(data), mip, _fp(out), out.size), "decode_dds")
        return out

    def TransformSH(self):
        f = self._fluid
        f._need()
        out = np.empty((9, 3), np.float32)
        capi.check(f._lib.fx_sh_transform(f._ctx, _fp(self._radiance), self._radiance.shape[1], _fp(out)), "TransformSH")
        self._sh = out

    def GetSH(self):
        return self._sh
