"""Python mirror of the reference's render surface, over the C ABI.

Reference interface (iMacsimus/Triangles-SDF-CPU-RayTracing @ 2025-07-04):
  FrameBuffer {color, t}; clear()             src/raytracing.hpp:9-20
  ShadingMode {Normal, Lambert, Color}         src/raytracing.hpp:99
  Renderer {lightPos, enableShadows, enableReflections, shadingMode};
      float draw(scene, frameBuffer, camera, projInv)  src/raytracing.hpp:101-117
  IScene::intersect(rayPos, rayDir, tNear, tFar) -> HitInfo  src/raytracing.hpp:75-81
  BVHBuilder::perform(SimpleMesh)               src/triangles_raytracing.hpp:38-67
  SDFGrid / loadSDFGrid                         src/grid_raytracing.hpp:10-22
  SDFOctree / loadSDFOctree                     src/octree_raytracing.hpp:20-49
  Plane(normal, offset), SceneUnion(a, b)       src/raytracing.hpp:83-97, 119-186
  Camera(position, target, up)                  src/camera.hpp:7-61
  cmesh4::LoadMeshFromObj + loadAndScale        src/core/mesh.cpp:178, src/main.cpp:326-343

Every call goes to the HIP implementation in librtamd.so; errors raise RtError.
"""
from __future__ import annotations

import ctypes as C
import enum
from dataclasses import dataclass

import numpy as np

from ._lib import (RT_FLAG_CLEAR, RT_FLAG_HITS_ONLY, RT_INSTANCE_DISABLED, RT_INSTANCED_TLAS, RT_MESH_DYNAMIC,
                   RT_POINTS_UNSIGNED, RT_RAYS_ANY_HIT, RT_SHADE_CLEAR, CameraState, Instance, PointBatch, RayBatch, RenderParams, RtError, Tile, check, lib)

__all__ = [
    "ShadingMode", "SimpleMesh", "FrameBuffer", "Camera", "Renderer", "HitInfo", "IScene",
    "BVHBuilder", "SDFGrid", "SDFOctree", "InstancedScene", "InstanceTable", "affine_inverse", "instance_world_box", "morton_order", "Plane", "SceneUnion", "load_mesh_from_obj",
    "load_sdf_grid", "load_sdf_octree", "camera_matrices", "render_params", "RtError",
    "RT_FLAG_CLEAR", "Tile", "device_count", "SDFMesh", "subdivide_mesh", "save_mesh_to_obj",
    "MultiRenderer", "eye_rays_device",
]


def _p(a):
    return None if a is None else C.c_void_p(a.ctypes.data)


def device_count() -> int:
    return lib().rt_device_count()


class ShadingMode(enum.IntEnum):
    Normal = 0
    Lambert = 1
    Color = 2


@dataclass
class SimpleMesh:
    """cmesh4::SimpleMesh positions + indices (src/core/mesh.h:15-55)."""
    vPos4f: np.ndarray      # float32 [N, 4]
    indices: np.ndarray     # uint32 [3*T]

    def TrianglesNum(self) -> int:
        return len(self.indices) // 3


def load_mesh_from_obj(path: str, scale: bool = True) -> SimpleMesh:
    """LoadMeshFromObj (+ loadAndScale when scale=True, as main.cpp does for every .obj)."""
    L = lib()
    nv, ni = C.c_int64(0), C.c_int64(0)
    check(L.rt_load_obj(path.encode(), int(scale), None, C.byref(nv), None, C.byref(ni)))
    v = np.empty((nv.value, 4), np.float32)
    i = np.empty(ni.value, np.uint32)
    check(L.rt_load_obj(path.encode(), int(scale), _p(v), C.byref(nv), _p(i), C.byref(ni)))
    return SimpleMesh(v, i)


def save_mesh_to_obj(path: str, mesh: SimpleMesh, normals=None, texcoords=None):
    """cmesh4::SaveMeshToObj (src/core/mesh.cpp:14-63), byte for byte."""
    v = np.ascontiguousarray(mesh.vPos4f, np.float32)
    i = np.ascontiguousarray(mesh.indices, np.uint32)
    n = None if normals is None else np.ascontiguousarray(normals, np.float32)
    t = None if texcoords is None else np.ascontiguousarray(texcoords, np.float32)
    check(lib().rt_save_obj(str(path).encode(), _p(v), len(v), _p(i), len(i), _p(n), _p(t)))


def load_sdf_grid(path: str):
    """loadSDFGrid -> (size uint32[3], values float32[sx*sy*sz])."""
    L = lib()
    size = np.zeros(3, np.uint32)
    check(L.rt_load_grid(path.encode(), _p(size), None))
    vals = np.empty(int(size[0]) * int(size[1]) * int(size[2]), np.float32)
    check(L.rt_load_grid(path.encode(), _p(size), _p(vals)))
    return size, vals


def load_sdf_octree(path: str) -> np.ndarray:
    """loadSDFOctree -> raw nodes, uint8 [count*36] (SDFOctreeNode, 36 B each)."""
    L = lib()
    n = C.c_int64(0)
    check(L.rt_load_octree(path.encode(), C.byref(n), None))
    buf = np.empty(n.value * 36, np.uint8)
    check(L.rt_load_octree(path.encode(), C.byref(n), _p(buf)))
    return buf


def camera_matrices(position, target=(0.0, 0.0, 0.0), up=(0.0, 1.0, 0.0), fovy=45.0,
                    aspect=16.0 / 9.0, znear=0.01, zfar=100.0):
    """(view_inv, proj_inv) column-major float32[16]:
    inverse4x4(Camera(position, target, up).lookAtMatrix()) and
    inverse4x4(perspectiveMatrix(fovy, aspect, znear, zfar)) (main.cpp:198-201)."""
    # keep the argument arrays alive across the call (a temporary's buffer may be freed)
    pos = np.array(position, np.float32)
    tgt = np.array(target, np.float32)
    upv = np.array(up, np.float32)
    vi = np.zeros(16, np.float32)
    pi = np.zeros(16, np.float32)
    check(lib().rt_camera(_p(pos), _p(tgt), _p(upv), fovy, aspect, znear, zfar, _p(vi), _p(pi)))
    return vi, pi


def render_params(cam_pos, view_inv, proj_inv, light=(2.0, 2.0, 2.0), mode=ShadingMode.Lambert,
                  shadows=True, reflections=True) -> RenderParams:
    P = RenderParams()
    P.camera_pos[:] = [float(x) for x in cam_pos]
    P.view_inv[:] = [float(x) for x in view_inv]
    P.proj_inv[:] = [float(x) for x in proj_inv]
    P.light_pos[:] = [float(x) for x in light]
    P.shading_mode = int(mode)
    P.enable_shadows = int(bool(shadows))
    P.enable_reflections = int(bool(reflections))
    P.reserved = 0
    return P


def eye_rays_device(params: RenderParams, W: int, H: int, origin_ptr: int | None, dir_ptr: int | None,
                    stream: int | None = None):
    """The eye rays of the frame `params` describes as a ray batch in device
    buffers (rt_eye_rays_device): ray y * W + x is pixel (x, y); float32[3 W H]
    each, either pointer may be None. Queued on `stream`; only launches."""
    check(lib().rt_eye_rays_device(C.byref(params), W, H, C.c_void_p(origin_ptr or None),
                                   C.c_void_p(dir_ptr or None), C.c_void_p(stream) if stream else None))


class Camera:
    """Camera (src/camera.hpp:7-61, src/camera.cpp:1-72): the viewer's orbit
    camera -- position, target and an orientation quaternion -- through the
    host-side C ABI (rt_camera_*), bit-identical to the reference's float math."""

    def __init__(self, position=(0.0, 0.0, 2.5), target=(0.0, 0.0, 0.0), up=(0.0, 1.0, 0.0)):
        self._s = CameraState()
        p, t, u = (np.ascontiguousarray(x, np.float32) for x in (position, target, up))
        check(lib().rt_camera_init(_p(p), _p(t), _p(u), C.byref(self._s)))

    def position(self):
        return np.array(self._s.position, np.float32)

    def target(self):
        return np.array(self._s.target, np.float32)

    def _basis(self):
        u, r, f = (np.zeros(3, np.float32) for _ in range(3))
        check(lib().rt_camera_basis(C.byref(self._s), _p(u), _p(r), _p(f)))
        return u, r, f

    def up(self):
        return self._basis()[0]

    def right(self):
        return self._basis()[1]

    def forward(self):
        return self._basis()[2]

    def sensetivity(self) -> float:  # (sic) camera.hpp:38
        return float(self._s.sensitivity)

    def rotate(self, dx: float, dy: float):
        """Camera::rotate (camera.cpp:5-20); the viewer calls rotate(-dx, -dy) on a drag."""
        check(lib().rt_camera_rotate(C.byref(self._s), float(dx), float(dy)))

    def resetPosition(self, position):
        p = np.ascontiguousarray(position, np.float32)
        check(lib().rt_camera_reset_position(C.byref(self._s), _p(p)))

    def resetTarget(self, target):
        t = np.ascontiguousarray(target, np.float32)
        check(lib().rt_camera_reset_target(C.byref(self._s), _p(t)))

    def setLockUp(self, on: bool):
        check(lib().rt_camera_set_lock_up(C.byref(self._s), int(bool(on))))

    def isLockedUp(self) -> bool:
        return bool(self._s.lock_up)

    def zoom(self, wheel: float):
        """The viewer's mouse wheel (main.cpp:281-288)."""
        check(lib().rt_camera_zoom(C.byref(self._s), float(wheel)))

    def view_inv(self):
        """inverse4x4(lookAtMatrix()), column-major float32[16]."""
        vi = np.zeros(16, np.float32)
        check(lib().rt_camera_view_inverse(C.byref(self._s), _p(vi)))
        return vi

    def state(self) -> CameraState:
        return self._s


class FrameBuffer:
    """FrameBuffer {Image2D<uint32_t> color; Image2D<float> t;} (raytracing.hpp:9-20)."""

    def __init__(self, width: int, height: int):
        self.resize(width, height)

    def resize(self, width: int, height: int):
        self.color = np.zeros((height, width), np.uint32)
        self.t = np.full((height, width), np.inf, np.float32)

    def clear(self):
        self.color.fill(0)
        self.t.fill(np.inf)

    @property
    def width(self):
        return self.color.shape[1]

    @property
    def height(self):
        return self.color.shape[0]

    def save_png(self, path: str):
        """The colour buffer as an 8-bit RGBA PNG (rt_write_png)."""
        c = np.ascontiguousarray(self.color, np.uint32)
        check(lib().rt_write_png(str(path).encode(), _p(c), self.width, self.height))


@dataclass
class HitInfo:
    """HitInfo (raytracing.hpp:67-73) for a batch; prim is this build's primitive id."""
    hitten: np.ndarray
    t: np.ndarray
    normal: np.ndarray
    prim: np.ndarray


class IScene:
    """A scene resident on the current HIP device (one rt_scene handle)."""

    _h = None
    _plane = None

    def _handle(self):
        if self._h is None:
            raise RtError("scene not built")
        return self._h

    def set_plane(self, plane: "Plane | None"):
        self._plane = plane
        if plane is None:
            check(lib().rt_scene_set_plane(self._handle(), 0, None, 0.0))
        else:
            n = np.asarray(plane.normal, np.float32)
            check(lib().rt_scene_set_plane(self._handle(), 1, _p(n), float(plane.offset)))

    def intersect(self, ray_pos, ray_dir, tNear=0.01, tFar=100.0) -> HitInfo:
        """IScene::intersect for a batch of rays ([N,3] origins and directions)."""
        o = np.ascontiguousarray(np.asarray(ray_pos, np.float32).reshape(-1, 3))
        d = np.ascontiguousarray(np.asarray(ray_dir, np.float32).reshape(-1, 3))
        n = len(o)
        hit = np.zeros(n, np.int32)
        t = np.zeros(n, np.float32)
        nrm = np.zeros((n, 3), np.float32)
        prim = np.zeros(n, np.int64)
        check(lib().rt_intersect_rays(self._handle(), _p(o), _p(d), n, tNear, tFar, _p(hit), _p(t),
                                      _p(nrm), _p(prim)))
        return HitInfo(hit.astype(bool), t, nrm, prim)

    def render(self, params: RenderParams, color: np.ndarray, t: np.ndarray, clear: bool = False,
               cleared: bool = False):
        """Renderer::draw on host buffers; returns the kernel time in ms.
        clear: FrameBuffer::clear() + draw fused (every pixel written);
        cleared: the buffers already hold a cleared frame (only the hits'
        bounding box is copied back); neither: t is read as tPrev."""
        H, W = color.shape
        assert color.dtype == np.uint32 and t.dtype == np.float32 and t.shape == color.shape
        assert color.flags.c_contiguous and t.flags.c_contiguous
        ms = C.c_float(0.0)
        flags = (RT_FLAG_CLEAR | RT_FLAG_HITS_ONLY) if cleared else RT_FLAG_CLEAR if clear else 0
        check(lib().rt_render(self._handle(), C.byref(params), _p(color), _p(t), W, H, flags, C.byref(ms)))
        return ms.value

    def render_device(self, params: RenderParams, color_ptr: int, t_ptr: int, W: int, H: int,
                      clear: bool = True, tile: Tile | None = None, stream: int | None = None,
                      flags: int = 0):
        """Renderer::draw into device buffers (e.g. torch tensors' data_ptr()).
        `flags` adds RT_FLAG_TILE_NATURAL / RT_FLAG_HITS_ONLY (include/rtamd.h)."""
        check(lib().rt_render_device(self._handle(), C.byref(params), C.c_void_p(color_ptr),
                                     C.c_void_p(t_ptr), W, H, (RT_FLAG_CLEAR if clear else 0) | flags,
                                     C.byref(tile) if tile is not None else None,
                                     C.c_void_p(stream) if stream else None))

    def render_device_frames(self, params_list, color_ptrs, t_ptrs, W: int, H: int, flags: int,
                             tile: Tile | None = None, stream: int | None = None):
        """rt_render_device_frames: up to 16 frames per launch, one host call."""
        n = len(params_list)
        arr = (RenderParams * n)(*params_list)
        cp = (C.c_void_p * n)(*color_ptrs)
        tp = (C.c_void_p * n)(*t_ptrs)
        check(lib().rt_render_device_frames(self._handle(), arr, n, cp, tp, W, H, flags,
                                            C.byref(tile) if tile is not None else None,
                                            C.c_void_p(stream) if stream else None))

    def trace_device(self, origin_ptr: int, dir_ptr: int, n: int, *, hit_ptr: int | None = None,
                     t_ptr: int | None = None, normal_ptr: int | None = None, prim_ptr: int | None = None,
                     tnear: float = 0.01, tfar: float = 100.0, tnear_ptr: int | None = None,
                     tfar_ptr: int | None = None, any_hit: bool = False, stream: int | None = None):
        """IScene::intersect on device buffers (rt_trace_rays_device): n rays at
        origin_ptr / dir_ptr (float32[3n], e.g. torch tensors' data_ptr()),
        traced in stream order on `stream`; the call only launches. Outputs
        left None are neither computed nor written (int32 hit, float32 t,
        float32[3n] normal, int64 prim). tnear_ptr / tfar_ptr (float32[n])
        replace the scalars per ray. any_hit: hit_ptr only, the traversal
        stops at the first hit."""
        b = RayBatch(int(n), origin_ptr or None, dir_ptr or None, tnear_ptr or None, tfar_ptr or None,
                     float(tnear), float(tfar), hit_ptr or None, t_ptr or None, normal_ptr or None,
                     prim_ptr or None)
        check(lib().rt_trace_rays_device(self._handle(), C.byref(b), RT_RAYS_ANY_HIT if any_hit else 0,
                                         C.c_void_p(stream) if stream else None))

    def shade_device(self, origin_ptr: int, dir_ptr: int, n: int, params: RenderParams, color_ptr: int, *,
                     t_ptr: int | None = None, hit_ptr: int | None = None, prim_ptr: int | None = None,
                     tnear: float = 0.01, tfar: float = 100.0, tnear_ptr: int | None = None,
                     tfar_ptr: int | None = None, clear: bool = True, stream: int | None = None):
        """The per-ray body of Renderer::draw on device buffers
        (rt_shade_rays_device): n rays at origin_ptr / dir_ptr (float32[3n])
        are intersected with the scene and its plane and shaded under
        `params` (its light, shading mode and switches); a ray that hits gets
        its packed RGBA8 colour at color_ptr (uint32[n]) and its t at t_ptr.
        clear: a miss gets 0 / +inf; otherwise it writes neither, and
        tfar_ptr may be t_ptr (the reference's tPrev). hit_ptr (int32) and
        prim_ptr (int64) are always written when given. Queued on `stream`;
        the call only launches. All scene kinds, instanced ones included."""
        b = RayBatch(int(n), origin_ptr or None, dir_ptr or None, tnear_ptr or None, tfar_ptr or None,
                     float(tnear), float(tfar), hit_ptr or None, t_ptr or None, None, prim_ptr or None)
        check(lib().rt_shade_rays_device(self._handle(), C.byref(b), C.byref(params), C.c_void_p(color_ptr or None),
                                         RT_SHADE_CLEAR if clear else 0, C.c_void_p(stream) if stream else None))

    def bench_frames(self, params_list, W: int, H: int, clear: bool = True):
        arr = (RenderParams * len(params_list))(*params_list)
        mean, total = C.c_float(0.0), C.c_float(0.0)
        check(lib().rt_bench_frames(self._handle(), arr, len(params_list), W, H,
                                    RT_FLAG_CLEAR if clear else 0, C.byref(mean), C.byref(total)))
        return mean.value, total.value

    COUNTER_NAMES = ("bvh_inner", "bvh_leaf", "bvh_tri", "grid_sdf", "oct_node", "oct_leaf",
                     "oct_step", "oct_normal", "rays")

    def count_work(self, params_list, W: int, H: int, clear: bool = True,
                   tile: Tile | None = None) -> dict:
        """Reference-traversal work counters over the given frames (rt_count_work)."""
        arr = (RenderParams * len(params_list))(*params_list)
        out = np.zeros(9, np.int64)
        check(lib().rt_count_work(self._handle(), arr, len(params_list), W, H,
                                  RT_FLAG_CLEAR if clear else 0,
                                  C.byref(tile) if tile is not None else None, _p(out)))
        return dict(zip(self.COUNTER_NAMES, out.tolist()))

    def count_share(self, params_list, W: int, H: int) -> dict:
        """Wave-level counters of the primary mesh path over the given frames
        (rtx_count_share, the counting kernel): expansions below the root that
        fetched their node once for the wave through LDS, and all of them.
        They are no part of count_work's dict, so algorithmic_bytes and the
        oracle's counters stay what they are."""
        arr = (RenderParams * len(params_list))(*params_list)
        out = np.zeros(2, np.int64)
        check(lib().rtx_count_share(self._handle(), arr, len(params_list), W, H, RT_FLAG_CLEAR, _p(out)))
        return {"bvh_shared": int(out[0]), "bvh_wave_expansions": int(out[1])}

    @staticmethod
    def algorithmic_bytes(c: dict, pixels: int) -> int:
        """Bytes the reference's data layout touches for this work:
        BVH 200 B / inner-node visit (Box8 + realCount + offset), 8 B / leaf visit,
        60 B / triangle test (3 indices + 3 float4 vertices); grid 32 B / sdf
        evaluation (8 taps); octree 4 B / node visit, 32 B / leaf visit, 32 B /
        march step, 32 B / normal; + 8 B / pixel of framebuffer (colour + t)."""
        return int(200 * c["bvh_inner"] + 8 * c["bvh_leaf"] + 60 * c["bvh_tri"] + 32 * c["grid_sdf"]
                   + 4 * c["oct_node"] + 32 * c["oct_leaf"] + 32 * c["oct_step"]
                   + 32 * c["oct_normal"] + 8 * pixels)

    def device_bytes(self) -> int:
        return int(lib().rt_scene_device_bytes(self._handle()))

    def tree_stats(self):
        n, i, d = C.c_int64(0), C.c_int64(0), C.c_int32(0)
        check(lib().rt_scene_bvh_stats(self._handle(), C.byref(n), C.byref(i), C.byref(d)))
        return n.value, i.value, d.value

    def close(self):
        if self._h is not None:
            check(lib().rt_scene_destroy(self._h))
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class BVHBuilder(IScene):
    """BVHBuilder::perform(mesh): host SAH BVH8 build + device upload."""

    def __init__(self, mesh: SimpleMesh | None = None, dynamic: bool = False):
        if mesh is not None:
            self.perform(mesh, dynamic)

    def perform(self, mesh: SimpleMesh, dynamic: bool = False):
        """dynamic: the vertices may be moved afterwards (update_vertices*,
        RT_MESH_DYNAMIC); the scene then keeps its index array and a vertex
        staging buffer on the device."""
        self.close()
        v = np.ascontiguousarray(mesh.vPos4f, np.float32)
        i = np.ascontiguousarray(mesh.indices, np.uint32)
        h = C.c_void_p()
        if dynamic:
            check(lib().rt_scene_create_mesh_ex(_p(v), len(v), _p(i), len(i), RT_MESH_DYNAMIC, C.byref(h)))
        else:
            check(lib().rt_scene_create_mesh(_p(v), len(v), _p(i), len(i), C.byref(h)))
        self._h = h
        return self

    def update_vertices(self, vPos4f):
        """Refit the tree to new positions (float32 [N, 4] on the host, N as at
        creation): rt_scene_update_vertices. Returns when the scene is updated."""
        v = np.ascontiguousarray(vPos4f, np.float32)
        if v.ndim != 2 or v.shape[1] != 4:
            raise RtError(f"update_vertices: shape {v.shape}, expected [N, 4]")
        check(lib().rt_scene_update_vertices(self._handle(), _p(v), len(v)))

    def update_vertices_device(self, ptr: int, nverts: int, stream: int | None = None):
        """The same from device memory (float32[4 * nverts] at ptr, e.g. a torch
        tensor's data_ptr()), queued on `stream` after the work already there:
        rt_scene_update_vertices_device. One host wait; no allocation."""
        check(lib().rt_scene_update_vertices_device(self._handle(), C.c_void_p(ptr) if ptr else None, int(nverts),
                                                    C.c_void_p(stream) if stream else None))


class SDFGrid(IScene):
    def __init__(self, size, values):
        size = np.ascontiguousarray(size, np.uint32)
        values = np.ascontiguousarray(values, np.float32)
        h = C.c_void_p()
        check(lib().rt_scene_create_grid(_p(size), _p(values), C.byref(h)))
        self._h = h
        self.size = size

    def update_device(self, ptr: int, stream: int | None = None):
        """New values from device memory (float32[sx*sy*sz] at ptr in the layout
        (x*sy+y)*sz+z, e.g. what SDFMesh.grid_device wrote), queued on `stream`:
        rt_scene_update_grid_device. The call only launches; the scene keeps
        its device array, so instanced scenes over it follow."""
        check(lib().rt_scene_update_grid_device(self._handle(), C.c_void_p(ptr) if ptr else None,
                                                C.c_void_p(stream) if stream else None))


class SDFOctree(IScene):
    def __init__(self, nodes36: np.ndarray):
        nodes36 = np.ascontiguousarray(nodes36).view(np.uint8)
        h = C.c_void_p()
        check(lib().rt_scene_create_octree(_p(nodes36), nodes36.nbytes // 36, C.byref(h)))
        self._h = h

    @classmethod
    def dynamic(cls, depth: int, max_nodes: int) -> "SDFOctree":
        """An octree scene with room for max_nodes nodes of a tree of at most
        `depth` levels, which SDFMesh.octree_device rebuilds on the device
        (rt_scene_create_octree_dynamic). It starts as one empty leaf."""
        h = C.c_void_p()
        check(lib().rt_scene_create_octree_dynamic(int(depth), int(max_nodes), C.byref(h)))
        self = cls.__new__(cls)
        self._h = h
        return self

    def status(self):
        """-> (nodes the scene holds now, 1 if its last device build overflowed
        and was dropped), after a wait for the device: rt_scene_octree_status."""
        n, o = C.c_int64(0), C.c_int32(0)
        check(lib().rt_scene_octree_status(self._handle(), C.byref(n), C.byref(o)))
        return n.value, o.value

    def nodes(self) -> np.ndarray:
        """-> raw nodes, uint8 [count*36], rebuilt from what the scene holds on
        the device now (rt_scene_get_octree)."""
        n = C.c_int64(0)
        check(lib().rt_scene_get_octree(self._handle(), C.byref(n), None))
        buf = np.empty(n.value * 36, np.uint8)
        check(lib().rt_scene_get_octree(self._handle(), C.byref(n), _p(buf)))
        return buf[:n.value * 36]


def affine_inverse(xform) -> np.ndarray:
    """rt_affine_inverse: the world-to-object matrix M the library stores for an
    object-to-world map (12 floats, row-major 3x4), as float32 [3, 4]. Raises
    RtError for a singular or non-finite matrix."""
    x = np.ascontiguousarray(xform, np.float32).reshape(12)
    inv = np.zeros(12, np.float32)
    check(lib().rt_affine_inverse(_p(x), _p(inv)))
    return inv.reshape(3, 4)


def instance_world_box(xform, obox) -> np.ndarray:
    """rt_instance_world_box: the world box (lo.xyz, hi.xyz, float32 [6]) an
    RT_INSTANCED_TLAS scene gives an instance with object-to-world map `xform`
    of a BLAS whose root box is `obox` (lo.xyz, hi.xyz)."""
    x = np.ascontiguousarray(xform, np.float32).reshape(12)
    b = np.ascontiguousarray(obox, np.float32).reshape(6)
    w = np.zeros(6, np.float32)
    check(lib().rt_instance_world_box(_p(x), _p(b), _p(w)))
    return w


def morton_order(centres) -> np.ndarray:
    """A permutation of instance indices along the 30-bit Morton curve of
    their centres ([K, 3], any float type): 10 bits per axis over the centres'
    own bounding box, ties in the given order. The top-level tree of
    InstancedScene(..., tlas=True) is a complete binary tree over the
    instances IN INDEX ORDER, so its quality is the spatial coherence of that
    order; pass instances[morton_order(centres)] when the order is free.
    (prim then reports the permuted index.)"""
    c = np.asarray(centres, np.float64).reshape(-1, 3)
    lo, ext = c.min(0), np.maximum(c.max(0) - c.min(0), 1e-300)
    q = np.minimum((c - lo) / ext * 1024.0, 1023.0).astype(np.uint64)
    code = np.zeros(len(c), np.uint64)
    for bit in range(10):
        for a in range(3):
            code |= ((q[:, a] >> np.uint64(bit)) & np.uint64(1)) << np.uint64(3 * bit + 2 - a)
    return np.argsort(code, kind="stable")


@dataclass
class InstanceTable:
    """What the device holds of an InstancedScene (rt_scene_get_instances)."""
    blas: np.ndarray     # int32 [K]
    flags: np.ndarray    # uint32 [K]
    xform: np.ndarray    # float32 [K, 3, 4]: the inverse of inv (zeros for a skipped instance)
    inv: np.ndarray      # float32 [K, 3, 4]: M, world to object
    skipped: np.ndarray  # uint32 [K]: 1 = refused by the device pose update


def _instance_array(blas, xforms, flags):
    x = np.ascontiguousarray(xforms, np.float32)
    if x.ndim < 2 or x.size != x.shape[0] * 12:
        raise RtError(f"instance matrices: shape {x.shape}, expected [K, 3, 4] or [K, 12]")
    x = x.reshape(-1, 12)
    arr = (Instance * len(x))()
    for k in range(len(x)):
        arr[k].blas = int(blas[k])
        arr[k].flags = int(flags[k])
        arr[k].xform[:] = x[k].tolist()
    return arr


class InstancedScene(IScene):
    """Rigid (affine) copies of mesh scenes under one ray query
    (rt_scene_create_instanced). blas_list: BVHBuilder scenes on the current
    device; instances: (blas index, xform) or (blas index, xform, flags)
    tuples, xform the object-to-world map as 12 floats (row-major 3x4). Ray
    queries only (intersect, trace_device, torch_rays.trace): prim is
    (instance << 32) | triangle id. Keeps its BLAS objects alive.
    tlas=True (RT_INSTANCED_TLAS): a top-level tree over the instances' world
    boxes, for hundreds of instances; its quality is the spatial coherence of
    the index order (morton_order).
    blas_list may also hold SDFGrid and SDFOctree scenes
    (rt_scene_create_instanced_any): prim's low word is then the grid cell or
    the octree node of the winner, and `mixed` is True. An SDF instance wants
    a rigid pose: the march steps in units of the transformed direction."""

    DISABLED = RT_INSTANCE_DISABLED

    def __init__(self, blas_list, instances, tlas: bool = False):
        self._blas_objs = list(blas_list)
        inst = [tuple(t) for t in instances]
        self._blas_idx = np.asarray([t[0] for t in inst], np.int32)
        self._flags = np.asarray([t[2] if len(t) > 2 else 0 for t in inst], np.uint32)
        handles = (C.c_void_p * len(self._blas_objs))(*[b._handle() for b in self._blas_objs])
        xforms = np.asarray([np.asarray(t[1], np.float32).reshape(12) for t in inst], np.float32).reshape(-1, 12)
        arr = _instance_array(self._blas_idx, xforms, self._flags)
        h = C.c_void_p()
        # mesh-only lists keep their entry; the general one only when it is needed
        self.mixed = any(not isinstance(b, BVHBuilder) for b in self._blas_objs)
        create = lib().rt_scene_create_instanced_any if self.mixed else lib().rt_scene_create_instanced_ex
        check(create(handles, len(self._blas_objs), arr, len(inst), RT_INSTANCED_TLAS if tlas else 0, C.byref(h)))
        self._h = h
        self.has_tlas = bool(tlas)

    def __len__(self):
        return len(self._blas_idx)

    def update_instances(self, xforms, first: int = 0, flags=None, blas=None):
        """New poses (and, with flags, new flags; with blas, new BLAS indices)
        for instances first .. first + K - 1 from host matrices [K, 3, 4] or
        [K, 12]; without blas the indices stay (rt_scene_update_instances). A
        refused call changes nothing."""
        x = np.ascontiguousarray(xforms, np.float32)
        k = x.shape[0] if x.ndim >= 2 else 0
        if first < 0 or first + k > len(self):
            raise RtError(f"update_instances: [{first}, {first + k}) outside the scene's {len(self)} instances")
        fl = self._flags[first:first + k] if flags is None else np.broadcast_to(np.asarray(flags, np.uint32), (k,))
        bi = self._blas_idx[first:first + k] if blas is None else np.broadcast_to(np.asarray(blas, np.int32), (k,))
        arr = _instance_array(bi, x, fl)
        check(lib().rt_scene_update_instances(self._handle(), int(first), k, arr))
        self._flags[first:first + k] = fl
        self._blas_idx[first:first + k] = bi

    def update_instances_device(self, ptr: int, count: int, first: int = 0, stream: int | None = None):
        """The same from device memory: `count` matrices (float32[12 * count] at
        ptr) inverted by a kernel queued on `stream`; only launches
        (rt_scene_update_instances_device). A matrix the inverse refuses makes
        its instance skipped until its next update."""
        check(lib().rt_scene_update_instances_device(self._handle(), int(first), int(count),
                                                     C.c_void_p(ptr) if ptr else None,
                                                     C.c_void_p(stream) if stream else None))

    def tlas(self):
        """The top-level tree as the device holds it (rt_scene_get_tlas, one
        synchronisation) -> (leaf boxes float32 [K, 6], node boxes float32
        [2P, 6]; lo.xyz hi.xyz, node 0 unused)."""
        P = C.c_int32(0)
        check(lib().rt_scene_get_tlas(self._handle(), None, None, C.byref(P)))
        leaf = np.zeros((len(self), 6), np.float32)
        node = np.zeros((2 * P.value, 6), np.float32)
        check(lib().rt_scene_get_tlas(self._handle(), _p(leaf), _p(node), None))
        return leaf, node

    def instances(self) -> InstanceTable:
        """Read the instance table back from the device (one synchronisation)."""
        k = len(self)
        arr = (Instance * k)()
        inv = np.zeros((k, 3, 4), np.float32)
        skipped = np.zeros(k, np.uint32)
        check(lib().rt_scene_get_instances(self._handle(), 0, k, arr, _p(inv), _p(skipped)))
        return InstanceTable(np.asarray([a.blas for a in arr], np.int32), np.asarray([a.flags for a in arr], np.uint32),
                             np.asarray([list(a.xform) for a in arr], np.float32).reshape(k, 3, 4), inv, skipped)


@dataclass
class Plane:
    """Plane(normal, offset): the plane dot(p, normal) = offset (raytracing.hpp:121-124)."""
    normal: tuple = (0.0, 1.0, 0.0)
    offset: float = 0.0


class SceneUnion:
    """SceneUnion(scene, plane) (raytracing.hpp:83-97). The second operand must be a Plane."""

    def __init__(self, first: IScene, second: Plane):
        if not isinstance(second, Plane):
            raise RtError("SceneUnion supports (scene, Plane) as in the reference application")
        self.first, self.second = first, second


class Renderer:
    """Renderer (raytracing.hpp:101-117)."""

    def __init__(self):
        self.lightPos = (2.0, 2.0, 2.0)  # main.cpp:60
        self.enableShadows = True
        self.enableReflections = True
        self.shadingMode = ShadingMode.Lambert

    def draw(self, scene, frame_buffer: FrameBuffer, camera: Camera, proj_inv) -> float:
        """Renderer::draw: renders into frame_buffer (t read as tPrev, written on hit)."""
        if isinstance(scene, SceneUnion):
            base = scene.first
            base.set_plane(scene.second)
        else:
            base = scene
            base.set_plane(None)
        P = render_params(camera.position(), camera.view_inv(), proj_inv, self.lightPos,
                          self.shadingMode, self.enableShadows, self.enableReflections)
        return base.render(P, frame_buffer.color, frame_buffer.t, clear=False)


# ------------------------------------ one process, several GPUs (rt_multi) --
class MultiRenderer:
    """Renderer::draw over several GPUs of one process (rt_multi_*): the
    scene (on devices[0]) is replicated on the other devices, the frame is cut
    into row bands (band b -> slot b mod n, as the reference's draw splits rows
    over OpenMP threads, raytracing.cpp:77-96), each slot renders its bands on
    its own stream and one gather per frame (RCCL ncclGather for distinct
    devices, peer copies when a device repeats) assembles it on devices[0]."""

    RCCL, PEER_COPY = 1, 2

    def __init__(self, scene: IScene, devices, band_rows: int = 8):
        devs = (C.c_int32 * len(devices))(*[int(d) for d in devices])
        h = C.c_void_p()
        check(lib().rt_multi_create(scene._handle(), devs, len(devices), int(band_rows), C.byref(h)))
        self._h = h
        self.scene = scene  # the root scene must outlive the handle

    def info(self):
        """-> (slots, exchange (MultiRenderer.RCCL / PEER_COPY), band_rows)."""
        n, x, b = C.c_int32(0), C.c_int32(0), C.c_int32(0)
        check(lib().rt_multi_info(self._h, C.byref(n), C.byref(x), C.byref(b)))
        return n.value, x.value, b.value

    def render(self, params: RenderParams, color: np.ndarray, t: np.ndarray, clear: bool = False,
               cleared: bool = False) -> float:
        """The same contract as IScene.render (host buffers); returns the device
        time from the first launch to the assembled frame, in ms."""
        H, W = color.shape
        assert color.dtype == np.uint32 and t.dtype == np.float32 and t.shape == color.shape
        assert color.flags.c_contiguous and t.flags.c_contiguous
        ms = C.c_float(0.0)
        flags = (RT_FLAG_CLEAR | RT_FLAG_HITS_ONLY) if cleared else RT_FLAG_CLEAR if clear else 0
        check(lib().rt_multi_render(self._h, C.byref(params), _p(color), _p(t), W, H, flags, C.byref(ms)))
        return ms.value

    def render_device_frames(self, params_list, color_ptrs, t_ptrs, W: int, H: int,
                             stream: int | None = None):
        """Frames into device buffers on devices[0], stream-ordered on `stream`."""
        n = len(params_list)
        arr = (RenderParams * n)(*params_list)
        cp = (C.c_void_p * n)(*color_ptrs)
        tp = (C.c_void_p * n)(*t_ptrs)
        check(lib().rt_multi_render_device_frames(self._h, arr, n, cp, tp, W, H, RT_FLAG_CLEAR,
                                                  C.c_void_p(stream) if stream else None))

    def close(self):
        if getattr(self, "_h", None):
            check(lib().rt_multi_destroy(self._h))
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# --------------------------------------------- mesh -> SDF --
class SDFMesh:
    """A triangle mesh prepared on the GPU for signed-distance queries
    (rt_sdf_mesh_*): point queries, SDFGrid lattices and sparse SDFOctrees in
    the reference's file formats (grid_raytracing.cpp:127-134,
    octree_raytracing.cpp:8-16). Generates the config-3/4 stand-ins.

    dynamic: the vertices may be moved afterwards (update_vertices*,
    RT_MESH_DYNAMIC): the handle then keeps its index array, the weld map of
    creation with its incidence lists, a vertex staging buffer and scratch on
    the device (device_bytes()), and an update recomputes tree boxes, triangle
    records and pseudonormals there."""

    def __init__(self, mesh: SimpleMesh, dynamic: bool = False):
        v = np.ascontiguousarray(mesh.vPos4f, np.float32)
        i = np.ascontiguousarray(mesh.indices, np.uint32)
        h = C.c_void_p()
        if dynamic:
            check(lib().rt_sdf_mesh_create_ex(_p(v), len(v), _p(i), len(i), RT_MESH_DYNAMIC, C.byref(h)))
        else:
            check(lib().rt_sdf_mesh_create(_p(v), len(v), _p(i), len(i), C.byref(h)))
        self._h = h
        self.ntri = len(i) // 3

    def update_vertices(self, vPos4f):
        """Move the mesh to new positions (float32 [N, 4] on the host, N as at
        creation): rt_sdf_mesh_update_vertices. Returns when the update is complete."""
        v = np.ascontiguousarray(vPos4f, np.float32)
        if v.ndim != 2 or v.shape[1] != 4:
            raise RtError(f"update_vertices: shape {v.shape}, expected [N, 4]")
        check(lib().rt_sdf_mesh_update_vertices(self._h, _p(v), len(v)))

    def update_vertices_device(self, ptr: int, nverts: int, stream: int | None = None):
        """The same from device memory (float32[4 * nverts] at ptr, e.g. a torch
        tensor's data_ptr()), queued on `stream` after the work already there:
        rt_sdf_mesh_update_vertices_device. The call only launches."""
        check(lib().rt_sdf_mesh_update_vertices_device(self._h, C.c_void_p(ptr) if ptr else None, int(nverts),
                                                       C.c_void_p(stream) if stream else None))

    def pseudonormals(self) -> np.ndarray:
        """The pseudonormals the device holds now, float32 [T, 7, 4] (features
        0..2 vertex a, b, c; 3 ab; 4 ac; 5 bc; 6 face), after one device
        synchronisation: rt_sdf_mesh_get_pseudonormals."""
        pn = np.empty((self.ntri, 7, 4), np.float32)
        check(lib().rt_sdf_mesh_get_pseudonormals(self._h, _p(pn), self.ntri))
        return pn

    def device_bytes(self) -> int:
        """Bytes of the handle's mesh arrays on the device (rt_sdf_mesh_device_bytes)."""
        n = int(lib().rt_sdf_mesh_device_bytes(self._h))
        if n < 0:
            check(n)
        return n

    def points(self, p3) -> np.ndarray:
        p3 = np.ascontiguousarray(p3, np.float32).reshape(-1, 3)
        out = np.empty(len(p3), np.float32)
        check(lib().rt_sdf_mesh_points(self._h, _p(p3), len(p3), _p(out)))
        return out

    def grid(self, size):
        """-> (size uint32[3], values float32[sx*sy*sz]) as SDFGrid holds them."""
        size = np.ascontiguousarray(np.broadcast_to(np.asarray(size, np.uint32), (3,)))
        vals = np.empty(int(size[0]) * int(size[1]) * int(size[2]), np.float32)
        check(lib().rt_sdf_mesh_grid(self._h, _p(size), _p(vals)))
        return size, vals

    def device(self) -> int:
        """HIP device the mesh was prepared on."""
        return int(lib().rt_sdf_mesh_device(self._h))

    def points_device(self, point_ptr: int, n: int, *, radius: float = float("inf"), radius_ptr: int | None = None,
                      dist_ptr: int | None = None, closest_ptr: int | None = None, prim_ptr: int | None = None,
                      feature_ptr: int | None = None, unsigned: bool = False, stream: int | None = None):
        """Closest point and signed distance on device buffers
        (rt_sdf_mesh_points_device): n points at point_ptr (float32[3n], e.g.
        a torch tensor's data_ptr()), queried in stream order on `stream`; the
        call only launches. Outputs left None are neither computed nor written
        (float32 dist, float32[3n] closest, int64 prim, int32 feature). Only
        triangles within `radius` count (radius_ptr: float32[n], one per
        point); a point without one gets +inf, itself, -1 and -1. unsigned:
        the distance without its sign (the pseudonormals are not read)."""
        b = PointBatch(int(n), point_ptr or None, radius_ptr or None, float(radius), dist_ptr or None,
                       closest_ptr or None, prim_ptr or None, feature_ptr or None)
        check(lib().rt_sdf_mesh_points_device(self._h, C.byref(b), RT_POINTS_UNSIGNED if unsigned else 0,
                                              C.c_void_p(stream) if stream else None))

    def grid_device(self, size, ptr: int, stream: int | None = None):
        """grid() into a device buffer of sx*sy*sz float32 at `ptr`
        (rt_sdf_mesh_grid_device), queued on `stream`; the call only launches."""
        size = np.ascontiguousarray(np.broadcast_to(np.asarray(size, np.uint32), (3,)))
        check(lib().rt_sdf_mesh_grid_device(self._h, _p(size), C.c_void_p(ptr) if ptr else None,
                                            C.c_void_p(stream) if stream else None))

    def octree(self, depth: int) -> np.ndarray:
        """-> raw nodes, uint8 [count*36] (SDFOctreeNode records, BFS)."""
        n = C.c_int64(0)
        check(lib().rt_sdf_mesh_octree(self._h, int(depth), C.byref(n), None))
        buf = np.empty(n.value * 36, np.uint8)
        check(lib().rt_sdf_mesh_octree(self._h, int(depth), C.byref(n), _p(buf)))
        return buf

    def octree_device(self, scene: "SDFOctree", stream: int | None = None):
        """Rebuild `scene` (SDFOctree.dynamic) on the device as the octree of
        the mesh as it is now, at the scene's depth, queued on `stream`
        (rt_sdf_mesh_octree_device); the call only launches. A tree that
        passes the scene's capacity is dropped: scene.status()."""
        check(lib().rt_sdf_mesh_octree_device(self._h, scene._handle() if scene is not None else None,
                                              C.c_void_p(stream) if stream else None))

    def close(self):
        if getattr(self, "_h", None):
            check(lib().rt_sdf_mesh_destroy(self._h))
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def subdivide_mesh(mesh: SimpleMesh, levels: int) -> SimpleMesh:
    """Midpoint subdivision (rt_mesh_subdivide): the config-5 stand-in mesh."""
    L = lib()
    v = np.ascontiguousarray(mesh.vPos4f, np.float32)
    i = np.ascontiguousarray(mesh.indices, np.uint32)
    nv, ni = C.c_int64(0), C.c_int64(0)
    check(L.rt_mesh_subdivide(_p(v), len(v), _p(i), len(i), int(levels), None, C.byref(nv), None,
                              C.byref(ni)))
    ov = np.empty((nv.value, 4), np.float32)
    oi = np.empty(ni.value, np.uint32)
    check(L.rt_mesh_subdivide(_p(v), len(v), _p(i), len(i), int(levels), _p(ov), C.byref(nv), _p(oi),
                              C.byref(ni)))
    return SimpleMesh(ov, oi)
