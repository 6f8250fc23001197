"""Ray queries on torch tensors: IScene::intersect (raytracing.hpp:77-79) for
rays that already live on the GPU, through rt_trace_rays_device.

    from rtamd import torch_rays
    r = torch_rays.trace(scene, origins, dirs, outputs=("hit", "t"))

The launch is queued on torch.cuda.current_stream(): it is ordered with the
torch work around it, and nothing is copied or synchronised. torch is
imported when trace() is called, so ``import rtamd`` stays torch-free.

    torch_rays.update_vertices(scene, verts)

moves the vertices of a dynamic mesh scene (BVHBuilder(mesh, dynamic=True))
to a tensor's positions: the BVH8 refit of rt_scene_update_vertices_device, on
the same stream.

    torch_rays.update_instances(scene, xforms, first=0)

gives an rtamd.InstancedScene new poses from a tensor of object-to-world
matrices (rt_scene_update_instances_device: one small kernel on the same
stream, nothing else), and split_prim() takes such a scene's primitive ids
apart into (instance, triangle).

    o, d = torch_rays.eye_rays(params, W, H)
    r = torch_rays.shade(scene, o, d, params)

is the renderer's colour for rays on the GPU (rt_eye_rays_device,
rt_shade_rays_device): eye_rays writes the frame's eye rays as a ray batch, and
shade runs the reference's shading (Lambert with its shadow ray and reflection
bounce, Color, Normal) on any rays, for every scene kind. Eye rays plus shade
is a frame; for an rtamd.InstancedScene it is the way to a picture.

    h = torch_rays.closest(sdf_mesh, points, radius=0.05, outputs=("dist", "closest", "prim"))
    g = torch_rays.sdf_grid(sdf_mesh, (128, 128, 64))

are the point queries of an rtamd.SDFMesh (rt_sdf_mesh_points_device,
rt_sdf_mesh_grid_device): signed distance, closest point, triangle and Voronoi
feature of points on the GPU, optionally only within a radius, and the
SDFGrid lattice as a tensor. torch_rays.update_sdf_mesh(sdf_mesh, verts) moves
an SDFMesh(mesh, dynamic=True) to new vertex positions on the current stream
(rt_sdf_mesh_update_vertices_device), ahead of the queries queued after it.
"""
from __future__ import annotations

from dataclasses import dataclass

from ._lib import lib

OUTPUTS = ("hit", "t", "normal", "prim")
SHADE_OUTPUTS = ("color", "t", "hit", "prim")
POINT_OUTPUTS = ("dist", "closest", "prim", "feature")


@dataclass
class RayHits:
    """The requested outputs of one trace() ([N] tensors on the rays' device;
    normal is [N,3]); the others are None."""
    hit: "object | None" = None      # torch.int32, 0 / 1
    t: "object | None" = None        # torch.float32, +inf on a miss
    normal: "object | None" = None   # torch.float32 [N,3], (0,1,0) on a miss, not flipped
    prim: "object | None" = None     # torch.int64, include/rtamd.h's primitive id


@dataclass
class RayColors:
    """The outputs of one shade() ([N] tensors on the rays' device); the ones
    not requested are None."""
    color: "object | None" = None    # torch.int32: the RGBA8 word, R in the low byte (view it as uint8 [N,4])
    t: "object | None" = None        # torch.float32
    hit: "object | None" = None      # torch.int32, 1 where a colour was stored
    prim: "object | None" = None     # torch.int64, the first intersection's primitive id (-2 plane, -1 miss)


@dataclass
class PointHits:
    """The requested outputs of one closest() ([N] tensors on the points'
    device; closest is [N,3]); the others are None."""
    dist: "object | None" = None     # torch.float32, signed (or |.| with unsigned); +inf where nothing is within the radius
    closest: "object | None" = None  # torch.float32 [N,3], the point itself where nothing is within the radius
    prim: "object | None" = None     # torch.int64, original triangle index, -1 = none
    feature: "object | None" = None  # torch.int32, 0..2 vertex a,b,c; 3 ab; 4 ac; 5 bc; 6 face; -1 = none


def _rays(torch, x, what, device):
    if not isinstance(x, torch.Tensor):
        raise ValueError(f"{what}: expected a torch tensor, got {type(x).__name__}")
    if x.dtype != torch.float32:
        raise ValueError(f"{what}: dtype {x.dtype}, expected torch.float32")
    if x.dim() != 2 or x.shape[1] != 3:
        raise ValueError(f"{what}: shape {tuple(x.shape)}, expected [N, 3]")
    if x.device.type != "cuda" or x.device.index != device:
        raise ValueError(f"{what}: on {x.device}, the scene is on HIP device {device}")
    if not x.is_contiguous():
        raise ValueError(f"{what}: not contiguous")
    return x


def _interval(torch, x, what, n, device):
    """-> (scalar, pointer): a float, or a float32 [N] tensor on the device."""
    if not isinstance(x, torch.Tensor):
        return float(x), None
    if x.dtype != torch.float32 or x.dim() != 1 or x.shape[0] != n:
        raise ValueError(f"{what}: {x.dtype} {tuple(x.shape)}, expected a float or torch.float32 [{n}]")
    if x.device.type != "cuda" or x.device.index != device:
        raise ValueError(f"{what}: on {x.device}, the scene is on HIP device {device}")
    if not x.is_contiguous():
        raise ValueError(f"{what}: not contiguous")
    return 0.0, x


def update_vertices(scene, verts) -> None:
    """Refit a dynamic mesh scene (rtamd.BVHBuilder(mesh, dynamic=True)) to the
    positions in `verts`, a contiguous float32 tensor on the scene's device
    with one row per creation vertex: [V, 4] (x, y, z, w) is read in place;
    [V, 3] gets a w = 1 column through torch first -- the one allocation, a
    [V, 4] tensor. The refit is queued on torch.cuda.current_stream(), after
    the torch kernels that produced `verts` there, and the call returns after
    its one host wait (rt_scene_update_vertices_device). Raises ValueError on a
    bad tensor before anything is launched."""
    import torch

    device = int(lib().rt_scene_device(scene._handle()))
    if not isinstance(verts, torch.Tensor):
        raise ValueError(f"verts: expected a torch tensor, got {type(verts).__name__}")
    if verts.dtype != torch.float32:
        raise ValueError(f"verts: dtype {verts.dtype}, expected torch.float32")
    if verts.dim() != 2 or verts.shape[1] not in (3, 4) or verts.shape[0] == 0:
        raise ValueError(f"verts: shape {tuple(verts.shape)}, expected [V, 4] or [V, 3]")
    if verts.device.type != "cuda" or verts.device.index != device:
        raise ValueError(f"verts: on {verts.device}, the scene is on HIP device {device}")
    if not verts.is_contiguous():
        raise ValueError("verts: not contiguous")
    with torch.cuda.device(device):
        if verts.shape[1] == 3:
            verts = torch.cat([verts, verts.new_ones((verts.shape[0], 1))], dim=1)
        scene.update_vertices_device(verts.data_ptr(), verts.shape[0],
                                     stream=torch.cuda.current_stream(device).cuda_stream)


def update_sdf_mesh(sdf_mesh, verts) -> None:
    """Move a dynamic rtamd.SDFMesh (SDFMesh(mesh, dynamic=True)) to the
    positions in `verts`, with the tensor rules of update_vertices: a
    contiguous float32 tensor on the handle's device with one row per creation
    vertex, [V, 4] (x, y, z, w) read in place or [V, 3], which gets a w = 1
    column through torch first. The update is queued on
    torch.cuda.current_stream(), after the torch kernels that produced `verts`
    there and before the queries queued there afterwards
    (rt_sdf_mesh_update_vertices_device); the call only launches, with no host
    wait. Raises ValueError on a bad tensor before anything is launched."""
    import torch

    device = sdf_mesh.device()
    if not isinstance(verts, torch.Tensor):
        raise ValueError(f"verts: expected a torch tensor, got {type(verts).__name__}")
    if verts.dtype != torch.float32:
        raise ValueError(f"verts: dtype {verts.dtype}, expected torch.float32")
    if verts.dim() != 2 or verts.shape[1] not in (3, 4) or verts.shape[0] == 0:
        raise ValueError(f"verts: shape {tuple(verts.shape)}, expected [V, 4] or [V, 3]")
    if verts.device.type != "cuda" or verts.device.index != device:
        raise ValueError(f"verts: on {verts.device}, the mesh is on HIP device {device}")
    if not verts.is_contiguous():
        raise ValueError("verts: not contiguous")
    with torch.cuda.device(device):
        if verts.shape[1] == 3:
            verts = torch.cat([verts, verts.new_ones((verts.shape[0], 1))], dim=1)
        sdf_mesh.update_vertices_device(verts.data_ptr(), verts.shape[0],
                                        stream=torch.cuda.current_stream(device).cuda_stream)


def update_instances(scene, xforms, first: int = 0) -> None:
    """New poses for instances first .. first + K - 1 of an
    rtamd.InstancedScene from `xforms`, a contiguous float32 [K, 3, 4] or
    [K, 12] tensor of object-to-world matrices (row-major 3x4) on the scene's
    device. The inversion kernel is queued on torch.cuda.current_stream(),
    after the torch kernels that produced `xforms` there; the call only
    launches. A singular or non-finite matrix cannot be refused (the data is
    on the device): its instance is skipped by every query until its next
    update. Raises ValueError on a bad tensor or range before anything is
    launched."""
    import torch

    device = int(lib().rt_scene_device(scene._handle()))
    if not isinstance(xforms, torch.Tensor):
        raise ValueError(f"xforms: expected a torch tensor, got {type(xforms).__name__}")
    if xforms.dtype != torch.float32:
        raise ValueError(f"xforms: dtype {xforms.dtype}, expected torch.float32")
    if not ((xforms.dim() == 3 and tuple(xforms.shape[1:]) == (3, 4)) or (xforms.dim() == 2 and xforms.shape[1] == 12)):
        raise ValueError(f"xforms: shape {tuple(xforms.shape)}, expected [K, 3, 4] or [K, 12]")
    if xforms.device.type != "cuda" or xforms.device.index != device:
        raise ValueError(f"xforms: on {xforms.device}, the scene is on HIP device {device}")
    if not xforms.is_contiguous():
        raise ValueError("xforms: not contiguous")
    k = int(xforms.shape[0])
    if first < 0 or first + k > len(scene):
        raise ValueError(f"instances [{first}, {first + k}) outside the scene's {len(scene)}")
    if k == 0:
        return
    with torch.cuda.device(device):
        scene.update_instances_device(xforms.data_ptr(), k, first=int(first),
                                      stream=torch.cuda.current_stream(device).cuda_stream)


def split_prim(prim):
    """(instance, triangle) of an InstancedScene's primitive ids (an int64
    tensor or numpy array): prim = (instance << 32) | triangle on a hit.
    Misses (-1) and the plane (-2) give instance -1 and triangle -1 / -2.
    The low word is what the instance's BLAS kind reports: original triangle
    id (mesh), c0 cell (SDFGrid) or leaf node (SDFOctree)."""
    neg = prim < 0
    inst = prim >> 32  # arithmetic shift: -1 for the negative ids
    tri = prim & 0xFFFFFFFF
    return inst, tri * (~neg) + prim * neg


def trace(scene, origins, dirs, tnear=0.01, tfar=100.0, any_hit=False, outputs=OUTPUTS) -> RayHits:
    """Closest hit (or, with any_hit, the hit flag alone) of N rays against
    `scene` (an rtamd.IScene). origins, dirs: contiguous float32 [N,3] tensors
    on the scene's device (dirs are used as given, not normalised); tnear,
    tfar: floats or float32 [N] tensors. Only the outputs named are computed
    and allocated (torch.empty); any_hit allows "hit" alone. Raises ValueError
    on a bad tensor before anything is launched."""
    import torch

    device = int(lib().rt_scene_device(scene._handle()))
    o = _rays(torch, origins, "origins", device)
    d = _rays(torch, dirs, "dirs", device)
    if o.shape != d.shape:
        raise ValueError(f"origins {tuple(o.shape)} and dirs {tuple(d.shape)} differ in shape")
    n = o.shape[0]
    tn, tn_t = _interval(torch, tnear, "tnear", n, device)
    tf, tf_t = _interval(torch, tfar, "tfar", n, device)
    outputs = tuple(outputs)
    if not outputs or any(k not in OUTPUTS for k in outputs) or len(set(outputs)) != len(outputs):
        raise ValueError(f"outputs {outputs}: a non-empty selection of {OUTPUTS}")
    if any_hit:
        if outputs not in (OUTPUTS, ("hit",)):  # (the default selection means "hit" here)
            raise ValueError('any_hit writes the hit flag only: outputs must be ("hit",)')
        outputs = ("hit",)
    kinds = {"hit": ((n,), torch.int32), "t": ((n,), torch.float32), "normal": ((n, 3), torch.float32),
             "prim": ((n,), torch.int64)}
    r = RayHits(**{k: torch.empty(kinds[k][0], dtype=kinds[k][1], device=o.device) for k in outputs})
    ptr = lambda x: x.data_ptr() if x is not None and x.numel() else None
    if n == 0:
        return r
    with torch.cuda.device(device):
        scene.trace_device(o.data_ptr(), d.data_ptr(), n, hit_ptr=ptr(r.hit), t_ptr=ptr(r.t),
                           normal_ptr=ptr(r.normal), prim_ptr=ptr(r.prim), tnear=tn, tfar=tf,
                           tnear_ptr=ptr(tn_t), tfar_ptr=ptr(tf_t), any_hit=any_hit,
                           stream=torch.cuda.current_stream(device).cuda_stream)
    return r


def eye_rays(params, W: int, H: int, device=None):
    """The eye rays of the W x H frame `params` (an rtamd.RenderParams)
    describes, as a ray batch: (origins, dirs), float32 [W*H, 3] each, ray
    y * W + x being pixel (x, y) of the rendered frame. The directions are the
    ones the frame kernels trace, bit for bit; the origins are camera_pos.
    Written by one kernel on torch.cuda.current_stream() of `device` (default:
    the current one)."""
    import torch

    dev = torch.device("cuda", device) if isinstance(device, int) else torch.device(device or "cuda")
    if dev.type != "cuda":
        raise ValueError(f"device {dev}: eye rays are written on a HIP device")
    if dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    W, H = int(W), int(H)
    if W <= 0 or H <= 0:
        raise ValueError(f"frame size {W} x {H}")
    o = torch.empty((W * H, 3), dtype=torch.float32, device=dev)
    d = torch.empty((W * H, 3), dtype=torch.float32, device=dev)
    from .api import eye_rays_device
    with torch.cuda.device(dev):
        eye_rays_device(params, W, H, o.data_ptr(), d.data_ptr(), stream=torch.cuda.current_stream(dev).cuda_stream)
    return o, d


def _given(torch, x, what, dtype, n, device):
    if not isinstance(x, torch.Tensor) or x.dtype != dtype or x.dim() != 1 or x.shape[0] != n:
        raise ValueError(f"{what}: expected a {dtype} [{n}] tensor")
    if x.device.type != "cuda" or x.device.index != device:
        raise ValueError(f"{what}: on {x.device}, the scene is on HIP device {device}")
    if not x.is_contiguous():
        raise ValueError(f"{what}: not contiguous")
    return x


def shade(scene, origins, dirs, params, tnear=0.01, tfar=100.0, clear=True, color=None, t=None,
          outputs=("color", "t")) -> RayColors:
    """The renderer's colour of N rays against `scene` (an rtamd.IScene of any
    kind, its plane included): Renderer::intersectionColor under `params`
    (light, shading mode, shadow and reflection switches), packed as the frame
    kernels pack it. origins, dirs, tnear, tfar: as trace(). "color" is always
    produced; outputs selects what else is ("t", "hit", "prim").

    clear=True: every ray is written (a miss: colour 0, t = +inf). clear=False:
    a miss writes neither colour nor t, so the buffers must hold something --
    pass them as color (int32 [N]) and t (float32 [N]); they are written in
    place and returned. tfar may be that same t tensor: each ray then only
    accepts a hit in front of what the buffers hold, and several scenes shaded
    one after another compose by depth (the reference's tPrev). Queued on
    torch.cuda.current_stream(); raises ValueError on a bad tensor before
    anything is launched."""
    import torch

    device = int(lib().rt_scene_device(scene._handle()))
    o = _rays(torch, origins, "origins", device)
    d = _rays(torch, dirs, "dirs", device)
    if o.shape != d.shape:
        raise ValueError(f"origins {tuple(o.shape)} and dirs {tuple(d.shape)} differ in shape")
    n = o.shape[0]
    tn, tn_t = _interval(torch, tnear, "tnear", n, device)
    tf, tf_t = _interval(torch, tfar, "tfar", n, device)
    outputs = tuple(outputs)
    if any(k not in SHADE_OUTPUTS for k in outputs) or len(set(outputs)) != len(outputs):
        raise ValueError(f"outputs {outputs}: a selection of {SHADE_OUTPUTS}")
    if not clear and color is None:
        raise ValueError("clear=False leaves the rays that miss unwritten: pass the color (and t) tensors to keep")
    r = RayColors()
    r.color = torch.empty((n,), dtype=torch.int32, device=o.device) if color is None else \
        _given(torch, color, "color", torch.int32, n, device)
    if t is not None:
        r.t = _given(torch, t, "t", torch.float32, n, device)
    elif "t" in outputs:
        if not clear:
            raise ValueError("clear=False with a fresh t tensor: pass t")
        r.t = torch.empty((n,), dtype=torch.float32, device=o.device)
    if "hit" in outputs:
        r.hit = torch.empty((n,), dtype=torch.int32, device=o.device)
    if "prim" in outputs:
        r.prim = torch.empty((n,), dtype=torch.int64, device=o.device)
    ptr = lambda x: x.data_ptr() if x is not None and x.numel() else None
    if n == 0:
        return r
    with torch.cuda.device(device):
        scene.shade_device(o.data_ptr(), d.data_ptr(), n, params, r.color.data_ptr(), t_ptr=ptr(r.t),
                           hit_ptr=ptr(r.hit), prim_ptr=ptr(r.prim), tnear=tn, tfar=tf, tnear_ptr=ptr(tn_t),
                           tfar_ptr=ptr(tf_t), clear=bool(clear),
                           stream=torch.cuda.current_stream(device).cuda_stream)
    return r


def closest(sdf_mesh, points, radius=float("inf"), outputs=("dist",), unsigned=False) -> PointHits:
    """The closest triangle of `sdf_mesh` (an rtamd.SDFMesh) to each of N
    points: a contiguous float32 [N,3] tensor on the mesh's device. radius: a
    float (>= 0, +inf = unbounded) or a float32 [N] tensor; only triangles
    within it count, and a point without one (also one with a negative or NaN
    radius) gets dist +inf, itself as closest, prim -1 and feature -1. Only
    the outputs named are computed and allocated (torch.empty); unsigned
    gives the distance without its sign. The exact definition is
    include/rtamd.h's. Queued on torch.cuda.current_stream(); raises
    ValueError on a bad tensor or radius before anything is launched."""
    import math

    import torch

    device = sdf_mesh.device()
    p = _rays(torch, points, "points", device)
    n = p.shape[0]
    r, r_t = _interval(torch, radius, "radius", n, device)
    if r_t is None and (math.isnan(r) or r < 0.0):
        raise ValueError(f"radius {r}: expected >= 0 (inf = unbounded)")
    outputs = tuple(outputs)
    if not outputs or any(k not in POINT_OUTPUTS for k in outputs) or len(set(outputs)) != len(outputs):
        raise ValueError(f"outputs {outputs}: a non-empty selection of {POINT_OUTPUTS}")
    kinds = {"dist": ((n,), torch.float32), "closest": ((n, 3), torch.float32), "prim": ((n,), torch.int64),
             "feature": ((n,), torch.int32)}
    h = PointHits(**{k: torch.empty(kinds[k][0], dtype=kinds[k][1], device=p.device) for k in outputs})
    ptr = lambda x: x.data_ptr() if x is not None and x.numel() else None
    if n == 0:
        return h
    with torch.cuda.device(device):
        sdf_mesh.points_device(p.data_ptr(), n, radius=r, radius_ptr=ptr(r_t), dist_ptr=ptr(h.dist),
                               closest_ptr=ptr(h.closest), prim_ptr=ptr(h.prim), feature_ptr=ptr(h.feature),
                               unsigned=bool(unsigned), stream=torch.cuda.current_stream(device).cuda_stream)
    return h


def sdf_grid(sdf_mesh, size):
    """SDFMesh.grid as a tensor: the signed distance on a size[0] x size[1] x
    size[2] lattice over [-1,1]^3 (sample i at 2i/(size-1)-1 per axis; an int
    means a cube), float32 [sx, sy, sz] on the mesh's device, written by one
    kernel on torch.cuda.current_stream() (rt_sdf_mesh_grid_device). Raises
    ValueError on a size outside [2, 4096] before anything is launched."""
    import torch

    device = sdf_mesh.device()
    size = tuple(int(x) for x in ((size,) * 3 if isinstance(size, int) else size))
    if len(size) != 3 or any(x < 2 or x > 4096 for x in size):
        raise ValueError(f"size {size}: three lattice sizes in [2, 4096]")
    g = torch.empty(size, dtype=torch.float32, device=torch.device("cuda", device))
    with torch.cuda.device(device):
        sdf_mesh.grid_device(size, g.data_ptr(), stream=torch.cuda.current_stream(device).cuda_stream)
    return g


def update_sdf_grid(scene, values) -> None:
    """New values for an rtamd.SDFGrid from a tensor (SDFGrid.update_device,
    rt_scene_update_grid_device): `values` is a contiguous float32 tensor on
    the scene's device with the scene's sx * sy * sz samples in the layout of
    sdf_grid ([sx, sy, sz] or flat). The copy is queued on
    torch.cuda.current_stream(), after the torch kernels that produced `values`
    there and before the frames and ray queries queued there afterwards; the
    call only launches. Raises ValueError on a bad tensor before anything is
    launched."""
    import torch

    device = int(lib().rt_scene_device(scene._handle()))
    n = int(scene.size[0]) * int(scene.size[1]) * int(scene.size[2])
    if not isinstance(values, torch.Tensor):
        raise ValueError(f"values: expected a torch tensor, got {type(values).__name__}")
    if values.dtype != torch.float32:
        raise ValueError(f"values: dtype {values.dtype}, expected torch.float32")
    if values.numel() != n:
        raise ValueError(f"values: {values.numel()} samples, the scene's size {tuple(int(x) for x in scene.size)} has {n}")
    if values.device.type != "cuda" or values.device.index != device:
        raise ValueError(f"values: on {values.device}, the scene is on HIP device {device}")
    if not values.is_contiguous():
        raise ValueError("values: not contiguous")
    with torch.cuda.device(device):
        scene.update_device(values.data_ptr(), stream=torch.cuda.current_stream(device).cuda_stream)


def update_sdf_octree(sdf_mesh, scene) -> None:
    """Rebuild an rtamd.SDFOctree.dynamic scene from an rtamd.SDFMesh as it is
    now (SDFMesh.octree_device, rt_sdf_mesh_octree_device), queued on
    torch.cuda.current_stream(): behind an update_sdf_mesh queued there before,
    ahead of the ray queries queued there afterwards; the call only launches.
    scene.status() tells afterwards whether the tree fitted."""
    import torch

    device = sdf_mesh.device()
    with torch.cuda.device(device):
        sdf_mesh.octree_device(scene, stream=torch.cuda.current_stream(device).cuda_stream)
