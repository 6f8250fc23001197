/* rtamd.h -- C ABI of the MI355X-native primary-ray renderer.
 *
 * Drop-in boundary for the per-pixel intersection hot path of
 * iMacsimus/Triangles-SDF-CPU-RayTracing (reference @ 2025-07-04). The reference
 * has no FFI for this path other than the per-node ISPC exports
 * (src/ray_pack.ispc:220,242,290); a per-node call across a device boundary is
 * infeasible, so the boundary sits at FRAME granularity, mirroring
 *     float Renderer::draw(const IScene&, FrameBuffer&, const Camera&,
 *                          const float4x4 projInv) const       (src/raytracing.hpp:109-110)
 * and, for ray-level checks,
 *     virtual HitInfo IScene::intersect(rayPos, rayDir, tNear, tFar) const
 *                                                           (src/raytracing.hpp:77-79)
 *
 * Plain C types only: pointers + sizes, no torch, no HIP types in signatures
 * (streams are passed as void*). Every entry point returns 0 on success or a
 * negative RT_E* code; rt_last_error() gives a message (thread-local).
 * Nothing throws across the ABI.
 */
#ifndef RTAMD_H
#define RTAMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RTAMD_ABI_VERSION 8

enum rt_status {
  RT_OK = 0,
  RT_E_INVALID = -1,   /* bad argument */
  RT_E_IO = -2,        /* file missing / truncated */
  RT_E_DEVICE = -3,    /* HIP runtime error (no GPU, OOM, launch failure) */
  RT_E_STATE = -4      /* wrong scene kind for the call */
};

/* ShadingMode, same order as the reference enum (src/raytracing.hpp:99). */
enum rt_shading_mode { RT_SHADING_NORMAL = 0, RT_SHADING_LAMBERT = 1, RT_SHADING_COLOR = 2 };

enum rt_scene_kind { RT_SCENE_MESH = 1, RT_SCENE_GRID = 2, RT_SCENE_OCTREE = 3, RT_SCENE_INSTANCED = 4 };

/* rt_render flags */
#define RT_FLAG_CLEAR 1u /* treat the framebuffer as FrameBuffer::clear()ed (color=0, t=+inf;
                            src/raytracing.hpp:16-19) and write every pixel: clear+draw fused.
                            Without it, t is read as tPrev and color/t are written only on hit
                            (src/raytracing.cpp:89-94). */
#define RT_FLAG_TILE_NATURAL 2u /* with a tile: write this rank's bands at their own rows of a
                                   full W*H frame (e.g. rank 0's frame mapped over xGMI by
                                   rt_ipc_open) instead of packed */
#define RT_FLAG_HITS_ONLY 4u /* with RT_FLAG_CLEAR: the frame is already cleared (rt_clear_device,
                                or FrameBuffer::clear() for rt_render's host buffers), so only hit
                                pixels are stored -- the same image as CLEAR alone, with misses
                                costing no stores (no xGMI traffic for background; for rt_render,
                                only the hits' bounding box is copied back) */

typedef struct rt_scene rt_scene; /* opaque: owns the device copy of one scene on one GPU */
typedef struct rt_sdf_mesh rt_sdf_mesh; /* opaque: a triangle mesh prepared for SDF queries */

/* Per-frame parameters. Matrices are column-major float[16] (LiteMath float4x4
 * m_col[4] layout: element (r,c) at [c*4 + r]).
 *   view_inv = inverse4x4(camera.lookAtMatrix())           (src/raytracing.cpp:73-75)
 *   proj_inv = inverse4x4(perspectiveMatrix(45, W/H, 0.01, 100)) (src/main.cpp:198-201)
 * rtamd_camera() computes both exactly as the reference does. */
typedef struct rt_render_params {
  float camera_pos[3];       /* Camera::position()                          */
  float view_inv[16];
  float proj_inv[16];
  float light_pos[3];        /* Renderer::lightPos  (src/raytracing.hpp:103) */
  int32_t shading_mode;      /* rt_shading_mode     (src/raytracing.hpp:106) */
  int32_t enable_shadows;    /* Renderer::enableShadows      (:104)          */
  int32_t enable_reflections;/* Renderer::enableReflections  (:105)          */
  int32_t reserved;          /* must be 0 */
} rt_render_params;

/* Row-band tiling for multi-GPU rendering: image rows are cut into bands of
 * band_rows rows; band b belongs to rank (b % num_ranks). A rank renders only
 * its bands and writes them PACKED (its bands in increasing order, each band
 * W*band_rows pixels, the last band possibly shorter). rank=0,num_ranks=1
 * renders the full frame in natural layout. */
typedef struct rt_tile {
  int32_t band_rows;
  int32_t rank;
  int32_t num_ranks;
  int32_t reserved;
} rt_tile;

/* ---- errors / device ---------------------------------------------------- */
const char *rt_last_error(void);
int rt_abi_version(void);
/* First 16 hex digits of the sha256 of the sources this library was built
 * from (triangles-sdf-cpu-raytracing_amd/csrc/{*.cpp,*.h,*.hip} sorted, then
 * include/rtamd.h): ties a shipped binary to a source tree. */
const char *rt_build_id(void);
/* Number of visible HIP devices (0 if none); never fails. */
int rt_device_count(void);
/* Select the HIP device used by subsequent scene creation on this thread. */
int rt_set_device(int device);

/* ---- host-side inputs (loaders; mirror the reference loaders) ----------- */
/* cmesh4::LoadMeshFromObj (src/core/mesh.cpp:178-287) [+ loadAndScale,
 * src/main.cpp:326-343, when scale != 0]. Two-call protocol: call with
 * vpos4 = idx = NULL to get the counts, then with buffers of that size.
 * vpos4: float[4*nverts] (x,y,z,w), idx: uint32[nidx]. */
int rt_load_obj(const char *path, int scale, float *vpos4, int64_t *nverts, uint32_t *idx,
                int64_t *nidx);
/* loadSDFGrid (src/grid_raytracing.cpp:127-134): 12-byte header uint32 size[3],
 * then float values[size.x*size.y*size.z], index (x*sy+y)*sz+z. Two-call protocol. */
int rt_load_grid(const char *path, uint32_t size[3], float *values);
/* loadSDFOctree (src/octree_raytracing.cpp:8-16): uint32 count, then count x
 * 36-byte SDFOctreeNode {float values[8]; uint32 childrenOffset}. Two-call protocol. */
int rt_load_octree(const char *path, int64_t *count, void *nodes36);

/* Camera(pos, target, up).lookAtMatrix() inverse and perspective inverse,
 * following src/camera.cpp:36-62 + LiteMath ("unpinned"). */
int rt_camera(const float pos[3], const float target[3], const float up[3], float fovy_deg,
              float aspect, float znear, float zfar, float view_inv[16], float proj_inv[16]);

/* Host-only: build the BVH8 exactly as rt_scene_create_mesh does and export it
 * in canonical pre-order (52 x uint32 per node: isLeaf, realCount|count,
 * startIndex, 0, then the reference Box8 SoA as float bits, +inf in unused
 * slots, zeros for leaves) plus the triangle permutation (original triangle id
 * per triangle slot, i.e. BVHBuilder's reordered mesh.indices / 3). Two-call
 * protocol on *nnodes. Used to check the tree against the reference's. */
int rt_bvh_export(const float *vpos4, int64_t nverts, const uint32_t *idx, int64_t nidx,
                  uint32_t *canon, int64_t *nnodes, uint32_t *perm_tri, int32_t *max_depth);
/* Which builder rt_scene_create_mesh / rt_bvh_export use for BVHBuilder::perform
 * (src/triangles_raytracing.cpp:12-258): RT_BVH_HOST (OpenMP on the host),
 * RT_BVH_DEVICE (on the current HIP device: libstdc++'s introsort replicated
 * with parallel partitions, SAH sweeps as device scans) or RT_BVH_AUTO (the
 * device from 32,768 triangles when a device is visible). Both give the
 * identical tree. Process-wide. */
enum rt_bvh_builder { RT_BVH_AUTO = 0, RT_BVH_HOST = 1, RT_BVH_DEVICE = 2 };
int rt_set_bvh_builder(int mode);

/* ---- scenes ------------------------------------------------------------- */
/* BVHBuilder::perform (src/triangles_raytracing.cpp:227-258): builds the same
 * 8-wide SAH BVH on the host, then uploads a GPU layout of it. */
int rt_scene_create_mesh(const float *vpos4, int64_t nverts, const uint32_t *idx, int64_t nidx,
                         rt_scene **out);
/* The same with flags. 0: exactly rt_scene_create_mesh. RT_MESH_DYNAMIC: the
 * scene's vertices may be moved afterwards (rt_scene_update_vertices*); it
 * additionally keeps on the device the index array (nidx words) and a vertex
 * staging buffer (16 * nverts bytes), both counted in rt_scene_device_bytes.
 * Either builder (rt_set_bvh_builder) serves both. No reference counterpart:
 * the reference's meshes are immutable. */
#define RT_MESH_DYNAMIC 1u
int rt_scene_create_mesh_ex(const float *vpos4, int64_t nverts, const uint32_t *idx, int64_t nidx,
                            uint32_t flags, rt_scene **out);
/* Deforming meshes: refit the BVH8 of an RT_MESH_DYNAMIC scene to new vertex
 * positions, on the GPU. The triangle list and the tree topology stay;
 * nverts must equal the creation value. Afterwards the scene is the tree of
 * the same topology over the new positions: every leaf triangle is rewritten
 * (v /= v.w, e1 = v1 - v0, e2 = v2 - v0, its original index kept) and every
 * child box is the exact min/max of its subtree, so a query finds the same
 * closest hit as on a freshly built scene of the new mesh. (As between any two
 * valid trees, the answers can differ where two triangles give bit-equal t,
 * and for a triangle hit before tNear: the reference's triangle test has no t
 * range, so such a hit is reported when its leaf's box reaches into [tNear,
 * tFar], which depends on the leaf's other triangles.)
 * A refit keeps the old split decisions: a heavily deformed mesh
 * traverses slower than a fresh build of it, and destroy + create is the
 * remedy (README.md has the measured trade).
 *   rt_scene_update_vertices         vpos4 is a host buffer (copied through
 *                                    the scene's staging buffer).
 *   rt_scene_update_vertices_device  d_vpos4 is device memory on the scene's
 *       device, which must be the current one; the kernels are queued on
 *       `stream` (hipStream_t or NULL) after the work already there, so the
 *       buffer may be the output of the caller's previous kernel on it.
 * Both return after ONE host wait: the scene constants the host keeps (root
 * box, the tile cull's bounds, the reciprocal's direction bound) are read back
 * from the refitted tree, and the call waits for that copy. Every later call
 * on any stream therefore sees the updated scene; the caller orders the
 * update after earlier work that still uses the scene on OTHER streams.
 * Nothing is allocated per call. Vertex values are not validated (device data
 * cannot be without a readback): topology is never touched, so no value can
 * make a traversal index out of bounds; NaN or infinite positions give boxes
 * and triangles that rays miss or hit as the arithmetic says.
 * Errors: RT_E_INVALID for a NULL scene or pointer, nverts <= 0 or another
 * nverts than at creation; RT_E_STATE for a scene that is not a mesh or was
 * not created with RT_MESH_DYNAMIC. A refused call leaves the scene as it was. */
int rt_scene_update_vertices(rt_scene *s, const float *vpos4, int64_t nverts);
int rt_scene_update_vertices_device(rt_scene *s, const float *d_vpos4, int64_t nverts, void *stream);
/* SDFGrid (src/grid_raytracing.hpp:10-21). values: x-major, float[sx*sy*sz]. */
int rt_scene_create_grid(const uint32_t size[3], const float *values, rt_scene **out);
/* SDFOctree (src/octree_raytracing.hpp:20-47). nodes36: count x 36 bytes. */
int rt_scene_create_octree(const void *nodes36, int64_t count, rt_scene **out);
/* SceneUnion(scene, Plane(normal, offset)) (src/raytracing.hpp:83-97,119-186;
 * src/main.cpp:189-190). enabled=0 renders the scene alone. */
int rt_scene_set_plane(rt_scene *s, int enabled, const float normal[3], float offset);
int rt_scene_kind(const rt_scene *s);
/* Device bytes held by the scene (nodes/triangles/voxels). */
int64_t rt_scene_device_bytes(const rt_scene *s);
/* Statistics of the host BVH (mesh scenes): node count, inner count, max depth. */
int rt_scene_bvh_stats(const rt_scene *s, int64_t *nodes, int64_t *inner, int32_t *max_depth);
int rt_scene_destroy(rt_scene *s);
/* A copy of scene s on another HIP device (device arrays copied device to
 * device, over xGMI between GPUs; no rebuild): the same tree, plane and kernel
 * instantiation, so every frame it renders is bitwise s's. For replicating one
 * scene on the GPUs of a single-process multi-GPU render (rt_multi_create).
 * The copy of an RT_MESH_DYNAMIC scene is a plain snapshot of its current
 * geometry: it is not dynamic and does not follow later updates (rt_multi
 * refreshes its own replicas when the root scene has been updated). */
int rt_scene_replicate(const rt_scene *s, int device, rt_scene **out);
/* HIP device the scene lives on. */
int rt_scene_device(const rt_scene *s);
/* The plane last given to rt_scene_set_plane (enabled, normal, offset). */
int rt_scene_get_plane(const rt_scene *s, int *enabled, float normal[3], float *offset);

/* ---- instanced scenes: rigid (affine) copies of mesh scenes under one query --
 * An instanced scene (RT_SCENE_INSTANCED) is a list of K >= 1 instances over
 * B >= 1 bottom-level scenes ("BLAS"): existing RT_SCENE_MESH scenes on the
 * same device, dynamic or not. Instance i is {blas index, xform[12]}; xform is
 * the object-to-world affine map, row-major 3x4:
 *     p_world[r] = x[4r]*p.x + x[4r+1]*p.y + x[4r+2]*p.z + x[4r+3].
 * The library stores its inverse M (world to object, the same layout), as
 * rt_affine_inverse computes it. No reference counterpart: the reference's
 * scenes are one mesh in one pose.
 *
 * THE ORDER IS THE DEFINITION. The reference's triangle test has no t range
 * (see rt_scene_update_vertices above: a triangle hit before tNear is reported
 * when its leaf's box reaches into [tNear, tFar]), so no order-free definition
 * is exact. For a ray (o, d, tNear, tFar), in float arithmetic without fusing:
 *     best = +inf; win = none
 *     for i = 0 .. K-1 in index order, skipping disabled (and skipped) instances:
 *         o'[r] = ((M[4r]*o.x + M[4r+1]*o.y) + M[4r+2]*o.z) + M[4r+3]
 *         d'[r] =  (M[4r]*d.x + M[4r+1]*d.y) + M[4r+2]*d.z     (not renormalised: t is shared)
 *         tf_i  = best < tFar ? best : tFar
 *         h = IScene::intersect of BLAS[blas_i] alone (its own plane ignored) on (o', d', tNear, tf_i)
 *         if h.hit and h.t < best: best = h.t; win = (i, h)    (ties keep the lower index)
 * A hit gives t = best and prim = ((int64)i << 32) | original triangle id
 * (misses stay -1, the plane -2). With n the object-space normal the BLAS
 * reports, w[c] = (M[c]*n.x + M[4+c]*n.y) + M[8+c]*n.z (the inverse transpose)
 * and normal = w / sqrt((w.x*w.x + w.y*w.y) + w.z*w.z), computed for the winner
 * only, after the loop, not flipped. The instanced scene's own plane
 * (rt_scene_set_plane, world space) takes part exactly as for the other kinds.
 * RT_RAYS_ANY_HIT is the OR over the instances of the BLAS any hit on
 * (o', d', tNear, tFar), stopping at the first hit; it equals the closest-hit
 * query's flag. A scene created by this entry is a flat
 * list: every ray visits every instance, and skips one only by the traversal's
 * own root-box test on the transformed ray, which cannot change an answer.
 * Hundreds of instances want the top-level tree of RT_INSTANCED_TLAS
 * (rt_scene_create_instanced_ex below), whose world-box test is part of that
 * mode's definition.
 *
 * rt_trace_rays_device and rt_intersect_rays accept the kind with all their
 * argument rules; rt_scene_kind, rt_scene_device, rt_scene_device_bytes (the
 * instance and BLAS tables only), rt_scene_set_plane, rt_scene_get_plane and
 * rt_scene_destroy work. Every other entry that takes a scene (rt_render*,
 * rt_bench_frames, rt_count_work, rt_scene_replicate, rt_multi_create,
 * rt_scene_update_vertices*, rt_scene_bvh_stats) returns RT_E_STATE and
 * touches nothing.
 * A BLAS refitted by rt_scene_update_vertices* is seen by the next trace: each
 * trace compares the BLAS scenes' update counters with the ones it last saw
 * and rewrites stale table entries in stream order ahead of its launch,
 * without a host wait. The caller orders BLAS and pose updates against traces
 * that are still running on OTHER streams. */
#define RT_INSTANCE_DISABLED 1u /* the instance is skipped by every query */
typedef struct rt_instance {
  int32_t blas;    /* index into the BLAS list given at creation */
  uint32_t flags;  /* 0 or RT_INSTANCE_DISABLED */
  float xform[12]; /* object to world, row-major 3x4 */
} rt_instance;
/* Host-only: inv = the inverse of the affine map xform (both row-major 3x4),
 * the one definition of M: cofactors over the determinant expanded along the
 * first row, then -(inv3 * translation) summed left to right; exact for the
 * identity, translations, power-of-two scales and signed axis permutations.
 * The device pose update runs the same code and gives the same bits.
 * RT_E_INVALID when the 3x3 determinant is zero or not finite, or when any
 * entry is not finite (inv is then untouched). */
int rt_affine_inverse(const float xform[12], float inv[12]);
/* The BLAS scenes are not owned and must outlive the handle, as with
 * rt_multi_create. The scene is created on the current device. RT_E_STATE for
 * a BLAS that is not a mesh; RT_E_INVALID for a NULL pointer, nblas or
 * ninst < 1, a blas index out of range, unknown flag bits, a BLAS on another
 * device, or a matrix rt_affine_inverse refuses. */
int rt_scene_create_instanced(rt_scene *const *blas, int32_t nblas, const rt_instance *inst, int32_t ninst,
                              rt_scene **out);
/* ---- RT_INSTANCED_TLAS: a top-level tree over the instances' world boxes ---
 * rt_scene_create_instanced_ex with flags = 0 is rt_scene_create_instanced;
 * unknown flag bits return RT_E_INVALID. For a scene created with
 * RT_INSTANCED_TLAS the loop above gains ONE line and nothing else changes:
 *     for i = 0 .. K-1 in index order, skipping disabled (and skipped) instances:
 *         tf_i = best < tFar ? best : tFar
 *         if not box_pass(wbox_i, o, d, tNear, tf_i): continue      (on the WORLD ray)
 *         ... transform, BLAS intersect under tf_i, ties keep the lower index: as above
 * RT_RAYS_ANY_HIT is the OR over the instances with box_pass(wbox_i, o, d,
 * tNear, tFar) of the BLAS any hit; box_pass is monotone in tFar, so it still
 * equals the closest-hit flag. The test is part of the
 * definition, not an approximation of the flat list's answer: the oracle of the
 * tests runs the same test. Both functions are plain float operations in the
 * written order, never fused, the same code on the host and on the device:
 *   box_pass(b = lo.xyz hi.xyz, o, d, tn, tf): false when b[0] > b[3] (the one
 *     encoding of the empty box: lo = +inf, hi = -inf). Otherwise true when a
 *     component of 1/d is not finite (a ray with a zero direction component
 *     visits every non-empty instance, as in the flat list). Otherwise, with
 *     t1 = (lo - o) * (1/d), t2 = (hi - o) * (1/d), mn(a, b) = a < b ? a : b,
 *     mx(a, b) = a > b ? a : b:
 *       tMin = mx(mx(mn(t1x, t2x), mx(mn(t1y, t2y), mn(t1z, t2z))), tn)
 *       tMax = mn(mn(mx(t1x, t2x), mn(mx(t1y, t2y), mx(t1z, t2z))), tf)
 *       pass = !(tMax < 0 || tMin > tMax)
 *     (the BVH traversal's own root-box test, on a world box).
 *   wbox_i = rt_instance_world_box(xform_i, the BLAS's root box): for corner
 *     c = 0..7 (bit a of c picks hi on axis a) p[r] = ((x[4r]*c.x + x[4r+1]*c.y)
 *     + x[4r+2]*c.z) + x[4r+3]; lo and hi folded in corner order by mn and mx;
 *     then m = max_r mx(|lo_r|, |hi_r|) + max_r (hi_r - lo_r), e = 2^-16 * m and
 *     wbox = (lo - e, hi + e). The pad is a definition, not a proof: 128 ulps of
 *     the box's own scale, where the two tests' roundings are a few ulps. An
 *     instance of a BLAS that is one leaf (no root box) has (-inf, +inf) on
 *     every axis; a disabled or skipped instance and an instance of an empty
 *     BLAS have the empty box.
 * The tree is implicit: P = the smallest power of two >= K leaves in index
 * order (leaf P + i = wbox_i, empty for i >= K), inner node n = the exact
 * min / max of nodes 2n and 2n + 1, which the monotone test lets a ray skip
 * exactly. Depth first, left to right, it yields a ray's candidates in index
 * order. ITS QUALITY IS THE SPATIAL COHERENCE OF THE CALLER'S INDEX ORDER
 * (INTEGRATION.md section 6c). The device holds the nodes (2P x 32 bytes) and
 * the object-to-world matrices (K x 48 bytes) besides the two tables;
 * rt_scene_device_bytes counts them. The boxes and the tree are recomputed on
 * the device: at creation, by rt_scene_update_instances (done on return), by
 * rt_scene_update_instances_device (queued on its stream behind the pose
 * kernel: still no allocation, no copy, no host wait) and by a trace that
 * finds a refitted BLAS (behind the rewritten table entry, on its stream). */
#define RT_INSTANCED_TLAS 1u
int rt_scene_create_instanced_ex(rt_scene *const *blas, int32_t nblas, const rt_instance *inst, int32_t ninst,
                                 uint32_t flags, rt_scene **out);
/* ---- mixed bottom-level kinds: meshes, SDF grids and SDF octrees -----------
 * rt_scene_create_instanced_any is rt_scene_create_instanced_ex (flags 0 or
 * RT_INSTANCED_TLAS, every argument rule the same) whose BLAS may also be
 * RT_SCENE_GRID and RT_SCENE_OCTREE scenes; an instanced scene as a BLAS is
 * still RT_E_STATE. When every BLAS is a mesh the call IS
 * rt_scene_create_instanced_ex: the same scene, kernels and
 * rt_scene_device_bytes. Otherwise the scene (still RT_SCENE_INSTANCED) is
 * "mixed": the device holds one 112-byte table record per BLAS instead of the
 * 56-byte mesh record, which rt_scene_device_bytes counts, and its queries run
 * kernels of their own. The definition is the loop above (THE ORDER IS THE
 * DEFINITION), read literally:
 *   - h = IScene::intersect of BLAS[blas_i] alone on (o', d', tNear, tf_i) is
 *     that BLAS kind's own entry: the answer rt_trace_rays_device gives for the
 *     BLAS scene on that ray, bit for bit;
 *   - prim = ((int64)i << 32) | p with p what the plain kind reports: the
 *     original triangle id, the grid cell, or the octree node;
 *   - the world normal is the same inverse-transpose formula on the
 *     object-space normal the BLAS reports for the winner;
 *   - for RT_INSTANCED_TLAS the box_pass line is unchanged; the object box of
 *     an SDF BLAS is (-1,-1,-1, 1,1,1), the cube both SDF kinds live in;
 *   - the flat list skips an SDF instance only by a test its own intersection
 *     makes (a mesh instance by the traversal's root-box test, as above);
 *   - RT_RAYS_ANY_HIT is the OR over the instances (with box_pass under the
 *     full tFar for RT_INSTANCED_TLAS) of the BLAS any hit under the full tFar.
 *     It equals the closest-hit flag for SDF kinds as well, and the reason needs
 *     no monotonicity of a BLAS in tFar: until a ray's first accepted hit best
 *     is +inf, so tf_i IS tFar and both loops ask every instance the same
 *     question; the first instance that answers yes sets both flags. (The
 *     composed oracle of tests/test_mixed_host.py finds 0 differing rays.)
 * d' is not renormalised. A sphere march steps by the sampled distance in
 * units of |d'|, so under a map with scale an SDF BLAS is marched with steps
 * that are too long or too short by that factor: the definition, and the bits,
 * are still the composition above, but the picture is geometrically
 * meaningful for rigid maps only (|d'| = 1 up to rounding). Meshes have no
 * such limit.
 * Every entry listed above for instanced scenes works on a mixed one with its
 * rules: rt_trace_rays_device, rt_intersect_rays, rt_shade_rays_device,
 * rt_scene_update_instances (which may move an instance to a BLAS of another
 * kind), rt_scene_update_instances_device, rt_scene_get_instances,
 * rt_scene_get_tlas, the plane, kind, device and byte getters and
 * rt_scene_destroy; a dynamic mesh BLAS refitted by rt_scene_update_vertices*
 * is seen by the next query. SDF scenes cannot change after creation. The
 * frame entries keep returning RT_E_STATE. */
int rt_scene_create_instanced_any(rt_scene *const *blas, int32_t nblas, const rt_instance *inst, int32_t ninst,
                                  uint32_t flags, rt_scene **out);
/* Host-only: the definition of an instance's world box (above). */
int rt_instance_world_box(const float xform[12], const float obox[6], float wbox[6]);
/* The tree as the device holds it, after one device synchronisation:
 * leaf_boxes[6 i ..] = wbox_i for i < K, node_boxes[6 n ..] for n < 2P (node 0
 * is not used: zeros), *leaves = P. Any output may be NULL. RT_E_STATE for a
 * scene without a top-level tree. */
int rt_scene_get_tlas(const rt_scene *s, float *leaf_boxes, float *node_boxes, int32_t *leaves);
/* Replace instances first .. first + count - 1 from a host buffer (blas, flags
 * and pose); validated as at creation, and a refused call leaves the scene
 * unchanged. The records are copied to the device before the call returns. */
int rt_scene_update_instances(rt_scene *s, int32_t first, int32_t count, const rt_instance *inst);
/* New poses from DEVICE memory: count object-to-world matrices (12 floats
 * each) at d_xform12 are inverted by a kernel queued on `stream` (hipStream_t
 * or NULL), so the buffer may be the output of the caller's previous kernel
 * there. The call only launches: no allocation, no copy, no host wait (nothing
 * the host keeps depends on a pose). The scene's device must be the current
 * one. Device data cannot be validated: an instance whose matrix
 * rt_affine_inverse would refuse is skipped by every query until its next
 * update, and an accepted matrix clears that mark. The blas index and flags
 * given at creation or by rt_scene_update_instances stay. */
int rt_scene_update_instances_device(rt_scene *s, int32_t first, int32_t count, const float *d_xform12,
                                     void *stream);
/* What the device holds for instances first .. first + count - 1, after one
 * device synchronisation: inst[j] = {blas, flags, the inverse of the stored M
 * (the given xform up to rounding; zeros for a skipped instance)}, inv12[12j ..]
 * = M itself, skipped[j] = 1 for an instance the device pose update refused.
 * Any output may be NULL. */
int rt_scene_get_instances(const rt_scene *s, int32_t first, int32_t count, rt_instance *inst, float *inv12,
                           uint32_t *skipped);

/* ---- frames ------------------------------------------------------------- */
/* Renderer::draw on HOST buffers color[W*H] (RGBA8 packed, R in the low byte)
 * and t[W*H] (row-major y*W+x). Uploads, renders, downloads, synchronises.
 * flags: 0 (t read as tPrev, write on hit), RT_FLAG_CLEAR (clear + draw, every
 * pixel written) or RT_FLAG_CLEAR | RT_FLAG_HITS_ONLY (the caller's buffers
 * already hold a cleared frame, src/main.cpp:197). Without RT_FLAG_CLEAR, or
 * with both, only the bounding box of the stored hits is copied back: the
 * other pixels keep the caller's values, as Renderer::draw leaves them. Once a
 * copy is queued every return, an error included, waits for it first, so the
 * buffers may be unpinned / freed when the call returns.
 * *ms (optional) receives the kernel time in milliseconds (HIP events). */
int rt_render(rt_scene *s, const rt_render_params *p, uint32_t *color, float *t, int32_t W,
              int32_t H, uint32_t flags, float *ms);
/* Pin (page-lock) a host framebuffer range, mapped on every device: rt_render
 * and rt_multi_render then store a cleared frame's hits straight into it and
 * DMA the other frames' copies directly. The caller keeps it pinned while it
 * reuses the buffer (the reference app keeps one FrameBuffer across frames,
 * src/main.cpp:88) and MUST unpin it before freeing it: a range freed while
 * pinned stays mapped to its old pages, and a later buffer at the same address
 * would be written through that stale mapping (rt_host_pin refuses a range
 * that overlaps one still pinned). rt_host_unpin first drains every stream the
 * library created. Optional: on pageable memory the library copies through its
 * own pinned staging frames on the host, so the HIP runtime never DMAs from or
 * to a caller's pageable memory. The range is
 * registered coarse-grained: it is coherent with the host at stream
 * synchronisation points only, which every rt_render / rt_multi_render call
 * reaches before it returns; a caller that hands the same range to its own
 * HIP work must synchronise that work before reading the range on the host. */
int rt_host_pin(void *ptr, int64_t bytes);
int rt_host_unpin(void *ptr);
/* Same on DEVICE buffers, asynchronously on `stream` (hipStream_t or NULL).
 * With tile != NULL only this rank's bands are rendered, packed (rt_tile). */
int rt_render_device(rt_scene *s, const rt_render_params *p, uint32_t *d_color, float *d_t,
                     int32_t W, int32_t H, uint32_t flags, const rt_tile *tile, void *stream);
/* Scatter gathered packed bands of all ranks (ranks x per-rank capacity, as
 * produced by rt_render_device with a tile) into a natural-layout frame, on
 * the device. per_rank_pixels = capacity of one rank's packed slot. */
int rt_untile_device(const uint32_t *d_packed_color, const float *d_packed_t, int64_t per_rank_pixels,
                     uint32_t *d_color, float *d_t, int32_t W, int32_t H, const rt_tile *tile,
                     void *stream);
/* Pixels a rank owns under `tile` (its packed buffer length). */
int64_t rt_tile_pixels(int32_t W, int32_t H, const rt_tile *tile);
/* rt_render_device for `frames` frames of one size/tile/shading path, on
 * `stream`: frame f uses params[f], d_color[f], d_t[f]. Up to 16 frames share
 * ONE launch (blockIdx.z = frame), so each frame's silhouette tail is covered
 * by the next frames' tiles; the image of every frame is identical to
 * rt_render_device's. */
int rt_render_device_frames(rt_scene *s, const rt_render_params *params, int32_t frames,
                            uint32_t *const *d_color, float *const *d_t, int32_t W, int32_t H,
                            uint32_t flags, const rt_tile *tile, void *stream);
/* FrameBuffer::clear() (src/raytracing.hpp:16-19) on device buffers: color = 0,
 * t = +inf over n pixels, on `stream`. */
int rt_clear_device(uint32_t *d_color, float *d_t, int64_t n, void *stream);
/* Per-stream render state (the multi-frame launches' work-queue heads),
 * allocated and zeroed in stream order on the current device. Optional:
 * rt_render_device_frames creates it on a stream's first use, also in stream
 * order (no device-wide synchronisation); calling this first keeps that
 * allocation out of a timed region. rt_stream_release frees it (stream
 * ordered); a later launch on the stream re-creates it. No reference
 * counterpart: the reference renders on the host (src/raytracing.cpp:67-102). */
int rt_stream_prepare(void *stream);
int rt_stream_release(void *stream);

/* ---- multi-GPU rendering in ONE process (Renderer::draw over n devices) --
 * The reference renders a frame with one call, Renderer::draw (src/main.cpp:
 * 196-207), which splits it by image rows across OpenMP threads
 * (src/raytracing.cpp:77-96). rt_multi does the same across GPUs of one
 * process: the scene (on devices[0], the root) is replicated on every other
 * device (rt_scene_replicate), the frame is cut into bands of band_rows rows,
 * band b -> slot b mod n (rt_tile), every slot renders its bands packed on its
 * own stream, and the bands come to the root in one gather per frame and
 * buffer: RCCL ncclGather over a communicator from ncclCommInitAll when the
 * devices are distinct, device-to-device (peer) copies when a device is
 * listed more than once (RCCL refuses a device twice in one communicator; the
 * one-GPU test box runs {0, 0}). The root de-interleaves them
 * (rt_untile_device). Frames are bitwise the single-device frames. */
typedef struct rt_multi rt_multi;
enum rt_multi_exchange { RT_MULTI_RCCL = 1, RT_MULTI_PEER_COPY = 2 };
/* scene must live on devices[0]; it is not owned and must outlive the handle
 * (its plane is re-read at every render, and after an
 * rt_scene_update_vertices* the replicas' trees are re-copied at the next
 * render). band_rows <= 0 selects 8. */
int rt_multi_create(rt_scene *scene, const int32_t *devices, int32_t n, int32_t band_rows, rt_multi **out);
/* Slots, the exchange in use (rt_multi_exchange) and the band height. */
int rt_multi_info(const rt_multi *m, int32_t *n, int32_t *exchange, int32_t *band_rows);
/* Renderer::draw on HOST buffers, the same contract as rt_render (flags 0 =
 * tPrev frame, RT_FLAG_CLEAR, RT_FLAG_CLEAR | RT_FLAG_HITS_ONLY). Blocks until
 * the frame is in color / t. The cleared frame (RT_FLAG_CLEAR |
 * RT_FLAG_HITS_ONLY, the app's clear() + draw) takes no gather: every slot
 * stores its bands' hits at their own rows straight into host memory (the
 * caller's buffers when rt_host_pin pinned them, else a pinned staging frame
 * whose stored spans the host copies). The other flags gather on the root.
 * *ms (optional): device time from the first launch to the assembled frame
 * (HIP events). */
int rt_multi_render(rt_multi *m, const rt_render_params *p, uint32_t *color, float *t, int32_t W, int32_t H,
                    uint32_t flags, float *ms);
/* Version code of the RCCL library rt_multi's gather runs on (ncclGetVersion:
 * major * 10000 + minor * 100 + patch), i.e. whichever librccl the process
 * resolved first (torch loads its own). */
int rt_multi_rccl_version(int32_t *version);
/* `frames` frames into DEVICE buffers on the root (d_color[f], d_t[f]),
 * flags must contain RT_FLAG_CLEAR. Stream-ordered on `stream` (a stream of
 * the root device, or NULL): the slots start after the work queued on it so
 * far, and it waits for the assembled frames; the host does not block. Each
 * slot renders up to 16 frames per launch (rt_render_device_frames). */
int rt_multi_render_device_frames(rt_multi *m, const rt_render_params *params, int32_t frames,
                                  uint32_t *const *d_color, float *const *d_t, int32_t W, int32_t H,
                                  uint32_t flags, void *stream);
int rt_multi_destroy(rt_multi *m);

/* ---- frame exchange over xGMI (multi-GPU, one process per GPU) -----------
 * Rank 0 allocates its frame slots with rt_exchange_alloc, exports them with
 * rt_ipc_get_handle, and every other rank maps them with rt_ipc_open; the ranks
 * then render their bands straight into rank 0's frame (RT_FLAG_TILE_NATURAL |
 * RT_FLAG_CLEAR | RT_FLAG_HITS_ONLY). Slots are uncached device memory, so
 * peer stores land where rank 0's kernels read them. Replaces the reference's
 * framebuffer (src/raytracing.hpp:9-20) for the row-split render. */
#define RT_IPC_HANDLE_BYTES 64
int rt_exchange_alloc(int64_t bytes, void **d_ptr);
int rt_exchange_free(void *d_ptr);
int rt_ipc_get_handle(void *d_ptr, uint8_t handle[RT_IPC_HANDLE_BYTES]);
/* Map a peer's exported allocation on the current device; *d_ptr is usable by
 * kernels of this device (peer access over xGMI). */
int rt_ipc_open(const uint8_t handle[RT_IPC_HANDLE_BYTES], void **d_ptr);
int rt_ipc_close(void *d_ptr);

/* ---- rays (IScene::intersect) ------------------------------------------- */
/* Batch of n rays, host buffers. hit[i] (0/1), t[i], normal[3i..3i+2] exactly
 * as HitInfo (src/raytracing.hpp:67-73; normal NOT flipped toward the ray),
 * prim[i] = primitive id (mesh: original triangle index in OBJ face order;
 * grid: linear index of the c0 cell of the hit sample; octree: leaf node
 * index; instanced: (instance << 32) | original triangle index; plane: -2;
 * miss: -1). */
int rt_intersect_rays(rt_scene *s, const float *o, const float *d, int64_t n, float tnear,
                      float tfar, int32_t *hit, float *t, float *normal, int64_t *prim);
/* IScene::intersect (src/raytracing.hpp:77-79) for rays that are already on
 * the GPU: n rays in DEVICE buffers, traced in stream order on `stream`
 * (hipStream_t or NULL). The call only launches: no allocation, no copy, no
 * host synchronisation. The scene's device must be the current one, as for
 * rt_render_device. Every value written is exactly what rt_intersect_rays
 * writes for the same ray (hit 0/1; t +inf on a miss; normal (0,1,0) on a
 * miss, not flipped; prim as above; the scene's plane takes part). An output
 * pointer left NULL is not written, and a batch without d_normal computes no
 * normal at all. n == 0 launches nothing; n is limited to what one launch
 * holds (2^32 - 64 rays), larger batches are split by the caller. */
typedef struct rt_ray_batch {
  int64_t n;               /* rays */
  const float *d_origin;   /* float[3n], device */
  const float *d_dir;      /* float[3n], device; not normalised by the library */
  const float *d_tnear;    /* float[n] per-ray tNear, or NULL: use tnear */
  const float *d_tfar;     /* float[n] per-ray tFar,  or NULL: use tfar  */
  float tnear, tfar;
  int32_t *d_hit;          /* outputs, device; each may be NULL = not wanted */
  float   *d_t;
  float   *d_normal;       /* float[3n] */
  int64_t *d_prim;
} rt_ray_batch;
/* Any hit: only d_hit is written (d_t, d_normal, d_prim must be NULL), with
 * HitInfo::hitten of the closest-hit query -- for the union with the plane the
 * OR of both -- and the traversal stops at the first hit (the Lambert shadow
 * ray's query, src/raytracing.cpp:36-41). */
#define RT_RAYS_ANY_HIT 1u
int rt_trace_rays_device(rt_scene *s, const rt_ray_batch *b, uint32_t flags, void *stream);

/* ---- shaded rays (the per-ray body of Renderer::draw) -------------------- */
/* The reference's eye rays as a ray batch in DEVICE buffers: ray i = y*W + x
 * is pixel (x, y) of rt_render's frame. d_dir[3i..] is the direction the frame
 * kernels trace for that pixel (EyeRayDir4f of loop row H - y - 1 under
 * proj_inv and view_inv, src/raytracing.cpp:83-88), d_origin[3i..] is
 * camera_pos. Either output may be NULL (not written), not both. p, W and H
 * are checked as rt_render_device checks them. The call only launches on
 * `stream`: no allocation, no copy, no host synchronisation. */
int rt_eye_rays_device(const rt_render_params *p, int32_t W, int32_t H,
                       float *d_origin, float *d_dir, void *stream);

/* Renderer::intersectionColor, color_pack_rgba and draw's store rule
 * (src/raytracing.cpp:13-102) for rays in device buffers, in stream order on
 * `stream`; the call only launches (no allocation, no copy, no host
 * synchronisation; the scene's device must be the current one). All four
 * scene kinds, an instanced scene in both of its modes.
 *
 * Ray i, with (o, d) from the batch, tn_i = d_tnear ? d_tnear[i] : tnear and
 * tf_i = d_tfar ? d_tfar[i] : tfar, is intersected with the union of the scene
 * and its plane over [tn_i, tf_i] and shaded as the frame kernels shade a
 * pixel: Lambert with the shadow ray (origin point + 0.3 sd over [0.01, 100])
 * and one reflection bounce off the plane (origin point + 0.02 R over
 * [0.01, 100]), or the Color / Normal modes. Of `p` only light_pos,
 * shading_mode, enable_shadows and enable_reflections are read; reserved must
 * be 0. For an instanced scene every one of the up to four rays per input ray
 * goes through the loop above (with its box_pass line for RT_INSTANCED_TLAS);
 * a shadow query may stop at its first hit, its flag being the closest-hit
 * flag. A BLAS refitted since the scene last saw it is caught up in stream
 * order ahead of the launch, as for rt_trace_rays_device.
 *
 * store = hit && !isinf(t), the frame kernels' rule. If store: d_color[i] =
 * the packed RGBA8 colour and, when b->d_t is given, d_t[i] = t. Else with
 * RT_SHADE_CLEAR: d_color[i] = 0 and d_t[i] = +inf. Else ray i writes neither
 * (Renderer::draw on a frame that already holds something). b->d_hit[i] =
 * store ? 1 : 0 and b->d_prim[i] = the first intersection's primitive id
 * (-2 the plane, -1 a miss) are always written when given. b->d_normal must
 * be NULL: colour is the output here, the normal is rt_trace_rays_device's.
 *
 * d_tfar may be the same buffer as d_t: each ray reads its own interval before
 * its own stores, and no ray reads another's. Several scenes shaded one after
 * another into one (d_color, d_t) pair without RT_SHADE_CLEAR, each with
 * d_tfar = d_t, then compose by depth as the reference's tPrev does
 * (tFar = min(tFar, tPrev), src/raytracing.cpp:89-94): a later scene's hit is
 * stored only where it lies in front of what the pair holds.
 *
 * n == 0 launches nothing; n is limited as for rt_trace_rays_device. */
#define RT_SHADE_CLEAR 1u
int rt_shade_rays_device(rt_scene *s, const rt_ray_batch *b, const rt_render_params *p,
                         uint32_t *d_color, uint32_t flags, void *stream);

/* Timing helper for benchmarks: renders `frames` frames back to back on the
 * device (buffers owned by the library), returns the mean kernel ms per frame
 * and the total in *total_ms. params[frames] gives one camera per frame. */
int rt_bench_frames(rt_scene *s, const rt_render_params *params, int32_t frames, int32_t W,
                    int32_t H, uint32_t flags, float *mean_ms, float *total_ms);

/* Work counters of the reference traversal for `frames` frames (diagnostic
 * kernel variant; same traversal as the timed kernels): counters[0..8] =
 * BVH inner-node visits, BVH leaf visits, triangle tests, grid sdf
 * evaluations, octree node visits, octree leaf visits, octree march steps,
 * octree normal evaluations, rays (scene intersections). Shadow rays stop at
 * their first hit here, so with shadows on the counts are lower than the
 * reference's full traversal; primary-ray counts are identical. */
int rt_count_work(rt_scene *s, const rt_render_params *params, int32_t frames, int32_t W, int32_t H,
                  uint32_t flags, const rt_tile *tile, int64_t counters[9]);

/* ---- mesh -> SDF construction -------------------
 * The reference renders SDF grids/octrees it does not generate (course data in
 * the formats read by loadSDFGrid, src/grid_raytracing.cpp:127-134, and
 * loadSDFOctree, src/octree_raytracing.cpp:8-16 / octree_raytracing.hpp:8-18);
 * BASELINE configs 3-4 name large inputs absent from the reference
 * (.MISSING_LARGE_BLOBS). These entry points build them deterministically on
 * the GPU: signed distance = distance to the closest triangle (ties: lowest
 * triangle id), sign from the angle-weighted pseudonormal of the closest
 * feature, positions after v /= v.w. See DESIGN.md 9. */
int rt_sdf_mesh_create(const float *vpos4, int64_t nverts, const uint32_t *idx, int64_t nidx,
                       rt_sdf_mesh **out);
/* Signed distance at n points p3[3n] (host buffers). */
int rt_sdf_mesh_points(rt_sdf_mesh *m, const float *p3, int64_t n, float *dist);
/* SDFGrid values for a size[0] x size[1] x size[2] lattice over [-1,1]^3
 * (sample i at 2i/(size-1)-1, index (x*sy+y)*sz+z), host buffer. */
int rt_sdf_mesh_grid(rt_sdf_mesh *m, const uint32_t size[3], float *values);
/* Closest point and signed distance for points that are already on the GPU:
 * n points in DEVICE buffers, queried in stream order on `stream` (hipStream_t
 * or NULL). The definition is the project's own (oracle/cpuref.cpp, sdfref;
 * the reference has no such query). Point i, p = d_point[3i..3i+2], with
 * r_i = d_radius ? d_radius[i] : radius:
 *
 *   r2 = r_i * r_i
 *   for every triangle T = (a, b, c) of the mesh, in original (OBJ face) order:
 *     (q, feat) = the closest point of T to p and its Voronoi region
 *                 (sdfref::closest: Ericson, Real-Time Collision Detection
 *                 5.1.5, f32, op for op)
 *     d2 = dot(p - q, p - q)           (x*x + y*y + z*z left to right, unfused)
 *     T is a candidate iff r_i >= 0 && d2 <= r2
 *   the winner is the candidate with the least (d2, triangle id),
 *   lexicographically
 *
 * so a NaN radius, a negative radius or a NaN point has no candidate, and
 * radius = +inf is the unbounded query. With a winner: d_dist[i] = sqrt(d2),
 * negated where dot(p - q, N) < 0 for N the angle-weighted pseudonormal of
 * region `feat` of the winner (rt_sdf_mesh_points' sign; RT_POINTS_UNSIGNED:
 * never negated); d_closest[3i..] = q; d_prim[i] = the winner's original
 * triangle index; d_feature[i] = feat. Without one: d_dist[i] = +inf,
 * d_closest[3i..] = p (copied bit for bit), d_prim[i] = -1, d_feature[i] = -1.
 * With radius = +inf and no flag, d_dist is bit for bit what
 * rt_sdf_mesh_points returns for the same points.
 *
 * Exactness: the kernel walks the BVH8 and skips a box whose squared distance
 * exceeds (sqrt(best d2 so far, or r2) + 1e-5)^2. The absolute slack of 1e-5
 * covers the f32 rounding of the triangle test for points and meshes in about
 * [-1,1]^3; that is the domain in which the result is the loop
 * above bit for bit, for this entry as for rt_sdf_mesh_points and _grid.
 *
 * The call only launches on `stream`: no allocation, no copy, no host
 * synchronisation. The handle's device must be the current one. An output
 * left NULL is neither written nor computed: without d_dist, or with
 * RT_POINTS_UNSIGNED, no sign is computed and the pseudonormals are not read.
 * n == 0 launches nothing; n is limited as for rt_trace_rays_device. The
 * kernel only reads the handle's immutable arrays, so calls on different
 * streams may overlap; the handle must outlive the work queued with it
 * (rt_sdf_mesh_destroy does not wait for the caller's streams).
 * RT_E_INVALID, with nothing launched: a NULL handle or batch, n < 0, a NULL
 * d_point with n > 0, all four outputs NULL, an unknown flag bit, and a
 * `radius` that is NaN or negative when d_radius is NULL. */
typedef struct rt_point_batch {
  int64_t n;              /* points */
  const float *d_point;   /* float[3n], device */
  const float *d_radius;  /* float[n] per-point search radius, or NULL: use radius */
  float radius;           /* +inf = unbounded */
  float   *d_dist;        /* outputs, device; each may be NULL = not wanted, not all */
  float   *d_closest;     /* float[3n] */
  int64_t *d_prim;        /* original triangle index (OBJ face order), -1 = none */
  int32_t *d_feature;     /* 0..2 vertex a,b,c; 3 ab; 4 ac; 5 bc; 6 face; -1 = none */
} rt_point_batch;
#define RT_POINTS_UNSIGNED 1u   /* d_dist = sqrt(d2), no sign; the pseudonormals are not read */
int rt_sdf_mesh_points_device(rt_sdf_mesh *m, const rt_point_batch *b, uint32_t flags, void *stream);
/* rt_sdf_mesh_grid into a DEVICE buffer of size[0]*size[1]*size[2] floats: the
 * same size checks, the same bits, the same kernel, queued on `stream`, and
 * nothing else happens (no allocation, no copy, no host synchronisation). The
 * handle's device must be the current one and the handle must outlive the
 * queued work. */
int rt_sdf_mesh_grid_device(rt_sdf_mesh *m, const uint32_t size[3], float *d_values, void *stream);
/* HIP device the handle's arrays live on (the one current at rt_sdf_mesh_create). */
int rt_sdf_mesh_device(const rt_sdf_mesh *m);
/* Sparse SDFOctree of max depth `depth` (36-byte nodes, BFS, 8 children
 * contiguous): a node is refined when |sdf(centre)| <= its half-diagonal;
 * unrefined nodes are empty leaves (values 1000); depth-`depth` nodes are
 * leaves holding the SDF at their corners. Two-call protocol on *count (the
 * result is cached in the handle). */
int rt_sdf_mesh_octree(rt_sdf_mesh *m, int32_t depth, int64_t *count, void *nodes36);
int rt_sdf_mesh_destroy(rt_sdf_mesh *m);

/* ---- deforming meshes under point queries -----------------
 * rt_sdf_mesh_create_ex with flags = 0 is exactly rt_sdf_mesh_create. With
 * RT_MESH_DYNAMIC the vertices may be moved afterwards: an update keeps the
 * topology of creation and recomputes on the device everything that depends on
 * a position.
 *
 * What stays: the tree (child words), the leaf order, the original triangle
 * ids, and the weld map of creation -- vertices whose divided positions
 * (v / v.w) had equal bits at creation share one pseudonormal for the life of
 * the handle, wherever they move; an edge is the pair of its welded end
 * points. nverts must equal the creation value.
 *
 * What is recomputed, from the new positions:
 *   (a) every triangle record: the corners v / v.w (correctly rounded
 *       division) in the order idx[3 id + 0..2];
 *   (b) every child box: the exact min/max of its subtree's divided corners
 *       (the order and the std::min / std::max tie rules of the scene refit,
 *       rt_scene_update_vertices);
 *   (c) the 7 pseudonormals of every original triangle, as creation computes
 *       them: the face normal nf in float (cross product, sqrt, divide; zero
 *       when the length is 0); each corner angle in double (0 when an adjacent
 *       edge has zero length, the cosine clamped to [-1, 1]); each welded
 *       vertex the double sum of ang * nf over its incident (triangle, corner)
 *       pairs in ascending triangle id, then corner; each welded edge the
 *       double sum of nf over its incident triangles in ascending triangle id,
 *       then ab, ac, bc; each sum rounded to float once.
 *
 * Against a fresh handle of the moved mesh (rt_sdf_mesh_create of the new
 * positions, when they have the weld classes of creation): distance magnitude,
 * closest point, triangle and feature of every query are bit for bit the
 * fresh handle's, and the brute-force loop's above (the winner is the least
 * (d2, id), which any valid tree finds; the exactness domain is the one named
 * there, points and meshes in about [-1,1]^3). The sign is the fresh handle's
 * wherever the winning feature's pseudonormal has the same bits. Face and edge
 * normals always have: they are IEEE operations in a fixed order. Vertex
 * normals go through acos in double, and the device's acos may differ from the
 * host library's in the last bits of the double; that can, rarely, move the
 * final float rounding of a component by one ulp.
 *
 * Vertex values are not validated: topology is only read, so no value can make
 * a walk index out of bounds, and NaN positions give NaN distances, as the
 * arithmetic says.
 *
 * rt_sdf_mesh_update_vertices_device only launches on `stream` (hipStream_t or
 * NULL): no allocation, no copy, no host wait; the handle's device must be the
 * current one; d_vpos4 is read by the queued kernels. Queries queued on the
 * same stream afterwards see the moved mesh; the caller orders updates against
 * queries still running on other streams. Each update records an event on
 * `stream` after its last kernel, and the handle's own host entries
 * (rt_sdf_mesh_points, _grid, _octree) make their stream wait for it before
 * they read. rt_sdf_mesh_update_vertices copies a host buffer through a
 * staging buffer the handle keeps and returns when the update is complete.
 * Both invalidate the octree cache of rt_sdf_mesh_octree.
 *
 * RT_E_INVALID: a NULL handle or pointer, nverts unlike creation, an unknown
 * flag bit. RT_E_STATE: an update of a handle created without RT_MESH_DYNAMIC.
 * A refused call launches nothing and leaves the handle as it was.
 *
 * A handle without the flag holds three device arrays: the inner nodes (224
 * bytes each), the triangle records (48 bytes per triangle) and the
 * pseudonormals (112 bytes per triangle). With T triangles, V vertices, WV
 * welded vertices and WE welded edges a dynamic handle adds: the index array
 * (12 T), the vertex staging buffer (16 V), the weld id per vertex (4 V), the
 * welded edge ids (12 T), the incidence lists of the welded vertices
 * (4 (WV + 1) + 12 T) and edges (4 (WE + 1) + 12 T), the face normals (16 T)
 * and corner angles (24 T) as scratch, and the welded vertex (16 WV) and edge
 * (16 WE) normals. rt_sdf_mesh_device_bytes returns the sum for the handle
 * (its query staging, which grows with use, is not counted). RT_MESH_DYNAMIC
 * is the flag of rt_scene_create_mesh_ex. */
int rt_sdf_mesh_create_ex(const float *vpos4, int64_t nverts, const uint32_t *idx, int64_t nidx,
                          uint32_t flags, rt_sdf_mesh **out);
int rt_sdf_mesh_update_vertices(rt_sdf_mesh *m, const float *vpos4, int64_t nverts);              /* host buffer */
int rt_sdf_mesh_update_vertices_device(rt_sdf_mesh *m, const float *d_vpos4, int64_t nverts, void *stream);
/* After one device synchronisation: pn28[28 t + 4 f + 0..2] = the pseudonormal
 * of feature f (0..6) of ORIGINAL triangle t, as the device holds it (the 4th
 * float of each is whatever is stored). Any handle, dynamic or not; ntri must
 * be the handle's triangle count (else RT_E_INVALID). */
int rt_sdf_mesh_get_pseudonormals(const rt_sdf_mesh *m, float *pn28, int64_t ntri);
int64_t rt_sdf_mesh_device_bytes(const rt_sdf_mesh *m);   /* RT_E_INVALID for a NULL handle */

/* ---- SDF scenes that follow a deforming mesh on the device ---
 * A grid scene takes new values from a device buffer, and an octree scene is
 * rebuilt from an SDF-mesh handle, both in stream order: the calls only launch
 * on `stream` (hipStream_t or NULL), with no allocation, no copy and no host
 * wait. The scene keeps its device arrays, so ray queries and frames queued on
 * the same stream afterwards see the new scene, and so does an instanced scene
 * that holds it as a bottom-level scene (its table holds the same pointers; it
 * is not touched). The caller orders a call against work that still uses the
 * scene on OTHER streams. Copies made by rt_scene_replicate (rt_multi's
 * included) are snapshots and do not follow.
 *
 * rt_scene_update_grid_device: any grid scene, linear or bricked. d_values
 * holds size[0]*size[1]*size[2] floats of the scene's own size in the layout
 * (x*sy+y)*sz+z, which is what rt_sdf_mesh_grid_device writes; the scene's
 * array is rewritten in the layout the scene was created with (a copy kernel,
 * or the bricking kernel of creation). The scene's device must be the current
 * one. RT_E_STATE for a scene that is not a grid, RT_E_INVALID for a NULL
 * argument or another current device.
 *
 * rt_scene_create_octree_dynamic: an octree scene with room for max_nodes
 * nodes of a tree of at most `depth` levels; depth in [0, 12] (the range of
 * rt_sdf_mesh_octree), max_nodes in [1, 2^32 - 1], checked before anything
 * touches a device (RT_E_INVALID). Every device buffer a rebuild will ever
 * need is allocated here and counted in rt_scene_device_bytes: per node of
 * capacity 40 bytes of scene (8 word + 32 values) and 52 bytes of build
 * scratch (the same again, 8 for the node's cell, 4 for its refine flag), and
 * a table of at most 150 KB. The kernel's stack class is the one of a
 * `depth`-level tree for the scene's life (rt_scene_bvh_stats reports
 * `depth`), whatever tree it holds. The initial tree is one root that is an
 * empty leaf (values 1000): every ray misses.
 *
 * rt_sdf_mesh_octree_device: the scene becomes the tree rt_sdf_mesh_octree
 * defines for the handle's current mesh at the scene's depth, as
 * rt_scene_create_octree would hold it:
 *   - a node of level d < depth in cell (i, j, k) is refined iff |sdf(centre)|
 *     <= 1.7320508f * 2^-d, centre = (float)(2i+1) * 2^-d - 1.0f per axis;
 *     an unrefined node is an empty leaf with eight values of 1000, a refined
 *     one has values 0;
 *   - a level-`depth` node holds the SDF at its corners, (float)(i + x) *
 *     2^(1-depth) - 1.0f per axis, as values[(x<<2)|(y<<1)|z];
 *   - nodes in BFS order, the eight children of a node contiguous and in the
 *     order of their parents, so leaf indices (rt_ray_batch prim) are those of
 *     a fresh scene of the same nodes;
 *   - a leaf never hits if all its values are > 10, or all == 0, or all >=
 *     1e-4; the child masks are those of rt_scene_create_octree.
 * Every distance has the bits rt_sdf_mesh_points gives for the point. A build
 * is 5 * depth + 5 launches (4 at depth 0) sized by depth and max_nodes, never
 * by the mesh. Handle and scene must live on the current device
 * (RT_E_INVALID); a scene not made by
 * rt_scene_create_octree_dynamic gives RT_E_STATE; a refused call launches
 * nothing. The caller also orders the build against updates of the handle on
 * other streams, as for rt_sdf_mesh_points_device.
 * Overflow: a tree that needs more than max_nodes nodes is dropped on the
 * device. The scene keeps, bit for bit, the tree it had, and a device flag
 * records the drop until the next build that fits. Size max_nodes with
 * rt_sdf_mesh_octree(m, depth, &count, NULL).
 *
 * rt_scene_octree_status / rt_scene_get_octree wait for the device first. Any
 * octree scene: *count = the nodes it holds now, *overflow = 1 if its last
 * build was dropped (a plain octree: its size, 0). rt_scene_get_octree returns
 * the 36-byte nodes rebuilt from what the scene holds (values as stored, the
 * children offset, 0 for a leaf of either kind); two-call protocol on *count. */
int rt_scene_update_grid_device(rt_scene *s, const float *d_values, void *stream);
int rt_scene_create_octree_dynamic(int32_t depth, int64_t max_nodes, rt_scene **out);
int rt_sdf_mesh_octree_device(rt_sdf_mesh *m, rt_scene *s, void *stream);
int rt_scene_octree_status(rt_scene *s, int64_t *count, int32_t *overflow);
int rt_scene_get_octree(rt_scene *s, int64_t *count, void *nodes36);
/* Host-only: midpoint subdivision `levels` times (each triangle -> 4, edge
 * midpoints shared, (a+b)*0.5 on the 4 components): the config-5 stand-in
 * for MotorcycleCylinderHead.obj. Two-call protocol on the counts. */
int rt_mesh_subdivide(const float *vpos4, int64_t nverts, const uint32_t *idx, int64_t nidx, int32_t levels,
                      float *out_vpos4, int64_t *out_nverts, uint32_t *out_idx, int64_t *out_nidx);

/* ---- the viewer's orbit camera and image output --
 * Camera (src/camera.hpp:7-61, src/camera.cpp:1-72, src/quaternion.hpp:8-70):
 * position/target plus an orientation quaternion; rotate(dx, dy) is the
 * viewer's mouse drag (main.cpp:277-280: rotate(-dx, -dy)), zoom(wheel) its
 * mouse wheel (main.cpp:281-288). Host-only; the state is a plain struct. */
typedef struct rt_camera_state {
  float position[3];
  float target[3];
  float orientation[4]; /* x, y, z, w (un-normalised after construction, as the reference) */
  float sensitivity;    /* 0.01 (camera.hpp:55) */
  int32_t lock_up;
  float locked_up[3];
} rt_camera_state;
int rt_camera_init(const float pos[3], const float target[3], const float up[3], rt_camera_state *c);
int rt_camera_rotate(rt_camera_state *c, float dx, float dy);
int rt_camera_reset_position(rt_camera_state *c, const float pos[3]);
int rt_camera_reset_target(rt_camera_state *c, const float target[3]);
int rt_camera_set_lock_up(rt_camera_state *c, int on);
int rt_camera_zoom(rt_camera_state *c, float wheel);
/* up(), right(), forward() (camera.hpp:29-37); any pointer may be NULL. */
int rt_camera_basis(const rt_camera_state *c, float up[3], float right[3], float forward[3]);
/* inverse4x4(lookAtMatrix()) -- the view_inv of rt_render_params. */
int rt_camera_view_inverse(const rt_camera_state *c, float view_inv[16]);
/* Write a colour buffer (W*H packed RGBA8, R in the low byte, row 0 = top) as
 * an 8-bit RGBA PNG (what the viewer shows, main.cpp:239-242). */
int rt_write_png(const char *path, const uint32_t *color, int32_t W, int32_t H);
/* cmesh4::SaveMeshToObj (src/core/mesh.cpp:14-63), byte for byte: v / vt / vn
 * per vertex with std::to_string, faces "f i/i/i". vnorm4 (4 per vertex) and
 * vtex2 (2 per vertex) may be NULL: fix_missing's defaults (0,0,1) / (0,0). */
int rt_save_obj(const char *path, const float *vpos4, int64_t nverts, const uint32_t *idx, int64_t nidx,
                const float *vnorm4, const float *vtex2);

#ifdef __cplusplus
}
#endif
#endif /* RTAMD_H */
