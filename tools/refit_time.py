"""What a BVH8 refit costs and what it buys (rt_scene_update_vertices_device),
for the bunny and the 1.1 M-triangle stand-in (the bunny subdivided twice,
rt_mesh_subdivide), both deformed by the tests' sine shear x += 0.15 sin(4 y):

  update   host wall time of one rt_scene_update_vertices_device (it returns
           after its one host wait, so this is the whole update), against
  rebuild  rt_scene_destroy + rt_scene_create_mesh of the same deformed mesh
           (the default builder choice, RT_BVH_AUTO), through --base-lib when
           given -- a librtamd.so built from the commit before the refit --
           else through this library, whose rt_scene_create_mesh is that code;
           medians over --reps alternating repeats, in one process;
  trace    rt_trace_rays_device kernel time (torch events, closest hit with
           all outputs) of the 1080p eye rays on the refitted tree against a
           freshly built tree of the same deformed mesh: the traversal quality
           a refit gives up for its speed.

usage: python tools/refit_time.py [--scenes bunny,big] [--reps 9] [--base-lib PATH] [--json OUT]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, p) for p in ("triangles-sdf-cpu-raytracing_amd", "oracle", "tests")]

W, H, POS = 1920, 1080, (0.0, 0.0, 2.5)


def shear(v):
    w = np.array(v, np.float32)
    w[:, 0] += (np.float32(0.15) * np.sin(np.float32(4.0) * w[:, 1])).astype(np.float32)
    return w


def base_create(path):
    """rt_scene_create_mesh / rt_scene_destroy of another librtamd.so."""
    L = C.CDLL(path)
    L.rt_scene_create_mesh.restype = C.c_int
    L.rt_scene_create_mesh.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.POINTER(C.c_void_p)]
    L.rt_scene_destroy.restype = C.c_int
    L.rt_scene_destroy.argtypes = [C.c_void_p]
    L.rt_build_id.restype = C.c_char_p
    return L


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", default="bunny,big")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--base-lib")
    ap.add_argument("--json")
    a = ap.parse_args()

    import torch

    import cpuref
    import rtamd
    import scenes as S

    if rtamd.device_count() < 1:
        sys.exit("refit_time.py: no HIP device visible")
    L = rtamd.lib()
    B = base_create(a.base_lib) if a.base_lib else L
    print(f"librtamd {L.rt_build_id().decode()} on {torch.cuda.get_device_name(0)}; rebuilds through "
          f"{'librtamd ' + B.rt_build_id().decode() if a.base_lib else 'the same library'}", flush=True)
    dev = torch.device("cuda")
    _, (v0, i0), _ = S.inputs("stanford-bunny.obj")
    eye_d = np.ascontiguousarray(cpuref.primary_rays(S.params("stanford-bunny.obj", W, H, "primary", POS, "ref"), W, H)
                                 .reshape(-1, 3))
    o_t = torch.from_numpy(np.tile(np.float32(POS), (len(eye_d), 1))).to(dev)
    d_t = torch.from_numpy(eye_d).to(dev)
    n = o_t.shape[0]
    out = {"hit": torch.empty(n, dtype=torch.int32, device=dev), "t": torch.empty(n, dtype=torch.float32, device=dev),
           "normal": torch.empty((n, 3), dtype=torch.float32, device=dev),
           "prim": torch.empty(n, dtype=torch.int64, device=dev)}
    results = []
    for key in a.scenes.split(","):
        mesh = rtamd.SimpleMesh(np.ascontiguousarray(v0, np.float32), np.ascontiguousarray(i0, np.uint32))
        if key == "big":
            mesh = rtamd.subdivide_mesh(mesh, 2)
        v, i = mesh.vPos4f, mesh.indices
        w = shear(v)
        v_t, w_t = torch.from_numpy(v).to(dev), torch.from_numpy(w).to(dev)
        torch.cuda.synchronize()
        dyn = rtamd.BVHBuilder(mesh, dynamic=True)
        _, _, depth = dyn.tree_stats()
        pv, pw, pi = (C.c_void_p(x.ctypes.data) for x in (v, w, i))
        h = C.c_void_p()
        assert B.rt_scene_create_mesh(pw, len(w), pi, len(i), C.byref(h)) == 0
        upd, reb = [], []
        for r in range(a.reps + 2):  # (two warm-up rounds)
            src = w_t if r % 2 == 0 else v_t  # alternate the two positions: every update moves the tree
            t0 = time.perf_counter()
            dyn.update_vertices_device(src.data_ptr(), len(v))
            t1 = time.perf_counter()
            assert B.rt_scene_destroy(h) == 0
            assert B.rt_scene_create_mesh(pw if r % 2 == 0 else pv, len(w), pi, len(i), C.byref(h)) == 0
            t2 = time.perf_counter()
            if r >= 2:
                upd.append((t1 - t0) * 1e3)
                reb.append((t2 - t1) * 1e3)
        assert B.rt_scene_destroy(h) == 0
        # traversal: the refitted tree against a fresh build of the same deformed mesh
        dyn.update_vertices_device(w_t.data_ptr(), len(v))
        fresh = rtamd.BVHBuilder(rtamd.SimpleMesh(w, i))
        ms = {"refit": [], "fresh": []}
        ptr = {k: x.data_ptr() for k, x in out.items()}
        hits = {}
        for r in range(3):
            for name, sc in (("refit", dyn), ("fresh", fresh)):
                call = lambda: sc.trace_device(o_t.data_ptr(), d_t.data_ptr(), n, hit_ptr=ptr["hit"], t_ptr=ptr["t"],
                                               normal_ptr=ptr["normal"], prim_ptr=ptr["prim"])
                for _ in range(a.warmup):
                    call()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.launches):
                    call()
                e1.record()
                e1.synchronize()
                ms[name].append(e0.elapsed_time(e1) / a.launches)
                hits[name] = int(out["hit"].sum().item())
        res = {"scene": key, "triangles": len(i) // 3, "bvh_depth": depth,
               "update_ms": float(np.median(upd)), "update_ms_min_max": [min(upd), max(upd)],
               "rebuild_ms": float(np.median(reb)), "rebuild_ms_min_max": [min(reb), max(reb)],
               "rebuild_over_update": float(np.median(reb) / np.median(upd)),
               "trace_refit_ms": float(np.median(ms["refit"])), "trace_fresh_ms": float(np.median(ms["fresh"])),
               "trace_refit_over_fresh": float(np.median(ms["refit"]) / np.median(ms["fresh"])),
               "eye_rays": n, "hits_refit": hits["refit"], "hits_fresh": hits["fresh"]}
        results.append(res)
        print(f"{key:6} {res['triangles']:8d} triangles, depth {depth}: update {res['update_ms']:.3f} ms "
              f"[{min(upd):.3f}, {max(upd):.3f}], rebuild {res['rebuild_ms']:.2f} ms [{min(reb):.2f}, {max(reb):.2f}] "
              f"= {res['rebuild_over_update']:.0f} x; 1080p eye rays {res['trace_refit_ms']:.3f} ms on the refitted "
              f"tree, {res['trace_fresh_ms']:.3f} ms on a fresh one = {res['trace_refit_over_fresh']:.2f} x "
              f"(hits {hits['refit']} / {hits['fresh']})", flush=True)
        dyn.close()
        fresh.close()
    if a.json:
        with open(a.json, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
