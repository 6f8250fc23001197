"""What it costs an SDF scene to follow its mesh on the device
(rt_sdf_mesh_octree_device, rt_scene_update_grid_device), against the host
route each replaces, in one build of the library, for the bunny:

  octree   depths 6 and 8: one device rebuild of a dynamic scene, event time
           (torch CUDA events around the call's launches) and the host time of
           the call, against rt_sdf_mesh_octree with its cache invalidated (a
           depth-0 query in between, outside the timed part) +
           rt_scene_create_octree + rt_scene_destroy, host wall time;
  grid     96^3 and 256^3: rt_scene_update_grid_device from the lattice a
           previous rt_sdf_mesh_grid_device left on the device, event time,
           against the download of that lattice + rt_scene_create_grid +
           rt_scene_destroy, host wall time. The lattice kernel itself is on
           both routes and is timed apart;
  trace    the 1920x1080 eye rays (t only) through the rebuilt / updated scene
           and through a fresh scene of the same arrays, event time.

Every figure is the median of --reps (5) repeats that alternate between the
two sides. Also printed: whether the two scenes' t have the same bits, and the
scenes' device bytes.

usage: python tools/sdf_scene_time.py [--depths 6,8] [--grids 96,256] [--reps 5] [--json OUT]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, p) for p in ("triangles-sdf-cpu-raytracing_amd", "oracle", "tests", "tools")]


def med(x):
    return float(np.median(x))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--depths", default="6,8")
    ap.add_argument("--grids", default="96,256")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--json")
    a = ap.parse_args()

    import torch

    import rtamd
    import scenes as S
    from rtamd import torch_rays

    if rtamd.device_count() < 1:
        sys.exit("sdf_scene_time.py: no HIP device visible")
    print(f"librtamd {rtamd.lib().rt_build_id().decode()} on {torch.cuda.get_device_name(0)}", flush=True)
    _, (v, i), _ = S.inputs("stanford-bunny.obj")
    mesh = rtamd.SimpleMesh(np.ascontiguousarray(v, np.float32), np.ascontiguousarray(i, np.uint32))
    m = rtamd.SDFMesh(mesh)
    st = torch.cuda.current_stream().cuda_stream
    W, H = 1920, 1080
    pos = (0.0, 0.0, 2.5)
    vi, pi = rtamd.camera_matrices(pos, aspect=W / H)
    eye_o, eye_d = torch_rays.eye_rays(rtamd.render_params(pos, vi, pi), W, H)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        t0 = time.perf_counter()
        out = fn()
        t1 = time.perf_counter()
        e1.record()
        return (e0, e1), (t1 - t0) * 1e3, out

    def trace_pair(new, fresh):
        ev = {"new": [], "fresh": []}
        t = {}
        for r in range(a.reps + a.warmup):
            for k, s in (("new", new), ("fresh", fresh)):
                e, _, h = timed(lambda: torch_rays.trace(s, eye_o, eye_d, outputs=("t",)))
                t[k] = h.t
                if r >= a.warmup:
                    ev[k].append(e)
        torch.cuda.synchronize()
        ms = {k: [e0.elapsed_time(e1) for e0, e1 in x] for k, x in ev.items()}
        same = bool(torch.equal(t["new"].view(torch.int32), t["fresh"].view(torch.int32)))
        return med(ms["new"]), med(ms["fresh"]), same, ms

    results = []
    for depth in [int(x) for x in a.depths.split(",") if x]:
        nodes = m.octree(depth)
        count = nodes.size // 36
        dyn = rtamd.SDFOctree.dynamic(depth, count)
        ev, call, host = [], [], []
        for r in range(a.reps + a.warmup):
            e, c, _ = timed(lambda: m.octree_device(dyn, stream=st))
            torch.cuda.synchronize()
            m.octree(0)  # (another depth: the handle's cache no longer holds this one)
            t0 = time.perf_counter()
            fresh = rtamd.SDFOctree(m.octree(depth))
            fresh.close()
            t1 = time.perf_counter()
            if r >= a.warmup:
                ev.append(e)
                call.append(c)
                host.append((t1 - t0) * 1e3)
        ev = [e0.elapsed_time(e1) for e0, e1 in ev]
        assert dyn.status() == (count, 0) and np.array_equal(dyn.nodes(), nodes)
        fresh = rtamd.SDFOctree(nodes)
        tn, tf, same, tms = trace_pair(dyn, fresh)
        res = {"kind": "octree", "depth": depth, "nodes": count, "launches": 5 * depth + 4 + (depth > 0),
               "device_ms": med(ev), "device_ms_all": ev, "call_ms": med(call), "host_route_ms": med(host),
               "host_route_ms_all": host, "host_over_device": med(host) / med(ev),
               "device_bytes_dynamic": dyn.device_bytes(), "device_bytes_fresh": fresh.device_bytes(),
               "maxd_dynamic_depth": dyn.tree_stats()[2], "maxd_fresh_depth": fresh.tree_stats()[2],
               "trace_ms_dynamic": tn, "trace_ms_fresh": tf, "trace_ms_all": tms, "trace_same_bits": same}
        print(f"octree depth {depth}: {count} nodes, device rebuild {res['device_ms']:.3f} ms event time "
              f"[{min(ev):.3f}, {max(ev):.3f}] ({res['call_ms']:.3f} ms in the call, {res['launches']} launches), host "
              f"build + create + destroy {res['host_route_ms']:.2f} ms [{min(host):.2f}, {max(host):.2f}] = "
              f"{res['host_over_device']:.1f} x; 1080p eye rays {tn:.3f} ms dynamic, {tf:.3f} ms fresh, t bits equal: "
              f"{same}; device bytes {res['device_bytes_dynamic']} dynamic, {res['device_bytes_fresh']} fresh", flush=True)
        results.append(res)
        dyn.close()
        fresh.close()

    for n in [int(x) for x in a.grids.split(",") if x]:
        size = (n, n, n)
        lat = torch_rays.sdf_grid(m, size)
        torch.cuda.synchronize()
        g = rtamd.SDFGrid(size, np.zeros(n ** 3, np.float32))
        ev, lev, host = [], [], []
        for r in range(a.reps + a.warmup):
            le, _, _ = timed(lambda: m.grid_device(size, lat.data_ptr(), stream=st))
            e, _, _ = timed(lambda: g.update_device(lat.data_ptr(), stream=st))
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fresh = rtamd.SDFGrid(size, lat.cpu().numpy().ravel())
            fresh.close()
            t1 = time.perf_counter()
            if r >= a.warmup:
                ev.append(e)
                lev.append(le)
                host.append((t1 - t0) * 1e3)
        ev = [e0.elapsed_time(e1) for e0, e1 in ev]
        lev = [e0.elapsed_time(e1) for e0, e1 in lev]
        fresh = rtamd.SDFGrid(size, lat.cpu().numpy().ravel())
        tn, tf, same, tms = trace_pair(g, fresh)
        res = {"kind": "grid", "size": n, "device_ms": med(ev), "device_ms_all": ev, "lattice_ms": med(lev),
               "host_route_ms": med(host), "host_route_ms_all": host, "host_over_device": med(host) / med(ev),
               "device_bytes": g.device_bytes(), "trace_ms_updated": tn, "trace_ms_fresh": tf, "trace_ms_all": tms,
               "trace_same_bits": same}
        print(f"grid {n}^3: device update {res['device_ms']:.3f} ms event time [{min(ev):.3f}, {max(ev):.3f}] (the lattice "
              f"kernel before it: {res['lattice_ms']:.3f} ms), download + create + destroy {res['host_route_ms']:.2f} ms "
              f"[{min(host):.2f}, {max(host):.2f}] = {res['host_over_device']:.1f} x; 1080p eye rays {tn:.3f} ms updated, "
              f"{tf:.3f} ms fresh, t bits equal: {same}; device bytes {res['device_bytes']}", flush=True)
        results.append(res)
        g.close()
        fresh.close()
    m.close()
    if a.json:
        with open(a.json, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
