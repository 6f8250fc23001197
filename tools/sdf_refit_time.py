"""What a refit of an SDF-mesh handle costs and what it costs the queries
(rt_sdf_mesh_update_vertices_device), for the bunny and the 1.1 M-triangle
stand-in (the bunny subdivided twice, rt_mesh_subdivide), both deformed by the
tests' sine shear x += 0.15 sin(4 y):

  update   one rt_sdf_mesh_update_vertices_device: event time (torch CUDA
           events around the call's launches) and the host time of the call,
           which only launches, against
  rebuild  the rt_sdf_mesh_destroy + rt_sdf_mesh_create it replaces, of the
           same deformed mesh (host wall time: it is host work and uploads);
  points   rt_sdf_mesh_points_device, dist only, on the 2^20 lattice points of
           tools/points_time.py in brick order and shuffled: event time on the
           refitted tree against a fresh handle of the same deformed mesh --
           what the refit's looser boxes cost the query.

Every figure is the median of --reps (5) repeats that alternate between the
two sides (and, for the update, between the two positions, so every update
moves the mesh). Also printed: whether the two handles' distances have the same
bits, and how many pseudonormal components of the refitted handle differ from
the fresh one's (the host's acos against the device's; 0 is expected).

usage: python tools/sdf_refit_time.py [--scenes bunny,big] [--reps 5] [--json OUT]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, p) for p in ("triangles-sdf-cpu-raytracing_amd", "oracle", "tests", "tools")]


def shear(v):
    w = np.array(v, np.float32)
    w[:, 0] += (np.float32(0.15) * np.sin(np.float32(4.0) * w[:, 1])).astype(np.float32)
    return w


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", default="bunny,big")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--json")
    a = ap.parse_args()

    import torch

    import rtamd
    import scenes as S
    from points_time import point_sets

    if rtamd.device_count() < 1:
        sys.exit("sdf_refit_time.py: no HIP device visible")
    print(f"librtamd {rtamd.lib().rt_build_id().decode()} on {torch.cuda.get_device_name(0)}", flush=True)
    dev = torch.device("cuda")
    _, (v0, i0), _ = S.inputs("stanford-bunny.obj")
    sets = {k: x for k, x in point_sets(v0, i0).items() if k in ("brick", "shuffled")}
    results = []
    for key in a.scenes.split(","):
        mesh = rtamd.SimpleMesh(np.ascontiguousarray(v0, np.float32), np.ascontiguousarray(i0, np.uint32))
        if key == "big":
            mesh = rtamd.subdivide_mesh(mesh, 2)
        v, i = mesh.vPos4f, mesh.indices
        w = shear(v)
        v_t, w_t = torch.from_numpy(v).to(dev), torch.from_numpy(w).to(dev)
        st = torch.cuda.current_stream().cuda_stream
        dyn = rtamd.SDFMesh(mesh, dynamic=True)
        plain = rtamd.SDFMesh(rtamd.SimpleMesh(w, i))
        torch.cuda.synchronize()
        upd_ev, upd_host, reb = [], [], []
        events = []
        for r in range(a.reps + a.warmup):
            src = w_t if r % 2 == 0 else v_t
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            t0 = time.perf_counter()
            dyn.update_vertices_device(src.data_ptr(), len(v), stream=st)
            t1 = time.perf_counter()
            e1.record()
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            plain.close()
            plain = rtamd.SDFMesh(rtamd.SimpleMesh(w if r % 2 == 0 else v, i))
            t3 = time.perf_counter()
            if r >= a.warmup:
                events.append((e0, e1))
                upd_host.append((t1 - t0) * 1e3)
                reb.append((t3 - t2) * 1e3)
        upd_ev = [e0.elapsed_time(e1) for e0, e1 in events]
        # both handles on the sheared mesh: the refitted tree and a fresh one
        dyn.update_vertices_device(w_t.data_ptr(), len(v), stream=st)
        plain.close()
        plain = rtamd.SDFMesh(rtamd.SimpleMesh(w, i))
        pn_diff = int((dyn.pseudonormals().view(np.uint32) != plain.pseudonormals().view(np.uint32)).sum())
        res = {"scene": key, "triangles": len(i) // 3, "vertices": len(v),
               "device_bytes_plain": plain.device_bytes(), "device_bytes_dynamic": dyn.device_bytes(),
               "update_event_ms": float(np.median(upd_ev)), "update_event_ms_min_max": [min(upd_ev), max(upd_ev)],
               "update_host_ms": float(np.median(upd_host)),
               "rebuild_ms": float(np.median(reb)), "rebuild_ms_min_max": [min(reb), max(reb)],
               "rebuild_over_update": float(np.median(reb) / np.median(upd_ev)),
               "pn_components_differing": pn_diff, "pn_components": len(i) // 3 * 21, "points": {}}
        print(f"{key:6} {res['triangles']:8d} triangles: update {res['update_event_ms']:.3f} ms event time "
              f"[{min(upd_ev):.3f}, {max(upd_ev):.3f}] ({res['update_host_ms']:.3f} ms in the call), destroy + create "
              f"{res['rebuild_ms']:.1f} ms [{min(reb):.1f}, {max(reb):.1f}] = {res['rebuild_over_update']:.0f} x; "
              f"{pn_diff} of {res['pn_components']} pseudonormal components differ from a fresh handle's; device bytes "
              f"{res['device_bytes_plain']} plain, {res['device_bytes_dynamic']} dynamic", flush=True)
        for pset, host in sets.items():
            n = len(host)
            pts = torch.from_numpy(host).to(dev)
            out = {"refit": torch.empty(n, dtype=torch.float32, device=dev),
                   "fresh": torch.empty(n, dtype=torch.float32, device=dev)}
            calls = {"refit": lambda: dyn.points_device(pts.data_ptr(), n, dist_ptr=out["refit"].data_ptr(), stream=st),
                     "fresh": lambda: plain.points_device(pts.data_ptr(), n, dist_ptr=out["fresh"].data_ptr(), stream=st)}
            for _ in range(a.warmup):
                for c in calls.values():
                    c()
            torch.cuda.synchronize()
            ev = {k: [] for k in calls}
            for _ in range(a.reps):
                for k, c in calls.items():
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    c()
                    e1.record()
                    ev[k].append((e0, e1))
            torch.cuda.synchronize()
            ms = {k: [e0.elapsed_time(e1) for e0, e1 in x] for k, x in ev.items()}
            same_abs = bool(torch.equal(out["refit"].abs().view(torch.int32), out["fresh"].abs().view(torch.int32)))
            same = bool(torch.equal(out["refit"].view(torch.int32), out["fresh"].view(torch.int32)))
            mr, mf = float(np.median(ms["refit"])), float(np.median(ms["fresh"]))
            res["points"][pset] = {"n": n, "refit_ms": mr, "fresh_ms": mf, "refit_over_fresh": mr / mf,
                                   "refit_ms_all": ms["refit"], "fresh_ms_all": ms["fresh"],
                                   "same_magnitude_bits": same_abs, "same_bits": same}
            print(f"  {pset:9} {n} points: {mr:.3f} ms on the refitted tree, {mf:.3f} ms on a fresh one = {mr / mf:.3f} x; "
                  f"|dist| bits equal: {same_abs}, dist bits equal: {same}", flush=True)
        results.append(res)
        dyn.close()
        plain.close()
    if a.json:
        with open(a.json, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
