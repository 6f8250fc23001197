"""Ray-batch time of instanced scenes with a top-level tree
(rtamd.InstancedScene(..., tlas=True), RT_INSTANCED_TLAS) against the flat list
(the same call with tlas=False) and the same geometry flattened into one mesh,
in one process.

The lattice, the ray sets and the timing are tools/instances_time.py's: K = 1,
8, 64, 256 and 1024 placements of the bunny (pitch 2.2, pure translations, in
the lattice's own index order unless --morton), the 1080p eye rays of a camera
that sees the whole lattice and 2^21 incoherent rays through its box; closest
hit with all four outputs, and any hit. Every figure is the time per launch from
torch CUDA events around `--launches` back-to-back launches (after `--warmup`),
taken `--reps` times with the variants alternating, and reported as the median.
Besides:
  * BLAS traversals per ray of the TLAS scene (the kernel's own counter,
    rtx_set_tlas_count; the flat list offers every ray all K instances),
  * the alternating pairs the TLAS scene wins against the flat list,
  * one device pose update of all K poses, TLAS scene against flat scene,
  * the sweep of the shared path's lane threshold (rtx_set_tlas_uniform_min)
    over --sweep-counts, summed over both ray sets and both modes.

usage: python tools/tlas_time.py [--counts 1,8,64,256,1024] [--json OUT.json]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, p) for p in ("triangles-sdf-cpu-raytracing_amd", "oracle", "tests", "tools")]

import instances_time as IT  # noqa: E402  (the lattice, the ray sets)

IT.DIMS[1024] = (16, 8, 8)
UMINS = (1, 16, 32, 65)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--counts", default="1,8,64,256,1024")
    ap.add_argument("--sweep-counts", default="64,256")
    ap.add_argument("--flatten-max", type=int, default=1024, help="no flattened mesh above this K (71 M triangles at 1024)")
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--morton", action="store_true", help="instances in rtamd.morton_order of their centres")
    ap.add_argument("--json")
    a = ap.parse_args()

    import torch

    import cpuref
    import rtamd
    import scenes as S
    from rtamd import torch_rays

    if rtamd.device_count() < 1:
        sys.exit("tlas_time.py: no HIP device visible")
    L = rtamd.lib()
    print(f"librtamd {L.rt_build_id().decode()} on {torch.cuda.get_device_name(0)}", flush=True)
    dev = torch.device("cuda")
    v, i = S.inputs("stanford-bunny.obj")[1]
    blas = rtamd.BVHBuilder(rtamd.SimpleMesh(v, i))
    results = []
    sweep_counts = [int(x) for x in a.sweep_counts.split(",") if x]
    sweep_sum = {u: 0.0 for u in UMINS}

    def timed(call):
        for _ in range(a.warmup):
            call()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.launches):
            call()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / a.launches * 1e3  # us per launch

    for k in (int(x) for x in a.counts.split(",")):
        centres = IT.lattice(k)
        if a.morton:
            centres = centres[rtamd.morton_order(centres)]
        inst = [(0, x, 0) for x in IT.xforms(centres)]
        variants = {"flat": rtamd.InstancedScene([blas], inst), "tlas": rtamd.InstancedScene([blas], inst, tlas=True)}
        if k <= a.flatten_max:
            t0 = time.perf_counter()
            variants["flattened"] = rtamd.BVHBuilder(rtamd.SimpleMesh(*IT.flatten(v, i, centres)))
            print(f"K = {k}: flattened scene of {k * (len(i) // 3)} triangles created in {time.perf_counter() - t0:.2f} s",
                  flush=True)
        print(f"K = {k}: flat scene {variants['flat'].device_bytes()} bytes, TLAS scene {variants['tlas'].device_bytes()} bytes",
              flush=True)
        for rset, (o, d) in IT.ray_sets(k, cpuref).items():
            o_t, d_t = torch.from_numpy(o).to(dev), torch.from_numpy(d).to(dev)
            n = o_t.shape[0]
            out = {"hit": torch.empty(n, dtype=torch.int32, device=dev), "t": torch.empty(n, dtype=torch.float32, device=dev),
                   "normal": torch.empty((n, 3), dtype=torch.float32, device=dev),
                   "prim": torch.empty(n, dtype=torch.int64, device=dev)}
            p = {key: x.data_ptr() for key, x in out.items()}

            def caller(sc, mode):
                if mode == "any":
                    return lambda: sc.trace_device(o_t.data_ptr(), d_t.data_ptr(), n, hit_ptr=p["hit"], any_hit=True)
                return lambda: sc.trace_device(o_t.data_ptr(), d_t.data_ptr(), n, hit_ptr=p["hit"], t_ptr=p["t"],
                                               normal_ptr=p["normal"], prim_ptr=p["prim"])

            # BLAS traversals per ray of the TLAS scene, by the kernel's own counter
            cnt = torch.zeros(n, dtype=torch.int32, device=dev)
            L.rtx_set_tlas_count(C.c_void_p(cnt.data_ptr()))
            caller(variants["tlas"], "closest+normal")()
            torch.cuda.synchronize()
            L.rtx_set_tlas_count(None)
            trav = float(cnt.double().mean())
            for mode in ("closest+normal", "any"):
                us = {name: [] for name in variants}
                hits = {}
                for _ in range(a.reps):  # alternating repeats
                    for name, sc in variants.items():
                        us[name].append(timed(caller(sc, mode)))
                        hits[name] = int(out["hit"].sum())
                med = {name: float(np.median(x)) for name, x in us.items()}
                won = sum(1 for f, t in zip(us["flat"], us["tlas"]) if t < f)
                line = f"K {k:4d} {rset:6} {mode:14} {n:8d} rays, {hits['tlas']:8d} hits:"
                for name in variants:
                    line += f"  {name} {med[name]:9.1f} us ({min(us[name]):.1f}-{max(us[name]):.1f})"
                line += f"  tlas / flat {med['tlas'] / med['flat']:.3f} (tlas wins {won}/{a.reps} pairs)"
                if "flattened" in med:
                    line += f"  tlas / flattened {med['tlas'] / med['flattened']:.2f}"
                line += f"  BLAS traversals per ray {k} -> {trav:.2f}"
                print(line, flush=True)
                if len(set(hits.values())) != 1:
                    print(f"  note: hit counts differ between the variants: {hits}", flush=True)
                rec = {"K": k, "set": rset, "mode": mode, "rays": n, "hits": hits, "us_median": med, "us_all": us,
                       "tlas_pairs_won": won, "tlas_traversals_per_ray": trav}
                if k in sweep_counts:
                    sw = {u: [] for u in UMINS}
                    for _ in range(a.reps):
                        for u in UMINS:
                            L.rtx_set_tlas_uniform_min(u)
                            sw[u].append(timed(caller(variants["tlas"], mode)))
                    L.rtx_set_tlas_uniform_min(0)  # the shipped default
                    smed = {u: float(np.median(x)) for u, x in sw.items()}
                    for u in UMINS:
                        sweep_sum[u] += smed[u]
                    print(f"       umin sweep: " + "  ".join(f"{u}: {smed[u]:.1f} us" for u in UMINS), flush=True)
                    rec["umin_sweep_us"] = {str(u): x for u, x in sw.items()}
                results.append(rec)
        # one device pose update of all K poses
        x_t = torch.from_numpy(IT.xforms(centres)).to(dev)
        upd = {name: [] for name in ("flat", "tlas")}
        for _ in range(a.reps):
            for name in upd:
                upd[name].append(timed(lambda: torch_rays.update_instances(variants[name], x_t)))
        print(f"K {k:4d} pose update of all {k} poses: " +
              "  ".join(f"{name} {np.median(x):.1f} us ({min(x):.1f}-{max(x):.1f})" for name, x in upd.items()), flush=True)
        results.append({"K": k, "pose_update_us": upd})
        for sc in variants.values():
            sc.close()
    if sweep_counts:
        best = min(UMINS, key=lambda u: sweep_sum[u])
        print(f"umin sweep, summed medians over K in {sweep_counts}, both ray sets, both modes: " +
              "  ".join(f"{u}: {sweep_sum[u]:.1f} us" for u in UMINS) + f"  -> lowest: {best}", flush=True)
        results.append({"umin_sweep_sum_us": {str(u): s for u, s in sweep_sum.items()}, "umin_lowest": best})
    if a.json:
        with open(a.json, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
