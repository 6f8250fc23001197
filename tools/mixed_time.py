"""Ray-batch time of mixed instanced scenes (rtamd.InstancedScene over meshes,
SDF grids and SDF octrees; rt_scene_create_instanced_any), in one process.

The lattice, the ray sets and the timing are tools/instances_time.py's: K = 1,
8, 64 and 256 placements (pitch 2.2, pure translations, so every pose is
rigid), the 1080p eye rays of a camera that sees the whole lattice and 2^21
incoherent rays through its box; closest hit with all four outputs, and any
hit; the flat list and the top-level tree. Three populations:
  mesh  all bunnies, through the mixed kernels (one disabled octree instance
        placed last makes the scene mixed), against the mesh-only scene of the
        same bunnies: what the kind branch costs where nothing is gained
  sdf   all sdf_6.octree
  mix   bunny, example_grid.grid, sdf_6.octree in turn
Baselines, at K = 1 and 8 only:
  loop  what a caller does without the feature: one trace per instance on
        rays transformed in torch, combined with torch.where (closest hit: t,
        hit and prim; no normal, which would need one more pass per instance)
  plain at K = 1, the plain scene's own trace of the same rays: the layer's
        overhead
Every figure is the time per launch from torch CUDA events around `--launches`
back-to-back launches (after `--warmup`), taken `--reps` times with the
variants alternating, and reported as the median.

usage: python tools/mixed_time.py [--counts 1,8,64,256] [--json OUT.json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, p) for p in ("triangles-sdf-cpu-raytracing_amd", "oracle", "tests", "tools")]

import instances_time as IT  # noqa: E402  (the lattice, the ray sets)

POPULATIONS = {"mesh": ("bunny",), "sdf": ("octree",), "mix": ("bunny", "grid", "octree")}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--counts", default="1,8,64,256")
    ap.add_argument("--populations", default="mesh,sdf,mix")
    ap.add_argument("--launches", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--loop-max", type=int, default=8, help="the per-instance baseline up to this K")
    ap.add_argument("--json")
    a = ap.parse_args()

    import torch

    import cpuref
    import rtamd
    import scenes as S

    if rtamd.device_count() < 1:
        sys.exit("mixed_time.py: no HIP device visible")
    print(f"librtamd {rtamd.lib().rt_build_id().decode()} on {torch.cuda.get_device_name(0)}", flush=True)
    dev = torch.device("cuda")
    blas = {"bunny": rtamd.BVHBuilder(rtamd.SimpleMesh(*S.inputs("stanford-bunny.obj")[1])),
            "grid": rtamd.SDFGrid(*S.inputs("example_grid.grid")[1]),
            "octree": rtamd.SDFOctree(S.inputs("sdf_6.octree")[1])}
    results = []

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
        xf = IT.xforms(centres)
        rays = {name: (torch.from_numpy(o).to(dev), torch.from_numpy(d).to(dev)) for name, (o, d) in IT.ray_sets(k, cpuref).items()}
        for pop in a.populations.split(","):
            kinds = POPULATIONS[pop]
            which = [kinds[j % len(kinds)] for j in range(k)]
            names = list(kinds)
            inst = [(names.index(w), xf[j], 0) for j, w in enumerate(which)]
            objs = [blas[n] for n in names]
            variants = {}
            if pop == "mesh":
                # the same bunnies through both sets of kernels
                forced = inst + [(1, xf[0], rtamd.InstancedScene.DISABLED)]
                for tl in (False, True):
                    variants[f"mesh-only {'tree' if tl else 'flat'}"] = rtamd.InstancedScene(objs, inst, tlas=tl)
                    variants[f"mixed {'tree' if tl else 'flat'}"] = rtamd.InstancedScene(objs + [blas["octree"]], forced, tlas=tl)
                    assert variants[f"mixed {'tree' if tl else 'flat'}"].mixed
            else:
                for tl in (False, True):
                    variants[f"mixed {'tree' if tl else 'flat'}"] = rtamd.InstancedScene(objs, inst, tlas=tl)
            for rset, (o_t, d_t) in rays.items():
                n = o_t.shape[0]
                out = {"hit": torch.empty(n, dtype=torch.int32, device=dev), "t": torch.empty(n, dtype=torch.float32, device=dev),
                       "normal": torch.empty((n, 3), dtype=torch.float32, device=dev),
                       "prim": torch.empty(n, dtype=torch.int64, device=dev)}
                p = {key: x.data_ptr() for key, x in out.items()}

                def caller(sc, mode, o=o_t, d=d_t):
                    if mode == "any":
                        return lambda: sc.trace_device(o.data_ptr(), d.data_ptr(), n, hit_ptr=p["hit"], any_hit=True)
                    return lambda: sc.trace_device(o.data_ptr(), d.data_ptr(), n, hit_ptr=p["hit"], t_ptr=p["t"],
                                                   normal_ptr=p["normal"], prim_ptr=p["prim"])

                # the caller's loop of today: transform, trace each instance, reduce
                c_t = torch.from_numpy(centres.astype(np.float32)).to(dev)
                best = torch.empty(n, dtype=torch.float32, device=dev)
                bprim = torch.empty(n, dtype=torch.int64, device=dev)
                oo = torch.empty_like(o_t)

                def loop(mode):
                    def run():
                        best.fill_(float("inf"))
                        bprim.fill_(-1)
                        for j, w in enumerate(which):
                            torch.sub(o_t, c_t[j], out=oo)  # pure translations: d' = d
                            if mode == "any":
                                blas[w].trace_device(oo.data_ptr(), d_t.data_ptr(), n, hit_ptr=p["hit"], any_hit=True)
                                bprim.copy_(torch.where(out["hit"] != 0, 0, bprim))
                            else:
                                blas[w].trace_device(oo.data_ptr(), d_t.data_ptr(), n, hit_ptr=p["hit"], t_ptr=p["t"], prim_ptr=p["prim"])
                                win = (out["hit"] != 0) & (out["t"] < best)
                                best.copy_(torch.where(win, out["t"], best))
                                bprim.copy_(torch.where(win, out["prim"] | (j << 32), bprim))
                    return run

                for mode in ("closest+normal", "any"):
                    calls = {name: caller(sc, mode) for name, sc in variants.items()}
                    if k <= a.loop_max:
                        calls["loop"] = loop(mode)
                    if k == 1 and pop != "mix":
                        calls["plain"] = caller(blas[which[0]], mode, oo)  # oo = o - centre 0 from the loop's last pass
                        torch.sub(o_t, c_t[0], out=oo)
                    us = {name: [] for name in calls}
                    for _ in range(a.reps):  # alternating repeats
                        for name, call in calls.items():
                            us[name].append(timed(call))
                    med = {name: float(np.median(x)) for name, x in us.items()}
                    line = f"K {k:4d} {pop:5} {rset:6} {mode:14} {n:8d} rays:"
                    for name in calls:
                        line += f"  {name} {med[name]:9.1f} us ({min(us[name]):.1f}-{max(us[name]):.1f})"
                    print(line, flush=True)
                    results.append({"K": k, "population": pop, "set": rset, "mode": mode, "rays": n, "us_median": med, "us_all": us})
            for sc in variants.values():
                sc.close()
    if a.json:
        with open(a.json, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
