"""Ray-batch time of instanced scenes (rtamd.InstancedScene, rt_trace_rays_device)
against the same geometry flattened into one mesh scene.

K = 1, 8, 64 and 256 placements of the bunny on a lattice (pitch 2.2, pure
translations), two ray sets:
  eye      the 1080p eye rays of a camera that sees the whole lattice
  random   2^21 incoherent rays through the lattice's box
and two modes: closest hit with all four outputs, and any hit. Every figure is
the time per launch from torch CUDA events around `--launches` back-to-back
launches (after `--warmup`), taken `--reps` times with the variants
alternating -- instanced, flattened, and for K = 1 (identity matrix) the plain
BLAS trace, which shows the layer's own overhead -- and reported as the median.
Last, one rt_scene_update_instances_device of 256 poses (device events) against
destroy + create of the flattened 256-bunny scene (host clock around the
synchronised calls).

usage: python tools/instances_time.py [--counts 1,8,64,256] [--json OUT.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, p) for p in ("triangles-sdf-cpu-raytracing_amd", "oracle", "tests")]

W, H = 1920, 1080
PITCH = 2.2
DIMS = {1: (1, 1, 1), 8: (2, 2, 2), 64: (4, 4, 4), 256: (8, 8, 4)}


def lattice(k):
    """k translations on a centred nx x ny x nz lattice -> float64 [k, 3]."""
    nx, ny, nz = DIMS[k]
    g = np.stack(np.meshgrid(np.arange(nx), np.arange(ny), np.arange(nz), indexing="ij"), -1).reshape(-1, 3)
    return (g - (np.float64([nx, ny, nz]) - 1) / 2) * PITCH


def xforms(centres):
    x = np.zeros((len(centres), 3, 4), np.float32)
    x[:, 0, 0] = x[:, 1, 1] = x[:, 2, 2] = 1.0
    x[:, :, 3] = centres
    return x


def flatten(v, i, centres):
    """One mesh of all placements: positions divided by w, moved in float32."""
    p = (v[:, :3] / v[:, 3:4]).astype(np.float32)
    vs, ids = [], []
    for k, c in enumerate(centres):
        w = np.ones((len(p), 4), np.float32)
        w[:, :3] = p + c.astype(np.float32)
        vs.append(w)
        ids.append(i + np.uint32(k * len(p)))
    return np.concatenate(vs), np.concatenate(ids).astype(np.uint32)


def ray_sets(k, cpuref):
    half = (np.float64(DIMS[k]) - 1) / 2 * PITCH + 1.0  # the lattice's box, bunnies included
    # the camera looks down -z from where a 45 degree frustum holds the box
    dist = float(half[2] + 1.3 * max(half[0] / (W / H), half[1]) / np.tan(np.radians(22.5)))
    pos = (0.0, 0.0, dist)
    vi, pi = cpuref.camera_matrices(pos, (0, 0, 0), (0, 1, 0), 45.0, W / H, 0.01, 100.0)
    eye_d = np.ascontiguousarray(cpuref.primary_rays(cpuref.make_params(pos, vi, pi), W, H).reshape(-1, 3))
    eye_o = np.tile(np.float32(pos), (len(eye_d), 1))
    rng = np.random.default_rng(14 + k)
    n = 1 << 21
    ro = rng.uniform(-1, 1, (n, 3)) * (half + 1.0)
    rd = rng.normal(size=(n, 3))
    rd /= np.linalg.norm(rd, axis=1, keepdims=True)
    return {"eye": (eye_o, eye_d), "random": (ro.astype(np.float32), rd.astype(np.float32))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--counts", default="1,8,64,256")
    ap.add_argument("--launches", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--json")
    a = ap.parse_args()

    import torch

    import cpuref
    import rtamd
    import scenes as S
    from rtamd import torch_rays

    if rtamd.device_count() < 1:
        sys.exit("instances_time.py: no HIP device visible")
    print(f"librtamd {rtamd.lib().rt_build_id().decode()} on {torch.cuda.get_device_name(0)}", flush=True)
    dev = torch.device("cuda")
    v, i = S.inputs("stanford-bunny.obj")[1]
    blas = rtamd.BVHBuilder(rtamd.SimpleMesh(v, i))
    print(f"bunny: {len(i) // 3} triangles", flush=True)
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
        centres = lattice(k)
        inst = rtamd.InstancedScene([blas], [(0, x, 0) for x in xforms(centres)])
        t0 = time.perf_counter()
        flat = rtamd.BVHBuilder(rtamd.SimpleMesh(*flatten(v, i, centres)))
        print(f"K = {k}: flattened scene of {k * (len(i) // 3)} triangles created in {time.perf_counter() - t0:.2f} s; "
              f"instanced scene holds {inst.device_bytes()} bytes", flush=True)
        variants = {"instanced": inst, "flattened": flat}
        if k == 1:
            variants["plain BLAS"] = blas
        for rset, (o, d) in ray_sets(k, cpuref).items():
            o_t, d_t = torch.from_numpy(o).to(dev), torch.from_numpy(d).to(dev)
            n = o_t.shape[0]
            out = {"hit": torch.empty(n, dtype=torch.int32, device=dev), "t": torch.empty(n, dtype=torch.float32, device=dev),
                   "normal": torch.empty((n, 3), dtype=torch.float32, device=dev),
                   "prim": torch.empty(n, dtype=torch.int64, device=dev)}
            p = {key: x.data_ptr() for key, x in out.items()}
            for mode in ("closest+normal", "any"):
                us = {name: [] for name in variants}
                hits = {}
                for _ in range(a.reps):  # alternating repeats
                    for name, sc in variants.items():
                        if mode == "any":
                            call = lambda: sc.trace_device(o_t.data_ptr(), d_t.data_ptr(), n, hit_ptr=p["hit"], any_hit=True)
                        else:
                            call = lambda: sc.trace_device(o_t.data_ptr(), d_t.data_ptr(), n, hit_ptr=p["hit"], t_ptr=p["t"],
                                                           normal_ptr=p["normal"], prim_ptr=p["prim"])
                        us[name].append(timed(call))
                        hits[name] = int(out["hit"].sum())
                med = {name: float(np.median(x)) for name, x in us.items()}
                line = f"K {k:3d} {rset:6} {mode:14} {n:8d} rays, {hits['instanced']:8d} hits:"
                for name in variants:
                    line += f"  {name} {med[name]:9.1f} us ({min(us[name]):.1f}-{max(us[name]):.1f})"
                line += f"  instanced / flattened {med['instanced'] / med['flattened']:.2f}"
                if k == 1:
                    line += f"  instanced / plain {med['instanced'] / med['plain BLAS']:.3f}"
                print(line, flush=True)
                if len(set(hits.values())) != 1:
                    print(f"  note: hit counts differ between the variants: {hits}", flush=True)
                results.append({"K": k, "set": rset, "mode": mode, "rays": n, "hits": hits, "us_median": med, "us_all": us})
        if k == 256:
            # one device pose update of all 256 poses against destroy + create of the flattened scene
            x_t = torch.from_numpy(xforms(centres)).to(dev)
            upd = [timed(lambda: torch_rays.update_instances(inst, x_t)) for _ in range(a.reps)]
            fv, fi = flatten(v, i, centres)
            rebuild = []
            for _ in range(3):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                flat.close()
                flat = rtamd.BVHBuilder(rtamd.SimpleMesh(fv, fi))
                torch.cuda.synchronize()
                rebuild.append((time.perf_counter() - t0) * 1e3)
            print(f"pose update of 256 instances: {np.median(upd):.1f} us per launch ({min(upd):.1f}-{max(upd):.1f}); "
                  f"destroy + create of the flattened scene: {np.median(rebuild):.1f} ms "
                  f"({min(rebuild):.1f}-{max(rebuild):.1f})", flush=True)
            results.append({"pose_update_256_us": upd, "flattened_destroy_create_ms": rebuild})
        inst.close()
        flat.close()
    if a.json:
        with open(a.json, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
