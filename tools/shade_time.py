"""Time of shaded ray queries (rt_shade_rays_device, rt_eye_rays_device) at 1080p.

plain      the bunny above its base plane, Lambert with shadows and
           reflections, one process, one build:
             frame        rt_render_device, one cleared frame
             shade        rt_shade_rays_device on pre-generated eye rays
             eye+shade    rt_eye_rays_device, then the shade
             trace        rt_trace_rays_device (closest hit, t / normal / prim)
                          on the same rays: what the shading adds to a query
instanced  tools/instances_time.py's bunny lattice at K = 1, 8, 64, 256 above a
           plane under the lattice, its 1080p eye rays, the same shading:
           the flat list, the top-level tree and the flattened mesh through
           the plain path, shade and trace each; shaded rays per second.

Every figure is the time per launch from torch CUDA events around `--launches`
back-to-back launches (after `--warmup`), taken `--reps` times with the
variants alternating, and reported as the median (min-max). A library built by
tools/build_variant.sh is selected through RTAMD_LIB, one process per library.

usage: python tools/shade_time.py [--parts plain,instanced] [--counts 1,8,64,256] [--json OUT.json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, p) for p in ("triangles-sdf-cpu-raytracing_amd", "oracle", "tests", "tools")]

import instances_time as IT  # noqa: E402  (the lattice, its camera)

W, H = IT.W, IT.H
CAMERA = (0.9, 0.7, 2.3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="plain,instanced")
    ap.add_argument("--counts", default="1,8,64,256")
    ap.add_argument("--launches", type=int, default=20)
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
        sys.exit("shade_time.py: no HIP device visible")
    print(f"librtamd {rtamd.lib().rt_build_id().decode()} on {torch.cuda.get_device_name(0)}", flush=True)
    dev = torch.device("cuda")
    n = W * H
    v, i = S.inputs("stanford-bunny.obj")[1]
    blas = rtamd.BVHBuilder(rtamd.SimpleMesh(v, i))
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

    def params(pos, light):
        vi, pi = cpuref.camera_matrices(pos, (0, 0, 0), (0, 1, 0), 45.0, W / H, 0.01, 100.0)
        return rtamd.render_params(pos, vi, pi, light, rtamd.ShadingMode.Lambert, True, True)

    out = {"color": torch.empty(n, dtype=torch.int32, device=dev), "t": torch.empty(n, dtype=torch.float32, device=dev),
           "hit": torch.empty(n, dtype=torch.int32, device=dev), "prim": torch.empty(n, dtype=torch.int64, device=dev),
           "normal": torch.empty((n, 3), dtype=torch.float32, device=dev)}
    p = {k: x.data_ptr() for k, x in out.items()}

    def shade_call(sc, o_t, d_t, P):
        return lambda: sc.shade_device(o_t.data_ptr(), d_t.data_ptr(), n, P, p["color"], t_ptr=p["t"])

    def trace_call(sc, o_t, d_t):
        return lambda: sc.trace_device(o_t.data_ptr(), d_t.data_ptr(), n, t_ptr=p["t"], normal_ptr=p["normal"],
                                       prim_ptr=p["prim"])

    def report(title, calls):
        us = {name: [] for name in calls}
        for _ in range(a.reps):  # alternating repeats
            for name, call in calls.items():
                us[name].append(timed(call))
        med = {name: float(np.median(x)) for name, x in us.items()}
        print(title + "  " + "  ".join(f"{name} {med[name]:9.1f} us ({min(us[name]):.1f}-{max(us[name]):.1f})" for name in calls),
              flush=True)
        return med, us

    if "plain" in a.parts.split(","):
        blas.set_plane(rtamd.Plane((0.0, 1.0, 0.0), S.inputs("stanford-bunny.obj")[2]))
        P = params(CAMERA, (2.0, 2.0, 2.0))
        o_t, d_t = torch_rays.eye_rays(P, W, H)

        def eye_shade():
            rtamd.api.eye_rays_device(P, W, H, o_t.data_ptr(), d_t.data_ptr())
            blas.shade_device(o_t.data_ptr(), d_t.data_ptr(), n, P, p["color"], t_ptr=p["t"])

        calls = {"frame": lambda: blas.render_device(P, p["color"], p["t"], W, H, clear=True),
                 "shade": shade_call(blas, o_t, d_t, P), "eye+shade": eye_shade,
                 "eye": lambda: rtamd.api.eye_rays_device(P, W, H, o_t.data_ptr(), d_t.data_ptr()),
                 "trace": trace_call(blas, o_t, d_t)}
        med, us = report(f"plain bunny + plane, {n} rays:", calls)
        stored = int((out["t"] < float("inf")).sum())
        print(f"  shade / frame {med['shade'] / med['frame']:.2f}  eye+shade / frame {med['eye+shade'] / med['frame']:.2f}  "
              f"shade / trace {med['shade'] / med['trace']:.2f}  {n / med['shade']:.0f} M shaded rays/s  ({stored} pixels stored)",
              flush=True)
        results.append({"part": "plain", "rays": n, "us_median": med, "us_all": us})
        blas.set_plane(None)

    if "instanced" in a.parts.split(","):
        for k in (int(x) for x in a.counts.split(",")):
            centres = IT.lattice(k)
            inst = [(0, x, 0) for x in IT.xforms(centres)]
            half = (np.float64(IT.DIMS[k]) - 1) / 2 * IT.PITCH + 1.0
            variants = {"flat": rtamd.InstancedScene([blas], inst), "tlas": rtamd.InstancedScene([blas], inst, tlas=True),
                        "flattened": rtamd.BVHBuilder(rtamd.SimpleMesh(*IT.flatten(v, i, centres)))}
            for sc in variants.values():
                sc.set_plane(rtamd.Plane((0.0, 1.0, 0.0), float(-half[1])))
            eye_o, eye_d = IT.ray_sets(k, cpuref)["eye"]
            o_t, d_t = torch.from_numpy(eye_o).to(dev), torch.from_numpy(eye_d).to(dev)
            P = params(tuple(float(x) for x in eye_o[0]), (float(half[0]) + 2.0, float(half[1]) + 4.0, float(eye_o[0][2])))
            calls = {}
            for name, sc in variants.items():
                calls[f"{name} shade"] = shade_call(sc, o_t, d_t, P)
                calls[f"{name} trace"] = trace_call(sc, o_t, d_t)
            med, us = report(f"K {k:4d}, {n} eye rays:", calls)
            print("  " + "  ".join(f"{name}: {n / med[name + ' shade']:.0f} M shaded rays/s, shade / trace "
                                   f"{med[name + ' shade'] / med[name + ' trace']:.2f}" for name in variants) +
                  f"  tlas / flat {med['tlas shade'] / med['flat shade']:.3f}  tlas / flattened "
                  f"{med['tlas shade'] / med['flattened shade']:.2f}", flush=True)
            results.append({"part": "instanced", "K": k, "rays": n, "us_median": med, "us_all": us})
            for sc in variants.values():
                sc.close()
    if a.json:
        with open(a.json, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
