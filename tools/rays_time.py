"""Ray-batch throughput of rt_trace_rays_device (IScene.trace_device) on device
buffers: bunny, the shipped 65^3 grid and sdf_6.octree, three ray sets:
  eye      the 1080p eye rays of the standard camera (0, 0, 2.5)
  random   2^21 incoherent rays (tests/test_gpu_parity.py's _random_rays recipe)
  shadow   the shadow rays of the eye rays' hits toward the light at (2, 2, 2),
           built as lambert_color builds them (any hit only)
For each it prints Mrays/s of the three kernel modes (closest hit with all four
outputs, closest hit without the normal, any hit), timed with torch CUDA
events over 20 launches after 5 warm-ups.

usage: python tools/rays_time.py [--scenes bunny,grid,octree]
       rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o p -- \\
           python3 tools/rays_time.py --profile OUT/plan.json
       python tools/rays_time.py --summarise OUT/plan.json OUT/.../p_kernel_trace.csv
--profile: no event timing; every set goes, three times alternating, through
the host entry rt_intersect_rays (rays_kernel, the kernel this one is measured
against) and through the three modes of the new kernel, and the order of the
launches is written to the plan file. --summarise pairs the plan with the
kernel trace: kernel-only microseconds per launch, both kernels under the same
tool; the spread among rays_kernel's three is the noise margin.
"""
import argparse
import csv
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, p) for p in ("triangles-sdf-cpu-raytracing_amd", "oracle", "tests")]

SCENES = {"bunny": "stanford-bunny.obj", "grid": "example_grid.grid", "octree": "sdf_6.octree"}
MODES = ("closest+normal", "closest", "any")
W, H, POS, LIGHT = 1920, 1080, (0.0, 0.0, 2.5), (2.0, 2.0, 2.0)


def random_rays(n, seed, inside_frac=0.5):
    rng = np.random.default_rng(seed)
    o = rng.uniform(-3, 3, (n, 3)).astype(np.float32)
    m = rng.random(n) < inside_frac
    o[m] = rng.uniform(-0.9, 0.9, (int(m.sum()), 3)).astype(np.float32)
    d = rng.normal(size=(n, 3)).astype(np.float32)
    k = n // 8
    axis = rng.integers(0, 3, k)
    d[:k] = 0.0
    d[np.arange(k), axis] = rng.choice([-1.0, 1.0], k).astype(np.float32)
    d /= np.linalg.norm(d, axis=1, keepdims=True).astype(np.float32)
    return o, d.astype(np.float32)


def summarise(plan_path, trace_path):
    plan = json.load(open(plan_path))
    rows = []
    with open(trace_path) as fh:
        for row in csv.DictReader(fh):
            if "rays_kernel" in row["Kernel_Name"]:
                rows.append((int(row["Start_Timestamp"]), row["Kernel_Name"],
                             (int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3))
    rows.sort()
    if len(rows) != len(plan):
        sys.exit(f"{len(rows)} ray-kernel launches in the trace, {len(plan)} in the plan")
    us = {}
    for (_, kname, d), p in zip(rows, plan):
        if ("trace_rays_kernel" in kname) != (p["kernel"] != "rays_kernel"):
            sys.exit(f"launch order differs from the plan at {p}: {kname[:60]}")
        if not p["kernel"].endswith("(setup)"):
            us.setdefault((p["scene"], p["set"], p["kernel"]), []).append(d)
    print(f"{'scene':8}{'set':8}{'kernel':34}{'n':>9}  us per launch (in launch order)      median  Mrays/s")
    n_of = {(p["scene"], p["set"]): p["n"] for p in plan}
    for (scene, rset, kernel), v in us.items():
        med = float(np.median(v))
        print(f"{scene:8}{rset:8}{kernel:34}{n_of[scene, rset]:9d}  " + " ".join(f"{x:9.1f}" for x in v) +
              f"  {med:9.1f}  {n_of[scene, rset] / med:7.1f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", default="bunny,grid,octree")
    ap.add_argument("--profile", metavar="PLAN.json")
    ap.add_argument("--summarise", nargs=2, metavar=("PLAN.json", "kernel_trace.csv"))
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    if a.summarise:
        return summarise(*a.summarise)

    import torch

    import cpuref
    import rtamd
    import scenes as S

    if rtamd.device_count() < 1:
        sys.exit("rays_time.py: no HIP device visible")
    print(f"librtamd {rtamd.lib().rt_build_id().decode()} on {torch.cuda.get_device_name(0)}", flush=True)
    dev = torch.device("cuda")
    ro, rd = random_rays(1 << 21, 12)
    plan = []
    for key in a.scenes.split(","):
        name = SCENES[key]
        gs = S.gpu_scene(name)
        gs.set_plane(None)
        eye_d = np.ascontiguousarray(cpuref.primary_rays(S.params(name, W, H, "primary", POS, "ref"), W, H)
                                     .reshape(-1, 3))
        eye_o = np.tile(np.float32(POS), (len(eye_d), 1))
        sets = {"eye": (eye_o, eye_d), "random": (ro, rd)}
        dsets = {k: (torch.from_numpy(o).to(dev), torch.from_numpy(d).to(dev)) for k, (o, d) in sets.items()}
        # the shadow rays of the eye rays' hits (lambert_color: from the hit
        # point moved 0.3 along the unit direction to the light)
        o_t, d_t = dsets["eye"]
        n = o_t.shape[0]
        hit = torch.empty(n, dtype=torch.int32, device=dev)
        t = torch.empty(n, dtype=torch.float32, device=dev)
        gs.trace_device(o_t.data_ptr(), d_t.data_ptr(), n, hit_ptr=hit.data_ptr(), t_ptr=t.data_ptr())
        plan.append({"scene": key, "set": "eye", "n": n, "kernel": "trace_rays_kernel (setup)"})
        m = hit != 0
        point = o_t[m] + t[m, None] * d_t[m]
        sd = torch.tensor(LIGHT, device=dev) - point
        sd = sd / sd.norm(dim=1, keepdim=True)
        dsets["shadow"] = ((point + 0.3 * sd).contiguous(), sd.contiguous())
        sets["shadow"] = tuple(x.cpu().numpy() for x in dsets["shadow"])
        torch.cuda.synchronize()
        for rset, (o_t, d_t) in dsets.items():
            n = o_t.shape[0]
            out = {"hit": torch.empty(n, dtype=torch.int32, device=dev),
                   "t": torch.empty(n, dtype=torch.float32, device=dev),
                   "normal": torch.empty((n, 3), dtype=torch.float32, device=dev),
                   "prim": torch.empty(n, dtype=torch.int64, device=dev)}
            p = {k: v.data_ptr() for k, v in out.items()}
            calls = {
                "closest+normal": lambda: gs.trace_device(o_t.data_ptr(), d_t.data_ptr(), n, hit_ptr=p["hit"],
                                                          t_ptr=p["t"], normal_ptr=p["normal"], prim_ptr=p["prim"]),
                "closest": lambda: gs.trace_device(o_t.data_ptr(), d_t.data_ptr(), n, hit_ptr=p["hit"],
                                                   t_ptr=p["t"], prim_ptr=p["prim"]),
                "any": lambda: gs.trace_device(o_t.data_ptr(), d_t.data_ptr(), n, hit_ptr=p["hit"], any_hit=True),
            }
            if a.profile:
                ho, hd = sets[rset]
                for _ in range(a.reps):
                    gs.intersect(ho, hd, 0.01, 100.0)
                    plan.append({"scene": key, "set": rset, "n": n, "kernel": "rays_kernel"})
                    for mode in MODES:
                        calls[mode]()
                        plan.append({"scene": key, "set": rset, "n": n, "kernel": "trace_rays_kernel " + mode})
                    torch.cuda.synchronize()
                continue
            line = f"{key:7} {rset:7} {n:8d} rays:"
            for mode in MODES:
                for _ in range(a.warmup):
                    calls[mode]()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.launches):
                    calls[mode]()
                e1.record()
                e1.synchronize()
                ms = e0.elapsed_time(e1) / a.launches
                line += f"  {mode} {n / ms / 1e3:8.1f} Mrays/s ({ms * 1e3:8.1f} us)"
            print(line, flush=True)
    if a.profile:
        with open(a.profile, "w") as f:
            json.dump(plan, f)
        print(f"{len(plan)} launches planned -> {a.profile}")


if __name__ == "__main__":
    main()
