"""Point-query time of rt_sdf_mesh_points_device (SDFMesh.points_device) on
device buffers: the bunny, 2^20 points in three orders
  brick     a 128 x 128 x 64 lattice over [-1,1]^3, each 64 consecutive points
            one 4x4x4 brick (the order rt_sdf_mesh_grid's kernel walks)
  shuffled  the same points in random order
  surface   points within 0.01 of the surface (a random point of a random
            triangle plus a random offset of length <= 0.01)
each timed four ways: dist only, all four outputs, RT_POINTS_UNSIGNED (dist
only) and dist only within radius 0.05. Event time per launch (torch CUDA
events around the one launch), the median of 5 repeats that alternate between
the four.

usage: python tools/points_time.py
       rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o p -- \\
           python3 tools/points_time.py --profile OUT/plan.json
       python tools/points_time.py --summarise OUT/plan.json OUT/.../p_kernel_trace.csv
--profile: no event timing; every order goes, five times alternating, through
the host entry rt_sdf_mesh_points (sdf_kernel<false>, the kernel this one is
measured against; 2^20 points are one staged batch, so one launch) and through
the new kernel, dist only and unbounded, and the order of the launches is
written to the plan file. --summarise pairs the plan with the kernel trace:
kernel-only microseconds per launch, both kernels under the same tool; the
spread among sdf_kernel's five is the noise margin the new kernel is held to.
--lds-pad B[,B...]: the event timing once per value, with B unused bytes of
LDS added to every launch (rtx_set_points_lds_pad): the same kernel at fewer
workgroups per CU, i.e. what the stack's LDS footprint costs or would give back.
"""
import argparse
import csv
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, p) for p in ("triangles-sdf-cpu-raytracing_amd", "oracle", "tests")]

MESH = "stanford-bunny.obj"
SIZE = (128, 128, 64)
MODES = ("dist", "all four", "unsigned", "radius 0.05")
REPS = 5


def point_sets(v, i, seed=20):
    n0, n1, n2 = SIZE
    # brick order: block (ib, jb, kb) row-major, lane = (i & 3) * 16 + (j & 3) * 4 + (k & 3)
    b = np.arange(n0 * n1 * n2, dtype=np.int64)
    lane, blk = b % 64, b // 64
    kb, jb, ib = blk % (n2 // 4), (blk // (n2 // 4)) % (n1 // 4), blk // ((n2 // 4) * (n1 // 4))
    ijk = np.stack([ib * 4 + lane // 16, jb * 4 + (lane // 4) % 4, kb * 4 + lane % 4], 1).astype(np.float32)
    brick = (np.float32(2.0) * ijk / (np.asarray(SIZE, np.float32) - 1) - np.float32(1.0)).astype(np.float32)
    rng = np.random.default_rng(seed)
    shuffled = brick[rng.permutation(len(brick))]
    p = (v[:, :3] / v[:, 3:4]).astype(np.float64)
    t = np.asarray(i, np.int64).reshape(-1, 3)[rng.integers(0, len(i) // 3, len(brick))]
    u = rng.random((len(brick), 2))
    flip = u.sum(1) > 1
    u[flip] = 1 - u[flip]
    on = p[t[:, 0]] + u[:, :1] * (p[t[:, 1]] - p[t[:, 0]]) + u[:, 1:] * (p[t[:, 2]] - p[t[:, 0]])
    d = rng.normal(size=on.shape)
    d *= (0.01 * rng.random((len(on), 1))) / np.linalg.norm(d, axis=1, keepdims=True)
    return {"brick": brick, "shuffled": np.ascontiguousarray(shuffled),
            "surface": np.ascontiguousarray((on + d).astype(np.float32))}


def summarise(plan_path, trace_path):
    plan = json.load(open(plan_path))
    rows = []
    with open(trace_path) as fh:
        for row in csv.DictReader(fh):
            if "sdf_kernel" in row["Kernel_Name"] or "points_kernel" in row["Kernel_Name"]:
                rows.append((int(row["Start_Timestamp"]), row["Kernel_Name"],
                             (int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3))
    rows.sort()
    if len(rows) != len(plan):
        sys.exit(f"{len(rows)} point-kernel launches in the trace, {len(plan)} in the plan")
    us = {}
    for (_, kname, d), p in zip(rows, plan):
        if ("points_kernel" in kname) != (p["kernel"] == "points_kernel"):
            sys.exit(f"launch order differs from the plan at {p}: {kname[:60]}")
        us.setdefault((p["set"], p["kernel"]), []).append(d)
    print(f"{'set':10}{'kernel':16}  us per launch (in launch order)" + " " * 24 + "median  spread")
    for (pset, kernel), v in us.items():
        med = float(np.median(v))
        print(f"{pset:10}{kernel:16}  " + " ".join(f"{x:9.1f}" for x in v) +
              f"  {med:9.1f}  {(max(v) - min(v)) / med * 100:5.2f} %")
    print()
    for pset in dict.fromkeys(k[0] for k in us):
        a, b = us[pset, "sdf_kernel"], us[pset, "points_kernel"]
        ma, mb = float(np.median(a)), float(np.median(b))
        print(f"{pset:10}points_kernel / sdf_kernel medians: {mb / ma:6.4f}  ({(mb / ma - 1) * 100:+5.2f} %; "
              f"sdf_kernel's own spread {(max(a) - min(a)) / ma * 100:4.2f} %)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--profile", metavar="PLAN.json")
    ap.add_argument("--summarise", nargs=2, metavar=("PLAN.json", "kernel_trace.csv"))
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--lds-pad", default="0", help="comma-separated pads in bytes")
    ap.add_argument("--sets", default="brick,shuffled,surface")
    a = ap.parse_args()
    if a.summarise:
        return summarise(*a.summarise)

    import torch

    import rtamd
    import scenes as S

    if rtamd.device_count() < 1:
        sys.exit("points_time.py: no HIP device visible")
    print(f"librtamd {rtamd.lib().rt_build_id().decode()} on {torch.cuda.get_device_name(0)}", flush=True)
    _, (v, i), _ = S.inputs(MESH)
    sets = {k: x for k, x in point_sets(v, i).items() if k in a.sets.split(",")}
    pads = [int(x) for x in a.lds_pad.split(",")]
    dev = torch.device("cuda")
    plan = []
    with rtamd.SDFMesh(rtamd.SimpleMesh(v, i)) as m:
        for pset, host in sets.items():
            n = len(host)
            pts = torch.from_numpy(host).to(dev)
            out = {"dist": torch.empty(n, dtype=torch.float32, device=dev),
                   "closest": torch.empty((n, 3), dtype=torch.float32, device=dev),
                   "prim": torch.empty(n, dtype=torch.int64, device=dev),
                   "feature": torch.empty(n, dtype=torch.int32, device=dev)}
            q = {k + "_ptr": x.data_ptr() for k, x in out.items()}
            st = torch.cuda.current_stream().cuda_stream
            calls = {
                "dist": lambda: m.points_device(pts.data_ptr(), n, dist_ptr=q["dist_ptr"], stream=st),
                "all four": lambda: m.points_device(pts.data_ptr(), n, stream=st, **q),
                "unsigned": lambda: m.points_device(pts.data_ptr(), n, dist_ptr=q["dist_ptr"], unsigned=True, stream=st),
                "radius 0.05": lambda: m.points_device(pts.data_ptr(), n, dist_ptr=q["dist_ptr"], radius=0.05, stream=st),
            }
            torch.cuda.synchronize()
            if a.profile:
                for _ in range(REPS):
                    m.points(host)
                    plan.append({"set": pset, "n": n, "kernel": "sdf_kernel"})
                    calls["dist"]()
                    plan.append({"set": pset, "n": n, "kernel": "points_kernel"})
                    torch.cuda.synchronize()
                continue
            for pad in pads:
                rtamd._lib.check(rtamd.lib().rtx_set_points_lds_pad(pad))
                for _ in range(a.warmup):
                    for mode in MODES:
                        calls[mode]()
                torch.cuda.synchronize()
                ev = {mode: [] for mode in MODES}
                for _ in range(REPS):
                    for mode in MODES:
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record()
                        calls[mode]()
                        e1.record()
                        ev[mode].append((e0, e1))
                torch.cuda.synchronize()
                within = float((out["dist"].abs() <= 0.05).float().mean())  # (the last launch was radius 0.05)
                print(f"{pset}: {n} points, {within * 100:.1f} % within 0.05 of the surface, "
                      f"LDS per workgroup {rtamd.lib().rtx_sdf_mesh_lds_bytes(m._h) + pad} bytes (pad {pad})")
                for mode in MODES:
                    ms = [e0.elapsed_time(e1) for e0, e1 in ev[mode]]
                    med = float(np.median(ms))
                    print(f"  {mode:12} " + " ".join(f"{x * 1e3:9.1f}" for x in ms) +
                          f"  median {med * 1e3:9.1f} us  {n / med / 1e3:8.1f} Mpoints/s", flush=True)
            rtamd.lib().rtx_set_points_lds_pad(0)
    if a.profile:
        with open(a.profile, "w") as f:
            json.dump(plan, f)
        print(f"{len(plan)} launches planned -> {a.profile}")


if __name__ == "__main__":
    main()
