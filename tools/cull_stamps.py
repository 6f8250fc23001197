"""What the work-queue items outside the tile cull's rectangle still cost in a
persistent launch (dev tool; decided whether the queue's item grid is shrunk,
profiles/r08/README.md).

Host part (no GPU): the share of 8x8 tiles inside the rectangle for each frame
of the 64-frame orbit (rtx_cull_rect on the model's bounds).
GPU part, with the stamps build: one launch of `group` orbit frames and one of
`group` frames whose cameras look away from the model (every item is culled:
claim, the frame's scalar loads, the cleared stores), each with per-wave
stamps. The all-culled launch gives the wave time of a culled item; times the
orbit launch's items outside the rectangle, over that launch's wave time, it
is the share those items take.
  bash tools/build_variant.sh stamps -DRT_PERSIST_STAMPS
  RTAMD_LIB=.../lib/var_stamps.so python tools/cull_stamps.py [group] [--host-only] [--flags clear|hits_only]

--flags hits_only renders RT_FLAG_CLEAR | RT_FLAG_HITS_ONLY into frames cleared
beforehand, so a culled tile and a missed pixel store nothing: the all-culled
launch is then the pure claim cost of its items, and the difference to
--flags clear (the default) is what the background's stores cost
(profiles/r09/README.md).

The launches run on the whole frame's item grid (rtx_set_queue_grid(0)): the
tool measures what the items outside the rectangle cost, and with the item
rectangle on the all-culled launch has no items at all.
"""
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "triangles-sdf-cpu-raytracing_amd"))

import numpy as np  # noqa: E402

import rtamd  # noqa: E402
from rtamd import data  # noqa: E402
from rtamd import workloads as WL  # noqa: E402

W, H = 1920, 1080
CAP = 1 << 14


def tile_shares(L, mesh):
    p = (mesh.vPos4f[:, :3] / mesh.vPos4f[:, 3:4]).astype(np.float32)
    box = np.concatenate([p.min(0), p.max(0)]).astype(np.float32)
    total = ((W + 7) // 8) * ((H + 7) // 8)
    out = []
    for pos in WL.orbit_positions(64):
        P = WL.params_for(pos, W, H)
        r = np.zeros(4, np.int32)
        ok = L.rtx_cull_rect(C.byref(P), W, H, box.ctypes.data, r.ctypes.data)
        out.append((int(r[1] - r[0]) * int(r[3] - r[2]) / total) if ok else 1.0)
    return np.array(out)


def main():
    argv = sys.argv[1:]
    mode = "clear"
    if "--flags" in argv:
        i = argv.index("--flags")
        mode = argv[i + 1]
        del argv[i:i + 2]
        if mode not in ("clear", "hits_only"):
            sys.exit("--flags clear|hits_only")
    args = [a for a in argv if not a.startswith("--")]
    group = int(args[0]) if args else 10
    L = rtamd.lib()
    mesh = rtamd.load_mesh_from_obj(data.path("stanford-bunny.obj"), scale=True)
    sh = tile_shares(L, mesh)
    print(f"tiles inside the rectangle, 64-frame orbit at {W}x{H}: min {sh.min():.3f} mean {sh.mean():.3f} max {sh.max():.3f}"
          f" -> culled {1 - sh.max():.3f} .. {1 - sh.min():.3f}, mean {1 - sh.mean():.3f}")
    if "--host-only" in sys.argv:
        return
    import torch
    L.rtx_set_persist_stamps.argtypes = [C.c_void_p, C.c_int64]
    if hasattr(L, "rtx_set_queue_grid"):  # (a library from before the item rectangle has no such switch)
        rtamd._lib.check(L.rtx_set_queue_grid(0))
    L.rt_set_device(0)
    sc = rtamd.BVHBuilder(mesh)
    sc.set_plane(None)
    orbit = WL.orbit_positions(64)
    near = [WL.params_for(p, W, H) for p in orbit[:group]]
    away = []
    for p in orbit[:group]:  # the same positions, looking the other way
        vi, pi = rtamd.camera_matrices(p, tuple(2.0 * x for x in p), (0.0, 1.0, 0.0), 45.0, W / H, 0.01, 100.0)
        away.append(rtamd.render_params(p, vi, pi, (2.0, 2.0, 2.0), rtamd.ShadingMode.Normal, True, True))
    dev = torch.device("cuda")
    fb = [(torch.empty((H, W), dtype=torch.int32, device=dev), torch.empty((H, W), dtype=torch.float32, device=dev))
          for _ in range(group)]
    st = torch.cuda.current_stream().cuda_stream
    flags = rtamd.RT_FLAG_CLEAR | (rtamd._lib.RT_FLAG_HITS_ONLY if mode == "hits_only" else 0)
    print(f"flags: {mode}")

    def launch(prm, stamps):
        if mode == "hits_only":  # the cleared frame the flag asks for
            for c, t in fb:
                c.zero_()
                t.fill_(float("inf"))
            torch.cuda.synchronize()
        rtamd._lib.check(L.rtx_set_persist_stamps(C.c_void_p(stamps.data_ptr()) if stamps is not None else None,
                                                   CAP if stamps is not None else 0))
        sc.render_device_frames(prm, [c.data_ptr() for c, _ in fb], [t.data_ptr() for _, t in fb], W, H,
                                flags, stream=st)
        torch.cuda.synchronize()

    for prm in (near, away, near, away):  # warm
        launch(prm, None)
    res = {}
    for rep in range(3):
        for name, prm in (("orbit", near), ("away", away)):
            sb = torch.zeros(CAP * 8, dtype=torch.int64, device=dev)
            launch(prm, sb)
            s = sb.view(-1, 8).cpu().numpy()
            s = s[s[:, 1] > 0]
            wave_us = (s[:, 1] - s[:, 0]).sum() / 100.0
            items = int((s[:, 2] & 0xFFFFFFFF).sum())
            span = (s[:, 1].max() - s[:, 0].min()) / 100.0
            res[name] = (wave_us, items, span, len(s))
            print(f"rep {rep} {name}: {len(s)} waves, {items} items, span {span:.1f} us, wave time {wave_us:.0f} us"
                  f" ({wave_us / items * 1e3:.1f} ns per item; {items / span:.1f} claims per us)")
        (wo, io, so, _), (wa, ia, sa, _) = res["orbit"], res["away"]
        out_items = io * (1.0 - sh[:group].mean())
        print(f"rep {rep}: items outside the rectangle ~{out_items:.0f} of {io}: {out_items * wa / ia:.0f} us of the orbit"
              f" launch's {wo:.0f} us wave time = {out_items * wa / ia / wo:.3f}; the all-culled launch's span is"
              f" {sa / so:.3f} of the orbit launch's")
    rtamd._lib.check(L.rtx_set_persist_stamps(None, 0))
    sc.close()


if __name__ == "__main__":
    main()
