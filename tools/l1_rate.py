"""How fast a CU answers loads that always hit: its vector L1 against its LDS
(rtx_l1_rate, csrc/rt_diag.hip; dev tool behind profiles/r16/README.md).

  python tools/l1_rate.py [iters [blocks ...]]

Three cases, each at several numbers of 16-wave workgroups (256 CUs: 256
workgroups are 4 waves per SIMD, 512 are 8):
  same   global_load_dwordx4, all 64 lanes of a wave on the same 16 bytes
  own    global_load_dwordx4, every lane on its own 16 bytes of a 4 KiB set
  lds    14 ds_read_b128 of one address per round (the shared node fetch's reads)
Per case: load instructions per shader clock and CU, the bytes per clock that
is for the lanes, and 64-byte L1 accesses per clock at 16 per instruction (what
TCP_TOTAL_CACHE_ACCESSES counts for a 16-byte-per-lane load, bench.py's
calibration). The clock is each wave's own s_memtime over its loop; the waves
of a CU run together, so rate per CU = waves per CU x loads per wave / mean
cycles per wave.
"""
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "triangles-sdf-cpu-raytracing_amd"))

import numpy as np  # noqa: E402

import rtamd  # noqa: E402

CUS = 256
MODES = (("same", 0), ("own", 1), ("lds", 2))


def main():
    iters = int(sys.argv[1]) if len(sys.argv) > 1 else 2000
    blocks = [int(x) for x in sys.argv[2:]] or [256, 512]
    L = rtamd.lib()
    L.rt_set_device(0)
    L.rtx_l1_rate.restype = C.c_int
    L.rtx_l1_rate.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.c_void_p]
    print(f"{'case':6s}{'blocks':>8s}{'waves/CU':>10s}{'loads/wave':>12s}{'cycles/wave':>13s}{'max':>10s}"
          f"{'MHz':>7s}{'loads/clk/CU':>14s}{'B/clk/CU':>10s}{'64B acc/clk/CU':>16s}")
    for name, mode in MODES:
        for nb in blocks:
            out = np.zeros(5, np.uint64)
            rtamd._lib.check(L.rtx_l1_rate(mode, iters, nb, out.ctypes.data))  # warm: clocks up, set resident
            rtamd._lib.check(L.rtx_l1_rate(mode, iters, nb, out.ctypes.data))
            waves, loads, cyc, cmax, ticks = (float(x) for x in out)
            mean = cyc / waves
            per_cu = waves / CUS
            rate = per_cu * loads / mean
            mhz = 100.0 * cyc / ticks if ticks else 0.0
            acc = "" if mode == 2 else f"{16 * rate:16.3f}"
            print(f"{name:6s}{nb:8d}{per_cu:10.1f}{loads:12.0f}{mean:13.0f}{cmax:10.0f}{mhz:7.0f}"
                  f"{rate:14.4f}{rate * 1024:10.1f}{acc}", flush=True)


if __name__ == "__main__":
    main()
