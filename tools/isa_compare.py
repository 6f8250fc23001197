#!/usr/bin/env python3
"""Compare two `make isa` outputs kernel by kernel (dev tool; the check that a
refactor left the compiled kernels alone, profiles/r11/README.md).

usage: python tools/isa_compare.py PARENT_BUILD_DIR NEW_BUILD_DIR [unit ...]
(units default to rt_device rt_diag rt_bvhgpu rt_sdfgen)

Kernels are matched in listing order, since a renamed template argument
renames them. Mangled symbols become K<n> by first appearance and local
labels L, then per kernel: the resource-usage remarks of both builds, the
differing instruction lines, the differing lines once register numbers are
masked as well (what is left is a different instruction or a different order,
not a different register), and whether both builds issue the same multiset of
mnemonics (the _e32 / _e64 encodings of one instruction counted together).
Two histograms by mnemonic follow: of the exact and of the register-masked
differing lines (parent's plus new's).
"""
import collections
import os
import re
import subprocess
import sys
import tempfile

FIELDS = [("VGPRs", "VGPRs"), ("AGPRs", "AGPRs"), ("ScratchSize [bytes/lane]", "scratch"),
          ("Occupancy [waves/SIMD]", "occupancy"), ("LDS Size [bytes/block]", "LDS"),
          ("SGPRs Spill", "SGPR spills"), ("VGPRs Spill", "VGPR spills")]


def resources(path):
    out, cur = [], None
    for line in open(path, errors="replace"):
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            cur = (m.group(1), {})
            out.append(cur)
            continue
        m = re.search(r"remark:\s+([A-Za-z][A-Za-z \[\]/]*): (\d+)", line)
        if m and cur:
            cur[1][m.group(1).strip()] = int(m.group(2))
    return out


def kernels(path):
    """[(symbol, [normalised lines])] in listing order; the last entry also holds the metadata"""
    idx = {}

    def sub(m):
        return "K%d" % idx.setdefault(m.group(0), len(idx))

    ks, cur = [], None
    for ln in open(path, errors="replace"):
        ln = ln.rstrip("\n")
        m = re.match(r"([A-Za-z_]\S*):\s+; @", ln)
        if m:
            cur = []
            ks.append((m.group(1), cur))
        if cur is not None:
            ln = re.sub(r"_Z[A-Za-z0-9_.$]+|__hip_cuid_[0-9a-f]+", sub, ln)
            cur.append(re.sub(r"\.L[A-Za-z_]*\d+(_\d+)?", "L", ln))
    return ks


def is_code(ln):
    s = ln.strip()
    return bool(s) and s[0] not in ";." and not s.endswith(":")


def is_meta(ln):
    return re.match(r"\s*(\.offset:|\.size:|\.kernarg_segment_size:|\.amdhsa_kernarg_size)", ln) is not None


def mask(ln):
    ln = re.sub(r"\b([vsa])\[\d+:\d+\]", r"\1R", ln)
    ln = re.sub(r"\b([vsa])\d+\b", r"\1R", ln)
    return re.sub(r"\bvcc(_lo|_hi)?\b", "sR", ln)


def diff(a, b):
    names = []
    for lines in (a, b):
        with tempfile.NamedTemporaryFile("w", delete=False) as f:
            f.write("\n".join(lines) + "\n")
            names.append(f.name)
    out = subprocess.run(["diff"] + names, capture_output=True, text=True).stdout
    for n in names:
        os.unlink(n)
    return [ln[2:] for ln in out.split("\n") if ln[:2] in ("< ", "> ")]


def mnemonic(ln):
    return ln.split()[0]


def base(ln):
    """mnemonic without its encoding suffix (v_cmp_gt_f32_e32 and _e64 are one instruction)"""
    return re.sub(r"_e(32|64)$", "", mnemonic(ln))


def short(sym):
    d = subprocess.run(["c++filt", sym], capture_output=True, text=True).stdout.strip()
    d = d.replace("(anonymous namespace)::", "").replace("void ", "")
    return d[:d.index(">(") + 1] if ">(" in d else d.split("(")[0]


def main():
    a, b = sys.argv[1], sys.argv[2]
    units = sys.argv[3:] or ["rt_device", "rt_diag", "rt_bvhgpu", "rt_sdfgen"]
    exact, masked = collections.Counter(), collections.Counter()
    print("kernel | parent: VGPRs scratch occupancy LDS | new: the same | other resource fields | "
          "differing lines | register-masked | same mnemonics | metadata lines")
    for u in units:
        ra, rb = resources(f"{a}/{u}.resource_usage.txt"), resources(f"{b}/{u}.resource_usage.txt")
        ka, kb = kernels(f"{a}/{u}.s"), kernels(f"{b}/{u}.s")
        if not len(ka) == len(kb) == len(ra) == len(rb):
            sys.exit(f"{u}: kernel counts differ: {len(ka)} {len(kb)} listings, {len(ra)} {len(rb)} remarks")
        print(f"-- {u}: {len(ka)} kernels")
        for (_, la), (nb, lb), (_, fa), (_, fb) in zip(ka, kb, ra, rb):
            ca, cb = [l for l in la if is_code(l)], [l for l in lb if is_code(l)]
            de = diff(ca, cb)
            dm = diff([mask(l) for l in ca], [mask(l) for l in cb]) if de else []
            meta = diff([l for l in la if is_meta(l)], [l for l in lb if is_meta(l)])
            exact.update(mnemonic(l) for l in de)
            masked.update(mnemonic(l) for l in dm)
            same = collections.Counter(map(base, ca)) == collections.Counter(map(base, cb))

            def row(f):
                return " ".join(str(f[k]) for k in ("VGPRs", "ScratchSize [bytes/lane]", "Occupancy [waves/SIMD]",
                                                    "LDS Size [bytes/block]"))
            other = ", ".join(f"{s} {fa[k]} -> {fb[k]}" for k, s in FIELDS if fa.get(k) != fb.get(k)) or "same"
            print(f"{short(nb)} | {row(fa)} | {row(fb)} | {other} | {len(de)} | {len(dm)} | "
                  f"{'yes' if same else 'no'} | {len(meta)}")
    for title, h in (("differing instruction lines", exact), ("register-masked differing lines", masked)):
        print(f"\n{title} by mnemonic (parent's + new's):")
        for k, v in sorted(h.items(), key=lambda kv: (-kv[1], kv[0])):
            print(f"  {v:6d} {k}")


if __name__ == "__main__":
    main()
