#!/usr/bin/env python3
"""Compare two `make isa` outputs kernel by kernel (dev tool; the check that a
refactor left the compiled kernels alone, profiles/r11/README.md).

usage: python tools/isa_compare.py PARENT_BUILD_DIR NEW_BUILD_DIR [unit ...]
(units default to every *.s present in each directory)

Kernels are matched by demangled name (template arguments included, the
parameter list and the anonymous namespace left out) across all units of both
builds, so a kernel may move from one unit to another between the builds; a
kernel that only one build has is reported and the exit status is 1. Within a
kernel, mangled symbols become K<n> by first appearance and local labels L,
then per kernel: the resource-usage remarks of both builds, the differing
instruction lines, the differing lines once register numbers are masked as
well (what is left is a different instruction or a different order, not a
different register), whether both builds issue the same multiset of mnemonics
(the _e32 / _e64 encodings of one instruction counted together), and the
differing lines of the kernel-argument metadata (offsets, sizes and kinds of
the arguments, the segment size). Two histograms by mnemonic follow: of the
exact and of the register-masked differing lines (parent's plus new's).
"""
import collections
import glob
import os
import re
import subprocess
import sys
import tempfile

FIELDS = [("VGPRs", "VGPRs"), ("AGPRs", "AGPRs"), ("ScratchSize [bytes/lane]", "scratch"),
          ("Occupancy [waves/SIMD]", "occupancy"), ("LDS Size [bytes/block]", "LDS"),
          ("SGPRs Spill", "SGPR spills"), ("VGPRs Spill", "VGPR spills")]
SYMBOL = r"_Z[A-Za-z0-9_.$]+|__hip_cuid_[0-9a-f]+"


def resources(path):
    """{symbol: {field: value}} of one unit's resource-usage remarks"""
    out, cur = {}, None
    for line in open(path, errors="replace"):
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            cur = out.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark:\s+([A-Za-z][A-Za-z \[\]/]*): (\d+)", line)
        if m and cur is not None:
            cur[m.group(1).strip()] = int(m.group(2))
    return out


def normalise(lines):
    idx = {}

    def sub(m):
        return "K%d" % idx.setdefault(m.group(0), len(idx))

    # (block labels carry the function's index in its unit, in comments too: "Header=BB4_16")
    return [re.sub(r"\.L[A-Za-z_]*\d+(_\d+)?|\bBB\d+_\d+", "L", re.sub(SYMBOL, sub, ln)) for ln in lines]


def kernels(path):
    """{symbol: (code and directive lines, metadata lines)} of one unit's listing, both normalised"""
    code, meta, cur, entry = {}, {}, None, None
    for ln in open(path, errors="replace"):
        ln = ln.rstrip("\n")
        if ln.startswith("amdhsa.kernels:"):
            cur, entry = None, []
            continue
        if entry is not None:  # the metadata's kernel list: one entry per "  - ." line
            if re.match(r"  - \.", ln):
                entry = []
            elif not ln.startswith("    "):
                if ln.strip() and not ln.startswith("  "):
                    entry = None
                continue
            entry.append(ln)
            m = re.match(r"\s+\.name:\s+(\S+)", ln)
            if m:
                meta[m.group(1)] = entry
            continue
        m = re.match(r"([A-Za-z_]\S*):\s+; @", ln)
        if m:
            cur = code.setdefault(m.group(1), [])
        elif re.match(r"\s*\.amdgpu_metadata", ln):  # the unit's last kernel ends here
            cur = None
        if cur is not None:
            cur.append(ln)
    return {k: (normalise(v), normalise(meta.get(k, []))) for k, v in code.items()}


def is_code(ln):
    s = ln.split(";")[0].strip()  # (a label line may end in a comment)
    return bool(s) and s[0] != "." and not s.endswith(":")


def is_meta(ln):
    return re.match(r"\s*(-\s+)?(\.offset:|\.size:|\.value_kind:|\.kernarg_segment_size:|\.amdhsa_kernarg_size)",
                    ln) is not None


def mask(ln):
    ln = re.sub(r"\b([vsa])\[\d+:\d+\]", r"\1R", ln)
    ln = re.sub(r"\b([vsa])\d+\b", r"\1R", ln)
    return re.sub(r"\bvcc(_lo|_hi)?\b", "sR", ln)


def diff(a, b):
    if a == b:
        return []
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


def short_names(syms):
    """{symbol: demangled name without the parameter list}, one c++filt run for all"""
    syms = list(syms)
    out = subprocess.run(["c++filt"], input="\n".join(syms) + "\n", capture_output=True, text=True).stdout.split("\n")
    names = {}
    for s, d in zip(syms, out):
        d = d.strip().replace("(anonymous namespace)::", "").replace("void ", "")
        names[s] = d[:d.index(">(") + 1] if ">(" in d else d.split("(")[0]
    return names


def load(build, units):
    """{demangled name: (unit, symbol, code, metadata, resources)} over the units of one build"""
    present = sorted(os.path.basename(p)[:-2] for p in glob.glob(f"{build}/*.s"))
    units = [u for u in units if u in present] or present if units else present  # (a unit may exist in one build only)
    found = []
    for u in units:
        res = resources(f"{build}/{u}.resource_usage.txt")
        for sym, (code, meta) in kernels(f"{build}/{u}.s").items():
            found.append((u, sym, code, meta, res.get(sym, {})))
    names = short_names(f[1] for f in found)
    out = {}
    for f in found:
        n, k = names[f[1]], 1
        while (n if k == 1 else f"{n} #{k}") in out:  # overloads: numbered in listing order
            k += 1
        out[n if k == 1 else f"{n} #{k}"] = f
    return units, out


def main():
    a, b = sys.argv[1], sys.argv[2]
    ua, ka = load(a, sys.argv[3:])
    ub, kb = load(b, sys.argv[3:])
    exact, masked = collections.Counter(), collections.Counter()
    print(f"parent: {len(ka)} kernels in {' '.join(ua)}")
    print(f"new:    {len(kb)} kernels in {' '.join(ub)}")
    print("kernel | parent unit -> new unit | parent: VGPRs scratch occupancy LDS | new: the same | "
          "other resource fields | differing lines | register-masked | same mnemonics | metadata lines")
    changed = 0
    for name in sorted(set(ka) & set(kb)):
        (xa, _, la, ma, fa), (xb, _, lb, mb, fb) = ka[name], kb[name]
        ca, cb = [l for l in la if is_code(l)], [l for l in lb if is_code(l)]
        de = diff(ca, cb)
        dm = diff([mask(l) for l in ca], [mask(l) for l in cb]) if de else []
        meta = diff([l for l in la + ma if is_meta(l)], [l for l in lb + mb if is_meta(l)])
        exact.update(mnemonic(l) for l in de)
        masked.update(mnemonic(l) for l in dm)
        same = collections.Counter(map(base, ca)) == collections.Counter(map(base, cb))

        def row(f):
            return " ".join(str(f.get(k, "?")) for k in ("VGPRs", "ScratchSize [bytes/lane]", "Occupancy [waves/SIMD]",
                                                         "LDS Size [bytes/block]"))
        other = ", ".join(f"{s} {fa.get(k)} -> {fb.get(k)}" for k, s in FIELDS if fa.get(k) != fb.get(k)) or "same"
        changed += bool(de or meta or other != "same" or not fa or not fb)
        print(f"{name} | {xa} -> {xb} | {row(fa)} | {row(fb)} | {other} | {len(de)} | {len(dm)} | "
              f"{'yes' if same else 'no'} | {len(meta)}")
    for title, h in (("differing instruction lines", exact), ("register-masked differing lines", masked)):
        print(f"\n{title} by mnemonic (parent's + new's):")
        for k, v in sorted(h.items(), key=lambda kv: (-kv[1], kv[0])):
            print(f"  {v:6d} {k}")
    lost, gained = sorted(set(ka) - set(kb)), sorted(set(kb) - set(ka))
    print(f"\n{len(set(ka) & set(kb))} kernels in both builds, {changed} of them with a difference; "
          f"{len(lost)} only in the parent, {len(gained)} only in the new build")
    for n in lost:
        print(f"  only in the parent ({ka[n][0]}): {n}")
    for n in gained:
        print(f"  only in the new build ({kb[n][0]}): {n}")
    if lost or gained:
        sys.exit(1)


if __name__ == "__main__":
    main()
