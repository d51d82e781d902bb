"""Registers, scratch and waves per SIMD of the three wide LocalBA kernels, as the compiler reports them for the Makefile's flags
(-Rpass-analysis=kernel-resource-usage, device code only; no device needed, about a minute).  k_lin<true> and k_points_walk sit at the
register limit of three waves per SIMD: lin_points_walk forms the addresses of its last stores behind an empty asm statement, and k_lin does
not request a landmark's first loads ahead of the LDS staging, because either costs scratch there.  Both depend on the register
allocator: run this after a change of the compiler or of these kernels.  Exits 1 when a figure is worse than LIMITS.
    python tools/lba_kernel_resources.py"""
import os
import re
import subprocess
import sys
import tempfile

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "active-orb-slam2_amd", "csrc")
# kernel -> (VGPRs at most, scratch bytes per lane at most, waves per SIMD at least)
LIMITS = {"k_points_walk": (168, 0, 3), "k_lin<true>": (168, 0, 3), "k_schur": (168, 36, 3)}
MANGLED = {"k_points_walk": "_ZN4aos213k_points_walkE", "k_lin<true>": "_ZN4aos25k_linILb1EE", "k_schur": "_ZN4aos27k_schurE"}


def makefile_flags():
    text = open(os.path.join(CSRC, "Makefile")).read()
    flags = re.search(r"^FLAGS\s*=\s*(.*)$", text, re.M).group(1).replace("$(ARCH)", re.search(r"^ARCH\s*\?=\s*(\S+)", text, re.M).group(1))
    return re.search(r"^HIPCC\s*\?=\s*(\S+)", text, re.M).group(1), flags.split()


def main():
    hipcc, flags = makefile_flags()
    with tempfile.TemporaryDirectory() as tmp:
        p = subprocess.run([os.environ.get("HIPCC", hipcc)] + flags + ["--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-c", "lba.hip",
                            "-o", os.path.join(tmp, "lba.o")], cwd=CSRC, stderr=subprocess.PIPE, text=True)
    if p.returncode:
        sys.exit(p.stderr)
    got, cur = {}, None
    for line in p.stderr.splitlines():
        m = re.search(r"remark: \s*(Function Name|VGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]): (\S+)", line)
        if not m:
            continue
        if m.group(1) == "Function Name":
            cur = next((k for k, v in MANGLED.items() if m.group(2).startswith(v)), None)
        elif cur:
            got.setdefault(cur, {})[m.group(1).split()[0]] = int(m.group(2))
    bad = 0
    for k, (vgpr, scratch, waves) in LIMITS.items():
        g = got.get(k)
        ok = g is not None and g["VGPRs"] <= vgpr and g["ScratchSize"] <= scratch and g["Occupancy"] >= waves
        bad += not ok
        print("%-14s %s   (limits: %d VGPRs, %d B of scratch, %d waves per SIMD)%s" % (k, g, vgpr, scratch, waves, "" if ok else "   <-- WORSE"))
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
