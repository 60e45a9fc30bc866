#!/usr/bin/env python3
"""Per-kernel resource table of one HIP source, from the compiler's own remarks (no GPU, nothing is run):

    python tools/kernel_resources.py cdlrm_amd/csrc/embbag_bwd.hip [--match AdaRow] [--out profiles/NAME.txt] [--title TEXT]

compiles the file with -Rpass-analysis=kernel-resource-usage for gfx950 and prints one line per kernel: VGPRs, AGPRs, SGPRs,
scratch bytes per lane, occupancy in waves per SIMD, static LDS bytes per workgroup.  Exit status 1 if a selected kernel uses
scratch."""
import argparse
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = [("VGPR", r"VGPRs: (\d+)"), ("AGPR", r"AGPRs: (\d+)"), ("SGPR", r"SGPRs: (\d+)"),
          ("scratch", r"ScratchSize \[bytes/lane\]: (\d+)"), ("occ", r"Occupancy \[waves/SIMD\]: (\d+)"),
          ("LDS", r"LDS Size \[bytes/block\]: (\d+)"), ("Sspill", r"SGPRs Spill: (\d+)"), ("Vspill", r"VGPRs Spill: (\d+)")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("source")
    ap.add_argument("--match", default="", help="only kernels whose demangled name contains this")
    ap.add_argument("--out")
    ap.add_argument("--title", default="")
    a = ap.parse_args()
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    cmd = [hipcc, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-fno-gpu-rdc", "--cuda-device-only",
           "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(ROOT, a.source), "-o", os.devnull]
    err = subprocess.run(cmd, stderr=subprocess.PIPE, stdout=subprocess.DEVNULL, text=True, check=True).stderr
    kernels, cur = {}, None
    for line in err.splitlines():
        m = re.search(r"remark: .*Function Name: (\S+)", line)
        if m:
            cur = kernels.setdefault(m.group(1), {})
            continue
        if cur is None:
            continue
        for key, pat in FIELDS:
            m = re.search(pat, line)
            if m:
                cur[key] = int(m.group(1))
    names = sorted(kernels)
    dem = subprocess.run(["c++filt"], input="\n".join(names), stdout=subprocess.PIPE, text=True).stdout.splitlines()
    rows = [(d.split("(")[0].replace("void ", ""), kernels[n]) for n, d in zip(names, dem) if a.match in d]
    w = max(len(r[0]) for r in rows)
    out = []
    if a.title:
        out += [a.title, ""]
    out += ["This is COMPILER OUTPUT, not a measurement:",
            "    hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage -c " + a.source,
            "scratch: bytes per lane; occ: waves per SIMD; LDS: static bytes per workgroup.  %d kernels." % len(rows), "",
            "kernel".ljust(w) + "".join(k.rjust(8) for k, _ in FIELDS)]
    for name, r in rows:
        out.append(name.ljust(w) + "".join(str(r.get(k, "?")).rjust(8) for k, _ in FIELDS))
    bad = [name for name, r in rows if r.get("scratch", 0) or r.get("Vspill", 0)]
    out += ["", "kernels with scratch: " + (", ".join(bad) if bad else "none")]
    text = "\n".join(out) + "\n"
    if a.out:
        with open(os.path.join(ROOT, a.out), "w") as f:
            f.write(text)
    sys.stdout.write(text)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
