#!/usr/bin/env python3
"""Registers, scratch, LDS and occupancy of the pass's kernels, read from the compiler: cross-compiles contrack_amd/csrc/ctk_api.hip for
gfx950 (device code only, nothing is linked or run, no GPU needed) with -Rpass-analysis=kernel-resource-usage and prints one line per
kernel instance whose demangled name matches a pattern.

    python tools/kernel_resources.py                      # k_overlap, k_rowcount
    python tools/kernel_resources.py -k 'k_label2d_lds' -o profiles/rNN_kernel_resources.txt

Workgroups per CU: the smallest of what VGPRs allow (512 per SIMD lane, granules of 8, at most 8 waves per SIMD), what LDS allows
(160 KB) and 2048 threads.  The compiler's own `Occupancy [waves/SIMD]` is printed next to it."""
import argparse
import os
import re
import shutil
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = (("sgpr", r"SGPRs:\s*(\d+)"), ("vgpr", r"\bVGPRs:\s*(\d+)"), ("agpr", r"AGPRs:\s*(\d+)"),
          ("scratch", r"ScratchSize \[bytes/lane\]:\s*(\d+)"), ("occ", r"Occupancy \[waves/SIMD\]:\s*(\d+)"),
          ("lds", r"LDS Size \[bytes/block\]:\s*(\d+)"))


def remarks(hipcc, arch, extra):
    src = os.path.join(ROOT, "contrack_amd", "csrc", "ctk_api.hip")
    cmd = [hipcc, "--offload-arch=" + arch, "--cuda-device-only", "-O3", "-std=c++17", "-ffp-contract=off",
           "-Rpass-analysis=kernel-resource-usage", "-c", src, "-o", os.devnull] + extra
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True)
    if r.returncode:
        sys.stderr.write(r.stderr)
        raise SystemExit("hipcc failed")
    return r.stderr


def demangle(names):
    filt = shutil.which("llvm-cxxfilt") or shutil.which("c++filt") or "/opt/rocm/llvm/bin/llvm-cxxfilt"
    try:
        out = subprocess.run([filt], input="\n".join(names) + "\n", stdout=subprocess.PIPE, universal_newlines=True, check=True).stdout
        return out.splitlines()
    except (OSError, subprocess.CalledProcessError):
        return list(names)


def threads_of(name):
    """the workgroup size an instance is launched with, where its template arguments tell (k_overlap<OVB, THREADS, ...>)"""
    m = re.match(r".*k_overlap<\d+, (\d+)", name)
    if m:
        return int(m.group(1))
    m = re.match(r".*k_label2d_lds<\d+, \d+, -?\d+, (\d+)", name)
    if m:
        return int(m.group(1))
    return 256


def per_cu(k, threads):
    waves = (threads + 63) // 64
    gran = (max(k["vgpr"] + k["agpr"], 1) + 7) // 8 * 8
    by_vgpr = min(8, 512 // gran) * 4 // waves
    by_lds = (160 * 1024) // max(k["lds"], 1)
    return max(0, min(by_vgpr, by_lds, 2048 // threads, 32))


def parse(text):
    out, cur = [], None
    for line in text.splitlines():
        m = re.search(r"Function Name:\s*(\S+)", line)
        if m:
            cur = {"mangled": m.group(1)}
            out.append(cur)
            continue
        if cur is None:
            continue
        for key, pat in FIELDS:
            m = re.search(pat, line)
            if m:
                cur[key] = int(m.group(1))
    return [k for k in out if all(f in k for f, _ in FIELDS)]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("-k", "--kernels", default=r"\bk_overlap<|\bk_rowcount", help="regular expression on the demangled name")
    ap.add_argument("-o", "--out", help="also write the table to this file")
    ap.add_argument("--hipcc", default=os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"))
    ap.add_argument("--arch", default="gfx950")
    ap.add_argument("extra", nargs="*", help="further compiler arguments (after --)")
    a = ap.parse_args()
    ks = parse(remarks(a.hipcc, a.arch, a.extra))
    for k, n in zip(ks, demangle([k["mangled"] for k in ks])):
        k["name"] = re.sub(r"\(.*$", "", re.sub(r"^void ", "", n))
    ks = sorted((k for k in ks if re.search(a.kernels, k["name"])), key=lambda k: k["name"])
    lines = ["# hipcc --offload-arch=%s -O3 -Rpass-analysis=kernel-resource-usage (cross-compiled; nothing was run)" % a.arch,
             "%-44s %5s %5s %8s %7s %9s %7s %6s" % ("kernel", "VGPRs", "SGPRs", "scratch", "LDS", "waves/SIMD", "threads", "WG/CU")]
    for k in ks:
        th = threads_of(k["name"])
        lines.append("%-44s %5d %5d %8d %7d %9d %7d %6d" % (k["name"], k["vgpr"] + k["agpr"], k["sgpr"], k["scratch"], k["lds"], k["occ"],
                                                          th, per_cu(k, th)))
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
