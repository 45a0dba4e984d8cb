#!/usr/bin/env python3
"""Register / scratch / occupancy / LDS table of the kernels of one HIP source of lisec_amd/csrc (no GPU needed).

    python tools/kernel_resources.py igemm.hip [--log FILE]

Compiles the file's device code for gfx950 with -Rpass-analysis=kernel-resource-usage into a temporary directory and prints one
line per kernel, sorted by demangled name.  --log FILE reads a saved compiler log (the remarks on stderr) instead of compiling.
igemm.hip takes about three minutes."""
import argparse, os, re, subprocess, sys, tempfile

CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "lisec_amd", "csrc")
FIELDS = [("VGPRs", "vgpr"), ("AGPRs", "agpr"), ("ScratchSize [bytes/lane]", "scratch"), ("VGPRs Spill", "vspill"),
          ("Occupancy [waves/SIMD]", "occ"), ("LDS Size [bytes/block]", "lds")]


def table(log):
    rows, cur = {}, None
    for m in re.finditer(r"remark:\s+(?:\S+:\d+:\d+:\s+)?(.+?): (\S+) \[-Rpass-analysis", log):
        if m.group(1) == "Function Name":
            cur = rows.setdefault(m.group(2), {})
        elif cur is not None:
            cur[m.group(1)] = m.group(2)
    names = subprocess.run(["c++filt"], input="\n".join(rows), capture_output=True, text=True).stdout.split("\n")
    clean = [re.sub(r"^void |lisec::\(anonymous namespace\)::|\(.*$", "", n) for n in names]
    return sorted((n, [int(r[k]) for k, _ in FIELDS]) for n, r in zip(clean, rows.values()))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("source", help="a .hip file of lisec_amd/csrc")
    ap.add_argument("--log", help="saved compiler output to read instead of compiling")
    a = ap.parse_args()
    if a.log:
        log = open(a.log).read()
    else:
        with tempfile.TemporaryDirectory() as tmp:
            cmd = [os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "-O3", "-std=c++17", "--offload-arch=gfx950", "--cuda-device-only",
                   "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(CSRC, a.source), "-o", os.path.join(tmp, "out.o")]
            log = subprocess.run(cmd, capture_output=True, text=True, check=True).stderr
    rows = table(log)
    width = max(len(n) for n, _ in rows)
    print(f"{'kernel':<{width}} " + " ".join(f"{h:>7}" for _, h in FIELDS))
    for n, v in rows:
        print(f"{n:<{width}} " + " ".join(f"{x:>7}" for x in v))


if __name__ == "__main__":
    sys.exit(main())
