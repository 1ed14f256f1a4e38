#!/usr/bin/env python3
"""Print VGPR / AGPR / spill / scratch / LDS / occupancy per kernel of one csrc file (hipcc -Rpass-analysis=kernel-resource-usage).
`scratch` (bytes per lane) can be non-zero with zero spills: a register array indexed at run time, or filled under a condition,
is placed in scratch memory.
    kernel_resources.py <file> [name pattern] [--build-flags]        (--build-flags last)
Default: build.py's common FLAGS for every file.  --build-flags adds the file's own entry of build.py's EXTRA_FLAGS (later flags win),
i.e. the code the shipped library holds; the flags used are printed first."""
import os, re, runpy, subprocess, sys
if len(sys.argv) < 2 or sys.argv[1].startswith("--") or (len(sys.argv) > 2 and "--build-flags" in sys.argv[1:-1]):
    sys.exit(__doc__)
build_flags = sys.argv[-1] == "--build-flags"
args = sys.argv[1:-1] if build_flags else sys.argv[1:]
src = args[0]
pat = args[1] if len(args) > 1 else ""
flags = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=fast", "-Xclang", "-target-feature", "-Xclang", "-packed-fp32-ops"]   # (the shipped build's code generation: build.py FLAGS)
if build_flags:
    build_py = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "multimodal-brain-pattern-identification_xai_amd", "build.py")
    flags += runpy.run_path(build_py)["EXTRA_FLAGS"].get(os.path.basename(src), [])
print("flags:", " ".join(flags))
out = subprocess.run(["/opt/rocm/bin/hipcc", *flags, "-c", src, "-o", "/tmp/_kr.o", "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True).stderr
cur = {}
for line in out.splitlines():
    m = re.search(r"remark: [^:]*:\d+:\d+: +(.*?)( \[-Rpass)", line) or re.search(r"remark: +(.*?)( \[-Rpass)", line)
    if not m: continue
    t = m.group(1).strip()
    if t.startswith("Function Name:"):
        cur = {"name": t.split(":", 1)[1].strip()}
    elif ":" in t:
        k, v = t.split(":", 1); cur[k.strip()] = v.strip()
        if k.strip().startswith("LDS Size"):
            if pat in cur["name"]:
                print(f"{cur['name'][:60]:60s} VGPR {cur.get('VGPRs','?'):>4s} AGPR {cur.get('AGPRs','?'):>4s} spill {cur.get('VGPR Spill', cur.get('VGPRs Spill','?')):>3s} scratch {cur.get('ScratchSize [bytes/lane]','?'):>4s} "
                      f"occ {cur.get('Occupancy [waves/SIMD]','?'):>2s} LDS {cur.get('LDS Size [bytes/block]','?')}")
