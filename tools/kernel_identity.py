#!/usr/bin/env python3
"""Development aid: one line per gfx950 kernel of the given .hip files, to show that a move of code left the kernels alone.
  python tools/kernel_identity.py tiler_amd/csrc/tm_kmeans*.hip tiler_amd/csrc/tm_palettize.hip > after.txt
Columns: mangled name, next_free_vgpr, next_free_sgpr, static LDS bytes, scratch bytes, and a hash of the instruction stream
between the kernel's label and its .Lfunc_end with comments dropped and the numbers of local labels removed.  Kernels outside
namespace tmx (rocPRIM's) are listed by name only.  Compiles with the flags of tiler_amd/csrc/build.sh; extra flags via TM_EXTRA_FLAGS."""
import hashlib, os, re, subprocess, sys

FLAGS = "--offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off -fno-fast-math -fvisibility=hidden -Wall -Wno-unused-function"
FIELDS = ("next_free_vgpr", "next_free_sgpr", "group_segment_fixed_size", "private_segment_fixed_size")


def kernels(src):
    cmd = [os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")] + FLAGS.split() + os.environ.get("TM_EXTRA_FLAGS", "").split()
    asm = subprocess.run(cmd + ["--cuda-device-only", "-S", src, "-o", "-"], check=True, capture_output=True, text=True).stdout
    lines = [re.sub(r"\.(LBB|Ltmp|LJTI|Lfunc_begin)[0-9_]+", r".\1", l.split(";")[0].rstrip()) for l in asm.split("\n")]
    for m in re.finditer(r"^\t\.amdhsa_kernel (\S+)\n(.*?)^\t\.end_amdhsa_kernel", asm, re.S | re.M):
        name = m.group(1)
        if not name.startswith("_ZN3tmx"):
            yield name, None
            continue
        desc = dict(re.findall(r"\.amdhsa_(\w+) (\d+)", m.group(2)))
        begin = lines.index(name + ":")
        end = next(i for i in range(begin, len(lines)) if lines[i].startswith(".Lfunc_end"))
        # (the kernel's own name, which its descriptor and section lines repeat, stays out of the hash: a parameter type that moves to
        # another namespace renames the kernel and nothing else)
        body = "\n".join(l.replace(name, "<kernel>") for l in lines[begin + 1:end] if l.strip())
        yield name, [desc[f] for f in FIELDS] + [str(body.count("\n") + 1), hashlib.sha256(body.encode()).hexdigest()[:16]]


rows = sorted(k for src in sys.argv[1:] for k in kernels(src))
for name, figures in rows:
    print(name if figures is None else name + " " + " ".join(figures))
