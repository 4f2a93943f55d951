#!/bin/bash
# registers, spills, scratch and LDS of every kernel in csrc/pt_kernels.hip (from the code object's metadata); a lit kernel's mangled
# name ends in its kind as a number (pt_kernels.h: ptk_lit_kind), printed decoded in the last column
cd "$(dirname "$0")/../oclpathtracer_amd/csrc" || exit 1
/opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -fno-fast-math -fno-slp-vectorize --cuda-device-only -S -o /tmp/pt_kernels.s pt_kernels.hip "$@" 2>/dev/null || exit 1
python3 - <<'PY'
import re
t = open("/tmp/pt_kernels.s").read()
md = t[t.index(".amdgpu_metadata"):]
BITS = ("mis", "power", "rr", "list", "ris", "env", "rays")   # bits 1 .. 7 of a kind; bit 0 is indirect
def kind(name):   # the kind is the lit templates' last argument, an unsigned: ...Lj<kind>EE
    m = re.match(r"_Z\d+pt_(?:direct|indirect)_(?:rr_|bvh_)?kernelI.*?Lj(\d+)EE", name)
    if not m:
        return ""
    k = int(m.group(1))
    return "+".join(["indirect" if k & 1 else "direct"] + [b for i, b in enumerate(BITS) if k >> (i + 1) & 1])
print("%-78s %5s %5s %7s %7s %6s %8s  %s" % ("kernel", "VGPR", "SGPR", "v-spill", "s-spill", "LDS", "scratch", "kind"))
for blk in md.split("  - .agpr_count")[1:]:
    g = lambda k: re.search(r"\.%s:\s*(\S+)" % k, blk).group(1)
    print("%-78s %5s %5s %7s %7s %6s %8s  %s" % (g("name")[:78], g("vgpr_count"), g("sgpr_count"), g("vgpr_spill_count"), g("sgpr_spill_count"), g("group_segment_fixed_size"), g("private_segment_fixed_size"), kind(g("name"))))
PY
