#!/usr/bin/env python3
"""Are the kernels of two builds the same instruction streams?  tools/kernel_streams.py A.s B.s

A.s and B.s are device assemblies of the same source file at two commits (hipcc with the Makefile's HIPFLAGS and --cuda-device-only -S,
no GPU).  Per kernel: the text between its label and its .Lfunc_end, without comments and directive lines and with the function's number
taken out of its .LBBn_ labels, hashed.  Kernels are grouped by template name -- a refactor may rename an instantiation, so the two
sides are compared as sorted lists of hashes per template, not name by name.  Text only: nothing is interpreted.  Exit status 1 when a
template's lists differ."""
import collections
import hashlib
import re
import sys


def template_name(mangled):
    m = re.match(r"_Z(\d+)", mangled)
    return mangled[m.end():m.end() + int(m.group(1))] if m else mangled


def streams(path):
    """{template name: sorted hashes of its kernels' normalised streams}"""
    lines = open(path).read().split("\n")
    kernels = {l.split()[1] for l in lines if l.lstrip().startswith(".amdhsa_kernel ")}
    out = collections.defaultdict(list)
    name, body = None, []
    for l in lines:
        l = l.split(";")[0].strip()
        if name is None:
            if l.endswith(":") and l[:-1] in kernels:
                name, body = l[:-1], []
        elif l.startswith(".Lfunc_end"):
            out[template_name(name)].append(hashlib.sha256("\n".join(body).encode()).hexdigest())
            name = None
        elif l and (not l.startswith(".") or l.endswith(":")):   # an instruction or a label; directives go
            body.append(re.sub(r"\.LBB\d+_", ".LBB_", l))
    return {t: sorted(h) for t, h in out.items()}


def main(a_path, b_path):
    a, b = streams(a_path), streams(b_path)
    differ = 0
    print("%-34s %5s %5s  %s" % ("template", "A", "B", "streams"))
    for t in sorted(set(a) | set(b)):
        ha, hb = a.get(t, []), b.get(t, [])
        same = ha == hb
        differ += not same
        moved = len(set(ha) ^ set(hb))
        print("%-34s %5d %5d  %s" % (t, len(ha), len(hb), "identical" if same else "DIFFER (%d hashes on one side only)" % moved))
    na, nb = sum(map(len, a.values())), sum(map(len, b.values()))
    print("%d kernels in A, %d in B; %s" % (na, nb, "every template's streams identical" if not differ else "%d templates differ" % differ))
    return 1 if differ else 0


if __name__ == "__main__":
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    sys.exit(main(sys.argv[1], sys.argv[2]))
