#!/usr/bin/env python3
"""Instruction classes of the trace kernel's bounce loop, by phase, weighted by the phases' measured time shares.

The PT_STAMPS=1 diagnostic build brackets the loop's phases with s_memtime (csrc/pt_kernels.hip: t0 loop top, t1 after regeneration,
t2 after shading, ta / tb around pass 1 of the closest-hit search that follows it, t3 after pass 2); tools/stamps.py measures the phases' shares of a
wave-bounce on the GPU.  This script compiles that build to assembly (no GPU needed), cuts the loop of pt_trace_kernel<true,1,3>
at the stamps, classifies every instruction between two stamps, and prints per class
    sum over phases of  (time share of the phase) x (class's share of the phase's VALU instructions)
i.e. an estimate of the class's share of the loop's VALU issue -- exact if a phase's instructions all ran equally often (inner loops
make it an estimate; the phases are cut so that each is dominated by one loop body).
usage: python tools/isa_histogram.py [regen%% pass1%% pass2%% shade%%]   (default: the shares of profiles/r04/stamps_r04.txt if present)

       python tools/isa_histogram.py --moves [--parent-src <a checkout's csrc>]
The MOVE CLASS of the bounce loop of the SHIPPED build (not the PT_STAMPS one): every v_mov*, v_readlane, v_writelane, v_readfirstlane and
v_accvgpr* of the loop with its phase, its cause and whether a default configs[2] render executes it, priced with
profiles/r01/ubench_issue.log -- with --parent-src the same for another checkout's sources, the two summaries side by side.  The build
carries line tables (-gline-tables-only: the instruction stream is the shipped one, which the listing's count lets one check); a basic
block's phase is the phase of the source lines most of its instructions come from.  This mode reads assembly for these instructions only."""
import os, re, struct, subprocess, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "oclpathtracer_amd", "csrc")
ASM = "/tmp/pt_kernels_stamps.s"
KERNEL = "_Z15pt_trace_kernelILb1ELi1ELi3EEv13PtTraceParams"

def build():
    cmd = ["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-fno-slp-vectorize",
           "-DPT_STAMPS=1", "--cuda-device-only", "-S", "-o", ASM, "pt_kernels.hip"]
    subprocess.run(cmd, cwd=SRC, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)

def classify(op, args):
    if op.startswith("v_pk_"): return "packed f32 (v_pk_*)"
    if op.endswith("_f64") or "_f64_" in op: return "binary64"
    if re.match(r"v_(rcp|rsq|sqrt|exp|log|sin|cos)_", op): return "transcendental (quarter rate)"
    if op.startswith("v_cvt_"): return "convert"
    if re.match(r"v_(cmp|cmpx)_", op) or op.startswith("v_cndmask") or op.startswith("v_addc_co") or op.startswith("v_subb"): return "compare / select / carry"
    if re.match(r"v_(min|max|med3)", op): return "min / max / med3"
    if re.match(r"v_(fma|fmac|fmaak|fmamk|mul|add|sub|mad|mac)_(f32|legacy_f32)", op) or op in ("v_subrev_f32",):
        scalar = bool(re.search(r"(?<![a-z0-9_])(s\d+|s\[\d+:\d+\]|vcc|0x[0-9a-f]+|-?\d+\.\d+|-?\d+(?![:\]]))", args.split(",", 1)[1] if "," in args else ""))
        return "FMA / MUL / ADD f32, an SGPR or constant operand" if scalar else "FMA / MUL / ADD f32, all VGPR"
    if re.match(r"v_(mov|readlane|readfirstlane|writelane|swap|permlane|accvgpr)", op): return "move / lane access"
    if op.startswith("v_"): return "integer / bit (RNG, indices, masks)"
    if op.startswith("ds_"): return "LDS"
    if re.match(r"(global|buffer|scratch|flat)_", op): return "vector memory"
    if op.startswith("s_load") or op.startswith("s_buffer_load") or op.startswith("s_memtime"): return "scalar memory"
    if op.startswith("s_"): return "SALU / branch / wait"
    return "other"

def main():
    build()
    t = open(ASM).read()
    a = t.index(KERNEL + ":"); b = t.index(".Lfunc_end", a)
    lines = t[a:b].split("\n")
    stamps = [i for i in range(len(lines)) if "s_memtime" in lines[i]]   # t0 t1 t2 ta tb t3, in program order (the kernel has no others)
    names = ["regeneration (t0-t1)", "shading (t1-t2)", "search set-up (t2-ta)", "pass 1 (ta-tb)", "pass 2 (tb-t3)"]
    if len(stamps) != 6:
        print("expected 6 stamps in the kernel, found %d at %r" % (len(stamps), stamps)); sys.exit(1)
    args = [float(x) for x in sys.argv[1:5]]
    if len(args) != 4:
        f = os.path.join(ROOT, "profiles", "r04", "stamps_r04.txt")
        m = re.search(r"shares: regen ([\d.]+) pass1 ([\d.]+) pass2 ([\d.]+) shade ([\d.]+)", open(f).read()) if os.path.exists(f) else None
        args = [float(x) for x in m.groups()] if m else [6.5, 29.5, 30.7, 33.3]
    regen, p1, p2, shade = args
    share = {names[0]: regen, names[1]: shade, names[2]: 0.0, names[3]: p1, names[4]: p2}   # (the set-up is inside the "loop" figure of stamps.py: counted with pass 2)
    hist, per_phase = {}, {}
    for k, name in enumerate(names):
        counts = {}
        for l in lines[stamps[k] + 1:stamps[k + 1]]:
            m = re.match(r"^\s+([a-z_0-9]+)\s*(.*?)(?:\s*;.*)?$", l)
            if not m or m.group(1).startswith("."): continue
            c = classify(m.group(1), m.group(2))
            counts[c] = counts.get(c, 0) + 1
        per_phase[name] = counts
    # the set-up's instructions run once per bounce like pass 2's head: fold them into pass 2
    for c, n in per_phase[names[2]].items(): per_phase[names[4]][c] = per_phase[names[4]].get(c, 0) + n
    valu = lambda c: not c in ("LDS", "vector memory", "scalar memory", "SALU / branch / wait", "other")
    print("static instructions of the bounce loop of %s (PT_STAMPS=1 build), by phase; shares of a wave-bounce: regeneration %.1f %%, pass 1 %.1f %%, pass 2 %.1f %%, shading %.1f %%"
          % ("pt_trace_kernel<true,1,3>", regen, p1, p2, shade))
    for name in (names[0], names[3], names[4], names[1]):
        counts = per_phase[name]
        nv = sum(n for c, n in counts.items() if valu(c))
        print("\n%s: %d instructions, %d of them VALU" % (name, sum(counts.values()), nv))
        for c, n in sorted(counts.items(), key=lambda x: -x[1]):
            print("   %-52s %4d  %s" % (c, n, "%5.1f %% of the phase's VALU" % (100.0 * n / nv) if valu(c) else ""))
            if valu(c): hist[c] = hist.get(c, 0.0) + share[name] * n / nv
    tot = sum(hist.values())
    print("\nestimated share of the loop's VALU issue by class (time share of the phase x the class's share of its VALU instructions):")
    for c, v in sorted(hist.items(), key=lambda x: -x[1]):
        print("   %-52s %5.1f %%" % (c, 100.0 * v / tot))

# ---- the move class of the shipped build's bounce loop (--moves) -------------------------------------------------------------------
# cycles per wave-instruction at 8 waves per SIMD (profiles/r01/ubench_issue.log): v_mov_b32 v,v 2.38 (a constant source is priced the
# same; a 64-bit move as two), v_mov_b32 v,s 4.38, a lane access 4.39
PRICE = {"constant": 2.38, "vgpr": 2.38, "sgpr": 4.38, "lane": 4.39}
PHASES = ("regeneration", "pass 1", "pass 2", "shading")
REGEN_FN = re.compile(r"pt_(queue_|pool_|path_|hit_|shade_miss|start_fresh|sample_begin|generate_ray|camera_|pixel_|stripe_row|ring_offset|carry_|mbcnt|hash)")
PASS1_FN = re.compile(r"pt_(quad3_pass1|pk_|push_flag|tri_pass1|load_tri)")
PASS2_FN = re.compile(r"pt_(pass2_|tri_pass2|tail_|tri_candidate|fetch_rec|from_lane|stage_tile|intersect_primary)")
SHADE_FN = re.compile(r"pt_shade(?!_miss)")   # (the miss part runs with the store, at the top of the iteration)

def source_phases(src):
    """line of pt_kernels.hip -> phase, from the function the line is in (and, inside the loop's own functions, from where in them)"""
    lines = open(os.path.join(src, "pt_kernels.hip")).read().split("\n")
    phase, fn, mark = {}, None, None
    for i, l in enumerate(lines, 1):
        m = re.match(r"^(?:PTK_DEV|void|__global__)[^;=]*?\b(pt_\w+)\s*\(", l)
        if m and not l.rstrip().endswith(";"): fn, mark = m.group(1), None
        if fn is None: continue
        if fn == "pt_intersect_two_pass":
            if "if (!alive) m = 0u" in l: mark = "pass 2"
            phase[i] = mark or "pass 1"
        elif fn == "pt_trace_body":
            if "PT_STAMP(t1)" in l: mark = "shading"
            if "PT_STAMP(t2)" in l: mark = "pass 2"       # (the search's call: its set-up and whatever is left of it there)
            phase[i] = mark or "regeneration"
        elif SHADE_FN.match(fn): phase[i] = "shading"
        elif PASS1_FN.match(fn): phase[i] = "pass 1"
        elif PASS2_FN.match(fn): phase[i] = "pass 2"
        elif REGEN_FN.match(fn): phase[i] = "regeneration"
    # the long form of the finished path's store (a ring above 4 GiB): never taken by a default render
    longform = set()
    for i, l in enumerate(lines, 1):
        if "const unsigned fr = s.fl + KR->ring_phase" in l: longform.update(range(i - 3, i + 4))
    return phase, longform

def const_name(s):
    if re.match(r"^0x[0-9a-f]+$", s):
        v = int(s, 16)
        return "%s (%.9g as binary32)" % (s, struct.unpack("<f", struct.pack("<I", v & 0xffffffff))[0])
    return s

def regs_of(operand):
    """the 32-bit VGPRs an operand names"""
    m = re.match(r"^[-|]*v(\d+)", operand)
    if m: return {int(m.group(1))}
    m = re.match(r"^[-|]*v\[(\d+):(\d+)\]", operand)
    return set(range(int(m.group(1)), int(m.group(2)) + 1)) if m else set()

def move_audit(src):
    asm = "/tmp/pt_kernels_moves_%d.s" % os.getpid()
    cmd = ["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-fno-slp-vectorize",
           "-gline-tables-only", "--cuda-device-only", "-S", "-o", asm, "pt_kernels.hip"]
    subprocess.run(cmd, cwd=src, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    t = open(asm).read(); os.remove(asm)
    a = t.index(KERNEL + ":"); b = t.index(".Lfunc_end", a)
    phase_of, longform = source_phases(src)
    # instructions with their block, the block's loop note and their source lines (the .loc chain, innermost first)
    ins, blocks, cur, loc = [], [], None, []
    for l in t[a:b].split("\n"):
        s = l.strip()
        m = re.match(r"^(\.LBB\d+_\d+:|; %bb\.\d+:)\s*(;.*)?$", s)
        if m:
            cur = {"name": m.group(1).rstrip(":"), "note": m.group(2) or "", "labelled": s.startswith(".L"), "ins": []}
            blocks.append(cur); continue
        if s.startswith(";") and cur is not None and not cur["ins"] and not s.startswith(";;"):
            cur["note"] += " " + s; continue
        if s.startswith(".loc"):
            c = s.split(";", 1)[1] if ";" in s else ""
            loc = [int(x) for x in re.findall(r"pt_kernels\.hip:(\d+)", c)]; continue
        m = re.match(r"^([a-z_0-9]+)\s*(.*?)(?:\s*;.*)?$", s)
        if not m or s.startswith(".") or s.startswith(";") or cur is None: continue
        d = {"op": m.group(1), "args": [x.strip() for x in m.group(2).split(",")] if m.group(2) else [], "loc": loc, "block": cur}
        cur["ins"].append(d); ins.append(d)
    n_total = len(ins)
    # the bounce loop: the depth-1 loop with the most blocks
    hdrs = {}
    for bl in blocks:
        for h in re.findall(r"(?:Header=|Parent Loop )(BB\d+_\d+)", bl["note"]): hdrs[h] = hdrs.get(h, 0) + 1
    loop = max(hdrs, key=hdrs.get)
    inloop = [bl for bl in blocks if loop in bl["note"] or bl["name"] == ".L" + loop]
    # phase and path of every block
    prev_phase, prev_off = "regeneration", None
    for bl in inloop:
        votes = {}
        for d in bl["ins"]:
            for ln in d["loc"]:
                if ln in phase_of: votes[phase_of[ln]] = votes.get(phase_of[ln], 0) + 1; break
        bl["phase"] = max(votes, key=votes.get) if votes else prev_phase
        ops = [d["op"] for d in bl["ins"]]
        off = None
        if any("_f64" in o for o in ops) and bl["phase"] == "shading": off = "binary64 sincos arm"
        elif any(o.startswith(("v_div_scale", "v_div_fmas", "v_div_fixup")) for o in ops): off = "generic division"
        elif any(ln in longform for d in bl["ins"] for ln in d["loc"][:1]) and sum(1 for d in bl["ins"] if d["loc"][:1] and d["loc"][0] in longform) * 2 > len(bl["ins"]): off = "long ring form"
        elif not bl["labelled"] and prev_off: off = prev_off          # reached only by falling out of a block that is not taken
        bl["off"] = off
        prev_phase, prev_off = bl["phase"], off
    # every instruction of the class, with its cause (a lane access with an immediate lane number is a spill or its reload)
    rows = []
    for bl in inloop:
        for k, d in enumerate(bl["ins"]):
            op, args = d["op"], d["args"]
            if not re.match(r"v_(mov_|readlane|writelane|readfirstlane|accvgpr)", op): continue
            if op.startswith("v_mov"):
                srcop = args[1]
                dst = regs_of(args[0])
                user = "?"
                for e in bl["ins"][k + 1:]:
                    if any(regs_of(x) & dst for x in e["args"][1:]) or (e["op"].startswith(("global_store", "ds_write", "v_cmp", "v_writelane")) and any(regs_of(x) & dst for x in e["args"])):
                        user = e["op"]; break
                    if regs_of(e["args"][0]) >= dst if e["args"] else False: user = "(redefined: " + e["op"] + ")"; break
                if user == "?": user = "a later block"
                if re.match(r"^[-|]*v", srcop):
                    definer = "live into the block"
                    for e in reversed(bl["ins"][:k]):
                        if e["args"] and regs_of(e["args"][0]) & regs_of(srcop): definer = "result of " + e["op"]; break
                    kind, cause = "vgpr", "phi / two-address copy of %s (%s) for %s" % (srcop, definer, user)
                elif re.match(r"^(s\d+|s\[|vcc|exec|m0)", srcop): kind, cause = "sgpr", "SGPR -> VGPR copy of %s for %s" % (srcop, user)
                else: kind, cause = "constant", "constant %s for %s" % (const_name(srcop), user)
                n = 2 if "b64" in op else 1
            else:
                n = 1; kind = "lane"
                lane = args[2] if len(args) > 2 else ""
                if op == "v_readfirstlane_b32": cause = "readfirstlane of %s (wave-uniform value from a VGPR)" % args[1]
                elif op.startswith("v_accvgpr"): cause = "AGPR move"
                elif re.match(r"^\d+$", lane): cause = ("spill of %s to lane %s of %s" % (args[1], lane, args[0])) if op.startswith("v_writelane") else ("reload of %s from lane %s of %s" % (args[0], lane, args[1]))
                else: cause = "lane access chosen at run time (%s): the algorithm's own, not a spill" % lane
            rows.append({"phase": bl["phase"], "off": bl["off"], "kind": kind, "n": n, "text": "%s %s" % (op, ", ".join(args)), "cause": cause,
                         "block": bl["name"], "src": "pt_kernels.hip:%d" % d["loc"][0] if d["loc"] else "-",
                         "spill": cause.startswith(("spill of", "reload of"))})
    return {"rows": rows, "n_total": n_total, "loop": loop, "n_loop": sum(len(bl["ins"]) for bl in inloop), "n_blocks": len(inloop)}

def summarise(A):
    S = {}
    for r in A["rows"]:
        cause = {"constant": "constant materialised", "sgpr": "SGPR -> VGPR copy", "vgpr": "phi / two-address copy"}.get(r["kind"]) or \
                ("SGPR spill / reload" if r["spill"] else "lane access (algorithm)")
        k = (r["phase"], cause, "default path" if not r["off"] else "not taken: " + r["off"])
        c = S.setdefault(k, [0, 0.0]); c[0] += 1; c[1] += r["n"] * PRICE[r["kind"]]
    return S

def moves_main(argv):
    here = move_audit(SRC)
    parent = move_audit(argv[argv.index("--parent-src") + 1]) if "--parent-src" in argv else None
    print("The move class of the bounce loop of pt_trace_kernel<true,1,3>, shipped build (tools/isa_histogram.py --moves; no GPU: static counts).")
    print("Prices per wave-instruction at 8 waves per SIMD (profiles/r01/ubench_issue.log): v_mov v,v or v,constant %.2f cycles (a 64-bit move as two),"
          % PRICE["vgpr"])
    print("v_mov v,s %.2f, v_readlane / v_writelane / v_readfirstlane %.2f.  An instruction inside an inner loop is counted once, as written." % (PRICE["sgpr"], PRICE["lane"]))
    sides = [("parent", parent), ("change", here)] if parent else [("this tree", here)]
    for name, A in sides:
        print("%s: kernel %d instructions, bounce loop (header %s) %d instructions in %d blocks, %d of the class" % (name, A["n_total"], A["loop"], A["n_loop"], A["n_blocks"], len(A["rows"])))
    S = [summarise(A) for _, A in sides]
    keys = sorted(set().union(*S), key=lambda k: (PHASES.index(k[0]), k[2] != "default path", k[1], k[2]))
    print("\n%-13s %-26s %-34s" % ("phase", "cause", "path") + "".join("  %8s %7s" % (n, "cycles") for n, _ in sides))
    tot = [[0, 0.0, 0, 0.0] for _ in sides]
    for k in keys:
        line = "%-13s %-26s %-34s" % k
        for j, s in enumerate(S):
            c = s.get(k, [0, 0.0]); line += "  %8d %7.1f" % (c[0], c[1])
            o = 0 if k[2] == "default path" else 2
            tot[j][o] += c[0]; tot[j][o + 1] += c[1]
        print(line)
    print("%-75s" % "total on the default path" + "".join("  %8d %7.1f" % (x[0], x[1]) for x in tot))
    print("%-75s" % "total behind branches a default render never takes" + "".join("  %8d %7.1f" % (x[2], x[3]) for x in tot))
    for j, (name, A) in enumerate(sides):
        sp = [r for r in A["rows"] if r["spill"]]
        print("%s: %d spill / reload lane accesses in the loop, %d of them on the default path" % (name, len(sp), sum(1 for r in sp if not r["off"])))
    for name, A in sides:
        print("\n---- %s: every instruction of the class, in program order ----" % name)
        print("%-12s %-24s %-11s %-16s %-46s %s" % ("phase", "path", "block", "source", "instruction", "cause"))
        for r in A["rows"]:
            print("%-12s %-24s %-11s %-16s %-46s %s" % (r["phase"], r["off"] or "default", r["block"], r["src"].replace("pt_kernels.hip", ""), r["text"][:46], r["cause"]))

if __name__ == "__main__":
    if "--moves" in sys.argv: moves_main(sys.argv)
    else: main()
