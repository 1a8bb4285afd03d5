#!/usr/bin/env python3
"""Compare the kernels of two device-only assembly listings of one source file of model_matching_amd/csrc, kernel by kernel: the
same file compiled at two commits with the Makefile's flags plus --cuda-device-only -S.

usage: isa_diff.py OLD.s NEW.s

A kernel's body is the text between its label and its .Lfunc_end; mangled names and basic-block numbers are replaced by
placeholders before the comparison.  Prints one markdown table row per kernel of NEW: identical or the number of differing lines,
and VGPRs / SGPRs / LDS bytes / scratch bytes of both listings.  Kernels are paired by their demangled names (any file); for the
queue and per-step kernels of lcp.hip, the accumulation of refine.hip and the damped solve of refine_visible.hip pair_name() also knows
how their template arguments were renamed."""
import difflib
import re
import subprocess
import sys


def kernels(path):
    text = open(path).read()
    out = {}
    for m in re.finditer(r"^(\w+):[^\n]*\n(.*?)^\.Lfunc_end\d+:", text, re.S | re.M):
        name, body = m.group(1), m.group(2)
        if ".amdhsa_kernel " + name not in text:
            continue
        desc = text[text.index(".amdhsa_kernel " + name):]
        desc = desc[:desc.index(".end_amdhsa_kernel")]
        res = {k: int(re.search(r"\.amdhsa_%s (\d+)" % k, desc).group(1))
               for k in ("next_free_vgpr", "next_free_sgpr", "group_segment_fixed_size", "private_segment_fixed_size")}
        body = body.split("\t.section\t.rodata")[0]          # (the kernel descriptor sits between the code and .Lfunc_end)
        body = body.replace(name, "<kernel>")
        body = re.sub(r"\.LBB\d+_", ".LBB_", body)
        body = re.sub(r"\s*;.*$", "", body, flags=re.M)      # remarks (they carry block numbers too)
        out[name] = (body.splitlines(), res)
    return out


def template_args(mangled):
    m = re.search(r"kernelI((?:L[bi]\d+E)+)E", mangled)
    return [int(x) for x in re.findall(r"L[bi](\d+)E", m.group(1))] if m else []


def pair_name(old):
    """the key under which an old and a new kernel meet"""
    a = template_args(old)
    if "lcp_coopq_kernel" in old:
        if len(a) == 16:   # DETAIL UNR SORTQ PIPE IDX WPB FLAT SPLIT TILE EARLY GL FIRST NOSENT NEAR TINY CU
            a = [a[0], a[9], a[7], a[6], a[13], a[15]]
        gate = len(a) == 8 and a.pop() == 1     # GATE = 1 likewise: main() compares it with the form without the gate
        shared = len(a) == 7 and a.pop() == 1   # SHARED = 1 has no form of its own in an older listing: main() compares it with SHARED = 0
        return "queue<detail=%d dense=%d split=%d flat=%d near=%d cu=%d>" % tuple(a) + (" shared" if shared else "") + (" gate" if gate else "")
    if "lcp_coop_kernel" in old:
        if len(a) == 7:    # DETAIL UNR MASK EARLY IDX WPB SPLIT
            a = [a[0], a[6]]
        return "step<detail=%d split=%d>" % tuple(a)
    d = subprocess.run(["c++filt", old], capture_output=True, text=True).stdout.strip()
    d = re.sub(r"\(.*", "", d).replace("void ", "").replace("stocs::", "")
    # refine.hip: the shipping forms carry an empty detail argument and, refine_accumulate_kernel, an empty gate argument; its gate-on
    # form is what an older listing calls robust_fused_kernel<L>
    d = d.replace(", RefNoGate>", ">").replace(", RefGate>", ", gate>")
    d = re.sub(r"robust_fused_kernel<(\w+)>", r"refine_accumulate_kernel<\1, gate>", d)
    # refine_visible.hip: the two forms of the one damped solve are what an older listing calls ..._damped_solve_kernel and ..._contour_solve_kernel
    d = d.replace("refine_visible_damped_solve_kernel<RvDampedForm>", "refine_visible_damped_solve_kernel")
    d = d.replace("refine_visible_damped_solve_kernel<RvContourForm>", "refine_visible_contour_solve_kernel")
    return d.replace(", RefNoDetail", "").replace("<RefNoDetail>", "")


def main():
    old, new = kernels(sys.argv[1]), kernels(sys.argv[2])
    oldk = {pair_name(k): v for k, v in old.items()}
    print("| kernel | body | VGPR | SGPR | LDS B | scratch B |")
    print("|---|---|---|---|---|---|")
    seen = set()
    for k, (body, res) in sorted((pair_name(k), v) for k, v in new.items()):
        if k not in oldk and k.endswith(" gate") and k[:-5] in oldk:
            oldk[k] = oldk[k[:-5]]
        if k not in oldk and k.endswith(" shared") and k[:-7] in oldk:
            oldk[k] = oldk[k[:-7]]
        if k not in oldk:
            print("| %s | no counterpart | %s |" % (k, res))
            continue
        obody, ores = oldk[k]
        seen.add(k)
        nd = sum(1 for l in difflib.unified_diff(obody, body, lineterm="", n=0) if l[:1] in "+-" and l[:3] not in ("+++", "---"))
        cell = lambda key: ("%d" % res[key]) if ores[key] == res[key] else "%d -> %d" % (ores[key], res[key])
        print("| %s | %s | %s | %s | %s | %s |" % (k, "identical" if nd == 0 else "differs by %d lines (%d -> %d)" % (nd, len(obody), len(body)),
                                                 cell("next_free_vgpr"), cell("next_free_sgpr"), cell("group_segment_fixed_size"), cell("private_segment_fixed_size")))
    for k in sorted(set(oldk) - seen):
        print("| %s | only in the old listing | |" % k)


if __name__ == "__main__":
    main()
