#!/usr/bin/env python3
"""Static instructions of the headline step kernel by source line (build-container tool: no GPU needed).

    python tools/static_by_source.py [--root CHECKOUT] [--label NAME] [--json OUT] [--top 40] [--exec-regions]

Compiles the single-object, single-instantiation form of the step library (marl-mass_amd/csrc/mm_step_all.hip) for gfx950 to assembly with line tables
(-gline-tables-only: code generation is the release build's), walks the body of step_kernel<8, MM_ENV_V1, MM_SHIELD_MASS, false,
false, false, false, false> and books every instruction on the `.loc` in force, i.e. on the innermost inlined source line.  Output:
totals per file, per function of include/mm_math.h and marl-mass_amd/csrc/mm_device.h (by the line ranges of their
definitions), literal s_mov_b32, fp64 divisions (v_div_fmas_f64) per function, and the heaviest lines.

--exec-regions books the exec-mask instructions instead (s_*_saveexec_b64 and s_cbranch_*: what a short-circuit chain or a
divergent `if` compiles to) on their source lines: totals, per file, per function of the two headers and EVERY line that holds
one, heaviest first -- the candidate list for the next select-form rewrite, read from a file instead of derived again.
"""
import argparse
import collections
import json
import os
import re
import subprocess
import tempfile

KERNEL = "step_kernel<8, 1, 2, false, false, false, false, false>"
FLAGS = ["-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "-fno-fast-math", "-DMM_ONLY_G=8", "-DMM_ONLY_MIXED=false",
         "-DMM_ONLY_SHIELD=2", "-gline-tables-only", "--cuda-device-only", "-S"]


def functions(path):
    """[(first line, name)] of the function definitions of a header (MMM_FN / MM_DEV ... name(...) {)."""
    out = []
    for n, ln in enumerate(open(path), 1):
        m = re.match(r"(?:template\s*<[^>]*>\s*)?(?:MMM_FN|MM_DEV)\s+[\w:<> ]*?[\s&*](\w+)\(", ln)
        if m:
            out.append((n, m.group(1)))
    return out


def owner(funcs, line):
    name = None
    for first, f in funcs:
        if first > line:
            break
        name = f
    return name


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--label", default="tree")
    ap.add_argument("--json", default=None)
    ap.add_argument("--top", type=int, default=40)
    ap.add_argument("--exec-regions", action="store_true")
    ap.add_argument("--hipcc", default=os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"))
    args = ap.parse_args()
    csrc = os.path.join(args.root, "marl-mass_amd", "csrc")
    with tempfile.TemporaryDirectory() as td:
        asm = os.path.join(td, "k.s")
        subprocess.check_call([args.hipcc] + FLAGS + ["-o", asm, "mm_step_all.hip"], cwd=csrc)
        text = open(asm).read().splitlines()
    syms = [m.group(1) for ln in text for m in [re.match(r"(_Z\w*step_kernel\w*):", ln)] if m]
    dem = subprocess.run(["c++filt"], input="\n".join(syms), capture_output=True, text=True).stdout.splitlines()
    sym = [s for s, d in zip(syms, dem) if KERNEL in d][0]
    files, cur, inside = {}, None, False
    by_line, by_file = collections.Counter(), collections.Counter()
    lit, div = collections.Counter(), collections.Counter()
    saveexec, cbranch = collections.Counter(), collections.Counter()
    total = 0
    for ln in text:
        m = re.match(r"\s*\.file\s+(\d+)\s+\"([^\"]*)\"(?:\s+\"([^\"]*)\")?", ln)
        if m:
            files[int(m.group(1))] = os.path.basename(m.group(3) or m.group(2))
            continue
        if ln.startswith(sym + ":"):
            inside = True
            continue
        if inside and ln.startswith(".Lfunc_end"):
            break
        if not inside:
            continue
        m = re.match(r"\s*\.loc\s+(\d+)\s+(\d+)", ln)
        if m:
            cur = (files.get(int(m.group(1)), "?"), int(m.group(2)))
            continue
        m = re.match(r"\s+([sv]_\w+|ds_\w+|global_\w+|flat_\w+|buffer_\w+|scratch_\w+)\b(.*)", ln)
        if not m or cur is None:
            continue
        total += 1
        by_line[cur] += 1
        by_file[cur[0]] += 1
        if m.group(1) == "s_mov_b32" and re.search(r",\s*(0x[0-9a-f]+|-?\d+\.?\d*(e[-+]?\d+)?)\s*(;.*)?$", m.group(2)):
            lit[cur] += 1
        if m.group(1) == "v_div_fmas_f64":
            div[cur] += 1
        if re.match(r"s_\w+_saveexec_b64$", m.group(1)):
            saveexec[cur] += 1
        if m.group(1).startswith("s_cbranch_"):
            cbranch[cur] += 1
    fn = {"mm_math.h": functions(os.path.join(args.root, "include", "mm_math.h")),
          "mm_device.h": functions(os.path.join(csrc, "mm_device.h"))}
    if args.exec_regions:
        lines = sorted(set(saveexec) | set(cbranch), key=lambda k: (-(saveexec[k] + cbranch[k]), k))
        per_file, per_fn = collections.Counter(), collections.Counter()
        for f, l in lines:
            per_file[f] += saveexec[(f, l)] + cbranch[(f, l)]
            if f in fn:
                per_fn["%s:%s" % (f, owner(fn[f], l) or "(line 0: compiler-generated)")] += saveexec[(f, l)] + cbranch[(f, l)]
        res = {"label": args.label, "kernel": KERNEL, "flags": " ".join(FLAGS), "total": total, "saveexec": sum(saveexec.values()),
               "cbranch": sum(cbranch.values()), "by_file": dict(per_file.most_common()), "by_function": dict(per_fn.most_common()),
               "lines": [{"file": f, "line": l, "saveexec": saveexec[(f, l)], "cbranch": cbranch[(f, l)]} for f, l in lines]}
        print(json.dumps({k: v for k, v in res.items() if k != "lines"}, indent=1))
        for r in res["lines"][:args.top]:
            print("%-16s %5d  saveexec %3d  cbranch %3d" % (r["file"], r["line"], r["saveexec"], r["cbranch"]))
        if args.json:
            json.dump(res, open(args.json, "w"), indent=1)
        return
    by_fn, lit_fn, div_fn = collections.Counter(), collections.Counter(), collections.Counter()
    for (f, l), n in by_line.items():
        if f in fn:
            key = "%s:%s" % (f, owner(fn[f], l))
            by_fn[key] += n
            lit_fn[key] += lit[(f, l)]
            div_fn[key] += div[(f, l)]
    res = {"label": args.label, "kernel": KERNEL, "flags": " ".join(FLAGS), "total": total, "by_file": dict(by_file.most_common()),
           "literal_s_mov_b32": sum(lit.values()), "fp64_divisions": sum(div.values()),
           "by_function": {k: {"instructions": n, "literal_s_mov_b32": lit_fn[k], "fp64_divisions": div_fn[k]} for k, n in by_fn.most_common()},
           "top_lines": [{"file": f, "line": l, "instructions": n} for (f, l), n in by_line.most_common(args.top)]}
    print(json.dumps(res, indent=1))
    if args.json:
        json.dump(res, open(args.json, "w"), indent=1)


if __name__ == "__main__":
    main()
