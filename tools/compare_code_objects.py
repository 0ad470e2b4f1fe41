#!/usr/bin/env python3
"""Compare the gfx950 code of two builds of marl-mass_amd/csrc, file by file (a refactor that only moves text must change none).

    python tools/compare_code_objects.py [--subset] BUILD_A BUILD_B [name.o | name.so ...]     (default: every *.o of BUILD_A)

For each object or library present in both directories: the device code objects are taken out of its .hip_fatbin section
(clang-offload-bundler, one per translation unit) and compared by
  * the instructions of every kernel and device function (llvm-objdump -d; position-free: no addresses, no encodings, no pc-relative
    displacements),
    and, as a stricter whole, the full disassembly text in file order;
  * the kernel metadata of the notes (registers, scratch, LDS, kernarg size);
  * the non-local host symbols, defined and undefined (llvm-readelf --syms), apart from the per-file __hip_cuid_* identifier.
Prints one JSON line per file and exits 1 if anything differs (--subset: BUILD_B may lack kernels and symbols of BUILD_A, as a
tuning build that instantiates less; what both hold must still be equal).  Needs no GPU.
"""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile

MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"
META_KEYS = (".vgpr_count", ".sgpr_count", ".agpr_count", ".private_segment_fixed_size", ".group_segment_fixed_size",
             ".kernarg_segment_size", ".max_flat_workgroup_size", ".wavefront_size")


def run(llvm, tool, *args):
    return subprocess.run([os.path.join(llvm, tool), *args], check=True, capture_output=True, text=True).stdout


def code_objects(llvm, arch, path, tmp):
    """the device code objects of `path`, in file order"""
    fat = os.path.join(tmp, "fatbin")
    run(llvm, "llvm-objcopy", "--dump-section", ".hip_fatbin=" + fat, path)
    blob = open(fat, "rb").read()
    starts = [m.start() for m in re.finditer(re.escape(MAGIC), blob)]
    out = []
    for k, a in enumerate(starts):
        piece = os.path.join(tmp, "bundle%d" % k)
        open(piece, "wb").write(blob[a:starts[k + 1] if k + 1 < len(starts) else len(blob)])
        co = os.path.join(tmp, "co%d" % k)
        run(llvm, "clang-offload-bundler", "--unbundle", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--" + arch,
            "--input=" + piece, "--output=" + co)
        out.append(co)
    return out


def describe(llvm, arch, path):
    with tempfile.TemporaryDirectory() as tmp:
        whole, funcs, meta = [], {}, {}
        for co in code_objects(llvm, arch, path, tmp):
            whole.append("\n".join(l for l in run(llvm, "llvm-objdump", "-d", co).splitlines() if "file format" not in l))
            name = None
            for line in run(llvm, "llvm-objdump", "-d", "--no-leading-addr", "--no-show-raw-insn", co).splitlines():
                m = re.match(r"^[0-9a-f]* ?<(.+)>:$", line)
                if m:
                    name = m.group(1)
                    funcs[name] = []
                elif name and line.strip() not in ("", "..."):  # ("...": padding behind a function; the trailing comment repeats address and encoding, a branch target stays)
                    text = re.sub(r"//\s*[0-9A-Fa-f]+:(\s+[0-9A-Fa-f]{8})+", "//", line.strip())
                    if funcs[name] and funcs[name][-1].startswith("s_getpc_b64"):  # pc-relative address of a variable in a linked
                        text = re.sub(r"^(s_add_u32 \S+ \S+) \S+", r"\1 <pc-relative>", text)  # code object: where it lies, not what runs
                    funcs[name].append(" ".join(text.split()))
            entry = None
            for line in run(llvm, "llvm-readelf", "--notes", co).splitlines():
                if re.match(r"^\s+- \.\w+:", line) and line.startswith("  - "):
                    entry = {}
                m = re.match(r"^\s+(?:- )?(\.\w+):\s+(\S.*)$", line)
                if m and entry is not None:
                    if m.group(1) == ".name":
                        meta[m.group(2)] = entry
                    elif m.group(1) in META_KEYS:
                        entry[m.group(1)] = m.group(2)
        syms = set()
        for line in run(llvm, "llvm-readelf", "--wide", "--dyn-syms" if path.endswith(".so") else "--syms", path).splitlines():
            parts = line.split()  # Num Value Size Type Bind Vis Ndx Name
            if len(parts) == 8 and parts[4] in ("GLOBAL", "WEAK") and not parts[7].startswith("__hip_cuid_"):
                syms.add(("undefined" if parts[6] == "UND" else "defined", parts[7]))
        return {"whole": whole, "funcs": funcs, "meta": meta, "syms": syms}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("a")
    ap.add_argument("b")
    ap.add_argument("files", nargs="*")
    ap.add_argument("--llvm", default="/opt/rocm/lib/llvm/bin")
    ap.add_argument("--arch", default="gfx950")
    ap.add_argument("--subset", action="store_true", help="BUILD_B may hold fewer kernels and host symbols than BUILD_A")
    args = ap.parse_args()
    files = args.files or sorted(f for f in os.listdir(args.a) if f.endswith(".o"))
    bad = 0
    for f in files:
        pa, pb = os.path.join(args.a, f), os.path.join(args.b, f)
        if not os.path.exists(pb):
            print(json.dumps({"file": f, "only_in": args.a}))
            bad += 1
            continue
        da, db = describe(args.llvm, args.arch, pa), describe(args.llvm, args.arch, pb)
        common = set(da["funcs"]) & set(db["funcs"])
        row = {"file": f, "kernels": [len(da["meta"]), len(db["meta"])], "functions_compared": len(common),
               "functions_only_a": sorted(set(da["funcs"]) - common), "functions_only_b": sorted(set(db["funcs"]) - common),
               "instructions_differ": sorted(n for n in common if da["funcs"][n] != db["funcs"][n]),
               "metadata_differ": sorted(n for n in set(da["meta"]) & set(db["meta"]) if da["meta"][n] != db["meta"][n]),
               "whole_disassembly_equal": da["whole"] == db["whole"],
               "symbols_only_a": sorted(map(" ".join, da["syms"] - db["syms"])),
               "symbols_only_b": sorted(map(" ".join, db["syms"] - da["syms"]))}
        print(json.dumps(row))
        differs = row["instructions_differ"] or row["metadata_differ"] or row["functions_only_b"] or row["symbols_only_b"]
        if differs or (not args.subset and (row["functions_only_a"] or row["symbols_only_a"])):
            bad += 1
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
