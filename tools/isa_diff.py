#!/usr/bin/env python3
"""Show that a csrc change left the gfx950 code of every kernel alone (CPU only).

    python tools/isa_diff.py PARENT_BUILD_DIR NEW_BUILD_DIR [--allow-pcrel]

Both directories hold the objects of one `make -C .../csrc` (csrc/build/*.o), built with the
same hipcc.  Each object's gfx950 code object is disassembled (csrc/check_hazards.py
disassemble) and compared function by function by mangled name, the `//` comments (addresses)
stripped; the per-kernel metadata of `llvm-readobj --notes` (vgpr / agpr / sgpr counts, spills,
private and group segment size, max workgroup size, kernarg size) is compared per kernel.  One
summary line per object and a total are printed; the exit status is 1 on any difference.

--allow-pcrel accepts lines that differ only in the 32-bit literal of the s_add_u32 /
s_addc_u32 pair that follows an s_getpc_b64: pc-relative addresses, which move when a
neighbouring function is added, removed or reordered.  A change that touches no kernel must not
need it.  The comparison is textual; it looks for no particular instruction.
"""
import argparse
import glob
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fine-grained-emotional-control-of-tts_amd", "csrc"))
import check_hazards  # noqa: E402

META = ("vgpr_count", "agpr_count", "sgpr_count", "vgpr_spill_count", "sgpr_spill_count",
        "private_segment_fixed_size", "group_segment_fixed_size", "max_flat_workgroup_size",
        "kernarg_segment_size")


def code_object(obj, out):
    """Unbundle the gfx950 code object of a hipcc -c object into the file `out`; its size."""
    fb = out + ".fb"
    subprocess.run([f"{check_hazards.LLVM}/llvm-objcopy", "-O", "binary",
                    "--only-section=.hip_fatbin", obj, fb], check=True)
    subprocess.run([f"{check_hazards.LLVM}/clang-offload-bundler", "--type=o",
                    f"--targets={check_hazards.TARGET}", f"--input={fb}", f"--output={out}",
                    "--unbundle"], check=True)
    return os.path.getsize(out)


def functions(text):
    """{mangled name: [instruction lines, comments stripped]} in the order of the code object."""
    out, cur = {}, None
    for line in text.splitlines():
        m = re.match(r"^[0-9a-f]+ <(.+)>:$", line)
        if m:
            cur = out.setdefault(m.group(1), [])
        elif cur is not None and line.strip():
            cur.append(line.split("//")[0].strip())
    return out


def metadata(co):
    """{kernel name: {field: value}} from the AMDGPU metadata note (kernel-level keys only)."""
    notes = subprocess.run([f"{check_hazards.LLVM}/llvm-readobj", "--notes", co], check=True,
                           capture_output=True, text=True).stdout
    kernels, cur = {}, None
    for line in notes.splitlines():
        m = re.match(r"^(  - | {4})\.(\w+):\s*(.*)$", line)
        if not m:
            continue
        if m.group(1) == "  - ":
            cur = {}
        if cur is None:
            continue
        if m.group(2) == "name":
            kernels[m.group(3)] = cur
        elif m.group(2) in META:
            cur[m.group(2)] = m.group(3)
    return kernels


_LITERAL = re.compile(r",\s*(0x[0-9a-f]+|-?\d+)$")   # the last operand, a literal


def diff_lines(a, b):
    """(lines that differ, of those the pc-relative literal lines) of two instruction lists."""
    if len(a) != len(b):
        return max(len(a), len(b)), 0
    bad = pcrel = 0
    since_getpc = 99
    for x, y in zip(a, b):
        since_getpc = 0 if x.startswith("s_getpc_b64") else since_getpc + 1
        if x == y:
            continue
        bad += 1
        if (since_getpc <= 2 and re.match(r"s_addc?_u32 ", x)
                and _LITERAL.sub("", x) == _LITERAL.sub("", y)):
            pcrel += 1
    return bad, pcrel


def compare(parent, new, allow_pcrel):
    with tempfile.TemporaryDirectory() as td:
        pa, pb = os.path.join(td, "a.co"), os.path.join(td, "b.co")
        sa, sb = code_object(parent, pa), code_object(new, pb)
        fa = functions(check_hazards.disassemble(parent))
        fb = functions(check_hazards.disassemble(new))
        ma, mb = metadata(pa), metadata(pb)
    removed = [n for n in fa if n not in fb]
    added = [n for n in fb if n not in fa]
    common = [n for n in fa if n in fb]
    differing = pcrel = 0
    detail = []
    for n in common:
        bad, pc = diff_lines(fa[n], fb[n])
        if bad:
            detail.append(f"  differs ({bad} lines, {pc} pc-relative) {n}")
        differing += bad - pc
        pcrel += pc
    mism = 0
    for n in common:
        if n in ma or n in mb:
            if ma.get(n) != mb.get(n):
                mism += 1
                detail.append(f"  metadata {ma.get(n)} -> {mb.get(n)} {n}")
    same_order = common == [n for n in fb if n in fa]
    name = os.path.basename(parent)
    print(f"{name}: code object {sa} -> {sb} bytes; functions compared {len(common)} (with "
          f"metadata: {len(ma)} kernels in parent, {len(mb)} in branch), removed {len(removed)}, "
          f"added {len(added)}, differing lines {differing}, pc-relative literal lines that "
          f"differ {pcrel}, metadata mismatches {mism}, order "
          f"{'kept' if same_order else 'changed'}")
    for n in removed:
        print(f"  removed {n}")
    for n in added:
        print(f"  added {n}")
    for d in detail:
        print(d)
    fail = len(removed) + len(added) + differing + mism + (0 if allow_pcrel else pcrel)
    return len(common), len(removed), len(added), differing, pcrel, mism, fail


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("parent_build_dir")
    ap.add_argument("new_build_dir")
    ap.add_argument("--allow-pcrel", action="store_true")
    a = ap.parse_args()
    names = sorted({os.path.basename(p) for d in (a.parent_build_dir, a.new_build_dir)
                    for p in glob.glob(os.path.join(d, "*.o"))})
    if not names:
        sys.exit("no objects found")
    tot = [0] * 7
    for n in names:
        pa, pb = os.path.join(a.parent_build_dir, n), os.path.join(a.new_build_dir, n)
        if not (os.path.exists(pa) and os.path.exists(pb)):
            print(f"{n}: only in {'parent' if os.path.exists(pa) else 'branch'}")
            tot[6] += 1
            continue
        tot = [x + y for x, y in zip(tot, compare(pa, pb, a.allow_pcrel))]
    print(f"total: compared {tot[0]}, removed {tot[1]}, added {tot[2]}, differing lines {tot[3]}, "
          f"{'allowed ' if a.allow_pcrel else ''}pc-relative literal lines {tot[4]}, metadata "
          f"mismatches {tot[5]}")
    return 1 if tot[6] else 0


if __name__ == "__main__":
    sys.exit(main())
