#!/usr/bin/env python3
"""Do two source trees compile a translation unit to the same gfx950 kernels?

    python tools/compare_kernel_asm.py OLD_TREE NEW_TREE riab_rates.hip [-D...]

Compiles ratinabox_amd/csrc/<TU> of both trees to device assembly with the flags of ratinabox_amd/_build.py (plus any
extra flags given), cuts the two texts into functions and prints the symbols that exist in one tree only and those
whose text differs, with the size of the difference.  Exit status 0: the same symbols, the same text for each.

Plain text comparison: a function's text is everything between the assembler's "Begin function" / "End function"
comments — instructions, the kernel descriptor, the resource summary.  Three things are taken out first: the padding
in front of a comment (the assembler aligns a label's comment, so the width of the label shows), the
per-translation-unit symbol __hip_cuid_<hash>, and the function's ordinal in local labels (.LBB12_3 -> .LBB_3, also
where comments name them), which changes when the order of instantiation does.  Two .s files can be given in place of the trees (nothing is compiled)."""
import difflib
import importlib.util
import os
import re
import shutil
import subprocess
import sys
import tempfile

# (the build recipe alone: importing the package would build and load the library)
_spec = importlib.util.spec_from_file_location(
    "riab_build", os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "ratinabox_amd", "_build.py"))
_build = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(_build)

BEGIN = re.compile(r"-- Begin function (\S+)")
PAD = re.compile(r"[ \t]+;")
LOCAL = re.compile(r"(\.L|\b)(BB|func_begin|func_end|tmp)\d+")


def assemble(tree, tu, extra, out):
    hipcc = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    cmd = [hipcc, *_build.FLAGS, *extra, "-I", os.path.join(tree, "include"), "-I",
           os.path.join(tree, "ratinabox_amd", "csrc"), "--cuda-device-only", "-S",
           os.path.join(tree, "ratinabox_amd", "csrc", tu), "-o", out]
    return subprocess.Popen(cmd)


def functions(path):
    out, name, lines = {}, None, []
    with open(path) as f:
        for line in f:
            if "__hip_cuid_" in line:
                continue
            m = BEGIN.search(line)
            if m:
                name, lines = m.group(1), []
            if name is not None:
                line = LOCAL.sub(lambda k: k.group(1) + k.group(2), line)
                lines.append(PAD.sub(" ;", line))  # (the assembler pads a label's comment to a column: the ordinal's width shows)
                if "-- End function" in line:
                    out[name], name = lines, None
    return out


def main(argv):
    tmp = None
    if len(argv) == 2 and all(a.endswith(".s") for a in argv):
        old_s, new_s = argv
    elif len(argv) >= 3:
        old_tree, new_tree, tu, extra = argv[0], argv[1], argv[2], argv[3:]
        tmp = tempfile.mkdtemp(prefix="kernel_asm_")
        old_s, new_s = os.path.join(tmp, "old.s"), os.path.join(tmp, "new.s")
        jobs = [assemble(old_tree, tu, extra, old_s), assemble(new_tree, tu, extra, new_s)]  # side by side
        failed = [j.wait() for j in jobs]
        if any(failed):
            shutil.rmtree(tmp, ignore_errors=True)
            print("compilation failed")
            return 2
    else:
        print(__doc__)
        return 2
    old, new = functions(old_s), functions(new_s)
    if tmp:
        shutil.rmtree(tmp, ignore_errors=True)
    bad = 0
    for sym in sorted(set(old) ^ set(new)):
        print(("only in old: " if sym in old else "only in new: ") + sym)
        bad += 1
    for sym in sorted(set(old) & set(new)):
        if old[sym] != new[sym]:
            d = [l for l in difflib.unified_diff(old[sym], new[sym], n=0) if l[0] in "+-" and l[:3] not in ("+++", "---")]
            print("differs (%d lines of %d): %s" % (len(d), len(old[sym]), sym))
            bad += 1
    print("%d functions in old, %d in new, %d differ or are missing" % (len(old), len(new), bad))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
