#!/usr/bin/env python3
"""Do two source trees compile a translation unit to the same gfx950 kernels?

    python tools/compare_kernel_asm.py OLD_TREE NEW_TREE riab_rates.hip [-D...]

Compiles ratinabox_amd/csrc/<TU> of both trees to device assembly with the flags of ratinabox_amd/_build.py (plus any
extra flags given), cuts the two texts into functions and prints the symbols that exist in one tree only and those
whose text is not identical, with the size of the difference and a verdict: `permuted` — the same instructions up to
their order and the numbers of their registers, everything else (kernel descriptor, resource comments, labels) the same
text, see classify() — or `differs`.  Exit status 0: the same symbols, the same text for each; 3: the same symbols, each
identical or permuted; 1: a symbol differs or is missing; 2: usage, or a compilation failed.

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
INSTRUCTION = re.compile(r"\s+([a-z][a-z0-9_]*\b|;\s*(implicit-def|kill):)")  # (directives start with a dot, labels in column 0)
REG = re.compile(r"\b([vsa])(?:\d+\b|(\[)\d+:\d+\])")
NOTE_REG = re.compile(r"\$([vsa])gpr\d+(?:_[vsa]gpr\d+)*")


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


def _is_instruction(line):
    """An instruction, or the allocator's note on a register in front of one (`; implicit-def: $vgpr18`, `; kill: ...`)."""
    return bool(INSTRUCTION.match(line))


def _mask(line):
    return NOTE_REG.sub(lambda m: m.group(1) + "gpr#", REG.sub(lambda m: m.group(1) + ("[#]" if m.group(2) else "#"), line))


def classify(old, new):
    """'identical', 'permuted' or 'differs' for two functions' lines (as functions() returns them).

    permuted: the same instructions up to their order and the numbers of their registers — everything that is not an
    instruction (labels, directives, the .amdhsa_ kernel descriptor, the resource comments: register counts, scratch and
    LDS size, code length, occupancy) is the same text in the same order, and the instruction lines are the same
    multiset once v12, s[4:5], a3, v[6:7] read v#, s[#], a#, v[#].  An opcode, an immediate, a label or a wait count
    that changed is 'differs'."""
    if old == new:
        return "identical"
    if [l for l in old if not _is_instruction(l)] != [l for l in new if not _is_instruction(l)]:
        return "differs"
    if sorted(_mask(l) for l in old if _is_instruction(l)) != sorted(_mask(l) for l in new if _is_instruction(l)):
        return "differs"
    return "permuted"


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
    bad = permuted = 0
    for sym in sorted(set(old) ^ set(new)):
        print(("only in old: " if sym in old else "only in new: ") + sym)
        bad += 1
    for sym in sorted(set(old) & set(new)):
        verdict = classify(old[sym], new[sym])
        if verdict != "identical":
            d = [l for l in difflib.unified_diff(old[sym], new[sym], n=0) if l[0] in "+-" and l[:3] not in ("+++", "---")]
            print("%s (%d lines of %d): %s" % (verdict, len(d), len(old[sym]), sym))
            permuted += verdict == "permuted"
            bad += verdict == "differs"
    print("%d functions in old, %d in new, %d permuted, %d differ or are missing" % (len(old), len(new), permuted, bad))
    return 1 if bad else 3 if permuted else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
