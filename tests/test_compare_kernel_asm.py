"""tools/compare_kernel_asm.py's verdict on two functions' assembly text: identical, permuted (the same instructions up to
their order and register numbers) or differs.  Hand-written texts; nothing is compiled."""
import importlib.util
import os

_spec = importlib.util.spec_from_file_location(
    "compare_kernel_asm", os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tools", "compare_kernel_asm.py"))
cmp_asm = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(cmp_asm)

BASE = """\
\t.globl\tkern ; -- Begin function kern
kern:
; %bb.0:
\ts_load_dwordx2 s[4:5], s[0:1], 0x0
\tv_mov_b64_e32 v[6:7], 0
\tv_mov_b32_e32 v12, 0
 ; implicit-def: $vgpr12
\ts_waitcnt lgkmcnt(0)
\tv_lshl_add_u64 v[2:3], v[0:1], 3, s[4:5]
\tglobal_store_dwordx2 v[2:3], v[6:7], off
.LBB0_1:
\ts_endpgm
\t.amdhsa_next_free_vgpr 13
; NumVgprs: 13
; ScratchSize: 0
\t; -- End function
""".splitlines(keepends=True)


def _changed(old, new):
    assert sum(old in l for l in BASE) == 1
    return [l.replace(old, new) for l in BASE]


def test_identical():
    assert cmp_asm.classify(BASE, list(BASE)) == "identical"


def test_one_line_moved_is_permuted():
    moved = list(BASE)
    moved.insert(3, moved.pop(4))  # the zero initialisation in front of the load
    assert moved != BASE
    assert cmp_asm.classify(BASE, moved) == "permuted"


def test_one_register_renamed_is_permuted():
    renamed = [l.replace("v12", "v9").replace("vgpr12", "vgpr9") for l in BASE]
    assert cmp_asm.classify(BASE, renamed) == "permuted"
    pair = [l.replace("v[6:7]", "v[8:9]") for l in BASE]
    assert cmp_asm.classify(BASE, pair) == "permuted"


def test_one_opcode_changed_differs():
    assert cmp_asm.classify(BASE, _changed("v_mov_b32_e32 v12, 0", "v_not_b32_e32 v12, 0")) == "differs"


def test_operand_kind_immediate_or_wait_changed_differs():
    assert cmp_asm.classify(BASE, _changed("3, s[4:5]", "3, v[4:5]")) == "differs"  # (a scalar pair is not a vector pair)
    assert cmp_asm.classify(BASE, _changed("0x0", "0x8")) == "differs"
    assert cmp_asm.classify(BASE, _changed("lgkmcnt(0)", "lgkmcnt(1)")) == "differs"


def test_resources_or_labels_changed_differs():
    assert cmp_asm.classify(BASE, _changed("NumVgprs: 13", "NumVgprs: 14")) == "differs"
    assert cmp_asm.classify(BASE, _changed(".amdhsa_next_free_vgpr 13", ".amdhsa_next_free_vgpr 14")) == "differs"
    assert cmp_asm.classify(BASE, _changed(".LBB0_1:", ".LBB0_2:")) == "differs"


def test_summary_and_exit_status(tmp_path, capsys):
    def write(name, functions):
        p = tmp_path / name
        p.write_text("".join("".join(f) for f in functions))
        return str(p)

    other = [l.replace("kern", "kern2") for l in BASE]
    moved = list(other)
    moved.insert(3, moved.pop(4))
    old = write("old.s", [BASE, other])
    assert cmp_asm.main([old, write("same.s", [BASE, other])]) == 0
    assert cmp_asm.main([old, write("perm.s", [BASE, moved])]) == 3
    assert "permuted (" in capsys.readouterr().out
    assert cmp_asm.main([old, write("diff.s", [_changed("v_mov_b32_e32 v12, 0", "v_not_b32_e32 v12, 0"), moved])]) == 1
    out = capsys.readouterr().out
    assert "1 permuted, 1 differ or are missing" in out
