"""tools/kernel_isa.py, the per-kernel digest of hipcc -S listings: what it must ignore (comments, assembler directives, the
function number in basic-block labels), what it must see (one operand), and that the comparison reports a kernel that is on
one side only.  Synthetic listings of a few lines; no compiler, no GPU."""
import importlib.util
import os

_spec = importlib.util.spec_from_file_location(
    "kernel_isa", os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tools", "kernel_isa.py"))
kernel_isa = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(kernel_isa)


def listing(name, fn, operand="v1", comment="first build", with_directives=True):
    """One kernel the way hipcc lays it out: label, body with block labels, the .amdhsa_kernel block, .Lfunc_end."""
    extra = "\t.p2align\t8\n\t.loc\t1 7 0\n" if with_directives else ""
    return f"""\t.text
\t.globl\t{name}
\t.type\t{name},@function
{name}:                                 ; @{name}
; %bb.0:                                ; {comment}
\ts_load_dwordx2 s[0:1], s[4:5], 0x0
{extra}\tv_cmp_gt_u32_e32 vcc, 4, v0
\ts_cbranch_vccz .LBB{fn}_2
.LBB{fn}_1:                             ; %loop
\tv_add_f32_e32 v0, v0, {operand}        ; {comment}

\ts_branch .LBB{fn}_1
.LBB{fn}_2:
\ts_endpgm
\t.section\t.rodata,"a",@progbits
\t.p2align\t6, 0x0
\t.amdhsa_kernel {name}
\t\t.amdhsa_group_segment_fixed_size 512
\t\t.amdhsa_private_segment_fixed_size 16
\t\t.amdhsa_next_free_vgpr 12
\t\t.amdhsa_next_free_sgpr 20
\t.end_amdhsa_kernel
\t.text
.Lfunc_end{fn}:
\t.size\t{name}, .Lfunc_end{fn}-{name}
                                        ; -- End function
"""


def one(text):
    rows = kernel_isa.digest([text])
    assert len(rows) == 1
    return rows[0].split("\t")


def test_comments_directives_and_function_number_do_not_count():
    a = one(listing("kern_a", 0))
    b = one(listing("kern_a", 7, comment="second build, another file", with_directives=False))
    assert a == b
    # name, hash, instructions (labels not counted), vgpr, sgpr, scratch, lds
    assert a[0] == "kern_a" and a[2:] == ["6", "12", "20", "16", "512"]


def test_one_operand_changes_the_hash():
    a = one(listing("kern_a", 0))
    c = one(listing("kern_a", 0, operand="v2"))
    assert a[1] != c[1] and a[2:] == c[2:]
    assert kernel_isa.diff(["\t".join(a)], ["\t".join(c)])


def test_block_labels_are_kept():
    text = listing("kern_a", 0)
    moved = text.replace("\ts_branch .LBB0_1\n.LBB0_2:\n", ".LBB0_2:\n\ts_branch .LBB0_1\n")
    assert moved != text and one(moved)[1] != one(text)[1]


def test_diff_reports_a_kernel_on_one_side_only():
    both = kernel_isa.digest([listing("kern_a", 0) + listing("kern_b", 1)])
    only_a = kernel_isa.digest([listing("kern_a", 0)])
    assert len(both) == 2
    assert kernel_isa.diff(both, both) == []
    assert kernel_isa.diff(both, only_a) == ["only in first:  kern_b"]
    assert kernel_isa.diff(only_a, both) == ["only in second: kern_b"]
    # '#' lines (the header, notes on renamed kernels) are not kernels
    assert kernel_isa.diff([kernel_isa.HEADER] + both, both) == []


def test_command_line_exit_status(tmp_path, capsys):
    s = tmp_path / "k.s"
    s.write_text(listing("kern_a", 0) + listing("kern_b", 1))
    assert kernel_isa.main(["digest", str(s)]) == 0
    full = capsys.readouterr().out
    a, b = tmp_path / "a.txt", tmp_path / "b.txt"
    a.write_text(full)
    b.write_text("\n".join(l for l in full.splitlines() if not l.startswith("kern_b")) + "\n")
    assert kernel_isa.main(["diff", str(a), str(a)]) == 0
    assert kernel_isa.main(["diff", str(a), str(b)]) == 1
    assert "only in first:  kern_b" in capsys.readouterr().out
