"""``scripts/kernel_bodies.py diff`` compares EVERY kernel the listing's ``amdhsa.kernels`` metadata names: ``c++filt``
prints a return type only for template instantiations, so a selection on the ``void`` prefix once left every non-template
kernel out without a word.  Two small synthetic listings, one template kernel and one non-template kernel each."""
import os
import subprocess
import sys

import pytest

SCRIPT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scripts", "kernel_bodies.py")
TEMPLATE = "_ZN12_GLOBAL__N_17k_shearILi2EEEvlPf"      # void (anonymous namespace)::k_shear<2>(long, float*)
PLAIN = "_ZN12_GLOBAL__N_16k_wallElPf"                 # (anonymous namespace)::k_wall(long, float*)
HELPER = "_ZN12_GLOBAL__N_16helperEf"                  # a device function that was not inlined: no kernel


def listing(plain_op="v_add_f32_e32 v0, v0, v1", helper_op="v_mov_b32_e32 v0, 0", label=7):
    def fn(i, name, body):
        return (f"\t.globl\t{name}\n\t.p2align\t8\n\t.type\t{name},@function\n{name}:   ; @{name}\n; %bb.0:\n{body}"
                f"\ts_endpgm\n.Lfunc_end{i}:\n\t.size\t{name}, .Lfunc_end{i}-{name}\n")
    meta = "".join(f"  - .agpr_count:     0\n    .args:\n      - .offset:         0\n        .size:           8\n"
                   f"    .group_segment_fixed_size: 0\n    .name:           {n}\n    .private_segment_fixed_size: 0\n"
                   f"    .sgpr_count:     12\n    .symbol:         {n}.kd\n    .vgpr_count:     {v}\n"
                   for n, v in ((TEMPLATE, 9), (PLAIN, 5)))
    return ("\t.text\n"
            + fn(0, TEMPLATE, f"\ts_load_dwordx2 s[0:1], s[4:5], 0x0\n\ts_cbranch_scc1 .LBB0_{label}\n"
                              f"\tv_mul_f32_e32 v0, v0, v0 ; a comment\n.LBB0_{label}:\n")
            + fn(1, PLAIN, f"\ts_load_dwordx2 s[0:1], s[4:5], 0x0\n\t{plain_op}\n")
            + fn(2, HELPER, f"\t{helper_op}\n")
            + "\t.section\t.note.GNU-stack\n\t.amdgpu_metadata\n---\namdhsa.kernels:\n" + meta
            + "amdhsa.target:   amdgcn-amd-amdhsa--gfx950\n...\n\t.end_amdgpu_metadata\n")


def run(*args):
    r = subprocess.run([sys.executable, SCRIPT, *args], capture_output=True, text=True)
    return r.returncode, r.stdout


@pytest.fixture()
def parent(tmp_path):
    p = tmp_path / "parent.s"
    p.write_text(listing())
    return p


def test_template_and_plain_kernels_are_both_compared(tmp_path, parent):
    head = tmp_path / "head.s"
    head.write_text(listing(helper_op="v_mov_b32_e32 v0, 1", label=3))   # labels renumbered, a non-kernel function changed
    rc, out = run("diff", str(parent), str(head), "k_")
    assert rc == 0, out
    lines = [l for l in out.splitlines() if l.startswith("identical")]
    assert len(lines) == 2 and sum("k_shear<2>" in l for l in lines) == 1 and sum("k_wall" in l for l in lines) == 1, out
    assert "helper" not in out and "2 kernels compared, 0 differ" in out, out


def test_changed_instruction_in_the_plain_kernel_is_reported(tmp_path, parent):
    head = tmp_path / "head.s"
    head.write_text(listing(plain_op="v_sub_f32_e32 v0, v0, v1"))
    rc, out = run("diff", str(parent), str(head), "k_")
    assert rc == 1, out
    different = [l for l in out.splitlines() if l.startswith("DIFFERENT")]
    assert len(different) == 1 and "k_wall" in different[0], out
    assert any(l.startswith("identical") and "k_shear<2>" in l for l in out.splitlines()), out
    assert "2 kernels compared, 1 differ" in out, out
    rc, out = run("diff", str(parent), str(head), "k_wall")      # by its own name too
    assert rc == 1 and "1 kernels compared, 1 differ" in out, out


def test_pattern_that_matches_nothing_fails(parent):
    rc, out = run("diff", str(parent), str(parent), "k_no_such_kernel")
    assert rc == 1 and "0 kernels compared" in out, out


def test_meta_lists_both_kernels(parent):
    rc, out = run("meta", str(parent), "k_")
    assert rc == 0 and len(out.splitlines()) == 2 and "vgpr    9" in out and "vgpr    5" in out, out
