"""The instruction census' tooling (scripts/instruction_census.py, scripts/census_timed_build_check.py) without a GPU or a compiler:
instruction classes, basic blocks of a listing, and the rule that the census' counters exist in diagnostic builds only."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import census_timed_build_check as chk  # noqa: E402
import instruction_census as ic  # noqa: E402

LISTING = """\t.file\t1 "/x" "csrc/rt_device.h"
_ZN3rtd13render_kernelILb1ELb0ELi1024ELi2ELb0EEEvNS_12RenderParamsE:
\t.loc\t1 45 0
\tv_add_f64 v[0:1], v[2:3], v[4:5]
\tv_fmac_f64_e32 v[0:1], v[2:3], v[4:5]
\ts_cbranch_execz .LBB0_2
\tv_cndmask_b32_e64 v2, 0, 1, vcc
\tv_readlane_b32 s4, v126, 10
.LBB0_2:
\t.loc\t1 0 0
\tv_cmp_lt_f64_e32 vcc, v[0:1], v[2:3]
\tds_read_b64 v[0:1], v2
1:
\tv_fma_f32 v100, v100, v25, v27
\ts_branch 1b
\ts_endpgm
.Lfunc_end0:
"""


@pytest.mark.parametrize("op,cls", [("v_add_f64", "f64_add"), ("v_mul_f64", "f64_mul"), ("v_fma_f64", "f64_fma"), ("v_fmac_f64_e32", "f64_fma"),
                                    ("v_rcp_f64_e32", "f64_trans"), ("v_rsq_f64_e32", "f64_trans"), ("v_max_f64", "f64_other"), ("v_cmp_lt_f64_e32", "cmp"),
                                    ("v_cmp_eq_u32_sdwa", "cmp"), ("v_cndmask_b32_e64", "selmov"), ("v_mov_b64_e32", "selmov"), ("v_cvt_f32_f64_e32", "cvt"),
                                    ("v_readlane_b32", "xlane"), ("v_mbcnt_hi_u32_b32", "xlane"), ("v_readfirstlane_b32", "xlane"), ("v_fma_f32", "f32"),
                                    ("v_add_u32_e32", "int"), ("v_lshl_add_u64", "int"), ("v_alignbit_b32", "int")])
def test_classes(op, cls):
    assert ic.classify(op) == cls
    assert ic.cost_of(op) > 3.0


def test_blocks_of_a_listing(tmp_path):
    p = tmp_path / "k.s"
    p.write_text(LISTING)
    bl = ic.blocks(str(p))
    assert [len(b.valu()) for b in bl] == [2, 2, 1, 1, 0]  # split after the branch, at the label, at the numeric label of inline assembly
    assert bl[0].by_class() == {"f64_add": 1, "f64_fma": 1}
    assert bl[1].by_class() == {"selmov": 1, "xlane": 1}
    assert bl[2].where()[1:] == ("rt_device.h", 45)  # line 0 (compiler-made code) is counted with the line before it
    depth, spans = ic.loop_depth(bl)
    assert depth[3] == 1 and depth[0] == 0


def test_strip_diag_keeps_the_else_part():
    text = "a\n#ifdef RTD_STAGE_CLOCKS\nb\n#if X\nc\n#endif\n#else\nd\n#endif\n#ifdef OTHER\ne\n#endif\nf\n"
    assert chk.strip_diag(text) == "a\nd\n#ifdef OTHER\ne\n#endif\nf\n"


def test_census_counters_exist_in_diagnostic_builds_only(rt):
    csrc = os.path.join(ROOT, "ray-tracing-fsharp_amd", "csrc")
    for f in ("rt_device.h", "rt_render_kernel.h", "rt_launch_consts.h", "rt_launch_plan.h", "rtfs_amd.hip"):
        plain = chk.strip_diag(open(os.path.join(csrc, f)).read())
        assert "g_census" not in plain and "rt_diag_census" not in plain, f
    assert "rt_diag_census" not in open(os.path.join(ROOT, "include", "rtfs_amd.h")).read()
    assert not hasattr(rt.lib, "rt_diag_census")  # the product library's exported symbols are those of include/rtfs_amd.h
