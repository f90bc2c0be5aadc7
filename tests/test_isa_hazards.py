"""The instructions that ship, audited for wait states (tools/isa_hazards.py) — no GPU needed.

The dense engine of the default MLP path (csrc/gemm_glds64.h) issues its MFMAs from inline assembly, and the compiler
pads no hazard of an instruction inside an asm string.  A missing wait state gives "wrong values on some waves of some
launches": numeric tests may pass for ever.  So the compiled code itself is checked: every translation unit of
csrc/build.sh is compiled to assembly with build.sh's flags (once per session, in parallel) and every kernel is walked
along every static successor edge.  The first half of this file tests the checker on hand-written snippets."""
import os
import sys
import time

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import isa_hazards as ih  # noqa: E402


# ------------------------------------------------------------------------------------------- the checker on snippets
def _kernel(body):
    return ("\t.type\tk,@function\nk:                                      ; @k\n; %bb.0:\n" + body +
            "\n.Lfunc_end0:\n\t.size\tk, .Lfunc_end0-k\n")


def _audit(body):
    findings, stats, table = ih.audit({"snippet.s": _kernel(body)}, ih.H1_EXPECTED)
    return findings


def _inline(*lines):
    return "\t;;#ASMSTART\n" + "".join(f"\t{x}\n" for x in lines) + "\t;;#ASMEND\n"


MFMA = "v_mfma_f32_16x16x4_f32 v[0:3], v4, v5, v[0:3]"
UNRELATED = "\ts_add_i32 s0, s1, 1\n\tv_add_u32_e32 v20, v21, v22\n\ts_cmp_lt_i32 s5, 32\n"


def test_h1_copy_in_front_of_the_untied_nops_is_flagged():
    """the shape found in mlp_layer_glds: MFMA, three unrelated instructions, a v_mov_b64 of D, THEN the nops"""
    f = _audit(_inline(MFMA) + UNRELATED + "\tv_mov_b64_e32 v[14:15], v[0:1]\n" + _inline("s_nop 15", "s_nop 15") +
               "\ts_endpgm")
    assert [(x.rule, x.found, x.required) for x in f] == [("H1", 3, 10)]
    assert "v_mov_b64" in f[0].consumer and "v_mfma" in f[0].producer


def test_h1_nops_in_front_of_the_copy_are_clean():
    assert _audit(_inline(MFMA) + _inline("s_nop 11") + UNRELATED + "\tv_mov_b64_e32 v[14:15], v[0:1]\n\ts_endpgm") == []
    # exactly the requirement: s_nop 9 = 10 states; one fewer is a finding
    assert _audit(_inline(MFMA) + "\ts_nop 9\n\tv_mov_b32_e32 v9, v3\n\ts_endpgm") == []
    f = _audit(_inline(MFMA) + "\ts_nop 8\n\tv_mov_b32_e32 v9, v3\n\ts_endpgm")
    assert [(x.rule, x.found) for x in f] == [("H1", 9)]


def test_h1_a_write_to_d_counts_like_a_read():
    f = _audit(_inline(MFMA) + "\tv_lshlrev_b32_e32 v2, 4, v50\n\ts_endpgm")
    assert [(x.rule, x.found) for x in f] == [("H1", 0)]


def test_h1_violation_only_behind_a_branch_target_is_flagged():
    """the fall-through path is padded; the reader behind the branch target is not"""
    body = (_inline(MFMA) + "\ts_cbranch_scc1 .LBB0_2\n; %bb.1:\n\ts_nop 15\n\tv_mov_b32_e32 v8, v0\n\ts_endpgm\n"
            ".LBB0_2:\n\tv_mov_b32_e32 v9, v1\n\ts_endpgm")
    f = _audit(body)
    assert [(x.rule, x.found) for x in f] == [("H1", 1)] and "v9, v1" in f[0].consumer


def test_h1_what_follows_in_the_text_but_not_in_the_control_flow_is_clean():
    """a linear scan would flag the reader behind the unconditional branch; no path leads there from the MFMA"""
    body = (_inline(MFMA) + "\ts_branch .LBB0_2\n.LBB0_1:\n\tv_mov_b32_e32 v8, v0\n\ts_endpgm\n"
            ".LBB0_2:\n\ts_nop 15\n\tv_mov_b32_e32 v9, v1\n\ts_endpgm")
    assert _audit(body) == []


def test_h1_loop_back_edge_is_followed():
    body = (".LBB0_1:\n\tv_mov_b32_e32 v9, v1\n" + "\ts_nop 15\n" + _inline(MFMA) + "\ts_cbranch_scc0 .LBB0_1\n\ts_nop 15\n\ts_endpgm")
    f = _audit(body)
    assert [(x.rule, x.found) for x in f] == [("H1", 1)]


def test_h1_accumulate_chain_is_clean_and_its_near_misses_are_not():
    chain = _inline(MFMA) + _inline(MFMA) + _inline("v_mfma_f32_16x16x4_f32 v[0:3], v6, v7, v[0:3]") + "\ts_nop 15\n\ts_endpgm"
    assert _audit(chain) == []
    # D read as an A operand; C overlapping D without being D
    f = _audit(_inline(MFMA) + _inline("v_mfma_f32_16x16x4_f32 v[0:3], v1, v5, v[0:3]") + "\ts_nop 15\n\ts_endpgm")
    assert [x.rule for x in f] == ["H1"]
    f = _audit(_inline(MFMA) + _inline("v_mfma_f32_16x16x4_f32 v[8:11], v6, v7, v[2:5]") + "\ts_nop 15\n\ts_endpgm")
    assert [x.rule for x in f] == ["H1"]
    # the chain hands the hazard on: the reader is measured from the LAST MFMA
    f = _audit(_inline(MFMA) + "\ts_nop 15\n" + _inline(MFMA) + "\tv_mov_b32_e32 v9, v1\n\ts_endpgm")
    assert [(x.rule, x.found) for x in f] == [("H1", 0)]


def test_h1_other_shape_has_its_own_requirement():
    m = "v_mfma_f32_32x32x2_f32 v[0:15], v20, v21, v[0:15]"
    assert [(x.found, x.required) for x in _audit(f"\t{m}\n\ts_nop 11\n\tv_mov_b32_e32 v30, v15\n\ts_endpgm")] == [(12, 18)]
    assert _audit(f"\t{m}\n\ts_nop 15\n\ts_nop 1\n\tv_mov_b32_e32 v30, v15\n\ts_endpgm") == []


DPP = "v_min_u32_dpp v4, v1, v1 row_shr:1 row_mask:0xf bank_mask:0xf"


def test_h2_valu_write_to_dpp_read():
    f = _audit("\tv_add_u32_e32 v1, v2, v3\n" + _inline(DPP) + "\ts_endpgm")
    assert [(x.rule, x.found, x.required) for x in f] == [("H2", 0, 2)]
    f = _audit("\tv_add_u32_e32 v1, v2, v3\n" + _inline("s_nop 0", DPP) + "\ts_endpgm")
    assert [(x.rule, x.found) for x in f] == [("H2", 1)]
    assert _audit("\tv_add_u32_e32 v1, v2, v3\n" + _inline("s_nop 1", DPP) + "\ts_endpgm") == []
    assert _audit("\tv_add_u32_e32 v7, v2, v3\n" + _inline(DPP) + "\ts_endpgm") == []          # another register
    # not only the first producer of a kernel is followed
    f = _audit("\tv_add_u32_e32 v30, v2, v3\n\ts_nop 7\n\tv_add_u32_e32 v1, v2, v3\n" + _inline(DPP) + "\ts_endpgm")
    assert [(x.rule, x.found) for x in f] == [("H2", 0)]
    # a DPP instruction is a VALU write itself: the next DPP step reads its result
    assert [x.rule for x in _audit(_inline("s_nop 1", "v_min_u32_dpp v1, v1, v1 row_shr:1", "v_min_u32_dpp v1, v1, v1 row_shr:2") + "\ts_endpgm")] == ["H2"]


def test_h3_valu_written_sgpr_to_vmem():
    f = _audit("\tv_readfirstlane_b32 s4, v0\n\tglobal_load_dword v1, v2, s[4:5]\n\ts_endpgm")
    assert [(x.rule, x.found, x.required) for x in f] == [("H3", 0, 5)]
    f = _audit("\tv_cmp_lt_u32_e64 s[4:5], v0, v1\n\ts_nop 3\n\tbuffer_load_dword v1, v2, s[4:7], 0 offen\n\ts_endpgm")
    assert [(x.rule, x.found) for x in f] == [("H3", 4)]
    assert _audit("\tv_readfirstlane_b32 s4, v0\n\ts_nop 4\n\tglobal_load_dword v1, v2, s[4:5]\n\ts_endpgm") == []
    assert _audit("\ts_mov_b32 s4, s9\n\tglobal_load_dword v1, v2, s[4:5]\n\ts_endpgm") == []  # a scalar write is no such hazard
    assert _audit("\tv_readfirstlane_b32 s4, v0\n\ts_mov_b32 m0, s4\n\ts_endpgm") == []          # nor is a scalar read


def test_h4_lds_dma_and_m0():
    good = _inline("s_mov_b32 m0, s29", "s_nop 0", "global_load_lds_dwordx4 v1, s[40:41]")
    assert _audit(good + "\ts_endpgm") == []
    f = _audit(_inline("s_mov_b32 m0, s29", "global_load_lds_dwordx4 v1, s[40:41]") + "\ts_endpgm")
    assert [(x.rule, x.found, x.required) for x in f] == [("H4", 0, 1)]
    # m0 written in ANOTHER asm block: the compiler does not preserve it between statements
    f = _audit(_inline("s_mov_b32 m0, s29", "s_nop 0") + _inline("global_load_lds_dwordx4 v1, s[40:41]") + "\ts_endpgm")
    assert [x.rule for x in f] == ["H4"]
    # compiler code that touches m0 in a kernel with such a DMA
    f = _audit(good + "\ts_mov_b32 s3, m0\n\ts_endpgm")
    assert [x.rule for x in f] == ["H4"] and "s3, m0" in f[0].consumer
    assert _audit("\ts_mov_b32 m0, -1\n\ts_endpgm") == []                                       # no DMA: m0 is the compiler's


def test_h5_valu_write_to_inline_mfma_operand():
    f = _audit("\tv_mov_b32_e32 v4, v9\n" + _inline(MFMA) + "\ts_nop 15\n\ts_endpgm")
    assert [(x.rule, x.found, x.required) for x in f] == [("H5", 0, 2)]
    assert _audit("\tv_mov_b32_e32 v4, v9\n\ts_nop 1\n" + _inline(MFMA) + "\ts_nop 15\n\ts_endpgm") == []
    assert _audit("\tv_mov_b32_e32 v4, v9\n\t" + MFMA + "\n\ts_nop 15\n\ts_endpgm") == []        # a builtin MFMA: the compiler's job


def test_allow_list_flags_a_new_inline_instruction():
    f = _audit(_inline("v_add_f32_e32 v1, v2, v3") + "\ts_endpgm")
    assert [x.rule for x in f] == ["allow-list"]
    f = _audit(_inline("s_mov_b32 s3, s4") + "\ts_endpgm")                                      # s_mov_b32 is listed for m0 only
    assert [x.rule for x in f] == ["allow-list"]


def test_wait_states_and_register_parsing():
    ks = ih.parse(_kernel("\ts_nop 15\n\tv_fma_f32 v1, -v[2:3], |v4|, s[6:7] op_sel:[0,1]\n\ts_waitcnt vmcnt(0)\n\ts_endpgm"))
    assert [i.states for i in ks[0].ins] == [16, 1, 1, 1]
    assert ks[0].ins[1].regs == {("v", 1), ("v", 2), ("v", 3), ("v", 4), ("s", 6), ("s", 7)}
    assert ks[0].ins[1].writes == {("v", 1)}
    assert ks[0].ins[3].succ == [] and ks[0].ins[0].succ == [1]


def test_flags_come_from_the_build_script():
    hipcc, flags, units = ih.build_recipe()
    assert "--offload-arch=gfx950" in flags and "-O3" in flags and "-ffp-contract=off" in flags
    assert sorted(u + ".hip" for u in units) == sorted(f for f in os.listdir(ih.CSRC) if f.endswith(".hip"))


# ------------------------------------------------------------------------------------------------ the checker on the tree
_TREE = {}


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    """every unit of build.sh compiled to assembly (<= 16 jobs) and audited, once per session"""
    if not _TREE:
        t0 = time.time()
        files = ih.compile_tree(str(tmp_path_factory.mktemp("isa")))
        t1 = time.time()
        findings, stats, table = ih.audit(files, ih.H1_EXPECTED)
        _TREE.update(files=files, findings=findings, stats=stats, table=table, seconds=(t1 - t0, time.time() - t1))
        print(f"isa_hazards: compile {t1 - t0:.0f} s, scan {time.time() - t1:.0f} s")
    return _TREE


def test_h1_table_is_what_the_compiler_leaves_behind_its_own_mfmas(tree):
    """The requirement for inline MFMAs is measured, not remembered: the smallest distance over all BUILTIN sites per
    shape, attained often enough to be a rule (passes + 2), and — the checker's calibration — no builtin site anywhere
    below it: zero findings on compiler-scheduled code, or the checker is wrong."""
    table = tree["table"]
    print("measured H1 table (shape: states, sites attaining them):", table)
    assert {s: v[0] for s, v in table.items()} == {"16x16x4_f32": 10, "32x32x2_f32": 18}
    assert table["16x16x4_f32"][1] >= 50 and table["32x32x2_f32"][1] >= 4
    assert {s: v[0] for s, v in table.items()} == ih.H1_EXPECTED
    below = [(k, st["h1_min_builtin"]) for k, st in tree["stats"].items()
             if st["h1_min_builtin"] is not None and st["h1_min_builtin"] < 10]
    assert below == []


def test_no_hazard_in_any_kernel_of_the_library(tree):
    rep = ih.format_report(tree["findings"], tree["stats"], tree["table"])
    assert tree["findings"] == [], rep[rep.index("findings:"):]


def test_inline_mfma_sites_keep_the_measured_distance(tree):
    """every kernel with inline MFMAs: the nearest non-chain access to an accumulator is at or above the table"""
    with_inline = {k: st for k, st in tree["stats"].items() if st["mfma_inline"]}
    assert len(with_inline) >= 2                                   # mlp_layer_glds<true>, <false>
    assert all("mlp_layer_glds" in k[1] for k in with_inline), list(with_inline)
    for k, st in with_inline.items():
        assert st["h1_min_inline"] is not None and st["h1_min_inline"] >= 10, (k, st)


def test_inline_opcodes_are_exactly_the_allow_list(tree):
    seen = {}
    for name, path in tree["files"].items():
        for op, lst in ih.inline_opcodes(ih.parse(open(path).read())).items():
            seen.setdefault(op, []).extend(lst)
    assert set(seen) == set(ih.INLINE_ALLOWED), (sorted(set(seen) - set(ih.INLINE_ALLOWED)), sorted(set(ih.INLINE_ALLOWED) - set(seen)))
    for op, lst in seen.items():
        bad = [i for i in lst if not ih.INLINE_ALLOWED[op](i)]
        assert not bad, (op, bad[:3])


def test_every_lds_dma_has_its_own_m0_write_and_nothing_else_touches_m0(tree):
    n_dma = n_w = 0
    for k, st in tree["stats"].items():
        if st["m0_dma"]:
            assert st["m0_writes"] == st["m0_dma"] and st["m0_other"] == 0, (k, st)
            n_dma += st["m0_dma"]; n_w += st["m0_writes"]
    assert n_dma == n_w and n_dma >= 64            # the two engines: gemm_glds.h (cost matrix) and gemm_glds64.h (MLP layers)


def test_committed_report_matches_the_tree(tree):
    """profiles/isa_hazards.txt is the report of THIS tree (timings aside)"""
    want = [l for l in ih.format_report(tree["findings"], tree["stats"], tree["table"]).split("\n") if not l.startswith("# compile")]
    have = [l for l in open(os.path.join(ROOT, "profiles", "isa_hazards.txt")).read().split("\n") if not l.startswith("# compile")]
    assert have == want, "regenerate: python tools/isa_hazards.py --out profiles/isa_hazards.txt"
