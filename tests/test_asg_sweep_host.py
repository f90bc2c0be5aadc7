"""No GPU: the code object of the lean sweep kernel (csrc/assign.hip: asg_sweep), from the compiler's own bookkeeping as
tools/isa_report.py reads it.  The kernel exists to share a CU with dense workgroups: eight waves per SIMD (at most 64
VGPRs), no scratch, no spills, at most 8 KiB of LDS."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import isa_report  # noqa: E402


def test_asg_sweep_fits_beside_dense_workgroups():
    rows = isa_report.report(os.path.join(isa_report.CSRC, "assign.hip"))
    sweep = [r for r in rows if r["kernel"].startswith("asg_sweep(")]
    assert len(sweep) == 1, [r["kernel"] for r in rows]
    r = sweep[0]
    print(r)
    assert r["vgpr"] <= 64 and r["agpr"] == 0, r
    assert r["scratch"] == 0, r
    assert r["spill"] == 0, r
    assert r["lds"] <= 8192, r
    # the kernel it relieves is still the 16-wave one
    assert any(x["kernel"].startswith("asg_step(") for x in rows)
