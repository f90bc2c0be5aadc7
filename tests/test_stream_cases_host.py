"""CPU: the case table of tests/stream_cases.py covers every entry of include/cfm_gfx950.h that takes a `stream`."""
import os
import re

import stream_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _prototypes():
    """{entry: parameter text} of every prototype in the header (comments stripped), as tests/test_abi_exports.py reads it."""
    src = open(os.path.join(ROOT, "include", "cfm_gfx950.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return {m.group(1): m.group(2) for m in re.finditer(r"\b(cfm_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", src)}


def _stream_taking():
    return sorted(n for n, params in _prototypes().items() if re.search(r"void\s*\*+\s*stream\b", params))


def test_header_parse_finds_the_known_entries():
    names = _stream_taking()
    protos = _prototypes()
    assert len(protos) >= 63 and len(names) >= 55
    for must in ("cfm_sqeuclid_cost_f32", "cfm_assign_exact_f32", "cfm_ode_adaptive_rec_mlp_f32", "cfm_stream_destroy",
                 "cfm_stream_create_cu_mask", "cfm_action_matching_grad_f32", "cfm_adam_step_f32"):
        assert must in names
    for host_only in ("cfm_abi_version", "cfm_workspace_bytes", "cfm_ode_fixed_grad_available", "cfm_ode_adaptive_grad_available"):
        assert host_only in protos and host_only not in names


def test_every_stream_taking_entry_has_a_case_or_a_stated_exemption():
    names = set(_stream_taking())
    covered, exempt = set(sc.CASES), set(sc.EXEMPT)
    assert not covered & exempt
    assert names - covered - exempt == set(), sorted(names - covered - exempt)
    assert (covered | exempt) - names == set(), sorted((covered | exempt) - names)


def test_exemptions_are_only_the_entries_that_enqueue_nothing():
    assert set(sc.EXEMPT) <= sc.EXEMPT_ALLOWED
    assert sc.EXEMPT_ALLOWED == {"cfm_stream_create_cu_mask", "cfm_stream_destroy", "cfm_ode_fixed_grad_available",
                                 "cfm_ode_adaptive_grad_available"}
    for name, why in sc.EXEMPT.items():
        assert isinstance(why, str) and len(why.strip()) > 10 and "\n" not in why, name


def test_cases_are_well_formed():
    ids = [c.id for c in sc.all_cases()]
    assert len(ids) == len(set(ids))
    for entry, cases in sc.CASES.items():
        assert cases
        for c in cases:
            assert c.entry == entry and callable(c.make) and callable(c.op)
            assert c.syncs == (entry in sc.SYNCING)
    assert sc.SYNCING <= set(sc.CASES)
    assert set(sc.HOST_DATA) <= set(sc.CASES) and not set(sc.HOST_DATA) & sc.SYNCING
    for entry, name in sc.HOST_DATA_EXTRA:
        assert entry in sc.HOST_DATA and name in [c.name for c in sc.CASES[entry][1:]]


def test_host_decoys_are_valid_grids_and_records():
    """The host arrays of the decoy sets: strictly monotone grids of the true grid's direction, finite step records with
    positive steps (a decoy must give a wrong answer, never a fault)."""
    import numpy as np
    for rev in (False, True):
        a, b = sc._grid(0, 9, rev), sc._grid(1, 9, rev)
        assert a.dtype == b.dtype == np.float32 and a.shape == b.shape and not np.array_equal(a, b)
        assert np.all(np.diff(a) * np.diff(b) > 0)
    for srk in (False, True):
        a, b = sc._sde_records(0, srk), sc._sde_records(1, srk)
        assert a.shape == b.shape == ((32 if srk else 16) * sc.SDE_STEPS,) and not np.array_equal(a, b)
        f = b.view(np.float32).reshape(sc.SDE_STEPS, -1)
        assert np.isfinite(f[:, :6 if srk else 3]).all() and (f[:, 3 if srk else 1] > 0).all()
        flags = b.view(np.int32).reshape(sc.SDE_STEPS, -1)[:, 6 if srk else 3]
        assert flags.sum() == sc.SDE_OUT and set(flags.tolist()) <= {0, 1}
