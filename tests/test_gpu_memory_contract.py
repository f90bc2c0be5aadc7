"""GPU (-m gpu): the memory contract of include/cfm_gfx950.h's conventions, for every entry of the case table of
tests/stream_cases.py and for the edge shapes of FOOTPRINT_EXTRA below:

    the contents of `ws` and of the output buffers on entry are arbitrary; outputs are written whole; nothing outside the
    outputs and the first cfm_workspace_bytes bytes of `ws` is written; inputs are not modified (except in place, where
    the header says so).

Protocol, per case.  A plain run on the true inputs (seed 0) gives the reference: the entry's own result as every other
test of the suite sees it (its values are pinned there).  Then four runs inside tests/footprint_util.py's harness, each on a
private, guarded clone of the inputs and with this thread's workspace cache cleared (so the workspace, too, is carved inside the
harness and gets its guards): the true inputs on buffers filled with 0x00, with 0xFF, the decoy (seed 1) on 0x00, and the
true inputs on what that decoy run left in every buffer ("stale").  Every guarded run of the true inputs must give the
reference's return code and host results; outputs bit for bit (rtol None) or within the case's own atomics-order
tolerance; untouched guards around every output, gradient table and workspace; and bit-identical inputs (those that are not
outputs themselves: the in-place entries return their input, recognised by data_ptr).  A case that DECLINES (a documented
CFM_EINVAL before any work) must leave every buffer exactly as the harness filled it.

Read before run: the workspace words an entry waits on or indexes by, and where it initialises them (all on `stream`):

  entry                                  words waited on / indexed by                     initialised by
  -------------------------------------  -----------------------------------------------  -----------------------------------------
  adaptive ODE / CNF / gradient-field    3 x 1024 fp64 arrival slots of the grid          ode_dopri5_small: hipMemsetAsync(partial,
  solves, one-launch form (ode.hip,      rendezvous (sm_grid_allsum polls them for a      0xFF, 3 * SM_MAXGRID * 8) before the
  ode_small_dopri)                       non-negative value); SmState (t, dt, ckpt, par)  launch; SmState by hipMemcpyAsync from the
                                                                                          host; the next row re-armed by its owner
  adaptive solves, layer form            red[0..7] (fp64 norm sums, atomics)              hipMemsetAsync(red, 0, ..) before each sum
  cfm_assign_exact(_batch)_f32,          AsgState.mode / error (every kernel's guard),    asg_init (state block as kernel argument;
  chip-wide machine (assign.hip)         arrive_sub[256] arrival words                    zeroes arrive_sub) before the first step
    asg_auction (the loop at             auc: async_word, async_claim, async_done,        the INITRED control step, which alone sets
    assign.hip:1781)                     bidcnt, ctl[2]; key[n], bidcol[n],               mode = AUCTION (asg_auction returns in any
                                         grp_ticket[n]                                    other mode); key / bidcol / grp_ticket by
                                                                                          the UMIN0 sweep (wide_umin0)
    candidate lists cl[n][64], cT, pb    column indices the list solver indexes by        asg_build writes every row's list before
                                                                                          asg_solve (MODE_SOLVER is set behind it)
  one-workgroup solver (assign_small.h,  actl / fm / key / arow ... : LDS only            the kernel's own prologue; the workspace
  the loop at :395)                                                                       holds only the status block it writes whole
  cfm_transport_exact_f32                ticket (last-workgroup-done), colsum, cmax       hipMemsetAsync(colsum, 0, align(4 C) + 256)
                                                                                          covers colsum and the cmax / ticket block
  cfm_unbalanced_sinkhorn_f64,           UbState.tiles_done (ticket), done, fold, mx      ub_state_init, the first launch
  cfm_partial_entropic_f64
  cfm_sinkhorn_log(_points)_f32          SkState (iteration, done flag), u, v             sk_init, the first launch
  fixed-step solves, SDE, gradients      the device copy of t_span / the step records     hipMemcpyAsync from the host, first

The harness cannot see a store further than its guard (4096 bytes) from a buffer, nor an out-of-bounds read."""
import functools
import time

import numpy as np
import pytest
import torch

import footprint_util as fu
import stream_cases as sc
from exact_util import _first_diff
from footprint_util import GUARD, guarded

pytestmark = pytest.mark.gpu

EINVAL = -1


@pytest.fixture(scope="module")
def dev():
    import cfm_amd  # noqa: F401
    from cfm_amd import _lib
    _lib.load()
    d = torch.device("cuda:0")
    torch.cuda.set_device(d)
    return d


# ------------------------------------------------------------------------------------------------ edge shapes
FOOTPRINT_EXTRA = []


def extra(entry, name, make, op, prep=None, declines=False, note=""):
    c = sc.Case(entry, "fp-" + name, make, op, prep, note)
    c.declines = declines
    FOOTPRINT_EXTRA.append(c)


# -- small-field kernels (64-row tiles): one partial workgroup, exactly one, one row into the second; d = 1 and d = 63
#    (d + 1 <= 64 is the envelope's edge); n_t = 2.  B = 1, d = 1 has B d < n_t: the plain fixed-step entry then takes its
#    layer driver, which is as much that entry as the one-launch kernel.
TILE_SHAPES = [(B, d) for B in (1, 64, 65) for d in (1, 63)]
CORNERS = [(1, 1), (65, 63)]
for B, d in TILE_SHAPES:
    s = f"B{B}-d{d}"
    extra("cfm_ode_fixed_mlp_f32", f"rk4-{s}", sc._mk_ode(B=B, d=d, n_t=2), sc._op_fixed("cfm_ode_fixed_mlp_f32", 2))
    extra("cfm_ode_euler_cnf_mlp_f32", f"exact-{s}", sc._mk_ode(B=B, d=d, n_t=2, aug=1),
          sc._op_cnf_fixed("cfm_ode_euler_cnf_mlp_f32", 0, 0))
    extra("cfm_ode_fixed_cnf_mlp_f32", f"hutch-rk4-{s}", sc._mk_ode(B=B, d=d, n_t=2, aug=1, eps=True),
          sc._op_cnf_fixed("cfm_ode_fixed_cnf_mlp_f32", 1, 2))
    # (the SDE workspace at exactly the sizeof(record) * n_steps bytes the header asks for)
    extra("cfm_sde_em_mlp_f32", s, sc._mk_sde(False, B=B, d=d), sc._op_sde(False, slack=0))
    extra("cfm_sde_srk_mlp_f32", s, sc._mk_sde(True, B=B, d=d), sc._op_sde(True, slack=0))
    extra("cfm_ode_fixed_grad_f32", f"rk4-{s}", sc._mk_grad(0, B=B, d=d, n_t=2), sc._op_solve_grad("cfm_ode_fixed_grad_f32"))
    extra("cfm_cnf_euler_grad_f32", f"exact-{s}", sc._mk_grad(1, B=B, d=d, n_t=2), sc._op_solve_grad("cfm_cnf_euler_grad_f32"))
    extra("cfm_cnf_reg_euler_grad_f32", f"mask3-{s}", sc._mk_grad(3, jac=True, B=B, d=d, n_t=2),
          sc._op_solve_grad("cfm_cnf_reg_euler_grad_f32"))
for B, d in CORNERS:
    s = f"B{B}-d{d}"
    extra("cfm_ode_euler_mlp_f32", s, sc._mk_ode(B=B, d=d, n_t=2), sc._op_fixed("cfm_ode_euler_mlp_f32", 0))
    extra("cfm_ode_fixed_gradmlp_f32", f"midpoint-{s}", sc._mk_ode(B=B, d=d, n_t=2, out_dim=1),
          sc._op_fixed("cfm_ode_fixed_gradmlp_f32", 1))
    extra("cfm_ode_fixed_pair_mlp_f32", f"rk4-{s}", sc._mk_ode(B=B, d=d, n_t=2, pair=True), sc._op_pair)
    extra("cfm_ode_fixed_cnf_gradmlp_f32", f"euler-{s}", sc._mk_ode(B=B, d=d, n_t=2, aug=1, out_dim=1),
          sc._op_cnf_fixed("cfm_ode_fixed_cnf_gradmlp_f32", 0, 0))
    extra("cfm_ode_euler_cnf_reg_mlp_f32", s, sc._mk_ode(B=B, d=d, n_t=2, aug=3), sc._op_cnf_reg)
    extra("cfm_ode_adaptive_mlp_f32", f"tsit5-{s}", sc._mk_ode(B=B, d=d, n_t=2), sc._op_adaptive("cfm_ode_adaptive_mlp_f32", 1))
    extra("cfm_ode_adaptive_cnf_mlp_f32", f"exact-dopri5-{s}", sc._mk_ode(B=B, d=d, n_t=2, aug=1),
          sc._op_cnf_adaptive("cfm_ode_adaptive_cnf_mlp_f32", 0, 0))
extra("cfm_ode_adaptive_gradmlp_f32", "tsit5-B65-d63", sc._mk_ode(B=65, d=63, n_t=2, out_dim=1),
      sc._op_adaptive("cfm_ode_adaptive_gradmlp_f32", 1))
# -- n_t = 1: the header defines zero parameter gradients
for entry, aug, jac in (("cfm_ode_fixed_grad_f32", 0, False), ("cfm_cnf_euler_grad_f32", 1, False),
                        ("cfm_cnf_reg_euler_grad_f32", 3, True)):
    extra(entry, "nt1-B65-d2", sc._mk_grad(aug, jac=jac, B=65, n_t=1), sc._op_solve_grad(entry))

# -- the t_span copy's room: B D floats (adaptive, one buffer) or 3 B D (fixed CNF, three buffers).  Just inside the call
#    runs with the copy ending on the buffer's last float; just outside the plain entries take the layer driver and the
#    others DECLINE (CFM_EINVAL before any work): outputs, workspace and guards stay as they were.
extra("cfm_ode_adaptive_mlp_f32", "dopri5-Bd-eq-nt", sc._mk_ode(B=1, d=2, n_t=2), sc._op_adaptive("cfm_ode_adaptive_mlp_f32", 0))
extra("cfm_ode_adaptive_mlp_f32", "dopri5-Bd-lt-nt-layers", sc._mk_ode(B=1, d=2, n_t=3),
      sc._op_adaptive("cfm_ode_adaptive_mlp_f32", 0))
extra("cfm_ode_fixed_mlp_f32", "rk4-Bd-eq-nt", sc._mk_ode(B=1, d=2, n_t=2), sc._op_fixed("cfm_ode_fixed_mlp_f32", 2))
extra("cfm_ode_fixed_mlp_f32", "rk4-Bd-lt-nt-layers", sc._mk_ode(B=1, d=2, n_t=3), sc._op_fixed("cfm_ode_fixed_mlp_f32", 2))
extra("cfm_ode_adaptive_rec_mlp_f32", "tsit5-Bd-eq-nt", sc._mk_ode(B=1, d=2, n_t=2), sc._op_rec)
extra("cfm_ode_adaptive_rec_mlp_f32", "tsit5-Bd-lt-nt-declines", sc._mk_ode(B=1, d=2, n_t=3), sc._op_rec, declines=True)
extra("cfm_ode_adaptive_gradmlp_f32", "tsit5-Bd-eq-nt", sc._mk_ode(B=1, d=2, n_t=2, out_dim=1),
      sc._op_adaptive("cfm_ode_adaptive_gradmlp_f32", 1))
extra("cfm_ode_adaptive_gradmlp_f32", "tsit5-Bd-lt-nt-declines", sc._mk_ode(B=1, d=1, n_t=2, out_dim=1),
      sc._op_adaptive("cfm_ode_adaptive_gradmlp_f32", 1), declines=True)
extra("cfm_ode_adaptive_cnf_mlp_f32", "exact-BD-lt-nt-declines", sc._mk_ode(B=1, d=1, n_t=3, aug=1),
      sc._op_cnf_adaptive("cfm_ode_adaptive_cnf_mlp_f32", 0, 0), declines=True)
extra("cfm_ode_fixed_cnf_mlp_f32", "exact-nt-eq-3BD", sc._mk_ode(B=1, d=1, n_t=6, aug=1),
      sc._op_cnf_fixed("cfm_ode_fixed_cnf_mlp_f32", 0, 1))
extra("cfm_ode_fixed_cnf_mlp_f32", "exact-nt-gt-3BD-declines", sc._mk_ode(B=1, d=1, n_t=7, aug=1),
      sc._op_cnf_fixed("cfm_ode_fixed_cnf_mlp_f32", 0, 1), declines=True)
extra("cfm_ode_fixed_cnf_gradmlp_f32", "nt-eq-3BD", sc._mk_ode(B=1, d=1, n_t=6, aug=1, out_dim=1),
      sc._op_cnf_fixed("cfm_ode_fixed_cnf_gradmlp_f32", 0, 1))
extra("cfm_ode_fixed_cnf_gradmlp_f32", "nt-gt-3BD-declines", sc._mk_ode(B=1, d=1, n_t=7, aug=1, out_dim=1),
      sc._op_cnf_fixed("cfm_ode_fixed_cnf_gradmlp_f32", 0, 1), declines=True)
extra("cfm_ode_euler_cnf_reg_mlp_f32", "nt-eq-3BD", sc._mk_ode(B=1, d=1, n_t=12, aug=3), sc._op_cnf_reg)
extra("cfm_ode_euler_cnf_reg_mlp_f32", "nt-gt-3BD-declines", sc._mk_ode(B=1, d=1, n_t=13, aug=3), sc._op_cnf_reg, declines=True)
# -- the first size past the register-resident form (8192 rows on MI355X): x and k_1 travel through the parity buffers
extra("cfm_ode_adaptive_mlp_f32", "tsit5-B8193", sc._mk_ode(B=8193), sc._op_adaptive("cfm_ode_adaptive_mlp_f32", 1))


# -- the recording solve with max_steps = the accepted count of this very solve: log and ysteps are exactly full, the guard
#    sits directly behind the last record.  (The decoy runs with the true problem's count too, so that the buffers have the
#    same sizes; it may stop on a full log, which is as good a source of stale bytes.)
def _mk_rec_full(seed, dev):
    probe = sc._mk_ode(B=65)(0, dev)
    _, host = sc._op_rec(probe)
    torch.cuda.synchronize()
    assert host[0] == 0 and 0 < host[3] < sc.MAX_STEPS, host
    inp = sc._mk_ode(B=65)(seed, dev)
    inp["_max_steps"] = host[3]
    return inp


extra("cfm_ode_adaptive_rec_mlp_f32", "tsit5-log-exactly-full", _mk_rec_full, sc._op_rec)

# -- Sinkhorn family, kernel-space solvers, transport: thin, odd and tile-sized; 33 x 257 is one past both steps of the
#    strip count that sizes the Sinkhorn and unbalanced workspaces (32 rows per strip, 256 columns per tile); the transport
#    carve rounds 4 R C, 8 R, 8 C and 4 C up to 256 bytes: 33 x 65 and 65 x 33 (the transposed form) sit one past a step of each
SK_SHAPES = [(1, 200), (300, 1), (257, 129), (128, 128), (33, 257)]
for b0, b1 in SK_SHAPES:
    s = f"{b0}x{b1}"
    mk = functools.partial(sc._mk_cost, b0=b0, b1=b1)
    extra("cfm_sinkhorn_log_f32", s, mk, sc._op_sinkhorn)
    extra("cfm_sinkhorn_log_points_f32", s, sc._mk_clouds(b0, b1, 2), sc._op_sinkhorn_points)
    extra("cfm_sinkhorn_potentials_f64", s, sc._mk_solved(b0=b0, b1=b1), sc._op_potentials)
    extra("cfm_sinkhorn_plan_f64", s, sc._mk_solved(b0=b0, b1=b1), sc._op_plan)
    extra("cfm_sinkhorn_cost_f64", s, sc._mk_solved(b0=b0, b1=b1), sc._op_sk_cost)
    extra("cfm_plan_sample_dense", s, sc._mk_solved(sc.NDRAW, b0=b0, b1=b1), sc._op_sample_dense)
    extra("cfm_plan_sample_rows_dense", s, sc._mk_solved(sc.NDRAW, rows=True, b0=b0, b1=b1), sc._op_rows_dense)
    extra("cfm_unbalanced_sinkhorn_f64", s, mk, sc._op_kernel_space("ub"))
    extra("cfm_partial_entropic_f64", s, mk, sc._op_kernel_space("partial"))
for b0, b1 in SK_SHAPES + [(33, 65), (65, 33)]:
    extra("cfm_transport_exact_f32", f"{b0}x{b1}", functools.partial(sc._mk_cost, b0=b0, b1=b1), sc._op_transport)

# -- the cost kernels: a single entry, a single row, and the matrix-core form at its smallest shape (d = 64, B = 256: whole
#    tiles) and one past it each way
for b0, b1, d in ((1, 1, 1), (1, 200, 3), (300, 1, 3)):
    extra("cfm_sqeuclid_cost_f32", f"{b0}x{b1}-d{d}", sc._mk_clouds(b0, b1, d), sc._op_cost(False))
for b0, b1, d in ((256, 256, 64), (257, 257, 65)):
    extra("cfm_sqeuclid_cost_ws_f32", f"gram-{b0}x{b1}-d{d}", sc._mk_clouds(b0, b1, d), sc._op_cost(True))

# -- assignment: the trivial size, the smallest real one, the one-workgroup solver's last size (257, the first of the
#    chip-wide machine, is the table's); a batch of three at n = 65
for n in (1, 2, 256):
    extra("cfm_assign_exact_f32", f"n{n}", sc._mk_square(1, n), sc._op_assign)
extra("cfm_assign_exact_batch_f32", "3-of-n65", sc._mk_square(3, 65), sc._op_assign_batch)

# -- MLP forward, forward-for-training, backward and the fused steps around the 128-row tile; the two-net steps take two
#    workspaces back to back, the guard stands behind the second
for B in (1, 127, 129):
    extra("cfm_mlp_forward_f32", f"B{B}", sc._mk_fwd(B, 5, 64), sc._op_fwd)
    extra("cfm_mlp_forward_train_f32", f"B{B}", functools.partial(sc._mk_fwd_train, B=B), sc._op_fwd_train)
    extra("cfm_mlp_backward_f32", f"B{B}", functools.partial(sc._mk_backward, B=B), sc._op_backward)
    extra("cfm_mlp_regression_step_f32", f"B{B}", sc._mk_step("reg", B), sc._op_regression)
    extra("cfm_mlp_sf2m_step_f32", f"B{B}", sc._mk_step("two", B), sc._op_sf2m)
    extra("cfm_mlp_dsbm_step_f32", f"B{B}", sc._mk_step("two", B), sc._op_dsbm_step)

extra("cfm_adam_step_f32", "numel-1-255-256-257", functools.partial(sc._mk_adam, numels=(1, 255, 256, 257)), sc._op_adam,
      prep=sc._prep_adam)

for B, d in ((1, 5), (257, 1), (1, 1)):
    s = f"B{B}-d{d}"
    extra("cfm_sample_xt_ut_f32", s, sc._mk_xt("icfm", B, d), sc._op_xt)
    extra("cfm_sample_xt_ut_sched_f32", s, sc._mk_xt("sched", B, d), sc._op_xt_sched)
    extra("cfm_sample_dsbm_f32", s, sc._mk_xt("sched", B, d), sc._op_dsbm_sample)
    extra("cfm_gather_rows", s, sc._mk_xt("icfm", B, d), sc._op_gather)
    extra("cfm_traj_xt_ut_f32", s, functools.partial(sc._mk_traj, B=B, d=d), sc._op_traj)


# ------------------------------------------------------------------------------------------------ protocol
def _clone(inp):
    return {k: (v.clone() if torch.is_tensor(v) else v.copy() if isinstance(v, np.ndarray) else v) for k, v in inp.items()}


def _decoy_on_true_host_arguments(decoy, true):
    """Device buffers of the decoy, host arguments (grids, records, scalars) of the true set."""
    out = _clone(true)
    for k, v in decoy.items():
        if torch.is_tensor(v) and not k.startswith("_"):
            out[k] = v.clone()
    return out


def _bits(t):
    return t.contiguous().view(-1).view(torch.uint8)


def _tensors(inp):
    return {k: v for k, v in inp.items() if torch.is_tensor(v)}


def _plain_run(case, inp):
    c = _clone(inp)
    if case.prep:
        case.prep(c)
    outs, host = case.op(c)
    torch.cuda.synchronize()
    return outs, host, c


_ACTIVE = [None]          # the harness of the guarded run in progress (the self-test's faulty op looks its buffer up there)


def _guarded_run(case, inp, fill, dev, op=None, prev=None):
    """(harness, outs, host, the working copy of the inputs, its pristine copy)"""
    fu.clear_workspace_cache()
    g = guarded(fill, dev)
    if prev is not None:
        g.stale_from(prev)
    try:
        with g:
            _ACTIVE[0] = g
            # the working copy of every device input stands between guards too: an in-place entry has no other buffer
            c = {k: (g.copy_of(v) if torch.is_tensor(v) and v.numel() else v) for k, v in _clone(inp).items()}
            if case.prep:
                case.prep(c)
            pristine = {k: v.clone() for k, v in _tensors(c).items()}
            torch.cuda.synchronize()
            outs, host = (op or case.op)(c)
            torch.cuda.synchronize()
    finally:
        _ACTIVE[0] = None
        fu.clear_workspace_cache()
    return g, outs, host, c, pristine


def _violations(case, what, run, ref_outs, ref_host):
    """Every way the guarded run `run` of the TRUE inputs breaks the contract, as strings."""
    g, outs, host, c, pristine = run
    bad = []
    if host != ref_host:
        bad.append(f"{what}: host results {host}, reference {ref_host}")
    for r in g.check():
        bad.append(f"{what}: footprint: allocation {r[0]} {r[1]} {r[2]}: {r[5]} bytes of the {r[3]} guard changed, first at "
                   f"offset {r[4]}")
    if getattr(case, "declines", False):
        if not g.untouched():
            bad.append(f"{what}: a declining call wrote to an output or to the workspace")
    else:
        if [o[0] for o in outs] != [o[0] for o in ref_outs]:
            bad.append(f"{what}: outputs {[o[0] for o in outs]}")
        for (name, a, rtol), (_, b, _) in zip(outs, ref_outs):
            if rtol is None:
                ok = a.shape == b.shape and torch.equal(_bits(a), _bits(b))
            else:
                ok = a.shape == b.shape and torch.allclose(a.double(), b.double(), rtol=rtol, atol=0.0)
            if not ok:
                bad.append(f"{what}: output {name} (rtol {rtol}): {_first_diff(a, b)}")
    out_ptrs = {t.data_ptr() for _, t, _ in outs}
    for k, v in _tensors(c).items():
        if v.data_ptr() not in out_ptrs and not torch.equal(_bits(v), _bits(pristine[k])):
            bad.append(f"{what}: input {k} was modified: {_first_diff(v, pristine[k])}")
    return bad


RAN = {}                  # case id -> fills the true inputs ran under


def _contract(case, dev, op=None):
    """The whole protocol on one case; returns the violations of the three guarded runs of the true inputs."""
    true, decoy = case.make(0, dev), case.make(1, dev)
    torch.cuda.synchronize()
    ref_outs, ref_host, _keep = _plain_run(case, true)
    if ref_host and ref_host[0] > 0:
        raise RuntimeError(f"hipError_t {ref_host[0]} from {case.entry}")
    if getattr(case, "declines", False):
        assert ref_host and ref_host[0] == EINVAL, (case.id, "meant to decline", ref_host)
    elif ref_host:
        assert ref_host[0] == 0, (case.id, "the reference run failed: the inputs are not valid", ref_host)
    bad = []
    for fill in ("00", "ff"):
        run = _guarded_run(case, true, fill, dev, op)
        bad += _violations(case, f"fill {fill}", run, ref_outs, ref_host)
        RAN.setdefault(case.id, set()).add(fill)
    dec = _guarded_run(case, _decoy_on_true_host_arguments(decoy, true), "00", dev, op)
    for r in dec[0].check():
        bad.append(f"decoy run: footprint: allocation {r[0]} {r[1]} {r[2]} {r[3]} guard at offset {r[4]}")
    run = _guarded_run(case, true, "stale", dev, op, prev=dec[0])
    bad += _violations(case, "fill stale", run, ref_outs, ref_host)
    RAN[case.id].add("stale")
    return bad


ALL = sc.all_cases() + FOOTPRINT_EXTRA


def test_the_lists_are_well_formed():
    ids = [c.id for c in ALL]
    assert len(ids) == len(set(ids))
    assert {c.entry for c in FOOTPRINT_EXTRA} <= set(sc.CASES)
    assert all(c in ALL for cs in sc.CASES.values() for c in cs)


@pytest.mark.parametrize("case", ALL, ids=[c.id for c in ALL])
def test_entry_on_poisoned_guarded_buffers(dev, case):
    t0 = time.perf_counter()
    try:
        bad = _contract(case, dev)
    except RuntimeError as e:
        if "HIP error" in str(e) or "hipError" in str(e):        # the device context is gone: nothing after this means anything
            pytest.exit(f"{case.id}: {e}", returncode=3)
        raise
    print(f"\n[memory contract] {case.id}: {1e3 * (time.perf_counter() - t0):.0f} ms, {len(bad)} violations")
    assert not bad, "\n".join([case.id] + bad)


def test_the_protocol_reports_an_unwritten_last_element(dev):
    """The harness on itself, on a real entry: the op is wrapped so that the LAST element of its output is as if the kernel
    had never stored it (put back, with torch ops after the entry returned, to what the buffer held before the call).  Each
    of the three fills must report that output, and nothing else."""
    case = sc.CASES["cfm_sqeuclid_cost_f32"][0]
    assert _contract(case, dev) == []

    def skips_the_last_element(inp):
        outs, host = case.op(inp)
        g, M = _ACTIVE[0], outs[0][1]
        k = [r.arena.data_ptr() + GUARD for r in g.records].index(M.data_ptr())
        last = g.records[k].body[-M.element_size():]
        if g.fill == "stale":
            last.copy_(g._prev.records[k].body[-M.element_size():])
        else:
            last.fill_(0x00 if g.fill == "00" else 0xFF)
        return outs, host
    bad = _contract(case, dev, op=skips_the_last_element)
    print("\n[memory contract] reported:\n" + "\n".join(bad))
    assert len(bad) == 3 and all("output M" in b and f"fill {f}" in b for b, f in zip(bad, ("00", "ff", "stale"))), bad
    assert all("1 of 60000 differ; first at (299, 199)" in b for b in bad), bad


def test_every_case_ran_under_all_three_fills(request):
    """Last in the module: every case of the table and of FOOTPRINT_EXTRA that this session selected has run the true inputs
    under "00", "ff" and "stale", and a full run selects them all."""
    selected = {i.callspec.params["case"].id for i in request.session.items
                if i.name.startswith("test_entry_on_poisoned_guarded_buffers[") and hasattr(i, "callspec")}
    assert selected, "no case of the memory contract was selected"
    for cid in sorted(selected):
        assert RAN.get(cid) == {"00", "ff", "stale"}, (cid, RAN.get(cid))
    if len(selected) == len(ALL):
        assert {c.entry for c in ALL} == set(sc.CASES)
