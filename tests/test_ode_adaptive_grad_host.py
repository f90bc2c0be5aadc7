"""CPU: the gradient of the adaptive solves (dopri5, tsit5).  The float64 replay of a step log
(tests/ode_adaptive_grad_restate.py) is pinned by the reverse sweep written out without autograd (what the kernel runs,
DESIGN.md 4.17); then AdaptiveDifferentiableNeuralODE's generic path is pinned against both on its own step log, the
log's invariants are checked, and the C ABI carries the new entries."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import cfm_amd
import cnf_restate as cr
import ode_adaptive_grad_restate as ar
from cfm_amd import _lib
from cfm_amd.utils import torch_wrapper

UP = np.array([0.0, 0.07, 0.3, 0.35, 0.81, 1.0], np.float32)                      # increasing, non-uniform
DOWN = np.array([1.0, 0.9, 0.55, 0.5, 0.12, 0.0], np.float32)                     # decreasing, non-uniform
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "cfm_gfx950.h")
TOL = dict(atol=1e-5, rtol=1e-5)      # tight enough that the steps are shorter than the grid's intervals


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


def _generic(Ws, bs, xa, ts, solver, G, **kw):
    """The generic path in float64: (node, trajectory, [8 parameter gradients, dx]) as numpy."""
    m = cr.make_mlp(Ws, bs, dtype=torch.float64)
    node = cfm_amd.AdaptiveDifferentiableNeuralODE(torch_wrapper(m), solver=solver, **{**TOL, **kw})
    x = torch.tensor(xa, requires_grad=True)
    t_eval, traj = node(x, torch.tensor(ts))
    assert node.last_path == "generic" and traj.dtype == torch.float64 and tuple(traj.shape) == (len(ts),) + xa.shape
    ps = [p for l in m._linears() for p in (l.weight, l.bias)]
    got = torch.autograd.grad((traj * torch.tensor(G)).sum(), ps + [x])
    return node, traj.detach().numpy(), [q.numpy() for q in got]


def _case(ts, seed=2):
    d, w, B = 3, (33, 64, 48), 6
    Ws, bs = cr.mlp_params(d, w, seed=seed)
    g = np.random.default_rng(11)
    return Ws, bs, g.normal(size=(B, d)), g.normal(size=(len(ts), B, d))


@pytest.mark.parametrize("ts", [DOWN, UP], ids=["down", "up"])
@pytest.mark.parametrize("solver", ar.SOLVERS)
def test_generic_path_equals_the_replay_of_its_own_log(solver, ts):
    """Trajectory and gradients of the generic path against the float64 replay of its step log, by autograd and by the
    written-out reverse sweep.  Bound: test_ode_grad_host.py's 1e-12 of max|g| per tensor."""
    Ws, bs, xa, G = _case(ts)
    tsign = 1.0 if ts[1] > ts[0] else -1.0
    node, traj, got = _generic(Ws, bs, xa, ts, solver, G)
    log = node.step_log
    assert log.dtype == torch.float64 and tuple(log.shape) == (node.n_accepted, 4) and node.n_accepted >= len(ts) - 1
    assert node.n_steps >= node.n_accepted and node.nfe == 2 + 6 * node.n_steps
    traj64, gp64, gx64 = ar.grads_for_upstream(Ws, bs, xa, log.numpy(), G, solver, tsign)
    gp, gx = ar.reverse_sweep(Ws, bs, xa, log.numpy(), G, solver, tsign)
    print(f"{solver}: {node.n_accepted} accepted of {node.n_steps}; trajectory {_rel(traj, traj64):.2e}")
    assert _rel(traj, traj64) <= 1e-12
    for n, (a, b, c) in enumerate(zip(got, gp64 + [gx64], gp + [gx])):
        print(f"{solver} tensor {n}: autograd {_rel(a, b):.2e} sweep {_rel(a, c):.2e}")
        assert _rel(a, b) <= 1e-12 and _rel(a, c) <= 1e-12


@pytest.mark.parametrize("ts", [DOWN, UP], ids=["down", "up"])
@pytest.mark.parametrize("solver", ar.SOLVERS)
def test_step_log_invariants(solver, ts):
    Ws, bs, xa, G = _case(ts)
    tsign = 1.0 if ts[1] > ts[0] else -1.0
    node, _, _ = _generic(Ws, bs, xa, ts, solver, G)
    log = node.step_log.numpy()
    t, dt, tk1, out = log.T
    s = (tsign * ts).astype(np.float32)                       # the grid in solver time
    assert np.all(np.diff(t) > 0) and np.all(dt > 0)          # t increasing
    assert [int(o) for o in out if o >= 0] == list(range(1, len(ts)))      # out enumerates 1 .. n_t - 1 in order
    assert np.all((out == -1) | (out >= 1)) and out[-1] == len(ts) - 1
    assert tk1[0] == t[0] == s[0]
    # the step ends sum to the grid: a landing step ends ON its point (its successor starts there, bit for bit), any
    # other step ends at t + dt in float32
    for n in range(len(t)):
        end = s[int(out[n])] if out[n] >= 0 else np.float32(np.float32(t[n]) + np.float32(dt[n]))
        if n + 1 < len(t):
            assert t[n + 1] == end
            assert tk1[n + 1] == np.float32(np.float32(t[n]) + np.float32(dt[n]))     # k_7's time, not the landing point
        else:
            assert end == s[-1]
        if out[n] >= 0:
            assert abs((t[n] + dt[n]) - end) <= 2 * np.spacing(np.float32(abs(end)))
    assert any(o >= 0 for o in out[:-1]) and any(o < 0 for o in out)      # both kinds of step ran


@pytest.mark.parametrize("solver", ar.SOLVERS)
def test_decreasing_grid_is_the_forward_solve_of_the_time_negated_field(solver):
    """g(s, y) = -f(-s, y) on s = -t_span: the same trajectory, step log and dx; the gradients of W0's time column and of
    the last layer change sign."""
    Ws, bs, xa, G = _case(DOWN)
    d = xa.shape[1]
    node, traj, got = _generic(Ws, bs, xa, DOWN, solver, G)
    Wn, bn = cr.negated_mlp_params(Ws, bs)
    node_n, traj_n, got_n = _generic(Wn, bn, xa, -DOWN, solver, G)
    assert torch.equal(node.step_log, node_n.step_log) and node.n_steps == node_n.n_steps
    assert _rel(traj, traj_n) <= 1e-12
    flip = [np.ones_like(q) for q in got]
    flip[0][:, d] = -1.0
    flip[6] = -flip[6]; flip[7] = -flip[7]
    for n, (a, b, f) in enumerate(zip(got, got_n, flip)):
        print(f"{solver} tensor {n}: {_rel(a, f * b):.2e}")
        assert _rel(a, f * b) <= 1e-12


def test_unknown_solvers_are_refused_and_the_grid_is_checked():
    m = cfm_amd.MLP(dim=2, time_varying=True, w=16)
    for solver in ("euler", "midpoint", "rk4", "heun"):
        with pytest.raises(NotImplementedError, match="dopri5.*tsit5"):
            cfm_amd.AdaptiveDifferentiableNeuralODE(torch_wrapper(m), solver=solver)
    node = cfm_amd.AdaptiveDifferentiableNeuralODE(torch_wrapper(m))
    assert node.solver == "dopri5" and node.max_steps == 512 and (node.atol, node.rtol) == (1e-3, 1e-3)
    with pytest.raises(ValueError):
        node.trajectory(torch.zeros(3, 2), torch.tensor([0.0, 0.5, 0.2]))
    with pytest.raises(ValueError):
        node.trajectory(torch.zeros(3, 2), torch.tensor([0.5]))


@pytest.mark.parametrize("solver", ar.SOLVERS)
def test_too_small_max_steps_raises(solver):
    Ws, bs, xa, G = _case(UP)
    node, _, _ = _generic(Ws, bs, xa, UP, solver, G)
    need = node.n_accepted
    assert need > len(UP) - 1
    _generic(Ws, bs, xa, UP, solver, G, max_steps=need)                   # exactly enough
    with pytest.raises(RuntimeError, match="max_steps"):
        _generic(Ws, bs, xa, UP, solver, G, max_steps=need - 1)
    with pytest.raises(RuntimeError, match="max_steps"):
        _generic(Ws, bs, xa, UP, solver, G, max_steps=1)


def test_float32_state_on_the_cpu_runs_generic_and_carries_a_graph():
    m = cfm_amd.MLP(dim=2, time_varying=True, w=16)
    node = cfm_amd.AdaptiveDifferentiableNeuralODE(torch_wrapper(m), solver="tsit5")
    x = torch.randn(5, 2, requires_grad=True)
    traj = node.trajectory(x, torch.linspace(0, 1, 3))
    assert node.last_path == "generic" and traj.requires_grad and tuple(traj.shape) == (3, 5, 2)
    g = torch.autograd.grad(traj[-1].sum(), [x] + list(m.parameters()))
    assert all(torch.isfinite(q).all() for q in g)


def test_header_and_binding_carry_the_new_entries():
    text = open(HEADER).read()
    for name, nargs in (("cfm_ode_adaptive_rec_mlp_f32", 20), ("cfm_ode_adaptive_grad_f32", 17),
                        ("cfm_ode_adaptive_grad_available", 2)):
        decl = re.search(r"\bint " + name + r"\(([^;]*)\);", text)
        assert decl is not None, name
        assert len(decl.group(1).split(",")) == nargs
        assert len(_lib.SIGNATURES[name][1]) == nargs and _lib.SIGNATURES[name][0] is ctypes.c_int
    assert "#define CFM_ABI_VERSION 3" in text and _lib.ABI_VERSION == 3


def test_query_needs_no_gpu_and_follows_the_fixed_step_envelope():
    lib = _lib.load()

    def ask(*dims):
        return lib.cfm_ode_adaptive_grad_available((ctypes.c_int * len(dims))(*dims), len(dims) - 1)
    assert ask(3, 64, 64, 64, 2) == 0 and ask(64, 33, 1, 48, 63) == 0
    assert ask(3, 65, 64, 64, 2) == -1 and ask(65, 64, 64, 64, 64) == -1 and ask(3, 64, 64, 2) == -1
    lib.cfm_ode_set_fused(0)
    try:
        assert ask(3, 64, 64, 64, 2) == -1
    finally:
        lib.cfm_ode_set_fused(1)
    assert ask(3, 64, 64, 64, 2) == 0


# ---- what float32 arithmetic alone does to the gradients of the GPU tests' cases -------------------------------------------
def _float32_log(Ws, bs, x, ts, solver, tol):
    """The step log of the generic path in float32 on the CPU: the steps the GPU forward takes, up to rounding."""
    node = cfm_amd.AdaptiveDifferentiableNeuralODE(torch_wrapper(cr.make_mlp([w.copy() for w in Ws], [b.copy() for b in bs])),
                                                   solver=solver, atol=tol, rtol=tol)
    node.trajectory(torch.tensor(np.array(x)), torch.tensor(ts))
    return node


@pytest.mark.parametrize("solver", ar.SOLVERS)
@pytest.mark.parametrize("shape", ar.GPU_SHAPES + [ar.STRIDE_SHAPE, ar.streamed_shape(8192), "default"], ids=str)
def test_float32_replay_leaves_three_quarters_of_the_bound(shape, solver):
    """tests/test_gpu_ode_adaptive_grad.py holds the HIP gradients to 1e-5 of the float64 replay.  That bound stands for a
    shape only while the float32 replay's own ratio to the float64 replay is covered by a quarter of it (tsit5 has tableau
    entries near 13): measured here for every shape of that file, both directions, and for its default-initialised cases
    (rows within 1e-5 of a kink zeroed in G and left out of dx, as there)."""
    quarter = 1e-5 / 4
    if shape == "default":
        Ws, bs, x, G, ts, tol = ar.default_case(solver)
        node = _float32_log(Ws, bs, x, ts, solver, tol)
        log = node.step_log.numpy()
        keep = ar.kink_distance(Ws, bs, x, log, len(ts), solver, 1.0) >= 1e-5
        G = G.copy(); G[:, ~keep] = 0.0
        r = ar.float32_replay_ratio(Ws, bs, x, log, G, solver, 1.0, rows=keep)
        print(f"default net {solver}: accepted {node.n_accepted} of {node.n_steps}, {int((~keep).sum())} rows dropped, ratio {r:.2e}")
        assert node.n_steps > node.n_accepted and (~keep).sum() <= len(x) / 4      # what the case was chosen for
        assert r <= quarter
        return
    Ws, bs, x, G = ar.smooth_case(shape)
    for direction in ("down", "up"):
        ts = ar.grid(direction, shape[3])
        tsign = 1.0 if direction == "up" else -1.0
        node = _float32_log(Ws, bs, x, ts, solver, ar.GPU_TOL["atol"])
        r = ar.float32_replay_ratio(Ws, bs, x, node.step_log.numpy(), G, solver, tsign)
        print(f"{shape} {solver} {direction}: accepted {node.n_accepted} of {node.n_steps}, ratio {r:.2e}")
        assert r <= quarter
