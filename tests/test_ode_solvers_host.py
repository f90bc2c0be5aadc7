"""CPU: the solver set of NeuralODE (euler, midpoint, rk4, dopri5, tsit5) — the tableaus against their order
conditions, the generic path against the float64 restatements of tests/ode_rk_ref.py, empirical orders, reverse time,
argument checks, and the pass-throughs (FlowSolver, log_likelihood).  No GPU needed."""
import os

import numpy as np
import pytest
import torch

import cfm_oracle as oracle
import cnf_restate as R
import ode_rk_ref as rk

SOLVERS = ("euler", "midpoint", "rk4", "dopri5", "tsit5")


class _NetField(torch.nn.Module):
    """f(t, x) = MLP.net([x, t]) on the CPU (the module graph: no HIP inference path involved)."""

    def __init__(self, m, sign=1.0):
        super().__init__()
        self.m, self.sign = m, sign

    def forward(self, t, x):
        tt = torch.as_tensor(t, dtype=x.dtype).reshape(1, 1).expand(x.shape[0], 1)
        if self.sign < 0:
            return -self.m.net(torch.cat([x, -tt], 1))
        return self.m.net(torch.cat([x, tt], 1))


def _mlp64(d=2, w=16, seed=3):
    Ws, bs = R.mlp_params(d, w, seed)
    return R.make_mlp(Ws, bs, dtype=torch.float64), Ws, bs


# ------------------------------------------------------------------------------------------------------- tableaus
def _package_tableaus():
    from cfm_amd import ode
    return ode.ADAPTIVE_TABLEAUS, ode.FIXED_TABLEAUS


def test_solver_set_is_torchdyns():
    from cfm_amd import ode
    adaptive, fixed = _package_tableaus()
    assert tuple(ode.SOLVERS) == SOLVERS
    assert sorted(adaptive) == ["dopri5", "tsit5"] and sorted(fixed) == ["euler", "midpoint", "rk4"]


def test_every_tableau_satisfies_its_order_conditions():
    """float64: row sums equal c; tsit5's and dopri5's b (= the last row of a) hold all 17 conditions through order 5 to
    1e-14; their embedded b - e holds through order 4 and NOT order 5; rk4 holds through order 4 (and not 5), midpoint
    through order 2 (and not 3), euler order 1.  This pins the constants without torchdyn."""
    adaptive, fixed = _package_tableaus()
    for name, tab in adaptive.items():
        b = list(tab["a"][5]) + [0.0]
        A, bv, c = rk.butcher(tab["c"], tab["a"], b)
        assert np.abs(A.sum(1) - c).max() <= 1e-14, name
        assert tab["order"] == 5
        res = rk.order_residuals(A, bv, c)
        assert sum(len(v) for v in res.values()) == 17
        worst = max(abs(r) for v in res.values() for r in v)
        print(name, "b: worst residual through order 5:", worst)
        assert worst <= 1e-14, (name, worst)
        emb = rk.order_residuals(A, bv - np.asarray(tab["e"], dtype=np.float64), c)
        low = max(abs(r) for o in (1, 2, 3, 4) for r in emb[o])
        o5 = np.abs(emb[5])
        print(name, "b - e: worst residual through order 4:", low, "order 5:", o5.min(), "..", o5.max())
        # (e is written with 15 decimals: 7 entries * 5e-16 * weights <= 1)
        assert low <= 1e-14, (name, low)
        assert o5.max() >= 1e-5, (name, o5)
    for name, order in (("euler", 1), ("midpoint", 2), ("rk4", 4)):
        tab = fixed[name]
        A, bv, c = rk.butcher(tab["c"], tab["a"], tab["b"])
        assert np.abs(A.sum(1) - c).max() <= 1e-15, name
        assert tab["order"] == order
        res = rk.order_residuals(A, bv, c)
        assert max(abs(r) for o in range(1, order + 1) for r in res[o]) <= 1e-15, name
        assert max(abs(r) for r in res[order + 1]) >= 1e-3, name


def test_package_tableaus_equal_the_restatements_copy():
    adaptive, fixed = _package_tableaus()
    for name, tab in adaptive.items():
        ref = rk.ADAPTIVE[name]
        assert list(tab["c"]) == list(ref["c"]) and [list(r) for r in tab["a"]] == [list(r) for r in ref["a"]]
        assert list(tab["e"]) == list(ref["e"])
    for name, tab in fixed.items():
        ref = rk.FIXED[name]
        assert list(tab["c"]) == list(ref["c"]) and [list(r) for r in tab["a"]] == [list(r) for r in ref["a"]]
        assert list(tab["b"]) == list(ref["b"])


def test_kernel_source_carries_the_same_tsit5_constants():
    """csrc/ode_tableau.h (the one table of ode.hip's solvers and small_grad.hip's gradient kernels) spells every tsit5
    entry with the digits of the package's table (the casts to float happen at the use, from these float64 constants)."""
    adaptive, _ = _package_tableaus()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(root, "conditional-flow-matching_amd", "csrc", "ode_tableau.h")).read()
    tab = adaptive["tsit5"]
    for v in [x for row in tab["a"] for x in row] + list(tab["c"][:4]) + list(tab["e"][:6]):
        assert repr(abs(v)) in src, v
    assert "-1.0 / 66" in src


def test_restatement_with_the_dopri5_tableau_is_the_oracles_dopri5(golden_dir):
    """(to rounding: the two take the controller's float32 powers with different NumPy routines, one ulp apart on some
    inputs, so dt may differ in its last bits; a trajectory point then moves by far less than the local error)"""
    d = np.load(os.path.join(golden_dir, "ode_cases.npz"))
    Ws, bs = [d[f"W{k}"] for k in range(4)], [d[f"b{k}"] for k in range(4)]
    f = lambda t, y: oracle.mlp_forward_f64(Ws, bs, y, t)
    for ts, tol in ((d["t_span"], 1e-4), (np.array([0.0, 1.0], dtype=np.float32), 1e-6)):
        a, ia = rk.adaptive_trajectory(f, d["x"], ts, tol, tol, "dopri5", return_log=True)
        b, ib = oracle.dopri5_trajectory(f, d["x"], ts, tol, tol, return_log=True)
        assert (ia["steps"], ia["nfe"]) == (ib["steps"], ib["nfe"]) and [l[3] for l in ia["log"]] == [l[3] for l in ib["log"]]
        assert np.abs(a - b).max() <= 1e-7 * np.abs(b).max()
    assert np.array_equal(rk.fixed_trajectory(f, d["x"], d["t_span"], "euler"), oracle.euler_trajectory(f, d["x"], d["t_span"]))


def test_recorded_fixtures_are_what_the_restatement_gives(golden_dir):
    """ode_solvers_cases.npz (tests/golden/make_ode_solvers_golden.py), the golden-MLP part; every recorded adaptive log
    keeps its error ratios out of [0.99, 1.01]."""
    d = np.load(os.path.join(golden_dir, "ode_cases.npz"))
    g = np.load(os.path.join(golden_dir, "ode_solvers_cases.npz"))
    Ws, bs = [d[f"W{k}"] for k in range(4)], [d[f"b{k}"] for k in range(4)]
    f = lambda t, y: oracle.mlp_forward_f64(Ws, bs, y, t)
    tr, info = rk.adaptive_trajectory(f, d["x"], d["t_span"], 1e-4, 1e-4, "tsit5", return_log=True)
    assert info["steps"] == int(g["g_tsit5_steps"]) and info["nfe"] == int(g["g_tsit5_nfe"]) == 2 + 6 * info["steps"]
    np.testing.assert_allclose(tr, g["g_tsit5"], rtol=1e-12)
    rk.assert_same_log(info["log"], g["g_tsit5_log"])
    for scheme in ("midpoint", "rk4"):
        np.testing.assert_allclose(rk.fixed_trajectory(f, d["x"], d["t_span"], scheme), g[f"g_{scheme}"], rtol=1e-12)
    for k in ("g", "c", "l"):
        assert rk.ratios_clear_of_one(g[f"{k}_tsit5_log"]), k
        assert int(g[f"{k}_tsit5_nfe"]) == 2 + 6 * int(g[f"{k}_tsit5_steps"]) == 2 + 6 * len(g[f"{k}_tsit5_log"])


# ------------------------------------------------------------------------------------------------------- generic path
@pytest.mark.parametrize("ts", [[0.0, 0.3, 0.55, 1.0], [0.0, 1.0]])
def test_generic_tsit5_matches_the_restatement(ts):
    """float64 field on the CPU: same n_steps / nfe, trajectories to 1e-12 (the restatement with float64 tableau entries,
    as the generic path multiplies them; the float32 controller is the same).  The tolerance is a power of two: the
    restatement rounds atol / rtol to float32 as the kernels' float arguments are, NeuralODE keeps the Python floats.
    Both grids give rejected steps."""
    from cfm_amd.ode import NeuralODE
    m, Ws, bs = _mlp64()
    torch.manual_seed(0)
    x = torch.randn(33, 2, dtype=torch.float64)
    ts = torch.tensor(ts)
    tol = 2.0 ** -20
    node = NeuralODE(_NetField(m), solver="tsit5", atol=tol, rtol=tol)
    tr = node.trajectory(x, ts)
    assert node.last_path == "generic" and tr.dtype == torch.float64
    ref, info = rk.adaptive_trajectory(R.mlp_field_np(Ws, bs), x.numpy(), ts.numpy(), tol, tol, "tsit5",
                                       coef_dtype=np.float64, return_log=True)
    assert not all(l[3] for l in info["log"])
    assert (node.n_steps, node.nfe) == (info["steps"], info["nfe"]) and node.nfe == 2 + 6 * node.n_steps
    assert tr.shape == ref.shape
    assert np.abs(tr.numpy() - ref).max() <= 1e-12 * max(1.0, np.abs(ref).max())


@pytest.mark.parametrize("solver", ["midpoint", "rk4"])
def test_generic_fixed_step_matches_the_restatement(solver):
    from cfm_amd.ode import NeuralODE
    m, Ws, bs = _mlp64()
    torch.manual_seed(1)
    x = torch.randn(17, 2, dtype=torch.float64)
    ts = torch.linspace(0, 1, 9)
    node = NeuralODE(_NetField(m), solver=solver, atol=1e-9, rtol=1e-9)      # tolerances: ignored, silently
    tr = node.trajectory(x, ts)
    ref = rk.fixed_trajectory(R.mlp_field_np(Ws, bs), x.numpy(), ts.numpy(), solver, coef_dtype=np.float64)
    stages = {"midpoint": 2, "rk4": 4}[solver]
    assert node.last_path == "generic" and (node.n_steps, node.nfe) == (8, stages * 8)
    assert np.abs(tr.numpy() - ref).max() <= 1e-12 * max(1.0, np.abs(ref).max())
    assert torch.equal(tr, NeuralODE(_NetField(m), solver=solver).trajectory(x, ts))


class _Oscillator(torch.nn.Module):
    """y'' = -y (pendulum=False) or y'' = -sin y: smooth and AUTONOMOUS.  The solvers keep t and the stage times in
    float32, which would put a ~1e-8 floor under the error of a time-dependent field — above tsit5's error at the
    finer grids."""

    def __init__(self, pendulum):
        super().__init__()
        self.pendulum = pendulum

    def forward(self, t, x):
        return torch.stack([x[:, 1], -torch.sin(x[:, 0]) if self.pendulum else -x[:, 0]], 1)


_X0 = np.array([[1.0, 0.0], [0.3, -0.8], [-1.2, 0.5]])


def _fixed_dt_errors(field, solver, T, ns, exact):
    """Errors at T on grids of n equal steps (dt a power of two: exact in float32).  The adaptive solver steps the
    grid: at atol = rtol = 1 every attempt is accepted with a tiny error ratio and wants to grow tenfold, and the
    initial step (~0.5) exceeds every dt used, so each step is clipped to the next t_span point: n_steps == n."""
    from cfm_amd.ode import NeuralODE
    errs = []
    for n in ns:
        node = NeuralODE(field, solver=solver, atol=1.0, rtol=1.0)
        tr = node.trajectory(torch.from_numpy(_X0), torch.linspace(0, T, n + 1))
        assert tr.shape == (n + 1, 3, 2) and node.n_steps == n
        errs.append(np.abs(tr[-1].numpy() - exact).max())
    return errs, [float(np.log2(errs[i] / errs[i + 1])) for i in range(3)]


@pytest.mark.parametrize("solver,order", [("midpoint", 2), ("rk4", 4), ("tsit5", 5)])
def test_empirical_order(solver, order):
    """y'' = -y to T = 16 with dt = 1/8, 1/16, 1/32, 1/64 against the exact rotation: the slope of each of the three
    halvings is the order within 0.3.  (tsit5's principal error constant is small by design, so its slopes come down
    to 5 from above and are within 0.3 only from dt = 1/8 on; T = 16 keeps its error at dt = 1/64, 7e-13, well above
    float64 rounding.)"""
    T = 16.0
    c, s = np.cos(T), np.sin(T)
    exact = np.stack([c * _X0[:, 0] + s * _X0[:, 1], -s * _X0[:, 0] + c * _X0[:, 1]], 1)
    errs, slopes = _fixed_dt_errors(_Oscillator(False), solver, T, (128, 256, 512, 1024), exact)
    print(solver, "errors", errs, "slopes", slopes)
    assert all(abs(sl - order) <= 0.3 for sl in slopes), (errs, slopes)


@pytest.mark.parametrize("solver,order", [("midpoint", 2), ("rk4", 4), ("tsit5", 5)])
def test_empirical_order_nonlinear(solver, order):
    """The pendulum y'' = -sin y to T = 2 with dt = 1/4 .. 1/32 against DOP853 at rtol = 1e-13 (every order condition
    takes part, not only the linear ones): midpoint and rk4 within 0.3 of their order.  tsit5's fifth-order regime lies
    below float64 resolution on this problem (error 2e-12 at dt = 1/32 with the sixth-order term still visible): its
    slopes lie between its order and the next, and fall."""
    from scipy.integrate import solve_ivp
    sol = solve_ivp(lambda t, y: np.stack([y.reshape(3, 2)[:, 1], -np.sin(y.reshape(3, 2)[:, 0])], 1).ravel(), (0.0, 2.0),
                    _X0.ravel(), method="DOP853", rtol=1e-13, atol=1e-14)
    errs, slopes = _fixed_dt_errors(_Oscillator(True), solver, 2.0, (8, 16, 32, 64), sol.y[:, -1].reshape(3, 2))
    print(solver, "errors", errs, "slopes", slopes)
    if solver == "tsit5":
        assert all(order - 0.3 <= sl <= order + 1 for sl in slopes) and slopes[0] > slopes[1] > slopes[2], (errs, slopes)
    else:
        assert all(abs(sl - order) <= 0.3 for sl in slopes), (errs, slopes)


@pytest.mark.parametrize("solver", ["midpoint", "rk4", "tsit5"])
def test_backward_solve_equals_forward_solve_of_the_negated_field(solver):
    from cfm_amd.ode import NeuralODE
    m, _, _ = _mlp64()
    torch.manual_seed(0)
    x = torch.randn(33, 2, dtype=torch.float64)
    ts = torch.linspace(1, 0, 5)
    node = NeuralODE(_NetField(m), solver=solver, atol=1e-6, rtol=1e-6)
    tr = node.trajectory(x, ts)
    assert tr.shape == (5, 33, 2) and node.last_path == "generic"
    fwd = NeuralODE(_NetField(m, sign=-1.0), solver=solver, atol=1e-6, rtol=1e-6)
    tf = fwd.trajectory(x, -ts)
    assert torch.equal(tr, tf)
    assert (node.n_steps, node.nfe) == (fwd.n_steps, fwd.nfe)


@pytest.mark.parametrize("ts", [[0.0, 0.5, 0.4, 1.0], [1.0, 1.0, 0.0], [0.0, 0.3, 0.3]])
def test_non_monotone_t_span_raises_value_error_for_every_solver(ts):
    from cfm_amd.ode import NeuralODE
    m, _, _ = _mlp64()
    for solver in SOLVERS:
        with pytest.raises(ValueError):
            NeuralODE(_NetField(m), solver=solver).trajectory(torch.zeros(3, 2, dtype=torch.float64), torch.tensor(ts))


def test_unknown_solver_raises_and_names_the_set():
    from cfm_amd.ode import NeuralODE
    m, _, _ = _mlp64()
    for bad in ("alf", "rk-4", "dopri8", "ieuler"):
        with pytest.raises(NotImplementedError) as e:
            NeuralODE(_NetField(m), solver=bad)
        assert all(s in str(e.value) for s in SOLVERS)
    assert NeuralODE(_NetField(m)).solver == "dopri5"           # the default stays


# ------------------------------------------------------------------------------------------------------- accuracy
def test_tsit5_accuracy_against_dop853(golden_dir):
    """tsit5 at atol = rtol = 1e-6 on the MLP field of ode_cases.npz against scipy's DOP853 at rtol = 1e-10: within 1e-4
    relative — the check that validates the restated dopri5 (tests/test_oracle_golden.py), for the restatement and for
    NeuralODE's generic path."""
    from scipy.integrate import solve_ivp
    from cfm_amd.ode import NeuralODE
    d = np.load(os.path.join(golden_dir, "ode_cases.npz"))
    Ws, bs = [d[f"W{k}"] for k in range(4)], [d[f"b{k}"] for k in range(4)]
    f = lambda t, y: oracle.mlp_forward_f64(Ws, bs, y, t)
    x0 = d["x"][:8].astype(np.float64)
    sol = solve_ivp(lambda t, y: f(t, y.reshape(8, 2)).ravel(), (0.0, 1.0), x0.ravel(), method="DOP853", rtol=1e-10,
                    atol=1e-12)
    exact = sol.y[:, -1].reshape(8, 2)
    mine = rk.adaptive_trajectory(f, x0, d["t_span"], 1e-6, 1e-6, "tsit5")[-1]
    m = R.make_mlp(Ws, bs, dtype=torch.float64)
    node = NeuralODE(_NetField(m), solver="tsit5", atol=1e-6, rtol=1e-6)
    ours = node.trajectory(torch.from_numpy(x0), torch.from_numpy(d["t_span"]))[-1].numpy()
    for got in (mine, ours):
        rel = np.abs(got - exact).max() / np.abs(exact).max()
        print("tsit5 vs DOP853, relative:", rel)
        assert rel <= 1e-4


# ------------------------------------------------------------------------------------------------------- pass-throughs
def test_flow_solver_passes_tsit5_through():
    from cfm_amd.ode import NeuralODE
    from cfm_amd.sde import FlowSolver
    m, _, _ = _mlp64()
    torch.manual_seed(2)
    x = torch.randn(11, 2, dtype=torch.float64)
    ts = torch.linspace(0, 1, 4)
    for solver in ("tsit5", "rk4", "midpoint"):
        fs = FlowSolver(_NetField(m), dim=2, ode_solver=solver, atol=1e-6, rtol=1e-6)
        out = fs.odeint(x, ts)
        node = NeuralODE(_NetField(m), solver=solver, atol=1e-6, rtol=1e-6)
        assert torch.equal(out, node.trajectory(x, ts)) and fs.nfe == node.nfe > 0


@pytest.mark.parametrize("solver", ["tsit5", "rk4"])
def test_log_likelihood_passes_the_solver_through(solver):
    """log p(x) on the generic path (CPU, float64) against the restatement on the reverse augmented field."""
    import cfm_amd
    m, Ws, bs = _mlp64(d=2, w=16)
    torch.manual_seed(5)
    x = torch.randn(12, 2, dtype=torch.float64)
    ts = torch.linspace(1, 0, 9)
    lp, z = cfm_amd.log_likelihood(m, x, t_span=ts, solver=solver, atol=1e-6, rtol=1e-6, return_z=True)
    y0 = np.concatenate([np.zeros((12, 1)), x.numpy()], 1)
    F = R.aug_field_np(Ws, bs)
    if solver == "tsit5":
        ref = rk.adaptive_trajectory(R.reverse(F), y0, -ts.numpy(), 1e-6, 1e-6, "tsit5", coef_dtype=np.float64)[-1]
    else:
        ref = rk.fixed_trajectory(F, y0, ts.numpy(), solver, coef_dtype=np.float64)[-1]
    z_ref = ref[:, 1:]
    lp_ref = -0.5 * (z_ref ** 2).sum(1) - np.log(2 * np.pi) - ref[:, 0]
    assert np.abs(z.numpy() - z_ref).max() <= 1e-6 * max(1.0, np.abs(z_ref).max())
    assert np.abs(lp.numpy() - lp_ref).max() <= 1e-6 * max(1.0, np.abs(lp_ref).max())
