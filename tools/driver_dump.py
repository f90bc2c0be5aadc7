"""What the Python drivers return (ode.py, cnf.py, sde.py, train.py, action_matching.py) on fixed seeds, in one .npz:

    python tools/driver_dump.py OUT.npz [--tree DIR]     (CFM_LIB_PATH selects the build of the library)
    python tools/driver_dump.py --compare A.npz B.npz

--tree DIR imports the package of another checkout (DIR/cfm_amd.py); the default is this one.  tools/ode_unit_dump.py calls
the C entries directly and so does not see a change of the Python marshalling; this tool goes through the public classes.  A
refactor of the drivers moves no floating-point operation, no random draw and no refusal, so two checkouts on ONE build of
the library must agree bit for bit: run the dump once per checkout, each in a fresh process, then --compare
(numpy.array_equal array by array, no tolerance; nfe / n_steps / last_path and the text of every refusal included; exit 1 on
any difference or any key present on one side only).

Shapes: B = 17 (two 16-row tiles, the second with one row), d = 2, hidden width 33 (padded columns) for the one-launch paths
and 128 for the layer-per-kernel paths, n_t = 4 on a non-uniform grid both ways, dt = 0.25 (the refined SDE grid has 5
steps).  Every case seeds torch before it builds its nets and again before it runs.  Without a GPU only the cases that need
none run (CPU float64 paths and refusals), which is what a development machine can compare.  Measurement infrastructure."""
import itertools
import os
import sys

import numpy as np

OUT = {}
GRID = [0.0, 0.3, 0.55, 1.0]
B, D, DT = 17, 2, 0.25


def put(key, *values):
    """tensors, numbers and strings under key, key + ' 1', ...; tuples and lists are flattened"""
    import torch

    def flatten(v):
        return [x for item in v for x in flatten(item)] if isinstance(v, (tuple, list)) else [v]
    for i, v in enumerate(flatten(values)):
        if isinstance(v, torch.Tensor):
            v = v.detach().cpu().numpy()
        v = np.asarray("None" if v is None else v)
        if v.dtype == object:
            raise TypeError(f"{key}: value {i} is neither a tensor, a number nor a string")
        OUT[key if i == 0 else f"{key} {i}"] = v


def case(key, fn):
    """fn()'s values, or the type and text of its refusal"""
    import torch
    torch.manual_seed(1234)
    try:
        got = fn()
    except (ValueError, NotImplementedError, TypeError, RuntimeError) as e:
        got = f"{type(e).__name__}: {e}"
    put(key, got)


def mlp(w, seed, d=D, out_dim=None, dev="cuda", dtype=None):
    import torch, cfm_amd
    torch.manual_seed(seed)
    m = cfm_amd.MLP(dim=d, out_dim=out_dim, time_varying=True, w=w).to(dev)
    return m.to(dtype) if dtype is not None else m


def randn(seed, *shape, dev="cuda", dtype=None):
    import torch
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed), dtype=dtype).to(dev)


def grads(loss, leaves):
    import torch
    return [g if g is not None else "None" for g in torch.autograd.grad(loss, leaves, allow_unused=True)]


def spans():
    import torch
    return {"up": torch.tensor(GRID), "down": torch.tensor(GRID[::-1])}


def ode_cases(gpu):
    import torch
    from cfm_amd.models import GradModel
    from cfm_amd.ode import SOLVERS, NeuralODE
    from cfm_amd.utils import torch_wrapper
    fields = {"callable": (lambda: (lambda t, x: -x * (1.0 + t)), "cpu")}
    if gpu:
        fields.update({"small": (lambda: torch_wrapper(mlp(33, 1)), "cuda"), "wide": (lambda: torch_wrapper(mlp(128, 1)), "cuda"),
                       "grad": (lambda: torch_wrapper(GradModel(mlp(33, 2, out_dim=1))), "cuda")})
    for (name, (make, dev)), solver, (way, ts) in itertools.product(fields.items(), SOLVERS, spans().items()):
        def run():
            node = NeuralODE(make(), solver=solver, atol=1e-4, rtol=1e-4)
            traj = node.trajectory(randn(3, B, D, dev=dev), ts)
            return traj, node.nfe, node.n_steps, node.last_path
        case(f"ode {name} {solver} {way}", run)


def cnf_cases(gpu):
    import torch
    from cfm_amd.cnf import CNF, log_likelihood
    from cfm_amd.models import GradModel
    from cfm_amd.ode import NeuralODE
    if not gpu:
        return
    probe = torch.sign(randn(4, B, D))
    for solver, est, (way, ts) in itertools.product(("euler", "dopri5"), ("exact", "hutch_rademacher"), spans().items()):
        noise = probe if est != "exact" else None

        def run():
            node = NeuralODE(CNF(mlp(33, 5), estimator=est, noise=noise), solver=solver, atol=1e-4, rtol=1e-4)
            traj = node.trajectory(randn(6, B, 1 + D), ts)
            return traj, node.nfe, node.n_steps, node.last_path
        case(f"cnf trajectory {solver} {est} {way}", run)
        if way == "down":
            case(f"cnf log_likelihood {solver} {est}",
                 lambda: log_likelihood(mlp(33, 5), randn(7, B, D), t_span=ts, solver=solver, atol=1e-4, rtol=1e-4, estimator=est,
                                        noise=noise, return_z=True))

    def run_grad():
        node = NeuralODE(CNF(GradModel(mlp(33, 8, out_dim=1))), solver="euler")
        traj = node.trajectory(randn(6, B, 1 + D), spans()["down"])
        return traj, node.nfe, node.n_steps, node.last_path
    case("cnf trajectory gradmodel euler", run_grad)


def ode_grad_cases(gpu):
    import torch
    from cfm_amd.ode import DifferentiableNeuralODE
    from cfm_amd.utils import torch_wrapper
    places = [("generic", "cpu", torch.float64)] + ([("hip", "cuda", None)] if gpu else [])
    for (name, dev, dtype), solver, (way, ts) in itertools.product(places, ("euler", "rk4"), spans().items()):
        def run():
            m = mlp(33, 9, dev=dev, dtype=dtype)
            node = DifferentiableNeuralODE(torch_wrapper(m), solver=solver)
            x = randn(10, B, D, dev=dev, dtype=dtype).requires_grad_(True)
            traj = node.trajectory(x, ts)
            loss = (traj * randn(11, 4, B, D, dev=dev, dtype=dtype)).sum()
            return traj, grads(loss, [x] + list(m.parameters())), node.nfe, node.n_steps, node.last_path
        case(f"odegrad {name} {solver} {way}", run)


def cnf_train_cases(gpu):
    import torch
    from cfm_amd.cnf import DifferentiableCNF, RegularizedCNF
    places = [("generic", "cpu", torch.float64, B)] + ([("hip", "cuda", None, B)] if gpu else [])
    for (name, dev, dtype, rows), est in itertools.product(places, ("exact", "hutch_rademacher")):
        noise = torch.sign(randn(12, rows, D, dev=dev, dtype=dtype)) if est != "exact" else None

        def run():
            m = mlp(33, 13, dev=dev, dtype=dtype)
            cnf = DifferentiableCNF(m, estimator=est, noise=noise)
            loss = cnf.nll(randn(14, rows, D, dev=dev, dtype=dtype), steps=3)
            return loss, grads(loss, list(m.parameters())), cnf.last_path
        case(f"cnftrain nll {name} {est}", run)
        for mask in (1, 2, 3) if est == "exact" else (1,):
            def run_reg():
                m = mlp(33, 13, dev=dev, dtype=dtype)
                cnf = RegularizedCNF(m, squared_l2_reg=0.1 * (mask & 1), jacobian_frobenius_reg=0.05 * (mask >> 1),
                                     estimator=est, noise=noise)
                reg, nll = cnf.loss(randn(14, rows, D, dev=dev, dtype=dtype), steps=3)
                return reg, nll, grads(reg + nll, list(m.parameters())), cnf.last_path
            case(f"cnftrain reg {name} {est} mask{mask}", run_reg)
    if gpu:
        def declined(make):
            def run():
                m = mlp(33, 13)
                cnf = make(m)
                out = cnf.loss(randn(14, 1, D), steps=100) if isinstance(cnf, RegularizedCNF) else cnf.nll(randn(14, 1, D), steps=100)
                loss = out[0] + out[1] if isinstance(out, tuple) else out
                return out, grads(loss, list(m.parameters())), cnf.last_path
            return run
        case("cnftrain nll declined B1", declined(lambda m: DifferentiableCNF(m)))
        case("cnftrain reg declined B1", declined(lambda m: RegularizedCNF(m, squared_l2_reg=0.1)))


def sde_cases(gpu):
    import torch
    from cfm_amd.schedule import LinearDecreasingNoiseScheduler
    from cfm_amd.sde import DriftSDE, FlowScoreSDE, sdeint
    ts = torch.tensor(GRID)
    sigmas = {"const": lambda: 0.3, "sched": lambda: LinearDecreasingNoiseScheduler(0.1, 0.5)}

    def make(kind, w, d, sigma, reverse, dev="cuda"):
        if kind == "flowscore":
            return FlowScoreSDE(mlp(w, 15, d=d, dev=dev), mlp(w, 16, d=d, dev=dev), sigma=sigma, reverse=reverse)
        return DriftSDE(mlp(w, 15, d=d, dev=dev), sigma=sigma, reverse=reverse)

    def noise_of(mode, method, d=D):
        if mode != "tensor":
            return mode
        return randn(17, 5, 2, B, d) if method == "srk" else randn(17, 5, B, d)

    def run_one(kind, method, fused, reverse, sig, mode, w=33, d=D):
        def run():
            sde = make(kind, w, d, sigmas[sig](), reverse)
            out = sdeint(sde, randn(18, B, d), ts, method=method, dt=DT, noise=noise_of(mode, method, d), fused=fused)
            return out, sde.last_path
        return run
    if gpu:
        for kind, method, fused, reverse, sig, mode in itertools.product(("flowscore", "drift"), ("euler", "srk"), (None, False, True),
                                                                         (False, True), sigmas, ("tensor", "torch", "philox")):
            case(f"sde {kind} {method} fused={fused} reverse={reverse} {sig} {mode}", run_one(kind, method, fused, reverse, sig, mode))
        case("sde flowscore euler d64", run_one("flowscore", "euler", None, False, "const", "philox", d=64))
        case("sde flowscore euler wide", run_one("flowscore", "euler", None, True, "sched", "tensor", w=128))
        case("sde flowscore srk wide", run_one("flowscore", "srk", None, False, "const", "torch", w=128))
        case("sde flowscore euler wide fused=True", run_one("flowscore", "euler", True, False, "const", "philox", w=128))
        case("sde flowscore euler d3 state fused=True", lambda: sdeint(make("flowscore", 33, D, 0.3, False), randn(18, B, 3), ts, dt=DT,
                                                                      fused=True))

        def state_dependent(fused):
            def run():
                sde = make("flowscore", 33, D, lambda t: 0.1 + 0.2 * t * torch.ones(B, 1, device="cuda"), False)
                out = sdeint(sde, randn(18, B, D), ts, dt=DT, noise=randn(17, 5, B, D), fused=fused)
                return out, sde.last_path
            return run
        case("sde state-dependent sigma", state_dependent(None))
        case("sde state-dependent sigma fused=True", state_dependent(True))
    # eager, CPU float64: fields that are no cfm_amd.MLP
    for kind, method, reverse, mode in itertools.product(("flowscore", "drift"), ("euler", "srk"), (False, True), ("tensor", "torch")):
        def run():
            torch.manual_seed(19)
            nets = [torch.nn.Sequential(torch.nn.Linear(D + 1, 16), torch.nn.Tanh(), torch.nn.Linear(16, D)).double() for _ in range(2)]
            sde = FlowScoreSDE(nets[0], nets[1], sigma=0.3, reverse=reverse) if kind == "flowscore" else DriftSDE(nets[0], 0.3, reverse)
            noise = mode if mode != "tensor" else randn(17, *((5, 2, B, D) if method == "srk" else (5, B, D)), dev="cpu", dtype=torch.float64)
            out = sdeint(sde, randn(18, B, D, dev="cpu", dtype=torch.float64), ts, method=method, dt=DT, noise=noise)
            return out, sde.last_path
        case(f"sde eager f64 {kind} {method} reverse={reverse} {mode}", run)
    x = randn(18, B, D, dev="cpu")
    sde = FlowScoreSDE(lambda z: z[:, :D], lambda z: -z[:, :D], sigma=0.3)
    case("sde refusal method", lambda: sdeint(sde, x, ts, method="milstein"))
    case("sde refusal noise name", lambda: sdeint(sde, x, ts, dt=DT, noise="numpy"))
    case("sde refusal noise type", lambda: sdeint(sde, x, ts, dt=DT, noise=3))
    case("sde refusal noise shape", lambda: sdeint(sde, x, ts, dt=DT, noise=torch.zeros(4, B, D)))
    case("sde refusal noise shape srk", lambda: sdeint(sde, x, ts, method="srk", dt=DT, noise=torch.zeros(5, B, D)))
    case("sde refusal srk decreasing", lambda: sdeint(sde, x, torch.tensor(GRID[::-1]), method="srk", dt=DT))
    case("sde refusal srk callable sigma", lambda: sdeint(FlowScoreSDE(sde.drift, sde.score, sigma=lambda t: 0.3), x, ts, method="srk"))
    case("sde refusal fused unknown fields", lambda: sdeint(sde, x, ts, dt=DT, fused=True))


def solver_cases(gpu):
    import torch
    from cfm_amd.schedule import LinearDecreasingNoiseScheduler
    from cfm_amd.sde import DSBMFlowSolver, FlowSolver
    from cfm_amd.utils import torch_wrapper
    ts = torch.tensor(GRID)
    sched = LinearDecreasingNoiseScheduler(0.1, 0.5)

    def fields(kind, w):
        if kind == "eager":     # plain callables f(t, x) on CPU float64
            return (lambda t, x: -x * (1.0 + t)), (lambda t, x: 0.5 * x - t), "cpu", torch.float64
        return torch_wrapper(mlp(w, 20)), (mlp(w, 21) if kind == "bare" else torch_wrapper(mlp(w, 21))), "cuda", None
    kinds = [("eager", 0)] + ([("wrapped", 33), ("bare", 33), ("wrapped", 128)] if gpu else [])
    for cls, (kind, w) in itertools.product((FlowSolver, DSBMFlowSolver), kinds):
        tag = f"{cls.__name__} {kind} w{w}"
        for reverse in (False, True):
            def run():
                f, s, dev, dtype = fields(kind, w)
                fs = cls(f, D, score_field=s, sigma=sched, dt=DT)
                out = fs.sdeint(randn(22, B, D, dev=dev, dtype=dtype), ts, reverse=reverse)
                return out, fs.nfe, fs.last_path
            case(f"solver {tag} sdeint reverse={reverse}", run)
        for solver, fused in itertools.product(("euler", "rk4", "dopri5"), (None, False)):
            def run():
                f, s, dev, dtype = fields(kind, w)
                fs = cls(f, D, score_field=s, sigma=sched, ode_solver=solver, dt=DT)
                x0 = randn(22, B, D, dev=dev, dtype=dtype)
                out = fs.odeint(x0, ts, fused=fused) if cls is DSBMFlowSolver else fs.odeint(x0, ts)
                return out, fs.nfe, fs.last_path
            if cls is DSBMFlowSolver or fused is None:
                case(f"solver {tag} odeint {solver} fused={fused}", run)

        def run_srk():
            f, s, dev, dtype = fields(kind, w)
            return cls(f, D, score_field=s, sigma=sched, sde_solver="srk").sdeint(randn(22, B, D, dev=dev, dtype=dtype), ts)
        case(f"solver {tag} srk", run_srk)
        if cls is DSBMFlowSolver:
            def run():
                f, s, dev, dtype = fields(kind, w)
                fs = cls(f, D, score_field=s, sigma=0.4, dt=DT)
                out = fs.resample_pairs(randn(22, B, D, dev=dev, dtype=dtype), randn(23, B, D, dev=dev, dtype=dtype),
                                        noise=randn(24, 4, B, D, dev=dev, dtype=dtype))
                return out, fs.nfe, fs.last_path
            case(f"solver {tag} resample_pairs", run)
    case("solver DSBMFlowSolver no sigma", lambda: DSBMFlowSolver(lambda t, x: x, D, score_field=lambda t, x: x).sdeint(randn(22, B, D, dev="cpu"), ts))
    case("solver DSBMFlowSolver no score", lambda: DSBMFlowSolver(lambda t, x: x, D))


def train_cases(gpu):
    import torch, cfm_amd
    from cfm_amd.train import DSBMStep, RegressionStep, SF2MStep
    dev = "cuda" if gpu else "cpu"

    def batch(k):
        return {n: randn(30 + 10 * k + i, *shape, dev=dev) for i, (n, shape) in enumerate(
            (("t", (B,)), ("xt", (B, D)), ("ut", (B, D)), ("eps", (B, D)), ("lam", (B,)), ("bt", (B, D))))}

    def three_steps(make, call, nets):
        def run():
            params = [p for m in nets for p in m.parameters()]
            step = make(nets, cfm_amd.FusedAdam(params, lr=1e-2))
            losses = [call(step, batch(k)).clone() for k in range(3)]
            return losses, step.flat_grad, params
        return run
    calls = {
        "regression": (lambda nets, opt: RegressionStep(nets[0], opt), lambda s, b: s(b["t"].abs() % 1, b["xt"], b["ut"]), 1),
        "sf2m": (lambda nets, opt: SF2MStep(nets[0], nets[1], opt, score_weight=0.5),
                 lambda s, b: s(b["t"].abs() % 1, b["xt"], b["ut"], b["eps"], b["lam"]), 2),
        "dsbm": (lambda nets, opt: DSBMStep(nets[0], nets[1], opt),
                 lambda s, b: s(b["t"].abs() % 1, b["xt"], b["ut"], b["bt"], b["lam"].abs(), b["eps"][:, 0].abs()), 2),
    }
    for (name, (make, call, n_nets)), w in itertools.product(calls.items(), (64, 33)):
        if gpu:
            case(f"train {name} w{w}", three_steps(make, call, [mlp(w, 25 + i) for i in range(n_nets)]))
    # refusals: at construction (also without a GPU: then "not on the GPU" is the text) and at the call
    opt = None
    for name, (make, call, n_nets) in calls.items():
        def nets(w=33, **kw):
            return [mlp(w, 25 + i, dev=dev, **kw) for i in range(n_nets)]

        def no_bias():
            ms = nets()
            ms[-1].net[2] = torch.nn.Linear(33, 33, bias=False).to(dev)
            return make(ms, opt)
        case(f"train {name} refusal no bias", no_bias)
        case(f"train {name} refusal fp64", lambda: make(nets(dtype=torch.float64), opt))
        case(f"train {name} refusal not an MLP", lambda: make([torch.nn.Linear(3, 2).to(dev)] * n_nets, opt))
        if n_nets == 2:
            case(f"train {name} refusal sizes", lambda: make([mlp(33, 25, dev=dev), mlp(64, 26, dev=dev)], opt))
            case(f"train {name} refusal same module", lambda: make([mlp(33, 25, dev=dev)] * 2, opt))
            case(f"train {name} refusal 8 layers", lambda: call(make([deep(dev, 25), deep(dev, 26)], opt), batch(0)))
        if gpu:
            ms = nets()
            step = make(ms, cfm_amd.FusedAdam([p for m in ms for p in m.parameters()]))
            b = batch(0)
            case(f"train {name} refusal xt columns", lambda: call(step, dict(b, xt=randn(1, B, D + 1))))
            case(f"train {name} refusal ut columns", lambda: call(step, dict(b, ut=randn(1, B, D + 1))))
            case(f"train {name} refusal ut rows", lambda: call(step, dict(b, ut=randn(1, B - 1, D))) if n_nets == 2 else "not run")
            case(f"train {name} refusal times", lambda: call(step, dict(b, t=randn(1, B - 1))))
            if n_nets == 2:
                case(f"train {name} refusal lambda_t", lambda: call(step, dict(b, lam=randn(1, B - 1))))
                case(f"train {name} refusal eps", lambda: call(step, dict(b, eps=randn(1, B - 1, D))))


def deep(dev, seed):
    """an MLP of 8 Linear layers (the two-net steps take at most 7)"""
    import torch
    m = mlp(33, seed, dev=dev)
    layers = list(m.net)[:-1]
    for _ in range(4):
        layers += [torch.nn.Linear(33, 33), torch.nn.SELU()]
    m.net = torch.nn.Sequential(*layers, torch.nn.Linear(33, D)).to(dev)
    return m


def action_cases(gpu):
    import torch, cfm_amd
    places = [("generic", "cpu", torch.float64)] + ([("hip", "cuda", None)] if gpu else [])
    for (name, dev, dtype), given_xt in itertools.product(places, (False, True)):
        def run():
            m = mlp(33, 27, out_dim=1, dev=dev, dtype=dtype)
            x0, x1, t = (randn(28 + i, *shape, dev=dev, dtype=dtype) for i, shape in enumerate(((B, D), (B, D), (B,))))
            t = t.abs() % 1
            xt = (0.9 * t[:, None] * x1 + (1 - t[:, None]) * x0) if given_xt else None
            loss = cfm_amd.action_matching_loss(m, x0, x1, t, xt=xt)
            return loss, grads(loss, list(m.parameters())), cfm_amd.action_matching_loss.last_path
        case(f"action {name} xt={given_xt}", run)
    case("action refusal shapes", lambda: cfm_amd.action_matching_loss(mlp(33, 27, out_dim=1, dev="cpu"), torch.zeros(B, D), torch.zeros(B, 3),
                                                                       torch.zeros(B)))
    case("action refusal times", lambda: cfm_amd.action_matching_loss(mlp(33, 27, out_dim=1, dev="cpu"), torch.zeros(B, D), torch.zeros(B, D),
                                                                      torch.zeros(B - 1)))


GROUPS = (("ode ", ode_cases), ("cnf ", cnf_cases), ("odegrad ", ode_grad_cases), ("cnftrain ", cnf_train_cases), ("sde ", sde_cases),
          ("solver ", solver_cases), ("train ", train_cases), ("action ", action_cases))     # (key prefix, cases)


def compare(a, b):
    A, Bz = np.load(a), np.load(b)
    bad = [k for k in sorted(set(A.files) | set(Bz.files)) if k not in A.files or k not in Bz.files or not np.array_equal(A[k], Bz[k])]
    for kind, _ in GROUPS:
        ks = [k for k in A.files if k.startswith(kind)]
        refused = sum(A[k].dtype.kind == "U" and ": " in str(A[k]) for k in ks)
        print(f"{kind.strip()}: {len(ks)} arrays ({refused} refusals), {sum(k in bad for k in ks)} differ")
    print("differing:", bad if bad else "none")
    return 1 if bad else 0


if __name__ == "__main__":
    if sys.argv[1] == "--compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    tree = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if "--tree" in sys.argv:
        tree = os.path.abspath(sys.argv[sys.argv.index("--tree") + 1])
    sys.path.insert(0, tree)
    import torch
    import cfm_amd
    gpu = torch.cuda.is_available()
    for _, cases in GROUPS:
        cases(gpu)
    np.savez(sys.argv[1], **OUT)
    from cfm_amd import _lib
    print(f"{len(OUT)} arrays from the package at {os.path.dirname(cfm_amd.__file__)} on {_lib.LIB_PATH} "
          f"({'GPU' if gpu else 'no GPU: CPU cases only'}) -> {sys.argv[1]}")
