"""CPU: AugmentationModule, FlowSolver.odeint under augmentations and RegularizedCNF(l1_reg, l2_reg) on their generic
paths, in float64, against the reference's own integrands (tests/golden/augmentation_integrands.json, written by
tools/make_augmentation_golden.py) and the restatement of tests/augment_restate.py.

Bounds: 1e-12 relative for one evaluation of the integrands and 1e-10 for a solve or its gradient, float64 on both
sides: the two sides order a few hundred float64 operations per value differently (2^-53 each), nothing else."""
import itertools
import json
import os

import numpy as np
import pytest
import torch

import cfm_amd
import augment_restate as ar
import cnf_restate as cr
import cnf_train_restate as tr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KW = {"L1": "l1_reg", "L2": "l2_reg", "squared_L2": "squared_l2_reg", "jacobian_frobenius": "jacobian_frobenius_reg"}
ORDER = ["L1", "L2", "squared_L2", "jacobian_frobenius"]


def _field64(Ws, bs):
    """f(t, x) of the net in float64 torch ops (differentiable in x); t a float or a 0-dim tensor."""
    W = [torch.tensor(np.asarray(w, np.float64)) for w in Ws]
    b = [torch.tensor(np.asarray(q, np.float64)) for q in bs]

    def f(t, x):
        h = torch.cat([x, torch.full_like(x[:, :1], float(t))], 1)
        for l in range(3):
            h = tr.selu(h @ W[l].T + b[l])
        return h @ W[3].T + b[3]
    return f


def _rel(a, b):
    return float(np.abs(np.asarray(a, np.float64) - b).max() / np.abs(b).max())


@pytest.mark.parametrize("estimator", [None, "exact"])
def test_names_coeffs_dims_and_forward_for_every_subset(estimator):
    for r in range(5):
        for subset in itertools.combinations(ORDER, r):
            coeff = {n: 0.25 * (k + 1) for k, n in enumerate(subset)}
            am = cfm_amd.AugmentationModule(estimator, **{KW[n]: c for n, c in coeff.items()})
            names = (["log_prob"] if estimator else []) + [n for n in ORDER if n in subset]
            assert am.names == names and am.aug_dims == len(names)
            want = ([1.0] if estimator else []) + [coeff[n] for n in ORDER if n in subset]
            assert am.coeffs.tolist() == want
            assert am.reg_mask == sum(ar.BITS[n] for n in subset)
            a, x = len(names), torch.arange(3.0 * (len(names) + 2)).reshape(3, -1)
            got = am(x)
            if estimator is None:
                assert len(got) == 2 and torch.equal(got[1], x[:, a:])
                if a == 0:
                    assert torch.equal(got[0], torch.zeros(1))
                else:
                    assert torch.equal(got[0], x[:, :a] * torch.tensor(want))
            else:
                assert len(got) == 3 and torch.equal(got[0], x[:, :1]) and torch.equal(got[2], x[:, a:])
                if a == 1:
                    assert torch.equal(got[1], torch.zeros(1))
                else:
                    assert torch.equal(got[1], x[:, 1:a] * torch.tensor(want[1:]))


def test_the_three_refusals():
    with pytest.raises(ValueError, match="cnf_estimator"):
        cfm_amd.AugmentationModule("hutch")
    with pytest.raises(NotImplementedError, match=r"::d.*first output's gradient.*no config"):
        cfm_amd.AugmentationModule(jacobian_diag_frobenius_reg=0.1)
    with pytest.raises(NotImplementedError, match=r"::d.*first output's gradient.*no config"):
        cfm_amd.AugmentationModule(jacobian_off_diag_frobenius_reg=0.1)
    cfm_amd.AugmentationModule(jacobian_diag_frobenius_reg=0.0, jacobian_off_diag_frobenius_reg=0.0)


def test_generic_integrands_are_the_reference_s():
    gold = json.load(open(os.path.join(ROOT, "tests", "golden", "augmentation_integrands.json")))
    Ws, bs, x, times = ar.golden_case(seed=gold["seed"])
    assert list(times) == gold["times"] and np.array_equal(np.asarray(x, np.float64), np.asarray(gold["x"]))
    f = _field64(Ws, bs)
    am = cfm_amd.AugmentationModule("exact", l1_reg=1, l2_reg=1, squared_l2_reg=1, jacobian_frobenius_reg=1)
    for t, row in zip(times, gold["integrands"]):
        augs, dx = am.integrands(f, t, torch.tensor(np.asarray(x, np.float64)))
        assert augs.dtype == torch.float64 and augs.shape == (8, 5) and dx.shape == (8, 2)
        for k, n in enumerate(am.names):
            err = _rel(augs[:, k].numpy(), np.asarray(row[n]))
            print(f"t = {t} {n}: {err:.2e}")
            assert err <= 1e-12, (t, n, err)
        # and the restatement the GPU tests measure against is the reference's too
        _, cols = ar.integrands(tr.as_params(Ws, bs, False), torch.tensor(np.asarray(x, np.float64)), t, 0, 15)
        for n, c in zip(ar.columns(0, 15), cols):
            assert _rel(c.numpy(), np.asarray(row[n])) <= 1e-12, (t, n)


def _solver(f, solver, am=None, **kw):
    return cfm_amd.FlowSolver(f, 2, ode_solver=solver, augmentations=am, **kw)


def test_odeint_with_and_without_augmentations():
    Ws, bs = cr.mlp_params(2, 16, 3)
    f = _field64(Ws, bs)
    x0 = torch.tensor(np.random.default_rng(0).normal(size=(7, 2)))
    ts = torch.linspace(0, 1, 6)
    fs = _solver(f, "euler")
    assert fs.augmentations is None
    plain = fs.odeint(x0, ts)
    assert torch.is_tensor(plain) and plain.shape == (6, 7, 2)
    fs.augmentations = cfm_amd.AugmentationModule(l1_reg=1, l2_reg=1, squared_l2_reg=1)        # assigned later, as the runner does
    got = fs.odeint(x0, ts)
    assert isinstance(got, tuple) and len(got) == 2
    traj, aug = got
    assert traj.shape == (6, 7, 2) and aug.shape == (6, 7, 3) and fs.last_path == "eager" and fs.nfe == 5
    assert torch.equal(aug[0], torch.zeros(7, 3, dtype=torch.float64)) and torch.equal(traj[0], x0)
    assert torch.equal(traj, plain)
    assert bool((aug[1:] > 0).all()) and bool((aug[1:] >= aug[:-1]).all())
    # through the constructor; no column at all: the plain trajectory and an empty aug
    traj0, aug0 = _solver(f, "euler", cfm_amd.AugmentationModule()).odeint(x0, ts)
    assert torch.equal(traj0, plain) and aug0.shape == (6, 7, 0)
    fs.augmentations = None
    assert torch.equal(fs.odeint(x0, ts), plain)
    # DSBMFlowSolver: the combined callable, on the generic path
    ds = cfm_amd.DSBMFlowSolver(f, 2, score_field=lambda t, x: -f(t, x), sigma=1.0, ode_solver="euler",
                                augmentations=cfm_amd.AugmentationModule(l2_reg=1))
    td, ad = ds.odeint(x0, ts)
    assert ds.last_path == "eager" and ad.shape == (6, 7, 1) and _rel(td.numpy(), plain.numpy()) <= 1e-12


@pytest.mark.parametrize("solver", ["euler", "rk4"])
@pytest.mark.parametrize("estimator,kw", [(None, dict(l1_reg=1, l2_reg=1, squared_l2_reg=1)),
                                          ("exact", dict(l1_reg=0.5, l2_reg=2, squared_l2_reg=1, jacobian_frobenius_reg=3)),
                                          ("exact", {})], ids=["sampler", "all", "log_prob"])
def test_cpu_float64_solve_against_the_restatement(solver, estimator, kw):
    Ws, bs = cr.mlp_params(2, 16, 3)
    x0 = np.random.default_rng(1).normal(size=(9, 2))
    ts = torch.linspace(0, 1, 6)
    am = cfm_amd.AugmentationModule(estimator, **kw)
    fs = _solver(_field64(Ws, bs), solver, am)
    traj, aug = fs.odeint(torch.tensor(x0), ts)
    mode = 0 if estimator else 2
    want = ar.trajectory64(Ws, bs, x0, ts.numpy(), mode, am.reg_mask, scheme=solver)
    a = am.aug_dims
    assert fs.last_path == "eager" and traj.dtype == torch.float64 and aug.shape == (6, 9, a)
    assert fs.nfe == 5 * (4 if solver == "rk4" else 1)
    assert _rel(traj.numpy(), want[:, :, a:]) <= 1e-10
    for k, n in enumerate(am.names):
        err = _rel(aug[:, :, k].numpy(), want[:, :, k])
        print(f"{solver} {n}: {err:.2e}")
        assert err <= 1e-10, (n, err)


@pytest.mark.parametrize("estimator", ["exact", "hutch_gaussian"])
def test_regularized_cnf_generic_gradients_with_l1_and_l2(estimator):
    d, B = 2, 9
    Ws, bs = cr.mlp_params(d, 16, 2)
    g = np.random.default_rng(2)
    cnf = cfm_amd.RegularizedCNF(cr.make_mlp(Ws, bs, dtype=torch.float64), squared_l2_reg=0.3, l1_reg=0.2, l2_reg=0.4, estimator=estimator,
                                 noise=None if estimator == "exact" else torch.tensor(g.normal(size=(B, d))))
    assert cnf.names == ["log_prob", "L1", "L2", "squared_L2"] and cnf.reg_mask == 13 and cnf.aug_dims == 4
    assert cnf.coeffs.tolist() == pytest.approx([1.0, 0.2, 0.4, 0.3])
    assert cfm_amd.cnf.REG_NAMES == ("squared_L2", "jacobian_frobenius")
    assert [n for n, _ in cfm_amd.cnf.AUG_REG_BITS] == ORDER
    xa = g.normal(size=(B, 4 + d))
    G = 0.5 + g.normal(size=(B, 4 + d))
    ts = np.linspace(1.0, 0.0, 5).astype(np.float32)
    eps = None if estimator == "exact" else cnf.noise.numpy()
    x = torch.tensor(xa, requires_grad=True)
    out = cnf.solve(x, torch.tensor(ts))
    assert cnf.last_path == "generic" and out.dtype == torch.float64
    ps = [p for l in cnf.model._linears() for p in (l.weight, l.bias)]
    got = torch.autograd.grad((out * torch.tensor(G)).sum(), ps + [x])
    out64, gp64, gx64 = ar.grads_for_upstream(Ws, bs, xa, ts, G, 0 if eps is None else 1, 13, eps)
    assert _rel(out.detach().numpy(), out64) <= 1e-10
    for a, b in zip(got, gp64 + [gx64]):
        assert _rel(a.detach().numpy(), b) <= 1e-10
    # split / loss in the reference's layout
    dl, reg, z = cnf.split(out.detach())
    assert dl.shape == (B, 1) and reg.shape == (B, 3) and z.shape == (B, d)


def test_negative_coefficient_is_refused():
    with pytest.raises(ValueError):
        cfm_amd.RegularizedCNF(cfm_amd.MLP(dim=2, time_varying=True), l1_reg=-1.0)


def test_the_header_names_the_modes_and_the_bits():
    h = open(os.path.join(ROOT, "include", "cfm_gfx950.h")).read()
    want = {"CFM_TRACE_EXACT": 0, "CFM_TRACE_HUTCH": 1, "CFM_TRACE_NONE": 2, "CFM_REG_SQUARED_L2": 1,
            "CFM_REG_JACOBIAN_FROBENIUS": 2, "CFM_REG_L1": 4, "CFM_REG_L2": 8}
    import re
    for name, value in want.items():
        m = re.search(rf"^#define {name}\s+(\d+)\b", h, re.M)
        assert m and int(m.group(1)) == value, name
    assert "#define CFM_ABI_VERSION 3" in h
    from cfm_amd import cnf
    assert (cnf.TRACE_EXACT, cnf.TRACE_HUTCH, cnf.TRACE_NONE) == (0, 1, 2)
    assert dict(cnf.AUG_REG_BITS) == ar.BITS
