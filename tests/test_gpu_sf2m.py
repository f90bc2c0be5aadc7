"""GPU: the [SF]2M training step (cfm_mlp_sf2m_step_f32 / cfm_amd.SF2MStep) — a flow net and a score net in the launches
of one regression step — against float64 autograd of the reference's lines, against the recorded float64 run of the
reference's own loop (tests/golden/sf2m_cases.npz), and bit for bit against the one-net step it is built from."""
import copy
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

NAMES = ("net.0.weight", "net.0.bias", "net.2.weight", "net.2.bias", "net.4.weight", "net.4.bias", "net.6.weight", "net.6.bias")


@pytest.fixture(scope="module")
def dev():
    from cfm_amd import _lib
    _lib.load()
    return _lib.require_gpu()


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "sf2m_cases.npz"))


def _rel(a, b):
    return float((a - b).abs().max() / b.abs().max())


def _params(*nets):
    return [p for n in nets for p in n.parameters()]


def _f64(flow, score, t, xt, ut, eps, lam, score_weight=1.0):
    """the reference's lines in float64 on the host: (flow_loss, score_loss, gradients flow first)"""
    f, s = copy.deepcopy(flow).double().cpu(), copy.deepcopy(score).double().cpu()
    for p in _params(f, s):
        p.grad = None
    x = xt.double().cpu() if t is None else torch.cat([xt.double().cpu(), t.double().cpu()[:, None]], dim=-1)
    fl = torch.mean((f.net(x) - ut.double().cpu()) ** 2)
    sl = torch.mean((lam.double().cpu()[:, None] * s.net(x) + eps.double().cpu()) ** 2)
    (fl + score_weight * sl).backward()
    return float(fl.detach()), float(sl.detach()), [p.grad for p in _params(f, s)]


def _random_case(dev, B, d, w, seed, tv=True, layers=None):
    """seeded nets and a batch shaped like the matcher's: lambda_t = 2 sqrt(t (1 - t)) / sigma at sigma = 0.5 (<= 2)"""
    import cfm_amd
    torch.manual_seed(seed)
    nets = []
    for _ in range(2):
        net = cfm_amd.MLP(dim=d, time_varying=tv, w=w)
        if layers is not None:
            widths = [d + int(tv)] + [w] * (layers - 1) + [d]
            mods = []
            for k in range(layers):
                mods += ([torch.nn.SELU()] if k else []) + [torch.nn.Linear(widths[k], widths[k + 1])]
            net.net = torch.nn.Sequential(*mods)
        nets.append(net.to(dev))
    t = torch.rand(B, device=dev)
    xt = torch.randn(B, d, device=dev); ut = torch.randn(B, d, device=dev); eps = torch.randn(B, d, device=dev)
    lam = 2 * torch.sqrt(t * (1 - t)) / 0.5
    return nets[0], nets[1], (t if tv else None, xt, ut, eps, lam)


def _golden_case(dev, z, case, k=0):
    import cfm_amd
    B, d, w, sigma = z[f"{case}_meta"]
    nets = []
    for tag in ("flow", "score"):
        net = cfm_amd.MLP(dim=int(d), w=int(w), time_varying=True)
        net.load_state_dict({n: torch.from_numpy(z[f"{case}_{tag}_{n}"]) for n in NAMES})
        nets.append(net.to(dev))
    return nets[0], nets[1], _golden_batch(dev, z, case, k)


def _golden_batch(dev, z, case, k):
    return tuple(torch.from_numpy(z[f"{case}_b{k}_{n}"]).to(dev) for n in ("t", "xt", "ut", "eps", "lam"))


def _step(flow, score, score_weight=1.0, lr=1e-3):
    import cfm_amd
    return cfm_amd.SF2MStep(flow, score, cfm_amd.FusedAdam(_params(flow, score), lr=lr), score_weight=score_weight)


def _check_vs_f64(flow, score, losses, want_fl, want_sl, want_grads, what):
    fl, sl = (float(v) for v in losses.cpu())
    devs = [abs(fl - want_fl) / abs(want_fl), abs(sl - want_sl) / abs(want_sl)]
    devs += [_rel(p.grad.double().cpu(), g) for p, g in zip(_params(flow, score), want_grads)]
    print(f"{what}: losses {devs[0]:.2e} {devs[1]:.2e}, gradients max {max(devs[2:]):.2e}")
    assert max(devs) <= 1e-5, devs


@pytest.mark.parametrize("case", ["s1", "s01"])
def test_fixture_gradients_and_losses_match_the_recorded_float64(dev, golden, case):
    """step 0 of the reference's own loop (float64, recorded): both losses and every gradient <= 1e-5 relative"""
    flow, score, batch = _golden_case(dev, golden, case)
    losses = _step(flow, score).backward_only(*batch)
    want = [torch.from_numpy(golden[f"{case}_grad0_{tag}_{n}"]) for tag in ("flow", "score") for n in NAMES]
    _check_vs_f64(flow, score, losses, golden[f"{case}_losses"][0, 0], golden[f"{case}_losses"][0, 1], want, case)


# (130, 7, 33): ragged tiles, odd widths, scalar loads, unpaired backward launches; (512, 20, 64): a direct-to-LDS hidden
# layer, a register-staged first layer, a paired backward; (512, 784, 512): the 785-wide 4-byte-aligned rows of the
# direct-to-LDS engine; (64, 3, 16) x 7 layers: the final reduction's table at its bound (32 of 34 jobs)
@pytest.mark.parametrize("B,d,w,layers", [(130, 7, 33, None), (512, 20, 64, None), (512, 784, 512, None), (64, 3, 16, 7)])
def test_gradients_and_losses_match_float64_autograd(dev, B, d, w, layers):
    flow, score, batch = _random_case(dev, B, d, w, seed=B + d, layers=layers)
    losses = _step(flow, score).backward_only(*batch)
    fl, sl, grads = _f64(flow, score, *batch)
    _check_vs_f64(flow, score, losses, fl, sl, grads, f"({B}, {d}, {w}, {layers})")


@pytest.mark.parametrize("B,d,w", [(256, 2, 64), (512, 20, 64)])
def test_each_half_is_bit_equal_to_the_one_net_step(dev, B, d, w):
    """Every product's kernel is chosen per net as if it ran alone, so: the flow net's gradients and loss are the bits
    of RegressionStep on (t, xt, ut); with lambda_t = 1 and score_weight = 1 the score net's are its bits on -eps."""
    import cfm_amd
    flow, score, (t, xt, ut, eps, lam) = _random_case(dev, B, d, w, seed=31 + B)
    fc, sc = copy.deepcopy(flow), copy.deepcopy(score)
    step = _step(flow, score)
    losses = step.backward_only(t, xt, ut, eps, lam).clone()
    gflow = [p.grad.clone() for p in flow.parameters()]
    one = cfm_amd.RegressionStep(fc, cfm_amd.FusedAdam(fc.parameters()))
    lf = one.backward_only(t, xt, ut)
    assert float(lf) == float(losses[0])
    assert all(torch.equal(a, p.grad) for a, p in zip(gflow, fc.parameters()))
    # lambda = 1: the flow half does not move, the score half is the plain step on u = -eps
    l1 = step.backward_only(t, xt, ut, eps, torch.ones_like(lam)).clone()
    assert float(l1[0]) == float(losses[0]) and all(torch.equal(a, p.grad) for a, p in zip(gflow, flow.parameters()))
    one_s = cfm_amd.RegressionStep(sc, cfm_amd.FusedAdam(sc.parameters()))
    ls = one_s.backward_only(t, xt, -eps)
    assert float(ls) == float(l1[1])
    assert all(torch.equal(p.grad, q.grad) for p, q in zip(score.parameters(), sc.parameters()))


def test_score_weight_scales_the_score_gradients_only(dev):
    B, d, w = 512, 20, 64
    flow, score, batch = _random_case(dev, B, d, w, seed=77)
    base = _step(flow, score)
    l_one = base.backward_only(*batch).clone()
    gflow = [p.grad.clone() for p in flow.parameters()]
    half = _step(flow, score, score_weight=0.5)
    l_half = half.backward_only(*batch).clone()
    assert torch.equal(l_one, l_half)                                  # both losses are reported unweighted
    assert all(torch.equal(a, p.grad) for a, p in zip(gflow, flow.parameters()))
    fl, sl, grads = _f64(flow, score, *batch, score_weight=0.5)
    _check_vs_f64(flow, score, l_half, fl, sl, grads, "score_weight 0.5")
    assert abs(float(half.loss()) - (fl + 0.5 * sl)) <= 1e-5 * (fl + 0.5 * sl)
    assert abs(float(base.loss()) - (fl + sl)) <= 1e-5 * (fl + sl)


def test_the_same_call_twice_gives_the_same_bits(dev):
    flow, score, batch = _random_case(dev, 512, 20, 64, seed=5)
    step = _step(flow, score)
    a = step.backward_only(*batch).clone(); ga = [p.grad.clone() for p in _params(flow, score)]
    b = step.backward_only(*batch)
    assert torch.equal(a, b) and all(torch.equal(x, p.grad) for x, p in zip(ga, _params(flow, score)))


@pytest.mark.parametrize("case", ["s1", "s01"])
def test_five_steps_track_the_recorded_float64_loop(dev, golden, case):
    """SF2MStep + one FusedAdam(lr=1e-3) over both nets on the recorded batches: both loss sequences within 1e-4 relative
    of the reference's loop in float64 (its own float32 loop: <= 5e-7)"""
    flow, score, _ = _golden_case(dev, golden, case)
    step = _step(flow, score, lr=1e-3)
    got = np.asarray([step(*_golden_batch(dev, golden, case, k)).cpu().numpy().astype(np.float64) for k in range(5)])
    want = golden[f"{case}_losses"]
    rel = np.abs(got - want) / np.abs(want)
    print(f"{case}: five-step losses vs float64, max relative {rel.max():.2e}")
    assert rel.max() <= 1e-4, rel
    assert all(int(st["step"]) == 5 for st in step.opt.state.values()) and len(step.opt.state) == 16


def test_without_time_column_against_the_autograd_path(dev):
    """same forward kernels on both sides (no time column to round differently): the losses differ by the order of their
    sums and, for the score loss, by the one rounding of fma(lam, s, e) against mul + add — a few fp32 ulps, bound 1e-6
    (16 ulps) as for the one-net step; gradients 1e-5 of the largest entry"""
    flow, score, (t, xt, ut, eps, lam) = _random_case(dev, 200, 6, 32, seed=7, tv=False)
    assert t is None
    losses = _step(flow, score).backward_only(None, xt, ut, eps, lam).clone()
    g = [p.grad.clone() for p in _params(flow, score)]
    for p in _params(flow, score):
        p.grad = None
    fl = torch.mean((flow(xt) - ut) ** 2); sl = torch.mean((lam[:, None] * score(xt) + eps) ** 2)
    (fl + sl).backward()
    assert abs(float(fl.detach()) - float(losses[0])) <= 1e-6 * float(losses[0])
    assert abs(float(sl.detach()) - float(losses[1])) <= 1e-6 * float(losses[1])
    for a, p in zip(g, _params(flow, score)):
        assert (a - p.grad).abs().max() <= 1e-5 * p.grad.abs().max()


def test_refusals(dev, monkeypatch):
    from cfm_amd import _lib
    flow, score, (t, xt, ut, eps, lam) = _random_case(dev, 64, 3, 16, seed=1, layers=8)
    step = _step(flow, score)
    with pytest.raises(RuntimeError, match="at most 7"):
        step.backward_only(t, xt, ut, eps, lam)
    step.MAX_LAYERS = 16                                             # past the Python check: the C call refuses too
    with pytest.raises(_lib.CfmBackendError, match="CFM_EINVAL"):
        step.backward_only(t, xt, ut, eps, lam)
    flow, score, (t, xt, ut, eps, lam) = _random_case(dev, 64, 3, 16, seed=1)
    step = _step(flow, score)
    with pytest.raises(RuntimeError, match="lambda_t has 63 values for 64 rows"):
        step.backward_only(t, xt, ut, eps, lam[:63])
    with pytest.raises(RuntimeError, match="eps has shape"):
        step.backward_only(t, xt, ut, eps[:, :2], lam)
    import torch.distributed as dist
    monkeypatch.setattr(dist, "is_initialized", lambda: True)
    monkeypatch.setattr(dist, "get_world_size", lambda *a, **k: 2)
    before = [p.detach().clone() for p in _params(flow, score)]
    with pytest.raises(NotImplementedError, match="data parallel"):
        step(t, xt, ut, eps, lam)
    assert all(torch.equal(a, p) for a, p in zip(before, _params(flow, score)))
