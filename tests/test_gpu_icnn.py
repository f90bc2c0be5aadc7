"""GPU (-m gpu): the four ICNN operations on the HIP path (cfm_icnn_f32, csrc/icnn.hip) against the float64 restatement of
tests/icnn_restate.py, plus the properties a training loop relies on.

No rows are dropped: Softplus has no kink but the threshold at 20, where value, slope and curvature jump by about 2e-9,
and the restatement applies the same threshold.

Tolerance: per gradient tensor max|g_hip - g_64| <= max(1e-5 max|g_64|, 2^-24 S), S the largest sum
over the rows of |a row's float64 contribution| to one element (divided by B, as the gradient is); the transport map the
same with S over its layer summands; a loss 1e-5 of the mean over the rows of its summed |terms| (plus the penalty).

Measured on an MI355X (worst err / scale over the tensors of a case): 2.5e-6 on the "large" case, at most 1.3e-6 on the
others; see DESIGN.md 4.19."""
import functools

import numpy as np
import pytest
import torch

import icnn_restate as ir

pytestmark = pytest.mark.gpu

BOUND = 1e-5
ROUNDING = 2.0 ** -24
CG_MAXGRID = 256          # csrc/small_field.h: workgroups (= partial gradients) at most
MAX = 64                  # CFM_ICNN_MAX_DIM; test_constants_match checks it

# (B, d, dimh, L, kind, reg): "large" scales the inputs by 30, "neg" makes every Wzs entry negative
CASES = [
    (1, 2, 64, 4, "plain", 0.1),
    (16, 2, 64, 4, "plain", 0.1),
    (17, 5, 33, 4, "plain", 0.1),
    (40, 1, 64, 2, "plain", 0.1),
    (40, 16, 64, 3, "plain", 0.1),
    (40, MAX, 64, 4, "plain", 0.1),
    (17, MAX, 33, 4, "plain", 0.1),
    (100, 3, 1, 2, "plain", 0.1),
    (16 * CG_MAXGRID + 5, 2, 64, 4, "plain", 0.1),
    (40, 2, 64, 4, "large", 0.1),
    (40, 2, 64, 4, "neg", 0.1),
    (40, 2, 64, 4, "plain", 0.0),
]
IDS = ["B%d_d%d_h%d_L%d_%s_reg%g" % c for c in CASES]


def _f32(P):
    return {k: v.astype(np.float32).astype(np.float64) for k, v in P.items()}


@functools.lru_cache(maxsize=None)
def _case(B, d, H, L, kind, reg):
    """fp32-representable parameters and inputs, and the float64 reference (computed once, shared, never written to)"""
    sign = -1 if kind == "neg" else 0
    Pf, Pg = _f32(ir.gen_params(21, d, H, L, sign)), _f32(ir.gen_params(22, d, H, L, sign))
    x, y = ir.gen_data(23, B, d, scale=30.0 if kind == "large" else 1.0)
    x, y = x.astype(np.float32).astype(np.float64), y.astype(np.float32).astype(np.float64)
    ref = {"T": ir.transport(Pf, x, with_S=True), "w2": ir.w2(Pf, Pg, x, y), "f": ir.f_step(Pf, Pg, x, y, reg),
           "g": ir.g_step(Pf, Pg, x, y, reg)}
    for a in (x, y, *Pf.values(), *Pg.values()):
        a.setflags(write=False)
    return Pf, Pg, x, y, ref


def _net(P, dev, dtype=torch.float32):
    import cfm_amd
    L = len([k for k in P if k.startswith("Wzs.")]) - 2
    H, d = P["Wzs.0.weight"].shape
    n = cfm_amd.ICNN(dim=d, dimh=H, num_hidden_layers=L)
    n.load_state_dict({k: torch.tensor(v) for k, v in P.items()}, strict=True)
    return n.to(device=dev, dtype=dtype)


def _T(v, dev, dtype=torch.float32):
    return torch.tensor(np.asarray(v), device=dev, dtype=dtype)


def _run(Pf, Pg, x, y, reg, dev, dtype=torch.float32):
    """the four operations through the public functions, as float64 numpy, and the paths that ran"""
    import cfm_amd
    f, g = _net(Pf, dev, dtype), _net(Pg, dev, dtype)
    xt, yt = _T(x, dev, dtype), _T(y, dev, dtype)
    out, paths = {}, []
    out["T"] = f.transport(xt).cpu().double().numpy()
    paths.append(cfm_amd.ICNN.transport.last_path)
    out["w2"] = [float(v) for v in cfm_amd.icnn_w2(f, g, xt, yt, return_loss=True)]
    paths.append(cfm_amd.icnn_w2.last_path)
    for key, fn, net, other in (("f", cfm_amd.icnn_f_loss, f, g), ("g", cfm_amd.icnn_g_loss, g, f)):
        loss = fn(f, g, xt, yt, reg=reg)
        paths.append(fn.last_path)
        loss.backward()
        assert all(p.grad is None for p in other.parameters()), key
        out[key] = (float(loss.detach()), {k: p.grad.detach().cpu().double().numpy() for k, p in net.named_parameters()})
        net.zero_grad(set_to_none=True)
    return out, paths


def _check(tag, out, ref, bound=BOUND):
    """prints every figure before it asserts"""
    bad, line = [], []
    g64, S = ref["T"]
    err, scale, floor = np.abs(out["T"] - g64).max(), np.abs(g64).max(), ROUNDING * S.max()
    line.append(f"T {err / scale:.2e} (floor {floor / scale:.1e})")
    if err > max(bound * scale, floor):
        bad.append(("T", err, scale, floor))
    for k, (v, want, mag) in enumerate(zip(out["w2"], *ref["w2"])):
        line.append(f"w2[{k}] {abs(v - want) / mag:.2e}")
        if abs(v - want) > bound * mag:
            bad.append(("w2", k, v, want, mag))
    for key in ("f", "g"):
        l64, G64, S64, mag = ref[key][:4]
        loss, G = out[key]
        line.append(f"{key}_loss {abs(loss - l64) / mag:.2e}")
        if abs(loss - l64) > bound * mag:
            bad.append((key, "loss", loss, l64, mag))
        assert sorted(G) == sorted(G64)
        for k in G64:
            err, scale, floor = np.abs(G[k] - G64[k]).max(), np.abs(G64[k]).max(), ROUNDING * S64[k]
            line.append(f"{key}.{k} {err / max(scale, 1e-300):.2e} (floor {floor / max(scale, 1e-300):.1e})")
            if err > max(bound * scale, floor):
                bad.append((key, k, err, scale, floor))
    print(f"{tag}: " + " ".join(line))
    assert not bad, bad


def test_constants_match():
    import cfm_amd
    assert cfm_amd.icnn.HIP_MAX_DIM == MAX


def test_the_large_case_saturates_softplus_on_both_sides():
    Pf, Pg, x, y, ref = _case(*CASES[9])
    for P, pts in ((Pf, x), (Pg, y)):
        a = np.concatenate([z.ravel() for z in ir.forward(P, pts)[1]])
        assert (a > 20).mean() >= 0.10 and (a < -20).mean() >= 0.10, ((a > 20).mean(), (a < -20).mean())


def test_the_negative_case_has_a_dense_penalty():
    Pf, Pg, x, y, ref = _case(*CASES[10])
    assert all((v < 0).all() for P in (Pf, Pg) for k, v in P.items() if k.startswith("Wzs.") and k.endswith(".weight"))


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_four_operations_against_float64(case):
    Pf, Pg, x, y, ref = _case(*case)
    dev = torch.device("cuda")
    out, paths = _run(Pf, Pg, x, y, case[5], dev)
    assert paths == ["hip"] * 4
    assert np.isfinite(out["T"]).all() and all(np.isfinite(g).all() for key in "fg" for g in out[key][1].values())
    _check(IDS[CASES.index(case)], out, ref)
    again, paths = _run(Pf, Pg, x, y, case[5], dev)
    assert paths == ["hip"] * 4
    assert np.array_equal(out["T"], again["T"]) and out["w2"] == again["w2"]
    for key in "fg":
        assert out[key][0] == again[key][0]
        for k, v in out[key][1].items():
            assert np.array_equal(v, again[key][1][k]), (key, k)


def test_reg_zero_leaves_the_data_gradient_alone():
    """with reg = 0 the gradient is the data term's bit for bit: the penalty adds nothing, not even a rounding"""
    Pf, Pg, x, y, _ = _case(*CASES[11])
    dev = torch.device("cuda")
    a, _ = _run(Pf, Pg, x, y, 0.0, dev)
    b, _ = _run(Pf, Pg, x, y, 0.1, dev)
    for key in "fg":
        for k, v in a[key][1].items():
            if k.startswith("Wzs.") and k.endswith(".weight"):
                P = Pf if key == "f" else Pg
                want = v.astype(np.float32) - np.float32(0.1) * np.maximum(-P[k].astype(np.float32), np.float32(0))
                assert np.array_equal(want.astype(np.float64), b[key][1][k]), (key, k)
            else:
                assert np.array_equal(v, b[key][1][k]), (key, k)


def test_upstream_scalar_scales_and_a_second_backward_raises():
    import cfm_amd
    Pf, Pg, x, y, _ = _case(*CASES[1])
    dev = torch.device("cuda")
    f, g = _net(Pf, dev), _net(Pg, dev)
    xt, yt = _T(x, dev), _T(y, dev)
    for fn, net in ((cfm_amd.icnn_f_loss, f), (cfm_amd.icnn_g_loss, g)):
        fn(f, g, xt, yt).backward()
        assert fn.last_path == "hip"
        once = [p.grad.clone() for p in net.parameters()]
        net.zero_grad(set_to_none=True)
        (2 * fn(f, g, xt, yt)).backward()
        for p, q in zip(net.parameters(), once):
            assert torch.equal(p.grad, 2 * q)
        net.zero_grad(set_to_none=True)
        loss = fn(f, g, xt, yt)
        gs = torch.autograd.grad(loss, list(net.parameters()), create_graph=True)
        with pytest.raises(RuntimeError):
            gs[0].sum().backward()
    assert all(p.grad is None for p in g.parameters())


@pytest.mark.parametrize("how", ["d_over", "L5", "float64", "fused_off"])
def test_outside_the_envelope_the_generic_path_agrees(how):
    from cfm_amd import _lib
    dev = torch.device("cuda")
    B, d, H, L = 40, 2, 64, 4
    if how == "d_over":
        d = MAX + 1
    if how == "L5":
        L = 5
    dtype = torch.float64 if how == "float64" else torch.float32
    Pf, Pg, x, y, ref = _case(B, d, H, L, "plain", 0.1)
    lib = _lib.load()
    if how == "fused_off":
        lib.cfm_ode_set_fused(0)
    try:
        out, paths = _run(Pf, Pg, x, y, 0.1, dev, dtype)
    finally:
        lib.cfm_ode_set_fused(1)
    assert paths == ["generic"] * 4
    _check("generic " + how, out, ref)
    if how in ("float64", "fused_off"):
        hip, paths = _run(Pf, Pg, x, y, 0.1, dev)
        assert paths == ["hip"] * 4
        _check("hip beside " + how, hip, ref)


def test_ten_adam_steps_track_the_float64_generic_path():
    """the reference's alternation (a g-step, then an f-step; Adam lr 1e-4, betas (0.5, 0.9)) for ten rounds"""
    import cfm_amd
    dev = torch.device("cuda")
    B, d, H, L = 64, 2, 64, 4
    Pf, Pg = _f32(ir.gen_params(31, d, H, L)), _f32(ir.gen_params(32, d, H, L))
    x, y = ir.gen_data(33, B, d)
    x, y = x.astype(np.float32), y.astype(np.float32)
    result = []
    for dtype in (torch.float32, torch.float64):
        f, g = _net(Pf, dev, dtype), _net(Pg, dev, dtype)
        xt, yt = _T(x, dev, dtype), _T(y, dev, dtype)
        fo = torch.optim.Adam(f.parameters(), lr=1e-4, betas=(0.5, 0.9))
        go = torch.optim.Adam(g.parameters(), lr=1e-4, betas=(0.5, 0.9))
        for _ in range(10):
            for fn, opt in ((cfm_amd.icnn_g_loss, go), (cfm_amd.icnn_f_loss, fo)):
                opt.zero_grad(set_to_none=True)
                fn(f, g, xt, yt, reg=0.1).backward()
                assert fn.last_path == ("hip" if dtype == torch.float32 else "generic")
                opt.step()
        result.append({k: p.detach().cpu().double().numpy() for n, net in (("f", f), ("g", g)) for k, p in
                       ((n + "." + k, p) for k, p in net.named_parameters())})
    worst = 0.0
    for k, v in result[1].items():
        rel = np.abs(result[0][k] - v).max() / np.abs(v).max()
        worst = max(worst, rel)
        assert rel <= 1e-4, (k, rel)
    print(f"ten Adam rounds: worst relative parameter difference {worst:.2e}")
