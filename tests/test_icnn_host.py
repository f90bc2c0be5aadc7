"""CPU: the ICNN model, the generic path and the hand-derived restatement against float64 autograd through the
reference's own class (tests/golden/icnn_reference.json, written by tools/make_icnn_golden.py), the descriptor of
cfm_icnn_f32 against the header's text, and the entry's refusals, which it makes before any HIP call."""
import ctypes
import json
import os
import re

import numpy as np
import pytest
import torch

import icnn_restate as ir

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-12
CG_MAXGRID = 256          # csrc/small_field.h: workgroups (= partial gradients) at most


@pytest.fixture(scope="module")
def golden(golden_dir):
    return json.load(open(os.path.join(golden_dir, "icnn_reference.json")))


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


def _nets(golden):
    import cfm_amd
    nets = []
    for key in ("f", "g"):
        n = cfm_amd.ICNN(golden["dim"], golden["dimh"], golden["num_hidden_layers"]).double()
        n.load_state_dict({k: torch.tensor(v, dtype=torch.float64) for k, v in golden[key].items()}, strict=True)
        nets.append(n)
    return nets


def test_fixture_is_the_seeded_case_with_both_signs(golden):
    Pf, Pg, x, y, reg = ir.golden_case()
    assert (golden["dim"], golden["dimh"], golden["num_hidden_layers"], golden["reg"]) == (2, 8, 4, reg) and len(x) == 6
    assert _rel(x, golden["x"]) == 0 and _rel(y, golden["y"]) == 0
    for P, key in ((Pf, "f"), (Pg, "g")):
        for k, v in P.items():
            assert _rel(v, golden[key][k]) == 0
            if k.startswith("Wzs.") and k.endswith(".weight"):
                assert (v < 0).any() and (v > 0).any()
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "icnn_reference.json")) < 100 * 1024


def test_state_dict_is_the_references(golden):
    import cfm_amd
    net = cfm_amd.ICNN(golden["dim"], golden["dimh"], golden["num_hidden_layers"])
    assert [[k, list(v.shape)] for k, v in net.state_dict().items()] == golden["keys"]
    assert [k for k, _ in net.named_parameters()] == ir.names(4)
    L = 4
    assert net.Wzs[0].bias is not None and all(net.Wzs[l].bias is None for l in range(1, L + 1))
    assert all(net.Wxs[l].bias is not None for l in range(L - 1)) and net.Wxs[L - 1].bias is None
    assert isinstance(net.act, torch.nn.Softplus) and net.act.beta == 1 and net.act.threshold == 20
    for d, H, L in ((3, 5, 2), (1, 1, 3)):
        n = cfm_amd.ICNN(dim=d, dimh=H, num_hidden_layers=L)
        assert {k: tuple(v.shape) for k, v in n.state_dict().items()} == ir.shapes(d, H, L)
        assert n(torch.zeros(4, d)).shape == (4, 1)


def test_generic_path_matches_the_fixture_in_float64(golden):
    import cfm_amd
    f, g = _nets(golden)
    x, y = torch.tensor(golden["x"], dtype=torch.float64), torch.tensor(golden["y"], dtype=torch.float64)
    assert _rel(f(x)[:, 0].detach(), golden["f_out"]) <= TOL
    assert _rel(f.transport(x), golden["f_transport"]) <= TOL and _rel(g.transport(y), golden["g_transport"]) <= TOL
    assert cfm_amd.ICNN.transport.last_path == "generic"
    loss = cfm_amd.icnn_g_loss(f, g, x, y, reg=golden["reg"])
    loss.backward()
    assert cfm_amd.icnn_g_loss.last_path == "generic" and loss.shape == ()
    assert abs(loss.item() - golden["g_loss"]) <= TOL * abs(golden["g_loss"])
    for k, p in g.named_parameters():
        assert _rel(p.grad, golden["g_grads"][k]) <= TOL, k
    assert all(p.grad is None for p in f.parameters())
    g.zero_grad(set_to_none=True)
    loss = cfm_amd.icnn_f_loss(f, g, x, y, reg=golden["reg"])
    loss.backward()
    assert cfm_amd.icnn_f_loss.last_path == "generic"
    assert abs(loss.item() - golden["f_loss"]) <= TOL * abs(golden["f_loss"])
    for k, p in f.named_parameters():
        assert _rel(p.grad, golden["f_grads"][k]) <= TOL, k
    assert all(p.grad is None for p in g.parameters())
    vals = cfm_amd.icnn_w2(f, g, x, y, return_loss=True)
    assert cfm_amd.icnn_w2.last_path == "generic" and not any(v.requires_grad for v in vals)
    for v, want in zip(vals, golden["w2"]):
        assert abs(v.item() - want) <= TOL * abs(want)
    assert cfm_amd.icnn_w2(f, g, x, y).item() == vals[0].item()


def test_generic_path_is_twice_differentiable_and_reg_zero_has_no_penalty(golden):
    import cfm_amd
    f, g = _nets(golden)
    x, y = torch.tensor(golden["x"], dtype=torch.float64), torch.tensor(golden["y"], dtype=torch.float64)
    loss = cfm_amd.icnn_g_loss(f, g, x, y, reg=0.0)
    (g0,) = torch.autograd.grad(loss, g.Wzs[1].weight, create_graph=True)
    g0.square().sum().backward()
    assert g.Wzs[1].weight.grad is not None
    Pf, Pg, xs, ys, _ = ir.golden_case()
    assert abs(loss.item() - ir.g_step(Pf, Pg, xs, ys, 0.0)[0]) <= TOL * abs(loss.item())


def test_restatement_matches_the_fixture(golden):
    """the hand-derived sweeps of DESIGN.md 4.19, the g-step's double backward included, against autograd"""
    Pf, Pg, x, y, reg = ir.golden_case()
    assert _rel(ir.forward(Pf, x)[0], golden["f_out"]) <= TOL
    assert _rel(ir.transport(Pf, x), golden["f_transport"]) <= TOL and _rel(ir.transport(Pg, y), golden["g_transport"]) <= TOL
    lf, Gf, Sf, _ = ir.f_step(Pf, Pg, x, y, reg)
    lg, Gg, Sg, _, p, w = ir.g_step(Pf, Pg, x, y, reg)
    assert abs(lf - golden["f_loss"]) <= TOL * abs(lf) and abs(lg - golden["g_loss"]) <= TOL * abs(lg)
    assert sorted(Gf) == sorted(Gg) == sorted(golden["f_grads"])
    for k in Gf:
        assert _rel(Gf[k], golden["f_grads"][k]) <= TOL, k
        assert _rel(Gg[k], golden["g_grads"][k]) <= TOL, k
        assert Sf[k] > 0 and Sg[k] > 0
    assert _rel(ir.w2(Pf, Pg, x, y)[0], golden["w2"]) <= TOL
    assert _rel(p, golden["g_transport"]) <= TOL and _rel(w, ir.transport(Pf, p) - y) == 0


def test_restatement_applies_torchs_softplus_threshold():
    z = torch.tensor([-800.0, -30.0, -1.0, 0.0, 1.0, 19.999, 20.0, 20.001, 90.0, 3e38], dtype=torch.float64, requires_grad=True)
    h = torch.nn.functional.softplus(z)
    (s,) = torch.autograd.grad(h.sum(), z, create_graph=True)
    (q,) = torch.autograd.grad(s.sum(), z)
    zn = z.detach().numpy()
    with np.errstate(over="raise", invalid="raise"):
        hn, sn, qn = ir.softplus(zn), ir.sigma(zn), ir.sigma_slope(zn)
    assert np.allclose(hn, h.detach().numpy(), rtol=1e-14, atol=0) and np.allclose(sn, s.detach().numpy(), rtol=1e-14, atol=1e-300)
    # autograd forms 1 - sigma by subtraction (1e-8 relative at z = 19.999), and AT z = 20 its second derivative already
    # takes the linear branch while its first does not: a point of measure zero, left out
    keep = zn != 20.0
    assert np.allclose(qn[keep], q.numpy()[keep], rtol=1e-7, atol=1e-300)
    assert sn[7] == 1.0 and qn[7] == 0.0 and hn[7] == zn[7] and sn[6] < 1.0


def _struct_fields(src, name):
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), src, flags=re.S).group(1)
    out = []
    for decl in body.split(";"):
        decl = " ".join(decl.split())
        if not decl:
            continue
        m = re.fullmatch(r"(.+?)\s*\b(\w+)(?:\[(\d+)\])?", decl)
        out.append((m.group(2), " ".join(m.group(1).split()), int(m.group(3)) if m.group(3) else 0))
    return out


def test_descriptor_mirrors_the_header(lib_built):
    src = open(os.path.join(ROOT, "include", "cfm_gfx950.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    ctype = {"size_t": ctypes.c_size_t, "int": ctypes.c_int, "float": ctypes.c_float, "cfm_icnn_net": lib_built.IcnnNet}
    for name, struct in (("cfm_icnn_net", lib_built.IcnnNet), ("cfm_icnn_call", lib_built.IcnnCall)):
        want = []
        for field, typ, n in _struct_fields(src, name):
            t = ctypes.c_void_p if typ.endswith("*") else ctype[typ]
            want.append((field, t * n if n else t))
        have = [(f, t) for f, t in struct._fields_]
        assert [f for f, _ in have] == [f for f, _ in want]
        for (f, a), (_, b) in zip(have, want):
            assert ctypes.sizeof(a) == ctypes.sizeof(b) and (a is b or (hasattr(a, "_length_") and a._length_ == b._length_)), f
    assert lib_built.IcnnCall._fields_[0][0] == "size" and lib_built.IcnnCall._fields_[-1][0] == "stream"
    assert ctypes.sizeof(lib_built.IcnnNet) == 8 * 26
    assert re.search(r"#define CFM_OP_ICNN\s+13\b", src) and lib_built.OP_ICNN == 13
    assert int(re.search(r"#define CFM_ICNN_MAX_DIM\s+(\d+)", src).group(1)) == lib_built.ICNN_MAX_DIM
    for k, name in enumerate(("TRANSPORT", "W2", "F_STEP", "G_STEP")):
        assert int(re.search(r"#define CFM_ICNN_%s\s+(\d+)" % name, src).group(1)) == k == getattr(lib_built, "ICNN_" + name)
    import cfm_amd
    assert 16 <= cfm_amd.icnn.HIP_MAX_DIM == lib_built.ICNN_MAX_DIM <= 64
    assert lib_built.SIGNATURES["cfm_icnn_f32"] == (ctypes.c_int, [ctypes.c_void_p])


def _valid_call(lib_built, op=3, d=2, dimh=64, L=4, B=8):
    """a descriptor whose every operand is a non-null address: only calls that the entry refuses are made with it"""
    c = lib_built.IcnnCall()
    c.size = ctypes.sizeof(lib_built.IcnnCall)
    c.op, c.d, c.dimh, c.L, c.B, c.reg = op, d, dimh, L, B, 0.1
    for net in (c.f, c.g):
        for name, typ in lib_built.IcnnNet._fields_:
            if hasattr(typ, "_length_"):
                arr = getattr(net, name)
                for k in range(typ._length_):
                    arr[k] = 0x1000
            else:
                setattr(net, name, 0x1000)
    for name in ("x", "y", "p", "w", "losses", "ws"):
        setattr(c, name, 0x1000)
    return c


def test_entry_refuses_before_any_hip_call(lib_built):
    """no GPU here: a refusal that came after a HIP call would not come back as CFM_EINVAL"""
    lib = lib_built.load()
    MAX = lib_built.ICNN_MAX_DIM
    assert lib.cfm_icnn_f32(None) == -1
    bad = [dict(L=1), dict(L=5), dict(dimh=0), dict(dimh=65), dict(d=0), dict(d=MAX + 1), dict(op=-1), dict(op=4), dict(B=0)]
    for kw in bad:
        assert lib.cfm_icnn_f32(ctypes.byref(_valid_call(lib_built, **kw))) == -1, kw
    for delta in (-8, 8):
        c = _valid_call(lib_built)
        c.size += delta
        assert lib.cfm_icnn_f32(ctypes.byref(c)) == -1
    for op in (0, 1, 2):
        c = _valid_call(lib_built, op=op)
        c.x = None
        assert lib.cfm_icnn_f32(ctypes.byref(c)) == -1, op
    for op, field in ((3, "y"), (3, "w"), (2, "losses"), (1, "ws"), (0, "p")):
        c = _valid_call(lib_built, op=op)
        setattr(c, field, None)
        assert lib.cfm_icnn_f32(ctypes.byref(c)) == -1, (op, field)
    c = _valid_call(lib_built, op=3)
    c.g.dWz[2] = None
    assert lib.cfm_icnn_f32(ctypes.byref(c)) == -1
    c = _valid_call(lib_built, op=2)
    c.f.bz0 = None
    assert lib.cfm_icnn_f32(ctypes.byref(c)) == -1
    lib.cfm_ode_set_fused(0)
    try:
        assert lib.cfm_icnn_f32(ctypes.byref(_valid_call(lib_built))) == -1
    finally:
        lib.cfm_ode_set_fused(1)


def test_workspace_bytes(lib_built):
    lib = lib_built.load()
    assert lib.cfm_workspace_bytes(13, 0, 0, 0) == 0 and lib.cfm_workspace_bytes(13, -3, 0, 0) == 0
    sizes = [lib.cfm_workspace_bytes(13, B, 0, 0) for B in (1, 16, 17, 256, 16 * CG_MAXGRID - 1, 16 * CG_MAXGRID, 16 * CG_MAXGRID + 5, 10 ** 6)]
    assert all(n > 0 and n % 256 == 0 for n in sizes) and sizes == sorted(sizes)
    assert sizes[0] == sizes[1] < sizes[2] and sizes[4] == sizes[5] == sizes[6] == sizes[7]
    # one partial per workgroup: 8 loss terms and the widest net's gradient
    P = 8 + 4 * 64 * lib_built.ICNN_MAX_DIM + 4 * 64 + 3 * 64 * 64 + 64 + lib_built.ICNN_MAX_DIM
    assert sizes[-1] == 4 * CG_MAXGRID * P and sizes[0] == -(-4 * P // 256) * 256


def test_mismatched_columns_raise_before_any_path_is_chosen(golden):
    """data whose column count is not the nets' dim: the kernels index every buffer as [B, dim], so nothing may reach them"""
    import cfm_amd
    from cfm_amd import icnn
    f, g = _nets(golden)
    good = torch.zeros(6, 2, dtype=torch.float64)
    for cols in (1, 3):
        bad = torch.zeros(6, cols, dtype=torch.float64)
        for fn in (cfm_amd.icnn_g_loss, cfm_amd.icnn_f_loss, cfm_amd.icnn_w2):
            with pytest.raises(ValueError, match="columns"):
                fn(f, g, bad, bad)
            with pytest.raises(ValueError):
                fn(f, g, good, bad)
        with pytest.raises(ValueError):
            f.transport(bad)
        assert not icnn._hip_ok((f, g), (bad.float(), bad.float()))
    other = cfm_amd.ICNN(3, 8, 4).double()
    with pytest.raises(ValueError, match="columns"):
        cfm_amd.icnn_g_loss(f, other, good, good)
    # the marshalling itself refuses a buffer of another shape, whoever calls it
    with pytest.raises(ValueError, match=r"\[B, d\]"):
        icnn._call(0, f, None, torch.zeros(6, 1), None, 0.0, torch.zeros(6, 1))
