"""CPU: the [SF]2M training step's declaration, export, constructor refusals and fixture (no GPU needed)."""
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("net.0.weight", "net.0.bias", "net.2.weight", "net.2.bias", "net.4.weight", "net.4.bias", "net.6.weight", "net.6.bias")


def test_header_declares_the_entry_point_with_its_reference_lines():
    src = open(os.path.join(ROOT, "include", "cfm_gfx950.h")).read()
    assert re.search(r"\bint\s+cfm_mlp_sf2m_step_f32\s*\(", src)
    doc = src[:src.index("int cfm_mlp_sf2m_step_f32")]
    doc = doc[doc.rindex("/*"):]
    assert "SF2M_tutorial.ipynb" in doc and "cfm_module.py:896-909" in doc and "CFM_OP_MLP_TRAIN" in doc


def test_binding_lists_the_entry_point(lib_built):
    res, args = lib_built.SIGNATURES["cfm_mlp_sf2m_step_f32"]
    assert len(args) == 20 and hasattr(lib_built.load(), "cfm_mlp_sf2m_step_f32")


def test_sf2m_step_is_exported():
    import cfm_amd
    assert cfm_amd.SF2MStep is cfm_amd.train.SF2MStep
    for name in ("backward_only", "loss", "__call__"):
        assert callable(getattr(cfm_amd.SF2MStep, name))


def test_constructor_names_what_it_refuses():
    import cfm_amd
    a, b = cfm_amd.MLP(dim=2, w=16, time_varying=True), cfm_amd.MLP(dim=2, w=16, time_varying=True)
    opt = torch.optim.Adam(list(a.parameters()) + list(b.parameters()))
    with pytest.raises(TypeError, match="not on the GPU"):
        cfm_amd.SF2MStep(a, b, opt)
    with pytest.raises(TypeError, match="layer sizes differ"):
        cfm_amd.SF2MStep(a, cfm_amd.MLP(dim=2, w=32, time_varying=True), opt)
    with pytest.raises(TypeError, match="layer sizes differ"):
        cfm_amd.SF2MStep(a, cfm_amd.MLP(dim=3, w=16, time_varying=False), opt)      # same widths, another input
    with pytest.raises(TypeError, match="the score model is a Sequential, not a cfm_amd.MLP"):
        cfm_amd.SF2MStep(a, torch.nn.Sequential(torch.nn.Linear(3, 2)), opt)
    with pytest.raises(TypeError, match="the flow model is a Linear"):
        cfm_amd.SF2MStep(torch.nn.Linear(3, 2), b, opt)
    nb = cfm_amd.MLP(dim=2, w=16, time_varying=True)
    nb.net[6] = torch.nn.Linear(16, 2, bias=False)
    with pytest.raises(TypeError, match="without bias"):
        cfm_amd.SF2MStep(a, nb, opt)
    with pytest.raises(TypeError, match="not fp32"):
        cfm_amd.SF2MStep(a, cfm_amd.MLP(dim=2, w=16, time_varying=True).double(), opt)


@pytest.mark.parametrize("case", ["s1", "s01"])
def test_fixture_is_self_consistent(golden_dir, case):
    """step 0 of the recorded float64 run, recomputed with torch autograd from the stored arrays alone"""
    import cfm_amd
    z = np.load(os.path.join(golden_dir, "sf2m_cases.npz"))
    B, d, w, sigma = z[f"{case}_meta"]
    nets = {}
    for tag in ("flow", "score"):
        nets[tag] = cfm_amd.MLP(dim=int(d), w=int(w), time_varying=True).double()
        nets[tag].load_state_dict({k: torch.from_numpy(z[f"{case}_{tag}_{k}"]).double() for k in NAMES})
    t, xt, ut, eps, lam = (torch.from_numpy(z[f"{case}_b0_{k}"]).double() for k in ("t", "xt", "ut", "eps", "lam"))
    assert t.shape == (int(B),) and xt.shape == (int(B), int(d)) and z[f"{case}_losses"].shape == (5, 2)
    # lambda_t is the matcher's: 2 sigma_t / (sigma^2 + 1e-8), sigma_t = sigma sqrt(t (1 - t)); float32 arithmetic there
    want = 2 * sigma * np.sqrt(z[f"{case}_b0_t"].astype(np.float64) * (1 - z[f"{case}_b0_t"].astype(np.float64))) / (sigma ** 2 + 1e-8)
    assert np.abs(z[f"{case}_b0_lam"] - want).max() <= 1e-5 * want.max()
    if case == "s01":
        assert max(z[f"{case}_b{k}_lam"].max() for k in range(5)) > 9.9
    x = torch.cat([xt, t[:, None]], dim=-1)
    fl = torch.mean((nets["flow"].net(x) - ut) ** 2)
    sl = torch.mean((lam[:, None] * nets["score"].net(x) + eps) ** 2)
    (fl + sl).backward()
    fl, sl = float(fl.detach()), float(sl.detach())
    assert abs(fl - z[f"{case}_losses"][0, 0]) <= 1e-12 * abs(fl)
    assert abs(sl - z[f"{case}_losses"][0, 1]) <= 1e-12 * abs(sl)
    for tag in ("flow", "score"):
        for k, p in nets[tag].named_parameters():
            g = torch.from_numpy(z[f"{case}_grad0_{tag}_{k}"])
            assert g.dtype == torch.float64 and (g - p.grad).abs().max() <= 1e-12 * g.abs().max(), (tag, k)
