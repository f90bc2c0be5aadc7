"""Regenerates tests/golden/sf2m_cases.npz: the [SF]2M training loop of the reference (examples/2D_tutorials/
SF2M_tutorial.ipynb cell 3) on its own classes, in float64.

    python tests/golden/make_sf2m_golden.py

Needs the unmodified reference tree (oracle/ref_import.py): SchrodingerBridgeConditionalFlowMatcher comes from its
torchcfm/conditional_flow_matching.py, MLP from its torchcfm/models/models.py, loaded by path.  Per case
(B, d, w, sigma), seeded:
  * both nets' initial fp32 state dicts (flow_*, score_*);
  * for each of 5 steps t, xt, ut, eps, lambda_t (fp32): t and eps are drawn here, xt, ut and lambda_t come from the
    matcher's own sample_xt, compute_conditional_flow and compute_lambda on them (no coupling: x0, x1 are paired as
    drawn — the coupling is not what this fixture is about);
  * the float64 losses and float64 parameter gradients of step 0 (fp32 inputs and weights, upcast);
  * the float64 five-step sequences of flow_loss and score_loss under torch.optim.Adam(lr=1e-3) over both nets.
The reference's loop is also run in float32 and must stay within 1e-5 (relative) of the float64 sequences: the recorded
batches are therefore well conditioned enough that a float32 implementation can be held to the tests' bounds.
"""
import copy
import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "oracle")):
    if p not in sys.path:
        sys.path.insert(0, p)

import ref_import  # noqa: E402

CASES = {"s1": (256, 2, 64, 1.0, 11), "s01": (256, 2, 64, 0.1, 12)}      # name: (B, d, w, sigma, seed)
STEPS = 5


def reference_mlp():
    spec = importlib.util.spec_from_file_location(
        "torchcfm_ref_models", os.path.join(ref_import.REFERENCE_ROOT, "torchcfm", "models", "models.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m.MLP


def losses(model, score_model, t, xt, ut, eps, lam):
    """the tutorial's lines, verbatim"""
    vt = model(torch.cat([xt, t[:, None]], dim=-1))
    st = score_model(torch.cat([xt, t[:, None]], dim=-1))
    flow_loss = torch.mean((vt - ut) ** 2)
    score_loss = torch.mean((lam[:, None] * st + eps) ** 2)
    return flow_loss, score_loss


def loop(model, score_model, batches, dtype):
    model, score_model = copy.deepcopy(model).to(dtype), copy.deepcopy(score_model).to(dtype)
    opt = torch.optim.Adam(list(model.parameters()) + list(score_model.parameters()), lr=1e-3)
    seq, grads0 = [], None
    for k, b in enumerate(batches):
        opt.zero_grad()
        fl, sl = losses(model, score_model, *[x.to(dtype) for x in b])
        (fl + sl).backward()
        if k == 0:
            grads0 = [p.grad.detach().clone() for p in list(model.parameters()) + list(score_model.parameters())]
        opt.step()
        seq.append((float(fl.detach()), float(sl.detach())))
    return np.asarray(seq, dtype=np.float64), grads0


def make_case(name, B, d, w, sigma, seed, out):
    cfm, _ = ref_import.import_reference()
    MLP = reference_mlp()
    FM = cfm.SchrodingerBridgeConditionalFlowMatcher(sigma=sigma)
    torch.manual_seed(seed)
    model, score_model = MLP(dim=d, w=w, time_varying=True), MLP(dim=d, w=w, time_varying=True)
    batches = []
    for k in range(STEPS):
        x0 = torch.randn(B, d)
        x1 = torch.randn(B, d) * 0.5 + torch.tensor([2.0, -1.0])[:d]
        t = torch.rand(B)
        eps = torch.randn(B, d)
        xt = FM.sample_xt(x0, x1, t, eps)
        ut = FM.compute_conditional_flow(x0, x1, t, xt)
        lam = FM.compute_lambda(t)
        batches.append((t, xt, ut, eps, lam))
    seq64, g64 = loop(model, score_model, batches, torch.float64)
    seq32, _ = loop(model, score_model, batches, torch.float32)
    dev = float(np.max(np.abs(seq32 - seq64) / np.abs(seq64)))
    print(f"{name}: B={B} d={d} w={w} sigma={sigma}: max lambda {float(max(b[4].max() for b in batches)):.3f}, "
          f"reference fp32 loop vs float64: {dev:.2e}")
    assert dev <= 1e-5, dev
    for tag, net in (("flow", model), ("score", score_model)):
        for k, v in net.state_dict().items():
            out[f"{name}_{tag}_{k}"] = v.detach().numpy().astype(np.float32)
    for k, b in enumerate(batches):
        for nm, v in zip(("t", "xt", "ut", "eps", "lam"), b):
            out[f"{name}_b{k}_{nm}"] = v.numpy().astype(np.float32)
    names = [f"flow_{k}" for k, _ in model.named_parameters()] + [f"score_{k}" for k, _ in score_model.named_parameters()]
    for nm, g in zip(names, g64):
        out[f"{name}_grad0_{nm}"] = g.numpy().astype(np.float64)
    out[f"{name}_losses"] = seq64                                   # [STEPS, 2]: flow, score
    out[f"{name}_meta"] = np.asarray([B, d, w, sigma], dtype=np.float64)


def main():
    out = {}
    for name, (B, d, w, sigma, seed) in CASES.items():
        make_case(name, B, d, w, sigma, seed, out)
    path = os.path.join(HERE, "sf2m_cases.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {os.path.getsize(path) / 1024:.0f} kB")


if __name__ == "__main__":
    main()
