"""Outputs of every small-field entry point (csrc/ode.hip, sde_small.h and the gradient entries of csrc/small_grad.hip) on
fixed seeds, in one .npz:

    python tools/ode_unit_dump.py OUT.npz            (CFM_LIB_PATH selects the build of the library)
    python tools/ode_unit_dump.py --compare A.npz B.npz

A refactor of that unit moves no floating-point operation, so two builds must agree bit for bit: run the dump once per
build, each in a fresh process, then --compare (numpy.array_equal array by array, n_steps / nfe included; exit 1 on any
difference).  Shapes: B = 1 and 17 (two tiles, the second with one row); d = 2 and 63 (ODE / CNF: d + 1 = 64 is the
envelope's edge) or 64 (SDE); hidden width 64 and 33 (padded columns); n_t = 4 both ways; B = 9000 at d = 2 for the
adaptive solves (the only shape on the non-resident ode_small_dopri).  The gradient entries besides
cfm_cnf_euler_grad_f32 (GRAD_SHAPES): B = 4112 is 257 tiles, so workgroup 0 of the 256 runs a second tile; n_t small.
Measurement infrastructure."""
import ctypes
import itertools
import os
import struct
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = {}


def net(d, w, seed):
    import torch, cfm_amd
    torch.manual_seed(seed)
    return cfm_amd.MLP(dim=d, time_varying=True, w=w).hip_params()


def randn(seed, *shape):
    import torch
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)).cuda()


def ode_cases(lib, L, ptr, sp):
    import torch
    ts_up = np.array([0.0, 0.3, 0.55, 1.0], np.float32)
    shapes = [(B, d) for B in (1, 17) for d in (2, 63)] + [(9000, 2)]
    for (B, d), w, up, solver, est in itertools.product(shapes, (64, 33), (1, 0), ("euler", "midpoint", "rk4", "dopri5", "tsit5"),
                                                        ("plain", "exact", "hutch")):
        if B == 9000 and solver in L.ODE_SCHEME:
            continue
        Wp, bp, dims, keep = net(d, w, 1)
        ts = ts_up if up else np.ascontiguousarray(ts_up[::-1])
        tsp, D = ts.ctypes.data_as(ctypes.c_void_p), d + (est != "plain")
        x = randn(2, B, D)
        eps = torch.sign(randn(3, B, d)) if est == "hutch" else None
        traj = torch.zeros((4, B, D), device="cuda")
        ws = L.workspace(L.OP_ODE, B, w, D)
        nfe, steps = ctypes.c_int(0), ctypes.c_int(0)
        cnf = () if est == "plain" else (int(est == "hutch"), ptr(eps))
        if solver in L.ODE_SCHEME:
            f = lib.cfm_ode_fixed_mlp_f32 if est == "plain" else lib.cfm_ode_fixed_cnf_mlp_f32
            rc = f(Wp, bp, dims, 4, ptr(x), B, tsp, 4, *cnf, L.ODE_SCHEME[solver], ptr(traj), ctypes.byref(nfe), ptr(ws), sp())
        else:
            f = lib.cfm_ode_adaptive_mlp_f32 if est == "plain" else lib.cfm_ode_adaptive_cnf_mlp_f32
            rc = f(Wp, bp, dims, 4, ptr(x), B, tsp, 4, *cnf, L.ODE_TABLEAU[solver], 1e-4, 1e-4, ptr(traj), ctypes.byref(steps),
                   ctypes.byref(nfe), ptr(ws), sp())
        # the one refusal there is: an adaptive CNF solve of fewer elements (B D = 3) than grid points answers CFM_EINVAL
        if not (rc == -1 and B * D < 4 and est != "plain" and solver in L.ODE_TABLEAU):
            L.check(rc, f"{solver} {est}")
        key = f"ode B{B} d{d} w{w} {'up' if up else 'down'} {solver} {est}"
        OUT[key], OUT[key + " counts"] = traj.cpu().numpy(), np.array([rc, steps.value, nfe.value])


def div_grad_cases(lib, L, ptr, sp):
    import torch
    for (B, d), w, mode in itertools.product([(1, 2), (17, 2), (17, 5), (17, 63)], (64, 33), (0, 1)):
        Wp, bp, dims, keep = net(d, w, 4)
        x, eps = randn(5, B, d), torch.sign(randn(6, B, d))
        v, div = torch.zeros((B, d), device="cuda"), torch.zeros(B, device="cuda")
        L.check(lib.cfm_mlp_divergence_f32(Wp, bp, dims, 4, ptr(x), B, 0.37, mode, ptr(eps), ptr(v), ptr(div), None, sp()), "div")
        OUT[f"div B{B} d{d} w{w} mode{mode} v"], OUT[f"div B{B} d{d} w{w} mode{mode} div"] = v.cpu().numpy(), div.cpu().numpy()
        if B != 17 or d > 5:
            continue
        ts = np.array([1.0, 0.6, 0.25, 0.0], np.float32)
        tsp, nfe = ts.ctypes.data_as(ctypes.c_void_p), ctypes.c_int(0)
        traj, g0 = torch.zeros((4, B, d + 1), device="cuda"), torch.zeros((B, d + 1), device="cuda")
        L.check(lib.cfm_ode_fixed_cnf_mlp_f32(Wp, bp, dims, 4, ptr(randn(7, B, d + 1)), B, tsp, 4, mode, ptr(eps), 0, ptr(traj),
                                              ctypes.byref(nfe), ptr(L.workspace(L.OP_ODE, B, w, d + 1)), sp()), "euler cnf")
        dW, db = [torch.zeros_like(t) for t in keep[0]], [torch.zeros_like(t) for t in keep[1]]
        dWp, dbp = ((ctypes.c_void_p * 4)(*[t.data_ptr() for t in g]) for g in (dW, db))
        L.check(lib.cfm_cnf_euler_grad_f32(Wp, bp, dims, 4, ptr(traj), B, tsp, 4, mode, ptr(eps), ptr(randn(8, B, d + 1)), dWp, dbp,
                                           ptr(g0), ptr(L.workspace(L.OP_CNF_GRAD, B, 4, 0)), sp()), "grad")
        for i, t in enumerate(dW + db + [g0]):
            OUT[f"grad d{d} w{w} mode{mode} {i}"] = t.cpu().numpy()


def sde_cases(lib, L, ptr, sp):
    import torch
    hs, outs = (0.25, 0.25, 0.3, 0.2), (1, 0, 1, 1)
    for B, d, w, srk, score, philox, rev in itertools.product((1, 17), (2, 64), (64, 33), (0, 1), (1, 0), (0, 1), (0, 1)):
        (Wf, bf, dims, k1), (Ws, bs, _, k2) = net(d, w, 9), net(d, w, 10)
        t, recs = 0.0, []
        for h, o in zip(hs, outs):
            te = [1.0 - u if rev else u for u in (t, t + h, t + 0.5 * h)]
            gs = 0.3 * abs(h) ** 0.5
            recs.append(struct.pack("<ffffffii", *te, h, gs, 0.75 * gs, o, 0) if srk else struct.pack("<fffi", te[0], h, gs, o))
            t += h
        host = ctypes.create_string_buffer(b"".join(recs))
        xi = None if philox else randn(11, 4, 2, B, d) if srk else randn(11, 4, B, d)
        out, ws = torch.zeros((3, B, d), device="cuda"), torch.zeros(4 * 32 + 256, dtype=torch.uint8, device="cuda")
        f = lib.cfm_sde_srk_mlp_f32 if srk else lib.cfm_sde_em_mlp_f32
        L.check(f(Wf, bf, Ws if score else None, bs if score else None, dims, 4, ptr(randn(12, B, d)), B, host, 4, rev, ptr(xi), 1234,
                  ptr(out), ptr(ws), sp()), "sde")
        torch.cuda.synchronize()
        OUT[f"sde B{B} d{d} w{w} {'srk' if srk else 'em'} score{score} philox{philox} rev{rev}"] = out.cpu().numpy()


GRAD_SHAPES = [(1, 2, 64), (17, 2, 33), (17, 63, 64), (4112, 2, 64)]         # (B, d, hidden width)
SPANS = {1: [0.0], 2: [0.0, 1.0], 4: [0.0, 0.3, 0.55, 1.0], 5: [0.0, 0.2, 0.45, 0.7, 1.0]}


def span(n_t, up):
    ts = np.array(SPANS[n_t], np.float32)
    ts = ts if up else np.ascontiguousarray(ts[::-1])
    return ts, ts.ctypes.data_as(ctypes.c_void_p)


def grads_of(keep):
    """zeroed dW, db like the net's tensors and their pointer tables"""
    import torch
    dW, db = [torch.zeros_like(t) for t in keep[0]], [torch.zeros_like(t) for t in keep[1]]
    return dW, db, *((ctypes.c_void_p * 4)(*[t.data_ptr() for t in g]) for g in (dW, db))


def put(key, tensors):
    for i, t in enumerate(tensors):
        OUT[f"{key} {i}"] = t.cpu().numpy()


def fixed_grad_cases(lib, L, ptr, sp):
    import torch
    for (B, d, w), solver, n_t, up, with_g0 in itertools.product(GRAD_SHAPES, ("euler", "midpoint", "rk4"), (1, 2, 4), (1, 0), (1, 0)):
        Wp, bp, dims, keep = net(d, w, 13)
        ts, tsp = span(n_t, up)
        x, nfe = randn(14, B, d), ctypes.c_int(0)
        traj = torch.zeros((n_t, B, d), device="cuda")
        traj[0] = x
        if n_t > 1:
            L.check(lib.cfm_ode_fixed_mlp_f32(Wp, bp, dims, 4, ptr(x), B, tsp, n_t, L.ODE_SCHEME[solver], ptr(traj), ctypes.byref(nfe),
                                              ptr(L.workspace(L.OP_ODE, B, w, d)), sp()), "fixed solve")
        dW, db, dWp, dbp = grads_of(keep)
        g0 = torch.zeros((B, d), device="cuda") if with_g0 else None
        L.check(lib.cfm_ode_fixed_grad_f32(Wp, bp, dims, 4, ptr(traj), B, tsp, n_t, L.ODE_SCHEME[solver], ptr(randn(15, n_t, B, d)), dWp,
                                           dbp, ptr(g0), ptr(L.workspace(L.OP_ODE_GRAD, B, n_t, 0)), sp()), "fixed grad")
        put(f"fixedgrad B{B} d{d} w{w} {solver} nt{n_t} {'up' if up else 'down'} g0{with_g0}", dW + db + ([g0] if with_g0 else []))


def adaptive_grad_cases(lib, L, ptr, sp):
    import torch
    max_steps = 64
    for (B, d, w), solver, n_t, up in itertools.product(GRAD_SHAPES, ("dopri5", "tsit5"), (2, 5), (1, 0)):
        Wp, bp, dims, keep = net(d, w, 16)
        ts, tsp = span(n_t, up)
        x = randn(17, B, d)
        traj = torch.zeros((n_t, B, d), device="cuda")
        log, ysteps = torch.zeros((max_steps, 4), device="cuda"), torch.zeros((max_steps, B, d), device="cuda")
        steps, nfe, n_acc = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0)
        rc = lib.cfm_ode_adaptive_rec_mlp_f32(Wp, bp, dims, 4, ptr(x), B, tsp, n_t, L.ODE_TABLEAU[solver], 1e-5, 1e-5, ptr(traj),
                                              ctypes.byref(steps), ctypes.byref(nfe), max_steps, ptr(log), ptr(ysteps),
                                              ctypes.byref(n_acc), ptr(L.workspace(L.OP_ODE, B, w, d)), sp())
        torch.cuda.synchronize()
        key = f"adaptivegrad B{B} d{d} w{w} {solver} nt{n_t} {'up' if up else 'down'}"
        n = n_acc.value
        OUT[key + " counts"] = np.array([rc, steps.value, nfe.value, n])
        OUT[key + " traj"], OUT[key + " ysteps"] = traj.cpu().numpy(), ysteps[:n].cpu().numpy()
        OUT[key + " log"] = log[:n].cpu().numpy().view(np.int32)          # bit patterns: out = -1 is a NaN as a float
        if rc != 0:            # a solve the recording entry declines (fewer elements than grid points) has no gradient
            continue
        for with_g0 in (1, 0):
            dW, db, dWp, dbp = grads_of(keep)
            g0 = torch.zeros((B, d), device="cuda") if with_g0 else None
            L.check(lib.cfm_ode_adaptive_grad_f32(Wp, bp, dims, 4, ptr(ysteps), ptr(log), n, B, n_t, L.ODE_TABLEAU[solver],
                                                  1.0 if up else -1.0, ptr(randn(18, n_t, B, d)), dWp, dbp, ptr(g0),
                                                  ptr(L.workspace(L.OP_ODE_GRAD, B, n_t, 0)), sp()), "adaptive grad")
            put(f"{key} g0{with_g0}", dW + db + ([g0] if with_g0 else []))


def cnf_reg_grad_cases(lib, L, ptr, sp):
    import torch
    B, n_t = 17, 4
    ts, tsp = span(n_t, 0)
    for d, w, (mode, mask) in itertools.product((2, 5), (64, 33), ((0, 1), (0, 2), (0, 3), (1, 1))):
        Wp, bp, dims, keep = net(d, w, 19)
        D = d + 1 + (mask & 1) + (mask >> 1)
        eps, nfe = torch.sign(randn(20, B, d)), ctypes.c_int(0)
        traj, jsq, g0 = torch.zeros((n_t, B, D), device="cuda"), torch.zeros((n_t - 1, B), device="cuda"), torch.zeros((B, D), device="cuda")
        L.check(lib.cfm_ode_euler_cnf_reg_mlp_f32(Wp, bp, dims, 4, ptr(randn(21, B, D)), B, tsp, n_t, mode, ptr(eps), mask, ptr(traj),
                                                  ptr(jsq), ctypes.byref(nfe), ptr(L.workspace(L.OP_ODE, B, w, D)), sp()), "reg solve")
        dW, db, dWp, dbp = grads_of(keep)
        L.check(lib.cfm_cnf_reg_euler_grad_f32(Wp, bp, dims, 4, ptr(traj), B, tsp, n_t, mode, ptr(eps), mask, ptr(jsq),
                                               ptr(randn(22, B, D)), dWp, dbp, ptr(g0), ptr(L.workspace(L.OP_CNF_GRAD, B, n_t, 0)), sp()),
                "reg grad")
        put(f"reggrad d{d} w{w} mode{mode} mask{mask}", dW + db + [g0, traj, jsq])


def action_grad_cases(lib, L, ptr, sp):
    import torch, cfm_amd
    for B, d, w, with_xt in itertools.product((1, 17, 4112), (2, 63), (64, 33), (1, 0)):
        torch.manual_seed(23)
        Wp, bp, dims, keep = cfm_amd.MLP(dim=d, out_dim=1, time_varying=True, w=w).hip_params()
        x0, x1, t = randn(24, B, d), randn(25, B, d), torch.rand(B, generator=torch.Generator().manual_seed(26)).cuda()
        xt = randn(27, B, d) if with_xt else None
        loss = torch.zeros(1, device="cuda")
        dW, db, dWp, dbp = grads_of(keep)
        L.check(lib.cfm_action_matching_grad_f32(Wp, bp, dims, 4, ptr(x0), ptr(x1), ptr(xt), ptr(t), B, ptr(loss), dWp, dbp,
                                                 ptr(L.workspace(L.OP_ACTION_GRAD, B, 0, 0)), sp()), "action grad")
        put(f"actiongrad B{B} d{d} w{w} xt{with_xt}", dW + db + [loss])


def compare(a, b):
    A, B = np.load(a), np.load(b)
    bad = [k for k in sorted(set(A.files) | set(B.files)) if k not in A.files or k not in B.files or not np.array_equal(A[k], B[k])]
    for kind in ("ode ", "div ", "grad ", "sde ", "fixedgrad ", "adaptivegrad ", "reggrad ", "actiongrad "):
        ks = [k for k in A.files if k.startswith(kind)]
        print(f"{kind.strip()}: {len(ks)} arrays, {sum(k in bad for k in ks)} differ")
    print("differing:", bad if bad else "none")
    return 1 if bad or set(A.files) != set(B.files) else 0


if __name__ == "__main__":
    if sys.argv[1] == "--compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    import cfm_amd._lib as L
    lib = L.load()
    for cases in (ode_cases, div_grad_cases, sde_cases, fixed_grad_cases, adaptive_grad_cases, cnf_reg_grad_cases, action_grad_cases):
        cases(lib, L, L.ptr, L.stream_ptr)
    np.savez(sys.argv[1], **OUT)
    print(f"{len(OUT)} arrays from {L.LIB_PATH} -> {sys.argv[1]}")
