"""Outputs of every small-field entry point (csrc/ode.hip, sde_small.h and the gradient entries of csrc/small_grad.hip) on
fixed seeds, in one .npz:

    python tools/ode_unit_dump.py OUT.npz            (CFM_LIB_PATH selects the build of the library)
    python tools/ode_unit_dump.py --compare A.npz B.npz [A2.npz]

A refactor of that unit moves no floating-point operation, so two builds must agree bit for bit: run the dump once per
build, each in a fresh process, then --compare (numpy.array_equal array by array, rc / n_steps / nfe / n_accepted
included; exit 1 on any difference).  A2, a second dump of A's build, tells which arrays that build does not reproduce
itself (the layer path's fp64 norms are atomic sums of one term per 256 elements: order-free above B d = 256); those are
counted apart and held against B at the spread A and A2 show.
Shapes: B = 1 and 17 (two tiles, the second with one row); d = 2 and 63 (ODE / CNF: d + 1 = 64 is the
envelope's edge) or 64 (SDE); hidden width 64 and 33 (padded columns); n_t = 4 both ways; B = 9000 at d = 2 for the
adaptive solves (the only shape on the non-resident ode_small_dopri).  The gradient entries besides
cfm_cnf_euler_grad_f32 (GRAD_SHAPES): B = 4112 is 257 tiles, so workgroup 0 of the 256 runs a second tile; n_t small.
The host drivers of csrc/ode.hip, entry by entry (EXTRA names them):
  layer    the layer-per-kernel path of the fixed, adaptive and pair entries, every scheme and tableau: by
           cfm_ode_set_fused(0) at the shapes above and by a field outside the envelope (hidden width 65, d = 64), on the
           register-staged layer core (cfm_mlp_set_glds(0)) and on the default engine
  host     the pair entry on its one-launch path, cfm_mlp_grad_field_f32 with and without the Laplacian, the three
           gradient-field solves, the four old alias entries
  edge     n_t = 1 and 2 and the two grids that are not strictly monotone, every entry (B d < n_t: B = 1, d = 2 above)
  refuse   what every entry declines: unknown selector, n_t below its minimum, B = 0, mode 1 without eps, unknown modes
           and masks, the fused path switched off, the recording entry outside the envelope
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


# ---- the host drivers of csrc/ode.hip: every forward entry by a short name -------------------------------------------
# extra state columns of x0 / traj (the regularised solve at mode 0, reg_mask 1: l and the kinetic energy)
EXTRA = {"fixed": 0, "euler": 0, "pair": 0, "fixed_cnf": 1, "euler_cnf": 1, "fixed_gradmlp": 0, "fixed_cnf_gradmlp": 1, "reg": 2,
         "adaptive": 0, "dopri5": 0, "rec": 0, "adaptive_cnf": 1, "dopri5_cnf": 1, "adaptive_gradmlp": 0}
FIXED_ENTRIES = ("fixed", "pair", "fixed_cnf", "fixed_gradmlp", "fixed_cnf_gradmlp", "reg")
ADAPTIVE_ENTRIES = ("adaptive", "rec", "adaptive_cnf", "adaptive_gradmlp")
SELECTORS = {**{e: (0, 1, 2) for e in FIXED_ENTRIES}, **{e: (0, 1) for e in ADAPTIVE_ENTRIES}, "reg": (0,)}
MAX_STEPS = 64


def nets_of(d, w, seed):
    """field net, second (backward drift) net and action net of one shape: pointer tables and what keeps them alive"""
    import torch, cfm_amd
    f, b = net(d, w, seed), net(d, w, seed + 100)
    torch.manual_seed(seed + 200)
    a = cfm_amd.MLP(dim=d, out_dim=1, time_varying=True, w=w).hip_params()
    return {"f": f, "b": b, "a": a}


def call(lib, L, name, nets, B, d, w, ts, sel, key, mode=0, eps=None, mask=1, n_t=None, B_arg=None, jsq=False):
    """One call of a forward entry on seeded inputs; records traj and (rc, n_steps, nfe, n_accepted) under `key`.  n_t / B_arg
    override what the entry is told (refusals: every buffer still has the true size)."""
    import torch
    ptr, sp = L.ptr, L.stream_ptr
    D = d + EXTRA[name]
    x, traj = randn(30, B, D), torch.zeros((len(ts), B, D), device="cuda")
    ws = L.workspace(L.OP_ODE, B, w, D)
    steps, nfe, nacc = ctypes.c_int(-7), ctypes.c_int(-7), ctypes.c_int(-7)
    Wp, bp, dims, _ = nets["a" if "gradmlp" in name else "f"]
    head = (Wp, bp, dims, 4, ptr(x), B if B_arg is None else B_arg, ts.ctypes.data_as(ctypes.c_void_p), len(ts) if n_t is None else n_t)
    ftail = (ptr(traj), ctypes.byref(nfe), ptr(ws), sp())
    atail = (1e-4, 1e-4, ptr(traj), ctypes.byref(steps), ctypes.byref(nfe))
    if name == "fixed":
        rc = lib.cfm_ode_fixed_mlp_f32(*head, sel, *ftail)
    elif name == "euler":
        rc = lib.cfm_ode_euler_mlp_f32(*head, *ftail)
    elif name == "pair":
        Wq, bq = nets["b"][:2]
        rc = lib.cfm_ode_fixed_pair_mlp_f32(Wp, bp, Wq, bq, *head[2:], sel, *ftail)
    elif name == "fixed_cnf":
        rc = lib.cfm_ode_fixed_cnf_mlp_f32(*head, mode, ptr(eps), sel, *ftail)
    elif name == "euler_cnf":
        rc = lib.cfm_ode_euler_cnf_mlp_f32(*head, mode, ptr(eps), *ftail)
    elif name == "fixed_gradmlp":
        rc = lib.cfm_ode_fixed_gradmlp_f32(*head, sel, *ftail)
    elif name == "fixed_cnf_gradmlp":
        rc = lib.cfm_ode_fixed_cnf_gradmlp_f32(*head, mode, ptr(eps), sel, *ftail)
    elif name == "reg":
        side = torch.zeros((len(ts), B), device="cuda") if jsq else None
        rc = lib.cfm_ode_euler_cnf_reg_mlp_f32(*head, mode, ptr(eps), mask, ptr(traj), ptr(side), ctypes.byref(nfe), ptr(ws), sp())
    elif name == "adaptive":
        rc = lib.cfm_ode_adaptive_mlp_f32(*head, sel, *atail, ptr(ws), sp())
    elif name == "dopri5":
        rc = lib.cfm_ode_dopri5_mlp_f32(*head, *atail, ptr(ws), sp())
    elif name == "rec":
        log, ysteps = torch.zeros((MAX_STEPS, 4), device="cuda"), torch.zeros((MAX_STEPS, B, d), device="cuda")
        rc = lib.cfm_ode_adaptive_rec_mlp_f32(*head, sel, *atail, MAX_STEPS, ptr(log), ptr(ysteps), ctypes.byref(nacc), ptr(ws), sp())
    elif name == "adaptive_cnf":
        rc = lib.cfm_ode_adaptive_cnf_mlp_f32(*head, mode, ptr(eps), sel, *atail, ptr(ws), sp())
    elif name == "dopri5_cnf":
        rc = lib.cfm_ode_dopri5_cnf_mlp_f32(*head, mode, ptr(eps), *atail, ptr(ws), sp())
    else:
        rc = lib.cfm_ode_adaptive_gradmlp_f32(*head, sel, *atail, ptr(ws), sp())
    torch.cuda.synchronize()
    assert rc in (0, -1), (key, rc)          # a solve or CFM_EINVAL; anything else is a failure of the run itself
    OUT[key], OUT[key + " counts"] = traj.cpu().numpy(), np.array([rc, steps.value, nfe.value, nacc.value])


def layer_cases(lib, L, ptr, sp):
    """The layer-per-kernel drivers (fixed, adaptive, pair): reached by cfm_ode_set_fused(0) at the shapes of ode_cases and,
    with the switch on, by a field outside the envelope (hidden width 65, d = 64); on the register-staged layer core
    (cfm_mlp_set_glds(0)) and on the default engine.  The fp64 norms of the adaptive driver are atomic sums of one term per
    256 elements: run-dependent above B d = 256."""
    shapes = [(B, d, w, 0) for B in (1, 17) for d in (2, 63) for w in (64, 33)] + [(1, 64, 65, 1), (17, 64, 65, 1)]
    glds0 = lib.cfm_mlp_get_glds()
    try:
        for (B, d, w, fused), glds, up in itertools.product(shapes, (0, glds0), (1, 0)):
            lib.cfm_ode_set_fused(fused); lib.cfm_mlp_set_glds(glds)
            nets, (ts, _) = nets_of(d, w, 40), span(4, up)
            for name in ("fixed", "adaptive", "pair"):
                for sel in SELECTORS[name]:
                    call(lib, L, name, nets, B, d, w, ts, sel, f"layer {name}{sel} B{B} d{d} w{w} fused{fused} "
                         f"glds{'0' if glds == 0 else 'default'} {'up' if up else 'down'}")
    finally:
        lib.cfm_ode_set_fused(1); lib.cfm_mlp_set_glds(glds0)


def pair_and_gradmlp_cases(lib, L, ptr, sp):
    """The pair entry on its one-launch path, the three gradient-field solves and the four old alias entries."""
    for B, d, w, up in itertools.product((1, 17), (2, 63), (64, 33), (1, 0)):
        nets, (ts, _) = nets_of(d, w, 41), span(4, up)
        for name in ("pair", "fixed_gradmlp", "fixed_cnf_gradmlp", "adaptive_gradmlp"):
            for sel in SELECTORS[name]:
                call(lib, L, name, nets, B, d, w, ts, sel, f"host {name}{sel} B{B} d{d} w{w} {'up' if up else 'down'}")
        if w == 64:
            for name in ("euler", "dopri5", "euler_cnf", "dopri5_cnf"):
                call(lib, L, name, nets, B, d, w, ts, 0, f"host alias {name} B{B} d{d} {'up' if up else 'down'}")


def grad_field_cases(lib, L, ptr, sp):
    import torch
    for (B, d), w, with_lap in itertools.product([(1, 2), (17, 2), (17, 63)], (64, 33), (1, 0)):
        Wa, ba, adims, keep = nets_of(d, w, 42)["a"]
        v, lap = torch.zeros((B, d), device="cuda"), torch.zeros(B, device="cuda")
        L.check(lib.cfm_mlp_grad_field_f32(Wa, ba, adims, 4, ptr(randn(43, B, d)), d, B, 0.37, ptr(v), ptr(lap) if with_lap else None,
                                           None, sp()), "grad field")
        torch.cuda.synchronize()
        OUT[f"host gradfield B{B} d{d} w{w} lap{with_lap} v"], OUT[f"host gradfield B{B} d{d} w{w} lap{with_lap} lap"] = v.cpu().numpy(), lap.cpu().numpy()


NON_MONOTONE = {"back": [0.0, 0.5, 0.25, 1.0], "repeat": [0.0, 0.5, 0.5, 1.0]}


def edge_cases(lib, L, ptr, sp):
    """n_t = 1 and 2, grids that are not strictly monotone (B d < n_t is ode_cases' B = 1, d = 2), and the refusals of every
    entry.  A refusal passes only what the entry checks before it touches memory: every pointer is a live buffer of the true
    size, and the argument under test is an integer, or a NULL that the entry tests for (eps at mode 1, jac_sq at reg_mask 2)."""
    import torch
    d, w = 2, 64
    everything = FIXED_ENTRIES + ADAPTIVE_ENTRIES
    for B in (1, 17):
        nets = nets_of(d, w, 44)
        for name in everything:
            for sel in SELECTORS[name]:
                for n_t in (1, 2):               # (n_t = 1: a solve without a step, fixed; a refusal, adaptive)
                    call(lib, L, name, nets, B, d, w, span(n_t, 1)[0], sel, f"edge {name}{sel} B{B} nt{n_t}")
                for gname, g in NON_MONOTONE.items():
                    call(lib, L, name, nets, B, d, w, np.array(g, np.float32), sel, f"edge {name}{sel} B{B} grid {gname}")
        ts = span(4, 1)[0]
        for name in everything:
            bad = 3 if name in FIXED_ENTRIES else 2
            if name != "reg":
                for sel in (-1, bad):
                    call(lib, L, name, nets, B, d, w, ts, sel, f"refuse {name} B{B} selector{sel}")
            call(lib, L, name, nets, B, d, w, ts, 0, f"refuse {name} B{B} nt0", n_t=0)
            call(lib, L, name, nets, B, d, w, ts, 0, f"refuse {name} B{B} Bzero", B_arg=0)
            if EXTRA[name] and name != "reg":
                for mode in (1, 2, -1):          # mode 1 without eps; unknown modes
                    call(lib, L, name, nets, B, d, w, ts, 0, f"refuse {name} B{B} mode{mode} noeps", mode=mode)
        for mode, mask, jsq in ((1, 1, 0), (3, 1, 0), (0, 0, 0), (0, 16, 0), (0, 2, 0), (1, 2, 1)):
            eps = torch.sign(randn(45, B, d)) if (mode, mask) == (1, 2) else None      # (the Jacobian penalty wants mode 0)
            call(lib, L, "reg", nets, B, d, w, ts, 0, f"refuse reg B{B} mode{mode} mask{mask} jsq{jsq}", mode=mode, mask=mask, eps=eps, jsq=jsq)
        v, div = torch.zeros((B, d), device="cuda"), torch.zeros(B, device="cuda")
        Wp, bp, dims, _ = nets["f"]
        for mode, Ba in ((1, B), (2, B), (0, 0)):
            rc = lib.cfm_mlp_divergence_f32(Wp, bp, dims, 4, ptr(randn(46, B, d)), Ba, 0.37, mode, None, ptr(v), ptr(div), None, sp())
            OUT[f"refuse divergence B{B} mode{mode} Barg{Ba} counts"] = np.array([rc])
        Wa, ba, adims, _ = nets["a"]
        for Ba, ldx in ((0, d), (B, d - 1)):
            rc = lib.cfm_mlp_grad_field_f32(Wa, ba, adims, 4, ptr(randn(46, B, d)), ldx, Ba, 0.37, ptr(v), None, None, sp())
            OUT[f"refuse gradfield B{B} Barg{Ba} ldx{ldx} counts"] = np.array([rc])
        torch.cuda.synchronize()
        OUT[f"refuse evals B{B} v"], OUT[f"refuse evals B{B} div"] = v.cpu().numpy(), div.cpu().numpy()
        # off the one-launch path the recording entry declines (and every one-launch-only entry with it)
        lib.cfm_ode_set_fused(0)
        try:
            for name in everything:
                if name not in ("fixed", "pair", "adaptive"):
                    call(lib, L, name, nets, B, d, w, span(2, 1)[0], 0, f"refuse {name} B{B} fused0")
        finally:
            lib.cfm_ode_set_fused(1)
        call(lib, L, "rec", nets_of(64, 65, 44), B, 64, 65, span(2, 1)[0], 0, f"refuse rec B{B} w65")


KINDS = ("ode ", "div ", "grad ", "sde ", "fixedgrad ", "adaptivegrad ", "reggrad ", "actiongrad ", "layer ", "host ", "edge ", "refuse ")


def compare(a, b, a2=None):
    """A (parent) against B (head); with A2, a second run of the parent's build, the arrays that differ between A and A2 are
    run-dependent: counted apart, and held against B at the spread the two parent runs show (max |A - A2|)."""
    A, B = np.load(a), np.load(b)
    A2 = np.load(a2) if a2 else A
    differ = lambda X, Y, k: k not in X.files or k not in Y.files or not np.array_equal(X[k], Y[k])       # noqa: E731
    keys = sorted(set(A.files) | set(B.files) | set(A2.files))
    loose = [k for k in keys if differ(A, A2, k)]
    bad = [k for k in keys if k not in loose and differ(A, B, k)]
    far = []
    for k in loose:
        if k in A.files and k in A2.files and k in B.files and A[k].shape == A2[k].shape == B[k].shape:
            spread, dist = np.abs(A[k].astype(np.float64) - A2[k]).max(), np.abs(A[k].astype(np.float64) - B[k]).max()
            print(f"run-dependent: {k}: parent runs differ by {spread:.3g}, head from parent by {dist:.3g}")
            if dist <= spread:
                continue
        far.append(k)
    for kind in KINDS:
        ks = [k for k in A.files if k.startswith(kind)]
        print(f"{kind.strip()}: {len(ks)} arrays, {sum(k in bad for k in ks)} differ, {sum(k in loose for k in ks)} run-dependent")
    print("differing:", bad if bad else "none")
    print("run-dependent beyond the parent's spread:", far if far else "none")
    return 1 if bad or far or set(A.files) != set(B.files) else 0


if __name__ == "__main__":
    if sys.argv[1] == "--compare":
        sys.exit(compare(*sys.argv[2:5]))
    import cfm_amd._lib as L
    lib = L.load()
    for cases in (ode_cases, div_grad_cases, sde_cases, fixed_grad_cases, adaptive_grad_cases, cnf_reg_grad_cases, action_grad_cases,
                  layer_cases, pair_and_gradmlp_cases, grad_field_cases, edge_cases):
        cases(lib, L, L.ptr, L.stream_ptr)
    np.savez(sys.argv[1], **OUT)
    print(f"{len(OUT)} arrays from {L.LIB_PATH} -> {sys.argv[1]}")
