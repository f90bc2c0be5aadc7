"""Outputs of the entropic OT units (csrc/sinkhorn.hip, sinkhorn_pts.hip, sample.hip, unbalanced.hip: everything that
meets at csrc/sinkhorn_state.h) on fixed seeds, in one .npz:

    python tools/ot_unit_dump.py OUT.npz            (CFM_LIB_PATH selects the build of the library)
    python tools/ot_unit_dump.py --compare A.npz B.npz

A refactor of these units moves no floating-point operation, so two builds must agree bit for bit: run the dump once per
build, each in a fresh process, then --compare (numpy.array_equal array by array; exit 1 on any difference).
Shapes are the ones the kernels can go wrong at (the tables of tests/test_gpu_sinkhorn_paths.py and
tests/ub_shape_cases.py), not the workload's: B0 of 1, 13 and 2055, B1 of 1, 5, 1024, 1027 and 16388 among them, a
misaligned matrix, d of 1, 5, 6 and 8 for the point-cloud solver, the (max_iter, check_every) pairs of
test_check_bookkeeping, a solve behind the host's `done` poll, one that stops early in fp32 and one that goes through
the fp64 regime, and plans with a massless row for the samplers.  Per solve: f, g, iters, err, the fp64 potentials, the
first 48 bytes of the workspace (16 of words, 32 of errors), and for the matrix solver the plan and <pi, M>.

Arrays whose name ends in "~" differ between two runs of ONE build, in the last bits.  Most are sums that the device
forms with atomic adds of more than two terms in arrival order: the marginal violation, <pi, M>, the kernel sum and the
transported mass of the partial solver, with what follows from them.  The others are the potentials (and plan) of a
solve that enters the fp64 regime: in the launch where block 0 sets `precise`, the other workgroups read the flag
before or after that store, so that one half-step mixes fp32 and fp64 exps differently from run to run (iters and the
state words of those solves stay exact).  --compare counts the "~" arrays apart and they do not set the exit code;
compare two dumps of the same build to see what they do on their own.
Measurement infrastructure."""
import hashlib
import itertools
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = {}

# (B0, B1, misaligned): the row-pass families and their edges (TABLE of tests/test_gpu_sinkhorn_paths.py)
SK_SHAPES = [(1, 1024, 0), (13, 1024, 0), (67, 3072, 0), (5, 16384, 0), (2055, 1024, 0), (40, 1024, 1), (33, 16388, 0),
             (6, 16390, 0), (10, 6148, 0), (33, 1027, 0), (9, 257, 0), (1, 1, 0), (1, 5, 0), (5, 1, 0)]
CONV_SHAPES = [(13, 1024, 0), (67, 3072, 0), (2055, 1024, 0), (33, 1027, 0), (6, 16390, 0), (40, 1024, 1)]
BOOK = [(0, 10), (1, 10), (2, 10), (10, 10), (11, 10), (12, 10), (7, 3), (4, 1)]       # (max_iter, check_every)
PTS_SHAPES = [(1, 5), (13, 1024), (2055, 1027), (13, 16388)]      # 16388 points: two or more staged chunks for every d
PTS_DIMS = (1, 5, 6, 8)
UB_SHAPES = [(1, 1), (1, 7), (7, 1), (5, 3), (33, 65), (96, 257), (257, 255), (40, 514), (31, 1030), (1100, 130), (2049, 66)]


def clouds(B0, B1, d=2):
    rng = np.random.default_rng(1000 * B0 + B1 + d)
    return rng.standard_normal((B0, d)).astype(np.float32), (rng.standard_normal((B1, d)) + 0.5).astype(np.float32)


def host_cost(x0, x1):
    """fp32 squared distances from the host: independent of the cost kernels"""
    M = np.zeros((x0.shape[0], x1.shape[0]))
    for q in range(x0.shape[1]):
        M += (x0[:, q:q + 1].astype(np.float64) - x1[None, :, q].astype(np.float64)) ** 2
    return M.astype(np.float32)


def to_dev(Mnp, mis=0):
    import torch
    if not mis:
        return torch.from_numpy(Mnp).cuda().contiguous()
    buf = torch.zeros(Mnp.size + 8, dtype=torch.float32, device="cuda")     # a contiguous view one float off the 16-byte grid
    M = buf[1:1 + Mnp.size].view(*Mnp.shape)
    M.copy_(torch.from_numpy(Mnp))
    return M


def keep(t):
    """the array, or beyond 1 MiB its SHA-256: the comparison is one of bytes anyway"""
    x = t.cpu().numpy()
    return x if x.nbytes <= 1 << 20 else np.frombuffer(hashlib.sha256(x.tobytes()).digest(), np.uint8)


def put_solve(key, lib, L, B0, B1, f, g, it, err, ws, M=None, reg=None):
    """what a solve left behind; "~": see the module docstring (the violation is an atomic sum over B1 / 64 or B1 / 16
    terms; a solve that enters the fp64 regime carries the launch of the switch in its potentials)"""
    import torch
    u, v = torch.empty(B0, dtype=torch.float64, device="cuda"), torch.empty(B1, dtype=torch.float64, device="cuda")
    L.check(lib.cfm_sinkhorn_potentials_f64(L.ptr(ws), B0, B1, L.ptr(u), L.ptr(v), L.stream_ptr()), "potentials")
    state = ws[:48].cpu().numpy()
    t, tp = "~" if B1 > 32 else "", "~" if "fp64 regime" in key else ""
    OUT[key + " f" + tp], OUT[key + " g" + tp], OUT[key + " u" + tp], OUT[key + " v" + tp] = (x.cpu().numpy() for x in (f, g, u, v))
    OUT[key + " iters"], OUT[key + " state words"] = it.cpu().numpy(), state[:16]
    OUT[key + " err" + t], OUT[key + " state errors" + t] = err.cpu().numpy().view(np.int32), state[16:]
    if M is not None:
        pi, c = torch.empty((B0, B1), dtype=torch.float64, device="cuda"), torch.zeros(1, dtype=torch.float64, device="cuda")
        L.check(lib.cfm_sinkhorn_plan_f64(L.ptr(M), B0, B1, reg, L.ptr(ws), L.ptr(pi), L.stream_ptr()), "plan")
        L.check(lib.cfm_sinkhorn_cost_f64(L.ptr(M), B0, B1, reg, L.ptr(ws), L.ptr(c), L.stream_ptr()), "cost")
        OUT[key + " plan" + tp], OUT[key + " cost" + ("~" if B0 * B1 > 512 or tp else "")] = keep(pi), c.cpu().numpy()


def solve(lib, L, M, pts, B0, B1, reg, max_iter, stop_thr, check_every):
    """one solve by the matrix solver (pts None) or the point-cloud solver (pts = (x0, x1) on the device)"""
    import torch
    f, g = torch.empty(B0, device="cuda"), torch.empty(B1, device="cuda")
    it, err = torch.zeros(1, dtype=torch.int32, device="cuda"), torch.zeros(1, device="cuda")
    ws = torch.zeros(lib.cfm_workspace_bytes(L.OP_SINKHORN, B0, B1, 0), dtype=torch.uint8, device="cuda")
    tail = (reg, max_iter, stop_thr, check_every, L.ptr(f), L.ptr(g), L.ptr(it), L.ptr(err), L.ptr(ws), L.stream_ptr())
    if pts is None:
        L.check(lib.cfm_sinkhorn_log_f32(L.ptr(M), B0, B1, *tail), "sinkhorn")
    else:
        L.check(lib.cfm_sinkhorn_log_points_f32(L.ptr(pts[0]), L.ptr(pts[1]), B0, B1, pts[0].shape[1], *tail), "sinkhorn points")
    return f, g, it, err, ws


# (reg, max_iter, stop_thr, check_every): 30 iterations in fp32; POT's defaults through the fp64 regime (stops at 21);
# an early stop in fp32 (at 11); the same stop behind the host's poll of `done` (max_iter > 4096)
REGIMES = {"fixed30": (0.1, 30, 0.0, 10), "fp64 regime": (2.0, 1000, 1e-9, 10), "fp32 stop": (2.0, 1000, 1e-4, 10),
           "polled": (2.0, 5000, 1e-4, 10)}


def sinkhorn_cases(lib, L):
    for (B0, B1, mis), regime in itertools.product(SK_SHAPES, REGIMES):
        if (regime != "fixed30" and (B0, B1, mis) not in CONV_SHAPES) or (regime == "polled" and B0 != 13):
            continue
        reg, mi, st, ce = REGIMES[regime]
        M = to_dev(host_cost(*clouds(B0, B1)), mis)
        put_solve(f"sk {B0}x{B1}{' misaligned' if mis else ''} {regime}", lib, L, B0, B1, *solve(lib, L, M, None, B0, B1, reg, mi, st, ce),
                  M=M, reg=reg)
    for (B0, B1), (mi, ce) in itertools.product([(13, 1024), (33, 1027)], BOOK):
        M = to_dev(host_cost(*clouds(B0, B1)))
        put_solve(f"sk {B0}x{B1} book {mi}/{ce}", lib, L, B0, B1, *solve(lib, L, M, None, B0, B1, 0.1, mi, 0.0, ce))


def points_cases(lib, L):
    import torch
    for (B0, B1), d, regime in itertools.product(PTS_SHAPES, PTS_DIMS, REGIMES):
        if (regime != "fixed30" and B0 != 13) or (regime == "polled" and (B1 != 1024 or d != 5)):
            continue
        reg, mi, st, ce = REGIMES[regime]
        pts = tuple(torch.from_numpy(x).cuda() for x in clouds(B0, B1, d))
        put_solve(f"pts {B0}x{B1} d{d} {regime}", lib, L, B0, B1, *solve(lib, L, None, pts, B0, B1, reg, mi, st, ce))
    for (B0, B1), (mi, ce) in itertools.product([(13, 1024), (33, 1027)], BOOK):
        pts = tuple(torch.from_numpy(x).cuda() for x in clouds(B0, B1, 2))
        put_solve(f"pts {B0}x{B1} d2 book {mi}/{ce}", lib, L, B0, B1, *solve(lib, L, None, pts, B0, B1, 0.1, mi, 0.0, ce))


def uniforms(n, seed):
    u = np.random.default_rng(seed).random(n)
    u[0], u[1], u[-1] = 0.0, 0.5, 1.0 - 2.0 ** -53          # the ends of the cdf
    return u


def sampler_cases(lib, L):
    import torch
    n = 96
    for B0, B1 in [(2055, 1024), (6, 16390), (13, 1024), (1, 5), (5, 1)]:
        M = to_dev(host_cost(*clouds(B0, B1)))
        _, _, _, _, sk_ws = solve(lib, L, M, None, B0, B1, 0.5, 30, 0.0, 10)
        u01 = torch.from_numpy(uniforms(n, 7)).cuda()
        rows = torch.from_numpy(np.random.default_rng(8).integers(0, B0, n)).cuda()
        rows[0], rows[-1] = 0, B0 - 1
        i, j, jr = (torch.zeros(n, dtype=torch.int64, device="cuda") for _ in range(3))
        ws = L.workspace(L.OP_SAMPLE_DENSE, B0, B1, 0)
        L.check(lib.cfm_plan_sample_dense(L.ptr(M), B0, B1, 0.5, L.ptr(sk_ws), L.ptr(u01), n, L.ptr(i), L.ptr(j), L.ptr(ws), L.stream_ptr()),
                "sample dense")
        L.check(lib.cfm_plan_sample_rows_dense(L.ptr(M), B0, B1, 0.5, L.ptr(sk_ws), L.ptr(rows), L.ptr(u01), n, L.ptr(jr), L.ptr(ws),
                                               L.stream_ptr()), "sample rows dense")
        for name, t in (("i", i), ("j", j), ("rows j", jr)):
            OUT[f"sample dense {B0}x{B1} {name}"] = t.cpu().numpy()
    # explicit fp64 plans: sparse, with a massless row in the middle, massless last columns and a massless last row
    for B0, B1 in [(13, 5), (7, 1027), (2055, 70), (1, 1)]:
        rng = np.random.default_rng(B0 + B1)
        P = rng.random((B0, B1)) * (rng.random((B0, B1)) < 0.3)
        P[:, B1 - B1 // 3:] = 0.0
        P[B0 // 2] = 0.0
        P[B0 - 1] = 0.0
        P[0, 0] = 0.25
        pi = torch.from_numpy(P).cuda()
        u01 = torch.from_numpy(uniforms(n, 9)).cuda()
        rows = torch.from_numpy(np.random.default_rng(10).integers(0, B0, n)).cuda()
        rows[0], rows[1], rows[-1] = 0, B0 // 2, B0 - 1
        i, j, jr = (torch.zeros(n, dtype=torch.int64, device="cuda") for _ in range(3))
        ws = L.workspace(L.OP_SAMPLE_DENSE, B0, B1, 0)
        L.check(lib.cfm_plan_sample_pi_f64(L.ptr(pi), B0, B1, L.ptr(u01), n, L.ptr(i), L.ptr(j), L.ptr(ws), L.stream_ptr()), "sample pi")
        L.check(lib.cfm_plan_sample_rows_pi_f64(L.ptr(pi), B0, B1, L.ptr(rows), L.ptr(u01), n, L.ptr(jr), L.stream_ptr()), "sample rows pi")
        for name, t in (("i", i), ("j", j), ("rows j", jr)):
            OUT[f"sample pi {B0}x{B1} {name}"] = t.cpu().numpy()


def kernel_space_cases(lib, L):
    import torch
    for B0, B1 in UB_SHAPES:
        x0, x1 = clouds(B0, B1)
        M = to_dev(host_cost(x0, 0.7 * x1))
        # (entry, second parameter, max_iter, stop_thr); the partial solver's kernel sum (B0 B1 / 256 terms) and
        # transported mass (B1 / 64 terms) are atomic sums: "~" beyond two terms
        for name, fn, second, mi, st, t in (("unbalanced", lib.cfm_unbalanced_sinkhorn_f64, 1.0, 1000, 1e-6, ""),
                                            ("partial m1", lib.cfm_partial_entropic_f64, 1.0, 40, -1.0, "~"),
                                            ("partial m0.7", lib.cfm_partial_entropic_f64, 0.7, 40, -1.0, "~")):
            plan = torch.zeros((B0, B1), dtype=torch.float64, device="cuda")
            info = torch.zeros(4, dtype=torch.int32, device="cuda")
            L.check(fn(L.ptr(M), B0, B1, 0.5, second, mi, st, L.ptr(plan), L.ptr(info), L.ptr(L.workspace(L.OP_UNBALANCED, B0, B1, 0)),
                       L.stream_ptr()), name)
            t = t if (B0 * B1 > 512 or B1 > 128) else ""
            OUT[f"{name} {B0}x{B1} plan{t}"], OUT[f"{name} {B0}x{B1} info"] = keep(plan), info.cpu().numpy()


KINDS = ("sk ", "pts ", "sample dense ", "sample pi ", "unbalanced ", "partial ")


def compare(a, b):
    A, B = np.load(a), np.load(b)
    # (bytes, not values: a NaN plan equals itself)
    differ = lambda k: A[k].shape != B[k].shape or A[k].dtype != B[k].dtype or A[k].tobytes() != B[k].tobytes()
    missing = sorted(set(A.files) ^ set(B.files))
    bad = [k for k in sorted(set(A.files) & set(B.files)) if differ(k)]
    for kind in KINDS:
        ks = [k for k in A.files if k.startswith(kind)]
        exact, atomic = [k for k in ks if not k.endswith("~")], [k for k in ks if k.endswith("~")]
        print(f"{kind.strip()}: {len(exact)} arrays, {sum(k in bad for k in exact)} differ; "
              f"{len(atomic)} run-dependent (~), {sum(k in bad for k in atomic)} differ")
    strict = [k for k in bad if not k.endswith("~")]
    print("only in one dump:", missing if missing else "none")
    print("differing:", strict if strict else "none")
    print("differing run-dependent arrays:", len([k for k in bad if k.endswith("~")]))
    return 1 if strict or missing else 0


if __name__ == "__main__":
    if sys.argv[1] == "--compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    import torch
    import cfm_amd._lib as L
    lib = L.load()
    for cases in (sinkhorn_cases, points_cases, sampler_cases, kernel_space_cases):
        cases(lib, L)
        torch.cuda.synchronize()
    np.savez(sys.argv[1], **OUT)
    print(f"{len(OUT)} arrays from {L.LIB_PATH} -> {sys.argv[1]}")
