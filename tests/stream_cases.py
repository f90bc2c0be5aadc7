"""Case table of tests/test_gpu_stream_contract.py and tests/test_stream_cases_host.py: one or more cases per C entry of
include/cfm_gfx950.h that takes a `stream`.

A case gives
  make(seed, dev) -> dict   every buffer the entry READS: device tensors (the nets' weights included) and, under the keys of
                            HOST_KEYS, the host data arrays (t_span, step records) as NumPy arrays.  seed 0 is the TRUE
                            input set, seed 1 the DECOY set: the same shapes, valid values (finite, in-range indices, valid
                            permutations, strictly monotone grids of the same direction, positive reg) from another seed.
  prep(inp)                 optional: device buffers derived from the ADDRESSES of inp (Adam's record table); run before the
                            side-stream section, because a host-to-device copy from pageable memory may block the host.
  op(inp) -> (outs, host)   one call of the entry on the CURRENT stream.  outs: list of (label, tensor, rtol); rtol None =
                            bit for bit.  host: the host results (return code, n_steps, nfe, ...).  op may work in place:
                            the harness hands it a private copy of the inputs.
  syncs                     the entry synchronises the host before it returns (include/cfm_gfx950.h names those).

The optimal-transport entries go through the tensor-level functions of cfm_amd.optimal_transport; the network, ODE, CNF and
SDE entries are called through the binding's library object on weight tensors the case owns (their Python wrappers take
Modules and build the pointer tables themselves, so a working buffer could not be swapped under them).

A tolerance appears only where the entry adds floating-point partial sums with atomics in an order that changes from run to
run (the kernel sums of cfm_rbf_mix_sum_f32 and cfm_sinkhorn_cost_f64, the marginal error of the Sinkhorn solves, the
total cost of the exact solvers, the mass normalisation of the kernel-space solvers): that output alone is compared at a
relative tolerance named in the case — the RBF sum at the 1e-6 of its own tests (tests/glue_cases.py), an fp64 sum at 1e-12
(the bound tests/test_gpu_unbalanced.py puts on a plan's mass; 2^-52 per addition leaves room for 4000 of them), the fp32
marginal error at 1e-5 — and everything else bit for bit.  The assignment cases compare the permutation only.

The factories take shape parameters whose defaults are the table's shapes, and the ops read their sizes from the inputs:
tests/test_gpu_memory_contract.py builds its edge shapes (FOOTPRINT_EXTRA) from them; the table's cases and ids do not move.

Importing this module needs neither a device nor the library (the host test reads the table's keys)."""
import ctypes
import math
import struct

import numpy as np
import torch

HOST_KEYS = ("t_span", "steps")

# Entries with a `stream` parameter that enqueue no work.
EXEMPT = {
    "cfm_stream_create_cu_mask": "creates a stream (`stream` is the output handle); enqueues nothing",
    "cfm_stream_destroy": "destroys the stream it is given; enqueues nothing",
}
# ... and the only names that list may ever hold
EXEMPT_ALLOWED = {"cfm_stream_create_cu_mask", "cfm_stream_destroy", "cfm_ode_fixed_grad_available",
                  "cfm_ode_adaptive_grad_available"}

# Entries that synchronise the host (data-dependent control flow): named by the header's conventions.
SYNCING = {"cfm_assign_exact_f32", "cfm_assign_exact_batch_f32", "cfm_ode_dopri5_mlp_f32", "cfm_ode_adaptive_mlp_f32",
           "cfm_ode_dopri5_cnf_mlp_f32", "cfm_ode_adaptive_cnf_mlp_f32", "cfm_ode_adaptive_rec_mlp_f32",
           "cfm_ode_adaptive_gradmlp_f32"}

# Entries that take host DATA (a grid or step records, not pointer tables): "a HOST array passed to an entry may be
# overwritten or freed as soon as the call returns".
HOST_DATA = ["cfm_ode_fixed_mlp_f32", "cfm_ode_fixed_cnf_mlp_f32", "cfm_ode_fixed_gradmlp_f32",
             "cfm_ode_fixed_cnf_gradmlp_f32", "cfm_ode_fixed_pair_mlp_f32", "cfm_ode_euler_cnf_reg_mlp_f32",
             "cfm_ode_fixed_grad_f32", "cfm_cnf_euler_grad_f32", "cfm_cnf_reg_euler_grad_f32", "cfm_sde_em_mlp_f32",
             "cfm_sde_srk_mlp_f32"]
# ... and further cases of those entries for the host-array test (the first case of each entry is always taken)
HOST_DATA_EXTRA = [("cfm_sde_em_mlp_f32", "long-640KB")]

vp, ci = ctypes.c_void_p, ctypes.c_int


class Case:
    def __init__(self, entry, name, make, op, prep=None, note=""):
        self.entry, self.name, self.make, self.op, self.prep, self.note = entry, name, make, op, prep, note
        self.syncs = entry in SYNCING

    @property
    def id(self):
        return f"{self.entry}-{self.name}"


CASES = {}


def case(entry, name="base", prep=None, note=""):
    """Decorator on op; the function's `make` attribute is set by the caller: case(...)(make, op)."""
    def reg(make, op):
        CASES.setdefault(entry, []).append(Case(entry, name, make, op, prep, note))
    return reg


# ------------------------------------------------------------------------------------------------ helpers
def _lib():
    from cfm_amd import _lib as L
    return L


def _g(seed, salt):
    return torch.Generator().manual_seed(1000 * salt + 17 * seed + 3)


def _randn(g, *shape):
    return torch.randn(*shape, generator=g, dtype=torch.float32)


def _rand(g, *shape):
    return torch.rand(*shape, generator=g, dtype=torch.float32)


def _to(dev, d):
    return {k: (v.to(dev).contiguous() if torch.is_tensor(v) else v) for k, v in d.items()}


def _net(g, dims, pre=""):
    """torch.nn.Linear's initialisation range for each layer: W{l} [out, in], b{l} [out]."""
    out = {}
    for l in range(len(dims) - 1):
        k = 1.0 / math.sqrt(dims[l])
        out[f"{pre}W{l}"] = (_rand(g, dims[l + 1], dims[l]) * 2 - 1) * k
        out[f"{pre}b{l}"] = (_rand(g, dims[l + 1]) * 2 - 1) * k
    return out


def _tables(inp, pre=""):
    n = 0
    while f"{pre}W{n}" in inp:
        n += 1
    Ws, bs = [inp[f"{pre}W{l}"] for l in range(n)], [inp[f"{pre}b{l}"] for l in range(n)]
    dims = [Ws[0].shape[1]] + [w.shape[0] for w in Ws]
    return (vp * n)(*[w.data_ptr() for w in Ws]), (vp * n)(*[b.data_ptr() for b in bs]), (ci * (n + 1))(*dims), dims, n


def _ptrs(ts):
    return (vp * len(ts))(*[(t.data_ptr() if t is not None else 0) for t in ts])


def _hp(a):
    """Pointer into a NumPy host array."""
    return a.ctypes.data_as(vp)


def _grid(seed, n_t, reverse=False):
    """Strictly monotone float32 grid; the decoy has the same direction and another end."""
    ts = np.linspace(0.0, 1.0 if seed == 0 else 0.7, n_t).astype(np.float32)
    return np.ascontiguousarray(ts[::-1] if reverse else ts)


def _ws(op, a, b, c, dev):
    return _lib().workspace(op, a, b, c, dev)


def _clouds(g, B0, B1, d):
    return _randn(g, B0, d), _randn(g, B1, d) + 0.25


def _cost(g, B0, B1, d=3):
    """A normalised squared-distance matrix (max 1), built on the host."""
    x0, x1 = _clouds(g, B0, B1, d)
    M = torch.cdist(x0.double(), x1.double()) ** 2
    return (M / M.max()).float()


B0, B1 = 300, 200          # Sinkhorn and cost: more than one tile each way
NA = 257                   # assignment: past the one-workgroup solver (n <= 256)
BS = 130                   # the 64-row small-field kernels: three workgroups, the last one partial
REG = 0.05


# ------------------------------------------------------------------------------------------------ cost
def _mk_clouds(B0_, B1_, d):
    def make(seed, dev):
        x0, x1 = _clouds(_g(seed, 1), B0_, B1_, d)
        return _to(dev, {"x0": x0, "x1": x1})
    return make


def _op_cost(matrix_cores):
    def op(inp):
        from cfm_amd import optimal_transport as ot
        return [("M", ot.cost_matrix(inp["x0"], inp["x1"], matrix_cores=matrix_cores), None)], ()
    return op


case("cfm_sqeuclid_cost_f32")(_mk_clouds(B0, B1, 5), _op_cost(False))
case("cfm_sqeuclid_cost_ws_f32", "gram", note="d >= 64 and B >= 256: the matrix-core form")(_mk_clouds(300, 257, 64), _op_cost(True))


def _mk_matrix(seed, dev):
    g = _g(seed, 2)
    return _to(dev, {"M": _rand(g, B0, B1) + 0.1, "mx": _rand(g, 1) + 0.5})


def _op_scale_inv(inp):
    L = _lib()
    rc = L.load().cfm_scale_inv_f32(L.ptr(inp["M"]), inp["M"].numel(), L.ptr(inp["mx"]), L.stream_ptr())
    return [("M", inp["M"], None)], (rc,)


def _op_sqrt(inp):
    L = _lib()
    rc = L.load().cfm_sqrt_inplace_f32(L.ptr(inp["M"]), inp["M"].numel(), L.stream_ptr())
    return [("M", inp["M"], None)], (rc,)


case("cfm_scale_inv_f32")(_mk_matrix, _op_scale_inv)
case("cfm_sqrt_inplace_f32")(_mk_matrix, _op_sqrt)


# ------------------------------------------------------------------------------------------------ Sinkhorn family
SK_ITERS = 20              # stop_thr = 0: a fixed iteration count, far above the fp32 noise floor (no switch to fp64 exp)
ERR_RTOL = 1e-5            # last_err: fp32 partial sums added with atomics


def _mk_cost(seed, dev, b0=B0, b1=B1):
    return _to(dev, {"M": _cost(_g(seed, 3), b0, b1)})


def _op_sinkhorn(inp):
    from cfm_amd import optimal_transport as ot
    r = ot.sinkhorn_log(inp["M"], REG, max_iter=SK_ITERS, stop_thr=0.0)
    return [("f", r.f, None), ("g", r.g, None), ("iters", r.iters, None), ("err", r.err, ERR_RTOL)], ()


def _op_sinkhorn_points(inp):
    from cfm_amd import optimal_transport as ot
    r = ot.sinkhorn_log_points(inp["x0"], inp["x1"], None, 0.5, max_iter=SK_ITERS, stop_thr=0.0)
    return [("f", r.f, None), ("g", r.g, None), ("iters", r.iters, None), ("err", r.err, ERR_RTOL)], ()


case("cfm_sinkhorn_log_f32")(_mk_cost, _op_sinkhorn)
case("cfm_sinkhorn_log_points_f32")(_mk_clouds(B0, B1, 2), _op_sinkhorn_points)


def _mk_solved(with_u=0, rows=False, b0=B0, b1=B1):
    """M and the Sinkhorn workspace of a finished solve on it (default stream, synchronised); u01 / rows for the samplers."""
    def make(seed, dev):
        from cfm_amd import optimal_transport as ot
        g = _g(seed, 4)
        M = _cost(g, b0, b1).to(dev)
        r = ot.sinkhorn_log(M, REG, max_iter=SK_ITERS, stop_thr=0.0)
        torch.cuda.synchronize()
        inp = {"M": M, "ws": r.ws}
        if with_u:
            inp["u01"] = torch.rand(with_u, generator=g, dtype=torch.float64).to(dev)
        if rows:
            inp["rows"] = torch.randint(0, b0, (with_u,), generator=g, dtype=torch.int64).to(dev)
        return inp
    return make


def _result(inp):
    from cfm_amd import optimal_transport as ot
    r = ot.SinkhornResult()
    r.M, r.ws, r.reg = inp["M"], inp["ws"], REG
    return r


def _op_potentials(inp):
    L = _lib()
    dev = inp["M"].device
    b0, b1 = inp["M"].shape
    u, v = torch.empty(b0, dtype=torch.float64, device=dev), torch.empty(b1, dtype=torch.float64, device=dev)
    rc = L.load().cfm_sinkhorn_potentials_f64(L.ptr(inp["ws"]), b0, b1, L.ptr(u), L.ptr(v), L.stream_ptr())
    return [("u", u, None), ("v", v, None)], (rc,)


def _op_plan(inp):
    from cfm_amd import optimal_transport as ot
    return [("pi", ot.sinkhorn_plan(_result(inp)), None)], ()


def _op_sk_cost(inp):
    L = _lib()
    out = torch.zeros(1, dtype=torch.float64, device=inp["M"].device)
    b0, b1 = inp["M"].shape
    rc = L.load().cfm_sinkhorn_cost_f64(L.ptr(inp["M"]), b0, b1, REG, L.ptr(inp["ws"]), L.ptr(out), L.stream_ptr())
    return [("cost", out, 1e-12)], (rc,)


case("cfm_sinkhorn_potentials_f64")(_mk_solved(), _op_potentials)
case("cfm_sinkhorn_plan_f64")(_mk_solved(), _op_plan)
case("cfm_sinkhorn_cost_f64", note="fp64 partial sums added with atomics: 1e-12 relative")(_mk_solved(), _op_sk_cost)


def _op_kernel_space(which):
    def op(inp):
        from cfm_amd import optimal_transport as ot
        plan, info = (ot.unbalanced_plan(inp["M"], REG, 1.0, max_iter=30) if which == "ub"
                      else ot.partial_plan(inp["M"], REG, 0.7, max_iter=30))
        return [("plan", plan, 1e-12), ("info", info, None)], ()
    return op


case("cfm_unbalanced_sinkhorn_f64", note="plan at 1e-12: fp64 sums by atomics")(_mk_cost, _op_kernel_space("ub"))
case("cfm_partial_entropic_f64", note="plan at 1e-12: the mass normalisation is an atomic fp64 sum")(_mk_cost, _op_kernel_space("partial"))


# ------------------------------------------------------------------------------------------------ exact solvers
def _mk_square(nb=1, n=NA):
    """n = 1: _cost normalises by a maximum that is zero there; a constant 1 x 1 matrix instead."""
    def make(seed, dev):
        g = _g(seed, 5)
        if n == 1:
            return _to(dev, {f"M{k}": torch.full((1, 1), 0.5 + 0.25 * seed + k) for k in range(nb)})
        return _to(dev, {f"M{k}": _cost(g, n, n) for k in range(nb)})
    return make


def _op_assign(inp):
    from cfm_amd import optimal_transport as ot
    return [("perm", ot.assign_exact(inp["M0"]), None)], ()


def _op_assign_batch(inp):
    from cfm_amd import optimal_transport as ot
    return [("perm", ot.assign_exact_batch([inp[k] for k in sorted(inp) if k[0] == "M"]), None)], ()


case("cfm_assign_exact_f32")(_mk_square(1), _op_assign)
case("cfm_assign_exact_batch_f32")(_mk_square(2), _op_assign_batch)


def _op_transport(inp):
    L = _lib()
    M = inp["M"]
    dev = M.device
    b0, b1 = M.shape
    plan = torch.empty((b0, b1), dtype=torch.float64, device=dev)
    tot = torch.empty(1, dtype=torch.float64, device=dev)
    info = torch.empty(8, dtype=torch.int32, device=dev)
    ws = _ws(L.OP_TRANSPORT, b0, b1, 0, dev)
    rc = L.load().cfm_transport_exact_f32(L.ptr(M), b0, b1, None, L.ptr(plan), L.ptr(tot), L.ptr(info), L.ptr(ws), L.stream_ptr())
    return [("plan", plan, None), ("total", tot, 1e-12), ("status", info[:1], None)], (rc,)


case("cfm_transport_exact_f32", note="the plan is integer units / lcm: exact; its cost is an fp64 sum, 1e-12")(_mk_cost, _op_transport)


# ------------------------------------------------------------------------------------------------ samplers, gathers
NDRAW = 515


def _mk_perm(seed, dev):
    g = _g(seed, 6)
    return _to(dev, {"perm": torch.randperm(1000, generator=g).to(torch.int32), "u01": torch.rand(NDRAW, generator=g, dtype=torch.float64)})


def _op_sample_perm(inp):
    from cfm_amd import optimal_transport as ot
    i, j = ot.sample_perm(inp["perm"], inp["u01"], 1000)
    return [("i", i, None), ("j", j, None)], ()


def _op_sample_dense(inp):
    from cfm_amd import optimal_transport as ot
    i, j = ot.sample_dense(_result(inp), inp["u01"])
    return [("i", i, None), ("j", j, None)], ()


def _op_rows_dense(inp):
    from cfm_amd import optimal_transport as ot
    return [("j", ot.sample_rows_dense(_result(inp), inp["rows"], inp["u01"]), None)], ()


def _mk_pi(rows):
    def make(seed, dev):
        g = _g(seed, 7)
        pi = torch.rand(B0, B1, generator=g, dtype=torch.float64) + 0.01
        inp = {"pi": pi / pi.sum(), "u01": torch.rand(NDRAW, generator=g, dtype=torch.float64)}
        if rows:
            inp["rows"] = torch.randint(0, B0, (NDRAW,), generator=g, dtype=torch.int64)
        return _to(dev, inp)
    return make


def _op_sample_pi(inp):
    from cfm_amd import optimal_transport as ot
    i, j = ot.sample_pi(inp["pi"], inp["u01"])
    return [("i", i, None), ("j", j, None)], ()


def _op_rows_pi(inp):
    from cfm_amd import optimal_transport as ot
    return [("j", ot.sample_rows_pi(inp["pi"], inp["rows"], inp["u01"]), None)], ()


case("cfm_plan_sample_perm")(_mk_perm, _op_sample_perm)
case("cfm_plan_sample_dense")(_mk_solved(NDRAW), _op_sample_dense)
case("cfm_plan_sample_pi_f64")(_mk_pi(False), _op_sample_pi)
case("cfm_plan_sample_rows_dense")(_mk_solved(NDRAW, rows=True), _op_rows_dense)
case("cfm_plan_sample_rows_pi_f64")(_mk_pi(True), _op_rows_pi)

XB, XD = 1000, 5


def _mk_xt(kind, B=XB, d=XD):
    def make(seed, dev):
        g = _g(seed, 8)
        inp = {"x0": _randn(g, B, d), "x1": _randn(g, B, d) + 0.25, "eps": _randn(g, B, d),
               "i": torch.randperm(B, generator=g), "j": torch.randperm(B, generator=g)}
        if kind == "icfm":
            inp["t"] = _rand(g, B)
        else:
            inp["coef"] = _rand(g, B, 4) * 0.9 + 0.05
        return _to(dev, inp)
    return make


def _op_xt(inp):
    L = _lib()
    xt, ut, x0g, x1g = (torch.empty_like(inp["eps"]) for _ in range(4))
    p = L.ptr
    rc = L.load().cfm_sample_xt_ut_f32(L.VARIANT_ICFM, p(inp["x0"]), p(inp["x1"]), p(inp["i"]), p(inp["j"]), p(inp["t"]),
                                       p(inp["eps"]), 0.1, None, None, None, *inp["eps"].shape, p(xt), p(ut), p(x0g), p(x1g), L.stream_ptr())
    return [("xt", xt, None), ("ut", ut, None), ("x0g", x0g, None), ("x1g", x1g, None)], (rc,)


def _op_xt_sched(inp):
    L = _lib()
    xt, ut = torch.empty_like(inp["eps"]), torch.empty_like(inp["eps"])
    p = L.ptr
    rc = L.load().cfm_sample_xt_ut_sched_f32(p(inp["x0"]), p(inp["x1"]), p(inp["i"]), p(inp["j"]), p(inp["coef"]), p(inp["eps"]),
                                             None, *inp["eps"].shape, p(xt), p(ut), L.stream_ptr())
    return [("xt", xt, None), ("ut", ut, None)], (rc,)


def _op_dsbm_sample(inp):
    L = _lib()
    xt, ft, bt = (torch.empty_like(inp["eps"]) for _ in range(3))
    p = L.ptr
    rc = L.load().cfm_sample_dsbm_f32(p(inp["x0"]), p(inp["x1"]), p(inp["i"]), p(inp["j"]), p(inp["coef"]), p(inp["eps"]),
                                      *inp["eps"].shape, p(xt), p(ft), p(bt), L.stream_ptr())
    return [("xt", xt, None), ("ft", ft, None), ("bt", bt, None)], (rc,)


def _op_gather(inp):
    from cfm_amd import optimal_transport as ot
    return [("out", ot.gather_rows(inp["x0"], inp["i"]), None)], ()


case("cfm_sample_xt_ut_f32")(_mk_xt("icfm"), _op_xt)
case("cfm_sample_xt_ut_sched_f32")(_mk_xt("sched"), _op_xt_sched)
case("cfm_sample_dsbm_f32")(_mk_xt("sched"), _op_dsbm_sample)
case("cfm_gather_rows")(_mk_xt("icfm"), _op_gather)

TT = 5


def _mk_traj(seed, dev, B=XB, d=XD):
    g = _g(seed, 9)
    return _to(dev, {"X": _randn(g, B, TT, d), "t_select": torch.randint(0, TT - 1, (B,), generator=g, dtype=torch.int64),
                     "t": _rand(g, B) * 0.99, "eps": _randn(g, B, d)})


def _op_traj(inp):
    L = _lib()
    p = L.ptr
    xt, ut = torch.empty_like(inp["eps"]), torch.empty_like(inp["eps"])
    tn = torch.empty_like(inp["t"])
    B, d = inp["eps"].shape
    rc = L.load().cfm_traj_xt_ut_f32(0, L.VARIANT_ICFM, p(inp["X"]), B, TT, d, None, p(inp["t_select"]), p(inp["t"]),
                                     p(inp["eps"]), 0.1, None, 0, None, p(xt), p(ut), p(tn), L.stream_ptr())
    return [("xt", xt, None), ("ut", ut, None), ("t_net", tn, None)], (rc,)


case("cfm_traj_xt_ut_f32")(_mk_traj, _op_traj)


# ------------------------------------------------------------------------------------------------ MLP inference / training
def _mk_fwd(B, d, w):
    def make(seed, dev):
        g = _g(seed, 10)
        return _to(dev, {**_net(g, [d + 1, w, w, w, d]), "x": _randn(g, B, d), "t": _rand(g, B)})
    return make


def _op_fwd(inp):
    L = _lib()
    Wp, bp, cd, dims, n = _tables(inp)
    x = inp["x"]
    B = x.shape[0]
    out = torch.empty((B, dims[n]), dtype=torch.float32, device=x.device)
    ws = _ws(L.OP_MLP, B, max(dims[1:n]), 0, x.device)
    rc = L.load().cfm_mlp_forward_f32(L.ptr(x), L.ptr(inp["t"]), 1, Wp, bp, cd, n, B, L.ptr(out), L.ptr(ws), L.stream_ptr())
    return [("out", out, None)], (rc,)


case("cfm_mlp_forward_f32", "small")(_mk_fwd(BS, 5, 64), _op_fwd)
case("cfm_mlp_forward_f32", "layers-784x512", note="the layer driver's shape")(_mk_fwd(24, 784, 512), _op_fwd)

TD = [6, 64, 64, 64, 5]    # training nets: [xt | t] -> 5


def _train_bufs(dims, B, dev, nets=1):
    hid = [torch.empty((B, dims[l + 1]), dtype=torch.float32, device=dev) for _ in range(nets) for l in range(len(dims) - 2)]
    pre = [torch.empty_like(h) for h in hid]
    return hid, pre


def _train_ws(dims, B, dev, nets=1):
    L = _lib()
    n = len(dims) - 1
    one = L.load().cfm_workspace_bytes(L.OP_MLP_TRAIN, B, max(dims), max(dims[l] * dims[l + 1] for l in range(n)))
    return torch.empty(one * nets, dtype=torch.uint8, device=dev)


def _mk_fwd_train(seed, dev, B=BS):
    g = _g(seed, 11)
    return _to(dev, {**_net(g, TD), "x": _randn(g, B, TD[0])})


def _op_fwd_train(inp):
    L = _lib()
    Wp, bp, cd, dims, n = _tables(inp)
    dev = inp["x"].device
    B = inp["x"].shape[0]
    hid, pre = _train_bufs(dims, B, dev)
    out = torch.empty((B, dims[n]), dtype=torch.float32, device=dev)
    rc = L.load().cfm_mlp_forward_train_f32(L.ptr(inp["x"]), Wp, bp, cd, n, B, _ptrs(hid), _ptrs(pre), L.ptr(out), L.stream_ptr())
    return [("out", out, None)] + [(f"hidden{l}", h, None) for l, h in enumerate(hid)] + [(f"preact{l}", z, None) for l, z in enumerate(pre)], (rc,)


case("cfm_mlp_forward_train_f32")(_mk_fwd_train, _op_fwd_train)


def _mk_backward(seed, dev, B=BS):
    g = _g(seed, 12)
    inp = {**_net(g, TD), "a0": _randn(g, B, TD[0]), "dout": _randn(g, B, TD[-1])}
    for l in range(1, 4):
        inp[f"z{l}"] = _randn(g, B, TD[l])
        inp[f"a{l}"] = torch.nn.functional.selu(inp[f"z{l}"])
    return _to(dev, inp)


def _grads(inp, pre=""):
    Ws, bs = [], []
    n = 0
    while f"{pre}W{n}" in inp:
        Ws.append(torch.empty_like(inp[f"{pre}W{n}"])); bs.append(torch.empty_like(inp[f"{pre}b{n}"]))
        n += 1
    return Ws, bs


def _grad_outs(dW, db):
    return [(f"dW{l}", w, None) for l, w in enumerate(dW)] + [(f"db{l}", b, None) for l, b in enumerate(db)]


def _op_backward(inp):
    L = _lib()
    Wp, _, cd, dims, n = _tables(inp)
    dev = inp["dout"].device
    dW, db = _grads(inp)
    dx = torch.empty_like(inp["a0"])
    B = inp["a0"].shape[0]
    ws = _train_ws(dims, B, dev)
    rc = L.load().cfm_mlp_backward_f32(_ptrs([inp[f"a{l}"] for l in range(n)]), _ptrs([None] + [inp[f"z{l}"] for l in range(1, n)]),
                                       Wp, cd, n, B, L.ptr(inp["dout"]), _ptrs(dW), _ptrs(db), L.ptr(dx), L.ptr(ws), L.stream_ptr())
    return _grad_outs(dW, db) + [("dx", dx, None)], (rc,)


case("cfm_mlp_backward_f32")(_mk_backward, _op_backward)


def _mk_step(kind, B=BS):
    def make(seed, dev):
        g = _g(seed, 13)
        d, o = TD[0] - 1, TD[-1]
        inp = {**_net(g, TD, "f"), "xt": _randn(g, B, d), "t": _rand(g, B), "ut": _randn(g, B, o)}
        if kind != "reg":
            inp.update(_net(g, TD, "s"))
            inp.update({"eps": _randn(g, B, o), "lam": _rand(g, B) + 0.5, "wb": _rand(g, B) + 0.5})
        return _to(dev, inp)
    return make


def _op_regression(inp):
    L = _lib()
    p = L.ptr
    Wp, bp, cd, dims, n = _tables(inp, "f")
    dev = inp["xt"].device
    B = inp["xt"].shape[0]
    hid, pre = _train_bufs(dims, B, dev)
    dW, db = _grads(inp, "f")
    g = torch.empty((B, dims[n]), dtype=torch.float32, device=dev)
    loss = torch.empty(1, dtype=torch.float32, device=dev)
    ws = _train_ws(dims, B, dev)
    rc = L.load().cfm_mlp_regression_step_f32(p(inp["xt"]), p(inp["t"]), p(inp["ut"]), Wp, bp, cd, n, B, _ptrs(hid), _ptrs(pre),
                                              p(g), _ptrs(dW), _ptrs(db), p(loss), None, p(ws), L.stream_ptr())
    return _grad_outs(dW, db) + [("g", g, None), ("loss", loss, None)], (rc,)


def _two_net(inp):
    Wf, bf, cd, dims, n = _tables(inp, "f")
    Wsn, bsn, _, _, _ = _tables(inp, "s")
    Wp, bp = (vp * (2 * n))(*(list(Wf) + list(Wsn))), (vp * (2 * n))(*(list(bf) + list(bsn)))
    dWf, dbf = _grads(inp, "f")
    dWs, dbs = _grads(inp, "s")
    return Wp, bp, cd, dims, n, dWf + dWs, dbf + dbs


def _op_sf2m(inp):
    L = _lib()
    p = L.ptr
    Wp, bp, cd, dims, n, dW, db = _two_net(inp)
    dev = inp["xt"].device
    B = inp["xt"].shape[0]
    hid, pre = _train_bufs(dims, B, dev, nets=2)
    gf = torch.empty((B, dims[n]), dtype=torch.float32, device=dev)
    gs = torch.empty_like(gf)
    losses = torch.empty(2, dtype=torch.float32, device=dev)
    ws = _train_ws(dims, B, dev, nets=2)
    rc = L.load().cfm_mlp_sf2m_step_f32(p(inp["xt"]), p(inp["t"]), p(inp["ut"]), p(inp["eps"]), p(inp["lam"]), Wp, bp, _ptrs(hid),
                                        _ptrs(pre), _ptrs(dW), _ptrs(db), cd, n, B, p(gf), p(gs), p(losses), 0.5, p(ws), L.stream_ptr())
    return _grad_outs(dW, db) + [("g_flow", gf, None), ("g_score", gs, None), ("losses", losses, None)], (rc,)


def _op_dsbm_step(inp):
    L = _lib()
    p = L.ptr
    Wp, bp, cd, dims, n, dW, db = _two_net(inp)
    dev = inp["xt"].device
    B = inp["xt"].shape[0]
    hid, pre = _train_bufs(dims, B, dev, nets=2)
    gf = torch.empty((B, dims[n]), dtype=torch.float32, device=dev)
    gb = torch.empty_like(gf)
    losses = torch.empty(2, dtype=torch.float32, device=dev)
    ws = _train_ws(dims, B, dev, nets=2)
    rc = L.load().cfm_mlp_dsbm_step_f32(p(inp["xt"]), p(inp["t"]), p(inp["ut"]), p(inp["eps"]), p(inp["lam"]), p(inp["wb"]), Wp, bp,
                                        _ptrs(hid), _ptrs(pre), _ptrs(dW), _ptrs(db), cd, n, B, p(gf), p(gb), p(losses), p(ws), L.stream_ptr())
    return _grad_outs(dW, db) + [("g_fwd", gf, None), ("g_bwd", gb, None), ("losses", losses, None)], (rc,)


case("cfm_mlp_regression_step_f32")(_mk_step("reg"), _op_regression)
case("cfm_mlp_sf2m_step_f32")(_mk_step("two"), _op_sf2m)
case("cfm_mlp_dsbm_step_f32")(_mk_step("two"), _op_dsbm_step)

ADAM_NUMELS = [257, 1, 65537]


def _mk_adam(seed, dev, numels=tuple(ADAM_NUMELS)):
    g = _g(seed, 14)
    inp = {}
    for k, n in enumerate(numels):
        inp.update({f"p{k}": _randn(g, n), f"g{k}": _randn(g, n), f"m{k}": _randn(g, n) * 0.1, f"v{k}": _rand(g, n) * 0.01})
    return _to(dev, inp)


def _adam_numels(inp):
    out = []
    while f"p{len(out)}" in inp:
        out.append(inp[f"p{len(out)}"].numel())
    return out


def _prep_adam(inp):
    rec = [[inp[f"{c}{k}"].data_ptr() for c in "pgmv"] + [n] for k, n in enumerate(_adam_numels(inp))]
    inp["_table"] = torch.tensor(rec, dtype=torch.int64).to(inp["p0"].device)


def _op_adam(inp):
    L = _lib()
    nt = len(_adam_numels(inp))
    rc = L.load().cfm_adam_step_f32(L.ptr(inp["_table"]), nt, 1e-3, 0.9, 0.999, 1e-8, 0.01, 3, 0.5, L.stream_ptr())
    return [(f"{c}{k}", inp[f"{c}{k}"], None) for k in range(nt) for c in "pgmv"], (rc,)


case("cfm_adam_step_f32", prep=_prep_adam)(_mk_adam, _op_adam)


# ------------------------------------------------------------------------------------------------ SDE steps, RBF sums
SN = 70001


def _mk_sde_step(seed, dev):
    g = _g(seed, 15)
    return _to(dev, {k: _randn(g, SN) for k in ("y", "v1", "s1", "v2", "s2", "v3", "s3", "xi1", "xi2")})


def _op_em_step(inp):
    L = _lib()
    p = L.ptr
    rc = L.load().cfm_sde_em_step_f32(p(inp["y"]), p(inp["v1"]), p(inp["s1"]), p(inp["xi1"]), 0.01, 0.3, 1.0, SN, L.stream_ptr())
    return [("y", inp["y"], None)], (rc,)


def _op_srk_step(inp):
    L = _lib()
    p = L.ptr
    ys = torch.empty_like(inp["y"])
    rc = L.load().cfm_sde_srk_step_f32(2, p(inp["y"]), p(ys), p(inp["v1"]), p(inp["s1"]), p(inp["v2"]), p(inp["s2"]), p(inp["v3"]),
                                       p(inp["s3"]), p(inp["xi1"]), p(inp["xi2"]), 0.01, 0.3, 1.0, SN, L.stream_ptr())
    return [("ys", ys, None)], (rc,)


case("cfm_sde_em_step_f32")(_mk_sde_step, _op_em_step)
case("cfm_sde_srk_step_f32", "stage2")(_mk_sde_step, _op_srk_step)


def _mk_rbf(seed, dev):
    g = _g(seed, 16)
    return _to(dev, {"D": _randn(g, 70001) ** 2, "gammas": torch.tensor([1.0 / (2 * s * s) for s in (0.1, 1.0, 10.0)], dtype=torch.float32) * (1 + seed)})


def _op_rbf(inp):
    L = _lib()
    out = torch.zeros(1, dtype=torch.float64, device=inp["D"].device)
    rc = L.load().cfm_rbf_mix_sum_f32(L.ptr(inp["D"]), inp["D"].numel(), L.ptr(inp["gammas"]), 3, L.ptr(out), L.stream_ptr())
    return [("sum", out, 1e-6)], (rc,)


case("cfm_rbf_mix_sum_f32", note="atomic fp64 sum: RBF_RTOL = 1e-6 of tests/glue_cases.py")(_mk_rbf, _op_rbf)

SDE_STEPS = 12
SDE_OUT = 4
SDE_LONG = 40000           # 16-byte records: a 640 KB host array, far past any small-copy staging threshold


def _sde_records(seed, srk, n=SDE_STEPS):
    """Step records of a uniform grid of n steps on [0, 1] (decoy: [0, 0.7]) with four states an output: the layouts of
    cfm_amd.sde._em_records / _srk_records, sigma = 0.3."""
    T = 1.0 if seed == 0 else 0.7
    h = T / n
    every = n // SDE_OUT
    recs = []
    for k in range(n):
        t, out = k * h, 1 if (k % every == every - 1) else 0
        gs = 0.3 * math.sqrt(h)
        recs.append(struct.pack("<ffffffii", t, t + h, t + 0.5 * h, h, gs, 0.75 * gs, out, 0) if srk
                    else struct.pack("<fffi", t, h, gs, out))
    return np.frombuffer(b"".join(recs), dtype=np.uint8).copy()


def _mk_sde(srk, n_steps=SDE_STEPS, B=BS, d=2):
    def make(seed, dev):
        g = _g(seed, 17)
        dims = [d + 1, 64, 64, 64, d]
        inp = _to(dev, {**_net(g, dims, "f"), **_net(g, dims, "s"), "y0": _randn(g, B, d)})
        inp["steps"] = _sde_records(seed, srk, n_steps)
        return inp
    return make


def _op_sde(srk, n_steps=SDE_STEPS, slack=256):
    """slack: bytes of workspace beyond the sizeof(record) * n_steps the header asks for."""
    def op(inp):
        L = _lib()
        Wf, bf, cd, dims, n = _tables(inp, "f")
        Wsn, bsn, _, _, _ = _tables(inp, "s")
        y0 = inp["y0"]
        B, d = y0.shape
        rec = 32 if srk else 16
        out = torch.empty((SDE_OUT, B, d), dtype=torch.float32, device=y0.device)
        ws = torch.empty(rec * n_steps + slack, dtype=torch.uint8, device=y0.device)
        fn = getattr(L.load(), "cfm_sde_srk_mlp_f32" if srk else "cfm_sde_em_mlp_f32")
        rc = fn(Wf, bf, Wsn, bsn, cd, n, L.ptr(y0), B, _hp(inp["steps"]), n_steps, 0, None, 1234, L.ptr(out), L.ptr(ws), L.stream_ptr())
        return [("traj", out, None)], (rc,)
    return op


case("cfm_sde_em_mlp_f32", note="Philox noise from a fixed seed")(_mk_sde(False), _op_sde(False))
case("cfm_sde_srk_mlp_f32", note="Philox noise from a fixed seed")(_mk_sde(True), _op_sde(True))
case("cfm_sde_em_mlp_f32", "long-640KB", note="a host array of 640 KB")(_mk_sde(False, SDE_LONG), _op_sde(False, SDE_LONG))


# ------------------------------------------------------------------------------------------------ ODE / CNF solves
OD, OW, ONT = 2, 64, 9     # small field: d = 2, w = 64, 9 grid points
TOL = 1e-4


def _mk_ode(B=BS, d=OD, w=OW, n_t=ONT, aug=0, out_dim=None, pair=False, eps=False, reverse=False, salt=18):
    """x0 [B, aug + d] (the augmented columns start at zero in the true set and small values in the decoy), the field's
    weights, the host grid."""
    def make(seed, dev):
        g = _g(seed, salt)
        dims = [d + 1, w, w, w, d if out_dim is None else out_dim]
        inp = _net(g, dims, "")
        if pair:
            inp.update(_net(g, dims, "s"))
        x = _randn(g, B, d)
        inp["x0"] = torch.cat([_randn(g, B, aug) * 0.1 * seed, x], 1) if aug else x
        if eps:
            inp["eps"] = (torch.randint(0, 2, (B, d), generator=g) * 2 - 1).float()
        inp = _to(dev, inp)
        inp["t_span"] = _grid(seed, n_t, reverse)
        return inp
    return make


def _ode_common(inp, aug=0):
    L = _lib()
    Wp, bp, cd, dims, n = _tables(inp)
    x0 = inp["x0"]
    B, D = x0.shape
    ts = inp["t_span"]
    traj = torch.empty((len(ts), B, D), dtype=torch.float32, device=x0.device)
    ws = _ws(L.OP_ODE, B, max(dims[1:n]), D, x0.device)
    return L, Wp, bp, cd, n, x0, B, ts, traj, ws


def _op_fixed(entry, scheme):
    def op(inp):
        L, Wp, bp, cd, n, x0, B, ts, traj, ws = _ode_common(inp)
        nfe = ci(-1)
        fn = getattr(L.load(), entry)
        if entry == "cfm_ode_euler_mlp_f32":
            rc = fn(Wp, bp, cd, n, L.ptr(x0), B, _hp(ts), len(ts), L.ptr(traj), ctypes.byref(nfe), L.ptr(ws), L.stream_ptr())
        else:
            rc = fn(Wp, bp, cd, n, L.ptr(x0), B, _hp(ts), len(ts), scheme, L.ptr(traj), ctypes.byref(nfe), L.ptr(ws), L.stream_ptr())
        return [("traj", traj, None)], (rc, nfe.value)
    return op


def _op_adaptive(entry, tab, tol=TOL):
    def op(inp):
        L, Wp, bp, cd, n, x0, B, ts, traj, ws = _ode_common(inp)
        nfe, steps = ci(-1), ci(-1)
        fn = getattr(L.load(), entry)
        if entry == "cfm_ode_dopri5_mlp_f32":
            rc = fn(Wp, bp, cd, n, L.ptr(x0), B, _hp(ts), len(ts), tol, tol, L.ptr(traj), ctypes.byref(steps), ctypes.byref(nfe),
                    L.ptr(ws), L.stream_ptr())
        else:
            rc = fn(Wp, bp, cd, n, L.ptr(x0), B, _hp(ts), len(ts), tab, tol, tol, L.ptr(traj), ctypes.byref(steps),
                    ctypes.byref(nfe), L.ptr(ws), L.stream_ptr())
        return [("traj", traj, None)], (rc, steps.value, nfe.value)
    return op


def _op_pair(inp):
    L, Wp, bp, cd, n, x0, B, ts, traj, ws = _ode_common(inp)
    Wb, bb, _, _, _ = _tables(inp, "s")
    nfe = ci(-1)
    rc = L.load().cfm_ode_fixed_pair_mlp_f32(Wp, bp, Wb, bb, cd, n, L.ptr(x0), B, _hp(ts), len(ts), 2, L.ptr(traj), ctypes.byref(nfe),
                                             L.ptr(ws), L.stream_ptr())
    return [("traj", traj, None)], (rc, nfe.value)


case("cfm_ode_euler_mlp_f32")(_mk_ode(), _op_fixed("cfm_ode_euler_mlp_f32", 0))
case("cfm_ode_fixed_mlp_f32", "rk4-one-launch")(_mk_ode(), _op_fixed("cfm_ode_fixed_mlp_f32", 2))
case("cfm_ode_fixed_mlp_f32", "midpoint-layers-784x512", note="outside the small-field envelope: the layer driver")(
    _mk_ode(B=24, d=784, w=512, n_t=4), _op_fixed("cfm_ode_fixed_mlp_f32", 1))
case("cfm_ode_fixed_gradmlp_f32", "midpoint-reverse")(_mk_ode(out_dim=1, reverse=True), _op_fixed("cfm_ode_fixed_gradmlp_f32", 1))
case("cfm_ode_fixed_pair_mlp_f32", "rk4")(_mk_ode(pair=True), _op_pair)
case("cfm_ode_dopri5_mlp_f32")(_mk_ode(B=300), _op_adaptive("cfm_ode_dopri5_mlp_f32", 0))
case("cfm_ode_adaptive_mlp_f32", "tsit5")(_mk_ode(B=300, d=5), _op_adaptive("cfm_ode_adaptive_mlp_f32", 1))
case("cfm_ode_adaptive_mlp_f32", "dopri5-layers-784x512", note="the layer driver with its host read-backs")(
    _mk_ode(B=24, d=784, w=512, n_t=3), _op_adaptive("cfm_ode_adaptive_mlp_f32", 0))
case("cfm_ode_adaptive_gradmlp_f32", "tsit5")(_mk_ode(B=300, out_dim=1), _op_adaptive("cfm_ode_adaptive_gradmlp_f32", 1))


def _op_cnf_fixed(entry, mode, scheme):
    def op(inp):
        L, Wp, bp, cd, n, x0, B, ts, traj, ws = _ode_common(inp)
        nfe = ci(-1)
        fn = getattr(L.load(), entry)
        eps = L.ptr(inp.get("eps"))
        if entry == "cfm_ode_euler_cnf_mlp_f32":
            rc = fn(Wp, bp, cd, n, L.ptr(x0), B, _hp(ts), len(ts), mode, eps, L.ptr(traj), ctypes.byref(nfe), L.ptr(ws), L.stream_ptr())
        else:
            rc = fn(Wp, bp, cd, n, L.ptr(x0), B, _hp(ts), len(ts), mode, eps, scheme, L.ptr(traj), ctypes.byref(nfe), L.ptr(ws),
                    L.stream_ptr())
        return [("traj", traj, None)], (rc, nfe.value)
    return op


def _op_cnf_adaptive(entry, mode, tab, tol=TOL):
    def op(inp):
        L, Wp, bp, cd, n, x0, B, ts, traj, ws = _ode_common(inp)
        nfe, steps = ci(-1), ci(-1)
        fn = getattr(L.load(), entry)
        eps = L.ptr(inp.get("eps"))
        if entry == "cfm_ode_dopri5_cnf_mlp_f32":
            rc = fn(Wp, bp, cd, n, L.ptr(x0), B, _hp(ts), len(ts), mode, eps, tol, tol, L.ptr(traj), ctypes.byref(steps),
                    ctypes.byref(nfe), L.ptr(ws), L.stream_ptr())
        else:
            rc = fn(Wp, bp, cd, n, L.ptr(x0), B, _hp(ts), len(ts), mode, eps, tab, tol, tol, L.ptr(traj), ctypes.byref(steps),
                    ctypes.byref(nfe), L.ptr(ws), L.stream_ptr())
        return [("traj", traj, None)], (rc, steps.value, nfe.value)
    return op


case("cfm_ode_euler_cnf_mlp_f32", "exact")(_mk_ode(aug=1), _op_cnf_fixed("cfm_ode_euler_cnf_mlp_f32", 0, 0))
case("cfm_ode_fixed_cnf_mlp_f32", "hutch-rk4")(_mk_ode(aug=1, eps=True), _op_cnf_fixed("cfm_ode_fixed_cnf_mlp_f32", 1, 2))
case("cfm_ode_fixed_cnf_gradmlp_f32", "euler")(_mk_ode(aug=1, out_dim=1), _op_cnf_fixed("cfm_ode_fixed_cnf_gradmlp_f32", 0, 0))
case("cfm_ode_dopri5_cnf_mlp_f32", "exact")(_mk_ode(B=300, aug=1), _op_cnf_adaptive("cfm_ode_dopri5_cnf_mlp_f32", 0, 0))
case("cfm_ode_adaptive_cnf_mlp_f32", "hutch-tsit5")(_mk_ode(B=300, aug=1, eps=True), _op_cnf_adaptive("cfm_ode_adaptive_cnf_mlp_f32", 1, 1))


def _mk_eval(out_dim=None, B=BS, d=OD):
    def make(seed, dev):
        g = _g(seed, 19)
        return _to(dev, {**_net(g, [d + 1, OW, OW, OW, d if out_dim is None else out_dim]), "x": _randn(g, B, d)})
    return make


def _op_divergence(inp):
    L = _lib()
    Wp, bp, cd, dims, n = _tables(inp)
    x = inp["x"]
    B = x.shape[0]
    v, div = torch.empty_like(x), torch.empty(B, dtype=torch.float32, device=x.device)
    rc = L.load().cfm_mlp_divergence_f32(Wp, bp, cd, n, L.ptr(x), B, 0.3, 0, None, L.ptr(v), L.ptr(div), None, L.stream_ptr())
    return [("v", v, None), ("div", div, None)], (rc,)


def _op_grad_field(inp):
    L = _lib()
    Wp, bp, cd, dims, n = _tables(inp)
    x = inp["x"]
    B, d = x.shape
    v, lap = torch.empty_like(x), torch.empty(B, dtype=torch.float32, device=x.device)
    rc = L.load().cfm_mlp_grad_field_f32(Wp, bp, cd, n, L.ptr(x), d, B, 0.3, L.ptr(v), L.ptr(lap), None, L.stream_ptr())
    return [("v", v, None), ("lap", lap, None)], (rc,)


case("cfm_mlp_divergence_f32")(_mk_eval(), _op_divergence)
case("cfm_mlp_grad_field_f32")(_mk_eval(1), _op_grad_field)

REG_MASK = 3               # both penalties: rows [l, e, f, x]


def _op_cnf_reg(inp):
    L, Wp, bp, cd, n, x0, B, ts, traj, ws = _ode_common(inp)
    nfe = ci(-1)
    jsq = torch.empty((max(len(ts) - 1, 1), B), dtype=torch.float32, device=x0.device)
    rc = L.load().cfm_ode_euler_cnf_reg_mlp_f32(Wp, bp, cd, n, L.ptr(x0), B, _hp(ts), len(ts), 0, None, REG_MASK, L.ptr(traj), L.ptr(jsq),
                                                ctypes.byref(nfe), L.ptr(ws), L.stream_ptr())
    return [("traj", traj, None), ("jac_sq", jsq, None)], (rc, nfe.value)


case("cfm_ode_euler_cnf_reg_mlp_f32")(_mk_ode(aug=3), _op_cnf_reg)


# ------------------------------------------------------------------------------------------------ gradients of the solves
def _mk_grad(aug, jac=False, B=BS, d=OD, n_t=ONT):
    """The checkpoints a gradient entry reads are inputs like any other: finite states, not necessarily a solve's."""
    def make(seed, dev):
        g = _g(seed, 20)
        D = aug + d
        inp = {**_net(g, [d + 1, OW, OW, OW, d]), "traj": _randn(g, n_t, B, D),
               "g": _randn(g, n_t, B, D) if aug == 0 else _randn(g, B, D)}
        if jac:
            inp["jac_sq"] = _rand(g, max(n_t - 1, 1), B) + 0.5
        inp = _to(dev, inp)
        inp["t_span"] = _grid(seed, n_t) if n_t > 1 else np.array([0.25 * seed], dtype=np.float32)
        return inp
    return make


def _op_solve_grad(entry):
    def op(inp):
        L = _lib()
        p = L.ptr
        Wp, bp, cd, dims, n = _tables(inp)
        traj, ts = inp["traj"], inp["t_span"]
        dev = traj.device
        ONT, BS = traj.shape[0], traj.shape[1]           # (this case's own n_t and B)
        dW, db = _grads(inp)
        gi = torch.empty_like(traj[0])
        fn = getattr(L.load(), entry)
        if entry == "cfm_ode_fixed_grad_f32":
            ws = _ws(L.OP_ODE_GRAD, BS, ONT, 0, dev)
            rc = fn(Wp, bp, cd, n, p(traj), BS, _hp(ts), ONT, 2, p(inp["g"]), _ptrs(dW), _ptrs(db), p(gi), p(ws), L.stream_ptr())
        elif entry == "cfm_cnf_euler_grad_f32":
            ws = _ws(L.OP_CNF_GRAD, BS, ONT, 0, dev)
            rc = fn(Wp, bp, cd, n, p(traj), BS, _hp(ts), ONT, 0, None, p(inp["g"]), _ptrs(dW), _ptrs(db), p(gi), p(ws), L.stream_ptr())
        else:
            ws = _ws(L.OP_CNF_GRAD, BS, ONT, 0, dev)
            rc = fn(Wp, bp, cd, n, p(traj), BS, _hp(ts), ONT, 0, None, REG_MASK, p(inp["jac_sq"]), p(inp["g"]), _ptrs(dW), _ptrs(db),
                    p(gi), p(ws), L.stream_ptr())
        return _grad_outs(dW, db) + [("g_initial", gi, None)], (rc,)
    return op


case("cfm_ode_fixed_grad_f32", "rk4")(_mk_grad(0), _op_solve_grad("cfm_ode_fixed_grad_f32"))
case("cfm_cnf_euler_grad_f32", "exact")(_mk_grad(1), _op_solve_grad("cfm_cnf_euler_grad_f32"))
case("cfm_cnf_reg_euler_grad_f32", "mask3")(_mk_grad(3, jac=True), _op_solve_grad("cfm_cnf_reg_euler_grad_f32"))

MAX_STEPS = 64             # step log of the recording solve; zero-filled, so a record past a solve's end is {0, 0, 0, out 0}


def _rec_call(inp, log, ysteps, tol=TOL):
    MAX_STEPS = ysteps.shape[0]
    L, Wp, bp, cd, n, x0, B, ts, traj, ws = _ode_common(inp)
    nfe, steps, nacc = ci(-1), ci(-1), ci(-1)
    rc = L.load().cfm_ode_adaptive_rec_mlp_f32(Wp, bp, cd, n, L.ptr(x0), B, _hp(ts), len(ts), 1, tol, tol, L.ptr(traj), ctypes.byref(steps),
                                               ctypes.byref(nfe), MAX_STEPS, L.ptr(log), L.ptr(ysteps), ctypes.byref(nacc), L.ptr(ws),
                                               L.stream_ptr())
    return traj, (rc, steps.value, nfe.value, nacc.value)


def _op_rec(inp, tol=TOL):
    x0 = inp["x0"]
    max_steps = inp.get("_max_steps", MAX_STEPS)
    log = torch.zeros(max_steps * 4, dtype=torch.int32, device=x0.device)
    ysteps = torch.zeros((max_steps,) + tuple(x0.shape), dtype=torch.float32, device=x0.device)
    traj, host = _rec_call(inp, log, ysteps, tol)
    return [("traj", traj, None), ("log", log, None), ("ysteps", ysteps, None)], host


case("cfm_ode_adaptive_rec_mlp_f32", "tsit5")(_mk_ode(B=300), _op_rec)


def _mk_adaptive_grad(seed, dev):
    """The log and step states of a recording solve of this seed's own problem (default stream, synchronised)."""
    inp = _mk_ode(B=300)(seed, dev)
    x0 = inp["x0"]
    log = torch.zeros(MAX_STEPS * 4, dtype=torch.int32, device=dev)
    ysteps = torch.zeros((MAX_STEPS,) + tuple(x0.shape), dtype=torch.float32, device=dev)
    _, host = _rec_call(inp, log, ysteps)
    torch.cuda.synchronize()
    assert host[0] == 0 and 0 < host[3] < MAX_STEPS, host
    g = _g(seed, 21)
    out = {k: v for k, v in inp.items() if k[0] in "Wb"}
    out.update({"log": log, "ysteps": ysteps, "g": _randn(g, ONT, 300, OD).to(dev)})
    # (host argument, the same for both sets: the decoy's log is read over the TRUE count of records; it is zero-filled)
    out["_n_accepted"] = host[3] if seed == 0 else None
    return out


def _op_adaptive_grad(inp):
    L = _lib()
    p = L.ptr
    Wp, bp, cd, dims, n = _tables(inp)
    dev = inp["g"].device
    dW, db = _grads(inp)
    gi = torch.empty((300, OD), dtype=torch.float32, device=dev)
    ws = _ws(L.OP_ODE_GRAD, 300, ONT, 0, dev)
    rc = L.load().cfm_ode_adaptive_grad_f32(Wp, bp, cd, n, p(inp["ysteps"]), p(inp["log"]), inp["_n_accepted"], 300, ONT, 1, 1.0,
                                            p(inp["g"]), _ptrs(dW), _ptrs(db), p(gi), p(ws), L.stream_ptr())
    return _grad_outs(dW, db) + [("g_initial", gi, None)], (rc,)


case("cfm_ode_adaptive_grad_f32", "tsit5", note="n_accepted (a host scalar) is the true solve's in every run")(_mk_adaptive_grad, _op_adaptive_grad)


def _mk_action(seed, dev):
    g = _g(seed, 22)
    return _to(dev, {**_net(g, [OD + 1, OW, OW, OW, 1]), "x0": _randn(g, BS, OD), "x1": _randn(g, BS, OD) + 0.5, "t": _rand(g, BS)})


def _op_action(inp):
    L = _lib()
    p = L.ptr
    Wp, bp, cd, dims, n = _tables(inp)
    dev = inp["t"].device
    dW, db = _grads(inp)
    loss = torch.empty(1, dtype=torch.float32, device=dev)
    ws = _ws(L.OP_ACTION_GRAD, BS, 0, 0, dev)
    rc = L.load().cfm_action_matching_grad_f32(Wp, bp, cd, n, p(inp["x0"]), p(inp["x1"]), None, p(inp["t"]), BS, p(loss), _ptrs(dW),
                                               _ptrs(db), p(ws), L.stream_ptr())
    return _grad_outs(dW, db) + [("loss", loss, None)], (rc,)


case("cfm_action_matching_grad_f32")(_mk_action, _op_action)


def all_cases():
    return [c for cs in CASES.values() for c in cs]
