"""GPU: the lean sweep kernel (asg_sweep) against the 16-wave step kernel (asg_step) it relieves — bit for bit.

1. ONE sweep step per mode through cfm_assign_debug_sweep, with cfm_assign_set_sweep at 0 and at 1, on the same state:
   every array a sweep writes (bidval, key, p), the cost range, the mode the control step leaves and the certificate's
   verdict / minimum slack are compared bitwise; the certificate's total cost (an atomic sum in both kernels) within
   1e-12 relative.  The hook fills the workspace with all-ones bytes first, so an element the other grid skips shows.
   Sizes: 512 (smallest size of the chip-wide machine, two column groups of the 64-column INITRED form), 768, 1000 (no
   multiple of 64: ragged last pieces of a row), 1002 (no multiple of 4: the scalar paths), 3072 (smallest size of the 16-byte INITRED form), 4096.  Matrices: seeded random costs,
   and one with duplicated rows and a constant column (ties; a column of zero cost range).
2. Whole solves, lone and in batches of 3 and 4, with the switch at 0 and at 1: same permutations, certified, same cost,
   no dense fallback, and the launches the driver's program predicts for each form.
"""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

UMIN0, INITRED, UMIN, COLRED, ROOTMIN, CERT = 0, 1, 5, 6, 7, 10
DEFAULT_SWEEP = -1         # cfm_assign_set_sweep(< 0): the library's own defaults again, restored behind every test


@pytest.fixture(scope="module")
def dev():
    from cfm_amd import _lib
    return _lib.require_gpu()


@pytest.fixture()
def lib():
    from cfm_amd import _lib
    l = _lib.load()
    yield l
    l.cfm_assign_set_sweep(DEFAULT_SWEEP)


_cache = {}


def _matrix(n, kind):
    """host fp32 matrix; "tied": every odd row repeats the row above it, column 5 is constant"""
    if (n, kind) not in _cache:
        g = torch.Generator().manual_seed(1000 + n)
        M = torch.rand(n, n, generator=g) * 4.0
        if kind == "tied":
            M[1::2] = M[0::2]
            M[:, 5] = 0.25
        _cache[(n, kind)] = M.contiguous()
    return _cache[(n, kind)]


def _vp(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def _step(lib, mode, Md, n, ws, blocks=0, p=None, u=None, lst=None, perm=None):
    out = {"bidval": np.zeros(n, np.float64), "key": np.zeros(n, np.uint64), "p": np.zeros(n, np.float64),
           "state": np.zeros(8, np.int32), "cost": np.zeros(1, np.float64)}
    rc = lib.cfm_assign_debug_sweep(mode, ctypes.c_void_p(Md.data_ptr()), n, blocks, _vp(p), _vp(u), _vp(lst),
                                    0 if lst is None else len(lst), _vp(perm), _vp(out["bidval"]), _vp(out["key"]),
                                    _vp(out["p"]), _vp(out["state"]), _vp(out["cost"]), ctypes.c_void_p(ws.data_ptr()), None)
    assert rc == 0, (mode, n, rc)
    return out


def _both(lib, mode, Md, n, ws, what, **kw):
    got = []
    for sw in (0, 1):
        lib.cfm_assign_set_sweep(sw)
        got.append(_step(lib, mode, Md, n, ws, **kw))
    a, b = got
    for name in ("bidval", "key", "p"):
        x, y = a[name].view(np.uint64), b[name].view(np.uint64)
        bad = np.nonzero(x != y)[0]
        assert bad.size == 0, (what, name, bad[:8].tolist(), a[name][bad[:4]].tolist(), b[name][bad[:4]].tolist())
    assert a["state"].tolist() == b["state"].tolist(), (what, a["state"].tolist(), b["state"].tolist())
    assert a["state"][6] == 1, (what, "one control step per launch", a["state"].tolist())
    ca, cb = float(a["cost"][0]), float(b["cost"][0])
    assert abs(ca - cb) <= 1e-12 * max(abs(ca), abs(cb)), (what, ca, cb)
    return a


@pytest.mark.parametrize("kind", ["random", "tied"])
@pytest.mark.parametrize("n", [512, 768, 1000, 1002, 3072, 4096])
def test_sweeps_bit_for_bit(dev, lib, n, kind):
    from cfm_amd import _lib
    Mh = _matrix(n, kind)
    Md = Mh.to(dev)
    ws = _lib.workspace(_lib.OP_ASSIGN, n, n, 0, dev)
    M64 = Mh.numpy().astype(np.float64)
    rng = np.random.default_rng(n)
    ones = np.uint64(0xFFFFFFFFFFFFFFFF)
    for blocks in ((0, 16) if n in (1000, 4096) else (0,)):      # the grid of a lone solve; of a batch of four
        tag = f"n={n} {kind} blocks={blocks}"
        # UMIN0: row minima, cost range, key reset
        r = _both(lib, UMIN0, Md, n, ws, tag + " UMIN0", blocks=blocks)
        assert np.array_equal(r["bidval"], M64.min(axis=1)), tag
        assert not np.any(r["key"]), (tag, "a key was not reset")
        assert r["state"][2] == INITRED
        u0 = r["bidval"].copy()
        # INITRED: p_j = max_i (u_i - c_ij) into the keys
        r = _both(lib, INITRED, Md, n, ws, tag + " INITRED", blocks=blocks, u=u0)
        assert np.all(r["key"] != 0) and np.all(r["key"] != ones), (tag, "a column got no initial price")
        # UMIN on arbitrary prices
        p = -rng.random(n) * 0.5
        r = _both(lib, UMIN, Md, n, ws, tag + " UMIN", blocks=blocks, p=p)
        assert np.array_equal(r["bidval"], (M64 + p[None, :]).min(axis=1)), tag
        assert r["state"][2] == COLRED
        u = r["bidval"].copy()
        # COLRED with few, some and nearly all columns free
        for nfc in (1, 63, n - 1):
            lst = rng.permutation(n)[:nfc].astype(np.int32)
            r = _both(lib, COLRED, Md, n, ws, f"{tag} COLRED {nfc}", blocks=blocks, p=p, u=u, lst=lst)
            want = p.copy()
            want[lst] = np.minimum(p[lst], (u[:, None] - M64[:, lst]).max(axis=0))
            assert np.array_equal(r["p"], want), (tag, nfc)
        # ROOTMIN: the free rows' minima
        lst = rng.permutation(n)[:63].astype(np.int32)
        _both(lib, ROOTMIN, Md, n, ws, tag + " ROOTMIN", blocks=blocks, p=p, lst=lst)
        # CERT: a matching that fails the certificate with these duals ...
        perm = rng.permutation(n).astype(np.int32)
        r = _both(lib, CERT, Md, n, ws, tag + " CERT", blocks=blocks, p=p, perm=perm)
        assert r["state"][3] == 0 and r["state"][2] == 13
        assert abs(r["cost"][0] - M64[np.arange(n), perm].sum()) <= 1e-12 * abs(r["cost"][0])
        # ... and one that passes: the matched entry is every row's strict minimum, zero duals
        M2 = Mh.clone()
        M2[torch.arange(n), torch.from_numpy(perm.astype(np.int64))] = Mh.min(dim=1).values - 1.0
        r = _both(lib, CERT, M2.to(dev), n, ws, tag + " CERT ok", blocks=blocks, p=np.zeros(n), perm=perm)
        assert r["state"][3] == 1, (tag, r["state"].tolist())
        # ... and a broken matching (a column used twice)
        perm2 = perm.copy(); perm2[1] = perm2[0]
        r = _both(lib, CERT, Md, n, ws, tag + " CERT bad", blocks=blocks, p=p, perm=perm2)
        assert r["state"][3] == 0


def _record(lib):
    rec = (ctypes.c_int * 8)()
    assert lib.cfm_assign_debug_sweep(-1, None, 0, 0, None, None, None, 0, None, None, None, None, rec, None, None, None) == 0
    return list(rec)


def _fallbacks(lib):
    fb = (ctypes.c_int * 2)(); lib.cfm_assign_debug_fallback(fb)
    return int(fb[0])


@pytest.mark.parametrize("nb", [1, 3, 4])
@pytest.mark.parametrize("n", [512, 1000, 4096])
def test_whole_solves(dev, lib, n, nb):
    import cfm_amd.optimal_transport as ot
    g = torch.Generator().manual_seed(7 * n + nb)
    x0 = torch.randn(nb, n, 16, generator=g)
    x1 = torch.randn(nb, n, 16, generator=g) * 0.5 + 0.3
    Ms = [ot.cost_matrix(x0[b].to(dev), x1[b].to(dev)) for b in range(nb)]
    fb0 = _fallbacks(lib)
    res = []
    for sw in (0, 1):
        lib.cfm_assign_set_sweep(sw)
        if nb == 1:
            perm, info = ot.assign_exact(Ms[0], return_info=True)
            perm, info = perm[None], [info]
        else:
            perm, info = ot.assign_exact_batch(Ms, return_info=True)
        torch.cuda.synchronize()
        rec = _record(lib)
        print(f"n={n} nb={nb} sweep={sw}: launch record {rec}")
        # the launches the driver's program predicts for this form: the whole solve as the unpolled head —
        # 8 asg_step launches, or 1 + 5 asg_sweep — and polled chunks of asg_step launches behind it when a problem left the road
        launches, steps, sweeps, chunks, head, chunk, form, _ = rec
        assert form == sw
        assert head == (9 if sw else 11), rec
        assert launches == head + chunks * chunk, rec
        assert sweeps == (5 if sw else 0), rec
        assert steps == (1 if sw else 8) + chunks * (chunk - 3), rec      # (a chunk: the auction, its steps, the list pair, 2 steps)
        assert all(i["certified"] for i in info)
        res.append((perm.cpu(), [i["total_cost"] for i in info]))
    assert _fallbacks(lib) == fb0, "a solve was redone by the dense machine"
    assert torch.equal(res[0][0], res[1][0])
    for b in range(nb):
        assert sorted(res[0][0][b].tolist()) == list(range(n))
        ca, cb = res[0][1][b], res[1][1][b]
        assert abs(ca - cb) <= 1e-12 * abs(ca), (b, ca, cb)
