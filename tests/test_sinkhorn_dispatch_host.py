"""CPU: the shape arithmetic of the two Sinkhorn entry points (cfm_sinkhorn_dispatch_info /
cfm_sinkhorn_points_dispatch_info: the helpers the entry points themselves call, no GPU call) — the row strips of the
column pass, the workspace carving and the kernel selection at its thresholds."""
import ctypes

import pytest

OP_SINKHORN = 1
FIELDS = ("vec", "row_fast", "v_in_lds", "nchunk", "rows_per_chunk", "rows_per_wg", "row_wgs", "stream_nf4",
          "stream_want", "lds_bytes", "off_u", "off_v0", "off_v1", "off_pm", "off_ps", "off_end")
PTS_FIELDS = ("stage_cap", "col_grid", "row_grid", "trip_u", "pre", "lds_bytes", "chunks_x0", "chunks_x1")


def _info(lib, B0, B1, aligned=1):
    out = (ctypes.c_longlong * 16)()
    assert lib.cfm_sinkhorn_dispatch_info(B0, B1, aligned, out) == 0
    return dict(zip(FIELDS, out))


def _pts_info(lib, B0, B1, d):
    out = (ctypes.c_longlong * 8)()
    assert lib.cfm_sinkhorn_points_dispatch_info(B0, B1, d, out) == 0
    return dict(zip(PTS_FIELDS, out))


@pytest.mark.parametrize("B1", [64, 1024, 4096, 16384])
def test_strips_cover_the_rows_and_the_workspace_fits(lib_built, B1):
    lib = lib_built.load()
    first_empty = None
    for B0 in range(1, 4201):
        s = _info(lib, B0, B1)
        n, rpc = s["nchunk"], s["rows_per_chunk"]
        assert 1 <= n <= 64
        # strips [c * rpc, min(B0, (c + 1) * rpc)): together exactly [0, B0) ...
        assert n * rpc >= B0 and rpc >= 1
        sizes = [max(0, min(B0, (c + 1) * rpc) - c * rpc) for c in range(n)]
        assert sum(sizes) == B0
        # ... and only trailing strips are empty
        seen_empty = False
        for sz in sizes:
            if sz == 0:
                seen_empty = True
            else:
                assert not seen_empty, (B0, B1, sizes)
        if seen_empty and first_empty is None:
            first_empty = B0
        # the carved workspace: state block, u, v[0], v[1], the two strip-partial arrays, in this order, inside the
        # size the ABI reports
        assert s["off_u"] == 256 and s["off_v0"] == 256 + 8 * B0 and s["off_v1"] == s["off_v0"] + 8 * B1
        assert s["off_pm"] == s["off_v1"] + 8 * B1 and s["off_ps"] == s["off_pm"] + 8 * n * B1
        assert s["off_end"] == s["off_ps"] + 8 * n * B1
        assert s["off_end"] <= lib.cfm_workspace_bytes(OP_SINKHORN, B0, B1, 0)
    if B1 <= 4096:
        assert first_empty == 2049       # 64 strips of 33 rows: the last one starts behind the matrix
    else:
        assert first_empty is None       # 16 strips at most, of 32 rows or more from B0 = 512 on: 15 of them never cover B0


def test_row_pass_selection_thresholds(lib_built):
    lib = lib_built.load()
    # streaming row pass: B1 % 1024 == 0, B1 <= 16384, aligned matrix
    for B1 in (1024, 3072, 16384):
        s = _info(lib, 67, B1)
        assert (s["vec"], s["row_fast"], s["v_in_lds"], s["stream_nf4"], s["stream_want"]) == (1, 1, 1, 4, 9)
        assert s["lds_bytes"] == 8 * B1 and s["rows_per_wg"] == 4 and s["row_wgs"] == 17
        m = _info(lib, 67, B1, aligned=0)     # the same shape off the 16-byte grid: generic, scalar loads
        assert (m["vec"], m["row_fast"], m["v_in_lds"], m["stream_nf4"], m["stream_want"]) == (0, 0, 1, 0, 0)
        assert m["rows_per_wg"] == 8 and m["row_wgs"] == 9
    # with 4 float4 per lane and unit the loop can only pick 4: the wider instantiations are unreachable
    assert {_info(lib, 8, 1024 * k)["stream_nf4"] for k in range(1, 17)} == {4}
    s = _info(lib, 9, 17408)                  # a multiple of 1024 that does not fit LDS
    assert (s["vec"], s["row_fast"], s["v_in_lds"], s["lds_bytes"]) == (1, 0, 0, 0)
    for B1, vec, lds in ((16380, 1, 1), (16384, 1, 1), (16385, 0, 0), (16388, 1, 0), (16390, 0, 0), (1027, 0, 1),
                         (1028, 1, 1), (6140, 1, 1), (6148, 1, 1), (1, 0, 1)):
        s = _info(lib, 12, B1)
        assert (s["vec"], s["v_in_lds"]) == (vec, lds), B1
        assert s["row_fast"] == (1 if B1 == 16384 else 0)
    assert _info(lib, 10, 6140)["lds_bytes"] <= 48 * 1024 < _info(lib, 10, 6148)["lds_bytes"]
    assert _info(lib, 2055, 1024)["stream_want"] == 257      # more than the 256 CUs of the chip: the grid is capped
    assert lib.cfm_sinkhorn_dispatch_info(0, 4, 1, (ctypes.c_longlong * 16)()) != 0
    assert lib.cfm_sinkhorn_dispatch_info(4, 4, 1, None) != 0


def test_points_staging_capacity(lib_built):
    lib = lib_built.load()
    for d, cap in ((1, 10752), (2, 8192), (3, 6144), (4, 5120), (5, 4608), (6, 4096), (7, 3584), (8, 3072)):
        s = _pts_info(lib, 20000, 20, d)
        assert s["stage_cap"] == cap == (128 * 1024 // (8 + 4 * d)) // 512 * 512
        assert s["lds_bytes"] == cap * (8 + 4 * d) <= 128 * 1024
        assert (s["trip_u"], s["pre"]) == ((8, 4) if d <= 5 else (4, 2))
        assert s["chunks_x0"] == -(-20000 // cap) and s["chunks_x1"] == 1
        assert (s["col_grid"], s["row_grid"]) == (2, 1250)
        # the second chunk starts one point behind the capacity
        assert _pts_info(lib, 20, cap, d)["chunks_x1"] == 1 and _pts_info(lib, 20, cap + 1, d)["chunks_x1"] == 2
    # small clouds: the staged chunk is the larger cloud rounded up to whole trips of 512 points
    assert _pts_info(lib, 130, 77, 4)["stage_cap"] == 512 and _pts_info(lib, 513, 77, 4)["stage_cap"] == 1024
    for bad in ((0, 4, 2), (4, 4, 0), (4, 4, 9)):
        assert lib.cfm_sinkhorn_points_dispatch_info(*bad, (ctypes.c_longlong * 8)()) != 0
