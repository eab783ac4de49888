"""
The block-wide runs of the f pass's decided path (fpr_locate in fcd_common.h, through the library's host entry points
fcd_f_run_count / fcd_f_run_locate; no GPU): the runs partition the pair-aligned tiles, each lies in one row pair and one block
of 16 columns, and the Philox blocks they draw come to the count made on the CPU.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import f_sure_ref as R  # noqa: E402


@pytest.fixture(scope="module")
def lib():
    from fcdiff_amd import _lib
    return _lib.load()


def runs_of(lib, N):
    out = (C.c_int64 * 9)()
    rows = []
    for t in range(lib.fcd_f_run_count(N)):
        assert lib.fcd_f_run_locate(N, t, out) == 0
        rows.append(tuple(out))
    return rows


def row_ids(n, mb, N):
    return [n * (n - 1) // 2 + m for m in range(mb, min(mb + 16, n))] if n < N else []


@pytest.mark.parametrize("N", range(2, 71))
def test_runs_partition_the_pair_aligned_tiles(lib, N):
    tiles = R.tiles(N)
    runs = runs_of(lib, N)
    seen = []
    for (n0, mb, cnt0, cnt1, tile0, ntile, cr0, cr1, blocks) in runs:
        assert n0 % 2 == 0 and mb % 16 == 0 and 1 <= ntile <= 4
        (ids0, ids1) = (row_ids(n0, mb, N), row_ids(n0 + 1, mb, N))
        assert (cnt0, cnt1) == (len(ids0), len(ids1))
        assert not ids0 or cr0 == ids0[0]
        assert not ids1 or cr1 == ids1[0]
        # its tiles: consecutive, of this row pair, inside this block of 16 columns, and together exactly the run's edges
        ids = []
        for t in range(tile0, tile0 + ntile):
            for c in tiles[t]:
                (n, m) = divmod_edge(int(c))
                assert n in (n0, n0 + 1) and mb <= m < mb + 16
            ids += [int(c) for c in tiles[t]]
        assert sorted(ids) == sorted(ids0 + ids1)
        assert blocks == sum(len({c >> 2 for c in r}) for r in (ids0, ids1))
        seen += list(range(tile0, tile0 + ntile))
    assert seen == list(range(len(tiles)))


def divmod_edge(c):
    n = int((1 + np.sqrt(8.0 * c + 1)) / 2)
    while n * (n - 1) // 2 > c:
        n -= 1
    while (n + 1) * n // 2 <= c:
        n += 1
    return n, c - n * (n - 1) // 2


@pytest.mark.parametrize("N,n_runs,n_blocks", ((200, 676, 5989), (64, 80, 624)))
def test_philox_blocks_per_pass(lib, N, n_runs, n_blocks):
    runs = runs_of(lib, N)
    assert len(runs) == n_runs
    assert sum(r[8] for r in runs) == n_blocks


def test_locate_refuses_what_is_outside(lib):
    out = (C.c_int64 * 9)()
    assert lib.fcd_f_run_locate(64, 80, out) != 0
    assert lib.fcd_f_run_locate(64, -1, out) != 0
    assert lib.fcd_f_run_locate(1, 0, out) != 0
