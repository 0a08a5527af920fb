"""Every kernel instantiation of libqle_budget.so (csrc/Makefile, SIDE_OPEN) as a test case, in the shape of tests/side_variant_table.py:
the library is outside the closed census of the eleven side libraries, so its rows live here until they are folded into that table.
tests/test_budget_cpu.py holds the table to the built library and every row's inputs to the conditions below; tests/test_gpu_budget.py
runs every row on the device inside the library's own launch census.

The rows restate the dispatch ladder of budget_capi.hip: k_budget<T, PFP, COMPACT> by the handle's dtype, per-filter parameters and
compact records, and k_budget_reduce behind every call -- nine kernels.  Each row: id, library, call, dtype, record (full15 / full9 /
compact9), pfp, kernels (the exact set the call launches) and reference.

Inputs (class Inputs, numpy only, the same on every machine): side_variant_table's consistency inputs -- consistency_util.make_case on
B = 165 filters, two full tiles and a ragged one of 37, a mask with the first tile on and mixed bits elsewhere, one all-zero record --
and one filter, on, with a NaN covariance word.  What keeps a row from hiding a failure (conditions(row), on the reference alone): at
least half of the filters are counted, every tile holds at least two counted filters, and all three status values occur.

The reference of the sums is exact (words_ref, tile_sum, group_sums): the 256 words of every filter formed in numpy from images of the
device words, the xor-butterfly of wave_sum per tile, the tiles from left to right from +0.0 per group.  No tolerance is involved.
"""
import itertools

import numpy as np

import side_variant_table as st

LIBRARY = "budget"
WORDS = 256
B = st.B
NAN_FILTER = 140               # a lane of the ragged tile, on, with a NaN covariance word inside the pose block
NAN_WORD = (2, 5)
OFF, COUNTED, NONFINITE = 0, 1, 2


def k_budget(T, pfp, record):
    return (LIBRARY, f"k_budget<{st.T_NAMES[T]}, {st.b(pfp)}, {st.b(st.RECORDS[record][1])}>")


def build_rows():
    rows = []
    for T, record, F in itertools.product(st.DTYPES, st.RECORDS, st.BOOLS):
        rows.append(dict(id=f"DeviceIO.budget-{T}-{record}" + ("-pfp" if F else ""), library=LIBRARY, call="DeviceIO.budget", dtype=T, record=record,
                         direct=True, pfp=F, kernels=frozenset({k_budget(T, F, record), (LIBRARY, "k_budget_reduce")}),
                         reference="exact: tile_sum of the 256 words, the tiles from left to right"))
    return rows


ROWS = build_rows()
assert len({r["id"] for r in ROWS}) == len(ROWS), "row ids must be unique"


def covered_kernels():
    return {k for r in ROWS for _, k in r["kernels"]}


def tri(i, j):
    return 15 * i - i * (i - 1) // 2 + (j - i)


TRI = [(i, j) for i in range(15) for j in range(i, 15)]
assert [tri(i, j) for i, j in TRI] == list(range(120))


class Inputs(st.Inputs):
    """side_variant_table's consistency inputs (x, P, xt, mask, pfp, ab, wb) with the NaN filter added, and what the kernel must decide:
    status [B]."""

    def __init__(self, row):
        super().__init__(dict(row, library="consistency"))
        i, (a, b) = NAN_FILTER, NAN_WORD
        assert i != self.ZERO and self.x[i, 6:10].any()
        self.P[i, a, b] = self.P[i, b, a] = np.nan
        self.mask[i] = 1
        self.on = (self.mask != 0) & self.x[:, 6:10].any(axis=1)
        self.status = np.where(self.on, COUNTED, OFF).astype(np.uint8)
        self.status[i] = NONFINITE


def conditions(row):
    """Asserts, on the reference alone, that the row cannot hide a failure (the module docstring); -> the Inputs."""
    d = Inputs(row)
    counted = d.status == COUNTED
    assert d.B == B and counted.sum() * 2 >= B, (row["id"], int(counted.sum()))
    per_tile = [int(counted[t:t + 64].sum()) for t in range(0, B, 64)]
    assert len(per_tile) == 3 and min(per_tile) >= 2, (row["id"], per_tile)
    assert set(np.unique(d.status)) == {OFF, COUNTED, NONFINITE}, row["id"]
    assert d.mask[:64].all() and 0 < d.mask[64:].sum() < B - 64
    assert not d.x[d.ZERO].any() and d.status[d.ZERO] == OFF and d.mask[NAN_FILTER] and d.status[NAN_FILTER] == NONFINITE
    assert np.isfinite(d.P[counted]).all() and np.isfinite(d.x[counted]).all() and np.isfinite(d.xt).all()
    return d


# ------------------------------------------------------------------------------------------------ the exact reference
def words_ref(err, status, P):
    """The 256 float64 words of every filter [B,256] from err [B,n] and P [B,n,n] (float64 images of the device words) and status [B]:
    1, e_k, e_i e_j (one rounding: the product of two doubles), P_ij in the row-major upper triangle; zeros where status != 1 and in
    the components a handle with n = 9 does not have."""
    nB, n = err.shape
    e = np.zeros((nB, 15)); e[:, :n] = err
    P15 = np.zeros((nB, 15, 15)); P15[:, :n, :n] = P
    w = np.zeros((nB, WORDS))
    w[:, 0] = 1.0
    w[:, 1:16] = e
    for t, (i, j) in enumerate(TRI):
        w[:, 16 + t] = e[:, i] * e[:, j]
        w[:, 136 + t] = P15[:, i, j]
    w[status != COUNTED] = 0.0
    return w


def tile_sum(w):
    """w [64,256] float64, lanes beyond the end 0.0 -> [256]: the xor-butterfly of wave_sum (csrc/ekf_layout.hpp), by definition the
    tile's field"""
    for o in (32, 16, 8, 4, 2, 1):
        w = w + w[np.arange(64) ^ o]
    return w[0]


def tile_partials(words):
    """[B,256] -> [tiles,256]"""
    nB = words.shape[0]
    tiles = -(-nB // 64)
    pad = np.zeros((tiles * 64, WORDS)); pad[:nB] = words
    return np.stack([tile_sum(pad[64 * t:64 * t + 64]) for t in range(tiles)])


def group_sums(partials, group_tiles):
    """[tiles,256] -> [groups,256]: each group's tiles added from left to right, from +0.0; group_tiles None / 0: one group"""
    tiles = partials.shape[0]
    gt = tiles if not group_tiles else int(group_tiles)
    out = []
    for t0 in range(0, tiles, gt):
        acc = np.zeros(WORDS)
        for t in range(t0, min(t0 + gt, tiles)):
            acc = acc + partials[t]
        out.append(acc)
    return np.stack(out)


def same_bits(a, b, what):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape, (what, a.dtype, b.dtype, a.shape, b.shape)
    u = {1: np.uint8, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize]
    same = a.view(u) == b.view(u)
    assert same.all(), f"{what}: {int((~same).sum())} of {same.size} words differ, first at {np.argwhere(~same)[0]}"
