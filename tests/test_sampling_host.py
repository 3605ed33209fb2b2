"""
The pure parts of the posterior-draw driver (gpim_amd/_sampling.py), no GPU and no device: the one formula for the bytes of
a padded factorisation workspace, the width of z that each method's description plans against what the oracles of the six
methods state, and the library-side memory formula of method='columns' against the integers its earlier home returned.

The width checks use the cases of the oracles' own host tests.  For 'pathwise', 'blocks' and 'border' the oracle states
the width as an assertion on the z it is given: it is handed a z of the description's width and must take it.
"""
import numpy as np
import pytest

import blocks_oracle as BO
import border_sample_oracle as BS
import columns_sample_oracle as CO
import kron_sample_oracle as KO
import pathwise_oracle as PO
import sample_oracle as SO
from columns_oracle import cube
from gpim_amd import _sampling, _solvers
from gpim_amd.gprutils import column_blocks

GRIDS = ((6, 5), (5, 5), (8, 8), (4, 3, 4))             # tests/test_pathwise_host.py, test_blocks_host.py, test_border_sample_host.py
M = _sampling.METHODS


def width(method, g, noiseless):
    W, layout, need, subject = M[method].plan(g, 2, noiseless, False)
    assert isinstance(W, int) and isinstance(layout, str) and isinstance(subject, str) and int(need) > 0
    return W


@pytest.mark.parametrize("n", (1, 127, 128, 129, 1023, 1024, 1025))
def test_factor_bytes(n):
    order = -(-n // 128) * 128
    assert _sampling.factor_bytes(n) == order * (order + (16 if order >= 1024 else 0)) * 8
    # written out once more, by size class: one tile; whole tiles below 1024; padded rows from 1024 on
    assert _sampling.factor_bytes(n) == {1: 128 * 128 * 8, 127: 128 * 128 * 8, 128: 128 * 128 * 8, 129: 256 * 256 * 8,
                                         1023: 1024 * 1040 * 8, 1024: 1024 * 1040 * 8, 1025: 1152 * 1168 * 8}[n]


def test_the_six_methods():
    assert list(M) == ["joint", "pathwise", "blocks", "border", "kron", "columns"]
    assert all(M[name].name == name for name in M)


@pytest.mark.parametrize("N,Mt", sorted({(c[1], c[2]) for c in SO.CASES}))
def test_width_joint(N, Mt):
    for noiseless in (False, True):
        assert width("joint", {"N": N, "M": Mt}, noiseless) == Mt          # z is (S, M): sample_oracle draws mean + L z


@pytest.mark.parametrize("shape", GRIDS, ids=lambda s: "x".join(str(n) for n in s))
def test_width_pathwise_blocks_border(shape):
    P = PO.Params("RBF", 1.3, [2.0, 3.1, 1.7][:len(shape)], 0.02, alpha=1.7, jitter=1e-5)
    blocks = PO.Blocks(PO.full_grid(shape)[0])
    Mg = blocks.M
    idx = np.sort(np.random.default_rng(0).permutation(Mg)[:7]).astype(np.int64)        # test_pathwise_host.make
    y = np.sin(blocks.G.sum(1) / 5.0)
    nq = int(np.prod([(n + 1) // 2 for n in shape]))
    for noiseless in (False, True):
        W = width("pathwise", {"N": len(idx), "M": Mg, "nq": nq}, noiseless)
        assert W == Mg + len(idx) + (0 if noiseless else Mg)
        assert PO.draws(P, blocks, idx, y[idx], np.zeros((1, W)), noiseless)["out"].shape == (1, Mg)
        W = width("blocks", {"N": Mg, "M": Mg, "nq": nq}, noiseless)
        assert W == 2 * Mg + (0 if noiseless else Mg)
        assert BO.draws(P, blocks, y, np.zeros((1, W)), noiseless)["out"].shape == (1, Mg)
        W = width("border", {"M": Mg, "nq": nq}, noiseless)
        assert W == 2 * Mg + (0 if noiseless else Mg)
        miss = BS.missing_sets(shape)["single"]
        assert BS.draws(P, blocks, miss, y, np.zeros((1, W)), noiseless)["out"].shape == (1, Mg)
        with pytest.raises(AssertionError):                                     # (the oracles do refuse another width)
            BO.draws(P, blocks, y, np.zeros((1, W + 1)), noiseless)


@pytest.mark.parametrize("name", sorted(KO.GRIDS))
def test_width_kron(name):
    c, t, _ = KO.GRIDS[name]
    g = M["kron"].sizes(c, t)
    PU, N, Mt = KO.widths(c, t)
    assert (g["PU"], g["N"], g["M"]) == (PU, N, Mt)
    for noiseless in (False, True):
        assert width("kron", g, noiseless) == PU + N + Mt


COLUMN_CASES = [("8x7x5", (8, 7, 5), False), ("8x7x5-finer", (8, 7, 5), True), ("6x5x4x3", (6, 5, 4, 3), False)]


@pytest.mark.parametrize("name,shape,finer", COLUMN_CASES, ids=[c[0] for c in COLUMN_CASES])
def test_width_columns(name, shape, finer):
    """The cases of tests/test_columns_sample_host.py: 40 % of the pixels observed, the cube's own grid or the half-step one."""
    Xg, X, y = cube(shape, (0, 1), 0.6, seed=3)
    C = column_blocks(X, y)
    taxes = [np.arange(0, n - 0.75, 0.5) for n in shape] if finer else [np.arange(n, dtype=np.float64) for n in shape]
    Xt = np.array(np.meshgrid(taxes[0], taxes[1], indexing="ij")).reshape(2, -1).T
    g = M["columns"].sizes(_solvers.Columns(C), taxes)
    Us, U, N, Mt = CO.widths(C["Xs"], C["axes_c"], Xt, taxes[2:])
    assert (g["Us"], g["U"], g["N"], g["M"]) == (Us, U, N, Mt)
    for noiseless in (False, True):
        assert width("columns", g, noiseless) == Us * U + N + Mt


@pytest.mark.parametrize("args,doubles", [
    ((2, 22, 56, 56, 5, [5], [5], [5]), 289552),                    # the 8 x 7 x 5 cube on its own grid, S = 2
    ((3, 12, 120, 132, 4, [7], [4], [7]), 350472),                  # a finer test grid: union axis != training axis
    ((5, 166, 256, 256, 12, [7, 5], [4, 3], [7, 5]), 1415424),      # two block columns, two complete axes
    ((100000, 86, 144, 144, 6, [6], [6], [6]), 33401344),           # more draws than one group holds
])
def test_columns_library_doubles(args, doubles):
    """(S, N_s, M_s, U_s, J, union / training / test orders of the complete axes) -> the integers the function returned as
    reconstructor._columns_library_doubles, before it moved here."""
    assert _sampling._columns_library_doubles(*args) == doubles
