"""The host side of the MFMA tile engine (gemm.hip, gemm_kernel.hpp; it carries every O(N^3) stage that replaces
torch.linalg.cholesky and the solves at gpim/gpreg/gpr.py:192-193,248): the two index maps the kernels evaluate per
workgroup and the choice of the workgroup shape, called on the CPU through the diagnostic exports of gpimhip.h.  The maps
are the very functions the kernels inline (common.hpp: gemm_tile_pos, gemm_rect_tile, __host__ __device__; the float
kernels expand a text of their own, GEMM_TILE_POS_T, which the export with fp32 = 1 runs), so a tile that a launch would
drop, compute twice or look up past the end of its list shows up here without a GPU.

An out-of-range READ of the engine can only come from (a) a list position outside [0, ntiles) -- the bijection tests
below -- or (b) a block index the list itself names, which is the caller's; the k-range arithmetic is covered on the GPU
with NaN-poisoned operands (tests/test_gpu_gemm.py)."""
import ctypes

import numpy as np
import pytest

I32P = ctypes.POINTER(ctypes.c_int32)
NT, NN, TN = (0, 0), (0, 1), (1, 1)
STORE, COLSUMSQ = 0, 1

# The table of the dispatch (gemm.hip: gemm_shape_f64, gemm_kernel.hpp: gemm_shape_generic), per element type: the store
# epilogue runs quadrants (row halves when `inplace`) up to `small` tiles, 8 waves with a CU per tile up to `mid`, beyond
# that 8 waves for NT and 4 waves for NN / TN; the column-sum epilogue runs 8 waves up to `col` tiles, else 4 waves.
# tests/test_gpu_gemm.py reaches its shapes through this table too.
TABLE = {0: dict(small=640, mid=1100, col=256), 1: dict(small=256, mid=2048, col=256)}


def expected_shape(fp32, layout, epi, ntiles, batch, shape_div=0, inplace=0):
    from gpim_amd import _lib
    t = TABLE[fp32]
    if fp32:
        total = ntiles if epi == COLSUMSQ else ntiles * batch       # (the float engine has no shape_div)
    else:
        total = ntiles * batch // (shape_div if shape_div > 1 else 1)
    if epi == COLSUMSQ:
        name = "8w" if total <= t["col"] else "4w"
    elif total <= t["small"]:
        name = "rowhalf" if inplace else "quad"
    elif total <= t["mid"]:
        name = "8w_lds"
    else:
        name = "8w" if layout == NT else "4w"
    return _lib.GEMM_SHAPES[name]


@pytest.fixture(scope="module")
def lib(ensure_built):
    from gpim_amd import _lib
    return _lib.load()


def tile_pos(lib, fp32, n, chunk, quads):
    p = np.empty(n * quads, dtype=np.int32)
    q = np.empty(n * quads, dtype=np.int32)
    assert lib.gpimhip_gemm_tile_pos_host(fp32, n, chunk, quads, 0, n * quads, p.ctypes.data_as(I32P), q.ctypes.data_as(I32P)) == 0
    return p, q


# fp32 = 1: the copy of the map that the single-precision kernels compile (gemm_kernel.hpp: GEMM_TILE_POS_T)
@pytest.mark.parametrize("fp32", [0, 1])
@pytest.mark.parametrize("chunk", [0, 1, 3, 8, 64])
def test_tile_remap_is_a_bijection(lib, chunk, fp32):
    """One workgroup per tile: b -> p permutes [0, n) for every n, whatever n % (8 chunk) is."""
    for n in range(1, 4101):
        p, q = tile_pos(lib, fp32, n, chunk, 1)
        assert p.min() >= 0 and p.max() < n, (n, chunk)
        assert (np.bincount(p, minlength=n) == 1).all(), (n, chunk)
        assert not q.any()


@pytest.mark.parametrize("chunk", [0, 1, 3, 8, 64])
def test_tile_remap_same_in_both_engines(lib, chunk):
    for n in (1, 7, 8, 9, 63, 64, 65, 515, 1024, 4100):
        for quads in (1, 2, 4):
            a, b = tile_pos(lib, 0, n, chunk, quads), tile_pos(lib, 1, n, chunk, quads)
            assert (a[0] == b[0]).all() and (a[1] == b[1]).all()


@pytest.mark.parametrize("fp32", [0, 1])
@pytest.mark.parametrize("quads", [2, 4])
def test_tile_remap_split_tiles(lib, quads, fp32):
    """Several workgroups per tile (row halves, quadrants): bx -> (p, quad) covers [0, n) x [0, quads) once.  The map
    of these shapes does not look at chunk and is linear in bx: every n up to 130 and the largest n of the test above."""
    for chunk in (0, 1, 3, 8, 64):
        for n in list(range(1, 131)) + [4100]:
            p, q = tile_pos(lib, fp32, n, chunk, quads)
            assert p.min() >= 0 and p.max() < n and q.min() >= 0 and q.max() < quads
            assert (np.bincount(p * quads + q, minlength=n * quads) == 1).all(), (n, chunk, quads)


def test_tile_remap_keeps_chunks_together(lib):
    """chunk > 0: inside the full rounds, XCD x (= b % 8) walks whole chunks of consecutive list positions."""
    for n, c in ((8 * 8 * 3 + 5, 8), (64 * 8 * 2 + 100, 64), (3 * 8 * 4 + 2, 3)):
        p, _ = tile_pos(lib, 0, n, c, 1)
        full = n // (8 * c) * (8 * c)
        for x in range(8):
            mine = p[x:full:8]                       # in the order XCD x runs them
            blocks = mine.reshape(-1, c)
            assert (np.diff(blocks, axis=1) == 1).all() and (blocks[:, 0] % c == 0).all()
        assert (p[full:] == np.arange(full, n)).all()


def test_tile_pos_rejects_out_of_range(lib):
    buf = np.zeros(8, dtype=np.int32).ctypes.data_as(I32P)
    for fp32 in (0, 1):
        assert lib.gpimhip_gemm_tile_pos_host(fp32, 4, 0, 1, 0, 5, buf, buf) == -1
        assert lib.gpimhip_gemm_tile_pos_host(fp32, 4, 0, 3, 0, 4, buf, buf) == -1
        assert lib.gpimhip_gemm_tile_pos_host(fp32, 0, 0, 1, 0, 0, buf, buf) == -1
    assert lib.gpimhip_gemm_rect_tile_host(2, 2, 0, 5, buf, buf) == -1
    assert lib.gpimhip_gemm_rect_tile_host(0, 2, 0, 0, buf, buf) == -1


@pytest.mark.parametrize("rows", [1, 7, 8, 9, 13, 16, 17])
@pytest.mark.parametrize("cols", [1, 2, 5])
def test_rect_map_is_a_bijection(lib, rows, cols):
    n = rows * cols
    ci = np.empty(n, dtype=np.int32)
    cj = np.empty(n, dtype=np.int32)
    assert lib.gpimhip_gemm_rect_tile_host(rows, cols, 0, n, ci.ctypes.data_as(I32P), cj.ctypes.data_as(I32P)) == 0
    assert ci.min() >= 0 and ci.max() < rows and cj.min() >= 0 and cj.max() < cols
    assert (np.bincount(ci * cols + cj, minlength=n) == 1).all()
    # strips of eight rows, one after the other; inside a strip column by column
    strip = ci // 8
    assert (np.diff(strip) >= 0).all()
    for s in range((rows + 7) // 8):
        sel = strip == s
        h = min(8, rows - 8 * s)
        assert (cj[sel] == np.repeat(np.arange(cols), h)).all()
        assert (ci[sel] == 8 * s + np.tile(np.arange(h), cols)).all()


@pytest.mark.parametrize("rows,cols", [(8, 8), (16, 8), (16, 16), (24, 40)])
def test_rect_map_patches(lib, rows, cols):
    """rect_rows % 8 == 0: every 8 x 8 patch of tiles is 64 consecutive positions (with chunk = 64: one patch per XCD at
    a time)."""
    n = rows * cols
    ci = np.empty(n, dtype=np.int32)
    cj = np.empty(n, dtype=np.int32)
    assert lib.gpimhip_gemm_rect_tile_host(rows, cols, 0, n, ci.ctypes.data_as(I32P), cj.ctypes.data_as(I32P)) == 0
    assert (np.bincount(ci * cols + cj, minlength=n) == 1).all()
    for p0 in range(0, n, 64):
        a, b = ci[p0:p0 + 64], cj[p0:p0 + 64]
        assert a.max() - a.min() == 7 and a.min() % 8 == 0 and b.max() - b.min() == 7 and b.min() % 8 == 0
        assert len(set(zip(a.tolist(), b.tolist()))) == 64


def _splits(total):
    """(ntiles, batch) pairs with ntiles * batch == total"""
    return [(total // b, b) for b in (1, 2, 3, 5, 7, 10) if total % b == 0]


@pytest.mark.parametrize("fp32", [0, 1])
def test_shape_function_follows_the_table(lib, fp32):
    from gpim_amd import _lib
    t = TABLE[fp32]
    seen = set()
    edges = sorted({1, t["col"], t["col"] + 1, t["small"], t["small"] + 1, t["mid"], t["mid"] + 1, 5000})
    for total in edges:
        for ntiles, batch in _splits(total):
            for layout in (NT, NN, TN):
                for inplace in (0, 1):
                    got = lib.gpimhip_gemm_shape_host(fp32, layout[0], layout[1], STORE, ntiles, batch, 0, inplace)
                    assert got == expected_shape(fp32, layout, STORE, ntiles, batch, 0, inplace), (total, ntiles, batch, layout, inplace)
                    seen.add((STORE, got))
            got = lib.gpimhip_gemm_shape_host(fp32, 0, 1, COLSUMSQ, ntiles, batch, 0, 0)
            assert got == expected_shape(fp32, NN, COLSUMSQ, ntiles, batch), (total, ntiles, batch)
            seen.add((COLSUMSQ, got))
    S = _lib.GEMM_SHAPES
    assert seen == {(STORE, S["quad"]), (STORE, S["rowhalf"]), (STORE, S["8w_lds"]), (STORE, S["8w"]), (STORE, S["4w"]),
                    (COLSUMSQ, S["8w"]), (COLSUMSQ, S["4w"])}
    # `inplace` only matters while the launch is small
    assert lib.gpimhip_gemm_shape_host(fp32, 0, 0, STORE, t["small"] + 1, 1, 0, 1) == S["8w_lds"]


def test_shape_colsumsq_counts_per_type(lib):
    """The column-sum epilogue of the float engine takes its shape from ONE problem's tiles (a problem of a batch keeps the
    bits of its stand-alone run); the double engine counts the batch, unless shape_div takes it out again."""
    from gpim_amd import _lib
    S = _lib.GEMM_SHAPES
    assert lib.gpimhip_gemm_shape_host(1, 0, 1, COLSUMSQ, 72, 4, 0, 0) == S["8w"]
    assert lib.gpimhip_gemm_shape_host(1, 0, 1, COLSUMSQ, 257, 1, 0, 0) == S["4w"]
    assert lib.gpimhip_gemm_shape_host(0, 0, 1, COLSUMSQ, 72, 4, 0, 0) == S["4w"]
    assert lib.gpimhip_gemm_shape_host(0, 0, 1, COLSUMSQ, 72, 4, 4, 0) == S["8w"]
    assert lib.gpimhip_gemm_shape_host(0, 0, 1, COLSUMSQ, 72, 3, 0, 0) == S["8w"]


def test_shape_div(lib):
    """Double engine: ntiles * batch / shape_div decides (the sparse model's lock-step batches); 0 and 1 mean no division.
    The float engine does not implement it: no shape."""
    for ntiles, batch, div in ((48, 14, 14), (48, 14, 2), (48, 24, 2), (48, 24, 24), (100, 7, 7), (641, 4, 4), (1101, 3, 2)):
        for layout in (NT, NN, TN):
            got = lib.gpimhip_gemm_shape_host(0, layout[0], layout[1], STORE, ntiles, batch, div, 0)
            assert got == expected_shape(0, layout, STORE, ntiles * batch // div, 1), (ntiles, batch, div)
            assert got == expected_shape(0, layout, STORE, ntiles, batch, div)
    for div in (0, 1):
        assert lib.gpimhip_gemm_shape_host(0, 0, 0, STORE, 48, 14, div, 0) == expected_shape(0, NT, STORE, 48 * 14, 1)
        assert lib.gpimhip_gemm_shape_host(1, 0, 0, STORE, 48, 6, div, 0) == expected_shape(1, NT, STORE, 48 * 6, 1)
    assert lib.gpimhip_gemm_shape_host(1, 0, 0, STORE, 48, 6, 2, 0) == -1


def test_shape_rejects(lib):
    for fp32 in (0, 1):
        assert lib.gpimhip_gemm_shape_host(fp32, 1, 0, STORE, 10, 1, 0, 0) == -1        # TT: no such kernel
        for layout in (NT, TN, (1, 0)):
            assert lib.gpimhip_gemm_shape_host(fp32, layout[0], layout[1], COLSUMSQ, 10, 1, 0, 0) == -1
        assert lib.gpimhip_gemm_shape_host(fp32, 0, 0, 2, 10, 1, 0, 0) == -1
        assert lib.gpimhip_gemm_shape_host(fp32, 0, 0, STORE, 0, 1, 0, 0) == -1
        assert lib.gpimhip_gemm_shape_host(fp32, 0, 0, STORE, 10, 0, 0, 0) == -1
