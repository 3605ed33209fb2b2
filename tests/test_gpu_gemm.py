"""The MFMA tile engine by itself (gemm.hip / gemm_body.hpp: double, gemm_kernel.hpp: float; it carries every O(N^3) stage
that replaces torch.linalg.cholesky and the solves at gpim/gpreg/gpr.py:192-193,248), launched through the diagnostic entry
gpimhip_gemm_tiles -- the production dispatch, one launch -- and compared with plain block arithmetic on the CPU:

    C[ci + c_roff, ccb + c_coff] = alpha * sum_{kb in [kb0, kb1)} A-block(ci, kb) B-block(kb, cj) + beta * C

Exact cases: operands are integers in [-8, 8], alpha in {1, -2, 0.5}, beta in {0, 1, -1}, at most 6 k-blocks, so every
partial sum is an integer below 6 * 128 * 64 < 2^24 (times 2, plus |C| <= 50): exact in float and double in any order of
summation, and the comparison is assert_array_equal.
  NaN poison  every element of A and B that no listed tile needs is NaN -- the padding behind each row (every leading
              dimension exceeds the addressed width, all three differ), the blocks no tile names, guard block rows behind
              the last one, and under `rag` the elements the engine is documented to skip.  A NaN in the output proves
              that an out-of-range element went into a product.
  canary      C starts as random integers, guard rows and padding included; whatever no tile owns must keep its bits.  With
              beta = 1 a tile computed twice shows as a doubled product.
The guard rows are sized so that an index bug of the kinds the engine could have (a k-range walked the wrong way, a
rectangle strip taken as full) still lands inside the allocations.

Shapes are reached as the dispatch reaches them -- by tile count (tests/test_gemm_host.py holds the table) -- and every
case asserts the shape it ran in through gpimhip_gemm_shape_host."""
import ctypes

import numpy as np
import pytest
import torch

from test_gemm_host import COLSUMSQ, NN, NT, STORE, TABLE, TN, expected_shape

pytestmark = pytest.mark.gpu

NB = 128
PREC = {"f64": dict(np=np.float64, precision="double", u=2.0 ** -53, bits=np.int64, fp32=0),
        "f32": dict(np=np.float32, precision="single", u=2.0 ** -24, bits=np.int32, fp32=1)}
LAYOUTS = {"NT": NT, "NN": NN, "TN": TN}
AB = [(1.0, 0.0), (-2.0, 1.0), (0.5, -1.0), (1.0, 1.0), (-2.0, 0.0), (0.5, 1.0), (1.0, -1.0), (-2.0, -1.0), (0.5, 0.0)]
# batches that take a 48-tile launch into the shapes chosen by count: one CU per tile, and beyond (test_gemm_host.TABLE)
BATCH48 = {("f64", "8w_lds"): 14, ("f64", "big"): 24, ("f32", "8w_lds"): 6, ("f32", "big"): 43}


@pytest.fixture(scope="module")
def eng(ensure_built):
    from gpim_amd import _lib
    H = {k: _lib.Handle(precision=v["precision"]) for k, v in PREC.items()}
    yield _lib, H
    for h in H.values():
        h.close()


def shape_name(prec, layout, shape):
    """the GemmShape a case is meant to run in: 'big' is what lies beyond the one-CU-per-tile range"""
    return {"big": "8w" if layout == NT else "4w"}.get(shape, shape)


class Launch:
    """One launch of the engine: operands, canary, descriptor, and the CPU reference."""

    def __init__(self, prec, layout, tiles=None, epi=STORE, alpha=1.0, beta=0.0, offs=(0, 0, 0, 0, 0, 0), kfix=(0, 0), krev=0,
                 chunk=0, rect=(0, 0), cj_max=0, cmap=0, rag=0, inplace=0, bshift=0, shape_div=0, batch=1, share_a=True,
                 share_b=True, real=False, seed=0, c_guard=8):
        self.prec, self.layout, self.epi, self.alpha, self.beta, self.offs = prec, layout, epi, alpha, beta, offs
        self.kfix, self.krev, self.chunk, self.rect, self.cj_max, self.cmap, self.rag = kfix, krev, chunk, rect, cj_max, cmap, rag
        self.inplace, self.bshift, self.shape_div, self.batch = inplace, bshift, shape_div, batch
        self.share_a, self.share_b, self.real = share_a, share_b, real
        self.listed = rect[1] == 0
        # a rectangle launch names no list: it covers every tile of rect_rows x rect_cols (GemmArgs::rect_rows)
        self.tiles = [tuple(t) for t in tiles] if self.listed else [(ci, cj, 0, 0) for ci in range(rect[0]) for cj in range(rect[1])]
        self.build(np.random.default_rng(seed), c_guard)

    # rows of block row ci that a launch computes, and k of block kq that a range ending at k1 reads (GemmArgs::rag)
    def mrows(self, ci):
        return 64 if self.rag and ci == self.rag - 1 else NB

    def klen(self, k1, kq):
        return 64 if self.rag and k1 == self.rag and kq == k1 - 1 else NB

    def effective(self):
        """(ci, cj, k0, k1, output block column, skipped) per tile"""
        out = []
        for ci, cj, kb0, kb1 in self.tiles:
            k0, k1 = self.kfix if self.kfix[1] > self.kfix[0] else (kb0, kb1)
            out.append((ci, cj, k0, k1, kb0 if self.cmap else cj, self.cj_max > 0 and cj >= self.cj_max))
        return out

    def a_region(self, ci, kq, kl):
        a_r, a_c = self.offs[0], self.offs[1]
        if self.layout[0]:
            return slice((kq + a_r) * NB, (kq + a_r) * NB + kl), slice((ci + a_c) * NB, (ci + a_c) * NB + self.mrows(ci))
        return slice((ci + a_r) * NB, (ci + a_r) * NB + self.mrows(ci)), slice((kq + a_c) * NB, (kq + a_c) * NB + kl)

    def b_region(self, cj, kq, kl):
        b_r, b_c = self.offs[2], self.offs[3]
        if self.layout[1]:
            return slice((kq + b_r) * NB, (kq + b_r) * NB + kl), slice((cj + b_c) * NB, (cj + b_c) * NB + NB)
        return slice((cj + b_r) * NB, (cj + b_r) * NB + NB), slice((kq + b_c) * NB, (kq + b_c) * NB + kl)

    def build(self, rng, c_guard):
        P = PREC[self.prec]
        a_km, b_km = self.layout
        a_r, a_c, b_r, b_c, c_r, c_c = self.offs
        E = self.E = self.effective()
        mb, nbk = max(e[0] for e in E) + 1, max(e[1] for e in E) + 1
        kb, cb = max([e[3] for e in E] + [1]), max(e[4] for e in E) + 1
        og = max(8, kb)                                         # guard block rows behind the operands
        rows_a, cols_a = (kb + a_r + og, mb + a_c) if a_km else (mb + a_r + og, kb + a_c)
        rows_b, cols_b = (kb + b_r + og, nbk + b_c) if b_km else (nbk + b_r + og, kb + b_c)
        self.lda, self.ldb, self.ldc = cols_a * NB + 16, cols_b * NB + 32, (cb + c_c) * NB + 48
        mask_a, mask_b = np.zeros((rows_a * NB, self.lda), bool), np.zeros((rows_b * NB, self.ldb), bool)
        for ci, cj, k0, k1, _, skipped in E:
            if skipped:
                continue
            for kq in range(k0, k1):
                mask_a[self.a_region(ci, kq, self.klen(k1, kq))] = True
                mask_b[self.b_region(cj, kq, self.klen(k1, kq))] = True

        def operand(n, mask):
            shape = (n,) + mask.shape
            v = rng.uniform(-1.0, 1.0, shape) if self.real else rng.integers(-8, 9, shape)
            v = v.astype(P["np"])
            v[:, ~mask] = np.nan
            return v
        self.A = operand(1 if self.share_a else self.batch, mask_a)
        self.B = operand(1 if self.share_b else self.batch >> self.bshift, mask_b)
        # (one problem more than the batch: the canary behind the last one)
        if self.epi == STORE:
            self.C0 = rng.integers(-50, 51, (self.batch + 1, (mb + c_r + c_guard) * NB, self.ldc), dtype=np.int8).astype(P["np"])
            self.cp0 = None
        else:
            self.C0 = None
            self.ld_cp = (nbk + c_c) * NB + 16
            self.cp0 = rng.integers(-50, 51, (self.batch + 1, mb, self.ld_cp)).astype(np.float64)

    def product(self, p, i):
        """tile i of problem p in float64: sum over its k-range of A-block B-block, and of |A-block| |B-block|"""
        pa, pb = 0 if self.share_a else p, 0 if self.share_b else p >> self.bshift
        key = (pa, pb, i)
        if key not in self.cache:
            ci, cj, k0, k1, _, _ = self.E[i]
            acc, mag = np.zeros((self.mrows(ci), NB)), np.zeros((self.mrows(ci), NB))
            for kq in range(k0, k1):
                kl = self.klen(k1, kq)
                a = self.A[pa][self.a_region(ci, kq, kl)].astype(np.float64)
                b = self.B[pb][self.b_region(cj, kq, kl)].astype(np.float64)
                a, b = (a.T if self.layout[0] else a), (b if self.layout[1] else b.T)
                acc += a @ b
                if self.real:
                    mag += np.abs(a) @ np.abs(b)
            self.cache[key] = (acc, mag)
        return self.cache[key]

    def reference(self):
        """expected output (in the engine's type), the mask of what the launch owns, and for real inputs the float64
        reference with the magnitude sum |A||B|"""
        self.cache = {}
        c_r, c_c = self.offs[4], self.offs[5]
        out0 = self.C0 if self.epi == STORE else self.cp0
        want, own = out0.copy(), np.zeros(out0.shape, bool)
        ref, mag = (np.zeros(out0.shape), np.zeros(out0.shape)) if self.real else (None, None)
        for p in range(self.batch):
            for i, (ci, cj, k0, k1, ccb, skipped) in enumerate(self.E):
                if skipped:
                    continue
                acc, m = self.product(p, i)
                if self.epi == STORE:
                    at = (p, slice((ci + c_r) * NB, (ci + c_r) * NB + self.mrows(ci)), slice((ccb + c_c) * NB, (ccb + c_c) * NB + NB))
                    assert not own[at].any(), "the case lists an output tile twice"
                    val = self.alpha * acc + self.beta * self.C0[at].astype(np.float64)
                    if self.real:
                        ref[at], mag[at] = val, abs(self.alpha) * m
                else:
                    at = (p, ci, slice((cj + c_c) * NB, (cj + c_c) * NB + NB))
                    val = (acc * acc).sum(axis=0)
                    if self.real:
                        ref[at], mag[at] = val, (2.0 * np.abs(acc) * m).sum(axis=0)
                want[at] = val
                own[at] = True
        return want, own, ref, mag

    def descriptor(self, _lib, dev):
        P = PREC[self.prec]
        self.dA, self.dB = torch.from_numpy(self.A).to(dev), torch.from_numpy(self.B).to(dev)
        self.dC = torch.from_numpy(self.C0).to(dev) if self.epi == STORE else None
        self.dcp = torch.from_numpy(self.cp0).to(dev) if self.epi == COLSUMSQ else None
        d = _lib.GemmTestStruct()
        d.A, d.lda, d.a_roff, d.a_coff = self.dA.data_ptr(), self.lda, self.offs[0], self.offs[1]
        d.B, d.ldb, d.b_roff, d.b_coff = self.dB.data_ptr(), self.ldb, self.offs[2], self.offs[3]
        d.C, d.ldc, d.c_roff, d.c_coff = (self.dC.data_ptr() if self.dC is not None else None), self.ldc, self.offs[4], self.offs[5]
        if self.dcp is not None:
            d.colpart, d.ld_colpart, d.sColpart = self.dcp.data_ptr(), self.ld_cp, self.cp0.shape[1] * self.ld_cp
        d.alpha, d.beta = self.alpha, self.beta
        self.host_tiles = np.ascontiguousarray(np.array(self.tiles, dtype=np.int32).reshape(-1, 4))
        d.tiles = self.host_tiles.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)) if self.listed else None
        d.ntiles = len(self.tiles)
        d.a_km, d.b_km, d.epi = self.layout[0], self.layout[1], self.epi
        d.krev, d.chunk, d.kfix0, d.kfix1 = self.krev, self.chunk, self.kfix[0], self.kfix[1]
        d.rect_rows, d.rect_cols, d.cj_max, d.cmap, d.rag = self.rect[0], self.rect[1], self.cj_max, self.cmap, self.rag
        d.inplace, d.bshift, d.shape_div, d.batch = self.inplace, self.bshift, self.shape_div, self.batch
        d.sA = 0 if self.share_a else self.A.shape[1] * self.lda
        d.sB = 0 if self.share_b else self.B.shape[1] * self.ldb
        d.sC = self.C0.shape[1] * self.ldc if self.epi == STORE else 0
        assert P["np"] == self.A.dtype
        return d

    def shape(self, lib):
        return lib.gpimhip_gemm_shape_host(PREC[self.prec]["fp32"], self.layout[0], self.layout[1], self.epi, len(self.tiles),
                                           self.batch, self.shape_div, self.inplace)

    def run(self, eng, want_shape=None):
        """launches; returns the return code and the output (C, or colpart) as the host sees it afterwards"""
        _lib, H = eng
        h = H[self.prec]
        if want_shape is not None:
            name = shape_name(self.prec, self.layout, want_shape)
            assert self.shape(h.lib) == _lib.GEMM_SHAPES[name], "the case does not reach the %s shape" % name
            assert self.shape(h.lib) == expected_shape(PREC[self.prec]["fp32"], self.layout, self.epi, len(self.tiles), self.batch,
                                                       self.shape_div, self.inplace)
        d = self.descriptor(_lib, h.device)
        rc = h.lib.gpimhip_gemm_tiles(h.h, ctypes.byref(d))
        out = (self.dC if self.epi == STORE else self.dcp).cpu().numpy()
        self.dA = self.dB = self.dC = self.dcp = None
        return rc, out

    def check_exact(self, got):
        want, own, _, _ = self.reference()
        bits = PREC[self.prec]["bits"] if self.epi == STORE else np.int64
        if np.array_equal(got.view(bits), want.view(bits)):
            return
        assert not np.isnan(got).any(), "NaN in the output: an element no tile may address went into a product"
        stray = (got.view(bits) != want.view(bits)) & ~own
        assert not stray.any(), "%d elements outside the launch's tiles changed, first at %s" % (stray.sum(), np.argwhere(stray)[0])
        np.testing.assert_array_equal(got, want)

    def check_bound(self, got, factor):
        """real inputs: |got - ref| <= factor * gamma_k * (|A||B|) elementwise, gamma_k = k u / (1 - k u) for the longest
        k-range of the launch -- the bound of a dot product summed in any order; what the launch does not own keeps its bits"""
        want, own, ref, mag = self.reference()
        k = max(e[3] - e[2] for e in self.E) * NB
        ku = k * PREC[self.prec]["u"]
        bits = PREC[self.prec]["bits"]
        assert not np.isnan(got).any()
        assert np.array_equal(got.view(bits)[~own], want.view(bits)[~own])
        err, bound = np.abs(got.astype(np.float64) - ref)[own], (factor * ku / (1.0 - ku) * mag)[own]
        print("k = %d: max |C - ref| / (gamma_k |A||B|) = %.3f (allowed %.1f)" % (k, (err / (ku / (1.0 - ku) * mag[own])).max(), factor))
        assert (err <= bound).all()


def run_exact(eng, L, want_shape=None):
    rc, got = L.run(eng, want_shape)
    assert rc == 0, eng[0].load().gpimhip_last_error()
    L.check_exact(got)


def grid48(i):
    """tile i of 48 on a 6 x 8 grid, k-ranges of 1 .. 3 blocks starting at block 0 or 1"""
    return (i // 8, i % 8, i % 2, i % 2 + 1 + i % 3)


def lower_list(nb, ends):
    """the lower tiles of an nb x nb block matrix with the k-ranges of the triangular inverse, [cj, ci] ('in'), or of
    K^-1 = L^-T L^-1, [ci, nb) ('end'); plus two tiles above the diagonal with ranges of length 0"""
    t = [(ci, cj, cj, ci + 1) if ends == "in" else (ci, cj, ci, nb) for ci in range(nb) for cj in range(ci + 1)]
    return t + [(0, 1, 2, 2), (1, nb - 1, 0, 0)]


# ------------------------------------------------------------------------------------------
# layouts x shapes
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["quad", "rowhalf", "8w_lds", "big"])
@pytest.mark.parametrize("layout", ["NT", "NN", "TN"])
@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_layouts_in_every_shape(eng, prec, layout, shape):
    """48 tiles, operands shared by the problems of the batch (strides 0), C distinct per problem.  The row-half shape is
    reached with inplace = 1 and a C that aliases nothing."""
    batch = BATCH48.get((prec, shape), 1)
    L = Launch(prec, LAYOUTS[layout], [grid48(i) for i in range(48)], alpha=-2.0, beta=1.0, batch=batch, chunk=8,
               inplace=int(shape == "rowhalf"), c_guard=8 if batch == 1 else 0, seed=48)
    run_exact(eng, L, shape)


# ------------------------------------------------------------------------------------------
# k-ranges
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["quad", "rowhalf", "8w_lds"])
@pytest.mark.parametrize("layout", ["NT", "NN", "TN"])
@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_k_ranges_per_tile(eng, prec, layout, shape):
    """Ranges of 0 .. 4 blocks that differ from tile to tile, both triangular lists, walked from either end."""
    nb = 4 if shape != "8w_lds" else 3
    n = 0
    for ends in ("in", "end"):
        tiles = lower_list(nb, ends)
        batch = 1 if shape != "8w_lds" else TABLE[PREC[prec]["fp32"]]["small"] // len(tiles) + 1
        for krev in (0, 1):
            alpha, beta = AB[n % len(AB)]
            n += 1
            L = Launch(prec, LAYOUTS[layout], tiles, alpha=alpha, beta=beta, krev=krev, chunk=n % 2, batch=batch,
                       inplace=int(shape == "rowhalf"), c_guard=8 if batch == 1 else 0, seed=n)
            run_exact(eng, L, shape)


@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_k_range_of_length_zero(eng, prec):
    """An empty range leaves beta * C, and exactly 0 where beta = 0 -- whatever alpha is, krev or not."""
    tiles = [(0, 0, 0, 0), (0, 1, 3, 3), (1, 0, 1, 1), (1, 1, 0, 2)]
    for layout in (NT, NN, TN):
        for (alpha, beta), krev, inplace in zip(AB, (0, 1) * 5, (0, 0, 1) * 3):
            L = Launch(prec, layout, tiles, alpha=alpha, beta=beta, krev=krev, inplace=inplace, seed=7)
            rc, got = L.run(eng, "rowhalf" if inplace else "quad")
            assert rc == 0
            L.check_exact(got)
            for ci, cj in ((0, 0), (0, 1), (1, 0)):
                blk = got[0, ci * NB:(ci + 1) * NB, cj * NB:(cj + 1) * NB]
                assert np.array_equal(blk, beta * L.C0[0, ci * NB:(ci + 1) * NB, cj * NB:(cj + 1) * NB])
                if beta == 0.0:
                    assert not blk.any()


@pytest.mark.parametrize("layout", ["NT", "NN", "TN"])
@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_kfix_overrides_the_list(eng, prec, layout):
    """kfix0 < kfix1: every tile uses that range; its own -- empty, longer, elsewhere -- is ignored (its blocks are NaN)."""
    tiles = [(0, 0, 0, 0), (0, 1, 0, 6), (1, 0, 5, 6), (1, 1, 2, 3), (2, 0, 1, 2), (2, 1, 4, 4)]
    for n, (kfix, krev) in enumerate((((1, 3), 0), ((1, 3), 1), ((0, 1), 0), ((2, 6), 1))):
        alpha, beta = AB[n]
        run_exact(eng, Launch(prec, LAYOUTS[layout], tiles, alpha=alpha, beta=beta, kfix=kfix, krev=krev, seed=n), "quad")


# ------------------------------------------------------------------------------------------
# tile counts against the XCD remap
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chunk,ntiles", [(0, 1), (0, 7), (0, 8), (0, 9), (0, 11), (0, 16), (1, 1), (1, 7), (1, 8), (1, 9),
                                          (1, 19), (8, 63), (8, 64), (8, 65), (8, 131)])
@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_tile_counts_against_the_remap(eng, prec, chunk, ntiles):
    """One workgroup per tile (the batch takes the launch out of the quadrant shape, where chunk plays no part): with
    beta = 1 a tile the remap drops keeps its canary and one it deals twice gets its product twice.  8 c - 1, 8 c,
    8 c + 1 and 16 c + 3 tiles for chunk c; chunk 0 with ntiles % 8 in {0, 1, 3, 7}."""
    w = min(ntiles, 8)
    tiles = [(i // w, i % w, 0, 1) for i in range(ntiles)]
    batch = TABLE[PREC[prec]["fp32"]]["small"] // ntiles + 1
    run_exact(eng, Launch(prec, NT, tiles, alpha=1.0, beta=1.0, chunk=chunk, batch=batch, c_guard=0, seed=ntiles), "8w_lds")


# ------------------------------------------------------------------------------------------
# offsets, leading dimensions, batch addressing
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["NT", "NN", "TN"])
@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_block_offsets(eng, prec, layout):
    """All six block offsets non-zero at once (lda, ldb, ldc differ in every case of this file)."""
    tiles = lower_list(3, "in")
    for n, inplace in enumerate((0, 1)):
        alpha, beta = AB[n + 1]
        L = Launch(prec, LAYOUTS[layout], tiles, alpha=alpha, beta=beta, offs=(2, 1, 1, 3, 1, 2), krev=n, inplace=inplace, seed=n)
        assert len({L.lda, L.ldb, L.ldc}) == 3
        run_exact(eng, L, "rowhalf" if inplace else "quad")


@pytest.mark.parametrize("layout", ["NT", "NN", "TN"])
@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_batch_strides(eng, prec, layout):
    """batch 3 with operands and strides of their own; batch 4 with bshift = 1: problems 2 q and 2 q + 1 share B."""
    tiles = lower_list(3, "end")
    run_exact(eng, Launch(prec, LAYOUTS[layout], tiles, alpha=0.5, beta=-1.0, batch=3, share_a=False, share_b=False, seed=3), "quad")
    run_exact(eng, Launch(prec, LAYOUTS[layout], tiles, alpha=-2.0, beta=1.0, batch=4, share_a=False, share_b=False, bshift=1,
                          krev=1, seed=4), "quad")
    run_exact(eng, Launch(prec, LAYOUTS[layout], tiles, alpha=1.0, beta=0.0, batch=4, share_a=True, share_b=False, bshift=2,
                          inplace=1, seed=5), "rowhalf")


@pytest.mark.parametrize("layout", ["NT", "NN", "TN"])
def test_shape_div(eng, layout):
    """shape_div = 2 (double engine): 48 tiles x 14 run in the shape of 336 tiles -- quadrants, not one CU per tile."""
    L = Launch("f64", LAYOUTS[layout], [grid48(i) for i in range(48)], alpha=0.5, beta=1.0, batch=14, shape_div=2, share_b=False,
               c_guard=0, seed=14)
    run_exact(eng, L, "quad")


# ------------------------------------------------------------------------------------------
# switches of the double engine
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cols", [1, 3])
@pytest.mark.parametrize("rows", [1, 8, 9, 13])
def test_rectangle_without_a_list(eng, rows, cols):
    """rect_rows x rect_cols with tiles = NULL (the distributed solve's NN update, the border's TN product)."""
    for n, (layout, chunk) in enumerate(((NN, 64), (TN, 0))):
        alpha, beta = AB[n + 1]
        run_exact(eng, Launch("f64", layout, rect=(rows, cols), kfix=(n, n + 2), alpha=alpha, beta=beta, chunk=chunk, krev=n,
                              offs=(n, 0, 0, n, n, 0), seed=rows * cols), "quad")


@pytest.mark.parametrize("rows", [9, 13])
def test_rectangle_one_workgroup_per_tile(eng, rows):
    """... dealt to the XCDs in 8 x 8 patches (chunk = 64), a last strip lower than eight rows"""
    batch = TABLE[0]["small"] // (rows * 3) + 1
    run_exact(eng, Launch("f64", NN, rect=(rows, 3), kfix=(0, 1), alpha=-2.0, beta=1.0, chunk=64, batch=batch, c_guard=0, seed=rows),
              "8w_lds")


@pytest.mark.parametrize("layout", ["NT", "NN", "TN"])
def test_cj_max(eng, layout):
    """tiles with cj >= cj_max are untouched and their operand blocks never read"""
    tiles = [(ci, cj, 0, 1 + (ci + cj) % 2) for ci in range(3) for cj in range(4)]
    for n, cj_max in enumerate((2, 1, 4)):
        alpha, beta = AB[n]
        run_exact(eng, Launch("f64", LAYOUTS[layout], tiles, alpha=alpha, beta=beta, cj_max=cj_max, inplace=n % 2, seed=n),
                  "rowhalf" if n % 2 else "quad")


@pytest.mark.parametrize("layout", ["NT", "NN", "TN"])
def test_cmap(eng, layout):
    """cmap: the output block column is the tile's kb0 (operand columns stay cj); the k-range comes from kfix"""
    tiles = [(ci, cj, (cj + ci) % 4, (cj + ci) % 4) for ci in range(3) for cj in range(4)]       # (a permutation of the columns per row)
    for n, kfix in enumerate(((0, 2), (1, 2))):
        alpha, beta = AB[n + 1]
        run_exact(eng, Launch("f64", LAYOUTS[layout], tiles, alpha=alpha, beta=beta, cmap=1, kfix=kfix, offs=(0, 0, 0, 0, 1, 1),
                              seed=n), "quad")


def rag_tiles(nb):
    """every tile of an nb x nb matrix whose last block is ragged: on and below the diagonal the range [ci, nb) ends
    with it (one block only in the last row), above the diagonal [0, cj) does not"""
    return [(ci, cj, ci, nb) if cj <= ci else (ci, cj, 0, cj) for ci in range(nb) for cj in range(nb)]


@pytest.mark.parametrize("shape", ["quad", "rowhalf", "8w_lds", "big"])
@pytest.mark.parametrize("layout", ["NT", "NN", "TN"])
def test_rag(eng, layout, shape):
    """rag = nb: rows >= 64 of block row nb - 1 of C keep their canary, and the last 64 k of a range ending at block nb are
    SKIPPED, as GemmArgs::rag says -- those elements of A and B are NaN here (and so are rows >= 64 of A's last block
    row), not the identity padding of the callers.  Every shape the dispatch can give a ragged launch; beta = 0 in the
    first launch, where a dead row that is stored after all becomes 0."""
    nb = 3
    tiles = rag_tiles(nb)
    batch = {"8w_lds": TABLE[0]["small"] // len(tiles) + 1, "big": TABLE[0]["mid"] // len(tiles) + 1}.get(shape, 1)
    for n, ((alpha, beta), krev) in enumerate((((1.0, 0.0), 1), ((0.5, -1.0), 0))):
        L = Launch("f64", LAYOUTS[layout], tiles, alpha=alpha, beta=beta, rag=nb, krev=krev, chunk=n, batch=batch,
                   inplace=int(shape == "rowhalf"), c_guard=8 if batch == 1 else 0, seed=n)
        run_exact(eng, L, shape)


# ------------------------------------------------------------------------------------------
# column sums of squares
# ------------------------------------------------------------------------------------------
def pred_tiles(mb, nc):
    """the variance product L^-1 K*: row block ci reads the blocks [0, ci] of the lower-triangular operand"""
    return [(ci, cj, 0, min(ci + 1, 6)) for ci in range(mb) for cj in range(nc)]


@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_colsumsq_eight_waves(eng, prec):
    """colpart[ci][(cj + c_coff) 128 + col] = the exact integer column sums of squares (sums below 2^53), for a batch
    with sColpart and distinct B; what no tile owns keeps its canary."""
    L = Launch(prec, NN, pred_tiles(5, 3), epi=COLSUMSQ, batch=3, share_b=False, offs=(0, 0, 0, 0, 0, 1), chunk=8, seed=1)
    run_exact(eng, L, "8w")


@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_colsumsq_four_waves(eng, prec):
    """more than 256 tiles: of the batch for the double engine, of one problem for the float engine"""
    if prec == "f64":
        L = Launch(prec, NN, pred_tiles(9, 8), epi=COLSUMSQ, batch=4, share_b=False, chunk=8, seed=2)
    else:
        L = Launch(prec, NN, pred_tiles(17, 16), epi=COLSUMSQ, batch=2, share_b=False, chunk=8, seed=2)
    run_exact(eng, L, "4w")


@pytest.mark.parametrize("shape", ["8w", "4w"])
def test_colsumsq_cj_max_and_rag(eng, shape):
    """double engine: skipped column tiles keep their canary; under rag the last row block sums its 64 live rows and a
    range ending at block rag stops 64 short"""
    mb, nc, batch = (4, 5, 2) if shape == "8w" else (9, 8, 4)
    tiles = [(ci, cj, 0, ci + 1) for ci in range(mb) for cj in range(nc)]
    run_exact(eng, Launch("f64", NN, tiles, epi=COLSUMSQ, batch=batch, share_b=False, cj_max=nc - 2, seed=3), shape)
    run_exact(eng, Launch("f64", NN, tiles, epi=COLSUMSQ, batch=batch, share_b=False, rag=mb, seed=4), shape)
    run_exact(eng, Launch("f64", NN, tiles, epi=COLSUMSQ, batch=batch, share_b=False, rag=mb, cj_max=nc - 1, chunk=8, seed=5), shape)


@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_colsumsq_bits_alone_and_in_a_batch(eng, prec):
    """Real inputs.  A problem gives the same colpart bits alone and inside a batch that takes the launch past 256 tiles:
    the float engine picks the shape from one problem's tiles; the double engine does when the caller divides the batch
    out again (shape_div = batch, the sparse model's rule).  Against float64: the products are off by at most
    gamma_k |A||B| (twice that for the double engine's reference), the squares and their 128-term sum add gamma_130."""
    _lib, H = eng
    batch = 4
    kw = dict(epi=COLSUMSQ, share_b=False, real=True, chunk=8, seed=11)
    L = Launch(prec, NN, pred_tiles(9, 8), batch=batch, shape_div=batch if prec == "f64" else 0, **kw)
    rc, got = L.run(eng, "8w")
    assert rc == 0
    want, own, ref, mag = L.reference()
    assert np.array_equal(got.view(np.int64)[~own], want.view(np.int64)[~own])
    ku, factor = 6 * NB * PREC[prec]["u"], 2.0 if prec == "f64" else 1.0
    e = factor * ku / (1.0 - ku)            # a product p is off by at most e m, m = (|A||B|) <= 768: its square by 2 |p| e m + (e m)^2
    bound = e * mag + NB * (e * 6 * NB) ** 2 + 130 * 2.0 ** -53 * 1.01 * (ref + e * mag)
    assert (np.abs(got - ref)[own] <= bound[own]).all()
    for p in range(batch):
        S = Launch(prec, NN, pred_tiles(9, 8), batch=1, **kw)
        S.B = L.B[p:p + 1].copy()
        assert np.array_equal(S.A, L.A, equal_nan=True)
        rc, alone = S.run(eng, "8w")
        assert rc == 0
        assert np.array_equal(alone[0].view(np.int64)[own[p]], got[p].view(np.int64)[own[p]]), p


# ------------------------------------------------------------------------------------------
# rounding
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["NT", "NN", "TN"])
@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_rounding(eng, prec, layout):
    """Real inputs uniform in [-1, 1], 6 tiles, 3 k-blocks: against float64 block arithmetic on the same (rounded) inputs,
    |C - ref| <= f gamma_384 (|A||B|) elementwise, f = 2 for double (the reference rounds like the engine) and 1 for
    float (the reference's error is 2^-29 of the bound)."""
    tiles = [(ci, cj, 0, 3) for ci in range(2) for cj in range(3)]
    L = Launch(prec, LAYOUTS[layout], tiles, alpha=1.0, beta=0.0, real=True, seed=384)
    rc, got = L.run(eng, "quad")
    assert rc == 0
    L.check_bound(got, 2.0 if prec == "f64" else 1.0)


# ------------------------------------------------------------------------------------------
# what the entry and the float engine refuse
# ------------------------------------------------------------------------------------------
def refused(eng, L, edit):
    """the descriptor of L after edit(d) returns BADARG with a message and launches nothing: C keeps its bits"""
    _lib, H = eng
    h = H[L.prec]
    d = L.descriptor(_lib, h.device)
    edit(d)
    rc = h.lib.gpimhip_gemm_tiles(h.h, ctypes.byref(d))
    msg = h.lib.gpimhip_last_error().decode()
    out = (L.dC if L.epi == STORE else L.dcp).cpu().numpy()
    out0 = L.C0 if L.epi == STORE else L.cp0
    assert rc == _lib.E_BADARG and msg
    assert np.array_equal(out.view(np.uint8), out0.view(np.uint8))
    return msg


@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_entry_rejects_bad_descriptors(eng, prec):
    L = Launch(prec, NN, [(0, 0, 0, 1), (1, 0, 0, 2)], seed=1)
    for field in ("A", "B", "C", "tiles"):
        assert "null" in refused(eng, L, lambda d, f=field: setattr(d, f, None))
    for field, value in (("ntiles", 0), ("ntiles", -3), ("batch", 0), ("batch", -1), ("lda", 0), ("ldc", -8)):
        refused(eng, L, lambda d, f=field, v=value: setattr(d, f, v))
    assert "layout" in refused(eng, L, lambda d: (setattr(d, "a_km", 1), setattr(d, "b_km", 0)))
    assert "layout" in refused(eng, L, lambda d: (setattr(d, "epi", COLSUMSQ), setattr(d, "colpart", d.C), setattr(d, "b_km", 0),
                                                  setattr(d, "ld_colpart", 256)))
    assert "kfix" in refused(eng, L, lambda d: (setattr(d, "rect_rows", 2), setattr(d, "rect_cols", 1), setattr(d, "tiles", None)))
    assert "kfix" in refused(eng, L, lambda d: setattr(d, "cmap", 1))
    refused(eng, L, lambda d: (setattr(d, "rect_rows", 3), setattr(d, "rect_cols", 1), setattr(d, "kfix1", 1)))    # ntiles != 3 x 1
    refused(eng, L, lambda d: setattr(d, "epi", 2))
    K = Launch(prec, NN, [(0, 0, 0, 1)], epi=COLSUMSQ, seed=2)
    assert "null" in refused(eng, K, lambda d: setattr(d, "colpart", None))
    _lib, H = eng
    assert H[prec].lib.gpimhip_gemm_tiles(H[prec].h, None) == _lib.E_BADARG
    assert H[prec].lib.gpimhip_gemm_tiles(None, None) == _lib.E_BADARG


@pytest.mark.parametrize("switch", ["rect_cols", "cj_max", "cmap", "rag", "shape_div"])
def test_float_engine_refuses_what_it_does_not_implement(eng, switch):
    """The float kernels have no code for these GemmArgs switches: a launch that carries one is an error, not a launch
    that ignores it (or, with rect_cols, one that reads a null tile list)."""
    L = Launch("f32", NN, [(ci, cj, 0, 1) for ci in range(2) for cj in range(2)], kfix=(0, 1), beta=1.0, seed=3)
    edits = {"rect_cols": lambda d: (setattr(d, "rect_rows", 2), setattr(d, "rect_cols", 2), setattr(d, "tiles", None)),
             "cj_max": lambda d: setattr(d, "cj_max", 1), "cmap": lambda d: setattr(d, "cmap", 1),
             "rag": lambda d: setattr(d, "rag", 2), "shape_div": lambda d: setattr(d, "shape_div", 2)}
    assert switch in refused(eng, L, edits[switch])
    # (unedited, the descriptor runs)
    run_exact(eng, L, "quad")
