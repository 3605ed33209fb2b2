"""The work plan of lds_factor_inv (gpim_amd/csrc/blocklds.hpp: the Cholesky factorisation of an LDS-resident block of
npan 16-column panels with the triangular inverse built row by row behind it -- the core of the fused trainer for
N <= 128, smalln.hip, at npan = ceil(N / 16), and of the diagonal blocks of the blocked Cholesky at npan = 8) checked
on the HOST, for every npan = 1 .. 8: gpimhip_fi_plan_host returns the words of make_fi_plan(), the constexpr function
the device table c_fi_plan is initialised from.

  * the words are decoded exactly as lds_factor_inv decodes them and held to the invariants that decoding relies on
    (every tile of row p of the inverse formed once, every trailing tile updated once, nothing that does not fit the
    64-bit word);
  * the phases of lds_factor_inv are replayed in numpy on b x b blocks (the plan is expressed in tile indices, so small
    blocks execute the dependency structure of the kernel): per step the panel-solve phase (with the deferred stores of
    the inverse's tiles a worker has held in registers since the previous step, and wave 4's copy of the diagonal
    tile's inverse) and the update phase (row p of the inverse, the trailing tiles, wave 0's diagonal tile and its
    factorisation).  A barrier separates the phases, nothing orders the waves inside one: every operation reads the
    state the phase started from, no tile may be written twice in a phase and none read that another operation of the
    phase writes.  The result is inv(cholesky(A)).

No GPU involved."""
import ctypes

import numpy as np
import pytest

NONE = 15
NWORKER = 7          # workers 0-5: waves 1, 2, 3, 5, 6, 7; worker 6: wave 0 (takes part in the last step only)


def library_words(npan, p):
    from gpim_amd import _lib
    lib = _lib.load()
    out = (ctypes.c_uint64 * NWORKER)()
    assert lib.gpimhip_fi_plan_host(npan, p, out) == 0
    return [int(v) for v in out]


def decode(word):
    """(inverse tiles [j1, j2] with 15 = none, item count, the four 12-bit item fields as (rtA, ctA, rtB, ctB)) -- the
    shifts and masks of lds_factor_inv"""
    inv = [word & 15, (word >> 4) & 15]
    ntr = (word >> 8) & 15
    fields = []
    for n in range(4):
        it = (word >> (12 + 12 * n)) & 0xFFF
        fields.append((it >> 9, (it >> 6) & 7, (it >> 3) & 7, it & 7))
    return inv, ntr, fields


def check_invariants(npan, words=library_words):
    for p in range(npan):
        last = p == npan - 1
        inv_seen, trail_seen = [], []
        for w, word in enumerate(words(npan, p)):
            assert 0 <= word < 1 << 64
            assert word >> 60 == 0                              # 12 + 4 x 12 bits: nothing beyond the fourth item
            inv, ntr, fields = decode(word)
            assert ntr <= 4, "a fifth item does not fit the 64-bit word"
            assert ntr == sum(1 for f in fields if f != (0, 0, 0, 0)), "count field != number of non-zero item fields"
            assert all(f != (0, 0, 0, 0) for f in fields[:ntr]), "the items a worker runs are its first ntr fields"
            held = [j for j in inv if j != NONE]
            assert all(j < p for j in held), (npan, p, w, inv)
            if inv[0] == NONE:
                assert inv[1] == NONE                           # lds_factor_inv skips fi_inv_pair when the first is none
            if len(held) == 2:
                assert inv[0] < inv[1], "fi_inv_pair assumes j1 < j2"
            if w == 6 and not last:
                assert not held and ntr == 0, "wave 0 factors the next diagonal tile in every step but the last"
            inv_seen += held
            for rtA, ctA, rtB, ctB in fields[:ntr]:
                assert max(rtA, ctA, rtB, ctB) <= 7             # (3-bit fields: true by construction, stated for the reader)
                tiles = [(rtA, ctA)] + ([(rtB, ctB)] if rtB != 0 else [])
                if rtB == 0:
                    assert ctB == 0
                for rt, ct in tiles:
                    assert p < ct <= rt < npan and (rt, ct) != (p + 1, p + 1), (npan, p, w, rt, ct)
                trail_seen += tiles
        assert sorted(inv_seen) == list(range(p)), "row %d of the inverse: tiles %s" % (p, sorted(inv_seen))
        want = [] if last else sorted((rt, ct) for rt in range(p + 1, npan) for ct in range(p + 1, rt + 1)
                                      if (rt, ct) != (p + 1, p + 1))
        assert sorted(trail_seen) == want, "step %d of %d: trailing tiles %s" % (p, npan, sorted(trail_seen))


class Phase:
    """One barrier-to-barrier phase: operations read the state the phase started from and record what they touch."""

    def __init__(self, D, Xs, bs):
        self.D, self.Xs, self.bs = D, Xs, bs
        self.D0, self.Xs0 = D.copy(), [x.copy() for x in Xs]
        self.ops = []               # (reads, writes) per operation
        self.cur = None

    def op(self):
        self.cur = (set(), set())
        self.ops.append(self.cur)

    def blk(self, M, i, j):
        return M[i * self.bs:(i + 1) * self.bs, j * self.bs:(j + 1) * self.bs]

    def read(self, i, j):
        self.cur[0].add(("D", i, j))
        return self.blk(self.D0, i, j)

    def read_xs(self, q):
        self.cur[0].add(("Xs", q & 1))
        return self.Xs0[q & 1]

    def write(self, i, j, v):
        self.cur[1].add(("D", i, j))
        self.blk(self.D, i, j)[...] = v

    def write_xs(self, q, v):
        self.cur[1].add(("Xs", q & 1))
        self.Xs[q & 1][...] = v

    def close(self):
        for n, (rd, wr) in enumerate(self.ops):
            for m, (rd2, wr2) in enumerate(self.ops):
                if m == n:
                    continue
                assert not (wr & wr2), "two operations of one phase write %s" % sorted(wr & wr2)
                assert not (rd & wr2), "an operation reads %s, which another one of the same phase writes" % sorted(rd & wr2)


def chol_tile(ph, i):
    """chol16_lp on diagonal tile i (lower part): the factor in place, its inverse to scratch tile i & 1"""
    d = np.tril(ph.blk(ph.D, i, i))
    Lt = np.linalg.cholesky(d + np.tril(d, -1).T)
    ph.write(i, i, Lt)
    ph.write_xs(i, np.linalg.inv(Lt))


def replay(npan, bs, seed=0, words=library_words):
    rng = np.random.default_rng(seed)
    n = npan * bs
    G = rng.standard_normal((n, n))
    K = G @ G.T / n + 2.0 * np.eye(n)
    D = np.full((n, n), np.nan)          # the strictly upper tiles are never read
    for i in range(npan):
        D[i * bs:(i + 1) * bs, :(i + 1) * bs] = K[i * bs:(i + 1) * bs, :(i + 1) * bs]
    Xs = [np.full((bs, bs), np.nan), np.full((bs, bs), np.nan)]
    ph = Phase(D, Xs, bs)
    ph.op()
    chol_tile(ph, 0)
    ph.close()
    keep = [[None, None] for _ in range(NWORKER)]      # tiles of block row p - 1 of X in the workers' registers
    held = [[NONE, NONE] for _ in range(NWORKER)]
    for p in range(npan + 1):
        # ---- panel-solve phase
        ph = Phase(D, Xs, bs)
        for slot in range(7):                          # the seven waves but wave 4
            t = p + 1 + slot
            if p < npan and t < npan:
                ph.op()
                ph.write(t, p, ph.read(t, p) @ ph.read_xs(p).T)
        for w in range(NWORKER):
            for c in range(2):
                if held[w][c] != NONE:
                    ph.op()
                    ph.write(p - 1, held[w][c], keep[w][c])
        if p > 0:                                      # wave 4: X(p-1, p-1) over L(p-1, p-1)
            ph.op()
            ph.write(p - 1, p - 1, ph.read_xs(p - 1))
        ph.close()
        if p == npan:
            break
        # ---- update phase
        last = p == npan - 1
        ph = Phase(D, Xs, bs)
        plan = words(npan, p)
        for w in range(NWORKER):
            held[w] = [NONE, NONE]
            if w == 6 and not last:
                continue
            inv, ntr, fields = decode(plan[w])
            held[w] = inv
            if inv[0] != NONE:                         # fi_inv_pair, its loop bounds as written there
                ph.op()
                j1, j2 = inv
                t1, t2 = np.zeros((bs, bs)), np.zeros((bs, bs))
                ke = j2 if j2 != NONE else p
                k = j1
                if k < ke:
                    for k in range(j1, ke):
                        t1 = t1 + ph.read(p, k) @ ph.read(k, j1)
                    k = ke
                for k in range(k, p):
                    t1 = t1 + ph.read(p, k) @ ph.read(k, j1)
                    t2 = t2 + ph.read(p, k) @ ph.read(k, j2)
                xp = ph.read_xs(p)
                keep[w] = [-xp @ t1, -xp @ t2]
            for rtA, ctA, rtB, ctB in fields[:ntr]:
                ph.op()                                # (fi_trail2 loads both tiles' operands before it stores either)
                for rt, ct in [(rtA, ctA)] + ([(rtB, ctB)] if rtB != 0 else []):
                    ph.write(rt, ct, ph.read(rt, ct) - ph.read(rt, p) @ ph.read(ct, p).T)
        if not last:                                   # wave 0: its own tile, then the 16x16 factorisation
            ph.op()
            s0 = ph.read(p + 1, p)
            ph.write(p + 1, p + 1, ph.read(p + 1, p + 1) - s0 @ s0.T)
            chol_tile(ph, p + 1)
        ph.close()
    want = np.linalg.inv(np.linalg.cholesky(K))
    got = np.tril(D)
    assert not np.isnan(got).any()
    assert np.abs(got - want).max() < 1e-12, np.abs(got - want).max()


@pytest.mark.parametrize("npan", range(1, 9))
def test_plan_invariants(ensure_built, npan):
    check_invariants(npan)


@pytest.mark.parametrize("bs", [2, 3])
@pytest.mark.parametrize("npan", range(1, 9))
def test_plan_replay(ensure_built, npan, bs):
    replay(npan, bs, seed=10 * npan + bs)


def test_plan_arguments(ensure_built):
    from gpim_amd import _lib
    lib = _lib.load()
    out = (ctypes.c_uint64 * NWORKER)()
    for npan, p in [(0, 0), (9, 0), (-1, 0), (1, 1), (8, 8), (5, -1), (3, 3)]:
        assert lib.gpimhip_fi_plan_host(npan, p, out) == _lib.E_BADARG
    assert lib.gpimhip_fi_plan_host(4, 1, None) == _lib.E_BADARG
    assert lib.gpimhip_fi_plan_host(8, 7, out) == 0 and lib.gpimhip_fi_plan_host(1, 0, out) == 0
    # one panel: nothing but the factorisation of the first tile
    assert [int(v) for v in out] == [0xFF] * NWORKER
