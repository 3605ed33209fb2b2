"""The launch plan of the blocked Cholesky with the triangular inverse riding in its launches (cholstep.hip:
plan_updates / plan_inverse; replaces torch.linalg.cholesky + the solves at gpim/gpreg/gpr.py:192-193,248) replayed on
the HOST with small blocks: the plan is expressed in block indices, so an interpreter with 2x2 or 3x3 blocks executes
exactly the dependency structure the GPU launches have.  Launch semantics: every tile operation of a launch reads the
state the launch started from (hosted workgroups run concurrently with each other and with the factorisation of the
diagonal block), so a schedule that hands an operation to a launch too early, lets two operations of one launch write
the same tile, or reads a tile another operation of the same launch writes, fails here.  No GPU involved.

The plan of single-precision handles (plan_updates_f32; executed by cholstep32.hip) is replayed the same way further
down: it has a launch of its own before the first step of a panel (what of the panel's bulk update exceeds the cap on
hosted tiles, from 88 block columns), applies panels two at a time from 160 block columns, and its launch after the
panel solve updates every diagonal tile of the window."""
import ctypes

import numpy as np
import pytest


def plan(nb, with_inverse):
    from gpim_amd import _lib
    lib = _lib.load()
    n = ctypes.c_int64()
    assert lib.gpimhip_step_plan_host(nb, with_inverse, None, 0, ctypes.byref(n)) == 0
    buf = np.zeros((max(n.value, 1), 6), dtype=np.int32)
    assert lib.gpimhip_step_plan_host(nb, with_inverse, buf.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), n.value,
                                      ctypes.byref(n)) == 0
    return buf[:n.value]


def replay(nb, bs, with_inverse, seed=0):
    rng = np.random.default_rng(seed)
    n = nb * bs
    G = rng.standard_normal((n, n))
    K = G @ G.T / n + 2.0 * np.eye(n)
    A = np.tril(K).copy()
    A += np.tril(K, -1).T * 0.0          # (upper part unused)
    Tm = np.full((n, n), np.nan)
    rec = plan(nb, with_inverse)
    by_launch = {}
    for r in rec:
        by_launch.setdefault(int(r[0]), []).append(tuple(int(v) for v in r[1:]))
    blk = lambda M, i, j: M[i * bs:(i + 1) * bs, j * bs:(j + 1) * bs]
    W = 4

    def hosted(ops, A, Tm):
        A0, T0 = A.copy(), Tm.copy()
        written = set()
        reads = set()
        for ci, cj, k0, k1, kind in ops:
            assert 0 <= k0 < k1 and cj <= ci
            dst = ("T" if kind in (1, 2) else "A", ci, cj)
            assert dst not in written, "two operations of one launch write %s" % (dst,)
            written.add(dst)
            acc = np.zeros((bs, bs))
            for k in range(k0, k1):
                if kind == 0:
                    acc += blk(A0, ci, k) @ blk(A0, cj, k).T
                    reads.update({("A", ci, k), ("A", cj, k)})
                elif kind in (1, 2):
                    acc += blk(A0, ci, k) @ blk(A0, k, cj)
                    reads.update({("A", ci, k), ("A", k, cj)})
                else:
                    acc += blk(A0, ci, k) @ blk(T0, k, cj)
                    reads.update({("A", ci, k), ("T", k, cj)})
            if kind == 0:
                blk(A, ci, cj)[...] = blk(A0, ci, cj) - acc
            elif kind == 1:
                blk(Tm, ci, cj)[...] = acc
            elif kind == 2:
                blk(Tm, ci, cj)[...] = blk(T0, ci, cj) + acc
            elif kind == 3:
                blk(A, ci, cj)[...] = -acc
            else:
                blk(A, ci, cj)[...] = blk(A0, ci, cj) - acc
        assert not (written & reads), "an operation reads what another operation of the same launch writes"
        return written

    Lref = np.linalg.cholesky(K)
    for j in range(nb):
        ops = by_launch.get(j, [])
        for o in ops:
            assert o[3] <= j or o[4] != 0, "a trailing update uses a block column that is not final"
        written = hosted(ops, A, Tm)
        assert ("A", j, j) not in written
        # factorisation role of the same launch (concurrent with the hosted tiles: it only touches block (j, j))
        d = np.tril(blk(A, j, j))
        d = np.tril(d) + np.tril(d, -1).T
        Lj = np.linalg.cholesky(d)
        Dinv = np.linalg.inv(Lj)
        blk(A, j, j)[...] = Dinv if with_inverse else Lj
        # panel solve, then the next diagonal tiles
        for i in range(j + 1, nb):
            blk(A, i, j)[...] = blk(A, i, j) @ Dinv.T
        # D_j: the NEXT diagonal tile only (its older window columns are hosted tile operations of launch j)
        if j + 1 < nb:
            blk(A, j + 1, j + 1)[...] -= blk(A, j + 1, j) @ blk(A, j + 1, j).T
    for l in sorted(k for k in by_launch if k >= nb):
        hosted(by_launch[l], A, Tm)
    want = np.linalg.inv(Lref) if with_inverse else Lref
    got = np.tril(A)
    if not with_inverse:
        # diagonal blocks hold the factor's block (lower)
        pass
    scale = np.abs(want).max()
    assert np.abs(got - want).max() < 1e-10 * scale, np.abs(got - want).max()
    return rec


@pytest.mark.parametrize("nb", [1, 2, 3, 5, 8, 10, 13, 33, 40])
def test_plan_with_inverse_small(ensure_built, nb):
    replay(nb, 2, 1, seed=nb)


@pytest.mark.parametrize("nb", [5, 33])
def test_plan_factor_only(ensure_built, nb):
    replay(nb, 2, 0, seed=nb)


@pytest.mark.parametrize("nb,with_inverse", [(67, 1), (96, 1), (128, 0), (130, 1)])
def test_plan_large(ensure_built, nb, with_inverse):
    """nb >= 64: the full-round hosting policy with per-tile pending ranges (and the inverse in the chain-bound tail)."""
    rec = replay(nb, 1, with_inverse, seed=nb)
    upd = rec[rec[:, 5] == 0]
    if nb >= 96:
        assert (upd[:, 4] - upd[:, 3]).max() >= 8        # deferred tiles come back deeper
    if with_inverse:
        hosted_inv = rec[(rec[:, 5] > 0) & (rec[:, 0] < nb)]
        assert len(hosted_inv) > 0                        # part of the inverse rides in the step launches


@pytest.mark.parametrize("nb", [10, 33, 47, 128])
def test_lists_are_dispatched_deepest_first(ensure_built, nb):
    """Dispatch order = list order.  A launch of more workgroups than the chip has slots packs two shallow chunks into one
    slot only if the deep ones go first: the list of every launch (trailing updates and the inverse's chunks together)
    is sorted by k-depth, deepest first (N = 4212: launches of 260-290 quadrants 49 -> 38 us when this was fixed)."""
    rec = plan(nb, 1)
    for launch in np.unique(rec[:, 0]):
        r = rec[rec[:, 0] == launch]
        depth = r[:, 4] - r[:, 3]
        assert (np.diff(depth) <= 0).all(), int(launch)


# ---- the plan of single-precision handles ------------------------------------------------------------------------------
def plan_f32(nb, with_inverse):
    """records (launch, ci, cj, kb0, kb1, kind) and the diagonal tiles per step; launch -(p + 1) = before panel p"""
    from gpim_amd import _lib
    lib = _lib.load()
    ip = ctypes.POINTER(ctypes.c_int32)
    n = ctypes.c_int64()
    assert lib.gpimhip_step_plan_host_f32(nb, with_inverse, None, 0, ctypes.byref(n), None) == 0
    buf = np.zeros((max(n.value, 1), 6), dtype=np.int32)
    diag = np.full(nb, -1, dtype=np.int32)
    assert lib.gpimhip_step_plan_host_f32(nb, with_inverse, buf.ctypes.data_as(ip), n.value, ctypes.byref(n),
                                          diag.ctypes.data_as(ip)) == 0
    return buf[:n.value], diag


def launch_f32(ops, A, Tm, bs):
    """One launch: every operation reads the state the launch started from; one matrix product over the whole k-range
    per operation (at 1x1 blocks the dot product of two row slices)."""
    nb = A.shape[0] // bs
    A0, T0 = A.copy(), Tm.copy()
    wrA, wrT = np.zeros((nb, nb), bool), np.zeros((nb, nb), bool)
    rdA, rdT = np.zeros((nb, nb), bool), np.zeros((nb, nb), bool)
    for ci, cj, k0, k1, kind in ops:
        assert 0 <= k0 < k1 <= nb and 0 <= cj <= ci < nb and 0 <= kind <= 4
        r, c, k = slice(ci * bs, (ci + 1) * bs), slice(cj * bs, (cj + 1) * bs), slice(k0 * bs, k1 * bs)
        wr = wrT if kind in (1, 2) else wrA
        assert not wr[ci, cj], "two operations of one launch write tile (%d, %d)" % (ci, cj)
        wr[ci, cj] = True
        rdA[ci, k0:k1] = True
        if kind == 0:
            rdA[cj, k0:k1] = True
            A[r, c] = A0[r, c] - A0[r, k] @ A0[c, k].T
        elif kind in (1, 2):
            rdA[k0:k1, cj] = True
            acc = A0[r, k] @ A0[k, c]
            Tm[r, c] = acc if kind == 1 else T0[r, c] + acc
        else:
            rdT[k0:k1, cj] = True
            acc = A0[r, k] @ T0[k, c]
            A[r, c] = -acc if kind == 3 else A0[r, c] - acc
    assert not (wrA & rdA).any() and not (wrT & rdT).any(), "an operation reads what another of the same launch writes"
    return wrA


def replay_f32(nb, bs, with_inverse, seed=0):
    rng = np.random.default_rng(seed)
    n = nb * bs
    G = rng.standard_normal((n, n))
    K = G @ G.T / n + 2.0 * np.eye(n)
    A = np.tril(K).copy()
    Tm = np.full((n, n), np.nan)
    rec, diag = plan_f32(nb, with_inverse)
    by_launch = {}
    for r in rec.tolist():
        by_launch.setdefault(r[0], []).append(tuple(r[1:]))
    blk = lambda M, i, j: M[i * bs:(i + 1) * bs, j * bs:(j + 1) * bs]
    W = 4
    for j in range(nb):
        if j % W == 0:
            # the launch before the panel's first step: trailing updates with the columns of finished panels
            ops = by_launch.get(-(j // W + 1), [])
            for o in ops:
                assert o[4] == 0 and o[3] <= j and o[1] >= j + W, o
            launch_f32(ops, A, Tm, bs)
        ops = by_launch.get(j, [])
        for o in ops:
            assert o[3] <= j or o[4] != 0, "a trailing update uses a block column that is not final"
        written = launch_f32(ops, A, Tm, bs)
        assert not written[j, j]
        # the factorisation role of the same launch touches block (j, j) only
        d = np.tril(blk(A, j, j))
        Lj = np.linalg.cholesky(d + np.tril(d, -1).T)
        Dinv = np.linalg.inv(Lj)
        blk(A, j, j)[...] = Dinv if with_inverse else Lj
        # F_j: the panel solve of column j
        A[(j + 1) * bs:, j * bs:(j + 1) * bs] = A[(j + 1) * bs:, j * bs:(j + 1) * bs] @ Dinv.T
        # D_j: the next diag[j] diagonal tiles receive column j
        assert 0 <= diag[j] <= nb - 1 - j
        for jj in range(j + 1, j + 1 + diag[j]):
            blk(A, jj, jj)[...] -= blk(A, jj, j) @ blk(A, jj, j).T
    assert min(by_launch, default=0) >= -((nb + W - 1) // W)          # launch -(p + 1): before panel p
    for l in sorted(k for k in by_launch if k >= nb):
        assert with_inverse
        launch_f32(by_launch[l], A, Tm, bs)
    Lref = np.linalg.cholesky(K)
    want = np.linalg.inv(Lref) if with_inverse else Lref
    got = np.tril(A)
    scale = np.abs(want).max()
    assert np.abs(got - want).max() < 1e-10 * scale, np.abs(got - want).max()
    return rec, diag


F32_CAP = {False: 128, True: 64}          # hosted bulk tiles per launch from 88 block columns / in pair mode (from 160)


@pytest.mark.parametrize("with_inverse", [0, 1])
@pytest.mark.parametrize("nb", [1, 2, 4, 5, 8, 9, 13, 33, 87, 88, 96, 159, 160, 161, 168])
def test_float_plan_replay(ensure_built, nb, with_inverse):
    """Block-column counts on both sides of every policy change of the float plan: everything hosted (< 88), capped fill
    and a launch before the panel's first step (88 .. 159), panels applied two at a time (>= 160)."""
    rec, diag = replay_f32(nb, 2 if nb <= 13 else 1, with_inverse, seed=nb)
    W = 4
    upd = rec[rec[:, 5] == 0]
    before = rec[rec[:, 0] < 0]
    # bulk tiles of a step launch: trailing updates of columns right of the window (the column update is column `launch`)
    step_upd = upd[upd[:, 0] >= 0]
    bulk = step_upd[step_upd[:, 2] != step_upd[:, 0]]
    assert (bulk[:, 2] >= (bulk[:, 0] // W) * W + W).all()
    per_launch = np.bincount(bulk[:, 0], minlength=nb) if len(bulk) else np.zeros(nb, int)
    # the window's diagonal tiles, eagerly: everything up to the end of the next panel
    for j in range(nb):
        assert diag[j] == max(0, min(nb, min((j // W) * W + W, nb) + W) - (j + 1))
    if nb < 88:
        assert len(before) == 0
    else:
        assert per_launch.max() <= F32_CAP[nb >= 160]
        assert len(before) > 0
    depth = np.append(upd[:, 4] - upd[:, 3], 0)
    if nb >= 160:
        assert depth.max() == 2 * W                      # a deferred tile comes back 8 block columns deep
    else:
        assert depth.max() <= 2 * W - 1                  # (the column update's window of two panels)
