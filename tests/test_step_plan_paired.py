"""The PAIRED step schedule of the blocked Cholesky with the fused inverse (cholstep.hip: plan_updates / plan_inverse with
`lead`; what a handle of at most four problems runs from 68 block columns) replayed on the HOST with 1x1 blocks, with the
semantics of the launches as they run:

  HH_j   every hosted operation reads the state the launch started from; the role workgroup factors block j, runs the bridge
         (L[j+1,j] = A[j+1,j] X_j^T, A[j+1,j+1] -= L[j+1,j] L[j+1,j]^T) and factors block j+1 -- it touches the tiles (j,j),
         (j+1,j), (j+1,j+1) only, which no hosted operation of the launch may read or write;
  FD2_j  the launch after it: L[i,j] = A[i,j] X_j^T and L[i,j+1] = (A[i,j+1] - L[i,j] L[j+1,j]^T) X_{j+1}^T for i >= j+2, and
         columns j, j+1 applied to the tiles (j+2,j+2), (j+3,j+2), (j+3,j+3) -- the records of kind 5.

Columns outside the bulk regime run one per launch (H_j, F_j, D_j) as tests/test_step_plan.py replays them.  No GPU involved."""
import ctypes

import numpy as np
import pytest

W = 4


def plan_paired(nb):
    from gpim_amd import _lib
    lib = _lib.load()
    ip = ctypes.POINTER(ctypes.c_int32)
    n = ctypes.c_int64()
    assert lib.gpimhip_step_plan_host_paired(nb, None, 0, ctypes.byref(n), None) == 0
    buf = np.zeros((max(n.value, 1), 6), dtype=np.int32)
    lead = np.full(nb, -1, dtype=np.int32)
    assert lib.gpimhip_step_plan_host_paired(nb, buf.ctypes.data_as(ip), n.value, ctypes.byref(n),
                                             lead.ctypes.data_as(ip)) == 0
    return buf[:n.value], lead


def plan_unpaired(nb):
    from gpim_amd import _lib
    lib = _lib.load()
    n = ctypes.c_int64()
    assert lib.gpimhip_step_plan_host(nb, 1, None, 0, ctypes.byref(n)) == 0
    buf = np.zeros((max(n.value, 1), 6), dtype=np.int32)
    assert lib.gpimhip_step_plan_host(nb, 1, buf.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), n.value,
                                      ctypes.byref(n)) == 0
    return buf[:n.value]


def hosted(ops, A, Tm, got, role_tiles):
    """One launch's hosted operations (kinds 0-4) on 1x1 blocks; got[ci, cj, k] counts the k-blocks a tile has received."""
    A0, T0 = A.copy(), Tm.copy()
    written, reads = set(), set()
    for ci, cj, k0, k1, kind in ops:
        assert 0 <= k0 < k1 and cj <= ci and 0 <= kind <= 4
        dst = ("T" if kind in (1, 2) else "A", ci, cj)
        assert dst not in written, "two operations of one launch write %s" % (dst,)
        written.add(dst)
        k = slice(k0, k1)
        if kind == 0:
            reads.update(("A", ci, c) for c in range(k0, k1))
            reads.update(("A", cj, c) for c in range(k0, k1))
            A[ci, cj] = A0[ci, cj] - A0[ci, k] @ A0[cj, k]
            got[ci, cj, k] += 1
        elif kind in (1, 2):
            reads.update(("A", ci, c) for c in range(k0, k1))
            reads.update(("A", c, cj) for c in range(k0, k1))
            acc = A0[ci, k] @ A0[k, cj]
            Tm[ci, cj] = acc if kind == 1 else T0[ci, cj] + acc
        else:
            reads.update(("A", ci, c) for c in range(k0, k1))
            reads.update(("T", c, cj) for c in range(k0, k1))
            acc = A0[ci, k] @ T0[k, cj]
            A[ci, cj] = -acc if kind == 3 else A0[ci, cj] - acc
    assert not (written & reads), "an operation reads what another operation of the same launch writes"
    role = {("A", i, j) for i, j in role_tiles}
    assert not (written & role) and not (reads & role), "a hosted operation touches a tile of the factorisation role"


def replay(nb, seed=0):
    rng = np.random.default_rng(seed)
    G = rng.standard_normal((nb, nb))
    K = G @ G.T / nb + 2.0 * np.eye(nb)
    A = np.tril(K).copy()
    Tm = np.full((nb, nb), np.nan)
    rec, lead = plan_paired(nb)
    by_launch, fd2 = {}, {}
    for r in rec.tolist():
        (fd2 if r[5] == 5 else by_launch).setdefault(r[0], []).append(tuple(r[1:]))
    got = np.zeros((nb, nb, nb), dtype=np.int64)
    j = 0
    while j < nb:
        ops = by_launch.get(j, [])
        for o in ops:
            assert o[4] != 0 or (o[3] <= j and o[1] >= j), "a trailing update uses a block column that is not final"
        if lead[j] == 1:
            assert j + 3 < nb and lead[j + 1] == 2 and (j + 1) not in by_launch and (j + 1) not in fd2
            hosted(ops, A, Tm, got, [(j, j), (j + 1, j), (j + 1, j + 1)])
            # role j, bridge, role j+1
            X0 = 1.0 / np.sqrt(A[j, j])
            A[j, j] = X0
            A[j + 1, j] *= X0
            A[j + 1, j + 1] -= A[j + 1, j] * A[j + 1, j]
            got[j + 1, j + 1, j] += 1
            X1 = 1.0 / np.sqrt(A[j + 1, j + 1])
            A[j + 1, j + 1] = X1
            # FD2_j
            want = {(i, j + 1, j, j + 1, 5) for i in range(j + 2, nb)}
            want |= {(j + 2, j + 2, j, j + 2, 5), (j + 3, j + 2, j, j + 2, 5), (j + 3, j + 3, j, j + 2, 5)}
            assert set(fd2.get(j, [])) == want and len(fd2[j]) == len(want)
            A[j + 2:, j] *= X0
            A[j + 2:, j + 1] -= A[j + 2:, j] * A[j + 1, j]
            got[j + 2:, j + 1, j] += 1
            A[j + 2:, j + 1] *= X1
            for ci, cj in ((j + 2, j + 2), (j + 3, j + 2), (j + 3, j + 3)):
                A[ci, cj] -= A[ci, j:j + 2] @ A[cj, j:j + 2]
                got[ci, cj, j:j + 2] += 1
            j += 2
        else:
            assert lead[j] == 0 and j not in fd2
            hosted(ops, A, Tm, got, [(j, j)])
            X0 = 1.0 / np.sqrt(A[j, j])
            A[j, j] = X0
            A[j + 1:, j] *= X0
            if j + 1 < nb:
                A[j + 1, j + 1] -= A[j + 1, j] * A[j + 1, j]
                got[j + 1, j + 1, j] += 1
            j += 1
    for l in sorted(k for k in by_launch if k >= nb):
        hosted(by_launch[l], A, Tm, got, [])
    # every tile has received each k-block left of it exactly once
    expect = np.zeros_like(got)
    for cj in range(nb):
        expect[cj:, cj, :cj] = 1
    assert (got == expect).all(), np.argwhere(got != expect)[:5]
    want = np.linalg.inv(np.linalg.cholesky(K))
    scale = np.abs(want).max()
    assert np.abs(np.tril(A) - want).max() < 1e-10 * scale, np.abs(np.tril(A) - want).max()
    return rec, lead


@pytest.mark.parametrize("nb", [68, 72, 76, 77, 96, 128, 130])
def test_paired_plan_replay(ensure_built, nb):
    """68: one bulk panel, windows starting at 0; 76: three, windows two panels back and deadline tiles; 77 / 130: a panel
    of fewer than four columns at the end; 128: the headline."""
    rec, lead = replay(nb, seed=nb)
    # the pairs: both halves of every panel that leaves at least 64 block columns right of it
    for j in range(nb):
        p0 = (j // W) * W
        bulk = nb - p0 - W >= 64
        assert lead[j] == ((1 if (j - p0) % 2 == 0 else 2) if bulk else 0), j
    assert lead[0] == 1
    # dispatch order = list order: deepest first (test_step_plan.py: test_lists_are_dispatched_deepest_first)
    run = rec[rec[:, 5] != 5]
    for launch in np.unique(run[:, 0]):
        depth = (run[run[:, 0] == launch][:, 4] - run[run[:, 0] == launch][:, 3])
        assert (np.diff(depth) <= 0).all(), int(launch)
    # part of the inverse rides in the step launches (pair leaders included once the tree has finished nodes left of them)
    hosted_inv = run[(run[:, 5] > 0) & (run[:, 0] < nb)]
    assert len(hosted_inv) > 0
    if nb >= 72:
        assert (lead[hosted_inv[:, 0]] == 1).any()


@pytest.mark.parametrize("nb", [1, 5, 33, 64, 67])
def test_paired_export_below_the_bulk_regime(ensure_built, nb):
    """No panel of fewer than 68 block columns is in the bulk regime: the per-column plan, record for record."""
    rec, lead = plan_paired(nb)
    assert (lead == 0).all()
    assert np.array_equal(rec, plan_unpaired(nb))
