"""Reference of the link diff (cm_link_diff), in numpy, written from the cm_memory_cell rows alone: (address, value[4], clock,
multiplicity), ascending address.  Shared by tests/test_run_check_abi.py and tests/test_gpu_run_check.py; it never calls the
product's diff.

Rule: only a cell's four value words are leaves of the partial Merkle tree, and an absent leaf hashes like a zero leaf
(adapter/merkle.rs fills missing nodes with default hashes, the default leaf being 0).  So a cell present on one side only with
value (0, 0, 0, 0) cannot change the root: it is counted as zero-only and not listed."""
import numpy as np


def link_diff_ref(prev_final, next_initial):
    """prev_final / next_initial: (n, 7) u32 rows.  Returns (cells, totals): cells (k, 11) u32 = kind, address, prev_value[4],
    next_value[4], prev_clock in ascending address order (kind 1 changed, 2 only in next, 3 only in prev); totals = dict of
    n_changed, n_only_next, n_only_prev, n_zero_only."""
    a = np.asarray(prev_final, dtype=np.uint32).reshape(-1, 7)
    b = np.asarray(next_initial, dtype=np.uint32).reshape(-1, 7)
    assert (np.diff(a[:, 0].astype(np.int64)) > 0).all() and (np.diff(b[:, 0].astype(np.int64)) > 0).all()
    _, ia, ib = np.intersect1d(a[:, 0], b[:, 0], assume_unique=True, return_indices=True)
    changed = (a[ia, 1:5] != b[ib, 1:5]).any(axis=1)
    only_a = np.ones(len(a), dtype=bool)
    only_a[ia] = False
    only_b = np.ones(len(b), dtype=bool)
    only_b[ib] = False
    nz_a, nz_b = a[:, 1:5].any(axis=1), b[:, 1:5].any(axis=1)
    recs = []
    for i, j in zip(ia[changed], ib[changed]):
        recs.append([1, a[i, 0], *a[i, 1:5], *b[j, 1:5], a[i, 5]])
    for j in np.nonzero(only_b & nz_b)[0]:
        recs.append([2, b[j, 0], 0, 0, 0, 0, *b[j, 1:5], 0])
    for i in np.nonzero(only_a & nz_a)[0]:
        recs.append([3, a[i, 0], *a[i, 1:5], 0, 0, 0, 0, a[i, 5]])
    cells = np.array(recs, dtype=np.uint32).reshape(-1, 11)
    cells = cells[np.argsort(cells[:, 1], kind="stable")]
    totals = {"n_changed": int(changed.sum()), "n_only_next": int((only_b & nz_b).sum()), "n_only_prev": int((only_a & nz_a).sum()),
              "n_zero_only": int((only_a & ~nz_a).sum() + (only_b & ~nz_b).sum())}
    return cells, totals
