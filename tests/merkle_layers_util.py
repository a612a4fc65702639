"""Shared by the GPU Merkle tests: commit a column layout through cm_merkle_commit_layers and compare the root and every node of
every stored layer with the oracle's merkle_commit, word for word."""
import ctypes as C

import numpy as np

from cairo_m_amd.lib import merkle_plan
from tests.merkle_op_shapes import TUNING_DEFAULTS

P = 2**31 - 1
CARVE_FROM = 64   # a size with more columns than this is one upload, its columns carved out of it


class tuned:
    """cm_set_tuning of the given (key, value) pairs for a with-block; the defaults come back in a finally"""
    def __init__(self, L, pairs):
        self.L, self.pairs = L, pairs

    def __enter__(self):
        try:
            for k, v in self.pairs:
                assert self.L.cm_set_tuning(k.encode(), C.c_int32(v)) == 0, (k, v)
        except BaseException:
            self.__exit__()
            raise

    def __exit__(self, *exc):
        for k, _ in self.pairs:
            self.L.cm_set_tuning(k.encode(), C.c_int32(TUNING_DEFAULTS[k]))


def random_columns(logs, seed):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, P, size=1 << l, dtype=np.uint32) for l in logs]


def upload_columns(backend, cols, logs):
    """(one handle per column, the handles to free).  The 4000-column shapes would cost one small allocation per column: the
    columns of a size that has many are carved out of one upload (a handle of this library is the column's device address)."""
    handles, owned = [None] * len(cols), []
    for l in sorted(set(logs)):
        idx = [i for i, x in enumerate(logs) if x == l]
        if len(idx) > CARVE_FROM:
            base = backend.upload(np.concatenate([cols[i] for i in idx]))
            owned.append(base)
            for k, i in enumerate(idx):
                handles[i] = base + 4 * (k << l)
        else:
            for i in idx:
                handles[i] = backend.upload(cols[i])
                owned.append(handles[i])
    return handles, owned


def layer_offsets(max_log):
    """word offset of layer l in the concatenation "largest first, 8 words per node\""""
    off, at = {}, 0
    for l in range(max_log, -1, -1):
        off[l] = at
        at += 8 << l
    assert at == ((2 << max_log) - 1) * 8
    return off


def first_difference(got, want, logs):
    """None, or a sentence naming the first differing layer (from the leaves down), its first differing node and the launch that
    wrote it according to cm_merkle_plan"""
    if got.size == want.size and np.array_equal(got, want):
        return None
    max_log = max(logs) if logs else 0
    if got.size != want.size:
        return f"{got.size} layer words, the oracle has {want.size}"
    off = layer_offsets(max_log)
    plan = merkle_plan(logs)
    for l in range(max_log, -1, -1):
        g = got[off[l]:off[l] + (8 << l)].reshape(-1, 8)
        w = want[off[l]:off[l] + (8 << l)].reshape(-1, 8)
        bad = np.flatnonzero((g != w).any(axis=1))
        if bad.size:
            r = next(r for r in plan if r["lo"] <= l <= r["hi"])
            how = f"{r['kind']} launch of layers {r['hi']}..{r['lo']}" + (" (wide path)" if l in r["wide"] else "")
            if r["kind"] == "narrow":
                how += f" <PREV={int(r['prev'])}, NC={r['nc']}> npw={r['npw']}"
            return (f"layer 2^{l} ({logs.count(l)} columns), written by the {how}: {bad.size} of {1 << l} nodes differ, the first is node "
                    f"{int(bad[0])}: got {g[bad[0]].tolist()}, the oracle has {w[bad[0]].tolist()}")
    raise AssertionError("unreachable")


def assert_all_layers_equal_oracle(backend, oracle, logs, seed):
    """returns (root, layers) of the HIP commitment after asserting both equal the oracle's"""
    logs = list(logs)
    cols = random_columns(logs, seed)
    handles, owned = upload_columns(backend, cols, logs)
    try:
        root, got = backend.merkle_commit_layers(handles, logs)
    finally:
        for h in owned:
            backend.col_free(h)
    want_root, want = oracle.merkle_commit(cols)
    diff = first_difference(got, want, logs)
    assert diff is None, diff
    assert root == want_root
    assert got[-8:].tobytes() == root   # the root IS layer 0
    return root, got
