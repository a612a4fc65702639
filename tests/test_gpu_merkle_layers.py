"""Every stored layer of the Merkle commitment, word for word against the oracle (no tolerance).

k_merkle_multi, k_merkle_tail and both phases of k_merkle_top hash each parent from an LDS copy of its children and write the
layer to HBM in a separate store, so the root proves nothing about the stored layers — and the decommitment gathers its hash
witnesses from exactly those.  cm_merkle_commit_layers reads the tree's own layer buffers back; the shapes of
tests/merkle_op_shapes.py reach every variant of the six kernels (tests/test_merkle_plan_cpu.py proves that on the CPU and pins
which kernel runs).  The fold and transcript extras of k_merkle_top (fold_mode 1 / 2, chan) have no op-level entry: whole-proof
parity covers them, these tests do not.

Measured on an MI355X: the 61 cases of this module take under 3 s together; the slowest, tail_wide_5_3_0 (712 columns), 0.18 s."""
import numpy as np
import pytest

from cairo_m_amd.lib import merkle_layer_npw, merkle_plan, set_framing
from tests.merkle_layers_util import assert_all_layers_equal_oracle, random_columns, tuned
from tests.merkle_op_shapes import MERKLE_OP_SHAPES, NARROW_LAYER_FORMS, NARROW_LAYER_LOG, NPW_AT_2_14, RFC_SHAPES

pytestmark = pytest.mark.gpu

POISON = 0xDEADBEEF   # no hash word of these inputs; not a canonical M31 either


@pytest.mark.parametrize("logs,tuning", [(s, t) for _, s, t in MERKLE_OP_SHAPES], ids=[i for i, _, _ in MERKLE_OP_SHAPES])
def test_every_stored_layer_equals_the_oracle(backend, oracle, logs, tuning):
    """The root and every node of every layer, for every shape of tests/merkle_op_shapes.py; tuned shapes hold their keys through
    cm_set_tuning for the commitment only.  A mismatch names the layer, its first differing node and the launch that wrote it.
    The largest input is narrow_natural_npw2 ([21] * 4: 32 MB of columns, 4 M nodes hashed by the oracle): 0.16 s."""
    with tuned(backend.L, tuning):
        assert_all_layers_equal_oracle(backend, oracle, logs, seed=8000 + len(logs))


@pytest.mark.parametrize("name", RFC_SHAPES)
def test_every_stored_layer_under_rfc_node_framing(backend, oracle, name):
    """hash_node=rfc (NodeFrame<true>: the other instantiation of every kernel) on one shape per kernel kind, the wide paths of
    the tail, the top kernel's phase 2 and the quad kernel included; the oracle runs under the same switch."""
    logs, tuning = next((s, t) for i, s, t in MERKLE_OP_SHAPES if i == name)
    try:
        set_framing("hash_node=rfc", backend.L)
        oracle.set_framing("hash_node=rfc")
        with tuned(backend.L, tuning):
            root, _ = assert_all_layers_equal_oracle(backend, oracle, logs, seed=8100 + len(logs))
    finally:
        set_framing("", backend.L)
        oracle.set_framing("")
    # and the switch does something: the default framing gives another root for the same columns
    want_default, _ = oracle.merkle_commit(random_columns(logs, 8100 + len(logs)))
    assert root != want_default


@pytest.fixture(scope="module")
def narrow_reference(oracle):
    """columns and oracle layers for the three narrow forms at 2^14, computed once: (columns here, child hashes or None,
    expected hashes) by (n_cols, with_prev)"""
    L = NARROW_LAYER_LOG
    rng = np.random.default_rng(1414)
    upper = [rng.integers(0, 2**31 - 1, size=2 << L, dtype=np.uint32) for _ in range(2)]
    here = [rng.integers(0, 2**31 - 1, size=1 << L, dtype=np.uint32) for _ in range(4)]
    ref = {}
    for n_cols, with_prev in NARROW_LAYER_FORMS:
        cols = (upper if with_prev else []) + here[:n_cols]
        _, layers = oracle.merkle_commit(cols)
        if with_prev:
            children, want = layers[: 16 << L], layers[16 << L: (16 << L) + (8 << L)]
        else:
            children, want = None, layers[: 8 << L]
        want.setflags(write=False)
        ref[(n_cols, with_prev)] = (here[:n_cols], children, want)
    return ref


@pytest.mark.parametrize("npw", [1, 2, 3, 4, 5, 6, 7, 8, 0])
@pytest.mark.parametrize("n_cols,with_prev", NARROW_LAYER_FORMS, ids=["children_only", "children_and_4", "leaf_4"])
def test_commit_layer_at_2_14_under_every_npw(backend, narrow_reference, n_cols, with_prev, npw):
    """cm_merkle_commit_layer at 2^14 nodes, the smallest size merkle_layer() hands to k_merkle_narrow, for its three <PREV, NC>
    forms under every merkle_npw: 2 / 4 / 8 and 5 (halved to 2) walk several chunks per wave, so the next chunk's prefetch runs;
    3, 6 and 7 halve down to 1; 0 is k_merkle_layer.  Which of them runs is asserted, not assumed (cm_merkle_layer_npw reads the
    predicate merkle_layer() launches by), and the output starts as poison: a node the kernel skips cannot pass for one it wrote."""
    L = NARROW_LAYER_LOG
    here, children, want = narrow_reference[(n_cols, with_prev)]
    hs = [backend.upload(c) for c in here]
    prev = backend.upload(children) if with_prev else 0
    out = backend.upload(np.full(8 << L, POISON, dtype=np.uint32))
    try:
        with tuned(backend.L, [("merkle_npw", npw)]):
            assert merkle_layer_npw(L, with_prev, n_cols, backend.L) == NPW_AT_2_14[npw]
            backend.merkle_commit_layer(L, prev, hs, out)
        got = backend.download(out, 8 << L)
    finally:
        for h in hs + [out] + ([prev] if prev else []):
            backend.col_free(h)
    assert not (got == POISON).any(), f"{int((got == POISON).sum())} words were never written"
    bad = np.flatnonzero((got.reshape(-1, 8) != want.reshape(-1, 8)).any(axis=1))
    assert bad.size == 0, f"{bad.size} of {1 << L} nodes differ, the first is node {int(bad[0])} (chunk {int(bad[0]) // 64})"


def test_a_wrong_layer_is_named(backend, oracle):
    """the comparison itself: a flipped word in a stored layer is reported with its layer, node and launch kind"""
    from tests.merkle_layers_util import first_difference, layer_offsets
    logs = [10] * 3 + [4] * 2
    cols = random_columns(logs, 5)
    _, want = oracle.merkle_commit(cols)
    assert first_difference(want.copy(), want, logs) is None
    bad = want.copy()
    bad[layer_offsets(10)[6] + 8 * 5 + 3] ^= 1
    msg = first_difference(bad, want, logs)
    assert "layer 2^6" in msg and "first is node 5" in msg and "top launch of layers 10..0" in msg, msg
    assert merkle_plan(logs)[0]["kind"] == "top"
