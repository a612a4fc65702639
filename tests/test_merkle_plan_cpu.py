"""Which Merkle kernel hashes which layers (no GPU: cm_merkle_plan and cm_merkle_layer_npw are host code, MerkleTree::plan_commit
consumes the records the first returns and merkle_layer() calls the predicate behind the second, and the wide-path flags come
from the functions the kernels evaluate).  The plan of every shape the GPU op tests commit (tests/merkle_op_shapes.py), of the
twelve shapes of test_merkle_commit_parity and of the four commitment trees of fib(3000) is pinned to a table written out by
hand; so are merkle_multi_top at both ends, merkle_npw 0..8 at 2^14 and 2^21 and, in a child process (the switch is read once),
CM_NO_MERKLE_TOP=1.  The records of tests/merkle_op_shapes.py must together contain every feature of FEATURES: after a change
of the planner or a new kernel variant this fails here, on the CPU, until a shape reaches the new variant.

Not reached by any op shape, on purpose: the fold and transcript extras of k_merkle_top (fold_mode 1 / 2, chan), which only the
FRI phase sets; whole-proof parity covers them."""
import ctypes as C
import json
import os
import subprocess
import sys

import pytest

from cairo_m_amd.lib import CmError, load_library, merkle_layer_npw, merkle_plan
from tests.merkle_op_shapes import (COMMIT_PARITY_SHAPES, MERKLE_OP_SHAPES, NARROW_LAYER_FORMS, NARROW_LAYER_LOG, NO_TOP_SHAPES,
                                    NPW_AT_2_14, NPW_AT_2_21, RFC_SHAPES, TUNING_DEFAULTS)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class tuned:
    """cm_set_tuning of the given (key, value) pairs for a with-block; the defaults come back afterwards"""
    def __init__(self, pairs):
        self.pairs, self.L = pairs, load_library()

    def __enter__(self):
        for k, v in self.pairs:
            assert self.L.cm_set_tuning(k.encode(), C.c_int32(v)) == 0, (k, v)

    def __exit__(self, *exc):
        for k, _ in self.pairs:
            assert self.L.cm_set_tuning(k.encode(), C.c_int32(TUNING_DEFAULTS[k])) == 0, k


# ---- the hand-written table: one tuple per launch -------------------------------------------------------------------------
def _spread(hi, lo, cols):
    """{layer: columns} -> the column count of every layer hi .. lo"""
    assert all(lo <= l <= hi for l in cols), (hi, lo, cols)
    return [cols.get(l, 0) for l in range(hi, lo - 1, -1)]


def layer(log, prev, n):
    return ("layer", log, log, bool(prev), [n], [])


def narrow(log, prev, nc, npw):
    return ("narrow", log, log, bool(prev), [nc], [], bool(prev), nc, npw)


def quad(log, prev, n, wide=True):
    return ("quad", log, log, bool(prev), [n], [log] if wide else [])


def multi(hi, lo, prev, ncols):
    assert len(ncols) == hi - lo + 1
    return ("multi", hi, lo, bool(prev), list(ncols), [])


def top(hi, prev, cols=None, wide=()):
    return ("top", hi, 0, bool(prev), _spread(hi, 0, cols or {}), list(wide))


def tail(hi, prev, cols=None, wide=()):
    return ("tail", hi, 0, bool(prev), _spread(hi, 0, cols or {}), list(wide))


def _narrow_forms(npw):
    return [narrow(19, 0, 4, npw), narrow(18, 1, 0, npw), narrow(17, 1, 4, npw), top(16, 1)]


_LAYER_9 = lambda k: [quad(10, 0, 64), layer(9, 1, k), tail(8, 1, {1: 64}, wide=[1])]   # noqa: E731

OP_SHAPE_PLANS = {
    "tail_wide_5_3_0": [tail(8, 0, {8: 16, 7: 17, 5: 48, 4: 47, 3: 129, 0: 50}, wide=[5, 3, 0])],
    "tail_wide_8_6_5_cap": [tail(8, 0, {8: 49, 6: 65, 5: 2048, 2: 2049}, wide=[8, 6, 5])],
    "tail_from_6": [tail(6, 0, {6: 48, 3: 3}, wide=[6])],
    "quad_leaf_then_tail": [quad(9, 0, 64), tail(8, 1, {8: 48}, wide=[8])],
    "quad_groups": [quad(12, 0, 64), quad(11, 1, 65), quad(10, 1, 128), quad(9, 1, 443), tail(8, 1)],
    "quad_fallback_then_top2": [quad(10, 0, 2049, wide=False), top(9, 1)],
    "layer_0_cols": _LAYER_9(0),
    "layer_15_cols": _LAYER_9(15),
    "layer_16_cols": _LAYER_9(16),
    "layer_17_cols": _LAYER_9(17),
    "group_of_one": [layer(13, 0, 5), quad(12, 1, 64), top(11, 1)],
    "layer_4_cols_below_narrow": [layer(13, 0, 4), quad(12, 1, 64), top(11, 1)],
    "multi_2_levels": [multi(14, 13, 0, [3, 1]), quad(12, 1, 64), top(11, 1)],
    "multi_3_levels": [multi(15, 13, 0, [2, 0, 17]), quad(12, 1, 64), top(11, 1)],
    "multi_4_levels_then_top": [multi(18, 15, 0, [1, 16, 17, 1]), top(14, 1, {14: 33})],
    "multi_with_prev": [layer(19, 0, 1), multi(18, 15, 1, [0, 2, 0, 0]), top(14, 1)],
    "top256_phase2_wide": [top(16, 0, {16: 1, 6: 48, 5: 130, 0: 49}, wide=[6, 5, 0])],
    "top2_phase2_wide_root": [top(9, 0, {9: 63, 0: 48}, wide=[0])],
    "top_every_layer": [top(16, 0, {l: 1 for l in range(17)})],
    "narrow_natural_npw2": [narrow(21, 0, 4, 2), narrow(20, 1, 0, 1), narrow(19, 1, 0, 1), multi(18, 15, 1, [0, 0, 0, 0]), top(14, 1)],
    "multi_top_17": [narrow(18, 0, 4, 1), narrow(17, 1, 0, 1), top(16, 1)],
    "multi_top_23": [multi(20, 17, 0, [3, 18, 0, 0]), top(16, 1)],
    "narrow_forms_npw8": _narrow_forms(8),
    "narrow_forms_npw4": _narrow_forms(4),
    "narrow_forms_npw2": _narrow_forms(2),
    "narrow_forms_npw1": _narrow_forms(1),
    "narrow_forms_off": [layer(19, 0, 4), layer(18, 1, 0), layer(17, 1, 4), top(16, 1)],
}

# tests/test_gpu_poly_merkle.py::test_merkle_commit_parity, in its order
COMMIT_PARITY_PLANS = [
    [tail(6, 0, {6: 3})],
    [tail(8, 0, {8: 17, 5: 3, 3: 1})],
    [top(10, 0, {10: 40, 9: 16, 4: 5})],
    [tail(1, 0, {1: 1})],
    [top(12, 0, {12: 1, 3: 1})],
    [multi(17, 14, 0, [3, 2, 0, 0]), top(13, 1, {13: 5, 9: 2, 7: 20, 5: 3, 2: 1})],
    [top(16, 0, {16: 4})],
    [top(9, 0, {9: 33})],
    [multi(15, 12, 0, [2, 0, 0, 0]), quad(11, 1, 70), top(10, 1, {6: 3})],
    [layer(20, 0, 3), layer(19, 1, 18), multi(18, 15, 1, [0, 0, 0, 0]), top(14, 1, {12: 2})],
    [narrow(19, 0, 4, 1), multi(18, 15, 1, [0, 0, 0, 0]), top(14, 1)],
    [layer(21, 0, 1), layer(20, 1, 42), layer(19, 1, 1), multi(18, 15, 1, [0, 0, 0, 0]), top(14, 1)],
]

# The four commitment trees of fib(3000) at blowup 1.  Component log sizes (claim order): 4 4 12 13 4 12 13 14, eighteen idle
# opcode components at 4, then 6 9 4 9 8 16 20 18; a component's trace and interaction columns are committed at log + 1, the
# seven preprocessed columns at 18 18 18 18 8 16 20 plus 1, the four composition columns at max + 2.  {log: columns} per tree:
FIB3000_TREES = [
    {21: 1, 19: 4, 17: 1, 9: 1},
    {21: 1, 19: 1, 17: 1, 15: 18, 14: 32, 13: 16, 10: 453, 9: 1, 7: 9, 5: 474},
    {21: 4, 19: 4, 17: 4, 15: 24, 14: 44, 13: 28, 10: 16, 9: 4, 7: 12, 5: 1040},
    {22: 4},
]
FIB3000_PLANS = [
    [layer(21, 0, 1), narrow(20, 1, 0, 1), narrow(19, 1, 4, 1), multi(18, 15, 1, [0, 1, 0, 0]), top(14, 1, {9: 1})],
    # the 453 poseidon2 columns at 2^10 keep the top launch out: fused groups, the quad kernel, one layer, the tail (wide at 5)
    [layer(21, 0, 1), narrow(20, 1, 0, 1), layer(19, 1, 1), multi(18, 15, 1, [0, 1, 0, 18]), multi(14, 11, 1, [32, 16, 0, 0]),
     quad(10, 1, 453), layer(9, 1, 1), tail(8, 1, {7: 9, 5: 474}, wide=[5])],
    [narrow(21, 0, 4, 2), narrow(20, 1, 0, 1), narrow(19, 1, 4, 1), multi(18, 15, 1, [0, 4, 0, 24]),
     top(14, 1, {14: 44, 13: 28, 10: 16, 9: 4, 7: 12, 5: 1040}, wide=[5])],
    [narrow(22, 0, 4, 4), narrow(21, 1, 0, 2), narrow(20, 1, 0, 1), narrow(19, 1, 0, 1), multi(18, 15, 1, [0, 0, 0, 0]), top(14, 1)],
]

# CM_NO_MERKLE_TOP=1: NO_TOP_SHAPES and [9] * 33, a leaf layer the default plan gives to the top launch
NO_TOP_PLANS = [
    [multi(16, 13, 0, [4, 0, 0, 0]), multi(12, 9, 1, [0, 0, 3, 0]), tail(8, 1, {4: 50}, wide=[4])],
    [multi(11, 9, 0, [5, 0, 0]), tail(8, 1)],
    [multi(10, 9, 0, [40, 16]), tail(8, 1, {4: 5})],
    [layer(9, 0, 33), tail(8, 1)],
]
NO_TOP_EXTRA_SHAPES = [COMMIT_PARITY_SHAPES[7]]


def as_tuples(plan):
    """merkle_plan's dicts in the table's form; first_col must be the running column count"""
    out, seen = [], 0
    for r in plan:
        assert r["first_col"] == seen, r
        seen += sum(r["ncols"])
        t = (r["kind"], r["hi"], r["lo"], r["has_prev"], r["ncols"], r["wide"])
        if r["kind"] == "narrow":
            t += (r["prev"], r["nc"], r["npw"])
        out.append(t)
    return out


def expand(tree):
    return [l for l, n in tree.items() for _ in range(n)]


def _assert_default_environment():
    assert "CM_NO_MERKLE_TOP" not in os.environ, "unset CM_NO_MERKLE_TOP: this test pins the default plan"
    assert "CM_MERKLE_NPW" not in os.environ and "CM_MERKLE_MULTI_TOP" not in os.environ, "unset the Merkle tuning variables"


def test_op_shape_plans_equal_the_table():
    _assert_default_environment()
    assert [i for i, _, _ in MERKLE_OP_SHAPES] == list(OP_SHAPE_PLANS), "a shape of tests/merkle_op_shapes.py without a pinned plan"
    for name, logs, tuning in MERKLE_OP_SHAPES:
        with tuned(tuning):
            assert as_tuples(merkle_plan(logs)) == OP_SHAPE_PLANS[name], name
    assert set(RFC_SHAPES) <= set(OP_SHAPE_PLANS)


def test_commit_parity_and_fib3000_plans_equal_the_table():
    _assert_default_environment()
    for k, (logs, want) in enumerate(zip(COMMIT_PARITY_SHAPES, COMMIT_PARITY_PLANS)):
        assert as_tuples(merkle_plan(logs)) == want, k
    for k, (tree, want) in enumerate(zip(FIB3000_TREES, FIB3000_PLANS)):
        assert as_tuples(merkle_plan(expand(tree))) == want, k


def test_plan_does_not_depend_on_the_order_of_the_columns_and_covers_every_layer_once():
    _assert_default_environment()
    for logs in [s for _, s, t in MERKLE_OP_SHAPES if not t] + COMMIT_PARITY_SHAPES:
        plan = merkle_plan(logs)
        assert as_tuples(merkle_plan(sorted(logs))) == as_tuples(plan) == as_tuples(merkle_plan(logs[::-1]))
        assert plan[0]["hi"] == max(logs) and plan[-1]["lo"] == 0 and not plan[0]["has_prev"]
        assert all(a["lo"] == b["hi"] + 1 and b["has_prev"] for a, b in zip(plan, plan[1:]))
        for r in plan:
            assert r["ncols"] == [logs.count(l) for l in range(r["hi"], r["lo"] - 1, -1)]
    assert as_tuples(merkle_plan([])) == [tail(0, 0)]
    with pytest.raises(CmError):
        merkle_plan([32])


def test_multi_top_at_both_ends():
    """merkle_multi_top = the first layer size that gets a launch of its own instead of a fused group (17..23, default 19)"""
    _assert_default_environment()
    big = [23] + [22] + [21] + [17] * 2
    lone = lambda l, n: layer(l, l < 23, n) if n else narrow(l, 1, 0, 1)   # noqa: E731
    with tuned([("merkle_multi_top", 17)]):
        assert as_tuples(merkle_plan(big)) == [layer(23, 0, 1), layer(22, 1, 1), layer(21, 1, 1), narrow(20, 1, 0, 1), narrow(19, 1, 0, 1),
                                               narrow(18, 1, 0, 1), layer(17, 1, 2), top(16, 1)]
    assert as_tuples(merkle_plan(big)) == [lone(23, 1), lone(22, 1), lone(21, 1), lone(20, 0), lone(19, 0), multi(18, 15, 1, [0, 2, 0, 0]),
                                           top(14, 1)]
    with tuned([("merkle_multi_top", 23)]):
        assert as_tuples(merkle_plan(big)) == [layer(23, 0, 1), multi(22, 19, 1, [1, 1, 0, 0]), multi(18, 15, 1, [0, 2, 0, 0]), top(14, 1)]
    L = load_library()
    for bad in (16, 24):
        assert L.cm_set_tuning(b"merkle_multi_top", C.c_int32(bad)) != 0


def test_npw_at_2_14_and_2_21():
    """merkle_npw: 0 = k_merkle_layer, k > 0 = k chunks per wave, halved until 256 * k divides the layer; -1 (default) = by the
    layer's size.  2^14 only through cm_merkle_layer_npw (no commitment hands a 2^14 layer to merkle_layer() alone), 2^21 also
    through the plan of [21] * 4."""
    _assert_default_environment()
    assert sorted(NPW_AT_2_14) == sorted(NPW_AT_2_21) == list(range(-1, 9))
    for key in range(-1, 9):
        with tuned([("merkle_npw", key)]):
            for nc, prev in NARROW_LAYER_FORMS:
                assert merkle_layer_npw(NARROW_LAYER_LOG, prev, nc) == NPW_AT_2_14[key], (key, nc, prev)
                assert merkle_layer_npw(21, prev, nc) == NPW_AT_2_21[key], (key, nc, prev)
                assert merkle_layer_npw(13, prev, nc) == 0          # below 2^14: k_merkle_layer whatever the key
            for nc, prev in [(0, False), (1, True), (3, False), (5, True), (8, True), (16, False), (17, True)]:
                assert merkle_layer_npw(NARROW_LAYER_LOG, prev, nc) == 0, (key, nc, prev)   # not a narrow layer
            first = as_tuples(merkle_plan([21] * 4))[0]
            assert first == (narrow(21, 0, 4, NPW_AT_2_21[key]) if key else layer(21, 0, 4)), key
    for log, want in [(14, 1), (19, 1), (20, 1), (21, 2), (22, 4), (23, 8), (24, 8)]:
        assert merkle_layer_npw(log, True, 0) == want, log
    L = load_library()
    for bad in (-2, 9):
        assert L.cm_set_tuning(b"merkle_npw", C.c_int32(bad)) != 0


def test_no_merkle_top_in_a_child_process():
    """CM_NO_MERKLE_TOP=1 is a function-local static, read once: a child.  No record is a top launch; what the default plan
    gives to k_merkle_top becomes fused groups and a tail with a previous layer."""
    shapes = NO_TOP_SHAPES + NO_TOP_EXTRA_SHAPES
    code = ("import json, sys; from cairo_m_amd.lib import merkle_plan; "
            "print(json.dumps([merkle_plan(s) for s in json.loads(sys.argv[1])]))")
    r = subprocess.run([sys.executable, "-c", code, json.dumps(shapes)], cwd=ROOT, env=dict(os.environ, CM_NO_MERKLE_TOP="1"),
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    plans = json.loads(r.stdout.strip().splitlines()[-1])
    assert len(plans) == len(NO_TOP_PLANS)
    for k, (plan, want) in enumerate(zip(plans, NO_TOP_PLANS)):
        assert as_tuples(plan) == want, k


# ---- coverage: what the op shapes must reach --------------------------------------------------------------------------------
def _chunk_class(n):
    """a column count as the 16-column chunk loops see it"""
    return "0" if n == 0 else "1..15" if n < 16 else "16" if n == 16 else "17+"


def features_of(plan, tuning):
    """the features (FEATURES below) the launches of one plan reach"""
    f = set()
    for r in plan:
        kind, hi, lo, prev, ncols, wide = r["kind"], r["hi"], r["lo"], r["has_prev"], r["ncols"], r["wide"]
        pv = "prev" if prev else "no prev"
        f.add((kind, pv))
        if kind == "layer":
            n = ncols[0]
            f.add(("layer", "z16 branch below 2^14") if n == 4 and hi < 14 else ("layer", "cols " + _chunk_class(n)))
        elif kind == "narrow":
            f.add(("narrow", r["prev"], r["nc"], r["npw"]))
        elif kind == "quad":
            n = ncols[0]
            if not wide:
                f.add(("quad", "fallback above 2048 columns"))
            else:   # 64 nodes x 16 words per thread: groups of 64 columns
                f.add(("quad", "lds one group") if n <= 64 else ("quad", "lds group plus one column") if n == 65 else ("quad", "lds several groups"))
        elif kind == "multi":
            f.add(("multi", "levels", hi - lo + 1))
            for lv, n in enumerate(ncols):
                if n:
                    f.add(("multi", "columns at level", lv))
                    f.add(("multi", "column count", {16: "16", 17: "17", 1: "1"}.get(n, "other")))
        elif kind == "top":
            f.add(("top", "blocks", 1 << (hi - 8)))
            for k, n in enumerate(ncols):
                if n:
                    f.add(("top", "columns at", "lane-per-node level" if k <= 1 else "quad level" if k <= 8 else "phase 2"))
            if hi - 9 == 7:
                f.add(("top", "phase 2 first layer of 128 nodes"))
            if wide:
                f.add(("top", "phase 2 wide"))
        elif kind == "tail":
            f.add(("tail", "top_log 8" if hi == 8 else "top_log below 8"))
            for l in wide:
                f.add(("tail", "wide at", "l = 8" if l == 8 else "l = 0" if l == 0 else "a middle layer"))
            if any(n == 47 for n in ncols) and 47 not in [ncols[hi - l] for l in wide]:
                f.add(("tail", "not wide at 47 columns"))
    for k, v in tuning:
        if k == "merkle_multi_top":
            f.add(("merkle_multi_top", v))
    return f


FEATURES = (
    [(k, p) for k in ("layer", "quad", "multi", "top", "tail") for p in ("prev", "no prev")]
    + [("layer", "cols " + c) for c in ("0", "1..15", "16", "17+")] + [("layer", "z16 branch below 2^14")]
    + [("narrow", prev, nc, npw) for prev, nc in ((True, 0), (True, 4), (False, 4)) for npw in (1, 2, 4, 8)]
    + [("quad", "lds one group"), ("quad", "lds group plus one column"), ("quad", "lds several groups"), ("quad", "fallback above 2048 columns")]
    + [("multi", "levels", n) for n in (2, 3, 4)] + [("multi", "columns at level", lv) for lv in range(4)]
    + [("multi", "column count", c) for c in ("16", "17", "1")]
    + [("top", "blocks", 2), ("top", "blocks", 256)]
    + [("top", "columns at", w) for w in ("lane-per-node level", "quad level", "phase 2")]
    + [("top", "phase 2 first layer of 128 nodes"), ("top", "phase 2 wide")]
    + [("tail", "top_log 8"), ("tail", "top_log below 8"), ("tail", "wide at", "l = 8"), ("tail", "wide at", "a middle layer"),
       ("tail", "wide at", "l = 0"), ("tail", "not wide at 47 columns")]
    + [("merkle_multi_top", 17), ("merkle_multi_top", 23)]
)


def test_op_shapes_reach_every_feature():
    _assert_default_environment()
    got = set()
    for name, logs, tuning in MERKLE_OP_SHAPES:
        with tuned(tuning):
            got |= features_of(merkle_plan(logs), tuning)
    assert sorted(map(str, set(FEATURES) - got)) == [], "kernel variants no shape of tests/merkle_op_shapes.py reaches"
    # the natural (untuned) two chunks per wave: the prefetch of the next chunk under the default tuning
    natural = set()
    for name, logs, tuning in MERKLE_OP_SHAPES:
        if not tuning:
            natural |= features_of(merkle_plan(logs), tuning)
    assert ("narrow", False, 4, 2) in natural
    # the hash_node=rfc shapes: one per kernel kind, every wide path
    rfc = set()
    for name, logs, tuning in MERKLE_OP_SHAPES:
        if name in RFC_SHAPES:
            with tuned(tuning):
                rfc |= features_of(merkle_plan(logs), tuning)
    assert {k for k, *_ in rfc} >= {"layer", "narrow", "quad", "multi", "top", "tail"}
    assert {("top", "phase 2 wide"), ("tail", "wide at", "a middle layer"), ("quad", "lds several groups")} <= rfc
