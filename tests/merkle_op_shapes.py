"""The column layouts (log size per column, commitment order) the GPU op tests of tests/test_gpu_merkle_layers.py commit and
compare layer by layer with the oracle.  tests/test_merkle_plan_cpu.py pins the launches cm_merkle_plan reports for each of
them and proves, without a GPU, that together they reach every variant of the six Merkle kernels listed there.

An entry is (id, column logs, tuning): `tuning` = the (key, value) pairs cm_set_tuning holds while the shape runs."""

MULTI_TOP_17 = ("merkle_multi_top", 17)
# layers 2^19 (4 columns, no children), 2^18 (children only) and 2^17 (children and 4 columns) as launches of their own: the
# three <PREV, NC> forms of k_merkle_narrow — or, under merkle_npw = 0, k_merkle_layer with 4 / 0 / 4 columns
NARROW_FORMS = [19] * 4 + [17] * 4

MERKLE_OP_SHAPES = [
    # k_merkle_tail alone: wide at 5 (48 columns = 3 chunks), at 3 (129 = 9 chunks, the last of one column) and at 0 (50 = 4
    # chunks), one group each (a group of the tail is 4096 words: 4096 >> l columns); 47 columns at 4 stay on the direct path;
    # 16 / 17 columns at 8 / 7 are the one- and two-chunk direct nodes
    ("tail_wide_5_3_0", [8] * 16 + [7] * 17 + [5] * 48 + [4] * 47 + [3] * 129 + [0] * 50, ()),
    # the tail wide at 8 (16 columns per group: 49 = 4 groups), at 6 (65 = 2 groups) and at 5 (2048 = the pointer table's cap, 16
    # groups); 2049 columns at 2 fall back to the direct path
    ("tail_wide_8_6_5_cap", [8] * 49 + [6] * 65 + [5] * 2048 + [2] * 2049, ()),
    # a tail that starts below 2^8, wide on its first layer
    ("tail_from_6", [6] * 48 + [3] * 3, ()),
    # k_merkle_layer_quad without a previous layer (64 columns = one group), then a tail with one, wide at 8 (48 = 3 groups)
    ("quad_leaf_then_tail", [9] * 64 + [8] * 48, ()),
    # four quad launches: 64 (one group, no previous layer), 65 (a group plus one column), 128 (two groups), 443 (seven groups,
    # the last of 11 columns); the tail below carries no columns
    ("quad_groups", [12] * 64 + [11] * 65 + [10] * 128 + [9] * 443, ()),
    # the quad kernel's fallback (more columns than the pointer table holds), then k_merkle_top of 2 blocks with children
    ("quad_fallback_then_top2", [10] * 2049, ()),
    # k_merkle_layer at 2^9 with children, with 0, 15, 16 and 17 columns: the one layer between a quad layer and the tail when 64
    # columns further down (here at 2^1, wide in the tail) keep the top launch out
    ("layer_0_cols", [10] * 64 + [1] * 64, ()),
    ("layer_15_cols", [10] * 64 + [9] * 15 + [1] * 64, ()),
    ("layer_16_cols", [10] * 64 + [9] * 16 + [1] * 64, ()),
    ("layer_17_cols", [10] * 64 + [9] * 17 + [1] * 64, ()),
    # a group cut down to one level by the quad layer below it: k_merkle_layer without children, 5 columns / the 4-column
    # branch with twelve literal zeros, which layers of 2^14 and more leave to k_merkle_narrow
    ("group_of_one", [13] * 5 + [12] * 64, ()),
    ("layer_4_cols_below_narrow", [13] * 4 + [12] * 64, ()),
    # k_merkle_multi of 2 levels, no previous layer: 3 columns at level 0, 1 at level 1; the quad layer below ends the group
    ("multi_2_levels", [14] * 3 + [13] + [12] * 64, ()),
    # k_merkle_multi of 3 levels: columns at levels 0 and 2 (17 = two chunks)
    ("multi_3_levels", [15] * 2 + [13] * 17 + [12] * 64, ()),
    # k_merkle_multi of 4 levels without a previous layer, 1 / 16 / 17 / 1 columns at levels 0..3, then k_merkle_top of 64 blocks
    # with a previous layer and 33 columns on its first level
    ("multi_4_levels_then_top", [18] + [17] * 16 + [16] * 17 + [15] + [14] * 33, ()),
    # k_merkle_multi WITH a previous layer (2^19 is a launch of its own) and no columns at level 0
    ("multi_with_prev", [19] + [17] * 2, ()),
    # k_merkle_top of 256 blocks, no previous layer; phase 2 (layers 7..0) wide at 6 (48 = 1 group of 3 chunks), at 5 (130 = 9
    # chunks: a group of 8 and one of 1) and at 0; layer 7 has 128 nodes: two passes of the 64-quad loop
    ("top256_phase2_wide", [16] + [6] * 48 + [5] * 130 + [0] * 49, ()),
    # k_merkle_top of 2 blocks, no previous layer, 63 columns on its first level; phase 2 is layer 0 alone, wide
    ("top2_phase2_wide_root", [9] * 63 + [0] * 48, ()),
    # one column at every layer of a 256-block top launch: lane-per-node levels, quad levels and phase 2
    ("top_every_layer", list(range(16, -1, -1)), ()),
    # the natural narrow npw = 2 at 2^21 (4 columns, no previous layer), then children only at 2^20 and 2^19 (npw 1); multi; top
    ("narrow_natural_npw2", [21] * 4, ()),
    # merkle_multi_top at the low end: 2^18 and 2^17 become launches of their own (narrow), then a top of 256 blocks
    ("multi_top_17", [18] * 4, (MULTI_TOP_17,)),
    # merkle_multi_top at the high end: a fused group starts at 2^20 (levels 20..17)
    ("multi_top_23", [20] * 3 + [19] * 18, (("merkle_multi_top", 23),)),
    # forced chunk counts on the three narrow forms, and none (k_merkle_layer)
    ("narrow_forms_npw8", NARROW_FORMS, (MULTI_TOP_17, ("merkle_npw", 8))),
    ("narrow_forms_npw4", NARROW_FORMS, (MULTI_TOP_17, ("merkle_npw", 4))),
    ("narrow_forms_npw2", NARROW_FORMS, (MULTI_TOP_17, ("merkle_npw", 2))),
    ("narrow_forms_npw1", NARROW_FORMS, (MULTI_TOP_17, ("merkle_npw", 1))),
    ("narrow_forms_off", NARROW_FORMS, (MULTI_TOP_17, ("merkle_npw", 0))),
]

TUNING_DEFAULTS = {"merkle_multi_top": 19, "merkle_npw": -1}

# the shape lists of tests/test_gpu_poly_merkle.py::test_merkle_commit_parity, in its order
COMMIT_PARITY_SHAPES = [
    [6, 6, 6], [8] * 17 + [5] * 3 + [3], [10] * 40 + [9] * 16 + [4] * 5, [1], [12, 3],
    [17] * 3 + [16] * 2 + [13] * 5 + [9] * 2 + [7] * 20 + [5] * 3 + [2], [16] * 4, [9] * 33,
    [15] * 2 + [11] * 70 + [6] * 3,
    [20] * 3 + [19] * 18 + [12] * 2, [19] * 4, [21] + [20] * 42 + [19],
]

# hash_node=rfc framing: one shape per kernel kind (layer, narrow, quad, multi, top, tail), the wide paths of the tail, of the
# top kernel's phase 2 and of the quad kernel included
RFC_SHAPES = ["tail_wide_5_3_0", "quad_groups", "layer_17_cols", "multi_4_levels_then_top", "top256_phase2_wide", "multi_top_17"]

# CM_NO_MERKLE_TOP=1 (tests/env_path_child.py): multi groups of 4 and 4, of 3 and of 2 levels, each above a tail with a previous
# layer (wide at 2^4 in the first)
NO_TOP_SHAPES = [[16] * 4 + [10] * 3 + [4] * 50, [11] * 5, [10] * 40 + [9] * 16 + [4] * 5]

# cm_merkle_commit_layer at 2^14, the smallest layer merkle_layer() hands to k_merkle_narrow: (columns, children) of the three
# narrow forms, and for every merkle_npw the chunk count it resolves to there (256 * npw must divide 2^14: 3 -> 1, 5 -> 2,
# 6 -> 3 -> 1, 7 -> 3 -> 1); 0 = k_merkle_layer; -1 (default) = one chunk per wave below 2^21
NARROW_LAYER_LOG = 14
NARROW_LAYER_FORMS = [(0, True), (4, True), (4, False)]
NPW_AT_2_14 = {-1: 1, 0: 0, 1: 1, 2: 2, 3: 1, 4: 4, 5: 2, 6: 1, 7: 1, 8: 8}
# the same at 2^21, where the default resolves to 2 chunks
NPW_AT_2_21 = {-1: 2, 0: 0, 1: 1, 2: 2, 3: 1, 4: 4, 5: 2, 6: 1, 7: 1, 8: 8}
