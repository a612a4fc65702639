"""What tests/test_verify_shapes_cpu.py and tests/test_gpu_verify_shapes.py share: the wide query configs, the column log sizes of
a proof worked out from its claim alone, the flips that land in every trip of the device verifier's stride loops, and — written
as plain Python over the proof's layout, never read from the library's plan — which device checks each flip must raise.

The dataflow behind the predictions (cairo_m_amd/csrc/verify_device.hip): a queried value of a column of extended log l feeds the
root of its commitment tree and the DEEP answer of size group l; the answer is one value of a first-layer pair (first-layer
commitment), the folded pair is added into the inner layer of layer_log l - 1, and from there every fold carries it on: each later
inner layer's pairs (its commitment) and at last the value the last polynomial is compared with.  Inner layers above l - 1 never
see it.  A hash witness feeds one root and nothing else."""
import ctypes as C

from tests.verify_many_util import proof_layout

# (pow_bits, log_blowup_factor, log_last_layer_degree_bound, n_queries)
ONE_QUERY = (0, 1, 0, 1)
FRI_TWO_TRIPS = (3, 2, 1, 129)      # more than FRI_THREADS = 128 pairs in an inner layer
WIDE = (0, 1, 0, 300)               # more than 256 pairs, more than 2 * MERKLE_THREADS = 512 nodes in a level
AT_THE_LIMIT = (0, 1, 2, 512)       # 1024 nodes in a level: 64 KB of LDS
ABOVE_THE_LIMIT = (0, 1, 0, 700)
ACCEPTED = [ONE_QUERY, FRI_TWO_TRIPS, WIDE, AT_THE_LIMIT]
REFUSAL = "cm_verify_many: more than 1024 nodes in one level of a tree (n_queries above 512) is not supported on the device"

MERKLE, FRI_FIRST_COMMITMENT, FRI_INNER_COMMITMENT, FRI_LAST_EVALS = 7, 10, 12, 13      # CM_VERIFY_* (include/cairom_hip.h)


def column_logs(L, words):
    """column log sizes per tree (preprocessed, trace, interaction, composition) from the claim in the proof's words and the
    AIR's column counts (cm_component_info, a table lookup), checked against the number of sampled columns the proof carries"""
    from cairo_m_amd.lib import PREPROCESSED_LOG
    w = [int(x) for x in words[:6 + int(words[5])]]
    claim = w[6:6 + w[5]]
    logs = [list(PREPROCESSED_LOG), [], [], [max(claim) + 1] * 4]
    for c, lg in enumerate(claim):
        n_tr, n_it, n_con = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0)
        assert L.cm_component_info(C.c_int32(c), C.byref(n_tr), C.byref(n_it), C.byref(n_con)) == 0
        logs[1] += [lg] * n_tr.value
        logs[2] += [lg] * n_it.value
    assert [len(x) for x in logs] == [len(x) for x in proof_layout(words)["sampled"]]
    return logs


def query_logs(logs, cfg):
    """the distinct extended log sizes, descending (one size group of the first FRI layer each)"""
    return sorted({lg + cfg[1] for tree in logs for lg in tree}, reverse=True)


def group_columns(logs, cfg, ext_log):
    """(tree, column) of every column of one size group, in the order the sample batch at the OODS point lists them"""
    return [(t, c) for t in range(4) for c, lg in enumerate(logs[t]) if lg + cfg[1] == ext_log]


def widest_group(logs, cfg):
    """(extended log, columns) of the size group with the most columns: its OODS batch is the widest sample batch"""
    return max(((lg, group_columns(logs, cfg, lg)) for lg in query_logs(logs, cfg)), key=lambda g: len(g[1]))


def last_entry_of_the_widest_batch(logs, cfg, words):
    """word offset of the queried value the LAST entry of the widest sample batch reads at the last query row of its group.  The
    queried values of a tree run from the largest columns to the smallest, row by row: when the widest group is the smallest one
    of the last entry's tree, that value is the tree's last queried word."""
    ext_log, cols = widest_group(logs, cfg)
    t, c = cols[-1]
    assert ext_log == min(logs[t]) + cfg[1]
    off, n = proof_layout(words)["queried"][t]
    return len(cols) - 1, off + n - 1


def _three(off, n, unit):
    """the first, the middle and the last word of n records of `unit` words at off"""
    return [off, off + unit * (n // 2) + unit // 2, off + unit * n - 1]


def loop_flips(words):
    """name -> word offset: the first, the middle and the last word of every array the stride loops of the three kernels walk"""
    lay = proof_layout(words)
    out = {}

    def put(name, off, n, unit):
        assert n > 0, name
        for where, pos in zip(("first", "middle", "last"), _three(off, n, unit)):
            out["%s, %s word" % (name, where)] = pos

    for t in range(4):
        put("queried values of tree %d" % t, *lay["queried"][t], 1)
        put("hash witness of tree %d" % t, *lay["decommitments"][t]["hash_witness"], 8)
    put("first-layer FRI witness", *lay["fri_first"]["fri_witness"], 4)
    inner = [k for k, d in enumerate(lay["fri_inner"]) if d["fri_witness"][1]]
    for k in sorted({inner[0], inner[len(inner) // 2], inner[-1]}):
        put("FRI witness of inner layer %d" % k, *lay["fri_inner"][k]["fri_witness"], 4)
    return out


def slot_keys(n_inner):
    """the device slots of a proof that plans through, in the host verifier's order"""
    return [("tree", t) for t in range(4)] + [("first",)] + [("inner", k) for k in range(n_inner)] + [("last",)]


def slot_key(check, message):
    """a slot of cm_verify_many_detail by what it checks"""
    if check == MERKLE:
        assert message.startswith("Merkle(tree ") and message.endswith("): RootMismatch"), message
        return ("tree", int(message[len("Merkle(tree "):message.index(")")]))
    if check == FRI_FIRST_COMMITMENT:
        assert message == "Fri(FirstLayerCommitmentInvalid): RootMismatch", message
        return ("first",)
    if check == FRI_INNER_COMMITMENT:
        assert message.startswith("Fri(InnerLayerCommitmentInvalid ") and message.endswith("): RootMismatch"), message
        return ("inner", int(message[len("Fri(InnerLayerCommitmentInvalid "):message.index(")")]))
    assert (check, message) == (FRI_LAST_EVALS, "Fri(LastLayerEvaluationsInvalid)"), (check, message)
    return ("last",)


def verdict_cases(L, words, cfg):
    """[(name, word offset of the flip or None, the set of device slots that must be raised)]"""
    lay = proof_layout(words)
    logs = column_logs(L, words)
    q_logs = query_logs(logs, cfg)
    n_inner = len(lay["fri_inner"])
    assert n_inner == q_logs[0] - 1 - (cfg[2] + cfg[1])
    layer_log = [q_logs[0] - 1 - k for k in range(n_inner)]

    def behind_group(ext_log):
        """what a changed value of the first-layer size group of this log reaches"""
        return {("first",), ("last",)} | {("inner", k) for k in range(n_inner) if layer_log[k] <= ext_log - 1}

    cases = [("untouched", None, set())]
    # a hash witness: its own root, nothing else
    for t in range(4):
        off, n = lay["decommitments"][t]["hash_witness"]
        assert n
        cases.append(("hash witness of tree %d" % t, off + 8 * (n // 2) + 3, {("tree", t)}))
    off, n = lay["fri_first"]["hash_witness"]
    assert n
    cases.append(("hash witness of the first FRI layer", off + 8 * (n - 1) + 7, {("first",)}))
    with_hash = [k for k, d in enumerate(lay["fri_inner"]) if d["hash_witness"][1]]
    for k in sorted({with_hash[0], with_hash[len(with_hash) // 2], with_hash[-1]}):
        off, n = lay["fri_inner"][k]["hash_witness"]
        cases.append(("hash witness of inner layer %d" % k, off + 8 * (n // 2), {("inner", k)}))
    # a queried value.  The queried values of a tree run from its largest columns to its smallest: the first word of the
    # composition tree is a column of the LARGEST size group (nothing else is that large), the last word of a tree is its smallest
    # column, which for the trace and the interaction tree is the SMALLEST size group
    assert q_logs[0] == logs[3][0] + cfg[1] and all(lg + cfg[1] < q_logs[0] for t in range(3) for lg in logs[t])
    cases.append(("queried value of the largest size group (tree 3)", lay["queried"][3][0], {("tree", 3)} | behind_group(q_logs[0])))
    assert min(logs[1]) + cfg[1] == q_logs[-1] == min(logs[2]) + cfg[1]
    for t in range(3):
        off, n = lay["queried"][t]
        ext = min(logs[t]) + cfg[1]
        which = "the smallest size group" if ext == q_logs[-1] else "the size group of log %d" % ext
        cases.append(("queried value of %s (tree %d)" % (which, t), off + n - 1, {("tree", t)} | behind_group(ext)))
    # the first layer's FRI witness fills the pairs group by group, largest first; with fewer than 1024 positions in a domain of
    # 2^20 or more the largest group does not have every sibling queried, so the first witness value is its
    assert q_logs[0] >= 20 and cfg[3] < 1024
    cases.append(("first-layer FRI witness of the largest size group", lay["fri_first"]["fri_witness"][0] + 2, behind_group(q_logs[0])))
    # an inner layer's FRI witness: that layer's pairs, and every fold behind it
    for k, d in enumerate(lay["fri_inner"]):
        off, n = d["fri_witness"]
        if n:
            cases.append(("FRI witness of inner layer %d" % k, off + 4 * (n // 2) + 1,
                          {("last",)} | {("inner", j) for j in range(k, n_inner)}))
    return cases


def flipped(words, pos):
    bad = words.copy()
    bad[pos] ^= 1
    return bad
