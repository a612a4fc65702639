"""Plain restatement of Stwo's MerkleProver::decommit walk and of what the device-side proof tail's lists are in its terms
(cairo_m_amd/csrc/tail_device.hpp): U[k] / W[k] / F[k] of a sorted query set S on a domain of 2^L0 points.  A helper: no test
functions.  tests/test_tail_lists.py compares the host mirror (cm_tail_list) with it, tests/test_gpu_tail_ops.py the kernels."""


def fold(positions, n=1):
    out = []
    for p in positions:
        if not out or out[-1] != p >> n:
            out.append(p >> n)
    return out


def pairs(positions):
    out = []
    for parent in fold(positions):
        out += [2 * parent, 2 * parent + 1]
    return out


def generic_walk(n_layers, col_layers, by_log):
    """MerkleProver::decommit: layers n_layers - 1 .. 0; `col_layers` = set of layers carrying columns; by_log[l] = sorted queried
    nodes of layer l.  Returns (hash witness [(layer, node)], column rows [(layer, node, is_query)]) in emission order."""
    hashes, rows = [], []
    last = []
    for layer in range(n_layers - 1, -1, -1):
        colq = by_log.get(layer, [])
        has_prev = layer + 1 < n_layers
        total, pi, qi = [], 0, 0
        while pi < len(last) or qi < len(colq):
            cands = []
            if pi < len(last):
                cands.append(last[pi] // 2)
            if qi < len(colq):
                cands.append(colq[qi])
            node = min(cands)
            if has_prev:
                if pi < len(last) and last[pi] == 2 * node:
                    pi += 1
                else:
                    hashes.append((layer + 1, 2 * node))
                if pi < len(last) and last[pi] == 2 * node + 1:
                    pi += 1
                else:
                    hashes.append((layer + 1, 2 * node + 1))
            isq = qi < len(colq) and colq[qi] == node
            if isq:
                qi += 1
            if layer in col_layers:
                rows.append((layer, node, isq))
            total.append(node)
        last = total
    return hashes, rows


def witness(q):
    """the unqueried siblings of the sorted nodes q: what opening whole sibling pairs adds"""
    have = set(q)
    return [p for p in pairs(q) if p not in have]


def ref_lists(S, L0, qmask):
    """(U, W, F), each a list over the shifts k = 0 .. L0 (layer l = L0 - k of 2^l nodes):
    U[k] = the queried nodes of the layer: S folded k times;
    W[k] = their unqueried siblings (none at the root: a layer of one node has no pair);
    F[k] = the hashes of layer l + 1 that the decommitment walk asks for at layer l in a tree that is queried at S and opens whole
           sibling pairs at every layer l >= 1 whose bit is set in qmask (the first FRI tree's column-bearing layers)."""
    U = [fold(S, k) for k in range(L0 + 1)]
    W = [witness(U[k]) if k < L0 else [] for k in range(L0 + 1)]
    by_log = {L0: list(S)}
    for l in range(1, L0 + 1):
        if qmask >> l & 1:
            by_log[l] = pairs(U[L0 - l])
    hashes, _ = generic_walk(L0 + 1, set(by_log), by_log)
    F = [[] for _ in range(L0 + 1)]
    for layer, node in hashes:
        F[L0 - layer + 1].append(node)
    return U, W, F
