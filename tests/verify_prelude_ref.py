"""Pure-Python reference of the public data's LogUp contribution (PublicData::initial_logup_sum, public_data.rs:291-412) over the
q_* functions of tests/field_edges.py, and the shapes the prelude-op tests share.

A relation's `combine` is sum_i alpha^i * v_i - z.  The four fixed terms: the initial registers (pc, fp, 1) are emitted, the final
ones (pc, fp, clock + 1) consumed (the denominator is negated), and both memory roots enter as Merkle tuples (0, 0, root, root).
Every PRESENT public entry adds its memory tuple (addr, clock, value[0..4]) with multiplicity +1 for program and input and -1 for
output, and consumes its four Merkle leaves (4 * addr + k, TREE_HEIGHT, value[k], root) under the initial root (program, input) or
the final root (output).  The sum of the inverses of all these denominators is the result; the library's inverse of zero is zero,
so a vanishing denominator contributes nothing, and the reference says the same."""
import numpy as np

from tests.field_edges import P, RELATION_WORDS, edge_mix, q_add, q_inv, q_mul, q_neg, q_sub

REL_REGISTERS, REL_MEMORY, REL_MERKLE = 0, 1, 2          # air_common.hpp
TREE_HEIGHT = 30                                         # adapter/merkle.rs:63
B = 256                                                  # CM_PUBLIC_SUM_ENTRIES: entries per workgroup of k_verify_public_sum


def rel_z(rel, r):
    return tuple(int(w) for w in rel[4 * r:4 * r + 4])


def rel_alpha(rel, r, i):
    o = 32 + 4 * (16 * r + i)
    return tuple(int(w) for w in rel[o:o + 4])


def combine(rel, r, vals):
    acc = (0, 0, 0, 0)
    for i, v in enumerate(vals):
        acc = q_add(acc, tuple((a * (int(v) % P)) % P for a in rel_alpha(rel, r, i)))
    return q_sub(acc, rel_z(rel, r))


def inv0(x):
    return (0, 0, 0, 0) if not any(x) else q_inv(x)


def denominators(head, program, inp, output, rel):
    """every denominator of initial_logup_sum, in its order; lists are rows of (present, addr, v0, v1, v2, v3, clock)"""
    ipc, ifp, fpc, ffp, clock, iroot, froot = (int(w) for w in head)
    dens = [combine(rel, REL_REGISTERS, (ipc, ifp, 1)),
            q_neg(combine(rel, REL_REGISTERS, (fpc, ffp, (clock + 1) % P))),
            combine(rel, REL_MERKLE, (0, 0, iroot, iroot)),
            combine(rel, REL_MERKLE, (0, 0, froot, froot))]
    for rows, emit in ((program, True), (inp, True), (output, False)):
        root = iroot if emit else froot
        for row in np.asarray(rows, dtype=np.uint32).reshape(-1, 7):
            present, addr, v0, v1, v2, v3, clk = (int(w) for w in row)
            if not present:
                continue
            mem = combine(rel, REL_MEMORY, (addr, clk, v0, v1, v2, v3))
            dens.append(mem if emit else q_neg(mem))
            for k, v in enumerate((v0, v1, v2, v3)):
                dens.append(q_neg(combine(rel, REL_MERKLE, ((4 * addr + k) % P, TREE_HEIGHT, v, root))))
    return dens


def initial_logup_sum(head, program, inp, output, rel):
    s = (0, 0, 0, 0)
    for d in denominators(head, program, inp, output, rel):
        s = q_add(s, inv0(d))
    return s


# ---- shapes ------------------------------------------------------------------------------------------------------------------
def entries(rng, n_rows, absent=()):
    """n_rows rows of edge words (0, P - 1, 2^30, ...), present except at the row indices in `absent`"""
    rows = edge_mix(rng, 7 * n_rows).reshape(n_rows, 7).copy()
    rows[:, 0] = 1
    for k in absent:
        rows[k, 0] = 0
    return rows


def random_rel(rng):
    return rng.integers(0, P, size=RELATION_WORDS, dtype=np.uint32)


def rel_with_zero_denominator(rel, r, vals):
    """`rel` with z of relation r moved so that combine(rel, r, vals) is exactly zero"""
    out = np.array(rel, dtype=np.uint32)
    out[4 * r:4 * r + 4] = 0
    out[4 * r:4 * r + 4] = combine(out, r, vals)     # sum alpha^i v_i - 0
    assert not any(combine(out, r, vals))
    return out


def split3(n, how):
    """n rows over (program, input, output)"""
    if how == "spread":
        a = n // 3
        return a, (n - a) // 2, n - a - (n - a) // 2
    if how == "output only":
        return 0, 0, n
    if how == "no input":
        return n // 2, 0, n - n // 2
    assert how == "program only"
    return n, 0, 0


def sum_cases():
    """[(name, head, program, input, output, rel)]: present totals 0, 1, B - 1, B, B + 1 and 3B + 1, spread over the three lists and
    with empty lists, absent entries first and last in a workgroup's chunk, one zero memory denominator, one zero Merkle leaf"""
    rng = np.random.default_rng(20240611)
    out = []
    for total in (0, 1, B - 1, B, B + 1, 3 * B + 1):
        for how in ("spread", "output only", "no input", "program only"):
            if total == 3 * B + 1 and how not in ("spread", "output only"):
                continue
            counts = split3(total, how)
            head = edge_mix(rng, 7)
            lists = []
            for n_present in counts:
                # absent rows interleaved: the first and the last row of the first chunk, and one in the middle
                n_rows = n_present + (3 if n_present >= 3 else 0)
                absent = (0, n_rows // 2, min(n_rows, B) - 1) if n_present >= 3 else ()
                lists.append(entries(rng, n_rows, absent))
            assert sum(int(x[:, 0].sum()) for x in lists) == total
            out.append(("%d present, %s" % (total, how), head, lists[0], lists[1], lists[2], random_rel(rng)))
    # exactly one memory denominator is zero: an input entry in the second chunk
    head = edge_mix(rng, 7)
    lists = [entries(rng, 5), entries(rng, B + 9), entries(rng, 4)]
    row = [int(w) for w in lists[1][B + 3]]
    rel = rel_with_zero_denominator(random_rel(rng), REL_MEMORY, (row[1], row[6], row[2], row[3], row[4], row[5]))
    out.append(("zero memory denominator", head, lists[0], lists[1], lists[2], rel))
    # exactly one Merkle leaf is zero: leaf 2 of an output entry, under the final root
    head = edge_mix(rng, 7)
    lists = [entries(rng, 3), entries(rng, 0), entries(rng, 7)]
    row = [int(w) for w in lists[2][4]]
    rel = rel_with_zero_denominator(random_rel(rng), REL_MERKLE, ((4 * row[1] + 2) % P, TREE_HEIGHT, row[4], int(head[6])))
    out.append(("zero Merkle leaf", head, lists[0], lists[1], lists[2], rel))
    return out


def count_zero_denominators(case):
    _, head, program, inp, output, rel = case
    return sum(1 for d in denominators(head, program, inp, output, rel) if not any(d))


# ---- point evaluation ----------------------------------------------------------------------------------------------------------
N_COMPONENTS, N_PREPROCESSED = 34, 7


def component_counts(L, cid):
    """(trace words, interaction sample words, coefficient words) of a component from cm_component_info"""
    import ctypes as C
    n_tr, n_it, n_con = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0)
    assert L.cm_component_info(C.c_int32(cid), C.byref(n_tr), C.byref(n_it), C.byref(n_con)) == 0
    return 4 * n_tr.value, 4 * (n_it.value + 4), 4 * n_con.value


def eval_job_words(L, cid, rng, edge):
    """(tr, it, pp, rel, coeff, shift) for one job: random words below P, or edge words, in every slot; the shift is never zero"""
    n_tr, n_it, n_co = component_counts(L, cid)
    draw = (lambda n: edge_mix(rng, n)) if edge else (lambda n: rng.integers(0, P, size=n, dtype=np.uint32))
    shift = draw(4)
    shift[0] = shift[0] or 1
    return draw(n_tr), draw(n_it), draw(4 * N_PREPROCESSED), draw(RELATION_WORDS), draw(n_co), shift
