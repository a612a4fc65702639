"""Witness and LogUp of the opcode components on EDGE operands, against cells derived mechanically from the reference.

tests/test_air_witness_golden.py and tests/test_logup_golden.py pin the AIR descriptions to the reference's `write_trace` /
`write_interaction_trace` closures on one program of random 16-bit limbs, which essentially never reaches the rows where the
closures branch: limb sums of exactly 0xFFFF / 0x10000, remainders next to the divisor, ties of the three arcs of
store_le_fp_imm, equal operands of a comparison, bytes 0x00 / 0xFF, felt 0 and P-1.  tests/edge_programs.py places those
operands one instruction each; tools/rsref/rs_witness.py / rs_logup.py `--program edge|div0` interpret the reference's closures
on that run and write tests/golden/air_witness_edge.npz, air_logup_edge.npz, air_witness_div0.npz (numbers only).  Here the
oracle — which instantiates the product's own cairo_m_amd/csrc/air descriptions — must reproduce them word for word; the GPU
twin is tests/test_gpu_air_edge_golden.py.  No tolerance anywhere: every comparison is equality of M31 words.

(The issue that asked for these tests calls the two division components "18 and 22" after their opcodes; in air::ComponentId
order they are 22, u32_store_div_fp_fp, and 14, u32_store_div_fp_imm.)"""
import os

import numpy as np
import pytest

from cairo_m_amd.lib import prover_input_arrays, vm_run
from tests.edge_programs import COMPONENT_OF, EDGE_OPS, P2H, P3H, div_by_zero_program, edge_program
from tests.test_air_witness_golden import OPCODE_FILES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WIT = np.load(os.path.join(ROOT, "tests", "golden", "air_witness_edge.npz"))
LOG = np.load(os.path.join(ROOT, "tests", "golden", "air_logup_edge.npz"))
DIV0 = np.load(os.path.join(ROOT, "tests", "golden", "air_witness_div0.npz"))
P = 2**31 - 1
M32 = 0xFFFFFFFF
NAMES = list(OPCODE_FILES) + ["memory", "merkle"]
C_DIV_IMM, C_DIV_FP = 14, 22
N_REL, MAX_REL = 8, 16


def program_words(prog):
    """the layout tools/rsref/rs_witness.py stores a program in: (length, words.., -1 padding) per instruction"""
    w = np.full((len(prog), 7), -1, dtype=np.int64)
    for k, ins in enumerate(prog):
        w[k, 0], w[k, 1:1 + len(ins)] = len(ins), ins
    return w


def edge_table(gold):
    return [(str(n), int(c), int(r)) for n, c, r in zip(gold["edge_names"], gold["edge_cid"], gold["edge_row"])]


def relation_words(log):
    """cm_relations of the seeded relations stored with a LogUp fixture: z[8][4] then alpha_pow[8][16][4]"""
    from tests.test_gpu_logup_golden import qmul
    pw = np.zeros((N_REL, MAX_REL, 4), dtype=np.uint32)
    for r in range(N_REL):
        a, cur = tuple(int(x) for x in log["rel_alpha"][r]), (1, 0, 0, 0)
        for i in range(MAX_REL):
            pw[r, i] = cur
            cur = qmul(cur, a)
    return np.concatenate([log["rel_z"].astype(np.uint32).reshape(-1), pw.reshape(-1)])


def describe_mismatch(name, cid, got, want, edges):
    """first differing cell of a component's trace: component, column, row, and the edge placed on that row if there is one"""
    if got.shape != want.shape:
        return f"{name}: trace shape {got.shape}, fixture {want.shape}"
    bad = np.argwhere(got != want)
    if bad.size == 0:
        return None
    col, row = (int(x) for x in bad[0])
    at = {(c, r): n for n, c, r in edges}.get((cid, row))
    return (f"{name} (component {cid}): column {col}, row {row}" + (f", edge '{at}'" if at else "") +
            f": got {int(got[col, row])}, reference-derived {int(want[col, row])}; {len(bad)} cells differ")


def check_logup_columns(name, got, cs, want):
    """got: (n_cols, 4, n) interaction columns, cs: claimed sum, want: (n_cols, n, 4) per-row running sums of the fractions (the
    form of tests/test_logup_golden.py: every column but the last cell by cell, the last as the prefix sum of the row totals)"""
    n_cols, n = want.shape[0], want.shape[1]
    last = n_cols - 1
    for j in range(last):
        bad = np.argwhere(got[j].T != want[j])
        assert bad.size == 0, f"{name}: LogUp column {j}: first differing (row, coordinate) {bad[:4].tolist()}"
    total = want[last]
    claimed = total.sum(axis=0) % P
    assert [int(x) for x in cs] == [int(x) for x in claimed], f"{name}: claimed sum"
    shift = claimed * pow(n, P - 2, P) % P
    c = got[last].T
    key = lambda a: sorted(map(tuple, a.tolist()))
    assert key((c - total + shift) % P) == key(c), f"{name}: last column is not the running sum of the row totals minus the shift"


MULT_LOGS = (8, 16, 20, 18)            # range_check_8 / 16 / 20, bitwise


def expected_multiplicities(gold):
    """the four multiplicity columns from the reference closures' recorded `lookup_data` (rows: component id, tuple..): plain
    numpy bincounts; a bitwise tuple (op, a, b, result) sits at op * 2^16 + a * 2^8 + b (preprocessed/bitwise.rs:283-319)"""
    out = []
    for kind, lg in zip(("range_check_8", "range_check_16", "range_check_20"), MULT_LOGS):
        v = gold["lookup_" + kind][:, 1].astype(np.int64)
        assert v.size and v.max() < 1 << lg, kind
        out.append(np.bincount(v, minlength=1 << lg).astype(np.uint32))
    bw = gold["lookup_bitwise"][:, 1:].astype(np.int64)
    op, a, b, res = bw.T
    assert op.max() < 3 and a.max() < 256 and b.max() < 256
    assert np.array_equal(res, np.where(op == 0, a & b, np.where(op == 1, a | b, a ^ b)))
    out.append(np.bincount((op << 16) + (a << 8) + b, minlength=1 << 18).astype(np.uint32))
    return out


@pytest.fixture(scope="module")
def run():
    prog, steps, edges = edge_program()
    inp = vm_run(prog, entry_pc=0, args=(), n_returns=0)
    assert inp.steps == steps
    yield inp, prog, edges, prover_input_arrays(inp.view)
    inp.free()


@pytest.fixture(scope="module")
def div0_run():
    prog, steps, edges = div_by_zero_program()
    inp = vm_run(prog, entry_pc=0, args=(), n_returns=0)
    assert inp.steps == steps
    yield inp, prog, edges, prover_input_arrays(inp.view)
    inp.free()


def test_fixtures_were_made_from_todays_programs(run, div0_run):
    """a changed generator without regenerated fixtures is named as such, not as a witness mismatch"""
    for gold, (inp, prog, edges, _) in ((WIT, run), (DIV0, div0_run)):
        assert np.array_equal(gold["program"], program_words(prog)) and int(gold["steps"][0]) == inp.steps
        assert edge_table(gold) == edges
    assert np.array_equal(LOG["program"], WIT["program"])
    assert inp.steps < 4096


def test_edge_program_is_valid(oracle, run):
    """every constraint vanishes on every row and the LogUp sums cancel"""
    rc, err = oracle.assert_constraints(run[0].view)
    assert rc == 0, err


@pytest.mark.parametrize("cid", range(28), ids=NAMES)
def test_witness_matches_reference_derived_cells(oracle, run, cid):
    inp, _, edges, arrs = run
    want = WIT[NAMES[cid]]
    got = oracle.component_trace(inp.view, cid)
    msg = describe_mismatch(NAMES[cid], cid, got, want, edges)
    assert msg is None, msg
    if cid < 26:
        assert int(want[0].sum()) == arrs[f"bundles{cid}"].shape[0]       # the enabler column counts the live rows


@pytest.mark.parametrize("cid", range(27), ids=NAMES[:27])
def test_oracle_logup_columns_equal_reference_derived_fractions(oracle, run, cid):
    name = NAMES[cid]
    want = LOG[name].astype(np.int64)
    n_cols, n = want.shape[0], want.shape[1]
    cols, cs = oracle.component_interaction(run[0].view, cid, relation_words(LOG), 4 * n_cols, n.bit_length() - 1)
    check_logup_columns(name, cols.astype(np.int64).reshape(n_cols, 4, n), cs, want)


def test_oracle_multiplicities_equal_bincounts_of_the_reference_lookups(oracle, run):
    """the lookup tables' multiplicity columns (components 30..33) against the range-check / bitwise tuples the reference's
    closures recorded, padding lanes included"""
    for k, (cid, want) in enumerate(zip((30, 31, 32, 33), expected_multiplicities(WIT))):
        got = oracle.component_trace(run[0].view, cid)[0]
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, f"component {cid}: multiplicities differ at entries {bad[:5].tolist()}"


# ---- the edge guard: what a row really carries, decoded from the run's bundles ---------------------------------------
def operands(op, b, acc):
    """(x, y) of the instruction in bundle row `b` (pc, fp, clock, inst_prev_clock, words[6], span_start, span_len); `acc` = its
    data accesses (address, prev_clock, prev_value, value) in the order the runner logs them (sources, then destinations)"""
    w = [int(x) for x in b[4:10]]
    v = [int(a[3]) for a in acc]
    u = lambda k: v[k] | (v[k + 1] << 16)
    if op.startswith("u_") and op.endswith("_ff"):
        return u(0), u(2)
    if op.startswith("u_") and op.endswith("_fi"):
        return u(0), w[2] | (w[3] << 16)
    if op == "u_imm":
        return w[1], w[2]
    if op in ("add", "sub", "mul", "div"):
        return v[0], v[1]
    if op in ("addi", "muli", "le"):
        return v[0], w[2]
    if op in ("store_imm", "jmp_rel", "sfp"):
        return w[1], 0
    if op == "jnz":
        return v[0], 0
    if op.startswith("dderef_fi"):
        return w[2], 0
    if op.startswith("dderef_ff"):
        return v[1], 0
    raise KeyError(op)


def _div(n, d):
    q, r = divmod(n, d)
    return q, r, r & 0xFFFF, r >> 16, d & 0xFFFF, d >> 16


def _arcs(src, imm):
    a, b = min(src, imm), max(src, imm)
    return [a, b - a, P - 1 - b]


def _kept(src, imm):
    arcs = _arcs(src, imm)
    return sorted(arcs)[:2], arcs


TAGS = {
    "d=1": lambda n, d: d == 1, "d=max": lambda n, d: d == M32, "n<d": lambda n, d: n < d, "n=d": lambda n, d: n == d,
    "n=max": lambda n, d: n == M32, "n=0": lambda n, d: n == 0 and d > 0, "d=0": lambda n, d: d == 0,
    "r_lo=ffff,d_lo=0": lambda n, d: _div(n, d)[2] == 0xFFFF and _div(n, d)[4] == 0,
    "r_lo=d_lo,r_hi<d_hi": lambda n, d: _div(n, d)[2] == _div(n, d)[4] and _div(n, d)[3] < _div(n, d)[5],
    "r=d-1": lambda n, d: n % d == d - 1 and n // d > 0,
    "q*d+r carries at 0x10000": lambda n, d: ((n // d) * d & 0xFFFF) + (n % d & 0xFFFF) == 0x10000,
    "eq": lambda a, b: a == b,
    "lo": lambda a, b: a >> 16 == b >> 16 and a & 0xFFFF != b & 0xFFFF,
    "hi": lambda a, b: a >> 16 != b >> 16 and a & 0xFFFF == b & 0xFFFF,
    "hi<,lo>": lambda a, b: a >> 16 < b >> 16 and a & 0xFFFF > b & 0xFFFF,
    "hi>,lo<": lambda a, b: a >> 16 > b >> 16 and a & 0xFFFF < b & 0xFFFF,
    "ends": lambda a, b: {a, b} == {0, M32},
    "x,x": lambda a, b: a == b and a not in (0, M32), "x,~x": lambda a, b: a ^ b == M32 and a not in (0, M32),
    "0,max": lambda a, b: (a, b) == (0, M32), "max,0": lambda a, b: (a, b) == (M32, 0),
    "bytes": lambda a, b: all(((x >> s) & 0xFF) in (0, 0xFF) for x in (a, b) for s in (0, 8, 16, 24)),
    "a=b": lambda s, i: s == i and 0 < s < P - 1, "a=0": lambda s, i: s == 0 < i < P - 1, "b=P-1": lambda s, i: 0 < s < i == P - 1,
    "a=b=0": lambda s, i: s == i == 0, "a=b=P-1": lambda s, i: s == i == P - 1, "a=0,b=P-1": lambda s, i: (s, i) == (0, P - 1),
    "tie01 short": lambda s, i: s < i and _arcs(s, i)[0] == _arcs(s, i)[1] < _arcs(s, i)[2],
    "tie02 short": lambda s, i: s < i and _arcs(s, i)[0] == _arcs(s, i)[2] < _arcs(s, i)[1],
    "tie12 long": lambda s, i: s < i and _arcs(s, i)[1] == _arcs(s, i)[2] > _arcs(s, i)[0],
    "tie01 long": lambda s, i: s < i and _arcs(s, i)[0] == _arcs(s, i)[1] > _arcs(s, i)[2],
    "tie02 long": lambda s, i: s <= i and _arcs(s, i)[0] == _arcs(s, i)[2] > _arcs(s, i)[1],
    "tie012": lambda s, i: s < i and len(set(_arcs(s, i))) == 1,
    "short=k*P3H,long=k*P2H": lambda s, i: s < i and _kept(s, i)[0][0] % P3H == 0 and _kept(s, i)[0][1] % P2H == 0 and _kept(s, i)[0][0] > 0,
    "one below": lambda s, i: s < i and _kept(s, i)[0][0] % P3H == P3H - 1 and _kept(s, i)[0][1] % P2H == P2H - 1,
    "arcs 1,2 kept": lambda s, i: s < i and max(_arcs(s, i)) == _arcs(s, i)[0] and _kept(s, i)[0][0] % P3H == 0 and _kept(s, i)[0][1] % P2H == P2H - 1,
    "gt tie01 short": lambda s, i: s > i and _arcs(s, i)[0] == _arcs(s, i)[1] < _arcs(s, i)[2],
    "gt a=0,b=P-1": lambda s, i: (s, i) == (P - 1, 0), "gt tie012": lambda s, i: s > i and len(set(_arcs(s, i))) == 1,
    "gt by one": lambda s, i: s == i + 1, "gt tie12 long": lambda s, i: s > i and _arcs(s, i)[1] == _arcs(s, i)[2] > _arcs(s, i)[0],
    "backward": lambda off, _: off > P // 2, "negative": lambda off, _: off > P // 2,
}


def check_edges(edges, arrs):
    seen = set()
    for name, cid, row in edges:
        op, rest = name.split(":")
        spec, _, tag = rest.partition("#")
        x, y = (int(t, 16) for t in spec.split(","))
        bundles = arrs[f"bundles{cid}"]
        assert row < bundles.shape[0], f"edge '{name}': component {cid} has only {bundles.shape[0]} live rows"
        b = bundles[row]
        assert int(b[4]) == EDGE_OPS[op] and COMPONENT_OF[EDGE_OPS[op]] == cid, f"edge '{name}': row {row} of component {cid} runs opcode {int(b[4])}"
        assert (cid, row) not in seen, f"edge '{name}' shares its row with another edge"
        seen.add((cid, row))
        if op == "call":        # depth d: the frame pointer has moved d - 1 times from the entry frame's
            fps = sorted({int(r[1]) for r in bundles})
            assert fps.index(int(b[1])) == x - 1, f"edge '{name}': call at frame {fps.index(int(b[1]))}"
            continue
        acc = arrs["data_accesses"][int(b[10]):int(b[10]) + int(b[11])]
        got = operands(op, b, acc)
        assert got == (x, y), f"edge '{name}': row {row} of component {cid} carries ({got[0]:#x}, {got[1]:#x})"
        if tag:
            assert tag in TAGS, f"edge '{name}': no predicate for its tag"
            assert TAGS[tag](*got), f"edge '{name}': the operands ({got[0]:#x}, {got[1]:#x}) do not have the property '{tag}'"


def test_every_edge_row_carries_the_named_operands(run, div0_run):
    check_edges(run[2], run[3])
    check_edges(div0_run[2], div0_run[3])
    assert len(run[2]) == len(set(n for n, _, _ in run[2]))


def _required():
    """the cases the edge list asks for, written out here independently of the generator's tables: (name prefix, tag or None)"""
    X, NX = 0xDEADBEEF, 0xDEADBEEF ^ M32
    req = []
    for f in ("u_add_ff", "u_add_fi"):
        req += [(f"{f}:{a:x},{b:x}", None) for a, b in ((0, 0), (0xFFFF, 1), (0xFFFF0000, 0x10000), (M32, 1), (M32, M32))]
    req += [("u_sub_ff:0,1", None), ("u_sub_ff:10000,1", None), ("u_sub_ff:12345678,12345678", None)]
    for f in ("u_mul_ff", "u_mul_fi"):
        req += [(f"{f}:0,", None)] + [(f"{f}:{a:x},{b:x}", None) for a, b in ((M32, M32), (0x10000, 0x10000), (0xFFFF, 0xFFFF), (0xFF, 0x101))]
    for f in ("u_div_ff", "u_div_fi"):
        req += [(f"{f}:", t) for t in ("d=1", "d=max", "n<d", "n=d", "r_lo=ffff,d_lo=0", "r_lo=d_lo,r_hi<d_hi", "r=d-1", "n=0")]
        req += [(f"{f}:{M32:x},{d:x}", "n=max") for d in (0xFF, 0x100, 0x10000, 0x10001)]
    for f in ("u_lt_ff", "u_lt_fi"):
        req += [(f"{f}:", "eq"), (f"{f}:10002,10003", "lo"), (f"{f}:10003,10002", "lo"), (f"{f}:20001,30001", "hi"), (f"{f}:30001,20001", "hi"),
                (f"{f}:", "hi<,lo>"), (f"{f}:0,{M32:x}", "ends"), (f"{f}:{M32:x},0", "ends")]
    for k in ("and", "or", "xor"):
        for f in (f"u_{k}_ff", f"u_{k}_fi"):
            req += [(f"{f}:{X:x},{X:x}", "x,x"), (f"{f}:{X:x},{NX:x}", "x,~x"), (f"{f}:0,{M32:x}", "0,max"), (f"{f}:ff00ff,ff00ff00", "bytes")]
    req += [("u_imm:0,0", None), ("u_imm:ffff,ffff", None)]
    req += [(f"add:{P - 1:x},1", None), ("sub:0,1", None), (f"mul:{P - 1:x},{P - 1:x}", None), ("div:1234567,1", None),
            (f"div:1234567,{P - 1:x}", None), ("div:1234567,1234567", None),
            ("addi:1234567,0", None), (f"addi:1234567,{P - 1:x}", None), (f"addi:{P - 1:x},1", None),
            ("muli:1234567,0", None), (f"muli:{P - 1:x},{P - 1:x}", None), ("store_imm:0,0", None), (f"store_imm:{P - 1:x},0", None)]
    req += [("le:", t) for t in ("a=b", "a=0", "b=P-1", "a=b=0", "tie01 short", "tie02 short", "tie12 long", "tie01 long", "tie02 long",
                                 "short=k*P3H,long=k*P2H", "one below", "gt by one", "gt tie012")]
    req += [("le:2aaaaaaa,55555554", "tie012")]                            # a = 715827882, b = 1431655764: 3a = P - 1
    req += [("jnz:0,0", None), ("jnz:1,0", None), (f"jnz:{P - 1:x},0", None), ("jmp_rel:", "backward"), ("call:2,0", "depth 2")]
    for f in ("dderef_fi_load", "dderef_fi_store", "dderef_ff_load", "dderef_ff_store", "sfp"):
        req += [(f"{f}:0,0", None), (f"{f}:", "negative")]
    return req


def test_every_case_of_the_edge_list_is_placed(run):
    """(the cases the generator's docstring lists as not expressible are placed in their nearest valid form: `x op x` over two
    cells, subtraction and felt sub / div without an immediate form, division by zero in div_by_zero_program)"""
    names = [n for n, _, _ in run[2]]
    for prefix, tag in _required():
        hit = [n for n in names if n.startswith(prefix) and (tag is None or n.endswith("#" + tag))]
        assert hit, f"no edge '{prefix}..{'#' + tag if tag else ''}' in the edge program"
    assert 715827882 == 0x2AAAAAAA and 1431655764 == 0x55555554


def test_live_row_counts(run):
    """a component with exactly one live row, one that fills a packed row of 16 with no padding lane, one with 17"""
    n = [run[3][f"bundles{c}"].shape[0] for c in range(26)]
    assert n[0] == 1 and n[10] == 16 and n[3] == 17, n
    assert n[15] == n[16] == 0 and all(x > 0 for c, x in enumerate(n) if c not in (15, 16)), n
    for cid, want in ((0, 1), (10, 16), (3, 17)):
        assert int(WIT[NAMES[cid]][0].sum()) == want and WIT[NAMES[cid]].shape[1] == (16 if want <= 16 else 32)


# ---- division by zero: rows no valid run contains -------------------------------------------------------------------
@pytest.mark.parametrize("cid", [C_DIV_IMM, C_DIV_FP], ids=["u32_store_div_fp_imm", "u32_store_div_fp_fp"])
def test_division_by_zero_witness_matches_reference_derived_cells(oracle, div0_run, cid):
    """the reference's write_trace maps d = 0 to quotient 0, remainder 0 (u32_store_div_fp_fp.rs:362-364)"""
    inp, _, edges, _ = div0_run
    got = oracle.component_trace(inp.view, cid)
    msg = describe_mismatch(NAMES[cid], cid, got, DIV0[NAMES[cid]], edges)
    assert msg is None, msg


def test_division_by_zero_is_not_provable(oracle, div0_run):
    rc, err = oracle.assert_constraints(div0_run[0].view)
    assert rc != 0 and ("U32StoreDivFpImm" in err or "U32StoreDivFpFp" in err), (rc, err)
    assert "row 0" in err, err
