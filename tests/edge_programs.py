"""Edge-operand programs for the AIR golden tests (tests/test_air_edge_golden.py, tests/test_gpu_air_edge_golden.py).

``edge_program()`` is the counterpart of ``cairo_m_amd.workloads.all_opcodes_program``: where that one feeds every opcode
random 16-bit limbs, this one places, one instruction per case, the operands at which the reference's witness code branches or
a restatement could be off by one (limb carries at 0xFFFF / 0x10000, borrow comparisons of the division core, division
remainders next to the divisor, ties of the three arcs of store_le_fp_imm, bitwise bytes 0x00 / 0xFF, felt values 0 and P-1,
jumps backwards, nested calls, negative offsets).  It is straight-line apart from three short forward skips, one backward jump
and a call nested two deep, every operand lives in a fresh frame cell written by a preceding STOREI / U_IMM, and it runs on
the synthetic VM (``vm_run``) in well under 4096 steps.  It returns ``(program, steps, edges)``; ``edges`` lists
``(name, component_id, live_row_index)`` for every case placed, the row index being the position of the instruction among the
bundles of its opcode component (air::ComponentId order, tests/test_air_witness_golden.py::OPCODE_FILES; within a component
the bundles are grouped by opcode, each group in the order of execution).

Edge names are the specification the tests check the run against: ``"<op>:<a>,<b>"`` with hexadecimal operand VALUES (for an
immediate form the second operand is the immediate), optionally followed by ``"#<tag>"`` naming the property the operands were
chosen for.  ``EDGE_OPS`` maps ``<op>`` to its opcode, ``COMPONENT_OF`` an opcode to its component.

Cases of the list that are NOT placed, and why:

* ``x op x`` (u32 sub, bitwise, felt div) naming ONE cell as both source operands: the reference's components read each
  source once per instruction and a second read of the same cell would need ``clock < clock``; its compiler rewrites such
  instructions with a temporary copy (crates/compiler/codegen/src/passes/mod.rs:9-19, :367).  The cases are placed with the
  same VALUE in two distinct cells.
* u32 sub in an fp_imm form: the instruction set has no U32StoreSubFpImm (crates/common/src/instruction.rs:431-476: the u32 fp_imm
  opcodes are 19 add, 21 mul, 22 div/rem; 20 is unassigned), so the three subtraction cases exist in the fp_fp form only.
* felt sub / div by an immediate: likewise there is no StoreSubFpImm / StoreDivFpImm opcode (instruction.rs:343-356: 4 add, 6 mul; 5 and 7
  are unassigned), the felt immediate cases are addi / muli / store_imm.
* ``U32StoreEqFpFp`` / ``U32StoreEqFpImm``: not emitted, see ``all_opcodes_program``.
* division by zero: the reference RUNNER refuses it (crates/runner/src/vm/instructions/store.rs:362-366, :412-416) while the
  prover's witness maps it to (0, 0) (u32_store_div_fp_fp.rs:362-364); no valid program contains it, so it lives in
  ``div_by_zero_program()``, which is witness-only (its rows do not satisfy the constraints).
"""
from cairo_m_amd.workloads import (ADD, ADDI, ASSERT_EQ, CALL, DDEREF, DDEREF_FF, DIV, JMPR, JNZ, LE, MUL, MULI, RET, SFP, STOREI, SUB,
                                   TO_DDEREF, TO_DDEREF_FF, U_ADD, U_ADDI, U_AND, U_ANDI, U_DIV, U_DIVI, U_IMM, U_LT, U_LTI, U_MUL,
                                   U_MULI, U_OR, U_ORI, U_SUB, U_XOR, U_XORI, Asm, P)

M32 = 0xFFFFFFFF
# opcode -> air::ComponentId (components/opcodes/mod.rs:223-268)
COMPONENT_OF = {ASSERT_EQ: 0, CALL: 1, 12: 2, JMPR: 2, JNZ: 3, RET: 4, STOREI: 5, ADD: 6, SUB: 6, MUL: 6, DIV: 6, ADDI: 7, MULI: 7,
                DDEREF: 8, TO_DDEREF: 8, DDEREF_FF: 9, TO_DDEREF_FF: 9, SFP: 10, U_IMM: 11, U_ADDI: 12, U_MULI: 13, U_DIVI: 14,
                U_LTI: 17, U_LT: 18, U_ADD: 19, U_SUB: 20, U_MUL: 21, U_DIV: 22, U_AND: 23, U_OR: 23, U_XOR: 23,
                U_ANDI: 24, U_ORI: 24, U_XORI: 24, LE: 25}
# edge-name prefix -> opcode
EDGE_OPS = {"u_add_ff": U_ADD, "u_add_fi": U_ADDI, "u_sub_ff": U_SUB, "u_mul_ff": U_MUL, "u_mul_fi": U_MULI,
            "u_div_ff": U_DIV, "u_div_fi": U_DIVI, "u_lt_ff": U_LT, "u_lt_fi": U_LTI,
            "u_and_ff": U_AND, "u_or_ff": U_OR, "u_xor_ff": U_XOR, "u_and_fi": U_ANDI, "u_or_fi": U_ORI, "u_xor_fi": U_XORI,
            "u_imm": U_IMM, "add": ADD, "sub": SUB, "mul": MUL, "div": DIV, "addi": ADDI, "muli": MULI, "store_imm": STOREI,
            "le": LE, "jnz": JNZ, "jmp_rel": JMPR, "call": CALL, "dderef_fi_load": DDEREF, "dderef_fi_store": TO_DDEREF,
            "dderef_ff_load": DDEREF_FF, "dderef_ff_store": TO_DDEREF_FF, "sfp": SFP}

U_ADD_CASES = [(0, 0), (0xFFFF, 1), (0xFFFF0000, 0x10000), (M32, 1), (M32, M32), (0xFFFEFFFE, 0x10001)]   # the last: both limb sums = 0xFFFF
U_SUB_CASES = [(0, 1), (0x10000, 1), (0x12345678, 0x12345678)]
U_MUL_CASES = [(0, 0x89ABCDEF), (M32, M32), (0x10000, 0x10000), (0xFFFF, 0xFFFF), (0xFF, 0x101)]
# (n, d, tag): q * d + r = n in 8-bit limbs, borrow comparisons d_lo < r_lo + 1, d_hi < r_hi + borrow
U_DIV_CASES = [(0x12345678, 1, "d=1"), (0x12345678, M32, "d=max"), (5, 7, "n<d"), (0x12345678, 0x12345678, "n=d"),
               (M32, 0xFF, "n=max"), (M32, 0x100, "n=max"), (M32, 0x10000, "n=max"), (M32, 0x10001, "n=max"),
               (0x7FFFF, 0x20000, "r_lo=ffff,d_lo=0"), (0x7000F, 0x30005, "r_lo=d_lo,r_hi<d_hi"), (1999, 1000, "r=d-1"),
               (0x8FFFF, 0x30000, "r=d-1"), (0, 7, "n=0"), (0xFFFF, 0x10000, "r_lo=ffff,d_lo=0"), (0x10000, 3, "q*d+r carries at 0x10000")]
U_LT_CASES = [(5, 5, "eq"), (0x89ABCDEF, 0x89ABCDEF, "eq"), (0x10002, 0x10003, "lo"), (0x10003, 0x10002, "lo"),
              (0x20001, 0x30001, "hi"), (0x30001, 0x20001, "hi"), (0x1FFFF, 0x20000, "hi<,lo>"), (0x20000, 0x1FFFF, "hi>,lo<"),
              (0, M32, "ends"), (M32, 0, "ends")]
U_BIT_CASES = [(0xDEADBEEF, 0xDEADBEEF, "x,x"), (0xDEADBEEF, 0xDEADBEEF ^ M32, "x,~x"), (0, M32, "0,max"), (M32, 0, "max,0"),
               (0x00FF00FF, 0xFF00FF00, "bytes"), (0xFF00FF00, 0xFF00FF00, "bytes")]
U_IMM_CASES = [(0, 0), (0xFFFF, 0xFFFF)]
X = 0x1234567
FELT_CASES = [("add", P - 1, 1), ("add", 0, 0), ("add", P - 1, P - 1), ("sub", 0, 1), ("sub", X, X), ("sub", 0, P - 1),
              ("mul", P - 1, P - 1), ("mul", 0, X), ("div", X, 1), ("div", X, P - 1), ("div", X, X), ("div", 0, X)]
FELT_IMM_CASES = [("addi", P - 1, 1), ("addi", X, 0), ("addi", X, P - 1), ("addi", 0, 0),
                  ("muli", P - 1, P - 1), ("muli", X, 0), ("muli", X, 1), ("muli", 0, P - 1)]
STORE_IMM_CASES = [0, P - 1]
P3H, P2H = ((P // 3) >> 16) + 1, ((P // 2) >> 16) + 1     # PRIME_OVER_3_HIGH / PRIME_OVER_2_HIGH (store_le_fp_imm.rs:132-133)
T3 = (P - 1) // 3                                         # 715827882: 3 * T3 = P - 1
# (src, imm, tag): the component orders (src, imm) into a <= b and keeps the two shorter of the arcs a, b - a, P - 1 - b
LE_CASES = [(7, 7, "a=b"), (0, 5, "a=0"), (5, P - 1, "b=P-1"), (0, 0, "a=b=0"), (P - 1, P - 1, "a=b=P-1"), (0, P - 1, "a=0,b=P-1"),
            (1000, 2000, "tie01 short"), (1000, P - 1 - 1000, "tie02 short"), (2, 1 << 30, "tie12 long"),
            (T3 + 1, 2 * T3 + 2, "tie01 long"), ((1 << 30) - 1, (1 << 30) - 1, "tie02 long"), (T3, 2 * T3, "tie012"),
            (3 * P3H, 3 * P3H + 5 * P2H, "short=k*P3H,long=k*P2H"), (3 * P3H - 1, 3 * P3H - 1 + 5 * P2H - 1, "one below"),
            (P - 1 - 5 * P2H, P - 1 - 3 * P3H, "arcs 1,2 kept"),
            (2000, 1000, "gt tie01 short"), (P - 1, 0, "gt a=0,b=P-1"), (2 * T3, T3, "gt tie012"), (8, 7, "gt by one"),
            (1 << 30, 2, "gt tie12 long")]


class _Gen:
    def __init__(self):
        self.a = Asm()
        self.next = 0
        self.exec = []           # (component id, opcode, position in the order of execution, edge name or None)
        self.steps = 0

    def slot(self, n=1):
        s = self.next
        self.next += n
        return s

    def emit(self, *words, edge=None, executed=True, runs_after=None):
        """runs_after: the executed-list index of the instruction this one runs right after, where the text order differs from
        the order of execution (the backward jump)"""
        self.a.emit(*words)
        if executed:
            key = len(self.exec) if runs_after is None else runs_after + 0.5
            self.exec.append((COMPONENT_OF[words[0]], words[0], key, edge))
            self.steps += 1

    def count(self, cid):
        return sum(1 for e in self.exec if e[0] == cid)

    def edges(self):
        """(name, component id, live row): a component's rows are its instructions grouped by opcode (ascending), each group in
        the order of execution — the order the adapter hands the bundles over in (the reference groups the states by opcode: crates/prover/src/adapter/mod.rs:108-129)"""
        out = []
        for cid in sorted({e[0] for e in self.exec}):
            rows = sorted((e for e in self.exec if e[0] == cid), key=lambda e: (e[1], e[2]))
            out += [(e[2], e[3], cid, r) for r, e in enumerate(rows) if e[3] is not None]
        return [(name, cid, r) for _, name, cid, r in sorted(out)]

    def felt(self, v):
        s = self.slot()
        self.emit(STOREI, v % P, s)
        return s

    def u32(self, v):
        s = self.slot(2)
        self.emit(U_IMM, v & 0xFFFF, v >> 16, s)
        return s


def _name(op, a, b, tag=None):
    return f"{op}:{a:x},{b:x}" + (f"#{tag}" if tag else "")


def edge_program():
    g = _Gen()
    lo, hi = (lambda v: v & 0xFFFF), (lambda v: v >> 16)
    # ---- u32 arithmetic, fp_fp and fp_imm
    for op_ff, op_fi, cases in (("u_add_ff", "u_add_fi", U_ADD_CASES), ("u_sub_ff", None, U_SUB_CASES), ("u_mul_ff", "u_mul_fi", U_MUL_CASES)):
        for x, y in cases:
            sx, sy = g.u32(x), g.u32(y)
            g.emit(EDGE_OPS[op_ff], sx, sy, g.slot(2), edge=_name(op_ff, x, y))
            if op_fi:
                g.emit(EDGE_OPS[op_fi], sx, lo(y), hi(y), g.slot(2), edge=_name(op_fi, x, y))
    for n, d, tag in U_DIV_CASES:
        sn, sd = g.u32(n), g.u32(d)
        g.emit(U_DIV, sn, sd, g.slot(2), g.slot(2), edge=_name("u_div_ff", n, d, tag))
        g.emit(U_DIVI, sn, lo(d), hi(d), g.slot(2), g.slot(2), edge=_name("u_div_fi", n, d, tag))
    for x, y, tag in U_LT_CASES:
        sx, sy = g.u32(x), g.u32(y)
        g.emit(U_LT, sx, sy, g.slot(), edge=_name("u_lt_ff", x, y, tag))
        g.emit(U_LTI, sx, lo(y), hi(y), g.slot(), edge=_name("u_lt_fi", x, y, tag))
    for x, y, tag in U_BIT_CASES:
        sx, sy = g.u32(x), g.u32(y)
        for k in ("and", "or", "xor"):
            g.emit(EDGE_OPS[f"u_{k}_ff"], sx, sy, g.slot(2), edge=_name(f"u_{k}_ff", x, y, tag))
            g.emit(EDGE_OPS[f"u_{k}_fi"], sx, lo(y), hi(y), g.slot(2), edge=_name(f"u_{k}_fi", x, y, tag))
    for l, h in U_IMM_CASES:
        g.emit(U_IMM, l, h, g.slot(2), edge=_name("u_imm", l, h))
    # ---- felt
    for k, x, y in FELT_CASES:
        sx, sy = g.felt(x), g.felt(y)
        g.emit(EDGE_OPS[k], sx, sy, g.slot(), edge=_name(k, x, y))
    for k, x, imm in FELT_IMM_CASES:
        g.emit(EDGE_OPS[k], g.felt(x), imm, g.slot(), edge=_name(k, x, imm))
    for v in STORE_IMM_CASES:
        g.emit(STOREI, v, g.slot(), edge=_name("store_imm", v, 0))
    for src, imm, tag in LE_CASES:
        g.emit(LE, g.felt(src), imm, g.slot(), edge=_name("le", src, imm, tag))
    # ---- jnz on 0 (falls through), 1 and P-1 (taken, skipping one instruction)
    for i, c in enumerate((0, 1, P - 1)):
        sc, t = g.felt(c), g.slot()
        g.emit(JNZ, sc, ("rel", f"jnz{i}"), edge=_name("jnz", c, 0))
        g.emit(STOREI, 77, t, executed=(c == 0))
        g.a.label(f"jnz{i}")
    # ---- a backward relative jump: fwd -> L2, L2 jumps back to L1 (offset P - 2), L1 -> L3
    t = g.slot()
    first = len(g.exec)
    g.emit(JMPR, ("rel", "L2"))
    g.a.label("L1")
    g.emit(STOREI, 1, t)
    g.emit(JMPR, ("rel", "L3"))                       # runs third
    g.a.label("L2")
    g.emit(JMPR, ("rel", "L1"), edge=_name("jmp_rel", P - 2, 0, "backward"), runs_after=first)      # runs second
    g.a.label("L3")
    # ---- double_deref, both forms, offsets 0 and -3; store_frame_pointer offsets 0 and -2
    cell = g.slot(4)                                  # cell .. cell + 3: targets of the dereferences
    for k in range(4):
        g.emit(STOREI, 100 + k, cell + k)
    ptr = g.slot()
    g.emit(SFP, cell + 3, ptr)                        # [ptr] = fp + cell + 3
    off0, offm = g.felt(0), g.felt(P - 3)
    g.emit(DDEREF, ptr, 0, g.slot(), edge=_name("dderef_fi_load", 0, 0))
    g.emit(DDEREF, ptr, P - 3, g.slot(), edge=_name("dderef_fi_load", P - 3, 0, "negative"))
    v = g.felt(555)
    g.emit(TO_DDEREF, ptr, 0, v, edge=_name("dderef_fi_store", 0, 0))
    g.emit(TO_DDEREF, ptr, P - 3, v, edge=_name("dderef_fi_store", P - 3, 0, "negative"))
    g.emit(DDEREF_FF, ptr, off0, g.slot(), edge=_name("dderef_ff_load", 0, 0))
    g.emit(DDEREF_FF, ptr, offm, g.slot(), edge=_name("dderef_ff_load", P - 3, 0, "negative"))
    g.emit(TO_DDEREF_FF, ptr, off0, v, edge=_name("dderef_ff_store", 0, 0))
    g.emit(TO_DDEREF_FF, ptr, offm, v, edge=_name("dderef_ff_store", P - 3, 0, "negative"))
    g.emit(SFP, 0, g.slot(), edge=_name("sfp", 0, 0))
    g.emit(SFP, P - 2, g.slot(), edge=_name("sfp", P - 2, 0, "negative"))
    # ---- live-row counts: assert_eq exactly 1, store_frame_pointer exactly 16, jnz exactly 17 (plain repeats)
    g.emit(ASSERT_EQ, g.felt(P - 1), P - 1)
    while g.count(COMPONENT_OF[SFP]) < 16:
        g.emit(SFP, 1, g.slot())
    zero = g.felt(0)
    while g.count(COMPONENT_OF[JNZ]) < 17:
        g.emit(JNZ, zero, 1)
    # ---- a call nested two deep (the callees' frames start past every cell used above)
    frame = g.slot(16)
    g.emit(CALL, frame, ("abs", "f1"), edge=_name("call", 1, 0, "depth 1"))
    g.emit(RET)                                                                # main's, runs last
    g.a.label("f1")
    g.emit(CALL, 4, ("abs", "f2"), edge=_name("call", 2, 0, "depth 2"))
    g.emit(RET)
    g.a.label("f2")
    g.emit(STOREI, 9, 0)
    g.emit(RET)
    a = g.a
    assert g.steps < 4096
    return a.build(), g.steps, g.edges()


def div_by_zero_program(n=0x12345678):
    """U_DIV and U_DIVI with d = 0: the two rows no valid run contains.  Returns (program, steps, edges)."""
    g = _Gen()
    sn, sd = g.u32(n), g.u32(0)
    g.emit(U_DIV, sn, sd, g.slot(2), g.slot(2), edge=_name("u_div_ff", n, 0, "d=0"))
    g.emit(U_DIVI, sn, 0, 0, g.slot(2), g.slot(2), edge=_name("u_div_fi", n, 0, "d=0"))
    g.emit(RET)
    return g.a.build(), g.steps, g.edges()
