"""Hand-built runner segments for the adapters, and a second reference of `import_from_runner_output`.

The adapter never executes anything: it needs a trace of (pc, fp), a memory log whose per-step entry counts match the opcode
fetched at pc, and the memory at segment start.  `build` / `build_arrays` lay such a segment out directly in numpy, so a test can
put any clock gap and any address pattern where it wants it, at adapter cost.

`reference` restates crates/prover/src/adapter (mod.rs:97-193, memory.rs:427-535) in plain numpy and shares nothing with the
library's two adapters (host_adapter.hpp import_segment, adapter_device.hip): a stable argsort of the log by address makes the
predecessor in that order the previous access; the clock-update loop of memory.rs:511-525 is written out as is.  Only the two
partial Merkle trees come from the library (cm_adapter_partial_tree, pinned to merkle.rs by tests/test_adapter.py).

No test functions here: tests/test_adapter_segments_cpu.py, tests/test_gpu_adapter_segments.py and tests/test_gpu_run_segments.py
import this module."""
import functools

import numpy as np

P = 2**31 - 1
LIMIT = (1 << 20) - 1            # RC20_LIMIT: the largest clock difference one memory access may span
MAX_ADDRESS = (1 << 28) - 1
M31_NEG1 = P - 1
N_COMPONENTS = 26

# opcode -> (size in M31 words, operand accesses), crates/common/src/instruction.rs:314-577, as data
OPCODES = {
    0: (4, 3), 1: (4, 3), 2: (4, 3), 3: (4, 3), 4: (4, 2), 6: (4, 2), 8: (4, 3), 9: (3, 1), 10: (3, 2), 11: (1, 2), 12: (2, 0),
    13: (2, 0), 14: (3, 1), 15: (4, 6), 16: (4, 6), 17: (4, 6), 18: (5, 8), 19: (5, 4), 21: (5, 4), 22: (6, 6), 23: (4, 2),
    24: (4, 5), 28: (4, 5), 30: (5, 3), 34: (5, 3), 36: (4, 6), 37: (4, 6), 38: (4, 6), 39: (5, 4), 40: (5, 4), 41: (5, 4),
    42: (4, 4), 43: (3, 1), 44: (4, 3), 45: (4, 4), 48: (4, 2), 50: (3, 1),
}
# the opcode groups of define_opcodes! (components/opcodes/mod.rs:223-268) in macro order: component k = group k
GROUPS = [[50], [10], [12, 13], [14], [11], [9], [0, 1, 2, 3], [4, 6], [8, 44], [42, 45], [43], [23], [19], [21], [22], [24], [30],
          [34], [28], [15], [16], [17], [18], [36, 37, 38], [39, 40, 41], [48]]
assert len(GROUPS) == N_COMPONENTS and sorted(o for g in GROUPS for o in g) == sorted(OPCODES)
COMPONENT = {op: c for c, g in enumerate(GROUPS) for op in g}

SIZE = np.zeros(64, dtype=np.int64)
ACC = np.zeros(64, dtype=np.int64)
COMP = np.full(64, -1, dtype=np.int64)
for _op, (_s, _a) in OPCODES.items():
    SIZE[_op], ACC[_op], COMP[_op] = _s, _a, COMPONENT[_op]
ENTRIES = np.where(COMP >= 0, 1 + (SIZE > 4) + ACC, 0)      # log entries of one step; 0 = not an opcode


class Segment:
    """trace (n + 1, 2) (pc, fp); log (m, 5) (address, value[4]); image (k, 4) = the locals at segment start; heap (h, 4), index i =
    the cell at MAX_ADDRESS - i; ranges = program, input, output [start, end)."""

    def __init__(self, trace, log, image, heap, ranges, **info):
        u = lambda a, w: np.ascontiguousarray(np.asarray(a, dtype=np.uint32).reshape(-1, w))
        self.trace, self.log, self.image, self.heap = u(trace, 2), u(log, 5), u(image, 4), u(heap, 4)
        self.ranges = [int(x) for x in ranges]
        self.info = info

    def copy(self, **kw):
        d = dict(trace=self.trace.copy(), log=self.log.copy(), image=self.image.copy(), heap=self.heap.copy(), ranges=list(self.ranges))
        d.update(kw)
        return Segment(d["trace"], d["log"], d["image"], d["heap"], d["ranges"], **self.info)

    def array_segment(self):
        from cairo_m_amd.lib import ArraySegment
        return ArraySegment(self.trace, self.log, self.image, self.heap, self.ranges)

    @property
    def n_steps(self):
        return self.trace.shape[0] - 1


NO_RANGES = (0, 0, 0, 0, 0, 0)


def build_arrays(pc, fp, cells, acc, image, heap=(), ranges=NO_RANGES, final=None, **info):
    """Vectorised builder.  pc, fp: (n,); cells: (n, 8) = the four words of the cell at pc, then the four words of the cell at
    pc + 1 (read only by 5/6-word instructions); acc: (sum of the steps' operand accesses, 5) in step order.  The log gets one
    fetch entry at pc, one more at pc + 1 for 5/6-word instructions, then the operand entries; the image gets every instruction
    at its pc (the FIRST step that runs a pc wins: a later step may log other words, see rewritten_code)."""
    pc, fp = np.asarray(pc, dtype=np.int64), np.asarray(fp, dtype=np.int64)
    cells = np.asarray(cells, dtype=np.int64).reshape(-1, 8)
    acc = np.asarray(acc, dtype=np.int64).reshape(-1, 5)
    n = pc.shape[0]
    op = cells[:, 0]
    assert (op < 64).all() and (COMP[op] >= 0).all(), "the builder only lays out opcodes of its table"
    two = SIZE[op] > 4
    ne = ENTRIES[op]
    off = np.cumsum(ne) - ne
    m = int(ne.sum())
    assert acc.shape[0] == int(ACC[op].sum()), (acc.shape[0], int(ACC[op].sum()))
    log = np.zeros((m, 5), dtype=np.int64)
    operand = np.ones(m, dtype=bool)
    log[off, 0], log[off, 1:] = pc, cells[:, :4]
    operand[off] = False
    log[off[two] + 1, 0], log[off[two] + 1, 1:] = pc[two] + 1, cells[two, 4:]
    operand[off[two] + 1] = False
    log[operand] = acc
    image = np.array(image, dtype=np.int64).reshape(-1, 4)
    inside = pc < image.shape[0]
    image[pc[inside][::-1]] = cells[inside][::-1, :4]
    t2 = two & (pc + 1 < image.shape[0])
    image[pc[t2][::-1] + 1] = cells[t2][::-1, 4:]
    final = (pc[-1], fp[-1]) if final is None else final
    trace = np.concatenate([np.stack([pc, fp], axis=1), np.array([final], dtype=np.int64)])
    assert log.max(initial=0) < 2**32 and (log[:, 1:] < P).all(), "log words are canonical M31"
    return Segment(trace, log, image, np.array(heap, dtype=np.int64).reshape(-1, 4), ranges, **info)


def build(steps, image, heap=(), ranges=NO_RANGES, final=None, **info):
    """steps: [(pc, fp, instruction words, [(address, value4), ...]), ...]; instruction words = 1..6 words, opcode first (up to 8
    to put words into the unused part of the second cell).  value4 = four words, or one word for (v, 0, 0, 0)."""
    n = len(steps)
    pc, fp, cells, acc = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64), np.zeros((n, 8), dtype=np.int64), []
    for t, (p, f, words, accesses) in enumerate(steps):
        pc[t], fp[t] = p, f
        cells[t, :len(words)] = words
        assert len(accesses) == OPCODES[words[0]][1], (t, words, len(accesses))
        for a, v in accesses:
            v = list(v) if hasattr(v, "__len__") else [v, 0, 0, 0]
            acc.append([a] + v)
    return build_arrays(pc, fp, cells, acc, image, heap, ranges, final, **info)


# ---- the reference -----------------------------------------------------------------------------------------------------------
class Refused(ValueError):
    """the segment is not a runner output (the message names why, in the adapters' words)"""


def step_offsets(seg):
    """every step's first log entry, by the LOG's own opcodes (the log is the adapter's contract)"""
    n, m = seg.n_steps, seg.log.shape[0]
    w0 = seg.log[:, 1].astype(np.int64)
    ne = np.where(w0 < 64, ENTRIES[np.minimum(w0, 63)], 0).tolist()
    off, e = [], 0
    for _ in range(n):
        if e >= m:
            raise Refused("memory trace length does not match the instructions executed")
        if ne[e] == 0:
            raise Refused("invalid opcode")
        off.append(e)
        e += ne[e]
    if e != m:
        raise Refused("memory trace length does not match the instructions executed")
    off = np.array(off, dtype=np.int64)
    if not np.array_equal(seg.log[off, 0], seg.trace[:n, 0]):
        raise Refused("a step's first memory entry is not the instruction fetch at pc")
    return off


def _links(seg, off):
    """per log entry: clock, previous access (entry index or -1), the cell's initial value (image, heap, else the first logged)"""
    n, m = seg.n_steps, seg.log.shape[0]
    log = seg.log.astype(np.int64)
    op = log[off, 1]
    clock = np.repeat(np.arange(n, dtype=np.int64), ENTRIES[op]) + 1
    addr = log[:, 0]
    order = np.argsort(addr, kind="stable")
    sa = addr[order]
    head = np.ones(m, dtype=bool)
    head[1:] = sa[1:] != sa[:-1]
    prev_e = np.full(m, -1, dtype=np.int64)
    prev_e[order[1:]] = np.where(head[1:], -1, order[:-1])
    head_pos = np.maximum.accumulate(np.where(head, np.arange(m), 0))
    first_e = np.empty(m, dtype=np.int64)
    first_e[order] = order[head_pos]
    k, h = seg.image.shape[0], seg.heap.shape[0]
    in_lo = addr < k
    hidx = MAX_ADDRESS - addr
    in_hi = ~in_lo & (hidx >= 0) & (hidx < h)
    init4 = log[first_e, 1:5].copy()
    init4[in_lo] = seg.image[addr[in_lo]]
    init4[in_hi] = seg.heap[hidx[in_hi]]
    return dict(log=log, op=op, clock=clock, addr=addr, order=order, head=head, prev_e=prev_e, init4=init4, known=in_lo | in_hi)


def sorted_layout(seg):
    """(sorted addresses, head flags) of the log in the order both adapters' previous-access rule implies: for the coverage
    assertions on wave / block boundaries"""
    L = _links(seg, step_offsets(seg))
    return L["addr"][L["order"]], L["head"]


def reference(seg):
    """-> the dict cairo_m_amd.lib.prover_input_arrays returns for this segment's ProverInput"""
    from cairo_m_amd.lib import partial_merkle_tree
    n = seg.n_steps
    if n < 1:
        raise Refused("empty trace")
    off = step_offsets(seg)
    L = _links(seg, off)
    log, op, clock, addr, prev_e, init4 = L["log"], L["op"], L["clock"], L["addr"], L["prev_e"], L["init4"]
    m = log.shape[0]
    has_prev = prev_e >= 0
    prev_clock = np.where(has_prev, clock[prev_e], 0)
    prev_v0 = np.where(has_prev, log[prev_e, 1], init4[:, 0])
    # ---- Memory::push, memory.rs:511-525, for the entries it can apply to, in log order ----
    clock_updates = []
    adjusted = prev_clock.copy()
    for e in np.nonzero(clock - prev_clock > LIMIT)[0].tolist():
        current_clk, prev_clk = int(clock[e]), int(prev_clock[e])
        if current_clk > prev_clk:
            delta = current_clk - prev_clk
            if delta > LIMIT:
                num_steps = delta // LIMIT
                for _ in range(num_steps):
                    clock_updates.append([int(addr[e]), prev_clk] + init4[e].tolist())
                    prev_clk += LIMIT
        adjusted[e] = prev_clk
    # ---- data accesses and bundles (mod.rs:118-166) ----
    size, na = SIZE[op], ACC[op]
    two = size > 4
    operand = np.ones(m, dtype=bool)
    operand[off] = False
    operand[off[two] + 1] = False
    data_accesses = np.stack([addr, adjusted, prev_v0, log[:, 1]], axis=1)[operand]
    c0 = log[off, 1:5]
    c1 = np.zeros((n, 4), dtype=np.int64)
    c1[two] = log[off[two] + 1, 1:5]
    rows = np.zeros((n, 12), dtype=np.int64)
    rows[:, 0], rows[:, 1], rows[:, 2], rows[:, 3] = seg.trace[:n, 0], seg.trace[:n, 1], np.arange(n) + 1, adjusted[off]
    for k in range(4):
        rows[:, 4 + k] = np.where(k < size, c0[:, k], 0)
    rows[:, 8], rows[:, 9] = np.where(size > 4, c1[:, 0], 0), np.where(size > 5, c1[:, 1], 0)
    rows[:, 10], rows[:, 11] = np.cumsum(na) - na, na
    out = {"regs": [int(x) for x in (seg.trace[0, 0], seg.trace[0, 1], seg.trace[n, 0], seg.trace[n, 1])], "ranges": list(seg.ranges)}
    comp = COMP[op]
    for c in range(N_COMPONENTS):
        sel = np.nonzero(comp == c)[0]
        sel = sel[np.argsort(op[sel], kind="stable")]          # variants in ascending opcode, step order inside one
        out[f"bundles{c}"] = rows[sel].astype(np.uint32)
    out["data_accesses"] = data_accesses.astype(np.uint32).reshape(-1, 4)
    out["clock_updates"] = np.array(clock_updates, dtype=np.uint32).reshape(-1, 6)
    # ---- boundary memory: Memory::new + the touched cells, update_multiplicities (memory.rs:427-461), ascending address ----
    order, head = L["order"], L["head"]
    tail = np.ones(m, dtype=bool)
    tail[:-1] = head[1:]
    t_addr, t_first, t_last = addr[order[head]], order[head], order[tail]
    k, h = seg.image.shape[0], seg.heap.shape[0]
    if k + h > MAX_ADDRESS + 1:
        raise Refused("locals and heap overlap")
    A = np.unique(np.concatenate([np.arange(k, dtype=np.int64), MAX_ADDRESS - np.arange(h, dtype=np.int64), t_addr]))
    init = np.zeros((A.shape[0], 7), dtype=np.int64)
    init[:, 0] = A
    lo, hi = A < k, (A >= k) & (MAX_ADDRESS - A < h)
    init[lo, 1:5] = seg.image[A[lo]]
    init[hi, 1:5] = seg.heap[MAX_ADDRESS - A[hi]]
    ti = np.searchsorted(A, t_addr)
    new = ~(lo | hi)[ti]
    init[ti[new], 1:5] = log[t_first[new], 1:5]
    init[ti, 6] = 1
    fin = init.copy()
    fin[:, 6] = 0
    fin[ti, 1:5], fin[ti, 5], fin[ti, 6] = log[t_last, 1:5], clock[t_last], M31_NEG1
    r = seg.ranges
    for s, e in ((r[0], r[1]), (r[2], r[3])):
        sel = (A >= s) & (A < e)
        init[sel, 6] = 0
        fin[sel & (fin[:, 6] == 0), 6] = M31_NEG1
    sel = (A >= r[4]) & (A < r[5])
    fin[sel, 6] = 0
    init[sel, 6] = 1
    out["initial_memory"], out["final_memory"] = init.astype(np.uint32), fin.astype(np.uint32)
    out["initial_tree"], root_i = partial_merkle_tree(init[:, :5], True, r)
    out["final_tree"], root_f = partial_merkle_tree(fin[:, :5], False, r)
    out["roots"] = [int(root_i), int(root_f)]
    return out


def public_entries(ref):
    """make_public_data over the reference's rows: program and input from the initial rows, output from the final ones; seven
    words per address of a range (present, address, value[4], clock), zero where the boundary memory has no such cell"""
    r = ref["ranges"]

    def take(rows, s, e):
        out = np.zeros((max(e - s, 0), 7), dtype=np.uint32)
        sel = (rows[:, 0] >= s) & (rows[:, 0] < e)
        j = rows[sel, 0] - s
        out[j, 0], out[j, 1], out[j, 2:6], out[j, 6] = 1, rows[sel, 0], rows[sel, 1:5], rows[sel, 5]
        return out
    return {"program": take(ref["initial_memory"], r[0], r[1]), "input": take(ref["initial_memory"], r[2], r[3]),
            "output": take(ref["final_memory"], r[4], r[5])}


def image_after(seg, n_memory_end, n_heap_end):
    """the memory a run carries into the next segment: each region grown (with zeros) to its end length, every touched cell inside
    a region at its last logged value"""
    lo = np.zeros((n_memory_end, 4), dtype=np.uint32)
    hi = np.zeros((n_heap_end, 4), dtype=np.uint32)
    lo[:seg.image.shape[0]] = seg.image
    hi[:seg.heap.shape[0]] = seg.heap
    for a, *v in seg.log.tolist():                      # (log order: the last write wins)
        if a < n_memory_end:
            lo[a] = v
        elif MAX_ADDRESS - a < n_heap_end:
            hi[MAX_ADDRESS - a] = v
    return lo, hi


# ---- the segments ------------------------------------------------------------------------------------------------------------
def _values(rng, n):
    """n cells of canonical M31 words; every word is live, so that a value taken from the wrong entry shows"""
    return rng.integers(1, P, size=(n, 4), dtype=np.int64)


LADDER_DELTAS = (LIMIT - 1, LIMIT, LIMIT + 1, 2 * LIMIT - 1, 2 * LIMIT, 2 * LIMIT + 1)
LADDER_STEPS = 2 * LIMIT + 300
LADDER_IMAGE, LADDER_HEAP, LADDER_END = 64, 32, 10_000     # cells of the locals / heap at start; the locals at the end (for a run)


def expected_updates(delta):
    return delta // LIMIT if delta > LIMIT else 0


@functools.lru_cache(maxsize=1)
def gap_ladder():
    """2 * LIMIT + 300 steps: filler steps (opcode 12, no operand) alternating between pc 0 and pc 1, and probe steps that touch one
    dedicated cell per (class, delta).  clock = step + 1.  info["cells"][(class, delta)] = [(address, expected updates), ...]."""
    rng = np.random.default_rng(20)
    n = LADDER_STEPS
    t = np.arange(n, dtype=np.int64)
    pc = t & 1
    cells = np.zeros((n, 8), dtype=np.int64)
    cells[:, 0], cells[:, 1] = 12, 1 - pc
    fp = np.full(n, 7, dtype=np.int64)
    image = np.zeros((LADDER_IMAGE, 4), dtype=np.int64)
    image[40:52] = _values(rng, 12)
    heap = _values(rng, LADDER_HEAP)
    probes, cover = {}, {}
    HOT = 0                                             # an operand nobody looks at goes to the filler's own cell: never idle

    def probe(clock, p, words, accesses):
        assert 1 <= clock <= n and clock not in probes, clock
        probes[clock] = (p, words, [(a, _values(rng, 1)[0]) for a in accesses])

    P1, P2, P3 = 2, 3, 4                                # shared probe instructions: 1, 2 and 3 operand accesses
    for i, d in enumerate(LADDER_DELTAS):
        k = expected_updates(d)
        # (a) a local with a non-zero initial value, (c) a heap cell, (d) a cell outside the image: first touched at clock == delta
        a, c, dd = 40 + i, MAX_ADDRESS - (3 + i), 9000 + 3 * i
        probe(d, P3, [0, 1, 2, 3], [a, c, dd])
        cover[("a", d)], cover[("c", d)], cover[("d", d)] = [(a, k)], [(c, k)], [(dd, k)]
        # (b) a cell between the regions: first access, second `delta` later with another value
        c0, b = 4 * (1 + i), 5000 + 10 * i
        probe(c0, P1, [9, 5, 6], [b])
        probe(c0 + d, P1, [9, 5, 6], [b])
        cover[("b", d)] = [(b, k)]
        if d == LIMIT + 1:                              # ... a third a further LIMIT + 1 later with a third value: one update more
            probe(c0 + d + LIMIT + 1, P1, [9, 5, 6], [b])
            cover[("b", d)] = [(b, 2)]
            for j in range(70):                         # neighbours touched many times in between (bisection lands on the head)
                probe(1002 + 4 * j, P2, [4, 1, 2, 3], [b - 1, b + 1])
        # (c2) a heap cell touched twice, `delta` apart
        c0, c2 = 4 * (7 + i), MAX_ADDRESS - (12 + i)
        probe(c0, P1, [9, 5, 6], [c2])
        probe(c0 + d, P1, [9, 5, 6], [c2])
        cover[("c2", d)] = [(c2, k)]
        # (e) the fetch cell of a one-word instruction (ret) executed `delta` apart: inst_prev_clock
        c0, e = 4 * (13 + i), 10 + i
        probe(c0, e, [11], [HOT, HOT])
        probe(c0 + d, e, [11], [HOT, HOT])
        cover[("e", d)] = [(e, k)]
        # (f) a six-word instruction executed `delta` apart: both instruction cells fall due
        c0, f = 4 * (19 + i), 20 + 2 * i
        probe(c0, f, [22, 1, 2, 3, 4, 5], [HOT] * 6)
        probe(c0 + d, f, [22, 1, 2, 3, 4, 5], [HOT] * 6)
        cover[("f", d)] = [(f, k), (f + 1, k)]
    # (g) one step touching the same cell twice: the second access has delta 0 (early, and on a cell first touched after LIMIT)
    probe(50, P2, [4, 1, 2, 3], [7000, 7000])
    probe(LIMIT + 6, P2, [4, 1, 2, 3], [7001, 7001])
    cover[("g", 0)] = [(7000, 0), (7001, 1)]
    # (h) two probes in one step, the higher address first, and a later step's probe at a still lower address: log order is the
    # reverse of address order
    probe(LIMIT + 10, P2, [4, 1, 2, 3], [8002, 8001])
    probe(LIMIT + 14, P1, [9, 5, 6], [8000])
    cover[("h", LIMIT + 10)] = [(8002, 1), (8001, 1), (8000, 1)]
    acc = []
    for clock in sorted(probes):
        p, words, accesses = probes[clock]
        pc[clock - 1] = p
        cells[clock - 1] = 0
        cells[clock - 1, :len(words)] = words
        acc += [[a] + v.tolist() for a, v in accesses]
    return build_arrays(pc, fp, cells, acc, image, heap, (0, 32, 40, 43, 43, 46), cells_by_class=cover)


def ladder_update_counts(ref):
    """address -> clock-update rows the reference emits for it"""
    a, c = np.unique(ref["clock_updates"][:, 0], return_counts=True)
    return dict(zip(a.tolist(), c.tolist()))


LAYOUT_SIZES = (1, 2, 63, 64, 65, 255, 256, 257, 1000, 4099)
LAYOUT_IMAGE, LAYOUT_HEAP = 160, 16


def layout_mix(n_steps, seed=None):
    """a seeded mix of every opcode of the table (each at its own pc, all of them present from 37 steps up); operand addresses from
    a small pool just above the image (long runs), a 27-bit pool and the heap; fp, values and the unused instruction words random"""
    rng = np.random.default_rng(1000 + n_steps if seed is None else seed)
    ops = np.array(sorted(OPCODES), dtype=np.int64)
    op = rng.choice(ops, size=n_steps)
    if n_steps >= ops.size:
        op[:ops.size] = rng.permutation(ops)
    pc = 2 * np.searchsorted(ops, op) + 1
    cells = np.zeros((n_steps, 8), dtype=np.int64)
    per_op = {int(o): rng.integers(1, P, size=8) for o in ops}      # one instruction per pc: every word live, used or not
    for o in ops:
        cells[op == o] = per_op[int(o)]
    cells[:, 0] = op
    na = int(ACC[op].sum())
    pool = np.concatenate([LAYOUT_IMAGE + rng.integers(0, 2, size=na), rng.integers(1 << 26, 1 << 27, size=na),
                           MAX_ADDRESS - rng.integers(0, LAYOUT_HEAP + 4, size=na), rng.integers(100, LAYOUT_IMAGE, size=na)]).reshape(4, na)
    addr = pool[rng.integers(0, 4, size=na), np.arange(na)]
    acc = np.concatenate([addr[:, None], _values(rng, na)], axis=1)
    image = _values(rng, LAYOUT_IMAGE)
    return build_arrays(pc, rng.integers(0, P, size=n_steps), cells, acc, image, _values(rng, LAYOUT_HEAP),
                        (0, 80, 100, 120, LAYOUT_IMAGE - 4, LAYOUT_IMAGE + 6))


def _store_steps(rng, addresses, pc=0, image_cells=4):
    """one opcode-9 step (a fetch at `pc` and one operand access) per address"""
    steps = [(pc, 3, [9, 5, 6], [(int(a), _values(rng, 1)[0])]) for a in addresses]
    return steps, _values(rng, image_cells)


def layout_fixed():
    """name -> Segment: the fixed layout cases"""
    rng = np.random.default_rng(77)
    out = {}
    # one cell accessed exactly 64, 65, 256 and 257 times (runs that end on, and one past, a wave and a block of the sorted log)
    addrs = np.concatenate([np.full(c, 1000 + c) for c in (64, 65, 256, 257)])
    out["run_lengths"] = build(*_store_steps(rng, rng.permutation(addrs)))
    # pads that place a run's head at sorted position == 0 and == 63 (mod 64), 0 and 255 (mod 256): the fetch cell's run comes
    # first (one entry per step), then n_pad cells touched once, then a cell touched 70 times; a lone jump makes the total odd
    for name, n_pad, jump in (("head_at_0_mod_64", 29, False), ("head_at_63_mod_64", 28, True), ("head_at_0_mod_256", 93, False),
                              ("head_at_255_mod_256", 92, True)):
        steps, image = _store_steps(rng, rng.permutation(np.concatenate([500 + np.arange(n_pad), np.full(70, 9999)])))
        if jump:                                        # (its own fetch cell, address 1, sorts between the two)
            steps.insert(int(rng.integers(0, len(steps))), (1, 3, [12, 0], []))
        out[name] = build(steps, image)
    out["n_mem_256"] = build(*_store_steps(rng, 300 + rng.integers(0, 40, size=128)))
    out["n_mem_768"] = build(*_store_steps(rng, 300 + rng.integers(0, 40, size=384)))
    # a self-jump at pc 0: every address is 0
    out["only_address_0"] = build([(0, 0, [12, 0], [])] * 5, np.zeros((1, 4), dtype=np.int64))
    out["only_address_0_long"] = build([(0, 0, [12, 0], [])] * 300, np.zeros((1, 4), dtype=np.int64))
    # addresses only in {0, 1}
    out["addresses_0_1"] = build([(t & 1, 1, [9, 5, 6], [(1 - (t & 1), _values(rng, 1)[0])]) for t in range(67)], _values(rng, 2))
    # a cell at MAX_ADDRESS: outside the image, and as heap cell 0
    steps, image = _store_steps(rng, [MAX_ADDRESS, 5, MAX_ADDRESS, MAX_ADDRESS - 1])
    out["max_address_outside"] = build(steps, image)
    out["max_address_heap"] = build(steps, image, heap=_values(rng, 1))
    # only the lowest component, only the highest, both with nothing between
    lowest = lambda t: (0, 9, [50, 1, 2], [(40 + t % 3, _values(rng, 1)[0])])
    highest = lambda t: (1, 9, [48, 1, 2, 3], [(50 + t % 3, _values(rng, 1)[0]), (60, _values(rng, 1)[0])])
    out["only_lowest_component"] = build([lowest(t) for t in range(9)], _values(rng, 4))
    out["only_highest_component"] = build([highest(t) for t in range(9)], _values(rng, 4))
    out["lowest_and_highest_component"] = build([(lowest if (t * 7) % 3 else highest)(t) for t in range(300)], _values(rng, 4))
    # all variants of one component interleaved (store_fp_fp: opcodes 0..3; u32 bitwise fp_fp: 36..38)
    for name, variants, na in (("variants_of_component_6", (0, 1, 2, 3), 3), ("variants_of_component_23", (36, 37, 38), 6)):
        ops = rng.choice(variants, size=300)
        steps = [(int(o) % 4, t, [int(o), 1, 2, 3], [(30 + int(rng.integers(0, 5)), _values(rng, 1)[0]) for _ in range(na)]) for t, o in enumerate(ops)]
        out[name] = build(steps, _values(rng, 8))
    return out


TREE_MEMORIES = {"0": [], "max": [MAX_ADDRESS], "0_max": [0, MAX_ADDRESS], "even_odd": [2 * 37, 2 * 37 + 1], "odd_even": [2 * 37 + 1, 2 * 37 + 2],
                 "around_2": [1, 2, 3], "around_32": [31, 32, 33], "around_2^13": [(1 << 13) - 1, 1 << 13, (1 << 13) + 1],
                 "around_2^27": [(1 << 27) - 1, 1 << 27, (1 << 27) + 1]}


def tree_segment(name):
    """boundary memory = the program cell 0 (a fetch needs a cell of the image) and the cells of TREE_MEMORIES[name]; the program
    range holds cell 0 and the output range the first touched cell, so leaf multiplicity 2 occurs in both trees"""
    rng = np.random.default_rng(5)
    cells = TREE_MEMORIES[name]
    if not cells:
        return build([(0, 0, [12, 0], [])] * 3, _values(rng, 1), ranges=(0, 1, 0, 0, 0, 1))
    steps, image = _store_steps(rng, cells + cells[::-1], image_cells=1)
    return build(steps, image, ranges=(0, 1, 0, 0, cells[0], cells[0] + 1))


RUN_LO, RUN_HI = 48, 6                                    # cells of the locals / the heap when the run starts


def run_case(n_segments, ranges="public"):
    """[(Segment, n_memory_end, n_heap_end)]: chained synthetic segments over a carried image.  Between the regions: reads of
    untouched cells (value zero, never carried), cells the locals then grow over, heap growth.  ranges: the input range spans
    locals, absent gap addresses and touched gap cells; the output range reaches from the gap into the heap; or all empty."""
    rng = np.random.default_rng(300 + n_segments)
    top = MAX_ADDRESS + 1
    rg = (0, 8, RUN_LO - 2, RUN_LO + 6, top - RUN_HI - 3, top - RUN_HI + 2) if ranges == "public" else (5, 5, 9, 9, 9, 3)
    lo, hi = _values(rng, RUN_LO), _values(rng, RUN_HI)
    ends = [(RUN_LO + 10, RUN_HI + 4), (RUN_LO + 10, RUN_HI + 4), (RUN_LO + 300, RUN_HI + 40)][:n_segments]
    out = []
    zero = np.zeros(4, dtype=np.int64)
    for s, (n_lo_end, n_hi_end) in enumerate(ends):
        n_lo, n_hi = lo.shape[0], hi.shape[0]
        steps = []
        val = lambda: _values(rng, 1)[0]
        for t in range(90):
            kind = t % 6
            if kind == 0:      # a local and a heap cell of the image
                steps.append((t % 5, t, [4, 1, 2, 3], [(20 + int(rng.integers(0, n_lo - 20)), val()), (MAX_ADDRESS - int(rng.integers(0, n_hi)), val())]))
            elif kind == 1:    # reads of untouched cells that stay outside both regions: zero
                steps.append((5, t, [4, 1, 2, 3], [(n_lo_end + 1 + 2 * int(rng.integers(0, 4)), zero), (top - n_hi_end - 2, zero)]))
            elif kind == 2:    # cells the locals / the heap grow over in this segment: any value
                a = n_lo + int(rng.integers(0, n_lo_end - n_lo)) if n_lo_end > n_lo else 9
                b = top - n_hi - 1 - int(rng.integers(0, n_hi_end - n_hi)) if n_hi_end > n_hi else MAX_ADDRESS
                steps.append((6, t, [4, 1, 2, 3], [(a, val()), (b, val())]))
            elif kind == 3:    # a six-word instruction, operands in the image
                steps.append((10, t, [22, 1, 2, 3, 4, 5], [(24 + k, val()) for k in range(6)]))
            elif kind == 4:    # touched gap cells inside the input range (RUN_LO + 1, RUN_LO + 3 while the locals end below them)
                a = RUN_LO + 1 + 2 * (t % 2)
                steps.append((7, t, [9, 5, 6], [(a, val() if a < n_lo_end else zero)]))
            else:
                steps.append((8, t, [12, 0], []))
        seg = build(steps, lo, hi, rg)
        out.append((seg, n_lo_end, n_hi_end))
        lo, hi = (x.astype(np.int64) for x in image_after(seg, n_lo_end, n_hi_end))
    return out


def refusals():
    """name -> (Segment, needle of the device adapter's message); each is a valid segment with one thing broken"""
    rng = np.random.default_rng(9)
    base = build([(0, 1, [9, 5, 6], [(20 + t % 7, _values(rng, 1)[0])]) for t in range(299)] + [(1, 1, [9, 5, 6], [(33, _values(rng, 1)[0])])],
                 _values(rng, 6))
    out = {}
    bad = base.copy()
    bad.image[1, 0] = bad.log[-2, 1] = 5                 # the last step (in the second block of steps) fetches a word that is no opcode
    out["invalid_opcode_in_last_block"] = (bad, "invalid opcode")
    out["log_one_short"] = (base.copy(log=base.log[:-1].copy()), "length does not match")
    out["log_one_long"] = (base.copy(log=np.concatenate([base.log, base.log[-1:]])), "length does not match")
    bad = base.copy()
    bad.log[2 * 150, 0] = 3                              # step 150's first entry names another address than its pc
    out["first_entry_not_pc"] = (bad, "not the instruction fetch at pc")
    bad = base.copy()
    bad.trace[200, 0] = bad.log[2 * 200, 0] = base.image.shape[0] + 5
    out["pc_beyond_image"] = (bad, "invalid opcode")
    return out


def rewritten_code(new_words):
    """step 0 runs pc 2 (opcode 9), step 1 stores another instruction over cell 2, step 2 fetches cell 2 again and logs the new
    words.  new_words (5, ...): another size and access count; (50, ...): same shape, another component."""
    rng = np.random.default_rng(11)
    new = list(new_words) + [0] * (4 - len(new_words))
    acc = [(30 + k, _values(rng, 1)[0]) for k in range(OPCODES[new[0]][1])]
    steps = [(2, 1, [9, 5, 6], [(20, _values(rng, 1)[0])]), (3, 1, [9, 7, 8], [(2, new)]), (2, 1, new, acc), (3, 1, [9, 7, 8], [(21, _values(rng, 1)[0])])]
    return build(steps, _values(rng, 8))
