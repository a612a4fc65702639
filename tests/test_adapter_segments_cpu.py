"""Hand-built segments (tests/adapter_segments.py) on the CPU: the builder's opcode table against the library, the host adapter over
a caller-supplied segment (cm_adapt_segment_host) against cm_vm_run and against the numpy reference, and the coverage assertions:
what every segment is there to reach is read off the REFERENCE's output, so a segment that lost its feature fails here instead of
passing vacuously on the GPU.  No GPU, no proofs (synthetic values do not satisfy the AIR)."""
import ctypes as C

import numpy as np
import pytest

from cairo_m_amd.lib import CmError, adapt_segment_host, load_library, prover_input_arrays, synth_fibonacci, synth_fibonacci_segment, vm_run, vm_segment
from tests import adapter_segments as S
from tests.test_gpu_adapter import _same, scatter_store_program

LIMIT = S.LIMIT


def host_arrays(seg):
    a = seg.array_segment()
    h = adapt_segment_host(a)
    out = prover_input_arrays(h.view)
    h.free()
    return out


def _host_equals_reference(seg):
    ref = S.reference(seg)
    _same(ref, host_arrays(seg))
    return ref


# ---- the opcode table ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("op", range(64))
def test_opcode_table_against_the_library(op):
    """one-step segments: with the table's entry count the library accepts the step, files it under the table's component with
    the table's span and keeps exactly `size` instruction words; one operand entry more or fewer, and every word that is no
    opcode, is refused"""
    rng = np.random.default_rng(op)
    words = rng.integers(1, S.P, size=8)
    words[0] = op
    if op not in S.OPCODES:
        seg = S.build([(0, 0, [12, 0], [])], np.zeros((2, 4)))
        seg.image[0, 0] = seg.log[0, 1] = op
        with pytest.raises(CmError, match="invalid opcode"):
            host_arrays(seg)
        return
    size, acc = S.OPCODES[op]
    seg = S.build([(0, 5, words.tolist(), [(10 + k, S._values(rng, 1)[0]) for k in range(acc)])], np.zeros((2, 4)))
    got = host_arrays(seg)
    _same(S.reference(seg), got)
    b = got[f"bundles{S.COMPONENT[op]}"]
    assert b.shape[0] == 1 and b[0, 10:].tolist() == [0, acc] and got["data_accesses"].shape[0] == acc
    inst = words[:4].tolist() + words[4:6].tolist()
    assert b[0, 4:10].tolist() == [w if k < size else 0 for k, w in enumerate(inst)]
    assert seg.log.shape[0] == 1 + (size > 4) + acc
    for log in (seg.log[:-1], np.concatenate([seg.log, seg.log[-1:]])):
        needle = "length does not match" if log.shape[0] else "empty memory trace"      # (a step without operands: nothing is left)
        with pytest.raises(CmError, match=needle):
            host_arrays(seg.copy(log=log.copy()))


# ---- cm_adapt_segment_host == cm_vm_run on the synthetic VM's own segments --------------------------------------------------------
def _vm_cases():
    from tests.casm_fixtures import heap_program
    from tests.test_oracle_air import CHAIN_PROG, felt_program, u32_loop_program, u32_program
    hp, hentry, hnret, _ = heap_program()
    cases = [("fib3", lambda: (synth_fibonacci(3), synth_fibonacci_segment(3))), ("fib1000", lambda: (synth_fibonacci(1000), synth_fibonacci_segment(1000))),
             ("fib_clock_updates", lambda: (synth_fibonacci(419_000), synth_fibonacci_segment(419_000)))]
    for name, prog, kw in (("felt", felt_program(), dict(n_returns=1)), ("u32", u32_program(), {}), ("u32_loop", u32_loop_program(50), {}),
                           ("scatter3000", scatter_store_program(3000), {}), ("wide", scatter_store_program(300, base=(1 << 27) + 12345), {}),
                           ("heap", hp, dict(entry_pc=hentry, n_returns=hnret))):
        cases.append((name, lambda prog=prog, kw=kw: (vm_run(prog, **kw), vm_segment(prog, **kw))))
    for s in range(4):
        cases.append((f"chain{s}", lambda s=s: (vm_run(CHAIN_PROG, max_steps=2, segment=s), vm_segment(CHAIN_PROG, max_steps=2, segment=s))))
        cases.append((f"heap_cut{s}", lambda s=s: (vm_run(hp, entry_pc=hentry, n_returns=hnret, max_steps=8, segment=s),
                                                  vm_segment(hp, entry_pc=hentry, n_returns=hnret, max_steps=8, segment=s))))
    return cases


@pytest.mark.parametrize("name,make", _vm_cases(), ids=[c[0] for c in _vm_cases()])
def test_host_entry_point_equals_vm_run(name, make):
    hi, hs = make()
    h2 = adapt_segment_host(hs)
    _same(prover_input_arrays(hi.view), prover_input_arrays(h2.view))
    hi.free(); hs.free(); h2.free()


# ---- the ladder ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ladder_ref():
    return S.reference(S.gap_ladder())


def test_ladder_host_adapter_equals_reference(ladder_ref):
    _same(ladder_ref, host_arrays(S.gap_ladder()))


def test_ladder_coverage(ladder_ref):
    """every (class, delta) pair yields the expected number of clock-update rows: 0, 1 or 2"""
    seg = S.gap_ladder()
    assert seg.n_steps == 2 * LIMIT + 300
    counts = S.ladder_update_counts(ladder_ref)
    cover = seg.info["cells_by_class"]
    assert sorted({k[0] for k in cover}) == ["a", "b", "c", "c2", "d", "e", "f", "g", "h"]
    for cls in "abcdef":
        assert sorted(d for c, d in cover if c == cls) == sorted(S.LADDER_DELTAS), cls
    for (cls, delta), cells in cover.items():
        for addr, want in cells:
            assert counts.get(addr, 0) == want, (cls, delta - LIMIT, addr, counts.get(addr, 0), want)
    per_delta = {d: S.expected_updates(d) for d in S.LADDER_DELTAS}
    assert [per_delta[d] for d in S.LADDER_DELTAS] == [0, 0, 1, 1, 2, 2]
    cu = ladder_ref["clock_updates"]
    k, h = seg.image.shape[0], seg.heap.shape[0]
    # what the update carries: the image's value, the heap's value, else the first logged value (never a later one)
    log = seg.log
    for addr, prev_clock, *value in cu.tolist():
        if addr < k:
            want = seg.image[addr].tolist()
        elif S.MAX_ADDRESS - addr < h:
            want = seg.heap[S.MAX_ADDRESS - addr].tolist()
        else:
            want = log[np.nonzero(log[:, 0] == addr)[0][0], 1:].tolist()
        assert value == want, addr
    b3 = cover[("b", LIMIT + 1)][0][0]
    vals = log[log[:, 0] == b3][:, 1:]
    assert vals.shape[0] == 3 and len({tuple(v) for v in vals.tolist()}) == 3          # three accesses, three values
    assert (log[:, 0] == b3 - 1).sum() == 70 and (log[:, 0] == b3 + 1).sum() == 70      # neighbours on both sides
    # updates on: a local of the image, a gap cell, a heap cell, both cells of a six-word instruction, a cell first touched late
    f = cover[("f", 2 * LIMIT)][0][0]
    assert counts[f] == 2 and counts[f + 1] == 2
    assert counts[cover[("c", LIMIT + 1)][0][0]] == 1 and counts[cover[("d", 2 * LIMIT + 1)][0][0]] == 2
    # log order and address order of the update rows disagree
    assert not np.array_equal(cu[:, 0], np.sort(cu[:, 0], kind="stable"))
    # one step, one cell, two accesses: the second has delta 0
    da = ladder_ref["data_accesses"]
    g = da[da[:, 0] == 7001]
    assert g.shape[0] == 2 and g[0, 1] == LIMIT and g[1, 1] == LIMIT + 6
    # inst_prev_clock of class e: the second run of the instruction at clock c0 + delta sees c0 + k * LIMIT
    e_cell = cover[("e", LIMIT + 1)][0][0]
    rows = ladder_ref[f"bundles{S.COMPONENT[11]}"]
    rows = rows[rows[:, 0] == e_cell]
    assert rows.shape[0] == 2 and rows[1, 3] == rows[0, 2] + LIMIT and rows[1, 2] == rows[0, 2] + LIMIT + 1


@pytest.mark.parametrize("delta", S.LADDER_DELTAS)
def test_ladder_deltas_through_memory_push(delta):
    """Memory::push itself (cm_adapter_memory_script) at the six deltas, against the loop of memory.rs:511-525 written out"""
    L = load_library()
    c0 = 17
    scr = np.array([100, 1, 2, 3, 4, c0, 100, 5, 6, 7, 8, c0 + delta], dtype=np.uint32)
    res, cu, ncu = np.zeros(10, dtype=np.uint32), np.zeros(6 * 8, dtype=np.uint32), C.c_uint32(0)
    q, st = np.zeros(1, dtype=np.uint32), np.zeros(14, dtype=np.uint32)
    p = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint32))
    assert L.cm_adapter_memory_script(p(q), C.c_uint32(0), p(scr), C.c_uint32(2), p(res), C.byref(ncu), p(cu), C.c_uint32(8), p(q), C.c_uint32(0), p(st)) == 0
    want, prev_clk, current_clk = [], c0, c0 + delta
    if current_clk > prev_clk:
        d = current_clk - prev_clk
        if d > LIMIT:
            num_steps = d // LIMIT
            for _ in range(num_steps):
                want.append([100, prev_clk, 1, 2, 3, 4])
                prev_clk += LIMIT
    assert cu[:6 * ncu.value].reshape(-1, 6).tolist() == want and len(want) == S.expected_updates(delta)
    assert res[5] == prev_clk and res[6:].tolist() == [1, 2, 3, 4]


# ---- layout ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_steps", S.LAYOUT_SIZES)
def test_layout_mix(n_steps):
    seg = S.layout_mix(n_steps)
    ref = _host_equals_reference(seg)
    assert seg.n_steps == n_steps
    present = [c for c in range(S.N_COMPONENTS) if ref[f"bundles{c}"].shape[0]]
    if n_steps >= 255:
        assert present == list(range(S.N_COMPONENTS))
        ops = set(np.concatenate([ref[f"bundles{c}"][:, 4] for c in range(S.N_COMPONENTS)]).tolist())
        assert ops == set(S.OPCODES)
        a = ref["data_accesses"][:, 0]
        k, h = seg.image.shape[0], seg.heap.shape[0]
        assert (a < k).any() and ((a >= k) & (a < k + 8)).any() and (a >= 1 << 26).any() and (a > S.MAX_ADDRESS - h).any()
        assert ((a <= S.MAX_ADDRESS - h) & (a > S.MAX_ADDRESS - h - 4)).any()          # just below the heap
        _, runs = np.unique(seg.log[:, 0], return_counts=True)
        assert runs.max() >= 64 and (runs == 1).sum() > 10                            # long runs and singletons
    # unused instruction words are live in the log and masked in the bundle
    for c in range(S.N_COMPONENTS):
        for row in ref[f"bundles{c}"][:3]:
            size = S.OPCODES[int(row[4])][0]
            assert (row[5:4 + size] != 0).all() and (row[4 + size:10] == 0).all()


FIXED = S.layout_fixed()


@pytest.mark.parametrize("name", sorted(FIXED))
def test_layout_fixed_host_equals_reference(name):
    _host_equals_reference(FIXED[name])


def test_layout_fixed_coverage():
    """each fixed case shows what it is there for, in the log and in the reference's output"""
    sa, head = S.sorted_layout(FIXED["run_lengths"])
    _, runs = np.unique(sa, return_counts=True)
    assert {64, 65, 256, 257} <= set(runs.tolist())
    for name, pos, mod in (("head_at_0_mod_64", 0, 64), ("head_at_63_mod_64", 63, 64), ("head_at_0_mod_256", 0, 256), ("head_at_255_mod_256", 255, 256)):
        sa, head = S.sorted_layout(FIXED[name])
        at = int(np.nonzero(sa == 9999)[0][0])
        assert head[at] and at % mod == pos and at > 0 and (sa == 9999).sum() == 70, (name, at)
        assert (at + 69) // 64 > at // 64                                             # the run straddles a wave boundary
    for name, k in (("n_mem_256", 1), ("n_mem_768", 3)):
        assert FIXED[name].log.shape[0] == 256 * k
    for name in ("only_address_0", "only_address_0_long"):
        assert not FIXED[name].log[:, 0].any()
    assert FIXED["only_address_0_long"].n_steps > 256
    assert set(FIXED["addresses_0_1"].log[:, 0].tolist()) == {0, 1}
    for name in ("max_address_outside", "max_address_heap"):
        assert FIXED[name].log[:, 0].max() == S.MAX_ADDRESS
    assert FIXED["max_address_outside"].heap.shape[0] == 0 and FIXED["max_address_heap"].heap.shape[0] == 1
    comps = lambda name: [c for c in range(S.N_COMPONENTS) if S.reference(FIXED[name])[f"bundles{c}"].shape[0]]
    assert comps("only_lowest_component") == [0] and comps("only_highest_component") == [S.N_COMPONENTS - 1]
    assert comps("lowest_and_highest_component") == [0, S.N_COMPONENTS - 1]
    for name, c, variants in (("variants_of_component_6", 6, [0, 1, 2, 3]), ("variants_of_component_23", 23, [36, 37, 38])):
        rows = S.reference(FIXED[name])[f"bundles{c}"]
        assert rows.shape[0] == 300 and sorted(set(rows[:, 4].tolist())) == variants
        assert rows[:, 4].tolist() == sorted(rows[:, 4].tolist())                     # grouped by variant ...
        assert not np.array_equal(rows[:, 2], np.sort(rows[:, 2]))                    # ... so not in step order
        for v in variants:
            assert np.all(np.diff(rows[rows[:, 4] == v][:, 2].astype(np.int64)) > 0)     # step order inside a variant


# ---- trees, runs, refusals, rewritten code ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(S.TREE_MEMORIES))
def test_tree_segments(name):
    seg = S.tree_segment(name)
    ref = _host_equals_reference(seg)
    assert ref["initial_memory"][:, 0].tolist() == sorted(set([0] + S.TREE_MEMORIES[name]))
    for tree in ("initial_tree", "final_tree"):
        leaves = ref[tree][ref[tree][:, 1] == 30]
        assert (leaves[:, 5:7] == 2).any() and ((leaves[:, 5:7] == 1).any() or name == "0"), (name, tree)   # public and private leaves
    assert ref["initial_tree"][:, 1].min() == 1


@pytest.mark.parametrize("n_segments,ranges", [(2, "public"), (3, "public"), (3, "empty")])
def test_run_segments(n_segments, ranges):
    case = S.run_case(n_segments, ranges)
    assert len(case) == n_segments
    lo, hi = case[0][0].image, case[0][0].heap
    for k, (seg, n_lo_end, n_hi_end) in enumerate(case):
        assert np.array_equal(seg.image, lo) and np.array_equal(seg.heap, hi), k           # the builder did not touch the carried image
        ref = _host_equals_reference(seg)
        n_lo, n_hi = lo.shape[0], hi.shape[0]
        a = np.unique(seg.log[:, 0]).astype(np.int64)
        gap = a[(a >= n_lo) & (a <= S.MAX_ADDRESS - n_hi)]
        outside = gap[(gap >= n_lo_end) & (gap <= S.MAX_ADDRESS - n_hi_end)]
        assert outside.size >= 2 and (outside < 1 << 20).any() and (outside > 1 << 27).any()      # zero reads on both sides
        assert not seg.log[np.isin(seg.log[:, 0], outside)][:, 1:].any()
        if n_lo_end > n_lo:
            grown = gap[gap < n_lo_end]
            assert grown.size and seg.log[np.isin(seg.log[:, 0], grown)][:, 1:].any()             # the locals grow over touched cells
        if n_hi_end > n_hi:
            assert (gap > S.MAX_ADDRESS - n_hi_end).any()                                         # and so does the heap
        pub = S.public_entries(ref)
        if ranges == "public":
            inp, outp = pub["input"], pub["output"]
            if k == 0:
                assert inp[:2, 0].tolist() == [1, 1] and 0 in inp[2:, 0] and 1 in inp[2:, 0]      # locals, absent and touched gap cells
            assert outp[-2:, 0].tolist() == [1, 1] and outp[0, 1] in (0, S.MAX_ADDRESS - S.RUN_HI - 2)
            assert (outp[:, 6] > 0).any()                                                        # a final clock in the output
        else:
            assert not any(v.shape[0] for v in pub.values())
        lo, hi = S.image_after(seg, n_lo_end, n_hi_end)
    assert case[-1][1] > case[0][0].image.shape[0] and case[-1][2] > case[0][0].heap.shape[0]


@pytest.mark.parametrize("name", sorted(S.refusals()))
def test_refusals_on_the_host(name):
    """the reference refuses each; the host adapter follows the log, so a pc beyond the image is a first access like any other"""
    seg, needle = S.refusals()[name]
    if name == "pc_beyond_image":
        _host_equals_reference(seg)
        return
    with pytest.raises(S.Refused, match=needle):
        S.reference(seg)
    with pytest.raises(CmError, match=needle) as e:
        host_arrays(seg)
    assert "status 1:" in str(e.value)


@pytest.mark.parametrize("new_words", [(4, 1, 2, 3), (50, 1, 2)])
def test_rewritten_code_follows_the_log_on_the_host(new_words):
    seg = S.rewritten_code(new_words)
    ref = _host_equals_reference(seg)
    assert seg.image[2, 0] == 9 and seg.log[seg.log[:, 0] == 2][:, 1].tolist() == [9, new_words[0], new_words[0]]
    new = ref[f"bundles{S.COMPONENT[new_words[0]]}"]
    assert new.shape[0] == 1 and new[0, 0] == 2 and new[0, 2] == 3 and new[0, 11] == S.OPCODES[new_words[0]][1]
    assert ref[f"bundles{S.COMPONENT[9]}"].shape[0] == 3
