"""cm_verify_many_ex with CM_VERIFY_ARITH_ON_DEVICE on whole proofs: the public LogUp sum and the OODS composition check decided by
the GPU as the first two slots of every proof, the verdicts and words still cm_verify_proof's.

Proofs: oracle proofs of synth_fibonacci(7) under the accepted configs of tests/verify_shapes_util.py, and one HIP proof of a
padded program with 408 present public entries (cairo_m_amd/workloads.py: all_opcodes_program(1) with data cells behind it up to
400 cells, plus the entries the run adds) — more than one workgroup (256 entries) of k_verify_public_sum; the test states and
checks the count."""
import ctypes as C

import numpy as np
import pytest

from cairo_m_amd.workloads import all_opcodes_program, padded_program
from cairo_m_amd.lib import synth_fibonacci, verify_many, verify_many_detail, verify_many_timing, verify_run, vm_run
from tests.verify_many_util import proof_from_words, proof_layout
from tests.verify_shapes_util import ACCEPTED, FRI_TWO_TRIPS

pytestmark = pytest.mark.gpu

LOGUP_SUM, OODS = 3, 4           # CM_VERIFY_* (include/cairom_hip.h)
BIG = "big program"              # key of the HIP proof; its config is the default one
N_BIG_PRESENT = 408
BIG_CELLS = 400


@pytest.fixture(scope="module")
def proofs(backend, oracle):
    """{config or BIG: (words, Proof, config)} — left unchanged by every test below"""
    L = backend.L
    out = {}
    inp = synth_fibonacci(7)
    for cfg in ACCEPTED:
        words, _ = oracle.prove(inp.view, cfg)
        out[cfg] = (words, proof_from_words(L, words), cfg)
    inp.free()
    inp = vm_run(padded_program(all_opcodes_program(1)[0], BIG_CELLS), entry_pc=0, args=(), n_returns=0)
    p = backend.prove(inp)
    inp.free()
    out[BIG] = (p.words(), p, None)
    yield out
    for _, p, _ in out.values():
        p.free()


def _public_lists(words):
    """[(offset of the list's count word, rows)] of program, input, output"""
    w = [int(x) for x in words]
    i = 6 + 5 * w[5] + 7
    out = []
    for _ in range(3):
        out.append((i, np.array(w[i + 1:i + 1 + 7 * w[i]], dtype=np.uint32).reshape(-1, 7)))
        i += 1 + 7 * w[i]
    return out


def test_the_big_program_fills_more_than_one_workgroup(proofs):
    lists = _public_lists(proofs[BIG][0])
    present = sum(int(rows[:, 0].sum()) for _, rows in lists)
    print("present public entries:", [int(rows[:, 0].sum()) for _, rows in lists])
    assert present == N_BIG_PRESENT > 256 and max(rows.shape[0] for _, rows in lists) > 256


def test_accepted_with_the_flag(backend, proofs):
    L = backend.L
    for key, (words, p, cfg) in proofs.items():
        got = verify_many([p], cfg, L, checks=True, arith="device")
        print(key, got, verify_many_timing(L))
        assert got == [(0, "", 0)] == verify_many([p], cfg, L, checks=True), key
        assert p.verify(cfg) == (0, ""), key
        (verdict, slots), = verify_many_detail([p], cfg, L, arith="device")
        (_, plain_slots), = verify_many_detail([p], cfg, L)
        assert verdict == (0, "", 0)
        assert slots[0] == (LOGUP_SUM, "InvalidLogupSum", True, False) and slots[1] == (OODS, "OodsNotMatching", True, False), key
        assert slots[2:] == plain_slots and all(on and not up for _, _, on, up in slots), key      # the default mode's slots follow
    # a batch under one config, and the run entry
    same_cfg = [proofs[FRI_TWO_TRIPS][1]] * 3
    assert verify_many(same_cfg, FRI_TWO_TRIPS, L, arith="device") == [(0, "")] * 3
    assert verify_run([proofs[BIG][1]], None, L, device=True, arith="device") == (0, "")


def _flip(words, *positions):
    bad = words.copy()
    for pos in positions:
        bad[pos] ^= 1
    return bad


def _pow_flip(L, words, cfg):
    """a nonce bit whose flip the host rejects as ProofOfWork (a flipped nonce still passes with probability 2^-pow_bits)"""
    pos = proof_layout(words)["pow"]
    for bit in range(64):
        bad = words.copy()
        bad[pos + bit // 32] ^= np.uint32(1 << (bit % 32))
        p = proof_from_words(L, bad)
        verdict = p.verify(cfg)
        p.free()
        if verdict == (11, "verification failed: ProofOfWork"):
            return pos + bit // 32, np.uint32(1 << (bit % 32))
    raise AssertionError("no nonce bit is rejected")


def _host_says_oods(L, words, cfg):
    p = proof_from_words(L, words)
    verdict = p.verify(cfg)
    p.free()
    return verdict == (11, "verification failed: OodsNotMatching")


def _tampers(L, words, cfg):
    """[(name, words, expected CM_VERIFY_* id or None, slot expectations)]; a slot expectation is checked by _check_slots"""
    lay = proof_layout(words)
    nc = int(words[5])
    claimed = 6 + nc + 4 * (nc // 2) + 1                  # one word of a claimed sum
    cases = [("(a) claimed sum", _flip(words, claimed), 3, "logup raised")]
    for t in range(4):
        cols = lay["sampled"][t]
        last = cols[-1] + (4 if t == 2 else 0) + 3        # the last value of tree 2's last column is its second sample
        # (a trace column that no constraint reads exists — its flip passes the OODS check on the host as well; the middle
        # value is the one nearest the middle that the host verifier's OODS check reads)
        middle = next(c for c in sorted(cols, key=lambda c: abs(cols.index(c) - len(cols) // 2)) if _host_says_oods(L, _flip(words, c + 1), cfg))
        for where, pos in (("first", cols[0]), ("middle", middle + 1), ("last", last)):
            cases.append(("(b) %s sampled value of tree %d" % (where, t), _flip(words, pos), 4, "oods raised"))
    assert int(words[lay["sampled"][2][-1] - 1]) == 2        # a LogUp column with the [-1, 0] mask: previous row first
    cases.append(("(b) previous-row sample of a LogUp column", _flip(words, lay["sampled"][2][-1] + 2), 4, "oods raised"))
    pow_pos, pow_bit = _pow_flip(L, words, cfg)
    bad = words.copy()
    bad[pow_pos] ^= pow_bit
    cases.append(("(c) proof-of-work nonce", bad, 6, "planned third"))
    both = bad.copy()
    both[claimed] ^= 1
    cases.append(("(d) claimed sum and nonce", both, 3, None))
    cases.append(("(e) interaction_pow", _flip(words, lay["commitments"][0] - 3), 2, "early"))
    off, n = lay["last_poly"]
    short = np.concatenate([words[:off - 1], np.array([n - 1], dtype=np.uint32), words[off:off + 4 * (n - 1)], words[off + 4 * n:]])
    cases.append(("(g) last-layer polynomial one coefficient short", short, 5, "arithmetic unraised"))
    lists = _public_lists(words)
    for off, rows in lists:
        if rows.shape[0]:
            k = rows.shape[0] - 1                          # the last entry of the first non-empty list: its third value word
            cases.append(("(f) public entry value", _flip(words, off + 1 + 7 * k + 4), None, None))
            break
    return cases


def _check_slots(name, want, verdict, slots):
    if want == "early":
        assert slots == [], name
        return
    assert [s[:3] for s in slots[:2]] == [(LOGUP_SUM, "InvalidLogupSum", True), (OODS, "OodsNotMatching", True)], name
    if want == "logup raised":
        assert slots[0][3], name
    elif want == "oods raised":
        assert not slots[0][3] and slots[1][3], name
    elif want == "planned third":
        assert len(slots) == 3 and not slots[0][3] and not slots[1][3], name
        assert slots[2] == (6, "ProofOfWork", False, True), name
    elif want == "arithmetic unraised":
        assert not slots[0][3] and not slots[1][3], name
        assert len(slots) == 3 and slots[2][0] == 5 and not slots[2][2] and slots[2][3], name


def _drop_last_sampled_column(words, tree):
    """the proof with the last sampled column of one tree taken out (the stream still parses)"""
    cols = proof_layout(words)["sampled"][tree]
    last, count_pos = cols[-1], cols[0] - 2
    assert int(words[count_pos]) == len(cols)
    bad = np.concatenate([words[:last - 1], words[last + 4 * int(words[last - 1]):]])
    bad[count_pos] -= 1
    return bad


@pytest.mark.parametrize("key", [FRI_TWO_TRIPS, BIG], ids=["oracle fib7", "big program"])
@pytest.mark.parametrize("tree", [0, 1, 2, 3])
def test_a_shape_failure_sits_between_the_two_deferred_checks(backend, proofs, key, tree):
    """the sampled values lose a column: the host decides InvalidStructure(sampled columns) BEHIND the LogUp sum and in front of
    the OODS check, so the LogUp slot goes out, the OODS slot does not, and the failure is the planned slot behind it; with a
    claimed sum flipped as well the LogUp slot is raised and wins"""
    L = backend.L
    words, good, cfg = proofs[key]
    dropped = _drop_last_sampled_column(words, tree)
    both = dropped.copy()
    both[6 + int(words[5]) + 4 * (int(words[5]) // 2) + 1] ^= 1
    batch = [proof_from_words(L, dropped), proof_from_words(L, both), good]
    assert all(p is not None for p in batch)
    got = verify_many(batch, cfg, L, checks=True, arith="device")
    detail = verify_many_detail(batch, cfg, L, arith="device")
    assert got == verify_many(batch, cfg, L, checks=True) == [v for v, _ in detail]
    assert [g[:2] for g in got] == [p.verify(cfg) for p in batch]
    assert got == [(11, "verification failed: InvalidStructure(sampled columns)", 1), (11, "verification failed: InvalidLogupSum", 3), (0, "", 0)]
    shape = (1, "InvalidStructure(sampled columns)", False, True)
    assert detail[0][1] == [(LOGUP_SUM, "InvalidLogupSum", True, False), shape]
    assert detail[1][1] == [(LOGUP_SUM, "InvalidLogupSum", True, True), shape]
    for p in batch[:2]:
        p.free()


@pytest.mark.parametrize("key", [FRI_TWO_TRIPS, BIG], ids=["oracle fib7", "big program"])
def test_tampers_and_a_mixed_batch(backend, proofs, key):
    """every tamper of the table, alone in its slots and together in ONE batch behind an accepted proof: each proof gets the host
    verifier's verdict, and the call's status and cm_last_error() name the lowest rejected index"""
    L = backend.L
    words, good, cfg = proofs[key]
    cases = _tampers(L, words, cfg)
    assert {c[0][:3] for c in cases} == {"(a)", "(b)", "(c)", "(d)", "(e)", "(f)", "(g)"}
    batch = [good]
    for name, w, _, _ in cases:
        p = proof_from_words(L, w)
        assert p is not None, name
        batch.append(p)
    got = verify_many(batch, cfg, L, checks=True, arith="device")
    plain = verify_many(batch, cfg, L, checks=True)
    detail = verify_many_detail(batch, cfg, L, arith="device")
    assert got[0] == (0, "", 0)
    for (name, _, want_id, want_slots), p, g, pl, (verdict, slots) in zip(cases, batch[1:], got[1:], plain[1:], detail[1:]):
        host = p.verify(cfg)
        print(name, "->", g, [(c, on, up) for c, _, on, up in slots[:3]])
        assert g[:2] == host and g == pl == verdict, (name, g, pl, host)
        assert host[0] == 11, name
        if want_id is not None:
            assert g[2] == want_id, (name, g)
        if want_slots is not None:
            _check_slots(name, want_slots, verdict, slots)
    # the call's own status and words: the lowest rejected proof
    hs = (C.c_void_p * len(batch))(*[p.h.value for p in batch])
    cfg_c = (C.c_uint32 * 4)(*cfg) if cfg else None
    assert L.cm_verify_many_ex(hs, C.c_uint32(len(batch)), cfg_c, C.c_uint32(1), None, C.c_uint64(0)) == 11
    buf = C.create_string_buffer(512)
    L.cm_last_error(buf, C.c_size_t(512))
    assert buf.value.decode() == "proof 1: %s" % got[1][1]
    # the same proofs the other way round: the verdicts follow their proofs
    assert verify_many(batch[::-1], cfg, L, checks=True, arith="device") == got[::-1]
    for p in batch[1:]:
        p.free()
