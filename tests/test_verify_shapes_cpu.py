"""The wide query shapes of the device verifier, as far as they can be checked without a GPU (tests/test_gpu_verify_shapes.py
runs them): cm_verify_plan_stats — host code that reads the tables cm_verify_many's planner built — says in numbers that each config
reaches the edge it is there for (a second trip of a kernel's stride loop, the 64 KB LDS limit, the refusal above it); the host
verifier and the oracle's verifier, two implementations, agree on proofs of these sizes; and every tamper position the GPU tests
use parses and is rejected by the host verifier, so that none of them can drop out there as unparsed.

The proofs are the oracle's, of synth_fibonacci(7), made once per module.  With that input the 512-query config gives a widest
tree level of exactly 1024 nodes; another input that does not needs another Fibonacci argument, not a weaker assertion."""
import ctypes as C
import os
import re

import pytest

from cairo_m_amd.lib import VerifySlotC, VerifyStatsC, load_library, synth_fibonacci, verify_plan_stats
from tests.verify_many_util import proof_from_words, proof_layout
from tests.verify_shapes_util import (ABOVE_THE_LIMIT, ACCEPTED, AT_THE_LIMIT, FRI_TWO_TRIPS, ONE_QUERY, WIDE, column_logs, flipped,
                                      last_entry_of_the_widest_batch, loop_flips, query_logs, verdict_cases, widest_group)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = open(os.path.join(ROOT, "include", "cairom_hip.h")).read()
CONFIGS = ACCEPTED + [ABOVE_THE_LIMIT]
FRI_THREADS, MERKLE_THREADS, ANS_THREADS = 128, 256, 256      # cairo_m_amd/csrc/verify_device.hip


@pytest.fixture(scope="module")
def proofs(oracle):
    """{config: (words, Proof)} — oracle proofs of synth_fibonacci(7), left unchanged by every test below"""
    L = load_library()
    inp = synth_fibonacci(7)
    out = {}
    for cfg in CONFIGS:
        words, _ = oracle.prove(inp.view, cfg)
        out[cfg] = (words, proof_from_words(L, words))
    inp.free()
    yield out
    for _, p in out.values():
        p.free()


@pytest.fixture(scope="module")
def stats(proofs):
    return {cfg: verify_plan_stats([p], cfg)[0] for cfg, (_, p) in proofs.items()}


def test_symbols_structs_and_revision():
    L = load_library()
    for name in ("cm_verify_plan_stats", "cm_verify_many_detail"):
        getattr(L, name)
        assert re.search(r"int32_t\s+%s\(" % name, HDR), name
    assert int(re.search(r"#define CM_ABI_REVISION (\d+)", HDR).group(1)) == 10
    comment = HDR[:HDR.index("#define CM_ABI_REVISION")]
    assert "cm_verify_plan_stats" in comment and "cm_verify_many_detail" in comment
    hdr = re.sub(r"/\*.*?\*/", "", HDR, flags=re.S)
    for name, cls in (("cm_verify_stats", VerifyStatsC), ("cm_verify_slot", VerifySlotC)):
        body = re.search(r"typedef struct %s \{([^}]*)\} %s;" % (name, name), hdr, re.S).group(1)
        fields = [f for decl in body.split(";") if decl.strip() for f in re.sub(r"^\s*\w+\s+", "", decl.strip()).split(",")]
        assert [re.sub(r"\[\d+\]", "", f).strip() for f in fields] == [f[0] for f in cls._fields_], name
    assert C.sizeof(VerifyStatsC) == 56 and C.sizeof(VerifySlotC) == 128
    assert VerifyStatsC._fields_[0][0] == "struct_size"


def test_argument_errors():
    L = load_library()
    one = (VerifyStatsC * 1)()
    assert L.cm_verify_plan_stats(None, C.c_uint32(0), None, one) == 1
    first = (C.c_uint32 * 2)()
    assert L.cm_verify_many_detail(None, C.c_uint32(0), None, None, None, C.c_uint32(0), first, C.c_uint64(0)) == 1
    assert L.cm_verify_many_detail(None, C.c_uint32(0), None, None, None, C.c_uint32(0), None, C.c_uint64(0)) == 1


def test_struct_size_is_checked_and_kept(proofs):
    L = load_library()
    p = proofs[ONE_QUERY][1]
    hs = (C.c_void_p * 1)(p.h.value)
    one = (VerifyStatsC * 1)()
    assert L.cm_verify_plan_stats(hs, C.c_uint32(1), (C.c_uint32 * 4)(*ONE_QUERY), one) == 1      # struct_size 0
    one[0].struct_size = C.sizeof(VerifyStatsC)
    assert L.cm_verify_plan_stats(hs, C.c_uint32(1), (C.c_uint32 * 4)(*ONE_QUERY), one) == 0
    assert one[0].struct_size == C.sizeof(VerifyStatsC) and one[0].n_slots > 0


def test_both_references_accept_every_proof(oracle, proofs):
    for cfg, (words, p) in proofs.items():
        assert p.verify(cfg) == (0, ""), cfg
        assert oracle.verify(words, cfg)[0] == 0, cfg


def test_the_configs_reach_the_edges(stats):
    for cfg, s in stats.items():
        print(cfg, s)
        assert s["early_check"] == 0
    assert stats[FRI_TWO_TRIPS]["max_inner_pairs"] > FRI_THREADS
    assert stats[WIDE]["max_inner_pairs"] > 2 * FRI_THREADS and stats[WIDE]["max_first_pairs"] > 2 * FRI_THREADS
    assert stats[WIDE]["max_level_nodes"] > 2 * MERKLE_THREADS
    assert stats[AT_THE_LIMIT]["max_level_nodes"] == 1024 and stats[AT_THE_LIMIT]["merkle_lds_bytes"] == 65536
    assert stats[ABOVE_THE_LIMIT]["max_level_nodes"] > 1024
    assert stats[ABOVE_THE_LIMIT]["merkle_lds_bytes"] == 64 * stats[ABOVE_THE_LIMIT]["max_level_nodes"]
    assert any(s["max_batch_entries"] > ANS_THREADS for s in stats.values())
    # no more pairs, and no more nodes in a level, than the positions can give
    for cfg, s in stats.items():
        assert s["max_inner_pairs"] <= s["max_first_pairs"] <= cfg[3] and s["max_level_nodes"] <= 2 * cfg[3]


def test_the_widest_batch_is_the_smallest_size_group(proofs, stats):
    """the widest sample batch counted in plain Python from the claim: every column of the smallest size group at the OODS point.
    Its last entry — index above 256, so a second trip of k_verify_answers' loop — reads the interaction tree's last queried word."""
    L = load_library()
    for cfg, (words, _) in proofs.items():
        logs = column_logs(L, words)
        ext_log, cols = widest_group(logs, cfg)
        assert ext_log == query_logs(logs, cfg)[-1] and cols[-1][0] == 2
        assert stats[cfg]["max_batch_entries"] == len(cols) > ANS_THREADS
        index, pos = last_entry_of_the_widest_batch(logs, cfg, words)
        off, n = proof_layout(words)["queried"][2]
        assert index == len(cols) - 1 >= ANS_THREADS and pos == off + n - 1


def test_one_query_gives_what_one_position_gives(proofs, stats):
    L = load_library()
    words, _ = proofs[ONE_QUERY]
    s = stats[ONE_QUERY]
    logs = column_logs(L, words)
    n_groups = len(query_logs(logs, ONE_QUERY))
    n_inner = len(proof_layout(words)["fri_inner"])
    assert s["n_answer_jobs"] == n_groups                              # one row per size group
    assert s["max_first_pairs"] == 1 and s["max_inner_pairs"] == 1
    assert s["max_level_nodes"] == 2 and s["merkle_lds_bytes"] == 128    # both values of the one pair are leaves of a FRI tree
    assert s["n_tree_jobs"] == 4 + 1 + n_inner and s["n_slots"] == s["n_tree_jobs"] + 1
    assert s["max_batch_entries"] == len(widest_group(logs, ONE_QUERY)[1])
    # scratch, in words: per size group an answer (4), a pair (8) and its fold (4); two evaluation buffers of one value; a pair per
    # inner layer
    assert s["scratch_words"] == 16 * n_groups + 8 + 8 * n_inner
    assert s["blob_words"] > words.size // 2


def test_a_proof_decided_before_the_queries_reports_zeros(proofs):
    p = proofs[ONE_QUERY][1]
    s = verify_plan_stats([p], WIDE)[0]                                # the verifier expects another config
    assert p.verify(WIDE)[1].startswith("verification failed: InvalidStructure(config)")
    assert s.pop("early_check") == 1                                   # CM_VERIFY_STRUCTURE
    assert set(s.values()) == {0}


@pytest.mark.parametrize("cfg", CONFIGS, ids=lambda c: "q%d" % c[3])
def test_every_tamper_position_parses_and_is_rejected(proofs, cfg):
    """the flips of tests/test_gpu_verify_shapes.py (the HIP proofs there are these word streams: smoke() holds them bit-identical)"""
    L = load_library()
    words, _ = proofs[cfg]
    flips = list(loop_flips(words).items()) + [(name, pos) for name, pos, _ in verdict_cases(L, words, cfg) if pos is not None]
    logs = column_logs(L, words)
    flips.append(("last entry of the widest batch", last_entry_of_the_widest_batch(logs, cfg, words)[1]))
    assert len(flips) > 50
    for name, pos in flips:
        q = proof_from_words(L, flipped(words, pos))
        assert q is not None, name
        got = q.verify(cfg)
        q.free()
        assert got[0] == 11, (name, got)
