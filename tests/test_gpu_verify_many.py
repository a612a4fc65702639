"""cm_verify_many / cm_verify_run_device: the query phase of the verifier on the GPU, for a whole batch of proofs.

The contract is parity with the host verifier (cm_verify_proof), which tests/test_verifier.py pins against the CPU oracle's: for
every proof the same status and the same words — that is, the EARLIEST failed check in the host's order, although the device
evaluates the checks side by side.  The proofs are HIP proofs of the suite's small workloads, made once per module."""
import ctypes as C

import numpy as np
import pytest

from cairo_m_amd.lib import (mem_stats, set_framing, synth_fibonacci, synth_fibonacci_segment, verify_many, verify_run, vm_run)
from tests.verify_many_util import hand_flips, proof_from_words, proof_layout

pytestmark = pytest.mark.gpu

CONFIGS = [None, (5, 2, 0, 20), (5, 1, 2, 20)]     # default; blowup above 1; non-zero last-layer bound (tests/test_verifier.py)


def _inputs():
    from tests.test_oracle_air import u32_program
    return {"fib7": synth_fibonacci(7), "fib3000": synth_fibonacci(3000), "u32": vm_run(u32_program(), entry_pc=0, args=(), n_returns=0)}


@pytest.fixture(scope="module")
def proofs(backend):
    """{(workload, config): Proof} — HIP proofs, shared and left unchanged by every test below"""
    inputs = _inputs()
    out = {(name, cfg): backend.prove(inp, cfg) for name, inp in inputs.items() for cfg in CONFIGS}
    for inp in inputs.values():
        inp.free()
    yield out
    for p in out.values():
        p.free()


def _host(p, cfg=None):
    return p.verify(cfg)


def _flip(words, pos):
    bad = words.copy()
    bad[pos] ^= 1
    return bad


def test_accepts_what_the_host_accepts(backend, proofs):
    for cfg in CONFIGS:
        batch = [proofs[(name, cfg)] for name in ("fib7", "fib3000", "u32")]
        got = backend.verify_many(batch, cfg)
        print(cfg, got)
        assert got == [(0, "")] * 3
        assert [_host(p, cfg) for p in batch] == [(0, "")] * 3


def _moved_queried_value(words):
    """tree 2 is handed one queried value more and tree 3 one less (the stream keeps its length and parses)"""
    lay = proof_layout(words)
    (o2, n2), (o3, n3) = lay["queried"][2], lay["queried"][3]
    w = list(words)
    return np.array(w[:o2 - 1] + [n2 + 1] + w[o2:o2 + n2] + [5, n3 - 1] + w[o3:o3 + n3 - 1] + w[o3 + n3:], dtype=np.uint32)


def _longer_first_layer_witness(words):
    """two more FRI first-layer witness values, one hash witness less"""
    lay = proof_layout(words)
    (ow, nw), (oh, nh) = lay["fri_first"]["fri_witness"], lay["fri_first"]["hash_witness"]
    w = list(words)
    return np.array(w[:ow - 1] + [nw + 2] + w[ow:ow + 4 * nw] + [0] * 8 + [nh - 1] + w[oh + 8:], dtype=np.uint32)


def test_tamper_parity_in_one_batch(backend, proofs):
    """64 seeded one-bit flips (default_rng(1), words [8, size - 1): with the host verifier 64 of them are rejected and all 64 parse —
    tests/test_verify_many_cpu.py checks those counts without a GPU), a hand-placed flip in every part of the proof, and three
    tamperings the host decides while PLANNING (a structural failure in tree 2, alone and behind a root mismatch in tree 0, and a
    first-layer witness of the wrong length) — all in ONE call, interleaved with untouched originals."""
    L = backend.L
    good = proofs[("fib7", None)]
    words = good.words()
    cases = [("random %d" % pos, _flip(words, pos)) for pos in np.random.default_rng(1).integers(8, words.size - 1, size=64)]
    hand = hand_flips(words)
    assert {"commitment root", "sampled value", "hash witness of tree 1", "column witness of tree 1", "FRI first-layer witness",
            "FRI inner-layer witness", "FRI inner-layer hash witness", "last-layer polynomial", "proof-of-work nonce"} <= set(hand)
    assert all(f"queried value of tree {t}" in hand for t in range(4))
    cases += [("hand: " + name, _flip(words, pos)) for name, pos in hand.items()]
    moved = _moved_queried_value(words)
    cases += [("planned: queried value moved from tree 3 to tree 2", moved),
              ("planned: the same behind a flipped queried value of tree 0", _flip(moved, hand["queried value of tree 0"])),
              ("planned: first-layer witness too long", _longer_first_layer_witness(words))]
    batch, names, unparsed = [], [], []
    for name, w in cases:
        p = proof_from_words(L, w)
        if p is None:
            unparsed.append(name)          # rejected by both paths before either verifier runs: counted apart
            continue
        batch += [p, good]
        names += [name, None]
    got = verify_many(batch, checks=True)
    assert len(got) == len(batch)
    rejected = {}
    for name, p, (status, message, check) in zip(names, batch, got):
        if name is None:
            assert (status, message, check) == (0, "", 0)
            continue
        want = _host(p)
        print(name, "->", status, check, message)
        assert (status, message) == want, (name, want)
        assert (check == 0) == (status == 0)
        rejected[name] = status == 11
    n_random = sum(v for k, v in rejected.items() if k.startswith("random")) + sum(k.startswith("random") for k in unparsed)
    assert n_random >= 62 and sum(k.startswith("random") for k in unparsed) <= 2, (n_random, unparsed)
    assert all(v for k, v in rejected.items() if not k.startswith("random")), rejected
    # what the planned cases have to say, in the host's words
    by_name = dict(zip(names, got))
    assert by_name["planned: queried value moved from tree 3 to tree 2"][1] == "verification failed: Merkle(tree 2): TooManyQueriedValues"
    assert by_name["planned: the same behind a flipped queried value of tree 0"][1] == "verification failed: Merkle(tree 0): RootMismatch"
    assert by_name["planned: first-layer witness too long"][1] == "verification failed: Fri(FirstLayerEvaluationsInvalid)"
    # the call's own status and words: the lowest rejected proof
    hs = (C.c_void_p * len(batch))(*[p.h.value for p in batch])
    assert L.cm_verify_many(hs, C.c_uint32(len(batch)), None, None, C.c_uint64(0)) == 11
    buf = C.create_string_buffer(512)
    L.cm_last_error(buf, C.c_size_t(512))
    first = next(i for i, g in enumerate(got) if g[0])
    assert buf.value.decode() == "proof %d: %s" % (first, got[first][1])
    for name, p in zip(names, batch):
        if name is not None:
            p.free()


@pytest.mark.parametrize("n", [1, 2, 33])
def test_batch_shape(backend, proofs, n):
    """results follow their proofs: mixed workloads, one rejected proof among them, two different orders"""
    L = backend.L
    pool = [proofs[(name, None)] for name in ("fib7", "fib3000", "u32")]
    bad = proof_from_words(L, _flip(pool[1].words(), hand_flips(pool[1].words())["queried value of tree 2"]))
    want_bad = _host(bad)
    assert want_bad[0] == 11
    for order in (lambda i: i, lambda i: n - 1 - i):
        batch = [pool[order(i) % 3] for i in range(n)]
        where = order(n // 2)
        batch[where] = bad
        got = backend.verify_many(batch)
        assert got == [want_bad if i == where else (0, "") for i in range(n)]
    bad.free()


def test_wrong_config(backend, proofs):
    p = proofs[("fib7", (5, 2, 0, 20))]
    got = backend.verify_many([p, proofs[("fib7", None)]])
    assert got[0] == _host(p) and got[0][1].startswith("verification failed: InvalidStructure(config): ") and got[1] == (0, "")
    assert verify_many([p], checks=True)[0][2] == 1


@pytest.mark.parametrize("spec", ["hash_node=rfc", "sample_batch=sorted"])
def test_framings(backend, spec):
    L = backend.L
    try:
        set_framing(spec, L)
        inp = synth_fibonacci(7)
        p = backend.prove(inp)
        inp.free()
        words = p.words()
        hand = hand_flips(words)
        bad = [proof_from_words(L, _flip(words, hand[k])) for k in ("queried value of tree 1", "sampled value")]
        got = backend.verify_many([p] + bad)
        print(spec, got)
        assert got[0] == (0, "") == _host(p)
        for g, b in zip(got[1:], bad):
            assert g == _host(b) and g[0] == 11
        for q in [p] + bad:
            q.free()
    finally:
        set_framing("", L)


def test_run_on_the_device(backend):
    """a 3-segment run: cm_verify_run_device accepts it, names a broken link and a proof that does not verify in cm_verify_run's words"""
    L = backend.L
    segs = [synth_fibonacci_segment(300, max_steps=1100, segment=s) for s in range(3)]
    got = backend.prove_run(segs, inflight=2)
    assert len(got) == 3
    assert verify_run(got) == (0, "") == backend.verify_run(got, device=True)
    swapped = [got[0], got[2], got[1]]
    want = verify_run(swapped)
    assert want[0] == 11 and " initial_" in want[1] and want[1].startswith("run: segment ")
    assert backend.verify_run(swapped, device=True) == want
    words = got[1].words()
    bad = proof_from_words(L, _flip(words, hand_flips(words)["queried value of tree 1"]))
    tampered = [got[0], bad, got[2]]
    want = verify_run(tampered)
    assert want[0] == 11 and want[1].startswith("run: segment 1: verification failed: Merkle(tree 1)")
    assert backend.verify_run(tampered, device=True) == want
    bad.free()
    for p in got:
        p.free()
    for s in segs:
        s.free()


def test_the_call_keeps_nothing(backend, proofs):
    L = backend.L
    pool = [proofs[(name, None)] for name in ("fib7", "fib3000", "u32")]
    own = [proof_from_words(L, pool[i % 3].words()) for i in range(33)]
    before = mem_stats(L).live_bytes
    assert backend.verify_many(own) == [(0, "")] * 33
    assert mem_stats(L).live_bytes == before
    for p in own:
        assert L.cm_proof_free(p.h) == 0
        p.h = None
