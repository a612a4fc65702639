"""cm_verify_many at the query shapes where its kernels take a second trip of their stride loops, at the 64 KB LDS limit and
above it — and every device check seen to say no ON ITS OWN (cm_verify_many_detail), not only as the first failure of a proof.

tests/test_gpu_verify_many.py runs at most 80 queries (one trip of every loop) and tampers with one-word flips, which always trip
an early check: a kernel that compared the last layer wrongly, or folded a size group into the wrong inner layer, would pass it.
Here the reference is the host verifier (cm_verify_proof; tests/test_verify_shapes_cpu.py holds it to the oracle's at these sizes)
for verdicts, and for the per-check flags a prediction from the dataflow written in plain Python (tests/verify_shapes_util.py).
That the configs reach the edges they are named for is asserted in numbers by tests/test_verify_shapes_cpu.py, without a GPU.
The last polynomial's stride loop in k_verify_fri is the one loop left at one trip: a last-layer bound above 2 cannot be proved
for this AIR, so a valid proof has at most 4 coefficients.  HIP proofs of the suite's small inputs, made once per module."""
import pytest

from cairo_m_amd.lib import (CmError, mem_stats, set_framing, synth_fibonacci, synth_fibonacci_segment, verify_many, verify_many_detail,
                             verify_many_timing, verify_plan_stats, verify_run, vm_run)
from tests.verify_many_util import proof_from_words, proof_layout
from tests.verify_shapes_util import (ABOVE_THE_LIMIT, ACCEPTED, AT_THE_LIMIT, REFUSAL, WIDE, column_logs, flipped,
                                      last_entry_of_the_widest_batch, loop_flips, slot_key, slot_keys, verdict_cases)

pytestmark = pytest.mark.gpu

NAMES = ("fib7", "fib3000", "u32")


def _inputs():
    from tests.test_oracle_air import u32_program
    return {"fib7": synth_fibonacci(7), "fib3000": synth_fibonacci(3000), "u32": vm_run(u32_program(), entry_pc=0, args=(), n_returns=0)}


@pytest.fixture(scope="module")
def proofs(backend):
    """{(workload, config): Proof} — HIP proofs, shared and left unchanged by every test below"""
    inputs = _inputs()
    out = {(name, cfg): backend.prove(inputs[name], cfg) for name in NAMES for cfg in ACCEPTED}
    out[("fib7", ABOVE_THE_LIMIT)] = backend.prove(inputs["fib7"], ABOVE_THE_LIMIT)
    for inp in inputs.values():
        inp.free()
    yield out
    for p in out.values():
        p.free()


@pytest.mark.parametrize("cfg", ACCEPTED, ids=lambda c: "q%d" % c[3])
def test_accepts_at_every_shape(backend, proofs, cfg):
    batch = [proofs[(name, cfg)] for name in NAMES]
    got = backend.verify_many(batch, cfg)
    print(cfg, got)
    assert got == [(0, "")] * 3
    assert [p.verify(cfg) for p in batch] == [(0, "")] * 3


def test_run_on_the_device_at_300_queries(backend):
    segs = [synth_fibonacci_segment(300, max_steps=1100, segment=s) for s in range(3)]
    got = backend.prove_run(segs, inflight=2, cfg=WIDE)
    assert len(got) == 3
    assert verify_run(got, WIDE) == (0, "") == backend.verify_run(got, WIDE, device=True)
    for p in got:
        p.free()
    for s in segs:
        s.free()


@pytest.mark.parametrize("cfg", [WIDE, AT_THE_LIMIT], ids=lambda c: "q%d" % c[3])
def test_flips_in_every_trip_of_every_loop(backend, proofs, cfg):
    """the first, the middle and the last word of every array a stride loop walks, and the queried value the last entry of the
    widest sample batch reads — one batch, interleaved with the untouched proof; status and words are the host verifier's"""
    L = backend.L
    good = proofs[("fib7", cfg)]
    words = good.words()
    flips = loop_flips(words)
    index, pos = last_entry_of_the_widest_batch(column_logs(L, words), cfg, words)
    assert index >= 256
    flips["last entry (%d) of the widest sample batch" % index] = pos
    batch, names = [], []
    for name, pos in flips.items():
        p = proof_from_words(L, flipped(words, pos))
        assert p is not None, name
        batch += [p, good]
        names += [name, None]
    got = verify_many(batch, cfg, checks=True)
    assert len(got) == len(batch)
    for name, p, g in zip(names, batch, got):
        if name is None:
            assert g == (0, "", 0)
            continue
        want = p.verify(cfg)
        print(name, "->", g)
        assert g[:2] == want and g[0] == 11 and g[2] != 0, (name, g, want)
    for name, p in zip(names, batch):
        if name is not None:
            p.free()


def _check_every_verdict(L, good, cfg):
    """every case of verdict_cases in one batch: the raised device slots are the predicted ones, the verdict is the lowest of them
    in the host's words, and it is cm_verify_many's and the host verifier's.  Returns {slot: {raised?}} over the cases."""
    words = good.words()
    n_inner = len(proof_layout(words)["fri_inner"])
    cases = verdict_cases(L, words, cfg)
    batch = []
    for name, pos, _ in cases:
        p = good if pos is None else proof_from_words(L, flipped(words, pos))
        assert p is not None, name
        batch.append(p)
    detail = verify_many_detail(batch, cfg, L)
    plain = verify_many(batch, cfg, L, checks=True)
    seen = {key: set() for key in slot_keys(n_inner)}
    for (name, pos, want), p, (verdict, slots), plain_verdict in zip(cases, batch, detail, plain):
        keys = [slot_key(check, message) for check, message, _, _ in slots]
        assert keys == slot_keys(n_inner), name
        assert all(on_device for _, _, on_device, _ in slots), name
        raised = {key for key, (_, _, _, up) in zip(keys, slots) if up}
        print(name, "->", verdict, sorted(raised))
        assert raised == want, (name, sorted(raised), sorted(want))
        assert verdict == plain_verdict and verdict[:2] == p.verify(cfg), name
        if want:
            check, message = next((c, m) for c, m, _, up in slots if up)
            assert verdict == (11, "verification failed: " + message, check), name
        else:
            assert verdict == (0, "", 0), name
        for key in keys:
            seen[key].add(key in raised)
    for (name, pos, _), p in zip(cases, batch):
        if pos is not None:
            p.free()
    return seen


@pytest.mark.parametrize("cfg", [WIDE, AT_THE_LIMIT], ids=lambda c: "q%d" % c[3])
def test_every_device_check_says_no_on_its_own(backend, proofs, cfg):
    seen = _check_every_verdict(backend.L, proofs[("fib7", cfg)], cfg)
    # every FRI check was seen raised in one case and clear in another
    fri = [key for key in seen if key[0] != "tree"]
    assert ("first",) in fri and ("last",) in fri and sum(key[0] == "inner" for key in fri) == len(fri) - 2 >= 10
    assert all(seen[key] == {True, False} for key in seen), {k: v for k, v in seen.items() if v != {True, False}}


def test_the_limit(backend, proofs):
    """512 queries: 1024 nodes in a level, 64 KB of dynamic LDS, accepted.  700 queries: refused on the host, before any launch —
    the timing of the last launched call is untouched, no device memory is held, and the next call answers."""
    L = backend.L
    at = proofs[("fib7", AT_THE_LIMIT)]
    s = verify_plan_stats([at], AT_THE_LIMIT, L)[0]
    assert s["max_level_nodes"] == 1024 and s["merkle_lds_bytes"] == 65536
    assert verify_many([at], AT_THE_LIMIT, L) == [(0, "")] == [at.verify(AT_THE_LIMIT)]
    above = proofs[("fib7", ABOVE_THE_LIMIT)]
    assert above.verify(ABOVE_THE_LIMIT) == (0, "")
    assert verify_plan_stats([above], ABOVE_THE_LIMIT, L)[0]["max_level_nodes"] > 1024
    # a batch shares one expected config: the good proof next to the wide one is either made under it too (and as wide), or a
    # proof of another config, which the verifier decides in front of the queries and which plans nothing
    other = proofs[("fib7", WIDE)]
    before, launched = mem_stats(L).live_bytes, verify_many_timing(L)
    for batch in ([above], [other, above], [above, other], [above, above]):
        with pytest.raises(CmError) as e:
            verify_many(batch, ABOVE_THE_LIMIT, L)
        assert str(e.value) == "libcairom_hip status 1: " + REFUSAL
        with pytest.raises(CmError) as e:
            verify_many_detail(batch, ABOVE_THE_LIMIT, L)
        assert str(e.value) == "libcairom_hip status 1: " + REFUSAL
        rc, msg = verify_run(batch, ABOVE_THE_LIMIT, L, device=True)
        assert (rc, msg) == (1, REFUSAL)
    after = verify_many_timing(L)
    assert [after[k] for k in ("upload", "kernels", "download")] == [launched[k] for k in ("upload", "kernels", "download")]
    assert mem_stats(L).live_bytes == before
    assert verify_many([at, proofs[("u32", AT_THE_LIMIT)]], AT_THE_LIMIT, L) == [(0, ""), (0, "")]
    assert mem_stats(L).live_bytes == before


def test_rfc_framing_at_300_queries(backend):
    """k_verify_merkle<true>: the RFC node framing counts bytes on its own path; the accept case and every verdict case again"""
    L = backend.L
    try:
        set_framing("hash_node=rfc", L)
        inp = synth_fibonacci(7)
        p = backend.prove(inp, WIDE)
        inp.free()
        assert verify_many([p], WIDE, L) == [(0, "")] == [p.verify(WIDE)]
        seen = _check_every_verdict(L, p, WIDE)
        assert all(seen[key] == {True, False} for key in seen)
        p.free()
    finally:
        set_framing("", L)
