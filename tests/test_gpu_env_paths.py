"""Code paths that only an environment variable selects keep the proof bytes.

The library reads these switches once per process into static values, so cm_set_tuning and monkeypatching cannot flip them:
each case starts `python -m tests.env_path_child` as a fresh process with the variables set, which proves fib(3000) and
u32_loop_program(40) twice each and writes the proof words; the parent asserts exit status 0 and word equality with the oracle's
proof (computed once per module).  CM_FFT_OLD_PLAN, CM_SCAN_PAIRED and CM_COL_SKEW_BYTES also prove fib(30 000) and fib(40 000).
The largest component of fib(n) has about 4n rows: 2^17 at 30 000 (old plan 11 + 7 at 2^18, scan at U = 6) and 2^18 at 40 000,
which takes the old plan's three passes 11 + 4 + 4 at 2^19 and the scan at U = 7.  The expected words for those inputs are the
default-environment proofs made in the parent (test_configs1 pins the default path to the oracle at 100 000).
CM_FRI_PLAN_GENERIC is read by the host's decommitment planner, which only runs with the device tail off: the case that sets it
together with CM_DEVICE_TAIL=0 is the one that reaches it.  CM_FRI_TAIL_LOG=1 means no tail launch at all (the last layer has 2
values): every layer takes the per-layer path, which is what that case exercises.

Children run one at a time (the parent and one child hold the GPU: two processes), each under subprocess.run(timeout=...).  The
limit is ten times the wall time of the default-environment child, with a floor of 60 s.  Measured on an MI355X: that child
takes 0.7 s from start to exit (0.53 s inside it, library load to last proof), and the child that also proves fib(30 000) and
fib(40 000) 0.9 s (0.68 s inside), so ten times either is below the floor and the limit is 60 s.  A child that ends with any
status but 0 or at its limit sets a module flag, and every later case fails at once without starting a process: nothing more
runs on a GPU that has just faulted or hung.  Run the module with -x.

Left out on purpose: CM_FLAG_MEM (the memory kind of the spin flags, not a result), the logging switches (CM_HOST_TRACE,
CM_HOST_MARKS, CM_ADAPTER_TAIL_LOG, CM_QUIET, CM_KPROF_EXT) and CM_FLAG_JOIN_DEBUG.

CM_HOST_B2S_NO_AVX512=1 is host code and its test needs no GPU: a child with the variable set gives the verdicts and messages
the parent gives without it, for an oracle-made proof of fib(7) and each hand-placed tampering of it.  On a CPU without AVX-512
both sides take the portable path and the test compares it with itself; the GPU machines have AVX-512."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = ["fib3000", "u32loop40"]
BIG = ["fib30000", "fib40000"]
CHILD_WALL_S = 0.7          # default-environment child (both small inputs, twice each), start to exit, measured on an MI355X
CHILD_LIMIT_S = max(60.0, 10 * CHILD_WALL_S)

_gpu_lost = []   # why, once a child ended with a non-zero status or at its limit

# (id, environment, also prove the two larger inputs)
CASES = [
    ("default", {}, False),
    ("fft_old_plan", {"CM_FFT_OLD_PLAN": "1"}, True),
    ("scan_unpaired", {"CM_SCAN_PAIRED": "0"}, True),
    ("no_merkle_top", {"CM_NO_MERKLE_TOP": "1"}, False),
    ("no_small_commit", {"CM_NO_SMALL_COMMIT": "1"}, False),
    ("no_small_batch", {"CM_NO_SMALL_BATCH": "1"}, False),
    ("fri_plan_generic", {"CM_FRI_PLAN_GENERIC": "1"}, False),
    # the host plans a decommitment only when the device tail is off: alone, the switch above selects nothing
    ("fri_plan_generic_host_tail", {"CM_FRI_PLAN_GENERIC": "1", "CM_DEVICE_TAIL": "0"}, False),
    ("fri_tail_log_1", {"CM_FRI_TAIL_LOG": "1"}, False),
    ("fri_tail_log_7", {"CM_FRI_TAIL_LOG": "7"}, False),
    ("fri_tail_log_13", {"CM_FRI_TAIL_LOG": "13"}, False),
    ("no_early_acc_interp", {"CM_NO_EARLY_ACC_INTERP": "1"}, False),
    ("host_oods", {"CM_HOST_OODS": "1"}, False),
    ("col_skew_256", {"CM_COL_SKEW_BYTES": "256"}, True),
    ("col_skew_4096", {"CM_COL_SKEW_BYTES": "4096"}, True),
    ("pipe_prio_minus_1", {"CM_PIPE_PRIO": "-1"}, False),
    ("pipe_prio_1", {"CM_PIPE_PRIO": "1"}, False),
    ("pipe_prio_0_stream_1", {"CM_PIPE_PRIO": "0", "CM_PIPE_STREAM": "1"}, False),
]
SWITCHES = sorted({k for _, env, _ in CASES for k in env})


def _child_env(extra):
    env = {k: v for k, v in os.environ.items() if k not in SWITCHES}   # a switch set around the test run must not leak into a case
    env.update(extra)
    return env


@pytest.fixture(scope="module")
def expected(backend, oracle):
    """name -> the words every path must produce: the oracle's proof of the small inputs, the parent's default-path proofs of the two larger ones"""
    from tests.env_path_child import make_input
    want = {}
    for name in SMALL:
        inp = make_input(name)
        want[name] = oracle.prove(inp.view)[0]
        inp.free()
    for name in BIG:
        inp = make_input(name)
        p = backend.prove(inp)
        want[name] = p.words().copy()
        p.free()
        inp.free()
    return want


@pytest.mark.gpu
@pytest.mark.parametrize("env,big", [(e, b) for _, e, b in CASES], ids=[i for i, _, _ in CASES])
def test_env_selected_path_keeps_the_proof_bytes(expected, tmp_path, env, big):
    if _gpu_lost:
        pytest.fail("not started: " + _gpu_lost[0])
    names = SMALL + (BIG if big else [])
    cmd = [sys.executable, "-m", "tests.env_path_child", "prove", str(tmp_path), ",".join(names)]
    try:
        r = subprocess.run(cmd, cwd=ROOT, env=_child_env(env), capture_output=True, text=True, timeout=CHILD_LIMIT_S)
    except subprocess.TimeoutExpired:
        _gpu_lost.append(f"the child with {env} did not end within {CHILD_LIMIT_S} s")
        pytest.fail(_gpu_lost[0])
    if r.returncode != 0:   # a signal, a time limit, or a HIP error the child met as an exception: the GPU may be faulted
        _gpu_lost.append(f"the child with {env} ended with status {r.returncode}: {r.stderr[-400:]}")
    assert r.returncode == 0, (env, r.returncode, r.stderr[-2000:])
    out = json.loads(r.stdout.strip().splitlines()[-1])
    print(f"child {env}: {out['wall_s']} s")
    assert sorted(out["files"]) == sorted(names)
    for name in names:
        assert len(out["files"][name]) == 2
        for k, path in enumerate(out["files"][name]):
            got = np.load(path)
            want = expected[name]
            assert got.size == want.size, (env, name, k, got.size, want.size)
            diff = np.flatnonzero(got != want)
            assert diff.size == 0, (env, name, k, "first differing word", int(diff[0]), "of", got.size)


@pytest.mark.gpu
def test_no_merkle_top_stores_every_layer(backend):
    """CM_NO_MERKLE_TOP=1 in one fresh process: the shapes NO_TOP_SHAPES of tests/merkle_op_shapes.py become k_merkle_multi groups
    of 4 + 4, 3 and 2 levels, each above a k_merkle_tail with a previous layer, and the child compares the root and every node of
    every stored layer with the oracle (the proof-parity case above touches some 80 query paths per tree).  Same limit and the
    same rule as the other children: a child that ends badly stops every later case."""
    if _gpu_lost:
        pytest.fail("not started: " + _gpu_lost[0])
    env = {"CM_NO_MERKLE_TOP": "1"}
    cmd = [sys.executable, "-m", "tests.env_path_child", "merkle_layers"]
    try:
        r = subprocess.run(cmd, cwd=ROOT, env=_child_env(env), capture_output=True, text=True, timeout=CHILD_LIMIT_S)
    except subprocess.TimeoutExpired:
        _gpu_lost.append(f"the merkle_layers child with {env} did not end within {CHILD_LIMIT_S} s")
        pytest.fail(_gpu_lost[0])
    if r.returncode != 0 and "AssertionError" not in r.stderr:   # a comparison that fails is a finding, not a lost GPU
        _gpu_lost.append(f"the merkle_layers child with {env} ended with status {r.returncode}: {r.stderr[-400:]}")
    assert r.returncode == 0, (env, r.returncode, r.stderr[-2000:])
    out = json.loads(r.stdout.strip().splitlines()[-1])
    print(f"merkle_layers child {env}: {out['wall_s']} s")
    M, T = "multi", "tail"
    assert out["plans"] == [[[M, 16, 13, False], [M, 12, 9, True], [T, 8, 0, True]], [[M, 11, 9, False], [T, 8, 0, True]],
                            [[M, 10, 9, False], [T, 8, 0, True]]]


def test_host_blake2s_without_avx512_gives_the_same_verdicts(oracle, tmp_path):
    from cairo_m_amd.lib import load_library, synth_fibonacci
    from tests.verify_many_util import hand_flips, host_verify_words
    L = load_library()
    inp = synth_fibonacci(7)
    words, _ = oracle.prove(inp.view)
    inp.free()
    flips = {name: int(pos) for name, pos in hand_flips(words).items()}
    want = {"": list(host_verify_words(L, words))}
    for name, pos in flips.items():
        bad = words.copy()
        bad[pos] ^= 1
        want[name] = list(host_verify_words(L, bad))
    assert want[""] == [0, ""] and all(v[0] == 11 and v[1] for k, v in want.items() if k), want
    np.save(tmp_path / "words.npy", words)
    (tmp_path / "flips.json").write_text(json.dumps(flips))
    cmd = [sys.executable, "-m", "tests.env_path_child", "verify", str(tmp_path / "words.npy"), str(tmp_path / "flips.json")]
    r = subprocess.run(cmd, cwd=ROOT, env=dict(os.environ, CM_HOST_B2S_NO_AVX512="1"), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    got = json.loads(r.stdout.strip().splitlines()[-1])["verdicts"]
    assert got == want
