"""BASELINE configs[2] and configs[4] workloads on the GPU.

* all-opcode program (cairo_m_amd/workloads.py::all_opcodes_program, operands from xorshift32(0xC0FFEE)): the HIP witness
  kernels against the golden cells derived mechanically from the reference's write_trace closures
  (tests/golden/air_witness_vectors.npz) — HIP vs reference-derived data, no oracle in between; the whole proof
  bit-identical to the oracle's; at 2^20 steps through the device adapter, accepted by both verifiers.
* SHA-256 (examples/sha256-cairo-m algorithm on the u32 opcodes): the VM digest equals hashlib's, the HIP proof equals the
  oracle's bit for bit, a multi-block message verifies."""
import hashlib
import os

import numpy as np
import pytest

from cairo_m_amd.lib import prover_input_arrays, vm_run, vm_segment
from cairo_m_amd.workloads import all_opcodes_program, sha256_program

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = np.load(os.path.join(ROOT, "tests", "golden", "air_witness_vectors.npz"))
from tests.test_air_witness_golden import OPCODE_FILES  # noqa: E402


def test_hip_witness_equals_reference_derived_cells(backend):
    prog, steps = all_opcodes_program(int(GOLD["iters"][0]), int(GOLD["seed"][0]))
    inp = vm_run(prog, entry_pc=0, args=(), n_returns=0)
    assert inp.steps == steps
    dev = backend.upload_input(inp)
    checked = 0
    for cid, name in list(enumerate(OPCODE_FILES)) + [(26, "memory"), (27, "merkle")]:
        if name not in GOLD.files:
            continue
        want = GOLD[name]
        log = backend.component_log_size(dev, cid)
        assert want.shape[1] == 1 << log
        cols = [backend.col_alloc(1 << log) for _ in range(want.shape[0])]
        backend.trace_write(dev, cid, cols)
        got = np.stack([backend.download(h, 1 << log) for h in cols])
        bad = np.argwhere(got != want)
        assert bad.size == 0, f"{name}: first differing (column, row) {bad[:5].tolist()}"
        for h in cols:
            backend.col_free(h)
        checked += 1
    assert checked == 28          # 26 opcode components + memory + merkle
    # poseidon2 (443 columns): the first 192 rows (the golden holds the first 200 hash inputs of the run)
    log = backend.component_log_size(dev, 29)
    cols = [backend.col_alloc(1 << log) for _ in range(443)]
    backend.trace_write(dev, 29, cols)
    got = np.stack([backend.download(h, 192) for h in cols])
    assert np.array_equal(got, GOLD["poseidon2"][:, :192])
    for h in cols:
        backend.col_free(h)
    # the four multiplicity columns against bincounts of the reference closures' recorded lookup_data (air_lookup_vectors.npz)
    from tests.test_gpu_air_edge_golden import check_histogram
    lookups = np.load(os.path.join(ROOT, "tests", "golden", "air_lookup_vectors.npz"))
    assert int(lookups["iters"][0]) == int(GOLD["iters"][0]) and int(lookups["seed"][0]) == int(GOLD["seed"][0])
    check_histogram(backend, dev, lookups, "all-opcode program")
    backend.free_input(dev)
    inp.free()


def test_all_opcodes_proof_bit_exact(backend, oracle):
    prog, steps = all_opcodes_program(300)
    inp = vm_run(prog, entry_pc=0, args=(), n_returns=0)
    assert inp.steps == steps
    p = backend.prove(inp)
    want, _ = oracle.prove(inp.view)
    got = p.words()
    assert got.size == want.size and np.array_equal(got, want)
    assert p.verify()[0] == 0
    p.free()
    inp.free()


def test_all_opcodes_at_2pow20_steps_verifies(backend, oracle):
    """configs[4] shape on one GPU: every opcode component live at ~2^20 steps in one segment, runner segment -> device
    adapter -> HIP prover; both verifiers accept."""
    iters = 24_000
    prog, steps = all_opcodes_program(iters)
    assert 2**19 < steps < 2**20
    hs = vm_segment(prog, entry_pc=0, args=(), n_returns=0)
    dev = backend.adapt_segment(hs)
    p = backend.prove_device(dev)
    st = p.stats()
    assert st["steps"] == steps
    rc, err = p.verify()
    assert rc == 0, err
    rc, err = oracle.verify(p.words())
    assert rc == 0, err
    p.free()
    backend.free_input(dev)
    hs.free()


def test_configs4_all_opcodes_at_2pow26_rows_verifies(backend, oracle):
    """BASELINE configs[4] at its full size on ONE GPU: the all-opcode loop with 67 207 510 steps (2^26 rows, 5.9e9 committed
    cells, ~116 GiB of the 288 GiB HBM3E); runner segment -> device adapter -> HIP prover; both verifiers accept.  The oracle
    PROVER is not run at this size (minutes); bit-exactness of the same program is checked at 300 iterations above."""
    import ctypes as C

    def free_hbm():
        f, t = C.c_uint64(0), C.c_uint64(0)
        assert backend.L.cm_device_mem_info(C.byref(f), C.byref(t)) == 0
        return f.value
    free = free_hbm()
    if free < 150 * 2**30:
        pytest.skip("needs ~116 GiB of free HBM")
    prog, steps = all_opcodes_program(1_545_000)
    assert 2**26 < steps < 2**26 + 2**18
    hs = vm_segment(prog, entry_pc=0, args=(), n_returns=0)
    dev = backend.adapt_segment(hs)
    hs.free()
    p = backend.prove_device(dev)
    st = p.stats()
    assert st["steps"] == steps and st["cells"] > 5.9e9
    rc, err = p.verify()
    assert rc == 0, err
    rc, err = oracle.verify(p.words())
    assert rc == 0, err
    p.free()
    backend.free_input(dev)
    assert backend.L.cm_pool_trim() == 0     # hand the ~116 GiB of cached blocks back before the next test
    assert free_hbm() > free - 8 * 2**30


def _digest(inp, slots):
    a = prover_input_arrays(inp.view)
    fp = a["regs"][1]
    fin = {int(r[0]): int(r[1]) for r in a["final_memory"]}
    return b"".join(((fin[fp + s + 1] << 16) | fin[fp + s]).to_bytes(4, "big") for s in slots)


def test_sha256_digest_and_proof_bit_exact(backend, oracle):
    msg = b"abc"
    prog, slots = sha256_program(msg)
    inp = vm_run(prog, entry_pc=0, args=(), n_returns=0)
    assert _digest(inp, slots) == hashlib.sha256(msg).digest()
    p = backend.prove(inp)
    want, _ = oracle.prove(inp.view)
    got = p.words()
    assert got.size == want.size and np.array_equal(got, want)
    assert p.verify()[0] == 0
    p.free()
    inp.free()


def test_sha256_multi_block_verifies(backend, oracle):
    msg = bytes(range(256)) * 4          # 1 KiB -> 17 blocks, ~59 k steps, straight-line program
    prog, slots = sha256_program(msg)
    inp = vm_run(prog, entry_pc=0, args=(), n_returns=0)
    assert _digest(inp, slots) == hashlib.sha256(msg).digest()
    p = backend.prove(inp)
    rc, err = p.verify()
    assert rc == 0, err
    rc, err = oracle.verify(p.words())
    assert rc == 0, err
    p.free()
    inp.free()
