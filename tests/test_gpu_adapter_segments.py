"""The device adapter (cm_adapt_segment_device: adapter_device.hip) on hand-built segments (tests/adapter_segments.py): clock gaps
at LIMIT - 1 .. 2 LIMIT + 1 on every kind of cell, wave / block boundaries of the sorted log, one-bit address sorts, absent
components, partial Merkle trees over chosen boundary memories, refusals.  The small cases are compared with the numpy
reference, the gap ladder (2.1 M steps) with cm_adapt_segment_host, which tests/test_adapter_segments_cpu.py holds to the same
reference; that file also asserts that every segment here still shows what it was built to reach.  No proofs: synthetic values do
not satisfy the AIR."""
import numpy as np
import pytest

from cairo_m_amd.lib import CmError, adapt_segment_host, prover_input_arrays
from tests import adapter_segments as S
from tests.test_gpu_adapter import _same

pytestmark = pytest.mark.gpu


def device_arrays(backend, seg, entries=False):
    a = seg.array_segment()
    dev = backend.adapt_segment(a)
    back = backend.download_input(dev)
    out = prover_input_arrays(back.view)
    pub = backend.public_entries(dev) if entries else None
    back.free()
    backend.free_input(dev)
    return (out, pub) if entries else out


def _device_equals_reference(backend, seg):
    ref = S.reference(seg)
    got, pub = device_arrays(backend, seg, entries=True)
    _same(ref, got)
    _same(S.public_entries(ref), pub)


def test_gap_ladder(backend):
    seg = S.gap_ladder()
    h = adapt_segment_host(seg.array_segment())
    want = prover_input_arrays(h.view)
    h.free()
    assert want["clock_updates"].shape[0] > 0
    _same(want, device_arrays(backend, seg))


@pytest.mark.parametrize("n_steps", S.LAYOUT_SIZES)
def test_layout_mix(backend, n_steps):
    _device_equals_reference(backend, S.layout_mix(n_steps))


FIXED = S.layout_fixed()


@pytest.mark.parametrize("name", sorted(FIXED))
def test_layout_fixed(backend, name):
    _device_equals_reference(backend, FIXED[name])


@pytest.mark.parametrize("device_trees", [False, True], ids=["default", "device_trees"])
@pytest.mark.parametrize("name", sorted(S.TREE_MEMORIES))
def test_trees(backend, monkeypatch, name, device_trees):
    """CM_ADAPTER_DEVICE_TREE_MIN=1 takes the level-by-level GPU builder (k_tree_flags / k_tree_level) for these tiny memories"""
    if device_trees:
        monkeypatch.setenv("CM_ADAPTER_DEVICE_TREE_MIN", "1")
    _device_equals_reference(backend, S.tree_segment(name))


def test_layout_with_device_trees(backend, monkeypatch):
    monkeypatch.setenv("CM_ADAPTER_DEVICE_TREE_MIN", "1")
    _device_equals_reference(backend, S.layout_mix(1000))


@pytest.mark.parametrize("name", sorted(S.refusals()))
def test_refusals(backend, name):
    seg, needle = S.refusals()[name]
    with pytest.raises(CmError, match=needle) as e:
        device_arrays(backend, seg)
    assert "status 1:" in str(e.value)
    _device_equals_reference(backend, S.layout_mix(2))          # the library goes on working


@pytest.mark.parametrize("new_words", [(4, 1, 2, 3), (50, 1, 2)], ids=["other_size", "same_size"])
def test_rewritten_code_is_refused_by_name(backend, new_words):
    """A fetch that logs another opcode than the memory at segment start holds: the host adapter and the reference follow the log
    (tests/test_adapter_segments_cpu.py); the device sizes every step's slice of the log by that memory and cannot, so it says so
    instead of "length does not match" or an input built from two different opcodes."""
    seg = S.rewritten_code(new_words)
    with pytest.raises(CmError) as e:
        device_arrays(backend, seg)
    assert "status 1:" in str(e.value) and "logged opcode differs from the memory at segment start" in str(e.value), str(e.value)
    assert "length does not match" not in str(e.value)
