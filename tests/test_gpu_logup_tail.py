"""The LogUp tail scan (logup_finalize_all, kernels_air.inc), exactly, one case per path.  The running sum of the last interaction
column is scanned by one k_scan_local block up to 2^10 rows, by several blocks joined by k_scan_blocks at 2^11 and 2^12, and by
k_scan2_paired from 2^13 on (U = log - 11 unrolled steps: U = 2 is the smallest, 3 and 5 follow).  synth_fibonacci(n) puts about
4n rows into its largest opcode component (store_add_fp_fp), so n picks the path; the component's size is asserted.  For that
component cm_trace_write then cm_interaction_write must equal the oracle's interaction columns — every one, the scanned last one
included — and the claimed sum, word for word.  2^4 rows is the partially filled single block."""
import numpy as np
import pytest

from cairo_m_amd.lib import N_PREPROCESSED, PREPROCESSED_LOG, RELATION_WORDS, synth_fibonacci

pytestmark = pytest.mark.gpu
P = 2**31 - 1


@pytest.fixture(scope="module")
def preprocessed(backend):
    cols = []
    for k in range(N_PREPROCESSED):
        h = backend.col_alloc(1 << PREPROCESSED_LOG[k])
        backend.preprocessed_column(k, h)
        cols.append(h)
    yield cols
    for h in cols:
        backend.col_free(h)


@pytest.mark.parametrize("n,log", [(2, 4), (150, 10), (300, 11), (700, 12), (1500, 13), (3000, 14), (13000, 16)])
def test_logup_tail_paths_equal_the_oracle(backend, oracle, preprocessed, n, log):
    inp = synth_fibonacci(n)
    dev = backend.upload_input(inp)
    logs = [backend.component_log_size(dev, cid) for cid in range(26)]
    cid = int(np.argmax(logs))
    assert logs[cid] == log, (n, logs)
    n_tr, n_it, _ = backend.component_info(cid)
    rel = np.random.default_rng(8800 + log).integers(0, P, size=RELATION_WORDS, dtype=np.uint32)
    cols = [backend.col_alloc(1 << log) for _ in range(n_tr)]
    out = [backend.col_alloc(1 << log) for _ in range(n_it)]
    try:
        backend.trace_write(dev, cid, cols)
        cs = backend.interaction_write(cid, cols, preprocessed, log, rel, out)
        got = np.stack([backend.download(h, 1 << log) for h in out])
        want, want_cs = oracle.component_interaction(inp.view, cid, rel, n_it, log)
        for k in range(n_it):
            diff = np.flatnonzero(got[k] != want[k])
            assert diff.size == 0, (n, cid, "interaction column", k, "of", n_it, "first differing row", int(diff[0]))
        assert np.array_equal(cs, want_cs), (n, cid, "claimed sum")
    finally:
        for h in cols + out:
            backend.col_free(h)
        backend.free_input(dev)
        inp.free()
