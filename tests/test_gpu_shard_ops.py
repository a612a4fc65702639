"""The data-movement kernels of the sharded prover (kernels_shard.hip: k_pack_parity, k_halo_build, k_sum_copies<true | false>,
k_copy_segments) op by op through the C ABI (shard_ops.hip), bit for bit against tests/shard_ref.py: the previous-row model for
the halo, numpy for the sums and copies.  A slice handle is a column handle plus a word offset (a handle is the device address)."""
import numpy as np
import pytest

from tests import field_edges as fe
from tests import shard_ref as sr
from tests.field_edges import P

pytestmark = pytest.mark.gpu
GUARD = 0xA5A5A5A5          # no M31 word, and no sum of the counts below


def _free(backend, hs):
    for h in hs:
        backend.col_free(h)


def _at(h, words):
    return int(h) + 4 * int(words)


# ---- pack_parity + halo_build --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("half_len", [1, 255, 256, 257])
def test_pack_parity(backend, half_len):
    """k_pack_parity alone: dst[i] = src[2 i + parity] for one word, a block less one, a block, a block and one; the word behind the
    destination is untouched.  The source holds its own index, so a wrong index is visible as a value."""
    src = np.arange(2 * half_len, dtype=np.uint32) + np.uint32(1000)
    hs = backend.upload(src)
    try:
        for parity in (0, 1):
            hd = backend.upload(np.full(half_len + 1, GUARD, dtype=np.uint32))
            backend.pack_parity(hs, hd, half_len, parity)
            got = backend.download(hd, half_len + 1)
            backend.col_free(hd)
            assert np.array_equal(got[:half_len], sr.pack_parity(src, half_len, parity)), parity
            assert got[half_len] == GUARD, parity
    finally:
        backend.col_free(hs)


@pytest.fixture(scope="module")
def prev_rows():
    """Per n: the model's previous row of every storage row (trace_log = n - 1, what the prover passes: prover_sharded.inc hands
    k_halo_build n = clog + 1 and trace_log = clog for every split component, so no other relation reaches the kernel)."""
    cache = {}

    def get(n):
        if n not in cache:
            cache[n] = np.array([sr.shifted_row(r, n, n - 1, -1) for r in range(1 << n)], dtype=np.int64)
        return cache[n]
    return get


@pytest.mark.parametrize("n,log_ranks", [(9, 1), (9, 2), (9, 3), (13, 1), (13, 2), (13, 3), (6, 3)])
def test_halo_exchange(backend, prev_rows, n, log_ranks):
    """2, 4 and 8 ranks emulated on one column of 2^n words (n = 6 with 8 ranks: slices of 8 words): every rank packs both halves of
    its slice (k_pack_parity), rank R is handed the even half of rank brev(brev(R) - 1) and the odd half of rank brev(brev(R) + 1),
    and k_halo_build's out[q] equals the column at the model's previous row of row0 + q for every q, with err == 0.  Two columns:
    edge_mix, and one that holds its own index."""
    n_ranks, length = 1 << log_ranks, 1 << (n - log_ranks)
    half = length // 2
    prev = prev_rows(n)
    for column in (fe.edge_mix(np.random.default_rng(3000 + n), 1 << n), np.arange(1 << n, dtype=np.uint32)):
        hcol = backend.upload(column)
        halves = {}
        try:
            for r in range(n_ranks):
                for parity in (0, 1):
                    halves[(r, parity)] = backend.upload(np.full(half, GUARD, dtype=np.uint32))
                    backend.pack_parity(_at(hcol, r * length), halves[(r, parity)], half, parity)
            for r in range(n_ranks):
                src_even, src_odd = sr.halo_sources(r, log_ranks)
                ho = backend.upload(np.full(length + 1, GUARD, dtype=np.uint32))
                err = backend.halo_build(halves[(src_even, 0)], halves[(src_odd, 1)], src_even, src_odd, r * length, length, n, n - 1, log_ranks, ho)
                got = backend.download(ho, length + 1)
                backend.col_free(ho)
                assert err == 0, (r,)
                assert np.array_equal(got[:length], column[prev[r * length:(r + 1) * length]]), (r,)
                assert got[length] == GUARD, (r, "guard")
        finally:
            _free(backend, [hcol] + list(halves.values()))
    assert np.array_equal(sr.halo_reference(column, 0, 8, n, n - 1), column[prev[:8]])


def test_halo_wrong_neighbour_sets_the_error_word(backend, prev_rows):
    """The kernel's designed error path: halves announced as coming from a rank that is not the neighbour give err == 1, and the
    output words whose lookup fell outside stay unwritten — the even positions when the even source is wrong, all of them when
    both are; the positions of the right source are still filled."""
    n, log_ranks, r = 9, 2, 1
    length = 1 << (n - log_ranks)
    prev = prev_rows(n)
    column = np.arange(1 << n, dtype=np.uint32)
    src_even, src_odd = sr.halo_sources(r, log_ranks)
    hcol = backend.upload(column)
    he, hod = backend.col_alloc(length // 2), backend.col_alloc(length // 2)
    try:
        backend.pack_parity(_at(hcol, src_even * length), he, length // 2, 0)
        backend.pack_parity(_at(hcol, src_odd * length), hod, length // 2, 1)
        want = column[prev[r * length:(r + 1) * length]]
        for wrong_even, wrong_odd in ((True, False), (False, True), (True, True)):
            ho = backend.upload(np.full(length, GUARD, dtype=np.uint32))
            err = backend.halo_build(he, hod, r if wrong_even else src_even, r if wrong_odd else src_odd, r * length, length, n, n - 1, log_ranks, ho)
            got = backend.download(ho, length)
            backend.col_free(ho)
            assert err == 1
            assert (got[0::2] == GUARD).all() if wrong_even else np.array_equal(got[0::2], want[0::2])
            assert (got[1::2] == GUARD).all() if wrong_odd else np.array_equal(got[1::2], want[1::2])
    finally:
        _free(backend, [hcol, he, hod])


# ---- sum_copies ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("words", [1, 255, 257, 2**20 + 3])
def test_sum_copies(backend, words):
    """k_sum_copies<true> and <false> for 1, 2 and 8 copies: 2^20 + 3 words are more than the 4096 blocks of the launch hold, so
    the grid stride runs; stride = words + 5 with guard words in the gaps, which a wrong stride would add in.  Modular: all P-1
    (every partial sum wraps) and near_p; plain: counts near 2^32 whose sum wraps.  The word behind the output is untouched."""
    rng = np.random.default_rng(4000 + words % 1000)
    stride = words + 5
    for n_copies in (1, 2, 8):
        datas = [(True, fe.const(P - 1, n_copies * words)), (True, fe.near_p(rng, n_copies * words)),
                 (False, rng.integers(2**32 - 9, 2**32, size=n_copies * words, dtype=np.uint64).astype(np.uint32))]
        for modular, data in datas:
            buf = np.full(n_copies * stride, GUARD, dtype=np.uint32)
            for k in range(n_copies):
                buf[k * stride:k * stride + words] = data[k * words:(k + 1) * words]
            hi, ho = backend.upload(buf), backend.upload(np.full(words + 1, GUARD, dtype=np.uint32))
            try:
                backend.sum_copies(hi, n_copies, stride, words, ho, modular)
                got = backend.download(ho, words + 1)
            finally:
                _free(backend, [hi, ho])
            assert np.array_equal(got[:words], sr.sum_copies(buf, n_copies, stride, words, modular)), (n_copies, modular)
            assert got[words] == GUARD, (n_copies, modular, "guard")
            if not modular and n_copies > 1:
                assert int(data[0]) + int(data[words]) >= 2**32          # the sum did pass 2^32


# ---- copy_segments -------------------------------------------------------------------------------------------------------
def _copy_and_check(backend, sizes):
    """One call with segments of `sizes` words cut from one source buffer into one destination buffer, a guard word behind each."""
    src = (np.arange(sum(sizes), dtype=np.uint32) * np.uint32(2654435761)) >> np.uint32(1)
    s_off = [int(o) for o in np.cumsum([0] + list(sizes))]
    d_off = [int(o) for o in np.cumsum([0] + [w + 1 for w in sizes])]
    hs, hd = backend.upload(src), backend.upload(np.full(d_off[-1], GUARD, dtype=np.uint32))
    try:
        backend.copy_segments([(_at(hs, s_off[i]), _at(hd, d_off[i]), w) for i, w in enumerate(sizes)])
        got = backend.download(hd, d_off[-1])
    finally:
        _free(backend, [hs, hd])
    for i, w in enumerate(sizes):
        assert np.array_equal(got[d_off[i]:d_off[i] + w], src[s_off[i]:s_off[i] + w]), (i, w)
        assert got[d_off[i] + w] == GUARD, (i, w, "guard")


@pytest.mark.parametrize("sizes", [[0, 1, 1023, 1025, 300000], [300000], [5], [7] * 300], ids=["mixed", "one_large", "one_small", "300x7"])
def test_copy_segments(backend, sizes):
    """k_copy_segments: segments of 0, 1, 1023, 1025 and 300 000 words in one call — the largest asks for more than the 256 blocks a
    segment gets, so its blocks stride, and the small ones share that grid and mostly idle; a single segment; 300 segments of 7
    words.  Every destination equals its source and the guard word behind it is untouched."""
    _copy_and_check(backend, sizes)


def test_copy_segments_all_empty_is_a_no_op(backend):
    """No segment, and segments of no words (null handles allowed there), launch nothing and touch nothing."""
    hd = backend.upload(np.full(4, GUARD, dtype=np.uint32))
    try:
        backend.copy_segments([])
        backend.copy_segments([(0, 0, 0), (hd, hd, 0)])
        assert (backend.download(hd, 4) == GUARD).all()
    finally:
        backend.col_free(hd)
