"""The four kernels of the device-side proof tail (cairo_m_amd/csrc/tail_device.hip: k_tail_last, k_tail_grind, k_tail_tables,
k_tail_gather) and cm_bit_reverse, one at a time through the op-level entry points (cairo_m_amd/csrc/tail_ops.hip), on query sets,
nonces and coefficients this file chooses.  In a whole proof the transcript chooses them, so duplicate draws, a fully queried
layer, positions 0 and 2^L0 - 1, more than 1024 descriptors, a nonce in the second sweep or a last layer of one value come up by
luck or never.  Every comparison is bit-exact.  References, none of them the code under test:
  positions   mix_u64(nonce) and the raw draws of the oracle's Channel (oracle.query_draws), masked, sorted, made unique here;
  lists       tests/tail_lists_ref.py (the MerkleProver::decommit walk restated); the host mirror cm_tail_list must agree as well;
  gathers     numpy indexing of the uploaded arrays by the reference lists, pieces laid out at the reference offsets;
  grind       oracle.grind and the pow_zeros predicate of tests/test_ref_ops.py;
  last layer  chosen coefficients evaluated in Python integers at the line domain's points (oracle.domain_point), Blake2s of the
              oracle over digest || coefficients."""
import ctypes as C

import numpy as np
import pytest

from cairo_m_amd.lib import (TAIL_COORDS_W, TAIL_HASH_F, TAIL_HASH_W, TAIL_MISS, TAIL_NO_NONCE, TAIL_ROWS_U, set_framing)
from tests import field_edges as fe
from tests.field_edges import P
from tests.tail_lists_ref import ref_lists
from tests.test_ref_ops import pow_zeros
from tests.test_tail_lists import tail_list

pytestmark = pytest.mark.gpu

# (digest, nonce) of the table and gather cases: digests chosen by search with the reference so that, under both mix_u64 framings,
# the (1, 9) case queries both nodes; the second nonce has a non-zero high word
D0 = bytes.fromhex("575450f640675a5ef05e5a7ef0eac7d29e615ba886dfb33db867f09c51ec522e")
D1 = bytes.fromhex("f866422e1576a4a51bbe2e62013973343e976aee8db6296d20b5ca1fd566b024")
CASES = [(D0, 5), (D1, (1 << 32) + 3)]
# proof-of-work digests (default framing), each found by searching with oracle.grind on the CPU over Blake2s("tail-ops/<case>/<i>"),
# i = 0, 1, ..; the tests re-derive the property.  The first and the third are one-in-e^8 events (i = 1599 and 2335); the second,
# 256 / 2^14 rarer still (i = 245777), was found by testing the nonces of that block first and confirming with oracle.grind.
D_SWEEP2 = bytes.fromhex("e175bdd242dae5768f23d9036eec1a4bcd9258d822ed95c20262c92711710c15")      # oracle.grind(d, 14) = 154693: in [2^17, 2^18), the second sweep
D_LASTBLOCK = bytes.fromhex("04198d1950c8a352934f2afddc3ec4c40526f41d4db10323b28d176db9829e5e")   # oracle.grind(d, 14) = 131046: in [2^17 - 256, 2^17), block 511 of the first sweep
D_CAPPED = bytes.fromhex("f52cab15c0d83477a206f081c296c9f05cf05fd153f6c8eb96b9c20da5d02c6e")      # oracle.grind(d, 8) = 2175 >= 2^11: above "tail_grind_cap" = 12

SHAPES = [(1, 1, 1), (1, 9, 16), (3, 20, 32), (5, 7, 8), (10, 64, 64), (10, 65, 128), (10, 1024, 1024), (12, 300, 512),
          (16, 1023, 1024), (17, 30, 32), (31, 1024, 1024)]


def masks(L0):
    """qmask shapes that decide the F lists: none, every layer, only the top layer, alternating"""
    return [0, (2 << L0) - 1, 1 << L0, 0x55555555 & ((2 << L0) - 1)]


@pytest.fixture(params=["", "mix_u64=u32s"], ids=["mix_u64_raw", "mix_u64_u32s"])
def framing(request, backend, oracle):
    """both mix_u64 framings: k_tail_grind and k_tail_tables are templated on it"""
    set_framing(request.param, backend.L)
    oracle.set_framing(request.param)
    yield request.param
    set_framing("", backend.L)
    oracle.set_framing("")


def ref_positions(oracle, digest, nonce, nq, L0):
    """(sorted unique positions, the masked draws in draw order)"""
    drawn = [int(w) & ((1 << L0) - 1) for w in oracle.query_draws(digest, nonce, nq)]
    assert len(drawn) == nq
    return sorted(set(drawn)), drawn


def check_tables(backend, oracle, digest, nonce, nq, pad, L0, qmask, got=None):
    S, _ = ref_positions(oracle, digest, nonce, nq, L0)
    if got is None:
        got = backend.tail_tables(digest, nonce, nq, pad, L0, qmask)
    hdr = got["hdr"]
    assert hdr[0] == 0 and int(hdr[1]) | (int(hdr[2]) << 32) == nonce and hdr[8] == 1
    assert hdr[3] == len(S) and got["positions"].tolist() == S
    U, W, F = ref_lists(S, L0, qmask)
    for which, name, ref in ((0, "U", U), (1, "W", W), (2, "F", F)):
        assert got["cnt"][which][:L0 + 1].tolist() == [len(x) for x in ref], (name, L0, nq, qmask)
        assert not got["cnt"][which][L0 + 1:].any()
        for k in range(L0 + 1):
            assert got[name][k].tolist() == ref[k], (name, k, L0, nq, qmask)
            assert tail_list(backend.L, S, L0, qmask, which, k) == ref[k], ("host mirror", name, k, L0, nq, qmask)
    return S, (U, W, F), got


@pytest.mark.parametrize("L0,nq,pad", SHAPES)
def test_tables_equal_the_walk(backend, oracle, framing, L0, nq, pad):
    for digest, nonce in CASES:
        S, drawn = ref_positions(oracle, digest, nonce, nq, L0)
        if (L0, nq) == (3, 20):
            assert len(S) < nq, "duplicate draws: n_unique < n_queries"
        if (L0, nq) == (1, 9):
            assert S == [0, 1], "a full layer: both nodes queried"
        if pad == nq:
            assert pad & (pad - 1) == 0
        for qmask in masks(L0):
            _, (U, W, F), got = check_tables(backend, oracle, digest, nonce, nq, pad, L0, qmask)
            assert got["hdr"][4] == 0 and got["words"].size == 0
            if (L0, nq) == (1, 9):
                assert all(len(w) == 0 for w in W), "every W is empty when every node is queried"


def test_table_cases_cover_the_edges(oracle):
    """over the whole table: position 0, position 2^L0 - 1, a queried sibling pair and a lone node each occur (reference only)"""
    for spec in ("", "mix_u64=u32s"):
        oracle.set_framing(spec)
        try:
            seen = set()
            for L0, nq, _ in SHAPES:
                for digest, nonce in CASES:
                    S, _ = ref_positions(oracle, digest, nonce, nq, L0)
                    have = set(S)
                    seen |= {"zero"} if 0 in have else set()
                    seen |= {"top"} if (1 << L0) - 1 in have else set()
                    seen |= {"pair"} if any(p ^ 1 in have for p in S) else set()
                    seen |= {"lone"} if any(p ^ 1 not in have for p in S) else set()
            assert seen == {"zero", "top", "pair", "lone"}, (spec, seen)
        finally:
            oracle.set_framing("")


# ---- descriptors and gathers --------------------------------------------------------------------------------------------------
class TailData:
    """random arrays a decommitment gathers from, per shift k (layer l = L0 - k): H[k] the layer's hashes (8 words per node),
    C[k] four coordinate columns, R[k] a pool of five row columns; uploaded once, (handle, array) pairs"""

    def __init__(self, backend, L0, seed):
        rng = np.random.default_rng(seed)
        self.be, self.L0, self.handles = backend, L0, []

        def up(n):
            a = rng.integers(0, 2**32, size=n, dtype=np.uint32)
            h = backend.upload(a)
            self.handles.append(h)
            return (h, a)
        self.H = [up(8 << (L0 - k)) for k in range(L0 + 1)]
        self.C = [[up(1 << (L0 - k)) for _ in range(4)] for k in range(L0 + 1)]
        self.R = [[up(1 << (L0 - k)) for _ in range(5)] for k in range(L0 + 1)]

    def piece(self, kind, k, width=0, salt=0):
        """(kind, k, [(handle, array)]): F pieces index layer l + 1, row pieces repeat the pool's handles"""
        if kind == TAIL_HASH_W:
            return (kind, k, [self.H[k]])
        if kind == TAIL_HASH_F:
            return (kind, k, [self.H[k - 1]])
        if kind == TAIL_COORDS_W:
            return (kind, k, self.C[k])
        return (kind, k, [self.R[k][(3 * c + salt) % 5] for c in range(width)])

    def free(self):
        for h in self.handles:
            self.be.col_free(h)


def ref_gather(spec, lists):
    """the witness stream: pieces in descriptor order -> (offsets, words)"""
    U, W, F = lists
    offsets, parts, total = [], [], 0
    for kind, k, cols in spec:
        idx = np.asarray({TAIL_HASH_W: W, TAIL_HASH_F: F, TAIL_COORDS_W: W, TAIL_ROWS_U: U}[kind][k], dtype=np.int64)
        if kind in (TAIL_HASH_W, TAIL_HASH_F):
            w = cols[0][1].reshape(-1, 8)[idx].ravel()
        else:
            w = np.stack([a[idx] for _, a in cols], axis=1).ravel() if idx.size else np.zeros(0, dtype=np.uint32)
        offsets.append(total)
        parts.append(w)
        total += w.size
    return offsets, (np.concatenate(parts) if parts else np.zeros(0, dtype=np.uint32))


def run_gather(backend, oracle, data, spec, digest, nonce, nq, pad, qmask):
    L0 = data.L0
    got = backend.tail_tables(digest, nonce, nq, pad, L0, qmask, [(kind, k, [h for h, _ in cols]) for kind, k, cols in spec])
    _, lists, _ = check_tables(backend, oracle, digest, nonce, nq, pad, L0, qmask, got=got)
    offsets, words = ref_gather(spec, lists)
    assert got["offsets"].tolist() == offsets
    assert got["hdr"][4] == words.size, "total words against the reference sum"
    assert np.array_equal(got["words"], words)
    return lists, offsets


@pytest.fixture(scope="module")
def data4(backend):
    d = TailData(backend, 4, 41)
    yield d
    d.free()


@pytest.fixture(scope="module")
def data10(backend):
    d = TailData(backend, 10, 42)
    yield d
    d.free()


def every_kind(data):
    L0 = data.L0
    spec = [data.piece(TAIL_HASH_W, k) for k in range(L0 + 1)]
    spec += [data.piece(TAIL_COORDS_W, k) for k in (0, 1, L0)]      # W[L0] is empty: the root has no sibling
    spec += [data.piece(TAIL_HASH_F, k) for k in range(L0, 0, -1)]
    spec += [data.piece(TAIL_ROWS_U, k, w, salt) for salt, (k, w) in enumerate([(0, 1), (1, 255), (0, 256), (2, 257), (0, 600), (L0, 3)])]
    return spec


@pytest.mark.parametrize("L0,nq,pad", [(4, 20, 32), (4, 64, 64), (10, 300, 512), (10, 1024, 1024)])   # small_y = 1, 2, 10, 32
def test_gathers_every_kind_and_width(backend, oracle, framing, data4, data10, L0, nq, pad):
    data = data4 if L0 == 4 else data10
    spec = every_kind(data)
    digest, nonce = CASES[(nq >> 2) & 1]
    for qmask in masks(L0)[1:]:
        lists, offsets = run_gather(backend, oracle, data, spec, digest, nonce, nq, pad, qmask)
        assert len(lists[1][L0]) == 0 and offsets[L0 + 3] == offsets[L0 + 4], "a piece whose list is empty"


def test_gather_more_than_1024_descriptors(backend, oracle, data4):
    """1030 descriptors over shared small buffers: the offset scan's carry from the first 1024 into the rest"""
    small = []
    for i in range(1003):
        kind = (TAIL_HASH_W, TAIL_HASH_F, TAIL_COORDS_W)[i % 3]
        small.append(data4.piece(kind, 1 + i % 4 if kind == TAIL_HASH_F else i % 5))
    rows = [data4.piece(TAIL_ROWS_U, i % 5, 1 + i % 7, i) for i in range(27)]
    spec = small + rows
    assert len(spec) == 1030
    lists, offsets = run_gather(backend, oracle, data4, spec, D0, 5, 20, 32, 0x15)
    assert offsets[1024] > offsets[1023] > 0 and offsets[-1] > offsets[1024]


def test_a_missed_nonce_comes_back_as_no_nonce_and_nothing_else(backend, data4):
    spec = every_kind(data4)
    got = backend.tail_tables(D0, TAIL_MISS, 20, 32, 4, 0x15, [(kind, k, [h for h, _ in cols]) for kind, k, cols in spec])
    hdr = got["hdr"]
    assert hdr[0] == TAIL_NO_NONCE and hdr[1] == hdr[2] == 0xFFFFFFFF
    assert hdr[3] == 0 and hdr[4] == 0 and hdr[8] == 1
    assert not got["cnt"].any() and not got["offsets"].any() and got["words"].size == 0


# ---- proof of work ---------------------------------------------------------------------------------------------------------------
def test_tail_grind_equals_the_oracle(backend, oracle, framing):
    rng = np.random.default_rng(7)
    for bits in (0, 2, 8, 12, 14):
        digest = bytes(rng.integers(0, 256, size=32, dtype=np.uint8))
        want = oracle.grind(digest, bits)
        if framing == "":
            assert pow_zeros(digest, want) >= bits and (want == 0 or pow_zeros(digest, want - 1) < bits)
        assert want < 1 << max(bits + 4, 8), "inside the search limit (a miss has probability e^-16)"
        assert backend.tail_grind(digest, bits) == want, bits


def test_tail_grind_second_sweep(backend, oracle):
    want = oracle.grind(D_SWEEP2, 14)
    assert 1 << 17 <= want < 1 << 18, "the case: a smallest nonce behind the first sweep of 2^17, inside the limit of 2^18"
    assert pow_zeros(D_SWEEP2, want) >= 14
    assert backend.tail_grind(D_SWEEP2, 14) == want


def test_tail_grind_last_block_of_the_first_sweep(backend, oracle):
    want = oracle.grind(D_LASTBLOCK, 14)
    assert (1 << 17) - 256 <= want < 1 << 17, "the case: block 511 of the 512-block grid"
    assert backend.tail_grind(D_LASTBLOCK, 14) == want


def test_tail_grind_miss_under_the_cap(backend, oracle):
    """"tail_grind_cap" = 12 ends the search after 2^11 nonces: a digest whose nonce lies above that leaves the cell at ~0"""
    want = oracle.grind(D_CAPPED, 8)
    assert 1 << 11 <= want < 1 << 12, "the case: above the cap, inside the uncapped limit"
    try:
        assert backend.L.cm_set_tuning(b"tail_grind_cap", C.c_int32(12)) == 0
        assert backend.tail_grind(D_CAPPED, 8) == TAIL_MISS
    finally:
        assert backend.L.cm_set_tuning(b"tail_grind_cap", C.c_int32(0)) == 0
    assert backend.tail_grind(D_CAPPED, 8) == want


# ---- the last layer ----------------------------------------------------------------------------------------------------------------
def bitrev(i, bits):
    return int(format(i, "0%db" % bits)[::-1], 2) if bits else 0


def line_evaluations(oracle, ordered, log_n):
    """ordered[p] = the QM31 coefficient (4 words) of the basis element prod_{bit k of p} pi^k(x), pi(x) = 2 x^2 - 1.  Returns the
    four coordinate columns of the evaluations on the line domain half_odds(log_n) — its point j is point j of
    CanonicCoset(log_n + 1).circle_domain() — in bit-reversed order."""
    n = 1 << log_n
    cols = np.zeros((4, n), dtype=np.uint32)
    for i in range(n):
        x = oracle.domain_point(log_n + 1, bitrev(i, log_n))[0]
        pis = []
        for _ in range(log_n):
            pis.append(x)
            x = (2 * x * x - 1) % P
        acc = [0, 0, 0, 0]
        for p, c in enumerate(ordered):
            m = 1
            for k in range(log_n):
                if p >> k & 1:
                    m = m * pis[k] % P
            acc = [(a + m * int(w)) % P for a, w in zip(acc, c)]
        cols[:, i] = acc
    return cols


def run_last(backend, oracle, digest, ordered, log_n, log_keep, ar):
    cols = line_evaluations(oracle, ordered, log_n)
    hs = [backend.upload(c) for c in cols]
    try:
        dig, flag, last, ar_out, cell = backend.tail_last(digest, hs, log_n, log_keep, ar)
    finally:
        for h in hs:
            backend.col_free(h)
    assert np.array_equal(last, cols), "the evaluations handed to the host"
    assert np.array_equal(ar_out, ar), "the copy of the challenges and roots"
    assert cell == TAIL_MISS, "the nonce cell is armed"
    return dig, flag


@pytest.mark.parametrize("log_n", [0, 1, 2, 3, 6])
def test_last_layer_from_chosen_coefficients(backend, oracle, log_n):
    """(the prover's last layer can have one value — DeviceTail::supported does not refuse log_n = 0 — so the entry takes it too)"""
    rng = np.random.default_rng(100 + log_n)
    n = 1 << log_n
    digest = bytes(rng.integers(0, 256, size=32, dtype=np.uint8))
    for log_keep in range(log_n + 1):
        keep = 1 << log_keep
        sets = [rng.integers(0, P, size=(keep, 4), dtype=np.uint32), fe.edge_mix(rng, 4 * keep).reshape(keep, 4)]
        sets += [fe.const(v, 4 * keep).reshape(keep, 4) for v in (0, 1, P - 1, 2**30)]
        for i, lp in enumerate(sets):                      # lp: the kept coefficients in LinePoly order
            ar = rng.integers(0, 2**32, size=12 * (20 if i & 1 else 1), dtype=np.uint32)
            ordered = [lp[bitrev(p, log_keep)] for p in range(keep)]
            dig, flag = run_last(backend, oracle, digest, ordered, log_n, log_keep, ar)
            assert flag == 0
            assert dig == oracle.blake2s(digest + lp.astype("<u4").tobytes()), (log_n, log_keep, i)
        for extra in sorted({keep, n - 1}):                 # one non-zero coefficient above the bound
            if extra < keep or extra >= n:
                continue
            lp = sets[0]
            ordered = [lp[bitrev(p, log_keep)] for p in range(keep)] + [np.zeros(4, dtype=np.uint32)] * (n - keep)
            ordered[extra] = np.array([0, 0, 1, 0], dtype=np.uint32) if extra & 1 else rng.integers(1, P, size=4, dtype=np.uint32)
            _, flag = run_last(backend, oracle, digest, ordered, log_n, log_keep, np.zeros(12, dtype=np.uint32))
            assert flag == 1, (log_n, log_keep, extra)


# ---- cm_bit_reverse ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("log_n", [1, 2, 8, 9, 16, 20])
def test_bit_reverse_against_a_numpy_permutation(backend, log_n):
    n = 1 << log_n
    idx = np.arange(n, dtype=np.uint32)
    perm = np.zeros(n, dtype=np.uint32)
    for b in range(log_n):
        perm |= ((idx >> b) & 1) << (log_n - 1 - b)
    rng = np.random.default_rng(log_n)
    for ncols in (1, 3, 17):
        cols = [rng.integers(0, 2**32, size=n, dtype=np.uint32) for _ in range(ncols)]
        hs = [backend.upload(c) for c in cols]          # distinct handles: one launch swaps every column in place
        try:
            backend.bit_reverse(hs, log_n)
            for h, c in zip(hs, cols):
                assert np.array_equal(backend.download(h, n), c[perm]), (log_n, ncols)
            backend.bit_reverse(hs, log_n)
            for h, c in zip(hs, cols):
                assert np.array_equal(backend.download(h, n), c), "applied twice: the input"
        finally:
            for h in hs:
                backend.col_free(h)
