"""ctypes binding of libcairom_hip.so (C ABI in include/cairom_hip.h).

Mirrors, op by op, the Stwo backend-trait calls the reference prover makes
(/root/reference/crates/prover/src/prover.rs:56-131): twiddles, interpolate, evaluate,
eval_at_point, Merkle commit, grind, and the whole-segment ``prove``.
"""
import ctypes as C
import os
import numpy as np

# CAIROM_HIP_LIB: development override (A/B timing of two builds inside one GPU session); the shipped path is in-tree
LIB_PATH = os.environ.get("CAIROM_HIP_LIB") or os.path.join(os.path.dirname(os.path.abspath(__file__)), "libcairom_hip.so")
_u32p = C.POINTER(C.c_uint32)
_u64p = C.POINTER(C.c_uint64)


class CmError(RuntimeError):
    pass


def load_library(path=LIB_PATH):
    if not os.path.exists(path):
        raise CmError(f"{path} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                      "(no CPU fallback exists)")
    return C.CDLL(path)


def _p(a):
    return a.ctypes.data_as(_u32p)


def fft_plan(log_n, lib=None):
    """cm_fft_plan: the passes of a 2^log_n transform as (lo, hi, tile_log, M) tuples in layer order (tile_log 0 = the generic
    kernel).  Host code: needs no GPU."""
    L = lib or load_library()
    out = ((C.c_uint32 * 4) * 8)()
    n = C.c_uint32(0)
    rc = L.cm_fft_plan(C.c_uint32(log_n), out, C.byref(n))
    if rc != 0:
        raise _lib_error(L, rc)
    return [tuple(out[i]) for i in range(n.value)]


def fft_extend_fused(log_n, lib=None):
    """cm_fft_extend_fused: whether cm_interpolate_extend takes the fused sweep at 2^log_n rows.  Host code: needs no GPU."""
    L = lib or load_library()
    f = C.c_uint32(0)
    rc = L.cm_fft_extend_fused(C.c_uint32(log_n), C.byref(f))
    if rc != 0:
        raise _lib_error(L, rc)
    return bool(f.value)


MERKLE_PLAN_WORDS = 26
MERKLE_KINDS = ("layer", "narrow", "quad", "multi", "top", "tail")


def merkle_plan(col_logs, lib=None):
    """cm_merkle_plan: the launches of cm_merkle_commit for columns of these log sizes (commitment order), in launch order.  One
    dict per launch: kind (a MERKLE_KINDS name), hi, lo, has_prev, ncols (columns of layer hi, hi - 1, .., lo), wide (the layers
    that stream their columns through LDS, descending), first_col, and for "narrow" prev / nc / npw.  Host code: needs no GPU."""
    L = lib or load_library()
    logs = np.ascontiguousarray(col_logs, dtype=np.uint32)
    out = ((C.c_uint32 * MERKLE_PLAN_WORDS) * 33)()
    n = C.c_uint32(0)
    rc = L.cm_merkle_plan(_p(logs), C.c_uint32(logs.size), out, C.c_uint32(33), C.byref(n))
    if rc != 0:
        raise _lib_error(L, rc)
    plan = []
    for i in range(n.value):
        w = list(out[i])
        hi, lo = w[1], w[2]
        rec = {"kind": MERKLE_KINDS[w[0]], "hi": hi, "lo": lo, "has_prev": bool(w[3]), "ncols": w[9:9 + hi - lo + 1],
               "wide": [l for l in range(hi, -1, -1) if w[7] >> l & 1], "first_col": w[8]}
        if rec["kind"] == "narrow":
            rec.update(prev=bool(w[4]), nc=w[5], npw=w[6])
        plan.append(rec)
    return plan


def merkle_layer_npw(log_size, has_prev, n_cols, lib=None):
    """cm_merkle_layer_npw: what cm_merkle_commit_layer launches for such a layer: 0 = k_merkle_layer, else the chunks per wave
    of k_merkle_narrow.  Host code: needs no GPU."""
    L = lib or load_library()
    npw = C.c_uint32(0)
    rc = L.cm_merkle_layer_npw(C.c_uint32(log_size), C.c_uint32(1 if has_prev else 0), C.c_uint32(n_cols), C.byref(npw))
    if rc != 0:
        raise _lib_error(L, rc)
    return npw.value


TAIL_HASH_W, TAIL_HASH_F, TAIL_COORDS_W, TAIL_ROWS_U = 0, 1, 2, 3   # cm_tail_piece.kind
TAIL_HDR_WORDS, TAIL_SHIFTS, TAIL_NO_NONCE = 16, 32, 1
TAIL_MISS = (1 << 64) - 1                                           # the nonce cell of a proof of work that found nothing


class TailPiece(C.Structure):
    """cm_tail_piece"""
    _fields_ = [("kind", C.c_uint32), ("k", C.c_uint32), ("width", C.c_uint32), ("reserved", C.c_uint32), ("cols", C.POINTER(C.c_uint64))]


class TailTablesOut(C.Structure):
    """cm_tail_tables_out"""
    _fields_ = [("struct_size", C.c_uint32), ("reserved", C.c_uint32), ("hdr", _u32p), ("positions", _u32p), ("tab", _u32p),
                ("offsets", _u32p), ("words", _u32p), ("words_cap", C.c_uint64)]


EVAL_MAX_JOBS, EVAL_GUARD_WORDS, EVAL_GUARD = 64, 4, 0xA5A5A5A5     # cm_eval_at_points_op


FOLD_CIRCLE, FOLD_ACCUMULATE, FOLD_ALPHA_ON_DEVICE = 1, 2, 4     # cm_fri_fold_rows_op flags
# cm_accumulate_quotients_rows_op: the kernel family launch_quotients chose
QUOT_PATHS = {1: "rows2", 2: "rows4", 3: "rows2-leaf", 4: "one-row", 5: "slices8", 6: "slices64"}


class SampleBatches(C.Structure):
    """cm_sample_batches"""
    _fields_ = [("n_batches", C.c_uint32), ("points", C.c_void_p), ("batch_off", C.c_void_p), ("col_index", C.c_void_p),
                ("values", C.c_void_p)]


class EvalJob(C.Structure):
    """cm_eval_job"""
    _fields_ = [("log_n", C.c_uint32), ("n_cols", C.c_uint32), ("coeffs", C.POINTER(C.c_uint64)), ("point", C.c_uint32 * 8),
                ("has_shift", C.c_uint32), ("shift_x", C.c_uint32), ("shift_y", C.c_uint32), ("reserved", C.c_uint32)]


def _digest_words(digest):
    return np.frombuffer(bytes(digest), dtype="<u4").astype(np.uint32)


class Backend:
    """Host-side handle on the HIP backend.  One instance per process / GPU."""

    def __init__(self, device=0, path=LIB_PATH):
        self.L = load_library(path)
        self.L.cm_last_error.restype = C.c_int32
        self._ck(self.L.cm_init(C.c_int32(device)))

    # -- plumbing ------------------------------------------------------------------------
    def _ck(self, rc):
        if rc != 0:
            buf = C.create_string_buffer(1024)
            self.L.cm_last_error(buf, C.c_size_t(1024))
            raise CmError(f"libcairom_hip status {rc}: {buf.value.decode(errors='replace')}")

    def col_alloc(self, n):
        h = C.c_uint64(0)
        self._ck(self.L.cm_col_alloc(C.c_uint64(n), C.byref(h)))
        return h.value

    def col_free(self, h):
        self._ck(self.L.cm_col_free(C.c_uint64(h)))

    def upload(self, arr):
        arr = np.ascontiguousarray(arr, dtype=np.uint32)
        h = self.col_alloc(arr.size)
        self._ck(self.L.cm_col_h2d(C.c_uint64(h), _p(arr), C.c_uint64(arr.size), C.c_uint64(0)))
        return h

    def download(self, h, n):
        out = np.empty(n, dtype=np.uint32)
        self._ck(self.L.cm_col_d2h(C.c_uint64(h), _p(out), C.c_uint64(n), C.c_uint64(0)))
        return out

    def col_read(self, h, offset, n):
        out = np.empty(n, dtype=np.uint32)
        self._ck(self.L.cm_col_read(C.c_uint64(h), C.c_uint64(offset), _p(out), C.c_uint64(n), C.c_uint64(0)))
        return out

    def col_write(self, h, offset, arr):
        arr = np.ascontiguousarray(arr, dtype=np.uint32)
        self._ck(self.L.cm_col_write(C.c_uint64(h), C.c_uint64(offset), _p(arr), C.c_uint64(arr.size), C.c_uint64(0)))

    def col_copy(self, dst, src, n):
        self._ck(self.L.cm_col_copy(C.c_uint64(dst), C.c_uint64(src), C.c_uint64(n), C.c_uint64(0)))

    @staticmethod
    def _harr(hs):
        return (C.c_uint64 * len(hs))(*hs)

    # -- PolyOps ----------------------------------------------------------------------------
    def twiddles(self, log_size):
        h = C.c_uint64(0)
        self._ck(self.L.cm_twiddles_precompute(C.c_uint32(log_size), C.byref(h)))
        return h.value

    def twiddles_free(self, tw):
        self._ck(self.L.cm_twiddles_free(C.c_uint64(tw)))

    def interpolate(self, cols, log_n, tw):
        self._ck(self.L.cm_interpolate(self._harr(cols), C.c_uint32(len(cols)), C.c_uint32(log_n), C.c_uint64(tw),
                                       C.c_uint64(0)))

    def evaluate(self, coeffs, log_n, log_out, tw, out):
        self._ck(self.L.cm_evaluate(self._harr(coeffs), C.c_uint32(len(coeffs)), C.c_uint32(log_n),
                                    C.c_uint32(log_out), C.c_uint64(tw), self._harr(out), C.c_uint64(0)))

    def interpolate_extend(self, evals, coeffs, lde, log_n, tw):
        """extend_evals at blowup 1: evals -> coeffs (2^log_n) and lde (2^(log_n + 1)); evals may be the coeffs handles"""
        self._ck(self.L.cm_interpolate_extend(self._harr(evals), self._harr(coeffs), self._harr(lde), C.c_uint32(len(evals)),
                                              C.c_uint32(log_n), C.c_uint64(tw), C.c_uint64(0)))

    def bit_reverse(self, cols, log_n):
        """ColumnOps::bit_reverse_column in place on every column of `cols` (2^log_n words each).  One launch swaps all columns at
        once, so the same handle must not appear twice: its swaps would race with each other."""
        self._ck(self.L.cm_bit_reverse(self._harr(cols), C.c_uint32(len(cols)), C.c_uint32(log_n), C.c_uint64(0)))

    def eval_at_point(self, coeffs, log_n, pt_xy):
        pt = np.ascontiguousarray(pt_xy, dtype=np.uint32)
        out = np.empty(4 * len(coeffs), dtype=np.uint32)
        self._ck(self.L.cm_eval_at_point(self._harr(coeffs), C.c_uint32(len(coeffs)), C.c_uint32(log_n), _p(pt),
                                         _p(out), C.c_uint64(0)))
        return out.reshape(-1, 4)

    # -- MerkleOps / GrindOps ---------------------------------------------------------------
    def merkle_commit(self, cols, col_logs):
        logs = np.ascontiguousarray(col_logs, dtype=np.uint32)
        root = (C.c_uint8 * 32)()
        self._ck(self.L.cm_merkle_commit(self._harr(cols), _p(logs), C.c_uint32(len(cols)), root, C.c_uint64(0)))
        return bytes(root)

    def merkle_commit_layers(self, cols, col_logs):
        """cm_merkle_commit_layers: (root, layers) with every stored layer largest first, 8 words per node — the layout of the
        oracle's merkle_commit."""
        logs = np.ascontiguousarray(col_logs, dtype=np.uint32)
        root = (C.c_uint8 * 32)()
        layers = np.zeros(((2 << (int(logs.max()) if logs.size else 0)) - 1) * 8, dtype=np.uint32)
        self._ck(self.L.cm_merkle_commit_layers(self._harr(cols), _p(logs), C.c_uint32(len(cols)), root, _p(layers),
                                                C.c_uint64(layers.size), C.c_uint64(0)))
        return bytes(root), layers

    def merkle_commit_layer(self, log_size, prev, cols, out):
        self._ck(self.L.cm_merkle_commit_layer(C.c_uint32(log_size), C.c_uint64(prev), self._harr(cols),
                                               C.c_uint32(len(cols)), C.c_uint64(out), C.c_uint64(0)))

    def grind(self, digest, bits):
        d = (C.c_uint8 * 32)(*digest)
        nonce = C.c_uint64(0)
        self._ck(self.L.cm_grind(d, C.c_uint32(bits), C.byref(nonce), C.c_uint64(0)))
        return nonce.value

    # -- the device-side proof tail, kernel by kernel (cm_tail_*_op) ---------------------------
    def tail_grind(self, digest, bits):
        """cm_tail_grind_op: k_tail_grind on `digest` (32 bytes); the nonce cell afterwards, TAIL_MISS (~0) = no nonce within the
        search limit (or the "tail_grind_cap" tuning)."""
        nonce = C.c_uint64(0)
        self._ck(self.L.cm_tail_grind_op(_p(_digest_words(digest)), C.c_uint32(bits), C.byref(nonce), C.c_uint64(0)))
        return nonce.value

    def tail_tables(self, digest, nonce, n_queries, nq_pad, log_domain, qmask, pieces=(), n_small=None):
        """cm_tail_tables_op: k_tail_tables + k_tail_gather.  pieces: (kind, k, handles) in output order (TAIL_HASH_W / TAIL_HASH_F:
        one handle; TAIL_COORDS_W: four; TAIL_ROWS_U: one per word of a row); n_small defaults to the number of leading pieces that
        are not row pieces.  Returns a dict: hdr (16 words), positions (the n_unique sorted positions), cnt (3 x 32: U, W, F),
        U / W / F (one array per shift k <= log_domain), offsets (per piece), words (the gathered stream)."""
        pieces = list(pieces)
        if n_small is None:
            n_small = next((i for i, p in enumerate(pieces) if p[0] == TAIL_ROWS_U), len(pieces))
        keep, arr = [], (TailPiece * max(len(pieces), 1))()
        bound = 0
        for i, (kind, k, handles) in enumerate(pieces):
            hs = self._harr(list(handles))
            keep.append(hs)
            arr[i].kind, arr[i].k, arr[i].width, arr[i].cols = kind, k, len(handles), C.cast(hs, C.POINTER(C.c_uint64))
            items = min(n_queries, 1 << max(log_domain - k, 0))
            bound += items * {TAIL_HASH_W: 8, TAIL_HASH_F: 24, TAIL_COORDS_W: 4}.get(kind, len(handles))
        self.L.cm_tail_tab_words.restype = C.c_uint64
        hdr = np.zeros(TAIL_HDR_WORDS, dtype=np.uint32)
        pos = np.zeros(max(nq_pad, 1), dtype=np.uint32)
        tab = np.zeros(int(self.L.cm_tail_tab_words(C.c_uint32(min(max(nq_pad, 1), 1024)))), dtype=np.uint32)
        off = np.zeros(max(len(pieces), 1), dtype=np.uint32)
        words = np.zeros(max(bound, 1), dtype=np.uint32)
        out = TailTablesOut(C.sizeof(TailTablesOut), 0, _p(hdr), _p(pos), _p(tab), _p(off), _p(words), bound)
        self._ck(self.L.cm_tail_tables_op(_p(_digest_words(digest)), C.c_uint64(nonce), C.c_uint32(n_queries), C.c_uint32(nq_pad),
                                          C.c_uint32(log_domain), C.c_uint32(qmask), arr, C.c_uint32(len(pieces)), C.c_uint32(n_small),
                                          C.byref(out), C.c_uint64(0)))
        cnt = tab[:3 * TAIL_SHIFTS].reshape(3, TAIL_SHIFTS).copy()
        base = 3 * TAIL_SHIFTS
        lists = {}
        for which, name, per in ((0, "U", 1), (1, "W", 1), (2, "F", 4)):
            lists[name] = [tab[base + k * per * nq_pad: base + k * per * nq_pad + int(cnt[which][k])].copy() for k in range(log_domain + 1)]
            base += TAIL_SHIFTS * per * nq_pad
        return dict(hdr=hdr, positions=pos[:int(hdr[3])].copy() if hdr[0] == 0 else pos[:0], cnt=cnt, offsets=off[:len(pieces)],
                    words=words[:int(hdr[4])].copy(), **lists)

    def tail_last(self, digest, last4, log_n, log_keep, ar=()):
        """cm_tail_last_op: k_tail_last on the four coordinate columns last4 (2^log_n words each).  Returns (digest after mix_felts
        as 32 bytes, degree flag, the 4 x 2^log_n words handed to the host, the copy of `ar`, the nonce cell)."""
        ar = np.ascontiguousarray(ar, dtype=np.uint32)
        dig = np.zeros(8, dtype=np.uint32)
        flag, cell = C.c_uint32(0), C.c_uint64(0)
        last_out = np.zeros(4 << log_n, dtype=np.uint32)
        ar_out = np.zeros(max(ar.size, 1), dtype=np.uint32)
        self._ck(self.L.cm_tail_last_op(_p(_digest_words(digest)), self._harr(last4), C.c_uint32(log_n), C.c_uint32(log_keep), _p(ar),
                                        C.c_uint32(ar.size), _p(dig), C.byref(flag), _p(last_out), _p(ar_out), C.byref(cell), C.c_uint64(0)))
        return dig.tobytes(), flag.value, last_out.reshape(4, -1), ar_out[:ar.size], cell.value

    # -- the provers' out-of-domain sampling on chosen inputs (cm_eval_at_points_op) ------------
    def eval_at_points(self, jobs, t=None, landing=False):
        """cm_eval_at_points_op: eval_at_point_multi on `jobs`, each a dict with log_n, coeffs (handles) and either point (8 words, x
        then y: the host-point form, t None) or optionally shift (the M31 point (x, y) added to the point of the felt `t`: the
        device-point form).  Returns a dict: values (per job, n_cols x 4 words from device memory), guards (per job, the
        EVAL_GUARD_WORDS words behind its slice), and with landing=True land_values / land_guards (the pinned landing buffer, laid
        out the same way)."""
        jobs = list(jobs)
        arr, keep = (EvalJob * max(len(jobs), 1))(), []
        for i, j in enumerate(jobs):
            hs = self._harr(list(j["coeffs"]))
            keep.append(hs)
            arr[i].log_n, arr[i].n_cols, arr[i].coeffs = j["log_n"], len(j["coeffs"]), C.cast(hs, C.POINTER(C.c_uint64))
            arr[i].point = (C.c_uint32 * 8)(*[int(w) for w in j.get("point", (0,) * 8)])
            if j.get("shift") is not None:
                arr[i].has_shift, arr[i].shift_x, arr[i].shift_y = 1, int(j["shift"][0]), int(j["shift"][1])
        words = sum(4 * len(j["coeffs"]) + EVAL_GUARD_WORDS for j in jobs)
        out = np.zeros(max(words, 1), dtype=np.uint32)
        land = np.zeros(max(words, 1), dtype=np.uint32)
        t4 = None if t is None else np.ascontiguousarray(t, dtype=np.uint32)
        self._ck(self.L.cm_eval_at_points_op(arr, C.c_uint32(len(jobs)), None if t4 is None else _p(t4), C.c_uint32(1 if landing else 0),
                                             _p(out), _p(land) if landing else None, C.c_uint64(0)))

        def split(buf):
            vals, guards, off = [], [], 0
            for j in jobs:
                n = 4 * len(j["coeffs"])
                vals.append(buf[off:off + n].reshape(-1, 4).copy())
                guards.append(buf[off + n:off + n + EVAL_GUARD_WORDS].copy())
                off += n + EVAL_GUARD_WORDS
            return vals, guards
        res = dict(zip(("values", "guards"), split(out)))
        if landing:
            res.update(zip(("land_values", "land_guards"), split(land)))
        return res

    # -- FieldOps / FriOps / QuotientOps ----------------------------------------------------
    def batch_inverse_m31(self, src, dst, n):
        self._ck(self.L.cm_batch_inverse_m31(C.c_uint64(src), C.c_uint64(dst), C.c_uint64(n), C.c_uint64(0)))

    def batch_inverse_qm31(self, src4, dst4, n):
        self._ck(self.L.cm_batch_inverse_qm31(self._harr(src4), self._harr(dst4), C.c_uint64(n), C.c_uint64(0)))

    def fri_fold_circle_into_line(self, dst4, src4, alpha, log_n, tw):
        a = np.ascontiguousarray(alpha, dtype=np.uint32)
        self._ck(self.L.cm_fri_fold_circle_into_line(self._harr(dst4), self._harr(src4), _p(a), C.c_uint32(log_n),
                                                     C.c_uint64(tw), C.c_uint64(0)))

    def fri_fold_line(self, src4, alpha, log_n, tw, out4):
        a = np.ascontiguousarray(alpha, dtype=np.uint32)
        self._ck(self.L.cm_fri_fold_line(self._harr(src4), _p(a), C.c_uint32(log_n), C.c_uint64(tw),
                                         self._harr(out4), C.c_uint64(0)))

    def fri_fold_line_leaves(self, src4, alpha, log_n, tw, out4, leaf_hashes, circle4=None, alpha_circle=None):
        """A FRI layer (fold_line of src4, fold_circle of circle4 accumulated in; either may be None) and the leaf hashes of the
        folded layer in one pass."""
        a = None if alpha is None else np.ascontiguousarray(alpha, dtype=np.uint32)
        ac = None if alpha_circle is None else np.ascontiguousarray(alpha_circle, dtype=np.uint32)
        self._ck(self.L.cm_fri_fold_line_leaves(None if src4 is None else self._harr(src4), None if circle4 is None else self._harr(circle4),
                                                None if a is None else _p(a), None if ac is None else _p(ac), C.c_uint32(log_n),
                                                C.c_uint64(tw), self._harr(out4), C.c_uint64(leaf_hashes), C.c_uint64(0)))

    def accumulate_quotients(self, log_size, cols, points, batch_off, col_index, values, coeff, out4, tw):
        """points: (n_batches, 8) u32; batch_off: n_batches+1; col_index: entries; values: (entries, 4)."""
        class Batches(C.Structure):
            _fields_ = [("n_batches", C.c_uint32), ("points", C.c_void_p), ("batch_off", C.c_void_p),
                        ("col_index", C.c_void_p), ("values", C.c_void_p)]
        pts = np.ascontiguousarray(points, dtype=np.uint32)
        off = np.ascontiguousarray(batch_off, dtype=np.uint32)
        ci = np.ascontiguousarray(col_index, dtype=np.uint32)
        vals = np.ascontiguousarray(values, dtype=np.uint32)
        co = np.ascontiguousarray(coeff, dtype=np.uint32)
        b = Batches(len(off) - 1, pts.ctypes.data, off.ctypes.data, ci.ctypes.data, vals.ctypes.data)
        self._ck(self.L.cm_accumulate_quotients(C.c_uint32(log_size), self._harr(cols), C.c_uint32(len(cols)), C.byref(b),
                                                _p(co), self._harr(out4), C.c_uint64(tw), C.c_uint64(0)))

    # -- row-range and prover-only forms, the sharded prover's data movement (cm_*_rows_op, shard_ops.hip) --------------
    def fri_fold_rows(self, out4, src4, alpha, log_n, tw, i0, n_out, circle=False, accumulate=False, alpha_on_device=False):
        """cm_fri_fold_rows_op: outputs [i0, i0 + n_out) of fold_line (circle: fold_circle_into_line) of 2^log_n values; src4 holds
        source rows [2 i0, 2 (i0 + n_out)), out4 the outputs."""
        a = np.ascontiguousarray(alpha, dtype=np.uint32)
        flags = (FOLD_CIRCLE if circle else 0) | (FOLD_ACCUMULATE if accumulate else 0) | (FOLD_ALPHA_ON_DEVICE if alpha_on_device else 0)
        self._ck(self.L.cm_fri_fold_rows_op(self._harr(out4), self._harr(src4), _p(a), C.c_uint32(log_n), C.c_uint64(tw), C.c_uint32(i0),
                                            C.c_uint32(n_out), C.c_uint32(flags), C.c_uint64(0)))

    def fri_fold_leaves_rows(self, src4, alpha, log_n, tw, row0, n_rows, out4, leaf_hashes, circle4=None, alpha_circle=None):
        """cm_fri_fold_leaves_rows_op: fri_fold_line_leaves on outputs [row0, row0 + n_rows).  Returns `fused` (1: k_fold_leaf ran)."""
        a = None if alpha is None else np.ascontiguousarray(alpha, dtype=np.uint32)
        ac = None if alpha_circle is None else np.ascontiguousarray(alpha_circle, dtype=np.uint32)
        fused = C.c_uint32(0xFFFFFFFF)
        self._ck(self.L.cm_fri_fold_leaves_rows_op(None if src4 is None else self._harr(src4), None if circle4 is None else self._harr(circle4),
                                                   None if a is None else _p(a), None if ac is None else _p(ac), C.c_uint32(log_n),
                                                   C.c_uint64(tw), C.c_uint32(row0), C.c_uint32(n_rows), self._harr(out4),
                                                   C.c_uint64(leaf_hashes), C.byref(fused), C.c_uint64(0)))
        return fused.value

    def accumulate_quotients_rows(self, log_size, cols, points, batch_off, col_index, values, coeff, out4, tw, row0=0, n_rows=0,
                                  leaf_hashes=0, sample_idx=None):
        """cm_accumulate_quotients_rows_op on rows [row0, row0 + n_rows) (n_rows 0: the whole domain); cols / out4 hold that range.
        sample_idx None: `values` is (entries, 4) and the coefficients are computed on the host; returns the path name.
        sample_idx given: `values` is (n_samples, 4), k_quotient_coeffs computes the coefficients on the device; returns
        (path name, coef_c (entries, 4), sum_a, sum_b, batch_coeff (n_batches, 4 each))."""
        pts = np.ascontiguousarray(points, dtype=np.uint32)
        off = np.ascontiguousarray(batch_off, dtype=np.uint32)
        ci = np.ascontiguousarray(col_index, dtype=np.uint32)
        vals = np.ascontiguousarray(values, dtype=np.uint32)
        co = np.ascontiguousarray(coeff, dtype=np.uint32)
        b = SampleBatches(len(off) - 1, pts.ctypes.data, off.ctypes.data, ci.ctypes.data, vals.ctypes.data)
        path = C.c_uint32(0)
        dev = sample_idx is not None
        si = np.ascontiguousarray(sample_idx, dtype=np.uint32) if dev else None
        cc = np.zeros((ci.size, 4), dtype=np.uint32)
        sums = np.zeros((len(off) - 1, 12), dtype=np.uint32)
        self._ck(self.L.cm_accumulate_quotients_rows_op(
            C.c_uint32(log_size), self._harr(cols), C.c_uint32(len(cols)), C.byref(b), _p(co), self._harr(out4), C.c_uint64(tw),
            C.c_uint32(row0), C.c_uint32(n_rows), C.c_uint64(leaf_hashes), C.c_uint32(1 if dev else 0), _p(si) if dev else None,
            C.c_uint32(vals.size // 4 if dev else 0), C.byref(path), _p(cc) if dev else None, _p(sums) if dev else None, C.c_uint64(0)))
        name = QUOT_PATHS[path.value]
        return (name, cc, sums[:, 0:4].copy(), sums[:, 4:8].copy(), sums[:, 8:12].copy()) if dev else name

    def pack_parity(self, src, dst, half_len, parity):
        self._ck(self.L.cm_pack_parity_op(C.c_uint64(src), C.c_uint64(dst), C.c_uint32(half_len), C.c_uint32(parity), C.c_uint64(0)))

    def halo_build(self, even_half, odd_half, even_src, odd_src, row0, length, n, trace_log, log_ranks, out):
        """cm_halo_build_op; returns the kernel's error word."""
        err = C.c_uint32(0xFFFFFFFF)
        self._ck(self.L.cm_halo_build_op(C.c_uint64(even_half), C.c_uint64(odd_half), C.c_uint32(even_src), C.c_uint32(odd_src),
                                         C.c_uint32(row0), C.c_uint32(length), C.c_uint32(n), C.c_uint32(trace_log), C.c_uint32(log_ranks),
                                         C.c_uint64(out), C.byref(err), C.c_uint64(0)))
        return err.value

    def sum_copies(self, src, n_copies, stride, words, out, modular):
        self._ck(self.L.cm_sum_copies_op(C.c_uint64(src), C.c_uint32(n_copies), C.c_uint64(stride), C.c_uint64(words), C.c_uint64(out),
                                         C.c_uint32(1 if modular else 0), C.c_uint64(0)))

    def copy_segments(self, segs):
        """cm_copy_segments_op: segs = [(src handle, dst handle, words)]."""
        n = len(segs)
        src, dst = self._harr([s[0] for s in segs] or [0]), self._harr([s[1] for s in segs] or [0])
        words = (C.c_uint64 * max(n, 1))(*([s[2] for s in segs] or [0]))
        self._ck(self.L.cm_copy_segments_op(src, dst, words, C.c_uint32(n), C.c_uint64(0)))


class HostInput:
    """ProverInput built on the host by the synthetic VM + adapter (no GPU needed)."""

    def __init__(self, lib, handle):
        self.L = lib
        self.h = handle
        self.L.cm_host_input_view.restype = C.c_void_p
        self.L.cm_host_input_steps.restype = C.c_uint64

    @property
    def view(self):
        return C.c_void_p(self.L.cm_host_input_view(self.h))

    @property
    def steps(self):
        return int(self.L.cm_host_input_steps(self.h))

    def free(self):
        if self.h:
            self.L.cm_host_input_free(self.h)
            self.h = None


def _lib_error(L, rc):
    buf = C.create_string_buffer(2048)
    L.cm_last_error(buf, C.c_size_t(2048))
    return CmError(f"libcairom_hip status {rc}: {buf.value.decode(errors='replace')}")


def synth_fibonacci(n, max_steps=1 << 30, segment=0, lib=None):
    """fibonacci_loop(n) through the synthetic VM + adapter: 10*n + 12 steps."""
    L = lib or load_library()
    h = C.c_void_p()
    rc = L.cm_synth_fibonacci(C.c_uint32(n), C.c_uint64(max_steps), C.c_uint32(segment), C.byref(h))
    if rc:
        raise _lib_error(L, rc)
    return HostInput(L, h)


def vm_run(program, entry_pc=0, args=(), n_returns=0, max_steps=1 << 30, segment=0, lib=None):
    """Run a CASM program (list of instruction word lists) and adapt one segment."""
    L = lib or load_library()
    words = np.array([w for ins in program for w in ins], dtype=np.uint32)
    lens = np.array([len(ins) for ins in program], dtype=np.uint32)
    a = np.array(list(args), dtype=np.uint32)
    h = C.c_void_p()
    nseg = C.c_uint32(0)
    rc = L.cm_vm_run(_p(words), _p(lens), C.c_uint32(len(program)), C.c_uint32(entry_pc), _p(a), C.c_uint32(len(a)),
                     C.c_uint32(n_returns), C.c_uint64(max_steps), C.c_uint32(segment), C.byref(h), C.byref(nseg))
    if rc:
        raise _lib_error(L, rc)
    hi = HostInput(L, h)
    hi.n_segments = nseg.value
    return hi


class Proof:
    PHASES = ["setup", "preprocessed", "trace_gen", "trace_commit", "interaction_gen", "interaction_commit",
              "constraints", "composition_commit", "oods_sampling", "quotients", "fri_commit", "pow", "decommit"]

    def __init__(self, lib, handle):
        self.L = lib
        self.h = handle

    def words(self):
        p = C.POINTER(C.c_uint32)()
        n = C.c_uint64(0)
        rc = self.L.cm_proof_words(self.h, C.byref(p), C.byref(n))
        if rc:
            raise _lib_error(self.L, rc)
        return np.ctypeslib.as_array(p, shape=(n.value,)).copy()

    def json(self):
        p = C.c_char_p()
        n = C.c_size_t(0)
        rc = self.L.cm_proof_json(self.h, C.byref(p), C.byref(n))
        if rc:
            raise _lib_error(self.L, rc)
        return C.string_at(p, n.value).decode()

    def commitments(self):
        roots = ((C.c_uint8 * 32) * 4)()
        self.L.cm_proof_commitments(self.h, roots)
        return [bytes(r) for r in roots]

    def stats(self):
        cells, steps = C.c_uint64(0), C.c_uint64(0)
        ph = (C.c_double * 32)()
        n = self.L.cm_proof_stats(self.h, C.byref(cells), C.byref(steps), ph, C.c_uint32(32))
        out = {"cells": cells.value, "steps": steps.value,
               "phase_ms": dict(zip(self.PHASES, [ph[i] for i in range(min(n, 32))]))}
        if hasattr(self.L, "cm_proof_memory"):      # (CAIROM_HIP_LIB may name a build older than header revision 9)
            out["memory"] = self.memory().as_dict(self.PHASES)
        return out

    def memory(self):
        """cm_proof_memory: what this proof took from the proving thread's device pool (ProofMem)."""
        m = ProofMem()
        m.struct_size = C.sizeof(ProofMem)
        rc = self.L.cm_proof_memory(self.h, C.byref(m))
        if rc:
            raise _lib_error(self.L, rc)
        return m

    def verify(self, cfg=None):
        """verify_cairo_m(proof, pcs_config) on this proof (product-side verifier, host code): (status, message).
        cfg = the PcsConfig the verifier expects, None = REGULAR_96_BITS (never taken from the proof)."""
        rc = self.L.cm_verify_proof(self.h, _cfg(cfg))
        buf = C.create_string_buffer(512)
        self.L.cm_last_error(buf, C.c_size_t(512))
        return rc, buf.value.decode(errors="replace") if rc else ""

    def public_data(self):
        """cm_proof_public_data + cm_proof_public_entries (revision 10): the registers, clock and memory roots the proof is about,
        and the public entries of the three ranges as (n, 7) arrays of (present, address, value[4], clock)."""
        d = PublicDataC()
        d.struct_size = C.sizeof(PublicDataC)
        rc = self.L.cm_proof_public_data(self.h, C.byref(d))
        if rc:
            raise _lib_error(self.L, rc)
        out = {n: getattr(d, n) for n in ("initial_pc", "initial_fp", "final_pc", "final_fp", "clock", "initial_root", "final_root")}
        for which, name in enumerate(("program", "input", "output")):
            n = C.c_uint64(0)
            rc = self.L.cm_proof_public_entries(self.h, C.c_uint32(which), None, C.c_uint64(0), C.byref(n))
            if rc:
                raise _lib_error(self.L, rc)
            a = np.zeros((n.value, 7), dtype=np.uint32)
            rc = self.L.cm_proof_public_entries(self.h, C.c_uint32(which), _p(a), C.c_uint64(n.value), C.byref(n))
            if rc:
                raise _lib_error(self.L, rc)
            out[name] = a
        return out

    def transcript(self):
        """cm_proof_transcript: the Fiat-Shamir steps of this proof (list of {"op", "digest", "n_words", "words"}); empty
        unless set_transcript_log(True) was in force when it was made."""
        import json
        p = C.c_char_p()
        n = C.c_size_t(0)
        rc = self.L.cm_proof_transcript(self.h, C.byref(p), C.byref(n))
        if rc:
            raise _lib_error(self.L, rc)
        return json.loads(C.string_at(p, n.value).decode())

    def free(self):
        if self.h:
            self.L.cm_proof_free(self.h)
            self.h = None


def set_framing(spec, lib=None):
    """cm_set_framing (process-wide; host code, works without a GPU): named switches for the Stwo-side conventions no
    reference vector settles — include/cairom_hip.h.  "" restores the defaults."""
    L = lib or load_library()
    rc = L.cm_set_framing((spec or "").encode())
    if rc:
        raise _lib_error(L, rc)


def get_framing(lib=None):
    L = lib or load_library()
    buf = C.create_string_buffer(256)
    L.cm_get_framing(buf, C.c_size_t(256))
    return buf.value.decode()


def set_transcript_log(on, lib=None):
    (lib or load_library()).cm_set_transcript_log(C.c_int32(1 if on else 0))


class ArrayInput:
    """A ProverInput given as explicit arrays (hand-built inputs such as crates/prover/tests/prover.rs:33-112, or the `input`
    object of a tests/golden/ref_*.json file): the same `.view` / `.steps` / `.free()` surface as HostInput.
    arrays: dict with regs[4], roots[2], ranges[6], bundles<k> (n x 12), data_accesses (n x 4), initial_memory / final_memory
    (n x 7: address, v0..v3, clock, multiplicity — IN THE ROW ORDER the memory component must use), clock_updates (n x 6),
    initial_tree / final_tree (n x 8) — the layout prover_input_arrays() returns."""

    def __init__(self, arrays):
        self._keep = []
        v = ProverInputView()

        def arr(name, words):
            a = np.ascontiguousarray(np.array(arrays.get(name, []), dtype=np.uint32).reshape(-1, words))
            self._keep.append(a)
            return a

        for i, x in enumerate(arrays.get("regs", [0, 0, 0, 0])):
            v.regs[i] = int(x)
        total = 0
        for i in range(N_OPCODE_COMPONENTS):
            a = arr(f"bundles{i}", 12)
            v.bundles[i] = a.ctypes.data if a.shape[0] else None
            v.n_bundles[i] = a.shape[0]
            total += a.shape[0]
        for name, words, fld in (("data_accesses", 4, "data_accesses"), ("initial_memory", 7, "initial_memory"),
                                 ("final_memory", 7, "final_memory"), ("clock_updates", 6, "clock_updates"),
                                 ("initial_tree", 8, "initial_tree"), ("final_tree", 8, "final_tree")):
            a = arr(name, words)
            setattr(v, fld, a.ctypes.data if a.shape[0] else None)
            setattr(v, "n_" + fld, a.shape[0])
        for i, x in enumerate(arrays.get("roots", [0, 0])):
            v.roots[i] = int(x)
        for i, x in enumerate(arrays.get("ranges", [0] * 6)):
            v.ranges[i] = int(x)
        self._v = v
        self.steps = total

    @property
    def view(self):
        return C.cast(C.pointer(self._v), C.c_void_p)

    def free(self):
        pass


def partial_merkle_tree(cells, initial=True, ranges=(0, 0, 0, 0, 0, 0), lib=None):
    """build_partial_merkle_tree (crates/prover/src/adapter/merkle.rs:183-295) over cells = [(address, v0, v1, v2, v3), ...]:
    (nodes n x 8, root).  Host code."""
    L = lib or load_library()
    c = np.ascontiguousarray(np.array(cells, dtype=np.uint32).reshape(-1, 5))
    cap = max(4096, 64 * c.shape[0] * 31)
    out = np.zeros((cap, 8), dtype=np.uint32)
    n, root = C.c_uint64(0), C.c_uint32(0)
    rc = L.cm_adapter_partial_tree(_p(c), C.c_uint32(c.shape[0]), C.c_int32(1 if initial else 0), (C.c_uint32 * 6)(*ranges), _p(out),
                                   C.c_uint64(cap), C.byref(n), C.byref(root))
    if rc:
        raise _lib_error(L, rc)
    return out[:n.value].copy(), root.value


def _cfg(cfg):
    if cfg is None:
        return None
    return (C.c_uint32 * 4)(*cfg)  # pow_bits, log_blowup_factor, log_last_layer_degree_bound, n_queries


def _backend_prove(self, host_input, cfg=None):
    """prove_cairo_m (crates/prover/src/prover.rs:23): upload + prove."""
    h = C.c_void_p()
    self._ck(self.L.cm_prove_segment(host_input.view, _cfg(cfg), C.byref(h)))
    return Proof(self.L, h)


def _backend_upload(self, host_input):
    h = C.c_void_p()
    self._ck(self.L.cm_input_upload(host_input.view, C.byref(h)))
    return h


def _backend_prove_device(self, dev_input, cfg=None):
    h = C.c_void_p()
    self._ck(self.L.cm_prove_device(dev_input, _cfg(cfg), C.byref(h)))
    return Proof(self.L, h)


Backend.prove = _backend_prove
Backend.upload_input = _backend_upload
Backend.prove_device = _backend_prove_device
Backend.free_input = lambda self, h: self.L.cm_input_free(h)


# ---- runner segments and the device-side adapter (include/cairom_hip.h: cm_runner_segment) -----------------
N_OPCODE_COMPONENTS = 26


class ProverInputView(C.Structure):
    """cm_prover_input (read-only mirror, used to compare adapters field by field)."""
    _fields_ = [("regs", C.c_uint32 * 4),
                ("bundles", C.c_void_p * N_OPCODE_COMPONENTS), ("n_bundles", C.c_uint64 * N_OPCODE_COMPONENTS),
                ("data_accesses", C.c_void_p), ("n_data_accesses", C.c_uint64),
                ("initial_memory", C.c_void_p), ("n_initial_memory", C.c_uint64),
                ("final_memory", C.c_void_p), ("n_final_memory", C.c_uint64),
                ("clock_updates", C.c_void_p), ("n_clock_updates", C.c_uint64),
                ("initial_tree", C.c_void_p), ("n_initial_tree", C.c_uint64),
                ("final_tree", C.c_void_p), ("n_final_tree", C.c_uint64),
                ("roots", C.c_uint32 * 2), ("ranges", C.c_uint32 * 6)]


def prover_input_arrays(view_ptr):
    """cm_prover_input* -> dict of numpy arrays / scalars (copies)."""
    v = C.cast(view_ptr, C.POINTER(ProverInputView)).contents

    def arr(ptr, n, words):
        if not n:
            return np.zeros((0, words), dtype=np.uint32)
        return np.ctypeslib.as_array(C.cast(ptr, _u32p), shape=(int(n), words)).copy()

    out = {"regs": list(v.regs), "roots": list(v.roots), "ranges": list(v.ranges)}
    for i in range(N_OPCODE_COMPONENTS):
        out[f"bundles{i}"] = arr(v.bundles[i], v.n_bundles[i], 12)
    out["data_accesses"] = arr(v.data_accesses, v.n_data_accesses, 4)
    out["initial_memory"] = arr(v.initial_memory, v.n_initial_memory, 7)
    out["final_memory"] = arr(v.final_memory, v.n_final_memory, 7)
    out["clock_updates"] = arr(v.clock_updates, v.n_clock_updates, 6)
    out["initial_tree"] = arr(v.initial_tree, v.n_initial_tree, 8)
    out["final_tree"] = arr(v.final_tree, v.n_final_tree, 8)
    return out


class RunnerSegmentView(C.Structure):
    """cm_runner_segment (read-only mirror)."""
    _fields_ = [("trace", C.c_void_p), ("n_trace", C.c_uint64), ("memory_trace", C.c_void_p), ("n_memory_trace", C.c_uint64),
                ("initial_memory", C.c_void_p), ("n_initial_memory", C.c_uint64), ("ranges", C.c_uint32 * 6),
                ("initial_heap", C.c_void_p), ("n_initial_heap", C.c_uint64)]


def runner_segment_arrays(view_ptr):
    """cm_runner_segment* -> {"trace": (n, 2) (pc, fp), "memory_trace": (n, 5), "initial_memory": (n, 4), "ranges": [6]} (copies)."""
    v = C.cast(view_ptr, C.POINTER(RunnerSegmentView)).contents

    def arr(ptr, n, words):
        if not n:
            return np.zeros((0, words), dtype=np.uint32)
        return np.ctypeslib.as_array(C.cast(ptr, _u32p), shape=(int(n), words)).copy()
    return {"trace": arr(v.trace, v.n_trace, 2), "memory_trace": arr(v.memory_trace, v.n_memory_trace, 5),
            "initial_memory": arr(v.initial_memory, v.n_initial_memory, 4), "ranges": list(v.ranges),
            "initial_heap": arr(v.initial_heap, v.n_initial_heap, 4)}   # index i = the cell at 2^28 - 1 - i


class HostSegment:
    """Raw output of the synthetic VM for one segment (trace, memory log, memory at segment start)."""

    def __init__(self, lib, handle):
        self.L = lib
        self.h = handle
        self.L.cm_host_segment_view.restype = C.c_void_p

    @property
    def view(self):
        return C.c_void_p(self.L.cm_host_segment_view(self.h))

    def free(self):
        if self.h:
            self.L.cm_host_segment_free(self.h)
            self.h = None


def synth_fibonacci_segment(n, max_steps=1 << 30, segment=0, lib=None):
    L = lib or load_library()
    h = C.c_void_p()
    rc = L.cm_synth_fibonacci_segment(C.c_uint32(n), C.c_uint64(max_steps), C.c_uint32(segment), C.byref(h))
    if rc:
        raise _lib_error(L, rc)
    return HostSegment(L, h)


def vm_segment(program, entry_pc=0, args=(), n_returns=0, max_steps=1 << 30, segment=0, lib=None):
    L = lib or load_library()
    words = np.array([w for ins in program for w in ins], dtype=np.uint32)
    lens = np.array([len(ins) for ins in program], dtype=np.uint32)
    a = np.array(list(args), dtype=np.uint32)
    h = C.c_void_p()
    nseg = C.c_uint32(0)
    rc = L.cm_vm_segment(_p(words), _p(lens), C.c_uint32(len(program)), C.c_uint32(entry_pc), _p(a), C.c_uint32(len(a)),
                         C.c_uint32(n_returns), C.c_uint64(max_steps), C.c_uint32(segment), C.byref(h), C.byref(nseg))
    if rc:
        raise _lib_error(L, rc)
    hs = HostSegment(L, h)
    hs.n_segments = nseg.value
    return hs


class ArraySegment:
    """A cm_runner_segment over caller-supplied arrays (hand-built segments: tests/adapter_segments.py): the `.view` / `.free()`
    surface of HostSegment.  trace (n + 1, 2) (pc, fp); memory_trace (m, 5); initial_memory (k, 4); initial_heap (h, 4), index i =
    the cell at 2^28 - 1 - i; ranges = program, input, output [start, end)."""

    def __init__(self, trace, memory_trace, initial_memory, initial_heap=(), ranges=(0, 0, 0, 0, 0, 0)):
        f = lambda a, w: np.ascontiguousarray(np.asarray(a, dtype=np.uint32).reshape(-1, w))
        self.trace, self.memory_trace = f(trace, 2), f(memory_trace, 5)
        self.initial_memory, self.initial_heap = f(initial_memory, 4), f(initial_heap, 4)
        self.ranges = [int(x) for x in ranges]
        ptr = lambda a: a.ctypes.data if a.shape[0] else None
        self._v = RunnerSegmentView(ptr(self.trace), self.trace.shape[0], ptr(self.memory_trace), self.memory_trace.shape[0],
                                    ptr(self.initial_memory), self.initial_memory.shape[0], (C.c_uint32 * 6)(*self.ranges),
                                    ptr(self.initial_heap), self.initial_heap.shape[0])

    @property
    def view(self):
        return C.cast(C.pointer(self._v), C.c_void_p)

    def run_segment(self, n_memory_end, n_heap_end):
        """the cm_run_segment of this segment's trace and log (this object must outlive it)"""
        return RunSegmentC(self._v.trace, self._v.n_trace, self._v.memory_trace, self._v.n_memory_trace, int(n_memory_end), int(n_heap_end))

    def free(self):
        pass


def adapt_segment_host(segment, lib=None):
    """cm_adapt_segment_host: the host adapter (import_segment, what cm_vm_run runs) over a HostSegment / ArraySegment.  No GPU."""
    L = lib or load_library()
    h = C.c_void_p()
    rc = L.cm_adapt_segment_host(segment.view, C.byref(h))
    if rc:
        raise _lib_error(L, rc)
    return HostInput(L, h)


def _backend_public_entries(self, dev_input):
    """cm_device_input_public_entries: {"program" | "input" | "output": (n, 7) present, address, value[4], clock} as the device
    input holds them (what its proof will carry)."""
    out = {}
    for which, name in enumerate(("program", "input", "output")):
        n = C.c_uint64(0)
        self._ck(self.L.cm_device_input_public_entries(dev_input, C.c_uint32(which), None, C.c_uint64(0), C.byref(n)))
        a = np.zeros((n.value, 7), dtype=np.uint32)
        self._ck(self.L.cm_device_input_public_entries(dev_input, C.c_uint32(which), _p(a), C.c_uint64(n.value), C.byref(n)))
        out[name] = a
    return out


def _backend_adapt_segment(self, host_segment):
    """import_from_runner_output on the GPU: runner segment -> device-resident ProverInput."""
    h = C.c_void_p()
    self._ck(self.L.cm_adapt_segment_device(host_segment.view, C.byref(h)))
    return h


def _backend_download_input(self, dev_input):
    h = C.c_void_p()
    self._ck(self.L.cm_device_input_download(dev_input, C.byref(h)))
    return HostInput(self.L, h)


Backend.adapt_segment = _backend_adapt_segment
Backend.download_input = _backend_download_input
Backend.public_entries = _backend_public_entries


def _backend_prove_many(self, dev_inputs, inflight=3, cfg=None):
    """Segment pipeline (cm_prove_many): independent segment proofs, up to `inflight` on the GPU at once."""
    n = len(dev_inputs)
    ins = (C.c_void_p * n)(*[d.value if isinstance(d, C.c_void_p) else d for d in dev_inputs])
    outs = (C.c_void_p * n)()
    rc = self.L.cm_prove_many(ins, C.c_uint32(n), _cfg(cfg), C.c_uint32(inflight), outs)
    proofs = [Proof(self.L, C.c_void_p(outs[i])) if outs[i] else None for i in range(n)]
    if rc != 0:
        try:
            self._ck(rc)                       # raises CmError with the first failure's message
        except CmError as e:
            e.partial = proofs                 # the proofs that were built (None where a segment failed): caller frees them
            raise
    return proofs


Backend.prove_many = _backend_prove_many


def _prove_streamed(self, fn, views, inflight, cfg):
    n = len(views)
    ins = (C.c_void_p * n)(*[C.cast(v, C.c_void_p).value for v in views])
    outs = (C.c_void_p * n)()
    rc = fn(ins, C.c_uint32(n), _cfg(cfg), C.c_uint32(inflight), outs)
    proofs = [Proof(self.L, C.c_void_p(outs[i])) if outs[i] else None for i in range(n)]
    if rc != 0:
        try:
            self._ck(rc)
        except CmError as e:
            e.partial = proofs
            raise
    return proofs


def _backend_prove_many_host(self, host_inputs, inflight=3, cfg=None):
    """Streaming ingest (cm_prove_many_host): HOST ProverInputs; input i + 1 uploads while up to `inflight` proofs run."""
    return _prove_streamed(self, self.L.cm_prove_many_host, [h.view for h in host_inputs], inflight, cfg)


def _backend_prove_many_segments(self, host_segments, inflight=3, cfg=None):
    """Streaming ingest from runner segments (cm_prove_many_segments): segment i + 1 goes through the device adapter while up to
    `inflight` proofs run."""
    return _prove_streamed(self, self.L.cm_prove_many_segments, [h.view for h in host_segments], inflight, cfg)


Backend.prove_many_host = _backend_prove_many_host
Backend.prove_many_segments = _backend_prove_many_segments


def _backend_set_preprocessed_cache(self, on):
    """cm_set_preprocessed_cache: keep the committed preprocessed tree (tree 0) between proofs; off by default."""
    self._ck(self.L.cm_set_preprocessed_cache(C.c_int32(1 if on else 0)))


Backend.set_preprocessed_cache = _backend_set_preprocessed_cache
Backend.set_twiddle_cache = lambda self, on: self._ck(self.L.cm_set_twiddle_cache(C.c_int32(1 if on else 0)))
Backend.set_device_tail = lambda self, on: self._ck(self.L.cm_set_device_tail(C.c_int32(1 if on else 0)))
Backend.pool_trim = lambda self: self._ck(self.L.cm_pool_trim())   # this thread's cached device blocks back to the driver


def _backend_mem_info(self):
    """cm_device_mem_info: (free, total) bytes of the library device's HBM."""
    f, t = C.c_uint64(0), C.c_uint64(0)
    self._ck(self.L.cm_device_mem_info(C.byref(f), C.byref(t)))
    return f.value, t.value


Backend.mem_info = _backend_mem_info


# ---- a whole run (include/cairom_hip.h, revision 10): memory carried on the device, chained segment proofs ------
class PublicDataC(C.Structure):
    """cm_public_data"""
    _fields_ = [("struct_size", C.c_uint32), ("reserved0", C.c_uint32),
                ("initial_pc", C.c_uint32), ("initial_fp", C.c_uint32), ("final_pc", C.c_uint32), ("final_fp", C.c_uint32),
                ("clock", C.c_uint32), ("initial_root", C.c_uint32), ("final_root", C.c_uint32),
                ("n_program", C.c_uint32), ("n_input", C.c_uint32), ("n_output", C.c_uint32)]


class RunSegmentC(C.Structure):
    """cm_run_segment"""
    _fields_ = [("trace", C.c_void_p), ("n_trace", C.c_uint64), ("memory_trace", C.c_void_p), ("n_memory_trace", C.c_uint64),
                ("n_memory_end", C.c_uint64), ("n_heap_end", C.c_uint64)]


def segment_end_lengths(host_segment):
    """cm_host_segment_end_lengths: cells in the synthetic VM's locals / heap vectors when the segment ended."""
    a, b = C.c_uint64(0), C.c_uint64(0)
    rc = host_segment.L.cm_host_segment_end_lengths(host_segment.h, C.byref(a), C.byref(b))
    if rc:
        raise _lib_error(host_segment.L, rc)
    return a.value, b.value


def run_segment(host_segment, n_memory_end=None, n_heap_end=None):
    """cm_run_segment over a HostSegment's trace and log (the HostSegment must outlive it); the end lengths default to the
    synthetic VM's own."""
    v = C.cast(host_segment.view, C.POINTER(RunnerSegmentView)).contents
    ends = segment_end_lengths(host_segment)
    return RunSegmentC(v.trace, v.n_trace, v.memory_trace, v.n_memory_trace,
                       ends[0] if n_memory_end is None else n_memory_end, ends[1] if n_heap_end is None else n_heap_end)


class Run:
    """cm_run: a program's memory kept on the device from segment to segment."""

    def __init__(self, backend, initial_memory, initial_heap, ranges):
        self.B, self.L = backend, backend.L
        lo = np.ascontiguousarray(initial_memory, dtype=np.uint32).reshape(-1, 4)
        hi = np.ascontiguousarray(initial_heap, dtype=np.uint32).reshape(-1, 4)
        h = C.c_void_p()
        backend._ck(self.L.cm_run_begin(_p(lo), C.c_uint64(lo.shape[0]), _p(hi), C.c_uint64(hi.shape[0]),
                                        (C.c_uint32 * 6)(*[int(x) for x in ranges]), C.byref(h)))
        self.h = h

    @classmethod
    def from_segment(cls, backend, host_segment):
        """the run that starts with this segment: its initial memory, heap and ranges"""
        a = runner_segment_arrays(host_segment.view)
        return cls(backend, a["initial_memory"], a["initial_heap"], a["ranges"])

    def adapt_next(self, seg):
        """cm_run_adapt_next: seg = a RunSegmentC (run_segment) or a HostSegment; returns the device input, advances the image."""
        if not isinstance(seg, RunSegmentC):
            seg = run_segment(seg)
        h = C.c_void_p()
        self.B._ck(self.L.cm_run_adapt_next(self.h, C.byref(seg), C.byref(h)))
        return h

    def lengths(self):
        """cm_run_memory without arrays: (cells in the locals, cells in the heap)"""
        nl, nh = C.c_uint64(0), C.c_uint64(0)
        self.B._ck(self.L.cm_run_memory(self.h, None, C.c_uint64(0), C.byref(nl), None, C.c_uint64(0), C.byref(nh)))
        return nl.value, nh.value

    def memory(self):
        """cm_run_memory: (locals (n, 4), heap (n, 4)); heap index i = the cell at 2^28 - 1 - i"""
        nl, nh = (C.c_uint64(x) for x in self.lengths())
        lo, hi = np.zeros((nl.value, 4), dtype=np.uint32), np.zeros((nh.value, 4), dtype=np.uint32)
        self.B._ck(self.L.cm_run_memory(self.h, _p(lo), C.c_uint64(nl.value), C.byref(nl), _p(hi), C.c_uint64(nh.value), C.byref(nh)))
        return lo, hi

    def prove(self, segs, inflight=3, cfg=None, transitions=False):
        """cm_prove_run: the next segments of this run (RunSegmentC or HostSegment each), proved in order of `segs`.
        transitions=True: cm_prove_run_transitions -> (proofs, [MemTransition]), every segment's write set between its two roots."""
        segs = [s if isinstance(s, RunSegmentC) else run_segment(s) for s in segs]
        n = len(segs)
        ins = (C.c_void_p * n)(*[C.addressof(s) for s in segs])
        outs = (C.c_void_p * n)()
        if transitions:
            ts = (C.c_void_p * n)()
            rc = self.L.cm_prove_run_transitions(self.h, ins, C.c_uint32(n), _cfg(cfg), C.c_uint32(inflight), outs, ts)
            moves = [_take_transition(self.L, C.c_void_p(ts[i])) if ts[i] else None for i in range(n)]
        else:
            rc = self.L.cm_prove_run(self.h, ins, C.c_uint32(n), _cfg(cfg), C.c_uint32(inflight), outs)
        proofs = [Proof(self.L, C.c_void_p(outs[i])) if outs[i] else None for i in range(n)]
        if rc != 0:
            try:
                self.B._ck(rc)
            except CmError as e:
                e.partial = proofs
                e.partial_transitions = moves if transitions else None
                raise
        return (proofs, moves) if transitions else proofs

    def free(self):
        if self.h:
            self.L.cm_run_free(self.h)
            self.h = None


def prove_run(backend, host_segments, inflight=3, cfg=None):
    """A whole run from its runner segments: one cm_run from the first segment's memory, every segment through cm_prove_run."""
    run = Run.from_segment(backend, host_segments[0])
    try:
        return run.prove(host_segments, inflight, cfg)
    finally:
        run.free()


class VerifyResultC(C.Structure):
    """cm_verify_result: one proof's verdict from cm_verify_many"""
    _fields_ = [("status", C.c_int32), ("check", C.c_int32), ("message", C.c_char * 160)]


def _proof_handles(proofs):
    return (C.c_void_p * len(proofs))(*[p.h.value if isinstance(p.h, C.c_void_p) else p.h for p in proofs])


VERIFY_ARITH_ON_DEVICE = 1   # CM_VERIFY_ARITH_ON_DEVICE


def _verify_flags(arith):
    if arith not in ("host", "device"):
        raise ValueError("arith must be 'host' or 'device'")
    return VERIFY_ARITH_ON_DEVICE if arith == "device" else 0


def verify_many(proofs, cfg=None, lib=None, stream=0, checks=False, arith="host"):
    """cm_verify_many (GPU, no CPU fallback): every proof's verdict from one batch — [(status, message)], the host verifier's own
    status and words per proof (checks=True: (status, message, CM_VERIFY_* id)).  Raises CmError for everything that is not a
    verdict (no device, no proofs).  arith="device": cm_verify_many_ex with CM_VERIFY_ARITH_ON_DEVICE, the public LogUp sum and
    the OODS check decided by the GPU as well."""
    L = lib or proofs[0].L
    n = len(proofs)
    res = (VerifyResultC * max(n, 1))()
    flags = _verify_flags(arith)
    if flags:
        rc = L.cm_verify_many_ex(_proof_handles(proofs), C.c_uint32(n), _cfg(cfg), C.c_uint32(flags), res, C.c_uint64(stream))
    else:
        rc = L.cm_verify_many(_proof_handles(proofs), C.c_uint32(n), _cfg(cfg), res, C.c_uint64(stream))
    if rc not in (0, 11):
        raise _lib_error(L, rc)
    out = [(r.status, r.message.decode(errors="replace")) + ((r.check,) if checks else ()) for r in res[:n]]
    return out


class VerifyStatsC(C.Structure):
    """cm_verify_stats: the shapes of one proof's device-verifier plan"""
    _fields_ = [("struct_size", C.c_uint32), ("early_check", C.c_int32), ("n_answer_jobs", C.c_uint32), ("max_batch_entries", C.c_uint32),
                ("max_first_pairs", C.c_uint32), ("max_inner_pairs", C.c_uint32), ("max_level_nodes", C.c_uint32),
                ("merkle_lds_bytes", C.c_uint32), ("n_tree_jobs", C.c_uint32), ("n_slots", C.c_uint32),
                ("blob_words", C.c_uint64), ("scratch_words", C.c_uint64)]


class VerifySlotC(C.Structure):
    """cm_verify_slot: one check of one proof as cm_verify_many_detail left it"""
    _fields_ = [("check", C.c_int32), ("on_device", C.c_uint32), ("raised", C.c_uint32), ("message", C.c_char * 116)]


def verify_plan_stats(proofs, cfg=None, lib=None):
    """cm_verify_plan_stats (host code, no GPU): per proof a dict of the shapes cm_verify_many's plan has for it alone"""
    L = lib or proofs[0].L
    n = len(proofs)
    out = (VerifyStatsC * max(n, 1))()
    for s in out:
        s.struct_size = C.sizeof(VerifyStatsC)
    rc = L.cm_verify_plan_stats(_proof_handles(proofs), C.c_uint32(n), _cfg(cfg), out)
    if rc:
        raise _lib_error(L, rc)
    return [{name: getattr(s, name) for name, _ in VerifyStatsC._fields_[1:]} for s in out[:n]]


def verify_many_detail(proofs, cfg=None, lib=None, stream=0, arith="host"):
    """cm_verify_many_detail (GPU): per proof ((status, message, check), [(check, message, on_device, raised)]) — cm_verify_many's
    verdict and every slot of the proof in the host verifier's order, from the same launches.  arith="device":
    cm_verify_many_detail_ex with CM_VERIFY_ARITH_ON_DEVICE (the LogUp sum and the OODS check are the first two slots)."""
    L = lib or proofs[0].L
    n = len(proofs)
    flags = _verify_flags(arith)
    res = (VerifyResultC * max(n, 1))()
    first = (C.c_uint32 * (n + 1))()
    cap = 64 * max(n, 1)
    while True:
        slots = (VerifySlotC * cap)()
        if flags:
            rc = L.cm_verify_many_detail_ex(_proof_handles(proofs), C.c_uint32(n), _cfg(cfg), C.c_uint32(flags), res, slots, C.c_uint32(cap),
                                            first, C.c_uint64(stream))
        else:
            rc = L.cm_verify_many_detail(_proof_handles(proofs), C.c_uint32(n), _cfg(cfg), res, slots, C.c_uint32(cap), first, C.c_uint64(stream))
        if rc == 1 and first[n] > cap:
            cap = first[n]
            continue
        break
    if rc not in (0, 11):
        raise _lib_error(L, rc)
    return [((r.status, r.message.decode(errors="replace"), r.check),
             [(s.check, s.message.decode(errors="replace"), bool(s.on_device), bool(s.raised)) for s in slots[first[i]:first[i + 1]]])
            for i, r in enumerate(res[:n])]


def verify_many_timing(lib=None):
    """cm_verify_many_timing: where the calling thread's last cm_verify_many spent its time (ms)"""
    L = lib or load_library()
    ms = (C.c_double * 4)()
    L.cm_verify_many_timing(ms)
    return dict(zip(("plan", "upload", "kernels", "download"), list(ms)))


def verify_run(proofs, cfg=None, lib=None, device=False, arith="host"):
    """cm_verify_run (host code; device=True: cm_verify_run_device, the proofs checked on the GPU in one batch): (status, message);
    0 = every proof verifies and each starts where its predecessor stopped.  arith="device" (with device=True):
    cm_verify_run_device_ex with CM_VERIFY_ARITH_ON_DEVICE."""
    L = lib or proofs[0].L
    n = len(proofs)
    hs = _proof_handles(proofs)
    flags = _verify_flags(arith)
    if flags and not device:
        raise ValueError("arith='device' needs device=True")
    if flags:
        rc = L.cm_verify_run_device_ex(hs, C.c_uint32(n), _cfg(cfg), C.c_uint32(flags))
    else:
        rc = (L.cm_verify_run_device if device else L.cm_verify_run)(hs, C.c_uint32(n), _cfg(cfg))
    buf = C.create_string_buffer(1024)
    L.cm_last_error(buf, C.c_size_t(1024))
    return rc, buf.value.decode(errors="replace") if rc else ""


Backend.run_begin = lambda self, initial_memory, initial_heap, ranges: Run(self, initial_memory, initial_heap, ranges)
Backend.prove_run = lambda self, host_segments, inflight=3, cfg=None: prove_run(self, host_segments, inflight, cfg)
Backend.verify_run = lambda self, proofs, cfg=None, device=False, arith="host": verify_run(proofs, cfg, self.L, device, arith)
Backend.verify_many = lambda self, proofs, cfg=None, arith="host": verify_many(proofs, cfg, self.L, arith=arith)
Backend.verify_many_detail = lambda self, proofs, cfg=None, arith="host": verify_many_detail(proofs, cfg, self.L, arith=arith)
Backend.verify_plan_stats = lambda self, proofs, cfg=None: verify_plan_stats(proofs, cfg, self.L)


# ---- the verifier prelude's arithmetic, op level (include/cairom_hip.h: cm_public_logup_sum_op, cm_point_eval_op) ------------
VERIFY_PUBLIC_SUM_ENTRIES = 256   # CM_PUBLIC_SUM_ENTRIES: entries per workgroup of k_verify_public_sum
RELATIONS_WORDS = 4 * 8 * (1 + 16)  # CM_RELATIONS_WORDS


class PublicSumJobC(C.Structure):
    """cm_public_sum_job"""
    _fields_ = [("head", C.c_uint32 * 7), ("n_program", C.c_uint32), ("n_input", C.c_uint32), ("n_output", C.c_uint32),
                ("entries", C.c_void_p), ("rel_words", C.c_void_p)]


class PointEvalJobC(C.Structure):
    """cm_point_eval_job"""
    _fields_ = [("component", C.c_uint32), ("n_tr_words", C.c_uint32), ("n_it_words", C.c_uint32), ("n_coeff_words", C.c_uint32),
                ("tr", C.c_void_p), ("it", C.c_void_p), ("pp", C.c_void_p), ("rel_words", C.c_void_p), ("coeff", C.c_void_p),
                ("shift", C.c_uint32 * 4)]


def _u32_words(a):
    return np.ascontiguousarray(a, dtype=np.uint32).reshape(-1)


def _addr(a):
    return a.ctypes.data if a.size else None


def public_sum_job(head, program, inp, output, rel_words):
    """(cm_public_sum_job, the arrays it points into): head = 7 words; each list = rows of the 7 words present, addr, value[4], clock"""
    lists = [_u32_words(x) for x in (program, inp, output)]
    for x in lists:
        assert x.size % 7 == 0
    entries = np.concatenate(lists) if sum(x.size for x in lists) else np.zeros(0, np.uint32)
    rel = _u32_words(rel_words)
    assert rel.size == RELATIONS_WORDS and len(head) == 7
    j = PublicSumJobC()
    j.head[:] = [int(w) for w in head]
    j.n_program, j.n_input, j.n_output = (x.size // 7 for x in lists)
    j.entries, j.rel_words = _addr(entries), _addr(rel)
    return j, (entries, rel)


def point_eval_job(component, tr, it, pp, rel_words, coeff, shift):
    """(cm_point_eval_job, the arrays it points into): every array is flat uint32 words, four per QM31"""
    keep = tuple(_u32_words(x) for x in (tr, it, pp, rel_words, coeff))
    j = PointEvalJobC()
    j.component = component
    j.n_tr_words, j.n_it_words, j.n_coeff_words = keep[0].size, keep[1].size, keep[4].size
    j.tr, j.it, j.pp, j.rel_words, j.coeff = (_addr(x) for x in keep)
    j.shift[:] = [int(w) for w in shift]
    return j, keep


def _op_jobs(ctype, jobs):
    arr = (ctype * max(len(jobs), 1))()
    for k, (j, _) in enumerate(jobs):
        arr[k] = j
    return arr


def _op_ck(L, rc):
    if rc:
        raise _lib_error(L, rc)


def public_logup_sum(jobs, lib=None, stream=0):
    """cm_public_logup_sum_op (GPU): jobs = [public_sum_job(...)]; one 4-word tuple per job"""
    L = lib or load_library()
    out = (C.c_uint32 * (4 * max(len(jobs), 1)))()
    _op_ck(L, L.cm_public_logup_sum_op(_op_jobs(PublicSumJobC, jobs), C.c_uint32(len(jobs)), C.c_uint64(stream), out))
    return [tuple(out[4 * k:4 * k + 4]) for k in range(len(jobs))]


def public_logup_sum_host(job, lib=None):
    """cm_public_logup_sum_host (host code, no GPU): the host verifier's initial_logup_sum of one job"""
    L = lib or load_library()
    out = (C.c_uint32 * 4)()
    _op_ck(L, L.cm_public_logup_sum_host(C.byref(job[0]), out))
    return tuple(out)


def point_eval(jobs, lib=None, stream=0):
    """cm_point_eval_op (GPU): jobs = [point_eval_job(...)]; one 4-word tuple per job"""
    L = lib or load_library()
    out = (C.c_uint32 * (4 * max(len(jobs), 1)))()
    _op_ck(L, L.cm_point_eval_op(_op_jobs(PointEvalJobC, jobs), C.c_uint32(len(jobs)), C.c_uint64(stream), out))
    return [tuple(out[4 * k:4 * k + 4]) for k in range(len(jobs))]


def point_eval_host(job, lib=None):
    """cm_point_eval_host (host code, no GPU): the host verifier's point_eval of one job"""
    L = lib or load_library()
    out = (C.c_uint32 * 4)()
    _op_ck(L, L.cm_point_eval_host(C.byref(job[0]), out))
    return tuple(out)


Backend.public_logup_sum = lambda self, jobs, stream=0: public_logup_sum(jobs, self.L, stream)
Backend.public_logup_sum_host = lambda self, job: public_logup_sum_host(job, self.L)
Backend.point_eval = lambda self, jobs, stream=0: point_eval(jobs, self.L, stream)
Backend.point_eval_host = lambda self, job: point_eval_host(job, self.L)


# ---- device-memory accounting, estimate and budget (include/cairom_hip.h, revision 9) --------------------------
N_COMPONENTS = 34


class MemStats(C.Structure):
    """cm_mem_stats: process-wide counters over all thread pools."""
    _fields_ = [("struct_size", C.c_uint32), ("proofs_in_flight", C.c_uint32), ("peak_proofs_in_flight", C.c_uint32),
                ("reserved0", C.c_uint32),
                ("live_bytes", C.c_uint64), ("reserved_bytes", C.c_uint64), ("peak_live_bytes", C.c_uint64),
                ("peak_reserved_bytes", C.c_uint64), ("pinned_host_bytes", C.c_uint64), ("driver_allocs", C.c_uint64),
                ("budget_bytes", C.c_uint64)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_ if n not in ("struct_size", "reserved0")}


class ProofMem(C.Structure):
    """cm_proof_mem: one proof's share of the proving thread's pool."""
    _fields_ = [("struct_size", C.c_uint32), ("n_phases", C.c_uint32),
                ("start_live_bytes", C.c_uint64), ("peak_live_bytes", C.c_uint64), ("peak_reserved_bytes", C.c_uint64),
                ("input_bytes", C.c_uint64), ("driver_allocs", C.c_uint64), ("phase_peak_live_bytes", C.c_uint64 * 32)]

    def as_dict(self, phases=None):
        d = {n: getattr(self, n) for n in ("start_live_bytes", "peak_live_bytes", "peak_reserved_bytes", "input_bytes", "driver_allocs")}
        peaks = [self.phase_peak_live_bytes[i] for i in range(self.n_phases)]
        d["phase_peak_live_bytes"] = dict(zip(phases, peaks)) if phases and len(phases) >= len(peaks) else peaks
        return d


class MemEstimate(C.Structure):
    """cm_mem_estimate: input_bytes, working_bytes (upper bound of a lone proof's peak over its start), cached_bytes."""
    _fields_ = [("struct_size", C.c_uint32), ("reserved0", C.c_uint32),
                ("input_bytes", C.c_uint64), ("working_bytes", C.c_uint64), ("cached_bytes", C.c_uint64)]

    def as_dict(self):
        return {"input_bytes": self.input_bytes, "working_bytes": self.working_bytes, "cached_bytes": self.cached_bytes}


def mem_stats(lib=None):
    """cm_mem_stats_get (host code: works without a GPU and before cm_init)."""
    L = lib or load_library()
    s = MemStats()
    s.struct_size = C.sizeof(MemStats)
    rc = L.cm_mem_stats_get(C.byref(s))
    if rc:
        raise _lib_error(L, rc)
    return s


def mem_reset_peak(lib=None):
    (lib or load_library()).cm_mem_reset_peak()


def set_memory_budget(n_bytes, lib=None):
    """cm_set_memory_budget: 0 = none."""
    (lib or load_library()).cm_set_memory_budget(C.c_uint64(int(n_bytes)))


def estimate_memory(view=None, log_sizes=None, cfg=None, world=1, lib=None):
    """cm_estimate_memory (view = a cm_prover_input*, e.g. HostInput.view) or cm_estimate_memory_logs (34 component log sizes)."""
    L = lib or load_library()
    e = MemEstimate()
    e.struct_size = C.sizeof(MemEstimate)
    if view is not None:
        rc = L.cm_estimate_memory(view, _cfg(cfg), C.c_uint32(world), C.byref(e))
    else:
        logs = (C.c_uint32 * N_COMPONENTS)(*[int(x) for x in log_sizes])
        rc = L.cm_estimate_memory_logs(logs, _cfg(cfg), C.c_uint32(world), C.byref(e))
    if rc:
        raise _lib_error(L, rc)
    return e


Backend.mem_stats = lambda self: mem_stats(self.L)
Backend.mem_reset_peak = lambda self: mem_reset_peak(self.L)
Backend.set_memory_budget = lambda self, n_bytes: set_memory_budget(n_bytes, self.L)
Backend.estimate_memory = lambda self, view=None, log_sizes=None, cfg=None, world=1: estimate_memory(view, log_sizes, cfg, world, self.L)


# ---- compiled-program JSON (crates/common/src/program.rs:143-170, instruction.rs:609-655) ----------------------
def load_program_json(text):
    """Compiled `Program` as the reference serialises it with serde_json: {"data": [{"Instruction": ["0x9", "0x1", ...]}
    | {"Value": [[a, b], [c, d]]}, ...], "entrypoints": {name: {"pc": n, "params": [...], "returns": [...]}},
    "metadata": {...}}.  Returns (cells, entrypoints): `cells` = one word list per program datum — instruction words
    (opcode first, 1..6 words) or the 4 words of a raw QM31 value — in the form cm_vm_run / vm_run take."""
    import json
    doc = json.loads(text)
    unknown = set(doc) - {"data", "entrypoints", "metadata"}
    if unknown:
        raise ValueError(f"unknown Program fields {sorted(unknown)} (the reference denies unknown fields)")
    cells = []
    for item in doc["data"]:
        if "Instruction" in item:
            words = [int(s, 16) for s in item["Instruction"]]
            if not 1 <= len(words) <= 6:
                raise ValueError("instruction must have 1..6 M31 words")
        elif "Value" in item:
            (a, b), (c, d) = item["Value"]
            words = [int(a), int(b), int(c), int(d)]
        else:
            raise ValueError(f"unknown ProgramData variant {list(item)}")
        if any(w >= 2**31 - 1 for w in words):
            raise ValueError("program word is not a canonical M31")
        cells.append(words)
    entry = {name: {"pc": int(e["pc"]), "n_params": sum(_abi_slots(p["ty"]) for p in e.get("params", [])),
                    "n_returns": sum(_abi_slots(r["ty"]) for r in e.get("returns", []))}
             for name, e in doc.get("entrypoints", {}).items()}
    return cells, entry


def _abi_slots(ty):
    """AbiType::size_in_slots (program.rs:30-42); serde externally-tagged enum: "Felt" | {"Pointer": {...}} | ..."""
    if isinstance(ty, str):
        return {"Felt": 1, "Bool": 1, "U32": 2, "Unit": 0}[ty]
    (tag, body), = ty.items()
    if tag == "Pointer":
        return 1
    if tag == "Tuple":
        return sum(_abi_slots(t) for t in body)
    if tag == "Struct":
        return sum(_abi_slots(t) for _, t in body["fields"])
    if tag == "FixedSizeArray":
        return int(body["size"]) * _abi_slots(body["element"])
    raise ValueError(f"unknown AbiType {tag}")


def program_to_json(cells, entrypoints=None):
    """Inverse of load_program_json for instruction-only programs (hex strings like `format!("0x{:x}")`)."""
    import json
    return json.dumps({"data": [{"Instruction": [f"0x{w:x}" for w in ins]} for ins in cells],
                       "entrypoints": entrypoints or {}, "metadata": {}})


# ---- per-component AIR ops (include/cairom_hip.h) -----------------------------------------------------
N_COMPONENTS = 34
N_PREPROCESSED = 7
PREPROCESSED_LOG = (18, 18, 18, 18, 8, 16, 20)
RELATION_WORDS = 8 * 4 + 8 * 16 * 4   # cm_relations: z[8][4], alpha_pow[8][16][4]


def _b_component_info(self, cid):
    a, b, c = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0)
    self._ck(self.L.cm_component_info(C.c_int32(cid), C.byref(a), C.byref(b), C.byref(c)))
    return a.value, b.value, c.value


def _b_component_log_size(self, dev_input, cid):
    lg = C.c_uint32(0)
    self._ck(self.L.cm_component_log_size(dev_input, C.c_int32(cid), C.byref(lg)))
    return lg.value


def _b_trace_write(self, dev_input, cid, cols):
    self._ck(self.L.cm_trace_write(dev_input, C.c_int32(cid), self._harr(cols), C.c_uint64(0)))


def _b_histogram(self, cid, trace_cols, log_size, rc8, rc16, rc20, bitwise):
    self._ck(self.L.cm_histogram(C.c_int32(cid), self._harr(trace_cols), C.c_uint32(log_size), C.c_uint64(rc8), C.c_uint64(rc16),
                                 C.c_uint64(rc20), C.c_uint64(bitwise), C.c_uint64(0)))


def _b_preprocessed_column(self, pp_id, col):
    self._ck(self.L.cm_preprocessed_column(C.c_int32(pp_id), C.c_uint64(col), C.c_uint64(0)))


def _b_interaction_write(self, cid, trace_cols, preprocessed, log_size, rel_words, out_cols):
    r = np.ascontiguousarray(rel_words, dtype=np.uint32)
    assert r.size == RELATION_WORDS
    cs = np.zeros(4, dtype=np.uint32)
    self._ck(self.L.cm_interaction_write(C.c_int32(cid), self._harr(trace_cols), self._harr(preprocessed), C.c_uint32(log_size),
                                         _p(r), self._harr(out_cols), _p(cs), C.c_uint64(0)))
    return cs


def _b_constraints_accumulate(self, cid, trace_lde, interaction_lde, preprocessed_lde, log_size, rel_words, coeff_words,
                              claimed_sum, acc4):
    r = np.ascontiguousarray(rel_words, dtype=np.uint32)
    co = np.ascontiguousarray(coeff_words, dtype=np.uint32)
    cs = np.ascontiguousarray(claimed_sum, dtype=np.uint32)
    self._ck(self.L.cm_constraints_accumulate(C.c_int32(cid), self._harr(trace_lde), self._harr(interaction_lde),
                                              self._harr(preprocessed_lde), C.c_uint32(log_size), _p(r), _p(co), _p(cs),
                                              self._harr(acc4), C.c_uint64(0)))


def _b_fri_decompose(self, f4, log_n):
    lam = np.zeros(4, dtype=np.uint32)
    self._ck(self.L.cm_fri_decompose(self._harr(f4), C.c_uint32(log_n), _p(lam), C.c_uint64(0)))
    return lam


Backend.component_info = _b_component_info
Backend.component_log_size = _b_component_log_size
Backend.trace_write = _b_trace_write
Backend.histogram = _b_histogram
Backend.preprocessed_column = _b_preprocessed_column
Backend.interaction_write = _b_interaction_write
Backend.constraints_accumulate = _b_constraints_accumulate
Backend.fri_decompose = _b_fri_decompose


def _b_accumulate(self, dst4, src4, n):
    self._ck(self.L.cm_accumulate(self._harr(dst4), self._harr(src4), C.c_uint64(n), C.c_uint64(0)))


def _b_secure_powers(self, felt, n):
    f = np.ascontiguousarray(felt, dtype=np.uint32)
    out = np.zeros(4 * n, dtype=np.uint32)
    self._ck(self.L.cm_generate_secure_powers(_p(f), C.c_uint64(n), _p(out)))
    return out.reshape(n, 4)


def _b_col_zero(self, h, n):
    self._ck(self.L.cm_col_zero(C.c_uint64(h), C.c_uint64(n), C.c_uint64(0)))


Backend.accumulate = _b_accumulate
Backend.secure_powers = _b_secure_powers
Backend.col_zero = _b_col_zero


# ---- PCS-free AIR check (include/cairom_hip.h: cm_check_report; reference: debug_tools::assert_constraints) ----------------
N_RELATIONS = 8
RELATION_NAMES = ("registers", "memory", "merkle", "poseidon2", "range_check_8", "range_check_16", "range_check_20", "bitwise")
P_M31 = (1 << 31) - 1


class _CheckReportC(C.Structure):
    _fields_ = [("status", C.c_int32), ("component", C.c_int32), ("constraint", C.c_int32), ("reserved", C.c_int32),
                ("row", C.c_uint64),
                ("failing_rows", C.c_uint64 * N_COMPONENTS),
                ("first_constraint", C.c_int32 * N_COMPONENTS),
                ("first_row", C.c_uint64 * N_COMPONENTS),
                ("claimed_sum", (C.c_uint32 * 4) * N_COMPONENTS),
                ("relation_sum", ((C.c_uint32 * 4) * N_RELATIONS) * N_COMPONENTS),
                ("public_sum", (C.c_uint32 * 4) * N_RELATIONS),
                ("total", C.c_uint32 * 4),
                ("relations", C.c_uint32 * RELATION_WORDS),
                ("message", C.c_char * 256)]


class CheckReport(_CheckReportC):
    """Verdict of cm_check_constraints (the fields of cm_check_report): status 0 ok, 1 lookup value out of range, 2 a constraint
    fails, 3 the LogUp sums do not cancel.  QM31 values are 4 words (to_m31_array order)."""

    @property
    def message(self):
        return _CheckReportC.message.__get__(self).decode(errors="replace")

    @property
    def claimed_sums(self):
        return np.ctypeslib.as_array(self.claimed_sum).copy()

    @property
    def relation_sums(self):
        return np.ctypeslib.as_array(self.relation_sum).copy()

    @property
    def public_sums(self):
        return np.ctypeslib.as_array(self.public_sum).copy()

    @property
    def relation_words(self):
        return np.ctypeslib.as_array(self.relations).copy()

    def relation_balance(self):
        """[8, 4]: sum over the components of relation_sum[c][r] + public_sum[r], per relation (all zero when it balances)"""
        s = self.relation_sums.astype(np.int64).sum(axis=0) + self.public_sums.astype(np.int64)
        return (s % P_M31).astype(np.uint32)

    def unbalanced_relations(self):
        return [RELATION_NAMES[r] for r, w in enumerate(self.relation_balance()) if w.any()]

    def __repr__(self):
        return f"CheckReport(status={self.status}, message={self.message!r})"


def _b_check(self, dev_or_host_input, relations=None):
    """debug_tools::assert_constraints on the GPU.  dev_or_host_input: a device input (upload_input / adapt_segment) or a host
    input with a `.view` (uploaded for the call).  relations: cm_relations words, None = drawn from a default channel."""
    rep = CheckReport()
    r = None
    if relations is not None:
        r = np.ascontiguousarray(relations, dtype=np.uint32)
        assert r.size == RELATION_WORDS
    dev, own = dev_or_host_input, False
    if hasattr(dev_or_host_input, "view"):
        dev, own = self.upload_input(dev_or_host_input), True
    try:
        self._ck(self.L.cm_check_constraints(dev, _p(r) if r is not None else None, C.byref(rep)))
    finally:
        if own:
            self.free_input(dev)
    return rep


def _b_constraints_check(self, cid, trace_cols, interaction_cols, preprocessed, log_size, rel_words, claimed_sum, row_status=0):
    """one component on its trace domain: (failing_rows, first_constraint, first_row); row_status = an optional column handle"""
    r = np.ascontiguousarray(rel_words, dtype=np.uint32)
    assert r.size == RELATION_WORDS
    cs = np.ascontiguousarray(claimed_sum, dtype=np.uint32)
    n, k, row = C.c_uint64(0), C.c_int32(0), C.c_uint64(0)
    self._ck(self.L.cm_constraints_check(C.c_int32(cid), self._harr(trace_cols), self._harr(interaction_cols), self._harr(preprocessed),
                                         C.c_uint32(log_size), _p(r), _p(cs), C.c_uint64(row_status), C.byref(n), C.byref(k),
                                         C.byref(row), C.c_uint64(0)))
    return n.value, k.value, row.value


def _b_relation_sums(self, cid, trace_cols, preprocessed, log_size, rel_words):
    """[8, 4] words: per relation, sum over rows and entries of mult / combine(values)"""
    r = np.ascontiguousarray(rel_words, dtype=np.uint32)
    assert r.size == RELATION_WORDS
    out = np.zeros((N_RELATIONS, 4), dtype=np.uint32)
    self._ck(self.L.cm_relation_sums(C.c_int32(cid), self._harr(trace_cols), self._harr(preprocessed), C.c_uint32(log_size), _p(r),
                                     _p(out), C.c_uint64(0)))
    return out


Backend.check = _b_check
Backend.constraints_check = _b_constraints_check
Backend.relation_sums = _b_relation_sums


# ---- relation tracker (include/cairom_hip.h: cm_relation_entry; reference: debug_tools/relation_tracker.rs) ----------------
MAX_RELATION_SIZE = 16
COMPONENT_NAMES = ("AssertEqFpImm", "CallAbsImm", "JmpImm", "JnzFpImm", "Ret", "StoreImm", "StoreFpFp", "StoreFpImm", "DoubleDerefFpImm",
                   "DoubleDerefFpFp", "StoreFramePointer", "U32StoreImm", "U32StoreAddFpImm", "U32StoreMulFpImm", "U32StoreDivFpImm",
                   "U32StoreEqFpFp", "U32StoreEqFpImm", "U32StoreLtFpImm", "U32StoreLtFpFp", "U32StoreAddFpFp", "U32StoreSubFpFp",
                   "U32StoreMulFpFp", "U32StoreDivFpFp", "U32StoreBitwiseFpFp", "U32StoreBitwiseFpImm", "StoreLeFpImm", "MemoryC", "MerkleC",
                   "ClockUpdateC", "Poseidon2C", "RangeCheck8C", "RangeCheck16C", "RangeCheck20C", "BitwiseC", "PublicData")
assert len(COMPONENT_NAMES) == N_COMPONENTS + 1


class RelationEntry(C.Structure):
    """One tuple of the tracker's summary (cm_relation_entry): net multiplicity (canonical M31, never 0), the lowest
    (component, row) merged into it (component N_COMPONENTS = public data) and the number of entries merged."""
    _fields_ = [("relation", C.c_uint32), ("multiplicity", C.c_uint32), ("n_values", C.c_uint32), ("first_component", C.c_uint32),
                ("first_row", C.c_uint64), ("n_entries", C.c_uint64), ("values", C.c_uint32 * MAX_RELATION_SIZE)]

    @property
    def relation_name(self):
        return RELATION_NAMES[self.relation]

    @property
    def tuple(self):
        """the values without trailing zeros"""
        return tuple(int(v) for v in self.values[:self.n_values])

    @property
    def signed_multiplicity(self):
        m = int(self.multiplicity)
        return m - P_M31 if m > P_M31 // 2 else m

    def __repr__(self):
        return (f"RelationEntry({self.relation_name}, {list(self.tuple)} -> {self.signed_multiplicity}, "
                f"{COMPONENT_NAMES[self.first_component]} row {self.first_row}, {self.n_entries} entries)")


class RelationSummary:
    """What the tracker returns: .entries (at most cap of them, by relation id, then by grouping key), .n_total, .truncated,
    .report (the CheckReport of the whole-segment call, None at the op level)."""

    def __init__(self, entries, n_total, report=None):
        self.entries, self.n_total, self.report = entries, n_total, report

    @property
    def truncated(self):
        return self.n_total > len(self.entries)

    def as_dict(self):
        """{(relation name, values without trailing zeros): net multiplicity}"""
        return {(e.relation_name, e.tuple): int(e.multiplicity) for e in self.entries}

    def __str__(self):
        lines, last = [], None
        for e in self.entries:
            if e.relation != last:
                lines.append(e.relation_name)
                last = e.relation
            lines.append(f"  {list(e.tuple)} -> {e.signed_multiplicity}   ({COMPONENT_NAMES[e.first_component]} row {e.first_row}, "
                         f"{e.n_entries} entries)")
        if self.truncated:
            lines.append(f"  ... {self.n_total - len(self.entries)} more")
        return "\n".join(lines)


def _relation_words(relations):
    if relations is None:
        return None
    r = np.ascontiguousarray(relations, dtype=np.uint32)
    assert r.size == RELATION_WORDS
    return r


def _b_track_relations(self, dev_or_host_input, relations=None, mask=0, cap=4096):
    """The relation tracker on a whole segment: the check's passes, then the tuples of the tracked relations whose multiplicities
    do not cancel, public data included.  mask 0 = the relations whose sums do not cancel; bit r = track relation r regardless."""
    rep = CheckReport()
    r = _relation_words(relations)
    buf = (RelationEntry * max(cap, 1))()
    n_total = C.c_uint64(0)
    dev, own = dev_or_host_input, False
    if hasattr(dev_or_host_input, "view"):
        dev, own = self.upload_input(dev_or_host_input), True
    try:
        self._ck(self.L.cm_track_relations(dev, _p(r) if r is not None else None, C.c_uint32(mask), C.byref(rep),
                                           buf if cap else None, C.c_uint64(cap), C.byref(n_total)))
    finally:
        if own:
            self.free_input(dev)
    return RelationSummary([buf[i] for i in range(min(n_total.value, cap))], n_total.value, rep)


def _b_relation_entries(self, cid, trace_cols, preprocessed, log_size, rel_words, mask=0, cap=4096):
    """the tracker's summary of ONE component's trace-domain columns (no public data); mask 0 = all 8 relations"""
    r = _relation_words(rel_words)
    buf = (RelationEntry * max(cap, 1))()
    n_total = C.c_uint64(0)
    self._ck(self.L.cm_relation_entries(C.c_int32(cid), self._harr(trace_cols), self._harr(preprocessed), C.c_uint32(log_size), _p(r),
                                        C.c_uint32(mask), buf if cap else None, C.c_uint64(cap), C.byref(n_total), C.c_uint64(0)))
    return RelationSummary([buf[i] for i in range(min(n_total.value, cap))], n_total.value)


Backend.track_relations = _b_track_relations
Backend.relation_entries = _b_relation_entries


# ---- a whole run, checked before it is proved (include/cairom_hip.h: cm_link_diff, cm_check_chain, cm_check_run) -----------
LINK_KINDS = {1: "changed", 2: "only in next", 3: "only in prev"}


class LinkCell(C.Structure):
    """cm_link_cell: one cell that makes a link's roots differ — kind 1 present in both with different values, 2 present only in
    the later segment's initial memory, 3 only in the earlier segment's final memory."""
    _fields_ = [("kind", C.c_uint32), ("address", C.c_uint32), ("prev_value", C.c_uint32 * 4), ("next_value", C.c_uint32 * 4),
                ("prev_clock", C.c_uint32)]

    def words(self):
        return [self.kind, self.address] + list(self.prev_value) + list(self.next_value) + [self.prev_clock]

    def __repr__(self):
        return (f"LinkCell({LINK_KINDS.get(self.kind, self.kind)}, address {self.address}, {list(self.prev_value)} -> "
                f"{list(self.next_value)}, prev clock {self.prev_clock})")


class _LinkReportC(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("reserved0", C.c_uint32),
                ("prev_final_pc", C.c_uint32), ("prev_final_fp", C.c_uint32), ("next_initial_pc", C.c_uint32), ("next_initial_fp", C.c_uint32),
                ("pc_equal", C.c_uint32), ("fp_equal", C.c_uint32), ("roots_equal", C.c_uint32), ("reserved1", C.c_uint32),
                ("prev_final_root", C.c_uint32), ("next_initial_root", C.c_uint32),
                ("n_changed", C.c_uint64), ("n_only_next", C.c_uint64), ("n_only_prev", C.c_uint64), ("n_zero_only", C.c_uint64),
                ("message", C.c_char * 160)]


class LinkReport(_LinkReportC):
    """cm_link_report: registers and roots on both sides of a link, per-kind totals of the listed cells, the count of cells that
    are present on one side only with an all-zero value (they do not change the root and are not listed), and the message."""

    @property
    def message(self):
        return _LinkReportC.message.__get__(self).decode(errors="replace")

    @property
    def first_sentence(self):
        """cm_verify_run's words for this link, "" when registers and roots chain"""
        m = self.message
        return m.split(". ")[0] if m.startswith("run: ") else ""

    @property
    def n_total(self):
        return self.n_changed + self.n_only_next + self.n_only_prev

    @property
    def ok(self):
        return bool(self.pc_equal and self.fp_equal and self.roots_equal and self.n_total == 0)

    def __repr__(self):
        return f"LinkReport(ok={self.ok}, message={self.message!r})"


class RunCheckC(C.Structure):
    """cm_run_check: one segment's record of cm_check_run / cm_check_chain"""
    _fields_ = [("check", CheckReport), ("link", LinkReport), ("link_cells_written", C.c_uint64), ("link_cells_total", C.c_uint64)]


class LinkDiff:
    """One link: .report (LinkReport), .cells (the first `cap` LinkCells in ascending address order), .n_total, .truncated."""

    def __init__(self, report, cells, n_total):
        self.report, self.cells, self.n_total = report, cells, n_total

    @property
    def truncated(self):
        return self.n_total > len(self.cells)

    def cell_words(self):
        """(len(cells), 11) u32: kind, address, prev_value[4], next_value[4], prev_clock"""
        return np.array([c.words() for c in self.cells], dtype=np.uint32).reshape(-1, 11)

    def __repr__(self):
        return f"LinkDiff({self.report.message!r}, {len(self.cells)} of {self.n_total} cells)"


class SegmentCheck:
    """One segment of a checked run: .check (CheckReport, None from check_chain), .link (LinkDiff, None for the first segment)."""

    def __init__(self, check, link):
        self.check, self.link = check, link

    @property
    def ok(self):
        return (self.check is None or self.check.status == 0) and (self.link is None or self.link.report.ok)


class RunCheck:
    """What Run.check / check_run / check_chain return: .segments (SegmentCheck each), .summary (the library's one line about the
    first bad link or segment, "" when the run will prove and chain), .ok."""

    def __init__(self, segments, summary):
        self.segments, self.summary = segments, summary

    @property
    def ok(self):
        return all(s.ok for s in self.segments)

    def __repr__(self):
        return f"RunCheck(ok={self.ok}, summary={self.summary!r}, {len(self.segments)} segments)"


def _copy_struct(cls, src):
    out = cls()
    C.memmove(C.byref(out), C.byref(src), C.sizeof(cls))
    return out


def _run_check_result(L, recs, cells, n, cap, with_air):
    buf = C.create_string_buffer(1024)
    L.cm_last_error(buf, C.c_size_t(1024))
    segs = []
    for i in range(n):
        link = None
        if i > 0:
            got = [_copy_struct(LinkCell, cells[i * cap + k]) for k in range(recs[i].link_cells_written)]
            link = LinkDiff(_copy_struct(LinkReport, recs[i].link), got, recs[i].link_cells_total)
        segs.append(SegmentCheck(_copy_struct(CheckReport, recs[i].check) if with_air else None, link))
    return RunCheck(segs, buf.value.decode(errors="replace"))


def link_diff(prev, next, cap=64, lib=None):
    """cm_link_diff: the cells that make `next`'s initial root differ from `prev`'s final root (two device inputs, e.g. of
    Backend.adapt_segment / Run.adapt_next) -> LinkDiff.  The report's first sentence numbers prev 0 and next 1."""
    L = lib or load_library()
    rep = LinkReport()
    rep.struct_size = C.sizeof(LinkReport)
    buf = (LinkCell * max(cap, 1))()
    n_total = C.c_uint64(0)
    rc = L.cm_link_diff(prev, next, C.byref(rep), buf if cap else None, C.c_uint64(cap), C.byref(n_total))
    if rc:
        raise _lib_error(L, rc)
    return LinkDiff(rep, [_copy_struct(LinkCell, buf[i]) for i in range(min(n_total.value, cap))], n_total.value)


def check_chain(dev_inputs, cap=64, lib=None):
    """cm_check_chain: the links of segments adapted one by one (device inputs in run order) -> RunCheck without AIR reports."""
    L = lib or load_library()
    n = len(dev_inputs)
    ins = (C.c_void_p * n)(*[d.value if isinstance(d, C.c_void_p) else d for d in dev_inputs])
    recs = (RunCheckC * max(n, 1))()
    cells = (LinkCell * max(n * cap, 1))()
    rc = L.cm_check_chain(ins, C.c_uint32(n), recs, cells if cap else None, C.c_uint64(cap))
    if rc:
        raise _lib_error(L, rc)
    return _run_check_result(L, recs, cells, n, cap, False)


def _run_check(self, segs, relations=None, cap=64):
    """cm_check_run: the next segments of this run (RunSegmentC or HostSegment each) adapted, AIR-checked and link-diffed instead
    of proved -> RunCheck; the image advances as under prove().  A segment that cannot be adapted raises CmError with the records
    in front of it as e.partial (a RunCheck) and leaves the image at that segment's start."""
    segs = [s if isinstance(s, RunSegmentC) else run_segment(s) for s in segs]
    n = len(segs)
    ins = (C.c_void_p * n)(*[C.addressof(s) for s in segs])
    recs = (RunCheckC * max(n, 1))()
    cells = (LinkCell * max(n * cap, 1))()
    r = _relation_words(relations)
    rc = self.L.cm_check_run(self.h, ins, C.c_uint32(n), _p(r) if r is not None else None, recs, cells if cap else None, C.c_uint64(cap))
    if rc != 0:
        try:
            self.B._ck(rc)
        except CmError as e:
            done = 0
            while done < n and any(recs[done].check.relations):    # (a record the call reached holds the relations it used)
                done += 1
            e.partial = _run_check_result(self.L, recs, cells, done, cap, True)
            raise
    return _run_check_result(self.L, recs, cells, n, cap, True)


Run.check = _run_check


def check_run(backend, host_segments, relations=None, cap=64):
    """A whole run checked from its runner segments: makes and frees its own Run, so a later prove_run starts from the run's
    beginning."""
    run = Run.from_segment(backend, host_segments[0])
    try:
        return run.check(host_segments, relations, cap)
    finally:
        run.free()


Backend.check_run = lambda self, host_segments, relations=None, cap=64: check_run(self, host_segments, relations, cap)
Backend.check_chain = lambda self, dev_inputs, cap=64: check_chain(dev_inputs, cap, self.L)
Backend.link_diff = lambda self, prev, next, cap=64: link_diff(prev, next, cap, self.L)


# ---- memory openings (include/cairom_hip.h, additive to revision 10) ----------------------------------------------
ADDRESS_SPACE = 1 << 28


class MemOpening(C.Structure):
    """cm_mem_opening: one cell's value and its authentication path under a memory root (siblings[k] = depth 28 - k)."""
    _fields_ = [("address", C.c_uint32), ("present", C.c_uint32), ("value", C.c_uint32 * 4), ("siblings", C.c_uint32 * 28)]

    def words(self):
        return [self.address, self.present] + list(self.value) + list(self.siblings)

    @classmethod
    def from_words(cls, words):
        w = [int(x) for x in words]
        return cls(w[0], w[1], (C.c_uint32 * 4)(*w[2:6]), (C.c_uint32 * 28)(*w[6:34]))

    def __repr__(self):
        return f"MemOpening(address={self.address}, present={self.present}, value={tuple(self.value)})"


def _opening_array(openings):
    """openings (a list of MemOpening, a ctypes array of them, or an (n, 34) word array) -> (ctypes array, n)"""
    if isinstance(openings, C.Array):
        return openings, len(openings)
    if isinstance(openings, np.ndarray):
        openings = [MemOpening.from_words(r) for r in openings.reshape(-1, 34)]
    n = len(openings)
    buf = (MemOpening * max(n, 1))()
    for i, o in enumerate(openings):
        C.memmove(C.byref(buf, i * C.sizeof(MemOpening)), C.byref(o), C.sizeof(MemOpening))
    return buf, n


def _open_call(L, fn, head, addresses):
    a = np.ascontiguousarray(np.array(addresses, dtype=np.uint64).reshape(-1))
    if a.size and int(a.max()) >= 1 << 32:
        raise ValueError("an address does not fit 32 bits")
    a = a.astype(np.uint32)
    n = a.shape[0]
    buf = (MemOpening * max(n, 1))()
    root = C.c_uint32(0)
    rc = fn(*head, _p(a) if n else None, C.c_uint64(n), buf if n else None, C.byref(root))
    if rc:
        raise _lib_error(L, rc)
    return [_copy_struct(MemOpening, buf[i]) for i in range(n)], root.value


def _backend_open_memory(self, dev_input, which, addresses):
    """cm_input_open_memory: the openings of `addresses` under the input's initial (which = 0) or final (1) tree, built on the GPU
    -> ([MemOpening], root)."""
    return _open_call(self.L, self.L.cm_input_open_memory, (dev_input, C.c_uint32(which)), addresses)


def _run_open(self, addresses):
    """cm_run_open_memory: openings under the root of the image as it is now -> ([MemOpening], root).  The image's tree is built
    on first use and dropped when the image advances."""
    return _open_call(self.L, self.L.cm_run_open_memory, (self.h,), addresses)


def verify_openings(root, openings, lib=None, stream=0):
    """cm_verify_memory_openings (GPU, batched) -> [bool], one per opening."""
    L = lib or load_library()
    buf, n = _opening_array(openings)
    ok = (C.c_uint8 * max(n, 1))()
    rc = L.cm_verify_memory_openings(C.c_uint32(root), buf if n else None, C.c_uint64(n), ok if n else None, C.c_uint64(stream))
    if rc:
        raise _lib_error(L, rc)
    return [bool(ok[i]) for i in range(n)]


def verify_opening(root, opening, lib=None):
    """cm_verify_memory_opening (host code, no GPU) -> (status, message): (0, "") accepted, (11, why) rejected."""
    L = lib or load_library()
    rc = L.cm_verify_memory_opening(C.c_uint32(root), C.byref(opening))
    if not rc:
        return 0, ""
    buf = C.create_string_buffer(512)
    L.cm_last_error(buf, C.c_size_t(512))
    return rc, buf.value.decode(errors="replace")


Backend.open_memory = _backend_open_memory
Backend.verify_openings = lambda self, root, openings, stream=0: verify_openings(root, openings, self.L, stream)
Run.open = _run_open


# ---- range openings (include/cairom_hip.h, additive to revision 10) -------------------------------------------------
RANGE_MAX_CELLS = 1 << 24
RANGE_KERNELS = ("cells", "level", "tail")


class MemRangeOpening(C.Structure):
    """cm_mem_range_opening: a contiguous run of cells under a memory root.  left[k] / right[k] = the node left / right of the
    interval the range covers at depth 28 - k, where hashing it up needs one, else 0.  The values travel beside the record."""
    _fields_ = [("start", C.c_uint32), ("n_cells", C.c_uint32), ("left", C.c_uint32 * 28), ("right", C.c_uint32 * 28)]

    def words(self):
        return [self.start, self.n_cells] + list(self.left) + list(self.right)

    @classmethod
    def from_words(cls, words):
        w = [int(x) for x in words]
        return cls(w[0], w[1], (C.c_uint32 * 28)(*w[2:30]), (C.c_uint32 * 28)(*w[30:58]))

    def __repr__(self):
        return f"MemRangeOpening(start={self.start}, n_cells={self.n_cells})"


class MemRangeStep(C.Structure):
    """cm_mem_range_step: one hashing step of a range's verification (cm_mem_range_plan)."""
    _fields_ = [("depth", C.c_uint32), ("lo", C.c_uint32), ("hi", C.c_uint32), ("kernel", C.c_uint32), ("uses_left", C.c_uint32),
                ("uses_right", C.c_uint32)]


def _range_call(L, fn, head, start, n):
    start, n = int(start), int(n)
    if not (0 <= start < 1 << 32 and 0 <= n < 1 << 32):
        raise ValueError("start or n does not fit 32 bits")
    # (a refused call writes nothing: the array only has to exist)
    values = np.zeros((n if 0 < n <= RANGE_MAX_CELLS else 1, 4), dtype=np.uint32)
    out, root = MemRangeOpening(), C.c_uint32(0)
    rc = fn(*head, C.c_uint32(start), C.c_uint32(n), _p(values), C.byref(out), C.byref(root))
    if rc:
        raise _lib_error(L, rc)
    return out, values, root.value


def _backend_open_memory_range(self, dev_input, which, start, n):
    """cm_input_open_memory_range: the cells [start, start + n) under the input's initial (which = 0) or final (1) tree, built on
    the GPU -> (MemRangeOpening, values (n, 4), root)."""
    return _range_call(self.L, self.L.cm_input_open_memory_range, (dev_input, C.c_uint32(which)), start, n)


def _run_open_range(self, start, n):
    """cm_run_open_memory_range: a range under the root of the image as it is now -> (MemRangeOpening, values (n, 4), root).
    Shares the cached image tree of Run.open."""
    return _range_call(self.L, self.L.cm_run_open_memory_range, (self.h,), start, n)


def _run_open_image(self):
    """The whole image under its one root: the locals [0, n_l) and the heap [2^28 - n_h, 2^28), each omitted when empty ->
    ([(MemRangeOpening, values)], root).  Every other cell is zero exactly when both ranges verify under a root that commits to
    nothing else: the sibling words of the two records are what stands next to the image."""
    n_l, n_h = self.lengths()
    spans = [(s, n) for s, n in ((0, n_l), (ADDRESS_SPACE - n_h, n_h)) if n]
    if not spans:
        raise CmError("open_image: the image is empty: there is no tree to open")
    out, root = [], None
    for s, n in spans:
        for off in range(0, n, RANGE_MAX_CELLS):                                  # (one call takes 2^24 cells)
            rec, values, root = self.open_range(s + off, min(RANGE_MAX_CELLS, n - off))
            out.append((rec, values))
    return out, root


def _range_values(opening, values):
    v = np.ascontiguousarray(values, dtype=np.uint32).reshape(-1)
    if v.size != 4 * opening.n_cells and opening.n_cells <= RANGE_MAX_CELLS:
        raise ValueError(f"{v.size} value words for a range of {opening.n_cells} cells")
    return v if v.size else np.zeros(4, dtype=np.uint32)


def verify_range(root, opening, values, lib=None, stream=0):
    """cm_verify_memory_range (GPU) -> bool: record and values are well formed and hash to `root`."""
    L = lib or load_library()
    v = _range_values(opening, values)
    ok = C.c_uint8(0)
    rc = L.cm_verify_memory_range(C.c_uint32(root), C.byref(opening), _p(v), C.byref(ok), C.c_uint64(stream))
    if rc:
        raise _lib_error(L, rc)
    return bool(ok.value)


def verify_range_host(root, opening, values, lib=None):
    """cm_verify_memory_range_host (host code, no GPU) -> (status, message): (0, "") accepted, (11, why) rejected."""
    L = lib or load_library()
    v = _range_values(opening, values)
    rc = L.cm_verify_memory_range_host(C.c_uint32(root), C.byref(opening), _p(v))
    if not rc:
        return 0, ""
    buf = C.create_string_buffer(512)
    L.cm_last_error(buf, C.c_size_t(512))
    return rc, buf.value.decode(errors="replace")


def mem_range_plan(start, n, lib=None):
    """cm_mem_range_plan: the hashing steps of a range's verification, one dict per step: depth, lo, hi (the nodes the step
    produces), kernel (a RANGE_KERNELS name), uses_left, uses_right.  Host code: needs no GPU."""
    L = lib or load_library()
    steps = (MemRangeStep * 29)()
    k = C.c_uint32(0)
    rc = L.cm_mem_range_plan(C.c_uint32(start), C.c_uint32(n), steps, C.c_uint32(29), C.byref(k))
    if rc:
        raise _lib_error(L, rc)
    return [{"depth": s.depth, "lo": s.lo, "hi": s.hi, "kernel": RANGE_KERNELS[s.kernel], "uses_left": bool(s.uses_left),
             "uses_right": bool(s.uses_right)} for s in steps[:k.value]]


Backend.open_memory_range = _backend_open_memory_range
Backend.verify_range = lambda self, root, opening, values, stream=0: verify_range(root, opening, values, self.L, stream)
Run.open_range = _run_open_range
Run.open_image = _run_open_image


# ---- set openings (include/cairom_hip.h, additive to revision 10) ---------------------------------------------------
SET_MAX_CELLS = 1 << 20
SET_KERNELS = ("cells", "level", "tail")


class MemSetStep(C.Structure):
    """cm_mem_set_step: one hashing step of a set's verification (cm_mem_set_plan)."""
    _fields_ = [("depth", C.c_uint32), ("n_nodes", C.c_uint32), ("n_siblings", C.c_uint32), ("kernel", C.c_uint32)]


class MemSetOpening:
    """Any set of cells under a memory root: .addresses (strictly ascending), .values (n, 4), .siblings (depth by depth from depth
    28 up, inside a depth by ascending node: the sibling of every node on a path of the set whose sibling is on none) and
    .counts (28: the words per depth, a function of the addresses alone).  Built by Backend.open_memory_set / Run.open_set, or
    from arrays as they are (a verifier's input: nothing is checked here)."""

    def __init__(self, addresses, values, siblings, counts=None):
        self.addresses = np.ascontiguousarray(addresses, dtype=np.uint32).reshape(-1)
        self.values = np.ascontiguousarray(values, dtype=np.uint32).reshape(-1, 4)
        self.siblings = np.ascontiguousarray(siblings, dtype=np.uint32).reshape(-1)
        self.counts = None if counts is None else [int(c) for c in counts]

    @property
    def nbytes(self):
        """what travels: addresses, values and sibling words"""
        return 20 * self.addresses.size + 4 * self.siblings.size

    def __repr__(self):
        return f"MemSetOpening(n={self.addresses.size}, n_siblings={self.siblings.size})"


def _set_addresses(addresses):
    a = np.array(addresses, dtype=np.uint64).reshape(-1)
    if a.size and int(a.max()) >= 1 << 32:
        raise ValueError("an address does not fit 32 bits")
    return np.ascontiguousarray(a.astype(np.uint32))


def mem_set_plan(addresses, lib=None):
    """cm_mem_set_plan of strictly ascending addresses: ([one dict per hashing step: depth, n_nodes, n_siblings, kernel (a
    SET_KERNELS name)], the record's sibling words in all).  Host code: needs no GPU."""
    L = lib or load_library()
    a = _set_addresses(addresses)
    steps = (MemSetStep * 29)()
    k, m = C.c_uint32(0), C.c_uint32(0)
    rc = L.cm_mem_set_plan(_p(a), C.c_uint64(a.size), steps, C.c_uint32(29), C.byref(k), C.byref(m))
    if rc:
        raise _lib_error(L, rc)
    return [{"depth": s.depth, "n_nodes": s.n_nodes, "n_siblings": s.n_siblings, "kernel": SET_KERNELS[s.kernel]} for s in steps[:k.value]], m.value


def _set_call(L, fn, head, addresses):
    """any order, any repeats: sorted and made unique here (the C ABI takes strictly ascending addresses only)"""
    a = np.unique(_set_addresses(addresses))
    plan, m = mem_set_plan(a, L)                                                  # (refuses what the call would refuse)
    values, siblings = np.zeros((a.size, 4), dtype=np.uint32), np.zeros(max(m, 1), dtype=np.uint32)
    need, root = C.c_uint32(0), C.c_uint32(0)
    rc = fn(*head, _p(a), C.c_uint64(a.size), _p(values), _p(siblings), C.c_uint32(m), C.byref(need), C.byref(root))
    if rc:
        raise _lib_error(L, rc)
    return MemSetOpening(a, values, siblings[:need.value], [s["n_siblings"] for s in plan[1:]]), root.value


def _backend_open_memory_set(self, dev_input, which, addresses):
    """cm_input_open_memory_set: the cells `addresses` (any order, repeats allowed) under the input's initial (which = 0) or
    final (1) tree, built on the GPU -> (MemSetOpening, root)."""
    return _set_call(self.L, self.L.cm_input_open_memory_set, (dev_input, C.c_uint32(which)), addresses)


def _run_open_set(self, addresses):
    """cm_run_open_memory_set: a set of cells under the root of the image as it is now -> (MemSetOpening, root).  Shares the
    cached image tree of Run.open and Run.open_range."""
    return _set_call(self.L, self.L.cm_run_open_memory_set, (self.h,), addresses)


def _set_args(opening, values=None):
    a, s = opening.addresses, opening.siblings
    v = opening.values if values is None else np.ascontiguousarray(values, dtype=np.uint32)
    if v.size != 4 * a.size:
        raise ValueError(f"{v.size} value words for a set of {a.size} cells")
    pad = lambda x: x if x.size else np.zeros(4, dtype=np.uint32)                 # (an empty array still has to be an address)
    return (_p(pad(a)), C.c_uint64(a.size), _p(pad(v.reshape(-1))), _p(pad(s)), C.c_uint32(s.size)), (a, v, s)


def verify_set(root, opening, lib=None, stream=0, with_root=False):
    """cm_verify_memory_set (GPU) -> bool: addresses, values and sibling words are well formed and fold to `root`; with_root:
    (bool, the root they fold to, 0 when malformed)."""
    L = lib or load_library()
    args, keep = _set_args(opening)
    ok, got = C.c_uint8(0), C.c_uint32(0)
    rc = L.cm_verify_memory_set(C.c_uint32(root), *args, C.byref(ok), C.byref(got), C.c_uint64(stream))
    if rc:
        raise _lib_error(L, rc)
    return (bool(ok.value), got.value) if with_root else bool(ok.value)


def verify_set_host(root, opening, lib=None):
    """cm_verify_memory_set_host (host code, no GPU) -> (status, message): (0, "") accepted, (11, why) rejected."""
    L = lib or load_library()
    args, keep = _set_args(opening)
    rc = L.cm_verify_memory_set_host(C.c_uint32(root), *args)
    if not rc:
        return 0, ""
    buf = C.create_string_buffer(512)
    L.cm_last_error(buf, C.c_size_t(512))
    return rc, buf.value.decode(errors="replace")


def set_root(opening, values=None, lib=None):
    """cm_memory_set_root_host (host code, no GPU): the root the record folds to with its own values or with `values` in their
    place — the root AFTER a write that touched only cells of the set, from the sibling words opened BEFORE it."""
    L = lib or load_library()
    args, keep = _set_args(opening, values)
    got = C.c_uint32(0)
    rc = L.cm_memory_set_root_host(*args, C.byref(got))
    if rc:
        raise _lib_error(L, rc)
    return got.value


Backend.open_memory_set = _backend_open_memory_set
Backend.verify_set = lambda self, root, opening, stream=0, with_root=False: verify_set(root, opening, self.L, stream, with_root)
Run.open_set = _run_open_set


# ---- memory transitions (include/cairom_hip.h: cm_input_write_set .. cm_prove_run_transitions) ----------------------------------
class MemTransitionViewC(C.Structure):
    """cm_mem_transition_view"""
    _fields_ = [(n, C.c_uint32) for n in ("struct_size", "root_before", "root_after", "n", "n_siblings", "n_zero_only")] + \
               [(n, _u32p) for n in ("addresses", "old_values", "new_values", "siblings")]


class MemTransition:
    """A set of cells with their values under two roots and one list of sibling words (a set opening's): `old_values` fold to
    `root_before`, `new_values` to `root_after`, so the two memories agree outside `addresses`."""

    def __init__(self, addresses, old_values, new_values, siblings, root_before, root_after, n_zero_only=0):
        self.addresses = np.ascontiguousarray(addresses, dtype=np.uint32).reshape(-1)
        self.old_values = np.ascontiguousarray(old_values, dtype=np.uint32).reshape(-1, 4)
        self.new_values = np.ascontiguousarray(new_values, dtype=np.uint32).reshape(-1, 4)
        self.siblings = np.ascontiguousarray(siblings, dtype=np.uint32).reshape(-1)
        self.root_before, self.root_after, self.n_zero_only = int(root_before), int(root_after), int(n_zero_only)

    @property
    def nbytes(self):
        """what travels: addresses, old and new values, sibling words"""
        return 36 * self.addresses.size + 4 * self.siblings.size

    def updates(self):
        """[(address, (v0, v1, v2, v3))]: what a follower writes into its copy of the memory"""
        return [(int(a), tuple(int(x) for x in v)) for a, v in zip(self.addresses, self.new_values)]

    def __repr__(self):
        return f"MemTransition(n={self.addresses.size}, n_siblings={self.siblings.size}, {self.root_before} -> {self.root_after})"


def _take_transition(L, h):
    """the arrays of a cm_mem_transition, copied; the handle is freed"""
    v = MemTransitionViewC()
    v.struct_size = C.sizeof(MemTransitionViewC)
    try:
        rc = L.cm_mem_transition_get(h, C.byref(v))
        if rc:
            raise _lib_error(L, rc)
        take = lambda p, k: np.ctypeslib.as_array(p, shape=(k,)).copy() if k else np.zeros(0, dtype=np.uint32)
        return MemTransition(take(v.addresses, v.n), take(v.old_values, 4 * v.n), take(v.new_values, 4 * v.n), take(v.siblings, v.n_siblings),
                             v.root_before, v.root_after, v.n_zero_only)
    finally:
        L.cm_mem_transition_free(h)


def _backend_write_set(self, dev_input, cap=None, with_counts=False):
    """cm_input_write_set (GPU): the ascending addresses of the cells whose value differs between the input's initial and final
    boundary memory; with_counts: (addresses, n_total, n_zero_only).  cap: room for that many (the rest is counted, not listed)."""
    n, z = C.c_uint64(0), C.c_uint64(0)
    if cap is None:
        self._ck(self.L.cm_input_write_set(dev_input, None, C.c_uint64(0), C.byref(n), C.byref(z)))
        cap = n.value
    a = np.zeros(max(cap, 1), dtype=np.uint32)
    self._ck(self.L.cm_input_write_set(dev_input, _p(a), C.c_uint64(cap), C.byref(n), C.byref(z)))
    a = a[:min(cap, n.value)].copy()
    return (a, n.value, z.value) if with_counts else a


def _backend_open_transition(self, dev_input, addresses=None):
    """cm_input_open_transition (GPU) -> MemTransition of the input from its initial to its final tree: over the segment's write
    set, or over `addresses` (any order, repeats allowed), which must hold every cell the segment changes."""
    h = C.c_void_p()
    if addresses is None:
        self._ck(self.L.cm_input_open_transition(dev_input, None, C.c_uint64(0), C.byref(h)))
    else:
        a = np.unique(_set_addresses(addresses))
        pad = a if a.size else np.zeros(1, dtype=np.uint32)
        self._ck(self.L.cm_input_open_transition(dev_input, _p(pad), C.c_uint64(a.size), C.byref(h)))
    return _take_transition(self.L, h)


def _transition_args(t):
    a, s = t.addresses, t.siblings
    old, new = t.old_values.reshape(-1), t.new_values.reshape(-1)
    if old.size != 4 * a.size or new.size != 4 * a.size:
        raise ValueError(f"{old.size} old and {new.size} new value words for a transition of {a.size} cells")
    pad = lambda x: x if x.size else np.zeros(4, dtype=np.uint32)                 # (an empty array still has to be an address)
    keep = (pad(a), pad(old), pad(new), pad(s))
    return (C.c_uint32(t.root_before), C.c_uint32(t.root_after), _p(keep[0]), C.c_uint64(a.size), _p(keep[1]), _p(keep[2]), _p(keep[3]),
            C.c_uint32(s.size)), keep


def verify_transition(t, lib=None, stream=0, with_roots=False):
    """cm_verify_memory_transition (GPU) -> bool: the transition is well formed, its old values fold to root_before and its new
    values to root_after; with_roots: (bool, (the two roots they fold to, zeros when malformed))."""
    L = lib or load_library()
    args, keep = _transition_args(t)
    ok, got = C.c_uint8(0), (C.c_uint32 * 2)()
    rc = L.cm_verify_memory_transition(*args, C.byref(ok), got, C.c_uint64(stream))
    if rc:
        raise _lib_error(L, rc)
    return (bool(ok.value), (got[0], got[1])) if with_roots else bool(ok.value)


def verify_transition_host(t, lib=None):
    """cm_verify_memory_transition_host (host code, no GPU) -> (status, message): (0, "") accepted, (11, why) rejected."""
    L = lib or load_library()
    args, keep = _transition_args(t)
    rc = L.cm_verify_memory_transition_host(*args)
    if not rc:
        return 0, ""
    buf = C.create_string_buffer(512)
    L.cm_last_error(buf, C.c_size_t(512))
    return rc, buf.value.decode(errors="replace")


def _roots_fit(who, i, proof, t):
    d = proof.public_data()
    for side, want in (("before", d["initial_root"]), ("after", d["final_root"])):
        got = getattr(t, "root_" + side)
        if got != want:
            raise CmError(f"{who}segment {i}: the transition's root {side} is {got}, the proof's is {want}")


def follow_run(proofs, transitions, lib=None, device=True, batched=False):
    """What a client that holds only the proofs' roots does with a run's transitions: transition i must go from proof i's public
    initial_root to its final_root and must verify (device=True: on the GPU, else in host code).  Returns the updates
    [(address, new value)] in run order; raises CmError naming the first segment whose transition does not fit.
    batched=True (GPU only): the same root checks, in order, up to the first segment whose roots do not fit; ONE
    verify_transitions over the segments in front of it; the same CmError for the first segment that fails either way."""
    L = lib or proofs[0].L
    if len(proofs) != len(transitions):
        raise CmError(f"follow_run: {len(transitions)} transitions for {len(proofs)} proofs")
    if batched:
        if not device:
            raise CmError("follow_run: batched=True verifies on the GPU (device=True)")
        misfit, fit = None, 0
        for i, (p, t) in enumerate(zip(proofs, transitions)):
            try:
                _roots_fit("follow_run: ", i, p, t)
            except CmError as e:
                misfit = e
                break
            fit += 1
        oks = verify_transitions(transitions[:fit], L) if fit else []
        if not all(oks):
            raise CmError(f"follow_run: segment {oks.index(False)}: the transition does not verify on the GPU")
        if misfit:
            raise misfit
        return [u for t in transitions for u in t.updates()]
    out = []
    for i, (p, t) in enumerate(zip(proofs, transitions)):
        d = p.public_data()
        for side, want in (("before", d["initial_root"]), ("after", d["final_root"])):
            got = getattr(t, "root_" + side)
            if got != want:
                raise CmError(f"follow_run: segment {i}: the transition's root {side} is {got}, the proof's is {want}")
        if device:
            ok, why = verify_transition(t, L), "the transition does not verify on the GPU"
        else:
            rc, why = verify_transition_host(t, L)
            ok = rc == 0
        if not ok:
            raise CmError(f"follow_run: segment {i}: {why}")
        out += t.updates()
    return out


def _transition_view(t):
    """(a filled cm_mem_transition_view over t's arrays, the arrays to keep alive)"""
    a, s = t.addresses, t.siblings
    old, new = t.old_values.reshape(-1), t.new_values.reshape(-1)
    if old.size != 4 * a.size or new.size != 4 * a.size:
        raise ValueError(f"{old.size} old and {new.size} new value words for a transition of {a.size} cells")
    v = MemTransitionViewC()
    v.struct_size = C.sizeof(MemTransitionViewC)
    v.root_before, v.root_after, v.n, v.n_siblings, v.n_zero_only = t.root_before, t.root_after, a.size, s.size, t.n_zero_only
    for name, x in (("addresses", a), ("old_values", old), ("new_values", new), ("siblings", s)):
        if x.size:
            setattr(v, name, _p(x))
    return v, (a, old, new, s)


def compose_transitions(transitions, lib=None, device=True):
    """cm_compose_transitions -> MemTransition: the chain transitions[0] -> ... -> transitions[-1] as ONE transition from the first
    root before to the last root after over the union of their cells, from the records alone (device=True: on the GPU, else in
    host code; the same bytes).  Nothing is hashed: the result is valid if every part is and the roots chain.  Raises CmError
    (with .status and .message) for input that is detectably broken."""
    L = lib or load_library()
    transitions = list(transitions)
    views = (MemTransitionViewC * max(len(transitions), 1))()
    keep = []
    for i, t in enumerate(transitions):
        views[i], k = _transition_view(t)
        keep.append(k)
    h = C.c_void_p()
    rc = L.cm_compose_transitions(views, C.c_uint32(len(transitions)), C.c_uint32(1 if device else 0), C.byref(h))
    if rc:
        err = _lib_error(L, rc)
        err.status, err.message = rc, str(err).split(": ", 1)[1]
        raise err
    return _take_transition(L, h)


def run_transition(proofs, transitions, lib=None, device=True):
    """What a client that wants only the run's first and last memory does with a run's transitions: compose them into one, require
    its roots to be proof 0's initial_root and the last proof's final_root, and verify it (device=True: composed and verified on
    the GPU, else in host code).  Returns the composed MemTransition; raises CmError saying which of the three failed."""
    L = lib or proofs[0].L
    try:
        t = compose_transitions(transitions, L, device)
    except CmError as e:
        raise CmError(f"run_transition: the transitions do not compose: {e}") from e
    for side, want in (("before", proofs[0].public_data()["initial_root"]), ("after", proofs[-1].public_data()["final_root"])):
        got = getattr(t, "root_" + side)
        if got != want:
            which = "first proof's initial_root" if side == "before" else "last proof's final_root"
            raise CmError(f"run_transition: the composed transition's root {side} is {got}, the {which} is {want}")
    if device:
        ok, why = verify_transition(t, L), "the composed transition does not verify on the GPU"
    else:
        rc, why = verify_transition_host(t, L)
        ok = rc == 0
    if not ok:
        raise CmError(f"run_transition: {why}")
    return t


# ---- batched verification of transitions and sets (include/cairom_hip.h: cm_verify_memory_transitions .. cm_mem_batch_plan) -----
class MemSetViewC(C.Structure):
    """cm_mem_set_view"""
    _fields_ = [(n, C.c_uint32) for n in ("struct_size", "root", "n", "n_siblings")] + [(n, _u32p) for n in ("addresses", "values", "siblings")]


class MemBatchStep(C.Structure):
    """cm_mem_batch_step: one hashing step of a batch (cm_mem_batch_plan)."""
    _fields_ = [("depth", C.c_uint32), ("n_nodes", C.c_uint32), ("widest_part", C.c_uint32), ("kernel", C.c_uint32)]


def _set_view(root, opening):
    """(a filled cm_mem_set_view over the opening's arrays, the arrays to keep alive)"""
    a, s, v = opening.addresses, opening.siblings, opening.values.reshape(-1)
    if v.size != 4 * a.size:
        raise ValueError(f"{v.size} value words for a set of {a.size} cells")
    view = MemSetViewC()
    view.struct_size = C.sizeof(MemSetViewC)
    view.root, view.n, view.n_siblings = int(root), a.size, s.size
    for name, x in (("addresses", a), ("values", v), ("siblings", s)):
        if x.size:
            setattr(view, name, _p(x))
    return view, (a, v, s)


def _verify_batch(L, fn, views, n, planes, stream):
    ok, got = (C.c_uint8 * max(n, 1))(), (C.c_uint32 * max(planes * n, 1))()
    rc = fn(views, C.c_uint32(n), ok, got, C.c_uint64(stream))
    if rc:
        _raise_status(L, rc)
    return [bool(x) for x in ok[:n]], list(got[:planes * n])


def verify_transitions(ts, lib=None, stream=0, with_roots=False):
    """cm_verify_memory_transitions (GPU) -> [bool]: verify_transition of every MemTransition of `ts`, in one batch whose number of
    launches does not depend on len(ts); with_roots: [(bool, (the two roots it folds to, zeros when malformed))].  A malformed
    part is a verdict and does not disturb the others; CmError (.status, .message) only for what the call itself refuses."""
    L = lib or load_library()
    ts = list(ts)
    views = (MemTransitionViewC * max(len(ts), 1))()
    keep = []
    for i, t in enumerate(ts):
        views[i], k = _transition_view(t)
        keep.append(k)
    ok, got = _verify_batch(L, L.cm_verify_memory_transitions, views, len(ts), 2, stream)
    return [(o, (got[2 * i], got[2 * i + 1])) for i, o in enumerate(ok)] if with_roots else ok


def verify_sets(roots, openings, lib=None, stream=0, with_roots=False):
    """cm_verify_memory_sets (GPU) -> [bool]: verify_set(roots[i], openings[i]) for every i in one batch; with_roots: [(bool, the
    root it folds to, 0 when malformed)].  `roots` may be one root for all."""
    L = lib or load_library()
    openings = list(openings)
    roots = [int(roots)] * len(openings) if np.isscalar(roots) else [int(r) for r in roots]
    if len(roots) != len(openings):
        raise ValueError(f"{len(roots)} roots for {len(openings)} sets")
    views = (MemSetViewC * max(len(openings), 1))()
    keep = []
    for i, (r, o) in enumerate(zip(roots, openings)):
        views[i], k = _set_view(r, o)
        keep.append(k)
    ok, got = _verify_batch(L, L.cm_verify_memory_sets, views, len(openings), 1, stream)
    return list(zip(ok, got)) if with_roots else ok


def mem_batch_plan(address_lists, lib=None):
    """cm_mem_batch_plan of the parts' strictly ascending address lists: [one dict per hashing step of the batch: depth, n_nodes (of
    all parts together), widest_part, kernel (a SET_KERNELS name)]; [] when no part reaches the device.  Consecutive tail steps
    are one launch.  Host code: needs no GPU."""
    L = lib or load_library()
    lists = [_set_addresses(a) for a in address_lists]
    ptrs = (_u32p * max(len(lists), 1))()
    for i, a in enumerate(lists):
        if a.size:
            ptrs[i] = _p(a)
    n = np.array([a.size for a in lists] or [0], dtype=np.uint32)
    steps, k = (MemBatchStep * 29)(), C.c_uint32(0)
    rc = L.cm_mem_batch_plan(ptrs, _p(n), C.c_uint32(len(lists)), steps, C.c_uint32(29), C.byref(k))
    if rc:
        _raise_status(L, rc)
    return [{"depth": s.depth, "n_nodes": s.n_nodes, "widest_part": s.widest_part, "kernel": SET_KERNELS[s.kernel]} for s in steps[:k.value]]


def mem_batch_launches(plan):
    """the hashing launches of a mem_batch_plan: the cells, one per level step, one tail"""
    kinds = [s["kernel"] for s in plan]
    return kinds.count("cells") + kinds.count("level") + (1 if "tail" in kinds else 0)


Backend.write_set = _backend_write_set
Backend.open_transition = _backend_open_transition
Backend.verify_transitions = lambda self, ts, stream=0, with_roots=False: verify_transitions(ts, self.L, stream, with_roots)
Backend.verify_sets = lambda self, roots, openings, stream=0, with_roots=False: verify_sets(roots, openings, self.L, stream, with_roots)
Backend.mem_batch_plan = lambda self, address_lists: mem_batch_plan(address_lists, self.L)
Backend.verify_transition = lambda self, t, stream=0, with_roots=False: verify_transition(t, self.L, stream, with_roots)
Backend.compose_transitions = lambda self, transitions, device=True: compose_transitions(transitions, self.L, device)


# ---- followed memory (include/cairom_hip.h: cm_mem_image_create .. cm_mem_image_open_memory_set) --------------------------------
class MemImageStatsC(C.Structure):
    """cm_mem_image_stats"""
    _fields_ = [("struct_size", C.c_uint32), ("device", C.c_uint32), ("n_cells", C.c_uint64), ("n_nodes", C.c_uint64), ("bytes", C.c_uint64)]


def _raise_status(L, rc):
    """CmError with .status and .message (the text behind "libcairom_hip status <rc>: ")"""
    err = _lib_error(L, rc)
    err.status, err.message = rc, str(err).split(": ", 1)[1]
    raise err


def _cell_values(values, n):
    v = np.ascontiguousarray(values, dtype=np.uint32).reshape(-1)
    if v.size != 4 * n:
        raise ValueError(f"{v.size} value words for {n} cells")
    return v if v.size else np.zeros(4, dtype=np.uint32)


def _bare(self):
    """A copy without sibling words: addresses, both value planes and the two roots, all a holder of the tree needs
    (MemImage.apply_transition never reads the words)."""
    return MemTransition(self.addresses.copy(), self.old_values.copy(), self.new_values.copy(), np.zeros(0, dtype=np.uint32), self.root_before,
                         self.root_after, self.n_zero_only)


MemTransition.bare = _bare
MemTransition.nbytes_bare = property(lambda self: 20 * self.addresses.size, doc="what a follower needs: addresses and new values")


class MemImage:
    """cm_mem_image: a memory image with its partial Merkle tree, on the GPU (device=True) or in host memory, independent of any
    prover handle.  It absorbs updates by re-hashing only the dirty paths, checks itself against the roots it is given and opens
    cells under its current root.  A refused update raises CmError (.status, .message) and leaves the image as it was."""

    def __init__(self, lib, handle, device):
        self.L, self.h, self.device = lib, handle, bool(device)

    @classmethod
    def from_cells(cls, cells, lib=None, device=True):
        """cells: [(address, v0, v1, v2, v3)] in any order, addresses distinct"""
        L = lib or load_library()
        c = np.array(sorted(tuple(int(x) for x in r) for r in cells), dtype=np.uint64).reshape(-1, 5)
        if c.size and int(c.max()) >= 1 << 32:
            raise ValueError("a word does not fit 32 bits")
        a = np.ascontiguousarray(c[:, 0].astype(np.uint32))
        v = np.ascontiguousarray(c[:, 1:].astype(np.uint32)).reshape(-1)
        pad = lambda x: x if x.size else np.zeros(4, dtype=np.uint32)
        h = C.c_void_p()
        rc = L.cm_mem_image_create(_p(pad(a)), _p(pad(v)), C.c_uint64(a.size), C.c_uint32(1 if device else 0), C.byref(h))
        if rc:
            _raise_status(L, rc)
        return cls(L, h, device)

    @classmethod
    def from_run(cls, run, device=True):
        """the image of a Run as it is now (Run.memory()): locals dense from 0, heap cell i at 2^28 - 1 - i"""
        lo, hi = run.memory()
        cells = [(a,) + tuple(int(x) for x in lo[a]) for a in range(lo.shape[0])]
        cells += [(ADDRESS_SPACE - 1 - i,) + tuple(int(x) for x in hi[i]) for i in range(hi.shape[0])]
        return cls.from_cells(cells, run.L, device)

    def _ck(self, rc):
        if rc:
            _raise_status(self.L, rc)

    @property
    def root(self):
        r = C.c_uint32(0)
        self._ck(self.L.cm_mem_image_root(self.h, C.byref(r)))
        return r.value

    def stats(self):
        """{"device", "n_cells", "n_nodes", "bytes"}"""
        s = MemImageStatsC()
        s.struct_size = C.sizeof(MemImageStatsC)
        self._ck(self.L.cm_mem_image_stats_get(self.h, C.byref(s)))
        return {"device": bool(s.device), "n_cells": s.n_cells, "n_nodes": s.n_nodes, "bytes": s.bytes}

    @property
    def n_cells(self):
        return self.stats()["n_cells"]

    def read(self, addresses):
        """values (n, 4) of `addresses`, any order, repeats allowed; an absent cell reads as zeros"""
        a = _set_addresses(addresses)
        v = np.zeros((a.size, 4), dtype=np.uint32)
        if a.size:
            self._ck(self.L.cm_mem_image_read(self.h, _p(a), C.c_uint64(a.size), _p(v)))
        return v

    def cells(self):
        """(addresses ascending, values (n, 4)) of every cell the image holds"""
        n = self.n_cells
        a, v, total = np.zeros(max(n, 1), dtype=np.uint32), np.zeros((max(n, 1), 4), dtype=np.uint32), C.c_uint64(0)
        self._ck(self.L.cm_mem_image_cells(self.h, _p(a), _p(v), C.c_uint64(n), C.byref(total)))
        return a[:n].copy(), v[:n].copy()

    def nodes(self):
        """the node list (n, 8): index, depth, left, right, parent and three multiplicity words that enter no hash"""
        n = self.stats()["n_nodes"]
        out, total = np.zeros((max(n, 1), 8), dtype=np.uint32), C.c_uint64(0)
        self._ck(self.L.cm_mem_image_nodes(self.h, out.ctypes.data_as(C.c_void_p), C.c_uint64(n), C.byref(total)))
        return out[:n].copy()

    def apply(self, addresses, new_values, old_values=None, root_before=None, root_after=None, record=False):
        """cm_mem_image_apply: write new_values (n, 4) to the strictly ascending `addresses`.  old_values, root_before and
        root_after are checked when given.  Returns the new root, or (root, MemTransition) with record=True: the full transition
        over the addresses, its old values and sibling words read from the tree before the update."""
        a = _set_addresses(addresses)
        nv = _cell_values(new_values, a.size)
        ov = None if old_values is None else _cell_values(old_values, a.size)
        word = lambda x: None if x is None else C.byref(C.c_uint32(int(x)))
        root, h = C.c_uint32(0), C.c_void_p()
        pad = a if a.size else np.zeros(1, dtype=np.uint32)
        self._ck(self.L.cm_mem_image_apply(self.h, _p(pad), _p(nv), C.c_uint64(a.size), None if ov is None else _p(ov), word(root_before),
                                           word(root_after), C.byref(root), C.byref(h) if record else None))
        return (root.value, _take_transition(self.L, h)) if record else root.value

    def apply_transition(self, t, record=False):
        """cm_mem_image_apply_transition: apply with t's addresses, both value planes and both roots; t's sibling words are never
        read (MemTransition.bare()).  Returns the new root, or (root, the full MemTransition) with record=True."""
        view, keep = _transition_view(t)
        h = C.c_void_p()
        self._ck(self.L.cm_mem_image_apply_transition(self.h, C.byref(view), C.byref(h) if record else None))
        return (self.root, _take_transition(self.L, h)) if record else self.root

    def open(self, addresses):
        """cm_mem_image_open_memory -> ([MemOpening], root): under the image's current root (device images)"""
        return _open_call(self.L, self.L.cm_mem_image_open_memory, (self.h,), addresses)

    def open_range(self, start, n):
        """cm_mem_image_open_memory_range -> (MemRangeOpening, values (n, 4), root)"""
        return _range_call(self.L, self.L.cm_mem_image_open_memory_range, (self.h,), start, n)

    def open_set(self, addresses):
        """cm_mem_image_open_memory_set -> (MemSetOpening, root); any order, repeats allowed"""
        return _set_call(self.L, self.L.cm_mem_image_open_memory_set, (self.h,), addresses)

    def free(self):
        if self.h:
            self.L.cm_mem_image_free(self.h)
            self.h = None


def follow_run_image(proofs, updates, image, batched=False):
    """What a follower that keeps its own copy of the memory does with a run: update i — a MemTransition, bare or full, or an
    (addresses, new_values) pair — is applied to `image` from proof i's public initial_root to its final_root.  Raises CmError
    naming the first segment that does not fit; the image then stays at the last good segment.  Returns the image's root.
    batched=True: every update is a full MemTransition.  The records of the segments in front of the first whose roots do not fit
    are screened by ONE verify_transitions before the image is touched, and the segments in front of the first failure are
    applied as usual.  That segment then goes to the image like any other, so what it refuses is refused in its own words; a
    record the image takes (it never reads the sibling words, and checks the values against both roots itself) is still an
    error here: "the transition does not verify on the GPU"."""
    if len(proofs) != len(updates):
        raise CmError(f"follow_run_image: {len(updates)} updates for {len(proofs)} proofs")
    screened = None
    if batched:
        if not all(isinstance(u, MemTransition) for u in updates):
            raise CmError("follow_run_image: batched=True takes full MemTransitions only")
        fit = 0
        for i, (p, u) in enumerate(zip(proofs, updates)):
            try:
                _roots_fit("", i, p, u)
            except CmError:
                break
            fit += 1
        oks = verify_transitions(updates[:fit], image.L) if fit else []
        screened = oks.index(False) if not all(oks) else None
    for i, (p, u) in enumerate(zip(proofs, updates)):
        d = p.public_data()
        try:
            if i == screened:
                image.apply_transition(u)
                raise CmError("the transition does not verify on the GPU")
            if isinstance(u, MemTransition):
                for side, want in (("before", d["initial_root"]), ("after", d["final_root"])):
                    if getattr(u, "root_" + side) != want:
                        raise CmError(f"the transition's root {side} is {getattr(u, 'root_' + side)}, the proof's is {want}")
                image.apply_transition(u)
            elif len(u[0]):
                image.apply(u[0], u[1], root_before=d["initial_root"], root_after=d["final_root"])
            else:
                image.apply_transition(MemTransition([], [], [], [], d["initial_root"], d["final_root"]))
        except CmError as e:
            raise CmError(f"follow_run_image: segment {i}: {getattr(e, 'message', e)}") from e
    return image.root


# ---- batched image updates (include/cairom_hip.h: cm_mem_images_apply) ----------------------------------------------------------
class MemImageUpdateC(C.Structure):
    """cm_mem_image_update"""
    _fields_ = [("struct_size", C.c_uint32), ("n", C.c_uint32), ("img", C.c_void_p)] + \
               [(n, _u32p) for n in ("addresses", "new_values", "old_values", "root_before", "root_after")]


class MemImageResultC(C.Structure):
    """cm_mem_image_result"""
    _fields_ = [("status", C.c_int32), ("root", C.c_uint32), ("message", C.c_char * 248)]


def _image_update(u):
    """(image, addresses, new_values, old_values | None, root_before | None, root_after | None) of one entry of apply_images"""
    if len(u) == 2 and isinstance(u[1], MemTransition):
        t = u[1]
        return u[0], t.addresses, t.new_values, t.old_values, t.root_before, t.root_after
    image, a, nv, ov, rb, ra = tuple(u) + (None,) * (6 - len(u))
    return image, a, nv, ov, rb, ra


def apply_images(updates, lib=None, with_rc=False):
    """cm_mem_images_apply: one update each to DIFFERENT device images in one call, through one ladder of launches.  updates:
    [(image, MemTransition)] or [(image, addresses, new_values[, old_values, root_before, root_after])].  Returns one
    (status, root, message) per part: what MemImage.apply would have done with that part alone — 0 and the new root, or the
    refusal's status and words with the image as it was; a refused part does not disturb the others.  Raises CmError (.status,
    .message) only when the call as a whole is refused.  with_rc: (the call's return value — 0, or the status of the lowest part
    that has another, which cm_last_error() then names — and the list).  The batch makes no record: MemImage.apply(record=True)
    does."""
    ups = [_image_update(u) for u in updates]
    L = lib or (ups[0][0].L if ups else load_library())
    n = len(ups)
    parts, res, keep = (MemImageUpdateC * max(n, 1))(), (MemImageResultC * max(n, 1))(), []
    word = lambda x: None if x is None else C.pointer(C.c_uint32(int(x)))
    for p, (image, a, nv, ov, rb, ra) in zip(parts, ups):
        a = _set_addresses(a)
        nv = _cell_values(nv, a.size)
        ov = None if ov is None else _cell_values(ov, a.size)
        pad = a if a.size else np.zeros(1, dtype=np.uint32)
        words = (word(rb), word(ra))
        keep.append((pad, nv, ov, words))
        p.struct_size, p.n, p.img = C.sizeof(MemImageUpdateC), a.size, image.h
        p.addresses, p.new_values = _p(pad), _p(nv)
        if ov is not None:
            p.old_values = _p(ov)
        if words[0]:
            p.root_before = words[0]
        if words[1]:
            p.root_after = words[1]
    for r in res:
        r.status = -1                                                             # (a call refused as a whole writes no result)
    rc = L.cm_mem_images_apply(parts, C.c_uint32(n), res)
    judged = n > 0 and all(r.status != -1 for r in res[:n])
    out = [(r.status, r.root, r.message.decode(errors="replace")) for r in res[:n]] if judged else None
    if rc and (not judged or all(r.status != rc for r in res[:n]) or rc in (2, 3)):
        try:
            _raise_status(L, rc)
        except CmError as e:
            e.results = out                                                       # (without a GPU: the host's own verdicts)
            raise
    return (rc, out) if with_rc else out


def follow_runs_images(runs):
    """follow_run_image for many runs at once.  runs: [(proofs, updates, image)], the images different device images.  Round j
    applies segment j of every run that is still alive in ONE apply_images, from proof j's public initial_root to its final_root
    (a MemTransition's own roots are first held against the proof's, as follow_run_image does; an update without cells changes
    nothing and goes through the single call, which still checks the roots).  A run stops at its first refusal, its image at the
    last good segment, and the others go on.  Returns per run (root, None) or (root, "segment <j>: <message>")."""
    runs = [(list(p), list(u), im) for p, u, im in runs]
    for p, u, _ in runs:
        if len(p) != len(u):
            raise CmError(f"follow_runs_images: {len(u)} updates for {len(p)} proofs")
    said = [None] * len(runs)
    for j in range(max((len(p) for p, _, _ in runs), default=0)):
        batch, who = [], []
        for r, (proofs, updates, image) in enumerate(runs):
            if said[r] is not None or j >= len(proofs):
                continue
            d, u = proofs[j].public_data(), updates[j]
            try:
                if isinstance(u, MemTransition):
                    for side, want in (("before", d["initial_root"]), ("after", d["final_root"])):
                        if getattr(u, "root_" + side) != want:
                            raise CmError(f"the transition's root {side} is {getattr(u, 'root_' + side)}, the proof's is {want}")
                    a, nv, ov = u.addresses, u.new_values, u.old_values
                else:
                    a, nv, ov = u[0], u[1], None
                if len(a):
                    batch.append((image, a, nv, ov, d["initial_root"], d["final_root"]))
                    who.append(r)
                else:
                    image.apply_transition(MemTransition([], [], [], [], d["initial_root"], d["final_root"]))
            except CmError as e:
                said[r] = f"segment {j}: {getattr(e, 'message', e)}"
        if batch:
            for r, (status, _, message) in zip(who, apply_images(batch, runs[who[0]][2].L)):
                if status:
                    said[r] = f"segment {j}: {message}"
    return [(image.root, said[r]) for r, (_, _, image) in enumerate(runs)]


# ---- batched set openings (include/cairom_hip.h: cm_mem_images_open_memory_sets) -------------------------------------------------
class MemSetRequestC(C.Structure):
    """cm_mem_set_request"""
    _fields_ = [("struct_size", C.c_uint32), ("n", C.c_uint32), ("img", C.c_void_p), ("addresses", _u32p), ("values", _u32p), ("siblings", _u32p),
                ("cap_siblings", C.c_uint32), ("reserved", C.c_uint32)]


class MemSetResultC(C.Structure):
    """cm_mem_set_result"""
    _fields_ = [("status", C.c_int32), ("root", C.c_uint32), ("n_siblings", C.c_uint32), ("reserved", C.c_uint32), ("message", C.c_char * 240)]


def open_sets(requests, lib=None, with_rc=False):
    """cm_mem_images_open_memory_sets: many sets under device images in one call, through one chain of launches and one round trip.
    requests: [(image, addresses)]; several may name one image; the addresses in any order, repeats allowed (sorted and made
    unique here, per part, as MemImage.open_set does).  Returns one (status, message, MemSetOpening or None, root) per part: what
    MemImage.open_set would have done with that part alone — 0, "", the record and the root it opens under, or the refusal's status
    and words and no record; a bad part does not disturb the others.  Raises CmError (.status, .message) only when the call as a
    whole is refused or has no device (.results then holds the host's own verdicts).  with_rc: (the call's return value — 0, or
    the status of the lowest part that has another, which cm_last_error() then names — and the list)."""
    reqs = [(image, np.unique(_set_addresses(a))) for image, a in requests]
    L = lib or (reqs[0][0].L if reqs else load_library())
    n = len(reqs)
    parts, res, keep = (MemSetRequestC * max(n, 1))(), (MemSetResultC * max(n, 1))(), []
    for p, (image, a) in zip(parts, reqs):
        try:
            plan, m = mem_set_plan(a, L)
        except CmError:
            plan, m = [], 0                                                       # (no cells, an address beyond 2^28: the part's own refusal)
        values, siblings = np.zeros((max(a.size, 1), 4), dtype=np.uint32), np.zeros(max(m, 1), dtype=np.uint32)
        pad = a if a.size else np.zeros(1, dtype=np.uint32)
        keep.append((pad, values, siblings, [s["n_siblings"] for s in plan[1:]]))
        p.struct_size, p.n, p.img, p.cap_siblings = C.sizeof(MemSetRequestC), a.size, image.h, m
        p.addresses, p.values, p.siblings = _p(pad), _p(values), _p(siblings)
    for r in res:
        r.status = -1                                                             # (a call refused as a whole writes no result)
    rc = L.cm_mem_images_open_memory_sets(parts, C.c_uint32(n), res)
    judged = n > 0 and all(r.status != -1 for r in res[:n])
    out = None
    if judged:
        out = []
        for r, (image, a), (_, values, siblings, counts) in zip(res[:n], reqs, keep):
            rec = MemSetOpening(a, values[:a.size], siblings[:r.n_siblings], counts) if r.status == 0 else None
            out.append((r.status, r.message.decode(errors="replace"), rec, r.root))
    if rc and (not judged or all(r.status != rc for r in res[:n]) or rc in (2, 3)):
        try:
            _raise_status(L, rc)
        except CmError as e:
            e.results = out
            raise
    return (rc, out) if with_rc else out


def _image_open_sets(self, address_lists):
    """open_sets with every part under this image -> [(MemSetOpening, root)]; raises CmError (.status, .message, .results) when
    any part fails"""
    rc, out = open_sets([(self, a) for a in address_lists], self.L, with_rc=True)
    if rc:
        try:
            _raise_status(self.L, rc)
        except CmError as e:
            e.results = out
            raise
    return [(rec, root) for _, _, rec, root in out]


MemImage.open_sets = _image_open_sets


# ---- program identity and the statement of a run (include/cairom_hip.h: cm_program_id_entries .. cm_run_statement_of) ----------
class RunStatementC(C.Structure):
    """cm_run_statement"""
    _fields_ = [(n, C.c_uint32) for n in ("struct_size", "n_segments", "program_id", "program_start", "n_program", "initial_pc",
                                          "initial_fp", "final_pc", "final_fp", "initial_root", "final_root", "n_input", "n_output",
                                          "reserved0")]


def program_entries(start, values):
    """The (n, 7) entry array (present, address, value[4], clock) of a program whose cells start, start + 1, .. hold `values`
    (n x 4 words, or n shorter rows padded with zeros); clocks 0."""
    rows = [list(v) + [0] * (4 - len(v)) for v in values]
    v = np.array(rows, dtype=np.uint32).reshape(-1, 4)
    e = np.zeros((v.shape[0], 7), dtype=np.uint32)
    e[:, 0] = 1
    e[:, 1] = (int(start) + np.arange(v.shape[0], dtype=np.uint64)).astype(np.uint32)
    e[:, 2:6] = v
    return e


def _entries(entries):
    e = np.ascontiguousarray(entries, dtype=np.uint32)
    if e.size % 7:
        raise ValueError(f"{e.size} words are not seven-word entries")
    return e.reshape(-1, 7)


def program_id(entries, lib=None):
    """cm_program_id_entries (host code, no GPU): the id of the program whose public entries these are — the root of the partial
    memory tree that holds only these cells (Proof::program_id of the reference).  Raises CmError where the reference panics (an
    absent entry, no entries) and for entries that are no dense range of field words."""
    L = lib or load_library()
    e = _entries(entries)
    got = C.c_uint32(0)
    pad = e if e.size else np.zeros((1, 7), dtype=np.uint32)                     # (an empty array still has to be an address)
    rc = L.cm_program_id_entries(_p(pad), C.c_uint64(e.shape[0]), C.byref(got))
    if rc:
        raise _lib_error(L, rc)
    return got.value


def _proof_program_id(self):
    """cm_proof_program_id (host code, no GPU): which program this proof is about."""
    got = C.c_uint32(0)
    rc = self.L.cm_proof_program_id(self.h, C.byref(got))
    if rc:
        raise _lib_error(self.L, rc)
    return got.value


def _backend_program_ids(self, items, stream=0, with_status=False):
    """cm_program_ids / cm_proofs_program_ids (GPU): the ids of a batch of programs in one call.  items: Proofs, or entry arrays
    (n, 7).  Returns the ids; a bad item raises CmError naming the lowest one — with_status: (ids, status list, message) instead."""
    items = list(items)
    n = len(items)
    ids = np.zeros(max(n, 1), dtype=np.uint32)
    status = np.zeros(max(n, 1), dtype=np.int32)
    st = status.ctypes.data_as(C.POINTER(C.c_int32))
    if n and all(isinstance(x, Proof) for x in items):
        rc = self.L.cm_proofs_program_ids(_proof_handles(items), C.c_uint32(n), _p(ids), st, C.c_uint64(stream))
    else:
        keep = [_entries(x) for x in items]
        ptrs = (C.c_void_p * max(n, 1))(*[k.ctypes.data if k.size else None for k in keep])
        counts = (C.c_uint64 * max(n, 1))(*[k.shape[0] for k in keep])
        rc = self.L.cm_program_ids(ptrs, counts, C.c_uint32(n), _p(ids), st, C.c_uint64(stream))
    buf = C.create_string_buffer(1024)
    self.L.cm_last_error(buf, C.c_size_t(1024))
    msg = buf.value.decode(errors="replace") if rc else ""
    if rc and (rc != 1 or not msg.startswith("item ") or not with_status):
        raise CmError(f"libcairom_hip status {rc}: {msg}")
    return (ids[:n].copy(), status[:n].tolist(), msg) if with_status else ids[:n].copy()


def run_statement(proofs, cfg=None, program_id=None, device=False, lib=None):
    """cm_run_statement_of -> (status, message, dict): the chain check of verify_run (device=True: on the GPU), then one program in
    every segment, then its id (hashed on the GPU when device=True) against `program_id` when that is given.  The dict (None
    unless status 0) holds the fields of cm_run_statement plus the run's `input` (proof 0's) and `output` (the last proof's) entry
    arrays."""
    L = lib or proofs[0].L
    out = RunStatementC()
    out.struct_size = C.sizeof(RunStatementC)
    want = C.byref(C.c_uint32(int(program_id))) if program_id is not None else None
    rc = L.cm_run_statement_of(_proof_handles(proofs), C.c_uint32(len(proofs)), _cfg(cfg), want, C.c_uint32(1 if device else 0), C.byref(out))
    if rc:
        buf = C.create_string_buffer(1024)
        L.cm_last_error(buf, C.c_size_t(1024))
        return rc, buf.value.decode(errors="replace"), None
    d = {n: getattr(out, n) for n, _ in RunStatementC._fields_ if n not in ("struct_size", "reserved0")}
    d["input"] = proofs[0].public_data()["input"]
    d["output"] = proofs[-1].public_data()["output"]
    return 0, "", d


Proof.program_id = _proof_program_id
Backend.program_ids = _backend_program_ids
Backend.run_statement = lambda self, proofs, cfg=None, program_id=None, device=False: run_statement(proofs, cfg, program_id, device, self.L)
