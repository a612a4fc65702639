"""Helpers of the cm_verify_many tests: where the parts of a proof sit in its flat word stream (cairo_m_amd/csrc/proof.hpp
proof_to_words), and the host verifier's answer for a word stream."""
import ctypes as C

import numpy as np


def proof_layout(words):
    """offsets (in words) of the parts of a proof word stream a tampering test aims at"""
    w = [int(x) for x in words]
    lay = {}
    i = 5                                   # magic, four config words
    nc = w[i]; i += 1 + nc + 4 * nc         # claim: log sizes, claimed sums
    i += 7                                  # registers, clock, roots
    for _ in range(3):                      # program, input, output entries (7 words each)
        i += 1 + 7 * w[i]
    i += 2                                  # interaction proof of work
    nt = w[i]
    lay["commitments"] = [i + 1 + 8 * t for t in range(nt)]
    i += 1 + 8 * nt
    lay["sampled"] = []                     # per tree: offset of the first value of every column
    for _ in range(nt):
        ncol = w[i]; i += 1
        cols = []
        for _ in range(ncol):
            ns = w[i]; cols.append(i + 1); i += 1 + 4 * ns
        lay["sampled"].append(cols)

    def dec(i):
        nh = w[i]; hw = (i + 1, nh); i += 1 + 8 * nh
        ncw = w[i]; cw = (i + 1, ncw); i += 1 + ncw
        return i, {"hash_witness": hw, "column_witness": cw}

    lay["decommitments"] = []
    for _ in range(nt):
        i, d = dec(i)
        lay["decommitments"].append(d)
    lay["queried"] = []
    for _ in range(nt):
        lay["queried"].append((i + 1, w[i])); i += 1 + w[i]
    lay["pow"] = i; i += 2

    def layer(i):
        nw = w[i]; fw = (i + 1, nw); i += 1 + 4 * nw
        i, d = dec(i)
        d["fri_witness"] = fw
        d["commitment"] = i
        return i + 8, d

    i, lay["fri_first"] = layer(i)
    nl = w[i]; i += 1
    lay["fri_inner"] = []
    for _ in range(nl):
        i, d = layer(i)
        lay["fri_inner"].append(d)
    lay["last_poly"] = (i + 1, w[i]); i += 1 + 4 * w[i]
    i += 1
    assert i == len(w), (i, len(w))
    return lay


def host_verify_words(L, words, cfg=None):
    """cm_verify_proof_words: (status, message)"""
    w = np.ascontiguousarray(words, dtype=np.uint32)
    rc = L.cm_verify_proof_words(w.ctypes.data_as(C.POINTER(C.c_uint32)), C.c_uint64(w.size), (C.c_uint32 * 4)(*cfg) if cfg else None)
    buf = C.create_string_buffer(512)
    L.cm_last_error(buf, C.c_size_t(512))
    return rc, buf.value.decode(errors="replace") if rc else ""


def proof_from_words(L, words):
    """cm_proof_from_words: a Proof, or None when the stream does not parse"""
    from cairo_m_amd.lib import Proof
    w = np.ascontiguousarray(words, dtype=np.uint32)
    h = C.c_void_p()
    rc = L.cm_proof_from_words(w.ctypes.data_as(C.POINTER(C.c_uint32)), C.c_uint64(w.size), C.byref(h))
    return Proof(L, h) if rc == 0 else None


def hand_flips(words):
    """name -> word offset of one hand-placed flip in every part of the proof the query phase reads (and three it does not)"""
    lay = proof_layout(words)
    out = {"commitment root": lay["commitments"][1] + 3, "sampled value": lay["sampled"][1][5] + 2, "proof-of-work nonce": lay["pow"]}
    for t in range(4):
        off, n = lay["queried"][t]
        out[f"queried value of tree {t}"] = off + n // 2
    off, n = lay["decommitments"][1]["hash_witness"]
    if n:
        out["hash witness of tree 1"] = off + 8 * (n // 2) + 1
    off, n = lay["decommitments"][1]["column_witness"]
    # (the column witness of a commitment tree is empty whenever every node of a column layer on a query path is itself queried —
    # always, for trees whose columns are queried at the folded positions; the flip then lands in its length word)
    out["column witness of tree 1"] = off + n // 2 if n else off - 1
    off, n = lay["fri_first"]["fri_witness"]
    out["FRI first-layer witness"] = off + 4 * (n // 2) + 1
    inner = [d for d in lay["fri_inner"] if d["fri_witness"][1]]
    off, n = inner[len(inner) // 2]["fri_witness"]
    out["FRI inner-layer witness"] = off + 4 * (n // 2) + 2
    inner = [d for d in lay["fri_inner"] if d["hash_witness"][1]]
    off, n = inner[len(inner) // 2]["hash_witness"]
    out["FRI inner-layer hash witness"] = off + 8 * (n // 2) + 5
    out["last-layer polynomial"] = lay["last_poly"][0] + 1
    return out
