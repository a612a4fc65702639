"""Followed memory in host code (cm_mem_image_*, device = 0): an image absorbs the update of every entry of SETS in its three forms
and then holds exactly the reference tree; the re-emitted record is the reference transition; every refusal leaves the image
byte-identical; the empty image; a chain applied part by part against its composition applied once; the ABI.  CPU only."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from cairo_m_amd.lib import (CmError, MemImage, MemImageStatsC, MemTransition, compose_transitions, load_library, verify_transition_host)
from tests import mem_compose_ref as mc
from tests.mem_image_ref import (FORMS, P, SET_IDS, SETS, RefTree, apply_form, assert_image_is, assert_refused, default_hashes, first_tree, reference,
                                 refusals, same_record, second_tree, snapshot, transition, tree_cells, words)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = open(os.path.join(ROOT, "include", "cairom_hip.h")).read()
NEW = ["cm_mem_image_create", "cm_mem_image_free", "cm_mem_image_root", "cm_mem_image_stats_get", "cm_mem_image_read", "cm_mem_image_cells",
       "cm_mem_image_nodes", "cm_mem_image_apply", "cm_mem_image_apply_transition", "cm_mem_image_open_memory", "cm_mem_image_open_memory_range",
       "cm_mem_image_open_memory_set"]
MULTI = 6                                                                         # SETS[6]: seven cells of memory "c", a held zero cell among them


def host_image(name):
    return MemImage.from_cells(first_tree(name).cells, device=False)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("i", range(len(SETS)), ids=SET_IDS)
def test_apply_gives_the_reference_tree(i, form):
    name, a = SETS[i]
    r = reference(i)
    im = host_image(name)
    try:
        assert_image_is(im, first_tree(name))
        assert apply_form(im, i, form) == r["root1"]
        assert_image_is(im, second_tree(i))
        assert np.array_equal(im.read(a[::-1]), r["new"][::-1])                  # any order
    finally:
        im.free()


@pytest.mark.parametrize("i", range(len(SETS)), ids=SET_IDS)
def test_record_is_the_reference_transition(i):
    im = host_image(SETS[i][0])
    try:
        root, t = apply_form(im, i, "pair", record=True)
        assert root == reference(i)["root1"] and same_record(t, reference(i))
        assert verify_transition_host(t) == (0, "")
        assert t.nbytes == 36 * t.addresses.size + 4 * t.siblings.size and t.nbytes_bare == 20 * t.addresses.size
    finally:
        im.free()


@pytest.mark.parametrize("what", list(refusals(MULTI)))
def test_refusals_leave_the_image_as_it_was(what):
    call, status, needle = refusals(MULTI)[what]
    im = host_image(SETS[MULTI][0])
    try:
        assert_refused(im, call, status, needle)
        apply_form(im, MULTI, "full")                                             # and the image still takes the valid update
        assert_image_is(im, second_tree(MULTI))
    finally:
        im.free()


def test_null_arguments_are_status_1():
    L = load_library()
    im = host_image("a")
    a, v, root, h = (C.c_uint32 * 1)(5), (C.c_uint32 * 4)(), C.c_uint32(0), C.c_void_p()

    def refused(rc):
        buf = C.create_string_buffer(256)
        L.cm_last_error(buf, C.c_size_t(256))
        return rc == 1 and b"null" in buf.value

    try:
        before = snapshot(im)
        for args in ((None, a, v, C.c_uint64(1), None, None, None, C.byref(root), None), (im.h, None, v, C.c_uint64(1), None, None, None, C.byref(root), None),
                     (im.h, a, None, C.c_uint64(1), None, None, None, C.byref(root), None), (im.h, a, v, C.c_uint64(1), None, None, None, None, None)):
            assert refused(L.cm_mem_image_apply(*args))
        assert refused(L.cm_mem_image_apply_transition(im.h, None, None)) and refused(L.cm_mem_image_apply_transition(None, None, None))
        assert refused(L.cm_mem_image_create(None, None, C.c_uint64(1), C.c_uint32(0), C.byref(h))) and not h.value
        assert refused(L.cm_mem_image_root(im.h, None)) and refused(L.cm_mem_image_stats_get(im.h, None))
        assert L.cm_mem_image_apply(im.h, a, v, C.c_uint64(0), None, None, None, C.byref(root), None) == 1   # n = 0
        assert snapshot(im) == before
    finally:
        im.free()


def test_create_refuses_bad_cells():
    for cells, needle in (([(5, 1, 2, 3, 4), (5, 1, 2, 3, 4)], "address 1 is not above address 0"), ([(1 << 28, 1, 2, 3, 4)], "address 0 is beyond the address space"),
                          ([(4, 1, 2, 3, 4), (9, 1, P, 3, 4)], "value word 1 of cell 9 is not below P")):
        with pytest.raises(CmError) as e:
            MemImage.from_cells(cells, device=False)
        assert e.value.status == 1 and needle in e.value.message
    L, h = load_library(), C.c_void_p()
    assert L.cm_mem_image_create(None, None, C.c_uint64(0), C.c_uint32(2), C.byref(h)) == 1      # `device` is 0 or 1


def test_the_empty_image():
    im = MemImage.from_cells([], device=False)
    other = None
    try:
        assert im.root == default_hashes()[0] and im.n_cells == 0 and im.nodes().shape == (0, 8) and im.cells()[0].size == 0
        assert np.array_equal(im.read([3, 3, 0]), np.zeros((3, 4), dtype=np.uint32))
        for call in (lambda: im.open([5]), lambda: im.open_range(0, 2), lambda: im.open_set([5])):
            with pytest.raises(CmError) as e:
                call()
            assert "status 1:" in str(e.value) and "a host image serves no openings" in str(e.value)
        tree = first_tree("c")
        a, v = tree_cells(tree)
        root, t = im.apply(a, v, old_values=np.zeros_like(v), root_before=default_hashes()[0], root_after=tree.root, record=True)
        assert root == tree.root and verify_transition_host(t) == (0, "") and not t.old_values.any()
        assert_image_is(im, tree)
        other = MemImage.from_cells(tree.cells, device=False)
        assert snapshot(other)[0] == snapshot(im)[0] and np.array_equal(words(other.nodes()), words(im.nodes()))
    finally:
        im.free()
        if other:
            other.free()


@pytest.mark.parametrize("name", ["wide", "gap_and_restore", "create_and_zero", "empties"])
def test_a_chain_part_by_part_equals_its_composition_once(name):
    c = mc.chain(name)
    parts = mc.parts_of(name)
    one, once = MemImage.from_cells(c["trees"][0].cells, device=False), MemImage.from_cells(c["trees"][0].cells, device=False)
    try:
        for i, p in enumerate(parts):
            assert one.apply_transition(p.bare()) == c["trees"][i + 1].root
        assert once.apply_transition(compose_transitions(parts, device=False).bare()) == c["ref"]["root1"]
        assert snapshot(one)[0] == snapshot(once)[0] and np.array_equal(words(one.nodes()), words(once.nodes()))
        assert all(x.tobytes() == y.tobytes() for x, y in zip(one.cells(), once.cells()))
        assert_image_is(one, c["trees"][-1])
    finally:
        one.free()
        once.free()


def test_new_symbols_are_exported_and_declared():
    L = load_library()
    for name in NEW:
        getattr(L, name)
        assert re.search(r"int32_t\s+%s\(" % name, HDR), name
    assert int(re.search(r"#define CM_ABI_REVISION (\d+)", HDR).group(1)) == 10      # additive


def test_ctypes_mirror_matches_the_header():
    m = re.search(r"typedef struct \{([^{}]*?)\} cm_mem_image_stats;\s*/\* sizeof = (\d+) \*/", HDR, re.S)
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    fields = [re.match(r"uint(?:32|64)_t\s+(\w+)$", d.strip()).group(1) for d in body.split(";") if d.strip()]
    assert fields == [f[0] for f in MemImageStatsC._fields_] == ["struct_size", "device", "n_cells", "n_nodes", "bytes"]
    assert [getattr(MemImageStatsC, f).offset for f in fields] == [0, 4, 8, 16, 24]
    assert C.sizeof(MemImageStatsC) == int(m.group(2)) == 32
    im = host_image("a")
    try:
        s = MemImageStatsC()
        s.struct_size = 8                                                         # too short
        assert load_library().cm_mem_image_stats_get(im.h, C.byref(s)) == 1
        assert im.stats() == {"device": False, "n_cells": 1, "n_nodes": 31, "bytes": im.stats()["bytes"]} and im.stats()["bytes"] >= 31 * 32
    finally:
        im.free()
