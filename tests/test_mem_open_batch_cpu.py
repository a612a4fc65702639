"""Batched set openings without a GPU (cm_mem_images_open_memory_sets): the symbol and the two structs against the header; every
refusal of the call as a whole, decided before any address is read and with nothing written to the results; host images and the
other host-side verdicts as parts with status 1 in the single call's words; the word count of a part whose room is short; and that
a call which passes the argument checks then asks for the device.  CPU only: with a GPU present the tests still hold what they can
(the host's verdicts)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from cairo_m_amd.lib import CmError, MemImage, MemSetRequestC, MemSetResultC, load_library, mem_set_plan, open_sets
from tests.mem_image_ref import first_tree, snapshot
from tests.mem_set_ref import SETS, SPACE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = open(os.path.join(ROOT, "include", "cairom_hip.h")).read()
BAD = C.cast(1, C.POINTER(C.c_uint32))                                           # an address nobody may read
SENTINEL = 0xA5A5A5A5
ptr = lambda x: x.ctypes.data_as(C.POINTER(C.c_uint32))


def last_error(L):
    buf = C.create_string_buffer(1024)
    L.cm_last_error(buf, C.c_size_t(1024))
    return buf.value.decode()


def part(img, n=1, addresses=BAD, values=BAD, siblings=BAD, cap=28, struct_size=None):
    p = MemSetRequestC()
    p.struct_size = C.sizeof(MemSetRequestC) if struct_size is None else struct_size
    p.n, p.img, p.addresses, p.values, p.siblings, p.cap_siblings = n, img, addresses, values, siblings, cap
    return p


def call(L, parts, n=None, results=True):
    """parts None: a NULL `parts`; every byte of the results is a sentinel before the call"""
    k = len(parts or [])
    arr = (MemSetRequestC * max(k, 1))(*(parts or []))
    res = (MemSetResultC * max(k, 1))()
    C.memset(res, 0x5A, C.sizeof(res))
    rc = L.cm_mem_images_open_memory_sets(None if parts is None else arr, C.c_uint32(k if n is None else n), res if results else None)
    return rc, last_error(L), res


def untouched(res):
    return bytes(res) == b"\x5a" * C.sizeof(res)


class Arrays:
    """a part with arrays of its own, filled with a sentinel: addresses `a` as they are (the C ABI's view), room for `cap` words"""

    def __init__(self, img, a, cap=None, values=True, n=None):
        self.a = np.array(a if len(a) else [0], dtype=np.uint32)
        self.need = mem_set_plan(a)[1] if len(a) and sorted(set(a)) == list(a) and a[-1] < SPACE else 0
        self.cap = self.need if cap is None else cap
        self.v = np.full(4 * max(len(a), 1), SENTINEL, dtype=np.uint32)
        self.w = np.full(max(self.cap, 1), SENTINEL, dtype=np.uint32)
        self.part = part(img, len(a) if n is None else n, ptr(self.a), ptr(self.v) if values else None, ptr(self.w), self.cap)

    def clean(self):
        return bool((self.v == SENTINEL).all() and (self.w == SENTINEL).all())


@pytest.fixture(scope="module")
def hosts():
    ims = [MemImage.from_cells(first_tree("a").cells, device=False) for _ in range(2)]
    yield ims
    for im in ims:
        im.free()


def test_the_symbol_is_exported_and_declared_and_the_revision_stays():
    L = load_library()
    L.cm_mem_images_open_memory_sets
    assert re.search(r"int32_t\s+cm_mem_images_open_memory_sets\(const cm_mem_set_request\* parts, uint32_t n_parts, cm_mem_set_result\* results\);", HDR)
    assert int(re.search(r"#define CM_ABI_REVISION (\d+)", HDR).group(1)) == 10      # additive


def test_ctypes_mirrors_match_the_header():
    m = re.search(r"typedef struct \{([^{}]*?)\} cm_mem_set_request;\s*/\* sizeof = (\d+) \*/", HDR, re.S)
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    fields = [re.match(r"(?:const )?(?:uint32_t|cm_mem_image)\*?\s+(\w+)$", d.strip()).group(1) for d in body.split(";") if d.strip()]
    assert fields == [f[0] for f in MemSetRequestC._fields_] == ["struct_size", "n", "img", "addresses", "values", "siblings", "cap_siblings", "reserved"]
    assert [getattr(MemSetRequestC, f).offset for f in fields] == [0, 4, 8, 16, 24, 32, 40, 44]
    assert C.sizeof(MemSetRequestC) == int(m.group(2)) == 48
    m = re.search(r"typedef struct \{([^{}]*?)\} cm_mem_set_result;\s*/\* sizeof = (\d+) \*/", HDR, re.S)
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    assert [d.strip() for d in body.split(";") if d.strip()] == ["int32_t status", "uint32_t root", "uint32_t n_siblings", "uint32_t reserved",
                                                                 "char message[240]"]
    assert [getattr(MemSetResultC, f).offset for f in ("status", "root", "n_siblings", "reserved", "message")] == [0, 4, 8, 12, 16]
    assert C.sizeof(MemSetResultC) == int(m.group(2)) == 256


def test_the_call_level_refusals_leave_the_results_untouched(hosts):
    """status 1 each, the message as the header words it, no byte of the results written and no address read (BAD would fault)"""
    L = load_library()
    a, b = (im.h for im in hosts)
    head = "cm_mem_images_open_memory_sets: "
    cases = [
        (lambda: call(L, None, n=1), head + "null argument"),
        (lambda: call(L, [part(a)], results=False), head + "null argument"),
        (lambda: call(L, [part(a)], n=0), head + "no parts, or more than 2^16 parts in one call: open in groups"),
        (lambda: call(L, [part(a)], n=(1 << 16) + 1), head + "no parts, or more than 2^16 parts in one call: open in groups"),
        (lambda: call(L, [part(a), part(b, struct_size=40)]),
         head + "part 1: struct_size does not cover cm_mem_set_request (set it to sizeof(cm_mem_set_request))"),
        (lambda: call(L, [part(a), part(a), part(None)]), head + "part 2: null image"),
        (lambda: call(L, [part(a, n=1 << 20), part(a, n=1)]), head + f"the parts hold {(1 << 20) + 1} cells, more than 2^20 in one call: open in groups"),
    ]
    for f, want in cases:
        rc, msg, res = f()
        assert rc == 1 and msg == want, (rc, msg)
        assert untouched(res)
    # the python wrapper raises for these, and for a missing device
    with pytest.raises(CmError) as e:
        open_sets([], lib=L)
    assert e.value.status == 1 and "no parts" in e.value.message and e.value.results is None
    with pytest.raises(CmError) as e:
        hosts[0].open_sets([])
    assert e.value.status == 1 and "no parts" in e.value.message


def test_host_side_verdicts_are_parts_with_status_1_and_the_call_asks_for_the_device(hosts):
    """Every kind of part the host judges, in one call, two of them under ONE image: each has its own status 1 in the single
    call's words, its arrays keep their sentinel, and the root is the image's.  The call passed the argument checks, so it asked
    for the device: without one it returns cm_init's status 3 and its message, and every part the host did not judge holds
    cm_init's status and message; with one, the lowest part's."""
    L = load_library()
    before = [snapshot(im) for im in hosts]
    h0, h1 = hosts[0].h, hosts[1].h
    who = "cm_mem_image_open_memory_set: "
    cases = [
        (Arrays(h0, [4, 5]), who + "a host image serves no openings: create the image with device = 1"),
        (Arrays(h0, []), who + "a set of no cells"),
        (Arrays(h1, [6, 4]), who + "address 1 is not above address 0 (4): the addresses must be strictly ascending and below 2^28"),
        (Arrays(h1, [5, 5]), who + "address 1 is not above address 0 (5): the addresses must be strictly ascending and below 2^28"),
        (Arrays(h0, [7, SPACE]), who + f"address 1 is beyond the address space of 2^28 cells ({SPACE}): the addresses must be strictly ascending and below 2^28"),
        (Arrays(h1, [4, 6], values=False), who + "null argument"),
        (Arrays(h0, [4, 6], cap=mem_set_plan([4, 6])[1] - 1), who + f"room for {mem_set_plan([4, 6])[1] - 1} sibling words where the set needs {mem_set_plan([4, 6])[1]}"),
        (Arrays(h1, [5]), who + "a host image serves no openings: create the image with device = 1"),
    ]
    rc, msg, res = call(L, [c.part for c, _ in cases])
    assert rc in (1, 3)
    for i, (r, (c, want)) in enumerate(zip(res, cases)):
        assert (r.status, r.message.decode()) == (1, want), i
        assert c.clean(), i
        assert r.root == first_tree("a").root and r.reserved == 0
    assert [r.n_siblings for r in res] == [mem_set_plan([4, 5])[1], 0, 0, 0, 0, 0, mem_set_plan([4, 6])[1], 28]
    if rc == 3:
        assert msg.startswith("cm_mem_images_open_memory_sets: no HIP device") and "part " not in msg   # cm_init's own words
        assert all(r.status in (1, 3) and (r.status == 1 or r.message.decode() == msg) for r in res)
        with pytest.raises(CmError) as e:
            open_sets([(hosts[0], [5, 4, 5]), (hosts[1], [SPACE])])
        assert e.value.status == 3 and [(s, rec) for s, _, rec, _ in e.value.results] == [(1, None), (1, None)]
        assert "a host image serves no openings" in e.value.results[0][1] and "beyond the address space" in e.value.results[1][1]
    else:
        assert msg == "part 0: " + cases[0][1]
        got = open_sets([(hosts[0], [5, 4, 5]), (hosts[1], [SPACE])])
        assert [(s, rec) for s, _, rec, _ in got] == [(1, None), (1, None)]
        with pytest.raises(CmError) as e:
            hosts[0].open_sets([[5]])
        assert e.value.status == 1 and e.value.message.startswith("part 0: " + who + "a host image")
    assert [snapshot(im) for im in hosts] == before


@pytest.mark.parametrize("i", range(len(SETS)))
def test_a_short_room_still_states_the_plans_word_count(hosts, i):
    """every one of the twelve sets with room for one word less than it needs: status 1, the single call's message, n_siblings =
    cm_mem_set_plan's, nothing written — decided by the host before the image is looked at, so a host image shows it"""
    L = load_library()
    a = SETS[i][1]
    need = mem_set_plan(a)[1]
    short, exact = Arrays(hosts[0].h, a, cap=need - 1), Arrays(hosts[1].h, a)
    rc, msg, res = call(L, [short.part, exact.part])
    assert rc in (1, 3)
    assert res[0].status == 1 and res[0].message.decode() == f"cm_mem_image_open_memory_set: room for {need - 1} sibling words where the set needs {need}"
    assert res[1].status == 1 and b"a host image serves no openings" in res[1].message
    assert res[0].n_siblings == res[1].n_siblings == need
    assert short.clean() and exact.clean()
