"""Batched image updates without a GPU (cm_mem_images_apply): every refusal of the call as a whole, with its message and decided
before any address is read; the two structs against the header; a batch of host images, each with its own status 1; and that a
call which passes the argument checks then asks for the device.  CPU only: with a GPU present the last test still holds what it
can (the host's verdicts)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from cairo_m_amd.lib import (CmError, MemImage, MemImageResultC, MemImageUpdateC, apply_images, follow_runs_images, load_library, mem_batch_plan,
                             mem_batch_launches)
from tests.mem_image_ref import SETS, first_tree, snapshot, transition

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = open(os.path.join(ROOT, "include", "cairom_hip.h")).read()
BAD = C.cast(1, C.POINTER(C.c_uint32))                                           # an address nobody may read


def last_error(L):
    buf = C.create_string_buffer(1024)
    L.cm_last_error(buf, C.c_size_t(1024))
    return buf.value.decode()


def part(img, n=1, addresses=BAD, new_values=BAD, struct_size=None):
    p = MemImageUpdateC()
    p.struct_size = C.sizeof(MemImageUpdateC) if struct_size is None else struct_size
    p.n, p.img, p.addresses, p.new_values = n, img, addresses, new_values
    return p


def call(L, parts, n=None, results=True):
    """parts None: a NULL `parts`"""
    k = len(parts or [])
    arr = (MemImageUpdateC * max(k, 1))(*(parts or []))
    res = (MemImageResultC * max(k, 1))()
    for r in res:
        r.status = -7
    rc = L.cm_mem_images_apply(None if parts is None else arr, C.c_uint32(k if n is None else n), res if results else None)
    return rc, last_error(L), res


@pytest.fixture(scope="module")
def hosts():
    ims = [MemImage.from_cells(first_tree("a").cells, device=False) for _ in range(3)]
    yield ims
    for im in ims:
        im.free()


def test_the_symbol_is_exported_and_declared_and_the_revision_stays():
    L = load_library()
    L.cm_mem_images_apply
    assert re.search(r"int32_t\s+cm_mem_images_apply\(const cm_mem_image_update\* parts, uint32_t n_parts, cm_mem_image_result\* results\);", HDR)
    assert int(re.search(r"#define CM_ABI_REVISION (\d+)", HDR).group(1)) == 10      # additive


def test_ctypes_mirrors_match_the_header():
    m = re.search(r"typedef struct \{([^{}]*?)\} cm_mem_image_update;\s*/\* sizeof = (\d+) \*/", HDR, re.S)
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    fields = [re.match(r"(?:const )?(?:uint32_t|cm_mem_image)\*?\s+(\w+)$", d.strip()).group(1) for d in body.split(";") if d.strip()]
    assert fields == [f[0] for f in MemImageUpdateC._fields_] == ["struct_size", "n", "img", "addresses", "new_values", "old_values", "root_before",
                                                                  "root_after"]
    assert [getattr(MemImageUpdateC, f).offset for f in fields] == [0, 4, 8, 16, 24, 32, 40, 48]
    assert C.sizeof(MemImageUpdateC) == int(m.group(2)) == 56
    m = re.search(r"typedef struct \{([^{}]*?)\} cm_mem_image_result;\s*/\* sizeof = (\d+) \*/", HDR, re.S)
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    assert [d.strip() for d in body.split(";") if d.strip()] == ["int32_t status", "uint32_t root", "char message[248]"]
    assert [getattr(MemImageResultC, f).offset for f in ("status", "root", "message")] == [0, 4, 8]
    assert C.sizeof(MemImageResultC) == int(m.group(2)) == 256


def test_the_call_level_refusals(hosts):
    """status 1 each, the message as the header words it, no result written and no address read (BAD would fault)"""
    L = load_library()
    a, b, c = (im.h for im in hosts)
    before = [snapshot(im) for im in hosts]
    cases = [
        (lambda: call(L, None, n=1), "cm_mem_images_apply: null argument"),
        (lambda: call(L, [part(a)], results=False), "cm_mem_images_apply: null argument"),
        (lambda: call(L, [part(a)], n=0), "no parts, or more than 2^16 parts in one call: apply in groups"),
        (lambda: call(L, [part(a)], n=(1 << 16) + 1), "no parts, or more than 2^16 parts in one call: apply in groups"),
        (lambda: call(L, [part(a), part(b, struct_size=48)]),
         "part 1: struct_size does not cover cm_mem_image_update (set it to sizeof(cm_mem_image_update))"),
        (lambda: call(L, [part(a), part(b), part(None)]), "part 2: null image"),
        (lambda: call(L, [part(a, n=1 << 20), part(b, n=1)]), f"the parts hold {(1 << 20) + 1} cells, more than 2^20 in one call: apply in groups"),
        (lambda: call(L, [part(c), part(a), part(b), part(a)]), "parts 1 and 3 name one image: updates of one image depend on each other"),
    ]
    for f, needle in cases:
        rc, msg, res = f()
        assert rc == 1 and needle in msg, (rc, msg)
        assert all(r.status == -7 for r in res)
    assert [snapshot(im) for im in hosts] == before
    # the python wrapper raises for these, and only for these
    t = transition(0)
    with pytest.raises(CmError) as e:
        apply_images([(hosts[0], t), (hosts[0], t)])
    assert e.value.status == 1 and "parts 0 and 1 name one image" in e.value.message and e.value.results is None
    with pytest.raises(CmError) as e:
        apply_images([], lib=L)
    assert e.value.status == 1 and "no parts" in e.value.message


def test_host_images_are_parts_with_status_1_and_the_call_asks_for_the_device(hosts):
    """Every part is a host image: each has its own status 1 in the openers' words and is unchanged.  The call passed the
    argument checks, so it asked for the device: without one it returns cm_init's status 3; with one, the lowest part's."""
    L = load_library()
    before = [snapshot(im) for im in hosts]
    t = transition(0)                                                             # SETS[0]: cell 5 of memory "a", a valid update
    a, nv = np.array(t.addresses), np.ascontiguousarray(t.new_values).reshape(-1)
    ptr = lambda x: x.ctypes.data_as(C.POINTER(C.c_uint32))
    rc, msg, res = call(L, [part(im.h, n=a.size, addresses=ptr(a), new_values=ptr(nv)) for im in hosts])
    assert rc in (1, 3)
    for r, im in zip(res, hosts):
        assert r.status == 1 and b"device images only" in r.message and r.message.startswith(b"cm_mem_images_apply: ")
        assert r.root == im.root == first_tree("a").root
    if rc == 3:
        assert "part " not in msg and msg                                         # cm_init's own words
        with pytest.raises(CmError) as e:
            apply_images([(im, t) for im in hosts])
        assert e.value.status == 3 and [s for s, _, _ in e.value.results] == [1, 1, 1]
    else:
        assert msg.startswith("part 0: cm_mem_images_apply: device images only")
        assert [s for s, _, _ in apply_images([(im, t) for im in hosts])] == [1, 1, 1]
    assert [snapshot(im) for im in hosts] == before
    assert follow_runs_images([]) == []


def _mix(copies):
    """the address lists of `copies` batches of all twelve SETS: dense parts beside one- and two-cell parts"""
    return [a for _ in range(copies) for _, a in SETS]


def test_the_ladder_does_not_depend_on_the_number_of_parts():
    """host code only: the plan the launch path runs has the same steps for 1, 12 and 36 parts of the same set mix — the ladder is
    that of the part with the most per-level steps (the 1 667-cell dense set: six) plus the cells and one tail"""
    widest = max(SETS, key=lambda s: len(s[1]))[1]
    one, twelve, many = mem_batch_plan([widest]), mem_batch_plan(_mix(1)), mem_batch_plan(_mix(3))
    shape = lambda plan: [(s["depth"], s["kernel"]) for s in plan]
    assert shape(one) == shape(twelve) == shape(many) and len(one) == 29
    assert mem_batch_launches(one) == mem_batch_launches(twelve) == mem_batch_launches(many) == 1 + 6 + 1
    assert [s["widest_part"] for s in twelve] == [s["widest_part"] for s in many]
    assert [s["n_nodes"] for s in many] == [3 * s["n_nodes"] for s in twelve]
