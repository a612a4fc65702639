"""Which transform kernel runs at which size (no GPU: cm_fft_plan and cm_fft_extend_fused are host code, and every launch reads
the same function).  The plan of every log size 1..28 is pinned to a table written out by hand, under the default plan and, in a
child process (the switch is read once), under CM_FFT_OLD_PLAN=1; and the sizes the GPU op tests run (tests/fft_op_sizes.py) must
reach every (direction, tile, W) instantiation that kernels_fft.hip can dispatch, read off its source.  After a change of the plan
or a new instantiation this fails here, on the CPU, until tests/fft_op_sizes.py has a size that runs the new kernel."""
import json
import os
import re
import subprocess
import sys

import pytest

from cairo_m_amd.lib import CmError, fft_extend_fused, fft_plan
from tests.fft_op_sizes import FFT_OP_SIZES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def S(lo, hi, tile):
    """one pass: layers [lo, hi) on a tile of 2^tile (0 = the generic kernel); M = the rest of the tile, 0 for the contiguous pass"""
    return (lo, hi, tile, tile - (hi - lo) if lo else 0)


# default plan: generic kernel up to 2^10; one contiguous pass of 11 / 12; [0, 12) + one strided pass (2^11 tile for 1..5 layers,
# 2^14 tile for 6..9); 22 = 13 + 9; from 23 on two balanced strided passes behind [0, 12)
DEFAULT_PLAN = {n: [S(0, n, 0)] for n in range(1, 11)}
DEFAULT_PLAN.update({
    11: [S(0, 11, 11)], 12: [S(0, 12, 12)],
    13: [S(0, 12, 12), S(12, 13, 11)], 14: [S(0, 12, 12), S(12, 14, 11)], 15: [S(0, 12, 12), S(12, 15, 11)],
    16: [S(0, 12, 12), S(12, 16, 11)], 17: [S(0, 12, 12), S(12, 17, 11)],
    18: [S(0, 12, 12), S(12, 18, 14)], 19: [S(0, 12, 12), S(12, 19, 14)], 20: [S(0, 12, 12), S(12, 20, 14)],
    21: [S(0, 12, 12), S(12, 21, 14)],
    22: [S(0, 13, 13), S(13, 22, 14)],
    23: [S(0, 12, 12), S(12, 18, 14), S(18, 23, 11)], 24: [S(0, 12, 12), S(12, 18, 14), S(18, 24, 14)],
    25: [S(0, 12, 12), S(12, 19, 14), S(19, 25, 14)], 26: [S(0, 12, 12), S(12, 19, 14), S(19, 26, 14)],
    27: [S(0, 12, 12), S(12, 20, 14), S(20, 27, 14)], 28: [S(0, 12, 12), S(12, 20, 14), S(20, 28, 14)],
})
# CM_FFT_OLD_PLAN=1: contiguous pass of 11 layers, strided passes of at most 7
OLD_PLAN = {n: [S(0, n, 0)] for n in range(1, 11)}
OLD_PLAN.update({
    11: [S(0, 11, 11)],
    12: [S(0, 11, 11), S(11, 12, 11)], 13: [S(0, 11, 11), S(11, 13, 11)], 14: [S(0, 11, 11), S(11, 14, 11)],
    15: [S(0, 11, 11), S(11, 15, 11)], 16: [S(0, 11, 11), S(11, 16, 11)],
    17: [S(0, 11, 11), S(11, 17, 14)], 18: [S(0, 11, 11), S(11, 18, 14)],
    19: [S(0, 11, 11), S(11, 15, 11), S(15, 19, 11)], 20: [S(0, 11, 11), S(11, 16, 11), S(16, 20, 11)],
    21: [S(0, 11, 11), S(11, 16, 11), S(16, 21, 11)], 22: [S(0, 11, 11), S(11, 17, 14), S(17, 22, 11)],
    23: [S(0, 11, 11), S(11, 17, 14), S(17, 23, 14)], 24: [S(0, 11, 11), S(11, 18, 14), S(18, 24, 14)],
    25: [S(0, 11, 11), S(11, 18, 14), S(18, 25, 14)],
    26: [S(0, 11, 11), S(11, 16, 11), S(16, 21, 11), S(21, 26, 11)],
    27: [S(0, 11, 11), S(11, 17, 14), S(17, 22, 11), S(22, 27, 11)],
    28: [S(0, 11, 11), S(11, 17, 14), S(17, 23, 14), S(23, 28, 11)],
})
# cm_interpolate_extend: the fused sweep serves the plans "[0, 12) + one 2^14-tile pass"
FUSED_LOGS = [18, 19, 20, 21]


def dispatchable():
    """what launch_w and launch_fft_fused_rb of kernels_fft.hip can launch, read off the source: {(tile, W)}, {fused W}"""
    src = open(os.path.join(ROOT, "cairo_m_amd", "csrc", "kernels_fft.hip")).read()
    body = src[src.index("static void launch_w("):src.index("uint32_t fft_pass_rb_tile_log(")]
    passes = {(int(tl), int(w)) for w, tl in re.findall(r"launch_one<INV, (\d+), (\d+), \d+>", body)}
    fused_body = src[src.index("void launch_fft_fused_rb("):src.index("template <bool INV, int W, int TL, int E>\nstatic void launch_one(")]
    fused = {int(w) for w in re.findall(r"launch_fused_one<(\d+)>", fused_body)}
    assert len(passes) >= 10 and len(fused) >= 4, "the source no longer reads as this test expects"
    return passes, fused


def test_default_plan_equals_the_table():
    # the library reads the switch at its first plan query: this process must not have carried it
    assert "CM_FFT_OLD_PLAN" not in os.environ, "unset CM_FFT_OLD_PLAN: this test pins the default plan"
    for n in range(1, 29):
        assert fft_plan(n) == DEFAULT_PLAN[n], n
    for n in range(1, 28):
        assert fft_extend_fused(n) == (n in FUSED_LOGS), n
    for bad in (0, 29):
        with pytest.raises(CmError):
            fft_plan(bad)
    with pytest.raises(CmError):
        fft_extend_fused(28)


def test_plan_passes_tile_the_layers_and_fit_the_kernels():
    """every pass of every plan is one the launch code can serve: consecutive layer ranges covering [0, n), M = tile - W on the
    register-blocked kernels, a contiguous run no longer than the stride below it (M <= lo), the tile inside the transform"""
    assert "CM_FFT_OLD_PLAN" not in os.environ, "unset CM_FFT_OLD_PLAN: this test reads the default plan"
    passes, _ = dispatchable()
    for n in range(1, 29):
        plan = fft_plan(n)
        assert plan[0][0] == 0 and plan[-1][1] == n and all(a[1] == b[0] for a, b in zip(plan, plan[1:])), (n, plan)
        for lo, hi, tile, m in plan:
            w = hi - lo
            if tile:
                assert (tile, w) in passes and m == (tile - w if lo else 0) and m <= lo and w + m <= n, (n, lo, hi, tile, m)
            else:
                assert w + m <= 11 and m <= lo, (n, lo, hi, tile, m)   # the generic kernel's LDS tile


def _reached(plan_of, fused_of):
    """(direction, tile, W) of every pass the op tests run, and the fused W's, for FFT_OP_SIZES under the given plan"""
    got, fused = set(), set()
    for n in FFT_OP_SIZES["inverse"]:
        got |= {("inverse", t, hi - lo if t else 0) for lo, hi, t, _ in plan_of(n)}
    for n in FFT_OP_SIZES["forward"]:
        got |= {("forward", t, hi - lo if t else 0) for lo, hi, t, _ in plan_of(n)}
    for n in FFT_OP_SIZES["extend"]:
        if fused_of(n):   # interpolate_extend: [0, 12) inverse at n | the fused sweep | [0, 12) forward at n + 1
            fused.add(n - 12)
            got |= {("inverse", 12, 12), ("forward", 12, 12)}
        else:
            got |= {("inverse", t, hi - lo if t else 0) for lo, hi, t, _ in plan_of(n)}
            got |= {("forward", t, hi - lo if t else 0) for lo, hi, t, _ in plan_of(n + 1)}
    return got, fused


def test_op_test_sizes_reach_every_instantiation():
    assert "CM_FFT_OLD_PLAN" not in os.environ, "unset CM_FFT_OLD_PLAN: this test reads the default plan"
    passes, fused = dispatchable()
    want = {(d, t, w) for d in ("inverse", "forward") for t, w in passes} | {("inverse", 0, 0), ("forward", 0, 0)}
    got, got_fused = _reached(fft_plan, fft_extend_fused)
    assert sorted(want - got) == [], "instantiations no op test of tests/fft_op_sizes.py runs"
    assert sorted(got - want) == [], "the plan selects a kernel kernels_fft.hip does not instantiate"
    assert got_fused == fused


def test_old_plan_equals_its_table_and_selects_no_other_kernel():
    """CM_FFT_OLD_PLAN=1 (read once per process: a child).  Its passes differ, its kernels do not: every (tile, W) it selects is one
    the default plan selects too, so the op tests cover the kernels and tests/test_gpu_env_paths.py the plan."""
    code = ("import json; from cairo_m_amd.lib import fft_plan, fft_extend_fused; "
            "print(json.dumps({'plan': [fft_plan(n) for n in range(1, 29)], 'fused': [fft_extend_fused(n) for n in range(1, 28)]}))")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=dict(os.environ, CM_FFT_OLD_PLAN="1"), capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    out = json.loads(r.stdout.strip().splitlines()[-1])
    for n, plan in zip(range(1, 29), out["plan"]):
        assert [tuple(p) for p in plan] == OLD_PLAN[n], n
    assert not any(out["fused"])   # its contiguous pass is 11 layers: the fused sweep never serves it
    default_kernels = {(t, hi - lo) for plan in DEFAULT_PLAN.values() for lo, hi, t, _ in plan}
    assert {(t, hi - lo) for plan in OLD_PLAN.values() for lo, hi, t, _ in plan} <= default_kernels
