"""Child process of tests/test_gpu_env_paths.py (`python -m tests.env_path_child ...`): the library reads its environment-only
switches once, into static values, so a switched path needs a process that starts with the variable set.  The parent sets the
environment; this module only does the work and prints one JSON line.

  prove  OUT_DIR NAME[,NAME...]   proves each named input twice on GPU 0 and writes the words to OUT_DIR/NAME.K.npy
  verify WORDS.npy FLIPS.json     host code only: cm_verify_proof_words of the words and of each one-bit tampering
  merkle_layers                   commits NO_TOP_SHAPES (tests/merkle_op_shapes.py) on GPU 0 and compares every stored layer
                                  with the oracle; reports the launch kinds cm_merkle_plan names in this environment
"""
import json
import os
import sys
import time

import numpy as np


def make_input(name):
    from cairo_m_amd.lib import synth_fibonacci, vm_run
    if name.startswith("fib"):
        return synth_fibonacci(int(name[3:]))
    if name.startswith("u32loop"):
        from tests.test_oracle_air import u32_loop_program
        return vm_run(u32_loop_program(int(name[7:])), entry_pc=0, args=(), n_returns=0)
    raise SystemExit(f"unknown input {name}")


def prove(out_dir, names):
    from cairo_m_amd import Backend
    t0 = time.time()
    be = Backend(0)
    files = {}
    for name in names:
        inp = make_input(name)
        files[name] = []
        for k in range(2):   # (twice: a switch may change what a finished proof parks for its successor)
            p = be.prove(inp)
            path = os.path.join(out_dir, f"{name}.{k}.npy")
            np.save(path, p.words())
            p.free()
            files[name].append(path)
        inp.free()
    return {"files": files, "wall_s": round(time.time() - t0, 3)}


def verify(words_path, flips_path):
    from cairo_m_amd.lib import load_library
    from tests.verify_many_util import host_verify_words
    L = load_library()
    words = np.load(words_path)
    out = {"": list(host_verify_words(L, words))}
    for name, pos in json.load(open(flips_path)).items():
        bad = words.copy()
        bad[pos] ^= 1
        out[name] = list(host_verify_words(L, bad))
    return {"verdicts": out}


def merkle_layers():
    from cairo_m_amd import Backend
    from cairo_m_amd.lib import merkle_plan
    from tests.merkle_layers_util import assert_all_layers_equal_oracle
    from tests.merkle_op_shapes import NO_TOP_SHAPES
    from tests.oracle_binding import Oracle
    t0 = time.time()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    orc = Oracle(os.path.join(root, "oracle", "liboracle.so"))
    be = Backend(0)
    plans = []
    for k, logs in enumerate(NO_TOP_SHAPES):
        assert_all_layers_equal_oracle(be, orc, logs, seed=8200 + k)   # (an AssertionError ends the child with status 1)
        plans.append([[r["kind"], r["hi"], r["lo"], r["has_prev"]] for r in merkle_plan(logs)])
    return {"plans": plans, "wall_s": round(time.time() - t0, 3)}


if __name__ == "__main__":
    mode = sys.argv[1]
    if mode == "merkle_layers":
        res = merkle_layers()
    else:
        res = prove(sys.argv[2], sys.argv[3].split(",")) if mode == "prove" else verify(sys.argv[2], sys.argv[3])
    print(json.dumps(res), flush=True)
