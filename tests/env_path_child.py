"""Child process of tests/test_gpu_env_paths.py (`python -m tests.env_path_child ...`): the library reads its environment-only
switches once, into static values, so a switched path needs a process that starts with the variable set.  The parent sets the
environment; this module only does the work and prints one JSON line.

  prove  OUT_DIR NAME[,NAME...]   proves each named input twice on GPU 0 and writes the words to OUT_DIR/NAME.K.npy
  verify WORDS.npy FLIPS.json     host code only: cm_verify_proof_words of the words and of each one-bit tampering
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


if __name__ == "__main__":
    mode = sys.argv[1]
    res = prove(sys.argv[2], sys.argv[3].split(",")) if mode == "prove" else verify(sys.argv[2], sys.argv[3])
    print(json.dumps(res), flush=True)
