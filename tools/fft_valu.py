#!/usr/bin/env python3
"""Static instruction audit of the transform kernels (no GPU: hipcc cross-compiles gfx950).

Compiles cairo_m_amd/csrc/kernels_fft.hip to assembly and prints, per kernel, the vector-ALU instructions of the kernel's text,
the `v_readfirstlane_b32` among them, the 64-bit compares, the VOP3-encoded selects, the scalar loads, the conditional branches
and the VGPRs.  The rounds are fully unrolled, so the text is what a thread executes EXCEPT for the launch-wide alternatives, of
which one runs: the first round's loads (plain | extension by two | zero-padded with a select per element: 16 elements x 5) and,
in the inverse strided kernels, the output scaling (none | 31-bit rotation 16 x 3 | multiply 16 x 5; 8 elements on the 2^11 tile).

usage: python tools/fft_valu.py [-DCM_FFT_UNIFORM_TW=0 ...] [--all]      (default: the strided shapes; --all: every kernel)"""
import collections, os, re, subprocess, sys, tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "cairo_m_amd", "csrc", "kernels_fft.hip")


def demangle(n):
    m = re.match(r"_ZN2cm14k_fft_fused_rbILi(\d+)ELi(\d+)E", n)
    if m:
        return "k_fft_fused_rb<%s,%s>" % m.groups()
    m = re.match(r"_ZN2cm13k_fft_pass_rbILb(\d)ELi(\d+)ELi(\d+)ELi(\d+)E", n)
    if m:
        return "k_fft_pass_rb<%s,%s,%s,%s>" % ((("false", "true")[int(m.group(1))],) + m.groups()[1:])
    return n


def main():
    defs = [a for a in sys.argv[1:] if a.startswith("-D")]
    every = "--all" in sys.argv[1:]
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "fft.s")
        subprocess.check_call(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", "-S", "--cuda-device-only",
                               "-Wno-unused-command-line-argument", *defs, SRC, "-o", out])
        lines = open(out).read().split("\n")
    ops, vgpr, cur = {}, {}, None
    for l in lines:
        m = re.match(r"^(_Z\w+):", l)
        if m:
            cur = m.group(1); ops[cur] = collections.Counter(); continue
        if l.startswith(".Lfunc_end"):
            cur = None; continue
        if cur is None:
            continue
        t = l.strip()
        if not t or t[0] in ";." or t.endswith(":"):
            continue
        ops[cur][t.split()[0]] += 1
    # VGPRs from the kernel descriptors' comments (`; NumVgprs: n` follows each kernel's text)
    name = None
    for l in lines:
        m = re.match(r"^(_Z\w+):", l)
        if m:
            name = m.group(1)
        m = re.match(r";\s*NumVgprs:\s*(\d+)", l)
        if m and name:
            vgpr[name] = int(m.group(1))
    print("build:", " ".join(defs) or "(default)")
    print("%-34s %6s %6s %8s %8s %7s %8s %5s" % ("kernel", "VALU", "rfl", "cmp_u64", "cnd_e64", "s_load", "branches", "VGPR"))
    for n, c in ops.items():
        dn = demangle(n)
        if not every and not (dn.startswith("k_fft_fused_rb") or re.search(r",(14|11),\d>$", dn) and ",11,11," not in dn):
            continue
        valu = sum(v for k, v in c.items() if k.startswith("v_"))
        print("%-34s %6d %6d %8d %8d %7d %8d %5d" % (
            dn, valu, c["v_readfirstlane_b32"], sum(v for k, v in c.items() if re.match(r"v_cmp\w*_[ui]64", k)),
            c["v_cndmask_b32_e64"], sum(v for k, v in c.items() if k.startswith("s_load_") or k.startswith("s_buffer_load_")),
            sum(v for k, v in c.items() if k.startswith("s_cbranch")), vgpr.get(n, -1)))


if __name__ == "__main__":
    main()
