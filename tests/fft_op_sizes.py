"""The log sizes at which the GPU op tests of tests/test_gpu_poly_merkle.py run the transforms, in ONE place: those tests take
their parameters from here, and tests/test_fft_plan_cpu.py walks the same lists through cm_fft_plan on the CPU to prove that
every kernel instantiation the plan can select is run by one of them.  A change of the plan that selects a kernel at no size
listed here fails that CPU test until a size is added."""

# cm_interpolate at 2^n against the oracle (test_interpolate_evaluate_every_plan: n <= 22 with two columns, 23 and 24 with one)
INTERPOLATE_LOGS = list(range(1, 25))
# cm_evaluate from 2^n_in coefficients to 2^n_out values against the oracle.  test_interpolate_evaluate_every_plan: n -> n + 1 up
# to 23 -> 24 and the same-size n -> n (the round trip back to the evaluations) for every n; test_evaluate_zero_padded: the
# inputs shorter than half the output, where the last pass reads implicit zeros (in_len)
EVALUATE_EXTEND_LOGS = list(range(1, 24))
EVALUATE_PADDED = [(10, 12), (12, 14), (16, 19), (18, 20)]
# cm_interpolate_extend (test_interpolate_extend_parity): the fused sweep where cm_fft_extend_fused says so, else the two transforms
EXTEND_LOGS = [4, 12, 17, 18, 19, 20, 21, 22]

FFT_OP_SIZES = {
    "inverse": sorted(set(INTERPOLATE_LOGS)),
    "forward": sorted(set(INTERPOLATE_LOGS) | {n + 1 for n in EVALUATE_EXTEND_LOGS} | {o for _, o in EVALUATE_PADDED}),
    "extend": list(EXTEND_LOGS),
}
