"""Bounds of tests/test_align_cpu.py::test_well_conditioned_sets_against_svd: the worst element-wise difference between the
restatement's fp32 transform and the float64 SVD solution over the 120 problems of ``_align_ref.well_conditioned_problems()``, times 2.
They are set by the fp32 rounding of the output (2^-24 = 6e-8 relative; |T| reaches 3, s reaches 2), not by the solve, whose float64
result differs from the SVD's by 1e-14."""
R_MEASURED, T_MEASURED, S_MEASURED = 2.95e-08, 1.19e-07, 8.78e-08
R_BOUND, T_BOUND, S_BOUND = 2 * R_MEASURED, 2 * T_MEASURED, 2 * S_MEASURED
