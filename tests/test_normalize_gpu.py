"""GPU: l2_normalize_kernel (csrc/search_index.hip; normalize_L2 and count_nonfinite_and_normalize) per element against the float64
reference and the derived bound of oracle/reduce_ref.py.  Inputs and checks: reduce_cases.py, proven on the CPU by
test_reduce_ref_cpu.py."""
import pytest

import reduce_cases as C

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("d", C.NORMALIZE_D)
def test_normalize_within_the_derived_bound(d):
    """n = 1, 4, 5, 1027; rows of scales 0.01 .. 100; every output row has float64 norm 1 within unit_norm_bound(d)."""
    print(f"\nd={d}: largest error / bound = {C.check_normalize_bound(C.Gpu, d):.3f}")


def test_zero_rows_keep_their_sign_bits_and_power_of_two_scaling_changes_no_bit():
    C.check_normalize_special(C.Gpu)


def test_nonfinite_count_is_per_element_and_adds_up_across_workgroups():
    C.check_nonfinite_count(C.Gpu)
