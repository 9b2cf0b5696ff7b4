"""GPU: rowwise_cosine_kernel (csrc/dedup.hip) per element against the float64 reference and the derived bound of
oracle/reduce_ref.py.  The inputs and the checks live in reduce_cases.py; test_reduce_ref_cpu.py shows on a numpy emulation of the
kernel that a correct one passes them and that typical faults (a dropped last column, tail lanes reading past d, a clamped norm) do
not."""
import pytest

import reduce_cases as C

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("d", C.COSINE_D)
def test_rowwise_cosine_within_the_derived_bound(d):
    """n = 1, 4, 5, 103 (a partly filled last workgroup of four waves); Gaussian rows, rows of mean 5 and spread 0.1, rows made
    orthogonal in float64."""
    print(f"\nd={d}: largest error / bound = {C.check_cosine_bound(C.Gpu, d):.3f}")


def test_zero_rows_perfect_squares_and_power_of_two_scaling():
    C.check_cosine_special(C.Gpu)


def test_calculate_similarities_is_rowwise_cosine_of_the_shifted_rows():
    """Bit for bit, with a second operand that starts d floats into the buffer (12 bytes at d = 3: not 16-byte aligned)."""
    C.check_calculate_similarities(C.Gpu)


@pytest.mark.parametrize("d", [1025, 2048])
def test_exact_cosines_of_zero_one_rows(d):
    """Non-zeros at columns 0, 63, 64 and d - 1; every sum is exact in any order, so cos is exactly 0, 0.5 and 1."""
    C.check_cosine_exact(C.Gpu, d)
