"""GPU: segment_mean_kernel (csrc/search_ivf.hip; ivr_segment_mean, _kmeans.segment_means and through them every centroid of every
inverted-file index and PQ codebook) per element against the float64 reference and the derived bound of oracle/reduce_ref.py.
Inputs and checks: reduce_cases.py, proven on the CPU by test_reduce_ref_cpu.py (a dropped last row, a start taken from the next
offset and float32 column sums all fail them)."""
import pytest

import reduce_cases as C

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("d", C.SEGMENT_D)
def test_segment_mean_within_the_derived_bound(d):
    """Segments of 0, 1, 2, 63, 1000, 0, 5, 0 rows (empty first, in the middle and last), the rows as one segment, segments on
    their own; normalize off and on; a one-row segment is that row, empty segments are NaN rows."""
    print(f"\nd={d}: largest error / bound = {C.check_segment_mean(C.Gpu, d):.3f}")


def test_offsets_are_clipped():
    C.check_segment_offsets(C.Gpu)


def test_zero_mean_stays_zero():
    C.check_segment_zero_mean(C.Gpu)


def test_column_sums_are_double():
    C.check_segment_double_sum(C.Gpu)


def test_segment_means_on_column_slices_with_and_without_order():
    C.check_segment_means_wrapper(C.Gpu)


@pytest.mark.parametrize("spherical", [True, False])
@pytest.mark.parametrize("n,d,nlist", C.KMEANS_CASES)
def test_one_kmeans_step_is_the_segment_mean_of_the_library_assignment(n, d, nlist, spherical):
    """IVFFlatIndex.train(niter=1) against the centroids of niter=0: the assignment is the library's own nearest-centroid search
    (checked to be a best one within the index's stated error), no cluster is empty, and the trained centroids are the segment
    means of exactly that assignment - no allowance for rows that could have gone either way."""
    from ivr_amd._kmeans import kmeans_sample
    from ivr_amd.index import FlatIPIndex
    from ivr_amd.ivf import IVFFlatIndex
    x = C.kmeans_rows(n, d)
    cents = []
    for niter in (0, 1):
        ivf = IVFFlatIndex(d, nlist)
        ivf.train(x, niter=niter, spherical=spherical)
        cents.append(ivf.centroids.copy())
    xs = x[kmeans_sample(n, nlist)]
    flat = FlatIPIndex(d)
    flat.add(cents[0])
    D, I = flat.search(xs, 1)
    flat.close()
    r = C.check_kmeans_step(xs, cents[0], D, I, cents[1], spherical, 1)
    print(f"\nlargest error / bound = {r:.3f}")
