// The segment bounds of the self-joins (self_join.h): the one kernel of their frame that is not inlined into the callers' own.
#include "ivr_common.h"
#include "self_join.h"

namespace {

__global__ __launch_bounds__(256) void sj_bounds_kernel(int n, const int64_t *__restrict__ seg_off, int nseg, int *__restrict__ seg_lo,
                                                        int *__restrict__ seg_hi) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= n) return;
    int lo = 0, hi = n;
    if (seg_off) {
        lo = hi = j + 1;                             // outside every segment
        if (seg_off[0] <= j) {
            const int s = ivr_last_le(seg_off, nseg + 1, j);
            if (s < nseg) {                          // seg_off[s] <= j < seg_off[s + 1]
                lo = (int)max(seg_off[s], (int64_t)0);
                hi = (int)min(seg_off[s + 1], (int64_t)n);
            }
        }
    }
    seg_lo[j] = lo;
    seg_hi[j] = hi;
}

}  // namespace

int sj_prepare(ivr_index *x, int qt, const int64_t *seg_off, int nseg, hipStream_t s, SjArgs &a) {
    const int n = (int)x->ntotal;
    const int64_t stride = ivr_round_up(n, 64);
    const int rc = ivr_reserve({{&x->sj_seg, (size_t)2 * stride * 4}});
    if (rc != IVR_OK) return rc;
    int *seg_lo = x->sj_seg, *seg_hi = seg_lo + stride;
    hipLaunchKernelGGL(sj_bounds_kernel, dim3((unsigned)ivr_ceil_div(n, 256)), dim3(256), 0, s, n, seg_off, nseg, seg_lo, seg_hi);
    IVR_LAUNCH_CHECK();
    a = SjArgs{reinterpret_cast<const float4 *>(x->data), x->dp4, qt, n, seg_lo, seg_hi};
    return IVR_OK;
}
