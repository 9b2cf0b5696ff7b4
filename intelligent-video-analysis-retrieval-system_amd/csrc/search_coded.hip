// The device half of the coded-index layer: the row store of the flat coded indexes (CodeRows) and their two-level top-k
// (GroupTopK), both declared in search_coded.h.  search_binary.hip, search_sq.hip and search_pqfs.hip keep their layout kernels and
// scans over a CodeRows; search_pq.hip, search_sq.hip and search_pqfs.hip scan into a GroupTopK.  The kernels both launch are emitted
// here alone: the empty-index fill, the integer finish and the instantiations of select_topk_kernel over the sources below.
// DESIGN.md section 4, "The coded-index layer".
#include "ivr_common.h"
#include "search_coded.h"
#include "search_lists.h"
#include "search_select.h"

#include <cfloat>

namespace {

// the keys of the two selections: instantiations of select_topk_kernel of this file's own (search_select.h)
struct SrcCodedGroups {    // the float group maxima of query q
    const float *gmax;
    int64_t mstride;
    int64_t n;
    __device__ uint64_t key(int q, int64_t i) const {
        return ivr_key(gmax[(int64_t)q * mstride + i], (uint32_t)i);
    }
};
struct SrcCodedGroupsI32 { // the int32 group maxima of query q
    const int32_t *gmax;
    int64_t mstride;
    int64_t n;
    __device__ uint64_t key(int q, int64_t i) const {
        return ((uint64_t)((uint32_t)gmax[(int64_t)q * mstride + i] ^ 0x80000000u) << 32) | (uint32_t)(0xFFFFFFFFu - (uint32_t)i);
    }
};
struct SrcCodedKeys {      // the re-scored rows of the selected groups
    const uint64_t *keys;
    int64_t n;
    __device__ uint64_t key(int q, int64_t i) const { return keys[(int64_t)q * n + i]; }
};

// every result slot unused: an empty index
__global__ __launch_bounds__(256) void coded_absent_kernel(int64_t n, float *__restrict__ D, int64_t *__restrict__ I) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) {
        D[i] = -FLT_MAX;
        I[i] = -1;
    }
}

// D[i] holds ivr_ord2f(key >> 32) of slot i as select_topk_kernel wrote it (I[i] >= 0) -> float(acc) * scale + bias of its query
__global__ __launch_bounds__(256) void coded_finish_kernel(float *__restrict__ D, const int64_t *__restrict__ I, const float *__restrict__ scale,
                                                           const float *__restrict__ bias, int64_t n, int k) {
    SQ_NO_CONTRACT
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n || I[i] < 0) return;
    const uint32_t u = __float_as_uint(D[i]);
    const uint32_t o = (u & 0x80000000u) ? ~u : (u | 0x80000000u);       // the inverse of ivr_ord2f
    const int32_t acc = (int32_t)(o ^ 0x80000000u);
    const int64_t q = i / k;
    const float p = (float)acc * scale[q];
    D[i] = p + bias[q];
}

}  // namespace

// ---- CodeRows ----------------------------------------------------------------------------------------------------------------------
int CodeRows::grow(int64_t rows) {
    rows = ivr_round_up(std::max<int64_t>(rows, granule), granule);
    uint4 *nd = nullptr;
    IVR_HIP(hipMalloc(&nd, bytes(rows)));
    IVR_HIP(hipMemset(nd, 0, bytes(rows)));
    if (data) {
        // whole granules: a layout may interleave the rows of one, so that the groups in front of ntotal are no prefix of its bytes
        if (ntotal > 0) IVR_HIP(hipMemcpy(nd, data, bytes(ivr_round_up(ntotal, granule)), hipMemcpyDeviceToDevice));
        IVR_HIP(hipFree(data));
    }
    data = nd;
    cap = rows;
    return IVR_OK;
}

int CodeRows::reserve_for_add(int64_t n, const char *what) {
    if (ntotal + n <= cap) return IVR_OK;
    IVR_REQUIRE(ntotal + n < (1ll << 31) - granule, "%s: index would exceed 2^31 rows", what);
    IVR_HIP(hipDeviceSynchronize());
    return grow(std::max<int64_t>(ntotal + n, cap + cap / 2));
}

int CodeRows::add(const char *what, const void *codes, int64_t n, const std::function<void()> &pack) {
    IVR_REQUIRE(codes || n == 0, "%s: NULL argument", what);
    IVR_REQUIRE(n >= 0, "%s: n=%lld", what, (long long)n);
    std::lock_guard<std::mutex> lk(mu);
    if (n == 0) return IVR_OK;
    IVR_HIP(hipSetDevice(ctx->device));
    if (int rc = reserve_for_add(n, what)) return rc;
    pack();
    IVR_LAUNCH_CHECK();
    ntotal += n;
    return IVR_OK;
}

int CodeRows::get_codes(const char *what, int64_t start, int64_t n, const void *out, const std::function<void()> &unpack) {
    IVR_REQUIRE(out || n == 0, "%s: NULL argument", what);
    std::lock_guard<std::mutex> lk(mu);
    IVR_REQUIRE(start >= 0 && n >= 0 && start + n <= ntotal, "%s: rows [%lld,%lld) outside [0,%lld)", what, (long long)start,
                (long long)(start + n), (long long)ntotal);
    if (n == 0) return IVR_OK;
    IVR_HIP(hipSetDevice(ctx->device));
    unpack();
    IVR_LAUNCH_CHECK();
    return IVR_OK;
}

int CodeRows::reset(bool zero_fill) {
    std::lock_guard<std::mutex> lk(mu);
    if (!zero_fill && ntotal == 0) return IVR_OK;
    IVR_HIP(hipSetDevice(ctx->device));
    IVR_HIP(hipDeviceSynchronize());             // a search in flight still reads the rows
    if (zero_fill) IVR_HIP(hipMemset(data, 0, bytes(cap)));
    ntotal = 0;
    return IVR_OK;
}

// ---- GroupTopK ---------------------------------------------------------------------------------------------------------------------
int GroupTopK::absent(int nq, int k, float *D, int64_t *I, hipStream_t s) {
    const int64_t n = (int64_t)nq * k;
    hipLaunchKernelGGL(coded_absent_kernel, dim3((unsigned)ivr_ceil_div(n, 256)), dim3(256), 0, s, n, D, I);
    IVR_LAUNCH_CHECK();
    return IVR_OK;
}

int GroupTopK::plan(int nq, int k, int64_t ngroups, int pass) {
    mstride = ivr_round_up(ngroups, 64);
    ksel = (int)std::min<int64_t>(k, ngroups);
    const int64_t fit = std::min<int64_t>({(int64_t)kMaxChunk, kChunkKeys / ((int64_t)ksel * 64), kChunkKeys / mstride});
    qc = (int)std::min<int64_t>(nq, std::max<int64_t>(pass, fit / pass * pass));
    return ivr_reserve({{&gmax, (size_t)qc * mstride * 4}, {&sel, (size_t)qc * ksel * sizeof(uint32_t)},
                        {&keys, (size_t)qc * ksel * 64 * sizeof(uint64_t)}});
}

void GroupTopK::select_groups(bool int32_maxima, int nqc, int64_t ngroups, hipStream_t s) {
    const SelectOut o = SelectOut::to_groups(sel);
    if (int32_maxima) launch_select<OUT_GROUPS>(SrcCodedGroupsI32{static_cast<const int32_t *>(gmax.ptr), mstride, ngroups}, nqc, ksel, o, s);
    else launch_select<OUT_GROUPS>(SrcCodedGroups{static_cast<const float *>(gmax.ptr), mstride, ngroups}, nqc, ksel, o, s);
}

void GroupTopK::select_rows(int nqc, int k, float *D, int64_t *I, hipStream_t s) {
    launch_select<OUT_DI>(SrcCodedKeys{keys, (int64_t)ksel * 64}, nqc, k, SelectOut::to_rows(D, I), s);
}

void GroupTopK::finish(float *D, const int64_t *I, const float *scale, const float *bias, int64_t n, int k, hipStream_t s) {
    hipLaunchKernelGGL(coded_finish_kernel, dim3((unsigned)ivr_ceil_div(n, 256)), dim3(256), 0, s, D, I, scale, bias, n, k);
}
