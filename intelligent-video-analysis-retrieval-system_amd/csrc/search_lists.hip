// The device half of the inverted-file layer: the list store of the coded inverted-file indexes (ListRows, search_lists.h) and the
// probe tables of the list-major scans (ProbeTables, search_internal.h) with the four kernels that build them.  search_ivfpq.hip and
// search_ivfsq.hip keep their layout kernels and scans over a ListRows; search_ivf.hip and search_ivfsq.hip scan what
// ProbeTables::build leaves.  DESIGN.md section 4, "The inverted-file layer".
#include "ivr_common.h"
#include "search_internal.h"
#include "search_lists.h"
#include "search_select.h"

#include <algorithm>

namespace {

// One wave per query of the chunk.  slot[q][j] = first slot of entry j's list in the scratch (q * qstride + the rows of the query's
// earlier lists), -1 for a skipped entry; qtotal[q] = the rows the query probes.  A query whose lists hold more than qstride rows
// (the caller's bound is wrong) probes nothing rather than write past its stretch.
__global__ __launch_bounds__(256) void probe_slots_kernel(const int64_t *__restrict__ assign, int p, int nqc, const int64_t *__restrict__ list_off,
                                                          int nlist, int64_t ntotal, int64_t qstride, int64_t *__restrict__ slot,
                                                          int64_t *__restrict__ qtotal) {
    const int lane = threadIdx.x & 63;
    const int q = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (q >= nqc) return;
    const int64_t *a = assign + (int64_t)q * p;
    int64_t total = 0;
    for (int pass = 0; pass < 2; ++pass) {
        const bool fits = total <= qstride;          // pass 1 only: the total of pass 0
        int64_t carry = 0;
        for (int j0 = 0; j0 < p; j0 += 64) {
            const int j = j0 + lane;
            const bool valid = probe_valid(a, j, p, nlist);
            int64_t size = 0;
            if (valid) {
                int64_t r0, r1;
                list_run(list_off, a[j], ntotal, r0, r1);
                size = r1 - r0;
            }
            int64_t inc = size;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const int64_t t = __shfl_up(inc, o, 64);
                if (lane >= o) inc += t;
            }
            if (pass == 1 && j < p) slot[(int64_t)q * p + j] = valid && fits ? (int64_t)q * qstride + carry + inc - size : -1;
            carry += __shfl(inc, 63, 64);
        }
        total = carry;
    }
    if (lane == 0) qtotal[q] = total <= qstride ? total : 0;
}

__global__ __launch_bounds__(256) void probe_count_kernel(const int64_t *__restrict__ assign, const int64_t *__restrict__ slot, int64_t npairs,
                                                          int *__restrict__ count) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < npairs && slot[i] >= 0) atomicAdd(&count[assign[i]], 1);
}

// one workgroup of 256 threads: pair_off[l] = pairs of the lists below l, tile_off[l] = their 16-query pair tiles, l <= nlist; the
// counts become the fill cursors (zero)
__global__ __launch_bounds__(256) void probe_offsets_kernel(int *__restrict__ count, int nlist, int64_t *__restrict__ pair_off,
                                                            int64_t *__restrict__ tile_off) {
    __shared__ int64_t wp[4], wt[4];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    int64_t cp = 0, ct = 0;                          // carried over the rounds
    for (int l0 = 0; l0 <= nlist; l0 += 256) {
        const int l = l0 + threadIdx.x;
        const int64_t c = l < nlist ? count[l] : 0, t = (c + 15) >> 4;
        if (l < nlist) count[l] = 0;
        int64_t ip = c, it = t;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int64_t a = __shfl_up(ip, o, 64), b = __shfl_up(it, o, 64);
            if (lane >= o) {
                ip += a;
                it += b;
            }
        }
        if (lane == 63) {
            wp[w] = ip;
            wt[w] = it;
        }
        __syncthreads();
        int64_t bp = cp, bt = ct, tp = 0, tt = 0;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            if (i < w) {
                bp += wp[i];
                bt += wt[i];
            }
            tp += wp[i];
            tt += wt[i];
        }
        if (l <= nlist) {
            pair_off[l] = bp + ip - c;
            tile_off[l] = bt + it - t;
        }
        cp += tp;
        ct += tt;
        __syncthreads();
    }
}

__global__ __launch_bounds__(256) void probe_fill_kernel(const int64_t *__restrict__ assign, const int64_t *__restrict__ slot, int p, int64_t npairs,
                                                         int *__restrict__ cursor, const int64_t *__restrict__ pair_off,
                                                         int *__restrict__ pair_q, int64_t *__restrict__ pair_slot) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= npairs) return;
    const int64_t s = slot[i];
    if (s < 0) return;
    const int64_t l = assign[i];
    const int64_t at = pair_off[l] + atomicAdd(&cursor[l], 1);      // the order of a list's queries does not reach the result
    pair_q[at] = (int)(i / p);
    pair_slot[at] = s;
}


struct SrcSlots {      // the keys of query q: slots [q * qstride, q * qstride + qtotal[q]) of the scratch
    const uint64_t *keys;
    const int64_t *qtotal;
    int64_t qstride;
    int64_t n;         // the longest stretch a query of the launch may hold
    __device__ uint64_t key(int q, int64_t i) const { return i < qtotal[q] ? keys[(int64_t)q * qstride + i] : 0; }
};

}  // namespace

// ---- ProbeTables -------------------------------------------------------------------------------------------------------------------
int ProbeTables::plan(int nq, int p, int64_t qstride, int nlist, int *chunk, int64_t *nkeys) {
    // queries per chunk: the scratch holds chunk_slots keys (one query's stretch at least), the pair tables kIvfChunkPairs pairs
    *chunk = (int)std::max<int64_t>(1, std::min<int64_t>({(int64_t)nq, chunk_slots / std::max<int64_t>(qstride, 1), kIvfChunkPairs / p}));
    *nkeys = (int64_t)*chunk * qstride;
    const int64_t cpairs = (int64_t)*chunk * p;
    const int rc = ivr_reserve({{&keys, (size_t)std::max<int64_t>(*nkeys, 1) * 8}, {&slot, (size_t)cpairs * 8}, {&qtotal, (size_t)*chunk * 8},
                                {&pair_q, (size_t)cpairs * 4}, {&pair_slot, (size_t)cpairs * 8}});
    return rc != IVR_OK ? rc : ivr_reserve({{&count, (size_t)nlist * 4}, {&off, (size_t)(nlist + 1) * 16}}, true);
}

int ProbeTables::build(const int64_t *assign, int p, int nqc, const int64_t *list_off, int nlist, int64_t ntotal, int64_t qstride, hipStream_t s) {
    const int64_t npairs = (int64_t)nqc * p;
    IVR_HIP(hipMemsetAsync((int *)count, 0, (size_t)nlist * 4, s));
    hipLaunchKernelGGL(probe_slots_kernel, dim3((unsigned)ivr_ceil_div(nqc, 4)), dim3(256), 0, s, assign, p, nqc, list_off, nlist, ntotal, qstride,
                       (int64_t *)slot, (int64_t *)qtotal);
    hipLaunchKernelGGL(probe_count_kernel, dim3((unsigned)ivr_ceil_div(npairs, 256)), dim3(256), 0, s, assign, (const int64_t *)slot, npairs,
                       (int *)count);
    hipLaunchKernelGGL(probe_offsets_kernel, dim3(1), dim3(256), 0, s, (int *)count, nlist, pair_off(), tile_off(nlist));
    hipLaunchKernelGGL(probe_fill_kernel, dim3((unsigned)ivr_ceil_div(npairs, 256)), dim3(256), 0, s, assign, (const int64_t *)slot, p, npairs,
                       (int *)count, pair_off(), (int *)pair_q, (int64_t *)pair_slot);
    return IVR_OK;
}

void ProbeTables::select(int nqc, int k, int64_t qstride, float *D, int64_t *I, const int64_t *ids, hipStream_t s) {
    const SrcSlots src{keys, qtotal, qstride, qstride};
    const SelectOut o = SelectOut::to_rows(D, I, 0, ids);
    if (ids) launch_select<OUT_DI_IDS>(src, nqc, k, o, s);
    else launch_select<OUT_DI>(src, nqc, k, o, s);
}

// ---- ListRows ----------------------------------------------------------------------------------------------------------------------
int ListRows::init(ivr_ctx *c, int lists, const char *chunk_slots_env) {
    ctx = c;
    nlist = lists;
    by_size.assign((size_t)nlist + 1, 0);
    chunk_slots = ivr_env_positive(chunk_slots_env, kIvfChunkSlots);
    return ivr_reserve({{&offs, (size_t)(nlist + 1) * 16}}, true);       // no rows: every offset 0
}

int ListRows::set_lists(const char *what, const void *codes, const int64_t *src_ids, const int64_t *list_off, int64_t n, int64_t group_words,
                        bool by_rows, const std::function<void(int64_t)> &pack) {
    IVR_REQUIRE(list_off && ((codes && src_ids) || n == 0), "%s: NULL argument", what);
    IVR_REQUIRE(n >= 0, "%s: n=%lld", what, (long long)n);
    std::lock_guard<std::mutex> lk(mu);
    std::vector<int64_t> host((size_t)(nlist + 1) * 2), sizes((size_t)nlist);
    int64_t *goff = host.data() + nlist + 1;
    IVR_REQUIRE(list_off[0] == 0 && list_off[nlist] == n, "%s: list_off must run from 0 to n=%lld", what, (long long)n);
    goff[0] = 0;
    for (int l = 0; l < nlist; ++l) {
        IVR_REQUIRE(list_off[l + 1] >= list_off[l], "%s: list_off descends at list %d", what, l);
        const int64_t rows = list_off[l + 1] - list_off[l], groups = ivr_ceil_div(rows, 64);
        sizes[l] = by_rows ? rows : groups;
        goff[l + 1] = goff[l] + groups;
        host[l] = list_off[l];
    }
    host[nlist] = n;
    const int64_t groups = goff[nlist];
    IVR_REQUIRE(groups < (1ll << 26), "%s: %lld padded rows: packed positions must stay below 2^32", what, (long long)(groups * 64));
    IVR_HIP(hipSetDevice(ctx->device));
    IVR_HIP(hipDeviceSynchronize());             // a search in flight still reads the lists
    // empty until the new content is in place, and empty for good when a step below fails: no rows, and no list long enough to probe
    ntotal = ngroups = 0;
    std::fill(by_size.begin(), by_size.end(), 0);
    int rc = ivr_reserve({{&data, (size_t)groups * group_words * sizeof(uint4)}, {&ids, (size_t)groups * 64 * sizeof(int64_t)}});
    hipError_t e = hipSuccess;
    if (rc == IVR_OK) e = hipMemcpy((int64_t *)offs, host.data(), host.size() * sizeof(int64_t), hipMemcpyHostToDevice);
    if (rc == IVR_OK && e == hipSuccess && groups > 0) {
        pack(groups);
        e = hipGetLastError();
    }
    if (rc != IVR_OK || e != hipSuccess) {
        (void)hipMemset((int64_t *)offs, 0, host.size() * sizeof(int64_t));       // every list empty again
        if (rc != IVR_OK) return rc;
        return ivr_fail(e == hipErrorOutOfMemory ? IVR_ERR_OOM : IVR_ERR_HIP, "%s: %s", what, hipGetErrorString(e));
    }
    std::sort(sizes.begin(), sizes.end(), [](int64_t a, int64_t b) { return a > b; });
    for (int l = 0; l < nlist; ++l) by_size[l + 1] = by_size[l] + sizes[l];
    ntotal = n;
    ngroups = groups;
    return IVR_OK;
}

int ListRows::reset(const char *what) {
    std::vector<int64_t> zero((size_t)nlist + 1, 0);
    return set_lists(what, nullptr, nullptr, zero.data(), 0, 0, true, nullptr);
}

int ListRows::get_codes(const char *what, int64_t start, int64_t n, const void *codes, const int64_t *out_ids, const std::function<void()> &unpack) {
    IVR_REQUIRE(codes || out_ids || n == 0, "%s: NULL argument", what);
    std::lock_guard<std::mutex> lk(mu);
    IVR_REQUIRE(start >= 0 && n >= 0 && start + n <= ntotal, "%s: rows [%lld,%lld) outside [0,%lld)", what, (long long)start,
                (long long)(start + n), (long long)ntotal);
    if (n == 0) return IVR_OK;
    IVR_HIP(hipSetDevice(ctx->device));
    unpack();
    IVR_LAUNCH_CHECK();
    return IVR_OK;
}
