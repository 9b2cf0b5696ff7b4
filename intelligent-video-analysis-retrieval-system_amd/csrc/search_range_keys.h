// Range tail over key stretches: every key of a query's stretch whose score is >= a threshold, as the lims / D / I / cap contract of
// ivr_index_range_search writes its results.  The keys are the 64-bit (ordered score, ~row) keys of ivr_key, 0 for "no row"; a key
// source Src has  uint64_t key(int q, int64_t i)  for 0 <= i < n, as the sources of search_select.h have, and names the rows of one
// query in ascending order, so the results of a query come out in ascending row order without a sort.  Three launches per chunk of
// queries, nothing synchronises with the host:
//   range_keys_count    one workgroup per (query, block of kRangeKeysBlock keys): the hits of the block
//   range_keys_prefix   one workgroup: the counts become output positions (exclusive prefix over the chunk in (query, block) order, on
//                       top of the running total the previous chunk left on the device), and lims of the chunk's queries is written
//   range_keys_write    the grid of the count pass again: each hit to its position when that is below cap
// The count and the write pass evaluate the same test on the same keys, so their hit sets agree.  Each body is stated once, here;
// a file that includes the header gets instantiations of its own (search_seq.hip does; the list scans may).  Not part of the C ABI.
#pragma once
#include "ivr_common.h"
#include "search_internal.h"

namespace {

constexpr int kRangeKeysThreads = 256;
constexpr int kRangeKeysPerThread = 16;
constexpr int kRangeKeysBlock = kRangeKeysThreads * kRangeKeysPerThread;      // keys per workgroup: 4096

// a present key whose score is >= threshold (false for a NaN score); the score is the one the select tail reports (-0.0 as +0.0)
__device__ __forceinline__ bool range_key_hit(uint64_t key, float threshold, float &score) {
    score = ivr_ord2f((uint32_t)(key >> 32));
    return key != 0 && score >= threshold;
}

// exclusive prefix sum over the workgroup (blockDim.x a multiple of 64, at most 1024); total = the workgroup's sum.  wsum: LDS [16]
__device__ __forceinline__ uint32_t range_keys_block_scan(uint32_t v, uint32_t &total, uint32_t *wsum) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, nw = blockDim.x >> 6;
    const uint32_t incl = ivr_wave_incl_scan(v, lane);
    if (lane == 63) wsum[w] = incl;
    __syncthreads();
    uint32_t before = 0, tot = 0;
    for (int i = 0; i < nw; ++i) {
        const uint32_t c = wsum[i];
        before += i < w ? c : 0u;
        tot += c;
    }
    __syncthreads();                    // wsum is reused by the next call
    total = tot;
    return before + incl - v;
}

// Workgroup j: block j % nblk of query q = j / nblk; thread t holds keys 16 t .. 16 t + 15 of the block (ascending rows), bit u of
// hits = key u of the thread is a hit
template <typename Src>
__device__ __forceinline__ void range_keys_load(const Src &src, int64_t nblk, float threshold, int &q, uint32_t &hits,
                                                   uint64_t (&keys)[kRangeKeysPerThread]) {
    q = (int)((int64_t)blockIdx.x / nblk);
    const int64_t i0 = ((int64_t)blockIdx.x % nblk) * kRangeKeysBlock + (int64_t)threadIdx.x * kRangeKeysPerThread;
    hits = 0;
#pragma unroll
    for (int u = 0; u < kRangeKeysPerThread; ++u) {
        keys[u] = i0 + u < src.n ? src.key(q, i0 + u) : 0;
        float sc;
        if (range_key_hit(keys[u], threshold, sc)) hits |= 1u << u;
    }
}

template <typename Src>
__global__ __launch_bounds__(kRangeKeysThreads) void range_keys_count_kernel(Src src, int64_t nblk, float threshold, int64_t *__restrict__ cnt) {
    __shared__ uint32_t wsum[16];
    int q;
    uint32_t hits, total;
    uint64_t keys[kRangeKeysPerThread];
    range_keys_load(src, nblk, threshold, q, hits, keys);
    (void)range_keys_block_scan((uint32_t)__popc(hits), total, wsum);
    if (threadIdx.x == 0) cnt[blockIdx.x] = total;
}

// One workgroup.  cnt [nq * nblk] hits per (query, block) -> in place, the output position of the block's first hit: the running total
// (*total, 0 for the first chunk) plus the hits of everything in front of it.  lims[q0 + q] = the position of query q's first block,
// lims[q0 + nq] = the new running total, which also goes back to *total for the next chunk.
__global__ __launch_bounds__(1024) void range_keys_prefix_kernel(int64_t *__restrict__ cnt, int64_t nblk, int nq, int64_t q0, int first,
                                                                 int64_t *__restrict__ total, int64_t *__restrict__ lims) {
    __shared__ uint32_t wsum[16];
    int64_t carry = first ? 0 : *total;
    __syncthreads();                    // every thread has read the total before thread 0 replaces it
    const int64_t n = (int64_t)nq * nblk;
    for (int64_t j0 = 0; j0 < n; j0 += blockDim.x) {
        const int64_t j = j0 + threadIdx.x;
        const uint32_t v = j < n ? (uint32_t)cnt[j] : 0u;
        uint32_t tot;
        const int64_t pos = carry + range_keys_block_scan(v, tot, wsum);
        if (j < n) {
            cnt[j] = pos;
            if (j % nblk == 0) lims[q0 + j / nblk] = pos;
        }
        carry += tot;
    }
    if (threadIdx.x == 0) {
        lims[q0 + nq] = carry;
        *total = carry;
    }
}

// ids != NULL: the label of row r is ids[r], else r itself
template <typename Src>
__global__ __launch_bounds__(kRangeKeysThreads) void range_keys_write_kernel(Src src, int64_t nblk, float threshold, const int64_t *__restrict__ pos0,
                                                                             float *__restrict__ D, int64_t *__restrict__ I, int64_t cap,
                                                                             const int64_t *__restrict__ ids) {
    __shared__ uint32_t wsum[16];
    int q;
    uint32_t hits, total;
    uint64_t keys[kRangeKeysPerThread];
    range_keys_load(src, nblk, threshold, q, hits, keys);
    int64_t pos = pos0[blockIdx.x] + range_keys_block_scan((uint32_t)__popc(hits), total, wsum);
    if (total == 0) return;
#pragma unroll
    for (int u = 0; u < kRangeKeysPerThread; ++u) {
        if (!((hits >> u) & 1u)) continue;
        if (pos < cap) {
            const uint32_t row = 0xFFFFFFFFu - (uint32_t)keys[u];
            D[pos] = ivr_ord2f((uint32_t)(keys[u] >> 32));
            I[pos] = ids ? ids[row] : (int64_t)row;
        }
        ++pos;
    }
}

// blocks of one query's stretch: the position scratch of a chunk of nq queries is nq * range_keys_blocks(n) int64
inline int64_t range_keys_blocks(int64_t n) { return std::max<int64_t>(1, ivr_ceil_div(n, kRangeKeysBlock)); }

// The range tail of one chunk of nq queries whose results start at lims[q0].  off: the position scratch; total: one int64 on the
// device that carries the running total from chunk to chunk (the same address for every chunk of a call); first: the chunk starts
// the call (its positions count from 0 and *total is not read)
template <typename Src>
void launch_range_keys(const Src &src, int nq, int64_t q0, bool first, float threshold, int64_t *off, int64_t *total, int64_t *lims, float *D,
                       int64_t *I, int64_t cap, const int64_t *ids, hipStream_t s) {
    const int64_t nblk = range_keys_blocks(src.n), nwg = (int64_t)nq * nblk;
    hipLaunchKernelGGL(range_keys_count_kernel<Src>, dim3((unsigned)nwg), dim3(kRangeKeysThreads), 0, s, src, nblk, threshold, off);
    hipLaunchKernelGGL(range_keys_prefix_kernel, dim3(1), dim3(1024), 0, s, off, nblk, nq, q0, first ? 1 : 0, total, lims);
    hipLaunchKernelGGL(range_keys_write_kernel<Src>, dim3((unsigned)nwg), dim3(kRangeKeysThreads), 0, s, src, nblk, threshold,
                       (const int64_t *)off, D, I, cap, ids);
}

}  // namespace
