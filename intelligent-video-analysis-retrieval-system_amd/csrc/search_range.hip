// ---------------------------------------------------------------------------------------------
// exact range search (ivr_index_range_search): every stored row with <q, row> > radius, per chunk of <= 64 queries
//   1 group maxima      the scans of search.hip, unchanged (bf16 candidate scan, or the float32 scan)
//   2 candidates        range_candidates_kernel: the groups that can hold a row > radius, ascending, one workgroup per query
//   3 exact re-score    range_rescore_kernel: one wave per (query, candidate group) -> 64-bit hit mask + its popcount
//   4 offsets, output   range_offsets_kernel (prefix of the hit counts within each query), range_write_kernel (lims, then
//                       (score, id) of every hit in row order; the hit pairs are re-scored instead of storing 64 scores per pair)
// The number of (query, candidate) pairs is known on the device only: passes 3 and 4 run a persistent grid that strides over it.
// ---------------------------------------------------------------------------------------------
#include "ivr_common.h"
#include "search_internal.h"

namespace {

// exclusive prefix sum over the workgroup (blockDim.x a multiple of 64, at most 1024); total = the workgroup's sum.  wsum: LDS [16]
__device__ __forceinline__ uint32_t range_block_scan(uint32_t v, uint32_t &total, uint32_t *wsum) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, nw = blockDim.x >> 6;
    uint32_t incl = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t u = __shfl_up(incl, o, 64);
        if (lane >= o) incl += u;
    }
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

// Pass 2, one workgroup per query of the chunk.  A group is kept when it can hold a row scoring > radius:
//   exact maxima (float32 scan): the group maximum IS the largest exact score of the group (bit-identical to the re-score), so the
//   group is kept iff gmax > radius.
//   bf16 maxima (qnorm != NULL): per row |approx - exact| <= e = rel_eps |q| max|row| (the bound the verification of the top-k
//   search uses, 1.01 inflation included), so a row with exact score > radius lifts its group's approximate maximum above
//   radius - e.  Kept iff fl(gmax + e) >= radius: rounding is monotone and radius is a float, so the float test keeps every group
//   the real-number test keeps.  A non-finite e (NaN / inf in the rows or the query) keeps every group.
__global__ __launch_bounds__(1024) void range_candidates_kernel(const float *__restrict__ gmax, int64_t mstride, int64_t ngroups,
                                                                float radius, const float *__restrict__ qnorm, float rel_eps,
                                                                const unsigned int *__restrict__ maxnorm_bits, uint32_t *__restrict__ cand,
                                                                int64_t cstride, uint32_t *__restrict__ ncand) {
    __shared__ uint32_t wsum[16];
    const int q = blockIdx.x;
    const bool approx = qnorm != nullptr;
    const float e = approx ? rel_eps * qnorm[q] * __uint_as_float(*maxnorm_bits) : 0.f;
    const bool all = approx && !isfinite(e);
    const float *gm = gmax + (int64_t)q * mstride;
    uint32_t *out = cand + (int64_t)q * cstride;
    uint32_t base = 0;
    for (int64_t g0 = 0; g0 < ngroups; g0 += blockDim.x) {
        const int64_t g = g0 + threadIdx.x;
        bool keep = false;
        if (g < ngroups) {
            const float m = gm[g];
            keep = approx ? (all || m + e >= radius) : m > radius;
        }
        uint32_t tot;
        const uint32_t pos = range_block_scan(keep ? 1u : 0u, tot, wsum);
        if (keep) out[base + pos] = (uint32_t)g;
        base += tot;
    }
    if (threadIdx.x == 0) ncand[q] = base;
}

// pre[0] = 0, pre[i + 1] = pre[i] + ncand[i] over the chunk's queries (LDS, one thread: at most 64 terms)
__device__ __forceinline__ void range_pair_prefix(const uint32_t *__restrict__ ncand, int nqc, int64_t *pre) {
    if (threadIdx.x == 0) {
        int64_t s = 0;
        pre[0] = 0;
        for (int i = 0; i < nqc; ++i) {
            s += ncand[i];
            pre[i + 1] = s;
        }
    }
}

// The 64 rows of group g against query q of the chunk (qtile = the chunk's first query tile), scored by pair_score (search_internal.h)
// as rescore_groups_kernel scores them: each score is bit-identical to the one ivr_index_search reports for that row.  In the lanes
// with (lane & 15) == (q & 15), acc[t][r] = score of row 64 g + 16 t + 4 (lane >> 4) + r.  Returns the hit mask (bit i: row 64 g + i exists and scores
// > radius), the same in every lane.
// MASK: rows that are not allowed are never hits.
template <bool MASK = false, typename... M>
__device__ __forceinline__ uint64_t range_group_scores(const float *__restrict__ data, const float *__restrict__ qtile, int dp4,
                                                       int64_t ntotal, uint32_t g, int q, float radius, f32x4 (&acc)[4], const M &...rm) {
    const int lane = threadIdx.x & 63;
    uint32_t mbyte = 0;
    if constexpr (MASK) mbyte = row_mask_fetch(rm..., (int64_t)g * kGroupRows);
    const int per_tile = dp4 * 16, kchunks = dp4 >> 2;
    const float4 *b = reinterpret_cast<const float4 *>(qtile) + (int64_t)(q >> 4) * per_tile + lane;
    const bool mine = (lane & 15) == (q & 15);
    uint64_t m = 0;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        acc[t] = pair_score(reinterpret_cast<const float4 *>(data) + ((int64_t)g * 4 + t) * per_tile + lane, b, kchunks);
        if constexpr (!MASK) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int rl = t * 16 + (lane >> 4) * 4 + r;
                if (mine && (int64_t)g * kGroupRows + rl < ntotal && acc[t][r] > radius) m |= 1ull << rl;
            }
        }
    }
    if constexpr (MASK) {
        const uint64_t mw = row_mask_word(rm..., (int64_t)g * kGroupRows, mbyte);
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int rl = t * 16 + (lane >> 4) * 4 + r;
                if (mine && ((mw >> rl) & 1ull) && acc[t][r] > radius) m |= 1ull << rl;
            }
    }
    // the query's column lives in lanes c, c + 16, c + 32, c + 48 (c = q & 15), each with 16 of the 64 rows
    uint32_t lo = (uint32_t)m, hi = (uint32_t)(m >> 32);
    lo |= __shfl_xor(lo, 16, 64);
    hi |= __shfl_xor(hi, 16, 64);
    lo |= __shfl_xor(lo, 32, 64);
    hi |= __shfl_xor(hi, 32, 64);
    lo = __shfl(lo, q & 15, 64);
    hi = __shfl(hi, q & 15, 64);
    return ((uint64_t)hi << 32) | lo;
}

// Pass 3: persistent grid of 4-wave workgroups; wave w of the grid takes the pairs w, w + waves, ... in (query, group) order
template <bool MASK, typename... M>
__global__ __launch_bounds__(256) void range_rescore_kernel(const float *__restrict__ data, const float *__restrict__ qtile, int dp4,
                                                            int64_t ntotal, float radius, int nqc, const uint32_t *__restrict__ cand,
                                                            int64_t cstride, const uint32_t *__restrict__ ncand, uint64_t *__restrict__ mask,
                                                            uint32_t *__restrict__ hits, M... rm) {
    __shared__ int64_t pre[65];
    range_pair_prefix(ncand, nqc, pre);
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int64_t npairs = pre[nqc];
    for (int64_t p = (int64_t)blockIdx.x * 4 + wave; p < npairs; p += (int64_t)gridDim.x * 4) {
        const int q = ivr_last_le(pre, nqc, p);
        const int64_t at = (int64_t)q * cstride + (p - pre[q]);
        f32x4 acc[4];
        const uint64_t m = range_group_scores<MASK>(data, qtile, dp4, ntotal, cand[at], q, radius, acc, rm...);
        if (lane == 0) {
            mask[at] = m;
            hits[at] = (uint32_t)__popcll(m);
        }
    }
}

// Pass 4a, one workgroup per query: hit counts of its pairs -> their exclusive prefix sum (in place), nhits[q] = the query's hits
__global__ __launch_bounds__(1024) void range_offsets_kernel(const uint32_t *__restrict__ ncand, int64_t cstride, uint32_t *__restrict__ off,
                                                             uint32_t *__restrict__ nhits) {
    __shared__ uint32_t wsum[16];
    const int q = blockIdx.x;
    const uint32_t n = ncand[q];
    uint32_t *o = off + (int64_t)q * cstride;
    uint32_t base = 0;
    for (uint32_t j0 = 0; j0 < n; j0 += blockDim.x) {
        const uint32_t j = j0 + threadIdx.x;
        const uint32_t v = j < n ? o[j] : 0u;
        uint32_t tot;
        const uint32_t pos = range_block_scan(v, tot, wsum);
        if (j < n) o[j] = base + pos;
        base += tot;
    }
    if (threadIdx.x == 0) nhits[q] = base;
}

// Pass 4b, persistent grid like pass 3 (also behind a filtered search: it emits only bits of the hit masks, which the masked pass 3
// has restricted to the allowed rows).  Query i of the chunk starts at output position qb[i] = (running total before the chunk) +
// hits of queries 0 .. i-1; workgroup 0 writes lims[q0 .. q0 + nqc] and the new running total.  The total ping-pongs between two
// slots (read total[parity], write total[parity ^ 1]) so that no workgroup of this launch can read a value written by it; the first
// chunk starts from 0.  Pairs with hits are re-scored (same function as pass 3: the same scores, the same mask) and each hit is
// written at its position when that is < cap.  -0.0 is written as +0.0, as the top-k search reports it.
template <bool IDS>
__global__ __launch_bounds__(256) void range_write_kernel(const float *__restrict__ data, const float *__restrict__ qtile, int dp4,
                                                          int64_t ntotal, float radius, int nqc, int q0, const uint32_t *__restrict__ cand,
                                                          int64_t cstride, const uint32_t *__restrict__ ncand, const uint64_t *__restrict__ mask,
                                                          const uint32_t *__restrict__ off, const uint32_t *__restrict__ nhits,
                                                          int64_t *__restrict__ total, int first, int parity, int64_t *__restrict__ lims,
                                                          float *__restrict__ D, int64_t *__restrict__ I, int64_t cap, int64_t id_base,
                                                          const int64_t *__restrict__ ids) {
    __shared__ int64_t pre[65], qb[65];
    if (threadIdx.x == 0) {
        int64_t s = 0, h = first ? 0 : total[parity];
        pre[0] = 0;
        qb[0] = h;
        for (int i = 0; i < nqc; ++i) {
            s += ncand[i];
            h += nhits[i];
            pre[i + 1] = s;
            qb[i + 1] = h;
        }
    }
    __syncthreads();
    if (blockIdx.x == 0) {
        for (int i = threadIdx.x; i <= nqc; i += blockDim.x) lims[q0 + i] = qb[i];
        if (threadIdx.x == 0) total[parity ^ 1] = qb[nqc];
    }
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int64_t npairs = pre[nqc];
    for (int64_t p = (int64_t)blockIdx.x * 4 + wave; p < npairs; p += (int64_t)gridDim.x * 4) {
        const int q = ivr_last_le(pre, nqc, p);
        const int64_t at = (int64_t)q * cstride + (p - pre[q]);
        const uint64_t m = mask[at];
        if (m == 0) continue;
        const uint32_t g = cand[at];
        f32x4 acc[4];
        (void)range_group_scores(data, qtile, dp4, ntotal, g, q, radius, acc);
        if ((lane & 15) == (q & 15)) {
            const int64_t o = qb[q] + off[at];
#pragma unroll
            for (int t = 0; t < 4; ++t)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int rl = t * 16 + (lane >> 4) * 4 + r;
                    if ((m >> rl) & 1) {
                        const int64_t pos = o + __popcll(m & ((1ull << rl) - 1));
                        if (pos < cap) {
                            D[pos] = acc[t][r] + 0.f;
                            const int64_t row = (int64_t)g * kGroupRows + rl;
                            I[pos] = IDS ? ids[row] : id_base + row;
                        }
                    }
                }
        }
    }
}

// range-search workspace for the index's current capacity (grow-only): the counters, and 64 rows of mstride entries per buffer
int reserve_range(ivr_index *x) {
    int rc = ivr_reserve({{&x->rs_count, 128 * sizeof(uint32_t) + 2 * sizeof(int64_t)}}, true);
    if (rc != IVR_OK) return rc;
    const size_t n = (size_t)64 * x->mstride();
    return ivr_reserve({{&x->rs_cand, n * sizeof(uint32_t)}, {&x->rs_mask, n * sizeof(uint64_t)}, {&x->rs_off, n * sizeof(uint32_t)}});
}

// ivr_index_range_search over the rows of view v; the caller holds x->mu
int range_search_view(ivr_index *x, const View &v, const float *q, int nq, float radius, int normalize_q, int64_t *lims, float *D, int64_t *I,
                      int64_t cap, hipStream_t s) {
    const int64_t id_base = v.id_base;
    const int64_t ngroups = v.ngroups;
    if (ngroups == 0) {
        IVR_HIP(hipMemsetAsync(lims, 0, (size_t)(nq + 1) * sizeof(int64_t), s));
        return IVR_OK;
    }
    int rc = ivr_reserve_queries(x, (int)ivr_ceil_div(nq, 16));
    if (rc == IVR_OK) rc = ivr_reserve_gmax(x);
    if (rc == IVR_OK) rc = reserve_range(x);
    if (rc != IVR_OK) return rc;
    rc = ivr_launch_tile_rows(x, x->qtiled, q, 0, nq, normalize_q, nullptr, s);
    if (rc != IVR_OK) return rc;
    // chunks as in ivr_index_search; the bf16 candidate scan from the size at which the top-k search (k = 1) takes it
    const int chunk = 16 * x->qt_max();
    const bool fast = x->fast_scan(ngroups, 1);
    const int64_t mstride = x->mstride(), cstride = mstride;       // the candidate rows are as long as the group-maximum rows
    uint32_t *ncand = x->rs_count, *nhits = x->rs_count + 64;
    int64_t *total = reinterpret_cast<int64_t *>(x->rs_count + 128);
    const unsigned pgrid = (unsigned)std::max(1, x->ctx->cu_count * 4);     // persistent passes: 4 workgroups of 4 waves per CU
    for (int q0 = 0, c = 0; q0 < nq; q0 += chunk, ++c) {
        const int nqc = std::min(chunk, nq - q0);
        const int qt = pick_qt(nqc);
        const float *qtile = x->qtiled + (int64_t)(q0 / 16) * 16 * x->dp;
        if (fast) ivr_launch_fast_scan(x, v, qt, q0 / 16, s);
        else ivr_launch_scan_qt(x, v, qt, qtile, s);
        IVR_LAUNCH_CHECK();
        {
            IvrProf prof("range_candidates", s, (double)nqc * ngroups * 4, true);
            hipLaunchKernelGGL(range_candidates_kernel, dim3(nqc), dim3(1024), 0, s, x->gmax, mstride, ngroups, radius,
                               fast ? x->qnorm + q0 : (const float *)nullptr, x->rel_eps(), x->maxnorm, x->rs_cand, cstride, ncand);
            IVR_LAUNCH_CHECK();
        }
        {
            IvrProf prof("range_rescore", s, 0.0, true);     // the pairs are counted on the device
            with_mask(v.mask, [&](auto masked, auto... m) {
                hipLaunchKernelGGL((range_rescore_kernel<decltype(masked)::value, decltype(m)...>), dim3(pgrid), dim3(256), 0, s, v.data, qtile,
                                   x->dp4, v.ntotal, radius, nqc, x->rs_cand, cstride, ncand, x->rs_mask, x->rs_off, m...);
            });
            IVR_LAUNCH_CHECK();
        }
        {
            IvrProf prof("range_offsets", s, 0.0, true);
            hipLaunchKernelGGL(range_offsets_kernel, dim3(nqc), dim3(1024), 0, s, ncand, cstride, x->rs_off, nhits);
            IVR_LAUNCH_CHECK();
        }
        {
            IvrProf prof("range_write", s, 0.0, true);
            hipLaunchKernelGGL(v.ids ? range_write_kernel<true> : range_write_kernel<false>, dim3(pgrid), dim3(256), 0, s, v.data, qtile, x->dp4, v.ntotal, radius, nqc, q0,
                               x->rs_cand, cstride, ncand, x->rs_mask, x->rs_off, nhits, total, c == 0 ? 1 : 0, c & 1, lims, D, I, cap,
                               id_base, v.ids);
            IVR_LAUNCH_CHECK();
        }
    }
    return IVR_OK;
}

}  // namespace

extern "C" {

int ivr_index_range_search(ivr_index *x, const float *q, int nq, float radius, int normalize_q, int64_t id_base, int64_t *lims,
                           float *D, int64_t *I, int64_t cap, ivr_stream stream) {
    return ivr_index_range_search_filtered(x, q, nq, radius, normalize_q, id_base, nullptr, lims, D, I, cap, stream);
}

int ivr_index_range_search_filtered(ivr_index *x, const float *q, int nq, float radius, int normalize_q, int64_t id_base,
                                    const ivr_id_filter *filter, int64_t *lims, float *D, int64_t *I, int64_t cap, ivr_stream stream) {
    IVR_REQUIRE(x && q && lims && D && I, "ivr_index_range_search: NULL argument");
    IVR_REQUIRE(nq >= 1, "ivr_index_range_search: nq=%d", nq);
    IVR_REQUIRE(cap >= 0, "ivr_index_range_search: cap=%lld", (long long)cap);
    IVR_REQUIRE(!(radius != radius), "ivr_index_range_search: radius is NaN");
    return with_view(x, id_base, filter, (hipStream_t)stream, "ivr_index_range_search_filtered", [&](const View &v) {
        return range_search_view(x, v, q, nq, radius, normalize_q, lims, D, I, cap, (hipStream_t)stream);
    });
}

}  // extern "C"
