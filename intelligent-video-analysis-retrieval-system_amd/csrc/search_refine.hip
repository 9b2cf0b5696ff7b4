// Exact re-ranking of candidate lists on the flat index (ivr_index_rescore): faiss IndexFlat::compute_distance_subset, and the
// ordering pass that makes faiss IndexRefineFlat out of it.  DESIGN.md section 4, "re-ranking".
//
// Every query brings its own list of kc storage rows.  A candidate's score is accumulated by mfma_chunk4 in ascending chunk order from
// the float32 tiles of the storage and the tiled query buffer, from a zero accumulator: the sequence of every float32 score of the
// index (search_internal.h), so a (query, row) pair gets the bits ivr_index_search reports for it.  The bf16 scan copy is not read.
// A candidate row is addressed like a gathered row (search_rows.hip): tile r >> 4, slot r & 15, one 16-byte piece per 64-byte line of
// the tile, so a row costs 16 times its bytes in cache lines; nothing here hides that.
//
// Launches, both on the caller's stream:
//   refine_score  one wave per (query, 16 candidates), four waves to a workgroup, so that one query's list spreads over the grid:
//                 scores -> D_all and 64-bit keys (ordered score, ~row), key 0 for an absent entry
//   refine_order  one workgroup per query: bitonic sort of its kc keys in LDS, descending -> the first k as D / I.  Equal keys (a row
//                 named more than once) are legal here and end up in adjacent slots; select_topk_kernel (search_select.h) ranks by
//                 counting the keys above each one and needs them unique, so it is not used.
#include "ivr_common.h"
#include "search_internal.h"

#include <cfloat>

namespace {

struct RefineScore {
    const float4 *data;          // the float32 tiles of the storage
    const float4 *qtiled;        // the queries, tiled
    int dp4;
    int64_t ntotal;
    const int64_t *cand;         // [nq][kc] storage rows; outside [0, ntotal): absent
    int kc, groups;              // groups = ceil(kc / 16)
    int64_t nwaves;              // nq * groups
    uint64_t *keys;              // [nq][kc] or NULL
    float *D_all;                // [nq][kc] or NULL
};

// Wave w: query w / groups, candidates 16 g .. 16 g + 15 of its list, g = w % groups.  Lane l holds quad l >> 4 of every chunk of the
// row of candidate 16 g + (l & 15) (the A operand) and the same quad of the query (B: the query in all 16 columns), so after
// pair_score (search_internal.h; pa, pb: this lane's quad of chunk 0 of its candidate row and of the query; trips of 16, 4, then
// single chunks) acc[x] of lane l is the score of candidate 16 g + 4 (l >> 4) + x in every column; column 0 writes.  An absent
// lane reads row 0 and its score is dropped.  The host launches nothing on an empty index.
__global__ __launch_bounds__(256) void refine_score_kernel(RefineScore a) {
    const int lane = threadIdx.x & 63;
    const int64_t w = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (w >= a.nwaves) return;
    const int64_t q = w / a.groups;
    const int g = (int)(w - q * a.groups);
    const int j = 16 * g + (lane & 15), qd = lane >> 4;
    const int64_t c = j < a.kc ? a.cand[q * a.kc + j] : -1;
    const bool ok = c >= 0 && c < a.ntotal;
    const int64_t r = ok ? c : 0;
    const uint32_t row32 = ok ? (uint32_t)c : 0xFFFFFFFFu;      // the capacity of an index stays below 2^32 - 64 rows
    const int per_tile = a.dp4 * 16, kchunks = a.dp4 >> 2;
    const float4 *pa = a.data + (r >> 4) * per_tile + qd * 16 + (r & 15);
    const float4 *pb = a.qtiled + (q >> 4) * per_tile + qd * 16 + (q & 15);
    const f32x4 acc = pair_score<4>(pa, pb, kchunks);
    uint32_t rows[4];                                            // the rows of candidates 16 g + 4 qd + x, from a lane that holds them
#pragma unroll
    for (int x = 0; x < 4; ++x) rows[x] = __shfl(row32, 4 * qd + x, 64);
    if ((lane & 15) != 0) return;
#pragma unroll
    for (int x = 0; x < 4; ++x) {
        const int jj = 16 * g + 4 * qd + x;
        if (jj >= a.kc) continue;
        const bool present = rows[x] != 0xFFFFFFFFu;
        const uint32_t ord = ivr_f2ord(acc[x]);
        const int64_t at = q * a.kc + jj;
        if (a.keys) a.keys[at] = present ? ((uint64_t)ord << 32) | (uint32_t)(0xFFFFFFFFu - rows[x]) : 0ull;
        if (a.D_all) a.D_all[at] = present ? ivr_ord2f(ord) : -FLT_MAX;
    }
}

// One workgroup per query: its kc keys, padded with absent ones to P = a power of two, sorted descending in LDS; slot j < k gets the
// j-th key's score and row, (-FLT_MAX, -1) once the present candidates run out.
__global__ __launch_bounds__(1024) void refine_order_kernel(const uint64_t *__restrict__ keys, int kc, int P, int k, float *__restrict__ D,
                                                            int64_t *__restrict__ I) {
    __shared__ uint64_t s[IVR_MAX_K];
    const int tid = threadIdx.x, nthr = blockDim.x;
    const uint64_t *c = keys + (int64_t)blockIdx.x * kc;
    for (int i = tid; i < P; i += nthr) s[i] = i < kc ? c[i] : 0ull;
    __syncthreads();
    for (int size = 2; size <= P; size <<= 1) {
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int i = tid; i < (P >> 1); i += nthr) {
                const int lo = ((i / stride) * stride << 1) + (i % stride), hi = lo + stride;
                const bool desc = (lo & size) == 0;
                const uint64_t x = s[lo], y = s[hi];
                if ((x < y) == desc) {
                    s[lo] = y;
                    s[hi] = x;
                }
            }
            __syncthreads();
        }
    }
    for (int i = tid; i < k; i += nthr) {
        const uint64_t key = s[i];
        D[(int64_t)blockIdx.x * k + i] = key ? ivr_ord2f((uint32_t)(key >> 32)) : -FLT_MAX;
        I[(int64_t)blockIdx.x * k + i] = key ? (int64_t)(0xFFFFFFFFu - (uint32_t)key) : -1;
    }
}

// every result absent: an empty index
__global__ __launch_bounds__(256) void refine_absent_kernel(int64_t nall, float *__restrict__ D_all, int64_t nsel, float *__restrict__ D,
                                                            int64_t *__restrict__ I) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (D_all && i < nall) D_all[i] = -FLT_MAX;
    if (D && i < nsel) {
        D[i] = -FLT_MAX;
        I[i] = -1;
    }
}

// block size of the ordering pass by key count, as sel_threads (search_select.h): short lists pay for fewer waves at every barrier
int order_threads(int P) { return P <= 512 ? 256 : 1024; }

}  // namespace

// search_internal.h.  Stages the queries and launches refine_score over the whole lists
int ivr_launch_refine_score(ivr_index *x, const float *q, int nq, const int64_t *cand, int kc, int normalize_q, uint64_t *keys, float *D_all,
                            hipStream_t s) {
    int rc = ivr_reserve_queries(x, (int)ivr_ceil_div(nq, 16));
    if (rc != IVR_OK) return rc;
    rc = ivr_launch_tile_rows(x, x->qtiled, q, 0, nq, normalize_q, nullptr, s);
    if (rc != IVR_OK) return rc;
    const int64_t nall = (int64_t)nq * kc;
    const int groups = (int)ivr_ceil_div(kc, 16);
    const int64_t nwaves = (int64_t)nq * groups;
    // algorithmic bytes: every candidate row once + its table entry, key and score (the lines that move are 16 times the rows)
    IvrProf prof("refine_score", s, (double)nall * x->dp * 4 + (double)nall * 20);
    const RefineScore a{reinterpret_cast<const float4 *>(x->data), reinterpret_cast<const float4 *>((const float *)x->qtiled), x->dp4, x->ntotal,
                        cand, kc, groups, nwaves, keys, D_all};
    hipLaunchKernelGGL(refine_score_kernel, dim3((unsigned)ivr_ceil_div(nwaves, 4)), dim3(256), 0, s, a);
    IVR_LAUNCH_CHECK();
    return IVR_OK;
}

extern "C" {

int ivr_index_rescore(ivr_index *x, const float *q, int nq, const int64_t *cand, int kc, int k, int normalize_q, float *D_all, float *D,
                      int64_t *I, ivr_stream stream) {
    IVR_REQUIRE(x && q && cand, "ivr_index_rescore: NULL argument");
    IVR_REQUIRE(nq >= 1, "ivr_index_rescore: nq=%d", nq);
    IVR_REQUIRE(kc >= 1 && kc <= IVR_MAX_K, "ivr_index_rescore: kc=%d outside [1,%d]", kc, IVR_MAX_K);
    IVR_REQUIRE((int64_t)nq * kc < (1ll << 31), "ivr_index_rescore: nq * kc = %lld outside [1, 2^31)", (long long)nq * kc);
    IVR_REQUIRE((D == nullptr) == (I == nullptr), "ivr_index_rescore: D and I go together");
    IVR_REQUIRE(D_all || D, "ivr_index_rescore: no output requested");
    IVR_REQUIRE(!D || (k >= 1 && k <= kc), "ivr_index_rescore: k=%d outside [1,kc=%d]", k, kc);
    hipStream_t s = (hipStream_t)stream;
    std::lock_guard<std::mutex> lk(x->mu);
    IVR_HIP(hipSetDevice(x->ctx->device));
    const int64_t nall = (int64_t)nq * kc, nsel = D ? (int64_t)nq * k : 0;
    if (x->ntotal == 0) {
        hipLaunchKernelGGL(refine_absent_kernel, dim3((unsigned)ivr_ceil_div(std::max(nall, nsel), 256)), dim3(256), 0, s, nall, D_all, nsel, D, I);
        IVR_LAUNCH_CHECK();
        return IVR_OK;
    }
    int rc = D ? ivr_reserve({{&x->refine_keys, (size_t)nall * 8}}) : IVR_OK;
    if (rc != IVR_OK) return rc;
    rc = ivr_launch_refine_score(x, q, nq, cand, kc, normalize_q, D ? (uint64_t *)x->refine_keys : nullptr, D_all, s);
    if (rc != IVR_OK) return rc;
    if (D) {
        int P = 2;
        while (P < kc) P <<= 1;
        IvrProf prof("refine_order", s, (double)nall * 8 + (double)nsel * 12, true);
        hipLaunchKernelGGL(refine_order_kernel, dim3((unsigned)nq), dim3(order_threads(P)), 0, s, (const uint64_t *)x->refine_keys, kc, P, k, D, I);
        IVR_LAUNCH_CHECK();
    }
    return IVR_OK;
}

}  // extern "C"
