// Diversified search on the flat index (ivr_index_diversify): maximal marginal relevance and near-duplicate suppression over a
// candidate list, the greedy selection on the device.  DESIGN.md section 4, "diversified search".
//
// Every query brings its own list of kc storage rows, as for ivr_index_rescore.  R[j] is the relevance of candidate j (refine_score as
// it is, so the bits of ivr_index_search), P[s, j] the score of candidate j with the stored row of candidate s as the query, m[j] the
// greatest P[s, j] over the rows chosen so far.  Step t chooses the live candidate with the greatest (value, ~row, lower position):
//   MMR       value = R[j] at t = 0, then (lambda * R[j]) - (mu * m[j]), three roundings, mu = 1.0f - lambda
//   suppress  value = R[j]; a candidate whose m[j] reaches the threshold is out for good, and the selection ends when none is left
// P is never materialised: after each choice the block scores row s against all live candidates (k * kc * d multiply-adds per query
// instead of kc * kc * d), with pair_score, so every P[s, j] has the bits ivr_index_rescore reports for (query = stored row s, row j).
//
// Launches, both on the caller's stream:
//   refine_score    (search_refine.hip) the relevance of every candidate -> x->dv_scores
//   diverse_select  one workgroup per query, k steps of (pick the best live candidate, score the chosen row against the others)
#include "ivr_common.h"
#include "search_internal.h"
#include "search_lists.h"

#include <cfloat>
#include <climits>

namespace {

struct DiverseSelect {
    const float4 *data;          // the float32 tiles of the storage
    int dp4;
    int64_t ntotal;
    const int64_t *cand;         // [nq][kc] storage rows; outside [0, ntotal): absent
    const float *R;              // [nq][kc] relevance of every candidate (not read for an absent one)
    int kc, k;
    float lambda, mu;            // MMR
    float threshold;             // suppress
    const int64_t *ids;          // id-mapped index: the label of row r is ids[r]; NULL: r
    float *D;                    // [nq][k]
    int64_t *I;                  // [nq][k]
    float *M;                    // [nq][k] or NULL
};

// state of a candidate: absent from the start, live, or out (chosen, or suppressed by a chosen row)
enum : uint8_t { kAbsent = 0, kLive = 1, kOut = 2 };

// (key, position) ranks above (okey, opos): the greater key, equal keys (a row named twice) the lower position.  "No candidate" is
// (0, INT_MAX), below every real pair
__device__ __forceinline__ bool ranks_above(uint64_t key, int pos, uint64_t okey, int opos) { return key > okey || (key == okey && pos < opos); }

// One workgroup per query.  LDS: R, m, the 32-bit row and the state of every candidate, 13 bytes each, and one (key, position) per wave.
// A step: every thread ranks its candidates j = tid, tid + THREADS, ..., a butterfly over the wave and a pass over the waves' winners
// give the choice s to every thread; thread 0 writes the result slot; then wave w scores the groups w, w + NW, ... of 16 candidates
// against row s as refine_score scores them against a query: lane l holds quad l >> 4 of every chunk of the row of candidate
// 16 g + (l & 15) (A) and the same quad of row s read from the storage tiles as they lie (B: row s in all 16 columns), so acc[x] of
// lane l is P[s, 16 g + 4 (l >> 4) + x] in every column and the column-0 lanes fold it into m.  A group without a live candidate is
// skipped.  An absent lane reads row 0; a choice exists only when a candidate is present, so row 0 is stored then.
template <int THREADS, bool MMR>
__global__ __launch_bounds__(THREADS) void diverse_select_kernel(DiverseSelect a) {
    SQ_NO_CONTRACT
    constexpr int NW = THREADS / 64;
    __shared__ float sR[IVR_MAX_K], sm[IVR_MAX_K];
    __shared__ uint32_t srow[IVR_MAX_K];
    __shared__ uint8_t sstate[IVR_MAX_K];
    __shared__ uint64_t wkey[NW];
    __shared__ int wpos[NW];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, qd = lane >> 4;
    const int64_t q = blockIdx.x;
    const int per_tile = a.dp4 * 16, kchunks = a.dp4 >> 2, groups = (a.kc + 15) >> 4;
    for (int j = tid; j < a.kc; j += THREADS) {
        const int64_t c = a.cand[q * a.kc + j];
        const bool ok = c >= 0 && c < a.ntotal;
        srow[j] = ok ? (uint32_t)c : 0xFFFFFFFFu;                // the capacity of an index stays below 2^32 - 64 rows
        sR[j] = ok ? a.R[q * a.kc + j] : -FLT_MAX;
        sm[j] = -FLT_MAX;
        sstate[j] = ok ? kLive : kAbsent;
    }
    __syncthreads();
    int t = 0;
    for (; t < a.k; ++t) {
        uint64_t bkey = 0;
        int bpos = INT_MAX;
        for (int j = tid; j < a.kc; j += THREADS) {
            if (sstate[j] != kLive) continue;
            float v = sR[j];
            if (MMR && t > 0) {
                const float rel = a.lambda * sR[j];
                const float red = a.mu * sm[j];
                v = rel - red;
            }
            const uint64_t key = ivr_key(v, srow[j]);
            if (ranks_above(key, j, bkey, bpos)) {
                bkey = key;
                bpos = j;
            }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const uint32_t hi = __shfl_xor((uint32_t)(bkey >> 32), o, 64), lo = __shfl_xor((uint32_t)bkey, o, 64);
            const int opos = __shfl_xor(bpos, o, 64);
            const uint64_t okey = ((uint64_t)hi << 32) | lo;
            if (ranks_above(okey, opos, bkey, bpos)) {
                bkey = okey;
                bpos = opos;
            }
        }
        if (lane == 0) {
            wkey[wave] = bkey;
            wpos[wave] = bpos;
        }
        __syncthreads();
        bkey = wkey[0];
        bpos = wpos[0];
#pragma unroll
        for (int w = 1; w < NW; ++w)
            if (ranks_above(wkey[w], wpos[w], bkey, bpos)) {
                bkey = wkey[w];
                bpos = wpos[w];
            }
        const int s = bpos;
        if (s == INT_MAX) break;                                  // nothing live is left: the same for every thread
        const uint32_t rs = srow[s];
        if (tid == 0) {
            const int64_t at = q * a.k + t;
            a.D[at] = sR[s];
            a.I[at] = a.ids ? a.ids[rs] : (int64_t)rs;
            if (a.M) a.M[at] = sm[s];                             // -FLT_MAX at t = 0; nobody else touches m[s] in this step
            sstate[s] = kOut;
        }
        if (t + 1 < a.k) {
            const float4 *pb = a.data + (int64_t)(rs >> 4) * per_tile + qd * 16 + (rs & 15);
            for (int g = wave; g < groups; g += NW) {
                const int j = 16 * g + (lane & 15);
                const bool live = j < a.kc && j != s && sstate[j] == kLive;     // j != s first: thread 0 is writing state[s]
                if (__ballot(live) == 0) continue;
                const uint32_t r32 = j < a.kc ? srow[j] : 0xFFFFFFFFu;
                const int64_t r = r32 != 0xFFFFFFFFu ? (int64_t)r32 : 0;
                const float4 *pa = a.data + (r >> 4) * per_tile + qd * 16 + (r & 15);
                const f32x4 acc = pair_score<4>(pa, pb, kchunks);
                if ((lane & 15) == 0) {
#pragma unroll
                    for (int x = 0; x < 4; ++x) {
                        const int jj = 16 * g + 4 * qd + x;
                        if (jj >= a.kc || jj == s || sstate[jj] != kLive) continue;
                        const float p = ivr_ord2f(ivr_f2ord(acc[x]));           // as ivr_index_rescore reports it: -0.0 as +0.0
                        const float mx = p > sm[jj] ? p : sm[jj];
                        sm[jj] = mx;
                        if (!MMR && mx >= a.threshold) sstate[jj] = kOut;
                    }
                }
            }
            __syncthreads();
        }
    }
    for (int i = t + tid; i < a.k; i += THREADS) {                // the slots behind an early end
        const int64_t at = q * a.k + i;
        a.D[at] = -FLT_MAX;
        a.I[at] = -1;
        if (a.M) a.M[at] = -FLT_MAX;
    }
}

// block size by list length, as the ordering pass of the re-ranking (search_refine.hip): short lists pay for fewer waves at every barrier
int select_threads(int kc) { return kc <= 512 ? 256 : 1024; }

template <bool MMR>
void launch_select(const DiverseSelect &a, int nq, hipStream_t s) {
    if (select_threads(a.kc) == 256) hipLaunchKernelGGL((diverse_select_kernel<256, MMR>), dim3((unsigned)nq), dim3(256), 0, s, a);
    else hipLaunchKernelGGL((diverse_select_kernel<1024, MMR>), dim3((unsigned)nq), dim3(1024), 0, s, a);
}

}  // namespace

extern "C" {

int ivr_index_diversify(ivr_index *x, const float *q, int nq, const int64_t *cand, int kc, int k, int mode, float param, int normalize_q,
                        float *D, int64_t *I, float *M, ivr_stream stream) {
    IVR_REQUIRE(x && q && cand && D && I, "ivr_index_diversify: NULL argument");
    IVR_REQUIRE(nq >= 1, "ivr_index_diversify: nq=%d < 1", nq);
    IVR_REQUIRE(kc >= 1 && kc <= IVR_MAX_K, "ivr_index_diversify: kc=%d outside [1,%d]", kc, IVR_MAX_K);
    IVR_REQUIRE(k >= 1 && k <= kc, "ivr_index_diversify: k=%d outside [1,kc=%d]", k, kc);
    IVR_REQUIRE((int64_t)nq * kc < (1ll << 31), "ivr_index_diversify: nq * kc = %lld outside [1, 2^31)", (long long)nq * kc);
    IVR_REQUIRE(mode == IVR_DIVERSE_MMR || mode == IVR_DIVERSE_SUPPRESS, "ivr_index_diversify: mode=%d is neither IVR_DIVERSE_MMR nor IVR_DIVERSE_SUPPRESS", mode);
    IVR_REQUIRE(param == param, "ivr_index_diversify: param=%g is NaN", (double)param);
    IVR_REQUIRE(mode != IVR_DIVERSE_MMR || (param >= 0.0f && param <= 1.0f), "ivr_index_diversify: lambda=%g outside [0,1]", (double)param);
    hipStream_t s = (hipStream_t)stream;
    std::lock_guard<std::mutex> lk(x->mu);
    IVR_HIP(hipSetDevice(x->ctx->device));
    const int64_t nall = (int64_t)nq * kc;
    if (x->ntotal > 0) {
        int rc = ivr_reserve({{&x->dv_scores, (size_t)nall * 4}});
        if (rc != IVR_OK) return rc;
        rc = ivr_launch_refine_score(x, q, nq, cand, kc, normalize_q, nullptr, x->dv_scores, s);
        if (rc != IVR_OK) return rc;
    }
    // on an empty index every entry is absent: the selection reads no score and no row and fills the slots
    const DiverseSelect a{reinterpret_cast<const float4 *>(x->data), x->dp4, x->ntotal, cand, x->dv_scores, kc, k,
                          param, 1.0f - param, param, x->has_ids ? x->ids : nullptr, D, I, M};
    // algorithmic bytes: the chosen row and every candidate row once per step but the last
    IvrProf prof("diverse_select", s, (double)nall * (k - 1) * x->dp * 4 + (double)nall * 12);
    if (mode == IVR_DIVERSE_MMR) launch_select<true>(a, nq, s);
    else launch_select<false>(a, nq, s);
    IVR_LAUNCH_CHECK();
    return IVR_OK;
}

}  // extern "C"
