// The graph index (ivr_graph): HNSW's neighbour-selection heuristic over candidate lists (ivr_graph_prune) and the best-first walk
// of a fixed-degree graph (ivr_graph_search).  DESIGN.md section 4, "graph index"; the definitions both kernels are pinned to
// element for element are the numpy functions of ivr_amd/graph.py.
//
// Rows: a row-major float32 copy, each row padded with zeros to dp = a multiple of 16 floats, so that the four lanes that hold the
// quads of one 16-float chunk of a row read 64 contiguous bytes.  Every score is accumulated by mfma_chunk4 in ascending chunk order
// from a zero accumulator, which is the summation order of every float32 score of the flat index: the same pair gives the same
// bits.  (The MFMA multiplies the two operands of a pair commutatively, so which of them is A and which is B does not matter.)
//
// Search: one workgroup of four waves per query.  L, the candidate list, is an array of 64-bit (ordered score, ~row) keys in
// descending order in LDS with one expanded flag per entry; both are double-buffered.  One step:
//   pick     the first entry of L that is not expanded (atomic minimum of the positions); none: stop
//   read     the `degree` neighbours of that row; entries outside [0, ntotal) become -1
//   drop     a neighbour that is -1, that is in L (a scan of L's rows), or that repeats an earlier neighbour
//   compact  the survivors, in order, by one ballot
//   score    sixteen survivors to a wave: the query (from LDS) is the A operand, lane l holds quad l >> 4 of row l & 15
//   merge    every old and every new key computes its position in the merged order (own index + keys of the other set above it;
//            the keys are distinct), positions >= ef fall off
// The entry rows go through the same steps against an empty L.  There is no visited set: a row that was rejected or pushed out has
// a key below L's worst, and L's worst only improves, so offering it again changes nothing.
// Every loop is bounded: steps by max_expansions (clamped to [1, ntotal] by the host), the rest by degree, ef and dp.
#include "search_internal.h"

#include <climits>

namespace {

constexpr int kGraphMaxEf = IVR_GRAPH_MAX_EF;
constexpr int kGraphMaxCand = IVR_GRAPH_MAX_CAND;
constexpr int kGraphMaxDegree = IVR_GRAPH_MAX_DEGREE;
constexpr int kGraphMaxDim = 8192;       // the staged query takes 4 dp bytes of LDS
constexpr int64_t kGraphMaxBlocks = 1 << 22;   // blocks of 256 per launch: a launch of 2^32 threads or more is refused by the runtime
static_assert(kGraphMaxEf == 256, "the search kernel scans L in four parts of 64 with 256 threads");
static_assert(kGraphMaxCand == 64 && kGraphMaxDegree == 64, "one wave holds a candidate list / a neighbour list");

}  // namespace

struct ivr_graph {
    ivr_ctx *ctx = nullptr;
    int d = 0, dp = 0, degree = 0;
    int64_t cap = 0, ntotal = 0;         // rows allocated / stored
    float *rows = nullptr;               // [cap][dp]
    int32_t *nbr = nullptr;              // [cap][degree]
    int64_t nbr_rows = 0;                // rows of the installed neighbour table (0: none)
    std::mutex mu;
    DevBuf<float> qn;                    // [nq][d] normalised queries (normalize_q only), grow-only
};

namespace {

// Grid-stride over the n * dp padded floats: the grid is capped (kGraphMaxBlocks), so any n < 2^31 is one launch.
__global__ __launch_bounds__(256) void graph_pad_rows_kernel(const float *__restrict__ src, float *__restrict__ dst, int64_t n, int d, int dp) {
    const int64_t total = n * dp, stride = (int64_t)gridDim.x * 256;
    for (int64_t i = blockIdx.x * 256ll + threadIdx.x; i < total; i += stride) {
        const int64_t r = i / dp;
        const int c = (int)(i - r * dp);
        dst[i] = c < d ? src[r * d + c] : 0.f;
    }
}

// One workgroup per base row r = r0 + blockIdx.x (the host launches at most kGraphMaxBlocks rows at a time).
// Wave w multiplies candidates 16 w .. 16 w + 15 (A operand) against every 16-candidate tile (B) and
// against the base row (B: the base in every column): G[i][j] = <cand i, cand j>, sb[i] = <r, cand i>.  Wave 0 then walks the
// candidates: lane i holds the i-th kept candidate and tests the current one against it.
__global__ __launch_bounds__(256) void graph_prune_kernel(const float *__restrict__ rows, int dp, int64_t ntotal, int64_t r0,
                                                          const int32_t *__restrict__ cand, int C, int M, int32_t *__restrict__ nbr,
                                                          float *__restrict__ nbr_score) {
    __shared__ float G[kGraphMaxCand][kGraphMaxCand + 1];
    __shared__ float sb[kGraphMaxCand];
    __shared__ int s_c[kGraphMaxCand];
    const int64_t r = r0 + blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid < kGraphMaxCand) {
        const int c = tid < C ? cand[r * C + tid] : -1;
        s_c[tid] = c >= 0 && c < ntotal ? c : -1;
    }
    __syncthreads();
    const int tiles = (C + 15) >> 4;
    if (wave < tiles) {
        const int g = lane >> 4, li = lane & 15;
        const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
        const int ca = s_c[16 * wave + li];
        const float4 *pa = ca >= 0 ? reinterpret_cast<const float4 *>(rows + (int64_t)ca * dp) + g : nullptr;
        const float4 *pb[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int cb = s_c[16 * t + li];
            pb[t] = t < tiles && cb >= 0 ? reinterpret_cast<const float4 *>(rows + (int64_t)cb * dp) + g : nullptr;
        }
        const float4 *pr = reinterpret_cast<const float4 *>(rows + r * dp) + g;
        f32x4 acc[5];
#pragma unroll
        for (int t = 0; t < 5; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
        const int kchunks = dp >> 4;
        for (int kc = 0; kc < kchunks; ++kc) {
            const float4 a = pa ? pa[kc * 4] : zero;
            const float4 base = pr[kc * 4];
            float4 b[4];
#pragma unroll
            for (int t = 0; t < 4; ++t) b[t] = pb[t] ? pb[t][kc * 4] : zero;
#pragma unroll
            for (int t = 0; t < 4; ++t) mfma_chunk4(acc[t], a, b[t]);
            mfma_chunk4(acc[4], a, base);
        }
        // acc[t][x] = <cand 16 wave + 4 g + x, cand 16 t + li>; acc[4][x] = <cand 16 wave + 4 g + x, base>
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            if (t < tiles) {
#pragma unroll
                for (int x = 0; x < 4; ++x) G[16 * wave + 4 * g + x][16 * t + li] = acc[t][x] + 0.0f;
            }
        }
        if (li == 0) {
#pragma unroll
            for (int x = 0; x < 4; ++x) sb[16 * wave + 4 * g + x] = acc[4][x] + 0.0f;
        }
    }
    __syncthreads();
    if (wave != 0) return;
    int nkept = 0, mine = 0;
    for (int ci = 0; ci < C && nkept < M; ++ci) {
        if (s_c[ci] < 0) continue;
        const float sbc = sb[ci];
        const bool bad = lane < nkept && !(G[ci][mine] <= sbc);      // a kept neighbour is closer to the candidate than the base is
        if (__ballot(bad) == 0ull) {
            if (lane == nkept) mine = ci;
            ++nkept;
        }
    }
    if (lane < M) {
        nbr[r * M + lane] = lane < nkept ? s_c[mine] : -1;
        nbr_score[r * M + lane] = lane < nkept ? sb[mine] : 0.f;
    }
}

struct GraphSearch {
    const float *rows;
    int dp, d;
    int64_t ntotal;
    const int32_t *graph;
    int degree;
    const float *q;
    int k, ef;
    const int32_t *entries;
    int ne;
    int max_exp;
    float *D;
    int64_t *I;
    int32_t *nexp;
};

__device__ __forceinline__ int graph_key_row(uint64_t key) { return (int)(0xFFFFFFFFu - (uint32_t)key); }

__global__ __launch_bounds__(256) void graph_search_kernel(GraphSearch a) {
    extern __shared__ __attribute__((aligned(16))) float4 qs[];      // the query: dp floats, zero past d
    __shared__ uint64_t s_L[2][kGraphMaxEf];
    __shared__ uint8_t s_F[2][kGraphMaxEf];
    __shared__ uint64_t s_new[kGraphMaxDegree];
    __shared__ int s_nb[kGraphMaxDegree], s_drop[kGraphMaxDegree], s_row[kGraphMaxDegree];
    __shared__ int s_nnew, s_cur;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t qi = blockIdx.x;
    for (int i = tid; i < a.dp; i += 256) reinterpret_cast<float *>(qs)[i] = i < a.d ? a.q[qi * a.d + i] : 0.f;
    int len = 0, buf = 0, nexp = 0;
    // step -1 offers the entry rows to the empty list; steps 0 .. max_exp - 1 expand
    for (int it = -1; it < a.max_exp; ++it) {
        const int32_t *src;
        int cnt, cur = -1;
        if (it < 0) {
            src = a.entries + qi * a.ne;
            cnt = a.ne;
        } else {
            if (tid == 0) s_cur = INT_MAX;
            __syncthreads();
            if (tid < len && !s_F[buf][tid]) atomicMin(&s_cur, tid);
            __syncthreads();
            cur = s_cur;
            if (cur == INT_MAX) break;               // the same value in every thread
            src = a.graph + (int64_t)graph_key_row(s_L[buf][cur]) * a.degree;
            cnt = a.degree;
            ++nexp;
        }
        if (tid < kGraphMaxDegree) {
            int nb = tid < cnt ? src[tid] : -1;
            if (nb < 0 || nb >= a.ntotal) nb = -1;
            s_nb[tid] = nb;
            s_drop[tid] = nb < 0;
            if (tid == 0 && cur >= 0) s_F[buf][cur] = 1;
        }
        __syncthreads();
        {   // thread (j, part): neighbour j against part `part` of L and against part `part` of the neighbours in front of it
            const int j = lane, part = wave;
            const int nb = s_nb[j];
            if (nb >= 0) {
                bool hit = false;
                const int hi = min(len, part * 64 + 64);
                for (int i = part * 64; i < hi; ++i) hit |= graph_key_row(s_L[buf][i]) == nb;
                const int hj = min(j, part * 16 + 16);
                for (int i = part * 16; i < hj; ++i) hit |= s_nb[i] == nb;
                if (hit) s_drop[j] = 1;
            }
        }
        __syncthreads();
        if (wave == 0) {
            const bool keep = !s_drop[lane];
            const uint64_t mask = __ballot(keep);
            if (keep) s_row[__popcll(mask & ((1ull << lane) - 1ull))] = s_nb[lane];
            if (lane == 0) s_nnew = __popcll(mask);
        }
        __syncthreads();
        const int nnew = s_nnew;
        if (wave * 16 < nnew) {
            const int g = lane >> 4, idx = wave * 16 + (lane & 15);
            const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
            const float4 *pr = idx < nnew ? reinterpret_cast<const float4 *>(a.rows + (int64_t)s_row[idx] * a.dp) + g : nullptr;
            f32x4 acc = {0.f, 0.f, 0.f, 0.f};
            const int kchunks = a.dp >> 4;
            int kc = 0;
            for (; kc + 8 <= kchunks; kc += 8) {
                float4 rv[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) rv[u] = pr ? pr[(kc + u) * 4] : zero;
#pragma unroll
                for (int u = 0; u < 8; ++u) mfma_chunk4(acc, qs[(kc + u) * 4 + g], rv[u]);
            }
            for (; kc < kchunks; ++kc) mfma_chunk4(acc, qs[kc * 4 + g], pr ? pr[kc * 4] : zero);
            // every A row is the query: acc[0] of lane l < 16 = <query, survivor 16 wave + l>
            if (lane < 16 && idx < nnew) s_new[idx] = ivr_key(acc[0], (uint32_t)s_row[idx]);
        }
        __syncthreads();
        const int nbuf = buf ^ 1;
        if (tid < len) {
            const uint64_t key = s_L[buf][tid];
            int pos = tid;
            for (int i = 0; i < nnew; ++i) pos += s_new[i] > key;
            if (pos < a.ef) {
                s_L[nbuf][pos] = key;
                s_F[nbuf][pos] = s_F[buf][tid];
            }
        }
        if (tid < nnew) {
            const uint64_t key = s_new[tid];
            int lo = 0, hi = len;                    // lo = keys of L above this one (L is descending)
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (s_L[buf][mid] > key) lo = mid + 1;
                else hi = mid;
            }
            int pos = lo;
            for (int i = 0; i < nnew; ++i) pos += s_new[i] > key;
            if (pos < a.ef) {
                s_L[nbuf][pos] = key;
                s_F[nbuf][pos] = 0;
            }
        }
        __syncthreads();
        len = min(a.ef, len + nnew);
        buf = nbuf;
    }
    for (int i = tid; i < a.k; i += 256) {
        const uint64_t key = i < len ? s_L[buf][i] : 0ull;
        a.D[qi * a.k + i] = i < len ? ivr_ord2f((uint32_t)(key >> 32)) : -FLT_MAX;
        a.I[qi * a.k + i] = i < len ? (int64_t)graph_key_row(key) : -1;
    }
    if (tid == 0 && a.nexp) a.nexp[qi] = nexp;
}

}  // namespace

extern "C" {

int ivr_graph_max_ef(void) { return kGraphMaxEf; }
int ivr_graph_max_cand(void) { return kGraphMaxCand; }

int ivr_graph_create(ivr_ctx *ctx, int d, int degree, ivr_graph **out) {
    IVR_REQUIRE(ctx && out, "ivr_graph_create: NULL argument");
    IVR_REQUIRE(d >= 1 && d <= kGraphMaxDim, "ivr_graph_create: d=%d out of range [1,%d]", d, kGraphMaxDim);
    IVR_REQUIRE(degree >= 1 && degree <= kGraphMaxDegree, "ivr_graph_create: degree=%d out of range [1,%d]", degree, kGraphMaxDegree);
    ivr_graph *g = new ivr_graph();
    g->ctx = ctx;
    g->d = d;
    g->dp = (int)ivr_round_up(d, 16);
    g->degree = degree;
    *out = g;
    return IVR_OK;
}

int ivr_graph_destroy(ivr_graph *g) {
    if (!g) return IVR_OK;
    if (g->rows) (void)hipFree(g->rows);
    if (g->nbr) (void)hipFree(g->nbr);
    delete g;
    return IVR_OK;
}

int ivr_graph_reset(ivr_graph *g) {
    IVR_REQUIRE(g, "ivr_graph_reset: NULL graph");
    std::lock_guard<std::mutex> lk(g->mu);
    g->ntotal = 0;
    g->nbr_rows = 0;
    return IVR_OK;
}

int64_t ivr_graph_ntotal(ivr_graph *g) { return g ? g->ntotal : 0; }

int ivr_graph_set_rows(ivr_graph *g, const float *rows, int64_t n, ivr_stream stream) {
    IVR_REQUIRE(g && (rows || n == 0), "ivr_graph_set_rows: NULL argument");
    IVR_REQUIRE(n >= 0 && n < (1ll << 31) - 1, "ivr_graph_set_rows: n=%lld out of range", (long long)n);
    std::lock_guard<std::mutex> lk(g->mu);
    IVR_HIP(hipSetDevice(g->ctx->device));
    g->nbr_rows = 0;
    if (n > g->cap) {
        IVR_HIP(hipDeviceSynchronize());         // a search in flight still reads the old blocks
        if (g->rows) (void)hipFree(g->rows);
        if (g->nbr) (void)hipFree(g->nbr);
        g->rows = nullptr;
        g->nbr = nullptr;
        g->cap = 0;
        g->ntotal = 0;
        IVR_HIP(hipMalloc(&g->rows, (size_t)n * g->dp * sizeof(float)));
        IVR_HIP(hipMalloc(&g->nbr, (size_t)n * g->degree * sizeof(int32_t)));
        g->cap = n;
    }
    g->ntotal = n;
    if (n == 0) return IVR_OK;
    hipStream_t s = (hipStream_t)stream;
    IvrProf prof("graph_set_rows", s, (double)n * (g->d + g->dp) * 4, true);
    const int64_t blocks = std::min<int64_t>(ivr_ceil_div(n * g->dp, 256), kGraphMaxBlocks);
    hipLaunchKernelGGL(graph_pad_rows_kernel, dim3((unsigned)blocks), dim3(256), 0, s, rows, g->rows, n, g->d, g->dp);
    IVR_LAUNCH_CHECK();
    return IVR_OK;
}

int ivr_graph_prune(ivr_graph *g, const int32_t *cand, int C, int M, int32_t *nbr, float *nbr_score, ivr_stream stream) {
    IVR_REQUIRE(g && cand && nbr && nbr_score, "ivr_graph_prune: NULL argument");
    IVR_REQUIRE(C >= 1 && C <= kGraphMaxCand, "ivr_graph_prune: C=%d outside [1,%d]", C, kGraphMaxCand);
    IVR_REQUIRE(M >= 1 && M <= 64, "ivr_graph_prune: M=%d outside [1,64]", M);
    std::lock_guard<std::mutex> lk(g->mu);
    if (g->ntotal == 0) return IVR_OK;
    IVR_HIP(hipSetDevice(g->ctx->device));
    hipStream_t s = (hipStream_t)stream;
    IvrProf prof("graph_prune", s, 2.0 * (double)g->ntotal * (C + 1) * C * g->dp);
    for (int64_t r0 = 0; r0 < g->ntotal; r0 += kGraphMaxBlocks) {
        const int64_t nb = std::min<int64_t>(kGraphMaxBlocks, g->ntotal - r0);
        hipLaunchKernelGGL(graph_prune_kernel, dim3((unsigned)nb), dim3(256), 0, s, (const float *)g->rows, g->dp, g->ntotal, r0, cand, C, M, nbr,
                           nbr_score);
        IVR_LAUNCH_CHECK();
    }
    return IVR_OK;
}

int ivr_graph_set_neighbors(ivr_graph *g, const int32_t *graph, int64_t n, ivr_stream stream) {
    IVR_REQUIRE(g && (graph || n == 0), "ivr_graph_set_neighbors: NULL argument");
    std::lock_guard<std::mutex> lk(g->mu);
    IVR_REQUIRE(n == g->ntotal, "ivr_graph_set_neighbors: n=%lld, the object holds %lld rows", (long long)n, (long long)g->ntotal);
    if (n == 0) return IVR_OK;
    IVR_HIP(hipSetDevice(g->ctx->device));
    IVR_HIP(hipMemcpyAsync(g->nbr, graph, (size_t)n * g->degree * sizeof(int32_t), hipMemcpyDeviceToDevice, (hipStream_t)stream));
    g->nbr_rows = n;
    return IVR_OK;
}

int ivr_graph_search(ivr_graph *g, const float *q, int nq, int k, int ef, const int32_t *entries, int ne, int max_expansions, int normalize_q,
                     float *D, int64_t *I, int32_t *n_expanded, ivr_stream stream) {
    IVR_REQUIRE(g && q && entries && D && I, "ivr_graph_search: NULL argument");
    IVR_REQUIRE(nq >= 1 && nq <= kGraphMaxBlocks, "ivr_graph_search: nq=%d outside [1,%lld]", nq, (long long)kGraphMaxBlocks);
    IVR_REQUIRE(ef >= 1 && ef <= kGraphMaxEf, "ivr_graph_search: ef=%d outside [1,%d]", ef, kGraphMaxEf);
    IVR_REQUIRE(k >= 1 && k <= ef, "ivr_graph_search: k=%d outside [1,ef=%d]", k, ef);
    IVR_REQUIRE(ne >= 1 && ne <= kGraphMaxDegree, "ivr_graph_search: ne=%d outside [1,%d]", ne, kGraphMaxDegree);
    std::lock_guard<std::mutex> lk(g->mu);
    if (g->ntotal > 0 && g->nbr_rows != g->ntotal) return ivr_fail(IVR_ERR_STATE, "ivr_graph_search: rows are stored but no neighbour table is set");
    IVR_HIP(hipSetDevice(g->ctx->device));
    hipStream_t s = (hipStream_t)stream;
    if (normalize_q) {
        int rc = ivr_reserve({{&g->qn, (size_t)nq * g->d * sizeof(float)}});
        if (rc != IVR_OK) return rc;
        IVR_HIP(hipMemcpyAsync(g->qn, q, (size_t)nq * g->d * sizeof(float), hipMemcpyDeviceToDevice, s));
        rc = ivr_l2_normalize(g->ctx, g->qn, nq, g->d, nullptr, stream);
        if (rc != IVR_OK) return rc;
        q = g->qn;
    }
    const int max_exp = (int)std::max<int64_t>(1, std::min<int64_t>(max_expansions, g->ntotal));
    GraphSearch a{g->rows, g->dp, g->d, g->ntotal, g->nbr, g->degree, q, k, ef, entries, ne, max_exp, D, I, n_expanded};
    IvrProf prof("graph_search", s, 0.0);
    hipLaunchKernelGGL(graph_search_kernel, dim3((unsigned)nq), dim3(256), (size_t)g->dp * sizeof(float), s, a);
    IVR_LAUNCH_CHECK();
    return IVR_OK;
}

}  // extern "C"
