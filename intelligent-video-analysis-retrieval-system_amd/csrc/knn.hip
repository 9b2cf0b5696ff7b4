// The neighbour graph of the flat index (ivr_index_knn_graph): for every stored row its k best OTHER rows of the same segment,
// optionally above a score.  The reference's MetadataManager._build_similarity_relationships (core.py:3493-3531: per folder the full
// cosine matrix, a sort of every row, the top 10 others with cosine > 0.7) for all folders in one call and without a matrix.  DESIGN.md
// section 4, "neighbour graph".
//
// Score S[j, i] = <stored row j as the query, stored row i> with the bits ivr_index_search and ivr_index_rescore report for that
// pair.  The segment bounds, the query block in LDS and the scoring of a stored tile are the self-join frame's (self_join.h), shared
// with cluster.hip; here are the walk of the full square in parts, the lists in LDS and the merge.  Unlike cluster.hip's triangle every
// ORDERED pair is scored with its own j as the query, so nothing rests on S[j, i] and S[i, j] having the same bits.
//   candidates of j   the rows i != j with seg_lo[j] <= i < seg_hi[j] (so i < ntotal), S[j, i] not NaN, and S[j, i] > threshold when
//                     one is given (-inf: none)
//   order             ivr_key(S[j, i], i): score descending, equal scores the lower row.  The keys of one row are unique
//
// Launches, all on the caller's stream and without a host round trip:
//   sj_bounds   per row: seg_lo, seg_hi (the run of seg_off that holds it, clipped to [0, n); empty for a row outside every segment)
//   kn_score    per chunk of query blocks: the tiled self-join; workgroup (b, y) keeps the best k keys of part y of block b's walk per
//               query column in LDS and writes them to the scratch
//   kn_merge    per chunk: the best k of a row's parts -> D, I, count
// A query block is 16 qt rows (qt tiles, as many as the LDS holds beside the lists); its walk runs from the tile of the lowest segment
// start among its rows to the tile of the highest segment end, and is cut into at most kKnMaxParts equal parts of at least kSjSplit
// tiles.  Scratch: query blocks of a chunk x kKnMaxParts x 64 x k keys, at most kKnScratchKeys; a larger index takes several chunks.
#include <climits>

#include "ivr_common.h"
#include "self_join.h"

namespace {

constexpr int kKnMaxParts = 16;                 // grid.y: parts of one query block's walk, each with its own partial lists
constexpr int64_t kKnScratchKeys = 1ll << 25;   // keys of the partial lists of one chunk of query blocks: 256 MiB

struct KnArgs {
    SjArgs j;                    // query blocks of kn_qt() tiles
    int k;
    int parts;                   // grid.y of the score launch
    float thr;
    int has_thr;
    uint64_t *keys;              // [query blocks of a chunk][parts][64][k]
};

// The walk of the query block of `nrows` <= 64 rows from row0 on: tiles [t0, t0 + tiles) hold every candidate of its rows; it is cut
// into nparts <= parts pieces of len tiles (nparts = 0: no row of the block lies in a segment).  Called by whole waves; every wave of
// the score and of the merge launch computes the same values from the same words.
struct KnWalk {
    int t0, t1, len, nparts;
};
__device__ __forceinline__ KnWalk kn_walk(const KnArgs &a, int row0, int nrows) {
    const int lane = threadIdx.x & 63, j = row0 + lane;
    int lo = INT_MAX, hi = 0;
    if (lane < nrows && j < a.j.n) {
        const int l = a.j.seg_lo[j], h = a.j.seg_hi[j];
        if (l < h) lo = l, hi = h;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        lo = min(lo, __shfl_xor(lo, o, 64));
        hi = max(hi, __shfl_xor(hi, o, 64));
    }
    KnWalk w{0, 0, 0, 0};
    if (lo < hi) {
        w.t0 = lo >> 4;
        w.t1 = (hi + 15) >> 4;                       // hi <= n: inside the tiles that hold stored rows
        const int tiles = w.t1 - w.t0;
        w.len = max(kSjSplit, (tiles + a.parts - 1) / a.parts);
        w.nparts = (tiles + w.len - 1) / w.len;
    }
    return w;
}

// Workgroup (b, y) holds the tiles of query block blk0 + b in LDS as they lie in the storage and streams part y of the block's walk,
// one stored tile per wave and round.  The trip count of the rounds is the same for every wave (a wave past its last tile idles
// through them), because a round ends in workgroup barriers.  Per query column the LDS holds a list of k keys, descending, 0 = unused:
// list[slot][column].  Its last slot is the column's threshold: a lane tests its 16 scores of a tile against the thresholds of its four
// columns and only a key above one survives.  The waves with survivors in a round then take turns, a barrier after each: within a turn
// the lane (q, c) owns column 16 q + c, collects the survivors of that column from the four quad rows of its wave by shuffles and
// inserts them.  So a list is written by one lane at a time, a stale threshold is only ever too low, and since the candidates of a
// column have unique keys its final list is the best k of the part whatever the order of the insertions.
__global__ __launch_bounds__(64 * kSjWaves) void kn_score_kernel(KnArgs a, int blk0) {
    extern __shared__ __attribute__((aligned(16))) float4 qs[];
    const int k = a.k, ncol = a.j.qt * 16;
    const int ntiles = (a.j.n + 15) >> 4;
    const int tb0 = (blk0 + (int)blockIdx.x) * a.j.qt, nq = min(a.j.qt, ntiles - tb0);
    const KnWalk w = kn_walk(a, tb0 * 16, nq * 16);
    if ((int)blockIdx.y >= w.nparts) return;         // the whole workgroup: nothing staged, no barrier reached, nothing written
    const int pa0 = w.t0 + (int)blockIdx.y * w.len, pa1 = min(w.t1, pa0 + w.len);
    uint64_t *list = reinterpret_cast<uint64_t *>(qs + a.j.qt * a.j.dp4 * 16);    // [k][ncol]
    unsigned *flag = reinterpret_cast<unsigned *>(list + k * ncol);               // [3]: the waves with survivors in round r, at r % 3
    sj_stage(a.j, tb0, nq, qs);
    for (int i = threadIdx.x; i < k * ncol; i += blockDim.x) list[i] = 0;
    if (threadIdx.x < 3) flag[threadIdx.x] = 0;
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, h = lane >> 4, c = lane & 15;
    // this lane's column of each query tile: row col.jq, candidate rows [col.lo, col.hi) except col.jq
    const SjCols col = sj_columns(a.j, tb0, nq);
    int round = 0;
    for (int t0 = pa0; t0 < pa1; t0 += kSjWaves, ++round) {
        const int ta = t0 + wave;
        uint64_t key[4][4];
        bool mine = false;
        if (ta < pa1) {                              // wave-uniform
            f32x4 acc[4];
            sj_score_tile(a.j, qs, nq, ta, acc);
            const int i0 = ta * 16 + h * 4;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const uint64_t low = q < nq ? list[(k - 1) * ncol + q * 16 + c] : ~0ull;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int i = i0 + r;
                    const float s = acc[q][r];
                    const bool ok = i >= col.lo[q] && i < col.hi[q] && i != col.jq[q] && s == s && (!a.has_thr || s > a.thr);
                    const uint64_t x = ivr_key(s, (uint32_t)i);
                    key[q][r] = ok && x > low ? x : 0;
                    mine = mine || key[q][r] != 0;
                }
            }
        } else {
#pragma unroll
            for (int q = 0; q < 4; ++q)
#pragma unroll
                for (int r = 0; r < 4; ++r) key[q][r] = 0;
        }
        const bool any = __any(mine);
        if (any && lane == 0) atomicOr(flag + round % 3, 1u << wave);
        __syncthreads();
        const unsigned turns = flag[round % 3];
        if (threadIdx.x == 0) flag[(round + 2) % 3] = 0;         // read last in the round before, set next in the round after the next
        for (int v = 0; v < kSjWaves; ++v) {
            if (!((turns >> v) & 1u)) continue;                  // the same word in every thread: the barrier below is uniform
            if (v == wave) {
#pragma unroll
                for (int s = 0; s < 4; ++s) {
                    // this lane gives what it holds for the column of query tile (h - s) & 3 and takes, as the owner of column 16 h + c, what
                    // the lane of quad row (h + s) & 3 holds for query tile h
                    const int qsrc = (h - s) & 3, from = ((h + s) & 3) * 16 + c;
                    uint64_t give[4], take[4];
                    bool some = false;
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        give[r] = key[0][r];
#pragma unroll
                        for (int q = 1; q < 4; ++q) give[r] = qsrc == q ? key[q][r] : give[r];
                        some = some || give[r] != 0;
                    }
                    if (!__any(some)) continue;          // most steps of a late round: nothing to hand over
#pragma unroll
                    for (int r = 0; r < 4; ++r) {        // the eight shuffles of a step are independent: one latency, not eight
                        const uint32_t xh = __shfl((uint32_t)(give[r] >> 32), from, 64), xl = __shfl((uint32_t)give[r], from, 64);
                        take[r] = ((uint64_t)xh << 32) | xl;
                    }
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const uint64_t x = take[r];
                        if (x != 0 && x > list[(k - 1) * ncol + lane]) {       // x != 0: query tile h exists, so lane < ncol
                            int p = k - 1;
                            while (p > 0) {
                                const uint64_t y = list[(p - 1) * ncol + lane];
                                if (y > x) break;
                                list[p * ncol + lane] = y;
                                --p;
                            }
                            list[p * ncol + lane] = x;
                        }
                    }
                }
            }
            __syncthreads();
        }
    }
    // the lists of the block's columns, column-major, behind those of the parts before
    uint64_t *out = a.keys + ((int64_t)blockIdx.x * a.parts + blockIdx.y) * 64 * k;
    for (int i = threadIdx.x; i < nq * 16 * k; i += blockDim.x) out[i] = list[(i % k) * ncol + i / k];
}

// the keys of the descending list l[0 .. k) (0 = unused, at its end) that are above x
__device__ __forceinline__ int kn_above(const uint64_t *l, int k, uint64_t x) {
    int lo = 0, hi = k;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (l[mid] > x) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// One workgroup per query block of the chunk, one wave per row at a time: the partial lists of the row's parts are descending and
// their keys unique, so the rank of a key is its slot in its own list plus the keys above it in every other list.
__global__ __launch_bounds__(256) void kn_merge_kernel(KnArgs a, int blk0, float *__restrict__ D, int64_t *__restrict__ I,
                                                       int32_t *__restrict__ count) {
    extern __shared__ __attribute__((aligned(16))) uint64_t ml[];                 // [4 waves][parts][k]
    const int k = a.k, row0 = (blk0 + (int)blockIdx.x) * a.j.qt * 16, nrows = min(a.j.qt * 16, a.j.n - row0);
    const KnWalk w = kn_walk(a, row0, nrows);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint64_t *l = ml + wave * a.parts * k;
    for (int c0 = 0; c0 < nrows; c0 += 4) {          // the same trip count in every wave
        const int c = c0 + wave;
        const bool live = c < nrows;
        const uint64_t *src = a.keys + ((int64_t)blockIdx.x * a.parts * 64 + c) * k;
        if (live && lane < k)
            for (int p = 0; p < w.nparts; ++p) l[p * k + lane] = src[(int64_t)p * 64 * k + lane];
        __syncthreads();
        if (live) {
            const int64_t j = row0 + c;
            int total = 0;
            for (int p = 0; p < w.nparts; ++p) {
                const uint64_t x = lane < k ? l[p * k + lane] : 0;
                total += __popcll(__ballot(x != 0));
                if (x == 0) continue;
                int rank = lane;
                for (int o = 0; o < w.nparts; ++o)
                    if (o != p) rank += kn_above(l + o * k, k, x);
                if (rank < k) {
                    D[j * k + rank] = ivr_ord2f((uint32_t)(x >> 32));
                    I[j * k + rank] = (int64_t)(0xFFFFFFFFu - (uint32_t)x);
                }
            }
            const int cnt = min(total, k);
            if (lane < k && lane >= cnt) {
                D[j * k + lane] = -FLT_MAX;
                I[j * k + lane] = -1;
            }
            if (lane == 0) count[j] = cnt;
        }
        __syncthreads();
    }
}

// query tiles of a block: as many (at most 4) as leave room for their lists in 160 KiB of LDS
size_t kn_lds(int qt, int dp, int k) { return (size_t)qt * 16 * ((size_t)dp * 4 + (size_t)k * 8) + 16; }
int kn_qt(int dp, int k) {
    int qt = 4;
    while (qt > 1 && kn_lds(qt, dp, k) > 160 * 1024) --qt;
    return qt;
}

}  // namespace

extern "C" {

int ivr_knn_max_k(void) { return IVR_KNN_MAX_K; }

int ivr_knn_piece_rows(void) { return kSjSplit * 16; }

int ivr_index_knn_graph(ivr_index *x, int k, const int64_t *seg_off, int nseg, float threshold, float *D, int64_t *I, int32_t *count,
                        ivr_stream stream) {
    IVR_REQUIRE(x && D && I && count, "ivr_index_knn_graph: NULL argument");
    IVR_REQUIRE(k >= 1 && k <= IVR_KNN_MAX_K, "ivr_index_knn_graph: k=%d outside [1,%d]", k, IVR_KNN_MAX_K);
    IVR_REQUIRE(threshold == threshold, "ivr_index_knn_graph: threshold=%g is NaN", (double)threshold);
    IVR_REQUIRE(!seg_off || nseg >= 1, "ivr_index_knn_graph: nseg=%d with seg_off", nseg);
    hipStream_t s = (hipStream_t)stream;
    std::lock_guard<std::mutex> lk(x->mu);
    IVR_REQUIRE(x->ntotal < (1ll << 31), "ivr_index_knn_graph: ntotal=%lld >= 2^31", (long long)x->ntotal);
    if (x->ntotal == 0) return IVR_OK;
    IVR_HIP(hipSetDevice(x->ctx->device));
    const int n = (int)x->ntotal, ntiles = (int)ivr_ceil_div(n, 16);
    const int qt = kn_qt(x->dp, k);
    const int nblocks = (int)ivr_ceil_div(ntiles, qt);
    const int parts = (int)std::min<int64_t>(kKnMaxParts, ivr_ceil_div(ntiles, kSjSplit));
    const int chunk = (int)std::max<int64_t>(1, std::min<int64_t>(nblocks, kKnScratchKeys / ((int64_t)parts * 64 * k)));
    int rc = ivr_reserve({{&x->kn_keys, (size_t)chunk * parts * 64 * k * 8}});
    if (rc != IVR_OK) return rc;
    const size_t lds = kn_lds(qt, x->dp, k), mlds = (size_t)4 * parts * k * 8;
    rc = ivr_func_max_lds(reinterpret_cast<const void *>(kn_score_kernel), (int)lds);
    if (rc != IVR_OK) return rc;
    SjArgs j;
    rc = sj_prepare(x, qt, seg_off, nseg, s, j);
    if (rc != IVR_OK) return rc;
    const KnArgs a{j, k, parts, threshold, threshold != -INFINITY, x->kn_keys};
    for (int b0 = 0; b0 < nblocks; b0 += chunk) {
        const unsigned nb = (unsigned)std::min(chunk, nblocks - b0);
        {
            IvrProf prof("knn_score", s, (double)nb * qt * 16 * n * x->dp);
            hipLaunchKernelGGL(kn_score_kernel, dim3(nb, (unsigned)parts), dim3(64 * kSjWaves), lds, s, a, b0);
            IVR_LAUNCH_CHECK();
        }
        hipLaunchKernelGGL(kn_merge_kernel, dim3(nb), dim3(256), mlds, s, a, b0, D, I, count);
        IVR_LAUNCH_CHECK();
    }
    return IVR_OK;
}

}  // extern "C"
