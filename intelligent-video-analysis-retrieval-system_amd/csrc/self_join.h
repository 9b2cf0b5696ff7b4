// The frame of the tiled self-joins over the flat index: frame clustering (cluster.hip) and the neighbour graph (knn.hip).  Not part of
// the C ABI.  tags.hip uses the staging and the scoring of a tile with a second matrix (the label tiles) as the streamed side.
//
// Score S[j, i] = <stored row j as the query, stored row i>, accumulated by stream_tile / mfma_chunk4 (search_internal.h), so it has
// the bits ivr_index_search and ivr_index_rescore report for that pair.  The float32 storage tiles have the layout of the tiled query
// buffer, so a stored 16-row tile is the query operand as it lies: a workgroup copies a query block of up to four tiles into LDS and
// streams stored tiles past it, one per wave at a time.  What is here: the per-row segment bounds, the staging of the block, the
// per-lane columns and the scoring of one stored tile.  Which tiles a workgroup walks and what it does with the 16 scores a lane
// holds per tile is the caller's.
#pragma once
#include <climits>

#include "search_internal.h"

// Measured on 20,000 / 100,000 x 512 rows as one segment (whole call).  DBSCAN: 4 waves and unsplit walks 18.0 / 277 ms, 4 waves and
// pieces of 128 tiles 12.6 / 281 ms, 8 waves and pieces of 64 / 128 / 256 tiles 9.5 / 9.7 / 10.8 ms and 219 / 217 / 216 ms.  Neighbour
// graph (k = 10, threshold 0.7 / none; third figure: 1M rows in 2,000 folders): 8 waves, parts of >= 128 tiles, <= 16 parts 6.56 / 12.6,
// 151 / 216 and 15.8 / 26.2 ms; 4 waves 8.59 / 14.5, 199 / 263 and 19.3 / 29.5 ms; parts of >= 512 tiles 6.92 / 9.53, 150 / 204 and
// 15.9 / 26.4 ms; <= 32 parts 6.58 / 12.7, 152 / 261 and 17.0 / 27.8 ms
constexpr int kSjWaves = 8;          // waves of a score workgroup: two per SIMD, so that one's tile loads overlap the other's MFMAs
constexpr int kSjSplit = 128;        // stored 16-row tiles of one piece of a walk: a query block's walk is cut into pieces of (at least) this

struct SjArgs {
    const float4 *data;              // the float32 tiles of the storage
    int dp4;
    int qt;                          // 16-row tiles of a query block, at most 4
    int n;                           // stored rows
    const int *seg_lo, *seg_hi;      // [n]: row j's segment is [seg_lo[j], seg_hi[j])
};

// self_join.hip.  The arguments of a self-join over the stored rows of x (0 < ntotal < 2^31; the caller holds x->mu) with query
// blocks of qt tiles, and one launch on s that fills the segment bounds (x->sj_seg): the run of seg_off [nseg + 1] that holds row j,
// clipped to [0, n); [0, n) without seg_off; the empty range lo = hi = j + 1 for a row outside every run.  So seg_lo ascends with the
// row, seg_lo[j] <= j exactly for the rows inside a segment, and an empty range holds no row and is inside no other row's range.
int sj_prepare(ivr_index *x, int qt, const int64_t *seg_off, int nseg, hipStream_t s, SjArgs &a);

// The tiles tb0 .. tb0 + nq - 1 into LDS as they lie in the storage; the caller's barrier ends the copy
__device__ __forceinline__ void sj_stage(const SjArgs &a, int tb0, int nq, float4 *qs) {
    const float4 *src = a.data + (int64_t)tb0 * a.dp4 * 16;
    for (int i = threadIdx.x; i < nq * a.dp4 * 16; i += blockDim.x) qs[i] = src[i];
}

// This lane's column of each query tile of the block: row jq[q] with its segment [lo[q], hi[q]); an empty range (no row i has
// i >= lo) for a column that is no stored row
struct SjCols {
    int jq[4], lo[4], hi[4];
};
__device__ __forceinline__ SjCols sj_columns(const SjArgs &a, int tb0, int nq) {
    SjCols c;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        c.jq[q] = (tb0 + q) * 16 + (threadIdx.x & 15);
        const bool valid = q < nq && c.jq[q] < a.n;
        c.lo[q] = valid ? a.seg_lo[c.jq[q]] : INT_MAX;
        c.hi[q] = valid ? a.seg_hi[c.jq[q]] : 0;
    }
    return c;
}

// Stored tile ta against the staged block: acc[q][r] = S[j, i] for j = the lane's column of query tile q < nq and i = 16 ta +
// 4 (lane >> 4) + r.  The tile lies inside the storage's allocation, whose capacity is a multiple of 64 rows >= ntotal.
__device__ __forceinline__ void sj_score_tile(const SjArgs &a, const float4 *qs, int nq, int ta, f32x4 (&acc)[4]) {
    const int per_tile = a.dp4 * 16, lane = threadIdx.x & 63;
#pragma unroll
    for (int q = 0; q < 4; ++q) acc[q] = f32x4{0.f, 0.f, 0.f, 0.f};
    stream_tile<4>(a.data + (int64_t)ta * per_tile + lane, a.dp4 >> 2, [&](int q, int kc, const float4 &av) {
        if (q < nq) mfma_chunk4(acc[q], av, qs[q * per_tile + kc * 64 + lane]);
    });
}
