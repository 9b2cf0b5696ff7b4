// Internal interface between search.hip (index object, selection, re-score) and search_scanq.hip (the large-query-batch
// candidate scan).  Not part of the C ABI.
#pragma once
#include "ivr_common.h"

#include <cfloat>

// One launch of the large-query candidate scan: every stored row against every query of the batch on the bf16 MFMA,
// reduced on the fly to one maximum per (query, 16-row tile) and one per (query, 128-row block).  The index is streamed
// from HBM once per launch whatever the number of queries ("large query batches").
//   data16 : bf16 scan copy of the rows, [row tile of 16][pieces][64 lanes x 16 B]; allocation padded to 256 rows
//   q16    : the queries in the same layout (bf16, rounded to nearest), padded with zero rows to a multiple of 256 queries
//   pieces : 1 KiB pieces per 16-row tile (even)
//   tmax   : [padded queries][tstride] maximum of each 16-row tile; bmax: [padded queries][bstride] maximum of each 128-row block
struct ScanQArgs {
    const uint4 *data16;
    const uint4 *q16;
    int pieces;
    int qblocks;          // padded queries / 256
    int64_t ntotal;       // stored rows; rows >= ntotal are masked out of the maxima
    int64_t nblocks;      // ceil(ntotal / 256)
    float *tmax;
    int64_t tstride;
    float *bmax;
    int64_t bstride;
};

// Filtered search (ivr_index_search_filtered): the rows a launch may rank, in the row numbering of the part of the index it scans.
// Row r is allowed iff lo <= r < hi and, when bits != NULL, bit (bit0 + r) of bits is set (LSB first within a byte).  The host clips
// [lo, hi) to the scanned rows and to the bitmap's length, so a bitmap byte is only read for an allowed-range row.
struct RowMask {
    int64_t lo = 0, hi = 0;
    const uint8_t *bits = nullptr;
    int64_t bit0 = 0;
};

// The mask of 64 consecutive rows r0 .. r0 + 63 as one wave-uniform word, in two steps so that the bitmap load can be issued early:
// row_mask_fetch (lane l: the bitmap byte of row r0 + l; one load per lane, no use of it), later row_mask_word (bit l = row r0 + l
// allowed, by ballot).  Without a bitmap nothing is loaded.
__device__ __forceinline__ uint32_t row_mask_fetch(const RowMask &m, int64_t r0) {
    if (!m.bits) return 0u;
    const int64_t r = r0 + (threadIdx.x & 63);
    const int64_t b = m.bit0 + (r >= m.lo && r < m.hi ? r : m.lo);     // an in-range byte for every lane: no branch around the load
    return m.bits[b >> 3];
}
__device__ __forceinline__ uint64_t row_mask_word(const RowMask &m, int64_t r0, uint32_t byte) {
    const int64_t r = r0 + (threadIdx.x & 63);
    bool ok = r >= m.lo && r < m.hi;
    if (m.bits) ok = ok && ((byte >> ((m.bit0 + r) & 7)) & 1u);
    return __ballot(ok);
}
// score of a row in a masked maximum: -inf for a row that is not allowed (a maximum of -inf = no allowed row), allowed rows clamped to
// >= -FLT_MAX so that they stay above that sentinel
__device__ __forceinline__ float row_mask_score(uint64_t word_shifted, int bit, float s) {
    return ((word_shifted >> bit) & 1ull) ? fmaxf(s, -FLT_MAX) : -INFINITY;
}

int ivr_launch_scanq(ivr_ctx *ctx, const ScanQArgs &a, hipStream_t s, const RowMask *mask = nullptr);
