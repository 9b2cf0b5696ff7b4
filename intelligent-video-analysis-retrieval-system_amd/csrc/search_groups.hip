// Grouped search over the flat index (ivr_index_search_groups, ivr_index_best_per_segment): per query the best G segments (videos) of
// seg_off, each with its g best rows.  The missing member of the seg_off family: the clip search, the event search, the clustering and
// the neighbour graph all answer "per video", the plain query did not.  DESIGN.md section 4, "grouped search".
//
// Frame score S[q, r] = <query q, stored row r>, accumulated by stream_tile / mfma_chunk4 (first pass) and by pair_score (rows pass):
// the accumulation order of every float32 score of the index (search_internal.h), so it has the bits ivr_index_search reports for that
// pair.  Row key K[q, r] = ivr_key(S[q, r], r): the larger key ranks first, equal scores the lower row, -0.0 equal to +0.0.  The key of
// segment j is the greatest K[q, r] over its rows; groups are ranked by it, and since the key holds the row, equal best scores rank the
// segment with the lower best row = the lower segment first.
//
// Launches, all on the caller's stream and without a host round trip:
//   grp_rowseg    once per call: the segment number of every stored row (-1 in front of seg_off[0], nseg behind seg_off[nseg] and for
//                 the padding rows of the last tile), so the table ascends with the row and a 16-row tile lies inside one segment
//                 exactly when its first and last entry agree
//   per chunk of queries (whole 16-query tiles):
//   fill          segbest [queries of the chunk][nseg] = 0: key 0 is "no row"
//   grp_segbest   THE HOT PATH.  The shape of the clip search's score pass: a workgroup takes 64 stored 16-row tiles against one
//                 16-query tile staged in LDS, one tile per wave at a time.  No score is written.  A lane's accumulator holds four
//                 consecutive rows of one query column: it folds them into one running key per lane while the wave's tiles stay inside
//                 one segment; when the segment changes (and at the end of the walk) the four lanes of a column are folded with two
//                 cross-lane moves and ONE lane per column issues a 64-bit atomicMax into segbest[q][segment].  A tile that straddles
//                 segments is folded once per segment it touches.  So a tile inside one segment costs at most one atomic per query
//                 column, and a workgroup whose 1,024 rows lie inside one segment costs one per column and wave: 4, where one per row
//                 would be 1,024
//   grp_select    select_topk_kernel (search_select.h) over segbest[q][0 .. nseg): the best G keys per query -> the best row of every
//                 chosen group.  ivr_index_best_per_segment decodes segbest instead (grp_decode)
//   grp_label     per result slot: the segment of the best row (ivr_last_le), and with g = 1 the label of the row: the call ends here
//   grp_rows      g > 1: workgroup (slot, y) walks piece y of the slot's segment with pair_score against the query's column of the
//                 tiled query buffer, rows outside [lo, hi) masked by number.  Each wave keeps a list of g <= 64 keys, descending, one
//                 key per lane in registers; a key above the list's last is inserted with one ballot and one lane shift
//   grp_merge     one wave per slot: the lists of the slot's pieces and waves -> D / I, labelled through the id table where there is one
//
// Why the result is the same on every run: segbest only ever receives maxima of 64-bit keys that are unique per (query, row).  A
// maximum does not depend on the order in which its operands arrive, so whatever the schedule of the workgroups segbest ends as the
// greatest key of each (query, segment).  Everything behind it selects among unique keys.
//
// Piece size (ivr_group_piece_rows): 128 tiles = 2,048 rows, the piece of the neighbour graph's walk.  A video of a few hundred
// keyframes is one piece, read by four waves of one workgroup (32 tiles each at most); a long segment spreads over up to kGrMaxParts
// workgroups per slot, whose lists the merge folds.  Shorter pieces multiply the lists of the merge, longer ones leave a slot of a
// long video on one CU.
//
// Scratch on the index, grow-only: 8 bytes per (query of a chunk, segment), 4 bytes per stored row (rounded up to 16), 12 bytes per
// result slot (query of a chunk, group), and for g > 1 another 8 g bytes per (result slot, piece, wave).  A chunk holds as many queries
// as keep segbest and the lists within IVR_SEQ_CHUNK_SLOTS slots each, in whole 16-query tiles, 16 at least and 4,096 at most (which
// keeps the grid of the first pass, row blocks x query tiles, below 2^31).
#include "ivr_common.h"
#include "search_internal.h"
#include "search_select.h"

namespace {

constexpr int kGrTilesPerBlock = 64;     // 16-row tiles per workgroup of the first pass, as the clip search's score pass
constexpr int kGrMaxChunk = 1 << 12;     // queries per chunk at most
constexpr int kGrPieceTiles = 128;       // 16-row tiles of one piece of a segment in the rows pass
constexpr int kGrMaxParts = 16;          // grid.y of the rows pass: pieces of one segment at most (longer pieces beyond that)
constexpr int kGrWaves = 4;              // waves of a rows workgroup, each with a list of its own

// Thread i: row i of the padded row range [0, 16 ntiles)
__global__ __launch_bounds__(256) void grp_rowseg_kernel(int n, int64_t nrows, const int64_t *__restrict__ seg_off, int nseg, int *__restrict__ rowseg) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= nrows) return;
    int s = nseg;
    if (i < n) {
        if (!seg_off) s = 0;
        else if (seg_off[0] > i) s = -1;
        else s = ivr_last_le(seg_off, nseg + 1, i);          // nseg: behind the last offset
    }
    rowseg[i] = s;
}

}  // namespace

// search_internal.h: the table as the grouped search and the moment search (search_moments.hip) launch it
int ivr_launch_rowseg(ivr_index *x, const int64_t *seg_off, int nseg, hipStream_t s) {
    const int64_t nrows = ivr_ceil_div(x->ntotal, 16) * 16;
    const int rc = ivr_reserve({{&x->gr_seg, (size_t)nrows * 4}});
    if (rc != IVR_OK) return rc;
    hipLaunchKernelGGL(grp_rowseg_kernel, dim3((unsigned)ivr_ceil_div(nrows, 256)), dim3(256), 0, s, (int)x->ntotal, nrows, seg_off, seg_off ? nseg : 1,
                       x->gr_seg);
    IVR_LAUNCH_CHECK();
    return IVR_OK;
}

namespace {

struct GrBest {
    const float4 *data;          // the float32 tiles of the storage
    const float4 *qtile;         // the first 16-query tile of the chunk in the tiled query buffer
    int dp4;
    int qtiles;                  // 16-query tiles of the chunk
    int64_t ntiles;              // 16-row tiles that hold stored rows
    const int *rowseg;           // [16 ntiles], ascending
    int nseg;
    int ncols;                   // queries of the chunk
    uint64_t *segbest;           // [ncols][nseg]
};

// the maximum over the four lanes (quad rows) that hold one query column
__device__ __forceinline__ uint64_t grp_fold_column(uint64_t v) {
    uint64_t t = __shfl_xor(v, 16, 64);
    v = t > v ? t : v;
    t = __shfl_xor(v, 32, 64);
    return t > v ? t : v;
}

// Workgroup b: query tile y = b % qtiles of the chunk against the row tiles 64 x .. 64 x + 63, x = b / qtiles, as seq_score_kernel
// walks them.  Every tile read lies inside the storage's allocation (capacity a multiple of 64 rows >= ntotal), every rowseg read below
// 16 ntiles, and an atomic goes to segbest[col][sg] with col < ncols and 0 <= sg < nseg only.  The segment variables (cur_sg, first,
// last, sg) are the same in every lane of a wave, so every shuffle below is reached by whole waves.
__global__ __launch_bounds__(256) void grp_segbest_kernel(GrBest a) {
    extern __shared__ __attribute__((aligned(16))) float4 qs[];
    const int per_tile = a.dp4 * 16, kchunks = a.dp4 >> 2;
    const int y = (int)(blockIdx.x % a.qtiles);
    const int64_t x = blockIdx.x / a.qtiles;
    const float4 *qt = a.qtile + (int64_t)y * per_tile;
    for (int i = threadIdx.x; i < per_tile; i += blockDim.x) qs[i] = qt[i];
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, h = lane >> 4;
    const int col = y * 16 + (lane & 15);
    const bool writer = lane < 16 && col < a.ncols;
    uint64_t *best = a.segbest + (int64_t)(col < a.ncols ? col : 0) * a.nseg;
    const int64_t t0 = x * kGrTilesPerBlock, t1 = min(t0 + kGrTilesPerBlock, a.ntiles);
    int cur_sg = -1;             // the segment the running key belongs to; outside [0, nseg): none
    uint64_t cur = 0;            // this lane's running maximum for cur_sg
    auto flush = [&](int sg, uint64_t v) {
        if (sg < 0 || sg >= a.nseg) return;
        v = grp_fold_column(v);
        if (writer && v) atomicMax(reinterpret_cast<unsigned long long *>(best + sg), (unsigned long long)v);
    };
    for (int64_t t = t0 + wave; t < t1; t += 4) {
        const float4 *at = a.data + t * per_tile + lane;
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        stream_tile<1>(at, kchunks, [&](int, int kc, const float4 &av) { mfma_chunk4(acc, av, qs[kc * 64 + lane]); });
        // acc[r] = <row 16 t + 4 h + r, query column (lane & 15) of the tile>
        const int4 sg4 = *reinterpret_cast<const int4 *>(a.rowseg + t * 16 + h * 4);
        const int sgr[4] = {sg4.x, sg4.y, sg4.z, sg4.w};
        const uint32_t row0 = (uint32_t)(t * 16 + h * 4);
        uint64_t key[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) key[r] = ivr_key(acc[r], row0 + r);
        const int first = __builtin_amdgcn_readlane(sg4.x, 0), last = __builtin_amdgcn_readlane(sg4.w, 48);
        if (first != cur_sg) {
            flush(cur_sg, cur);
            cur = 0;
        }
        // the segments of the tile in front of its last one, each folded on its own; the running key belongs to the first of them
        for (int sg = first; sg != last;) {
            uint64_t v = cur;
            cur = 0;
            int nx = last;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                if (sgr[r] == sg) v = key[r] > v ? key[r] : v;
                if (sgr[r] > sg) nx = min(nx, sgr[r]);
            }
            flush(sg, v);
            nx = min(nx, __shfl_xor(nx, 16, 64));
            nx = min(nx, __shfl_xor(nx, 32, 64));
            sg = __builtin_amdgcn_readfirstlane(nx);         // ascending and <= last: the loop ends
        }
        // the tile's last segment (the only one of a tile inside one segment) runs on
        cur_sg = last;
        if (last >= 0 && last < a.nseg) {
#pragma unroll
            for (int r = 0; r < 4; ++r)
                if (sgr[r] == last) cur = key[r] > cur ? key[r] : cur;
        }
    }
    flush(cur_sg, cur);
}

struct SrcSegBest {    // the segment keys of query q of the chunk, every one written (0 = no row)
    const uint64_t *keys;
    int64_t n;
    __device__ uint64_t key(int q, int64_t i) const { return keys[(int64_t)q * n + i]; }
};

// ivr_index_best_per_segment.  Thread i: (query, segment) i of the chunk
__global__ __launch_bounds__(256) void grp_decode_kernel(const uint64_t *__restrict__ segbest, int64_t nslots, const int64_t *__restrict__ ids,
                                                         float *__restrict__ D, int64_t *__restrict__ I) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= nslots) return;
    const uint64_t key = segbest[i];
    const int64_t row = (int64_t)(0xFFFFFFFFu - (uint32_t)key);
    D[i] = key ? ivr_ord2f((uint32_t)(key >> 32)) : -FLT_MAX;
    I[i] = key ? (ids ? ids[row] : row) : -1;
}

// Thread i: result slot i of the chunk, whose best row the selection left in rows (-1: unused).  I != NULL (g = 1): the row's label
__global__ __launch_bounds__(256) void grp_label_kernel(const int64_t *__restrict__ rows, int64_t nslots, const int64_t *__restrict__ seg_off, int nseg,
                                                        const int64_t *__restrict__ ids, int64_t *__restrict__ Gseg, int64_t *__restrict__ I) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= nslots) return;
    const int64_t row = rows[i];
    Gseg[i] = row < 0 ? -1 : (seg_off ? ivr_last_le(seg_off, nseg + 1, row) : 0);
    if (I) I[i] = row < 0 ? -1 : (ids ? ids[row] : row);
}

struct GrRows {
    const float4 *data;
    const float4 *qtiled;        // the tiled query buffer of the whole call
    int dp4;
    int n;                       // stored rows
    const int64_t *seg_off;
    int nseg;
    int q0;                      // first query of the chunk
    int G, g;
    int parts;                   // grid.y of the rows pass
    const int64_t *rows;         // [slots of the chunk]: the best row of the slot's group, -1 for an unused slot
    uint64_t *lists;             // [slots of the chunk][parts][kGrWaves][g]
    const int64_t *ids;
};

// The walk of a slot whose group holds `row`: the tiles [t0, t1) that overlap the rows [lo, hi) of its segment, cut into nparts <=
// parts pieces of len tiles.  The rows pass and the merge compute the same values from the same words.
struct GrWalk {
    int lo, hi, t0, t1, len, nparts;
};
__device__ __forceinline__ GrWalk grp_walk(const GrRows &a, int64_t row) {
    GrWalk w{0, a.n, 0, 0, 0, 0};
    if (a.seg_off) {
        // row is the best row of a segment: seg_off[sg] <= row and sg < nseg (the clamp keeps sg + 1 inside offsets that do not ascend)
        const int sg = min(ivr_last_le(a.seg_off, a.nseg + 1, row), a.nseg - 1);
        w.lo = (int)max(a.seg_off[sg], (int64_t)0);
        w.hi = (int)min(a.seg_off[sg + 1], (int64_t)a.n);
    }
    w.t0 = w.lo >> 4;
    w.t1 = (w.hi + 15) >> 4;                                              // hi <= n: inside the tiles that hold stored rows
    const int tiles = w.t1 - w.t0;
    w.len = max(kGrPieceTiles, (tiles + a.parts - 1) / a.parts);
    w.nparts = (tiles + w.len - 1) / w.len;
    return w;
}

// A wave's list of g keys, descending, 0 = unused: lane i < g holds entry i, the lanes from g on hold 0.  x is above the last entry
__device__ __forceinline__ void grp_insert(uint64_t &L, uint64_t x, int g, int lane) {
    const int pos = __popcll(__ballot(L > x));                            // < g, since entry g - 1 is below x
    const uint64_t up = __shfl_up(L, 1, 64);
    L = lane < pos ? L : (lane == pos ? x : up);
    if (lane >= g) L = 0;
}

// Workgroup (slot, y): piece y of the slot's walk, one tile per wave at a time; no barrier, the waves are independent.  A tile is
// scored against the whole 16-query tile of the slot's query (pair_score); the lanes of the query's column hold its 16 rows.  Every
// tile read lies inside the storage's allocation, every list store inside the slot's own stretch of the scratch.
__global__ __launch_bounds__(64 * kGrWaves) void grp_rows_kernel(GrRows a) {
    const int64_t slot = blockIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, h = lane >> 4;
    const int64_t row = a.rows[slot];
    if (row < 0) return;                                                  // unused slot: the merge reads none of its lists
    const GrWalk w = grp_walk(a, row);
    if ((int)blockIdx.y >= w.nparts) return;
    const int pa0 = w.t0 + (int)blockIdx.y * w.len, pa1 = min(w.t1, pa0 + w.len);
    const int q = a.q0 + (int)(slot / a.G), qc = q & 15;
    const int per_tile = a.dp4 * 16, kchunks = a.dp4 >> 2;
    const float4 *qb = a.qtiled + (int64_t)(q >> 4) * per_tile + lane;
    const bool mine = (lane & 15) == qc;
    uint64_t L = 0;
    for (int t = pa0 + wave; t < pa1; t += kGrWaves) {
        const f32x4 acc = pair_score<4>(a.data + (int64_t)t * per_tile + lane, qb, kchunks);
        // acc[r] = <row 16 t + 4 h + r, query (lane & 15) of the query tile>
        uint64_t key[4], top = 0;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int i = t * 16 + h * 4 + r;
            key[r] = mine && i >= w.lo && i < w.hi ? ivr_key(acc[r], (uint32_t)i) : 0;
            top = key[r] > top ? key[r] : top;
        }
        uint64_t low = __shfl(L, a.g - 1, 64);
        if (!__any(top > low)) continue;
#pragma unroll
        for (int hh = 0; hh < 4; ++hh)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const uint64_t xk = __shfl(key[r], hh * 16 + qc, 64);
                if (xk > low) {                                           // the same in every lane
                    grp_insert(L, xk, a.g, lane);
                    low = __shfl(L, a.g - 1, 64);
                }
            }
    }
    uint64_t *out = a.lists + ((slot * a.parts + blockIdx.y) * kGrWaves + wave) * a.g;
    if (lane < a.g) out[lane] = L;
}

// One wave per slot of the chunk: the keys of every list of the slot's pieces through the same insertion -> D, I [slot][g]; the keys
// of a slot are unique, so the result is the best g of the segment whatever the order
__global__ __launch_bounds__(256) void grp_merge_kernel(GrRows a, int64_t nslots, float *__restrict__ D, int64_t *__restrict__ I) {
    const int64_t slot = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (slot >= nslots) return;
    const int lane = threadIdx.x & 63;
    const int64_t row = a.rows[slot];
    uint64_t L = 0;
    if (row >= 0) {
        const GrWalk w = grp_walk(a, row);
        const uint64_t *src = a.lists + slot * a.parts * kGrWaves * a.g;
        uint64_t low = 0;
        for (int p = 0; p < w.nparts; ++p)
            for (int v = 0; v < kGrWaves; ++v) {
                const uint64_t xk = lane < a.g ? src[((int64_t)p * kGrWaves + v) * a.g + lane] : 0;
                uint64_t m = __ballot(xk > low);
                while (m) {
                    const uint64_t c = __shfl(xk, __ffsll((unsigned long long)m) - 1, 64);
                    m &= m - 1;
                    if (c > low) {
                        grp_insert(L, c, a.g, lane);
                        low = __shfl(L, a.g - 1, 64);
                    }
                }
            }
    }
    if (lane < a.g) {
        const int64_t r = (int64_t)(0xFFFFFFFFu - (uint32_t)L);
        D[slot * a.g + lane] = L ? ivr_ord2f((uint32_t)(L >> 32)) : -FLT_MAX;
        I[slot * a.g + lane] = L ? (a.ids ? a.ids[r] : r) : -1;
    }
}

// an empty index: every slot unused
__global__ __launch_bounds__(256) void grp_absent_kernel(int64_t nG, int64_t *__restrict__ Gseg, int64_t nD, float *__restrict__ D, int64_t *__restrict__ I) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (Gseg && i < nG) Gseg[i] = -1;
    if (i < nD) {
        D[i] = -FLT_MAX;
        I[i] = -1;
    }
}

struct GrArgs {
    const float *q;
    int nq;
    const int64_t *seg_off;
    int nseg;
    int G, g;                    // G = 0: best per segment, D / I [nq][nseg] (nseg = 1 without seg_off)
    int normalize_q;
    int64_t *Gseg;
    float *D;
    int64_t *I;
};

// both entry points once their arguments are checked; the caller holds x->mu
int grp_search(const char *what, ivr_index *x, const GrArgs &a, hipStream_t s) {
    IVR_REQUIRE(x->ntotal < (1ll << 31), "%s: ntotal=%lld >= 2^31", what, (long long)x->ntotal);
    const int n = (int)x->ntotal, nseg = a.seg_off ? a.nseg : 1;
    if (n == 0) {
        const int64_t nG = a.G ? (int64_t)a.nq * a.G : 0, nD = a.G ? nG * a.g : (int64_t)a.nq * nseg;
        hipLaunchKernelGGL(grp_absent_kernel, dim3((unsigned)ivr_ceil_div(nD, 256)), dim3(256), 0, s, nG, a.Gseg, nD, a.D, a.I);
        IVR_LAUNCH_CHECK();
        return IVR_OK;
    }
    const int64_t ntiles = ivr_ceil_div(n, 16);
    const bool rows_pass = a.G && a.g > 1;
    const int parts = rows_pass ? (int)std::min<int64_t>(kGrMaxParts, ivr_ceil_div(ntiles, kGrPieceTiles)) : 0;
    const int64_t per_slot = (int64_t)parts * kGrWaves * a.g;             // list keys of one result slot
    // queries per chunk, in whole 16-query tiles: segbest and the lists within the slot budget each
    int64_t cb = std::min<int64_t>({ivr_round_up(a.nq, 16), x->seq_chunk_slots / nseg, (int64_t)kGrMaxChunk});
    if (rows_pass) cb = std::min<int64_t>(cb, x->seq_chunk_slots / ((int64_t)a.G * per_slot));
    cb = std::max<int64_t>(16, cb / 16 * 16);
    const int64_t slots = cb * std::max(a.G, 1);
    int rc = ivr_reserve_queries(x, (int)ivr_ceil_div(a.nq, 16));
    // each buffer grows on its own: calls of different shapes must not shrink one another's scratch
    if (rc == IVR_OK) rc = ivr_reserve({{&x->gr_best, (size_t)cb * nseg * 8}});
    if (rc == IVR_OK && a.G) rc = ivr_reserve({{&x->gr_rows, (size_t)slots * 12}});
    if (rc == IVR_OK && rows_pass) rc = ivr_reserve({{&x->gr_lists, (size_t)slots * per_slot * 8}});
    const size_t lds = (size_t)16 * x->dp * 4;
    if (rc == IVR_OK) rc = ivr_func_max_lds(reinterpret_cast<const void *>(grp_segbest_kernel), (int)lds);
    if (rc != IVR_OK) return rc;
    rc = ivr_launch_tile_rows(x, x->qtiled, a.q, 0, a.nq, a.normalize_q, nullptr, s);
    if (rc != IVR_OK) return rc;
    rc = ivr_launch_rowseg(x, a.seg_off, nseg, s);
    if (rc != IVR_OK) return rc;
    const int64_t *ids = x->has_ids ? x->ids : nullptr;
    const float4 *data = reinterpret_cast<const float4 *>(x->data), *qtiled = reinterpret_cast<const float4 *>((const float *)x->qtiled);
    int64_t *rows = x->gr_rows;
    float *head = reinterpret_cast<float *>(rows + slots);               // the group scores of a call with g > 1: read by nobody
    for (int b0 = 0; b0 < a.nq; b0 += (int)cb) {
        const int cnt = (int)std::min<int64_t>(cb, a.nq - b0);
        const int qtiles = (int)ivr_ceil_div(cnt, 16);
        IVR_HIP(hipMemsetAsync(x->gr_best, 0, (size_t)cnt * nseg * 8, s));
        {
            IvrProf prof("grp_segbest", s, (double)qtiles * 16 * n * 2.0 * x->dp);
            const GrBest gb{data, qtiled + (int64_t)(b0 >> 4) * x->dp4 * 16, x->dp4, qtiles, ntiles, x->gr_seg, nseg, cnt, x->gr_best};
            hipLaunchKernelGGL(grp_segbest_kernel, dim3((unsigned)(ivr_ceil_div(ntiles, kGrTilesPerBlock) * qtiles)), dim3(256), lds, s, gb);
            IVR_LAUNCH_CHECK();
        }
        if (!a.G) {
            const int64_t nslots = (int64_t)cnt * nseg;
            IvrProf prof("grp_select", s, (double)nslots * 8, true);
            hipLaunchKernelGGL(grp_decode_kernel, dim3((unsigned)ivr_ceil_div(nslots, 256)), dim3(256), 0, s, x->gr_best, nslots, ids,
                               a.D + (int64_t)b0 * nseg, a.I + (int64_t)b0 * nseg);
            IVR_LAUNCH_CHECK();
            continue;
        }
        const int64_t nslots = (int64_t)cnt * a.G;
        {
            IvrProf prof("grp_select", s, (double)cnt * nseg * 8, true);
            launch_select<OUT_DI>(SrcSegBest{x->gr_best, nseg}, cnt, a.G, SelectOut::to_rows(rows_pass ? head : a.D + (int64_t)b0 * a.G, rows), s);
            IVR_LAUNCH_CHECK();
            hipLaunchKernelGGL(grp_label_kernel, dim3((unsigned)ivr_ceil_div(nslots, 256)), dim3(256), 0, s, rows, nslots, a.seg_off, nseg, ids,
                               a.Gseg + (int64_t)b0 * a.G, rows_pass ? nullptr : a.I + (int64_t)b0 * a.G);
            IVR_LAUNCH_CHECK();
        }
        if (!rows_pass) continue;
        const GrRows gr{data, qtiled, x->dp4, n, a.seg_off, nseg, b0, a.G, a.g, parts, rows, x->gr_lists, ids};
        {
            IvrProf prof("grp_rows", s, (double)nslots * 16 * x->dp * 4);
            hipLaunchKernelGGL(grp_rows_kernel, dim3((unsigned)nslots, (unsigned)parts), dim3(64 * kGrWaves), 0, s, gr);
            IVR_LAUNCH_CHECK();
        }
        IvrProf prof("grp_merge", s, (double)nslots * per_slot * 8, true);
        hipLaunchKernelGGL(grp_merge_kernel, dim3((unsigned)ivr_ceil_div(nslots, 4)), dim3(256), 0, s, gr, nslots, a.D + (int64_t)b0 * a.G * a.g,
                           a.I + (int64_t)b0 * a.G * a.g);
        IVR_LAUNCH_CHECK();
    }
    return IVR_OK;
}

}  // namespace

extern "C" {

int ivr_group_piece_rows(void) { return kGrPieceTiles * 16; }

int ivr_index_search_groups(ivr_index *x, const float *q, int nq, const int64_t *seg_off, int nseg, int G, int g, int normalize_q, int64_t *Gseg,
                            float *D, int64_t *I, ivr_stream stream) {
    IVR_REQUIRE(x && q && Gseg && D && I, "ivr_index_search_groups: NULL argument");
    IVR_REQUIRE(nq >= 1, "ivr_index_search_groups: nq=%d < 1", nq);
    IVR_REQUIRE(G >= 1, "ivr_index_search_groups: G=%d < 1", G);
    IVR_REQUIRE(g >= 1 && g <= IVR_GROUP_MAX_ROWS, "ivr_index_search_groups: g=%d outside [1,%d]", g, IVR_GROUP_MAX_ROWS);
    IVR_REQUIRE((int64_t)G * g <= IVR_MAX_K, "ivr_index_search_groups: G * g = %lld > %d", (long long)G * g, IVR_MAX_K);
    IVR_REQUIRE(!seg_off || nseg >= 1, "ivr_index_search_groups: nseg=%d with seg_off", nseg);
    std::lock_guard<std::mutex> lk(x->mu);
    IVR_HIP(hipSetDevice(x->ctx->device));
    return grp_search("ivr_index_search_groups", x, GrArgs{q, nq, seg_off, nseg, G, g, normalize_q, Gseg, D, I}, (hipStream_t)stream);
}

int ivr_index_best_per_segment(ivr_index *x, const float *q, int nq, const int64_t *seg_off, int nseg, int normalize_q, float *D, int64_t *I,
                               ivr_stream stream) {
    IVR_REQUIRE(x && q && D && I, "ivr_index_best_per_segment: NULL argument");
    IVR_REQUIRE(nq >= 1, "ivr_index_best_per_segment: nq=%d < 1", nq);
    IVR_REQUIRE(!seg_off || nseg >= 1, "ivr_index_best_per_segment: nseg=%d with seg_off", nseg);
    IVR_REQUIRE(!seg_off || (int64_t)nq * nseg < (1ll << 31), "ivr_index_best_per_segment: nq * nseg = %lld >= 2^31", (long long)nq * nseg);
    std::lock_guard<std::mutex> lk(x->mu);
    IVR_HIP(hipSetDevice(x->ctx->device));
    return grp_search("ivr_index_best_per_segment", x, GrArgs{q, nq, seg_off, nseg, 0, 1, normalize_q, nullptr, D, I}, (hipStream_t)stream);
}

}  // extern "C"
