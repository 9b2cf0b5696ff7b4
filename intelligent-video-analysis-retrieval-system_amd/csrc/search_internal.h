// The one internal header of the flat index.  Not part of the C ABI.  What it holds, in order:
//   plan constants, ScanQArgs     the sizes the flat search files agree on; one launch of the large-batch candidate scan
//   RowMask, with_mask            the allowed rows of a filtered search, and the plain-or-masked choice of a kernel instantiation
//   the float32 score             mfma_chunk4 (one 16-float chunk), stream_tile (one stored 16-row tile against query tiles staged
//                                 in LDS) and pair_score (one tile against one query column in global memory).  Together they are
//                                 THE accumulation order of every float32 score: ascending chunks, x y z w inside a chunk, zero
//                                 accumulator.  Every exact kernel goes through them, which is why a (query, row) pair has the same
//                                 bits wherever it is scored ("one accumulation order")
//   small device helpers          ivr_load_quad, ivr_key, ivr_wave_incl_scan, ivr_last_le, ivr_comp, probe_valid
//   DevMem, DevBuf, ivr_reserve   grow-only device buffers
//   ProbeTables                   the probe tables of the inverted-list scans (defined in search_lists.hip)
//   ivr_index                     the index object: storage, every workspace, and the plan of a search
//   View, with_view               the rows one search scans
//   launchers                     defined in one file and called from another
//   bin_load_row, bin_with_words  the loaders of the binary-code layout (search_binary.hip, search_pq.hip, search_ivfpq.hip; the
//                                 coded-index structs themselves are in search_coded.h)
// Users: search_index.hip (the index object and its storage), search.hip (group-maximum scans and the top-k driver), search_range.hip,
// search_scanq.hip, search_ids.hip, search_rows.hip, search_refine.hip, search_seq.hip, search_events.hip, search_groups.hip,
// search_moments.hip, search_diverse.hip, search_fused.hip, search_videos.hip, search_ivf.hip and the other list scans, and through self_join.h cluster.hip, knn.hip and tags.hip.
#pragma once
#include "ivr_common.h"

#include <algorithm>
#include <cfloat>
#include <initializer_list>
#include <type_traits>
#include <utility>

constexpr int kGroupRows = 64;       // rows per scan group (4 MFMA row tiles)
constexpr int kBigChunk = 1024;      // queries per launch chain of the large-batch scan
// default of IVR_FIND_TABLE_MIN_KEYS (ivr_index_find_ids): the smallest measured key count at which a table lookup INCLUDING one rebuild
// beats the scan on 1M rows (0.161 ms against 0.171 ms; at 256 keys the scan's 0.097 ms wins; profiles/r14a_bench_row_access.log)
constexpr long long kFindTableMinKeys = 512;
constexpr int kBigMaxK = 128;        // beyond this k the chunks of 64 queries are used (candidate lists grow with k)

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

// Plain or masked instantiation of a kernel, chosen once: f(std::false_type) without a mask, f(std::true_type, mask) with one.  A
// launcher writes  with_mask(v.mask, [&](auto masked, auto... m) { auto *k = kernel<.., decltype(masked)::value, decltype(m)...>;
// ... launch k with (args..., m...) })  and so names its kernel and its argument list once.
template <typename M, typename F>
void with_mask(const M *mask, F &&f) {
    if (mask) f(std::true_type{}, *mask);
    else f(std::false_type{});
}

// One 16-float chunk of a float32 score: lane l holds floats 4 (l >> 4) .. + 3 of the chunk for row / query (l & 15) in a and b.
// Every float32 score of the index is accumulated by this sequence in ascending chunk order from a zero accumulator, through one of
// the two loops below; that is what makes them bit-identical to each other.
__device__ __forceinline__ void mfma_chunk4(f32x4 &acc, const float4 &a, const float4 &b) {
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, b.x, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, b.y, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, b.z, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, b.w, acc, 0, 0, 0);
}

// One stored 16-row tile streamed against QT query tiles: at is this lane's float4 of the tile's chunk 0 (a tile is [d/4][16 rows]
// [4 floats], so its chunks are 64 float4 = 1 KiB apart and adjacent in memory), f(q, kc, av) accumulates chunk kc, whose A operand
// is av, into query tile q (mfma_chunk4 with the caller's B operand, usually read from LDS).  Eight chunks per trip, the eight
// independent 1 KiB loads = 8 KiB contiguous in flight per wave before the first MFMA, then single chunks.  Per accumulator the
// chunk order is ascending whatever the trip shape.
template <int QT, typename F>
__device__ __forceinline__ void stream_tile(const float4 *__restrict__ at, int kchunks, F &&f) {
    int kc = 0;
    for (; kc + 8 <= kchunks; kc += 8) {
        float4 av[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) av[u] = at[(kc + u) * 64];
#pragma unroll
        for (int u = 0; u < 8; ++u)
#pragma unroll
            for (int q = 0; q < QT; ++q) f(q, kc + u, av[u]);
    }
    for (; kc < kchunks; ++kc) {
        const float4 av = at[kc * 64];
#pragma unroll
        for (int q = 0; q < QT; ++q) f(q, kc, av);
    }
}

// One 16-row tile against one query column, both operands in global memory: a and b are this lane's float4 of chunk 0 of the row tile
// and of the tiled query tile (chunks 64 float4 apart in both).  pair_chunks: U chunks from kc0 on, every load of both operands
// issued before the first MFMA.  pair_score: the whole row, 16 chunks at a time, then MID at a time when MID > 1, then single chunks.
template <int U>
__device__ __forceinline__ void pair_chunks(f32x4 &acc, const float4 *__restrict__ a, const float4 *__restrict__ b, int kc0) {
    float4 av[U], bv[U];
#pragma unroll
    for (int u = 0; u < U; ++u) av[u] = a[(kc0 + u) * 64];
#pragma unroll
    for (int u = 0; u < U; ++u) bv[u] = b[(kc0 + u) * 64];
#pragma unroll
    for (int u = 0; u < U; ++u) mfma_chunk4(acc, av[u], bv[u]);
}
template <int MID = 1>
__device__ __forceinline__ f32x4 pair_score(const float4 *__restrict__ a, const float4 *__restrict__ b, int kchunks) {
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    int kc = 0;
    for (; kc + 16 <= kchunks; kc += 16) pair_chunks<16>(acc, a, b, kc);
    if constexpr (MID > 1)
        for (; kc + MID <= kchunks; kc += MID) pair_chunks<MID>(acc, a, b, kc);
    for (; kc < kchunks; ++kc) pair_chunks<1>(acc, a, b, kc);
    return acc;
}

// One quad of a row-major float32 row for the tiled layouts: floats k0 .. k0 + 3 of `row`, zero past d.  vec: one 16-byte load (the
// caller guarantees k0 + 3 < d and the alignment)
__device__ __forceinline__ float4 ivr_load_quad(const float *__restrict__ row, int k0, int d, bool vec) {
    if (vec) return *reinterpret_cast<const float4 *>(row + k0);
    float4 v;
    v.x = k0 + 0 < d ? row[k0 + 0] : 0.f;
    v.y = k0 + 1 < d ? row[k0 + 1] : 0.f;
    v.z = k0 + 2 < d ? row[k0 + 2] : 0.f;
    v.w = k0 + 3 < d ? row[k0 + 3] : 0.f;
    return v;
}

// The 64-bit result key of every top-k of the project: (ordered score, ~position).  The larger key ranks first, so equal scores rank
// the LOWER position first; 0 is below every key and stands for "no row".
__device__ __forceinline__ uint64_t ivr_key(float score, uint32_t pos) {
    return ((uint64_t)ivr_f2ord(score) << 32) | (uint32_t)(0xFFFFFFFFu - pos);
}

// inclusive prefix sum over the 64 lanes of a wave (lane = threadIdx.x & 63, which most callers hold already)
template <typename T>
__device__ __forceinline__ T ivr_wave_incl_scan(T v, int lane = threadIdx.x & 63) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const T t = __shfl_up(v, o, 64);
        if (lane >= o) v += t;
    }
    return v;
}

// the last i in [0, n) with off[i] <= v (off ascending, off[0] <= v): with empty runs (equal neighbours) that is the one run that
// holds v
__device__ __forceinline__ int ivr_last_le(const int64_t *off, int n, int64_t v) {
    int lo = 0, hi = n - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (off[mid] <= v) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// component c of a 16-byte word (the table-lookup scans walk a code four bytes at a time)
__device__ __forceinline__ uint32_t ivr_comp(const uint4 &v, int c) { return c == 0 ? v.x : c == 1 ? v.y : c == 2 ? v.z : v.w; }

// An inverted-file search names its lists in assign [nq][p], every row ascending (so a list named twice sits in adjacent entries and
// counts once); entries outside [0, nlist) are skipped.  true: entry j of row a is the first mention of a valid list
__device__ __forceinline__ bool probe_valid(const int64_t *__restrict__ a, int j, int p, int nlist) {
    if (j >= p) return false;
    const int64_t l = a[j];
    return l >= 0 && l < nlist && (j == 0 || a[j - 1] != l);
}

// Grow-only device buffer: DevMem owns the block and frees it in its destructor, DevBuf<T> is the same block read as a T *.  Grown
// by ivr_reserve (search_index.hip).
struct DevMem {
    void *ptr = nullptr;
    size_t bytes = 0;
    DevMem() = default;
    DevMem(const DevMem &) = delete;
    DevMem &operator=(const DevMem &) = delete;
    ~DevMem() {
        if (ptr) (void)hipFree(ptr);
    }
};
template <typename T>
struct DevBuf : DevMem {
    operator T *() const { return static_cast<T *>(ptr); }
};
// ivr_reserve({{&buf, bytes}, ...}, zero) grows a group of buffers that are sized together.  Nothing happens while EVERY buffer of
// the group holds the bytes asked of it.  Otherwise every old block is freed before the first new one is allocated (a workspace
// never holds two generations), then each is allocated (a size of 0 leaves that buffer empty) and, when asked, zero-filled.  All
// or nothing: when an allocation fails the whole group is left empty and the error returned, so a repeated call tries again.
typedef std::initializer_list<std::pair<DevMem *, size_t>> DevSizes;
int ivr_reserve(DevSizes bufs, bool zero = false);
// every buffer of the group empty again (the sizes are not read); the first error, if any
int ivr_release(DevSizes bufs);

// ---- probe tables of a list-major inverted-list scan (defined in search_lists.hip) ---------------------------------------------
// keys of the scratch a chunk of queries may fill: 2^25 slots of 8 bytes = 256 MiB, plus one query's stretch when a single query
// probes more rows than that (its stretch is never split)
constexpr int64_t kIvfChunkSlots = 1ll << 25;
// pairs of a chunk: bounds the pair tables (20 bytes per pair) at 80 MiB
constexpr int64_t kIvfChunkPairs = 1ll << 22;

// The scratch, the chunk plan and the table build of a scan that groups the (query, list) pairs of a chunk of queries by list
// (search_ivf.hip, search_ivfsq.hip).  Grow-only.
struct ProbeTables {
    int64_t chunk_slots = kIvfChunkSlots;    // key slots of a chunk of queries (one query's stretch at least)
    DevBuf<uint64_t> keys;               // [chunk][qstride]: the key of every probed row, in its query's own stretch
    DevBuf<int64_t> slot;                // [chunk][p]: first key slot of each probed list, -1 for a skipped entry
    DevBuf<int64_t> qtotal;              // [chunk]: rows each query probes
    DevBuf<int> count;                   // [nlist]: queries per list, then the fill cursors
    DevBuf<int64_t> off;                 // [nlist + 1] pairs in front of each list, then [nlist + 1] 16-query pair tiles in front of it
    DevBuf<int> pair_q;                  // [pairs of a chunk]: the (query, list) pairs grouped by list: the query of the chunk ...
    DevBuf<int64_t> pair_slot;           // ... and its first key slot for that list
    int64_t *pair_off() const { return off; }
    int64_t *tile_off(int nlist) const { return (int64_t *)off + nlist + 1; }
    // pair tiles of a chunk of npairs pairs at most: every probed list has one partly filled tile at most
    static int64_t tiles(int nlist, int64_t npairs) { return std::min<int64_t>(nlist, npairs) + npairs / 16; }
    // The plan of a search of nq queries that name p lists each and may probe qstride rows each: chunk = queries per chunk (the
    // scratch holds chunk_slots keys, the pair tables kIvfChunkPairs pairs), nkeys = key slots of a chunk; reserves one chunk
    int plan(int nq, int p, int64_t qstride, int nlist, int *chunk, int64_t *nkeys);
    // The tables of the nqc queries whose ascending assign rows [nqc][p] start at `assign`, over the lists list_off [nlist + 1] of
    // ntotal rows: a memset and four launches on stream s (probe_slots, probe_count, probe_offsets, probe_fill); the caller checks
    // the launches
    int build(const int64_t *assign, int p, int nqc, const int64_t *list_off, int nlist, int64_t ntotal, int64_t qstride, hipStream_t s);
    // The best k keys of each of the nqc queries' stretches -> D, I [nqc][k]; the label of a key's low word r is ids[r], or r itself
    // without ids (select_topk_kernel, one workgroup per query)
    void select(int nqc, int k, int64_t qstride, float *D, int64_t *I, const int64_t *ids, hipStream_t s);
};

struct ivr_index {
    ivr_ctx *ctx = nullptr;
    int d = 0, dp = 0, dp4 = 0;
    int64_t cap = 0, ntotal = 0;     // cap is a multiple of kGroupRows
    float *data = nullptr;
    std::mutex mu;
    // search workspace (grow-only)
    DevBuf<float> qtiled;            // [qtiles][dp4][16][4]
    DevBuf<float> qnorm;             // [qtiles*16] upper bound of each tiled query's norm (bf16 candidate scan verification)
    DevBuf<float> gmax;              // [qcols][mstride]
    DevBuf<uint32_t> sel;            // [nq][ksel]
    DevBuf<uint64_t> cand;           // [nq][ksel*64]
    // bf16 candidate scan (scan16_groupmax_kernel): scan copy of the rows, split queries, verification state
    bool scan16 = false;             // IVR_SCAN_BF16 (default on), fixed at creation
    int pieces = 0;                  // 1 KiB pieces of a 16-row tile = ceil(dp / 32)
    uint4 *data16 = nullptr;         // [cap/16][pieces][64]
    DevBuf<uint4> q16hi, q16lo;      // [qtiles][pieces][64]
    DevBuf<unsigned int> maxnorm;    // DEV: bits of the largest stored row norm
    DevBuf<int> okflag;              // DEV [64] per scan chunk + [4] tile flags behind it
    int last_nqc = 0;                // queries of the last chunk that went through the candidate scan
    // large-batch candidate scan (search_scanq.hip): more than 64 queries per call
    DevBuf<unsigned int> maxdelta;   // DEV: bits of the largest |row - bf16(row)| over the stored rows
    DevBuf<float> qdelta;            // DEV [qtiles*16]: |q - bf16(q)| of each tiled query
    DevBuf<float> tmax;              // DEV [padded queries of a chunk][tstride]: 16-row tile maxima (also the gmax of its exact pass)
    DevBuf<float> bmax;              // DEV [padded queries of a chunk][bstride]: 128-row block maxima
    DevBuf<uint32_t> selb;           // DEV [queries of a chunk][kp + 1]: selected blocks
    DevBuf<int> okq;                 // DEV [kBigChunk] verification result per query, [4] failure count, [kBigChunk] failed queries
    bool last_big = false;           // the last search went through the large-batch scan
    bool bigq = true;                // IVR_SCAN_BIGQ=0 keeps every batch on the 64-query chunks (A/B switch, read at creation)
    bool prune = true;               // IVR_SCAN_PRUNE=0: the large-batch re-score fetches all kp selected tiles (A/B switch)
    bool ring = true;                // IVR_SCAN_RING=0: the <= 16-query candidate scan streams the index through registers (A/B switch)
    // exact range search (ivr_index_range_search), one chunk of <= 64 queries: [64][mstride] entries each, grow-only
    DevBuf<uint32_t> rs_cand;        // candidate groups of each query, ascending
    DevBuf<uint64_t> rs_mask;        // hit mask of each (query, candidate group): bit i = row 64 g + i scores > radius
    DevBuf<uint32_t> rs_off;         // hits of each pair, then (in place) their exclusive prefix sum within the query
    DevBuf<uint32_t> rs_count;       // DEV [64] candidate groups per query, [64] hits per query, then int64 [2]: running total
    // row removal (ivr_index_remove_ids), grow-only: the tail = the rows from the 256-row block of the first allowed row on
    int64_t remove_chunk = 65536;    // IVR_REMOVE_CHUNK_ROWS: source rows per step through the bounce buffer (a multiple of 64, read at creation)
    DevBuf<uint64_t> rm_word;        // DEV [groups of the tail + 1]: bit i = row 64 g + i is stored and stays
    DevBuf<uint32_t> rm_kept;        // DEV [groups of the tail + 1]: kept rows of each group, then their prefix inside a block of 1024 groups
    DevBuf<uint32_t> rm_top;         // DEV [blocks of 1024 groups]: kept rows of each block, then their exclusive prefix
    DevBuf<uint32_t> rm_state;       // DEV: first removed row of the tail (0xffffffff: none), kept rows of the tail, then the kept rows in
                                     // front of every unit of 16 groups: what the host reads back to plan the walk
    DevBuf<float> rm_bounce;         // DEV [remove_chunk / 16 + 1 tiles]: the survivors of one step, already tiled for their destination
    DevBuf<uint4> rm_bounce16;       // the same tiles of the bf16 scan copy
    // stable external ids (ivr_index_add_with_ids, search_ids.hip): an id-mapped index labels row r ids[r] instead of id_base + r
    bool has_ids = false;            // set by the first ivr_index_add_with_ids on an empty index, cleared by ivr_index_reset
    int64_t *ids = nullptr;          // DEV [cap] while has_ids: grows with the rows (index_alloc), entries >= ntotal are never read
    DevBuf<uint64_t> ids_rows;       // DEV [cap / 64] row bitmap of a filter over stored ids: bit i of word g = row 64 g + i is allowed
    DevBuf<int64_t> ids_moved;       // DEV [rows from the first removed one on]: their surviving ids in order (ivr_index_remove_ids)
    // hash table from stored id to lowest row (ivr_index_find_ids, search_ids.hip): open addressing, linear probing, empty key -1
    int64_t find_table_min = 0;      // IVR_FIND_TABLE_MIN_KEYS: lookups of at least this many keys use the table (read at creation)
    DevBuf<int64_t> tab_keys;        // DEV [tab_slots]: nothing until the first table lookup; freed by ivr_index_reset
    DevBuf<unsigned long long> tab_rows;     // DEV [tab_slots]: the lowest row that holds the slot's key
    int64_t tab_slots = 0;           // power of two >= 2 ntotal of the build
    bool tab_ok = false;             // the table matches ids[0 .. ntotal): cleared by add_with_ids, remove_ids and reset
    // ivr_index_search_reconstruct (search_rows.hip): the row position behind every result slot of a search
    DevBuf<int64_t> rpos;            // DEV [nq][k], sized by ivr_index_reserve_search
    ProbeTables ivf;                 // inverted-list search (ivr_index_search_lists, search_ivf.hip); chunk_slots: IVR_IVF_CHUNK_SLOTS (read at creation)
    // exact re-ranking of candidate lists (ivr_index_rescore, search_refine.hip); grow-only
    DevBuf<uint64_t> refine_keys;    // DEV [nq][kc]: (ordered score, ~row) of every candidate, 0 for an absent one
    // clip search (ivr_index_search_sequences, search_seq.hip), one chunk of target windows; grow-only
    int64_t seq_chunk_slots = 1ll << 25;     // IVR_SEQ_CHUNK_SLOTS: key slots of a chunk of windows (one window's stretch at least; read at creation)
    DevBuf<float> seq_scores;        // DEV [frames of a chunk, whole 16-frame tiles][stored rows rounded up to 16]: frame scores S
    DevBuf<uint64_t> seq_keys;       // DEV [windows of a chunk][N - L + 1]: (ordered window score, ~start row), 0 for a start that is no candidate
    DevBuf<int64_t> seq_off;         // DEV [windows of a chunk][4096-key blocks of a stretch]: hits of each block, then their output positions
    DevBuf<int64_t> seq_total;       // DEV [1]: the running total of the range call, carried from chunk to chunk
    // the self-joins (self_join.h); grow-only
    DevBuf<int32_t> sj_seg;          // DEV [2][ntotal rounded up to 64]: start and end of each row's segment
    // event search (ivr_index_search_events, search_events.hip), one chunk of chains; grow-only.  The frame scores go to seq_scores
    DevBuf<uint64_t> ev_keys;        // DEV [2][chains of a chunk][ntotal]: (ordered C[j], ~row) of the previous and of this step, 0 = no candidate
    DevBuf<uint16_t> ev_pred;        // DEV [chains of a chunk][m - 1][ntotal]: r - P[j, r] of every candidate of step j >= 1
    DevBuf<int64_t> ev_rows;         // DEV [chains of a chunk][k or nseg]: the end row behind every result slot, -1 for an unused one
    // frame clustering (ivr_index_dbscan, cluster.hip); grow-only
    DevBuf<int32_t> cl_words;        // DEV [5][ntotal + 1 rounded up to 64]: degree, parent, root, border root, root prefix of each row
    // neighbour graph (ivr_index_knn_graph, knn.hip); grow-only
    DevBuf<uint64_t> kn_keys;        // DEV [query blocks of a chunk][parts of a walk][64][k]: the partial lists, at most 2^25 keys
    // grouped search (ivr_index_search_groups, search_groups.hip), one chunk of queries; grow-only, each on its own
    DevBuf<int32_t> gr_seg;          // DEV [ntotal rounded up to 16]: the segment of each row, -1 in front of the first and nseg behind the last
    DevBuf<uint64_t> gr_best;        // DEV [queries of a chunk][nseg]: the greatest (ordered score, ~row) of each segment, 0 = no row
    DevBuf<int64_t> gr_rows;         // DEV [queries of a chunk][G]: the best row of each chosen group (-1: unused), then as many floats
    DevBuf<uint64_t> gr_lists;       // DEV [queries of a chunk][G][pieces][4 waves][g]: the partial row lists, at most IVR_SEQ_CHUNK_SLOTS keys
    // diversified search (ivr_index_diversify, search_diverse.hip); grow-only
    DevBuf<float> dv_scores;         // DEV [nq][kc]: the relevance score of every candidate, -FLT_MAX for an absent one
    // fused search (ivr_index_search_fused, search_fused.hip), one chunk of fused queries; grow-only
    DevBuf<uint64_t> fu_keys;        // DEV [fused queries of a chunk][ntotal rounded up to 16]: (ordered F, ~row), 0 for a padding row
    DevBuf<int64_t> fu_off;          // DEV [fused queries of a chunk][4096-key blocks of a stretch]: hits of each block, then their output positions
    DevBuf<int64_t> fu_total;        // DEV [1]: the running total of the range call, carried from chunk to chunk
    // moment search (ivr_index_search_moments, search_moments.hip), one chunk of queries; grow-only.  The frame scores go to seq_scores,
    // the row -> segment table to gr_seg
    DevBuf<int32_t> mo_blk;          // DEV [queries of a chunk][row blocks][4]: first hot row, last hot row, heads, then the prev it enters with
    DevBuf<int64_t> mo_q;            // DEV [queries of a chunk][2]: the moments of each query, then the number of its first moment in the chunk;
                                     // behind them int64 [3]: the running total of the call, the total in front of the chunk, the chunk's moments
    DevBuf<uint64_t> mo_mom;         // DEV, 24 bytes per moment a chunk may hold: peak keys (uint64), lo (int64), hi (int32), cnt (int32), one array each
    DevBuf<int64_t> mo_rows;         // DEV [queries of a chunk][k]: the low word of every chosen rank key (-1: unused), then as many floats
    // zero-shot tagging (ivr_index_tag_rows, ivr_index_tag_segments, tags.hip); grow-only, each on its own
    DevBuf<float> tg_labels;         // DEV [C rounded up to 16][dp]: the labels in the storage-tile layout, zero rows behind the last
    DevBuf<uint64_t> tg_table;       // DEV [nseg][C] uint64 mass, [nseg][C] int32 votes, [nseg] int32 rows: the segment tables of a call
    DevBuf<uint64_t> tg_lists;       // DEV: J, D, P [rows of a chunk][t], then count and Z [rows of a chunk]: the row pass of the segment call
    // video search (ivr_index_video_scores, ivr_index_video_search, search_videos.hip), one chunk of query sets; grow-only, each on its
    // own.  The row -> segment table goes to gr_seg
    DevBuf<float> vi_pack;           // DEV [members rounded up to 16][dp]: the members of the call in the tiled query layout, packed
    DevBuf<float> vi_q;              // DEV [16-member tiles of the call][16][dp]: the same, every set from a tile boundary on
    DevBuf<int32_t> vi_tab;          // DEV [3][nsets + 1]: members, tiles and blocks in front of every set
    DevBuf<uint32_t> vi_fmax;        // DEV [members of a chunk][nseg]: the greatest ordered score of each (member, video), 0 = no row
    DevBuf<uint32_t> vi_bmax;        // DEV [sets of a chunk][ntotal rounded up to 16]: the greatest ordered score of each (set, row)
    DevBuf<uint64_t> vi_sums;        // DEV [3][sets of a chunk][nseg]: Fsum, Bsum (int64), then the keys (ordered V, ~video)

    // The plan of a search: the sizes, bounds and path choices that the reserve functions and the drivers must agree on.
    // strides of the per-query rows of group / 16-row tile / 128-row block maxima, for the index's capacity
    int64_t mstride() const { return ivr_round_up(cap / kGroupRows, 64); }
    int64_t tstride() const { return ivr_round_up(ivr_round_up(cap, 256) / 16, 64); }
    int64_t bstride() const { return ivr_round_up(ivr_round_up(cap, 256) / 128, 64); }
    // 16-query tiles per index pass of the streamed scans: as many as fit 128 KiB of LDS, at most 4; a chunk is 16 * qt_max() queries
    int qt_max() const { return (int)std::max<int64_t>(1, std::min<int64_t>(4, (128 * 1024) / ((int64_t)16 * dp * 4))); }
    // groups re-scored exactly behind the bf16 candidate scan: k plus slack for what the approximate ranking may displace
    static int fast_groups(int k) { return k + std::max(22, k); }
    // bf16 candidate scan first when it can pay: enough groups that kp of them are a small fraction, k within the selector's range
    bool fast_scan(int64_t ngroups, int k) const {
        return scan16 && ngroups >= 4 * (int64_t)(fast_groups(k) + 1) && fast_groups(k) + 1 <= IVR_MAX_K;
    }
    // more than 64 queries: the tiled large-batch scan (search_scanq.hip) instead of chunks of 64 queries past the streamed index
    bool use_big(int nq, int k) const { return scan16 && bigq && nq > 64 && k <= kBigMaxK; }
    // error bound of the bf16 candidate scan relative to |q| max|row|: bf16 keeps 8 significant bits, |row - bf16(row)| <= 2^-8 |row|
    // per element; the query's hi + lo leaves 2^-16; f32 accumulation
    float rel_eps() const { return (0.00390625f + 0.0000306f + (float)dp * 1.2e-7f) * 1.01f; }
    float acc_eps() const { return (float)dp * 1.2e-7f; }        // the accumulation term alone (large-batch scan)
};

// choose the query tile width of the scan (queries per index pass = 16*QT)
inline int pick_qt(int nq) { return nq <= 16 ? 1 : nq <= 32 ? 2 : nq <= 48 ? 3 : 4; }

// The rows one search scans: the whole index, or for a filtered search the whole 256-row blocks that cover the allowed rows, treated as
// an index of their own (the tiled layouts are contiguous per 16-row tile, so data and data16 are offset by whole blocks and the ids
// shifted by the same rows; whole 256-row blocks keep the large-batch scan's block reads inside the allocation).  mask != NULL: the
// masked kernels run, with the allowed rows in this view's numbering.
struct View {
    const float *data;
    const uint4 *data16;
    int64_t ntotal, ngroups, id_base;
    const RowMask *mask;
    const int64_t *ids;      // id-mapped index: the label of row r is ids[r] (id_base is 0 and unused); NULL: id_base + r
};

// search_index.hip.  The view of a search: the whole index without a filter; with one (id = id_base + row) the part it allows and,
// in m, the mask of its allowed rows (a view of 0 rows when nothing is allowed)
View ivr_make_view(const ivr_index *x, int64_t id_base, const ivr_id_filter *f, RowMask &m);

// search_ids.hip.  The view of a search on an id-mapped index: always the whole index, labelled from the id table.  A filter names
// stored ids: one pass over the table on stream s turns it into the row bitmap x->ids_rows, which m then points at (no host
// synchronisation; a view of 0 rows when the filter's range is empty)
int ivr_make_ids_view(ivr_index *x, const ivr_id_filter *f, RowMask &m, hipStream_t s, View &out);

// The shared body of the search entry points once their own arguments are checked: filter check, lock, device, body(view).  s: the
// stream the body launches on
template <typename F>
int with_view(ivr_index *x, int64_t id_base, const ivr_id_filter *f, hipStream_t s, const char *what, F &&body) {
    IVR_REQUIRE(!f || f->nbits >= 0, "%s: filter nbits=%lld < 0", what, (long long)(f ? f->nbits : 0));
    std::lock_guard<std::mutex> lk(x->mu);
    IVR_HIP(hipSetDevice(x->ctx->device));
    RowMask m;
    if (!x->has_ids) return body(ivr_make_view(x, id_base, f, m));
    View v;
    const int rc = ivr_make_ids_view(x, f, m, s, v);
    return rc != IVR_OK ? rc : body(v);
}

// search_index.hip.  dst == x->data: index rows (bf16 scan copy + max norm alongside); dst == x->qtiled: queries (bf16 hi / lo split
// alongside); any other dst (tags.hip's label tiles): the float32 tiles alone, padding rows of the last tile zero-filled as for queries
int ivr_launch_tile_rows(ivr_index *x, float *dst, const float *src, int64_t start, int64_t n, int normalize, int32_t *nonfinite,
                         hipStream_t s, const int64_t *start_dev = nullptr, int64_t max_tiles = 0);
// search_rows.hip.  out[i] = stored row row_base + rows[i] (row-major float32); NaN rows for negative entries and for rows outside
// [0, ntotal); the caller holds x->mu
int ivr_launch_gather(ivr_index *x, const int64_t *rows, int64_t row_base, int64_t n, float *out, hipStream_t s);
// search_refine.hip.  The first launch of ivr_index_rescore for the diversified search too: stages the queries in x->qtiled and scores
// every (query, candidate) pair -> keys [nq][kc] (ordered score, ~row; 0 for an absent entry) and / or D_all [nq][kc] (-FLT_MAX for an
// absent entry), either may be NULL.  The caller holds x->mu, has checked the sizes and launches nothing on an empty index
int ivr_launch_refine_score(ivr_index *x, const float *q, int nq, const int64_t *cand, int kc, int normalize_q, uint64_t *keys, float *D_all,
                            hipStream_t s);
// search.hip.  The search of ivr_index_search_filtered over view v that also leaves the row behind every result slot in x->rpos (DEV
// [nq][k]: its number in the view, -1 for an unused slot); the caller holds x->mu
int ivr_search_view_pos(ivr_index *x, const View &v, const float *q, int nq, int k, int normalize_q, float *D, int64_t *I, hipStream_t s);
// search.hip.  Tiled query buffers for `qtiles` 16-query tiles, and the group maxima of one scan chunk (grow-only); the float32
// scan of 16*qt query columns (tile_flag: see scan_groupmax_kernel) and the bf16 candidate scan of the query tiles from tile0 on,
// both into x->gmax
int ivr_reserve_queries(ivr_index *x, int qtiles);
int ivr_reserve_gmax(ivr_index *x);
void ivr_launch_scan_qt(ivr_index *x, const View &v, int qt, const float *qtile, hipStream_t s, const int *tile_flag = nullptr);
void ivr_launch_fast_scan(ivr_index *x, const View &v, int qt, int64_t tile0, hipStream_t s);
// search_seq.hip.  The score pass of the clip search and the event search: the 16-frame tiles qtile0 .. qtile0 + qtiles - 1 of
// x->qtiled against every stored row -> x->seq_scores [16 qtiles][ntotal rounded up to 16], line f = frame 16 qtile0 + f.  The caller
// holds x->mu, has reserved seq_scores and keeps ceil(ntotal / 1024) * qtiles below 2^31 (the grid)
int ivr_launch_seq_score(ivr_index *x, int qtile0, int qtiles, hipStream_t s);
// search_groups.hip.  The segment number of every stored row -> x->gr_seg [ntotal rounded up to 16] (reserved here): -1 in front of
// seg_off[0], nseg behind seg_off[nseg] and for the padding rows, 0 for every stored row without seg_off (nseg is then taken as 1).
// The caller holds x->mu
int ivr_launch_rowseg(ivr_index *x, const int64_t *seg_off, int nseg, hipStream_t s);
// search_sq.hip.  t int16 [nq][d] -> the int8 halves t = 128 h + l of the int8 MFMA scans, tiled per 16 queries: qh and ql
// [qtiles][ksteps][64], zeros past d and past nq
void ivr_launch_sq_stage(const int16_t *t, int nq, int d, int ksteps, int64_t qtiles, uint4 *qh, uint4 *ql, hipStream_t s);
// search_scanq.hip
int ivr_launch_scanq(ivr_ctx *ctx, const ScanQArgs &a, hipStream_t s, const RowMask *mask = nullptr);

// ---- the layout of binary codes (search_binary.hip), scanned by search_pq.hip and, per list, by search_ivfpq.hip too ---------------
// The row of this lane: row 64 g + lane of the index layout
template <int W>
__device__ __forceinline__ void bin_load_row(const uint4 *__restrict__ data, int64_t g, uint4 (&row)[W]) {
    const uint4 *p = data + g * (W * 64) + (threadIdx.x & 63);
#pragma unroll
    for (int w = 0; w < W; ++w) row[w] = p[w * 64];
}

// f(std::integral_constant<int, W>) for the index's word count
template <typename F>
void bin_with_words(int w16, F &&f) {
    switch (w16) {
        case 1: f(std::integral_constant<int, 1>{}); break;
        case 2: f(std::integral_constant<int, 2>{}); break;
        case 3: f(std::integral_constant<int, 3>{}); break;
        case 4: f(std::integral_constant<int, 4>{}); break;
        case 8: f(std::integral_constant<int, 8>{}); break;
        default: f(std::integral_constant<int, 16>{}); break;
    }
}
