// Flat inner-product index on MI355X: tiled HBM layout, streaming scan with f32 MFMA,
// exact top-k by group maxima + radix select.  (I1, N2/N3, S1 of SURVEY.md section 8a.)
//
// Replaces faiss.IndexFlatIP.add/search as called at unified_index.py:1767-1779,503 and
// core.py:827,891.  Design:
//
//   layout   rows are stored in tiles of 16 rows; inside a tile the order is [d/4][16 rows][4 floats],
//            so lane l of a wave reading float4 number l of a 1 KiB piece holds row (l & 15),
//            floats 16*kc + 4*(l >> 4) .. +3: exactly the A fragment of v_mfma_f32_16x16x4_f32 for four
//            consecutive MFMAs.  Every wave-wide load is 1 KiB contiguous.  Queries use the same layout
//            (they are the B fragment), staged once per workgroup in LDS.
//   pass 1   scan: each wave scores a group of 64 rows x (16*QT) queries, reduces the 64 scores of each
//            query to their maximum (15 v_max + 2 wave shuffles) and stores it.  No data-dependent
//            control flow, the index is read exactly once per 16*QT queries.
//   pass 2   per query, radix-select the k groups with the largest (max, lowest group id).  The k best
//            rows always lie inside those k groups (proof in DESIGN.md).
//   pass 3   re-score the selected groups with the same MFMA sequence (bit-identical scores) and emit
//            64-bit keys (ordered score, ~row).
//   pass 4   per query, radix-select + bitonic sort of the k best keys -> D (float32), I (int64).
//   files    the index object and the row layout kernels: search_index.hip; the selector of passes 2 and 4: search_select.h; the
//            shard merge: search_merge.hip; range search: search_range.hip; the large-batch candidate scan: search_scanq.hip.
//   filtered (ivr_index_search_filtered): the same passes over the 256-row blocks that cover the allowed id range,
//            on the masked instantiations (MASK): rows that are not allowed count as -inf in every maximum and get no key.
#include "ivr_common.h"
#include "search_internal.h"
#include "search_select.h"

namespace {

// ---------------------------------------------------------------------------------------------
// the 64-row x 16-query score tile (shared by pass 1 and pass 3 so the scores are bit-identical)
// ---------------------------------------------------------------------------------------------
// a: this lane's float4 pointer into the group's first tile; tiles are tile_stride float4 apart.
// acc[t][r] = <row 16t + 4(lane>>4) + r , query (lane&15)>
template <int QT, typename BLoad>
__device__ __forceinline__ void score_group(const float4 *__restrict__ a, int64_t tile_stride, int kchunks,
                                            BLoad bload, f32x4 (&acc)[QT][4]) {
#pragma unroll
    for (int q = 0; q < QT; ++q)
#pragma unroll
        for (int t = 0; t < 4; ++t) acc[q][t] = f32x4{0.f, 0.f, 0.f, 0.f};
    // one row tile at a time (stream_tile, search_internal.h): per accumulator the K order is ascending, so scan and re-score stay
    // bit-identical
#pragma unroll
    for (int t = 0; t < 4; ++t)
        stream_tile<QT>(a + t * tile_stride, kchunks, [&](int q, int kc, const float4 &av) { mfma_chunk4(acc[q][t], av, bload(q, kc)); });
}

// pass 1.  gmax layout: [16*QT queries][mstride groups]
// the wave loop of the exact scan: every 64-row group against the 16*QT queries staged in qs
// MASK (filtered search): rows that are not allowed count as -inf, allowed ones as max(score, -FLT_MAX) (search_internal.h)
// The masked instantiations take the mask as a trailing parameter pack (one RowMask; empty for the plain ones, whose parameter lists and
// code stay exactly what they were).
template <int QT, bool MASK = false, typename... M>
__device__ __forceinline__ void scan_groups_body(const float4 *__restrict__ qs, const float *__restrict__ data, int dp4, int64_t ngroups,
                                                 int64_t ntotal, float *__restrict__ gmax, int64_t mstride, const M &...rm) {
    const int per_tile = dp4 * 16;   // float4 per 16-row tile
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
    const int kchunks = dp4 >> 2;
    auto bload = [&](int q, int kc) { return qs[q * per_tile + kc * 64 + lane]; };
    for (int64_t g = (int64_t)blockIdx.x * nw + wave; g < ngroups; g += (int64_t)gridDim.x * nw) {
        f32x4 acc[QT][4];
        const float4 *a = reinterpret_cast<const float4 *>(data) + g * 4 * (int64_t)per_tile + lane;
        uint32_t mbyte = 0;
        if constexpr (MASK) mbyte = row_mask_fetch(rm..., g * kGroupRows);
        score_group<QT>(a, per_tile, kchunks, bload, acc);
        const bool partial = (g + 1) * kGroupRows > ntotal;   // wave-uniform: only the last group
        uint64_t mw = 0;
        if constexpr (MASK) mw = row_mask_word(rm..., g * kGroupRows, mbyte) >> ((lane >> 4) * 4);
#pragma unroll
        for (int q = 0; q < QT; ++q) {
            float m = MASK ? -INFINITY : -FLT_MAX;
#pragma unroll
            for (int t = 0; t < 4; ++t)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    float s = acc[q][t][r];
                    if constexpr (MASK) s = row_mask_score(mw, t * 16 + r, s);
                    else if (partial && g * kGroupRows + t * 16 + (lane >> 4) * 4 + r >= ntotal) s = -FLT_MAX;
                    m = fmaxf(m, s);
                }
            m = fmaxf(m, __shfl_xor(m, 16, 64));
            m = fmaxf(m, __shfl_xor(m, 32, 64));
            if (lane < 16) gmax[(int64_t)(q * 16 + lane) * mstride + g] = m;
        }
    }
}

template <int QT, bool MASK, typename... M>
__global__ __launch_bounds__(512) void scan_groupmax_kernel(const float *__restrict__ data,
                                                            const float *__restrict__ qtiled, int dp4,
                                                            int64_t ngroups, int64_t ntotal,
                                                            float *__restrict__ gmax, int64_t mstride,
                                                            const int *__restrict__ tile_flag, M... rm) {
    extern __shared__ __attribute__((aligned(16))) float4 qs[];
    if (tile_flag) {       // fallback pass behind the bf16 candidate scan: only query tiles that failed their verification
        bool any = false;
#pragma unroll
        for (int i = 0; i < QT; ++i) any |= tile_flag[i] != 0;
        if (!any) return;
    }
    const int per_tile = dp4 * 16;
    for (int i = threadIdx.x; i < QT * per_tile; i += blockDim.x) qs[i] = reinterpret_cast<const float4 *>(qtiled)[i];
    __syncthreads();
    scan_groups_body<QT, MASK>(qs, data, dp4, ngroups, ntotal, gmax, mstride, rm...);
}

// Exact pass behind the LARGE-batch candidate scan: the queries whose verification failed were appended to `list` by the final
// selection (count = *nlist, known on the device only).  Each chunk of 16*QT listed queries is gathered from the tiled query
// buffer straight into LDS (element (kc, lane) of a staged tile = the float4 of query (lane & 15), quad (lane >> 4), chunk kc)
// and scanned like any other; nothing listed: every workgroup exits at once.  gmax row = position in the list.
template <int QT, bool MASK, typename... M>
__global__ __launch_bounds__(512) void scan_groupmax_list_kernel(const float *__restrict__ data, const float *__restrict__ qtiled,
                                                                 int dp4, int64_t ngroups, int64_t ntotal, float *__restrict__ gmax,
                                                                 int64_t mstride, const int *__restrict__ nlist,
                                                                 const int *__restrict__ list, M... rm) {
    extern __shared__ __attribute__((aligned(16))) float4 qs[];
    const int nf = *nlist;
    const int per_tile = dp4 * 16;
    for (int c0 = 0; c0 < nf; c0 += 16 * QT) {
        __syncthreads();                               // the previous chunk's waves are done with qs
        for (int i = threadIdx.x; i < QT * per_tile; i += blockDim.x) {
            const int t = i / per_tile, r = i - t * per_tile, l = r & 63;
            const int pos = c0 + t * 16 + (l & 15);
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (pos < nf) {
                const int src = list[pos];
                v = reinterpret_cast<const float4 *>(qtiled)[(int64_t)(src >> 4) * per_tile + (r - l) + (l & 48) + (src & 15)];
            }
            qs[i] = v;
        }
        __syncthreads();
        scan_groups_body<QT, MASK>(qs, data, dp4, ngroups, ntotal, gmax + (int64_t)c0 * mstride, mstride, rm...);
    }
}

// ---------------------------------------------------------------------------------------------
// bf16 candidate scan (half the index bytes per pass): group maxima of  <bf16(row), q_hi + q_lo>  on v_mfma_f32_16x16x32_bf16.
// The result only RANKS groups; every reported score comes from the exact float32 re-score.  Exactness is kept by a check:
// with e = |approx - exact| <= (2^-8 + 2^-15 + dp 2^-23) |row| |q|  (bf16 rounding of the row, the dropped q remainder, f32
// accumulation), all rows of a group excluded after the kp best approximate maxima score <= (kp+1)-th approximate maximum + e.
// If that is strictly below the k-th exact score found among the kp re-scored groups, no excluded row can enter or tie the
// top k.  Queries that fail the check are redone by the exact float32 scan (same launch sequence, predicated on device).
// ---------------------------------------------------------------------------------------------
template <int QT, bool MASK, typename... M>
__global__ __launch_bounds__(512) void scan16_groupmax_kernel(const uint4 *__restrict__ data16, const uint4 *__restrict__ qhi,
                                                              const uint4 *__restrict__ qlo, int pieces, int64_t ngroups,
                                                              int64_t ntotal, float *__restrict__ gmax, int64_t mstride, M... rm) {
    typedef __bf16 bf16x8_t __attribute__((ext_vector_type(8)));
    extern __shared__ __attribute__((aligned(16))) uint4 qs16[];      // [QT][2][pieces][64]
    const int per_q = pieces * 64;
    for (int i = threadIdx.x; i < QT * per_q; i += blockDim.x) {
        const int q = i / per_q, r = i - q * per_q;
        qs16[(q * 2) * per_q + r] = qhi[i];
        qs16[(q * 2 + 1) * per_q + r] = qlo[i];
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
    for (int64_t g = (int64_t)blockIdx.x * nw + wave; g < ngroups; g += (int64_t)gridDim.x * nw) {
        f32x4 acc[QT][4];
#pragma unroll
        for (int q = 0; q < QT; ++q)
#pragma unroll
            for (int t = 0; t < 4; ++t) acc[q][t] = f32x4{0.f, 0.f, 0.f, 0.f};
        const uint4 *a = data16 + g * 4 * (int64_t)per_q + lane;
        uint32_t mbyte = 0;
        if constexpr (MASK) mbyte = row_mask_fetch(rm..., g * kGroupRows);
        // K outermost: a query fragment pair (hi, lo) is read from LDS once and used for the four row tiles (one LDS read per
        // four MFMAs; tile-outermost it is one per MFMA, which saturates the LDS port from two query tiles on)
        int kb = 0;
        for (; kb + 2 <= pieces; kb += 2) {
            uint4 av[2][4];
#pragma unroll
            for (int u = 0; u < 2; ++u)
#pragma unroll
                for (int t = 0; t < 4; ++t) av[u][t] = a[(t * pieces + kb + u) * 64];
#pragma unroll
            for (int u = 0; u < 2; ++u)
#pragma unroll
                for (int q = 0; q < QT; ++q) {
                    const uint4 bh = qs16[(q * 2) * per_q + (kb + u) * 64 + lane], bl = qs16[(q * 2 + 1) * per_q + (kb + u) * 64 + lane];
#pragma unroll
                    for (int t = 0; t < 4; ++t) {
                        acc[q][t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, av[u][t]), __builtin_bit_cast(bf16x8_t, bh), acc[q][t], 0, 0, 0);
                        acc[q][t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, av[u][t]), __builtin_bit_cast(bf16x8_t, bl), acc[q][t], 0, 0, 0);
                    }
                }
        }
        for (; kb < pieces; ++kb) {
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const uint4 av = a[(t * pieces + kb) * 64];
#pragma unroll
                for (int q = 0; q < QT; ++q) {
                    const uint4 bh = qs16[(q * 2) * per_q + kb * 64 + lane], bl = qs16[(q * 2 + 1) * per_q + kb * 64 + lane];
                    acc[q][t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, av), __builtin_bit_cast(bf16x8_t, bh), acc[q][t], 0, 0, 0);
                    acc[q][t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, av), __builtin_bit_cast(bf16x8_t, bl), acc[q][t], 0, 0, 0);
                }
            }
        }
        const bool partial = (g + 1) * kGroupRows > ntotal;   // wave-uniform: only the last group
        uint64_t mw = 0;
        if constexpr (MASK) mw = row_mask_word(rm..., g * kGroupRows, mbyte) >> ((lane >> 4) * 4);
#pragma unroll
        for (int q = 0; q < QT; ++q) {
            float m = MASK ? -INFINITY : -FLT_MAX;
#pragma unroll
            for (int t = 0; t < 4; ++t)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    float s = acc[q][t][r];
                    if constexpr (MASK) s = row_mask_score(mw, t * 16 + r, s);
                    else if (partial && g * kGroupRows + t * 16 + (lane >> 4) * 4 + r >= ntotal) s = -FLT_MAX;
                    m = fmaxf(m, s);
                }
            m = fmaxf(m, __shfl_xor(m, 16, 64));
            m = fmaxf(m, __shfl_xor(m, 32, 64));
            if (lane < 16) gmax[(int64_t)(q * 16 + lane) * mstride + g] = m;
        }
    }
}

// The same candidate pass for at most 16 queries (QT = 1: the 10-query search of BASELINE configs[1] and of the streaming step), with
// the index streamed through an LDS-DMA ring instead of through registers.  The register version keeps 8 KiB per wave in flight and
// runs at 5.0 TB/s; HBM wants several times that outstanding.  Here every wave owns a ring of PIECES slots of 1 KiB (= one 16-row tile
// of the bf16 copy): piece kb of the next tile is requested (buffer_load ... lds, no registers, no address arithmetic per lane) as soon
// as piece kb of the current tile has been consumed, so a whole tile per wave = PIECES KiB x 8 waves per workgroup stays in flight.
// The query fragments (hi + lo) live in registers (2 x PIECES x 4 VGPRs), the LDS holds nothing but the rings; a wave reads only what
// it requested itself, so its own counted vmcnt orders every read (no workgroup barrier anywhere in the loop).  MFMA sequence per
// accumulator = scan16_groupmax_kernel<1>'s (hi then lo, ascending K), so the group maxima are bit-identical to it.
// MASK: the bitmap bytes of a group are loaded where the group's tile 0 is requested (right behind its piece 0), one load per lane.
// The counted waits stay as they are: that load is one more in flight among the ring's, and loads retire in order, so a wait can
// only become longer (by one piece, until the load has landed), never release a slot early.
template <int PIECES, bool MASK, typename... M>
__global__ __launch_bounds__(512) void scan16_ring_kernel(const uint4 *__restrict__ data16, const uint4 *__restrict__ qhi,
                                                          const uint4 *__restrict__ qlo, int64_t ngroups, int64_t ntotal,
                                                          float *__restrict__ gmax, int64_t mstride, M... rm) {
    typedef __bf16 bf16x8_t __attribute__((ext_vector_type(8)));
    typedef uint32_t u32x4_t __attribute__((ext_vector_type(4)));
    extern __shared__ __attribute__((aligned(16))) unsigned char ring_all[];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int nw = blockDim.x >> 6;
    unsigned char *ring = ring_all + wave * PIECES * 1024;
    const unsigned ring_lds = (unsigned)(size_t)ring + lane * 16;
    u32x4_t bh[PIECES], bl[PIECES];
#pragma unroll
    for (int kb = 0; kb < PIECES; ++kb) {
        const uint4 h = qhi[kb * 64 + lane], l = qlo[kb * 64 + lane];
        bh[kb] = u32x4_t{h.x, h.y, h.z, h.w};
        bl[kb] = u32x4_t{l.x, l.y, l.z, l.w};
    }
    const int64_t g0 = (int64_t)blockIdx.x * nw + wave, gstep = (int64_t)gridDim.x * nw;
    if (g0 >= ngroups) return;
    constexpr unsigned kGroupBytes = 4u * PIECES * 1024u;
    const unsigned voff = (unsigned)lane * 16u;
    // one buffer descriptor per 64-row group (64-bit base, 32-bit offsets inside the group); no lambda here: a lambda returning the
    // descriptor type inside a kernel TEMPLATE makes hipcc drop the host-side instantiation silently (undefined kernel stub at load)
#define IVR_GROUP_RSRC(G)                                                                                                      \
    __builtin_amdgcn_make_buffer_rsrc(const_cast<char *>(reinterpret_cast<const char *>(data16)) + (G) * (int64_t)kGroupBytes, 0, \
                                      (int)kGroupBytes, 0x00020000)
    // prologue: tile 0 of the first group
    uint32_t mbyte = 0, mbyte_next = 0;
    {
        const auto rs0 = IVR_GROUP_RSRC(g0);
#pragma unroll
        for (int kb = 0; kb < PIECES; ++kb) {
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rs0, (__attribute__((address_space(3))) void *)(ring + kb * 1024), 16, voff, (unsigned)kb * 1024u, 0,
                                                     0);
            if constexpr (MASK)
                if (kb == 0) mbyte = row_mask_fetch(rm..., g0 * kGroupRows);
        }
    }
    for (int64_t g = g0; g < ngroups; g += gstep) {
        const bool more = g + gstep < ngroups;
        const auto rs = IVR_GROUP_RSRC(g);
        const auto rs_next = IVR_GROUP_RSRC(more ? g + gstep : g);
        f32x4 acc[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int kb = 0; kb < PIECES; ++kb) {
                // the oldest request in flight is this slot's.  In the steady state PIECES are outstanding (slots kb .. of this tile, slots
                // .. kb-1 of the next), so all but the PIECES - 1 youngest must have landed; in the wave's very last tile nothing is
                // requested any more and the count falls: that tile is waited for as a whole.  (The one gmax store per group counts in
                // vmcnt too; it can only lengthen these waits: loads retire in order among themselves.)
                if (t == 3 && !more) {
                    if (kb == 0) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // the whole last tile, once
                } else {
                    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(PIECES - 1) : "memory");
                }
                u32x4_t a;
                asm volatile("ds_read_b128 %0, %1\n\ts_waitcnt lgkmcnt(0)" : "=&v"(a) : "v"(ring_lds + (unsigned)kb * 1024u) : "memory");
                // the slot is free again: request the same piece of the next tile (of this group, or of the wave's next group)
                if (t < 3)
                    __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (__attribute__((address_space(3))) void *)(ring + kb * 1024), 16, voff,
                                                             (unsigned)((t + 1) * PIECES + kb) * 1024u, 0, 0);
                else if (more) {
                    __builtin_amdgcn_raw_ptr_buffer_load_lds(rs_next, (__attribute__((address_space(3))) void *)(ring + kb * 1024), 16, voff,
                                                             (unsigned)kb * 1024u, 0, 0);
                    if constexpr (MASK)
                        if (kb == 0) mbyte_next = row_mask_fetch(rm..., (g + gstep) * kGroupRows);
                }
                acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, a), __builtin_bit_cast(bf16x8_t, bh[kb]), acc[t], 0, 0, 0);
                acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, a), __builtin_bit_cast(bf16x8_t, bl[kb]), acc[t], 0, 0, 0);
            }
        }
        const bool partial = (g + 1) * kGroupRows > ntotal;   // wave-uniform: only the last group
        uint64_t mw = 0;
        if constexpr (MASK) {
            mw = row_mask_word(rm..., g * kGroupRows, mbyte) >> ((lane >> 4) * 4);
            mbyte = mbyte_next;
        }
        float m = MASK ? -INFINITY : -FLT_MAX;
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                float sc = acc[t][r];
                if constexpr (MASK) sc = row_mask_score(mw, t * 16 + r, sc);
                else if (partial && g * kGroupRows + t * 16 + (lane >> 4) * 4 + r >= ntotal) sc = -FLT_MAX;
                m = fmaxf(m, sc);
            }
        m = fmaxf(m, __shfl_xor(m, 16, 64));
        m = fmaxf(m, __shfl_xor(m, 32, 64));
        if (lane < 16) gmax[(int64_t)lane * mstride + g] = m;
    }
#undef IVR_GROUP_RSRC
}

// pass 3: one wave per (query, selected group, 16-row tile).  cand[q][j*64 + row] = key(score, row id).
// A tile's accumulator sees exactly the MFMA sequence it sees in score_group (ascending K, x y z w per chunk), so the scores are
// bit-identical to pass 1; splitting the group over four waves and keeping 16 KiB of the tile in flight per wave is what makes
// this pass short: it is a latency chain of k x 64 rows per query, not a bandwidth problem.
// TILES: the selection holds 16-row tiles instead of 64-row groups (large-batch scan): one wave per (query, selected tile),
// cand[q][j*16 + row].  qmap (list-driven exact pass): query q of this launch is the list's q-th entry, qmap[q] in the tiled
// query buffer; waves past *qcount exit.
// Pruning of the large-batch re-score (TILES only): the selection is sorted by approximate tile maximum, so with t_k = the k-th
// selected tile's approximate maximum there are k tiles that each hold a row with exact score >= t_k - e; a tile whose approximate
// maximum is below t_k - 2e holds only rows with exact score < t_k - e and cannot reach the top k.  Such tiles are not fetched
// (their candidate slots are written as absent); e is the verification's bound, from the same measured residuals.
struct PruneArgs {
    const float *tmax = nullptr;          // non-NULL enables pruning
    int64_t tstride = 0;
    int k = 0;
    const float *qnorm = nullptr, *qdelta = nullptr;
    const unsigned int *maxnorm_bits = nullptr, *maxdelta_bits = nullptr;
    float acc_eps = 0.f;
};

// MASK: rows that are not allowed get key 0 (absent), like rows past ntotal
template <bool TILES, bool MASK, typename... M>
__global__ __launch_bounds__(256) void rescore_groups_kernel(const float *__restrict__ data,
                                                             const float *__restrict__ qtiled, int dp4,
                                                             int64_t ntotal, const uint32_t *__restrict__ sel,
                                                             int sel_stride, int ksel, int nq, uint64_t *__restrict__ cand,
                                                             const int *__restrict__ skip, ListArgs la, PruneArgs pr, M... rm) {
    constexpr int kRows = TILES ? 16 : kGroupRows, kSplit = TILES ? 1 : 4;
    const int lane = threadIdx.x & 63;
    const int64_t w = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (w >= (int64_t)nq * ksel * kSplit) return;
    const int t = TILES ? 0 : (int)(w & 3);
    const int64_t qj = TILES ? w : w >> 2;
    const int q = (int)(qj / ksel), j = (int)(qj % ksel);
    if (skip && skip[q]) return;
    if (la.count && q >= *la.count) return;
    const int qs = la.list ? la.list[q] : q;       // row of the tiled query buffer
    const uint32_t g = sel[(int64_t)q * sel_stride + j];
    uint64_t *out = cand + ((int64_t)q * ksel + j) * kRows + t * 16;
    if (g == 0xFFFFFFFFu) {   // fewer groups than k
        if (lane < 16) out[lane] = 0;
        return;
    }
    if (TILES && pr.tmax && j >= pr.k) {          // the first k tiles are always re-scored
        const uint32_t gk = sel[(int64_t)q * sel_stride + pr.k - 1];
        if (gk != 0xFFFFFFFFu) {
            const float rmax = __uint_as_float(*pr.maxnorm_bits), qn = pr.qnorm[q], qd = pr.qdelta[q];
            const float e = 1.01f * ((qn + qd) * __uint_as_float(*pr.maxdelta_bits) + qd * rmax + pr.acc_eps * qn * rmax);
            // NaN / inf bounds compare false: nothing is pruned then
            if (pr.tmax[(int64_t)q * pr.tstride + g] < pr.tmax[(int64_t)q * pr.tstride + gk] - 2.f * e) {
                if (lane < 16) out[lane] = 0;
                return;
            }
        }
    }
    const int per_tile = dp4 * 16, kchunks = dp4 >> 2;
    const float4 *b = reinterpret_cast<const float4 *>(qtiled) + (int64_t)(qs >> 4) * per_tile + lane;
    const float4 *a = reinterpret_cast<const float4 *>(data) + ((int64_t)g * kSplit + t) * per_tile + lane;
    uint32_t mbyte = 0;
    if constexpr (MASK) mbyte = row_mask_fetch(rm..., (int64_t)g * kRows + t * 16);
    const f32x4 acc = pair_score(a, b, kchunks);
    uint64_t mw = 0;
    if constexpr (MASK) mw = row_mask_word(rm..., (int64_t)g * kRows + t * 16, mbyte);
    if ((lane & 15) == (qs & 15)) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int rl = (lane >> 4) * 4 + r;
            const int64_t row = (int64_t)g * kRows + t * 16 + rl;
            uint64_t key = 0;
            if (MASK ? ((mw >> rl) & 1ull) != 0 : row < ntotal) key = ivr_key(acc[r], (uint32_t)row);
            out[rl] = key;
        }
    }
}

// -------------------------------------------------------------------------------------------------
// host side
// -------------------------------------------------------------------------------------------------

constexpr int kScanThreads = 512;    // the streamed scans run workgroups of 8 waves

// Grid of a streamed scan: per_cu workgroups on every CU whose waves stride over the 64-row groups, never more than the groups need
unsigned scan_grid(const ivr_index *x, int64_t ngroups, int per_cu) {
    return (unsigned)std::max<int64_t>(1, std::min<int64_t>(ivr_ceil_div(ngroups, kScanThreads / 64), (int64_t)x->ctx->cu_count * per_cu));
}
// the scans that stage their query tiles in LDS: as many workgroups per CU as the LDS allows, at most 4
int scan_per_cu(size_t lds) { return (int)std::max<size_t>(1, std::min<size_t>(4, (160 * 1024) / std::max<size_t>(lds, 1))); }

template <int QT>
void launch_scan(ivr_index *x, const View &v, const float *qt, hipStream_t s, const int *tile_flag) {
    const size_t lds = (size_t)QT * 16 * x->dp * 4;
    with_mask(v.mask, [&](auto masked, auto... m) {
        auto *k = scan_groupmax_kernel<QT, decltype(masked)::value, decltype(m)...>;
        (void)hipFuncSetAttribute(reinterpret_cast<const void *>(k), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        // algorithmic bytes: every stored row once + the query tile + one maximum per (group, query)
        IvrProf prof("scan_groupmax", s, (double)v.ntotal * x->dp * 4 + (double)QT * 16 * x->dp * 4 + (double)v.ngroups * QT * 16 * 4,
                     tile_flag != nullptr);      // behind the bf16 candidate scan it is the predicated fallback and normally exits at once
        hipLaunchKernelGGL(k, dim3(scan_grid(x, v.ngroups, scan_per_cu(lds))), dim3(kScanThreads), lds, s, v.data, qt, x->dp4, v.ngroups,
                           v.ntotal, x->gmax, x->mstride(), tile_flag, m...);
    });
}

template <int QT>
void launch_scan16(ivr_index *x, const View &v, int64_t tile0, hipStream_t s) {
    const size_t lds = (size_t)QT * 2 * x->pieces * 1024;
    with_mask(v.mask, [&](auto masked, auto... m) {
        auto *k = scan16_groupmax_kernel<QT, decltype(masked)::value, decltype(m)...>;
        (void)hipFuncSetAttribute(reinterpret_cast<const void *>(k), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        // algorithmic bytes: the bf16 copy of every stored row once + the split query tiles + one maximum per (group, query)
        IvrProf prof("scan16_groupmax", s,
                     (double)v.ntotal * x->pieces * 64 + (double)QT * 2 * x->pieces * 1024 + (double)v.ngroups * QT * 16 * 4);
        hipLaunchKernelGGL(k, dim3(scan_grid(x, v.ngroups, scan_per_cu(lds))), dim3(kScanThreads), lds, s, v.data16,
                           x->q16hi + tile0 * x->pieces * 64, x->q16lo + tile0 * x->pieces * 64, x->pieces, v.ngroups, v.ntotal, x->gmax,
                           x->mstride(), m...);
    });
}

// at most 16 queries and a piece count the ring kernel is built for: stream the index through the LDS-DMA rings
template <int PIECES>
void launch_scan16_ring(ivr_index *x, const View &v, int64_t tile0, hipStream_t s) {
    const size_t lds = (size_t)(kScanThreads / 64) * PIECES * 1024;
    with_mask(v.mask, [&](auto masked, auto... m) {
        auto *k = scan16_ring_kernel<PIECES, decltype(masked)::value, decltype(m)...>;
        (void)ivr_func_max_lds(reinterpret_cast<const void *>(k), (int)lds);
        IvrProf prof("scan16_groupmax", s, (double)v.ntotal * x->pieces * 64 + (double)2 * x->pieces * 1024 + (double)v.ngroups * 16 * 4);
        // one workgroup per CU (its 8 rings already keep PIECES x 8 KiB in flight), two when the rings are small; groups are dealt
        // round-robin to the waves of the grid
        hipLaunchKernelGGL(k, dim3(scan_grid(x, v.ngroups, lds <= 64 * 1024 ? 2 : 1)), dim3(kScanThreads), lds, s, v.data16,
                           x->q16hi + tile0 * x->pieces * 64, x->q16lo + tile0 * x->pieces * 64, v.ngroups, v.ntotal, x->gmax, x->mstride(),
                           m...);
    });
}

template <int QT>
void launch_scan_list(ivr_index *x, const View &v, const float *qt, float *gmax, const ListArgs &la, hipStream_t s) {
    const size_t lds = (size_t)QT * 16 * x->dp * 4;
    with_mask(v.mask, [&](auto masked, auto... m) {
        auto *k = scan_groupmax_list_kernel<QT, decltype(masked)::value, decltype(m)...>;
        (void)hipFuncSetAttribute(reinterpret_cast<const void *>(k), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        IvrProf prof("scan_groupmax_list", s, 0.0, true);      // normally nothing is listed and every workgroup exits at once
        hipLaunchKernelGGL(k, dim3(scan_grid(x, v.ngroups, scan_per_cu(lds))), dim3(kScanThreads), lds, s, v.data, qt, x->dp4, v.ngroups,
                           v.ntotal, gmax, x->mstride(), la.count, la.list, m...);
    });
}

// pass 3 of the top-k search: the plain or the masked re-score
template <bool TILES>
void launch_rescore(const View &v, unsigned blocks, hipStream_t s, const float *qtiled, int dp4, const uint32_t *sel, int sel_stride, int ksel,
                    int nq, uint64_t *cand, const int *skip, const ListArgs &la, const PruneArgs &pr = PruneArgs()) {
    with_mask(v.mask, [&](auto masked, auto... m) {
        hipLaunchKernelGGL((rescore_groups_kernel<TILES, decltype(masked)::value, decltype(m)...>), dim3(blocks), dim3(256), 0, s, v.data, qtiled,
                           dp4, v.ntotal, sel, sel_stride, ksel, nq, cand, skip, la, pr, m...);
    });
}

// What the final selection of a chunk (queries from q0 on) verifies the bf16 candidate scan with, and with pr what the large-batch
// re-score prunes with.  The 64-query chunks check group maxima with the relative bound and flag query tiles; the large-batch scan
// (big) checks tile maxima with the measured rounding residuals and lists the queries that fail.
VerifyArgs verify_args(const ivr_index *x, int q0, int k, bool big, PruneArgs *pr = nullptr) {
    VerifyArgs vf;
    vf.sel = x->sel;
    vf.kp = ivr_index::fast_groups(k);
    vf.ksel2 = vf.kp + 1;
    vf.qnorm = x->qnorm + q0;
    vf.maxnorm_bits = x->maxnorm;
    if (!big) {
        vf.gmax = x->gmax;
        vf.mstride = x->mstride();
        vf.rel_eps = x->rel_eps();
        vf.ok = x->okflag;
        vf.tile_flag = x->okflag + 64;
        return vf;
    }
    vf.gmax = x->tmax;
    vf.mstride = x->tstride();
    vf.ok = x->okq;
    vf.qdelta = x->qdelta + q0;
    vf.maxdelta_bits = x->maxdelta;
    vf.acc_eps = x->acc_eps();
    vf.fail_count = x->okq + kBigChunk;
    vf.fail_list = x->okq + kBigChunk + 4;
    if (pr && x->prune) {
        pr->tmax = vf.gmax;
        pr->tstride = vf.mstride;
        pr->k = k;
        pr->qnorm = vf.qnorm;
        pr->qdelta = vf.qdelta;
        pr->maxnorm_bits = vf.maxnorm_bits;
        pr->maxdelta_bits = vf.maxdelta_bits;
        pr->acc_eps = vf.acc_eps;
    }
    return vf;
}

// ivr_index_search_reconstruct: where the final selections of a search leave the row behind every result slot, as its number in the
// scanned view (pos: DEV [nq][k], NULL for every other search)
struct RowPos {
    int64_t *pos = nullptr;
    void set(SelectOut &o, int q0, int k) const {
        if (pos) o.pos = pos + (int64_t)q0 * k;
    }
};

// Passes 2 to 4 of the exact search for one chunk whose float32 group maxima are in gmax: for the queries without skip[q] (the
// 64-query chunks), or for the listed ones (la: behind the large-batch scan, where the amount of work is known on the device only).
// qtile = the chunk's first query tile: the re-score reads query tile (q >> 4) relative to it.
int exact_tail(ivr_index *x, const View &v, const float *gmax, const float *qtile, int q0, int nqc, int k, const int *skip,
               const ListArgs &la, float *D, int64_t *I, const RowPos &rp, hipStream_t s) {
    const bool counted = la.count == nullptr;
    const int64_t waves = (int64_t)nqc * k;
    {
        IvrProf prof("select_groups", s, counted ? (double)nqc * v.ngroups * 4 : 0.0, true);
        SelectOut o = SelectOut::to_groups(x->sel);
        o.skip = skip;
        o.la = la;
        launch_select<OUT_GROUPS>(SrcGroupMax{gmax, x->mstride(), v.ngroups}, nqc, k, o, s);
        IVR_LAUNCH_CHECK();
    }
    {
        IvrProf prof("rescore_groups", s, counted ? (double)waves * kGroupRows * x->dp * 4 : 0.0, true);
        launch_rescore<false>(v, (unsigned)waves, s, qtile, x->dp4, x->sel, k, k, nqc, x->cand, skip, la);
        IVR_LAUNCH_CHECK();
    }
    IvrProf prof("select_final", s, counted ? (double)waves * kGroupRows * 8 : 0.0, true);
    SelectOut o = SelectOut::to_rows(D + (int64_t)q0 * k, I + (int64_t)q0 * k, v.id_base, v.ids);
    o.skip = skip;
    o.la = la;
    rp.set(o, q0, k);
    launch_select_rows(SrcKeys{x->cand, (int64_t)k * kGroupRows}, nqc, k, o, s);
    IVR_LAUNCH_CHECK();
    return IVR_OK;
}

// One chunk (<= kBigChunk queries, already tiled at tile q0 / 16) of a large batch:
//   scanq (index read once) -> top kp+1 blocks of 128 rows per query -> top kp+1 tiles of 16 rows among those blocks' tiles (the kp+1
//   best tiles always lie inside the kp+1 best blocks: the argument of DESIGN.md section 4 with tiles for rows) -> exact float32
//   re-score of kp tiles -> final selection, which also verifies the approximate ranking per query and lists the queries that
//   fail -> list-driven exact pass (four launches that exit at once when the list is empty; no host round trip).
int search_big(ivr_index *x, const View &v, int q0, int nqc, int k, float *D, int64_t *I, const RowPos &rp, hipStream_t s) {
    const int kp = ivr_index::fast_groups(k), ksel2 = kp + 1;
    const int64_t tstride = x->tstride(), bstride = x->bstride();
    const int64_t nblk128 = ivr_ceil_div(v.ntotal, 128), ntiles = ivr_ceil_div(v.ntotal, 16);
    const float *qtile = x->qtiled + (int64_t)(q0 / 16) * 16 * x->dp;
    PruneArgs pr;
    const VerifyArgs vf = verify_args(x, q0, k, true, &pr);
    const ScanQArgs a{v.data16, x->q16hi + (int64_t)(q0 / 16) * x->pieces * 64, x->pieces, (int)ivr_round_up(nqc, 256) / 256, v.ntotal,
                      ivr_ceil_div(v.ntotal, 256), x->tmax, tstride, x->bmax, bstride};
    int rc = ivr_launch_scanq(x->ctx, a, s, v.mask);
    if (rc != IVR_OK) return rc;
    {
        IvrProf prof("select_blocks", s, (double)nqc * nblk128 * 4, true);
        SelectOut o = SelectOut::to_groups(x->selb);
        o.reset_flags = vf.fail_count;
        launch_select<OUT_GROUPS>(SrcGroupMax{x->bmax, bstride, nblk128}, nqc, ksel2, o, s);
        IVR_LAUNCH_CHECK();
    }
    {
        IvrProf prof("select_tiles", s, (double)nqc * ksel2 * 8 * 4, true);
        launch_select<OUT_GROUPS>(SrcTilesOf{x->tmax, tstride, x->selb, ksel2, ntiles, (int64_t)ksel2 * 8}, nqc, ksel2,
                                  SelectOut::to_groups(x->sel), s);
        IVR_LAUNCH_CHECK();
    }
    {
        const int64_t waves = (int64_t)nqc * kp;
        IvrProf prof("rescore_tiles", s, (double)waves * 16 * x->dp * 4, true);
        launch_rescore<true>(v, (unsigned)ivr_ceil_div(waves, 4), s, qtile, x->dp4, x->sel, ksel2, kp, nqc, x->cand, nullptr, ListArgs(), pr);
        IVR_LAUNCH_CHECK();
    }
    {
        IvrProf prof("select_final", s, (double)nqc * kp * 16 * 8, true);
        SelectOut o = SelectOut::to_rows(D + (int64_t)q0 * k, I + (int64_t)q0 * k, v.id_base, v.ids);
        o.vf = vf;
        rp.set(o, q0, k);
        launch_select_rows(SrcKeys{x->cand, (int64_t)kp * 16}, nqc, k, o, s);
        IVR_LAUNCH_CHECK();
    }
    // exact pass over the listed queries; its group maxima reuse the tile-maxima buffer (read for the last time just above)
    const ListArgs la{vf.fail_count, vf.fail_list};
    switch (x->qt_max()) {
        case 1: launch_scan_list<1>(x, v, qtile, x->tmax, la, s); break;
        case 2: launch_scan_list<2>(x, v, qtile, x->tmax, la, s); break;
        case 3: launch_scan_list<3>(x, v, qtile, x->tmax, la, s); break;
        default: launch_scan_list<4>(x, v, qtile, x->tmax, la, s); break;
    }
    IVR_LAUNCH_CHECK();
    return exact_tail(x, v, x->tmax, qtile, q0, nqc, k, nullptr, la, D, I, rp, s);
}

int reserve_search(ivr_index *x, int nq, int k) {
    const bool big = x->use_big(nq, k);
    // the large-batch scan reads whole blocks of 256 queries: the tiled query buffers are padded (zero rows) to that
    int rc = ivr_reserve_queries(x, (int)ivr_ceil_div(big ? ivr_round_up(nq, 256) : nq, 16));
    if (rc == IVR_OK) rc = ivr_reserve_gmax(x);
    const size_t chunk_q = std::min(nq, big ? kBigChunk : 64), ksel2 = ivr_index::fast_groups(k) + 1;
    const size_t need_sel = chunk_q * (x->scan16 ? ksel2 : k);   // per scan chunk
    if (rc == IVR_OK) rc = ivr_reserve({{&x->sel, need_sel * 4}, {&x->cand, need_sel * kGroupRows * 8}});
    if (rc == IVR_OK) rc = ivr_reserve({{&x->rpos, (size_t)nq * k * sizeof(int64_t)}});     // ivr_index_search_reconstruct
    if (rc != IVR_OK || !big) return rc;
    const size_t qpad = ivr_round_up(chunk_q, 256);
    rc = ivr_reserve({{&x->tmax, qpad * x->tstride() * 4}});
    if (rc == IVR_OK) rc = ivr_reserve({{&x->bmax, qpad * x->bstride() * 4}});
    if (rc == IVR_OK) rc = ivr_reserve({{&x->selb, chunk_q * ksel2 * 4}});
    if (rc == IVR_OK) rc = ivr_reserve({{&x->okq, (2 * kBigChunk + 4) * sizeof(int)}}, true);
    return rc;
}

// ivr_index_search over the rows of view v (the whole index, or the part a filter allows); the caller holds x->mu
// want_pos: the row of the view behind every result slot goes to x->rpos
int search_view(ivr_index *x, const View &v, const float *q, int nq, int k, int normalize_q, float *D, int64_t *I, bool want_pos,
                hipStream_t s) {
    int rc = reserve_search(x, nq, k);
    if (rc != IVR_OK) return rc;
    const RowPos rp{want_pos ? (int64_t *)x->rpos : nullptr};
    // queries -> tiled layout (normalised on the way when asked: N2 on the query side, core.py:875)
    rc = ivr_launch_tile_rows(x, x->qtiled, q, 0, nq, normalize_q, nullptr, s);
    if (rc != IVR_OK) return rc;
    // The bf16 candidate scan goes first when it can pay.  Its result is verified per query on the device; failures are redone by
    // the exact pass (tile flags / skip, or the failure list of the large-batch scan).
    const bool fast = x->fast_scan(v.ngroups, k);
    x->last_big = false;
    if (fast && x->use_big(nq, k)) {
        // large batch: the index is read once per kBigChunk queries instead of once per 64
        for (int q0 = 0; q0 < nq; q0 += kBigChunk) {
            const int nqc = std::min(kBigChunk, nq - q0);
            rc = search_big(x, v, q0, nqc, k, D, I, rp, s);
            if (rc != IVR_OK) return rc;
            x->last_nqc = nqc;
        }
        x->last_big = true;
        return IVR_OK;
    }
    const int chunk = 16 * x->qt_max(), kp = ivr_index::fast_groups(k), ksel2 = kp + 1;
    for (int q0 = 0; q0 < nq; q0 += chunk) {
        const int nqc = std::min(chunk, nq - q0);
        const int qt = pick_qt(nqc);
        const float *qtile = x->qtiled + (int64_t)(q0 / 16) * 16 * x->dp;
        const int *tile_flag = nullptr, *skip = nullptr;
        x->last_nqc = fast ? nqc : 0;
        if (fast) {
            const VerifyArgs vf = verify_args(x, q0, k, false);
            ivr_launch_fast_scan(x, v, qt, q0 / 16, s);
            IVR_LAUNCH_CHECK();
            {
                IvrProf prof("select_groups", s, (double)nqc * v.ngroups * 4, true);
                SelectOut o = SelectOut::to_groups(x->sel);
                o.reset_flags = vf.tile_flag;
                launch_select<OUT_GROUPS>(SrcGroupMax{x->gmax, x->mstride(), v.ngroups}, nqc, ksel2, o, s);
                IVR_LAUNCH_CHECK();
            }
            const int64_t waves = (int64_t)nqc * kp;
            {
                IvrProf prof("rescore_groups", s, (double)waves * kGroupRows * x->dp * 4, true);
                launch_rescore<false>(v, (unsigned)waves, s, qtile, x->dp4, x->sel, ksel2, kp, nqc, x->cand, nullptr, ListArgs());
                IVR_LAUNCH_CHECK();
            }
            {
                IvrProf prof("select_final", s, (double)waves * kGroupRows * 8, true);
                SelectOut o = SelectOut::to_rows(D + (int64_t)q0 * k, I + (int64_t)q0 * k, v.id_base, v.ids);
                o.vf = vf;
                rp.set(o, q0, k);
                launch_select_rows(SrcKeys{x->cand, (int64_t)kp * kGroupRows}, nqc, k, o, s);
                IVR_LAUNCH_CHECK();
            }
            // the exact pass below redoes the queries whose check failed: every kernel of it exits at once when nothing is flagged
            tile_flag = vf.tile_flag;
            skip = vf.ok;
        }
        if (v.ngroups > 0) {
            ivr_launch_scan_qt(x, v, qt, qtile, s, tile_flag);
            IVR_LAUNCH_CHECK();
        }
        rc = exact_tail(x, v, x->gmax, qtile, q0, nqc, k, skip, ListArgs(), D, I, rp, s);
        if (rc != IVR_OK) return rc;
    }
    return IVR_OK;
}

}  // namespace

int ivr_search_view_pos(ivr_index *x, const View &v, const float *q, int nq, int k, int normalize_q, float *D, int64_t *I, hipStream_t s) {
    return search_view(x, v, q, nq, k, normalize_q, D, I, true, s);
}

// tiled query buffers (float32, norms, bf16 hi / lo, rounding residuals) for `qtiles` 16-query tiles, zero-filled
int ivr_reserve_queries(ivr_index *x, int qtiles) {
    const size_t want = std::max(qtiles, 4), q16 = x->scan16 ? want * x->pieces * 1024 : 0;
    return ivr_reserve({{&x->qtiled, want * 16 * x->dp * 4}, {&x->qnorm, want * 16 * 4}, {&x->q16hi, q16}, {&x->q16lo, q16},
                        {&x->qdelta, x->scan16 ? want * 16 * 4 : 0}}, true);
}

// group maxima of one scan chunk (up to 64 query columns)
int ivr_reserve_gmax(ivr_index *x) { return ivr_reserve({{&x->gmax, (size_t)64 * x->mstride() * 4}}); }

void ivr_launch_scan_qt(ivr_index *x, const View &v, int qt, const float *qtile, hipStream_t s, const int *tile_flag) {
    switch (qt) {
        case 1: launch_scan<1>(x, v, qtile, s, tile_flag); break;
        case 2: launch_scan<2>(x, v, qtile, s, tile_flag); break;
        case 3: launch_scan<3>(x, v, qtile, s, tile_flag); break;
        default: launch_scan<4>(x, v, qtile, s, tile_flag); break;
    }
}

// the bf16 candidate scan of one chunk of at most 64 queries (16*qt query columns from tile tile0 on): the LDS-DMA ring for at most
// 16 queries when it is built for the piece count, else the register-streamed kernel
void ivr_launch_fast_scan(ivr_index *x, const View &v, int qt, int64_t tile0, hipStream_t s) {
    switch (qt) {
        case 1:
            if (x->ring && x->pieces == 16) launch_scan16_ring<16>(x, v, tile0, s);
            else if (x->ring && x->pieces == 12) launch_scan16_ring<12>(x, v, tile0, s);
            else if (x->ring && x->pieces == 8) launch_scan16_ring<8>(x, v, tile0, s);
            else launch_scan16<1>(x, v, tile0, s);
            break;
        case 2: launch_scan16<2>(x, v, tile0, s); break;
        case 3: launch_scan16<3>(x, v, tile0, s); break;
        default: launch_scan16<4>(x, v, tile0, s); break;
    }
}

extern "C" {

int ivr_index_reserve_search(ivr_index *x, int max_nq, int max_k) {
    IVR_REQUIRE(x, "ivr_index_reserve_search: NULL index");
    IVR_REQUIRE(max_nq >= 1 && max_k >= 1 && max_k <= IVR_MAX_K, "ivr_index_reserve_search: nq=%d k=%d", max_nq, max_k);
    std::lock_guard<std::mutex> lk(x->mu);
    IVR_HIP(hipSetDevice(x->ctx->device));
    return reserve_search(x, max_nq, max_k);
}

int ivr_index_search(ivr_index *x, const float *q, int nq, int k, int normalize_q, int64_t id_base, float *D, int64_t *I,
                     ivr_stream stream) {
    return ivr_index_search_filtered(x, q, nq, k, normalize_q, id_base, nullptr, D, I, stream);
}

int ivr_index_search_filtered(ivr_index *x, const float *q, int nq, int k, int normalize_q, int64_t id_base, const ivr_id_filter *filter,
                              float *D, int64_t *I, ivr_stream stream) {
    IVR_REQUIRE(x && q && D && I, "ivr_index_search: NULL argument");
    IVR_REQUIRE(nq >= 1, "ivr_index_search: nq=%d", nq);
    IVR_REQUIRE(k >= 1 && k <= IVR_MAX_K, "ivr_index_search: k=%d outside [1,%d]", k, IVR_MAX_K);
    return with_view(x, id_base, filter, (hipStream_t)stream, "ivr_index_search_filtered",
                     [&](const View &v) { return search_view(x, v, q, nq, k, normalize_q, D, I, false, (hipStream_t)stream); });
}

int ivr_index_scan_stats(ivr_index *x, int *out) {
    IVR_REQUIRE(x && out, "ivr_index_scan_stats: NULL argument");
    std::lock_guard<std::mutex> lk(x->mu);
    out[0] = x->scan16 ? 1 : 0;
    out[1] = 0;
    if (!x->scan16) return IVR_OK;
    IVR_HIP(hipSetDevice(x->ctx->device));
    IVR_HIP(hipDeviceSynchronize());
    if (x->last_big) {       // large-batch scan: the length of the failure list of the last chunk
        IVR_HIP(hipMemcpy(&out[1], x->okq + kBigChunk, sizeof(int), hipMemcpyDeviceToHost));
        return IVR_OK;
    }
    int ok[64];
    IVR_HIP(hipMemcpy(ok, x->okflag, sizeof(ok), hipMemcpyDeviceToHost));
    for (int i = 0; i < x->last_nqc; ++i) out[1] += ok[i] == 0;
    return IVR_OK;
}

}  // extern "C"
