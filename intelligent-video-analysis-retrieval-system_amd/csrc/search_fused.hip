// Fused search over the flat index (ivr_index_search_fused, ivr_index_range_search_fused): ONE ranking of the stored rows from a SET
// of query vectors per query (expansions of a text, text + example image, "like these but not like that one", "all of these
// concepts").  The member of the seg_off-free epilogue family that folds across the QUERY COLUMNS of the MFMA tile instead of across
// rows.  DESIGN.md section 4, "fused search".
//
// Member score S[j, r] = <member j, stored row r>, accumulated by stream_tile / mfma_chunk4 from a zero accumulator: the accumulation
// order of every float32 score of the index (search_internal.h), taken as ivr_index_search reports it (-0.0 as +0.0).  Per row:
//   T[j]   = w[j] * S[j, r]                                  one float32 product, rounded on its own (no fused multiply-add)
//   P      = fold of T over the positive members             max, min, or the balanced pairwise sum over the slots of the set
//                                                            ((T0 + T1) + (T2 + T3)) + ..., +0.0f for a slot that is no positive member
//   Nn     = max of T over the negative members
//   F      = P without negatives; margin: P - Nn; veto: P when P > Nn, else -(Nn * Nn)
// Rows rank by ivr_key(F, row).
//
// Column layout: the members of fused query f are the rows f * slots .. f * slots + slots - 1 of q, slots a power of two <= 16, so
// they are an aligned group of `slots` consecutive columns of one 16-column query tile and a tile holds 16 / slots fused queries.
// The weight and the role of a column are read from the caller's tables by the column's number.
//
// Launches per chunk of fused queries (whole query tiles), all on the caller's stream:
//   fused_score   the frame of seq_score / grp_segbest: a workgroup takes 64 stored 16-row tiles against one query tile staged in
//                 LDS, one tile per wave at a time.  In a lane acc[r] is row 16 t + 4 (lane >> 4) + r against column lane & 15.  The lane
//                 forms T, feeds the positive and the negative accumulator (the fold's neutral element for any other role), and both
//                 are folded across the columns of the set with log2(slots) cross-lane exchanges (xor 1, 2, 4, 8).  The butterfly
//                 gives every lane of a set the same bits (float addition is commutative, so the sum is the pairwise tree in every
//                 lane).  The first lane of a set forms F and writes the four keys of its rows into the fused query's stretch of the
//                 key scratch with two 16-byte stores; a row at or beyond ntotal gets key 0.  Every slot of a stretch is written
//   tail          top-k: select_topk_kernel (search_select.h), one workgroup per fused query; range: the count / prefix / write passes
//                 of search_range_keys.h, with the running total carried on the device from chunk to chunk
// A stretch is 16 ceil(ntotal / 16) keys, so that the stores are aligned; a chunk holds as many fused queries as fit
// IVR_SEQ_CHUNK_SLOTS key slots, in whole query tiles, one tile at least and 4,096 columns at most.
#include "ivr_common.h"
#include "search_internal.h"
#include "search_lists.h"
#include "search_range_keys.h"
#include "search_select.h"

#include <cmath>
#include <vector>

namespace {

constexpr int kFuTilesPerBlock = 64;     // 16-row tiles per workgroup, as the clip search's score pass
constexpr int kFuMaxChunkTiles = 256;    // query tiles per chunk at most = 4,096 columns: keeps the grid (row blocks * query tiles) below 2^31

typedef unsigned long long fu_u64x2 __attribute__((ext_vector_type(2)));

struct FuScore {
    const float4 *data;          // the float32 tiles of the storage
    const float4 *qtile;         // the first query tile of the chunk in the tiled query buffer
    int dp4;
    int qtiles;                  // query tiles of the chunk
    int64_t ntiles;              // 16-row tiles that hold stored rows
    int64_t ntotal;
    const float *w;              // [ncols] weight of every column of the chunk
    const int8_t *role;          // [ncols] 1 positive, -1 negative, 0 absent
    int ncols;                   // columns of the chunk that belong to a fused query: a multiple of slots
    int slots;                   // columns of a set: 1, 2, 4, 8 or 16
    int combine;
    uint64_t *keys;              // [fused queries of the chunk][sstride]
    int64_t sstride;             // 16 ntiles
};

// Workgroup b: query tile y = b % qtiles of the chunk against the row tiles 64 x .. 64 x + 63, x = b / qtiles, as seq_score_kernel
// walks them.  Every tile read lies inside the storage's allocation (capacity a multiple of 64 rows >= ntotal); a table read has
// col < ncols; a key store goes to set col / slots < ncols / slots at row offset 16 t + 4 (lane >> 4) .. + 3 < 16 ntiles = sstride.  slots
// is the same in every lane and the walk of a wave does not depend on the lane, so every shuffle is reached by whole waves.
template <int FOLD>
__global__ __launch_bounds__(256) void fused_score_kernel(FuScore a) {
    SQ_NO_CONTRACT
    extern __shared__ __attribute__((aligned(16))) float4 qs[];
    const int per_tile = a.dp4 * 16, kchunks = a.dp4 >> 2;
    const int y = (int)(blockIdx.x % a.qtiles);
    const int64_t x = blockIdx.x / a.qtiles;
    const float4 *qt = a.qtile + (int64_t)y * per_tile;
    for (int i = threadIdx.x; i < per_tile; i += blockDim.x) qs[i] = qt[i];
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, h = lane >> 4;
    const int col = y * 16 + (lane & 15);
    const bool present = col < a.ncols;
    const float w = present ? a.w[col] : 0.f;
    const int role = present ? (int)a.role[col] : 0;
    int hasneg = role < 0 ? 1 : 0;
    for (int o = 1; o < a.slots; o <<= 1) hasneg |= __shfl_xor(hasneg, o, 64);
    const bool writer = present && (lane & (a.slots - 1)) == 0;
    uint64_t *out = a.keys + (int64_t)(present ? col / a.slots : 0) * a.sstride + h * 4;
    const float neutral = FOLD == IVR_FUSE_MAX ? -INFINITY : FOLD == IVR_FUSE_MIN ? INFINITY : 0.0f;
    const int64_t t0 = x * kFuTilesPerBlock, t1 = min(t0 + kFuTilesPerBlock, a.ntiles);
    for (int64_t t = t0 + wave; t < t1; t += 4) {
        const float4 *at = a.data + t * per_tile + lane;
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        stream_tile<1>(at, kchunks, [&](int, int kc, const float4 &av) { mfma_chunk4(acc, av, qs[kc * 64 + lane]); });
        // acc[r] = <row 16 t + 4 h + r, column (lane & 15) of the tile>
        float P[4], Nn[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float S = acc[r] + 0.0f;                        // as ivr_index_search reports it: -0.0 as +0.0
            const float T = w * S;
            P[r] = role > 0 ? T : neutral;
            Nn[r] = role < 0 ? T : -INFINITY;
        }
        for (int o = 1; o < a.slots; o <<= 1) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float p = __shfl_xor(P[r], o, 64), n = __shfl_xor(Nn[r], o, 64);
                if constexpr (FOLD == IVR_FUSE_MAX) P[r] = p > P[r] ? p : P[r];
                else if constexpr (FOLD == IVR_FUSE_MIN) P[r] = p < P[r] ? p : P[r];
                else P[r] = P[r] + p;
                Nn[r] = n > Nn[r] ? n : Nn[r];
            }
        }
        if (!writer) continue;
        uint64_t key[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            float F = P[r];
            if (hasneg) {
                if (a.combine == IVR_FUSE_MARGIN) {
                    F = P[r] - Nn[r];
                } else if (!(P[r] > Nn[r])) {
                    const float sq = Nn[r] * Nn[r];
                    F = -sq;
                }
            }
            const int64_t row = t * 16 + h * 4 + r;
            key[r] = row < a.ntotal ? ivr_key(F, (uint32_t)row) : 0ull;
        }
        fu_u64x2 *dst = reinterpret_cast<fu_u64x2 *>(out + t * 16);
        dst[0] = fu_u64x2{key[0], key[1]};
        dst[1] = fu_u64x2{key[2], key[3]};
    }
}

struct SrcFused {      // the keys of fused query q of the chunk: slots [q * n, (q + 1) * n) of the scratch, every one written
    const uint64_t *keys;
    int64_t n;
    __device__ uint64_t key(int q, int64_t i) const { return keys[(int64_t)q * n + i]; }
};

// an empty index: every top-k slot unused, every lims entry 0
__global__ __launch_bounds__(256) void fused_absent_kernel(int64_t nsel, float *__restrict__ D, int64_t *__restrict__ I, int64_t nlims,
                                                           int64_t *__restrict__ lims) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (D && i < nsel) {
        D[i] = -FLT_MAX;
        I[i] = -1;
    }
    if (lims && i < nlims) lims[i] = 0;
}

struct FuArgs {
    const float *q;
    int nq, slots;
    const float *w;
    const int8_t *role;
    int fold, combine, normalize_q;
    // top-k (k > 0): D / I [nq][k]; range (k == 0): lims [nq + 1], D / I [cap]
    int k;
    float threshold;
    int64_t *lims;
    float *D;
    int64_t *I;
    int64_t cap;
};

int fu_check(const char *what, ivr_index *x, const FuArgs &a) {
    IVR_REQUIRE(x && a.q && a.w && a.role && a.D && a.I, "%s: NULL argument", what);
    IVR_REQUIRE(a.nq >= 1, "%s: nq=%d < 1", what, a.nq);
    IVR_REQUIRE(a.slots == 1 || a.slots == 2 || a.slots == 4 || a.slots == 8 || a.slots == 16, "%s: slots=%d is not one of 1, 2, 4, 8, 16", what,
                a.slots);
    IVR_REQUIRE((int64_t)a.nq * a.slots < (1ll << 31), "%s: nq * slots = %lld >= 2^31", what, (long long)a.nq * a.slots);
    IVR_REQUIRE(a.fold == IVR_FUSE_MAX || a.fold == IVR_FUSE_MIN || a.fold == IVR_FUSE_SUM,
                "%s: fold=%d is none of IVR_FUSE_MAX, IVR_FUSE_MIN, IVR_FUSE_SUM", what, a.fold);
    IVR_REQUIRE(a.combine == IVR_FUSE_MARGIN || a.combine == IVR_FUSE_VETO, "%s: combine=%d is neither IVR_FUSE_MARGIN nor IVR_FUSE_VETO", what,
                a.combine);
    return IVR_OK;
}

// The tables of the call, read back once before anything is launched: every role one of 1, -1, 0, every weight finite, every set with
// a positive member.  s has run when this returns
int fu_check_tables(const char *what, const FuArgs &a, hipStream_t s) {
    const size_t n = (size_t)a.nq * a.slots;
    std::vector<float> w(n);
    std::vector<int8_t> role(n);
    IVR_HIP(hipMemcpyAsync(w.data(), a.w, n * sizeof(float), hipMemcpyDeviceToHost, s));
    IVR_HIP(hipMemcpyAsync(role.data(), a.role, n, hipMemcpyDeviceToHost, s));
    IVR_HIP(hipStreamSynchronize(s));
    for (int f = 0; f < a.nq; ++f) {
        bool positive = false;
        for (int j = 0; j < a.slots; ++j) {
            const size_t c = (size_t)f * a.slots + j;
            IVR_REQUIRE(role[c] >= -1 && role[c] <= 1, "%s: role=%d of member %d of set %d is none of 1, -1, 0", what, (int)role[c], j, f);
            IVR_REQUIRE(std::isfinite(w[c]), "%s: weight %g of member %d of set %d is not finite", what, (double)w[c], j, f);
            positive = positive || role[c] > 0;
        }
        IVR_REQUIRE(positive, "%s: set %d has no positive member", what, f);
    }
    return IVR_OK;
}

template <int FOLD>
int fu_launch_score(ivr_index *x, const FuScore &sc, hipStream_t s) {
    const size_t lds = (size_t)16 * x->dp * 4;
    const int rc = ivr_func_max_lds(reinterpret_cast<const void *>(fused_score_kernel<FOLD>), (int)lds);
    if (rc != IVR_OK) return rc;
    IvrProf prof("fused_score", s, (double)sc.qtiles * 16 * x->ntotal * 2.0 * x->dp);
    hipLaunchKernelGGL(fused_score_kernel<FOLD>, dim3((unsigned)(ivr_ceil_div(sc.ntiles, kFuTilesPerBlock) * sc.qtiles)), dim3(256), lds, s, sc);
    IVR_LAUNCH_CHECK();
    return IVR_OK;
}

// both entry points once their arguments are checked; the caller holds x->mu
int fu_search(const char *what, ivr_index *x, const FuArgs &a, hipStream_t s) {
    IVR_REQUIRE(x->ntotal < (1ll << 31), "%s: ntotal=%lld >= 2^31", what, (long long)x->ntotal);
    int rc = fu_check_tables(what, a, s);
    if (rc != IVR_OK) return rc;
    if (x->ntotal == 0) {
        const int64_t nsel = a.k ? (int64_t)a.nq * a.k : 0, nlims = a.k ? 0 : a.nq + 1;
        hipLaunchKernelGGL(fused_absent_kernel, dim3((unsigned)ivr_ceil_div(std::max(nsel, nlims), 256)), dim3(256), 0, s, nsel, a.k ? a.D : nullptr,
                           a.I, nlims, a.k ? nullptr : a.lims);
        IVR_LAUNCH_CHECK();
        return IVR_OK;
    }
    const int64_t ntiles = ivr_ceil_div(x->ntotal, 16), sstride = ntiles * 16;
    const int per_tile = 16 / a.slots;                                    // fused queries of one query tile
    const int64_t ncols = (int64_t)a.nq * a.slots;
    // query tiles per chunk: the stretches within the slot budget, one tile at least
    const int64_t ct = std::max<int64_t>(1, std::min<int64_t>({ivr_ceil_div(a.nq, per_tile), x->seq_chunk_slots / sstride / per_tile,
                                                               (int64_t)kFuMaxChunkTiles}));
    const int64_t fc = ct * per_tile;                                     // fused queries per chunk
    const int64_t fmax = std::min<int64_t>(fc, a.nq);                     // stretches a chunk writes and reads at most: a last tile may be partly filled
    const int64_t nblk = range_keys_blocks(sstride);
    rc = ivr_reserve_queries(x, (int)ivr_ceil_div(ncols, 16));
    if (rc == IVR_OK) rc = ivr_reserve({{&x->fu_keys, (size_t)fmax * sstride * 8}});
    if (rc == IVR_OK && !a.k) rc = ivr_reserve({{&x->fu_off, (size_t)fmax * nblk * 8}, {&x->fu_total, 8}});
    if (rc != IVR_OK) return rc;
    rc = ivr_launch_tile_rows(x, x->qtiled, a.q, 0, ncols, a.normalize_q, nullptr, s);
    if (rc != IVR_OK) return rc;
    const int64_t *ids = x->has_ids ? x->ids : nullptr;
    const float4 *qtiled = reinterpret_cast<const float4 *>((const float *)x->qtiled);
    for (int64_t f0 = 0; f0 < a.nq; f0 += fc) {
        const int fcnt = (int)std::min<int64_t>(fc, a.nq - f0);
        const int64_t col0 = f0 * a.slots;                                // a multiple of 16: f0 is a multiple of per_tile
        const int cols = fcnt * a.slots;
        const FuScore sc{reinterpret_cast<const float4 *>(x->data), qtiled + (col0 >> 4) * x->dp4 * 16, x->dp4, (int)ivr_ceil_div(cols, 16), ntiles,
                         x->ntotal, a.w + col0, a.role + col0, cols, a.slots, a.combine, x->fu_keys, sstride};
        rc = a.fold == IVR_FUSE_MAX   ? fu_launch_score<IVR_FUSE_MAX>(x, sc, s)
             : a.fold == IVR_FUSE_MIN ? fu_launch_score<IVR_FUSE_MIN>(x, sc, s)
                                      : fu_launch_score<IVR_FUSE_SUM>(x, sc, s);
        if (rc != IVR_OK) return rc;
        const SrcFused src{x->fu_keys, sstride};
        if (a.k) {
            IvrProf prof("select_final", s, (double)fcnt * sstride * 8, true);
            const SelectOut o = SelectOut::to_rows(a.D + f0 * a.k, a.I + f0 * a.k, 0, ids);
            if (o.ids) launch_select<OUT_DI_IDS>(src, fcnt, a.k, o, s);
            else launch_select<OUT_DI>(src, fcnt, a.k, o, s);
        } else {
            IvrProf prof("fused_range_tail", s, (double)fcnt * sstride * 16, true);
            launch_range_keys(src, fcnt, f0, f0 == 0, a.threshold, x->fu_off, x->fu_total, a.lims, a.D, a.I, a.cap, ids, s);
        }
        IVR_LAUNCH_CHECK();
    }
    return IVR_OK;
}

}  // namespace

extern "C" {

int ivr_index_search_fused(ivr_index *x, const float *q, int nq, int slots, const float *w, const int8_t *role, int fold, int combine, int k,
                           int normalize_q, float *D, int64_t *I, ivr_stream stream) {
    const char *what = "ivr_index_search_fused";
    const FuArgs a{q, nq, slots, w, role, fold, combine, normalize_q, k, 0.f, nullptr, D, I, 0};
    const int rc = fu_check(what, x, a);
    if (rc != IVR_OK) return rc;
    IVR_REQUIRE(k >= 1 && k <= IVR_MAX_K, "%s: k=%d outside [1,%d]", what, k, IVR_MAX_K);
    std::lock_guard<std::mutex> lk(x->mu);
    IVR_HIP(hipSetDevice(x->ctx->device));
    return fu_search(what, x, a, (hipStream_t)stream);
}

int ivr_index_range_search_fused(ivr_index *x, const float *q, int nq, int slots, const float *w, const int8_t *role, int fold, int combine,
                                 float threshold, int normalize_q, int64_t *lims, float *D, int64_t *I, int64_t cap, ivr_stream stream) {
    const char *what = "ivr_index_range_search_fused";
    const FuArgs a{q, nq, slots, w, role, fold, combine, normalize_q, 0, threshold, lims, D, I, cap};
    const int rc = fu_check(what, x, a);
    if (rc != IVR_OK) return rc;
    IVR_REQUIRE(lims, "%s: NULL argument", what);
    IVR_REQUIRE(cap >= 0, "%s: cap=%lld", what, (long long)cap);
    IVR_REQUIRE(!(threshold != threshold), "%s: threshold is NaN", what);
    std::lock_guard<std::mutex> lk(x->mu);
    IVR_HIP(hipSetDevice(x->ctx->device));
    return fu_search(what, x, a, (hipStream_t)stream);
}

}  // extern "C"
