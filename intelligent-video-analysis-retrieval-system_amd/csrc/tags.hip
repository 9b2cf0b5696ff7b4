// Zero-shot tagging over the flat index (ivr_index_tag_rows, ivr_index_tag_segments): for every stored row the best t of C label
// vectors with their softmax probabilities over ALL C labels, and per segment (video) the top labels by summed probability or by
// votes.  CLIP's logits_per_image.softmax(dim=1) for the stored frames, which fills what the reference leaves to a remote vision
// call (KeyframeMetadata.scene_tags, core.py:101; MetadataManager.add_semantic_tags, core.py:3278).  DESIGN.md section 4, "zero-shot
// tagging".
//
// Score S[j, i] = <stored row j as the query, label i as the stored row>: the bits a FlatIPIndex holding the labels reports for
// the reconstructed row j as the query.  That is the direction the self-join frame (self_join.h) gives as it stands: the block of
// stored tiles staged in LDS is the B operand, the label tiles are streamed past it as the A operand by stream_tile / mfma_chunk4.
// The frame's segment bounds are not used: every label is a candidate of every row.
//   candidates of j   the labels i < C with S[j, i] not NaN (+-inf scores are outside the definition)
//   order             ivr_key(S[j, i], i): score descending, equal scores the lower label
//   probability       P[j, i] = exp(scale (S[j, i] - m_j)) / Z_j,  m_j the best score, Z_j the sum over the candidates
//
// Launches of ivr_index_tag_rows, all on the caller's stream and without a host round trip:
//   tile_rows   the labels -> x->tg_labels in the storage-tile layout (C padded to 16 with zero rows; normalised as add() does)
//   tg_rows     workgroup b stages block b of the row range (tg_qt() tiles) and streams ALL label tiles past it, one per wave and
//               round.  Per column a knn-style list of t keys in LDS; per lane and column a running (max, sum) of an online softmax.
//               The partial pairs of the 4 quad rows x kSjWaves waves of a column are merged in a fixed order at the end.
// ivr_index_tag_segments runs that pass into scratch per chunk of rows, adds the rows' lists up per (segment, label) with integer
// atomics only (tg_agg), and picks the top g labels of every segment (tg_select).
#include <cfloat>
#include <climits>

#include "ivr_common.h"
#include "self_join.h"

namespace {

constexpr int64_t kTgTableSlots = 1ll << 25;     // nseg x C entries of the segment tables (12 bytes each): beyond that IVR_ERR_INVALID
constexpr int64_t kTgChunkSlots = 1ll << 24;     // rows x t list slots of one chunk of the segment call's row pass (24 bytes each + 8 per row)

struct TgArgs {
    SjArgs rows;                 // the stored rows: blocks of rows.qt tiles are staged
    SjArgs lab;                  // the label tiles: streamed
    int C, t;
    float scale, min_prob;
    int row0, row1;              // rows [row0, row1) are written
    int64_t out0;                // row j goes to line j - out0 of the outputs
    float *D, *P;
    int64_t *J;
    int32_t *count;
    float *Z;
};

// the merge of the online-softmax pairs of one column, in the order they are given: (m, z) <- (m, z) + (pm, pz)
__device__ __forceinline__ void tg_fold(float &m, float &z, float pm, float pz, float scale) {
    if (pz == 0.f) return;                           // a partial without candidates
    const float mn = fmaxf(m, pm);
    z = z * expf(scale * (m - mn)) + pz * expf(scale * (pm - mn));
    m = mn;
}

// Workgroup b holds the tiles of block b of the row range in LDS as they lie in the storage and streams every label tile, tile
// 8 r + w in round r on wave w: the assignment of labels to waves, and with it every partial sum, is fixed.  The lists are the
// neighbour graph's (knn.hip, kn_score_kernel): list[slot][column], descending, 0 = unused, the last slot is the column's threshold;
// the waves with survivors in a round take turns, a barrier after each, and within a turn lane (q, c) owns column 16 q + c.  The
// keys of a column are unique, so its final list is the best t whatever the order of the insertions.
__global__ __launch_bounds__(64 * kSjWaves) void tg_rows_kernel(TgArgs a) {
    extern __shared__ __attribute__((aligned(16))) float4 qs[];
    const int t = a.t, qt = a.rows.qt, ncol = qt * 16;
    const int tile0 = a.row0 >> 4, tile1 = (a.row1 + 15) >> 4;                   // row1 <= n: inside the tiles that hold stored rows
    const int tb0 = tile0 + (int)blockIdx.x * qt, nq = min(qt, tile1 - tb0);
    const int ctiles = (a.C + 15) >> 4;
    uint64_t *list = reinterpret_cast<uint64_t *>(qs + qt * a.rows.dp4 * 16);     // [t][ncol]
    float2 *part = reinterpret_cast<float2 *>(list + t * ncol);                   // [kSjWaves][4 quad rows][64 columns]: (max, sum)
    float2 *tot = part + kSjWaves * 4 * 64;                                       // [64 columns]: (m, Z)
    int *used = reinterpret_cast<int *>(tot + 64);                                // [64 columns]: the first slot that is not used
    unsigned *flag = reinterpret_cast<unsigned *>(used + 64);                     // [3]: the waves with survivors in round r, at r % 3
    sj_stage(a.rows, tb0, nq, qs);
    for (int i = threadIdx.x; i < t * ncol; i += blockDim.x) list[i] = 0;
    if (threadIdx.x < 64) used[threadIdx.x] = t;
    if (threadIdx.x < 3) flag[threadIdx.x] = 0;
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, h = lane >> 4, c = lane & 15;
    float m[4], z[4];                                // this lane's share of column 16 q + c: labels 16 ta + 4 h + r of its wave's tiles
#pragma unroll
    for (int q = 0; q < 4; ++q) m[q] = -FLT_MAX, z[q] = 0.f;
    int round = 0;
    for (int t0 = 0; t0 < ctiles; t0 += kSjWaves, ++round) {
        const int ta = t0 + wave;
        uint64_t key[4][4];
        bool mine = false;
        if (ta < ctiles) {                           // wave-uniform
            f32x4 acc[4];
            sj_score_tile(a.lab, qs, nq, ta, acc);
            const int i0 = ta * 16 + h * 4;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const uint64_t low = q < nq ? list[(t - 1) * ncol + q * 16 + c] : ~0ull;
                float s[4], mx = -FLT_MAX;
                bool ok[4], any = false;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    s[r] = acc[q][r] + 0.0f;         // -0.0 counts as +0.0, as in the key
                    ok[r] = q < nq && i0 + r < a.C && s[r] == s[r];
                    if (ok[r]) mx = fmaxf(mx, s[r]), any = true;
                    const uint64_t x = ivr_key(s[r], (uint32_t)(i0 + r));
                    key[q][r] = ok[r] && x > low ? x : 0;
                    mine = mine || key[q][r] != 0;
                }
                if (any) {                           // the online softmax: rescale the sum to the new maximum, add the four terms
                    const float mn = fmaxf(m[q], mx);
                    float zz = z[q] * expf(a.scale * (m[q] - mn));
#pragma unroll
                    for (int r = 0; r < 4; ++r)
                        if (ok[r]) zz += expf(a.scale * (s[r] - mn));
                    m[q] = mn, z[q] = zz;
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
                    // this lane gives what it holds for the column of row tile (h - s) & 3 and takes, as the owner of column 16 h + c, what
                    // the lane of quad row (h + s) & 3 holds for row tile h
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
                    if (!__any(some)) continue;
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const uint32_t xh = __shfl((uint32_t)(give[r] >> 32), from, 64), xl = __shfl((uint32_t)give[r], from, 64);
                        take[r] = ((uint64_t)xh << 32) | xl;
                    }
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const uint64_t x = take[r];
                        if (x != 0 && x > list[(t - 1) * ncol + lane]) {       // x != 0: row tile h exists, so lane < ncol
                            int p = t - 1;
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
    // the partial pairs of column 16 q + c: one per wave and quad row
#pragma unroll
    for (int q = 0; q < 4; ++q) part[(wave * 4 + h) * 64 + q * 16 + c] = make_float2(m[q], z[q]);
    __syncthreads();
    if (threadIdx.x < nq * 16) {                     // merged wave by wave, quad row by quad row: one order, so one sum
        float mm = -FLT_MAX, zz = 0.f;
        for (int p = 0; p < kSjWaves * 4; ++p) {
            const float2 v = part[p * 64 + threadIdx.x];
            tg_fold(mm, zz, v.x, v.y, a.scale);
        }
        tot[threadIdx.x] = make_float2(mm, zz);
        const int j = tb0 * 16 + (int)threadIdx.x;
        if (j >= a.row0 && j < a.row1) a.Z[j - a.out0] = zz;
    }
    __syncthreads();
    // P of every list slot, twice with the same operations: first for the column's first slot below min_prob (or empty), then for
    // the output.  A slot is used while P >= min_prob, so min_prob truncates the list
    for (int pass = 0; pass < 2; ++pass) {
        for (int i = threadIdx.x; i < nq * 16 * t; i += blockDim.x) {
            const int col = i / t, p = i % t, j = tb0 * 16 + col;
            if (j < a.row0 || j >= a.row1) continue;
            const uint64_t x = list[p * ncol + col];
            const float2 mz = tot[col];
            const float s = ivr_ord2f((uint32_t)(x >> 32));
            const float pr = x != 0 ? expf(a.scale * (s - mz.x)) / mz.y : 0.f;
            const bool keep = x != 0 && pr >= a.min_prob;
            if (pass == 0) {
                if (!keep) atomicMin(used + col, p);
                continue;
            }
            const bool on = p < used[col];
            const int64_t o = (j - a.out0) * t + p;
            a.D[o] = on ? s : -FLT_MAX;
            a.P[o] = on ? pr : 0.f;
            a.J[o] = on ? (int64_t)(0xFFFFFFFFu - (uint32_t)x) : -1;
            if (p == 0) a.count[j - a.out0] = used[col];
        }
        __syncthreads();
    }
}

// row tiles of a block: as many (at most 4) as leave room for their lists in 160 KiB of LDS
size_t tg_lds(int qt, int dp, int t) {
    return (size_t)qt * 16 * ((size_t)dp * 4 + (size_t)t * 8) + (size_t)kSjWaves * 4 * 64 * 8 + 64 * 8 + 64 * 4 + 16;
}
int tg_qt(int dp, int t) {
    int qt = 4;
    while (qt > 1 && tg_lds(qt, dp, t) > 160 * 1024) --qt;
    return qt;
}

// ---- the tags of a segment ------------------------------------------------------------------------------------------------------
struct TgSeg {
    int n0, n1;                  // the rows of the chunk
    int t, C, nseg;
    const int *rowseg;           // [n]: the segment of each row, -1 / nseg outside every segment
    const float *P;              // the row pass of the chunk: line j - n0
    const int64_t *J;
    const int32_t *count;
    unsigned long long *mass;    // [nseg][C]
    int *votes;                  // [nseg][C]
    int *rows;                   // [nseg]
};

// One thread per list slot of the chunk.  Integer adds only: any arrival order gives the same tables.
__global__ __launch_bounds__(256) void tg_agg_kernel(TgSeg a) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (int64_t)(a.n1 - a.n0) * a.t) return;
    const int r = (int)(i / a.t), p = (int)(i % a.t);
    const int s = a.rowseg[a.n0 + r];
    if (s < 0 || s >= a.nseg) return;
    if (p == 0) atomicAdd(a.rows + s, 1);
    if (p >= a.count[r]) return;
    const int64_t e = (int64_t)s * a.C + a.J[i];
    atomicAdd(a.mass + e, (unsigned long long)__float2uint_rn(a.P[i] * 16777216.f));         // P 2^24 is exact in float32
    if (p == 0) atomicAdd(a.votes + e, 1);
}

// One workgroup per segment, g rounds: the greatest (value, lower label) that is below the pick of the round before.  value = mass
// or votes; a label whose value is 0 is no tag of the segment.
__global__ __launch_bounds__(256) void tg_select_kernel(const unsigned long long *__restrict__ mass, const int *__restrict__ votes,
                                                        const int *__restrict__ rows, int C, int g, int by_votes, int64_t *__restrict__ L,
                                                        unsigned long long *__restrict__ M, int32_t *__restrict__ V,
                                                        int32_t *__restrict__ R) {
    __shared__ unsigned long long wv[4];
    __shared__ int wl[4];
    const int seg = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long *ms = mass + (int64_t)seg * C;
    const int *vs = votes + (int64_t)seg * C;
    if (threadIdx.x == 0) R[seg] = rows[seg];
    unsigned long long pv = ~0ull;                   // the pick of the round before: everything is below (~0, -1)
    int pl = -1;
    for (int k = 0; k < g; ++k) {
        unsigned long long bv = 0;
        int bl = INT_MAX;
        for (int i = threadIdx.x; i < C; i += 256) {
            const unsigned long long v = by_votes ? (unsigned long long)vs[i] : ms[i];
            const bool below = v < pv || (v == pv && i > pl);
            if (v != 0 && below && (v > bv || (v == bv && i < bl))) bv = v, bl = i;
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const unsigned long long ov = ((unsigned long long)__shfl_xor((uint32_t)(bv >> 32), o, 64) << 32) | __shfl_xor((uint32_t)bv, o, 64);
            const int ol = __shfl_xor(bl, o, 64);
            if (ov > bv || (ov == bv && ol < bl)) bv = ov, bl = ol;
        }
        if (lane == 0) wv[wave] = bv, wl[wave] = bl;
        __syncthreads();
        bv = wv[0], bl = wl[0];
#pragma unroll
        for (int w = 1; w < 4; ++w)
            if (wv[w] > bv || (wv[w] == bv && wl[w] < bl)) bv = wv[w], bl = wl[w];
        __syncthreads();
        const bool hit = bv != 0;
        if (threadIdx.x == 0) {
            const int64_t o = (int64_t)seg * g + k;
            L[o] = hit ? bl : -1;
            M[o] = hit ? ms[bl] : 0;
            V[o] = hit ? vs[bl] : 0;
        }
        if (hit) pv = bv, pl = bl;
        else pv = 0, pl = INT_MAX;                   // nothing is below (0, INT_MAX): the remaining rounds write unused slots
    }
}

// The checks both entry points share, and the label tiles.  The caller holds x->mu
int tg_check(const char *what, const ivr_index *x, const float *labels, int C, float scale, int t, float min_prob) {
    IVR_REQUIRE(labels, "%s: NULL labels", what);
    IVR_REQUIRE(C >= 1 && C <= IVR_TAG_MAX_LABELS, "%s: C=%d outside [1,%d]", what, C, IVR_TAG_MAX_LABELS);
    IVR_REQUIRE(t >= 1 && t <= IVR_TAG_MAX_TOP, "%s: top=%d outside [1,%d]", what, t, IVR_TAG_MAX_TOP);
    IVR_REQUIRE(scale > 0.f && scale <= FLT_MAX, "%s: scale=%g is not a positive finite number", what, (double)scale);
    IVR_REQUIRE(min_prob == min_prob, "%s: min_prob=%g is NaN", what, (double)min_prob);
    return IVR_OK;
}

int tg_stage_labels(ivr_index *x, const float *labels, int C, int normalize, hipStream_t s) {
    const int rc = ivr_reserve({{&x->tg_labels, (size_t)ivr_round_up(C, 16) * x->dp * 4}});
    if (rc != IVR_OK) return rc;
    return ivr_launch_tile_rows(x, x->tg_labels, labels, 0, C, normalize, nullptr, s);
}

// the row pass over rows [row0, row1) of x (0 <= row0 < row1 <= ntotal < 2^31) against the staged labels
int tg_launch_rows(ivr_index *x, int C, float scale, int t, float min_prob, int row0, int row1, int64_t out0, float *D, float *P,
                   int64_t *J, int32_t *count, float *Z, hipStream_t s) {
    const int qt = tg_qt(x->dp, t);
    const size_t lds = tg_lds(qt, x->dp, t);
    const int rc = ivr_func_max_lds(reinterpret_cast<const void *>(tg_rows_kernel), (int)lds);
    if (rc != IVR_OK) return rc;
    const SjArgs rows{reinterpret_cast<const float4 *>(x->data), x->dp4, qt, (int)x->ntotal, nullptr, nullptr};
    const SjArgs lab{reinterpret_cast<const float4 *>((const float *)x->tg_labels), x->dp4, qt, C, nullptr, nullptr};
    const TgArgs a{rows, lab, C, t, scale, min_prob, row0, row1, out0, D, P, J, count, Z};
    const int tiles = ((row1 + 15) >> 4) - (row0 >> 4);
    IvrProf prof("tag_rows", s, 2.0 * (row1 - row0) * (double)C * x->dp);
    hipLaunchKernelGGL(tg_rows_kernel, dim3((unsigned)ivr_ceil_div(tiles, qt)), dim3(64 * kSjWaves), lds, s, a);
    IVR_LAUNCH_CHECK();
    return IVR_OK;
}

}  // namespace

extern "C" {

int ivr_tag_max_labels(void) { return IVR_TAG_MAX_LABELS; }

int ivr_tag_max_top(void) { return IVR_TAG_MAX_TOP; }

int ivr_index_tag_rows(ivr_index *x, const float *labels, int C, int normalize, float scale, int t, float min_prob, int64_t row0,
                       int64_t row1, float *D, float *P, int64_t *J, int32_t *count, float *Z, ivr_stream stream) {
    IVR_REQUIRE(x && D && P && J && count && Z, "ivr_index_tag_rows: NULL argument");
    int rc = tg_check("ivr_index_tag_rows", x, labels, C, scale, t, min_prob);
    if (rc != IVR_OK) return rc;
    IVR_REQUIRE(row0 >= 0 && row0 <= row1, "ivr_index_tag_rows: rows [%lld,%lld) are no range", (long long)row0, (long long)row1);
    hipStream_t s = (hipStream_t)stream;
    std::lock_guard<std::mutex> lk(x->mu);
    IVR_REQUIRE(x->ntotal < (1ll << 31), "ivr_index_tag_rows: ntotal=%lld >= 2^31", (long long)x->ntotal);
    row1 = std::min(row1, x->ntotal);
    if (row0 >= row1) return IVR_OK;
    IVR_HIP(hipSetDevice(x->ctx->device));
    rc = tg_stage_labels(x, labels, C, normalize, s);
    if (rc != IVR_OK) return rc;
    return tg_launch_rows(x, C, scale, t, min_prob, (int)row0, (int)row1, 0, D, P, J, count, Z, s);
}

int ivr_index_tag_segments(ivr_index *x, const float *labels, int C, int normalize, float scale, int t, float min_prob,
                           const int64_t *seg_off, int nseg, int g, int rank, int64_t *L, uint64_t *mass, int32_t *votes, int32_t *rows,
                           ivr_stream stream) {
    IVR_REQUIRE(x && L && mass && votes && rows, "ivr_index_tag_segments: NULL argument");
    int rc = tg_check("ivr_index_tag_segments", x, labels, C, scale, t, min_prob);
    if (rc != IVR_OK) return rc;
    IVR_REQUIRE(g >= 1 && g <= IVR_TAG_MAX_TOP, "ivr_index_tag_segments: top_labels=%d outside [1,%d]", g, IVR_TAG_MAX_TOP);
    IVR_REQUIRE(rank == IVR_TAG_RANK_MASS || rank == IVR_TAG_RANK_VOTES, "ivr_index_tag_segments: rank=%d is neither mass nor votes", rank);
    IVR_REQUIRE(!seg_off || nseg >= 1, "ivr_index_tag_segments: nseg=%d with seg_off", nseg);
    if (!seg_off) nseg = 1;
    IVR_REQUIRE((int64_t)nseg * C <= kTgTableSlots, "ivr_index_tag_segments: nseg x C = %lld table entries > %lld", (long long)nseg * C,
                (long long)kTgTableSlots);
    hipStream_t s = (hipStream_t)stream;
    std::lock_guard<std::mutex> lk(x->mu);
    IVR_REQUIRE(x->ntotal < (1ll << 31), "ivr_index_tag_segments: ntotal=%lld >= 2^31", (long long)x->ntotal);
    if (x->ntotal == 0) return IVR_OK;
    IVR_HIP(hipSetDevice(x->ctx->device));
    const int n = (int)x->ntotal;
    const int64_t slots = (int64_t)nseg * C;
    // mass [nseg][C] uint64, votes [nseg][C] int32, rows [nseg] int32: one block, zeroed per call
    const size_t table = (size_t)slots * 12 + (size_t)nseg * 4;
    const int chunk = (int)std::min<int64_t>(ivr_round_up(n, 64), kTgChunkSlots / t / 64 * 64);      // whole 64-row blocks
    rc = ivr_reserve({{&x->tg_table, table}});
    if (rc != IVR_OK) return rc;
    unsigned long long *tmass = reinterpret_cast<unsigned long long *>((uint64_t *)x->tg_table);
    int *tvotes = reinterpret_cast<int *>(tmass + slots), *trows = tvotes + slots;
    IVR_HIP(hipMemsetAsync(tmass, 0, table, s));
    // the row pass of one chunk: J first (8-byte words), then D, P, count, Z
    rc = ivr_reserve({{&x->tg_lists, (size_t)chunk * ((size_t)t * 16 + 8)}});
    if (rc != IVR_OK) return rc;
    int64_t *J = reinterpret_cast<int64_t *>((uint64_t *)x->tg_lists);
    float *D = reinterpret_cast<float *>(J + (int64_t)chunk * t), *P = D + (int64_t)chunk * t;
    int32_t *count = reinterpret_cast<int32_t *>(P + (int64_t)chunk * t);
    float *Z = reinterpret_cast<float *>(count + chunk);
    rc = tg_stage_labels(x, labels, C, normalize, s);
    if (rc != IVR_OK) return rc;
    rc = ivr_launch_rowseg(x, seg_off, nseg, s);
    if (rc != IVR_OK) return rc;
    for (int64_t r0 = 0; r0 < n; r0 += chunk) {
        const int r1 = (int)std::min<int64_t>(n, r0 + chunk);
        rc = tg_launch_rows(x, C, scale, t, min_prob, (int)r0, r1, r0, D, P, J, count, Z, s);
        if (rc != IVR_OK) return rc;
        const TgSeg a{(int)r0, r1, t, C, nseg, x->gr_seg, P, J, count, tmass, tvotes, trows};
        IvrProf prof("tag_agg", s, (double)(r1 - r0) * t * 16, true);
        hipLaunchKernelGGL(tg_agg_kernel, dim3((unsigned)ivr_ceil_div((r1 - r0) * t, 256)), dim3(256), 0, s, a);
        IVR_LAUNCH_CHECK();
    }
    IvrProf prof("tag_select", s, (double)slots * 12, true);
    hipLaunchKernelGGL(tg_select_kernel, dim3((unsigned)nseg), dim3(256), 0, s, tmass, tvotes, trows, C, g, rank == IVR_TAG_RANK_VOTES, L,
                       reinterpret_cast<unsigned long long *>(mass), votes, rows);
    IVR_LAUNCH_CHECK();
    return IVR_OK;
}

}  // extern "C"
