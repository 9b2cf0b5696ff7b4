// Frame clustering over the flat index (ivr_index_dbscan) and the representative of a run of rows (ivr_segment_best_cosine): the
// reference's AdvancedKeyframeExtractor.cluster_similar_frames / select_representative_frame (filter_research_update.py:113-155)
// without the N x N distance matrix and without sklearn.  DESIGN.md section 4, "frame clustering".
//
// Score S[j, i] = <stored row j as the query, stored row i> with the bits ivr_index_search and ivr_index_rescore report for that
// pair.  The segment bounds, the query block in LDS and the scoring of a stored tile are the self-join frame's (self_join.h); here are
// the walk of the triangle, the three integer epilogues and the union-find.
//   edge     rows i < j of one segment with 1.0f - S[j, i] <= eps (one rounded subtraction; only the higher row is ever the query)
//   core     1 + edges at the row >= min_samples, and the row lies in a segment
//   cluster  a connected component of the core rows; its root is its lowest row
//   border   a non-core row with a core neighbour takes the cluster with the lowest root among its core neighbours
//   label    the rank of the cluster's root among the roots of its own segment, -1 for noise
//
// Launches, all on the caller's stream and without a host round trip:
//   sj_bounds    per row: seg_lo (the start of its segment, row + 1 outside every segment); deg is cleared by a memset beside it
//   cl_score<COUNT>   the tiled self-join, every accepted pair adds 1 to deg of both rows
//   cl_core      per row: the core byte, and parent = row, broot = none for the two passes behind it
//   cl_score<UNITE>   accepted pairs of two core rows: union-find over parent, written only through atomicMin
//   cl_flatten   root[i] = find(i), into its own array
//   cl_score<BORDER>  accepted pairs of one core and one non-core row: broot[non-core] = min(broot, root[core])
//   cl_scan      exclusive prefix sum of the root flags (one workgroup)
//   cl_labels    labels, and the cluster count of every segment
// Every result is an integer and every atomic is an integer add or min, so the output has the same bits on every run.
#include <climits>

#include "ivr_common.h"
#include "self_join.h"

namespace {

enum { CL_COUNT = 0, CL_UNITE = 1, CL_BORDER = 2 };
constexpr int kNoRoot = INT_MAX;
constexpr int kClMaxPieces = 65535;         // grid.y; an index of more than 65535 kSjSplit tiles gets longer pieces

// The per-row words of a call: the segment starts of the self-join frame, and one block of x->cl_words, each array rounded up to a
// multiple of 64 words
struct ClWords {
    const int *seg_lo;
    int *deg, *parent, *root, *broot, *prefix;      // prefix is [n + 1]
    static int64_t stride(int64_t n) { return ivr_round_up(n + 1, 64); }
    ClWords(const int *seg, int *p, int64_t n) {
        const int64_t s = stride(n);
        seg_lo = seg, deg = p, parent = p + s, root = p + 2 * s, broot = p + 3 * s, prefix = p + 4 * s;
    }
};

__device__ __forceinline__ int cl_load(const int *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// parent[x] <= x always (it starts as x and only atomicMin writes it), so a walk strictly descends and ends after at most x steps,
// whatever other threads write meanwhile
__device__ __forceinline__ int cl_find(const int *parent, int x) {
    for (int p = cl_load(parent + x); p != x; p = cl_load(parent + x)) x = p;
    return x;
}

// Union by index: the larger root is hooked under the smaller with atomicMin.  When the atomicMin finds that `hi` was no root any
// more (its old parent `old` != hi), parent[hi] is now min(old, lo) and the link that lost is restored by uniting old with lo.  Both
// are < hi, so the larger of the pair strictly decreases from round to round: at most max(a, b) rounds.  No thread waits for another's
// write.  The smaller root always wins, so the lowest row of a component is never hooked and is its root in the end, whatever the
// interleaving.
__device__ __forceinline__ void cl_unite(int *parent, int a, int b) {
    for (;;) {
        a = cl_find(parent, a);
        b = cl_find(parent, b);
        if (a == b) return;
        const int hi = max(a, b), lo = min(a, b);
        const int old = atomicMin(parent + hi, lo);
        if (old == hi || old == lo) return;
        a = old;
        b = lo;
    }
}

struct ClScore {
    SjArgs j;                    // query blocks of ivr_index::qt_max() tiles
    int ntiles;                  // 16-row tiles that hold stored rows
    int split;                   // stored tiles per piece of a walk: kSjSplit, more when that would be more than kClMaxPieces pieces
    float eps;
    ClWords w;
    const uint8_t *core;         // UNITE, BORDER
};

// Workgroup (b, c) holds the tiles tb0 .. tb0 + nq - 1 of the rows j (the queries) in LDS, as they lie in the storage, and streams
// the stored tiles ta of the rows i, one per wave at a time: of the walk from the tile of seg_lo[16 tb0] up to the block's own last
// tile it takes the piece inside [c split, (c + 1) split), and leaves at once when that is empty.  Pieces of equal length
// balance the triangle (the last query block walks the whole index, the first one tile).  seg_lo ascends with the row (segments are
// contiguous and ascending; a row outside them has row + 1), so seg_lo[16 tb0] is the lowest segment start among the workgroup's
// columns.  Tile pairs with ta above tb are scored but accept nothing (i < j fails), which wastes at most 6 of the pairs of a query
// block.  The query block is the fast grid index, so the workgroups that stream the same piece run together and share it in cache.
// Every tile read lies inside the storage's allocation, whose capacity is a multiple of 64 rows >= ntotal; every word written belongs
// to a row < n, because an accepted entry has i < j < n.
template <int EPI>
__global__ __launch_bounds__(64 * kSjWaves) void cl_score_kernel(ClScore a) {
    extern __shared__ __attribute__((aligned(16))) float4 qs[];
    const int tb0 = (int)blockIdx.x * a.j.qt, nq = min(a.j.qt, a.ntiles - tb0);
    const int ta0 = max(min(a.j.seg_lo[tb0 * 16], tb0 * 16) >> 4, (int)blockIdx.y * a.split);
    const int ta1 = min(tb0 + nq, (int)std::min<int64_t>(((int64_t)blockIdx.y + 1) * a.split, INT_MAX));
    if (ta0 >= ta1) return;          // the whole workgroup: nothing staged, no barrier reached
    sj_stage(a.j, tb0, nq, qs);
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    // this lane's column of each query tile: row col.jq, accepted rows i in [col.lo, col.jq); col.lo is INT_MAX for a column that is no stored row
    const SjCols col = sj_columns(a.j, tb0, nq);
    int cj[4];
    bool corej[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        corej[q] = EPI != CL_COUNT && col.lo[q] != INT_MAX && a.core[col.jq[q]];
        cj[q] = 0;
    }
    for (int ta = ta0 + wave; ta < ta1; ta += kSjWaves) {
        f32x4 acc[4];
        sj_score_tile(a.j, qs, nq, ta, acc);
        const int i0 = ta * 16 + (lane >> 4) * 4;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            bool ok[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) ok[r] = i0 + r >= col.lo[q] && i0 + r < col.jq[q] && 1.0f - acc[q][r] <= a.eps;
            if (!__any(ok[0] || ok[1] || ok[2] || ok[3])) continue;
            if (EPI == CL_COUNT) {
                // deg[j]: summed in the lane over the whole walk, reduced once at the end.  deg[i]: the 16 lanes of a quad row hold
                // row i0 + r for the 16 columns, one ballot per r counts them and lane r of the quad row adds the count
                cj[q] += (int)ok[0] + (int)ok[1] + (int)ok[2] + (int)ok[3];
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const uint64_t m = __ballot(ok[r]);
                    const int c = __popc((unsigned)(m >> (lane & 48)) & 0xffffu);
                    if ((lane & 15) == r && c) atomicAdd(a.w.deg + i0 + r, c);
                }
            } else {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    if (!ok[r]) continue;
                    const int i = i0 + r;
                    const bool corei = a.core[i];
                    if (EPI == CL_UNITE) {
                        if (corei && corej[q]) cl_unite(a.w.parent, i, col.jq[q]);
                    } else if (corei != corej[q]) {
                        if (corei) atomicMin(a.w.broot + col.jq[q], a.w.root[i]);
                        else atomicMin(a.w.broot + i, a.w.root[col.jq[q]]);
                    }
                }
            }
        }
    }
    if (EPI == CL_COUNT) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            int c = cj[q];
            c += __shfl_xor(c, 16, 64);
            c += __shfl_xor(c, 32, 64);
            if (lane < 16 && c) atomicAdd(a.w.deg + col.jq[q], c);      // c > 0: column col.jq[q] accepted something, so it is a stored row
        }
    }
}

// the core byte of every row, and the start of the two passes behind it: every row its own root, no border root
__global__ __launch_bounds__(256) void cl_core_kernel(int n, int min_samples, ClWords w, uint8_t *__restrict__ core) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    core[i] = w.seg_lo[i] <= i && (int64_t)w.deg[i] + 1 >= min_samples;
    w.parent[i] = i;
    w.broot[i] = kNoRoot;
}

__global__ __launch_bounds__(256) void cl_flatten_kernel(int n, ClWords w) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) w.root[i] = cl_find(w.parent, i);
}

// prefix[i] = roots among the rows below i, prefix[n] = all of them: one workgroup walks the rows 1024 at a time and carries the sum
__global__ __launch_bounds__(1024) void cl_scan_kernel(int n, ClWords w, const uint8_t *__restrict__ core) {
    __shared__ int wsum[16];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int carry = 0;
    for (int i0 = 0; i0 < n; i0 += 1024) {
        const int i = i0 + (int)threadIdx.x;
        const int f = i < n && core[i] && w.root[i] == i;
        const int incl = ivr_wave_incl_scan(f, lane);
        if (lane == 63) wsum[wave] = incl;
        __syncthreads();
        int before = carry, total = carry;
        for (int v = 0; v < 16; ++v) {
            if (v < wave) before += wsum[v];
            total += wsum[v];
        }
        if (i < n) w.prefix[i] = before + incl - f;
        carry = total;
        __syncthreads();
    }
    if (threadIdx.x == 0) w.prefix[n] = carry;
}

// The root of row i's cluster c lies in i's segment, so its rank there is prefix[c] - prefix[seg_lo[i]].  Thread s < nseg also counts
// the roots of segment s (offsets clipped to [0, n]); without segments nclusters[0] is the total.
__global__ __launch_bounds__(256) void cl_labels_kernel(int n, ClWords w, const uint8_t *__restrict__ core, const int64_t *__restrict__ seg_off,
                                                        int nseg, int32_t *__restrict__ labels, int32_t *__restrict__ nclusters) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) {
        const int c = core[i] ? w.root[i] : w.broot[i];
        labels[i] = c == kNoRoot ? -1 : w.prefix[c] - w.prefix[w.seg_lo[i]];
    }
    if (!seg_off) {
        if (i == 0) nclusters[0] = w.prefix[n];
    } else if (i < nseg) {
        const int64_t s0 = min(max(seg_off[i], (int64_t)0), (int64_t)n), s1 = min(max(seg_off[i + 1], s0), (int64_t)n);
        nclusters[i] = w.prefix[s1] - w.prefix[s0];
    }
}

// One workgroup per run of rows; wave v takes the rows s0 + v, s0 + v + 4, ...  The cosine of a row with the run's centre is the
// arithmetic of rowwise_cosine_kernel (csrc/dedup.hip) with a = the row and b = the centre: lane l runs the fma chains over the
// columns l, l + 64, ..., ivr_wave_sum adds the lanes, a zero norm counts as 1.  The centre's squared norm is that chain once.  A wave
// keeps its first best row (strict >), the four waves are merged by (cosine, lower row); a NaN cosine is never the best.
__global__ __launch_bounds__(256) void segment_best_cosine_kernel(const float *__restrict__ rows, int64_t n, const int64_t *__restrict__ seg_off, int d,
                                                                  const float *__restrict__ centers, int64_t *__restrict__ best,
                                                                  float *__restrict__ score) {
    __shared__ float bc[4];
    __shared__ int64_t br[4];
    const int64_t sgm = blockIdx.x;
    const int64_t s0 = min(max(seg_off[sgm], (int64_t)0), n), s1 = min(max(seg_off[sgm + 1], s0), n);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const float *pb = centers + sgm * d;
    float sb = 0.f;
    for (int k = lane; k < d; k += 64) sb = fmaf(pb[k], pb[k], sb);
    sb = ivr_wave_sum(sb);
    const float nb = sb > 0.f ? sqrtf(sb) : 1.f;
    float cbest = -FLT_MAX;
    int64_t rbest = -1;
    for (int64_t r = s0 + wave; r < s1; r += 4) {
        const float *pa = rows + r * d;
        float dot = 0.f, sa = 0.f;
        for (int k = lane; k < d; k += 64) {
            const float x = pa[k], y = pb[k];
            dot = fmaf(x, y, dot);
            sa = fmaf(x, x, sa);
        }
        dot = ivr_wave_sum(dot);
        sa = ivr_wave_sum(sa);
        const float na = sa > 0.f ? sqrtf(sa) : 1.f;
        const float c = dot / (na * nb);
        if (c > cbest || (rbest < 0 && c == c)) cbest = c, rbest = r;
    }
    if (lane == 0) bc[wave] = cbest, br[wave] = rbest;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int v = 1; v < 4; ++v)
            if (br[v] >= 0 && (br[0] < 0 || bc[v] > bc[0] || (bc[v] == bc[0] && br[v] < br[0]))) bc[0] = bc[v], br[0] = br[v];
        best[sgm] = br[0];
        score[sgm] = br[0] < 0 ? -FLT_MAX : bc[0];
    }
}

template <int EPI>
int cl_launch_score(const char *name, ivr_index *x, const ClScore &a, hipStream_t s) {
    const size_t lds = (size_t)a.j.qt * 16 * x->dp * 4;
    const int rc = ivr_func_max_lds(reinterpret_cast<const void *>(cl_score_kernel<EPI>), (int)lds);
    if (rc != IVR_OK) return rc;
    IvrProf prof(name, s, (double)x->ntotal * x->ntotal * x->dp);
    hipLaunchKernelGGL(cl_score_kernel<EPI>, dim3((unsigned)ivr_ceil_div(a.ntiles, a.j.qt), (unsigned)ivr_ceil_div(a.ntiles, a.split)),
                       dim3(64 * kSjWaves), lds, s, a);
    IVR_LAUNCH_CHECK();
    return IVR_OK;
}

}  // namespace

extern "C" {

int ivr_index_dbscan(ivr_index *x, float eps, int min_samples, const int64_t *seg_off, int nseg, int32_t *labels, uint8_t *core,
                     int32_t *nclusters, ivr_stream stream) {
    IVR_REQUIRE(x && labels && core && nclusters, "ivr_index_dbscan: NULL argument");
    IVR_REQUIRE(eps >= 0.f, "ivr_index_dbscan: eps=%g is negative or NaN", (double)eps);
    IVR_REQUIRE(min_samples >= 1, "ivr_index_dbscan: min_samples=%d < 1", min_samples);
    IVR_REQUIRE(!seg_off || nseg >= 1, "ivr_index_dbscan: nseg=%d with seg_off", nseg);
    hipStream_t s = (hipStream_t)stream;
    std::lock_guard<std::mutex> lk(x->mu);
    IVR_REQUIRE(x->ntotal < (1ll << 31), "ivr_index_dbscan: ntotal=%lld >= 2^31", (long long)x->ntotal);
    if (x->ntotal == 0) return IVR_OK;
    IVR_HIP(hipSetDevice(x->ctx->device));
    const int n = (int)x->ntotal;
    int rc = ivr_reserve({{&x->cl_words, (size_t)5 * ClWords::stride(n) * 4}});
    if (rc != IVR_OK) return rc;
    SjArgs j;
    rc = sj_prepare(x, x->qt_max(), seg_off, nseg, s, j);
    if (rc != IVR_OK) return rc;
    const ClWords w(j.seg_lo, x->cl_words, n);
    const unsigned nblk = (unsigned)ivr_ceil_div(n, 256);
    IVR_HIP(hipMemsetAsync(w.deg, 0, (size_t)n * 4, s));
    const int ntiles = (int)ivr_ceil_div(n, 16);
    const ClScore sc{j, ntiles, std::max(kSjSplit, (int)ivr_ceil_div(ntiles, kClMaxPieces)), eps, w, core};
    rc = cl_launch_score<CL_COUNT>("cluster_count", x, sc, s);
    if (rc != IVR_OK) return rc;
    hipLaunchKernelGGL(cl_core_kernel, dim3(nblk), dim3(256), 0, s, n, min_samples, w, core);
    IVR_LAUNCH_CHECK();
    rc = cl_launch_score<CL_UNITE>("cluster_unite", x, sc, s);
    if (rc != IVR_OK) return rc;
    hipLaunchKernelGGL(cl_flatten_kernel, dim3(nblk), dim3(256), 0, s, n, w);
    IVR_LAUNCH_CHECK();
    rc = cl_launch_score<CL_BORDER>("cluster_border", x, sc, s);
    if (rc != IVR_OK) return rc;
    hipLaunchKernelGGL(cl_scan_kernel, dim3(1), dim3(1024), 0, s, n, w, (const uint8_t *)core);
    IVR_LAUNCH_CHECK();
    const unsigned lblk = (unsigned)ivr_ceil_div(std::max(n, seg_off ? nseg : 1), 256);
    hipLaunchKernelGGL(cl_labels_kernel, dim3(lblk), dim3(256), 0, s, n, w, (const uint8_t *)core, seg_off, nseg, labels, nclusters);
    IVR_LAUNCH_CHECK();
    return IVR_OK;
}

int ivr_segment_best_cosine(ivr_ctx *ctx, const float *rows, int64_t n, const int64_t *seg_off, int nseg, int d, const float *centers,
                            int64_t *best, float *score, ivr_stream stream) {
    IVR_REQUIRE(ctx && seg_off && centers && best && score && (rows || n == 0), "ivr_segment_best_cosine: NULL argument");
    IVR_REQUIRE(n >= 0 && nseg >= 1 && d >= 1, "ivr_segment_best_cosine: n=%lld nseg=%d d=%d", (long long)n, nseg, d);
    IVR_HIP(hipSetDevice(ctx->device));
    hipStream_t s = (hipStream_t)stream;
    IvrProf prof("segment_best_cosine", s, (double)n * d * 4 + (double)nseg * d * 4, true);
    hipLaunchKernelGGL(segment_best_cosine_kernel, dim3((unsigned)nseg), dim3(256), 0, s, rows, n, seg_off, d, centers, best, score);
    IVR_LAUNCH_CHECK();
    return IVR_OK;
}

}  // extern "C"
