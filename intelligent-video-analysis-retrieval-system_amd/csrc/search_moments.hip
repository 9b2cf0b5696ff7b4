// Moment search over the flat index (ivr_index_search_moments, ivr_index_range_search_moments): the ranked time intervals of a query.
// A text query that matches a shot matches a run of adjacent keyframes; a moment is that run, "video X, frames 412 - 447", with its
// best frame.  The scored form of the reference's unscored temporal_context (system.py:1967-1974).  DESIGN.md section 4, "moment
// search".
//
// Frame score S[q, r] = <query q, stored row r>: the score pass of the clip search (ivr_launch_seq_score), so it has the bits
// ivr_index_search and ivr_index_rescore report for that pair.  Row r is HOT for q when it lies in a segment and S[q, r] >= threshold
// (false for NaN).  prev(r) = the greatest hot row below r.  A hot row is a HEAD when prev(r) is none, lies in another segment, or
// r - prev(r) > max_gap + 1.  A moment = a head and the hot rows behind it up to the next head: lo (the head), hi (its last hot row),
// cnt (its hot rows), peak (its best hot row by ivr_key: score descending, row ascending, -0.0 equal to +0.0).
//
// Launches per chunk of queries (whole 16-query tiles), all on the caller's stream and without a host round trip; the row -> segment
// table (ivr_launch_rowseg, search_groups.hip) once per call in front.  B = kMomBlock rows:
//   seq_score    the chunk's queries against every row -> S (search_seq.hip)
//   mom_count    one workgroup per (query, block of B rows), a thread holds 16 consecutive rows: the hot bits from S, the threshold and
//                the segment table; an exclusive running maximum of "last hot row" over the threads gives every hot row but the block's
//                first its prev.  Per (query, block): the first hot row, the last hot row, the heads among the hot rows other than the
//                first.  Those depend on the block alone
//   mom_prefix   one workgroup per query over its block summaries: the exclusive running maximum of the last hot row is the prev a
//                block enters with, which decides whether its first hot row is a head; the exclusive prefix sum of the heads numbers
//                the block's first moment within the query
//   mom_lims     one workgroup: the moments per query -> the number of each query's first moment in the chunk, lims of the range
//                form, and the running total of the call, carried on the device from chunk to chunk
//   mom_zero     hi, cnt and peak key of the chunk's moments = 0 (as many as the chunk has, read from the device)
//   mom_write    the grid of the count pass again.  Every hot row learns its moment: number of the block's first moment + heads up to
//                it - 1; the rows in front of the block's first head belong to the moment open on entry.  A thread folds its rows per
//                moment in registers, the workgroup folds per moment in LDS with integer atomics, and every (moment, block) pair then
//                contributes ONCE: lo is a plain store by the head; a moment that starts and ends inside the block is stored plainly;
//                the moment open on entry and the block's last one go through integer atomicMax (hi, 64-bit peak key) and atomicAdd
//                (cnt).  Only integer maxima and sums: the result does not depend on the order of arrival.  No float atomic, and
//                nothing in a launch waits for another workgroup: every carry across blocks crosses a launch boundary
//   tail         range form: mom_decode, the moments of the chunk to D / I / Lo / Hi / Cnt at lims order, positions >= cap counted and
//                not written.  Top-k form: select_topk_kernel (search_select.h) over the rank keys of each query's moments (0 past the
//                query's count and for cnt < min_count), then mom_gather: the moment behind a chosen key by ivr_last_le over the
//                query's ascending lo array, from the peak row (rank peak) or from lo itself (rank count)
// The cost does not depend on max_gap: it enters as one comparison per hot row.
//
// Moments of one query at most: heads of one segment are at least max_gap + 2 rows apart, so sum over the segments of
// ceil(len / (max_gap + 2)) <= ntotal / (max_gap + 2) + nseg, and never more than ntotal.  Scratch on the index, grow-only, each
// buffer on its own: S (4 bytes per (query of a chunk, row)), 16 bytes per (query of a chunk, block), 16 bytes per query of a chunk,
// 24 bytes per moment a chunk may hold, 12 bytes per result slot of the top-k form.  A chunk holds as many queries as keep S within
// IVR_SEQ_CHUNK_SLOTS floats (which keeps the moment arrays within as many slots: a query has no more moments than rows), in whole
// 16-query tiles, 16 at least and kMomMaxChunk at most (which keeps the grid of the run passes, blocks x queries, below 2^31).
#include "ivr_common.h"
#include "search_internal.h"
#include "search_select.h"

#include <cmath>

namespace {

constexpr int kMomThreads = 256;
constexpr int kMomPerThread = 16;                            // consecutive rows of one thread: four 16-byte loads of S and of the table
constexpr int kMomBlock = kMomThreads * kMomPerThread;       // rows per workgroup of the run passes: 4096, the block of the range tail
constexpr int kMomMaxChunk = 1 << 11;                        // queries per chunk at most
constexpr int kMomFillBlocks = 2048;                         // grid of the passes that run over a count read from the device
constexpr size_t kMomLds = (size_t)(kMomBlock + 1) * 16;     // mom_write: peak key, hi and cnt of the block's <= B + 1 moments

struct MomArgs {
    const float *S;              // line of the chunk's first query
    int64_t sstride;             // stored rows rounded up to 16: a line of S, and the length of rowseg
    const int *rowseg;           // the segment of every row: -1 in front of the first, nseg behind the last and for the padding rows
    int nseg;
    float threshold;
    int max_gap;
    int nblk;                    // row blocks per query
    int *blk;                    // [queries of the chunk][nblk][4]: first hot row, last hot row (-1: none), heads other than the first
                                 // hot row; after mom_prefix: [2] the number of the block's first moment in its query, [3] the prev it enters with
    int64_t *mq;                 // [cb] moments per query, [cb] the number of each query's first moment in the chunk, [3] totals
    int cb;                      // queries per chunk of the call (the layout of mq)
    int64_t mcap;                // moments the arrays hold
    uint64_t *peak;              // [mcap] (ordered S, ~row) of the best hot row
    int64_t *lo;                 // [mcap]
    int *hi, *cnt;               // [mcap]
};

// exclusive scans over the kMomThreads threads of a workgroup in thread order.  Sum: total = the workgroup's sum; wsum: LDS [4]
template <typename T>
__device__ __forceinline__ T mom_excl_sum(T v, T &total, T *wsum) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const T incl = ivr_wave_incl_scan(v, lane);
    if (lane == 63) wsum[w] = incl;
    __syncthreads();
    T before = 0, tot = 0;
    for (int i = 0; i < kMomThreads / 64; ++i) {
        const T c = wsum[i];
        before += i < w ? c : (T)0;
        tot += c;
    }
    __syncthreads();                    // wsum is reused by the next call
    total = tot;
    return before + incl - v;
}
// Maximum of rows, -1 = none (also in front of the first thread); total = the maximum of all.  wmax: LDS [4]
__device__ __forceinline__ int mom_excl_max(int v, int &total, int *wmax) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    int incl = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int t = __shfl_up(incl, o, 64);
        if (lane >= o) incl = max(incl, t);
    }
    int ex = __shfl_up(incl, 1, 64);
    if (lane == 0) ex = -1;
    if (lane == 63) wmax[w] = incl;
    __syncthreads();
    int before = -1, tot = -1;
    for (int i = 0; i < kMomThreads / 64; ++i) {
        const int c = wmax[i];
        before = i < w ? max(before, c) : before;
        tot = max(tot, c);
    }
    __syncthreads();
    total = tot;
    return max(ex, before);
}

// the hot row r of segment sr, whose prev is the hot row p of segment sp: does r start a moment?
__device__ __forceinline__ bool mom_head(int p, int sp, int r, int sr, int max_gap) { return sp != sr || (int64_t)r - p - 1 > (int64_t)max_gap; }

// Workgroup j: block j % nblk of query q = j / nblk of the chunk; thread t holds rows r0 .. r0 + 15, r0 = B (j % nblk) + 16 t, bit u
// of the result = row r0 + u is hot.  r0 is a multiple of 16, so a thread's rows lie below sstride all or none: every read lies inside
// the query's line of S and inside the table.  A padding row has segment nseg and is never hot
__device__ __forceinline__ uint32_t mom_load(const MomArgs &a, int &q, int64_t &r0, float (&sc)[kMomPerThread], int (&sg)[kMomPerThread]) {
    q = (int)(blockIdx.x / (unsigned)a.nblk);
    r0 = (int64_t)(blockIdx.x % (unsigned)a.nblk) * kMomBlock + (int64_t)threadIdx.x * kMomPerThread;
    if (r0 >= a.sstride) return 0u;
    const float4 *sp = reinterpret_cast<const float4 *>(a.S + (int64_t)q * a.sstride + r0);
    const int4 *gp = reinterpret_cast<const int4 *>(a.rowseg + r0);
    float4 s4[4];
    int4 g4[4];
#pragma unroll
    for (int v = 0; v < 4; ++v) s4[v] = sp[v];
#pragma unroll
    for (int v = 0; v < 4; ++v) g4[v] = gp[v];
    uint32_t hot = 0;
#pragma unroll
    for (int v = 0; v < 4; ++v) {
        sc[4 * v + 0] = s4[v].x, sc[4 * v + 1] = s4[v].y, sc[4 * v + 2] = s4[v].z, sc[4 * v + 3] = s4[v].w;
        sg[4 * v + 0] = g4[v].x, sg[4 * v + 1] = g4[v].y, sg[4 * v + 2] = g4[v].z, sg[4 * v + 3] = g4[v].w;
    }
#pragma unroll
    for (int u = 0; u < kMomPerThread; ++u)
        if (sg[u] >= 0 && sg[u] < a.nseg && sc[u] >= a.threshold) hot |= 1u << u;
    return hot;
}

// The hot rows of a thread in ascending order: f(u, row, head).  p: the prev of the thread's first hot row, -1 for none; what a row
// without prev counts as is the caller's (none_is_head)
template <typename F>
__device__ __forceinline__ void mom_walk(const MomArgs &a, uint32_t hot, int64_t r0, const int (&sg)[kMomPerThread], int p, bool none_is_head,
                                         F &&f) {
    int sp = p >= 0 ? a.rowseg[p] : 0;
#pragma unroll
    for (int u = 0; u < kMomPerThread; ++u) {
        if (!((hot >> u) & 1u)) continue;
        const int r = (int)(r0 + u);
        f(u, r, p < 0 ? none_is_head : mom_head(p, sp, r, sg[u], a.max_gap));
        p = r;
        sp = sg[u];
    }
}

__device__ __forceinline__ int mom_last_hot(uint32_t hot, int64_t r0) { return hot ? (int)r0 + 31 - __clz((int)hot) : -1; }

__global__ __launch_bounds__(kMomThreads) void mom_count_kernel(MomArgs a) {
    __shared__ int wmax[kMomThreads / 64];
    __shared__ uint32_t wsum[kMomThreads / 64];
    int q, blast;
    int64_t r0;
    float sc[kMomPerThread];
    int sg[kMomPerThread];
    const uint32_t hot = mom_load(a, q, r0, sc, sg);
    const int prev = mom_excl_max(mom_last_hot(hot, r0), blast, wmax);
    uint32_t heads = 0, total;
    mom_walk(a, hot, r0, sg, prev, false, [&](int, int, bool head) { heads += head ? 1u : 0u; });
    (void)mom_excl_sum(heads, total, wsum);
    int *out = a.blk + (int64_t)blockIdx.x * 4;
    if (hot && prev < 0) out[0] = (int)r0 + __ffs((int)hot) - 1;         // the one thread that holds the block's first hot row
    if (threadIdx.x == 0) {
        if (blast < 0) out[0] = -1;
        out[1] = blast;
        out[2] = (int)total;
    }
}

// Workgroup q: the nblk summaries of query q of the chunk, kMomThreads at a time with the carries in registers
__global__ __launch_bounds__(kMomThreads) void mom_prefix_kernel(MomArgs a) {
    __shared__ int wmax[kMomThreads / 64];
    __shared__ uint32_t wsum[kMomThreads / 64];
    int4 *blk = reinterpret_cast<int4 *>(a.blk) + (int64_t)blockIdx.x * a.nblk;
    int carry_last = -1;
    uint32_t carry = 0;
    for (int j0 = 0; j0 < a.nblk; j0 += kMomThreads) {
        const int j = j0 + (int)threadIdx.x;
        int4 b = {-1, -1, 0, -1};
        if (j < a.nblk) b = blk[j];
        int tot;
        const int prev = max(mom_excl_max(b.y, tot, wmax), carry_last);
        uint32_t heads = (uint32_t)b.z, t;
        if (b.x >= 0 && (prev < 0 || mom_head(prev, a.rowseg[prev], b.x, a.rowseg[b.x], a.max_gap))) ++heads;
        const uint32_t ex = mom_excl_sum(heads, t, wsum);
        if (j < a.nblk) {
            b.z = (int)(carry + ex);
            b.w = prev;
            blk[j] = b;
        }
        carry_last = max(carry_last, tot);
        carry += t;
    }
    if (threadIdx.x == 0) a.mq[blockIdx.x] = carry;
}

// One workgroup.  mq[0 .. nq): moments per query -> mq[cb + q] = the number of query q's first moment in the chunk; lims[q0 + q] =
// that on top of the running total (tot[0], 0 for the first chunk), lims[q0 + nq] = the new running total.  tot = mq + 2 cb: the
// running total, the total in front of the chunk, the moments of the chunk
__global__ __launch_bounds__(kMomThreads) void mom_lims_kernel(int64_t *__restrict__ mq, int nq, int cb, int64_t q0, int first,
                                                                int64_t *__restrict__ lims) {
    __shared__ int64_t wsum[kMomThreads / 64];
    int64_t *qoff = mq + cb, *tot = mq + 2 * (int64_t)cb;
    const int64_t before = first ? 0 : tot[0];
    __syncthreads();                    // every thread has read the total before thread 0 replaces it
    int64_t run = 0;
    for (int i0 = 0; i0 < nq; i0 += kMomThreads) {
        const int i = i0 + (int)threadIdx.x;
        int64_t t;
        const int64_t ex = mom_excl_sum<int64_t>(i < nq ? mq[i] : 0, t, wsum);
        if (i < nq) {
            qoff[i] = run + ex;
            if (lims) lims[q0 + i] = before + run + ex;
        }
        run += t;
    }
    if (threadIdx.x == 0) {
        if (lims) lims[q0 + nq] = before + run;
        tot[0] = before + run;
        tot[1] = before;
        tot[2] = run;
    }
}

__global__ __launch_bounds__(256) void mom_zero_kernel(MomArgs a) {
    const int64_t n = min(a.mq[2 * (int64_t)a.cb + 2], a.mcap);
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        a.peak[i] = 0;
        a.hi[i] = 0;
        a.cnt[i] = 0;
    }
}

// Slot h of the block = the moment of the hot rows with h heads of the block up to and including them: slot 0 is the moment open on
// entry, slot h >= 1 the h-th moment that starts in the block, T <= B the last.  Moment number in the chunk = base + h - 1.  Slot 0
// has rows only when the block's first hot row is no head; then its prev is a row of the same query and base - 1 a moment of that
// query.  Every global store goes to a moment below mcap (and by the bound in the head of the file every moment lies below it)
__global__ __launch_bounds__(kMomThreads) void mom_write_kernel(MomArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char mom_lds[];
    __shared__ int wmax[kMomThreads / 64];
    __shared__ uint32_t wsum[kMomThreads / 64];
    const int4 b = reinterpret_cast<const int4 *>(a.blk)[blockIdx.x];
    if (b.x < 0) return;                // no hot row in the block: the whole workgroup leaves
    unsigned long long *lpeak = reinterpret_cast<unsigned long long *>(mom_lds);
    int *lhi = reinterpret_cast<int *>(lpeak + kMomBlock + 1), *lcnt = lhi + kMomBlock + 1;
    int q, blast;
    int64_t r0;
    float sc[kMomPerThread];
    int sg[kMomPerThread];
    const uint32_t hot = mom_load(a, q, r0, sc, sg);
    const int64_t base = a.mq[a.cb + q] + b.z;
    int prev = mom_excl_max(mom_last_hot(hot, r0), blast, wmax);
    if (prev < 0) prev = b.w;
    uint32_t heads = 0, T;
    mom_walk(a, hot, r0, sg, prev, true, [&](int, int, bool head) { heads += head ? 1u : 0u; });
    uint32_t h = mom_excl_sum(heads, T, wsum);
    for (uint32_t i = threadIdx.x; i <= T; i += kMomThreads) {
        lpeak[i] = 0;
        lhi[i] = 0;
        lcnt[i] = 0;
    }
    __syncthreads();
    // this thread's rows of the moment in slot h so far
    unsigned long long pk = 0;
    int top = 0, c = 0;
    auto flush = [&]() {
        if (!c) return;
        atomicMax(&lpeak[h], pk);
        atomicMax(&lhi[h], top);
        atomicAdd(&lcnt[h], c);
    };
    mom_walk(a, hot, r0, sg, prev, true, [&](int u, int r, bool head) {
        if (head) {
            flush();
            ++h;
            pk = 0, c = 0;
            if (base + h - 1 < a.mcap) a.lo[base + h - 1] = r;
        }
        const unsigned long long key = ivr_key(sc[u], (uint32_t)r);
        pk = key > pk ? key : pk;
        top = r;
        ++c;
    });
    flush();
    __syncthreads();
    for (uint32_t i = threadIdx.x; i <= T; i += kMomThreads) {
        const int n = lcnt[i];
        const int64_t m = base + i - 1;
        if (!n || m < 0 || m >= a.mcap) continue;
        if (i == 0 || i == T) {         // the moment may hold rows of other blocks
            atomicMax(reinterpret_cast<unsigned long long *>(a.peak + m), lpeak[i]);
            atomicMax(a.hi + m, lhi[i]);
            atomicAdd(a.cnt + m, n);
        } else {                        // it starts behind the block's first row and ends in front of the block's last head
            a.peak[m] = lpeak[i];
            a.hi[m] = lhi[i];
            a.cnt[m] = n;
        }
    }
}

// the range form's tail: moment i of the chunk to position tot[1] + i when that is below cap
__global__ __launch_bounds__(256) void mom_decode_kernel(MomArgs a, const int64_t *__restrict__ ids, float *__restrict__ D, int64_t *__restrict__ I,
                                                         int64_t *__restrict__ Lo, int64_t *__restrict__ Hi, int64_t *__restrict__ Cnt, int64_t cap) {
    const int64_t *tot = a.mq + 2 * (int64_t)a.cb;
    const int64_t n = min(tot[2], a.mcap), before = tot[1];
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n && before + i < cap; i += (int64_t)gridDim.x * 256) {
        const uint64_t key = a.peak[i];
        const int64_t row = (int64_t)(0xFFFFFFFFu - (uint32_t)key), pos = before + i;
        D[pos] = ivr_ord2f((uint32_t)(key >> 32));
        I[pos] = ids ? ids[row] : row;
        Lo[pos] = a.lo[i];
        Hi[pos] = a.hi[i];
        Cnt[pos] = a.cnt[i];
    }
}

struct SrcMoments {    // the rank key of moment i of query q of the chunk; 0 past the query's moments and for a moment below min_count
    const int64_t *mq;
    int cb;
    const uint64_t *peak;
    const int64_t *lo;
    const int *cnt;
    int min_count, rank;
    int64_t n;                   // moments of one query at most
    __device__ uint64_t key(int q, int64_t i) const {
        if (i >= mq[q]) return 0;
        const int64_t m = mq[cb + q] + i;
        const int c = cnt[m];
        if (c < min_count) return 0;
        return rank == IVR_MOMENT_RANK_COUNT ? ((uint64_t)(uint32_t)c << 32) | (uint32_t)(0xFFFFFFFFu - (uint32_t)lo[m]) : peak[m];
    }
};

// Thread i: result slot i of the chunk, query i / k.  rows[i]: the low word of the chosen key, -1 for an unused slot: the peak row of
// the moment (rank peak) or its lo (rank count), either of which lies in [lo, hi] of that moment and of no other
__global__ __launch_bounds__(256) void mom_gather_kernel(MomArgs a, const int64_t *__restrict__ rows, int64_t nslots, int k,
                                                         const int64_t *__restrict__ ids, float *__restrict__ D, int64_t *__restrict__ I,
                                                         int64_t *__restrict__ Lo, int64_t *__restrict__ Hi, int64_t *__restrict__ Cnt) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= nslots) return;
    const int64_t at = rows[i];
    const int q = (int)(i / k);
    const int64_t nm = a.mq[q];
    if (at < 0 || nm <= 0) {
        D[i] = -FLT_MAX;
        I[i] = Lo[i] = Hi[i] = -1;
        Cnt[i] = 0;
        return;
    }
    const int64_t first = a.mq[a.cb + q];
    const int64_t m = first + ivr_last_le(a.lo + first, (int)nm, at);
    const uint64_t key = a.peak[m];
    const int64_t row = (int64_t)(0xFFFFFFFFu - (uint32_t)key);
    D[i] = ivr_ord2f((uint32_t)(key >> 32));
    I[i] = ids ? ids[row] : row;
    Lo[i] = a.lo[m];
    Hi[i] = a.hi[m];
    Cnt[i] = a.cnt[m];
}

// an empty index: every top-k slot unused, every lims entry 0
__global__ __launch_bounds__(256) void mom_absent_kernel(int64_t nsel, float *__restrict__ D, int64_t *__restrict__ I, int64_t *__restrict__ Lo,
                                                         int64_t *__restrict__ Hi, int64_t *__restrict__ Cnt, int64_t nlims,
                                                         int64_t *__restrict__ lims) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < nsel) {
        D[i] = -FLT_MAX;
        I[i] = Lo[i] = Hi[i] = -1;
        Cnt[i] = 0;
    }
    if (i < nlims) lims[i] = 0;
}

struct MomCall {
    const float *q;
    int nq;
    const int64_t *seg_off;
    int nseg;
    float threshold;
    int max_gap;
    int normalize_q;
    // top-k (k > 0): D / I / Lo / Hi / Cnt [nq][k]; range (k == 0): lims [nq + 1], the outputs [cap]
    int k, min_count, rank;
    int64_t *lims;
    float *D;
    int64_t *I, *Lo, *Hi, *Cnt;
    int64_t cap;
};

int mom_check(const char *what, ivr_index *x, const MomCall &a) {
    IVR_REQUIRE(x && a.q && a.D && a.I && a.Lo && a.Hi && a.Cnt, "%s: NULL argument", what);
    IVR_REQUIRE(a.nq >= 1, "%s: nq=%d < 1", what, a.nq);
    IVR_REQUIRE(!a.seg_off || a.nseg >= 1, "%s: nseg=%d with seg_off", what, a.nseg);
    IVR_REQUIRE(!(a.threshold != a.threshold), "%s: threshold is NaN", what);
    IVR_REQUIRE(a.max_gap >= 0 && a.max_gap <= 0x7FFFFFFE, "%s: max_gap=%d outside [0,2^31-2]", what, a.max_gap);
    return IVR_OK;
}

// both entry points once their arguments are checked; the caller holds x->mu
int mom_search(const char *what, ivr_index *x, const MomCall &a, hipStream_t s) {
    IVR_REQUIRE(x->ntotal < (1ll << 31), "%s: ntotal=%lld >= 2^31", what, (long long)x->ntotal);
    const int64_t n = x->ntotal;
    if (n == 0) {
        const int64_t nsel = a.k ? (int64_t)a.nq * a.k : 0, nlims = a.k ? 0 : (int64_t)a.nq + 1;
        hipLaunchKernelGGL(mom_absent_kernel, dim3((unsigned)ivr_ceil_div(std::max(nsel, nlims), 256)), dim3(256), 0, s, nsel, a.D, a.I, a.Lo, a.Hi,
                           a.Cnt, nlims, a.lims);
        IVR_LAUNCH_CHECK();
        return IVR_OK;
    }
    const int nseg = a.seg_off ? a.nseg : 1;
    const int64_t sstride = ivr_ceil_div(n, 16) * 16;
    const int nblk = (int)ivr_ceil_div(n, kMomBlock);
    const int64_t maxm = std::min<int64_t>(n, n / ((int64_t)a.max_gap + 2) + nseg);          // moments of one query at most
    // queries per chunk, in whole 16-query tiles: S within the slot budget
    int64_t cb = std::min<int64_t>({ivr_round_up(a.nq, 16), x->seq_chunk_slots / n, (int64_t)kMomMaxChunk});
    cb = std::max<int64_t>(16, cb / 16 * 16);
    const int64_t mcap = cb * maxm;
    int rc = ivr_reserve_queries(x, (int)ivr_ceil_div(a.nq, 16));
    // each buffer grows on its own: calls of different shapes must not shrink one another's scratch
    if (rc == IVR_OK) rc = ivr_reserve({{&x->seq_scores, (size_t)cb * sstride * 4}});
    if (rc == IVR_OK) rc = ivr_reserve({{&x->mo_blk, (size_t)cb * nblk * 16}});
    if (rc == IVR_OK) rc = ivr_reserve({{&x->mo_q, (size_t)(2 * cb + 3) * 8}});
    if (rc == IVR_OK) rc = ivr_reserve({{&x->mo_mom, (size_t)mcap * 24}});
    if (rc == IVR_OK && a.k) rc = ivr_reserve({{&x->mo_rows, (size_t)cb * a.k * 12}});
    if (rc == IVR_OK) rc = ivr_func_max_lds(reinterpret_cast<const void *>(mom_write_kernel), (int)kMomLds);
    if (rc != IVR_OK) return rc;
    rc = ivr_launch_tile_rows(x, x->qtiled, a.q, 0, a.nq, a.normalize_q, nullptr, s);
    if (rc == IVR_OK) rc = ivr_launch_rowseg(x, a.seg_off, nseg, s);
    if (rc != IVR_OK) return rc;
    const int64_t *ids = x->has_ids ? x->ids : nullptr;
    uint64_t *peak = x->mo_mom;
    int64_t *lo = reinterpret_cast<int64_t *>(peak + mcap);
    int *hi = reinterpret_cast<int *>(lo + mcap);
    const MomArgs m{x->seq_scores, sstride, x->gr_seg, nseg, a.threshold, a.max_gap, nblk, x->mo_blk, x->mo_q, (int)cb, mcap, peak, lo, hi, hi + mcap};
    const unsigned fill = (unsigned)std::min<int64_t>(kMomFillBlocks, ivr_ceil_div(mcap, 256));
    for (int b0 = 0; b0 < a.nq; b0 += (int)cb) {
        const int cnt = (int)std::min<int64_t>(cb, a.nq - b0);
        rc = ivr_launch_seq_score(x, b0 >> 4, (int)ivr_ceil_div(cnt, 16), s);
        if (rc != IVR_OK) return rc;
        const unsigned grid = (unsigned)((int64_t)cnt * nblk);
        {
            // bytes the run passes move per (query, row): S and the table, twice
            IvrProf prof("mom_runs", s, (double)cnt * n * 16.0);
            hipLaunchKernelGGL(mom_count_kernel, dim3(grid), dim3(kMomThreads), 0, s, m);
            hipLaunchKernelGGL(mom_prefix_kernel, dim3((unsigned)cnt), dim3(kMomThreads), 0, s, m);
            hipLaunchKernelGGL(mom_lims_kernel, dim3(1), dim3(kMomThreads), 0, s, m.mq, cnt, (int)cb, (int64_t)b0, b0 == 0 ? 1 : 0, a.k ? nullptr : a.lims);
            hipLaunchKernelGGL(mom_zero_kernel, dim3(fill), dim3(256), 0, s, m);
            hipLaunchKernelGGL(mom_write_kernel, dim3(grid), dim3(kMomThreads), kMomLds, s, m);
            IVR_LAUNCH_CHECK();
        }
        IvrProf prof("mom_tail", s, (double)cnt * maxm * 8, true);
        if (a.k) {
            int64_t *rows = x->mo_rows;
            const int64_t nslots = (int64_t)cnt * a.k, o = (int64_t)b0 * a.k;
            launch_select<OUT_DI>(SrcMoments{m.mq, (int)cb, peak, lo, m.cnt, a.min_count, a.rank, maxm}, cnt, a.k,
                                  SelectOut::to_rows(reinterpret_cast<float *>(rows + cb * a.k), rows), s);
            hipLaunchKernelGGL(mom_gather_kernel, dim3((unsigned)ivr_ceil_div(nslots, 256)), dim3(256), 0, s, m, (const int64_t *)rows, nslots, a.k, ids,
                               a.D + o, a.I + o, a.Lo + o, a.Hi + o, a.Cnt + o);
        } else {
            hipLaunchKernelGGL(mom_decode_kernel, dim3(fill), dim3(256), 0, s, m, ids, a.D, a.I, a.Lo, a.Hi, a.Cnt, a.cap);
        }
        IVR_LAUNCH_CHECK();
    }
    return IVR_OK;
}

}  // namespace

extern "C" {

int ivr_moment_block_rows(void) { return kMomBlock; }

int ivr_index_search_moments(ivr_index *x, const float *q, int nq, const int64_t *seg_off, int nseg, float threshold, int max_gap, int min_count,
                             int rank, int k, int normalize_q, float *D, int64_t *I, int64_t *Lo, int64_t *Hi, int64_t *Cnt, ivr_stream stream) {
    const char *what = "ivr_index_search_moments";
    const MomCall a{q, nq, seg_off, nseg, threshold, max_gap, normalize_q, k, min_count, rank, nullptr, D, I, Lo, Hi, Cnt, 0};
    const int rc = mom_check(what, x, a);
    if (rc != IVR_OK) return rc;
    IVR_REQUIRE(min_count >= 1, "%s: min_count=%d < 1", what, min_count);
    IVR_REQUIRE(rank == IVR_MOMENT_RANK_PEAK || rank == IVR_MOMENT_RANK_COUNT, "%s: rank=%d is neither IVR_MOMENT_RANK_PEAK nor IVR_MOMENT_RANK_COUNT",
                what, rank);
    IVR_REQUIRE(k >= 1 && k <= IVR_MAX_K, "%s: k=%d outside [1,%d]", what, k, IVR_MAX_K);
    std::lock_guard<std::mutex> lk(x->mu);
    IVR_HIP(hipSetDevice(x->ctx->device));
    return mom_search(what, x, a, (hipStream_t)stream);
}

int ivr_index_range_search_moments(ivr_index *x, const float *q, int nq, const int64_t *seg_off, int nseg, float threshold, int max_gap,
                                   int normalize_q, int64_t *lims, float *D, int64_t *I, int64_t *Lo, int64_t *Hi, int64_t *Cnt, int64_t cap,
                                   ivr_stream stream) {
    const char *what = "ivr_index_range_search_moments";
    const MomCall a{q, nq, seg_off, nseg, threshold, max_gap, normalize_q, 0, 1, IVR_MOMENT_RANK_PEAK, lims, D, I, Lo, Hi, Cnt, cap};
    const int rc = mom_check(what, x, a);
    if (rc != IVR_OK) return rc;
    IVR_REQUIRE(lims, "%s: NULL argument", what);
    IVR_REQUIRE(cap >= 0, "%s: cap=%lld < 0", what, (long long)cap);
    std::lock_guard<std::mutex> lk(x->mu);
    IVR_HIP(hipSetDevice(x->ctx->device));
    return mom_search(what, x, a, (hipStream_t)stream);
}

}  // extern "C"
