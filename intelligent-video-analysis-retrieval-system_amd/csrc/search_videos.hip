// Video search over the flat index (ivr_index_video_scores, ivr_index_video_search): stored videos (the segments of seg_off) ranked
// against SETS of query vectors, by the two-sided reduction of the frame score matrix that vector stores ship for multi-vector
// documents as MaxSim / Chamfer similarity.  The first member of the seg_off family with several vectors on both sides: query by
// whole video, "contains all of these sub-queries", and the related-videos list.  DESIGN.md section 4, "video search".
//
// Frame score S[i, r] = <query member i, stored row r>, accumulated by stream_tile / mfma_chunk4: the accumulation order of every
// float32 score of the index (search_internal.h), so it has the bits ivr_index_search reports for that pair; -0.0 counts as +0.0.
//   set s       the members [set_off[s], set_off[s + 1]) of q, m_s >= 1
//   video j     the rows [seg_off[j], seg_off[j + 1]) clipped to the stored rows, n_j of them
//   fix(t)      int64(rint(t 2^24)): the fixed point of the tagging masses; t 2^24 is exact in float32
//   Fsum[s, j]  the sum over the members i of s of fix(max over the rows r of j of S[i, r])      every query frame finds its best match
//   Bsum[s, j]  the sum over the rows r of j of fix(max over the members i of s of S[i, r])      every stored frame finds its best match
//   V[s, j]     forward float(F64), backward float(B64), symmetric float((F64 + B64) 0.5), with F64 = double(Fsum) / (m_s 2^24) and
//               B64 = double(Bsum) / (n_j 2^24); -FLT_MAX for an empty video, which is never ranked
//
// Launches, all on the caller's stream; set_off is read back once before the first of them (the one host round trip of a call):
//   tile_rows     the members -> vid_pack in the tiled query layout, normalised as the queries of a search are
//   vid_tables    member, tile and block offsets of every set: a set starts on a tile boundary of the tiled buffer and on a block
//                 boundary of the grid, so a 16-member tile and a workgroup belong to one set
//   vid_retile    vid_pack -> vid_q, every set from a tile boundary on; the padding columns are zero and masked by number below
//   grp_rowseg    the segment number of every stored row (search_groups.hip)
//   per chunk of sets:
//   vid_score     THE HOT PATH, in the shape of the self-join frame: a workgroup stages a block of up to four 16-member tiles of one
//                 set in LDS and streams a piece of 128 stored 16-row tiles past it, a run of 16 tiles per wave.  No score is written;
//                 both reductions are fed from the same accumulators:
//                   per member   the maximum per (member, video) as grp_segbest takes it: a running ordered score per lane while the
//                                wave's tiles stay inside one video, a fold of the four lanes of a column when the video changes, one
//                                32-bit atomicMax per (column, video run, wave) into fmax[member][video]
//                   per row      the maximum over the members of the block: the query tiles folded in registers, then the 16 lanes of
//                                a row.  A set that fits one block stores it plainly into bmax[set][row]; a larger set issues one
//                                32-bit atomicMax per (row, block)
//   vid_reduce_f  Fsum: a thread per video adds fix of the maxima of up to 64 members (one block of the set): one 64-bit integer
//                 atomicAdd per (set, video, block of members)
//   vid_reduce_b  Bsum: a workgroup takes 1,024 rows of one set, four adjacent rows per thread; rows of one video are added up per
//                 thread, per wave when the wave lies inside one video, then per workgroup in LDS: one 64-bit integer atomicAdd per
//                 (set, video touched, workgroup)
//   vid_finish    V in float64 as defined, and the 64-bit keys (ordered V, ~video); 0 for an empty or excluded video
//   select        select_topk_kernel (search_select.h) over the keys of a set
//
// Why the result is the same on every run: fmax and bmax only ever receive maxima, and a maximum does not depend on the order in
// which its operands arrive; Fsum and Bsum are integer sums, which do not either.  No float is ever added by an atomic.
//
// Scratch on the index, grow-only, each buffer on its own: 4 bytes per (member of a chunk, video), 4 bytes per (set of a chunk, stored
// row rounded up to 16), 24 bytes per (set of a chunk, video), the two query buffers and 12 bytes per set.  A chunk holds as many
// whole sets as keep each of the three tables within IVR_SEQ_CHUNK_SLOTS slots, one set at least.
#include <climits>
#include <vector>

#include "ivr_common.h"
#include "search_internal.h"
#include "search_select.h"

namespace {

constexpr int kViWaves = 8;              // waves of a score workgroup: two per SIMD, as the self-join frame
constexpr int kViRun = 16;               // stored 16-row tiles of one wave's run
constexpr int kViPiece = kViWaves * kViRun;      // stored tiles of one workgroup
constexpr int kViReduceRows = 1024;      // rows of one workgroup of the backward reduction: four per thread

struct ViTables {
    const int *moff, *toff, *boff;       // [nsets + 1] each: members, 16-member tiles and blocks in front of every set
};

// the last i in [0, n) with off[i] <= v (off ascending, off[0] <= v)
__device__ __forceinline__ int vid_last_le(const int *off, int n, int v) {
    int lo = 0, hi = n - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (off[mid] <= v) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// One workgroup of 1,024 threads: thread i takes a run of sets, the runs are scanned through LDS.  set_off == NULL: one set of nq
// members.  bt: tiles of a block
__global__ __launch_bounds__(1024) void vid_tables_kernel(const int64_t *__restrict__ set_off, int nsets, int nq, int bt, int *__restrict__ moff,
                                                          int *__restrict__ toff, int *__restrict__ boff) {
    __shared__ int st[1024], sb[1024];
    const int per = (nsets + 1023) / 1024;
    const int s0 = min(nsets, (int)threadIdx.x * per), s1 = min(nsets, s0 + per);
    auto off = [&](int s) { return set_off ? (int)set_off[s] : (s ? nq : 0); };
    int t = 0, b = 0;
    for (int s = s0; s < s1; ++s) {
        const int tiles = (off(s + 1) - off(s) + 15) >> 4;
        t += tiles;
        b += (tiles + bt - 1) / bt;
    }
    st[threadIdx.x] = t;
    sb[threadIdx.x] = b;
    __syncthreads();
    if (threadIdx.x == 0) {
        int at = 0, ab = 0;
        for (int i = 0; i < 1024; ++i) {
            const int vt = st[i], vb = sb[i];
            st[i] = at, sb[i] = ab;
            at += vt, ab += vb;
        }
    }
    __syncthreads();
    t = st[threadIdx.x], b = sb[threadIdx.x];
    for (int s = s0; s < s1; ++s) {
        moff[s] = off(s), toff[s] = t, boff[s] = b;
        const int tiles = (off(s + 1) - off(s) + 15) >> 4;
        t += tiles;
        b += (tiles + bt - 1) / bt;
    }
    // the last thread's run ends the sets (1024 per >= nsets), whether it holds a set or not: its prefix is the total
    if (threadIdx.x == 1023) moff[nsets] = off(nsets), toff[nsets] = t, boff[nsets] = b;
}

// Wave w: tile w of the set-aligned buffer, copied float4 by float4 from the packed tiles.  Column c of tile toff[s] + k is member
// moff[s] + 16 k + c = that row of q; a column past the set's last member is zero
__global__ __launch_bounds__(256) void vid_retile_kernel(const float4 *__restrict__ pack, float4 *__restrict__ dst, ViTables tb, int nsets, int dp4) {
    const int tile = (int)blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (tile >= tb.toff[nsets]) return;
    const int s = vid_last_le(tb.toff, nsets + 1, tile);                 // sets are not empty: toff ascends strictly, so s < nsets
    const int mem = tb.moff[s] + (tile - tb.toff[s]) * 16 + (lane & 15);
    const bool valid = mem < tb.moff[s + 1];
    const int src = valid ? mem : 0;                                     // a row of q in every lane: no branch around the load
    const float4 *from = pack + (int64_t)(src >> 4) * dp4 * 16 + (lane >> 4) * 16 + (src & 15);
    float4 *to = dst + (int64_t)tile * dp4 * 16 + lane;
    for (int kc = 0; kc < (dp4 >> 2); ++kc) {
        const float4 v = from[kc * 64];
        to[kc * 64] = valid ? v : make_float4(0.f, 0.f, 0.f, 0.f);
    }
}

struct ViScore {
    const float4 *data;          // the float32 tiles of the storage
    const float4 *qt;            // the set-aligned query tiles of the whole call
    int dp4;
    int bt;                      // tiles of a block, at most 4
    int64_t ntiles;              // 16-row tiles that hold stored rows
    const int *rowseg;           // [16 ntiles], ascending
    int nseg, nsets;
    ViTables tb;
    int s0, b0, nb;              // the chunk: its first set, its first block and its blocks
    int do_f, do_b;              // which reductions the mode reads
    uint32_t *fmax;              // [members of the chunk][nseg]: the greatest ordered score, 0 = no row
    uint32_t *bmax;              // [sets of the chunk][16 ntiles]
};

__device__ __forceinline__ uint32_t vid_umax(uint32_t a, uint32_t b) { return a > b ? a : b; }
// the maximum over the four lanes (quad rows) that hold one member column
__device__ __forceinline__ uint32_t vid_fold_column(uint32_t v) {
    v = vid_umax(v, (uint32_t)__shfl_xor(v, 16, 64));
    return vid_umax(v, (uint32_t)__shfl_xor(v, 32, 64));
}
// the maximum over the 16 lanes (member columns) that hold one stored row
__device__ __forceinline__ uint32_t vid_fold_row(uint32_t v) {
    v = vid_umax(v, (uint32_t)__shfl_xor(v, 1, 64));
    v = vid_umax(v, (uint32_t)__shfl_xor(v, 2, 64));
    v = vid_umax(v, (uint32_t)__shfl_xor(v, 4, 64));
    return vid_umax(v, (uint32_t)__shfl_xor(v, 8, 64));
}

// Workgroup x: block b = b0 + x % nb of the chunk against the row tiles of piece x / nb, wave w its tiles 16 w .. 16 w + 15.  Every
// tile read lies inside the storage's allocation (capacity a multiple of 64 rows >= ntotal), every rowseg read below 16 ntiles.  An
// atomic or store goes to fmax[member][sg] with a member of the chunk and 0 <= sg < nseg, and to bmax[set][row] with a row whose
// segment is in [0, nseg), so row < ntotal.  The segment variables (cur_sg, first, last, sg) are the same in every lane of a wave, qn
// and single in every lane of the workgroup: every shuffle below is reached by whole waves.
__global__ __launch_bounds__(64 * kViWaves) void vid_score_kernel(ViScore a) {
    extern __shared__ __attribute__((aligned(16))) float4 qs[];
    const int per_tile = a.dp4 * 16, kchunks = a.dp4 >> 2;
    const int b = a.b0 + (int)(blockIdx.x % a.nb);
    const int64_t piece = blockIdx.x / a.nb;
    const int s = vid_last_le(a.tb.boff, a.nsets + 1, b);                 // boff ascends strictly: s < nsets
    const int kb = b - a.tb.boff[s];
    const int tile0 = a.tb.toff[s] + kb * a.bt, qn = min(a.bt, a.tb.toff[s + 1] - tile0);
    const bool single = a.tb.boff[s + 1] - a.tb.boff[s] == 1;
    {
        const float4 *src = a.qt + (int64_t)tile0 * per_tile;
        for (int i = threadIdx.x; i < qn * per_tile; i += blockDim.x) qs[i] = src[i];
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, h = lane >> 4, c = lane & 15;
    const int m0 = a.tb.moff[s] + (kb * a.bt) * 16 + c, mend = a.tb.moff[s + 1], mchunk = a.tb.moff[a.s0];
    bool valid[4];
    uint32_t *fm[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        valid[q] = q < qn && m0 + 16 * q < mend;
        fm[q] = a.fmax + (int64_t)(valid[q] ? m0 + 16 * q - mchunk : 0) * a.nseg;
    }
    uint32_t *bm = a.bmax + (int64_t)(s - a.s0) * a.ntiles * 16;
    const int64_t t0 = piece * kViPiece + (int64_t)wave * kViRun, t1 = min(t0 + kViRun, a.ntiles);
    int cur_sg = -1;             // the video the running maxima belong to; outside [0, nseg): none
    uint32_t cur[4] = {0, 0, 0, 0};
    auto flush = [&](int sg, const uint32_t (&v)[4]) {
        if (sg < 0 || sg >= a.nseg) return;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            if (q >= qn) break;
            const uint32_t f = vid_fold_column(v[q]);
            if (h == 0 && valid[q] && f) atomicMax(fm[q] + sg, f);
        }
    };
    for (int64_t t = t0; t < t1; ++t) {
        f32x4 acc[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) acc[q] = f32x4{0.f, 0.f, 0.f, 0.f};
        stream_tile<4>(a.data + t * per_tile + lane, kchunks, [&](int q, int kc, const float4 &av) {
            if (q < qn) mfma_chunk4(acc[q], av, qs[q * per_tile + kc * 64 + lane]);
        });
        // acc[q][r] = <row 16 t + 4 h + r, member column c of query tile q>
        const int4 sg4 = *reinterpret_cast<const int4 *>(a.rowseg + t * 16 + h * 4);
        const int sgr[4] = {sg4.x, sg4.y, sg4.z, sg4.w};
        uint32_t key[4][4];
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
            for (int r = 0; r < 4; ++r) key[q][r] = valid[q] ? ivr_f2ord(acc[q][r]) : 0u;
        if (a.do_b) {
            uint32_t out = 0;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const uint32_t v = vid_fold_row(vid_umax(vid_umax(key[0][r], key[1][r]), vid_umax(key[2][r], key[3][r])));
                out = (c & 3) == r ? v : out;
            }
            // lane c < 4 of quad row h writes row 16 t + 4 h + c
            int sg = sgr[0];
#pragma unroll
            for (int r = 1; r < 4; ++r) sg = (c & 3) == r ? sgr[r] : sg;
            if (c < 4 && sg >= 0 && sg < a.nseg) {
                uint32_t *p = bm + t * 16 + h * 4 + c;
                if (single) *p = out;
                else if (out) atomicMax(p, out);
            }
        }
        if (!a.do_f) continue;
        const int first = __builtin_amdgcn_readlane(sg4.x, 0), last = __builtin_amdgcn_readlane(sg4.w, 48);
        if (first != cur_sg) {
            flush(cur_sg, cur);
#pragma unroll
            for (int q = 0; q < 4; ++q) cur[q] = 0;
        }
        // the videos of the tile in front of its last one, each folded on its own; the running maxima belong to the first of them
        for (int sg = first; sg != last;) {
            uint32_t v[4];
            int nx = last;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                v[q] = cur[q];
                cur[q] = 0;
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    if (sgr[r] == sg) v[q] = vid_umax(v[q], key[q][r]);
            }
#pragma unroll
            for (int r = 0; r < 4; ++r)
                if (sgr[r] > sg) nx = min(nx, sgr[r]);
            flush(sg, v);
            nx = min(nx, __shfl_xor(nx, 16, 64));
            nx = min(nx, __shfl_xor(nx, 32, 64));
            sg = __builtin_amdgcn_readfirstlane(nx);         // ascending and <= last: the loop ends
        }
        // the tile's last video (the only one of a tile inside one video) runs on
        cur_sg = last;
        if (last >= 0 && last < a.nseg) {
#pragma unroll
            for (int q = 0; q < 4; ++q)
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    if (sgr[r] == last) cur[q] = vid_umax(cur[q], key[q][r]);
        }
    }
    if (a.do_f) flush(cur_sg, cur);
}

// fix of an ordered score; t 2^24 is exact in float32 and, for |t| <= 256, below 2^33
__device__ __forceinline__ long long vid_fix(uint32_t ord) { return (long long)rintf(ivr_ord2f(ord) * 16777216.f); }

struct ViReduce {
    ViTables tb;
    int nsets, nseg;
    int s0, b0;                  // the chunk's first set and first block
    int bt;
    int64_t nrows;               // stored rows rounded up to 16
    const int *rowseg;
    const uint32_t *fmax, *bmax;
    unsigned long long *fsum, *bsum;     // [sets of the chunk][nseg], zeroed
};

// Workgroup y xb + x (xb = ceil(nseg / 256)): videos 256 x .. 256 x + 255 for block y of the chunk = up to 16 bt members of one set; thread j reads one word
// of every member's line, coalesced across the workgroup
__global__ __launch_bounds__(256) void vid_reduce_f_kernel(ViReduce a) {
    const int xb = (a.nseg + 255) >> 8;
    const int j = (int)(blockIdx.x % xb) * 256 + threadIdx.x;
    if (j >= a.nseg) return;
    const int b = a.b0 + (int)(blockIdx.x / xb);
    const int s = vid_last_le(a.tb.boff, a.nsets + 1, b);
    const int m0 = a.tb.moff[s] + (b - a.tb.boff[s]) * a.bt * 16, m1 = min(m0 + a.bt * 16, a.tb.moff[s + 1]);
    const uint32_t *f = a.fmax + (int64_t)(m0 - a.tb.moff[a.s0]) * a.nseg + j;
    long long sum = 0;
    bool any = false;
    for (int i = 0; i < m1 - m0; ++i) {
        const uint32_t o = f[(int64_t)i * a.nseg];
        if (o) sum += vid_fix(o), any = true;
    }
    if (any) atomicAdd(a.fsum + (int64_t)(s - a.s0) * a.nseg + j, (unsigned long long)sum);
}

// Workgroup y xb + x (xb = ceil(nrows / 1024)): rows 1024 x .. 1024 x + 1023 of set y of the chunk, thread i its rows 4 i .. 4 i + 3.
// The segment table ascends, so the videos of the workgroup are first .. last and a video's slot in the LDS table is its distance
// from first: below 1,024 unless empty videos lie in between.  Integer adds only
__global__ __launch_bounds__(256) void vid_reduce_b_kernel(ViReduce a) {
    __shared__ unsigned long long part[kViReduceRows];
    __shared__ int s_first;
    const int xb = (int)((a.nrows + kViReduceRows - 1) / kViReduceRows), y = (int)(blockIdx.x / xb);
    const int64_t r0 = (int64_t)(blockIdx.x % xb) * kViReduceRows + threadIdx.x * 4;
    for (int i = threadIdx.x; i < kViReduceRows; i += 256) part[i] = 0;
    int sg[4] = {INT_MAX, INT_MAX, INT_MAX, INT_MAX};
    uint32_t o[4] = {0, 0, 0, 0};
    if (r0 < a.nrows) {                              // nrows is a multiple of 16: the four rows are inside both tables
        const int4 s4 = *reinterpret_cast<const int4 *>(a.rowseg + r0);
        const uint4 o4 = *reinterpret_cast<const uint4 *>(a.bmax + (int64_t)y * a.nrows + r0);
        sg[0] = s4.x, sg[1] = s4.y, sg[2] = s4.z, sg[3] = s4.w;
        o[0] = o4.x, o[1] = o4.y, o[2] = o4.z, o[3] = o4.w;
    }
    if (threadIdx.x == 0) s_first = sg[0];           // the workgroup's first row exists: the grid covers nrows
    __syncthreads();
    const int first = s_first;
    unsigned long long *out = a.bsum + (int64_t)y * a.nseg;
    // this thread's rows video by video: the rows of one video are adjacent
    long long sum = 0;
    int cur = INT_MAX;
    bool any = false;
    auto put = [&](int v, long long x) {
        if (v < 0 || v >= a.nseg) return;
        const int64_t slot = (int64_t)v - first;
        // empty videos in between can put a video's number 1,024 or more past the first: its rows go to the sums directly
        if (slot >= 0 && slot < kViReduceRows) atomicAdd(part + slot, (unsigned long long)x);
        else atomicAdd(out + v, (unsigned long long)x);
    };
    const int wfirst = __shfl(sg[0], 0, 64), wlast = __shfl(sg[3], 63, 64);
    const bool whole = wfirst == wlast && wfirst >= 0 && wfirst < a.nseg;        // the wave lies inside one video: the same in every lane
    if (whole) {
#pragma unroll
        for (int r = 0; r < 4; ++r)
            if (o[r]) sum += vid_fix(o[r]);
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) sum += __shfl_xor(sum, off, 64);
        if ((threadIdx.x & 63) == 0 && sum) put(wfirst, sum);
    } else {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            if (sg[r] != cur) {
                if (any) put(cur, sum);
                cur = sg[r], sum = 0, any = false;
            }
            if (o[r] && sg[r] >= 0 && sg[r] < a.nseg) sum += vid_fix(o[r]), any = true;
        }
        if (any) put(cur, sum);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < kViReduceRows; i += 256) {
        const unsigned long long v = part[i];
        const int64_t sg = (int64_t)first + i;
        if (v && sg >= 0 && sg < a.nseg) atomicAdd(out + sg, v);
    }
}

struct ViFinish {
    ViTables tb;
    int s0, cnt;                 // the sets of the chunk
    int nseg, n, mode;
    const int64_t *seg_off;
    const unsigned long long *fsum, *bsum;
    const int64_t *exclude;      // [sets of the call] or NULL
    float *V;                    // [sets of the chunk][nseg] or NULL
    uint64_t *keys;              // [sets of the chunk][nseg] or NULL
};

// Thread i: (set, video) i of the chunk
__global__ __launch_bounds__(256) void vid_finish_kernel(ViFinish a) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (int64_t)a.cnt * a.nseg) return;
    const int sc = (int)(i / a.nseg), j = (int)(i % a.nseg), s = a.s0 + sc;
    int64_t lo = 0, hi = a.n;
    if (a.seg_off) {
        lo = min(max(a.seg_off[j], (int64_t)0), (int64_t)a.n);
        hi = min(max(a.seg_off[j + 1], (int64_t)0), (int64_t)a.n);
    }
    const int64_t nj = hi - lo;
    float v = -FLT_MAX;
    if (nj > 0) {
        const int m = a.tb.moff[s + 1] - a.tb.moff[s];
        const double f = (double)(long long)a.fsum[i] / ((double)m * 16777216.0);
        const double b = (double)(long long)a.bsum[i] / ((double)nj * 16777216.0);
        v = a.mode == IVR_VIDEO_FORWARD ? (float)f : a.mode == IVR_VIDEO_BACKWARD ? (float)b : (float)((f + b) * 0.5);
    }
    if (a.V) a.V[i] = v;
    if (a.keys) a.keys[i] = nj > 0 && !(a.exclude && a.exclude[s] == j) ? ivr_key(v, (uint32_t)j) : 0;
}

struct SrcVideoKeys {  // the video keys of set q of the chunk, every one written (0 = empty or excluded)
    const uint64_t *keys;
    int64_t n;
    __device__ uint64_t key(int q, int64_t i) const { return keys[(int64_t)q * n + i]; }
};

// an empty index: every video is empty
__global__ __launch_bounds__(256) void vid_absent_kernel(int64_t nV, float *__restrict__ V, int64_t nD, float *__restrict__ D, int64_t *__restrict__ I) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (V && i < nV) V[i] = -FLT_MAX;
    if (D && i < nD) {
        D[i] = -FLT_MAX;
        I[i] = -1;
    }
}

struct ViArgs {
    const float *q;
    int nq;
    const int64_t *set_off;
    int nsets;
    const int64_t *seg_off;
    int nseg;
    int mode, normalize_q;
    int k;                       // 0: the scores of every video
    const int64_t *exclude;
    float *V;
    int64_t *Vseg;
    float *D;
};

// both entry points once their arguments are checked; the caller holds x->mu
int vid_search(const char *what, ivr_index *x, const ViArgs &a, hipStream_t s) {
    IVR_REQUIRE(x->ntotal < (1ll << 31), "%s: ntotal=%lld >= 2^31", what, (long long)x->ntotal);
    const int n = (int)x->ntotal, nseg = a.seg_off ? a.nseg : 1, nsets = a.set_off ? a.nsets : 1;
    // the sets, read back once: everything below is planned from them
    std::vector<int64_t> off(nsets + 1);
    if (a.set_off) {
        IVR_HIP(hipMemcpyAsync(off.data(), a.set_off, (size_t)(nsets + 1) * sizeof(int64_t), hipMemcpyDeviceToHost, s));
        IVR_HIP(hipStreamSynchronize(s));
    } else {
        off[0] = 0, off[1] = a.nq;
    }
    IVR_REQUIRE(off[0] >= 0 && off[nsets] <= a.nq, "%s: set_off [%lld,%lld] outside the %d members", what, (long long)off[0], (long long)off[nsets],
                a.nq);
    for (int i = 0; i < nsets; ++i) {
        IVR_REQUIRE(off[i + 1] >= off[i], "%s: set_off must ascend, got set_off[%d]=%lld > set_off[%d]=%lld", what, i, (long long)off[i], i + 1,
                    (long long)off[i + 1]);
        IVR_REQUIRE(off[i + 1] > off[i], "%s: set %d is empty", what, i);
        IVR_REQUIRE(off[i + 1] - off[i] <= IVR_VIDEO_MAX_MEMBERS, "%s: set %d has %lld members > %d", what, i, (long long)(off[i + 1] - off[i]),
                    IVR_VIDEO_MAX_MEMBERS);
    }
    if (n == 0) {
        const int64_t nV = a.k ? 0 : (int64_t)nsets * nseg, nD = (int64_t)nsets * a.k;
        hipLaunchKernelGGL(vid_absent_kernel, dim3((unsigned)ivr_ceil_div(std::max(nV, nD), 256)), dim3(256), 0, s, nV, a.V, nD, a.D, a.Vseg);
        IVR_LAUNCH_CHECK();
        return IVR_OK;
    }
    const int bt = x->qt_max();                                           // tiles of a block
    const int64_t ntiles = ivr_ceil_div(n, 16), nrows = ntiles * 16, pieces = ivr_ceil_div(ntiles, kViPiece);
    // host copies of what vid_tables computes
    std::vector<int> toff(nsets + 1), boff(nsets + 1);
    toff[0] = boff[0] = 0;
    for (int i = 0; i < nsets; ++i) {
        const int tiles = (int)ivr_ceil_div(off[i + 1] - off[i], 16);
        toff[i + 1] = toff[i] + tiles;
        boff[i + 1] = boff[i] + (int)ivr_ceil_div(tiles, bt);
    }
    // the chunks: whole sets, each table within the slot budget, one set at least
    const int64_t budget = x->seq_chunk_slots;
    std::vector<int> cuts{0};
    int64_t max_mem = 0, max_sets = 0;
    for (int i = 0; i < nsets;) {
        int e = i + 1;
        while (e < nsets && (off[e + 1] - off[i]) * nseg <= budget && (int64_t)(e + 1 - i) * nrows <= budget && (int64_t)(e + 1 - i) * nseg <= budget) ++e;
        max_mem = std::max<int64_t>(max_mem, off[e] - off[i]);
        max_sets = std::max<int64_t>(max_sets, e - i);
        IVR_REQUIRE((int64_t)(boff[e] - boff[i]) * pieces < (1ll << 31), "%s: %lld blocks x %lld pieces of rows >= 2^31", what,
                    (long long)(boff[e] - boff[i]), (long long)pieces);
        IVR_REQUIRE(ivr_ceil_div(nseg, 256) * (boff[e] - boff[i]) < (1ll << 31) && ivr_ceil_div(nrows, kViReduceRows) * (e - i) < (1ll << 31),
                    "%s: the reductions of %d sets over %d videos and %lld rows need >= 2^31 workgroups", what, e - i, nseg, (long long)nrows);
        cuts.push_back(e);
        i = e;
    }
    const bool do_f = a.mode != IVR_VIDEO_BACKWARD, do_b = a.mode != IVR_VIDEO_FORWARD;
    // each buffer grows on its own: calls of different shapes must not shrink one another's scratch
    int rc = ivr_reserve({{&x->vi_pack, (size_t)ivr_round_up(a.nq, 16) * x->dp * 4}});
    if (rc == IVR_OK) rc = ivr_reserve({{&x->vi_q, (size_t)toff[nsets] * 16 * x->dp * 4}});
    if (rc == IVR_OK) rc = ivr_reserve({{&x->vi_tab, (size_t)3 * (nsets + 1) * 4}});
    if (rc == IVR_OK && do_f) rc = ivr_reserve({{&x->vi_fmax, (size_t)max_mem * nseg * 4}});
    if (rc == IVR_OK && do_b) rc = ivr_reserve({{&x->vi_bmax, (size_t)max_sets * nrows * 4}});
    if (rc == IVR_OK) rc = ivr_reserve({{&x->vi_sums, (size_t)max_sets * nseg * 24}});
    int max_qn = 1;
    for (int i = 0; i < nsets; ++i) max_qn = std::max(max_qn, std::min(bt, toff[i + 1] - toff[i]));
    const size_t lds = (size_t)max_qn * 16 * x->dp * 4;
    if (rc == IVR_OK) rc = ivr_func_max_lds(reinterpret_cast<const void *>(vid_score_kernel), (int)lds);
    if (rc != IVR_OK) return rc;
    rc = ivr_launch_tile_rows(x, x->vi_pack, a.q, 0, a.nq, a.normalize_q, nullptr, s);
    if (rc != IVR_OK) return rc;
    int *moff_d = x->vi_tab, *toff_d = moff_d + nsets + 1, *boff_d = toff_d + nsets + 1;
    const ViTables tb{moff_d, toff_d, boff_d};
    hipLaunchKernelGGL(vid_tables_kernel, dim3(1), dim3(1024), 0, s, a.set_off, nsets, a.nq, bt, moff_d, toff_d, boff_d);
    IVR_LAUNCH_CHECK();
    hipLaunchKernelGGL(vid_retile_kernel, dim3((unsigned)ivr_ceil_div(toff[nsets], 4)), dim3(256), 0, s,
                       reinterpret_cast<const float4 *>((const float *)x->vi_pack), reinterpret_cast<float4 *>((float *)x->vi_q), tb, nsets, x->dp4);
    IVR_LAUNCH_CHECK();
    rc = ivr_launch_rowseg(x, a.seg_off, nseg, s);
    if (rc != IVR_OK) return rc;
    unsigned long long *fsum = reinterpret_cast<unsigned long long *>((uint64_t *)x->vi_sums);
    for (size_t ci = 0; ci + 1 < cuts.size(); ++ci) {
        const int s0 = cuts[ci], s1 = cuts[ci + 1], cnt = s1 - s0, nb = boff[s1] - boff[s0];
        const int64_t slots = (int64_t)cnt * nseg;
        unsigned long long *bsum = fsum + slots;
        uint64_t *keys = reinterpret_cast<uint64_t *>(bsum + slots);
        bool plain = true;                                                // every set of the chunk fits one block: bmax is stored, not maximised
        for (int i = s0; i < s1; ++i) plain = plain && boff[i + 1] - boff[i] == 1;
        if (do_f) IVR_HIP(hipMemsetAsync(x->vi_fmax, 0, (size_t)(off[s1] - off[s0]) * nseg * 4, s));
        if (do_b && !plain) IVR_HIP(hipMemsetAsync(x->vi_bmax, 0, (size_t)cnt * nrows * 4, s));
        IVR_HIP(hipMemsetAsync(fsum, 0, (size_t)slots * 16, s));
        {
            IvrProf prof("vid_score", s, (double)(toff[s1] - toff[s0]) * 16 * n * 2.0 * x->dp);
            const ViScore sc{reinterpret_cast<const float4 *>(x->data), reinterpret_cast<const float4 *>((const float *)x->vi_q), x->dp4, bt, ntiles,
                             x->gr_seg, nseg, nsets, tb, s0, boff[s0], nb, do_f, do_b, x->vi_fmax, x->vi_bmax};
            hipLaunchKernelGGL(vid_score_kernel, dim3((unsigned)(pieces * nb)), dim3(64 * kViWaves), lds, s, sc);
            IVR_LAUNCH_CHECK();
        }
        {
            IvrProf prof("vid_reduce", s, (do_f ? (double)(off[s1] - off[s0]) * nseg * 4 : 0.0) + (do_b ? (double)cnt * nrows * 4 : 0.0));
            const ViReduce rd{tb, nsets, nseg, s0, boff[s0], bt, nrows, x->gr_seg, x->vi_fmax, x->vi_bmax, fsum, bsum};
            if (do_f) {
                hipLaunchKernelGGL(vid_reduce_f_kernel, dim3((unsigned)(ivr_ceil_div(nseg, 256) * nb)), dim3(256), 0, s, rd);
                IVR_LAUNCH_CHECK();
            }
            if (do_b) {
                hipLaunchKernelGGL(vid_reduce_b_kernel, dim3((unsigned)(ivr_ceil_div(nrows, kViReduceRows) * cnt)), dim3(256), 0, s, rd);
                IVR_LAUNCH_CHECK();
            }
        }
        IvrProf prof("vid_select", s, (double)slots * 24, true);
        const ViFinish fin{tb, s0, cnt, nseg, n, a.mode, a.seg_off, fsum, bsum, a.exclude, a.k ? nullptr : a.V + (int64_t)s0 * nseg,
                           a.k ? keys : nullptr};
        hipLaunchKernelGGL(vid_finish_kernel, dim3((unsigned)ivr_ceil_div(slots, 256)), dim3(256), 0, s, fin);
        IVR_LAUNCH_CHECK();
        if (a.k) {
            launch_select<OUT_DI>(SrcVideoKeys{keys, nseg}, cnt, a.k, SelectOut::to_rows(a.D + (int64_t)s0 * a.k, a.Vseg + (int64_t)s0 * a.k), s);
            IVR_LAUNCH_CHECK();
        }
    }
    return IVR_OK;
}

int vid_check(const char *what, const ivr_index *x, const float *q, int nq, const int64_t *set_off, int nsets, const int64_t *seg_off, int nseg,
              int mode) {
    IVR_REQUIRE(x && q, "%s: NULL argument", what);
    IVR_REQUIRE(nq >= 1, "%s: nq=%d < 1", what, nq);
    IVR_REQUIRE(!set_off || nsets >= 1, "%s: nsets=%d with set_off", what, nsets);
    IVR_REQUIRE(set_off || nq <= IVR_VIDEO_MAX_MEMBERS, "%s: one set of %d members > %d", what, nq, IVR_VIDEO_MAX_MEMBERS);
    IVR_REQUIRE(!seg_off || nseg >= 1, "%s: nseg=%d with seg_off", what, nseg);
    IVR_REQUIRE(mode == IVR_VIDEO_FORWARD || mode == IVR_VIDEO_BACKWARD || mode == IVR_VIDEO_SYMMETRIC,
                "%s: mode=%d is none of IVR_VIDEO_FORWARD, IVR_VIDEO_BACKWARD, IVR_VIDEO_SYMMETRIC", what, mode);
    return IVR_OK;
}

}  // namespace

extern "C" {

int ivr_index_video_scores(ivr_index *x, const float *q, int nq, const int64_t *set_off, int nsets, const int64_t *seg_off, int nseg, int mode,
                           int normalize_q, float *V, ivr_stream stream) {
    const int rc = vid_check("ivr_index_video_scores", x, q, nq, set_off, nsets, seg_off, nseg, mode);
    if (rc != IVR_OK) return rc;
    IVR_REQUIRE(V, "ivr_index_video_scores: NULL argument");
    std::lock_guard<std::mutex> lk(x->mu);
    IVR_HIP(hipSetDevice(x->ctx->device));
    return vid_search("ivr_index_video_scores", x, ViArgs{q, nq, set_off, nsets, seg_off, nseg, mode, normalize_q, 0, nullptr, V, nullptr, nullptr},
                      (hipStream_t)stream);
}

int ivr_index_video_search(ivr_index *x, const float *q, int nq, const int64_t *set_off, int nsets, const int64_t *seg_off, int nseg, int mode,
                           int normalize_q, int k, const int64_t *exclude, int64_t *Vseg, float *D, ivr_stream stream) {
    const int rc = vid_check("ivr_index_video_search", x, q, nq, set_off, nsets, seg_off, nseg, mode);
    if (rc != IVR_OK) return rc;
    IVR_REQUIRE(Vseg && D, "ivr_index_video_search: NULL argument");
    IVR_REQUIRE(k >= 1 && k <= IVR_MAX_K, "ivr_index_video_search: k=%d outside [1,%d]", k, IVR_MAX_K);
    std::lock_guard<std::mutex> lk(x->mu);
    IVR_HIP(hipSetDevice(x->ctx->device));
    return vid_search("ivr_index_video_search", x, ViArgs{q, nq, set_off, nsets, seg_off, nseg, mode, normalize_q, k, exclude, nullptr, Vseg, D},
                      (hipStream_t)stream);
}

}  // extern "C"
