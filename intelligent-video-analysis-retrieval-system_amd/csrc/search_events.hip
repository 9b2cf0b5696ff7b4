// Event search over the flat index (ivr_index_search_events, ivr_index_best_events_per_segment): where in the stored rows do m query
// events occur IN ORDER, consecutive events between min_gap and max_gap rows apart and all inside one segment?  The gapped form of the
// clip search (search_seq.hip).  DESIGN.md section 4, "event search".
//
// Frame score S[j, r] = <event j of the chain, stored row r>: the score pass of the clip search (ivr_launch_seq_score), so it has the
// bits ivr_index_search and ivr_index_rescore report for that pair.  Per chain, over the rows inside a segment:
//   C[0, r] = S[0, r]
//   P[j, r] = the candidate p of step j - 1 in [max(lo(r), r - max_gap), r - min_gap] with the greatest ivr_key(C[j-1, p], p): the
//             greatest score, -0.0 equal to +0.0, equal scores the lower row; lo(r) the start of r's segment.  No such p: r is no
//             candidate of step j
//   C[j, r] = (C[j-1, P[j, r]] + 0.0f) + S[j, r]          one float32 addition
//   W[r]    = C[m-1, r] / (float)m                        one correctly rounded division
// Float32 addition is monotone, so C[m-1, r] is the maximum over all admissible chains that end in r of the left-to-right sum.
//
// Launches per chunk of chains, all on the caller's stream and without a host round trip (the segment bounds of sj_prepare once per
// call in front):
//   seq_score     the chunk's frames against every row -> S (search_seq.hip)
//   event_step    m - 1 launches (one event_first launch when m = 1).  A workgroup owns kEvRows rows of one chain: it loads the keys
//                 (ordered C[j-1], ~row) of rows [tile - max_gap, tile + kEvRows - 1 - min_gap] into LDS (step 1 forms them from S[0] and
//                 the segment bounds), 0 for a row that is no candidate.  The unclamped window of a row has w = max_gap - min_gap + 1
//                 slots, so with the slots cut into blocks of w a window touches two neighbouring blocks at most: its maximum is
//                 max(suffix maximum of its block at the lower end, prefix maximum of its block at the upper end) (van Herk / Gil-Werman).
//                 The lo(r) clamp is folded into the prefix scan, which also restarts at every row that starts a segment; the suffix
//                 needs no restart, because a window that reads it ends beyond its block.  Both scans: each thread runs over its own odd
//                 number of consecutive slots, the threads' totals are scanned with shuffles inside a wave and through LDS across the
//                 four waves, and a second run adds the carry.  Work per row is independent of max_gap but for the halo a tile loads.
//                 The last step writes the keys of W; every step writes r - P[j, r] as 16 bits
//   tail          top-k: select_topk_kernel over the W keys (search_select.h), the end rows into scratch; best per segment: one workgroup
//                 per (chain, segment) takes the key maximum of the segment's rows.  Then event_backtrack, one thread per result slot,
//                 follows the m - 1 predecessor distances and writes the labelled path
#include "ivr_common.h"
#include "search_internal.h"
#include "search_select.h"
#include "self_join.h"

namespace {

constexpr int kEvRows = 1024;        // rows of one chain a step workgroup owns
constexpr int kEvThreads = 256;
constexpr int kEvMaxFrames = 1 << 12;    // frames per chunk at most: keeps the score pass's grid (row blocks * frame tiles) below 2^31

struct EvStep {
    const float *S;              // line of event 0 of the chunk's first chain
    int64_t sstride;
    int m, j;                    // events per chain; the step, 1 <= j < m
    int n;                       // stored rows
    int min_gap, max_gap;
    const int *seg_lo;           // [n]: start of the row's segment, row + 1 for a row outside every segment
    const uint64_t *prev;        // [chains][n] keys of step j - 1; NULL for j == 1 (formed from S and seg_lo)
    uint64_t *next;              // [chains][n] keys of step j; of W when j == m - 1
    uint16_t *pred;              // [chains][m - 1][n]
    int tiles;                   // row tiles per chain
    int per_thread;              // LDS slots per thread, odd: lanes 8 * odd bytes apart spread over every bank
};

// The combined total of the threads in front of this one (REV: behind it) in a segmented maximum scan: a thread's total is (flag = its
// run holds a restart, key = the running maximum at its far end).  Only the key of the carry is needed.  wtot: [4] per wave and kind
template <bool REV>
__device__ __forceinline__ uint64_t ev_carry(bool flag, uint64_t key, uint64_t *wkey, int *wflag) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int src = REV ? lane + o : lane - o;
        const uint64_t tk = __shfl(key, src & 63, 64);
        const int tf = __shfl((int)flag, src & 63, 64);
        if (src >= 0 && src < 64) {
            if (!flag) key = tk > key ? tk : key;
            flag = flag || tf;
        }
    }
    // inclusive -> exclusive
    const int nb = REV ? lane + 1 : lane - 1;
    uint64_t ek = __shfl(key, nb & 63, 64);
    bool ef = __shfl((int)flag, nb & 63, 64);
    if (nb < 0 || nb >= 64) {
        ek = 0;
        ef = false;
    }
    if (lane == (REV ? 0 : 63)) {
        wkey[wave] = key;
        wflag[wave] = flag;
    }
    __syncthreads();
    uint64_t ck = 0;             // the waves in front, nearest last
    if (REV) {
        for (int w = kEvThreads / 64 - 1; w > wave; --w) ck = wflag[w] ? wkey[w] : (wkey[w] > ck ? wkey[w] : ck);
    } else {
        for (int w = 0; w < wave; ++w) ck = wflag[w] ? wkey[w] : (wkey[w] > ck ? wkey[w] : ck);
    }
    return ef ? ek : (ek > ck ? ek : ck);
}

// Workgroup b: rows [t0, t0 + kEvRows) of chain b / tiles, t0 = kEvRows (b % tiles).  LDS slot i holds row t0 - max_gap + i; the slots
// past the last row a window of the tile can reach, rows below 0 and rows >= n hold key 0.  Every global read is guarded by
// 0 <= row < n, every LDS index lies below per_thread * kEvThreads, every store is to a row < n of the chain's own stretch.
__global__ __launch_bounds__(kEvThreads) void event_step_kernel(EvStep a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char ev_lds[];
    __shared__ uint64_t wkey[2][kEvThreads / 64];
    __shared__ int wflag[2][kEvThreads / 64];
    const int tid = threadIdx.x;
    const int nslot = a.per_thread * kEvThreads;
    uint64_t *pre = reinterpret_cast<uint64_t *>(ev_lds), *suf = pre + nslot;
    uint8_t *mark = reinterpret_cast<uint8_t *>(suf + nslot);     // bit 0: the prefix restarts here; bit 1: the suffix restarts here
    const int chain = blockIdx.x / a.tiles;
    const int64_t t0 = (int64_t)(blockIdx.x % a.tiles) * kEvRows, base = t0 - a.max_gap;
    const int w = a.max_gap - a.min_gap + 1, nload = kEvRows + w - 1;
    const float *Sc = a.S + ((int64_t)chain * a.m + a.j) * a.sstride;         // this step's line; the line before it is step j - 1's
    const uint64_t *prev = a.prev ? a.prev + (int64_t)chain * a.n : nullptr;
    for (int i = tid; i < nslot; i += kEvThreads) {
        const int64_t row = base + i;
        const bool in = i < nload && row >= 0 && row < a.n;
        uint64_t key = 0;
        int lo = -1;
        if (in) {
            lo = a.seg_lo[row];
            if (prev) key = prev[row];
            else if (lo <= row) key = ivr_key((Sc - a.sstride)[row], (uint32_t)row);
        }
        const int ib = i % w;
        pre[i] = key;
        suf[i] = key;
        mark[i] = (uint8_t)((ib == 0 || lo == row ? 1 : 0) | (ib == w - 1 ? 2 : 0));
    }
    __syncthreads();
    const int i0 = tid * a.per_thread;
    uint64_t run = 0, runs = 0;
    bool seen = false, seens = false;
    for (int e = 0; e < a.per_thread; ++e) {
        const uint64_t v = pre[i0 + e];
        if (mark[i0 + e] & 1) {
            run = v;
            seen = true;
        } else {
            run = v > run ? v : run;
        }
        pre[i0 + e] = run;
    }
    for (int e = a.per_thread - 1; e >= 0; --e) {
        const uint64_t v = suf[i0 + e];
        if (mark[i0 + e] & 2) {
            runs = v;
            seens = true;
        } else {
            runs = v > runs ? v : runs;
        }
        suf[i0 + e] = runs;
    }
    const uint64_t cp = ev_carry<false>(seen, run, wkey[0], wflag[0]);
    const uint64_t cs = ev_carry<true>(seens, runs, wkey[1], wflag[1]);
    for (int e = 0; e < a.per_thread && !(mark[i0 + e] & 1); ++e) pre[i0 + e] = cp > pre[i0 + e] ? cp : pre[i0 + e];
    for (int e = a.per_thread - 1; e >= 0 && !(mark[i0 + e] & 2); --e) suf[i0 + e] = cs > suf[i0 + e] ? cs : suf[i0 + e];
    __syncthreads();
    uint64_t *next = a.next + (int64_t)chain * a.n;
    uint16_t *pred = a.pred + ((int64_t)chain * (a.m - 1) + (a.j - 1)) * a.n;
    const bool last = a.j == a.m - 1;
    for (int q = tid; q < kEvRows; q += kEvThreads) {
        const int64_t r = t0 + q;
        if (r >= a.n) break;
        const int64_t lo = a.seg_lo[r], b = r - a.min_gap;
        const int64_t f = max(lo, r - a.max_gap);
        uint64_t pk = 0;
        if (f <= b) {
            const int ia = (int)(f - base), ib = (int)(b - base);         // 0 <= ia <= ib = q + w - 1 < nload
            pk = pre[ib];
            if (ia / w != ib / w) pk = suf[ia] > pk ? suf[ia] : pk;
        }
        uint64_t key = 0;
        uint16_t dist = 0;
        if (pk) {
            const uint32_t p = 0xFFFFFFFFu - (uint32_t)pk;
            const float c = ivr_ord2f((uint32_t)(pk >> 32)) + Sc[r];
            key = ivr_key(last ? c / (float)a.m : c, (uint32_t)r);
            dist = (uint16_t)(r - p);
        }
        next[r] = key;
        pred[r] = dist;
    }
}

// m == 1: the keys of W = S[0] / 1 of the rows inside a segment.  Thread i: chain i / n, row i % n
__global__ __launch_bounds__(256) void event_first_kernel(const float *S, int64_t sstride, int n, int64_t nslots, const int *seg_lo,
                                                          uint64_t *keys) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= nslots) return;
    const int64_t c = i / n, r = i - c * n;
    keys[i] = seg_lo[r] <= r ? ivr_key(S[c * sstride + r], (uint32_t)r) : 0ull;
}

struct SrcEvents {     // the W keys of chain q of the chunk, every one written
    const uint64_t *keys;
    int64_t n;
    __device__ uint64_t key(int q, int64_t i) const { return keys[(int64_t)q * n + i]; }
};

// Workgroup b: segment b % nseg of chain b / nseg: the greatest key of its rows -> D and the end row (-FLT_MAX, -1 without a chain).
// A row outside every segment holds key 0 already
__global__ __launch_bounds__(256) void event_segbest_kernel(const uint64_t *keys, int n, const int64_t *seg_off, int nseg, float *D, int64_t *rows) {
    __shared__ uint64_t wbest[4];
    const int c = blockIdx.x / nseg, sg = blockIdx.x % nseg;
    const int64_t lo = seg_off ? max(seg_off[sg], (int64_t)0) : 0, hi = seg_off ? min(seg_off[sg + 1], (int64_t)n) : n;
    const uint64_t *kc = keys + (int64_t)c * n;
    uint64_t best = 0;
    for (int64_t r = lo + threadIdx.x; r < hi; r += 256) best = kc[r] > best ? kc[r] : best;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const uint64_t t = __shfl_xor(best, o, 64);
        best = t > best ? t : best;
    }
    if ((threadIdx.x & 63) == 0) wbest[threadIdx.x >> 6] = best;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int v = 1; v < 4; ++v) best = wbest[v] > best ? wbest[v] : best;
        D[blockIdx.x] = best ? ivr_ord2f((uint32_t)(best >> 32)) : -FLT_MAX;
        rows[blockIdx.x] = best ? (int64_t)(0xFFFFFFFFu - (uint32_t)best) : -1;
    }
}

// Thread i: result slot i of the chunk (chain i / kk): from its end row m - 1 dependent reads of the predecessor distances; the path
// in event order, as row numbers or as stored ids; -1 in all m entries of an unused slot
__global__ __launch_bounds__(256) void event_backtrack_kernel(const int64_t *rows, int64_t nslots, int kk, int m, int n, const uint16_t *pred,
                                                              const int64_t *ids, int64_t *I) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= nslots) return;
    int64_t r = rows[i];
    int64_t *out = I + i * m;
    if (r < 0 || r >= n) {
        for (int j = 0; j < m; ++j) out[j] = -1;
        return;
    }
    const uint16_t *pc = pred + (i / kk) * (int64_t)(m - 1) * n;
    for (int j = m - 1; j >= 1; --j) {
        out[j] = ids ? ids[r] : r;
        r -= pc[(int64_t)(j - 1) * n + r];
    }
    out[0] = ids ? ids[r] : r;
}

// no chain at all (no stored rows, or fewer than the shortest chain spans): every slot unused
__global__ __launch_bounds__(256) void event_absent_kernel(int64_t nD, float *__restrict__ D, int64_t nI, int64_t *__restrict__ I) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < nD) D[i] = -FLT_MAX;
    for (int64_t t = i; t < nI; t += (int64_t)gridDim.x * 256) I[t] = -1;
}

struct EvArgs {
    const float *q;
    int B, m, min_gap, max_gap;
    const int64_t *seg_off;
    int nseg;
    int normalize_q;
    int k;                       // top-k: D [B][k], I [B][k][m]; 0: best per segment, D [B][nseg], I [B][nseg][m] (nseg = 1 without seg_off)
    float *D;
    int64_t *I;
};

int ev_check(const char *what, ivr_index *x, const EvArgs &a) {
    IVR_REQUIRE(x && a.q && a.D && a.I, "%s: NULL argument", what);
    IVR_REQUIRE(a.m >= 1 && a.m <= IVR_EVENT_MAX_LEN, "%s: m=%d outside [1,%d]", what, a.m, IVR_EVENT_MAX_LEN);
    IVR_REQUIRE(a.B >= 1 && a.B <= (1 << 24), "%s: B=%d outside [1,2^24]", what, a.B);
    IVR_REQUIRE(a.min_gap >= 1 && a.min_gap <= a.max_gap && a.max_gap <= IVR_EVENT_MAX_GAP, "%s: gaps [%d,%d] outside 1 <= min_gap <= max_gap <= %d",
                what, a.min_gap, a.max_gap, IVR_EVENT_MAX_GAP);
    IVR_REQUIRE(!a.seg_off || a.nseg >= 1, "%s: nseg=%d with seg_off", what, a.nseg);
    return IVR_OK;
}

// both entry points once their arguments are checked; the caller holds x->mu
int ev_search(const char *what, ivr_index *x, const EvArgs &a, hipStream_t s) {
    IVR_REQUIRE(x->ntotal < (1ll << 31), "%s: ntotal=%lld >= 2^31", what, (long long)x->ntotal);
    const int kk = a.k ? a.k : (a.seg_off ? a.nseg : 1);
    const int n = (int)x->ntotal;
    if ((int64_t)n <= (int64_t)(a.m - 1) * a.min_gap) {           // the shortest chain spans (m - 1) min_gap + 1 rows
        const int64_t nD = (int64_t)a.B * kk, nI = nD * a.m;
        hipLaunchKernelGGL(event_absent_kernel, dim3((unsigned)ivr_ceil_div(nD, 256)), dim3(256), 0, s, nD, a.D, nI, a.I);
        IVR_LAUNCH_CHECK();
        return IVR_OK;
    }
    // chains per chunk: the key slots of the clip search's budget, and the frames one score launch may take
    const int cb = (int)std::max<int64_t>(1, std::min<int64_t>({(int64_t)a.B, x->seq_chunk_slots / n, (int64_t)kEvMaxFrames / a.m}));
    const int64_t sstride = ivr_ceil_div(n, 16) * 16, nframes = (int64_t)a.B * a.m;
    const int64_t ftiles = std::min<int64_t>(ivr_ceil_div(nframes, 16), ivr_ceil_div((int64_t)cb * a.m, 16) + 1);
    const int tiles = (int)ivr_ceil_div(n, kEvRows);
    const int w = a.max_gap - a.min_gap + 1;
    const int per_thread = (int)ivr_ceil_div(kEvRows + w - 1, kEvThreads) | 1;
    const size_t lds = (size_t)per_thread * kEvThreads * 17;
    int rc = ivr_reserve_queries(x, (int)ivr_ceil_div(nframes, 16));
    if (rc == IVR_OK)
        rc = ivr_reserve({{&x->seq_scores, (size_t)ftiles * 16 * sstride * 4},
                          {&x->ev_keys, (size_t)2 * cb * n * 8},
                          {&x->ev_pred, (size_t)cb * std::max(a.m - 1, 1) * n * 2},
                          {&x->ev_rows, (size_t)cb * kk * 8}});
    if (rc == IVR_OK && a.m > 1) rc = ivr_func_max_lds(reinterpret_cast<const void *>(event_step_kernel), (int)lds);
    if (rc != IVR_OK) return rc;
    SjArgs sj;
    rc = sj_prepare(x, 1, a.seg_off, a.nseg, s, sj);
    if (rc != IVR_OK) return rc;
    rc = ivr_launch_tile_rows(x, x->qtiled, a.q, 0, nframes, a.normalize_q, nullptr, s);
    if (rc != IVR_OK) return rc;
    const int64_t *ids = x->has_ids ? x->ids : nullptr;
    uint64_t *kbuf[2] = {x->ev_keys, (uint64_t *)x->ev_keys + (int64_t)cb * n};
    for (int b0 = 0; b0 < a.B; b0 += cb) {
        const int cnt = std::min(cb, a.B - b0);
        const int64_t f0 = (int64_t)b0 * a.m, f1 = f0 + (int64_t)cnt * a.m;       // the chunk's frames
        const int qtile0 = (int)(f0 >> 4), qtiles = (int)((f1 - 1) >> 4) - qtile0 + 1;
        rc = ivr_launch_seq_score(x, qtile0, qtiles, s);
        if (rc != IVR_OK) return rc;
        const float *S0 = (const float *)x->seq_scores + (f0 - 16 * (int64_t)qtile0) * sstride;
        const int64_t nslots = (int64_t)cnt * n;
        const uint64_t *wkeys;
        if (a.m == 1) {
            IvrProf prof("event_step", s, (double)nslots * 16);
            hipLaunchKernelGGL(event_first_kernel, dim3((unsigned)ivr_ceil_div(nslots, 256)), dim3(256), 0, s, S0, sstride, n, nslots, sj.seg_lo, kbuf[0]);
            IVR_LAUNCH_CHECK();
            wkeys = kbuf[0];
        } else {
            // bytes a step must move per row: the previous keys (step 1: S[0] and the bounds), S[j], the bounds, the new key, the distance
            IvrProf prof("event_step", s, (double)nslots * (a.m - 1) * 26.0);
            for (int j = 1; j < a.m; ++j) {
                const EvStep st{S0, sstride, a.m, j, n, a.min_gap, a.max_gap, sj.seg_lo, j == 1 ? nullptr : kbuf[j & 1], kbuf[(j + 1) & 1],
                                x->ev_pred, tiles, per_thread};
                hipLaunchKernelGGL(event_step_kernel, dim3((unsigned)((int64_t)cnt * tiles)), dim3(kEvThreads), lds, s, st);
                IVR_LAUNCH_CHECK();
            }
            wkeys = kbuf[a.m & 1];
        }
        IvrProf prof("event_tail", s, (double)nslots * 8, true);
        if (a.k) {
            launch_select<OUT_DI>(SrcEvents{wkeys, n}, cnt, a.k, SelectOut::to_rows(a.D + (int64_t)b0 * a.k, x->ev_rows), s);
        } else {
            hipLaunchKernelGGL(event_segbest_kernel, dim3((unsigned)((int64_t)cnt * kk)), dim3(256), 0, s, wkeys, n, a.seg_off, kk,
                               a.D + (int64_t)b0 * kk, x->ev_rows);
        }
        IVR_LAUNCH_CHECK();
        const int64_t nres = (int64_t)cnt * kk;
        hipLaunchKernelGGL(event_backtrack_kernel, dim3((unsigned)ivr_ceil_div(nres, 256)), dim3(256), 0, s, x->ev_rows, nres, kk, a.m, n, x->ev_pred,
                           ids, a.I + (int64_t)b0 * kk * a.m);
        IVR_LAUNCH_CHECK();
    }
    return IVR_OK;
}

}  // namespace

extern "C" {

int ivr_index_search_events(ivr_index *x, const float *q, int B, int m, int min_gap, int max_gap, const int64_t *seg_off, int nseg, int k,
                            int normalize_q, float *D, int64_t *I, ivr_stream stream) {
    const EvArgs a{q, B, m, min_gap, max_gap, seg_off, nseg, normalize_q, k, D, I};
    const int rc = ev_check("ivr_index_search_events", x, a);
    if (rc != IVR_OK) return rc;
    IVR_REQUIRE(k >= 1 && k <= IVR_MAX_K, "ivr_index_search_events: k=%d outside [1,%d]", k, IVR_MAX_K);
    std::lock_guard<std::mutex> lk(x->mu);
    IVR_HIP(hipSetDevice(x->ctx->device));
    return ev_search("ivr_index_search_events", x, a, (hipStream_t)stream);
}

int ivr_index_best_events_per_segment(ivr_index *x, const float *q, int B, int m, int min_gap, int max_gap, const int64_t *seg_off, int nseg,
                                      int normalize_q, float *D, int64_t *I, ivr_stream stream) {
    const EvArgs a{q, B, m, min_gap, max_gap, seg_off, nseg, normalize_q, 0, D, I};
    const int rc = ev_check("ivr_index_best_events_per_segment", x, a);
    if (rc != IVR_OK) return rc;
    IVR_REQUIRE(!seg_off || (int64_t)B * nseg < (1ll << 31), "ivr_index_best_events_per_segment: B * nseg = %lld >= 2^31", (long long)B * nseg);
    std::lock_guard<std::mutex> lk(x->mu);
    IVR_HIP(hipSetDevice(x->ctx->device));
    return ev_search("ivr_index_best_events_per_segment", x, a, (hipStream_t)stream);
}

}  // extern "C"
