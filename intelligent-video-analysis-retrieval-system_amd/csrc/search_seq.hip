// Clip search over the flat index (ivr_index_search_sequences, ivr_index_range_search_sequences): where in the stored rows does a run
// of L consecutive query frames occur?  The reference's TemporalAnalyzer.find_similar_sequences (core.py:3644-3702) as a sliding-window
// match.  DESIGN.md section 4, "clip search".
//
// Frame score S[t, s] = <query frame t, stored row s>, accumulated by mfma_chunk4 in ascending chunk order from the float32 tiles of
// the storage and the tiled query buffer, from a zero accumulator: the sequence of every float32 score of the index
// (search_internal.h), so it has the bits ivr_index_search and ivr_index_rescore report for that pair.  Window score of target window
// t against the stored run that starts at row s:
//   W[t, s] = (((S[t, s] + S[t + 1, s + 1]) + ...) + S[t + L - 1, s + L - 1]) / float32(L)
// L - 1 float32 additions in ascending order, each rounded on its own, and one correctly rounded division.  A start is a candidate
// when [s, s + L) lies inside one segment of seg_off (the whole index without one).
//
// Launches per chunk of target windows, all on the caller's stream and without a host round trip:
//   seq_score    one workgroup per (64 row tiles, 16 query frames): the frames in LDS in the operand layout, S -> scratch [frame][row]
//   seq_window   one thread per (window, start): the L diagonal reads, the ordered sum, the division, the segment test -> a 64-bit key
//                (ordered W, ~start) in the window's stretch of the key scratch, 0 for a start that is no candidate.  Every slot of a
//                stretch is written: the scratch is reused
//   tail         top-k: select_topk_kernel (search_select.h), one workgroup per window; range: the count / prefix / write passes of
//                search_range_keys.h, with the running total carried on the device from chunk to chunk
// A chunk holds as many windows as fit IVR_SEQ_CHUNK_SLOTS key slots (one window's stretch at least); the frames of consecutive
// chunks overlap by L - 1 (in whole 16-frame tiles), which are scored again.
#include "ivr_common.h"
#include "search_internal.h"
#include "search_range_keys.h"
#include "search_select.h"

namespace {

constexpr int kSeqMaxChunk = 1 << 12;    // windows per chunk at most: keeps the score pass's grid (row blocks * frame tiles) below 2^31
constexpr int kSeqTilesPerBlock = 64;    // 16-row tiles per workgroup of the score pass: the staged frames are 1/64 of the bytes it reads

struct SeqScore {
    const float4 *data;          // the float32 tiles of the storage
    const float4 *qtile;         // the first 16-frame tile of the chunk in the tiled query buffer
    int dp4;
    int qtiles;                  // 16-frame tiles of the chunk
    int64_t ntiles;              // 16-row tiles that hold stored rows
    float *S;                    // [16 qtiles][sstride]
    int64_t sstride;             // 16 ntiles
};

// Workgroup b: frame tile y = b % qtiles of the chunk against the row tiles 64 x .. 64 x + 63, x = b / qtiles, four at a time, one per
// wave.  The frame tile is the fast index, so the workgroups that read the same rows are dispatched together and all but the first
// find them in cache.  The frame tile is copied to LDS as it lies in the tiled query buffer (element (kc, lane) = the float4 of frame
// (lane & 15), quad (lane >> 4), chunk kc); the padding frames of the last tile are zero rows there.  Every tile read lies inside the
// storage's allocation, whose capacity is a multiple of 64 rows >= ntotal, and every store inside frame tile y's 16 lines of S.
__global__ __launch_bounds__(256) void seq_score_kernel(SeqScore a) {
    extern __shared__ __attribute__((aligned(16))) float4 qs[];
    const int per_tile = a.dp4 * 16, kchunks = a.dp4 >> 2;
    const int y = (int)(blockIdx.x % a.qtiles);
    const int64_t x = blockIdx.x / a.qtiles;
    const float4 *qt = a.qtile + (int64_t)y * per_tile;
    for (int i = threadIdx.x; i < per_tile; i += blockDim.x) qs[i] = qt[i];
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t t0 = x * kSeqTilesPerBlock, t1 = min(t0 + kSeqTilesPerBlock, a.ntiles);
    float *out = a.S + ((int64_t)y * 16 + (lane & 15)) * a.sstride + (lane >> 4) * 4;
    for (int64_t t = t0 + wave; t < t1; t += 4) {
        const float4 *at = a.data + t * per_tile + lane;
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        stream_tile<1>(at, kchunks, [&](int, int kc, const float4 &av) { mfma_chunk4(acc, av, qs[kc * 64 + lane]); });
        // acc[r] = <row 16 t + 4 (lane >> 4) + r, frame (lane & 15) of the tile>
        *reinterpret_cast<f32x4 *>(out + t * 16) = acc;
    }
}

}  // namespace

// search_internal.h: the score pass as the clip search and the event search (search_events.hip) launch it
int ivr_launch_seq_score(ivr_index *x, int qtile0, int qtiles, hipStream_t s) {
    const size_t lds = (size_t)16 * x->dp * 4;
    const int rc = ivr_func_max_lds(reinterpret_cast<const void *>(seq_score_kernel), (int)lds);
    if (rc != IVR_OK) return rc;
    const int64_t ntiles = ivr_ceil_div(x->ntotal, 16);
    IvrProf prof("seq_score", s, (double)qtiles * 16 * x->ntotal * 2.0 * x->dp);
    const SeqScore sc{reinterpret_cast<const float4 *>(x->data), reinterpret_cast<const float4 *>((const float *)x->qtiled) + (int64_t)qtile0 * x->dp4 * 16,
                      x->dp4, qtiles, ntiles, x->seq_scores, ntiles * 16};
    hipLaunchKernelGGL(seq_score_kernel, dim3((unsigned)(ivr_ceil_div(ntiles, kSeqTilesPerBlock) * qtiles)), dim3(256), lds, s, sc);
    IVR_LAUNCH_CHECK();
    return IVR_OK;
}

namespace {

struct SeqWindow {
    const float *S;
    int64_t sstride;
    int f0;                      // line of S that holds the first frame of the chunk's first window
    int L;
    int64_t nstart;              // starts per window: ntotal - L + 1
    int64_t nslots;              // windows of the chunk * nstart
    const int64_t *seg_off;      // [nseg + 1] or NULL
    int nseg;
    uint64_t *keys;
};

// Thread i: window i / nstart of the chunk, start row s = i % nstart.  Its L reads lie on a diagonal of S: line f0 + w + j, row s + j,
// with s + L - 1 < ntotal.  The sum is written out term by term (additions and one division: nothing a contraction could fuse).
__global__ __launch_bounds__(256) void seq_window_kernel(SeqWindow a) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= a.nslots) return;
    const int64_t w = i / a.nstart, s = i - w * a.nstart;
    const float *p = a.S + (a.f0 + w) * a.sstride + s;
    float sum = p[0];
    for (int j = 1; j < a.L; ++j) {
        p += a.sstride + 1;
        sum = sum + p[0];
    }
    const float W = sum / (float)a.L;
    bool ok = true;
    if (a.seg_off) {
        // the segment that holds s: the last offset <= s (with empty segments, the one run that holds s)
        ok = a.seg_off[0] <= s;
        if (ok) {
            const int j = ivr_last_le(a.seg_off, a.nseg + 1, s);
            ok = j < a.nseg && s + a.L <= a.seg_off[j + 1];
        }
    }
    a.keys[i] = ok ? ivr_key(W, (uint32_t)s) : 0ull;
}

struct SrcWindows {    // the keys of window q of the chunk: slots [q * n, (q + 1) * n) of the scratch, every one written
    const uint64_t *keys;
    int64_t n;
    __device__ uint64_t key(int q, int64_t i) const { return keys[(int64_t)q * n + i]; }
};

// no candidate at all (fewer stored rows than L): every top-k slot unused, every lims entry 0
__global__ __launch_bounds__(256) void seq_absent_kernel(int64_t nsel, float *__restrict__ D, int64_t *__restrict__ I, int64_t nlims,
                                                         int64_t *__restrict__ lims) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (D && i < nsel) {
        D[i] = -FLT_MAX;
        I[i] = -1;
    }
    if (lims && i < nlims) lims[i] = 0;
}

struct SeqArgs {
    const float *q;
    int T, L;
    const int64_t *seg_off;
    int nseg;
    int normalize_q;
    // top-k (k > 0): D / I [T - L + 1][k]; range (k == 0): lims [T - L + 2], D / I [cap]
    int k;
    float threshold;
    int64_t *lims;
    float *D;
    int64_t *I;
    int64_t cap;
};

int seq_check(const char *what, ivr_index *x, const float *q, int T, int L, const int64_t *seg_off, int nseg, const float *D, const int64_t *I) {
    IVR_REQUIRE(x && q && D && I, "%s: NULL argument", what);
    IVR_REQUIRE(L >= 1 && L <= IVR_SEQ_MAX_LEN, "%s: L=%d outside [1,%d]", what, L, IVR_SEQ_MAX_LEN);
    IVR_REQUIRE(T >= L, "%s: T=%d frames < L=%d", what, T, L);
    IVR_REQUIRE(!seg_off || nseg >= 1, "%s: nseg=%d with seg_off", what, nseg);
    return IVR_OK;
}

// both entry points once their arguments are checked; the caller holds x->mu
int seq_search(ivr_index *x, const SeqArgs &a, hipStream_t s) {
    const int nwin = a.T - a.L + 1;
    const int64_t nstart = x->ntotal - a.L + 1;
    if (nstart <= 0) {
        const int64_t nsel = a.k ? (int64_t)nwin * a.k : 0, nlims = a.k ? 0 : nwin + 1;
        hipLaunchKernelGGL(seq_absent_kernel, dim3((unsigned)ivr_ceil_div(std::max(nsel, nlims), 256)), dim3(256), 0, s, nsel, a.k ? a.D : nullptr,
                           a.I, nlims, a.k ? nullptr : a.lims);
        IVR_LAUNCH_CHECK();
        return IVR_OK;
    }
    // windows per chunk; frame tiles of a chunk: its wc + L - 1 frames start anywhere in their first tile
    // (at most kSeqMaxChunk, which bounds the grid of the score pass: row blocks * frame tiles)
    const int wc = (int)std::max<int64_t>(1, std::min<int64_t>({(int64_t)nwin, x->seq_chunk_slots / nstart, (int64_t)kSeqMaxChunk}));
    const int64_t ntiles = ivr_ceil_div(x->ntotal, 16), sstride = ntiles * 16;
    const int64_t ftiles = std::min<int64_t>(ivr_ceil_div(a.T, 16), ivr_ceil_div(wc + a.L - 1, 16) + 1);
    const int64_t nblk = range_keys_blocks(nstart);
    int rc = ivr_reserve_queries(x, (int)ivr_ceil_div(a.T, 16));
    if (rc == IVR_OK) rc = ivr_reserve({{&x->seq_scores, (size_t)ftiles * 16 * sstride * 4}, {&x->seq_keys, (size_t)wc * nstart * 8}});
    if (rc == IVR_OK && !a.k) rc = ivr_reserve({{&x->seq_off, (size_t)wc * nblk * 8}, {&x->seq_total, 8}});
    if (rc != IVR_OK) return rc;
    rc = ivr_launch_tile_rows(x, x->qtiled, a.q, 0, a.T, a.normalize_q, nullptr, s);
    if (rc != IVR_OK) return rc;
    const int64_t *ids = x->has_ids ? x->ids : nullptr;
    for (int w0 = 0; w0 < nwin; w0 += wc) {
        const int wcnt = std::min(wc, nwin - w0);
        const int qtile0 = w0 >> 4, qtiles = ((w0 + wcnt + a.L - 2) >> 4) - qtile0 + 1;
        rc = ivr_launch_seq_score(x, qtile0, qtiles, s);
        if (rc != IVR_OK) return rc;
        const int64_t nslots = (int64_t)wcnt * nstart;
        {
            IvrProf prof("seq_window", s, (double)nslots * (4.0 * a.L + 8));
            const SeqWindow sw{x->seq_scores, sstride, w0 - 16 * qtile0, a.L, nstart, nslots, a.seg_off, a.nseg, x->seq_keys};
            hipLaunchKernelGGL(seq_window_kernel, dim3((unsigned)ivr_ceil_div(nslots, 256)), dim3(256), 0, s, sw);
            IVR_LAUNCH_CHECK();
        }
        const SrcWindows src{x->seq_keys, nstart};
        if (a.k) {
            IvrProf prof("select_final", s, (double)nslots * 8, true);
            const SelectOut o = SelectOut::to_rows(a.D + (int64_t)w0 * a.k, a.I + (int64_t)w0 * a.k, 0, ids);
            if (o.ids) launch_select<OUT_DI_IDS>(src, wcnt, a.k, o, s);
            else launch_select<OUT_DI>(src, wcnt, a.k, o, s);
        } else {
            IvrProf prof("seq_range_tail", s, (double)nslots * 16, true);
            launch_range_keys(src, wcnt, w0, w0 == 0, a.threshold, x->seq_off, x->seq_total, a.lims, a.D, a.I, a.cap, ids, s);
        }
        IVR_LAUNCH_CHECK();
    }
    return IVR_OK;
}

}  // namespace

extern "C" {

int ivr_index_search_sequences(ivr_index *x, const float *q, int T, int L, const int64_t *seg_off, int nseg, int k, int normalize_q, float *D,
                               int64_t *I, ivr_stream stream) {
    const int rc = seq_check("ivr_index_search_sequences", x, q, T, L, seg_off, nseg, D, I);
    if (rc != IVR_OK) return rc;
    IVR_REQUIRE(k >= 1 && k <= IVR_MAX_K, "ivr_index_search_sequences: k=%d outside [1,%d]", k, IVR_MAX_K);
    std::lock_guard<std::mutex> lk(x->mu);
    IVR_HIP(hipSetDevice(x->ctx->device));
    return seq_search(x, SeqArgs{q, T, L, seg_off, nseg, normalize_q, k, 0.f, nullptr, D, I, 0}, (hipStream_t)stream);
}

int ivr_index_range_search_sequences(ivr_index *x, const float *q, int T, int L, const int64_t *seg_off, int nseg, float threshold,
                                     int normalize_q, int64_t *lims, float *D, int64_t *I, int64_t cap, ivr_stream stream) {
    const int rc = seq_check("ivr_index_range_search_sequences", x, q, T, L, seg_off, nseg, D, I);
    if (rc != IVR_OK) return rc;
    IVR_REQUIRE(lims, "ivr_index_range_search_sequences: NULL argument");
    IVR_REQUIRE(cap >= 0, "ivr_index_range_search_sequences: cap=%lld", (long long)cap);
    IVR_REQUIRE(!(threshold != threshold), "ivr_index_range_search_sequences: threshold is NaN");
    std::lock_guard<std::mutex> lk(x->mu);
    IVR_HIP(hipSetDevice(x->ctx->device));
    return seq_search(x, SeqArgs{q, T, L, seg_off, nseg, normalize_q, 0, threshold, lims, D, I, cap}, (hipStream_t)stream);
}

}  // extern "C"
