// Inverted lists over the flat index (ivr_index_search_lists) and the centroid update of their k-means (ivr_segment_mean).
//
// An inverted-file index keeps its rows in one id-mapped ivr_index ordered by list: list l is the run of rows
// [list_off[l], list_off[l + 1]).  A search scores, per query, only the rows of the lists it probes.  The scan is list-major: the
// (query, list) pairs of a chunk of queries are grouped by list, and a workgroup multiplies the 16-row tiles that cover one list's run
// against up to 16 of the queries that probe it on the float32 MFMA, so a list probed by up to 16 queries of a batch is read once.
// The scores are accumulated by mfma_chunk4 in ascending chunk order from the same float32 tiles as every other score of the index
// (search_internal.h): bit-identical to the flat search.  Each score becomes a 64-bit key (ordered score, ~row) in a slot of the
// query's own stretch of a scratch buffer, one slot per row of its probed lists, and select_topk_kernel (search_select.h) ranks the
// keys of each query: equal scores rank the lower storage row first, i.e. the lower list and inside a list the row added earlier,
// whatever order the lists were probed in.
//
// Launches per chunk of queries, all on the caller's stream and without a host round trip:
//   probe_slots   one wave per query: the slot stretch of each of its lists (exclusive prefix of the list sizes), -1 for skipped entries
//   probe_count   one thread per pair: queries per list
//   probe_offsets one workgroup: exclusive prefixes over the lists of the pairs and of the 16-query pair tiles
//   probe_fill    one thread per pair: the pairs grouped by list
//   list_scan     one workgroup per (pair tile, row split): scores -> keys
//   select_topk   one workgroup per query
// The probe tables and the selection over the key stretches are ProbeTables' (search_internal.h, search_lists.hip: the four probe
// kernels, build, select); search_ivfsq.hip scans the same tables.  Only list_scan_kernel is emitted here.
#include "ivr_common.h"
#include "search_internal.h"
#include "search_lists.h"

namespace {

struct ListScan {
    const float4 *data;          // the float32 tiles of the storage
    const float4 *qtiled;        // the chunk's queries, tiled
    int dp4;
    int nlist;
    int q0, nqc;                 // the chunk's queries: q0 .. q0 + nqc of the tiled buffer; pair_q counts from q0
    int64_t ntotal;
    const int64_t *list_off;
    const int64_t *pair_off, *tile_off;
    const int *pair_q;
    const int64_t *pair_slot;
    uint64_t *keys;
    int64_t nkeys;               // slots of the scratch: nothing is written at or past it
};

// Workgroup (w, y): pair tile w = up to 16 queries that probe one list, found by a binary search of w in tile_off; of the 16-row tiles
// that cover the list's run it takes number 16 y .. 16 y + 15 (256 rows: the staged queries are 1/16 of the bytes it reads), then those
// 16 gridDim.y further on, four to a wave, and exits at once when the run ends before its first tile.  The queries are gathered from the tiled query
// buffer into LDS in the operand layout (element (kc, lane) = the float4 of query (lane & 15), quad (lane >> 4), chunk kc; unused
// columns zero).  Rows of a covering tile that lie outside the run belong to a neighbouring list (or to no row): they get no key.
// Every tile read lies inside the storage's allocation, whose capacity is a multiple of 64 rows >= ntotal.
__global__ __launch_bounds__(256) void list_scan_kernel(ListScan a) {
    extern __shared__ __attribute__((aligned(16))) float4 qs[];
    __shared__ int s_q[16];
    __shared__ int64_t s_slot[16];
    const int64_t w = blockIdx.x;
    if (w >= a.tile_off[a.nlist]) return;
    int lo = 0, hi = a.nlist - 1;                    // the last list whose first pair tile is at or below w
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (a.tile_off[mid] <= w) lo = mid;
        else hi = mid - 1;
    }
    const int64_t p0 = a.pair_off[lo] + (w - a.tile_off[lo]) * 16;
    const int cnt = (int)min((int64_t)16, a.pair_off[lo + 1] - p0);
    int64_t r0, r1;
    list_run(a.list_off, lo, a.ntotal, r0, r1);
    const int64_t t1 = (r1 + 15) >> 4;
    if (r1 <= r0 || cnt <= 0 || (r0 >> 4) + (int64_t)blockIdx.y * 16 >= t1) return;
    if (threadIdx.x < 16) {
        const bool on = (int)threadIdx.x < cnt;
        const int q = on ? a.pair_q[p0 + threadIdx.x] : -1;
        s_q[threadIdx.x] = q >= 0 && q < a.nqc ? q : -1;
        s_slot[threadIdx.x] = on ? a.pair_slot[p0 + threadIdx.x] : 0;
    }
    __syncthreads();
    const int per_tile = a.dp4 * 16, kchunks = a.dp4 >> 2;
    for (int i = threadIdx.x; i < per_tile; i += blockDim.x) {
        const int q = s_q[i & 15];
        const int qg = a.q0 + q;
        qs[i] = q >= 0 ? a.qtiled[(int64_t)(qg >> 4) * per_tile + (i & ~15) + (qg & 15)] : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int col = lane & 15;
    for (int64_t tb = (r0 >> 4) + (int64_t)blockIdx.y * 16; tb < t1; tb += (int64_t)gridDim.y * 16)
    for (int64_t t = tb + wave; t < min(tb + 16, t1); t += 4) {
        const float4 *at = a.data + t * per_tile + lane;
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        stream_tile<1>(at, kchunks, [&](int, int kc, const float4 &av) { mfma_chunk4(acc, av, qs[kc * 64 + lane]); });
        // acc[r] = <row 16 t + 4 (lane >> 4) + r, query column (lane & 15)>
        if (s_q[col] < 0) continue;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int64_t row = t * 16 + (lane >> 4) * 4 + r;
            if (row < r0 || row >= r1) continue;
            const int64_t s = s_slot[col] + (row - r0);
            if (s >= 0 && s < a.nkeys) a.keys[s] = ivr_key(acc[r], (uint32_t)row);
        }
    }
}

// ---------------------------------------------------------------------------------------------
// ivr_segment_mean
// ---------------------------------------------------------------------------------------------
// One workgroup per segment; thread t owns the columns t, t + 256, ...: a column is summed over the segment's rows in ascending row
// order in double precision (no atomics: the same bits on every run), divided by the count and rounded to float32.  With normalize
// the squared means are summed per thread in column order and over the workgroup by a fixed tree, and a second sweep scales the
// row.  An empty segment gives a NaN row.
__global__ __launch_bounds__(256) void segment_mean_kernel(const float *__restrict__ rows, const int64_t *__restrict__ seg_off, int64_t n, int d,
                                                           int normalize, float *__restrict__ out) {
    __shared__ double red[256];
    const int64_t sgm = blockIdx.x;
    const int64_t s0 = min(max(seg_off[sgm], (int64_t)0), n), s1 = min(max(seg_off[sgm + 1], s0), n);
    float *o = out + sgm * (int64_t)d;
    if (s1 <= s0) {
        for (int c = threadIdx.x; c < d; c += 256) o[c] = __uint_as_float(0x7fc00000u);
        return;
    }
    const double inv = 1.0 / (double)(s1 - s0);
    double ss = 0.0;
    for (int c = threadIdx.x; c < d; c += 256) {
        double sum = 0.0;
        for (int64_t r = s0; r < s1; ++r) sum += (double)rows[r * d + c];
        const float m = (float)(sum * inv);
        o[c] = m;
        ss += (double)m * (double)m;
    }
    if (!normalize) return;
    red[threadIdx.x] = ss;
    __syncthreads();
    for (int o2 = 128; o2 > 0; o2 >>= 1) {
        if ((int)threadIdx.x < o2) red[threadIdx.x] += red[threadIdx.x + o2];
        __syncthreads();
    }
    const float nrm = red[0] > 0.0 ? (float)sqrt(red[0]) : 1.f;
    for (int c = threadIdx.x; c < d; c += 256) o[c] = o[c] / nrm;      // each thread rescales what it wrote itself
}

}  // namespace

extern "C" {

int ivr_index_search_lists(ivr_index *x, const int64_t *list_off, int nlist, const float *q, int nq, const int64_t *assign, int p,
                           int64_t max_probe_rows, int k, int normalize_q, float *D, int64_t *I, ivr_stream stream) {
    IVR_REQUIRE(x && list_off && q && assign && D && I, "ivr_index_search_lists: NULL argument");
    IVR_REQUIRE(nlist >= 1 && nq >= 1 && p >= 1, "ivr_index_search_lists: nlist=%d nq=%d p=%d", nlist, nq, p);
    IVR_REQUIRE(k >= 1 && k <= IVR_MAX_K, "ivr_index_search_lists: k=%d outside [1,%d]", k, IVR_MAX_K);
    IVR_REQUIRE(max_probe_rows >= 0, "ivr_index_search_lists: max_probe_rows=%lld", (long long)max_probe_rows);
    hipStream_t s = (hipStream_t)stream;
    std::lock_guard<std::mutex> lk(x->mu);
    IVR_HIP(hipSetDevice(x->ctx->device));
    const int64_t qstride = std::min(max_probe_rows, x->ntotal);
    ProbeTables &pt = x->ivf;
    int chunk;
    int64_t nkeys;
    int rc = ivr_reserve_queries(x, (int)ivr_ceil_div(nq, 16));
    if (rc == IVR_OK) rc = pt.plan(nq, p, qstride, nlist, &chunk, &nkeys);
    if (rc != IVR_OK) return rc;
    rc = ivr_launch_tile_rows(x, x->qtiled, q, 0, nq, normalize_q, nullptr, s);
    if (rc != IVR_OK) return rc;
    const size_t lds = (size_t)16 * x->dp * 4;
    rc = ivr_func_max_lds(reinterpret_cast<const void *>(list_scan_kernel), (int)lds);
    if (rc != IVR_OK) return rc;
    // row splits of a list: 256 rows each, for a list as long as everything one query may probe; at most 64, longer lists loop
    const unsigned ysplit = (unsigned)std::max<int64_t>(1, std::min<int64_t>(64, ivr_ceil_div(qstride, 256)));
    for (int q0 = 0; q0 < nq; q0 += chunk) {
        const int nqc = std::min(chunk, nq - q0);
        const int64_t npairs = (int64_t)nqc * p;
        const int64_t *a = assign + (int64_t)q0 * p;
        {
            IvrProf prof("ivf_probe_tables", s, (double)npairs * 48, true);
            rc = pt.build(a, p, nqc, list_off, nlist, x->ntotal, qstride, s);
            if (rc != IVR_OK) return rc;
            IVR_LAUNCH_CHECK();
        }
        if (x->ntotal > 0 && qstride > 0) {
            ListScan ls{reinterpret_cast<const float4 *>(x->data), reinterpret_cast<const float4 *>((const float *)x->qtiled), x->dp4, nlist, q0, nqc,
                        x->ntotal, list_off, pt.pair_off(), pt.tile_off(nlist), pt.pair_q, pt.pair_slot, pt.keys, nkeys};
            IvrProf prof("ivf_list_scan", s, 0.0);
            hipLaunchKernelGGL(list_scan_kernel, dim3((unsigned)ProbeTables::tiles(nlist, npairs), ysplit), dim3(256), lds, s, ls);
            IVR_LAUNCH_CHECK();
        }
        IvrProf prof("select_final", s, (double)nqc * qstride * 8, true);
        pt.select(nqc, k, qstride, D + (int64_t)q0 * k, I + (int64_t)q0 * k, x->has_ids ? x->ids : nullptr, s);
        IVR_LAUNCH_CHECK();
    }
    return IVR_OK;
}

int ivr_segment_mean(ivr_ctx *ctx, const float *rows, int64_t n, const int64_t *seg_off, int nseg, int d, int normalize, float *out,
                     ivr_stream stream) {
    IVR_REQUIRE(ctx && seg_off && out && (rows || n == 0), "ivr_segment_mean: NULL argument");
    IVR_REQUIRE(n >= 0 && nseg >= 1 && d >= 1, "ivr_segment_mean: n=%lld nseg=%d d=%d", (long long)n, nseg, d);
    IVR_HIP(hipSetDevice(ctx->device));
    hipStream_t s = (hipStream_t)stream;
    IvrProf prof("segment_mean", s, (double)n * d * 4 + (double)nseg * d * 4, true);
    hipLaunchKernelGGL(segment_mean_kernel, dim3((unsigned)nseg), dim3(256), 0, s, rows, seg_off, n, d, normalize, out);
    IVR_LAUNCH_CHECK();
    return IVR_OK;
}

}  // extern "C"
