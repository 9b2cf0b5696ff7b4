// What the flat coded indexes share on the device: ivr_bin_index (search_binary.hip, scanned by search_pq.hip too), ivr_sq_index
// (search_sq.hip) and ivr_pqfs_index (search_pqfs.hip).
//   CodeRows     the growable row store with the bodies of _add, _get_codes and _reset
//   GroupTopK    the two-level top-k of a coded scan: workspace, chunk plan, the two selections, the integer finish and the chunk loop
// Both are defined in search_coded.hip, which alone emits the kernels they launch.  An index supplies its layout (granule,
// group_words), its pack and unpack kernels, its scan kernel and its keys kernel.  DESIGN.md section 4, "The coded-index layer".
// Not part of the C ABI.
#pragma once
#include "ivr_common.h"
#include "search_internal.h"

#include <cstdio>
#include <functional>

// The growable row store of a coded index: whatever the layout inside, 64 rows are group_words 16-byte words and the rows of one
// granule are contiguous.  Growing zero-fills the new block and copies the granules that hold rows.
struct CodeRows {
    ivr_ctx *ctx = nullptr;
    int granule = 0;                     // rows the capacity is a multiple of (itself a multiple of 64)
    int64_t group_words = 0;
    int64_t cap = 0, ntotal = 0;
    uint4 *data = nullptr;               // [cap / 64][group_words]
    std::mutex mu;
    ~CodeRows() { (void)hipFree(data); }
    size_t bytes(int64_t rows) const { return (size_t)ivr_ceil_div(rows, 64) * group_words * sizeof(uint4); }
    int grow(int64_t rows);              // a block of at least `rows` rows (one granule at least) that takes over the stored rows
    // room for n more rows: when they do not fit, wait for the device (work in flight may still read the old block) and grow to
    // max(ntotal + n, 1.5 cap).  what: the caller's name, for the message of an index that would exceed 2^31 rows
    int reserve_for_add(int64_t n, const char *what);
    // The bodies of the entry points; what: the entry point's name, for the messages.
    // Append n rows: the checks, the lock, room for the rows, then pack() launches the index's pack kernel for rows ntotal ..
    // ntotal + n of data; ntotal advances once the launch is accepted
    int add(const char *what, const void *codes, int64_t n, const std::function<void()> &pack);
    // the checks of rows [start, start + n) under the lock, then unpack() launches the index's unpack kernel
    int get_codes(const char *what, int64_t start, int64_t n, const void *out, const std::function<void()> &unpack);
    // No rows.  zero_fill: always wait for the device and clear the block (a layout whose scans read the pad bits of stored rows);
    // otherwise an empty store returns at once and the bytes stay (every kernel masks the rows at or beyond ntotal by number)
    int reset(bool zero_fill);
};

// The two-level top-k of a coded scan: per chunk of queries the scan leaves the best score of every 64-row group in gmax,
// select_topk_kernel picks the best ksel groups into sel, their rows are re-scored into keys and select_topk_kernel orders those.
// Grow-only workspace.
struct GroupTopK {
    static constexpr int kMaxChunk = 4096;               // queries per chunk at most
    static constexpr int64_t kChunkKeys = 1ll << 25;     // keys and group maxima of a chunk (256 + 128 MiB), or one pass's if more
    DevMem gmax;                         // [chunk][mstride] 4-byte entries (float or int32): best score of each 64-row group
    DevBuf<uint32_t> sel;                // [chunk][ksel]: the selected groups, 0xFFFFFFFF = none
    DevBuf<uint64_t> keys;               // [chunk][ksel * 64]: (ordered score, ~row) of the rows of the selected groups
    int64_t mstride = 0;                 // the plan of the search under way
    int ksel = 0, qc = 0;
    // every result slot (-FLT_MAX, -1): the answer of an empty index
    static int absent(int nq, int k, float *D, int64_t *I, hipStream_t s);
    // The plan of a search of nq queries for k rows over ngroups > 0 groups whose scan takes `pass` queries at a time: mstride =
    // ngroups rounded up to 64, ksel = min(k, ngroups), qc = queries per chunk (whole passes, at least one); reserves one chunk
    int plan(int nq, int k, int64_t ngroups, int pass);
    // the launches of a chunk of nqc queries that are the same for every index (the caller checks them)
    void select_groups(bool int32_maxima, int nqc, int64_t ngroups, hipStream_t s);      // gmax -> sel
    void select_rows(int nqc, int k, float *D, int64_t *I, hipStream_t s);               // keys -> D (the key's high word), I
    // D = float(acc) * scale + bias of the slot's query, from the int32 acc that select_rows left in D as the key's high word
    static void finish(float *D, const int64_t *I, const float *scale, const float *bias, int64_t n, int k, hipStream_t s);

    // The chunk loop of a planned search -> D, I [nq][k].  Per chunk of nqc queries from query c0 on: scan(c0, nqc) fills gmax
    // (an error code ends the search), select_groups, keys(c0, nqc, npairs) fills keys for the npairs = nqc * ksel selected
    // (query, group) pairs, select_rows, and with scale != NULL finish.  scale == NULL: float maxima and scores (a table-lookup sum);
    // otherwise int32 accumulators throughout.  scan and keys open their own profiling scopes; the shared launches are named
    // <prefix>_select_groups, <prefix>_select_rows and <prefix>_finish.  what: the entry point's name, for the message
    template <typename Scan, typename Keys>
    int run(const char *what, const char *prefix, int nq, int k, int64_t ngroups, float *D, int64_t *I, const float *scale, const float *bias,
            hipStream_t s, Scan &&scan, Keys &&keys) {
        char groups_name[32] = "", rows_name[32] = "", finish_name[32] = "";
        if (ivr_prof_level() >= 2) {     // the shared launches are minor scopes: their names are only read from this level on
            snprintf(groups_name, sizeof groups_name, "%s_select_groups", prefix);
            snprintf(rows_name, sizeof rows_name, "%s_select_rows", prefix);
            snprintf(finish_name, sizeof finish_name, "%s_finish", prefix);
        }
        for (int c0 = 0; c0 < nq; c0 += qc) {            // c0 is a multiple of the scan's pass
            const int nqc = std::min(qc, nq - c0);
            if (int rc = scan(c0, nqc)) return rc;
            {
                IvrProf prof(groups_name, s, (double)nqc * ngroups * 4, true);
                select_groups(scale != nullptr, nqc, ngroups, s);
            }
            keys(c0, nqc, (int64_t)nqc * ksel);
            float *Dc = D + (int64_t)c0 * k;
            int64_t *Ic = I + (int64_t)c0 * k;
            {
                IvrProf prof(rows_name, s, (double)nqc * ksel * 64 * 8, true);
                select_rows(nqc, k, Dc, Ic, s);
            }
            if (scale) {
                const int64_t n = (int64_t)nqc * k;
                IvrProf prof(finish_name, s, (double)n * 16, true);
                finish(Dc, Ic, scale + c0, bias + c0, n, k, s);
            }
            if (hipGetLastError() != hipSuccess) return ivr_fail(IVR_ERR_HIP, "%s: launch failed", what);
        }
        return IVR_OK;
    }
};

// ---- binary codes (search_binary.hip) and the product-quantisation scan over the same storage (search_pq.hip) -----------------
constexpr int kBinBlockRows = 256;       // rows per workgroup block: one row per lane, four 64-row groups (the store's granule)
constexpr int kBinMaxChunk = 64;         // queries per chunk at most
constexpr int kBinHistLds = 48 * 1024;   // LDS of the histogram pass: (nbits + 1) bins of 4 bytes per query of a chunk

struct ivr_bin_index : CodeRows {        // data: [cap / 64][w16][64], group_words = 64 w16
    int nbits = 0, code_size = 0, w16 = 0;
    // search workspace (grow-only)
    DevBuf<uint4> q;                     // [nq][w16] staged queries, row-major
    DevBuf<uint32_t> hist;               // [chunk][nbits + 1]
    DevBuf<uint32_t> thr;                // [chunk][4]: t, need, below
    DevBuf<uint32_t> cnt;                // [2][chunk][groups]: rows below t / at t per 64-row group, then their exclusive prefix
    DevBuf<uint64_t> cand;               // [chunk][k]: (distance << 32 | row) of the chosen rows, kBinEmpty elsewhere
    GroupTopK pq;                        // product-quantisation scan (ivr_bin_index_search_pq, search_pq.hip): float maxima

    int chunk() const { return std::max(1, std::min(kBinMaxChunk, kBinHistLds / (4 * (nbits + 1)))); }
};
