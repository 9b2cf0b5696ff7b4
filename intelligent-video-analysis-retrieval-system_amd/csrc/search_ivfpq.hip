// Inverted lists over product-quantised codes (faiss IndexIVFPQ, inner product, 8-bit codes): the list store (ivr_ivfpq_set_lists /
// _get_codes) and the probed table-lookup top-k (ivr_ivfpq_search).  DESIGN.md section 4, "inverted lists over PQ codes"; the
// definitions are the numpy functions ivfpq_pack_ref, ivfpq_unpack_ref and ivfpq_scan_ref of ivr_amd/ivfpq.py.
//
// Storage.  A code is M bytes (search_pq.hip).  The store is a ListRows (search_lists.h): the codes ordered by list, every list padded
// to whole 64-row groups, list l owning the groups [goff[l], goff[l + 1]), goff = the exclusive prefix of ceil(size / 64).  Inside a group the layout is that of
// ivr_bin_index (search_binary.hip): W = 1, 2, 3, 4 or 8 words of 16 bytes per row, word w of the row in lane i at
// data[g * W * 64 + w * 64 + i], pad bytes and pad rows zero, so bin_load_row loads one group of ONE list into a wave.  A row's
// packed position is 64 g + i; ids[position] is its label, -1 on a pad row.  Positions stay below 2^32 (they are the low word of a key).
//
// Search, per chunk of queries, all on the caller's stream and without a host round trip:
//   ivfpq_probe   one wave per query over its ascending assign row: gpre[q][j] = the 64-row groups of the valid, first-mentioned
//                 entries in front of entry j (an exclusive prefix; a skipped entry adds nothing), qgroups[q] = their total
//   ivfpq_scan    workgroup (b, q), 8 waves: the M x 256 table of query q in LDS (M KiB), then the query's groups b of gridDim.x
//                 shares, each wave a contiguous run of them: the wave finds the entry of its first group by counting gpre, walks
//                 forward from there, and every lane scores one row: coarse[q][j] first, then the table entries in ascending m.
//                 Key (ordered score << 32) | ~position at slot 64 u + lane of the query's stretch, u = the group's number among
//                 the query's groups; 0 for a pad row
//   select_topk   one workgroup per query over its stretch; labels through ids (OUT_DI_IDS)
// Equal scores rank the lower position first: the lower list, and inside a list the row added earlier.
#include "ivr_common.h"
#include "search_internal.h"
#include "search_lists.h"
#include "search_select.h"

namespace {

constexpr int kIvfpqKsub = 256;              // centroids per slice (8-bit codes)
constexpr int kIvfpqScanThreads = 512;       // the scan's workgroup: 8 waves share one LDS image of one query's table
constexpr int kIvfpqProbeQueries = 4;        // queries (waves) per workgroup of the probe kernel
constexpr int kIvfpqMaxChunk = 16384;        // queries per chunk at most (the scan's grid is (shares, queries))
// 64-row groups a scan workgroup takes per copy of a query's table.  Loading the table costs about as many LDS operations as scoring 4
// groups; 8, 32, 128 and 512 were measured (tools/bench_ivfpq.py --ab; figures in DESIGN.md section 4, "inverted lists over PQ codes",
// "Share of the scan"): 128 and 512 are level, fewer lose at many queries, and up to 64 queries the share is set by filling the device
constexpr int kIvfpqGroupsPerWg = 128;

int ivfpq_words(int M) {
    const int w = (M + 15) / 16;
    return w <= 4 ? w : 8;
}

// bytes [b0, b0 + 4) of a code as one little-endian word, zero past M
__device__ __forceinline__ uint32_t ivfpq_code_word(const uint8_t *__restrict__ p, int b0, int M, bool vec) {
    if (vec && b0 + 4 <= M) return *reinterpret_cast<const uint32_t *>(p + b0);
    uint32_t x = 0;
    for (int b = 0; b < 4; ++b)
        if (b0 + b < M) x |= (uint32_t)p[b0 + b] << (8 * b);
    return x;
}

// list-ordered row-major codes [n][M] and labels [n] -> the packed layout.  One thread per (packed row, word), the row fastest; every
// word of every group is written (pads zero), and word 0's thread writes the label (-1 on a pad row)
__global__ __launch_bounds__(256) void ivfpq_pack_kernel(const uint8_t *__restrict__ codes, const int64_t *__restrict__ src_ids,
                                                         const int64_t *__restrict__ list_off, const int64_t *__restrict__ goff, int nlist,
                                                         int64_t ngroups, int M, int w16, int vec, uint4 *__restrict__ data,
                                                         int64_t *__restrict__ ids) {
    const int64_t t = blockIdx.x * 256ll + threadIdx.x;
    const int lane = (int)(t & 63);
    const int64_t gw = t >> 6;
    const int w = (int)(gw % w16);
    const int64_t g = gw / w16;
    if (g >= ngroups) return;
    const int l = ivr_last_le(goff, nlist, g);
    const int64_t i = (g - goff[l]) * 64 + lane, r = list_off[l] + i;
    const bool valid = r < list_off[l + 1];
    uint4 v = uint4{0u, 0u, 0u, 0u};
    if (valid) {
        const uint8_t *p = codes + r * M;
        v.x = ivfpq_code_word(p, 16 * w + 0, M, vec);
        v.y = ivfpq_code_word(p, 16 * w + 4, M, vec);
        v.z = ivfpq_code_word(p, 16 * w + 8, M, vec);
        v.w = ivfpq_code_word(p, 16 * w + 12, M, vec);
    }
    data[g * w16 * 64 + (int64_t)w * 64 + lane] = v;
    if (w == 0) ids[g * 64 + lane] = valid ? src_ids[r] : -1;
}

// list-ordered rows start .. start + n -> row-major codes [n][M] and / or labels [n].  One thread per (row, 4 bytes)
__global__ __launch_bounds__(256) void ivfpq_unpack_kernel(const uint32_t *__restrict__ data, const int64_t *__restrict__ ids,
                                                           const int64_t *__restrict__ list_off, const int64_t *__restrict__ goff, int nlist,
                                                           int64_t start, int64_t n, int M, int w16, uint8_t *__restrict__ out_codes,
                                                           int64_t *__restrict__ out_ids) {
    const int c4 = (M + 3) / 4;
    const int64_t t = blockIdx.x * 256ll + threadIdx.x;
    const int64_t i = t / c4;
    const int j = (int)(t % c4);
    if (i >= n) return;
    const int64_t r = start + i;
    const int l = ivr_last_le(list_off, nlist, r);
    const int64_t pos = goff[l] * 64 + (r - list_off[l]);
    if (out_codes) {
        const uint32_t x = data[((pos >> 6) * w16 * 64 + (int64_t)(j >> 2) * 64 + (pos & 63)) * 4 + (j & 3)];
        for (int b = 0; b < 4; ++b)
            if (4 * j + b < M) out_codes[i * M + 4 * j + b] = (uint8_t)(x >> (8 * b));
    }
    if (out_ids && j == 0) out_ids[i] = ids[pos];
}

// One wave per query of the chunk.  A query whose lists hold more than max_groups groups (the caller's bound is wrong) probes
// nothing rather than write past its stretch.
__global__ __launch_bounds__(64 * kIvfpqProbeQueries) void ivfpq_probe_kernel(const int64_t *__restrict__ assign, int p, int nqc,
                                                                               const int64_t *__restrict__ goff, int nlist, int64_t max_groups,
                                                                               int *__restrict__ gpre, int *__restrict__ qgroups) {
    const int lane = threadIdx.x & 63;
    const int q = blockIdx.x * kIvfpqProbeQueries + (threadIdx.x >> 6);
    if (q >= nqc) return;
    const int64_t *a = assign + (int64_t)q * p;
    int64_t carry = 0;
    for (int j0 = 0; j0 < p; j0 += 64) {
        const int j = j0 + lane;
        int64_t size = 0;
        if (probe_valid(a, j, p, nlist)) size = goff[a[j] + 1] - goff[a[j]];
        int64_t inc = size;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int64_t t = __shfl_up(inc, o, 64);
            if (lane >= o) inc += t;
        }
        // a prefix past the bound is clamped: qgroups is 0 then and no entry of this row is read
        if (j < p) gpre[(int64_t)q * p + j] = (int)min(carry + inc - size, max_groups);
        carry += __shfl(inc, 63, 64);
    }
    if (lane == 0) qgroups[q] = carry <= max_groups ? (int)carry : 0;
}

// the score of the lane's row against one query's table t ([M][256], LDS): s0, then the entries in ascending m.  The 16 bytes of a
// word, or the 4 of a component, are looked up together wherever M leaves them whole (the lookups do not depend on the additions,
// and a whole word costs one wave-uniform branch)
template <int W>
__device__ __forceinline__ float ivfpq_score_row(const uint4 (&row)[W], const float *__restrict__ t, int M, float s0) {
    float s = s0;
#pragma unroll
    for (int w = 0; w < W; ++w) {
        if (16 * w + 16 <= M) {
            float v[16];
#pragma unroll
            for (int b = 0; b < 16; ++b) v[b] = t[(16 * w + b) * kIvfpqKsub + ((ivr_comp(row[w], b >> 2) >> (8 * (b & 3))) & 255u)];
#pragma unroll
            for (int b = 0; b < 16; ++b) s = s + v[b];
            continue;
        }
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int m0 = 16 * w + 4 * c;
            const uint32_t x = ivr_comp(row[w], c);
            if (m0 + 4 <= M) {
                float v[4];
#pragma unroll
                for (int b = 0; b < 4; ++b) v[b] = t[(m0 + b) * kIvfpqKsub + ((x >> (8 * b)) & 255u)];
#pragma unroll
                for (int b = 0; b < 4; ++b) s = s + v[b];
            } else if (m0 < M) {
#pragma unroll
                for (int b = 0; b < 3; ++b)
                    if (m0 + b < M) s = s + t[(m0 + b) * kIvfpqKsub + ((x >> (8 * b)) & 255u)];
            }
        }
    }
    return s;
}

struct IvfpqScan {
    const uint4 *data;
    const int64_t *ids;          // [groups * 64]: -1 marks a pad row
    const int64_t *goff;         // [nlist + 1]
    const float *T;              // the chunk's tables [nqc][M][256]
    const float *coarse;         // the chunk's coarse scores [nqc][p], or NULL: +0.0
    const int64_t *assign;       // the chunk's ascending assign rows [nqc][p]
    const int *gpre, *qgroups;
    uint64_t *keys;
    int64_t qstride;             // slots of a query's stretch (a multiple of 64)
    int64_t ngroups;             // groups of the store: no group at or past it is read
    int p, M, nlist;
};

template <int W>
__global__ __launch_bounds__(kIvfpqScanThreads) void ivfpq_scan_kernel(IvfpqScan a) {
    extern __shared__ __attribute__((aligned(16))) float lt[];      // [M][256]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int q = blockIdx.y;
    const int total = min(a.qgroups[q], (int)(a.qstride >> 6));
    // the share of this workgroup, then the run of this wave inside it: whole groups, contiguous
    const int per_wg = (total + (int)gridDim.x - 1) / (int)gridDim.x;
    const int b0 = min((int)blockIdx.x * per_wg, total), b1 = min(b0 + per_wg, total);
    if (b0 >= b1) return;                            // the whole workgroup: before the barrier
    const int tab = a.M * kIvfpqKsub;
    {
        const float4 *src = reinterpret_cast<const float4 *>(a.T + (int64_t)q * tab);
        float4 *dst = reinterpret_cast<float4 *>(lt);
        for (int i = tid; i < tab / 4; i += kIvfpqScanThreads) dst[i] = src[i];
    }
    __syncthreads();
    constexpr int kWaves = kIvfpqScanThreads / 64;
    const int per_wave = (b1 - b0 + kWaves - 1) / kWaves;
    const int u0 = min(b0 + wave * per_wave, b1), u1 = min(u0 + per_wave, b1);
    if (u0 >= u1) return;
    const int *gp = a.gpre + (int64_t)q * a.p;
    const int64_t *as = a.assign + (int64_t)q * a.p;
    // entry of group u0: the last j with gpre[j] <= u0 (gpre is ascending and gpre[0] = 0), counted by the whole wave
    int cnt = 0;
    for (int j0 = 0; j0 < a.p; j0 += 64) {
        const int j = j0 + lane;
        cnt += __popcll(__ballot(j < a.p && gp[j] <= u0));
    }
    int j = max(cnt - 1, 0);
    int next = j + 1 < a.p ? gp[j + 1] : total;       // the first group of the entry behind j
    for (int u = u0; u < u1; ++u) {
        while (j + 1 < a.p && next <= u) {           // skipped and empty entries start where their successor does
            ++j;
            next = j + 1 < a.p ? gp[j + 1] : total;
        }
        const int64_t l = as[j];
        const int64_t g = (l >= 0 && l < a.nlist ? a.goff[l] : -1) + (u - gp[j]);
        uint64_t key = 0;
        if (l >= 0 && l < a.nlist && g >= 0 && g < a.ngroups) {      // wave-uniform; always true for a probe table of ivfpq_probe
            uint4 row[W];
            bin_load_row<W>(a.data, g, row);
            const int64_t pos = g * 64 + lane;
            const float s = ivfpq_score_row<W>(row, lt, a.M, a.coarse ? a.coarse[(int64_t)q * a.p + j] : 0.f);
            if (a.ids[pos] >= 0) key = ivr_key(s, (uint32_t)pos);
        }
        a.keys[(int64_t)q * a.qstride + (int64_t)u * 64 + lane] = key;
    }
}

struct SrcIvfpqSlots {     // the keys of query q: slots [q * qstride, q * qstride + 64 qgroups[q]) of the scratch
    const uint64_t *keys;
    const int *qgroups;
    int64_t qstride;
    int64_t n;             // the longest stretch a query of the launch may hold
    __device__ uint64_t key(int q, int64_t i) const { return i < (int64_t)qgroups[q] * 64 ? keys[(int64_t)q * qstride + i] : 0; }
};

}  // namespace

struct ivr_ivfpq : ListRows {          // data: [ngroups][w16][64]; by_size counts groups; chunk_slots: IVR_IVFPQ_CHUNK_SLOTS
    int M = 0, w16 = 0;
    int64_t groups_per_wg = kIvfpqGroupsPerWg;   // IVR_IVFPQ_GROUPS_PER_WG: the scan's share size (A/B switch, read at creation)
    // search scratch of one chunk of queries (grow-only)
    DevBuf<uint64_t> keys;               // [chunk][qstride]
    DevBuf<int> gpre;                    // [chunk][p]
    DevBuf<int> qgroups;                 // [chunk]
};

extern "C" {

int ivr_ivfpq_probe_queries(void) { return kIvfpqProbeQueries; }

int ivr_ivfpq_create(ivr_ctx *ctx, int M, int nlist, ivr_ivfpq **out) {
    IVR_REQUIRE(ctx && out, "ivr_ivfpq_create: NULL argument");
    IVR_REQUIRE(M >= 1 && M <= IVR_PQ_MAX_M, "ivr_ivfpq_create: M=%d outside [1,%d]", M, IVR_PQ_MAX_M);
    IVR_REQUIRE(nlist >= 1 && nlist < (1 << 30), "ivr_ivfpq_create: nlist=%d out of range", nlist);
    IVR_HIP(hipSetDevice(ctx->device));
    ivr_ivfpq *x = new ivr_ivfpq();
    x->M = M;
    x->w16 = ivfpq_words(M);
    x->groups_per_wg = ivr_env_positive("IVR_IVFPQ_GROUPS_PER_WG", kIvfpqGroupsPerWg);
    const int rc = x->init(ctx, nlist, "IVR_IVFPQ_CHUNK_SLOTS");
    if (rc != IVR_OK) {
        delete x;
        return rc;
    }
    *out = x;
    return IVR_OK;
}

int ivr_ivfpq_destroy(ivr_ivfpq *x) {
    delete x;                            // the buffers free themselves
    return IVR_OK;
}

int64_t ivr_ivfpq_ntotal(ivr_ivfpq *x) { return x ? x->ntotal : 0; }

int ivr_ivfpq_set_lists(ivr_ivfpq *x, const uint8_t *codes, const int64_t *ids, const int64_t *list_off, int64_t n, ivr_stream stream) {
    IVR_REQUIRE(x, "ivr_ivfpq_set_lists: NULL argument");
    return x->set_lists("ivr_ivfpq_set_lists", codes, ids, list_off, n, (int64_t)x->w16 * 64, false, [&](int64_t ngroups) {
        const int64_t threads = ngroups * x->w16 * 64;
        const int vec = x->M % 4 == 0 && ((uintptr_t)codes & 3) == 0;
        hipLaunchKernelGGL(ivfpq_pack_kernel, dim3((unsigned)ivr_ceil_div(threads, 256)), dim3(256), 0, (hipStream_t)stream, codes, ids,
                           x->list_off(), x->goff(), x->nlist, ngroups, x->M, x->w16, vec, (uint4 *)x->data, (int64_t *)x->ids);
    });
}

int ivr_ivfpq_reset(ivr_ivfpq *x) {
    IVR_REQUIRE(x, "ivr_ivfpq_reset: NULL index");
    return x->reset("ivr_ivfpq_set_lists");
}

int ivr_ivfpq_get_codes(ivr_ivfpq *x, int64_t start, int64_t n, uint8_t *codes, int64_t *ids, ivr_stream stream) {
    IVR_REQUIRE(x, "ivr_ivfpq_get_codes: NULL argument");
    return x->get_codes("ivr_ivfpq_get_codes", start, n, codes, ids, [&] {
        const int64_t threads = n * ((x->M + 3) / 4);
        hipLaunchKernelGGL(ivfpq_unpack_kernel, dim3((unsigned)ivr_ceil_div(threads, 256)), dim3(256), 0, (hipStream_t)stream,
                           reinterpret_cast<const uint32_t *>((const uint4 *)x->data), (const int64_t *)x->ids, x->list_off(), x->goff(), x->nlist,
                           start, n, x->M, x->w16, codes, ids);
    });
}

int ivr_ivfpq_search(ivr_ivfpq *x, const float *T, const float *coarse, const int64_t *assign, int nq, int p, int k, float *D, int64_t *I,
                     ivr_stream stream) {
    IVR_REQUIRE(x && T && assign && D && I, "ivr_ivfpq_search: NULL argument");
    IVR_REQUIRE(nq >= 1 && p >= 1, "ivr_ivfpq_search: nq=%d p=%d", nq, p);
    IVR_REQUIRE(k >= 1 && k <= IVR_MAX_K, "ivr_ivfpq_search: k=%d outside [1,%d]", k, IVR_MAX_K);
    IVR_REQUIRE(((uintptr_t)T & 15) == 0, "ivr_ivfpq_search: the tables must be 16-byte aligned");
    IVR_REQUIRE(x->w16 <= 8, "ivr_ivfpq_search: %d words per row", x->w16);
    hipStream_t s = (hipStream_t)stream;
    std::lock_guard<std::mutex> lk(x->mu);
    IVR_HIP(hipSetDevice(x->ctx->device));
    // what one query may probe: the groups of its p longest lists
    const int64_t max_groups = x->by_size[(size_t)std::min<int64_t>(p, x->nlist)], qstride = max_groups * 64;
    const int chunk = (int)std::max<int64_t>(1, std::min<int64_t>({(int64_t)nq, (int64_t)kIvfpqMaxChunk, x->chunk_slots / std::max<int64_t>(qstride, 1)}));
    int rc = ivr_reserve({{&x->keys, (size_t)std::max<int64_t>((int64_t)chunk * qstride, 1) * 8}, {&x->gpre, (size_t)chunk * p * 4},
                          {&x->qgroups, (size_t)chunk * 4}});
    if (rc != IVR_OK) return rc;
    const int tab = x->M * kIvfpqKsub;
    const size_t lds = (size_t)tab * sizeof(float);
    for (int q0 = 0; q0 < nq; q0 += chunk) {
        const int nqc = std::min(chunk, nq - q0);
        const int64_t *a = assign + (int64_t)q0 * p;
        {
            IvrProf prof("ivfpq_probe", s, (double)nqc * p * 12, true);
            hipLaunchKernelGGL(ivfpq_probe_kernel, dim3((unsigned)ivr_ceil_div(nqc, kIvfpqProbeQueries)), dim3(64 * kIvfpqProbeQueries), 0, s, a, p,
                               nqc, x->goff(), x->nlist, max_groups, (int *)x->gpre, (int *)x->qgroups);
            IVR_LAUNCH_CHECK();
        }
        if (max_groups > 0) {
            // shares of a query's groups: groups_per_wg groups each, but enough of them that the chunk fills the device twice over,
            // and never less than one group per wave
            const int64_t fill = ivr_ceil_div(2ll * x->ctx->cu_count, nqc);
            const int64_t gx = std::max<int64_t>(1, std::min<int64_t>(ivr_ceil_div(max_groups, kIvfpqScanThreads / 64),
                                                                      std::max<int64_t>(ivr_ceil_div(max_groups, x->groups_per_wg), fill)));
            const IvfpqScan sc{x->data, x->ids, x->goff(), T + (int64_t)q0 * tab, coarse ? coarse + (int64_t)q0 * p : nullptr, a,
                               x->gpre, x->qgroups, x->keys, qstride, x->ngroups, p, x->M, x->nlist};
            bin_with_words(x->w16, [&](auto w) {
                constexpr int W = decltype(w)::value > 8 ? 8 : decltype(w)::value;      // 16 words: refused above
                rc = ivr_func_max_lds(reinterpret_cast<const void *>(ivfpq_scan_kernel<W>), (int)lds);
                if (rc != IVR_OK) return;
                IvrProf prof("ivfpq_scan", s, (double)nqc * max_groups * 64 * x->M);
                hipLaunchKernelGGL(ivfpq_scan_kernel<W>, dim3((unsigned)gx, (unsigned)nqc), dim3(kIvfpqScanThreads), lds, s, sc);
            });
            if (rc != IVR_OK) return rc;
            IVR_LAUNCH_CHECK();
        }
        IvrProf prof("ivfpq_select", s, (double)nqc * qstride * 8, true);
        const SrcIvfpqSlots src{x->keys, x->qgroups, qstride, qstride};
        launch_select<OUT_DI_IDS>(src, nqc, k, SelectOut::to_rows(D + (int64_t)q0 * k, I + (int64_t)q0 * k, 0, x->ids), s);
        IVR_LAUNCH_CHECK();
    }
    return IVR_OK;
}

}  // extern "C"
