// Inverted lists over scalar-quantiser codes (faiss IndexIVFScalarQuantizer, QT_8bit, inner product): the list store
// (ivr_ivfsq_set_lists / _get_codes) and the probed int8 MFMA top-k (ivr_ivfsq_search).  DESIGN.md section 4, "inverted lists over SQ
// codes"; the definitions are the numpy functions ivfsq_pack_ref, ivfsq_unpack_ref and ivfsq_scan_ref of ivr_amd/ivfsq.py.
//
// Storage.  A code is d bytes (search_sq.hip).  The store is a ListRows (search_lists.h): the codes ordered by list, every list padded
// to whole 64-row groups, list l owning the groups [goff[l], goff[l + 1]), goff = the exclusive prefix of ceil(size / 64), and row i
// of the list at the packed position 64 goff[l] + i.  Over the packed positions the layout is that of search_sq.hip: the stored byte is
// c' = code - 128, K is padded with zero bytes to ksteps = ceil(d / 64) steps, and position P sits in tile P / 16, whose piece s holds
// bytes 64 s + 16 c .. + 15 of the row in lane (P & 15) + 16 c: one wave-wide 16-byte load is the A operand of one
// v_mfma_i32_16x16x64_i8.  Pad rows and pad bytes are zero; ids[position] is the row's label, -1 on a pad row.  Positions stay below
// 2^32 (they are the low word of a key).
//
// Search, per chunk of queries, all on the caller's stream and without a host round trip:
//   sq_stage      once per call: t (int16) -> the two int8 halves, tiled per 16 queries (ivr_launch_sq_stage, search_sq.hip)
//   probe tables  ProbeTables::build (search_lists.hip) over the unpadded list sizes: the (query, list) pairs grouped by list, the
//                 16-query pair tiles, one key slot per probed row in the query's own stretch
//   ivfsq_scan    one workgroup per (pair tile, row split): both halves of its up to 16 queries gathered into LDS as B operands, its
//                 waves walk the 16-row tiles of the list; acc = 128 acc_h + acc_l, D = ((float(acc) * scale) + bias) + coarse,
//                 key (ordered D, ~position) into the row's slot
//   select_topk   ProbeTables::select: one workgroup per query over its stretch; labels through ids (OUT_DI_IDS)
// Equal D rank the lower position first: the lower list, and inside a list the row added earlier.
#include "ivr_common.h"
#include "search_internal.h"
#include "search_lists.h"

namespace {

constexpr int kIvfsqMaxD = 1024;             // IVR_SQ_MAX_D: 16256 * 128 * d fits int32 up to here
constexpr int kIvfsqThreads = 256;           // the scan's workgroup: 4 waves share one LDS image of a pair tile's queries
constexpr int kIvfsqSplitTiles = 16;         // 16-row tiles of a list a workgroup takes at a time: 256 rows, four to a wave

// list-ordered row-major codes [n][d] and labels [n] -> the packed layout.  One thread per 16-byte word of the store, in storage
// order; every word of every group is written (pads zero), and the thread of a position's first word writes its label (-1 on a pad row)
__global__ __launch_bounds__(256) void ivfsq_pack_kernel(const uint8_t *__restrict__ codes, const int64_t *__restrict__ src_ids,
                                                         const int64_t *__restrict__ list_off, const int64_t *__restrict__ goff, int nlist,
                                                         int64_t nwords, int d, int ksteps, int vec, uint4 *__restrict__ data,
                                                         int64_t *__restrict__ ids) {
    const int64_t w = blockIdx.x * 256ll + threadIdx.x;
    if (w >= nwords) return;
    const int lane = (int)(w & 63);
    const int s = (int)((w >> 6) % ksteps);
    const int64_t pos = ((w >> 6) / ksteps) * 16 + (lane & 15);
    const int b0 = 64 * s + 16 * (lane >> 4);
    const int l = ivr_last_le(goff, nlist, pos >> 6);
    const int64_t r = list_off[l] + (pos - goff[l] * 64);
    const bool valid = r < list_off[l + 1];
    uint4 v = uint4{0u, 0u, 0u, 0u};
    if (valid && b0 < d) {
        const uint8_t *p = codes + r * d + b0;
        if (vec && b0 + 16 <= d) {
            v = *reinterpret_cast<const uint4 *>(p);
            v.x ^= 0x80808080u;
            v.y ^= 0x80808080u;
            v.z ^= 0x80808080u;
            v.w ^= 0x80808080u;
        } else {
            uint32_t x[4] = {0u, 0u, 0u, 0u};
            for (int b = 0; b < 16; ++b)
                if (b0 + b < d) x[b >> 2] |= (uint32_t)(p[b] ^ 0x80u) << (8 * (b & 3));
            v = uint4{x[0], x[1], x[2], x[3]};
        }
    }
    data[w] = v;
    if (b0 == 0) ids[pos] = valid ? src_ids[r] : -1;
}

// list-ordered rows start .. start + n -> row-major codes [n][d] (unsigned) and / or labels [n].  One thread per (row, 16 bytes)
__global__ __launch_bounds__(256) void ivfsq_unpack_kernel(const uint4 *__restrict__ data, const int64_t *__restrict__ ids,
                                                           const int64_t *__restrict__ list_off, const int64_t *__restrict__ goff, int nlist,
                                                           int64_t start, int64_t n, int d, int ksteps, uint8_t *__restrict__ out_codes,
                                                           int64_t *__restrict__ out_ids) {
    const int nch = (d + 15) / 16;
    const int64_t t = blockIdx.x * 256ll + threadIdx.x;
    const int64_t i = t / nch;
    const int c = (int)(t % nch);
    if (i >= n) return;
    const int64_t r = start + i;
    const int l = ivr_last_le(list_off, nlist, r);
    const int64_t pos = goff[l] * 64 + (r - list_off[l]);
    if (out_codes) {
        const uint4 v = data[((pos >> 4) * ksteps + (c >> 2)) * 64 + (pos & 15) + 16 * (c & 3)];
        const uint32_t x[4] = {v.x, v.y, v.z, v.w};
        uint8_t *o = out_codes + i * d + 16 * c;
        for (int b = 0; b < 16; ++b)
            if (16 * c + b < d) o[b] = (uint8_t)((x[b >> 2] >> (8 * (b & 3))) ^ 0x80u);
    }
    if (out_ids && c == 0) out_ids[i] = ids[pos];
}

struct IvfsqScan {
    const uint4 *data;           // the int8 tiles of the store: [ngroups * 4][ksteps][64]
    const uint4 *qh, *ql;        // both halves of the call's staged queries: [query tiles][ksteps][64]
    const float *scale, *bias;   // the chunk's [nqc]
    const float *coarse;         // the chunk's [nqc][p], or NULL: +0.0
    const int64_t *assign;       // the chunk's ascending assign rows [nqc][p]
    int ksteps, nlist, p;
    int q0, nqc;                 // the chunk's queries: q0 .. q0 + nqc of the staged buffers; pair_q counts from q0
    int64_t ntotal, ngroups;
    const int64_t *list_off, *goff;
    const int64_t *pair_off, *tile_off;
    const int *pair_q;
    const int64_t *pair_slot;
    uint64_t *keys;
    int64_t nkeys;               // slots of the scratch: nothing is written at or past it
};

// Workgroup (w, y): pair tile w = up to 16 queries that probe one list, found by a binary search of w in tile_off; of the list's
// 16-row tiles (they start at tile 4 goff[l]: a list owns whole groups) it takes number 16 y .. 16 y + 15, then those 16 gridDim.y
// further on, four to a wave, and exits at once when the list ends before its first tile.  Both halves of the queries are gathered
// from the staged tiles into LDS in the B-operand layout (element (s, lane) = the 16 bytes of query (lane & 15), K bytes 64 s +
// 16 (lane >> 4) ..; unused columns zero): consecutive threads write consecutive 16-byte words, and the scan reads them back the
// same way, one ds_read_b128 per lane over 1 KiB contiguous.  In an accumulator tile lane l holds query column l & 15 and rows
// 4 (l >> 4) + reg.  Rows at or past the list's size are pad rows: no key.  Every tile read lies inside the list's own groups.
__global__ __launch_bounds__(kIvfsqThreads) void ivfsq_scan_kernel(IvfsqScan a) {
    SQ_NO_CONTRACT
    extern __shared__ uint4 lq[];                    // [half][ksteps][64]
    __shared__ int s_q[16];
    __shared__ int64_t s_slot[16];
    __shared__ float s_scale[16], s_bias[16], s_coarse[16];
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
    const int64_t g0 = a.goff[lo];
    const int64_t size = min(r1 - r0, (a.ngroups - g0) * 64);        // never past the store, whatever the offsets say
    const int64_t ntiles = (size + 15) >> 4;
    if (size <= 0 || cnt <= 0 || g0 < 0 || (int64_t)blockIdx.y * kIvfsqSplitTiles >= ntiles) return;
    if (threadIdx.x < 16) {
        const bool on = (int)threadIdx.x < cnt;
        int q = on ? a.pair_q[p0 + threadIdx.x] : -1;
        if (q < 0 || q >= a.nqc) q = -1;
        float sc = 0.f, bi = 0.f, co = 0.f;
        if (q >= 0) {
            sc = a.scale[q];
            bi = a.bias[q];
            if (a.coarse) {
                // the first mention of the list in the query's ascending row: a lower-bound search
                const int64_t *as = a.assign + (int64_t)q * a.p;
                int j0 = 0, j1 = a.p;
                while (j0 < j1) {
                    const int mid = (j0 + j1) >> 1;
                    if (as[mid] < lo) j0 = mid + 1;
                    else j1 = mid;
                }
                co = a.coarse[(int64_t)q * a.p + min(j0, a.p - 1)];
            }
        }
        s_q[threadIdx.x] = q;
        s_slot[threadIdx.x] = on ? a.pair_slot[p0 + threadIdx.x] : 0;
        s_scale[threadIdx.x] = sc;
        s_bias[threadIdx.x] = bi;
        s_coarse[threadIdx.x] = co;
    }
    __syncthreads();
    const int tw = a.ksteps * 64;
    for (int i = threadIdx.x; i < tw; i += kIvfsqThreads) {
        const int q = s_q[i & 15];
        const int qg = a.q0 + q;
        const int64_t at = (int64_t)(qg >> 4) * tw + (i & ~15) + (qg & 15);
        lq[i] = q >= 0 ? a.qh[at] : uint4{0u, 0u, 0u, 0u};
        lq[tw + i] = q >= 0 ? a.ql[at] : uint4{0u, 0u, 0u, 0u};
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int col = lane & 15;
    const bool live = s_q[col] >= 0;
    const float sc = s_scale[col], bi = s_bias[col], co = s_coarse[col];
    const int64_t slot0 = s_slot[col];
    for (int64_t tb = (int64_t)blockIdx.y * kIvfsqSplitTiles; tb < ntiles; tb += (int64_t)gridDim.y * kIvfsqSplitTiles)
    for (int64_t t = tb + wave; t < min(tb + kIvfsqSplitTiles, ntiles); t += kIvfsqThreads / 64) {
        const uint4 *at = a.data + (g0 * 4 + t) * tw + lane;
        i32x4 ah = {0, 0, 0, 0}, al = {0, 0, 0, 0};
        int s = 0;
        for (; s + 4 <= a.ksteps; s += 4) {
            uint4 av[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) av[u] = at[(s + u) * 64];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                ah = __builtin_amdgcn_mfma_i32_16x16x64_i8(sq_frag(av[u]), sq_frag(lq[(s + u) * 64 + lane]), ah, 0, 0, 0);
                al = __builtin_amdgcn_mfma_i32_16x16x64_i8(sq_frag(av[u]), sq_frag(lq[tw + (s + u) * 64 + lane]), al, 0, 0, 0);
            }
        }
        for (; s < a.ksteps; ++s) {
            const i32x4 av = sq_frag(at[s * 64]);
            ah = __builtin_amdgcn_mfma_i32_16x16x64_i8(av, sq_frag(lq[s * 64 + lane]), ah, 0, 0, 0);
            al = __builtin_amdgcn_mfma_i32_16x16x64_i8(av, sq_frag(lq[tw + s * 64 + lane]), al, 0, 0, 0);
        }
        if (!live) continue;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int64_t i = t * 16 + (lane >> 4) * 4 + r;          // the row's number in its list
            if (i >= size) continue;
            const int32_t acc = sq_combine(ah[r], al[r]);
            // the definition's four float32 steps, each rounded by itself (no contraction in this body)
            const float f = (float)acc;
            const float m = f * sc;
            const float b = m + bi;
            const float D = b + co;
            const int64_t sl = slot0 + i;
            if (sl >= 0 && sl < a.nkeys) a.keys[sl] = ivr_key(D, (uint32_t)(g0 * 64 + i));
        }
    }
}

}  // namespace

struct ivr_ivfsq : ListRows {          // data: [ngroups * 4][ksteps][64]; by_size counts rows; chunk_slots: IVR_IVFSQ_CHUNK_SLOTS
    int d = 0, ksteps = 0;
    // search scratch (grow-only): the staged queries of a call, then the tables of one chunk of queries
    DevBuf<uint4> qh, ql;                // [query tiles][ksteps][64]
    ProbeTables pt;                      // keys: (ordered D, ~position) of every probed row
    int64_t tile_words() const { return (int64_t)ksteps * 64; }
};

extern "C" {

int ivr_ivfsq_create(ivr_ctx *ctx, int d, int nlist, ivr_ivfsq **out) {
    IVR_REQUIRE(ctx && out, "ivr_ivfsq_create: NULL argument");
    IVR_REQUIRE(d >= 1 && d <= kIvfsqMaxD, "ivr_ivfsq_create: d=%d outside [1,%d]", d, kIvfsqMaxD);
    IVR_REQUIRE(nlist >= 1 && nlist < (1 << 30), "ivr_ivfsq_create: nlist=%d out of range", nlist);
    IVR_HIP(hipSetDevice(ctx->device));
    ivr_ivfsq *x = new ivr_ivfsq();
    x->d = d;
    x->ksteps = (d + 63) / 64;
    const int rc = x->init(ctx, nlist, "IVR_IVFSQ_CHUNK_SLOTS");
    if (rc != IVR_OK) {
        delete x;
        return rc;
    }
    x->pt.chunk_slots = x->chunk_slots;
    *out = x;
    return IVR_OK;
}

int ivr_ivfsq_destroy(ivr_ivfsq *x) {
    delete x;                            // the buffers free themselves
    return IVR_OK;
}

int64_t ivr_ivfsq_ntotal(ivr_ivfsq *x) { return x ? x->ntotal : 0; }

int ivr_ivfsq_set_lists(ivr_ivfsq *x, const uint8_t *codes, const int64_t *ids, const int64_t *list_off, int64_t n, ivr_stream stream) {
    IVR_REQUIRE(x, "ivr_ivfsq_set_lists: NULL argument");
    return x->set_lists("ivr_ivfsq_set_lists", codes, ids, list_off, n, 4 * x->tile_words(), true, [&](int64_t ngroups) {
        const int64_t nwords = ngroups * 4 * x->tile_words();
        const int vec = x->d % 16 == 0 && ((uintptr_t)codes & 15) == 0;
        hipLaunchKernelGGL(ivfsq_pack_kernel, dim3((unsigned)ivr_ceil_div(nwords, 256)), dim3(256), 0, (hipStream_t)stream, codes, ids,
                           x->list_off(), x->goff(), x->nlist, nwords, x->d, x->ksteps, vec, (uint4 *)x->data, (int64_t *)x->ids);
    });
}

int ivr_ivfsq_reset(ivr_ivfsq *x) {
    IVR_REQUIRE(x, "ivr_ivfsq_reset: NULL index");
    return x->reset("ivr_ivfsq_set_lists");
}

int ivr_ivfsq_get_codes(ivr_ivfsq *x, int64_t start, int64_t n, uint8_t *codes, int64_t *ids, ivr_stream stream) {
    IVR_REQUIRE(x, "ivr_ivfsq_get_codes: NULL argument");
    return x->get_codes("ivr_ivfsq_get_codes", start, n, codes, ids, [&] {
        const int64_t threads = n * ((x->d + 15) / 16);
        hipLaunchKernelGGL(ivfsq_unpack_kernel, dim3((unsigned)ivr_ceil_div(threads, 256)), dim3(256), 0, (hipStream_t)stream,
                           (const uint4 *)x->data, (const int64_t *)x->ids, x->list_off(), x->goff(), x->nlist, start, n, x->d, x->ksteps, codes,
                           ids);
    });
}

int ivr_ivfsq_search(ivr_ivfsq *x, const int16_t *t, const float *scale, const float *bias, const float *coarse, const int64_t *assign, int nq,
                     int p, int k, float *D, int64_t *I, ivr_stream stream) {
    IVR_REQUIRE(x && t && scale && bias && assign && D && I, "ivr_ivfsq_search: NULL argument");
    IVR_REQUIRE(nq >= 1 && p >= 1, "ivr_ivfsq_search: nq=%d p=%d", nq, p);
    IVR_REQUIRE(k >= 1 && k <= IVR_MAX_K, "ivr_ivfsq_search: k=%d outside [1,%d]", k, IVR_MAX_K);
    hipStream_t s = (hipStream_t)stream;
    std::lock_guard<std::mutex> lk(x->mu);
    IVR_HIP(hipSetDevice(x->ctx->device));
    const int nlist = x->nlist;
    // what one query may probe: the rows of its p longest lists
    const int64_t qstride = x->by_size[(size_t)std::min<int64_t>(p, nlist)];
    const int64_t tw = x->tile_words(), qtiles = ivr_ceil_div(nq, 16);
    ProbeTables &pt = x->pt;
    int chunk;
    int64_t nkeys;
    int rc = ivr_reserve({{&x->qh, (size_t)(qtiles * tw) * sizeof(uint4)}, {&x->ql, (size_t)(qtiles * tw) * sizeof(uint4)}});
    if (rc == IVR_OK) rc = pt.plan(nq, p, qstride, nlist, &chunk, &nkeys);
    if (rc != IVR_OK) return rc;
    const size_t lds = (size_t)2 * tw * sizeof(uint4);               // 2 KiB per K step: 32 KiB at d = 1024
    rc = ivr_func_max_lds(reinterpret_cast<const void *>(ivfsq_scan_kernel), (int)lds);
    if (rc != IVR_OK) return rc;
    {
        IvrProf prof("ivfsq_stage", s, (double)nq * x->d * 2, true);
        ivr_launch_sq_stage(t, nq, x->d, x->ksteps, qtiles, x->qh, x->ql, s);
        IVR_LAUNCH_CHECK();
    }
    // row splits of a list: 256 rows each, for a list as long as everything one query may probe; at most 64, longer lists loop
    const unsigned ysplit = (unsigned)std::max<int64_t>(1, std::min<int64_t>(64, ivr_ceil_div(qstride, 16 * kIvfsqSplitTiles)));
    for (int q0 = 0; q0 < nq; q0 += chunk) {
        const int nqc = std::min(chunk, nq - q0);
        const int64_t npairs = (int64_t)nqc * p;
        const int64_t *a = assign + (int64_t)q0 * p;
        {
            IvrProf prof("ivfsq_probe_tables", s, (double)npairs * 48, true);
            rc = pt.build(a, p, nqc, x->list_off(), nlist, x->ntotal, qstride, s);
            if (rc != IVR_OK) return rc;
            IVR_LAUNCH_CHECK();
        }
        if (x->ntotal > 0 && qstride > 0) {
            const IvfsqScan sc{x->data, x->qh, x->ql, scale + q0, bias + q0, coarse ? coarse + (int64_t)q0 * p : nullptr, a, x->ksteps, nlist, p,
                               q0, nqc, x->ntotal, x->ngroups, x->list_off(), x->goff(), pt.pair_off(), pt.tile_off(nlist), pt.pair_q, pt.pair_slot,
                               pt.keys, nkeys};
            IvrProf prof("ivfsq_list_scan", s, 0.0);
            hipLaunchKernelGGL(ivfsq_scan_kernel, dim3((unsigned)ProbeTables::tiles(nlist, npairs), ysplit), dim3(kIvfsqThreads), lds, s, sc);
            IVR_LAUNCH_CHECK();
        }
        IvrProf prof("ivfsq_select", s, (double)nqc * qstride * 8, true);
        pt.select(nqc, k, qstride, D + (int64_t)q0 * k, I + (int64_t)q0 * k, x->ids, s);
        IVR_LAUNCH_CHECK();
    }
    return IVR_OK;
}

}  // extern "C"
