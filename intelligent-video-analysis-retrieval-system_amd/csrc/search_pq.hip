// Product quantisation (faiss IndexPQ, inner product, 8-bit codes): the encoder (ivr_pq_encode), the lookup tables of a batch of
// queries (ivr_pq_tables) and the table-lookup top-k over the stored codes (ivr_bin_index_search_pq).  DESIGN.md section 4, "product
// quantisation"; the definitions are the numpy functions pq_encode_ref, pq_tables_ref and pq_scan_ref of ivr_amd/pq.py.
//
// Storage.  A code is M bytes, byte m = the centroid of slice m.  The codes live in an ivr_bin_index of 8 M bits (search_binary.hip:
// W = 1, 2, 3, 4 or 8 words of 16 bytes per row, interleaved per 64 rows, pad bytes zero), so add / get_codes / reset are that
// object's and one lane holds one row: byte m of a row is byte m & 3 of component (m >> 2) & 3 of word m >> 4.
//
// Search, per chunk of queries, all on the caller's stream:
//   pq_scan     a workgroup of 8 waves holds the tables of a group of queries in LDS ([queries][M][256] floats, M KiB per query) and
//               walks the rows; a wave scores two 64-row groups at a time (one from 5 words per row on, where two rows no longer
//               fit the registers), so that the dependent additions of one row overlap with the lookups of the other, and every
//               code word it has loaded serves all queries of the group.  A score is
//               ((T[0][c0] + T[1][c1]) + ...) in ascending m.  Written: the best score of each (query, 64-row group)
//   select      select_topk_kernel over the group maxima: the best min(k, groups) groups of each query by (maximum, lower group).
//               They hold the top k rows: a row outside them is beaten by one row of each of k groups, by score or, at equal score,
//               by the lower row
//   pq_keys     one wave per (query, selected group): the same additions again, from the tables in global memory, into keys
//               (ordered score, ~row); 0 for the rows past ntotal and for an unused selection slot
//   select      select_topk_kernel over the keys -> D, I
// The lookups are gathers of 4 bytes at random columns of a 1 KiB table row: a wave's 64 addresses fall on the 32 banks of ds_read_b32
// as they come, which no layout of a table can change, and the scan is bound by them, not by the code stream.
// Scratch (grow-only, the GroupTopK of the index object): 4 bytes per (query, group) and 520 per (query, selected group) of a chunk.
#include "ivr_common.h"
#include "search_coded.h"
#include "search_internal.h"

#include <cfloat>

namespace {

constexpr int kPqKsub = 256;                 // centroids per slice (8-bit codes)
constexpr int kPqScanThreads = 512;          // the scan's workgroup: 8 waves share one LDS image of the tables
// 64-row groups a wave scores at a time: two rows of 8 words each (256 VGPRs and scratch) lose to one
constexpr int pq_scan_rows(int W) { return W <= 4 ? 2 : 1; }
constexpr int kPqTableLds = 128 * 1024;      // LDS a workgroup spends on tables at most: 128 / M queries of M KiB each
constexpr int kPqMaxGroupQ = 8;              // queries of a group at most (their scores are live at once)
constexpr int kPqEncodeMaxReg = 64;          // widest slice the encoder keeps in registers and its codebook in LDS
constexpr int kPqTabQ = 8;                   // queries per thread of the table builder

// s[r] = the score of row[r] against one query's table t ([M][256], LDS or global): additions in ascending m for every row, the R
// rows side by side.  Four bytes of a code are looked up together wherever M leaves them whole
template <int W, int R>
__device__ __forceinline__ void pq_score_rows(const uint4 (&row)[R][W], const float *__restrict__ t, int M, float (&s)[R]) {
#pragma unroll
    for (int r = 0; r < R; ++r) s[r] = 0.f;
#pragma unroll
    for (int w = 0; w < W; ++w) {
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int m0 = 16 * w + 4 * c;
            if (m0 + 4 <= M) {
                float v[R][4];
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    const uint32_t x = ivr_comp(row[r][w], c);
#pragma unroll
                    for (int b = 0; b < 4; ++b) v[r][b] = t[(m0 + b) * kPqKsub + ((x >> (8 * b)) & 255u)];
                }
#pragma unroll
                for (int b = 0; b < 4; ++b) {
#pragma unroll
                    for (int r = 0; r < R; ++r) s[r] = m0 + b == 0 ? v[r][b] : s[r] + v[r][b];
                }
            } else if (m0 < M) {
#pragma unroll
                for (int b = 0; b < 3; ++b) {
                    if (m0 + b < M) {
#pragma unroll
                        for (int r = 0; r < R; ++r) {
                            const uint32_t x = ivr_comp(row[r][w], c);
                            const float v = t[(m0 + b) * kPqKsub + ((x >> (8 * b)) & 255u)];
                            s[r] = m0 + b == 0 ? v : s[r] + v;
                        }
                    }
                }
            }
        }
    }
}

// gmax[q][g] = the best score of the stored rows of group g, for the queries q0 = blockIdx.y * qg .. of the chunk.  Wave w of
// workgroup b takes the units (R groups each) b * 8 + w, + gridDim.x * 8, ...
template <int W, int R>
__global__ __launch_bounds__(kPqScanThreads) void pq_scan_kernel(const uint4 *__restrict__ data, int64_t ntotal, int64_t ngroups,
                                                                 const float *__restrict__ T, int nq, int qg, int M, float *__restrict__ gmax,
                                                                 int64_t mstride) {
    extern __shared__ float lt[];            // [queries of the group][M][256]
    const int tid = threadIdx.x, lane = tid & 63;
    const int q0 = blockIdx.y * qg, nqg = min(qg, nq - q0);
    const int tab = M * kPqKsub;
    {
        const float4 *src = reinterpret_cast<const float4 *>(T + (int64_t)q0 * tab);
        float4 *dst = reinterpret_cast<float4 *>(lt);
        const int n4 = nqg * tab / 4;
        for (int i = tid; i < n4; i += kPqScanThreads) dst[i] = src[i];
    }
    __syncthreads();
    constexpr int kWaves = kPqScanThreads / 64;
    const int64_t nunits = (ngroups + R - 1) / R;
    for (int64_t u = (int64_t)blockIdx.x * kWaves + (tid >> 6); u < nunits; u += (int64_t)gridDim.x * kWaves) {
        uint4 row[R][W];
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int64_t g = u * R + r;
            if (g < ngroups) {
                bin_load_row<W>(data, g, row[r]);
            } else {
#pragma unroll
                for (int w = 0; w < W; ++w) row[r][w] = uint4{0u, 0u, 0u, 0u};
            }
        }
        for (int qi = 0; qi < nqg; ++qi) {
            float s[R];
            pq_score_rows<W, R>(row, lt + qi * tab, M, s);
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const int64_t g = u * R + r;
                if (g < ngroups) {           // wave-uniform: the reduction below runs with every lane
                    const float v = g * 64 + lane < ntotal ? fmaxf(s[r], -FLT_MAX) : -INFINITY;
                    const float best = ivr_wave_max(v);
                    if (lane == 0) gmax[(int64_t)(q0 + qi) * mstride + g] = best;
                }
            }
        }
    }
}

// keys[p][lane] for pair p = (query p / ksel, its selected group sel[p]): one wave per pair
template <int W>
__global__ __launch_bounds__(256) void pq_keys_kernel(const uint4 *__restrict__ data, int64_t ntotal, int64_t ngroups,
                                                      const float *__restrict__ T, int M, const uint32_t *__restrict__ sel, int ksel,
                                                      int64_t npairs, uint64_t *__restrict__ keys) {
    const int lane = threadIdx.x & 63;
    const int64_t p = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (p >= npairs) return;
    const uint32_t g = sel[p];
    uint64_t key = 0;
    if ((int64_t)g < ngroups) {              // 0xFFFFFFFF: fewer groups than slots
        uint4 row[1][W];
        bin_load_row<W>(data, (int64_t)g, row[0]);
        float s[1];
        pq_score_rows<W, 1>(row, T + (p / ksel) * ((int64_t)M * kPqKsub), M, s);
        const int64_t r = (int64_t)g * 64 + lane;
        if (r < ntotal) key = ivr_key(s[0], (uint32_t)r);
    }
    keys[p * 64 + lane] = key;
}

// ---- encoder ----------------------------------------------------------------------------------------------------------------------
// Workgroup (b, m): slice m of the rows b * 256 + tid, + gridDim.x * 256, ...; one row per thread, the slice in XR >= dsub registers
// (zeros behind dsub), the slice's codebook in LDS with rows of XR floats (zeros behind dsub, so the inner loop has no bound) and
// |c|^2 behind it.  Every lane reads the same centroid at the same time: LDS broadcasts, no bank conflicts.
template <int XR>
__global__ __launch_bounds__(256) void pq_encode_kernel(const float *__restrict__ x, int64_t n, int d, const float *__restrict__ cb, int M,
                                                        int dsub, uint8_t *__restrict__ codes) {
    extern __shared__ float lc[];            // [256][XR] centroids, [256] squared norms
    float *cn = lc + kPqKsub * XR;
    const int tid = threadIdx.x, m = blockIdx.y;
    const float *c = cb + (int64_t)m * kPqKsub * dsub;
    for (int i = tid; i < kPqKsub * XR; i += 256) {
        const int j = i / XR, t = i % XR;
        lc[i] = t < dsub ? c[j * dsub + t] : 0.f;
    }
    __syncthreads();
    {
        float s = 0.f;
        for (int t = 0; t < XR; ++t) s = fmaf(lc[tid * XR + t], lc[tid * XR + t], s);
        cn[tid] = s;
    }
    __syncthreads();
    for (int64_t i = (int64_t)blockIdx.x * 256 + tid; i < n; i += (int64_t)gridDim.x * 256) {
        const float *xp = x + i * d + m * dsub;
        float xr[XR];
#pragma unroll
        for (int t = 0; t < XR; ++t) xr[t] = t < dsub ? xp[t] : 0.f;
        float best = INFINITY;
        int bj = 0;
#pragma unroll 4
        for (int j = 0; j < kPqKsub; ++j) {
            const float *cj = lc + j * XR;
            float dot = 0.f;
#pragma unroll
            for (int t = 0; t < XR; ++t) dot = fmaf(xr[t], cj[t], dot);
            const float dist = cn[j] - 2.f * dot;
            if (dist < best) {               // strictly: equal distances keep the lower j
                best = dist;
                bj = j;
            }
        }
        codes[i * M + m] = (uint8_t)bj;
    }
}

// dsub > kPqEncodeMaxReg: the same evaluation with the row and the codebook read through the caches (a centroid's address is
// wave-uniform)
__global__ __launch_bounds__(256) void pq_encode_wide_kernel(const float *__restrict__ x, int64_t n, int d, const float *__restrict__ cb,
                                                             int M, int dsub, uint8_t *__restrict__ codes) {
    const int m = blockIdx.y;
    const float *c = cb + (int64_t)m * kPqKsub * dsub;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const float *xp = x + i * d + m * dsub;
        float best = INFINITY;
        int bj = 0;
        for (int j = 0; j < kPqKsub; ++j) {
            const float *cj = c + j * dsub;
            float dot = 0.f, nrm = 0.f;
            for (int t = 0; t < dsub; ++t) {
                const float cv = cj[t];
                dot = fmaf(xp[t], cv, dot);
                nrm = fmaf(cv, cv, nrm);
            }
            const float dist = nrm - 2.f * dot;
            if (dist < best) {
                best = dist;
                bj = j;
            }
        }
        codes[i * M + m] = (uint8_t)bj;
    }
}

// ---- tables -----------------------------------------------------------------------------------------------------------------------
// Workgroup (b, m), thread j: T[q][m][j] for the queries q = b * kPqTabQ .. + kPqTabQ - 1; a centroid coordinate is read once for all
// of them, a query coordinate is wave-uniform
__global__ __launch_bounds__(256) void pq_tables_kernel(const float *__restrict__ q, int nq, int d, const float *__restrict__ cb, int M,
                                                        int dsub, float *__restrict__ T) {
    const int m = blockIdx.y, j = threadIdx.x;
    const int q0 = blockIdx.x * kPqTabQ;
    const float *c = cb + ((int64_t)m * kPqKsub + j) * dsub;
    const float *qp[kPqTabQ];
    float acc[kPqTabQ];
#pragma unroll
    for (int i = 0; i < kPqTabQ; ++i) {
        qp[i] = q + (int64_t)min(q0 + i, nq - 1) * d + m * dsub;
        acc[i] = 0.f;
    }
    for (int t = 0; t < dsub; ++t) {
        const float cv = c[t];
#pragma unroll
        for (int i = 0; i < kPqTabQ; ++i) acc[i] = fmaf(qp[i][t], cv, acc[i]);
    }
#pragma unroll
    for (int i = 0; i < kPqTabQ; ++i)
        if (q0 + i < nq) T[((int64_t)(q0 + i) * M + m) * kPqKsub + j] = acc[i];
}

template <int XR>
int pq_launch_encode(const float *x, int64_t n, int d, const float *cb, int M, int dsub, uint8_t *codes, unsigned gx, hipStream_t s) {
    const int lds = (kPqKsub * XR + kPqKsub) * (int)sizeof(float);
    const int rc = ivr_func_max_lds(reinterpret_cast<const void *>(pq_encode_kernel<XR>), lds);
    if (rc != IVR_OK) return rc;
    hipLaunchKernelGGL(pq_encode_kernel<XR>, dim3(gx, (unsigned)M), dim3(256), (size_t)lds, s, x, n, d, cb, M, dsub, codes);
    return IVR_OK;
}

}  // namespace

extern "C" {

int ivr_pq_encode(ivr_ctx *ctx, const float *x, int64_t n, int d, const float *codebooks, int M, uint8_t *codes, ivr_stream stream) {
    IVR_REQUIRE(ctx && codebooks && ((x && codes) || n == 0), "ivr_pq_encode: NULL argument");
    IVR_REQUIRE(n >= 0 && n < (1ll << 33), "ivr_pq_encode: n=%lld out of range", (long long)n);
    IVR_REQUIRE(d >= 1 && d <= 65536, "ivr_pq_encode: d=%d out of range [1,65536]", d);
    IVR_REQUIRE(M >= 1 && M <= IVR_PQ_MAX_M && d % M == 0, "ivr_pq_encode: M=%d outside [1,%d] or not a divisor of d=%d", M, IVR_PQ_MAX_M, d);
    if (n == 0) return IVR_OK;
    IVR_HIP(hipSetDevice(ctx->device));
    hipStream_t s = (hipStream_t)stream;
    const int dsub = d / M;
    // enough workgroups per slice to fill the device a few times over; a workgroup stages its codebook once and then walks rows
    const unsigned gx = (unsigned)std::max<int64_t>(1, std::min<int64_t>(ivr_ceil_div(n, 256), ivr_ceil_div(8ll * ctx->cu_count, M)));
    IvrProf prof("pq_encode", s, 2.0 * (double)n * d * kPqKsub);
    int rc = IVR_OK;
    if (dsub <= 4) rc = pq_launch_encode<4>(x, n, d, codebooks, M, dsub, codes, gx, s);
    else if (dsub <= 8) rc = pq_launch_encode<8>(x, n, d, codebooks, M, dsub, codes, gx, s);
    else if (dsub <= 16) rc = pq_launch_encode<16>(x, n, d, codebooks, M, dsub, codes, gx, s);
    else if (dsub <= 32) rc = pq_launch_encode<32>(x, n, d, codebooks, M, dsub, codes, gx, s);
    else if (dsub <= kPqEncodeMaxReg) rc = pq_launch_encode<kPqEncodeMaxReg>(x, n, d, codebooks, M, dsub, codes, gx, s);
    else hipLaunchKernelGGL(pq_encode_wide_kernel, dim3(gx, (unsigned)M), dim3(256), 0, s, x, n, d, codebooks, M, dsub, codes);
    if (rc != IVR_OK) return rc;
    IVR_LAUNCH_CHECK();
    return IVR_OK;
}

int ivr_pq_tables(ivr_ctx *ctx, const float *q, int nq, int d, const float *codebooks, int M, float *T, ivr_stream stream) {
    IVR_REQUIRE(ctx && q && codebooks && T, "ivr_pq_tables: NULL argument");
    IVR_REQUIRE(nq >= 1, "ivr_pq_tables: nq=%d < 1", nq);
    IVR_REQUIRE(d >= 1 && d <= 65536, "ivr_pq_tables: d=%d out of range [1,65536]", d);
    IVR_REQUIRE(M >= 1 && M <= IVR_PQ_MAX_M && d % M == 0, "ivr_pq_tables: M=%d outside [1,%d] or not a divisor of d=%d", M, IVR_PQ_MAX_M, d);
    IVR_HIP(hipSetDevice(ctx->device));
    hipStream_t s = (hipStream_t)stream;
    IvrProf prof("pq_tables", s, 2.0 * (double)nq * d * kPqKsub, true);
    hipLaunchKernelGGL(pq_tables_kernel, dim3((unsigned)ivr_ceil_div(nq, kPqTabQ), (unsigned)M), dim3(256), 0, s, q, nq, d, codebooks, M, d / M,
                       T);
    IVR_LAUNCH_CHECK();
    return IVR_OK;
}

int ivr_bin_index_search_pq(ivr_bin_index *x, const float *T, int nq, int M, int k, float *D, int64_t *I, ivr_stream stream) {
    IVR_REQUIRE(x && T && D && I, "ivr_bin_index_search_pq: NULL argument");
    IVR_REQUIRE(nq >= 1, "ivr_bin_index_search_pq: nq=%d < 1", nq);
    IVR_REQUIRE(k >= 1 && k <= IVR_MAX_K, "ivr_bin_index_search_pq: k=%d outside [1,%d]", k, IVR_MAX_K);
    IVR_REQUIRE(M >= 1 && M <= IVR_PQ_MAX_M, "ivr_bin_index_search_pq: M=%d outside [1,%d]", M, IVR_PQ_MAX_M);
    IVR_REQUIRE(x->nbits == 8 * M, "ivr_bin_index_search_pq: M=%d on an index of %d-bit codes", M, x->nbits);
    IVR_REQUIRE(((uintptr_t)T & 15) == 0, "ivr_bin_index_search_pq: the tables must be 16-byte aligned");
    std::lock_guard<std::mutex> lk(x->mu);
    IVR_HIP(hipSetDevice(x->ctx->device));
    hipStream_t s = (hipStream_t)stream;
    const int64_t ntotal = x->ntotal, ngroups = ivr_ceil_div(ntotal, 64);
    if (ntotal == 0) return GroupTopK::absent(nq, k, D, I, s);
    // never: M <= 128 is 8 words at most; the 16-word scan is not built
    if (x->w16 > 8) return ivr_fail(IVR_ERR_INVALID, "ivr_bin_index_search_pq: %d words per row", x->w16);
    GroupTopK &t = x->pq;
    int rc = t.plan(nq, k, ngroups, 1);          // the scan takes any number of queries: a pass is one
    if (rc != IVR_OK) return rc;
    const int tab = M * kPqKsub;
    const int qg_max = std::max(1, std::min(kPqMaxGroupQ, kPqTableLds / (tab * (int)sizeof(float))));
    return t.run(
        "ivr_bin_index_search_pq", "pq", nq, k, ngroups, D, I, nullptr, nullptr, s,
        [&](int c0, int nqc) {
            int rc = IVR_OK;
            bin_with_words(x->w16, [&](auto w) {
                constexpr int WS = decltype(w)::value > 8 ? 8 : decltype(w)::value, R = pq_scan_rows(WS);
                const int qg = std::min(qg_max, nqc);
                const size_t lds = (size_t)qg * tab * sizeof(float);
                rc = ivr_func_max_lds(reinterpret_cast<const void *>(pq_scan_kernel<WS, R>), (int)lds);
                if (rc != IVR_OK) return;
                // workgroups per CU that the LDS lets be resident, at most 2 (16 waves); each walks the rows with 8 waves
                const int64_t per_cu = std::max<int64_t>(1, std::min<int64_t>(2, (160 * 1024) / (int64_t)lds));
                const unsigned gx = (unsigned)std::max<int64_t>(
                    1, std::min<int64_t>(ivr_ceil_div(ivr_ceil_div(ngroups, R), kPqScanThreads / 64), per_cu * x->ctx->cu_count));
                IvrProf prof("pq_scan", s, (double)nqc * ntotal * M);
                hipLaunchKernelGGL((pq_scan_kernel<WS, R>), dim3(gx, (unsigned)ivr_ceil_div(nqc, qg)), dim3(kPqScanThreads), lds, s, x->data, ntotal,
                                   ngroups, T + (int64_t)c0 * tab, nqc, qg, M, static_cast<float *>(t.gmax.ptr), t.mstride);
            });
            return rc;
        },
        [&](int c0, int, int64_t npairs) {
            bin_with_words(x->w16, [&](auto w) {
                constexpr int WS = decltype(w)::value > 8 ? 8 : decltype(w)::value;
                IvrProf prof("pq_keys", s, (double)npairs * 64 * M, true);
                hipLaunchKernelGGL(pq_keys_kernel<WS>, dim3((unsigned)ivr_ceil_div(npairs, 4)), dim3(256), 0, s, x->data, ntotal, ngroups,
                                   T + (int64_t)c0 * tab, M, (const uint32_t *)t.sel, t.ksel, npairs, (uint64_t *)t.keys);
            });
        });
}

}  // extern "C"
