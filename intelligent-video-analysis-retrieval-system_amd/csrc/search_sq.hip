// Scalar quantisation (faiss IndexScalarQuantizer, QT_8bit, inner product): the encoder (ivr_sq_encode), the integer form of a batch
// of queries (ivr_sq_query) and the int8 MFMA top-k over the stored codes (ivr_sq_index_*).  DESIGN.md section 4, "scalar
// quantisation"; the definitions are the numpy functions sq_encode_ref, sq_query_ref and sq_scan_ref of ivr_amd/sq.py.
//
// Storage.  A row is d bytes; what is stored is the signed c' = code - 128 (the byte with its top bit flipped), K padded with zero
// bytes to ksteps = ceil(d / 64) steps of 64.  Rows are tiled per 16: tile T = row / 16 is ksteps pieces of 1 KiB, and in piece s
// lane l = (row & 15) + 16 c holds bytes 64 s + 16 c .. + 15 of the row, so one wave-wide 16-byte load is 1 KiB contiguous and is the
// A operand of one v_mfma_i32_16x16x64_i8.  The K order is the natural one; the staged queries use the same layout as the B
// operand, and whatever order the instruction gives the 64 products of a lane group, an integer sum does not depend on it.
// Capacity comes in whole 64-row groups; rows at or beyond ntotal hold whatever earlier use left there and are masked by row number.
//
// Search, per chunk of queries, all on the caller's stream:
//   sq_stage    t (int16) -> the halves t = 128 h + l, l = ((t + 64) & 127) - 64, both int8, tiled per 16 queries like the rows
//   sq_scan     a workgroup of 4 waves holds both halves of a pass of 32 queries in LDS and walks the 64-row groups; a wave loads the
//               four row tiles of a group once per K step and uses them for 16 MFMAs (2 query tiles x 2 halves x 4 row tiles).
//               acc = 128 acc_h + acc_l in int32.  Written: the best acc of each (query, 64-row group)
//   select      select_topk_kernel over the group maxima: the best min(k, groups) groups of each query by (maximum, lower group)
//   sq_keys     one wave per (query, selected group): the same MFMAs again, into keys (acc ^ 0x80000000) << 32 | ~row; 0 for the
//               rows past ntotal and for an unused selection slot
//   select      select_topk_kernel over the keys -> I, and in D the key's high word as select_topk_kernel hands every score back
//               (ivr_ord2f, a bijection of 32-bit patterns)
//   sq_finish   D = float(acc) * scale + bias from that word: one conversion, one multiplication, one addition
// Scratch (grow-only, on the index object): both halves of the staged queries and, in its GroupTopK, 4 bytes per (query, group) and
// 520 per (query, selected group) of a chunk.  sq_frag, sq_combine and SQ_NO_CONTRACT are in search_lists.h and sq_stage_kernel is
// behind ivr_launch_sq_stage: search_ivfsq.hip stages its queries and combines its halves the same way.
#include "ivr_common.h"
#include "search_coded.h"
#include "search_internal.h"
#include "search_lists.h"

#include <cfloat>
#include <climits>

struct ivr_sq_index : CodeRows {         // data: [cap / 16][ksteps][64], group_words = 4 tile_words()
    int d = 0, ksteps = 0;
    // search workspace (grow-only)
    DevBuf<uint4> qh, ql;                // [query tiles, a multiple of kSqQT][ksteps][64]: the two halves of the staged queries
    GroupTopK topk;                      // int32 maxima: best acc of each 64-row group

    int64_t tile_words() const { return (int64_t)ksteps * 64; }      // 16-byte words of one 16-row (or 16-query) tile
};

namespace {

constexpr int kSqMaxD = 1024;                // 16256 * 128 * d fits int32 up to here
constexpr float kSqTMax = 16256.f;           // 127 * 128: the largest |t|
constexpr int kSqQT = 2;                     // 16-query tiles per index pass: 32 queries
constexpr int kSqThreads = 256;              // the scan's workgroup: 4 waves share one LDS image of the queries

// t int16 [nq][d] -> both halves, tiled: one thread per (query tile, K step, lane); zeros past d and past nq.  |t| is clamped to
// 16256 so that h stays an int8 whatever the caller supplies
__global__ __launch_bounds__(256) void sq_stage_kernel(const int16_t *__restrict__ t, int nq, int d, int ksteps, int64_t nwords,
                                                       uint4 *__restrict__ qh, uint4 *__restrict__ ql) {
    const int64_t w = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (w >= nwords) return;
    const int lane = (int)(w & 63);
    const int s = (int)((w >> 6) % ksteps);
    const int64_t q = ((w >> 6) / ksteps) * 16 + (lane & 15);
    const int k0 = 64 * s + 16 * (lane >> 4);
    uint32_t h[4] = {0u, 0u, 0u, 0u}, l[4] = {0u, 0u, 0u, 0u};
    if (q < nq) {
        const int16_t *tp = t + q * d;
#pragma unroll
        for (int b = 0; b < 16; ++b) {
            if (k0 + b < d) {
                const int v = min(max((int)tp[k0 + b], -16256), 16256);
                const int lo = ((v + 64) & 127) - 64, hi = (v - lo) >> 7;
                h[b >> 2] |= (uint32_t)(hi & 255) << (8 * (b & 3));
                l[b >> 2] |= (uint32_t)(lo & 255) << (8 * (b & 3));
            }
        }
    }
    qh[w] = uint4{h[0], h[1], h[2], h[3]};
    ql[w] = uint4{l[0], l[1], l[2], l[3]};
}

// gmax[q][g] = the best acc of the stored rows of group g for the 32 queries of pass blockIdx.y.  Wave w of workgroup b takes the
// groups b * 4 + w, + gridDim.x * 4, ...  In an accumulator tile lane l holds query l & 15 and rows 4 (l >> 4) + reg.
__global__ __launch_bounds__(kSqThreads) void sq_scan_kernel(const uint4 *__restrict__ data, int64_t ntotal, int64_t ngroups, int ksteps,
                                                             const uint4 *__restrict__ qh, const uint4 *__restrict__ ql, int nq,
                                                             int32_t *__restrict__ gmax, int64_t mstride) {
    extern __shared__ uint4 lq[];            // [half][kSqQT][ksteps][64]
    const int tid = threadIdx.x, lane = tid & 63;
    const int tw = ksteps * 64, nw = kSqQT * tw;
    {
        const uint4 *sh = qh + (int64_t)blockIdx.y * nw, *sl = ql + (int64_t)blockIdx.y * nw;
        for (int i = tid; i < nw; i += kSqThreads) {
            lq[i] = sh[i];
            lq[nw + i] = sl[i];
        }
    }
    __syncthreads();
    const int q0 = blockIdx.y * (16 * kSqQT);
    for (int64_t g = (int64_t)blockIdx.x * (kSqThreads / 64) + (tid >> 6); g < ngroups; g += (int64_t)gridDim.x * (kSqThreads / 64)) {
        i32x4 ah[kSqQT][4], al[kSqQT][4];
#pragma unroll
        for (int qt = 0; qt < kSqQT; ++qt) {
#pragma unroll
            for (int t = 0; t < 4; ++t) ah[qt][t] = al[qt][t] = i32x4{0, 0, 0, 0};
        }
        const uint4 *rp = data + g * 4 * tw + lane;
        for (int s = 0; s < ksteps; ++s) {
            i32x4 a[4];
#pragma unroll
            for (int t = 0; t < 4; ++t) a[t] = sq_frag(rp[(int64_t)t * tw + s * 64]);
#pragma unroll
            for (int qt = 0; qt < kSqQT; ++qt) {
                const i32x4 bh = sq_frag(lq[(qt * ksteps + s) * 64 + lane]), bl = sq_frag(lq[nw + (qt * ksteps + s) * 64 + lane]);
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    ah[qt][t] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a[t], bh, ah[qt][t], 0, 0, 0);
                    al[qt][t] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a[t], bl, al[qt][t], 0, 0, 0);
                }
            }
        }
#pragma unroll
        for (int qt = 0; qt < kSqQT; ++qt) {
            int32_t m = INT_MIN;             // below every acc: |acc| <= 16256 * 128 * 1024 < 2^31
#pragma unroll
            for (int t = 0; t < 4; ++t) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int64_t row = g * 64 + t * 16 + 4 * (lane >> 4) + r;
                    if (row < ntotal) m = max(m, sq_combine(ah[qt][t][r], al[qt][t][r]));
                }
            }
            m = max(m, __shfl_xor(m, 16, 64));
            m = max(m, __shfl_xor(m, 32, 64));
            const int q = q0 + qt * 16 + lane;
            if (lane < 16 && q < nq) gmax[(int64_t)q * mstride + g] = m;
        }
    }
}

// keys[p][row of the group] for pair p = (query p / ksel, its selected group sel[p]): one wave per pair, the query's own 16-query
// tile as the B operand; the lanes of its column hold the results
__global__ __launch_bounds__(256) void sq_keys_kernel(const uint4 *__restrict__ data, int64_t ntotal, int64_t ngroups, int ksteps,
                                                      const uint4 *__restrict__ qh, const uint4 *__restrict__ ql,
                                                      const uint32_t *__restrict__ sel, int ksel, int64_t npairs, uint64_t *__restrict__ keys) {
    const int lane = threadIdx.x & 63;
    const int64_t p = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (p >= npairs) return;
    const uint32_t g = sel[p];
    if ((int64_t)g >= ngroups) {             // 0xFFFFFFFF: fewer groups than slots (wave-uniform)
        keys[p * 64 + lane] = 0;
        return;
    }
    const int q = (int)(p / ksel);
    const int tw = ksteps * 64;
    const uint4 *rp = data + (int64_t)g * 4 * tw + lane;
    const uint4 *hp = qh + (int64_t)(q >> 4) * tw + lane, *lp = ql + (int64_t)(q >> 4) * tw + lane;
    i32x4 ah[4], al[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) ah[t] = al[t] = i32x4{0, 0, 0, 0};
    for (int s = 0; s < ksteps; ++s) {
        const i32x4 bh = sq_frag(hp[s * 64]), bl = sq_frag(lp[s * 64]);
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const i32x4 a = sq_frag(rp[(int64_t)t * tw + s * 64]);
            ah[t] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a, bh, ah[t], 0, 0, 0);
            al[t] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a, bl, al[t], 0, 0, 0);
        }
    }
    if ((lane & 15) == (q & 15)) {
#pragma unroll
        for (int t = 0; t < 4; ++t) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int in = t * 16 + 4 * (lane >> 4) + r;
                const int64_t row = (int64_t)g * 64 + in;
                const uint32_t acc = (uint32_t)sq_combine(ah[t][r], al[t][r]);
                keys[p * 64 + in] = row < ntotal ? ((uint64_t)(acc ^ 0x80000000u) << 32) | (uint32_t)(0xFFFFFFFFu - (uint32_t)row) : 0;
            }
        }
    }
}

// caller bytes [n][d] (unsigned codes) -> rows start .. start + n of the tiled layout (signed, zero past d): one thread per (row, 16
// bytes).  vec: d % 16 == 0 and the source 16-byte aligned
__global__ __launch_bounds__(256) void sq_pack_kernel(const uint8_t *__restrict__ src, uint4 *__restrict__ dst, int64_t start, int64_t n, int d,
                                                      int ksteps, int vec) {
    const int64_t w = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int nch = ksteps * 4;
    const int64_t i = w / nch;
    const int c = (int)(w % nch);
    if (i >= n) return;
    const uint8_t *p = src + i * d + 16 * c;
    uint4 v;
    if (vec && 16 * c + 16 <= d) {
        v = *reinterpret_cast<const uint4 *>(p);
        v.x ^= 0x80808080u;
        v.y ^= 0x80808080u;
        v.z ^= 0x80808080u;
        v.w ^= 0x80808080u;
    } else {
        uint32_t x[4] = {0u, 0u, 0u, 0u};
        for (int b = 0; b < 16; ++b)
            if (16 * c + b < d) x[b >> 2] |= (uint32_t)(p[b] ^ 0x80u) << (8 * (b & 3));
        v = uint4{x[0], x[1], x[2], x[3]};
    }
    const int64_t r = start + i;
    dst[((r >> 4) * ksteps + (c >> 2)) * 64 + (r & 15) + 16 * (c & 3)] = v;
}

// rows start .. start + n of the tiled layout -> caller bytes [n][d] (unsigned codes): one thread per (row, 16 bytes)
__global__ __launch_bounds__(256) void sq_unpack_kernel(const uint4 *__restrict__ data, int64_t start, int64_t n, int d, int ksteps,
                                                        uint8_t *__restrict__ out) {
    const int64_t w = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int nch = (d + 15) / 16;
    const int64_t i = w / nch;
    const int c = (int)(w % nch);
    if (i >= n) return;
    const int64_t r = start + i;
    const uint4 v = data[((r >> 4) * ksteps + (c >> 2)) * 64 + (r & 15) + 16 * (c & 3)];
    const uint32_t x[4] = {v.x, v.y, v.z, v.w};
    uint8_t *o = out + i * d + 16 * c;
    for (int b = 0; b < 16; ++b)
        if (16 * c + b < d) o[b] = (uint8_t)((x[b >> 2] >> (8 * (b & 3))) ^ 0x80u);
}

// ---- encoder ----------------------------------------------------------------------------------------------------------------------
// faiss's Codec8bit behind the non-uniform quantiser: every operation a single float32 rounding
__global__ __launch_bounds__(256) void sq_encode_kernel(const float *__restrict__ x, int64_t total, int d, const float *__restrict__ vmin,
                                                        const float *__restrict__ vdiff, uint8_t *__restrict__ codes) {
    SQ_NO_CONTRACT
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int j = (int)(i % d);
        const float vd = vdiff[j];
        float xi = 0.f;
        if (vd != 0.f) xi = fminf(fmaxf((x[i] - vmin[j]) / vd, 0.f), 1.f);
        codes[i] = (uint8_t)min(255, (int)(255.f * xi));
    }
}

// ---- query preparation ------------------------------------------------------------------------------------------------------------
// One workgroup per query: w = q * gain, m = max |w|, s = m / 16256 (1 when m == 0), t = clamp(rint(w / s)), bias = sum q * offset
__global__ __launch_bounds__(256) void sq_query_kernel(const float *__restrict__ q, int d, const float *__restrict__ gain,
                                                       const float *__restrict__ offset, int16_t *__restrict__ t, float *__restrict__ scale,
                                                       float *__restrict__ bias) {
    SQ_NO_CONTRACT
    __shared__ float rm[4], rb[4];
    const int tid = threadIdx.x;
    const float *qp = q + (int64_t)blockIdx.x * d;
    float m = 0.f, b = 0.f;
    for (int j = tid; j < d; j += 256) {
        m = fmaxf(m, fabsf(qp[j] * gain[j]));
        b = fmaf(qp[j], offset[j], b);
    }
    m = ivr_wave_max(m);
    b = ivr_wave_sum(b);
    if ((tid & 63) == 0) {
        rm[tid >> 6] = m;
        rb[tid >> 6] = b;
    }
    __syncthreads();
    m = fmaxf(fmaxf(rm[0], rm[1]), fmaxf(rm[2], rm[3]));
    const float s = m == 0.f ? 1.f : m / kSqTMax;
    for (int j = tid; j < d; j += 256) {
        const float v = rintf(qp[j] * gain[j] / s);
        t[(int64_t)blockIdx.x * d + j] = (int16_t)(int)fminf(fmaxf(v, -kSqTMax), kSqTMax);
    }
    if (tid == 0) {
        scale[blockIdx.x] = s;
        bias[blockIdx.x] = (rb[0] + rb[1]) + (rb[2] + rb[3]);
    }
}

}  // namespace

void ivr_launch_sq_stage(const int16_t *t, int nq, int d, int ksteps, int64_t qtiles, uint4 *qh, uint4 *ql, hipStream_t s) {
    const int64_t nwords = qtiles * ksteps * 64;
    hipLaunchKernelGGL(sq_stage_kernel, dim3((unsigned)ivr_ceil_div(nwords, 256)), dim3(256), 0, s, t, nq, d, ksteps, nwords, qh, ql);
}

extern "C" {

int ivr_sq_encode(ivr_ctx *ctx, const float *x, int64_t n, int d, const float *vmin, const float *vdiff, uint8_t *codes, ivr_stream stream) {
    IVR_REQUIRE(ctx && vmin && vdiff && ((x && codes) || n == 0), "ivr_sq_encode: NULL argument");
    IVR_REQUIRE(n >= 0 && n < (1ll << 33), "ivr_sq_encode: n=%lld out of range", (long long)n);
    IVR_REQUIRE(d >= 1 && d <= kSqMaxD, "ivr_sq_encode: d=%d out of range [1,%d]", d, kSqMaxD);
    if (n == 0) return IVR_OK;
    IVR_HIP(hipSetDevice(ctx->device));
    hipStream_t s = (hipStream_t)stream;
    const int64_t total = n * d;
    const unsigned gx = (unsigned)std::max<int64_t>(1, std::min<int64_t>(ivr_ceil_div(total, 256), 32ll * ctx->cu_count));
    IvrProf prof("sq_encode", s, (double)total * 5);
    hipLaunchKernelGGL(sq_encode_kernel, dim3(gx), dim3(256), 0, s, x, total, d, vmin, vdiff, codes);
    IVR_LAUNCH_CHECK();
    return IVR_OK;
}

int ivr_sq_query(ivr_ctx *ctx, const float *q, int nq, int d, const float *gain, const float *offset, int16_t *t, float *scale, float *bias,
                 ivr_stream stream) {
    IVR_REQUIRE(ctx && q && gain && offset && t && scale && bias, "ivr_sq_query: NULL argument");
    IVR_REQUIRE(nq >= 1, "ivr_sq_query: nq=%d < 1", nq);
    IVR_REQUIRE(d >= 1 && d <= kSqMaxD, "ivr_sq_query: d=%d out of range [1,%d]", d, kSqMaxD);
    IVR_HIP(hipSetDevice(ctx->device));
    hipStream_t s = (hipStream_t)stream;
    IvrProf prof("sq_query", s, (double)nq * d * 6, true);
    hipLaunchKernelGGL(sq_query_kernel, dim3((unsigned)nq), dim3(256), 0, s, q, d, gain, offset, t, scale, bias);
    IVR_LAUNCH_CHECK();
    return IVR_OK;
}

int ivr_sq_index_create(ivr_ctx *ctx, int d, ivr_sq_index **out) {
    IVR_REQUIRE(ctx && out, "ivr_sq_index_create: NULL argument");
    IVR_REQUIRE(d >= 1 && d <= kSqMaxD, "ivr_sq_index_create: d=%d out of range [1,%d]", d, kSqMaxD);
    ivr_sq_index *x = new ivr_sq_index();    // rows are allocated by the first add
    x->ctx = ctx;
    x->d = d;
    x->ksteps = (d + 63) / 64;
    x->granule = 64;
    x->group_words = 4 * x->tile_words();
    *out = x;
    return IVR_OK;
}

int ivr_sq_index_destroy(ivr_sq_index *x) {
    IVR_REQUIRE(x, "ivr_sq_index_destroy: NULL index");
    delete x;                                // the rows and the workspace buffers free themselves
    return IVR_OK;
}

int ivr_sq_index_reset(ivr_sq_index *x) {
    IVR_REQUIRE(x, "ivr_sq_index_reset: NULL index");
    return x->reset(false);
}

int64_t ivr_sq_index_ntotal(ivr_sq_index *x) {
    IVR_REQUIRE(x, "ivr_sq_index_ntotal: NULL index");
    return x->ntotal;
}

int ivr_sq_index_add(ivr_sq_index *x, const uint8_t *codes, int64_t n, ivr_stream stream) {
    IVR_REQUIRE(x, "ivr_sq_index_add: NULL argument");
    return x->add("ivr_sq_index_add", codes, n, [&] {
        const int64_t words = n * x->ksteps * 4;
        const int vec = x->d % 16 == 0 && ((uintptr_t)codes & 15) == 0;
        hipLaunchKernelGGL(sq_pack_kernel, dim3((unsigned)ivr_ceil_div(words, 256)), dim3(256), 0, (hipStream_t)stream, codes, x->data, x->ntotal,
                           n, x->d, x->ksteps, vec);
    });
}

int ivr_sq_index_get_codes(ivr_sq_index *x, int64_t start, int64_t n, uint8_t *out, ivr_stream stream) {
    IVR_REQUIRE(x, "ivr_sq_index_get_codes: NULL argument");
    return x->get_codes("ivr_sq_index_get_codes", start, n, out, [&] {
        const int64_t words = n * ((x->d + 15) / 16);
        hipLaunchKernelGGL(sq_unpack_kernel, dim3((unsigned)ivr_ceil_div(words, 256)), dim3(256), 0, (hipStream_t)stream, x->data, start, n, x->d,
                           x->ksteps, out);
    });
}

int ivr_sq_index_search(ivr_sq_index *x, const int16_t *t, const float *scale, const float *bias, int nq, int k, float *D, int64_t *I,
                        ivr_stream stream) {
    IVR_REQUIRE(x && t && scale && bias && D && I, "ivr_sq_index_search: NULL argument");
    IVR_REQUIRE(nq >= 1, "ivr_sq_index_search: nq=%d < 1", nq);
    IVR_REQUIRE(k >= 1 && k <= IVR_MAX_K, "ivr_sq_index_search: k=%d outside [1,%d]", k, IVR_MAX_K);
    std::lock_guard<std::mutex> lk(x->mu);
    IVR_HIP(hipSetDevice(x->ctx->device));
    hipStream_t s = (hipStream_t)stream;
    const int64_t ntotal = x->ntotal, ngroups = ivr_ceil_div(ntotal, 64);
    if (ntotal == 0) return GroupTopK::absent(nq, k, D, I, s);
    constexpr int kPass = 16 * kSqQT;        // queries of one index pass
    GroupTopK &g = x->topk;
    int rc = g.plan(nq, k, ngroups, kPass);
    if (rc != IVR_OK) return rc;
    const int64_t tw = x->tile_words(), qtiles = ivr_round_up(ivr_ceil_div(nq, 16), kSqQT);
    rc = ivr_reserve({{&x->qh, (size_t)(qtiles * tw) * sizeof(uint4)}, {&x->ql, (size_t)(qtiles * tw) * sizeof(uint4)}});
    if (rc != IVR_OK) return rc;
    const size_t lds = (size_t)2 * kSqQT * tw * sizeof(uint4);           // 4 KiB per K step: 64 KiB at d = 1024
    rc = ivr_func_max_lds(reinterpret_cast<const void *>(sq_scan_kernel), (int)lds);
    if (rc != IVR_OK) return rc;
    {
        IvrProf prof("sq_stage", s, (double)nq * x->d * 2, true);
        ivr_launch_sq_stage(t, nq, x->d, x->ksteps, qtiles, x->qh, x->ql, s);
    }
    // workgroups per CU that the LDS lets be resident, at most 4 (16 waves); each walks the groups with 4 waves
    const int64_t per_cu = std::max<int64_t>(1, std::min<int64_t>(4, (160 * 1024) / (int64_t)lds));
    return g.run(
        "ivr_sq_index_search", "sq", nq, k, ngroups, D, I, scale, bias, s,
        [&](int c0, int nqc) {
            const unsigned passes = (unsigned)ivr_ceil_div(nqc, kPass);
            const unsigned gx = (unsigned)std::max<int64_t>(
                1, std::min<int64_t>(ivr_ceil_div(ngroups, kSqThreads / 64), ivr_ceil_div(per_cu * x->ctx->cu_count, passes)));
            IvrProf prof("sq_scan", s, (double)passes * ngroups * 4 * tw * 16);
            hipLaunchKernelGGL(sq_scan_kernel, dim3(gx, passes), dim3(kSqThreads), lds, s, x->data, ntotal, ngroups, x->ksteps,
                               x->qh + (int64_t)(c0 / 16) * tw, x->ql + (int64_t)(c0 / 16) * tw, nqc, static_cast<int32_t *>(g.gmax.ptr), g.mstride);
            return IVR_OK;
        },
        [&](int c0, int, int64_t npairs) {
            IvrProf prof("sq_keys", s, (double)npairs * 4 * tw * 16, true);
            hipLaunchKernelGGL(sq_keys_kernel, dim3((unsigned)ivr_ceil_div(npairs, 4)), dim3(256), 0, s, x->data, ntotal, ngroups, x->ksteps,
                               x->qh + (int64_t)(c0 / 16) * tw, x->ql + (int64_t)(c0 / 16) * tw, (const uint32_t *)g.sel, g.ksel, npairs,
                               (uint64_t *)g.keys);
        });
}

}  // extern "C"
