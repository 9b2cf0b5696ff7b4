// 4-bit product quantisation (faiss IndexPQFastScan, inner product): the encoder (ivr_pqfs_encode), the float and the 8-bit lookup
// tables of a batch of queries (ivr_pqfs_tables, ivr_pqfs_quantize) and the in-register table-lookup top-k over the stored codes
// (ivr_pqfs_index_*).  DESIGN.md section 4, "4-bit product quantisation"; the definitions are the numpy functions pqfs_encode_ref,
// pqfs_tables_ref, pqfs_quantize_ref and pqfs_scan_ref of ivr_amd/pqfs.py.
//
// Storage.  A code is M nibbles; the caller's form is M / 2 bytes, byte j = code[2 j] | code[2 j + 1] << 4 (faiss's packing).  Rows
// are stored per block of 256: lane l of a wave holds rows l, l + 64, l + 128 and l + 192 of the block, and dword j of the lane is the
// four caller bytes j of those rows (row l + 64 b in byte b).  So x & 0x0f0f0f0f is the four codes of sub-quantizer 2 j and
// (x >> 4) & 0x0f0f0f0f those of 2 j + 1, each already a v_perm_b32 selector.  Four dwords (8 sub-quantizers) make one 16-byte word
// per lane, 1 KiB contiguous per wave; a block is W = ceil(M / 8) such words, and the sub-quantizers behind M hold code 0 and have
// all-zero tables.  Capacity comes in whole blocks; rows at or beyond ntotal hold whatever earlier use left there and are masked
// by row number.
//
// Search, per chunk of queries, all on the caller's stream:
//   pqfs_stage  U [nq][M][16] -> [queries padded to whole passes][8 W] tables of 16 bytes, zero where padded
//   pqfs_scan   a wave walks the blocks, up to four side by side; for a pass of kPqfsPassQ queries (fewer in a call of fewer) it
//               loads a code word once, makes the selectors and the high-half masks of its 8 sub-quantizers once, and then, per
//               query, reads each 16-byte table from a wave-uniform address (a scalar load) and looks four rows up at a time: two
//               v_perm_b32 (entries 0-7, 8-15) and one v_bfi_b32.  The four bytes of a result belong to the four 64-row groups of
//               the block.  They are summed as packed u16: r itself (bytes 0 and 2 in the low bytes of the halves, wrapping) and
//               r >> 8 per half (bytes 1 and 3); the sum of bytes 0 and 2 is the first minus 256 times the second, exact modulo
//               2^16 since 255 M <= 65535.  Written: the best acc of each (query, 64-row group)
//   select      select_topk_kernel over the group maxima: the best min(k, groups) groups of each query by (maximum, lower group)
//   pqfs_keys   one wave per (query, selected group): the same lookups again, into keys (acc ^ 0x80000000) << 32 | ~row; 0 for the
//               rows past ntotal and for an unused selection slot
//   select      select_topk_kernel over the keys -> I, and in D the key's high word as select_topk_kernel hands every score back
//   pqfs_finish D = float(acc) * scale + bias from that word: one conversion, one multiplication, one addition
// Scratch (grow-only, on the index object): 128 W bytes per staged query and, in its GroupTopK, 4 bytes per (query, group) and 520
// per (query, selected group) of a chunk.
#include "ivr_common.h"
#include "search_coded.h"
#include "search_internal.h"
#include "search_lists.h"

#include <cfloat>

struct ivr_pqfs_index : CodeRows {       // data: [cap / 256][W][64], group_words = 16 W (a quarter of a block)
    int M = 0, W = 0;
    // search workspace (grow-only)
    DevBuf<uint4> ut;                    // [queries, a multiple of kPqfsPassQ][8 W]: the staged tables
    GroupTopK topk;                      // int32 maxima: best acc of each 64-row group

    int64_t block_words() const { return (int64_t)W * 64; }          // 16-byte words of one 256-row block
};

namespace {

constexpr int kPqfsKsub = 16;                // centroids per slice (4-bit codes)
constexpr int kPqfsBlockRows = 256;          // rows per block: four per lane
// Queries per index pass and 256-row blocks a wave scores side by side.  v_perm_b32 takes one scalar operand, so two of a table's
// four dwords are copied to vector registers first: two v_mov_b32 per table, shared by the blocks of a unit (8 vector instructions per
// four lookups with one block, 6.5 with four).  Measured on 1M rows, M = 128, 1,000 queries, whole search: 16 queries x 1 block 9.42
// ms, 8 x 1 9.33, 8 x 2 7.92, 16 x 2 8.10, 4 x 4 7.52, 8 x 4 7.70 (and the fastest at 64 queries, 0.540 ms): the queries per pass
// hardly matter, the blocks per wave do.  8 x 4 is 156 VGPRs (three waves per SIMD), 8 x 1 is 46.  The tables of a pass are
// 128 W bytes per query, 16 KiB at M = 128: the size of the scalar cache
constexpr int kPqfsPassQ = 8;
constexpr int kPqfsUnit = 4;
constexpr int kPqfsThreads = 256;            // the scan's workgroup: 4 independent waves

typedef unsigned short pqfs_u16x2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ uint32_t pqfs_pk_add(uint32_t a, uint32_t b) {
    return __builtin_bit_cast(uint32_t, __builtin_bit_cast(pqfs_u16x2, a) + __builtin_bit_cast(pqfs_u16x2, b));
}
__device__ __forceinline__ uint32_t pqfs_pk_sub(uint32_t a, uint32_t b) {
    return __builtin_bit_cast(uint32_t, __builtin_bit_cast(pqfs_u16x2, a) - __builtin_bit_cast(pqfs_u16x2, b));
}
__device__ __forceinline__ uint32_t pqfs_pk_shr8(uint32_t a) {
    return __builtin_bit_cast(uint32_t, __builtin_bit_cast(pqfs_u16x2, a) >> (unsigned short)8);
}
__device__ __forceinline__ uint32_t pqfs_pk_shl8(uint32_t a) {
    return __builtin_bit_cast(uint32_t, __builtin_bit_cast(pqfs_u16x2, a) << (unsigned short)8);
}
__device__ __forceinline__ uint32_t pqfs_pk_max(uint32_t a, uint32_t b) {
    return __builtin_bit_cast(uint32_t, __builtin_elementwise_max(__builtin_bit_cast(pqfs_u16x2, a), __builtin_bit_cast(pqfs_u16x2, b)));
}
// the wave-wide maximum of both u16 halves: ivr_wave_max_u32's butterfly with a packed maximum
__device__ __forceinline__ uint32_t pqfs_wave_pk_max(uint32_t v) {
    v = pqfs_pk_max(v, ivr_dpp_u<0xB1>(v));
    v = pqfs_pk_max(v, ivr_dpp_u<0x4E>(v));
    v = pqfs_pk_max(v, ivr_dpp_u<0x141>(v));
    v = pqfs_pk_max(v, ivr_dpp_u<0x140>(v));
    auto a = __builtin_amdgcn_permlane16_swap(v, v, false, false);
    v = pqfs_pk_max((uint32_t)a[0], (uint32_t)a[1]);
    auto b = __builtin_amdgcn_permlane32_swap(v, v, false, false);
    return pqfs_pk_max((uint32_t)b[0], (uint32_t)b[1]);
}

// The selectors of one code word: sel[2 c + h] picks, for the four rows of the lane, entry (code & 7) of either half of the table of
// sub-quantizer 2 c + h of the word, and hm[2 c + h] is 0xff in the bytes whose code is 8 or more
__device__ __forceinline__ void pqfs_selectors(const uint4 &cw, uint32_t (&sel)[8], uint32_t (&hm)[8]) {
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const uint32_t x = ivr_comp(cw, c);
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const uint32_t n = (h ? x >> 4 : x) & 0x0f0f0f0fu;
            const uint32_t top = (n >> 3) & 0x01010101u;
            sel[2 * c + h] = n & 0x07070707u;
            hm[2 * c + h] = (top << 8) - top;            // top * 255 without the quarter-rate multiplication
        }
    }
}

// One table against four rows: byte b of the result = t[code of row l + 64 b].  Added to a02 whole (packed u16, wrapping) and to a13
// shifted down by a byte per half
__device__ __forceinline__ void pqfs_lookup(const uint4 &t, uint32_t sel, uint32_t hm, uint32_t &a02, uint32_t &a13) {
    const uint32_t lo = __builtin_amdgcn_perm(t.y, t.x, sel), hi = __builtin_amdgcn_perm(t.w, t.z, sel);
    const uint32_t r = (hi & hm) | (lo & ~hm);
    a02 = pqfs_pk_add(a02, r);
    a13 = pqfs_pk_add(a13, pqfs_pk_shr8(r));
}
// (a02, a13) after the last table -> the acc of rows l and l + 128 in the halves of a02, of l + 64 and l + 192 in those of a13
__device__ __forceinline__ uint32_t pqfs_even_rows(uint32_t a02, uint32_t a13) { return pqfs_pk_sub(a02, pqfs_pk_shl8(a13)); }

// gmax[q][g] = the best acc of the stored rows of group g for the Q queries of pass blockIdx.y (Q = kPqfsPassQ, or a lower power of
// two for a call of fewer queries, which would otherwise pay for the absent ones).  Wave w of workgroup b takes the units (R blocks
// each) b * 4 + w, + gridDim.x * 4, ...  A row past ntotal counts as 0: every group that is read has a stored row, and no acc is below 0.  The four
// maxima of a block are one 16-byte store (a row of gmax is padded to 64 groups)
template <int Q, int R>
__global__ __launch_bounds__(kPqfsThreads) void pqfs_scan_kernel(const uint4 *__restrict__ data, int64_t ntotal, int64_t nblocks, int W,
                                                                 const uint4 *__restrict__ ut, int nq, int32_t *__restrict__ gmax,
                                                                 int64_t mstride) {
    const int lane = threadIdx.x & 63;
    const int q0 = blockIdx.y * Q;
    const uint4 *tq = ut + (int64_t)q0 * (8 * W);            // wave-uniform: the tables of the pass
    const int64_t nunits = (nblocks + R - 1) / R;
    for (int64_t u = (int64_t)blockIdx.x * (kPqfsThreads / 64) + (threadIdx.x >> 6); u < nunits; u += (int64_t)gridDim.x * (kPqfsThreads / 64)) {
        uint32_t a02[R][Q], a13[R][Q];
        const uint4 *rp[R];
#pragma unroll
        for (int r = 0; r < R; ++r) {
#pragma unroll
            for (int qi = 0; qi < Q; ++qi) a02[r][qi] = a13[r][qi] = 0u;
            rp[r] = data + min(u * R + r, nblocks - 1) * ((int64_t)W * 64) + lane;       // a block past the end: the last one again, not stored
        }
        for (int w = 0; w < W; ++w) {
            uint32_t sel[R][8], hm[R][8];
#pragma unroll
            for (int r = 0; r < R; ++r) pqfs_selectors(rp[r][w * 64], sel[r], hm[r]);
#pragma unroll
            for (int qi = 0; qi < Q; ++qi) {
                const uint4 *t = tq + (qi * W + w) * 8;
#pragma unroll
                for (int s = 0; s < 8; ++s) {
                    const uint4 tb = t[s];
#pragma unroll
                    for (int r = 0; r < R; ++r) pqfs_lookup(tb, sel[r][s], hm[r][s], a02[r][qi], a13[r][qi]);
                }
            }
        }
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int64_t blk = u * R + r;
            if (blk >= nblocks) break;           // wave-uniform
            const int64_t r0 = blk * kPqfsBlockRows + lane;
            const uint32_t m02 = (r0 < ntotal ? 0xffffu : 0u) | (r0 + 128 < ntotal ? 0xffff0000u : 0u);
            const uint32_t m13 = (r0 + 64 < ntotal ? 0xffffu : 0u) | (r0 + 192 < ntotal ? 0xffff0000u : 0u);
#pragma unroll
            for (int qi = 0; qi < Q; ++qi) {
                const uint32_t e = pqfs_wave_pk_max(pqfs_even_rows(a02[r][qi], a13[r][qi]) & m02), o = pqfs_wave_pk_max(a13[r][qi] & m13);
                if (lane == 0 && q0 + qi < nq)
                    *reinterpret_cast<int4 *>(gmax + (int64_t)(q0 + qi) * mstride + blk * 4) =
                        int4{(int)(e & 0xffffu), (int)(o & 0xffffu), (int)(e >> 16), (int)(o >> 16)};
            }
        }
    }
}

// f(Q, R) as integral constants for a chunk of nq queries: passes of kPqfsPassQ queries, or of the power of two that holds a smaller
// call; kPqfsUnit blocks per wave from three passes on (fewer passes leave too few units of that size to fill the device)
template <typename F>
void pqfs_with_pass(int nq, F &&f) {
    const std::integral_constant<int, 1> one{};
    if (nq <= 1) f(std::integral_constant<int, 1>{}, one);
    else if (nq <= 2) f(std::integral_constant<int, 2>{}, one);
    else if (nq <= 4) f(std::integral_constant<int, 4>{}, one);
    else if (nq <= 2 * kPqfsPassQ) f(std::integral_constant<int, kPqfsPassQ>{}, one);
    else f(std::integral_constant<int, kPqfsPassQ>{}, std::integral_constant<int, kPqfsUnit>{});
}

// keys[p][lane] for pair p = (query p / ksel, its selected group sel[p]): one wave per pair, lane l scores row 64 g + l (byte g & 3
// of its block's dwords) with the lookups of the scan
__global__ __launch_bounds__(256) void pqfs_keys_kernel(const uint4 *__restrict__ data, int64_t ntotal, int64_t ngroups, int W,
                                                        const uint4 *__restrict__ ut, const uint32_t *__restrict__ gsel, int ksel,
                                                        int64_t npairs, uint64_t *__restrict__ keys) {
    const int lane = threadIdx.x & 63;
    const int64_t p = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (p >= npairs) return;
    const uint32_t g = gsel[p];
    uint64_t key = 0;
    if ((int64_t)g < ngroups) {              // 0xFFFFFFFF: fewer groups than slots (wave-uniform)
        const uint4 *rp = data + (int64_t)(g >> 2) * ((int64_t)W * 64) + lane;
        const uint4 *t = ut + (p / ksel) * (8 * W);
        uint32_t a02 = 0u, a13 = 0u;
        for (int w = 0; w < W; ++w) {
            uint32_t sel[8], hm[8];
            pqfs_selectors(rp[w * 64], sel, hm);
#pragma unroll
            for (int s = 0; s < 8; ++s) pqfs_lookup(t[w * 8 + s], sel[s], hm[s], a02, a13);
        }
        const uint32_t pair = (g & 1u) ? a13 : pqfs_even_rows(a02, a13);
        const uint32_t acc = (g & 2u) ? pair >> 16 : pair & 0xffffu;
        const int64_t r = (int64_t)g * 64 + lane;
        if (r < ntotal) key = ((uint64_t)(acc ^ 0x80000000u) << 32) | (uint32_t)(0xFFFFFFFFu - (uint32_t)r);
    }
    keys[p * 64 + lane] = key;
}

// U [nq][M][16] -> ut [nqp][8 W] tables of 16 bytes, zero for the sub-quantizers behind M and the queries behind nq
__global__ __launch_bounds__(256) void pqfs_stage_kernel(const uint4 *__restrict__ U, int nq, int M, int W, int64_t total, uint4 *__restrict__ ut) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int64_t q = i / (8 * W);
    const int m = (int)(i % (8 * W));
    ut[i] = q < nq && m < M ? U[q * M + m] : uint4{0u, 0u, 0u, 0u};
}

// caller bytes [n][M / 2] -> rows start .. start + n of the block layout: one thread per (row, dword of the lane), one byte store
// each; the dwords behind M / 2 are written 0
__global__ __launch_bounds__(256) void pqfs_pack_kernel(const uint8_t *__restrict__ src, uint8_t *__restrict__ dst, int64_t start, int64_t n,
                                                        int cs, int W) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int nd = 4 * W;
    const int64_t i = t / nd;
    const int j = (int)(t % nd);
    if (i >= n) return;
    const int64_t r = start + i;
    dst[((((r >> 8) * W + (j >> 2)) * 64 + (r & 63)) * 4 + (j & 3)) * 4 + ((r >> 6) & 3)] = j < cs ? src[i * cs + j] : (uint8_t)0;
}

// rows start .. start + n of the block layout -> caller bytes [n][M / 2]: one thread per byte
__global__ __launch_bounds__(256) void pqfs_unpack_kernel(const uint8_t *__restrict__ data, int64_t start, int64_t n, int cs, int W,
                                                          uint8_t *__restrict__ out) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t i = t / cs;
    const int j = (int)(t % cs);
    if (i >= n) return;
    const int64_t r = start + i;
    out[t] = data[((((r >> 8) * W + (j >> 2)) * 64 + (r & 63)) * 4 + (j & 3)) * 4 + ((r >> 6) & 3)];
}

// ---- encoder ----------------------------------------------------------------------------------------------------------------------
// Workgroup (b, j): byte j (slices 2 j and 2 j + 1) of the rows b * 256 + tid, + gridDim.x * 256, ...  The 16 squared distances of a
// slice are summed side by side, sum (x - c)^2 in ascending t, so that a coordinate of the row is read once; a centroid coordinate
// is wave-uniform
__global__ __launch_bounds__(256) void pqfs_encode_kernel(const float *__restrict__ x, int64_t n, int d, const float *__restrict__ cb, int M,
                                                          int dsub, uint8_t *__restrict__ codes) {
    const int jb = blockIdx.y;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        uint32_t byte = 0;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int m = 2 * jb + h;
            const float *xp = x + i * d + (int64_t)m * dsub;
            const float *c = cb + (int64_t)m * kPqfsKsub * dsub;
            float dist[kPqfsKsub];
#pragma unroll
            for (int j = 0; j < kPqfsKsub; ++j) dist[j] = 0.f;
            for (int t = 0; t < dsub; ++t) {
                const float xv = xp[t];
#pragma unroll
                for (int j = 0; j < kPqfsKsub; ++j) {
                    const float df = xv - c[j * dsub + t];
                    dist[j] = fmaf(df, df, dist[j]);
                }
            }
            float best = dist[0];
            uint32_t bj = 0;
#pragma unroll
            for (int j = 1; j < kPqfsKsub; ++j) {
                if (dist[j] < best) {            // strictly: equal distances keep the lower j
                    best = dist[j];
                    bj = j;
                }
            }
            byte |= bj << (4 * h);
        }
        codes[i * (M / 2) + jb] = (uint8_t)byte;
    }
}

// ---- tables -----------------------------------------------------------------------------------------------------------------------
// The quantiser of one query's float tables lt [M][16] (LDS, complete and visible to the workgroup of 256): pqfs_quantize_ref, every
// step one float32 rounding.  slo, srg: [256] floats of LDS
__device__ __forceinline__ void pqfs_quantize_block(const float *lt, int M, float *slo, float *srg, uint8_t *__restrict__ U,
                                                    float *__restrict__ scale, float *__restrict__ bias) {
    SQ_NO_CONTRACT
    const int tid = threadIdx.x;
    float rg = 0.f;
    if (tid < M) {
        float lo = lt[tid * 16], hi = lo;
#pragma unroll
        for (int j = 1; j < 16; ++j) {
            lo = fminf(lo, lt[tid * 16 + j]);
            hi = fmaxf(hi, lt[tid * 16 + j]);
        }
        slo[tid] = lo;
        rg = hi - lo;
    }
    rg = ivr_wave_max(rg);
    if ((tid & 63) == 0) srg[tid >> 6] = rg;
    __syncthreads();
    const float span = fmaxf(fmaxf(srg[0], srg[1]), fmaxf(srg[2], srg[3]));
    float a = 255.f / span, sc = span / 255.f;
    if (span == 0.f || !isfinite(a)) a = sc = 0.f;
    for (int e = tid; e < M * 16; e += 256) {
        const float df = lt[e] - slo[e >> 4];
        const float v = rintf(df * a);
        U[e] = (uint8_t)(int)fminf(fmaxf(v, 0.f), 255.f);
    }
    if (tid == 0) {
        float b = slo[0];
        for (int m = 1; m < M; ++m) b = b + slo[m];
        *scale = sc;
        *bias = b;
    }
}

// One workgroup per query: T[m][j] = <slice m of q, centroids[m][j]> from zero in ascending t (thread e takes the entries e, e + 256,
// ...; a query coordinate is read by 16 threads, a centroid coordinate once), then the quantiser on those very floats
__global__ __launch_bounds__(256) void pqfs_tables_kernel(const float *__restrict__ q, int d, const float *__restrict__ cb, int M, int dsub,
                                                          float *__restrict__ T, uint8_t *__restrict__ U, float *__restrict__ scale,
                                                          float *__restrict__ bias) {
    __shared__ float lt[IVR_PQFS_MAX_M * 16], slo[IVR_PQFS_MAX_M], srg[4];
    const int64_t qi = blockIdx.x;
    const float *qp = q + qi * d;
    for (int e = threadIdx.x; e < M * 16; e += 256) {
        const float *xs = qp + (e >> 4) * dsub, *c = cb + (int64_t)e * dsub;
        float acc = 0.f;
        for (int t = 0; t < dsub; ++t) acc = fmaf(xs[t], c[t], acc);
        lt[e] = acc;
        if (T) T[qi * M * 16 + e] = acc;
    }
    __syncthreads();
    pqfs_quantize_block(lt, M, slo, srg, U + qi * M * 16, scale + qi, bias + qi);
}

// the quantiser alone, on caller-supplied float tables
__global__ __launch_bounds__(256) void pqfs_quantize_kernel(const float *__restrict__ T, int M, uint8_t *__restrict__ U, float *__restrict__ scale,
                                                            float *__restrict__ bias) {
    __shared__ float lt[IVR_PQFS_MAX_M * 16], slo[IVR_PQFS_MAX_M], srg[4];
    const int64_t qi = blockIdx.x;
    for (int e = threadIdx.x; e < M * 16; e += 256) lt[e] = T[qi * M * 16 + e];
    __syncthreads();
    pqfs_quantize_block(lt, M, slo, srg, U + qi * M * 16, scale + qi, bias + qi);
}

bool pqfs_valid_m(int M) { return M >= 2 && M <= IVR_PQFS_MAX_M && M % 2 == 0; }

}  // namespace

extern "C" {

int ivr_pqfs_pass_queries(void) { return kPqfsPassQ; }

int ivr_pqfs_encode(ivr_ctx *ctx, const float *x, int64_t n, int d, const float *centroids, int M, uint8_t *codes, ivr_stream stream) {
    IVR_REQUIRE(ctx && centroids && ((x && codes) || n == 0), "ivr_pqfs_encode: NULL argument");
    IVR_REQUIRE(n >= 0 && n < (1ll << 33), "ivr_pqfs_encode: n=%lld out of range", (long long)n);
    IVR_REQUIRE(d >= 1 && d <= 65536, "ivr_pqfs_encode: d=%d out of range [1,65536]", d);
    IVR_REQUIRE(pqfs_valid_m(M) && d % M == 0, "ivr_pqfs_encode: M=%d odd, outside [2,%d] or not a divisor of d=%d", M, IVR_PQFS_MAX_M, d);
    if (n == 0) return IVR_OK;
    IVR_HIP(hipSetDevice(ctx->device));
    hipStream_t s = (hipStream_t)stream;
    const unsigned gx = (unsigned)std::max<int64_t>(1, std::min<int64_t>(ivr_ceil_div(n, 256), ivr_ceil_div(16ll * ctx->cu_count, M / 2)));
    IvrProf prof("pqfs_encode", s, 3.0 * (double)n * d * kPqfsKsub);
    hipLaunchKernelGGL(pqfs_encode_kernel, dim3(gx, (unsigned)(M / 2)), dim3(256), 0, s, x, n, d, centroids, M, d / M, codes);
    IVR_LAUNCH_CHECK();
    return IVR_OK;
}

int ivr_pqfs_tables(ivr_ctx *ctx, const float *q, int nq, int d, const float *centroids, int M, float *T, uint8_t *U, float *scale,
                    float *bias, ivr_stream stream) {
    IVR_REQUIRE(ctx && q && centroids && U && scale && bias, "ivr_pqfs_tables: NULL argument");
    IVR_REQUIRE(nq >= 1, "ivr_pqfs_tables: nq=%d < 1", nq);
    IVR_REQUIRE(d >= 1 && d <= 65536, "ivr_pqfs_tables: d=%d out of range [1,65536]", d);
    IVR_REQUIRE(pqfs_valid_m(M) && d % M == 0, "ivr_pqfs_tables: M=%d odd, outside [2,%d] or not a divisor of d=%d", M, IVR_PQFS_MAX_M, d);
    IVR_HIP(hipSetDevice(ctx->device));
    hipStream_t s = (hipStream_t)stream;
    IvrProf prof("pqfs_tables", s, 2.0 * (double)nq * d * kPqfsKsub, true);
    hipLaunchKernelGGL(pqfs_tables_kernel, dim3((unsigned)nq), dim3(256), 0, s, q, d, centroids, M, d / M, T, U, scale, bias);
    IVR_LAUNCH_CHECK();
    return IVR_OK;
}

int ivr_pqfs_quantize(ivr_ctx *ctx, const float *T, int nq, int M, uint8_t *U, float *scale, float *bias, ivr_stream stream) {
    IVR_REQUIRE(ctx && T && U && scale && bias, "ivr_pqfs_quantize: NULL argument");
    IVR_REQUIRE(nq >= 1, "ivr_pqfs_quantize: nq=%d < 1", nq);
    IVR_REQUIRE(pqfs_valid_m(M), "ivr_pqfs_quantize: M=%d odd or outside [2,%d]", M, IVR_PQFS_MAX_M);
    IVR_HIP(hipSetDevice(ctx->device));
    hipStream_t s = (hipStream_t)stream;
    IvrProf prof("pqfs_quantize", s, (double)nq * M * 16 * 5, true);
    hipLaunchKernelGGL(pqfs_quantize_kernel, dim3((unsigned)nq), dim3(256), 0, s, T, M, U, scale, bias);
    IVR_LAUNCH_CHECK();
    return IVR_OK;
}

int ivr_pqfs_index_create(ivr_ctx *ctx, int M, ivr_pqfs_index **out) {
    IVR_REQUIRE(ctx && out, "ivr_pqfs_index_create: NULL argument");
    IVR_REQUIRE(pqfs_valid_m(M), "ivr_pqfs_index_create: M=%d odd or outside [2,%d]", M, IVR_PQFS_MAX_M);
    ivr_pqfs_index *x = new ivr_pqfs_index();        // rows are allocated by the first add
    x->ctx = ctx;
    x->M = M;
    x->W = (M + 7) / 8;
    x->granule = kPqfsBlockRows;
    x->group_words = x->block_words() / 4;
    *out = x;
    return IVR_OK;
}

int ivr_pqfs_index_destroy(ivr_pqfs_index *x) {
    IVR_REQUIRE(x, "ivr_pqfs_index_destroy: NULL index");
    delete x;                                // the rows and the workspace buffers free themselves
    return IVR_OK;
}

int ivr_pqfs_index_reset(ivr_pqfs_index *x) {
    IVR_REQUIRE(x, "ivr_pqfs_index_reset: NULL index");
    return x->reset(false);
}

int64_t ivr_pqfs_index_ntotal(ivr_pqfs_index *x) {
    IVR_REQUIRE(x, "ivr_pqfs_index_ntotal: NULL index");
    return x->ntotal;
}

int ivr_pqfs_index_add(ivr_pqfs_index *x, const uint8_t *codes, int64_t n, ivr_stream stream) {
    IVR_REQUIRE(x, "ivr_pqfs_index_add: NULL argument");
    return x->add("ivr_pqfs_index_add", codes, n, [&] {
        const int64_t total = n * 4 * x->W;
        hipLaunchKernelGGL(pqfs_pack_kernel, dim3((unsigned)ivr_ceil_div(total, 256)), dim3(256), 0, (hipStream_t)stream, codes,
                           reinterpret_cast<uint8_t *>(x->data), x->ntotal, n, x->M / 2, x->W);
    });
}

int ivr_pqfs_index_get_codes(ivr_pqfs_index *x, int64_t start, int64_t n, uint8_t *out, ivr_stream stream) {
    IVR_REQUIRE(x, "ivr_pqfs_index_get_codes: NULL argument");
    return x->get_codes("ivr_pqfs_index_get_codes", start, n, out, [&] {
        const int64_t total = n * (x->M / 2);
        hipLaunchKernelGGL(pqfs_unpack_kernel, dim3((unsigned)ivr_ceil_div(total, 256)), dim3(256), 0, (hipStream_t)stream,
                           reinterpret_cast<const uint8_t *>(x->data), start, n, x->M / 2, x->W, out);
    });
}

int ivr_pqfs_index_search(ivr_pqfs_index *x, const uint8_t *U, const float *scale, const float *bias, int nq, int k, float *D, int64_t *I,
                          ivr_stream stream) {
    IVR_REQUIRE(x && U && scale && bias && D && I, "ivr_pqfs_index_search: NULL argument");
    IVR_REQUIRE(nq >= 1, "ivr_pqfs_index_search: nq=%d < 1", nq);
    IVR_REQUIRE(k >= 1 && k <= IVR_MAX_K, "ivr_pqfs_index_search: k=%d outside [1,%d]", k, IVR_MAX_K);
    IVR_REQUIRE(((uintptr_t)U & 15) == 0, "ivr_pqfs_index_search: the tables must be 16-byte aligned");
    std::lock_guard<std::mutex> lk(x->mu);
    IVR_HIP(hipSetDevice(x->ctx->device));
    hipStream_t s = (hipStream_t)stream;
    const int64_t ntotal = x->ntotal, ngroups = ivr_ceil_div(ntotal, 64), nblocks = ivr_ceil_div(ntotal, kPqfsBlockRows);
    if (ntotal == 0) return GroupTopK::absent(nq, k, D, I, s);
    GroupTopK &g = x->topk;
    int rc = g.plan(nq, k, ngroups, kPqfsPassQ);
    if (rc != IVR_OK) return rc;
    const int W = x->W;
    const int64_t nqp = ivr_round_up(nq, kPqfsPassQ), tw = 8 * W;        // 16-byte tables per query
    rc = ivr_reserve({{&x->ut, (size_t)(nqp * tw) * sizeof(uint4)}});
    if (rc != IVR_OK) return rc;
    {
        IvrProf prof("pqfs_stage", s, (double)nqp * tw * 32, true);
        hipLaunchKernelGGL(pqfs_stage_kernel, dim3((unsigned)ivr_ceil_div(nqp * tw, 256)), dim3(256), 0, s, reinterpret_cast<const uint4 *>(U), nq,
                           x->M, W, nqp * tw, (uint4 *)x->ut);
    }
    return g.run(
        "ivr_pqfs_index_search", "pqfs", nq, k, ngroups, D, I, scale, bias, s,
        [&](int c0, int nqc) {
            pqfs_with_pass(nqc, [&](auto qv, auto rv) {
                constexpr int Q = decltype(qv)::value, R = decltype(rv)::value;
                const unsigned passes = (unsigned)ivr_ceil_div(nqc, Q);
                // 8 workgroups (32 waves) per CU over all passes; each walks the units of R blocks with 4 waves
                const unsigned gx = (unsigned)std::max<int64_t>(
                    1, std::min<int64_t>(ivr_ceil_div(ivr_ceil_div(nblocks, R), kPqfsThreads / 64), ivr_ceil_div(8ll * x->ctx->cu_count, passes)));
                IvrProf prof("pqfs_scan", s, (double)passes * nblocks * x->block_words() * 16);
                hipLaunchKernelGGL((pqfs_scan_kernel<Q, R>), dim3(gx, passes), dim3(kPqfsThreads), 0, s, x->data, ntotal, nblocks, W,
                                   x->ut + (int64_t)c0 * tw, nqc, static_cast<int32_t *>(g.gmax.ptr), g.mstride);
            });
            return IVR_OK;
        },
        [&](int c0, int, int64_t npairs) {
            IvrProf prof("pqfs_keys", s, (double)npairs * x->block_words() * 16, true);
            hipLaunchKernelGGL(pqfs_keys_kernel, dim3((unsigned)ivr_ceil_div(npairs, 4)), dim3(256), 0, s, x->data, ntotal, ngroups, W,
                               x->ut + (int64_t)c0 * tw, (const uint32_t *)g.sel, g.ksel, npairs, (uint64_t *)g.keys);
        });
}

}  // extern "C"
