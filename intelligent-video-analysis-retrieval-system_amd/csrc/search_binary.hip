// Binary codes: the flat Hamming index (faiss IndexBinaryFlat) and the sign-bit encoder of IndexLSH (ivr_sign_encode).
//
// Storage.  A code of nbits bits is padded with zeros to W words of 16 bytes (W in {1, 2, 3, 4, 8, 16}: the distance loop is unrolled
// over it) and stored interleaved per 64 rows: word w of row r is data[(r / 64) * W * 64 + w * 64 + r % 64].  One lane holds one row, and
// every 16-byte load of a wave is 1 KiB contiguous.  Pad bits (at or above nbits) are cleared when a code is stored and when a query is
// staged, so popcount(xor) never sees them.
//
// Search ("binary codes").  A Hamming distance is an integer in [0, nbits]: the top k is found by counting,
// per chunk of queries, in passes that each read the codes once and write nothing per (query, row):
//   histogram   rows per (query, distance): LDS histogram per workgroup over many row blocks, then integer atomics into the global one
//               for the bins up to the workgroup's own k-th smallest distance (the global one is no larger)
//   threshold   one wave per query: t = smallest distance whose cumulative count reaches k, below = rows nearer than t, need = k - below
//   count       per (query, 64-row group): rows with dist < t and rows with dist == t (ballot + popcount)
//   prefix      exclusive prefix of both counts over the groups of a query
//   emit        every row with dist < t at slot prefix + rank, the first `need` rows with dist == t (ascending row) behind them: a row's
//               slot is a function of the data alone (no cursor atomics), so the same rows are chosen on every run
//   order       bitonic sort of the k (distance, row) keys of a query in one workgroup; D / I written
// Scratch: nq W 16 bytes of staged queries, and per chunk (nbits + 1) 4 + (rows / 64) 8 + k 8 bytes per query.
#include "search_coded.h"
#include "search_internal.h"

#include <climits>

namespace {

constexpr uint64_t kBinEmpty = ~0ull;    // key of an unused result slot
constexpr int64_t kSignEncodeSmall = 4096;   // ivr_sign_encode: up to this many rows take the latency-oriented instantiation

// struct ivr_bin_index: search_coded.h; bin_load_row and bin_with_words: search_internal.h (search_pq.hip scans the same storage)

int bin_words(int code_size) {
    const int w = (code_size + 15) / 16;
    return w <= 4 ? w : w <= 8 ? 8 : 16;
}

// bytes [b0, b0 + 4) of a code as one little-endian word, zero past code_size, bits at or above nbits cleared
__device__ __forceinline__ uint32_t bin_code_word(const uint8_t *__restrict__ p, int b0, int code_size, int nbits, bool vec) {
    uint32_t x = 0;
    if (vec && b0 + 4 <= code_size) {
        x = *reinterpret_cast<const uint32_t *>(p + b0);
    } else {
        for (int b = 0; b < 4; ++b)
            if (b0 + b < code_size) x |= (uint32_t)p[b0 + b] << (8 * b);
    }
    const int bit0 = 8 * b0;
    if (bit0 >= nbits) return 0u;
    if (bit0 + 32 > nbits) x &= (1u << (nbits - bit0)) - 1u;
    return x;
}

// caller bytes [n][code_size] -> padded words.  interleaved = 1: rows start .. start + n of the index layout; 0: row-major [n][w16]
// (staged queries).  One thread per (row, word), the row fastest.
__global__ __launch_bounds__(256) void bin_pack_kernel(const uint8_t *__restrict__ src, uint4 *__restrict__ dst, int64_t start, int64_t n,
                                                       int nbits, int code_size, int w16, int interleaved, int vec) {
    const int64_t t = blockIdx.x * 256ll + threadIdx.x;
    const int lane = (int)(t & 63);
    const int64_t gw = t >> 6;
    const int w = (int)(gw % w16);
    const int64_t i = (gw / w16) * 64 + lane;
    if (i >= n) return;
    const uint8_t *p = src + i * code_size;
    uint4 v;
    v.x = bin_code_word(p, 16 * w + 0, code_size, nbits, vec);
    v.y = bin_code_word(p, 16 * w + 4, code_size, nbits, vec);
    v.z = bin_code_word(p, 16 * w + 8, code_size, nbits, vec);
    v.w = bin_code_word(p, 16 * w + 12, code_size, nbits, vec);
    const int64_t r = start + i;
    dst[interleaved ? (r >> 6) * w16 * 64 + (int64_t)w * 64 + (r & 63) : i * w16 + w] = v;
}

// rows start .. start + n of the index layout -> caller bytes [n][code_size].  One thread per (row, 4 bytes)
__global__ __launch_bounds__(256) void bin_unpack_kernel(const uint32_t *__restrict__ data, int64_t start, int64_t n, int code_size, int w16,
                                                         uint8_t *__restrict__ out) {
    const int c4 = (code_size + 3) / 4;
    const int64_t t = blockIdx.x * 256ll + threadIdx.x;
    const int64_t i = t / c4;
    const int j = (int)(t % c4);
    if (i >= n) return;
    const int64_t r = start + i;
    const uint32_t x = data[((r >> 6) * w16 * 64 + (int64_t)(j >> 2) * 64 + (r & 63)) * 4 + (j & 3)];
    for (int b = 0; b < 4; ++b)
        if (4 * j + b < code_size) out[i * code_size + 4 * j + b] = (uint8_t)(x >> (8 * b));
}

// Hamming distance of the lane's row to a query (q: wave-uniform address, so its words arrive through the scalar cache)
template <int W>
__device__ __forceinline__ uint32_t bin_dist(const uint4 (&row)[W], const uint4 *__restrict__ q) {
    uint32_t d = 0;
#pragma unroll
    for (int w = 0; w < W; ++w) {
        const uint4 x = q[w];
        d += __popc(row[w].x ^ x.x);
        d += __popc(row[w].y ^ x.y);
        d += __popc(row[w].z ^ x.z);
        d += __popc(row[w].w ^ x.w);
    }
    return d;
}

// Pass 1.  hist[q][dist] += 1 for every stored row.  A workgroup walks the 256-row blocks blockIdx.x, + gridDim.x, ... and keeps the
// histograms of the chunk's queries in LDS; the bins that can matter go to the global histogram at the end.
template <int W>
__global__ __launch_bounds__(256) void bin_hist_kernel(const uint4 *__restrict__ data, int64_t ntotal, int64_t nblocks,
                                                       const uint4 *__restrict__ q, int nqc, int nbins, int k, uint32_t *__restrict__ hist) {
    extern __shared__ uint32_t lh[];     // [nqc][nbins]
    const int tid = threadIdx.x;
    for (int i = tid; i < nqc * nbins; i += 256) lh[i] = 0u;
    __syncthreads();
    // the rows of the next block are in flight while this one is scored
    uint4 next[W];
    if (blockIdx.x < nblocks) bin_load_row<W>(data, blockIdx.x * 4ll + (tid >> 6), next);
    for (int64_t b = blockIdx.x; b < nblocks; b += gridDim.x) {
        const bool valid = b * kBinBlockRows + tid < ntotal;
        uint4 row[W];
#pragma unroll
        for (int w = 0; w < W; ++w) row[w] = next[w];
        if (b + gridDim.x < nblocks) bin_load_row<W>(data, (b + gridDim.x) * 4 + (tid >> 6), next);
        for (int qi = 0; qi < nqc; ++qi) {
            const uint32_t d = min(bin_dist<W>(row, q + (int64_t)qi * W), (uint32_t)(nbins - 1));
            if (valid) atomicAdd(&lh[qi * nbins + d], 1u);
        }
    }
    __syncthreads();
    // One wave per query.  Only the bins up to the one at which this workgroup's OWN rows reach k are added to the global histogram:
    // the k-th smallest distance over all rows is no larger, so every bin the threshold pass reads before it stops is complete, and the
    // crowded bins around the mean distance, which every workgroup would add to, are left out
    const int lane = tid & 63;
    for (int qi = tid >> 6; qi < nqc; qi += 4) {
        const uint32_t *h = lh + qi * nbins;
        uint32_t below = 0;
        for (int base = 0; base < nbins && below < (uint32_t)k; base += 64) {
            const int i = base + lane;
            const uint32_t c = i < nbins ? h[i] : 0u;
            const uint32_t incl = below + ivr_wave_incl_scan(c);
            if (c && incl - c < (uint32_t)k) atomicAdd(&hist[qi * nbins + i], c);
            below = __shfl(incl, 63, 64);
        }
    }
}

// Pass 2.  One wave per query: thr[q] = (t, need, below).  Fewer than k rows in all: t = nbins (every row is below it), need = 0.
__global__ __launch_bounds__(64) void bin_thresh_kernel(const uint32_t *__restrict__ hist, int nbins, int k, uint32_t *__restrict__ thr) {
    const int lane = threadIdx.x;
    const uint32_t *h = hist + (int64_t)blockIdx.x * nbins;
    uint32_t below = 0, t = (uint32_t)nbins, need = 0;
    for (int base = 0; base < nbins; base += 64) {
        const uint32_t c = base + lane < nbins ? h[base + lane] : 0u;
        const uint32_t incl = below + ivr_wave_incl_scan(c);
        const uint64_t hit = __ballot(incl >= (uint32_t)k);
        if (hit) {
            const int first = __ffsll((unsigned long long)hit) - 1;
            const uint32_t incl_f = __shfl(incl, first, 64), c_f = __shfl(c, first, 64);
            t = (uint32_t)(base + first);
            below = incl_f - c_f;
            need = (uint32_t)k - below;
            break;
        }
        below = __shfl(incl, 63, 64);
    }
    if (lane == 0) {
        thr[blockIdx.x * 4 + 0] = t;
        thr[blockIdx.x * 4 + 1] = need;
        thr[blockIdx.x * 4 + 2] = below;
    }
}

// Pass 3a.  cnt_lt[q][g], cnt_eq[q][g]: rows of 64-row group g with dist < t and with dist == t
template <int W>
__global__ __launch_bounds__(256) void bin_count_kernel(const uint4 *__restrict__ data, int64_t ntotal, int64_t ngroups,
                                                        const uint4 *__restrict__ q, int nqc, const uint32_t *__restrict__ thr,
                                                        uint32_t *__restrict__ cnt_lt, uint32_t *__restrict__ cnt_eq) {
    const int lane = threadIdx.x & 63;
    const int64_t g = blockIdx.x * 4ll + (threadIdx.x >> 6);
    if (g >= ngroups) return;
    const bool valid = g * 64 + lane < ntotal;
    uint4 row[W];
    bin_load_row<W>(data, g, row);
    for (int qi = 0; qi < nqc; ++qi) {
        const uint32_t d = bin_dist<W>(row, q + (int64_t)qi * W);
        const uint32_t t = thr[qi * 4];
        const uint64_t lt = __ballot(valid && d < t), eq = __ballot(valid && d == t);
        if (lane == 0) {
            cnt_lt[qi * ngroups + g] = (uint32_t)__popcll(lt);
            cnt_eq[qi * ngroups + g] = (uint32_t)__popcll(eq);
        }
    }
}

// Pass 3b.  In-place exclusive prefix over the n entries of row blockIdx.x of a ([rows][n]); one workgroup per row, 8192 entries per
// step (two steps at 1M rows), the running total carried from step to step.  Global loads and stores are coalesced; a thread scans 32
// consecutive entries, which it reads from an LDS image of the step padded by one word per 32 (thread t starts at word 33 t: no bank
// conflicts)
__global__ __launch_bounds__(256) void bin_scan_kernel(uint32_t *__restrict__ a, int64_t n) {
    constexpr int E = 32, kTile = 256 * E;
    __shared__ uint32_t buf[kTile + kTile / 32];
    __shared__ uint32_t ws[4];
    uint32_t *row = a + (int64_t)blockIdx.x * n;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    uint32_t carry = 0;
    for (int64_t base = 0; base < n; base += kTile) {
#pragma unroll
        for (int e = 0; e < E; ++e) {
            const int j = e * 256 + tid;
            buf[j + (j >> 5)] = base + j < n ? row[base + j] : 0u;
        }
        __syncthreads();
        uint32_t v[E], sum = 0;
#pragma unroll
        for (int e = 0; e < E; ++e) {
            v[e] = buf[tid * (E + 1) + e];
            sum += v[e];
        }
        const uint32_t incl = ivr_wave_incl_scan(sum);
        if (lane == 63) ws[wave] = incl;
        __syncthreads();
        uint32_t woff = 0, tot = 0;
        for (int w = 0; w < 4; ++w) {
            if (w < wave) woff += ws[w];
            tot += ws[w];
        }
        uint32_t off = carry + woff + incl - sum;
#pragma unroll
        for (int e = 0; e < E; ++e) {
            buf[tid * (E + 1) + e] = off;
            off += v[e];
        }
        __syncthreads();
#pragma unroll
        for (int e = 0; e < E; ++e) {
            const int j = e * 256 + tid;
            if (base + j < n) row[base + j] = buf[j + (j >> 5)];
        }
        carry += tot;
        __syncthreads();
    }
}

// Pass 3c.  cand[q][slot] = (dist << 32 | row): rows below t at slot (rows below t in earlier groups) + (rank in the group), rows at t
// with rank r among the rows at t (all groups, ascending row) below need at slot below + r
template <int W>
__global__ __launch_bounds__(256) void bin_emit_kernel(const uint4 *__restrict__ data, int64_t ntotal, int64_t ngroups,
                                                       const uint4 *__restrict__ q, int nqc, const uint32_t *__restrict__ thr,
                                                       const uint32_t *__restrict__ pre_lt, const uint32_t *__restrict__ pre_eq, int k,
                                                       uint64_t *__restrict__ cand) {
    const int lane = threadIdx.x & 63;
    const int64_t g = blockIdx.x * 4ll + (threadIdx.x >> 6);
    if (g >= ngroups) return;
    const int64_t r = g * 64 + lane;
    const bool valid = r < ntotal;
    const uint64_t lower = (1ull << lane) - 1ull;
    uint4 row[W];
    bin_load_row<W>(data, g, row);
    for (int qi = 0; qi < nqc; ++qi) {
        const uint32_t d = bin_dist<W>(row, q + (int64_t)qi * W);
        const uint32_t t = thr[qi * 4], need = thr[qi * 4 + 1], below = thr[qi * 4 + 2];
        const bool is_lt = valid && d < t, is_eq = valid && d == t;
        const uint64_t lt = __ballot(is_lt), eq = __ballot(is_eq);
        if ((lt | eq) == 0) continue;
        const uint64_t key = ((uint64_t)d << 32) | (uint64_t)r;
        uint64_t *out = cand + (int64_t)qi * k;
        if (is_lt) {
            const uint32_t slot = pre_lt[qi * ngroups + g] + (uint32_t)__popcll(lt & lower);
            if (slot < (uint32_t)k) out[slot] = key;
        } else if (is_eq) {
            const uint32_t rank = pre_eq[qi * ngroups + g] + (uint32_t)__popcll(eq & lower);
            if (rank < need && below + rank < (uint32_t)k) out[below + rank] = key;
        }
    }
}

// Pass 4.  One workgroup per query: its k keys in ascending (distance, row) order -> D, I; empty slots (INT32_MAX, -1)
__global__ __launch_bounds__(256) void bin_order_kernel(const uint64_t *__restrict__ cand, int k, int32_t *__restrict__ D, int64_t *__restrict__ I) {
    __shared__ uint64_t s[IVR_MAX_K];
    const int tid = threadIdx.x;
    int P = 2;
    while (P < k) P <<= 1;
    const uint64_t *c = cand + (int64_t)blockIdx.x * k;
    for (int i = tid; i < P; i += 256) s[i] = i < k ? c[i] : kBinEmpty;
    __syncthreads();
    for (int size = 2; size <= P; size <<= 1) {
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int i = tid; i < P / 2; i += 256) {
                const int lo = ((i / stride) * stride << 1) + (i % stride), hi = lo + stride;
                const bool up = (lo & size) == 0;
                const uint64_t a = s[lo], b = s[hi];
                if ((a > b) == up) {
                    s[lo] = b;
                    s[hi] = a;
                }
            }
            __syncthreads();
        }
    }
    for (int i = tid; i < k; i += 256) {
        const uint64_t key = s[i];
        D[(int64_t)blockIdx.x * k + i] = key == kBinEmpty ? INT32_MAX : (int32_t)(key >> 32);
        I[(int64_t)blockIdx.x * k + i] = key == kBinEmpty ? -1 : (int64_t)(key & 0xffffffffull);
    }
}

// ---- sign-bit encoder -------------------------------------------------------------------------------------------------------------
// proj = x rot^T on the float32 MFMA, packed to sign bits in the same kernel.  A wave owns 16 rows x 64 bits: four 16 x 16 accumulator
// tiles (independent, so the MFMA issues back to back), summed over d in ascending 16-float chunks in the order of mfma_chunk4.  In an
// accumulator tile lane l holds column l & 15 and rows 4 (l >> 4) + reg, so the ballot of register reg of tile t carries, in bits
// 16 g .. 16 g + 15, the bits 16 t .. 16 t + 15 of row 4 g + reg; lanes 0 .. 15 put the 64 bits of one row each together.
template <int U>
__global__ __launch_bounds__(256) void sign_encode_mfma_kernel(const float *__restrict__ x, int64_t n, int d, const float *__restrict__ rot,
                                                               const float *__restrict__ thr, int nbits, int code_size,
                                                               uint8_t *__restrict__ codes, float *__restrict__ proj, int vec) {
    const int lane = threadIdx.x & 63;
    const int64_t i0 = (blockIdx.x * 4ll + (threadIdx.x >> 6)) * 16;
    if (i0 >= n) return;
    const int j0 = blockIdx.y * 64;
    const int li = lane & 15, g = lane >> 4;
    const float *xr = x + std::min<int64_t>(i0 + li, n - 1) * d;
    const float *rr[4];
    float th[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const int j = min(j0 + 16 * t + li, nbits - 1);
        rr[t] = rot + (int64_t)j * d;
        th[t] = thr ? thr[j] : 0.f;
    }
    f32x4 acc[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    // U chunks per round: their 5 U loads are issued together, then the 16 U MFMAs (a chunk past d loads zeros and adds nothing)
    const int nchunks = (d + 15) / 16;
    for (int c0 = 0; c0 < nchunks; c0 += U) {
        float4 a[U], b[U][4];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int k0 = 16 * (c0 + u) + 4 * g;
            const bool v = vec && k0 + 3 < d;
            a[u] = ivr_load_quad(xr, k0, d, v);
#pragma unroll
            for (int t = 0; t < 4; ++t) b[u][t] = ivr_load_quad(rr[t], k0, d, v);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
#pragma unroll
            for (int t = 0; t < 4; ++t) mfma_chunk4(acc[t], a[u], b[u][t]);
        }
    }
    uint64_t bal[4][4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const int j = j0 + 16 * t + li;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float p = acc[t][r];
            const int64_t i = i0 + 4 * g + r;
            if (proj && i < n && j < nbits) proj[i * nbits + j] = p;
            bal[t][r] = __ballot(j < nbits && p - th[t] >= 0.0f);
        }
    }
    if (lane < 16 && i0 + lane < n) {
        const int r = lane & 3, sh = 16 * (lane >> 2);
        uint64_t code = 0;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const uint64_t b = r == 0 ? bal[t][0] : r == 1 ? bal[t][1] : r == 2 ? bal[t][2] : bal[t][3];
            code |= ((b >> sh) & 0xffffull) << (16 * t);
        }
        uint8_t *o = codes + (i0 + lane) * code_size;
        for (int b = 0; b < 8; ++b)
            if (j0 / 8 + b < code_size) o[j0 / 8 + b] = (uint8_t)(code >> (8 * b));
    }
}

// rot == NULL: proj[i][j] = x[i][j] (the first nbits coordinates).  One wave per (row, 64 bits)
__global__ __launch_bounds__(256) void sign_encode_plain_kernel(const float *__restrict__ x, int64_t n, int d, const float *__restrict__ thr,
                                                                int nbits, int code_size, uint8_t *__restrict__ codes,
                                                                float *__restrict__ proj) {
    const int lane = threadIdx.x & 63;
    const int64_t i = blockIdx.x * 4ll + (threadIdx.x >> 6);
    if (i >= n) return;
    const int j0 = blockIdx.y * 64, j = j0 + lane;
    const bool in = j < nbits;
    const float p = in ? x[i * d + j] : 0.f;
    const float th = in && thr ? thr[j] : 0.f;
    if (proj && in) proj[i * nbits + j] = p;
    const uint64_t code = __ballot(in && p - th >= 0.0f);
    if (lane < 8 && j0 / 8 + lane < code_size) codes[i * code_size + j0 / 8 + lane] = (uint8_t)(code >> (8 * lane));
}

void bin_launch_pack(const ivr_bin_index *x, const uint8_t *src, uint4 *dst, int64_t start, int64_t n, int interleaved, hipStream_t s) {
    const int64_t threads = ivr_ceil_div(n, 64) * x->w16 * 64;
    const int vec = x->code_size % 4 == 0 && ((uintptr_t)src & 3) == 0;
    hipLaunchKernelGGL(bin_pack_kernel, dim3((unsigned)ivr_ceil_div(threads, 256)), dim3(256), 0, s, src, dst, start, n, x->nbits, x->code_size,
                       x->w16, interleaved, vec);
}

}  // namespace

extern "C" {

int ivr_bin_index_block_rows(void) { return kBinBlockRows; }

int ivr_bin_index_create(ivr_ctx *ctx, int nbits, int64_t capacity_rows, ivr_bin_index **out) {
    IVR_REQUIRE(ctx && out, "ivr_bin_index_create: NULL argument");
    IVR_REQUIRE(nbits >= 1 && nbits <= IVR_BIN_MAX_BITS, "ivr_bin_index_create: nbits=%d out of range [1,%d]", nbits, IVR_BIN_MAX_BITS);
    IVR_REQUIRE(capacity_rows >= 0 && capacity_rows < (1ll << 31) - kBinBlockRows, "ivr_bin_index_create: capacity %lld out of range",
                (long long)capacity_rows);
    IVR_HIP(hipSetDevice(ctx->device));
    ivr_bin_index *x = new ivr_bin_index();
    x->ctx = ctx;
    x->nbits = nbits;
    x->code_size = (nbits + 7) / 8;
    x->w16 = bin_words(x->code_size);
    x->granule = kBinBlockRows;
    x->group_words = (int64_t)x->w16 * 64;
    const int rc = x->grow(capacity_rows);
    if (rc != IVR_OK) {
        delete x;
        return rc;
    }
    *out = x;
    return IVR_OK;
}

int ivr_bin_index_destroy(ivr_bin_index *x) {
    delete x;                        // the rows and the workspace buffers free themselves
    return IVR_OK;
}

int ivr_bin_index_reset(ivr_bin_index *x) {
    IVR_REQUIRE(x, "ivr_bin_index_reset: NULL index");
    return x->reset(true);                       // the distance loop reads the pad bits and the scans whole groups: all zero again
}

int64_t ivr_bin_index_ntotal(ivr_bin_index *x) { return x ? x->ntotal : 0; }

int ivr_bin_index_add(ivr_bin_index *x, const uint8_t *codes, int64_t n, ivr_stream stream) {
    IVR_REQUIRE(x, "ivr_bin_index_add: NULL argument");
    return x->add("ivr_bin_index_add", codes, n, [&] { bin_launch_pack(x, codes, x->data, x->ntotal, n, 1, (hipStream_t)stream); });
}

int ivr_bin_index_get_codes(ivr_bin_index *x, int64_t start, int64_t n, uint8_t *out, ivr_stream stream) {
    IVR_REQUIRE(x, "ivr_bin_index_get_codes: NULL argument");
    return x->get_codes("ivr_bin_index_get_codes", start, n, out, [&] {
        const int64_t threads = n * ((x->code_size + 3) / 4);
        hipLaunchKernelGGL(bin_unpack_kernel, dim3((unsigned)ivr_ceil_div(threads, 256)), dim3(256), 0, (hipStream_t)stream,
                           reinterpret_cast<const uint32_t *>(x->data), start, n, x->code_size, x->w16, out);
    });
}

int ivr_bin_index_search(ivr_bin_index *x, const uint8_t *qcodes, int nq, int k, int32_t *D, int64_t *I, ivr_stream stream) {
    IVR_REQUIRE(x && qcodes && D && I, "ivr_bin_index_search: NULL argument");
    IVR_REQUIRE(nq >= 1, "ivr_bin_index_search: nq=%d < 1", nq);
    IVR_REQUIRE(k >= 1 && k <= IVR_MAX_K, "ivr_bin_index_search: k=%d outside [1,%d]", k, IVR_MAX_K);
    std::lock_guard<std::mutex> lk(x->mu);
    IVR_HIP(hipSetDevice(x->ctx->device));
    hipStream_t s = (hipStream_t)stream;
    const int64_t ntotal = x->ntotal, nblocks = ivr_ceil_div(ntotal, kBinBlockRows), ngroups = ivr_ceil_div(ntotal, 64);
    const int qc = std::min(x->chunk(), nq), nbins = x->nbits + 1;
    const size_t cnt_row = (size_t)std::max<int64_t>(ngroups, 1) * sizeof(uint32_t);
    int rc = ivr_reserve({{&x->q, (size_t)nq * x->w16 * sizeof(uint4)},
                          {&x->hist, (size_t)qc * nbins * sizeof(uint32_t)},
                          {&x->thr, (size_t)qc * 4 * sizeof(uint32_t)},
                          {&x->cnt, 2 * qc * cnt_row},
                          {&x->cand, (size_t)qc * k * sizeof(uint64_t)}});
    if (rc != IVR_OK) return rc;
    bin_launch_pack(x, qcodes, x->q, 0, nq, 0, s);
    IVR_LAUNCH_CHECK();
    // histogram pass: workgroups per CU.  Every workgroup ends with atomics on the same few bins of the global histogram, so few
    // queries (little work per block) run best with 2 per CU and a full chunk with what its LDS lets be resident (3 at 256 bits);
    // measured at 1M rows x 256 bits: 1 query 13 / 13 / 18 / 30 us with 1 / 2 / 4 / 8 per CU, 47 queries 88 / 60 / 52 us with 1 / 2 / 3
    const size_t hist_lds = (size_t)qc * nbins * sizeof(uint32_t);
    const int64_t hist_per_cu = std::max<int64_t>(1, std::min<int64_t>(qc <= 8 ? 2 : 4, (160 * 1024) / (int64_t)hist_lds));
    const unsigned hist_grid = (unsigned)std::max<int64_t>(1, std::min<int64_t>(nblocks, hist_per_cu * x->ctx->cu_count));
    for (int c0 = 0; c0 < nq; c0 += qc) {
        const int nqc = std::min(qc, nq - c0);
        const uint4 *q = x->q + (int64_t)c0 * x->w16;
        uint32_t *cnt_lt = x->cnt, *cnt_eq = x->cnt + (int64_t)nqc * ngroups;
        IVR_HIP(hipMemsetAsync(x->cand, 0xff, (size_t)nqc * k * sizeof(uint64_t), s));
        if (ntotal > 0) {
            IVR_HIP(hipMemsetAsync(x->hist, 0, (size_t)nqc * nbins * sizeof(uint32_t), s));
            const double scan_bytes = (double)ngroups * x->group_words * 16;
            bin_with_words(x->w16, [&](auto w) {
                constexpr int W = decltype(w)::value;
                {
                    IvrProf prof("bin_hist", s, scan_bytes);
                    hipLaunchKernelGGL(bin_hist_kernel<W>, dim3(hist_grid), dim3(256), (size_t)nqc * nbins * sizeof(uint32_t), s, x->data, ntotal,
                                       nblocks, q, nqc, nbins, k, x->hist);
                }
                {
                    IvrProf prof("bin_thresh", s, (double)nqc * nbins * 4, true);
                    hipLaunchKernelGGL(bin_thresh_kernel, dim3(nqc), dim3(64), 0, s, x->hist, nbins, k, x->thr);
                }
                {
                    IvrProf prof("bin_count", s, scan_bytes);
                    hipLaunchKernelGGL(bin_count_kernel<W>, dim3((unsigned)nblocks), dim3(256), 0, s, x->data, ntotal, ngroups, q, nqc, x->thr,
                                       cnt_lt, cnt_eq);
                }
                {
                    IvrProf prof("bin_scan", s, (double)nqc * ngroups * 16, true);
                    hipLaunchKernelGGL(bin_scan_kernel, dim3(2 * nqc), dim3(256), 0, s, x->cnt, ngroups);
                }
                {
                    IvrProf prof("bin_emit", s, scan_bytes);
                    hipLaunchKernelGGL(bin_emit_kernel<W>, dim3((unsigned)nblocks), dim3(256), 0, s, x->data, ntotal, ngroups, q, nqc, x->thr,
                                       cnt_lt, cnt_eq, k, x->cand);
                }
            });
            IVR_LAUNCH_CHECK();
        }
        IvrProf prof("bin_order", s, (double)nqc * k * 20, true);
        hipLaunchKernelGGL(bin_order_kernel, dim3(nqc), dim3(256), 0, s, x->cand, k, D + (int64_t)c0 * k, I + (int64_t)c0 * k);
        IVR_LAUNCH_CHECK();
    }
    return IVR_OK;
}

int ivr_sign_encode(ivr_ctx *ctx, const float *x, int64_t n, int d, const float *rot, const float *thr, int nbits, uint8_t *codes,
                    float *proj, ivr_stream stream) {
    IVR_REQUIRE(ctx && ((x && codes) || n == 0), "ivr_sign_encode: NULL argument");
    IVR_REQUIRE(n >= 0 && n < (1ll << 33), "ivr_sign_encode: n=%lld out of range", (long long)n);
    IVR_REQUIRE(d >= 1 && d <= 65536, "ivr_sign_encode: d=%d out of range [1,65536]", d);
    IVR_REQUIRE(nbits >= 1 && nbits <= IVR_BIN_MAX_BITS, "ivr_sign_encode: nbits=%d out of range [1,%d]", nbits, IVR_BIN_MAX_BITS);
    IVR_REQUIRE(rot || nbits <= d, "ivr_sign_encode: nbits=%d > d=%d without a rotation", nbits, d);
    if (n == 0) return IVR_OK;
    IVR_HIP(hipSetDevice(ctx->device));
    hipStream_t s = (hipStream_t)stream;
    const int code_size = (nbits + 7) / 8;
    const unsigned slabs = (unsigned)ivr_ceil_div(nbits, 64);
    if (rot) {
        const int vec = d % 4 == 0 && (((uintptr_t)x | (uintptr_t)rot) & 15) == 0;
        IvrProf prof("sign_encode", s, 2.0 * (double)n * d * nbits);
        // a few rows (queries) are latency-bound: four chunks of loads in flight per wave; many rows run best with the registers of one
        auto *kern = n <= kSignEncodeSmall ? sign_encode_mfma_kernel<4> : sign_encode_mfma_kernel<1>;
        hipLaunchKernelGGL(kern, dim3((unsigned)ivr_ceil_div(n, 64), slabs), dim3(256), 0, s, x, n, d, rot, thr, nbits, code_size, codes, proj,
                           vec);
    } else {
        IvrProf prof("sign_encode", s, (double)n * (nbits * 4 + code_size));
        hipLaunchKernelGGL(sign_encode_plain_kernel, dim3((unsigned)ivr_ceil_div(n, 4), slabs), dim3(256), 0, s, x, n, d, thr, nbits, code_size,
                           codes, proj);
    }
    IVR_LAUNCH_CHECK();
    return IVR_OK;
}

}  // extern "C"
