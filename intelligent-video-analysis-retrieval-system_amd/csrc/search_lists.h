// What the inverted-list scans and the int8 scans share: search_ivf.hip (lists over the flat index), search_sq.hip (the scalar-quantiser
// index) and search_ivfsq.hip (lists over scalar-quantiser codes).  The probe tables of a chunk of queries (probe_slots / probe_count /
// probe_offsets / probe_fill, with list_run and the key source SrcSlots of the selection behind them), and the int8 operand helpers of
// the v_mfma_i32_16x16x64_i8 scans (sq_stage_kernel, sq_frag, sq_combine, SQ_NO_CONTRACT).  Each body is stated once, here; every file
// that includes the header gets instantiations of its own.  Not part of the C ABI.
#pragma once
#include "ivr_common.h"
#include "search_internal.h"

namespace {

// ---- probe tables ------------------------------------------------------------------------------------------------------------------
// keys of the scratch a chunk of queries may fill: 2^25 slots of 8 bytes = 256 MiB, plus one query's stretch when a single query
// probes more rows than that (its stretch is never split)
constexpr int64_t kIvfChunkSlots = 1ll << 25;
// pairs of a chunk: bounds the pair tables (20 bytes per pair) at 80 MiB
constexpr int64_t kIvfChunkPairs = 1ll << 22;

// rows of list l, clipped to the stored rows
__device__ __forceinline__ void list_run(const int64_t *__restrict__ list_off, int64_t l, int64_t ntotal, int64_t &r0, int64_t &r1) {
    r0 = min(max(list_off[l], (int64_t)0), ntotal);
    r1 = min(max(list_off[l + 1], r0), ntotal);
}

// One wave per query of the chunk.  slot[q][j] = first slot of entry j's list in the scratch (q * qstride + the rows of the query's
// earlier lists), -1 for a skipped entry; qtotal[q] = the rows the query probes.  A query whose lists hold more than qstride rows
// (the caller's bound is wrong) probes nothing rather than write past its stretch.
__global__ __launch_bounds__(256) void probe_slots_kernel(const int64_t *__restrict__ assign, int p, int nqc, const int64_t *__restrict__ list_off,
                                                          int nlist, int64_t ntotal, int64_t qstride, int64_t *__restrict__ slot,
                                                          int64_t *__restrict__ qtotal) {
    const int lane = threadIdx.x & 63;
    const int q = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (q >= nqc) return;
    const int64_t *a = assign + (int64_t)q * p;
    int64_t total = 0;
    for (int pass = 0; pass < 2; ++pass) {
        const bool fits = total <= qstride;          // pass 1 only: the total of pass 0
        int64_t carry = 0;
        for (int j0 = 0; j0 < p; j0 += 64) {
            const int j = j0 + lane;
            const bool valid = probe_valid(a, j, p, nlist);
            int64_t size = 0;
            if (valid) {
                int64_t r0, r1;
                list_run(list_off, a[j], ntotal, r0, r1);
                size = r1 - r0;
            }
            int64_t inc = size;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const int64_t t = __shfl_up(inc, o, 64);
                if (lane >= o) inc += t;
            }
            if (pass == 1 && j < p) slot[(int64_t)q * p + j] = valid && fits ? (int64_t)q * qstride + carry + inc - size : -1;
            carry += __shfl(inc, 63, 64);
        }
        total = carry;
    }
    if (lane == 0) qtotal[q] = total <= qstride ? total : 0;
}

__global__ __launch_bounds__(256) void probe_count_kernel(const int64_t *__restrict__ assign, const int64_t *__restrict__ slot, int64_t npairs,
                                                          int *__restrict__ count) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < npairs && slot[i] >= 0) atomicAdd(&count[assign[i]], 1);
}

// one workgroup of 256 threads: pair_off[l] = pairs of the lists below l, tile_off[l] = their 16-query pair tiles, l <= nlist; the
// counts become the fill cursors (zero)
__global__ __launch_bounds__(256) void probe_offsets_kernel(int *__restrict__ count, int nlist, int64_t *__restrict__ pair_off,
                                                            int64_t *__restrict__ tile_off) {
    __shared__ int64_t wp[4], wt[4];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    int64_t cp = 0, ct = 0;                          // carried over the rounds
    for (int l0 = 0; l0 <= nlist; l0 += 256) {
        const int l = l0 + threadIdx.x;
        const int64_t c = l < nlist ? count[l] : 0, t = (c + 15) >> 4;
        if (l < nlist) count[l] = 0;
        int64_t ip = c, it = t;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int64_t a = __shfl_up(ip, o, 64), b = __shfl_up(it, o, 64);
            if (lane >= o) {
                ip += a;
                it += b;
            }
        }
        if (lane == 63) {
            wp[w] = ip;
            wt[w] = it;
        }
        __syncthreads();
        int64_t bp = cp, bt = ct, tp = 0, tt = 0;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            if (i < w) {
                bp += wp[i];
                bt += wt[i];
            }
            tp += wp[i];
            tt += wt[i];
        }
        if (l <= nlist) {
            pair_off[l] = bp + ip - c;
            tile_off[l] = bt + it - t;
        }
        cp += tp;
        ct += tt;
        __syncthreads();
    }
}

__global__ __launch_bounds__(256) void probe_fill_kernel(const int64_t *__restrict__ assign, const int64_t *__restrict__ slot, int p, int64_t npairs,
                                                         int *__restrict__ cursor, const int64_t *__restrict__ pair_off,
                                                         int *__restrict__ pair_q, int64_t *__restrict__ pair_slot) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= npairs) return;
    const int64_t s = slot[i];
    if (s < 0) return;
    const int64_t l = assign[i];
    const int64_t at = pair_off[l] + atomicAdd(&cursor[l], 1);      // the order of a list's queries does not reach the result
    pair_q[at] = (int)(i / p);
    pair_slot[at] = s;
}

struct SrcSlots {      // the keys of query q: slots [q * qstride, q * qstride + qtotal[q]) of the scratch
    const uint64_t *keys;
    const int64_t *qtotal;
    int64_t qstride;
    int64_t n;         // the longest stretch a query of the launch may hold
    __device__ uint64_t key(int q, int64_t i) const { return i < qtotal[q] ? keys[(int64_t)q * qstride + i] : 0; }
};

// ---- int8 operands -----------------------------------------------------------------------------------------------------------------
typedef int i32x4 __attribute__((ext_vector_type(4)));

// The definitions count float32 roundings.  The build contracts a * b + c into one fused multiply-add, and __fmul_rn / __fadd_rn are
// the plain operators in this toolchain's headers, so the kernels that evaluate a definition turn contraction off for their body and write the operators out (the pragma is lexical: it
// does not reach into an inlined function).  Division is correctly rounded by default
#define SQ_NO_CONTRACT _Pragma("clang fp contract(off)")

__device__ __forceinline__ i32x4 sq_frag(const uint4 &v) { return __builtin_bit_cast(i32x4, v); }
// 128 acc_h + acc_l; unsigned so that an intermediate beyond int32 wraps (the sum itself always fits)
__device__ __forceinline__ int32_t sq_combine(int h, int l) { return (int32_t)(128u * (uint32_t)h + (uint32_t)l); }

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

}  // namespace
