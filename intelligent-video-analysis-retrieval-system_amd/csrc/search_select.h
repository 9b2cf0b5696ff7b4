// Per-query exact top-k of 64-bit keys (select_topk_kernel) with its key sources, shared by search.hip (group maxima, tile maxima,
// re-scored keys) and search_merge.hip (shard merge).  Without relocatable device code a kernel template that two translation units
// launch has to live in a header; each instantiation is emitted by the one file that launches it, and the two sets are disjoint.
// The unnamed namespace keeps them private to their file; tools/isa_compare.py reports an instantiation that two objects emit.
#pragma once
#include "ivr_common.h"
#include "search_internal.h"

#include <cfloat>

namespace {

constexpr int kSelThreads = 1024;   // select kernel block size
constexpr int kMaxSort = IVR_MAX_K; // bitonic sort capacity (power of two)

// Verification of the bf16 candidate scan, done by the final selection of each query (select_topk_kernel<SrcKeys, OUT_DI>): does
// the (kp+1)-th approximate group maximum + error bound stay strictly below the k-th exact score?  ok[q] = 1 keeps the fast
// result; otherwise the query's tile is flagged for the exact pass.  tile_flag[0..3] is reset by the group selection launched
// before (same stream), so the blocks of the final selection only ever raise flags.
struct VerifyArgs {
    const float *gmax = nullptr;          // approximate group maxima [query column][mstride]
    int64_t mstride = 0;
    const uint32_t *sel = nullptr;        // [nq][ksel2]: selected groups, entry kp = the first excluded one
    int ksel2 = 0, kp = 0;
    const float *qnorm = nullptr;         // upper bound of each query's stored norm (tile_rows_kernel)
    float rel_eps = 0.f;
    const unsigned int *maxnorm_bits = nullptr;
    int *ok = nullptr;                    // NULL = no verification in this launch
    int *tile_flag = nullptr;
    // large-batch scan (scanq_kernel: both operands rounded to bf16): the bound uses the measured rounding residuals,
    //   |approx - exact| <= (|q| + |dq|) max|dr| + |dq| max|r| + acc_eps |q| max|r|,   dq = q - bf16(q), dr = row - bf16(row);
    // a failed query is appended to fail_list (its exact pass is list-driven, scan_groupmax_list_kernel)
    const float *qdelta = nullptr;        // non-NULL selects this mode
    const unsigned int *maxdelta_bits = nullptr;
    float acc_eps = 0.f;
    int *fail_count = nullptr, *fail_list = nullptr;
};

// list-driven launches (the exact pass behind the large-batch scan): block b works on list position b and exits when
// b >= *count; results go to output row list[b]
struct ListArgs {
    const int *count = nullptr;
    const int *list = nullptr;
};

// ---------------------------------------------------------------------------------------------
// per-query exact top-k of 64-bit keys: MSB-first radix select (8 x 8 bits) + bitonic sort
// ---------------------------------------------------------------------------------------------
struct SrcGroupMax {   // pass 2: keys from the group-maximum column of query q
    const float *gmax;
    int64_t mstride;
    int64_t n;
    __device__ uint64_t key(int q, int64_t i) const {
        return ivr_key(gmax[(int64_t)q * mstride + i], (uint32_t)i);
    }
};
struct SrcTilesOf {    // large-batch scan, second level: the 16-row tile maxima of the 128-row blocks selected at the first level
    const float *tmax;
    int64_t tstride;
    const uint32_t *selb;      // [nq][kb] selected blocks (0xFFFFFFFF = none)
    int kb;
    int64_t ntiles;            // ceil(ntotal / 16)
    int64_t n;                 // kb * 8
    __device__ uint64_t key(int q, int64_t i) const {
        const uint32_t b = selb[(int64_t)q * kb + (i >> 3)];
        if (b == 0xFFFFFFFFu) return 0;
        const int64_t t = (int64_t)b * 8 + (i & 7);
        if (t >= ntiles) return 0;
        return ivr_key(tmax[(int64_t)q * tstride + t], (uint32_t)t);
    }
};
struct SrcKeys {       // pass 4: keys already materialised
    const uint64_t *keys;
    int64_t n;
    __device__ uint64_t key(int q, int64_t i) const { return keys[(int64_t)q * n + i]; }
};
struct SrcParts {      // shard merge: candidate p = part*k + j; ties resolve to the lower p = lower global id
    const float *D;
    const int64_t *I;
    int nq, k;
    int64_t n;         // parts * k
    __device__ uint64_t key(int q, int64_t p) const {
        const int64_t part = p / k, j = p % k;
        const int64_t off = (part * nq + q) * k + j;
        if (I[off] < 0) return 0;
        return ivr_key(D[off], (uint32_t)p);
    }
};

struct SrcPacked {     // shard merge straight from the all-gather buffer: candidate = three int32 words (score bits, id lo, id hi)
    const int32_t *cand;   // [parts][nq][k][3]
    int nq, k;
    int64_t n;             // parts * k
    __device__ const int32_t *at(int q, int64_t p) const { return cand + (((p / k) * nq + q) * k + (p % k)) * 3; }
    __device__ uint64_t key(int q, int64_t p) const {
        const int32_t *c = at(q, p);
        if (c[2] < 0) return 0;                       // id -1: unused slot
        return ivr_key(__int_as_float(c[0]), (uint32_t)p);
    }
};

// OUT_DI_IDS: OUT_DI on an id-mapped index, the label of row r is ids[r] (the table travels in the I_parts argument); an
// instantiation of its own, so that the kernels a plain index launches stay as they are
// OUT_DI_POS / OUT_DI_IDS_POS (ivr_index_search_reconstruct): OUT_DI / OUT_DI_IDS that also report the row behind every result slot,
// as its number in the scanned view (-1 for an unused slot), into an int64 [nq][k] buffer that travels in the out_groups argument
// (unused by every OUT_DI* otherwise).  Instantiations of their own again: the kernels of every other search keep their code.
enum { OUT_GROUPS = 0, OUT_DI = 1, OUT_DI_PARTS = 2, OUT_DI_PACKED = 3, OUT_DI_IDS = 4, OUT_DI_POS = 5, OUT_DI_IDS_POS = 6 };

constexpr int kRegKeys = 16;   // keys cached per thread: n <= 16 * 1024 is selected without re-reading global memory

template <typename Src, int OUT>
__global__ __launch_bounds__(kSelThreads) void select_topk_kernel(Src src, int qcol0, int k, int64_t id_base,
                                                                  uint32_t *__restrict__ out_groups,
                                                                  float *__restrict__ D, int64_t *__restrict__ I,
                                                                  const int64_t *__restrict__ I_parts,
                                                                  const int *__restrict__ skip = nullptr, VerifyArgs vf = VerifyArgs(),
                                                                  int *__restrict__ reset_flags = nullptr, ListArgs la = ListArgs()) {
    if (reset_flags && blockIdx.x == 0 && threadIdx.x < 4) reset_flags[threadIdx.x] = 0;
    if (skip && skip[blockIdx.x]) return;          // whole block: this query kept its fast-path result
    if (la.count && (int)blockIdx.x >= *la.count) return;
    __shared__ unsigned int hist[256];
    __shared__ unsigned long long s_prefix, s_mask;
    __shared__ unsigned int s_kth, s_cnt, s_valid;
    __shared__ uint64_t sorted[kMaxSort];
    const int q = blockIdx.x;
    const int qsrc = qcol0 + q;
    const int tid = threadIdx.x;
    const int nthr = blockDim.x;          // 256 for short candidate lists (cheaper barriers), else 1024
    const int64_t n = src.n;
    // The candidate keys of one query are few (N/64 group maxima, or k*64 rescored rows): keep them in registers so
    // that the eight radix passes cost LDS histogram time only, not eight dependent trips to L2.
    const bool cached = n <= (int64_t)kRegKeys * nthr;
    uint64_t kreg[kRegKeys];
    if (cached) {
#pragma unroll
        for (int j = 0; j < kRegKeys; ++j) {
            const int64_t i = (int64_t)j * nthr + tid;
            kreg[j] = i < n ? src.key(qsrc, i) : 0;
        }
    }
    auto for_each_key = [&](auto &&fn) {
        if (cached) {
#pragma unroll
            for (int j = 0; j < kRegKeys; ++j) fn(kreg[j]);
        } else {
            for (int64_t i = tid; i < n; i += nthr) fn(src.key(qsrc, i));
        }
    };

    // count valid keys (key 0 = absent)
    if (tid == 0) s_valid = 0;
    __syncthreads();
    {
        unsigned int c = 0;
        for_each_key([&](uint64_t key) { c += key != 0; });
        for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
        if ((tid & 63) == 0 && c) atomicAdd(&s_valid, c);
    }
    __syncthreads();
    const unsigned int keff = min((unsigned int)k, s_valid);
    __shared__ uint64_t wmax[kSelThreads / 64];
    // Small k (the reference asks for 10..50; here up to 16 keys per wave): no serial extraction rounds.
    //  (1) every thread's largest key; (2) a lower bound T of the keff-th largest key: each wave removes the largest of its
    //  per-thread maxima r = ceil(keff / #waves) times (one DPP wave-max of the 32-bit score per round; equal scores leave
    //  together) and T is the smallest score removed last by any wave - every wave then holds >= r keys >= T, the block >= keff;
    //  (3) the keys >= T are collected, typically a few times keff of them; (4) each survivor counts the survivors above it:
    //  that is its rank (keys are unique).  Four barriers in all; the radix / extraction paths below remain the fallback when
    //  too many keys survive (scores tied in bulk).
    __shared__ uint64_t surv[kSelThreads];
    __shared__ unsigned int s_nsurv;
    __shared__ uint32_t wlow[kSelThreads / 64];
    bool done = false;
    const unsigned int nwv = (unsigned int)nthr >> 6;
    const unsigned int rounds = (keff + nwv - 1) / nwv;
    if (keff >= 1 && rounds <= 16) {
        uint64_t tm = 0;
        for_each_key([&](uint64_t key) { tm = key > tm ? key : tm; });
        uint32_t cur = (uint32_t)(tm >> 32), last = 0;
        for (unsigned int it = 0; it < rounds; ++it) {
            last = ivr_wave_max_u32(cur);
            if (cur == last) cur = 0;
        }
        if ((tid & 63) == 0) wlow[tid >> 6] = last;
        if (tid == 0) s_nsurv = 0;
        __syncthreads();
        uint32_t T = 0xFFFFFFFFu;
        for (unsigned int w = 0; w < nwv; ++w) T = min(T, wlow[w]);
        if (T != 0) {                              // 0: some wave ran out of keys - the fallback handles short lists
            const uint64_t T64 = (uint64_t)T << 32;
            for_each_key([&](uint64_t key) {
                if (key >= T64) {
                    const unsigned int slot = atomicAdd(&s_nsurv, 1u);
                    if (slot < (unsigned int)kSelThreads) surv[slot] = key;
                }
            });
        }
        __syncthreads();
        const unsigned int ns = s_nsurv;
        if (T != 0 && ns <= (unsigned int)nthr) {   // uniform: T and ns come from shared memory; ns >= keff by construction
            if ((unsigned int)tid < ns) {
                const uint64_t mine = surv[tid];
                unsigned int rank = 0;
                for (unsigned int j2 = 0; j2 < ns; ++j2) rank += surv[j2] > mine;
                if (rank < keff) sorted[rank] = mine;
            }
            done = true;
            __syncthreads();
        }
    }
    if (done) {
        // sorted[0 .. keff) is filled
    } else if (cached && keff <= 64) {
        // Small k (the reference asks for 10..50): extract the maximum keff times.  Per round: 16 register compares, a
        // wave max by shuffles, one LDS word per wave, two barriers - a few hundred cycles, against radix passes whose LDS
        // histogram atomics all collide on one bin when the scores share their leading bits.
        for (unsigned int it = 0; it < keff; ++it) {
            uint64_t m = 0;
#pragma unroll
            for (int j = 0; j < kRegKeys; ++j) m = kreg[j] > m ? kreg[j] : m;
            uint64_t wm = m;
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                const uint32_t hi = __shfl_xor((uint32_t)(wm >> 32), o, 64), lo = __shfl_xor((uint32_t)wm, o, 64);
                const uint64_t other = ((uint64_t)hi << 32) | lo;
                wm = other > wm ? other : wm;
            }
            if ((tid & 63) == 0) wmax[tid >> 6] = wm;
            __syncthreads();
            uint64_t gm = 0;
#pragma unroll
            for (int w = 0; w < kSelThreads / 64; ++w) gm = (w < (nthr >> 6) && wmax[w] > gm) ? wmax[w] : gm;
            if (tid == 0) sorted[it] = gm;
            if (m == gm) {                     // keys are unique: exactly one thread owns it
#pragma unroll
                for (int j = 0; j < kRegKeys; ++j)
                    if (kreg[j] == gm) kreg[j] = 0;
            }
            __syncthreads();
        }
    } else {
    uint64_t tau = ~0ull;   // nothing selected when keff == 0
    if (keff > 0) {
        if (tid == 0) {
            s_prefix = 0;
            s_mask = 0;
            s_kth = keff;
        }
        for (int pass = 0; pass < 8; ++pass) {
            const int shift = 56 - 8 * pass;
            if (tid < 256) hist[tid] = 0;
            __syncthreads();
            const unsigned long long prefix = s_prefix, mask = s_mask;
            for_each_key([&](uint64_t key) {
                if (key != 0 && (key & mask) == prefix) atomicAdd(&hist[(key >> shift) & 255], 1u);
            });
            __syncthreads();
            if (tid == 0) {
                unsigned int kth = s_kth, cum = 0;
                int dsel = 0;
                for (int dgt = 255; dgt >= 0; --dgt) {
                    const unsigned int h = hist[dgt];
                    if (cum + h >= kth) {
                        dsel = dgt;
                        break;
                    }
                    cum += h;
                }
                s_kth = kth - cum;
                s_prefix = prefix | ((unsigned long long)dsel << shift);
                s_mask = mask | (0xFFull << shift);
            }
            __syncthreads();
        }
        tau = s_prefix;   // the keff-th largest key (keys are unique)
    }
    // gather keys >= tau, pad, sort descending
    int P = 1;
    while (P < (int)keff) P <<= 1;
    if (tid == 0) s_cnt = 0;
    for (int i = tid; i < P; i += nthr) sorted[i] = 0;
    __syncthreads();
    if (keff > 0) {
        for_each_key([&](uint64_t key) {
            if (key != 0 && key >= tau) {
                const unsigned int slot = atomicAdd(&s_cnt, 1u);
                if (slot < (unsigned int)kMaxSort) sorted[slot] = key;
            }
        });
    }
    __syncthreads();
    for (int size = 2; size <= P; size <<= 1) {
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int i = tid; i < (P >> 1); i += nthr) {
                const int lo = ((i / stride) * stride * 2) + (i % stride);
                const int hi = lo + stride;
                const bool desc = ((lo & size) == 0);
                const uint64_t a = sorted[lo], b = sorted[hi];
                if ((a < b) == desc) {
                    sorted[lo] = b;
                    sorted[hi] = a;
                }
            }
            __syncthreads();
        }
    }
    }
    for (int j = tid; j < k; j += nthr) {
        const uint64_t key = j < (int)keff ? sorted[j] : 0;
        const uint32_t low = 0xFFFFFFFFu - (uint32_t)key;
        if (OUT == OUT_GROUPS) {
            out_groups[(int64_t)q * k + j] = key ? low : 0xFFFFFFFFu;
        } else {
            const int64_t qo = la.list ? la.list[q] : q;     // output row
            D[qo * k + j] = key ? ivr_ord2f((uint32_t)(key >> 32)) : -FLT_MAX;
            int64_t id = -1;
            if (key) {
                if (OUT == OUT_DI_PARTS) {
                    const int kk = ((const SrcParts *)&src)->k, nq = ((const SrcParts *)&src)->nq;
                    id = I_parts[((int64_t)(low / kk) * nq + q) * kk + (low % kk)];
                } else if (OUT == OUT_DI_PACKED) {
                    const int32_t *c = ((const SrcPacked *)&src)->at(q, low);
                    id = ((int64_t)c[2] << 32) | (uint32_t)c[1];
                } else if (OUT == OUT_DI_IDS || OUT == OUT_DI_IDS_POS) {
                    id = I_parts[low];
                } else {
                    id = id_base + (int64_t)low;
                }
            }
            I[qo * k + j] = id;
            if (OUT == OUT_DI_POS || OUT == OUT_DI_IDS_POS) reinterpret_cast<int64_t *>(out_groups)[qo * k + j] = key ? (int64_t)low : -1;
        }
    }
    if ((OUT == OUT_DI || OUT == OUT_DI_IDS || OUT == OUT_DI_POS || OUT == OUT_DI_IDS_POS) && vf.ok && tid == 0) {
        const uint32_t g = vf.sel[(int64_t)q * vf.ksel2 + vf.kp];
        int good = 1;
        if (g != 0xFFFFFFFFu) {                       // there IS an excluded group
            const float rmax = __uint_as_float(*vf.maxnorm_bits);
            float e;
            if (vf.qdelta) {
                const float qn = vf.qnorm[q], qd = vf.qdelta[q];
                e = 1.01f * ((qn + qd) * __uint_as_float(*vf.maxdelta_bits) + qd * rmax + vf.acc_eps * qn * rmax);
            } else {
                e = vf.rel_eps * vf.qnorm[q] * rmax;
            }
            const float bound = vf.gmax[(int64_t)q * vf.mstride + g] + e;
            const float kth = (int)keff >= k ? ivr_ord2f((uint32_t)(sorted[k - 1] >> 32)) : -FLT_MAX;
            good = bound < kth;                        // false for NaN / inf bounds too
        }
        vf.ok[q] = good;
        if (!good) {
            if (vf.fail_list) vf.fail_list[atomicAdd(vf.fail_count, 1)] = q;
            else atomicOr(&vf.tile_flag[q >> 4], 1);
        }
    }
}

int sel_threads(int64_t n) { return n <= 16 * 256 ? 256 : kSelThreads; }

// What a launch of the selection writes and what it does besides: only what a call site uses is set
struct SelectOut {
    uint32_t *groups = nullptr;           // OUT_GROUPS: [nq][k] selected groups
    float *D = nullptr;                   // OUT_DI*: [nq][k] scores and ids; id = id_base + row, or taken from the source's parts
    int64_t *I = nullptr;
    int64_t id_base = 0;
    const int64_t *ids = nullptr;         // OUT_DI_IDS: id = ids[row] (launch_select_rows picks the instantiation)
    const int64_t *I_parts = nullptr;     // OUT_DI_PARTS
    const int *skip = nullptr;            // queries with skip[q] != 0 keep what they have
    VerifyArgs vf;
    int *reset_flags = nullptr;           // tile flags [4] zeroed by this launch
    ListArgs la;
    int64_t *pos = nullptr;               // final selection of a search: [nq][k] rows of the view behind the slots (OUT_DI*_POS), or NULL
    static SelectOut to_groups(uint32_t *groups) {
        SelectOut o;
        o.groups = groups;
        return o;
    }
    static SelectOut to_rows(float *D, int64_t *I, int64_t id_base = 0, const int64_t *ids = nullptr) {
        SelectOut o;
        o.D = D;
        o.I = I;
        o.id_base = id_base;
        o.ids = ids;
        return o;
    }
};

// one workgroup per query; the block size follows the number of keys
template <int OUT, typename Src>
void launch_select(const Src &src, int nq, int k, const SelectOut &o, hipStream_t s) {
    constexpr bool kPos = OUT == OUT_DI_POS || OUT == OUT_DI_IDS_POS, kIds = OUT == OUT_DI_IDS || OUT == OUT_DI_IDS_POS;
    hipLaunchKernelGGL((select_topk_kernel<Src, OUT>), dim3(nq), dim3(sel_threads(src.n)), 0, s, src, 0, k, o.id_base,
                       kPos ? reinterpret_cast<uint32_t *>(o.pos) : o.groups, o.D, o.I, kIds ? o.ids : o.I_parts, o.skip, o.vf, o.reset_flags,
                       o.la);
}

// the final selection of a search (scores and labels of index rows): labels from the id table when the index has one
template <typename Src>
void launch_select_rows(const Src &src, int nq, int k, const SelectOut &o, hipStream_t s) {
    if (o.pos) {
        if (o.ids) launch_select<OUT_DI_IDS_POS>(src, nq, k, o, s);
        else launch_select<OUT_DI_POS>(src, nq, k, o, s);
    } else if (o.ids) launch_select<OUT_DI_IDS>(src, nq, k, o, s);
    else launch_select<OUT_DI>(src, nq, k, o, s);
}

}  // namespace
