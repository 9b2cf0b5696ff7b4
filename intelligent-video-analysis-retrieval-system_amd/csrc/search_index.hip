// The flat index object (ivr_index) and its storage: rows are kept in tiles of 16 rows, inside a tile in the order
// [d/4][16 rows][4 floats] (the MFMA operand layout that search.hip scans, see there), with a bf16 scan copy alongside.  Create /
// destroy / reset / add / add_with_ids / write / reconstruct / remove_ids, the tiling kernels (also used for the queries of a search) and the grow-only
// workspace buffers.
#include "ivr_common.h"
#include "search_internal.h"

namespace {

// ---------------------------------------------------------------------------------------------
// tiling: row-major [n,d] -> tiled, with optional L2 normalisation (N2/N3) and non-finite count
// ---------------------------------------------------------------------------------------------
// one wave per 16-row tile; lane l owns row (l & 15) and quad (l >> 4) of every 16-float chunk.
// Optionally also writes the bf16 scan copy of the tile (dst16; and the rounding remainder dst16lo for query tiles):
// per 32 floats of K one 1 KiB piece, lane l -> 16 bytes = the two quads this lane owns in the pair of 16-float chunks, i.e.
// the operand of one v_mfma_f32_16x16x32_bf16 with K permuted the same way for index rows and queries.
__global__ __launch_bounds__(256) void tile_rows_kernel(const float *__restrict__ src, float *__restrict__ dst,
                                                        int64_t row_start, int64_t n, int d, int dp4,
                                                        int normalize, int32_t *__restrict__ nonfinite,
                                                        const int64_t *__restrict__ start_dev, uint4 *__restrict__ dst16,
                                                        uint4 *__restrict__ dst16lo, unsigned int *__restrict__ maxnorm_bits,
                                                        float *__restrict__ rownorm, int zero_fill, int pstride,
                                                        unsigned int *__restrict__ maxdelta_bits, float *__restrict__ rowdelta) {
    if (start_dev) row_start = *start_dev;          // ring cursor kept in HBM so a captured graph can replay it
    const int lane = threadIdx.x & 63;
    const int64_t tile0 = row_start >> 4;
    const int64_t ntiles = ((row_start + n + 15) >> 4) - tile0;
    const int64_t t = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (t >= ntiles) return;
    const int64_t tile = tile0 + t;
    const int rr = lane & 15, qd = lane >> 4;
    const int64_t row = tile * 16 + rr;
    const bool valid = row >= row_start && row < row_start + n;
    const float *srow = src + (valid ? (row - row_start) : 0) * (int64_t)d;
    const bool vec = (d & 3) == 0 && ((reinterpret_cast<uintptr_t>(src) & 15) == 0);
    const int kchunks = dp4 >> 2;
    float ss = 0.f;
    int bad = 0;
    if (normalize || nonfinite || maxnorm_bits || rownorm) {
        // eight chunks per trip, all loads issued before the first use: a query batch is a handful of rows, so this kernel is
        // a latency chain (32 dependent trips of ~0.4 us at d = 512 before); the sum keeps its ascending-k order
        for (int kc0 = 0; kc0 < kchunks; kc0 += 8) {
            float4 v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int k0 = (kc0 + u) * 16 + qd * 4;
                v[u] = make_float4(0.f, 0.f, 0.f, 0.f);
                if (valid && kc0 + u < kchunks && k0 < d) v[u] = ivr_load_quad(srow, k0, d, vec && k0 + 3 < d);
            }
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                ss = fmaf(v[u].x, v[u].x, ss);
                ss = fmaf(v[u].y, v[u].y, ss);
                ss = fmaf(v[u].z, v[u].z, ss);
                ss = fmaf(v[u].w, v[u].w, ss);
                bad += !isfinite(v[u].x) + !isfinite(v[u].y) + !isfinite(v[u].z) + !isfinite(v[u].w);
            }
        }
        ss += __shfl_xor(ss, 16, 64);
        ss += __shfl_xor(ss, 32, 64);
        if (nonfinite) {
            bad += __shfl_xor(bad, 16, 64);
            bad += __shfl_xor(bad, 32, 64);
            if (bad && qd == 0) atomicAdd(nonfinite, bad);
        }
    }
    // core.py:1194-1196: norms[norms == 0] = 1; features / norms
    const float nrm = normalize ? (ss > 0.f ? sqrtf(ss) : 1.f) : 1.f;
    if (maxnorm_bits) {
        // largest stored row norm (an upper bound: overwritten rows keep counting), for the error bound of the bf16 scan;
        // a normalised row is 1 up to rounding, the 1e-6 covers it.  Positive floats order like their bit patterns.
        float stored = valid ? (normalize ? (ss > 0.f ? 1.000001f : 0.f) : sqrtf(ss)) : 0.f;
        if (!(stored == stored)) stored = INFINITY;      // NaN rows: no bound -> the verification always fails over to the exact path
#pragma unroll
        for (int o = 1; o < 16; o <<= 1) stored = fmaxf(stored, __shfl_xor(stored, o, 64));
        const unsigned int bits = __float_as_uint(stored);
        if (lane == 0 && bits > *maxnorm_bits) atomicMax(maxnorm_bits, bits);
    }
    // query tiles: an upper bound of the stored row's norm for the error bound of the bf16 candidate scan (1 up to rounding once
    // normalised, as for the index rows above)
    if (rownorm && valid && qd == 0) rownorm[row - row_start] = normalize ? (ss > 0.f ? 1.000001f : 0.f) : sqrtf(ss);
    float4 *out = reinterpret_cast<float4 *>(dst) + tile * (int64_t)dp4 * 16 + lane;
    const int pieces = (kchunks + 1) >> 1;          // pieces that carry data; the tile's stride is pstride (even, see ivr_index_create)
    const bool store = valid || zero_fill;          // query tiles: the padding rows of the last tile are written as zeros
    float sd = 0.f;                                 // squared norm of this lane's part of  row - bf16(row)
    for (int kb0 = 0; kb0 < pieces; kb0 += 4) {
      float4 vv[4][2];
#pragma unroll
      for (int b4 = 0; b4 < 4; ++b4)
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int kc = 2 * (kb0 + b4) + u, k0 = kc * 16 + qd * 4;
            vv[b4][u] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (valid && kc < kchunks && k0 < d) vv[b4][u] = ivr_load_quad(srow, k0, d, vec && k0 + 3 < d);
        }
#pragma unroll
      for (int b4 = 0; b4 < 4; ++b4) {
        const int kb = kb0 + b4;
        if (kb >= pieces) break;
        float4 (&v)[2] = vv[b4];
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int kc = 2 * kb + u;
            if (store && kc < kchunks) {
                if (valid && normalize) {
                    v[u].x /= nrm;
                    v[u].y /= nrm;
                    v[u].z /= nrm;
                    v[u].w /= nrm;
                }
                out[kc * 64] = v[u];
            }
        }
        if (dst16 && store) {
            uint4 hi;
            hi.x = ivr_pack_bf16x2(v[0].x, v[0].y);
            hi.y = ivr_pack_bf16x2(v[0].z, v[0].w);
            hi.z = ivr_pack_bf16x2(v[1].x, v[1].y);
            hi.w = ivr_pack_bf16x2(v[1].z, v[1].w);
            dst16[(tile * pstride + kb) * 64 + lane] = hi;
            // what rounding to bf16 dropped: exact in float32 (the difference of a float and its own leading bits)
            auto lo2 = [&sd](uint32_t h, float a, float b) {
                const float ra = a - __uint_as_float(h << 16), rb = b - __uint_as_float(h & 0xffff0000u);
                sd = fmaf(ra, ra, sd);
                sd = fmaf(rb, rb, sd);
                return ivr_pack_bf16x2(ra, rb);
            };
            uint4 lo;
            lo.x = lo2(hi.x, v[0].x, v[0].y);
            lo.y = lo2(hi.y, v[0].z, v[0].w);
            lo.z = lo2(hi.z, v[1].x, v[1].y);
            lo.w = lo2(hi.w, v[1].z, v[1].w);
            if (dst16lo) dst16lo[(tile * pstride + kb) * 64 + lane] = lo;
        }
      }
    }
    // |row - bf16(row)| per stored row, for the error bound of the large-batch candidate scan (both operands rounded to nearest):
    // the largest over the index rows, one value per query
    if (dst16 && (maxdelta_bits || rowdelta)) {
        sd += __shfl_xor(sd, 16, 64);
        sd += __shfl_xor(sd, 32, 64);
        float dl = valid ? sqrtf(sd) * 1.0001f : 0.f;
        if (!(dl == dl)) dl = INFINITY;             // NaN rows: no bound, every verification fails over to the exact path
        if (rowdelta && valid && qd == 0) rowdelta[row - row_start] = dl;
        if (maxdelta_bits) {
#pragma unroll
            for (int o = 1; o < 16; o <<= 1) dl = fmaxf(dl, __shfl_xor(dl, o, 64));
            const unsigned int bits = __float_as_uint(dl);
            if (lane == 0 && bits > *maxdelta_bits) atomicMax(maxdelta_bits, bits);
        }
    }
}

__global__ __launch_bounds__(256) void untile_rows_kernel(const float *__restrict__ src, float *__restrict__ dst,
                                                          int64_t row_start, int64_t n, int d, int dp4) {
    const int lane = threadIdx.x & 63;
    const int64_t tile0 = row_start >> 4;
    const int64_t ntiles = ((row_start + n + 15) >> 4) - tile0;
    const int64_t t = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (t >= ntiles) return;
    const int64_t tile = tile0 + t;
    const int rr = lane & 15, qd = lane >> 4;
    const int64_t row = tile * 16 + rr;
    if (row < row_start || row >= row_start + n) return;
    const float4 *in = reinterpret_cast<const float4 *>(src) + tile * (int64_t)dp4 * 16 + lane;
    float *drow = dst + (row - row_start) * (int64_t)d;
    for (int kc = 0; kc < (dp4 >> 2); ++kc) {
        const int k0 = kc * 16 + qd * 4;
        const float4 v = in[kc * 64];
        if (k0 + 0 < d) drow[k0 + 0] = v.x;
        if (k0 + 1 < d) drow[k0 + 1] = v.y;
        if (k0 + 2 < d) drow[k0 + 2] = v.z;
        if (k0 + 3 < d) drow[k0 + 3] = v.w;
    }
}

__global__ void advance_cursor_kernel(int64_t *cursor, int64_t n, int64_t modulo) { *cursor = (*cursor + n) % modulo; }

// in-place row normalisation of a row-major matrix (ivr_l2_normalize): one wave per row
__global__ __launch_bounds__(256) void l2_normalize_kernel(float *__restrict__ x, int64_t n, int d,
                                                           int32_t *__restrict__ nonfinite) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= n) return;
    float *p = x + row * (int64_t)d;
    float ss = 0.f;
    int bad = 0;
    for (int k = lane; k < d; k += 64) {
        const float v = p[k];
        ss = fmaf(v, v, ss);
        bad += !isfinite(v);
    }
    ss = ivr_wave_sum(ss);
    if (nonfinite) {
        for (int o = 32; o > 0; o >>= 1) bad += __shfl_xor(bad, o, 64);
        if (bad && lane == 0) atomicAdd(nonfinite, bad);
    }
    const float nrm = ss > 0.f ? sqrtf(ss) : 1.f;
    for (int k = lane; k < d; k += 64) p[k] = p[k] / nrm;
}

// ---------------------------------------------------------------------------------------------
// row removal (ivr_index_remove_ids): order-preserving in-place compaction of both tiled layouts
// ---------------------------------------------------------------------------------------------
// The tail is the part of the index from the 256-row block of the first allowed row on; every row number below is relative to its
// first row.  Kept row number q of the tail (in row order) moves to row q.  Three passes give every 64-row group its kept rows as a
// word and the number of kept rows in front of it, a fourth copies that number at every unit boundary to the host.  The host then
// walks the tail in steps of whole units of source rows, in ascending order.  A step whose destination rows all lie below its
// first source row is one launch: gather its survivors straight into their destination tiles.  Any other step is two stream-ordered
// launches: gather the survivors into the bounce buffer in the tile layout of their destination, place the bounce into the index.
// Either way a step writes only rows below the end of its own source rows (destinations never lie above their sources), a launch
// that writes the index reads none of the rows it writes, and later steps read only rows at or above that end: no launch overwrites
// a row that another workgroup has yet to read ("row removal").
constexpr int kScanBlock = 1024;     // groups per block of the kept-row prefix

struct RemovePlan {
    uint64_t *word;      // [ngroups + 1] bit i = row 64 g + i is stored and stays
    uint32_t *kept;      // [ngroups + 1] kept rows of group g, then the kept rows in front of it inside its block of kScanBlock groups
    uint32_t *top;       // [blocks] kept rows of each block, then their exclusive prefix
    uint32_t *state;     // [0] first removed row (0xffffffff: none), [1] kept rows of the tail, [2 + i] kept rows in front of unit i
    int64_t nrows;       // rows of the tail
    int64_t ngroups;     // ceil(nrows / 64); entry ngroups is an empty group, so the prefix in front of it is the total
};

__device__ __forceinline__ uint64_t stored_word(const RemovePlan &p, int64_t g) {
    const int64_t left = p.nrows - g * 64;
    return left >= 64 ? ~0ull : left <= 0 ? 0ull : (1ull << left) - 1;
}
// kept rows in front of group g (g <= ngroups), once the three passes have run
__device__ __forceinline__ uint32_t kept_before(const RemovePlan &p, int64_t g) { return p.top[g / kScanBlock] + p.kept[g]; }

// exclusive prefix sum over the 256 threads of a block, and the block's total; wsum: LDS [4]
__device__ __forceinline__ uint32_t block_scan_excl(uint32_t v, uint32_t *wsum, uint32_t &total) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const uint32_t inc = ivr_wave_incl_scan(v, lane);
    if (lane == 63) wsum[w] = inc;
    __syncthreads();
    uint32_t base = 0;
    total = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        if (i < w) base += wsum[i];
        total += wsum[i];
    }
    __syncthreads();                                // wsum may be written again
    return base + inc - v;
}

// pass 1: one wave per 64-row group; the filter allows = removes
__global__ __launch_bounds__(256) void remove_count_kernel(RemovePlan p, RowMask m) {
    const int64_t g = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (g > p.ngroups) return;
    const uint64_t allowed = row_mask_word(m, g * 64, row_mask_fetch(m, g * 64));
    const uint64_t keep = stored_word(p, g) & ~allowed;
    if ((threadIdx.x & 63) == 0) {
        p.word[g] = keep;
        p.kept[g] = (uint32_t)__popcll(keep);
    }
}

// pass 2: one block per kScanBlock groups: the counts become prefixes inside the block, the block's total goes to top; the first
// removed row of the tail by one atomic per block
__global__ __launch_bounds__(256) void remove_scan_kernel(RemovePlan p) {
    __shared__ uint32_t wsum[4];
    __shared__ uint32_t first;
    if (threadIdx.x == 0) first = 0xffffffffu;
    __syncthreads();
    const int64_t e0 = (int64_t)blockIdx.x * kScanBlock + threadIdx.x * 4;
    uint32_t c[4], sum = 0, fr = 0xffffffffu;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int64_t e = e0 + u;
        c[u] = e <= p.ngroups ? p.kept[e] : 0u;
        sum += c[u];
        if (e < p.ngroups) {
            const uint64_t removed = stored_word(p, e) & ~p.word[e];
            if (removed && fr == 0xffffffffu) fr = (uint32_t)(e * 64 + __builtin_ctzll(removed));
        }
    }
    if (fr != 0xffffffffu) atomicMin(&first, fr);
    uint32_t total;
    uint32_t ex = block_scan_excl(sum, wsum, total);        // its barriers also order the atomics on `first`
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        if (e0 + u <= p.ngroups) p.kept[e0 + u] = ex;
        ex += c[u];
    }
    if (threadIdx.x == 0) {
        p.top[blockIdx.x] = total;
        if (first != 0xffffffffu) atomicMin(&p.state[0], first);
    }
}

// pass 3: one block: exclusive prefix of the block totals, and the kept rows of the tail
__global__ __launch_bounds__(256) void remove_scan_top_kernel(RemovePlan p, int64_t nblocks) {
    __shared__ uint32_t wsum[4];
    uint32_t carry = 0;
    for (int64_t b0 = 0; b0 < nblocks; b0 += 256) {
        const int64_t b = b0 + threadIdx.x;
        const uint32_t v = b < nblocks ? p.top[b] : 0u;
        uint32_t total;
        const uint32_t ex = block_scan_excl(v, wsum, total);
        if (b < nblocks) p.top[b] = carry + ex;
        carry += total;
    }
    if (threadIdx.x == 0) p.state[1] = carry;
}

// pass 4: the kept rows in front of every unit of `unit` groups (and in front of the end of the tail), for the host's plan
__global__ __launch_bounds__(256) void remove_bounds_kernel(RemovePlan p, int64_t unit, int64_t nunits) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i <= nunits) p.state[2 + i] = kept_before(p, min(i * unit, p.ngroups));
}

// One step of the walk: the source groups [ga, gb).  Its survivors go to the rows [dst_a, dst_b) = the kept rows in front of ga
// and gb, clipped below to the first removed row (rows in front of it stay where they are).  With the bounce buffer, bounce tile j
// holds destination tile (dst_a >> 4) + j with the rows in their destination slots; slots outside [dst_a, dst_b) are neither
// written nor read.  direct: the gather writes those slots of the destination tiles themselves (dst_b <= the step's first source row).
struct RemoveMove {
    float4 *data;        // the tail's float32 tiles
    uint4 *data16;       // its bf16 scan copy, or NULL
    float4 *bounce;
    uint4 *bounce16;
    int kchunks;         // 16-float chunks of a row = float4 per lane and tile
    int pieces;          // bf16 pieces that carry data
    int pstride;         // bf16 pieces per tile
    int64_t ga, gb;
    uint32_t dst_a, dst_b;
    int direct;
};

// the i-th set bit of w (i < popcount(w))
__device__ __forceinline__ int select_bit(uint64_t w, uint32_t i) {
    int pos = 0;
#pragma unroll
    for (int width = 32; width >= 1; width >>= 1) {
        const uint64_t low = w & ((1ull << width) - 1);
        const uint32_t c = (uint32_t)__popcll(low);
        if (i >= c) {
            i -= c;
            pos += width;
            w >>= width;
        } else {
            w = low;
        }
    }
    return pos;
}

// this wave's destination tile and whether this lane's slot of it belongs to the chunk; false for every lane: nothing to do
__device__ __forceinline__ bool remove_slot(const RemoveMove &mv, int64_t &j, int64_t &tile, uint32_t &row) {
    j = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    tile = (int64_t)(mv.dst_a >> 4) + j;
    row = (uint32_t)(tile * 16 + (threadIdx.x & 15));
    return tile * 16 < (int64_t)mv.dst_b && row >= mv.dst_a && row < mv.dst_b;
}

// copy this lane's 16 bytes of every chunk of one tile (float32: kchunks float4, bf16: pieces uint4), kCopyInFlight loads in flight
constexpr int kCopyInFlight = 8;
template <typename T>
__device__ __forceinline__ void copy_lane(const T *__restrict__ in, T *__restrict__ out, int n) {
    for (int k0 = 0; k0 < n; k0 += kCopyInFlight) {
        T v[kCopyInFlight];
#pragma unroll
        for (int u = 0; u < kCopyInFlight; ++u)
            if (k0 + u < n) v[u] = in[(k0 + u) * 64];
#pragma unroll
        for (int u = 0; u < kCopyInFlight; ++u)
            if (k0 + u < n) out[(k0 + u) * 64] = v[u];
    }
}

// one wave per destination tile: lane l fetches the 16 bytes per chunk that row slot (l & 15), quad (l >> 4) of the tile will hold
__global__ __launch_bounds__(256) void remove_gather_kernel(RemovePlan p, RemoveMove mv) {
    int64_t j, tile;
    uint32_t row;
    const bool valid = remove_slot(mv, j, tile, row);
    if (!__any(valid)) return;
    const int lane = threadIdx.x & 63;
    uint32_t src = 0;
    if (valid && lane < 16) {
        // the last group of the chunk with at most `row` kept rows in front of it holds kept row number `row`
        int64_t lo = mv.ga, hi = mv.gb - 1;
        while (lo < hi) {
            const int64_t mid = (lo + hi + 1) >> 1;
            if (kept_before(p, mid) <= row) lo = mid;
            else hi = mid - 1;
        }
        src = (uint32_t)(lo * 64 + select_bit(p.word[lo], row - kept_before(p, lo)));
    }
    src = __shfl(src, lane & 15, 64);
    if (!valid) return;
    const int64_t stile = src >> 4;
    const int slot = (int)(src & 15) + (lane & 48);
    float4 *out = mv.direct ? mv.data + tile * mv.kchunks * 64 : mv.bounce + j * mv.kchunks * 64;
    copy_lane(mv.data + stile * mv.kchunks * 64 + slot, out + lane, mv.kchunks);
    if (mv.data16) {
        uint4 *out16 = mv.direct ? mv.data16 + tile * mv.pstride * 64 : mv.bounce16 + j * mv.pstride * 64;
        copy_lane(mv.data16 + stile * mv.pstride * 64 + slot, out16 + lane, mv.pieces);
    }
}

// one wave per destination tile: the chunk's slots of the tile from the bounce buffer, the other slots untouched
__global__ __launch_bounds__(256) void remove_place_kernel(RemoveMove mv) {
    int64_t j, tile;
    uint32_t row;
    if (!remove_slot(mv, j, tile, row)) return;
    const int lane = threadIdx.x & 63;
    copy_lane(mv.bounce + j * mv.kchunks * 64 + lane, mv.data + tile * mv.kchunks * 64 + lane, mv.kchunks);
    if (mv.data16) copy_lane(mv.bounce16 + j * mv.pstride * 64 + lane, mv.data16 + tile * mv.pstride * 64 + lane, mv.pieces);
}

// Id table of an id-mapped index: the ids of the kept rows from the first removed row on, in row order, out of place into `moved`
// (kept row number q >= first goes to moved[q - first]; an in-place pass would overwrite ids that other workgroups have yet to
// read).  One thread per row from the group of the first removed row on; the host copies moved back to ids[first ..).
__global__ __launch_bounds__(256) void remove_ids_gather_kernel(RemovePlan p, const int64_t *__restrict__ ids, int64_t *__restrict__ moved,
                                                                uint32_t first) {
    const int64_t r = (int64_t)(first / kGroupRows) * kGroupRows + (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= p.nrows) return;
    const int64_t g = r / kGroupRows;
    const int i = (int)(r % kGroupRows);
    const uint64_t w = p.word[g];
    if (!((w >> i) & 1ull)) return;
    const uint32_t dst = kept_before(p, g) + (uint32_t)__popcll(w & ((1ull << i) - 1));
    if (dst >= first) moved[dst - first] = ids[r];
}

// the slots slot0 .. 15 of one tile zero in both layouts: one wave
__global__ __launch_bounds__(64) void zero_slots_kernel(float4 *tile, uint4 *tile16, int slot0, int kchunks, int pstride) {
    const int lane = threadIdx.x;
    if ((lane & 15) < slot0) return;
    for (int k = 0; k < kchunks; ++k) tile[k * 64 + lane] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (tile16)
        for (int k = 0; k < pstride; ++k) tile16[k * 64 + lane] = make_uint4(0u, 0u, 0u, 0u);
}

int64_t tile_bytes(const ivr_index *x, int64_t rows) { return rows * (int64_t)x->dp * 4; }

int64_t tile16_bytes(const ivr_index *x, int64_t rows) { return (rows / 16) * (int64_t)x->pieces * 1024; }

int index_alloc(ivr_index *x, int64_t rows) {
    rows = ivr_round_up(std::max<int64_t>(rows, kGroupRows), kGroupRows);
    float *nd = nullptr;
    IVR_HIP(hipMalloc(&nd, (size_t)tile_bytes(x, rows)));
    IVR_HIP(hipMemset(nd, 0, (size_t)tile_bytes(x, rows)));
    uint4 *nd16 = nullptr;
    if (x->scan16) {
        // padded to whole 256-row blocks: the large-batch scan streams blocks (rows past ntotal are masked, never out of bounds)
        IVR_HIP(hipMalloc(&nd16, (size_t)tile16_bytes(x, ivr_round_up(rows, 256))));
        IVR_HIP(hipMemset(nd16, 0, (size_t)tile16_bytes(x, ivr_round_up(rows, 256))));
    }
    int64_t *nids = nullptr;
    if (x->has_ids) {
        IVR_HIP(hipMalloc(&nids, (size_t)rows * sizeof(int64_t)));
        if (x->ids && x->ntotal > 0) IVR_HIP(hipMemcpy(nids, x->ids, (size_t)x->ntotal * sizeof(int64_t), hipMemcpyDeviceToDevice));
    }
    if (x->ids) IVR_HIP(hipFree(x->ids));
    x->ids = nids;
    if (x->data) {
        if (x->ntotal > 0) {
            IVR_HIP(hipMemcpy(nd, x->data, (size_t)tile_bytes(x, ivr_round_up(x->ntotal, 16)), hipMemcpyDeviceToDevice));
            if (x->scan16)
                IVR_HIP(hipMemcpy(nd16, x->data16, (size_t)tile16_bytes(x, ivr_round_up(x->ntotal, 16)), hipMemcpyDeviceToDevice));
        }
        IVR_HIP(hipFree(x->data));
        if (x->data16) IVR_HIP(hipFree(x->data16));
    }
    x->data = nd;
    x->data16 = nd16;
    x->cap = rows;
    return IVR_OK;
}

int allocate_all(DevSizes bufs, bool zero) {
    for (const auto &b : bufs) {
        if (b.second == 0) continue;
        IVR_HIP(hipMalloc(&b.first->ptr, b.second));
        b.first->bytes = b.second;
        if (zero) IVR_HIP(hipMemset(b.first->ptr, 0, b.second));
    }
    return IVR_OK;
}

// ivr_index_add (ids == NULL) and ivr_index_add_with_ids: the mode check, growth, the tiling launch and, with ids, one device-to-device
// copy of the labels behind the table's stored part
int index_append(ivr_index *x, const float *rows, const int64_t *ids, int64_t n, int normalize, hipStream_t s, const char *what) {
    IVR_REQUIRE(x && (rows || n == 0), "%s: NULL argument", what);
    IVR_REQUIRE(n >= 0, "%s: n=%lld", what, (long long)n);
    std::lock_guard<std::mutex> lk(x->mu);
    if (ids && !x->has_ids && x->ntotal > 0)
        return ivr_fail(IVR_ERR_STATE, "%s: the index holds %lld rows without ids (ids are chosen while it is empty, or after ivr_index_reset)",
                        what, (long long)x->ntotal);
    if (!ids && x->has_ids)
        return ivr_fail(IVR_ERR_STATE, "%s: the index is id-mapped: add rows with ivr_index_add_with_ids (or ivr_index_reset first)", what);
    IVR_HIP(hipSetDevice(x->ctx->device));
    const bool first_ids = ids && !x->has_ids;
    if (x->ntotal + n > x->cap || first_ids) {
        IVR_REQUIRE(x->ntotal + n < (1ll << 32) - 64, "%s: index would exceed 2^32 rows", what);
        // growing re-allocates: wait for work that may still read the old buffer
        IVR_HIP(hipDeviceSynchronize());
        if (x->ntotal + n > x->cap) {
            x->has_ids = ids != nullptr;
            int rc = index_alloc(x, std::max<int64_t>(x->ntotal + n, x->cap + x->cap / 2));
            if (rc != IVR_OK) {
                if (first_ids) x->has_ids = false;
                return rc;
            }
        } else {                                 // an empty index becomes id-mapped inside its capacity: the table alone
            IVR_HIP(hipMalloc(&x->ids, (size_t)x->cap * sizeof(int64_t)));
            x->has_ids = true;
        }
    }
    int rc = ivr_launch_tile_rows(x, x->data, rows, x->ntotal, n, normalize, nullptr, s);
    if (rc != IVR_OK) return rc;
    if (ids && n > 0) IVR_HIP(hipMemcpyAsync(x->ids + x->ntotal, ids, (size_t)n * sizeof(int64_t), hipMemcpyDeviceToDevice, s));
    if (ids) x->tab_ok = false;                  // the lookup table of ivr_index_find_ids is rebuilt by its next lookup
    x->ntotal += n;
    return IVR_OK;
}

}  // namespace

int ivr_release(DevSizes bufs) {
    hipError_t first = hipSuccess;
    for (const auto &b : bufs) {
        const hipError_t e = b.first->ptr ? hipFree(b.first->ptr) : hipSuccess;
        if (first == hipSuccess) first = e;
        b.first->ptr = nullptr;
        b.first->bytes = 0;
    }
    IVR_HIP(first);
    return IVR_OK;
}

int ivr_reserve(DevSizes bufs, bool zero) {
    bool enough = true;
    for (const auto &b : bufs) enough = enough && b.second <= b.first->bytes;
    if (enough) return IVR_OK;
    int rc = ivr_release(bufs);
    if (rc == IVR_OK) rc = allocate_all(bufs, zero);
    // all or nothing: after a failed allocation no buffer of the group is left behind, so the next call starts over and reports the
    // error again instead of finding some buffers present and launching on the missing ones
    if (rc != IVR_OK) (void)ivr_release(bufs);
    return rc;
}

View ivr_make_view(const ivr_index *x, int64_t id_base, const ivr_id_filter *f, RowMask &m) {
    if (!f) return View{x->data, x->data16, x->ntotal, ivr_ceil_div(x->ntotal, kGroupRows), id_base, nullptr, nullptr};
    __int128 lo = f->lo, hi = f->hi;
    if (f->bits) {                              // ids the bitmap covers: [0, nbits)
        lo = std::max<__int128>(lo, 0);
        hi = std::min<__int128>(hi, f->nbits);
    }
    const __int128 rlo = std::max<__int128>(lo - id_base, 0), rhi = std::min<__int128>(hi - id_base, x->ntotal);
    if (rlo >= rhi) return View{x->data, x->data16, 0, 0, id_base, &m, nullptr};
    const int64_t b0 = (int64_t)rlo / 256 * 256, n = (int64_t)rhi - b0;
    m.lo = (int64_t)rlo - b0;
    m.hi = n;
    m.bits = f->bits;
    m.bit0 = id_base + b0;
    return View{x->data + b0 * x->dp, x->data16 ? x->data16 + (b0 / 16) * x->pieces * 64 : nullptr, n, ivr_ceil_div(n, kGroupRows),
                id_base + b0, &m, nullptr};
}

int ivr_launch_tile_rows(ivr_index *x, float *dst, const float *src, int64_t start, int64_t n, int normalize, int32_t *nonfinite,
                         hipStream_t s, const int64_t *start_dev, int64_t max_tiles) {
    if (n <= 0) return IVR_OK;
    const int64_t ntiles = max_tiles ? max_tiles : ((start + n + 15) >> 4) - (start >> 4);
    const unsigned grid = (unsigned)ivr_ceil_div(ntiles, 4);
    const bool rows = dst == x->data, queries = dst == x->qtiled;
    const bool scan16 = x->scan16 && (rows || queries);      // any other destination (the label tiles of tags.hip): float32 tiles alone
    IvrProf prof("tile_rows", s, (double)n * (x->d + x->dp) * 4 + (scan16 ? (double)n * x->pieces * 64 * (rows ? 1 : 2) : 0.0), true);
    // query tiles: the padding rows of the last tile are zero-filled by the kernel itself (no memset in front of it)
    hipLaunchKernelGGL(tile_rows_kernel, dim3(grid), dim3(256), 0, s, src, dst, start, n, x->d, x->dp4, normalize, nonfinite, start_dev,
                       scan16 ? (rows ? x->data16 : x->q16hi) : (uint4 *)nullptr, scan16 && !rows ? x->q16lo : (uint4 *)nullptr,
                       scan16 && rows ? x->maxnorm : (unsigned int *)nullptr, queries ? x->qnorm : (float *)nullptr, rows ? 0 : 1,
                       x->pieces, scan16 && rows ? x->maxdelta : (unsigned int *)nullptr,
                       scan16 && queries ? x->qdelta : (float *)nullptr);
    IVR_LAUNCH_CHECK();
    return IVR_OK;
}

extern "C" {

int ivr_index_create(ivr_ctx *ctx, int d, int64_t capacity_rows, ivr_index **out) {
    IVR_REQUIRE(ctx && out, "ivr_index_create: NULL argument");
    IVR_REQUIRE(d >= 1 && d <= 2048, "ivr_index_create: d=%d out of range [1,2048]", d);
    IVR_REQUIRE(capacity_rows >= 0 && capacity_rows < (1ll << 32) - 64, "ivr_index_create: capacity %lld out of range",
                (long long)capacity_rows);
    IVR_HIP(hipSetDevice(ctx->device));
    ivr_index *x = new ivr_index();
    x->ctx = ctx;
    x->d = d;
    x->dp = (int)ivr_round_up(d, 16);
    x->dp4 = x->dp / 4;
    x->pieces = (x->dp + 31) / 32;
    {
        const char *e = getenv("IVR_SCAN_BF16");       // A/B switch, read when the index is created
        x->scan16 = !(e && e[0] == '0');   // LDS per 16-query tile (hi + lo) = 64 dp bytes, the same as the float32 scan's
        const char *b = getenv("IVR_SCAN_BIGQ");
        x->bigq = !(b && b[0] == '0');
        const char *pr = getenv("IVR_SCAN_PRUNE");
        x->prune = !(pr && pr[0] == '0');
        const char *rg = getenv("IVR_SCAN_RING");
        x->ring = !(rg && rg[0] == '0');
        // source rows per chunk of ivr_index_remove_ids' walk = the size of its bounce buffer; whole groups, at most 2^22 rows
        const char *rc = getenv("IVR_REMOVE_CHUNK_ROWS");
        const long long rows = rc ? atoll(rc) : 0;
        if (rows > 0) x->remove_chunk = ivr_round_up(std::min<long long>(rows, 1ll << 22), kGroupRows);
        // ivr_index_search_sequences: key slots per chunk of target windows (one window's stretch at least), at most 2^30
        const char *sq = getenv("IVR_SEQ_CHUNK_SLOTS");
        const long long slots = sq ? atoll(sq) : 0;
        if (slots > 0) x->seq_chunk_slots = std::min<long long>(slots, 1ll << 30);
        // ivr_index_search_lists: key slots per chunk of queries (one query's stretch at least; tests force several chunks)
        x->ivf.chunk_slots = ivr_env_positive("IVR_IVF_CHUNK_SLOTS", kIvfChunkSlots);
        // ivr_index_find_ids: lookups of at least this many keys go through the hash table (0: always, a huge value: never)
        const char *ft = getenv("IVR_FIND_TABLE_MIN_KEYS");
        x->find_table_min = ft && ft[0] ? std::max<long long>(0, atoll(ft)) : kFindTableMinKeys;
    }
    // an even number of pieces per tile: the large-batch scan steps K by two pieces; an odd tail piece stays all zero on both sides
    x->pieces = (int)ivr_round_up(x->pieces, 2);
    int rc = IVR_OK;
    if (x->scan16) rc = ivr_reserve({{&x->maxnorm, 4}, {&x->okflag, 68 * sizeof(int)}, {&x->maxdelta, 4}}, true);
    if (rc == IVR_OK) rc = index_alloc(x, capacity_rows);
    if (rc != IVR_OK) {
        delete x;
        return rc;
    }
    *out = x;
    return IVR_OK;
}

int ivr_index_destroy(ivr_index *x) {
    if (!x) return IVR_OK;
    if (x->data) (void)hipFree(x->data);
    if (x->data16) (void)hipFree(x->data16);
    if (x->ids) (void)hipFree(x->ids);
    delete x;                        // the workspace buffers free themselves
    return IVR_OK;
}

int ivr_index_reset(ivr_index *x) {
    IVR_REQUIRE(x, "ivr_index_reset: NULL index");
    std::lock_guard<std::mutex> lk(x->mu);
    IVR_HIP(hipSetDevice(x->ctx->device));
    IVR_HIP(hipMemset(x->data, 0, (size_t)tile_bytes(x, x->cap)));
    if (x->scan16) {
        IVR_HIP(hipMemset(x->data16, 0, (size_t)tile16_bytes(x, ivr_round_up(x->cap, 256))));
        IVR_HIP(hipMemset(x->maxnorm, 0, 4));
        IVR_HIP(hipMemset(x->maxdelta, 0, 4));
    }
    x->ntotal = 0;
    // the mode is undecided again: the next ivr_index_add makes a plain index, the next ivr_index_add_with_ids an id-mapped one
    x->has_ids = false;
    x->tab_ok = false;
    x->tab_slots = 0;
    if (x->ids) {
        int64_t *old = x->ids;
        x->ids = nullptr;
        IVR_HIP(hipDeviceSynchronize());         // work that may still read the table
        IVR_HIP(hipFree(old));
        return ivr_release({{&x->tab_keys, 0}, {&x->tab_rows, 0}});      // the lookup table goes with the ids
    }
    return IVR_OK;
}

int64_t ivr_index_ntotal(ivr_index *x) { return x ? x->ntotal : 0; }
int ivr_index_dim(ivr_index *x) { return x ? x->d : 0; }
int64_t ivr_index_capacity(ivr_index *x) { return x ? x->cap : 0; }

int ivr_index_add(ivr_index *x, const float *rows, int64_t n, int normalize, ivr_stream stream) {
    return index_append(x, rows, nullptr, n, normalize, (hipStream_t)stream, "ivr_index_add");
}

int ivr_index_add_with_ids(ivr_index *x, const float *rows, const int64_t *ids, int64_t n, int normalize, ivr_stream stream) {
    IVR_REQUIRE(ids || n == 0, "ivr_index_add_with_ids: NULL ids");
    static const int64_t none = 0;               // n == 0 still decides the mode of an empty index
    return index_append(x, rows, ids ? ids : &none, n, normalize, (hipStream_t)stream, "ivr_index_add_with_ids");
}

int ivr_index_write(ivr_index *x, int64_t start, const float *rows, int64_t n, int normalize, ivr_stream stream) {
    IVR_REQUIRE(x && (rows || n == 0), "ivr_index_write: NULL argument");
    std::lock_guard<std::mutex> lk(x->mu);
    IVR_REQUIRE(start >= 0 && n >= 0 && start + n <= x->ntotal, "ivr_index_write: rows [%lld,%lld) outside [0,%lld)",
                (long long)start, (long long)(start + n), (long long)x->ntotal);
    IVR_HIP(hipSetDevice(x->ctx->device));
    return ivr_launch_tile_rows(x, x->data, rows, start, n, normalize, nullptr, (hipStream_t)stream);
}

int ivr_index_write_ring(ivr_index *x, const float *rows, int64_t n, int normalize, int64_t *cursor, ivr_stream stream) {
    IVR_REQUIRE(x && rows && cursor, "ivr_index_write_ring: NULL argument");
    std::lock_guard<std::mutex> lk(x->mu);
    IVR_REQUIRE(n >= 1 && x->ntotal >= n && x->ntotal % n == 0,
                "ivr_index_write_ring: batch of %lld rows must divide ntotal=%lld (no wrap inside a batch)", (long long)n,
                (long long)x->ntotal);
    IVR_HIP(hipSetDevice(x->ctx->device));
    hipStream_t s = (hipStream_t)stream;
    // the cursor is only known on the device: launch for the worst-case number of touched tiles
    int rc = ivr_launch_tile_rows(x, x->data, rows, 0, n, normalize, nullptr, s, cursor, ivr_ceil_div(n, 16) + 1);
    if (rc != IVR_OK) return rc;
    hipLaunchKernelGGL(advance_cursor_kernel, dim3(1), dim3(1), 0, s, cursor, n, x->ntotal);
    IVR_LAUNCH_CHECK();
    return IVR_OK;
}

int ivr_index_reconstruct(ivr_index *x, int64_t start, int64_t n, float *out, ivr_stream stream) {
    IVR_REQUIRE(x && (out || n == 0), "ivr_index_reconstruct: NULL argument");
    std::lock_guard<std::mutex> lk(x->mu);
    IVR_REQUIRE(start >= 0 && n >= 0 && start + n <= x->ntotal, "ivr_index_reconstruct: rows [%lld,%lld) outside [0,%lld)",
                (long long)start, (long long)(start + n), (long long)x->ntotal);
    if (n == 0) return IVR_OK;
    IVR_HIP(hipSetDevice(x->ctx->device));
    const int64_t ntiles = ((start + n + 15) >> 4) - (start >> 4);
    hipLaunchKernelGGL(untile_rows_kernel, dim3((unsigned)ivr_ceil_div(ntiles, 4)), dim3(256), 0, (hipStream_t)stream, x->data,
                       out, start, n, x->d, x->dp4);
    IVR_LAUNCH_CHECK();
    return IVR_OK;
}

int ivr_index_remove_ids(ivr_index *x, int64_t id_base, const ivr_id_filter *filter, int64_t *n_removed, ivr_stream stream) {
    IVR_REQUIRE(x, "ivr_index_remove_ids: NULL index");
    IVR_REQUIRE(filter, "ivr_index_remove_ids: NULL filter (there is no \"remove everything\" default)");
    if (n_removed) *n_removed = 0;
    return with_view(x, id_base, filter, (hipStream_t)stream, "ivr_index_remove_ids", [&](const View &v) -> int {
        if (v.ntotal == 0) return IVR_OK;                       // no stored row has an allowed id
        hipStream_t s = (hipStream_t)stream;
        // first row of the tail: the 256-row block of the first allowed row; an id-mapped index is filtered as a whole (row 0)
        const int64_t row0 = x->has_ids ? 0 : v.id_base - id_base;
        RemovePlan p;
        p.nrows = x->ntotal - row0;
        p.ngroups = ivr_ceil_div(p.nrows, kGroupRows);
        const int64_t nblocks = ivr_ceil_div(p.ngroups + 1, kScanBlock);
        // the host plans the walk in units of 16 groups = 1,024 rows (a whole chunk when that is smaller); a chunk is whole units
        const int64_t unit = std::min<int64_t>(16, x->remove_chunk / kGroupRows);
        const int64_t chunk_units = std::min(ivr_ceil_div(x->remove_chunk / kGroupRows, unit), ivr_ceil_div(p.ngroups, unit));
        const int64_t nunits = ivr_ceil_div(p.ngroups, unit);
        int rc = ivr_reserve({{&x->rm_word, (size_t)(p.ngroups + 1) * 8}, {&x->rm_kept, (size_t)(p.ngroups + 1) * 4},
                              {&x->rm_top, (size_t)nblocks * 4}, {&x->rm_state, (size_t)(nunits + 3) * 4}});
        if (rc != IVR_OK) return rc;
        p.word = x->rm_word;
        p.kept = x->rm_kept;
        p.top = x->rm_top;
        p.state = x->rm_state;
        IVR_HIP(hipMemsetAsync(p.state, 0xff, 4, s));
        hipLaunchKernelGGL(remove_count_kernel, dim3((unsigned)ivr_ceil_div(p.ngroups + 1, 4)), dim3(256), 0, s, p, *v.mask);
        hipLaunchKernelGGL(remove_scan_kernel, dim3((unsigned)nblocks), dim3(256), 0, s, p);
        hipLaunchKernelGGL(remove_scan_top_kernel, dim3(1), dim3(256), 0, s, p, nblocks);
        hipLaunchKernelGGL(remove_bounds_kernel, dim3((unsigned)ivr_ceil_div(nunits + 1, 256)), dim3(256), 0, s, p, unit, nunits);
        IVR_LAUNCH_CHECK();
        std::vector<uint32_t> state((size_t)nunits + 3);
        IVR_HIP(hipMemcpyAsync(state.data(), p.state, state.size() * 4, hipMemcpyDeviceToHost, s));
        IVR_HIP(hipStreamSynchronize(s));                       // the one synchronisation: the host sets ntotal from the count
        const int64_t removed = p.nrows - (int64_t)state[1];
        if (removed <= 0) return IVR_OK;
        const uint32_t first = state[0], *bound = state.data() + 2;         // bound[i]: kept rows in front of unit i, i <= nunits
        rc = ivr_reserve({{&x->rm_bounce, (size_t)tile_bytes(x, (chunk_units * unit * 4 + 1) * 16)},   // + 1: destinations start inside a tile
                          {&x->rm_bounce16, x->scan16 ? (size_t)tile16_bytes(x, (chunk_units * unit * 4 + 1) * 16) : 0}});
        if (rc != IVR_OK) return rc;
        if (x->has_ids && (int64_t)state[1] > (int64_t)first) {
            // the id table follows the rows: the surviving ids from the first removed row on, gathered out of place and copied back
            const int64_t from = (int64_t)(first / kGroupRows) * kGroupRows, moved = (int64_t)state[1] - first;
            rc = ivr_reserve({{&x->ids_moved, (size_t)moved * sizeof(int64_t)}});
            if (rc != IVR_OK) return rc;
            {
                IvrProf prof("remove_ids_gather", s, (double)(p.nrows - from) * 8 + (double)moved * 8, true);
                hipLaunchKernelGGL(remove_ids_gather_kernel, dim3((unsigned)ivr_ceil_div(p.nrows - from, 256)), dim3(256), 0, s, p,
                                   x->ids + row0, (int64_t *)x->ids_moved, first);
                IVR_LAUNCH_CHECK();
            }
            IVR_HIP(hipMemcpyAsync(x->ids + row0 + first, (int64_t *)x->ids_moved, (size_t)moved * sizeof(int64_t), hipMemcpyDeviceToDevice, s));
        }
        RemoveMove mv;
        mv.data = reinterpret_cast<float4 *>(x->data + row0 * x->dp);
        mv.data16 = x->scan16 ? x->data16 + (row0 / 16) * x->pieces * 64 : nullptr;
        mv.bounce = reinterpret_cast<float4 *>((float *)x->rm_bounce);
        mv.bounce16 = x->rm_bounce16;
        mv.kchunks = x->dp / 16;
        mv.pieces = (mv.kchunks + 1) / 2;
        mv.pstride = x->pieces;
        for (int64_t i = first / (unit * kGroupRows); i < nunits;) {
            // the rows of this step that are read: from its first source row, or the first removed row, on.  As many units as end
            // at or below that row can go straight to their destination.  Taken when that is at least a chunk, or the rest of the
            // walk: a launch of fewer rows does not fill the chip, and several of them cost more than the second trip through the
            // bounce buffer (51 launches of 10,240 rows: 2.3 ms against 2.0 ms for 8 chunk pairs, 1M x 512 rows)
            const uint32_t read_from = std::max<uint32_t>((uint32_t)(i * unit * kGroupRows), first);
            int64_t j = std::upper_bound(bound + i + 1, bound + nunits + 1, read_from) - bound - 1;
            mv.direct = j > i && (j == nunits || j - i >= chunk_units);
            if (!mv.direct) j = std::min(i + chunk_units, nunits);
            mv.ga = i * unit;
            mv.gb = std::min(j * unit, p.ngroups);
            mv.dst_a = std::max(bound[i], first);
            mv.dst_b = bound[j];
            i = j;
            if (mv.dst_b <= mv.dst_a) continue;
            const unsigned grid = (unsigned)ivr_ceil_div(ivr_ceil_div(mv.dst_b, 16) - mv.dst_a / 16, 4);
            const double bytes = 2.0 * (mv.dst_b - mv.dst_a) * (x->dp * 4 + (x->scan16 ? mv.pieces * 64 : 0));    // read + written
            {
                IvrProf prof(mv.direct ? "remove_gather_direct" : "remove_gather", s, bytes, true);
                hipLaunchKernelGGL(remove_gather_kernel, dim3(grid), dim3(256), 0, s, p, mv);
            }
            if (!mv.direct) {
                IvrProf prof("remove_place", s, bytes, true);
                hipLaunchKernelGGL(remove_place_kernel, dim3(grid), dim3(256), 0, s, mv);
            }
        }
        IVR_LAUNCH_CHECK();
        // rows [ntotal', ntotal) back to zero: the slots of a partly filled tile, then whole tiles
        const int64_t keep = x->ntotal - removed;
        int64_t t0 = keep / 16;
        const int64_t t1 = ivr_ceil_div(x->ntotal, 16);
        if (keep % 16) {
            hipLaunchKernelGGL(zero_slots_kernel, dim3(1), dim3(64), 0, s, reinterpret_cast<float4 *>(x->data + t0 * 16 * x->dp),
                               x->scan16 ? x->data16 + t0 * x->pieces * 64 : (uint4 *)nullptr, (int)(keep % 16), mv.kchunks, x->pieces);
            IVR_LAUNCH_CHECK();
            ++t0;
        }
        if (t1 > t0) {
            IVR_HIP(hipMemsetAsync(x->data + t0 * 16 * x->dp, 0, (size_t)tile_bytes(x, (t1 - t0) * 16), s));
            if (x->scan16) IVR_HIP(hipMemsetAsync(x->data16 + t0 * x->pieces * 64, 0, (size_t)tile16_bytes(x, (t1 - t0) * 16), s));
        }
        x->ntotal = keep;
        x->tab_ok = false;                       // rows moved: the lookup table of ivr_index_find_ids is stale
        if (n_removed) *n_removed = removed;
        return IVR_OK;
    });
}

int ivr_l2_normalize(ivr_ctx *ctx, float *x, int64_t n, int d, int32_t *nonfinite, ivr_stream stream) {
    IVR_REQUIRE(ctx && (x || n == 0), "ivr_l2_normalize: NULL argument");
    IVR_REQUIRE(n >= 0 && d >= 1, "ivr_l2_normalize: n=%lld d=%d", (long long)n, d);
    if (n == 0) return IVR_OK;
    IVR_HIP(hipSetDevice(ctx->device));
    if (nonfinite) IVR_HIP(hipMemsetAsync(nonfinite, 0, 4, (hipStream_t)stream));
    hipLaunchKernelGGL(l2_normalize_kernel, dim3((unsigned)ivr_ceil_div(n, 4)), dim3(256), 0, (hipStream_t)stream, x, n, d,
                       nonfinite);
    IVR_LAUNCH_CHECK();
    return IVR_OK;
}

}  // extern "C"
