// The flat index object (ivr_index) and its storage: rows are kept in tiles of 16 rows, inside a tile in the order
// [d/4][16 rows][4 floats] (the MFMA operand layout that search.hip scans, see there), with a bf16 scan copy alongside.  Create /
// destroy / reset / add / write / reconstruct, the tiling kernels (also used for the queries of a search) and the grow-only
// workspace buffers.
#include "ivr_common.h"
#include "search_internal.h"

namespace {

// ---------------------------------------------------------------------------------------------
// tiling: row-major [n,d] -> tiled, with optional L2 normalisation (N2/N3) and non-finite count
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ float4 load_quad(const float *__restrict__ row, int k0, int d, bool vec) {
    if (vec) return *reinterpret_cast<const float4 *>(row + k0);   // k0 + 3 < d guaranteed by caller when vec
    float4 v;
    v.x = k0 + 0 < d ? row[k0 + 0] : 0.f;
    v.y = k0 + 1 < d ? row[k0 + 1] : 0.f;
    v.z = k0 + 2 < d ? row[k0 + 2] : 0.f;
    v.w = k0 + 3 < d ? row[k0 + 3] : 0.f;
    return v;
}

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
                if (valid && kc0 + u < kchunks && k0 < d) v[u] = load_quad(srow, k0, d, vec && k0 + 3 < d);
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
            if (valid && kc < kchunks && k0 < d) vv[b4][u] = load_quad(srow, k0, d, vec && k0 + 3 < d);
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

// every buffer of the group empty again; the first error, if any
int release_all(DevSizes bufs) {
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

int allocate_all(DevSizes bufs, bool zero) {
    for (const auto &b : bufs) {
        if (b.second == 0) continue;
        IVR_HIP(hipMalloc(&b.first->ptr, b.second));
        b.first->bytes = b.second;
        if (zero) IVR_HIP(hipMemset(b.first->ptr, 0, b.second));
    }
    return IVR_OK;
}

}  // namespace

int ivr_reserve(DevSizes bufs, bool zero) {
    bool enough = true;
    for (const auto &b : bufs) enough = enough && b.second <= b.first->bytes;
    if (enough) return IVR_OK;
    int rc = release_all(bufs);
    if (rc == IVR_OK) rc = allocate_all(bufs, zero);
    // all or nothing: after a failed allocation no buffer of the group is left behind, so the next call starts over and reports the
    // error again instead of finding some buffers present and launching on the missing ones
    if (rc != IVR_OK) (void)release_all(bufs);
    return rc;
}

View ivr_make_view(const ivr_index *x, int64_t id_base, const ivr_id_filter *f, RowMask &m) {
    if (!f) return View{x->data, x->data16, x->ntotal, ivr_ceil_div(x->ntotal, kGroupRows), id_base, nullptr};
    __int128 lo = f->lo, hi = f->hi;
    if (f->bits) {                              // ids the bitmap covers: [0, nbits)
        lo = std::max<__int128>(lo, 0);
        hi = std::min<__int128>(hi, f->nbits);
    }
    const __int128 rlo = std::max<__int128>(lo - id_base, 0), rhi = std::min<__int128>(hi - id_base, x->ntotal);
    if (rlo >= rhi) return View{x->data, x->data16, 0, 0, id_base, &m};
    const int64_t b0 = (int64_t)rlo / 256 * 256, n = (int64_t)rhi - b0;
    m.lo = (int64_t)rlo - b0;
    m.hi = n;
    m.bits = f->bits;
    m.bit0 = id_base + b0;
    return View{x->data + b0 * x->dp, x->data16 ? x->data16 + (b0 / 16) * x->pieces * 64 : nullptr, n, ivr_ceil_div(n, kGroupRows),
                id_base + b0, &m};
}

int ivr_launch_tile_rows(ivr_index *x, float *dst, const float *src, int64_t start, int64_t n, int normalize, int32_t *nonfinite,
                         hipStream_t s, const int64_t *start_dev, int64_t max_tiles) {
    if (n <= 0) return IVR_OK;
    const int64_t ntiles = max_tiles ? max_tiles : ((start + n + 15) >> 4) - (start >> 4);
    const unsigned grid = (unsigned)ivr_ceil_div(ntiles, 4);
    const bool rows = dst == x->data;
    IvrProf prof("tile_rows", s, (double)n * (x->d + x->dp) * 4 + (x->scan16 ? (double)n * x->pieces * 64 * (rows ? 1 : 2) : 0.0), true);
    // query tiles: the padding rows of the last tile are zero-filled by the kernel itself (no memset in front of it)
    hipLaunchKernelGGL(tile_rows_kernel, dim3(grid), dim3(256), 0, s, src, dst, start, n, x->d, x->dp4, normalize, nonfinite, start_dev,
                       x->scan16 ? (rows ? x->data16 : x->q16hi) : (uint4 *)nullptr, x->scan16 && !rows ? x->q16lo : (uint4 *)nullptr,
                       x->scan16 && rows ? x->maxnorm : (unsigned int *)nullptr, rows ? (float *)nullptr : x->qnorm, rows ? 0 : 1,
                       x->pieces, x->scan16 && rows ? x->maxdelta : (unsigned int *)nullptr,
                       x->scan16 && !rows ? x->qdelta : (float *)nullptr);
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
    return IVR_OK;
}

int64_t ivr_index_ntotal(ivr_index *x) { return x ? x->ntotal : 0; }
int ivr_index_dim(ivr_index *x) { return x ? x->d : 0; }
int64_t ivr_index_capacity(ivr_index *x) { return x ? x->cap : 0; }

int ivr_index_add(ivr_index *x, const float *rows, int64_t n, int normalize, ivr_stream stream) {
    IVR_REQUIRE(x && (rows || n == 0), "ivr_index_add: NULL argument");
    IVR_REQUIRE(n >= 0, "ivr_index_add: n=%lld", (long long)n);
    std::lock_guard<std::mutex> lk(x->mu);
    IVR_HIP(hipSetDevice(x->ctx->device));
    if (x->ntotal + n > x->cap) {
        IVR_REQUIRE(x->ntotal + n < (1ll << 32) - 64, "ivr_index_add: index would exceed 2^32 rows");
        // growing re-allocates: wait for work that may still read the old buffer
        IVR_HIP(hipDeviceSynchronize());
        int rc = index_alloc(x, std::max<int64_t>(x->ntotal + n, x->cap + x->cap / 2));
        if (rc != IVR_OK) return rc;
    }
    int rc = ivr_launch_tile_rows(x, x->data, rows, x->ntotal, n, normalize, nullptr, (hipStream_t)stream);
    if (rc != IVR_OK) return rc;
    x->ntotal += n;
    return IVR_OK;
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
