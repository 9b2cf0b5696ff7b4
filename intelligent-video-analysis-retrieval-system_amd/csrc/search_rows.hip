// Row access by position on the flat index: gather (faiss reconstruct_batch), scatter (update of vectors in place) and the search
// that also returns the rows behind its results (faiss search_and_reconstruct).  The rows live in 16-row tiles, inside a tile in the
// order [d/4][16 rows][4 floats] (search_index.hip), with the bf16 scan copy in the same tile order: one row of d floats is d / 4
// pieces of 16 bytes, 256 bytes apart.  A random row therefore touches every cache line of its tile, 16 times its own bytes on the
// index side; nothing here tries to hide that (no LDS staging: a wave has no second row of the same tile to share the lines with).
// The row-major side is what these kernels keep dense: lanes of a wave cover consecutive floats of one row.
#include "ivr_common.h"
#include "search_internal.h"

namespace {

// One wave per output row: lane l moves float4 number l, l + 64, ... of the row.  Float4 f of row r sits at chunk f >> 2, quad f & 3,
// slot r & 15 of tile r >> 4: a 16-byte load per lane, 256 bytes apart across the wave; the stores of a wave are 1 KiB contiguous.
// The row is row_base + rows[i] (row_base: the first row of the view a search reported its rows in, else 0); a negative entry or a row
// outside [0, ntotal) gives a NaN row.  The loop bound and the row are wave-uniform.
__global__ __launch_bounds__(256) void gather_rows_kernel(const float *__restrict__ data, const int64_t *__restrict__ rows, int64_t row_base,
                                                          int64_t n, int64_t ntotal, float *__restrict__ out, int d, int dp4) {
    const int lane = threadIdx.x & 63;
    const int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= n) return;
    const int64_t e = rows[i], r = row_base + e;
    const bool ok = e >= 0 && r >= 0 && r < ntotal;
    const float4 *in = reinterpret_cast<const float4 *>(data) + (ok ? (r >> 4) * (int64_t)dp4 * 16 + (r & 15) : 0);
    float *orow = out + i * (int64_t)d;
    const bool vec = (d & 3) == 0 && ((reinterpret_cast<uintptr_t>(out) & 15) == 0);
    const float qnan = __uint_as_float(0x7fc00000u);
    for (int f = lane; f < dp4; f += 64) {
        const int k0 = f * 4;
        if (k0 >= d) break;                                       // the padding of the last 16-float chunk
        const float4 v = ok ? in[(f >> 2) * 64 + (f & 3) * 16] : make_float4(qnan, qnan, qnan, qnan);
        if (vec) {
            *reinterpret_cast<float4 *>(orow + k0) = v;
        } else {
            orow[k0] = v.x;
            if (k0 + 1 < d) orow[k0 + 1] = v.y;
            if (k0 + 2 < d) orow[k0 + 2] = v.z;
            if (k0 + 3 < d) orow[k0 + 3] = v.w;
        }
    }
}

// tile_rows_kernel (search_index.hip) with a destination per lane: one wave per 16 SOURCE rows, lane l owns source row 16 w + (l & 15)
// and quad (l >> 4) of every 16-float chunk, and writes slot rows[i] & 15 of tile rows[i] >> 4 instead of its own slot of the wave's
// tile.  The contract is bit-identity with n single-row calls of ivr_index_write, so everything that decides a bit is that kernel's:
// the loads per lane, the norm (fmaf over this lane's quads in ascending chunk order, then the two shuffles across the quads), the
// division, the bf16 rounding and its remainder, and the two scan bounds (a maximum, so the order of the atomics does not matter).
// Entries outside [0, ntotal) are skipped like the rows a partial tile does not hold there.
__global__ __launch_bounds__(256) void scatter_rows_kernel(const float *__restrict__ src, const int64_t *__restrict__ rows, int64_t n,
                                                           int64_t ntotal, float *__restrict__ dst, int d, int dp4, int normalize,
                                                           uint4 *__restrict__ dst16, unsigned int *__restrict__ maxnorm_bits, int pstride,
                                                           unsigned int *__restrict__ maxdelta_bits) {
    const int lane = threadIdx.x & 63;
    const int64_t w = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (w * 16 >= n) return;
    const int rr = lane & 15, qd = lane >> 4;
    const int64_t i = w * 16 + rr;
    const int64_t r = i < n ? rows[i] : -1;
    const bool valid = r >= 0 && r < ntotal;
    const float *srow = src + (valid ? i : 0) * (int64_t)d;
    const bool vec = (d & 3) == 0 && ((reinterpret_cast<uintptr_t>(src) & 15) == 0);
    const int kchunks = dp4 >> 2;
    float ss = 0.f;
    if (normalize || maxnorm_bits) {
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
            }
        }
        ss += __shfl_xor(ss, 16, 64);
        ss += __shfl_xor(ss, 32, 64);
    }
    const float nrm = normalize ? (ss > 0.f ? sqrtf(ss) : 1.f) : 1.f;
    if (maxnorm_bits) {
        float stored = valid ? (normalize ? (ss > 0.f ? 1.000001f : 0.f) : sqrtf(ss)) : 0.f;
        if (!(stored == stored)) stored = INFINITY;
#pragma unroll
        for (int o = 1; o < 16; o <<= 1) stored = fmaxf(stored, __shfl_xor(stored, o, 64));
        const unsigned int bits = __float_as_uint(stored);
        if (lane == 0 && bits > *maxnorm_bits) atomicMax(maxnorm_bits, bits);
    }
    const int64_t tile = valid ? r >> 4 : 0;
    const int slot = qd * 16 + (valid ? (int)(r & 15) : 0);      // this lane's float4 / uint4 inside a 1 KiB piece of its tile
    float4 *out = reinterpret_cast<float4 *>(dst) + tile * (int64_t)dp4 * 16 + slot;
    const int pieces = (kchunks + 1) >> 1;
    float sd = 0.f;
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
            float4(&v)[2] = vv[b4];
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const int kc = 2 * kb + u;
                if (valid && kc < kchunks) {
                    if (normalize) {
                        v[u].x /= nrm;
                        v[u].y /= nrm;
                        v[u].z /= nrm;
                        v[u].w /= nrm;
                    }
                    out[kc * 64] = v[u];
                }
            }
            if (dst16 && valid) {
                uint4 hi;
                hi.x = ivr_pack_bf16x2(v[0].x, v[0].y);
                hi.y = ivr_pack_bf16x2(v[0].z, v[0].w);
                hi.z = ivr_pack_bf16x2(v[1].x, v[1].y);
                hi.w = ivr_pack_bf16x2(v[1].z, v[1].w);
                dst16[(tile * pstride + kb) * 64 + slot] = hi;
                auto lo2 = [&sd](uint32_t h, float a, float b) {
                    const float ra = a - __uint_as_float(h << 16), rb = b - __uint_as_float(h & 0xffff0000u);
                    sd = fmaf(ra, ra, sd);
                    sd = fmaf(rb, rb, sd);
                };
                lo2(hi.x, v[0].x, v[0].y);
                lo2(hi.y, v[0].z, v[0].w);
                lo2(hi.z, v[1].x, v[1].y);
                lo2(hi.w, v[1].z, v[1].w);
            }
        }
    }
    if (dst16 && maxdelta_bits) {
        sd += __shfl_xor(sd, 16, 64);
        sd += __shfl_xor(sd, 32, 64);
        float dl = valid ? sqrtf(sd) * 1.0001f : 0.f;
        if (!(dl == dl)) dl = INFINITY;
#pragma unroll
        for (int o = 1; o < 16; o <<= 1) dl = fmaxf(dl, __shfl_xor(dl, o, 64));
        const unsigned int bits = __float_as_uint(dl);
        if (lane == 0 && bits > *maxdelta_bits) atomicMax(maxdelta_bits, bits);
    }
}

}  // namespace

int ivr_launch_gather(ivr_index *x, const int64_t *rows, int64_t row_base, int64_t n, float *out, hipStream_t s) {
    if (n <= 0) return IVR_OK;
    // index side: a 16-byte piece per 64-byte line of the tile moves whole; row-major side: the row once
    IvrProf prof("gather_rows", s, (double)n * x->dp * 4 + (double)n * x->d * 4 + (double)n * 8, true);
    hipLaunchKernelGGL(gather_rows_kernel, dim3((unsigned)ivr_ceil_div(n, 4)), dim3(256), 0, s, x->data, rows, row_base, n, x->ntotal, out,
                       x->d, x->dp4);
    IVR_LAUNCH_CHECK();
    return IVR_OK;
}

extern "C" {

int ivr_index_gather(ivr_index *x, const int64_t *rows, int64_t n, float *out, ivr_stream stream) {
    IVR_REQUIRE(x && ((rows && out) || n == 0), "ivr_index_gather: NULL argument");
    IVR_REQUIRE(n >= 0 && n < (1ll << 32), "ivr_index_gather: n=%lld outside [0, 2^32)", (long long)n);
    std::lock_guard<std::mutex> lk(x->mu);
    if (n == 0) return IVR_OK;
    IVR_HIP(hipSetDevice(x->ctx->device));
    return ivr_launch_gather(x, rows, 0, n, out, (hipStream_t)stream);
}

int ivr_index_scatter(ivr_index *x, const int64_t *rows, const float *src, int64_t n, int normalize, ivr_stream stream) {
    IVR_REQUIRE(x && ((rows && src) || n == 0), "ivr_index_scatter: NULL argument");
    IVR_REQUIRE(n >= 0 && n < (1ll << 32), "ivr_index_scatter: n=%lld outside [0, 2^32)", (long long)n);
    std::lock_guard<std::mutex> lk(x->mu);
    if (n == 0) return IVR_OK;
    IVR_HIP(hipSetDevice(x->ctx->device));
    hipStream_t s = (hipStream_t)stream;
    IvrProf prof("scatter_rows", s, (double)n * (x->d + x->dp) * 4 + (x->scan16 ? (double)n * x->pieces * 64 : 0.0) + (double)n * 8, true);
    hipLaunchKernelGGL(scatter_rows_kernel, dim3((unsigned)ivr_ceil_div(ivr_ceil_div(n, 16), 4)), dim3(256), 0, s, src, rows, n, x->ntotal,
                       x->data, x->d, x->dp4, normalize, x->scan16 ? x->data16 : (uint4 *)nullptr,
                       x->scan16 ? (unsigned int *)x->maxnorm : (unsigned int *)nullptr, x->pieces,
                       x->scan16 ? (unsigned int *)x->maxdelta : (unsigned int *)nullptr);
    IVR_LAUNCH_CHECK();
    return IVR_OK;
}

int ivr_index_search_reconstruct(ivr_index *x, const float *q, int nq, int k, int normalize_q, int64_t id_base, const ivr_id_filter *filter,
                                 float *D, int64_t *I, float *R, ivr_stream stream) {
    IVR_REQUIRE(x && q && D && I && R, "ivr_index_search_reconstruct: NULL argument");
    IVR_REQUIRE(nq >= 1, "ivr_index_search_reconstruct: nq=%d", nq);
    IVR_REQUIRE(k >= 1 && k <= IVR_MAX_K, "ivr_index_search_reconstruct: k=%d outside [1,%d]", k, IVR_MAX_K);
    hipStream_t s = (hipStream_t)stream;
    return with_view(x, id_base, filter, s, "ivr_index_search_reconstruct", [&](const View &v) {
        // the view of a filtered search on a plain index starts at a 256-row block of its own; an id-mapped one is always whole
        const int64_t row_base = x->has_ids ? 0 : v.id_base - id_base;
        const int rc = ivr_search_view_pos(x, v, q, nq, k, normalize_q, D, I, s);
        return rc != IVR_OK ? rc : ivr_launch_gather(x, x->rpos, row_base, (int64_t)nq * k, R, s);
    });
}

}  // extern "C"
