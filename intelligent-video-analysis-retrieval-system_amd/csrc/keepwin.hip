// The two look-back filters of the research keyframe extractor (filter_research_update.py): the perceptual-duplicate filter inside a
// scene (:157-162, :289-298) and the final temporal filter over a video's representatives (:316-338).
//
// Both keep a row unless it is too close to one of the last `window` KEPT rows of its segment.  Whether a row is kept decides what the
// next row is compared with, so the rows of one segment are a serial chain; segments run in parallel, one wave (hashes) or one
// workgroup (embeddings) each.  The window lives in lanes: lane j holds entry j of a ring, `pos` is the slot the next kept row
// takes, which is the oldest entry once the ring is full.
#include "ivr_common.h"

namespace {

// [lo, hi) of segment s, clipped to [0, n); seg_off == NULL: the one segment [0, n)
__device__ __forceinline__ void segment_range(const int64_t *__restrict__ seg_off, int s, int64_t n, int64_t *lo, int64_t *hi) {
    if (!seg_off) {
        *lo = 0;
        *hi = n;
        return;
    }
    *lo = min(max(seg_off[s], (int64_t)0), n);
    *hi = min(max(seg_off[s + 1], *lo), n);
}

// One wave per segment.  64 rows at a time: lane l loads hash lo + l, the wave walks the 64 in order (each broadcast from its lane),
// lane l collects the decision of its row, and the 64 decisions go out as 64 adjacent bytes.
__global__ __launch_bounds__(256) void hash_keep_kernel(const uint8_t *__restrict__ hashes, int64_t n, const int64_t *__restrict__ seg_off,
                                                        int nseg, int threshold, int window, uint8_t *__restrict__ keep) {
    const int lane = threadIdx.x & 63;
    const int seg = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (seg >= nseg) return;
    int64_t lo, hi;
    segment_range(seg_off, seg, n, &lo, &hi);
    uint32_t win_lo = 0, win_hi = 0;      // this lane's window entry
    int count = 0, pos = 0;               // wave-uniform
    for (int64_t base = lo; base < hi; base += 64) {
        const int rows = (int)min((int64_t)64, hi - base);
        uint32_t my_lo = 0, my_hi = 0;
        if (lane < rows) {
            const uint8_t *p = hashes + (base + lane) * 8;
            my_lo = p[0] | (p[1] << 8) | (p[2] << 16) | ((uint32_t)p[3] << 24);
            my_hi = p[4] | (p[5] << 8) | (p[6] << 16) | ((uint32_t)p[7] << 24);
        }
        int mine = 0;
        for (int r = 0; r < rows; ++r) {
            const uint32_t h_lo = __builtin_amdgcn_readlane(my_lo, r), h_hi = __builtin_amdgcn_readlane(my_hi, r);
            const bool near = lane < count && __popc(h_lo ^ win_lo) + __popc(h_hi ^ win_hi) <= threshold;
            const bool kept = __ballot(near) == 0ull;
            if (kept) {                   // wave-uniform
                if (lane == pos) {
                    win_lo = h_lo;
                    win_hi = h_hi;
                }
                pos = pos + 1 == window ? 0 : pos + 1;
                count = min(count + 1, window);
            }
            if (lane == r) mine = kept ? 1 : 0;
        }
        if (lane < rows) keep[base + lane] = (uint8_t)mine;
    }
}

// 1 / 0-safe norms of the rows, as ivr_rowwise_cosine forms them: a per-lane fma chain over the columns l, l + 64, ..., the wave sum,
// sqrt, a zero norm counts as 1.  One wave per row.
__global__ __launch_bounds__(256) void row_norm_kernel(const float *__restrict__ emb, int64_t n, int d, float *__restrict__ norm) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= n) return;
    const float *p = emb + row * d;
    float ss = 0.f;
    for (int k = lane; k < d; k += 64) {
        const float x = p[k];
        ss = fmaf(x, x, ss);
    }
    ss = ivr_wave_sum(ss);
    if (lane == 0) norm[row] = ss > 0.f ? sqrtf(ss) : 1.f;
}

// One workgroup of four waves per segment.  Every wave carries the same window (row numbers, in lanes) and the same ring state; for
// row i wave v tests the entries v, v + 4, ... and raises a flag in LDS when one of them reaches the threshold.  One barrier per row:
// the flags rotate through three slots, so the slot of row i + 1 is cleared while nobody can still be reading it (its last readers,
// of row i - 2, have passed the barrier of row i - 1).
__global__ __launch_bounds__(256) void kept_window_kernel(const float *__restrict__ emb, int64_t n, int d, const float *__restrict__ norm,
                                                          const int64_t *__restrict__ seg_off, float threshold, int window,
                                                          uint8_t *__restrict__ keep) {
    __shared__ int hit[3];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int64_t lo, hi;
    segment_range(seg_off, blockIdx.x, n, &lo, &hi);
    if (threadIdx.x < 3) hit[threadIdx.x] = 0;
    __syncthreads();
    uint32_t win = 0;                     // this lane's window entry: a row number relative to lo
    int count = 0, pos = 0, slot = 0;     // uniform over the workgroup
    for (int64_t i = lo; i < hi; ++i) {
        const float *pa = emb + i * d;
        const float na = norm[i];
        bool found = false;
        for (int j = wave; j < count; j += 4) {
            const int64_t rj = lo + __builtin_amdgcn_readlane(win, j);
            const float *pb = emb + rj * d;
            float dot = 0.f;
            for (int k = lane; k < d; k += 64) dot = fmaf(pa[k], pb[k], dot);
            dot = ivr_wave_sum(dot);
            if (dot / (na * norm[rj]) >= threshold) found = true;
        }
        if (found && lane == 0) hit[slot] = 1;
        if (threadIdx.x == 0) hit[slot == 2 ? 0 : slot + 1] = 0;
        __syncthreads();
        const bool kept = hit[slot] == 0;
        slot = slot == 2 ? 0 : slot + 1;
        if (kept) {
            if (lane == pos) win = (uint32_t)(i - lo);
            pos = pos + 1 == window ? 0 : pos + 1;
            count = min(count + 1, window);
        }
        if (threadIdx.x == 0) keep[i] = kept ? 1 : 0;
    }
}

}  // namespace

extern "C" int ivr_hash_keep_mask(ivr_ctx *ctx, const uint8_t *hashes, int64_t n, const int64_t *seg_off, int nseg, int threshold,
                                  int window, uint8_t *keep, ivr_stream stream) {
    IVR_REQUIRE(ctx && (n == 0 || (hashes && keep)), "ivr_hash_keep_mask: NULL argument");
    IVR_REQUIRE(n >= 0 && nseg >= 0 && (nseg > 0) == (seg_off != nullptr), "ivr_hash_keep_mask: n=%lld nseg=%d (seg_off with nseg >= 1, or neither)",
                (long long)n, nseg);
    IVR_REQUIRE(window >= 1 && window <= IVR_KEEPWIN_MAX_WINDOW, "ivr_hash_keep_mask: window=%d outside [1,%d]", window,
                IVR_KEEPWIN_MAX_WINDOW);
    if (n == 0) return IVR_OK;
    IVR_HIP(hipSetDevice(ctx->device));
    hipStream_t s = (hipStream_t)stream;
    const int segs = seg_off ? nseg : 1;
    if (seg_off) IVR_HIP(hipMemsetAsync(keep, 0, (size_t)n, s));                   // rows outside every segment
    hipLaunchKernelGGL(hash_keep_kernel, dim3((unsigned)ivr_ceil_div(segs, 4)), dim3(256), 0, s, hashes, n, seg_off, segs, threshold, window,
                       keep);
    IVR_LAUNCH_CHECK();
    return IVR_OK;
}

extern "C" int ivr_kept_window_mask(ivr_ctx *ctx, const float *emb, int64_t n, int d, const int64_t *seg_off, int nseg, float threshold,
                                    int window, uint8_t *keep, ivr_stream stream) {
    IVR_REQUIRE(ctx && (n == 0 || (emb && keep)), "ivr_kept_window_mask: NULL argument");
    IVR_REQUIRE(n >= 0 && d >= 1 && nseg >= 0 && (nseg > 0) == (seg_off != nullptr),
                "ivr_kept_window_mask: n=%lld d=%d nseg=%d (seg_off with nseg >= 1, or neither)", (long long)n, d, nseg);
    IVR_REQUIRE(window >= 1 && window <= IVR_KEEPWIN_MAX_WINDOW, "ivr_kept_window_mask: window=%d outside [1,%d]", window,
                IVR_KEEPWIN_MAX_WINDOW);
    IVR_REQUIRE(threshold == threshold, "ivr_kept_window_mask: threshold is NaN");
    if (n == 0) return IVR_OK;
    IVR_HIP(hipSetDevice(ctx->device));
    hipStream_t s = (hipStream_t)stream;
    IVR_REQUIRE(ivr_ceil_div(n, 4) < (1ll << 31), "ivr_kept_window_mask: n=%lld exceeds the grid", (long long)n);
    std::lock_guard<std::mutex> enqueue(ctx->enqueue_mu);           // the two launches share the stream's scratch block
    void *scratch = nullptr;
    if (int rc = ivr_ctx_scratch(ctx, s, (size_t)n * sizeof(float), &scratch)) return rc;
    float *norm = reinterpret_cast<float *>(scratch);
    hipLaunchKernelGGL(row_norm_kernel, dim3((unsigned)ivr_ceil_div(n, 4)), dim3(256), 0, s, emb, n, d, norm);
    IVR_LAUNCH_CHECK();
    if (seg_off) IVR_HIP(hipMemsetAsync(keep, 0, (size_t)n, s));
    hipLaunchKernelGGL(kept_window_kernel, dim3((unsigned)(seg_off ? nseg : 1)), dim3(256), 0, s, emb, n, d, norm, seg_off, threshold,
                       window, keep);
    IVR_LAUNCH_CHECK();
    return IVR_OK;
}
