// Perceptual hash of a batch of frames on MI355X: imagehash.phash (filter_research_update.py:97-99, called per frame at :250).
//
//   grey    (R*19595 + G*38470 + B*7471 + 0x8000) >> 16, Pillow's convert('L')
//   resize  to 32x32 with Pillow's 8-bit resampler and the Lanczos filter: the 22-bit fixed-point taps of resample_taps.h, int32
//           accumulate from 1<<21, >>22, clamp, a uint8 image between the horizontal and the vertical pass
//   DCT     float64, type II, unnormalised, columns then rows, low 8x8 block; every product and sum rounded on its own
//   bits    coefficient > median of the 64, packed row-major, most significant bit first
//
// Two launches.  phash_rows_kernel reads the frame bytes, exactly once: one workgroup per (frame, band of rows) loads its rows (one
// contiguous run of bytes) with 16-byte loads into LDS, turns them grey there and writes 32 bytes per row.  phash_frame_kernel, one
// workgroup per frame, reads those [h,32] bytes: vertical pass, the two DCT stages, the median by rank counting, one ballot.
#include "ivr_common.h"
#include "resample_taps.h"

#include <cmath>
#include <map>
#include <tuple>

namespace {

using ivr_resample::kPrecisionBits;

constexpr int kSide = 32;            // the resized image
constexpr int kMaxBandRows = 16;     // rows of one workgroup of the row kernel (accumulators per thread)
constexpr int kBandLds = 32000;      // LDS bytes the rows of a band may take (raw RGB + grey): 4 or 5 workgroups per CU

// ---------------------------------------------------------------------------------------------
// grey + horizontal pass.  tab: xmin[32], xcnt[32], kk[ksize][32] (NULL: w == 32, no pass).  out: uint8 [n,h,32].
// Thread (x = tid & 31, part = tid >> 5) sums the taps part, part + 8, ... of output column x for every row of the band, so a tap
// is loaded once per band, not once per row; the eight partial sums meet in LDS (integer adds: any order gives the same sum).
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void phash_rows_kernel(const uint8_t *__restrict__ src, uint8_t *__restrict__ out, int h, int w,
                                                         int band_rows, int bands, int bgr, const int32_t *__restrict__ tab) {
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    const int tid = threadIdx.x;
    const int f = blockIdx.x / bands, y0 = (blockIdx.x % bands) * band_rows;
    const int rows = min(band_rows, h - y0);
    const int nbytes = rows * w * 3;
    uint8_t *raw = lds;                                                            // [shift + nbytes]
    uint8_t *grey = lds + (((size_t)band_rows * w * 3 + 16 + 15) & ~(size_t)15);   // [rows][w]
    int32_t *acc = reinterpret_cast<int32_t *>(grey + (((size_t)band_rows * w + 3) & ~(size_t)3));   // [rows][32]
    const uint8_t *g = src + ((int64_t)f * h + y0) * w * 3;
    // the band's bytes land at raw + shift, so that 16-byte aligned global addresses are 16-byte aligned in LDS as well
    const int shift = (int)(reinterpret_cast<uintptr_t>(g) & 15);
    const int head = min(nbytes, (16 - shift) & 15);
    const int body = (nbytes - head) & ~15;
    const int tail = nbytes - head - body;
    if (tid < head) raw[shift + tid] = g[tid];
    if (tid >= 64 && tid - 64 < tail) raw[shift + head + body + tid - 64] = g[head + body + tid - 64];
    for (int i = tid * 16; i < body; i += 256 * 16)
        *reinterpret_cast<uint4 *>(raw + shift + head + i) = *reinterpret_cast<const uint4 *>(g + head + i);
    for (int i = tid; i < rows * kSide; i += 256) acc[i] = 1 << (kPrecisionBits - 1);
    __syncthreads();
    const int cr = bgr ? 2 : 0, cb = bgr ? 0 : 2;
    for (int i = tid; i < rows * w; i += 256) {
        const uint8_t *p = raw + shift + 3 * i;
        grey[i] = (uint8_t)(((uint32_t)p[cr] * 19595u + (uint32_t)p[1] * 38470u + (uint32_t)p[cb] * 7471u + 0x8000u) >> 16);
    }
    __syncthreads();
    uint8_t *o = out + ((int64_t)f * h + y0) * kSide;
    if (!tab) {                                                                    // w == 32
        for (int i = tid; i < rows * kSide; i += 256) o[i] = grey[i];
        return;
    }
    const int x = tid & 31, part = tid >> 5;
    const int lo = tab[x], cnt = tab[kSide + x];
    const int32_t *kk = tab + 2 * kSide + x;
    int32_t sum[kMaxBandRows];
#pragma unroll
    for (int r = 0; r < kMaxBandRows; ++r) sum[r] = 0;
    for (int t = part; t < cnt; t += 8) {
        const int32_t k = kk[t * kSide];
        const uint8_t *gp = grey + lo + t;
#pragma unroll
        for (int r = 0; r < kMaxBandRows; ++r)
            if (r < rows) sum[r] += (int32_t)gp[r * w] * k;
    }
#pragma unroll
    for (int r = 0; r < kMaxBandRows; ++r)
        if (r < rows) atomicAdd(&acc[r * kSide + x], sum[r]);
    __syncthreads();
    for (int i = tid; i < rows * kSide; i += 256) {
        const int32_t a = acc[i] >> kPrecisionBits;
        o[i] = (uint8_t)(a < 0 ? 0 : (a > 255 ? 255 : a));
    }
}

// ---------------------------------------------------------------------------------------------
// vertical pass + DCT + median + bits, one workgroup per frame.  rows: uint8 [n,h,32]; tab as above for the vertical axis (NULL:
// h == 32); ctab: the 256 doubles of ivr_phash_cos_table.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void phash_frame_kernel(const uint8_t *__restrict__ rows, int h, const int32_t *__restrict__ tab,
                                                          const double *__restrict__ ctab, uint8_t *__restrict__ hash,
                                                          uint8_t *__restrict__ pixels) {
#pragma clang fp contract(off)     // every product and every sum of the DCT is rounded on its own
    __shared__ uint8_t px[kSide * kSide];
    __shared__ double C[8 * kSide], A[8 * kSide], B[64], mid[2];
    const int tid = threadIdx.x, lane = tid & 63;
    const int64_t f = blockIdx.x;
    const uint8_t *in = rows + f * h * kSide;
    C[tid] = ctab[tid];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int o = tid + 256 * j, y = o >> 5, x = o & 31;
        int v;
        if (tab) {
            const int lo = tab[y], cnt = tab[kSide + y];
            const int32_t *kk = tab + 2 * kSide + y;
            int32_t a = 1 << (kPrecisionBits - 1);
            for (int t = 0; t < cnt; ++t) a += (int32_t)in[(lo + t) * kSide + x] * kk[t * kSide];
            a >>= kPrecisionBits;
            v = a < 0 ? 0 : (a > 255 ? 255 : a);
        } else {
            v = in[o];
        }
        px[o] = (uint8_t)v;
        if (pixels) pixels[f * kSide * kSide + o] = (uint8_t)v;
    }
    __syncthreads();
    {   // A[k][x] = 2 sum_y C[k][y] p[y][x], ascending y
        const int k = tid >> 5, x = tid & 31;
        double s = 0.0;
        for (int y = 0; y < kSide; ++y) {
            const double p = C[k * kSide + y] * (double)px[y * kSide + x];
            s = s + p;
        }
        A[tid] = 2.0 * s;
    }
    __syncthreads();
    // B[k][l] = 2 sum_x A[k][x] C[l][x], ascending x: lane = 8 k + l of the first wave owns one coefficient
    double b = 0.0;
    if (tid < 64) {
        const int k = lane >> 3, l = lane & 7;
        double s = 0.0;
        for (int x = 0; x < kSide; ++x) {
            const double p = A[k * kSide + x] * C[l * kSide + x];
            s = s + p;
        }
        b = 2.0 * s;
        B[lane] = b;
    }
    __syncthreads();
    if (tid < 64) {
        int rank = 0;                                       // position of b in the sorted order (equal values: by lane)
        for (int j = 0; j < 64; ++j) {
            const double o = B[j];
            rank += (o < b || (o == b && j < lane)) ? 1 : 0;
        }
        if (rank == 31) mid[0] = b;
        if (rank == 32) mid[1] = b;
    }
    __syncthreads();
    if (tid >= 64) return;
    const double med = (mid[0] + mid[1]) * 0.5;
    const unsigned long long bits = __ballot(b > med);      // bit 8 k + l
    if (lane < 8) hash[f * 8 + lane] = (uint8_t)(__brev((unsigned)((bits >> (8 * lane)) & 0xff)) >> 24);
}

struct HashPlan {                       // the tap tables of one (h, w) on one device
    int32_t *d_h = nullptr, *d_v = nullptr;
    int band_rows = 1;
};
struct HashPlans {
    std::mutex mu;
    std::map<std::tuple<int, int, int>, HashPlan> plans;
    std::map<int, double *> cos;        // device -> the cosine table
};
HashPlans &hash_plans() {
    static HashPlans p;
    return p;
}

int upload_taps(int in_size, int32_t **out) {
    const ivr_resample::Taps t = ivr_resample::make_taps(in_size, kSide, 0, kSide, ivr_resample::kLanczos);
    std::vector<int32_t> host((size_t)kSide * (2 + t.ksize));
    for (int i = 0; i < kSide; ++i) {
        host[i] = t.xmin[i];
        host[kSide + i] = t.xcnt[i];
    }
    for (size_t i = 0; i < t.kk.size(); ++i) host[2 * kSide + i] = t.kk[i];
    IVR_HIP(hipMalloc(out, host.size() * 4));
    IVR_HIP(hipMemcpy(*out, host.data(), host.size() * 4, hipMemcpyHostToDevice));
    return IVR_OK;
}

int get_hash_plan(int device, int h, int w, const HashPlan **out, const double **d_cos) {
    HashPlans &hp = hash_plans();
    std::lock_guard<std::mutex> lk(hp.mu);
    auto ci = hp.cos.find(device);
    if (ci == hp.cos.end()) {
        double host[256], *d = nullptr;
        ivr_phash_cos_table(host);
        IVR_HIP(hipMalloc(&d, sizeof(host)));
        IVR_HIP(hipMemcpy(d, host, sizeof(host), hipMemcpyHostToDevice));
        ci = hp.cos.emplace(device, d).first;
    }
    *d_cos = ci->second;
    auto key = std::make_tuple(device, h, w);
    auto it = hp.plans.find(key);
    if (it == hp.plans.end()) {
        HashPlan p;
        if (w != kSide)
            if (int rc = upload_taps(w, &p.d_h)) return rc;
        if (h != kSide)
            if (int rc = upload_taps(h, &p.d_v)) return rc;
        p.band_rows = std::max(1, std::min(kMaxBandRows, kBandLds / (4 * w)));
        it = hp.plans.emplace(key, p).first;
    }
    *out = &it->second;
    return IVR_OK;
}

}  // namespace

extern "C" {

int ivr_phash_cos_table(double *out) {
    IVR_REQUIRE(out, "ivr_phash_cos_table: NULL argument");
    for (int k = 0; k < 8; ++k)
        for (int m = 0; m < kSide; ++m) out[k * kSide + m] = std::cos(M_PI * (double)(k * (2 * m + 1)) / 64.0);
    return IVR_OK;
}

int64_t ivr_phash_scratch_bytes(int n, int h, int w) {
    (void)w;
    return (int64_t)n * h * kSide + 256;
}

int ivr_phash(ivr_ctx *ctx, const uint8_t *src, int n, int h, int w, int flags, uint8_t *hash, uint8_t *pixels, ivr_stream stream) {
    IVR_REQUIRE(ctx, "ivr_phash: NULL argument");
    IVR_REQUIRE(n >= 0 && h >= 1 && w >= 1 && h <= IVR_PHASH_MAX_SIDE && w <= IVR_PHASH_MAX_SIDE,
                "ivr_phash: n=%d h=%d w=%d (1 <= h, w <= %d)", n, h, w, IVR_PHASH_MAX_SIDE);
    IVR_REQUIRE((flags & ~IVR_PP_BGR) == 0, "ivr_phash: flags=0x%x (IVR_PP_BGR only)", flags);
    IVR_REQUIRE(n == 0 || (src && hash), "ivr_phash: NULL frame or hash buffer");
    if (n == 0) return IVR_OK;
    IVR_HIP(hipSetDevice(ctx->device));
    hipStream_t s = (hipStream_t)stream;
    std::lock_guard<std::mutex> enqueue(ctx->enqueue_mu);           // the two launches share the stream's scratch block
    const HashPlan *p = nullptr;
    const double *d_cos = nullptr;
    if (int rc = get_hash_plan(ctx->device, h, w, &p, &d_cos)) return rc;
    void *scratch = nullptr;
    if (int rc = ivr_ctx_scratch(ctx, s, (size_t)ivr_phash_scratch_bytes(n, h, w), &scratch)) return rc;
    uint8_t *rows = reinterpret_cast<uint8_t *>(scratch);
    const int R = p->band_rows, bands = (int)ivr_ceil_div(h, R);
    IVR_REQUIRE((int64_t)n * bands < (1ll << 31), "ivr_phash: n=%d frames of %d bands exceed the grid", n, bands);
    const size_t lds = (((size_t)R * w * 3 + 16 + 15) & ~(size_t)15) + (((size_t)R * w + 3) & ~(size_t)3) + (size_t)R * kSide * 4;
    {
        IvrProf prof("phash_rows", s, (double)n * h * w * 3 + (double)n * h * kSide);       // bytes read + written
        hipLaunchKernelGGL(phash_rows_kernel, dim3((unsigned)((int64_t)n * bands)), dim3(256), lds, s, src, rows, h, w, R, bands,
                           (flags & IVR_PP_BGR) ? 1 : 0, p->d_h);
    }
    IVR_LAUNCH_CHECK();
    hipLaunchKernelGGL(phash_frame_kernel, dim3((unsigned)n), dim3(256), 0, s, rows, h, p->d_v, d_cos, hash, pixels);
    IVR_LAUNCH_CHECK();
    return IVR_OK;
}

}  // extern "C"
