// Merge of per-shard top-k lists (sharded index): the radix selector of search_select.h over the candidates of all parts, as
// (D, I) arrays or as the packed three-word candidates of the all-gather buffer.
#include "ivr_common.h"
#include "search_select.h"

namespace {

__global__ __launch_bounds__(256) void pack_candidates_kernel(const float *__restrict__ D, const int64_t *__restrict__ I, int64_t n,
                                                              int32_t *__restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int64_t id = I[i];
    out[3 * i] = __float_as_int(D[i]);
    out[3 * i + 1] = (int32_t)(uint32_t)(id & 0xffffffffll);
    out[3 * i + 2] = (int32_t)(id >> 32);
}

}  // namespace

extern "C" {

int ivr_topk_merge(ivr_ctx *ctx, const float *D_parts, const int64_t *I_parts, int parts, int nq, int k, float *D,
                   int64_t *I, ivr_stream stream) {
    IVR_REQUIRE(ctx && D_parts && I_parts && D && I, "ivr_topk_merge: NULL argument");
    IVR_REQUIRE(parts >= 1 && nq >= 1 && k >= 1 && k <= IVR_MAX_K, "ivr_topk_merge: parts=%d nq=%d k=%d", parts, nq, k);
    IVR_HIP(hipSetDevice(ctx->device));
    SelectOut o = SelectOut::to_rows(D, I);
    o.I_parts = I_parts;
    launch_select<OUT_DI_PARTS>(SrcParts{D_parts, I_parts, nq, k, (int64_t)parts * k}, nq, k, o, (hipStream_t)stream);
    IVR_LAUNCH_CHECK();
    return IVR_OK;
}

int ivr_topk_pack(ivr_ctx *ctx, const float *D, const int64_t *I, int nq, int k, int32_t *packed, ivr_stream stream) {
    IVR_REQUIRE(ctx && D && I && packed, "ivr_topk_pack: NULL argument");
    IVR_REQUIRE(nq >= 1 && k >= 1, "ivr_topk_pack: nq=%d k=%d", nq, k);
    IVR_HIP(hipSetDevice(ctx->device));
    const int64_t n = (int64_t)nq * k;
    hipLaunchKernelGGL(pack_candidates_kernel, dim3((unsigned)ivr_ceil_div(n, 256)), dim3(256), 0, (hipStream_t)stream, D, I, n, packed);
    IVR_LAUNCH_CHECK();
    return IVR_OK;
}

int ivr_topk_merge_packed(ivr_ctx *ctx, const int32_t *packed_parts, int parts, int nq, int k, float *D, int64_t *I, ivr_stream stream) {
    IVR_REQUIRE(ctx && packed_parts && D && I, "ivr_topk_merge_packed: NULL argument");
    IVR_REQUIRE(parts >= 1 && nq >= 1 && k >= 1 && k <= IVR_MAX_K, "ivr_topk_merge_packed: parts=%d nq=%d k=%d", parts, nq, k);
    IVR_HIP(hipSetDevice(ctx->device));
    launch_select<OUT_DI_PACKED>(SrcPacked{packed_parts, nq, k, (int64_t)parts * k}, nq, k, SelectOut::to_rows(D, I), (hipStream_t)stream);
    IVR_LAUNCH_CHECK();
    return IVR_OK;
}

}  // extern "C"
