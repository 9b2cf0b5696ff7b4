// Stable external ids (faiss IndexIDMap2 / add_with_ids): what an id-mapped index does with its id table besides carrying it.  The
// table itself (ivr_index::ids, one int64 label per stored row) is allocated, grown, appended to and compacted with the rows in
// search_index.hip; the label of a result is read from it by the final write of each search path (select_topk_kernel<.., OUT_DI_IDS>,
// range_write_kernel<true>).  Here: the pass that turns a filter over stored ids into a row bitmap, so that every masked kernel runs
// as it is, the lookup of rows by id, and the two entry points that read the table back.
#include "ivr_common.h"
#include "search_internal.h"

namespace {

// One wave per 64-row group: lane l tests the id of row 64 g + l against the filter, the ballot is the group's word of the row bitmap.
// lo < hi, and with a bitmap [lo, hi) lies inside [0, nbits): the host clipped them.  A bitmap byte exists only for ids in [lo, hi)
// (the caller may pass `bits` offset in front of its buffer), so a lane whose id is outside loads the byte of `lo` instead: an
// in-range address for every lane, no branch around the load.  Table entries of the rows >= ntotal of the last group lie inside the
// allocation (cap is a multiple of 64) and are masked by the row test.
__global__ __launch_bounds__(256) void ids_row_mask_kernel(const int64_t *__restrict__ ids, int64_t ntotal, int64_t ngroups, int64_t lo,
                                                           int64_t hi, const uint8_t *__restrict__ bits, uint64_t *__restrict__ out) {
    const int lane = threadIdx.x & 63;
    const int64_t g = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (g >= ngroups) return;
    const int64_t r = g * kGroupRows + lane;
    const int64_t id = ids[r];                                   // 512 B per wave, coalesced
    bool ok = r < ntotal && id >= lo && id < hi;
    if (bits) {
        const int64_t b = ok ? id : lo;
        const uint32_t byte = bits[b >> 3];
        ok = ok && ((byte >> (id & 7)) & 1u);
    }
    const uint64_t word = __ballot(ok);
    if (lane == 0) out[g] = word;
}

// rows[i] = the lowest row whose id is keys[i], or -1: a grid-stride scan of the table, every thread compares its id with every key
// (the keys are read at wave-uniform addresses) and a match lowers the key's slot by an atomic minimum.  The slots start as -1 =
// the largest unsigned value, so "none" needs no second pass.  O(keys x ntotal) compares: meant for a handful of keys.
__global__ __launch_bounds__(256) void ids_find_kernel(const int64_t *__restrict__ ids, int64_t ntotal, const int64_t *__restrict__ keys,
                                                       int64_t nkeys, unsigned long long *__restrict__ rows) {
    for (int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x; r < ntotal; r += (int64_t)gridDim.x * 256) {
        const int64_t id = ids[r];
        for (int64_t i = 0; i < nkeys; ++i)
            if (keys[i] == id) atomicMin(&rows[i], (unsigned long long)r);
    }
}

}  // namespace

int ivr_make_ids_view(ivr_index *x, const ivr_id_filter *f, RowMask &m, hipStream_t s, View &out) {
    const int64_t ngroups = ivr_ceil_div(x->ntotal, kGroupRows);
    out = View{x->data, x->data16, x->ntotal, ngroups, 0, nullptr, x->ids};
    if (!f) return IVR_OK;
    // stored ids are >= 0 (-1 labels an unused slot), and a bitmap covers the ids [0, nbits)
    const int64_t lo = std::max<int64_t>(f->lo, 0), hi = f->bits ? std::min(f->hi, f->nbits) : f->hi;
    out.mask = &m;
    if (lo >= hi || x->ntotal == 0) {
        out.ntotal = out.ngroups = 0;
        return IVR_OK;
    }
    // sized by the capacity, so that a search after ivr_index_reserve_search allocates nothing until the index grows
    int rc = ivr_reserve({{&x->ids_rows, (size_t)(x->cap / kGroupRows) * sizeof(uint64_t)}});
    if (rc != IVR_OK) return rc;
    {
        IvrProf prof("ids_row_mask", s, (double)x->ntotal * 8 + (double)ngroups * 8);
        hipLaunchKernelGGL(ids_row_mask_kernel, dim3((unsigned)ivr_ceil_div(ngroups, 4)), dim3(256), 0, s, x->ids, x->ntotal, ngroups, lo, hi,
                           f->bits, (uint64_t *)x->ids_rows);
        IVR_LAUNCH_CHECK();
    }
    m.lo = 0;
    m.hi = x->ntotal;
    m.bits = reinterpret_cast<const uint8_t *>((uint64_t *)x->ids_rows);   // bit r & 7 of byte r >> 3 = bit r & 63 of word r >> 6
    m.bit0 = 0;
    return IVR_OK;
}

extern "C" {

int ivr_index_has_ids(ivr_index *x) { return x && x->has_ids ? 1 : 0; }

int ivr_index_get_ids(ivr_index *x, int64_t start, int64_t n, int64_t *out, ivr_stream stream) {
    IVR_REQUIRE(x && (out || n == 0), "ivr_index_get_ids: NULL argument");
    std::lock_guard<std::mutex> lk(x->mu);
    if (!x->has_ids) return ivr_fail(IVR_ERR_STATE, "ivr_index_get_ids: the index is not id-mapped");
    IVR_REQUIRE(start >= 0 && n >= 0 && start + n <= x->ntotal, "ivr_index_get_ids: rows [%lld,%lld) outside [0,%lld)", (long long)start,
                (long long)(start + n), (long long)x->ntotal);
    if (n == 0) return IVR_OK;
    IVR_HIP(hipSetDevice(x->ctx->device));
    IVR_HIP(hipMemcpyAsync(out, x->ids + start, (size_t)n * sizeof(int64_t), hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return IVR_OK;
}

int ivr_index_find_ids(ivr_index *x, const int64_t *keys, int64_t n, int64_t *rows, ivr_stream stream) {
    IVR_REQUIRE(x && ((keys && rows) || n == 0), "ivr_index_find_ids: NULL argument");
    IVR_REQUIRE(n >= 0, "ivr_index_find_ids: n=%lld", (long long)n);
    std::lock_guard<std::mutex> lk(x->mu);
    if (!x->has_ids) return ivr_fail(IVR_ERR_STATE, "ivr_index_find_ids: the index is not id-mapped");
    if (n == 0) return IVR_OK;
    IVR_HIP(hipSetDevice(x->ctx->device));
    hipStream_t s = (hipStream_t)stream;
    IVR_HIP(hipMemsetAsync(rows, 0xff, (size_t)n * sizeof(int64_t), s));         // -1: no row holds the key
    if (x->ntotal == 0) return IVR_OK;
    const int64_t blocks = std::min<int64_t>(ivr_ceil_div(x->ntotal, 256), (int64_t)x->ctx->cu_count * 8);
    IvrProf prof("ids_find", s, (double)x->ntotal * 8, true);
    hipLaunchKernelGGL(ids_find_kernel, dim3((unsigned)blocks), dim3(256), 0, s, x->ids, x->ntotal, keys, n,
                       reinterpret_cast<unsigned long long *>(rows));
    IVR_LAUNCH_CHECK();
    return IVR_OK;
}

}  // extern "C"
