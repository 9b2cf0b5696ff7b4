// Stable external ids (faiss IndexIDMap2 / add_with_ids): what an id-mapped index does with its id table besides carrying it.  The
// table itself (ivr_index::ids, one int64 label per stored row) is allocated, grown, appended to and compacted with the rows in
// search_index.hip; the label of a result is read from it by the final write of each search path (select_topk_kernel<.., OUT_DI_IDS>,
// range_write_kernel<true>).  Here: the pass that turns a filter over stored ids into a row bitmap, so that every masked kernel runs
// as it is, the lookup of rows by id (a scan of the table for a few keys, a hash table from id to lowest row for many), and the two
// entry points that read the table back.
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
// the largest unsigned value, so "none" needs no second pass.  O(keys x ntotal) compares: the path of lookups below
// IVR_FIND_TABLE_MIN_KEYS keys, which need no table built.
__global__ __launch_bounds__(256) void ids_find_kernel(const int64_t *__restrict__ ids, int64_t ntotal, const int64_t *__restrict__ keys,
                                                       int64_t nkeys, unsigned long long *__restrict__ rows) {
    for (int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x; r < ntotal; r += (int64_t)gridDim.x * 256) {
        const int64_t id = ids[r];
        for (int64_t i = 0; i < nkeys; ++i)
            if (keys[i] == id) atomicMin(&rows[i], (unsigned long long)r);
    }
}

// Hash table from stored id to the lowest row that holds it: open addressing with linear probing over a power-of-two number of slots
// >= 2 ntotal (load factor <= 1/2, so every probe sequence ends at an empty slot), empty key -1 (stored ids are >= 0).  The slot of an
// id comes from all of its bits (the 64-bit finaliser of MurmurHash3): sequential ids, and ids that share a large base, spread.
__device__ __forceinline__ uint64_t ids_slot(int64_t id, uint64_t mask) {
    uint64_t h = (uint64_t)id;
    h ^= h >> 33;
    h *= 0xff51afd7ed558ccdull;
    h ^= h >> 33;
    h *= 0xc4ceb9fe1a85ec53ull;
    h ^= h >> 33;
    return h & mask;
}

// One thread per stored row: a 64-bit compare-and-swap claims the first slot of the probe sequence that is empty or already holds the
// id, an atomic minimum lowers that slot's row.  Rows under one id all end in the same slot (a claimed key never changes), so the slot
// holds the lowest of them whatever the order of the threads: what the scan path returns.  keys / rows start as all ones (-1).
__global__ __launch_bounds__(256) void ids_table_build_kernel(const int64_t *__restrict__ ids, int64_t ntotal, unsigned long long *__restrict__ keys,
                                                              unsigned long long *__restrict__ rows, uint64_t mask) {
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= ntotal) return;
    const unsigned long long id = (unsigned long long)ids[r];
    for (uint64_t h = ids_slot((int64_t)id, mask);; h = (h + 1) & mask) {
        const unsigned long long prev = atomicCAS(&keys[h], ~0ull, id);
        if (prev == ~0ull || prev == id) {
            atomicMin(&rows[h], (unsigned long long)r);
            return;
        }
    }
}

// One thread per key: walk the probe sequence to the key or to the first empty slot.  A negative key is no stored id (and -1 is the
// empty marker): -1 without a probe.
__global__ __launch_bounds__(256) void ids_table_find_kernel(const int64_t *__restrict__ tkeys, const unsigned long long *__restrict__ trows,
                                                             uint64_t mask, const int64_t *__restrict__ keys, int64_t nkeys,
                                                             int64_t *__restrict__ rows) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= nkeys) return;
    const int64_t key = keys[i];
    int64_t row = -1;
    if (key >= 0) {
        for (uint64_t h = ids_slot(key, mask);; h = (h + 1) & mask) {
            const int64_t k = tkeys[h];
            if (k == key) row = (int64_t)trows[h];
            if (k == key || k == -1) break;
        }
    }
    rows[i] = row;
}

// the table of x brought up to date with ids[0 .. ntotal) on stream s (ntotal > 0): allocates when the slot count changes
int ids_table_build(ivr_index *x, hipStream_t s) {
    if (x->tab_ok) return IVR_OK;
    int64_t slots = 2;
    while (slots < 2 * x->ntotal) slots <<= 1;
    const size_t bytes = (size_t)slots * 8;
    if (x->tab_keys.bytes != bytes) {
        // exactly the slots of this build, so that the table never holds more than 64 bytes per stored row
        int rc = ivr_release({{&x->tab_keys, 0}, {&x->tab_rows, 0}});
        if (rc == IVR_OK) rc = ivr_reserve({{&x->tab_keys, bytes}, {&x->tab_rows, bytes}});
        if (rc != IVR_OK) return rc;
    }
    x->tab_slots = slots;
    IVR_HIP(hipMemsetAsync(x->tab_keys, 0xff, bytes, s));
    IVR_HIP(hipMemsetAsync(x->tab_rows, 0xff, bytes, s));
    IvrProf prof("ids_table_build", s, (double)x->ntotal * 8 + 4.0 * bytes, true);
    hipLaunchKernelGGL(ids_table_build_kernel, dim3((unsigned)ivr_ceil_div(x->ntotal, 256)), dim3(256), 0, s, x->ids, x->ntotal,
                       reinterpret_cast<unsigned long long *>((int64_t *)x->tab_keys), (unsigned long long *)x->tab_rows, (uint64_t)slots - 1);
    IVR_LAUNCH_CHECK();
    x->tab_ok = true;
    return IVR_OK;
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
    if (x->ntotal > 0 && n >= x->find_table_min) {
        // many keys: the hash table, (re)built first when rows or ids changed since its last build
        const int rc = ids_table_build(x, s);
        if (rc != IVR_OK) return rc;
        IvrProf prof("ids_table_find", s, (double)n * 32, true);
        hipLaunchKernelGGL(ids_table_find_kernel, dim3((unsigned)ivr_ceil_div(n, 256)), dim3(256), 0, s, (const int64_t *)x->tab_keys,
                           (const unsigned long long *)x->tab_rows, (uint64_t)x->tab_slots - 1, keys, n, rows);
        IVR_LAUNCH_CHECK();
        return IVR_OK;
    }
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
