// What the inverted-file indexes share on the device, and the int8 operand helpers of the v_mfma_i32_16x16x64_i8 scans.
//   ListRows     the list store of a coded inverted-file index (search_ivfpq.hip, search_ivfsq.hip): offsets, padded groups, labels,
//                the whole of _set_lists; defined in search_lists.hip
//   list_run     the rows of a list, for the list-major scans (search_ivf.hip, search_ivfsq.hip) over the probe tables (ProbeTables,
//                search_internal.h; built and selected from in search_lists.hip)
//   sq_frag, sq_combine, SQ_NO_CONTRACT, i32x4: the int8 scans (search_sq.hip, search_ivfsq.hip; search_pqfs.hip for the pragma)
// No kernel is defined here: an object emits only the kernels it launches.  Not part of the C ABI.
#pragma once
#include "ivr_common.h"
#include "search_internal.h"

#include <functional>
#include <vector>

// The list store of a coded inverted-file index: the codes ordered by list, every list padded to whole 64-row groups.  List l owns
// the groups [goff[l], goff[l + 1]), goff = the exclusive prefix of ceil(size / 64), and row i of the list has the packed position
// 64 goff[l] + i; ids[position] is the row's label, -1 on a pad row.  Whatever the layout inside, a group is group_words 16-byte
// words; the index supplies them, its pack and unpack kernels and its scan.
struct ListRows {
    ivr_ctx *ctx = nullptr;
    int nlist = 0;
    int64_t ntotal = 0, ngroups = 0;
    std::mutex mu;
    DevBuf<uint4> data;                  // [ngroups][group_words]
    DevBuf<int64_t> ids;                 // [ngroups * 64]: the label of every packed position, -1 on a pad row
    DevBuf<int64_t> offs;                // [nlist + 1] list_off (rows in front of each list), then [nlist + 1] goff (groups in front of it)
    std::vector<int64_t> by_size;        // HOST [nlist + 1]: rows or groups of the p longest lists
    int64_t chunk_slots = kIvfChunkSlots;        // key slots of a chunk of queries (environment, read at creation; tests)
    const int64_t *list_off() const { return offs; }
    const int64_t *goff() const { return (const int64_t *)offs + nlist + 1; }
    // an empty store of nlist lists; chunk_slots from the environment variable chunk_slots_env
    int init(ivr_ctx *c, int lists, const char *chunk_slots_env);
    // Replace the content by n list-ordered rows (list l = rows list_off[l] .. list_off[l + 1]).  what: the caller's entry point,
    // for the messages.  A refused argument leaves the store as it was.  Then: wait for the device (a search in flight still
    // reads the lists), empty the store, reserve data and ids, upload the offsets, pack(ngroups) launches the index's pack kernel
    // (not called for 0 groups); when a step fails the store stays empty.  by_size counts rows (by_rows) or groups
    int set_lists(const char *what, const void *codes, const int64_t *src_ids, const int64_t *list_off, int64_t n, int64_t group_words,
                  bool by_rows, const std::function<void(int64_t)> &pack);
    int reset(const char *what);
    // the checks of _get_codes for rows [start, start + n) under the lock, then unpack() launches the index's unpack kernel
    int get_codes(const char *what, int64_t start, int64_t n, const void *codes, const int64_t *out_ids, const std::function<void()> &unpack);
};

namespace {

// rows of list l, clipped to the stored rows
__device__ __forceinline__ void list_run(const int64_t *__restrict__ list_off, int64_t l, int64_t ntotal, int64_t &r0, int64_t &r1) {
    r0 = min(max(list_off[l], (int64_t)0), ntotal);
    r1 = min(max(list_off[l + 1], r0), ntotal);
}

// ---- int8 operands -----------------------------------------------------------------------------------------------------------------
typedef int i32x4 __attribute__((ext_vector_type(4)));

// The definitions count float32 roundings.  The build contracts a * b + c into one fused multiply-add, and __fmul_rn / __fadd_rn are
// the plain operators in this toolchain's headers, so the kernels that evaluate a definition turn contraction off for their body and write the operators out (the pragma is lexical: it
// does not reach into an inlined function).  Division is correctly rounded by default
#define SQ_NO_CONTRACT _Pragma("clang fp contract(off)")

__device__ __forceinline__ i32x4 sq_frag(const uint4 &v) { return __builtin_bit_cast(i32x4, v); }
// 128 acc_h + acc_l; unsigned so that an intermediate beyond int32 wraps (the sum itself always fits)
__device__ __forceinline__ int32_t sq_combine(int h, int l) { return (int32_t)(128u * (uint32_t)h + (uint32_t)l); }

}  // namespace
