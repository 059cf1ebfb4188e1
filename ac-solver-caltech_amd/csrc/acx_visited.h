// acx_visited.h -- the visited set of the BFS engines: an open-addressing hash table in buckets of
// 8 entries (one 64-B line per probe),
//     entry = epoch << 58 | code << 24 | 24-bit fingerprint of the state's key hash.
// A code names a node, or a child of the running chunk / round, and orders as the reference's
// sequential order does; the engine says how a code is turned into that state's key (codes
// < 2^34).  An entry of another epoch (an earlier search on the same workspace) is an empty slot,
// so a search does not clear the table (it did: a 512 MB memset per 10^7-node search); the table
// is cleared only when the 6-bit epoch wraps (next_epoch).
//
// acx_bfs.hip, acx_mbfs.hip and acx_mgreedy.hip insert with insert() below (the batched engines
// through the table view of acx_batch.h).  acx_greedy.hip shares the bucket and
// fingerprint format only: its entries are (id + 1) << 24 | fingerprint without an epoch, and
// its read-only probe and CAS-only commit follow a protocol of their own (ids >= lo are skipped).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace acx {
namespace visited {

constexpr int BUCKET = 8;  // table entries per bucket (64 B)
constexpr uint32_t FP_MASK = 0xffffffu;
constexpr int CODE_SHIFT = 24;
constexpr uint64_t CODE_MASK = (1ull << 34) - 1;
constexpr int EP_SHIFT = 58;
constexpr int EPOCHS = 64;
constexpr uint64_t NO_CODE = ~0ull;

__host__ __device__ __forceinline__ uint32_t fp_of(uint64_t hash) { return (uint32_t)(hash >> 40); }
// ep: the search's epoch, already shifted (next_epoch)
__host__ __device__ __forceinline__ uint64_t entry(uint64_t ep, uint64_t code, uint32_t fp) {
    return ep | (code << CODE_SHIFT) | fp;
}
__host__ __device__ __forceinline__ uint64_t entry_code(uint64_t v) { return (v >> CODE_SHIFT) & CODE_MASK; }
__host__ __device__ __forceinline__ uint32_t entry_fp(uint64_t v) { return (uint32_t)v & FP_MASK; }
__host__ __device__ __forceinline__ bool entry_live(uint64_t v, uint64_t ep) { return (v >> EP_SHIFT) == (ep >> EP_SHIFT); }
// the same entry naming another code (mbfs: a round code becomes the node's index)
__host__ __device__ __forceinline__ uint64_t entry_recode(uint64_t v, uint64_t code) {
    return (v & ~(CODE_MASK << CODE_SHIFT)) | (code << CODE_SHIFT);
}

enum Outcome : int {
    FULL = 0,  // the probe walked every bucket (cannot happen at load <= 1/2)
    SEEN = 1,  // an earlier occurrence of the state (a smaller code) holds the entry
    HELD = 2,  // this child holds the state's entry
};

// Probe / claim / join for the child `code` (its key's hash is `hash`).  An empty slot is claimed
// by CAS; an entry of an equal state is taken by atomicMin, so whatever order the lanes run in,
// the first occurrence in code order ends up holding it, and a child that replaces a later one is
// given that child's code to tell it so (no one re-reads the table to learn who survived).
// An entry only goes empty -> one state's code -> a smaller code of the same state.
//   Table    where the buckets are: Index type, buckets(), first(hash), next(b), bucket(b), and
//            load(bucket, e[8]) -- how a bucket line is read (see each engine's comment on why
//            its reads are safe);
//   key_eq   key_eq(c): does the state named by code c have this key (the engine knows where the
//            keys live; a predicate, not an address, so that each read keeps its address space);
//   on_held  on_held(slot, displaced), called once when the result is HELD: the index of the
//            entry in the table, and the code of the later child whose entry this one took, or
//            NO_CODE.  What to do with them (mark that child lost, keep the slot) is the
//            engine's.  They are handed over where the entry is taken and not returned: as
//            return values they stay live across the probe loop, which cost mbfs_kernel<3> two
//            VGPRs (96 -> 98, one allocation granule, 4 workgroups per CU instead of 5).
template <class Table, class KeyEq, class OnHeld>
__device__ __forceinline__ Outcome insert(const Table& tb, uint64_t ep, uint64_t code, uint64_t hash, KeyEq key_eq,
                                          OnHeld on_held) {
    using Index = typename Table::Index;
    const uint32_t fp = fp_of(hash);
    const uint64_t my = entry(ep, code, fp);
    Outcome r = FULL;
    Index b = tb.first(hash);
    for (Index it = 0; it < tb.buckets() && r == FULL; ++it, b = tb.next(b)) {
        uint64_t* bk = tb.bucket(b);
        uint64_t e[BUCKET];
        tb.load(bk, e);
#pragma unroll
        for (int j = 0; j < BUCKET && r == FULL; ++j) {
            uint64_t v = e[j];
            if (!entry_live(v, ep)) {  // empty in this search
                const uint64_t old = atomicCAS((unsigned long long*)(bk + j), (unsigned long long)v,
                                               (unsigned long long)my);
                if (old == v) {
                    on_held(b * BUCKET + j, NO_CODE);
                    r = HELD;
                    break;
                }
                v = old;  // claimed meanwhile: a value of this search
            }
            if (entry_fp(v) != fp) continue;
            const uint64_t vc = entry_code(v);
            if (!key_eq(vc)) continue;
            if (vc < code) {  // a node, or an earlier child
                r = SEEN;
                break;
            }
            const uint64_t old = atomicMin((unsigned long long*)(bk + j), (unsigned long long)my);
            if (old < my) r = SEEN;
            else {  // replaced a later child
                on_held(b * BUCKET + j, entry_code(old));
                r = HELD;
            }
        }
    }
    return r;
}

// the next search's epoch (shifted) on a reusable table of `bytes` bytes; the table is cleared,
// asynchronously on `st`, when the epoch wraps: once every 63 searches.  `epoch` is the last
// search's (0: a table that is all zero).  false: the clear could not be enqueued.
static inline bool next_epoch(int& epoch, uint64_t* table, size_t bytes, hipStream_t st, uint64_t& ep) {
    if (++epoch == EPOCHS) {
        if (hipMemsetAsync(table, 0, bytes, st) != hipSuccess) return false;
        epoch = 1;
    }
    ep = (uint64_t)epoch << EP_SHIFT;
    return true;
}

}  // namespace visited
}  // namespace acx
