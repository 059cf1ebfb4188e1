// CPU check of the BFS engines' chunk verdict (ac-solver-caltech_amd/csrc/acx_bfs_verdict.h)
// against a plain sequential restatement of the reference's loop (breadth_first.py:84-95): child
// by child, the raising move or the success where it stands, the budget test after each parent.
// Stand-alone: no libacx, no GPU (tests/test_bfs_verdict_host.py builds and runs it, and holds
// _sharded_bfs.py's _chunk_verdict to the table this prints).
//   verdict_check  ->  one row "P succ err cut kind looked last" per case (-1: none), then
//                      "ok <cases>" and exit 0, or "FAIL ..." lines and exit 1
// Cases: P in {1, 2, 3}; first success seq and first raising seq each in {none} + [0, 12 P);
// cut parent in {none} + [0, P).
#include <cstdint>
#include <cstdio>

#include "acx_bfs_verdict.h"

using acx::bfs::NO_SEQ;
using acx::bfs::Verdict;

// the reference, one child at a time.  `err` is the first child whose move raises (the reference
// never gets to look at it), `succ` the first with total length 2, `cut` the first parent after
// which len(tree_nodes) >= max_nodes.
static Verdict sequential(uint32_t succ, uint32_t err, uint32_t cut, uint32_t P) {
    uint32_t looked = 0;
    for (uint32_t p = 0; p < P; ++p) {
        for (uint32_t a = 0; a < 12; ++a) {
            const uint32_t s = 12 * p + a;
            if (s == err) return {ACX_BFS_MOVE_ERROR, looked, p};  // ACMove raises (utils.py:264-266)
            ++looked;
            if (s == succ) return {ACX_BFS_FOUND, looked, p};  // breadth_first.py:84-85
        }
        if (cut != NO_SEQ && p >= cut) return {ACX_BFS_BUDGET, looked, p};  // :91-95
    }
    return {0, looked, P - 1};
}

static long show(uint32_t v) { return v == NO_SEQ ? -1 : (long)v; }

int main() {
    int fails = 0;
    long cases = 0;
    for (uint32_t P = 1; P <= 3; ++P)
        for (uint32_t si = 0; si <= 12 * P; ++si)
            for (uint32_t ei = 0; ei <= 12 * P; ++ei)
                for (uint32_t ci = 0; ci <= P; ++ci) {
                    const uint32_t succ = si ? si - 1 : NO_SEQ, err = ei ? ei - 1 : NO_SEQ, cut = ci ? ci - 1 : NO_SEQ;
                    const Verdict want = sequential(succ, err, cut, P);
                    const Verdict got = acx::bfs::chunk_verdict(succ, err, cut, P);
                    ++cases;
                    if (got.kind != want.kind || got.looked != want.looked || got.last_p != want.last_p) {
                        if (++fails <= 20)
                            std::printf("FAIL P %u succ %ld err %ld cut %ld: got (%d, %u, %u), the reference (%d, %u, %u)\n", P,
                                        show(succ), show(err), show(cut), got.kind, got.looked, got.last_p, want.kind,
                                        want.looked, want.last_p);
                        continue;
                    }
                    std::printf("%u %ld %ld %ld %d %u %u\n", P, show(succ), show(err), show(cut), want.kind, want.looked,
                                want.last_p);
                }
    if (fails) return 1;
    std::printf("ok %ld\n", cases);
    return 0;
}
