// acx_bfs_verdict.h -- the reference's decision for a run of consecutive parents (a chunk of the
// device BFS, a round of the batched BFS), from what the expansion and the commit found in it.
// Host / device like acx_key.h: the device engines call it (bfs_close_kernel, mbfs_kernel's decide
// phase), tests/verdict_check.cpp compiles it with the host compiler against a child-by-child
// restatement of breadth_first.py:84-95, and _sharded_bfs.py's _chunk_verdict is held to the same
// table.
#pragma once
#include <stdint.h>

#include "acx.h"
#include "acx_key.h"

namespace acx {
namespace bfs {

constexpr uint32_t NO_SEQ = 0xffffffffu;  // no such child / no such parent

struct Verdict {
    int32_t kind;     // ACX_BFS_MOVE_ERROR, ACX_BFS_FOUND, ACX_BFS_BUDGET, or 0: the search goes on
    uint32_t looked;  // children of the run the reference looked at, in sequential order
    uint32_t last_p;  // the last parent it counts as expanded
};

// succ, err: the first child (seq = 12 * parent + action) with total length 2 / whose move raised;
// cut_p: the first parent after which len(tree_nodes) >= max_nodes; NO_SEQ where there is none.
// The reference walks child by child: the raising move ends the search where it stands (the
// child is not looked at), the success child where it stands (it is), the budget test comes
// after each parent's 12 children.  So: a raising child not after the first success and not
// after the cut parent; else a success not after the cut parent; else the cut; else go on.
// (A move either raises or returns a child, so err == succ only as NO_SEQ; the raise is taken
// first there, as the reference would.)
ACX_HD inline Verdict chunk_verdict(uint32_t succ, uint32_t err, uint32_t cut_p, uint32_t P) {
    if (err != NO_SEQ && err <= succ && err / 12 <= cut_p) return {ACX_BFS_MOVE_ERROR, err, err / 12};
    if (succ != NO_SEQ && succ / 12 <= cut_p) return {ACX_BFS_FOUND, succ + 1, succ / 12};
    if (cut_p != NO_SEQ) return {ACX_BFS_BUDGET, (cut_p + 1) * 12u, cut_p};
    return {0, P * 12u, P - 1};
}

}  // namespace bfs
}  // namespace acx
