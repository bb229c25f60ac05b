/* lshrs_groups.h - connected components of an edge list, on the device: the C ABI of liblshrs_groups.so, a library of its own
 * beside liblshrs_hip.so (it needs no symbol of that one; from lshrs_hip.h it takes the LSHRS_E_* codes and the conventions:
 * a status of 0, a negative LSHRS_E_* code, or minus a HIP error; nothing thrown across the ABI; every pointer but `stream`
 * is device memory).  lshrs_groups_abi_version() returns 1.
 *
 * ---- the components (csrc/groups.hip; lshrs_amd.group_pairs): a union-find forest `parent` (int32 [n]) over the dense
 * vertices [0, n).  An edge is (a[e], b[e]), undirected, in either orientation; a repeated edge and an edge with a == b change
 * nothing.
 * init: parent[x] = x, one lane per vertex.
 * hook: one lane per edge in a grid-stride loop, the grid sized to the device and not to n_edges.  The lane finds the roots of
 * its two endpoints and hangs the LARGER root under the SMALLER one by a compare-and-swap of the larger root's own entry from
 * itself; on a lost race it goes on from whatever the swap returned.  It may be called any number of times on one `parent`,
 * with slices of one edge list or with several lists: the result is that of one call over all the edges.
 * flatten: parent[x] = the root of x, one lane per vertex; lane x is the only writer of parent[x] and moves it up two levels
 * at a time until it names a root.
 * After flatten parent[x] is the SMALLEST vertex of x's component, in whatever order the lanes ran.
 *
 * Invariants, at every moment of every kernel:
 *   (1) parent[x] <= x.
 *   (2) hook changes the entry of a root only by that compare-and-swap from itself.
 *   (3) every other write to parent[x] stores a vertex that was an ancestor of x when it was read (path halving in hook's
 *       finds, the two-level moves of flatten).  Halving is needed, not optional: without it a path whose edges arrive in
 *       descending order is a chain of depth n and costs n^2 steps.
 *   (4) a vertex that stopped being a root never becomes one again.
 * From (1) every walk towards a root descends strictly, so it ends, and the root of a tree is its smallest vertex; from (2) to
 * (4) two vertices once in one tree stay in one tree, trees are merged only along edges, and when the lane of an edge leaves,
 * its endpoints are in one tree: at the end the trees are the components, whatever the interleaving.
 *
 * Memory model: inside hook every CU reads and writes `parent` in one launch, and the XCDs' L2s are not coherent with each
 * other: every access to `parent` there is an agent-scope relaxed atomic (load, store, compare-and-swap).  Relaxed is enough -
 * a stale value is an earlier ancestor, which (3) allows, and the only decision is the compare-and-swap.  flatten's accesses
 * are the same atomics (a fresh value saves steps; a stale one is still an ancestor); init stores plainly behind the kernel
 * boundary.  No kernel waits for another workgroup; no host synchronisation inside an entry.
 *
 * err (int32[1], or-ed into, never cleared): bit 0 - an endpoint outside [0, n): its edge is skipped before `parent` is
 * touched, the other edges are joined; bit 1 - a lane passed the iteration cap of one of its loops (the proven bound: 2 n + 16
 * steps for an edge of hook, n + 16 for a vertex of flatten) and left: a logic error, `parent` is then not to be used.
 * Status, all decided before anything touches a device: n or n_edges negative: LSHRS_E_BADARG; n above 2^31 - 1:
 * LSHRS_E_TOOLARGE; n == 0 or n_edges == 0: 0, nothing launched and no pointer looked at; else a null or misaligned pointer
 * (parent, err: 4 bytes; a, b: 8 bytes): LSHRS_E_BADARG. */
#ifndef LSHRS_GROUPS_H
#define LSHRS_GROUPS_H

#include "lshrs_hip.h"

#define LSHRS_GROUPS_ABI_VERSION 1
#define LSHRS_CC_ERR_ENDPOINT 0x1 /* err bit 0 */
#define LSHRS_CC_ERR_CAP      0x2 /* err bit 1 */

#ifdef __cplusplus
extern "C" {
#endif

int lshrs_groups_abi_version(void);
int lshrs_cc_init_i32(int32_t* parent, int64_t n, void* stream);
int lshrs_cc_hook_i64(const int64_t* a, const int64_t* b, int64_t n_edges, int32_t* parent, int64_t n, int32_t* err,
                      void* stream);
int lshrs_cc_flatten_i32(int32_t* parent, int64_t n, int32_t* err, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* LSHRS_GROUPS_H */
