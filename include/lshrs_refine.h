/* lshrs_refine.h - one local-join round over a k-NN graph, on the device: from a neighbour table to an undirected edge list, and
 * from an adjacency to every row's rows AT DISTANCE ONE OR TWO, each once.  The C ABI of liblshrs_refine.so, a library of its own
 * beside liblshrs_hip.so, liblshrs_groups.so and liblshrs_graph.so (it needs no symbol of any of them; from lshrs_hip.h it takes
 * the LSHRS_E_* codes and the conventions: a status of 0, a negative LSHRS_E_* code, or minus a HIP error; nothing thrown across
 * the ABI; every pointer but `stream` is device memory).  lshrs_refine_abi_version() returns 1.
 *
 * ---- the edges (csrc/refine.hip; lshrs_amd._refine.graph_edges): graph is int64 [n_rows][k_in], row positions, -1 for no
 * entry.  One lane per entry (r, c) writes keep[r * k_in + c] (uint8, 0 or 1: every byte is written).  The entry g = graph[r][c]
 * is kept iff  g >= 0,  no earlier column of row r holds g (the first occurrence counts),  and not both g < r and row g lists r
 * (of a mutual pair only the lower row's entry survives).  The kept (r, g) are every undirected pair of the table ONCE;
 * compacting them by keep is the caller's (torch.nonzero), and they go to lshrs_graph_degree_i64 / _fill_i64 as they are.
 * err (int32[1], or-ed into): bit 0 (LSHRS_REFINE_ERR_OUTSIDE) - an entry outside [-1, n_rows); bit 1 (LSHRS_REFINE_ERR_SELF) -
 * g == r.  Such an entry is not kept and nothing is read through it.
 *
 * ---- the expansion (lshrs_amd._refine.expand_candidates): nbr (int64, `total` entries) / row_off (int64 [n_rows + 1]) is an
 * adjacency in CSR form, what the fill of lshrs_graph.h leaves.  A(r): the list of r; deg(r): its length; M(r), the MIDPOINTS of
 * r: every m in A(r) with deg(m) <= max_degree (all of A(r) where max_degree <= 0: no cap); C(r): the union of A(r) and of A(m)
 * over all m in M(r), without r, each row once.  A row over the cap stays a candidate of its neighbours - it only stops being
 * a midpoint - so C(r) always holds A(r).
 * Two launches over the same rows, the step between them the caller's, as degree / prefix / fill are:
 * count:  cand_count[r] (int32 [n_rows]) = |C(r)|, or -1 where the row is beyond the device's tiers (below): the caller expands
 *         such a row itself, and puts its length in before the prefix.
 * prefix: cand_off (int64 [n_rows + 1]) = the exclusive prefix sum of the counts and their total, cand_total.
 * write:  C(r) into cand[cand_off[r] .. cand_off[r + 1]) (int64, cand_total entries); the rows the count left at -1 are not
 *         touched.  A slot at or beyond the end of its list is not written and sets err bit 0: that happens only when cand_off
 *         does not belong to this adjacency, and no store leaves cand.
 * THE ORDER INSIDE A LIST is whatever the hardware made it, and differs from run to run: nothing downstream may depend on it.
 * De-duplication is an open-addressing hash set of int32 row numbers in LDS: insertion is an LDS compare-and-swap, linear
 * probing, bounded by the table's size.  The TIER of a row is decided by its BOUND  U(r) = deg(r) + the sum of deg(m) over m in
 * M(r),  which both launches compute first, not by the unknown |C(r)|; a row's table has at least 2 U(r) slots and can never
 * fill up.  U(r) <= lshrs_refine_wave_set() = 1024: ONE WAVE per row in that wave's own slice of LDS (8 KiB), four rows per
 * workgroup, no workgroup barrier.  Up to lshrs_refine_max_set() = 8192: one workgroup per row, a table of 64 KiB, on a grid
 * sized to the device that walks the rows - two such workgroups' tables fit a CU's LDS together.  Beyond: -1.
 * err (int32[1], or-ed into): bit 0 (LSHRS_REFINE_ERR_RANGE) - a list of nbr that does not lie within [0, total] (nothing of it
 * is read: it counts as empty), a list of cand outside [0, cand_total] (nothing of it is written) or too short for its row;
 * bit 1 (LSHRS_REFINE_ERR_ENTRY) - an entry of nbr outside [0, n_rows): it is skipped, as candidate and as midpoint.  No load or
 * store leaves the arrays.
 *
 * Status, all decided before anything touches a device: a negative count: LSHRS_E_BADARG; n_rows above 2^31 - 1, or n_rows *
 * k_in above it: LSHRS_E_TOOLARGE; zero work (n_rows == 0 or k_in == 0 for the edges, n_rows == 0 for count and write): 0,
 * nothing launched and no pointer looked at; else a null or misaligned pointer (int64: 8 bytes, int32: 4; nbr may be NULL when
 * total == 0, cand when cand_total == 0): LSHRS_E_BADARG.  No host synchronisation; no kernel waits for another workgroup, and
 * what one launch writes is read by the next launch only; every loop has a bound that follows from the arguments. */
#ifndef LSHRS_REFINE_H
#define LSHRS_REFINE_H

#include "lshrs_hip.h"

#define LSHRS_REFINE_ABI_VERSION 1
#define LSHRS_REFINE_ERR_OUTSIDE 0x1 /* edges: err bit 0 */
#define LSHRS_REFINE_ERR_SELF    0x2 /* edges: err bit 1 */
#define LSHRS_REFINE_ERR_RANGE   0x1 /* count, write: err bit 0 */
#define LSHRS_REFINE_ERR_ENTRY   0x2 /* count, write: err bit 1 */

#ifdef __cplusplus
extern "C" {
#endif

int lshrs_refine_abi_version(void);
int32_t lshrs_refine_wave_set(void);
int32_t lshrs_refine_max_set(void);
int lshrs_refine_edges_i64(const int64_t* graph, int64_t n_rows, int32_t k_in, uint8_t* keep, int32_t* err, void* stream);
int lshrs_refine_expand_count_i64(const int64_t* nbr, const int64_t* row_off, int64_t n_rows, int64_t total, int32_t max_degree,
                                  int32_t* cand_count, int32_t* err, void* stream);
int lshrs_refine_expand_write_i64(const int64_t* nbr, const int64_t* row_off, int64_t n_rows, int64_t total, int32_t max_degree,
                                  const int64_t* cand_off, int64_t* cand, int64_t cand_total, int32_t* err, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* LSHRS_REFINE_H */
