/* lshrs_graph.h - from an unordered list of undirected pairs to per-row neighbour lists, and the best k of every list, on the
 * device: the C ABI of liblshrs_graph.so, a library of its own beside liblshrs_hip.so and liblshrs_groups.so (it needs no
 * symbol of either; from lshrs_hip.h it takes the LSHRS_E_* codes and the conventions: a status of 0, a negative LSHRS_E_*
 * code, or minus a HIP error; nothing thrown across the ABI; every pointer but `stream` is device memory).
 * lshrs_graph_abi_version() returns 1.
 *
 * ---- the adjacency (csrc/graph.hip; lshrs_amd._knn_join.pair_adjacency): the pairs (a[p], b[p]) over the rows [0, n_rows)
 * as one list per row, in CSR form.  Three steps, the middle one the caller's:
 * degree: one lane per pair, degree[a[p]] += 1 and degree[b[p]] += 1 (int32 [n_rows], zeroed by the caller).
 * prefix: row_off (int64 [n_rows + 1]) = the exclusive prefix sum of degree and its total (torch.cumsum).
 * fill:   one lane per pair; b[p] goes into the slot of row a[p]'s list [row_off[a], row_off[a + 1]) that an atomic add on
 * cursor[a] reserves (int32 [n_rows], zeroed by the caller), and a[p] into row b[p]'s list likewise.  nbr has 2 n_pairs
 * entries.  A slot at or beyond the end of its list, or outside nbr, is not written: that happens only when row_off does not
 * belong to these pairs, and no store leaves nbr.
 * A pair with an endpoint outside [0, n_rows) sets bit 0 of err (LSHRS_GRAPH_ERR_ENDPOINT), a pair with a[p] == b[p] bit 1
 * (LSHRS_GRAPH_ERR_LOOP); such a pair adds nothing in degree and is skipped by fill (which reports nothing: it has no err).
 * THE ORDER INSIDE A LIST is whatever the lanes' arrival made it, and differs from run to run: nothing downstream may depend
 * on it, and select does not.
 * The counters are int32 in global memory and every add is a device-scope atomicAdd, one per lane and endpoint.  Lanes of a
 * wave often add to the same word (consecutive raw pairs of a bucket share an endpoint); combining them inside the wave first
 * is the build -DLSHRS_GRAPH_COMBINE=1, measured and not shipped (profiles/lsh_knn.json).
 *
 * ---- the selection (lshrs_amd._knn_join.select_neighbors): row r owns the entries [row_off[r], row_off[r + 1]) of nbr
 * (int64) and of scores (float32), both of `total` entries.  The id of an entry is row_ids[nbr[e]] (row_ids: int64 [n_ids]),
 * or nbr[e] itself where row_ids is NULL.  Per row the best min(k, len) entries go to out_ids [n_rows][k] / out_scores
 * [n_rows][k] in the order of lshrs_topk_desc_f32 - the orderable key of a score (csrc/lshrs_rows.h): descending, +0.0 ahead of
 * -0.0, NaN last - with EQUAL KEYS BY ASCENDING ID, not by position: the answer is the same for every order of a list.  The
 * tail of an output row is -1 / NaN (0x7fc00000); out_count[r] = min(k, len).  A list longer than lshrs_graph_max_list() gets
 * out_count[r] = -1 and nothing else written: its caller ranks it.
 * Two launches over the same rows, neither reading what the other writes: lists of at most lshrs_graph_wave_list() entries
 * are sorted by ONE WAVE each, in that wave's own slice of LDS, with no workgroup barrier and four rows per workgroup; longer
 * lists by one workgroup each through LDS, a grid sized to the device walking the rows.  A sort item is 16 bytes - key, id,
 * position - so lshrs_graph_max_list() = 4096 items are the 64 KiB two workgroups of a CU can hold at a time.
 * err (int32[1], or-ed into): bit 0 (LSHRS_GRAPH_ERR_RANGE) - a row's list does not lie within [0, total]: nothing of it is
 * read, the row gets out_count 0 and the padding; bit 1 (LSHRS_GRAPH_ERR_ENTRY) - with row_ids, an entry outside [0, n_ids):
 * row_ids is not read for it and it goes under the id -1.
 *
 * Status, all decided before anything touches a device: a negative count, k < 1: LSHRS_E_BADARG; n_rows or n_pairs above
 * 2^31 - 1: LSHRS_E_TOOLARGE; zero work (n_pairs == 0 or n_rows == 0 for degree and fill, n_rows == 0 for select): 0, nothing
 * launched and no pointer looked at; else a null or misaligned pointer (int64: 8 bytes, int32 and float: 4; row_ids may be
 * NULL; nbr and scores may be NULL when total == 0): LSHRS_E_BADARG.  No host synchronisation; no kernel waits for another
 * workgroup, and what one launch writes is read by the next launch only; every loop has a bound that follows from the
 * arguments. */
#ifndef LSHRS_GRAPH_H
#define LSHRS_GRAPH_H

#include "lshrs_hip.h"

#define LSHRS_GRAPH_ABI_VERSION 1
#define LSHRS_GRAPH_ERR_ENDPOINT 0x1 /* degree: err bit 0 */
#define LSHRS_GRAPH_ERR_LOOP     0x2 /* degree: err bit 1 */
#define LSHRS_GRAPH_ERR_RANGE    0x1 /* select: err bit 0 */
#define LSHRS_GRAPH_ERR_ENTRY    0x2 /* select: err bit 1 */

#ifdef __cplusplus
extern "C" {
#endif

int lshrs_graph_abi_version(void);
int32_t lshrs_graph_max_list(void);
int32_t lshrs_graph_wave_list(void);
int lshrs_graph_degree_i64(const int64_t* a, const int64_t* b, int64_t n_pairs, int64_t n_rows, int32_t* degree, int32_t* err,
                           void* stream);
int lshrs_graph_fill_i64(const int64_t* a, const int64_t* b, int64_t n_pairs, int64_t n_rows, const int64_t* row_off,
                         int32_t* cursor, int64_t* nbr, void* stream);
int lshrs_graph_select_f32(const int64_t* nbr, const float* scores, const int64_t* row_off, int64_t n_rows, int64_t total,
                           const int64_t* row_ids, int64_t n_ids, int32_t k, int64_t* out_ids, float* out_scores,
                           int32_t* out_count, int32_t* err, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* LSHRS_GRAPH_H */
