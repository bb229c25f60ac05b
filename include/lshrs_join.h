/* lshrs_join.h - the LSH self-join of liblshrs_hip.so: three entries, additive to ABI 7 and declared beside lshrs_hip.h, whose
 * error codes (LSHRS_E_*) and conventions they share.
 *
 * ---- LSH self-join (csrc/join.hip; lshrs_amd.lsh_pairs_above): the candidate pairs of a banded LSH index - two members that
 * share a bucket in at least min_collisions bands - out of ONE bucket segment, each pair once, with the number of bands it
 * collides in.  The segment: n_codes buckets sorted by codes[g] = band << (8 * band_bytes) | key; bucket g holds the entries
 * [offsets[g], offsets[g + 1]) of the member list, every member at most once per bucket.  member_rows (n_members =
 * offsets[n_codes] entries) gives for every entry of the member list the row of the corpus that holds its vector.  A bucket
 * COUNTS when it has 2 .. max_bucket entries; the others count in no role.
 *
 * The row map (the workspace: int32 [n_rows][num_bands], lshrs_join_workspace_bytes(n_rows, num_bands) bytes at a 16-byte
 * aligned address) holds for every (row, band) the counted bucket the row is a member of, -1 where there is none.
 * rowmap: presets the map to -1 and fills it, one lane per entry of the member list (its bucket by bisection on offsets), each
 * cell by a compare-and-swap from -1.  err (int32[1], or-ed into, never cleared): bit 0 - a row is in two different counted
 * buckets of one band (an id indexed under two signatures and never deleted: the join refuses it, the map is then not to be
 * used); bit 1 - a code whose band lies outside [0, num_bands); bit 8 - an entry of member_rows is negative (a member
 * without a stored vector); bit 9 - an entry is at or beyond n_rows.  Every entry is checked, counted bucket or not; an entry
 * with bit 8 or 9 writes nothing.
 * emit: the raw pairs are the len (len - 1) / 2 pairs of every counted bucket, numbered through pair_prefix (int64
 * [n_codes + 1]: the exclusive prefix sum of those counts - 0 for a bucket that does not count - and their total).  One lane
 * per raw pair of [raw_begin, raw_begin + raw_count): its bucket by bisection on pair_prefix, its two entries from the
 * triangular index (a double-precision root corrected by integer steps: exact), the two rows of the map compared band by
 * band.  collisions = the bands where both rows name the same bucket; the pair goes out only from the FIRST such band's
 * bucket and only when collisions >= min_collisions: every candidate pair exactly once, nothing sorted.  Output as
 * lshrs_scan_pairs_*: a wave reserves the slots of its hits with one 64-bit add on `total`, which counts hits beyond
 * `capacity` too and is NOT reset by the entry (the launches of a sliced join add up: the caller zeroes it); out_a / out_b
 * (int64, row numbers, a < b) and out_hits (int32, collisions) get the hits that fit, in no particular order; no output
 * pointer is needed for a capacity of 0.  An entry whose rows are outside [0, n_rows) or equal is skipped.
 * Status, all decided before anything touches a device: a null or misaligned pointer, n_codes, n_members, n_rows, raw_begin,
 * raw_count or capacity negative, band_bytes outside [1, 6], num_bands < 1, max_bucket < 2, min_collisions outside
 * [1, num_bands]: LSHRS_E_BADARG; n_codes or n_rows above 2^31 - 1, a map beyond 2^40 cells, raw_count > 2^31:
 * LSHRS_E_TOOLARGE; n_codes == 0, n_members == 0 (rowmap: the map is still preset) or raw_count == 0: 0.  No host
 * synchronisation; no kernel waits for another workgroup. */
#ifndef LSHRS_JOIN_H
#define LSHRS_JOIN_H

#include "lshrs_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

int64_t lshrs_join_workspace_bytes(int64_t n_rows, int32_t num_bands);
int lshrs_join_rowmap_i64(const int64_t* codes, const int64_t* offsets, int64_t n_codes, int32_t band_bytes, int32_t num_bands,
                          const int64_t* member_rows, int64_t n_members, int64_t n_rows, int64_t max_bucket, void* workspace,
                          int32_t* err, void* stream);
int lshrs_join_emit_i64(const int64_t* offsets, const int64_t* pair_prefix, int64_t n_codes, const int64_t* member_rows,
                        int64_t n_rows, int32_t num_bands, const void* workspace, int64_t raw_begin, int64_t raw_count,
                        int32_t min_collisions, int64_t capacity, int64_t* out_a, int64_t* out_b, int32_t* out_hits,
                        uint64_t* total, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* LSHRS_JOIN_H */
