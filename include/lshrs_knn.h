/* lshrs_knn.h - the k-nearest-neighbour self-join of liblshrs_hip.so: six entries, additive to ABI 7 and declared beside
 * lshrs_hip.h, whose element codes (LSHRS_SCAN_*), error codes (LSHRS_E_*) and conventions they share.
 *
 * ---- k-NN self-join (csrc/scan.hip; lshrs_amd.exact_knn): the top-k scan (lshrs_scan_topk_*) with the stored rows themselves
 * as the queries.  For every row of [q_begin, q_begin + q_count) the `window` OTHER live rows of corpus of the largest
 * APPROXIMATE cosine: a row is never in its own window (by position), and all m rows are scanned for every query row - the
 * full square, not a triangle: a product would have to feed the window of its row side too, and the windows of a pass's 256
 * rows do not fit in LDS.  The approximate score is the one lshrs_scan_topk_* gives the row for the query row converted to
 * f32, bit for bit (a one-term row - bf16, int8, e4m3fn - is exact in bf16: the query's second term is zero and is neither
 * stored nor multiplied), so lshrs_scan_epsilon bounds it unchanged.
 * out_rows (q_count, window) int64, out_approx (q_count, window) float, out_count (q_count) int32: laid out as
 * lshrs_scan_topk_* leaves them - descending score, equal scores by ascending row, -1 / -inf behind out_count[i] entries.  A
 * dead query row (row_ids < 0) gets count 0, rows -1 and scores -inf.  err bit 4: a live row of zero norm as a query, bit 1:
 * as a row; a dead row sets no bit.
 * The query rows are taken a block at a time, one launch (and one merge) per block on `stream`, the blocks sharing the
 * workspace: qblock = 0 takes the planned block (at most 8192 rows, fewer where the image would pass 256 MiB or the range
 * ends), another multiple of 64 is taken as the block.
 * Status, all decided before anything touches a device: q_count < 0, q_begin < 0 or a range beyond m, window outside
 * [1, lshrs_scan_max_window()], qblock negative or no multiple of 64, ldc < dim, a null or misaligned pointer:
 * LSHRS_E_BADARG; dim > 16384, m >= 2^31, more than 65535 tiles of 64 in a block: LSHRS_E_TOOLARGE; q_count == 0: 0, nothing
 * is launched.  workspace: lshrs_scan_knn_workspace_bytes(q_count, m, dim, window, qblock) bytes at a 16-byte aligned
 * address: the image of one block (16 KiB per tile of 64 rows and chunk of 64 elements; the one-term types use half), a norm
 * per row of the block, (rows of a block) x (its slices of the m rows) x window 8-byte items - the largest over the blocks of
 * the call - and 16.  No host synchronisation. */
#ifndef LSHRS_KNN_H
#define LSHRS_KNN_H

#include "lshrs_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

int64_t lshrs_scan_knn_workspace_bytes(int32_t q_count, int64_t m, int32_t dim, int32_t window, int32_t qblock);
int lshrs_scan_knn_f32(const float* corpus, int64_t m, int64_t ldc, int32_t dim, const int64_t* row_ids, int64_t q_begin,
                       int32_t q_count, int32_t window, int32_t qblock, int64_t* out_rows, float* out_approx, int32_t* out_count,
                       void* workspace, int32_t* err, void* stream);
int lshrs_scan_knn_bf16(const uint16_t* corpus, int64_t m, int64_t ldc, int32_t dim, const int64_t* row_ids, int64_t q_begin,
                       int32_t q_count, int32_t window, int32_t qblock, int64_t* out_rows, float* out_approx, int32_t* out_count,
                       void* workspace, int32_t* err, void* stream);
int lshrs_scan_knn_f16(const uint16_t* corpus, int64_t m, int64_t ldc, int32_t dim, const int64_t* row_ids, int64_t q_begin,
                       int32_t q_count, int32_t window, int32_t qblock, int64_t* out_rows, float* out_approx, int32_t* out_count,
                       void* workspace, int32_t* err, void* stream);
int lshrs_scan_knn_i8(const int8_t* corpus, int64_t m, int64_t ldc, int32_t dim, const int64_t* row_ids, int64_t q_begin,
                       int32_t q_count, int32_t window, int32_t qblock, int64_t* out_rows, float* out_approx, int32_t* out_count,
                       void* workspace, int32_t* err, void* stream);
int lshrs_scan_knn_f8e4m3(const uint8_t* corpus, int64_t m, int64_t ldc, int32_t dim, const int64_t* row_ids, int64_t q_begin,
                       int32_t q_count, int32_t window, int32_t qblock, int64_t* out_rows, float* out_approx, int32_t* out_count,
                       void* workspace, int32_t* err, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* LSHRS_KNN_H */
