/* mmr.h -- C ABI of the MI355X-native CLIP encode + cosine top-k hot path.
 *
 * Drop-in boundary.  The reference has no FFI of its own: its scripts
 * call a Python object API (`clip.load(...)` -> model.encode_image / encode_text / model(...),
 * reference code/test_clip.py:6-16, code/search_image.py:132,156,335) and plain tensor
 * expressions for scoring/ranking (code/search_image.py:107, code/utils.py:17).  This header is
 * what a Python shim binds with ctypes to replace that path; INTEGRATION.md shows the stub.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer (tensor.data_ptr()) unless named *_host;
 *   - `stream` is a hipStream_t passed as void* (torch.cuda.current_stream().cuda_stream);
 *   - no allocation, no synchronisation inside: the caller owns outputs and workspace, calls
 *     are asynchronous on `stream` and are hipGraph-capturable;
 *   - return 0 on success or a negative errno-style code; mmr_last_error() gives the text
 *     (thread-local).  Arguments are validated on the host BEFORE any launch.
 */
#ifndef MMR_H
#define MMR_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* MMR_F16 (IEEE fp16): accepted by every similarity / ranking entry below wherever MMR_BF16 is, with the same contract,
 * the same workspace plan and the same cost (fp16 x fp16 products are exact in the fp32 MFMA accumulator, like bf16's; the
 * hi / split arguments are ignored as for bf16), and as the OUTPUT dtype of the encoders (mmr_tower_forward,
 * mmr_vit_encode_image, mmr_text_encode, mmr_bert_forward*).  Encoder inputs, weights and preprocess outputs are never
 * fp16. */
typedef enum { MMR_F32 = 0, MMR_BF16 = 1, MMR_F16 = 2 } mmr_dtype;

enum {
    MMR_OK = 0,
    MMR_EIO = -5,      /* a HIP runtime call failed */
    MMR_EINVAL = -22,  /* bad argument (shape, dtype, alignment, null pointer) */
    MMR_ENOSPC = -28,  /* workspace smaller than *_workspace_bytes() */
    MMR_ENOTSUP = -95  /* shape outside what the kernels are built for */
};

const char *mmr_last_error(void);
int mmr_version(void);

/* ------------------------------------------------------------------------------------------
 * Similarity / ranking  (replaces reference code/search_image.py:107 `100. * F @ r.t()`,
 * code/utils.py:17 `output.topk(k,1,True,True)`, code/search_image.py:133,157 `f /= f.norm()`).
 *
 * Non-finite values, ties and scale -- one contract for top-k, range search, the self-join, their masked forms and
 * the merge (tests/test_search_numeric_edges_gpu.py; the oracle's side in tests/test_oracle.py):
 *   - NaN is ABSENT.  A (query, row) pair whose exact dot64 is NaN is never returned by top-k, never matches a
 *     threshold (NaN >= t is false) and is dropped by the merge.  A gallery with NaN rows therefore gives exactly what
 *     the same call gives on the gallery with, per query, those rows removed (ids mapped back) -- the statement the
 *     masked calls make; masking or deleting such rows changes nothing, `status` included
 *     [test_nan_rows_are_absent_from_topk, test_nan_rows_never_match_in_range_search_or_self_join].  A NaN query gets
 *     -1 / -inf in every slot and no range match; its neighbours are unaffected
 *     [test_nan_query_gets_empty_slots_and_leaves_its_neighbours_alone].
 *   - +inf and -inf dots are ordinary numbers: +inf ranks first and matches every threshold; -inf ranks last and IS
 *     returned, with its row id, when fewer than k better rows exist (an empty slot has idx -1);
 *     score = (float)(dot64 * scale) [test_infinite_gallery_element_topk, ..._range_and_join].
 *   - Ties go to the lowest row id, also when a query ties with every row (an all-zero query, a gallery of identical
 *     rows).  An exact dot is never -0.0 (sums start from +0.0), so 0-valued ties have one bit pattern
 *     [test_zero_query_ties_with_every_row, test_gallery_of_identical_rows].
 *   - mmr_gallery_norm_bound skips rows whose sum of squares is NaN and returns +inf when a row's fp32 sum of squares
 *     overflows (a row norm above ~1.8e19) or a row holds an Inf.  COST: under an infinite measured bound no query is
 *     certified -- every top-k query takes the exhaustive path -- and every non-NaN pair is a range / self-join candidate
 *     (N*Q or N^2/2 candidate slots and fp64 rechecks).  The same holds per query when |q| * bound reaches FLT_MAX, where
 *     the scans' fp32 sums could overflow.  Results stay exact [test_power_of_two_scales_*].
 *   - Scale: results are exact for ANY finite inputs.  Multiplying the gallery and / or the queries by powers of two
 *     (exact in bf16, fp32 and fp64) leaves idx unchanged and multiplies every dot64 by that power, bit for bit
 *     [test_power_of_two_scales_topk, ..._crowded_boundary, ..._split_tiers, ..._range_and_join].
 *   - mmr_similarity propagates NaN / Inf as the fixed-order fp64 dot does; mmr_l2norm_rows of an all-zero row gives NaN
 *     in every element (the reference's 0/0) and leaves the other rows alone
 *     [test_similarity_propagates_non_finite_values_like_the_oracle,
 *      test_l2_normalize_of_a_zero_row_is_nan_and_the_search_drops_it].
 * ---------------------------------------------------------------------------------------- */

/* Bytes of scratch mmr_cosine_topk needs for this problem size. */
size_t mmr_search_workspace_bytes(int64_t N, int E, int Q, int k);

/* Top-k gallery rows per query by dot product, ordered by (-dot, +row index).
 *   q[Q,E], gallery[N,E] row-major, dtype fp32, bf16 or fp16 (both operands the same dtype).
 *   idx[Q,k] int32 row ids (-1 past N), score[Q,k] = (float)(dot64*scale),
 *   dot64[Q,k] (nullable) the exact fp64 dot products used for ranking,
 *   status[Q] (nullable): 0 = MFMA scan + certified exact re-rank, 1 = exhaustive exact path.
 *   scale must be > 0.
 *   gallery_norm_bound sizes the margin of the fast path's exactness certificate
 *   (8e-5 * ||q|| * bound, above the worst-case fp32 MFMA accumulation error for E <= 1024):
 *     <= 0 : measured by this call from the gallery itself (one extra streaming pass) -- always sound;
 *     >  0 : PRECONDITION: no gallery row has a larger L2 norm (1.0 for a normalised gallery).  An
 *            understated bound can let the certificate pass wrongly, i.e. return a top-k that is not exact;
 *            an overstated one only sends more queries down the exhaustive path.
 * Ranking is on fp64 dot products accumulated in the fixed order documented in
 * oracle/search_ref.c, so indices are bit-reproducible against the CPU oracle.
 * 1 <= k <= 64; k <= 26 can use the fast path, larger k is exhaustive only [test_k_at_the_fast_path_boundary_and_at_k_max].
 * NaN / Inf / ties / scale: "Non-finite values, ties and scale" above. */
int mmr_cosine_topk(const void *q, const void *gallery, mmr_dtype dtype, int Q, int64_t N, int E, int k,
                    float scale, float gallery_norm_bound, int32_t *idx, float *score, double *dot64,
                    int32_t *status, void *workspace, size_t workspace_bytes, void *stream);

/* bound_out[0] (device float) = the largest row L2 norm of gallery[N,E] (0 for N = 0), rounded up.
 * One HBM-bound pass; an index that is searched many times measures once and hands the scalar to
 * mmr_cosine_topk_ex. */
int mmr_gallery_norm_bound(const void *gallery, mmr_dtype dtype, int64_t N, int E, float *bound_out, void *stream);

/* mmr_cosine_topk with the norm bound read on the device: the margin uses
 * max(gallery_norm_bound, *gallery_norm_bound_dev) (either may be absent: <= 0 / NULL; both absent =
 * measured in the call), so a caller-supplied number can widen the margin but never shrink it below
 * the measured one.  No host read of the scalar: the call stays asynchronous and graph-capturable. */
int mmr_cosine_topk_ex(const void *q, const void *gallery, mmr_dtype dtype, int Q, int64_t N, int E, int k,
                       float scale, float gallery_norm_bound, const float *gallery_norm_bound_dev, int32_t *idx,
                       float *score, double *dot64, int32_t *status, void *workspace, size_t workspace_bytes,
                       void *stream);

/* fp32 galleries that are searched many times: split the gallery ONCE into hi = bf16(x) and lo = bf16(x - hi) (two bf16
 * arrays [N,E], together the bytes of the fp32 gallery), then search with mmr_cosine_topk_split.  That search runs in tiers:
 *   1. the bf16 scan over `hi` alone with bf16-rounded queries (half the gallery bytes, one MFMA product), certified with a
 *      margin that adds the measured rounding residuals |q - bf16(q)| * max|g| + |q| * max_row|g - hi| and 32 candidate tiles;
 *   2. only for queries tier 1 leaves open: the three-product scan q_hi.g_hi + q_lo.g_hi + q_hi.g_lo over hi and lo (the scan
 *      mmr_cosine_topk runs on fp32 rows, minus its per-tile split) with the 8e-5 |q||g| margin;
 *   3. the exhaustive fp64 path for what is still open.
 * Every tier ranks on exact fp64 re-scores of the fp32 rows, so idx / score / dot64 are IDENTICAL to
 * mmr_cosine_topk_ex(..., MMR_F32, ...); status is 0 for tiers 1-2 and 1 for tier 3.
 * mmr_gallery_split_bf16 also writes max_row ||g - hi||_2 to *resid_bound_out (device float, may be NULL); pass that pointer as
 * split_resid_bound_dev (NULL = the worst case 2^-8 * norm bound is assumed).  The split arrays and the bound must come from
 * mmr_gallery_split_bf16 of the SAME gallery contents.  Workspace: mmr_search_workspace_bytes.
 * The norm bound works as in mmr_cosine_topk_ex: none (<= 0 and NULL: measured in the call), a host number, a device scalar
 * or both; tests/test_search_split_abi_gpu.py holds every source to the identity above. */
int mmr_gallery_split_bf16(const float *gallery, int64_t N, int E, void *hi, void *lo, float *resid_bound_out, void *stream);
int mmr_cosine_topk_split(const void *q, const void *gallery, const void *gallery_hi, const void *gallery_lo,
                          const float *split_resid_bound_dev, int Q, int64_t N, int E, int k, float scale,
                          float gallery_norm_bound, const float *gallery_norm_bound_dev, int32_t *idx, float *score,
                          double *dot64, int32_t *status, void *workspace, size_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------------------------------
 * Threshold (range) search and gallery self-join  (replaces reference code/search_image.py:58-117
 * `get_similarity` + `find_thresholds`, and the O(N^2) loop of tool/find_repeated_in_same_folder.py).
 *
 * Match rule: a pair matches iff dot64 >= threshold, compared in fp64; dot64 is the fp64 dot product in the
 * fixed order of mmr_cosine_topk's dot64 (oracle/search_ref.c), `threshold` applies to the UNSCALED dot
 * (the cosine for unit rows; a caller with the reference's `100*cos >= t` passes t/100), and
 * score = (float)(dot64 * scale).  The result set and every dot64 are bit-identical to a brute-force fp64
 * evaluation.  Output pairs are sorted ascending by (query, row) -- (i, j) for the self-join, which returns
 * only pairs with i < j.  Galleries are fp32, bf16 or fp16 (fp16: gallery_hi is ignored, as for bf16), E in {128, 256, 512, 768}.
 * A NaN dot64 matches nothing, +inf matches everything: "Non-finite values, ties and scale" in the ranking block above,
 * which also states what an infinite norm bound costs here.
 *
 * How: an MFMA scan keeps every pair whose approximate dot reaches threshold - margin (8e-5 * |q| * G with G =
 * max(gallery_norm_bound, *gallery_norm_bound_dev), measured in the call when both are absent; fp32 galleries
 * are scanned through their bf16 hi half and add the split residual terms) as a CANDIDATE, an exact fp64
 * recheck keeps the matches, and a radix sort orders them.
 *
 * Capacities and overflow (counts[2], device int64: counts[0] = matches, counts[1] = candidates):
 *   - counts[1] > cand_cap: the candidate list overflowed and the outputs are INCOMPLETE (counts[0] then
 *     counts only the matches among the stored candidates).  Call again with cand_cap >= counts[1].
 *   - counts[0] > cap: the call wrote the first `cap` pairs in sorted order.  counts[0] <= counts[1] always.
 * fp32 galleries: gallery_hi = the `hi` array of mmr_gallery_split_bf16 (with resid_bound_dev = its
 * resid_bound_out, NULL = the worst case 2^-8 * G), or NULL: the call splits into its workspace.
 * bf16 galleries ignore gallery_hi and resid_bound_dev.
 * Workspace: mmr_range_workspace_bytes(N, E, Q, cand_cap, dtype, gallery_hi != NULL), Q = 0 for the self-join.
 * Outputs out_q / out_row (or out_i / out_j) int32, out_score fp32 and out_dot64 fp64 (nullable) hold `cap` entries. */
size_t mmr_range_workspace_bytes(int64_t N, int E, int Q, int64_t cand_cap, mmr_dtype dtype, int gallery_hi_given);
int mmr_cosine_range(const void *q, const void *gallery, const void *gallery_hi, mmr_dtype dtype, int Q, int64_t N,
                     int E, double threshold, float scale, float gallery_norm_bound,
                     const float *gallery_norm_bound_dev, const float *resid_bound_dev, int64_t cap, int64_t cand_cap,
                     int32_t *out_q, int32_t *out_row, float *out_score, double *out_dot64, int64_t *counts,
                     void *workspace, size_t workspace_bytes, void *stream);
/* All pairs (i, j), i < j, of gallery rows with dot64(row i, row j) >= threshold. */
int mmr_gallery_self_join(const void *gallery, const void *gallery_hi, mmr_dtype dtype, int64_t N, int E,
                          double threshold, float scale, float gallery_norm_bound,
                          const float *gallery_norm_bound_dev, const float *resid_bound_dev, int64_t cap,
                          int64_t cand_cap, int32_t *out_i, int32_t *out_j, float *out_score, double *out_dot64,
                          int64_t *counts, void *workspace, size_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------------------------------
 * Labelled threshold sweep  (the tail of every retrieval driver of the reference: `eval_threshold` /
 * `find_thresholds`, code/search_image.py:39-103 and code/main_custom.py:27-92; `evaluate_thresholds`,
 * CLIP/lab3.py:39-65, CLIP/union_dataset.py:46-61, CLIP-Chinese/lab_chinese.py:39-65).  Where mmr_cosine_range answers
 * ONE threshold, this call answers a whole grid in one pass: the reference's TP and FP counts at every grid point.
 *
 * Inputs: q[Q,E] and gallery[N,E] (both bf16 or both fp32, E in {128, 256, 512, 768}), labels[N] and targets[Q] int32
 * in device memory, thresholds_host[T] fp64 in HOST memory, strictly ascending and finite, 1 <= T <= MMR_SWEEP_T_MAX
 * (checked, like every argument, before any launch; the grid is copied before the call returns), row_mask in the
 * row-mask block's word format or NULL.  A row is live if its mask bit is set (every row under a NULL mask).
 * Outputs (device int64), all exact:
 *   ge[Q,2,T]    ge[q,1,i] = live rows r with labels[r] == targets[q] and dot64(q,r) >= thresholds[i]: the reference's
 *                TP; ge[q,0,i] = the same over rows with labels[r] != targets[q]: its FP.
 *   total[Q,2]   live rows of each class whose dot64(q,r) is not NaN.  FN = total[q,1] - TP, TN = total[q,0] - FP.
 *   counts[2]    counts[1] = candidate pairs the call needed, counts[0] = candidate pairs it rechecked.
 *                counts[1] > cand_cap: the list overflowed and ge / total are INCOMPLETE; repeat with
 *                cand_cap >= counts[1].
 * dot64 is the fixed-order fp64 dot of mmr_cosine_topk (oracle/search_ref.c); the comparison is made in fp64 on the
 * UNSCALED dot, as in mmr_cosine_range (the reference's `100*cos >= t` is t/100).  Every count equals a brute-force
 * fp64 evaluation, bit for bit; integer atomics make the result independent of arrival order, so two runs agree.
 * "Non-finite values, ties and scale" applies unchanged: a NaN dot is absent (counted nowhere, `total` included), +inf
 * clears every threshold, -inf clears none but counts in `total`, a NaN query gives all zeros, a pair that ties a
 * threshold exactly counts for it.  A masked call equals the unmasked call on the compacted gallery and labels.
 *
 * How: range search's MFMA scan with a binning epilogue.  With a = the approximate dot and eps = range search's margin
 * (8e-5 |q| G, plus the split terms for an fp32 gallery, plus 2^-137), a pair is DECIDED when no threshold lies in
 * [a - eps, a + eps] (bounds rounded outward): the exact dot then falls between the same two grid points, and the pair
 * is counted on chip, in an LDS histogram per workgroup.  Every other pair -- and every pair of a query for which
 * |q| G reaches FLT_MAX, or under an infinite norm bound -- is a CANDIDATE: stored as in range search, re-scored in
 * fp64 on the original rows and binned by binary search over the fp64 grid.  No [Q,N] array is written.
 * COST: ceil(Q / P) streams of the gallery, P = queries per pass = what fits in the 160 KiB of LDS beside the tile ring
 * (96 KiB for E >= 512), the labels of a task's rows (8 KiB) and the grid: 4 (T + 1) bytes of counts and 16 bytes of
 * parameters per query plus a small candidate staging per wave, at most 64 / 128 / 256 / 128 queries for
 * E = 128 / 256 / 512 / 768.  For E >= 512 that is 64 queries at T = 200 and 11 at T = 1001; shorter rows hold more
 * (29 at T = 1024 for E = 128).  Candidates: the share of pairs within eps of a grid point.
 * fp32 galleries are scanned through their bf16 hi half, whose margin (about 3e-3 for unit rows) exceeds a 1e-3 grid
 * step: nearly every pair inside the grid's span is then a candidate and is rechecked (exact, but sized for it:
 * cand_cap up to Q*N).
 * Norm bound sources (none = measured in the call, host number, device scalar, both), gallery_hi and resid_bound_dev
 * behave as in mmr_cosine_range.  Asynchronous on `stream`; not hipGraph-capturable (the grid is passed by value).
 * Workspace: mmr_sweep_workspace_bytes(N, E, Q, T, cand_cap, dtype, gallery_hi != NULL) = O(Q*T + cand_cap) bytes, plus
 * the hi copy (N*E*2) only for an fp32 gallery without gallery_hi: it does not otherwise grow with N. */
#define MMR_SWEEP_T_MAX 1024
size_t mmr_sweep_workspace_bytes(int64_t N, int E, int Q, int T, int64_t cand_cap, mmr_dtype dtype, int gallery_hi_given);
int mmr_threshold_sweep(const void *q, const void *gallery, const void *gallery_hi, mmr_dtype dtype, int Q, int64_t N,
                        int E, const int32_t *labels, const int32_t *targets, const double *thresholds_host, int T,
                        float gallery_norm_bound, const float *gallery_norm_bound_dev, const float *resid_bound_dev,
                        const uint32_t *row_mask, int64_t cand_cap, int64_t *ge, int64_t *total, int64_t *counts,
                        void *workspace, size_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------------------------------
 * Row-mask filtered search (a subset of the gallery without copying it out: the reference's per-class
 * `construct_dataset` galleries, code/search_image.py:167-182, and the rows the delete tools drop,
 * tool/delete repeated.py).
 *
 * Mask format: ceil(N/32) uint32 words in device memory, 4-byte aligned; bit (r & 31) of word (r >> 5) set means
 * row r may be returned.  Bits at or past N are ignored.  A NULL row_mask is the unmasked call.
 * Exactness: a masked call returns exactly what the unmasked call returns on the compacted gallery gallery[mask]
 * (row order kept), with row ids mapped back to the original rows: idx, score and dot64 bit for bit; for range
 * search and the self-join the same pairs in the same order (the self-join pairs two live rows only).  Fewer than k
 * live rows: the extra slots hold -1 / -inf.  `status` may differ from the compacted call's (the tiles differ); an
 * all-ones mask gives the unmasked call's outputs, status included.  Rows whose dot is NaN behave like masked rows
 * ("Non-finite values, ties and scale" above); a masked Inf row still counts in the norm bound.
 * The norm bound stays a bound over all N rows (a bound over a superset is still sound).  Workspaces are the unmasked
 * calls' (mmr_search_workspace_bytes, mmr_range_workspace_bytes).  Arguments, the mask's alignment included, are
 * checked on the host before any launch. */
int mmr_cosine_topk_masked(const void *q, const void *gallery, mmr_dtype dtype, int Q, int64_t N, int E, int k,
                           float scale, float gallery_norm_bound, const float *gallery_norm_bound_dev,
                           const uint32_t *row_mask, int32_t *idx, float *score, double *dot64, int32_t *status,
                           void *workspace, size_t workspace_bytes, void *stream);
int mmr_cosine_topk_split_masked(const void *q, const void *gallery, const void *gallery_hi, const void *gallery_lo,
                                 const float *split_resid_bound_dev, int Q, int64_t N, int E, int k, float scale,
                                 float gallery_norm_bound, const float *gallery_norm_bound_dev, const uint32_t *row_mask,
                                 int32_t *idx, float *score, double *dot64, int32_t *status, void *workspace,
                                 size_t workspace_bytes, void *stream);
int mmr_cosine_range_masked(const void *q, const void *gallery, const void *gallery_hi, mmr_dtype dtype, int Q,
                            int64_t N, int E, double threshold, float scale, float gallery_norm_bound,
                            const float *gallery_norm_bound_dev, const float *resid_bound_dev, const uint32_t *row_mask,
                            int64_t cap, int64_t cand_cap, int32_t *out_q, int32_t *out_row, float *out_score,
                            double *out_dot64, int64_t *counts, void *workspace, size_t workspace_bytes, void *stream);
int mmr_gallery_self_join_masked(const void *gallery, const void *gallery_hi, mmr_dtype dtype, int64_t N, int E,
                                 double threshold, float scale, float gallery_norm_bound,
                                 const float *gallery_norm_bound_dev, const float *resid_bound_dev,
                                 const uint32_t *row_mask, int64_t cap, int64_t cand_cap, int32_t *out_i, int32_t *out_j,
                                 float *out_score, double *out_dot64, int64_t *counts, void *workspace,
                                 size_t workspace_bytes, void *stream);
/* out[ceil(N/32)] = pack(keep[N] != 0) & (and_mask ? and_mask : ~0), in the mask format above (bits past N clear):
 * one launch, no host read.  keep: uint8 [N] in device memory (a bool tensor); out and and_mask 4-byte aligned. */
int mmr_row_mask_pack(const uint8_t *keep, const uint32_t *and_mask, int64_t N, uint32_t *out, void *stream);

/* ------------------------------------------------------------------------------------------
 * Decision masks: per-query thresholds, answered as row masks  (the tail of the reference's prediction pipelines:
 * `clip_en_predict` / `clip_cn_predict`, code/merge_dataset.py:259-311, `(similarity < threshold).int()` per class row;
 * their union, code/merge_dataset.py:440; `save_correct_samples` / `calc_combined_metrics`, CLIP/union_dataset.py:64-231;
 * the per-class production thresholds of code/union_clip_llava2.py:153-162).  Where mmr_cosine_range applies ONE
 * threshold to every query and returns sorted pairs, this call gives each of Q queries a threshold of its own and
 * returns Q row masks in the row-mask block's word format, in one pass over the gallery.
 *
 * Result: out_masks[Q, W] uint32, W = ceil(N/32).  Bit (r & 31) of out_masks[q*W + (r >> 5)] is 1 iff row r is live
 * (r < N, and its row_mask bit is set when row_mask is not NULL) and dot64(q, r) >= thresholds_dev[q].  dot64 is the
 * fixed-order fp64 dot of mmr_cosine_topk (oracle/search_ref.c); the comparison is made in fp64 on the UNSCALED dot,
 * as in mmr_cosine_range (the reference's `100*cos >= t` is t/100).  Bits at or past N are written as 0, and EVERY
 * word of out_masks is written by the call: the caller need not clear it.  A NaN dot sets no bit, +inf passes every
 * finite threshold, a tie passes ("Non-finite values, ties and scale" above).  A masked call equals the unmasked call
 * AND-ed with the mask.  The masks of two calls over the same rows combine word-wise (mmr_row_mask_combine), and a mask
 * row is a valid row_mask of every *_masked call.
 * thresholds_dev[Q]: fp64 in DEVICE memory, 8-byte aligned, finite.  The call cannot check them (no host read); a NaN
 * or infinite threshold makes every pair of that query a candidate, and the fp64 comparison then decides: NaN sets no
 * bit, +inf only the rows whose dot is +inf, -inf every live row whose dot is not NaN.
 * Galleries are fp32, bf16 or fp16, E in {128, 256, 512, 768}; gallery_hi, resid_bound_dev and the norm bound's sources
 * (none = measured in the call, host number, device scalar, both) behave as in mmr_cosine_range.
 *
 * How: range search's MFMA scan with a deciding epilogue.  With a = the approximate dot and eps = range search's margin,
 * a >= thresholds[q] + eps (rounded up to fp32) is a certain pass and a < thresholds[q] - eps (rounded down) a certain
 * fail; every other pair -- a NaN product, and every pair of a query for which |q| G reaches FLT_MAX or under an
 * infinite norm bound -- is a CANDIDATE: its bit is left 0, the pair is stored as in range search, re-scored in fp64 on
 * the original rows, and OR-ed in if it passes.  A 32-row scan tile is one mask word per query.  Integer OR only: two
 * runs give the same masks and counts.
 * counts[2] (device int64): counts[1] = candidate pairs the call needed, counts[0] = candidates it rechecked.
 * counts[1] > cand_cap: the masks are INCOMPLETE (bits of unstored candidates are 0); repeat with cand_cap >= counts[1].
 * Candidates are the pairs within eps of their threshold; all Q*N pairs of a wild query.
 * Arguments are checked on the host before any launch.  No allocation and no host read: asynchronous on `stream` and
 * hipGraph-capturable (new thresholds are new contents of thresholds_dev).  N == 0 writes only counts.
 * Workspace: mmr_decide_workspace_bytes(N, E, Q, cand_cap, dtype, gallery_hi != NULL) = 8 * cand_cap bytes plus fixed
 * scalars, plus the bf16 queries of an fp32 call, plus the hi copy (N*E*2) only for an fp32 gallery without
 * gallery_hi: no sort storage, and it does not otherwise grow with N. */
size_t mmr_decide_workspace_bytes(int64_t N, int E, int Q, int64_t cand_cap, mmr_dtype dtype, int gallery_hi_given);
int mmr_cosine_decide(const void *q, const void *gallery, const void *gallery_hi, mmr_dtype dtype, int Q, int64_t N, int E,
                      const double *thresholds_dev, float gallery_norm_bound, const float *gallery_norm_bound_dev,
                      const float *resid_bound_dev, const uint32_t *row_mask, int64_t cand_cap, uint32_t *out_masks,
                      int64_t *counts, void *workspace, size_t workspace_bytes, void *stream);
/* out[i] = a[i] | b[i] (op 0), a[i] & b[i] (op 1), a[i] & ~b[i] (op 2) over `words` words; out may alias a or b.
 * Union and intersection of decision masks (the reference's EN-or-CN rule), or of any row masks. */
int mmr_row_mask_combine(const uint32_t *a, const uint32_t *b, int op, int64_t words, uint32_t *out, void *stream);
/* The confusion counts of Q decision masks (masks[Q, ceil(N/32)]) against labels: out[Q,4] int64 = {TP, FP, POS, NEG},
 * TP / FP = set bits on live rows with labels[r] == targets[q] / != targets[q], POS / NEG = the live rows of each kind
 * (`calc_combined_metrics`' total_pos / total_neg, CLIP/union_dataset.py; FN = POS - TP, TN = NEG - FP).  labels ==
 * NULL: out[q] = {set bits on live rows, 0, live rows, 0}.  row_mask nullable (NULL: every row below N is live).
 * POS / NEG count live rows by label alone; mmr_threshold_sweep's `total` also drops the rows whose dot is NaN, so the
 * two agree on galleries without NaN dots.  Integer accumulation: two runs agree.  The call zeroes `out` itself. */
int mmr_decision_counts(const uint32_t *masks, int Q, int64_t N, const int32_t *labels, const int32_t *targets,
                        const uint32_t *row_mask, int64_t *out, void *stream);

/* ------------------------------------------------------------------------------------------
 * Nearest-centroid assignment and per-cluster sums: the two halves of a Lloyd iteration  (the reference's `KMeans` in
 * `get_cluster_features` / `get_text_cluster_features`, code/search_image.py:185-292, for a gallery instead of 10-50
 * shots).  Every other scan call reduces over rows per query; this one reduces over K centroids for every row, without
 * an [N, K] score matrix.
 *
 * Result: labels[N] int32.  With score(r, c) = dot64(g_r, c) + bias_dev[c] in fp64 -- dot64 the fixed-order fp64 dot of
 * mmr_cosine_topk (oracle/search_ref.c); bias_dev[K] fp64 in DEVICE memory, NULL = no bias term -- labels[r] is the c
 * with the largest score.  Ties go to the LOWEST c.  A NaN score never wins ("Non-finite values, ties and scale"
 * above); +-inf are numbers.  A row whose every score is NaN, and a row whose row_mask bit is clear, gets -1.  EVERY
 * element of labels is written, whatever the buffer held.  bias = -|c|^2 / 2 makes the winner the Euclidean nearest
 * centroid (a Lloyd step); no bias is the cosine / spherical rule.
 * best64[N] (nullable): the exact fp64 score of (r, labels[r]), NaN where the label is -1.
 * Galleries are bf16 or fp16 with the centroids in the gallery's dtype; an fp32 gallery is MMR_ENOTSUP: scanned through
 * its bf16 half it would leave 18-42 % of the rows to the exact recheck.  E in {128, 256, 512, 768},
 * 1 <= K <= 2^24, N < 2^31 - 1.  The norm bound's sources behave as in mmr_cosine_range.
 *
 * How: range search's MFMA scan with the operands swapped, in passes of 256 centroids (128 at E = 768).  Each wave
 * keeps, per row, the best and the second best approximate score over its 32 centroids; a merge after every pass folds
 * them into the winner's lower bound and the largest upper bound of any other centroid, with eps(c) = the scan's margin
 * plus the roundings of the fp32 bias add.  A row whose winner's lower bound is STRICTLY above every other upper bound
 * is decided.  Every other live row -- equal approximate scores, a product that is not finite, a wild centroid -- is
 * AMBIGUOUS: its id is stored and its K exact scores are compared in fp64.  Integer atomics only: two runs agree.
 * counts[2] (device int64): counts[1] = ambiguous rows the call found, counts[0] = ambiguous rows it rechecked.
 * counts[1] > amb_cap: labels are INCOMPLETE (an unstored ambiguous row holds -1); repeat with amb_cap >= counts[1].
 * On random unit rows about 1 % of the rows are ambiguous; duplicate centroids make every row ambiguous.
 * Arguments are checked on the host before any launch.  No allocation and no host read: asynchronous on `stream` and
 * hipGraph-capturable.  N == 0 writes only counts.
 * Workspace (256-byte aligned): mmr_assign_workspace_bytes(N, E, K, amb_cap, dtype) = 112 bytes per row (64 at E = 768)
 * + 4 * amb_cap + about 5 bytes per centroid; 0 for arguments the call would refuse. */
size_t mmr_assign_workspace_bytes(int64_t N, int E, int K, int64_t amb_cap, mmr_dtype dtype);
int mmr_cosine_assign(const void *gallery, const void *centroids, mmr_dtype dtype, int64_t N, int K, int E,
                      const double *bias_dev, float gallery_norm_bound, const float *gallery_norm_bound_dev,
                      const uint32_t *row_mask, int64_t amb_cap, int32_t *labels, double *best64, int64_t *counts,
                      void *workspace, size_t workspace_bytes, void *stream);
/* sums[K, E] fp64 and sizes[K] int64 of the rows carrying each label: sums[k] = the sum of the rows r with
 * labels[r] == k, sizes[k] their number.  Labels outside [0, K) -- -1 included -- are skipped.  Gallery fp32, bf16 or
 * fp16, 1 <= E <= 65536, 1 <= K <= 65535.  Bit-for-bit reproducible from run to run: no floating-point atomics; a
 * stable radix sort groups the row ids by label, each cluster's rows are summed in ascending row order in chunks of 256,
 * and the chunks' partial sums are added in a fixed order that depends on the labels, N and K alone.  An empty cluster
 * gets zeros.  The call writes every element of sums and sizes.
 * Workspace (256-byte aligned): mmr_cluster_sums_workspace_bytes(N, E, K) = 24 bytes per row plus the sort's storage
 * plus at most 8 * E * (N / 256 + K) bytes of partial sums; 0 for arguments the call would refuse. */
size_t mmr_cluster_sums_workspace_bytes(int64_t N, int E, int K);
int mmr_cluster_sums(const void *gallery, mmr_dtype dtype, int64_t N, int E, const int32_t *labels, int K, double *sums,
                     int64_t *sizes, void *workspace, size_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------------------------------
 * Silhouette sums and samples of a labelled gallery: how a user of the calls above picks K  (the reference's
 * `silhouette_score(image_features, kmeans.labels_)`, code/search_image.py:256-259).  One pairwise scan computes the
 * N x N distances with the gallery as both operands; nothing of size N x N is stored.
 *
 * Definition, in fp64 on the rows' 16-bit values.  Row r is LIVE when 0 <= labels[r] < K; every other label (-1
 * included) is skipped, as in mmr_cluster_sums.  sizes[c] = the live rows with label c.  d(i, j), metric 0 (euclidean):
 * sqrt(sum_e (x_ie - x_je)^2); metric 1 (cosine): 1 - x_i.x_j / (|x_i| |x_j|); d(i, i) = 0 exactly.
 * sums[i, c] = the sum of d(i, j) over the live j with labels[j] == c: written for EVERY i in [0, N) and c in [0, K),
 * whatever the buffer held -- a row that is not live gets its distances to each cluster too.
 * mmr_silhouette_samples: samples[i] of a live row, own = labels[i]: 0 when sizes[own] == 1; otherwise with
 * a = sums[i, own] / (sizes[own] - 1) and b = the smallest sums[i, c] / sizes[c] over c != own with sizes[c] > 0 (+inf
 * when there is none), (b - a) / max(a, b), and 0 when max(a, b) == 0; NaN when any of those means is NaN.  Rows that
 * are not live get NaN.  IEEE fp64 divisions, one subtraction and comparisons: numpy gives the same bits.
 *
 * mmr_silhouette_sums is approximate (the two calls above are exact): the dot products come from the MFMA scan in fp32,
 * |acc - dot64| <= 8e-5 |x_i| |x_j|, the squared norms are exact fp64 sums rounded once to fp32, euclidean distances are
 * sqrt(max(n_i + n_j - 2 acc, 0)) with the 1-ulp v_sqrt_f32, cosine ones 1 - acc / (|x_i| |x_j|) with fp32 reciprocal
 * norms, and no fp32 accumulator takes more than 1025 additions before its value goes to fp64.  With p = |x_i| |x_j|,
 * n = |x_i|^2 + |x_j|^2 and eta = 1.7e-4 p + 2^-21 n a pair is off by at most
 *   delta(i, j) = min(sqrt(eta), eta / d) + 2^-22 d      (euclidean)        1.7e-4 + 2^-21      (cosine)
 * and |sums[i, c] - exact| <= sum_j delta(i, j) + 1.001 * 2^-13 * sum_j (d(i, j) + delta(i, j))  (DESIGN.md section 3,
 * "Silhouette").  Exact duplicates therefore measure about sqrt(1e-7 p) apart instead of 0; the self pair is exact.
 * Non-finite rows take no special path: a row with an inf or NaN element, or whose squared norm overflows fp32 (cosine:
 * a zero row), makes sums[:, c] of its own cluster and its own row of sums non-finite; every other entry keeps the bound.
 * No floating-point atomics: two runs agree bit for bit, whatever the workspace held.
 * Galleries are bf16 or fp16; an fp32 gallery is MMR_ENOTSUP, as in mmr_cosine_assign: the score belongs to the 16-bit
 * gallery the clustering ran on.  E in {128, 256, 512, 768}, 1 <= K <= MMR_SILHOUETTE_K_MAX, N < 2^31 - 1.
 * Arguments are checked on the host before any launch.  No allocation and no host read: asynchronous on `stream` and
 * hipGraph-capturable.  N == 0 writes only sizes.
 * Workspace (256-byte aligned): mmr_silhouette_workspace_bytes(N, E, K, dtype) = a label-sorted copy of the gallery
 * (2 E bytes per row, at most 32 padding rows per cluster), 40 bytes per row, the sort's storage and 4 N bytes per chunk
 * of 2048 sorted rows (at most N / 2048 + K chunks); 0 for arguments the call would refuse. */
#define MMR_SILHOUETTE_K_MAX 1024
size_t mmr_silhouette_workspace_bytes(int64_t N, int E, int K, mmr_dtype dtype);
int mmr_silhouette_sums(const void *gallery, mmr_dtype dtype, int64_t N, int E, const int32_t *labels, int K, int metric,
                        double *sums /* [N, K] */, int64_t *sizes /* [K] */, void *workspace, size_t workspace_bytes,
                        void *stream);
int mmr_silhouette_samples(const double *sums, const int32_t *labels, const int64_t *sizes, int64_t N, int K,
                           double *samples /* [N] */, void *stream);

/* ------------------------------------------------------------------------------------------
 * k-means++ seeding: the start sklearn's KMeans gives the reference's clustering  (`KMeans(n_clusters=...)`,
 * code/search_image.py:185-292).  Greedy k-means++ as in sklearn.cluster._kmeans._kmeans_plusplus (sample_weight = 1),
 * made reproducible by integer weights: the device result EQUALS a restatement in integers (tests/kmeanspp_helpers.py).
 *
 * Inputs.  gallery [N, E], bf16 or fp16 (an fp32 gallery is MMR_ENOTSUP, as in mmr_cosine_assign); E in {128, 256, 512,
 * 768}; 1 <= N <= 2^24; 1 <= K <= 65535 and K <= the number of live rows (K <= N is checked; with a row_mask the rest is
 * the caller's promise); row_mask (nullable): the packed words of mmr_cosine_assign -- a row whose bit is clear is never
 * chosen and has weight 0; L = trials per step, 1 <= L <= MMR_KMEANSPP_TRIALS_MAX (sklearn's default is
 * 2 + int(ln K)); variates_dev: int64 [K, L] in DEVICE memory, each in [0, 2^53) (a value outside is clamped into it) --
 * step 0 uses only variates[0][0]; metric 0 (euclidean) or 1 (cosine, the spherical rule of k-means on unit rows).
 *
 * Scale.  G = max(gallery_norm_bound, *gallery_norm_bound_dev), measured in the call when both are absent (the sources
 * behave as in mmr_cosine_assign), widened to fp64.  Dmax = 4 * G * G (euclidean) or 1 + G * G (cosine), as fp64
 * operations.  shift = 37 - ilogb(Dmax), 0 when Dmax == 0; S = 2^shift.  The call writes shift to shift[0].
 *
 * Distance of row i to centre c.  dot = the fixed-order fp64 dot of mmr_cosine_topk (oracle/search_ref.c's
 * mmr_ref_dot64: exact products, fixed order); n_i = dot(x_i, x_i).  Euclidean: d = (n_i + n_c) - 2 * dot(x_i, x_c).
 * Cosine: d = 1 - dot(x_i, x_c).  w = min(int64(trunc(max(d, 0) * S)), 2^38 - 1) -- the scaling by S is exact -- and a
 * NaN d gives weight 0.  All sums of weights are int64: exact in any order, so two runs agree bit for bit.
 *
 * Sampling, from a weight vector w[0..N) with total T and a variate b: r = (b * T) >> 53 with a 128-bit product; the
 * sample is the smallest row i whose inclusive prefix sum exceeds r.  When T == 0 the sample is the lowest live row.  A
 * sampled id is always a live row in [0, N), whatever the buffers hold.
 *
 * Step 0: w_i = 1 on live rows; one sample with variates[0][0] gives indices[0]; closest = the distance weights to that
 * row (0 on rows that are not live); potentials[0] = sum(closest).
 * Step c >= 1: L samples from closest with variates[c][0..L); for each trial t, trial_t = min(closest, weights to
 * candidate t) elementwise and pot_t = sum(trial_t); the winner is the smallest pot_t, ties to the lowest t;
 * indices[c] = its row, closest = trial_winner, potentials[c] = pot_winner.
 *
 * Outputs: indices int32 [K], potentials int64 [K], shift int32 [1], centers [K, E] = the chosen rows in the gallery's
 * dtype.  What follows: a chosen row has weight 0 and is not drawn again while T > 0; with at least K distinct live
 * rows whose pairwise d * S is at least 1 the K seeds are distinct; when the distinct rows run out the remaining seeds
 * repeat the lowest live row (what sklearn's searchsorted on a zero cumsum does with index 0).  Rows with non-finite
 * elements are out of scope: weight 0 where d is NaN, the result otherwise unspecified but in range.
 *
 * How: per step one gallery pass (each row loaded and converted once, dotted in fp64 with the <= 16 candidate rows
 * staged in LDS, 8 * L bytes of trial weights stored per row against the row's 2 * E), one workgroup per trial for the
 * two-level sampling (per-block sums of MMR_KMEANSPP_BLOCK_ROWS rows, then the block's rows), and one small launch that
 * picks the winner; the next pass reads closest through the winner's plane number, nothing of size N is copied.  Three
 * launches per step.  Arguments are checked on the host before any launch.  No allocation, no host read and nothing
 * data-dependent on the host: asynchronous on `stream` and hipGraph-capturable.  Integer atomics only.
 * Workspace (256-byte aligned): mmr_kmeanspp_workspace_bytes(N, E, K, L) = (8 + 16 * L) bytes per row plus 16 * L bytes
 * per block of rows; 0 for arguments the call would refuse.  It may hold anything on entry. */
#define MMR_KMEANSPP_TRIALS_MAX 16
#define MMR_KMEANSPP_BLOCK_ROWS 256
size_t mmr_kmeanspp_workspace_bytes(int64_t N, int E, int K, int L);
int mmr_kmeanspp_seed(const void *gallery, mmr_dtype dtype, int64_t N, int E, int K, int L, int metric,
                      const uint32_t *row_mask, const int64_t *variates_dev, float gallery_norm_bound,
                      const float *gallery_norm_bound_dev, int32_t *indices, int64_t *potentials, int32_t *shift,
                      void *centers, void *workspace, size_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------------------------------
 * Distances to the own centre, per-cluster ranking and percentile trim: the reference's outlier-trimmed class centre
 * (`outlier_filter`, code/search_image.py:295-318: the mean of the rows within np.percentile(1 - rows @ mean, 95)) and
 * the "shots members nearest their cluster's centre" half of get_cluster_features (185-232), for a labelled gallery.
 *
 * mmr_cluster_rank.  Gallery [N, E] fp32, bf16 or fp16; E in {128, 256, 512, 768} (the fixed-order dot needs 64 chunks);
 * 1 <= K <= 65535; N < 2^31 - 1; centers [K, E] fp32 in device memory; row r is LIVE when 0 <= labels[r] < K, as in
 * mmr_cluster_sums.
 * Distance of a live row r, with c = centers[labels[r]] and s = dot64(x_r, c): dot64 is the fixed-order fp64 dot of
 * mmr_cosine_topk (oracle/search_ref.c's mmr_ref_dot64).  The row's elements and the fp32 centre widen to fp64 exactly,
 * every product is exact (at most 24 x 24 bits) and the order is fixed.  The centre is fp32 for that reason: rounding
 * the centre to fp32 ONCE, before the call, is what keeps the products exact -- an fp64 centre would round every product.
 *   metric 1 (cosine), outlier_filter's rule: d = 1.0 - s.  The centre is not normalised, as in the reference.
 *   metric 0 (euclidean), np.linalg.norm's order: d = (n_r + n_c) - 2 * s with n = dot64(v, v); a negative d becomes 0.
 *     This is the SQUARED distance, the expression of mmr_kmeanspp_seed.
 * -0.0 counts as +0.0.  NaN stays NaN (stored as the quiet NaN 0x7ff8000000000000).  dist[r] is written for every r and is
 * that NaN on rows that are not live.
 * order[start[k] .. start[k + 1]) holds cluster k's live rows sorted by (dist ascending, row id ascending); NaN comes
 * after +inf.  Positions from start[K] on hold the rows that are not live, in ascending row id; start[0] = 0.  Every
 * element of dist [N], order [N] and start [K + 1] is written, whatever the buffers held.  N == 0 writes only start.
 *
 * mmr_cluster_percentile_trim, on the arrays above and the same labels.  thresholds[k] = numpy's linear-interpolation
 * percentile q of cluster k's distances, bit for bit: with n = start[k + 1] - start[k], v = (q / 100.0) * (n - 1),
 * lo = floor(v), hi = min(lo + 1, n - 1), t = v - lo, a and b the distances at sorted positions lo and hi, diff = b - a:
 * thr = a + diff * t when t < 0.5, else b - diff * (1 - t) -- every operation a separate IEEE fp64 operation, none
 * contracted into an fma.  An empty cluster gives NaN; so does a cluster holding a NaN distance (np.percentile's rule).
 * 0 <= q <= 100 is checked on the host.
 * trimmed_labels[r] = labels[r] when r is live and dist[r] <= thresholds[labels[r]], else -1: the compare is by value,
 * so rows that tie with the threshold are all kept and a NaN never passes.  kept[k] = the number of cluster k's ranked
 * rows that pass.  Every element of thresholds [K], trimmed_labels [N] and kept [K] is written.
 *
 * Both calls: arguments are checked on the host before any launch.  No allocation and no host read: asynchronous on
 * `stream`.  No floating-point atomics (the trim uses no atomics at all): two runs agree bit for
 * bit, and the result does not depend on what the workspace held.
 * How: ONE pass over the gallery in row order, 16 lanes per row, the row's centre held in registers while consecutive
 * rows share a label, writes dist and a 16-byte record (label, a sortable 64-bit image of the distance, row id) per row;
 * ONE sort of the records by (label, image, row id) gives order; start comes by binary search.  Nothing of the gallery
 * is copied or re-ordered.  The trim is two small launches: one thread per cluster, then one per row.
 * Workspace (256-byte aligned): mmr_cluster_rank_workspace_bytes(N, E, K) = 32 bytes per row plus the sort's storage
 * plus 8 bytes per centre; 0 for arguments the call would refuse. */
size_t mmr_cluster_rank_workspace_bytes(int64_t N, int E, int K);
int mmr_cluster_rank(const void *gallery, mmr_dtype dtype, int64_t N, int E, const int32_t *labels, int K,
                     const float *centers /* [K, E] fp32, device */, int metric,
                     double *dist /* [N] */, int32_t *order /* [N] */, int64_t *start /* [K + 1] */,
                     void *workspace, size_t workspace_bytes, void *stream);
int mmr_cluster_percentile_trim(const double *dist, const int32_t *order, const int64_t *start, const int32_t *labels,
                                int64_t N, int K, double q,
                                double *thresholds /* [K] */, int32_t *trimmed_labels /* [N] */, int64_t *kept /* [K] */,
                                void *stream);

/* ------------------------------------------------------------------------------------------
 * Deep top-k: exact top-k for 1 <= k <= MMR_DEEP_K_MAX (recall@100, re-rank shortlists, k-NN lists; the reference's
 * `np.argsort(d)[:shots]` with an open `shots`).  mmr_cosine_topk* keep their limit of k <= 64.
 *
 * Result: per query the k best rows by (-dot64, +row), dot64 the fixed-order fp64 dot of mmr_cosine_topk
 * (oracle/search_ref.c): idx int64 [Q,k] (written as int64 by the call), score fp32 [Q,k] = (float)(dot64 * scale),
 * dot64 fp64 [Q,k] (nullable) -- bit for bit what mmr_cosine_topk returns where both accept k.  Fewer than k rows
 * to return: the extra slots hold -1 / -inf / -inf.  row_mask (nullable): the row-mask block's format and exactness.
 * Galleries are fp32, bf16 or fp16, E in {128, 256, 512, 768} (E = 1024: MMR_ENOTSUP, no MFMA scan exists there).
 * fp32 galleries: gallery_hi / gallery_lo = the arrays of mmr_gallery_split_bf16 with split_resid_bound_dev = its
 * resid_bound_out (NULL: the worst case 2^-8 * G) -- the call then scans the bf16 hi half with bf16-rounded queries
 * (gallery_lo is not read) -- or gallery_hi = NULL: the fp32 rows are scanned as mmr_cosine_topk scans them.  The
 * exact dots always read the fp32 rows.  bf16 galleries ignore the three arguments.
 *
 * How: the top-k scan leaves bmax[tile][q], the maximum of the approximate dots over each tile's live rows.  With b_k
 * the k-th largest entry of a query's column and eps the scan's margin (8e-5 |q| G with G = max(gallery_norm_bound,
 * *gallery_norm_bound_dev), measured in the call when both are absent; the hi-half scan adds the split residual terms
 * as in mmr_cosine_range), the k-th best exact dot is >= b_k - eps, so every top-k row lies in a tile with
 * bmax >= b_k - 2 eps: those (query, tile) pairs are LISTED, every live row of a listed tile is re-scored in fp64, the
 * rows with dot64 >= b_k - eps SURVIVE and are ranked by stable radix sorts.  No certificate, no fallback path.
 * Non-finite values ("Non-finite values, ties and scale" above): a row whose dot is NaN is absent, +inf ranks first,
 * -inf ranks last and is returned with its id.  A query with |q| G at fp32's edge, an infinite or NaN bound (an Inf
 * row makes every query such), or fewer than k tiles, gets -inf thresholds: every tile is listed and every non-NaN
 * row survives -- exact, at the cost of Q*N exact dots.  A query that ties with everything lists everything too.
 *
 * Capacities (counts[2], device int64: counts[0] = listed (query, tile) pairs, counts[1] = survivors):
 * counts[0] > tile_cap or counts[1] > surv_cap: the outputs are UNSPECIFIED; call again with capacities at least the
 * counts.  An overflowed tile list undercounts the survivors (they never exceed 32 per listed pair).  On ordinary
 * data both counts are a little above Q * k.  Integer atomics only: two runs give the same outputs and counts.
 * Arguments are checked on the host before any launch; Q == 0 returns MMR_OK, N == 0 fills the empty outputs.
 * No allocation and no host read: asynchronous on `stream` and hipGraph-capturable at fixed capacities.
 * Workspace: mmr_deep_topk_workspace_bytes(N, E, Q, k, tile_cap, surv_cap, dtype, gallery_hi != NULL)
 * = 4 * ceil(N / 32) * min(Q, queries per scan pass) bytes of bucket maxima (16-row tiles for an unsplit fp32 gallery) plus
 * 8 * tile_cap + 32 * surv_cap bytes of lists plus the sort's storage; 0 for arguments the call would refuse. */
#define MMR_DEEP_K_MAX 4096
size_t mmr_deep_topk_workspace_bytes(int64_t N, int E, int Q, int k, int64_t tile_cap, int64_t surv_cap, mmr_dtype dtype,
                                     int split_given);
int mmr_cosine_topk_deep(const void *q, const void *gallery, const void *gallery_hi, const void *gallery_lo,
                         const float *split_resid_bound_dev, mmr_dtype dtype, int Q, int64_t N, int E, int k, float scale,
                         float gallery_norm_bound, const float *gallery_norm_bound_dev, const uint32_t *row_mask,
                         int64_t tile_cap, int64_t surv_cap, int64_t *idx, float *score, double *dot64, int64_t *counts,
                         void *workspace, size_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------------------------------
 * A row mask per query: mmr_cosine_topk_deep_qmasked, mmr_threshold_sweep_qmasked  (the reference's retrieval protocol: every class's query leaves that class's own sample images
 * out of ITS gallery, `construct_dataset`, code/search_image.py:167-182 in the loop of :382-390, while they stay in
 * the other classes' galleries as negatives; and its cascade, code/merge_dataset.py:259-365: rank with one tower among
 * the rows another tower's thresholds accepted, i.e. the rows of an mmr_cosine_decide mask).  The *_masked calls take
 * ONE mask for all queries of a call; this call takes Q masks and still streams the gallery once.
 *
 * Masks: row_masks[Q, mask_stride] uint32 in device memory, 4-byte aligned, mask_stride >= W = ceil(N/32) words.  Row q
 * is query q's mask in the row-mask block's format; bits at or past N are ignored and the words at or past W of a row
 * are never read -- out_masks of mmr_cosine_decide serves as it is (mask_stride = W).  row_mask[W] (nullable) is one
 * more mask shared by all queries, AND-ed in (an index's deleted rows: no [Q, W] temporary).
 * Exactness: row q of idx, score and dot64 equals, bit for bit, what mmr_cosine_topk_deep returns for query q alone
 * with the single mask row_masks[q] & row_mask -- and so mmr_cosine_topk_masked's result where k <= 64.  counts may
 * differ (candidate sets depend on the tiles).  A query whose mask leaves fewer than k rows gets -1 / -inf / -inf in the
 * extra slots; an all-zero mask row gives that query an empty result and leaves its neighbours alone; masks that are
 * all ones give mmr_cosine_topk_deep's unmasked outputs.  "Non-finite values, ties and scale" applies unchanged: a row
 * whose dot is NaN is absent for a query whether that query's mask keeps it or not.
 * mmr_cosine_topk_deep's contract otherwise: capacities and counts, no status output, E = 1024 is MMR_ENOTSUP.  An fp32
 * gallery must come with gallery_hi (MMR_EINVAL otherwise): the scan runs on 16-bit operands, and the fp32 row scan of
 * mmr_cosine_topk_deep has no per-query form.  Arguments -- the masks' alignment and mask_stride >= W included -- are
 * checked on the host before any launch; no allocation and no host read; hipGraph-capturable at fixed capacities.
 * Not extended: mmr_cosine_decide with a filter per query is its result AND-ed with the masks (mmr_row_mask_combine);
 * the pairs of mmr_cosine_range can be filtered after the call; the self-join has no queries.
 * How: the scan keeps a task's mask words [tile][query] in LDS beside the tile ring, so a task holds fewer tiles when
 * many queries are resident; the plan therefore differs from mmr_cosine_topk_deep's.  Workspace:
 * mmr_deep_topk_qmasked_workspace_bytes, mmr_deep_topk_workspace_bytes's arguments (0 for an fp32 gallery without
 * split_given). */
size_t mmr_deep_topk_qmasked_workspace_bytes(int64_t N, int E, int Q, int k, int64_t tile_cap, int64_t surv_cap,
                                             mmr_dtype dtype, int split_given);
int mmr_cosine_topk_deep_qmasked(const void *q, const void *gallery, const void *gallery_hi, const void *gallery_lo,
                                 const float *split_resid_bound_dev, mmr_dtype dtype, int Q, int64_t N, int E, int k,
                                 float scale, float gallery_norm_bound, const float *gallery_norm_bound_dev,
                                 const uint32_t *row_masks, int64_t mask_stride, const uint32_t *row_mask, int64_t tile_cap,
                                 int64_t surv_cap, int64_t *idx, float *score, double *dot64, int64_t *counts,
                                 void *workspace, size_t workspace_bytes, void *stream);
/* mmr_threshold_sweep with a row mask per query, in the same words: query q counts only the rows of row_masks[q] &
 * row_mask.  ge[q] and total[q] equal, exactly, what mmr_threshold_sweep returns for query q alone with that single mask
 * (total[q] is per query: the rows of q's own gallery by label, NaN dots dropped); counts may differ.  The reference's
 * loop over classes and shot counts (code/search_image.py:340-390: 24 queries, 24 galleries) is one call and one gallery
 * pass.  The scan keeps the task's mask words in LDS beside its labels, so a pass holds somewhat fewer queries than
 * mmr_threshold_sweep's at the same T.  Arguments, contract and workspace (mmr_sweep_workspace_bytes: the plan is the
 * same) are mmr_threshold_sweep's; fp32 galleries are scanned through their hi half as there, given or built. */
int mmr_threshold_sweep_qmasked(const void *q, const void *gallery, const void *gallery_hi, mmr_dtype dtype, int Q, int64_t N,
                                int E, const int32_t *labels, const int32_t *targets, const double *thresholds_host, int T,
                                float gallery_norm_bound, const float *gallery_norm_bound_dev, const float *resid_bound_dev,
                                const uint32_t *row_masks, int64_t mask_stride, const uint32_t *row_mask, int64_t cand_cap,
                                int64_t *ge, int64_t *total, int64_t *counts, void *workspace, size_t workspace_bytes,
                                void *stream);
/* mmr_row_mask_pack for Q masks in one launch: out[q, w] = pack(keep[q, :] != 0)[w] & (and_mask ? and_mask[w] : ~0) for
 * w < W = ceil(N/32), and out[q, w] = 0 for W <= w < stride (the pad words are written).  keep: uint8 [Q, N] in device
 * memory; and_mask [W] nullable; stride >= W; Q <= 65535. */
int mmr_row_masks_pack(const uint8_t *keep, const uint32_t *and_mask, int Q, int64_t N, int64_t stride, uint32_t *out,
                       void *stream);

/* ------------------------------------------------------------------------------------------
 * Perceptual-hash Hamming joins  (the duplicate rule of the reference's clean-up tools: `are_images_similar`,
 * tool/find_repeated_in_same_folder.py:38-54 in the O(N^2) loop of :76-95 -- phash, dhash, whash, ANY distance <= 5; and
 * tool/delete repeated.py:11,120-135 -- dhash between a train and a test set, threshold 0).  The hashes come from
 * mmr_image_hashes below (decoded pixels in) or from the caller.
 *
 * Data: hashes[N, H, W] uint64 in device memory, row-major, 8-byte aligned: H = 1..4 hash kinds per image, W = 1 or 4
 * 64-bit words per hash (hash_size 8 or 16; other sizes are zero-padded by the caller).  Bits are unsigned; any fixed
 * bit order serves.  thresholds_host[H] int32 in HOST memory, read before the call returns; a negative entry disables
 * its kind, and at least one kind must be enabled.
 * Match rule, integer-exact: a pair matches iff for some enabled kind h
 *     popcount(a[h] ^ b[h]) (summed over the W words) <= thresholds_host[h].
 * mmr_hash_self_join returns every matching pair i < j of one set, sorted ascending by (i, j); mmr_hash_cross_join
 * every matching (q, r) of queries[M, H, W] x refs[N, H, W], sorted by (q, r).  Two runs give identical outputs.
 * Outputs: out_i / out_j (out_q / out_ref) int32[cap]; out_dist uint64[cap], nullable: kind h's distance in bits
 * [16h, 16h + 16) (distances reach 256), 0xFFFF for a disabled or absent kind.  row_mask: the row-mask block's word
 * format over the N rows, NULL for none; a self-join pair needs both rows live, a cross-join pair its ref row.
 * Capacity and overflow (counts[1], device int64): counts[0] = the number of matching pairs.  counts[0] > cap: the
 * outputs are INCOMPLETE (`cap` of the pairs, which ones is unspecified); repeat with cap >= counts[0].  This is range
 * search's protocol with one capacity: there are no candidates.  cap = 0 counts only (outputs may be NULL).
 * N <= 1 (M = 0 or N = 0 for the cross join) gives counts[0] = 0 and launches no kernel.
 * Arguments -- N, M < 2^31 - 1, H, W, an enabled kind, pointer alignment, the workspace size -- are checked on the host
 * before any launch.  Asynchronous on `stream`, no allocation, no host read; hipGraph-capturable (the thresholds travel
 * by value).  Workspace: mmr_hash_join_workspace_bytes(M or 0, N, H, W, cap) = O(cap) bytes (0: bad arguments).
 * How: one launch over a linearised grid of 1024 x 1024 tiles (the self-join: those on or above the diagonal), XOR and
 * v_bcnt_u32_b32 per word, matches compacted per wave and appended, then a radix sort.  VALU-bound: DESIGN.md section 3. */
size_t mmr_hash_join_workspace_bytes(int64_t M, int64_t N, int H, int W, int64_t cap);
int mmr_hash_self_join(const uint64_t *hashes, int64_t N, int H, int W, const int32_t *thresholds_host,
                       const uint32_t *row_mask, int64_t cap, int32_t *out_i, int32_t *out_j, uint64_t *out_dist,
                       int64_t *counts, void *workspace, size_t workspace_bytes, void *stream);
int mmr_hash_cross_join(const uint64_t *queries, int64_t M, const uint64_t *refs, int64_t N, int H, int W,
                        const int32_t *thresholds_host, const uint32_t *ref_row_mask, int64_t cap, int32_t *out_q,
                        int32_t *out_ref, uint64_t *out_dist, int64_t *counts, void *workspace, size_t workspace_bytes,
                        void *stream);

/* ------------------------------------------------------------------------------------------
 * Perceptual hashes of decoded images: the input of the joins above, computed on the device  (replaces the per-file
 * imagehash.phash / dhash / whash calls of tool/find_repeated_in_same_folder.py:8-19; hash_size 8 or 16, every other
 * imagehash argument at its default).
 *
 * With L = Pillow's convert("L") ((R*19595 + G*38470 + B*7471 + 0x8000) >> 16; a one-channel image is L itself) and
 * R(w, h) = L.resize((w, h), LANCZOS) (horizontal pass, round and clip to uint8, vertical pass, round and clip), hs = hash_size:
 *   dhash: p = R(hs+1, hs); bit[r][c] = p[r][c+1] > p[r][c].
 *   phash: n = 4 hs, p = R(n, n); d[u][v] = 4 sum_y sum_x p[y][x] cos(pi(2y+1)u/2n) cos(pi(2x+1)v/2n) for u, v < hs, summed in
 *          fp64 against cos_table; med = the mean of the two middle d; eps = 2^-32 d[0][0]; bit = (d - med) > eps.
 *          Status bit MMR_IMAGE_HASH_PHASH_NEAR_MEDIAN: some |d - med| <= eps, where imagehash's own bit (d > med) depends
 *          on its summation order (flat images, 1 x 1 images).
 *   whash: S = max(2^floor(log2(min(W, H))), hs), p = R(S, S), s[i][j] = the integer sum of block (i, j) of side S / hs;
 *          with a <= b the two middle s, bit = 2 s > a + b (imagehash's Haar rule restated in integers: DESIGN.md section 3).
 *          Status bit MMR_IMAGE_HASH_WHASH_TIED_MEDIAN: a == b, where imagehash's bit of a block equal to the median is
 *          floating-point noise; the integer rule gives 0.
 * Every byte of p equals Pillow's: the resize is its 8-bit fixed-point convolution with the host's coefficient tables
 * (preprocess.resample_tables(filter="lanczos"): bounds int32[out][2] = (first input index, taps), coeffs int32[out][k],
 * k a multiple of 4 with zero padding, |coefficient| < 2^23, 16-byte aligned), as in mmr_preprocess_batch_ex.
 *
 * out[B, K, Wd] uint64: K = popcount(kinds), rows in the order phash, dhash, whash; Wd = hs*hs/64 words per hash; element
 * [0][0] of a hash is bit 63 of word 0 (numpy's bits.flatten(), most significant bit first): the layout of the joins and
 * of str(imagehash).  status[B] int32, 0 for an ordinary image; MMR_IMAGE_HASH_BAD_DESC: the descriptor was rejected on
 * the device (size, null or misaligned table, scratch outside the workspace), its hashes are 0 and nothing else was touched.
 *
 * `desc_dev` is a DEVICE array of B descriptors (B <= 65535).  Sides are 1 .. MMR_IMAGE_HASH_MAX_SIDE = 16384: one L row plus
 * slack must fit the 32 KiB of LDS the horizontal pass gives itself (five workgroups per CU).  scratch_off: where this
 * image's scratch starts inside `workspace`, a multiple of 16; regions of mmr_image_hash_scratch_bytes(H, W, hash_size, kinds)
 * bytes (0: bad arguments) that do not overlap.  mmr_image_hashes_workspace_bytes reads a HOST copy of the descriptors,
 * checks them and returns the workspace size they need (0: bad arguments, mmr_last_error() says which).
 * debug_w (nullable, test aid): receives the S x S bytes of whash's resized image, which are otherwise never stored;
 * mmr_image_hash_scratch_layout gives the offsets, from scratch_off, of {block sums int64[hs][hs], dhash plane
 * uint8[hs][hs+1], phash plane uint8[4hs][4hs], and the three horizontal-pass planes [H][hs+1], [H][4hs], [H][S]}.
 * The workspace need not be cleared.  Asynchronous on `stream`, no allocation, no host read; hipGraph-capturable.
 * The pixels are read from memory once, for all three kinds.  DESIGN.md section 3 has the kernels and what bounds them. */
#define MMR_HASH_PHASH 1
#define MMR_HASH_DHASH 2
#define MMR_HASH_WHASH 4
#define MMR_IMAGE_HASH_MAX_SIDE 16384
#define MMR_IMAGE_HASH_PHASH_NEAR_MEDIAN 1
#define MMR_IMAGE_HASH_WHASH_TIED_MEDIAN 2
#define MMR_IMAGE_HASH_BAD_DESC 0x40000000
typedef struct {
    const uint8_t *img;                              /* uint8 [H, W, channels], rows contiguous */
    const int32_t *hb_d, *hc_d, *vb_d, *vc_d;        /* dhash: W -> hs+1 columns, H -> hs rows */
    const int32_t *hb_p, *hc_p, *vb_p, *vc_p;        /* phash: W -> 4hs, H -> 4hs */
    const int32_t *hb_w, *hc_w, *vb_w, *vc_w;        /* whash: W -> S, H -> S */
    const double *cos_table;                         /* [hs][4hs]: cos(pi (2x+1) v / (8 hs)) */
    uint8_t *debug_w;                                /* nullable: uint8 [S, S] */
    int64_t scratch_off;
    int32_t H, W, channels, hk_d, vk_d, hk_p, vk_p, hk_w, vk_w, reserved;
} mmr_image_hash_desc;
size_t mmr_image_hash_scratch_bytes(int H, int W, int hash_size, int kinds);
int mmr_image_hash_scratch_layout(int H, int W, int hash_size, int kinds, int64_t *offsets);
size_t mmr_image_hashes_workspace_bytes(const void *desc_host, int B, int hash_size, int kinds);
int mmr_image_hashes(const void *desc_dev, int B, int hash_size, int kinds, uint64_t *out, int32_t *status, void *workspace,
                     size_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------------------------------
 * JPEG decode: baseline files to RGB, every byte Pillow's  (replaces `Image.open(f).convert("RGB")`, reference
 * code/search_image.py:127,155, CLIP/lab3.py:28, tool/find_repeated_in_same_folder.py:12, tool/find_repeated.py:11-15).
 *
 * Two stages.  The serial one runs on the HOST: mmr_jpeg_probe reads the headers, mmr_jpeg_entropy_decode Huffman-decodes
 * a batch on up to 16 threads into int16 coefficients.  The parallel one runs on the DEVICE: mmr_jpeg_decode_device
 * dequantises, inverts the DCT (libjpeg's jidctint), upsamples the chroma (libjpeg's fancy upsampling) and converts
 * YCbCr to RGB, all in integers (DESIGN.md section "JPEG decode" has the arithmetic).  The bytes are those of Pillow
 * (libjpeg-turbo's defaults) whenever |coefficient * quantiser| < 2^15, which holds for every file an encoder wrote
 * from 8-bit pixels; outside that range libjpeg-turbo's SIMD code keeps 16 bits of the product and no parity is claimed.
 *
 * Scope: SOF0 / SOF1 with Huffman coding, 8-bit samples, 8-bit DQT; 1 component (returned as RGB, the three bytes equal) or
 * 3 components YCbCr with luma sampling 1x1, 2x1 or 2x2 and chroma 1x1; one interleaved scan; DRI and RST0-7; up to 4 DC and
 * 4 AC tables; APPn / COM skipped, fill bytes before markers, trailing bytes after EOI; sides 1 .. MMR_JPEG_MAX_SIDE.
 * Status per image: MMR_JPEG_UNSUPPORTED for a valid file outside that scope (progressive, arithmetic, lossless, 12-bit,
 * 4 components, other sampling, several scans, DNL, 16-bit DQT, an Adobe transform other than 1 or component ids R, G, B
 * without JFIF on 3 components, a zero dimension), MMR_JPEG_CORRUPT for truncated data, an undefined Huffman code, a
 * coefficient index past 63, a missing table, a wrong restart marker or a segment length past the end.  A bad image never
 * disturbs its neighbours.  No parity with Pillow is claimed for corrupt files.
 *
 * mmr_jpeg_probe (host, no device): fills `info` from the headers up to the first scan and returns info->status.
 * blocks_c is component c's padded block grid, (mcus_y v_c) x (mcus_x h_c) blocks with h_0 = hmax, v_0 = vmax and chroma
 * 1 x 1; coef_bytes = 128 (blocks0 + blocks1 + blocks2).  For a status other than 0 only W, H (as far as read) and status are set.
 * mmr_jpeg_entropy_decode (host, no device): all pointers are HOST memory.  datas_host: B pointers to the files,
 * sizes_host their lengths, infos_host the probes' results.  Image i's coefficients go to coef_host + coef_off_host[i] BYTES
 * (a multiple of 16; spans of infos_host[i].coef_bytes that do not overlap): int16 [block][64] in natural (de-zigzagged)
 * order, component after component, each component's blocks in raster order over its padded grid; the span is zero-filled
 * first.  qt_host: uint16 [B][3][64], component c's quantisation table in natural order.  status_host[B]: the codes above;
 * a row whose probe status is not 0 keeps it and is not decoded.  threads: 1..16.  Returns MMR_OK or MMR_EINVAL.
 *
 * mmr_jpeg_decode_device: `desc_dev` is a DEVICE array of B descriptors (B <= 65535).  A row with ncomp = 0 (a host status
 * other than 0) has no blocks and is skipped.  coef_off / qt_off are BYTE offsets into coef_dev / qt_dev, multiples of 16;
 * plane_off is where the row's uint8 component planes start in `ws` (a multiple of 16): component after component, plane c
 * (mcus_y v_c 8) rows of (mcus_x h_c 8) bytes, blocks0 * 64 + ... bytes in all.  block_first / run_first are the prefix sums
 * over the batch of the rows' block counts and of ceil(H W / 4), the units the two kernels share out.  out: uint8 [H, W, 3],
 * 4-byte aligned.  mmr_jpeg_workspace_bytes reads a HOST copy of the descriptors, checks them (sizes, sampling, alignment,
 * the prefixes, planes that overlap) and returns the bytes `ws` must hold (0: bad arguments or B = 0, mmr_last_error()
 * says which).  Two launches: (1) dequantise + inverse DCT into the planes, (2) upsample + colour into `out`.  The planes stay
 * in `ws` afterwards (a test aid).  Asynchronous on `stream`, no allocation, no host read; hipGraph-capturable.
 *
 * The Huffman stage on the DEVICE (optional; the host stage stays the default and the arbiter).  It writes the coefficient
 * layout of mmr_jpeg_entropy_decode, so mmr_jpeg_decode_device consumes either.
 * mmr_jpeg_scan_prepare (host, no device): probes B files (headers only; the scan's bytes are not walked) and fills, per
 * image, infos_host (as mmr_jpeg_probe), status_host, qt_host (uint16 [B][3][64], as mmr_jpeg_entropy_decode writes it),
 * one mmr_jpeg_scan_desc and MMR_JPEG_TABLE_BYTES of tables_host: up to 6 Huffman tables in the kernel's look-up form (per
 * table 512 uint16 of the 9-bit fast table, maxcode and delta of lengths 10..16 as int32, 256 symbol bytes).  scan_start is
 * where the entropy-coded bytes begin in the file, scan_bytes how many follow up to the END OF THE FILE; td_c / ta_c are the
 * table slots (0..5) of component c.  The offsets pack the batch: bytes_off / state_off (multiples of 16, scan_bytes rounded
 * up to 16 apart) are where the caller copies the scan's bytes into bytes_dev and where the row's states may go in `ws`;
 * tables_off = i * MMR_JPEG_TABLE_BYTES; coef_off the running sum of coef_bytes, as mmr_jpeg_entropy_decode's caller lays
 * them out.  A caller may move a span by rewriting its offset (multiples of 16).  A row whose probe status is not 0 keeps that
 * status and gets an empty descriptor (ncomp = 0); a scan longer than MMR_JPEG_DEVICE_MAX_SCAN bytes gets
 * MMR_JPEG_DECLINED, which bounds the time one file can hold a compute unit.  Returns MMR_OK or MMR_EINVAL.
 *
 * mmr_jpeg_entropy_decode_device: one workgroup per image.  SUBSEQUENCE k of an image covers scan bytes
 * [k S, (k + 1) S) COUNTED FROM THE FIRST ENTROPY-CODED BYTE (bytes_dev + bytes_off), S = subseq_bytes, a power of two in
 * 16..1024.  Lanes decode subsequences speculatively in rounds until no entry state (bit position, block slot, zigzag
 * index) changes, at most max_rounds (1..1024) rounds; a final pass decodes once more from the converged states under the
 * host stage's rules and writes int16 [block][64] in natural order at coef_dev + coef_off, component after component, raster
 * order over the padded grid, after zero-filling the span itself; DC values are the per-component running sums within each
 * restart segment, low 16 bits.  stat_dev: int32 [B][4] = status, rounds used, subsequences, 0.  Status 0 only if every rule
 * of the host stage held (no undefined code, DC category <= 15, no index past 63, no bit read past a marker, fewer than 8
 * bits and the right RSTn / EOI at every restart and at the end, the block total reached exactly) and the final pass
 * reproduced every converged state; then the coefficients are those of mmr_jpeg_entropy_decode.  ANYTHING ELSE IS
 * MMR_JPEG_DECLINED (no convergence within max_rounds, any irregularity, a marker other than EOI behind the last block, more
 * than 16 fill bytes before a marker, an MCU boundary inside the last byte before a restart marker that is not the
 * interval's): the device never answers CORRUPT or UNSUPPORTED itself, the host stage decides declined rows, whose
 * coefficient spans hold unspecified values.  A row with an empty descriptor reports the descriptor's status.  Every read of
 * scan bytes is checked against scan_bytes and every coefficient write against the block grid.  `ws` holds the states of rows
 * with more than 2048 subsequences (16 bytes per subsequence at state_off); mmr_jpeg_entropy_workspace_bytes reads a HOST
 * copy of the descriptors, checks them and returns the bytes needed for that S (0: bad arguments, mmr_last_error() says
 * which).  One launch; asynchronous on `stream`, no allocation, no host read; hipGraph-capturable. */
#define MMR_JPEG_OK 0
#define MMR_JPEG_UNSUPPORTED 1
#define MMR_JPEG_CORRUPT 2
#define MMR_JPEG_DECLINED 3
#define MMR_JPEG_MAX_SIDE 16384
#define MMR_JPEG_DEVICE_MAX_SCAN 4194304
#define MMR_JPEG_TABLE_BYTES 8064
typedef struct {
    int32_t W, H, ncomp, hmax, vmax, mcus_x, mcus_y, status;
    int32_t blocks0, blocks1, blocks2, reserved;
    int64_t coef_bytes;
} mmr_jpeg_info;
typedef struct {
    uint8_t *out;
    int64_t coef_off, qt_off, plane_off, block_first, run_first;
    int32_t W, H, ncomp, hmax, vmax, mcus_x, mcus_y, reserved;
} mmr_jpeg_desc;
int mmr_jpeg_probe(const uint8_t *data, int64_t size, mmr_jpeg_info *info);
int mmr_jpeg_entropy_decode(const void *datas_host, const int64_t *sizes_host, int B, const mmr_jpeg_info *infos_host,
                            int16_t *coef_host, const int64_t *coef_off_host, uint16_t *qt_host, int32_t *status_host,
                            int threads);
size_t mmr_jpeg_workspace_bytes(const void *desc_host, int B);
int mmr_jpeg_decode_device(const void *desc_dev, int B, const int16_t *coef_dev, const uint16_t *qt_dev, void *ws,
                           size_t ws_bytes, void *stream);
typedef struct {
    int64_t scan_start, scan_bytes, bytes_off, tables_off, coef_off, state_off;
    int32_t status, restart, ncomp, hmax, vmax, mcus_x, mcus_y, blocks0, blocks1, blocks2;
    int32_t td0, td1, td2, ta0, ta1, ta2;
} mmr_jpeg_scan_desc;
int mmr_jpeg_scan_prepare(const void *datas_host, const int64_t *sizes_host, int B, mmr_jpeg_info *infos_host,
                          mmr_jpeg_scan_desc *scan_desc_host, void *tables_host, uint16_t *qt_host, int32_t *status_host);
size_t mmr_jpeg_entropy_workspace_bytes(const void *scan_desc_host, int B, int subseq_bytes);
int mmr_jpeg_entropy_decode_device(const void *scan_desc_dev, int B, const void *bytes_dev, const void *tables_dev,
                                   int16_t *coef_dev, int32_t *stat_dev, int subseq_bytes, int max_rounds, void *ws,
                                   size_t ws_bytes, void *stream);

/* ------------------------------------------------------------------------------------------
 * JPEG encode: uint8 pixels on the device to baseline files, every byte Pillow's  (replaces the download plus
 * `img.save(path, 'JPEG', quality=95)`, reference tool/Image format conversion.py:41-62, the RGBA paste over white of
 * :49-53 included).
 *
 * Two stages, the decode's in the other direction.  The parallel one runs on the DEVICE: mmr_jpeg_encode_device converts
 * RGB to YCbCr (libjpeg's rgb_ycc), box-downsamples the chroma, expands the edges, runs the forward DCT (libjpeg's
 * jfdctint) and divides by the quantisation table, all in integers (DESIGN.md section "JPEG encode" has the arithmetic).
 * The serial one runs on the HOST: mmr_jpeg_entropy_encode Huffman-codes a batch on up to 16 threads with the Annex K
 * tables and frames the files.  The bytes are those of `Image.fromarray(x).save(f, 'JPEG', quality=q, subsampling=s)`
 * (libjpeg-turbo's defaults: the slow integer DCT, standard Huffman tables, JFIF 1.01 without density).
 *
 * Scope: greyscale (1 component) or YCbCr (3 components, luma sampling 1x1, 2x1 or 2x2, chroma 1x1); one interleaved
 * scan; an optional restart interval in MCUs; sides 1 .. MMR_JPEG_MAX_SIDE.  No optimised tables, no progressive output,
 * no metadata.
 *
 * mmr_jpeg_quant_tables (host): libjpeg's quality scaling of the Annex K tables, quality 1..100, into qt_luma / qt_chroma
 * (uint16 [64] each, NATURAL order).  Returns MMR_OK or MMR_EINVAL.
 *
 * mmr_jpeg_encode_device: `desc_dev` is a DEVICE array of B descriptors (B <= 65535), every one an image (no empty rows).
 * src: uint8 pixels on the device, row y at src + y * row_stride BYTES, `channels` interleaved bytes per pixel: 1 (grey;
 * ncomp must be 1), 3 (RGB) or 4 (RGBA, composited over `background` = R | G << 8 | B << 16 while it is loaded, as
 * Image.paste with the alpha band as mask does).  ncomp / hmax / vmax / mcus_x / mcus_y as in mmr_jpeg_info.  coef_off /
 * qt_off are BYTE offsets into coef_dev / qt_dev, multiples of 16; qt_dev holds uint16 [3][64] per offset (component c's
 * table in natural order, the layout mmr_jpeg_entropy_decode writes); plane_off is where the row's uint8 component planes
 * go in `ws` (a multiple of 16), laid out as mmr_jpeg_decode_device reads them.  block_first is the prefix sum of the rows'
 * block counts, run_first that of their 4-sample plane runs (16 per block).  total_blocks / total_runs are the batch's
 * totals: the grids are exact functions of them.  Two launches: (1) pixels -> planes: colour, downsampling, edge expansion;
 * (2) planes -> int16 coefficients at coef_dev + coef_off in the layout mmr_jpeg_entropy_decode writes, the luma blocks
 * outside the image (dummy blocks: DC of the block before them in the MCU, AC zero) included.  The planes stay in `ws`
 * afterwards (a test aid).  mmr_jpeg_encode_workspace_bytes reads a HOST copy of the descriptors, checks them (sizes,
 * sampling, channels, alignment, the prefixes, planes that overlap, totals within 2^31 - 1 launch units) and returns the
 * bytes `ws` must hold (0: bad arguments, mmr_last_error() says which).  Asynchronous on `stream`, no allocation, no host
 * read; hipGraph-capturable.
 *
 * mmr_jpeg_encode_bound (host): the most bytes a file of this geometry can take, headers included (0 for an info outside
 * the scope above).
 * mmr_jpeg_entropy_encode (host, no device): all pointers are HOST memory.  Image i's coefficients are read at coef_host +
 * coef_off_host[i] BYTES (a multiple of 2) in the layout above, infos_host[i] gives its geometry (status must be 0), qt_host
 * is uint16 [B][3][64] (row i's tables: [0] goes out as DQT 0, [1] as DQT 1 for 3 components).  restart_interval: 0 (none) ..
 * 65535 MCUs.  The file goes to out_host + out_off_host[i], at most out_cap_host[i] bytes; out_bytes_host[i] is its length.
 * status_host[i]: MMR_JPEG_OK; MMR_JPEG_NO_ROOM when the file does not fit out_cap_host[i] (out_bytes_host[i] = 0, nothing
 * is written past the capacity, the other rows are unaffected); MMR_JPEG_UNSUPPORTED for a geometry outside the scope, a
 * table entry outside 1..255, an AC coefficient outside +-1023 or a DC difference outside +-2047 (what the baseline tables
 * cannot code).  threads: 1..16.  Returns MMR_OK or MMR_EINVAL. */
#define MMR_JPEG_NO_ROOM 4
typedef struct {
    const uint8_t *src;
    int64_t row_stride, coef_off, qt_off, plane_off, block_first, run_first;
    int32_t channels, background, W, H, ncomp, hmax, vmax, mcus_x, mcus_y, reserved;
} mmr_jpeg_encode_desc;
int mmr_jpeg_quant_tables(int quality, uint16_t *qt_luma, uint16_t *qt_chroma);
size_t mmr_jpeg_encode_workspace_bytes(const void *desc_host, int B);
int mmr_jpeg_encode_device(const void *desc_dev, int B, const uint16_t *qt_dev, int16_t *coef_dev, void *ws, size_t ws_bytes,
                           int64_t total_blocks, int64_t total_runs, void *stream);
int64_t mmr_jpeg_encode_bound(const mmr_jpeg_info *info);
int mmr_jpeg_entropy_encode(const int16_t *coef_host, const int64_t *coef_off_host, const mmr_jpeg_info *infos_host,
                            const uint16_t *qt_host, int B, int restart_interval, uint8_t *out_host,
                            const int64_t *out_off_host, const int64_t *out_cap_host, int64_t *out_bytes_host,
                            int32_t *status_host, int threads);

/* out[Q,N] (fp32) = (float)(dot64 * scale): the materialised score matrix for small N. */
int mmr_similarity(const void *q, const void *gallery, mmr_dtype dtype, int Q, int64_t N, int E, float scale,
                   float *out, void *stream);

/* In-place row-wise x /= ||x||_2 (no epsilon, like the reference). */
int mmr_l2norm_rows(void *x, mmr_dtype dtype, int64_t rows, int E, void *stream);

/* Merge `parts` per-shard lists [parts,Q,k] (global int64 ids, fp64 dots; id < 0 = empty slot, its dot is ignored)
 * into one [Q,k] list with the same ordering.  Used after the RCCL all-gather.  k <= 64 and parts * k <= 1024
 * (MMR_EINVAL otherwise, before any launch).  Entries with a NaN dot are dropped, -inf dots are kept with their ids.
 * An id that appears in several parts WITH THE SAME DOT (overlapping shards) is returned once; the same id with
 * different dots is outside the contract (the kernel retires an id at its first pick)
 * [test_merge_on_synthetic_lists, test_argument_validation_happens_before_any_launch]. */
int mmr_topk_merge(const int64_t *idx_parts, const double *dot_parts, int parts, int Q, int k, float scale,
                   int64_t *idx, float *score, double *dot64, void *stream);

/* The same exchange with ONE message per rank: mmr_topk_pack writes packed[Q,k,2] int64 = (local id + row_offset or -1,
 * fp64 dot bits) from mmr_cosine_topk's idx/dot64; after the all-gather of those messages ([parts,Q,k,2])
 * mmr_topk_merge_packed ranks them.  Two launches around the collective instead of six tensor ops. */
int mmr_topk_pack(const int32_t *idx, const double *dot64, int Q, int k, int64_t row_offset, int64_t *packed, void *stream);
int mmr_topk_merge_packed(const int64_t *packed_parts, int parts, int Q, int k, float scale, int64_t *idx, float *score,
                          double *dot64, void *stream);

/* Multi-GPU leg for hosts without torch.distributed: one process per GPU; rank r searches its
 * gallery rows with mmr_cosine_topk(_ex), packs its list with mmr_topk_pack(row_offset = first global row of the shard),
 * then ONE RCCL all-gather over xGMI of the packed messages (mmr_allgather_topk_packed) and mmr_topk_merge_packed:
 *
 *     mmr_cosine_topk_ex(q, shard, ..., idx32, score, dot64, ...);          // local top-k, int32 local ids
 *     mmr_topk_pack(idx32, dot64, Q, k, row_offset, packed, stream);        // [Q,k,2] int64 = (global id | -1, dot bits)
 *     mmr_allgather_topk_packed(comm, packed, Q, k, parts, stream);         // [world,Q,k,2]   -- the collective
 *     mmr_topk_merge_packed(parts, world, Q, k, scale, idx64, score, dot64, stream);
 *
 * librccl is bound at run time (dlopen; MMR_RCCL_LIB overrides the name), so a single-GPU user needs no RCCL.  The Python
 * package performs the SAME exchange (one message of 2*Q*k int64 per rank) through torch.distributed's "nccl" (= RCCL)
 * backend (search.ShardedGalleryIndex.search_async). */
typedef struct mmr_comm mmr_comm;
#define MMR_COMM_ID_BYTES 128
/* rank 0: fill MMR_COMM_ID_BYTES bytes of HOST memory; the host program hands them to every rank (file, socket, MPI ...) */
int mmr_comm_unique_id(void *id_host);
/* collective over all ranks; binds the communicator to the calling thread's current HIP device */
int mmr_comm_init(int rank, int world, const void *id_host, mmr_comm **out);
void mmr_comm_destroy(mmr_comm *c);
/* packed_local [Q,k,2] int64 (device, mmr_topk_pack layout) -> packed_parts [world,Q,k,2] (device), asynchronous on
 * `stream`: ONE ncclAllGather.  Feed the result to mmr_topk_merge_packed(parts = world). */
int mmr_allgather_topk_packed(mmr_comm *c, const int64_t *packed_local, int Q, int k, int64_t *packed_parts, void *stream);
/* Unpacked form (kept for callers that hold separate arrays): idx_local / dot_local [Q,k] (device, GLOBAL int64 ids) ->
 * idx_parts / dot_parts [world,Q,k]; the two arrays travel as one grouped pair of all-gathers.  -> mmr_topk_merge. */
int mmr_allgather_topk(mmr_comm *c, const int64_t *idx_local, const double *dot_local, int Q, int k,
                       int64_t *idx_parts, double *dot_parts, void *stream);

/* Tip-Adapter logits, fused (replaces reference code/main_custom.py:111,124-127 and
 * code/utils.py:182-186):  tip = 100*F@W + alpha * (exp(-(beta - beta*(F@Kc))) @ V * 10).
 *   features[N,E]; clip_weights_t[C,E] = W^T; cache_keys_t[S,E] = Kc^T (all `dtype`);
 *   cache_values[S,C] fp32; tip_logits[N,C] fp32; clip_logits[N,C] fp32 (nullable) = 100*F@W.  C <= 64. */
int mmr_tip_adapter_logits(const void *features, const void *clip_weights_t, const void *cache_keys_t,
                           const float *cache_values, mmr_dtype dtype, int64_t N, int E, int C, int S, float alpha,
                           float beta, float *tip_logits, float *clip_logits, void *stream);

/* Tip-Adapter-F: one training step of the learnable cache keys (replaces the body of the loop of reference
 * code/main_custom.py:166-189: adapter forward, cross-entropy, backward, AdamW).  The encoder is frozen, so the step is
 *   A = F W^T,  P = exp(beta*A - beta),  L = 100 F Wc + 10 alpha P V,  loss = mean_b(logsumexp(L_b) - L_b[y_b]),
 *   G = (softmax(L) - onehot(y)) / B,  dA = beta P (10 alpha G V^T),  g = dA^T F,  then torch's AdamW on W with g:
 *   W *= 1 - lr*wd;  m += (g - m)(1 - beta1);  v = v*beta2 + (1 - beta2) g g;
 *   W -= lr / (1 - beta1^step) * m / (sqrt(v) / sqrt(1 - beta2^step) + eps).
 * features[B,E] and clip_weights_t[C,E] = Wc^T (`dtype`, widened exactly to fp32); targets[B] int64; cache_values[S,C]
 * fp32 (any matrix, not only one-hot); weight[S,E] fp32 = adapter.weight = cache_keys^T, the master copy; exp_avg,
 * exp_avg_sq[S,E] fp32 (both NULL: no update, weight untouched).  1 <= C <= 64, 1 <= S <= 16384, E as mmr_tip_adapter_logits.
 * The caller passes this step's learning rate (a schedule is the host's) and `step`, counted from 1.
 * Outputs: loss[1]; pred[B] int32 (nullable) = argmax_c L, lowest c on a tie; grad_out[S,E] (nullable) = g.
 * A row whose label lies outside [0,C) takes no part (loss_b = 0, its row of G = 0, the divisor stays B) and sets bit 0
 * of *status (nullable; the call never clears it).  Every sum runs in a fixed order with fp32 accumulation (the exact
 * fp32-input MFMA): equal inputs give equal bits, whatever the workspace held.  Two launches, no synchronisation.
 * B == 0 returns MMR_OK and touches nothing. */
size_t mmr_tip_adapter_f_workspace_bytes(int64_t B, int E, int C, int S);
int mmr_tip_adapter_f_step(const void *features, const int64_t *targets, mmr_dtype dtype, int64_t B, int E, int C, int S,
                           const void *clip_weights_t, const float *cache_values, float *weight, float *exp_avg,
                           float *exp_avg_sq, float alpha, float beta, double lr, double beta1, double beta2, double eps,
                           double weight_decay, int64_t step, float *loss, int32_t *pred, float *grad_out, int32_t *status,
                           void *workspace, size_t workspace_bytes, void *stream);

/* Tip-Adapter (beta, alpha) grid search: every tensor step of reference code/utils.py:159-206 (`search_hp`) with
 * `get_similarity` + `find_thresholds` + `eval_threshold` (code/main_custom.py:27-105) and the counts behind `cls_f1` and
 * `cls_acc` (code/utils.py:15-76), for nb x na grid points in three launches.
 * Stage 1, floating point, computed once and returned:
 *   A = F K (never written);  L0[N,C] = 100 F Wc;  cache[nb,N,C] = 10 * sum_s exp(beta_b A[n,s] - beta_b) V[s,c], s ascending.
 * features[N,E] and clip_weights_t[C,E] = Wc^T (`dtype`, widened exactly to fp32); keys_t[S,E] = K^T in `keys_dtype`, which
 * is `dtype` or MMR_F32 (the master weight of mmr_tip_adapter_f_step); cache_values[S,C] fp32; betas[nb], alphas[na] fp32;
 * labels[N] int64.  1 <= C <= 64, 1 <= S <= 16384, E as mmr_tip_adapter_logits, nb, na <= 65535.
 * The logit of grid point (b, a) is DEFINED as fl32(L0 + fl32(cache[b] * alphas[a])): one rounded multiply, one rounded add.
 * Stage 2 is an exact function of those logits widened to fp64:
 *   conf[nb,na,C,C] int32, [target, pred], pred = the lowest class at the row maximum;
 *   per class c, with pos = column c of the rows labelled c and neg = column c of the other rows:
 *     lo = max(min pos, min neg), hi = min(max pos, max neg), num_vals = int((hi - lo) * 10),
 *     t = np.linspace(lo, hi, num_vals): t_i = fl(fl(i * step) + lo), step = (hi - lo) / (num_vals - 1), t_last = hi,
 *     tp_i = #{pos >= t_i}, fp_i = #{neg >= t_i}, fn_i = #pos - tp_i, p = tp/(tp+fp), r = tp/(tp+fn), f1_i = ((2p)r)/(p+r),
 *     best = the first i whose f1_i is strictly above every earlier one, starting from 0.0 (0/0 is NaN and never wins);
 *   f1, threshold [nb,na,C] fp64 (0.0 when nothing beats 0); tp, fp, fn (at the best threshold), num_vals [nb,na,C] int32.
 * Degenerate classes have f1 = threshold = 0 and zero counts: pos or neg empty (num_vals = -1), hi < lo (num_vals keeps the
 * value int() gives, <= 0) and num_vals == 0.  A row whose label lies outside [0,C) takes no part and sets bit 0 of *status.
 * The two histograms of num_vals + 1 int32 bins each live in LDS, 64 KiB apiece, hence the cap: a point with
 * num_vals > MMR_TIP_GRID_MAX_VALS gets f1 = threshold = NaN, its num_vals, and bit 1 of *status (the call never clears
 * *status).  Equal inputs give equal bits, whatever the outputs held before.  No workspace is needed at present (the
 * query returns 0 and `workspace` may be NULL).  nb == 0 or na == 0 returns MMR_OK and touches nothing. */
#define MMR_TIP_GRID_MAX_VALS 16383
size_t mmr_tip_adapter_grid_workspace_bytes(int64_t N, int E, int C, int S, int nb, int na);
int mmr_tip_adapter_grid(const void *features, const int64_t *labels, mmr_dtype dtype, int64_t N, int E, int C, int S,
                         const void *clip_weights_t, const void *keys_t, mmr_dtype keys_dtype, const float *cache_values,
                         const float *betas, int nb, const float *alphas, int na, float *L0, float *cache, int32_t *conf,
                         double *f1, double *threshold, int32_t *tp, int32_t *fp, int32_t *fn, int32_t *num_vals,
                         int32_t *status, void *workspace, size_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------------------------------
 * Encoder towers  (replaces model.encode_image / encode_text of the `clip` package and
 * CLIPModel.get_image_features of transformers; arithmetic per SURVEY.md Appendix A).
 * ---------------------------------------------------------------------------------------- */

typedef struct {
    int kind;        /* 0 = CLIP vision, 1 = CLIP text, 2 = BERT-style text classifier (Taiyi) */
    int width;       /* d, multiple of 128 */
    int layers;
    int heads;       /* width / 64 */
    int mlp;         /* multiple of 128 */
    int tokens;      /* vision: 1 + (image_size/patch)^2; text: context length; kind 2: max positions */
    int embed_dim;   /* E, multiple of 128 */
    int image_size;  /* vision only */
    int patch;       /* vision only */
    int vocab;       /* text only */
    float ln_eps;
    int fold_ln;     /* kinds 0/1: 1 = the per-block LayerNorms are folded into the GEMMs that consume them.
                      * The blob then carries, per layer, QKV_W = bf16(W_qkv * ln1.w[None,:]),
                      * QKV_B = W_qkv @ ln1.b + b_qkv, QKV_C[n] = sum_k float(QKV_W[n,k]) and the same for
                      * FC1_{W,B,C} with ln2; LN1_x / LN2_x are not read.  The GEMM epilogue applies
                      * rstd*(acc - mean*C) + B from row statistics of the fp32 residual stream
                      * (same arithmetic as LN-then-GEMM up to bf16 rounding of W*gamma instead of LN(h)).
                      * 0 = separate LayerNorm launches, original tensors.  Must be 0 for kind 2. */
} mmr_tower_cfg;

/* Tensors of the weight blob.  Matrices are bf16 row-major [out,in]; vectors/embeddings fp32
 * except TOK_EMB (bf16 [vocab,d]).  PATCH_W is [d, Kpad] with K = (c,ky,kx) order zero-padded
 * to a multiple of 64.  `layer` is ignored for non-per-layer tensors. */
typedef enum {
    MMR_P_PATCH_W = 0, MMR_P_CLS, MMR_P_POS, MMR_P_LN_PRE_W, MMR_P_LN_PRE_B,
    MMR_P_LN1_W, MMR_P_LN1_B, MMR_P_QKV_W, MMR_P_QKV_B, MMR_P_OUT_W, MMR_P_OUT_B,
    MMR_P_LN2_W, MMR_P_LN2_B, MMR_P_FC1_W, MMR_P_FC1_B, MMR_P_FC2_W, MMR_P_FC2_B,
    MMR_P_LN_FINAL_W, MMR_P_LN_FINAL_B, MMR_P_PROJ, MMR_P_TOK_EMB,
    /* BERT-style text encoder only (kind 2): */
    MMR_P_TYPE_EMB, /* fp32 [2,d] token-type embeddings (row 0 is used) */
    MMR_P_POOL_W,   /* bf16 [d,d] pooler dense */
    MMR_P_POOL_B,   /* fp32 [d] */
    MMR_P_PROJ_B,   /* fp32 [E] classifier bias (MMR_P_PROJ is the classifier weight [E,d]) */
    /* fold_ln towers only, per layer: */
    MMR_P_QKV_C,    /* fp32 [3d] row sums of the gamma-folded QKV weight */
    MMR_P_FC1_C,    /* fp32 [mlp] row sums of the gamma-folded FC1 weight */
    MMR_P_COUNT
} mmr_param;

size_t mmr_tower_weights_bytes(const mmr_tower_cfg *cfg);
/* Byte offset/size of one tensor inside the blob; returns MMR_EINVAL if the tower has no such tensor. */
int mmr_tower_param_span(const mmr_tower_cfg *cfg, int param, int layer, size_t *offset, size_t *bytes);

typedef struct mmr_tower mmr_tower;

/* Workspace status word: every forward call (mmr_tower_forward / mmr_vit_encode_image / mmr_text_encode /
 * mmr_bert_forward*) zeroes the int32 at workspace offset 0 and the embedding kernels OR bits into it:
 *   bit 0 = a token id (or token type id) was out of range and was clamped.
 * The library never reads it back (no sync); a caller that feeds ids produced on the device reads it when it
 * chooses to synchronise.  Ids on the host are range-checked by the host shim before the call. */
#define MMR_STATUS_BAD_TOKEN_ID 1

/* `weights` is a device blob laid out per mmr_tower_param_span; it must outlive the tower.
 * Concurrency: a forward call only READS the tower and its weights; everything it writes lives in the caller's workspace and
 * output.  Forward calls that use DIFFERENT workspaces may therefore be in flight at once on different streams (two batches of
 * a gallery build: measured +10 % images/s on ViT-B/32 at batch 256, the second batch fills the CUs the first one's 150-200-tile
 * GEMM launches leave idle); calls that share a workspace must be stream-ordered.  The same holds for mmr_cosine_topk* and its
 * workspace (searches only read the gallery).  The Python shim calls such a workspace a "lane" (encode_image(lane=),
 * GalleryIndex.search(lane=)).
 * mmr_tower_set_shared_chip(t, 1) tells the tower that its forwards will run beside other work like that: the GEMM launches
 * then pick their tiles for efficiency per FLOP instead of for filling 256 CUs on their own (full 256x256 tiles where the
 * solo policy takes 256x192 ones, one workgroup per tile instead of 256 persistent ones for launches of a few long rounds:
 * +3-5 % images/s with two ViT-B/32 forwards in flight, -5 % with one).  Results do not
 * change (same K order per output element).  Set it while no forward of this tower is being issued. */
int mmr_tower_set_shared_chip(mmr_tower *t, int shared);
/* The forward entry points return pooled features only (one row per input), so from 2 048 padded token rows on they compute
 * the last block's queries, attention output, out-projection, LN2 and MLP for the pooled row of each input alone; only K
 * and V are still computed for every token.  Features are bit-identical to the full computation.  A tap of the last block
 * (tap_after == layers-1), fold_ln towers and BERT towers always run the full block.
 * mmr_tower_set_full_last_block(t, 1) forces the full block everywhere (an A/B aid; its initial value is taken from the
 * environment variable MMR_FULL_LAST_BLOCK=1 when the tower is created).  Set it while no forward of this tower is being
 * issued. */
int mmr_tower_set_full_last_block(mmr_tower *t, int on);
int mmr_tower_create(const mmr_tower_cfg *cfg, const void *weights, size_t weights_bytes, mmr_tower **out);
void mmr_tower_destroy(mmr_tower *t);
size_t mmr_tower_workspace_bytes(const mmr_tower *t, int batch);

/* pixels[B,3,S,S] NCHW contiguous (fp32 or bf16) -> out[B,E] (fp32, bf16 or fp16).
 * normalize != 0 applies the row L2 normalisation before the store. */
int mmr_vit_encode_image(mmr_tower *t, const void *pixels, mmr_dtype in_dtype, int B, void *out,
                         mmr_dtype out_dtype, int normalize, void *workspace, size_t workspace_bytes,
                         void *stream);

/* ids[N,T] int32 (EOT = largest id per row) -> out[N,E]. */
int mmr_text_encode(mmr_tower *t, const int32_t *ids, int N, void *out, mmr_dtype out_dtype, int normalize,
                    void *workspace, size_t workspace_bytes, void *stream);

/* BERT-style text encoder (kind 2): replaces `text_encoder(text).logits` of
 * BertForSequenceClassification (Taiyi-CLIP Chinese text tower; reference code/test_taiyi.py:12,24,
 * CLIP-Chinese/lab_chinese.py:81-93).  Post-LN blocks, exact GELU, full attention over all T tokens (the
 * reference passes no attention_mask), pooler = tanh(dense(first token)), classifier -> out[N,E].
 * ids[N,T] int32 with 1 <= T <= cfg.tokens.  tap/tap_after as in mmr_tower_forward (after block i). */
size_t mmr_bert_workspace_bytes(const mmr_tower *t, int N, int T);
int mmr_bert_forward(mmr_tower *t, const int32_t *ids, int N, int T, void *out, mmr_dtype out_dtype, int normalize,
                     int tap_after, float *tap, void *workspace, size_t workspace_bytes, void *stream);
/* The `text_encoder(**inputs)` form (reference CLIP/union_dataset.py:312-314, CLIP-Chinese/lab_chinese.py:90-92):
 * the tokenizer's whole output.  token_type_ids[N,T] int32 (nullable = all 0; values 0/1 select the type
 * embedding row); attention_mask[N,T] int32 (nullable = all 1; 0 = padding key: it receives no attention weight,
 * like HF's additive -inf mask; padded QUERY rows are still computed, as in HF, and do not reach the pooled
 * output, which reads token 0). */
int mmr_bert_forward_masked(mmr_tower *t, const int32_t *ids, const int32_t *token_type_ids,
                            const int32_t *attention_mask, int N, int T, void *out, mmr_dtype out_dtype, int normalize,
                            int tap_after, float *tap, void *workspace, size_t workspace_bytes, void *stream);

/* Same forward with a tap on the fp32 residual stream for stage-level parity tests:
 * tap_after = -1 copies h after the embedding (+pre-LN for vision); i >= 0 after block i.
 * tap[B*T, d] fp32 (nullable).  `input` is pixels (vision) or ids (text). */
int mmr_tower_forward(mmr_tower *t, const void *input, mmr_dtype in_dtype, int B, void *out,
                      mmr_dtype out_dtype, int normalize, int tap_after, float *tap, void *workspace,
                      size_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------------------------------
 * Preprocess  (replaces the PIL/torchvision `preprocess` applied per image at reference
 * code/search_image.py:127,155: Resize(BICUBIC) -> CenterCrop -> ToTensor -> Normalize).
 * ---------------------------------------------------------------------------------------- */

/* img: uint8 RGB [H,W,3].  The coefficient tables are Pillow's (precompute_coeffs +
 * normalize_coeffs_8bpc) for the S columns / rows of the centre-crop window, built on the host
 * (preprocess.py): bounds int32[S][2] = (first input index, taps), coeffs int32[S][k] in 22-bit
 * fixed point.  row0/rows = the input rows the vertical pass reads; tmp: uint8 [rows,S,3] scratch.
 * out: [3,S,S] fp32 or bf16 = ((u8/255) - mean) / std; out_u8 (nullable): the uint8 [S,S,3] crop. */
int mmr_preprocess_image(const uint8_t *img, int H, int W, int S, int row0, int rows, const int32_t *hbounds,
                         const int32_t *hcoeffs, int hk, const int32_t *vbounds, const int32_t *vcoeffs, int vk,
                         float mean0, float mean1, float mean2, float std0, float std1, float std2, uint8_t *tmp,
                         void *out, mmr_dtype out_dtype, uint8_t *out_u8, void *stream);

/* Batched form: B images of different sizes in one launch pair.  `desc` is a DEVICE array of B
 * descriptors; tables/pointers as in mmr_preprocess_image; out[B,3,S,S].  max_rows = max over images of
 * `rows` (sizes the grid). */
typedef struct {
    const uint8_t *img;
    const int32_t *hbounds, *hcoeffs, *vbounds, *vcoeffs;
    uint8_t *tmp;
    int32_t H, W, row0, rows, hk, vk;
} mmr_preprocess_desc;
int mmr_preprocess_batch(const void *desc, int B, int S, int max_rows, float mean0, float mean1, float mean2,
                         float std0, float std1, float std2, void *out, mmr_dtype out_dtype, void *stream);
/* Same, with max_width = the widest image of the batch (pixels): lets the horizontal pass stage whole input rows in LDS
 * (coalesced loads, ~1 global instruction per output pixel instead of 9).  The fast forms need every image's coefficient
 * rows padded with zero taps to a multiple of 4 (hk % 4 == 0, 16-byte aligned tables: what preprocess.py builds) and
 * S % 4 == 0; an image that does not qualify takes the byte-wise path inside the same launch.  Results are identical.
 * PRECONDITION of the fast forms: |coefficient| < 2^23 (they multiply on the 24-bit integer multiplier) -- true for every
 * table Pillow's normalize_coeffs_8bpc can produce (22 fractional bits, |weight| <= ~1.2); a caller with other tables
 * leaves hk unpadded (hk % 4 != 0) to stay on the 32-bit byte-wise path.  Nothing is read past the last byte of an image. */
int mmr_preprocess_batch_ex(const void *desc, int B, int S, int max_rows, int max_width, float mean0, float mean1, float mean2,
                            float std0, float std1, float std2, void *out, mmr_dtype out_dtype, void *stream);

/* ------------------------------------------------------------------------------------------
 * Train-time augmentation  (replaces RandomResizedCrop(S, BICUBIC) -> RandomHorizontalFlip -> ToTensor ->
 * Normalize of the reference's few-shot loader, code/custom.py:24-29).  The boxes are drawn on the host
 * (preprocess.random_resized_crop_params); the two calls below build each crop's Pillow coefficient tables on
 * the device and apply them: out equals Normalize(ToTensor(flip(img.crop(box).resize((S, S), BICUBIC)))) bit
 * for bit.  Neither call allocates; both take a stream and can be captured in a graph.
 * ---------------------------------------------------------------------------------------- */

/* One crop: rows [top, top+ch) x columns [left, left+cw) of the uint8 RGB image img[H,W,3], mirrored left-right
 * after the resize when flip != 0.  Many crops may name one image; images may differ in size.  tmp_off: where
 * this crop's intermediate rows (uint8 [ch,S,3]) lie in the scratch of mmr_augment_resample, in bytes, a
 * multiple of 16; the ranges of two crops must not overlap.  reserved: 0.  48 bytes. */
typedef struct {
    const uint8_t *img;
    int64_t tmp_off;
    int32_t H, W, top, left, ch, cw, flip, reserved;
} mmr_crop_desc;

/* Bytes of the tables of B crops: B * 2 * S * (8 + 4 * kmax); 0 for a bad argument. */
size_t mmr_augment_tables_bytes(int B, int S, int kmax);
/* Builds, in one launch, the horizontal (from cw) and vertical (from ch) tables of the full-box bicubic resize of
 * each of the B crops in the DEVICE array `desc` to S: Pillow's precompute_coeffs + normalize_coeffs_8bpc, every
 * double operation correctly rounded and unfused, so the integers are Pillow's.  tables (16-byte aligned):
 * bounds int32 [B][2][S][2] = (first input index relative to the crop, taps), then coeffs int32 [B][2][S][kmax]
 * in 22-bit fixed point, zero behind a row's taps; axis 0 is horizontal, 1 vertical.  A flipped crop's horizontal
 * row j is the row of S-1-j.  kmax: the largest Pillow ksize of the batch, ceil(2 * max(in / S, 1)) * 2 + 1 over
 * every ch and cw (in / S as (double)(float)in / S), rounded up to a multiple of 4; a crop whose ksize exceeds kmax,
 * or whose side is outside [1, 2^20], gets empty rows (taps 0).  B <= 65535, S <= 4096. */
int mmr_augment_tables(const void *desc, int B, int S, int kmax, void *tables, size_t tables_bytes, void *stream);
/* Applies those tables: horizontal pass (only the crop's rows and columns are read and staged; the 16-byte loads may
 * touch pixels right of the crop inside the same image, never a byte before the image or at or past H * W * 3),
 * then the vertical pass, /255, -mean, /std of mmr_preprocess_batch_ex.  out[B,3,S,S] fp32 or bf16; out_u8
 * (nullable, 4-byte aligned): the uint8 crops [B,S,S,3].  max_ch / max_cw: the largest ch / cw of the batch (size
 * the grid and the LDS plan).  scratch (16-byte aligned): every crop's [tmp_off, tmp_off + ch * S * 3 + 16) must lie
 * inside scratch_bytes; packed, that is sum over crops of align16(ch * S * 3), plus 16.  A crop's result does not
 * depend on the rest of the batch.  A crop that is not inside its image, exceeds max_ch / max_cw / kmax or leaves the
 * scratch is skipped (its outputs are not written): validate on the host, as preprocess.augment_batch does. */
int mmr_augment_resample(const void *desc, int B, int S, int kmax, int max_ch, int max_cw, const void *tables,
                         size_t tables_bytes, uint8_t *scratch, size_t scratch_bytes, float mean0, float mean1,
                         float mean2, float std0, float std1, float std2, void *out, mmr_dtype out_dtype,
                         uint8_t *out_u8, void *stream);

/* ------------------------------------------------------------------------------------------
 * Launch profiler (measurement aid for bench.py): HIP event pairs around every kernel launch of a
 * class, recorded on the launch stream.  Off by default.
 * ---------------------------------------------------------------------------------------- */
enum {
    MMR_PROF_GEMM = 0,       /* the three GEMM kernels (256-row, 128x128, 128x32), all epilogues */
    MMR_PROF_ATTENTION = 1,  /* attention_kernel / attention_stream_kernel */
    MMR_PROF_ROWWISE = 2,    /* LayerNorm / embedding / pooling / patch gather / output cast */
    MMR_PROF_SCAN = 3,       /* scan_kernel (gallery stream, HBM-bound) */
    MMR_PROF_FINALIZE = 4,   /* select / rescore / rank kernels (selection + exact re-rank) */
    MMR_PROF_EXACT = 5,      /* exhaustive exact kernels */
    MMR_PROF_CLASSES = 6
};
/* on != 0: reset and start recording up to max_launches launches; on == 0: stop. */
int mmr_prof_enable(int on, int max_launches);
/* Sum of event-pair durations (ms) and launch count of one class; synchronises those events. */
int mmr_prof_read(int cls, double *total_ms, long long *launches, long long *dropped);

/* ------------------------------------------------------------------------------------------
 * Kernel-level test hooks (used by tests/ to localise a parity failure; not part of the drop-in).
 * ---------------------------------------------------------------------------------------- */

/* out[M,N] = epilogue(A[M,K] . W[N,K]^T): epi 0 = +bias -> bf16, 1 = +bias, QuickGELU -> bf16,
 * 2 = fp32 out += acc + bias, 3 = plain fp32, 4 = +bias -> fp32, 5 = +bias, exact GELU -> bf16,
 * 6 = +bias, tanh -> bf16.  M,N multiples of 128, K multiple of 64. */
int mmr_debug_gemm(int epi, const void *A, const void *W, int M, int N, int K, const float *bias, void *out,
                   void *stream);
/* The LayerNorm-folded epilogues (mmr_tower_cfg.fold_ln), which mmr_debug_gemm refuses.  Row statistics are
 * [M][16] (sum, sum of squares) float pairs; a row's statistics are the sums of its 16 slots.
 *   epi 7: out_bf16 = rstd * (A . W^T - mean * colsum) + bias, mean / rstd from stats_in, inv_d = 1 / width, eps
 *   epi 8: the same, then QuickGELU
 *   epi 9: out_f32 += A . W^T + bias; xout_bf16[M,N] = bf16(out); stats_out = (sum, sumsq) partials of the new rows,
 *          one slot per column slab of the tile the launcher picks, the other slots zeroed
 * epi 7 / 8 read colsum[N], stats_in, inv_d, eps; epi 9 reads stats_out, xout; the others may be NULL / 0. */
int mmr_debug_gemm_fold(int epi, const void *A, const void *W, int M, int N, int K, const float *bias, void *out,
                        const float *colsum, const void *stats_in, float inv_d, float eps, void *stats_out,
                        void *xout, void *stream);
/* x_bf16[rows,d] = LayerNorm(h_f32[rows,d]) */
int mmr_debug_layernorm(const float *h, const float *w, const float *b, void *x, int64_t rows, int d, float eps,
                        void *stream);
/* the BERT tower's LayerNorm: h_f32[rows,d] = LayerNorm(h) in place, x_bf16[rows,d] = bf16(h) */
int mmr_debug_layernorm_inplace(float *h, const float *w, const float *b, void *x, int64_t rows, int d, float eps,
                                void *stream);
/* o_bf16[B*T, d] = softmax(QK^T/8 (+causal)) V per head, from packed qkv_bf16[B*T, 3d] */
int mmr_debug_attention(const void *qkv, void *o, int B, int T, int heads, int causal, void *stream);
/* the non-causal form with a key-padding mask key_mask[B,T] int32 (0 = masked key) */
int mmr_debug_attention_masked(const void *qkv, void *o, int B, int T, int heads, const int32_t *key_mask, void *stream);
/* the pooled-row form: o_bf16[B, d] = the attention row of query picks[b] of each sequence; q_bf16[B, d] is compact, row b
 * the Q part of qkv row b*T + picks[b] (0 <= picks[b] < T, on the device); K and V are read from qkv */
int mmr_debug_attention_pooled(const void *q, const void *qkv, const int32_t *picks, void *o, int B, int T, int heads,
                               int causal, void *stream);
/* Test hook: lowers the workgroup cap of every clamped 1-D launch to `cap` (cap >= 1), or restores the built-in caps
 * (cap == 0).  Returns the number of launches since the previous call whose grid the override made smaller than the
 * built-in rule would have; a negative cap is MMR_EINVAL and changes nothing.  Process-wide; never set outside tests. */
int64_t mmr_debug_grid_cap(int64_t cap);

#ifdef __cplusplus
}
#endif
#endif /* MMR_H */
