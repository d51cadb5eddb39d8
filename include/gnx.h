/* gnx.h -- C ABI of libgnx.so: gnntf's sparse propagation hot path on MI355X (gfx950).
 *
 * The reference (gnntf 0.0.20, paths relative to /root/reference) has NO FFI of its own:
 * the path is Python calling TensorFlow eager ops.  Each entry point below therefore
 * replaces a TensorFlow call site (or a short run of them) in the reference's Python, and
 * is what a ctypes binding inside gnntf would bind (INTEGRATION.md shows that binding).
 *
 * Conventions
 *   - every pointer named d_* is a DEVICE pointer (HBM of the current HIP device); the
 *     library borrows it for the duration of the call and never frees it;
 *   - `stream` is a hipStream_t passed as void* (NULL = the default stream); all work is
 *     enqueued on it and the call returns without waiting, except the graph constructors,
 *     which synchronise that stream (they read sizes back to size their allocations);
 *   - return value: 0 = ok, < 0 = error code below; gnx_last_error() then holds a
 *     thread-local message.  Nothing throws across this boundary;
 *   - a gnx_graph_t owns its device-side index arrays (hipMalloc) until gnx_graph_destroy.
 *     ONE STREAM PER HANDLE AT A TIME: a handle keeps per-handle scratch (the long-row partial slab, which is
 *     re-allocated when a wider C arrives, the transposed-value and degree scratch), so two streams or threads
 *     launching on the same handle concurrently race on it.  Different handles are independent;
 *   - features are row-major float32, leading dimension (`ld*`, in elements) given per call.
 */
#ifndef GNX_H
#define GNX_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct gnx_graph *gnx_graph_t;
typedef struct gnx_halo_plan *gnx_halo_plan_t;

enum { GNX_OK = 0, GNX_ERR_INVALID = -1, GNX_ERR_HIP = -2, GNX_ERR_ALLOC = -3, GNX_ERR_UNSUPPORTED = -4 };

/* `normalized` argument of GNN.get_adjacency (gnntf/core/gnn/gnn.py:36,40-47) */
enum { GNX_NORM_NONE = 0, GNX_NORM_SYMMETRIC = 1, GNX_NORM_BIPARTITE = 2 };
/* `add_eye` argument of GNN.get_adjacency (gnn.py:36,38-39,48-49) */
enum { GNX_EYE_NONE = 0, GNX_EYE_BEFORE = 1, GNX_EYE_AFTER = 2 };
/* epilogue activation: identity (filter.py:8 default) or relu (gcn.py:78 default) */
enum { GNX_ACT_NONE = 0, GNX_ACT_RELU = 1 };
/* tf.nn.leaky_relu at its default slope, v > 0 ? v : 0.2f * v (gcn.py:119): accepted by gnx_ngcf_step and gnx_ngcf_back_gate ONLY;
 * every other entry refuses it as an invalid activation */
enum { GNX_ACT_LEAKY = 2 };
/* flag OR'ed into `act` of gnx_spmm / gnx_spmm_rows: rows without stored entries are NOT written (their output would be
 * alpha * H0[row], which is what an earlier iteration of a propagation loop already left there) -- and cost nothing: the kernels
 * that walk the rows in degree-binned order do not launch their slots at all, the one-wave-per-row kernels walk the ascending
 * list of the rows that have entries.  Ignored when a diagonal weight is given. */
enum { GNX_ACT_SKIP_EMPTY = 256 };

/* Thread-local message of the last failing call on this thread ("" if none). */
const char *gnx_last_error(void);
/* ABI version: major*10000 + minor*100 + patch.  GNX_ABI_VERSION is what THIS header describes; a client compares it with
 * gnx_version() of the library it loaded and refuses a mismatch in major or minor: entry points changed argument lists under
 * the same names between 0.2 and 0.3 (gnx_halo_plan_create / _layout / _pack / _exchange gained `part` and split pull / push
 * counts; gnx_gcnii_step's d_work became d_mixed), so a 0.2 client linked against a 0.3+ library passes shifted arguments.
 * 0.4 adds gnx_graph_reserve and changes no existing signature; 0.5 adds gnx_graph_set_row_window, 0.6 gnx_appnp_propagate_act,
 * likewise; 0.6.1 adds the bf16 storage entries (gnx_cast_bf16, gnx_spmm_bf16, gnx_appnp_propagate_bf16) and changes nothing else;
 * 0.7 adds gnx_graph_enable_entry_dropout (the fused training entries accept handles with duplicate entries once it was called);
 * 0.8 adds the bf16 storage entries of the fused training loops (gnx_spmm_dropped_chained_bf16, gnx_spmm_dropped_back_bf16) and
 * changes nothing else; 0.9 adds the bf16 storage entries of the vertex-partitioned path (gnx_spmm_rows_bf16, gnx_halo_pack_bf16,
 * gnx_halo_exchange_bf16), likewise.  gnx_gcnii_step_bf16 was added WITHIN 0.9 (no existing signature changed, the number stays
 * 900): a client that wants it probes the library for the symbol (dlsym) instead of comparing versions.  So were the gather-order
 * entries (gnx_graph_gather_order, gnx_spmm_dropped_chained_ord, gnx_spmm_dropped_back_ord, GNX_RESERVE_TRAIN_GATHER), likewise, and
 * gnx_gcnii_step_back (the fused backward of the GCNII layer), likewise, and the feature dropout of the GCNII training layer
 * (gnx_gcnii_step_drop, gnx_feature_dropout, gnx_feature_dropout_back), likewise, and the bf16 row storage of GCNII training
 * (gnx_gcnii_step_train_bf16, gnx_feature_dropout_back_bf16, gnx_gcnii_step_back_bf16), likewise, and the GCNII weight gradient
 * without stored mixed rows (gnx_gcnii_wgrad, gnx_gcnii_wgrad_bf16, gnx_gcnii_step_drop_bf16, gnx_graph_hub_rows), likewise, and the
 * spectral-preserving GCNII layer in one launch (gnx_gcnii_step_spectral, gnx_gcnii_spectral_back), likewise, and the gather hints of
 * the wide eval launches (gnx_graph_set_gather_hints, gnx_graph_gather_hints, GNX_RESERVE_GATHER_HINTS), likewise, and the GCN layer
 * in one launch (gnx_gcn_step, gnx_gcn_step_dropped) with its input gradient (gnx_gcn_step_back, gnx_gcn_step_back_dropped), likewise,
 * and the NGCF layer in one launch with its backward's gate (gnx_ngcf_step, gnx_ngcf_back_gate, GNX_ACT_LEAKY) and the rest of its backward in
 * one launch (gnx_step_back_ngcf) and the layer at width 128 as the SpMM and one row-local launch (gnx_step_wide_ngcf) with its
 * backward as the gate, one row-local launch and the transposed SpMM (gnx_step_back_wide_ngcf), likewise, and the link
 * task on the device (gnx_sample_negatives, gnx_edge_plan_bytes, gnx_edge_plan, gnx_edge_sorted_work_floats,
 * gnx_edge_scores_backward_sorted), likewise, and the ranking evaluation of the link task (gnx_rank_candidates_bytes,
 * gnx_rank_candidates, GNX_RANK_MAX_K, GNX_RANK_POS_PASS, GNX_RANK_MAX_SPLITS), likewise, and the spectral-preserving GCN layer in
 * one launch (gnx_step_spectral_gcn, gnx_step_spectral_gcn_dropped), likewise, and the node signals at width 1 (gnx_signal_project,
 * gnx_signal_spmv, gnx_signal_ppr, gnx_signal_smoothness, gnx_signal_smoothness_back, gnx_signal_uniform), likewise. */
#define GNX_ABI_VERSION 900
int gnx_version(void);

/* ---- graph construction ------------------------------------------------------------
 * Replaces tf.sparse.SparseTensor(indices, values, shape) built by graph2adj
 * (gnntf/core/gnn/graph_manipulation.py:24-31): d_indices is int64 [nnz, 2] row-major
 * (row, col) pairs -- UNSORTED, duplicates allowed -- d_values float32 [nnz].
 * The handle keeps every entry (sorted by (row, col), input order kept among duplicates,
 * so per-entry edge dropout follows layered.py:47-50) plus the coalesced CSR in which
 * duplicates are summed (what tf.sparse.sparse_dense_matmul / reduce_sum compute).
 * Fails with GNX_ERR_INVALID on an index outside the shape. */
int gnx_graph_create_coo(int64_t n_rows, int64_t n_cols, int64_t nnz, const int64_t *d_indices,
                         const float *d_values, void *stream, gnx_graph_t *out);

/* Same from a ready CSR (rows ascending, columns ascending and unique inside a row):
 * d_rowptr int64 [n_rows+1], d_colidx int32 [nnz], d_values float32 [nnz].  Used for the
 * column-remapped shard of a vertex-partitioned graph. */
int gnx_graph_create_csr(int64_t n_rows, int64_t n_cols, int64_t nnz, const int64_t *d_rowptr,
                         const int32_t *d_colidx, const float *d_values, void *stream, gnx_graph_t *out);

int gnx_graph_destroy(gnx_graph_t g);

/* Sizes: stored COO entries and coalesced (unique (row, col)) entries. */
int gnx_graph_info(gnx_graph_t g, int64_t *n_rows, int64_t *n_cols, int64_t *nnz_entries,
                   int64_t *nnz_coalesced);
/* The hub rows of the matrix (added within ABI 0.9 -- probe for the symbol): how many rows are longer than the handle's long-row
 * threshold -- the rows the fused launches leave to the long-row kernels, and for which gnx_gcnii_wgrad needs d_hub_rows -- and the
 * threshold itself (entries; 512, or 128 between 2^15 and 2^20 rows).  Either pointer may be NULL.  A row window
 * (gnx_graph_set_row_window) re-plans the handle under the same threshold: the count does not change. */
int gnx_graph_hub_rows(gnx_graph_t g, int64_t *n_hub_rows, int64_t *threshold);

/* Borrowed device pointers to the coalesced CSR (valid until destroy):
 * rowptr int64 [n_rows+1], colidx int32 [nnz_coalesced], raw summed values float32. */
int gnx_graph_csr(gnx_graph_t g, const int64_t **d_rowptr, const int32_t **d_colidx,
                  const float **d_raw_values);
/* Copies of the coalesced CSR into caller-owned device buffers (any may be NULL = skip):
 * rowptr int64 [n_rows+1], colidx int32 [nnz_coalesced], raw values float32 [nnz_coalesced],
 * rowidx int32 [nnz_coalesced] (the row of every coalesced entry).  Stream-ordered. */
int gnx_graph_export(gnx_graph_t g, int64_t *d_rowptr_out, int32_t *d_colidx_out, float *d_raw_values_out,
                     int32_t *d_rowidx_out, void *stream);

/* ---- normalisation: GNN.get_adjacency (gnn.py:36-50) --------------------------------
 * One call = sparse_dropout (layered.py:47-50; only when dropout_p > 0 -- the caller passes
 * 0 in eval mode) -> add_eye "before" -> symmetric / bipartite scaling by COLUMN sums with
 * divide_no_nan -> add_eye "after".  Writes the values of A_hat in coalesced-CSR order to
 * d_vals_out [nnz_coalesced].  The identity added by add_eye is returned as a per-row
 * diagonal weight in d_diag_out [n_rows] (pass it to gnx_spmm); d_diag_out may be NULL when
 * add_eye == GNX_EYE_NONE.  Dropout draws come from the counter RNG keyed by (seed,
 * stream_id, row, col, duplicate rank), so they do not depend on how the graph is sharded.
 * Requires a square graph for symmetric/bipartite. */
int gnx_graph_normalize(gnx_graph_t g, int normalized, int add_eye, float dropout_p, uint64_t seed,
                        uint64_t stream_id, float *d_vals_out, float *d_diag_out, void *stream);

/* gnx_graph_reserve: builds, NOW, what the compute entries otherwise build on first use, sized for feature rows of up to C floats:
 * the slab the long rows' partial sums go through (every entry), with GNX_RESERVE_TRANSPOSED the transposed structure (gnx_spmm_t,
 * gnx_spmm_dropped(transposed), the column sums of a training step), with GNX_RESERVE_K_LOOP the relabelled copy
 * gnx_appnp_propagate runs narrow widths on, with
 * GNX_RESERVE_TRAIN_GATHER what gnx_spmm_dropped_chained_ord / gnx_spmm_dropped_back_ord walk (the gather order and the gather
 * columns of the matrix and of the transposed structure; implies GNX_RESERVE_TRANSPOSED; GNX_ERR_UNSUPPORTED on a vertex block, a
 * handle with duplicate entries or a handle with a row window), with GNX_RESERVE_GATHER_HINTS the hinted columns an eval launch of
 * width C would otherwise build on first use (gnx_graph_set_gather_hints; nothing where the handle or the width takes none).  Those lazy builds allocate and synchronise, which a stream that is
 * being captured into a hipGraph must not see: a compute entry that would have to grow something under capture fails with
 * GNX_ERR_UNSUPPORTED and a message naming this call.  Reserve (or run the launch once eagerly) BEFORE capturing; replays then
 * touch no allocator.  ("an optional caller-provided workspace" -- the workspace stays owned by the handle, the
 * caller decides when it is sized.)  Nothing in the reference corresponds: TensorFlow eager allocates per op. */
enum { GNX_RESERVE_TRANSPOSED = 1, GNX_RESERVE_K_LOOP = 2, GNX_RESERVE_TRAIN_GATHER = 4, GNX_RESERVE_GATHER_HINTS = 8 };
int gnx_graph_reserve(gnx_graph_t g, int64_t C, int flags, void *stream);

/* Gather hints (added within ABI 0.9 -- probe for the symbols).  On a power-law graph a few rows of the gathered matrix receive a
 * large share of all gathers; they are worth more in the caches than the many rows a launch gathers once or twice.  With hints
 * the handle keeps, per entry of the matrix, its column with bit 31 set when the column is COLD -- not one of the `hot_rows` rows
 * with the most stored entries, ties to the smaller id -- and the wide float32 eval launches (gnx_spmm and the loops built on it:
 * feature rows of at least 256 bytes, 4 values per lane) gather a cold row with a non-temporal load, which the L2 replaces first.
 * Same entries, same order, same fused multiply-adds: results are bitwise those without hints; gnx_graph_last_kernel reports the
 * same name either way (gnx_graph_gather_hints says whether the last launch took hints).  Costs 4 bytes per entry plus 4 per row; built on first use or by
 * gnx_graph_reserve(GNX_RESERVE_GATHER_HINTS) (under capture without it: GNX_ERR_UNSUPPORTED naming that call).  If the arrays
 * cannot be allocated the handle runs unhinted, the calls succeed and gnx_last_error says so.  Square stand-alone handles without a
 * row window only: a vertex block, a non-square handle and a handle with a row window take no hints, whatever is set.
 * gnx_graph_set_gather_hints: hot_rows = -1 automatic, the default (on structures of at least 2^25 rows: the rows that fill 256 MiB,
 * the Infinity Cache, at the width of the call; measured on R-MAT graphs: -5 % per propagation at 80M rows and C = 128 or 64, -1 to
 * -6 % at 40M, a loss of 2-7 % at 20M rows and below, which is why smaller structures take hints only when asked), 0 off (frees the arrays; synchronises the device), n > 0 that many hot rows (built now).  Not
 * capturable.  gnx_graph_gather_hints: the borrowed device array [nnz_coalesced] (NULL: none built, or the handle takes none) and
 * the hot_rows it was built for, and the hot_rows the LAST SpMM launch over the handle gathered with (0: it took no hints -- a narrow
 * width, a training or bf16 launch, hints off); any pointer may be NULL.  The training, GCNII and bf16 entries keep the plain columns.
 * Nothing in the reference corresponds. */
int gnx_graph_set_gather_hints(gnx_graph_t g, int64_t hot_rows, void *stream);
int gnx_graph_gather_hints(gnx_graph_t g, const int32_t **d_hint_cols, int64_t *hot_rows, int64_t *last_launch_hot_rows);

/* Pendant elision of the K loop (added within ABI 0.9 -- probe for the symbols).  A PENDANT row i stores exactly one entry (i, h).  It
 * is ELIDABLE when h != i, h stores at least two entries and no row but h stores an entry in column i: the iterates of i between
 * H0 and the result are then read by h alone.  gnx_appnp_propagate / _act (the wide float32 branch, K >= 2, no diagonal) then
 * launches such rows in the LAST iteration only; in the others h gathers H0[i] where it gathered the iterate -- the same bytes -- and
 * forms the iterate itself, from the value of entry (i, h) and its own row of two iterations ago, with the very operations the row's
 * own launch ran: results are bitwise those without elision, and the work buffer never holds an elidable row.  Rides on the
 * gather hints: active only where the loop's launches take them (gnx_graph_set_gather_hints), on handles of fewer than 2^30
 * columns.  Costs 4 bytes per entry and 7 per row; built on first use, by mode 1 or by gnx_graph_reserve(GNX_RESERVE_GATHER_HINTS)
 * (under capture without it: GNX_ERR_UNSUPPORTED naming that call); the build moves the elidable rows to the end of the one-entry
 * rows of the handle's launch order and synchronises the device.  If the arrays cannot be allocated the handle runs without it.
 * gnx_graph_set_pendant_elision: mode = -1 automatic, the default (exactly where the AUTOMATIC gather hints are on), 0 off, 1 on
 * wherever admissible (built now).  Not capturable.  gnx_graph_pendant_elision: the number of elidable rows, the borrowed device
 * array [n_rows] of bytes (1 = elidable; NULL and 0: no plan built) and whether the last gnx_appnp_propagate(_act) over the handle
 * elided; any pointer may be NULL.  Every other entry is untouched.  Nothing in the reference corresponds. */
int gnx_graph_set_pendant_elision(gnx_graph_t g, int mode, void *stream);
int gnx_graph_pendant_elision(gnx_graph_t g, int64_t *n_elidable, const uint8_t **d_elidable, int *last_loop_elided);

/* gnx_graph_enable_entry_dropout: builds, NOW, what the fused training entries (gnx_spmm_dropped, gnx_spmm_dropped_chained,
 * gnx_spmm_dropped_back) and the one-pass column sums of gnx_graph_colsum_streams need on a handle whose COO held duplicate entries
 * -- what graph2adj makes of a graph that stores both directions already (graph_manipulation.py:28-30): every (row, col) twice.
 * Per coalesced slot a multiplicity byte and the value its entries share, in CSR and in transposed order (5 bytes per slot each,
 * plus the transposed structure); slots whose entries differ walk the entry list.  The draws and sums stay those of
 * gnx_graph_normalize: keep bit = hash(seed, stream, row, col, duplicate rank), slot value = its kept entries * 1/(1-p) added in
 * input order.  Allocates and synchronises: call before capturing.  Until it has been called those entries return
 * GNX_ERR_UNSUPPORTED on such a handle; on a handle without duplicates it does nothing.  Nothing in the reference corresponds. */
int gnx_graph_enable_entry_dropout(gnx_graph_t g, void *stream);

/* gnx_graph_set_row_window: the caller declares that ITS numbering of the vertices carries locality -- neighbours in the graph
 * are neighbours in the numbering (a community / breadth-first order of the dataset; gnntf's GNN(reorder="locality") computes one).
 * The propagation launches then take the rows in WINDOWS of `window_rows` consecutive ids -- inside a window still in the
 * degree-binned order that gives the rows sharing a wave equal lengths -- so that the rows in flight together gather from one
 * neighbourhood of H (at narrow widths a gather moves a whole 128-byte line for a 16..160-byte row: what counts is how often the
 * line is still in a cache), and gnx_appnp_propagate does NOT run narrow widths on its degree-relabelled copy, which would scatter
 * that neighbourhood.  0 restores the default (global degree bins).  Results are the same sums in the same per-row order: bitwise
 * those of the default order except where the default would have used the relabelled copy.  Rebuilds the handle's launch plan:
 * synchronises the DEVICE (work on any stream may still read the old plan's arrays, which are freed), not capturable, and
 * INVALIDATES every hipGraph captured on this handle before the call (a replay would read the freed arrays): capture again.
 * Nothing in the reference corresponds (TensorFlow's kernel walks the COO as stored). */
int gnx_graph_set_row_window(gnx_graph_t g, int64_t window_rows, void *stream);

/* gnx_graph_set_dropout_counter: from now on every dropout stream id used with this handle is `stream_id + *d_counter`
 * (d_counter: one uint64 in device memory, read by the kernels when they run; NULL switches it off).  This is what lets a
 * whole training step be captured ONCE in a hipGraph and replayed every epoch with fresh masks: the ids baked into the
 * captured launches stay fixed, the step's last node advances the counter (layered.py:47-50 draws new masks per call). */
int gnx_graph_set_dropout_counter(gnx_graph_t g, const uint64_t *d_counter);

/* gnx_graph_set_block: declares the handle to be ONE VERTEX BLOCK of a larger square graph (multi-GPU training with edge
 * dropout): its row r is global vertex row0_global + r, its column c is global vertex d_col_gid[c]
 * (int32 [n_cols], copied), and local row r is column row0_buf + r of the block's own column space (the [regions | local rows |
 * regions] buffer of gnx_halo_plan_layout).  From then on the dropout draws of gnx_graph_colsum(_streams) /
 * gnx_graph_scale_values / gnx_spmm_dropped are keyed by the GLOBAL (row, col) -- the masks equal the one-GPU masks whatever
 * the partition -- and gnx_spmm_dropped accepts the rectangular block: d_D is then [n_cols] (scales of every buffer column),
 * row r's own scale being d_D[row0_buf + r].  gnx_graph_colsum gives the block's PARTIAL column sums; the caller adds the
 * blocks up (halo columns go back to their owners) before gnx_degree_scale.  d_col_gid == NULL undoes the declaration. */
int gnx_graph_set_block(gnx_graph_t g, int64_t row0_global, int64_t row0_buf, const int32_t *d_col_gid, void *stream);

/* gnx_graph_normalize_t: the same normalisation, but the values are written in the order of the TRANSPOSED
 * structure (the order gnx_spmm_tv consumes).  The backward pass of a training step only needs A_hat^T, so it
 * regenerates the iteration's dropped adjacency straight into this order instead of permuting a CSR-order
 * array (what tf.GradientTape keeps alive, trainable.py:70-78, is recomputed here from the counter RNG). */
int gnx_graph_normalize_t(gnx_graph_t g, int normalized, int add_eye, float dropout_p, uint64_t seed,
                          uint64_t stream_id, float *d_vals_t_out, float *d_diag_out, void *stream);

/* The three steps separately, for vertex-partitioned graphs where column sums need a
 * cross-rank all-reduce in between:
 *   colsum: d_colsum_out[j] = sum_i v_ij over this handle's rows (tf.sparse.reduce_sum
 *           axis=0, gnn.py:41,44), v = dropped raw values; fixed summation order.
 *   degree_scale: in place d[j] <- divide_no_nan(1, sqrt(d[j] + eye)) (symmetric) or
 *           divide_no_nan(1, d[j] + eye) (bipartite); eye = 1 for add_eye "before".
 *   scale_values: d_vals_out[k] = row_scale[row_k] * v_k * col_scale[col_k]; either scale
 *           may be NULL (= 1).  (gnn.py:42,45) */
int gnx_graph_colsum(gnx_graph_t g, float dropout_p, uint64_t seed, uint64_t stream_id,
                     float *d_colsum_out, void *stream);
/* gnx_graph_colsum for n_streams consecutive dropout streams (first_stream, first_stream + 1, ...) in one pass over the
 * structure: the K iterations of a training step drop their edges independently but share everything else.
 * d_colsum_out is [n_streams, n_cols]; every row is bit for bit what gnx_graph_colsum gives for that stream. */
int gnx_graph_colsum_streams(gnx_graph_t g, float dropout_p, uint64_t seed, uint64_t first_stream, int n_streams,
                             float *d_colsum_out, void *stream);
int gnx_degree_scale(float *d_deg, int64_t n, int normalized, int add_eye_before, void *stream);
int gnx_graph_scale_values(gnx_graph_t g, float dropout_p, uint64_t seed, uint64_t stream_id,
                           const float *d_row_scale, const float *d_col_scale, float *d_vals_out,
                           void *stream);

/* ---- the hot path ---------------------------------------------------------------------
 * gnx_spmm: out[i,:] = act( beta * ( sum_j A[i,j] X[j,:] + diag[i] X[i,:] ) + alpha * H0[i,:] )
 *   - replaces tf.sparse.sparse_dense_matmul (filter.py:19, gcn.py:88) and, with
 *     beta = 1-a, alpha = a, the residual mix fused behind it (filter.py:20-21) and the
 *     optional activation (filter.py:22);
 *   - d_vals: values in coalesced-CSR order (from gnx_graph_normalize), NULL = raw values;
 *   - d_diag: per-row diagonal weight or NULL; d_H0 may be NULL (then alpha is ignored); ldh0 == 0 broadcasts
 *     ONE row of C values to every output row (a bias: gcn.py:89);
 *   - X is [n_cols, C], out and H0 are [n_rows, C]; out must not alias X.
 * gnx_spmm_t: the same with the transposed matrix (out is [n_cols, C], X and H0 index by
 *   the other side) -- the backward of gnx_spmm (what tf.GradientTape derives,
 *   trainable.py:70-78).  d_vals are still given in coalesced-CSR order of A. */
int gnx_spmm(gnx_graph_t g, const float *d_vals, const float *d_diag, const float *d_X, int64_t ldx,
             int64_t C, const float *d_H0, int64_t ldh0, float beta, float alpha, int act,
             float *d_out, int64_t ldo, void *stream);
int gnx_spmm_t(gnx_graph_t g, const float *d_vals, const float *d_diag, const float *d_X, int64_t ldx,
               int64_t C, const float *d_H0, int64_t ldh0, float beta, float alpha, int act,
               float *d_out, int64_t ldo, void *stream);

/* gnx_spmm_tv: gnx_spmm_t with the values ALREADY in transposed order (from gnx_graph_normalize_t or
 * gnx_graph_permute_values_t); skips the per-call permutation. */
int gnx_spmm_tv(gnx_graph_t g, const float *d_vals_t, const float *d_diag, const float *d_X, int64_t ldx,
                int64_t C, const float *d_H0, int64_t ldh0, float beta, float alpha, int act,
                float *d_out, int64_t ldo, void *stream);
/* d_vals_t_out[p] = d_vals[perm[p]]: CSR-order values -> transposed order (for a constant adjacency). */
int gnx_graph_permute_values_t(gnx_graph_t g, const float *d_vals, float *d_vals_t_out, void *stream);

/* gnx_spmm_scatter: gnx_spmm whose result row i is written to out[d_out_rows[i], :] (int32 [n_rows], a
 * permutation).  Lets the LAST iteration of a propagation over a relabelled graph put the rows straight back
 * into the caller's order instead of paying a separate un-permute pass. */
int gnx_spmm_scatter(gnx_graph_t g, const float *d_vals, const float *d_diag, const float *d_X, int64_t ldx,
                     int64_t C, const float *d_H0, int64_t ldh0, float beta, float alpha, int act,
                     const int32_t *d_out_rows, float *d_out, int64_t ldo, void *stream);

/* gnx_spmm_dropped: gnx_spmm (transposed == 0) or gnx_spmm_tv (transposed != 0) over the dropped + symmetrically
 * re-normalised adjacency of ONE training iteration WITHOUT materialising its values: every entry's weight
 * (D[row] * dropout(raw)) * D[col] is produced inside the kernel from the counter RNG -- the same arithmetic, bit for bit, as
 * gnx_graph_normalize(g, GNX_NORM_SYMMETRIC, GNX_EYE_NONE, dropout_p, seed, stream_id, ...) followed by gnx_spmm.
 * d_D [n]: the degree scales of that iteration = gnx_graph_colsum(g, dropout_p, seed, stream_id, d_D) then
 * gnx_degree_scale(d_D, n, GNX_NORM_SYMMETRIC, 0).  Saves the nnz-sized value array and the pass that writes it
 * (layered.py:47-50 + gnn.py:41-42 happen in the SpMM's value fetch).  PRECONDITION: finite d_X and d_D -- a dropped entry is
 * skipped (its row of d_X is not read), while the two-call form multiplies it by an explicit zero, so a non-finite row behind a
 * dropped entry, or a NaN scale, turns the two-call result into NaN and not this one.  Square graphs or vertex blocks (gnx_graph_set_block).
 * When the COO held duplicate entries (per-entry dropout: a slot's weight is made from its kept entries) the handle needs
 * gnx_graph_enable_entry_dropout first; without it GNX_ERR_UNSUPPORTED (use gnx_graph_normalize), as for the two entries below. */
int gnx_spmm_dropped(gnx_graph_t g, const float *d_D, float dropout_p, uint64_t seed, uint64_t stream_id, int transposed,
                     const float *d_X, int64_t ldx, int64_t C, const float *d_H0, int64_t ldh0, float beta, float alpha,
                     int act, float *d_out, int64_t ldo, void *stream);

/* gnx_spmm_dropped_chained: the forward gnx_spmm_dropped for a LOOP of training iterations.  The weight of an entry needs its
 * column's degree scale, a random 4-byte gather per entry (0.7 of the 3.8 ms of a launch at C = 64); in a loop the previous
 * iteration can deliver it with the row instead: with d_D_next != NULL every finished row is multiplied by d_D_next[row]
 * (= the NEXT iteration's scale of that vertex as a column) on its way out, and with x_prescaled != 0 the kernel takes the rows
 * of d_X as carrying their column scale already.  Iteration 0 runs with x_prescaled = 0, the last one with d_D_next = NULL; the
 * H0 mix term is the plain one throughout.  Same masks and the same value as K gnx_spmm_dropped calls up to float32 rounding
 * (the scale is applied to the gathered row instead of the weight). */
int gnx_spmm_dropped_chained(gnx_graph_t g, const float *d_D, float dropout_p, uint64_t seed, uint64_t stream_id, int x_prescaled,
                             const float *d_D_next, const float *d_X, int64_t ldx, int64_t C, const float *d_H0, int64_t ldh0,
                             float beta, float alpha, int act, float *d_out, int64_t ldo, void *stream);

/* One BACKWARD training iteration inside a loop -- what tf.GradientTape derives for K PPRIteration layers (trainable.py:70-78 over
 * filter.py:19-21): g_k = (1-a) A_k^T g_{k+1}, dH0 = g_0 + a (g_1 + ... + g_K).  Walks the TRANSPOSED structure with the weights
 * of dropout stream `stream_id` made inside the kernel, acc[r] = sum_c A_k[c][r] X[c], and writes TWO results:
 *     S_out[r] = s_beta * acc[r] + s_alpha * S_in[r]          the running sum dH0 is built in (S_in may be S_out: in place)
 *     Y_out[r] = y_beta * acc[r] * D_next[r]                  g_k carrying the column scale of the NEXT step (stream_id - 1), or
 *                                                             plain when d_D_next is NULL; skipped when d_Y_out is NULL
 * With x_prescaled the rows of X carry their own scale D[c] already (the previous call's Y_out), so no per-entry gather of a
 * column scale is left -- in the un-chained form (gnx_spmm_dropped, transposed) that gather fetches a 128-byte line per kept
 * entry (profiles/NOTES.md round 4: +4.5 GB per launch at config 4, C = 64).  The loop: X = upstream gradient, S_in = X,
 * s_alpha = a for the first call; afterwards X = the previous Y_out, S_in = S_out, s_alpha = 1; s_beta = a (1-a), y_beta = 1-a;
 * the last call (stream 0) adds g_0 whole: s_beta = 1-a, no Y_out.  Square stand-alone graphs (with duplicate entries: after
 * gnx_graph_enable_entry_dropout).
 * act: GNX_ACT_NONE, or GNX_ACT_SKIP_EMPTY (with S_in == S_out) for every call but the first of a loop: rows without entries
 * contribute g_k = 0, so their sum stays what the first call made it and their Y row is never gathered -- they are left untouched
 * (honoured only on graphs where no entry references a row without entries; gnx_spmm_dropped_chained takes the same flag for
 * every iteration but the last of a forward loop).
 * Finite operands only (a dropped entry's row is not gathered), as for gnx_spmm_dropped. */
int gnx_spmm_dropped_back(gnx_graph_t g, const float *d_D, float dropout_p, uint64_t seed, uint64_t stream_id, int x_prescaled,
                          const float *d_D_next, const float *d_X, int64_t ldx, int64_t C, const float *d_S_in, int64_t lds_in,
                          float s_alpha, float s_beta, float *d_S_out, int64_t lds_out, float y_beta, float *d_Y_out, int64_t ldy,
                          int act, void *stream);

/* ---- the training loops over the handle's gather order ---------------------------------------------------------------------
 * At narrow widths a gather moves a whole 128-byte line for a 28..256-byte row, so what a training launch costs is how often that
 * line is found in a cache; in the caller's numbering the rows that receive most gathers (the hubs) are scattered.  The GATHER
 * ORDER of a square handle is the order gnx_appnp_propagate numbers its relabelled copy in: degree bins, heaviest first, and inside
 * a bin the vertices by the degree rank of their most popular neighbour -- hub rows share lines, a hub's leaves sit in consecutive
 * lines.  The two entries below keep rows, per-row entry order, masks, weights, scales and sums the caller's; only the matrix that
 * is GATHERED (and the one the next launch of the loop gathers) is stored in gather order, reached through a second column array
 * of 4 bytes per entry (built on first use or by gnx_graph_reserve(GNX_RESERVE_TRAIN_GATHER); under capture without it:
 * GNX_ERR_UNSUPPORTED naming gnx_graph_reserve).  Per row the same fused multiply-adds on the same values in the same order: the
 * results are BITWISE those of gnx_spmm_dropped_chained / gnx_spmm_dropped_back, whatever `order` says.
 * gnx_graph_gather_order: borrowed device pointers (valid until destroy or gnx_graph_set_row_window), either may be NULL:
 *   d_order int32 [n]: position in the gather order -> vertex; d_rank int32 [n]: vertex -> position.  "X stored in gather order"
 *   means row i of the buffer holds vertex d_order[i].  Builds the order on first use (allocates and synchronises the default
 *   stream: not under capture).  Square graphs; GNX_ERR_UNSUPPORTED on a handle with a row window.
 * `order` = an OR of
 *   GNX_ORD_X    the rows of d_X are stored in gather order;
 *   GNX_ORD_OUT  d_out (gnx_spmm_dropped_chained_ord) or d_Y_out (gnx_spmm_dropped_back_ord) is written in gather order.
 * Everything else -- d_H0, d_D, d_D_next, d_S_in / d_S_out -- is indexed by the caller's vertex ids; every other argument is the
 * namesake's.  order == 0 IS the namesake.  A K-iteration forward loop: iteration 0 passes GNX_ORD_OUT with X = H0 as the caller
 * holds it, the middle iterations both flags, the last one GNX_ORD_X, so H_K lands in the caller's order and no permute pass exists
 * at either end.  The backward loop mirrors it: the first call gathers the upstream gradient in the caller's order and writes its
 * Y_out in gather order, the last call has no Y_out.  GNX_ACT_SKIP_EMPTY keeps its rules.  Square stand-alone handles without
 * duplicate entries only: a vertex block (gnx_graph_set_block), a handle with duplicate entries and a handle with a row window
 * (its numbering carries locality already) get GNX_ERR_UNSUPPORTED and a message saying which.  gnx_graph_last_kernel reports the
 * training names with "_ord" appended and the hub launches named ("spmm_group8_drop_ord", "spmm_group16+long_drop_ord").
 * Nothing in the reference corresponds. */
enum { GNX_ORD_X = 1, GNX_ORD_OUT = 2 };
int gnx_graph_gather_order(gnx_graph_t g, const int32_t **d_order, const int32_t **d_rank);
int gnx_spmm_dropped_chained_ord(gnx_graph_t g, const float *d_D, float dropout_p, uint64_t seed, uint64_t stream_id, int x_prescaled,
                                 const float *d_D_next, const float *d_X, int64_t ldx, int64_t C, const float *d_H0, int64_t ldh0,
                                 float beta, float alpha, int act, float *d_out, int64_t ldo, int order, void *stream);
int gnx_spmm_dropped_back_ord(gnx_graph_t g, const float *d_D, float dropout_p, uint64_t seed, uint64_t stream_id, int x_prescaled,
                              const float *d_D_next, const float *d_X, int64_t ldx, int64_t C, const float *d_S_in, int64_t lds_in,
                              float s_alpha, float s_beta, float *d_S_out, int64_t lds_out, float y_beta, float *d_Y_out, int64_t ldy,
                              int act, int order, void *stream);

/* gnx_spmm_rows: the fused step for a handle that holds only a SUBSET of the output rows (the interior or the
 * boundary rows of a vertex block, compacted): result row r lands in out[d_rows[r], :] and mixes in
 * H0[d_rows[r], :] (d_rows int32 [n_rows of the handle]; out and H0 are the full-height matrices).  Same
 * arithmetic per row as gnx_spmm (filter.py:19-21); no diagonal term. */
int gnx_spmm_rows(gnx_graph_t g, const float *d_vals, const float *d_X, int64_t ldx, int64_t C, const float *d_H0,
                  int64_t ldh0, float beta, float alpha, int act, const int32_t *d_rows, float *d_out, int64_t ldo,
                  void *stream);

/* One PPRIteration.__forward__ (filter.py:17-22) with a fixed adjacency:
 * out = act( (A_hat . H)*(1-a) + H0*a ).  Thin wrapper over gnx_spmm. */
int gnx_ppr_step(gnx_graph_t g, const float *d_vals, const float *d_diag, const float *d_H,
                 const float *d_H0, float a, int64_t C, int act, float *d_out, void *stream);

/* The K-iteration loop of APPNP in eval mode (filter.py:34-35 with a constant A_hat):
 * H <- H0; repeat K times H <- (A_hat . H)*(1-a) + H0*a.  All matrices [n, C] contiguous
 * (square graph).  d_work is a caller-provided scratch [n, C]; the result lands in d_out.
 * d_out, d_work and d_H0 must be distinct buffers.  Two things the loop does that K separate gnx_ppr_step calls do not:
 *   - rows without stored entries (a * H0 after every iteration) are computed when each buffer is first a destination and left
 *     alone afterwards (GNX_ACT_SKIP_EMPTY) -- same bits, fewer bytes; when no entry references such a row (every symmetric
 *     pattern) they are written into d_out only and d_work never receives them (its rows of that kind stay as the caller left them);
 *   - for C <= 16 on graphs of at least 2^20 vertices (no diagonal) the iterations run on a degree-relabelled copy of the
 *     matrix (heaviest vertices first; inside a degree bin the vertices follow their most popular neighbour's rank) that the
 *     handle builds on first use (+ about 12 bytes per entry and an [n, C] scratch, owned by the handle): H0 is
 *     permuted on the way in, the last iteration scatters back into the caller's row order; a row's columns are then summed in
 *     the relabelled order, so the result equals the step-by-step one up to float32 rounding. */
int gnx_appnp_propagate(gnx_graph_t g, const float *d_vals, const float *d_diag, const float *d_H0,
                        float a, int K, int64_t C, float *d_out, float *d_work, void *stream);

/* The same loop with the reference's per-iteration activation (filter.py:22,28,35: APPNP hands its ``activation`` to every
 * PPRIteration): H <- act((A_hat . H)*(1-a) + H0*a), act = GNX_ACT_NONE (= gnx_appnp_propagate) or GNX_ACT_RELU, applied in every
 * iteration's epilogue -- bit for bit what K gnx_ppr_step calls with that act return (below the relabelling threshold).  A row
 * without entries is act(a * H0) after every iteration, so the settled-row rule above holds unchanged. */
int gnx_appnp_propagate_act(gnx_graph_t g, const float *d_vals, const float *d_diag, const float *d_H0,
                            float a, int K, int64_t C, int act, float *d_out, float *d_work, void *stream);

/* ---- opt-in bf16 feature storage: eval-mode propagation (no backward) -------------------------------------------------
 * bf16 values are passed as uint16_t bit patterns.  bf(x) = x rounded to nearest even, NaN stays NaN; u = 2^-8.
 * gnx_cast_bf16: dst = bf(src), [n_rows, C] with leading dimensions lds / ldd (elements); dst must not alias src.
 * gnx_spmm_bf16: out[i,:] = act( beta * ( sum_j A[i,j] X~[j,:] + diag[i] X~[i,:] ) + alpha * H0[i,:] ) with X~ bf16 (widened
 *   exactly), the sums, H0 and the epilogue in f32; out is f32 (out_bf16 = 0) or bf(.) (out_bf16 = 1).  The argument rules of
 *   gnx_spmm: d_vals NULL = raw values, d_diag optional (square graph), ldh0 == 0 broadcasts one H0 row, act may carry
 *   GNX_ACT_SKIP_EMPTY.  The per-row summation order follows the fixed rules of gnx_spmm (chunk order for long rows): two calls
 *   give the same bits.
 * gnx_appnp_propagate_bf16: the loop of gnx_appnp_propagate_act with the iterate stored as bf16 between iterations:
 *   H~_0 = bf(H0); H_{k+1} = act((1-a) A_hat . H~_k + a H0) with H0 f32 in the mix; H~_{k+1} = bf(H_{k+1}) for k < K-1; d_out
 *   receives f32 H_K for every row.  d_work holds TWO bf16 [n, C] buffers (the bytes of one f32 [n, C] buffer) and is needed for
 *   every K >= 1; K = 0 copies H0.  Rows without entries follow the settled-row rule of gnx_appnp_propagate.  No relabelled copy. */
int gnx_cast_bf16(const float *d_src, int64_t n_rows, int64_t C, int64_t lds, uint16_t *d_dst, int64_t ldd, void *stream);
int gnx_spmm_bf16(gnx_graph_t g, const float *d_vals, const float *d_diag, const uint16_t *d_X, int64_t ldx, int64_t C,
                  const float *d_H0, int64_t ldh0, float beta, float alpha, int act, void *d_out, int out_bf16, int64_t ldo,
                  void *stream);
int gnx_appnp_propagate_bf16(gnx_graph_t g, const float *d_vals, const float *d_diag, const float *d_H0, float a, int K, int64_t C,
                             int act, float *d_out, uint16_t *d_work, void *stream);
/* gnx_spmm_rows_bf16: gnx_spmm_rows with the gathered operand stored as bf16 and the result f32 (out_bf16 = 0) or bf(.) (out_bf16 = 1):
 *   for the interior / boundary handles of a vertex block.  Result row r lands in out[d_rows[r], :] and mixes in H0[d_rows[r], :]
 *   (f32); per row the arithmetic and summation order of gnx_spmm_bf16 over the same handle; act may carry GNX_ACT_SKIP_EMPTY. */
int gnx_spmm_rows_bf16(gnx_graph_t g, const float *d_vals, const uint16_t *d_X, int64_t ldx, int64_t C, const float *d_H0,
                       int64_t ldh0, float beta, float alpha, int act, const int32_t *d_rows, void *d_out, int out_bf16, int64_t ldo,
                       void *stream);

/* ---- opt-in bf16 feature storage: the fused training loops -----------------------------------------------------------------
 * gnx_spmm_dropped_chained and gnx_spmm_dropped_back, argument for argument, with the GATHERED operand d_X stored as bf16 (uint16_t
 * bit patterns, widened exactly to f32 as they arrive).  The masks, the kept sums, the degree scales d_D / d_D_next and every
 * weight are the f32 ones of the namesakes; every sum, H0, the mix, the running sum S and both results of a training step are f32.
 * Rounding points (bf = the cast of gnx_cast_bf16), for K iterations with scale vectors D_0 .. D_{K-1}:
 *   forward:  X_0 = bf(H0) gathered with x_prescaled = 0; H_{k+1} = beta * acc + alpha * H0 in f32; for k < K-1 the row leaves as
 *             X_{k+1}[i] = bf(H_{k+1}[i] * D_{k+1}[i]) (out_bf16 = 1, d_D_next = D_{k+1}): ONE rounding, after the scale; the last
 *             iteration writes f32 H_K (out_bf16 = 0, d_D_next = NULL).
 *   backward: the first call gathers bf(g) unscaled and starts the sum from f32 g (d_S_in = g); every call updates
 *             S = s_beta * acc + s_alpha * S_in in f32 and, unless d_Y_out is NULL, writes Y[r] = bf(y_beta * acc[r] * d_D_next[r]),
 *             the next call's operand.  The sum never sees a rounded addend; only what is propagated further is rounded.
 * With x_prescaled = 0 and d_D_next = NULL the first is a plain dropped SpMM over bf16 rows.  d_out of the first is f32
 * (out_bf16 = 0) or bf16 (out_bf16 = 1), [n, ldo] elements of that type.  Rows without entries follow the GNX_ACT_SKIP_EMPTY rules of
 * the namesakes.  The per-row summation order follows the fixed rules of the f32 training kernels (round order, chunk order for long
 * rows, no float atomics): two calls give the same bits; bit-equality with the f32 entries is not a goal.
 * Square stand-alone graphs only: a vertex block (gnx_graph_set_block) returns GNX_ERR_UNSUPPORTED; a handle with duplicate entries
 * needs gnx_graph_enable_entry_dropout first.  Allocation-free once the handle is reserved (gnx_graph_reserve: the long-row slab,
 * the transposed structure); under capture they return GNX_ERR_UNSUPPORTED naming gnx_graph_reserve where something would grow. */
int gnx_spmm_dropped_chained_bf16(gnx_graph_t g, const float *d_D, float dropout_p, uint64_t seed, uint64_t stream_id,
                                  int x_prescaled, const float *d_D_next, const uint16_t *d_X, int64_t ldx, int64_t C,
                                  const float *d_H0, int64_t ldh0, float beta, float alpha, int act,
                                  void *d_out, int out_bf16, int64_t ldo, void *stream);
int gnx_spmm_dropped_back_bf16(gnx_graph_t g, const float *d_D, float dropout_p, uint64_t seed, uint64_t stream_id,
                               int x_prescaled, const float *d_D_next, const uint16_t *d_X, int64_t ldx, int64_t C,
                               const float *d_S_in, int64_t lds_in, float s_alpha, float s_beta, float *d_S_out, int64_t lds_out,
                               float y_beta, uint16_t *d_Y_out, int64_t ldy, int act, void *stream);

/* One GCNIILayer.__forward__ (gnntf/core/gnn/architectures/gcn.py:22-27) with a fixed adjacency:
 *   out = act( ((A_hat . H)*(1-a) + H0*a) . M ),   M = (1-b) I + b W  given by the caller as a [C, C] matrix (ldm).
 * For C in {16, 32, 64} (16-byte aligned buffers) this is ONE launch for all rows of at most 512 entries: the mixed rows
 * T = (A_hat . H)*(1-a) + H0*a stay in LDS and meet M on the matrix cores (v_mfma_f32_16x16x4_f32, exact float32) before the only
 * store; hub rows go through the long-row kernels and the dense kernel.
 * d_mixed [n, C]: NULL in inference (T never reaches HBM).  In training pass a buffer: the same launch also writes T there -- what
 * tf.GradientTape keeps for dM = T^T g (trainable.py:70-78) -- so T is written once and not read back for the transform.
 * Other widths NEED d_mixed: they run gnx_spmm into it and then gnx_dense.  All matrices contiguous [n, C]; square graph. */
int gnx_gcnii_step(gnx_graph_t g, const float *d_vals, const float *d_H, const float *d_H0, float a, int64_t C,
                   const float *d_M, int64_t ldm, int act, float *d_out, float *d_mixed, void *stream);
/* gnx_gcnii_step_bf16 (opt-in bf16 feature storage, inference only; added within ABI 0.9 -- probe for the symbol): the same layer
 * with the GATHERED rows d_H stored as bf16 (uint16_t bit patterns, [n, C] contiguous):
 *   out = act( ((1-a) * A_hat . H~ + a * H0) . M )
 * Rounding points (bf = the cast of gnx_cast_bf16: round to nearest even, NaN stays NaN; u = 2^-8): H~ is widened exactly as it
 * arrives; the sums, H0 (f32), the mix and the transform (v_mfma_f32_16x16x4_f32, exact float32) are f32; out is f32 (out_bf16 = 0)
 * or bf(.) (out_bf16 = 1, uint16_t [n, C]) -- that ONE store is the only rounding the entry adds.  In a stack of layers the first
 * operand is bf(H) (gnx_cast_bf16), every layer but the last hands bf(out) to the next, the last writes f32; H0 stays f32.
 * Per row the entry order, the summation order (chunk order for hub rows) and the transform are those of gnx_gcnii_step: over
 * bf16-representable H, out_bf16 = 0 returns the bits of gnx_gcnii_step over the widened H (same dispatch class: buffers aligned
 * alike), and out_bf16 = 1 the bits of gnx_cast_bf16 of that; two calls give the same bits.  No d_mixed is kept: training uses
 * gnx_gcnii_step.  Square graphs; the argument checks of gnx_gcnii_step.
 * Dispatch: C in {16, 32, 64} with d_H (and a bf16 d_out) 8-byte aligned and the f32 buffers 16-byte aligned: the one fused launch,
 * bf16 rows loaded as 8-byte units of four columns; hub rows (longer than the handle's threshold) go through the bf16 long-row chunk
 * kernels into f32 mixed rows in d_work, the dense kernel transforms those rows alone, and they are rounded on the way out when
 * out_bf16 = 1.  Other widths / alignments: the SpMM + mix over bf16 rows into d_work (f32), the dense kernel, then the rounding
 * pass when out_bf16 = 1 (that form needs C <= 256: GNX_ERR_UNSUPPORTED above -- take out_bf16 = 0 and gnx_cast_bf16 there).
 * d_work: f32 [n, C], distinct from every other argument; may be NULL exactly when the fused launch applies and the handle has no hub
 * rows, otherwise NULL returns GNX_ERR_INVALID naming d_work.  Allocation-free once the handle is reserved (gnx_graph_reserve: the
 * long-row slab); under capture it returns GNX_ERR_UNSUPPORTED naming gnx_graph_reserve where the slab would have to grow. */
int gnx_gcnii_step_bf16(gnx_graph_t g, const float *d_vals, const uint16_t *d_H, const float *d_H0, float a, int64_t C,
                        const float *d_M, int64_t ldm, int act, void *d_out, int out_bf16, float *d_work, void *stream);

/* gnx_gcnii_step_back (training, opt-in; added within ABI 0.9 -- probe for the symbol): the backward of gnx_gcnii_step past the relu
 * gate.  With G = g * (out > 0) (the caller's: its neighbours' rows are gathered, so the gated gradient exists in memory anyway, and
 * gnx_dense_wgrad reads the same array), Mt = M^T given by the caller as a [C, C] matrix (ldmt; the entry never transposes) and
 *   Z[r] = sum_c A_hat[c][r] G[c]      over the handle's transposed structure, d_vals_t = the values in transposed order as
 *                                      gnx_spmm_tv takes them (gnx_graph_permute_values_t / gnx_graph_normalize_t; NULL: the raw values),
 *   dH[r]    = ((1-a) Z[r]) . Mt                          -- the gradient of H,
 *   S_out[r] = s_alpha * S_in[r] + (a G[r]) . Mt          -- the layer's term of dH0, on top of a running sum.
 * d_S_in == NULL drops the s_alpha term, d_S_out == NULL skips the second product (d_S_in must then be NULL too), d_S_in == d_S_out
 * is allowed (in place).  G, dH, S_in, S_out: [n, C] contiguous f32; square graph; d_dH aliases neither d_G nor d_S_in / d_S_out.
 * (1-a) A^T (G Mt) = ((1-a) A^T G) Mt, so for C in {16, 32, 64} with the four matrices 16-byte aligned this is ONE launch of the
 * forward's shape for all rows of at most 512 entries of the transposed structure: G itself is gathered, G . Mt is never written or
 * read back, the rows (1-a) Z meet Mt in LDS on the matrix cores (v_mfma_f32_16x16x4_f32, exact float32), and the same tile then takes
 * a G[r] for the second product -- every row below n, hub rows and rows without entries included.  A row without entries gets
 * dH = 0, written.  Hub rows of the transposed structure go through the long-row kernels into d_dH and the dense kernel transforms those
 * rows alone, in place.  Other widths / alignments run today's order: gnx_dense(G, Mt) into d_work, gnx_spmm_tv(d_work) with
 * beta = 1 - a into d_dH (bit for bit those two calls), S_out = s_alpha S_in + a d_work through gnx_linear_combination (S_in, S_out
 * and d_work 16-byte aligned).
 * d_work: f32 [n, C], a buffer of its own; needed exactly when the fused launch does not apply -- NULL there returns GNX_ERR_INVALID
 * naming d_work.  No float atomics: per-row entry order, chunk order for hub rows and the k order of the MFMA are fixed, two calls give
 * the same bits (the fused launch does not give the bits of the composed order: the products associate differently).
 * Allocation-free once the handle is reserved with gnx_graph_reserve(C, GNX_RESERVE_TRANSPOSED); under capture it returns
 * GNX_ERR_UNSUPPORTED naming gnx_graph_reserve where the transposed structure or the long-row slab would have to be built or grown. */
int gnx_gcnii_step_back(gnx_graph_t g, const float *d_vals_t, const float *d_G, float a, int64_t C,
                        const float *d_Mt, int64_t ldmt, float *d_dH,
                        const float *d_S_in, float s_alpha, float *d_S_out,
                        float *d_work, void *stream);

/* Feature dropout of the GCNII training layer from the counter RNG of the edge dropout (opt-in; added within ABI 0.9 -- probe for the
 * symbols): gcn.py:27 / layered.py:44-45, dropout(act(...)), without a framework op, a byte mask or a second pass over the rows.
 * The mask: for a matrix [n, C], a rate 0 <= p < 1 and (seed, stream_id), element (i, c) is KEPT iff
 *   hash_u24(seed, stream_id + counter, i, c, 0) >= (uint32_t)(p * 2^24)
 * -- the 24-bit counter hash of the edge dropout with i = the handle's row id (not a launch slot), c = the column, duplicate rank 0,
 * counter = the handle's dropout counter (gnx_graph_set_dropout_counter; 0 when none is set), and
 *   drop(v) = kept ? v * s : +0.0f,   s = 1.0f / (1.0f - (float)p)      (the f32 scale of the edge dropout).
 * dropout_p is a double: the threshold is taken from the caller's value, so that 0.6 means (uint32_t)(0.6 * 2^24) = 10066329 and not
 * the 10066330 its float rounding would give.  p == 0 hashes nothing and is the plain path.  No float atomics, nothing random beyond
 * (seed, stream_id, counter): two calls give the same bits, and a captured launch draws fresh masks per replay through the counter.
 *
 * gnx_gcnii_step_drop: gnx_gcnii_step with out = drop(act(T . M)); d_mixed still receives the UNDROPPED mixed rows T (dM = T^T G needs
 * them).  For C in {16, 32, 64} with 16-byte aligned buffers it is the one launch of gnx_gcnii_step, the mask applied to a row's
 * values as they leave the tile (after the matrix-core block); hub rows go through the long-row kernels and the dense kernel as there
 * and then take the mask from the row-list pass below, in place.  Other widths / alignments run gnx_spmm and the dense kernel as
 * there, then the pass over all rows in place.  Rows without entries are masked like every other row.  The argument checks of
 * gnx_gcnii_step, plus 0 <= p < 1; its capture and reserve rules (nothing new is allocated).
 *
 * gnx_feature_dropout: the mask as a pass of its own, out[r] = drop(X[r]) for row ids r = d_rows[0 .. n_rows) (int32), or r = 0 ..
 * n_rows - 1 with d_rows == NULL; any width (16-byte accesses where C, the strides and the bases allow them), d_out may be d_X (with
 * ldo == ldx).  The handle is read for its dropout counter only: any handle will do.
 *
 * gnx_feature_dropout_back: the backward's gate in one pass over rows 0 .. n_rows - 1, G = kept ? g * s : +0, and with
 * act == GNX_ACT_RELU also +0 where y <= 0, y being the DROPPED forward output (y > 0 then implies kept: the hash is taken only where
 * y lets the value through).  d_y may be NULL with GNX_ACT_NONE; d_G may be d_g (with ldG == ldg). */
int gnx_gcnii_step_drop(gnx_graph_t g, const float *d_vals, const float *d_H, const float *d_H0, float a, int64_t C,
                        const float *d_M, int64_t ldm, int act, double dropout_p, uint64_t seed, uint64_t stream_id,
                        float *d_out, float *d_mixed, void *stream);
int gnx_feature_dropout(gnx_graph_t g, const float *d_X, int64_t ldx, int64_t n_rows, int64_t C, const int32_t *d_rows,
                        double dropout_p, uint64_t seed, uint64_t stream_id, float *d_out, int64_t ldo, void *stream);
int gnx_feature_dropout_back(gnx_graph_t g, const float *d_g, int64_t ldg, const float *d_y, int64_t ldy, int64_t n_rows, int64_t C,
                             double dropout_p, uint64_t seed, uint64_t stream_id, int act, float *d_G, int64_t ldG, void *stream);

/* bf16 row storage for GCNII TRAINING (opt-in; added within ABI 0.9 -- probe for the symbols): the rows a training-mode stack of GCNII
 * layers gathers -- the layer's input on the way forward, the gated gradient on the way back -- are stored as bf16 (uint16_t bit
 * patterns, [n, C] contiguous; bf = the cast of gnx_cast_bf16), everything that is summed stays f32.  With the feature dropout in the
 * launch (above) nothing sits between two layers, so layer l hands bf(out_l) straight to layer l + 1, as gnx_gcnii_step_bf16 does in
 * inference.  The two launch entries take C in {16, 32, 64} with the f32 buffers 16-byte and the bf16 buffers 8-byte aligned and
 * return GNX_ERR_UNSUPPORTED (naming the width or the alignment) for anything else, nothing launched: callers keep f32 there.  Square
 * stand-alone graphs without a diagonal.  No float atomics: two calls give the same bits.
 *
 * gnx_gcnii_step_train_bf16, the forward: gnx_gcnii_step_drop over bf16 gathered rows d_H,
 *   T = (1-a) * A_hat . H~ + a * H0 (f32, UNDROPPED, into d_mixed by the same launch: required),   out = drop(act(T . M)),
 * stored as f32 (out_bf16 = 0, float [n, C]) or as bf(.) (out_bf16 = 1, uint16_t [n, C]): that one store is the only rounding the
 * entry adds.  p == 0 hashes nothing.  Over bf16-representable H, d_mixed and an f32 out are bit for bit those of gnx_gcnii_step_drop
 * (gnx_gcnii_step at p == 0) over the widened H, a bf16 out the bits of gnx_cast_bf16 of that.  Hub rows go through the bf16 long-row
 * chunk kernels straight into d_mixed; the dense kernel transforms those rows alone (into d_out, or into d_work when out_bf16 = 1), the
 * row-list dropout pass masks them in place and they are rounded into d_out when out_bf16 = 1.  d_work: f32 [n, C], a buffer of its
 * own; may be NULL exactly when the handle has no hub rows (GNX_ERR_INVALID naming d_work otherwise).  Capture and reserve: as
 * gnx_gcnii_step_bf16.  Reports "spmm_gcnii_mfma_train_bf16".
 *
 * gnx_feature_dropout_back_bf16, the gate: gnx_feature_dropout_back reading the STORED bf16 forward output y and writing the gated
 * gradient twice, G = kept ? g * s : +0 (f32; with GNX_ACT_RELU also +0 where the stored y <= 0 -- a positive f32 value that rounded
 * to bf16 zero was stored as zero and passes no gradient) and Gb = bf(G), the operand the backward gathers.  One pass, any width;
 * p == 0 is the relu gate plus the cast.  d_y may be NULL with GNX_ACT_NONE; d_G may be d_g (with ldG == ldg).  Reports nothing.
 *
 * gnx_gcnii_step_back_bf16, the backward: gnx_gcnii_step_back with the GATHERED operand in bf16,
 *   Z[r] = sum_c A_hat[c][r] Gb~[c],   dH[r] = ((1-a) Z[r]) . Mt (f32),   S_out[r] = s_alpha * S_in[r] + (a G[r]) . Mt
 * -- the row's own product reads the f32 d_G, so the running dH0 sum never sees a rounded addend.  d_G may be NULL exactly when
 * d_S_out is NULL.  Over bf16-representable G (Gb = bf(G) exactly) dH and S_out are bit for bit those of gnx_gcnii_step_back.  Hub rows
 * of the transposed structure go through the bf16 long-row chunk kernels into d_dH and the dense kernel transforms those rows alone,
 * in place.  d_work is not used (the other widths are refused, not composed) and may be NULL.  The aliasing, capture and reserve rules
 * of gnx_gcnii_step_back.  Reports "spmm_gcnii_back_mfma_bf16". */
int gnx_gcnii_step_train_bf16(gnx_graph_t g, const float *d_vals, const uint16_t *d_H, const float *d_H0, float a, int64_t C,
                              const float *d_M, int64_t ldm, int act, double dropout_p, uint64_t seed, uint64_t stream_id,
                              void *d_out, int out_bf16, float *d_mixed, float *d_work, void *stream);
int gnx_feature_dropout_back_bf16(gnx_graph_t g, const float *d_g, int64_t ldg, const uint16_t *d_y, int64_t ldy, int64_t n_rows,
                                  int64_t C, double dropout_p, uint64_t seed, uint64_t stream_id, int act, float *d_G, int64_t ldG,
                                  uint16_t *d_Gb, int64_t ldGb, void *stream);
int gnx_gcnii_step_back_bf16(gnx_graph_t g, const float *d_vals_t, const uint16_t *d_Gb, const float *d_G, float a, int64_t C,
                             const float *d_Mt, int64_t ldmt, float *d_dH, const float *d_S_in, float s_alpha, float *d_S_out,
                             float *d_work, void *stream);

/* The GCNII weight gradient WITHOUT stored mixed rows (training, opt-in; added within ABI 0.9 -- probe for the symbols):
 *   dM = T^T . G,   T = (1-a) * A_hat . H + a * H0   made again from its operands inside the launch and never written,
 * so a training layer keeps neither T between its forward and its backward (4 bytes per element and layer) nor writes it in the forward
 * (gnx_gcnii_step / gnx_gcnii_step_drop with d_mixed == NULL, gnx_gcnii_step_drop_bf16 below), and gnx_dense_wgrad does not read it.
 * H (the rows the forward gathered: f32, or bf16 for gnx_gcnii_wgrad_bf16, widened exactly), H0 and G (the gated gradient in f32, the
 * array gnx_dense_wgrad reads) are [n, C] contiguous, dM is [C, C] contiguous f32; d_vals as in gnx_gcnii_step (NULL: the raw values).
 * Square stand-alone graphs without a diagonal.  C in {16, 32, 64} with the f32 buffers 16-byte and a bf16 d_H 8-byte aligned;
 * anything else returns GNX_ERR_UNSUPPORTED (naming the width or the alignment), nothing launched: callers keep the stored rows there.
 * One launch of the forward's shape: a wave makes a 16-row tile of T in LDS with the forward's gather loop, entry order and mix -- the
 * same device code, so a row of T has the bits gnx_gcnii_step would have stored in d_mixed -- and multiplies T_tile^T . G_tile into its
 * accumulators on the matrix cores (v_mfma_f32_16x16x4_f32, exact float32: a k-ordered fmaf chain over the tile's row slots), tile after
 * tile; slots past n contribute nothing, a row without entries a * H0[r].  Hub rows (longer than the handle's threshold:
 * gnx_graph_hub_rows) go through the long-row chunk kernels first, into d_hub_rows (f32 [n, C], indexed by row id; only the hub rows
 * are written), where the launch reads their T: one summation structure, no second weight gradient.  d_hub_rows may be NULL exactly
 * when the handle has no hub rows (GNX_ERR_INVALID naming d_hub_rows otherwise).
 * d_work: work_floats >= C * C floats, used as min(work_floats / (C * C), 2048, ceil(n / 128)) slabs of one [C, C] partial each -- a
 * block per slab, eight waves per block; the tile -> wave -> block assignment is a function of (n, C, the number of slabs) alone, never
 * of the device -- added in slab order into d_dM by the last pass of gnx_dense_wgrad.  No float atomics: two calls with the same
 * arguments give the same bits; another work_floats gives another summation order.  d_dM, d_work and d_hub_rows are each a buffer of
 * their own.  The summation order is not gnx_dense_wgrad's over the stored T: the two agree to float32 rounding.
 * Capture and reserve: as gnx_gcnii_step_bf16 (the long-row slab; nothing else is allocated).
 * Reports "gcnii_wgrad_mfma" / "gcnii_wgrad_mfma_bf16".
 *
 * gnx_gcnii_step_drop_bf16, the forward that goes with gnx_gcnii_wgrad_bf16: gnx_gcnii_step_train_bf16 without d_mixed -- T never
 * reaches memory except for hub rows, which go through d_work (f32 [n, C], a buffer of its own; may be NULL exactly when the handle has
 * no hub rows) as in gnx_gcnii_step_bf16.  out has the bits of gnx_gcnii_step_train_bf16's out; its checks, widths and alignments
 * (GNX_ERR_UNSUPPORTED elsewhere).  Reports "spmm_gcnii_mfma_drop_bf16".  (The f32 side needs no new forward: gnx_gcnii_step and
 * gnx_gcnii_step_drop take d_mixed == NULL at these widths.) */
int gnx_gcnii_wgrad(gnx_graph_t g, const float *d_vals, const float *d_H, const float *d_H0, float a, int64_t C,
                    const float *d_G, float *d_dM, float *d_hub_rows, float *d_work, int64_t work_floats, void *stream);
int gnx_gcnii_wgrad_bf16(gnx_graph_t g, const float *d_vals, const uint16_t *d_H, const float *d_H0, float a, int64_t C,
                         const float *d_G, float *d_dM, float *d_hub_rows, float *d_work, int64_t work_floats, void *stream);
int gnx_gcnii_step_drop_bf16(gnx_graph_t g, const float *d_vals, const uint16_t *d_H, const float *d_H0, float a, int64_t C,
                             const float *d_M, int64_t ldm, int act, double dropout_p, uint64_t seed, uint64_t stream_id,
                             void *d_out, int out_bf16, float *d_work, void *stream);

/* The spectral-preserving GCNII layer (gcn.py:30-51) as one launch (opt-in; added within ABI 0.9 -- probe for the symbols), f32 rows:
 *   out = 2 * drop(act(P') - bias),   P' = T . M + bias,   T = (1-a) A . H + a H0
 * with drop, its mask and its scale s those of gnx_gcnii_step_drop above (p == 0 hashes nothing: out = 2 * (act(P') - bias)).
 *
 * gnx_gcnii_step_spectral: the launch of gnx_gcnii_step / gnx_gcnii_step_drop with another epilogue; d_bias is [C] f32.  Rounding
 * points: P' = fl(T . M + bias[c]), the bias added to the accumulator value as it leaves the matrix-core block, before the
 * activation; then Y = fl(act(P') - bias[c]), and out = 2 * (kept ? fl(Y * s) : +0).  d_mixed, when given, receives the undropped T,
 * bit for bit that of gnx_gcnii_step.
 * d_gate (uint32_t [n, ceil(C / 32)] contiguous; written for GNX_ACT_RELU only, may be NULL in inference): one bit per element,
 *   bit (c & 31) of word row * ceil(C / 32) + (c >> 5)  =  (P'[row, c] > 0);
 * the bits above C of a row's last word (the upper 16 at C = 16, the upper 8 of the one word at C = 24) are 0.  The gate is taken from
 * the pre-activation itself -- fl(relu(P') - bias) equals -bias for a tiny positive P', so it cannot be read back from out -- and is all
 * the backward needs of the forward: neither act(P') nor out has to be kept.  Every row's words are written whole by ONE lane with a
 * plain vector store (the lanes of a row OR their bits together first): no atomics.
 * Hub rows take the long-row kernels and the dense kernel (with the bias) on those rows alone, as in gnx_gcnii_step, and then a row-list
 * pass that applies - bias, the mask, x 2 and writes their gate words with the store loop's own code: a row has the same bits whichever
 * path made it.  Widths other than 16 / 32 / 64 (they need d_mixed) and unaligned buffers run gnx_spmm, the dense kernel and that pass
 * over all rows.  The argument checks of gnx_gcnii_step_drop, and: d_bias non-NULL; d_gate non-NULL when act is GNX_ACT_RELU and
 * d_mixed is given at one of the three widths (training; at the other widths every call passes d_mixed); d_bias and d_gate buffers of their own.  Its capture and reserve rules.  Reports
 * "spmm_gcnii_spectral_mfma" / "spmm_gcnii_spectral_mfma_drop" (p > 0), the other widths "spmm+dense_mfma_spectral" /
 * "spmm+dense_mfma_spectral_drop".
 *
 * gnx_gcnii_spectral_back: the first pass of the layer's backward, over rows 0 .. n_rows - 1 of the upstream gradient g (ldg) and the
 * gate words the forward wrote, with the forward's (p, seed, stream_id):  u = 2 * (kept ? fl(g * s) : +0),
 *   G'[i, c]  = gate ? u : +0          -- the gradient with respect to P': what gnx_dense_wgrad (dM = T^T G') and the dH / dH0 launches take;
 *   dbias[c]  = - sum_i (gate ? 0 : u[i, c])   -- where the relu is open the + bias and the - bias cancel, where it is shut - bias is left.
 * With GNX_ACT_NONE there is no gate (d_gate, d_work may be NULL): G' = u and dbias is written as exact zeros.  d_G may be d_g (with
 * ldG == ldg); d_dbias is [C].  No float atomics: block b of min(2048, ceil(n_rows / 256)) blocks -- a function of n_rows alone --
 * takes a contiguous range of rows, adds them in a fixed order into slab b ([C] floats) of d_work, and the slabs are added in index
 * order, as in gnx_gcnii_wgrad: two calls give the same bits on every device.  work_floats >= min(2048, ceil(n_rows / 256)) * C.  The
 * handle is read for its dropout counter only.  Reports nothing. */
int gnx_gcnii_step_spectral(gnx_graph_t g, const float *d_vals, const float *d_H, const float *d_H0, float a, int64_t C,
                            const float *d_M, int64_t ldm, const float *d_bias, int act, double dropout_p, uint64_t seed,
                            uint64_t stream_id, float *d_out, float *d_mixed, uint32_t *d_gate, void *stream);
int gnx_gcnii_spectral_back(gnx_graph_t g, const float *d_g, int64_t ldg, const uint32_t *d_gate, int64_t n_rows, int64_t C, int act,
                            double dropout_p, uint64_t seed, uint64_t stream_id, float *d_G, int64_t ldG, float *d_dbias,
                            float *d_work, int64_t work_floats, void *stream);

/* The GCNII layer UNDER EDGE DROPOUT as one launch, forward and backward (training, opt-in; added within ABI 0.9 -- probe for the
 * symbols), f32 rows: gnx_gcnii_step / gnx_gcnii_step_drop and gnx_gcnii_step_back over the dropped + symmetrically re-normalised
 * adjacency of one training iteration WITHOUT its value array.  (d_D, edge_p, edge_seed, edge_stream) are the arguments of
 * gnx_spmm_dropped: d_D the degree scales of that (seed, stream) (gnx_graph_colsum + gnx_degree_scale), and the weight of stored entry
 * (r, c) is made in the gather loop with the arithmetic of gnx_graph_scale_values,
 *   w = fl(fl(D[r] * fl(raw * s_e)) * D[c]) if hash_u24(edge_seed, edge_stream + counter, r, c, 0) >= int(edge_p * 2^24), else 0,
 * s_e the f32 1 / (1 - edge_p) -- bit for bit the value gnx_graph_normalize(symmetric, no add_eye, edge_p, edge_seed, edge_stream)
 * stores there; on a handle after gnx_graph_enable_entry_dropout a slot's weight is its kept sum, as in gnx_spmm_dropped.  Entry order,
 * the entries in flight, the fmaf chain, the mix, the transform and the long-row path are those of the constant-adjacency entries, so
 * every result has the bits of that entry over the materialised values.  SKIP SEMANTICS: an entry of weight exactly 0 (dropped, or a
 * kept sum of 0) does not gather its row, where the materialised form multiplies it by 0: the precondition of gnx_spmm_dropped --
 * finite features and finite degree scales -- holds here unchanged (0 * inf and 0 * NaN make a NaN there and not here).  A row all
 * of whose entries are dropped gives out = act((a H0[r]) . M) and dH[r] = 0.
 *
 * gnx_gcnii_step_dropped: out = drop_f(act(T . M)), T = (1-a) A_d . H + a H0; (feat_p, feat_seed, feat_stream) the feature mask of
 * gnx_gcnii_step_drop, keyed by (row, column) and made in the store loop -- feat_p == 0 means no mask and hashes nothing.  Rounding
 * points: those of gnx_gcnii_step_drop, with w above in place of the loaded value.  d_mixed receives the undropped T (NULL allowed at
 * C = 16 / 32 / 64 with aligned buffers).  Hub rows: the chunk kernels of gnx_spmm_dropped over the same weights, then the dense kernel
 * and the mask pass on those rows alone, as in gnx_gcnii_step_drop.  Other widths and misaligned buffers (they need d_mixed) run
 * gnx_spmm_dropped, the dense kernel and the mask pass.  Reports "spmm_gcnii_mfma_edrop" / "spmm_gcnii_mfma_edrop_drop" (feat_p > 0),
 * the other widths "spmm+dense_mfma_edrop" / "spmm+dense_mfma_edrop_drop".
 *
 * gnx_gcnii_step_back_dropped: the contract of gnx_gcnii_step_back (dH, S_in / s_alpha / S_out, d_work for the other widths, the
 * aliasing rules) with the weights of the transposed walk made from the same (d_D, edge_p, edge_seed, edge_stream): transposed entry
 * (r, c) is A_d[c][r] and draws with (c, r).  Reports "spmm_gcnii_back_mfma_edrop", the other widths "dense+spmm_back_edrop".
 *
 * Both refuse (GNX_ERR_UNSUPPORTED) a handle with duplicate COO entries and no entry tables, need a square stand-alone graph (no
 * vertex block), honour the handle's dropout counter for both masks, and follow the capture and reserve rules of the entries they
 * mirror (gnx_graph_reserve with GNX_RESERVE_TRANSPOSED before a captured backward).  No float atomics; no scratch beyond the
 * handle's long-row slab. */
int gnx_gcnii_step_dropped(gnx_graph_t g, const float *d_D, float edge_p, uint64_t edge_seed, uint64_t edge_stream, const float *d_H,
                           const float *d_H0, float a, int64_t C, const float *d_M, int64_t ldm, int act, double feat_p,
                           uint64_t feat_seed, uint64_t feat_stream, float *d_out, float *d_mixed, void *stream);
int gnx_gcnii_step_back_dropped(gnx_graph_t g, const float *d_D, float edge_p, uint64_t edge_seed, uint64_t edge_stream,
                                const float *d_G, float a, int64_t C, const float *d_Mt, int64_t ldmt, float *d_dH,
                                const float *d_S_in, float s_alpha, float *d_S_out, float *d_work, void *stream);

/* ---- the GCN layer in one launch (opt-in; added within ABI 0.9 -- probe for the symbols) -------------------------------
 * GCNLayer.__forward__ (gcn.py:88-89): out = drop(act((A . X) . W + bias)) -- the aggregation at the input width and the transform,
 * which gnx_spmm + gnx_dense run as two launches with the [n, C_in] matrix A . X written and read back between them.  X [n, C_in]
 * (ldx), W [C_in, C_out] (ldw), bias [C_out] or NULL, out [n, C_out] (ldo), all f32; act GNX_ACT_NONE or GNX_ACT_RELU.
 *
 * gnx_gcn_step: d_vals as in gnx_spmm (NULL: the handle's raw values).  For C_in in {16, 32, 64}, 1 <= C_out <= C_in, ldx % 4 == 0 and
 * 16-byte aligned X / d_agg / d_work it is ONE launch: a wave gathers a 16-row tile into LDS (entries in ascending order, four in
 * flight, one fmaf chain: the loop of gnx_gcnii_step without the mix), multiplies it by W -- in LDS, its columns padded with zeros to
 * a multiple of 16 there and nowhere else -- on v_mfma_f32_16x16x4_f32, adds the bias to the accumulator as it leaves the matrix
 * cores, applies the activation and stores the columns below C_out: whole 16-byte pieces where ldo % 4 == 0 and out is 16-byte
 * aligned, single values otherwise (C_out = 7 with ldo = 7 is fine); nothing is written past column C_out - 1 of any row.
 * Rounding points: each aggregated value is one fmaf chain over the row's entries; each output the f32 MFMA sum over k in
 * ascending order, then + bias, then the activation, then the mask.
 * d_agg [n, C_in] f32 contiguous or NULL: receives the aggregated rows A . X, written once by the lanes that made them and never
 * read back for the transform (training keeps them for dW = agg^T G'); it does not change a bit of out.
 * (dropout_p, seed, stream_id): the feature mask of gnx_gcnii_step_drop over the finished rows -- element (i, c) is kept iff
 * hash_u24(seed, stream_id + counter, i, c, 0) >= int(dropout_p * 2^24), kept values times the f32 1 / (1 - dropout_p), dropped ones
 * +0; dropout_p == 0 hashes nothing.  d_agg stays undropped.
 * Rows longer than the handle's long-row threshold (hub rows) take the long-row kernels of gnx_spmm, then the dense kernel on those
 * rows alone, then the mask pass on them; their aggregated rows go through d_agg, else through d_work (f32, at least n * C_in).
 * Every other case -- C_in outside {16, 32, 64}, C_out > C_in, misaligned rows -- runs gnx_spmm, the dense kernel and the mask pass
 * inside the call, through d_agg, else d_work.  Where a place for those rows is needed and both are NULL the call is refused, and
 * the message says which case needs it.
 * Checked before anything is launched (a refused call writes nothing): NULL handle / X / W / out, the activation, the rate in
 * [0, 1), ldx >= C_in, ldw >= C_out, ldo >= C_out, a square graph; out, d_agg and d_work are buffers of their own (none aliases
 * X, W, bias, the values, or another of the three).  Stream-ordered; under capture the long-row slab must already cover C_in
 * (gnx_graph_reserve), as for gnx_spmm.  No float atomics.
 * Reports "k_spmm_gcn<C_in>" (+ "_edrop" under edge dropout, + "_drop" with a mask, + "+long" when hub rows ran), the composed
 * form "spmm+dense_mfma_gcn" with the same suffixes.
 *
 * gnx_gcn_step_dropped: the same layer under the edge dropout of gnx_spmm_dropped -- (d_D, edge_p, edge_seed, edge_stream) as in
 * gnx_gcnii_step_dropped: every entry's weight is made in the gather loop, bit for bit the value gnx_graph_normalize(symmetric, no
 * add_eye, edge_p, edge_seed, edge_stream) stores, so out and d_agg have the bits of gnx_gcn_step over the materialised values (skip
 * semantics and the finite-features precondition of gnx_spmm_dropped).  Admission as gnx_gcnii_step_dropped: a square stand-alone
 * graph; a handle with duplicate COO entries needs gnx_graph_enable_entry_dropout. */
int gnx_gcn_step(gnx_graph_t g, const float *d_vals, const float *d_X, int64_t ldx, int64_t C_in, const float *d_W, int64_t ldw,
                 int64_t C_out, const float *d_bias, int act, double dropout_p, uint64_t seed, uint64_t stream_id, float *d_out,
                 int64_t ldo, float *d_agg, float *d_work, void *stream);
int gnx_gcn_step_dropped(gnx_graph_t g, const float *d_D, float edge_p, uint64_t edge_seed, uint64_t edge_stream, const float *d_X,
                         int64_t ldx, int64_t C_in, const float *d_W, int64_t ldw, int64_t C_out, const float *d_bias, int act,
                         double dropout_p, uint64_t seed, uint64_t stream_id, float *d_out, int64_t ldo, float *d_agg,
                         float *d_work, void *stream);

/* The spectral-preserving GCN layer (GCNSpectralPreservingLayer, gcn.py:92-105) as one launch (opt-in; added within ABI 0.9 -- probe
 * for the symbols), f32 rows:
 *   out = 2 * drop(act(P') - bias),   P' = (A . X) . W + bias
 * gnx_step_spectral_gcn is the launch of gnx_gcn_step with another store loop, gnx_step_spectral_gcn_dropped that of
 * gnx_gcn_step_dropped; the arguments, widths, strides, d_agg / d_work, the hub rows, the composed form of the other cases, the checks
 * (before any launch: a refused call writes nothing), the aliasing, capture and reserve rules, the skip semantics and the admission
 * under edge dropout are those entries', and d_agg is bit for bit theirs.  act is GNX_ACT_NONE or GNX_ACT_RELU.
 * Rounding points: each aggregated value is one fmaf chain over the row's entries; P' = fl(sum + bias[c]), the f32 MFMA sum over k
 * in ascending order with the bias added to the accumulator value as it leaves the matrix-core block, before the activation; then
 * Y = fl(act(P') - bias[c]); then out = 2 * (kept ? fl(Y * s) : +0), the mask and its f32 scale s = 1 / (1 - dropout_p) those of
 * gnx_gcn_step (dropout_p == 0 hashes nothing: out = 2 * Y).  d_bias NULL means a bias of zeros: out = 2 * drop(act(P')), and the
 * gate is still written.  With d_bias of zeros and dropout_p == 0, out is exactly twice gnx_gcn_step's.
 * d_gate (uint32_t [n, ceil(C_out / 32)] contiguous; written for GNX_ACT_RELU only, may be NULL in inference): one bit per element,
 *   bit (c & 31) of word row * ceil(C_out / 32) + (c >> 5)  =  (P'[row, c] > 0),
 * the format of gnx_gcnii_step_spectral at the OUTPUT width: the bits at or above C_out of a row's last word are 0, and no word at or
 * above ceil(C_out / 32) exists or is written.  The gate is taken from the pre-activation itself and is all the backward needs of
 * the forward (gnx_gcnii_spectral_back takes it at any width and row stride, then gnx_dense_wgrad and gnx_gcn_step_back).  Every
 * word is written whole by ONE lane with a plain vector store, after the lanes of the word OR their bits together: no atomics.  The
 * partial-piece store rules of gnx_gcn_step hold (C_out = 7 with ldo = 7 is fine): nothing is written past column C_out - 1.
 * Hub rows take the long-row kernels, the dense kernel with the bias on those rows alone, and a row-list pass that applies - bias, the
 * mask, x 2 and writes their gate words with the store loop's own code: a row has the same bits whichever path made it.  C_in
 * outside {16, 32, 64}, C_out > C_in and misaligned rows run gnx_spmm (gnx_spmm_dropped), the dense kernel and that pass over all
 * rows, through d_agg, else d_work.
 * Beyond gnx_gcn_step's checks: d_gate non-NULL when act is GNX_ACT_RELU and d_agg is given (training); d_gate a buffer of its own.
 * Reports "k_spmm_gcn_spectral<C_in>" (+ "_edrop" under edge dropout, + "_drop" with a mask, + "+long" when hub rows ran), the
 * composed form "spmm+dense_mfma_gcn_spectral" with the same suffixes. */
int gnx_step_spectral_gcn(gnx_graph_t g, const float *d_vals, const float *d_X, int64_t ldx, int64_t C_in, const float *d_W,
                          int64_t ldw, int64_t C_out, const float *d_bias, int act, double dropout_p, uint64_t seed,
                          uint64_t stream_id, float *d_out, int64_t ldo, float *d_agg, uint32_t *d_gate, float *d_work, void *stream);
int gnx_step_spectral_gcn_dropped(gnx_graph_t g, const float *d_D, float edge_p, uint64_t edge_seed, uint64_t edge_stream,
                                  const float *d_X, int64_t ldx, int64_t C_in, const float *d_W, int64_t ldw, int64_t C_out,
                                  const float *d_bias, int act, double dropout_p, uint64_t seed, uint64_t stream_id, float *d_out,
                                  int64_t ldo, float *d_agg, uint32_t *d_gate, float *d_work, void *stream);

/* gnx_gcn_step_back (training, opt-in; added within ABI 0.9 -- probe for the symbols): the gradient of X of gnx_gcn_step past the gate,
 *   dX[r, 0 .. C_in) = (sum_c A_hat[c][r] G'[c, 0 .. C_out)) . Wt,
 * G' [n, C_out] (ldg) the gated gradient the caller holds (gnx_dense_wgrad and the column sums read the same array), Wt = W^T given by
 * the caller as a [C_out, C_in] matrix (ldwt; the entry never transposes), dX [n, C_in] (lddx), d_vals_t the values in transposed
 * order as gnx_spmm_tv takes them (NULL: the raw values).  A^T (G' Wt) = (A^T G') Wt: for C_in in {16, 32, 64}, 1 <= C_out <= C_in,
 * ldg % 4 == 0, ldg >= roundup4(C_out), lddx % 4 == 0 and 16-byte aligned G' / dX / d_work it is ONE launch over the rows of at most the
 * long-row threshold of the transposed structure, and G' is gathered AT THE OUTPUT WIDTH: a row is walked by 4 NTG lanes, 16 NTG the
 * smallest of 16, 32, 64 that holds C_out (entries in ascending order, four in flight, one fmaf chain: the loop of
 * gnx_gcnii_step_back), every gather a whole 16-byte load -- the columns C_out .. roundup4(C_out) - 1 of a row of G' must be readable
 * and their content does not matter (they are selected away, never multiplied: a NaN there stays out of dX) -- and the gathered tile
 * meets Wt, in LDS with its rows from C_out on zero-filled there and nowhere else, on v_mfma_f32_16x16x4_f32 with k over the gathered
 * width in ascending order.  The [n, C_in] product G' . Wt is never written or gathered back.  A row without entries gets dX = 0,
 * written.  Hub rows of the transposed structure go through the long-row kernels at width C_out into d_work, at their row ids
 * ([n, C_out] contiguous), and the dense kernel transforms those rows alone into d_dX.  At C_out == C_in the result is bit for bit
 * gnx_gcnii_step_back(a = 0, Mt = Wt, S_out = NULL).
 * Every other case -- C_in outside {16, 32, 64}, C_out > C_in, ldg % 4 != 0 or ldg < roundup4(C_out), misaligned rows -- runs today's
 * order inside the call: gnx_dense(G', Wt) into d_work [n, C_in], then gnx_spmm_tv into d_dX; bit for bit those two calls.
 * d_work / work_floats: NULL (with 0) only where nothing passes through memory -- the one launch on a graph whose transposed structure
 * has no hub rows; else at least n * C_out floats (the one launch with hub rows) or n * C_in (the composed order).  Too little returns
 * GNX_ERR_INVALID and names what is needed and why.
 * Checked before anything is launched (a refused call writes nothing): NULL handle / G' / Wt / dX, the widths, ldg >= C_out,
 * ldwt >= C_in, lddx >= C_in, work_floats, a square graph; dX aliases no input and d_work is a buffer of its own.  No float atomics:
 * two calls give the same bits (the one launch does not give the bits of the composed order: the products associate differently).
 * Capture and reserve rules of gnx_gcnii_step_back (gnx_graph_reserve(C, GNX_RESERVE_TRANSPOSED) before a captured call).
 * Reports "k_spmm_gcn_back<C_in>" (+ "_edrop" under edge dropout, + "+long" when hub rows ran), the composed order
 * "dense+spmm_back_gcn" (+ "_edrop").
 *
 * gnx_gcn_step_back_dropped: the same under the edge dropout of gnx_spmm_dropped, the weights of the transposed walk made from
 * (d_D, edge_p, edge_seed, edge_stream) as in gnx_gcnii_step_back_dropped -- bit for bit gnx_gcn_step_back over the transposed values
 * of the materialised adjacency (skip semantics: finite G'); the composed order runs gnx_spmm_dropped(transposed = 1).  Admission as
 * gnx_gcnii_step_dropped. */
int gnx_gcn_step_back(gnx_graph_t g, const float *d_vals_t, const float *d_G, int64_t ldg, int64_t C_out, const float *d_Wt,
                      int64_t ldwt, int64_t C_in, float *d_dX, int64_t lddx, float *d_work, int64_t work_floats, void *stream);
int gnx_gcn_step_back_dropped(gnx_graph_t g, const float *d_D, float edge_p, uint64_t edge_seed, uint64_t edge_stream,
                              const float *d_G, int64_t ldg, int64_t C_out, const float *d_Wt, int64_t ldwt, int64_t C_in,
                              float *d_dX, int64_t lddx, float *d_work, int64_t work_floats, void *stream);

/* ---- the NGCF layer in one launch (opt-in; added within ABI 0.9 -- probe for the symbols) ------------------------------
 * NGCFLayer.__forward__ (gcn.py:116-135), A_hat the bipartite-normalised adjacency the caller built once:
 *   A = A_hat . X      P1 = (X * A) . W1 + b1      P2 = A . W2 + b2      u = act(P1) + act(P2)      out = l2_normalize(drop(u))
 * X [n, C_in] (ldx), W1 and W2 [C_in, C_out] (ldw1, ldw2), b1 and b2 [C_out] or NULL (each on its own), out [n, C_out] (ldo), all f32;
 * act GNX_ACT_NONE, GNX_ACT_RELU or GNX_ACT_LEAKY; normalize 0 or 1 (0: out = drop(u)).  d_vals as in gnx_spmm.
 *
 * gnx_ngcf_step: for C_in in {16, 32, 64}, 1 <= C_out <= C_in, ldx % 4 == 0 and 16-byte aligned X / d_agg / d_work it is ONE launch
 * over the rows of at most the long-row threshold: a wave gathers a 16-row tile into LDS exactly as gnx_gcn_step does (d_agg, when
 * given, is bit for bit gnx_gcn_step's d_agg); tile . W2 runs on v_mfma_f32_16x16x4_f32 with + b2 and the activation applied as the
 * accumulator leaves the matrix cores, and that term STAYS in the accumulator registers; each lane multiplies its four columns of
 * the tile in place by the row's own X[row, c .. c + 3]; tile . W1 runs, + b1, the activation, and act(P1) + act(P2) -- one f32 add
 * per element -- goes back through the same tile (one tile per wave).  Both weights sit in LDS, zero-padded to a multiple of 16
 * columns there and nowhere else.
 * Rounding points: A as in gnx_gcn_step; X * A one multiply; each P the f32 MFMA sum over k ascending, then + bias; the activation
 * (leaky: one multiply by 0.2f where P <= 0); one add; the mask (x * scale); with normalize the row's sum of squares over the
 * columns below C_out -- per lane one fmaf chain over its four columns ascending from 0, then the row's 4, 8 or 16 lanes added
 * through xor-shuffles at strides 1, 2, 4, 8 --, r = 1 / sqrt(max(sum, 1e-12f)) with the IEEE square root and division (each
 * correctly rounded), and out = x * r.
 * d_gate (uint32_t [n, 2 * ceil(C_out / 32)] contiguous; written for GNX_ACT_RELU and GNX_ACT_LEAKY, may be NULL): per row first the
 * ceil(C_out / 32) words of P1, then those of P2; bit c & 31 of word c >> 5 = (P[row, c] > 0), taken from the biased
 * pre-activation itself.  Bits beyond C_out are 0.
 * d_rnorm (float [n], only with normalize, may be NULL): r of the row, NEGATED where the clamp acted (sum < 1e-12f: r = -1e6f) --
 * the sign is how gnx_ngcf_back_gate tells the two derivatives apart; |d_rnorm| is the factor either way.
 * (dropout_p, seed, stream_id): the feature mask of gnx_gcn_step, applied to u before the norm.  d_agg, d_gate and d_rnorm do not
 * change a bit of out.  Nothing is written past column C_out - 1 of any row of out (whole 16-byte stores where ldo % 4 == 0 and out
 * is 16-byte aligned, single values otherwise).
 * Hub rows take the long-row kernels of gnx_spmm into d_agg, else into the first roundup4(n * C_in) floats of d_work, at their row
 * ids; on those rows alone the call then runs a product pass (X * A into compact rows), the dense kernel twice without activation,
 * and a row pass that runs the store loop's own code (activations, sum, gate words, mask, norm).  Every other case -- C_in outside
 * {16, 32, 64}, C_out > C_in, misaligned rows -- runs gnx_spmm and the same composition over all rows inside the call.
 * d_work / work_floats: with k = the handle's hub rows (gnx_graph_hub_rows) on the fused widths, k = n in the composed form,
 *     work_floats >= (k > 0 ? (d_agg ? 0 : roundup4(n * C_in)) + roundup4(k * C_in) + k * C_out : 0)
 * -- beyond gnx_gcn_step's [n, C_in] share the scratch of the fused widths grows with the hub rows, not with n.  NULL with 0 where
 * the formula gives 0.  Too little is refused and the message names the figure.
 * Checked before anything is launched (a refused call writes nothing): the checks of gnx_gcn_step, and W2 / ldw2, normalize in
 * {0, 1}, d_rnorm only with normalize, work_floats; out, d_agg, d_gate, d_rnorm and d_work are buffers of their own.  Stream-ordered;
 * no float atomics; under capture the long-row slab must already cover C_in (gnx_graph_reserve), as for gnx_gcn_step.
 * Reports "k_spmm_ngcf<C_in>" (+ "_drop" with a mask, + "_norm" with normalize, + "+long" when hub rows ran), the composed form
 * "spmm+dense_mfma_ngcf" with the same suffixes.
 *
 * gnx_ngcf_back_gate: the backward's first pass, elementwise with one row reduction.  g [n_rows, C_out] (ldg) the gradient of out,
 * y (ldy) the forward's out, d_rnorm and d_gate what the forward wrote:
 *   g_s = r (g - y (y . g))   where d_rnorm[row] = r > 0
 *   g_s = |r| g               where d_rnorm[row] < 0 (the clamp acted: out = 1e6f x there)
 *   g_s = g                   with d_rnorm == NULL: no normalisation was applied (d_y may then be NULL)
 *   g_u = kept ? g_s * scale : +0          the forward's mask made again from (dropout_p, seed, stream_id, the handle's counter)
 *   G1  = bit1 ? g_u : g_u * slope         G2 likewise with bit2; slope = 0.2f (LEAKY), 0 (RELU); GNX_ACT_NONE: G1 = G2 = g_u and
 *                                          d_gate is not looked at
 * G1 and G2 [n_rows, C_out] are written at row stride ldG; the columns C_out .. min(ldG, roundup4(C_out)) - 1 are written as zeros,
 * so that rows of stride roundup4(C_out) are whole 16-byte pieces for gnx_dense_wgrad, gnx_dense and the column sums.  y . g is
 * summed per lane as one fmaf chain (16 lanes per row, lane l the columns 4 l .. 4 l + 3 of every 64), then through xor-shuffles: no
 * float atomics, two calls give the same bits.  G1 and G2 are buffers of their own.  Reports nothing. */
int gnx_ngcf_step(gnx_graph_t g, const float *d_vals, const float *d_X, int64_t ldx, int64_t C_in, const float *d_W1, int64_t ldw1,
                  const float *d_W2, int64_t ldw2, int64_t C_out, const float *d_b1, const float *d_b2, int act, double dropout_p,
                  uint64_t seed, uint64_t stream_id, int normalize, float *d_out, int64_t ldo, float *d_agg, uint32_t *d_gate,
                  float *d_rnorm, float *d_work, int64_t work_floats, void *stream);
int gnx_ngcf_back_gate(gnx_graph_t g, const float *d_g, int64_t ldg, const float *d_y, int64_t ldy, const float *d_rnorm,
                       const uint32_t *d_gate, int64_t n_rows, int64_t C_out, int act, double dropout_p, uint64_t seed,
                       uint64_t stream_id, float *d_G1, float *d_G2, int64_t ldG, void *stream);

/* gnx_step_back_ngcf (training, opt-in; added within ABI 0.9 -- probe for the symbol): the backward of gnx_ngcf_step around its two
 * weight gradients, from what the forward kept -- X (ldx), A = d_agg [n, C_in] contiguous, d_gate, d_rnorm, y (ldy) -- and the
 * upstream gradient g (ldg), over the handle's n rows:
 *   G1, G2 = gnx_ngcf_back_gate's        db1 = sum_rows G1       db2 = sum_rows G2       P = X * A
 *   Q1 = G1 . W1^T      Q2 = G2 . W2^T      dA = Q1 * X + Q2      R = Q1 * A      dX = A_hat^T . dA + R
 * (dW1 = P^T . G1 and dW2 = A^T . G2 stay with gnx_dense_wgrad.)  For C_in in {16, 32, 64}, 1 <= C_out <= C_in, ldx % 4 == 0,
 * ldG % 4 == 0 and 16-byte aligned X / d_agg / G1 / G2 / P / dA / R; anything else returns GNX_ERR_UNSUPPORTED naming the width or the
 * alignment, nothing launched: there is no composed form inside the entry, callers keep the composed backward there.
 * ONE row-local launch without a gather: a wave takes 16 rows, makes their G1 / G2 with the arithmetic of gnx_ngcf_back_gate -- bit
 * for bit its results; written at row stride ldG with zeros in the columns C_out .. roundup4(C_out) - 1 --, puts G2 and then G1
 * through one tile in LDS against W2^T and W1^T (read from W1 / W2 [C_in, C_out] as stored, ldw1 / ldw2, laid down transposed in LDS:
 * no transposed copy is needed) on v_mfma_f32_16x16x4_f32, and walks the rows.
 * Rounding points: G1 / G2 as gnx_ngcf_back_gate; P one multiply; each Q the f32 MFMA sum over the output columns ascending;
 * dA = fmaf(Q1, X, Q2), one rounding; R one multiply.  db: a block covers a contiguous range of rows that depends on n alone, adds
 * the G1 / G2 columns of its rows in a fixed order into slab b of d_work, and two finishing launches add the slabs in index order, in groups of 64 and then the group sums -- no
 * float atomics: two calls give the same bits.
 * Then, when d_dX is given, gnx_spmm_tv(d_dA, H0 = d_R, beta = 1, alpha = 1) into d_dX (lddx) inside the call: d_vals_t the
 * adjacency's values in transposed order (NULL: the raw values); hub rows of the transposed structure are that launch's business.
 * d_dA and d_R: caller buffers [n, C_in] contiguous, observable afterwards.  d_dX == NULL: no products and no SpMM (X needs no
 * gradient); d_dA, d_R, d_W1 and d_W2 may then be NULL and are not looked at.  d_P, d_db1, d_db2 may each be NULL.  d_dX is a buffer
 * of its own (it may NOT be d_R).
 * d_work / work_floats (only where d_db1 or d_db2 is given): with s = max(1, min(8192, ceil(ceil(n / 16) / 4))) slabs,
 *     work_floats >= (s + ceil(s / 64)) * 2 * C_out
 * -- a slab per block and, behind them, a sum per group of 64 slabs (the finishing launches add the groups, then the group sums).
 * Too little is refused and the message names the figure.
 * Checked before anything is launched (a refused call writes nothing): the checks of gnx_ngcf_back_gate, the widths, pointers and
 * strides, a square stand-alone graph; every output -- G1, G2, P, db1, db2, dA, R, dX, d_work -- is a buffer of its own.
 * Stream-ordered and allocation-free once the handle is reserved; under capture the transposed structure and the long-row slab at
 * width C_in must exist already (gnx_graph_reserve with GNX_RESERVE_TRANSPOSED), as for gnx_spmm_tv.
 * Reports "k_ngcf_back<C_in>" (+ "_drop" with a mask, + "+spmm_tv" when dX ran).
 * (The layer's name stands behind the verb in this entry's name; gnx_ngcf_step and gnx_ngcf_back_gate keep theirs.) */
int gnx_step_back_ngcf(gnx_graph_t g, const float *d_vals_t, const float *d_g, int64_t ldg, const float *d_y, int64_t ldy,
                       const float *d_rnorm, const uint32_t *d_gate, int64_t C_out, int act, double dropout_p, uint64_t seed,
                       uint64_t stream_id, const float *d_X, int64_t ldx, const float *d_agg, int64_t C_in, const float *d_W1,
                       int64_t ldw1, const float *d_W2, int64_t ldw2, float *d_G1, float *d_G2, int64_t ldG, float *d_P, float *d_db1,
                       float *d_db2, float *d_dA, float *d_R, float *d_dX, int64_t lddx, float *d_work, int64_t work_floats,
                       void *stream);

/* gnx_step_wide_ngcf (opt-in; added within ABI 0.9 -- probe for the symbol): the layer of gnx_ngcf_step at C_in = 128, the width of
 * the reference's library_recommendation demo, as the SpMM and ONE row-local launch.  The parameter list, the outputs and their
 * formats are gnx_ngcf_step's -- d_gate [n, 2 * ceil(C_out / 32)], the P1 words then the P2 words, zero bits beyond C_out; d_rnorm
 * negated (-1e6f) where the clamp acted; out written only below column C_out, whole 16-byte stores where ldo % 4 == 0 and out is
 * 16-byte aligned, single values otherwise -- so gnx_ngcf_back_gate and a composed backward read them unchanged.
 * Supported: C_in == 128, 1 <= C_out <= 128, ldx % 4 == 0, and X, d_agg and d_work 16-byte aligned.  Anything else returns
 * GNX_ERR_UNSUPPORTED naming the widths or the alignment, nothing launched: callers keep gnx_ngcf_step there.
 * Step A: gnx_spmm(X) into d_agg -- bit for bit gnx_spmm's result, hub rows included -- or, when d_agg is NULL, into the first
 * roundup4(n * C_in) floats of d_work:
 *     work_floats >= (d_agg ? 0 : roundup4(n * C_in))
 * Too little is refused and the message names the figure.
 * Step B: one launch over all n rows without a gather (hub rows need nothing of their own once A is in memory), a block of eight
 * waves per CU, persistent over 16-row tiles; W1 and W2 sit in LDS in f32 (16 KiB per 16 output columns, 128 KiB at C_out > 112),
 * zero-padded to a multiple of 16 columns there and nowhere else; a wave holds its rows of X and A as MFMA operand fragments in
 * registers.
 * Rounding points: A as in gnx_spmm; X * A one multiply; each P the f32 sum of v_mfma_f32_16x16x4_f32 over k ascending, then + bias;
 * the activation (leaky: one multiply by 0.2f where P <= 0); one add; the mask (x * scale); with normalize the row's sum of squares
 * over the columns below C_out -- lane cc of the row's 16 lanes holds the columns cc, 16 + cc, 32 + cc, ..: one fmaf chain over them
 * ascending from 0, then the 16 lanes added through xor-shuffles at strides 1, 2, 4, 8 --, r = 1 / sqrt(max(sum, 1e-12f)) with the
 * IEEE square root and division (each correctly rounded), and out = x * r.  (The lanes of a row hold other columns than in
 * gnx_ngcf_step, so the sum of squares associates differently: the two entries agree to float32 rounding, not bit for bit.)  The
 * order depends neither on n, nor on the grid, nor on the wave that takes a row; no float atomics: two calls give the same bits.
 * Checked before anything is launched (a refused call writes nothing): the NULL handle and the dropout rate, the widths and the
 * alignment (above), then the checks of gnx_ngcf_step, then work_floats.  Stream-ordered; under capture the long-row slab must
 * already cover C_in (gnx_graph_reserve), as for gnx_spmm.
 * Reports "spmm+k_ngcf_rows<128>" (+ "_drop" with a mask, + "_norm" with normalize).
 * (The layer's name stands behind the verb in this entry's name, as in gnx_step_back_ngcf.) */
int gnx_step_wide_ngcf(gnx_graph_t g, const float *d_vals, const float *d_X, int64_t ldx, int64_t C_in, const float *d_W1, int64_t ldw1,
                       const float *d_W2, int64_t ldw2, int64_t C_out, const float *d_b1, const float *d_b2, int act, double dropout_p,
                       uint64_t seed, uint64_t stream_id, int normalize, float *d_out, int64_t ldo, float *d_agg, uint32_t *d_gate,
                       float *d_rnorm, float *d_work, int64_t work_floats, void *stream);

/* gnx_step_back_wide_ngcf (training, opt-in; added within ABI 0.9 -- probe for the symbol): the backward of gnx_step_wide_ngcf /
 * gnx_ngcf_step at C_in = 128 around its two weight gradients.  The parameter list, the meanings and the output formats are
 * gnx_step_back_ngcf's: G1, G2 [n, C_out] at row stride ldG with zeros in the columns C_out .. roundup4(C_out) - 1; P, dA, R [n, C_in]
 * contiguous; db1, db2 [C_out]; dX (lddx); d_P, d_db1, d_db2 may each be NULL; d_dX == NULL: no products and no SpMM, and d_dA, d_R,
 * d_W1 and d_W2 may then be NULL and are not looked at.
 *   G1, G2 = gnx_ngcf_back_gate's        db1 = sum_rows G1       db2 = sum_rows G2       P = X * A
 *   Q1 = G1 . W1^T      Q2 = G2 . W2^T      dA = Q1 * X + Q2      R = Q1 * A      dX = A_hat^T . dA + R
 * Supported: C_in == 128, 1 <= C_out <= 128, ldx % 4 == 0, ldG % 4 == 0, ldG >= roundup4(C_out), and X / d_agg / G1 / G2 / P / dA / R
 * 16-byte aligned.  Anything else returns GNX_ERR_UNSUPPORTED naming the widths or the alignment, nothing launched and nothing
 * written: there is no composed form inside the entry, callers keep the composed backward there.
 * Three stream-ordered steps inside the call:
 * Step A: the gate pass, gnx_ngcf_back_gate's own kernel -- G1 / G2 are bit for bit its results -- and, where d_db1 or d_db2 is
 * given, the column sums of G1 / G2: slab s of d_work holds the sums of the rows s * per .. min((s + 1) * per, n) - 1, per =
 * ceil(n / slabs) -- within a slab 256 / (roundup4(C_out) / 4) row lanes add every that-many-th row in ascending order and are then
 * added in lane order --, and one finishing launch adds the slabs in index order.
 * Step B: one launch over all n rows without a gather, a block of eight waves per CU, persistent over 16-row tiles.  W1^T and W2^T
 * sit in LDS in f32, read from W1 / W2 [C_in, C_out] as stored (ldw1 / ldw2; no transposed copy exists), 16 KiB per 16 output
 * columns, 128 KiB at C_out > 112, zero from column C_out on; a wave holds its rows of G1 and G2 as MFMA operand fragments in
 * registers (the columns from roundup4(C_out) on are never loaded), forms Q1 and Q2 on v_mfma_f32_16x16x4_f32 and writes dA, R and --
 * where d_P is given -- P as whole 16-byte stores.  With d_dX == NULL the launch makes P alone (nothing where d_P is NULL too).
 * Step C, when d_dX is given: gnx_spmm_tv(d_dA, H0 = d_R, beta = 1, alpha = 1) into d_dX (lddx): d_vals_t the adjacency's values in
 * transposed order (NULL: the raw values); hub rows of the transposed structure are that launch's business.
 * Rounding points: G1 / G2 as gnx_ngcf_back_gate; P one multiply; each Q the f32 MFMA sum over the output columns ascending (four
 * columns a step); dA = fmaf(Q1, X, Q2), one rounding; R one multiply; db the fixed slab order above; dX as gnx_spmm_tv.  The order
 * depends on (n, C_out) alone -- not on the CU count, the grid or the wave that takes a tile; no float atomics: two calls give the
 * same bits.  (The composed backward rounds dA twice and its products associate otherwise: the two agree to float32 rounding.)
 * d_work / work_floats (only where d_db1 or d_db2 is given): with s = max(1, min(1024, ceil(n / 512))) slabs,
 *     work_floats >= s * 2 * C_out
 * Too little is refused and the message names the figure.
 * Checked before anything is launched (a refused call writes nothing): the NULL handle, the checks of gnx_ngcf_back_gate, the widths,
 * pointers and strides, a square stand-alone graph; every output -- G1, G2, P, db1, db2, dA, R, dX, d_work -- is a buffer of its own
 * (d_dX may NOT be d_R); the alignment; work_floats.
 * Stream-ordered and allocation-free once the handle is reserved; under capture the transposed structure and the long-row slab at
 * width 128 must exist already (gnx_graph_reserve with GNX_RESERVE_TRANSPOSED), as for gnx_spmm_tv.
 * Reports "k_ngcf_rows_back<128>" (+ "_drop" with a mask, + "+spmm_tv" when dX ran).
 * (The layer's name stands behind the verb in this entry's name, as in gnx_step_back_ngcf and gnx_step_wide_ngcf.) */
int gnx_step_back_wide_ngcf(gnx_graph_t g, const float *d_vals_t, const float *d_g, int64_t ldg, const float *d_y, int64_t ldy,
                            const float *d_rnorm, const uint32_t *d_gate, int64_t C_out, int act, double dropout_p, uint64_t seed,
                            uint64_t stream_id, const float *d_X, int64_t ldx, const float *d_agg, int64_t C_in, const float *d_W1,
                            int64_t ldw1, const float *d_W2, int64_t ldw2, float *d_G1, float *d_G2, int64_t ldG, float *d_P,
                            float *d_db1, float *d_db2, float *d_dA, float *d_R, float *d_dX, int64_t lddx, float *d_work,
                            int64_t work_floats, void *stream);

/* ---- the dense ends of the path (matrix cores) -----------------------------------------------------------------------
 * gnx_dense: out = act(X . W + bias) -- Dense.__forward__ (gnntf/core/nn/layers.py:135-136) and the transform of
 * GCNLayer (gcn.py:89).  X [n, F] (ldx), W [F, O] (ldw), bias [O] or NULL, out [n, O] (ldo); float32 in and out, float32
 * accumulate on v_mfma_f32_16x16x4_f32.  out must not alias X. */
int gnx_dense(const float *d_X, int64_t ldx, int64_t n, int64_t F, const float *d_W, int64_t ldw, int64_t O,
              const float *d_bias, int act, float *d_out, int64_t ldo, void *stream);

/* gnx_dense_wgrad: dW = X^T . G, the weight gradient of gnx_dense (what tf.GradientTape derives for layers.py:136,
 * trainable.py:70-78): X [n, F], G [n, O] (the gradient of the pre-activation), dW [F, O] contiguous.  float32 MFMA over row
 * slabs; d_work [work_floats] is scratch for the per-slab partial sums (>= F * O floats; more scratch = more slabs in flight,
 * 2048 * F * O is the most it uses); the slabs are added in a fixed order (reproducible). */
int gnx_dense_wgrad(const float *d_X, int64_t ldx, const float *d_G, int64_t ldg, int64_t n, int64_t F, int64_t O, float *d_dW,
                    float *d_work, int64_t work_floats, void *stream);

/* Feature dropout around the dense transform, made inside its launches (opt-in; added within ABI 0.9 -- probe for the symbols):
 * layers.py:135-136 behind a Dropout layer (filter.py:30-33), out = drop_out(act(drop_in(X) . W + bias)), without a dropped copy of X,
 * a mask in memory or a pass of its own.  Both masks are the one of gnx_feature_dropout (above): element (i, c) of a side with rate
 * 0 <= p < 1 and (seed, stream_id) is KEPT iff hash_u24(seed, stream_id + counter, i, c, 0) >= (uint32_t)(p * 2^24), i the row, c the
 * column of X (input side) or of the WHOLE result (output side: column panels past the first are keyed by their global column), counter
 * the handle's dropout counter; drop(v) = kept ? v * s : +0.0f, s = 1.0f / (1.0f - (float)p).  The handle is read for its dropout counter
 * only: any handle will do.  A rate of 0 on a side hashes nothing there; both 0 is gnx_dense itself.
 *
 * gnx_dense_drop: the argument list and checks of gnx_dense plus the handle and the two triples; no row maps.  Rounding points, per
 * element: x' = fl(x * s_in) for a kept x (+0 for a dropped one), made as a lane picks up its four consecutive floats of a row for the
 * matrix cores; the k-ascending fmaf chain of gnx_dense over x' (whichever kernel carries the shape: the same order, the same bits);
 * + bias; relu; then fl(v * s_out) for a kept v, +0 for a dropped one.  Bit for bit
 *   gnx_feature_dropout(in) -> gnx_dense -> gnx_feature_dropout(out, in place).
 *
 * gnx_dense_wgrad_drop: dW = drop_in(X)^T . G, the argument list and checks of gnx_dense_wgrad plus the handle and the input triple; the
 * mask is made again from the triple as the rows of X are picked up (x' = fl(x * s_in) or +0, as above), the slabs, their assignment and
 * the summation order are those of gnx_dense_wgrad: bit for bit that entry over a materialised drop_in(X). */
int gnx_dense_drop(gnx_graph_t g, const float *d_X, int64_t ldx, int64_t n, int64_t F, const float *d_W, int64_t ldw, int64_t O,
                   const float *d_bias, int act, double in_p, uint64_t in_seed, uint64_t in_stream, double out_p, uint64_t out_seed,
                   uint64_t out_stream, float *d_out, int64_t ldo, void *stream);
int gnx_dense_wgrad_drop(gnx_graph_t g, const float *d_X, int64_t ldx, const float *d_G, int64_t ldg, int64_t n, int64_t F, int64_t O,
                         double in_p, uint64_t in_seed, uint64_t in_stream, float *d_dW, float *d_work, int64_t work_floats, void *stream);

/* The task head, NodeClassification (gnntf/core/gnn/graph_predictor.py:16-31), fused over the listed nodes.  All three are
 * stream-ordered and allocation-free (no synchronisation: they sit in the per-epoch loop of small graphs); node ids / labels
 * out of range are never dereferenced -- such an item's loss is NaN (and so is the mean), its argmax -1, its gradient zero.
 * gnx_node_ce:      d_loss_per_node[i] = logsumexp(logits[nodes[i], :]) - logits[nodes[i], labels[i]] and their mean in
 *                   d_mean_loss[0] (= SparseCategoricalCrossentropy(from_logits) of log_softmax, graph_predictor.py:24-25).
 *                   d_loss_per_node must hold m + 256 floats (the tail is scratch of the fixed-order two-level mean).
 * gnx_node_ce_backward: d_grad_logits[nodes[i], :] += d_grad_loss[0] / m * (softmax(logits[nodes[i], :]) - onehot(labels[i]));
 *                   the caller zero-fills d_grad_logits [n_rows, C] first.
 * gnx_node_argmax:  d_out[i] = first index of the maximum of logits[nodes[i], :] (d_nodes NULL: row i); graph_predictor.py:17.
 *                   A NaN entry never wins: the maximum is taken over the other entries, and a row of only NaNs reports 0. */
int gnx_node_ce(const float *d_logits, int64_t ldl, int64_t n_rows, int64_t C, const int64_t *d_nodes,
                const int64_t *d_labels, int64_t m, float *d_loss_per_node, float *d_mean_loss, void *stream);
int gnx_node_ce_backward(const float *d_logits, int64_t ldl, int64_t n_rows, int64_t C, const int64_t *d_nodes,
                         const int64_t *d_labels, int64_t m, const float *d_grad_loss, float *d_grad_logits, int64_t ldg,
                         void *stream);
int gnx_node_argmax(const float *d_logits, int64_t ldl, int64_t n_rows, int64_t C, const int64_t *d_nodes, int64_t m,
                    int64_t *d_out, void *stream);

/* ---- vertex-partitioned propagation (multi-GPU; the reference has no counterpart -- SURVEY.md section 8(e)) ----------------
 * One process per GPU owns a contiguous block of rows.  Its feature buffer is
 *     X = [ region(0) .. region(self-1) | n_local local rows | region(self+1) .. region(n_ranks-1) ],
 * region(q) = [ rows of H PULLED from rank q | partial sums sum_j A_hat[i, j] H[j] PUSHED by q for rows i of this block ]
 * (the caller's plan decides which entries are pulled and which pushed; gnntf/sharded.py chooses a vertex cover of the cross
 * entries).  The main CSR of the block indexes X directly (gnx_graph_create_coo / _csr over n_buf columns; pushed partial sums
 * appear as weight-1 entries).  The SEND buffer is [ pulled rows for peer 0, 1, .. | pushed rows for peer 0, 1, .. ]:
 * the pulled half is a gather of local rows (d_send_pull_src: the LOCAL row of every pulled row, int32, in send order), the
 * pushed half the product of the PUSH graph [sum(send_push_rows) x n_local] with the local rows.  The two halves can be packed
 * and exchanged separately (GNX_HALO_PULL, GNX_HALO_PUSH): the pulled rows cost a short copy and can be on the links while the
 * partial sums -- most of the pack time -- are still being summed; GNX_HALO_ALL does both in one call / one RCCL group.
 *   gnx_halo_plan_create   per-peer row counts of both halves in both directions + the pulled-row list + the push graph (both
 *                          borrowed; NULL when the half is empty).  A rank may list itself as a peer (loop-back region after the
 *                          local rows): a one-rank communicator then carries a real send / receive pair (tests on one GPU)
 *   gnx_halo_plan_layout   n_buf, first local row, rows to send (total, pulled half), first row of every peer's region in X,
 *                          first row of every peer's slice of the pulled / of the pushed half of the send buffer (any NULL = skip)
 *   gnx_halo_pack          d_send (row length lds) <- the chosen half (or both) from the local rows of d_X; stream-ordered
 *   gnx_halo_exchange      one RCCL group: ncclRecv into the chosen half of every region of d_X + ncclSend of the matching slices
 *                          of d_send; d_X and d_send contiguous with row length C; `nccl_comm` is the caller's ncclComm_t whose
 *                          ranks are the plan's ranks.  GNX_ERR_UNSUPPORTED when no RCCL entry points are known: move the rows
 *                          yourself (any transport) using the offsets of gnx_halo_plan_layout
 *   gnx_halo_bind_rccl     hands over ncclGroupStart / ncclGroupEnd / ncclSend / ncclRecv of the library instance that created
 *                          the communicator (all NULL = unbind).  Without it the exchange looks the symbols up in the RCCL that
 *                          is ALREADY loaded in the process; it never loads a copy of its own
 * One iteration = gnx_halo_pack -> exchange -> gnx_spmm (or gnx_spmm_rows) over X into the local rows of the other buffer. */
enum { GNX_HALO_ALL = 0, GNX_HALO_PULL = 1, GNX_HALO_PUSH = 2 };
int gnx_halo_plan_create(int n_ranks, int self, int64_t n_local, const int64_t *recv_pull_rows, const int64_t *recv_push_rows,
                         const int64_t *send_pull_rows, const int64_t *send_push_rows, const int32_t *d_send_pull_src,
                         gnx_graph_t push_graph, gnx_halo_plan_t *out);
int gnx_halo_plan_destroy(gnx_halo_plan_t plan);
int gnx_halo_plan_layout(gnx_halo_plan_t plan, int64_t *n_buf, int64_t *local_row0, int64_t *n_send, int64_t *n_send_pull,
                         int64_t *recv_row0, int64_t *send_pull_row0, int64_t *send_push_row0);
int gnx_halo_pack(gnx_halo_plan_t plan, int part, const float *d_X, int64_t ldx, int64_t C, float *d_send, int64_t lds, void *stream);
int gnx_halo_exchange(gnx_halo_plan_t plan, int part, void *nccl_comm, const float *d_send, float *d_X, int64_t C, void *stream);
int gnx_halo_bind_rccl(void *nccl_group_start, void *nccl_group_end, void *nccl_send, void *nccl_recv);
/* ---- opt-in bf16 feature storage on a vertex block: the [regions | local rows | regions] buffers, the send buffer and every row
 * on the links as bf16 (uint16_t bit patterns; bf = the cast of gnx_cast_bf16, u = 2^-8).  The plan and its layout are those of the
 * f32 entries (rows, not bytes).  Rounding points of K >= 1 iterations on a block:
 *   - X~_0 = bf(H0) (or bf(start)) for this rank's rows, cast into the local rows of the first buffer (gnx_cast_bf16, strided dst);
 *   - a PULLED row is a copy of the owner's bf16 row: no rounding (gnx_halo_pack_bf16, pull half: a gather of 16 / 8 / 4 / 2-byte
 *     units, whatever the width, the leading dimensions and the alignment allow);
 *   - a PUSHED partial sum s_iq = sum_j A_hat[i,j] X~_k[j] (j over the sender q's columns) is summed in f32 by the sender and sent as
 *     bf(s_iq) (gnx_halo_pack_bf16, push half = gnx_spmm_bf16 over the push graph with out_bf16 = 1): one extra rounding per pushed
 *     row and iteration; the receiver adds the widened value with weight 1;
 *   - H_{k+1} = (1-a) acc + a H0 in f32 with f32 H0 (gnx_spmm_bf16 / gnx_spmm_rows_bf16 over the block's handles); for k < K-1 it
 *     leaves the launch as bf(H_{k+1}) into the local rows of the other buffer (out_bf16 = 1), the last iteration writes f32 H_K;
 *   - rows without entries follow the settled-row rule of gnx_appnp_propagate (GNX_ACT_SKIP_EMPTY from k >= 2, or at once when nobody
 *     references them; never on the last iteration).
 * All sums, H0, the mix and the result are f32; no float atomics: two runs give the same bits.  A plan WITHOUT pushed rows performs
 * exactly the roundings of gnx_appnp_propagate_bf16, row by row in the same summation order: bit for bit the one-GPU bf16 loop.
 * gnx_halo_pack_bf16 / gnx_halo_exchange_bf16: gnx_halo_pack / gnx_halo_exchange argument for argument over bf16 buffers (the
 * exchange uses ncclBfloat16; same grouping, receives before sends, same error paths); an empty plan packs as GNX_OK. */
int gnx_halo_pack_bf16(gnx_halo_plan_t plan, int part, const uint16_t *d_X, int64_t ldx, int64_t C, uint16_t *d_send, int64_t lds,
                       void *stream);
int gnx_halo_exchange_bf16(gnx_halo_plan_t plan, int part, void *nccl_comm, const uint16_t *d_send, uint16_t *d_X, int64_t C,
                           void *stream);
/* out[r,:] = X[idx[r],:] for int32 row ids (the pulled half of gnx_halo_pack as a call of its own); any width, grid-stride. */
int gnx_gather_rows32(const float *d_X, int64_t ldx, const int32_t *d_idx, int64_t n_idx, int64_t C, float *d_out, int64_t ldo,
                      void *stream);

/* The link head, LinkPrediction.predict / loss (gnntf/core/gnn/graph_predictor.py:122-126, 136-144): the logit of every listed
 * edge, d_out[i] = sum_c F[u_i, c] * F[v_i, c] * (d_r[c] or 1) -- gather of both endpoint rows + product + (DistMult) weights
 * + reduction in one launch; d_edges int64 [m, 2].  Stream-ordered, allocation-free; an edge with an endpoint out of range
 * gets NaN (nothing is dereferenced) and no gradient.
 * gnx_edge_scores_backward: d_grad_F[u_i, :] += g_i * F[v_i, :] * r and the mirror for v_i (caller zero-fills d_grad_F). */
int gnx_edge_scores(const float *d_F, int64_t ldf, int64_t n_rows, int64_t C, const int64_t *d_edges, int64_t m,
                    const float *d_r, float *d_out, void *stream);
int gnx_edge_scores_backward(const float *d_F, int64_t ldf, int64_t n_rows, int64_t C, const int64_t *d_edges, int64_t m,
                             const float *d_r, const float *d_grad_out, float *d_grad_F, int64_t ldg, void *stream);

/* The edge sampler of the link task, negative_sampling.__call__ (gnntf/core/gnn/graph_predictor.py:52-98), as one launch: d_edges
 * int64 [m (1 + samples), 2] receives, per positive pair (u_i, v_i) of d_positive [m, 2], the pair itself and then `samples` rows
 * (u_i, w) -- the reference's layout.  One thread per slot e = i * samples + s.  Try t = 0, 1, ... of a slot draws
 *   hi = hash_u24(seed, stream_id + counter, e, 2 t, 0), lo = hash_u24(seed, stream_id + counter, e, 2 t + 1, 0)   (the counter RNG of
 *   the dropout masks, oracle/gnntf_oracle.py:hash_u24; counter = the handle's gnx_graph_set_dropout_counter value, 0 without one: a
 *   replayed hipGraph draws fresh negatives), x = hi 2^24 + lo, j = floor(x K / 2^48), w = d_candidates ? d_candidates[j] : j
 * and the first w is taken with w != u, w != v and neither (u, w) nor (w, u) a stored entry of the handle's coalesced pattern (binary
 * search in rows u and w; values are not read; a w outside [0, n_rows) has no stored entry).  After max_tries rejected tries the slot
 * keeps the LAST w drawn and *d_fallbacks is incremented (an integer atomic: order-free) -- the loop is bounded.  A positive row with an
 * endpoint outside [0, n_rows) is copied as it is and its negatives are (u, -1), which gnx_edge_scores answers with NaN.  d_candidates
 * int64 [K], or NULL: every row id, K == n_rows.  Refused: K < 1, K >= 2^31, samples < 1, max_tries < 1, m < 0, m * samples >= 2^31,
 * NULL pointers.  m == 0 writes nothing.  Stream-ordered, allocation-free. */
int gnx_sample_negatives(gnx_graph_t g, const int64_t *d_positive, int64_t m, int64_t samples, const int64_t *d_candidates, int64_t K,
                         int64_t max_tries, uint64_t seed, uint64_t stream_id, int64_t *d_edges, unsigned long long *d_fallbacks,
                         void *stream);

/* The link head's backward (graph_predictor.py:122-146 under the gradient tape) in a FIXED summation order: no float atomics, so a
 * training step repeats bit for bit.
 * gnx_edge_plan: position q = 2 i + side of the flattened list d_edges [m, 2] names node edges[q]; its other endpoint is edges[q ^ 1].
 *   d_keys uint32 [2 m], d_pos int32 [2 m] receive the STABLE ascending sort of the positions by named node (positions ascend inside a
 *   node); both positions of an edge with an endpoint outside [0, n_rows) are keyed n_rows and form a trailing bucket that the backward
 *   skips.  d_chunks int32 [2 m + 1]: d_chunks[0] = the number of chunks, then the sorted index at which every chunk begins, ascending
 *   -- a node's run of sorted indices is cut into chunks of 256 counted from the run's first index.  d_workspace: gnx_edge_plan_bytes(m)
 *   bytes (-1: failed), 16-byte aligned, the caller's; the sort and the compaction run in it (rocPRIM), so the call allocates nothing,
 *   waits for nothing and records into a hipGraph.  m < 2^30, n_rows < 2^31; m == 0 writes d_chunks[0] = 0 alone.
 * gnx_edge_scores_backward_sorted: the operands and the += contract of gnx_edge_scores_backward, the plan of the SAME list and n_rows,
 *   and d_work of gnx_edge_sorted_work_floats(m, C) floats.  The sum of a row is part of the interface:
 *     term of position q, i = q >> 1:  t_q[c] = fl(w_i[c] * F[edges[q ^ 1], c]),  w_i[c] = fl(g_i * r[c]), or g_i without d_r;
 *     a chunk's sum is sequential in ascending sorted index: s = t_first, s = fl(s + t_next), ...;
 *     a node of one chunk:  dF[x, c] = fl(dF[x, c] + s);  a node of several: S = s_0, S = fl(S + s_1), ... in chunk order (the chunk
 *     sums pass through d_work), then dF[x, c] = fl(dF[x, c] + S).
 *   Every named row of d_grad_F is read and written once, by one owner; rows that no position names and the columns from C on keep their
 *   bits.  A self-loop contributes both its positions to its node.  One lane group per chunk, lanes own columns; F rows are read with
 *   16-byte loads where C % 4 == 0, ldf % 4 == 0 and d_F is 16-byte aligned. */
int64_t gnx_edge_plan_bytes(int64_t m);
int gnx_edge_plan(const int64_t *d_edges, int64_t m, int64_t n_rows, uint32_t *d_keys, int32_t *d_pos, int32_t *d_chunks,
                  void *d_workspace, int64_t bytes, void *stream);
int64_t gnx_edge_sorted_work_floats(int64_t m, int64_t C);
int gnx_edge_scores_backward_sorted(const float *d_F, int64_t ldf, int64_t n_rows, int64_t C, const int64_t *d_edges, int64_t m,
                                    const float *d_r, const float *d_grad_out, float *d_grad_F, int64_t ldg, const uint32_t *d_keys,
                                    const int32_t *d_pos, const int32_t *d_chunks, float *d_work, int64_t work_floats, void *stream);

/* The ranking evaluation of the link task, MeanLinkPrediction.evaluate (gnntf/core/gnn/graph_predictor.py:154-203), for all source
 * nodes at once (added within ABI 0.9 -- probe for the symbols).  The list of source s = d_sources[i] is its held-out neighbours
 * d_pos_ids[d_pos_ptr[i] .. d_pos_ptr[i + 1]) in the order given (the positives), followed by the strangers: every candidate v of
 * d_candidates [K] (int64, STRICTLY ASCENDING) inside [0, n_rows_F) with v != s and neither (s, v) nor (v, s) a stored entry of the
 * handle's coalesced pattern (values are not read; an id at or beyond the handle's rows is linked to nothing).  A held-out neighbour
 * that is also a non-linked candidate is in the list twice, as in the reference.  A candidate outside [0, n_rows_F) is skipped.
 *   score(s, v) = sum_c fl(F[s, c] * r[c]) * F[v, c]  (d_r NULL: F[s, c] * F[v, c]), accumulated in f32 on v_mfma_f32_16x16x4_f32 in
 *   ascending groups of 16 columns; the score of a pair is the same bits wherever the call needs it.  d_F: f32 rows of any C >= 1 and
 *   any pitch ldf >= C (16-byte loads where ldf % 4 == 0 and d_F is 16-byte aligned); nothing from column C on is read.  FINITE
 *   embeddings and weights are a precondition: the order of NaN scores is not defined.
 * Outputs per source i, the caller's:
 *   d_n_pos[i]    the length of its held-out list;
 *   d_n_neg[i]    the number of strangers, or -1: the source, one of its held-out ids or its d_pos_ptr range is out of range -- then
 *                 less = equal = 0 and the top-k row is padding;
 *   d_less[i], d_equal[i]   summed over the positives p, the strangers whose score is < resp. == the score of p (-0 == +0): the
 *                 rank-statistic AUC is exactly (less + equal / 2) / (n_pos * n_neg);
 *   d_top_ids [S, k] int64, d_top_scores [S, k] f32, d_top_is_pos [S, k] uint8: the k first entries of the list in this TOTAL order --
 *                 a higher score comes first; among equal scores the entry LATER in the list comes first (what
 *                 np.argsort(scores, kind="stable")[-k:] selects, reversed): a stranger beats a positive, and among strangers the larger
 *                 candidate id wins.  Where the list is shorter than k: id -1, score -inf, is_pos 0.  1 <= k <= GNX_RANK_MAX_K.
 *   d_scores [S, K] f32, or NULL: the raw score of every (source, candidate) pair whose ids are in range, excluded or not; other
 *                 cells keep their bits.
 * The order is total and the counts are integers (integer atomics only, no float atomics), so no output depends on `splits` or on the
 * schedule.  splits: 0 = the library cuts the candidate tiles into as many parts as fill the device; n > 0 = into n parts (at most
 * GNX_RANK_MAX_SPLITS, never more than there are tiles of 64 candidates).  Positive scores beyond the first GNX_RANK_POS_PASS of a
 * source are compared from memory instead of LDS.  d_workspace: gnx_rank_candidates_bytes(S, P, K, k, splits) bytes (-1: refused),
 * 16-byte aligned.  The counts are taken over every candidate and corrected over the excluded pairs, which are found from the rows of
 * the source in the handle and in its TRANSPOSED structure: that is built on the first call (gnx_graph_reserve(GNX_RESERVE_TRANSPOSED)
 * before a capture); otherwise the call allocates nothing, waits for nothing and records into a hipGraph.  S == 0 does nothing.
 * Refused: S, P, K outside [0, 2^31), k outside [1, GNX_RANK_MAX_K], splits outside [0, GNX_RANK_MAX_SPLITS], C < 1, ldf < C, NULL
 * handle / operands / outputs, a short or misaligned workspace. */
#define GNX_RANK_MAX_K 32
#define GNX_RANK_POS_PASS 32
#define GNX_RANK_MAX_SPLITS 256
int64_t gnx_rank_candidates_bytes(int64_t S, int64_t P, int64_t K, int64_t k, int64_t splits);
int gnx_rank_candidates(gnx_graph_t g, const float *d_F, int64_t ldf, int64_t n_rows_F, int64_t C, const float *d_r,
                        const int64_t *d_sources, int64_t S, const int64_t *d_pos_ptr, const int64_t *d_pos_ids, int64_t P,
                        const int64_t *d_candidates, int64_t K, int64_t k, int64_t splits, int64_t *d_n_pos, int64_t *d_n_neg,
                        int64_t *d_less, int64_t *d_equal, int64_t *d_top_ids, float *d_top_scores, uint8_t *d_top_is_pos, float *d_scores,
                        void *d_workspace, int64_t bytes, void *stream);

/* ---- node signals at width 1 (added within ABI 0.9 -- probe for the symbols) -------------------------------------------------
 * One scalar per node: what PPRSweep and FastReg (gnntf/core/gnn/architectures/experimental_filter.py:7-43) compute.  The gather
 * deals a row's ENTRIES to the lanes of a group (the SpMM kernels deal its columns, of which there is one here): every lane runs its
 * own fmaf chain in entry order, the group's sums are added in a fixed xor tree; rows longer than the structure's long-row threshold
 * go one wave per chunk, the chunk sums added in chunk order.  No float atomics: every result is a function of the structure and the
 * operands alone, two calls give the same bits, a row without entries sums to +0.  All entries are stream-ordered and read no value
 * back; they allocate only what gnx_graph_reserve(g, 1, GNX_RESERVE_TRANSPOSED) builds ahead of a capture.
 * gnx_signal_project: d_out[i] = act(sum_c d_X[i * ldx + c] * d_w[c]), i < n; act = 1: 1 / (1 + expf(-z)) with the accurate expf
 *   (z = +-100 gives exactly 1 / 0, never NaN), act = 0: the dot product z.  Any C >= 1, ldx >= C; 16-byte loads where every row start
 *   allows.  Each lane adds its columns in ascending order, then a fixed xor tree.
 * gnx_signal_spmv: d_out[i] = beta * (sum_j A[i,j] d_x[j]) + alpha * h0[i] over the matrix (transposed == 0: d_x [n_cols], d_out and
 *   d_h0 [n_rows]) or its transpose (the other way round).  d_vals in the order of the structure WALKED (transposed: what
 *   gnx_graph_permute_values_t / gnx_graph_normalize_t write), NULL = the raw values.  d_h0 == NULL is the constant 1, bit for bit a
 *   vector of ones.  d_out must not be d_x.
 * gnx_signal_ppr: K steps x <- (1-a) A x + a h0 from x = h0 (NULL: the constant 1), ping-ponging through d_work [n] so that the last
 *   lands in d_out; bit for bit K calls of gnx_signal_spmv with beta = float(1 - a), alpha = a.  K = 0 copies h0.  Square graph; d_work
 *   is needed for K >= 2, and for K = 1 when d_h0 is NULL.
 * gnx_signal_smoothness: the forward of lambda = sum_i d_i^2 / sum_i D_i f_i^2, d = f - A f (experimental_filter.py:34-43 with
 *   f = the projected signal, D = d_colsum): writes d to d_diff_out [n] and {num, den, num / den} to d_sums_out [3] -- a plain IEEE
 *   division, so den == 0 gives what IEEE gives.  Blocks of 256 rows of the structure's row order leave their partial sums in d_work
 *   (at least n / 64 + 64 floats), a second launch adds them in index order (64 slabs per block, in levels beyond 2^14 rows).  Square graph.
 * gnx_signal_smoothness_back: gz_i = u * (2 / den) * ((d_i - (A^T d)_i) - lambda * D_i * f_i) * f_i * (1 - f_i): the gradient of
 *   u * lambda with respect to the pre-sigmoid projection, one walk of the transposed structure.  d_vals_t in transposed order (NULL:
 *   the raw values); d_sums as gnx_signal_smoothness left it; u = d_upstream[0], read on the device.
 * gnx_signal_uniform: d_out[i] = bound * u_i, i < n, u_i = (hash_u24(seed, stream_id, i, 0, 0) - 2^23) / 2^23: uniform on a 2^-23
 *   grid of [-1, 1), from the counter RNG of the edge dropout (the handle's dropout counter is added to stream_id): the fresh
 *   projection vector FastReg draws per forward, reproducible from (seed, stream) and replayable inside a hipGraph.
 * gnx_graph_last_kernel reports "signal_spmv_group8", "signal_smooth_group8", "signal_back_group8", with "+long" appended when hub
 * rows went through the chunk launch.  Refused (GNX_ERR_INVALID, "<entry>: ..."): a NULL handle or buffer, C < 1, ldx < C, K < 0, a
 * non-square graph where one is needed, an output that aliases an operand. */
int gnx_signal_project(const float *d_X, int64_t ldx, int64_t n, int64_t C, const float *d_w, int act, float *d_out, void *stream);
int gnx_signal_spmv(gnx_graph_t g, const float *d_vals, int transposed, const float *d_x, const float *d_h0, float beta, float alpha,
                    float *d_out, void *stream);
int gnx_signal_ppr(gnx_graph_t g, const float *d_vals, const float *d_h0, float a, int K, float *d_out, float *d_work, void *stream);
int gnx_signal_smoothness(gnx_graph_t g, const float *d_vals, const float *d_f, const float *d_colsum, float *d_diff_out,
                          float *d_sums_out, float *d_work, void *stream);
int gnx_signal_smoothness_back(gnx_graph_t g, const float *d_vals_t, const float *d_f, const float *d_diff, const float *d_colsum,
                               const float *d_sums, const float *d_upstream, float *d_gz_out, void *stream);
int gnx_signal_uniform(gnx_graph_t g, int64_t n, float bound, uint64_t seed, uint64_t stream_id, float *d_out, void *stream);

/* Halo packing for the vertex-partitioned path: out[r,:] = X[idx[r],:], idx int64 [n_idx]. */
int gnx_gather_rows(const float *d_X, int64_t ldx, const int64_t *d_idx, int64_t n_idx, int64_t C,
                    float *d_out, int64_t ldo, void *stream);

/* gnx_linear_combination: d_out[i] = sum_j coef[j] * d_src[j][i] over k <= 16 device arrays of n floats (d_src and coef are HOST
 * arrays of k entries; terms are added in index order; d_out may be one of the sources).  Ends the backward of the K-iteration
 * loop -- dH0 = g_0 + a (g_1 + ... + g_K), the adjoint of filter.py:20-21's "+ a * H0" in every iteration -- in one pass. */
int gnx_linear_combination(int k, const float *const *d_src, const float *coef, int64_t n, float *d_out, void *stream);

/* Measurement aid: a float4 streaming copy d_dst[0..n) = d_src[0..n) (n a multiple of 4, 16-byte aligned pointers).
 * bench.py times it next to the propagation as the measured-peak HBM rate (read + write bytes per second). */
int gnx_stream_copy(const float *d_src, float *d_dst, int64_t n_floats, void *stream);
/* The read-only yardstick: streams d_src[0..n) once and folds it into d_sink64 [64 floats] (accumulated, not cleared). */
int gnx_stream_read(const float *d_src, int64_t n_floats, float *d_sink64, void *stream);
/* Measurement aid: launches n_blocks workgroups and writes, per workgroup, the id of the XCD it ran on (HW_REG_XCC_ID, 0..7) to
 * d_xcd_out [n_blocks].  The row-window launch order (gnx_graph_set_row_window) ASSUMES, for speed only, that the dispatcher deals
 * workgroups round-robin over the eight XCDs (blocks b and b + 8 share one); tests record here whether the box at hand does. */
int gnx_probe_block_xcd(int64_t n_blocks, int32_t *d_xcd_out, void *stream);

/* Name of the SpMM kernel the last gnx_spmm/_t call on this handle dispatched (static
 * string; for profiles and tests): "spmm_wave", "spmm_group8" ... "spmm_group32" (lanes per row; "spmm_group4+chunks": the merged small-graph launch), "..._drop" (weights made
 * in the kernel), "...+chunks" (structures below 2^20 rows: the chunks of the long rows share the launch of the short rows),
 * "spmm_gcnii_mfma", "spmm+dense_mfma"; the bf16 entries report "spmm_wave_bf16", "spmm_group8_bf16" ... "spmm_group32_bf16",
 * "...+long_bf16" (hub rows through the chunk kernels) and "...+chunks_bf16" (gnx_spmm_rows_bf16 and the push half of
 * gnx_halo_pack_bf16 -- on the push graph's handle -- report these same names: no new suffix); the bf16 training entries report the f32 training
 * names with "_bf16" appended ("spmm_group16_drop_bf16", "spmm_wave_drop_entries_bf16", ...), "+long" after the row class when hub
 * rows went through the chunk kernels ("spmm_group8+long_drop_bf16"); gnx_gcnii_step_bf16 reports "spmm_gcnii_mfma_bf16" (the fused
 * launch, with or without hub rows) or "spmm+dense_mfma_bf16" (the other widths / alignments); gnx_gcnii_step_back reports
 * "spmm_gcnii_back_mfma" (the fused launch, with or without hub rows) or "dense+spmm_back" (the other widths / alignments);
 * gnx_gcnii_step_drop reports "spmm_gcnii_mfma_drop" or "spmm+dense_mfma_drop" likewise (with p == 0 the names of gnx_gcnii_step); the
 * two dropout passes report nothing; gnx_gcnii_step_train_bf16 reports "spmm_gcnii_mfma_train_bf16" and gnx_gcnii_step_back_bf16
 * "spmm_gcnii_back_mfma_bf16" (the fused launches, with or without hub rows: those two entries have no other form), and so do
 * gnx_gcnii_step_drop_bf16 ("spmm_gcnii_mfma_drop_bf16"), gnx_gcnii_wgrad ("gcnii_wgrad_mfma") and gnx_gcnii_wgrad_bf16
 * ("gcnii_wgrad_mfma_bf16"); gnx_gcnii_step_spectral reports "spmm_gcnii_spectral_mfma" / "spmm_gcnii_spectral_mfma_drop" or
 * "spmm+dense_mfma_spectral" / "spmm+dense_mfma_spectral_drop" (the other widths / alignments). */
const char *gnx_graph_last_kernel(gnx_graph_t g);

#ifdef __cplusplus
}
#endif
#endif /* GNX_H */
