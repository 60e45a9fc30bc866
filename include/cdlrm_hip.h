/*
 * libcdlrm_hip.so -- C ABI of the MI355X (gfx950) look-ahead embedding-cache training path.
 *
 * The reference (lkp411/cDLRM) is pure Python over stock ATen ops: it has NO FFI / plugin interface
 * for this path.  This header is therefore the build's own thin lower boundary; every
 * entry point names the reference call site (file:line in the reference tree) whose work it takes
 * over.  The upper boundary (same names / argument meaning as the reference) is the Python package
 * cdlrm_amd/{model_no_ddp,cache_manager,main_no_ddp}.py, which binds this library through ctypes
 * (INTEGRATION.md shows the stub a reference maintainer would add).
 *
 * Conventions
 *   - every function returns 0 on success, a positive hipError_t, or a negative CDLRM_E* code;
 *     nothing throws across the ABI; cdlrm_last_error() returns a thread-local message.
 *   - all tensor memory is CALLER-owned (torch tensors' data_ptr()); the library allocates only the
 *     opaque context (descriptor copies, small scan scratch, one device error word).
 *   - `stream` is a hipStream_t passed as void* (torch.cuda.current_stream().cuda_stream); calls are
 *     asynchronous on it unless the name ends in _sync.
 *   - "device-visible" pointers may point to HBM or to pinned / registered host memory.
 *   - slot ids follow the reference: slot = P_k * way + set, aux slots start at P_k * ways
 *     (model_no_ddp.py:174, 177); tags are int64 [P_k, ways] row-major, -1 = empty (:144-147).
 */
#ifndef CDLRM_HIP_H
#define CDLRM_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CDLRM_ABI_VERSION 1

#define CDLRM_EINVAL (-22)   /* bad argument / shape the kernels do not support            */
#define CDLRM_ERANGE (-34)   /* an index was outside its table, or a capacity was exceeded */
#define CDLRM_ENOMEM (-12)

typedef struct cdlrm_ctx cdlrm_ctx;

/* Geometry of one cache group (Embedding_Table_Cache_Group.__init__, model_no_ddp.py:101-147). */
typedef struct {
    int32_t num_tables;          /* T                                                     */
    int32_t dim;                 /* D, fp32 elements per row (multiple of 4)               */
    int32_t num_ways;            /* 1..64                                                  */
    int32_t aux_rows;            /* aux_table_size (main_no_ddp.py:348)                    */
    const int64_t* table_rows;   /* [T] n_k  rows of the host master table                 */
    const int64_t* cache_sets;   /* [T] P_k = min(n_k, find_next_prime(cache_size))        */
    int32_t device;              /* HIP device ordinal                                     */
    int32_t aux_phases;          /* 0/1: one aux region per table; 2: two (aux rows double-  */
                                 /* buffered: the NEXT batch's misses are filled while the    */
                                 /* current batch still trains on its own aux rows)           */
} cdlrm_geometry;

int cdlrm_abi_version(void);
/* DEVELOPMENT EXPORT, not part of the drop-in surface (no reference counterpart; a maintainer binds nothing to it): key 0 .. 7
 * selects a kernel variant the current one replaced, or a grid size, so that two builds' worth of behaviour can be timed against
 * each other on one box in one process (tools/ab_step.py --attr debug:<key>, bench.py --debug, which prints what it set in
 * config.debug).  All zero unless a tool sets them.  No key skips work in the shipped library (the two timing experiments that
 * do -- key 6, bits 1 and 2 -- are compiled in by -DCDLRM_DEV only and refused here otherwise); variants are bit-identical
 * except the GEMM kernel selectors of key 6, whose kernels differ in contraction order (equal to fp32 rounding); grid sizes
 * only change placement.  cdlrm_debug_set(7, 2): the weight gradients of a long-batch cdlrm_mlp_wgrad* call as one launch
 * per layer instead of the grouped launch (bit-identical).  The list of keys: csrc/common.h. */
int cdlrm_debug_set(int32_t key, int32_t value);
const char* cdlrm_last_error(void);

int cdlrm_ctx_create(const cdlrm_geometry* geo, cdlrm_ctx** out);
int cdlrm_ctx_destroy(cdlrm_ctx* ctx);

/* Bind the caller-owned cache state.  tags: int64 [sum_k P_k*ways] (table k at element offset
 * sum_{j<k} P_j*ways); weight: fp32 [sum_k rows_k, D], rows_k = ways*P_k + aux*max(1, aux_phases) (table k at row
 * sum_{j<k} rows_j; its first ways*P_k + aux rows are the reference's cache table).
 * Replaces the per-table nn.EmbeddingBag weights + CPU occupancy tables of model_no_ddp.py:130-147. */
int cdlrm_ctx_bind_cache(cdlrm_ctx* ctx, int64_t* tags, float* weight);

/* Bind the host master tables (Embedding_Table_Group.emb_l[k].weight, model_no_ddp.py:61-74):
 * host_rows[k] is a device-visible pointer to fp32 [n_k, D] (pinned/registered host memory, or HBM). */
int cdlrm_ctx_bind_host_tables(cdlrm_ctx* ctx, float* const* host_rows);

/* Pin an existing host allocation so kernels can read/write it over PCIe; returns its device alias. */
int cdlrm_host_register(void* host_ptr, uint64_t bytes, void** device_alias);
int cdlrm_host_unregister(void* host_ptr);

/* Read (and clear) the device error word set by kernels on out-of-range input (CDLRM_ERANGE). */
int cdlrm_ctx_check_sync(cdlrm_ctx* ctx, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Per-iteration path: Embedding_Table_Cache_Group.forward (model_no_ddp.py:149-212)
 * ------------------------------------------------------------------------------------------- */

/* Tag probe + slot translation + aux-row fill (model_no_ddp.py:163-187).
 *   idx        device int64 [T, n] (row stride ld_idx): the lookups of every table
 *   slots_out  device int32 [T, n] contiguous: cache_group_idxs (model_no_ddp.py:204); misses get
 *              aux slots P_k*ways + i in position order and aux row i is overwritten with the host
 *              row (:176-179).
 *   miss_pos   device int32 [T, n]: positions of table k's misses in order, first miss_count[k]
 *              entries of row k valid (victim_cache_entries, model_no_ddp.py:187)
 *   miss_count device int32 [T]: number of misses per table.
 *   aux_phase  which aux region receives the misses (0 unless the geometry has aux_phases = 2): aux slots are
 *              then P_k*ways + aux_phase*aux + i.                                                  */
int cdlrm_embbag_probe(cdlrm_ctx* ctx, const int64_t* idx, int64_t n, int64_t ld_idx,
                       int32_t* slots_out, int32_t* miss_pos, int32_t* miss_count, int32_t aux_phase,
                       void* stream);

/* Window-resident form of the same (round 2).  Tags only change at a refill (main_no_ddp.py:393-399), so the tag match
 * of model_no_ddp.py:163-174, the ordered miss numbering (:176-177) and the lookup of a miss in the window's victim list
 * need to run ONCE per look-ahead window, not once per iteration:
 *   cdlrm_window_resolve   idx [T, n] = the lookups of n/batch_len consecutive GLOBAL batches of batch_len lookups each;
 *                          every batch is cut into segments of seg_len lookups (= one rank's slice, ceil(B/world): the
 *                          last segment of a batch is shorter when world does not divide B, main_no_ddp.py:344, 388-391) and
 *                          the numbering restarts at every segment AND every batch boundary.  batch_len = 0: one run of
 *                          seg_len-long segments.  wslots int32 [T, n]: the slot of every lookup, misses numbered per segment in position
 *                          order as P_k*ways + i (aux phase 0); wsrc int32 [T, n]: for a miss, the position of its row in
 *                          the bound victim rows (cdlrm_ctx_bind_victims), -1 = read the host table; undefined for hits.
 *                          Call after the window's cdlrm_plan_commit + cdlrm_ctx_bind_victims.
 *   cdlrm_embbag_take      per iteration: slots_out int32 [T, n] = the batch's columns of wslots (misses moved to aux
 *                          region aux_phase) and the misses' rows copied into their aux rows -- exactly what
 *                          cdlrm_embbag_probe leaves behind for that batch.  wslots / wsrc / idx point at the batch's
 *                          first column; ld_w / ld_idx are the row strides. */
int cdlrm_window_resolve(cdlrm_ctx* ctx, const int64_t* idx, int64_t n, int64_t ld_idx, int64_t batch_len, int64_t seg_len,
                         int32_t* wslots, int32_t* wsrc, void* stream);
int cdlrm_embbag_take(cdlrm_ctx* ctx, const int64_t* idx, int64_t n, int64_t ld_idx, const int32_t* wslots,
                      const int32_t* wsrc, int64_t ld_w, int32_t* slots_out, int32_t aux_phase, void* stream);

/* --evict-victim-cache (main_no_ddp.py:96; victim_cache_entries, model_no_ddp.py:187 -- parsed / recorded by the reference
 * and never used: the update a MISSED row received is lost there).  Behind the step's embedding update: the trained aux row
 * of every miss of the batch is written to its host row and to its copy among the bound window victim rows; of several
 * misses of one index in the batch the LAST (position order) is written -- `emb_tables[k].weight[missing] = cache[k].weight[aux]`.
 *   idx [T, n] / slots [T, n] the batch's lookups and their slot ids as cdlrm_embbag_probe / _take left them (aux_phase: the
 *   aux region they used); wsrc [T, n] (row stride ld_w) the resolver's victim positions or NULL (the victim list is searched);
 *   work: device scratch of cdlrm_victim_writeback_work_bytes(T, n) bytes, 256-byte aligned. */
uint64_t cdlrm_victim_writeback_work_bytes(int32_t T, int64_t n);
int cdlrm_victim_writeback(cdlrm_ctx* ctx, const int64_t* idx, int64_t n, int64_t ld_idx, const int32_t* slots,
                           const int32_t* wsrc, int64_t ld_w, int32_t aux_phase, void* work, void* stream);

/* Fused multi-table sum-pool gather: nn.EmbeddingBag(mode="sum") forward on the cache rows for all
 * T tables in one launch (model_no_ddp.py:200-203).
 *   slots    device int32 [T, n]
 *   offsets  device int64 [T, n_bags] bag starts (row stride ld_off), or NULL for the Criteo layout
 *            offsets == arange (one index per bag, n_bags == n; data_loader_terabyte.py:83-87)
 *   out      device fp32: out[(b * ld_bag) + (t * ld_table) + c], c < D.  ld_bag = (T+1)*D and
 *            ld_table = D with out pointing at feature 1 writes straight into the [B, T+1, D]
 *            interaction operand (model_no_ddp.py:276).                                         */
int cdlrm_embbag_fwd(cdlrm_ctx* ctx, const int32_t* slots, const int64_t* offsets, int64_t n,
                     int64_t n_bags, int64_t ld_off, float* out, int64_t ld_bag, int64_t ld_table,
                     void* stream);

/* EmbeddingBag backward + sparse SGD on the cache rows, fused and atomics-free
 * (main_no_ddp.py:376, 409, 413): W[slot] -= lr * sum_{i: slot_i = slot} grad[bag(i)], repeated
 * slots summed in position order.  Also marks the touched rows for the table-agg merge.
 *   grad     device fp32, same addressing as `out` above (ld_bag / ld_table)
 *   work     device scratch, cdlrm_embbag_bwd_work_bytes(T, n) bytes
 *   touched  device uint8 [total cache rows] or NULL: set to 1 for every updated row of the cache proper (aux rows --
 *            transient copies of host rows, rewritten by every forward -- are never flagged)
 *            (replaces cache_group_idxs_window, main_no_ddp.py:417-423)                          */
uint64_t cdlrm_embbag_bwd_work_bytes(int32_t num_tables, int64_t n, int32_t dim);
/* The same in two halves: `prepare` (sort of the slot ids + run metadata into `work`) depends only on
 * the probe result, so a trainer issues it during the forward pass; `apply` consumes the gradient.
 * Every `apply` follows a `prepare` on the SAME work buffer, in stream order (prepare also empties the buffer's long-run list);
 * backward passes on different work buffers share no state and may be in flight together. */
int cdlrm_embbag_bwd_prepare(cdlrm_ctx* ctx, const int32_t* slots, int64_t n, void* work, void* stream);
int cdlrm_embbag_bwd_apply(cdlrm_ctx* ctx, const int64_t* offsets, int64_t n, int64_t n_bags,
                           int64_t ld_off, const float* grad, int64_t ld_bag, int64_t ld_table, float lr,
                           void* work, uint8_t* touched, void* stream);
int cdlrm_embbag_bwd_sgd(cdlrm_ctx* ctx, const int32_t* slots, const int64_t* offsets, int64_t n,
                         int64_t n_bags, int64_t ld_off, const float* grad, int64_t ld_bag,
                         int64_t ld_table, float lr, void* work, uint8_t* touched, void* stream);
/* `apply` behind cdlrm_gather_interact_bwd_sgd (below): the rows of slots that the batch reads ONCE were updated by that launch
 * and their gradient rows never written; this call sums and applies the runs of two and more lookups (and sets the touched
 * flags of all of them).  Same arguments as cdlrm_embbag_bwd_apply; together the two calls leave the cache rows bit for bit as
 * cdlrm_gather_interact_bwd + cdlrm_embbag_bwd_apply do (nn.EmbeddingBag backward + optim.SGD, main_no_ddp.py:376, 409, 413). */
int cdlrm_embbag_bwd_apply_rest(cdlrm_ctx* ctx, const int64_t* offsets, int64_t n, int64_t n_bags,
                                int64_t ld_off, const float* grad, int64_t ld_bag, int64_t ld_table, float lr,
                                void* work, uint8_t* touched, void* stream);
/* The once-only flags `prepare` left in `work`: uint8 [T, n], 1 where the lookup's slot occurs once in the batch (host-side
 * pointer arithmetic, no launch). */
int cdlrm_embbag_bwd_once_flags(cdlrm_ctx* ctx, void* work, int64_t n, const uint8_t** once);
/* The slot sort of a whole look-ahead CHUNK at once (round 6).  Slot ids of a window do not change while it trains
 * (cdlrm_window_resolve), so the `prepare` of its batches need not wait for their steps: nb batches x T tables are sorted by
 * one set of launches, on the resolver's stream, into the caller-owned `sorted` (cdlrm_embbag_bwd_sorted_bytes; 256-byte
 * aligned).  wslots: the resolver's int32 [T, ld_w]; batch j's n slot ids of table t at wslots[t * ld_w + j * batch_len ..]
 * (a rank passes wslots + its first column and n = its slice).  Aux slots are phase-0 slots, as the resolver writes them.
 * A call sorts `count` of the chunk's batches from batch j0 on (a SLICE: the trainer spreads a chunk's sort over several steps);
 * the lists of the other batches are left alone.
 *   _sorted_views: batch j's sorted keys / run distances / once-only flags; table t's at + t * nb * n elements.
 *   _apply_sorted: cdlrm_embbag_bwd_apply (rest = 0) or _apply_rest (rest = 1) over those lists instead of `work`'s own sort:
 *     `work` lends its scratch only (a buffer no `prepare` ever touched must be zero-filled); aux_phase: the aux region the
 *     batch trains on (what cdlrm_embbag_take was given).  One lookup per bag and table.  Same rows, bit for bit. */
uint64_t cdlrm_embbag_bwd_sorted_bytes(int32_t num_tables, int32_t nb, int64_t n);
int cdlrm_embbag_bwd_prepare_window(cdlrm_ctx* ctx, const int32_t* wslots, int64_t ld_w, int64_t batch_len, int32_t nb,
                                    int64_t n, int32_t j0, int32_t count, void* sorted, void* stream);
int cdlrm_embbag_bwd_sorted_views(cdlrm_ctx* ctx, void* sorted, int32_t nb, int64_t n, int32_t j, const uint64_t** keys,
                                  const int32_t** meta, const uint8_t** once);
int cdlrm_embbag_bwd_apply_sorted(cdlrm_ctx* ctx, int64_t n, const float* grad, int64_t ld_bag, int64_t ld_table, float lr,
                                  void* work, const uint64_t* keys, const int32_t* meta, int64_t tstride, int32_t aux_phase,
                                  int32_t rest, uint8_t* touched, void* stream);
/* The two applies with an optimizer for the cache rows.  Arguments: the sibling's, then, in front of the
 * stream (a launching entry point ends on its stream), opt / eps / state / state_base:
 *   opt = CDLRM_EMB_OPT_SGD: exactly the sibling's plan and launches; eps, state and state_base are not read.
 *   opt = CDLRM_EMB_OPT_ROWWISE_ADAGRAD: per run of a cache-proper slot s of table t, with G [D] the run's gradient sum (the
 *     sum, bit for bit, that the SGD kernels apply) and i = tags[s] the table index resident in s:
 *         S[i] += (1/D) sum_d G_d^2;   W[s] -= lr * G / (sqrt(S[i]) + eps)
 *     state: device fp32, one accumulator per TABLE row; table t's at state + state_base[t] (state_base: device int64 [T]),
 *     table_rows[t] of them.  Read and written once per looked-up slot, by the lane group that owns the run: no atomics, two
 *     launches on equal inputs give equal bits.  Aux slots (misses) are skipped: no row write, no state update.
 *     eps > 0; dim <= 1024; rest = 1 (the once-only slots already took an SGD step) is refused. */
#define CDLRM_EMB_OPT_SGD 0
#define CDLRM_EMB_OPT_ROWWISE_ADAGRAD 1
int cdlrm_embbag_bwd_apply_opt(cdlrm_ctx* ctx, const int64_t* offsets, int64_t n, int64_t n_bags,
                               int64_t ld_off, const float* grad, int64_t ld_bag, int64_t ld_table, float lr,
                               void* work, uint8_t* touched, int32_t opt, float eps, float* state,
                               const int64_t* state_base, void* stream);
int cdlrm_embbag_bwd_apply_sorted_opt(cdlrm_ctx* ctx, int64_t n, const float* grad, int64_t ld_bag, int64_t ld_table, float lr,
                                      void* work, const uint64_t* keys, const int32_t* meta, int64_t tstride, int32_t aux_phase,
                                      int32_t rest, uint8_t* touched, int32_t opt, float eps, float* state,
                                      const int64_t* state_base, void* stream);

/* Which kernels one embedding backward launches (cdlrm_embbag_bwd_route below). */
#define CDLRM_BWD_ENTRY_APPLY 0         /* cdlrm_embbag_bwd_prepare + cdlrm_embbag_bwd_apply (= cdlrm_embbag_bwd_sgd) */
#define CDLRM_BWD_ENTRY_REST 1          /* cdlrm_embbag_bwd_prepare + cdlrm_embbag_bwd_apply_rest */
#define CDLRM_BWD_ENTRY_SORTED 2        /* cdlrm_embbag_bwd_prepare_window + cdlrm_embbag_bwd_apply_sorted, rest = 0 */
#define CDLRM_BWD_ENTRY_SORTED_REST 3   /* cdlrm_embbag_bwd_prepare_window + cdlrm_embbag_bwd_apply_sorted, rest = 1 */
#define CDLRM_BWD_APPLY_CHUNKS 1        /* k_bwd_chunks: a lane group per sorted position */
#define CDLRM_BWD_APPLY_BLOCKS 2        /* k_bwd_blocks, full form: a lane group per block of 32 positions, 4 heads x 4 rows
                                           in flight (16 rows for a lone head) */
#define CDLRM_BWD_APPLY_BLOCKS_LEAN 3   /* k_bwd_blocks, lean form: one head x 4 rows (8 for a lone head) */
typedef struct cdlrm_emb_bwd_route {
    int32_t sort_chunk;         /* keys per sorting workgroup (1024, 2048, 8192) */
    int32_t sort_e;             /* keys per sorting thread (sort_chunk / 1024) */
    int32_t sort_chunks;        /* sorting workgroups per list */
    int32_t merge_passes;       /* k_merge_pass launches */
    int32_t seg_meta;           /* 1: k_seg_meta writes the run distances and once-only flags; 0: the sort kernel does */
    int32_t keys_in_b;          /* the sorted keys end in keys B (an odd number of merge passes) */
    int32_t apply;              /* CDLRM_BWD_APPLY_* */
    int32_t arange;             /* one lookup per bag (offsets NULL) */
    int32_t lpr;                /* lanes per row: 4 .. 64 */
    int32_t reserved;
    int64_t apply_grid_x, apply_grid_y;     /* the apply kernel's grid under the current cdlrm_debug_set values */
    int64_t long_grid;                      /* k_bwd_long's grid */
    int64_t keys_off, meta_off, once_off;   /* byte offsets of table 0's sorted keys / run distances / once-only flags inside
                                               `work` (table t's: t * n elements further), or inside `sorted` for batch j0 of a
                                               window chunk (table t's: t * nb * n elements further), as _sorted_views gives */
    int64_t apply_keys_off;                 /* byte offset of the keys the apply reads (== keys_off) */
} cdlrm_emb_bwd_route;
/* The plan of one backward without the launches: entry CDLRM_BWD_ENTRY_*, on num_tables tables of dim columns, n lookups per
 * table, offsets given or not (has_offsets; the window entries take none), nb / j0 / count as _prepare_window takes them (the
 * other entries ignore them).  The answer comes out of the same plan the launching calls launch from; no device is touched and
 * no pointer is read (the offsets are relative to the buffer's start). */
int cdlrm_embbag_bwd_route(int32_t num_tables, int32_t dim, int64_t n, int32_t has_offsets, int32_t entry, int32_t nb,
                           int32_t j0, int32_t count, cdlrm_emb_bwd_route* out);

/* ---------------------------------------------------------------------------------------------
 * Look-ahead window path: Prefetcher.process_batch_slice (cache_manager.py:28-46) and
 * CacheEmbeddings (main_no_ddp.py:148-209), split into plan (side stream, overlaps training of the
 * previous window) and commit (at the window boundary).
 * ------------------------------------------------------------------------------------------- */

/* Caller-owned plan buffers.  Capacities are in elements; a kernel that would exceed one sets the
 * device error word (CDLRM_ERANGE) instead of writing out of bounds. */
typedef struct {
    /* lookahead scan */
    uint64_t* bitmap;        /* [sum_k ceil(n_k/64)] zero on entry, zero again on return          */
    int64_t*  uniq;          /* [cap_uniq] sorted unique indices, table-major                      */
    int64_t*  uniq_off;      /* [T+1] start of table k in uniq                                     */
    int64_t   cap_uniq;
    /* insert plan */
    uint64_t* prot;          /* [sum_k P_k] ways hit by this window, per set (bit w)               */
    uint8_t*  hit;           /* [cap_uniq] 1 = already cached                                      */
    int32_t*  kept;          /* [cap_uniq] positions (into uniq) of the claimants, ascending       */
    int64_t*  kept_off;      /* [T+1]                                                              */
    uint8_t*  way;           /* [cap_uniq] way chosen by claimant m                                */
    uint8_t*  flags;         /* [cap_uniq] scratch for the compactions, 16-byte aligned            */
    int32_t*  winner;        /* [total cache rows] scratch, -1 on entry and on return              */
    int32_t*  win_claim;     /* [cap_win] claimant id m of winner w (ascending)                    */
    int64_t*  win_idx;       /* [cap_win] index being inserted                                     */
    int64_t*  win_row;       /* [cap_win] global cache row = row_base_k + P_k*way + set            */
    int64_t*  win_tag;       /* [cap_win] global tag element = tag_base_k + set*ways + way         */
    int64_t*  win_off;       /* [T+1]                                                              */
    int64_t   cap_win;
    float*    stage;         /* [cap_win, D] incoming rows; after commit: the rows they replaced   */
    int64_t*  ev_tag;        /* [cap_win] after commit: tag that was evicted, -1 if slot was empty */
} cdlrm_plan;

/* K1: sorted unique of every table's window indices (torch.unique, cache_manager.py:32) by bitmap +
 * popcount scan.  idx: device int64 [T, n] (row stride ld_idx).  Fills plan->uniq / uniq_off. */
int cdlrm_window_unique(cdlrm_ctx* ctx, const cdlrm_plan* plan, const int64_t* idx, int64_t n,
                        int64_t ld_idx, void* stream);
/* K1 streamed (cache_manager.py:85-110 collects a window batch by batch): _add folds one chunk [T, n] of the window
 * into the plan's bitmap, any number of times; _finish emits uniq / uniq_off for everything added since the last
 * finish and leaves the bitmap zero.  cdlrm_window_unique == one _add + _finish. */
int cdlrm_window_unique_add(cdlrm_ctx* ctx, const cdlrm_plan* plan, const int64_t* idx, int64_t n,
                            int64_t ld_idx, void* stream);
int cdlrm_window_unique_finish(cdlrm_ctx* ctx, const cdlrm_plan* plan, void* stream);

/* K2: tag probe of the unique list + full-set filter (main_no_ddp.py:155-180).
 * Fills hit / prot / kept / kept_off.  uniq and uniq_off must be valid (from cdlrm_window_unique or
 * written by the caller for the CacheEmbeddings drop-in entry). */
int cdlrm_plan_probe(cdlrm_ctx* ctx, const cdlrm_plan* plan, void* stream);

/* Copy uniq_off / kept_off / win_off ([T+1] each, any may be NULL) to host memory and wait. */
int cdlrm_plan_offsets_sync(cdlrm_ctx* ctx, const cdlrm_plan* plan, int64_t* uniq_off,
                            int64_t* kept_off, int64_t* win_off, void* stream);

/* K3: way choice + contested-slot resolution (main_no_ddp.py:171-185, 203-204).
 *   q  device fp32 [M_total, ways] Exp(1) draws in claimant order (parity mode: drawn by the torch
 *      CPU generator exactly as Categorical.sample() does), or NULL: counter-based Philox keyed by
 *      `seed` on the device (perf mode, not bit-comparable with the reference): claimant m draws, per
 *      way w, x_w = r[0] >> 8 of the Philox4x32-10 block at counter (lo, hi)(m * ways + w), c2 =
 *      0x43444c52, c3 = 0, key (lo, hi)(seed); u_w = (x_w + 1) * 2^-24, q_w = -log(u_w).
 * way = argmax_w((avail_w / sum avail) / q_w), first maximum (q == NULL: the first maximum of x_w
 * over the available ways, compared as integers); the claimant latest in ascending-index
 * order wins a contested (set, way).  Fills way / win_* . */
int cdlrm_plan_assign(cdlrm_ctx* ctx, const cdlrm_plan* plan, const float* q, uint64_t seed,
                      void* stream);

/* K3, opt-in "fill" insert policy: a collision-free, frequency-ranked way assignment that REPLACES the reference's way
 * choice and contested-slot rule (main_no_ddp.py:171-204).  A defined departure from the reference: no random number is
 * drawn, so the result is a pure function of (tags, window) and can be checked bit for bit.
 *   count     device int32 [plan->cap_uniq], caller-owned: count[u] = lookups of plan->uniq[u] in the window.
 *             _count_reset zeroes it; _count_add (after cdlrm_window_unique / _finish, any number of chunks [T, n] with
 *             row stride ld_idx) adds a chunk's lookups.  Out-of-range ids and ids that are not in the (possibly
 *             capacity-cut) unique list count nowhere.  A counter stops growing somewhere at or above 65 535: the
 *             priority is min(count, 65535).
 *   _assign_fill (after cdlrm_plan_probe, instead of cdlrm_plan_assign): inside one set of one table the claimants are
 *             ordered by priority descending, then index ascending; the claimant of rank r takes the set's r-th free way
 *             (~prot & full), empty ways (tag -1) first, then occupied ones, each group by ascending way number.
 *             Claimants of rank >= the number of free ways are not inserted (they become victims as cdlrm_plan_assign's
 *             losers do).  min(claimants, free ways) rows are inserted in every set, no slot is claimed twice, and no valid
 *             row is evicted while an empty way of its set stays empty.  count == NULL: all priorities equal (index order:
 *             the CacheEmbeddings drop-in entry has unique lists and no window).
 *   claim     device uint64 [sum_k P_k] scratch, caller-owned, zero on entry and on return.
 * Fills way / win_* exactly as cdlrm_plan_assign does; fetch, victims, commit and writeback follow unchanged. */
int cdlrm_plan_count_reset(cdlrm_ctx* ctx, const cdlrm_plan* plan, int32_t* count, void* stream);
int cdlrm_plan_count_add(cdlrm_ctx* ctx, const cdlrm_plan* plan, const int64_t* idx, int64_t n,
                         int64_t ld_idx, int32_t* count, void* stream);
int cdlrm_plan_assign_fill(cdlrm_ctx* ctx, const cdlrm_plan* plan, const int32_t* count,
                           uint64_t* claim, void* stream);

/* K5a: fetch the winners' rows into plan->stage.
 *   src_rows [T] host array of device-visible base pointers; by_position = 0: row = src[k][index]
 *   (host master tables, Embedding_Table_Group.fetch_unique_idx_slices, model_no_ddp.py:80-87);
 *   by_position = 1: row = src[k][position in uniq_k] (the `cached_entries_per_table` argument of
 *   CacheEmbeddings, main_no_ddp.py:205-206). */
int cdlrm_plan_fetch(cdlrm_ctx* ctx, const cdlrm_plan* plan, const float* const* src_rows,
                     int by_position, void* stream);

/* K4+K5b: at the window boundary swap stage <-> cache rows and write the tags
 * (main_no_ddp.py:190-206).  Afterwards stage[w] / ev_tag[w] hold the evicted row / tag. */
int cdlrm_plan_commit(cdlrm_ctx* ctx, const cdlrm_plan* plan, void* stream);

/* K14: eviction write-back (Prefetcher.eviction_manager, cache_manager.py:57-62):
 * host[k][ev_tag] = row, or (host + row) / 2 with average != 0.  dst_rows as src_rows above. */
int cdlrm_plan_writeback(cdlrm_ctx* ctx, const cdlrm_plan* plan, float* const* dst_rows,
                         int average, void* stream);

/* Window victims: the window's unique indices that stay OUTSIDE the cache after this plan commits (not cached
 * before, no way won).  The reference serves each of their lookups from the host table (aux rows,
 * model_no_ddp.py:176-179) -- the same host row every time while the window trains.  cdlrm_plan_victims (after
 * cdlrm_plan_assign, same stream) lists them and fetches their rows once into caller-owned HBM;
 * cdlrm_ctx_bind_victims (at the commit of that window) makes cdlrm_embbag_probe fill aux rows from there, falling
 * back to the host table for any index not in the list (beyond cap, or not from this window).  NULL unbinds. */
typedef struct {
    int32_t* pos;            /* [cap] positions into plan->uniq, ascending                                   */
    int64_t* idx;            /* [cap] the indices, ascending per table                                       */
    int64_t* off;            /* [T+2] start of table k; off[T] = entries listed (<= cap); off[T+1] = entries the    */
                             /*       window HAS (> cap: the list was cut -- a caller may come back with a larger one) */
    float*   rows;           /* [cap, D] their host rows                                                     */
    int64_t  cap;
} cdlrm_victims;
int cdlrm_plan_victims(cdlrm_ctx* ctx, const cdlrm_plan* plan, const cdlrm_victims* victims, void* stream);
/* The list only (pos / idx / off); the caller fills victims->rows itself (cdlrm_host_gather_rows + one DMA). */
int cdlrm_plan_victims_list(cdlrm_ctx* ctx, const cdlrm_plan* plan, const cdlrm_victims* victims, void* stream);

/* HOST function (no GPU work): dst[j, :] = tables[t(j)][idx[j], :] for j < off[T], t(j) = the table whose range
 * [off[t], off[t+1]) holds j; tables / idx / off / dst are host pointers (dst typically pinned), nthreads CPU threads.
 * The CPU-side counterpart of cdlrm_plan_fetch / the victims' row fetch -- what the reference's Prefetcher process does
 * in `emb_tables.fetch_unique_idx_slices` (model_no_ddp.py:80-87): gathered rows then reach HBM by ONE DMA copy, which
 * disturbs the training kernels far less than GPU waves reading host memory. */
int cdlrm_host_gather_rows(const float* const* tables, const int64_t* idx, const int64_t* off, int32_t T,
                           int32_t D, float* dst, int32_t nthreads);
int cdlrm_ctx_bind_victims(cdlrm_ctx* ctx, const cdlrm_victims* victims);

/* Generic row gather used by the drop-in process_batch_slice (rows = W_host[uniq],
 * model_no_ddp.py:84): out[i, :] = src[index[i], :]. */
int cdlrm_gather_rows(const float* src, const int64_t* index, int64_t count, int32_t dim,
                      float* out, void* stream);

/* Generic row scatter used by the drop-in Prefetcher.eviction_manager (cache_manager.py:57-62):
 * dst[index[i], :] = rows[i, :], or (dst + rows) / 2 with average != 0.  dst is device-visible.
 * average != 0 reads and writes dst in one pass and therefore needs DISTINCT indices; an eviction list in the
 * reference's format may repeat an index (one entry per claimant of an occupied slot, all carrying the same row,
 * SURVEY App. A): blend it first with cdlrm_blend_rows -- every entry computed from the OLD destination row, as
 * `W[idx] = (W[idx] + emb) / 2` (cache_manager.py:62) does -- then scatter the blended rows with average = 0. */
int cdlrm_scatter_rows(float* dst, const int64_t* index, const float* rows, int64_t count,
                       int32_t dim, int average, void* stream);
/* out[i, :] = (dst[index[i], :] + rows[i, :]) / 2   (the gather half of the averaging write-back) */
int cdlrm_blend_rows(const float* dst, const int64_t* index, const float* rows, int64_t count,
                     int32_t dim, float* out, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Quotient-remainder embedding bag, stand-alone operator (QREmbeddingBag.forward,
 * tricks/qr_embedding_bag.py:156-174; the reference never wires it into the cached path).
 *   q = (idx / collisions).long() as a float32 true division + truncation (quirk kept), r = idx % collisions;
 *   out[b] = sum_bag Wq[q] (op 0: * , 1: + , 2: concat) sum_bag Wr[r];  out is [n_bags, D] (2D for concat).
 *   eq_out / er_out (optional, [n_bags, D]) keep the pooled operands for the mult backward.
 *   err_word: device int32, set non-zero when a quotient falls outside Wq.
 * bwd accumulates DENSE gradients gWq [rows_q, D], gWr [collisions, D] (caller zeroes them); it skips a negative idx
 * (which the forward reports through err_word).  idx may be NULL when n == 0 (every bag empty: zero rows out).
 * ------------------------------------------------------------------------------------------- */
int cdlrm_qr_embbag_fwd(const int64_t* idx, const int64_t* offsets, int64_t n, int64_t n_bags,
                        const float* Wq, const float* Wr, int64_t rows_q, int32_t collisions, int32_t dim,
                        int32_t op, float* out, float* eq_out, float* er_out, int32_t* err_word, void* stream);
int cdlrm_qr_embbag_bwd(const int64_t* idx, const int64_t* offsets, int64_t n, int64_t n_bags,
                        const float* eq, const float* er, const float* grad_out, int64_t rows_q,
                        int32_t collisions, int32_t dim, int32_t op, float* gWq, float* gWr, void* stream);

/* ---------------------------------------------------------------------------------------------
 * The quotient-remainder trick ON the cached training step (the reference never wires it there, so the
 * semantics are this build's).  The cache holds QUOTIENT rows keyed by q; the remainder tables Wr fp32 [T, c, D] live whole
 * in HBM (the rows of plain tables unused).  One lookup per bag.  collisions: device int32 [T], c for a QR table, 0 for a
 * plain one (q = idx, r = 0, the row passes through).  op 0: mult, 1: add.
 *   cdlrm_qr_split   idx int64 [T, n] (row pitch ld_idx) -> q int64 (pitch ld_q; may alias idx) and r uint8 (pitch ld_r):
 *                    r = idx % c, q = (int64)((float)idx / (float)c) -- the stand-alone operator's float32 quotient -- and,
 *                    for an in-range idx, clamped to rows_q - 1 (rows_q = ceil(table_rows / c)).  table_rows: device int64
 *                    [T], the rows of the UNSPLIT tables; an idx outside [0, table_rows) sets the context's error word
 *                    (CDLRM_ERANGE) and yields q = r = 0.
 *   _fwd             out[b, k] = row(slots[k, b]) (*|+) Wr[k][r[k, b]]; slots int32 [T, n] as the probe / take left them,
 *                    out addressed as cdlrm_embbag_fwd's.  One rounding per element.
 *   _bwd             grad (addressed like out) holds dL/dE; rewritten IN PLACE to the cache rows' gradient (mult: g * Wr[k][r];
 *                    add: unchanged), what cdlrm_embbag_bwd_apply / _apply_sorted then consume; the [c, D] sums
 *                    gWr[k][r] = sum_b g * row (mult) / sum_b g (add) of fixed ranges of bags go to `work`
 *                    (cdlrm_qr_cached_bwd_work_bytes(T, n, D, c) bytes, 16-byte aligned), in a fixed order, no float atomics.
 *   _bwd_finish      adds those partial sums in ascending order and applies Wr -= lr * gWr; gWr fp32 [T, c, D] or NULL
 *                    receives the sums.  The partition depends on (T, n, D, c) only: two calls give the same bits.
 * Both factors of a step are read by _bwd before _bwd_finish (Wr) and the sparse-SGD path (rows) update them.
 * ------------------------------------------------------------------------------------------- */
int cdlrm_qr_split(cdlrm_ctx* ctx, const int64_t* idx, int64_t n, int64_t ld_idx, const int32_t* collisions,
                   const int64_t* table_rows, int64_t* q, int64_t ld_q, uint8_t* r, int64_t ld_r, void* stream);
int cdlrm_qr_cached_fwd(cdlrm_ctx* ctx, const int32_t* slots, const uint8_t* r, int64_t ld_r, const float* Wr,
                        const int32_t* collisions, int32_t c, int32_t op, int64_t n, float* out, int64_t ld_bag,
                        int64_t ld_table, void* stream);
uint64_t cdlrm_qr_cached_bwd_work_bytes(int32_t num_tables, int64_t n, int32_t dim, int32_t c);
int cdlrm_qr_cached_bwd(cdlrm_ctx* ctx, const int32_t* slots, const uint8_t* r, int64_t ld_r, const float* Wr,
                        const int32_t* collisions, int32_t c, int32_t op, int64_t n, float* grad, int64_t ld_bag,
                        int64_t ld_table, void* work, void* stream);
int cdlrm_qr_cached_bwd_finish(cdlrm_ctx* ctx, const int32_t* collisions, int32_t c, int64_t n, const void* work, float lr,
                               float* Wr, float* gWr, void* stream);

/* Plain EmbeddingBag(mode="sum") over one stand-alone table of ANY width, forward and dense backward: the `embs` of the
 * mixed-dimension trick's PrEmbeddingBag (tricks/md_embedding_bag.py:60-78; its widths are powers of two down to 1).
 * Stand-alone operator like the QR bag: the reference never wires it into the cached path (main_no_ddp.py:612-621).
 *   out [n_bags, dim] = sum over the bag's indices of W[idx];  gW [rows, dim] += grad_out[bag] (float atomics).
 *   err_word: device int32, bit 0 set when an index lies outside [0, rows); the backward skips such an index.
 *   idx may be NULL when n == 0. */
int cdlrm_bag_fwd(const int64_t* idx, const int64_t* offsets, int64_t n, int64_t n_bags, const float* W, int64_t rows,
                  int32_t dim, float* out, int32_t* err_word, void* stream);
int cdlrm_bag_bwd(const int64_t* idx, const int64_t* offsets, int64_t n, int64_t n_bags, const float* grad_out,
                  int64_t rows, int32_t dim, float* gW, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Table aggregation (broadcast_and_aggregate, main_no_ddp.py:250-292)
 * ------------------------------------------------------------------------------------------- */

/* touched[row_base_t + slots[t, i]] = 1 for slots int32 [T, n]: turns gathered cache_group_idxs
 * (main_no_ddp.py:254-268) into the touched-row flags cdlrm_agg_compact consumes. */
int cdlrm_mark_rows(cdlrm_ctx* ctx, const int32_t* slots, int64_t n, uint8_t* touched, void* stream);

/* Compact the touched-row flags into a sorted row list (torch.unique over the gathered
 * cache_group_idxs, :270) and clear them.  rows_out device int64 [cap]; count_out device int64 [1]. */
int cdlrm_agg_compact(cdlrm_ctx* ctx, uint8_t* touched, int64_t total_rows, int64_t* rows_out,
                      int64_t cap, int64_t* count_out, void* stream);
/* buf[i,:] = weight[rows[i],:] / scale   (:273-281)   /   weight[rows[i],:] = buf[i,:]   (:288-292)
 * for i < min(*count - first, cap): `rows` / `buf` point at entry `first` of a list whose total length is the device
 * word *count, so a merge can be cut into chunks (gather chunk i+1 while chunk i is reduced over xGMI) without the
 * host knowing more than an upper bound. */
int cdlrm_agg_gather(cdlrm_ctx* ctx, const int64_t* rows, const int64_t* count, float scale,
                     float* buf, int64_t cap, int64_t first, void* stream);
int cdlrm_agg_scatter(cdlrm_ctx* ctx, const int64_t* rows, const int64_t* count, const float* buf,
                      int64_t cap, int64_t first, void* stream);
/* Deadlines for the merge: a row only has to be merged before the first later step that USES it on any rank, and the look-ahead
 * window knows which rows the next batches use.
 * cdlrm_agg_mark_tier: tier[row] = value for every cache slot named by a [T, n] view (row pitch ld) of RESOLVED slot ids
 *   (cdlrm_window_resolve's wslots; aux slots are skipped).  Called class by class from the latest deadline to the earliest.
 * cdlrm_agg_split: stable counting sort of a merge's sorted row list (cdlrm_agg_compact; `count` entries, known to the host)
 *   by tier byte (values >= n_classes count as the last class): rows_out = the rows grouped by class, ascending inside a class
 *   -- identical on every rank --, class_off[n_classes + 1] (device) = where each class starts. */
int cdlrm_agg_mark_tier(cdlrm_ctx* ctx, const int32_t* slots, int64_t n, int64_t ld, int32_t value, uint8_t* tier, void* stream);
int cdlrm_agg_split(cdlrm_ctx* ctx, const int64_t* rows, int64_t count, const uint8_t* tier, int32_t n_classes,
                    int64_t* rows_out, int64_t* class_off, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Dense model: DLRM_Net (model_no_ddp.py:215-316), loss (main_no_ddp.py:212-221), SGD (:375, 415)
 * ------------------------------------------------------------------------------------------- */

/* interact_features "dot" (model_no_ddp.py:272-293): feat fp32 [B, F, D] (feature 0 = bottom-MLP
 * output x); R[b] = [x_b, <f_i, f_j> for i in 0..F-1 for j in 0..i-1(+itself)] fp32 [B, ld_r].  Columns of the row
 * pitch beyond the row's width are left alone or, up to the next multiple of 4, set to 0 (rows leave as whole float4
 * words when ld_r % 4 == 0 and R is 16-byte aligned). */
int cdlrm_interact_fwd(const float* feat, int64_t B, int32_t F, int32_t D, int32_t itself,
                       float* R, int64_t ld_r, void* stream);
/* dfeat[b] = (G + G^T) feat_b with G the strictly-lower (or lower) triangle filled from dR, plus dR's
 * first D columns added to feature 0.  x_act != 0: feature 0 is the output of an activation (1 ReLU,
 * 2 sigmoid; the bottom MLP's last layer, model_no_ddp.py:262-266) and its gradient row is multiplied by
 * act'(feat[b,0,:]) here, so the bottom MLP's backward starts from the pre-activation gradient. */
int cdlrm_interact_bwd(const float* feat, const float* dR, int64_t ld_r, int64_t B, int32_t F,
                       int32_t D, int32_t itself, int32_t x_act, float* dfeat, void* stream);
/* Cached EmbeddingBag forward + interact_features "dot" in ONE launch (model_no_ddp.py:200-203 + :272-293), Criteo layout
 * (one index per bag: the bag's sum-pool is its cache row).  The rows the slot ids name are read straight into the
 * interaction -- the [B, T, D] block cdlrm_embbag_fwd would write and cdlrm_interact_fwd read back is never moved.
 *   slots  device int32 [T, n] (cdlrm_embbag_probe / cdlrm_embbag_take), sample b of table t at slots[t * n + b], n >= B
 *   x      device fp32 [B, D] rows of pitch ld_x: the bottom MLP's output (feature 0)
 *   R      as cdlrm_interact_fwd's, F = T + 1; whole float4 rows (ld_r % 4 == 0, 16-byte aligned)
 * Bit-identical to cdlrm_embbag_fwd + cdlrm_interact_fwd.  Shapes: cdlrm_gather_interact_supported() (D in 32 / 64 / 128 /
 * 256, 16 < T + 1 <= 32); anything else is refused -- the caller issues the two operators.  A pair of events armed with
 * cdlrm_ctx_time_next_gather times this launch; a completion event attached with cdlrm_event_attach_next completes with it
 * (as the launch's stop event; recorded behind the launch when the launch is being timed). */
int cdlrm_gather_interact_supported(cdlrm_ctx* ctx);
int cdlrm_gather_interact_fwd(cdlrm_ctx* ctx, const int32_t* slots, int64_t n, const float* x, int64_t ld_x, int64_t B,
                              int32_t itself, float* R, int64_t ld_r, void* stream);
/* Its backward: cdlrm_interact_bwd with the rows read again from the cache (call it BEFORE the batch's embedding update:
 * cdlrm_embbag_bwd_apply rewrites them).  dfeat fp32 [B, T + 1, D] as cdlrm_interact_bwd's; carries an attached completion
 * event (cdlrm_event_attach_next) like cdlrm_interact_bwd. */
int cdlrm_gather_interact_bwd(cdlrm_ctx* ctx, const int32_t* slots, int64_t n, const float* x, int64_t ld_x,
                              const float* dR, int64_t ld_r, int64_t B, int32_t itself, int32_t x_act, float* dfeat,
                              void* stream);
/* The same with the sparse SGD step of the once-only slots folded in (main_no_ddp.py:376 backward + :413 optimizer_embeds.step()
 * for those rows).  once: uint8 flags of the batch's lookups, table t's at once + t * ld_once (cdlrm_embbag_bwd_once_flags of
 * the batch's prepared work buffer, ld_once = n; or cdlrm_embbag_bwd_sorted_views, ld_once = nb * n) -- written by a sort that has
 * COMPLETED (the caller orders the streams); lr: the embedding learning rate.  A lookup whose slot no other lookup of the batch
 * shares gets W[slot] -= lr * g in this launch (one addend: no order to keep) and its gradient row in dfeat is left UNDEFINED
 * (not written, but for stray words of the last table's); every other lookup's gradient row is written as before.  Follow
 * with cdlrm_embbag_bwd_apply_rest / _apply_sorted(rest = 1) on the same sort. */
int cdlrm_gather_interact_bwd_sgd(cdlrm_ctx* ctx, const int32_t* slots, int64_t n, const float* x, int64_t ld_x,
                                  const float* dR, int64_t ld_r, int64_t B, int32_t itself, int32_t x_act, float* dfeat,
                                  const uint8_t* once, int64_t ld_once, float lr, void* stream);
/* Which kernel an interaction call launches (cdlrm_interact_route below). */
#define CDLRM_IA_GENERIC 1      /* k_interact_fwd / k_interact_bwd: any D, a barrier per sample */
#define CDLRM_IA_ROW 2          /* k_interact_fwd_p / _bwd_p<d4>: software-pipelined, the sample's whole rows staged */
#define CDLRM_IA_SLAB 3         /* k_interact_fwd_s / _bwd_s<d4, ns, gather>: column slabs of D / ns columns */
#define CDLRM_IA_SLAB_DB 4      /* k_interact_fwd_s<d4, ns, true, true>: the slab slice double-buffered */
#define CDLRM_IA_OP_FWD 0               /* cdlrm_interact_fwd */
#define CDLRM_IA_OP_BWD 1               /* cdlrm_interact_bwd */
#define CDLRM_IA_OP_GATHER_FWD 2        /* cdlrm_gather_interact_fwd */
#define CDLRM_IA_OP_GATHER_BWD 3        /* cdlrm_gather_interact_bwd */
#define CDLRM_IA_OP_GATHER_BWD_SGD 4    /* cdlrm_gather_interact_bwd_sgd */
struct cdlrm_interact_route {   /* (a struct tag: the query below has the name) */
    int32_t family;             /* CDLRM_IA_* */
    int32_t d4;                 /* D / 4 (the template argument of the ROW / SLAB kernels) */
    int32_t ns;                 /* column slabs per sample (SLAB families), else 0 */
    int32_t reserved;
    int64_t grid;               /* workgroups of 256 lanes, under the current cdlrm_debug_set values (keys 4 and 5) */
    int64_t lds_bytes;          /* dynamic LDS of the launch */
};
/* The plan of one interaction call without the launch: op CDLRM_IA_OP_*, the call's B, F (= T + 1 for the gather ops), D,
 * itself and row pitch of R (forward) / dR (backward); aligned: bit 0 = R / dR is 16-byte aligned, bit 1 = dfeat is.  The answer
 * comes out of the same decision code the launching calls run; a shape the entry point refuses is refused here with its
 * error.  No device is touched. */
int cdlrm_interact_route(int32_t op, int64_t B, int32_t F, int32_t D, int32_t itself, int64_t ld_r, int32_t aligned,
                         struct cdlrm_interact_route* out);
/* Linear + activation (create_mlp, model_no_ddp.py:244-270): Y = act(X W^T + b).
 * X [M, K] ld_x, W [N, K] row-major (nn.Linear.weight), Y [M, N] ld_y. act: 0 none, 1 ReLU, 2 sigmoid. */
/* CDLRM_GEMM_ALONE, or-ed into `act` of cdlrm_linear_fwd / cdlrm_linear_bwd: the caller's promise that no other GEMM runs beside
 * this launch (the training step's top-MLP forward and dgrad chain).  A scheduling hint: long batches whose 128x128 tiles fill
 * the chip then take the one-workgroup-per-CU kernel (csrc/gemm_wide.h), which must not share its CU.  Same fp32 fma arithmetic;
 * the contraction order inside a 16-deep group differs from the default kernel's, so results may differ in the last bits. */
#define CDLRM_GEMM_ALONE 0x100
/* CDLRM_GEMM_BF16, or-ed into `act` of cdlrm_linear_fwd / cdlrm_linear_bwd (and their route queries), or passed as `flags` of the
 * cdlrm_mlp_wgrad*_ex calls: the opt-in bf16 matrix-core mode.  A layer with K >= 32 and N >= 32 (its shape only, never M) runs
 * all of its GEMMs on v_mfma_f32_32x32x16_bf16: each operand element is rounded once to bf16 (round-to-nearest-even, NaN kept)
 * on its way into LDS, products are exact, accumulation is fp32 in a fixed order.  Storage, bias, activations, act' masks, bias
 * gradients, slab reductions and SGD steps stay fp32.  Other layers take their fp32 route as without the flag. */
#define CDLRM_GEMM_BF16 0x200
/* CDLRM_GEMM_BF16X3, usable wherever CDLRM_GEMM_BF16 is (never both in one call: an error): the opt-in split-operand mode,
 * "near fp32" on the bf16 matrix cores.  Same layers, same kernels, same fp32 storage and epilogues; each operand element x is
 * split into two bf16 values, h = bf16(x) and l = bf16(x - h) (round-to-nearest-even; l = 0 where h is Inf or NaN), and a product
 * a * b is computed as al*bh + ah*bl + ah*bh -- three exact products, accumulated in fp32 in a fixed order; al*bl is dropped.
 * |x - h - l| <= 2^-16 |x|, so a result differs from the exact one by about 3 * 2^-16 * (|A| |B|) at most plus the fp32
 * accumulation error of 3 K terms: several times the error of an fp32 GEMM, ~1/500 of CDLRM_GEMM_BF16's.  A non-finite operand
 * element makes the outputs of its own row / column non-finite and no others; a NaN may stand where fp32 arithmetic gives an Inf
 * (Inf * l with l = 0). */
#define CDLRM_GEMM_BF16X3 0x400
int cdlrm_linear_fwd(const float* X, int64_t ld_x, const float* W, const float* bias, float* Y,
                     int64_t ld_y, int64_t M, int32_t N, int32_t K, int32_t act, void* stream);
/* Backward of the same layer.  act != 0: dY is the gradient w.r.t. the layer's OUTPUT and is overwritten
 * in place by dZ = dY * act'(Y); act == 0: dY already is dZ (Y may be NULL).
 * dX [M, K] ld_dx (may be NULL for the first layer), dW [N, K] (NULL: the weight gradient is taken later
 * by cdlrm_mlp_wgrad from the dZ left in dY), db [N] (may be NULL).
 * x_act != 0: X is itself the output of an activation (1 ReLU, 2 sigmoid) and dX is multiplied by act'(X)
 * in the GEMM epilogue, i.e. dX is then the dZ of the layer below (pass act = 0 there): the training
 * step chains the layers this way so no stand-alone activation-backward pass touches HBM.
 * work: device scratch of cdlrm_linear_bwd_work_bytes(M, N, K) bytes (split-M partial slabs of dW and of
 * db, summed in a fixed order: bitwise reproducible). */
uint64_t cdlrm_linear_bwd_work_bytes(int64_t M, int32_t N, int32_t K);
int cdlrm_linear_bwd(const float* X, int64_t ld_x, const float* W, const float* Y, int64_t ld_y,
                     float* dY, int64_t ld_dy, float* dX, int64_t ld_dx, float* dW, float* db,
                     int64_t M, int32_t N, int32_t K, int32_t act, int32_t x_act, void* work,
                     void* stream);

/* Which kernel a GEMM launch of cdlrm_linear_fwd / cdlrm_linear_bwd goes to (the route queries below). */
#define CDLRM_ROUTE_NONE 0          /* no such launch (no dX / no dW asked for) */
#define CDLRM_ROUTE_SMALLK_ROWS 1   /* k_linear_smallk_rows: K = 13, weights in registers */
#define CDLRM_ROUTE_SMALLK 2        /* k_linear_smallk: K <= 32 on the vector ALU */
#define CDLRM_ROUTE_DIRECT 3        /* k_gemm_direct: LDS-free 32x32 tiles */
#define CDLRM_ROUTE_STAGED 4        /* k_gemm_staged: 32x32 tiles, coalesced loads through wave-private LDS */
#define CDLRM_ROUTE_GEMM2 5         /* k_gemm2: LDS-DMA, (64 tm) x (64 tn) tiles */
#define CDLRM_ROUTE_GEMM3 6         /* k_gemm3: the wide kernel, (32 tm) x (32 tn) tiles, one workgroup per CU */
#define CDLRM_ROUTE_GEMM 7          /* k_gemm: register-staged, (64 tm) x (64 tn) tiles */
#define CDLRM_ROUTE_BF16 8          /* k_gemm_bf16 / k_gemm_bf16_group (CDLRM_GEMM_BF16): bf16 MFMA, (64 tm) x (64 tn) tiles */
#define CDLRM_ROUTE_BF16X3 9        /* the same kernels with two operand planes (CDLRM_GEMM_BF16X3): 64x64 or 64x128 tiles */
typedef struct cdlrm_gemm_route {
    int32_t family;         /* CDLRM_ROUTE_* */
    int32_t tm, tn;         /* tile: k_gemm / k_gemm2 in units of 64 rows / columns, k_gemm3 IM / JN in units of 32 */
    int32_t mode;           /* direct / staged: 0 one batch of loads, 1 two, 2 a loop */
    int32_t aligned;        /* direct: the aligned loader */
    int32_t splits;         /* contraction slabs (split-M weight gradient: > 1 adds the slab reduction) */
    int32_t vec_a, vec_b;   /* the kernel's 16-byte-load flags for A / B */
    int32_t fast;           /* tiles inside the matrix may take the loads-first / in-loop epilogue (k_gemm2 g2_epilogue_full,
                               k_gemm3 `fast`, the short-batch kernels' direct_prefetch) */
} cdlrm_gemm_route;
/* The plan of the same calls without the launches: same arguments (pointers are looked at for their alignment only, nothing is
 * read or written, no device is touched), plus n_cu, the compute-unit count the wide kernel's rule is evaluated for (256 on
 * MI355X).  The route is copied out of the plan the launching call builds: the launch reads the same plan.  fwd: out[0]; bwd:
 * out[0] the dgrad GEMM, out[1] the weight-gradient GEMM (family CDLRM_ROUTE_NONE where the call issues none). */
int cdlrm_linear_fwd_route(const float* X, int64_t ld_x, const float* W, const float* bias, float* Y,
                           int64_t ld_y, int64_t M, int32_t N, int32_t K, int32_t act, void* stream, int32_t n_cu,
                           cdlrm_gemm_route* out);
int cdlrm_linear_bwd_route(const float* X, int64_t ld_x, const float* W, const float* Y, int64_t ld_y,
                           float* dY, int64_t ld_dy, float* dX, int64_t ld_dx, float* dW, float* db,
                           int64_t M, int32_t N, int32_t K, int32_t act, int32_t x_act, void* work,
                           void* stream, int32_t n_cu, cdlrm_gemm_route* out);

/* Weight and bias gradients of n_layers Linear layers from the pre-activation gradients dZ[i] [M, N[i]] that
 * cdlrm_linear_bwd(dW = NULL) left behind: dW[i] [N[i], K[i]] = dZ[i]^T X[i], db[i] [N[i]] (entries may be NULL)
 * = column sums of dZ[i].  The arrays are HOST arrays of device pointers / sizes.  Replaces the per-parameter
 * autograd accumulation of the reference's loss.backward() (main_no_ddp.py:409) for the MLP weights: at small
 * per-GPU batches all layers run as one grouped launch (+ one grouped reduction of the batch slabs).
 * work: device scratch of cdlrm_mlp_wgrad_work_bytes(...) bytes, 256-byte aligned. */
uint64_t cdlrm_mlp_wgrad_work_bytes(int32_t n_layers, int64_t M, const int32_t* N, const int32_t* K);
int cdlrm_mlp_wgrad(int32_t n_layers, const float* const* X, const int64_t* ld_x, const float* const* dZ,
                    const int64_t* ld_dz, float* const* dW, float* const* db, int64_t M, const int32_t* N,
                    const int32_t* K, void* work, void* stream);
/* cdlrm_mlp_wgrad followed by the dense SGD step of the same layers -- W[i] -= lr * dW[i], b[i] -= lr * db[i]
 * (optimizer_mlps.step(), main_no_ddp.py:415) -- inside the same launches (the slab reduction writes the gradient and steps
 * the parameter): for callers with nothing between the two, i.e. one rank (no gradient exchange, :412-414).  W[i] [N[i], K[i]]
 * and b[i] [N[i]] (b[i] may be NULL where db[i] is); gradients are still left in dW / db.  Same arithmetic as
 * cdlrm_mlp_wgrad + cdlrm_sgd_step. */
int cdlrm_mlp_wgrad_sgd(int32_t n_layers, const float* const* X, const int64_t* ld_x, const float* const* dZ,
                        const int64_t* ld_dz, float* const* dW, float* const* db, float* const* W, float* const* b,
                        float lr, int64_t M, const int32_t* N, const int32_t* K, void* work, void* stream);

/* The same three calls with a flags word (0, CDLRM_GEMM_BF16 or CDLRM_GEMM_BF16X3).  flags = 0: exactly cdlrm_mlp_wgrad_work_bytes /
 * cdlrm_mlp_wgrad / cdlrm_mlp_wgrad_sgd.  CDLRM_GEMM_BF16: the layers with K[i] >= 32 and N[i] >= 32 run in bf16 (one grouped
 * launch, split-M slabs, the same fixed-order slab reduction with the SGD step inside), the others on their fp32 plan; work is
 * sized by cdlrm_mlp_wgrad_work_bytes_ex with the same flags.  CDLRM_GEMM_BF16X3: the same plan and the same work size with
 * the split operands. */
uint64_t cdlrm_mlp_wgrad_work_bytes_ex(int32_t n_layers, int64_t M, const int32_t* N, const int32_t* K, int32_t flags);
int cdlrm_mlp_wgrad_ex(int32_t n_layers, const float* const* X, const int64_t* ld_x, const float* const* dZ,
                       const int64_t* ld_dz, float* const* dW, float* const* db, int64_t M, const int32_t* N,
                       const int32_t* K, int32_t flags, void* work, void* stream);
int cdlrm_mlp_wgrad_sgd_ex(int32_t n_layers, const float* const* X, const int64_t* ld_x, const float* const* dZ,
                           const int64_t* ld_dz, float* const* dW, float* const* db, float* const* W, float* const* b,
                           float lr, int64_t M, const int32_t* N, const int32_t* K, int32_t flags, void* work, void* stream);
/* The dense optimizer (opt-in; a departure: the reference builds optimizer_mlps as optim.SGD, main_no_ddp.py:375,
 * and steps it at main_no_ddp.py:415).  CDLRM_DENSE_OPT_ADAGRAD is element-wise Adagrad -- optim.Adagrad with lr_decay = 0,
 * weight_decay = 0, initial_accumulator_value = 0 -- with one fp32 accumulator S per parameter, kept by the caller beside the
 * parameter, zero at the start:   S += g * g;   p -= lr * g / (sqrt(S) + eps)   (eps > 0; g = 0 on S = 0 leaves p unchanged). */
#define CDLRM_DENSE_OPT_SGD 0
#define CDLRM_DENSE_OPT_ADAGRAD 1
/* cdlrm_mlp_wgrad_sgd_ex with the optimizer named: its arguments, then opt, eps and the layers' accumulators SW[i] [N[i], K[i]],
 * Sb[i] [N[i]] (host arrays like W / b; Sb[i] may be NULL where the bias is not stepped) in front of work and stream.
 *   opt = CDLRM_DENSE_OPT_SGD: exactly cdlrm_mlp_wgrad_sgd_ex's plan and launches; eps, SW and Sb are not read.
 *   opt = CDLRM_DENSE_OPT_ADAGRAD: the same plan, the Adagrad step wherever the SGD step rides -- inside the slab reduction, or
 *   as an element-wise launch behind a layer whose gradient needs no reduction.  dW / db are left bit for bit as by
 *   cdlrm_mlp_wgrad_ex: the optimizer does not change the gradient. */
int cdlrm_mlp_wgrad_opt_ex(int32_t n_layers, const float* const* X, const int64_t* ld_x, const float* const* dZ,
                           const int64_t* ld_dz, float* const* dW, float* const* db, float* const* W, float* const* b,
                           float lr, int64_t M, const int32_t* N, const int32_t* K, int32_t flags, int32_t opt, float eps,
                           float* const* SW, float* const* Sb, void* work, void* stream);
/* The plan of cdlrm_mlp_wgrad_ex with the same arguments, without the launches (no pointer is read, no device touched): out[i] is
 * layer i's weight-gradient GEMM -- family, tile where the family has one, splits (slab count), vec_a / vec_b -- from the same
 * decision code.  n_cu as for cdlrm_linear_fwd_route. */
int cdlrm_mlp_wgrad_route(int32_t n_layers, const float* const* X, const int64_t* ld_x, const float* const* dZ,
                          const int64_t* ld_dz, float* const* dW, float* const* db, int64_t M, const int32_t* N,
                          const int32_t* K, int32_t flags, int32_t n_cu, cdlrm_gemm_route* out);

/* BCELoss(mean) forward + backward on the sigmoid output (torch clamps log at -100):
 * loss_out device fp32 [65]: [0] = loss, [1..64] = partial sums (fixed-order, reproducible);
 * dZ[i] = (z - t) / (max((1 - z) z, 1e-12) * n), may be NULL.  sigmoid_bwd != 0: Z came out of a
 * sigmoid (sigmoid_top, main_no_ddp.py:358) and dZ is additionally multiplied by (1 - z) z, i.e. it is
 * the gradient w.r.t. the last layer's pre-activation. */
int cdlrm_bce_fwd_bwd(const float* Z, const float* target, int64_t n, float* loss_out, float* dZ,
                      int32_t sigmoid_bwd, void* stream);

/* The loss with all its arms (main_no_ddp.py:212-221, 364-372) and the --loss-threshold clamp of the prediction
 * (model_no_ddp.py:311-314): kind 0 BCELoss(mean), 1 MSELoss(mean), 2 weighted BCE (w0 / w1 = --loss-weights for
 * target 0 / 1, mean of w[t] * BCE(none)); 0 < threshold < 1: z = clamp(Z, threshold, 1 - threshold), gradient only
 * where Z lies inside.  loss_out (>= 3 floats): [0] = loss, [1] = number of samples with round(prediction) == target
 * (the train-accuracy count of main_no_ddp.py:431, round half to even as np.round), [2] = loss * n in fp32 (the term
 * the reference adds to its running loss, :433) -- so a trainer keeps its print statistics on the device and reads them
 * at print boundaries.  dZ (may be NULL) = dL/dZ, times (1 - Z) Z when sigmoid_bwd != 0;
 * Zc (may be NULL) = the clamped prediction the reference's DLRM_Net.forward returns. */
int cdlrm_loss_fwd_bwd(const float* Z, const float* target, int64_t n, int32_t kind, float w0, float w1,
                       float threshold, float* loss_out, float* dZ, float* Zc, int32_t sigmoid_bwd, void* stream);

/* Output head in one launch: last top-MLP layer (out_features 1 + sigmoid, main_no_ddp.py:358; w [K], bias [1] or
 * NULL), the loss above, and the layer's input gradient.  Y [B, K] (row pitch ldy) is the layer's input, produced
 * by activation x_act (0 none, 1 ReLU, 2 sigmoid).  Outputs: Z [B] = sigmoid(Y w + b), Zc [B] (may be NULL) clamped
 * prediction, dZ [B] = dL/d(pre-activation of the last layer), dY [B, K] (pitch lddy; may be NULL) = dZ w^T times
 * the derivative of x_act, loss_out[0..2] as for cdlrm_loss_fwd_bwd.  scratch: cdlrm_head_scratch_floats() floats,
 * zeroed once by the caller (per-workgroup partial sums of the loss + one arrival counter the kernel leaves zero).  finish != 0: loss_out is complete when the call's work on `stream` is;
 * finish == 0: the partial sums are left in `scratch` and cdlrm_head_finish(scratch, B, loss_out, acc, any stream ordered
 * behind this call) turns them into loss_out -- the training step runs it beside the backward, not in front of it.
 * acc (may be NULL): device float64 [2], acc[0] += correct predictions, acc[1] += loss * B of this batch -- the running sums
 * the reference keeps on the host between two print boundaries (main_no_ddp.py:427-433), kept on the device instead. */
int64_t cdlrm_head_scratch_floats(void);
int cdlrm_head_fwd_bwd(const float* Y, int64_t ldy, const float* w, const float* bias, const float* target,
                       int64_t B, int32_t K, int32_t kind, float w0, float w1, float threshold, int32_t x_act,
                       float* Z, float* Zc, float* dZ, float* dY, int64_t lddy, float* loss_out, float* scratch,
                       int32_t finish, void* stream);
int cdlrm_head_finish(const float* scratch, int64_t B, float* loss_out, double* acc, void* stream);
struct cdlrm_head_route {       /* (a struct tag: the query below has the name) */
    int32_t vec;                /* 1: float4 accesses to Y, w and dY (K, both pitches multiples of 4, all three 16-byte aligned) */
    int32_t tail;               /* 1: the last workgroup to arrive completes loss_out in the same launch (finish, B <= 2048) */
    int32_t one;                /* 1: vec and K <= 256 -- a row is one float4 per lane; 0 with vec: several trips over K */
    int32_t finish_launch;      /* 1: cdlrm_head_fwd_bwd launches cdlrm_head_finish itself (finish, no tail) */
    int64_t grid;               /* workgroups of 256 lanes: 4 waves x 4 rows, at most 1024 */
    int64_t passes;             /* ceil(B / (16 * grid)): 4-row groups a wave walks */
};
/* The plan of one cdlrm_head_fwd_bwd call without the launch: the call's B, K, ldy, lddy and finish; aligned: bit 0 = Y is 16-byte
 * aligned, bit 1 = w is, bit 2 = dY is; has_dY: dY != NULL (0: lddy and bit 2 are not looked at).  The answer comes out of the
 * same decision code the launching call runs.  No device is touched. */
int cdlrm_head_route(int64_t B, int32_t K, int64_t ldy, int64_t lddy, int32_t aligned, int32_t has_dY, int32_t finish,
                     struct cdlrm_head_route* out);

/* p -= lr * g over a flat fp32 buffer (optim.SGD without momentum, main_no_ddp.py:375, 415). */
int cdlrm_sgd_step(float* param, const float* grad, int64_t n, float lr, void* stream);

/* dX *= act'(X) element-wise over an [M, N] block (row pitches lddx / ldx; act 1 ReLU output, 2 sigmoid output): the
 * "cat" interaction (model_no_ddp.py:297-299) passes the top MLP's input gradient straight to the bottom MLP's
 * output, whose activation derivative no other kernel applies. */
int cdlrm_act_bwd(float* dX, int64_t lddx, const float* X, int64_t ldx, int64_t M, int32_t N, int32_t act, void* stream);

/* The same update over two ranges [off0, off0 + n0) and [off1, off1 + n1) of one flat buffer in one launch (one
 * sub-network's weights and its biases: the bottom and the top MLP are updated at different points of the step). */
int cdlrm_sgd_step2(float* param, const float* grad, int64_t off0, int64_t n0, int64_t off1, int64_t n1, float lr,
                    void* stream);

/* cdlrm_sgd_step / cdlrm_sgd_step2 with the optimizer named (CDLRM_DENSE_OPT_*, above; departs from main_no_ddp.py:375, 415 in
 * the Adagrad mode only): `state` has param's layout.  opt = CDLRM_DENSE_OPT_SGD is exactly the sibling (state and eps not read,
 * state may be NULL); CDLRM_DENSE_OPT_ADAGRAD steps state and param over the range(s) and touches nothing outside them -- 16-byte
 * accesses where a range's start and length allow, scalar heads and tails elsewhere.  The two ranges of _step2 must not overlap. */
int cdlrm_dense_opt_step(float* param, const float* grad, float* state, int64_t n, float lr, int32_t opt, float eps,
                         void* stream);
int cdlrm_dense_opt_step2(float* param, const float* grad, float* state, int64_t off0, int64_t n0, int64_t off1, int64_t n1,
                          float lr, int32_t opt, float eps, void* stream);

/* x /= divisor (aggregate_gradients: layer.weight.grad /= world_size, main_no_ddp.py:239, 244). */
int cdlrm_scale_div(float* x, int64_t n, float divisor, void* stream);

/* ---- synthetic input (cdlrm_amd/synth.py; the reference has no Criteo-shaped generator: dlrm_data_pytorch.py:763-805 is
 * uniform multi-hot) ---------------------------------------------------------------------------------------------------------
 * out[i] = index of lookup first + i of one table's infinite, counter-based lookup stream: Zipf-like ranks (exponent alpha;
 * <= 0: uniform) scattered over [0, n_rows).  A pure function of (key, position): the trainer's batches and the look-ahead's
 * second pass over the same indices (cache_manager.py:87-90) regenerate identical data independently, one launch per table. */
int cdlrm_synth_indices(int64_t* out, int64_t count, int64_t first, int64_t n_rows, double alpha, uint64_t key, void* stream);

/* ---- ragged multi-hot bags on the device (engine.BagWindows; the reference slices by sample position,
 * main_no_ddp.py:388-391, which holds for one lookup per bag only) ---------------------------------------------------------
 * buf [total] int64: a look-ahead window of L batches, table k's list = the concatenation of its batches' table-k lists.
 * bpos [(L + 1) * T] int64: bpos[b * T + k] = position in buf of batch b's table-k list, bpos[L * T + k] = the end of table
 * k's list.  Every table list must hold >= 1 index (the host checks).  One launch covers every table. */
/* out [T, n_win] = engine.pad_window(): table k's window list, padded with its own first index (n_win >= the longest). */
int cdlrm_bags_window(const int64_t* buf, int64_t total, const int64_t* bpos, int32_t L, int32_t T, int64_t n_win,
                      int64_t* out, void* stream);
/* Batch b (global offsets off [T, nbag]), a rank's samples [s0, s1), nb = s1 - s0: engine.square_bags() of the rank's
 * lookups, rebased.  With a_k = off[k, s0], e_k = off[k, s1] (s1 < nbag) or the batch's table-k length, m_k = e_k - a_k:
 * idx [T, n] (16-byte aligned, n even and >= every m_k) = list_k[a_k + i] for i < m_k, padded with list_k[a_k];
 * off_out [T, nb + 1] = off[k, s0 + i] - a_k, and off_out[k, nb] = m_k (the padding lookups pool into the scratch bag nb). */
int cdlrm_bags_rank_slice(const int64_t* buf, int64_t total, const int64_t* bpos, int32_t L, int32_t b, int32_t T,
                          const int64_t* off, int64_t nbag, int64_t s0, int64_t s1, int64_t n, int64_t* idx, int64_t* off_out,
                          void* stream);

/* ---- Criteo day-file batches cut on the device (data_loader_terabyte.DeviceDayLoader) ---------------------------------
 * Replaces, for n raw rows of a pre-processed day file that lie in HBM as the file stores them (x_int int32 [n, n_dense],
 * x_cat int32 [n, n_cat], y int32 [n], row-major), the reference's per-batch host transform _transform_features
 * (data_loader_terabyte.py:68-87) and the trainer's per-step uploads of its result (main_no_ddp.py:388-391):
 *   X[col0 + i, :]                 fp32  = log((float)x_int[i, :] + 1.0f)    (int32 -> fp32 first, an fp32 add, as :73; the
 *                                          logarithm is taken in double and rounded once)
 *   lS_i[k * lS_i_pitch + col0 + i] int64 = x_cat[i, k], reduced by numpy's floor-mod when max_ind_range > 0 (:70-71: a negative
 *                                          entry gives a non-negative result), untouched otherwise
 *   T[col0 + i]                    fp32  = y[i]
 * X is fp32 [>= col0 + n, n_dense] row-major, T fp32 [>= col0 + n], lS_i int64 [n_cat, lS_i_pitch] with lS_i_pitch >= col0 + n:
 * several file segments of one look-ahead window land in one rectangle, one launch each; cells outside columns
 * [col0, col0 + n) are not written.  n_cat <= 60 (a tile of samples is staged in LDS).  Not a tape entry point: it never runs
 * on the training queue. */
int cdlrm_dayfile_window(const int32_t* x_int, const int32_t* x_cat, const int32_t* y, int64_t n, int32_t n_dense, int32_t n_cat,
                         int64_t max_ind_range, float* X, int64_t* lS_i, int64_t lS_i_pitch, int64_t col0, float* T,
                         void* stream);
/* samples per workgroup of cdlrm_dayfile_window (tests probe its edges; tools size their grids by it) */
int cdlrm_dayfile_tile(void);

/* ---- rows of the processed Criteo file, resident in HBM, cut by an order (data_loader_processed.DeviceProcessedLoader) ---
 * Replaces, for the in-memory processed file of the reference's default dataset path (dlrm_data_pytorch.py:198-254: the whole
 * X_int / X_cat / y re-listed row by row in the randomised order), its per-sample CriteoDataset.__getitem__ (:258-295, the
 * `% max_ind_range`), the DataLoader's collate_wrapper_criteo (:323-338) and the trainer's per-step uploads of the result
 * (main_no_ddp.py:388-391).  x_int int32 [n_rows, n_dense], x_cat int32 [n_rows, n_cat], y int32 [n_rows] are the file's
 * arrays as they lie in HBM; sample i of the piece is row order[i], order int64 [n] on the device, 8-byte aligned, every entry
 * in [0, n_rows) -- the caller's responsibility (the loader checks an order once on the host when it uploads it; the kernel
 * does not look again).  Outputs and their meaning are cdlrm_dayfile_window's, word for word, for x_int[order[i], :],
 * x_cat[order[i], :], y[order[i]]: the same log in double rounded once, the same floor-mod, T = (float)y, cells outside
 * columns [col0, col0 + n) not written, n_cat <= 60; for the same rows the two entry points give the same bits.  Every row
 * address is formed in 64 bits (row * 104 B passes 2^32 at 41.3 M rows).  A run of consecutive rows needs no order: it goes
 * through cdlrm_dayfile_window on offset pointers.  Not a tape entry point: it never runs on the training queue. */
int cdlrm_rows_window(const int32_t* x_int, const int32_t* x_cat, const int32_t* y, int64_t n_rows, const int64_t* order,
                      int64_t n, int32_t n_dense, int32_t n_cat, int64_t max_ind_range, float* X, int64_t* lS_i,
                      int64_t lS_i_pitch, int64_t col0, float* T, void* stream);
/* samples per workgroup of cdlrm_rows_window */
int cdlrm_rows_tile(void);

/* ---- MLPerf binary Criteo records cut on the device (data_loader_terabyte.DeviceBinLoader) ------------------------------
 * Replaces, for n records of the binary file that lie in HBM as the file stores them (rec int32 [n, 1 + n_dense + n_cat],
 * a record = [y | n_dense | n_cat], data_loader_terabyte.py:238-275), CriteoBinDataset.__getitem__'s host transform
 * (data_loader_terabyte.py:225-235 -> _transform_features, :68-87) and the trainer's per-step uploads of its result
 * (main_no_ddp.py:388-391).  Outputs and their meaning are cdlrm_dayfile_window's, word for word, with
 * x_int[i, :] = rec[i, 1 : 1 + n_dense], x_cat[i, :] = rec[i, 1 + n_dense :], y[i] = rec[i, 0]: the same log in double
 * rounded once, the same floor-mod, cells outside columns [col0, col0 + n) not written, n_cat <= 60; in addition a tile of
 * 256 whole records must fit the LDS (1 + n_dense + n_cat <= 159).  rec needs 4-byte alignment only.  Not a tape entry
 * point: it never runs on the training queue. */
int cdlrm_binfile_window(const int32_t* rec, int64_t n, int32_t n_dense, int32_t n_cat, int64_t max_ind_range, float* X,
                         int64_t* lS_i, int64_t lS_i_pitch, int64_t col0, float* T, void* stream);
/* samples per workgroup of cdlrm_binfile_window */
int cdlrm_binfile_tile(void);

/* ---- raw Criteo text -> processed arrays (cdlrm_amd/data_utils.py: getCriteoAdData) ---------------------------------------
 * The reference's ETL (data_utils.py:876-1121) reads the raw text line by line in Python (process_one_file, :966-1044),
 * sub-samples (:976-993), builds one dictionary per categorical column (:1008-1009, :1080-1089) and rewrites every value as
 * its id (processCriteoAdData, :111-169).  These entry points do the per-line work on a chunk of text in HBM; the grammar of
 * a line, the two departures from the reference (int32 X_cat; a hash >= 2^31 keeps its bit pattern) and the error codes are
 * csrc/etl_parse.h and DESIGN.md section 3.  None is a tape entry point; every launch is on the stream given.
 *
 * err: ONE 64-bit word on the device, set to all ones by the caller (= no error).  A malformed line, or a value missing from
 * a dictionary, lowers it to (line << 8 | code) by an integer atomic minimum, line the 1-based number in the file (row for
 * cdlrm_etl_encode): the host reads the FIRST bad line whatever the order the lanes ran in. */

/* bytes of cdlrm_etl_line_index's work buffer for a chunk of len bytes */
int64_t cdlrm_etl_line_index_work_bytes(int64_t len);
/* text [len] (16-byte aligned) -> starts[0] = 0, starts[j + 1] = one past the j-th newline, for j < min(count, cap);
 * *d_count = the number of newlines = of lines that END inside the chunk (data_utils.py:982: `for k, line in enumerate(f)`).
 * Line j is text[starts[j], starts[j + 1] - 1); bytes behind starts[count] are no line (the host carries them in front of the
 * next chunk); a chunk without a newline gives count 0.  starts holds cap + 1 entries. */
int cdlrm_etl_line_index(const uint8_t* text, int64_t len, int64_t* starts, int64_t cap, int64_t* d_count, void* work,
                         int64_t work_bytes, void* stream);
/* lines [0, n) of the index -> y [n], x_int [n, 13] (negatives already 0, data_utils.py:150), x_cat [n, 26] int32, the hex
 * value % max_ind_range first when max_ind_range > 0 (:984-1006).  line0: the 0-based number in its file of line 0 (for the
 * error word).  A malformed line gives zeros and its code; a span outside text[0, len) is never read. */
int cdlrm_etl_parse(const uint8_t* text, int64_t len, const int64_t* starts, int64_t n, int64_t line0, int64_t max_ind_range,
                    int32_t* y, int32_t* x_int, int32_t* x_cat, void* err, void* stream);
/* bytes of cdlrm_etl_subsample's work buffer for n rows */
int64_t cdlrm_etl_subsample_work_bytes(int64_t n);
/* data_utils.py:989-993: row i is dropped iff y[i] == 0 and rand_u[line0 + i] < rate (float64); the kept rows go, in order,
 * to rows [*rows_in, *rows_in + kept) of the out arrays (out_cap rows) and *rows_out = *rows_in + kept -- two different
 * device words, so consecutive chunks chain without a host read.  rate > 0: at rate 0 nothing is launched. */
int cdlrm_etl_subsample(const int32_t* y, const int32_t* x_int, const int32_t* x_cat, int64_t n, const double* rand_u,
                        int64_t n_rand, int64_t line0, double rate, int32_t* out_y, int32_t* out_x_int, int32_t* out_x_cat,
                        int64_t out_cap, const int64_t* rows_in, int64_t* rows_out, void* work, int64_t work_bytes, void* stream);
/* data_utils.py:144-147 (`X_cat_t[j, k] = convertDicts[j][x]`): x_cat[r, col] of a row-major [n, n_cols] array becomes
 * ids[k] where keys[k] equals it; keys [m] ascending, m < 2^31, found in at most 32 halvings.  A value keys does not hold
 * becomes 0 and sets err to (row0 + r + 1) << 8 | 6. */
int cdlrm_etl_encode(int32_t* x_cat, int64_t n, int32_t n_cols, int32_t col, const int32_t* keys, const int32_t* ids, int64_t m,
                     int64_t row0, void* err, void* stream);

/* ---- launch tapes -------------------------------------------------------------------------------------------------
 * A training step's call sequence (this library's entry points + event records / stream waits), recorded once per control
 * path by the host and re-issued by ONE call per step (the reference issues the same ops from Python every iteration,
 * main_no_ddp.py:404-415; at a per-rank batch of 1024 the interpreter alone costs more than the GPU work).  Calls are
 * stored as (function, integer-class arguments, float arguments); an integer argument may be a "cell" -- a slot of the
 * tape's cell array that the host patches before a replay (the batch's tensors).  Every entry point a tape may hold is
 * registered in csrc/tape.hip with its true type and called through a pointer of that type (cdlrm_tape_add refuses
 * anything else); cdlrm_tape_selftest() checks the argument unpacking. */
typedef struct cdlrm_tape cdlrm_tape;
cdlrm_tape* cdlrm_tape_create(int32_t n_cells);
void cdlrm_tape_destroy(cdlrm_tape* t);
/* fn: any entry point of this header with scalar arguments (<= 24 integer-class, <= 8 float); iargs/fargs in parameter
 * order per class; cell[i] >= 0 takes iargs[i] from that cell at replay time. */
int cdlrm_tape_add(cdlrm_tape* t, void* fn, int32_t n_int, const int64_t* iargs, const int32_t* cell, int32_t n_flt,
                   const float* fargs);
int64_t* cdlrm_tape_cells(cdlrm_tape* t);
int64_t cdlrm_tape_length(cdlrm_tape* t);
/* position, in fn's parameter list, of the stream the call issues on (the library's convention is "last parameter"; the
 * event / stream calls below differ); -1: the call issues nothing itself; -2: fn is not a registered tape entry point */
int32_t cdlrm_tape_stream_arg(void* fn);
/* development (tools/host_time.py): op k's entry-point name (NULL: no such op) and, in out[5], its lane, the replays timed,
 * the host nanoseconds spent inside the call and waiting for another lane's op, the longest single call; the clocks run under cdlrm_debug_set(3, 1) */
const char* cdlrm_tape_op_info(cdlrm_tape* t, int64_t k, int64_t* out);
int cdlrm_tape_replay(cdlrm_tape* t);      /* first non-zero return code of a replayed call, else 0 */
/* Multi-lane replay: at short per-rank batches the HOST thread that issues a step's ~45 runtime calls, not the GPU, sets the
 * step time.  lane[k] = 1 .. 3 hands op k to that helper thread of the process (one per side queue), lane[k] = 0 stays with
 * the thread that calls cdlrm_tape_replay (the training queue's calls); dep[k] >= 0 = the tape index of an earlier op of
 * ANOTHER lane that has to be issued first -- the host-side order of the record / wait calls on one event.
 * n = cdlrm_tape_length. */
int cdlrm_tape_set_lanes(cdlrm_tape* t, const int32_t* lane, const int32_t* dep, int64_t n);
int cdlrm_tape_selftest(void);
/* Float cells: float arguments that change from step to step -- the two learning rates under a schedule;
 * every kernel still takes its rate by value.  cdlrm_tape_set_float_cells gives the tape n (0 .. 16) of them, before the ops
 * that name them are added; cdlrm_tape_add_fc is cdlrm_tape_add with fcell[i] >= 0 taking fargs[i] from that float cell at
 * replay time (-1: the literal); the host writes cdlrm_tape_float_cells(t)[k] (NULL: the tape has none) before
 * cdlrm_tape_replay, which reads them only from then on, in every lane.  cdlrm_tape_float_cells_selftest(): one op with a
 * float cell in two argument positions next to literals, replayed with three values (no GPU involved). */
int cdlrm_tape_set_float_cells(cdlrm_tape* t, int32_t n);
float* cdlrm_tape_float_cells(cdlrm_tape* t);
int cdlrm_tape_add_fc(cdlrm_tape* t, void* fn, int32_t n_int, const int64_t* iargs, const int32_t* cell, int32_t n_flt,
                      const float* fargs, const int32_t* fcell);
int cdlrm_tape_float_cells_selftest(void);
/* Self-test hooks (no GPU involved; used by cdlrm_tape_selftest and tests/test_host_logic.py): a call with interleaved
 * float / int32 / pointer / int64 parameters that adds its arguments up, and a logging call (spins `spin` iterations, then
 * appends `tag` to a process-wide log that cdlrm_tape_probe_log_take drains; returns the number of entries logged). */
int cdlrm_tape_probe(float f0, int64_t a0, float f1, int32_t a1, void* a2, int64_t a3, float f2, int32_t a4, int64_t a5,
                     int64_t a6, void* a7, int32_t a8, float f3, int64_t a9);
int cdlrm_tape_probe_log(int64_t tag, int64_t spin);
int64_t cdlrm_tape_probe_log_take(int64_t* out, int64_t cap);
/* hipEventRecord / hipStreamWaitEvent as tape-able entry points (raw hipEvent_t / hipStream_t handles) */
int cdlrm_event_record(void* event, void* stream);
int cdlrm_stream_wait_event(void* stream, void* event);
/* `event` completes with the next kernel the calling thread launches on `stream` through cdlrm_linear_bwd,
 * cdlrm_interact_bwd, cdlrm_gather_interact_bwd or cdlrm_gather_interact_fwd -- attached to that launch as its stop event instead of recorded behind it: a record is a marker packet
 * and a 6-8 us bubble on the training queue, an attached event is free.  If the call cannot attach it (several launches, a
 * kernel path without the plumbing) it records the event behind its launches: same guarantees either way. */
int cdlrm_event_attach_next(void* event, void* stream);
/* a stream at an explicit priority (lower = more urgent, clamped into the device's range): the look-ahead plan's stream is
 * created at the least urgent level so that the training step goes first wherever the two compete for CUs */
void* cdlrm_stream_create(int32_t priority);
int cdlrm_stream_destroy(void* stream);
/* events of the library's own (handles exist from creation on); elapsed time in microseconds, waits for `stop` */
void* cdlrm_event_create(int32_t timing);
int cdlrm_event_destroy(void* event);
int cdlrm_event_elapsed_us(void* start, void* stop, float* us);
/* Measurement: the NEXT cdlrm_embbag_fwd (or cdlrm_gather_interact_fwd) on this context leaves its start / stop timestamps in the two (timing) events --
 * attached to the launch itself (hipExtLaunchKernel), no event records around it -- so bench.py can price the gather
 * (the roofline kernel) live, per launch.  A timed launch costs its queue ~7 us (completion signal); the elapsed time reads
 * 0.5-2 us above the profiler's duration of the same kernel. */
int cdlrm_ctx_time_next_gather(cdlrm_ctx* ctx, void* start_event, void* stop_event);

#ifdef __cplusplus
}
#endif
#endif /* CDLRM_HIP_H */
