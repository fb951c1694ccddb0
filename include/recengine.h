/* recengine — C-ABI of the MI355X-native sparse-embedding + feature-interaction engine that
 * stands in for the Paddle ops on the hot path of PaddleRec's models/rank CTR stack.
 *
 * The reference has no FFI seam of its own: the seam is the Paddle operator API used inside
 * net.py.  Each entry point below names the reference call site whose Paddle
 * ops it replaces; a Paddle custom-op shim (PD_BUILD_OP) or the ctypes/torch
 * adapter in paddlerec_amd/ binds exactly these symbols.
 *
 * Conventions
 *   - plain pointers + sizes only; every pointer is a DEVICE pointer unless marked "host".
 *   - the caller owns every buffer (tables, outputs, workspace); nothing is retained.
 *   - every launch is asynchronous on `stream` (a hipStream_t passed as void*); no internal sync.
 *   - return 0 on success or a negative rec_status; rec_last_error() gives thread-local text.
 *   - `status` arguments are device int32 words the kernels OR error bits into
 *     (REC_FLAG_*), so out-of-range indices are reported without a host sync.
 *   - tables are row-major f32 [num_rows, row_stride] with row_stride >= emb_dim (floats).
 */
#ifndef RECENGINE_H_
#define RECENGINE_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
  REC_OK = 0,
  REC_EINVAL = -1,     /* null pointer / negative size / unsupported combination */
  REC_ESHAPE = -2,     /* dimension outside what the kernels are built for */
  REC_EWORKSPACE = -3, /* workspace too small (query *_workspace_bytes first) */
  REC_EHIP = -4,       /* HIP runtime error at launch */
  REC_ENCCL = -5
} rec_status;

/* bits OR-ed into a device status word */
#define REC_FLAG_INDEX_OOB 1 /* an id was < 0 or >= num_rows (Paddle raises on OOB [EXT]) */
#define REC_FLAG_EXCHANGE_OVERFLOW 2 /* host binders (paddlerec_amd/sharded.py, deduplicated exchange): a rank needed more
                                        distinct rows of one owner than the fixed exchange capacity; the rows behind it
                                        read as zeros and their gradients are dropped — raise the capacity */

const char* rec_last_error(void); /* host; thread-local */
int rec_version(void);            /* host */

/* ------------------------------------------------------------------------------------------
 * DeepFM: embedding lookup + FM first/second order, fused.
 * Replaces concat + Embedding x2 + multiply/unsqueeze/sum/square/concat of
 *   models/rank/deepfm/net.py:105-139 (FM.forward).
 * ---------------------------------------------------------------------------------------- */
typedef struct {
  int64_t batch;       /* B */
  int32_t num_slots;   /* S  (26) : sparse fields, one id each */
  int32_t num_dense;   /* Dn (13) : dense fields, <= 16 */
  int32_t emb_dim;     /* D  <= 256 */
  int32_t row_stride;  /* floats between consecutive rows of W (>= D) */
  int64_t num_rows;    /* N rows in W / W1 (after slot offsets) */
  int64_t padding_idx; /* id that yields a zero row and no gradient; < 0 = none */
  int32_t w1_stride;   /* floats between consecutive entries of W1; 0 or 1 = dense [N] array.
                          HBM fetches whole 128-B lines: a table kept as 32-float records
                          [W(16) | W1 | ...] (W1 = W + 16, both strides 32) costs ONE line per
                          lookup instead of two (see DESIGN.md "table layout"). */
  int32_t compact_dense; /* 0: feat = [B, S+Dn, D] (= feat_embeddings, net.py:120).
                            1: feat = [B, S+1, D]: the S embedding rows plus ONE row holding the Dn raw dense
                            values (zero padded to D; needs Dn <= D).  The dense "embeddings" x_j*dense_w[j,:]
                            are never materialised: the FM sums still include them (computed in registers),
                            and the top MLP's first layer sees them through folded weights
                            (rec_dense_fold_fwd): feat'[B,(S+1)D] @ [W0_sparse; M; 0] == feat[B,(S+Dn)D] @ W0.
                            In this mode rec_deepfm_fm_bwd takes d_feat_dnn in the same [B,S+1,D] layout and
                            its d_dense_w holds the FM part only (the MLP part comes from rec_dense_fold_bwd). */
  int64_t feat_stride;   /* floats between consecutive samples of feat (and of d_feat_dnn in the backward); 0 = dense
                            (fields x emb_dim).  A caller whose first MLP layer wants an input width that is a multiple
                            of its GEMM tiles (39 fields x 10 = 390 -> 400) keeps feat in a zero-initialised
                            [B, feat_stride] buffer: the kernels never touch the padding columns. */
} rec_deepfm_desc;

/* ids [B,S] i64 (= paddle.concat(sparse_inputs,1), net.py:107); dense [B,Dn] f32;
 * W [N,stride], W1 [N]; dense_w [Dn,D]; dense_w_one [Dn];
 * slot_offset [S] i64 or NULL: row = id + slot_offset[s] (26 tables laid out as one);
 * outputs y1,y2 [B]; feat [B,S+Dn,D] (= feat_embeddings, net.py:120);
 * sum_emb [B,D] (= summed_features_emb, net.py:124; kept for backward). */
int rec_deepfm_fm_fwd(const rec_deepfm_desc* desc, const int64_t* ids, const float* dense,
                      const float* W, const float* W1, const float* dense_w,
                      const float* dense_w_one, const int64_t* slot_offset, float* y1, float* y2,
                      float* feat, float* sum_emb, int32_t* status, void* stream);

/* Backward of the block above (what loss.backward(), tools/trainer.py:151, runs for net.py:105-139).
 * In : dense, feat, sum_emb (saved by fwd), d_feat_dnn [B,S+Dn,D], dy1, dy2 [B];
 *      dense_w [Dn,D] or NULL: when given, the dense part of feat is recomputed as
 *      dense[b,j]*dense_w[j,:] (bit-identical to what fwd stored) instead of re-read.
 * Out: row_grad [B*S, D]  — SelectedRows.value of `embedding` (rows = flattened ids, unmerged);
 *      d_dense_w [Dn,D], d_dense_w_one [Dn] — batch sums, reduced in a fixed order (deterministic).
 *      The SelectedRows.value of `embedding_one` is dy1[b] for every (b,s); it is not
 *      materialised — rec_sparse_adam_rows reads dy1 through rec_grad_layout{S,0,0}. */
int rec_deepfm_fm_bwd_workspace_bytes(const rec_deepfm_desc* desc, size_t* bytes);
int rec_deepfm_fm_bwd(const rec_deepfm_desc* desc, const float* dense, const float* feat,
                      const float* sum_emb, const float* d_feat_dnn, const float* dy1,
                      const float* dy2, const float* dense_w, float* row_grad, float* d_dense_w,
                      float* d_dense_w_one, void* workspace, size_t workspace_bytes, void* stream);
/* The same backward with the SelectedRows value written in SORTED order: the gradient row of lookup (b, s) goes to
 * row_grad + row_rank[b*S+s] * D (row_rank from rec_ids_group_slots / rec_ids_rank; < 0 = padding, not written), so the
 * merge + optimizer kernel reads every row's duplicates as consecutive rows (rec_grad_layout.sorted = 1). */
int rec_deepfm_fm_bwd_sorted(const rec_deepfm_desc* desc, const float* dense, const float* feat,
                             const float* sum_emb, const float* d_feat_dnn, const float* dy1,
                             const float* dy2, const float* dense_w, const int32_t* row_rank, float* row_grad,
                             float* d_dense_w, float* d_dense_w_one, void* workspace, size_t workspace_bytes,
                             void* stream);

/* Folding the dense "embeddings" into the first MLP layer (compact_dense = 1 above).
 *   fwd: M[j,n] = sum_d dense_w[j,d] * W0[(S+j)*D + d, n]                    -> M [Dn, n_out]
 *        so that  sum_j x_j * (dense_w[j,:] @ W0_rows(j))  ==  x @ M   (net.py:110-119,170-171 re-associated)
 *   bwd: given dM [Dn, n_out] (rows S*D .. S*D+Dn-1 of feat'^T dZ0):
 *        dW0[(S+j)*D + d, n] = dense_w[j,d] * dM[j,n];   d_dense_w[j,d] (+)= sum_n dM[j,n] * W0[(S+j)*D+d, n]
 * W0 is the layer's weight [ (S+Dn)*D, n_out ] (Paddle [in,out]); dW0 its gradient buffer (only the dense rows
 * are written). */
int rec_dense_fold_fwd(int32_t num_slots, int32_t num_dense, int32_t emb_dim, int32_t n_out,
                       const float* dense_w, const float* W0, float* M, void* stream);
/* The same folds with the row copies around them, ONE launch each way (what a training step issues):
 *   fwd_full: W0_folded [(S+1)*D, n_out]: rows [0, S*D) = W0's, rows S*D + j = M[j,:] (the rest stays as the caller
 *             left it: zero);
 *   bwd_full: dW0_folded = feat'^T dZ0 [(S+1)*D, n_out] (a scratch of the caller's, NOT the gradient buffer): its sparse
 *             rows are copied into dW0, its rows S*D.. are dM -> the dense rows of dW0 and d_dense_w as above. */
int rec_dense_fold_fwd_full(int32_t num_slots, int32_t num_dense, int32_t emb_dim, int32_t n_out, const float* dense_w,
                            const float* W0, float* W0_folded, void* stream);
int rec_dense_fold_bwd_full(int32_t num_slots, int32_t num_dense, int32_t emb_dim, int32_t n_out, const float* dense_w,
                            const float* W0, const float* dW0_folded, float* dW0, float* d_dense_w,
                            int32_t accumulate_ddw, void* stream);
int rec_dense_fold_bwd(int32_t num_slots, int32_t num_dense, int32_t emb_dim, int32_t n_out,
                       const float* dense_w, const float* W0, const float* dM, float* dW0,
                       float* d_dense_w, int32_t accumulate_ddw, void* stream);

/* ------------------------------------------------------------------------------------------
 * Plain lookup and LoD sum-pool.
 *   rec_emb_gather         : nn.Embedding forward (deepfm/net.py:108,117; dcn_v2/net.py:93-96;
 *                            din/net.py:141-147).  out[i,:] = id==padding_idx ? 0 : W[id,:]
 *   rec_emb_gather_sumpool : sparse_embedding + sequence_pool('sum')
 *                            (models/rank/slot_dnn/net.py:63-75; dnn/static_model_lod.py:70-97).
 *                            out[b,:] = sum_{k in [lod[b],lod[b+1])} W[ids[k],:], padding ids skipped;
 *                            counts[b] = number of non-padding ids pooled (bit-exact).
 * ---------------------------------------------------------------------------------------- */
/* out_group > 0: lookup i is written at out + (i / out_group) * out_group_stride + (i % out_group) * D
 * (e.g. the S sparse fields of a sample into the head of a wider feature row, dcn_v2/net.py:100-108);
 * out_group <= 0: contiguous [n, D]. */
int rec_emb_gather(int64_t n, int32_t emb_dim, int32_t row_stride, int64_t num_rows,
                   int64_t padding_idx, const int64_t* ids, const float* W, float* out,
                   int32_t out_group, int64_t out_group_stride, int32_t* status, void* stream);
int rec_emb_gather_sumpool(int64_t batch, int32_t emb_dim, int32_t row_stride, int64_t num_rows,
                           int64_t padding_idx, const int64_t* ids, const int64_t* lod /*[B+1]*/,
                           const float* W, float* out, int32_t* counts, int32_t* status,
                           void* stream);
/* What an unborn row of a lazily created PS table reads as when the accessor does NOT zero-initialise embed_w
 * (rec_ps_accessor.embed_zero_init = 0; rec_ps_push_rows gives birth with the same values): element 0 (embed_w)
 * always, elements 1.. when init_dims > 1; keyed by (seed, row*row_mul+row_add, d).
 * init_range <= 0 (Paddle's default, zero_init): rows are plain memory — an unborn row reads as zeros. */
typedef struct {
  int32_t state_offset; /* floats from the row start to the state float (0 = unborn) */
  int32_t init_dims;
  float init_range;
  uint64_t seed;
  int64_t row_mul, row_add;
} rec_lazy_init;
/* Owner-side lookup of a row-sharded DeepFM table (tools/static_gpubox_trainer.py:152-160: the pull of the GPU
 * parameter server): out_w[i,:] = rec[rows[i], 0:D], out_w1[i] = rec[rows[i], D] — both embeddings of
 * deepfm/net.py:62-86 from the one record line of a row.  lazy may be NULL. */
int rec_record_gather(int64_t n, int32_t emb_dim, int32_t rec_stride, int64_t num_rows, const int64_t* rows,
                      const float* rec, float* out_w, float* out_w1, const rec_lazy_init* lazy,
                      int32_t* status, void* stream);

/* backward of the sum-pool: SelectedRows.value[k,:] = d_out[sample(k),:]  (rows = ids). */
int rec_emb_sumpool_bwd(int64_t batch, int32_t emb_dim, const int64_t* lod, const float* d_out,
                        float* row_grad, void* stream);

/* ------------------------------------------------------------------------------------------
 * ALL slots of a batch in one launch: the `for s_input in slot_inputs: sparse_embedding(...,
 * padding_idx=0, entry=ShowClickEntry) -> sequence_pool('sum')` loop + concat(axis=1) of
 * models/rank/slot_dnn/net.py:63-77 (408 slots x D 9) and dnn/static_model_lod.py:70-97.
 * Input = the slot-major CSR of rec_parse_feasign_slots, resident on the device:
 *   values [nnz]; ids of (slot s, sample b) = values[slot_base[s] + lod[s*lod_stride + b] ..
 *                                                    slot_base[s] + lod[s*lod_stride + b + 1])
 * key_mode 0: values are table rows (checked against [0,num_rows), REC_FLAG_INDEX_OOB otherwise);
 * key_mode 1: values are uint64 feasign bit patterns (what the reference feeds its PS hash map,
 *             queuedataset_reader.py:56-82); row = rec_feasign_rows' hash, 0 stays the padding row.
 * padding_idx is compared with the VALUE (before hashing); < 0 = no padding id.
 * Outputs: out [B, out_stride] with out[b, s*D:(s+1)*D] = sum of the segment's rows (padding skipped);
 *   counts [B,S] i32 (or NULL) = ids pooled per segment — bit-exact target;
 *   seg_of_value [nnz] i32 (or NULL) = b*S+s of every value: rec_grad_layout.index for the backward;
 *   rows_out [nnz] i64 (or NULL) = table row of every value (dropped ones -> the padding row): the `ids`
 *   of rec_ids_group(n = nnz, num_slots = 1) for the SelectedRows merge of the backward.
 * ---------------------------------------------------------------------------------------- */
typedef struct {
  int64_t batch;
  int32_t num_slots;
  int32_t emb_dim;
  int32_t row_stride;  /* floats between rows of W */
  int32_t key_mode;    /* 0 rows, 1 uint64 feasigns */
  int64_t num_rows;
  int64_t padding_idx;
  int64_t lod_stride;  /* elements between slot rows of lod; 0 = batch + 1 */
  int64_t out_stride;  /* floats between samples of out; 0 = num_slots * emb_dim */
  /* PS tables create a feature at its first pull (MemorySparseTable + SparseAdaGradSGDRule::InitValue [EXT],
   * slot_dnn/config_online.yaml:66-79 initial_range): init_range > 0 makes a row whose state float
   * W[row*row_stride + state_offset] is 0 read as its creation values — element d < init_dims =
   * uniform(+-init_range) keyed by (init_seed, row, d), the rest 0 — without writing the table
   * (rec_ps_push_rows gives birth with the same values).  init_range <= 0: off. */
  int32_t state_offset;
  int32_t init_dims;
  float init_range;
  uint64_t init_seed;
} rec_multislot_desc;
int rec_multislot_sumpool_fwd(const rec_multislot_desc* desc, const int64_t* values, const int64_t* lod,
                              const int64_t* slot_base, const float* W, float* out, int32_t* counts,
                              int32_t* seg_of_value, int64_t* rows_out, int32_t* status, void* stream);
/* The backward of the pool in ROWS FORM — the SelectedRows value of sequence_pool('sum') o sparse_embedding
 * (slot_dnn/net.py:63-75): row_grad[k, :] = d_out[b, s*D:(s+1)*D] for value k of segment seg_of_value[k] = b*S+s
 * (rows = rows_out of the forward).  For binders that must hand the gradient over as a dense [nnz, D] tensor (the
 * Paddle custom operator rec_multislot_sumpool); the engine's own steps read d_out through rec_grad_layout.index
 * and never materialise it.  desc: batch, num_slots, emb_dim, out_stride are read. */
int rec_multislot_sumpool_bwd(const rec_multislot_desc* desc, int64_t nnz, const int32_t* seg_of_value,
                              const float* d_out, float* row_grad, void* stream);
/* Row of a feasign in a hashed table of num_rows (>= 2) rows: 0 -> 0 (padding row), f -> 1 + mix64(f) %
 * (num_rows - 1) with mix64 = the murmur3 64-bit finaliser (SURVEY §8(d) cfg5 "64-bit mix % N").  Device
 * (keys/rows device pointers) and host variants, bit-identical. */
int rec_feasign_rows(int64_t n, int64_t num_rows, const int64_t* keys, int64_t* rows, void* stream);
int rec_feasign_rows_host(int64_t n, int64_t num_rows, const uint64_t* keys, int64_t* rows);

/* ------------------------------------------------------------------------------------------
 * SelectedRows merge (MergeAdd [EXT]) — integer part: group the n = B*S lookups by row.
 * Replaces the duplicate-row merge every consumer of a sparse=True embedding gradient performs
 * (deepfm/net.py:62-70,80 `sparse=use_sparse`).
 *   sorted_pos [n] i32 : positions (b*S+s) stably sorted by row; padding hits are dropped
 *   uniq_rows  [n] i64 : first n_uniq entries = distinct rows, ascending
 *   seg_offset [n+1] i32: sorted_pos[seg_offset[u] .. seg_offset[u+1]) belong to uniq_rows[u]
 *   n_uniq     [4] i32 : {number of distinct rows, number of non-padding positions, 1 if some row owns >=
 *                         REC_SEG_LONG positions else 0, 0}
 * All four are bit-exact targets.
 * ---------------------------------------------------------------------------------------- */
int rec_ids_group_workspace_bytes(int64_t n, int64_t num_rows, size_t* bytes);
int rec_ids_group(int64_t n, int32_t num_slots, int64_t num_rows, int64_t padding_idx,
                  const int64_t* ids, const int64_t* slot_offset, int32_t* sorted_pos,
                  int64_t* uniq_rows, int32_t* seg_offset, int32_t* n_uniq, int32_t* status,
                  void* workspace, size_t workspace_bytes, void* stream);
/* The same grouping with a caller-chosen 32-bit payload travelling with every lookup instead of its position:
 * sorted_pos[k] = payload[position].  The multi-slot CSR path (slot_dnn/net.py:63-75) passes the (sample, slot)
 * segment of every value (rec_multislot_sumpool_fwd's seg_of_value), so the row-update kernels find a position's
 * gradient row without the random read of rec_grad_layout.index that sorting positions would need (22.7 M
 * 4-byte reads, a memory line each, on the slot_dnn benchmark shape).  Stable in the positions, as above. */
int rec_ids_group_payload(int64_t n, int32_t num_slots, int64_t num_rows, int64_t padding_idx,
                          const int64_t* ids, const int64_t* slot_offset, const int32_t* payload,
                          int32_t* sorted_pos, int64_t* uniq_rows, int32_t* seg_offset, int32_t* n_uniq,
                          int32_t* status, void* workspace, size_t workspace_bytes, void* stream);
/* Host query (touches no device): the radix-sort plan rec_ids_group / rec_ids_group_payload — and the general path of
 * rec_ids_group_slots, with n = batch * num_slots and num_rows = num_slots * slot_rows — run for n lookups of a
 * num_rows-row table in this process.  The plan depends on sizes (key width of num_rows, 4 Mi / 8 Mi lookup thresholds)
 * and on the process environment (REC_RSORT_DIGIT, REC_RSORT_PACK, REC_GROUP_DROP, read once); the entry points execute
 * exactly what this reports, so a test that means one path asserts it here instead of trusting its shape.  n == 0:
 * nothing is sorted, passes = 0. */
typedef struct {
  int32_t passes;    /* LSD passes over the key (keys take the values 0 .. num_rows; num_rows = the dropped lookups) */
  int32_t bits[8];   /* digit width of pass i, least significant digit first; 0 behind the last pass */
  int32_t waves;     /* waves per block: 4 (tiles of 2048 lookups) or 16 (tiles of 8192) */
  int32_t key_bytes; /* 4: uint32_t keys (num_rows < 0xFFFFFFFF), 8: uint64_t keys */
  int32_t packed;    /* 1: the intermediate passes move packed (key, value) pairs and alias the key buffers */
  int32_t drop;      /* 1: padding / out-of-range lookups leave the sort after its first pass */
} rec_ids_group_plan_t;
int rec_ids_group_plan(int64_t n, int64_t num_rows, rec_ids_group_plan_t* out);

/* The same grouping for a [batch, num_slots] id batch whose slot s owns rows [s * slot_rows, (s + 1) * slot_rows) of the
 * table (BASELINE configs[1]: 26 tables x 1 000 000 rows as one table; deepfm/net.py:62-86 with one nn.Embedding per
 * slot) — i.e. rec_ids_group with slot_offset[s] = s * slot_rows and num_rows = num_slots * slot_rows, bit-identical
 * outputs, except that an id outside [0, slot_rows) is flagged REC_FLAG_INDEX_OOB and dropped (with separate tables it
 * IS out of range).  The slot digit of the key is free (column s of the batch is slot s), so the sort is num_slots
 * independent two-digit sorts inside L2-resident 256 KB slices: 7 launches instead of 13 (csrc/ids_group_slots.hip);
 * shapes that path does not cover (batch < 8192, slot_rows > 2^20, num_slots > 60) take the general sort.
 *   rank [batch*num_slots] i32 or NULL: rank[pos] = k with sorted_pos[k] = pos, -1 for dropped lookups — where a
 *   producer writes the gradient row of lookup pos so that the gradient buffer is in sorted order
 *   (rec_grad_layout.sorted). */
int rec_ids_group_slots_workspace_bytes(int64_t batch, int32_t num_slots, int64_t slot_rows, size_t* bytes);
int rec_ids_group_slots(int64_t batch, int32_t num_slots, int64_t slot_rows, int64_t padding_idx, const int64_t* ids,
                        int32_t* sorted_pos, int64_t* uniq_rows, int32_t* seg_offset, int32_t* n_uniq, int32_t* rank,
                        int32_t* status, void* workspace, size_t workspace_bytes, void* stream);
/* rank of any grouping whose sorted_pos holds positions (no payload): rank[0, n) = -1, then rank[sorted_pos[k]] = k for
 * k < n_uniq[1]. */
int rec_ids_rank(int64_t n, const int32_t* n_uniq, const int32_t* sorted_pos, int32_t* rank, void* stream);

/* ------------------------------------------------------------------------------------------
 * Optimizers.  paddle.optimizer.Adam [EXT] (deepfm/dygraph_model.py:61-65, static_model.py:83-84):
 *   lr_t = lr*sqrt(1-b2^t)/(1-b1^t);  m = b1*m+(1-b1)*g;  v = b2*v+(1-b2)*g*g;
 *   p -= lr_t * m / (sqrt(v) + eps*sqrt(1-b2^t))
 * ---------------------------------------------------------------------------------------- */
typedef struct {
  float lr, beta1, beta2, eps;
  int64_t step; /* t, 1-based */
} rec_adam_hyper;

/* Where the gradient row of lookup position `pos` (= b*S+s) lives inside `grad`:
 *   p = index ? index[pos] : pos;  q = p / div;
 *   offset = group > 0 ? (q / group) * group_stride + (q % group) * D : q * D
 * {1,0,0}: contiguous [n,D] (DeepFM row_grad); {S,0,0} with D = 1: dy1 [B] for the first-order table;
 * {1,S,d}: the first S*D columns of a [B,d] feature gradient (DCN-v2);
 * index = seg_of_value of rec_multislot_sumpool_fwd: every id of a pooled (sample, slot) segment reads the ONE
 * gradient row of that segment, d_out[b, s*D:(s+1)*D] — the backward of sequence_pool('sum') without a
 * materialised [nnz, D] row-gradient tensor (slot_dnn/net.py:73). */
typedef struct {
  int32_t div;
  int32_t group;
  int64_t group_stride;
  const float* partials; /* device, from rec_segment_partials for THIS grad + grouping, or NULL */
  const int32_t* index;  /* device [n] or NULL: lookup position -> gradient position */
  int32_t sorted;        /* 1: grad is [n, D] in SORTED order — row k belongs to sorted position k (written through
                          * the rank of rec_ids_group_slots / rec_ids_rank, e.g. by rec_deepfm_fm_bwd_sorted); div,
                          * group, group_stride and index are then ignored.  A row's duplicate gradients are
                          * consecutive rows: the update kernels stream them instead of chasing sorted_pos. */
} rec_grad_layout;

/* Hot rows.  With Zipf-distributed ids one row can own tens of thousands of the n lookups; the per-row
 * duplicate sum of the consumers below would then be a serial chain of that many reads.  rec_segment_partials
 * pre-reduces, per tile of REC_SEG_TILE sorted positions, the pieces of every segment of >= REC_SEG_LONG
 * positions into partials [ceil(n_max/REC_SEG_TILE), 2, emb_dim] (fixed summation tree: deterministic); a
 * consumer given grad_layout.partials adds one partial per tile for such rows.  Optional: with partials =
 * NULL every consumer sums position by position.  grad_layout->partials is ignored on input here. */
#define REC_SEG_TILE 64
#define REC_SEG_LONG 128
int rec_segment_partials_bytes(int64_t n_max, int32_t emb_dim, size_t* bytes);
int rec_segment_partials(int64_t n_max, int32_t emb_dim, const int32_t* n_uniq,
                         const int32_t* seg_offset, const int32_t* sorted_pos, const float* grad,
                         const rec_grad_layout* grad_layout, float* partials, void* stream);

/* lazy_mode=True Adam on the rows of a merged SelectedRows gradient, merge fused in:
 *   g[u,:] = sum_{k in seg(u)} grad_row(sorted_pos[k])            (ascending position order)
 * then Adam on rows uniq_rows[u] of P/M/V ([num_rows,row_stride]).  n_uniq is read on the device.
 * grad_layout NULL = {1,0,0}.  grad_scale (device float[1] or NULL): factor applied to the merged
 * gradient — the global-norm clipping coefficient of rec_clip_scale. */
int rec_sparse_adam_rows(int64_t n_max, int32_t emb_dim, int32_t row_stride,
                         int32_t state_stride /* row stride of M and V; 0 = row_stride */,
                         const int32_t* n_uniq, const int64_t* uniq_rows, const int32_t* seg_offset,
                         const int32_t* sorted_pos, const float* grad,
                         const rec_grad_layout* grad_layout, const float* grad_scale, float* P,
                         float* M, float* V, const rec_adam_hyper* hyper, void* stream);

/* The same with paddle.regularizer.L2Decay(l2_coeff) on the parameter: the merged (and scaled) gradient of a touched row
 * becomes g + l2_coeff * w before Adam.  l2_coeff == 0 runs the kernels of rec_sparse_adam_rows. */
int rec_sparse_adam_rows_l2(int64_t n_max, int32_t emb_dim, int32_t row_stride, int32_t state_stride,
                            const int32_t* n_uniq, const int64_t* uniq_rows, const int32_t* seg_offset,
                            const int32_t* sorted_pos, const float* grad, const rec_grad_layout* grad_layout,
                            const float* grad_scale, float* P, float* M, float* V, const rec_adam_hyper* hyper,
                            float l2_coeff, void* stream);

/* Both embeddings of a DeepFM row (deepfm/net.py:62-86: `embedding` [N,D] and `embedding_one` [N,1]) in one
 * pass over the record layout  rec [N, rec_stride] = W(D) | W1 | m1 | v1 | pad,  MV [N, state_stride] = m(D) at
 * 0 | v(D) at v_offset:  W/m/v from (grad, grad_layout), W1/m1/v1 from (grad1, grad1_layout) — for DeepFM
 * grad1 = dz [B] with layout {S,0,0}.  Same arithmetic as two rec_sparse_adam_rows calls; one record line and
 * one state line are read and written per touched row instead of the record line twice. */
int rec_sparse_adam_record(int64_t n_max, int32_t emb_dim, int32_t rec_stride, int32_t state_stride,
                           int32_t v_offset, const int32_t* n_uniq, const int64_t* uniq_rows,
                           const int32_t* seg_offset, const int32_t* sorted_pos, const float* grad,
                           const rec_grad_layout* grad_layout, const float* grad1,
                           const rec_grad_layout* grad1_layout, const float* grad_scale, float* rec,
                           float* MV, const rec_adam_hyper* hyper, void* stream);

/* PS / gpubox accessor rule — "SparseAdaGradSGDRule" + show/click counters (models/rank/slot_dnn/
 * config_online.yaml:57-79; dnn/net.py:71-79 feature value [show, click, embed_w, embedx(D-1)];
 * formula per SURVEY.md App. B-13 [EXT]: the rule itself lives in the un-vendored Paddle PS code):
 *   scale = sqrt(initial_g2sum / (initial_g2sum + g2sum));  w = clip(w - lr*g*scale, bounds);
 *   g2sum += mean(g^2) per part (embed_w = first weight, embedx = the other D-1);
 *   show += lookups of the row in this batch, click += sum of their labels (label [B] i64 or NULL).
 * rec: record table [num_rows, row_stride], row = [show | click | g2sum_w | g2sum_x | W(D) | pad];
 * the lookup table of rec_emb_gather / rec_emb_gather_sumpool is W = rec + 4 with the same stride
 * (continuous_value_model(use_cvm=False) = "return the embedding without the CVM columns").  num_slots maps a lookup
 * position to its sample (b = pos / num_slots) for the click counter. */
typedef struct {
  float lr, initial_g2sum, min_bound, max_bound;
} rec_adagrad_hyper;
int rec_sparse_adagrad_rows(int64_t n_max, int32_t emb_dim, int32_t row_stride, int32_t num_slots,
                            const int32_t* n_uniq, const int64_t* uniq_rows,
                            const int32_t* seg_offset, const int32_t* sorted_pos, const float* grad,
                            const rec_grad_layout* grad_layout, const int64_t* label, float* rec,
                            const rec_adagrad_hyper* hyper, void* stream);

/* ------------------------------------------------------------------------------------------
 * The full table accessor of the PS / gpubox mode (slot_dnn/config_online.yaml:57-89: SparseAccessor with
 * embedx_threshold, SparseAdaGradSGDRule for embed_w and embedx, ctr_accessor_param; slot_dnn/net.py:61-62
 * ShowClickEntry; tools/static_gpubox_trainer.py:152-160).  The arithmetic follows the published source of
 * PaddlePaddle release/2.4 [EXT] — paddle/fluid/distributed/ps/table/{sparse_sgd_rule.cc, ctr_accessor.cc,
 * memory_sparse_table.cc} and framework/fleet/heter_ps/optimizer.cuh.h — quoted in oracle/ps_ref.py.
 * A feature value lives in one record row; the layout says where its parts are (floats from the row start), so
 * DeepFM (embedx = the 16-dim embedding at 0, embed_w = the first-order weight behind it) and slot_dnn
 * (W = [embed_w, embedx(8)]) use the same kernels:
 *   stat_off: show, click, embed_g2sum, embedx_g2sum, state, delta_score, unseen_days   (7 consecutive floats;
 *             state 0 = no such key (zeroed memory: reads as embed_w = 0, embedx = 0, what PullSparse returns
 *             for a missing key), 1 = value without its embedx part, 2 = embedx exists)
 * rec_ps_push_rows = MemorySparseTable::PushSparse + CtrCommonAccessor::Update on the touched rows (merge of
 *   duplicate gradients fused in, ascending position order): a new key is created without embedx (embed_w = 0 when
 *   embed_zero_init, else uniform(+-initial_range)); show / click / delta_score / unseen_days; then
 *   SparseAdaGradSGDRule::UpdateValueWork on embed_w and (if it exists) embedx:
 *       float pushed = g * grad_scale;  double scaled = pushed / (show_scale ? pushed_show : 1)   [a FLOAT division, as
 *       `double scaled_grad = grad[i] / scale;` over `const float* grad`, `float scale` is];
 *       w = clip(float(w - lr * scaled * sqrtf(g0 / (g0 + g2sum))));  g2sum = float(g2sum + sum(scaled^2) / n)
 *   a value without embedx drops its embedx gradient and is extended (uniform(+-x_initial_range), a pure function
 *   of (seed,row,element); embedx_g2sum = 0) at the end of the push after which
 *   (show-click)*nonclk_coeff + click*click_coeff >= embedx_threshold (NeedExtendMF on the updated counters).
 *   show / click: per-SAMPLE int64 [B] (NULL: 1 per occurrence / 0); num_slots maps a lookup position to its
 *   sample.
 * rec_ps_shrink_rows = CtrCommonAccessor::Shrink over the table: counters decay, values whose score fell below
 *   delete_threshold or with unseen_days > delete_after_unseen_days are zeroed (the key is gone); n_deleted
 *   (device int64 or NULL) counts them.
 * rec_ps_save_select = Save(value, param) + UpdateStatAfterSave(value, param) for every row: selected[row]
 *   (device bytes or NULL) = 1 if a save of kind param writes the value — 0: all; 1 (delta) / 2 (base): score >=
 *   base_threshold && delta_score >= delta_threshold (0 for base) && unseen_days <= delta_keep_days, delta_score of
 *   the selected values reset; 3: all, and unseen_days += 1 (a day passes).
 * ---------------------------------------------------------------------------------------- */
typedef struct {
  float lr, initial_g2sum, min_bound, max_bound, initial_range;           /* embed_sgd_param  (embed_w)  */
  float x_lr, x_initial_g2sum, x_min_bound, x_max_bound, x_initial_range; /* embedx_sgd_param (embedx)   */
  float embedx_threshold, nonclk_coeff, click_coeff;
  float grad_scale;        /* pushed gradient = merged gradient * grad_scale (Paddle pushes the gradient of the SUMMED
                              loss: scale_sparse_gradient_with_batch_size / PushCopy's `* bs`); 1 = as given */
  int32_t show_scale;      /* 1 (Paddle's default): the rule divides the pushed gradient by the pushed show */
  int32_t embed_zero_init; /* 1 (Paddle's default): embed_w of a new value is 0; 0: uniform(+-initial_range) */
  uint64_t seed;
  int64_t row_mul, row_add; /* identity of table row r in the creation values: r * row_mul + row_add (a shard
                               passes {world, rank}: a feature is born with the same values however the table
                               is sharded); {1, 0} for an unsharded table */
} rec_ps_accessor;
typedef struct {
  int32_t row_stride, embed_off, embedx_off, embedx_dim, stat_off;
} rec_ps_layout;
typedef struct {
  const float* grad;       /* element (pos, c) at grad + offset(layout, pos, pitch) + col + c */
  rec_grad_layout layout;
  int32_t pitch;           /* the D of rec_grad_layout's offset formula for this source */
  int32_t col;
} rec_grad_src;
int rec_ps_push_rows(int64_t n_max, int32_t num_slots, const rec_ps_layout* layout, const int32_t* n_uniq,
                     const int64_t* uniq_rows, const int32_t* seg_offset, const int32_t* sorted_pos,
                     const rec_grad_src* grad_embedx, const rec_grad_src* grad_embed, const int64_t* show,
                     const int64_t* click, float* rec, const rec_ps_accessor* accessor, void* stream);
/* host: the creation value of element `element` (0 = embed_w, 1+j = embedx[j]) of feature `row` */
float rec_ps_init_value_host(uint64_t seed, int64_t row, int32_t element, float initial_range);
int rec_ps_shrink_rows(int64_t num_rows, const rec_ps_layout* layout, float* rec, float show_click_decay_rate,
                       float delete_threshold, float delete_after_unseen_days, const rec_ps_accessor* accessor,
                       int64_t* n_deleted, void* stream);
int rec_ps_save_select(int64_t num_rows, const rec_ps_layout* layout, float* rec, int32_t param,
                       float base_threshold, float delta_threshold, float delta_keep_days,
                       const rec_ps_accessor* accessor, uint8_t* selected, int64_t* n_selected, void* stream);

/* ------------------------------------------------------------------------------------------
 * Backward of a ONE-logit head Linear(n -> 1) behind a ReLU (deepfm/net.py:169-174 and the sibling CTR MLPs), in one
 * HBM-bound pass over the [batch, n] activation instead of a K = 1 dX GEMM plus a three-launch skinny dW path:
 *   dx[b,j] = (relu == 0 || act[b,j] > 0) ? dz[b] * w[j] : 0;   dw[j] = sum_b act[b,j] * dz[b];   db[0] = sum_b dz[b]
 * Fixed summation order (deterministic).  n % 4 == 0, n <= 512, 16-byte aligned rows.
 * ---------------------------------------------------------------------------------------- */
int rec_mlp_head_bwd_workspace_bytes(int64_t batch, int32_t n, size_t* bytes);
int rec_mlp_head_bwd(int64_t batch, int32_t n, const float* act, int64_t ld_act, const float* dz, const float* w,
                     int32_t relu, float* dx, int64_t ld_dx, float* dw, float* db, void* workspace,
                     size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * Train-mode Dropout and L2Decay of the DCN-v2 DNN tower (dcn_v2/net.py:158,164-170,181-183).
 * rec_dropout: out[r,c] = keep ? in[r,c] / (1-p)^nmask : 0 over a [rows, cols] matrix (row strides ld_in / ld_out,
 *   in place allowed).  keep is a pure function of (seed, stream id, r*cols + c) — no stored mask: the backward is the
 *   same call on the gradient.  nmask 2 applies streams a AND b at once (the reference's two dropouts around a ReLU).
 * rec_l2_decay_grad: grad += (coeff / grad_scale[0]) * w — L2Decay appended AFTER global-norm clipping [EXT]; the
 *   Adam kernels multiply the whole gradient by the clipping coefficient, hence the pre-division (grad_scale NULL: 1).
 * ---------------------------------------------------------------------------------------- */
int rec_dropout(int64_t rows, int32_t cols, int64_t ld_in, int64_t ld_out, const float* in, float* out, float p,
                uint64_t seed, uint64_t stream_a, uint64_t stream_b, int32_t nmask, void* stream);
int rec_l2_decay_grad(int64_t n, float* grad, const float* w, float coeff, const float* grad_scale, void* stream);

/* paddle.optimizer.SGD [EXT] (din/dygraph_model.py:64-73): p -= lr * g.  Rows whose gradient is zero do
 * not move, so updating the merged rows of a SelectedRows gradient equals the dense update. */
int rec_sparse_sgd_rows(int64_t n_max, int32_t emb_dim, int32_t row_stride, const int32_t* n_uniq,
                        const int64_t* uniq_rows, const int32_t* seg_offset, const int32_t* sorted_pos,
                        const float* grad, const rec_grad_layout* grad_layout, float* P, float lr,
                        void* stream);
int rec_sgd_dense(int64_t n, float* p, const float* g, float lr, void* stream);
/* The merge and the SGD row update of a SMALL SelectedRows gradient in one launch (n <= 15360 lookups,
 * emb_dim <= 256): at the reference's own batch size (din/config.yaml: batch_size 32, ~5 k lookups per table) the
 * sort-based rec_ids_group + rec_segment_partials + rec_sparse_sgd_rows are 12-13 launches per table whose launch
 * latency, not work, is the step time.  A wave per lookup finds the occurrences of its row with ballots over the id
 * list; the first occurrence's wave adds the gradient rows in ascending position (the SelectedRows merge order)
 * and applies p -= lr * g.  ids [n] i64 rows (padding_idx < 0: none); out-of-range ids are skipped and flagged in
 * status; grad / grad_layout as for rec_sparse_sgd_rows (partials ignored). */
int rec_sparse_sgd_small(int64_t n, int32_t emb_dim, int32_t row_stride, int64_t num_rows, int64_t padding_idx,
                         const int64_t* ids, const float* grad, const rec_grad_layout* grad_layout, float* P,
                         float lr, int32_t* status, void* stream);
/* The same for up to 8 tables in ONE launch (DIN updates seven embedding tables per step, din/dygraph_model.py:64-73:
 * independent of each other, so their merges share the chip instead of running one after the other). */
typedef struct {
  int64_t n;              /* lookups of this table (<= 15360) */
  int32_t emb_dim, row_stride;
  int64_t num_rows, padding_idx;
  const int64_t* ids;     /* [n] rows */
  const float* grad;
  rec_grad_layout grad_layout;
  float* P;
} rec_small_sgd_job;
int rec_sparse_sgd_small_multi(int32_t count, const rec_small_sgd_job* jobs, float lr, int32_t* status, void* stream);
/* The same one-launch merge with the lazy Adam update of BOTH embeddings of a DeepFM record (the arithmetic of
 * rec_sparse_adam_record: W, m, v and W1, m1, v1 of a touched row in one pass) — the reference's bigdata batch size
 * (deepfm/config_bigdata.yaml: 512 x 26 slots = 13312 lookups) replaces grouping sort + two partial passes + record
 * update, 12 launches, by one.  ids [n] (n = B * num_slots, row = id + slot_offset[pos % num_slots] when
 * slot_offset is given); grad: one emb_dim-wide row per position (grad_layout as rec_sparse_adam_record), grad1:
 * the first-order gradient source with its layout (dz with {div = num_slots}).
 * Above 2048 lookups, ONE table (or slot tables of rows <= 16 floats) is merged by ROW BUCKETS: block b owns the rows
 * hashing to bucket b and keeps their (row, position) pairs in ascending position — the same order of additions, the
 * same bits, without comparing every lookup with every other (the reference's one shared table: 98 -> 21 us). */
int rec_sparse_adam_record_small(int64_t n, int32_t num_slots, int32_t emb_dim, int32_t rec_stride,
                                 int32_t state_stride, int32_t v_offset, int64_t num_rows, int64_t padding_idx,
                                 const int64_t* ids, const int64_t* slot_offset, const float* grad,
                                 const rec_grad_layout* grad_layout, const float* grad1,
                                 const rec_grad_layout* grad1_layout, const float* grad_scale, float* rec, float* MV,
                                 const rec_adam_hyper* hyper, int32_t* status, int32_t* scratch, void* stream);
/* scratch: one device int32 of the caller's (may be NULL).  With it ONE block decides for the whole launch whether every
 * id stays inside its slot's span of rows (then a lookup is only compared with the lookups of its own slot); without it
 * every block of the launch reads the whole id list to take that decision itself. */

/* lazy_mode=False Adam on a SelectedRows gradient — the dygraph default (deepfm/dygraph_model.py:61-65,
 * SURVEY.md App. B-3): every one of the num_rows rows is updated, rows absent from the merged gradient with
 * g = 0.  Same arguments as rec_sparse_adam_rows; streams the whole table (6*N*D*4 B per step). */
int rec_adam_rows_all(int64_t num_rows, int32_t emb_dim, int32_t row_stride, int32_t state_stride,
                      const int32_t* n_uniq, const int64_t* uniq_rows, const int32_t* seg_offset,
                      const int32_t* sorted_pos, const float* grad, const rec_grad_layout* grad_layout,
                      const float* grad_scale, float* P, float* M, float* V, const rec_adam_hyper* hyper,
                      void* stream);

/* The same with L2Decay(l2_coeff): every row moves with g + l2_coeff * w (g = 0 for rows absent from the gradient).
 * l2_coeff == 0 runs the kernels of rec_adam_rows_all. */
int rec_adam_rows_all_l2(int64_t num_rows, int32_t emb_dim, int32_t row_stride, int32_t state_stride,
                         const int32_t* n_uniq, const int64_t* uniq_rows, const int32_t* seg_offset,
                         const int32_t* sorted_pos, const float* grad, const rec_grad_layout* grad_layout,
                         const float* grad_scale, float* P, float* M, float* V, const rec_adam_hyper* hyper,
                         float l2_coeff, void* stream);

/* The same on the record layout of rec_sparse_adam_record (rec = W(D) | W1 | m1 | v1 | pad, MV = m(D) | v(D) at v_offset):
 * both embeddings of every row in ONE pass — 512 B per row where two rec_adam_rows_all passes move 768 (the second
 * one reads and writes the whole record line for W1 / m1 / v1).  Same arithmetic and summation order: bit-identical. */
int rec_adam_record_all(int64_t num_rows, int32_t emb_dim, int32_t rec_stride, int32_t state_stride,
                        int32_t v_offset, const int32_t* n_uniq, const int64_t* uniq_rows,
                        const int32_t* seg_offset, const int32_t* sorted_pos, const float* grad,
                        const rec_grad_layout* grad_layout, const float* grad1,
                        const rec_grad_layout* grad1_layout, const float* grad_scale, float* rec, float* MV,
                        const rec_adam_hyper* hyper, void* stream);

/* dense Adam over a flat buffer (MLP + FM dense weights); grad_scale as above. */
int rec_adam_dense(int64_t n, float* p, float* m, float* v, const float* g, const float* grad_scale,
                   const rec_adam_hyper* hyper, void* stream);

/* paddle.nn.ClipGradByGlobalNorm(clip_norm) [EXT] (dcn_v2/dygraph_model.py:81-88):
 *   global_norm = sqrt(sum over ALL gradients of g^2);  every g *= clip_norm / max(global_norm, clip_norm).
 * rec_sumsq: out[0] (+)= sum x^2 over a dense buffer; rec_sparse_rows_sumsq: the same over the MERGED
 * rows of a SelectedRows gradient (duplicates summed first, as Paddle's merge does); both reduce in a
 * fixed order.  rec_clip_scale turns the total into the device scalar the Adam kernels take. */
int rec_sumsq_workspace_bytes(size_t* bytes);
int rec_sumsq(int64_t n, const float* x, float* out, int32_t accumulate, void* workspace,
              size_t workspace_bytes, void* stream);
int rec_sparse_rows_sumsq(int64_t n_max, int32_t emb_dim, const int32_t* n_uniq,
                          const int32_t* seg_offset, const int32_t* sorted_pos, const float* grad,
                          const rec_grad_layout* grad_layout, float* out, int32_t accumulate,
                          void* workspace, size_t workspace_bytes, void* stream);
int rec_clip_scale(const float* sumsq, float clip_norm, float* scale, void* stream);

/* CrossNetV2 backward glue (dcn_v2/net.py:222-226), one streaming pass:
 *   dU = dX * X0;   dX0_acc = (accumulate ? dX0_acc : 0) + dX * U       (all [m,n] with row strides) */
int rec_cross_bwd_prep(int64_t m, int32_t n, const float* dX, int32_t ld_dx, const float* X0,
                       int32_t ld_x0, const float* U, int32_t ld_u, float* dU, int32_t ld_du,
                       float* dX0_acc, int32_t ld_acc, int32_t accumulate, void* stream);

/* ------------------------------------------------------------------------------------------
 * DIN attention-pool, fused: 4 lookups -> [h, q, h-q, h*q] -> Linear/Sigmoid x2 -> Linear -> + mask ->
 * * E^-0.5 -> softmax over T -> weights @ h.   Replaces din/net.py:141-173; the [B,T,4E] concat and the
 * hidden activations never reach HBM (one block per sample, 32-position tiles, online softmax).
 *   hist_item/hist_cat/tgt_item_seq/tgt_cat_seq [B,T] i64 (no padding_idx: id 0 is a real row, App. B-11)
 *   mask [B,T] i64: 0 valid, -1e9 padding (din/dinReader.py:81-84,99)
 *   tables f32 [rows, stride]; hist and target tables are independent parameters (App. C)
 *   att_w1 [4E,H1] (Paddle [in,out]), att_b1 [H1], att_w2 [H1,H2], att_b2 [H2], att_w3 [H2], att_b3 [1]
 *   out [B,E];  att_weight [B,T] or NULL: the softmax weights (saved for the backward)
 * ---------------------------------------------------------------------------------------- */
typedef struct {
  int64_t batch;      /* B */
  int32_t max_len;    /* T (padded history length of this batch) */
  int32_t item_dim, cat_dim;   /* E = item_dim + cat_dim <= 256, both multiples of 4 */
  int32_t hidden1, hidden2;    /* 80, 40 */
  int64_t item_rows, cat_rows;
  int32_t item_stride, cat_stride;
} rec_din_desc;

/* act1 [B,T,H1] or NULL: layer-1 activations for the backward.  Written only when rec_din_saves_act1(desc)
 * returns 1 (the reference net's own shape: E 128, attention MLP 80-40-1); otherwise left untouched and the
 * backward must be given NULL for act1_saved. */
int rec_din_saves_act1(const rec_din_desc* desc);
int rec_din_attention_pool_fwd(const rec_din_desc* desc, const int64_t* hist_item,
                               const int64_t* hist_cat, const int64_t* tgt_item_seq,
                               const int64_t* tgt_cat_seq, const int64_t* mask,
                               const float* w_hist_item, const float* w_hist_cat,
                               const float* w_tgt_item_seq, const float* w_tgt_cat_seq,
                               const float* att_w1, const float* att_b1, const float* att_w2,
                               const float* att_b2, const float* att_w3, const float* att_b3,
                               float* out, float* att_weight, float* act1, int32_t* status, void* stream);
/* The same forward with a caller-owned workspace (rec_din_attention_pool_fwd_workspace_bytes; 0 bytes = the shape
 * never needs one; when the query is not 0, a missing or smaller workspace is REC_EWORKSPACE before any launch — a caller
 * without a workspace calls rec_din_attention_pool_fwd).  With it, a batch of FEW samples (the reference's din/config.yaml batch size 32: fewer samples than
 * the chip has block slots) is computed one block per 32-position history tile — each tile softmax-normalised on its
 * own, a second launch rescales the pieces to the softmax over the whole history — instead of one block per sample
 * walking its tiles one after the other (82 -> ~25 us at 32 x 152).  Same results up to fp32 rounding of the
 * softmax's normalisation order. */
int rec_din_attention_pool_fwd_workspace_bytes(const rec_din_desc* desc, size_t* bytes);
int rec_din_attention_pool_fwd_ws(const rec_din_desc* desc, const int64_t* hist_item,
                                  const int64_t* hist_cat, const int64_t* tgt_item_seq,
                                  const int64_t* tgt_cat_seq, const int64_t* mask,
                                  const float* w_hist_item, const float* w_hist_cat,
                                  const float* w_tgt_item_seq, const float* w_tgt_cat_seq,
                                  const float* att_w1, const float* att_b1, const float* att_w2,
                                  const float* att_b2, const float* att_w3, const float* att_b3,
                                  float* out, float* att_weight, float* act1, int32_t* status, void* workspace,
                                  size_t workspace_bytes, void* stream);

/* Backward of the block above w.r.t. the gathered rows (what loss.backward() computes for net.py:141-173):
 *   d_hist [B,T,E] = gradient of [hist_item_emb | hist_cat_emb] per position, d_tgt_seq [B,T,E] likewise
 *   for the target-seq tables; their row-wise merge (rec_ids_group + rec_sparse_sgd_rows) is the
 *   embedding gradient.  att_weight = the forward's softmax weights; att_w1_t = att_w1 transposed
 *   [H1,4E].  out_saved [B,E] / act1_saved [B,T,H1] (both nullable): the forward's output and the layer-1
 *   activations it wrote when its `act1` argument was non-null and rec_din_saves_act1(desc) == 1 (NULL here
 *   otherwise).  With both, the backward runs on the saved activations (dz1 W1^T on the matrix cores, W1^T in
 *   registers); without, hidden activations are recomputed.  The attention MLP's own weight gradients are not
 *   produced (not registered parameters in dygraph mode). */
int rec_din_attention_pool_bwd(const rec_din_desc* desc, const int64_t* hist_item,
                               const int64_t* hist_cat, const int64_t* tgt_item_seq,
                               const int64_t* tgt_cat_seq, const float* w_hist_item,
                               const float* w_hist_cat, const float* w_tgt_item_seq,
                               const float* w_tgt_cat_seq, const float* att_w1,
                               const float* att_w1_t, const float* att_b1, const float* att_w2,
                               const float* att_b2, const float* att_w3, const float* att_weight,
                               const float* out_saved, const float* act1_saved,
                               const float* d_out, float* d_hist, float* d_tgt_seq, void* stream);

/* The same backward with a caller-owned workspace (rec_din_attention_pool_bwd_workspace_bytes; 0 bytes = the shape never
 * needs one; otherwise a missing or smaller workspace is REC_EWORKSPACE before any launch, and a caller without one
 * calls rec_din_attention_pool_bwd): at batches larger than the resident grid the blocks of the saved-activation kernel draw their next SAMPLE
 * from a ticket counter in it instead of walking fixed ranges — samples cost between one and max_len / 32 tiles once
 * tiles whose saved weights are all zero are skipped.  Same results: which block computes a tile changes nothing. */
int rec_din_attention_pool_bwd_workspace_bytes(const rec_din_desc* desc, size_t* bytes);
int rec_din_attention_pool_bwd_ws(const rec_din_desc* desc, const int64_t* hist_item,
                                  const int64_t* hist_cat, const int64_t* tgt_item_seq,
                                  const int64_t* tgt_cat_seq, const float* w_hist_item,
                                  const float* w_hist_cat, const float* w_tgt_item_seq,
                                  const float* w_tgt_cat_seq, const float* att_w1,
                                  const float* att_w1_t, const float* att_b1, const float* att_w2,
                                  const float* att_b2, const float* att_w3, const float* att_weight,
                                  const float* out_saved, const float* act1_saved,
                                  const float* d_out, float* d_hist, float* d_tgt_seq, void* workspace,
                                  size_t workspace_bytes, void* stream);

/* CrossNetMix backward glue for one expert (dcn_v2/net.py:301-317), one pass over [m,n]:
 *   dU = dX*X0*p_e;  dX0_acc (+)= dX*p_e*U;  dp[i] = sum_j dX*X0*U      (p_e = prob[i*prob_stride])
 * and the softmax backward of the gate: dz = p * (dp - sum_e p_e dp_e) over n <= 64 columns. */
int rec_moe_bwd_prep(int64_t m, int32_t n, const float* dX, int32_t ld_dx, const float* X0,
                     int32_t ld_x0, const float* U, int32_t ld_u, const float* prob, int32_t prob_stride,
                     float* dU, int32_t ld_du, float* dX0_acc, int32_t ld_acc, int32_t accumulate,
                     float* dp, int32_t dp_stride, void* stream);
int rec_softmax_rows_bwd(int64_t m, int32_t n, const float* p, int32_t ldp, const float* dp,
                         int32_t lddp, float* dz, int32_t lddz, void* stream);

/* y[i,:] = softmax(x[i,:]) over n <= 64 columns (CrossNetMix expert gate, dcn_v2/net.py:313-316). */
int rec_softmax_rows(int64_t m, int32_t n, const float* x, int32_t ldx, float* y, int32_t ldy,
                     void* stream);

/* ------------------------------------------------------------------------------------------
 * xDeepFM Compressed Interaction Network (models/rank/xdeepfm/net.py:155-202), the passes around the GEMM.
 * Every X_k (k >= 1) is kept d-major, XT[(b,d), c] (row = b*D + d), so the reference's 1x1 Conv2D over the F*S
 * interaction channels (net.py:176-190) is one row-major GEMM  XT_{k+1} = Z @ Wc^T  with M = B*D, K = F*S, N = C
 * (rec_gemm_f32; Wc^T is the conv weight [C, F*S, 1, 1] viewed [C, F*S], passed with trans_b).
 *   rec_cin_view: element (b, j, d) of a feature tensor sits at base + b*stride_b + j*stride_j + d*stride_d
 *                 floats — feat_embeddings [B,F,D] is {F*D, D, 1}; an XT [B*D, ld] is {D*ld, 1, ld}.
 *   rec_cin_outer_fwd : Z[(b,d), f*S + s] = X0[b,f,d] * Xk[b,s,d]                    net.py:163-175
 *   rec_cin_outer_bwd : dX0[b,f,d] (+)= sum_s dZ[(b,d), f*S+s] Xk[b,s,d]
 *                       dXk[b,s,d] (+)= sum_f dZ[(b,d), f*S+s] X0[b,f,d]  (+ dpool[b,s]: the gradient of the
 *                       sum-pooled features of that layer, every d row gets it).  dX0 and dXk may alias
 *                       (layer 1, Xk = X0: pass both accumulate flags).
 *   rec_cin_sumpool(_bwd): pooled[b,c] = sum_d XT[(b,d), c]  (net.py:195-198) and its broadcast backward.
 * Z for a whole batch is B*D*F*S floats (11.8 GB at B 65536, D 9, 39 x 128): callers walk the batch in chunks.
 * ---------------------------------------------------------------------------------------- */
typedef struct {
  int64_t stride_b;
  int32_t stride_j, stride_d;
} rec_cin_view;

int rec_cin_outer_fwd(int64_t batch, int32_t emb_dim, int32_t F, int32_t S, const float* X0,
                      const rec_cin_view* v0, const float* Xk, const rec_cin_view* vk, float* Z, int64_t ldz,
                      void* stream);
int rec_cin_outer_bwd(int64_t batch, int32_t emb_dim, int32_t F, int32_t S, const float* dZ, int64_t ldz,
                      const float* X0, const rec_cin_view* v0, const float* Xk, const rec_cin_view* vk,
                      float* dX0, const rec_cin_view* dv0, int32_t accumulate_dx0, float* dXk,
                      const rec_cin_view* dvk, int32_t accumulate_dxk, const float* dpool, int64_t ld_dpool,
                      void* stream);
/* The other association of a layer, chosen when C < S (then Y is smaller than Z and its GEMM better shaped):
 *   Y = Xk @ W'^T  with W' = the same conv weight viewed [C*F, S]   (rec_gemm_f32, trans_b; M = B*D, K = S, N = C*F)
 *   rec_cin_contract_fwd : XT_{k+1}[(b,d), c] = sum_f X0[b,f,d] * Y[(b,d), c*F + f]
 *   rec_cin_contract_bwd : dY[(b,d), c*F+f] = dXT[(b,d), c] * X0[b,f,d];  dX0[b,f,d] (+)= sum_c dXT[(b,d),c] Y[(b,d), c*F+f]
 *   (then dW' = dY^T @ Xk and dXk = dY @ W' are plain GEMMs). */
int rec_cin_contract_fwd(int64_t batch, int32_t emb_dim, int32_t F, int32_t C, const float* Y, int64_t ldy,
                         const float* X0, const rec_cin_view* v0, float* XT, int64_t ldx, void* stream);
int rec_cin_contract_bwd(int64_t batch, int32_t emb_dim, int32_t F, int32_t C, const float* Y, int64_t ldy,
                         const float* dXT, int64_t ldx, const float* X0, const rec_cin_view* v0, float* dY,
                         int64_t lddy, float* dX0, const rec_cin_view* dv0, int32_t accumulate_dx0, void* stream);
int rec_cin_sumpool(int64_t batch, int32_t emb_dim, int32_t C, const float* XT, int64_t ldx, float* out,
                    int64_t ldo, void* stream);
int rec_cin_sumpool_bwd(int64_t batch, int32_t emb_dim, int32_t C, const float* dpool, int64_t ldp,
                        float* dXT, int64_t ldx, void* stream);

/* ------------------------------------------------------------------------------------------
 * DLRM (models/rank/dlrm/net.py): BatchNorm1D over the batch, the pairwise dot interaction, accuracy counts.
 *   rec_batchnorm_fwd : nn.BatchNorm1D on X [m, n] (net.py:151-153, after every Linear -> ReLU).  training != 0:
 *                       batch mean and BIASED batch variance, running = momentum*running + (1-momentum)*batch
 *                       (Paddle: momentum 0.9, epsilon 1e-5) [EXT]; training == 0: the running statistics.
 *                       save_mean / save_invstd [n] are kept for the backward.  Column sums in a fixed order.
 *   rec_batchnorm_bwd : dX, dgamma [n], dbeta [n];  relu_mask != 0: X was a ReLU output — dX is zeroed where
 *                       X <= 0 (the ReLU backward folded in), so dX is the gradient of the Linear's output.
 *   rec_dot_interact_fwd : T [batch, F, D] (sample stride ldt) = [emb_1 .. emb_{F-1}, x] ->
 *                       R [batch, D + F(F-1)/2] = [ x | <T_i, T_j> for i < j in row-major order ]   (net.py:96-123:
 *                       bmm + triu + masked_select + concat)
 *   rec_dot_interact_bwd : dT[b,i,:] = sum_{j != i} dZ(i,j) T[b,j,:]  (+ dR[b,:D] for the last field)
 *   rec_accuracy_count : paddle.metric.Accuracy top-1 of softmax(raw) for two classes: counts[0] += #(pred > 0.5
 *                       == label != 0), counts[1] += n   (int64, exact)          dygraph_model.py:58-63,79-81
 * ---------------------------------------------------------------------------------------- */
int rec_batchnorm_workspace_bytes(int64_t m, int32_t n, size_t* bytes);
int rec_batchnorm_fwd(int64_t m, int32_t n, const float* X, int64_t ldx, const float* gamma, const float* beta,
                      float* running_mean, float* running_var, float momentum, float eps, int32_t training,
                      float* Y, int64_t ldy, float* save_mean, float* save_invstd, void* workspace,
                      size_t workspace_bytes, void* stream);
int rec_batchnorm_bwd(int64_t m, int32_t n, const float* X, int64_t ldx, const float* dY, int64_t lddy,
                      const float* gamma, const float* save_mean, const float* save_invstd, int32_t relu_mask,
                      float* dX, int64_t lddx, float* dgamma, float* dbeta, void* workspace,
                      size_t workspace_bytes, void* stream);
int rec_dot_interact_fwd(int64_t batch, int32_t F, int32_t D, const float* T, int64_t ldt, float* R, int64_t ldr,
                         void* stream);
int rec_dot_interact_bwd(int64_t batch, int32_t F, int32_t D, const float* T, int64_t ldt, const float* dR,
                         int64_t ldr, float* dT, int64_t lddt, void* stream);
int rec_accuracy_count(int64_t n, const float* pred, const int64_t* label, int64_t* counts, void* stream);

/* ------------------------------------------------------------------------------------------
 * f32 GEMM on the matrix cores with fused epilogues: C[M,N] = epi(op(A)[M,K] @ op(B)[K,N]).
 * Replaces paddle.nn.Linear / paddle.matmul (+ the elementwise ops around them) on the hot path:
 *   top MLP fwd/bwd  deepfm/net.py:142-174, dcn_v2/net.py:140-184, din/net.py:104-137,175-181
 *   CrossNetV2       dcn_v2/net.py:214-226 : REC_EPI_CROSS computes X_l + X_0*(X_l W + b) in place
 *   CrossNetMix      dcn_v2/net.py:278-320 : REC_EPI_BIAS_TANH for the low-rank projections
 * Row-major everywhere; Paddle's Linear.weight is [in,out] = B[K,N].
 *   trans_a: A is stored [K,M] (dW = X^T G);  trans_b: B is stored [N,K] (dX = G W^T).
 * split_k: 0 = automatic, partial sums are reduced in a fixed order (deterministic).
 *
 * ARITHMETIC — two kernel families, chosen per call:
 *   (a) exact f32: v_mfma_f32_16x16x4_f32 = a k-ordered fmaf chain per output element.  Every call with M < 8192 rows, every
 *       shape (b) does not cover, and EVERY call when the process environment holds REC_GEMM_BF16X3=0.
 *   (b) bf16 x 3 (the DEFAULT for the tall GEMMs of the towers; csrc/gemm_bf16x3.h): each f32 operand is split into three
 *       bf16 terms (8 + 8 + 8 significand bits, round-to-nearest remainders) and the six term products with i + j <= 2
 *       are accumulated in f32 by v_mfma_f32_16x16x32_bf16.  Taken by   forward / dX calls (trans_a = 0): M >= 8192,
 *       N % 4 == 0, N within 15 % of a column-block multiple (336 <= N: 400, 432, 512, 768, 1560 ...), K % 8 == 0, K >= 64,
 *       16-byte aligned rows, split_k <= 1, no b_colsum;   weight-gradient calls (trans_a = 1, no epilogue): K >= 8192,
 *       336 <= M <= 448, 336 <= N <= 416 (REC_GEMM_BF16X3_DW=0: never).  Results are f32-GRADE — the error against
 *       float64 is that of (a), <= 4e-7 of sum |a||b| (tests/test_gemm_gpu.py) — but NOT the bit pattern of (a):
 *         - a step sharded so that a rank holds fewer than 8192 rows runs (a) and does not match the unsharded step's
 *           bits (it matches to the bound above);
 *         - non-finite operands: NaN propagates in both; an operand that is +-Inf, or finite with |x| > 3.39e38 (it
 *           rounds to the bf16 Inf), leaves Inf - Inf in its second term, so (b) returns NaN where (a) returns +-Inf —
 *           also behind REC_EPI_RELU_MASK / BIAS_RELU, where relu(-Inf) = 0 under (a) continues and NaN under (b) does
 *           not; operands whose third term falls below 2^-133 lose it (bf16 subnormals flush): the product of such an
 *           operand carries 16 instead of 24 significand bits, i.e. an absolute error below 2^-126 * |b| — not
 *           observable behind an f32 accumulation of normal numbers (tests/test_gemm_gpu.py::test_gemm_nonfinite_*).
 *       REC_GEMM_BF16X3 (read per call): unset = (b) as above; 1 = (b), but a weight-gradient call with an explicit
 *       split_k stays on (a) (the caller asked for few long blocks beside another kernel); 0 = (a) everywhere.
 *   WORKSPACE: under (b) a forward / dX call WRITES op(B)'s three-plane image into the workspace (unless
 *   rec_gemm_epilogue_args.b_image hands one in) and a weight-gradient call its partial tiles — so, unlike (a) without
 *   split-K, concurrent calls on two streams need one workspace each.  rec_gemm_f32_workspace_bytes covers both families.
 *   A call that takes a kernel of (b) is held to that figure: with fewer bytes than its image (forward / dX, no b_image) or
 *   its partial tiles (weight gradient) need it fails with REC_EWORKSPACE before any launch; it does not change family.
 * ---------------------------------------------------------------------------------------- */
typedef enum {
  REC_EPI_NONE = 0,
  REC_EPI_BIAS = 1,         /* acc + bias[j] */
  REC_EPI_BIAS_RELU = 2,    /* max(acc + bias[j], 0) */
  REC_EPI_RELU_MASK = 3,    /* aux0[i,j] > 0 ? acc : 0          (ReLU backward on dX) */
  REC_EPI_CROSS = 4,        /* aux1[i,j] + aux0[i,j] * (acc + bias[j])   (aux0 = X_0, aux1 = X_l) */
  REC_EPI_BIAS_SIGMOID = 5, /* sigmoid(acc + bias[j]) */
  REC_EPI_BIAS_TANH = 6,    /* tanh(acc + bias[j]); bias may be NULL */
  REC_EPI_ADD = 7,          /* acc + aux1[i,j] (+ bias[j], + aux0[i,j] when given) */
  REC_EPI_DTANH = 10,       /* acc * (1 - aux0[i,j]^2)             (tanh backward on dX, CrossNetMix) */
  REC_EPI_DSIGMOID = 9,     /* acc * aux0[i,j] * (1 - aux0[i,j])   (sigmoid backward on dX, din/net.py MLPs) */
  REC_EPI_MOE = 8           /* aux1[i,j] + aux0[i,j] * row_scale[i] * (acc + bias[j])
                               (CrossNetMix, dcn_v2/net.py:301-317: aux0 = x_0, aux1 = running x_{l+1},
                               row_scale = softmax gate of this expert) */
} rec_epilogue;

typedef struct {
  int64_t m;
  int32_t n, k;
  int32_t lda, ldb, ldc; /* leading dimensions in floats, of the arrays as stored */
  int32_t trans_a, trans_b;
  int32_t epilogue;      /* rec_epilogue */
  int32_t split_k;       /* 0 = automatic */
  int32_t num_cus;       /* 0 = the whole chip; > 0: the stream the call is issued on is confined to this many compute
                            units (rec_stream_create_cu_range): split-K and the bf16 x 3 weight-gradient grid are sized
                            for one resident round on THOSE, not on the chip */
} rec_gemm_desc;

typedef struct {
  const float* bias;        /* [N] */
  const float* aux0;        /* [M, ld_aux0] */
  int32_t ld_aux0;
  const float* aux1;        /* [M, ld_aux1] */
  int32_t ld_aux1;
  const float* row_scale;   /* [M] with stride row_scale_stride (REC_EPI_MOE) */
  int32_t row_scale_stride;
  float* out2;              /* [M, ld_out2] or NULL: REC_EPI_CROSS also stores u = acc + bias (for backward) */
  int32_t ld_out2;
  float* b_colsum;          /* [N] or NULL (trans_a calls only): also return the column sums of B over K — the
                               bias gradient when the call computes dW = X^T dY (B = dY), at no extra pass */
  const void* b_image;      /* NULL, or the bf16 x 3 image of THIS call's op(B) made by rec_gemm_b_images (same k, n,
                               trans_b, current values of B): the call then skips its own split launch and does not
                               write the workspace.  Ignored by calls that do not take the bf16 x 3 forward / dX kernel */
  void* relu_bits;          /* NULL, or rec_gemm_relu_bits_bytes(desc) bytes of device memory (8-byte aligned): the ReLU
                               mask of an activation as BITS.  A REC_EPI_BIAS_RELU call WRITES it beside C (one 64-bit word
                               per row, column block and lane group of the bf16 x 3 kernel); a REC_EPI_RELU_MASK call with
                               the same m and n READS it instead of aux0 (which may then be NULL): the dX GEMM of a tower
                               fetches 4 MB of bits where it fetched the 105 MB activation.  Same results bit for bit.
                               Only calls for which rec_gemm_relu_bits_bytes reports eligible = 1 (both sides take the
                               bf16 x 3 forward / dX kernel); any other call given relu_bits fails with REC_EINVAL */
} rec_gemm_epilogue_args;

int rec_gemm_f32_workspace_bytes(const rec_gemm_desc* desc, size_t* bytes);
/* Host query: *eligible = 1 and the size of rec_gemm_epilogue_args.relu_bits for this call (REC_EPI_BIAS_RELU or
 * REC_EPI_RELU_MASK on the bf16 x 3 forward / dX kernel), else 0 / 0.  The layout depends on m and n only: the mask a
 * forward call with (m, n) wrote is the one a dX call with the same (m, n) reads
 * (deepfm/net.py:142-174: Linear -> ReLU, and the ReLU' of its backward). */
int rec_gemm_relu_bits_bytes(const rec_gemm_desc* desc, int32_t* eligible, size_t* bytes);
/* Host query: the split-K factor the planner picks for `desc` (its split_k ignored) when the GEMM may use
 * num_cus compute units (<= 0: the whole chip) — one resident round of blocks.  A caller that runs the GEMM on
 * a CU-restricted stream (rec_stream_create_cu_range) passes the result as desc->split_k. */
int rec_gemm_plan_splits(const rec_gemm_desc* desc, int32_t num_cus, int32_t* splits);
int rec_gemm_f32(const rec_gemm_desc* desc, const float* A, const float* B, float* C,
                 const rec_gemm_epilogue_args* args /* may be NULL */, void* workspace,
                 size_t workspace_bytes, void* stream);
/* Two INDEPENDENT GEMMs — neither reads what the other writes — in one call: the backward of one Linear,
 * dW = X^T G (+ db = colsum(G): desc0, trans_a, no epilogue) and dX = G W^T (+ ReLU' of the layer in front: desc1,
 * trans_b, REC_EPI_NONE / REC_EPI_RELU_MASK / REC_EPI_DSIGMOID), both consume G and nothing of each other (ops.mlp_backward; the
 * reference's Linear backward is two matmul_grad kernels, `paddle.nn.Linear` in deepfm/net.py:142-174).  At the
 * reference's own batch sizes both are launch-bound (M N K < 1.5e8, K <= 1024: csrc/gemm_direct.h) and go out as ONE
 * launch whose workgroups run exactly the code of the single launches — bit-identical to two rec_gemm_f32 calls, one
 * ~4 us launch less; any other pair IS two rec_gemm_f32 calls, desc0 first (workspace: the larger of the two needs).
 * The call checks the workspace against the larger of the two rec_gemm_f32_workspace_bytes figures before EITHER GEMM is
 * launched (REC_EWORKSPACE: neither C0 nor C1 has been written).
 * REC_GEMM_PAIR=0: always two calls. */
int rec_gemm_f32_pair(const rec_gemm_desc* desc0, const float* A0, const float* B0, float* C0,
                      const rec_gemm_epilogue_args* args0 /* may be NULL */, const rec_gemm_desc* desc1, const float* A1,
                      const float* B1, float* C1, const rec_gemm_epilogue_args* args1 /* may be NULL */, void* workspace,
                      size_t workspace_bytes, void* stream);
/* Which kernel the calling thread's last rec_gemm_f32 / rec_gemm_f32_pair call launched (host bookkeeping: one struct
 * store per call, nothing on the device).  The routing rules depend on shapes, alignment and process environment; a
 * test that means one kernel asserts it here instead of trusting its shape.  A call refused before its launch leaves
 * the previous report; before the thread's first call family is -1. */
typedef enum {
  REC_GEMM_ROUTE_SKINNY_ROWS = 0, /* N <= 4: one wave per row */
  REC_GEMM_ROUTE_SKINNY_DW = 1,   /* N <= 4, trans_a, long K: k-chunk partials + the split-K reduce */
  REC_GEMM_ROUTE_X3_DW = 2,       /* bf16 x 3 weight gradient + the split-K reduce */
  REC_GEMM_ROUTE_X3 = 3,          /* bf16 x 3 forward / dX */
  REC_GEMM_ROUTE_PANEL = 4,       /* row-panel kernel */
  REC_GEMM_ROUTE_GLDS = 5,        /* LDS-DMA ring */
  REC_GEMM_ROUTE_DIRECT = 6,      /* one launch, a wave per 16 x 16 tile */
  REC_GEMM_ROUTE_TILED = 7        /* register-staged tiles (+ the split-K reduce when splits > 1) */
} rec_gemm_route_family;
enum {
  REC_GEMM_ROUTE_FAST = 1,        /* tiled: branch-free tile loaders (aligned operands, extents multiples of 4) */
  REC_GEMM_ROUTE_PIPE = 2,        /* tiled: the whole-tile pipe kernel */
  REC_GEMM_ROUTE_VEC = 4,         /* direct: float4 loads along k */
  REC_GEMM_ROUTE_KS4 = 8,         /* direct: K split over the workgroup's four waves */
  REC_GEMM_ROUTE_FOLD = 16,       /* tiled split-K: K slices folded into a 1-D grid */
  REC_GEMM_ROUTE_VEC_A = 32,      /* skinny rows: float4 loads of A */
  REC_GEMM_ROUTE_PAIR = 64        /* direct: both GEMMs of rec_gemm_f32_pair in one launch (VEC / KS4: of desc1) */
};
typedef struct {
  int32_t family; /* rec_gemm_route_family */
  int32_t cfg;    /* tiled: index of the tile config launched (0 128x80, 1 256x80, 2 256x128, 3 128x128, 4 80x80,
                     5 64x80, 6 128x80 at 4 blocks/CU, 7 144x80); else -1 */
  int32_t splits; /* tiled, skinny_dw, x3_dw: K slices; 1 = the GEMM kernel applied the epilogue itself, > 1 = the
                     reduce kernel did.  Every other family: 1 */
  int32_t flags;  /* REC_GEMM_ROUTE_* bits */
} rec_gemm_route;
int rec_gemm_last_route(rec_gemm_route* out);
/* Which kernels the calling thread's calls launched, for the entry points that route on the host by row width,
 * strides, pointer alignment and process environment (host bookkeeping, nothing on the device).  The log is per thread
 * and OFF by default; while off, a routing decision costs one thread-local flag test and nothing is formatted or stored.
 *   rec_route_log_begin : clears the calling thread's log and switches it on.
 *   rec_route_log_end   : switches it off and copies the notes to out, one per launch in call order, each followed by
 *                         '\n', NUL-terminated.  *needed (may be NULL) receives the bytes that takes.  bytes < *needed is
 *                         REC_EINVAL: the notes are kept until the next begin, so the call may be repeated with a larger
 *                         buffer.  Notes past the internal buffer (16 KiB) are never cut silently: REC_ESHAPE.
 * A note names the kernel template and its arguments:
 *   rows<VEC,LANES>                  every entry point that dispatches on (emb_dim, row stride): LANES lanes of VEC floats
 *   adam_rows_narrow<NV,V4,L2>       rec_sparse_adam_rows / _l2, one lane per row: NV float4 groups, float4 row access, decay
 *   ms_lane<D> | ms_rows<VEC,LANES,NSW,WAVES>           rec_multislot_sumpool_fwd
 *   ps_narrow<DX> | ps_narrow_whole<row9> | ps_rows<VEC,LANES,statv>   rec_ps_push_rows
 *   din_fwd:generic | din_fwd:ct:<nopf2|pf2|pf1>:<walk|tickets|split>  rec_din_attention_pool_fwd / _fwd_ws
 *   din_bwd:generic | din_bwd:ct:<walk|tickets>[:nosplit]              rec_din_attention_pool_bwd / _bwd_ws (nosplit:
 *                                                                      REC_DIN_TILE_SPLIT=0 holds in this process)
 * A call refused before it chooses a kernel leaves no note. */
int rec_route_log_begin(void);
int rec_route_log_end(char* out, size_t bytes, size_t* needed);
/* Weight images ahead of time.  Under the bf16 x 3 family every forward / dX call splits op(B) [k, n] into its plane image
 * first (a ~5 us launch per call); the weights of a tower change once per step, so a trainer makes ALL images of the step
 * in one launch right after its optimizer (rec_adam_dense) and passes them as rec_gemm_epilogue_args.b_image.
 *   rec_gemm_b_image_bytes : *eligible = 1 and the image size if an op(B) of k x n has an image form, else 0 / 0
 *   rec_gemm_b_images      : items[i].image <- image of op(B_i) (B_i as rec_gemm_f32 takes it: [k,n] row-major with ldb,
 *                            or [n,k] when trans_b); any count (8 images per launch).  items is a HOST array. */
typedef struct {
  const float* B;
  int32_t ldb, k, n, trans_b;
  void* image;     /* device, 16-byte aligned, rec_gemm_b_image_bytes(k, n) bytes */
} rec_gemm_b_image;
int rec_gemm_b_image_bytes(int32_t k, int32_t n, int32_t* eligible, size_t* bytes);
int rec_gemm_b_images(int32_t count, const rec_gemm_b_image* items, void* stream);

/* out[j] = sum_i G[i,j] (bias gradient of a Linear), fixed reduction order. */
int rec_colsum_workspace_bytes(int64_t m, int32_t n, size_t* bytes);
int rec_colsum(int64_t m, int32_t n, int32_t ld, const float* G, float* out, void* workspace,
               size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * CrossNet layers as ONE entry point per layer and direction (SURVEY.md §8(b) `crossnet_v2_layer`,
 * `crossnet_mix_layer`): what a Paddle custom op (PD_BUILD_OP / PD_BUILD_GRAD_OP) binds for
 *   dcn_v2/net.py:214-226  CrossNetV2:  x_{l+1} = x_l + x_0 * (x_l W_l + b_l)
 *   dcn_v2/net.py:278-320  CrossNetMix: x_{l+1} = x_l + sum_e p_e * x_0 * (tanh(tanh(x_l V_e) C_e^T) U_e^T + b_l),
 *                                       p = softmax_e(x_l gate_w + gate_b)
 * They launch the GEMMs (rec_gemm_f32 epilogues) and streaming glue passes declared above in a fixed order; no
 * kernel of their own.  Row strides (ld_*) in floats, 0 = d.  Workspace: query the _workspace_bytes function
 * (GEMM split-K partials + the layer's scratch tensors).
 * ---------------------------------------------------------------------------------------- */
typedef struct {
  int64_t batch;
  int32_t d;                            /* feature width: num_field * emb_dim */
  int32_t ld_x0, ld_xl, ld_out, ld_u;   /* X_0, X_l, X_{l+1}, saved U_l */
} rec_crossnet_v2_desc;
int rec_crossnet_v2_layer_workspace_bytes(const rec_crossnet_v2_desc* desc, size_t* fwd_bytes, size_t* bwd_bytes);
/* W [d,d] (Paddle [in,out]), bias [d]; U_saved [B, ld_u] (or NULL) receives u = x_l W + b for the backward. */
int rec_crossnet_v2_layer_fwd(const rec_crossnet_v2_desc* desc, const float* X0, const float* Xl, const float* W,
                              const float* bias, float* Xnext, float* U_saved, void* workspace,
                              size_t workspace_bytes, void* stream);
/* Given dXnext = d x_{l+1}:  dW [d,d], db [d], dXl = d x_l (may alias dXnext);  dX0_acc (+)= dXnext * U_l
 * (accumulate_dx0 = 0: overwritten, never read);  fold_dx0 != 0: dXl also receives dX0_acc (the first layer, x_l = x_0).
 * GRADIENT STRIDES (ld_dxnext, ld_acc, ld_dxl; 0 = d) are call arguments, not descriptor fields, so the workspace query
 * cannot see them, and the split-K partials of the GEMM that writes dXl are [splits][B][ld_dxl].  The contract, for this
 * entry point and for rec_crossnet_mix_layer_bwd:
 *   - the backward reads desc->ld_out for nothing but sizing: a caller whose gradient buffers are strided wider than the
 *     strides of its descriptor sets ld_out to the widest of them in the descriptor it hands to the query AND to the call,
 *     and bwd_bytes then covers the call;
 *   - every argument and workspace check of the call (strides < d: REC_EINVAL; workspace smaller than what the GEMMs
 *     need AT THE STRIDES PASSED: REC_EWORKSPACE) is made before the first launch: a negative status means that no
 *     output and no byte of dX0_acc was written.  A call either returns 0 with every output complete, or did nothing. */
int rec_crossnet_v2_layer_bwd(const rec_crossnet_v2_desc* desc, const float* X0, const float* Xl, const float* W,
                              const float* U_saved, const float* dXnext, int32_t ld_dxnext, float* dX0_acc,
                              int32_t ld_acc, int32_t accumulate_dx0, int32_t fold_dx0, float* dXl,
                              int32_t ld_dxl, float* dW, float* db, void* workspace, size_t workspace_bytes,
                              void* stream);

typedef struct {
  int64_t batch;
  int32_t d, rank, experts;             /* experts <= 64 */
  int32_t ld_x0, ld_xl, ld_out;
} rec_crossnet_mix_desc;
int rec_crossnet_mix_layer_workspace_bytes(const rec_crossnet_mix_desc* desc, size_t* fwd_bytes, size_t* bwd_bytes);
/* U, V [E,d,r], C [E,r,r], bias [d], gate_w [d,E] (the E Linear(d,1) stacked), gate_b [E].
 * Saved for the backward: t1 = tanh(x_l V_e), t2 = tanh(t1 C_e^T), both [B, E*r]; prob [B,E]. */
int rec_crossnet_mix_layer_fwd(const rec_crossnet_mix_desc* desc, const float* X0, const float* Xl, const float* U,
                               const float* V, const float* C, const float* bias, const float* gate_w,
                               const float* gate_b, float* Xnext, float* t1, float* t2, float* prob,
                               void* workspace, size_t workspace_bytes, void* stream);
/* gU, gV [E,d,r], gC [E,r,r], gbias [d] are written; the gating layers are shared by all cross layers
 * (net.py:267-268): g_gate_w [d,E] / g_gate_b [E] are overwritten when accumulate_gate == 0, added to otherwise.
 * dXl must not alias dXnext (REC_EINVAL).  dX0_acc / fold_dx0 / gradient strides and the all-or-nothing contract as above. */
int rec_crossnet_mix_layer_bwd(const rec_crossnet_mix_desc* desc, const float* X0, const float* Xl, const float* U,
                               const float* V, const float* C, const float* bias, const float* gate_w,
                               const float* t1, const float* t2, const float* prob, const float* dXnext,
                               int32_t ld_dxnext, float* dX0_acc, int32_t ld_acc, int32_t accumulate_dx0,
                               int32_t fold_dx0, float* dXl, int32_t ld_dxl, float* gU, float* gV, float* gC,
                               float* gbias, float* g_gate_w, float* g_gate_b, int32_t accumulate_gate,
                               void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * Loss head: predict = sigmoid(y1+y2+y_dnn) (deepfm/net.py:47);
 *            cost = log_loss(pred,label,eps=1e-4); avg = mean(cost) (deepfm/dygraph_model.py:53-58)
 * and its gradient dz = d avg / d z.  loss_out[0] = avg (reduced in a fixed order).
 * y2 / y_dnn may be NULL (treated as 0).  workspace >= rec_logloss_workspace_bytes(B).
 * mean_over = denominator of the mean (0 -> batch).  Data-parallel ranks pass the GLOBAL batch so
 * that summing gradients over ranks reproduces one step on the concatenated batch.
 * clip_lo < clip_hi: the logit goes through paddle.clip(z, clip_lo, clip_hi) first (slot_dnn/net.py:84,
 * `F.sigmoid(paddle.clip(y_dnn, min=-15.0, max=15.0))`), dz = 0 outside the open interval; clip_lo >= clip_hi: off.
 * ---------------------------------------------------------------------------------------- */
int rec_logloss_workspace_bytes(int64_t batch, size_t* bytes);
int rec_sigmoid_logloss(int64_t batch, int64_t mean_over, const float* y1, const float* y2,
                        const float* y_dnn,
                        const int64_t* label, float eps, float clip_lo, float clip_hi, float* pred,
                        float* dz, float* loss_out, void* workspace, size_t workspace_bytes, void* stream);

/* binary_cross_entropy_with_logits(reduction='mean') [EXT] (din/dygraph_model.py:58-61): loss_out[0] = mean,
 * pred = sigmoid(logit), dz = (pred - label) / mean_over (0 -> batch).  label is float32 as the DIN reader
 * feeds it.  workspace >= rec_logloss_workspace_bytes(batch). */
int rec_bce_with_logits(int64_t batch, int64_t mean_over, const float* logit, const float* label,
                        float* pred, float* dz, float* loss_out, void* workspace, size_t workspace_bytes,
                        void* stream);

/* paddle.metric.Auc("ROC").update [EXT] (deepfm/dygraph_model.py:69-73,83-84):
 *   bucket = int(pred*num_thresholds); stat_pos[bucket] += label!=0; stat_neg[bucket] += label==0.
 * stat_pos/stat_neg are i64 [num_thresholds+1], accumulated (not cleared). */
int rec_auc_histogram(int64_t batch, const float* pred, const int64_t* label,
                      int32_t num_thresholds, int64_t* stat_pos, int64_t* stat_neg, void* stream);

/* ------------------------------------------------------------------------------------------
 * Row-sharded tables: owner(r) = r mod G, local row = r div G.
 * Stands in for the key-sharded pull/push of core.PSGPU inside exe.train_from_dataset
 * (tools/static_gpubox_trainer.py:152-160,256; models/rank/dnn/net.py:71-79) [HeterPS is EXT].
 * One stable partition of the n = B*S lookups by owner:
 *   send_local_row [n] i64 : local rows grouped by owner (ascending position inside a group) —
 *                            the message of the ids all-to-all; first sum(send_counts[0..G)) valid
 *   send_pos       [n] i64 : position b*S+s of each entry (row-grad gather for the bwd exchange)
 *   send_sample    [n] i64 : b of each entry (dy1 gather for the first-order table)
 *   slot_of_pos    [n] i64 : 1 + index of a position in send order, 0 for padding — the reply of
 *                            the rows all-to-all arrives in send order, so this is the `ids` that
 *                            rec_deepfm_fm_fwd reads the reply buffer with (row 0 = zero row)
 *   send_counts  [G+1] i64 : entries per owner; [G] = dropped (padding / out-of-range) positions
 * All outputs are bit-exact targets.
 * ---------------------------------------------------------------------------------------- */
int rec_shard_route_workspace_bytes(int64_t n, int32_t num_shards, size_t* bytes);
int rec_shard_route(int64_t n, int32_t num_slots, int64_t num_rows, int64_t padding_idx,
                    int32_t num_shards, const int64_t* ids, const int64_t* slot_offset,
                    int64_t* send_local_row, int64_t* send_pos, int64_t* send_sample,
                    int64_t* slot_of_pos, int64_t* send_counts, int32_t* status, void* workspace,
                    size_t workspace_bytes, void* stream);

/* Deduplicated lookup plan: the DISTINCT rows a rank needs of every owner, in fixed-capacity send slots (owner o owns
 * slots [o * cap, (o + 1) * cap)) — what HeterPS does per pass before it builds the per-GPU tables
 * (tools/static_gpubox_trainer.py:237-246 load_into_memory -> PSGPU.begin_pass [EXT]).  rec_ids_group over the shard-major
 * key (row % G) * local_rows + row / G, then four small kernels; no host read, sizes are the capacity:
 *   sorted_pos / uniq_rows / seg_offset / n_uniq : the grouping (uniq_rows = shard-major keys), as rec_ids_group emits it —
 *                  the merge keys of rec_sparse_sgd_rows & co. for the local pre-merge of the row gradients
 *   send_rows    [G * cap] i64 : local row per slot; empty slots hold `local_rows` (the owner groups them away by
 *                  rec_ids_group(num_rows = local_rows + 1, padding_idx = local_rows))
 *   slot_of_pos  [n] i64 : 1 + slot of a position's row, 0 = padding / out of range / behind the capacity — the `ids`
 *                  rec_deepfm_fm_fwd reads the (G * cap + 1)-row reply table with (row 0 = zero row)
 *   slot_of_uniq [n] i64 : slot of distinct row u, G * cap = none;   counts [G] i64 : distinct rows per owner
 * An owner that needs more than cap distinct rows sets REC_FLAG_EXCHANGE_OVERFLOW.  All outputs are bit-exact targets. */
int rec_dedup_plan_workspace_bytes(int64_t n, int32_t num_shards, int64_t local_rows, size_t* bytes);
int rec_dedup_plan(int64_t n, int32_t num_slots, int64_t num_rows, int64_t padding_idx, int32_t num_shards,
                   int64_t local_rows, int32_t cap, const int64_t* ids, const int64_t* slot_offset, int32_t* sorted_pos,
                   int64_t* uniq_rows, int32_t* seg_offset, int32_t* n_uniq, int64_t* send_rows, int64_t* slot_of_pos,
                   int64_t* slot_of_uniq, int64_t* counts, int32_t* status, void* workspace, size_t workspace_bytes,
                   void* stream);

/* ------------------------------------------------------------------------------------------
 * Exchange layer of the row-sharded table (reference: the inter-GPU pull / push of
 * core.PSGPU, tools/static_gpubox_trainer.py:152-160,256 [EXT HeterPS]).  `comm` is an RCCL ncclComm_t — created
 * by rec_comm_init (one per process; rank 0 makes the id with rec_comm_unique_id and distributes its 128 bytes by
 * any means) or owned by the framework.  RCCL is bound at run time; REC_ENCCL when it is missing or fails.
 *   rec_alltoall_exchange: all-to-all(v) of rows of row_bytes bytes — send is grouped by destination rank
 *     (send_counts[d] rows, HOST array of `world` entries), recv by source rank; asynchronous on `stream`.
 *     A sharded step issues it three times: ids to owners, rows back, row-gradients to owners.
 *   rec_allreduce_sum_f32: the flat dense-gradient bucket.
 *   rec_alltoall_layout: HOST function, the arithmetic rec_alltoall_exchange does before it enters RCCL, for any
 *     `world` and without a communicator: {send,recv}_bytes[i] = {send,recv}_counts[i] * row_bytes, {send,recv}_displs[i]
 *     = the bytes of the peers before i, *total_{send,recv} = the sums (all HOST arrays of `world` entries).  A negative
 *     count, row_bytes <= 0, world < 1 or a null pointer is REC_EINVAL; a product or a running sum that does not fit
 *     int64 is REC_ESHAPE (rec_alltoall_exchange returns the same).  A refused call writes none of its outputs.
 * ---------------------------------------------------------------------------------------- */
int rec_comm_unique_id(void* id128);
int rec_comm_init(const void* id128, int32_t world, int32_t rank, void** comm);
int rec_comm_destroy(void* comm);
/* ranks of the communicator as RCCL reports them (ncclCommCount) */
int rec_comm_size(void* comm, int32_t* world);
/* 1 when RCCL's entry points resolve in this process (so that every rank can AGREE on the native exchange before
 * any of them enters ncclCommInitRank), else 0; never fails */
int rec_comm_available(void);
int rec_alltoall_exchange(void* comm, const void* send, const int64_t* send_counts, void* recv,
                          const int64_t* recv_counts, int32_t row_bytes, void* stream);
int rec_allreduce_sum_f32(void* comm, float* buf, int64_t n, void* stream);
int rec_alltoall_layout(int32_t world, const int64_t* send_counts, const int64_t* recv_counts, int32_t row_bytes,
                        int64_t* send_bytes, int64_t* send_displs, int64_t* recv_bytes, int64_t* recv_displs,
                        int64_t* total_send, int64_t* total_recv);

/* Row H — feature hash, HOST function: xxh32(str(field_idx)+value) % hash_dim
 * (models/rank/dnn/benchmark_reader.py:52).  `bytes` = the concatenated string. */
uint32_t rec_xxh32(const void* bytes, size_t len, uint32_t seed);
int rec_xxh32_hash_mod(const char* const* strings, const int32_t* field_idx, int64_t n,
                       uint32_t hash_dim, int64_t* out);

/* Rows R and H — input pipeline, HOST functions (no device code; outputs are caller-owned, ideally pinned).
 * rec_parse_slot_text : models/rank/deepfm/criteo_reader.py:61-103 (and dcn_v2/reader.py:41-89 with
 *   log1p_dense = 1): "click:L dense_feature:v x13 1:id ... 26:id" per line; missing sparse slot -> id 0,
 *   missing dense slot -> zeros, first value of a repeated slot wins.  label [n], ids [n,n_sparse] i64,
 *   dense [n,n_dense] f32 (parsed as double, then cast — as float() / np.float32 do).
 *   Number fields: "[-]digits[.digits]" with <= 15 significant digits is read as integer / 10^k (correctly rounded, the
 *   value strtod returns), "[-]digits" ids / labels of <= 18 digits by a digit loop; every other form goes to strtod /
 *   strtoll on a NUL-terminated copy of the field.  Only buf[0 .. len) is ever read (an mmap without a final newline is fine).
 * rec_parse_criteo_tsv: models/rank/dnn/benchmark_reader.py:39-54: "label \t 13 ints \t 26 strings";
 *   dense = (x - cont_min[j]) / cont_diff[j] ("" -> 0), ids = xxh32(str(field_idx)+string) % hash_dim with
 *   field_idx = 14..39 (the column index, as the reference hashes it).
 * threads <= 0: one per host core (capped at 64).  *n_lines = lines parsed (<= max_lines). */
int rec_count_lines(const char* buf, size_t len, int32_t threads, int64_t* n_lines); /* to size the outputs */
/* Indices (ascending) of the lines made of blanks only — the parsers above count them as lines; a loader that cuts
 * batches from a whole-file parse skips them like the reference's `for line in f` readers do.  *n_blank = how many
 * there are (may exceed max_out: only the first max_out are written). */
int rec_blank_lines(const char* buf, size_t len, int32_t threads, int64_t max_out, int64_t* idx, int64_t* n_blank);
/* One batch cut out of whole-file parses by line range (the in-memory pass of the gpubox loop): piece p = lines
 * [l0[p], l1[p]) of a rec_parse_feasign_slots result (values[p], lod[p] with row stride lod_stride[p], base[p]); the
 * batch's slot s holds its ids of piece 0, then of piece 1, ... — the CSR a parse of exactly those lines gives.
 * out_lod [num_slots, lines + 1], out_base [num_slots + 1], out_values [max_values >= total ids]. */
int rec_csr_cut(int32_t num_slots, int32_t n_pieces, const int64_t* const* values, const int64_t* const* lod,
                const int64_t* lod_stride, const int64_t* const* base, const int64_t* l0, const int64_t* l1,
                int32_t threads, int64_t* out_values, int64_t max_values, int64_t* out_lod, int64_t* out_base);
/* Occurrences of one byte value, multi-threaded (the ':' count bounds the values of rec_parse_feasign_slots). */
int rec_count_byte(const char* buf, size_t len, int32_t byte, int32_t threads, int64_t* n);
int rec_parse_slot_text(const char* buf, size_t len, int32_t n_sparse, int32_t n_dense,
                        int32_t log1p_dense, int64_t max_lines, int32_t threads, int64_t* label,
                        int64_t* ids, float* dense, int64_t* n_lines);
int rec_parse_criteo_tsv(const char* buf, size_t len, int32_t n_dense, int32_t n_sparse,
                         const float* cont_min, const float* cont_diff, uint32_t hash_dim,
                         int64_t max_lines, int32_t threads, int64_t* label, int64_t* ids, float* dense,
                         int64_t* n_lines);

/* Host parser of multi-value slot lines (models/rank/slot_dnn/queuedataset_reader.py:56-82): a line is
 * "feasign:slot feasign:slot ..." with uint64 feasigns and any number of values per slot.  Slots outside
 * [first_slot, first_slot + num_slots) are dropped; a slot that does not occur in a line gets the single padding
 * id 0 (line_process, :75-80).  Output = the layout rec_emb_gather_sumpool consumes, slot-major CSR:
 *   values[slot_base[s] + lod[s*(max_lines+1) + b] + j] = j-th value of slot s in line b      (token order)
 *   lod [num_slots, max_lines+1] (row s: offsets of slot s over the lines), slot_base [num_slots+1]
 * hash_rows = 0: values are the raw uint64 bit patterns (what the reference feeds its PS hash map);
 * hash_rows >= 2: rows of a hashed table, 0 -> 0 (padding row), f -> 1 + f % (hash_rows-1).
 * REC_EWORKSPACE (with *n_values = the size needed) when max_values is too small.  Multi-threaded, results do
 * not depend on the thread count. */
int rec_parse_feasign_slots(const char* buf, size_t len, int32_t first_slot, int32_t num_slots,
                            uint64_t hash_rows, int64_t max_lines, int64_t max_values, int32_t threads,
                            int64_t* values, int64_t* lod, int64_t* slot_base, int64_t* n_lines,
                            int64_t* n_values);

/* Fills buf[i] = i-th value of a counter-based generator, uniform in [lo,hi) — used to initialise
 * multi-GB tables on the device without a host round trip. */
int rec_fill_uniform(int64_t n, float* buf, float lo, float hi, uint64_t seed, void* stream);

/* Device-to-device copy on `stream` (hipMemcpyAsync).  The host mirrors copy parameter slices with it (the folded
 * layer-0 weights of DeepFM) so that a training step consists of C-ABI calls only and can be replayed from a recorded
 * call list (paddlerec_amd/plan.py). */
int rec_copy_async(void* dst, const void* src, size_t bytes, void* stream);
/* The same for a [rows, width_bytes] window of two pitched device buffers (hipMemcpy2DAsync): a binder that must hand
 * a framework a CONTIGUOUS column block of an engine output (the item / category halves of DIN's d_hist [B,T,E] as the
 * SelectedRows values of two separate embedding parameters, paddlerec_amd/paddle_ops/rec_paddle_ops.cc). */
int rec_copy_2d_async(void* dst, size_t dst_pitch_bytes, const void* src, size_t src_pitch_bytes, size_t width_bytes,
                      size_t rows, void* stream);
/* out [cols, rows] = in [rows, cols]^T (f32, both contiguous).  The DIN backward wants the first attention weight
 * transposed (att_w1_t); a binder without a tensor library of its own materialises it with this. */
int rec_transpose_f32(int64_t rows, int64_t cols, const float* in, float* out, void* stream);
/* dst[i] = (int64) round(src[i * src_stride]).  The gpubox nets carry the click label to the lookup as a float column
 * (show_click = concat([ones, cast(label)]), dnn/static_model.py:86-94); the accessor's push counts clicks in int64 —
 * a binder without a tensor library (the custom operator rec_ps_pull's gradient) converts the column with this. */
int rec_cast_f32_i64(int64_t n, const float* src, int64_t src_stride, int64_t* dst, void* stream);

/* MEASUREMENT AID, no reference counterpart: a stand-in link.  `blocks` (<= 64) workgroups copy `bytes` between two device
 * rings (ring_bytes each, a power of two; the copy wraps) and pace themselves so that the launch lasts bytes / gbytes_per_s + fixed_us
 * — what an RCCL all-to-all over xGMI is to the rest of the chip: a few resident workgroups moving bytes at the links'
 * rate.  paddlerec_amd/sharded.py issues it where the collectives of a world-1 run sit (REC_EMULATE_LINKS=<G>), so that
 * ONE GPU can show whether the exchange of a G-GPU step fits beside the dW GEMMs.
 * The launch holds its workgroups for the modelled duration fixed_us + bytes / (gbytes_per_s * 1e3) microseconds whatever
 * the copy manages, so a call whose modelled duration exceeds 1 s (rec_stream_spin's limit) is REC_EINVAL, as are a rate
 * <= 0, fixed_us < 0, blocks outside 1..64, a ring that is no power of two in [64 KB, 2^31] and a src / dst that is null
 * or not 16-byte aligned — all of it checked on the host before any HIP call. */
int rec_link_emulate(size_t bytes, float gbytes_per_s, float fixed_us, int32_t blocks, const void* src, void* dst,
                     size_t ring_bytes, void* stream);

/* One wave busy-waits `micros` microseconds on `stream`.  Host-side stream probe: HIP maps streams onto a
 * few hardware queues and kernels of two streams that share a queue run strictly one after the other, so a
 * caller that wants its HBM-bound side stream to run underneath the GEMMs of its main stream spins both and
 * checks with events that the two spins overlapped (paddlerec_amd/ops.py: concurrent_stream). */
int rec_stream_spin(int32_t micros, void* stream);

/* Streams confined to the compute units [cu_begin, cu_end) of the current device (bit i of the HSA CU mask;
 * gfx950 has 256).  The row-sharded step partitions the chip for its tail: the HBM / xGMI bound chain (gradient
 * all-to-all, sparse Adam, next lookup) on a few CUs, the MFMA-bound dW GEMMs on the rest — two kernels that
 * merely share all CUs do not co-schedule (the GEMM's long-lived blocks hold every wave slot).  The stream is a
 * plain hipStream_t owned by the caller: rec_stream_destroy when done. */
int rec_stream_create_cu_range(int32_t cu_begin, int32_t cu_end, void** stream);
/* ... or to every `stride`-th compute unit starting at `first` (bits first, first + stride, ... < cu_total of the HSA CU
 * mask): a share of the chip that takes the same number of CUs from every XCD whatever the bit -> XCD layout is
 * (workgroup b runs on XCD b % 8, so a contiguous range would starve one XCD's share of every other kernel). */
int rec_stream_create_cu_stride(int32_t first, int32_t stride, int32_t cu_total, void** stream);
int rec_stream_destroy(void* stream);

/* ------------------------------------------------------------------------------------------
 * The tail of a CTR tower and its backward in ONE pass over the last hidden activation h [batch, n] (behind a ReLU):
 *   y_dnn = h @ w + bias;  logit = y1 + y2 + y_dnn (y1 / y2 may be NULL);  pred = sigmoid(clip(logit));
 *   loss = mean(log_loss(pred, label, eps));   dz = d loss / d logit;
 *   dx[b,j] = (relu == 0 || h[b,j] > 0) ? dz[b] * w[j] : 0;   dw[j] = sum_b h[b,j] dz[b];   db = sum_b dz[b]
 * = deepfm/net.py:169-174 (the last Linear(400, 1)) + dygraph_model.py:76-85 (sigmoid, log_loss, mean) forward, and
 * the backward of both, i.e. what rec_gemm_f32 (one output column) + rec_sigmoid_logloss + rec_mlp_head_bwd do in five
 * launches and two passes over h.  Same arithmetic per element as those entry points (eps, clip and mean_over as in
 * rec_sigmoid_logloss); the reductions (loss, dw, db) run in a fixed order of their own.  n % 4 == 0, n <= 512, act / dx /
 * w 16-byte aligned.  y_dnn may be NULL. */
int rec_ctr_head_workspace_bytes(int64_t batch, int32_t n, size_t* bytes);
int rec_ctr_head_fwd_bwd(int64_t batch, int32_t n, int64_t mean_over, const float* act, int64_t ld_act, const float* w,
                         const float* bias, const float* y1, const float* y2, const int64_t* label, float eps,
                         float clip_lo, float clip_hi, int32_t relu, float* y_dnn, float* pred, float* dz,
                         float* loss_out, float* dx, int64_t ld_dx, float* dw, float* db, void* workspace,
                         size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * The WHOLE DeepFM train step behind one entry point: what `dy_model.train_forward` + `loss.backward()` +
 * `optimizer.step()` do per batch in tools/trainer.py:148-152 for models/rank/deepfm (net.py:21-174,
 * dygraph_model.py:76-88) — FM lookup and interactions, the top MLP forward, sigmoid + log-loss (+ the AUC buckets),
 * the MLP backward, the FM backward, the merged lazy-Adam update of both embeddings and Adam on the dense parameters.
 * It issues, on ONE stream, exactly the rec_* calls of this header that the Python mirror (paddlerec_amd/deepfm.py)
 * issues for a step it records into a call list (paddlerec_amd/plan.py): same kernels, same arguments, same order —
 * results are bit-identical to that path (tests/test_deepfm_step_c.py).  A binder that is not Python gets the
 * launch-bound small-batch step (the reference's bigdata batch size 512: ~40 dependent launches) without paying a
 * foreign-function round trip per launch.  At B * num_slots <= 15360 the SelectedRows merge happens inside the
 * record update (rec_sparse_adam_record_small); larger batches group their ids first (rec_ids_group_slots when
 * slot_rows > 0, else rec_ids_group_payload).  At those launch-bound sizes, when the merge runs by row buckets, the
 * entry point goes one step further than the call list: the folds of the head's and the FM backward's partial sums,
 * the folded layer 0's backward and rec_adam_dense run as ROLES of the row update's launch, layer 0's weight fold
 * behind the lookup's blocks (csrc/tail_roles.h: every value by the statements of the stand-alone kernel, the
 * parameters dealt out by owner) — 10 launches instead of 16, the same bits (REC_SMALL_TAIL=0: the call list).  side_stream (may be NULL: everything on `stream`): a second stream of
 * the caller's on which the entry point runs the mirror's large-batch schedule — the id grouping forked in front of the
 * lookup, the sparse update underneath the dW_0 GEMM — ordered against `stream` with events; on return both streams'
 * work is ordered before anything the caller issues on `stream` next.  One step at a time per process.
 *
 * rec_deepfm_net describes the model the way the reference's state_dict does, as pointers into caller-owned device
 * memory: the table as 128-B-line records rec [table_rows, rec_stride] = W(dim) | W1 | m1 | v1 | pad with the
 * second-order moments in mv [table_rows, mv_stride] = m(dim) | v(dim) at v_offset, and the dense parameters as views
 * into ONE flat buffer (flat_param, with flat_grad / flat_m / flat_v of the same length) that rec_adam_dense walks once.
 * Linear i has weight w[i] [in_i, widths[i]] (Paddle layout) and bias b[i]; in_0 = (num_slots + dense_dim) * dim,
 * widths[n_linear - 1] = 1.  With 0 < dense_dim <= dim the step runs layer 0 on folded weights (rec_deepfm_desc
 * .compact_dense = 1): w0_folded [(num_slots + 1) * dim, widths[0]] is scratch that the CALLER zero-initialises once
 * (its last dim - dense_dim rows stay zero). */
#define REC_DEEPFM_MAX_LINEAR 8
typedef struct {
  int32_t num_slots, dim, dense_dim, n_linear;
  int32_t widths[REC_DEEPFM_MAX_LINEAR];
  int64_t table_rows;          /* rows of rec / mv */
  int64_t num_rows;            /* logical rows of the id space after slot offsets (= table_rows unless sharded) */
  int64_t padding_idx;         /* < 0: none */
  int64_t slot_rows;           /* > 0: slot s owns rows [s * slot_rows, (s + 1) * slot_rows) (slot-local grouping) */
  const int64_t* slot_offset;  /* device [num_slots] or NULL */
  float* rec;
  int32_t rec_stride;
  float* mv;
  int32_t mv_stride, v_offset;
  float *dense_w, *dense_w_one;          /* [dense_dim, dim], [dense_dim] */
  float *g_dense_w, *g_dense_w_one;      /* their gradient views */
  float* w[REC_DEEPFM_MAX_LINEAR];
  float* b[REC_DEEPFM_MAX_LINEAR];
  float* gw[REC_DEEPFM_MAX_LINEAR];
  float* gb[REC_DEEPFM_MAX_LINEAR];
  float *flat_param, *flat_grad, *flat_m, *flat_v;
  int64_t flat_numel;
  float* w0_folded;            /* compact mode (see above) and layer0_width > 0 */
  int32_t layer0_width;        /* 0, or a padded input width of layer 0 >= (num_slots + dense_dim) * dim for nets without
                                  the dense fold (dense_dim > dim): the step keeps feat at this sample stride
                                  (rec_deepfm_desc.feat_stride) and runs layer 0 on w0_folded [layer0_width, widths[0]],
                                  a zero-initialised buffer of the caller's whose leading rows it refreshes from w[0]
                                  every step — 39 fields x D 10 = 390 columns become 400, whole GEMM tiles.
                                  w0_folded == w[0] says the caller keeps layer0_width rows behind BOTH w[0] and gw[0]
                                  (the extra rows zero, inside the flat buffers): the step then copies nothing and
                                  writes dW_0 [layer0_width, widths[0]] straight into gw[0] (its extra rows come out
                                  exactly zero, so they stay zero under rec_adam_dense) */
} rec_deepfm_net;
int rec_deepfm_train_step_workspace_bytes(const rec_deepfm_net* net, int64_t batch, size_t* bytes);
/* ids [batch, num_slots] i64, dense [batch, dense_dim] f32, label [batch] i64 -> loss_out [1], pred_out [batch];
 * hyper->step is Adam's 1-based step count.  auc_pos / auc_neg [num_thresholds + 1] i64 or NULL (no metric).
 * status: the sticky out-of-range flag of the lookups (may be NULL). */
int rec_deepfm_train_step(const rec_deepfm_net* net, int64_t batch, const int64_t* ids, const float* dense,
                          const int64_t* label, const rec_adam_hyper* hyper, int64_t* auc_pos, int64_t* auc_neg,
                          int32_t num_thresholds, float* loss_out, float* pred_out, int32_t* status, void* workspace,
                          size_t workspace_bytes, void* stream, void* side_stream);

/* ------------------------------------------------------------------------------------------
 * The whole DIN train step behind one call — the per-batch body of tools/trainer.py:148-152 for models/rank/din:
 * train_forward (din/dygraph_model.py:85-100 = net.py:139-184 + binary_cross_entropy_with_logits), loss.backward(),
 * SGD step (din/dygraph_model.py:64-73; the learning rate of PiecewiseDecay is the caller's: `lr`).  Issues the ~25
 * rec_* calls of paddlerec_amd/din.py:_step on `stream` (csrc/din_step.hip), bit-identical to it; at the reference's batch
 * size (din/config.yaml: 32) the seven embedding updates are one rec_sparse_sgd_small_multi launch, larger batches sort.
 * All pointers are device memory the caller owns: seven contiguous [rows, dim] tables (three item tables, three category
 * tables, item_b [item_rows, 1]: independent parameters), the frozen attention MLP (att_w1 [4E, h1] AND
 * its transpose att_w1_t [h1, 4E] — rec_transpose_f32 makes one —, b1, w2 [h1, h2], b2, w3 [h2], b3: not registered
 * parameters in the reference's dygraph mode, App. B-9), the four registered Linear layers as [in, out] + bias with their
 * gradient buffers, and the flat parameter / gradient buffers holding those eight tensors (rec_sgd_dense walks them).
 * ---------------------------------------------------------------------------------------- */
typedef struct {
  int32_t item_dim, cat_dim;            /* E = item_dim + cat_dim */
  int64_t item_rows, cat_rows;
  int32_t att_hidden1, att_hidden2;     /* attention MLP 4E -> h1 -> h2 -> 1 (80, 40) */
  int32_t mlp_hidden1, mlp_hidden2;     /* top MLP 2E -> m1 -> m2 -> 1 (80, 40), sigmoid */
  float *w_hist_item, *w_hist_cat, *w_tgt_item_seq, *w_tgt_cat_seq, *w_tgt_item, *w_tgt_cat, *w_item_b;
  const float *att_w1, *att_w1_t, *att_b1, *att_w2, *att_b2, *att_w3, *att_b3;
  float *w_con, *b_con, *w_l0, *b_l0, *w_l1, *b_l1, *w_l2, *b_l2;                  /* linearCon [E,E], linear_0..2 */
  float *g_w_con, *g_b_con, *g_w_l0, *g_b_l0, *g_w_l1, *g_b_l1, *g_w_l2, *g_b_l2;  /* their gradients (written) */
  float *flat_param, *flat_grad;
  int64_t flat_numel;
} rec_din_net;
int rec_din_train_step_workspace_bytes(const rec_din_net* net, int64_t batch, int32_t max_len, size_t* bytes);
/* hist_item / hist_cat / target_item_seq / target_cat_seq / mask [batch, max_len] i64 (mask 0 valid, -1e9 padding),
 * target_item / target_cat [batch] i64, label [batch] f32 -> loss_out [1] (mean BCE), pred_out [batch] = sigmoid(logit).
 * status: the sticky out-of-range flag of the lookups.
 * side_stream (NULL or == stream: everything on `stream`): batches above the one-launch merge group the merge keys of the
 * four [batch, max_len] tables on it from the start of the step and update two of the four tables on it behind the
 * backward (batch 4096: 1.72 -> 1.47 ms at max_len 100); joined into `stream` before the call returns.  Same result. */
int rec_din_train_step(const rec_din_net* net, int64_t batch, int32_t max_len, const int64_t* hist_item,
                       const int64_t* hist_cat, const int64_t* target_item, const int64_t* target_cat, const float* label,
                       const int64_t* mask, const int64_t* target_item_seq, const int64_t* target_cat_seq, float lr,
                       float* loss_out, float* pred_out, int32_t* status, void* workspace, size_t workspace_bytes,
                       void* stream, void* side_stream);

/* ------------------------------------------------------------------------------------------
 * The whole DCN-v2 train step behind one call — the per-batch body of tools/trainer.py:148-152 for models/rank/dcn_v2:
 * train_forward (dcn_v2/dygraph_model.py:103-127 = net.py:89-137: lookup + dense_emb Linear, CrossNetV2 or CrossNetMix,
 * the DNN tower with its train-mode Dropout pairs, the stacked or the parallel head, log_loss), loss.backward(), Adam with
 * ClipGradByGlobalNorm and L2Decay on the DNN weights (dygraph_model.py:73-88, net.py:164-170).  Issues the rec_* calls of
 * paddlerec_amd/dcn_v2.py:train_step on `stream` (csrc/dcn_v2_step.hip), bit-identical to it, for all four structures
 * (is_stacked x low_rank_mix) with and without dropout.  All pointers are device memory the caller owns: the table as
 * [num_rows, emb_stride] with its Adam moments [num_rows, state_stride], every dense parameter as Paddle's [in, out] with
 * its gradient buffer, and the flat buffers holding all dense parameters / gradients / moments in one order
 * (rec_adam_dense and rec_sumsq walk them).
 * ---------------------------------------------------------------------------------------- */
#define REC_DCN_MAX_LAYERS 8
typedef struct {
  int32_t num_slots, dim, dense_dim;    /* S, D, Dn: d = (S + Dn) * D */
  int64_t num_rows, padding_idx;        /* padding_idx < 0: none (net.py:45-54 uses 0) */
  int32_t emb_stride, state_stride;     /* row strides (floats) of emb and of emb_m / emb_v */
  float *emb, *emb_m, *emb_v;
  int32_t cross_num, n_dnn;             /* <= REC_DCN_MAX_LAYERS each */
  int32_t widths[REC_DCN_MAX_LAYERS];   /* layer_sizes of the DNN tower */
  int32_t is_stacked, low_rank_mix;     /* net.py:110-137 stacked / parallel; CrossNetV2 / CrossNetMix */
  int32_t num_experts, low_rank;        /* CrossNetMix only */
  float dropout_rate;                   /* 0: no dropout (eval-mode tower) */
  float l2_dnn, clip_norm;              /* 0: off */
  uint64_t dropout_seed;                /* mask streams of layer i at Adam step t: (t * n_dnn + i) * 2 and + 1 */
  float *dense_emb_w, *dense_emb_b, *g_dense_emb_w, *g_dense_emb_b;   /* Linear(Dn -> D*Dn) */
  float *cross_w[REC_DCN_MAX_LAYERS], *cross_b[REC_DCN_MAX_LAYERS];   /* CrossNetV2 [d,d], [d] */
  float *g_cross_w[REC_DCN_MAX_LAYERS], *g_cross_b[REC_DCN_MAX_LAYERS];
  float *mix_u[REC_DCN_MAX_LAYERS], *mix_v[REC_DCN_MAX_LAYERS], *mix_c[REC_DCN_MAX_LAYERS], *mix_bias[REC_DCN_MAX_LAYERS];
  float *g_mix_u[REC_DCN_MAX_LAYERS], *g_mix_v[REC_DCN_MAX_LAYERS], *g_mix_c[REC_DCN_MAX_LAYERS],
      *g_mix_bias[REC_DCN_MAX_LAYERS];                                /* CrossNetMix [E,d,r], [E,d,r], [E,r,r], [d] */
  float *gate_w, *gate_b, *g_gate_w, *g_gate_b;                       /* the E gating Linear(d,1) stacked: [d,E], [E] */
  float *dnn_w[REC_DCN_MAX_LAYERS], *dnn_b[REC_DCN_MAX_LAYERS], *g_dnn_w[REC_DCN_MAX_LAYERS], *g_dnn_b[REC_DCN_MAX_LAYERS];
  float *fc_w, *fc_b, *g_fc_w, *g_fc_b;                               /* [widths[n-1] (+ d when parallel), 1], [1] */
  float *flat_param, *flat_grad, *flat_m, *flat_v;
  int64_t flat_numel;
} rec_dcn_v2_net;
int rec_dcn_v2_train_step_workspace_bytes(const rec_dcn_v2_net* net, int64_t batch, size_t* bytes);
/* ids [batch, num_slots] i64, dense [batch, dense_dim] f32, label [batch] i64 -> loss_out [1], pred_out [batch];
 * hyper->step = the Adam step count t (1-based; also keys the dropout masks); auc_pos / auc_neg i64
 * [num_thresholds + 1] or NULL. */
int rec_dcn_v2_train_step(const rec_dcn_v2_net* net, int64_t batch, const int64_t* ids, const float* dense,
                          const int64_t* label, const rec_adam_hyper* hyper, int64_t* auc_pos, int64_t* auc_neg,
                          int32_t num_thresholds, float* loss_out, float* pred_out, int32_t* status, void* workspace,
                          size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * FFM: field-aware factorisation machine, models/rank/ffm/net.py:90-133 (FFM.forward).
 * F = num_slots + num_dense fields, R = F * dim: each sample's feature cube E [F, R] holds the table rows
 * W[id_s] (s < S) and the dense rows dense[b,k] * dense_w[k, :]; E[i, j*dim .. +dim) is field i's vector
 * for partner field j.
 *   y1[b] = sum_s W1[id_s] + sum_k dense[b,k] * dense_w_one[k]
 *   y2[b] = sum_{i<j} <E[i, j, :], E[j, i, :]>
 * Built for F <= 64 and dim <= 32 (REC_ESHAPE otherwise, before any launch).  An id outside [0, num_rows)
 * ORs REC_FLAG_INDEX_OOB into status and reads as a zero row.  When row_stride % 4 == 0 the kernels may read a
 * row's pad columns [R, round_up(R, 4)) (their values are ignored).
 * ---------------------------------------------------------------------------------------- */
typedef struct {
  int64_t batch;       /* B */
  int32_t num_slots;   /* S  (26): sparse fields, one id each */
  int32_t num_dense;   /* Dn (13): dense fields */
  int32_t dim;         /* D  (9) */
  int64_t num_rows;    /* N rows in W / W1 */
  int32_t row_stride;  /* floats between consecutive rows of W (>= R; 352 for R 351) */
  int32_t grad_stride; /* floats between consecutive rows of row_grad (>= R); the pad columns are written 0 */
} rec_ffm_desc;

/* ids [B,S] i64; dense [B,Dn]; W [N,row_stride]; W1 [N]; dense_w [Dn,R]; dense_w_one [Dn] -> y1, y2 [B] */
int rec_ffm_fwd(const rec_ffm_desc* desc, const int64_t* ids, const float* dense, const float* W, const float* W1,
                const float* dense_w, const float* dense_w_one, float* y1, float* y2, int32_t* status, void* stream);
/* Backward for dz [B] = dloss/d(y1 + y2 + bias):
 *   row_grad [B*S, grad_stride] — SelectedRows.value of `embedding`, unmerged, in position order:
 *     row b*S+i = dE[i] with dE[i, j, :] = dz * E[j, i, :] (j != i) and dE[i, i, :] = 0;
 *   d_dense_w [Dn,R] = sum_b dense[b,k] * dE_b[S+k],  d_dense_w_one [Dn] = sum_b dz[b] * dense[b,k] —
 *     per-block partials folded in a fixed order (two runs are bit-identical).
 * The SelectedRows value of `embedding_one` is dz[b] for every (b,s); it is not materialised (read dz through
 * rec_grad_layout{S,0,0}, as for rec_deepfm_fm_bwd). */
int rec_ffm_bwd_workspace_bytes(const rec_ffm_desc* desc, size_t* bytes);
int rec_ffm_bwd(const rec_ffm_desc* desc, const int64_t* ids, const float* dense, const float* W,
                const float* dense_w, const float* dz, float* row_grad, float* d_dense_w, float* d_dense_w_one,
                void* workspace, size_t workspace_bytes, int32_t* status, void* stream);

/* ------------------------------------------------------------------------------------------
 * FAT-DeepFFM: CENet attention over the cube slices + attention-scaled field-pair Hadamard features,
 * models/rank/fat_deepffm/net.py:105-151 (CENLayer.forward) and :219-251 (DeepFFM.forward, is_H).
 * The cube E, F and R are FFM's (above), as are the limits (F <= 64, dim <= 32: REC_ESHAPE before any launch) and the
 * handling of an id outside [0, num_rows).  F2 = F*F slices q = i*F + j with mirror q' = j*F + i; P = F (F - 1) / 2
 * pairs p = (i, j), i < j, in nested-loop order.
 *   pooled[b,q]    = max_d E[q, d]
 *   (the caller:     a = relu(relu(pooled @ W_red + b_red) @ W_add + b_add), two GEMMs)
 *   y1[b]          = sum_q a[b,q] * sum_d E[q, d]                     (the diagonal slices included)
 *   H[b, p*dim+d]  = a[b,q] E[q, d] * a[b,q'] E[q', d]
 * Backward for dz [B] = dloss/dlogit and dH = dloss/dH:
 *   t[q, d]        = dz + dH[p*dim+d] * a[q'] * E[q', d]  (i != j),   dz  (i == j)
 *   d_a[b,q]       = sum_d E[q, d] * t[q, d]
 *   dE[q, d]       = a[q] * t[q, d] + (d == argmax_d E[q, :]) * d_pooled[b,q]
 * The argmax is the smallest d among equal maxima; it is recomputed from the cube (no index tensor is stored).
 * ---------------------------------------------------------------------------------------- */
typedef struct {
  rec_ffm_desc ffm;   /* grad_stride is read by rec_fatffm_bwd only */
  int64_t ld_attn;    /* floats between consecutive rows of pooled / a / d_a / d_pooled (>= F2) */
  int64_t ld_pair;    /* floats between consecutive rows of H / dH (>= P*dim) */
} rec_fatffm_desc;

/* ids [B,S] i64; dense [B,Dn]; W [N,row_stride]; dense_w [Dn,R] -> pooled [B,ld_attn] */
int rec_fatffm_pool_fwd(const rec_fatffm_desc* desc, const int64_t* ids, const float* dense, const float* W,
                        const float* dense_w, float* pooled, int32_t* status, void* stream);
/* the same inputs + a [B,ld_attn] -> H [B,ld_pair], y1 [B].  The rows are gathered again: the cube is never stored. */
int rec_fatffm_inter_fwd(const rec_fatffm_desc* desc, const int64_t* ids, const float* dense, const float* W,
                         const float* dense_w, const float* a, float* H, float* y1, int32_t* status, void* stream);
/* the inputs + a, dH [B,ld_pair], dz [B] -> d_a [B,ld_attn] (before the ReLU mask a > 0, which is the caller's) */
int rec_fatffm_attn_bwd(const rec_fatffm_desc* desc, const int64_t* ids, const float* dense, const float* W,
                        const float* dense_w, const float* a, const float* dH, const float* dz, float* d_a,
                        int32_t* status, void* stream);
/* the inputs + a, dH, dz, d_pooled [B,ld_attn] ->
 *   row_grad [B*S, grad_stride] — SelectedRows.value of `embedding`, unmerged, in position order: row b*S+i = dE_b[i],
 *     written once and complete, 0 on the pad columns [R, grad_stride);
 *   d_dense_w [Dn,R] = sum_b dense[b,k] * dE_b[S+k] — per-block partials folded in block order (two runs are
 *     bit-identical). */
int rec_fatffm_bwd_workspace_bytes(const rec_fatffm_desc* desc, size_t* bytes);
int rec_fatffm_bwd(const rec_fatffm_desc* desc, const int64_t* ids, const float* dense, const float* W,
                   const float* dense_w, const float* a, const float* dH, const float* dz, const float* d_pooled,
                   float* row_grad, float* d_dense_w, void* workspace, size_t workspace_bytes, int32_t* status,
                   void* stream);

/* ------------------------------------------------------------------------------------------
 * FEFM: field-embedded factorisation machine, models/rank/deepfefm/net.py:118-187 (FEFM.forward).
 * F = num_slots + num_dense fields, P = F (F - 1) / 2 pairs p = (i, j), i < j, in itertools.combinations order.
 *   id[b,f]   = ids[b,f] (f < S),  int64(dense[b,f-S] * 1e5 + 1e6 + 2) (f >= S: three rounded f32 operations, truncated)
 *   x[b,f,:]  = W[id[b,f], 0:dim]   (0 where id == 0: padding_idx)
 *   y1[b]     = sum_{f<S} W1[id[b,f]] (0 where id == 0) + sum_k dense[b,k] * dense_w_one[k]
 *   t[b,p]    = x[b,i,:]^T (FE_p + FE_p^T) x[b,j,:],   y2[b] = sum_p t[b,p]
 *   dnn_in[b] = [ x[b, 0:S, :] (S*dim) | dense[b,:] * dense_w_one (Dn) | t[b,:] (P) ]   at row stride ld
 * Built for 2 <= F <= 64, dim <= 64, num_rows < 2^31 (REC_ESHAPE otherwise, before any launch).  An id outside
 * [0, num_rows) — a derived one included: negative, huge or NaN dense values — ORs REC_FLAG_INDEX_OOB into status and
 * reads as a zero row; it never indexes memory.  Exact f32.
 * ---------------------------------------------------------------------------------------- */
typedef struct {
  int64_t batch;       /* B */
  int32_t num_slots;   /* S  (26): sparse fields, one id each */
  int32_t num_dense;   /* Dn (13): dense fields, looked up in W through the derived id */
  int32_t dim;         /* D  (9 / 48) */
  int64_t num_rows;    /* N rows in W / W1 */
  int32_t row_stride;  /* floats between consecutive rows of W (>= D) */
  int32_t grad_stride; /* floats between consecutive rows of row_grad (>= D); the pad columns are written 0 */
  int64_t ld;          /* floats between consecutive rows of dnn_in / d_dnn_in (>= S*D + Dn + P) */
} rec_fefm_desc;

/* ids [B,S] i64; dense [B,Dn]; W [N,row_stride]; W1 [N]; dense_w_one [Dn]; FE [P,D,D] -> y1, y2 [B], dnn_in [B,ld] (the
 * three column groups, written in place), ids_all [B,F] i64 (the merge keys of the table gradient; -1 for a dense value
 * whose id is not a finite number).  workspace: rec_fefm_fwd_workspace_bytes (the symmetrised matrices, and the y2
 * partials of the blocks that share a tile when the batch has fewer tiles than the chip has CUs). */
int rec_fefm_fwd_workspace_bytes(const rec_fefm_desc* desc, size_t* bytes);
int rec_fefm_fwd(const rec_fefm_desc* desc, const int64_t* ids, const float* dense, const float* W, const float* W1,
                 const float* dense_w_one, const float* FE, float* y1, float* y2, float* dnn_in, int64_t* ids_all,
                 void* workspace, size_t workspace_bytes, int32_t* status, void* stream);
/* Backward for dz [B] = dloss / d(y1 + y2 + y_dnn) and d_dnn_in [B,ld] = dloss / d dnn_in;
 * g[b,p] = dz[b] + d_dnn_in[b, S*D + Dn + p]:
 *   row_grad [B*F, grad_stride] — SelectedRows.value of `embedding`, unmerged, in position order b*F + f:
 *     dx[b,i,:] = sum_{j != i} g[b,p(i,j)] (FE_p + FE_p^T) x[b,j,:]  (+ d_dnn_in[b, i*D .. (i+1)*D) for i < S);
 *     rows of padding positions (id == 0) and the pad columns are 0;
 *   d_dense_w_one [Dn] = sum_b (dz[b] + d_dnn_in[b, S*D + k]) * dense[b,k];
 *   d_FE [P,D,D] = sum_b g[b,p] (x_i x_j^T + x_j x_i^T), or NULL: that work is skipped.
 * Both batch sums are per-block partials folded in a fixed order (two runs are bit-identical).  The SelectedRows value
 * of `embedding_one` is dz[b] for the S sparse positions of a sample (rec_grad_layout{S,0,0} over a grouping of ids
 * [B,S]); it is not materialised. */
int rec_fefm_bwd_workspace_bytes(const rec_fefm_desc* desc, int32_t want_d_fe, size_t* bytes);
int rec_fefm_bwd(const rec_fefm_desc* desc, const int64_t* ids_all, const float* dense, const float* W, const float* FE,
                 const float* dz, const float* d_dnn_in, float* row_grad, float* d_dense_w_one, float* d_FE,
                 void* workspace, size_t workspace_bytes, int32_t* status, void* stream);

/* ------------------------------------------------------------------------------------------
 * DCN: the vector-form cross network of Deep & Cross, models/rank/dcn/net.py:117-135 (_cross_layer, _cross_net).
 * ONE weight w [d] and ONE bias b [d] are shared by all L layers:
 *   s_l[r]    = <x_l[r,:], w>                                   one scalar per sample row and layer
 *   x_{l+1}   = x_0 * s_l + b + x_l                             x_0 = the feature row, d floats (247)
 *   l2        = l2_coeff * sum_l sum_{r,k} (x_l[r,k] * w[k])^2  a sum over the batch, not a mean
 * The whole stack runs in one pass over a row: one 64-lane wave per row keeps x_0, x_l, w and b in registers.
 * Built for 1 <= d <= 512 (any d, multiple of 4 or not) and 1 <= num_layers <= 64; anything else, or a row stride
 * below d, is REC_EINVAL before any launch.  batch == 0 is a no-op: nothing is launched and no output is written.  Rows whose base address and stride are
 * multiples of 16 bytes move as 16-byte vectors; columns at or beyond d are never read or written.  Exact f32.
 * ---------------------------------------------------------------------------------------- */
typedef struct {
  int64_t batch;          /* B */
  int32_t d;              /* floats per row (S*D + Dn = 247) */
  int32_t num_layers;     /* L (cross_num: 2) */
  int64_t ld_x0;          /* floats between consecutive rows of X0 (>= d) */
  int64_t ld_out;         /* ... of the forward's XL (>= d): XL may be a column block of a wider buffer */
  int64_t ld_dxl;         /* ... of the backward's dXL (>= d; ignored by the rank-1 form) */
  int64_t ld_dx0;         /* ... of the backward's dX0 (>= d) */
  float l2_coeff;         /* coefficient of the l2 term in the loss (the reference: 1); 0 skips its arithmetic */
  int32_t accumulate_dx0; /* backward: 0 = dX0 is written, 1 = dX0 += (the DNN's layer-0 dX is already there) */
} rec_dcn_cross_desc;

/* Bytes of `workspace` for one shape: the backward's per-block partials of d_w / d_b; the forward's per-block l2
 * partials fit in the same figure.  Both calls hold the caller to this ONE figure: fewer bytes are REC_EWORKSPACE. */
int rec_dcn_cross_bwd_workspace_bytes(const rec_dcn_cross_desc* desc, size_t* bytes);
/* X0 [B,ld_x0]; w, b [d] -> XL [B,ld_out] = x_L;  saved [B,L] = s_l[r] at r*L + l, or NULL;  l2_out [1] or NULL.
 * Inference passes saved = l2_out = NULL: nothing is stored or summed for them and no workspace is needed.  With l2_out
 * the workspace is required; the per-block partials are folded in block order (two runs are bit-identical). */
int rec_dcn_cross_fwd(const rec_dcn_cross_desc* desc, const float* X0, const float* w, const float* b, float* XL,
                      float* saved, float* l2_out, void* workspace, size_t workspace_bytes, void* stream);
/* Backward of the stack AND of its l2 term (coefficient l2_coeff) for dXL [B,ld_dxl] = dloss / d x_L.  x_1 .. x_{L-1} are
 * rebuilt in registers from X0 and `saved` (x_l = x_0 * (1 + s_0 + .. + s_{l-1}) + l * b).  With g_L = dXL and, for
 * l = L-1 .. 0,  t_l = <g_{l+1}, x_0>,  g_l = g_{l+1} + t_l * w + 2 * l2_coeff * x_l * w^2:
 *   dX0 [B,ld_dx0] (+)= g_0 + sum_l g_{l+1} * s_l                     (desc->accumulate_dx0)
 *   d_w [d] = sum_r sum_l (t_l * x_l + 2 * l2_coeff * x_l^2 * w),    d_b [d] = sum_r sum_l g_{l+1}
 * d_w / d_b are per-block partials over a fixed row range, folded in block order (two runs are bit-identical).
 * Rank-1 form: dXL == NULL with dz [B] and u [d] non-NULL reads the upstream gradient as dz[r] * u[k] (the one-logit
 * head behind the stack: u = the tail of fc.weight) — no [B,d] matrix is made or read.  Otherwise dz / u are ignored. */
int rec_dcn_cross_bwd(const rec_dcn_cross_desc* desc, const float* X0, const float* w, const float* b,
                      const float* saved, const float* dXL, const float* dz, const float* u, float* dX0, float* d_w,
                      float* d_b, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * GateNet: the embedding gate and the hidden gate of models/rank/gatenet/net.py:88-118.
 * Embedding gate, field s of S, e = W[id] (D floats), ONE scalar weight w_s per field:
 *   t = sum_k e_k,   a = sigmoid(w_s * t),   out = e * a
 * Lookup i of n = B * S (field s = i % S, sample i / S) lives at  base + (i / S) * stride + s * D  (floats) on the
 * output side — the head of a feature row of S*D + Dn floats, whose dense columns and padding floats are never
 * touched.  An id outside [0, num_rows) gives a zero row and raises REC_FLAG_INDEX_OOB in *status; id == padding_idx
 * (-1: none) gives a zero row.  Rows whose base addresses and strides (table and output) are multiples of 16 bytes move
 * as 16-byte vectors when emb_dim % 4 == 0, anything else lane by lane.  n must be a multiple of num_fields, the output
 * stride at least num_fields * emb_dim: otherwise REC_EINVAL before any launch.  n == 0 launches nothing.  Exact f32.
 * ---------------------------------------------------------------------------------------- */
int rec_gate_emb_fwd(int64_t n, int32_t num_fields, int32_t emb_dim, int32_t row_stride, int64_t num_rows,
                     int64_t padding_idx, const int64_t* ids, const float* W, const float* gate_w, float* out,
                     int64_t out_stride, int32_t* status, void* stream);
/* Bytes of `workspace` for rec_gate_emb_bwd: its per-block partials of d_gate_w (at most 2048 blocks of num_fields).
 * The call holds the caller to this figure whatever lane shape runs: fewer bytes are REC_EWORKSPACE before any launch. */
int rec_gate_emb_bwd_workspace_bytes(int64_t n, int32_t num_fields, size_t* bytes);
/* Backward of the gate, IN PLACE on g (the layout of `out` above, stride g_stride): on entry g = dloss / d out, on
 * return g = dloss / d e.  e is gathered again from W (not yet updated), t and a are recomputed:
 *   da = <g, e>,   dp = da * a * (1 - a),   d e_k = g_k * a + dp * w_s,   d_gate_w[s] = sum over the batch of dp * t
 * Padding and out-of-range lookups get a zero row (the latter raise the flag).  d_gate_w [num_fields] is summed without
 * float atomics — per-block partials over fixed lookup ranges, folded in block order — so two runs are bit-identical;
 * n == 0 writes zeros to it (when non-NULL).  num_fields <= 1024. */
int rec_gate_emb_bwd(int64_t n, int32_t num_fields, int32_t emb_dim, int32_t row_stride, int64_t num_rows,
                     int64_t padding_idx, const int64_t* ids, const float* W, const float* gate_w, float* g,
                     int64_t g_stride, float* d_gate_w, int32_t* status, void* workspace, size_t workspace_bytes,
                     void* stream);
/* Hidden gate x = y * tanh(y @ G), elementwise over [batch, n] with row strides ld_* (floats, >= n); the two GEMMs
 * around it are rec_gemm_f32 calls.  Forward: t = y @ G on entry; x = y * tanh(t) is written and t is overwritten with
 * h = tanh(t), which the backward reads. */
int rec_gate_hidden_fwd(int64_t batch, int32_t n, const float* y, int64_t ld_y, float* t, int64_t ld_t, float* x,
                        int64_t ld_x, void* stream);
/* Backward for upstream u = dloss / d x:  dt = u * y * (1 - h^2)  (-> dG = y^T dt, and dt @ G^T into dy)  and the direct
 * term  uh = u * h.  The outputs alias nothing. */
int rec_gate_hidden_bwd(int64_t batch, int32_t n, const float* u, int64_t ld_u, const float* y, int64_t ld_y,
                        const float* h, int64_t ld_h, float* dt, int64_t ld_dt, float* uh, int64_t ld_uh, void* stream);
/* dy[r,c] = y[r,c] > 0 ? dy[r,c] : 0 — the ReLU in front of the gate; the mask is y's (the gated x can be <= 0 where y
 * is positive).  Floats between the rows are not touched. */
int rec_relu_mask_inplace(int64_t batch, int32_t n, float* dy, int64_t ld_dy, const float* y, int64_t ld_y,
                          void* stream);

/* ------------------------------------------------------------------------------------------
 * FLEN: the field-wise bi-interaction of models/rank/flen/net.py:79, 205-229, fused into the lookup.
 * ids [batch, num_slots] index ONE table W (raw ids, no padding row).  The slots are partitioned into num_groups field
 * groups: group g owns the slots [group_begin[g], group_begin[g + 1]); group_begin is a HOST array of num_groups + 1
 * ints that runs from 0 to num_slots with no empty group (checked before any launch).  2 <= num_groups <=
 * REC_FLEN_MAX_GROUPS, num_slots >= num_groups, emb_dim >= 1 (<= 64, or <= 256 with emb_dim % 4 == 0), and one sample's
 * (num_slots + num_groups + 1) * emb_dim floats must fit 64 KB of LDS.  With E[b,s] = W[ids[b,s]] (a zero row for an id
 * outside [0, num_rows), which raises REC_FLAG_INDEX_OOB in *status) and the pairs p = (i < j) of groups in
 * itertools.combinations order:
 *   X0 [batch, x0_stride]      X0[b, s*D:(s+1)*D] = E[b,s]            the DNN input; floats behind S*D are not touched
 *   FW [batch, num_groups*D]   FW[b,g] = sum of E[b,s] over the slots of group g, in slot order (kept for the backward)
 *   h_mf [batch, h_stride]     h_mf[b] = sum_p kernel_mf[p] * FW[b,i] * FW[b,j]   (floats behind D are not touched)
 * kernel_mf [P = num_groups * (num_groups - 1) / 2] is a device pointer.  Rows whose base addresses and strides (table
 * and X0) are multiples of 16 bytes move as 16-byte vectors when emb_dim % 4 == 0, anything else lane by lane.
 * batch == 0 launches nothing.  Exact f32, fixed summation order.
 * ---------------------------------------------------------------------------------------- */
#define REC_FLEN_MAX_GROUPS 8
int rec_flen_fwd(int64_t batch, int32_t num_slots, int32_t num_groups, int32_t emb_dim, int32_t row_stride,
                 int64_t num_rows, const int64_t* ids, const float* W, const int32_t* group_begin, const float* kernel_mf,
                 float* X0, int64_t x0_stride, float* h_mf, int64_t h_stride, float* FW, int32_t* status, void* stream);
/* Bytes of `workspace` for rec_flen_bwd: its per-block partials of d_kernel_mf (at most 2048 blocks of P floats). */
int rec_flen_bwd_workspace_bytes(int64_t batch, int32_t num_slots, int32_t num_groups, int32_t emb_dim, size_t* bytes);
/* Backward, IN PLACE on g (the layout of X0 above, stride g_stride) and without the table: on entry g = dloss / d X0
 * (the layer-0 dX), on return the per-lookup row gradient
 *   g[b,s] = g[b,s] + dH[b] * sum over g' != g(s) of kernel_mf[pair(g(s), g')] * FW[b,g']
 * where dH [batch, dh_stride] = dloss / d h_mf and FW is the forward's.  An id outside [0, num_rows) gets a zero row
 * (and raises the flag).  d_kernel_mf[p] = sum over b, d of dH * FW[b,i] * FW[b,j] is summed without float atomics —
 * per-block partials over fixed sample ranges, folded in block order — so two runs are bit-identical; batch == 0 writes
 * zeros to it.  g aliases neither FW nor dH. */
int rec_flen_bwd(int64_t batch, int32_t num_slots, int32_t num_groups, int32_t emb_dim, int64_t num_rows,
                 const int64_t* ids, const int32_t* group_begin, const float* kernel_mf, const float* FW, const float* dH,
                 int64_t dh_stride, float* g, int64_t g_stride, float* d_kernel_mf, int32_t* status, void* workspace,
                 size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * paddle.optimizer.Adagrad [EXT] (flen/dygraph_model.py:68-72):
 *   acc += g * g;   p -= lr * g / (sqrt(acc) + epsilon)
 * (not the PS accessor's rule of rec_sparse_adagrad_rows, which keeps one g2sum per row part).  The accumulator starts
 * at initial_accumulator_value: the caller fills it when it creates it.  g == 0 leaves p and acc bit-unchanged, so
 * there is no lazy / non-lazy distinction.
 * rec_adagrad_rows: the rule on the MERGED gradient of every unique row of a grouping (rec_ids_group: duplicates are
 * summed first, in position order, as Paddle merges a SelectedRows gradient: (sum g)^2, not sum g^2).  Arguments as
 * rec_sparse_adam_rows: grad_layout may carry the hot-row partials of rec_segment_partials; A [.., state_stride] is the
 * accumulator table (state_stride <= 0: row_stride).  Untouched rows are not read or written.
 * rec_adagrad_dense: the rule over n floats of a flat buffer (p, acc and g are three buffers).
 * ---------------------------------------------------------------------------------------- */
int rec_adagrad_rows(int64_t n_max, int32_t emb_dim, int32_t row_stride, int32_t state_stride, const int32_t* n_uniq,
                     const int64_t* uniq_rows, const int32_t* seg_offset, const int32_t* sorted_pos, const float* grad,
                     const rec_grad_layout* grad_layout, float* P, float* A, float lr, float epsilon, void* stream);
int rec_adagrad_dense(int64_t n, float* p, float* acc, const float* g, float lr, float epsilon, void* stream);

/* ------------------------------------------------------------------------------------------
 * AutoFIS (models/rank/autofis/net.py:78-99): the second-order term of AutoDeepFMLayer, fused into the lookup.
 * ids [batch, num_fields] index the tables V [num_rows, row_stride] (emb_dim floats of a row) and W1 [num_rows, w_stride]
 * (one float of a row); neither has a padding row; an id outside [0, num_rows) reads as a zero row and raises
 * REC_FLAG_INDEX_OOB in *status.  The pair list is two HOST int32 arrays cols[num_pairs], rows[num_pairs] with
 * 0 <= cols[p] < rows[p] < num_fields (checked on every call before any launch), plus plan_dev, the DEVICE copy of what
 * rec_autofis_plan lays out from the same list (rec_autofis_plan_ints int32s: cols | rows | num_fields + 1 adjacency
 * offsets | 2 num_pairs adjacency entries, partner + 256 * pair, in pair order).
 * Limits: 2 <= num_fields <= REC_AUTOFIS_MAX_FIELDS, 1 <= emb_dim <= REC_AUTOFIS_MAX_DIM, 1 <= num_pairs <=
 * min(REC_AUTOFIS_MAX_PAIRS, num_fields (num_fields - 1) / 2), batch * max(num_fields, num_pairs) < 2^31.
 *   X0[b]   = [V[ids[b,0]] | .. | V[ids[b,S-1]]]            (stride x0_stride; the rest of a row is not touched)
 *   L[b,p]  = <V[ids[b,cols[p]]], V[ids[b,rows[p]]]>        (stride l_stride >= num_pairs)
 *   s[b]    = sum_s W1[ids[b,s]] + sum_p mask[p] * BN_p(L[.,p])[b]
 * BN_p is Paddle's BatchNorm over the batch (biased variance).  training != 0: batch statistics -> save_mean,
 * save_invstd [num_pairs]; running = momentum * running + (1 - momentum) * batch; L is written (the backward reads it).
 * The statistics are (count, mean, M2) partials of fixed sample sets merged with Chan's formula in a fixed order — never
 * sum x^2 - mean^2.  training == 0: the running statistics, one launch; L is written only if want_L != 0.  The BatchNorm
 * output is never stored.  Rows of V and X0 that are multiples of 16 bytes move as 16-byte vectors when emb_dim % 4 == 0.
 * batch == 0 launches nothing.  Fixed summation order: two runs give the same bits.
 * ---------------------------------------------------------------------------------------- */
#define REC_AUTOFIS_MAX_FIELDS 64
#define REC_AUTOFIS_MAX_DIM 64
#define REC_AUTOFIS_MAX_PAIRS 2016
int rec_autofis_plan_ints(int32_t num_fields, int32_t num_pairs, size_t* ints);
/* Host only: validates the pair list and writes its device image into plan (host memory, rec_autofis_plan_ints ints). */
int rec_autofis_plan(int32_t num_fields, int32_t num_pairs, const int32_t* cols, const int32_t* rows, int32_t* plan);
int rec_autofis_fwd_workspace_bytes(int64_t batch, int32_t num_fields, int32_t emb_dim, int32_t num_pairs, size_t* bytes);
int rec_autofis_fwd(int64_t batch, int32_t num_fields, int32_t emb_dim, int32_t row_stride, int32_t w_stride,
                    int64_t num_rows, const int64_t* ids, const float* V, const float* W1, int32_t num_pairs,
                    const int32_t* cols, const int32_t* rows, const int32_t* plan_dev, const float* gamma,
                    const float* beta, const float* mask, float* running_mean, float* running_var, float momentum,
                    float eps, int32_t training, int32_t want_L, float* X0, int64_t x0_stride, float* L, int64_t l_stride,
                    float* s, float* save_mean, float* save_invstd, int32_t* status, void* workspace,
                    size_t workspace_bytes, void* stream);
int rec_autofis_bwd_workspace_bytes(int64_t batch, int32_t num_fields, int32_t emb_dim, int32_t num_pairs, size_t* bytes);
/* Backward of the training forward.  dz [batch] = dloss / d s; L, X0, save_mean, save_invstd are the forward's.  With
 * xhat = (L - mean) * invstd, S0 = sum_b dz[b], S1_p = sum_b dz[b] * xhat[b,p] (summed centred, by row blocks in block
 * order):
 *   d_mask[p] = gamma[p] * S1_p + beta[p] * S0;   d_gamma[p] = mask[p] * S1_p;   d_beta[p] = mask[p] * S0
 *   dL[b,p]   = gamma[p] * invstd[p] * mask[p] * (dz[b] - S0 / batch - xhat[b,p] * S1_p / batch)
 * and dX [batch, dx_stride] (the layout of X0; on entry the DNN's gradient) gets, IN PLACE, for the fields f of pair p:
 *   dX[b, cols[p]] += dL[b,p] * X0[b, rows[p]];   dX[b, rows[p]] += dL[b,p] * X0[b, cols[p]]
 * added per field in pair order.  A field in no pair is not written.  The gradient of a W1 lookup is dz[b]: no kernel.
 * batch == 0 writes zeros to the three gradients.  dX aliases neither X0 nor L. */
int rec_autofis_bwd(int64_t batch, int32_t num_fields, int32_t emb_dim, int32_t num_pairs, const int32_t* cols,
                    const int32_t* rows, const int32_t* plan_dev, const float* dz, const float* L, int64_t l_stride,
                    const float* X0, int64_t x0_stride, const float* save_mean, const float* save_invstd,
                    const float* gamma, const float* beta, const float* mask, float* dX, int64_t dx_stride, float* d_mask,
                    float* d_gamma, float* d_beta, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * Linear -> BatchNorm -> ReLU (autofis/net.py:84-88; rec_batchnorm_bwd's relu_mask covers the other order, ReLU -> BN).
 * rec_batchnorm_relu_fwd: rec_batchnorm_fwd with Y = max(BN(X), 0) written by the apply pass (Y != X).
 * rec_batchnorm_relu_bwd: dY counts only where Y > 0, in the column sums and in dX; arguments and workspace
 * (rec_batchnorm_workspace_bytes) as rec_batchnorm_bwd plus Y.
 * ---------------------------------------------------------------------------------------- */
int rec_batchnorm_relu_fwd(int64_t m, int32_t n, const float* X, int64_t ldx, const float* gamma, const float* beta,
                           float* running_mean, float* running_var, float momentum, float eps, int32_t training, float* Y,
                           int64_t ldy, float* save_mean, float* save_invstd, void* workspace, size_t workspace_bytes,
                           void* stream);
int rec_batchnorm_relu_bwd(int64_t m, int32_t n, const float* X, int64_t ldx, const float* Y, int64_t ldy, const float* dY,
                           int64_t lddy, const float* gamma, const float* save_mean, const float* save_invstd, float* dX,
                           int64_t lddx, float* dgamma, float* dbeta, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * SimpleGrda.step() on one parameter (autofis/optimizer.py:39-60), element-wise over n floats:
 *   acc <- acc + first_iter * p - lr * g;   p <- sign(acc) * max(|acc| - l1_accumulation, 0)
 * The caller keeps `iterations` and l1_accumulation (host doubles, the reference's expression) and passes
 * first_iter = max(1 - iterations, 0).  p, acc and g are three buffers.
 * ---------------------------------------------------------------------------------------- */
int rec_grda_step(int64_t n, float* p, float* acc, const float* g, float lr, float l1_accumulation, int32_t first_iter,
                  void* stream);

/* ------------------------------------------------------------------------------------------
 * DIEN (models/rank/dien/net.py) — csrc/dien_ops.hip.  Every sum has a fixed order: reruns are bit-identical.
 *
 * GRU recurrence, ONE launch for the whole time loop of one layer (paddle.nn.GRU / GRUCell [EXT], gate order r, z, c):
 *   r = sigmoid(Gi_r + W_hr h + b_hr)   z = sigmoid(Gi_z + W_hz h + b_hz)
 *   c = tanh(Gi_c + r * (W_hc h + b_hc))   h' = z * h + (1 - z) * c,   h_0 = 0
 * Gi [batch, steps, 3*hidden] = X W_ih^T + b_ih is the caller's GEMM (rec_gemm_f32 over batch*steps rows); W_hh
 * [3*hidden, hidden] row-major, 16-byte aligned; hidden a multiple of 4, <= 256.  The products h W_hh^T run on
 * v_mfma_f32_16x16x4_f32 (exact f32, k-ordered).
 * rec_gru_seq_fwd: H_out [batch, steps, hidden]; saved (nullable: inference) [batch, steps, 5*hidden] = r | z | c | hc
 *   | hp with hc = W_hc h + b_hc and hp = h_{t-1}.
 * rec_gru_seq_bwd: walks t = steps-1 .. 0 from dH_out [batch, steps, hidden] (a gradient per step) and / or dh_T
 *   [batch, hidden] (a gradient of the last state); both nullable.  Writes dGi and dGh [batch, steps, 3*hidden] (they
 *   differ in the c columns, by r) and carries dh_{t-1} = dGh_t W_hh + dh_t * z_t.  The weight gradients and dX are the
 *   caller's GEMMs over batch*steps rows: dW_ih = dGi^T X, db_ih = colsum(dGi), dW_hh = dGh^T H_prev, db_hh =
 *   colsum(dGh), dX = dGi W_ih (H_prev = the hp columns of saved, row stride 5*hidden).
 * ---------------------------------------------------------------------------------------- */
int rec_gru_seq_fwd(int64_t batch, int32_t steps, int32_t hidden, const float* Gi, const float* W_hh, const float* b_hh,
                    float* H_out, float* saved, void* stream);
int rec_gru_seq_bwd(int64_t batch, int32_t steps, int32_t hidden, const float* saved, const float* W_hh,
                    const float* dH_out, const float* dh_T, float* dGi, float* dGh, void* stream);

/* DIEN's auxiliary loss (net.py:219-254), kept as written: for t = 0 .. steps-2
 *   p = gru_out[b,t] . hist[b,t+1];   n = clip(gru_out[b,t] . neg[b,t+1], -15, 15)
 *   aux[0] = (1 / batch) sum_b sum_t log(1e-8 + sigmoid(p)) + log(1e-8 + sigmoid(n))
 * gru_out, hist [batch, steps, item_dim + cat_dim] (hist: the gathered rows); neg[b,t] = [W_neg_item[neg_item[b,t]] |
 * W_neg_cat[neg_cat[b,t]]], where the id padding_idx (< 0: none) reads as zeros and an id outside its table reads as
 * zeros and raises REC_FLAG_INDEX_OOB.  workspace >= rec_dien_aux_workspace_bytes.
 * rec_dien_aux_bwd, d_aux = dloss / d aux: d_gru_out [batch, steps, H] (zero at t = steps-1), d_hist[b,t+1] (+)=
 * dp gru_out[b,t] (accumulate_hist 0: written, zero at t = 0), d_neg [batch, steps, H] = the gradient of the
 * concatenated neg rows (zero at t = 0 and where |n| >= 15). */
int rec_dien_aux_workspace_bytes(int64_t batch, int32_t steps, size_t* bytes);
int rec_dien_aux_fwd(int64_t batch, int32_t steps, int32_t item_dim, int32_t cat_dim, const float* gru_out,
                     const float* hist, const int64_t* neg_item, const int64_t* neg_cat, const float* W_neg_item,
                     int32_t item_stride, int64_t item_rows, const float* W_neg_cat, int32_t cat_stride, int64_t cat_rows,
                     int64_t padding_idx, float* aux, int32_t* status, void* workspace, size_t workspace_bytes,
                     void* stream);
int rec_dien_aux_bwd(int64_t batch, int32_t steps, int32_t item_dim, int32_t cat_dim, const float* gru_out,
                     const float* hist, const int64_t* neg_item, const int64_t* neg_cat, const float* W_neg_item,
                     int32_t item_stride, int64_t item_rows, const float* W_neg_cat, int32_t cat_stride, int64_t cat_rows,
                     int64_t padding_idx, float d_aux, float* d_gru_out, float* d_hist, int32_t accumulate_hist,
                     float* d_neg, int32_t* status, void* stream);

/* DIEN's attention over positions (net.py:192-209), composed around the caller's GEMMs of the attention MLP:
 * rec_dien_att_feat_fwd: feat [n, 4*emb_dim] = [h, q, h - q, h * q] of hist, q [n, emb_dim] (n = batch * steps).
 * rec_dien_att_feat_bwd: d_hist (+)= d0 + d2 + d3 * q;  d_q = d1 - d2 + d3 * h  for dfeat = [d0, d1, d2, d3].
 * rec_dien_attention_seq_fwd: w [batch, steps] = softmax_t((score + mask) * scale), x_att [batch, steps, emb_dim] =
 *   w[b,t] * hist[b,t,:] (not pooled).  mask is additive f32 (0 / -1e9); a row masked everywhere comes out uniform by
 *   plain arithmetic.
 * rec_dien_attention_seq_bwd: from dx_att [batch, steps, emb_dim], g_t = dx_att_t . hist_t:
 *   dscore [batch, steps] = scale * w_t (g_t - sum_s w_s g_s)  (the gradient of the MLP's output),
 *   d_hist[b,t,:] (+)= w_t dx_att[b,t,:]. */
int rec_dien_att_feat_fwd(int64_t n, int32_t emb_dim, const float* hist, const float* q, float* feat, void* stream);
int rec_dien_att_feat_bwd(int64_t n, int32_t emb_dim, const float* hist, const float* q, const float* dfeat, float* d_hist,
                          int32_t accumulate_hist, float* d_q, void* stream);
int rec_dien_attention_seq_fwd(int64_t batch, int32_t steps, int32_t emb_dim, const float* score, const float* mask,
                               const float* hist, float scale, float* w, float* x_att, void* stream);
int rec_dien_attention_seq_bwd(int64_t batch, int32_t steps, int32_t emb_dim, const float* w, const float* hist,
                               const float* dx_att, float scale, float* dscore, float* d_hist, int32_t accumulate_hist,
                               void* stream);

/* ------------------------------------------------------------------------------------------
 * DMR (models/rank/dmr/net.py, Deep Match to Rank) — csrc/dmr_ops.hip.  Every sum has a fixed order: reruns are
 * bit-identical.  P = float32(-2^32 + 1) = -4294967296 is the reference's padding score.
 *
 * rec_dmr_prefix_pool_fwd (net.py:259-281 for a LIST of rows of the [B,T,T] tile; net.py:338-350 with the one row T-1):
 *   score [batch, steps]; mask [batch, steps] i64 (row stride ld_mask), valid iff == 1; hist[b,j,:] at hist + (b * steps
 *   + j) * ld_hist; rows[num_rows] (HOST memory, 1 <= num_rows <= 8, each in [0, steps)).  For every listed row r:
 *     v_j = (j <= r && mask_j == 1) ? score_j : P   for ALL j < steps;   w_r = softmax(v) (f32, maximum subtracted)
 *     out[b, r, :] = sum_j w_{r,j} hist[b,j,:]  (ascending j)   at out + b * ld_out + r * dim
 *   A prefix without a valid position has max = P and comes out uniform 1 / steps over ALL positions, as in the
 *   reference.  rel (nullable): rel[b * ld_rel] = sum_j (mask_j == 1 ? score_j : 0).  w [batch, num_rows, steps] is saved.
 * rec_dmr_prefix_pool_bwd: g_{r,j} = d_out[b,r] . hist[b,j];  dv_{r,j} = w_{r,j} (g_{r,j} - sum_s w_{r,s} g_{r,s});
 *   dscore[b,j] = sum_r [j <= r && mask_j == 1] dv_{r,j} + [mask_j == 1] d_rel[b * ld_drel]   (d_rel nullable; a padded
 *   entry gets no gradient even where its weight is 1 / steps);  d_hist[b,j,:] (+)= sum_r w_{r,j} d_out[b,r,:]
 *   (accumulate_hist 0: written).  steps <= 4096.
 * ---------------------------------------------------------------------------------------- */
int rec_dmr_prefix_pool_fwd(int64_t batch, int32_t steps, int32_t dim, const float* score, const int64_t* mask,
                            int64_t ld_mask, const float* hist, int64_t ld_hist, int32_t num_rows, const int32_t* rows,
                            float* out, int64_t ld_out, float* rel, int64_t ld_rel, float* w, void* stream);
int rec_dmr_prefix_pool_bwd(int64_t batch, int32_t steps, int32_t dim, const int64_t* mask, int64_t ld_mask,
                            const float* hist, int64_t ld_hist, int32_t num_rows, const int32_t* rows, const float* w,
                            const float* d_out, int64_t ld_dout, const float* d_rel, int64_t ld_drel, float* dscore,
                            float* d_hist, int64_t ld_dhist, int32_t accumulate_hist, void* stream);

/* paddle.nn.PReLU on X [m, n] (row strides): y = x > 0 ? x : alpha[ch] * x.  row_mode 0: ch = column (num_alpha == n;
 * n = 1 is one shared slope).  row_mode 1: ch = base + row % period (axis 1 of a [B, period, n] input given as
 * [B * period, n]; base + period <= num_alpha).
 * rec_prelu_bwd: dX = x > 0 ? dy : alpha[ch] dy;  dalpha[ch] = sum of dy * x over x <= 0 — ALL num_alpha entries are
 * written (0 for a channel the call does not reach); per-block partials in the workspace, folded in a fixed order. */
int rec_prelu_fwd(int64_t m, int32_t n, const float* X, int64_t ldx, const float* alpha, int32_t num_alpha,
                  int32_t row_mode, int32_t period, int32_t base, float* Y, int64_t ldy, void* stream);
int rec_prelu_workspace_bytes(int64_t m, int32_t n, int32_t row_mode, int32_t period, size_t* bytes);
int rec_prelu_bwd(int64_t m, int32_t n, const float* X, int64_t ldx, const float* dY, int64_t lddy, const float* alpha,
                  int32_t num_alpha, int32_t row_mode, int32_t period, int32_t base, float* dX, int64_t lddx,
                  float* dalpha, void* workspace, size_t workspace_bytes, void* stream);

/* DMR's auxiliary match loss (net.py:298-301): logits = U V^T + bias over ALL classes, mean softmax cross-entropy.
 * U [batch, k], V [classes, k] (row strides multiples of 4, 16-byte aligned; k a multiple of 4, <= 64), bias [classes]
 * nullable, label[b * ld_label] i64.  No buffer of batch x classes elements exists: the classes are cut into at most 64
 * chunks whose (max, sum exp) are folded in chunk order; plain f32 FMAs.
 *   lse[b] = log sum_c exp(logit[b,c]);   loss[0] = (1 / batch) sum_b (lse[b] - logit[b, label_b])
 * A label outside [0, classes) raises REC_FLAG_INDEX_OOB; such a row contributes its lse alone.
 * rec_dmr_match_loss_bwd recomputes the logits: G[b,c] = (d_loss / batch) (exp(logit - lse_b) - [c == label_b]);
 *   dU[b,:] = sum_c G[b,c] V[c,:];   dV[c,:] (+)= sum_b G[b,c] U[b,:] for EVERY class (accumulate_dv 0: written).
 * Workspaces: rec_dmr_match_loss_workspace_bytes (forward: (max, sum) per row and chunk; backward: the larger of the
 * per-chunk dU partials [batch, 64, k] and the per-batch-chunk dV partials [16, classes, k]); 16-byte aligned. */
int rec_dmr_match_loss_workspace_bytes(int64_t batch, int64_t classes, int32_t k, size_t* fwd_bytes, size_t* bwd_bytes);
int rec_dmr_match_loss_fwd(int64_t batch, int64_t classes, int32_t k, const float* U, int64_t ldu, const float* V,
                           int64_t ldv, const float* bias, const int64_t* label, int64_t ld_label, float* loss,
                           float* lse, int32_t* status, void* workspace, size_t workspace_bytes, void* stream);
int rec_dmr_match_loss_bwd(int64_t batch, int64_t classes, int32_t k, const float* U, int64_t ldu, const float* V,
                           int64_t ldv, const float* bias, const int64_t* label, int64_t ld_label, const float* lse,
                           float d_loss, float* dU, int64_t lddu, float* dV, int64_t lddv, int32_t accumulate_dv,
                           void* workspace, size_t workspace_bytes, void* stream);

/* The glue of DMR's tower input (net.py:471, 289-291, 512-516, 526), written straight into column ranges of `inp`:
 * rec_dmr_tail_fwd: hist_sum[b,:] = sum_t hist[b,t,:] over ALL t (the reference ignores the mask); prod = item_eb *
 *   hist_sum; rel_u2i[b] = uv[b,1,:] . V[cate_id[b]];  U2[b,:] = uv[b,0,:] * float(match_mask[b * ld_mm]).  dim = the
 *   width of hist / item_eb; uv [batch, 2, dim / 2] = the PReLU'd rows T-2 and T-1; U2 [batch, dim / 2].  A cate_id
 *   outside [0, classes) reads as a zero row and raises REC_FLAG_INDEX_OOB.
 * rec_dmr_tail_bwd_match: d_uv[b,0,:] = dU2[b,:] * match_mask[b] (dU2 nullable: 0);  d_uv[b,1,:] = d_rel[b] V[cate_id[b]];
 *   dV_rows[b,:] = d_rel[b] uv[b,1,:] (the gradient of the cate_id lookup of V).
 * rec_dmr_tail_bwd_hist: d_hist[b,t,:] += f1[b,t,:] + f2[b,t,:] + d_sum[b,:] + d_prod[b,:] * item_eb[b,:]  (f1, f2
 *   [batch, steps, dim] contiguous, nullable);  d_item[b,:] = d_item_direct[b,:] + d_prod[b,:] * hist_sum[b,:] +
 *   sum_t d_ctx[(b * steps + t) * ld_ctx + :]  (ascending t: the tiled item_eb of net.py:311-319). */
int rec_dmr_tail_fwd(int64_t batch, int32_t steps, int32_t dim, const float* hist, int64_t ld_hist, const float* item_eb,
                     int64_t ld_item, const float* uv, const int64_t* match_mask, int64_t ld_mm, const float* V,
                     int64_t ldv, int64_t classes, const int64_t* cate_id, float* hist_sum, int64_t ld_sum, float* prod,
                     int64_t ld_prod, float* rel_u2i, int64_t ld_rel, float* U2, int32_t* status, void* stream);
int rec_dmr_tail_bwd_match(int64_t batch, int32_t half_dim, const float* dU2, const float* d_rel, int64_t ld_drel,
                           const float* uv, const int64_t* match_mask, int64_t ld_mm, const float* V, int64_t ldv,
                           int64_t classes, const int64_t* cate_id, float* d_uv, float* dV_rows, int64_t ld_dvr,
                           void* stream);
int rec_dmr_tail_bwd_hist(int64_t batch, int32_t steps, int32_t dim, const float* f1, const float* f2, const float* d_sum,
                          int64_t ld_dsum, const float* d_prod, int64_t ld_dprod, const float* item_eb, int64_t ld_item,
                          const float* hist_sum, int64_t ld_sum, const float* d_item_direct, int64_t ld_did,
                          const float* d_ctx, int64_t ld_ctx, float* d_hist, int64_t ld_dhist, float* d_item,
                          int64_t ld_ditem, void* stream);

/* ------------------------------------------------------------------------------------------
 * BST (models/rank/bst/net.py): the Transformer encoder block.  All float32, fixed summation order, no float atomics.
 *
 * rec_mha_fwd: multi-head attention over [batch, seq_len] tokens (net.py:339-394 between the q / k / v Linears and
 *   po_liner).  q, k: [batch * seq_len, >= n_head * d_k], v: [.., >= n_head * d_v] with row strides ldq / ldk / ldv — three
 *   column ranges of one packed projection output, or separate matrices; head h is columns h * d .. (h + 1) * d.
 *     out[b*L + i, h*d_v : (h+1)*d_v] = sum_j drop(softmax_j(scale * q_i . k_j)) v_j     (the combined-heads layout)
 *     lse[(b*n_head + h)*L + i]       = log sum_j exp(scale * q_i . k_j)
 *   No [batch, n_head, L, L] array is written, forward or backward: keys and values are walked in tiles with the running
 *   maximum subtracted.  Limits: 1 <= seq_len <= 8192; d_k, d_v multiples of 4 in [4, 64]; every pointer 16-byte aligned
 *   and every row stride a multiple of 4.  scale is the factor on the scores (bst passes 1: net.py:366 does not scale).
 *   Dropout on the weights (upscale_in_train): element e = ((b*n_head + h)*L + i)*L + j is kept by rec_dropout's rule for
 *   (p, seed, stream_id) — rec_dropout on ones of shape [batch*n_head*L, L] reproduces the mask.  p = 0 skips the hashing.
 * rec_mha_bwd: recomputes the weights from lse; delta [batch*n_head*L] scratch (receives D_i = sum_j P_ij dP_ij / sum_j
 *   P_ij, summed over the recomputed weights in a sweep of its own; `out`, the forward's output, is validated and not
 *   read — dO_i . O_i is the same number only in exact arithmetic).  dq, dk, dv with their own row strides (column ranges of one packed gradient are fine); they
 *   alias no input and not each other.
 * ---------------------------------------------------------------------------------------- */
int rec_mha_fwd(int64_t batch, int32_t seq_len, int32_t n_head, int32_t d_k, int32_t d_v, const float* q, int64_t ldq,
                const float* k, int64_t ldk, const float* v, int64_t ldv, float scale, float p, uint64_t seed,
                uint64_t stream_id, float* out, int64_t ldo, float* lse, void* stream);
int rec_mha_bwd(int64_t batch, int32_t seq_len, int32_t n_head, int32_t d_k, int32_t d_v, const float* q, int64_t ldq,
                const float* k, int64_t ldk, const float* v, int64_t ldv, float scale, float p, uint64_t seed,
                uint64_t stream_id, const float* out, int64_t ldo, const float* d_out, int64_t ld_dout, const float* lse,
                float* delta, float* dq, int64_t lddq, float* dk, int64_t lddk, float* dv, int64_t lddv, void* stream);

/* y = LN(x + r) over the last axis of [m, n] (row strides), r nullable; no affine parameters (net.py:286-290: the
 * scale 1 / bias 0 that paddle.static.nn.layer_norm creates afresh on every dygraph call), biased variance, rstd =
 * 1 / sqrt(var + eps).  mean, rstd [m] are saved.  y may be x or r.  y_group > 0: row i of y sits at (i / y_group) *
 * ldy_group + (i % y_group) * ldy (the encoder output written to rows 1.. of each sample of the tower input).
 * rec_add_layer_norm_bwd: dx = rstd (dy - mean(dy) - y mean(dy y)) — the gradient of the SUM, which feeds both x and r;
 * dx may be dy, not y. */
int rec_add_layer_norm_fwd(int64_t m, int32_t n, const float* x, int64_t ldx, const float* r, int64_t ldr, float eps, float* y,
                           int64_t ldy, int64_t y_group, int64_t ldy_group, float* mean, float* rstd, void* stream);
int rec_add_layer_norm_bwd(int64_t m, int32_t n, const float* y, int64_t ldy, int64_t y_group, int64_t ldy_group,
                           const float* rstd, const float* dy, int64_t lddy, float* dx, int64_t lddx, void* stream);

/* paddle.nn.LeakyReLU: y = x > 0 ? x : slope x over [m, n] (row strides, in place allowed).  The backward reads the
 * OUTPUT: dx = y > 0 ? dy : slope dy (slope > 0: y has x's sign; at +-0 the gradient is the slope).  dx may be dy. */
int rec_leaky_relu_fwd(int64_t m, int32_t n, const float* x, int64_t ldx, float slope, float* y, int64_t ldy, void* stream);
int rec_leaky_relu_bwd(int64_t m, int32_t n, const float* y, int64_t ldy, const float* dy, int64_t lddy, float slope, float* dx,
                       int64_t lddx, void* stream);

/* BST's glue.
 * rec_bst_add: y = x + r over [m, n] (row strides; r nullable: a strided copy; in place allowed).
 * rec_bst_embed_fwd: the seven lookups of net.py:421-442.  ids / id_ld / tables / table_rows: 7 entries in the order
 *   hist item, hist cat, hist position ([batch, steps] ids, row stride id_ld), target item, target cat, target position,
 *   user ([batch] ids, element stride id_ld); tables are contiguous [rows, width], widths = {item, cat, position},
 *   d_model = their sum = the user table's width.  X[(b*(steps+1) + l)*ldx + :] = [item | cat | position] of position l
 *   (l = steps: the target);  user_out[b*ld_user + :] = user[uid[b]].  An id outside its table reads as a zero row and
 *   raises REC_FLAG_INDEX_OOB.
 * rec_bst_embed_bwd: dX [batch*(steps+1), d_model] -> grads[0..2] [batch*steps, width], grads[3..5] [batch, width], the
 *   contiguous gradient rows of the six sequence lookups.
 * rec_bst_possum_fwd: y[b] = sum_l z[b*positions + l] + bias[0] (net.py:456, 74).
 * rec_bst_possum_bwd: dz[b*positions + l] = dy[b];  dbias[0] = sum_b dy[b]. */
int rec_bst_add(int64_t m, int64_t n, const float* x, int64_t ldx, const float* r, int64_t ldr, float* y, int64_t ldy,
                void* stream);
int rec_bst_embed_fwd(int64_t batch, int32_t steps, const int64_t* const* ids, const int64_t* id_ld,
                      const float* const* tables, const int64_t* table_rows, const int32_t* widths, float* X, int64_t ldx,
                      float* user_out, int64_t ld_user, int32_t* status, void* stream);
int rec_bst_embed_bwd(int64_t batch, int32_t steps, const int32_t* widths, const float* dX, int64_t lddx, float* const* grads,
                      void* stream);
int rec_bst_possum_fwd(int64_t batch, int32_t positions, const float* z, const float* bias, float* y, void* stream);
int rec_bst_possum_bwd(int64_t batch, int32_t positions, const float* dy, float* dz, float* dbias, void* stream);

/* ----------------------------------------------------------------------------------------
 * The multitask family (models/multitask/mmoe, ple): the gate softmax, the gate-weighted mixture of expert outputs and the
 * two-class softmax / clip / log-loss head (csrc/mtl_ops.hip).  float32, no atomics, no workspace; every output element
 * is produced by one thread or one fixed-order fold, so a rerun is bit-identical.  Arguments are checked on the host
 * before any launch (REC_EINVAL); batch == 0 returns REC_OK without a launch.
 *
 * rec_mtl_mix_desc: H is [batch, n_slots * expert_size], n_slots column blocks of expert_size floats (the experts'
 *   post-ReLU outputs, a column range of the packed expert | gate GEMM's output).  Gate g mixes the expert slots
 *   [first0[g], first0[g] + count0[g]) followed by [first1[g], first1[g] + count1[g]), in that order: count0 >= 1,
 *   count1 >= 0, count0 + count1 <= 64, the two ranges disjoint and inside n_slots (first1 is not read when count1 is 0).
 *   MMoE uses one range per gate, PLE's task gates two (own experts, then the shared ones).  With n_g = count0[g] +
 *   count1[g], gate g's logits, probabilities and logit gradients occupy columns [sum_{g' < g} n_g', + n_g).
 *   Limits: expert_size 1..1024, n_slots 1..128, n_gates 1..16.  Row strides in floats; 0 means packed (n_slots *
 *   expert_size for ld_h / ld_dh, sum n_g for ld_logit / ld_prob / ld_dlogit, n_gates * expert_size for ld_out, which
 *   mix and dmix share); a non-zero value below the packed width is refused.  Columns beyond the packed width of a strided
 *   output are not touched.  float4 accesses are used when expert_size, ld_h, ld_out (and ld_dh) are multiples of 4 and
 *   H, mix / dmix (and dH) are 16-byte aligned; anything else runs the scalar form.
 * rec_mtl_mix_fwd: prob_g = softmax(logits_g) per row (maximum subtracted);
 *   mix[b, g * S + s] = sum_j prob[b, g, j] * H[b, slot(g, j) * S + s], j ascending.  prob is kept for the backward.
 * rec_mtl_mix_bwd: dp[g, j] = sum_s dmix[b, g, s] H[b, slot(g, j), s];  dlogits[g, j] = prob[g, j] (dp[g, j] - sum_k
 *   prob[g, k] dp[g, k]);  dH[b, e, s] = sum over the gates that select slot e, g ascending, of prob dmix[b, g, s],
 *   multiplied by (H > 0) when relu != 0 (the experts' ReLU).  A slot no gate selects gets zeros.  No output aliases an
 *   input.
 * rec_mtl_head: logits [batch, 2 * n_tasks] (row stride ld), label [batch, n_tasks] float (row stride ld_label), n_tasks
 *   1..REC_MTL_MAX_TASKS; 0 strides mean packed.  Per row and task: p = softmax(logits[2t : 2t + 2]);  pred[b, 2t : 2t + 2] = clip(p,
 *   1e-15, 1 - 1e-15) evaluated in float32 (the upper bound is 1);  cost[b, t] = -y log(pred1 + 1e-4) - (1 - y) log(1 -
 *   pred1 + 1e-4) with pred1 the clipped column 1;  dlogits [batch, 2 * n_tasks] (NULL at inference) = the gradient of
 *   grad_scale * cost through the clip (passing where lo <= p <= hi) and the softmax.  pred, cost and dlogits are packed.
 * ---------------------------------------------------------------------------------------- */
#define REC_MTL_MAX_GATES 16
#define REC_MTL_MAX_SLOTS 128
#define REC_MTL_MAX_PER_GATE 64
#define REC_MTL_MAX_EXPERT_SIZE 1024
#define REC_MTL_MAX_TASKS 16 /* rec_mtl_head's n_tasks */
typedef struct {
  int64_t batch;
  int32_t expert_size;
  int32_t n_slots;
  int32_t n_gates;
  int64_t ld_h, ld_logit, ld_prob, ld_out, ld_dh, ld_dlogit;
  int32_t first0[REC_MTL_MAX_GATES], count0[REC_MTL_MAX_GATES], first1[REC_MTL_MAX_GATES], count1[REC_MTL_MAX_GATES];
} rec_mtl_mix_desc;

int rec_mtl_mix_fwd(const rec_mtl_mix_desc* desc, const float* H, const float* logits, float* prob, float* mix, void* stream);
int rec_mtl_mix_bwd(const rec_mtl_mix_desc* desc, const float* H, const float* prob, const float* dmix, int32_t relu, float* dH,
                    float* dlogits, void* stream);
int rec_mtl_head(int64_t batch, int32_t n_tasks, const float* logits, int64_t ld, const float* label, int64_t ld_label,
                 float grad_scale, float* pred, float* cost, float* dlogits, void* stream);

/* ----------------------------------------------------------------------------------------
 * The entire-space multitask nets (models/multitask/esmm, escm2): the padded multi-field sum-pool and the entire-space
 * head (csrc/esm_ops.hip).  float32, no atomics, no workspace; every output element is produced by one thread or one
 * fixed-order fold, so a rerun is bit-identical.  Arguments are checked on the host before any launch (REC_EINVAL);
 * batch == 0 returns REC_OK without a launch.
 *
 * rec_field_sumpool_fwd: ids int64 [batch, num_fields, max_len], packed; W [num_rows, emb_dim] with row stride
 *   row_stride >= emb_dim.  out[b, f * emb_dim + d] = sum over l, ascending, starting from +0.0f, of W[ids[b, f, l], d];
 *   an id equal to padding_idx is skipped (padding_idx < 0: none).  An id outside [0, num_rows) sets REC_FLAG_INDEX_OOB
 *   in *status (status may be NULL), counts as padding, and its row is never read.  ld_out: row stride of out in floats,
 *   0 = packed (num_fields * emb_dim); a non-zero value below the packed width is refused; columns beyond the packed
 *   width are not touched.  float4 accesses when emb_dim, row_stride and ld_out are multiples of 4 and W and out are
 *   16-byte aligned; the scalar form otherwise.  Limits: max_len 1..64, emb_dim 1..1024, num_fields >= 1.
 *   There is no backward entry point: lookup i of the flattened ids takes row i / max_len of dX viewed as
 *   [batch * num_fields, emb_dim], i.e. rec_grad_layout.div = max_len for rec_segment_partials / rec_adam_rows_all.
 *
 * rec_esm_head: logits [batch, 2G] (row stride ld_logit, 0 = packed), G = 2 (tasks ctr, cvr) in the modes REC_ESM_ESMM and
 *   REC_ESM_IPW, G = 3 (ctr, cvr, imputation) in REC_ESM_DR; click, buy int64 [batch].  Per task p = softmax over its two
 *   logits (maximum subtracted); the ESCM2 modes (IPW, DR) clip p to [1e-15, 1 - 1e-15] evaluated in float32 (the upper
 *   bound is 1), ESMM does not.  With p1, q1, i1 column 1 of the ctr, cvr and imputation tasks, y = o = float(click), t =
 *   float(buy), r = p1 q1 and L(x, lab) = -lab log(x + 1e-4) - (1 - lab) log(1 - x + 1e-4):
 *     pred [batch, 2G + 2]: columns 2g, 2g + 1 task g's (clipped) softmax, the last two (1 - r, r);
 *     cost [batch, 3]:  cost0 = L(p1, y);  cost2 = L(r, t);  cost1 = 0 (ESMM),
 *       L(q1, t) IPS o with IPS = clip(1 / max(p1 float(N_click), 1e-6), -15, 15) float(batch)            (IPW),
 *       i1 + e IPS + e^2 IPS with e = L(q1, t) - i1 and IPS = clip(o / max(p1, 1e-6), -15, 15)             (DR);
 *     dlogits [batch, 2G] (NULL at inference): the gradient of grad_scale (cost0 + counterfactual_w cost1 + global_w
 *       cost2) through the clip (passing where lo <= p <= hi) and the softmax, IPS carrying none; per task ONE value is
 *       computed and column 0 holds its negation: dlogits[2g] == -dlogits[2g + 1] exactly.
 *   pred, cost and dlogits are packed.  The step's loss is mean(cost0) + counterfactual_w mean(cost1) + global_w
 *   mean(cost2), left to the caller.  click_count: int64 [1] device OUTPUT, N_click = sum click, filled first by one
 *   workgroup (an exact integer fold) whenever it is non-null; required in the IPW mode, may be NULL otherwise.
 * ---------------------------------------------------------------------------------------- */
#define REC_FIELD_SUMPOOL_MAX_LEN 64
#define REC_FIELD_SUMPOOL_MAX_DIM 1024
#define REC_ESM_ESMM 0
#define REC_ESM_IPW 1
#define REC_ESM_DR 2
typedef struct {
  int64_t batch;
  int32_t mode;
  int64_t ld_logit;
  float global_w, counterfactual_w, grad_scale;
} rec_esm_head_desc;

int rec_field_sumpool_fwd(int64_t batch, int32_t num_fields, int32_t max_len, int32_t emb_dim, int32_t row_stride,
                          int64_t num_rows, int64_t padding_idx, const int64_t* ids, const float* W, float* out, int64_t ld_out,
                          int32_t* status, void* stream);
int rec_esm_head(const rec_esm_head_desc* desc, const float* logits, const int64_t* click, const int64_t* buy,
                 int64_t* click_count, float* pred, float* cost, float* dlogits, void* stream);

/* ----------------------------------------------------------------------------------------
 * AITM (models/multitask/aitm): the per-field gather over tables of unequal size, the adaptive information transfer (AIT)
 * block, the coupled two-task head and the AUC histogram with more buckets than LDS holds (csrc/aitm_ops.hip).  float32;
 * no entry point takes a workspace; no float atomics; every output element has one writer and every cross-lane sum is a
 * fixed-order butterfly, so a rerun is bit-identical (the wide histogram adds INTEGERS atomically: exact in any order).
 * Arguments are checked on the host before any launch (REC_EINVAL); batch == 0 returns REC_OK without a launch after
 * those checks.  A row stride ld_* of 0 means packed; a non-zero value below the packed width is refused; columns beyond
 * the packed width are not touched.  The float4 form runs when the widths and strides are multiples of 4 and the row
 * pointers are 16-byte aligned, the scalar form otherwise (same order of operations, same result).
 *
 * rec_field_gather_fwd: ids int64 [batch, num_fields], packed; field f owns the rows [field_begin[f], field_begin[f + 1])
 *   of W (row stride row_stride >= emb_dim); field_begin int64 [num_fields + 1] is DEVICE memory.
 *   out[b, f * emb_dim + d] = W[field_begin[f] + ids[b, f], d].  There is no padding id: id 0 is a row like any other.
 *   An id outside [0, field_begin[f + 1] - field_begin[f]) — also one that is still inside the whole buffer, i.e. in a
 *   neighbouring field's rows — sets REC_FLAG_INDEX_OOB in *status (status may be NULL), is never read, and writes a zero
 *   row.  rows_out (int64 [batch * num_fields], may be NULL) receives the global row field_begin[f] + id, or -1 for such an
 *   id: rec_ids_group drops a negative id (it counts it as out of range: the flag is set there too, no row is touched),
 *   so rows_out with padding_idx = -1 and num_rows = field_begin[num_fields] is the grouping of the backward
 *   (rec_grad_layout.div = 1 over dX viewed as [batch * num_fields, emb_dim]).  emb_dim 1..1024, num_fields >= 1.
 *
 * rec_ait_fwd: QKV [batch * tokens, 3 dim] (row stride ld_qkv), row b * tokens + t = Q_t | K_t | V_t of sample b.
 *   s_t = <Q_t, K_t> / sqrt(dim) (each token's OWN Q and K: aitm/net.py:57), a = softmax over the tokens (maximum
 *   subtracted), out[b] = sum_t a_t V_t, t ascending (out [batch, dim], row stride ld_out); prob [batch, tokens] packed
 *   receives a.  tokens 1..8, dim 1..256.
 * rec_ait_bwd: the same QKV and prob, d_out [batch, dim] (ld_dout) -> dQKV [batch * tokens, 3 dim] (ld_dqkv):
 *   dV_t = a_t d_out, da_t = <d_out, V_t>, ds_t = a_t (da_t - sum_u a_u da_u), dQ_t = ds_t K_t / sqrt(dim),
 *   dK_t = ds_t Q_t / sqrt(dim); with tokens == 1, dQ and dK are exactly zero.  Weight and input gradients are GEMMs over
 *   dQKV (rec_gemm_f32_pair); nothing is reduced over the batch here.
 *
 * rec_aitm_head: tower_click, ait [batch, dim] (ld_click, ld_ait); w_click, w_conv [dim]; b_click, b_conv [1]; click, buy
 *   int64 [batch].  pCTR = sigmoid(<tower_click, w_click> + b_click), pCVR = sigmoid(<ait, w_conv> + b_conv);
 *     pred [batch, 2]: (pCTR, pCVR);
 *     cost [batch, 3]: BCE(pCTR, click), BCE(pCVR, buy), max(pCVR - pCTR, 0) with
 *       BCE(p, y) = -(y max(log p, -100) + (1 - y) max(log(1 - p), -100));
 *     dz [batch, 2] (NULL at inference): d / d(logit) of grad_scale (cost0 + cost1) + constraint_w cost2, as the chain
 *       (grad_scale (p - y) / max(p (1 - p), 1e-12) -/+ constraint_w [pCVR > pCTR]) p (1 - p): the hinge term is NOT scaled
 *       by grad_scale (the reference sums it over the batch and averages the BCE terms) and passes only where pCVR > pCTR
 *       strictly.
 *   pred, cost and dz are packed.  The step's loss, mean(cost0) + mean(cost1) + constraint_w sum(cost2), is left to the
 *   caller.  dim 1..4096.
 *
 * rec_auc_histogram_wide: rec_auc_histogram's buckets (bucket = clamp(int(pred * num_thresholds), 0, num_thresholds);
 *   stat_pos / stat_neg int64 [num_thresholds + 1] += 1) for 1 <= num_thresholds <= 2^24, accumulated straight into global
 *   memory with 64-bit integer atomics; pred[i] is read at pred[i * ld_pred] (0 = packed, 1), so a column of pred
 *   [batch, 2] needs no copy.
 * ---------------------------------------------------------------------------------------- */
#define REC_FIELD_GATHER_MAX_DIM 1024
#define REC_AIT_MAX_TOKENS 8
#define REC_AIT_MAX_DIM 256
#define REC_AITM_HEAD_MAX_DIM 4096
#define REC_AUC_WIDE_MAX_THRESHOLDS (1 << 24)
typedef struct {
  int64_t batch;
  int32_t dim;
  int64_t ld_click, ld_ait;
  float constraint_w, grad_scale;
} rec_aitm_head_desc;

int rec_field_gather_fwd(int64_t batch, int32_t num_fields, int32_t emb_dim, int32_t row_stride, const int64_t* field_begin,
                         const int64_t* ids, const float* W, float* out, int64_t ld_out, int64_t* rows_out, int32_t* status,
                         void* stream);
int rec_ait_fwd(int64_t batch, int32_t tokens, int32_t dim, const float* QKV, int64_t ld_qkv, float* out, int64_t ld_out,
                float* prob, void* stream);
int rec_ait_bwd(int64_t batch, int32_t tokens, int32_t dim, const float* QKV, int64_t ld_qkv, const float* prob,
                const float* d_out, int64_t ld_dout, float* dQKV, int64_t ld_dqkv, void* stream);
int rec_aitm_head(const rec_aitm_head_desc* desc, const float* tower_click, const float* ait, const float* w_click,
                  const float* b_click, const float* w_conv, const float* b_conv, const int64_t* click, const int64_t* buy,
                  float* pred, float* cost, float* dz, void* stream);
int rec_auc_histogram_wide(int64_t batch, const float* pred, int64_t ld_pred, const int64_t* label, int32_t num_thresholds,
                           int64_t* stat_pos, int64_t* stat_neg, void* stream);

/* ----------------------------------------------------------------------------------------
 * MIND (models/recall/mind): the capsule routing, the label-aware attention and the sampled-softmax head
 * (csrc/mind_ops.hip).  float32; no entry point takes a workspace; no float atomics; every output element has one writer
 * and every cross-lane sum is a fixed-order butterfly, so a rerun is bit-identical.  Arguments are checked on the host
 * before any launch (REC_EINVAL); batch == 0 returns REC_OK without a launch after those checks.  A row stride ld_* of 0
 * means packed; a non-zero value below the packed width is refused; columns beyond the packed width are not touched.
 *
 * rec_mind_routing_fwd: net.py:178-234.  low [batch * seq_len_max, hidden] (row stride ld_low; row b * seq_len_max + t):
 *   the history embeddings times bilinear_mapping_matrix, a GEMM of the caller.  seq_len int64 [batch]; position t of
 *   sample b is valid where t < seq_len[b] (0 or less: none; seq_len_max or more: all).  routing_logits [k_max, seq_len_max]
 *   is shared by the batch and only read.  With B = routing_logits, iters - 1 times:
 *     W = softmax over t of where(valid, B, -2^32 + 1);  Z = W x low;  caps = squash(Z);  B += low x caps^T (every t, the
 *     padded ones too);   squash(Z) = Z n2 / (1 + n2) / sqrt(n2 + 1e-8), n2 = |Z|^2;
 *   then W = softmax over the k_max CAPSULES of where(valid, B, -2^32 + 1) (net.py:226 takes axis 1): a padded position
 *   gets exactly 1 / k_max on every capsule and contributes whatever low holds there.  Outputs, packed: W [batch, k_max,
 *   seq_len_max], Z = W x low [batch, k_max, hidden], caps = squash(Z).  One launch; low[b] is read once and kept in LDS.
 *   seq_len_max 1..64, k_max 1..8, hidden 1..128, iters 1..8 (iters == 1: only the final softmax).
 * rec_mind_routing_bwd: W is a constant of the backward (B and the inner rounds sit behind stop_gradient), so from d_caps
 *   [batch, k_max, hidden], Z and W: dZ = f d_caps + 2 f'(n2) <Z, d_caps> Z with f the squash factor, and
 *   d_low[b * seq_len_max + t] = sum_k W[b, k, t] dZ[b, k] (row stride ld_dlow).  routing_logits has no gradient.
 *
 * rec_mind_label_attn_fwd: net.py:284-297.  caps2 [batch * k_max, hidden] (ld_caps), target [batch, hidden] (ld_target):
 *   s_k = pow(<caps2_k, target>, pow_p) (pow_p == 1 takes no pow), attn = softmax over k (packed [batch, k_max]),
 *   user = sum_k attn_k caps2_k ([batch, hidden], ld_user).  There is no capsule mask.
 * rec_mind_label_attn_bwd: d_user [batch, hidden] -> d_caps2 [batch * k_max, hidden] and d_target [batch, hidden].
 *
 * rec_mind_ssm_head: net.py:63-113 after the gathers.  user, true_w [batch, hidden] (ld_user, ld_true), true_b [batch],
 *   S [batch, n_sample] (ld_s) = user x sample_w^T from the caller's GEMM, sample_b [n_sample], labels int64 [batch],
 *   neg int64 [n_sample], logq_true [batch], logq_neg [n_sample]:
 *     x_0 = <user, true_w> + true_b - logq_true;  x_j = (labels[b] == neg[j] ? -1e30 : S[b, j] + sample_b[j]) - logq_neg[j]
 *   (the accidental-hit mask BEFORE the log_q subtraction), loss[b] = logsumexp(x) - x_0 with the maximum subtracted,
 *   S[b, j] <- grad_scale softmax(x)_j IN PLACE (exactly 0 at a hit) and d_true[b] = grad_scale (softmax(x)_0 - 1).
 *   The true column's two row scalings, each [batch, hidden] and each may be NULL: d_true_w = d_true user (ld_dtw), the
 *   gradient of the gathered true rows, and d_user0 = d_true true_w (ld_du0), the term of d(user) that the caller's
 *   dS x sample_w GEMM adds to (REC_EPI_ADD).
 *   hidden 1..1024, n_sample 1..65536.
 * ---------------------------------------------------------------------------------------- */
#define REC_MIND_MAX_T 64
#define REC_MIND_MAX_K 8
#define REC_MIND_MAX_H 128
#define REC_MIND_MAX_ITERS 8
#define REC_MIND_HEAD_MAX_DIM 1024
#define REC_MIND_MAX_NEG 65536

int rec_mind_routing_fwd(int64_t batch, int32_t seq_len_max, int32_t k_max, int32_t hidden, int32_t iters, const float* low,
                         int64_t ld_low, const int64_t* seq_len, const float* routing_logits, float* W, float* Z, float* caps,
                         void* stream);
int rec_mind_routing_bwd(int64_t batch, int32_t seq_len_max, int32_t k_max, int32_t hidden, const float* d_caps, const float* Z,
                         const float* W, float* d_low, int64_t ld_dlow, void* stream);
int rec_mind_label_attn_fwd(int64_t batch, int32_t k_max, int32_t hidden, float pow_p, const float* caps2, int64_t ld_caps,
                            const float* target, int64_t ld_target, float* user, int64_t ld_user, float* attn, void* stream);
int rec_mind_label_attn_bwd(int64_t batch, int32_t k_max, int32_t hidden, float pow_p, const float* caps2, int64_t ld_caps,
                            const float* target, int64_t ld_target, const float* attn, const float* d_user, int64_t ld_duser,
                            float* d_caps2, int64_t ld_dcaps, float* d_target, int64_t ld_dtarget, void* stream);
int rec_mind_ssm_head(int64_t batch, int32_t hidden, int32_t n_sample, const float* user, int64_t ld_user, const float* true_w,
                      int64_t ld_true, const float* true_b, float* S, int64_t ld_s, const float* sample_b, const int64_t* labels,
                      const int64_t* neg, const float* logq_true, const float* logq_neg, float grad_scale, float* loss,
                      float* d_true, float* d_true_w, int64_t ld_dtw, float* d_user0, int64_t ld_du0, void* stream);

/* ----------------------------------------------------------------------------------------
 * word2vec (models/recall/word2vec), skip-gram with negative sampling (csrc/w2v_ops.hip).  float32; no entry point takes a
 * workspace; no float atomics; every sum has a fixed order, so a rerun is bit-identical.  Arguments are checked on the host
 * before any launch (REC_EINVAL, the entry and the argument named in rec_last_error()); batch == 0 returns REC_OK without a
 * launch after those checks.  A row stride ld_* of 0 means packed; a value below the packed width is refused; floats behind
 * a row's width are never written.  Rows move as 16-byte vectors when emb_dim and the strides are multiples of 4 and the
 * bases 16-byte aligned, float by float otherwise.  There is no padding id: id 0 is an ordinary word.
 *
 * rec_w2v_sgns_fwd_bwd: net.py:57-81 and dygraph_model.py:53-69.  in_ids int64 [batch]; target_ids int64 [batch, 1 + neg],
 *   the true word first; emb, emb_w [num_rows, emb_dim] (ld_emb, ld_w), emb_b [num_rows, 1] (ld_b).
 *     logit[b, j] = <emb[in_ids[b]], emb_w[target_ids[b, j]]> + emb_b[target_ids[b, j]]
 *     p = 1 / (1 + exp(-logit));  term = -max(log(j == 0 ? p : 1 - p), -100)       (sigmoid, THEN BCE on the probability)
 *     loss[0] = sum_b term[b, 0] / batch + sum_{b, j > 0} term[b, j] / (batch neg)   (each BCE takes its own mean)
 *     g[b, j] = (p - y) / max((1 - p) p, 1e-12) * s_j * (1 - p) * p,  y = (j == 0),  s_0 = grad_scale / batch,
 *               s_j = grad_scale / (batch neg): a saturated float32 sigmoid gives a term of 100 and g exactly 0
 *     d_in[b] = sum_j g[b, j] emb_w[target_ids[b, j]]   ([batch, emb_dim], ld_din), j ascending
 *   Outputs, packed: true_logits [batch], neg_logits [batch, neg], g [batch, 1 + neg], loss [1].  An id outside
 *   [0, num_rows) sets REC_FLAG_INDEX_OOB in *status (may be NULL) and is never read: every pair (b, j) it takes part in has
 *   logit 0, g 0 and no loss term (an input id: the whole sample and a zero d_in row).  emb_dim 1..REC_W2V_MAX_DIM,
 *   neg 1..REC_W2V_MAX_NEG.
 *
 * rec_w2v_target_update: the SGD step of emb_w and emb_b.  n_uniq, uniq_rows, seg_offset, sorted_pos: the grouping of
 *   target_ids viewed as [batch (1 + neg)] as rec_ids_group leaves it (its own workspace query is that entry's); g and
 *   in_ids as above; emb is the input table BEFORE its own update and is only read.  For the u-th unique row r with the
 *   occurrences pos_k (ascending):
 *     dw = sum_k g[pos_k] emb[in_ids[pos_k / (1 + neg)]];  db = sum_k g[pos_k];  emb_w[r] -= lr dw;  emb_b[r] -= lr db
 *   The [batch, 1 + neg, emb_dim] gradient is never written.  d_w_rows [n, emb_dim] (ld_dw) and d_b_rows [n], each may be
 *   NULL, receive dw and db of unique row u.  A segment of at most 16 occurrences is summed in ascending order; a longer one
 *   as 64 interleaved partials (occurrence i in partial i % 64, each ascending) folded in a fixed order.  An occurrence whose
 *   input id is outside the table contributes nothing.  emb may not overlap emb_w (REC_EINVAL).
 *
 * rec_w2v_analogy_topk: net.py:100-110.  a, b, c int64 [n_query]; W [num_rows, emb_dim] (row_stride):
 *     score[q, v] = <W[b_q] - W[a_q] + W[c_q], W[v]> / max(|W[v]|, 1e-12)
 *   values [n_query, k] descending and ids int64 [n_query, k]; equal scores order by the lower id; an all-zero row scores
 *   exactly 0.  The [n_query, num_rows] scores are never written: a block takes REC_W2V_TOPK_TILE_ROWS rows for all queries
 *   and writes its k candidates per query to cand_values / cand_ids [n_tiles, n_query, k] (float32 / int64, the caller's),
 *   a second kernel merges them; n_tiles must equal ceil(num_rows / REC_W2V_TOPK_TILE_ROWS).  k 1..REC_W2V_MAX_TOPK,
 *   num_rows >= k.  An a / b / c outside the table sets REC_FLAG_INDEX_OOB in *status (may be NULL) and counts as a zero row.
 * ---------------------------------------------------------------------------------------- */
#define REC_W2V_MAX_DIM 1024
#define REC_W2V_MAX_NEG 32
#define REC_W2V_MAX_TOPK 8
#define REC_W2V_TOPK_TILE_ROWS 128

int rec_w2v_sgns_fwd_bwd(int64_t batch, int32_t emb_dim, int32_t neg, int64_t num_rows, const int64_t* in_ids,
                         const int64_t* target_ids, const float* emb, int64_t ld_emb, const float* emb_w, int64_t ld_w,
                         const float* emb_b, int64_t ld_b, float grad_scale, float* true_logits, float* neg_logits, float* g,
                         float* d_in, int64_t ld_din, float* loss, int32_t* status, void* stream);
int rec_w2v_target_update(int64_t batch, int32_t emb_dim, int32_t neg, int64_t num_rows, const int32_t* n_uniq,
                          const int64_t* uniq_rows, const int32_t* seg_offset, const int32_t* sorted_pos, const float* g,
                          const int64_t* in_ids, const float* emb, int64_t ld_emb, float* emb_w, int64_t ld_w, float* emb_b,
                          int64_t ld_b, float lr, float* d_w_rows, int64_t ld_dw, float* d_b_rows, void* stream);
int rec_w2v_analogy_topk(int64_t n_query, int32_t emb_dim, int64_t row_stride, int64_t num_rows, int32_t k, const int64_t* a,
                         const int64_t* b, const int64_t* c, const float* W, float* cand_values, int64_t* cand_ids,
                         int64_t n_tiles, float* values, int64_t* ids, int32_t* status, void* stream);

/* ----------------------------------------------------------------------------------------
 * TiSASRec (models/recall/tisas), time-interval-aware self-attention (csrc/tisas_ops.hip).  float32; no float atomics;
 * every sum has a fixed order, so a rerun is bit-identical.  No entry point takes a workspace: what a call needs beyond its
 * results are buffers of the caller's whose sizes follow from the shapes (gs, ga, partials below).  Arguments are checked
 * on the host before any launch (REC_EINVAL, the entry named in rec_last_error()); a size of 0 rows returns REC_OK without
 * a launch after those checks.  A mask stream is rec_dropout's: element e of the named virtual matrix is kept iff
 * rec_dropout with the same (p, seed, stream id) keeps it, and a kept value is multiplied by 1 / (1 - p); with p = 0 no
 * random number is drawn.
 *
 * rec_tisas_attn_fwd: net.py:85-164 after the three projections.  q, k, v [batch * seq_len, hidden] (ldq, ldk, ldv); heads
 *   are contiguous column slices of head = hidden / n_head.  tables: a HOST array of 4 device pointers pos_k, pos_v
 *   [seq_len, hidden] and time_k, time_v [time_rows, hidden], all packed.  tm int64 [batch, seq_len, seq_len]; log_seqs int64
 *   [batch, seq_len].  probs: HOST float[3] = dropout on the attention weights, the position rows, the time rows; streams:
 *   HOST uint64[5] = the mask streams of the weights (virtual [batch n_head seq_len, seq_len], as rec_mha_fwd), pos_k, pos_v
 *   (virtual [batch seq_len, hidden]: per sample), time_k, time_v (virtual [batch seq_len seq_len, hidden]).
 *     s_ij = scale q_i . (k_j + drop(pos_k)_bj + drop(time_k[tm[b,i,j]])_bij)          per head
 *     s_ij = -2^32 + 1 for EVERY j when log_seqs[b,i] == 0, and for j > i (a replacement, not an addition): a padded query
 *            row attends uniformly, 1 / seq_len, over all keys, future ones included
 *     a_i = drop(softmax_j s_ij);  out_i = sum_j a_ij (v_j + drop(pos_v)_bj + drop(time_v[tm[b,i,j]])_bij), j ascending
 *   out [batch * seq_len, hidden] (ldo), lse [batch, n_head, seq_len] = max_j s_ij + log sum_j exp(s_ij - max).  An id of tm
 *   outside [0, time_rows) sets REC_FLAG_INDEX_OOB in *status (may be NULL) and reads row 0.  The [batch, seq_len, seq_len,
 *   hidden] relation tensors are never formed: the time rows are gathered from the tables (L2-resident) per (i, j).
 *   Limits: seq_len 1..REC_TISAS_MAX_L, head 1..REC_TISAS_MAX_HEAD, seq_len * (head | 1) <= REC_TISAS_MAX_TILE (one
 *   sample's keys and values of a head sit in LDS), time_rows >= 1; anything else is REC_EINVAL.
 *
 * rec_tisas_attn_bwd: the same inputs, d_out [batch * seq_len, hidden] (ld_dout) and the forward's lse.  The weights are
 *   recomputed from lse and renormalised by their own sum (lse of a padded row rounds to -2^32).  Writes dq, dk, dv
 *   (lddq, lddk, lddv) and, through d_tables (HOST array of 4 device pointers, shapes of tables): d_pos_k, d_pos_v summed
 *   over the batch in ascending sample order, and d_time_k, d_time_v: row t is the sum over every (b, i, j) with
 *   tm[b,i,j] == t, a row nothing hit is exactly 0.  accumulate != 0 adds the four to what d_tables hold.  gs, ga
 *   [batch * n_head * seq_len * seq_len] receive scale * d s_ij and the dropped weights a_ij (the two small score-shaped
 *   arrays the key-side and table passes read);
 *   partials holds min(batch, REC_TISAS_MAX_PARTIALS) * 2 * time_rows * hidden floats: block p sums the samples
 *   b with b / ceil(batch / P) == p into its own [time_rows, head] LDS tile in ascending (b, i, j), one fold adds the
 *   tiles in ascending p.  Additional limit: time_rows * head <= REC_TISAS_MAX_TIME_TILE.
 *
 * rec_affine_layer_norm_fwd: t = x + r (r may be NULL), t = 0 in the rows whose row_ids entry (int64 [m], may be NULL) is 0;
 *   y = (t - mean) rstd gamma + beta over the last axis, biased variance, rstd = 1 / sqrt(var + eps).  sum_out (may be NULL;
 *   may be x) receives t.  mean, rstd [m] are saved.  paddle.nn.LayerNorm(hidden, epsilon) with the residual add and the
 *   `seqs *= (log_seqs != 0)` in front of it (net.py:273-287).
 * rec_affine_layer_norm_bwd: t as the forward formed it; g = dy + dy2 (dy2 may be NULL).
 *     dx = (rstd (g gamma - mean(g gamma) - xhat mean(g gamma xhat)) + e1 + e2), 0 in the rows row_ids masks
 *   — the gradient of x and of r alike; e1, e2 (may be NULL) are further gradients of t.  dx may be dy.  dgamma[c] = sum_rows
 *   g xhat, dbeta[c] = sum_rows g: one block per column, rows strided over its threads, then a tree (fixed order).
 *
 * rec_tisas_embed_fwd: out[r] = drop(table[ids[r]] * scale), a zero row for id 0 (padding_idx 0; net.py:245-247,263).  The
 *   mask stream's virtual matrix is [n, dim].  An id outside [0, num_rows) sets REC_FLAG_INDEX_OOB and gives a zero row.
 * rec_tisas_embed_bwd: rows[r] = the gradient of table[ids[r]]: d_out[r] * scale through the same mask, zero for id 0.
 *
 * rec_tisas_head: net.py:305-308 and dygraph_model.py:42-53.  feats [n, dim] (ld_feats), pos, neg int64 [n]:
 *     pl = <feats_r, table[pos_r]>, nl = <feats_r, table[neg_r]>, selected = pos_r != 0, cnt = the selected count
 *     loss2[0] = sum_selected (softplus(-pl) + softplus(nl)) / cnt, loss2[1] = cnt — taken on the device, no host sync;
 *     cnt == 0 gives loss NaN, as the reference's mean over an empty selection, and zero gradients
 *     coef_pos[r] = (sigmoid(pl) - 1) / cnt, coef_neg[r] = sigmoid(nl) / cnt, both 0 where not selected
 *     d_feats[r] = coef_pos table[pos_r] + coef_neg table[neg_r];  d_pos_rows[r] = coef_pos feats_r, d_neg_rows[r] =
 *     coef_neg feats_r (each [n, dim] with its row stride; either may be NULL).  row_loss [n] receives the per-row terms,
 *     pos_logits, neg_logits [n] (either may be NULL) pl and nl.
 *   An id outside [0, num_rows) sets REC_FLAG_INDEX_OOB and reads as a zero row.  dim 1..REC_TISAS_HEAD_MAX_DIM.
 * ---------------------------------------------------------------------------------------- */
#define REC_TISAS_MAX_L 128
#define REC_TISAS_MAX_HEAD 64
#define REC_TISAS_MAX_TILE 7168
#define REC_TISAS_MAX_TIME_TILE 16384
#define REC_TISAS_MAX_PARTIALS 128
#define REC_TISAS_HEAD_MAX_DIM 1024

int rec_tisas_attn_fwd(int64_t batch, int32_t seq_len, int32_t n_head, int32_t hidden, int32_t time_rows, const float* q,
                       int64_t ldq, const float* k, int64_t ldk, const float* v, int64_t ldv, const float* const* tables,
                       const int64_t* tm, const int64_t* log_seqs, float scale, const float* probs, uint64_t seed,
                       const uint64_t* streams, float* out, int64_t ldo, float* lse, int32_t* status, void* stream);
int rec_tisas_attn_bwd(int64_t batch, int32_t seq_len, int32_t n_head, int32_t hidden, int32_t time_rows, const float* q,
                       int64_t ldq, const float* k, int64_t ldk, const float* v, int64_t ldv, const float* const* tables,
                       const int64_t* tm, const int64_t* log_seqs, float scale, const float* probs, uint64_t seed,
                       const uint64_t* streams, const float* d_out, int64_t ld_dout, const float* lse, float* gs, float* ga,
                       float* dq, int64_t lddq, float* dk, int64_t lddk, float* dv, int64_t lddv, float* const* d_tables,
                       float* partials, int32_t accumulate, void* stream);
int rec_affine_layer_norm_fwd(int64_t m, int32_t n, const float* x, int64_t ldx, const float* r, int64_t ldr,
                              const float* gamma, const float* beta, float eps, const int64_t* row_ids, float* sum_out,
                              int64_t ld_sum, float* y, int64_t ldy, float* mean, float* rstd, void* stream);
int rec_affine_layer_norm_bwd(int64_t m, int32_t n, const float* t, int64_t ldt, const float* mean, const float* rstd,
                              const float* gamma, const float* dy, int64_t lddy, const float* dy2, int64_t lddy2,
                              const float* e1, int64_t lde1, const float* e2, int64_t lde2, const int64_t* row_ids, float* dx,
                              int64_t lddx, float* dgamma, float* dbeta, void* stream);
int rec_tisas_embed_fwd(int64_t n, int32_t dim, int64_t num_rows, const int64_t* ids, const float* table, int64_t ld_table,
                        float scale, float p, uint64_t seed, uint64_t stream_id, float* out, int64_t ldo, int32_t* status,
                        void* stream);
int rec_tisas_embed_bwd(int64_t n, int32_t dim, int64_t num_rows, const int64_t* ids, const float* d_out, int64_t ld_dout,
                        float scale, float p, uint64_t seed, uint64_t stream_id, float* rows, int64_t ld_rows, void* stream);
int rec_tisas_head(int64_t n, int32_t dim, int64_t num_rows, const float* feats, int64_t ld_feats, const int64_t* pos,
                   const int64_t* neg, const float* table, int64_t ld_table, float* loss2, float* row_loss, float* pos_logits,
                   float* neg_logits, float* coef_pos, float* coef_neg, float* d_feats, int64_t ld_dfeats, float* d_pos_rows, int64_t ld_dpos, float* d_neg_rows,
                   int64_t ld_dneg, int32_t* status, void* stream);

/* ----------------------------------------------------------------------------------------
 * ENSFM (models/recall/ensfm), the non-sampling factorization machine (csrc/ensfm_ops.hip).  float32; no float atomics;
 * every sum has a fixed order, so a rerun is bit-identical.  No entry point takes a workspace: what a call needs beyond its
 * results are buffers of the caller's whose sizes follow from the shapes (partials below).  Arguments are checked on the
 * host before any launch (REC_EINVAL, the entry named in rec_last_error()); a size of 0 rows returns REC_OK without a launch
 * after those checks.  C = emb_dim + 2 throughout; emb_dim 1..REC_ENSFM_MAX_DIM.  h = [H_i, 1, 1].  The reference's
 * [B, I+1, C] `dot` (net.py:87) and its three [B, P, C] tensors (net.py:92-97) are never formed.
 *
 * rec_ensfm_tower_fwd: net.py:65-83 for one side.  ids int64 [n, num_fields] into table [num_rows, emb_dim] (ld_table) and
 *   bias_table [bias_rows] (the reference sizes item_bias one row shorter than all_item_feature_emb):
 *     s = sum_f table[id_f];  score = (0.5 (s^2 - sum_f table[id_f]^2)) . H_s + sum_f bias_table[id_f] (+ bias[0]; may be NULL)
 *   out [n, C] (ld_out) = [s, score, 1] (item_layout == 0: p_emb) or [s, 1, score] (item_layout != 0: q_emb).  An id outside a
 *   table sets REC_FLAG_INDEX_OOB in *status (may be NULL) and contributes zero there.  The same id twice in a row is legal.
 * rec_ensfm_tower_bwd: from d_out [n, C] (ld_dout; the constant column is not read):
 *     rows[r num_fields + f] = d_out[r, :emb_dim] + dscore_r H_s o (s_r - table[id_f])      [n num_fields, emb_dim] (ld_rows):
 *                              the gradient row of every lookup, rec_grad_layout{1,0,0} for rec_adagrad_rows; zero for a bad id
 *     dscore [n]: the gradient of every bias lookup of row r, read through rec_grad_layout{num_fields,0,0} with emb_dim 1
 *     dH_s [emb_dim] (+)= sum_r dscore_r 0.5 (s_r^2 - sum_f e_f^2);  dbias [1] (may be NULL) (+)= sum_r dscore_r
 *   accumulate != 0 adds to what dH_s / dbias hold (H_s is shared by the two towers).  partials holds
 *   min(ceil(n / 4), REC_ENSFM_MAX_PARTIALS) * (emb_dim + 1) floats: a block sums a fixed slice of the rows, one fold adds the
 *   blocks.  n == 0 leaves dH_s / dbias as they are.
 * rec_ensfm_gram: G [cols, cols] = X^T X for X [n, cols] (ldx), cols 1..REC_ENSFM_MAX_DIM + 2.  partials holds
 *   min(ceil(n / 64), REC_ENSFM_GRAM_MAX_BLOCKS) * cols * cols floats.
 * rec_ensfm_pos_user: net.py:92-97, dygraph_model.py:50 and their backward in one pass, one block per user.  ur int64
 *   [batch, max_pos], padded with num_items; p [batch, C], q [num_items + 1, C], G_q = q^T q:
 *     pos_r[b, j] = m <p[b] o h, q[ur[b, j]]>, m = (ur[b, j] != num_items);  g[b, j] = m (2 (1 - w) pos_r - 2)
 *     loss_part[b] = sum_j ((1 - w) pos_r^2 - 2 pos_r);  dHi_part[b, :] = p[b, :emb_dim] o sum_j g q[ur[b, j], :emb_dim]
 *     dP[b, :] = h o sum_j g q[ur[b, j]] + 2 w h o (G_q (p[b] o h))
 *   pos_r may be NULL.  An id outside [0, num_items] sets REC_FLAG_INDEX_OOB and counts as padding.
 * rec_ensfm_pos_item: dQ [num_items + 1, C] for ALL rows, the padding row included:
 *     dQ[i, :] = h o sum_{(b, j) -> i} g[b, j] p[b] + 2 w h o (G_p (q[i] o h))
 *   n_uniq, uniq_rows, seg_offset, sorted_pos: rec_ids_group of ur viewed as [batch max_pos] with num_rows = num_items + 1 and
 *   padding_idx = num_items.  One block per item with positives; occurrence i of its list goes to partial i % 16, each in
 *   ascending i, folded in a fixed tree, so an item in every list is 16 chains and not one.
 * rec_ensfm_loss: loss[0] = w sum_{c, c'} G_q G_p h h + sum_b loss_part[b] (dygraph_model.py:40-51);
 *     dH_i[d] = sum_b dHi_part[b, d] + 2 w sum_c' G_q[d, c'] G_p[d, c'] h[c'].
 * rec_ensfm_score: pre [batch, num_rows] (ld_pre) = (p o h) q^T for --infer (net.py:87-90), LDS-tiled.
 * ---------------------------------------------------------------------------------------- */
#define REC_ENSFM_MAX_DIM 128
#define REC_ENSFM_MAX_PARTIALS 1024
#define REC_ENSFM_GRAM_MAX_BLOCKS 256

int rec_ensfm_tower_fwd(int64_t n, int32_t num_fields, int32_t emb_dim, int64_t num_rows, int64_t bias_rows, const int64_t* ids,
                        const float* table, int64_t ld_table, const float* bias_table, const float* H_s, const float* bias,
                        int32_t item_layout, float* out, int64_t ld_out, int32_t* status, void* stream);
int rec_ensfm_tower_bwd(int64_t n, int32_t num_fields, int32_t emb_dim, int64_t num_rows, const int64_t* ids, const float* table,
                        int64_t ld_table, const float* H_s, const float* d_out, int64_t ld_dout, int32_t item_layout, float* rows,
                        int64_t ld_rows, float* dscore, float* partials, float* dH_s, float* dbias, int32_t accumulate,
                        void* stream);
int rec_ensfm_gram(int64_t n, int32_t cols, const float* X, int64_t ldx, float* partials, float* G, void* stream);
int rec_ensfm_pos_user(int64_t batch, int32_t max_pos, int32_t emb_dim, int64_t num_items, float neg_weight, const int64_t* ur,
                       const float* p, int64_t ld_p, const float* q, int64_t ld_q, const float* H_i, const float* G_q, float* g,
                       float* pos_r, float* dP, int64_t ld_dp, float* loss_part, float* dHi_part, int32_t* status, void* stream);
int rec_ensfm_pos_item(int64_t batch, int32_t max_pos, int32_t emb_dim, int64_t num_items, float neg_weight, const int32_t* n_uniq,
                       const int64_t* uniq_rows, const int32_t* seg_offset, const int32_t* sorted_pos, const float* g,
                       const float* p, int64_t ld_p, const float* q, int64_t ld_q, const float* H_i, const float* G_p, float* dQ,
                       int64_t ld_dq, void* stream);
int rec_ensfm_loss(int64_t batch, int32_t emb_dim, float neg_weight, const float* G_p, const float* G_q, const float* H_i,
                   const float* loss_part, const float* dHi_part, float* loss, float* dH_i, void* stream);
int rec_ensfm_score(int64_t batch, int64_t num_rows, int32_t emb_dim, const float* p, int64_t ld_p, const float* q, int64_t ld_q,
                    const float* H_i, float* pre, int64_t ld_pre, void* stream);

/* ----------------------------------------------------------------------------------------
 * NCF (models/recall/ncf): NeuMF, GMF and MLP (csrc/ncf_ops.hip).  float32; no float atomics; every sum has a fixed order and
 * nothing depends on the order in which blocks run, so a rerun is bit-identical.  Arguments are checked on the host before
 * any launch (REC_EINVAL, the entry and the argument named in rec_last_error()); batch == 0 returns REC_OK without a launch
 * after those checks.
 *
 * The net ("desc" below) is five arguments of every entry: mf_dim (0: MLP mode), n_fc Linear layers in the tower (0: GMF
 *   mode), widths: a HOST array of n_fc + 1 int32 (may be NULL when n_fc is 0) with widths[0] = fc_layers[0] (the tower's
 *   input, even) and widths[l] = the output of Linear l (1..n_fc), num_users and num_items.  half = widths[0] / 2 (0 in GMF
 *   mode).
 * Packed tables: a user's MF row and MLP row are ONE row of user_table [num_users, Cu], Cu = mf_dim + half, MF first; the
 *   items the same in item_table [num_items, Ci], Ci = Cu.  Every table and output takes a row stride (ld >= width; the floats
 *   between rows are never read or written).
 * Dense buffer [P] (rec_ncf_dense_numel): for l = 1..n_fc: W_l [widths[l-1], widths[l]] row-major (Paddle's [in, out]), then
 *   b_l [widths[l]]; then prediction.weight [mf_dim + widths[n_fc]] (MF columns first; mf_dim alone in GMF mode) and
 *   prediction.bias [1].  EVERY tensor starts at a multiple of 4 floats: its size is rounded up, the padding floats are
 *   zero, get a zero gradient and so stay zero under rec_adam_dense.
 * An id outside its table sets REC_FLAG_INDEX_OOB in *status (may be NULL), reads as a zero row and gets a zero gradient row.
 *
 * rec_ncf_fused_eligible: *eligible = 1 when rec_ncf_step / rec_ncf_score take the net: n_fc <= REC_NCF_MAX_FC, mf_dim and every
 *   width <= REC_NCF_MAX_WIDTH, and 4 * (2 P + REC_NCF_TILE * S) <= REC_NCF_LDS_BYTES, where S = the floats of one sample of
 *   a tile: sum_{l=0..n_fc} (widths[l] | 1) activations, sum_{l=1..n_fc} (widths[l] | 1) deltas, 2 (mf_dim | 1) MF rows,
 *   dz, the loss term and the two validated ids (2 floats each).  A malformed desc is REC_EINVAL, not "ineligible".
 * rec_ncf_step: forward, log loss (Paddle's epsilon 1e-4) and backward in ONE launch, then a fold launch.  labels int64 [batch];
 *   mean_over: the mean's denominator (0 -> batch).  Outputs: pred [batch]; g_user [batch, Cu] (ld_gu) and g_item [batch, Ci]
 *   (ld_gi): the gradient row of every sample's lookup, rec_grad_layout{1,0,0} for rec_adam_rows_all; partials
 *   [min(ceil(batch / REC_NCF_TILE), REC_NCF_MAX_BLOCKS), P + 1]: every block's dense gradients and loss sum; g_dense [P] and
 *   loss [1]: their fold in ascending block order.  Block b takes the tiles b, b + G, ... in order; an element of a dense
 *   gradient is summed by one owner thread over a tile's samples in ascending order.  An ineligible net is REC_EINVAL.
 * rec_ncf_score: the same forward alone -> pred [batch].
 * rec_ncf_gather_fwd / rec_ncf_gather_bwd: the glue of the general route (any tower; they read mf_dim, widths[0] and whether
 *   n_fc is 0).  Forward: pred_in[b, :mf_dim] = mf_u o mf_i (ld_pred_in; the other columns are not touched: the tower's last
 *   rec_gemm_f32 writes them) and mlp_in [batch, widths[0]] = [mlp_u, mlp_i] (ld_mlp_in).  pred_in may be NULL when mf_dim is
 *   0, mlp_in when n_fc is 0.  Backward: from d_pred_in (its first mf_dim columns) and d_mlp_in it writes g_user / g_item as
 *   rec_ncf_step does.
 * ---------------------------------------------------------------------------------------- */
#define REC_NCF_MAX_FC 4
#define REC_NCF_MAX_WIDTH 128
#define REC_NCF_TILE 32
#define REC_NCF_MAX_BLOCKS 512
#define REC_NCF_LDS_BYTES 65536
int rec_ncf_dense_numel(int32_t mf_dim, int32_t n_fc, const int32_t* widths, int64_t num_users, int64_t num_items, int64_t* numel);
int rec_ncf_fused_eligible(int32_t mf_dim, int32_t n_fc, const int32_t* widths, int64_t num_users, int64_t num_items,
                           int32_t* eligible);
int rec_ncf_step(int32_t mf_dim, int32_t n_fc, const int32_t* widths, int64_t num_users, int64_t num_items, int64_t batch,
                 int64_t mean_over, const int64_t* users, const int64_t* items, const int64_t* labels, const float* user_table,
                 int64_t ld_user, const float* item_table, int64_t ld_item, const float* dense, float* pred, float* g_user,
                 int64_t ld_gu, float* g_item, int64_t ld_gi, float* partials, float* g_dense, float* loss, int32_t* status,
                 void* stream);
int rec_ncf_score(int32_t mf_dim, int32_t n_fc, const int32_t* widths, int64_t num_users, int64_t num_items, int64_t batch,
                  const int64_t* users, const int64_t* items, const float* user_table, int64_t ld_user, const float* item_table,
                  int64_t ld_item, const float* dense, float* pred, int32_t* status, void* stream);
int rec_ncf_gather_fwd(int32_t mf_dim, int32_t n_fc, const int32_t* widths, int64_t num_users, int64_t num_items,
                       int64_t batch, const int64_t* users, const int64_t* items, const float* user_table, int64_t ld_user,
                       const float* item_table, int64_t ld_item, float* pred_in, int64_t ld_pred_in, float* mlp_in,
                       int64_t ld_mlp_in, int32_t* status, void* stream);
int rec_ncf_gather_bwd(int32_t mf_dim, int32_t n_fc, const int32_t* widths, int64_t num_users, int64_t num_items,
                       int64_t batch, const int64_t* users, const int64_t* items, const float* user_table, int64_t ld_user,
                       const float* item_table, int64_t ld_item, const float* d_pred_in, int64_t ld_dpred_in,
                       const float* d_mlp_in, int64_t ld_dmlp_in, float* g_user, int64_t ld_gu, float* g_item, int64_t ld_gi,
                       void* stream);

/* ----------------------------------------------------------------------------------------
 * DSSM (models/match/dssm): the two-tower semantic-matching net (csrc/dssm_ops.hip).  float32; no float atomics; every sum
 * has a fixed order and nothing depends on the order in which blocks run, so a rerun is bit-identical.  Arguments are checked
 * on the host before any launch (REC_EINVAL, the entry and the argument named in rec_last_error()); a call with no rows
 * returns REC_OK without a launch after those checks.  No entry takes a workspace: every intermediate is a named buffer.
 *
 * A tower input of `rows` multi-hot rows over in_dim letter trigrams is CSR: cols [nnz] int64 (ascending within a row), vals
 * [nnz] float32, lod [rows + 1] int64 (lod[r] .. lod[r + 1] are row r's entries; values are clamped to 0 .. nnz).
 *
 * rec_dssm_lod_rows: row_of[j] = the row that holds entry j, int32 [nnz] (what the backward reads; a reader may supply it).
 * rec_dssm_sparse_linear_fwd: Y[r, :] = act(bias + sum_j vals[j] * W[cols[j], :]) over row r's entries in stored order; W
 *   [in_dim, n] row-major (ld_w), act = ReLU when relu != 0.  A row without entries gives act(bias).  A column outside
 *   [0, in_dim) sets REC_FLAG_INDEX_OOB in *status (may be NULL) and is skipped.  float4 lanes when n, ld_w and ld_y are
 *   multiples of 4 and W, bias and Y are 16-byte aligned, one float per lane otherwise.
 * rec_dssm_sparse_linear_bwd: dW[c, :] = sum vals[j] * dY[row_of[j], :] over the entries j with cols[j] == c in ascending j,
 *   for EVERY c of [0, in_dim): a column no row holds gets zeros, so no memset precedes the call.  The entries grouped by
 *   column are rec_ids_group's outputs for ids = cols, num_rows = in_dim (sorted_pos [nnz]: entry indices, stable; uniq_rows,
 *   seg_offset, n_uniq as documented there; out-of-range columns were dropped there).  One block of REC_DSSM_BWD_WAVES waves
 *   per column: wave w sums the w-th part of the column's entries (ceil(len / waves) each, ascending), the parts are folded in
 *   ascending w.  n <= REC_DSSM_MAX_WIDTH (the parts' LDS).  dY is the gradient already masked by the layer's ReLU; there is
 *   no dX (the inputs are data) and db is rec_colsum(dY).
 * rec_dssm_head_step: cosine, softmax, loss and their backward in one launch plus a one-wave fold.  q [batch, n] (ld_q);
 *   d [(1 + neg) * batch, n] (ld_d) field-major: the positives' rows first, then each negative's.  cos[b, k] = w12 /
 *   sqrt(max(w1 * w2, 1e-16)) (Paddle's cosine_similarity, eps 1e-8) -> cos [batch, 1 + neg]; hit_prob[b] =
 *   softmax_k(cos[b, :])[0] -> [batch]; loss_terms[b] = -log(hit_prob[b]) -> [batch]; loss [1] = the mean of the first M =
 *   min(batch, slice_end) terms in a fixed order; dq [batch, n] (ld_dq) and dd [(1 + neg) * batch, n] (ld_dd) = d loss, zeros
 *   for rows b >= M.  Where w1 * w2 < 1e-16 the clamped branch holds in value and gradient (d cos / d x = y / 1e-8).
 *   relu_mask != 0: q and d are ReLU outputs, and dq / dd are zeroed where they are not positive.  neg = 0 is legal;
 *   1 + neg <= REC_DSSM_MAX_DOCS; slice_end >= 1.
 * rec_dssm_cos: cos[b] of q [batch, n] against d [batch, n] alone (inference).
 * ---------------------------------------------------------------------------------------- */
#define REC_DSSM_MAX_DOCS 64
#define REC_DSSM_MAX_WIDTH 2048
#define REC_DSSM_BWD_WAVES 8
int rec_dssm_lod_rows(int64_t rows, int64_t nnz, const int64_t* lod, int32_t* row_of, void* stream);
int rec_dssm_sparse_linear_fwd(int64_t rows, int64_t nnz, int64_t in_dim, int32_t n, int32_t relu, const int64_t* cols,
                               const float* vals, const int64_t* lod, const float* W, int64_t ld_w, const float* bias, float* Y,
                               int64_t ld_y, int32_t* status, void* stream);
int rec_dssm_sparse_linear_bwd(int64_t rows, int64_t nnz, int64_t in_dim, int32_t n, const float* vals, const int32_t* row_of,
                               const int32_t* sorted_pos, const int64_t* uniq_rows, const int32_t* seg_offset,
                               const int32_t* n_uniq, const float* dY, int64_t ld_dy, float* dW, int64_t ld_dw, void* stream);
int rec_dssm_head_step(int64_t batch, int32_t neg, int32_t n, int64_t slice_end, int32_t relu_mask, const float* q, int64_t ld_q,
                       const float* d, int64_t ld_d, float* cos, float* hit_prob, float* loss_terms, float* loss, float* dq,
                       int64_t ld_dq, float* dd, int64_t ld_dd, void* stream);
int rec_dssm_cos(int64_t batch, int32_t n, const float* q, int64_t ld_q, const float* d, int64_t ld_d, float* cos, void* stream);

/* ----------------------------------------------------------------------------------------
 * MatchPyramid (models/match/match-pyramid): the interaction image of two sentences, convolved, rectified and max-pooled
 * (csrc/match_pyramid_ops.hip).  float32; no float atomics; every sum has a fixed order and nothing depends on the order in
 * which blocks run, so a rerun is bit-identical.  Arguments are checked on the host before any launch (REC_EINVAL, the entry
 * and the argument named in rec_last_error()); batch == 0 returns REC_OK without a launch after those checks.
 *
 * shape: a HOST array of REC_MPYR_SHAPE_LEN int32 = {left_len Ll, right_len Lr, emb_dim E, channels K, filter_h, filter_w,
 *   pool_h, pool_w, stride_h, stride_w, relu (0: no activation)}; the table has `vocab` rows of row stride ld_table;
 *   padding_idx -1: none.
 *   cross[i, j] = <table[left[i]], table[right[j]]>; a padding id, and an id outside [0, vocab), is a zero row (the latter
 *   sets REC_FLAG_INDEX_OOB in *status, which may be NULL, and reads nothing).  The convolution is stride 1, padding "SAME": k - 1
 *   zeros per axis, floor((k - 1) / 2) of them in front; conv_w is [K, 1, filter_h, filter_w], conv_b [K].  The pool is VALID:
 *   PH = (Ll - pool_h) / stride_h + 1, PW likewise; rows and columns beyond the last window are never computed.
 *   Limits (the LDS staging): Ll <= REC_MPYR_MAX_LEFT, Lr <= REC_MPYR_MAX_RIGHT, E <= REC_MPYR_MAX_EMB, filter_h * filter_w *
 *   roundup(K, 8) <= REC_MPYR_MAX_WEIGHTS, K * PH * PW <= REC_MPYR_MAX_POOLED, and the band one row of pool windows reads,
 *   (pool_h + filter_h - 1) * (Lr + filter_w - 1) floats, <= REC_MPYR_MAX_BAND; filter and pool no larger than the image.
 * rec_mpyr_fwd: left int64 [batch, Ll], right int64 [batch, Lr] -> pooled [batch, K * PH * PW] (ld_pooled) in NCHW order
 *   (k * PH * PW + ph * PW + pw) and argmax int32 of the same shape (ld_argmax): the cell i * Lr + j that won its window, the
 *   first in row-major order among equals.  One block per (sample, row of pool windows).
 * rec_mpyr_bwd: d_pooled (ld_dpooled) and the forward's argmax and inputs -> dL [batch * Ll, E] (ld_dl) and dR [batch * Lr, E]
 *   (ld_dr), every row written, the rows of padding and out-of-range ids exactly 0; d_conv_w [K * filter_h * filter_w] and
 *   d_conv_b [K].  A window whose winner's pre-activation is <= 0 under relu passes nothing; a cell that won several windows
 *   of a channel receives all of them, summed first in ascending window order (at the first of them).  The image is recomputed, not stored.  Two named intermediates: gated [batch, K * PH * PW] (the
 *   gradient that passes each window) and partials [batch * PH, K * filter_h * filter_w + K] (every block's share of d_conv_w |
 *   d_conv_b, folded in a fixed order: 16 interleaved ascending sums, then a tree).  d_cross is formed in gather form: a cell sums the windows whose winner's tap
 *   footprint reaches it in ascending (ph, pw, k).
 *   batch == 0 launches nothing and leaves every output, d_conv_w and d_conv_b included, untouched.
 * rec_mpyr_hinge: loss [1] = mean_{r < pairs} max(0, 1 - pred[r] + pred[pairs + r]) (dygraph_model.py:55-69 with pairs = 64);
 *   d_pred [batch]: -1 / pairs and +1 / pairs for the two rows of an open pair (0 <= the hinge's argument: the gradient flows at
 *   exactly 0), 0 for a closed one and for rows at or beyond 2 * pairs.  One block, fixed-order fold.  2 * pairs <= batch.
 * ---------------------------------------------------------------------------------------- */
#define REC_MPYR_MAX_LEFT 32
#define REC_MPYR_MAX_RIGHT 1024
#define REC_MPYR_MAX_EMB 128
#define REC_MPYR_MAX_WEIGHTS 1024
#define REC_MPYR_MAX_POOLED 1024
#define REC_MPYR_MAX_BAND 7168
#define REC_MPYR_SHAPE_LEN 11
int rec_mpyr_fwd(int64_t batch, const int32_t* shape, int64_t vocab, int64_t ld_table, int64_t padding_idx, const int64_t* left,
                 const int64_t* right, const float* table, const float* conv_w, const float* conv_b, float* pooled,
                 int64_t ld_pooled, int32_t* argmax, int64_t ld_argmax, int32_t* status, void* stream);
int rec_mpyr_bwd(int64_t batch, const int32_t* shape, int64_t vocab, int64_t ld_table, int64_t padding_idx, const int64_t* left,
                 const int64_t* right, const float* table, const float* conv_w, const float* conv_b, const float* d_pooled,
                 int64_t ld_dpooled, const int32_t* argmax, int64_t ld_argmax, float* gated, float* partials, float* dL,
                 int64_t ld_dl, float* dR, int64_t ld_dr, float* d_conv_w, float* d_conv_b, void* stream);
int rec_mpyr_hinge(int64_t batch, int64_t pairs, const float* pred, float* loss, float* d_pred, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* RECENGINE_H_ */
