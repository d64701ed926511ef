/* mkb_hip.h -- C ABI of libmkb_hip.so: the MI355X (gfx950) kernels behind mkb's triplet-scoring,
 * self-adversarial loss and filtered negative-sampling hot path.
 *
 * The reference (raphaelsty/mkb) is pure Python on PyTorch and has NO FFI / plugin interface
 * (SURVEY.md 8b); the boundary it offers is its public Python API.  Each entry point below names the
 * reference call it stands in for (paths relative to /root/reference).  The host side
 * (the mkb_amd Python package) mirrors that Python API and calls these symbols through ctypes.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer unless its name ends in _host; the caller (Python glue) owns and
 *     allocates every buffer, nothing is allocated or freed across the ABI except opaque handles;
 *   - `stream` is a hipStream_t passed as void* (0 = default stream); every call is asynchronous with
 *     respect to the host and ordered on that stream;
 *   - return value: 0 = ok, <0 = mkb_status_t error; mkb_last_error() gives the message (thread local);
 *   - floating point is IEEE fp32, indices are int64 (torch.LongTensor) unless stated;
 *   - tables are row-major contiguous: ent [n_entity, entity_dim], rel [n_relation, relation_dim];
 *     RotatE / ComplEx rows hold the real half first, then the imaginary half (models/rotate.py:76-77).
 */
#ifndef MKB_HIP_H
#define MKB_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 9: lr, beta1 and beta2 of the five mkb_adam_* calls are doubles (floats through 8).  The notes "under ABI 8" below say when a
 * group of symbols was added; all of them are part of 9. */
#define MKB_ABI_VERSION 9

typedef enum {
    MKB_OK = 0,
    MKB_ERR_INVALID = -1,   /* bad argument (shape, enum, null pointer, misalignment)            */
    MKB_ERR_HIP = -2,       /* a HIP runtime call failed                                          */
    MKB_ERR_KEY = -3,       /* sampler: (r,t) / (h,r) not in the training triples (ref: KeyError) */
    MKB_ERR_EMPTY = -4,     /* sampler: a row's filter removed the whole pool (ref: infinite loop)*/
    MKB_ERR_UNSUPPORTED = -5
} mkb_status_t;

/* models/transe.py:65, rotate.py:69, complex.py:65, distmult.py:63, protate.py:74 */
typedef enum { MKB_TRANSE = 0, MKB_ROTATE = 1, MKB_COMPLEX = 2, MKB_DISTMULT = 3, MKB_PROTATE = 4 } mkb_model_t;

/* models/base.py:153-164: any mode string other than the two below selects the default batch */
typedef enum { MKB_MODE_DEFAULT = 0, MKB_MODE_HEAD = 1, MKB_MODE_TAIL = 2 } mkb_mode_t;

/* Parameter set of one model == the nn.Parameters of models/base.py:66-100 (+ modulus, protate.py:72). */
typedef struct {
    int32_t model;            /* mkb_model_t */
    int32_t hidden_dim;
    int64_t n_entity, n_relation;
    int64_t entity_dim, relation_dim;
    const float *ent;         /* [n_entity, entity_dim]                       */
    const float *rel;         /* [n_relation, relation_dim]                   */
    const float *modulus;     /* [1] device scalar (pRotatE), may be null     */
    float gamma;              /* gamma.item()                                 */
    float phase_div;          /* fp32(embedding_range.item() / pi): rotate.py:79, protate.py:78-80 */
} mkb_tables_t;

/* Dense gradient buffers == .grad of the same parameters (accumulated into, never zeroed here). */
typedef struct {
    float *g_ent;             /* [n_entity, entity_dim]   */
    float *g_rel;             /* [n_relation, relation_dim] */
    float *g_modulus;         /* [1] (pRotatE) or null    */
    int32_t rows_clear;       /* mkb_pool_step / _bwd only, a promise of the caller: the g_ent rows of this batch's entities
                                 (pool ids, heads, tails) are all-zero on entry (fresh buffers; or the row-lazy optimizer's
                                 advance launch has just consumed and cleared them).  Rows that a single workgroup writes are
                                 then stored instead of read-modify-written.  0 = accumulate as always. */
} mkb_grads_t;

int mkb_abi_version(void);
const char *mkb_last_error(void);

/* Range check of the ids a scoring call is about to use: the reference's index_select (models/base.py:166-207) raises
 * IndexError for an id outside the table; the kernels index the tables directly, so the glue runs this (one small launch)
 * on user-supplied ids and raises when it next synchronises.  sample [B, 3], cand [n_cand] (or null); flag: one int32 on
 * the device, OR-ed with 1 (entity id in sample), 2 (relation id), 4 (candidate id) when something is out of range. */
int mkb_check_ids(const int64_t *sample, int64_t B, const int64_t *cand, int64_t n_cand, int64_t n_entity,
                  int64_t n_relation, int32_t *flag, void *stream);

/* ---- general scoring (arbitrary candidate ids) ------------------------------------------------------
 * mkb_score_fwd == model.forward(sample, negative_sample, mode)          (forward of each file under models/)
 *   sample [B,3]; cand [B,K] candidate entity ids (head-batch: heads, tail-batch: tails) or null with
 *   K = 1 for MKB_MODE_DEFAULT (candidate = the true tail, base.py:166-175); score [B,K] out.
 * mkb_score_bwd == autograd of the same call: accumulates d loss/d tables given dscore [B,K]
 *   (index_select backward = dense index_add_).
 */
int mkb_score_fwd(const mkb_tables_t *tb, const int64_t *sample, const int64_t *cand, int64_t B, int64_t K,
                  int mode, float *score, void *stream);
/* ws: caller-owned scratch of mkb_score_bwd_workspace_bytes(tb, B, K, mode) bytes, 256-byte aligned (the B*K (row, slot)
 * pairs radix-sorted by candidate, the queries, the sort's own storage); may be null when that returns 0 (default mode,
 * K = 1).  Nothing is allocated inside the call. */
int64_t mkb_score_bwd_workspace_bytes(const mkb_tables_t *tb, int64_t B, int64_t K, int mode);
int mkb_score_bwd(const mkb_tables_t *tb, const mkb_grads_t *gr, const int64_t *sample, const int64_t *cand,
                  int64_t B, int64_t K, int mode, const float *dscore, void *ws, void *stream);

/* ---- self-adversarial loss ---------------------------------------------------------------------------
 * mkb_adversarial == losses.Adversarial(alpha)(positive_score, negative_score, weight) AND its gradient
 * (losses/adversarial.py:21-30): loss[1], dpos[B], dneg[B,K] out.  cnt (uint16 [B,K]) is an optional
 * per-column multiplicity (null = all ones) used by the pooled path, where a column is a pool position.
 * scratch: B+1 floats of caller-owned device memory (W and the per-row partial sums; the reduction is a
 * fixed tree, so the loss is bit-reproducible run to run).
 * weight_sum: null, or a device scalar holding W when the rows are a SHARD of a larger batch (data-parallel
 * ranks pass the all-reduced sum of weights; loss then is this shard's share of the global loss).
 */
int mkb_adversarial(const float *pos, const float *neg, const float *weight, const uint16_t *cnt, int64_t B,
                    int64_t K, float alpha, const float *weight_sum, float *loss, float *dpos, float *dneg,
                    float *scratch, void *stream);

/* ---- negative-sampling loss family: margin ranking, pairwise logistic, sampled softmax ----------------------
 * No reference counterpart (the reference trains with Adversarial only); mkb_amd/csrc/ns_loss.hip.  New symbol under ABI 8: the
 * version is not bumped.  pos [B], neg [B, K] row-major, weight [B] or null (all ones), cnt [B, K] uint16 or null (all ones):
 * per-column multiplicities c_ij as for mkb_adversarial.  W = sum of weight (B when weight is null), or weight_sum[0] when given
 * (the rows are a shard, as for mkb_adversarial).  Scores are "higher is more plausible".
 *   MKB_LOSS_MARGIN / MKB_LOSS_PAIR_LOGISTIC (param = margin): a_ij = param + neg_ij - pos_i, row_i = sum_j p_ij f(a_ij) with
 *     f = max(0, a) / softplus(a) and the detached weight p_ij = c_ij exp(alpha neg_ij) / sum_l c_il exp(alpha neg_il)
 *     (alpha = 0: c_ij / C_i);  dneg_ij = (w_i / W) p_ij f'(a_ij) (margin: 1 where a > 0, else 0), dpos_i = -sum_j dneg_ij.
 *   MKB_LOSS_SOFTMAX (param = temperature T > 0; alpha is not used): row_i = log(exp(pos_i / T) + sum_j c_ij exp(neg_ij / T))
 *     - pos_i / T;  dneg_ij = (w_i / (W T)) c_ij exp(neg_ij / T) / Z_i, dpos_i = (w_i / (W T)) (exp(pos_i / T) / Z_i - 1).
 *   loss [1] = sum_i w_i row_i / W; dpos [B], dneg [B, K] = d loss / d pos, d loss / d neg.  A position with c_ij = 0 takes no part:
 *   its neg value is not used (it may be NaN) and its dneg is written as 0; a row that uses no position contributes 0.
 * scratch: B + 1 floats.  Forward and seeds in one pass over each row; fixed-order reductions, no float atomics: two runs give the
 * same bits.  Any K (rows of more than 1024 columns are re-read from global memory instead of staged in LDS).
 * A null pos / neg / loss / dpos / dneg / scratch, an unknown kind, B < 1, K < 1, B * K > 2^31 - 1, alpha < 0 or not finite, a
 * non-finite param, T <= 0 for the softmax -> MKB_ERR_INVALID before any launch. */
typedef enum { MKB_LOSS_MARGIN = 0, MKB_LOSS_PAIR_LOGISTIC = 1, MKB_LOSS_SOFTMAX = 2 } mkb_loss_t;
int mkb_ns_loss(int kind, const float *pos, const float *neg, const float *weight, const uint16_t *cnt, int64_t B, int64_t K,
                float param, float alpha, const float *weight_sum, float *loss, float *dpos, float *dneg, float *scratch,
                void *stream);

/* ---- negative sampler --------------------------------------------------------------------------------
 * mkb_sampler_create == sampling.NegativeSampling.__init__ (negative_sampling.py:133-151): takes the two
 *   filter dictionaries of positive_triples() (negative_sampling.py:7-28) as CSR on the HOST:
 *   keys sorted ascending (head filter: r*n_entity+t -> heads; tail filter: h*n_relation+r -> tails),
 *   offsets [nk+1], values sorted ascending within each set.  Copies them to the device.  K <= 1024.
 * mkb_sampler_generate == NegativeSampling.generate(sample, mode) (negative_sampling.py:158-201), bit-exact
 *   with numpy's legacy MT19937 randint + np.in1d(assume_unique=True, invert=True) of numpy >= 1.24:
 *   neg [B,K] int64 out; optional outs for the pooled scoring path: pool [2K] int64 (the shared candidate
 *   draw), pos [B,K] int32 (neg[i,j] == pool[pos[i,j]]), cnt [B,2K] uint16 (multiplicity of each pool
 *   position in row i), touched [2K + 2B] int64 (the entity rows a training step on this batch reads: the pool,
 *   then the batch's heads, then its tails -- the id list of mkb_adam_rows_advance / _step).  status [1] int32 device out: 0 / MKB_ERR_KEY / MKB_ERR_EMPTY (first failing row
 *   in status[1]); checked lazily by the host with mkb_sampler_status.
 */
typedef struct mkb_sampler mkb_sampler_t;
int mkb_sampler_create(mkb_sampler_t **out, int64_t n_entity, int64_t n_relation, int64_t K, uint32_t seed,
                       const int64_t *head_keys_host, int64_t n_head_keys, const int64_t *head_offsets_host,
                       const int64_t *head_values_host, const int64_t *tail_keys_host, int64_t n_tail_keys,
                       const int64_t *tail_offsets_host, const int64_t *tail_values_host, void *stream);
int mkb_sampler_generate(mkb_sampler_t *s, const int64_t *sample, int64_t B, int mode, int64_t *neg,
                         int64_t *pool, int32_t *pos, uint16_t *cnt, int64_t *touched, void *stream);
int mkb_sampler_status(mkb_sampler_t *s, void *stream); /* synchronises `stream`; returns 0 or the error */
/* Optional NON-PARITY pool draw (the reference has no counterpart; BASELINE north_star names it): kind 1 = rocRAND
 * Philox4x32-10 inside the same draw kernel (masked rejection like numpy's randint; counter based, so `draws` -- the number
 * of pools drawn so far -- is the whole generator state); kind 0 (default) = numpy's legacy MT19937, bit-exact negatives. */
int mkb_sampler_set_rng(mkb_sampler_t *s, int kind, uint64_t seed, uint64_t draws);
int mkb_sampler_get_rng(mkb_sampler_t *s, int *kind, uint64_t *seed, uint64_t *draws);
int mkb_sampler_get_state(mkb_sampler_t *s, uint32_t *key624_host, int32_t *pos_host, void *stream);
int mkb_sampler_set_state(mkb_sampler_t *s, const uint32_t *key624_host, int32_t pos, void *stream);
void mkb_sampler_destroy(mkb_sampler_t *s);

/* ---- pool samplers: negatives from a candidate pool the caller made --------------------------------------------------
 * No reference counterpart to match bit for bit (mkb/text/learn.py:366-400, in_batch_negative_triples, has the idea of one of
 * the pool sources); mkb_amd/csrc/sampler_pool.hip.  New symbols under ABI 9: the version is not bumped.
 * mkb_pool_filter: the per-row filter of a GIVEN pool [2K] of entity ids (duplicates allowed), with exact membership, and the
 *   outputs of mkb_sampler_generate with the same meaning, so that whatever consumes those (mkb_pool_step and its relatives)
 *   works unchanged.  sample [B, 3]; mode: MKB_MODE_HEAD (the row's target is its head, its query (?, r, t)) or MKB_MODE_TAIL.
 *   keys [n_keys]: the sorted key array of that side (mkb_amd/utils/true_keys.py: (a * n_relation + r) * n_entity + x, a the
 *   fixed entity, x the varying one), ascending and unique; null / 0 = no known answers.  A_i, the known answers of row i, is one
 *   contiguous range of it; a query with no key at all is legal (no MKB_ERR_KEY here).  Pool position p is KEPT for row i iff
 *   pool[p] is not in A_i and pool[p] is not the row's target (which is dropped even when the row's triple is not among the keys).
 *   neg [B, K] = concat(f, f, ...)[:K], f = the kept pool entries in pool order; pos [B, K] int32, neg[i, j] == pool[pos[i, j]];
 *   cnt [B, 2K] uint16, how often position p occurs among row i's K slots (every row sums to K); touched [2K + 2B] = the pool,
 *   then the batch's heads, then its tails.  pos, cnt and touched may be null.
 *   A row that keeps nothing: its neg / pos / cnt are zeroed and the call records MKB_ERR_EMPTY in status[0] and the smallest such
 *   row in status[1].  status [2] int32 on the device, 8-byte aligned, is zeroed ONCE by the caller and read when it likes: it
 *   accumulates over calls and no call waits for the device.
 *   A pool id outside [0, n_entity) is nobody's known answer and is never used as an index.  No float arithmetic and one writer
 *   per output element: two runs give the same bytes.
 *   K outside [1, 1024], B < 1, n_entity or n_relation outside [1, 2^31 - 1], a null sample / pool / neg / status, a status that
 *   is not 8-byte aligned, n_keys > 0 without keys, a mode other than head / tail -> MKB_ERR_INVALID before any launch.
 * mkb_pool_draw_alias: pool [2K] drawn from a discrete distribution over [0, n_entity) by the alias method.  accept [n_entity]
 *   int64 with values in [0, 2^32] and alias [n_entity] int32 are device tables (mkb_amd/sampling/pool_sampling.py builds them by
 *   Vose's method).  Counter based, like the rocRAND draw of mkb_sampler_set_rng: entry p of draw number `draw` uses Philox4x32-10
 *   at subsequence draw * 2K + p.  It chooses a column v uniform on [0, n_entity) by masked rejection (one 32-bit word per trial;
 *   n_entity = 1 consumes none), takes one more word u, and is v if (uint64)u < accept[v], else alias[v]: probability 1 and
 *   probability 0 are both exact.  words [2K, 2] uint32 or null: the accepted column word (0 when n_entity = 1) and u of every
 *   entry, for a host that wants to redo the integer arithmetic.
 *   A null accept / alias / pool, K outside [1, 1024], n_entity outside [1, 2^31 - 1] -> MKB_ERR_INVALID before any launch. */
int mkb_pool_filter(const int64_t *sample, int64_t B, int mode, int64_t n_entity, int64_t n_relation, const int64_t *pool, int64_t K,
                    const int64_t *keys, int64_t n_keys, int64_t *neg, int32_t *pos, uint16_t *cnt, int64_t *touched,
                    int32_t *status, void *stream);
int mkb_pool_draw_alias(const int64_t *accept, const int32_t *alias, int64_t n_entity, int64_t K, uint64_t seed, uint64_t draw,
                        int64_t *pool, uint32_t *words, void *stream);

/* ---- pooled training step ----------------------------------------------------------------------------
 * == compose/pipeline.py:211-236 for one batch whose negatives come from ONE shared pool
 * (negative_sampling.py:166): positive forward (mode None), negative forward (mode), Adversarial,
 * backward into the dense gradient buffers.  Uses pool/cnt from mkb_sampler_generate.
 *   ws: workspace of mkb_pool_step_workspace_bytes() bytes; pos_score [B] out, pool_score [B,2K] out
 *   (score of row i against pool position p, meaningful where cnt > 0: elsewhere the tile kernels write 0 and the GEMM
 *   route of ComplEx / DistMult leaves the unmasked product or, beyond the deepest position the row's tile uses, nothing),
 *   loss [1] out; weight_sum as in
 *   mkb_adversarial (null = sum of this call's weights).
 */
int mkb_pool_supported(const mkb_tables_t *tb, int64_t B, int64_t K); /* 1 if the pooled kernels cover this shape */
int64_t mkb_pool_step_workspace_bytes(const mkb_tables_t *tb, int64_t B, int64_t K);
int mkb_pool_step(const mkb_tables_t *tb, const mkb_grads_t *gr, const int64_t *sample, const float *weight,
                  const int64_t *pool, const uint16_t *cnt, int64_t B, int64_t K, int mode, float alpha,
                  const float *weight_sum, float *pos_score, float *pool_score, float *loss, void *ws, void *stream);
/* The two halves of mkb_pool_step (mkb_pool_step == fwd then bwd on the same buffers).  A caller that shards the
 * embedding DIMENSIONS over devices sums pos_score / pool_score across devices between the halves (scores are sums
 * over dims; gamma must enter once: e.g. only one device's tables carry it) and each device then back-propagates into its
 * own slice with no further exchange.
 * The backward half continues the forward half's workspace: besides the queries it holds the per-step occurrence counts
 * of the batch's entities (a gradient row whose entity occurs once is written without atomics) -- same ws, same batch,
 * forward first. */
int mkb_pool_step_fwd(const mkb_tables_t *tb, const int64_t *sample, const int64_t *pool, const uint16_t *cnt, int64_t B,
                      int64_t K, int mode, float *pos_score, float *pool_score, void *ws, void *stream);
int mkb_pool_step_bwd(const mkb_tables_t *tb, const mkb_grads_t *gr, const int64_t *sample, const float *weight,
                      const int64_t *pool, const uint16_t *cnt, int64_t B, int64_t K, int mode, float alpha,
                      const float *weight_sum, const float *pos_score, const float *pool_score, float *loss, void *ws,
                      void *stream);

/* pooled model.forward / its autograd as separate calls (README-style loops that call the model and the loss
 * themselves): pool_score [B,2K] out; dpool_score [B,2K] = d loss / d pool_score in. */
int mkb_pool_score_fwd(const mkb_tables_t *tb, const int64_t *sample, const int64_t *pool, const uint16_t *cnt,
                       int64_t B, int64_t K, int mode, float *pool_score, void *ws, void *stream);
int mkb_pool_score_bwd(const mkb_tables_t *tb, const mkb_grads_t *gr, const int64_t *sample, const int64_t *pool,
                       const uint16_t *cnt, int64_t B, int64_t K, int mode, const float *dpool_score, void *ws,
                       void *stream);

/* ---- distillation loss --------------------------------------------------------------------------------
 * == losses.KlDivergence()(student_score, teacher_score, T) (losses/kl_divergence.py:22-29), called by
 * distillation.Distillation.distill (distillation/distillation.py:633-683) from KdmkbModel.forward
 * (distillation/kdmkb_model.py:337-349): mean over all n*m entries of t (log t - log p), t = softmax(teacher / T, dim=1),
 * p = softmax(student / T, dim=1).  student, teacher: [n, m] row-major.  loss: 1 float.  dstudent [n, m] = d loss / d
 * student; dteacher [n, m] = d loss / d teacher, or null (the reference scores the teacher under no_grad).
 * scratch: n floats.
 */
int mkb_kl_divergence(const float *student, const float *teacher, int64_t n, int64_t m, float T, float *loss,
                      float *dstudent, float *dteacher, float *scratch, void *stream);

/* ---- dense Adam --------------------------------------------------------------------------------------
 * == torch.optim.Adam(lr, betas, eps).step() + zero_grad() for one parameter tensor as the README loop
 * uses it (README.md:123-126, pipeline.py:238-240): every element moves every step.  step is 1-based.
 * zero_grad != 0 also clears g (fused optimizer.zero_grad()).
 * lr, beta1 and beta2 are doubles, as torch holds them: 1 - beta and the bias corrections are formed in double from the caller's
 * own values and rounded once (from a float beta2 = 0.999f, 1 - beta2 is off by 1.3e-5 of itself, and exp_avg_sq with it).
 */
int mkb_adam_step(float *param, float *grad, float *exp_avg, float *exp_avg_sq, int64_t n, int64_t step, double lr,
                  double beta1, double beta2, float eps, int zero_grad, void *stream);

typedef struct {
    float *param, *grad, *exp_avg, *exp_avg_sq; /* a small dense tensor (e.g. the relation table), 16-byte aligned */
    int64_t n;                                  /* elements */
    int64_t step;                               /* its own step count (>= 1) */
} mkb_adam_dense_t;
/* mkb_adam_step for up to 8 parameter tensors in ONE launch (each with its own step count): what an optimizer over a model's
 * few dense tensors does per step -- small models are bound by launches, not by bytes (Umls TransE-64: 9 launches of ~5 us).
 * draw_ahead: null, or a sampler whose next pool draw runs as one more workgroup of this launch (see below). */
int mkb_adam_step_multi(const mkb_adam_dense_t *tensors_host, int n_tensors, double lr, double beta1, double beta2, float eps,
                        int zero_grad, mkb_sampler_t *draw_ahead, void *stream);

/* ---- row-lazy Adam: the same dense Adam, bit for bit, with the steps of untouched rows deferred (mkb_amd/csrc/adam.hip) ----
 * State of a table param [n_rows, D] besides exp_avg / exp_avg_sq: `last` [n_rows] int32 (zero-initialised; 0 = never
 * touched) = the step each row is current through; `consts` [capacity > step, 2] float = the per-step scalars
 * (-lr / (1 - beta1^s), sqrt(1 - beta2^s)), recorded by the launch that applies step s.
 *
 * mkb_adam_rows_step: apply step `step` with the real gradient to the rows in ids (duplicates allowed; they must be
 *   current through step - 1) and clear their gradient rows.  rider: null, or one dense tensor that takes its
 *   mkb_adam_step (with zero_grad) inside the same launch.
 * mkb_adam_rows_advance: make the listed rows current through step_upto by replaying their pending steps.
 *   grad == null, the plain catch-up: every pending step is a zero-gradient step; lr is ignored, a rider is refused.
 *   grad != null, the advance form: step step_upto itself was deferred (its mkb_adam_rows_step never ran).  The rows of
 *     that step's batch were made current through step_upto - 1 before its forward pass, so after backward they are
 *     "current through step_upto - 1, gradient of step_upto in the gradient row": the replay takes a row's gradient row
 *     (grad [n_rows, D]) for its FIRST pending step (zero for rows that were not touched then: the zero-gradient step, bit
 *     for bit) and clears it.  lr = learning rate of step_upto (recorded into consts[step_upto] by this launch); rider:
 *     null, or the small dense tensor that takes ITS step (rider->step) in the same launch.  mkb_adam_rows_step is then
 *     only needed for the very first step.  Callers must bring a row current BEFORE a backward pass writes its gradient row.
 *   The rows, in this order:
 *     global_ids [n_global > 0], world >= 1: GLOBAL entity ids of a row-sharded table (next section; e.g. the candidate
 *       pool, the same on every rank); entries another rank owns are skipped.  null, 0, 0, 0: the table is not sharded.
 *     ids [n_ids]: row (shard) indices; duplicates allowed, negative entries and entries >= n_rows are skipped; may be null.
 *     Both null: every row of the table (a flush: every direct read of the table must be preceded by one).
 *   draw_ahead: null, or a sampler whose NEXT pool draw (the single-workgroup kernel every mkb_sampler_generate starts
 *     with) runs as one more workgroup of this launch (ignored on a flush); the next mkb_sampler_generate on that sampler
 *     then only filters.  Same stream as the sampler's other calls; the negatives are bit-identical to drawing at generate
 *     time, and mkb_sampler_get_state keeps reporting the state before the pool drawn ahead.
 * mkb_adam_rows_advance_generate: mkb_sampler_generate(sampler, sample, B, mode, neg, pool, pos, cnt, touched) and
 *   mkb_adam_rows_advance over the rows that batch reads as ONE launch that also draws the sampler's next pool: the whole
 *   sampler runs in the shadow of the optimizer's replay.  Same outputs, bit for bit, as the two calls (size <= 512).
 *   world == 0: the rows are the batch's pool, heads and tails.  world >= 1 (shard of a row-sharded table; the sampler's
 *   pool holds global ids): the pool entries this rank owns, then the shard indices local_ids [n_local_ids].
 */
int mkb_adam_rows_step(float *param, float *grad, float *exp_avg, float *exp_avg_sq, int32_t *last, float *consts,
                       int64_t n_rows, int64_t D, const int64_t *ids, int64_t n_ids, int64_t step, double lr, double beta1,
                       double beta2, float eps, const mkb_adam_dense_t *rider, void *stream);
int mkb_adam_rows_advance(float *param, float *grad, float *exp_avg, float *exp_avg_sq, int32_t *last, float *consts,
                          int64_t n_rows, int64_t D, const int64_t *global_ids, int64_t n_global, int world, int rank,
                          const int64_t *ids, int64_t n_ids, int64_t step_upto, double lr, double beta1, double beta2,
                          float eps, const mkb_adam_dense_t *rider, mkb_sampler_t *draw_ahead, void *stream);
int mkb_adam_rows_advance_generate(float *param, float *grad, float *exp_avg, float *exp_avg_sq, int32_t *last, float *consts,
                                   int64_t n_rows, int64_t D, int world, int rank, const int64_t *local_ids,
                                   int64_t n_local_ids, int64_t step_upto, double lr, double beta1, double beta2, float eps,
                                   const mkb_adam_dense_t *rider, mkb_sampler_t *sampler, const int64_t *sample, int64_t B,
                                   int mode, int64_t *neg, int64_t *pool, int32_t *pos, uint16_t *cnt, int64_t *touched,
                                   void *stream);

/* ---- row-sparse Adagrad (mkb_amd/csrc/adagrad.hip) ----------------------------------------------------------------------
 * == torch.optim.Adagrad(lr, lr_decay, eps, weight_decay = 0).step() + zero_grad(), one launch per optimizer step:
 *   sum += g * g ; p -= clr * g / (sqrt(sum) + eps) ; g = 0        clr = lr / (1 + (step - 1) * lr_decay), computed by the caller
 * An element whose g is 0 keeps its p and sum exactly, so stepping only the rows a batch wrote is dense Adagrad bit for bit:
 * nothing is deferred, replayed or flushed.  State of a table param [n_rows, D]: sum [n_rows, D] and `last` [n_rows] int32
 * (zero-initialised) = the last step that visited a row; step is 1-based and strictly increasing per table.
 *   ids != null, the listed form: the rows ids[0 .. n_ids) take the step (duplicates allowed: one workgroup claims a row through
 *     `last`; negative entries and entries >= n_rows are skipped).  n_ids == 0: no row.
 *   ids == null && n_ids == 0, the all-rows form: every row of the table (a step whose written rows are not known).
 *   param == null, the dense-only form: no table; n_dense > 0.
 *   dense_host [n_dense <= 8]: small dense tensors (any alignment, any n) that take the same step, with the same clr, and have
 *     their gradients cleared by extra workgroups of the launch.
 *   draw_ahead: null, or a sampler whose NEXT pool draw runs as one more workgroup of this launch (as for mkb_adam_step_multi).
 */
typedef struct {
    float *param, *grad, *sum; /* a small dense tensor (the relation table, pRotatE's modulus); any alignment */
    int64_t n;                 /* elements */
} mkb_adagrad_dense_t;
int mkb_adagrad_step(float *param, float *grad, float *sum, int32_t *last, int64_t n_rows, int64_t D, const int64_t *ids,
                     int64_t n_ids, int64_t step, float clr, float eps, const mkb_adagrad_dense_t *dense_host, int n_dense,
                     mkb_sampler_t *draw_ahead, void *stream);

/* ---- row-sharded entity table (several GPUs; the reference is single-process: no counterpart to cite) ----------------
 * Rank g of `world` owns the entity rows e with e % world == g, at shard index e / world (table, dense gradient and Adam
 * state alike).  mkb_amd/table_rows.py moves rows between owners and users with these three calls and torch.distributed
 * (RCCL) collectives; the scoring step itself runs unchanged on a compact table [pool rows | ... | heads | tails].
 *
 * mkb_rows_route: group row requests by owner, request order kept inside a group.  sample_layout != 0: ids = sample [n, 3],
 *   the requests are its n heads followed by its n tails (2n requests); sample_layout == 0: ids = a flat list of n global
 *   entity ids.  send_ids = shard indices in grouped order (the payload of the id all-to-all), slot = where request j went,
 *   counts [world] = requests per owner (the all-to-all's split sizes), compact [n, 3] (sample layout only, or null) = the
 *   triples re-addressed into the compact table: (row0 + slot[j], r, row0 + slot[n + j]).
 * A row segment lists rows of the shard: world == 0: ids are shard indices; world > 0: ids are GLOBAL entity ids and only
 *   those this rank owns are touched (gather: the others become zero rows, so that an all-reduce over the ranks completes
 *   the block; scatter: skipped).  local_ids (gather, optional out [n]): the shard index of each entry, or -1.
 * mkb_rows_gather: rows[j] = shard[ids[j]] for up to 4 segments in one launch; riders of the same launch: weight_sum[0] =
 *   sum of weight [n_weight] (fixed-order tree; null = none) and clearing `zero` (zero_bytes, whole floats, 16-byte aligned; 0 = none).
 * mkb_rows_scatter_add: grad[ids[j]] += rows[j] (fp32 atomics: duplicates add); riders: dense_dst [dense_n] += dense_src,
 *   copy_dst [copy_n <= 256] = copy_src (how the step's loss leaves the reused step buffers without a launch of its own).
 * occ (optional, [n_local] uint32, zero-initialised ONCE by the caller): the gather launch counts how often each shard row
 *   is listed in its segments; the scatter launch of the SAME segments adds rows listed once without atomics and resets the
 *   counts.  null = always atomics.
 * bad (optional, int32 [1], zeroed by the caller): ids the reference's gather would answer with IndexError
 *   (models/base.py:193-207) never touch memory here -- bit 0: a negative id reached mkb_rows_route (routed as id 0);
 *   bit 1: a shard index outside [0, n_local) reached the gather / scatter (row skipped: zeros / nothing added). */
typedef struct {
    const int64_t *ids;
    int64_t n;
    float *rows;          /* [n, D] */
    int32_t world, rank;
    int64_t *local_ids;   /* gather only; may be null */
} mkb_row_seg_t;
int mkb_rows_route(const int64_t *ids, int64_t n, int sample_layout, int world, int64_t row0, int64_t *send_ids,
                   int32_t *slot, int64_t *counts, int64_t *compact, int32_t *bad, void *stream);
int mkb_rows_gather(const float *shard, int64_t n_local, int64_t D, const mkb_row_seg_t *segs, int n_segs,
                    const float *weight, int64_t n_weight, float *weight_sum, void *zero, int64_t zero_bytes, uint32_t *occ,
                    int32_t *bad, void *stream);
int mkb_rows_scatter_add(float *grad, int64_t n_local, int64_t D, const mkb_row_seg_t *segs, int n_segs, float *dense_dst,
                         const float *dense_src, int64_t dense_n, float *copy_dst, const float *copy_src, int64_t copy_n,
                         uint32_t *occ, int32_t *bad, void *stream);
/* The owner's row-lazy optimizer visits its shard with mkb_adam_rows_advance / _advance_generate at world >= 1 (above). */

/* ---- the row-sharded step's collectives, issued by the library (no reference counterpart: mkb is single-process) ------------
 * mkb_amd/table_rows.py used to issue the step's six collectives through torch.distributed and to read the all-to-alls' split
 * sizes back with an event wait: measured host-bound (0.43 ms / step against 0.19 ms of kernels, round 4).  With these entry
 * points the library holds its own RCCL communicators (bound at run time: mkb_rows_comm_available() is 0 on a box without
 * librccl, everything else still loads) and a step's communication is plan (ahead, side stream) + take + 2 x exchange.
 *
 * mkb_rows_comm_unique_id: rank 0 fills id_host [MKB_ROWS_COMM_ID_BYTES]; the caller hands the blob to every rank by whatever
 *   means it has (mkb_amd: one torch.distributed broadcast at set-up).
 * mkb_rows_comm_create: collective over the `world` ranks (each on its own current device).  max_requests = the largest 2 x b
 *   (positive-row requests of one rank's batch) any rank will ever plan: the id lists travel in fixed blocks of that capacity.
 * mkb_rows_comm_plan (slot in [0, 4): the caller's ring of plans in flight): on side_stream (after the work queued on
 *   after_stream so far, when given) -- mkb_rows_route on sample [b, 3] (send_ids [2b], slot_of [2b], counts [world],
 *   compact [b, 3]: as there), then the id exchange with in-band counts, then `want` [want_cap >= world's total requests to this
 *   owner; 2 b x world always suffices] = the shard indices the ranks ask this owner for, requester after requester.  Nothing
 *   returns to the host except through the mailbox below.  bad: as mkb_rows_route; bit 2 = a peer's block was malformed.
 * mkb_rows_comm_take: the split sizes of that plan -- sent_host [world] rows this rank asks each owner for, wanted_host [world]
 *   rows each rank asks this owner for -- read from a host-coherent mailbox the plan's last kernel wrote (no HIP call; spins
 *   only when the plan has not executed yet -- for at most MKB_ROWS_TAKE_TIMEOUT_S seconds (default 120), then MKB_ERR_HIP), and
 *   `stream` is made to wait for the plan.
 * mkb_rows_comm_exchange: on `stream`: the all-reduce (sum, in place) of reduce [reduce_n] floats (0 = none), then ONE RCCL
 *   group with the all-to-all of rows of D floats (MKB_ROWS_ONE_GROUP=1, and always at world 1: both in one group): send_rows_host[p] rows to rank p from `send` (consecutive), recv_rows_host[p] rows from
 *   rank p into `recv` (null count vectors = no all-to-all).  Forward: owners send `wanted`, users receive `sent`; the
 *   gradients' way back swaps the two.
 * mkb_rows_comm_stats: plans made, takes that found their plan not executed yet, and how many of those found `stream` idle
 *   (only those are bubbles on the device: the others mean the host ran ahead of it). */
#define MKB_ROWS_COMM_ID_BYTES 256
#define MKB_ROWS_MAX_WORLD 64
typedef struct mkb_rows_comm mkb_rows_comm_t;
/* what a plan posts for the host (inside a communicator: host-coherent memory): seq is stored LAST, with system-scope release */
typedef struct {
    int64_t seq;
    int64_t sent[MKB_ROWS_MAX_WORLD];    /* rows this rank asks each owner for (= the route's counts) */
    int64_t wanted[MKB_ROWS_MAX_WORLD];  /* rows each rank asks this owner for                        */
} mkb_rows_mailbox_t;
/* The two kernels of mkb_rows_comm_plan on their own (a caller with a transport of its own moves the blocks between them; the
 * tests play several ranks in one process with them).  blocks: [world][1 + cap] int64 -- pack writes block w = [counts[w] | the
 * ids of owner w's group of send_ids]; unpack reads block j = what rank j asks this owner for, writes `want` (requester after
 * requester), then mail->sent = counts, mail->wanted, and mail->seq = seq last.  mail: any device-visible memory. */
int mkb_rows_blocks_pack(const int64_t *counts, const int64_t *send_ids, int64_t *blocks, int world, int64_t cap, void *stream);
int mkb_rows_blocks_unpack(const int64_t *blocks, const int64_t *counts, int64_t *want, int64_t want_cap, mkb_rows_mailbox_t *mail,
                           int64_t seq, int32_t *bad, int world, int64_t cap, void *stream);
int mkb_rows_comm_available(void);
int mkb_rows_comm_unique_id(uint8_t *id_host);
/* In-process transport (ABI 6): RCCL refuses two ranks on one device, so plan / take / exchange cannot be driven for world > 1 on a
 * one-GPU box through it.  A communicator made by mkb_rows_comm_create_loopback moves its blocks and rows through a hub in THIS
 * process instead (device-to-device copies ordered by events, contributions of the all-reduce added in rank order): every rank is a
 * host thread with its own streams, all on the current device, and all the entry points above behave as they do over RCCL --
 * except that a peer that never makes the matching call, or disagrees about a split size, produces an ERROR after
 * MKB_ROWS_LOOP_TIMEOUT_S (default 20) seconds where RCCL would hang.  tests/test_gpu_rows_loopback.py; not used by the product. */
int mkb_rows_loop_hub_create(int world, void **hub);
void mkb_rows_loop_hub_destroy(void *hub);  /* after the communicators made over it */
int mkb_rows_comm_create_loopback(void *hub, int rank, int64_t max_requests, mkb_rows_comm_t **out);
int mkb_rows_comm_create(const uint8_t *id_host, int rank, int world, int64_t max_requests, mkb_rows_comm_t **out);
void mkb_rows_comm_destroy(mkb_rows_comm_t *comm);
int mkb_rows_comm_plan(mkb_rows_comm_t *comm, int slot, const int64_t *sample, int64_t b, int64_t row0, int64_t *send_ids,
                       int32_t *slot_of, int64_t *counts, int64_t *compact, int64_t *want, int64_t want_cap, int32_t *bad,
                       void *after_stream, void *side_stream);
int mkb_rows_comm_take(mkb_rows_comm_t *comm, int slot, int64_t *sent_host, int64_t *wanted_host, void *stream);
int mkb_rows_comm_exchange(mkb_rows_comm_t *comm, float *reduce, int64_t reduce_n, const float *send,
                           const int64_t *send_rows_host, float *recv, const int64_t *recv_rows_host, int64_t D, void *stream);
int mkb_rows_comm_stats(mkb_rows_comm_t *comm, int64_t *plans, int64_t *takes_that_waited, int64_t *waited_with_idle_stream);

/* ---- filtered ranking --------------------------------------------------------------------------------
 * == evaluation.Evaluation.compute_score for head-/tail-batch (evaluation/evaluation.py:217-279) with the
 * candidate list and filter bias of datasets.base.TestDataset (datasets/base.py:196-241): for each test triple
 * the rank of the target among all n_entity candidates, other true triples biased by -100000.
 *   true_keys: ascending int64 keys of ALL true triples (device), ordered for the mode so that one query's
 *   filter set is a contiguous range: tail-batch (h*n_relation + r)*n_entity + t, head-batch
 *   (t*n_relation + r)*n_entity + h.  rank [B] int64 out (1-based; ties count in the target's favour).
 *   ws: mkb_rank_workspace_bytes(tb, B) bytes, 256-byte aligned (queries + the [B, n_entity] score block).
 */
int64_t mkb_rank_workspace_bytes(const mkb_tables_t *tb, int64_t B);
int mkb_rank(const mkb_tables_t *tb, const int64_t *sample, int64_t B, int mode, const int64_t *true_keys,
             int64_t n_true, int64_t *rank, void *ws, int64_t ws_bytes, void *stream);
/* mkb_rank, and the score block the ranks were counted on handed out as well: scores [B, n_entity] fp32 =
 * model(sample, negative_sample = every entity id in order, mode) of evaluation.py:237 BEFORE the filter bias is added
 * (the same launches as mkb_rank plus one copy; the parity tests compare this block with the oracle's at full size, and
 * utils-style "score against all entities" callers get it without a [B, N, D] gather).  ABI 6. */
int mkb_rank_scores(const mkb_tables_t *tb, const int64_t *sample, int64_t B, int mode, const int64_t *true_keys,
                    int64_t n_true, int64_t *rank, float *scores, void *ws, int64_t ws_bytes, void *stream);

/* ---- filtered top-k entity prediction ------------------------------------------------------------------
 * For each query of `sample` [B, 3] int64 (device) the k best candidate entities of the mode's side, on the same all-entity
 * score block as mkb_rank_scores and the same candidate set as mkb_rank:
 *   mode: MKB_MODE_HEAD (candidates replace h; the query is (?, r, t)) or MKB_MODE_TAIL (candidates replace t; (h, r, ?)).
 *   true_keys: as for mkb_rank (ascending; tail-batch (h*n_relation + r)*n_entity + t, head-batch (t*n_relation + r)*n_entity + h);
 *   every entity whose corrupted triple is a key is left out; n_true == 0 filters nothing.  flags: MKB_TOPK_KEEP_TARGET keeps the
 *   query's own target (h for head-batch, t for tail-batch) in even when its triple is a key -- exactly the candidates the
 *   filtered rank is counted on; without it the target column of `sample` is not read as an entity id.
 *   ids [B, k] int64 / scores [B, k] fp32 out, best first in the order of the filtered rank: NaN first, then higher score, then
 *   lower entity id among equal scores (a stable descending sort).  scores are bit-identical to mkb_rank_scores' entries.  When
 *   fewer than k candidates are left, the trailing slots hold id -1 and score -inf.
 *   1 <= k <= MKB_TOPK_MAX_K (k > n_entity is allowed: padded); B as for mkb_rank; flags other than MKB_TOPK_KEEP_TARGET,
 *   a bad mode / k / B, null pointers or a short workspace -> MKB_ERR_INVALID before any launch.
 *   ws: mkb_topk_workspace_bytes(tb, B, k) bytes, 256-byte aligned (0 for a bad k).  No [B, n_entity] output.  ABI 7. */
#define MKB_TOPK_MAX_K 1024
#define MKB_TOPK_KEEP_TARGET 1
int64_t mkb_topk_workspace_bytes(const mkb_tables_t *tb, int64_t B, int k);
int mkb_topk(const mkb_tables_t *tb, const int64_t *sample, int64_t B, int mode, const int64_t *true_keys, int64_t n_true, int k,
             int flags, int64_t *ids, float *scores, void *ws, int64_t ws_bytes, void *stream);
/* mkb_topk over a subset of the entities: entity e is a candidate when bit e % 32 of word e / 32 of cand_bits
 * [ceil(n_entity / 32)] uint32 (device) is set.  An entity outside the mask is never returned: not with MKB_TOPK_KEEP_TARGET
 * either; it combines with the true_keys filter.  cand_bits == null: exactly mkb_topk, bit for bit.  Arguments, workspace
 * (mkb_topk_workspace_bytes(tb, B, k)), order and padding as for mkb_topk. */
int mkb_topk_masked(const mkb_tables_t *tb, const int64_t *sample, int64_t B, int mode, const int64_t *true_keys,
                    int64_t n_true, const uint32_t *cand_bits, int k, int flags, int64_t *ids, float *scores,
                    void *ws, int64_t ws_bytes, void *stream);
/* The same selection on a caller's fp32 block S [B, N] (device), rows ld >= N floats apart: for each row the k best columns,
 * NaN first, then higher value, then lower column; ids [B, k] int64 / scores [B, k] fp32 out (the block's own values, bit for
 * bit; -1 / -inf past the N columns).  No keys, no finisher, no workspace.  1 <= k <= MKB_TOPK_MAX_K, 0 <= B <= 2^31 - 1 (B = 0:
 * nothing), 1 <= N <= 2^31 - 1, ld >= N, non-null pointers; otherwise MKB_ERR_INVALID before any launch. */
int mkb_topk_block(const float *S, int64_t B, int64_t N, int64_t ld, int k, int64_t *ids, float *scores, void *stream);
/* Exact squared-L2 k nearest rows (a flat L2 index; the distillation sampler of TransE teachers): for each query row i of Q [B, D]
 * fp32 (device, rows ldq >= D floats apart) the k candidates c of cand [n_cand] int64 (device; row ids of X, rows ldx >= D floats
 * apart, duplicates allowed) with the smallest d(i, c) = sum_j (Q[i, j] - X[cand[c], j])^2, computed in this difference form (not
 * |q|^2 + |x|^2 - 2 q.x, which loses the distance under a large common offset).
 *   ids [B, k] int64: the cand VALUES, nearest first; dists [B, k] fp32: their distances.  Equal distances go to the lower position
 *   in cand; a NaN distance comes before every number (NaN rows first, lower position first among them).  When k > n_cand the
 *   trailing slots hold id -1 and distance +inf.  The distances are bit-identical on every shape and route.
 *   1 <= k <= MKB_TOPK_MAX_K, 0 <= B <= 2^31 - 1 (B = 0: nothing), 1 <= n_cand <= 2^31 - 1, D >= 1, ldq >= D, ldx >= D, non-null
 *   pointers, ws of mkb_topk_nearest_workspace_bytes(B, n_cand, k) bytes, 256-byte aligned (0 bytes for B = 0 or a bad argument);
 *   otherwise MKB_ERR_INVALID before any launch.  Every cand value must be a row of X (not checked: device memory).  ABI 7. */
int64_t mkb_topk_nearest_workspace_bytes(int64_t B, int64_t n_cand, int k);
int mkb_topk_nearest(const float *Q, int64_t ldq, const float *X, int64_t ldx, const int64_t *cand, int64_t n_cand, int64_t B,
                     int64_t D, int k, int64_t *ids, float *dists, void *ws, int64_t ws_bytes, void *stream);
/* The same, and the whole distance block the selection ran on handed out as well: block [B, n_cand] fp32 (device, rows n_cand
 * apart; the tests' reference).  Arguments and workspace as above; a null block -> MKB_ERR_INVALID. */
int mkb_topk_nearest_dists(const float *Q, int64_t ldq, const float *X, int64_t ldx, const int64_t *cand, int64_t n_cand, int64_t B,
                           int64_t D, int k, int64_t *ids, float *dists, float *block, void *ws, int64_t ws_bytes, void *stream);

/* ---- grouped evaluation report ---------------------------------------------------------------------------
 * The two reductions behind evaluation.Evaluation.types_relations / detail_eval (evaluation/evaluation.py:282-464).  Neither
 * needs a workspace; n == 0 (or an empty key array) is a valid call that writes zeros; integer atomics and a fixed-order
 * double sum only, so two runs give bit-identical output.  A non-positive table size, a negative count, or a null pointer
 * with a non-zero count -> MKB_ERR_INVALID before any launch.
 *
 * mkb_relation_fanout: what types_relations' two pandas group-bys count.  triples [n, 3] int64: the true triples as given,
 * duplicates included; head_keys [n_head] / tail_keys [n_tail]: the ascending, deduplicated keys of mkb_rank
 * ((t*n_relation + r)*n_entity + h and (h*n_relation + r)*n_entity + t).  counts [n_relation, 3] int64 out, per relation r:
 * the triples with relation r (with multiplicity), the distinct (t, r) pairs (boundaries of key / n_entity in head_keys,
 * bucketed by (key / n_entity) % n_relation), the distinct (h, r) pairs (the same from tail_keys).  A relation id outside
 * [0, n_relation) is not counted. */
int mkb_relation_fanout(const int64_t *triples, int64_t n, const int64_t *head_keys, int64_t n_head, const int64_t *tail_keys,
                        int64_t n_tail, int64_t n_entity, int64_t n_relation, int64_t *counts, void *stream);
/* mkb_rank_metrics: the five running means of compute_detailled_score as sums per group.  ranks [n] int64 (1-based) belong to
 * sample [n, 3]; item i is of group group_of_relation[sample[i][1]] ([n_relation] int32; negative, or >= n_groups: the item is
 * left out).  counts [n_groups, 5] int64 out: items, sum of ranks, ranks <= 1, <= 3, <= 10; rr_sum [n_groups] double out: sum
 * of 1 / rank.  One workgroup per group strides over all n items: meant for a whole test split and n_groups = 4 or n_relation. */
int mkb_rank_metrics(const int64_t *ranks, const int64_t *sample, int64_t n, const int32_t *group_of_relation, int64_t n_relation,
                     int n_groups, int64_t *counts, double *rr_sum, void *stream);

/* ---- triple classification (evaluation/classif.py:89-155: find_threshold, _accuracy) ----------------------
 * mkb_threshold_search: per group, the threshold find_threshold returns: thresholds[argmax(tpr - fpr)] of
 * sklearn.metrics.roc_curve(y, score) with drop_intermediate=True.  score [n] fp32, label [n] int64 (> 0: positive),
 * group [n] int32 or null (null: every item is of group 0; an id < 0 or >= n_groups: the item is of no group).  Among the
 * items of a group with a finite score, write for a score v: tp_ge / fp_ge the positives / negatives with a score >= v,
 * tp_gt / fp_gt those with a score > v, tp_nx / fp_nx those with a score >= the largest score below v.  The distinct score v
 * is a point of the curve when it is the highest or the lowest, or fp_nx - 2 fp_ge + fp_gt != 0, or the same of tp; its value is
 * J = (double)tp_ge / P - (double)fp_ge / N (P, N: the group's positives, negatives), and one more point, threshold +inf with
 * J = 0.0, comes first.  threshold [n_groups] fp32 out: the first point in descending threshold order with the largest J (-0.0
 * and +0.0 are one score: either may be written); +inf for a group with P == 0 or N == 0.  stats [n_groups, 6] int64 out: P, N,
 * tp_ge and fp_ge at the threshold written (0, 0 at +inf), the items of the group whose score is not finite (they take no part
 * and are not in P or N), all items of the group.  An all-pairs count, quadratic in n: n above MKB_THRESHOLD_SEARCH_MAX_N (from
 * where a host sort was measured faster) is refused with MKB_ERR_INVALID.  ws: mkb_threshold_search_workspace_bytes, 4-byte aligned (may be null when n == 0).
 * The selection, like mkb_threshold_accuracy, runs one workgroup per group over all n items (as mkb_rank_metrics does): the cost
 * has a term n_groups * n, meant for a few hundred groups; n_groups * n above 2^32 is refused by both entries. */
#ifndef MKB_THRESHOLD_SEARCH_MAX_N /* a measurement build may raise it: tools/eval_speed.py classif cap */
#define MKB_THRESHOLD_SEARCH_MAX_N 131072
#endif
int64_t mkb_threshold_search_workspace_bytes(int64_t n, int n_groups);
int mkb_threshold_search(const float *score, const int64_t *label, const int32_t *group, int64_t n, int n_groups, float *threshold,
                         int64_t *stats, void *ws, int64_t ws_bytes, void *stream);
/* mkb_threshold_accuracy: _accuracy as counts.  counts [n_groups, 2] int64 out per group: the items with (score >= threshold[g]
 * and label > 0) or (score < threshold[g] and label <= 0), and all items of the group (a NaN score is neither >= nor <: wrong).
 * group as above.  Every output is written, for an empty group and for n == 0 too. */
int mkb_threshold_accuracy(const float *score, const int64_t *label, const int32_t *group, int64_t n, const float *threshold,
                           int n_groups, int64_t *counts, void *stream);

/* ---- relation prediction (h, ?, t): scores, filtered rank, top k -------------------------------------------------
 * The relation-batch side of evaluation.Evaluation.compute_score (evaluation/evaluation.py:217-279) with the candidates and
 * bias of datasets.base.TestDatasetRelation (datasets/base.py:254-305), and the batched "which relation links these two
 * entities" call (mkb_amd/csrc/score_relation.hip).  New symbols under ABI 8: the version is not bumped.
 *   Every score is bit-identical to what mkb_score_fwd writes for the same (h, r, t) in MKB_MODE_DEFAULT on the same tables.
 *   true_keys: the ascending tail-batch keys of mkb_rank, (h*n_relation + r)*n_entity + t; n_true == 0 filters nothing.
 *   Order of the rank and of the top k: NaN first, then higher score, then lower relation id.
 *   mkb_rel_rank: with s the score block of a query and r its relation, v[r'] = s[r] + (-1.0f) where r' != r and (h, r', t) is a
 *   key, v[r'] = s[r'] elsewhere; rank = 1 + the number of r' != r with v[r'] ahead of v[r].  r must lie in [0, n_relation) (not
 *   checked: device memory).
 *   mkb_rel_topk: the k best relations of each query, every r' whose (h, r', t) is a key left out; MKB_TOPK_KEEP_TARGET keeps
 *   sample's own r in (the candidates of the rank) -- without it the relation column is not read.  1 <= k <= MKB_TOPK_MAX_K;
 *   past the candidates left: id -1, score -inf.  scores are the block's bits.
 *   B == 0 is a valid call that launches nothing (ws may then be null); 0 <= B <= 2^31 - 1.  A null pointer, a bad B / n_rel / ld /
 *   k / flags, n_true > 0 without keys, a short or misaligned (256 bytes) workspace, an unknown model -> MKB_ERR_INVALID before any
 *   launch; entity rows too long for the kernel's LDS staging (6 * entity_dim floats > 64 KB) -> MKB_ERR_UNSUPPORTED.  The
 *   workspace functions return 0 for B <= 0 or a bad k.  Nothing is allocated in a call; no float atomics: two runs give the
 *   same bits. */
/* scores[i * ld + j] = score of (h_i, rel_ids ? rel_ids[j] : j, t_i); sample [B, 3], its relation column is not read.
 * rel_ids [n_rel] int64 device, duplicates and any order allowed; null: n_rel must equal tb->n_relation. ld >= n_rel. */
int mkb_rel_scores(const mkb_tables_t *tb, const int64_t *sample, int64_t B, const int64_t *rel_ids, int64_t n_rel,
                   float *scores, int64_t ld, void *stream);

int64_t mkb_rel_rank_workspace_bytes(const mkb_tables_t *tb, int64_t B);
/* filtered rank (1-based) of sample's relation among all n_relation; scores: null, or [B, n_relation] out = the block
 * the ranks were counted on (before the filter), bit-identical to mkb_rel_scores */
int mkb_rel_rank(const mkb_tables_t *tb, const int64_t *sample, int64_t B, const int64_t *true_keys, int64_t n_true,
                 int64_t *rank, float *scores, void *ws, int64_t ws_bytes, void *stream);

int64_t mkb_rel_topk_workspace_bytes(const mkb_tables_t *tb, int64_t B, int k);
int mkb_rel_topk(const mkb_tables_t *tb, const int64_t *sample, int64_t B, const int64_t *true_keys, int64_t n_true,
                 int k, int flags, int64_t *ids, float *scores, void *ws, int64_t ws_bytes, void *stream);

/* ---- candidate lists in any one slot of a triple, differentiable ---------------------------------------------------
 * What distillation.Distillation.distill scores (distillation/distillation.py:82-92): for row i of sample [B, 3] the M triples
 * that replace column `part` of the row by cand[i, 0 .. M) (mkb_amd/csrc/score_cand.hip).  New symbols under ABI 8: the
 * version is not bumped.
 *   mkb_cand_score_fwd: score[i, j] has the bits mkb_score_fwd gives the substituted triple in MKB_MODE_DEFAULT.  The column of
 *   sample that `part` names is not read.  cand [B, M] int64 device: entity ids (head, tail) or relation ids; duplicates and the
 *   row's own ids allowed.  An id outside its table is read (and its gradient added) as the nearest row of the table: the glue
 *   flags it with mkb_check_ids.
 *   mkb_cand_score_bwd: accumulates d loss / d tables given dscore [B, M] into gr (never zeroed; g_modulus for pRotatE).  Head
 *   and relation part: a row pass (one workgroup per row: the two fixed operands' gradients, one atomic per element and row) and
 *   a candidate pass over the B*M pairs radix-sorted by candidate (the varying table's gradient, one atomic per element and run
 *   of equal candidates in a 64-pair chunk).  Tail part: the general two-pass backward of mkb_score_bwd in tail-batch mode.
 *   ws: mkb_cand_score_bwd_workspace_bytes(tb, B, M, part) bytes, 256-byte aligned, caller-owned; nothing is allocated in a call.
 *   0 <= B <= 2^31 - 1, 1 <= M, B * M <= 2^31 - 1; B == 0 is a valid call that launches nothing.  A null pointer, a bad B / M /
 *   part, a short or misaligned workspace, an unknown model -> MKB_ERR_INVALID before any launch; entity rows too long for the LDS
 *   staging ((2 + 4) * entity_dim * 4 > 64 KB) -> MKB_ERR_UNSUPPORTED for every part.  The workspace function returns 0 for
 *   B <= 0, M < 1, a bad part or null tables. */
typedef enum { MKB_PART_HEAD = 0, MKB_PART_RELATION = 1, MKB_PART_TAIL = 2 } mkb_part_t;
int mkb_cand_score_fwd(const mkb_tables_t *tb, const int64_t *sample, const int64_t *cand, int64_t B, int64_t M, int part,
                       float *score, void *stream);
int64_t mkb_cand_score_bwd_workspace_bytes(const mkb_tables_t *tb, int64_t B, int64_t M, int part);
int mkb_cand_score_bwd(const mkb_tables_t *tb, const mkb_grads_t *gr, const int64_t *sample, const int64_t *cand, int64_t B,
                       int64_t M, int part, const float *dscore, void *ws, int64_t ws_bytes, void *stream);

/* ---- embedding regularisers: Lp (p = 2, 3) / N3 on the rows of a batch's positive triples ----------------------------
 * No reference counterpart (a torch expression on gathered rows in user code); mkb_amd/csrc/reg_rows.hip.  New symbols under
 * ABI 8: the version is not bumped (symbols are only added).
 *   reg = sum_i (w_i / W) [lambda_ent (f(E[h_i]) + f(E[t_i])) + lambda_rel f(R[r_i])] over sample [B, 3]; weight [B] or null
 *   (all ones), W = sum of weight (B when null), or weight_sum[0] when given (the rows are a shard, as for the loss calls).
 *   f(x) = sum_k |x_k|^p; for a table whose rows the model reads as [re | im] halves (ComplEx: both tables, RotatE: the entity
 *   table) f(x) = sum_{k < hidden_dim} (re_k^2 + im_k^2)^(p / 2), the N3 of complex models; for p = 2 the two are the same sum.
 *   pRotatE's modulus takes no part.  The gradient of a real entry is p |x|^(p - 1) sign(x), of a pair p m^(p - 2) (re, im) with
 *   m = sqrt(re^2 + im^2): exactly 0 at m = 0.
 *   value [1] out (null: gradient only) = reg; gr (null: value only): scale[0] (device; null = 1) times the gradient of reg is
 *   ADDED to g_ent / g_rel (g_modulus and rows_clear are not used).  A table whose lambda is 0 is neither read nor written (its gradient buffer may be null).
 *   The occurrences of a row collapse into one coefficient: the 3 B occurrences are radix-sorted by row, each distinct row is
 *   read once and its gradient row written by a single workgroup with plain stores; fixed-order sums, no float atomics: two runs
 *   give the same bits in the value and in both gradient tables.  An id outside its table counts as the nearest row.
 *   ws: the workspace function's byte count, 256-byte aligned, caller-owned; nothing is allocated in a call.
 *   B == 0 is a valid call that launches no kernel and writes value = 0 (ws may be null).  p other than 2 or 3, a negative or
 *   non-finite lambda, null tb or sample, value and gr both null, B < 0, B >= 2^30 (the single int32 sort: 3 B and n_entity +
 *   n_relation must stay below 2^31), a short or misaligned workspace, an unknown model -> MKB_ERR_INVALID before any launch.
 *   The workspace function returns 0 for B <= 0, null tables or a B that the call refuses. */
int64_t mkb_reg_rows_workspace_bytes(const mkb_tables_t *tb, int64_t B);
int mkb_reg_rows(const mkb_tables_t *tb, const mkb_grads_t *gr, const int64_t *sample, const float *weight, int64_t B, int p,
                 float lambda_ent, float lambda_rel, const float *weight_sum, const float *scale, float *value, void *ws,
                 int64_t ws_bytes, void *stream);

/* ---- 1vsAll: softmax cross entropy over ALL entities, ComplEx and DistMult ---------------------------------------------
 * No reference counterpart (the reference trains against sampled negatives only); mkb_amd/csrc/score_all.hip.  New symbols under
 * ABI 8: the version is not bumped (symbols are only added).
 *   row_i = log sum_{e < n_entity} exp(s_i(e) / T) - s_i(target_i) / T,   loss = sum_i w_i row_i / W
 *   over sample [B, 3] in MKB_MODE_TAIL (s_i(e) = score of (h_i, r_i, e), target t_i) or MKB_MODE_HEAD ((e, r_i, t_i), target h_i);
 *   weight [B] or null (all ones), W = sum of weight (B when null), or weight_sum[0] when given (the rows are a shard, as for
 *   mkb_ns_loss).  No filtering of other known answers and no label smoothing in these calls: the "filtered 1vsAll" section
 *   below has both.  Only the two models whose all-entity block is one matrix product: TransE, RotatE and pRotatE -> MKB_ERR_UNSUPPORTED (their sampled softmax is mkb_ns_loss with MKB_LOSS_SOFTMAX, their all-entity losses the mkb_dist_all_* calls below).
 *   mkb_all_score_fwd: scores [B, n_entity] out = the all-entity block of the evaluation, the bits mkb_rank_scores hands out (the
 *   same routes, chosen in the same place).
 *   mkb_all_softmax: one pass per row over a block S [B, ld] of which the first N columns count, target[i * target_stride] the
 *   row's target column.  Writes loss [1] and pos [B] (the target's score, read before anything is overwritten) and OVERWRITES S
 *   with dS_ij = (w_i / (W T)) (p_ij - [j = target_i]); columns N .. ld - 1 take no part in the sums and are written as exactly 0.
 *   Stable logsumexp, fixed-order reductions, no float atomics.  scratch: 1 + B floats (device).  A target outside [0, N) counts as
 *   the nearest column: the glue flags it with mkb_check_ids.
 *   mkb_all_score_bwd: accumulates d loss / d tables given dscore [B, ld] (columns past n_entity are not read) into gr->g_ent and
 *   gr->g_rel (never zeroed; g_modulus and rows_clear are not used): dE += dscore^T . Q with every entity row written by exactly one
 *   tile (a K split is reduced in fixed order and the finished product added once), dQ = dscore . E chained into the query's entity
 *   row and relation row with one writer per distinct row.  No float atomics: two runs give the same bits.
 *   mkb_all_step: forward, softmax and backward in one call, the score block staying in the workspace; pos [B] out.
 *   ws: mkb_all_step_workspace_bytes(tb, B) bytes (the same for the three calls that take it), 256-byte aligned, caller-owned;
 *   nothing is allocated in a call.  A null pointer, a mode other than head-/tail-batch, B < 1, T <= 0 or not finite, ld < N,
 *   B * ld (or B * (n_entity + 3)) > 2^31 - 1, a short or misaligned workspace, an unknown model -> MKB_ERR_INVALID before any
 *   launch.  The workspace function returns 0 for B <= 0, null tables, another model or a B that the calls refuse. */
int64_t mkb_all_step_workspace_bytes(const mkb_tables_t *tb, int64_t B);
int mkb_all_score_fwd(const mkb_tables_t *tb, const int64_t *sample, int64_t B, int mode, float *scores, void *ws, int64_t ws_bytes,
                      void *stream);
int mkb_all_softmax(float *S, int64_t B, int64_t N, int64_t ld, const int64_t *target, int64_t target_stride, const float *weight,
                    const float *weight_sum, float T, float *loss, float *pos, float *scratch, void *stream);
int mkb_all_score_bwd(const mkb_tables_t *tb, const mkb_grads_t *gr, const int64_t *sample, int64_t B, int mode, const float *dscore,
                      int64_t ld, void *ws, int64_t ws_bytes, void *stream);
int mkb_all_step(const mkb_tables_t *tb, const mkb_grads_t *gr, const int64_t *sample, const float *weight, int64_t B, int mode,
                 float temperature, const float *weight_sum, float *loss, float *pos, void *ws, int64_t ws_bytes, void *stream);

/* ---- KvsAll: multi-label binary cross entropy over ALL entities, ComplEx and DistMult --------------------------------------
 * The 1-N recipe of ConvE / TuckER and of the reference's losses.BCEWithLogitsLoss, on the 1vsAll step's products;
 * mkb_amd/csrc/score_all.hip.  New symbols under ABI 8: the version is not bumped (symbols are only added).
 *   y_ij = (1 - eps) [j in A_i] + eps / N,   row_i = c sum_{j < N} (softplus(s_ij) - y_ij s_ij),   c = 1 / N or 1 (sum_over_entities),
 *   loss = sum_i w_i row_i / W,   dS_ij = (w_i c / W) (sigmoid(s_ij) - y_ij),   N = n_entity, eps = smoothing
 *   over sample [B, 3] in MKB_MODE_TAIL (query q_i = h_i n_relation + r_i, pos the score of t_i) or MKB_MODE_HEAD (q_i = t_i
 *   n_relation + r_i, pos the score of h_i).  A_i, the labels of row i: keys [n_keys] is the ascending int64 array of the known
 *   triples in the mode's ordering ((h R + r) N + t for tail-batch, (t R + r) N + h for head-batch: the filter arrays of mkb_rank),
 *   the row's labels are its keys in [q_i N, (q_i + 1) N), label column = key - q_i N.  A query without any key is legal (all of
 *   its labels are eps / N), so are two rows with one query; the row's own target need not be a label.  weight, W, weight_sum: as
 *   for the 1vsAll calls.  TransE, RotatE and pRotatE -> MKB_ERR_UNSUPPORTED.
 *   mkb_all_bce: one pass per row over a block S [B, ld] of which the first N columns count.  Writes loss [1] and pos [B] (the
 *   target's score, read before anything is overwritten) and OVERWRITES S with dS; columns N .. ld - 1 take no part in the sums
 *   and are written as exactly 0.  softplus(s) = max(s, 0) + log1p(exp(-|s|)): finite for any finite score.  Fixed-order
 *   reductions, no float atomics.  scratch: 1 + B floats (device).  An id outside its table counts as the nearest row (no label
 *   column leaves the row): the glue flags it with mkb_check_ids.
 *   mkb_all_kvs_step: forward, this loss and the backward of mkb_all_step in one call, the score block staying in the workspace;
 *   pos [B] out; gradients accumulate into gr as for mkb_all_step, two runs give the same bits.
 *   ws: mkb_all_step_workspace_bytes(tb, B) bytes, the 1vsAll step's.  A null pointer (keys may be null only with n_keys == 0),
 *   n_keys < 0, smoothing outside [0, 1) or not finite, a mode other than head-/tail-batch, B < 1, ld < N, the size limits of the
 *   1vsAll calls, (n_entity * n_relation + n_relation) * n_entity past 2^63 - 1, a short or misaligned workspace, an unknown
 *   model -> MKB_ERR_INVALID before any launch. */
int mkb_all_bce(float *S, int64_t B, int64_t N, int64_t ld, const int64_t *sample, int mode, int64_t n_relation, const int64_t *keys,
                int64_t n_keys, const float *weight, const float *weight_sum, float smoothing, int sum_over_entities, float *loss,
                float *pos, float *scratch, void *stream);
int mkb_all_kvs_step(const mkb_tables_t *tb, const mkb_grads_t *gr, const int64_t *sample, const float *weight, int64_t B, int mode,
                     const int64_t *keys, int64_t n_keys, float smoothing, int sum_over_entities, const float *weight_sum, float *loss,
                     float *pos, void *ws, int64_t ws_bytes, void *stream);

/* ---- filtered 1vsAll: the softmax cross entropy without a row's other known answers, with label smoothing ---------------------
 * The 1vsAll step around a third loss kernel; mkb_amd/csrc/score_all.hip.  New symbols under ABI 8: the version is not bumped
 * (symbols are only added).  With A_i the keys of row i's query (the key arrays and ranges of the KvsAll section), t_i its target:
 *   F_i = A_i \ {t_i} (filtered),   C_i = [0, N) \ F_i (kept),   n_i = |C_i| >= 1,   eps = smoothing
 *   y_ij = (1 - eps) [j = t_i] + eps / n_i,   row_i = log sum_{C_i} exp(s_ij / T) - (1 - eps) s_it / T - (eps / n_i) sum_{C_i} s_ij / T,
 *   loss = sum_i w_i row_i / W,   dS_ij = (w_i / (W T)) (p_ij - y_ij) on C_i with p_ij = exp(s_ij / T) / sum_{C_i} exp(s_ik / T),
 *   dS_ij = 0 exactly on F_i.  A filtered column takes no part in anything: not in the maximum, the partition sum, the linear sum or
 *   n_i.  The target is never filtered, whether or not it is a key.  Without keys this is the cross entropy with label smoothing
 *   over the whole row; with eps = 0 as well, the loss of mkb_all_softmax.  A query without keys and two rows with one query are
 *   legal.  weight, W, weight_sum: as for the 1vsAll calls.  TransE, RotatE and pRotatE -> MKB_ERR_UNSUPPORTED.
 *   mkb_all_softmax_filtered: one workgroup per row over a block S [B, ld] of which the first N columns count, target[i *
 *   target_stride] the row's target column, sample [B, 3] and mode naming its query (tail-batch: h_i n_relation + r_i; head-batch:
 *   t_i n_relation + r_i).  The target may differ from the sample's open-slot entity; that entity is then filtered like any other
 *   key.  Writes loss [1] and pos [B] (the target's score, read before anything is overwritten) and OVERWRITES S with dS; columns
 *   N .. ld - 1 take no part in the sums and are written as exactly 0.  Stable logsumexp over the kept columns only, fixed-order
 *   reductions, no float atomics.  scratch: 1 + B floats (device).  An id outside its table counts as the nearest row or column:
 *   the glue flags it with mkb_check_ids.
 *   mkb_all_filtered_step: forward, this loss and the backward of mkb_all_step in one call, the target the sample's open slot;
 *   pos [B] out; gradients accumulate into gr as for mkb_all_step, two runs give the same bits.
 *   ws: mkb_all_step_workspace_bytes(tb, B) bytes, the 1vsAll step's.  A null pointer (keys may be null only with n_keys == 0),
 *   n_keys < 0, T <= 0 or not finite, smoothing outside [0, 1) or not finite, a mode other than head-/tail-batch, B < 1, ld < N,
 *   the size limits of the 1vsAll calls, (n_entity * n_relation + n_relation) * n_entity past 2^63 - 1, a short or misaligned
 *   workspace, an unknown model -> MKB_ERR_INVALID before any launch. */
int mkb_all_softmax_filtered(float *S, int64_t B, int64_t N, int64_t ld, const int64_t *target, int64_t target_stride,
                             const int64_t *sample, int mode, int64_t n_relation, const int64_t *keys, int64_t n_keys,
                             const float *weight, const float *weight_sum, float T, float smoothing, float *loss, float *pos,
                             float *scratch, void *stream);
int mkb_all_filtered_step(const mkb_tables_t *tb, const mkb_grads_t *gr, const int64_t *sample, const float *weight, int64_t B, int mode,
                          const int64_t *keys, int64_t n_keys, float T, float smoothing, const float *weight_sum, float *loss,
                          float *pos, void *ws, int64_t ws_bytes, void *stream);

/* ---- all-entity losses, distance models: 1vsAll, filtered 1vsAll and KvsAll for TransE, RotatE and pRotatE ---------------------
 * The three all-entity losses above for the models whose score is gamma - (modulus) sum_k f(q_i[k], E[e][k]) and whose
 * all-entity block is therefore no matrix product; mkb_amd/csrc/score_all_dist.hip.  New symbols under ABI 9: the version is not
 * bumped (symbols are only added), and the mkb_all_* calls keep refusing these models.  Loss formulas, key arrays, weight, W and
 * weight_sum: those of the three sections above, by the call named beside each.
 *   mkb_dist_all_score_fwd: scores [B, n_entity] out = the all-entity block of the evaluation, finished scores, the bits
 *   mkb_rank_scores hands out (the same routes, chosen in the same place).
 *   mkb_dist_all_score_bwd: accumulates d loss / d tables given dscore [B, ld] (columns past n_entity are not read) into gr->g_ent,
 *   gr->g_rel and, for pRotatE, gr->g_modulus[0] (null: not wanted); never zeroed, rows_clear is not used.  Two passes that recompute
 *   the pair terms: dQ [B, De] = sum_e dscore_ie ds_i(e)/dq (a workgroup owns 16 query rows x 256 units and walks the entities; with
 *   few row tiles the entities are split into up to 8 slices whose partials are added left to right) and dE [n_entity, De] +=
 *   sum_i dscore_ie ds_i(e)/dx (a workgroup owns 16 entity rows x 256 units and walks the batch in order); the modulus gradient is
 *   summed from one partial per workgroup in fixed order; dQ is chained into the query's entity row and relation row with one
 *   writer per distinct row, as in mkb_all_score_bwd.  The derivatives at the edges are those of every other backward here: the
 *   sign of an exactly zero TransE difference is 0, a RotatE pair that coincides gets a gradient of exactly 0.  No float atomics:
 *   two runs give the same bits in every output.  Tables at any alignment, any B >= 1, any n_entity >= 1, entity_dim <= 4096.
 *   The two families share one protocol (mkb_amd/csrc/all_host.h holds it once): each of the six calls below is the mkb_all_* call
 *   of its name (mkb_dist_all_workspace_bytes: mkb_all_step_workspace_bytes) in arguments, checks, their order and their answers,
 *   with this family's models, workspace and backward; the steps run the loss kernel of their call on the finished block.
 *   ws: mkb_dist_all_workspace_bytes(tb, B) bytes (the same for the five calls), 256-byte aligned, caller-owned; nothing is
 *   allocated in a call.  ComplEx and DistMult -> MKB_ERR_UNSUPPORTED (the message names the mkb_all_* calls), and the workspace
 *   function returns 0 for them. */
int64_t mkb_dist_all_workspace_bytes(const mkb_tables_t *tb, int64_t B);
int mkb_dist_all_score_fwd(const mkb_tables_t *tb, const int64_t *sample, int64_t B, int mode, float *scores, void *ws, int64_t ws_bytes,
                           void *stream);
int mkb_dist_all_score_bwd(const mkb_tables_t *tb, const mkb_grads_t *gr, const int64_t *sample, int64_t B, int mode,
                           const float *dscore, int64_t ld, void *ws, int64_t ws_bytes, void *stream);
int mkb_dist_all_step(const mkb_tables_t *tb, const mkb_grads_t *gr, const int64_t *sample, const float *weight, int64_t B, int mode,
                      float temperature, const float *weight_sum, float *loss, float *pos, void *ws, int64_t ws_bytes, void *stream);
int mkb_dist_all_filtered_step(const mkb_tables_t *tb, const mkb_grads_t *gr, const int64_t *sample, const float *weight, int64_t B,
                               int mode, const int64_t *keys, int64_t n_keys, float T, float smoothing, const float *weight_sum,
                               float *loss, float *pos, void *ws, int64_t ws_bytes, void *stream);
int mkb_dist_all_kvs_step(const mkb_tables_t *tb, const mkb_grads_t *gr, const int64_t *sample, const float *weight, int64_t B, int mode,
                          const int64_t *keys, int64_t n_keys, float smoothing, int sum_over_entities, const float *weight_sum,
                          float *loss, float *pos, void *ws, int64_t ws_bytes, void *stream);

/* ---- relation prediction: -log P(r | h, t) over ALL relations as an auxiliary training term ------------------------------------
 * The auxiliary objective of Chen et al. (AKBC 2021), for any of the five models; mkb_amd/csrc/rel_step.hip.  New symbols under
 * ABI 9: the version is not bumped (symbols are only added).
 *   S_ij = score of (h_i, j, t_i) in MKB_MODE_DEFAULT for j < n_relation,   row_i = logsumexp_j (S_ij / T) - S_{i, r_i} / T,
 *   value = lambda sum_i w_i row_i / W,   dS_ij = lambda (w_i / (W T)) (p_ij - [j = r_i])
 *   over sample [B, 3]; weight [B] or null (all ones), W = sum of weight (B when null), or weight_sum[0] when given (the rows are a
 *   shard, as for the loss calls).  No filtering of a pair's other known relations, no label smoothing.
 *   mkb_rel_score_bwd: the backward of the mkb_rel_scores block over all relations: adds d loss / d tables given dscore [B, ld]
 *   (columns past n_relation are not read) to gr->g_ent rows h_i and t_i, to every row of gr->g_rel and, for pRotatE, to
 *   gr->g_modulus[0]; never zeroed, rows_clear is not used.  Two passes that recompute the pair terms: pair-major (a workgroup owns a
 *   sample row and walks the relations; dH[i], dT[i] into the workspace) and relation-major (a workgroup owns 8 relations x 256 units
 *   and walks a slice of the batch in order; the slices' partials are added left to right and the total added to g_rel once); the
 *   2 B occurrences of the batch's entities are radix-sorted and each distinct entity's row has one writer that sums its dH / dT
 *   rows in batch order and adds the sum once; entity rows outside the batch are not written.  No float atomics: two runs give the
 *   same bits.  The derivatives at the edges are those of every other backward here.
 *   mkb_rel_step: forward (the block of mkb_rel_scores in the workspace), the softmax of mkb_all_softmax on it and that backward in
 *   one call.  loss [1] out = value; pos [B] out = S_{i, r_i}, the bits mkb_score_fwd gives sample in MKB_MODE_DEFAULT.  lambda
 *   enters once: it multiplies the softmax's loss, and the backward passes read a seed as lambda dS_ij -- the explicit sequence
 *   (mkb_rel_scores, mkb_all_softmax, lambda times its seeds into mkb_rel_score_bwd) gives the bits of this call.
 *   ws: mkb_rel_step_workspace_bytes(tb, B) bytes (the same for both calls), 256-byte aligned, caller-owned; nothing is allocated
 *   in a call.  B == 0 is a valid call that launches nothing (ws may be null).  A null pointer (weight and weight_sum may be null),
 *   B < 0, T or lambda not finite and > 0, ld < n_relation, B * ld, B * n_relation, 2 * B * entity_dim, n_relation * relation_dim
 *   or n_entity past 2^31 - 1, a short or misaligned workspace, an unknown model -> MKB_ERR_INVALID before any launch; entity rows too
 *   long for the slot kernels' LDS staging -> MKB_ERR_UNSUPPORTED.  The workspace function returns 0 for B <= 0, null tables or a B
 *   that the calls refuse. */
int64_t mkb_rel_step_workspace_bytes(const mkb_tables_t *tb, int64_t B);
int mkb_rel_score_bwd(const mkb_tables_t *tb, const mkb_grads_t *gr, const int64_t *sample, int64_t B, const float *dscore, int64_t ld,
                      void *ws, int64_t ws_bytes, void *stream);
int mkb_rel_step(const mkb_tables_t *tb, const mkb_grads_t *gr, const int64_t *sample, const float *weight, int64_t B, float temperature,
                 float lambda, const float *weight_sum, float *loss, float *pos, void *ws, int64_t ws_bytes, void *stream);

/* ---- per-kernel timing (measurement aid, no reference counterpart) -------------------------------------
 * When enabled, the launches of the named kernel class are bracketed by hipEvents recorded on the SAME stream
 * the kernel is launched on (on = N > 1: every N-th launch only -- the two event records cost ~6 us of stream time
 * each, which a sampled measurement keeps out of most steps).  mkb_profile_read synchronises, returns the number of bracketed launches and
 * their summed duration in milliseconds, and resets the counters.  kernel: 0 = pooled backward (the dq and dx passes
 * in one launch; for ComplEx / DistMult the dQ GEMM),
 * 1 = pooled forward, 2 = the optimizer launches (every mkb_adam_* call and mkb_adagrad_step), 3 = sampler (draw + filter), 4 = adversarial loss, 5 = general forward,
 * 6 = general backward, 7 = pooled backward dx pass when it is launched alone (the GEMM route).  At most 8192 launches are kept between reads.
 */
#define MKB_PROF_POOL_BWD_Q 0
#define MKB_PROF_POOL_FWD 1
#define MKB_PROF_ADAM 2
#define MKB_PROF_SAMPLER 3
#define MKB_PROF_LOSS 4
#define MKB_PROF_GENERAL_FWD 5
#define MKB_PROF_GENERAL_BWD 6
#define MKB_PROF_POOL_BWD_X 7
#define MKB_PROF_KINDS 8
int mkb_profile_enable(int kernel, int on);
/* measurement aid: the shader clock in MHz as one wave sees it over ~20 us (s_memtime cycles per 100 MHz s_memrealtime tick) */
int mkb_debug_sclk_mhz(float *out_mhz_device, void *stream);
int mkb_profile_read(int kernel, int64_t *launches, double *total_ms);

#ifdef __cplusplus
}
#endif
#endif /* MKB_HIP_H */
