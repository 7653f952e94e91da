/*
 * rlvi_hip.h -- C ABI of librlvi_gfx950.so, the MI355X (gfx950 / CDNA4) implementation
 * of the RLVI E-step / M-step hot path.
 *
 * The reference (akarakulev/rlvi) is pure Python; its "FFI" for this path is the set of
 * torch / numpy calls inside the plug-in function
 *     methods.train_rlvi(train_loader, model, optimizer, residuals, weights, overfit, threshold)
 * (deep-learning/methods/train_rlvi.py:52-106, selected by --method=rlvi, main.py:26,277-280)
 * and its two helpers update_sample_weights (:14-38) / false_negative_criterion (:41-49),
 * plus standard-learning/rlvi.py:8-20,68-89 and online-learning/main.py:45-58,84-85.
 * Each entry point below names the reference statements it replaces.  The Python binding
 * a maintainer would add is rlvi_amd/_lib.py (ctypes); see INTEGRATION.md.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer (hipMalloc / torch "cuda" tensor) unless marked host;
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream);
 *   - functions only enqueue work: no allocation, no host synchronisation, graph-capturable;
 *   - return value: 0 = ok, < 0 = argument error (RLVI_E_*), > 0 = hipError_t of the launch;
 *   - scratch comes from a caller-owned workspace (rlvi_workspace_bytes / rlvi_workspace_init).
 *     One workspace must not be used by two streams at the same time.
 *   - device-side status: word 0 of the workspace is a sticky int32 status (0 = ok), bit flags
 *     RLVI_ST_*; out-of-range labels / indexes never touch memory, they set RLVI_ST_RANGE.
 *     The Python plug-in reads it at every epoch end and raises on any flag.
 *   - kernels whose workgroups wait for each other (E-step, threshold) size their grid from the
 *     occupancy query of the current device, so that all of them are resident at once; every wait
 *     is bounded in wall time (RLVI_SPIN_BOUND_MS, default 100) and sets RLVI_ST_TIMEOUT.
 *     The query sees THIS process only: when S processes drive the same GPU, tell each of them
 *     (rlvi_tune_set("RLVI_DEVICE_SHARERS", S), or the environment variable of that name) and every
 *     process takes 1/S of the proven capacity; rlvi_amd.dist does it for the ranks of a process
 *     group by comparing rlvi_device_pci_bus_id() over the ranks.
 */
#ifndef RLVI_HIP_H
#define RLVI_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RLVI_ABI_VERSION 3   /* 3: calls with `out` have records of their own (workspace layout), per-workspace options,
                                 rlvi_tune_unset / _overrides, rlvi_linear_regression_f64, rlvi_sample_weight_online_f64,
                                 rlvi_workspace_region / _reset_warm, rlvi_stream_copy
                                 2: workspace layout of round 2 (peer table, sharded state), rlvi_device_pci_bus_id,
                                 rlvi_estep_sharded_check; set_peers zeroes the local inbox */

#define RLVI_E_NULL   (-1) /* required pointer is NULL                 */
#define RLVI_E_SHAPE  (-2) /* negative / inconsistent size             */
#define RLVI_E_ALIGN  (-3) /* pointer or leading dimension misaligned  */
#define RLVI_E_WS     (-4) /* workspace too small / not initialised    */
#define RLVI_E_LIMIT  (-5) /* size beyond what the kernels support     */

#define RLVI_ST_RANGE   1  /* a label or index was out of range: the row contributes nothing (zero gradient row,
                              no residual written, not counted in loss / top-1)     */
#define RLVI_ST_TIMEOUT 2  /* an inter-workgroup wait hit its bound (the workgroups of a cooperating launch were
                              not all resident, e.g. beside another process's kernels): the launch left its
                              outputs -- pi, threshold -- as they were                */
#define RLVI_ST_NOCONV  4  /* the trajectory E-step did not reach its fixed point (results invalid) */
#define RLVI_ST_SINGULAR 8 /* weighted least squares: rank-deficient design; theta is the minimum-norm
                              solution (what the reference's lstsq returns), NaN for non-finite data */

int rlvi_abi_version(void);
const char *rlvi_error_string(int code);

/* Integer tuning / debug knob (same names as the RLVI_* environment variables, which it
 * overrides); takes effect from the next launch.  Not needed for normal operation. */
int rlvi_tune_set(const char *name, int value);
/* Forget a rlvi_tune_set value (environment variable / built-in default again); 1 if there was one, else 0. */
int rlvi_tune_unset(const char *name);
/* Names of the knobs that carry a rlvi_tune_set value now, comma-separated, into buf[len]; returns their number.
 * The knobs are process-wide: a test harness asserts 0 after every test. */
int rlvi_tune_overrides(char *buf, int len);
/* Compute units of the current device as the launchers see them. */
int rlvi_device_cus(void);
/* PCI bus id ("0000:c1:00.0") of the current device into buf[len >= 16]: the identity of the physical GPU,
 * the same in every process whatever the visible-device masks made of the ordinals. */
int rlvi_device_pci_bus_id(char *buf, int len);

/* Bytes of workspace needed for vectors up to max_n samples and batches up to max_b rows. */
size_t rlvi_workspace_bytes(int64_t max_n, int64_t max_b);
/* Zero the control words.  Call once after allocating (or to clear a sticky status). */
int rlvi_workspace_init(void *ws, size_t ws_bytes, void *stream);
/* Copy the sticky status word to *status_host (synchronises the stream). */
int rlvi_workspace_status(const void *ws, int32_t *status_host, void *stream);
/* Reset the sticky status word to 0 (nothing else: warm-start state and records are kept). */
int rlvi_workspace_clear_status(void *ws, void *stream);
/* What the CALLER of this workspace tells the launchers (host side, per workspace, from the next launch on;
 * rlvi_workspace_init forgets it):
 *   "logits_from_hbm" 1: the [B, C] blocks of the M-step calls on this workspace stream from HBM (larger than the
 *       Infinity Cache, or one of many blocks touched in rotation): a one-tile-per-wave launch then holds its
 *       gradient stores for the read time of the block (mstep.hip); 0 (default): nothing is assumed;
 *   "cold_start" 1: E-step and threshold take no guess from the previous call on this workspace (every call as the
 *       reference's loop starts it, train_rlvi.py:29; the results never depend on the guesses, only the time does).
 * RLVI_E_SHAPE for an unknown name. */
int rlvi_workspace_set_option(void *ws, const char *name, int value);
/* Which form the last M-step launch on this workspace took (tests of the dispatch): 0 none yet, 1 register rows,
 * 2 wave tiles in four-wave workgroups, 3 wave tiles in 16-wave workgroups, 4 word-wise bf16 / fp16 wave tiles (odd row
 * lengths), 5 long rows (more than 512 vectors per row: a wave or a workgroup per row, three passes); + 16 with a timed hold. */
int rlvi_workspace_last_mstep_form(const void *ws);
/* The kernel instantiation behind that form (host side, tests of the dispatch): V | G << 8 | KMAX << 16 -- elements per
 * vector access, lanes per row, vector slots per lane.  G = KMAX = 0 for the long-row form and for the word-wise
 * tile (whose V is 1: single 2-byte elements); 0 for a workspace that has seen no M-step launch. */
int rlvi_workspace_last_mstep_shape(const void *ws);
/* Forget the guesses earlier calls left for the next one (E-step trajectory and minimum, threshold key). */
int rlvi_workspace_reset_warm(void *ws, void *stream);
/* Byte offset (and size through *bytes) of a region of the workspace layout, for tools and tests: "records"
 * (accumulate-mode M-step records), "records_out" (records of calls with `out`), "warm", "scratch"; (size_t)-1
 * for an unknown name. */
size_t rlvi_workspace_region(const char *name, size_t *bytes);

/* ---------------------------------------------------------------------------------------
 * M-step over one mini-batch, forward + backward w.r.t. the logits, lagged pi.
 * Replaces train_rlvi.py:85 (top-1 of accuracy()), :89 (F.cross_entropy reduction='none'),
 * :90 (residuals[indexes] = loss), :92 (weights[indexes]), :93-94 (weighted mean) and the
 * autograd backward of those statements reached from :96.
 *
 *   logits      [B, C] row-major, leading dimension ld (elements)
 *   labels, idx [B] int64;   weights, residuals [N] fp32
 *   inv_scale   1/B for one device; 1/global_B when the batch is sharded over ranks
 *   grad_logits [B, C] (ldg) or NULL for forward only: inv_scale*pi_i*(softmax - onehot)
 *   out         [4] fp32 device: { sum_i pi_i*l_i * inv_scale, 100*hits/B, sum_i pi_i*l_i, hits }
 *               (a row with pi_i == 0 adds nothing to the sums, also when l_i is +inf: the small-loss baselines and
 *                BARE pass their 0/1 selection as the weights)
 * bf16 variant: logits / grad_logits are bfloat16, arithmetic is fp32 on the widened values.
 * Any C up to 2^20 (RLVI_E_LIMIT beyond); rows of more than 512 vectors (C > 2048 fp32 / 4096 bf16 with aligned
 * rows, C > 512 with an odd length or pitch) take a form that reads the row three times (a wave per row, a workgroup
 * per row for batches of up to four rows per CU).
 * The vector width V is the widest of {16 / sizeof(element), 4, 2, 1} that divides C, ld, ldg and the element offsets
 * logits / sizeof(element) and grad_logits / sizeof(element): a dense view whose base is not 16-byte aligned (row 1 of a
 * batch split along its rows) or an odd pitch runs narrower vectors, and leaves the LDS wave tiles for register rows;
 * the results are the same to rounding (rlvi_workspace_last_mstep_shape shows V).
 *
 * Evaluation form: weights == NULL (then idx and residuals must be NULL too) computes the plain
 * mean CE and the top-1 percentage of the batch -- utils.evaluate (deep-learning/utils.py:48-62)
 * without a separate softmax / argmax pass.
 *
 * out == NULL selects ACCUMULATE mode: nothing is finalised; every workgroup adds its partial sums
 * {loss_b, top-1 % of the batch, sum pi*l, hits} to its own record in the workspace (no atomics),
 * so a whole epoch of mini-batches costs one launch each, and rlvi_epoch_end_f32 (or
 * rlvi_mstep_reduce_f32) reduces and clears the records.  A call WITH `out` keeps its records apart
 * (ABI 3) -- it may be interleaved with an accumulate sequence on the same workspace, e.g. an evaluation
 * batch between two training batches -- and is a second (one-workgroup) launch behind the first: +2.6 us
 * in the stream at 65 536 x 100, +1.8 us at 4096 x 10 -- a training loop that needs the batch scalars
 * only at the epoch end wants ACCUMULATE.
 */
int rlvi_mstep_fwd_bwd_f32(const float *logits, int64_t ld, const int64_t *labels,
                           const int64_t *idx, const float *weights, float *residuals,
                           int64_t N, int64_t B, int64_t C, float inv_scale,
                           float *grad_logits, int64_t ldg, float *out, void *ws, void *stream);
int rlvi_mstep_fwd_bwd_bf16(const uint16_t *logits, int64_t ld, const int64_t *labels,
                            const int64_t *idx, const float *weights, float *residuals,
                            int64_t N, int64_t B, int64_t C, float inv_scale,
                            uint16_t *grad_logits, int64_t ldg, float *out, void *ws,
                            void *stream);

/* fp16 variant of the M-step (torch.autocast's default dtype): logits / grad_logits are IEEE binary16 (passed as
 * their 16-bit patterns), arithmetic is fp32 on the exactly widened values.  The same forms as the bf16 entry --
 * evaluation form (weights == NULL), ACCUMULATE mode (out == NULL), strided rows, RLVI_ST_RANGE -- and at every
 * shape the same kernel form as bf16 (same bytes; rlvi_workspace_last_mstep_form shows it).
 *   grad_scale  NULL, or a DEVICE pointer to one fp32 loss scale (torch.amp.GradScaler's scale tensor), read by the
 *               kernel (no host sync per batch): grad_logits = inv_scale * (*grad_scale) * pi_i * (softmax - onehot),
 *               rounded ONCE to fp16 -- nearest even, subnormals kept, +-inf on overflow (what the scaler's inf check
 *               looks for), NaN kept.  The loss, `out`, the residuals and the accumulate-mode records never see the
 *               scale.  4-byte aligned (RLVI_E_ALIGN otherwise).
 */
int rlvi_mstep_fwd_bwd_f16(const uint16_t *logits, int64_t ld, const int64_t *labels, const int64_t *idx,
                           const float *weights, float *residuals, int64_t N, int64_t B, int64_t C,
                           float inv_scale, const float *grad_scale, uint16_t *grad_logits, int64_t ldg,
                           float *out, void *ws, void *stream);

/* out[4] = scale * {sum loss_b, sum top-1 %_b}, sum pi*l, hits over the accumulated batches;
 * clears the records (scale = 1/batches gives the reference's train_acc, train_rlvi.py:105). */
int rlvi_mstep_reduce_f32(float *out, double scale, void *ws, void *stream);

/* ---------------------------------------------------------------------------------------
 * E-step, deep-learning variant, in place on both vectors.
 * Replaces update_sample_weights(residuals, weights, tol, maxiter), train_rlvi.py:14-38:
 * min-shift of the residuals (:27), e = exp(-l) (:28), the fixed point on mean(pi) with the
 * caller's pi entering the first error only (:29-37), and the final pi /= max(pi) (:38).
 *   out_iters  device int32 (may be NULL): iterations executed
 *   trace      device fp32 [2*maxiter] (may be NULL): error then mean-pi of every iteration
 * ------------------------------------------------------------------------------------- */
int rlvi_estep_deep_f32(float *residuals, float *weights, int64_t N, float tol, int maxiter,
                        int32_t *out_iters, float *trace, void *ws, void *stream);

/* ---------------------------------------------------------------------------------------
 * The same E-step with the samples SHARDED over the GPUs of one node (new; the reference is
 * single-device): one process per GPU, this rank holds n_local of the n_all samples.  The
 * per-sample work stays local; only the per-node totals of the trajectory solve (<= 24 nodes x 7
 * fp32 per round) cross the GPUs, written by the kernel's reducer workgroups straight into the other
 * ranks' inboxes over xGMI and summed in rank order, so every rank reaches the same fixed point bit
 * for bit and writes pi / the min-shifted residuals of its own samples.  No collective-library call
 * and no gather of the residual vector on the path.
 *
 *   rlvi_peer_alloc / _export / _open / _close / _free   one 320-KiB inbox per rank in uncached device
 *       memory, exchanged as 64-byte IPC handles by the host program (rlvi_amd.dist.setup_peers)
 *   rlvi_workspace_set_peers(ws, rank, world, inboxes, stream)   inboxes[r] = rank r's inbox as mapped
 *       in this process; call at the same program point on every rank: it resets the round counter and
 *       the sharded warm-start state and ZEROES THE LOCAL INBOX (records of an earlier set-up must not
 *       match the new rounds' tags), so a host-side barrier over the ranks must separate it from the
 *       first sharded call (a peer must not push before this rank's inbox is clean).  After a sharded
 *       call raised RLVI_ST_TIMEOUT the ranks' round counters may differ: set the peers up again (on
 *       every rank) before the next sharded call.
 *   rlvi_estep_sharded_check(n_local, n_all, maxiter, with_out)   0 if rlvi_estep_sharded_f32 would launch
 *       for this shape on this device now, RLVI_E_LIMIT if not; nothing is launched.  The ranks compare
 *       answers before the first collective call.  The sharded solve uses the 256-thread geometry on
 *       every rank (shards may differ in length; the exchanged record layout may not).
 *   rlvi_estep_sharded_f32   a collective: every rank calls it the same number of times; returns
 *       RLVI_E_LIMIT when the shape is outside the trajectory kernel (n_local < 64, ...).
 *       out != NULL: this rank's M-step scalars of the epoch too (as rlvi_epoch_end_f32, x 1/batches).
 *       Waits on a peer are bounded by 100 x the workspace's spin bound (a peer may legitimately be
 *       late); a rank that gives up raises RLVI_ST_TIMEOUT.
 * ------------------------------------------------------------------------------------- */
#define RLVI_PEER_HANDLE_BYTES 64
size_t rlvi_peer_inbox_bytes(void);
int rlvi_peer_alloc(void **inbox);
int rlvi_peer_free(void *inbox);
int rlvi_peer_export(void *inbox, void *handle64);
int rlvi_peer_open(const void *handle64, void **inbox);
int rlvi_peer_close(void *inbox);
int rlvi_peer_can_access(int peer_device);   /* 1 / 0: the current device can map `peer_device`'s memory */
int rlvi_workspace_set_peers(void *ws, int rank, int world, void *const *inboxes, void *stream);
int rlvi_workspace_clear_peers(void *ws, void *stream);   /* before closing / freeing the inboxes */
int rlvi_estep_sharded_check(int64_t n_local, int64_t n_all, int maxiter, int with_out);
int rlvi_estep_sharded_f32(float *residuals, float *weights, int64_t n_local, int64_t n_all,
                           float tol, int maxiter, int64_t batches, float *out, int32_t *out_iters,
                           void *ws, void *stream);
/* The type-II threshold + truncation (train_rlvi.py:41-49,:102-103) on weights sharded the same way:
 * the radix descent's per-bin totals take the same route through the inboxes (exact integers, so
 * bit-exact as on one device); *thr_inout and *kept_out (over ALL ranks) are identical on every rank,
 * the truncation and mask_gt cover this rank's n_local weights.  RLVI_E_LIMIT for n_local <= 1024;
 * a weight outside [0, 1] raises RLVI_ST_NOCONV (the one-device generic form cannot see the others). */
int rlvi_threshold_sharded_check(int64_t n_local, int64_t n_all);   /* 0 / RLVI_E_LIMIT: would the call below launch? */
int rlvi_threshold_truncate_sharded_f32(float *weights, int64_t n_local, int64_t n_all, float alpha,
                                        float *thr_inout, uint8_t *mask_gt, int64_t *kept_out,
                                        void *ws, void *stream);

/* ---------------------------------------------------------------------------------------
 * End of an epoch in one call, replaces train_rlvi.py:99-105: update_sample_weights over all N
 * samples; if `overfit`, *thr_inout = max(*thr_inout, criterion) and the truncation; and, if
 * out != NULL, the epoch's M-step scalars reduced from the accumulate-mode records by an extra
 * workgroup of the same launch: out[1] = mean over `batches` of the per-batch top-1 percentage
 * (= train_acc of :105), out[0] = mean batch loss.
 * ------------------------------------------------------------------------------------- */
int rlvi_epoch_end_f32(float *residuals, float *weights, int64_t N, float tol, int maxiter,
                       int overfit, float alpha, float *thr_inout, int64_t batches, float *out,
                       int32_t *out_iters, void *ws, void *stream);

/* ---------------------------------------------------------------------------------------
 * Type-II-error threshold, replaces false_negative_criterion(weights, alpha),
 * train_rlvi.py:41-49 (sum, sort, cumsum, count, gather) without sorting: the position is
 * found by a radix descent (8 bits per digit, most significant first) on the order-preserving key
 * with exact integer per-bin counts and sums.
 *   thr_out  device fp32: the threshold
 * rlvi_threshold_truncate_f32 additionally applies train_rlvi.py:102-103:
 *   *thr_inout = max(*thr_inout, criterion); weights[weights < *thr_inout] = 0
 * and, if mask_gt != NULL, writes mask_gt[i] = weights[i] > *thr_inout (main.py:343) and
 * kept_out = number of set mask entries (device int64, may be NULL).
 * ------------------------------------------------------------------------------------- */
int rlvi_fn_threshold_f32(const float *weights, int64_t N, float alpha, float *thr_out,
                          void *ws, void *stream);
int rlvi_threshold_truncate_f32(float *weights, int64_t N, float alpha, float *thr_inout,
                                uint8_t *mask_gt, int64_t *kept_out, void *ws, void *stream);
/* Elementwise part alone (threshold already known, on device). */
int rlvi_truncate_f32(float *weights, int64_t N, const float *thr, uint8_t *mask_gt,
                      void *stream);

/* ---------------------------------------------------------------------------------------
 * Small-loss selection (the baselines that share the "per-sample CE -> select -> mean" shape,
 * SURVEY 8(f)-4).  Replaces  ind_sorted = np.argsort(loss.cpu()); ind_update = ind_sorted[:k]
 * (train_usdnl.py:18-24, train_coteaching.py:18-30): mask_w[i] = 1.0f for the k smallest of the n
 * losses, else 0.0f; equal losses are taken in index order (a stable argsort), NaN orders last.
 * The selected rows are then weighted through rlvi_mstep_fwd_bwd_* with weights = mask_w,
 * idx = NULL and inv_scale = 1/k (usdnl) or 1/k^2 (co-teaching's mean followed by /num_remember,
 * train_coteaching.py:32-35).  k <= 0 selects nothing, k >= n everything.
 * ------------------------------------------------------------------------------------- */
int rlvi_select_smallest_f32(const float *loss, int64_t n, int64_t k, float *mask_w, void *stream);

/* ---------------------------------------------------------------------------------------
 * JoCoR's joint loss of two networks, forward and backward.  Replaces loss_jocor(y_1, y_2, t, forget_rate, ind,
 * co_lambda) of deep-learning/methods/train_jocor.py:29-43 -- F.cross_entropy of both blocks (:30-31),
 * kl_loss_compute both ways (:17-26, :33-34), the .cpu() and np.argsort (:34-36), the gather and the mean
 * (:37-42) -- and the backward of all of it into both blocks, reached from loss_1.backward() (:71).
 * As the reference runs it: kl_loss_compute(..., reduce='none') takes its `if reduce:` branch (the string is
 * truthy), so K_qp = mean_b KL(q_b || p_b) and K_pq = mean_b KL(p_b || q_b) are batch means, one scalar each, and
 *     loss_pick_i = ((0.9 CE1_i + 0.9 CE2_i) + lambda K_qp) + lambda K_pq      (fp32, the reference's rounding order;
 *                                                                               0.9 stands for 1 - lambda)
 * with p = softmax(logits1_i), q = softmax(logits2_i).  The k smallest loss_pick are kept (equal values in index
 * order, NaN last; np.argsort's order among equal values is unpinned) and L = their mean; k = 0 gives L = NaN.
 *
 * Forward, two launches (pass 1 over both blocks, then the selection in one workgroup), no host round trip:
 *   logits1, logits2  [B, C] row-major, leading dimensions ld1, ld2 (elements)
 *   labels            [B] int64; a label outside [0, C) sets RLVI_ST_RANGE, its row's cross-entropies are NaN
 *   k                 int((1 - forget_rate) * B) of the caller (:38-39); k >= B keeps every row
 *   co_lambda         lambda (0.1 in the reference)
 *   loss_pick  [B] fp32 out: every row's loss_pick;   sel [B] fp32 out: 1.0 for the kept rows, else 0.0
 *   out        [4] fp32 out: { L, K_qp, K_pq, 100 * (top-1 hits of logits1) / B } (train_jocor.py:58-60)
 *   ws         a workspace (its records of calls with `out`; any size)
 * Backward, one launch: grad1, grad2 [B, C] (ldg1, ldg2; either may be NULL) in the logits' dtype, rounded once:
 *   grad1 = g * ( sel_i (1-lambda)/k (p - e_y) + lambda/B ((p - q) + p (log p - log q - KL(p||q)_i)) )
 *   grad2 = g * ( sel_i (1-lambda)/k (q - e_y) + lambda/B ((q - p) + q (log q - log p - KL(q||p)_i)) )
 * every row, kept or not, receives the KL term; k = 0: both gradients are zero (nothing flows back from a mean of
 * nothing).  g = (*grad_out) * (*grad_scale): DEVICE pointers to one fp32 value each (autograd's upstream gradient,
 * a GradScaler's scale), read by the kernel; NULL stands for 1.  `sel`, `labels`, k and co_lambda must be those of
 * the forward call.
 * bf16 / fp16 entries: the logits and gradients are bfloat16 / IEEE binary16 (16-bit patterns), arithmetic is
 * fp32 on the exactly widened values; the gradients are rounded to nearest even (fp16: subnormals kept, +-inf on
 * overflow).  Any C up to 2^20 (RLVI_E_LIMIT beyond); rows of more than 1024 elements (fewer with an unaligned
 * pitch) take a slower form that sweeps each row from memory.  B < 2^31.
 * ------------------------------------------------------------------------------------- */
int rlvi_jocor_fwd_f32(const float *logits1, int64_t ld1, const float *logits2, int64_t ld2, const int64_t *labels,
                       int64_t B, int64_t C, int64_t k, float co_lambda, float *loss_pick, float *sel, float *out,
                       void *ws, void *stream);
int rlvi_jocor_fwd_bf16(const uint16_t *logits1, int64_t ld1, const uint16_t *logits2, int64_t ld2,
                        const int64_t *labels, int64_t B, int64_t C, int64_t k, float co_lambda, float *loss_pick,
                        float *sel, float *out, void *ws, void *stream);
int rlvi_jocor_fwd_f16(const uint16_t *logits1, int64_t ld1, const uint16_t *logits2, int64_t ld2,
                       const int64_t *labels, int64_t B, int64_t C, int64_t k, float co_lambda, float *loss_pick,
                       float *sel, float *out, void *ws, void *stream);
int rlvi_jocor_bwd_f32(const float *logits1, int64_t ld1, const float *logits2, int64_t ld2, const int64_t *labels,
                       const float *sel, int64_t B, int64_t C, int64_t k, float co_lambda, const float *grad_out,
                       const float *grad_scale, float *grad1, int64_t ldg1, float *grad2, int64_t ldg2, void *stream);
int rlvi_jocor_bwd_bf16(const uint16_t *logits1, int64_t ld1, const uint16_t *logits2, int64_t ld2,
                        const int64_t *labels, const float *sel, int64_t B, int64_t C, int64_t k, float co_lambda,
                        const float *grad_out, const float *grad_scale, uint16_t *grad1, int64_t ldg1,
                        uint16_t *grad2, int64_t ldg2, void *stream);
int rlvi_jocor_bwd_f16(const uint16_t *logits1, int64_t ld1, const uint16_t *logits2, int64_t ld2,
                       const int64_t *labels, const float *sel, int64_t B, int64_t C, int64_t k, float co_lambda,
                       const float *grad_out, const float *grad_scale, uint16_t *grad1, int64_t ldg1,
                       uint16_t *grad2, int64_t ldg2, void *stream);

/* ---------------------------------------------------------------------------------------
 * BARE's batch-statistics pruning, forward.  Replaces WeightedCCE.forward of deep-learning/methods/train_bare.py:28-57
 * -- softmax and clamp (:33-34), the one-hot block and pt_i = p[i, y_i] (:31-35), torch.mean / torch.std down the
 * batch (:38-41), the two matmuls against the one-hot block (:42-43), where / index_select / argmax (:44-51), the
 * second F.cross_entropy (:52-55) -- and the len(prun_idx) host sync (:50); and, through out[3], the top-1 of
 * accuracy(logits, labels) that train_bare takes beside it (:72).
 *     p = clamp(softmax(z), 1e-8, 1 - 1e-8);  mu_c = mean_i p[i, c];  sd_c = unbiased deviation of p[:, c] (B - 1)
 *     row i is kept when  p[i, y_i] - mu[y_i] >= k * sd[y_i]          (fp32, the reference's rounding order)
 *     L = mean over the kept rows of CE(z_i, y_i); no row kept (always for B = 1, where sd is NaN): the fallback,
 *     L = mean over all rows.
 *   logits  [B, C] row-major, leading dimension ld (elements); fp32, bf16 or fp16 (16-bit patterns), arithmetic in
 *           fp32 on the exactly widened values
 *   labels  [B] int64; a label outside [0, C) sets RLVI_ST_RANGE, its row is never kept and adds nothing to L
 *   k       BARE's k (train_bare uses 1); NaN is RLVI_E_SHAPE
 *   w    [B] fp32 out: 1 / n_kept on the kept rows, else 0; 1 / B on every row in the fallback
 *   sel  [B] fp32 out: 1.0 on the kept rows, else 0.0; all ones in the fallback
 *   out  [4] fp32 out: { L, n_kept (B in the fallback), fallback (0 / 1), 100 * top-1 hits / B }
 *   grad [B, C] (ldg) in the logits' dtype or NULL: written by the one-workgroup form only (see below)
 *   ws   a workspace of any size (the slabs of the column sums take its weighted-least-squares region)
 * No gradient flows through the statistics: dL/dz_i = w_i (softmax(z_i) - e_y).  Two forms (rlvi_bare_form tells
 * which one a shape takes: 1 / 0, or RLVI_E_SHAPE / RLVI_E_LIMIT; knob RLVI_BARE_FORM: -1 by size, 0 streaming,
 * 1 one workgroup wherever the block fits it):
 *   one workgroup, B * C <= 16 384 with B <= 1024 and C <= 1024 (the reference's batches, 32 x 10 to 128 x 100):
 *       statistics, selection, L and -- if grad != NULL -- the gradient w_i (softmax - e_y), rounded once, in ONE launch;
 *   streaming, everything else: two launches (pass 1 over the block, then one finishing workgroup), no host round
 *       trip; `grad` is left alone: the gradient is rlvi_mstep_fwd_bwd_* with weights = w, idx = NULL, inv_scale = 1
 *       (an upstream gradient or a loss scale goes in as its grad_scale, or multiplies the B values of w).
 * Both forms give the same sel, bit for bit, and every run gives the same bits: the column sums are exact fixed-point
 * integers (p, p^2 in units of 2^-40), the deviation is taken from them without a rounded subtraction.
 * C <= 4096 and B <= 2^22 (RLVI_E_LIMIT beyond).  Rows may be strided.
 * ------------------------------------------------------------------------------------- */
int rlvi_bare_form(int64_t B, int64_t C);
int rlvi_bare_fwd_f32(const float *logits, int64_t ld, const int64_t *labels, int64_t B, int64_t C, float k, float *w,
                      float *sel, float *out, float *grad, int64_t ldg, void *ws, void *stream);
int rlvi_bare_fwd_bf16(const uint16_t *logits, int64_t ld, const int64_t *labels, int64_t B, int64_t C, float k,
                       float *w, float *sel, float *out, uint16_t *grad, int64_t ldg, void *ws, void *stream);
int rlvi_bare_fwd_f16(const uint16_t *logits, int64_t ld, const int64_t *labels, int64_t B, int64_t C, float k,
                      float *w, float *sel, float *out, uint16_t *grad, int64_t ldg, void *ws, void *stream);

/* ---------------------------------------------------------------------------------------
 * CDR's gradient masking over all weight tensors of a network.  Replaces deep-learning/methods/train_cdr.py:22-44:
 * the torch.cat of every covered gradient and parameter (:22-29), metric = |g * v| (:30), torch.topk(metric, nz)
 * read for its last value (:33-34) and, per tensor, mask = (|v * g| >= thresh) * clip; g = mask * g (:40-44) --
 * without a concatenated copy and without a sort: the nz-th largest metric is found to the bit by a radix descent
 * (11 + 10 + 10 bits) on the metric's bit pattern, over a table of segments, one per tensor.  The result equals the
 * reference's bit for bit (fp32 products commute, `>=` keeps every tie); a NaN metric orders above +inf.
 *
 *   rlvi_cdr_table_bytes(nseg)    bytes of the segment table (host copy and device copy alike); 0 for nseg < 1
 *   rlvi_cdr_table_fill           HOST only, touches no device (train_cdr.py:24-27, the walk over the parameters):
 *       writes the table of segments {v[i], g[i], n[i], first chunk} into host_buf (8-byte aligned,
 *       rlvi_cdr_table_bytes(nseg) bytes); v[i] / g[i] are DEVICE pointers to n[i] contiguous fp32 values, 4-byte
 *       alignment is enough.  *total = sum n[i] (:31), *chunks = the fixed-size pieces of work all segments make.
 *       The caller uploads host_buf to 16-byte-aligned device memory, so that the launch below never copies.
 *       RLVI_E_NULL for a null pointer (an entry of v / g included), RLVI_E_SHAPE for nseg < 1 or an n[i] < 1,
 *       RLVI_E_ALIGN for a v[i] / g[i] that is not 4-byte aligned.
 *   rlvi_cdr_scratch_bytes(nseg)  bytes of device scratch for the histograms and the state of the descent
 *       (16-byte aligned, any contents; apart from the workspace, whose layout it leaves alone)
 *   rlvi_cdr_mask_f32             (train_cdr.py:30-44) five launches whatever nseg is:
 *       table_dev  the uploaded table;  nseg, total, chunks  as rlvi_cdr_table_fill gave them
 *       nz         int(nonzero_ratio * total) of the caller (:32), 1 <= nz <= total (the reference raises an
 *                  IndexError for nz == 0: the caller's to raise)
 *       clip       the scale of the kept gradients (:43)
 *       thr_out    device fp32: the nz-th largest |g * v| (:34)
 *       kept_out   device int64: entries with |g * v| >= *thr_out (>= nz; more when values tie at the threshold)
 *       every g[i] is overwritten with m * g[i], m = clip where |g[i] * v[i]| >= *thr_out, else 0.0f -- as that
 *       multiplication: a dropped entry keeps its sign on its zero, a dropped infinite gradient becomes NaN.
 *       RLVI_E_NULL / RLVI_E_SHAPE (nseg < 1, nz < 1, nz > total, chunks outside [nseg, total]) / RLVI_E_ALIGN (table
 *       or scratch not 16-byte aligned, thr_out, kept_out) / RLVI_E_WS (scratch_bytes too small) / RLVI_E_LIMIT
 *       (total >= 2^32), all before any launch.
 * ------------------------------------------------------------------------------------- */
size_t rlvi_cdr_table_bytes(int nseg);
int rlvi_cdr_table_fill(void *host_buf, const void *const *v, void *const *g, const int64_t *n, int nseg,
                        int64_t *total, int64_t *chunks);
size_t rlvi_cdr_scratch_bytes(int nseg);
int rlvi_cdr_mask_f32(const void *table_dev, int nseg, int64_t total, int64_t chunks, int64_t nz, float clip,
                      void *scratch, size_t scratch_bytes, float *thr_out, int64_t *kept_out, void *stream);

/* ---------------------------------------------------------------------------------------
 * precision@k.  Replaces accuracy(logit, target, topk) of deep-learning/utils.py:65-79 (softmax :67, torch.topk
 * :70, eq :72, the per-k counts :76-77): hits[j] = number of rows whose label is among the ks[j]
 * largest logits of its row, j < nk <= 8.  train_rlvi keeps only precision@1 (train_rlvi.py:85), which the
 * M-step kernel delivers on the side; this is the stand-alone form.  One pass, no softmax, no sort: the label's
 * rank is the count of columns ahead of it; equal values rank in column order (torch.topk's order among equal
 * values, and logits that differ but whose fp32 softmax values coincide, are implementation details of the
 * reference: unpinned).  A label outside [0, C) is never a hit (:72).
 *   ks     HOST array of nk values, each in [1, C] (RLVI_E_SHAPE beyond: torch.topk raises there)
 *   hits   DEVICE int32 [nk], zeroed by the call; precision@k = 100 * hits / B
 * ------------------------------------------------------------------------------------- */
int rlvi_topk_hits_f32(const float *logits, int64_t ld, const int64_t *labels, int64_t B, int64_t C,
                       const int32_t *ks, int nk, int32_t *hits, void *stream);
int rlvi_topk_hits_bf16(const uint16_t *logits, int64_t ld, const int64_t *labels, int64_t B, int64_t C,
                        const int32_t *ks, int nk, int32_t *hits, void *stream);
/* fp16 logits (16-bit patterns of IEEE binary16): the rank count on the exactly widened values, so the hits equal
 * rlvi_topk_hits_f32 on the same logits converted to fp32. */
int rlvi_topk_hits_f16(const uint16_t *logits, int64_t ld, const int64_t *labels, int64_t B, int64_t C,
                       const int32_t *ks, int nk, int32_t *hits, void *stream);

/* ---------------------------------------------------------------------------------------
 * In-batch fused E+M (online order, online-learning/main.py:296-299 applied to a logit block):
 * per-sample NLL -> E-step on THIS batch (deep variant, pi_in only feeds the first error)
 * -> weighted loss and gradient with the NEW pi.  Composition of a1, a7, a4, a5 -- as ONE launch for fp32 dense
 * rows (fused_em.hip), tried in this order on a 256-CU device:
 *   C <= 16 (the ten classes of MNIST / CIFAR-10), 64 <= B <= 65 536: a row per thread;
 *   4 | C, 16 < C <= 128, 64 <= B <= 16 384: four lanes per row, the rows in registers;
 *   4 | C, 32 <= C <= 128, 16 | B, 16 385 <= B <= 65 536 (and 16 129 <= B <= 16 384 when the form above is refused
 *   for lack of co-resident workgroups): the logit block resident in the chip's LDS between the two passes --
 *   bit-identical to the composition where the E-step slices coincide (B > 65 280), a few ulp elsewhere.
 * The two register forms: pi, loss rows and gradient within 1e-5 of the composition, same iteration count.
 * Everything else (bf16, 4 does not divide C > 16, more than 65 536 rows, strided rows): three launches.
 *   loss_rows [B] receives the min-shifted NLL, pi [B] the new posteriors (in/out).
 * ------------------------------------------------------------------------------------- */
int rlvi_fused_em_f32(const float *logits, int64_t ld, const int64_t *labels, float *loss_rows,
                      float *pi, int64_t B, int64_t C, float inv_scale, float tol, int maxiter,
                      float *grad_logits, int64_t ldg, float *out, int32_t *out_iters,
                      void *ws, void *stream);

/* ---------------------------------------------------------------------------------------
 * fp64 E-steps of the numpy paths.
 *   rlvi_update_weights_f64        standard-learning/rlvi.py:8-20   (update_weights)
 *   rlvi_update_weights_online_f64 online-learning/main.py:45-58    (update_weights_rlvi)
 * ------------------------------------------------------------------------------------- */
int rlvi_update_weights_f64(const double *losses, int64_t n, double tol, int maxiter,
                            double *out, int32_t *out_iters, void *ws, void *stream);
int rlvi_update_weights_online_f64(const double *losses, int64_t n, double tol, int maxiter,
                                   double *out, int32_t *out_iters, void *ws, void *stream);

/* ---------------------------------------------------------------------------------------
 * Per-sample NLL of the linear / logistic paths: the X.theta / X.w contraction on the fp64 matrix
 * cores (v_mfma_f64_16x16x4_f64, 16 rows per wave; n*d is 15-20 k elements: launch-latency-bound).
 *   rlvi_linreg_losses_f64  rlvi.py:72-74 / :81-83: r=(y-X theta)^2, sigma2=w.r/sum(w),
 *                           losses=0.5 r/sigma2;  sigma2_out device fp64
 *   rlvi_logistic_nll_f64   online-learning/main.py:295-296,:84-85: -log sigmoid(X w + b)
 * X is row-major [n, d].
 * ------------------------------------------------------------------------------------- */
/* Weighted least squares theta = argmin sum_i w_i (y_i - x_i.theta)^2, the M-step of
 * linear_regression (standard-learning/rlvi.py:70-71,:79-80, scipy lstsq on diag(sqrt(w))-scaled
 * rows there): [X | y]^T W [X | y] on the fp64 matrix cores (v_mfma_f64_16x16x4_f64), Cholesky +
 * triangular solves in one workgroup; a rank-deficient design sets RLVI_ST_SINGULAR and gets the
 * minimum-norm solution (Jacobi eigen-decomposition of the Gram matrix), as lstsq gives.  d <= 63.
 * Rank-deficient means: a column within ~1e-7 (relative) of the span of the columns before it -- the
 * pivot is compared with the column's own diagonal entry of the Gram matrix, so the SCALE of a column
 * (1e-60 or 1e9 beside unit columns) never reads as rank deficiency, here and in
 * rlvi_linear_regression_f64 below.  Accuracy goes as kappa^2 eps, kappa the condition number of
 * sqrt(W) X with unit-length columns: centre columns that sit far from the origin. */
int rlvi_wls_solve_f64(const double *X, const double *y, const double *w, int64_t n, int64_t d,
                       double *theta, void *ws, void *stream);
int rlvi_linreg_losses_f64(const double *X, const double *y, const double *theta,
                           const double *w, int64_t n, int64_t d, double *losses,
                           double *sigma2_out, void *ws, void *stream);
int rlvi_logistic_nll_f64(const double *X, const double *w, double b, int64_t n, int64_t d,
                          double *losses, void *stream);

/* ---------------------------------------------------------------------------------------
 * The whole estimator linear_regression(X, y, maxiter=100, tol=1e-3) of standard-learning/rlvi.py:68-89 as ONE
 * launch (standard.hip): weights = 1, weighted least squares (:70-71), Gaussian NLL (:72-74), then up to `maxiter`
 * times { update_weights(losses) with (estep_tol, estep_maxiter) = the reference's (1e-3, 100) (:77 -> :8-20),
 * weighted least squares (:79-80), NLL (:81-83), stop when ||theta - prev|| / ||prev|| <= tol (:85-87) } -- the
 * stop decision is taken on the device, the host waits once, for the result.  One persistent workgroup: the
 * weighted Gram matrix and X.theta on the fp64 matrix cores, an L D L^T solve on one wave.
 *   theta [d], weights [n] (the final pi), info int32[4] = { outer iterations, inner iterations of the last
 *   E-step, inner iterations in all, fallback } -- all device pointers.
 * n <= 4096 and d <= 31 (rlvi_linear_regression_check says 0 / RLVI_E_LIMIT without launching).  info[3] == 1: a
 * pivot of the normal equations was not safely positive (rank-deficient design, non-finite data); theta / weights
 * are then NOT written and the caller composes rlvi_wls_solve_f64 (minimum-norm solution, as the reference's
 * lstsq returns) / rlvi_linreg_losses_f64 / rlvi_update_weights_f64 itself, as for shapes beyond the limit.
 * ------------------------------------------------------------------------------------- */
int rlvi_linear_regression_check(int64_t n, int64_t d);
int rlvi_linear_regression_f64(const double *X, const double *y, int64_t n, int64_t d, int maxiter, double tol,
                               double estep_tol, int estep_maxiter, double *theta, double *weights,
                               int32_t *info, void *ws, void *stream);

/* ---------------------------------------------------------------------------------------
 * The whole estimator logistic_regression(X, y, maxiter=100, tol=1e-2) of standard-learning/rlvi.py:92-108 as ONE
 * launch (logreg.hip): weights = 1, fit, losses (:93-94), then up to `maxiter` times { update_weights(losses) with
 * (estep_tol, estep_maxiter) = the reference's (1e-3, 100) (:98 -> :8-20), fit, losses (:101), stop when
 * ||theta - prev|| / ||prev|| <= tol (:104-106) } -- decided on the device, the host waits once.
 *   The fit replaces utils.sklearn_log_reg (standard-learning/utils.py:61-73: liblinear, L2, primal, C = 1e2, the
 *   bias regularised, the weights divided by their maximum).  It returns the unique minimiser of
 *       f(v) = 1/2 v.v + C sum_i (w_i / max w) log(1 + exp(-s_i z_i)),  v = (coef, bias), z = X coef + bias, s = 2y - 1,
 *   which liblinear approximates to its tol = 1e-4: damped Newton from v = 0 (Hessian I + Z^T diag(.) Z as a weighted
 *   Gram matrix of [X | 1] on the fp64 matrix cores, L D L^T on one wave, Armijo halving), until
 *   ||g|| <= 1e-12 ||g(0)|| or a full step no longer lowers f; at most 50 Newton steps per fit.
 *   The losses are the reference's own (utils.py:62-64): -log p(class 0 | x) = log(1 + exp(z)) for EVERY sample.
 *   X [n, d] row-major, y [n] of 0.0 / 1.0; C > 0 (the reference: 1e2).
 *   theta [d + 1] = (intercept, coef ...) as utils.py:69, weights [n] (the final pi), losses [n] (of the last fit; may
 *   be NULL), info int32[4] = { outer iterations, inner iterations of the last E-step, Newton steps in all, flag } --
 *   all device pointers.  flag 1: data that is not finite, a y that is neither 0 nor 1, weights without a positive
 *   one, or a pivot that is not safely positive -- theta / weights / losses are then NOT written.  flag 2: a fit took
 *   its 50 Newton steps without meeting the stop test, or its 40 Armijo halvings found no acceptable step away from
 *   the rounding floor; RLVI_ST_NOCONV is raised in the workspace, the results are those of the last accepted step.
 * LIMITS: n <= 4096 (one workgroup, 16 samples per thread) and d <= 30 ([X | 1] and the gradient's column fill two
 * 16-column blocks); rlvi_logistic_regression_check says 0 / RLVI_E_LIMIT (RLVI_E_SHAPE for n or d <= 0) without
 * launching.
 * rlvi_logistic_fit_f64: ONE fit and its losses for the caller's weights w [n] (>= 0, one of them > 0) -- the
 * M-step on its own (utils.py:61-73), the same device code; info = { 0, 0, Newton steps, flag }.
 * ------------------------------------------------------------------------------------- */
int rlvi_logistic_regression_check(int64_t n, int64_t d);
int rlvi_logistic_regression_f64(const double *X, const double *y, int64_t n, int64_t d, int maxiter, double tol,
                                 double estep_tol, int estep_maxiter, double C, double *theta, double *weights,
                                 double *losses, int32_t *info, void *ws, void *stream);
int rlvi_logistic_fit_f64(const double *X, const double *y, const double *w, int64_t n, int64_t d, double C,
                          double *theta, double *losses, int32_t *info, void *ws, void *stream);

/* ---------------------------------------------------------------------------------------
 * The estimators mean, pca and covariance of standard-learning/rlvi.py as ONE launch each (moments.hip), and the
 * constrained E-step on its own.  One persistent workgroup; the sample [n, d] row-major is staged into LDS once;
 * weighted moments in two passes (sums, then the second moment about the mean just found), fp64 in a fixed order:
 * the same inputs give the same bits.  Every stop decision is taken on the device, the host waits once.
 *   mean        rlvi.py:46-65: weights = 1, theta = sum w x / sum w, r = ||theta - x||^2, sigma2 = sum w r / sum w,
 *               losses = 1/2 r / sigma2 (:47-51), then up to `maxiter` times { update_weights(losses) with
 *               (estep_tol, estep_maxiter) = the reference's (1e-3, 100) (:54 -> :8-20), theta and losses again
 *               (:56-59), stop when ||theta - prev|| / ||prev|| <= tol (:61-63) }.  theta [d].
 *   pca         rlvi.py:111-125 with utils.py:76-89: the fit is the first principal component of the rows w x
 *               (centred by their plain column mean; the eigenvector of the largest eigenvalue of their d x d scatter
 *               matrix by cyclic Jacobi sweeps, at most 30; normalised; the component of largest magnitude -- the
 *               first on a tie -- positive, which is sklearn's svd_flip), losses = ||x||^2 - (x.theta)^2 on the
 *               uncentred rows.  theta_init [d] or NULL: replaces the FIRST fit and is used as is, not normalised
 *               (utils.py:81-88).  d = 1 gives theta = [1].  An exactly repeated largest eigenvalue leaves the
 *               direction unpinned.  theta [d].
 *   covariance  rlvi.py:128-144 with utils.py:92-108: mu = sum w x / sum w, C = sum w (x - mu)(x - mu)^T / sum w,
 *               losses = 1/2 ((x - mu)^T C^-1 (x - mu) + log det C + d log 2 pi) by an L D L^T factorisation; the
 *               E-step is update_weights_constrained (below) with n_eff (the reference: n (1 - eps));
 *               Frobenius norms in the stop test.  theta [d * d] row-major.  Requires 0 < n_eff < n.
 *   rlvi_update_weights_constrained_f64   rlvi.py:23-43: update_weights(losses, tol, maxiter) first; if its weights
 *               sum to less than n_eff, out_i = 1 / (1 + c exp(l_i - s)), c = (n - n_eff) / n_eff, with the shift s
 *               at which they sum to n_eff -- the exact root (safeguarded Newton on the bracket [min l, max l],
 *               at most 200 evaluations) of what the reference hands to scipy's minimize_scalar as a square: the
 *               contract is the root, not Brent's iterate.  n <= 4096.
 *               info = { root-find evaluations, the fixed point's iterations, 1 if the constraint was active, flag }.
 * weights [n] (the final pi), info int32[4] = { outer iterations, inner iterations of the last E-step, count, flag },
 * count = mean: inner iterations in all; pca: Jacobi sweeps in all; covariance: E-steps in which the constraint was
 * active -- all device pointers.  flag 1: data that is not finite, no positive weight, a variance or a pivot that is
 * not safely positive, n_eff outside (0, n): NOTHING is written.  flag 2: the Jacobi cap or the root-find cap was
 * hit; RLVI_ST_NOCONV is raised in the workspace and the last iterate is returned.
 * LIMITS: 2 <= n <= 4096, 1 <= d <= 8 and n d <= 16 384 (the sample resident in 128 KB of LDS); rlvi_moments_check
 * says 0 / RLVI_E_LIMIT (RLVI_E_SHAPE for n or d <= 0) without launching.
 * ------------------------------------------------------------------------------------- */
int rlvi_moments_check(int64_t n, int64_t d);
int rlvi_robust_mean_f64(const double *sample, int64_t n, int64_t d, int maxiter, double tol, double estep_tol,
                         int estep_maxiter, double *theta, double *weights, int32_t *info, void *ws, void *stream);
int rlvi_robust_pca_f64(const double *sample, int64_t n, int64_t d, int maxiter, double tol,
                        const double *theta_init, double estep_tol, int estep_maxiter, double *theta,
                        double *weights, int32_t *info, void *ws, void *stream);
int rlvi_robust_covariance_f64(const double *sample, int64_t n, int64_t d, double n_eff, int maxiter, double tol,
                               double estep_tol, int estep_maxiter, double *theta, double *weights, int32_t *info,
                               void *ws, void *stream);
int rlvi_update_weights_constrained_f64(const double *losses, int64_t n, double n_eff, double tol, int maxiter,
                                        double *out, int32_t *info, void *ws, void *stream);

/* ---------------------------------------------------------------------------------------
 * A Monte-Carlo sweep in ONE launch: `batch` independent problems of one shape, one workgroup each (the kernels above
 * on a grid of `batch` workgroups; nothing waits for another workgroup, no cooperative launch).  The reference's
 * experiments are such loops (standard-learning/main.py):
 *   rlvi_linear_regression_batch_f64     main.py:261-273   20 corruption levels x 100 runs of 40 x 10
 *   rlvi_logistic_regression_batch_f64   main.py:431-437   100 runs of 200 x 2
 *   rlvi_robust_mean_batch_f64           main.py:180-188   20 x 100 runs of 100 x 2
 *   rlvi_robust_pca_batch_f64            main.py:489-494   100 runs of 40 x 2, one theta_init for all
 *   rlvi_robust_covariance_batch_f64     main.py:539-544   100 runs of 50 x 2, one eps for all
 * The single entry's argument list with `batch` in front of n, the arrays contiguous with the problem as the slowest
 * index: X / sample [batch, n, d], y [batch, n], theta [batch, nt] (nt = d; d + 1 logistic; d * d covariance), weights
 * [batch, n], losses [batch, n] (logistic; may be NULL), info int32[batch, 4].  theta_init [d] (or NULL) and n_eff are
 * shared by the whole batch.
 *   Problem b gets EXACTLY the theta, weights and info the single entry gives for it alone: the same kernel template,
 *   thread count, sums and dispatch by (n, d).  info[4 b + 3] is problem b's flag, with the single entry's meaning
 *   (linear regression 1: the caller takes the general path for THAT problem; its rows of theta / weights are not
 *   written).  RLVI_ST_NOCONV in the workspace is raised if ANY problem ends with flag 2.
 * Validation is the single entry's, and batch <= 0 is RLVI_E_SHAPE, batch > 1 048 576 RLVI_E_LIMIT.  Graph-capturable
 * as the single entries are.  A slice of a batch is 8-byte aligned, which is all the kernels ask of their fp64 arrays.
 * ------------------------------------------------------------------------------------- */
int rlvi_linear_regression_batch_f64(const double *X, const double *y, int64_t batch, int64_t n, int64_t d,
                                     int maxiter, double tol, double estep_tol, int estep_maxiter, double *theta,
                                     double *weights, int32_t *info, void *ws, void *stream);
int rlvi_logistic_regression_batch_f64(const double *X, const double *y, int64_t batch, int64_t n, int64_t d,
                                       int maxiter, double tol, double estep_tol, int estep_maxiter, double C,
                                       double *theta, double *weights, double *losses, int32_t *info, void *ws,
                                       void *stream);
int rlvi_robust_mean_batch_f64(const double *sample, int64_t batch, int64_t n, int64_t d, int maxiter, double tol,
                               double estep_tol, int estep_maxiter, double *theta, double *weights, int32_t *info,
                               void *ws, void *stream);
int rlvi_robust_pca_batch_f64(const double *sample, int64_t batch, int64_t n, int64_t d, int maxiter, double tol,
                              const double *theta_init, double estep_tol, int estep_maxiter, double *theta,
                              double *weights, int32_t *info, void *ws, void *stream);
int rlvi_robust_covariance_batch_f64(const double *sample, int64_t batch, int64_t n, int64_t d, double n_eff,
                                     int maxiter, double tol, double estep_tol, int estep_maxiter, double *theta,
                                     double *weights, int32_t *info, void *ws, void *stream);

/* ---------------------------------------------------------------------------------------
 * Robust Risk Minimization (standard-learning/rrm.py, Osama et al. 2020), the competitor the reference's experiments
 * fit on the same sample (main.py:184, :222, :492, :542): mean, pca and covariance as ONE launch each, their batch forms
 * and the weight rule on its own (moments.hip).  The kernels, fits, limits and flags of the rlvi_robust_* entries
 * above; what differs:
 *   rlvi_rrm_update_weights_f64   rrm.py:12-33: out_i = exp(-l_i / alpha) / sum_j exp(-l_j / alpha) at the alpha that
 *               minimises alpha (log sum_i exp(-l_i / alpha) - log((1 - eps) n)).  The reference hands that to scipy's
 *               minimize_scalar over xi = log alpha; here xi is the exact root of the stationarity condition
 *               "entropy of out = log((1 - eps) n)" (a bracket grown geometrically, then safeguarded Newton, at most
 *               200 evaluations): the contract is the root, not Brent's iterate.  The losses are shifted by their
 *               minimum (out does not change, nothing overflows) and the reference's floor of 1e-16 under every
 *               exponential is dropped.  If the samples tied at the minimum, m of them, are (1 - eps) n or more there is
 *               no root: out = 1 / m on them and 0 elsewhere, the limit alpha -> 0.  n <= 4096.
 *               info = { evaluations, 0, 1 if there was a root, flag }.
 *   rlvi_rrm_mean_f64         rrm.py:36-52: weights = 1 / n, theta = sum w x / sum w, losses = ||theta - x||^2 (no
 *               variance), then up to `maxiter` times { update_weights(losses, eps), theta and losses again, stop when
 *               ||theta - prev|| / ||prev|| <= tol }.
 *   rlvi_rrm_pca_f64          rrm.py:94-107 with utils.py:76-89: the fit and the losses of rlvi_robust_pca_f64.
 *   rlvi_rrm_covariance_f64   rrm.py:110-124 with utils.py:92-108: the fit and the losses of rlvi_robust_covariance_f64.
 *   rlvi_rrm_*_batch_f64      the loops of main.py:180-188, :489-494, :539-544 around them: `batch` in front of n, the
 *               arrays as for rlvi_robust_*_batch_f64, one eps (and theta_init) for all problems; problem b gets
 *               exactly the bits of the single entry.
 * eps takes the place of n_eff; there is no estep_tol / estep_maxiter.  info int32[4] = { outer iterations,
 * evaluations of the last root-find, count, flag }, count = mean, covariance: evaluations in all; pca: Jacobi sweeps in
 * all.  flag 1, NOTHING written: eps outside (0, 1), (1 - eps) n <= 1, a sample or a loss that is not finite, and
 * what the fits flag.  flag 2: the root-find cap or the Jacobi cap (RLVI_ST_NOCONV in the workspace).
 * ------------------------------------------------------------------------------------- */
int rlvi_rrm_mean_f64(const double *sample, int64_t n, int64_t d, double eps, int maxiter, double tol, double *theta,
                      double *weights, int32_t *info, void *ws, void *stream);
int rlvi_rrm_pca_f64(const double *sample, int64_t n, int64_t d, double eps, int maxiter, double tol,
                     const double *theta_init, double *theta, double *weights, int32_t *info, void *ws, void *stream);
int rlvi_rrm_covariance_f64(const double *sample, int64_t n, int64_t d, double eps, int maxiter, double tol,
                            double *theta, double *weights, int32_t *info, void *ws, void *stream);
int rlvi_rrm_mean_batch_f64(const double *sample, int64_t batch, int64_t n, int64_t d, double eps, int maxiter,
                            double tol, double *theta, double *weights, int32_t *info, void *ws, void *stream);
int rlvi_rrm_pca_batch_f64(const double *sample, int64_t batch, int64_t n, int64_t d, double eps, int maxiter,
                           double tol, const double *theta_init, double *theta, double *weights, int32_t *info,
                           void *ws, void *stream);
int rlvi_rrm_covariance_batch_f64(const double *sample, int64_t batch, int64_t n, int64_t d, double eps, int maxiter,
                                  double tol, double *theta, double *weights, int32_t *info, void *ws, void *stream);
int rlvi_rrm_update_weights_f64(const double *losses, int64_t n, double eps, double *out, int32_t *info, void *ws,
                                void *stream);

/* ---------------------------------------------------------------------------------------
 * The robust linear regressions the reference plots beside RLVI's (standard-learning/main.py:248-357) that are
 * iterations around a least-squares solve, as ONE launch each (robust_linreg.hip): the workgroup, the weighted
 * least-squares fit, the limits (n <= 4096, d <= 31), the argument checks and the batch convention of
 * rlvi_linear_regression_f64 / _batch_f64 above.  X [n, d], y [n] row-major fp64; batch forms: X [B, n, d], y [B, n],
 * every output with B rows, info int32[B, 4], problem b with exactly the bits of the single entry.
 *
 *   rlvi_rrm_linear_regression_f64      standard-learning/rrm.py:55-73: weights = 1 / n, theta = the weighted
 *               least-squares fit, losses = (y - X theta)^2; then up to `maxiter` times { update_weights(losses, eps)
 *               -- the exact root of rlvi_rrm_update_weights_f64 --, theta and losses again, stop when ||theta - prev|| /
 *               ||prev|| <= tol }.  maxiter = 0: the first fit.  theta [d], weights [n].
 *               info = { outer iterations, evaluations of the last root-find, evaluations in all, flag }.
 *               flag 1, nothing written: a pivot of a fit's normal equations is not safely positive (the scale-free test
 *               of rlvi_linear_regression_f64; weights that underflow to exactly 0 can cause it mid-loop) -- the
 *               reference's lstsq returns the minimum-norm solution there, compose rlvi_rrm_update_weights_f64 and
 *               rlvi_wls_solve_f64 instead.  flag 2, nothing written: a loss is not finite.  flag 3: a root-find hit its
 *               200 evaluations (RLVI_ST_NOCONV in the workspace; the results are written).
 *               eps outside (0, 1) or (1 - eps) n <= 1: RLVI_E_SHAPE.
 *   rlvi_rrm_linear_regression_batch_f64    the sweep of main.py:261-273 around rrm.linear_regression (:269).
 *
 *   rlvi_huber_linear_regression_f64    standard-learning/huber.py:13-40: theta0 = (X^T X)^-1 X^T y with X^T X formed
 *               and factored ONCE; then { r = y - X theta0, r_psi = r clipped at c sigma0 (:23), sigma = ||r_psi|| /
 *               sqrt(2 n alpha) (:25), r_psi = r clipped at c sigma (:27), theta = theta0 + (X^T X)^-1 X^T r_psi
 *               (:30-32); while ||theta - theta0|| / ||theta0|| > 1e-6: sigma0 = sigma, theta0 = theta }.  The reference's
 *               `while True` is capped at `maxiter` iterations (its default here: 1000); maxiter = 0: theta0, sigma0.
 *               alpha = rlvi_huber_alpha(c).  theta [d], scale [1] (the last sigma).
 *               info = { iterations, 0, 0, flag }.  flag 1, nothing written: X^T X has a pivot that is not safely
 *               positive (numpy.linalg.solve raises at huber.py:17).  flag 2, nothing written: a scale that is not
 *               positive and finite (an exactly interpolating fit: sigma = 0) or a theta that is not finite.  flag 3:
 *               the iteration still moved when the cap was reached (RLVI_ST_NOCONV; the last iterate is written).
 *               c <= 0 or sigma0 <= 0: RLVI_E_SHAPE.
 *   rlvi_huber_linear_regression_batch_f64  the sweep of main.py:261-273 around huber.linear_regression (:266);
 *               scale [B].
 *   rlvi_huber_alpha    huber.py:15, c^2 (1 - F1(c^2)) + F3(c^2) with the chi-square distribution functions in closed
 *               form: F1(c^2) = erf(c / sqrt 2), F3(c^2) = F1(c^2) - sqrt(2 / pi) c exp(-c^2 / 2).  Host only.
 * Return codes: RLVI_E_NULL, RLVI_E_SHAPE (batch, n, d <= 0, maxiter < 0, the parameters above), RLVI_E_LIMIT (n > 4096,
 * d > 31, batch > 1 048 576), RLVI_E_ALIGN, in this order.  Graph-capturable; no host synchronisation.
 * ------------------------------------------------------------------------------------- */
double rlvi_huber_alpha(double c);
int rlvi_rrm_linear_regression_f64(const double *X, const double *y, int64_t n, int64_t d, double eps, int maxiter,
                                   double tol, double *theta, double *weights, int32_t *info, void *ws, void *stream);
int rlvi_rrm_linear_regression_batch_f64(const double *X, const double *y, int64_t batch, int64_t n, int64_t d,
                                         double eps, int maxiter, double tol, double *theta, double *weights,
                                         int32_t *info, void *ws, void *stream);
int rlvi_huber_linear_regression_f64(const double *X, const double *y, int64_t n, int64_t d, double c, double sigma0,
                                     int maxiter, double *theta, double *scale, int32_t *info, void *ws, void *stream);
int rlvi_huber_linear_regression_batch_f64(const double *X, const double *y, int64_t batch, int64_t n, int64_t d,
                                           double c, double sigma0, int maxiter, double *theta, double *scale,
                                           int32_t *info, void *ws, void *stream);

/* ---------------------------------------------------------------------------------------
 * RRM's logistic regression, the third curve of the reference's logistic comparison (standard-learning/main.py:
 * 361-470), as ONE launch (robust_logreg.hip): the workgroup, the fit, the limits (n <= 4096, 1 <= d <= 30) and the
 * batch convention of rlvi_logistic_regression_f64 / _batch_f64 above, the weight rule of rlvi_rrm_update_weights_f64.
 *
 *   rlvi_rrm_logistic_regression_f64    standard-learning/rrm.py:76-91 on utils.py:61-73: weights = 1 / n, (theta,
 *               losses) = the fit (:77-78); then up to `maxiter` times { update_weights(losses, eps) (:81) -- the exact
 *               entropy root --, the fit with C weights / max weights (:84, utils.py:66), stop when ||theta - prev|| /
 *               ||prev|| <= tol (:87-89; a zero ||prev|| gives NaN and no stop, as there) }.  Reaching maxiter is silent,
 *               as in the reference; maxiter = 0: the bits of rlvi_logistic_fit_f64 with unit weights.  The losses are
 *               log(1 + exp(z)) for EVERY sample (utils.py:62-64).  X [n, d] row-major, y [n] of 0.0 / 1.0, C > 0 (the
 *               reference: 1e2).  theta [d + 1] = (intercept, coef ...), weights [n] (the last rule's output: they sum
 *               to 1; 1 / n with maxiter = 0), info int32[4] = { outer iterations, evaluations of the last root-find,
 *               Newton steps in all, flag }.
 *               flag 1, nothing written: a label that is neither 0 nor 1, or a value that is not finite.  flag 2: a fit
 *               ended at its 50 Newton steps or without an acceptable Armijo step.  flag 3: a root-find hit its 200
 *               evaluations.  For 2 and 3 RLVI_ST_NOCONV is raised in the workspace and the results are written.
 *   rlvi_rrm_logistic_regression_batch_f64    the sweep of main.py:372-401 around rrm.logistic_regression (:382): X [B, n, d],
 *               y [B, n], theta [B, d + 1], weights [B, n], info int32[B, 4]; problem b has the bits of the single entry.
 * Return codes: RLVI_E_NULL, RLVI_E_SHAPE (batch, n, d <= 0, maxiter < 0, C <= 0, eps outside (0, 1) or
 * (1 - eps) n <= 1), RLVI_E_LIMIT (n > 4096, d > 30, batch > 1 048 576), RLVI_E_ALIGN, in this order.
 * Graph-capturable; no host synchronisation.
 * ------------------------------------------------------------------------------------- */
int rlvi_rrm_logistic_regression_f64(const double *X, const double *y, int64_t n, int64_t d, double eps, int maxiter,
                                     double tol, double C, double *theta, double *weights, int32_t *info, void *ws,
                                     void *stream);
int rlvi_rrm_logistic_regression_batch_f64(const double *X, const double *y, int64_t batch, int64_t n, int64_t d,
                                           double eps, int maxiter, double tol, double C, double *theta,
                                           double *weights, int32_t *info, void *ws, void *stream);

/* ---------------------------------------------------------------------------------------
 * One mini-batch of the online path in ONE launch, replaces online-learning/main.py:293-297:
 *   log_proba = log(0.5) for the first batch (first != 0; X, w may be NULL), else clf.predict_log_proba(X)[:, 1]
 *   = log sigmoid(X w + b) (:295, X.w on the fp64 matrix cores); residuals = -log_proba (:296 with :84-85: the
 *   target does not enter); sample_weight = update_weights_rlvi(residuals, tol, maxiter) (:297 -> :45-58).
 *   losses_out [n] (may be NULL) receives the residuals, out_iters (may be NULL) the iterations.  n <= 4096.
 * ------------------------------------------------------------------------------------- */
int rlvi_sample_weight_online_f64(const double *X, const double *w, double b, int first, int64_t n, int64_t d,
                                  double tol, int maxiter, double *losses_out, double *sample_weight,
                                  int32_t *out_iters, void *stream);

/* ---------------------------------------------------------------------------------------
 * The online path's whole mini-batch in ONE launch (online_sgd.hip), replaces online-learning/
 * main.py:291-313 and :318-331 for one classifier: residuals -> sample weights -> clf.partial_fit(X, y, classes=[0, 1],
 * sample_weight=...) -> the four counts of clf.predict(X_test) against y_test.
 *   partial_fit is ONE pass of scikit-learn's _plain_sgd with the reference's settings (SGDClassifier(loss='log_loss',
 *   random_state=1): L2 penalty alpha, learning rate 'optimal', an intercept, one epoch, no averaging) over the rows in
 *   `order` (int32 [n], what scikit-learn's shuffle makes of the identity: it depends on n alone and the host computes
 *   it; NULL: natural order).  state [d + 2] = (coef [d], intercept, t) is read (unless first != 0: the unfitted
 *   classifier, coef 0, intercept 0, t 1) and updated in place; t grows by one per sample.
 *   method 0: unit weights (main.py:313); 1: update_weights_rlvi (:45-58, tol, maxiter) and 2: update_weights_rrm(eps)
 *   (:61-81, as the exact root: rlvi_rrm_update_weights_f64's rule) of the residuals -log sigmoid(X coef + intercept)
 *   -- log 2 for every row when first != 0 (:293); 3: the weights in sample_weight.
 *   X [n, d], y [n] in {0, 1} (as fp64; 1 is the positive class), Xt [m, d], yt [m] (m may be 0, then they may be NULL).
 *   sample_weight [n]: receives the weights (methods 0 .. 2; may be NULL there), is read by method 3.
 *   counts int32[4] = (tp, tn, fp, fn) of main.py:320-331 with the prediction `decision value > 0` and the NEW state.
 *   info int32[4] = { E-step iterations (method 1) or root-find evaluations (2), 1 if RRM's rule had a root, samples
 *   whose update was not zero, flag }; flag 1: a coefficient or the intercept is not finite (scikit-learn raises
 *   ValueError; the state is written as it is); 2: no weights -- a residual not finite, or (1 - eps) n <= 1: no pass,
 *   the state as it was; 3: the root-find hit its 200 evaluations (results written); 4: an index of `order` outside
 *   [0, n) (or, stream form, a row count outside its padding): nothing is read through it, no pass.
 *   1 <= n <= 4096, 0 <= m <= 4096, 1 <= d <= 128 (RLVI_E_LIMIT beyond); alpha > 0, 0 < eps < 1 for method 2.
 *
 * rlvi_online_stream_f64: T consecutive mini-batches for S <= 8 classifiers in ONE launch (main.py:288-339, the whole
 * loop of main()), one workgroup per classifier, all reading the same data; every classifier starts unfitted.
 *   X [T, n, d], y [T, n], Xt [T, m, d], yt [T, m] padded to the largest batch; rows int32 [T, 2] = (n_t, m_t), the
 *   real row counts (NULL: n and m everywhere; rows beyond them are never read); orders int32 [T, n] (NULL: natural).
 *   methods (HOST, int32 [S]) and eps (HOST, fp64 [S]; may be NULL without a method 2).
 *   state_hist [S, T, d + 2] (the state after every batch), counts int32 [S, T, 4], weights [S, T, n] (may be NULL
 *   without a method 3; a method 3 reads its weights there, the others write theirs), info int32 [S, T, 4].
 *   Every (classifier, batch) has the bits of the same sequence of rlvi_online_step_f64 calls.
 * ------------------------------------------------------------------------------------- */
int rlvi_online_step_f64(const double *X, const double *y, const int32_t *order, int64_t n, int64_t d, int method,
                         double eps, int first, double *state, const double *Xt, const double *yt, int64_t m,
                         double alpha, double tol, int maxiter, double *sample_weight, int32_t *counts,
                         int32_t *info, void *stream);
int rlvi_online_stream_f64(const double *X, const double *y, const double *Xt, const double *yt, const int32_t *rows,
                           const int32_t *orders, int64_t T, int64_t n, int64_t m, int64_t d, const int32_t *methods,
                           const double *eps, int64_t S, double alpha, double tol, int maxiter, double *state_hist,
                           int32_t *counts, double *weights, int32_t *info, void *stream);

/* Measurement aid (bench.py: roofline.copy_same_bytes_us): flat copy, 16 B per lane, nontemporal loads and stores,
 * 16 waves per CU -- the plainest kernel that moves the M-step's bytes.  16-byte aligned, bytes a multiple of 16. */
int rlvi_stream_copy(void *dst, const void *src, size_t bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* RLVI_HIP_H */
