/*
 * sea_hip.h - C ABI of libsea_hip.so: the MI355X (gfx950) attack-side hot path of
 * SEA (Segmentation Ensemble Attack) evaluation and the PIR-AT inner PGD loop.
 *
 * The reference (nmndeep/Robust-Segmentation) is 100 % Python: it has no FFI, its "interface" for
 * this path is the ATen op sequences inside semseg/attacker.py, semseg/val.py, semseg/metrics.py
 * and tools/worse_only.py.  Every entry point below replaces one such sequence and cites it
 * (paths relative to the reference repo root).  INTEGRATION.md shows the ctypes binding a
 * maintainer of the reference would add.
 *
 * Conventions
 *   - plain pointers + sizes, no torch types; all device pointers are HBM addresses on the
 *     current HIP device; the caller allocates and owns every buffer; the library keeps no mutable
 *     state and never allocates, frees or synchronises -> re-entrant per stream, graph-capturable.
 *     Which kernel runs is a function of the call's arguments alone (plus the two read-only words of
 *     sea_process_config); defaults and environment variables are the caller's business.
 *   - `stream` is a hipStream_t passed as void* (NULL = the legacy default stream).  All device
 *     work is stream ordered and asynchronous.
 *   - return value: 0 on success, otherwise a hipError_t value (1 = invalid argument).  Nothing
 *     throws across the ABI.
 *   - tensors are dense, NCHW ("planes") unless a layout argument says otherwise.
 *   - labels: any of int64 / int32 / int16 / uint8 (y_bytes = 8/4/2/1); the ignore label is -1
 *     (255 for uint8).  Labels outside [0,C) are treated as ignored.
 *   - loss modes: 0 mask-ce-avg, 1 mask-ce-bal, 2 js-avg, 3 ce / ce-avg.
 *   - logits dtype: 0 float32, 1 bfloat16, 2 float16 (dlogits has the same dtype and layout).
 */
#ifndef SEA_HIP_H
#define SEA_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SEA_MODE_MASK_CE 0
#define SEA_MODE_MASK_CE_BAL 1
#define SEA_MODE_JS 2
#define SEA_MODE_CE 3

#define SEA_DTYPE_F32 0
#define SEA_DTYPE_BF16 1
#define SEA_DTYPE_F16 2

#define SEA_LAYOUT_NCHW 0
#define SEA_LAYOUT_NHWC 1

/* library / build identification */
int sea_abi_version(void);   /* 3: kernel variants are arguments (sea_gemm_split*, sea_dwconv7x7_nhwc*, ...), no setters;
                              *    one replayable form of K1 / K7 (radius and run length in device memory) */
const char* sea_build_info(void);
/* The process configuration: two A/B switches that dozens of launchers consult, read from the environment ONCE at first use
 * and immutable afterwards; every other choice is an argument of the call it concerns.  Read-only; -1 for an unknown word.
 *   SEA_CONFIG_XCD_ORDER         env SEA_XCD_ORDER = 0 | 1 | 2: XCD-aware block order off / on (default) / also for pure streams
 *   SEA_CONFIG_UPSAMPLE_GENERAL  env SEA_UPSAMPLE_GENERAL = 1: general-ratio bilinear kernels even for power-of-two factors */
#define SEA_CONFIG_XCD_ORDER 0
#define SEA_CONFIG_UPSAMPLE_GENERAL 1
int sea_process_config(int which);
/* host only: the multiplier / shift the kernels use to divide a work index (< 2^31) by d without an integer division:
 * n / d == (mulhi32(n, *m) + n) >> *s.  Exposed for the unit test of that arithmetic. */
int sea_fastdiv_magic(uint32_t d, uint32_t* m, uint32_t* s);

/* ------------------------------------------------------------------------------------------------
 * K1  APGD L-inf step with momentum.            replaces semseg/attacker.py:389-410, 456
 *   g2 = x_adv - x_old ; z = x_adv + step[b]*sign(grad) ; z = clip(clip(z, x-eps, x+eps), 0, 1)
 *   z = x_adv + (z - x_adv)*a + g2*(1-a)        ; out = clip(clip(z, x-eps, x+eps), 0, 1)
 * Bit-exact w.r.t. the float32 op sequence of the reference.  `out` must not alias an input.
 * n_per_img = 3*H*W elements per image; step_b has B entries.
 */
int sea_apgd_linf_step(const float* x, const float* x_adv, const float* x_old, const float* grad,
                       const float* step_b, float eps, float a, float* out, int B,
                       int64_t n_per_img, void* stream);

/* K5a random start: out = clip(x + eps*(2u-1), 0, 1).          semseg/attacker.py:293-294, 308 */
/* K1' -- the L2 branch of apgd_train (semseg/attacker.py:412-436; per-image norm = autoattack.other_utils.L2_norm, attacker.py:6):
 * normalised gradient step, projection onto the eps-ball (L2) around x and [0, 1], momentum combination, projection again.
 * Four streaming passes that recompute the element-wise chain; the three per-image norms are sums of per-block partials in a
 * fixed order (double), no atomics.  workspace: sea_apgd_l2_workspace_bytes(B) bytes, 8-byte aligned.  No shipped entry point
 * of the reference reaches this branch: it completes the drop-in surface. */
int64_t sea_apgd_l2_workspace_bytes(int B);
int sea_apgd_l2_step(const float* x, const float* x_adv, const float* x_old, const float* grad, const float* step_b, float eps,
                     float a, float* out, void* workspace, int B, int64_t n_per_img, void* stream);
int sea_linf_random_start(const float* x, const float* u, float eps, float* out, int64_t n,
                          void* stream);
/* K5b stage re-projection: out = clip(x + clip(z-x,-eps,eps), 0, 1). semseg/attacker.py:683-690 */
int sea_linf_project(const float* z, const float* x, float eps, float* out, int64_t n,
                     void* stream);

/* K6  PIR-AT PGD step on the perturbation.                      semseg/val.py:209-214 (168-172)
 *   d = delta + alpha*sign(grad) ; d = clip(X+d,0,1) - X ; delta_out = clip(d,-eps,eps)
 * If x_in_out != NULL it also receives the next model input: X+delta_out (clamp_input=0,
 * Pgd_Attack_1, val.py:200) or clip(X+delta_out,0,1) (clamp_input=1, Pgd_Attack val.py:150 and the
 * final x_adv of both, val.py:177, 217).  delta_out may alias delta. */
int sea_pgd_linf_step(const float* X, const float* delta, const float* grad, float alpha,
                      float eps, float* delta_out, float* x_in_out, int clamp_input, int64_t n,
                      void* stream);

/* ------------------------------------------------------------------------------------------------
 * K2  fused per-pixel loss forward + logit gradient + tracking loss + accuracy + argmax.
 * replaces  masked_cross_entropy / _balanced / js_loss (semseg/attacker.py:143-173, 187-234),
 *           pixel_to_img_loss (237-240), the autograd of lines 347-350 / 462-469 down to the logits,
 *           the tracking loss (359-361, 473-475) and accuracy / argmax (370-373, 485-495);
 *           also the val.py losses (semseg/val.py:104-127) through `mode` + `grad_scale`.
 *
 *   logits   (B,C,H,W) [layout 0] or (B,H,W,C) [layout 1], dtype per `dtype`
 *   y        (B,H,W) labels, y_bytes wide
 *   w        (C) float32 class weights, required for mode/track_mode 1, else may be NULL
 *   grad_scale  upstream gradient per valid pixel (1/(H*W) for the per-image mean of the reference)
 *   dlogits  same shape/dtype/layout as logits, or NULL to skip the gradient (last APGD step,
 *            attacker.py:467, and clean/adversarial evaluation)
 *   pred     (B,H,W) argmax map (first maximum wins), pred_bytes wide (8/4/2/1) or NULL
 *   loss_px  (B,H,W) float32 per-pixel attack loss (reduction="none" of the reference functions) or NULL
 *   workspace  sea_loss_workspace_bytes(B,HW) bytes of scratch
 *   loss_sum / track_sum (B) float32: SUM over the image's pixels of the attack / tracking loss
 *            (the caller divides by H*W; attacker.py:240 divides by all pixels incl. ignored)
 *   n_correct (B) int32: #valid pixels with argmax == label
 *   Passing loss_sum = track_sum = n_correct = NULL defers the second reduction stage: the per-block
 *   records stay in `workspace` and sea_apgd_track (K7) sums them itself (`loss_workspace` argument), which
 *   saves one launch per APGD iteration.
 * Reductions are two-stage with a fixed order (no float atomics): results are run-to-run
 * deterministic.
 */
size_t sea_loss_workspace_bytes(int B, int64_t HW);
int sea_loss_fwd_bwd(const void* logits, int dtype, int layout, const void* y, int y_bytes,
                     const float* w, int mode, int track_mode, int B, int C, int64_t HW,
                     float grad_scale, void* dlogits, void* pred, int pred_bytes, float* loss_px,
                     void* workspace, size_t workspace_bytes, float* loss_sum, float* track_sum,
                     int32_t* n_correct, void* stream);
/* The same with a variant word that pins the kernel (tests, A/B runs); 0 = sea_loss_fwd_bwd.  Fields:
 *   SEA_K2_VEC_MASK      bits 0-3: pixels per lane of the register kernel, 1 | 2 | 4 (0 = the widest that H*W and the pointers'
 *                        alignment allow); a non-zero value also keeps the streaming and the split kernel out.
 *   SEA_K2_TUNE_SHIFT    bits 4-7: TUNE of the register kernel (1 = non-temporal gradient stores, 2 = non-temporal logit loads,
 *                        4 = 4 waves/SIMD).  Three fp32 cells have one: 7 at C = 21 with gradient, 6 at C = 21 without, 2 at
 *                        C = 151 with gradient, each the default of a word whose low 12 bits are 0; 15 = none.  Ignored elsewhere.
 *   SEA_K2_STREAM_SHIFT  bits 8-11: 1..4 = the streaming no-gradient kernel at any C, with (classes per chunk, waves/SIMD) =
 *                        (4, 5), (8, 3), (6, 4), (2, 8).  SEA_K2_NO_SPLIT (15 in this field): not the split kernel (gradient
 *                        at C = 150 / 151), the register kernel instead.
 *   SEA_K2_REG_ONLY      bit 12: neither the streaming nor the split kernel.
 * A word whose field names nothing (other bits, a TUNE without instantiation, a streaming variant where the split kernel would
 * run) is an invalid argument. */
#define SEA_K2_VARIANT_DEFAULT 0u
#define SEA_K2_VEC_MASK 0xfu
#define SEA_K2_TUNE_SHIFT 4
#define SEA_K2_STREAM_SHIFT 8
#define SEA_K2_NO_SPLIT (15u << SEA_K2_STREAM_SHIFT)
#define SEA_K2_REG_ONLY 0x1000u
int sea_loss_fwd_bwd_tuned(const void* logits, int dtype, int layout, const void* y, int y_bytes,
                           const float* w, int mode, int track_mode, int B, int C, int64_t HW,
                           float grad_scale, void* dlogits, void* pred, int pred_bytes, float* loss_px,
                           void* workspace, size_t workspace_bytes, float* loss_sum, float* track_sum,
                           int32_t* n_correct, void* stream, int variant);
/* host only, touches no device: the kernel a call with these arguments runs (csrc/loss_plan.h).  Only the alignment of the two
 * addresses matters; dlogits_addr is read when want_grad != 0.  Returns what the call would return for them (0, or 1 for a
 * shape or word without kernel) and fills out = {kernel, cpad, exact, vec, tune, ch, waves, tiles}: kernel 0 = register
 * (cpad class registers, vec pixels per lane, exact: C == cpad), 1 = two-pass (C > 192), 2 = streaming no-gradient (ch classes
 * per chunk), 3 = split, 4 = channels_last; waves = waves/SIMD asked of the compiler where the kernel has the knob; tiles =
 * blocks, and workspace records, per image. */
int sea_loss_plan(int dtype, int layout, int C, int64_t HW, int want_grad, size_t logits_addr, size_t dlogits_addr,
                  unsigned variant, int32_t out[8]);

/* K2u  K2 fused with the model's final bilinear upsample.
 * replaces  F.interpolate(logits, size=(H,W), mode="bilinear", align_corners=False)
 *           (semseg/models/uperforseg.py:416-418, semseg/models/segmenter.py:228) + everything K2 replaces
 *           + the interpolate backward: the (B,C,H,W) logits and their gradient are never materialised.
 *   low   (B,C,h,w) float32 NCHW low-resolution logits;  dlow same shape (or NULL: no gradient)
 *   y     (B,H,W) labels; pred (B,H,W) argmax map at full resolution (or NULL)
 *   loss_sum / track_sum / n_correct as in K2 (sums over the H*W full-resolution pixels)
 * Any scale H/h, W/w >= 1 (ATen's align_corners=False source-index rule).  Gradients are gathered in a
 * fixed order (no atomics): deterministic.
 * pow2 != 0 (shipped): factors 4 and 16 take the kernel with lanes along the classes; pow2 = 0 keeps the general gather
 * kernel for every factor (A/B).  Pass the same value to both calls: it sizes the workspace.
 */
size_t sea_loss_upsampled_workspace_bytes(int B, int C, int h, int w, int H, int W, int pow2);
int sea_loss_fwd_bwd_upsampled(const float* low, const void* y, int y_bytes, const float* w, int mode,
                               int track_mode, int B, int C, int h, int wl, int H, int W, float grad_scale,
                               float* dlow, void* pred, int pred_bytes, void* workspace,
                               size_t workspace_bytes, float* loss_sum, float* track_sum,
                               int32_t* n_correct, int pow2, void* stream);

/* ------------------------------------------------------------------------------------------------
 * K3  per-class integer statistics.
 * sea_class_counts replaces compute_iou_acc's loops (semseg/attacker.py:14-45), eval_performance
 * (tools/infer.py:90-116) and update_fn / update_fn_indiv (tools/worse_only.py:30-66).
 *   inter[c] += #{pred==y==c}; tgt_cnt[c] += #{y==c}; pred_cnt[c] += #{pred==c}
 *   mask_pred=1: pixels with ignored label do not count in pred_cnt (attacker.py:20, infer.py:90);
 *   mask_pred=0: they do (worse_only.py:42, 62).   union = tgt_cnt + pred_cnt - inter.
 *   per_image=1: outputs are (B,C), else (C).  Outputs are int64 and are ACCUMULATED into.
 * sea_confusion replaces Metrics.update's bincount (semseg/metrics.py:27-33): hist[t*C+p] += 1 for
 * every pixel whose label is valid.
 * Where only the argmax is needed (infer.py:88, metrics.py:28) call sea_loss_fwd_bwd with dlogits=NULL.
 */
int sea_class_counts(const void* pred, int pred_bytes, const void* y, int y_bytes, int B, int C,
                     int64_t HW, int mask_pred, int per_image, int64_t* inter, int64_t* pred_cnt,
                     int64_t* tgt_cnt, void* stream);
int sea_confusion(const void* pred, int pred_bytes, const void* y, int y_bytes, int64_t n, int C,
                  int64_t* hist, void* stream);

/* ------------------------------------------------------------------------------------------------
 * K4 + K7  device-resident APGD bookkeeping (no host round trip).
 *
 * sea_apgd_track: one tiny launch per iteration.  replaces semseg/attacker.py:370-383 (init=1),
 *   485-495 (best-adv tracking), 520-526 (best-loss tracking), 243-248 + 528-551 (oscillation
 *   check and step halving) and 568-569 (early stop, as a device flag).
 *     loss_sum/track_sum/n_correct  outputs of K2 for this iterate (or NULL + loss_workspace = the K2
 *               workspace of a deferred K2 call);  n_ignored (B) #ignored pixels
 *     iter      loop index i (ignored when init=1);  n_iter rows in loss_steps
 *     check_k   0, or the window k when this iteration is a checkpoint (schedule is data
 *               independent, attacker.py:528-551, so the host knows it)
 *   state (all (B) unless noted, updated in place):
 *     acc_cnt int32 (best = lowest #correct incl. ignored-as-correct), acc float = acc_cnt/HW,
 *     loss_best, loss_best_last, reduced_last, step (float32), loss_steps (n_iter,B) float32,
 *     flags uint8 (3,B): [0] copy x_adv->x_best_adv & pred->pred_best   (avg_acc <= acc)
 *                        [1] copy x_adv->x_best, grad->grad_best        (loss  >  loss_best)
 *                        [2] restart: x_adv<-x_best, grad<-grad_best    (step halved)
 *     done int32[1]: set to 1 when early_stop and every image has zero accuracy; once set, later
 *                    calls clear all flags and change nothing (the reference would have left the loop).
 * sea_select_copy: the conditional bulk copies selected by `flags` (attacker.py:494-495, 523-524,
 *   547-548), one launch.  pred/pred_best may be NULL.
 */
int sea_apgd_track(const float* loss_sum, const float* track_sum, const int32_t* n_correct,
                   const int32_t* n_ignored, int B, int64_t HW, int iter, int n_iter, int check_k,
                   int early_stop, int init, int32_t* acc_cnt, float* acc, float* loss_best,
                   float* loss_best_last, float* reduced_last, float* step, float* loss_steps,
                   uint8_t* flags, int32_t* done, const void* loss_workspace, void* stream);
/* Replayable forms of K1 / K7: what the attack loop runs every iteration, executed eagerly or recorded once in a HIP graph
 * and replayed.  Everything run-specific is a word in device memory and the buffers keep their addresses, so nothing is left
 * in the launch arguments: ONE recorded pair serves every stage, loss and batch of an evaluation (reference
 * semseg/attacker.py:691-728: three apgd_train calls per attack with eps 2e / 1.5e / e and 0.3n / 0.3n / 0.4n iterations;
 * tools/infer.py:338-370: three attacks per batch).
 *   sea_apgd_linf_step_graph: K1 IN PLACE (x_old <- x_adv, x_adv <- new iterate) with eps = *eps_dev (one float);
 *                             a = 1 when *iter_dev == 0, else 0.75.
 *   sea_apgd_track_graph:     K7 (init = 0) with iter = *iter_dev, n_iter = *n_iter_dev (one int32) and
 *                             check_k = check_table[iter] (0 = no checkpoint); advances *iter_dev by one at its end.
 *                             check_table and loss_steps must be sized for the longest run replayed. */
int sea_apgd_linf_step_graph(const float* x, float* x_adv, float* x_old, const float* grad, const float* step_b,
                             const float* eps_dev, const int32_t* iter_dev, int B, int64_t n_per_img, void* stream);
int sea_apgd_track_graph(const float* loss_sum, const float* track_sum, const int32_t* n_correct,
                         const int32_t* n_ignored, int B, int64_t HW, int32_t* iter_dev, const int32_t* check_table,
                         const int32_t* n_iter_dev, int early_stop, int32_t* acc_cnt, float* acc, float* loss_best,
                         float* loss_best_last, float* reduced_last, float* step, float* loss_steps, uint8_t* flags,
                         int32_t* done, const void* loss_workspace, void* stream);
int sea_select_copy(const uint8_t* flags, float* x_adv, float* grad, float* x_best,
                    float* grad_best, float* x_best_adv, const void* pred, void* pred_best,
                    int pred_bytes, int B, int64_t n_per_img, int64_t HW, void* stream);

/* sea_count_ignored: n_ignored[b] = #{y[b] ignored}  (attacker.py:302-306, 489). */
int sea_count_ignored(const void* y, int y_bytes, int B, int64_t HW, int32_t* n_ignored,
                      void* stream);

/* ------------------------------------------------------------------------------------------------
 * K8 + K9  worst-case bookkeeping over the attacks (HOST code, sequential by nature).
 * sea_worst_miou_greedy replaces evalSEA.worst_case_miou's greedy (tools/worse_only.py:279-334)
 * including _compute_miou / _compute_miou_subtraction (69-93) and Python's random.shuffle stream:
 *   ints/unions (A,N,C) float32 per-image tables (worse_only.py:200-234)
 *   mt_state    625 uint32: CPython `random.getstate()[1]` (624 words + position); advanced in
 *               place exactly as `random.shuffle` would, so the caller can `random.setstate` back
 *   outputs: *miou (fraction), selected (N) attack index per image, *rounds_run.
 * Arithmetic follows the reference bit for bit (float32 table differences, float32 rounding of the
 * running totals, float64 quotients, exactly rounded mean as in statistics.mean).
 */
int sea_worst_miou_greedy(const float* ints, const float* unions, int A, int N, int C,
                          uint32_t* mt_state, int n_rounds, double* miou, int32_t* selected,
                          int32_t* rounds_run);

/* ------------------------------------------------------------------------------------------------
 * M1  (model side) depthwise 7x7 convolution of the ConvNeXt block, stride 1, pad 3, fp32
 * NCHW: forward (flip=0, F.conv2d semantics incl. bias) and backward-data (flip=1: pass dy as x, bias
 * ignored).  Replaces the MIOpen/CK grouped convolution behind semseg/models/backbones/
 * convnext_orig.py:55-57, 75 - an HBM-bound stencil that the library runs ~25x below the roofline.
 *   x, y: (B*C, H, W) planes; w: (C,1,7,7); bias: (C) or NULL.
 */
int sea_dwconv7x7(const float* x, const float* w, const float* bias, float* y, int B, int C, int H,
                  int W, int flip, void* stream);
/* channels_last variant: x, y (B,H,W,C) contiguous, wt (49,C) taps-major (= w.view(C,49).T), C % 4 == 0.
 * With it the whole ConvNeXt block runs in NHWC: no permute / layout copy is left.
 * ab: A/B switches of the launcher, 0 = the shipped dispatch; a mask of 2 (plain block order), 4 (one output row per lane),
 * 8 (two rows per lane), 16 (the kernels without the software pipeline), 32 / 64 (filter rows from LDS never / always).
 * Every combination gives the same bits. */
int sea_dwconv7x7_nhwc(const float* x, const float* wt, const float* bias, float* y, int B, int C,
                       int H, int W, int flip, unsigned ab, void* stream);
/* same, plus an optional addend of y's shape: y = conv(x) + addend (added after the taps: bitwise what a separate
 * element-wise add gives).  The backward of a ConvNeXt block (x + branch(x), convnext_orig.py:75-86) passes the skip
 * gradient here, which removes one element-wise pass per block.  bias and addend are mutually exclusive. */
int sea_dwconv7x7_nhwc_add(const float* x, const float* wt, const float* bias, const float* addend, float* y, int B,
                           int C, int H, int W, int flip, unsigned ab, void* stream);

/* M2  (model side) bilinear up-sampling, align_corners=False, fp32 NCHW planes: forward and its
 * backward w.r.t. the input (gather formulation, deterministic; ATen scatters with atomics).
 * Replaces F.interpolate(..., mode="bilinear") in UperNet's FPN / PSP / final logits
 * (semseg/models/uperforseg.py:171-177, 236-262, 416-418) where ATen reaches ~0.3 TB/s.
 *   x / gx: (planes, h, w);  y / gy: (planes, H, W);  H >= h, W >= w, any (non-integer) scale.
 */
int sea_upsample_bilinear_fwd(const float* x, float* y, int64_t planes, int h, int w, int H, int W,
                              void* stream);
int sea_upsample_bilinear_bwd(const float* gy, float* gx, int64_t planes, int h, int w, int H, int W,
                              void* stream);
/* channels_last variants (x/gx: (B,h,w,C), y/gy: (B,H,W,C), C % 4 == 0, 16-byte aligned): lanes run
 * along C, so the head's NHWC tensors (what MIOpen's igemm convolutions return) need no layout copy.
 * y / gy may be a channel slice of a wider NHWC tensor (the FPN / PSP concatenation buffers,
 * uperforseg.py:171-177, 255-262): *_pixel_stride = floats between consecutive pixels (>= C, % 4 == 0),
 * batch stride = H*W*pixel_stride.  The up-sampled maps are then written straight into the buffer
 * torch.cat would have produced, and the gradient is gathered straight out of its gradient.
 * residual (NULL or dense (B,H,W,C)): y = residual + up(x), the FPN top-down add (uperforseg.py:243-250). */
int sea_upsample_bilinear_nhwc_fwd(const float* x, const float* residual, float* y, int B, int C, int h,
                                   int w, int H, int W, int64_t y_pixel_stride, void* stream);
int sea_upsample_bilinear_nhwc_bwd(const float* gy, float* gx, int B, int C, int h, int w, int H, int W,
                                   int64_t gy_pixel_stride, void* stream);
/* host only, touches no device: the kernel one of the four entries above, or sea_tap_gather_fwd / _bwd (M6), runs for these
 * integers (csrc/upsample_plan.h).  op = SEA_UP_*; planes_or_batch = planes for the NCHW entries, B for the others; C and
 * pixel_stride are read for NHWC (C for the tap gather too).  Only the alignment of the two addresses matters: src = what the
 * kernel reads (x | residual, gy, G, gz), dst = what it writes.  general_only / xcd_order: the two words of
 * sea_process_config that the entries themselves pass (SEA_UPSAMPLE_GENERAL, SEA_XCD_ORDER = 0 | 1 | 2).
 * out[20] = kernel (enum UpsampleKernel of the plan header, in its order), S (template parameter, 0 = none), grid x, grid y,
 * threads, dynamic LDS bytes, planes per launch and launches of the chunked general NCHW kernels, work items (low, high 32
 * bits), the kernel's xcd argument, nt, lcols, RP, bands, per_xcd, TI, RMAX, nbh, nbw.  Returns 1 for exactly the integers
 * for which the entry returns 1. */
#define SEA_UP_NCHW_FWD 0
#define SEA_UP_NCHW_BWD 1
#define SEA_UP_NHWC_FWD 2
#define SEA_UP_NHWC_BWD 3
#define SEA_UP_TAP_FWD 4
#define SEA_UP_TAP_BWD 5
int sea_upsample_plan(int op, int64_t planes_or_batch, int C, int h, int w, int H, int W, int64_t pixel_stride,
                      size_t src_addr, size_t dst_addr, int general_only, int xcd_order, int32_t out[20]);

/* M4  (model side) Winograd F(m x m, 3 x 3) transforms, m = 2 or 4, for the 3x3 / stride 1 / pad 1
 * convolutions of the UperNet head (uperforseg.py:200-215 fpn_convs, 255-262 fpn_bottleneck), fp32 NHWC.
 * The convolution becomes  y = OUT( bmm( IN(x), FIL(w) ) ): the (m+2)^2 GEMMs in the middle are a plain
 * strided-batched fp32 GEMM (hipBLASLt); these three entry points are the HBM-bound transforms.
 *   T = sea_wino_tiles(B, H, W, m) = B * ceil(H/m) * ceil(W/m),  A = m + 2
 *   sea_wino_input_transform :  x (B,H,W,C) -> V (A*A, T, C); x may be a channel slice of a wider NHWC
 *                               tensor (x_pixel_stride floats between pixels, >= C, % 4 == 0: the gradient
 *                               of a concatenation buffer is read in place), and V a channel slice of a
 *                               wider (A*A, T, v_tile_stride) tensor (inputs that the reference concatenates
 *                               are transformed side by side, never concatenated); with gate (B,H,W,C, dense) the tiles are loaded
 *                               as  gate > 0 ? x * scale[c] : 0  (scale NULL = 1): the backward of the
 *                               fused epilogue below, applied to the incoming output gradient
 *   sea_wino_filter_transform:  w (Cout,Cin,3,3) -> U (A*A, Cin, Cout)             (flip = 0, forward)
 *                               w -> U (A*A, Cout, Cin) of the 180-degree rotated filters (flip = 1: the
 *                               convolution that yields the input gradient from the output gradient)
 *   sea_wino_output_transform:  M (A*A, T, C) -> y (B,H,W,C) = act(scale[c] * (conv + addend) + bias[c]);
 *                               addend (B,H,W,C) / scale / bias may be NULL, act = ReLU when relu != 0.  With scale/bias = the folded
 *                               eval-mode BatchNorm this is the whole ConvModule (uperforseg.py:119-146).
 * C % 4 == 0, 16-byte aligned pointers.
 * Matrix convention (V, U and M mean something only relative to it): the published F(2x2,3x3) / F(4x4,3x3) matrices of
 * Lavin & Gray, "Fast Algorithms for Convolutional Neural Networks" (2015), interpolation points 0, +-1 (, +-2), infinity:
 *   V[i*A+j] = (B^T d B)[i][j],  d = the A x A input patch whose top-left pixel is (ty*m - 1, tx*m - 1), zero outside the image
 *   U[i*A+j] = (G g G^T)[i][j],  g = the 3 x 3 filter (rotated by 180 degrees when flip = 1)
 *   y tile   = A^T m A,          m[i][j] = M[i*A+j], the m x m output pixels from (ty*m, tx*m); pixels beyond H, W are not written
 *   m = 2:  B^T = [1 0 -1 0; 0 1 1 0; 0 -1 1 0; 0 1 0 -1]    G = [1 0 0; 1/2 1/2 1/2; 1/2 -1/2 1/2; 0 0 1]
 *           A^T = [1 1 1 0; 0 1 -1 -1]
 *   m = 4:  B^T = [4 0 -5 0 1 0; 0 -4 -4 1 1 0; 0 4 -4 -1 1 0; 0 -2 -1 2 1 0; 0 2 -1 -2 1 0; 0 4 0 -5 0 1]
 *           G   = [1/4 0 0; -1/6 -1/6 -1/6; -1/6 1/6 -1/6; 1/24 1/12 1/6; 1/24 -1/12 1/6; 0 0 1]
 *           A^T = [1 1 1 1 1 0; 0 1 -1 2 -2 0; 0 1 1 4 4 0; 0 1 -1 8 -8 1]
 * oracle/sea_oracle.py (wino_input_f64 / wino_filter_f64 / wino_output_f64) restates the three transforms in float64 from
 * these matrices; tests/test_wino_transforms_gpu.py compares every kernel variant with it.
 * vec4 (m = 4; A/B): four channels per lane instead of two; shipped: 1 in the input transforms, 0 in the output
 * transform. */
int64_t sea_wino_tiles(int B, int H, int W, int m);
int sea_wino_input_transform(const float* x, int64_t x_pixel_stride, const float* gate, const float* scale,
                             float* V, int64_t v_tile_stride, int B, int C, int H, int W, int m, int vec4, void* stream);
int sea_wino_filter_transform(const float* w, float* U, int Cout, int Cin, int m, int flip, void* stream);
/* sea_wino_input_transform that also max-accumulates, per tile t, the float bits of max|V[.][t][.]| into amax_out[t]
 * (sea_wino_tiles pre-zeroed words): the per-row fp16 x 2 scales of the Winograd-domain GEMMs (sea_gemm_split_f16 with
 * amax_rows = 1), each depending on its own tile only.  T < 2^31. */
int sea_wino_input_transform_amax(const float* x, int64_t x_pixel_stride, const float* gate, const float* scale, float* V,
                                  int64_t v_tile_stride, int B, int C, int H, int W, int m, int vec4, uint32_t* amax_out,
                                  void* stream);
int sea_wino_output_transform(const float* M, const float* addend, const float* scale, const float* bias,
                              int relu, float* y, int B, int C, int H, int W, int m, int vec4, void* stream);

/* M5  (model side) LayerNorm over the last dimension of a (rows, C) fp32 tensor with few channels (ConvNeXt:
 * C = 48..768, eps 1e-6; convnext_orig.py:19-40), forward and input gradient (w, b frozen).  A row is owned
 * by 16/32/64 lanes instead of a whole workgroup.  C % 4 == 0, C <= 1024; mean / rstd: (rows) saved statistics. */
int sea_layernorm_fwd(const float* x, const float* w, const float* b, float* y, float* mean, float* rstd,
                      int64_t rows, int C, float eps, void* stream);
int sea_layernorm_bwd(const float* g, const float* x, const float* w, const float* mean, const float* rstd,
                      float* dx, int64_t rows, int C, void* stream);

/* T3a (model side, training) sea_layernorm_bwd with trainable affine parameters (convnext_orig.py:19-40): dx, bit for bit
 * sea_layernorm_bwd's (one kernel source, one translation unit), plus dw[c] = sum_r g[r,c] * xhat[r,c] and
 * db[c] = sum_r g[r,c], xhat = (x - mean) * rstd.  Deterministic two-stage sum, no float atomics, grid a function of
 * (rows, C) only: a thread adds its rows in increasing index (dw: one fma per row), a block combines its row groups
 * through LDS in slot order into one partial row of `ws` (sea_layernorm_bwd_params_workspace(rows, C) floats, 16-byte
 * aligned), then the blocks are added in index order, associated as a balanced binary tree (adjacent blocks first: a
 * left-to-right walk over up to 1024 partial rows would round 1024 times at the magnitude of the total).  Same contract as M5: C % 4 == 0, C <= 1024, 16-byte alignment. */
int64_t sea_layernorm_bwd_params_workspace(int64_t rows, int C);
int sea_layernorm_bwd_params(const float* g, const float* x, const float* w, const float* mean, const float* rstd,
                             float* dx, float* dw, float* db, float* ws, int64_t rows, int C, void* stream);

/* T3b (model side, training) the tail of a ConvNeXt block on dense NHWC rows (convnext_orig.py:75-86: layer scale,
 * stochastic depth, residual add), rows = B * HW < 2^31, one streaming pass with 16-byte accesses per direction:
 *   forward :  out[r,c] = x[r,c] + (y[r,c] * gamma[c]) * s[r / HW]        (two rounded products, then the add)
 *   backward:  t = g[r,c] * s[r / HW];  gy[r,c] = t * gamma[c];  ggamma[c] = sum_r t * y[r,c]  (gx = g: no kernel)
 * s (B): 0 or 1 / keep per image, NULL = 1; gamma (C) or NULL = 1.  No special case for a dropped image: s = 0 multiplies.
 * ggamma (NULL: not computed; else y and `ws`, sea_block_tail_bwd_workspace(rows, C) floats, are required and gy may be
 * NULL) by the two-stage sum of T3a: per thread rows in increasing index by one fma each, row groups of a block through
 * LDS in slot order, blocks in index order as a balanced binary tree.  No float atomics; bitwise reproducible.  C % 4 == 0, C <= 1024, 16-byte
 * alignment of the row tensors, gamma and ws. */
int sea_block_tail_fwd(const float* x, const float* y, const float* gamma, const float* s, float* out, int64_t rows, int HW,
                       int C, void* stream);
int64_t sea_block_tail_bwd_workspace(int64_t rows, int C);
int sea_block_tail_bwd(const float* g, const float* y, const float* gamma, const float* s, float* gy, float* ggamma, float* ws,
                       int64_t rows, int HW, int C, void* stream);

/* M1w (model side, training) weight and bias gradient of the NHWC depthwise 7x7: gw (C,7,7), gb (C) or NULL from x and gy
 * (B,H,W,C) dense fp32 (PIR-AT's outer backward; convnext_orig.py:55-57).  Deterministic two-pass sum (per-tile partial
 * sums in `ws`, sea_dwconv7x7_nhwc_wgrad_workspace(B, C, H) floats, then the tiles in index order).  C % 4 == 0. */
int64_t sea_dwconv7x7_nhwc_wgrad_workspace(int B, int C, int H);
int sea_dwconv7x7_nhwc_wgrad(const float* x, const float* gy, float* gw, float* gb, float* ws, int B, int C, int H, int W,
                             void* stream);

/* M2'' (model side) adaptive average pooling of an NHWC fp32 map to oh x ow bins with ATen's bin rule (the pyramid pooling
 * of the head, uperforseg.py:150-177: 16 x 16 -> 1, 2, 3, 6), forward and input gradient; one block per bin x 16 channel
 * groups (ATen's NHWC kernel runs these maps on 8 blocks).  C % 4 == 0, oh <= H, ow <= W, dense tensors. */
int sea_adaptive_avg_pool_nhwc_fwd(const float* x, float* out, int B, int C, int H, int W, int oh, int ow, void* stream);
int sea_adaptive_avg_pool_nhwc_bwd(const float* g, float* dx, int B, int C, int H, int W, int oh, int ow, void* stream);

/* M9  (model side) the convolutional stem of the robust ConvNeXt backbones (backbones/convnext_orig.py:17-38:
 * Conv2d(3,48,3,s2,p1) -> LayerNorm(channels_first, eps 1e-6) -> GELU -> Conv2d(48,96,3,s2,p1) -> LayerNorm -> GELU), for
 * frozen parameters: forward and input gradient.  fp32 FMA in a fixed order (bitwise reproducible).  The image and its
 * gradient are NCHW; the tensors between the two convolutions are NHWC (the library's fast layout for the 48 -> 96
 * convolution, which stays a library call).
 *   sea_stem_conv1_ln_gelu: x (B,3,H,W) NCHW -> y (B,Ho,Wo,CO) NHWC = conv(x) + bias, and, unless a == NULL, a = GELU(LN_c(y))
 *                           (NHWC); Ho = (H-1)/2+1, Wo = (W-1)/2+1; w (CO,3,3,3); bias may be NULL; CO == 48.
 *   sea_stem_conv1_bwd    : dy (B,Ho,Wo,CO) NHWC -> dx (B,3,H,W) NCHW, the input gradient of that convolution.
 *   sea_ln_gelu_cl_fwd/bwd: a = GELU(LN over C of y) for y (B,HW,C) NHWC, C in {48, 96}; a / da are NHWC, or NCHW (B,C,HW)
 *                           when a_nchw != 0; dy (NHWC) from da with the statistics recomputed from y (nothing else is saved
 *                           by the forward).
 * Anything else (other CO / C) returns 1 (invalid argument): the caller keeps its library path. */
int sea_stem_conv1_ln_gelu(const float* x, const float* w, const float* bias, const float* gamma, const float* beta,
                           float* y, float* a, int B, int CO, int H, int W, float eps, void* stream);
int sea_stem_conv1_bwd(const float* dy, const float* w, float* dx, int B, int CO, int H, int W, void* stream);
int sea_ln_gelu_cl_fwd(const float* y, const float* gamma, const float* beta, float* a, int a_nchw, int B, int C, int64_t HW,
                       float eps, void* stream);
int sea_ln_gelu_cl_bwd(const float* da, int a_nchw, const float* y, const float* gamma, const float* beta, float* dy, int B,
                       int C, int64_t HW, float eps, void* stream);

/* M6  (model side) the FPN bottleneck without up-sampling its coarse inputs (uperforseg.py:255-262).  Channel
 * mixing commutes with bilinear up-sampling, so for an input that is an xs up-sampling (s >= 3) the nine 3x3
 * taps are applied as one GEMM at the coarse resolution, G = f @ W -> (B,h,w,9,C), and only a gather is left
 * at the output resolution:
 *   sea_tap_gather_fwd: extra (B,H,W,C) (+)= sum_taps shift_tap(up(G[..., tap, :]))   (accumulate != 0: +=)
 *   sea_tap_gather_bwd: gz (B,H,W,C) -> dG (B,h,w,9,C), the exact adjoint (then df = dG @ W^T)
 *   sea_gate_scale    : out = gate > 0 ? g * scale[c] : 0, the backward of relu(scale * z + shift) (NHWC)
 * `extra` enters sea_wino_output_transform as `addend`.  C % 4 == 0, 16-byte aligned.
 * inner (forward): non-zero = interior blocks take the path with compile-time interpolation weights (shipped), 0 = run-time
 * weights everywhere (A/B). */
int sea_tap_gather_fwd(const float* G, float* extra, int accumulate, int B, int C, int h, int w, int H, int W,
                       int inner, void* stream);
int sea_tap_gather_bwd(const float* gz, float* dG, int B, int C, int h, int w, int H, int W, void* stream);
int sea_gate_scale(const float* g, const float* gate, const float* scale, float* out, int64_t pixels, int C,
                   void* stream);

/* M3  (model side) NCHW <-> NHWC layout changes of the ConvNeXt block through LDS-tiled transposes,
 * fused with the per-channel layer scale and the residual add (convnext_orig.py:75-86: the two
 * `permute`s, `gamma * x` and `input + x`).  C % 4 == 0 and HW % 4 == 0.
 *   sea_nchw_to_nhwc: out[b,p,c] = scale[c] * in[b,c,p]                    (scale may be NULL)
 *   sea_nhwc_to_nchw: out[b,c,p] = residual[b,c,p] + scale[c] * in[b,p,c]  (scale / residual may be NULL)
 */
int sea_nchw_to_nhwc(const float* in, const float* scale, float* out, int B, int C, int64_t HW, void* stream);
int sea_nhwc_to_nchw(const float* in, const float* scale, const float* residual, float* out, int B, int C,
                     int64_t HW, void* stream);

/* 2x2 patch gather / scatter for the trunk's 2x2 / stride-2 down-sampling convolutions (convnext_orig.py:118-124):
 * pixels (B,H,W,C) channels_last <-> patch rows (B*H/2*W/2, 4*C) in (di, dj, c) order, so that the convolution is one GEMM
 * (bitwise reproducible, unlike the MIOpen kernel it replaces).  inverse != 0: patches -> pixels (the backward). */
int sea_patch2x2(const float* src, float* dst, int B, int H, int W, int C, int inverse, void* stream);

/* ------------------------------------------------------------------------------------------------
 * M7  fp32 multi-head attention on the matrix cores (v_mfma_f32_32x32x2_f32), flash formulation.
 *     replaces the explicit softmax(q k^T * scale) v of semseg/models/backbones/vit_encoder.py:106-127 (fp32 operands,
 *     N = 1025 tokens x 6 heads x 64 in Segmenter ViT-S/16) and its autograd backward.
 * q, k, v: element (b, h, t, d) at ptr + b*sb + h*sh + t*st + d floats (d contiguous; the three may be slices of one
 *   packed (B,T,3,H,64) qkv tensor: sb = T*3*H*64, sh = 64, st = 3*H*64).  D must be 64.  Rows 16-byte aligned.
 * out (B,T,H*64) contiguous: the layout the output projection consumes.  lse (B,H,T): log-sum-exp of the scaled scores.
 * backward: grad_out (B,T,H*64) contiguous; delta (B,H,T) scratch; dq/dk/dv are written with strides
 *   (gsb, gsh, gst) -- pass slices of one (B,T,3,H,64) gradient tensor to get d(qkv) without a concatenation.
 *   Deterministic (no atomics): S is recomputed in the dq kernel and in the dk/dv kernel.
 * Arithmetic (csrc/attention_bf16.hip): the products run on v_mfma_f32_32x32x16_bf16 with every fp32 operand split into
 *   `terms` bf16 numbers, fp32 accumulate: 3 (= the fp32 operands exactly, six products) or 2; terms = 0 selects the fp32 MFMA
 *   kernels of csrc/attention.hip.  The caller chooses per call; the library reads no environment.
 */
/* the backward, with the number of bf16 terms of its products given by the caller (3, 2, or 0 = fp32 MFMA):
 * 3 when the weights are trained through this backward, 2 when only the sign of the input gradient is consumed. */
int sea_attention_bwd_terms(const float* q, const float* k, const float* v, int64_t sb, int64_t sh, int64_t st, int B, int H,
                            int T, int D, float scale, const float* out, const float* grad_out, const float* lse,
                            float* delta, float* dq, float* dk, float* dv, int64_t gsb, int64_t gsh, int64_t gst,
                            int terms, void* stream);
/* The forward and the backward with fp16 x 2 operands: 22 significant bits per operand in THREE MFMA products per pair (the accuracy of the
 * three-term bf16 mode at the cost of the two-term one).  Power-of-two scales: the exact row maximum for a lane's own
 * Q / K / V / dO row, one per (image, head) for the staged tiles (from a pre-pass this call launches), analytic bounds for the
 * soft-max operands P and dS.  amax_ws: 4 B H uint32 words of device scratch. */
/* the forward, with the number of bf16 terms of the products given by the caller (3, 2, or 0 = fp32 MFMA) */
int sea_attention_fwd_terms(const float* q, const float* k, const float* v, int64_t sb, int64_t sh, int64_t st, int B, int H,
                            int T, int D, float scale, float* out, float* lse, int terms, void* stream);
int sea_attention_fwd_f16(const float* q, const float* k, const float* v, int64_t sb, int64_t sh, int64_t st, int B, int H,
                          int T, int D, float scale, uint32_t* amax_ws, float* out, float* lse, void* stream);
int sea_attention_bwd_f16(const float* q, const float* k, const float* v, int64_t sb, int64_t sh, int64_t st, int B, int H,
                          int T, int D, float scale, const float* out, const float* grad_out, const float* lse,
                          float* delta, uint32_t* amax_ws, float* dq, float* dk, float* dv, int64_t gsb, int64_t gsh,
                          int64_t gst, void* stream);

/* ------------------------------------------------------------------------------------------------
 * M8  fp32 GEMM with frozen weights on the bf16 matrix cores (v_mfma_f32_32x32x16_bf16) by operand splitting:
 *     every fp32 operand is the exact sum of `terms` bf16 numbers (3: all 24 significant bits, six products, fp32-level
 *     accuracy; 2: 16 bits, three products), fp32 accumulation, fixed order (bitwise reproducible).
 *     replaces the hipBLASLt fp32 GEMMs behind the frozen-weight layers of the attacked model: the Winograd-domain
 *     products of the UperNet head's 3x3 convolutions (semseg/models/uperforseg.py:200-215, 255-262), its 1x1
 *     ConvModules (uperforseg.py:119-146) and the point-wise layers of the ConvNeXt blocks, forward and input gradient.
 *   C[g] (M x N, row stride ldc) = A[g] (M x K fp32, row stride lda) * W[g]^T + bias[n], optional ReLU; g < batch,
 *   batch strides in elements (A, C) / bytes (packed W).  K % 32 == 0, lda % 4 == 0, A 16-byte aligned.
 * sea_gemm_split_pack: W (N x K row-major, or K x N with trans = 1; row stride ldw) -> the packed, pre-split image the
 *   kernel reads ([K/32][terms][ceil128(N)][32] bf16, sea_gemm_split_packed_bytes bytes).  Done once per weight.
 * terms = 1 keeps one bf16 term per operand (the operands of a bf16-autocast GEMM, one product, fp32 accumulate and fp32
 *   in / out): the attack forward / backward of PIR-AT's inner PGD under TRAIN.AMP (BASELINE configs[3]).
 * terms = 22 selects fp16 x 2 operands instead (hi = fp16(x*s), mid = fp16(x*s - hi): 22 significant bits, three
 *   products on v_mfma_f32_32x32x16_f16): fp16 has 5 exponent bits, so the weights are packed with a power-of-two scale per
 *   output row and the activations are scaled by a power of two derived from max|A|, which the caller obtains on the device
 *   with sea_absmax_bits (one 4-byte word, no host round trip) and hands to sea_gemm_split_f16; the epilogue undoes both
 *   scales exactly.  Elements more than 2^28 below the tensor's maximum flush to zero.
 *
 * variant (sea_gemm_split, _f16, _fused): which of the kernels behind the entry runs, per call.  0 = the shipped dispatch
 *   (chosen per launch from the shape, 32x32x16 fragments).  SEA_GEMM_PIPE_SINGLE = the single-stage K loop (three blocks per
 *   CU), SEA_GEMM_PIPE_PINGPONG = two LDS stages, one barrier per K step, the operand split in the shadow of the wave's own
 *   MFMAs (two blocks per CU), SEA_GEMM_PIPE_BIG = the one-block-per-CU 256 x 256 / 128 x 384 kernels wherever they apply.
 *   Same split and same MFMA order: every pipeline gives the same bits.  | SEA_GEMM_SHAPE16 = v_mfma_f32_16x16x32_* fragments
 *   (single-stage loop only; last bits differ: summation order).  Any other bit -> invalid argument.
 *   The whole map from (shape, strides, terms, prologue / epilogue, word) to kernel, template parameters, grid and LDS bytes
 *   is the one host function of csrc/gemm_plan.h; sea_gemm_plan below reports it without a launch.
 */
#define SEA_GEMM_VARIANT_DEFAULT 0u
#define SEA_GEMM_PIPE_SINGLE 1u
#define SEA_GEMM_PIPE_PINGPONG 2u
#define SEA_GEMM_PIPE_BIG 3u
#define SEA_GEMM_PIPE_MASK 3u
#define SEA_GEMM_SHAPE16 4u
/* host only, touches no device: the kernel a sea_gemm_split* call with these integers runs (csrc/gemm_plan.h).  terms 1 | 2 |
 * 3 | 22; ld_addend: SeaGemmEpilogue.ld_addend (0 without); prologue: 0 none, 1 a_gelu_grad_of, 2 a_gelu, 3 a_gelu_grad_of as
 * a_gate; fused: addend, gelu_out or gelu_grad_of given.  Returns what the call would return for them (0, or 1 = invalid
 * argument) and fills out = {kernel, terms_t, f16, s16, epi, pro, depth, bm, bn, npad, mblocks, nblocks, tiles, grid, threads,
 * lds}: kernel 0 = single-stage, 1 = ping-pong, 2 = 256 x 256 tiles, 3 = 128 x 384 tiles (one block per CU); terms_t .. depth
 * = the template parameters; bm x bn tiles, npad = rows of the packed weights, tiles = mblocks * nblocks * batch, grid =
 * blocks (tiles rounded up to a multiple of 8), threads per block, lds = dynamic LDS bytes. */
int sea_gemm_plan(int M, int N, int K, int terms, int batch, int64_t lda, int64_t ldc, int64_t ld_addend, int prologue, int fused,
                  unsigned variant, int32_t out[16]);
int64_t sea_gemm_split_packed_bytes(int N, int K, int terms);
int sea_absmax_bits(const float* A, int64_t lda, int M, int K, int batch, int64_t strideA, int rows_per_word,
                    uint32_t* out_bits, void* stream);
int sea_gemm_split_f16(const float* A, int64_t lda, const void* Wp, float* C, int64_t ldc, const float* bias, int relu, int M,
                       int N, int K, int batch, int64_t strideA, int64_t strideW_bytes, int64_t strideC,
                       const uint32_t* amax_bits, int amax_rows, uint32_t* out_amax, unsigned variant, void* stream);
/* The activation scale is a power of two PER ROW of A, taken from amax_bits[row / amax_rows] (amax_rows = 0: one word for
 * the whole tensor): a word is the float bits of any upper bound of max|A| over its rows (all batch entries).  With one
 * word per image (amax_rows = rows of an image) or per row, an image's result does not depend on the images it shares a
 * batch with -- a per-tensor scale moves the sub-normal cut-off of the low fp16 term with the batch maximum, which changes
 * last bits and was measured to break the sharded evaluation's bitwise 1-rank == 2-rank property.
 * sea_absmax_bits(rows_per_word) computes the words exactly (rows_per_word = 0: one word; 1: one word per row, one writer
 * per word -- the scales of a GRADIENT operand, whose rows span many orders of magnitude); producers can supply them for
 * free: sea_wino_input_transform_amax (one word per tile), analytic bounds (LayerNorm output: sqrt(C) max|w| + max|b|; a
 * GEMM's output: bound(input) * max_n ||W_n||_1 + max|bias|), or the out_amax word (whole-tensor max|C|) of the GEMM whose
 * output feeds a non-expanding element-wise function.  A loose bound costs nothing up to a factor ~2^10 (fp16 is floating
 * point: only the sub-normal cut-off of the low term moves; error <= looseness * 2^-40 of the bound). */
int sea_gemm_split_pack(const float* W, int64_t ldw, int trans, int N, int K, int terms, void* out, void* stream);
/* sea_gemm_splitk_reduce: second pass of a split-K product.  A GEMM whose 128 x 128 tile grid cannot fill the chip (few
 * rows, long K: the point-wise layers of the last ConvNeXt stages, the FPN taps' input gradient) is launched as a BATCH of
 * `splits` GEMMs over K slices (batch strides of sea_gemm_split: A + s K/splits, packed slices of W) into a dense
 * (splits, M, N) workspace; this kernel adds the slices in the fixed order 0, 1, .. (bitwise reproducible), then bias,
 * ReLU and the optional max|C| word.  N % 4 == 0, ldc % 4 == 0, 16-byte aligned pointers. */
int sea_gemm_splitk_reduce(const float* partial, int splits, int M, int N, const float* bias, const float* addend,
                           int64_t ld_addend, int relu, float* C, int64_t ldc, uint32_t* out_amax, void* stream);
/* sea_gemm_split_fused: the same GEMM (terms 2 / 3 / 22; amax_bits / out_amax as above, 22 only) with the element-wise
 * neighbours of the MLP of a ConvNeXt / ViT block (convnext_orig.py:38-58, vit_encoder.py:41-60) in its epilogue:
 *   v = A W^T + bias + addend;  relu;  v *= GELU'(gelu_grad_of);  C = v;  gelu_out = GELU(v)     (exact erf GELU)
 * addend: the residual of the block (forward of the second projection); gelu_out: forward of the first projection (C keeps
 * the pre-activation the backward needs); gelu_grad_of: backward of the second projection (the gradient of the first
 * projection's output, without a separate GELU-backward pass).  gelu_out / gelu_grad_of have C's layout (ldc, strideC).
 * epi may be NULL (= sea_gemm_split / sea_gemm_split_f16). */
typedef struct SeaGemmEpilogue {
  const float* addend;
  int64_t ld_addend, stride_addend;
  float* gelu_out;
  const float* gelu_grad_of;
  const float* a_gelu_grad_of; /* PROLOGUE instead of epilogue (exclusive with the fields above; terms 2 or 22): A is read as
                                * A * GELU'(a_gelu_grad_of), same layout as A (lda, strideA): the GELU backward in front of the
                                * first projection's input-gradient GEMM, applied while the tile is staged */
  int a_gate;                  /* with a_gelu_grad_of: the tensor is a ReLU gate instead, A is read as (gate > 0 ? A : 0): the
                                * backward of a fused GEMM + ReLU in front of its input-gradient GEMM */
  int a_gelu;                  /* PROLOGUE (exclusive with everything above): A is read as GELU(A): the activation in front of the
                                * second projection's forward GEMM, without materialising GELU(A) */
  float a_amax_mul;            /* terms 22, > 0: the amax_bits words bound max|A| only after multiplication by this constant (a
                                * producer-side per-row bound carried through the GEMM in between: rowmax(g) * max_n ||W_n||_1,
                                * times max|GELU'| = 1.13 for the a_gelu_grad_of prologue); 0 = 1: the words as they are */
  const float* a_amax_mul_dev; /* the same constant as ONE float in device memory (takes precedence when non-NULL): a caller whose
                                * weights change every step (PIR-AT) derives it on the device without a host round trip */
} SeaGemmEpilogue;
int sea_gemm_split_fused(const float* A, int64_t lda, const void* Wp, float* C, int64_t ldc, const float* bias, int relu, int M,
                         int N, int K, int terms, int batch, int64_t strideA, int64_t strideW_bytes, int64_t strideC,
                         const uint32_t* amax_bits, int amax_rows, uint32_t* out_amax, const SeaGemmEpilogue* epi,
                         unsigned variant, void* stream);
int sea_gemm_split(const float* A, int64_t lda, const void* Wp, float* C, int64_t ldc, const float* bias, int relu, int M,
                   int N, int K, int terms, int batch, int64_t strideA, int64_t strideW_bytes, int64_t strideC,
                   unsigned variant, void* stream);
/* ------------------------------------------------------------------------------------------------
 * M10  the decode head's classifier, a 1 x 1 convolution onto a SMALL number of classes (semseg/models/uperforseg.py:262
 *      `cls_seg`; reference autograd for the input gradient), forward and input gradient for frozen weights, on
 *      v_mfma_f32_32x32x2_f32 (exact fp32 products).  Replaces torch.matmul (hipBLASLt) on these shapes.
 *   y / gy: (B P, K) fp32 NHWC rows, contiguous, 16-byte aligned; W: (cls, K) contiguous, 16-byte aligned; bias (cls) or NULL;
 *   out / g: (B, cls, P) fp32 NCHW, contiguous.  Shapes: sea_classifier_supported (P % 32 == 0, K % 64 == 0, K <= 1024,
 *   cls <= 32); anything else -> SEA_ERR_ARG.
 *   backward, optional: gate (layout of gy) and gate_scale (K): gy = gate > 0 ? gy * gate_scale[k] : 0, the backward of the
 *   ReLU(scale z + shift) that produced y (uperforseg.py:296-304 with the eval-mode BatchNorm folded) -- bit for bit
 *   sea_gate_scale applied to the stored gradient, without the 0.8 GB pass. */
int sea_classifier_supported(int P, int K, int cls);
int sea_classifier_fwd(const float* y, const float* W, const float* bias, float* out, int B, int P, int K, int cls, void* stream);
int sea_classifier_bwd(const float* g, const float* W, float* gy, int B, int P, int K, int cls, const float* gate,
                       const float* gate_scale, void* stream);
/* ------------------------------------------------------------------------------------------------
 * M8f  the MLP of a ConvNeXt block, y = res + W2 GELU(W1 x + b1) + b2 (semseg/models/backbones/convnext_orig.py:77-79:
 *      pwconv1 -> act -> pwconv2 with the layer scale folded into W2; reference autograd for the input gradient), as ONE
 *      kernel per direction.  Replaces, bit for bit, the pair of sea_gemm_split_fused launches (a_gelu / a_gelu_grad_of
 *      prologues), the residual add and -- backward -- the sea_absmax_bits(rows_per_word = 1) pass: a wave owns 32 rows for
 *      the whole MLP, the 4C-wide hidden tensor lives in accumulators and operand registers only (it is the HBM traffic that
 *      bounds the two-GEMM form at C = 96 / 192).  The backward recomputes t = W1 x + b1: the forward saves nothing but x.
 *   x, res, y / g, dx: (M, C) fp32 rows (row strides in elements, % 4 == 0, 16-byte aligned); H = 4 C; C in {96, 192}
 *     (sea_mlp_fused_supported).  W1p = sea_gemm_split_pack(w1: N = H, K = C, terms 22), W2p = pack(w2: N = C, K = H);
 *     backward: W2tp = pack(w2, trans = 1: N = H, K = C), W1tp = pack(w1, trans = 1: N = C, K = H).
 *   amax_x / amax_h: ONE device word each, float bits of an upper bound of max|x| / max|GELU(W1 x + b1)| (the analytic
 *     bounds of sea_gemm_split_f16's comment); amax_mul_dev: ONE float, rowmax|g[r]| * it bounds row r of (g W2) GELU'
 *     (SeaGemmEpilogue.a_amax_mul_dev).  b2 / res may be NULL. */
int sea_mlp_fused_supported(int C, int H);
/* The same pair with the block's LayerNorm (over the C channels, affine ln_w / ln_b, eps) in front of the MLP
 * (convnext_orig.py:75-77: norm -> pwconv1): x is the LayerNorm's INPUT, amax_x bounds its OUTPUT; the backward returns the
 * gradient w.r.t. x (frozen affine parameters).  The channel sums follow sea_layernorm_fwd / _bwd's summation order: replaces
 * those two launches and the round trip of the normalised tensor without changing a bit. */
int sea_ln_mlp_fused_fwd(const float* x, int64_t ldx, const float* ln_w, const float* ln_b, float ln_eps, const void* W1p,
                         const float* b1, const void* W2p, const float* b2, const float* res, int64_t ldres, float* y,
                         int64_t ldy, int M, int C, int H, const uint32_t* amax_x, const uint32_t* amax_h, void* stream);
int sea_ln_mlp_fused_bwd(const float* g, int64_t ldg, const float* x, int64_t ldx, const float* ln_w, const float* ln_b,
                         float ln_eps, const void* W1p, const float* b1, const void* W2tp, const void* W1tp, float* dx,
                         int64_t lddx, int M, int C, int H, const uint32_t* amax_x, const float* amax_mul_dev, void* stream);
/* test probe: out[0], out[1] (two pre-zeroed 64-bit device words) += the number of fp32 bit patterns for which the branch-free
 * GELU / GELU' evaluation inside the fused kernels differs from the one of sea_gemm_split's prologues (must stay 0, 0) */
int sea_probe_gelu_mismatches(unsigned long long* out, void* stream);
/* test probe: the LayerNorm of the fused kernels' prologue on its own (x dense (M, C), C in {96, 192}): yn, mean, rstd must equal
 * sea_layernorm_fwd's bit for bit */
int sea_probe_ln_rows(const float* x, const float* ln_w, const float* ln_b, float eps, int M, int C, float* yn, float* mean,
                      float* rstd, void* stream);
/* diagnostic build of the C = 96 fused kernels with s_memtime stamps around the segments of a loop iteration
 * (devtools/mlp_fused_stamps.py); dbg: 8 uint64 per wave.  W2p: pack(w2) forward, pack(w2, trans) backward. */
int sea_mlp_fused_stamps(int bwd, const float* g, int64_t ldg, const float* x, int64_t ldx, const void* W1p, const float* b1,
                         const void* W2p, const void* W1tp, const float* b2, const float* res, float* y, int M, int C,
                         const uint32_t* amax_x, const uint32_t* amax_h, const float* amax_mul_dev, unsigned long long* dbg,
                         void* stream);
int sea_mlp_fused_fwd(const float* x, int64_t ldx, const void* W1p, const float* b1, const void* W2p, const float* b2,
                      const float* res, int64_t ldres, float* y, int64_t ldy, int M, int C, int H, const uint32_t* amax_x,
                      const uint32_t* amax_h, void* stream);
int sea_mlp_fused_bwd(const float* g, int64_t ldg, const float* x, int64_t ldx, const void* W1p, const float* b1,
                      const void* W2tp, const void* W1tp, float* dx, int64_t lddx, int M, int C, int H,
                      const uint32_t* amax_x, const float* amax_mul_dev, void* stream);
/* ------------------------------------------------------------------------------------------------
 * Measurement probes (bench.py / tools/kernel_bench.py only; nothing on the product path calls them).
 * sea_probe_stream_copy: dst[0:bytes] = src[0:bytes] with 16-byte-per-lane accesses (non_temporal != 0: nt loads and
 *   stores): the HBM copy ceiling the roofline fractions are also quoted against ("report against a
 *   measured stream ceiling on the box").  sea_probe_stream_read: read-only stream (sink: >= 2048 floats, untouched).
 * bytes % 16 == 0, 16-byte aligned pointers. */
int sea_probe_stream_copy(const void* src, void* dst, size_t bytes, int non_temporal, void* stream);
int sea_probe_stream_read(const void* src, float* sink, size_t bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * K10 multi-scale + flip evaluation (semseg.val.evaluate_msf), replacing the per-(scale, flip) ATen sequence of
 * semseg/val.py:340-365: interpolate(images, align_corners=True) [+ flip] -> model -> [flip] -> interpolate(logits,
 * (H, W), align_corners=True) -> softmax(dim=1) -> scaled_logits +=.
 * sea_msf_resize_input: x (planes, h, w) -> y and/or y_flip (planes, H, W), bilinear align_corners=True (ATen's fp32
 *   arithmetic); y_flip is the same image mirrored along W.  Either output may be NULL, not both.  Up or down.
 * sea_msf_accumulate: score (B, C, H, W) += softmax over C of the align_corners=True resize to (H, W) of the logits of
 *   one scaled forward, mirrored back along W when flip != 0.  logits (B, C, hl, wl): hl == Hs and wl == Ws = the model's
 *   output at the scaled size (Hs, Ws); smaller = its forward_lowres output, up-sampled to (Hs, Ws) on the fly with
 *   M2's align_corners=False rule (the scaled-size logits are never written).  C <= SEA_MSF_MAX_CLASSES, hl <= Hs,
 *   wl <= Ws, H*W and Hs*Ws < 2^31.  No atomics: bitwise reproducible.  score must not alias logits. */
#define SEA_MSF_MAX_CLASSES 192
int sea_msf_resize_input(const float* x, float* y, float* y_flip, int64_t planes, int h, int w, int H, int W,
                         void* stream);
int sea_msf_accumulate(const float* logits, float* score, int B, int C, int hl, int wl, int Hs, int Ws, int H, int W,
                       int flip, void* stream);

/* ------------------------------------------------------------------------------------------------
 * K11 sliding-window evaluation (semseg.utils.segmenter_eval), replacing merge_windows of
 * semseg/utils/segmenter_eval.py:51-92: logit[:, ha:ha+ws, wa:wa+ws] += window and count += 1 over the windows,
 * logit / count, interpolate(ori_shape, bilinear, align_corners=False), [flip along W], softmax(dim=0).
 * sea_sw_merge: logits (B * n_h * n_w, C, hl, wl), image-major (window ih * n_w + iw of image b is row
 *   b * n_h * n_w + ih * n_w + iw); window (ih, iw) covers rows h_anchors[ih] .. + ws and columns w_anchors[iw] .. + ws
 *   of the merged (H, W) image.  hl == ws and wl == ws: the model's output for the window; smaller: its forward_lowres
 *   output, up-sampled to (ws, ws) on the fly at the window-local coordinate with M2's align_corners=False rule and
 *   rounding (the window logits are never written).  Per merged pixel the covering windows' values are added in fp32
 *   from 0.f, h anchor outer, w anchor inner, and divided by their number: the reference's operations in its order.
 *   softmax == 0: out (B, C, H, W) = the averaged logits (flip and accumulate must be 0).
 *   softmax != 0: out = (accumulate ? out : 0) + softmax over C of the averaged logits, output column x taking merged
 *   column W-1-x when flip != 0; the averaged logits are never written.
 *   h_anchors[n_h], w_anchors[n_w]: HOST arrays, copied into the kernel arguments (no device allocation); on each axis
 *   1 .. SEA_SW_MAX_ANCHORS anchors, strictly ascending, the first 0, the last n - ws, consecutive ones at most ws apart.
 *   C <= SEA_MSF_MAX_CLASSES, hl <= ws, wl <= ws, H*W < 2^31, B * n_h * n_w <= 65535.  out must not alias logits.
 * sea_sw_finish: score (B, C, Ho, Wo) = (accumulate ? score : 0) + softmax over C of the align_corners=False bilinear
 *   resize (ATen's rule, up or down) of avg (B, C, H, W), mirrored along W when flip != 0: the tail of merge_windows for
 *   an original size that differs from the merged one.  score must not alias avg.
 * No atomics: both are bitwise reproducible. */
#define SEA_SW_MAX_ANCHORS 32
int sea_sw_merge(const float* logits, float* out, int B, int C, int hl, int wl, int ws, const int* h_anchors, int n_h,
                 const int* w_anchors, int n_w, int H, int W, int flip, int softmax, int accumulate, void* stream);
int sea_sw_finish(const float* avg, float* score, int B, int C, int H, int W, int Ho, int Wo, int flip, int accumulate,
                  void* stream);

/* The attack through the windows (semseg.utils.segmenter_eval.SlidingWindowModel): the cut of the windows and the
 * adjoints of cut and merge.  Anchors, limits and checks as for sea_sw_merge; all are gathers with one lane per output
 * element and a fixed summation order: no atomics, bitwise reproducible.
 * sea_sw_cut (K11c, semseg/utils/segmenter_eval.py:51-67, sliding_window): crops (B * n_h * n_w, Cx, ws, ws), image-major,
 *   window ih * n_w + iw = x[b, :, h_anchors[ih] .. + ws, w_anchors[iw] .. + ws] of x (B, Cx, H, W): a copy, the bits of
 *   the stack of slices.
 * sea_sw_cut_bwd (K11c', the adjoint of segmenter_eval.py:51-67): dx[b, c, y, x] = the fp32 sum, from 0.f, of
 *   dcrops[b, k, c, y - ha, x - wa] over the windows k that cover (y, x), h anchor outer, w anchor inner.
 * sea_sw_merge_bwd (K11a', the adjoint of segmenter_eval.py:70-83 = sea_sw_merge with softmax == 0): g (B, C, H, W) is the
 *   gradient of the averaged logits, dlogits (B * n_h * n_w, C, hl, wl) that of the window logits.
 *   hl == ws and wl == ws: dlogits[b, k, c, i, j] = g[b, c, ha + i, wa + j] / (float)count(ha + i, wa + j), one correctly
 *   rounded division (autograd through the reference's logit / count).
 *   smaller: the adjoint of the in-kernel M2 up-sampling, with the forward's taps and weights, applied to g / count
 *   restricted to the window; every low-resolution element adds its window pixels row-major (a row's sum, then the rows).
 *   Neither g / count nor a (B * n_h * n_w, C, ws, ws) gradient is written.  This mode keeps a table of the window's
 *   columns in LDS (8 bytes per column, padded; at most 48 KB): ws up to about 3000, beyond that hipErrorInvalidValue.
 *   dlogits must not alias g. */
int sea_sw_cut(const float* x, float* crops, int B, int Cx, int ws, const int* h_anchors, int n_h, const int* w_anchors,
               int n_w, int H, int W, void* stream);
int sea_sw_cut_bwd(const float* dcrops, float* dx, int B, int Cx, int ws, const int* h_anchors, int n_h,
                   const int* w_anchors, int n_w, int H, int W, void* stream);
int sea_sw_merge_bwd(const float* g, float* dlogits, int B, int C, int hl, int wl, int ws, const int* h_anchors, int n_h,
                     const int* w_anchors, int n_w, int H, int W, void* stream);

/* ------------------------------------------------------------------------------------------------
 * P1-P3: PSPNet-ResNet50 (semseg/models/ddcat_psp.py:372-486 with backbones/resnet_ddcat.py), the steps of its frozen
 * eval forward / input gradient that are not convolutions.  All fp32.
 * sea_psp_polyphase_split: x dense NHWC (B, H, W, C) -> y (B*P, ceil(H/d), ceil(W/d), C), P = d*d (first_only: P = 1,
 *   phase (0, 0) only), y[b*P + py*d + px][m][n] = x[b][py + d m][px + d n], 0 where that lies outside x.  Replaces the
 *   dilated 3x3 convolutions of layer3 / layer4 (ddcat_psp.py:429-438: dilation 2 / 4, padding = dilation) by ordinary
 *   3x3 convolutions of the sub-images (the zero tails are the zero padding), and, first_only with d = 2, the stride-2
 *   sampling of layer2's 1x1 downsample (resnet_ddcat.py:149-156).
 * sea_psp_polyphase_merge: the inverse on the valid positions (tails cropped) = the adjoint of the split; with
 *   first_only, x is zero off the phase-(0, 0) grid.  C % 4 == 0, 16-byte aligned, x != y.
 * sea_psp_upsample_ac: F.interpolate(x, (H, W), mode="bilinear", align_corners=True) of planes (h, w) -> (H, W), NCHW,
 *   ATen's arithmetic and evaluation order (the final logits, ddcat_psp.py:466-467).
 * sea_psp_upsample_ac_bwd: its input gradient by a two-pass separable gather (work: planes*H*w floats), no atomics.
 * sea_psp_upsample_ac_nhwc / _bwd: the same for a dense NHWC (B, h, w, C) input and an output (or output gradient) with
 *   pixel stride S >= C: a channel slice of the PPM's concatenation (ddcat_psp.py:23-30).  work: B*H*w*C floats.
 * sea_psp_add_relu: y = max(a + r, 0) (the bottleneck's out += residual; relu(out), resnet_ddcat.py:102-105).
 * sea_psp_add_relu_bwd: gx = y > 0 ? gy : 0 (the gradient of both a and r).  n % 4 == 0, 16-byte aligned. */
int sea_psp_polyphase_split(const float* x, float* y, int B, int H, int W, int C, int d, int first_only, void* stream);
int sea_psp_polyphase_merge(const float* y, float* x, int B, int H, int W, int C, int d, int first_only, void* stream);
int sea_psp_upsample_ac(const float* x, float* y, int64_t planes, int h, int w, int H, int W, void* stream);
int sea_psp_upsample_ac_bwd(const float* gy, float* gx, float* work, int64_t planes, int h, int w, int H, int W,
                            void* stream);
int sea_psp_upsample_ac_nhwc(const float* x, float* y, int B, int C, int h, int w, int H, int W, int S, void* stream);
int sea_psp_upsample_ac_nhwc_bwd(const float* gy, float* gx, float* work, int B, int C, int h, int w, int H, int W,
                                 int S, void* stream);
int sea_psp_add_relu(const float* a, const float* r, float* y, int64_t n, void* stream);
int sea_psp_add_relu_bwd(const float* gy, const float* y, float* gx, int64_t n, void* stream);

/* ------------------------------------------------------------------------------------------------
 * P4: the stem of PSPNet(clean=False), the torchvision-style ResNet-50 stem that takes an ImageNet-pre-trained backbone
 * (backbones/resnet_ddcat.py:115-131: conv1 = Conv2d(3, 64, 7, stride 2, padding 3, bias=False), bn1, relu, maxpool =
 * MaxPool2d(3, 2, 1); ddcat_psp.py:396-419: layer0 = Sequential(conv1, bn1, relu, maxpool)), for frozen parameters.  fp32
 * FMA in a fixed order, no atomics: bitwise repeatable.  Finite inputs; any H, W >= 1.
 * Hc = (H-1)/2 + 1, Hp = (Hc-1)/2 + 1 (W alike).
 * sea_psp_stem_fwd: out = maxpool3x3s2p1(relu(scale[c] * conv7x7s2p3(x, w)[c] + shift[c])) in ONE launch; the pre-pool
 *   map is never written.  x (B, 3, H, W) NCHW, w (64, 3, 7, 7), scale / shift (64): the folded eval BatchNorm, out
 *   (B, Hp, Wp, 64) NHWC.  rec, if not NULL: (B, Hp, Wp, 64) bytes, the window position ky*3 + kx (0-8) of the largest
 *   pre-activation, the first in row-major order among the positions inside the map (torch's choice), or 15 where that
 *   value is <= 0 (out is 0 there and no gradient passes).  Every element of out / rec is written.
 * sea_psp_stem_bwd: dx (B, 3, H, W) NCHW, the input gradient, as a gather: a pre-pool position belongs to at most 2 x 2
 *   pool windows; its gradient is the sum (rows outer, columns inner) of dout of those whose rec names it, times scale[c];
 *   dx is the transposed 7x7 stride-2 convolution of that.  Every element of dx is written (no zero-fill needed).
 *   Replaces the backward of the same four modules and what they keep for it (the pre-pool map, ATen's int64 indices). */
int sea_psp_stem_fwd(const float* x, const float* w, const float* scale, const float* shift, float* out,
                     unsigned char* rec, int B, int H, int W, void* stream);
int sea_psp_stem_bwd(const float* dout, const unsigned char* rec, const float* w, const float* scale, float* dx, int B,
                     int H, int W, void* stream);

/* ------------------------------------------------------------------------------------------------
 * P5: the dilated 3x3 branches of DeepLabV3's ASPP (ddcat_psp.py:44-58: Conv2d(in, out, 3, padding=rate, dilation=rate,
 * bias=False), BatchNorm, ReLU; ddcat_psp.py:69-81: their concatenation) for frozen parameters, as "product first, shift
 * second": Z = X . W_all^T on the un-shifted map (one M8 product; row (9 r + t) Cb + c of W_all = BatchNorm scale[c] *
 * weight_r[c][:][ky][kx], t = 3 ky + kx), then a 9-tap gather of Cb-channel rows.  fp32 NHWC rows, 64-bit element
 * offsets, one float4 per lane, no atomics: bitwise repeatable.
 * Every tensor is (B, H, W, .) rows with its own pixel stride ld (a multiple of 4) and first column col0 (a multiple of
 * 4) behind a 16-byte aligned base; R branches (1 <= R <= 4), rates[r] >= 1 (host array of R ints, read during the
 * call), Cb % 4 == 0.  Z's columns [z_col0, z_col0 + 9 R Cb) and Y's [y_col0, y_col0 + R Cb) must lie inside a pixel.
 * sea_aspp_tap_sum: Y[b][y][x][y_col0 + r Cb + c] = max(acc + shift[r Cb + c], 0) with acc = 0.f, then, for t = 0 .. 8
 *   in that order, acc += Z[b][y + (ky-1) rate_r][x + (kx-1) rate_r][z_col0 + (9 r + t) Cb + c]; a tap whose source
 *   pixel lies outside the map is skipped.  shift: R Cb floats (the folded BatchNorm shift).  Compiled without
 *   contraction: the bits are those of the written-out sum.  Nothing outside Y's R Cb columns is written.
 * sea_aspp_tap_sum_backward: dZ[b][y'][x'][z_col0 + (9 r + t) Cb + c] = Y[q] > 0 ? dY[q] : 0 at q = (y' - (ky-1) rate_r,
 *   x' - (kx-1) rate_r), 0 where q lies outside the map: a gather that writes every element of dZ's 9 R Cb columns
 *   exactly once, zeros included.  y: the forward's saved output (the ReLU gate, as sea_psp_add_relu_bwd). */
int sea_aspp_tap_sum(const float* z, int64_t ldz, int64_t z_col0, const float* shift, float* y, int64_t ldy,
                     int64_t y_col0, int B, int H, int W, int R, int Cb, const int* rates, void* stream);
int sea_aspp_tap_sum_backward(const float* dy, int64_t lddy, int64_t dy_col0, const float* y, int64_t ldy,
                              int64_t y_col0, float* dz, int64_t ldz, int64_t z_col0, int B, int H, int W, int R, int Cb,
                              const int* rates, void* stream);

/* ------------------------------------------------------------------------------------------------
 * T1: train-mode BatchNorm2d of PSPNet-ResNet50's PIR-AT outer step (the reference trains every nn.BatchNorm2d of
 * backbones/resnet_ddcat.py and ddcat_psp.py on batch statistics: tools/train_rob_seg.py:338-340), fused with the ReLU or
 * residual-add + ReLU that follows it (resnet_ddcat.py:97-105; ddcat_psp.py:21, 441-446).  fp32, x dense NHWC = an
 * (M, C) row-major matrix, M = B*H*W >= 2 rows, C % 4 == 0, every pointer 16-byte aligned.  No float atomics: the
 * results are bitwise reproducible.
 * sea_bn_train_workspace_floats: the floats of `work` that both calls below need for (M, C); -1 if unsupported.
 * sea_bn_train_fwd: torch.nn.functional.batch_norm(x, running_mean, running_var, gamma, beta, training=True, momentum,
 *   eps): mean and biased variance over the M rows (fixed-order two-stage Welford / Chan reduction), invstd =
 *   1/sqrt(var + eps), scale = gamma*invstd (all three written, C floats each), then y = (x - mean)*scale + beta
 *   [+ r] [ReLU] (r: NULL or an (M, C) residual; relu: 0 / 1).  running_mean <- (1-momentum)*
 *   running_mean + momentum*mean, running_var <- (1-momentum)*running_var + momentum*var*M/(M-1) and
 *   *num_batches_tracked += 1, as torch's _BatchNorm does with a float momentum; each of the three may be NULL (no update).
 * sea_bn_train_bwd: the gradient of sea_bn_train_fwd from dL/dy g: g' = relu ? (y > 0 ? g : 0) : g (y: the saved
 *   output), dbeta = sum g', dgamma = sum g'*xhat with xhat = (x - mean)*invstd, dx = scale*(g' - dbeta/M -
 *   xhat*dgamma/M), as torch's batch_norm_backward with training=True.  gr (the residual variant, relu = 1 only): g', the
 *   gradient of r; NULL otherwise.  mean / invstd / scale: the forward's outputs. */
int64_t sea_bn_train_workspace_floats(int64_t M, int C);
int sea_bn_train_fwd(const float* x, const float* r, const float* gamma, const float* beta, float* y, float* mean,
                     float* invstd, float* scale, float* running_mean, float* running_var, int64_t* num_batches_tracked,
                     float* work, int64_t M, int C, float eps, float momentum, int relu, void* stream);
int sea_bn_train_bwd(const float* g, const float* x, const float* y, const float* mean, const float* invstd,
                     const float* scale, float* dx, float* dgamma, float* dbeta, float* gr, float* work, int64_t M, int C,
                     int relu, void* stream);

/* ------------------------------------------------------------------------------------------------
 * T2: the training criteria of the PIR-AT outer step, CrossEntropy and OhemCrossEntropy of the reference's
 * semseg/losses.py:6-63, forward + hard-pixel selection + backward on the device.  logits: dense NCHW (B, C, H*W),
 * SEA_DTYPE_F32 or SEA_DTYPE_BF16; y: int64 labels (B, H*W) as the data loader hands them over; ignore_label: any
 * integer; w: C class weights or NULL.  A label outside [0, C) other than ignore_label is treated as ignored and sets
 * the error word.  B*H*W < 2^31.  No float atomics: bitwise reproducible.  Nothing is read by the host.
 * `words`: 64 bytes of device memory, ZEROED by the caller before sea_train_ce_fwd, 8-byte aligned:
 *   double sum_sel, sum_w, sum_loss; float loss, coef; uint32 t_bits; int32 take, n_sel, n_valid, n_hard, n_min, mode,
 *   err  (loss: the criterion's value; coef: 1/sum_w or 1/n_sel; mode: 0 threshold, 1 top-k; semseg/losses.py:48-55).
 * sea_train_ce_workspace_bytes: bytes of `workspace` (16-byte aligned) that the calls below need.
 * sea_train_ce_fwd: per pixel w[y]*(lse - z_y), 0 where ignored, into loss_px (B*H*W floats); per-block records
 *   {sum loss, sum w[y], sum of losses > thresh, n_valid, n_hard}, then their fixed-order sum in double.  reduce_mean
 *   = 1 (nn.CrossEntropyLoss, losses.py:15-19): loss = sum loss / sum w[y].  reduce_mean = 0 (losses.py:48-52): n_min =
 *   n_valid / 16 and the regime; in threshold mode (n_hard >= n_min) also the final words.
 * sea_train_ohem_select (after sea_train_ce_fwd with reduce_mean = 0, same workspace and words): in top-k mode the
 *   n_min-th largest loss t by a radix select over the float bits (four byte-histogram passes), the sum of the losses
 *   above t plus `take` ties at t (taken in ascending flat pixel index), the words (losses.py:53-55); in both modes the
 *   loss of every pixel that is not selected is overwritten with -1 in loss_px.  n_sel = 0 gives loss = NaN.
 * sea_train_ce_bwd: dlogits = g[0] * coef * w[y] * (softmax(z) - onehot(y)) at valid (ohem = 1: selected) pixels, 0
 *   elsewhere, in the logits' dtype; g: the upstream gradient, one float in device memory. */
size_t sea_train_ce_workspace_bytes(int B, int64_t HW);
int sea_train_ce_fwd(const void* logits, int dtype, const int64_t* y, const float* w, int64_t ignore_label, float thresh,
                     int reduce_mean, int B, int C, int64_t HW, float* loss_px, void* workspace, size_t workspace_bytes,
                     void* words, void* stream);
int sea_train_ohem_select(float* loss_px, int64_t N, void* workspace, size_t workspace_bytes, void* words, void* stream);
int sea_train_ce_bwd(const void* logits, int dtype, const int64_t* y, const float* w, int64_t ignore_label, int ohem,
                     int B, int C, int64_t HW, const float* loss_px, const float* g, const void* words, void* dlogits,
                     void* stream);

/* ------------------------------------------------------------------------------------------------
 * T2u: T2 fused with the model's final bilinear up-sampling.  Replaces, for one prediction of UperNet's training
 * forward, F.interpolate(low, (H, W), mode="bilinear", align_corners=False) + the criterion + both backward passes:
 * the (B, C, H, W) logits, their log-soft-max and their gradients are never materialised.
 * low: dense NCHW fp32 (B, C, h, w), 2 <= C <= 192; y: int64 labels (B, H, W), H >= h, W >= w, any ratio up to 28 per
 * axis (power of two or not); wgt: C class weights or NULL.  Outside these limits every entry point returns the argument
 * error (workspace_bytes: 0) and launches nothing; the caller then up-samples and calls T2.  B*H*W < 2^31.
 * Interpolation: ATen's upsample_bilinear2d, align_corners = 0: src = max(r*(dst+0.5)-0.5, 0), i1 = min(i0+1, n-1).
 * Everything else is T2's: labels, `words` (the same 64 bytes, ZEROED by the caller before the forward), the loss plane
 * loss_px (B*H*W floats at FULL resolution), the records summed in a fixed order in double, reduce_mean, thresh.
 * Nothing is read by the host; no float atomics: bitwise reproducible.
 * sea_train_ce_up_tile: edge TL of the low-resolution tile one workgroup owns for this shape (0: no plan).  A
 *   workgroup owns the loss of the full-resolution pixels whose top-left source pixel lies in its tile and the gradient
 *   of the tile; it recomputes the statistics of the one-cell halo of full-resolution pixels around it.
 * sea_train_ce_up_workspace_bytes: bytes of `workspace` (16-byte aligned); laid out as T2's, so that
 *   sea_train_ohem_select runs UNCHANGED on loss_px (N = B*H*W) with the same workspace and words after
 *   sea_train_ce_up_fwd with reduce_mean = 0.
 * sea_train_ce_up_fwd: per full-resolution pixel w[y]*(lse(z) - z_y) of the interpolated logits z, 0 where ignored, into
 *   loss_px; then the words as sea_train_ce_fwd.
 * sea_train_ce_up_bwd: dlow[b,c,i,j] = g[0] * coef * sum over the valid (ohem = 1: selected, loss_px != -1) pixels whose
 *   bilinear footprint touches (i, j) of weight * w[y] * (softmax(z)_c - [c == y]); a gather with one owner per element
 *   of dlow, summed cell by cell, row by row in double.  Every element of dlow is written.  workspace: unused by the
 *   gather (may be NULL). */
int sea_train_ce_up_tile(int C, int h, int w, int H, int W);
size_t sea_train_ce_up_workspace_bytes(int B, int C, int h, int w, int H, int W);
int sea_train_ce_up_fwd(const float* low, const int64_t* y, const float* wgt, int64_t ignore_label, float thresh,
                        int reduce_mean, int B, int C, int h, int w, int H, int W, float* loss_px, void* workspace,
                        size_t workspace_bytes, void* words, void* stream);
int sea_train_ce_up_bwd(const float* low, const int64_t* y, const float* wgt, int64_t ignore_label, int ohem, int B, int C,
                        int h, int w, int H, int W, const float* loss_px, const float* g, const void* words, float* dlow,
                        void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * T2u-ac: sea_train_ce_up_tile / _workspace_bytes / _fwd / _bwd with the interpolation of
 * F.interpolate(low, (H, W), mode="bilinear", align_corners=True), PSPNet's final up-sampling (ddcat_psp.py:467, 474).
 * Per axis: scale = (n_in - 1) / (n_out - 1) in float (0 for n_out == 1), src = scale * dst, i0 = (int)src,
 * i1 = i0 + (i0 < n_in - 1), lam = src - i0; the four values are combined with the fused multiply-adds of
 * sea_psp_upsample_ac (bitwise the tensor P2 would write).  Arguments, labels, words, loss plane, workspace layout,
 * ownership, summation order and reproducibility are those of the align_corners = 0 entry points above, and
 * sea_train_ohem_select runs unchanged after sea_train_ce_up_ac_fwd with reduce_mean = 0.  No plan (tile and
 * workspace_bytes 0, fwd / bwd the argument error): C outside 2..192, H < h or W < w, or no tile edge whose region fits
 * 72 pixels per axis and 64 KB of LDS (a ratio (n_out - 1) / (n_in - 1) above 34; n_in == 1, where the region is the
 * whole axis, with n_out above about 60); the caller then runs sea_psp_upsample_ac and T2. */
int sea_train_ce_up_ac_tile(int C, int h, int w, int H, int W);
size_t sea_train_ce_up_ac_workspace_bytes(int B, int C, int h, int w, int H, int W);
int sea_train_ce_up_ac_fwd(const float* low, const int64_t* y, const float* wgt, int64_t ignore_label, float thresh,
                           int reduce_mean, int B, int C, int h, int w, int H, int W, float* loss_px, void* workspace,
                           size_t workspace_bytes, void* words, void* stream);
int sea_train_ce_up_ac_bwd(const float* low, const int64_t* y, const float* wgt, int64_t ignore_label, int ohem, int B,
                           int C, int h, int w, int H, int W, const float* loss_px, const float* g, const void* words,
                           float* dlow, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * T2u for power-of-two ratios (csrc/train_loss_up_pow2.hip): nn.CrossEntropyLoss(weight, ignore_index, reduction="mean")
 * on F.interpolate(low, (H, W), mode="bilinear", align_corners=False), loss AND un-normalised gradient in ONE pass.
 * Replaces, per prediction, uperforseg.py:416-434 (main head x4, auxiliary head x16) and segmenter.py:228 +
 * train_rob_seg.py:346-347 (Segmenter's masks x16, then the criterion), with their backward passes.
 * Applies when H = r*h and W = r*w with r = 4 or r = 16 on both axes, low dense NCHW fp32 (B, C, h, w), 2 <= C <= 192,
 * h, w >= 1; y: int64 labels (B, H, W); wgt: C class weights or NULL; B*H*W < 2^31.  OHEM has no such kernel (its
 * selection needs every loss before any gradient): it keeps sea_train_ce_up_fwd / _bwd.
 * With mean reduction d loss / d low = g * (1 / sum w[y]) * raw, raw[b,c,i,j] = sum over the valid pixels whose bilinear
 * footprint touches (i, j) of weight * w[y] * (softmax(z)_c - [c == y]): the forward writes raw (B*C*h*w DOUBLES, every
 * element: the gradient is rounded to float once, by the scale pass), the backward is one scale pass.  No full-resolution plane of any kind is written.  Labels, `words` (the same
 * 64 bytes, ZEROED by the caller) and the edge cases are T2's: a label outside [0, C) other than ignore_label is ignored
 * and sets words.err; every label ignored gives loss = NaN, coef = inf and raw = 0.  Nothing is read by the host; no float
 * atomics; raw[b] depends on image b alone, bit for bit.  A refused call returns the argument error and writes nothing.
 * sea_train_ce_up_pow2_supported (host only): 1 if the shape is one of the above, else 0.
 * sea_train_ce_up_pow2_workspace_bytes: bytes of `workspace` (16-byte aligned: per-wave records and partial gradient
 *   vectors, 2*(h+1)*(w + segments)*C doubles per image); 0 if unsupported.
 * sea_train_ce_up_pow2_fwd: raw and the words as sea_train_ce_fwd with reduce_mean = 1 writes them.
 * sea_train_ce_up_pow2_scale: dlow[i] = (g[0] / words.sum_w) * raw[i] for i < n, the product in double and rounded once,
 *   and exactly 0 where raw[i] is 0 (so that a batch with every label ignored gets zeros, not 0 * inf); g: one float in
 *   device memory. */
int sea_train_ce_up_pow2_supported(int C, int h, int w, int H, int W);
size_t sea_train_ce_up_pow2_workspace_bytes(int B, int C, int h, int w, int H, int W);
int sea_train_ce_up_pow2_fwd(const float* low, const int64_t* y, const float* wgt, int64_t ignore_label, int B, int C,
                             int h, int w, int H, int W, double* raw, void* workspace, size_t workspace_bytes, void* words,
                             void* stream);
int sea_train_ce_up_pow2_scale(const double* raw, const float* g, const void* words, float* dlow, int64_t n, void* stream);

/* ------------------------------------------------------------------------------------------------
 * The attack through multi-scale + flip (semseg.utils.msf_model.MsfModel): the adjoints of K10 (csrc/msf_grad.hip).
 * Gathers with one lane per output element and a fixed summation order: no atomics, bitwise reproducible.  Every index
 * and weight is the forward's (the same device functions).
 * sea_msf_resize_bwd (K10r', the adjoint of sea_msf_resize_input = of the interpolate(images, align_corners=True)
 *   [+ flip] of semseg/val.py:340-365): g and / or g_flip (planes, H, W), the gradients of y and y_flip, -> dsrc
 *   (planes, h, w), the gradient of x.  Either may be NULL, not both.  Per source element, fp32 from 0.f:
 *   acc += (wy * wx) * g[p, Y, X] over the destination pixels (Y, X) whose forward map references it, Y ascending, then
 *   X ascending, row tap 0 before row tap 1, column tap 0 before column tap 1 (a clamped border pixel contributes both
 *   of its terms); all terms of g first, then those of g_flip (read at column W-1-X) in the same order.  An element
 *   that no destination references gets 0.  src_flip != 0: the mirror is on the SOURCE columns instead (element
 *   (i, c) collects the terms of map column w-1-c), as in sea_msf_accumulate with flip.  Up or down.  h*w and
 *   H*W < 2^31.  dsrc must alias neither gradient.
 * sea_msf_accumulate_bwd (K10g + K10r', the adjoint of sea_msf_accumulate with respect to the logits): dscore
 *   (B, C, H, W) is the gradient of score.  K10g recomputes per pixel the resized logits v and p = softmax(v) exactly
 *   as sea_msf_accumulate (both modes, flip) and writes G = p * (dscore - sum_c p_c dscore_c) into the workspace G
 *   (B, C, H, W); K10r' (src_flip = flip) then writes dscaled (B, C, Hs, Ws), the gradient on the scaled grid.  hl == Hs
 *   and wl == Ws: dscaled is the gradient of the logits.  Smaller (forward_lowres logits): the caller follows with
 *   sea_upsample_bilinear_bwd down to (hl, wl).  Limits as sea_msf_accumulate; the four buffers must not alias. */
int sea_msf_resize_bwd(const float* g, const float* g_flip, float* dsrc, int64_t planes, int h, int w, int H, int W,
                       int src_flip, void* stream);
int sea_msf_accumulate_bwd(const float* logits, const float* dscore, float* G, float* dscaled, int B, int C, int hl,
                           int wl, int Hs, int Ws, int H, int W, int flip, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SEA_HIP_H */
