/*
 * geeco_hip.h -- C ABI of the MI355X (gfx950) kernels behind GEECO's e2evmc training hot path.
 *
 * The reference (ogroth/geeco) has no FFI: every op below replaces a stock TensorFlow-1.15 op that
 * the reference's Python graph instantiates.  Each entry point cites the reference call site it
 * replaces (paths relative to the reference root).  INTEGRATION.md shows the ctypes binding.
 *
 * Conventions
 *   - all tensors are float32, device pointers, NHWC activations, HWIO conv kernels (TF layout);
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream); every call only enqueues
 *     work on that stream: no allocation, no synchronisation, no host<->device copies, so a caller
 *     may capture a sequence of calls into a hipGraph;
 *   - return value: 0 on success, a negative GEECO_E* code on bad arguments, or a positive
 *     hipError_t if the launch failed; geeco_last_error() gives a thread-local message;
 *   - "groups" let one launch serve several independent instances with identical shapes (the
 *     three encoders of geeco-f): instance g uses ptr + g * group_stride (strides in elements).
 */
#ifndef GEECO_HIP_H_
#define GEECO_HIP_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GEECO_ABI_VERSION 7  /* = the build round that last changed the entry points or their calling conventions */
/* added within 7 (additive: no existing entry point or convention changed): geeco_lstm_seq_heads_fwd,
 * geeco_pack_frames_by_address, geeco_window_states_fwd, geeco_window_states_bwd, geeco_gather_windows_by_address,
 * geeco_gather_windows_augmented, geeco_adam_tf_ema, geeco_adam_tf_segments_ema, geeco_clip_ws_floats,
 * geeco_grad_sumsq_segments, geeco_clip_scale, geeco_adam_tf_segments_clip, geeco_gather_windows_scene,
 * geeco_adam_prepare_schedule, geeco_slab_reduce_batch_prepare_schedule, geeco_lr_schedule_eval, geeco_guard_decide,
 * geeco_adam_tf_segments_guard, geeco_adam_tf_segments_scaled, geeco_variable_stats_ws_bytes, geeco_variable_stats,
 * geeco_heads_loss_shaped_fwd_bwd, geeco_lstm_step_heads_shaped_fwd_bwd, geeco_loss_shaping_sizeof,
 * geeco_grad_accumulate_segments, geeco_conv1_dgrad, geeco_pack_pixels_bwd, geeco_dynimg_bwd_ws_bytes, geeco_dynimg_bwd,
 * geeco_gather_windows_frames, geeco_replay_states, geeco_replay_errors, geeco_attr_path_point, geeco_attr_accumulate,
 * geeco_attr_finish, geeco_replay_images_ws_bytes, geeco_replay_images, geeco_replay_states_pair, geeco_perturb_desc_sizeof,
 * geeco_perturb_patch, geeco_perturb_apply, geeco_perturb_score, geeco_perturb_accumulate, geeco_perturb_finish */

#define GEECO_EINVAL  (-1)   /* bad shape / alignment / null pointer */
#define GEECO_ENOSUP  (-2)   /* shape outside what the kernels were built for */

int geeco_abi_version(void);
const char* geeco_last_error(void);
/* Always 0.  The library has one build (csrc/build.sh) holding only the kernels the measured-best path launches; it reads no
 * environment variable.  The development build that returned 1 and its switches were retired (scripts/dev/SWITCHES.md);
 * the entry point stays for ABI compatibility. */
int geeco_has_dev_kernels(void);

/* Diagnostics (bench.py's per-layer table): between _begin and _end on one host thread every
 * conv entry point records the names of the kernels it dispatched; _end returns them ';'-separated
 * (thread-local buffer, valid until the next _begin on that thread). */
void geeco_debug_kernel_trace_begin(void);
const char* geeco_debug_kernel_trace_end(void);

/* ---- dynamic image: src/models/e2evmc/graph.py:30-55 (dynimg), :17-28 (_H/_alpha) -------------
 * frames [N][K][H][W][C] (or, when frame_stride/sample_stride are given, any strided stack of
 * HWC frames) -> out [N][H][W][Cpad] = (D - min_n) / (max_n - min_n + 1e-6), D = sum_t alpha_t X_t.
 * Channels C..Cpad-1 of `out` are written as zero (Cpad is 4 for RGB so conv1 reads float4 pixels).
 * `alpha` is a HOST pointer to K coefficients (geeco_dynimg_alpha fills it).
 * `ws` is a device workspace of geeco_dynimg_ws_bytes(N, H*W*C) bytes.
 * Two-frame form (dyndiff, graph.py:397-400): pass K = 2, frames = cur, frames2 = tgt,
 * frame_stride ignored; otherwise frames2 = NULL. */
void geeco_dynimg_alpha(int K, float* alpha_host);
int64_t geeco_dynimg_ws_bytes(int N, int64_t hwc);
int geeco_dynimg_fwd(const float* frames, const float* frames2, int64_t sample_stride,
                     int64_t frame_stride, const float* alpha_host, int N, int K, int64_t HW,
                     int C, int Cpad, float* out, void* ws, void* stream);

/* RGB-D form of geeco_dynimg_fwd without packing: `rgb` [N][K][HW][3] and `depth` [N][K][HW] stay separate tensors
 * (each with its own sample / frame strides, 16-byte aligned, HW % 4 == 0) and tf.concat([rgb, depth], -1)
 * (estimator.py:169,172) happens in registers; out [N][HW][4] normalised over all four channels (graph.py:47-54).
 * Two-frame form: K = 2, rgb2 / depth2 = the second frame ([N][HW][3], [N][HW]). */
int geeco_dynimg_rgbd_fwd(const float* rgb, const float* rgb2, int64_t sample_stride, int64_t frame_stride,
                          const float* depth, const float* depth2, int64_t dsample_stride, int64_t dframe_stride,
                          const float* alpha_host, int N, int K, int64_t HW, float* out, void* ws, void* stream);
/* All three conv1 inputs of the goal model's dynimg branch (graph.py:386-401) in ONE launch and one pass over the window:
 * buf_out = dynimg of the K-frame stack, diff_out = dynimg of (last frame, target) with the 2-frame coefficients alpha2,
 * cur_out = the last frame channel-padded.  Both images stay in registers across their per-sample min / max (the blocks of
 * a sample meet at a per-sample arrival counter in `ws`) and are stored once, normalised; bitwise the images of
 * geeco_dynimg_fwd / geeco_dynimg_rgbd_fwd.  depth / tgt_depth NULL: RGB ((R, G, B, 0) pixels), else RGB-D from separate
 * tensors.  HW % 4 == 0, 16-byte aligned strides.
 * ws: geeco_goal_dynimgs_ws_bytes(N, HW) bytes that the caller ZERO-FILLS ONCE (per-sample arrival counters, which every call
 * finds and leaves zero, + per-block min / max slots); calls that share a `ws` must be stream-ordered. */
int64_t geeco_goal_dynimgs_ws_bytes(int N, int64_t HW);
int geeco_goal_dynimgs_fwd(const float* rgb, int64_t sample_stride, int64_t frame_stride, const float* tgt_rgb,
                           const float* depth, int64_t dsample_stride, int64_t dframe_stride, const float* tgt_depth,
                           const float* alpha_host, const float* alpha2_host, int N, int K, int64_t HW, float* cur_out,
                           float* buf_out, float* diff_out, void* ws, void* stream);
/* The blocks of a sample wait for each other (bounded: seconds).  A wait that expires -- only if the device did not start the
 * blocks of a launch in index order, see csrc/dynimg_goal.hip -- is never silent: that sample's two images are written as NaN (never
 * with stale min / max; NB a ReLU turns NaN into 0, so the loss behind them can be finite) and the block counts itself into a
 * sticky per-sample word in `ws`.  This entry sums those words
 * over the N samples into *count_host (0 = every image ever produced through this ws was normalised with its sample's true
 * min / max).  It copies N x 64 bytes to the host and SYNCHRONISES `stream`: call it where the host waits for the device
 * anyway (loss read-out, end of an epoch; the reference reads its loss in the same places, estimator.py:263-269).  A workspace
 * that has seen a timeout must be zero-filled again before its next use. */
int geeco_goal_dynimgs_timeouts(const void* ws, int N, void* stream, int64_t* count_host);
/* Process-wide number of polls a block waits before it reports (default 2^22); returns the previous value.  0 makes every block
 * that is not the last of its sample to arrive report at once -- the tests provoke the error path with it. */
unsigned geeco_goal_dynimgs_set_wait_polls(unsigned polls);
/* The same stage read straight from the episodes' resident uint8 frames: replaces the host-side window + division of the
 * reference's input pipeline (_window_v3, src/data/geeco_gym.py:615-631; rgb / 255.0, _parse_v4 :312) AND the fp32 window
 * tensor they produce.  win_ptrs_dev / tgt_ptrs_dev: DEVICE arrays of N addresses; window n = K consecutive [HW][3] uint8
 * frames starting at win_ptrs_dev[n] (4-byte aligned), its target frame [HW][3] uint8 at tgt_ptrs_dev[n].  The tables are
 * read when the kernel RUNS, so a captured graph follows the host repointing them between replays; the frames they point
 * at must stay allocated until that run has finished.  depth / tgt_depth: dense float32 [N][K][HW] / [N][HW] or NULL.
 * Outputs are bitwise those of geeco_gather_windows(divisor 255) followed by geeco_goal_dynimgs_fwd. */
int geeco_goal_dynimgs_u8_fwd(const void* const* win_ptrs_dev, const void* const* tgt_ptrs_dev, const float* depth,
                              int64_t dsample_stride, int64_t dframe_stride, const float* tgt_depth, const float* alpha_host,
                              const float* alpha2_host, int N, int K, int64_t HW, float* cur_out, float* buf_out,
                              float* diff_out, void* ws, void* stream);


/* Copy [npix][C] -> [npix][Cpad] (zero-filled tail).  Used for the "current frame" view
 * rgb[:, -1] (graph.py:387) and for RGB||depth concat (estimator.py:169,172) via src2. */
int geeco_pack_pixels(const float* src, int64_t src_sample_stride, const float* src2,
                      int64_t src2_sample_stride, int N, int64_t HW, int C1, int C2, int Cpad,
                      float* dst, void* stream);

/* On-device window builder (replaces the host-side _window_v3 of src/data/geeco_gym.py:615-631):
 * out[n][k][:] = float(src[starts_dev[n] + k][:]) / divisor.  `src` = an episode's frames resident in
 * HBM ([T][frame_elems], uint8 if src_is_u8 else float32); `starts_dev` = N int32 frame indices on the
 * device; divisor 255 reproduces `rgb /= 255.0` (geeco_gym.py:312) bit-exactly, 1 copies. */
int geeco_gather_windows(const void* src, int src_is_u8, const int* starts_dev, int N, int K,
                         int64_t frame_elems, float divisor, float* out, void* stream);
/* The same builder driven by a table, ONE launch for windows of any episode, order or frame kind (a batch of shuffled windows,
 * input_fn.pickplace_input_fn(shuffle_windows=True); the reference shuffles samples on the host, dataset.shuffle,
 * src/data/geeco_gym.py:701-703): addr [N] int64 and kind [N] int32 on the device, read when the kernel RUNS (they may ride in
 * the step's host-to-device block, queued in front of this call).  out[n][k][:] = conv(frame k of the K consecutive frames at
 * addr[n]); kind[n] = 0: uint8 frames, conv(u8) = float(u8) / 255.0f with the IEEE division, bitwise geeco_gather_windows
 * (divisor 255); kind[n] = 1: float32 frames, a copy (any other value is read as 0).  Windows may repeat and overlap.
 * frame_elems >= 4 and % 4 == 0, out 16-byte aligned, N and K <= 65535.  A window whose address is not aligned for the vector
 * loads (4 bytes uint8, 16 float32; float32 frames are 4-byte aligned in any case) goes one element at a time. */
int geeco_gather_windows_by_address(const int64_t* addr, const int* kind, int N, int K, int64_t frame_elems, float* out,
                                    void* stream);
/* The by-address builder with a per-window image augmentation (input_fn.pickplace_input_fn(augment=...); the
 * reference has none).  addr / kind as above; frames are [H][W][C], C = 3 (RGB) or 1 (depth); shift [N][2] int32 = (dy, dx) in
 * whole pixels; colour [N][2 * C] float32 = gain[C], bias[C], or NULL.  All four tables live on the device and are read when
 * the kernel RUNS.  For every frame of window n:  out[n][k][y][x][c] = tint(v), v = conv(source pixel (y - dy, x - dx), channel
 * c) as geeco_gather_windows_by_address converts it, tint(v) = min(max(v * gain[c] + bias[c], 0), 1) (the multiply-add may be
 * fused), tint = identity when colour is NULL;  exactly 0.0f where the source pixel lies outside [0, H) x [0, W) (not tinted).
 * Any int32 shift is valid: every source index is tested against the frame before it is read, |dy| >= H or |dx| >= W gives
 * zeros.  Shift (0, 0) without colour is bitwise geeco_gather_windows_by_address.  H * W * C < 2^31, out 16-byte aligned,
 * N and K <= 65535.  W * C % 4 == 0: 16-byte stores, loads as wide as the shifted source's address allows; else one element at
 * a time. */
int geeco_gather_windows_augmented(const int64_t* addr, const int32_t* kind, const int32_t* shift, const float* colour, int N,
                                   int K, int H, int W, int C, float* out, void* stream);
/* The augmented builder of an RGB stream (C must be 3) with occluders and sensor noise behind the gather
 * (input_fn.pickplace_input_fn(augment=dict(noise=, occlude=))).  addr / kind / shift / colour, the argument checks and
 * the launch shape as above.  Per element, in this order:  v1 = what geeco_gather_windows_augmented writes, bitwise;  v2 = the
 * colour component of the highest-numbered rectangle of window n that holds the element's OUTPUT pixel (y, x), else v1:
 * occ_rect [N][4][4] int32 = (y0, x0, h, w) per slot, a slot with h <= 0 or w <= 0 is empty, occ_colour [N][4][3] float32 = its
 * RGB; both NULL: no occluders.  Any int32 content is valid (containment is overflow-free, no address is formed from it); the
 * rectangles serve all K frames and paint over the zero border.  out = min(max(fma(sigma, z, v2), 0), 1), z standard normal from
 * Philox4x32-10 under the key noise_key[0..1] (two uint32 words on the device, read when the kernel RUNS; may be NULL only when
 * sigma == 0) and the counter (e / 4, k, n, tag), e = the element's offset in its frame: the four output words give the normals
 * of elements 4g .. 4g + 3 by Box-Muller (words 0, 1 -> the first two, words 2, 3 -> the last two), so z depends on (key, tag,
 * n, k, e) alone.  tag: 0 for 'rgb', 1 for 'target_rgb'.  0 <= sigma < 1; sigma == 0 skips the noise step (no clamp), and with
 * NULL occluders too the output is bitwise geeco_gather_windows_augmented. */
int geeco_gather_windows_scene(const int64_t* addr, const int32_t* kind, const int32_t* shift, const float* colour,
                               const int32_t* occ_rect, const float* occ_colour, const uint32_t* noise_key, float sigma, int tag,
                               int N, int K, int H, int W, int C, float* out, void* stream);
/* The scene builder following one address PER FRAME (camera frame drops and latency: input_fn.pickplace_input_fn(augment=dict(
 * frame_drop=, frame_lag=)); the reference has none).  frame_addr [N][K] int64 on the device, read when the kernel
 * RUNS (a captured step follows a re-pointed table): out[n][k] is built from the frame of kind[n] at frame_addr[n][k]; frames may
 * repeat within and between windows.  Every other argument, the argument checks and the launch shape as above, except: shift may
 * be NULL (no shift), and C = 1 (depth) is taken with shift and colour only (occ_rect, occ_colour NULL and sigma == 0), as
 * geeco_gather_windows_augmented takes it.  Per element the output is bitwise what geeco_gather_windows_scene writes for a window
 * whose k-th frame is that frame; with the scene arguments NULL / sigma == 0 bitwise geeco_gather_windows_augmented; with shift and
 * colour NULL too bitwise geeco_gather_windows_by_address.  The noise counter stays (e / 4, k, n, tag) with k the OUTPUT slot: a
 * frame shown in two slots gets independent sensor noise in each.  Alignment is decided per frame, never per window: uint8 frames
 * may lie at any byte address (frames of H * W * C % 4 != 0 bytes put neighbours at different residues), float32 frames at any
 * 4-byte aligned one; loads are as wide as each element's own source address allows.  The caller guarantees that every table
 * entry addresses H * W * C readable elements of kind[n]. */
int geeco_gather_windows_frames(const int64_t* frame_addr, const int32_t* kind, const int32_t* shift_or_null,
                                const float* colour_or_null, const int32_t* occ_rect_or_null, const float* occ_colour_or_null,
                                const uint32_t* noise_key_or_null, float sigma, int tag, int N, int K, int H, int W, int C,
                                float* out, void* stream);

/* ---- batched predictor I/O: B control loops per call (reference predictor.py:127-209 per env) ----------------------
 * The ingest and output stages of one replayed graph (geeco_amd/batched_predictor.py): range check -> window push ->
 * forward -> pack.  `ctl` = B + 1 int32 control words on the device: ctl[b] = 1 when env b's frame failed the range check,
 * ctl[B] = 1 when any did.  The range check only sets them, the pushes do nothing while ctl[B] is set (no env's window moves),
 * and geeco_predict_pack copies them to ctl_out and zeroes them for the next call.  K: 1..64; C: 3 (RGB) or 4 (RGB-D). */
/* Channels 0..2 of every env's new frame ([B][HW][C] float32) inside [lo, hi] (predictor.py:135-138; NaN fails). */
int geeco_predict_range_check(const float* frames, int B, int64_t HW, int C, float lo, float hi, int* ctl, void* stream);
/* Dense window push, in place: rgb [B][K][HW][3], depth [B][K][HW] (C == 4; split out of the [HW][4] frame), jnt_state
 * [B][K][J].  reset[b] != 0: all K slots get the new frame (predictor.py:197-198), else slots shift down by one and slot K-1
 * gets it (:144-146).  frames: [B][HW][C] float32, or uint8 when frames_u8 (C == 3; divided by 255 bitwise as
 * geeco_gather_windows(divisor 255)). */
int geeco_predict_push_dense(const void* frames, int frames_u8, const float* jnt, const int* reset, const int* any_bad,
                             int B, int K, int64_t HW, int C, int J, float* rgb, float* depth, float* jnt_state, void* stream);
/* Ring window push for uint8 RGB frames: ring [B][2K][HW * 3] bytes, mirrored (a frame goes to slots p and p + K), so an env's
 * window is always K contiguous frames; win_table[b] (int64, device) gets its start address, the input kernel of the model
 * (geeco_goal_dynimgs_u8_fwd) reads it when it runs.  heads [B] int32 on the device: the next slot of each env, advanced by
 * the launch itself (a replayed graph moves on by itself).  HW % 4 == 0.  jnt_state [B][K][J] is pushed densely. */
int geeco_predict_push_ring(const unsigned char* frames, const float* jnt, const int* reset, const int* any_bad, int B, int K,
                            int64_t HW, int J, unsigned char* ring, int* heads, int64_t* win_table, float* jnt_state,
                            void* stream);
/* Output pack (predictor.py:157-189): preds [B][P] -> out [B][F].  Segment s copies seg_len[s] columns from seg_src[s], or,
 * when seg_argmax[s], writes ONE column argmax - 1 over those logits (first maximum on ties, as np.argmax).  img0 / img1
 * (may be NULL): [B][HW][4] channel-padded images -> img_out [nimg][B][HW][C] (dynbuff / dyndiff endpoints).  The seg_*
 * arrays are host memory, nseg <= GEECO_PREDICT_PACK_MAXSEG. */
#define GEECO_PREDICT_PACK_MAXSEG 8
int geeco_predict_pack(const float* preds, int P, int B, int nseg, const int* seg_src, const int* seg_len, const int* seg_argmax,
                       float* out, int F, int* ctl, int* ctl_out, const float* img0, const float* img1, int64_t HW, int C,
                       float* img_out, void* stream);

/* ---- incremental predictor: per-frame encoder features cached on the device (batched_predictor.py, incremental=True) ----
 * The per-frame controllers (e2e_vmc; goal_e2evmc 'sequence' x 'constant' / 'residual') encode only the B new frames of a call;
 * the features of the K - 1 older frames of every window wait in a ring. */
/* Newest-frame input pack: frames [B][HW][C] (float32, or uint8 when frames_u8: C == 3, divided by 255 bitwise as
 * geeco_predict_push_dense does) -> the encoder input x_in [B][HW][4]; channel 3 = depth (C == 4) or 0. */
int geeco_predict_pack_newest(const void* frames, int frames_u8, int B, int64_t HW, int C, float* x_in, void* stream);
/* Feature push + state gather, one launch.  feat [B][cells][ch]: the encoder's features of the new frames; jnt [B][J].  On the
 * device: feat_ring [B][K][cells][ch], jnt_ring [B][K][J], heads [B] int32 (zero-filled once) = the slot of each env's next
 * frame, advanced by the launch itself.  reset[b] != 0: all K slots of env b get the new feature / joint state
 * (predictor.py:192-200), else slot heads[b] does.  Then states[t][b] ([K][B][state_stride]) is written for t = 0..K-1, oldest
 * frame first, with the columns of geeco_state_concat_fwd per cell: PLAIN [feat | jnt] (jnt_pos 1), CONSTANT [feat | jnt | tgt]
 * (jnt_pos 1, two maps), RESIDUAL [tgt - feat | jnt] (sub_from); tgt_feat [B][cells][ch] (NULL for PLAIN).  Nothing moves and
 * nothing is written while *any_bad is set.  K: 1..64. */
#define GEECO_PREDICT_FEAT_PLAIN 0
#define GEECO_PREDICT_FEAT_CONSTANT 1
#define GEECO_PREDICT_FEAT_RESIDUAL 2
int geeco_predict_push_features(const float* feat, const float* jnt, const int* reset, const int* any_bad, const float* tgt_feat,
                                int mode, int B, int K, int cells, int ch, int J, float* feat_ring, float* jnt_ring, int* heads,
                                float* states, int64_t state_stride, void* stream);

/* ---- shared-frame training of the per-frame controllers (graph.py: E2EVMC / GoalE2EVMC with shared_frames=F) ----
 * A batch of consecutive windows holds each frame up to K times; conv_encoder sees one frame at a time, so the step encodes a
 * table of F frame SLOTS once and the windows index it.  All three entries only enqueue on `stream`; none uses atomics. */
/* table [F] int64 (device): the address of each slot's resident RGB frame ([HW][3]; uint8 when frames_u8, else float32), 0 = an
 * unused slot.  x_in [F][HW][4] <- the frame with a zero fourth channel (uint8: float(u8) / 255.0f with the IEEE division, bitwise
 * the conversion of geeco_gather_windows / geeco_predict_pack_newest), zeros for an unused slot.  A frame whose address is not
 * aligned for the 4-pixel path (4 bytes uint8, 16 float32), or HW % 4 != 0, goes one pixel at a time. */
int geeco_pack_frames_by_address(const int64_t* table, int F, int frames_u8, int64_t HW, float* x_in, void* stream);
/* feat [F][cells][ch], idx [N][K] int32 (window position -> slot), jnt [N][K][J], tgt_idx [N] int32 (slot of window n's target
 * frame; NULL for PLAIN) -> states [K][N][state_stride], ONE launch for all K steps, with the columns geeco_state_concat_fwd
 * gives per cell: GEECO_PREDICT_FEAT_PLAIN [feat | jnt], _CONSTANT [feat | jnt | tgt], _RESIDUAL [tgt - feat | jnt].  N * K <= 1024.
 * An index outside [0, F) contributes zeros. */
int geeco_window_states_fwd(const float* feat, const int* idx, const float* jnt, const int* tgt_idx, int mode, int F, int N, int K,
                            int cells, int ch, int J, float* states, int64_t state_stride, void* stream);
/* The adjoint: dfeat[f] = sum over the positions (n, t) with idx[n][t] == f of the feature columns of dstates[t][n] (sign -1 in
 * RESIDUAL) + sum over the windows n with tgt_idx[n] == f and their K steps of the target columns; one block per slot, summed
 * in ONE fixed order (positions ascending n then t, then the target windows ascending n, t), so two launches are bitwise equal.
 * feat: the forward's features; the sum is masked by feat > 0 (ReluGrad of the encoder's last layer, as
 * geeco_state_concat_bwd).  Slots nobody references get exact zeros. */
int geeco_window_states_bwd(const float* dstates, int64_t state_stride, const float* feat, const int* idx, const int* tgt_idx,
                            int mode, int F, int N, int K, int cells, int ch, int J, float* dfeat, void* stream);

/* ---- conv encoder: graph.py:76-115 (tf.layers.conv2d 3x3, padding='SAME', bias, ReLU) ----------
 * x [G][N][H][W][Cin], w [G][3][3][Cin][Cout] (HWIO), b [G][Cout], y [G][N][Ho][Wo][Cout],
 * Ho = ceil(H/stride); TF SAME padding (pad_before = pad_total/2, i.e. 0 top/left for stride 2 on
 * even sizes).  Requires Cin % 4 == 0, Cout % 16 == 0. */
int geeco_conv3x3_fwd(const float* x, const float* w, const float* b, float* y, int groups,
                      int64_t gs_x, int64_t gs_w, int64_t gs_b, int64_t gs_y, int N, int H, int W,
                      int Cin, int Cout, int stride, int relu, void* ws, void* stream);
/* The encoders' TOP layer (conv8 + bias + ReLU, all `groups` encoders over the same N frames) together with the one-step
 * decoder's state concat (representation_concatenation_v2, graph.py:169-192; jnt_state_list[-1], :388): the launch that sums
 * the split-K slabs also writes state[n][cell * Ctot + feat_off[g] + c] = y[g][n][cell][c] and copies jnt[n][0..J) into the
 * columns [jnt_off, jnt_off + J) of every cell -- the values of geeco_conv3x3_fwd + geeco_state_concat_fwd, one dependent launch
 * fewer.  Returns GEECO_ENOSUP, having launched nothing, when the shape does not take the split-K path (ws NULL, no split for
 * this M, a halo-kernel shape): the caller then runs the two entry points. */
int geeco_conv3x3_fwd_state(const float* x, const float* w, const float* b, float* y, int groups, int64_t gs_x, int64_t gs_w,
                            int64_t gs_b, int64_t gs_y, int N, int H, int W, int Cin, int Cout, int stride, void* ws,
                            const int* feat_off, int Ctot, const float* jnt, int64_t jnt_stride, int jnt_off, int J,
                            float* state, int64_t state_stride, void* stream);

/* `ws` (may be NULL): device workspace of geeco_conv3x3_fwd_ws_bytes(...) bytes; layers whose
 * output is too small to fill 256 CUs (conv6..8) split their K loop over blocks through it. */
int64_t geeco_conv3x3_fwd_ws_bytes(int groups, int N, int H, int W, int Cin, int Cout, int stride);

/* Conv2DBackpropInput fused with the ReluGrad of the layer below (autodiff of graph.py:76-115 via
 * estimator.py:243-244):  dx = conv3x3_transpose(dz, w) * (ymask > 0).
 * dz [G][N][Ho][Wo][Cout], wt [G][3][3][Cout][Cin] (= geeco_transpose_hwio(w)), w (optional) the
 * HWIO kernel itself: the LDS-halo kernel of the 32->48 stride-2 layer reads it directly,
 * ymask [G][N][H][W][Cin] = forward output of the layer below (NULL: no mask), dx like ymask.
 * stride 1 or 2; all stride*stride parity classes run in one launch; `ws` as for the forward. */
int geeco_conv3x3_dgrad(const float* dz, const float* w, const float* wt, const float* ymask,
                        float* dx, int groups, int64_t gs_dz, int64_t gs_w, int64_t gs_wt,
                        int64_t gs_dx, int N, int H, int W, int Cin, int Cout, int stride, void* ws,
                        void* stream);
int64_t geeco_conv3x3_dgrad_ws_bytes(int groups, int N, int H, int W, int Cin, int Cout, int stride);
/* 0 if geeco_conv3x3_dgrad, GIVEN the HWIO kernel `w`, runs a kernel that reads `w` itself for this shape (the LDS-staged
 * kernels, and the gather GEMM whenever Cout % 16 == 0: it transposes the kernel tile on its way into LDS); the caller then
 * need not keep the transposed copy `wt` up to date and may pass NULL for it.  1 if `wt` is read. */
int geeco_conv3x3_dgrad_needs_wt(int H, int W, int Cin, int Cout, int stride);
int geeco_conv3x3_dgrad_relu_fields_supported(int H, int W, int Cin, int Cout, int stride);

/* Conv2DBackpropFilter + BiasAddGrad:  dw[ky][kx][ci][co] = sum_m x[pix(m,ky,kx)][ci] dz[m][co],
 * db[co] = sum_m dz[m][co].  dw/db are OVERWRITTEN (not accumulated).
 * `ws`: device workspace of geeco_conv3x3_wgrad_ws_bytes(...) bytes (split-K partial slabs). */
int64_t geeco_conv3x3_wgrad_ws_bytes(int groups, int N, int H, int W, int Cin, int Cout, int stride);
int geeco_conv3x3_wgrad(const float* x, const float* dz, float* dw, float* db, int groups,
                        int64_t gs_x, int64_t gs_dz, int64_t gs_dw, int64_t gs_db, int N, int H,
                        int W, int Cin, int Cout, int stride, void* ws, void* stream);

/* Encoder bottom, backward, fused (autodiff of graph.py:76-85 via estimator.py:243-244): conv2's input gradient and
 * conv1's filter/bias gradient in one kernel - conv1's input is data, so dz1 = (y1 > 0) * conv2_dgrad(dz2) has a
 * single consumer and never has to reach HBM:
 *   dw1[g][3][3][real_channels][32], db1[g][32]  <-  x [G][N][H][W][4], dz1
 * real_channels = 3: x is RGB zero-padded to 4 channels; dw1 has the reference's own [3][3][3][32] layout (the pad
 * channel has no row); real_channels = 4: RGB-D, all four input channels are real.
 * dz2 [G][N][H/2][W/2][48], w2 [G][3][3][32][48] (HWIO), y1 [G][N][H][W][32] (conv1's output: the ReLU mask).
 * dz1 (optional, may be NULL): if given, dz1 is ALSO written ([G][N][H][W][32], group stride gs_y1).
 * Shapes are fixed to the reference encoder's conv1 (4 -> 32, stride 1) / conv2 (32 -> 48, stride 2); H, W even.
 * Equivalent to geeco_conv3x3_dgrad(conv2) followed by geeco_conv3x3_wgrad(conv1); dw1/db1 are OVERWRITTEN. */
int64_t geeco_conv2_dgrad_conv1_wgrad_ws_bytes(int groups);
int geeco_conv2_dgrad_conv1_wgrad(const float* dz2, const float* w2, const float* y1, const float* x,
                                  float* dw1, float* db1, float* dz1, int groups, int64_t gs_dz2,
                                  int64_t gs_w2, int64_t gs_y1, int64_t gs_x, int64_t gs_dw1,
                                  int64_t gs_db1, int N, int H, int W, int real_channels, void* ws,
                                  void* stream);

/* Deferred slab sums.  The filter-gradient kernels leave one partial slab per split in `ws` and finish with a small
 * slab-sum launch.  The *_partial forms skip that launch and describe it in *pending instead (pending->S == 0: the
 * kernel wrote dw/db itself, nothing is pending); geeco_slab_reduce_batch then finishes up to GEECO_SLAB_REDUCE_MAX
 * of them in ONE launch (a training step: one per part of the backward instead of one per layer).  The `ws` of a
 * pending item must stay untouched until the batch has run.  Results are bitwise those of the plain calls (same
 * summation order).
 * reserved_cus (0..128; the forms below and geeco_conv2_dgrad_conv1_wgrad_bits): data parallel -- the two persistent
 * one-block-per-CU kernels at the bottom of the backward (conv2's filter gradient, the fused conv2-dgrad + conv1-wgrad)
 * normally occupy every CU while the early gradient bucket is all-reduced beside them; k > 0 makes THIS launch leave k CUs
 * to the collective's workgroups ((256 - k) / groups blocks per encoder; workspaces are sized for k = 0 and fit any k; other
 * kernels ignore it).  A launch argument since ABI 4 (a process-wide setter before): nothing outlives the call.  The
 * reference has no counterpart (no distributed code: SURVEY.md 2). */
typedef struct geeco_slab_reduce {
  const float* part;      /* [groups][S][KC + Cout] partial slabs */
  float* dw;              /* [groups] x KC floats, group stride gs_dw */
  float* db;              /* [groups] x Cout floats, group stride gs_db (may be NULL) */
  int64_t gs_dw, gs_db, KC;
  int32_t S, Cout, groups, reserved;
} geeco_slab_reduce;
#define GEECO_SLAB_REDUCE_MAX 8
int geeco_conv3x3_wgrad_partial(const float* x, const float* dz, float* dw, float* db, int groups,
                                int64_t gs_x, int64_t gs_dz, int64_t gs_dw, int64_t gs_db, int N, int H,
                                int W, int Cin, int Cout, int stride, void* ws, void* stream,
                                geeco_slab_reduce* pending, int reserved_cus);
int geeco_conv2_dgrad_conv1_wgrad_partial(const float* dz2, const float* w2, const float* y1, const float* x,
                                          float* dw1, float* db1, float* dz1, int groups, int64_t gs_dz2,
                                          int64_t gs_w2, int64_t gs_y1, int64_t gs_x, int64_t gs_dw1,
                                          int64_t gs_db1, int N, int H, int W, int real_channels, void* ws,
                                          void* stream, geeco_slab_reduce* pending, int reserved_cus);
int geeco_slab_reduce_batch(const geeco_slab_reduce* items, int n, void* stream);
/* ... and, as one more block of the same launch, geeco_adam_prepare (below): the step counter and lr_t depend on nothing the
 * slab sums touch and only have to be in place before geeco_adam_tf -- the training step's last slab-sum launch carries them
 * instead of a dependent launch of their own.  n may be 0. */
int geeco_slab_reduce_batch_prepare(const geeco_slab_reduce* items, int n, int64_t* global_step_dev, float lr, float beta1,
                                    float beta2, float* scal_dev, void* stream);
/* TWO independent filter gradients of the 64 x 64-tile generic kernel as ONE grid (the model: conv7's + conv8's, both ready
 * once conv8's input gradient exists; problem 0 = the longer one).  Arguments per problem as geeco_conv3x3_wgrad; common
 * groups / stride; pending2: NULL or TWO items (deferred slab sums as geeco_conv3x3_wgrad_partial; S = 0 where the kernel wrote
 * the gradient directly).  Bitwise the results of two geeco_conv3x3_wgrad calls.  GEECO_ENOSUP for shapes outside the paired
 * kernel (Cin = 256, Cout % 64 == 0, stride 2): launch twice then. */
int geeco_conv3x3_wgrad_pair(const float* x0, const float* dz0, float* dw0, float* db0, int64_t gs_x0, int64_t gs_dz0,
                             int64_t gs_dw0, int64_t gs_db0, int N0, int H0, int W0, int Cin0, int Cout0, void* ws0,
                             const float* x1, const float* dz1, float* dw1, float* db1, int64_t gs_x1, int64_t gs_dz1,
                             int64_t gs_dw1, int64_t gs_db1, int N1, int H1, int W1, int Cin1, int Cout1, void* ws1,
                             int groups, int stride, void* stream, geeco_slab_reduce* pending2);
/* ... and with conv7's INPUT gradient beside them (all three need only dz7; each alone fills the 256 CUs badly): ONE
 * heterogeneous grid, the filter-gradient blocks first.  Leading arguments as geeco_conv3x3_dgrad (stride 2; ws = its split-K
 * workspace, required), then the two problems of geeco_conv3x3_wgrad_pair.  Bitwise the separate calls.  GEECO_ENOSUP when
 * any of the three is outside the kernels this launch combines (the gather GEMM's 64 x 64 x 16 tiles; the paired 64 x 64
 * filter-gradient tiles): nothing has been launched, use the separate entry points.  x1 == NULL: ONE filter gradient beside
 * the input gradient (the model: conv8's pair, then conv7's). */
int geeco_conv_top_bwd(const float* dz, const float* w, const float* wt, const float* ymask, float* dx, int64_t gs_dz,
                       int64_t gs_w, int64_t gs_wt, int64_t gs_dx, int N, int H, int W, int Cin, int Cout, void* ws,
                       const float* x0, const float* dz0, float* dw0, float* db0, int64_t gs_x0, int64_t gs_dz0,
                       int64_t gs_dw0, int64_t gs_db0, int N0, int H0, int W0, int Cin0, int Cout0, void* ws0,
                       const float* x1, const float* dz1, float* dw1, float* db1, int64_t gs_x1, int64_t gs_dz1,
                       int64_t gs_dw1, int64_t gs_db1, int N1, int H1, int W1, int Cin1, int Cout1, void* ws1,
                       int groups, int stride, void* stream, geeco_slab_reduce* pending2);

/* ReLU sign bits as the ReluGrad mask of the encoder bottom.  conv1's output y1 (805 MB at the bench shape) is read by
 * the fused bottom backward only for its sign; geeco_conv1_fwd_relu_bits is conv1's forward (4 -> 32, stride 1, bias,
 * ReLU: geeco_conv3x3_fwd on those shapes) that ALSO writes one uint32 per pixel,
 *   bits[g][n][y][x]: Hp = geeco_relu_bits_rows(H) rows of Wp = geeco_relu_bits_pitch(W) words per image (whole 8 x 64
 *   tiles), group stride gs_bits words; bit (c & 3) * 8 + (c >> 2) set iff y1[g][n][y][x][c] > 0.
 * Only the words of real pixels are written: the caller zero-fills the array ONCE, the backward relies on zero padding.
 * geeco_conv2_dgrad_conv1_wgrad_bits is geeco_conv2_dgrad_conv1_wgrad taking those words instead of y1 (no dz1
 * output; pending: NULL = finish the slab sum, else defer it as geeco_conv2_dgrad_conv1_wgrad_partial does). */
int64_t geeco_relu_bits_pitch(int W);
int64_t geeco_relu_bits_rows(int H);
int geeco_conv1_fwd_relu_bits(const float* x, const float* w, const float* b, float* y, uint32_t* bits, int groups,
                              int64_t gs_x, int64_t gs_w, int64_t gs_b, int64_t gs_y, int64_t gs_bits, int N, int H,
                              int W, void* stream);
/* ... with the RGB model's kernel variable w3 [G][3][3][3][32] as it is stored (x stays channel-padded; the pad channel's
 * kernel rows count as zero): bitwise the same y / bits as with the padded copy, which then need not be re-derived after
 * every optimiser step. */
int geeco_conv1_fwd_relu_bits_rgb(const float* x, const float* w3, const float* b, float* y, uint32_t* bits, int groups,
                                  int64_t gs_x, int64_t gs_w, int64_t gs_b, int64_t gs_y, int64_t gs_bits, int N, int H,
                                  int W, void* stream);
/* The same idea one layer up: conv2's forward (32 -> 48, stride 2, bias, ReLU; x [G][N][H][W][32]) that also writes the
 * sign fields of its output y2, and conv3's input gradient (48 -> 64, stride 2; dz [G][N][H/2][W/2][64], dx = d(y2)
 * [G][N][H][W][48]) masked by those fields instead of by y2 itself (302 MB at the bench shape).
 *   fields[g][n][y][x][q], q = 0..3: uint16, bit 4 i + j set iff y2[g][n][y][x][16 i + 4 q + j] > 0; rows / columns
 *   padded to whole 8 x 64 tiles (geeco_relu_fields_elems uint16 per encoder), group stride gs_fields elements.
 * reserved_cus (round 5): as for the two launches behind it in the data-parallel step (geeco_conv3x3_wgrad_partial): this persistent
 *   one-block-per-CU kernel is the first of part 2 and leaves that many CUs to the collective running beside it; 0 otherwise. */
int64_t geeco_relu_fields_elems(int N, int H, int W);
int geeco_conv2_fwd_relu_fields(const float* x, const float* w, const float* b, float* y, uint16_t* fields, int groups,
                                int64_t gs_x, int64_t gs_w, int64_t gs_b, int64_t gs_y, int64_t gs_fields, int N, int H,
                                int W, void* stream);
int geeco_conv3_dgrad_relu_fields(const float* dz, const float* w, const uint16_t* y2_fields, float* dx, int groups,
                                  int64_t gs_dz, int64_t gs_w, int64_t gs_fields, int64_t gs_dx, int N, int H, int W,
                                  void* stream, int reserved_cus);
/* ... and one more layer up: conv3's forward (48 -> 64, stride 2) writing byte sign fields of its output y3, and the
 * LDS-staged input-gradient kernel of the next layer (the shapes geeco_conv3x3_dgrad_relu_fields_supported reports,
 * e.g. conv4: 64 -> 128) masked by them instead of by y3 (100 MB at the bench shape):
 *   fields[g][n][y][x][Cin / 8] bytes: byte (T >> 1) * 4 + q, bit 4 (T & 1) + j set iff y[g][n][y][x][16 T + 4 q + j] > 0
 *   (T = 16-channel tile, q = channel quad inside it); group stride gs_fields bytes; no padding. */
int geeco_conv3_fwd_relu_fields(const float* x, const float* w, const float* b, float* y, uint8_t* fields, int groups,
                                int64_t gs_x, int64_t gs_w, int64_t gs_b, int64_t gs_y, int64_t gs_fields, int N, int H,
                                int W, void* stream);
int geeco_conv3x3_dgrad_relu_fields(const float* dz, const float* w, const uint8_t* y_fields, float* dx, int groups,
                                    int64_t gs_dz, int64_t gs_w, int64_t gs_fields, int64_t gs_dx, int N, int H, int W,
                                    int Cin, int Cout, int stride, void* stream);
int geeco_conv2_dgrad_conv1_wgrad_bits(const float* dz2, const float* w2, const uint32_t* y1_bits, const float* x,
                                       float* dw1, float* db1, int groups, int64_t gs_dz2, int64_t gs_w2,
                                       int64_t gs_bits, int64_t gs_x, int64_t gs_dw1, int64_t gs_db1, int N, int H, int W,
                                       int real_channels, void* ws, void* stream, geeco_slab_reduce* pending,
                                       int reserved_cus);

/* [G][9][A][B] -> [G][9][B][A] per-tap transpose (HWIO -> HWOI) feeding geeco_conv3x3_dgrad. */
int geeco_transpose_hwio(const float* w, float* wt, int groups, int64_t gs_w, int64_t gs_wt, int Cin,
                         int Cout, void* stream);

/* All derived weight copies of an encoder stack in one launch (the per-step chain after Adam):
 * for l < nlayers: wt[l] = geeco_transpose_hwio(w[l]) with (Cin[l], Cout[l]), group strides gs_w (kernels,
 * common) and gs_wt[l]; and, if pad_src/pad_dst are given, conv1's kernel [G][9][pad_Cin][pad_Cout]
 * (stride gs_w) zero-padded to [G][9][pad_Cin_padded][pad_Cout] (stride gs_pad) = geeco_pad_mid per group. */
int geeco_derive_conv_weights(int nlayers, const float* const* w, float* const* wt, const int* Cin,
                              const int* Cout, const int64_t* gs_wt, int groups, int64_t gs_w,
                              const float* pad_src, float* pad_dst, int pad_Cin, int pad_Cin_padded,
                              int pad_Cout, int64_t gs_pad, void* stream);

/* src [A][B][C] -> dst [A][Bd][C], copying min(B,Bd) middle rows and zero-filling the rest: pads
 * conv1's RGB kernel [9][3][Co] to [9][4][Co] and un-pads its gradient. */
int geeco_pad_mid(const float* src, float* dst, int64_t A, int B, int Bd, int C, void* stream);

/* ---- state concat: graph.py:123-192 (tile jnt 2x2, concat along channels, flatten) -------------
 * Builds state [N][cells*(sum Cf + J)] from up to 3 feature maps [N][cells][Cf_i] and jnt [N][J];
 * `jnt_pos` = number of feature maps placed BEFORE the joint block (1: state_concatenation and
 * representation_concatenation, 2: representation_concatenation_v2).  `sub_from` (optional,
 * graph.py:369 'residual'): feature 0 is written as sub_from - feat0.
 * jnt rows are read at jnt + n * jnt_stride. */
int geeco_state_concat_fwd(const float* const* feats, const int* feat_ch, int nfeat, int jnt_pos,
                           const float* jnt, int64_t jnt_stride, int J, const float* sub_from,
                           int N, int cells, float* state, int64_t state_stride, void* stream);
/* Scatter scale * d(state) back into d(feat_i), applying the ReLU mask of the encoder's last layer
 * (feats_fwd_i > 0).  dfeats[i] may be NULL to skip.  accumulate != 0 adds into dfeats.  The
 * 'residual' target mode (graph.py:369: tgt_feat - feat) calls it with scale = -1 for feat and once
 * more with feats_fwd = tgt_feat, scale = +1, accumulate over the window. */
int geeco_state_concat_bwd(const float* dstate, int64_t dstate_stride, const float* const* feats_fwd,
                           float* const* dfeats, const int* feat_ch, int nfeat, int jnt_pos, int J,
                           int N, int cells, int accumulate, float scale, void* stream);

/* ---- dense GEMM used by the LSTM gate matmul and its backward (graph.py:217-225) ---------------
 * C[M][N] (ldc) = op(A) op(B) (+ C if accumulate).  ta/tb: 0 = as stored, 1 = transposed.
 * A is [M][K] (lda) or, if ta, [K][M]; B is [K][N] (ldb) or, if tb, [N][K].
 * `ws`: geeco_gemm_ws_bytes(M,N,K) bytes (split-K slabs). */
int64_t geeco_gemm_ws_bytes(int M, int N, int K);
int geeco_gemm_f32(const float* A, int64_t lda, int ta, const float* B, int64_t ldb, int tb, float* C,
                   int64_t ldc, int M, int N, int K, int accumulate, void* ws, void* stream);

/* ---- LSTM cell: tf.nn.rnn_cell.LSTMCell(num_units=H, state_is_tuple=False), graph.py:217-225 ----
 * z [N][4H] = [x|h_prev] W (from geeco_gemm_f32), gate order i, j, f, o, forget_bias 1.0:
 *   c = sigmoid(f + 1) c_prev + sigmoid(i) tanh(j);  h = sigmoid(o) tanh(c).
 * `gates` [N][4H] receives the activated gates (si, tj, sf, so) for the backward pass.
 * c_prev may be NULL (zero state, graph.py:218-220). */
int geeco_lstm_gates_fwd(const float* z, const float* bias, const float* c_prev, float* c, float* h,
                         float* gates, int N, int H, void* stream);
/* The FIRST step of the cell (zero state, graph.py:218-220: z = x wx alone) as two launches instead of three: the gate GEMM
 * (geeco_gemm_f32's kernel and K split) and the gate math with the split-K slab sum inside it.  x [N][D] (ldx), wx [D][4H]
 * (ldw); z, c, h, gates as geeco_lstm_gates_fwd; ws: geeco_gemm_ws_bytes(N, 4H, D).  Bitwise equal to geeco_gemm_f32 +
 * geeco_lstm_gates_fwd(c_prev = NULL). */
int geeco_lstm_input_step_fwd(const float* x, int64_t ldx, const float* wx, int64_t ldw, const float* bias, float* z, float* c,
                              float* h, float* gates, int N, int H, int D, void* ws, void* stream);
/* dz [N][4H] from dh, dc (either may be NULL = 0); dc_prev (optional) out. */
int geeco_lstm_gates_bwd(const float* gates, const float* c_prev, const float* c, const float* dh,
                         const float* dc, float* dz, float* dc_prev, int N, int H, void* stream);
/* TWO launches for everything a single LSTM step's backward needs after the gate gradients dz [N][4H] (the goal model's
 * dynimg branch runs one step: graph.py:405-407; autodiff of :217-225 + :169-192): dwx [D][4H] = x^T dz, db [4H] = column
 * sums of dz, dx [N][D] = dz wx^T and - if nfeat > 0 - the state-concat backward of dx (geeco_state_concat_bwd with
 * scale 1, accumulate 0: dfeats[i][n][cell][c] = (feats_fwd[i] > 0) * dx[n][cell * Ctot + off_i + c]).  Grid 1: the
 * tiles of dwx, the split-K tiles of dx and the column sums side by side; grid 2: dx's slab sum with the scatter in its
 * epilogue.  Replaces the five launches geeco_gemm_f32 (ta) + geeco_colsum + geeco_gemm_f32 (tb: split-K + reduce) +
 * geeco_state_concat_bwd.  dx: same K / slab order as geeco_gemm_f32, bitwise the same for every N.  dwx: ONE K loop over
 * the N rows (no split), bitwise equal to geeco_gemm_f32 where that does not split K either, i.e. N < 128 (the batch sizes
 * of the reference: params.py:26); for N >= 128 geeco_gemm_f32 splits the batch dimension and the two differ in rounding
 * (tests/test_kernels_gpu.py: tolerance there, bitwise below).  ws: geeco_lstm_step_bwd_ws_bytes bytes.
 * `pending` (may be NULL): the batch sums geeco_lstm_step_heads_fwd_bwd left behind (weight / bias gradients of fc1 and the
 * heads, loss means); they run as the first blocks of grid 1, beside the tiles of dwx / dx. */
typedef struct geeco_heads_finish { unsigned char opaque[1024]; } geeco_heads_finish;    /* filled and read by the library only */
int64_t geeco_lstm_step_bwd_ws_bytes(int N, int D, int H4);
int geeco_lstm_step_bwd(const float* x, int64_t ldx, const float* dz, int64_t ldz, const float* wx, int64_t ldw, float* dwx,
                        int64_t lddw, float* db, float* dx, int64_t lddx, int N, int D, int H4,
                        const float* const* feats_fwd, float* const* dfeats, const int* feat_ch, int nfeat, int jnt_pos,
                        int J, int cells, void* ws, const geeco_heads_finish* pending, void* stream);
/* column sums: out[j] = sum_i a[i][j] (bias gradients). */
int geeco_colsum(const float* a, int64_t lda, int M, int N, float* out, int accumulate, void* stream);

/* ---- fc1 + heads + losses, forward and backward ------------------------------------------------
 * graph.py:229-259 (fc1 ReLU, linear heads), :430-500 (losses), estimator.py:206-239 (targets,
 * loss composition).  `nheads` <= 5 linear heads [Hfc][size_i] are described by parallel arrays:
 *   head_kind 0: tf.losses.mean_squared_error against target rows (size_i floats at
 *                targets[i] + n * target_stride[i]);
 *   head_kind 1: softmax cross-entropy against one_hot(rint(targets[i][n * stride]) + 1)
 *                (the gripper command, estimator.py:213-215);
 *   loss = sum_i head_weight[i] * L_i (cartesian: 1, 1, lambda_aux, lambda_aux; velocity: all 1),
 *   every L_i a mean over the LOCAL batch N; gradients are scaled by `loss_scale`.
 * Cartesian mode heads: pred_cmd_ee (MSE vs cmd[:, :3]), logits_cmd_grp (CE vs cmd[:, 3]),
 * pred_aux_ee, pred_aux_obj (MSE vs features[...][:, -1, :3]).
 * Outputs: preds [N][sum size_i], losses[1 + nheads] = {total, L_0, ...} (unscaled local means); when
 * `backward` != 0 also dh [N][H] and d_fc1_w, d_fc1_b, d_heads_w[i], d_heads_b[i] (overwritten).
 * Two launches (round 5): one workgroup PER SAMPLE for everything that is independent per sample (fc1, heads, loss terms, and
 * back to dh), then a few blocks for what sums over the batch (weight / bias gradients, loss means; sums over n ascending).
 * H <= 128 and Hfc in {64, 128}; other sizes run a single-workgroup kernel.  N <= 4096, sum size_i <= 32. */
int geeco_heads_loss_fwd_bwd(const float* h, const float* fc1_w, const float* fc1_b, int nheads,
                             const float* const* heads_w, const float* const* heads_b,
                             const int* head_size, const int* head_kind, const float* head_weight,
                             const float* const* targets, const int64_t* target_stride,
                             float loss_scale, int N, int H, int Hfc, float* preds, float* losses,
                             int backward, float* dh, float* d_fc1_w, float* d_fc1_b,
                             float* const* d_heads_w, float* const* d_heads_b, float* ws, void* stream);
int64_t geeco_heads_ws_bytes(int N, int H, int Hfc);
/* The decoder of the models that run ONE LSTM step from the zero state (goal model, dynimg branch: graph.py:405-407, 217-260):
 * geeco_lstm_input_step_fwd + geeco_heads_loss_fwd_bwd + (backward) geeco_lstm_gates_bwd as TWO launches: the gate GEMM
 * (x [N][D] wx [D][4H], split-K slabs in gemm_ws), then one workgroup per sample that sums its slabs, runs the gate math
 * (z, c, h, gates written as geeco_lstm_input_step_fwd does), fc1, the heads and the loss terms and -- `backward` != 0 -- returns
 * through d(h) to the gate gradients dz [N][4H] (no dh output: nothing else reads it).  Arguments as the three entry points.
 * `pending` NULL: the batch sums (loss means; weight / bias gradients) run here as a third small launch; non-NULL: they are
 * described in *pending and geeco_lstm_step_bwd runs them inside its own first grid -- losses and the heads' / fc1's
 * gradients are valid only after that call.  GEECO_ENOSUP (nothing launched) outside H <= 128, Hfc in {64, 128}. */
int geeco_lstm_step_heads_fwd_bwd(const float* x, int64_t ldx, const float* wx, int64_t ldw, const float* bias, float* z,
                                  float* c, float* h, float* gates, int N, int H, int D, void* gemm_ws, const float* fc1_w,
                                  const float* fc1_b, int nheads, const float* const* heads_w, const float* const* heads_b,
                                  const int* head_size, const int* head_kind, const float* head_weight,
                                  const float* const* targets, const int64_t* target_stride, float loss_scale, int Hfc,
                                  float* preds, float* losses, int backward, float* dz, float* d_fc1_w, float* d_fc1_b,
                                  float* const* d_heads_w, float* const* d_heads_b, float* heads_ws,
                                  geeco_heads_finish* pending, void* stream);

/* ---- loss shaping: the optional arguments of the tf.losses calls above (TF 1.15: weights=, label_smoothing=,
 * tf.losses.huber_loss(delta=)), reduction SUM_BY_NONZERO_WEIGHTS.  The shaped entry points take the arguments of the entry
 * points they extend plus a geeco_loss_shaping (host struct, read during the call; its pointers are DEVICE pointers that the
 * kernels read when they RUN, so a captured graph follows new weights in the same buffers), and allow
 *   head_kind 2: tf.losses.huber_loss against target rows, delta = huber_delta[i] (finite, > 0):
 *                l = 0.5 q^2 + delta (|e| - q), q = min(|e|, delta), e = pred - target.
 * Effective weight of sample n: sample_weight[n * sample_weight_stride] (NULL: 1) for every head, times
 * class_weight[label_n] for the single kind-1 head when class_weight (device table [size of that head], NULL: none) is given;
 * an out-of-range label then weighs 0.  Weights are finite and >= 0.  Kind-1 targets are
 * one_hot * (1 - label_smoothing) + label_smoothing / size, label_smoothing in [0, 1).
 *   L_i = sum_n w_n sum_c l_{n,c} / (size_i * #{n : w_n != 0})   (kind 1: size_i = 1;  0, with zero gradients, when no w_n != 0)
 * and d(loss)/d(pred) carries w_n / (size_i * count_i) in place of 1 / (size_i * N).  The counts are integer counts formed inside
 * the same launches (every workgroup of the per-sample kernel reads the N weights and labels): the launches are those of the
 * unshaped entry points, with shaped kernels.  With every weight 1 (or NULL), label_smoothing 0 and no kind-2 head all outputs
 * are bitwise those of the unshaped entry points (single-workgroup kernel: for N <= 1024, where a thread sums one sample).
 * GEECO_EINVAL: shaping NULL, label_smoothing outside [0, 1), huber_delta[i] <= 0 or not finite on a kind-2 head, class_weight
 * without exactly one kind-1 head.  The unshaped entry points refuse head_kind 2. */
typedef struct geeco_loss_shaping {
  const float* sample_weight;
  int64_t sample_weight_stride;
  const float* class_weight;
  float label_smoothing;
  float huber_delta[5];
} geeco_loss_shaping;
int64_t geeco_loss_shaping_sizeof(void);
int geeco_heads_loss_shaped_fwd_bwd(const float* h, const float* fc1_w, const float* fc1_b, int nheads,
                                    const float* const* heads_w, const float* const* heads_b, const int* head_size,
                                    const int* head_kind, const float* head_weight, const float* const* targets,
                                    const int64_t* target_stride, float loss_scale, int N, int H, int Hfc,
                                    const geeco_loss_shaping* shaping, float* preds, float* losses, int backward, float* dh,
                                    float* d_fc1_w, float* d_fc1_b, float* const* d_heads_w, float* const* d_heads_b, float* ws,
                                    void* stream);
int geeco_lstm_step_heads_shaped_fwd_bwd(const float* x, int64_t ldx, const float* wx, int64_t ldw, const float* bias, float* z,
                                         float* c, float* h, float* gates, int N, int H, int D, void* gemm_ws,
                                         const float* fc1_w, const float* fc1_b, int nheads, const float* const* heads_w,
                                         const float* const* heads_b, const int* head_size, const int* head_kind,
                                         const float* head_weight, const float* const* targets, const int64_t* target_stride,
                                         float loss_scale, int Hfc, const geeco_loss_shaping* shaping, float* preds,
                                         float* losses, int backward, float* dz, float* d_fc1_w, float* d_fc1_b,
                                         float* const* d_heads_w, float* const* d_heads_b, float* heads_ws,
                                         geeco_heads_finish* pending, void* stream);

/* The INFERENCE decoder of the per-frame controllers (e2e_vmc, goal_e2evmc 'sequence': T = window_size steps from the zero state,
 * graph.py:217-260) after the hoisted input projection, as ONE launch: the T - 1 recurrent h wh products, the gate math of all T
 * steps, fc1 (ReLU) and the linear heads on h_{T-1}.  Replaces, per call, (T - 1) x geeco_gemm_f32 + T x geeco_lstm_gates_fwd +
 * geeco_heads_loss_fwd_bwd; no per-step z / gates / c / h history, no losses, no targets.
 *   zx [T][N][4H] (row t * N + n at zx + (t * N + n) * ldz, ldz >= 4H): X wx WITHOUT bias, as geeco_gemm_f32 leaves it;
 *   wh [H][4H] (ldw): rows D..D+H-1 of lstm_cell/kernel, addressed in place;  bias [4H];
 *   fc1_w [H][Hfc], fc1_b [Hfc]; nheads <= 5 heads [Hfc][size_i] / [size_i] as parallel arrays (geeco_heads_loss_fwd_bwd);
 *   preds [N][sum size_i];  h_last, c_last [N][H]: the final state, either may be NULL.
 * Arithmetic as the LSTM cell above (gate order i, j, f, o; forget_bias 1): z_0 = zx_0 + bias (step 0 forms no h wh term: T = 1
 * never reads wh's values), z_t = zx_t + bias + h_{t-1} wh.  One workgroup per sample walks the T steps alone, wh resident in its
 * registers: no workspace, nothing waits for another block, and a sample's outputs depend on its own zx rows and the weights
 * only -- bitwise the same for every N and every index n.
 * GEECO_EINVAL: null pointer, N < 1, T outside 1..64, nheads outside 1..5, sum size_i > 32, ldz / ldw < 4H.
 * GEECO_ENOSUP (nothing launched) outside H <= 128, Hfc in {64, 128}: the caller runs the separate entry points. */
int geeco_lstm_seq_heads_fwd(const float* zx, int64_t ldz, const float* wh, int64_t ldw, const float* bias, const float* fc1_w,
                             const float* fc1_b, int nheads, const float* const* heads_w, const float* const* heads_b,
                             const int* head_size, int N, int T, int H, int Hfc, float* preds, float* h_last, float* c_last,
                             void* stream);

/* ---- optimiser: tf.train.AdamOptimizer(lr).minimize, estimator.py:105,243-244 ------------------
 * TF semantics (epsilon outside the bias correction):
 *   m = b1 m + (1-b1) g;  v = b2 v + (1-b2) g^2;  p -= lr_t m / (sqrt(v) + eps),
 *   lr_t = lr sqrt(1-b2^t)/(1-b1^t).
 * geeco_adam_prepare increments the DEVICE-resident global step t (tf.train.get_global_step) and
 * writes lr_t to scal_dev[0]; keeping both on the device lets a captured hipGraph replay the step.
 * geeco_adam_tf is one fused pass over the flat parameter arena: grad_scale multiplies g first
 * (1/world after an all-reduce SUM); l2 adds l2 * p to g (tf.contrib.layers.l2_regularizer,
 * graph.py:13-15).  Arenas must be 16-byte aligned. */
int geeco_adam_prepare(int64_t* global_step_dev, float lr, float beta1, float beta2, float* scal_dev,
                       void* stream);
int geeco_adam_tf(float* p, const float* g, float* m, float* v, int64_t n, const float* lr_t_dev,
                  float beta1, float beta2, float eps, float grad_scale, float l2, void* stream);
/* The same update over up to GEECO_ADAM_SEGMENTS_MAX pieces of the arena (offsets and counts in floats, multiples of 4), each piece
 * with its own gradient source; g_out != NULL: every piece's (unscaled) gradients are also stored at its place in that arena.
 * Any partition of the arena gives bitwise geeco_adam_tf's result.  Data parallel (round 5): the variables whose gradients came
 * with the early bucket are updated while the late bucket is still on the wire; the encoders' conv1 / conv2 follow, their
 * gradients read straight from the late bucket's staging buffer (no unpack copies).  The reference has one optimiser op per
 * variable and no distributed code (estimator.py:243-244). */
#define GEECO_ADAM_SEGMENTS_MAX 8
typedef struct geeco_adam_segment {
  const float* g;       /* gradients of the piece (16-byte aligned) */
  int64_t p_off, count; /* its place in the parameter / moment arenas */
} geeco_adam_segment;
int geeco_adam_tf_segments(float* p, float* g_out, float* m, float* v, const geeco_adam_segment* segs, int nseg,
                           const float* lr_t_dev, float beta1, float beta2, float eps, float grad_scale, float l2,
                           void* stream);
/* The two updates above with an exponential moving average of the parameters kept by the same pass (opt-in; semantics of
 * tf.train.ExponentialMovingAverage with zero_debias=False and num_updates=global_step): p, m, v come out bit for bit as
 * geeco_adam_tf / geeco_adam_tf_segments leave them, and every updated element of the shadow arena `ema` (indexed like p, 16-byte
 * aligned) follows, in float32,
 *   d_t = min(decay, (1 + t) / (10 + t));   ema -= (ema - p') (1 - d_t),      p' = the parameter just written,
 * t = *global_step_dev as the prepare work of this step left it (geeco_adam_prepare or the last launch of
 * geeco_slab_reduce_batch_prepare, earlier on the stream): the t of lr_t.  No second read of p and no extra launch; any
 * partition of the arena gives bitwise the one-pass shadow arena too.  GEECO_EINVAL (nothing launched): ema or global_step_dev
 * NULL, ema misaligned, decay outside (0, 1). */
int geeco_adam_tf_ema(float* p, const float* g, float* m, float* v, float* ema, int64_t n, const float* lr_t_dev,
                      const int64_t* global_step_dev, float decay, float beta1, float beta2, float eps, float grad_scale,
                      float l2, void* stream);
int geeco_adam_tf_segments_ema(float* p, float* g_out, float* m, float* v, float* ema, const geeco_adam_segment* segs, int nseg,
                               const float* lr_t_dev, const int64_t* global_step_dev, float decay, float beta1, float beta2,
                               float eps, float grad_scale, float l2, void* stream);
/* Opt-in clipping of the gradient by its global norm (tf.clip_by_global_norm in front of the optimiser), three launches, all on
 * the device.  The total gradient of element i is the one Adam forms, G_i = g_i * grad_scale + l2 * p_i.
 * geeco_grad_sumsq_segments: partials[k] = the sum of G_i^2 over the arena offsets [k * CH, (k + 1) * CH) below n, CH a constant
 *   of the library, geeco_clip_ws_floats(n) partials in all.  The gradient of an element is found through the pieces (the table of
 *   geeco_adam_tf_segments, but ANY offset and count >= 1 inside [0, n), sources 4-byte aligned, pieces disjoint); an element no
 *   piece covers adds 0; p is read only when l2 != 0.  The summation order inside a chunk is fixed, so any partition of the same
 *   elements into pieces gives bitwise the same partials.
 * geeco_clip_scale: norm = sqrt(sum of the partials, one fixed order), out2[0] = s = clip / max(norm, clip) (exactly 1.0f whenever
 *   norm <= clip), out2[1] = norm.  clip: finite, > 0.  A non-finite norm is not guarded: s and every update are then NaN
 *   (the opt-in that skips such a step: geeco_guard_decide below).
 * geeco_adam_tf_segments_clip: geeco_adam_tf_segments (ema_or_null == NULL) or geeco_adam_tf_segments_ema on G_i * clip_dev[0];
 *   clip_dev[0] == 1.0f gives bitwise their p, m, v and shadow arena.  Offsets are multiples of 4 floats, counts any number >= 1
 *   (a piece ends in a scalar tail), so the whole arena is the one-piece call. */
int64_t geeco_clip_ws_floats(int64_t n);
int geeco_grad_sumsq_segments(const float* p, const geeco_adam_segment* segs, int nseg, int64_t n, float grad_scale, float l2,
                              float* partials, void* stream);
int geeco_clip_scale(const float* partials, int64_t nchunks, float clip, float* out2, void* stream);
int geeco_adam_tf_segments_clip(float* p, float* g_out, float* m, float* v, float* ema_or_null, const geeco_adam_segment* segs,
                                int nseg, const float* lr_t_dev, const int64_t* global_step_dev, float decay, const float* clip_dev,
                                float beta1, float beta2, float eps, float grad_scale, float l2, void* stream);
/* Opt-in skipping of optimiser steps whose gradient is not finite: geeco_grad_sumsq_segments, then the two entries below in place of
 * geeco_clip_scale and geeco_adam_tf_segments_clip.  The step is APPLIED iff norm = sqrt(sum of the partials), formed in float32 in
 * geeco_clip_scale's order, is finite.  A NaN or an infinity in any element a piece covers makes it non-finite, and so does a finite
 * gradient whose squares overflow float32 (|G_i| beyond about 1.8e19).
 * geeco_guard_decide: one 256-thread block.  clip: finite, >= 0; 0 = no clipping.  guard: int64[3] the caller zeroes once.
 *   finite norm:      out2[0] = geeco_clip_scale's s, bitwise (clip > 0), or 1.0f (clip == 0); out2[1] = norm;
 *                     guard[0] = 1, guard[1] (skipped steps in all) unchanged, guard[2] (skipped steps in a row) = 0
 *   non-finite norm:  out2[0] = 0.0f; out2[1] = norm as computed (NaN or +inf); guard[0] = 0, guard[1] += 1, guard[2] += 1
 * geeco_adam_tf_segments_guard: geeco_adam_tf_segments_clip behind one uniform test of guard_dev[0].  1: exactly that entry point's
 *   work (clip_dev[0] == 1.0f: bitwise the unclipped kernels' p, m, v and shadow arena).  0: g_out, where non-null, receives the
 *   pieces' gradients and p, m, v and the shadow arena are neither read nor written.  The step counter is not this kernel's: a
 *   skipped step has advanced it (the prepare work runs before the norm exists) and is a step with no update.
 * Both return GEECO_EINVAL before any launch for a null pointer (guard / guard_dev included), nchunks < 1, a clip that is negative or
 * not finite, and whatever geeco_adam_tf_segments_clip refuses. */
int geeco_guard_decide(const float* partials, int64_t nchunks, float clip, float* out2, int64_t* guard, void* stream);
int geeco_adam_tf_segments_guard(float* p, float* g_out, float* m, float* v, float* ema_or_null, const geeco_adam_segment* segs,
                                 int nseg, const float* lr_t_dev, const int64_t* global_step_dev, float decay, const float* clip_dev,
                                 const int64_t* guard_dev, float beta1, float beta2, float eps, float grad_scale, float l2,
                                 void* stream);
/* Opt-in fine-tuning: the update of geeco_adam_tf_segments_guard with a learning-rate multiplier per piece.  Piece k runs
 * lr_t_dev[0] * lr_mul[k], one float32 product per piece formed on the device from lr_t_dev[0] as the prepare work left it.
 * lr_mul: nseg floats on the HOST, each a finite number > 0.  A frozen variable is not a multiplier of 0 but a piece the caller leaves
 * out: what no piece covers is neither read nor written, its p, m, v and shadow weights keep every bit.
 * clip_dev_or_null == NULL: the gradient is not scaled (s is exactly 1.0f).  guard_dev_or_null == NULL: the step is always applied; a
 * verdict of 0 writes only g_out.  ema_or_null, g_out, offsets (multiples of 4 floats) and counts (any number >= 1, a piece ends in a
 * scalar tail) as geeco_adam_tf_segments_guard.  With every multiplier 1.0f the results are bit for bit those of
 * geeco_adam_tf_segments_clip (clip given), geeco_adam_tf_segments_guard (guard given), geeco_adam_tf_segments / _ema (neither).
 * GEECO_EINVAL (nothing launched): what geeco_adam_tf_segments_clip refuses, lr_mul NULL, a multiplier that is 0, negative or not
 * finite. */
int geeco_adam_tf_segments_scaled(float* p, float* g_out, float* m, float* v, float* ema_or_null, const geeco_adam_segment* segs,
                                  const float* lr_mul, int nseg, const float* lr_t_dev, const int64_t* global_step_dev, float decay,
                                  const float* clip_dev_or_null, const int64_t* guard_dev_or_null, float beta1, float beta2, float eps,
                                  float grad_scale, float l2, void* stream);
/* Opt-in learning-rate schedules, evaluated on the device from the step counter by the thread that does the prepare work: no
 * launch, no host synchronisation and no re-capture of a recorded step; a restored counter continues the schedule.
 * With t the counter after the increment (the t of lr_t), s = t - 1 the updates completed (the global_step TF 1.15's
 * tf.train.*_decay see), w = warmup_steps and u = s - w:
 *   s <  w:  lr(s) = L0 (s + 1) / w,  L0 = the schedule's value at its own step 0 (base_lr; values[0] for PIECEWISE)
 *   s >= w:  CONSTANT     base_lr
 *            EXPONENTIAL  base_lr decay_rate^(u / decay_steps); staircase != 0: the exponent is floor(u / decay_steps)
 *            COSINE       base_lr ((1 - alpha) 0.5 (1 + cos(pi min(u, decay_steps) / decay_steps)) + alpha)
 *            PIECEWISE    values[i] for the first i with u <= boundaries[i], else values[n_boundaries]; base_lr is ignored
 * (tf.train.exponential_decay, cosine_decay, piecewise_constant), all in double from the fields as declared, one rounding to float.
 * geeco_adam_prepare_schedule / geeco_slab_reduce_batch_prepare_schedule: their constant-lr counterparts with lr(s) in place of
 *   lr (slab sums bitwise geeco_slab_reduce_batch's); they also store lr(s) in scal_dev[2] (scal_dev[1] and [3] are not touched).
 * geeco_lr_schedule_eval: *lr_out = lr(step) on the host; needs no GPU.
 * All three return GEECO_EINVAL before any launch for: a null pointer, an unknown kind, warmup_steps < 0, decay_steps < 1
 * (EXPONENTIAL, COSINE), n_boundaries outside 0..GEECO_LR_BOUNDARIES_MAX or boundaries not strictly increasing, a rate or value that
 * is negative or not finite, decay_rate <= 0, alpha outside [0, 1]; geeco_lr_schedule_eval also for step < 0. */
#define GEECO_LR_CONSTANT 0
#define GEECO_LR_EXPONENTIAL 1
#define GEECO_LR_COSINE 2
#define GEECO_LR_PIECEWISE 3
#define GEECO_LR_BOUNDARIES_MAX 8
typedef struct geeco_lr_schedule {
  int32_t kind;                                  /* GEECO_LR_* */
  float base_lr;
  int64_t warmup_steps, decay_steps;
  float decay_rate, alpha;
  int32_t staircase, n_boundaries;
  int64_t boundaries[GEECO_LR_BOUNDARIES_MAX];   /* in steps after the warm-up (u) */
  float values[GEECO_LR_BOUNDARIES_MAX + 1];
} geeco_lr_schedule;
int geeco_adam_prepare_schedule(int64_t* global_step_dev, const geeco_lr_schedule* schedule, float beta1, float beta2,
                                float* scal_dev, void* stream);
int geeco_slab_reduce_batch_prepare_schedule(const geeco_slab_reduce* items, int n, int64_t* global_step_dev,
                                             const geeco_lr_schedule* schedule, float beta1, float beta2, float* scal_dev,
                                             void* stream);
int geeco_lr_schedule_eval(const geeco_lr_schedule* schedule, int64_t step, double* lr_out);
/* Opt-in per-variable statistics of the gradient, the parameters and the update direction: two launches, read-only on
 * the four arenas, meant for logging steps and never part of a captured step.
 * Variables: nvar >= 1 spans [var_off[i], var_off[i] + var_cnt[i]) of the arenas [0, n), offsets multiples of 4 floats, counts any
 *   number >= 1, disjoint, in any order, pad floats between them allowed.  Only the variables' own elements are read: no pad, no slack.
 *   var_off / var_cnt are HOST arrays (checked on every call); `table` is the DEVICE table the caller builds from them once, int64:
 *     table[2 i], table[2 i + 1]                       first chunk of variable i and its number of chunks, ceil(var_cnt[i] / CH)
 *     table[2 nvar + 2 c], table[2 nvar + 2 c + 1]     arena offset and element count (1..CH) of chunk c
 *   the chunks of a variable are consecutive, each CH = GEECO_VARSTATS_CHUNK elements but the variable's last, variables in the
 *   order of var_off, nchunks = the sum of their chunk counts.  The table is the caller's to get right (ops.VariableStatsPlan).
 * Gradient: G_i = g_i * grad_scale (one float32 product; no l2 term), g_i found through the pieces exactly as
 *   geeco_grad_sumsq_segments finds it (1..GEECO_ADAM_SEGMENTS_MAX disjoint pieces, any offset and count inside [0, n), sources 4-byte
 *   aligned).  An element no piece covers has no gradient: it is in none of the gradient's fields.  A variable no piece touches has
 *   grad_covered == 0 (its gradient is absent); a half-covered variable is NOT refused, its record describes the covered elements.
 * Update direction: u_i = m_i / (sqrtf(v_i) + eps) from the moments as they stand.
 * Record (one per variable, out[nvar]): counts are exact integers; sums are float32, over the FINITE elements only -- a NaN or an
 *   infinity is counted in `nonfinite` and is in no sum, extremum or class; min = +inf and max = -inf where nothing is finite.
 *   Magnitude classes of a finite non-zero x: e = ((bits >> 23) & 0xff) - 127 clamped to [-32, 7], class e + 32 (denormals: class 0,
 *   |x| >= 128: class 39), counted in `neg` or `pos` by sign; zeros (+-0) are counted in `zeros` and are in no class.
 * ws: geeco_variable_stats_ws_bytes(nchunks) bytes, 16-byte aligned (one partial record per chunk).  Reduction order: csrc/varstats.hip;
 *   the record is bitwise the same for any partition of the gradient into pieces and from call to call.
 * GEECO_EINVAL (nothing launched): a null pointer, p / m / v / ws / out / table misaligned (16 / 16 / 16 / 16 / 8 / 8 bytes), nvar < 1,
 *   an offset that is no multiple of 4, a count < 1, a variable outside [0, n), overlapping variables, nchunks other than the table's,
 *   nseg outside 1..GEECO_ADAM_SEGMENTS_MAX and whatever geeco_grad_sumsq_segments refuses of a piece, eps negative or not finite. */
#define GEECO_VARSTATS_CHUNK 4096
#define GEECO_VARSTATS_CLASSES 40
typedef struct geeco_varstats_tensor {
  int64_t nonfinite, zeros;
  float sum, sumsq, min, max;                    /* over the finite elements (zeros included) */
  int64_t neg[GEECO_VARSTATS_CLASSES], pos[GEECO_VARSTATS_CLASSES];
} geeco_varstats_tensor;
typedef struct geeco_varstats_record {
  int64_t grad_covered;                          /* elements of the variable that a piece covers; 0: the gradient is absent */
  geeco_varstats_tensor grad, param;
  int64_t update_nonfinite;
  float update_sumsq, update_max_abs;            /* over the finite u_i */
} geeco_varstats_record;
int64_t geeco_variable_stats_ws_bytes(int64_t nchunks);
int geeco_variable_stats(const float* p, const float* m, const float* v, const geeco_adam_segment* segs, int nseg, int64_t n,
                         float grad_scale, float eps, const int64_t* var_off, const int64_t* var_cnt, int nvar,
                         const int64_t* table, int64_t nchunks, void* ws, geeco_varstats_record* out, void* stream);
/* Opt-in gradient accumulation over micro-batches (additive within ABI 7): one streaming launch that stores or adds the
 * pieces of a micro-batch's gradient into the accumulator arena acc[0, n).  For every piece k and every i < count_k:
 *   overwrite != 0:  acc[p_off_k + i] = g_k[i]                      (acc is NOT read: an accumulator full of NaN comes out finite)
 *   overwrite == 0:  acc[p_off_k + i] = acc[p_off_k + i] + g_k[i]   (one float32 addition)
 * Pieces as geeco_adam_tf_segments_clip takes them: 1..GEECO_ADAM_SEGMENTS_MAX of them, offsets multiples of 4 floats, counts any
 * number >= 1 (a piece ends in a scalar tail), sources and acc 16-byte aligned.  Floats no piece covers, and those past n, keep every
 * bit.  The addition has nothing to contract with, so any partition of a range gives bitwise the one-piece result.
 * GEECO_EINVAL (nothing launched): a null pointer, nseg outside 1..GEECO_ADAM_SEGMENTS_MAX, n < 1, a misaligned offset, source or
 * accumulator, a count < 1, a piece not inside [0, n), a source that overlaps a range of acc the launch writes. */
int geeco_grad_accumulate_segments(float* acc, const geeco_adam_segment* segs, int nseg, int64_t n, int overwrite, void* stream);
/* sum of squares of an arena (for the L2 regularisation loss term); out[0] overwritten. */
int geeco_sumsq(const float* p, int64_t n, float* out, void* stream);

/* ---- input gradients: d(loss)/d(frames), for saliency maps (additive within ABI 7) ----------------------------
 * The training backward stops at conv1, whose input is data.  These entry points carry it on to the frames; no training step
 * launches them.  The reference has no counterpart: they are what tf.gradients(loss, features['rgb']) would compute. */
/* conv1's input gradient, Conv2DBackpropInput of the 3 x 3, stride-1, SAME layer with 32 output channels:
 *   dx[f][y][x][ci] = sum_{ky,kx,co} dz1[f][y+1-ky][x+1-kx][co] * w1[ky][kx][ci][co]
 * dz1 [G][F][H][W][32] (conv1's ReLU gradient already applied), w1 [G][3][3][Cin][32] = the variable itself (HWIO, Cin 3 or 4,
 * no padded copy), dx [G][F][H][W][4]; channel 3 is written as 0 when Cin == 3.  No ReLU mask (the input is data).  Any
 * H, W >= 1; F and G <= 65535; dz1 / dx 16-byte aligned.  VALU FMAs, dz1 staged through LDS once per 8 x 32 tile, one fmaf chain
 * per output (ky, kx, co ascending).  GEECO_ENOSUP, having launched nothing, for any other Cin or Cout. */
int geeco_conv1_dgrad(const float* dz1, const float* w1, float* dx, int groups, int64_t gs_dz, int64_t gs_w, int64_t gs_dx,
                      int F, int H, int W, int Cin, int Cout, void* stream);
/* The adjoint of geeco_pack_pixels: d_src[n][p][0..C1) takes d_dst[n][p][0..C1) (d_dst [N][HW][Cpad]; accumulate != 0: is added
 * to, one float32 addition), at its own sample stride; d_src2 (RGB-D's second tensor; may be NULL, as may d_src) takes the
 * channels C1..C1+C2 the same way under accumulate2.  The padding channels have no adjoint. */
int geeco_pack_pixels_bwd(const float* d_dst, float* d_src, int64_t src_sample_stride, int accumulate, float* d_src2,
                          int64_t src2_sample_stride, int accumulate2, int N, int64_t HW, int C1, int C2, int Cpad,
                          void* stream);
/* The adjoint of geeco_dynimg_fwd, both forms (K frames with sample / frame strides; K = 2 with frames2).  g [N][HW][Cpad] = the
 * gradient with respect to the normalised image (channels >= C are ignored); frames / frames2 / strides / alpha_host as the
 * forward took them: D = sum_t alpha_t X_t is recomputed in the forward's summation order, so min / max sit where the forward
 * found them.  Per sample, r = max - min + 1e-6, out = (D - min) / r:
 *   dD_i = g_i / r + [D_i == min] (sum_j g_j (out_j - 1) / r) / n_min - [D_i == max] (sum_j g_j out_j / r) / n_max
 * n_min / n_max = the number of elements equal to the extremum: TF 1.15's reduce_min / reduce_max gradient, which shares evenly
 * among ties.  d_frames[n][t] (+)= alpha_t dD[n] at d_sample_stride / d_frame_stride (accumulate), and in the two-frame form
 * d_frames[n] (+)= alpha_0 dD[n], d_frames2[n] (+)= alpha_1 dD[n] (dense [N][HW * C]; accumulate2); either destination may be
 * NULL.  Two launches (reduce, apply); ws: geeco_dynimg_bwd_ws_bytes(N, HW, C) bytes of per-block records.  No atomics; the sums
 * run in one fixed order (a thread over its elements ascending, the lanes of a wave in a fixed butterfly, the four waves
 * ascending, the blocks ascending), so two runs are bitwise equal. */
int64_t geeco_dynimg_bwd_ws_bytes(int N, int64_t HW, int C);
int geeco_dynimg_bwd(const float* g, const float* frames, const float* frames2, int64_t sample_stride, int64_t frame_stride,
                     const float* alpha_host, int N, int K, int64_t HW, int C, int Cpad, float* d_frames,
                     int64_t d_sample_stride, int64_t d_frame_stride, int accumulate, float* d_frames2, int accumulate2,
                     void* ws, void* stream);

/* ---- episode replay: a controller's commands for a whole recorded episode (replay.py; additive within ABI 7) ----
 * The per-frame controllers (e2e_vmc; goal_e2evmc 'sequence' x 'constant' / 'residual') over the T frames of one episode, every
 * frame encoded once.  Both entries only enqueue on `stream`; neither uses atomics. */
/* Window builder.  feat [T][cells][ch]: the encoder's features of the episode's frames; jnt [T][J]; tgt_feat [cells][ch]: the
 * features of the episode's goal frame (NULL for PLAIN).  Writes the windows t = t0 .. t1 - 1 into states [K][N][state_stride]
 * (N >= t1 - t0: the row count of a step; window t is row t - t0, rows t1 - t0 .. N - 1 are not touched): slot k (oldest first)
 * of window t shows frame max(0, t - K + 1 + k), what the predictor holds after a reset at frame 0 and t pushes
 * (predictor.py:192-200); the joint-state columns follow the same index.  Per cell the columns of geeco_predict_push_features for
 * `mode`, bit for bit (a copy; one subtraction tgt - feat in RESIDUAL).  Grid-stride over (k, window, unit): no cap on T * K.
 * 16-byte loads when ch % 4 == 0 and the sources are aligned; 16-byte stores when also J % 4 == 0, state_stride % 4 == 0 and
 * states is aligned (with J = 7 a cell's columns start at odd offsets), else one float per lane.  K: 1..64;
 * 0 <= t0 < t1 <= T. */
int geeco_replay_states(const float* feat, const float* jnt, const float* tgt_feat, int mode, int T, int t0, int t1, int N, int K,
                        int cells, int ch, int J, float* states, int64_t state_stride, void* stream);
/* Error reduction.  preds [T][P]: the decoder's heads side by side; labels [T][P]: the recorded values in the same columns (a
 * class head holds the class index in its first column).  Head h covers columns [head_off[h], + head_size[h]); head_kind[h] 0:
 * out_frame[t][h] = (sum_c (preds - labels)^2, c ascending, every product and sum rounded to float32) / head_size[h];
 * head_kind[h] 1: 1.0f where the argmax of the logits (first maximum on ties) equals the recorded class, else 0.0f, NaN when a
 * logit is NaN.  A NaN prediction gives a NaN error.  out_episode[h] = the mean of out_frame[.][h] over the T frames, formed by
 * ONE block of 256 threads: thread i adds the frames i, i + 256, .. in ascending order, the 256 partial sums are folded by halves
 * (128, 64, .., 1: element j takes j + half), the result is divided by T -- two runs are bitwise equal.  The head_* arrays are
 * host memory, nheads <= GEECO_REPLAY_MAXHEADS, head_size <= 64.  Two launches. */
#define GEECO_REPLAY_MAXHEADS 8
int geeco_replay_errors(const float* preds, const float* labels, int T, int P, int nheads, const int* head_off,
                        const int* head_size, const int* head_kind, float* out_frame, float* out_episode, void* stream);

/* ---- episode replay for the dynamic-image controllers (replay_dynimg.py; additive within ABI 7) -----------------
 * geeco-f (proc_obs 'dynimg') and 'sequence' x 'dyndiff' over the T frames of one episode with the goal frame fixed: every conv1
 * input is then a function of the frame number alone. */
/* Input stage, read straight from the resident episode.  frame_addr: a DEVICE array of T frame addresses; a frame is [HW][3],
 * uint8 (frames_u8 != 0; 4-byte aligned, read as float(u8) / 255 correctly rounded) or float32 in [0, 1] (16-byte aligned); goal:
 * one frame of the same kind.  alpha_host [K] / alpha2_host [2]: geeco_dynimg_alpha(K) / (2), host memory.  For the windows
 * t = t0 .. t1 - 1 (row t - t0 of each output, [t1 - t0][HW][4], 16-byte aligned):
 *   cur_out  = frame t as (R, G, B, 0);
 *   diff_out = the normalised two-frame dynamic image alpha2[0] frame_t + alpha2[1] goal;
 *   buf_out  = the normalised dynamic image sum_k alpha[k] frame_{max(0, t - K + 1 + k)}, k = 0 .. K - 1 ascending (the window the
 *              predictor holds after a reset at frame 0 and t pushes, predictor.py:192-200); buf_out == NULL skips the K-frame
 *              walk (the per-frame form of 'sequence' x 'dyndiff').
 * normalised = (D - min D) / (max D - min D + 1e-6f) over the window's HW x 3 values, the fourth channel 0.  The sums and the
 * normalisation are those of geeco_dynimg_fwd (C = 3, Cpad = 4), so every output is bitwise what geeco_goal_dynimgs_fwd /
 * geeco_goal_dynimgs_u8_fwd write for the explicitly built dense windows.  NOTE window 0 of buf_out: its K frames are equal and
 * sum alpha = 0, so its raw image is float32 rounding residue (exactly 0 at K <= 3) and its normalised image is that residue
 * scaled up: the reference's own behaviour after a reset, reproduced bit for bit, but nothing a float64 model predicts.
 * Two launches: (1) per block the min / max of both raw images into ws, (2) the window's partials folded in a fixed order, both
 * images formed again and stored normalised, once.  No block waits for another and there are no atomics: two runs are bitwise
 * equal.  ws: geeco_replay_images_ws_bytes(t1 - t0, HW) bytes, 16-byte aligned, no zero-fill needed.  Blocks stride over
 * (window, 1024-pixel block): no cap on T.  K: 1..64; HW % 4 == 0; 0 <= t0 < t1 <= T.  Nothing outside rows [0, t1 - t0) of the
 * outputs is written. */
int64_t geeco_replay_images_ws_bytes(int windows, int64_t HW);
int geeco_replay_images(const void* const* frame_addr, const void* goal, int frames_u8, const float* alpha_host,
                        const float* alpha2_host, int T, int t0, int t1, int K, int64_t HW, float* cur_out, float* buf_out,
                        float* diff_out, void* ws, void* stream);
/* geeco_replay_states with a per-frame second feature table: feat [T][cells][ch], tgt_feat [T][cells][ch_t], jnt [T][J] ->
 * states [K][N][state_stride]; slot k of window t (row t - t0) takes frame max(0, t - K + 1 + k) from all three.  Per cell the
 * columns are [feat (ch) | jnt (J) | tgt (ch_t)]: what geeco_state_concat_fwd writes for the dense 'sequence' x 'dyndiff' model
 * (features ConvEncoder, DynDiffEncoder; jnt_pos = 1), the reference's tf.concat([feat, jnt, tgt_feat]) (graph.py:146-167).
 * A copy, bit for bit.  16-byte loads when ch % 4 == 0, ch_t % 4 == 0 and both tables are aligned; 16-byte stores when also
 * J % 4 == 0, state_stride % 4 == 0 and states is aligned.  N >= t1 - t0; rows t1 - t0 .. N - 1 are not touched. */
int geeco_replay_states_pair(const float* feat, const float* tgt_feat, const float* jnt, int T, int t0, int t1, int N, int K,
                             int cells, int ch, int ch_t, int J, float* states, int64_t state_stride, void* stream);

/* ---- attributions: integrated gradients and SmoothGrad (attribution.py; additive within ABI 7) -------------------
 * Many input gradients along a family of perturbed inputs, summed on the device.  The three entries are the streaming stages
 * around the model's own forward, backward and input-gradient pass; no training step launches them.  Each only enqueues on
 * `stream`; none uses atomics; 16-byte accesses when the tensors are 16-byte aligned (and, for a broadcast baseline, its period
 * is a multiple of 4 floats), one float per access otherwise -- the values are the same bits on every path.  Every difference,
 * product and sum below is rounded to float32 on its own (no fused multiply-add).  All pointers are device memory, 4-byte
 * aligned.  Bad arguments return GEECO_EINVAL before anything is launched. */
/* The path point:  dst[i] = b + alpha * (x[i] - b) + sigma * z(key, step, i),  b = baseline[i % baseline_period], i < n.
 * baseline_period = n for a full baseline, one frame's element count for one frame broadcast over the frames; it must divide n.
 * baseline == NULL: b = 0 (the period is ignored).  sigma == 0 draws nothing and adds no noise term.  z ~ N(0, 1) comes from the
 * Philox4x32-10 / Box-Muller routine of the scene noise (csrc/philox_normal.h): element i takes normal i % 4 of the counter
 * (c0, c1, c2, c3) = (low word of i / 4, high word of i / 4, step, 0) under the key (low word of key, high word of key).
 * There is NO clamp: the result may leave [0, 1] (a path point is not an image; SmoothGrad's noise is not clipped).  dst may not
 * overlap x.  With baseline == NULL, alpha == 1 and sigma == 0 the result is x, bit for bit (-0 becomes +0). */
int geeco_attr_path_point(float* dst, const float* x, const float* baseline, int64_t baseline_period, float alpha, float sigma,
                          uint64_t key, uint32_t step, int64_t n, void* stream);
/* The running sum:  acc[i] = (overwrite ? 0 : acc[i]) + weight * g[i], the product rounded, then the sum.  overwrite != 0: acc is
 * not read.  acc may not overlap g. */
int geeco_attr_accumulate(float* acc, const float* g, float weight, int64_t n, int overwrite, void* stream);
/* The finish, on tensors [N][frames_per_sample][HW][C] (acc, x, attr; C in 1..4) and [N][frames_per_sample][HW] (saliency):
 *   attr[i] = multiply_by_input ? (x[i] - b) * acc[i] : acc[i]      (b as above; x and baseline are not read otherwise)
 *   saliency[pixel] = max_c |attr[pixel][c]|                         (NaN when one of them is NaN)
 *   sample_sum[n] = the sum of attr over sample n, in ONE fixed order: the sample's S = frames_per_sample * HW * C elements are
 *   taken in groups of four consecutive elements; group q belongs to slot q % 1024; a slot adds its groups in ascending order,
 *   the elements of a group in ascending order, starting from +0; the 1024 slot sums are folded by halves (512, 256, .., 1: slot
 *   j takes slot j + half); slot 0 is the result.  Two runs are bitwise equal, and tests/_attribution_ref.py restates the order.
 * Two launches: the elementwise one over the whole grid, then one block of 1024 threads per sample that reads attr back (there
 * is no workspace argument; the finish runs once per pass).  attr may be acc itself (in place); a partial overlap of the two, or any overlap of attr with x or
 * another output, is refused. */
int geeco_attr_finish(float* attr, float* saliency, float* sample_sum, const float* acc, const float* x, const float* baseline,
                      int64_t baseline_period, int multiply_by_input, int N, int frames_per_sample, int64_t HW, int C,
                      void* stream);

/* ---- perturbation attributions: occlusion sensitivity and RISE (perturbation.py; additive within ABI 7) ----------
 * Hide a region of the input, run the model's forward, see how far the command moves.  The entries are the streaming stages
 * around that forward; no training step launches them.  Conventions as for the attribution entries above: each only enqueues on
 * `stream`; no atomics; 16-byte accesses when the tensors are 16-byte aligned and every frame (for the sums: every sample) holds
 * a multiple of four floats, one float per access otherwise -- the same bits on every path; every float32 operation is rounded on
 * its own (no fused multiply-add); device pointers are 4-byte aligned; bad arguments return GEECO_EINVAL before anything is
 * launched.
 *
 * Step m of a pass has an OCCLUSION WEIGHT o(m, sample, y, x) in [0, 1], shared by all frames and channels of the pixel.  It is
 * a function of the description below, the step and the sample alone -- never of the launch geometry, the access path or which
 * entry asks -- and is never stored: apply and accumulate recompute it with one device function.
 *
 * GEECO_PERTURB_OCCLUSION: a hard patch on a grid.  The patch is (min(ph, H), min(pw, W)) (one larger than the image is clipped
 * to it).  Along y there are Gy = 1 positions if ph >= H, else ceil((H - ph) / sy) + 1; position j starts at min(j * sy, H - ph)
 * (the last one is clamped, so every pixel is covered); Gx likewise along x.  Step m = j * Gx + i, 0 <= m < Gy * Gx.  o = 1
 * inside the patch, 0 outside, for every sample.
 *
 * GEECO_PERTURB_RISE: a random smooth mask per (step, sample).  g = grid (2..31), cells (ch, cw) = (ceil(H / g), ceil(W / g)).
 * The draws are 32-bit words of the Philox4x32-10 routine of csrc/philox_normal.h: word i is output i % 4 of the counter
 * (c0, c1, c2, c3) = (i / 4, sample, step, 1) under the key (low word of key, high word of key); `sample` counts from the
 * entry's sample0.  Words 0 .. (g + 1)^2 - 1 decide the keep-bits, row-major: bit[r][c] = word[r * (g + 1) + c] < keep_threshold
 * (an integer compare; the caller forms the threshold from the keep probability).  dy = word[(g + 1)^2] % ch,
 * dx = word[(g + 1)^2 + 1] % cw.  Then, in float32, each operation rounded, with yy = y + dy, r = yy / ch (integers), r1 =
 * min(r + 1, g), fy = float(yy - r * ch) * (1.0f / float(ch)) (the reciprocal rounded first), and xx, c, c1, fx likewise:
 *   top = bit[r][c] + fx * (bit[r][c1] - bit[r][c]);  bot = bit[r1][c] + fx * (bit[r1][c1] - bit[r1][c]);
 *   keep = top + fy * (bot - top);  o = 1 - keep. */
#define GEECO_PERTURB_OCCLUSION 0
#define GEECO_PERTURB_RISE 1
typedef struct geeco_perturb_desc {
  int32_t method;              /* GEECO_PERTURB_* */
  int32_t H, W;                /* the image */
  int32_t ph, pw, sy, sx;      /* occlusion: patch and stride (>= 1); not read for RISE */
  int32_t grid;                /* RISE: g; not read for occlusion */
  uint32_t keep_threshold;     /* RISE: >= 1 */
  uint32_t reserved;
  uint64_t key;                /* RISE: the generator's key */
} geeco_perturb_desc;
int64_t geeco_perturb_desc_sizeof(void);
/* Host only, nothing is launched: out[0..5] = Gy, Gx and the patch of `step`, rows [y0, y1) x columns [x0, x1), as
 * (y0, y1, x0, x1).  RISE: Gy = Gx = 0 and an empty patch.  `desc` here and below: a host geeco_perturb_desc, read during the call. */
int geeco_perturb_patch(const void* desc, int step, int32_t* out);
/* The occluded input, tensors [N][frames][H * W][C], C in 1..4:
 *   dst[e] = x[e] where o == 0;  f where o == 1;  x[e] + o * (f - x[e]) otherwise;   f = fill[e % fill_period], e the element's
 * index in the tensor (fill == NULL: 0; periods as geeco_attr_path_point's baseline: C for a colour, H * W * C for a frame, the
 * tensor's size for a full array).  The two exact cases are copies (a -0 stays -0).  prev_step == -1 writes the whole input.
 * prev_step >= 0 with GEECO_PERTURB_OCCLUSION: dst holds the result of prev_step on the same x and fill; only the previous patch
 * (x again) and the step's own are written -- the same bits as the whole rewrite.  (RISE rewrites everything whatever prev_step.)
 * dst may not overlap x. */
int geeco_perturb_apply(float* dst, const float* x, const float* fill, int64_t fill_period, const void* desc, int step,
                        int prev_step, int sample0, int N, int frames, int C, void* stream);
/* The score: d[n] = sum_j w[j] * (preds[n][j] - preds0[n][j])^2 over j = 0 .. OT - 1 ascending from +0; difference, square,
 * weighting and sum each rounded. */
int geeco_perturb_score(float* d, const float* preds, const float* preds0, const float* w, int N, int OT, void* stream);
/* The running sums num, den [N][H * W]: where o != 0, num = (overwrite ? 0 : num) + d[n] * o and den = (overwrite ? 0 : den) + o;
 * where o == 0 the step adds nothing (overwrite: the pixel becomes +0), so a NaN score reaches exactly the pixels its step hid.
 * d: device, one score per sample of this launch.  overwrite != 0: num and den are not read. */
int geeco_perturb_accumulate(float* num, float* den, const float* d, const void* desc, int step, int sample0, int N, int overwrite,
                             void* stream);
/* saliency[i] = den[i] > 0 ? num[i] / den[i] : +0, i < n.  saliency may not overlap num or den. */
int geeco_perturb_finish(float* saliency, const float* num, const float* den, int64_t n, void* stream);

#ifdef __cplusplus
}
#endif
#endif  /* GEECO_HIP_H_ */
