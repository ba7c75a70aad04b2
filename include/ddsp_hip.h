/*
 * ddsp_hip.h -- C ABI of libddsp_hip.so: the MI355X (gfx950) DDSP synthesis hot path.
 *
 * The reference (kureta/ddsp-pytorch) has no FFI of its own: its hot path is two
 * Python nn.Modules made of stock torch ops.  These entry points are what a binding
 * for that path binds instead of those op sequences:
 *
 *   ddsp_osc_forward_ex    replaces OscillatorBank.forward / .live
 *                          (model/ddsp/harmonic_oscillator.py:57-62 and :64-75, i.e.
 *                           prepare_harmonics :24-37, generate_phases :39-43, generate_signal :45-50)
 *   ddsp_noise_forward_ws  replaces FilteredNoise.forward
 *                          (model/ddsp/filtered_noise.py:40-53, i.e. amp_to_impulse_response :7-22,
 *                           fft_convolve :25-32, and the torch.rand draw :44-48)
 *
 * Conventions: plain pointers and sizes only (no torch types); every pointer is DEVICE memory
 * unless said otherwise; tensors are dense row-major fp32 with the reference's shapes; nothing
 * is allocated or synchronised inside (the caller passes scratch; launches are asynchronous on
 * `stream`, a hipStream_t passed as void*; NULL = the default stream).  Return value: 0 on
 * success, a hipError_t (> 0) if a launch failed, or a negative DDSP_E* code for bad
 * arguments.  No exceptions cross the boundary.
 */
#ifndef DDSP_HIP_H
#define DDSP_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DDSP_HIP_ABI_VERSION 5

#define DDSP_EINVAL (-1)   /* null pointer / non-positive size */
#define DDSP_ERANGE (-2)   /* shape outside what the kernels are built for */
#define DDSP_EPERM  (-3)   /* a test / tuning hook called in a process that did not opt in (see ddsp_test_hooks_enabled) */

/* ABI version of the loaded library (== DDSP_HIP_ABI_VERSION it was built with). */
int ddsp_hip_abi_version(void);

/*
 * The process-global test / tuning hooks below (ddsp_osc_set_tiling, ddsp_noise_set_generic, ddsp_gru_set_mode,
 * ddsp_gru_set_fault_step) change every later launch of the process.  They only work when the environment variable
 * DDSP_TEST_HOOKS=1 was set at the moment the library was loaded (tests/conftest.py and the tools/ scripts do that);
 * in any other process they return DDSP_EPERM for a non-default value and change nothing, so a production process cannot
 * flip them by accident.  Returns 1 when the hooks are enabled.
 */
int ddsp_test_hooks_enabled(void);

/*
 * Bytes of device scratch ddsp_osc_forward_ex needs for a [B,T,H] problem (any hop): frame-rate increments fp32 [B,T,H] +
 * normalised amplitudes fp32 [B,T,H] + an fp64 region of [B,T,H] (chunk totals, or frame-start phases + their superblock
 * totals) + a few int32 arrays of at most B*T entries (16*B*T*H bytes + ~2*B*(T+3)/4*H + 12*B*T + 4*T*(B+16) + flag words;
 * 256-byte aligned parts).
 */
size_t ddsp_osc_scratch_bytes(int B, int T, int H);

/*
 * Harmonic oscillator bank (harmonic_oscillator.py:57-62; .live :64-75 when live_in != NULL).
 *   f0 [B,T,1] Hz, c [B,T,H] harmonic amplitudes, a [B,T,1] loudness  ->  y [B, T*hop]
 *   scratch        >= ddsp_osc_scratch_bytes(B,T,H) bytes, 256-byte aligned
 *   live_in  [H]   nullable: phase offsets added to the first increment row of batch row 0 (:70)
 *   live_out [H]   nullable: receives the last phase row of batch row 0 (:72); must not alias live_in
 *   dbg_phi  [B,T*hop,H] nullable (tests only): the wrapped phases, bit-exact w.r.t. torch CPU
 *   flags          0 or DDSP_OSC_KEEP_FRAME_SCRATCH.  With it, `scratch` keeps the frame-rate layout (start phase of every
 *                  frame) that ddsp_osc_backward re-walks: set it when the scratch goes to the backward.  Without it the
 *                  forward is free to take the chunked form (power-of-two hops >= 64), whose scratch the backward cannot
 *                  use (it then returns NaN gradients, not an error code).
 * Inputs are not modified.  Requires T*hop < 2^24 (exact fp32 sample indices).
 */
#define DDSP_OSC_KEEP_FRAME_SCRATCH 1u
int ddsp_osc_forward_ex(const float *f0, const float *c, const float *a, float *y, void *scratch,
                        const float *live_in, float *live_out, float *dbg_phi,
                        int B, int T, int H, int hop, int sample_rate, unsigned flags, void *stream);

/*
 * Filtered noise (filtered_noise.py:40-53) and its backward.  Both draw the same noise from the same arguments:
 *   uniform [B,T,hop]  nullable: the U[0,1) draw (what torch.rand returned, filtered_noise.py:44-48).
 *                      NULL => drawn on the device with Philox4x32-10 from `seed`, starting at counter
 *                      offset + *counter_dev; that stream is NOT the torch CPU generator's (documented in DESIGN.md).
 *   counter_dev        nullable (NULL counts as 0): a device uint64, only read, at launch time.  The caller advances it
 *                      between calls, e.g. by a node of the same hipGraph: a replayed graph then draws fresh noise every time.
 *                      uniform and counter_dev exclude each other (both non-NULL: DDSP_EINVAL).
 *   workspace          nullable: device memory of workspace_bytes, 16-byte aligned, contents undefined before and after.
 *                      ddsp_noise_workspace_bytes is 0 for the shapes that have no use for one; for the reference's default shape
 *                      (195 bands at hop 512, config/default.py:15,19: 2(F-1) = 388 has no radix-2 transform) at >= 512 frames
 *                      it holds the cosine operand and the impulse responses of the whole batch, which are then ONE split-bf16
 *                      matrix-core product (csrc/ddsp_noise_ir.hip) instead of F x S/4 cosine sums per frame pair: 2x faster
 *                      end to end at large batches (the forward takes it from 4 096 frames on, the backward from 512: below,
 *                      the extra launches cost more than the sums).  A NULL or too small workspace keeps the sums (same
 *                      results within rounding).
 *
 * ddsp_noise_forward_ws   Hmag [B,T,F] filter magnitudes -> y [B, T*hop]; per frame: zero-phase IR (irfft, length 2(F-1)),
 *                         periodic-Hann window, re-wrapped to hop samples (cropped when hop < 2(F-1)), then the first hop
 *                         samples of the linear convolution with uniform noise in [-1,1); frames are concatenated.
 *                         accumulate != 0: y += noise instead of y = noise (fuses decoder.py:132 `harmonics + noise`).
 * ddsp_noise_backward_ws  gradient w.r.t. Hmag (autograd of filtered_noise.py:40-53; the noise draw is a constant):
 *                         grad_y [B,T*hop] -> grad_H [B,T,F].  `uniform`, `seed`, `offset` and the value *counter_dev holds
 *                         must be the forward call's (a caller that owns the counter advances it only after both), so that
 *                         the backward sees the same draw as the forward.  For the default shape with a workspace the
 *                         correlation runs in the in-LDS FFT form and dH = dz C^T is one matrix-core product, instead of
 *                         the direct kernels' F x S/2 cosine sums per frame.  The workspace need not be the forward's.
 */
size_t ddsp_noise_workspace_bytes(int B, int T, int F, int hop);
int ddsp_noise_forward_ws(const float *Hmag, const float *uniform, float *y, int B, int T, int F, int hop, uint64_t seed,
                          uint64_t offset, const uint64_t *counter_dev, int accumulate, void *workspace, size_t workspace_bytes,
                          void *stream);
int ddsp_noise_backward_ws(const float *grad_y, const float *uniform, float *grad_H, int B, int T, int F, int hop, uint64_t seed,
                           uint64_t offset, const uint64_t *counter_dev, void *workspace, size_t workspace_bytes, void *stream);

/*
 * Filtered noise with overlap-add (csrc/ddsp_noise_ola.hip): an opt-in beside the reference's truncated
 * form above, chosen by the caller.  Same arguments, same draw (uniform, or seed / offset / counter_dev with the counter rule
 * offset + *counter_dev + frame ceil(hop / 4) + quad, frame = b T + t), so one (seed, offset) gives both forms the same samples.
 * With M = 2 (F - 1), N = T hop:
 *   1. x[b, t hop + j] = fl32(2 u[b, t, j] - 1).
 *   2. h_t[e] = (1/2 + 1/2 cos(2 pi e / M)) (1/M) sum_{k<F} c_k H_t[k] cos(2 pi k e / M) for e in [-M/2, M/2), c_0 = c_{F-1} = 1,
 *      c_k = 2 otherwise: the windowed zero-phase response before the reference pads or crops it.  h_t[-M/2] = 0 by its window
 *      weight; that tap is never evaluated.  h_t is even over the others.
 *   3. y[b, n] = sum_e h_{floor((n - e) / hop)}[e] x[b, n - e] over the e with 0 <= n - e < N: every noise sample is filtered by
 *      the response of its own frame, and each frame's hop + M - 1 samples are overlap-added at their place.  Frames outside the
 *      clip contribute nothing.  accumulate != 0: y += noise, bit-equal to adding the plain result to y in fp32.
 *   4. Backward (the draw is a constant; g = grad_y, 0 outside [0, N)): q_t[e] = sum_{j<hop} x[t hop + j] g[t hop + j + e],
 *      grad_H[t, k] = (c_k / M) sum_e (1/2 + 1/2 cos(2 pi e / M)) cos(2 pi k e / M) q_t[e].
 *   5. A non-finite H_t reaches the samples [t hop - M/2 + 1, (t + 1) hop + M/2 - 2] of its row inside [0, N) and nothing else;
 *      a non-finite g[n] reaches the frames t with n in that interval.
 * Every output is one chain of fp32 multiply-adds in a fixed order (y over ascending source sample, q over ascending j), so a
 * row's bits depend neither on the batch nor on the run.  No float atomics, nothing allocated or synchronised: two launches each
 * way.  workspace: ddsp_noise_ola_workspace_bytes(B, T, F, hop) bytes (the responses, or the folded correlations, of every
 * frame), required; the pointers need 4-byte alignment only.  Range: 2 <= F <= 257, 1 <= hop <= 1024, B T <= 2^31 - 1 and
 * T hop < 2^31 - 8192, DDSP_ERANGE beyond (the size query then returns 0); a null pointer, a size that is not positive or a
 * workspace that is too small is DDSP_EINVAL before anything touches the device; B == 0 returns 0.
 */
size_t ddsp_noise_ola_workspace_bytes(int B, int T, int F, int hop);
int ddsp_noise_ola_forward(const float *Hmag, const float *uniform, float *y, int B, int T, int F, int hop, uint64_t seed,
                           uint64_t offset, const uint64_t *counter_dev, int accumulate, void *workspace, size_t workspace_bytes,
                           void *stream);
int ddsp_noise_ola_backward(const float *grad_y, const float *uniform, float *grad_H, int B, int T, int F, int hop, uint64_t seed,
                            uint64_t offset, const uint64_t *counter_dev, void *workspace, size_t workspace_bytes, void *stream);

/*
 * The overlap-add noise as a stream: one block of T frames (n_b = T hop samples; T may change from call to call) per call, for the
 * real-time callback.  The response is zero-phase: y[n] depends on sources up to n + P - 1 (P = F - 1, M = 2 P), so the stream runs
 * D = P - 1 = F - 2 samples late, the smallest delay at which every emitted sample is complete, and the accumulated input `dry`
 * (the harmonics) is delayed by the same D.  With y the definition above extended to all integer n over the sources m >= 0 of the
 * concatenated blocks:
 *   stream[i] = y[i - D] + dry[i - D]      (dry[< 0] = 0; the first D samples hold the pre-ring y[-D .. -1] the offline form crops)
 * and a call returns the next n_b samples of it in out [B, n_b].
 *   state_in / state_out [B, 3F - 6]  per row M - 2 floats of tail -- the partial sums, over the sources so far, of the next M - 2
 *                      stream samples -- then D floats of dry history (the last D samples of dry).  All zeros start a stream.  Two
 *                      distinct buffers (workgroups read what others overwrite); F == 2 has no state and both may be NULL.  A tail
 *                      longer than the block is shifted and continued.
 *   dry [B, n_b]       nullable: NULL emits the noise alone (nothing is added, zeros enter the history).  Must not be `out`.
 *   draw               as above with frame = b T + t: for one row, advancing offset (or *counter_dev) by T ceil(hop / 4) per call
 *                      draws the samples of one long clip; a block needs no sample of an earlier block.
 * Every y[n] stays ONE chain of fp32 multiply-adds over ascending source sample: a block starts each chain from the tail's value
 * instead of 0 and stores it to out (plus the delayed dry value: one fp32 add) or to the new tail.  So the streamed blocks equal,
 * bit for bit, ddsp_noise_ola_forward on the concatenated controls behind leading silent frames (H = 0), shifted by D.  A
 * non-finite H_t reaches the stream samples [t hop, (t + 1) hop + M - 3] of its row and nothing else, across calls; after that the
 * state is finite again.  Two launches, no atomics, nothing allocated or synchronised.  workspace, range and error order as
 * ddsp_noise_ola_forward; out == dry, state_in == state_out or a null state pointer with F > 2 is DDSP_EINVAL before anything
 * touches the device.  ddsp_noise_ola_stream_state_floats: 3F - 6 per row; 0 for F < 3 or F out of range.
 */
size_t ddsp_noise_ola_stream_state_floats(int F);
int ddsp_noise_ola_stream(const float *Hmag, const float *uniform, const float *dry, float *out, const float *state_in,
                          float *state_out, int B, int T, int F, int hop, uint64_t seed, uint64_t offset, const uint64_t *counter_dev,
                          void *workspace, size_t workspace_bytes, void *stream);

/*
 * Backward of ddsp_osc_forward_ex w.r.t. c and a (autograd of harmonic_oscillator.py:24-62; f0 carries no gradient,
 * decoder.py:105).  `fwd_scratch` is the scratch buffer the matching ddsp_osc_forward_ex call filled with
 * DDSP_OSC_KEEP_FRAME_SCRATCH (same B,T,H,hop, sample_rate, same tiling); `bwd_scratch` >= ddsp_osc_backward_scratch_bytes(B,T,H).
 *   grad_y [B,T*hop] -> grad_c [B,T,H], grad_a [B,T,1]
 */
size_t ddsp_osc_backward_scratch_bytes(int B, int T, int H);
int ddsp_osc_backward(const float *grad_y, const float *f0, const float *c, const float *a, const void *fwd_scratch,
                      void *bwd_scratch, float *grad_c, float *grad_a, int B, int T, int H, int hop, int sample_rate,
                      void *stream);

/*
 * Tuning hook (benchmarks only): force the number of harmonics each lane keeps in registers
 * (one of 4,8,12,13,15,16,20,23,25); 0 restores the automatic choice.  Process-global, not
 * thread-safe; results are identical for every setting.
 */
int ddsp_osc_set_tiling(int harmonics_per_lane);
/* Test / tuning hook: 1 = frame kernels for every shape (the round 1-3 decomposition, one lane group per frame), 0 = automatic
 * (chunked form where it applies and the batch fills the row blocks to >= 88 %), 2 = chunked form for every eligible shape
 * whatever the batch (tests of small batches).  Same results within rounding. */
int ddsp_osc_set_path(int path);
/* What ddsp_osc_forward_ex (flags 0) would launch for this shape on the current device (HOST array of >= 8 ints): out[0] harmonics per
 * lane, [1] lanes per row group, [2] 1 = chunked form, then its [3] chunk length in samples, [4] chunks per row,
 * [5] row blocks, [6] compute units and [7] resident workgroups per unit the chunk length was sized for. */
int ddsp_osc_plan(int B, int T, int H, int hop, int sample_rate, int *out, int cap);
/* Diagnostic, SYNCHRONISES `stream`: the shader clock (GHz) one wavefront of the synth kernel of the LAST ddsp_osc_forward_ex
 * on `scratch` (same B, T, H, hop, sample_rate, same hooks) ran at: in-kernel shader-clock ticks over 100 MHz wall-clock
 * ticks between that wavefront's start and end.  ghz is a HOST pointer; 0.0 if the kernel did not run.  Not for launch paths. */
int ddsp_osc_clock(const void *scratch, int B, int T, int H, int hop, int sample_rate, double *ghz, void *stream);

/* Wavefronts per CU (1..8; 0 = the default, 4) of the hop-128 / 65-band noise kernel's persistent grid.  A production knob, not a
 * test hook: at the eight that fit, the kernel's power density makes an MI355X drop its shader clock for the ~25 ms that follow,
 * which costs the kernels around it more than the noise kernel gains; where the clock gives way differs from box to box (between
 * 4 and 8).  The default is safe on every box measured; a caller may measure its own box (the Python package's
 * calibrate_noise_residency) and set more.  Results are bit-identical whatever the value.  Process-global, read once per launch. */
int ddsp_noise_set_residency(int waves_per_cu);
int ddsp_noise_get_residency(void);
/* Test hook (DDSP_EPERM unless DDSP_TEST_HOOKS=1 was set when the library was loaded): the convolution stage of that kernel alone, on
 * one group of 16 frames, for tests/test_gpu_noise_conv_stage.py.  k (taps), x (noise) and y are device memory, [16][128] floats:
 * y[b][n] = sum_{m <= n} k[b][m] x[b][n - m], every output one fused multiply-add chain in fp32 (csrc/ddsp_noise_conv_plan.h).  The
 * kernel puts k and x into the two LDS tiles, runs the production kernel's own convolution and staging code and copies the staging
 * tile out; it does no arithmetic of its own.  A null pointer: DDSP_EINVAL.  One launch of one wavefront on `stream`. */
int ddsp_noise_conv_probe(const float *k, const float *x, float *y, void *stream);

/* Test / tuning hook (process-global, read once per launch): bit 0 forces the generic one-frame-per-workgroup noise kernels
 * (any hop) instead of the batched ones (hop % 8 == 0, tile fits LDS); bit 1 keeps the direct (time-domain) forms where the
 * in-LDS FFT form would run (hop 512 with 2(F-1) <= hop); bit 2 takes the FFT form for hop 256 too (correct, not faster);
 * bit 3 keeps the batched kernel where the wavefront-private form would run (hop 128, 65 bands); bit 4 keeps the cosine sums
 * where a workspace would give the matrix product;
 * (l + 1) << 8 forces 64 >> l frames per workgroup in the batched forward kernel (l = 0..3); 0 restores the defaults.
 * Same results within rounding. */
int ddsp_noise_set_generic(int on);

/*
 * Per-kernel timing with HIP events recorded on the launch stream (bench.py's roofline leg).
 *   ddsp_profile_enable(capacity)  capacity > 0: pre-create that many event pairs and start recording one
 *                                  pair around every kernel launch; capacity <= 0: stop and free them.
 *   ddsp_profile_read(ids, ms, cap) HOST arrays; waits for the recorded events, returns how many records were
 *                                  written (kernel id: 1 frame totals, 2 superblock scan, 3 synth, 4 noise;
 *                                  5 the 195-band noise product; elapsed milliseconds) and resets the pool.  Never called
 *                                  from a launch path.
 *   ddsp_profile_select(mask)      record only the kernels whose id bit is set (0: all, the default).  An event pair costs the
 *                                  stream ~4 us: bench.py records only the dominant kernel inside its timed region.
 */
int ddsp_profile_enable(int capacity);
int ddsp_profile_select(unsigned kernel_mask);
int ddsp_profile_read(int *kernel_ids, float *ms, int cap);

/*
 * Recurrence of the control network's GRU (model/autoencoder/decoder.py:60-65 builds
 * nn.GRU(2*width, units, layers, batch_first=True); :91 runs it).  One persistent launch
 * per direction replaces the ~20 library launches per time step of the stock path; the input projection
 * gi = x W_ih^T + b_ih (and the weight-gradient GEMMs) stay library GEMMs on the caller's side.
 * Single layer, unidirectional, gate order r|z|n as in torch; fp32; Hd <= 512.
 *
 *   ddsp_gru_scratch_bytes(B, Hd)   device scratch for either direction (status word + hand-off granules)
 *   ddsp_gru_max_batch(Hd, backward) rows one launch accepts on the current device (callers split larger
 *                                   batches: rows are independent); 0 if Hd is unsupported
 *   ddsp_gru_forward   gi [B,T,3Hd], w_hh [3Hd,Hd], b_hh [3Hd] (nullable), h0 [B,Hd] (nullable = zeros)
 *                      -> y [B,T,Hd] (all h_t), hT [B,Hd]; gates [B,T,3Hd] and hn [B,T,Hd] (both nullable
 *                      together) receive r|z|n and W_hn h_{t-1} + b_hn for the backward
 *   ddsp_gru_backward  dy [B,T,Hd], dhT [B,Hd] (nullable) + the forward's tensors
 *                      -> d_gi [B,T,3Hd] (gradient of gi), d_gh [B,T,3Hd] (gradient of W_hh h + b_hh), dh0 [B,Hd]
 *   ddsp_gru_status    HOST int*: 0, or 1 if a workgroup gave up waiting for its peers (outputs are then NaN);
 *                      synchronous copy, tests / diagnostics only
 * The grid is sized to be co-resident (one workgroup per CU) and checked against the runtime's occupancy answer
 * (DDSP_ERANGE if it could not be); launches of one process on one device are ordered behind each other on the device
 * (event wait on the launching stream; not inside a stream capture); every wait inside is bounded (2 s): on a time-out
 * the status word is raised and every output of the unfinished steps is NaN.
 */
size_t ddsp_gru_scratch_bytes(int B, int Hd);
int ddsp_gru_max_batch(int Hd, int backward);
int ddsp_gru_forward(const float *gi, const float *w_hh, const float *b_hh, const float *h0, float *y, float *hT,
                     float *gates, float *hn, void *scratch, int B, int T, int Hd, void *stream);
int ddsp_gru_backward(const float *dy, const float *dhT, const float *w_hh, const float *h0, const float *y,
                      const float *gates, const float *hn, float *d_gi, float *d_gh, float *dh0, void *scratch,
                      int B, int T, int Hd, void *stream);
int ddsp_gru_status(const void *scratch, int *status_host);
/* The same recurrences for torch.autocast callers (train/train.py:50 `precision=16`): the products h W_hh^T (forward) and
 * (dr, dz, dhn) W_hh (backward) run on the matrix cores in bf16 with fp32 accumulation (v_mfma_f32_16x16x32_bf16), every
 * tensor at the boundary, the gate arithmetic and the hand-off stay fp32.  At most 16 rows per group: ddsp_gru_max_batch(Hd, 2)
 * rows per launch.  Results differ from the fp32 entry points at bf16 precision (~1e-3).
 * Backward io_type (ABI 3): 0 = fp32 arrays as above; DDSP_IO_BF16 (= 1) = `d_gi` / `d_gh` are written as bf16 arrays -- what the
 * autocast GEMMs behind the recurrence consume, so that no cast pass runs on them. */
int ddsp_gru_forward_bf16(const float *gi, const float *w_hh, const float *b_hh, const float *h0, float *y, float *hT,
                          float *gates, float *hn, void *scratch, int B, int T, int Hd, void *stream);
int ddsp_gru_backward_bf16(const float *dy, const float *dhT, const float *w_hh, const float *h0, const float *y,
                           const float *gates, const float *hn, void *d_gi, void *d_gh, float *dh0, void *scratch,
                           int B, int T, int Hd, int io_type, void *stream);
/* Test hooks (process-global bit mask; 0 restores the default).  Bit 0: deal every group's workgroups over all XCDs (odd
 * blockIdx modulus) instead of keeping a group on one XCD -- bitwise the same results either way (placement only changes
 * speed).  Bit 1: fault injection -- workgroup 0 withholds its publishes from step ddsp_gru_set_fault_step() on and the
 * spin bound drops to 20 ms, so that the time-out path (status word, NaN in every unfinished output) can be tested. */
int ddsp_gru_set_mode(int mode);
int ddsp_gru_set_fault_step(int step);

/*
 * The FIRST block of the f0 / loudness stacks (model/autoencoder/decoder.py:9-39 with n_input = 1, :43-44):
 * Linear(1 -> D) -> LayerNorm -> LeakyReLU as one pass each way.  x [rows] fp32 (the one input feature), w [D] (the Linear's
 * [D, 1] weight), bias [D]; y [rows, D] in io_type (0 fp32, DDSP_IO_BF16, DDSP_IO_F16); mean / rstd [rows] kept for the backward.
 * The backward returns the four parameter gradients (fp32, deterministically summed) and NO input gradient -- callers whose
 * x requires one use the separate Linear and ddsp_ln_lrelu_*.  D = 256 or 512 (DDSP_ERANGE otherwise).
 * scratch >= ddsp_outer_ln_lrelu_scratch_bytes(D).
 */
size_t ddsp_outer_ln_lrelu_scratch_bytes(int D);
int ddsp_outer_ln_lrelu_forward(const float *x, const float *w, const float *bias, const float *gamma, const float *beta, void *y,
                                float *mean, float *rstd, long rows, int D, float eps, float slope, int io_type, void *stream);
int ddsp_outer_ln_lrelu_backward(const void *grad_y, const float *x, const float *w, const float *bias, const void *y,
                                 const float *gamma, const float *mean, const float *rstd, float *grad_w, float *grad_bias,
                                 float *grad_gamma, float *grad_beta, void *scratch, long rows, int D, float slope,
                                 int io_type, void *stream);

/*
 * Column sums of a row-major [M, N] matrix (fp32 io_type 0, bf16 DDSP_IO_BF16, fp16 DDSP_IO_F16) -> out [N] fp32: the bias
 * gradient of the control network's dense layers (decoder.py:9-39, :60-72), deterministic.  scratch: ddsp_colsum_scratch_bytes(N).
 */
size_t ddsp_colsum_scratch_bytes(int N);
int ddsp_colsum(const void *x, float *out, void *scratch, long M, int N, int io_type, void *stream);

/*
 * Framing of the multi-scale spectral loss (loss/mss_loss.py:11-33 on torch.stft semantics: center=True, reflect padding,
 * window of n_fft taps, frames = 1 + N / hop): everything around the batched library FFT of one scale.
 *   ddsp_stft_frames           x [B,N] -> frames [B, frames, n_fft] = x[reflect(f*hop + j - n_fft/2)] * window[j], contiguous
 *   ddsp_stft_frames_backward  grad_frames -> grad_x [B,N]: overlap-add and the padding's adjoint as a gather (deterministic;
 *                              accumulate != 0 adds to grad_x)
 * n_fft % 4 == 0, n_fft <= 8192, N > n_fft / 2.
 */
int ddsp_stft_frames(const float *x, const float *window, float *frames, long B, long N, int n_fft, int hop, void *stream);
int ddsp_stft_frames_backward(const float *grad_frames, const float *window, float *grad_x, long B, long N, int n_fft, int hop,
                              int accumulate, void *stream);

/*
 * One whole scale of the multi-scale spectral loss (loss/mss_loss.py:17-31: spectrogram of both signals, mean |P - Q| +
 * alpha * mean |log2(Q + eps) - log2(P + eps)|) in one kernel, transforms included (in-LDS FFTs; n_fft a power of two in
 * [64, 2048], L > n_fft / 2, torch.stft center / reflect semantics with the given window and hop):
 *   out3        {loss, linear term, log term} of this scale
 *   grad_frames nullable; [B * (1 + L / hop), n_fft] = d loss / d (windowed frame of x_pred), to be folded back onto the
 *               waveform with ddsp_stft_frames_backward (which applies the window)
 *   scratch     ddsp_mss_scale_scratch_bytes() bytes
 * eps must be a normal positive float (>= 1.1754944e-38; the kernels take the hardware log2 / reciprocal of P + eps), else
 * DDSP_EINVAL.  The window is read as [n_fft] floats (8-byte aligned for n_fft = 2048).
 */
size_t ddsp_mss_scale_scratch_bytes(void);
int ddsp_mss_scale_supported(int n_fft);
int ddsp_mss_scale(const float *x_pred, const float *x_true, const float *window, float *grad_frames, void *scratch, float *out3,
                   long B, long L, int n_fft, int hop, float alpha, float eps, void *stream);

/*
 * Reverb (model/ddsp/reverb.py:8-49).  noise [length], t [length] (seconds), decay / wet: one device
 * float each (the module's parameters, read on the device: nothing is synchronised).
 *
 * ddsp_reverb_impulse          build_impulse (:24-29) written straight into the buffer the convolution wants: taps
 *                              [0, min(length, n_out)) = noise * exp(-softplus(-decay) * t * 500) * sigmoid(wet) with tap 0
 *                              forced to 1 (:28), zeros up to n_out -- i.e. `F.pad(impulse, (0, n_out - length))` of :34,
 *                              which CROPS when n_out < length.
 * ddsp_reverb_impulse_backward gradient of the first n_used (<= length) taps w.r.t. noise [length] (zero where cropped and
 *                              at tap 0), decay and wet (one float each); deterministic.
 * ddsp_spectral_mul            y[r,f] = x[r,f] * k[f] on interleaved re/im spectra ([rows, bins] x [bins]): the product of
 *                              fft_convolve (filtered_noise.py:28-30) with one kernel shared by the rows.  The 2N-point real
 *                              transforms themselves stay library FFTs on the caller's side.
 * ddsp_spectral_mul_backward   gk[r,f] = g[r,f] conj(k[f]) (-> irfft -> grad of the signal; nullable) and
 *                              s[f] = sum_r g[r,f] conj(x[r,f]) (-> irfft -> grad of the kernel; nullable, rows summed in order).
 * ddsp_reverb_live             live_forward (:40-49): history_out = [history_in[n:], x]; y[j] = the last n samples of the
 *                              causal convolution of that window with the impulse, computed directly (n x length
 *                              multiply-adds, no FFT).  x [n], y [n], history_* [length], history_out must not alias
 *                              history_in; scratch >= ddsp_reverb_live_scratch_bytes(length, n); n <= length.
 */
int ddsp_reverb_impulse(const float *noise, const float *decay, const float *wet, const float *t, float *impulse,
                        int length, int n_out, void *stream);
int ddsp_reverb_impulse_backward(const float *grad_impulse, const float *noise, const float *decay, const float *wet,
                                 const float *t, float *grad_noise, float *grad_decay, float *grad_wet, int length,
                                 int n_used, void *stream);
int ddsp_spectral_mul(const float *x_ri, const float *k_ri, float *y_ri, long rows, long bins, void *stream);
int ddsp_spectral_mul_backward(const float *g_ri, const float *x_ri, const float *k_ri, float *gk_ri, float *s_ri,
                               long rows, long bins, void *stream);
size_t ddsp_reverb_live_scratch_bytes(int length, int n);
int ddsp_reverb_live(const float *x, const float *history_in, float *history_out, const float *noise, const float *decay,
                     const float *wet, const float *t, float *y, void *scratch, int length, int n, void *stream);

/*
 * One scale of the multi-scale spectral loss (loss/mss_loss.py:11-33: L1 of the power spectrograms + alpha * L1 of their
 * log2) fused into one pass over the two complex STFTs (interleaved re/im, n_bins complex bins each), with the
 * gradient w.r.t. the predicted STFT produced in the same pass (grad_ri nullable).  out3 (device) = {loss, linear term,
 * log term}; scratch >= ddsp_spectral_loss_scratch_bytes().  Deterministic summation.  The STFTs stay library FFTs.
 */
size_t ddsp_spectral_loss_scratch_bytes(void);
int ddsp_spectral_loss(const float *pred_ri, const float *true_ri, float *grad_ri, void *scratch, float *out3,
                       long n_bins, float alpha, float eps, void *stream);

/*
 * The control heads' output non-linearity (model/autoencoder/decoder.py:110-116): y = 2 * sigmoid(x)^2.3026 + 1e-7 over n
 * fp32 elements, and its backward grad_x = grad_y * dy/dx (x is the forward's input), one elementwise pass each.
 */
int ddsp_scaled_sigmoid_forward(const float *x, float *y, long n, void *stream);
int ddsp_scaled_sigmoid_backward(const float *x, const float *grad_y, float *grad_x, long n, void *stream);
/* The controller's three heads (decoder.py:96-100) after ONE GEMM on their concatenated weights: modified_sigmoid of x
 * [rows, n0+n1+n2] (io_type 0 fp32, 1 bf16, 2 fp16: the GEMM's output type) written as three dense fp32 tensors [rows,n0],
 * [rows,n1], [rows,n2]; the backward takes their three fp32 gradients and writes grad_x in x's type. */
int ddsp_heads_sigmoid_forward(const void *x, float *out0, float *out1, float *out2, long rows, int n0, int n1, int n2,
                               int io_type, void *stream);
int ddsp_heads_sigmoid_backward(const void *x, const float *g0, const float *g1, const float *g2, void *grad_x, long rows,
                                int n0, int n1, int n2, int io_type, void *stream);

/*
 * LayerNorm followed by LeakyReLU over rows of D = 256, 512, 768 or 1024 fp32 elements (the MLP blocks of
 * model/autoencoder/decoder.py:9-39 after their Linear): y = lrelu(gamma * (x - mean) * rstd + beta); the forward keeps
 * mean / rstd per row for the backward, which returns grad_x and (deterministically summed) grad_gamma / grad_beta -- and, when
 * grad_xsum is not null (ABI 3), the column sums of grad_x [D]: the bias gradient of the Linear in front of the block, which then
 * needs no pass of its own.  scratch >= ddsp_ln_lrelu_scratch_bytes(D).
 */
size_t ddsp_ln_lrelu_scratch_bytes(int D);
int ddsp_ln_lrelu_forward(const float *x, const float *gamma, const float *beta, float *y, float *mean, float *rstd,
                          long rows, int D, float eps, float slope, void *stream);
int ddsp_ln_lrelu_backward(const float *grad_y, const float *x, const float *y, const float *gamma, const float *mean,
                           const float *rstd, float *grad_x, float *grad_gamma, float *grad_beta, float *grad_xsum, void *scratch,
                           long rows, int D, float slope, void *stream);
/* The same passes on 16-bit activations (io_type: DDSP_IO_BF16 / DDSP_IO_F16) for torch.autocast callers: x, y and their
 * gradients are bf16 / fp16 arrays (read and written as such: no cast pass on either side), gamma / beta, the row
 * statistics, the parameter gradients and all arithmetic stay fp32.  Reference: train/train.py:50 (`precision=16`). */
#define DDSP_IO_BF16 1
#define DDSP_IO_F16 2
int ddsp_ln_lrelu_forward_16(const void *x, const float *gamma, const float *beta, void *y, float *mean, float *rstd,
                             long rows, int D, float eps, float slope, int io_type, void *stream);
int ddsp_ln_lrelu_backward_16(const void *grad_y, const void *x, const void *y, const float *gamma, const float *mean,
                              const float *rstd, void *grad_x, float *grad_gamma, float *grad_beta, float *grad_xsum, void *scratch,
                              long rows, int D, float slope, int io_type, void *stream);

/*
 * Audio encoder (model/autoencoder/encoder.py, crepe/crepe.py): everything around the CREPE convolutions (MIOpen) and its
 * classifier GEMM (rocBLAS).  All fp32, dense row-major.
 *
 * ddsp_resample      polyphase windowed-sinc resampler (torchaudio.transforms.Resample(orig, new) with its defaults, applied
 *                    at encoder.py:57), rates already reduced by their gcd: x [B, L] -> y [B, ceil(nw * L / orig)],
 *                    y[b, j] = sum_t table[r, t] * x[b, q * orig + first[r] + t]  (r = j mod nw, q = j div nw, x = 0 outside
 *                    [0, L)).  table [nw, ntaps] and first [nw] (int32) are the kernel matrix's taps inside the sinc's support,
 *                    built by the caller; nw * ntaps <= 16384 (DDSP_ERANGE otherwise).  Equal rates are the caller's identity.
 * ddsp_crepe_frames  CREPE's normalisation and framing (encoder.py:60-72, crepe.py:119): y [B, Lr] -> stats [B, 2] (mean,
 *                    unbiased std of each row) and frames [B * T, 254 + 1024 + 254] = (y[b, t * hop + p] - mean) / std inside,
 *                    zero in the margins: conv1's padded input.  (T - 1) * hop + 1024 <= Lr.  A constant row gives NaN frames,
 *                    as the reference does.
 * ddsp_crepe_epilogue one CREPE layer after its bias-free convolution (crepe.py:128-133): conv [N, C, Lc] -> +bias -> ReLU ->
 *                    BatchNorm (eval, eps 1e-3) -> max-pool (2, 1).  last = 0: out [N, C, 31 + Lc / 2 + 32], the next layer's
 *                    padded input; last != 0: out [N, (Lc / 2) * C] at l * C + c, the classifier's rows (crepe.py:101).
 * ddsp_pitch_decode  logits [N, 360] (classifier without bias) -> probabilities [N, 360] = sigmoid(logits + bias) (crepe.py:104),
 *                    bin = torch.argmax (first maximum; a NaN is the maximum and the first NaN wins), f0 = f0_table[bin],
 *                    harmonicity = probabilities[bin], cents = cents_table[bin] (encoder.py:120-128; tables [360] by the caller).
 */
int ddsp_resample(const float *x, const float *table, const int *first, float *y, long B, long L, int orig, int nw, int ntaps,
                  void *stream);
int ddsp_crepe_frames(const float *y, float *stats, float *frames, long B, long Lr, int hop, long T, void *stream);
int ddsp_crepe_epilogue(const float *conv, const float *bias, const float *running_mean, const float *running_var, const float *gamma,
                        const float *beta, float *out, long N, int C, int Lc, int last, void *stream);
int ddsp_pitch_decode(const float *logits, const float *bias, const float *f0_table, const float *cents_table, float *probs, float *f0,
                      float *harmonicity, float *cents, long N, void *stream);

/*
 * Pitch decoders over the probabilities ddsp_pitch_decode wrote.  All fp32, dense row-major; bins are int32.
 *
 * ddsp_pitch_centered  probs [N, 360], center [N] (bins in 0 .. 359; NULL: the frame's own torch argmax, first NaN wins, ties to
 *                    the lower bin) -> with w_i = probs[c + i] for i = -4 .. 4 inside 0 .. 359, else 0:
 *                      cents = (20 c + 1997.3794084376191) + 20 (sum_i i w_i) / (sum_i w_i)   (both sums in ascending i)
 *                      f0 = 10 * 2^(cents / 1200), harmonicity = probs[c], normalized_cents = (20 c + offset) / 7180,
 *                    every probability with its own bin's cents (the reference's pitch_centered pairs them rotated,
 *                    encoder.py:95-118).  NaN probabilities give NaN outputs.  bins_out [N] (may be NULL) receives c.
 * ddsp_pitch_viterbi probs [B, T, 360] -> bins [B, T], the path maximising
 *                      sum_t e_t[s_t] + sum_{t >= 1} log_trans[s_t][s_{t-1} - s_t + 11],   e_t[j] = log(max(probs[t][j], 1e-30))
 *                    (the max drops a NaN), over paths that move at most 11 bins per frame; ties go to the lower predecessor
 *                    and to the lower final state.  log_trans [360, 23], indexed by target bin j and k - j + 11, is the log of
 *                    the caller's transition matrix, -inf where k is outside 0 .. 359.  state_in [B, 360] (NULL: a uniform
 *                    prior) holds scores v of the frame before the first: v_0[j] = e_0[j] + max_k (state_in[k] + log A[k][j]);
 *                    state_out [B, 360] (may be NULL) receives the last frame's scores, which are defined up to one
 *                    constant per row (the kernel re-centres them as it goes).  One launch, no allocation, no host
 *                    synchronisation.  Back-pointers stay in LDS while T <= 446; longer rows need `workspace` of
 *                    ddsp_pitch_viterbi_workspace_bytes(B, T) bytes (0 while they fit; 4-byte aligned).  Rows are independent.
 */
int ddsp_pitch_centered(const float *probs, const int *center, float *f0, float *harmonicity, float *normalized_cents, int *bins_out,
                        long N, void *stream);
size_t ddsp_pitch_viterbi_workspace_bytes(long B, long T);
int ddsp_pitch_viterbi(const float *probs, const float *log_trans, const float *state_in, float *state_out, int *bins, void *workspace,
                       long B, long T, void *stream);

/*
 * Voicing: what follows a pitch decoder.  Per row of T frames, all fp32, dense [B, T]:
 *   f0, normalized   a decoder's frequency and normalised-cents outputs (one pair per frame)
 *   periodicity      its harmonicity
 *   loudness         LoudnessEncoder's units, or NULL: no loudness gate
 *   state_in         [B, 3] = {flag, last_n, last_f0} of the rows' previous blocks, or NULL
 * "Lower median" of (value, frame) pairs: element (count - 1) div 2 in ascending order of value, then of frame.
 *   1. ps[t] = lower median of periodicity[u] (a NaN read as 0) over |u - t| <= (period_window - 1) / 2 inside the row
 *   2. v[t] = true if ps[t] >= upper, false if ps[t] < lower, else v[t - 1]; v[-1] = (flag != 0), false without a state
 *   3. m[t] = v[t] and normalized[t] finite and (no loudness or loudness[t] >= silence; a NaN compares false)
 *   4. for m[t]: u* = the frame of the lower median, by normalized, of the frames |u - t| <= (pitch_window - 1) / 2 with m[u];
 *      the outputs are normalized[u*] and f0[u*], a decoded pair bit for bit
 *   5. for other frames, with a / b the nearest frame with m before / after t (a state whose last_n is not NaN is a frame
 *      at t = -1 with the values last_n, last_f0):
 *        DDSP_VOICING_FILL_NONE         the decoded normalized[t], f0[t]
 *        DDSP_VOICING_FILL_HOLD         the outputs of a, else those of b, else the decoded values
 *        DDSP_VOICING_FILL_INTERPOLATE  with both: w = fl32(t - a) / fl32(b - a), n = n_a + fl32(fl32(n_b - n_a) * w),
 *                                       f0 = fl32(10 * 2^((7180 n + 1997.3794084376191) / 1200)) evaluated in fp64; else as HOLD
 * Outputs: f0_out, normalized_out [B, T]; voiced_out [B, T] bytes = m; periodicity_out [B, T] = ps (may be NULL);
 * state_out [B, 3] (may be NULL) = {v[T - 1], the outputs of the last frame with m, the state's included, else NaN}.
 * No output may alias an input or another output.  The windows are 1, 3, 5, 7 or 9; upper >= lower; anything else, an
 * unknown fill or a missing required pointer is DDSP_EINVAL.  T >= 2^24 (frame distances are formed in fp32) or
 * B T >= 2^31 is DDSP_ERANGE.  One launch, one wavefront per row, no atomics, no allocation, no host synchronisation.  A
 * row's intermediates stay in LDS while T <= 4096; longer rows need `workspace` of ddsp_pitch_voicing_workspace_bytes(B, T)
 * bytes (0 while they fit; 4-byte aligned).  Rows are independent.
 */
#define DDSP_VOICING_FILL_NONE 0
#define DDSP_VOICING_FILL_HOLD 1
#define DDSP_VOICING_FILL_INTERPOLATE 2
size_t ddsp_pitch_voicing_workspace_bytes(long B, long T);
int ddsp_pitch_voicing(const float *f0, const float *normalized, const float *periodicity, const float *loudness,
                       const float *state_in, float *f0_out, float *normalized_out, uint8_t *voiced_out, float *periodicity_out,
                       float *state_out, void *workspace, long B, long T, int period_window, int pitch_window, float upper,
                       float lower, float silence, int fill, void *stream);

/*
 * Conditioning statistics and auto-adjust: the loudness distribution and the mean pitch of the
 * note-on frames of a set of rows, and the map of one performance's loudness and register onto another's.  Dense [rows, T]
 * fp32 inputs; `voiced` [rows, T] bytes or NULL.
 *   on      |loudness| < 2^15 and |cents| < 2^15 (so: both finite) and loudness > silence (-inf: no gate) and
 *           harmonicity >= confidence and (no voiced or voiced != 0); a NaN compares false
 *   cell    floorf(fl32(fl32(loudness - lo) * scale)) clamped to [0, bins - 1], scale = fl32(bins) / fl32(hi - lo)
 *   accum   ddsp_condition_accum_bytes(groups, bins) bytes, 8-byte aligned: uint32 counts [groups, bins], then (at the next
 *           multiple of 8 bytes) int64 sums [groups, 2] = {sum llrintf(cents 2^24), sum llrintf(loudness 2^24)} over the on
 *           frames.  groups = rows (pooled = 0: one workgroup per row, plain stores) or 1 (pooled != 0: workgroups take 1024
 *           frames at a time and merge with integer atomicAdd; the entry point zeroes accum with one hipMemsetAsync first).
 *           Only integers are accumulated: the result does not depend on the order of arrival.
 * ddsp_condition_tables, per group with counts c_b, inclusive cumulative counts C_b and N = C_last, for k = 0 .. Q:
 *   b = the smallest cell with c_b > 0 and Q C_b >= k N;  f = clamp((k N - Q (C_b - c_b)) / (Q c_b), 0, 1) in fp64;
 *   tables[g, k] = fl32(lo + (b + f) (hi - lo) / bins) in fp64, rounded once;  N = 0: NaN.
 *   mean_pitch[g] = sum_cents / (N 2^24), mean_loudness[g] likewise (fp64; NaN for N = 0);  frames[g] = N.
 * ddsp_condition_apply, per row with source tables S (source_groups = 1 or B) and target tables T (target_groups = 1 or B):
 *   a row whose source_frames < min_frames, or whose S or T holds a NaN, is copied through (octave 0);
 *   k = octave_mode OFF: 0, FORCED: `octaves`, AUTO: rint((target_mean_pitch - source_mean_pitch) 7180 / 1200) in fp64 (ties to
 *       even; 0 where that is not finite) clamped to +- max_octaves;
 *   f0_out = ldexpf(f0, k);  cents_out = cents + fl32(k 1200 / 7180);
 *   loudness l: not finite: l.  l < S[0]: m = l + (T[0] - S[0]).  l >= S[Q]: m = l + (T[Q] - S[Q]).  Otherwise with j the largest
 *       index with S[j] <= l (at most Q - 1), d = S[j + 1] - S[j], w = d > 0 ? (l - S[j]) / d : 0.5, m = T[j] + w (T[j + 1] - T[j]).
 *       loudness_out = l + s (m - l), s = strength_rows[row] (when given) or strength.  All fp32, nothing fused, the division
 *       correctly rounded.  S is expected non-decreasing.
 *   octaves_out [B] (int) and frames_out [B] (the row's source_frames) may be NULL.  No output may alias an input.
 * Launches: stats one (and the memset when pooled), tables one, apply one; no allocation, no host synchronisation.
 * DDSP_EINVAL: a missing pointer, bins outside 1 .. 8192, quantiles outside 1 .. 1024, hi <= lo (or a cell scale that is not
 * finite), T <= 0, group counts other than 1 or B, |octaves| or max_octaves beyond 32.  DDSP_ERANGE: rows T >= 2^32, a group of
 * more than 2^24 frames (with |value| < 2^15 that keeps every fixed-point sum below 2^63), or B ceil(T / 256) > 2^23 in apply.  rows = 0 (groups = 0, B = 0)
 * returns 0 without a launch.  ddsp_condition_launch_shape: the statistics pass's grid for this shape (workgroups, and the
 * frames of one unit of work).
 */
#define DDSP_CONDITION_MAX_BINS 8192
#define DDSP_CONDITION_MAX_QUANTILES 1024
#define DDSP_CONDITION_MAX_OCTAVES 32
#define DDSP_CONDITION_OCTAVES_OFF 0
#define DDSP_CONDITION_OCTAVES_AUTO 1
#define DDSP_CONDITION_OCTAVES_FORCED 2
size_t ddsp_condition_accum_bytes(long groups, int bins);
int ddsp_condition_launch_shape(int pooled, long rows, long T, int *blocks, long *unit_frames);
int ddsp_condition_stats(const float *loudness, const float *cents, const float *harmonicity, const uint8_t *voiced,
                         void *accum, long rows, long T, int pooled, int bins, float lo, float hi, float silence,
                         float confidence, void *stream);
int ddsp_condition_tables(const void *accum, float *tables, double *mean_pitch, double *mean_loudness, long *frames,
                          long groups, int bins, int quantiles, float lo, float hi, void *stream);
int ddsp_condition_apply(const float *f0, const float *cents, const float *loudness, const float *source_tables,
                         const double *source_mean_pitch, const long *source_frames, const float *target_tables,
                         const double *target_mean_pitch, const float *strength_rows, float *f0_out, float *cents_out,
                         float *loudness_out, int *octaves_out, long *frames_out, long B, long T, long source_groups,
                         long target_groups, int quantiles, int octave_mode, int octaves, int max_octaves, float strength,
                         long min_frames, void *stream);

/*
 * Auto-tune: how a performance is tuned -- its offset from A440 equal temperament and its key --, and
 * its notes moved onto a scale with vibrato and inflection kept.  Dense [rows, T] fp32 inputs; `voiced` [rows, T] bytes.
 * All positions are int64 counts of 2^-16 cent on the MIDI scale: note m is m S, S = 100 * 65536; A4 is note 69.
 *   1. Position of a frame: u = llrint(fl64(fl64(7180 (double)n) + K) 65536), n the frame's normalized_cents,
 *      K = 1997.3794084376191 - 1200 log2(44) + 6900 = 2346.0614660728625.  The product is exact in fp64: u carries one rounding.
 *   2. A frame is on iff |n| <= 4 (so: finite, and |u| < 2^31), voiced != 0 (where given), harmonicity >= confidence (where
 *      harmonicity is given) and loudness > silence (where loudness is given); a NaN compares false.  Off frames are never
 *      counted, never moved, and end a note.
 *   3. Statistics (pooled: groups = 1; per row: groups = rows): uint32 H[1200], one-cent pitch-class cells each centred on a whole
 *      cent, cell = floor_mod(u + 32768, 12 S) div 65536.  Only integers are accumulated: the same bits for any order, grid or
 *      row permutation.  accum is ddsp_tuning_accum_bytes(groups) = 4800 groups bytes, 8-byte aligned; pooled, the entry point
 *      zeroes it with one hipMemsetAsync and workgroups merge with integer atomicAdd; per row, plain stores.
 *   4. Estimate, per group.  Folded histogram D[d] = sum_p H[100 p + d].  Offset: o in -50 .. 49 minimises
 *      cost(o) = sum_d D[d] min((d - o) mod 100, (o - d) mod 100) (exact int64: the circular median of the deviations from the
 *      semitone grid); ties go to the smaller |o|, then to the non-negative one.  Pitch-class profile
 *      P[p] = sum_{j = -50}^{49} H[(100 p + o + j) mod 1200].  Root: with a scale mask (12 bits, bit i = the degree i semitones
 *      above the root is allowed), root = argmax_r sum_p P[p] bit((p - r) mod 12), ties to the smallest r; forced_root >= 0 is
 *      that root instead.  An empty group (N = 0) gives offset 0, root 0 (or the forced one), frames 0.  Masks: chromatic 0xFFF,
 *      major 0xAB5, minor (natural) 0x5AD, pentatonic 0x295; a zero mask is refused.
 *   5. Snapping, per row, given o, root, mask: v = u - 65536 o; q_t = the allowed note nearest to v_t, ties to the lower note;
 *      note_t = note_{t-1} if frames t and t - 1 are both on and |v_t - note_{t-1} S| <= |v_t - q_t S| + h, else q_t.  h is
 *      `hysteresis` in units, 0 .. 1200 * 65536; equality stays on the old note.
 *   6. A note is a maximal run of on frames with the same note_t, of length L.  With L < min_note_frames its frames get
 *      correction 0.  Otherwise, with DDSP_TUNING_VIBRATO, every frame of the note gets rdiv(note S L - sum v, L) (the note's
 *      centre moves onto the pitch, its vibrato and inflection stay); without, frame t gets note S - v_t (the hard snap).
 *      rdiv(a, b) = floor((2 a + b) / (2 b)).  With DDSP_TUNING_CONCERT the correction of every frame of such a note is
 *      reduced by 65536 o: it lands on A440's grid instead of the performance's own.
 *   7. Glide: for an on frame t the smoothed correction is rdiv(sum of the corrections, count) over the frames |u - t| <= glide
 *      of t's own run of consecutive on frames; glide = 0 gives the correction itself; it never reaches across an off frame.
 *   8. d_t = llrint((double)amount (double)smoothed_t), amount = amount_rows[row] (when given) or `amount`, clamped to [0, 1]
 *      (a NaN: 0).  cents_out = n + fl32((double)d / (65536 * 7180)); f0_out = fl32((double)f0 exp2((double)d / (65536 * 1200)));
 *      frames with d = 0, every off frame included, return n and f0 bit for bit.  notes_out (int, may be NULL) = note_t, or
 *      INT32_MIN for an off frame; correction_out (int, may be NULL) = d_t.
 * ddsp_tuning_apply reads offset and root [groups] (groups = 1 or B) from device memory: what ddsp_tuning_estimate wrote, or
 * hand-made values (an offset is clamped to +-50, a root taken mod 12).  One wavefront per row; a row's intermediates (32 bytes
 * per frame) stay in LDS while T <= DDSP_TUNING_LDS_FRAMES, longer rows need `workspace` of ddsp_tuning_workspace_bytes(B, T)
 * bytes (0 while they fit; 8-byte aligned).  No output may alias an input.
 * Launches: stats one (and the memset when pooled), estimate one, apply one; no allocation, no host synchronisation.
 * DDSP_EINVAL: a missing pointer, T <= 0, a mask outside 1 .. 0xFFF, a forced root outside -1 .. 11, hysteresis outside
 * 0 .. 1200 * 65536, a negative min_note_frames or glide, unknown flags, a NaN silence or confidence, an `amount` outside [0, 1]
 * without amount_rows, group counts other than 1 or B.  DDSP_ERANGE: rows T >= 2^32 or a group of more than 2^24 frames
 * (statistics); T >= 2^24 or B T >= 2^31 (apply).  rows = 0 (groups = 0, B = 0) returns 0 without a launch.
 */
#define DDSP_TUNING_CELLS 1200
#define DDSP_TUNING_LDS_FRAMES 1536
#define DDSP_TUNING_VIBRATO 1
#define DDSP_TUNING_CONCERT 2
size_t ddsp_tuning_accum_bytes(long groups);
int ddsp_tuning_stats(const float *cents, const float *harmonicity, const float *loudness, const uint8_t *voiced, void *accum,
                      long rows, long T, int pooled, float silence, float confidence, void *stream);
int ddsp_tuning_estimate(const void *accum, int *offset, int *root, long *profile, long *frames, long groups, int mask,
                         int forced_root, void *stream);
size_t ddsp_tuning_workspace_bytes(long B, long T);
int ddsp_tuning_apply(const float *f0, const float *cents, const float *harmonicity, const float *loudness, const uint8_t *voiced,
                      const int *offset, const int *root, const float *amount_rows, float *f0_out, float *cents_out, int *notes_out,
                      int *correction_out, void *workspace, long B, long T, long groups, int mask, int forced_root, long hysteresis,
                      long min_note_frames, long glide, int flags, float amount, float silence, float confidence, void *stream);

/*
 * YIN salience on CREPE's bin grid: a second source of the [B, T, 360] array the pitch decoders read.
 * y [B, Lr] fp32 at 16 kHz (what ddsp_resample returns) -> probs [B, T, 360]; frame t of row b is x = y[b, t hop .. t hop + 1024),
 * CREPE's framing without its normalisation.  Per frame, all fp32:
 *   d(tau)  = sum_{j = 0}^{511} (x[j] - x[j + tau])^2, tau = 0 .. 511, terms added in ascending j (each term one FMA on the
 *             rounded difference)
 *   c(tau)  = d(1) + ... + d(tau);  d'(0) = 1, d'(tau) = fl(d(tau) tau) / c(tau) where c(tau) > 0, else 1
 *   bin b:  v = Catmull-Rom through d'(i_b - 1), d'(i_b), d'(i_b + 1), d'(i_b + 2) at w_b,
 *           probs = clip(1 - v - cost_b, 0, 1), and 0 where that is not finite
 * A frame that holds a sample which is not finite is 0 in every bin.
 * bin_table [360, 4] fp32, 16-byte aligned, row b = {i_b, w_b, cost_b, unused}: the integer part (stored as a float; the kernel
 * clamps it to 1 .. 509 so that no table can make it read outside d') and the fraction of the bin's lag 16000 / f_b, and the
 * bin's octave cost, built by the caller in fp64 (encoder.yin_bin_table).
 * (T - 1) hop + 1024 <= Lr, Lr >= 1024 and hop > 0, DDSP_EINVAL otherwise; B Lr or 360 B T beyond 2^60 is DDSP_ERANGE.  One
 * launch, one wavefront per frame (grid-strided beyond 8192 frames), no atomics, no allocation, no host synchronisation;
 * no alignment is assumed of y, its rows or its frames.  Every sum has one order: a frame's result is the same bits from run
 * to run and whatever else is in the batch.
 */
int ddsp_yin_salience(const float *y, const float *bin_table, float *probs, long B, long Lr, int hop, long T, void *stream);

/*
 * Harmonic analysis: the inverse of the oscillator bank (DESIGN.md section 14 has the definition).  All fp32, dense row-major.
 *   audio [B, N], N = T hop;  f0 [B, T] Hz;  voiced [B, T] bytes or NULL
 * With up() the bank's own upsampling (pos = (n + 0.5) / hop - 0.5 clamped to [0, T - 1], linear between frames), f0* = f0 with
 * frames that are not finite or <= 0 set to 0, and theta[n] = sum_{m <= n} up(f0*)[m] / sample_rate in turns:
 *   frame t covers the samples s_t + j, j in [0, W), s_t = t hop - floor((W - hop) / 2), under the periodic Hann window w; samples
 *   outside [0, N) are left out of the sum and of norm_t = sum of the w[j] inside
 *   C[t, k] = (2 / norm_t) sum_j w[j] audio[s_t + j] exp(-2 pi i k theta[s_t + j]),  k = 1 .. H
 *   C[t, k] = 0 where fl32(k f0[t]) > sample_rate / 2 (integer division, as the bank masks), where f0[t] is not finite or <= 0,
 *   and where voiced[t] == 0
 *   amp = |C|, a[t] = sum_k amp[t, k], c[t, k] = amp[t, k] / a[t], and c[t, :] = 1 / H where a[t] == 0
 *   harm[n] = sum_k Re(up(C[:, k])[n] exp(+2 pi i k theta[n])),  resid = audio - harm
 * ddsp_harm_analysis  -> C [B, T, H] interleaved (re, im), a [B, T], c [B, T, H]; it fills `workspace` with theta.
 * ddsp_harm_resynth   C [B, T, H] interleaved (8-byte aligned) -> harm [B, N] and, where resid is not NULL, resid = audio - harm
 *                     (audio may be NULL otherwise).  With DDSP_HARM_PHASE_READY in flags the workspace still holds the theta
 *                     of a ddsp_harm_analysis or ddsp_harm_resynth call with the same f0, B, T, hop and sample_rate, and the
 *                     phase pass is not run again.
 * workspace: ddsp_harm_workspace_bytes(B, T, hop) bytes (0: the sizes are not positive or overflow), 16-byte aligned.  theta is
 * accumulated as 64-bit fixed point and kept per sample as a 32-bit fraction of a turn.  W even, 2 <= W <= 4096, H <= 256, any
 * hop >= 1 and T >= 1: a larger W or H, or sizes beyond 2^56 elements, are DDSP_ERANGE; a null pointer, an odd W or a size that is
 * not positive DDSP_EINVAL; B == 0 returns 0.  Four launches (analysis) or three (resynthesis; one with the flag), no atomics
 * on global memory, no allocation, no host synchronisation; every sum has one order: a row's results are the same bits from
 * run to run and whatever else is in the batch.  A sample that is not finite reaches the frames whose windows hold it and,
 * through them, the samples of `harm` that interpolate those frames; nothing else.
 */
#define DDSP_HARM_PHASE_READY 1u
size_t ddsp_harm_workspace_bytes(long B, long T, int hop);
int ddsp_harm_analysis(const float *audio, const float *f0, const uint8_t *voiced, float *C, float *a, float *c, void *workspace,
                       long B, long T, int hop, int W, int H, int sample_rate, void *stream);
int ddsp_harm_resynth(const float *C, const float *f0, const float *audio, float *harm, float *resid, void *workspace, long B,
                      long T, int hop, int H, int sample_rate, unsigned flags, void *stream);
/*
 * One step of the f0 refinement by frequency reassignment, in the notation above.  Frame t is interior
 * when 0 <= s_t and s_t + W <= N, and alive when f0_in[t] is finite and positive and voiced (nullable) is not 0 there.
 *   For an interior, alive frame, over the harmonics k the mask of the analysis keeps, with w'[j] = (pi / W) sin(2 pi j / W):
 *     C_k = sum_j w[j] audio[s_t + j] exp(-2 pi i k theta[s_t + j]), D_k the same sum with w' in place of w (theta from f0_in),
 *     num = sum_k k Im(D_k conj(C_k)),  den = sum_k k^2 |C_k|^2,  mean = sum_j w[j] up(f0_in*)[s_t + j] / sum_j w[j],
 *     g[t] = mean - (sample_rate / 2 pi) num / den, and g[t] = f0_in[t] where den = 0 or that is not finite.
 *   An alive frame before the first interior frame t_lo gets f0_in[t] g[t_lo] / f0_in[t_lo], one after the last interior frame
 *   t_hi f0_in[t] g[t_hi] / f0_in[t_hi] (the ratio is 1 where that frame is not alive); without an interior frame g = f0_in.
 *   Every alive g[t] is then clamped to f0_anchor[t] 2^(+-max_cents / 1200); a frame that is not alive keeps its bits.
 * -> f0_out [B, T] (not f0_in itself) and, where not NULL, num_out and den_out [B, T] (0 on the frames that are not measured).
 * It runs the phase pass on f0_in and three more launches; same ranges, checks, determinism and capturability as
 * ddsp_harm_analysis; max_cents > 0 and finite, flags = 0.  workspace: ddsp_harm_refine_workspace_bytes(B, T, hop) bytes, 16-byte
 * aligned; its first ddsp_harm_workspace_bytes(B, T, hop) bytes are laid out as the analysis leaves them.
 */
size_t ddsp_harm_refine_workspace_bytes(long B, long T, int hop);
int ddsp_harm_refine(const float *audio, const float *f0_in, const float *f0_anchor, const uint8_t *voiced, float *f0_out,
                     float *num_out, float *den_out, void *workspace, long B, long T, int hop, int W, int H, int sample_rate,
                     float max_cents, unsigned flags, void *stream);

/*
 * Noise analysis: the inverse of ddsp_noise_forward_ws, exact in expectation for the filter that call
 * applies (truncated to the frame, the anti-causal half wrapped, Hann-windowed).  Per row, all fp32, dense row-major:
 *   x [B, N], N = T hop; frame t is the samples [t hop, (t + 1) hop).  F = n_filters >= 2, M = 2 (F - 1), L = F - 1, hop >= M.
 *   1. k = Amat H, Amat [hop x F] = the impulse-response map on unit vectors (irfft, roll by M / 2, periodic Hann of size M, pad
 *      to hop, roll by -M / 2); its non-zero rows are d in [0, M / 2) and [hop - M / 2, hop).
 *   2. a frame of the noise is y[n] = sum_{m <= n} s[m] k[n - m] with s iid uniform(-1, 1), so its expected in-frame
 *      autocorrelation is R(H)[l] = 1/3 sum_{d = 0}^{hop - 1 - l} (hop - l - d) k[d] k[d + l], l in [0, L).
 *   3. r_t[l] = sum_{n = 0}^{hop - 1 - l} x[t hop + n] x[t hop + n + l]; rbar_t = the mean of r_t' over t' in [t - s, t + s]
 *      inside [0, T), s = (average - 1) / 2 (average odd; it may exceed T).
 *   4. P(r)[b] = S(q)[b], q[b] = sum_{l < L} c_l g[l] r[l] cos(pi b l / (F - 1)), c_0 = 1, c_l = 2, g[l] = 1/2 + 1/2 cos(pi l / L),
 *      S the smoothing (1/4, 1/2, 1/4) with mirrored ends (q[-1] = q[1], q[F] = q[F - 2]).
 *   5. p = max(P(rbar_t), 0); H^0 = sqrt(3 p / hop); H^{i + 1} = H^i sqrt(p / max(P(R(H^i)), FLT_MIN)); H = H^iterations >= 0.
 * ddsp_noise_analysis  -> H [B, T, F] and, where power is not NULL, power [B, T, F] = p.
 * workspace: ddsp_noise_analysis_workspace_bytes(B, T, F, hop) bytes (0: sizes that are not positive, overflow or lie outside the
 * range below), 16-byte aligned; the call fills it with its tables and r.  Range: 2 <= F <= 257 and 2 (F - 1) <= hop <= 1024,
 * B T <= 2^31 - 1: anything else is DDSP_ERANGE.  A null x, H or workspace, T, F - 1, hop or iterations + 1 that is not positive,
 * an average that is even or below 1: DDSP_EINVAL, before anything touches the device; B == 0 returns 0.  Three launches, no
 * atomics on global memory, no allocation, no host synchronisation; every sum has one order: a row's results are the same bits
 * from run to run and whatever else is in the batch.  A silent frame gives H = 0.  A sample that is not finite reaches the frames
 * whose averaging window holds its frame, and nothing else.
 */
size_t ddsp_noise_analysis_workspace_bytes(long B, long T, int F, int hop);
int ddsp_noise_analysis(const float *x, float *H, float *power, void *workspace, long B, long T, int F, int hop, int average,
                        int iterations, void *stream);

/*
 * Noise analysis for the overlap-add noise: the inverse of ddsp_noise_ola_forward.  That noise is
 * stationary, so the model has no truncation weights, products may cross frame boundaries and any hop >= 1 is analysable.
 * Arguments, layout, workspace rule and error order are ddsp_noise_analysis's.  F >= 2, M = 2 (F - 1), P = L = F - 1, N = T hop,
 * x[n] = 0 for n >= N:
 *   1. h[e], |e| <= P - 1: the even response ddsp_noise_ola_forward forms from H (its step 2),
 *      h[e] = (1/2 + 1/2 cos(2 pi e / M)) (1/M) sum_{k<F} c_k H[k] cos(2 pi k e / M).
 *   2. with H constant E[y[n] y[n + l]] = 1/3 rho(H)[l], rho(H)[l] = sum_e h[e] h[e + l] (both taps inside |e| <= P - 1); the model
 *      is R_ola(H)[l] = (hop / 3) rho(H)[l], l in [0, L): no truncation weights, hop only a scale.
 *   3. r_t[l] = (hop / c_t[l]) sum_{n < hop, t hop + n + l < N} x[t hop + n] x[t hop + n + l], c_t[l] = clamp(N - t hop - l, 0, hop)
 *      the count of terms (r_t[l] = 0 where it is 0): the expectation is exact at the clip's end too.  A frame whose own samples
 *      are all zero has r_t = 0 exactly.  rbar_t: the frame average of ddsp_noise_analysis (average odd; it may exceed T).
 *   4. P: ddsp_noise_analysis's step 4 unchanged.
 *   5. p = max(P(rbar_t), 0); H^0 = sqrt(3 p / hop); H^{i + 1} = H^i sqrt(p / max(P(R_ola(H^i)), FLT_MIN)); H = H^iterations >= 0.
 *   6. a sample at n that is not finite reaches the frames t with t hop <= n < t hop + hop + L - 1, widened by the averaging
 *      window, and nothing else.
 * workspace: ddsp_noise_analysis_ola_workspace_bytes(B, T, F, hop) bytes (0 outside the range), 16-byte aligned.  Range:
 * 2 <= F <= 257, 1 <= hop <= 1024, B T <= 2^31 - 1, T hop < 2^31 - 8192: anything else is DDSP_ERANGE.  A null x, H or workspace,
 * T, F - 1, hop or iterations + 1 that is not positive, an average that is even or below 1: DDSP_EINVAL, before anything touches
 * the device; B == 0 returns 0.  Three launches, no atomics on global memory, no allocation, no host synchronisation; every sum
 * has one order: a row's results are the same bits from run to run and whatever else is in the batch.
 */
size_t ddsp_noise_analysis_ola_workspace_bytes(long B, long T, int F, int hop);
int ddsp_noise_analysis_ola(const float *x, float *H, float *power, void *workspace, long B, long T, int F, int hop, int average,
                            int iterations, void *stream);

/*
 * Transformation of analysed controls (DESIGN.md section 14b has the definition): time stretch, transposition and formant shift
 * of what ddsp_harm_analysis and ddsp_noise_analysis return.  All fp32, dense row-major; rows are independent.
 *   f0 [B, T] Hz, a [B, T], c [B, T, H], noise [B, T, F] or NULL;  per output frame t' in [0, T_out): pos [B, T_out] a source position
 *   in input frames, ratio [B, T_out] the pitch ratio r, env [B, T_out] the envelope ratio q.
 * Source frame i is voiced where f0[i] is finite and positive.  A[i, k] = a[i] c[i, k] / S_i where frame i is voiced and
 * fl32(k f0[i]) > sample_rate / 2 (integer division, as the bank masks) is false, S_i the sum of c[i, k] over those k; A[i, k] = 0
 * elsewhere and where S_i = 0.  E_i(u) = A[i, 1] for u < 1, (1 - mu) A[i, m] + mu A[i, m + 1] for 1 <= u < H (m = floor(u),
 * mu = u - m), A[i, H] at u = H, 0 beyond.  Output frame t':
 *   p = pos clamped to [0, T - 1] (a NaN counts as 0), i0 = floor(p), i1 = min(i0 + 1, T - 1), lambda = p - i0
 *   f0_out = fl32(fl32(f0_s) r), f0_s = (1 - lambda) f0[i0] + lambda f0[i1] where both are voiced, else the voiced one's f0
 *   A'[k'] = (1 - lambda) E_i0(u) + lambda E_i1(u), u = k' r / q in double, k' = 1 .. H_out; 0 where fl32(k' f0_out) > sample_rate / 2
 *   a_out = sum_k' A', c_out = A' / a_out, and c_out = 1 / H_out where a_out = 0
 *   noise_out[j] = the same two interpolations of noise over lambda and the bands floor(v), floor(v) + 1 at v = j / q, 0 for v > F - 1
 * A frame whose neighbours are both unvoiced has f0_out = 0, a_out = 0, c_out = 1 / H_out (its noise is transformed all the same);
 * a frame whose r or q is not finite or not positive has that and noise_out = 0.
 * -> f0_out [B, T_out], a_out [B, T_out], c_out [B, T_out, H_out], noise_out [B, T_out, F] (NULL exactly when noise is).
 * B == 0 returns 0; a null pointer, noise without noise_out (or the reverse) or a size that is not positive is DDSP_EINVAL;
 * H or H_out > 256, F > 257 (F is ignored but must be positive without noise), B T or B T_out beyond 2^47 frames DDSP_ERANGE.  No
 * workspace, one launch, one wavefront per output frame (grid-strided beyond 8192 workgroups of four), no atomics, no
 * allocation, no host synchronisation; every sum has one order: a frame's results are the same bits from run to run and
 * whatever else is in the batch.  No input, NaN or huge, makes the kernel read or write outside its arrays.
 */
int ddsp_transform_controls(const float *f0, const float *a, const float *c, const float *noise, const float *pos, const float *ratio,
                            const float *env, float *f0_out, float *a_out, float *c_out, float *noise_out, long B, long T,
                            long T_out, int H, int H_out, int F, int sample_rate, void *stream);

/*
 * Morph of two sets of analysed controls (DESIGN.md section 14c has the definition): pitch, spectral envelope and noise bands
 * between those of sound A and sound B.  All fp32, dense row-major; rows are independent.  Per sound X in {a, b}:
 *   f0_X [B, T_X] Hz, a_X [B, T_X], c_X [B, T_X, H_X], noise_X [B, T_X, F] or NULL, pos_X [B, T_out] the source position of every
 *   output frame in X's frames;  mix_f0, mix_amp, mix_noise [B, T_out]: the weight of B for the pitch, the envelope, the bands.
 * A_X[i, k], the amplitudes the bank plays, E_X,i(u), and of pos_X the pair i0, i1 and lambda_X are ddsp_transform_controls'.
 * f_X = fl32((1 - lambda_X) f0_X[i0] + lambda_X f0_X[i1]) where both frames are voiced, else the voiced one's f0; X is present
 * where one of them is voiced.  Output frame t', with the weights w_f, w_h, w_n clamped to [0, 1]:
 *   f0_out = f_a at w_f = 0, f_b at w_f = 1, else fl32(exp2((1 - w_f) log2 f_a + w_f log2 f_b)) in double, kept within
 *            [min(f_a, f_b), max(f_a, f_b)]; with one sound present that sound's f_X; with none 0
 *   u_X = k' (coordinates DDSP_MORPH_HARMONIC) or (double)k' ((double)f0_out / (double)f_X) (DDSP_MORPH_HZ), k' = 1 .. H_out
 *   e_X[k'] = (1 - lambda_X) E_X,i0(u_X) + lambda_X E_X,i1(u_X), 0 where X is not present
 *   A'[k'] = (1 - w_h) e_a + w_h e_b; 0 where fl32(k' f0_out) > sample_rate / 2 (integer division, as the bank masks)
 *   a_out = sum_k' A', c_out = A' / a_out, and c_out = 1 / H_out where a_out = 0
 *   noise_out[j] = (1 - w_n) X_a[j] + w_n X_b[j], X_X[j] = (1 - lambda_X) noise_X[i0, j] + lambda_X noise_X[i1, j]
 * Every combination is (1 - w) x + w y with each product and the sum rounded to fp32: a weight of 0 or 1 selects an input, and
 * with all three at 0 (at 1) the outputs are, on finite and non-negative controls, the bits of ddsp_transform_controls on sound A
 * (B) at pos_a (pos_b) and ratio = env = 1 -- but for f0_out of a frame where that sound is absent and the other present, which is
 * the other's pitch at amplitude 0.  A frame with a weight that is not finite is silent: f0_out = 0, a_out = 0,
 * c_out = 1 / H_out, noise_out = 0.
 * -> f0_out [B, T_out], a_out [B, T_out], c_out [B, T_out, H_out], noise_out [B, T_out, F].  noise_a, noise_b and noise_out are all
 * NULL or all set.  B == 0 returns 0; a null pointer, one or two of the noise pointers, a size that is not positive or
 * coordinates that are neither constant: DDSP_EINVAL; H_a, H_b or H_out > 256, F > 257 (F is ignored but must be positive without
 * noise), B T_a, B T_b or B T_out beyond 2^47 frames: DDSP_ERANGE.  No workspace, one launch, one wavefront per output frame
 * (grid-strided beyond 8192 workgroups of four), no atomics, no allocation, no host synchronisation; every sum has one order: a
 * frame's results are the same bits from run to run and whatever else is in the batch.  No input, NaN or huge, makes the kernel
 * read or write outside its arrays.
 */
#define DDSP_MORPH_HZ 0
#define DDSP_MORPH_HARMONIC 1
int ddsp_morph_controls(const float *f0_a, const float *a_a, const float *c_a, const float *noise_a, const float *pos_a,
                        const float *f0_b, const float *a_b, const float *c_b, const float *noise_b, const float *pos_b,
                        const float *mix_f0, const float *mix_amp, const float *mix_noise, float *f0_out, float *a_out, float *c_out,
                        float *noise_out, long B, long T_a, long T_b, long T_out, int H_a, int H_b, int H_out, int F, int sample_rate,
                        int coordinates, void *stream);

/*
 * Dynamic time warping of two feature sequences (DESIGN.md section 14d has the definition): which frame of A goes with which
 * frame of B, and that path resampled onto an output timeline as the positions ddsp_morph_controls takes.  Rows are independent.
 *   x_a [B, T_a, D], x_b [B, T_b, D] fp32 feature rows.  Every product and sum below is rounded to fp32 on its own.
 *   d(i, j) = sum_k (x_a[i, k] - x_b[j, k])^2, ascending k, one accumulator; a value that is not < +inf (a NaN too) counts as +inf
 *   band: with p = T_a - 1, q = T_b - 1 (64-bit integers), d(i, j) = +inf where |i q - j p| > radius max(p, q); radius 0: no band
 *   D(0, 0) = d(0, 0); D(i, j) = d(i, j) + best, best the first of D(i - 1, j - 1), D(i - 1, j) + penalty, D(i, j - 1) + penalty
 *   (those that exist, in this order) that no later one is strictly below; the chosen one is the cell's back-pointer
 *   path: the back-pointers from (T_a - 1, T_b - 1) to (0, 0), in forward order; cost = D(T_a - 1, T_b - 1)
 *   timeline (fp64): tau = timing clamped to [0, 1], s_k = (1 - tau) i_k + tau j_k, S = s of the end cell; output frame t' targets
 *   s = min(t' S / (T_out - 1), S) (0 for T_out = 1); with k the largest index with s_k <= s the positions are the end cell where
 *   k is the last point, else (i_k, j_k) + lambda (i_k+1 - i_k, j_k+1 - j_k), lambda = (s - s_k) / (s_k+1 - s_k), rounded once to fp32
 * -> pos_a, pos_b [B, T_out] fp32 (monotone, inside [0, T_X - 1]), path [B, T_a + T_b - 1, 2] int32 (entries beyond length are -1),
 * length [B] int32 in [max(T_a, T_b), T_a + T_b - 1], cost [B] fp32.
 * workspace: ddsp_dtw_workspace_bytes(B, T_a, T_b) bytes of device memory for the back-pointers (0 outside the range below).
 * B == 0 returns 0; a null pointer, B < 0, T_a, T_b, D or T_out that is not positive, radius < 0, a penalty that is negative or
 * not finite, a timing that is not finite or a workspace that is too small is DDSP_EINVAL, before anything touches the device;
 * T_a or T_b > 2048, D > 64, B or T_out beyond 2^31 - 1: DDSP_ERANGE.  One launch, one wavefront per row, no atomics, no allocation,
 * no host synchronisation; a row's results are the same bits from run to run and whatever else is in the batch.  No feature
 * value, NaN or huge, reaches an index: the kernel reads and writes inside its arrays whatever they hold.
 */
size_t ddsp_dtw_workspace_bytes(long B, long T_a, long T_b);
int ddsp_dtw_align(const float *x_a, const float *x_b, float *pos_a, float *pos_b, int *path, int *length, float *cost,
                   void *workspace, size_t workspace_bytes, long B, long T_a, long T_b, int D, long T_out, long radius, float penalty,
                   double timing, void *stream);

/*
 * A-weighted loudness (model/autoencoder/encoder.py:131-156): x [B, L] -> out [B, F], F = 1 + (L - n_fft) / hop,
 *   out[b, f] = mean over k = 0 .. n_fft/2 of (20 log10(|X_f[k]| + 1e-20) + a_weight[k]) / 90 + 1
 * with X_f the un-windowed DFT of x[b, f * hop .. f * hop + n_fft) (torch.stft center=False, no window); a_weight [n_fft/2 + 1]
 * float64 (the reference's parameter dtype; each bin's fp32 level plus its weight is rounded to fp32 once, as torch's `+=` does).
 * One kernel, transforms in LDS; n_fft a power of two in [64, 2048] (ddsp_loudness_supported) and L >= n_fft, DDSP_ERANGE
 * otherwise.  Every frame is within 2e-6 of the fp64 value whatever the level of its neighbours (frames that share a packed
 * transform are equalised by powers of two); an all-zero frame gives the value of log10(1e-20) in every bin; a frame with a
 * NaN or an infinite sample is NaN and no other frame is.
 */
int ddsp_loudness_supported(int n_fft);
int ddsp_loudness(const float *x, const double *a_weight, float *out, long B, long L, int n_fft, int hop, void *stream);

/*
 * MFCC front end of the timbre encoder: x [B, L] fp32 -> mfcc [B, F, n_mfcc] and, where `logmel` is not
 * NULL, logmel [B, F, n_mels], F = 1 + (L - n_fft) / hop, in ONE launch.
 *   frame f   = x[f hop .. f hop + n_fft), times the periodic Hann window 0.5 - 0.5 cos(2 pi n / n_fft) (fp64, rounded to fp32)
 *   A[k]      = |FFT(frame)[k]| * scale, k = 0 .. n_fft / 2     (the caller passes scale = 2 / sum of the window)
 *   mel[m]    = sum_i band_w[o_m + i] * A[band_start[m] + i], i = 0 .. band_count[m] - 1 ascending; o_m = the sum of the counts
 *               of the bands before m (the weights are packed band after band); an empty band is legal
 *   logmel[m] = log(mel[m] + floor), the natural logarithm in fp32; a band whose sum is exactly 0 reads fl32(log(floor))
 *   mfcc[j]   = sum_m dct[j n_mels + m] * logmel[m], m ascending
 * A frame with a NaN or an infinite sample is NaN in both outputs and touches no other frame; an all-zero frame has
 * logmel = log(floor) in every band.  A frame's values do not depend on the rest of the batch or on the grid.  band_start and
 * band_count are clamped to the frame's bins when read; band_w must hold the sum of the counts.
 * DDSP_EINVAL: a null pointer (logmel excepted), n_fft not a power of two in 64 .. 2048, hop < 1, L < n_fft with B > 0,
 * n_mels outside 1 .. 128, n_mfcc outside 1 .. min(n_mels, 64), B < 0.  B = 0 with valid sizes returns 0 without a launch.
 * Nothing is launched before these checks.  No allocation and no host synchronisation: the call can be captured in a graph.
 */
int ddsp_mfcc(const float *x, const int *band_start, const int *band_count, const float *band_w, const float *dct, float *mfcc,
              float *logmel, long B, long L, int n_fft, int hop, int n_mels, int n_mfcc, float scale, float floor, void *stream);

/*
 * Polyphony: a score whose notes overlap is played by V monophonic voices, each a row of the batch that
 * ddsp_notes_render and the decoder already handle, and the B V rows of audio are summed back to B.  Declared here, ahead of the
 * notes they work on (below), whose record conventions they share.
 *
 * ddsp_voices_allocate: the five record arrays [B, N] and count [B] of ddsp_notes_extract -> the same five arrays as [B V, Nv]
 * (row b V + v is voice v of score b), v_count [B V], index [B V, Nv] (the source slot of each voice note), voice and slot [B, N]
 * (where each source note went) and stats [B, 2] (notes stolen, notes dropped), all int32 but the levels.  Per row, all in integer
 * arithmetic, for the notes i = 0 .. min(count, N) - 1 (a negative count is 0) in slot order; onsets are expected non-decreasing:
 *   1. A note with frames_i < 1, onset_i < 0, a pitch outside 0 .. 127 or |detune_i| > 2^30 sounds nowhere in ddsp_notes_render:
 *      voice_i = slot_i = -1 and nothing else changes.
 *   2. Voice v carries until_v (int64: onset + frames of its last note; -2^31 before its first), last_onset_v, last_pitch_v and
 *      last_level_v (of that note), and count_v.
 *   3. Voice v is free for note i iff until_v + gap <= onset_i.  Among the free voices the smallest key wins; a key is an int64
 *      k 64 + v, so that a tie goes to the lowest voice:  assign = DDSP_VOICES_LOWEST: k = 0;  DDSP_VOICES_OLDEST (round robin):
 *      k = until_v + 2^31;  DDSP_VOICES_NEAREST (a line stays in its voice, a re-struck pitch returns to it):
 *      k = |pitch_i - last_pitch_v|, 128 for a voice without a note yet.
 *   4. With no voice free (every voice then has a note):  steal = DDSP_VOICES_STEAL_OLDEST: the smallest key
 *      last_onset_v 64 + v;  DDSP_VOICES_STEAL_QUIETEST: the smallest key u(last_level_v) 64 + v, u the uint32 that orders fp32
 *      values (bits with the sign bit set where the sign is clear, all bits inverted where it is set), 0xFFFFFFFF for a NaN -- a
 *      note without a level is never the quietest;  DDSP_VOICES_DROP: voice_i = slot_i = -1, stats[b][1] grows, nothing else
 *      changes.  A steal shortens the stolen note in its voice row (where that note was written) to
 *      max(0, min(its frames, onset_i - last_onset_v)) frames, which may be 0, and stats[b][0] grows.
 *   5. The note goes to its voice's row at slot_i = count_v, every field copied, index = i; count_v grows by one, and the
 *      voice's until, last_onset, last_pitch and last_level become the note's.  Past Nv count_v still counts and nothing is
 *      written (ddsp_notes_extract's overflow rule); voice_i is the voice and slot_i = -1.
 *   6. Voice slots from min(count_v, Nv) on are filled: onset -1, frames 0, pitch INT32_MIN, detune 0, level NaN, index -1;
 *      voice and slot from min(count, N) on are -1.
 *   One wavefront per row (the lanes are the voices), a wave-wide minimum per note; a capped grid strides over the rows.
 *   DDSP_EINVAL: B, N or Nv < 0, V outside 1 .. 64, assign or steal outside 0 .. 2, gap outside 0 .. 2^24 - 1; then B = 0 returns
 *   0; then a missing count, v_count or stats, a missing source array, voice or slot with N > 0, a missing voice array or index
 *   with Nv > 0.  DDSP_ERANGE: B N >= 2^31 or B V Nv >= 2^31.
 *
 * ddsp_voices_mix: audio fp32 [B V, L], gains fp32 [B, V, C] (C = 1 or 2) and, where not NULL, active bytes [B V, T] (a frame is
 * active where its byte is not 0: ddsp_notes_render's `voiced`) -> out fp32 [B, C, L]:
 *      out[b, c, n] = sum over v ascending of (gains[b, v, c] g_v(n)) audio[b V + v, n], products and sums rounded to fp32, no
 *      fused multiply-add; the sum starts from voice 0's term (V = 1 with a gain of 1 and no gate copies the bits).
 *   Without `active` g = 1 and is not multiplied in.  With it, d_v(t) = the frames since row b V + v's last active frame at or
 *   before t, e(t) = 1 where d <= hold, max(0, (fade - (d - hold)) / fade) beyond (0 where there is no such frame; fade = 0: a
 *   hard gate), and g(n) = e(t) + (e(min(t + 1, T - 1)) - e(t)) (n mod hop) / hop with t = min(n / hop, T - 1).  The kernel forms
 *   it without cancellation: with F = max(fade, 1) and the integers a = F e(t), a' = F e(min(t + 1, T - 1)), r = n mod hop,
 *   g =fl32(a (hop - r) + a' r) * fl32(1 / fl32(F hop)), and exactly 1 where the numerator equals F hop: at most
 *   four roundings, six with the two products, V - 1 more in the sum.
 *   A workgroup per tile of up to 1024 samples of one score, 16-byte loads and stores where L is a multiple of 4 and audio and out
 *   are 16-byte aligned (4-byte ones otherwise, and in a tile's last partial group); the look-back for d is hold + fade frames at
 *   most.  One launch, no workspace.
 *   DDSP_EINVAL: B < 0, V outside 1 .. 64, C other than 1 or 2, L < 1, hold or fade negative or hold + fade >= 2^16, with `active`
 *   T < 1 or hop < 1; then B = 0 returns 0; then a missing audio, gains or out.  DDSP_ERANGE: L >= 2^31, with `active` hop > 2^15
 *   or T >= 2^31, B times a row's tiles (of 1024 samples; of 32 hop with `active` and hop < 32) >= 2^31, B V L or B V T >= 2^47.
 * Both: nothing is launched before these checks; no allocation, no host synchronisation; no output may alias an input.
 */
#define DDSP_VOICES_LOWEST 0
#define DDSP_VOICES_OLDEST 1
#define DDSP_VOICES_NEAREST 2
#define DDSP_VOICES_STEAL_OLDEST 0
#define DDSP_VOICES_STEAL_QUIETEST 1
#define DDSP_VOICES_DROP 2
int ddsp_voices_allocate(const int *onset, const int *frames, const int *pitch, const int *detune, const float *level,
                         const int *count, int *v_onset, int *v_frames, int *v_pitch, int *v_detune, float *v_level, int *v_count,
                         int *index, int *voice, int *slot, int *stats, long B, long N, int V, long Nv, int assign, int steal,
                         long gap, void *stream);
int ddsp_voices_mix(const float *audio, const float *gains, const uint8_t *active, float *out, long B, int V, int C, long L, long T,
                    long hop, long hold, long fade, void *stream);

/*
 * Wavetable synthesis (csrc/ddsp_wavetable.hip): N single-cycle tables of L points, one fp64 phase
 * accumulator per batch row reading them at f0 with linear interpolation, mixed by per-frame weights.
 *   f0 [B,T,1] Hz, c [B,T,N] mix weights (normalised by their sum per frame inside), a [B,T,1] loudness, tables [N,L]
 *   -> y [B, T*hop].  up() is the oscillator bank's upsampling; the phase P[b,n] = P0[b] + sum_{m<=n} up(fl32(f0/sample_rate))[b,m]
 *   in cycles; y = up(a) * sum_k up(c_k / sum c) * (W[k,j] + fr * (W[k,j+1] - W[k,j])) at j = floor(frac(P) L), j + 1 wrapping.
 *
 * ddsp_wavetable_supported  1 when the kernels take N tables of L points (1 <= N <= 1024, 2 <= L <= 65536, N L <= 2^18).
 * ddsp_wavetable_form       what the planner (csrc/ddsp_wavetable_plan.h) picks for the shape under the current hooks: the
 *                           forward's form in bits 0-1 and the backward's in bits 2-3, 1 = the tables staged in LDS, 2 = read
 *                           from memory; a negative DDSP_E* code for a shape the entry points would refuse.
 * ddsp_wavetable_scratch_bytes  bytes of `scratch` the forward wants: 0 today (neither form keeps anything, the backward
 *                           rebuilds the phases from f0); `scratch` may then be NULL.
 * ddsp_wavetable_forward    one launch.  phase_io [B] fp64, nullable: the start phases P0 (cycles), replaced in place by
 *                           frac(P[b, T*hop-1]) -- the state of a live stream, with no host round trip, so the call can be
 *                           captured in a graph.  NULL: P0 = 0 and nothing is carried.
 * ddsp_wavetable_backward   two launches.  grad_y [B, T*hop] -> grad_c [B,T,N] (with respect to the raw c: the normalisation's
 *                           backward is inside), grad_a [B,T,1], grad_tables [N,L]; f0 gets no gradient.  phase_in [B]: the P0 the
 *                           forward started from (nullable, read only).  scratch: >= ddsp_wavetable_backward_scratch_bytes bytes,
 *                           256-byte aligned: three partials per frame and table (3x grad_c) and one private [N,L] table per
 *                           workgroup of the plan (at most 256), sized under the test hooks in force when it is asked.  grad_c and grad_a are sums in a fixed order (the same bits every run); grad_tables
 *                           is accumulated with atomics inside a workgroup, then over the workgroups in a fixed order.
 * Both need hop <= 1024, T*hop <= 2^24 and return DDSP_ERANGE otherwise; with B == 0 they return 0 and write nothing.
 *
 * ddsp_wavetable_set_form   test hook: bits 0-1 force a form (0: the planner's, 1: LDS -- DDSP_ERANGE from the launch where it
 *                           does not fit --, 2: memory); bits 8-15 the frames of a chunk and bits 16-23 the frames of an iteration
 *                           (0: the planner's), so that the chunk prefix and the carried scan run at small shapes.
 * ddsp_wavetable_set_grid   test hook: at most this many workgroups (1..256; 0: the default), so that the stride over the units
 *                           runs at small shapes.
 */
int ddsp_wavetable_supported(int N, int L);
int ddsp_wavetable_form(int B, int T, int N, int L, int hop);
size_t ddsp_wavetable_scratch_bytes(int B, int T, int N, int L, int hop);
int ddsp_wavetable_forward(const float *f0, const float *c, const float *a, const float *tables, float *y, void *scratch,
                           double *phase_io, int B, int T, int N, int L, int hop, int sample_rate, void *stream);
size_t ddsp_wavetable_backward_scratch_bytes(int B, int T, int N, int L, int hop);
int ddsp_wavetable_backward(const float *grad_y, const float *f0, const float *c, const float *a, const float *tables,
                            const double *phase_in, void *scratch, float *grad_c, float *grad_a, float *grad_tables, int B, int T,
                            int N, int L, int hop, int sample_rate, void *stream);
int ddsp_wavetable_set_form(int mode);
int ddsp_wavetable_set_grid(int workgroups);

/*
 * Band-limited wavetables (csrc/ddsp_wavetable_mip.hip, csrc/ddsp_wavetable.hip): mip levels of the tables,
 * two of which every sample reads, chosen from its increment so that no harmonic above sample_rate / 2 is played.  L must be a
 * power of two with 16 <= L <= 4096 (DDSP_ERANGE otherwise); Q = log2 L and there are Q + 1 levels.
 *   levels M [Q+1, N, L] fp32: M[0] = tables bit for bit; M[q] for q >= 1 keeps the mean and the harmonics h <= L >> (q + 1):
 *   M[q,k,j] = sum_i tables[k,i] * kernels[q, (j - i) mod L], i ascending in fp32, with kernels [Q+1, L] fp32 the Dirichlet kernels
 *   D[q,j] = (1 + 2 sum_{h=1..L>>(q+1)} cos(2 pi h j / L)) / L computed by the caller in fp64 (row 0 is never read).
 *   A sample with increment u (as above) has r = L u.  not (r > 0.5): level 0 alone.  Otherwise r = m 2^e with m in [0.5, 1):
 *   levels e and e + 1 with weights 1 - t and t, t = 2 m - 1; e >= Q: level Q alone.  Everything else is ddsp_wavetable_forward's.
 *
 * ddsp_wavetable_mip_levels   Q + 1, or DDSP_ERANGE for a table size that cannot be band-limited.
 * ddsp_wavetable_mip_build    one launch, tables [N,L] -> levels; the same bits every run.
 * ddsp_wavetable_mip_adjoint  one launch, grad_levels [Q+1,N,L] -> grad_tables [N,L] = grad_levels[0] + sum_q the same circular
 *                             sum of grad_levels[q] with kernels[q] (they are symmetric); the same bits every run.
 * ddsp_wavetable_form_bl      the band-limited plan under the current hooks: bits 0-1 the forward's form and bits 2-3 the
 *                             backward's (1: a unit (row, chunk) stages the levels it hears in LDS when they fit, 2: every unit
 *                             reads the levels from memory), bits 8-15 and 16-23 the most levels a unit of the forward and of the
 *                             backward can stage; a negative DDSP_E* code for a shape the entry points would refuse.
 * ddsp_wavetable_forward_bl   one launch; ddsp_wavetable_forward with `levels` in place of the tables (no scratch).
 * ddsp_wavetable_backward_bl  two launches; as ddsp_wavetable_backward, with grad_levels [Q+1,N,L] out (give it to
 *                             ddsp_wavetable_mip_adjoint for the tables' gradient).  t and the table position carry no gradient.
 *                             scratch >= ddsp_wavetable_backward_bl_scratch_bytes, 256-byte aligned: the three partials per frame
 *                             and one private [Q+1,N,L] table per workgroup; the workgroups are limited so that those stay within
 *                             512 MiB.  grad_c and grad_a have the same bits every run; grad_levels is summed with atomics inside
 *                             a workgroup.
 * ddsp_wavetable_set_mip_lds  test hook: the LDS bytes a workgroup of the band-limited kernels may use (0: a CU's 160 KiB), so
 *                             that "the levels do not fit" happens at small shapes.  ddsp_wavetable_set_form's form bits apply
 *                             too: 1 returns DDSP_ERANGE unless all Q + 1 levels fit (then every unit stages), 2 stages nothing;
 *                             its chunk and iteration bits and ddsp_wavetable_set_grid act as on the unlimited kernels.
 */
int ddsp_wavetable_mip_levels(int L);
int ddsp_wavetable_mip_build(const float *tables, const float *kernels, float *levels, int N, int L, void *stream);
int ddsp_wavetable_mip_adjoint(const float *grad_levels, const float *kernels, float *grad_tables, int N, int L, void *stream);
int ddsp_wavetable_form_bl(int B, int T, int N, int L, int hop);
int ddsp_wavetable_forward_bl(const float *f0, const float *c, const float *a, const float *levels, float *y, double *phase_io,
                              int B, int T, int N, int L, int hop, int sample_rate, void *stream);
size_t ddsp_wavetable_backward_bl_scratch_bytes(int B, int T, int N, int L, int hop);
int ddsp_wavetable_backward_bl(const float *grad_y, const float *f0, const float *c, const float *a, const float *levels,
                               const double *phase_in, void *scratch, float *grad_c, float *grad_a, float *grad_levels, int B,
                               int T, int N, int L, int hop, int sample_rate, void *stream);
int ddsp_wavetable_set_mip_lds(long bytes);

/*
 * Inharmonic sinusoid bank (csrc/ddsp_sinusoids.hip): K sinusoids per batch row, each with its own
 * frame-rate frequency track.
 *   f [B,T,K] Hz, c [B,T,K], a [B,T,1] -> y [B, T*hop].  An entry of f is valid when it is finite and >= 0; an invalid one has
 *   g = 0 and weight 0, a valid one g = (double)f / sample_rate and weight c, or 0 where f > sample_rate / 2 (integer division).
 *   With `normalize` the weights of a frame are divided by their sum (fp64, rounded once; a zero sum gives zero weights).
 *   y = up(a) * sum_k up(wn_k) * sin(2 pi P_k), up() the oscillator bank's upsampling, and P_k[n] = P0_k + the inclusive sum of the
 *   same linear interpolation of g_k in real arithmetic, evaluated in fp64 through its closed form per segment
 *   (n = hop/2 + s hop + j: P = P0 + Phi[s] + (j + 1) (g[s] + (g[s+1] - g[s]) (j + e) / (2 hop)), e = 1 for an even hop, else 0).
 *
 * ddsp_sinusoids_supported   1 when the kernels take K partials at this hop (1 <= K <= 1024, 1 <= hop <= 1024).
 * ddsp_sinusoids_scratch_bytes  bytes of `scratch` the forward wants: 0 (one launch that keeps nothing); `scratch` may be NULL.
 * ddsp_sinusoids_forward     one launch, the same bits every run and under every plan.  phase_io [B,K] fp64, nullable: the start
 *                            phases P0 (turns), replaced in place by frac(P[b, T*hop-1, k]) -- the state of a live stream, with
 *                            no host round trip, so the call can be captured in a graph.  NULL: P0 = 0, nothing is carried.
 * ddsp_sinusoids_backward    two launches, three with grad_f.  grad_y [B, T*hop] -> grad_c [B,T,K] (with respect to the raw c:
 *                            the normalisation's backward and the mask are inside), grad_a [B,T,1] and, unless grad_f is NULL,
 *                            grad_f [B,T,K] (0 at invalid entries), the adjoint of the closed form: per segment the fp32 sums
 *                            of q = grad_y up(a) up(wn) 2 pi cos(2 pi P), plain and weighted by the coefficients of g[s] and
 *                            g[s+1], combined by an fp64 suffix sum over the segments.  `phase` [B,K]: the P0 the forward started
 *                            from (nullable, read only).  scratch: >= ddsp_sinusoids_backward_scratch_bytes bytes, 256-byte
 *                            aligned: four partials per frame and partial (4x grad_c) and with grad_f three more.  No atomics:
 *                            every gradient has the same bits every run.
 * All need T*hop <= 2^24 and return DDSP_ERANGE otherwise; with B == 0 they return 0 and write nothing.
 *
 * ddsp_sinusoids_set_form    test hook: bits 8-15 the segments of a chunk, bits 16-23 the segments of an iteration, bits 24-30 the
 *                            backward's sample records per tile in units of 64 (0: the planner's, csrc/ddsp_sinusoids_plan.h), so
 *                            that the chunk prefix, several iterations and several tiles run at small shapes; bits 0-7 must be 0.
 * ddsp_sinusoids_set_grid    test hook: at most this many workgroups (1..2048; 0: the default), so that the stride over the units
 *                            runs at small shapes.
 */
int ddsp_sinusoids_supported(int K, int hop);
size_t ddsp_sinusoids_scratch_bytes(int B, int T, int K, int hop);
int ddsp_sinusoids_forward(const float *f, const float *c, const float *a, float *y, void *scratch, double *phase_io, int B, int T,
                           int K, int hop, int sample_rate, int normalize, void *stream);
size_t ddsp_sinusoids_backward_scratch_bytes(int B, int T, int K, int hop, int want_grad_f);
int ddsp_sinusoids_backward(const float *grad_y, const float *f, const float *c, const float *a, void *scratch, float *grad_f,
                            float *grad_c, float *grad_a, const double *phase, int B, int T, int K, int hop, int sample_rate,
                            int normalize, void *stream);
int ddsp_sinusoids_set_form(int mode);
int ddsp_sinusoids_set_grid(int workgroups);

/*
 * Inharmonic analysis, the inverse of the sinusoid bank (csrc/ddsp_partials.hip).  All fp32 but the
 * workspace, dense row-major; rows are independent.
 *   audio [B, N], N = T hop; f [B, T, K] in Hz; voiced [B, T] bytes (nullable: every frame is voiced); sample rate sr; an even
 *   window W >= 2.
 *   1. g = (double)f / sr where f is finite and > 0, else 0.
 *   2. P_k[n] is the bank's phase with P0 = 0: the inclusive sum of the linearly interpolated g_k in real arithmetic through its
 *      closed form per segment (above: n = hop/2 + s hop + j: P = Phi[s] + (j + 1) (g[s] + (g[s+1] - g[s]) (j + e) / (2 hop)); the
 *      samples n < hop/2 in front: P = (n + 1) g[0]), in fp64, Phi kept modulo 1.
 *   3. Frame t covers the samples s_t + j, j < W, s_t = t hop - floor((W - hop) / 2); w is the periodic Hann window; samples
 *      outside [0, N) are left out and norm_t is the sum of w over the samples inside (ddsp_harm_analysis' items 3 and 4).
 *   4. C[t,k] = (2 / norm_t) sum_j w[j] audio[s_t + j] exp(-2 pi i P_k[s_t + j]).
 *   5. C[t,k] = 0 where f[t,k] is not finite or <= 0, where f[t,k] > sr / 2 (integer division; the bank's mask on the frame's own
 *      entry), and on an unvoiced frame.
 *   6. amp = |C|, a = sum_k amp, c = amp / a, and c = 1 / K where a = 0.
 *   7. On the frames whose window lies inside the clip and where C != 0, with D the sum of item 4 under w'[j] = (pi / W)
 *      sin(2 pi j / W), both unscaled:  f_re[t,k] = mean_w(up(f_k)) - sr / (2 pi) (Im D Re C - Re D Im C) / |C|^2, mean_w the
 *      window-weighted mean of the upsampled (cleaned) track in fp64.  Elsewhere f_re has the bits of f.
 *   8. harm[n] = sum_k Re(up(C[:,k])[n] exp(+2 pi i P_k[n])), resid = audio - harm.
 *
 * ddsp_partials_supported        1 when the kernels take this shape: 1 <= K <= 256, 1 <= hop <= 1024, W even in 2 .. 4096.  No device.
 * ddsp_partials_workspace_bytes  bytes of `workspace` (16-byte aligned) for both calls; 0: sizes that are not positive, out of range
 *                                or overflowing.  It holds the two windows and Phi, g and d / (2 hop) [B, T, K] in fp64.
 * ddsp_partials_analysis   -> C [B, T, K] interleaved (re, im), a [B, T], c [B, T, K] and, unless f_re is NULL, f_re [B, T, K]; it
 *                          fills `workspace`.  Three launches (prefix, windows, analysis).  With f_re == NULL the second window
 *                          and its two FMAs per (sample, partial) do not exist.
 * ddsp_partials_resynth    C [B, T, K] interleaved (8-byte aligned) -> harm [B, N] and, where resid is not NULL, resid = audio - harm
 *                          (audio may be NULL otherwise).  With DDSP_PARTIALS_PHASE_READY in flags the workspace still holds the
 *                          prefix of a ddsp_partials_analysis or ddsp_partials_resynth call with the same f, B, T, K, hop and
 *                          sample_rate, and the prefix launch is left out.  Two launches, one with the flag.
 * Beyond the range above, or with T hop > 2^24 or B T K or B T hop > 2^40: DDSP_ERANGE.  A null pointer, an odd W, an unknown flag
 * or a size that is not positive: DDSP_EINVAL before anything touches the device; B == 0 returns 0.  No atomics on global memory,
 * nothing allocated or synchronised: the calls can be captured in a graph.  The same bits every run, and for a row whatever its
 * batch.
 */
#define DDSP_PARTIALS_PHASE_READY 1u
int ddsp_partials_supported(int K, int hop, int W);
size_t ddsp_partials_workspace_bytes(long B, long T, int K, int hop, int W);
int ddsp_partials_analysis(const float *audio, const float *f, const uint8_t *voiced, float *C, float *a, float *c, float *f_re,
                           void *workspace, long B, long T, int K, int hop, int W, int sample_rate, void *stream);
int ddsp_partials_resynth(const float *C, const float *f, const float *audio, float *harm, float *resid, void *workspace, long B,
                          long T, int K, int hop, int sample_rate, unsigned flags, void *stream);

/*
 * Training-set audio (dataset/audio_dataset.py): the stages between the file read and the encoder.  All fp32 out.
 *
 * ddsp_pcm_to_mono   interleaved PCM pcm [L, C] (as the WAV file stores it) -> y [L]: each sample scaled as
 *                    torchaudio.load(normalize=True) scales it (format DDSP_PCM_S16: / 32768, DDSP_PCM_S32: / 2^31 -- a 24-bit
 *                    file reaches the caller left-justified in int32 --, DDSP_PCM_F32: as is), then for C > 1 the mean over
 *                    channels summed in channel order from 0 and divided by C (torch's CPU y.mean(dim=0), :30-37).  An unknown
 *                    format is DDSP_EINVAL; C <= 65535.
 * ddsp_make_examples the examples e0 .. e0 + E - 1 of several files' conf-rate mono audio, concatenated in y [y_len].  files
 *                    [n_files, 4] int64 (device): start of the file in y, its length, its front hop-pad pad // 2
 *                    (pad = length % hop, :46-47) and its first example's index; first is non-decreasing.  Example e of file f
 *                    is the padded file's samples (e - first) * step .. + duration (unfold(0, duration, step), :50-59), zero
 *                    outside [0, length).  Writes, either may be NULL but not both:
 *                      enc_in [E, duration + p]  the example between (p / 2, p - p / 2) zeros, p = n_fft - hop (:86, 90)
 *                      audio  [E, duration]      the bare example (the `audio` key, :95)
 *                    duration <= INT_MAX.  No read leaves y, whatever the table holds.
 */
#define DDSP_PCM_S16 1
#define DDSP_PCM_S32 2
#define DDSP_PCM_F32 3
int ddsp_pcm_to_mono(const void *pcm, float *y, long L, int C, int format, void *stream);
int ddsp_make_examples(const float *y, long y_len, const long *files, int n_files, long e0, long E, long duration, long step, int p,
                       float *enc_in, float *audio, void *stream);


/*
 * Griffin-Lim phase reconstruction (torchaudio 0.8.1 functional.griffinlim; style_transfer.py:149-156, helper.py:105-112).
 *   mag    [B, F, T] fp32, F = n_fft / 2 + 1: the magnitude ALREADY raised to 1 / power
 *   angles [B, F, T] complex64 (interleaved re, im) initial phases, or NULL: every angle 1 (rand_init=False)
 *   window [n_fft]   the analysis / synthesis window zero-padded and centred to n_fft (torch.stft's padding of win_length)
 *   env    [L]       the istft window envelope (sum of window^2 over the overlapping frames) at retained sample j, i.e. at
 *                    n_fft/2 + j of the overlap-added signal; read for j < min(L, n_fft/2 + hop (T - 1)) only.  The caller checks
 *                    it (NOLA) once.
 *   y      [B, L]    out: the signal; also the iteration's signal in between (no other output buffer is needed)
 * Each of the n_iter iterations is y = istft(mag * angles, center=True, length=L); R = stft(y, center=True, reflect, onesided);
 * angles = R - c R_prev (skipped for c == 0; R_prev = 0 in the first iteration); angles /= sqrt(re^2 + im^2) + 1e-16.  Then one
 * final istft.  c = fl32(momentum / (1 + momentum)) in [0, 1).  Constraints (DDSP_ERANGE otherwise): n_fft a power of two in
 * [64, 2048] (ddsp_griffinlim_supported), 1 + L / hop == T, L > n_fft / 2 (reflect padding), B <= 65535.  The workspace
 * (ddsp_griffinlim_workspace_bytes; with_angles: whether `angles` will be non-NULL) holds the frame-major magnitude, the
 * initial angles, two rebuilt spectra and the synthesised frames; nothing is allocated inside.  All launches are enqueued
 * on `stream` (three per iteration, no atomics: deterministic) and the call returns without synchronising.
 */
int ddsp_griffinlim_supported(int n_fft);
size_t ddsp_griffinlim_workspace_bytes(long B, long T, int n_fft, int with_angles);
int ddsp_griffinlim(const float *mag, const float *angles, const float *window, const float *env, float *y, void *workspace,
                    size_t workspace_bytes, long B, long T, int n_fft, int hop, long L, int n_iter, float c, void *stream);

/*
 * Test hook (DDSP_EPERM unless DDSP_TEST_HOOKS=1 was set when the library was loaded): the pieces of the shared one-wavefront
 * FFT (csrc/ddsp_wave_fft.h) on the caller's data, one wavefront per unit, for tests/test_gpu_wave_fft.py.  The kernels load the
 * input in the layout the header documents, call its function and store the result in natural order; they do no arithmetic of
 * their own.  Complex data is interleaved (re, im); `in` and `out` are device memory, 8-byte aligned, and must not overlap.
 *
 *   form                            in (floats per unit)                     out (floats per unit)
 *   DDSP_WFFT_PAIR_FWD + i, i < 5   [BT, N] complex, N = 64 << i,            [BT, N] complex: PairFft<N>::run<false>, natural(i)
 *   DDSP_WFFT_PAIR_INV + i          BT = 8, 4, 2, 1, 1 transforms per unit   the same with run<true> (unnormalised: N ifft)
 *   DDSP_WFFT_WAVE8_FWD, _INV       [512] complex                            [512] complex: fft_wave<8, INV, false>, store_natural
 *   DDSP_WFFT_WAVE8_HALFZERO        [256] complex (the lower half)           [512] complex: fft_wave<8, false, true>
 *   DDSP_WFFT_WAVE16_FWD, _INV      [1024] complex                           [1024] complex
 *   DDSP_WFFT_WAVE16_HALFZERO       [512] complex                            [1024] complex
 *   DDSP_WFFT_REAL2048_FWD          [2048] real                              [1025] complex: rfft (fft_wave<16>, split2048)
 *   DDSP_WFFT_REAL2048_INV          [1025] complex, bins 0 and 1024 real     [2048] real: 2048 irfft (pack2048, fft_wave<16, true>)
 *   DDSP_WFFT_TWIDDLES              nothing (in is not read)                 [64 lanes, DDSP_WFFT_TWIDDLE_COUNT] complex, per lane:
 *                                     Twiddles<8> t1[8], t2[0][8]; Twiddles<16> t1[16], t2[0][8], t2[1][8]; PairFft<128>::t1s[2];
 *                                     PairFft<256>::t1s[4]; PairFft<64>, <128>, <256>::tw.t2[0][8]; lane_w2048; twiddle2048 it = 0..8
 *   DDSP_WFFT_SCALE                 c_in, c_out in front, then one m a unit  (frame_scale_of(m, c_in, c_out).in, .out)
 *   DDSP_WFFT_WAVEMAX               [64]                                     [64]: wave_max as each lane sees it
 *
 * ddsp_wfft_probe_sizes gives the floats of `in` and `out` for `units` units.  An unknown form, a null pointer, negative units or
 * more than 2^20 of them: DDSP_EINVAL; units == 0 returns 0; nothing is launched before these checks.  One launch on `stream`.
 */
#define DDSP_WFFT_PAIR_FWD 0
#define DDSP_WFFT_PAIR_INV 5
#define DDSP_WFFT_WAVE8_FWD 10
#define DDSP_WFFT_WAVE8_INV 11
#define DDSP_WFFT_WAVE8_HALFZERO 12
#define DDSP_WFFT_WAVE16_FWD 13
#define DDSP_WFFT_WAVE16_INV 14
#define DDSP_WFFT_WAVE16_HALFZERO 15
#define DDSP_WFFT_REAL2048_FWD 16
#define DDSP_WFFT_REAL2048_INV 17
#define DDSP_WFFT_TWIDDLES 18
#define DDSP_WFFT_SCALE 19
#define DDSP_WFFT_WAVEMAX 20
#define DDSP_WFFT_TWIDDLE_COUNT 88
int ddsp_wfft_probe_sizes(int form, long units, long *in_floats, long *out_floats);
int ddsp_wfft_probe(int form, const float *in, float *out, long units, void *stream);

/*
 * Notes with their expression: the pitch and loudness curve a performer gave each note, taken from the
 * performance and carried through an edit of the notes.  Conventions, records and render as ddsp_notes_extract and
 * ddsp_notes_render below (positions are int64 counts of 2^-16 cent, S = 100 * 65536, rdiv as there); declared here, ahead of
 * ddsp_griffinlim_stage, because the header's last four declarations are pinned by tests.
 *
 * ddsp_notes_expression: cents (normalized_cents) [B, T], the record arrays onset, frames, pitch, detune [B, N], count [B],
 * offset [groups] -> bend int32 [B, T] and, where not NULL, owner int32 [B, T].  For frame t of a row:
 *   1. i* = the largest i < min(count, N) with onset_i <= t (ddsp_notes_render's step 3).
 *   2. The frame belongs to note i* iff i* exists, is valid (the render's step 2), t < onset_i* + frames_i* and |n_t| <= 4.
 *   3. Then bend_t = u_t - 65536 o - pitch_i* S - detune_i*, u_t the auto-tune's position of n_t (its step 1), o the clamped
 *      offset; a value outside int32 (records that do not match the track) is saturated.  owner_t = i*.
 *   4. Otherwise bend_t = 0 and owner_t = -1.
 *   Nothing is assumed about where the records came from: onsets out of order give unspecified values, never an access out of
 *   bounds.  One thread per frame; one launch, no allocation, no host synchronisation.
 *   DDSP_EINVAL: B < 0, T <= 0, N < 0; then B = 0 returns 0; then a missing pointer (owner may be NULL, the record arrays only
 *   with N = 0), group counts other than 1 or B.  DDSP_ERANGE: T >= 2^24, B T >= 2^31 or B N >= 2^31.
 *
 * ddsp_notes_render_expr: ddsp_notes_render -- every term of it, the glide, the synthetic vibrato and the ga and gr ramps
 * included -- plus, on the on frames, the curves of a source performance: `source` [B, N] (the source note of each note; NULL:
 * note i reads source note i), the source's records src_onset, src_frames, src_level [B, Nsrc] and src_count [B], its `bend`
 * int32 [B, Tsrc] (ddsp_notes_expression's) and, where not NULL, its loudness track src_loudness fp32 [B, Tsrc].
 *   1. For an on frame of note i (k = t - onset_i, L' its sounding length, the render's step 6), j = source[i], or i.  The
 *      source is valid iff 0 <= j < min(src_count, Nsrc), src_frames_j >= 1, src_onset_j >= 0 and
 *      src_onset_j + src_frames_j <= Tsrc.  A note without a valid source is rendered as by ddsp_notes_render; so is a frame
 *      with k >= L' (there is none while the onsets are in order); so are the off frames.
 *   2. Time map: with Ls = src_frames_j, a = min(keep_attack, Ls, L') and r = min(keep_release, Ls - a, L' - a), frame k reads
 *      the source note at (q, f), f in 2^-16 frame:
 *        k < a (head)          (k, 0)
 *        k >= L' - r (tail)    (Ls - (L' - k), 0)
 *        else (middle)         m = k - a + 1, Ns = Ls - a - r + 1, D = L' - a - r + 1:
 *                              q = a - 1 + (m Ns) div D, f = (((m Ns) mod D) 65536) div D
 *      then q < 0 gives (0, 0) and q >= Ls - 1 gives (Ls - 1, 0).  The middle interpolates between the anchors k = a - 1 <->
 *      a - 1 and k = L' - r <-> Ls - r, and is the identity when L' = Ls.  All products stay below 2^48.
 *   3. Pitch: with b_x = bend[src_onset_j + x], B = b_q + floor(((b_{q+1} - b_q) f + 32768) / 65536) in int64 (b_{q+1} is read
 *      only where f > 0), and p += llrint(bend_amount (double)B): one fp64 product, exact at amount 1.
 *   4. Loudness, where src_loudness is given, src_level_j is not a NaN and dyn_amount != 0: with l_x = src_loudness[src_onset_j
 *      + x], l(q, f) = l_q + (l_{q+1} - l_q) (f / 65536) in fp64 (l_q alone where f = 0), and
 *      loudness = fl32(base + dyn_amount (l(q, f) - (double)src_level_j)), base the render's floor + (lv - floor) ga gr.
 *   A thread reads at most two neighbouring source frames, both inside the source note.  One launch, no allocation, no host
 *   synchronisation.
 *   DDSP_EINVAL: ddsp_notes_render's options, then Tsrc <= 0, Nsrc < 0, an amount that is not finite or beyond 16 in magnitude,
 *   keep_attack or keep_release outside 0 .. 2^24 - 1; then B = 0 returns 0; then ddsp_notes_render's pointers, a NULL src_count
 *   or bend, a NULL src_onset, src_frames or src_level with Nsrc > 0.  DDSP_ERANGE: ddsp_notes_render's sizes, Tsrc >= 2^24,
 *   B Tsrc >= 2^31 or B Nsrc >= 2^31.
 */
int ddsp_notes_expression(const float *cents, const int *onset, const int *frames, const int *pitch, const int *detune,
                          const int *count, const int *offset, int *bend, int *owner, long B, long T, long N, long groups,
                          void *stream);
int ddsp_notes_render_expr(const int *onset, const int *frames, const int *pitch, const int *detune, const float *level,
                           const int *count, const int *offset, float *f0, float *cents, float *loudness, float *harmonicity,
                           uint8_t *voiced, long *position, int *owner, long B, long T, long N, long groups, int flags,
                           long transpose, long glide, long attack, long release, long vibrato_delay, long vibrato_ramp,
                           double vibrato_depth, double vibrato_omega, float floor_level, float default_level, const int *source,
                           const int *src_onset, const int *src_frames, const float *src_level, const int *src_count,
                           const int *bend, const float *src_loudness, long Tsrc, long Nsrc, double bend_amount, double dyn_amount,
                           long keep_attack, long keep_release, void *stream);

/*
 * Test hook (DDSP_EPERM unless DDSP_TEST_HOOKS=1 was set when the library was loaded): ONE of the three launches of a Griffin-Lim
 * iteration (csrc/ddsp_griffinlim.hip) on the caller's buffers, for tests/test_gpu_griffinlim_stages.py.  It fills the kernels'
 * parameter block and calls the launcher ddsp_griffinlim calls; it does no arithmetic of its own.  Everything is device memory in
 * the kernels' own frame-major layout (ddsp_griffinlim transposes into it), F = n_fft / 2 + 1, complex data interleaved (re, im),
 * 8-byte aligned; `out` must not overlap an input.
 *
 *   stage                    reads                                                                  out
 *   DDSP_GL_STAGE_SYNTH      S [B T, F]; ang0 [B T, F] complex or NULL (every angle 1), used when   frames [B T, n_fft]:
 *                            R is NULL; R [B T, F] complex or NULL; Rprev [B T, F] complex or NULL  irfft(S angles) window
 *                            (no momentum term), read with R only; window [n_fft]; c
 *   DDSP_GL_STAGE_OVERLAP    in = frames [B T, n_fft]; env [L] (read below min(L, n_fft/2 +         y [B, L]
 *                            hop (T - 1)) only)
 *   DDSP_GL_STAGE_ANALYSIS   in = y [B, L]; window [n_fft]                                          R [B T, F] complex
 *
 * Arguments a stage does not read may be NULL.  DDSP_EINVAL: an unknown stage, a null `out` or a null pointer the stage reads,
 * B, T, hop or L <= 0, c outside [0, 1).  DDSP_ERANGE: ddsp_griffinlim's constraints (n_fft, 1 + L / hop == T, L > n_fft / 2,
 * B <= 65535, the size limits).  Nothing is launched before these checks.  One launch on `stream`, no synchronisation.
 */
#define DDSP_GL_STAGE_SYNTH 0
#define DDSP_GL_STAGE_OVERLAP 1
#define DDSP_GL_STAGE_ANALYSIS 2
int ddsp_griffinlim_stage(int stage, const float *S, const float *ang0, const float *R, const float *Rprev, const float *in,
                          const float *window, const float *env, float *out, long B, long T, int n_fft, int hop, long L, float c,
                          void *stream);

/*
 * Notes: the note events of a pitch track, and note events rendered back to frame-rate controls, in the
 * integer conventions of the auto-tune above: a position is an int64 count of 2^-16 cent on the MIDI scale, S = 100 * 65536, K the
 * literal of step 1 there, rdiv(a, b) = floor((2 a + b) / (2 b)).
 *
 * ddsp_notes_extract, per row (inputs as ddsp_tuning_apply's; `loudness` gates a frame only with gate_loudness = 1):
 *   1. u_t, "on", v_t = u_t - 65536 o and note_t are steps 1, 2 and 5 of the auto-tune.
 *   2. A note is a maximal run of on frames with one note_t; its first frame is `onset`, its length L.
 *   3. Notes with L < min_note_frames are dropped: not reported, their frames belong to no note.
 *   4. A kept note's record: onset, frames = L, pitch = note_t, detune = -rdiv(pitch S L - sum v, L) (units above the pitch on the
 *      performance's own grid: exactly minus the correction the auto-tune gives the note with DDSP_TUNING_VIBRATO alone, amount 1,
 *      glide 0 -- the mean of v - pitch S rounded to the nearest unit, a tie going down, where rdiv(sum v - pitch S L, L) would
 *      send it up and differ from that correction by one unit), all int32; level fp32 = the largest loudness over the note's frames that is not a NaN (+0 above -0), the canonical NaN
 *      (0x7FC00000) where there is none or loudness is NULL.  A maximum: the same bits in any order.
 *   5. Records are written in order of onset into [B, N] arrays.  count[b] = the kept notes of the row, those beyond N included:
 *      overflow shows as count > N, and nothing is written past N.
 *   6. Slots from min(count, N) on are filled: onset -1, frames 0, pitch INT32_MIN, detune 0, level NaN.
 *   One wavefront per row, no per-frame storage, no atomics; one launch, no allocation, no host synchronisation.
 *
 * ddsp_notes_render: the five record arrays [B, N], count [B], offset [groups] -> f0, cents (normalized_cents), loudness,
 * harmonicity fp32 [B, T], voiced bytes [B, T], and where not NULL position int64 [B, T] and owner int32 [B, T].
 *   1. n = min(count, N) (a negative count is 0).  Onsets are expected non-decreasing over i < n; anything else gives
 *      unspecified values, never an access out of bounds.
 *   2. Note i is valid iff frames_i >= 1 and 0 <= pitch_i <= 127 and |detune_i| <= 2^30.
 *   3. i*(t) = the largest i < n with onset_i <= t: a later note cuts an earlier one off (monophonic).
 *   4. Frame t is on, and owner = i*, iff i* exists, is valid and t < onset_i* + frames_i*; otherwise owner = -1.
 *   5. b_i = pitch_i S + (DDSP_NOTES_KEEP_DETUNE ? detune_i : 0) + (DDSP_NOTES_CONCERT ? 0 : 65536 o) + transpose (units;
 *      o clamped to +-50 as in the auto-tune).
 *   6. L'_i = min(frames_i, onset_{i+1} - onset_i); for the last note L'_i = frames_i.
 *   7. On frames, k = t - onset_i: p = b_i + glide_term + vib_term.
 *      glide_term = rdiv((b_{i-1} - b_i) (G - k), G + 1) when G = glide > 0, k < G, note i - 1 exists and is valid and
 *      onset_i <= onset_{i-1} + frames_{i-1} (legato); else 0.
 *      vib_term = llrint(vibrato_depth min(1, (k - delay + 1) / ramp) sin(vibrato_omega (k - delay))) in fp64 (depth in units,
 *      omega in radians per frame), when vibrato_depth > 0 and k >= delay; else 0.
 *   8. Off frames hold a pitch: p = b_i* where i* exists and is valid, b_0 before the first onset where note 0 is valid, else
 *      6900 * 65536.
 *   9. cents = fl32((p / 65536 - K) / 7180), f0 = fl32(440 exp2((p / 65536 - 6900) / 1200)), both formed in fp64.
 *  10. On frames loudness = fl32(floor + (lv - floor) ga gr) in fp64: lv = level_i, or default_level where that is a NaN;
 *      ga = min(1, (k + 1) / attack) where attack > 0, else 1; gr = min(1, (L'_i - k) / release) where release > 0, else 1.
 *      Off frames: loudness = floor.  harmonicity is 1 on and 0 off, voiced the on flag.
 *   One thread per output frame, no atomics; one launch, no allocation, no host synchronisation.
 *
 * Both: DDSP_EINVAL: a missing pointer (the record arrays may be NULL only with N = 0), T <= 0, N < 0, group counts other than 1
 * or B; extract: a mask outside 1 .. 0xFFF, a forced root outside -1 .. 11, hysteresis outside 0 .. 1200 * 65536, a negative
 * min_note_frames, a NaN silence or confidence, gate_loudness outside 0 .. 1 or set without loudness; render: unknown flags,
 * |transpose| > 128 S, glide, attack, release, delay or ramp outside 0 .. 2^24 - 1, ramp < 1, a depth outside 0 .. 128 S, a NaN
 * or |omega| > 10^6, a floor or default level that is not finite.  DDSP_ERANGE: T >= 2^24, B T >= 2^31 or B N >= 2^31.
 * Nothing is launched before these checks; B = 0 returns 0 without a launch.  No output may alias an input.
 */
#define DDSP_NOTES_KEEP_DETUNE 1
#define DDSP_NOTES_CONCERT 2
int ddsp_notes_extract(const float *cents, const float *harmonicity, const float *loudness, const uint8_t *voiced, const int *offset,
                       const int *root, int *onset, int *frames, int *pitch, int *detune, float *level, int *count, long B, long T,
                       long N, long groups, int mask, int forced_root, long hysteresis, long min_note_frames, int gate_loudness,
                       float silence, float confidence, void *stream);
int ddsp_notes_render(const int *onset, const int *frames, const int *pitch, const int *detune, const float *level, const int *count,
                      const int *offset, float *f0, float *cents, float *loudness, float *harmonicity, uint8_t *voiced,
                      long *position, int *owner, long B, long T, long N, long groups, int flags, long transpose, long glide,
                      long attack, long release, long vibrato_delay, long vibrato_ramp, double vibrato_depth, double vibrato_omega,
                      float floor_level, float default_level, void *stream);

/*
 * The trainer's batch fetch from a device-resident training set (train/train.py:48: DataLoader(shuffle=True), collate, copy).
 *
 * ddsp_gather_batch  for each of n_arrays (<= DDSP_GATHER_MAX_ARRAYS) fp32 arrays: dst[a] [rows, row_floats[a]] row r <-
 *                    src[a] [n_examples, row_floats[a]] row perm[*cursor + r].  src, dst and row_floats are HOST arrays of
 *                    n_arrays entries (device addresses / lengths), read during the call; perm [perm_len] int64, cursor (one
 *                    int64) and error (one 32-bit word) are DEVICE memory, read when the kernel runs -- so a captured call
 *                    fetches the next batch at every replay.  With advance != 0 a second launch on the same stream then adds
 *                    rows to *cursor.  All arrays are copied by ONE launch whose grid is sized by bytes; rows whose length is a
 *                    multiple of 4 floats between 16-byte aligned bases move as 16-byte accesses, others as 4-byte ones.
 *                    No bad index is ever dereferenced: a position *cursor + r outside [0, perm_len) sets
 *                    DDSP_GATHER_BAD_CURSOR in *error, an example outside [0, n_examples) DDSP_GATHER_BAD_INDEX, and that row of
 *                    every dst is zero-filled.  The caller clears *error and reads it when it synchronises anyway.
 */
#define DDSP_GATHER_MAX_ARRAYS 8
#define DDSP_GATHER_BAD_INDEX 1
#define DDSP_GATHER_BAD_CURSOR 2
int ddsp_gather_batch(const void **src, void **dst, const long *row_floats, int n_arrays, const long *perm, long *cursor,
                      long perm_len, long n_examples, int rows, int advance, unsigned *error, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* DDSP_HIP_H */
