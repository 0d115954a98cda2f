/* mcvc.h -- C ABI of the MI355X-native MaskCycleGAN-VC hot path (libmcvc_hip.so, gfx950 only).
 *
 * The reference (GANtastic3/MaskCycleGAN-VC) has no FFI: its hot path is Python calling torch.nn
 * ops.  This ABI is the drop-in boundary *below* the Python nn.Module mirror in
 * maskcyclegan-vc_amd/mask_cyclegan_vc/: every entry point names the reference interface it
 * replaces (file:line relative to the reference repo root).
 *
 * Conventions
 *   - plain pointers and sizes; every pointer is a DEVICE pointer to contiguous fp32 unless noted;
 *   - `stream` is a hipStream_t passed as void* (0 = null stream); all calls are asynchronous w.r.t.
 *     the host and allocate no device memory on the compute path.  Process-wide state the library DOES keep
 *     (all behind mutexes): a pool of timing-less hipEvents for the lane <-> auxiliary-stream hand-offs, per-device
 *     weight-pack job tables (one small hipMalloc each on first use, outside stream capture), the cached workspace
 *     plans per (network, B, T), the deterministic-mode switch and the opt-in trace log.  Calls on different streams
 *     may be issued from different host threads, EXCEPT while the trace is enabled (its log is not thread-safe);
 *   - return value 0 = success, otherwise a hipError_t value or MCVC_ERR_* (>= 1000); the Python
 *     wrapper raises RuntimeError;
 *   - parameter tables are arrays of device pointers in the reference's `named_parameters()` order
 *     (Generator: 110 tensors, Discriminator: 20 tensors); gradient tables use
 *     the same order, entries may be NULL (skipped); gradients are ACCUMULATED (+=);
 *   - `packed` buffers hold the K-major re-packed weights the MFMA kernels read; they must be
 *     zero-initialised once by the caller and refreshed with mcvc_*_pack after every parameter update;
 *   - `stash` keeps what backward needs (conv outputs, InstanceNorm statistics, activations);
 *     `scratch` is transient (split-K slabs, gradient ping-pong buffers).
 */
#ifndef MCVC_H
#define MCVC_H

#ifdef __cplusplus
extern "C" {
#endif

#define MCVC_ABI_VERSION 3          /* r4: + mcvc_gen_backward_prefix, mcvc_set_trunk_passes_in_flight, op-level Winograd / staged-GEMM / trunk entries;
                                       3: + mcvc_gen_update_ranges / mcvc_disc_update_batch (optimizer step fused with the re-pack).
                                       Stays 3 where symbols, flag bits or argument values are only ADDED and every existing call keeps its
                                       meaning (MCVC_BWD_STORE_GRADS, mcvc_disc_backward_flags, mcvc_grad_store_mask, zero_grads == 2,
                                       mcvc_net_layout) */
#define MCVC_GEN_NPARAMS 110
#define MCVC_DISC_NPARAMS 20
#define MCVC_N_MEL 80

int mcvc_version(void);

/* Deterministic mode (default: env MCVC_DETERMINISTIC, else off).  When on, every reduction that would otherwise use
 * floating-point atomics (K-split accumulate of a conv / trunk data-gradient, the tiny-dW weight gradients) takes a
 * fixed-order path (private slabs summed by the consumer), so a step is bit-reproducible run to run like the
 * reference's CPU path.  Workspaces are always sized for both modes.  Returns the previous setting.             */
int mcvc_set_deterministic(int on);
int mcvc_get_deterministic(void);
/* Precise mode (default: env MCVC_PRECISE, else off; r6).  When on, the generators' 5x5 convolutions (model.py:86-99 downSample1/2,
 * :192-204 upSample1/2) run on the direct im2col-free kernels in every pass -- no Winograd scheme -- so the step's rounding is that of
 * plain fp32 sums, the reference's own (F.conv2d): against an fp64 run of the same four iterations the parameters then sit as close as
 * the reference's CPU fp32 arithmetic does (tests/test_hip_parity_fp64.py).  The default (fast) mode is 2-3x noisier on that measure and
 * inside 1e-3 on every single-iteration quantity.  Process-wide; set it before packing networks / building engines.  Returns the
 * previous setting.                                                                                                              */
int mcvc_set_precise(int on);
int mcvc_get_precise(void);
/* Small-batch generator passes (B * T/4 <= 32) run the 1-D trunk (six residual blocks + conv1dto2d, model.py:258-271) as ONE
 * persistent launch per direction instead of one fused launch per layer (default on).  Results are
 * bit-identical either way; the switch exists for A/B timing and tests.  Returns the previous setting.
 * The BACKWARD pass's data-gradient chain through the six blocks is one persistent launch as well (B * T/4 <= 16 at the 1024 staged
 * channels): on = 1 both directions, 2 forward only, 0 neither.  The persistent backward sums every K range in a
 * fixed order, so -- unlike the per-layer launches' atomic K-split -- its gradients are bit-reproducible in every mode; they agree with the
 * per-layer path to rounding.                                                                                  */
int mcvc_set_trunk_persistent(int on);

/* ---- grouped launches: two networks of the same architecture in one grid (new; the reference runs G_A2B / G_B2A and the discriminator
 *      pairs one after the other, train.py:203-216, 255-273).  Bracket TWO identical sequences of library calls that differ in pointers
 *      only (weights, activations, workspaces, destinations -- same B, T, flags, streams):
 *          mcvc_twin_begin();   <sequence on network 0>   mcvc_twin_switch();   <the same sequence on network 1>   rc = mcvc_twin_end();
 *      Between begin and switch nothing reaches the stream (the launches are recorded); the second sequence launches every kernel ONCE
 *      with gridDim.z = 2, one z-slice per network: half the launches, twice the workgroups per launch.  Any call that launches kernels
 *      may appear inside (passes, losses, packs, Adam); calls keep their meaning and return codes.  mcvc_twin_end returns MCVC_ERR_INVALID
 *      if the two sequences did not issue the same kernels with the same grids (nothing is repaired: treat the buffers as undefined).
 *      The bracket is per host thread; do not enqueue other work on the same streams between begin and switch (it would run BEFORE the
 *      grouped kernels).  The trace (mcvc_trace_*) counts a grouped launch once, with both networks' FLOPs and bytes.      */
int mcvc_twin_begin(void);
int mcvc_twin_switch(void);
int mcvc_twin_end(void);
int mcvc_twin_launches(void);           /* kernels recorded by the last bracket of this thread */

/* ---- sizes (floats) -------------------------------------------------------------------------- */
long long mcvc_gen_packed_floats(void);
long long mcvc_disc_packed_floats(void);
long long mcvc_gen_stash_floats(int B, int T);
long long mcvc_gen_scratch_floats(int B, int T);
long long mcvc_disc_stash_floats(int B, int T);
long long mcvc_disc_scratch_floats(int B, int T);
int mcvc_gen_out_frames(int T);          /* T' of Generator.forward (== T when T % 4 == 0) */
int mcvc_disc_out_frames(int T);         /* last dim of Discriminator.forward (T/8 when T % 8 == 0) */

/* ---- weight packing (after every optimizer step / load_state_dict) --------------------------- */
int mcvc_gen_pack(const float* const* params, float* packed, void* stream);
/*      Small-batch variant: when every pass until the next re-pack has batch <= max_batch at n_frames T and
 *      mcvc_gen_trunk_fused(max_batch, T) is 1, the 1-D trunk runs on the fused trunk kernels, which read the OIHW
 *      parameters directly -- the generic K-major copies of the trunk layers (60 % of the generator's weights) are then
 *      not refreshed.  Falls back to the full re-pack otherwise.                                                   */
int mcvc_gen_trunk_fused(int B, int T);
int mcvc_gen_pack_small_batch(const float* const* params, float* packed, int max_batch, int T, void* stream);
/* The same in two parts: sets = 1 refreshes only what a FORWARD pass reads (K-major forward copies, biases, forward Winograd sets),
 * sets = 2 only what a BACKWARD pass reads (data-gradient / transposed / data-gradient Winograd sets), 3 = both.  After sets = 1 a
 * backward pass on this buffer returns MCVC_ERR_INVALID until sets = 2 has run (the trainer's discriminator phase needs the updated
 * generators forward-only; the rest of the refresh runs beside it).                                    */
int mcvc_gen_pack_sets(const float* const* params, float* packed, int max_batch, int T, int sets, void* stream);
/* ... and restricted to parameter ranges (range_mask bit 0: parameters [100,110), bit 1: [24,100), bit 2: [0,24); 7 = all; r4: bits 3 / 4 / 5
 * = [12,24) / [4,12) / [0,4), the head in three parts -- see MCVC_BWD_FINE_MILESTONES): the ranges
 * whose gradients mcvc_gen_backward_overlap reports final one after the other, so that a range's optimizer step + re-pack can run beside the
 * rest of the backward pass.                                                                              */
int mcvc_gen_pack_ranges(const float* const* params, float* packed, int max_batch, int T, int sets, int range_mask, void* stream);
int mcvc_disc_pack(const float* const* params, float* packed, void* stream);
/*      The same restricted to what passes at n_frames T read when the three stride-2 layers run as implicit GEMMs (every batch size
 *      since r5): their tap-major K-major forward copy + biases only -- it serves the forward pass and, read row-major, the data gradient;
 *      the weight gradient reads no weights.  Falls back to the full re-pack when a layer would not take that path (planes whose width is
 *      no multiple of 8).  A pass that would need one of the stale copies returns MCVC_ERR_INVALID instead of reading it.                 */
int mcvc_disc_pack_small(const float* const* params, float* packed, int T, void* stream);
/*      ... for passes of up to max_batch samples (same copies at every max_batch since r5; the argument is kept for ABI 3).            */
int mcvc_disc_pack_batch(const float* const* params, float* packed, int max_batch, int T, void* stream);

/* ---- Generator: replaces Generator.forward (mask_cyclegan_vc/model.py:239-280) and its autograd
 *      x, mask: [B,80,T] (mask NULL = all ones, test.py:92); out: [B,80,T']
 *      T >= 5: at T <= 4 the residual trunk runs on a single frame, where the reference's InstanceNorm1d raises
 *      ("Expected more than 1 spatial element"); every generator pass (forward, backward, bf16 inference) then
 *      returns MCVC_ERR_INVALID.                                                                    */
int mcvc_gen_forward(const float* const* params, const float* packed, const float* x, const float* mask,
                     float* out, float* stash, float* scratch, long long scratch_floats, int B, int T, void* stream);
/*      dout: [B,80,T'] ; dx (nullable): [B,80,T], written or accumulated (accumulate_dx != 0)      */
int mcvc_gen_backward(const float* const* params, const float* packed, float* const* grads, const float* mask,
                      const float* dout, float* dx, int accumulate_dx, const float* stash,
                      float* scratch, long long scratch_floats, int B, int T, void* stream, void* aux_stream);
/*      aux_stream (nullable): a second hipStream_t on which the weight-gradient kernels run beside the data-gradient
 *      chain; the call returns with `stream` ordered after everything launched on aux_stream.            */
/*      Same, plus gradient-ready milestones for overlapping a data-parallel all-reduce with the rest of the pass
 *      (new: the reference has no distributed code).  milestones (nullable): two caller-owned hipEvent_t handles;
 *      [0] is recorded once every gradient of parameters [100,110) (upSample1/2 + lastConvLayer; named_parameters()
 *      order) has been produced, [1] once those of [24,100) (six residual blocks + conv1dto2d) have; the remaining
 *      [0,24) are complete when the call's work on `stream` is.  A consumer stream waits on the event.       */
int mcvc_gen_backward_overlap(const float* const* params, const float* packed, float* const* grads, const float* mask,
                              const float* dout, float* dx, int accumulate_dx, const float* stash,
                              float* scratch, long long scratch_floats, int B, int T, void* stream, void* aux_stream,
                              void* const* milestones);

/*      The small-batch passes run the residual trunk as ONE persistent launch whose 64 workgroups hand activations to each other inside
 *      the kernel (bounded spins).  Should a workgroup ever give up (the device cannot keep all 64 resident: more than four such passes in
 *      flight at once), the pass's output is poisoned with NaN -- so every loss of the step turns non-finite -- and an error word in the
 *      scratch buffer records the layer.  mcvc_gen_trunk_fault reads that word (0 = none, 1 + layer otherwise, negative = call failed) and
 *      optionally clears it; it SYNCHRONISES `stream`.  Call it with reset != 0 once after allocating a scratch buffer (the word is not
 *      initialised by the passes), then e.g. once per logging interval.  mcvc_debug_trunk_fault_inject(1) makes the following persistent
 *      launches lose one arrival (test hook for exactly this path); returns the previous setting.             */
int mcvc_gen_trunk_fault(float* scratch, int B, int T, int reset, void* stream);
int mcvc_debug_trunk_fault_inject(int on);

/*      Same with flags.  MCVC_BWD_NO_JOIN (1): return WITHOUT ordering `stream` after the weight-gradient kernels still running on aux_stream
 *      (the data-gradient result dx is complete on `stream`).  The caller then owes: (i) the next pass that accumulates into the same gradient
 *      tensors uses the SAME aux_stream (in-order) or waits for it, (ii) `scratch` and `stash` of this pass stay untouched until aux_stream
 *      has drained (the next pass uses other buffers), (iii) a later pass on that aux_stream joins (flags = 0) before the gradients are read.
 *      The trainer runs the cycle pass's backward this way: the translation pass's data-gradient chain starts ~0.2 ms earlier.       */
#define MCVC_BWD_NO_JOIN 1
/*      flags & MCVC_BWD_FINE_MILESTONES (r4): `milestones` holds FOUR events; [2] is recorded when the gradients of parameters [12,24)
 *      (downSample2, conv2dto1d) are final, [3] when those of [4,12) (downSample1) are: the head of the network in the order a backward pass
 *      finishes it, so that the optimizer step of all but conv1 (mcvc_gen_update_ranges, range_mask bits 8 / 16 / 32 = [12,24) / [4,12) /
 *      [0,4); bit 4 = their union, not to be combined with them) runs beside the rest of the pass instead of behind it.                */
#define MCVC_BWD_FINE_MILESTONES 2
/*      flags & MCVC_BWD_STORE_GRADS: on return every COVERED parameter gradient (mcvc_grad_store_mask: the weight tensors of the Winograd
 *      layers, the implicit-GEMM layers and the wide 1 x KW convolutions of the 1-D trunk -- more than 99 % of the parameters) EQUALS this
 *      pass's gradient, whatever the buffer held before: its writers store instead of reading the old value and adding to it.  The
 *      uncovered gradients (biases, norm affine parameters, the edge layers) are accumulated into, as without the flag.  Where the writer
 *      the planner picks for a covered layer can only add (an odd frame count, a missing workspace), the tensor is zero-filled first: the
 *      contract holds for every shape.  The first weight-gradient pass after an update with zero_grads == 2 passes it; later passes of the
 *      iteration do not.  The op-level entries (mcvc_conv2d_wgrad, mcvc_layer_*) accumulate; mcvc_layer_wgrad_flags alone takes this flag,
 *      so that one layer's store mode -- a pass in several sample chunks -- can be driven without a whole network.                      */
#define MCVC_BWD_STORE_GRADS 4
/*      covered[p] = 1 for the parameter tensors of network `net` (0 generator, 1 discriminator) that a store pass covers, else 0; 128 bytes
 *      are written.  Host only, no device call; a property of the layers alone: the mask is the same for every T >= 1 (the argument
 *      is checked and otherwise unused -- which WRITER a covered layer gets depends on T, whether it is covered does not).  Returns
 *      the network's parameter count (MCVC_GEN_NPARAMS / MCVC_DISC_NPARAMS), or MCVC_ERR_INVALID.                                       */
int mcvc_grad_store_mask(int net, int T, unsigned char* covered);
int mcvc_gen_backward_flags(const float* const* params, const float* packed, float* const* grads, const float* mask,
                            const float* dout, float* dx, int accumulate_dx, const float* stash,
                            float* scratch, long long scratch_floats, int B, int T, void* stream, void* aux_stream,
                            void* const* milestones, int flags);
/*      Backward over a PREFIX of a forward pass's samples (r4).  `stash` was written by mcvc_gen_forward with batch stash_B >= B; the pass
 *      back-propagates through its first B samples only (mask / dout / dx hold B samples; scratch is sized for B).  The trainer batches
 *      the discriminator phase's generator forwards of iteration t (train.py:259-273: outputs only, their backward is discarded) into the
 *      generator phase's forwards of iteration t+1 (train.py:203-210: same weights), so those passes run over 3 (2) samples and their
 *      backward over the first 2 (1).  The 2-D stash tensors are batch-major; the 1-D trunk's are [C][stash_B][T/4] and are read with that
 *      channel pitch.  stash_B == B is mcvc_gen_backward_flags.                                                                      */
int mcvc_gen_backward_prefix(const float* const* params, const float* packed, float* const* grads, const float* mask,
                             const float* dout, float* dx, int accumulate_dx, const float* stash, int stash_B,
                             float* scratch, long long scratch_floats, int B, int T, void* stream, void* aux_stream,
                             void* const* milestones, int flags);
/*      ... over the WINDOW [stash_b0, stash_b0 + B) of the forward pass's samples (stash_b0 * T/4 must be a multiple of 4).  The trainer
 *      back-propagates the identity sample of a merged pass (train.py:223-224: depends on nothing but its own forward) while the
 *      discriminators of the cycle chain are still running, and the translation sample -- the window [1, 2) -- at the end of the chain.  */
int mcvc_gen_backward_window(const float* const* params, const float* packed, float* const* grads, const float* mask,
                             const float* dout, float* dx, int accumulate_dx, const float* stash, int stash_B, int stash_b0,
                             float* scratch, long long scratch_floats, int B, int T, void* stream, void* aux_stream,
                             void* const* milestones, int flags);
/*      Number of persistent trunk passes the caller keeps in flight at once (a grouped launch counts as two; default 2).  The persistent
 *      kernels' 64 workgroups per pass wait for each other inside the kernel, so all of them must be resident: they are used only while
 *      64 x that number <= the device's compute units, otherwise the passes fall back to per-layer launches.  Returns the previous value. */
int mcvc_set_trunk_passes_in_flight(int n);
/*      bit 0 / bit 1: a (B, T) generator pass would run its forward / backward trunk on the persistent kernels under the current
 *      switches and residency bound (0: per-layer launches).                                                                          */
int mcvc_gen_trunk_persistent(int B, int T);

/* ---- Generator inference in bf16 (BASELINE configs[4]: generator_A2B, bs=16, 80 x 512 frames).  Replaces the call
 *      `generator(real, ones_like(real))` of the reference's inference driver (mask_cyclegan_vc/test.py:92, 107 ->
 *      Generator.forward, model.py:239-280) when the caller asks for bf16: NHWC bf16 activations, bf16 MFMA with fp32
 *      accumulation, fp32 InstanceNorm statistics; x / mask / out stay fp32 [B,80,T] at the boundary.
 *      packed: mcvc_gen_bf16_packed_bytes() bytes, refreshed with mcvc_gen_bf16_pack after every parameter change
 *      (weights are cast from the fp32 parameters); workspace: mcvc_gen_bf16_workspace_bytes(B, T) bytes, 256-byte aligned;
 *      mask NULL = all ones.  No gradient path.                                                               */
long long mcvc_gen_bf16_packed_bytes(void);
long long mcvc_gen_bf16_workspace_bytes(int B, int T);
int mcvc_gen_bf16_pack(const float* const* params, void* packed, void* stream);
int mcvc_gen_infer_bf16(const float* const* params, const void* packed, const float* x, const float* mask, float* out, void* workspace,
                        long long workspace_bytes, int B, int T, void* stream);

/*      single-op entry points of the bf16 path (kernel parity tests; same kernels the forward uses).  Tensors are NHWC bf16
 *      (raw 16-bit storage = torch.bfloat16): y[N][OH][OW][Cout] = conv2d(x[N][H][W][Cin], w[Cout][Cin][KH][KW] fp32 -> bf16) + bias;
 *      Cin % 32 == 0, Cout % 4 == 0; wpack: mcvc_bf16_conv2d_pack_bytes() bytes of scratch.                      */
long long mcvc_bf16_conv2d_pack_bytes(int Cout, int Cin, int KH, int KW);
int mcvc_bf16_conv2d(const void* x, const float* w, const float* bias, void* y, void* wpack, int N, int H, int W, int Cin, int Cout,
                     int KH, int KW, int stride, int pad_h, int pad_w, void* stream);
/*      Host view of what the bf16 convolution launcher decides for a problem (pure host code, no device call; the launcher runs this very
 *      plan).  mcvc_bf16_conv_plan: the problem of mcvc_bf16_conv2d with the same arguments (same Cout padding); returns what that launch
 *      would return, 0 or MCVC_ERR_INVALID, and fills out[0..12] (n_out >= 13) with
 *        cfg (tile configuration: 0 = 128 x 128, 1 = 64 x 64, 2 = 32 x 128, 3 = 128 x 64, 4 = 128 x 256, 5 = 128 x 512), BM, BN,
 *        KWT, PPT (the instantiated compile-time kernel width and input-prefetch depth; 0 = run-time width / synchronous staging),
 *        TH, TW (pixel tile), tiles_h, tiles_w, PH, PW (staged input patch: rows, row pitch in pixels), LDS bytes,
 *        1 when the kernel maps workgroups to tiles XCD-wise (0: channel tile = block % channel tiles).
 *      Fields decided before a rejection are filled, the rest are 0 (cfg = -1 when nothing was decided).
 *      mcvc_gen_bf16_conv_plans: one row of 14 ints {layer id, the 13 fields} per convolution that mcvc_gen_infer_bf16(B, T) runs on the
 *      generic kernel, in call order -- the forward itself in a plan-only mode, so fused layers (no row) and the unfused trunk are chosen as
 *      a real call chooses them.  Layer ids: 0 conv1, 1 downSample1, 2 downSample2, 3 conv2dto1d, 4 conv1dto2d, 5 upSample1, 6 upSample2,
 *      7 last conv, 10 + i / 20 + i the value|gate / output convolution of residual block i.  *n = rows of the plan; returns the first
 *      layer's error if a layer has no valid plan (what the forward would return), MCVC_ERR_WORKSPACE when cap is smaller than *n (the first
 *      cap rows are written), else 0.                                                                                                  */
int mcvc_bf16_conv_plan(int N, int H, int W, int Cin, int Cout, int KH, int KW, int stride, int pad_h, int pad_w, int* out, int n_out);
int mcvc_gen_bf16_conv_plans(int B, int T, int* rows, int cap, int* n);
/*      conv1 of the bf16 forward with its input preparation and gated GLU fused (r6; model.py:241-242):
 *      y[B][80][T][128] bf16 NHWC = conv2d(stack(x * mask, mask), w, b, padding (2, 7)) * sigmoid(conv2d(..., wg, bg)); x, mask fp32 [B][80][T]
 *      (mask NULL = ones), w / wg [128][2][5][15], b / bg [128] fp32; wpack: mcvc_bf16_conv1_glu_pack_bytes() bytes, 16-byte aligned.     */
long long mcvc_bf16_conv1_glu_pack_bytes(void);
int mcvc_bf16_conv1_glu(const float* x, const float* mask, const float* w, const float* b, const float* wg, const float* bg, void* y, void* wpack,
                        int B, int T, void* stream);
/*      the generator's last conv (r6; model.py:207-211, 278-279) through the fused kernel of the bf16 forward: out[B][80][T] fp32 =
 *      conv2d(x[B][80][T][128] bf16 NHWC, w[1][128][5][15], b[1], padding (2, 7)); wpack: mcvc_bf16_last_conv_pack_bytes() bytes, 16-byte aligned. */
long long mcvc_bf16_last_conv_pack_bytes(void);
int mcvc_bf16_last_conv(const void* x, const float* w, const float* b, float* out, void* wpack, int B, int T, void* stream);
/*      conv2dto1d (Conv1d 5120 -> 256, k = 1) + conv2dto1dLayer_tfan (r6; model.py:142-146, 254-255) through the fused kernel of the bf16 forward:
 *      x [B][W][5120] bf16 whose memory channel h * 256 + c holds the reference's channel c * 20 + h (the view(B, 5120, 1, -1) of :249-251 as the
 *      forward lays it out), w [256][5120] fp32 in the reference's order, gamma / beta [256]; y [B][W][256] bf16.  W <= 128 else MCVC_ERR_INVALID.  */
long long mcvc_bf16_c2d1d_pack_bytes(void);
int mcvc_bf16_c2d1d_norm(const void* x, const float* w, const float* gamma, const float* beta, void* y, void* wpack, int B, int W, void* stream);
/*      one layer of a residual block (r6; model.py:47-76) through the fused kernel of the bf16 forward -- Conv1d(k = 3, padding 1) + InstanceNorm1d
 *      (affine) + {value * sigmoid(gate) when w_gate != NULL | + residual}: x [B][W][Cin], y / residual [B][W][C] bf16 (channel-innermost);
 *      w / w_gate [C][Cin][3], gamma / beta (+ the gate's) [C] fp32.  W <= 128, Cin = 256 or 512, C % 32 == 0, else MCVC_ERR_INVALID
 *      (the forward then runs conv + norm as two launches).  wpack: mcvc_bf16_trunk_layer_pack_bytes() bytes, 16-byte aligned.               */
long long mcvc_bf16_trunk_layer_pack_bytes(int Cin, int C, int gated);
int mcvc_bf16_trunk_layer(const void* x, const float* w, const float* w_gate, const float* gamma, const float* beta, const float* gamma_gate,
                          const float* beta_gate, const void* residual, void* y, void* wpack, int B, int W, int Cin, int C, void* stream);
/*      y = act(InstanceNorm(x)) (+ residual): act 0 none, 1 gated GLU (Cx = 2C: value | gate), 2 x*sigmoid(x); pixel_shuffle != 0:
 *      the normalised tensor is PixelShuffle(2)(x), output [N][2H][2W][Cx/4].  scratch: N * 65 * Cx * 2 floats.      */
int mcvc_bf16_instnorm_act(const void* x, const float* gamma, const float* beta, const float* gamma_gate, const float* beta_gate,
                           const void* residual, void* y, float* scratch, int N, int H, int W, int Cx, int act, int pixel_shuffle, void* stream);

/* ---- Discriminator: replaces Discriminator.forward (model.py:340-349) and its autograd
 *      x: [B,80,T]; out: [B,1,10,T8] sigmoid probabilities                                          */
int mcvc_disc_forward(const float* const* params, const float* packed, const float* x, float* out,
                      float* stash, float* scratch, long long scratch_floats, int B, int T, void* stream);
/*      dout: [B,1,10,T8]; grad wrt the sigmoid OUTPUT (dout_is_logit_grad == 0) or wrt the pre-sigmoid
 *      logits (!= 0, what mcvc_lsgan_loss emits).  grads NULL = data-gradient only (generator phase,
 *      train.py:211-216 -- the reference computes D weight grads there and discards them).          */
int mcvc_disc_backward(const float* const* params, const float* packed, float* const* grads,
                       const float* dout, int dout_is_logit_grad, float* dx, int accumulate_dx,
                       const float* stash, float* scratch, long long scratch_floats, int B, int T, void* stream,
                       void* aux_stream);
/*      ... with flags: MCVC_BWD_STORE_GRADS as for the generator (any other bit: MCVC_ERR_INVALID); flags = 0 is mcvc_disc_backward.     */
int mcvc_disc_backward_flags(const float* const* params, const float* packed, float* const* grads,
                             const float* dout, int dout_is_logit_grad, float* dx, int accumulate_dx,
                             const float* stash, float* scratch, long long scratch_floats, int B, int T, void* stream,
                             void* aux_stream, int flags);

/* ---- losses (train.py:219-237, 276-294). loss_slot/term_slot: device floats, accumulated (+=) -- */
/* loss_slot += weight*mean|a-b|, term_slot += mean|a-b|, grad_a (=|+=) weight*sign(a-b)/n           */
int mcvc_l1_loss(const float* a, const float* b, long long n, float weight, float* loss_slot, float* term_slot,
                 float* grad_a, int accumulate_grad, void* stream);
/* d = discriminator sigmoid output; loss_slot += weight*mean((target-d)^2);
 * grad_logit = d(loss)/d(pre-sigmoid logit)                                                         */
int mcvc_lsgan_loss(const float* d, long long n, float target, float weight, float* loss_slot, float* term_slot,
                    float* grad_logit, void* stream);

/* The terms of one phase may be produced on different streams, each into its own pair pairs[2k] = weight*mean, pairs[2k+1] = mean
 * (pass them as loss_slot / term_slot above, zeroed before).  This adds pair k to slots[loss_dst[k]] / slots[term_dst[k]] (-1 =
 * skip), k = 0..n-1 in that order (n <= 16; the two index arrays are HOST memory): the order of the reference's sums
 * (train.py:233-237, 276-294) whatever the streams' timing was.                                       */
int mcvc_loss_combine(const float* pairs, int n, const int* loss_dst, const int* term_dst, float* slots, void* stream);

/* ---- optimizer: torch.optim.Adam(betas, eps, weight_decay=0) on a flat buffer (train.py:119-122) */
int mcvc_adam_step(float* p, const float* g, float* exp_avg, float* exp_avg_sq, long long n, float lr,
                   float beta1, float beta2, float eps, int step, float grad_scale, void* stream);
/*      The same step on the gradient g + g2 (g2 nullable: a second buffer that independent backward passes accumulated into, so that they need
 *      not be ordered against the passes that write g), optionally clearing the gradient buffer(s) behind the read (zero_grads != 0: what
 *      reset_grad / zero_grad, train.py:157-161, does before the next accumulation -- here without a separate pass over the buffers).   */
int mcvc_adam_step2(float* p, float* g, float* g2, int zero_grads, float* exp_avg, float* exp_avg_sq, long long n, float lr,
                    float beta1, float beta2, float eps, int step, float grad_scale, void* stream);
/*      optimizer.step() fused with the weight re-pack (reference train.py:242 / :299 are just `optimizer.step()`: the packed copies are this
 *      library's own, so their refresh belongs to the step): ONE launch in which a workgroup owns a tile of filters of one parameter tensor --
 *      it applies the Adam update above to the tile (bit-identical to mcvc_adam_step2), keeps the new weights in LDS and writes every packed
 *      copy derived from them (K-major / tap-major / data-gradient / transposed trunk / Winograd U sets) from there.  No second
 *      pass over the OIHW tensors: the per-step `pack` kernel family is gone (it remains for load_state_dict: mcvc_*_pack*).
 *      numel[i]: elements of parameter tensor i (0: a parameter that is neither updated nor packed -- the unused downSample4 block);
 *      flat / grad / grad2 (nullable) / exp_avg / exp_avg_sq: flat buffers in which params[i], its gradient(s) and moments sit at EQUAL
 *      offsets (gradient of params[i] = grad + (params[i] - flat)); range_mask / max_batch / T as mcvc_gen_pack_ranges / mcvc_disc_pack_batch.
 *      zero_grads: 0 leave the gradients, 1 clear them behind the read, 2 clear only the tensors a store pass does not cover
 *      (mcvc_grad_store_mask) and leave the covered ones as they are -- the next pass over the network passes MCVC_BWD_STORE_GRADS and never
 *      reads them, so neither the zeros' store nor their load happens (28 instead of 32 bytes per covered parameter).  2 needs grad2 == NULL;
 *      any other value, or 2 with a grad2: MCVC_ERR_INVALID.                                                                            */
int mcvc_gen_update_ranges(const float* const* params, const long long* numel, float* packed, int max_batch, int T, int range_mask,
                           const float* flat, float* grad, float* grad2, float* exp_avg, float* exp_avg_sq, float lr, float beta1,
                           float beta2, float eps, int step, float grad_scale, int zero_grads, void* stream);
int mcvc_disc_update_batch(const float* const* params, const long long* numel, float* packed, int max_batch, int T,
                           const float* flat, float* grad, float* grad2, float* exp_avg, float* exp_avg_sq, float lr, float beta1,
                           float beta2, float eps, int step, float grad_scale, int zero_grads, void* stream);

/* Host view of the job table a re-pack or fused update would use (pure host code, no device call): what mcvc_gen_pack_ranges (net 0) /
 * mcvc_disc_pack_batch (net 1; sets = 3, range_mask = 7) or, with update = 1, mcvc_gen_update_ranges / mcvc_disc_update_batch builds for
 * these arguments, as rows of 20 64-bit integers whose first entry names the record:
 *   0  header: net, update, jobs, owners, dgrad-argument entries, workgroups, packed floats, traced bytes and written bytes (bit patterns of
 *      the doubles), the planner's flags (generator: fused | wino_only<<1 | w4<<2 | w43<<3 | up1_w4<<4 | up1_w2<<5 | up2_w2<<6;
 *      discriminator: 1 full table, 4 implicit-GEMM table), 20
 *   1  job, in table order: layer index, form, kind, param, dst, floats of the region [dst, dst + len) it writes into, block0, gx, Cout, Cin,
 *      K, ld, co_off, KW, taps, xi_stride, dg
 *   2  owner (update = 1): param, block0, gx, Cout, Cin, taps, CB, IB, e0, ne, flat, vec4
 *   3  per layer the call touches: layer index, sets, the mask of forms it leaves fresh there
 *   4  dgrad arguments: index, Cin, KH, KW, step, ld, co_off, merged, mg_kh, mg_kw, ncls, tapmajor, cout_rows
 *   5  one of their classes: index, class, nth, ntw, khmax, kwmax, pad_h, pad_w, qh, qw, su, sv, offset
 * *n_rows = rows of the plan; MCVC_ERR_WORKSPACE when cap is smaller (the first cap rows are written), MCVC_ERR_INVALID as the entries. */
int mcvc_pack_plan(int net, int max_batch, int T, int sets, int range_mask, int update, long long* rows, int cap, int* n_rows);
/* Host view of the stash and scratch layouts of a (B, T) pass (pure host code, no device call): net 0 the generator, 1 the discriminator.
 * stash_B / stash_b0 as mcvc_gen_backward_window: the stash was written by a forward pass over stash_B samples (0 = B) and the pass walks
 * the samples [stash_b0, stash_b0 + B) of it; the discriminator has no windows (stash_B = 0 or B, stash_b0 = 0).  Rows of 12 64-bit integers:
 *   1  stash tensor, in stash order:  id, offset, floats (of all stash_B samples), N, C, H, W, sample / channel / row stride as the
 *      backward pass addresses it, offset of the window's first sample
 *   2  scratch buffer up to the slabs: the same columns (N .. strides = 0 for the untyped ping-pong buffers and workspaces)
 *   3  last row: 0, then the dry run's conv-slab, weight-gradient-slab, staging and weight-staging floats and the slab offset
 * Offsets are multiples of 4 floats; a row ends where the next begins (floats rounded up to 4), the last stash row at mcvc_*_stash_floats,
 * the last scratch row at the slab offset.  *n_rows / cap / return value as mcvc_pack_plan.                                              */
int mcvc_net_layout(int net, int B, int T, int stash_B, int stash_b0, long long* rows, int cap, int* n_rows);
int mcvc_axpy(float* y, const float* x, float alpha, long long n, void* stream);

/* ---- on-device input pipeline: replaces VCDataset.__getitem__ + DataLoader collate + 4 H2D copies per iteration
 *      (dataset/vc_dataset.py:19-77, mask_cyclegan_vc/train.py:82-96, 187-190) with one launch per minibatch.
 *      bank_X: [80][frames_X] fp32, all utterances of speaker X side by side along the frame axis; offs_X: int32 [n_X+1]
 *      first frame of each utterance (every utterance >= T frames).  Per sample and speaker: utterance ~ U{0..n-1},
 *      crop lo ~ U{0..len-T}, mask size ~ U{0..max_mask_len-1}, start ~ U{0..T-size-1} -- the reference's distributions
 *      (vc_dataset.py:33-70) from a counter-based SplitMix64 stream keyed by (seed, step, sample, speaker): restated
 *      bit-exactly in oracle/sampler_oracle.py.  Outputs [B][80][T]; draws (nullable): int32 [B][2][4] =
 *      (utterance, lo, size, start).                                                                        */
int mcvc_draw_batch(const float* bank_A, const int* offs_A, int n_A, long long frames_A, const float* bank_B, const int* offs_B, int n_B,
                    long long frames_B, int B, int T, int max_mask_len, unsigned long long seed, unsigned long long step,
                    float* real_A, float* mask_A, float* real_B, float* mask_B, int* draws, void* stream);

/* ---- waveform -> log-mel front-end (new: the reference computes its mel-spectrograms with the MelGAN vocoder's Audio2Mel module,
 *      fetched through torch.hub -- data_preprocessing/preprocess_vcc2018.py:26-60, mask_cyclegan_vc/utils.py).  The fixed transform
 *      Audio2Mel(n_fft 1024, hop 256, win 1024, 22050 Hz, 80 mel rows, fmin 0, fmax 11025) of a mono float waveform of L samples:
 *      reflect-pad 384 each side, T = (L - 256) / 256 + 1 frames of 1024 at hop 256, periodic Hann, |DFT| of bins 0..512, the
 *      [80][513] Slaney mel filterbank, log10(max(., 1e-5)).  L < 385 is refused (reflect padding needs L > 384).
 *      A BANK is n utterances concatenated in one fp32 buffer + int32 sample offsets [n + 1] (the layout of mcvc_draw_batch's banks);
 *      one launch turns it into out [80][total_frames], utterance u in columns frame_offs[u] .. frame_offs[u + 1].
 *        mcvc_audio_frames       frames of an L-sample utterance; 0 when L < 385.
 *        mcvc_audio_basis_floats size of the constant operand: the windowed cos / sin DFT basis in the order the kernel's lanes read it,
 *                                followed by the sparse mel table.
 *        mcvc_audio_basis_init   fills it, computed in float64 and rounded once.  `basis` is a HOST buffer; the caller uploads it
 *                                (16-byte aligned) and keeps it: it never changes.
 *        mcvc_audio_plan         HOST tables in, HOST tables out: frame_offs [n + 1] and the launch's work list tiles [n_tiles][4] int32
 *                                (at most 64 frames of one utterance each).  tiles == NULL: only *n_tiles and frame_offs are written.
 *                                MCVC_ERR_INVALID: n < 1, an utterance under 385 samples, >= 2^31 frames; MCVC_ERR_WORKSPACE: max_tiles
 *                                too small.
 *        mcvc_audio_log_mel      the launch: wave, tiles (16-byte aligned), basis, out are DEVICE pointers.  A work item that does not
 *                                lie inside [0, n_samples) x [0, total_frames) is skipped, never followed out of bounds.            */
int mcvc_audio_frames(int n_samples);
long long mcvc_audio_basis_floats(void);
int mcvc_audio_basis_init(float* basis);
int mcvc_audio_plan(const int* sample_offs, int n_utts, int* frame_offs, int* tiles, int max_tiles, int* n_tiles);
int mcvc_audio_log_mel(const float* wave, long long n_samples, const int* tiles, int n_tiles, const float* basis, float* out,
                       long long total_frames, void* stream);

/* ---- MelGAN decoder, log-mel -> waveform (new: the reference ends its inference driver in vocoder.inverse(mel) of the torch.hub MelGAN
 *      model -- mask_cyclegan_vc/test.py:94-103, utils.py:25-39).  Generator(input_size 80, ngf 32, n_residual_layers 3) of Kumar et al.
 *      2019 in fp32, inference only: mel [B][80][T] log10-mel -> out [B][256 T], T >= 4 (ReflectionPad1d(3)).  42 weight-normed Conv1d /
 *      ConvTranspose1d layers in state-dict order: 0 = model.1; stage s = 0..3 starts at 1 + 10 s with its transposed conv, followed per
 *      residual block by (block.2, block.4, shortcut); 41 = model.24.  One arithmetic, one accumulation order, no atomics: results are
 *      bit-reproducible whatever mcvc_set_deterministic says, and a sample's result does not depend on its batch.
 *        mcvc_voc_out_samples       256 T; 0 when T < 4.
 *        mcvc_voc_launches          kernel launches of one decode (30).
 *        mcvc_voc_packed_floats     size of the packed weights.
 *        mcvc_voc_pack              host_table: 42 x (weight, bias) HOST fp32 pointers with weight norm already folded (w = g v / ||v||, the
 *                                   norm over every dimension but 0), in torch's layouts ([Cout][Cin][k]; transposed: [Cin][Cout][2r]);
 *                                   packed_host: HOST buffer.  The caller uploads it (16-byte aligned) and keeps it per checkpoint.
 *        mcvc_voc_workspace_floats  transient activations of one decode; monotone in B and T.
 *        mcvc_voc_decode            all 30 launches on `stream`; no device allocation.  MCVC_ERR_INVALID: T < 4, B < 1, a misaligned
 *                                   pointer (packed, workspace, out: 16 bytes); MCVC_ERR_WORKSPACE: workspace too small -- nothing is launched.
 *      One layer through the same kernels (op-level parity).  kind: 0 Conv1d with reflection padding (k - 1) dilation / 2 (k odd);
 *      1 ConvTranspose1d(k = 2r, stride r, padding r / 2; r = 2, 4, 8, 16), y [B][Cout][r L]; 2 the stacked residual product
 *      y = w0 @ x0 + b0 + w1 @ lrelu(x1) + b1 (1 x 1, Cin = Cout); 3 LeakyReLU + Conv1d(Cin, 1, k) + tanh, y [B][L].  act_in: LeakyReLU(0.2)
 *      on the input of kinds 0 and 1.  Cout * max(r / 2, 1) % 32 == 0 and Cin % 16 == 0, else mcvc_voc_layer_packed_floats returns 0 and
 *      the others MCVC_ERR_INVALID.  mcvc_voc_layer_pack is HOST -> HOST like mcvc_voc_pack; packed and y are 16-byte aligned DEVICE pointers. */
int mcvc_voc_out_samples(int T);
int mcvc_voc_launches(void);
long long mcvc_voc_packed_floats(void);
int mcvc_voc_pack(const float* const* host_table, float* packed_host);
long long mcvc_voc_workspace_floats(int B, int T);
int mcvc_voc_decode(const float* packed, const float* mel, float* out, float* workspace, long long workspace_floats, int B, int T, void* stream);
long long mcvc_voc_layer_packed_floats(int kind, int Cin, int Cout, int k, int r);
int mcvc_voc_layer_pack(int kind, const float* w0, const float* b0, const float* w1, const float* b1, float* packed_host, int Cin, int Cout, int k, int r);
int mcvc_voc_layer(int kind, const float* packed, const float* x0, const float* x1, float* y, int B, int Cin, int Cout, int L, int k, int dilation, int r,
                   int act_in, void* stream);

/* ---- Griffin-Lim decoder, log-mel or linear magnitude -> waveform (new: audio without a vocoder checkpoint).  Phase reconstruction
 *      against the front-end's own STFT (reflect-pad 384, frames of 1024 at hop 256, periodic Hann w, bins 0..512), fp32, no weights:
 *        M = max(0, pinv(mel basis) @ 10^logmel), or the linear input;
 *        ISTFT(S): y[p] = sum_t (w irfft(S[:, t]))[p - 256 t] / sum_t w^2[p - 256 t], kept for p in [384, 384 + 256 T);
 *        A_0 = angles0 (unit modulus; NULL: zero phase), R_-1 = 0; for k < n_iter: R_k = STFT(ISTFT(M A_k)),
 *        Z = R_k - momentum / (1 + momentum) R_k-1, A_k+1 = Z / |Z| (0 where Z is 0);  out = ISTFT(M A_n_iter).
 *      in [B][80][T] (in_kind 0, log10-mel) or [B][513][T] (in_kind 1, magnitude >= 0); angles0 [B][513][T][2] = (re, im); out [B][256 T].
 *      No atomics, one accumulation order: bit-reproducible, and a sample's result does not depend on its batch.
 *        mcvc_gl_out_samples       256 T; 0 when T < 2 (256 T >= 385 samples: the front-end's reflect-padding rule).
 *        mcvc_gl_launches          kernel launches of one decode: 2 n_iter + 3; 0 when n_iter < 0.
 *        mcvc_gl_tables_floats     size of the constant operand: the inverse DFT basis in the order the kernel's lanes read it, the
 *                                  pseudo-inverse of the mel basis, the squared window and the front-end's operand (mcvc_audio_basis_init).
 *        mcvc_gl_tables_init       fills it.  host_pinv: HOST [513][80] fp32, the pseudo-inverse of the [80][513] mel basis, computed by the
 *                                  caller in float64; host_out: HOST buffer.  The caller uploads it (16-byte aligned) once per device.
 *        mcvc_gl_workspace_floats  transient state of one decode; monotone in B and T; 0 when B < 1, T < 2, B > 65535 or B T > 2^22.
 *        mcvc_gl_decode            all launches on `stream`; no device allocation.  MCVC_ERR_INVALID: a null in / tables / out, a misaligned
 *                                  pointer (in, out: 4 bytes; angles0: 8; tables, workspace: 16), T < 2, B < 1, n_iter < 0, momentum outside
 *                                  [0, 1), an unknown in_kind; MCVC_ERR_WORKSPACE: workspace null or too small -- nothing is launched.      */
int mcvc_gl_out_samples(int T);
int mcvc_gl_launches(int n_iter);
long long mcvc_gl_tables_floats(void);
int mcvc_gl_tables_init(const float* host_pinv, float* host_out);
long long mcvc_gl_workspace_floats(int B, int T);
int mcvc_gl_decode(const float* in, int in_kind, const float* angles0, const float* tables, float* out, float* workspace,
                   long long workspace_floats, int B, int T, int n_iter, float momentum, void* stream);

/* ---- mel inversion by non-negative least squares (new): log-mel [B][80][T] -> linear magnitude [B][513][T], what mcvc_gl_decode takes
 *      as in_kind 1 (csrc/melinv_kernels.hip; mask_cyclegan_vc/melinv.py and INTEGRATION.md restate this).  With y = 10^logmel, Bm the
 *      [80][513] mel basis, P its pseudo-inverse, s = 1 / lambda, lambda the largest eigenvalue of Bm Bm^T, and beta_k = (t_k - 1) / t_k+1,
 *      t_0 = 1, t_k+1 = (1 + sqrt(1 + 4 t_k^2)) / 2 (float64 on the host, rounded once to fp32), per frame:
 *        M_0 = max(0, P y), the decoder's own start value bit for bit (exp10f, one fmaf chain over filters 0..79 from zero); Z_0 = M_0;
 *        for k < n_iter:  r = Bm Z_k - y;  M_k+1 = max(0, Z_k - s Bm^T r);  Z_k+1 = M_k+1 + beta_k (M_k+1 - M_k);   the result is M_n_iter.
 *      No restart, no stopping test: the problem is underdetermined, the result is defined by this iteration.  Every sum is one fmaf chain
 *      over ascending bins from zero; no atomics: a frame's result does not depend on its batch, its position or T.  One launch.
 *        mcvc_melinv_max_iter       the largest n_iter (512).
 *        mcvc_melinv_tables_floats  size of the constant operand.
 *        mcvc_melinv_tables_init    HOST -> HOST.  host_basis [80][513] and host_pinv [513][80] fp32; lambda as above.  The kernel uses the
 *                                   basis through sparse tables (per bin: first filter and two weights; per filter: first bin and count), so
 *                                   MCVC_ERR_INVALID for a basis with a column of more than two non-zeros, with two that are not in adjacent
 *                                   filters, with a filter whose non-zeros are not contiguous bins, or with a value that is not finite; also
 *                                   for a null pointer or a lambda that is not positive and finite.  A refused call writes nothing.  The
 *                                   caller uploads the result (16-byte aligned) once per device.
 *        mcvc_melinv_solve          asynchronous on `stream`; no device allocation, no workspace.  MCVC_ERR_INVALID: a null or misaligned
 *                                   pointer (logmel, mag_out: 4 bytes; tables: 16), B < 1, T < 1, B > 65535, T > 2^20, B T > 2^22, n_iter
 *                                   outside [0, 512] -- nothing is launched.                                                          */
int mcvc_melinv_max_iter(void);
long long mcvc_melinv_tables_floats(void);
int mcvc_melinv_tables_init(const float* host_basis, const float* host_pinv, double lambda, float* host_out);
int mcvc_melinv_solve(const float* logmel, const float* tables, float* mag_out, int B, int T, int n_iter, void* stream);

/* ---- objective evaluation (new): mel-cepstra from log-mels and batched dynamic time warping (csrc/dtw_kernels.hip; the definitions are in
 *      mask_cyclegan_vc/metrics.py and INTEGRATION.md).  A feature bank is [K][N] fp32, time-contiguous per row: utterances back to back
 *      along time with an offset table offs[n + 1]; pair p aligns utterance p of bank x with utterance p of bank y.
 *        mcvc_dtw_max_frames   the longest utterance a pair may hold (4096: the strip boundary row lives in 32 KB of LDS).
 *        mcvc_dtw_launches     kernel launches of one run: 1, or 2 with paths (the backtrack is its own launch).
 *        mcvc_cep_basis_init   HOST buffer [n_cep][80]: rows 1 .. n_cep of the orthonormal DCT-II over the 80 mel bins, computed in float64
 *                              and rounded once; 1 <= n_cep <= 79.  The caller uploads it (16-byte aligned) once per device.
 *        mcvc_cep_project      the launch: out [n_cep][n_frames] = basis @ (ln 10 * mel [80][n_frames]); DEVICE pointers.  MCVC_ERR_INVALID:
 *                              a null or misaligned pointer (mel, out: 4 bytes; basis: 16), n_frames < 1, n_cep outside 1 .. 79.
 *        mcvc_dtw_plan         HOST offset tables in; HOST table [n_pairs][6] int64 out (table == NULL: sizes only), plus the workspace bytes
 *                              of a run (0 without paths: no Tx x Ty matrix exists then) and the rows of the path buffer.  Row p of the table:
 *                              x offset, Tx, y offset, Ty, offset of the pair's direction bytes in the workspace, first row of its path
 *                              (capacity Tx + Ty - 1 rows; `length` of them are written); the last two are -1 without paths.
 *                              MCVC_ERR_INVALID: n_pairs < 1, a negative first offset, an utterance of fewer than 1 or more than
 *                              4096 frames (offsets that do not rise included).
 *        mcvc_dtw_run          all launches on `stream`; no device allocation.  x, y, table (the plan's, uploaded, 16-byte aligned), cost
 *                              [n_pairs] fp32, length [n_pairs] int32, path (nullable: no paths) [path rows][2] int32 and workspace (16-byte
 *                              aligned) are DEVICE pointers; x_offs / y_offs are the HOST tables the plan saw, validated again here.
 *                              d(i, j) = scale * sqrt(sum_k (x[k][i] - y[k][j])^2).  MCVC_ERR_INVALID: a null or misaligned pointer,
 *                              K outside 1 .. 80, n_pairs < 1, a NaN scale, tables the plan refuses or that reach beyond x_frames / y_frames;
 *                              MCVC_ERR_WORKSPACE: workspace null or too small -- nothing is launched.                                  */
int mcvc_dtw_max_frames(void);
int mcvc_dtw_launches(int want_path);
int mcvc_cep_basis_init(int n_cep, float* basis_host);
int mcvc_cep_project(const float* mel, long long n_frames, const float* basis, int n_cep, float* out, void* stream);
int mcvc_dtw_plan(const int* x_offs, const int* y_offs, int n_pairs, int want_path, long long* table, long long* workspace_bytes, long long* path_rows);
int mcvc_dtw_run(const float* x, long long x_frames, const float* y, long long y_frames, int K, float scale, const int* x_offs, const int* y_offs,
                 const long long* table, int n_pairs, float* cost, int* length, int* path, void* workspace, long long workspace_bytes, void* stream);

/* ---- pitch tracking (new): YIN F0 contours on the front-end's frame grid and F0 statistics along DTW paths (csrc/f0_kernels.hip; the
 *      definitions are in mask_cyclegan_vc/pitch.py and INTEGRATION.md).  22050 Hz, hop 256, integration window W = 1024.  Frame t of an
 *      utterance (frames and work list: mcvc_audio_plan) is centred on sample c_t = 256 t + 128, the centre of mel frame t's window, and
 *      reads buf[j] = x[c_t - (W + tau_max) / 2 + j], zero outside the utterance.  d(tau) = sum_{j < W} (buf[j] - buf[j + tau])^2, from
 *      differences; d'(0) = 1, d'(tau) = d(tau) tau / sum_{1 <= k <= tau} d(k), 1 where that sum is 0.  Pick: the first tau in tau_min ..
 *      tau_max with d'(tau) < threshold, then upward while d'(tau + 1) < d'(tau); with a, b, c = d'(tau - 1), d'(tau), d'(tau + 1):
 *      off = 0 at tau_max or where den = (a - b) + (c - b) <= 0, else clamp(0.5 (a - c) / den, -0.5, 0.5); f0 = 22050 / (tau + off),
 *      aperiodicity = b.  No lag under the threshold: f0 = 0 (unvoiced), aperiodicity = min d'.  Comparisons are strict, on the stored fp32 d'.
 *        mcvc_f0_max_lag    the largest tau_max (640: 34.5 Hz).
 *        mcvc_f0_launches   kernel launches of one mcvc_f0_track (1, with or without cmnd).
 *        mcvc_f0_track      one launch on `stream`; no device allocation.  wave, tiles (mcvc_audio_plan's, uploaded, 16-byte aligned), f0 and
 *                           aperiodicity fp32 [total_frames], cmnd (nullable) fp32 [tau_max + 1][total_frames] -- the d' the pick was made on --
 *                           are DEVICE pointers.  A work item that does not lie inside [0, n_samples) x [0, total_frames) is skipped, never
 *                           followed.  MCVC_ERR_INVALID, before any pointer is touched: a null or misaligned pointer, a lag range outside
 *                           2 <= tau_min < tau_max <= 640, a threshold that is not finite or not in (0, 1], n_tiles < 1, total_frames < 1,
 *                           n_samples < 385.
 *        mcvc_f0_stats      one launch, one wavefront per pair.  fx [x_frames], fy [y_frames] fp32 F0 banks (0 = unvoiced); path int32 [rows][2]
 *                           as mcvc_dtw_run wrote it (8-byte aligned); pairs int64 [n_pairs][4] (16-byte aligned): x frame offset, y frame
 *                           offset, first path row, path rows -- DEVICE pointers all.  counts int32 [n_pairs][4]: rows with both sides voiced,
 *                           x only, y only, neither; sums fp32 [n_pairs][2]: sum c and sum c^2 over the both-voiced rows, c = 1200 log2(fx / fy)
 *                           cents.  Lane l takes rows l, l + 64, ... in order, then a fixed butterfly; no atomics: a batch equals its single
 *                           calls bit for bit.  A path row that points outside the banks is skipped; the extent of `path` is the caller's
 *                           contract.  MCVC_ERR_INVALID: a null or misaligned pointer, x_frames / y_frames / n_pairs < 1.               */
int mcvc_f0_max_lag(void);
int mcvc_f0_launches(int want_cmnd);
int mcvc_f0_track(const float* wave, long long n_samples, const int* tiles, int n_tiles, int tau_min, int tau_max, float threshold, float* f0,
                  float* aperiodicity, float* cmnd, long long total_frames, void* stream);
int mcvc_f0_stats(const float* fx, long long x_frames, const float* fy, long long y_frames, const int* path, const long long* pairs, int n_pairs,
                  int* counts, float* sums, void* stream);

/* ---- non-parallel evaluation (new): modulation spectra, global variance and the distance between two SETS of utterances
 *      (csrc/ms_kernels.hip; mask_cyclegan_vc/metrics.py and INTEGRATION.md restate this).  cep is a cepstra bank [K][n_frames] fp32 with
 *      offsets offs[n_utts + 1], as mcvc_cep_project fills it; 1 <= K <= 80; utterance u has T frames, T <= n_fft; n_fft is 1024, 2048 or 4096.
 *      Per utterance and row k:  mean = (1/T) sum_t c[k][t];  x[t] = c[k][t] - mean;  var = (1/T) sum_t x[t]^2 (population variance, from the
 *      deviations);  X[f] = sum_{t < T} x[t] exp(-2 pi i f t / n_fft), f = 1 .. n_fft / 2 (rectangular window zero-padded to n_fft; bin 0 is
 *      dropped, the mean was removed);  P[u][k][f - 1] = |X[f]|^2 / T.  Bin f lies at f (22050 / 256) / n_fft Hz.
 *      Twiddles: a table of cos(2 pi j / n_fft), j < n_fft, float64 rounded once, read at the INTEGER phase (f t) mod n_fft (exact argument
 *      reduction; the phase is never formed in floating point); the sine is the same table a quarter turn on.
 *      Per set of n utterances, floor = 1e-10 by definition:  LMS[k][f] = (1/n) sum_u 10 log10(max(P[u][k][f], floor)) dB and
 *      LGV[k] = (1/n) sum_u 10 log10(max(var[u][k], floor)) dB, utterances summed in index order.  Between two sets, over the first F bins:
 *      msd_per_dim[k] = sqrt((1/F) sum_f (LMS_A - LMS_B)^2), msd = sqrt((1/(K F)) sum_{k,f} (..)^2), gvd = sqrt((1/K) sum_k (LGV_A - LGV_B)^2).
 *      No atomics, every reduction in a fixed order; an utterance's P, mean and var depend on that utterance alone: a ragged batch equals its
 *      single calls bit for bit.  All calls are asynchronous on `stream`, allocate nothing on the device and launch nothing when they refuse.
 *        mcvc_ms_max_fft      4096 (= mcvc_dtw_max_frames()): the largest n_fft and the longest utterance.
 *        mcvc_ms_launches     kernel launches of one MSD + GVD evaluation of two sets from their cepstra banks: 8 (2 x mcvc_ms_power,
 *                             4 x mcvc_ms_mean_log for P and var of both sets, 2 x mcvc_ms_distance).
 *        mcvc_ms_table_init   HOST buffer [n_fft]: cos(2 pi j / n_fft).  The caller uploads it (16-byte aligned) once per device and n_fft.
 *        mcvc_ms_power        one launch for the whole bank.  cep, offs_dev (int32 [n_utts + 1]), table, power [n_utts][K][n_fft / 2], mean and
 *                             var [n_utts][K] are DEVICE pointers; offs_host is the same offset table on the HOST, validated here.
 *                             MCVC_ERR_INVALID: a null or misaligned pointer (4 bytes; table: 16), K outside 1 .. 80, an n_fft other than
 *                             the three, n_utts < 1, offsets that do not rise from 0 to n_frames, an utterance longer than n_fft.
 *        mcvc_ms_mean_log     values [n][R] -> out [R] = (1/n) sum_u 10 log10(max(values[u][r], floor)).  MCVC_ERR_INVALID: a null or misaligned
 *                             pointer, n < 1, R < 1, a floor that is not positive and finite.
 *        mcvc_ms_distance     a, b [K][n_bins] -> per_dim [K], total [1] over the first n_used bins of every row; one workgroup, fixed-order
 *                             trees.  GVD is the call with the [K] tables as one row of K bins.  MCVC_ERR_INVALID: a null or misaligned
 *                             pointer, K outside 1 .. 80, n_bins outside 1 .. 2048, n_used outside 1 .. n_bins.                         */
int mcvc_ms_max_fft(void);
int mcvc_ms_launches(void);
int mcvc_ms_table_init(int n_fft, float* table_host);
int mcvc_ms_power(const float* cep, long long n_frames, int K, const int* offs_dev, int n_utts, const int* offs_host, int n_fft, const float* table,
                  float* power, float* mean, float* var, void* stream);
int mcvc_ms_mean_log(const float* values, int n, long long R, float floor, float* out, void* stream);
int mcvc_ms_distance(const float* a, const float* b, int K, int n_bins, int n_used, float* per_dim, float* total, void* stream);

/* ---- sample-rate conversion (new): scipy.signal.resample_poly's default filter on a bank of utterances (csrc/resample_kernels.hip;
 *      data_preprocessing/resample.py and INTEGRATION.md restate this).  For coprime up / down, m = max(up, down), half = 10 m:
 *      taps h[0 .. 2 half] = up * firwin(2 half + 1, 1 / m, window = ('kaiser', 5.0)) from the CALLER (float32), n_out = ceil(n_in up / down),
 *          y[k] = sum_i x[i] h[k down + half - i up]     over the i in [0, n_in) whose tap index lies in [0, 2 half],
 *      evaluated in polyphase form: c = k down + half, q = c div up, r = c mod up, y[k] = sum_{j < J} P[r][j] x[q - j] with
 *      P[r][j] = h[r + j up] (zero past the last tap), J = ceil((2 half + 1) / up), x zero outside ITS utterance; fp32 fused multiply-adds in
 *      the order j = 0 .. J - 1.  A bank is n utterances back to back in one fp32 buffer + int32 offsets [n + 1] (mcvc_audio_log_mel's layout);
 *      one (up, down) per launch.  No atomics, no workspace, no device allocation; an utterance's result does not depend on its neighbours.
 *        mcvc_resample_max_factor    640: the largest max(up, down).
 *        mcvc_resample_tile_samples  1024: the most output samples of one work-list row (one workgroup).
 *        mcvc_resample_out_samples   ceil(n_in up / down); 0 for n_in < 1 or a factor outside 1 .. 640.
 *        mcvc_resample_table_floats  size of the packed polyphase table: up rows of an odd pitch J | 1, rounded up to 4 floats; 0 when refused.
 *        mcvc_resample_pack          HOST -> HOST: table[r (J | 1) + j] = h[r + j up], zero elsewhere.  MCVC_ERR_INVALID: a null pointer,
 *                                    a refused ratio, n_taps != 20 max(up, down) + 1.  The caller uploads the table (16-byte aligned).
 *        mcvc_resample_plan          HOST tables in, HOST tables out: out_offs [n + 1] and the work list tiles [n_tiles][8] int32 = first
 *                                    sample of the utterance in the input bank, its length, first output sample of the row in the output bank,
 *                                    output samples of the row, q and r of the row's first output (computed in 64 bits), 0, 0.  A row holds at
 *                                    most mcvc_resample_tile_samples() outputs, fewer where their input span would not fit in LDS.
 *                                    tiles == NULL: only *n_tiles and out_offs are written.  MCVC_ERR_INVALID: a null pointer, n_utts < 1,
 *                                    offsets that are negative or do not rise (an empty utterance), up == down, gcd(up, down) != 1, a factor
 *                                    outside 1 .. 640, an output bank of 2^31 samples or more; MCVC_ERR_WORKSPACE: max_tiles too small.
 *        mcvc_resample_run           one asynchronous launch on `stream`.  x, table (16-byte aligned), y are DEVICE pointers.  tiles is the
 *                                    plan's table (16-byte aligned) in PINNED HOST memory (hipHostMalloc / hipHostRegister): every row is
 *                                    checked here, on the host, and the kernel reads the same rows through the buffer's device mapping, so
 *                                    the buffer stays alive and unchanged until the launch has finished.  MCVC_ERR_INVALID, and nothing is
 *                                    launched: a null or misaligned pointer, tiles in memory the device cannot read, a refused ratio, a row
 *                                    that reaches beyond [0, n_in_total) or [0, n_out_total), that holds no or too many samples, or whose
 *                                    (q, r) are out of range.                                                                             */
int mcvc_resample_max_factor(void);
int mcvc_resample_tile_samples(void);
long long mcvc_resample_out_samples(long long n_in, int up, int down);
long long mcvc_resample_table_floats(int up, int down);
int mcvc_resample_pack(const float* h_host, int n_taps, int up, int down, float* table_host);
int mcvc_resample_plan(const int* in_offs, int n_utts, int up, int down, int* out_offs, int* tiles, int max_tiles, int* n_tiles);
int mcvc_resample_run(const float* x, long long n_in_total, const int* tiles, int n_tiles, const float* table, int up, int down, float* y,
                      long long n_out_total, void* stream);

/* ---- silence detection (new): the frame energies librosa.effects.trim / split decide on, for a bank of utterances at 22050 Hz
 *      (csrc/vad_kernels.hip; data_preprocessing/silence.py and INTEGRATION.md restate this; restated from librosa's published definition and
 *      not verified against librosa).  Frame length 2048, hop 512, both fixed.  An utterance of L >= 1 samples has T = 1 + L / 512 frames;
 *      frame t covers samples [512 t - 1024, 512 t + 1024), zero outside [0, L) of ITS utterance;
 *          mse[t] = (1 / 2048) sum x^2   (fp32),        ref = max_t mse[t].
 *      Frame t is non-silent iff max(mse[t], 1e-10f) > max(ref, 1e-10f) * r with r = float32(10^(-top_db / 10)): the CALLER's decision, on
 *      the host, from the returned values (one fp32 product, one compare).  The kernel forms each 512-sample block's sum of squares once
 *      (lane l owns samples 512 j + l + 64 i, i = 0 .. 7 in order; a butterfly of fixed shape across the wave) and a frame as
 *      ((b0 + b1) + b2) + b3 of its four blocks, times 2^-11: one order per frame whatever shares the bank with it and wherever the
 *      utterance starts.  The maximum is an integer atomic max on the bit pattern of the non-negative energies (no order dependence).  No
 *      float atomic adds, no workspace, no device allocation.  A bank is n utterances back to back + int32 offsets [n + 1].
 *        mcvc_vad_frame_length       2048.
 *        mcvc_vad_hop                512.
 *        mcvc_vad_tile_frames        64: the most frames of one work-list row (one workgroup).
 *        mcvc_vad_launches           2: a memset node that zeroes ref, then the kernel, both on `stream`.
 *        mcvc_vad_frames             1 + n / 512; 0 for n < 1.
 *        mcvc_vad_plan               HOST tables in, HOST tables out: frame_offs [n + 1] and the work list tiles [n_tiles][4] int32 = first
 *                                    sample of the utterance in the bank, its length, the utterance's index, first frame of the row in the
 *                                    utterance.  tiles == NULL: only *n_tiles and frame_offs are written.  MCVC_ERR_INVALID: a null
 *                                    pointer, n_utts < 1, offsets that are negative or do not rise (an empty utterance);
 *                                    MCVC_ERR_WORKSPACE: max_tiles too small (*n_tiles still holds the count).
 *        mcvc_vad_energy             asynchronous on `stream`.  wave, tiles (16-byte aligned), frame_offs_dev, mse [total_frames] and
 *                                    ref [n_utts] are DEVICE pointers.  MCVC_ERR_INVALID, nothing launched: a null pointer, a count < 1, a
 *                                    bank or a frame count of 2^31 or more, a misaligned pointer.  A work-list row that does not describe
 *                                    this bank and these offsets makes its workgroup leave without reading or writing.
 *        mcvc_audio_plan_segments    mcvc_audio_plan for segments (first sample in the bank, length) that lie anywhere in the bank, in any
 *                                    order, overlapping or not: the same frame_offs [n + 1] and [n_tiles][4] work list for mcvc_audio_log_mel
 *                                    (each segment is reflect-padded at its own two ends), byte-identical to mcvc_audio_plan's tables for
 *                                    contiguous segments.  MCVC_ERR_INVALID: a null pointer, n_segs < 1, a negative start, a segment under
 *                                    385 samples, start + length > 2^31 - 1; MCVC_ERR_WORKSPACE: max_tiles too small.                      */
int mcvc_vad_frame_length(void);
int mcvc_vad_hop(void);
int mcvc_vad_tile_frames(void);
int mcvc_vad_launches(void);
long long mcvc_vad_frames(long long n);
int mcvc_vad_plan(const int* sample_offs, int n_utts, int* frame_offs, int* tiles, int max_tiles, int* n_tiles);
int mcvc_vad_energy(const float* wave, long long n_samples, const int* tiles, int n_tiles, const int* frame_offs_dev, int n_utts,
                    float* mse, long long total_frames, float* ref, void* stream);
int mcvc_audio_plan_segments(const int* starts, const int* lengths, int n_segs, int* frame_offs, int* tiles, int max_tiles, int* n_tiles);

/* ---- single-op entry points (kernel parity tests; same kernels the network calls use) ---------- */
/* y[N,Cout,OH,OW] = conv2d(x[N,Cin,H,W], w[Cout,Cin,KH,KW]) + bias ; stride 1 or 2.
 * wpack: scratch of mcvc_conv2d_pack_floats() floats, zero-initialised by the caller.
 * slabs: optional split-K scratch (max_slabs-1)*N*Cout*OH*OW floats; the reduced result is in y.     */
long long mcvc_conv2d_pack_floats(int Cout, int Cin, int KH, int KW);
int mcvc_conv2d_forward(const float* x, const float* w, const float* bias, float* y, float* wpack,
                        float* slabs, int max_slabs, int N, int Cin, int H, int W, int Cout, int KH, int KW,
                        int stride, int pad_h, int pad_w, int pixel_shuffle, void* stream);
/* dx[N,Cin,H,W] = conv2d_backward_data(dy[N,Cout,OH,OW], w) */
int mcvc_conv2d_dgrad(const float* dy, const float* w, float* dx, float* wpack, float* slabs, int max_slabs,
                      int N, int Cin, int H, int W, int Cout, int KH, int KW, int stride, int pad_h, int pad_w,
                      void* stream);
/* dw[Cout,Cin,KH,KW] += conv2d_backward_weight(x, dy).  slabs: K-split scratch of
 * mcvc_conv2d_wgrad_slab_floats() floats (may be NULL: no split)                                      */
long long mcvc_conv2d_wgrad_slab_floats(int N, int Cin, int H, int W, int Cout, int KH, int KW, int stride, int pad_h, int pad_w);
int mcvc_conv2d_wgrad(const float* x, const float* dy, float* dw, float* slabs, long long slab_floats, int N, int Cin, int H, int W,
                      int Cout, int KH, int KW, int stride, int pad_h, int pad_w, void* stream);
/* ---- one convolution LAYER of the path, op by op (r4).  SURVEY.md section 8(b) asks for single-op entries of the kernels that are hot at
 *      the trainer's shapes: the 5x5 layers run as Winograd products (model.py:86-103 downSample: F(2x2,3x3) / F(4x4,3x3) over the four input
 *      phases; :226-237 upSample: F(2x2,5x5) / F(4x4,5x5)) and the discriminators' stride-2 3x3 layers (:298-314) as implicit GEMMs.  These
 *      entries run the planner the networks use (conv_fwd / conv_dgrad / conv_wgrad) on ONE layer of `branches` (1, or 2 = value | gate)
 *      convolutions Cin -> Cout:  x [N][Cin][H][W], y / dy [N][branches*Cout][OH][OW] (value rows first), dx like x, dw like the OIHW
 *      parameters (ACCUMULATED: pass zeros).  `packed` = mcvc_layer_pack of the parameters (every weight set the planner may read);
 *      `scratch` >= mcvc_layer_scratch_floats.  `scheme`: 0 the planner's choice at this shape, 1 Winograd with 2x2 output tiles, 2 Winograd
 *      with 4x4 output tiles (sample / tile thresholds lifted; image sides must be multiples of 4 -- 8 for the stride-2 layers),
 *      3 no Winograd (direct kernels for these layers since r5), 4 direct kernels only, 5 implicit GEMM (forward / dgrad / wgrad of the 3x3
 *      stride-2 layers: the kernels the discriminator passes run, sgemm.h; the dense operand is converted to their layout first).  w0 / w1 = the OIHW tensors themselves (the
 *      pre-r5 staged data gradient multiplied them in place; unused now).  pixel_shuffle: the forward store of the up-sampling layers (model.py:232).
 *      Schemes 1 / 2 and the tile count (a Winograd pass keeps at most 16384 tiles in its workspaces): a batch with more 2x2 tiles runs as
 *      several passes over equal chunks of samples (3 samples of 5550 tiles: 2 + 1), weight gradients adding up over the chunks.  ONE sample of
 *      exactly 16384 tiles (a 256 x 256 image of a stride-1 layer) still runs Winograd; one with more (258 x 256: 16512 tiles) is not refused:
 *      the scheme is declined without an error and forward, data gradient and weight gradient run on the direct kernels, with the same
 *      results to rounding (tests/test_hip_wino_chunks.py tells the two apart by the launch trace).   */
long long mcvc_layer_packed_floats(int Cin, int Cout, int branches, int KH, int KW, int stride, int pad_h, int pad_w);
long long mcvc_layer_scratch_floats(int N, int H, int W, int Cin, int Cout, int branches, int KH, int KW, int stride, int pad_h, int pad_w);
int mcvc_layer_pack(const float* w0, const float* b0, const float* w1, const float* b1, float* packed, int Cin, int Cout, int branches,
                    int KH, int KW, int stride, int pad_h, int pad_w, void* stream);
int mcvc_layer_forward(const float* x, const float* packed, const float* w0, const float* w1, float* y, float* scratch,
                       long long scratch_floats, int N, int H, int W, int Cin, int Cout, int branches, int KH, int KW, int stride,
                       int pad_h, int pad_w, int scheme, int pixel_shuffle, void* stream);
int mcvc_layer_dgrad(const float* dy, const float* packed, const float* w0, const float* w1, float* dx, float* scratch,
                     long long scratch_floats, int N, int H, int W, int Cin, int Cout, int branches, int KH, int KW, int stride,
                     int pad_h, int pad_w, int scheme, void* stream);
int mcvc_layer_wgrad(const float* x, const float* dy, float* dw0, float* dw1, float* scratch, long long scratch_floats, int N, int H,
                     int W, int Cin, int Cout, int branches, int KH, int KW, int stride, int pad_h, int pad_w, int scheme, void* stream);
/*      ... with flags = MCVC_BWD_STORE_GRADS: the planner's store mode on this one layer (a layer mcvc_grad_store_mask covers: dw = the
 *      gradient, whatever dw held; any other layer: dw += as above).  flags = 0 is mcvc_layer_wgrad; other bits: MCVC_ERR_INVALID.       */
int mcvc_layer_wgrad_flags(const float* x, const float* dy, float* dw0, float* dw1, float* scratch, long long scratch_floats, int N, int H,
                           int W, int Cin, int Cout, int branches, int KH, int KW, int stride, int pad_h, int pad_w, int scheme, int flags,
                           void* stream);
/*      The fused backward of one 1-D trunk layer (SURVEY.md section 8b resblock1d_bwd / gemm1x1_in_bwd; reference model.py:47-76 under
 *      autograd): InstanceNorm (+ gated GLU when the gate pointers are given) backward of dy [Cout][B][T4] recomputed inside the
 *      transposed-convolution launch; dconv [Cx][B][T4] = gradient w.r.t. the conv output (Cx = Cout or 2*Cout, value rows first);
 *      dx [Cin][B][T4] += data gradient; d(gamma), d(beta) += (nullable); x_in != NULL (k = 3): dw / dw_gate += weight gradients.
 *      wpack: Cin * Cx * KW floats of workspace (the transposed weight copy).  Deterministic mode: the K slices of the data gradient run as
 *      launches one after the other, each adding to dx with plain stores (this entry has no slab workspace), instead of one launch with atomics. */
int mcvc_trunk_layer_backward(const float* dy, const float* conv_out, const float* stats, const float* gamma, const float* beta,
                              const float* gamma_gate, const float* beta_gate, const float* w, const float* w_gate, const float* x_in,
                              float* dx, float* dconv, float* dgamma, float* dbeta, float* dgamma_gate, float* dbeta_gate, float* dw,
                              float* dw_gate, float* wpack, int B, int Cin, int T4, int Cout, int KW, void* stream);

/* InstanceNorm(affine) + activation.  act: 0 none, 1 gated GLU (x has 2C channels: value|gate), 2 SiLU.
 * x[N,Cx,H,W] -> y[N,C,H,W]; stats[N,Cx,2] (mean, rstd)                                              */
int mcvc_instnorm_act_forward(float* x, const float* gamma, const float* beta, const float* gamma_gate,
                              const float* beta_gate, const float* residual, float* y, float* stats,
                              int N, int C, int H, int W, int act, void* stream);
int mcvc_instnorm_act_backward(const float* x, const float* gamma, const float* beta, const float* gamma_gate,
                               const float* beta_gate, const float* stats, float* dy, float* dx,
                               float* dgamma, float* dbeta, float* dgamma_gate, float* dbeta_gate,
                               int N, int C, int H, int W, int act, void* stream);

/* Fused 1-D trunk layer at small batch (B * T4 <= 32): ONE launch for Conv1d(k = 1 | 3, padding (k-1)/2) + bias + InstanceNorm1d(affine)
 * + {gated GLU when w_gate != NULL | residual add | nothing} -- the building block of ResidualLayer.forward (model.py:47-76:
 * value|gate pair, then the output conv with the skip connection) and of conv1dto2dLayer + its norm (model.py:266-267) -- SURVEY.md
 * section 8b's resblock1d / gemm1x1_in ops.  Trunk layout, channel-major with the batch inside: x [Cin][B][T4], w [Cout][Cin][KW] (the
 * nn.Conv1d tensor as is), conv_out [Cout (x2 with a gate)][B][T4] (pre-norm, kept for backward), stats [B][Cout (x2)][2] = (mean, rstd),
 * y / residual [Cout][B][T4].                                                                                         */
int mcvc_trunk_layer_forward(const float* x, const float* w, const float* bias, const float* gamma, const float* beta, const float* w_gate,
                             const float* bias_gate, const float* gamma_gate, const float* beta_gate, const float* residual, float* conv_out,
                             float* stats, float* y, int B, int Cin, int T4, int Cout, int KW, void* stream);

/* Batched fp32 GEMM of the Winograd convolution paths (the 36 / 16 per-point products of upSample1/2 and downSample1/2, forward,
 * data-gradient and weight-gradient: the kernel family with the largest share of a bs=1 step).  For x in [0, nbatch):
 *   C_x[m][n] = sum_k A_x[k][m] * B_x[k][n]     A_x = a + x*a_stride, K-major [K][lda]; B_x [K][ldb]; C_x [M][ldc].
 * M % 128 == 0, K % 16 == 0, lda / ldb % 4 == 0, ldb >= 64, N <= ldb.  Exact fp32 (v_mfma_f32_32x32x2_f32).            */
int mcvc_batched_gemm(const float* a, const float* b, float* c, int nbatch, int M, int N, int K, int lda, int ldb, int ldc,
                      long long a_stride, long long b_stride, long long c_stride, void* stream);

/* db[C] += sum over (n, h, w) of dy[N,C,P] */
int mcvc_bias_grad(const float* dy, float* db, int N, int C, int P, void* stream);
/* norm-less activations: act 1 gated GLU (x[N,2C,P] -> y[N,C,P]), 2 x*sigmoid(x), 3 sigmoid */
int mcvc_act_forward(float* x, float* y, int N, int C, int P, int act, void* stream);
int mcvc_act_backward(const float* x, float* dy, float* dx, int N, int C, int P, int act, void* stream);
/* xin[N,2,P] = (x*mask, mask)   (model.py:241) ; dx (=|+=) dxin[:,0]*mask */
int mcvc_fif_input(const float* x, const float* mask, float* xin, int N, int P, void* stream);
int mcvc_fif_input_grad(const float* dxin, const float* mask, float* dx, int N, int P, int accumulate, void* stream);

/* ---- opt-in measurement (bench.py `roofline`): HIP events around every kernel launch ----------- */
int mcvc_trace_enable(int on);
int mcvc_trace_kinds(void);
const char* mcvc_trace_kind_name(int kind);
/* out[kind][4] = {launches, total_ms, algorithmic_flops, algorithmic_bytes}; clears the log; syncs  */
int mcvc_trace_collect(double* out);
/* raw records in launch order: out[i][4] = {kind, ms, flops, bytes}; returns the record count           */
int mcvc_trace_collect_raw(double* out, int max_records);

#ifdef __cplusplus
}
#endif
#endif /* MCVC_H */
