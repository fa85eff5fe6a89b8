/* libfst_hip.so — C ABI of the MI355X (gfx950) train-step kernels for the feature-level
 * style-transfer TSC hot path.
 *
 * The reference (BaeHann/feature_level_style_transfer_for_TSC) has no FFI: its hot path is stock
 * PyTorch ops called from nn.Modules.  Each entry point below names the reference call site it
 * replaces (file:line, relative to the reference root).  The Python host side
 * (feature_level_style_transfer_for_tsc_amd/_lib.py) binds exactly these symbols with ctypes.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer unless the name ends in _host; the caller owns all memory;
 *     the library never allocates, frees or retains device memory;
 *   - activations are fp32, NCL, channel stride = L, explicit batch stride (so channel slices of a
 *     wider tensor can be passed without a copy);
 *   - launches are asynchronous on `stream` (a hipStream_t passed as void*); no implicit syncs;
 *   - return 0 on success, <0 for an argument error detected on the host before any launch,
 *     >0 = hipError_t; fst_last_error() returns a thread-local message.  No exceptions cross the ABI.
 */
#ifndef FST_HIP_H
#define FST_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FST_ABI_VERSION 28

int fst_version(void);
const char* fst_last_error(void);

/* ---------------------------------------------------------------------------------------------
 * Conv plan.  A "plan" is a small int32 device table describing how a (multi-tap, optionally
 * dilated, optionally two-input) 1-D convolution is cut into K-chunks and 32-row M-blocks for the
 * f32 MFMA implicit GEMM.  It is built on the host (plan.py) once per layer shape.
 *
 *   plan[0..15]  header: n_chunks, n_mgroups, MB (32-row blocks per M-group), ntaps, dil, pad_left,
 *                        chunk_cap (max padded channels per chunk, even), total_records,
 *                        n_items, items_per_wg, n_stages, 5 reserved (0)
 *   plan[16 + 4*q ...]                 chunk q:        src (0|1), c_begin, c_count, 0
 *   plan[16 + 4*n_chunks + 4*(g*n_chunks+q) ...]  (g,q): tap_lo, tap_hi, record_offset, stage_offset
 *   plan[16 + 4*n_chunks*(1+n_mgroups) + 4*i ...] item i (weight-gradient plans only):
 *                                                       g, q, row_block, 0      (q < 0: padding item)
 *
 * A "record" is MB*64 floats: for one (tap, channel pair) the MB A-operand registers of one
 * v_mfma_f32_32x32x2_f32 k-step (lane l ↔ row l&31 of the block, channel parity l>>5).
 * Every entry point takes the table twice: `plan_dev` (read by the kernels through scalar loads) and
 * `plan_host` + `plan_len` (the same ints in host memory, used to validate shapes and size the launch).
 * ------------------------------------------------------------------------------------------- */
#define FST_PLAN_HEADER 16

/* Weight source description for pack/unpack: element (m, c, tap) of input `s` lives at
 * w[s][off0 + m*sm + c*sc + tap*st].  Forward convs use (sm, sc, st) = (C*ntaps, ntaps, 1);
 * the data-gradient conv uses the transposed, tap-flipped view of the same tensor. */
typedef struct {
  const float* w;   /* device */
  int64_t off0, sm, sc, st;
} fst_wsrc;

/* Pack PyTorch-layout weights into the plan's record layout.  Replaces the implicit weight use in
 * F.conv1d at OS_CNN/OS_CNN.py:71, Simplified_NF_WaveGlow.py:36,41,103,107,112,116,123. */
int fst_pack_weights(const int32_t* plan_dev, const int32_t* plan_host, int plan_len,
                     const fst_wsrc* src0_host, const fst_wsrc* src1_host,
                     int M, int g_begin, int g_end /* M-group range, -1 = all */, int row_base /* view row = m - row_base */,
                     float* a_packed, void* stream);

/* Same as fst_pack_weights, into the split-bf16 image the FST_GEMM_BF16X3 path of fst_conv_gemm reads
 * (plan.n_stages * MB * 2048 bytes + a 16-byte zero block): every weight w is stored as two round-to-nearest bf16 parts,
 * hi = bf16(w) and lo = bf16(w - hi); stage s (= one live (M-group, chunk, tap) triple, 16 channels deep),
 * 32-row block mb: 64 lanes x 8 hi parts, then 64 lanes x 8 lo parts, lane l = row l&31, channels 8*(l>>5)+0..7
 * — the A-operand fragments of v_mfma_f32_32x32x16_bf16.  Only for plans made of single-tap stages of at
 * most 16 channels (the pipelined kernel's plans). */
int fst_pack_weights_bf16x3(const int32_t* plan_dev, const int32_t* plan_host, int plan_len,
                            const fst_wsrc* src0_host, const fst_wsrc* src1_host,
                            int M, int g_begin, int g_end, int row_base, void* a_image, void* stream);

/* Inverse of fst_pack_weights for weight gradients: scatter a packed gradient back to PyTorch
 * layout (dw0/dw1 must be zero-filled by the caller when the plan does not cover every tap). */
int fst_unpack_weights(const int32_t* plan_dev, const int32_t* plan_host, int plan_len,
                       const float* a_packed, int M,
                       float* dw0, int64_t off0_0, int64_t sm0, int64_t sc0, int64_t st0,
                       float* dw1, int64_t off0_1, int64_t sm1, int64_t sc1, int64_t st1,
                       int n_slabs /* a_packed = n_slabs partial sums of plan.packed_floats each, added here */,
                       void* stream);

/* Omni-scale re-masking W ← W ⊙ mask, mask given as per-output-channel live tap range.
 * Replaces OS_CNN/OS_CNN.py:68. */
int fst_mask_taps(float* w, const int32_t* live_lo, const int32_t* live_hi, int M, int C, int K, void* stream);

/* y[b,m,t] = bias[m] + Σ_k A[m,k]·xcol[b,k,t]  — the forward engine (f32 MFMA, LDS-staged input
 * window).  Rows m < msplit go to y (+res if given); rows ≥ m2_start go to y2[m − m2_start]
 * (accumulated if FST_EPI_ACC2).  Replaces F.conv1d/nn.Conv1d at OS_CNN/OS_CNN.py:71,164 and
 * Simplified_NF_WaveGlow.py:36,41,103,107,112,116,123; with transposed packing it is also the
 * data-gradient conv of every one of those.
 *   flags: FST_EPI_RELU, FST_EPI_ACC2, FST_EPI_ATOMIC (ksplit>1; y must be pre-initialised);
 *   FST_GEMM_BF16X3: a_packed is the image written by fst_pack_weights_bf16x3 and every product is formed as
 *   hi*hi + hi*lo + lo*hi on v_mfma_f32_32x32x16_bf16 with fp32 accumulation (both operands split into two
 *   round-to-nearest bf16 parts; relative error of a product <= 3*2^-18, measured 5e-6 of the output scale)
 *   — about 5x the f32 MFMA rate.  Needs a pipelined plan, L % 4 == 0 and 16-byte aligned activations. */
#define FST_EPI_RELU    1
#define FST_EPI_ACC2    2
#define FST_EPI_ATOMIC  4
#define FST_EPI_ACC1    8
#define FST_GEMM_BF16X3 16
#define FST_WGRAD_SLABS 32   /* fst_conv_wgrad: da_packed holds one partial-sum slab per K slice (no atomics, no zero fill) */
int fst_conv_gemm(const float* x0, int64_t x0_bs, const float* x1, int64_t x1_bs,
                  const float* a_packed, const int32_t* plan_dev, const int32_t* plan_host, int plan_len,
                  const float* bias,
                  float* y, int64_t y_bs, const float* res, int64_t res_bs,
                  float* y2, int64_t y2_bs, int msplit, int m2_start /* rows [msplit, m2_start) are padding */,
                  int B, int L, int M, int nb_cfg, int ksplit, int flags, void* stream);

/* dA_packed[(g,q) records] += Σ_{b,t} dy[b,m,t]·xcol[b,k,t]  — weight-gradient engine (f32 MFMA,
 * split over (b,t) with fp32 atomics; the caller zero-fills da_packed).  Replaces the weight
 * gradient autograd derives for every conv listed above (Q1: with a dense plan it also yields the
 * masked-tap gradients the reference's GradNorm consumes, train_and_test.py:685-690).
 * FST_GEMM_BF16X3: products on v_mfma_f32_32x32x16_bf16 with both operands split into two bf16 parts
 * (hi*hi + hi*lo + lo*hi, fp32 accumulate), same layout of da_packed.
 * FST_WGRAD_SLABS: instead of fp32 atomics into one zero-filled buffer (1.3 TB/s chip-wide: 50 MB of them per in_layer
 * launch), K slice s stores its partial sums plainly into da_packed + s·packed_floats (the buffer holds
 * min(ksplit, B·⌈L/32⌉) slabs, no zero fill); fst_unpack_weights(n_slabs) adds them.
 * x0_mul_off != 0 (single-input 1x1 plans only): the x operand is the elementwise product x0[i]·x0[i + x0_mul_off] formed
 * while staging — the res_skip weight gradient reads acts = t·s from the gate halves the fused forward saved
 * (x0 = the t rows of ts, offset n·L to the s rows), so acts itself is never written to HBM. */
int fst_conv_wgrad(const float* x0, int64_t x0_bs, const float* x1, int64_t x1_bs,
                   const float* dy, int64_t dy_bs, const float* dy2, int64_t dy2_bs, int msplit,
                   float* da_packed, const int32_t* plan_dev, const int32_t* plan_host, int plan_len,
                   int B, int L, int M, int ksplit, int flags /* 0 or FST_GEMM_BF16X3 */, int64_t x0_mul_off, void* stream);

/* The kernel instance the last fst_conv_gemm / fst_conv_wgrad call of the calling host thread launched, recorded from the
 * values the launcher dispatched with (host-side, thread-local; a call refused before its launch clears it):
 *   out[0]     family: FST_ROUTE_GEMM conv_gemm_kernel<MB,NB>, FST_ROUTE_PIPE conv_gemm_pipe_kernel<MB,NB,VEC>,
 *              FST_ROUTE_BF3 conv_gemm_bf3_kernel<MB,NB>, FST_ROUTE_WIN_BF3 conv_win_bf3_kernel<MB,NB>,
 *              FST_ROUTE_WIN_ROWS conv_win_rows_kernel (no template arguments),
 *              FST_ROUTE_WGRAD conv_wgrad_kernel<CB,TW,WIDE,VEC,BF3>
 *   out[1..5]  the template arguments in declaration order, unused ones 0 (bools as 0 / 1)
 *   out[6]     forward epilogue: FST_ROUTE_EPI_PLAIN, _ADD, _ATOMIC, _VEC (16-byte plain), _VEC_ADD; -1 for fst_conv_wgrad
 *   out[7]     ksplit of the launch after the library's clamp
 * Returns 0, or -1 when no launch is recorded (out zero-filled) or out is null. */
#define FST_ROUTE_GEMM      1
#define FST_ROUTE_PIPE      2
#define FST_ROUTE_BF3       3
#define FST_ROUTE_WIN_BF3   4
#define FST_ROUTE_WIN_ROWS  5
#define FST_ROUTE_WGRAD     6
#define FST_ROUTE_EPI_PLAIN   0
#define FST_ROUTE_EPI_ADD     1
#define FST_ROUTE_EPI_ATOMIC  2
#define FST_ROUTE_EPI_VEC     3
#define FST_ROUTE_EPI_VEC_ADD 4
int fst_conv_last_route(int32_t out[8]);

/* out[m] = Σ_{b,t} x[b,m,t]   (bias gradients): one workgroup per row, written (no zero fill, no atomics, fixed order). */
int fst_row_sum(const float* x, int64_t x_bs, int B, int C, int L, float* out, void* stream);

/* ---------------------------------------------------------------------------------------------
 * BatchNorm1d over (B, L), train and eval — replaces nn.BatchNorm1d at OS_CNN/OS_CNN.py:72,165
 * and the ReLU / residual add at :74, :179.
 * stats layout (float[4*C]): mean | invstd | scale | shift   (scale = γ·invstd, shift = β − mean·scale)
 * ------------------------------------------------------------------------------------------- */
/* `numel` (here and below): the element count of the contiguous [B, C, L] tensors the launch walks, taken by the caller
 * from the tensors it holds — NOT recomputed from B, C, L.  The launcher refuses B*C*L != numel before launching, so a
 * batch argument that does not describe the buffers (the cause of round 1's GPU memory fault: the all-rank batch
 * passed as the launch batch of fst_bn_bwd_apply) is an error return, never an out-of-bounds walk. */
/* Batch moments as partials: part[c][slot] = (count, k, Σ(x − k), Σ(x − k)²) of the samples workgroup `slot` of channel c
 * walked, shifted by k = y[0][c][0] — FST_BN_SLOTS slots per channel, every one written (no zero fill by the caller, no
 * atomics).  Never Σx² − (Σx)²/N of the raw values: a channel of the univariate extractor's 1x1 shortcut has |mean|/std in
 * the hundreds, where that form has no correct digit of the variance in fp32. */
#define FST_BN_SLOTS 16
int fst_bn_stats(const float* y, int B, int C, int L, float* part /* [C][FST_BN_SLOTS][4], written */, int64_t numel, void* stream);
/* Turns every slot into (count, mean, M2) and merges the n_slots of a channel in slot order with Chan's formula (double
 * precision) into the batch mean / biased variance, updates
 * the running statistics (unbiased variance) and writes stats.  n_slots = FST_BN_SLOTS, or ranks·FST_BN_SLOTS in global-batch
 * data parallelism (SyncBN) after the caller gathered every rank's partials as part[c][rank·FST_BN_SLOTS + slot].
 * train = 0: part may be NULL; stats from the running statistics. */
int fst_bn_finalize(const float* part, int n_slots, const float* gamma, const float* beta,
                    float* running_mean, float* running_var, int train, int C, float eps, float momentum,
                    float* stats, void* stream);
/* out = act(y*scale + shift (+ res*res_scale + res_shift | + res)) */
int fst_bn_apply(const float* y, const float* stats, const float* res, const float* res_stats,
                 float* out, int B, int C, int L, int relu, int64_t numel, void* stream);
/* The BatchNorm's value of an element in front of the ReLU is pre(y) = fma(y, scale, shift) — for the join,
 * pre(ya) + pre(yb) — and fst_bn_apply stores max(pre, 0).  The backward functions need the ReLU only as the mask [out > 0],
 * and take it either from `out` (when the caller kept it) or, with out = NULL, from the sign of pre recomputed from y and stats
 * by the very function the forward calls: the same bits, one tensor read less per pass.
 *
 * reductions for backward, as FST_BN_SLOTS partial sums per channel (written, no zero fill, no atomics):
 * red[0][c][slot] = Σ dyʹ, red[1][c][slot] = Σ dyʹ·x̂, with dyʹ = dy·[out>0] when relu (out may be NULL: dy·[pre(y)>0]) */
int fst_bn_bwd_reduce(const float* dy, const float* y, const float* out, const float* stats,
                      int B, int C, int L, int relu, float* red /* [2][C][FST_BN_SLOTS] */, int64_t numel, void* stream);
/* dx = scale·(dyʹ − r0/N − x̂·r1/N) in train mode, scale·dyʹ in eval mode; r = the n_slots partials of red added in slot order
 * (n_slots = FST_BN_SLOTS as fst_bn_bwd_reduce leaves them, or 1 when the caller has already added them, e.g. over ranks);
 * N = B_total·L.  B is the batch of the tensors (launch shape); B_total >= B the batch red was summed over (= B, or all
 * ranks' batches for SyncBN).  red_out (optional, [2C]): receives (r0 | r1) = (dβ | dγ).  row_sums (optional, [B][C]): receives
 * Σ_t dx[b][c][t] — summed over b, the bias gradient of the conv in front of the BatchNorm (OS_CNN.py:67-72: conv1d with bias →
 * BatchNorm1d), which then needs no pass of its own over dx.  out: as for fst_bn_bwd_reduce (NULL with relu: mask from y). */
int fst_bn_bwd_apply(const float* dy, const float* y, const float* out, const float* stats, const float* red, int n_slots,
                     float* red_out, float* dx, float* row_sums, int B, int C, int L, int relu, int train, int B_total,
                     int64_t numel, void* stream);
/* Backward of the residual join out = relu(pre_a(ya) + pre_b(yb)) (fst_bn_apply with res and res_stats): both branches share dy
 * and the mask [pre_a(ya) + pre_b(yb) > 0], so one reduce walks dy, ya, yb once and one apply walks them once more and writes
 * both dx — 8 tensor passes where two fst_bn_bwd_reduce / fst_bn_bwd_apply pairs take 14.  Every result (partials, red_out, dx,
 * row sums) has the bits the two single-branch pairs leave: same element arithmetic, same summation order per branch.
 * red_a, red_b: distinct [2][C][FST_BN_SLOTS] buffers, laid out as fst_bn_bwd_reduce's. */
int fst_bn_bwd_reduce_join(const float* dy, const float* ya, const float* yb, const float* stats_a, const float* stats_b,
                           int B, int C, int L, float* red_a, float* red_b, int64_t numel, void* stream);
/* n_slots, B_total, train, red_out_*, row_sums_*: as for fst_bn_bwd_apply, shared by the branches.  dxa or dxb may be NULL
 * (that branch needs no input gradient; its row_sums must be NULL too): its red_out is still written. */
int fst_bn_bwd_apply_join(const float* dy, const float* ya, const float* yb, const float* stats_a, const float* stats_b,
                          const float* red_a, const float* red_b, int n_slots, float* red_out_a, float* red_out_b,
                          float* dxa, float* dxb, float* row_sums_a, float* row_sums_b, int B, int C, int L, int train,
                          int B_total, int64_t numel, void* stream);

/* ---------------------------------------------------------------------------------------------
 * WaveGlow pieces — Simplified_NF_WaveGlow.py
 * ------------------------------------------------------------------------------------------- */
/* gate (:44-54): g[B,2n,L] → t=tanh(g[:n]), s=sigmoid(g[n:]) written back over g; acts=t·s */
int fst_gate_fwd(float* g_ts, float* acts, int B, int n, int L, int64_t numel_acts, void* stream);
/* dg[:n] = dacts·s·(1−t²), dg[n:] = dacts·t·s·(1−s) */
int fst_gate_bwd(const float* ts, const float* dacts, float* dg, int B, int n, int L, int64_t numel_acts, void* stream);
/* affine coupling (:173-178): xn[:, :h]=u[:, :h]; xn[:, h:] = exp(o[:, h:])·u[:, h:] + o[:, :h].
 * sums (optional float[fst_coupling_sum_slots(B, h, L)][2], written): per-workgroup partials (Σ log_s, Σ xn²) — the
 * full-tensor reductions of WaveGlowLoss (Simplified_NF_WaveGlow.py:230-241) taken in the same pass; the caller adds the slots. */
int64_t fst_coupling_sum_slots(int B, int h, int L);
int fst_coupling_fwd(const float* u, const float* o, float* xn, int B, int h, int L, int64_t numel, float* sums, void* stream);
/* backward of the above given dxn (may be NULL = 0) and (added) d_logs; g_ls / g_sq (each optional, DEVICE scalars) = the
 * cotangents of the two sums: dxn_eff = dxn + 2·g_sq·xn, d log_s += g_ls; writes du (full 2h channels) and do */
int fst_coupling_bwd(const float* u, const float* o, const float* dxn, const float* dlogs, const float* g_ls, const float* g_sq,
                     float* du, float* d_o, int B, int h, int L, int64_t numel, void* stream);
/* inverse coupling (:193-196): xn[:, h:] = (x[:, h:] − o[:, :h]) / exp(o[:, h:]) */
int fst_coupling_inv_fwd(const float* x, const float* o, float* xn, int B, int h, int L, int64_t numel, void* stream);
int fst_coupling_inv_bwd(const float* xn, const float* o, const float* dxn,
                         float* dx, float* d_o, int B, int h, int L, int64_t numel, void* stream);

/* Weight-norm fold of every conv of one WN into the flat weight tensor the fused kernels read (and its backward), ONE launch per
 * direction (Simplified_NF_WaveGlow.py:69-99: old-style weight_norm, w = g·v/‖v‖ per output channel, 18 convs per WN).
 * table (DEVICE, n_rows x 6 int64): per row = one output channel of one conv, or one plain-copy segment (biases, the end conv):
 *   { address of the row of v, address of the row's g scalar (0 = plain copy), element offset into flat, row length,
 *     element offset of the row's v gradient in dpar, element offset of its g gradient in dpar }
 * forward: flat[dst + j] = v[j]·g/‖v‖ (norms[r] = ‖v‖ kept for the backward);  backward: dv = (g/‖v‖)(dw − v (dw·v)/‖v‖²),
 * dg = (dw·v)/‖v‖ written into the gradient buffer dpar (the caller hands out its segments as the parameters' gradients).
 * ‖v‖² is summed in fp32.  Where it underflows to 0 or overflows to inf the forward gives what fp32 torch._weight_norm gives on
 * the CPU (w = ±inf resp. ±0) and so does dg; dv is the formula above evaluated in fp32 as written — all ±inf for ‖v‖ = 0, where
 * torch's autograd, which groups the same terms differently, gives NaN in some elements, and ±0 for ‖v‖ = inf as torch does.  A row
 * needs |v| below 1e-19 or above 1e19 throughout to get there, and either result is already unusable: nothing to train on. */
int fst_wn_fold_fwd(const int64_t* table_dev, int n_rows, float* flat, float* norms /* [n_rows] */, void* stream);
int fst_wn_fold_bwd(const int64_t* table_dev, int n_rows, const float* d_flat, const float* norms, float* dpar, void* stream);

/* log|det W| of the invertible 1x1 conv's [n][n] weight (Simplified_NF_WaveGlow.py:40, torch.logdet) and W^{-T}, the gradient
 * d log|det W| / dW its backward needs, in ONE single-workgroup launch (in-place Gauss-Jordan with partial pivoting in double
 * precision in LDS) instead of an LU factorisation, two triangular solves and ~30 tiny launches.  out[0] = log|det W| with
 * torch.logdet's conventions (NaN for a negative determinant, -inf for a singular matrix), out[1] = sign(det);
 * inv_t [n][n] = (W^{-1})^T (NaN-filled when singular; a zero entry is always +0, so W^{-T} of a permutation matrix is that matrix
 * bit for bit).  n <= 96. */
int fst_logdet_inv(const float* W, int n, float* out /* [2] */, float* inv_t /* [n][n] */, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Fused WN layer (Simplified_NF_WaveGlow.py:101-123 with the gate of :44-54): ONE launch per layer
 *   g = in_layer(a) + cond_layer(u0)[2n·i : 2n·(i+1)]  →  t = tanh(g[:n]), s = sigmoid(g[n:]), acts = t·s
 *   r = res_skip_layer(acts);  a_next = a + r[:n];  out (+)= r[n:]        (last layer: r has n rows, out += r)
 * on the split-bf16 matrix cores; the [B, 2n, L] pre-activation stays in registers.  Needs n < 128 (one spare K row
 * carries the biases through the GEMMs), L % 4 == 0 and 16-byte aligned tensors.
 *   fst_wn_image_bytes(n, h)   size of one layer's packed weight image
 *   fst_wn_pack                effective (weight-norm folded) weights of one layer → image.  in_w [2n][n][3],
 *                              cond_w [2n][h] (this layer's rows of cond_layer), in_b / cond_b [2n],
 *                              rs_w [2n][n] and rs_b [2n]  (last layer: [n][n], [n])
 *   fst_wn_layer_fwd           a [B][n][L] (batch stride a_bs), u0 [B][h][L] (batch stride u0_bs: a channel slice of a wider
 *                              tensor passes without a copy), ts [B][2n][L] ← (t | s) kept for backward, acts [B][n][L] or NULL,
 *                              a_next [B][n][L] (NULL iff last), out [B][n][L] (written if first, else accumulated);
 *                              numel_a = element count of the [B][n][L] tensors as the caller holds them.
 * ------------------------------------------------------------------------------------------- */
int64_t fst_wn_image_bytes(int n, int h);
int fst_wn_pack(const float* in_w, const float* cond_w, const float* in_b, const float* cond_b,
                const float* rs_w, const float* rs_b, int n, int h, int ntaps /* of in_w; the fused kernels are 3-tap: anything
                else is refused (Simplified_NF_WaveGlow.py:60 allows any kernel_size; the host side then takes the generic
                conv-engine path) */, int last, void* image, int64_t image_bytes, void* stream);
/* Every layer of a WN stack in ONE launch each (ABI v17): HOST tables of nl <= 10 per-layer pointers (copied into the kernel
 * arguments), layer nl - 1 being the `last` one; images[i] receives byte for byte what the per-layer call writes.
 * image_bytes: the size of one image (fst_wn_pack_bwd_stack: of a layer below the top one; the top layer's is
 * fst_wn_bwd_image_bytes(n, 1)). */
int fst_wn_pack_stack(const float* const* in_w, const float* const* cond_w, const float* const* in_b, const float* const* cond_b,
                      const float* const* rs_w, const float* const* rs_b, int nl, int n, int h, int ntaps, void* const* images,
                      int64_t image_bytes, void* stream);
int fst_wn_pack_bwd_stack(const float* const* rs_w, int nl, int n, int acc_order, void* const* images, int64_t image_bytes,
                          void* stream);
int fst_wn_pack_dgrad_stack(const float* const* in_w, const float* const* cond_w, int nl, int n, int h, int ntaps,
                            void* const* images, int64_t image_bytes, void* stream);
/* The images of fst_wn_stack_bwd_proj (ABI v19), one launch per stack: per layer [d_a stages as fst_wn_pack_bwd with acc_order = 1]
 * [skip stages: F_iᵀ, F_i = W_end·W_skip,i ([h2][n]), ceil(h2/16) of them] (the top layer: skip stages only), then 16 B of zeros.
 * end_w [h2][n] is the end conv's weight, h2 <= 64.  Every F_i element is one fp32 fmaf chain over the n products in index order,
 * then the hi/lo split: no atomics, two runs give the same bytes.  image_bytes: that of a layer below the top one. */
int64_t fst_wn_bwd_proj_image_bytes(int n, int h2, int last);
int fst_wn_pack_bwd_proj_stack(const float* const* rs_w, const float* end_w, int nl, int n, int h2, void* const* images,
                               int64_t image_bytes, void* stream);
int fst_wn_layer_fwd(const float* a, int64_t a_bs, const float* u0, int64_t u0_bs, const void* image, int64_t image_bytes,
                     float* ts, float* acts, float* a_next, float* out, int first, int last,
                     int B, int L, int n, int h, int dil, int64_t numel_a, void* stream);

/* Backward of the same layer through res_skip and the gate, ONE launch:
 *   dacts = W_rsᵀ·[d_a_next ; d_out]   (last layer: W_rsᵀ·d_out),   dg[:n] = dacts·s·(1−t²),  dg[n:] = dacts·t·s·(1−s)
 * (the transposed 1x1 conv autograd derives for Simplified_NF_WaveGlow.py:116 and the gate backward of :44-54).
 * ts = the (t | s) tensor fst_wn_layer_fwd saved; dg [B][2n][L] feeds the in_layer data / weight gradients. */
int64_t fst_wn_bwd_image_bytes(int n, int last);
int fst_wn_pack_bwd(const float* rs_w, int n, int last,
                    int acc_order /* 0: the image fst_wn_layer_bwd reads; 1: the d_a stages in the k-order in which a 32x32 accumulator
                                     tile delivers its rows as a B operand — the image fst_wn_stack_bwd reads (ABI v10) */,
                    void* image, int64_t image_bytes, void* stream);
int fst_wn_layer_bwd(const float* d_a_next /* NULL iff last */, const float* d_out, const float* ts, const void* image,
                     int64_t image_bytes, float* dg,
                     float* row_sums /* optional [256][B·⌈L/128⌉]: per-workgroup Σ_t dg[row]; the caller adds each row's
                                        entries: the in_layer / cond_layer bias gradient without a pass over dg */,
                     int64_t row_sums_rows, int last, int B, int L, int n, int64_t numel_a, void* stream);

/* Data gradient of the same layer's in_layer + cond_layer in ONE launch (the transposed dilated conv and the transposed
 * 1x1 autograd derives for Simplified_NF_WaveGlow.py:107-112):
 *   d_a_new = d_a + Σ_τ W_in[:, :, τ]ᵀ · dg[t + (1 − τ)·dil]      (d_a NULL: no residual cotangent — the last layer)
 *   d_u0   += W_condᵀ · dg
 * in_w [2n][n][3], cond_w [2n][h] (this layer's rows); dg [B][2n][L]; d_a / d_a_new [B][n][L]; d_u0 [B][h][L] with batch stride
 * d_u0_bs (the first h channels of the coupling layer's full-width input gradient are accumulated into in place). */
int64_t fst_wn_dgrad_image_bytes(int n);
int fst_wn_pack_dgrad(const float* in_w, const float* cond_w, int n, int h, int ntaps /* must be 3 */, void* image,
                      int64_t image_bytes, void* stream);
/* 1 when fst_wn_layer_dgrad serves (n, h, dil) — n <= 128, h <= 32 and two window slots of 512 + 2·dil samples fit the 160 KiB
 * of LDS (dil <= 128: WN stacks of up to 8 layers) — else 0: the caller then uses fst_conv_gemm's data-gradient plan. */
int fst_wn_dgrad_fits(int n, int h, int dil);
int fst_wn_layer_dgrad(const float* dg, const void* image, int64_t image_bytes, const float* d_a, float* d_a_new, float* d_u0,
                       float* row_sums /* optional [128][B·⌈L/512⌉]: per-workgroup Σ_t d_a_new[row] */, int64_t row_sums_rows,
                       int B, int L, int n, int h, int dil, int64_t numel_a, int64_t d_u0_bs, void* stream);

/* The forward of a WHOLE WN stack (every layer of fst_wn_layer_fwd) as ONE persistent launch: one workgroup walks all 256-sample
 * tiles of its batch elements through all layers — a_next / out of one layer are read by the next through the same CU — so no launch
 * boundary synchronises the chip and every other workgroup starts half a tile late: one half of the CUs stores while the other
 * multiplies (the per-layer launches alternate between an idle and a saturated memory system).  Same arithmetic, same results as the
 * per-layer launches.  Tables of nl entries (host memory, copied into the kernel arguments): a_in[i] = input of layer i with batch
 * stride a_bs[i] (a_in[0] = the start conv's output, a_in[i+1] = a_next[i]), images[i] = fst_wn_pack image, ts[i] [B][2n][L] written,
 * a_next[i] [B][n][L] written (NULL on the last layer); out [B][n][L] the skip sum (written).  fst_wn_stack_fwd_ok: n < 128,
 * L % 256 == 0, nl <= 10.  Replaces the layer loop of WN.forward, /root/reference/Simplified_NF_WaveGlow.py:101-123. */
int fst_wn_stack_fwd_ok(int n, int h, int L, int nl);
int fst_wn_stack_fwd(const float* const* a_in, const int64_t* a_bs, const void* const* images, int64_t image_bytes, float* const* ts,
                     float* const* a_next, const float* u0, int64_t u0_bs, float* out, int nl, int B, int L, int n, int h,
                     int64_t numel_a, void* stream);

/* The same two forwards for a pass that no backward follows (ABI v20) — the sampling / transfer direction WaveGlow.infer
 * (Simplified_NF_WaveGlow.py:181-203), the feature dump of train_and_test.py:792-797, any forward under no_grad: the gate halves
 * (t | s) and acts are not stored — half of a layer's store bytes, and the only tensors a pass keeps per layer.  Everything else of
 * the tile body is the saving kernels', in the same order: a_next and out are bit for bit what fst_wn_layer_fwd / fst_wn_stack_fwd
 * write (wn_layer_infer_kernel<NW>, wn_stack_infer_kernel: the same tile body with the stores compiled out).
 *   fst_wn_layer_infer   the arguments, checks and tile-size choice of fst_wn_layer_fwd without ts and acts; a_next == a is
 *                        refused (a tile's neighbours read a's halo while the tile stores a_next).
 *   fst_wn_stack_infer   the tables of fst_wn_stack_fwd without ts, same shape rule (fst_wn_stack_fwd_ok).  a_in[i+1] == a_next[i]
 *                        as there; a_next[i] == a_in[i] is refused; a_next[i] == a_in[i-1] is allowed — two buffers in
 *                        alternation serve a stack of any depth (one workgroup walks every tile of a layer of its batch element
 *                        before the next layer starts, and launches are stream-ordered). */
int fst_wn_layer_infer(const float* a, int64_t a_bs, const float* u0, int64_t u0_bs, const void* image, int64_t image_bytes,
                       float* a_next, float* out, int first, int last, int B, int L, int n, int h, int dil, int64_t numel_a,
                       void* stream);
int fst_wn_stack_infer(const float* const* a_in, const int64_t* a_bs, const void* const* images, int64_t image_bytes,
                       float* const* a_next, const float* u0, int64_t u0_bs, float* out, int nl, int B, int L, int n, int h,
                       int64_t numel_a, void* stream);

/* The whole backward of a WN stack — fst_wn_layer_bwd and fst_wn_layer_dgrad of every layer, top layer first — as ONE persistent
 * launch (the backward autograd derives for the loop of Simplified_NF_WaveGlow.py:104-121), for sequences of up to 512 samples:
 * a 512-sample tile is then a whole sequence, the dilated taps never leave it, and one workgroup walks all layers of its batch
 * element with the cotangent of the residual stream (d_a) kept in its accumulators from layer to layer; what a phase writes
 * (dg, d_u0) the next reads back from L2 / the Infinity Cache, and the CUs are not held in step by launch boundaries.
 * All tables are HOST arrays of nl entries (layer 0 = dilation 1 first; layer i has dilation 2^i):
 *   ts[i] the saved gate halves; img_b[i] the fst_wn_pack_bwd image with acc_order = 1; img_d[i] the fst_wn_pack_dgrad image;
 *   dg[i] [B][2n][L] written (entries may alias each other when nothing reads dg afterwards); da_out[i] [B][n][L] the cotangent
 *   of layer i's input, written when not NULL (da_out[0], the start conv's cotangent, is required; the others are the d_a
 *   operands of the res_skip weight gradients: da_out[i+1] is the residual cotangent entering layer i); rs_b[i] / rs_d[i]
 *   optional [256][B] / [128][B] per-sequence row sums of dg / da_out (both tables or neither).
 * d_u0 [B][h][L] (batch stride d_u0_bs) is accumulated into in place.  fst_wn_stack_bwd_ok: 1 when (n, h, L, nl) is served. */
int fst_wn_stack_bwd_ok(int n, int h, int L, int nl);
int fst_wn_stack_bwd(const float* const* ts, const void* const* img_b, const void* const* img_d, float* const* dg,
                     float* const* da_out, float* const* rs_b /* optional */, float* const* rs_d /* optional */,
                     const float* d_out, float* d_u0, int64_t d_u0_bs, int nl, int B, int L, int n, int h, int64_t numel_a,
                     void* stream);
/* The same launch fed with the end conv's cotangent d_o [B][h2][L] (h2 = 2h <= 64; numel_o its element count) in place of
 * d_out = W_endᵀ·d_o: by associativity W_skip,iᵀ·d_out = (W_end·W_skip,i)ᵀ·d_o, and img_b[i] (fst_wn_pack_bwd_proj_stack) holds that
 * product, so the skip operand has h2 rows and ceil(h2/16) stages instead of n and ceil(n/16).  Everything else as above. */
int fst_wn_stack_bwd_proj(const float* const* ts, const void* const* img_b, const void* const* img_d, float* const* dg,
                          float* const* da_out, float* const* rs_b /* optional */, float* const* rs_d /* optional */,
                          const float* d_o, int h2, int64_t numel_o, float* d_u0, int64_t d_u0_bs, int nl, int B, int L, int n,
                          int h, int64_t numel_a, void* stream);

/* Weight gradients of the same layer (the gradients autograd derives for Simplified_NF_WaveGlow.py:107-116), time as the MFMA
 * reduction index, split-bf16 products, per-workgroup partial slabs added in a fixed order (deterministic, no atomics):
 *   fst_wn_wgrad_in   dw_in[m][c][τ] = Σ_{b,t} dg[b,m,t]·a[b,c,t+(τ−1)·dil]   ([2n][n][3]),   dw_cond[m][c] = Σ dg[b,m,t]·u0[b,c,t]  ([2n][h])
 *   fst_wn_wgrad_rs   dw_rs[m][c] = Σ_{b,t} [d_a ; d_out][b,m,t]·(t·s)[b,c,t]  ([2n][n]; last layer: d_a NULL, [n][n]) — acts = t·s is
 *                     re-formed from the gate halves ts [B][2n][L] the fused forward saved
 * kind 0 = in_layer + cond_layer, 1 = res_skip.  fst_wn_wgrad_ok: 1 when the shape is served (L % 32 == 0, n < 128, h <= 32 and for
 * kind 0 dil % 4 == 0); 2 (kind 0, dil < 4) when it is served provided the caller guarantees 16 readable bytes in front of and
 * behind `a` (a_slack: the 16-byte pieces of a shifted tap start up to 3 samples outside a row); 0: the caller uses fst_conv_wgrad.
 * Operand SETS: the applications of one WN in a train step (forward on the target batch, forward on the source batch, inverse)
 * share their weights, so their gradients are summed; dg/a/u0 (d_a/d_out/ts) are HOST arrays of n_sets (1..3) device pointers to
 * same-shaped operands and one launch sums over all of them — the partial slabs and their reduction, which cost as much as the
 * products of one set, are paid once instead of n_sets times.
 * workspace: fst_wn_wgrad_workspace_floats(...) floats, written (independent of n_sets). */
int fst_wn_wgrad_ok(int kind, int B, int L, int n, int h, int dil);
int64_t fst_wn_wgrad_workspace_floats(int kind, int B, int L, int n, int h, int last);
int fst_wn_wgrad_in(const float* const* dg, const float* const* a, const float* const* u0, int n_sets, int64_t u0_bs, float* dw_in,
                    float* dw_cond, float* workspace, int64_t workspace_floats, int B, int L, int n, int h, int dil, int a_slack,
                    int64_t numel_a, void* stream);
int fst_wn_wgrad_rs(const float* const* d_a /* NULL iff last */, const float* const* d_out, const float* const* ts, int n_sets,
                    float* dw_rs, float* workspace, int64_t workspace_floats, int last, int B, int L, int n, int64_t numel_a,
                    void* stream);
/* The same products WITHOUT their reduction (ABI v17): the per-workgroup slabs stay in `workspace`, which must then live until
 * fst_wn_wgrad_reduce_many has added them.  That call reduces the slab sets of 1..16 such calls — the layers of one WN, which
 * share B, L, n, h — in one launch and writes the gradients with the bits fst_wn_wgrad_in / _rs write (every element adds its
 * slabs in the same order).  HOST tables of n_entries values: kind[j] (0 | 1), last[j] (kind 1: the top layer), n_sets[j] (as the
 * product was launched: the slab count depends on it), workspace[j] / workspace_floats[j], dw0[j] = dw_in | dw_rs,
 * dw1[j] = dw_cond (kind 0; ignored for kind 1).  Every argument is checked before the launch: a refused call writes nothing. */
int fst_wn_wgrad_in_slabs(const float* const* dg, const float* const* a, const float* const* u0, int n_sets, int64_t u0_bs,
                          float* workspace, int64_t workspace_floats, int B, int L, int n, int h, int dil, int a_slack,
                          int64_t numel_a, void* stream);
int fst_wn_wgrad_rs_slabs(const float* const* d_a /* NULL iff last */, const float* const* d_out, const float* const* ts, int n_sets,
                          float* workspace, int64_t workspace_floats, int last, int B, int L, int n, int64_t numel_a, void* stream);
int fst_wn_wgrad_reduce_many(const int32_t* kind, const int32_t* last, const int32_t* n_sets, float* const* workspace,
                             const int64_t* workspace_floats, float* const* dw0, float* const* dw1, int n_entries, int B, int L,
                             int n, int h, void* stream);

/* C[m][n] = Σ_k A[m][k]·Bm[n][k]  (A [M][K], Bm [N][K] row-major, the reduction index contiguous in both; M <= 256, K % 32 == 0) on the
 * time-as-k kernel above: RandomLayer's feature-side product x·R₀ (/root/reference/C_DAN.py:21; Bm = R₀ᵀ kept contiguous) and its data
 * gradient dy·R₀ᵀ (Bm = R₀).  The K split leaves partial slabs in `workspace` (fst_nt_gemm_workspace_floats), added in a fixed order.
 * Optional epilogue = the rest of RandomLayer.forward (C_DAN.py:22-25): C[m][n] = acc·epi_scale·Σ_c epi_p[m][c]·epi_r1[c][n] with the
 * plain product acc stored in epi_raw (may be NULL); epi_p = epi_r1 = NULL: C = acc. */
int64_t fst_nt_gemm_workspace_floats(int M, int N, int K);
int fst_nt_gemm(const float* A, const float* Bm, float* C, float* workspace, int64_t workspace_floats, int M, int N, int K,
                const float* epi_p /* [M][ncls] */, const float* epi_r1 /* [ncls][N] */, int epi_ncls, float epi_scale,
                float* epi_raw /* [M][N] */, void* stream);

/* dW[m][c][τ] = Σ_{b,t} dy[b][m][t]·x[b][c][t + τ·dil − pad_left]: the dense weight gradient of a conv with at most four taps on the
 * time-as-k kernel (each tap = one k-row segment with its own shift) — the Q1 gradient of the shared omni-scale block's last layer
 * (/root/reference/OS_CNN/OS_CNN.py:67-71, 225 → 50 channels, two taps; train_and_test.py:685-690 reads it).  fst_tap_wgrad_ok: 1 served,
 * 2 served provided 16 bytes either side of x are readable (x_slack: a tap shift that is not a multiple of 4 samples, within ±3),
 * 0 not served (M > 256, L % 32 != 0, more than 4 taps, larger misaligned shifts): the caller uses fst_conv_wgrad. */
int fst_tap_wgrad_ok(int B, int L, int M, int C, int ntaps, int dil, int pad_left);
int64_t fst_tap_wgrad_workspace_floats(int B, int L, int M, int C, int ntaps);
int fst_tap_wgrad(const float* dy, const float* x, float* dw /* [M][C][ntaps], written */, float* workspace, int64_t workspace_floats,
                  int B, int L, int M, int C, int ntaps, int dil, int pad_left, int x_slack, int64_t numel_dy, int64_t numel_x,
                  void* stream);

/* The DENSE weight gradient of an omni-scale layer (every tap k < K <= 96 of every row, dilation 1; quirk Q1: the reference convolves the
 * dense Kmax kernel, /root/reference/OS_CNN/OS_CNN.py:67-71, and GradNorm's norms, train_and_test.py:685-690, run over the dense gradient):
 *   dw[m][c][k] = Σ_{b,t} dy[b][m][t]·x[b][c][t + k − pad_left]          (M <= 256, L % 32 == 0)
 * time as the MFMA reduction index; the K k-rows of a channel are read from eight pre-shifted bf16 copies of ONE staged window of the
 * channel (csrc/wn_wgrad.hip).  Partial slabs in `workspace` (fst_dense_tap_wgrad_workspace_floats), added in a fixed order: no atomics. */
int fst_dense_tap_wgrad_ok(int B, int L, int M, int C, int K, int pad_left);
int64_t fst_dense_tap_wgrad_workspace_floats(int B, int L, int M, int C, int K);
int fst_dense_tap_wgrad(const float* dy, const float* x, float* dw /* [M][C][K], written */, float* workspace, int64_t workspace_floats,
                        int B, int L, int M, int C, int K, int pad_left, int64_t numel_dy, int64_t numel_x, void* stream);

/* The kernel instance the last call of the calling host thread to one of the launchers above launched — fst_wn_wgrad_in / _rs,
 * fst_nt_gemm, fst_tap_wgrad, fst_dense_tap_wgrad, fst_wn_layer_fwd / _infer / _bwd / _dgrad, fst_wn_stack_fwd / _infer / _bwd — recorded from the
 * values the launcher dispatched with (host side, thread-local; a call refused before its launch clears it):
 *   out[0]     family: FST_WN_ROUTE_WGRAD wn_wgrad_kernel<2, KT, FULL, MUL, NE>, FST_WN_ROUTE_TZ tz_wgrad_kernel<MP, FULL>,
 *              FST_WN_ROUTE_LAYER_FWD wn_layer_fwd_kernel<NW>, FST_WN_ROUTE_STACK_FWD wn_stack_fwd_kernel (8-wave tiles),
 *              FST_WN_ROUTE_LAYER_BWD, FST_WN_ROUTE_LAYER_DGRAD, FST_WN_ROUTE_STACK_BWD (no template arguments),
 *              FST_WN_ROUTE_LAYER_INFER wn_layer_infer_kernel<NW>, FST_WN_ROUTE_STACK_INFER wn_stack_infer_kernel (8-wave tiles):
 *              the rest of their records is what the saving launch of the same shape records
 *   out[1..4]  the template arguments: KT, FULL, MUL, NE | MP, FULL | NW; unused ones 0 (bools as 0 / 1)
 *   out[5..7]  the grid: x = workgroups (weight gradients: the K split after the clamp; fused kernels: tiles, or the persistent
 *              grid), y = k-row / channel groups, z = row halves (tz); 1 where a dimension is not used
 *   out[8]     weight gradients: operand sets;  fused kernels: tiles per sequence
 *   out[9]     weight gradients: 1 when a tap shift is not a multiple of 4 samples;  fused kernels: LDS ring slots
 *   out[10]    weight gradients: 1 when the reduce pass ran, 0 when the workgroups stored straight into the output (fst_nt_gemm);
 *              fused kernels: layers of the launch
 *   out[11]    dynamic LDS bytes of the launch
 * Returns 0, or -1 when no launch is recorded (out zero-filled) or out is null. */
#define FST_WN_ROUTE_LEN         12
#define FST_WN_ROUTE_WGRAD       1
#define FST_WN_ROUTE_TZ          2
#define FST_WN_ROUTE_LAYER_FWD   3
#define FST_WN_ROUTE_STACK_FWD   4
#define FST_WN_ROUTE_LAYER_BWD   5
#define FST_WN_ROUTE_LAYER_DGRAD 6
#define FST_WN_ROUTE_STACK_BWD   7
#define FST_WN_ROUTE_LAYER_INFER 8
#define FST_WN_ROUTE_STACK_INFER 9
int fst_wn_last_route(int32_t out[FST_WN_ROUTE_LEN]);

/* NoiseTransfer (/root/reference/widgets.py:150-167): new_t = avg_t + r_t·mean_b(z_t), new_s likewise, dist = new_t − new_s,
 * learned = selu(W·dist + bias) (unbatched 1x1 conv over the [C, L] map), out[b] = learned + z_s[b].
 *   fst_batch_sum            part[z][s][i] = Σ_{b in slice s} x_z[b][i] (z < 2 tensors, x1 may be NULL; S contiguous slices of the
 *                            batch, N = C·L, N % 4 == 0) — partials added in slice order by the consumers: deterministic
 *   fst_noise_transfer_fwd   slice sums [2][S][C·L] → avg_t, avg_s updated IN PLACE (the reference's detached state), dist, pre = W·dist +
 *                            bias and learned = selu(pre) written ([C][L] each).  r_*_dev: the call's accumulation ratios as device
 *                            scalars (a captured step refreshes them between replays) or NULL: the host values r_t, r_s
 *   fst_bcast_add            out[b][i] = x[b][i] + v[i]
 *   fst_noise_transfer_bwd   slice sums [S][C·L] of the cotangent of out → dpre = Σ_b g · selu'(pre), dd = Wᵀ·dpre (cotangent of dist)
 *   fst_noise_transfer_dw    dW[o][c] = Σ_l dpre[o][l]·dist[c][l], dbias[o] = Σ_l dpre[o][l]
 *   fst_noise_transfer_bwd_apply   dz_t[b] = (r_t/B)·dd,  dz_s[b] = g[b] − (r_s/B)·dd  (either output may be NULL) */
int fst_batch_sum(const float* x0, const float* x1, float* part, int B, int64_t N, int S, void* stream);
int fst_noise_transfer_fwd(const float* part, int S, int B, const float* r_t_dev, const float* r_s_dev, float r_t, float r_s,
                           float* avg_t, float* avg_s, const float* W, const float* bias, float* dist, float* pre, float* learned,
                           int C, int L, void* stream);
int fst_bcast_add(float* out, const float* x, const float* v, int B, int64_t N, void* stream);
int fst_noise_transfer_bwd(const float* part, int S, const float* pre, const float* W, float* dpre, float* dd, int C, int L,
                           void* stream);
int fst_noise_transfer_dw(const float* dpre, const float* dist, float* dW, float* dbias, int C, int L, void* stream);
int fst_noise_transfer_bwd_apply(const float* g, const float* dd, const float* r_t_dev, const float* r_s_dev, float r_t, float r_s,
                                 int B, float* dz_t, float* dz_s, int64_t N, void* stream);

/* generic fp32 elementwise helpers on contiguous buffers */
int fst_relu_bwd(const float* dy, const float* y, float* out, int64_t n, void* stream);   /* out = dy·[y > 0] (epilogue-fused ReLUs) */

/* Dense products of the small heads on the matrix cores in split-bf16 — replaces the aten addmm / mm calls behind
 * /root/reference/widgets.py:73-75 (DimensionUnification.length_unification: [B·C_s, L_s] × [L_t, L_s]ᵀ + ReLU), :113-131
 * (AdversarialNetworkforCDAN's Linear-ReLU chain), :32-42 (FeatureDiscriminatorforSource's Linear-LeakyReLU chain) and their gradients:
 *     C[m][n] = act( Σ_k A(m,k)·B(n,k) + bias[n] ),   m < M, n < N, k < K,   C row-major with row pitch ldc
 * ta = 0: A(m,k) = A[m·lda + k] (reduction index contiguous);  ta = 1: A(m,k) = A[k·lda + m] (reduction index major);  tb likewise for
 * B(n,k) — so   y = x·Wᵀ is (x, 0, W, 0),   dx = g·W is (g, 0, W, 1),   dW = gᵀ·x is (g, 1, x, 1),   no transposed copies.
 * Any M, N, K and pitches; 16-byte loads where rows allow them.  K is split across workgroups when the tiles alone do not fill the
 * chip: partial tiles go to `workspace` (fst_gemm_workspace_floats, 0 when no split is used) and are added in a fixed order — the
 * same bits on every run.  bias (may be NULL) is per output column; act = FST_ACT_*, slope = LeakyReLU's negative slope. */
#define FST_ACT_NONE  0
#define FST_ACT_RELU  1
#define FST_ACT_LEAKY 2
int64_t fst_gemm_workspace_floats(int M, int N, int K);
int fst_gemm(const float* A, int64_t lda, int ta, const float* B, int64_t ldb, int tb, float* C, int64_t ldc, int M, int N, int K,
             const float* bias, int act, float slope, float* workspace, int64_t workspace_floats, void* stream);
/* fst_gemm's contract in EXACT fp32 (ABI v21): the same arguments, layouts, refusals, K split and workspace rule, the operands unsplit
 * on v_mfma_f32_32x32x2_f32 — RandomLayer's feature-side product torch.mm(feature, R₀) under FST_MATH=f32 (C_DAN.py:20-25 of the
 * reference: (x, 0, R₀ᵀ, 0) with R₀ᵀ kept contiguous) and its data gradient (dy, 0, R₀ᵀ, 1), which read the same copy of the matrix.
 * Every C element is one fmaf chain, bit for bit: inside a 32-k stage starting at k0 the order is k0, k0+16, k0+1, k0+17, …, k0+15,
 * k0+31; the stages of a split in ascending k0 from 0.f; then the splits, slab z joining chain z mod 4 in ascending z (a tail of
 * fewer than four slabs joins chain 0), ((s0 + s1) + (s2 + s3)) + bias, activation.  No atomics, no zero fill: the same bits on every
 * run, and an exact result wherever every partial sum is representable.  A refusal returns -1 and launches nothing. */
int64_t fst_gemm_f32_workspace_floats(int M, int N, int K);
int fst_gemm_f32(const float* A, int64_t lda, int ta, const float* B, int64_t ldb, int tb, float* C, int64_t ldc, int M, int N, int K,
                 const float* bias, int act, float slope, float* workspace, int64_t workspace_floats, void* stream);
/* out = dy·act'(y) from the activation's output y: dy where y > 0, slope·dy elsewhere (slope = 0: ReLU) — nn.ReLU / nn.LeakyReLU backward
 * behind an activation that ran in fst_gemm's / fst_gemm_f32's epilogue. */
int fst_act_bwd(const float* dy, const float* y, float* out, int64_t n, float slope, void* stream);
int fst_axpy(float* y, const float* x, float alpha, int64_t n, void* stream);          /* y += alpha*x */
int fst_add_slices(float* dst, int64_t dst_bs, const float* a, int64_t a_bs, const float* b, int64_t b_bs,
                   int B, int C, int L, void* stream);                                  /* dst = a + b (b may be null) */

/* ---------------------------------------------------------------------------------------------
 * CPC InfoNCE (Comparison/SLARDA/train.py:72-76): for every prediction step i,
 * total_i = enc_i·pred_iᵀ (B×B, K=C); nce_sum = Σ_i Σ_b log_softmax(total_i)[b,b]  (the caller
 * multiplies by −1/(B·T)).  enc element (i,b,c) is read in place at enc[i*s_i + b*s_b + c*s_c]
 * (a strided view of the [B,C,L] feature tensor); pred is [T,B,C] contiguous; lse [T,B] is kept
 * for backward.  gout is the DEVICE scalar d loss / d nce.  t0_dev (optional DEVICE int32 scalar) adds
 * t0_dev[0]·s_i elements to enc/denc, so the random start index can change between hipGraph replays.
 * Rows (B encodings of this rank) and columns (Bc predictions) may differ: "global batch" data parallelism scores
 * the local rows against the predictions gathered from every rank, the positives at columns col_off + b.
 * ------------------------------------------------------------------------------------------- */
/* Up to 256 columns and 64 channels (split-bf16 arithmetic): the forward transposes the T steps it reads into a workspace
 * [T][B][C] (whole lines in, whole lines out) and runs the cross-Gram on v_mfma_f32_32x32x16_bf16 with hi/lo operands (ABI v11).
 * More than 256 columns are processed as panels of 256: the forward then needs a workspace of
 * fst_cpc_workspace_floats(T, B, C, Bc) floats for the per-panel softmax statistics, and the backward
 * accumulates denc across panels with fp32 atomics (the caller zero-fills denc — it must anyway outside [t0, t0+T)). */
int64_t fst_cpc_workspace_floats(int T, int B, int C, int Bc);
/* nce_sum is an array of fst_cpc_nce_slots(T, B, Bc) partial sums, one per workgroup, every slot written (no zero fill): the
 * caller adds them in slot order, so the loss is bit-identical from run to run (ABI v9; a zeroed scalar fed by float atomics before). */
int64_t fst_cpc_nce_slots(int T, int B, int C, int Bc);
int fst_cpc_nce_fwd(const float* enc, int64_t s_i, int64_t s_b, int64_t s_c, const int32_t* t0_dev /* optional */,
                    const float* pred /* [T][Bc][C] */, int T, int B, int C,
                    int Bc /* columns = negatives; = B on one GPU */, int col_off /* column of row 0's positive */,
                    float* lse /* [T][B] */, float* nce_sum /* [fst_cpc_nce_slots] partial sums */, float* workspace /* NULL if Bc <= 256 */,
                    void* stream);
int fst_cpc_nce_bwd(const float* enc, int64_t s_i, int64_t s_b, int64_t s_c, const int32_t* t0_dev /* optional */,
                    const float* pred, const float* lse, int T, int B, int C, int Bc, int col_off, const float* gout,
                    float* denc /* same strides as enc */, float* dpred /* [T][Bc][C] */, void* stream);

/* ---------------------------------------------------------------------------------------------
 * GRU recurrence of the CPC context network (Comparison/SLARDA/train.py:65-67: nn.GRU(C, 64, batch_first=True), h0 = 0),
 * one persistent launch per direction.  xproj [B][S][3H] = x_t·W_ihᵀ + b_ih for every step (gate order r | z | n, torch's);
 * the kernel runs steps 0..t_last (t_last_dev: optional DEVICE scalar, read instead of t_last so a captured graph can vary
 * it), saves h_all [B][S][H] and gates [B][S][4H] = (r, z, n, W_hn·h + b_hn).  Only h at step t_last is consumed by CPC.
 * Backward: dout [B][H] = d loss / d h_{t_last}; writes dxproj [B][S][3H] (→ d input, dW_ih, db_ih by GEMMs outside) and
 * dgh [B][S][3H] (dW_hh = Σ dgh ⊗ h_{t−1}, db_hh = Σ dgh); both must be zero-filled by the caller (steps > t_last stay 0).
 * H = 64 only.  numel_h = element count of h_all as the caller holds it.
 * ------------------------------------------------------------------------------------------- */
int fst_gru_fwd(const float* xproj, const float* w_hh, const float* b_hh, float* h_all, float* gates,
                const int32_t* t_last_dev, int t_last, int B, int S, int H, int64_t numel_h, void* stream);
int fst_gru_bwd(const float* w_hh, const float* h_all, const float* gates, const float* dout,
                const int32_t* t_last_dev, int t_last, float* dxproj, float* dgh, int B, int S, int H,
                int64_t numel_h, void* stream);

/* ---------------------------------------------------------------------------------------------
 * The 2-step LSTM of ProbTransfer (widgets.py:46-55: nn.LSTM(C, C, batch_first=True) over the pooled feature repeated
 * twice, h0 = c0 = 0; only h_n is consumed), one launch per direction.  xproj [B][4H] = x·W_ihᵀ + b_ih + b_hh (gate order
 * i | f | g | o, torch's; the same projection feeds both steps).  Forward: w_hh_t = W_hhᵀ [H][4H]; writes h2 [B][H] and
 * save [B][11H] = gates of step 1 | gates of step 2 | c1 | c2 | h1.  Backward: dh2 [B][H] = d loss / d h_n; writes
 * dxproj [B][4H] (→ d x, dW_ih, db_ih = db_hh by GEMMs outside) and dpre2 [B][4H] (dW_hh = Σ_b dpre2 ⊗ h1, h1 = save[..., 10H:]).
 * H <= 256.  numel_xproj = element count of the [B][4H] tensors as the caller holds them.
 * ------------------------------------------------------------------------------------------- */
int fst_lstm2_fwd(const float* xproj, const float* w_hh_t, float* h2, float* save, int B, int H, int64_t numel_xproj, void* stream);
int fst_lstm2_bwd(const float* w_hh, const float* save, const float* dh2, float* dxproj, float* dpre2, int B, int H,
                  int64_t numel_xproj, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Optimiser updates (train_and_test.py:97-106 torch.optim.RMSprop x10, Adam for CPC; stepped at :742-754) as single-pass
 * multi-tensor launches: the *_host arguments are HOST arrays of n_tensors device pointers / element counts / learning rates;
 * up to 64 tensors ride in one launch's kernel arguments (so a captured hipGraph replays them as they are).  Same update
 * formulas and operation order as torch (RMSprop: centered = False, momentum = 0; Adam: the capturable branch with ONE shared
 * device step counter, already incremented by the caller).
 * ALL n_tensors entries are validated (non-null pointers, 0 < element count < 2^31, non-null learning-rate address) on the host
 * BEFORE the first launch: a call that returns < 0 has updated no parameter and no moment, whichever entry was bad.
 * The *_dev entry points compute the same updates (one update body, bit-identical results for equal fp32 rates) with the learning
 * rates on the DEVICE, read when the kernel runs and not when it is launched: lr_dev_host is a HOST array of n_tensors device
 * addresses of fp32 scalars (tensors may share one), lr_dev one device scalar beside step_dev.  A captured launch then follows
 * what is written to those scalars between replays.
 * ------------------------------------------------------------------------------------------- */
int fst_rmsprop_multi(float* const* p_host, const float* const* g_host, float* const* v_host, const int64_t* numel_host,
                      const float* lr_host, int n_tensors, float alpha, float eps, void* stream);
int fst_adam_multi(float* const* p_host, const float* const* g_host, float* const* m_host, float* const* v_host,
                   const int64_t* numel_host, int n_tensors, const float* step_dev, float lr, float beta1, float beta2, float eps,
                   void* stream);
int fst_rmsprop_multi_dev(float* const* p_host, const float* const* g_host, float* const* v_host, const int64_t* numel_host,
                          const float* const* lr_dev_host, int n_tensors, float alpha, float eps, void* stream);
int fst_adam_multi_dev(float* const* p_host, const float* const* g_host, float* const* m_host, float* const* v_host,
                       const int64_t* numel_host, int n_tensors, const float* step_dev, const float* lr_dev, float beta1, float beta2,
                       float eps, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Anomaly guard (ABI v18): skip a train step whose update would consume a NaN or an inf, decided on the device, so that it works
 * inside a replayed hipGraph (the reference's protection is torch.autograd.set_detect_anomaly, train_and_test.py:24).
 * nonfinite_multi counts the elements of n_tensors fp32 tensors whose exponent bits are all ones, per group (group_host[i] in
 * 0..31; pointers 4-byte aligned, 0 < element count < 2^31), and only reads them.  slots_dev is int32 scratch of at least
 * nonfinite_slots(n_tensors) words that every call rewrites (nothing has to be zeroed): per tensor a record of 65 words, its
 * group id and the counts of its up to 64 workgroups.  A finalising launch writes counts_dev[32]
 * (int32, all 32 words) and, where the pointer is not NULL: verdict_dev[0] = 1 if a group whose bit is set in verdict_mask counted
 * anything (bit g: group g), else 0; ok_dev[0] = 1.0f - verdict; skipped_dev[0] += verdict.  n_tensors == 0 is a clean verdict.
 * The *_multi_guard entry points are the updates of rmsprop_multi[_dev] / adam_multi[_dev] (same update bodies: same bits on a
 * clean step) behind verdict_dev, read when the kernel RUNS: with a non-zero word nothing is written.  Learning rates: by value
 * (lr_host / lr) or by device address (lr_dev_host / lr_dev); for RMSprop exactly one of the two arrays, for Adam lr_dev or NULL.
 * guard_copy_multi copies words_host[i] 4-byte words from src_host[i] to dst_host[i] (4-byte aligned device pointers, no overlap)
 * when verdict_dev is NULL or (verdict_dev[0] != 0) == when (0 or 1), read when the kernel runs; otherwise it writes nothing.
 * Every entry is validated on the host BEFORE the first launch, as for the optimisers: a refused call has written nothing.
 * ------------------------------------------------------------------------------------------- */
int64_t fst_nonfinite_slots(int n_tensors);
int fst_nonfinite_multi(const float* const* x_host, const int64_t* numel_host, const int32_t* group_host, int n_tensors,
                        int32_t verdict_mask, int32_t* slots_dev, int64_t slots_len, int32_t* counts_dev, int32_t* verdict_dev,
                        float* ok_dev, int32_t* skipped_dev, void* stream);
int fst_rmsprop_multi_guard(float* const* p_host, const float* const* g_host, float* const* v_host, const int64_t* numel_host,
                            const float* lr_host, const float* const* lr_dev_host, int n_tensors, float alpha, float eps,
                            const int32_t* verdict_dev, void* stream);
int fst_adam_multi_guard(float* const* p_host, const float* const* g_host, float* const* m_host, float* const* v_host,
                         const int64_t* numel_host, int n_tensors, const float* step_dev, float lr, const float* lr_dev, float beta1,
                         float beta2, float eps, const int32_t* verdict_dev, void* stream);
int fst_guard_copy_multi(void* const* dst_host, const void* const* src_host, const int64_t* words_host, int n_tensors,
                         const int32_t* verdict_dev, int when, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Gradient norms and clipping on the device (ABI v22), so that a replayed hipGraph can report and bound its gradients (what
 * torch.nn.utils.clip_grad_norm_ does with a host decision).  Tensors, groups, launch geometry, refusals and the slot discipline
 * are nonfinite_multi's: fp32 tensors with 4-byte aligned pointers and 0 < element count < 2^31, group_host[i] in 0..31, at most 64
 * tensors per launch, every entry validated on the host before the first launch.
 * sumsq_multi only reads the tensors.  slots_dev is fp32 scratch of at least sumsq_slots(n_tensors) words that every call
 * rewrites: per tensor a record of 65 words, its group id as a float and the partial sums of x*x of its up to 64 workgroups
 * (one fp32 fma chain per thread, a fixed-order reduction per workgroup, no float atomics).  A finalising launch of one workgroup
 * adds a tensor's slots in slot order and a group's tensors in call order in fp64 and writes
 *   norms_dev[g]  = (float)sqrt(sum_g) for g in 0..31, norms_dev[32] = (float)sqrt(sum over all groups)      (fp32[33])
 *   coef_dev[g]   = c_g * c                                                                                  (fp32[32])
 * with c_g = min(1, limits_dev[g] / (norms_dev[g] + 1e-6)), c = min(1, limits_dev[32] / (sqrt(sum_g (c_g norms_dev[g])^2) + 1e-6)),
 * computed in fp64 from the fp32 norms and rounded once; limits_dev is fp32[33], +inf = no limit.  If any of the 33 norms is not
 * finite every coefficient is 1.0f (the norms are reported as they came out).  The same inputs give the same words on every run.
 * n_tensors == 0 writes zero norms and unit coefficients.
 * scale_multi multiplies tensor i in place by coef_dev[group_host[i]], read when the kernel RUNS; a workgroup whose coefficient is
 * exactly 1.0f returns before it loads anything, so those tensors keep their bits.  Nothing outside [x, x + numel) is touched.
 * ------------------------------------------------------------------------------------------- */
int64_t fst_sumsq_slots(int n_tensors);
int fst_sumsq_multi(const float* const* x_host, const int64_t* numel_host, const int32_t* group_host, int n_tensors,
                    float* slots_dev, int64_t slots_len, const float* limits_dev, float* norms_dev, float* coef_dev, void* stream);
int fst_scale_multi(float* const* x_host, const int64_t* numel_host, const int32_t* group_host, int n_tensors,
                    const float* coef_dev, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Weight averaging on the device (ABI v23): an exponential moving average of parameters and fp32 buffers that a replayed
 * hipGraph keeps up to date (what timm's ModelEma and torch.optim.swa_utils.AveragedModel do from the host).  Pairs of fp32
 * tensors with 4-byte aligned pointers that do not overlap, 0 < element count < 2^31, group_host[i] in 0..31, at most 64 pairs per
 * launch, every entry validated on the host before the first launch: a refused call has written nothing.
 * state_dev is a block of 66 4-byte words: [0] decay (fp32), [1] warm-up flag (int32), [2..33] count[32] (int32, completed updates
 * per group), [34..65] w[32] (fp32).  ema_multi first launches one workgroup that, from the words as they are when it RUNS, writes
 *   w[g] = 1 - d,  d = warm-up ? min(decay, (1 + count[g]) / (10 + count[g])) : decay,  then count[g] += 1
 * for every group g of active_mask (bit g; group 31 is the sign bit), in fp32, and w[g] = 0 with count[g] unchanged for every other group -- and for every
 * group if verdict_dev (optional, the anomaly guard's word) is non-zero.  Then avg[i] = fma(w[g], live[i] - avg[i], avg[i]) per
 * element, the subtraction and the fma each rounded once; w == 1 stores live[i] itself.  A workgroup whose w is exactly 0 returns
 * before it loads anything: those averages keep their bits.  live is only read.  n_tensors == 0 runs the prologue alone.
 * swap_multi exchanges a[i] and b[i] element for element; twice is the identity on every bit.
 * Pairs whose two pointers are 16-byte aligned move in 16-byte accesses, all others in 4-byte ones.
 * ------------------------------------------------------------------------------------------- */
int fst_ema_multi(float* const* avg_host, const float* const* live_host, const int64_t* numel_host, const int32_t* group_host,
                  int n_tensors, int32_t active_mask, void* state_dev, const int32_t* verdict_dev, void* stream);
int fst_swap_multi(float* const* a_host, float* const* b_host, const int64_t* numel_host, int n_tensors, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Gradient accumulation on the device (ABI v24): one optimiser step over a WINDOW of k calls, each on its own micro-batch, whose
 * position in the window is a device word, so that one captured launch series serves every position.  Pairs (acc, g) as for
 * ema_multi: fp32, 4-byte aligned pointers that do not overlap, 0 < element count < 2^31, at most 64 pairs per launch, every entry
 * and the state pointer validated on the host before the first launch: a refused call has written nothing.
 * state_dev is a 16-byte aligned block of eight 4-byte words: [0] k (int32 >= 1), [1] j (int32, folds done in the open window,
 * 0 <= j < k), [2] inv_k (fp32, written by the host together with k: float32(1 / k)), [3] windows (int32, closed windows),
 * [4..7] reserved, zero.  From the words as they are when a kernel RUNS, first = (j == 0) and closing = (j + 1 >= k):
 *   first: acc = g (acc is not read: no zero fill is ever needed);  otherwise acc = acc + g, one fp32 addition rounded once;
 *   closing: then g = acc * inv_k in place, one fp32 multiplication rounded once;  on every other call g is only read.
 * With k == 1 a workgroup returns before it loads anything: g and acc keep every bit.  NaN and inf are not special-cased.
 * With advance != 0 a one-workgroup launch behind the folds sets j = closing ? 0 : j + 1 and windows += closing; n_tensors == 0
 * with advance runs that launch alone.  Calls with advance == 0 followed by one with advance != 0 all see the same j.
 * Pairs whose two pointers are 16-byte aligned move in 16-byte accesses, all others in 4-byte ones.
 * ------------------------------------------------------------------------------------------- */
int fst_accum_multi(float* const* acc_host, float* const* g_host, const int64_t* numel_host, int n_tensors, void* state_dev,
                    int advance, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Device-resident datasets (ABI v25): the batch of a step gathered on the device from a data set and an epoch plan that were
 * uploaded once, the plan's current row a device word, so that one launch pair serves every row and nothing crosses from the host
 * per step.  Up to 8 streams (x_t, y_t, x_s, y_s, ...), stream s being a source of n_rows[s] rows of row_words[s] 4-byte words,
 * a destination of batch[s] such rows and a device index table int32 [steps][batch[s]] (an int64 label is a row of 2 words); up to
 * 8 scalars, scalar k being a device table of 4-byte words [steps][n_scalars] and a destination word.  Every pointer non-null and
 * 4-byte aligned, 0 < row_words, n_rows, batch, row_words * batch < 2^31, no destination overlapping its source or the state
 * block, every entry validated on the host before the first launch: a refused call has written nothing.
 * state_dev is a 16-byte aligned block of eight int32 words: [0] cursor (current plan row), [1] steps (rows in the plan), [2] fed
 * (rows served), [3] overrun (calls that found cursor >= steps), [4] bad_index (rows whose index fell outside 0..n_rows-1),
 * [5..7] reserved, zero.  Two launches per call, both reading cursor and steps when they RUN.  If 0 <= cursor < steps:
 *   dst_s[b] = src_s[index_s[cursor * batch_s + b]] for every stream s and row b, moved as 32-bit integers (every bit pattern
 *   survives); a row whose index is outside 0..n_rows_s-1 is left unwritten and its index is never dereferenced;
 *   scalar_dst_k[0] = table_k[cursor * n_scalars + k];
 *   then a one-workgroup launch adds the row's count of such indices to bad_index, fed += 1, cursor += 1 (plain stores, one lane).
 * Otherwise no destination word is written, overrun += 1 and the cursor stays.
 * A stream whose row_words is a multiple of 4 and whose two base pointers are 16-byte aligned moves in 16-byte accesses, every
 * other in 4-byte ones.  A stream's batch is one flat range of such units over at most 2048 workgroups of the launch: a long row
 * spreads over several workgroups, short rows share one.
 * ------------------------------------------------------------------------------------------- */
int fst_feed_batch(const void* const* src_host, void* const* dst_host, const int32_t* const* index_host,
                   const int64_t* row_words_host, const int64_t* n_rows_host, const int64_t* batch_host, int n_streams,
                   const void* const* table_host, void* const* scalar_dst_host, int n_scalars, void* state_dev, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Evaluation on the device (ABI v26): a pass over a data set folded batch by batch into device words, and closed by a launch that
 * decides on the device whether the pass is the best so far.  Every argument is validated on the host before the first launch: a
 * refused call has written nothing.  Every word that steers a kernel is read when the kernel RUNS.  No float atomics.
 *
 * eval_fold folds one batch.  logits: fp32 [B][ld], ld >= C; labels: int64 [B]; valid_dev: one int32 word, clamped to 0..B: rows
 * 0..valid-1 count, the others are padding and are never read (neither their logits nor their labels).
 * state_dev is a 16-byte aligned block of eight int32 words: [0] seen (rows folded in this pass; also where this batch's outputs
 * go), [1] hits, [2] batches, [3] bad_label (labels outside 0..C-1), [4] nonfinite (rows holding a NaN or an inf), [5] overflow
 * (calls that found seen + valid > capacity), [6..7] reserved, zero.  loss_dev: one fp64 word.  confusion_dev: int32 [C][C],
 * row = label, column = prediction.  pred_out: int64 [capacity] and logits_out: fp32 [capacity][C], either may be NULL; both are
 * written at rows seen..seen+valid-1 (the logits moved as 32-bit integers: every bit pattern survives).  scratch: B fp64 words
 * followed by B int32 words, 8-byte aligned, contents of no meaning between calls.
 * If seen + valid > capacity the call writes nothing but overflow += 1.  Otherwise, per valid row:
 *   pred = the first index of the row's maximum as torch.argmax finds it on the CPU: a NaN beats every number and the first NaN
 *          wins; -0.0 == +0.0 is a tie that the lower index takes;
 *   nll  = -((x[label] - m) - log(sum_c exp(x[c] - m))), m the row's maximum, evaluated in fp64 from the fp32 logits: what
 *          F.cross_entropy(row.double(), label) evaluates; a NaN or an inf in the row so makes it NaN;
 *   a label outside 0..C-1 is counted in bad_label, its prediction (and logits) still stored, and it enters neither hits nor the
 *   confusion matrix nor the loss; otherwise confusion[label][pred] += 1 (integer atomic), hits += (pred == label);
 *   a row holding a NaN or an inf is counted in nonfinite and folded like any other.
 * A one-workgroup launch behind the rows then adds the rows' nll to loss_dev as ONE chain of fp64 additions in row order,
 * starting from the word's value (the loss of a pass does not depend on how the pass is cut into batches), and moves seen, hits,
 * batches and the counters on with plain stores from one lane.  One wave per row, four rows per 256-thread workgroup.
 * 1 <= B < 2^31, 1 <= C <= 4096, C <= ld < 2^31, 1 <= capacity < 2^31; pointers 4-byte aligned, those to int64 / fp64 data and the
 * scratch 8-byte, the state block 16-byte; no output (state, loss, confusion, pred_out, logits_out, scratch) overlaps an input
 * (logits, labels, valid) or another output.
 *
 * eval_finish closes a pass: one workgroup.  best_dev is a 16-byte aligned block of eight 4-byte words: [0] improved (int32,
 * written by every call), [1] passes, [2] best_hits (int32, initially -1), [3] best_pass (the value of passes, counted from 1, of
 * the best pass), [4..5] best_loss (fp64, initially +inf), [6] incomplete, [7] reserved.  The pass is complete if seen ==
 * expect_rows and overflow == 0 and bad_label == 0.  improved = complete and (mode == 0 ? hits > best_hits : loss < best_loss): a
 * tie does not improve and a NaN loss never does.  Where it improved, best_hits, best_loss and best_pass take this pass's values;
 * an incomplete pass adds one to incomplete; passes += 1 always.
 * ------------------------------------------------------------------------------------------- */
int fst_eval_fold(const float* logits, int64_t ld, const int64_t* labels, int64_t B, int C, const void* valid_dev, void* state_dev,
                  void* loss_dev, void* confusion_dev, int64_t* pred_out, float* logits_out, int64_t capacity, void* scratch,
                  void* stream);
int fst_eval_finish(const void* state_dev, const void* loss_dev, int64_t expect_rows, void* best_dev, int mode, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Multi-source voting on the device (ABI v27; multi_source_voting.py:265-429): K <= 16 target-side models vote on a test set, batch
 * by batch, into device words, as eval_fold folds one model's pass.  Every argument is validated on the host before the first
 * launch: a refused call has written nothing.  Every word that steers a kernel is read when the kernel RUNS.  No float atomics.
 * All arithmetic is fp64 (base and sharpen arrive as fp32 and are widened).  1 <= K <= 16, 1 <= C <= 4096.
 *
 * vote_weights: one launch, one thread per class.  confusion_host: a host array of K device pointers to int32 [C][C], row = label,
 * column = prediction (eval_fold's), read when the kernel runs.  weights_out, scale_out: fp64 [K][C], 8-byte aligned, overlapping
 * neither each other nor a matrix.  base > 0 and finite.  Per class c:
 *   predicted_k = sum_r cm_k[r][c] (an integer sum);  prec_k = predicted_k > 0 ? cm_k[c][c] / predicted_k : 0;
 *   mean = (sum_k prec_k) / K, summed with k ascending;  w_k = prec_k / mean, a quotient that is not finite (0 / 0) becoming 0;
 *   weights_out[k][c] = w_k;  scale_out[k][c] = pow(base, w_k).
 * (voting.precision_weights_from_confusion's arithmetic.)
 *
 * vote_fold folds one batch: two launches.  logits_host: a host array of K device pointers to fp32 [B][ld], ld >= C common to all;
 * scale: fp64 [K][C]; labels: int64 [B]; valid_dev: one int32 word, clamped to 0..B: rows 0..valid-1 count, the others are padding
 * and are never read.  state_dev: eval_fold's block of eight int32 words, the same meanings ([0] seen ... [5] overflow).
 * member_hits_dev: int32 [K].  confusion_dev: int32 [C][C] of the VOTED prediction.  pred_out: int64 [capacity]; scores_out: fp64
 * [capacity][C], may be NULL; both written at rows seen..seen+valid-1.  scratch: 2 B int32 words, contents of no meaning between
 * calls.  sharpen >= 0 and finite.  If seen + valid > capacity the call writes nothing but overflow += 1.  Otherwise, per valid
 * row and for each member k (x = its fp32 logits, widened):
 *   m_k = max_c x_c (a NaN in the row is the maximum);  e_c = exp(x_c - m_k);  s_k = sum_c e_c;
 *   T_k = sum_c e_c * (x_c - m_k), a term with e_c == 0 counting as 0 (a -inf logit has probability 0 and makes no NaN);
 *   H_k = log(s_k) - T_k / s_k  (= -sum p log p: two non-negative terms, no cancellation);  f_k = 1 + sharpen * exp(-H_k);
 * then score_c = sum_k e_kc / s_k * f_k * scale[k][c], summed with k ascending; the voted prediction is the argmax of the scores by
 * eval_fold's rule (first maximum; a NaN beats every number and the first NaN wins; -0.0 == +0.0 ties to the lower index);
 * member k's own prediction is that argmax of its fp32 logits.  A label outside 0..C-1 is counted in bad_label, the row's
 * prediction (and scores) still stored, and it enters neither hits nor member_hits nor the confusion matrix; otherwise
 * confusion[label][pred] += 1 (integer atomic), hits += (pred == label), member_hits[k] += (member k's prediction == label).  A row
 * holding a NaN or an inf in any member is counted once in nonfinite and folded like any other.
 * One wave per row, four rows per 256-thread workgroup, the classes strided over the lanes and every sum over classes closed by
 * a butterfly, so a row's bits do not depend on the batch it arrives in.  A one-workgroup launch behind the rows adds the rows'
 * counters in a fixed order and moves seen, hits, batches, the counters and member_hits on with plain stores from one lane.
 * 1 <= B < 2^31, C <= ld < 2^31, 1 <= capacity < 2^31; pointers 4-byte aligned, those to int64 / fp64 data 8-byte, the state block
 * 16-byte; no output (state, member_hits, confusion, pred_out, scores_out, scratch) overlaps an input (the logits, labels, scale,
 * valid) or another output.
 * ------------------------------------------------------------------------------------------- */
int fst_vote_weights(const void* const* confusion_host, int K, int C, float base, double* weights_out, double* scale_out,
                     void* stream);
int fst_vote_fold(const float* const* logits_host, int K, int64_t ld, const int64_t* labels, int64_t B, int C, const double* scale,
                  const void* valid_dev, void* state_dev, void* member_hits_dev, void* confusion_dev, int64_t* pred_out,
                  double* scores_out, float sharpen, int64_t capacity, void* scratch, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Transfer monitor (ABI v28; csrc/mmd.hip, monitor.py): the multi-kernel maximum mean discrepancy between feature sets — what the
 * reference's t-SNE dumps show by eye (train_and_test.py:564-621, :792-797).  Every argument is validated on the host before the
 * first launch: a refused call has written nothing.  Every device word is read when its kernel RUNS.  No float atomics, no zero
 * fill: same inputs, same bits.
 *
 * mmd_centre: centre[k] = the mean of column k over the n rows of one set x [n][ld], ld >= D (one launch; four row quarters per
 * column, each summed in row order, joined as (0 + 1) + (2 + 3)).  Pointers 4-byte aligned.
 *
 * mmd_gram: x_host / rows_host / ld_host are host arrays of n_sets <= 4 entries: device pointers to fp32 row sets X_s [rows_s][ld_s],
 * 16-byte aligned, ld_s >= D, anywhere in memory; R = sum rows_s <= 1024; 1 <= D <= 2^28.  centre: fp32 [D] or NULL.  Writes the
 * contiguous G [R][R] = Zc·Zc^T of the pooled rows Z = [X_0; X_1; ...] minus the centre (subtracted in fp32 while a row is staged),
 * in split-bf16 on the matrix cores.  Only the upper-triangular 128 x 128 tiles are computed; the reduce writes G_ij and G_ji from
 * one sum, so G equals its transpose bit for bit.  K is cut into slabs of 8192 columns (mmd_gram_splits; the cut depends on D
 * alone), partial tiles go to `workspace` (mmd_gram_workspace_floats(R, D) floats, 16-byte aligned) and are added in slab order.
 * The bits of G_ij depend on rows i and j only: not on the other sets of the call, nor on the rows' place in the pool.  Columns
 * past D in the last 32-column stage enter as zeros and are not read.  No output overlaps an input.
 *
 * mmd_fold: G as mmd_gram wrote it for the sets rows_host [n_sets]; pairs_host: n_pairs <= 8 pairs (a, b) of set indices, a != b,
 * both sets of at least 2 rows.  One workgroup per pair, all in fp64: with x = set a (n rows), y = set b (m rows), N = n + m,
 *   d2_ij = max(G_ii + G_jj - 2 G_ij, 0) (a NaN stays one), d2_ii = 0;   bw = sum_{i != j} d2_ij / (N^2 - N), replaced by
 *   *bandwidth_override_dev when that word (fp64, may be NULL) is positive;   k_ij = sum_{q < kernels} exp(-d2_ij / (bw mul^(q - kernels/2)));
 *   mmd2 = sum_{i != j in x} k / (n (n - 1)) + sum_{i != j in y} k / (m (m - 1)) - 2 sum_{i in x, j in y} k / (n m);  bw == 0: mmd2 = 0.
 * out [n_pairs][5] (fp64) = mmd2, bw, mean d2 within x, within y, between.  Unless *live_dev (int32, may be NULL) is 0: a pair whose
 * mmd2 is finite adds its five numbers to sum [n_pairs][5] and 1 to count [n_pairs] (int32); one whose mmd2 is not adds 1 to the
 * int32 word *nonfinite and leaves the sums alone.  1 <= kernels <= 16, 0 < mul <= 1e30 (it arrives as fp32 and is widened).
 * ------------------------------------------------------------------------------------------- */
#define FST_MMD_MAX_SETS 4
#define FST_MMD_MAX_ROWS 1024
#define FST_MMD_MAX_PAIRS 8
#define FST_MMD_MAX_KERNELS 16
int fst_mmd_gram_splits(int R, int D);
int64_t fst_mmd_gram_workspace_floats(int R, int D);
int fst_mmd_centre(const float* x, int64_t ld, int n, int D, float* centre, void* stream);
int fst_mmd_gram(const float* const* x_host, const int32_t* rows_host, const int64_t* ld_host, int n_sets, int D, const float* centre,
                 float* G, float* workspace, int64_t workspace_floats, void* stream);
int fst_mmd_fold(const float* G, const int32_t* rows_host, int n_sets, const int32_t* pairs_host, int n_pairs, int kernels, float mul,
                 const double* bandwidth_override_dev, const int32_t* live_dev, double* out, double* sum, int32_t* count,
                 int32_t* nonfinite, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* FST_HIP_H */
