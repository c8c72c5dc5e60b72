/* hpvg.h - C ABI of libhpvg.so, the MI355X (gfx950) kernels behind the HP-VAE-GAN train step.
 *
 * Boundary contract: the reference (lior1990/hp-vae-gan, /root/reference) has no
 * FFI of its own - the hot path sits behind a Python module surface (modules/networks_3d.py,
 * networks_2d.py, losses.py, utils.py, utils/images.py) whose arithmetic is torch ATen ops.  Each
 * entry point below replaces one such ATen op (or a fused group) at the call site cited.  The Python
 * mirror of that module surface (package hp-vae-gan_amd/) binds these with ctypes; INTEGRATION.md
 * shows the stub a reference maintainer would add.
 *
 * Rules for every entry point:
 *   - plain pointers and sizes only; all tensors fp32, contiguous, NCDHW (2-D convs: T = 1, KT = 1);
 *   - pointers are DEVICE pointers unless stated; the caller owns every buffer, including workspace;
 *   - never allocates, never synchronises, never throws; work is enqueued on `stream` (a hipStream_t);
 *   - returns 0 (HPVG_OK) or a negative error code.
 *
 * Alignment and extent: an fp32 or int32 tensor argument (activations, weights, gradients, statistics, mask words, outputs)
 * needs 4-byte alignment only - a view that starts anywhere inside a larger buffer (x[n:], out[o:o+n]) is a valid argument.
 * Where a kernel has a wider load or store form, the launch picks it from the pointer value and the sizes and falls back to
 * the narrower form otherwise (hpvg_vec_width_at); the result does not depend on the start except through that choice.
 * Workspaces (`ws`) need 16-byte alignment, as stated per function.  A launch reads and writes nothing outside [p, p + n) of
 * any tensor argument of n elements: no whole-vector overrun past the last row or plane, before the first, or into the
 * bytes an allocator leaves behind a tensor (tests/test_offset_launches.py runs every launch inside guard bands).
 * A uint8 or int8 tensor argument (volumes, images, masks, frames, projection directions, byte outputs) may have ANY byte
 * alignment - sample i of a [N][T][H][W][3] array is a valid argument, odd start included - and nothing outside [p, p + n) of
 * its n bytes is read or written: no whole-word read before the first byte or past the last, no store beyond the last byte
 * (tests/test_byte_offset_launches.py runs every such launch at every byte residue inside guard bands).
 */
#ifndef HPVG_H
#define HPVG_H
#include <stddef.h>
#ifdef __cplusplus
extern "C" {
#endif

#define HPVG_OK 0
#define HPVG_ERR_ARG (-1)
#define HPVG_ERR_WORKSPACE (-2)
#define HPVG_ERR_UNSUPPORTED (-3)
#define HPVG_ERR_LAUNCH (-4)

/* ---- convolution: nn.Conv3d/nn.Conv2d k=3 s=1 p=1 (modules/networks_3d.py:51,63,175,341,362; networks_2d.py:56,68,181,202,223)
 * KT = 3: 3x3x3 taps, KT = 1: 3x3 taps.  Weights are first packed into MFMA fragment order. */
size_t hpvg_conv_wpack_floats(int Cin, int Cout, int KT);
/* w: layer weight [Cout_layer][Cin_layer][KT][3][3]; inv_scale: device scalar 1/sigma (spectral norm) or NULL.
 * transpose_flip=0 -> pack for forward; 1 -> pack for backward-data (a conv with Cin=Cout_layer, Cout=Cin_layer). */
int hpvg_conv_pack_weight_f32(const float* w, const float* inv_scale, float* wp, int Cin_layer, int Cout_layer, int KT,
                              int transpose_flip, void* stream);
/* y = conv(f(x), wp) + bias; f = identity or LeakyReLU_opt(in_scale[c]*x + in_shift[c]) applied before zero padding
 * (fused BatchNorm-apply of the producing ConvBlock3D, networks_3d.py:54-55); out_lrelu: LeakyReLU(0.2) epilogue
 * (ConvBlock3DSN, networks_3d.py:59-70). bias may be NULL. */
/* n <= HPVG_PACK_BATCH_MAX weights of one square layer shape (C -> C, C > 4) packed in one launch; flip[i] != 0: the
 * backward-data pack of item i.  w / wp / flip: host arrays. */
#define HPVG_PACK_BATCH_MAX 16
int hpvg_conv_pack_weight_batch_f32(int n, const float* const* w, float* const* wp, const int* flip, int C, int KT, void* stream);
/* Geometry-aware packs.  A pack made by the functions above serves every launch of the layer; the _for forms leave out the
 * two-axis Winograd fragments (the largest section) unless a launch of the given geometry - kernel view: B, T, H, W of the
 * conv's input - will read them (hpvg_conv_wants_wino2d), and are valid for launches of that geometry only. */
size_t hpvg_conv_wpack_floats_for(int Cin, int Cout, int KT, int B, int T, int H, int W);
int hpvg_conv_wants_wino2d(int B, int Cin, int Cout, int T, int H, int W, int KT); /* host only: 1 / 0 */
int hpvg_conv_pack_weight_for_f32(const float* w, const float* inv_scale, float* wp, int Cin_layer, int Cout_layer, int KT,
                                  int transpose_flip, int B, int T, int H, int W, void* stream);
int hpvg_conv_pack_weight_batch_for_f32(int n, const float* const* w, float* const* wp, const int* flip, int C, int KT, int B, int T,
                                        int H, int W, void* stream);
/* ws (optional, may be NULL): scratch of hpvg_conv_fwd_ws_bytes() bytes for the stream-K schedule (512 persistent
 * workgroups share the (tile, channel-chunk) items evenly; tiles cut across workgroups pass through ws as partial sums
 * and are finished in fixed order).  Without it the same kernel runs one workgroup per tile: slower on grids of 1-5
 * tiles per CU slot, results equal up to fp32 summation order. */
size_t hpvg_conv_fwd_ws_bytes(int B, int Cin, int Cout, int T, int H, int W, int KT);
/* out_mask (optional, shaped like y): y *= (out_mask > 0 ? 1 : 0.2) in the epilogue - leaky_relu_backward
 * (networks_3d.py:21) of the activation BELOW, fused into the backward-data conv of the layer that consumed it (the
 * conv's output is the gradient w.r.t. that activation; out_mask = the activated tensor, i.e. this layer's saved input). */
int hpvg_conv_fwd_f32(const float* x, const float* wp, const float* bias, const float* in_scale, const float* in_shift,
                      int in_lrelu, float* y, int out_lrelu, const float* out_mask, void* ws, size_t ws_bytes, int B, int Cin,
                      int Cout, int T, int H, int W, int KT, void* stream);
/* The same conv with the LeakyReLU sign mask in 1-BIT form ([B][ceil(C/32)][T*H*W] words, bit c%32 of word c/32 = activation
 * of channel c > 0; hpvg_conv_mask_words() of them): `bits_out` (nullable) is written by an out_lrelu epilogue for the
 * backward-data conv of the layer that consumes the activation, which passes it as `mask_bits` (nullable; instead of the
 * fp32 `out_mask` of hpvg_conv_fwd_f32: 8 mask loads per tile and lane instead of 128).  Cout > 4 only. */
size_t hpvg_conv_mask_words(int B, int C, int T, int H, int W);
int hpvg_conv_fwd_bits_f32(const float* x, const float* wp, const float* bias, float* y, int out_lrelu, const unsigned* mask_bits,
                           unsigned* bits_out, void* ws, size_t ws_bytes, int B, int Cin, int Cout, int T, int H, int W, int KT,
                           void* stream);
int hpvg_conv_fwd_plan(int B, int Cin, int Cout, int T, int H, int W, int KT, int* out10); /* host only: tile plan */
/* host only: the kernel family a plain launch of this shape runs on: 0 direct implicit GEMM, 1 Winograd F(2,3) along W (2/3 of
 * the direct matrix-core work), 2 Winograd F(2x2,3x3) (4/9), 3 narrow-output kernel (Cout <= 4).  bench.py prices the
 * roofline's executed flops with it. */
int hpvg_conv_fwd_kernel_kind(int B, int Cin, int Cout, int T, int H, int W, int KT);
/* host only: how a kind-2 launch of this shape is cut (any other shape: HPVG_ERR_UNSUPPORTED).  The two-axis kernel runs
 * rounds of 256 whole tiles; the tiles of a last round that is at most half full (after at least one full round) run in a
 * second launch as half tiles (2 per tile) or, up to 64 of them, quarter tiles (4 per tile), one per workgroup, with the same
 * bits as whole tiles (HPVG_W2_SPLIT=0: never).  out[0..3] = tiles of the whole-tile launch, leftover tiles, parts per
 * leftover tile (1 = not cut, 2, 4), workgroups of the second launch (0 when not cut). */
int hpvg_conv_w2_split(int B, int Cin, int Cout, int T, int H, int W, int KT, int* out4);
/* Wide layers (kernel view Cin >= 8, Cout > 32) have a second kernel behind the same entry points: Winograd F(2,3) along W
 * (four products per output pair and (dt, dh) instead of six, summed over the channels before the output transform: 2/3 of
 * the matrix-core work; fp32, ~1e-6 of the output scale away from the direct kernel).  The weight pack carries both forms;
 * which kernel a launch runs is decided per shape.  hpvg_conv_wino_config: mode 0 = direct kernel only, 1 = Winograd from
 * `min_positions` output positions (B*T*H*W) up, 2 = every eligible launch (3 / 4: the same with the kernel's staging form
 * forced - rows as they lie in memory with 16-byte LDS-DMA pieces / halo'd bands with dword pieces; otherwise by size;
 * 5: every eligible launch, the TWO-axis kernel F(2x2,3x3) - 4/9 of the direct matrix-core work, 3x3x3 only - wherever it
 * can run, 6: the one-axis kernel only; by default the two-axis kernel takes the largest launches); a
 * negative argument leaves that setting as it is; returns the mode in force (HPVG_ERR_UNSUPPORTED when the process was
 * started with HPVG_WINO=0).  Host only. */
int hpvg_conv_wino_config(int mode, long min_positions);
/* host only: the Winograd kernel's tile plan: out[0..9] = L, Tw, nrange, ntw, RS, pair blocks per wave, m-tiles per
 * workgroup, gridy, lds_bytes, ntiles */
int hpvg_conv_wino_plan(int B, int Cin, int Cout, int T, int H, int W, int KT, int* out10);
/* host only: tile plan of the narrow-output kernel (Cout <= 4): out[0..6] = RS, Th, nth, nb, npos, G, pitch, then nb triples
 * (window start, first output column, output columns); out needs 7 + 3*16 ints */
int hpvg_conv_narrow_plan(int B, int Cin, int Cout, int T, int H, int W, int KT, int* out55);
/* The 3x3x3 narrow-output layers with an even Cin have a second kernel behind the same entry points: one workgroup walks the
 * input planes of its (sample, row block, column band) with the time taps in the GEMM's N axis, so every input plane is
 * read and multiplied once instead of once per output plane it reaches.  Which kernel a launch runs is decided by size.
 * hpvg_conv_narrowt_plan (host only): its tile plan whether or not the launch picks it: out[0..8] = RS, Th, nth, nb, npos, G,
 * pitch, lds_bytes, 1 when a plain launch of this shape runs on it in the mode in force, then nb triples (window start,
 * first output column, output columns); out needs 9 + 3*16 ints; HPVG_ERR_UNSUPPORTED where the kernel cannot run.
 * hpvg_conv_narrowt_config (host only; environment: HPVG_NARROWT): 0 = by size, 1 = never, 2 = wherever it can run; a negative
 * argument leaves the setting as it is; returns the mode in force. */
int hpvg_conv_narrowt_plan(int B, int Cin, int Cout, int T, int H, int W, int KT, int* out57);
int hpvg_conv_narrowt_config(int mode);
/* dW (natural layout) of the conv above: aten::convolution_backward weight half, reached from
 * total_loss.backward() / errD_total.backward() (train_video.py:182,200). accumulate!=0: dw += result. */
size_t hpvg_conv_bwd_weight_ws_bytes(int B, int Cin, int Cout, int T, int H, int W, int KT);
int hpvg_conv_bwd_weight_f32(const float* dy, const float* x, const float* in_scale, const float* in_shift, int in_lrelu,
                             float* dw, int accumulate, void* ws, size_t ws_bytes, int B, int Cin, int Cout, int T, int H,
                             int W, int KT, void* stream);
int hpvg_conv_bwd_weight_plan(int B, int Cin, int Cout, int T, int H, int W, int KT, int* out10); /* host only */
/* host only: the kernel family of the weight gradient at this shape: 0 / 1 direct (a workgroup per time tap / all taps per
 * workgroup), 2 Winograd along W (2/3 of the direct matrix-core work), 3 Winograd over H and W (4/9), 4 narrow kernels */
int hpvg_conv_bwd_weight_kernel_kind(int B, int Cin, int Cout, int T, int H, int W, int KT);
/* Wide layers (Cin > 4 and Cout > 4) have a Winograd weight-gradient kernel behind the same entry point (the transpose of
 * the forward F(2,3) along W: four products per pair of output columns and (dt, dh) instead of six, summed over all
 * positions before the output transform: 2/3 of the matrix-core work, fp32).  mode 0 = never (the direct kernels), 1 = the
 * default: every wide layer on a Winograd kernel - the one-axis kernel wins at every size - and the two-axis kernel (mode 5)
 * where its size rule picks it, 2 = every wide layer on the one-axis kernel,
 * 3 = every wide layer without the 16-byte staging form (widths that are multiples of 4 otherwise get it), 4 = every
 * wide layer with the 16-byte form on four waves instead of eight; 5 = every wide layer, the TWO-axis kernel (the transpose
 * of F(2x2,3x3) over H and W: 16 products per 2 x 2 output positions and dt instead of 36, 4/9 of the direct matrix-core work)
 * (any width; by default it takes the launches whose workgroups walk enough tiles), 6 = every wide layer,
 * the one-axis kernel only (2, 3, 4 also keep to the one-axis kernel); negative = query.  Returns the mode in force.  Host only. */
int hpvg_conv_bwd_weight_wino_config(int mode);
/* The weight gradient and the conv's bias gradient db[o] (+)= sum_{b,positions} dy[b][o] from ONE launch, for the layers
 * hpvg_conv_bwd_weight_fuses_bias() reports 1 for (the Winograd weight-gradient kernel runs them: its centre-tap workgroups
 * hold every dy pair in registers anyway); HPVG_ERR_UNSUPPORTED elsewhere (use hpvg_channel_sum_f32).  Same workspace as
 * hpvg_conv_bwd_weight_f32.  Reference: the bias half of aten::convolution_backward, train_video.py:182,200. */
int hpvg_conv_bwd_weight_fuses_bias(int B, int Cin, int Cout, int T, int H, int W, int KT);
int hpvg_conv_bwd_weight_bias_f32(const float* dy, const float* x, float* dw, int accumulate, float* db, int accumulate_db, void* ws,
                                  size_t ws_bytes, int B, int Cin, int Cout, int T, int H, int W, int KT, void* stream);
int hpvg_conv_bwd_weight_wino_plan(int B, int Cin, int Cout, int T, int H, int W, int KT, int* out10); /* host only */
/* host only: tile plan of the two-axis Winograd weight-gradient kernel: out[0..9] as above, out[10] = 1 when the shape runs it by
 * default (size rule) */
int hpvg_conv_bwd_weight_wino2_plan(int B, int Cin, int Cout, int T, int H, int W, int KT, int* out11);
/* ---- tap-generic convolution: nn.Conv3d / nn.Conv2d with ker_size K in {3, 5, 7}, stride 1, zero padding K / 2 (the
 * reference's --ker-size, train_video.py:275; networks_3d.py:51,63,175 with opt.ker_size != 3).  KT = K: K x K x K taps,
 * KT = 1: K x K taps (T = 1).  Both run on the exact-fp32 matrix cores; the Python layer routes weights of tap side 5 and 7
 * here and never a 3-tap weight (K = 3 is accepted so that the family can be held against the tuned one).
 *   Forward / backward-data.  w: the LAYER weight in its natural layout, [Cout][Cin][KT][K][K] in the kernel's view for
 * flip == 0.  flip != 0 runs the backward-data conv of a layer weight [Cin][Cout][KT][K][K] (kernel view: Cin = the layer's
 * Cout, Cout = the layer's Cin): the conv with W'[o][c][tap] = w[c][o][ntaps - 1 - tap].  y = conv(x, W) + bias (nullable),
 * then LeakyReLU(0.2) when out_lrelu, then y *= (out_mask > 0 ? 1 : 0.2) when out_mask (shaped like y) is given.  No fused
 * BatchNorm prologue and no 1-bit mask form.  Any Cin >= 1 and Cout >= 1.
 *   ws: hpvg_convk_fwd_ws_bytes() bytes, 16-byte aligned, required: each call first writes the weight there in MFMA fragment
 * order (a launch of its own on `stream`) and the conv reads it; nothing is kept between calls, so the result is a function
 * of the arguments alone and two calls with the same inputs give the same bits.
 *   Weight gradient.  dw[o][c][tap] (+)= sum_{b,pos} dy[b][o][pos] * x[b][c][pos + off(tap)], zero outside the volume; dw in
 * the natural layout [Cout][Cin][KT][K][K]; accumulate != 0: dw += result.  Partial sums over position ranges go through ws
 * (hpvg_convk_bwd_weight_ws_bytes() bytes, 16-byte aligned) and are added in a fixed order by a second launch: no float
 * atomics.
 *   Both: no allocation, no host synchronisation, capturable; tensors need 4-byte alignment only; nothing outside a tensor
 * is read or written.  HPVG_ERR_ARG: K not in {3, 5, 7}, KT not in {1, K}, a size < 1, KT == 1 with T != 1, a null x / w / y
 * (dy / x / dw).  HPVG_ERR_WORKSPACE: ws null, not 16-byte aligned, or shorter than the _ws_bytes() of the same arguments.
 * HPVG_ERR_UNSUPPORTED: T * H * W >= 2^31, or 2^24 spatial tiles and more.  _ws_bytes(): 0 for arguments the call refuses. */
size_t hpvg_convk_fwd_ws_bytes(int B, int Cin, int Cout, int T, int H, int W, int KT, int K);
int hpvg_convk_fwd_f32(const float* x, const float* w, const float* bias, float* y, int out_lrelu, const float* out_mask, int flip,
                       void* ws, size_t ws_bytes, int B, int Cin, int Cout, int T, int H, int W, int KT, int K, void* stream);
/* host only: how many 32-channel M tiles a workgroup of the forward kernel takes when Cout > 32: 0 = by size (two once that
 * grid has more workgroups than the chip has CUs, else one), 1 = always one, 2 = always two; any other argument leaves the setting as it is;
 * returns the mode in force.  Every output's sum has the same order in both forms: the bits do not depend on it. */
int hpvg_convk_fwd_mt_config(int mode);
size_t hpvg_convk_bwd_weight_ws_bytes(int B, int Cin, int Cout, int T, int H, int W, int KT, int K);
int hpvg_convk_bwd_weight_f32(const float* dy, const float* x, float* dw, int accumulate, void* ws, size_t ws_bytes, int B, int Cin,
                              int Cout, int T, int H, int W, int KT, int K, void* stream);
/* out[c] = sum_{b,s} x[b][c][s]: conv bias gradient.  accumulate != 0: out[c] += (the caller passes the parameter's
 * gradient buffer, which removes autograd's AccumulateGrad add kernel) */
size_t hpvg_channel_sum_ws_bytes(int C);
int hpvg_channel_sum_f32(const float* x, float* out, int accumulate, void* ws, size_t ws_bytes, int B, int C, long S,
                         void* stream);

/* ---- BatchNorm3d/2d, train mode on every forward (networks_3d.py:54), eps 1e-5, momentum 0.1 */
size_t hpvg_bn_ws_bytes(int C);
int hpvg_bn_train_stats_f32(const float* x, const float* gamma, const float* beta, float* running_mean, float* running_var,
                            float momentum, float eps, float* mean, float* invstd, float* scale, float* shift, void* ws,
                            size_t ws_bytes, int B, int C, long S, void* stream);
/* the two above in two launches instead of three (the apply kernel finalizes its own channel's statistics) */
int hpvg_bn_train_fwd_f32(const float* x, const float* gamma, const float* beta, float* running_mean, float* running_var,
                          float momentum, float eps, float* mean, float* invstd, float* scale, float* shift, float* y, int lrelu,
                          int groups, void* ws, size_t ws_bytes, int B, int C, long S, void* stream);
/* groups > 1: the batch holds `groups` independent passes (B / groups samples each, back to back), each normalised with its
 * own statistics; running statistics updated once per group, in order; statistics arrays laid out [groups][4][C] (pass the
 * addresses of group 0's mean / invstd / scale / shift); workspace hpvg_bn_ws_bytes(C * groups) */
/* y = LeakyReLU_opt(scale[c]*x + shift[c]) (BN apply + nn.LeakyReLU(0.2), networks_3d.py:21,54-56) */
int hpvg_affine_act_f32(const float* x, const float* scale, const float* shift, float* y, int lrelu, int B, int C, long S,
                        void* stream);
/* backward of h = LeakyReLU_opt(BN_train(r)): dr, dgamma, dbeta (native_batch_norm_backward + leaky_relu_backward);
 * accumulate != 0: dgamma / dbeta += */
int hpvg_bn_act_bwd_f32(const float* dh, const float* r, const float* mean, const float* invstd, const float* scale,
                        const float* shift, int lrelu, int groups, float* dr, float* dgamma, float* dbeta, int accumulate, void* ws,
                        size_t ws_bytes, int B, int C, long S, void* stream);
/* host only: launch plan of the two calls above for 16-byte-aligned tensors: out[0] = 1 when the statistics finalize is
 * folded into the apply kernel (two launches for all groups; else three per group), out[1] = partial blocks per channel
 * and group, out[2] = vector width (floats per load) of the reduction kernels */
int hpvg_bn_plan(int B, int C, long S, int groups, int* out3);
/* host only: the vector width (4, 2 or 1 floats per load) the per-channel reductions - the BatchNorm family and
 * hpvg_channel_sum_f32 - pick for rows of S floats that start at address p: 4 needs p % 16 == 0 and S % 4 == 0, 2 needs
 * p % 8 == 0 and S % 2 == 0.  A launch over several tensors takes the narrowest of them.  _bn_: the narrowest over the
 * starts of `groups` groups of B / groups samples.  p is only looked at, never dereferenced. */
int hpvg_vec_width_at(const void* p, long S);
int hpvg_bn_vec_width_at(const void* p, int B, int C, long S, int groups);
/* SECOND-order backward of the same block: the WGAN-GP of a critic that contains BatchNorm (WDiscriminatorBaselines,
 * networks_3d.py:184-210; modules/utils.py:14-18) differentiates the first-order backward once more.  g = dL/d(dr);
 * outputs (each nullable): g_dh = dL/d(dh), g_r = dL/d(r), g_gamma = dL/d(gamma) (+= when accumulate).  torch:
 * batchnorm_double_backward + leaky_relu_backward (LeakyReLU'' = 0). */
size_t hpvg_bn_bwd2_ws_bytes(int C);
int hpvg_bn_act_bwd2_f32(const float* dh, const float* g, const float* r, const float* mean, const float* invstd, const float* scale,
                         const float* shift, int lrelu, float* g_dh, float* g_r, float* g_gamma, int accumulate, void* ws,
                         size_t ws_bytes, int B, int C, long S, void* stream);
/* BatchNorm with the batch split over ranks (one process per GPU): the rank-local per-channel sums are double pairs the
 * caller all-reduces (RCCL) between the two halves; statistics, running buffers and dr then follow from the global sums.
 * Same arithmetic as the single-GPU entry points above (which are sums + finalize / sums + apply in one call). */
int hpvg_bn_sums_f32(const float* x, double* sums, void* ws, size_t ws_bytes, int B, int C, long S, void* stream);
int hpvg_bn_finalize_f32(const double* sums, double count, const float* gamma, const float* beta, float* running_mean,
                         float* running_var, float momentum, float eps, float* mean, float* invstd, float* scale, float* shift,
                         int C, void* stream);
int hpvg_bn_act_bwd_sums_f32(const float* dh, const float* r, const float* mean, const float* invstd, const float* scale,
                             const float* shift, int lrelu, double* sums, void* ws, size_t ws_bytes, int B, int C, long S,
                             void* stream);
int hpvg_bn_act_bwd_apply_f32(const float* dh, const float* r, const float* mean, const float* invstd, const float* scale,
                              const float* shift, int lrelu, const float* sums, float inv_count, float* dr, int B, int C, long S,
                              void* stream);
/* out = dy * (h > 0 ? 1 : 0.2): leaky_relu_backward on the in-place activated tensor (networks_3d.py:21) */
int hpvg_lrelu_mask_mul_f32(const float* dy, const float* h, float* out, long n, void* stream);

/* ---- generator glue: tanh / residual (networks_3d.py:377,404), reparameterize (networks_3d.py:29-33) */
/* out = a + b: residual add of the SinGAN baseline generator (networks_3d.py:319) */
int hpvg_add_f32(const float* a, const float* b, float* out, long n, void* stream);
/* dst = src, or dst = 0 when src is NULL - as a kernel (concatenations / zero fills of an iteration that may be captured
 * into a hipGraph must not become memcpy / memset nodes) */
int hpvg_copy_f32(const float* src, float* dst, long n, void* stream);
/* dst[bc, t, h, w] = src[bc, t - oT, h - oH, w - oW] where that index lies inside src, +0.0f elsewhere: the zero pad (offset +p)
 * and crop (offset -c) of the SinGAN baselines' valid convolutions and padded volumes (networks_3d.py:205,247-268,300-318) and their
 * backwards (-p / +c), as one kernel indexed by destination (no memset / memcpy node in a captured iteration).  src: [BC][sT][sH][sW],
 * dst: [BC][dT][dH][dW]; 2-D: sT = dT = 1, oT = 0.  Offsets may be negative; dT * dH * dW <= 2^30. */
int hpvg_box_copy_f32(const float* src, float* dst, long BC, int sT, int sH, int sW, int dT, int dH, int dW, int oT, int oH,
                      int oW, void* stream);
int hpvg_tanh_fwd_f32(const float* x, const float* res /*nullable*/, float* y, long n, void* stream);
int hpvg_tanh_bwd_f32(const float* dy, const float* y, float* dx, long n, void* stream);
int hpvg_reparam_fwd_f32(const float* mu, const float* logvar, const float* eps, float* z, long n, void* stream);
int hpvg_reparam_bwd_f32(const float* dz, const float* logvar, const float* eps, float* dlogvar, long n, void* stream);

/* ---- losses: kl_criterion (modules/losses.py:7-9), nn.MSELoss (train_video.py:355), WGAN means (train_video.py:170,178,194) */
size_t hpvg_reduce_ws_bytes(void);
int hpvg_kl_fwd_f32(const float* mu, const float* logvar, float* out, void* ws, size_t ws_bytes, long n, void* stream);
int hpvg_kl_bwd_f32(const float* gout, const float* mu, const float* logvar, float* dmu, float* dlogvar, long n, void* stream);
int hpvg_mse_fwd_f32(const float* a, const float* b, float* out, void* ws, size_t ws_bytes, long n, void* stream);
int hpvg_mse_bwd_f32(const float* gout, const float* a, const float* b, float* da, long n, void* stream);
int hpvg_sum_scaled_f32(const float* x, float* out, double scale, void* ws, size_t ws_bytes, long n, void* stream);
int hpvg_sqsum_f32(const float* x, float* out, void* ws, size_t ws_bytes, long n, void* stream);
int hpvg_fill_scaled_f32(const float* gout, float coef, float* out, long n, void* stream);

/* ---- WGAN-GP (modules/utils.py:4-19): interpolate, per-voxel channel norm penalty and its gradient */
int hpvg_lerp_f32(const float* a, const float* b, const float* alpha, float* out, long n, void* stream);
int hpvg_gp_fwd_f32(const float* g, float* out, float lambda, void* ws, size_t ws_bytes, int B, int C, long S, void* stream);
int hpvg_gp_bwd_f32(const float* gout, const float* g, float* dg, float lambda, int B, int C, long S, void* stream);

/* ---- pyramid resize: F.interpolate(mode=tri/bilinear, align_corners=True) (utils/images.py:13,17,24,83-105),
 * optional fused noise injection yn = y + amp*noise (networks_3d.py:399-400).  BC = batch*channels. */
int hpvg_upsample_linear_ac_f32(const float* x, float* y, const float* noise, float amp, float* yn, long BC, int Ti, int Hi,
                                int Wi, int To, int Ho, int Wo, void* stream);
/* ---- N(0,1) noise (utils/images.py:49 zeros(..).normal_(0,1); networks_3d.py:32 reparameterisation eps): counter-based
 * Philox4x32-10 + Box-Muller, stream = (seed, call_id, iter[0]); iter: device int bumped once per train iteration
 * (hpvg_counter_inc_i32), so a replayed hipGraph draws fresh noise with unchanged launch arguments; NULL = 0.
 * out[i] = value i % 4 of block i / 4: philox(counter = (q_lo, q_hi, call_id, iter), key = (seed_lo, seed_hi)).  The Box-Muller
 * uniforms are (k + 0.5) * 2^-24 of the words' top 24 bits k, rounded in fp32: in [2^-25, 1], NOT the open interval (0, 1) -
 * k = 2^24 - 1 rounds to 1.0, which as a radius gives a pair of signed zeros (never NaN); |out| <= 5.887. */
int hpvg_normal_f32(float* out, long n, unsigned long long seed, unsigned call_id, const int* iter, void* stream);
int hpvg_uniform_f32(float* out, long n, unsigned long long seed, unsigned call_id, const int* iter, void* stream); /* U[0,1) */
/* resize + level noise generated in the kernel (networks_3d.py:395-400): y = resize(x), yn = y + amp * N(0,1) where the noise
 * is exactly what hpvg_normal_f32 would write for the same stream; samples b < first_noisy get yn = y (C channels per sample). */
int hpvg_upsample_linear_ac_noise_f32(const float* x, float* y, float* yn, float amp, long BC, int C, int first_noisy, int Ti, int Hi,
                                      int Wi, int To, int Ho, int Wo, unsigned long long seed, unsigned call_id, const int* iter,
                                      void* stream);
/* backward: dx = resize^T(dy + dy2); dy2 (nullable) is the gradient of the noisy output yn.  A gather over the input
 * voxels in a fixed order: no float atomics, bitwise reproducible, dx need not be zeroed. */
int hpvg_upsample_linear_ac_bwd_f32(const float* dy, const float* dy2, float* dx, long BC, int Ti, int Hi, int Wi, int To, int Ho,
                                    int Wo, void* stream);

/* ---- rings on the sampling path (generate --wrap): the generator's volumes with some axes closed into rings.  No backward is
 * built: rings are a sampling feature.
 * Circular pad.  x: [NC][T][H][W], out: [NC][T + 2 pt][H + 2 ph][W + 2 pw] with pad = (pt, ph, pw) (a host array; 2-D: T = 1,
 * pt = 0):  out[c, t, y, x] = x[c, mod(t - pt, T), mod(y - ph, H), mod(x - pw, W)]  with the non-negative modulus.  pad[a] = 0
 * leaves that axis alone; a pad may exceed its side (a side of 1 with a pad of 3 repeats the one slice 7 times).  An exact copy:
 * one launch, no workspace, no atomics, no host synchronisation.  Both pointers may sit at any 4-byte offset (the 16-byte stores
 * of the body start at out's first aligned element; the elements before and behind it are stored one by one).
 * HPVG_ERR_ARG: a NULL pointer, a side < 1, a pad < 0, out overlapping x; HPVG_ERR_UNSUPPORTED: out holds 2^31 elements or more. */
int hpvg_ring_pad_f32(const float* x, long NC, int T, int H, int W, const int* pad, float* out, void* stream);
/* Separable linear resize x [NC][Ts][Hs][Ws] -> out [NC][To][Ho][Wo] with wrap = (wt, wh, ww) flags (a host array, each 0 or 1,
 * anything else HPVG_ERR_ARG; NULL = all zero).  An axis without its flag follows the rule of hpvg_upsample_linear_ac_f32 exactly.
 * A ring axis of S source and O output positions has the source coordinate o S / O:  i0 = (o S) / O,  f = ((o S) % O) / O (one
 * fp32 division of the two integers),  i1 = (i0 + 1) % S,  weights 1 - f and f - the last sample interpolates towards the first.
 * S == O is the identity along that axis.  All flags zero is hpvg_upsample_linear_ac_f32 without noise, bit for bit (the same
 * kernel).  With O = k S on a ring axis the weights depend on o mod k only, so rolling x by r along it rolls out by k r, bit for
 * bit.  Level noise is added afterwards (hpvg_upsample_linear_ac_f32 at equal sizes is y = x, yn = x + amp * noise). */
int hpvg_upsample_linear_ring_f32(const float* x, long NC, int Ts, int Hs, int Ws, float* out, int To, int Ho, int Wo, const int* wrap,
                                  void* stream);

/* ---- data front-end (the step before the path): frames [N][H][W][3] uint8 RGB -> the stage's clip tensor
 * [3][count][h][w] fp32: cv2.resize(INTER_LINEAR) geometry per frame (datasets/generate_frames.py:44-46), temporal window
 * frame[first + k*step] (datasets/video.py:56-57), /255, K.hflip, K.normalize(0.5, 0.5), permute C,T,H,W (video.py:58-82).
 * quantize != 0 rounds the resized value to a uint8 level first, as cv2.resize on uint8 does. */
int hpvg_frames_resize_norm_u8_f32(const unsigned char* src, float* dst, int N, int H, int W, int first, int step, int count, int h,
                                   int w, int hflip, int quantize, void* stream);

/* ---- the programs' outputs (train_video / train_image / generate) */
/* write_video's frame conversion (utils/saver.py:8-19): x [B][C][T][H][W] fp32 -> out [B][T][H][W][C] uint8 with
 * out = (uint8) truncf(clamp((x + 1) * 127.5, 0, 255)), add and multiply rounded separately in fp32; NaN -> 0.  C = 1 or 3
 * (images: T = 1). */
int hpvg_video_to_u8_f32(const float* x, unsigned char* out, int B, int C, int T, int H, int W, void* stream);
/* per-iteration loss log: row (*cursor % capacity) of table [capacity][K] <- (*p[0], ..., *p[K-1]), then *cursor += 1.  The
 * cursor (a device int) is read and written by the kernel, so a replayed hipGraph appends a fresh row each time.  Values are
 * copied bit for bit.  1 <= K <= HPVG_LOG_MAX_K; the pointer struct is passed by value. */
#define HPVG_LOG_MAX_K 16
typedef struct { const float* p[HPVG_LOG_MAX_K]; } hpvg_scalar_ptrs;
int hpvg_scalar_log_append_f32(hpvg_scalar_ptrs src, int K, float* table, int capacity, int* cursor, void* stream);

/* ---- evaluation: exact patch nearest neighbours between two uint8 volumes (bidirectional patch similarity, Simakov et al. 2008;
 * the reference has no such measure - its samples are judged by eye or by SVFID, which needs pretrained C3D weights).
 * q [Tq][Hq][Wq][3] and r [Tr][Hr][Wr][3] are channels-last uint8 (images: T = 1).  Patch i of a volume is the
 * patch[0] x patch[1] x patch[2] x 3 block at the i-th position, in (t, y, x) raster order, of the grid with that side's stride
 * (qstride / rstride, each 3 ints, >= 1); D = 3 * patch[0] * patch[1] * patch[2].  patch / qstride / rstride: host arrays.
 * d2[i] = min_j sum (q_i - r_j)^2 and nn[i] = the SMALLEST j that attains it, both int32 [Nq] and exact: the contraction runs
 * on the i8 matrix cores with int32 accumulation, which needs D * 255^2 < 2^31.  The result does not depend on launch geometry
 * or timing.  HPVG_ERR_ARG: a patch larger than a volume, a stride < 1, D * 255^2 >= 2^31, Nq or Nr >= 2^31. */
/* host only: out3 = Nq, Nr, D */
int hpvg_patchnn_counts(int Tq, int Hq, int Wq, int Tr, int Hr, int Wr, const int* patch, const int* qstride, const int* rstride,
                        int* out3);
/* host only: bytes of workspace (both packed int8 patch matrices, their squared norms, one 64-bit merge key per query patch);
 * 0 for arguments hpvg_patchnn_u8 refuses */
size_t hpvg_patchnn_ws_bytes(int Tq, int Hq, int Wq, int Tr, int Hr, int Wr, const int* patch, const int* qstride,
                             const int* rstride);
/* ws: 16-byte aligned, at least hpvg_patchnn_ws_bytes() bytes (HPVG_ERR_WORKSPACE otherwise) */
int hpvg_patchnn_u8(const unsigned char* q, int Tq, int Hq, int Wq, const unsigned char* r, int Tr, int Hr, int Wr, const int* patch,
                    const int* qstride, const int* rstride, int* d2, int* nn, void* ws, size_t ws_bytes, void* stream);

/* ---- generation: the two kernels of the patch nearest-neighbour generator (GPNN, Granot et al. 2022; VGPNN, Haim et al. 2022;
 * the generate_patchnn program).  Volumes, patches, strides, geometry refusals and the workspace are those of hpvg_patchnn_u8.
 * The search with a weight per reference patch (GPNN's completeness normalisation): rweight is float [Nr] on the device,
 * score[i] = min_j float32(d2_ij) * rweight[j] with d2_ij the exact int32 squared distance, converted round-to-nearest-even
 * and multiplied once in fp32; nn[i] = the SMALLEST j that attains the minimum.  score: float [Nq], nn: int32 [Nq].  Contract:
 * every weight is a finite, positive, normal fp32 and every product stays normal (or is 0); then the result is defined bit for
 * bit and does not depend on launch geometry or timing.  Outside the contract no index leaves [0, Nr): a query patch that no
 * comparison won (NaN weights) gets score = +inf, nn = -1.  Workspace: hpvg_patchnn_ws_bytes(). */
int hpvg_patchnn_weighted_u8(const unsigned char* q, int Tq, int Hq, int Wq, const unsigned char* r, int Tr, int Hr, int Wr,
                             const int* patch, const int* qstride, const int* rstride, const float* rweight, float* score, int* nn,
                             void* ws, size_t ws_bytes, void* stream);
/* The vote (fold): out [Tq][Hq][Wq][3] rebuilt from patches of the values volume v [Tr][Hr][Wr][3].  nn: int32 [Nq], for every
 * patch i of the (Tq, Hq, Wq) grid at qstride the index, in v's grid at rstride, of the patch voted there.  For every output
 * voxel and channel: sum = the sum over the grid patches i that cover the voxel of the byte of values patch nn[i] at the same
 * offset inside the patch, cnt = their number, out = (2 sum + cnt) / (2 cnt) in integer arithmetic (the mean, halves rounded
 * up).  Patches with nn[i] < 0 or nn[i] >= Nr are skipped (nothing outside v is read); where cnt == 0 - the uncovered tail of
 * a strided grid, or only skipped patches - out takes fallback's byte.  fallback: [Tq][Hq][Wq][3]; out must NOT overlap
 * fallback, v or nn (HPVG_ERR_ARG): they are read while out is written.  A gather, one thread per voxel: exact, no atomics, no workspace. */
int hpvg_patch_vote_u8(const unsigned char* v, int Tr, int Hr, int Wr, const int* nn, int Tq, int Hq, int Wq, const int* patch,
                       const int* qstride, const int* rstride, const unsigned char* fallback, unsigned char* out, void* stream);
/* host only: out3 = Nq, Nr, the number of output voxels that no patch of the query grid covers */
int hpvg_patch_vote_counts(int Tq, int Hq, int Wq, int Tr, int Hr, int Wr, const int* patch, const int* qstride, const int* rstride,
                           long* out3);
/* The search over selected patches of both grids (patch inpainting, generate_patchnn --mask: the patches that overlap the hole
 * against the patches that avoid it).  qsel / rsel: int32 lists of grid indices on the device, STRICTLY ASCENDING, nqsel /
 * nrsel entries (host values).  A null list is the whole grid and its count is ignored; a non-null list with a count < 1 or
 * > N is HPVG_ERR_ARG.  Only the listed patches are packed and compared, so the work and the workspace follow the counts.
 * d2 / nn: int32 [Nq], the FULL query grid.  For a listed query patch d2 = the exact minimum over the listed reference patches
 * and nn = the index IN r's GRID of the smallest listed patch that attains it; every other entry gets d2 = -1, nn = -1,
 * written by the call, so hpvg_patch_vote_u8 skips it.  Independent of launch geometry and timing; both lists null: bit for
 * bit hpvg_patchnn_u8.  Ascending and in-range entries are the caller's contract: an index is clamped into [0, N), so
 * nothing outside a volume or an output is touched, and the result for such a list is unspecified. */
/* host only: bytes of workspace for lists of nqsel / nrsel entries; a NEGATIVE count stands for a null list (then the result
 * is hpvg_patchnn_ws_bytes()'s); 0 for a geometry hpvg_patchnn_u8 refuses and for a count of 0 or > N */
size_t hpvg_patchnn_subset_ws_bytes(int Tq, int Hq, int Wq, int Tr, int Hr, int Wr, const int* patch, const int* qstride,
                                    const int* rstride, long nqsel, long nrsel);
int hpvg_patchnn_subset_u8(const unsigned char* q, int Tq, int Hq, int Wq, const unsigned char* r, int Tr, int Hr, int Wr,
                           const int* patch, const int* qstride, const int* rstride, const int* qsel, long nqsel, const int* rsel,
                           long nrsel, int* d2, int* nn, void* ws, size_t ws_bytes, void* stream);
/* count[i] = the nonzero bytes of mask [T][H][W] (uint8, on the device) under patch i of the strided grid, int32 [N], exact:
 * 0 for a patch that avoids the hole.  Geometry refusals as for hpvg_patchnn_u8; no workspace. */
int hpvg_patch_mask_count_u8(const unsigned char* mask, int T, int H, int W, const int* patch, const int* stride, int* count,
                             void* stream);
/* Deterministic PatchMatch (Barnes et al. 2009; generate_patchnn --search patchmatch): an APPROXIMATE nearest-neighbour field
 * whose cost is linear in the number of patches, defined bit for bit.  Volumes as for hpvg_patchnn_u8; both patch grids are
 * dense (stride 1), raster order (t, y, x); qg = (gT, gH, gW) is the query grid, rg = (kT, kH, kW) the key grid,
 * Nq = gT gH gW, Nr = kT kH kW, D = 3 patch[0] patch[1] patch[2].
 *   Key of a pair (i, j): (d2_ij, j), or (float32(d2_ij) * rweight[j], j) with weights; d2_ij is the exact int32 squared
 * distance (converted round-to-nearest-even, one fp32 multiply).  Keys compare lexicographically, and a candidate replaces the
 * running best only when its key is STRICTLY smaller.
 *   h32(x): x ^= x >> 16; x *= 0x7feb352d; x ^= x >> 15; x *= 0x846ca68b; x ^= x >> 16, on 32 bits.
 *   rnd(i, it, k, ax) = h32(seed + i * 0x9E3779B9 + (it * 64 + k * 4 + ax) * 0x85EBCA6B), everything mod 2^32 (seed too);
 * i = the flat query index, ax = 0, 1, 2 for t, y, x.
 *   Start: with nn_init (int32 [Nq] on the device) every entry clamped into [0, Nr); without it the key coordinate along ax is
 * rnd(i, 0xFFFFFF, 0, ax) % rg[ax].  iters = 0 returns the scored start.
 *   Iteration it = 0 .. iters - 1 reads ONLY the field of the previous iteration (Jacobi).  For the query patch at grid
 * coordinate a, starting from its own old match as the running best, in this order:
 *   1. propagation: for ax = t, y, x and s = -1 then +1: if a + s e_ax lies in the query grid, the candidate is the key
 *      coordinate of that neighbour's old match minus s e_ax; it is skipped when it leaves the key grid;
 *   2. random search: R = max(kT, kH, kW); for k = 0, 1, ... while r_k = R >> k >= 1 the candidate is the running best's key
 *      coordinate plus, per axis, rnd(i, it, k, ax) % (2 r_k + 1) - r_k, each axis clamped into the key grid.
 * So a patch's key never increases from one iteration to the next.  d2 / nn: int32 [Nq], the final field's exact distance and
 * index; score: float [Nq] = float32(d2) * rweight[nn], NULL without weights (and optional with them).  The result depends on
 * the arguments only - not on launch geometry, stream or timing - and no index leaves [0, Nr).  Weights: the contract of
 * hpvg_patchnn_weighted_u8 (finite, positive, normal products).  One launch for the start and one per iteration on `stream`,
 * two field buffers in the workspace, no host synchronisation, capturable.
 * HPVG_ERR_ARG: the geometry refusals of hpvg_patchnn_u8, a grid side >= 65536, iters outside [0, 1024], score without rweight,
 * a null q, r, d2 or nn.  HPVG_ERR_WORKSPACE: ws null, not 16-byte aligned or shorter than hpvg_patchmatch_ws_bytes(). */
/* host only: bytes of workspace (two fields of nn, d2 and score); 0 for a geometry hpvg_patchmatch_u8 refuses */
size_t hpvg_patchmatch_ws_bytes(int Tq, int Hq, int Wq, int Tr, int Hr, int Wr, const int* patch);
int hpvg_patchmatch_u8(const unsigned char* q, int Tq, int Hq, int Wq, const unsigned char* r, int Tr, int Hr, int Wr,
                       const int* patch, const float* rweight, const int* nn_init, int iters, long seed, int* d2, int* nn,
                       float* score, void* ws, size_t ws_bytes, void* stream);
/* ---- rings (generate_patchnn --wrap: seamless video loops and tileable samples).  A sample volume [T][H][W][3] uint8, a patch
 * (pt, ph, pw) and ring flags wrap = (wt, wh, ww), each 0 / 1 (host array of 3 ints; NULL = all zero).
 *   Periodic grid: along an axis of S voxels and patch side p the grid has S positions if the axis is a ring, else S - p + 1;
 * the patch at grid coordinate g covers the voxel coordinates (g + d) mod S, d = 0 .. p - 1, on a ring axis and g + d
 * elsewhere.  Raster order (t, y, x).  A flag on an axis with p = 1 is legal; only the neighbourhood rule of the PatchMatch
 * below changes there.
 *   Circular pad: the volume with its first p - 1 slices appended along every ring axis, in the order t, y, x.  The dense patch
 * grid of the padded volume is the periodic grid, patch for patch, so every search runs on padded volumes unchanged.  The real
 * clip is never a ring: keys and values stay dense, non-wrapping grids.
 *   The vote onto a ring.  (Tq, Hq, Wq) is the UNPADDED output and the query grid is its periodic grid, dense; nn: int32 with
 * one entry per periodic-grid patch, indexing v's grid at rstride.  Per output voxel and channel sum and cnt run over all
 * periodic-grid patches that cover the voxel (modulo S on ring axes), the offset inside the patch is the d above, and
 * out = (2 sum + cnt) / (2 cnt) in integers.  Entries outside [0, Nr) are skipped; cnt == 0 takes fallback.  A gather, one thread
 * per voxel: no atomics, no workspace, no host synchronisation.  Refusals (geometry of the unpadded volume, aliasing of out) are
 * those of hpvg_patch_vote_u8; a flag other than 0 / 1 is HPVG_ERR_ARG.  All flags zero: bit for bit hpvg_patch_vote_u8 at
 * qstride = (1, 1, 1).  (A vote into the padded volume cannot be folded back afterwards: it returns rounded means, not sums.) */
int hpvg_patch_vote_wrap_u8(const unsigned char* v, int Tr, int Hr, int Wr, const int* nn, int Tq, int Hq, int Wq, const int* patch,
                            const int* rstride, const int* wrap, const unsigned char* fallback, unsigned char* out, void* stream);
/* PatchMatch between rings: hpvg_patchmatch_u8 on volumes q and r that arrive ALREADY circularly padded by the caller; qwrap /
 * rwrap (host arrays of 3 ints, 0 / 1, NULL = all zero) say which axes of the query / key PATCH GRID are rings.  (The forward
 * search of a generator step has the padded guess as its query, the reverse search as its reference.)  The rule is that of
 * hpvg_patchmatch_u8 with these changes only:
 *   propagation, query side: on a qwrap axis the neighbour a + s e_ax is taken modulo the query grid side and is never skipped
 * (on a side of 1 the neighbour is the patch itself);
 *   propagation, key side: on an rwrap axis the candidate "neighbour's old match minus s e_ax" is taken modulo the key grid
 * side; on other axes it is skipped when it leaves the grid;
 *   random search: on an rwrap axis the candidate coordinate is taken modulo the key grid side (the non-negative modulus; the
 * offsets reach R, which may exceed the side) instead of being clamped.
 * Hash, start, order of candidates, keys and tie rule, Jacobi reads, the weights contract, refusals, launches and
 * hpvg_patchmatch_ws_bytes() are unchanged; a flag other than 0 / 1 is HPVG_ERR_ARG.  Both flag arrays null or all zero: bit for
 * bit hpvg_patchmatch_u8. */
int hpvg_patchmatch_wrap_u8(const unsigned char* q, int Tq, int Hq, int Wq, const unsigned char* r, int Tr, int Hr, int Wr,
                            const int* patch, const int* qwrap, const int* rwrap, const float* rweight, const int* nn_init,
                            int iters, long seed, int* d2, int* nn, float* score, void* ws, size_t ws_bytes, void* stream);
/* ---- the pyramid's resize (generate_patchnn --antialias / --t-ratio, evaluate --scales): an exact, antialiased resize of a
 * uint8 volume src [Ts][Hs][Ws][3] to out [To][Ho][Wo][3], separable in definition, with a single rounding.
 *   Weights, per axis of S source and O output positions: R = max(O - 1, S - 1) and w(o, i) = max(0, R - |i (O - 1) - o (S - 1)|),
 * an integer; an axis with S == O is the identity (w = 1 for i == o, else 0).  So O == 1 averages the whole axis, S == 1
 * copies, O > S is linear align-corners interpolation, and O < S is the triangle filter of half-width (S - 1) / (O - 1) source
 * voxels around the align-corners centre o (S - 1) / (O - 1), normalised by the weights that fall inside the volume.  w > 0
 * exactly where |i (O - 1) - o (S - 1)| < R: the connection rule of the generator's mask resize (patchnn_mask_resize).
 *   Output, per voxel and channel: N = sum_{t,h,w} wt wh ww v, D = (sum wt)(sum wh)(sum ww), out = (2 N + D) / (2 D) in integer
 * arithmetic (the weighted mean, halves rounded up).  Exact 64-bit sums: the result is a function of the inputs alone,
 * independent of launch geometry and of how the sums are split.  Example: the axis 7 -> 4 on [0, 60, 120, 180, 240, 255, 255]
 * gives [20, 120, 229, 255]; the weights of output 1 are [0, 3, 6, 3, 0, 0, 0].
 *   HPVG_ERR_ARG: a side < 1.  HPVG_ERR_UNSUPPORTED: a volume of 2^31 voxels or more (the limit of the other uint8 volume
 * entry points), or 511 Dmax >= 2^63 with Dmax the largest D over the outputs (the numerator 2 N + D must fit 64 bits). */
/* host only: the refusals above; out2 (nullable) = Dmax and the largest number of source voxels one output reads */
int hpvg_volume_resize_check(int Ts, int Hs, int Ws, int To, int Ho, int Wo, long* out2);
/* The same refusals, before any launch; a null src or out, or out overlapping src (a gather: src is read while out is written)
 * is HPVG_ERR_ARG.  One launch on `stream`, no workspace, no atomics, no host synchronisation. */
int hpvg_volume_resize_u8(const unsigned char* src, int Ts, int Hs, int Ws, unsigned char* out, int To, int Ho, int Wo,
                          void* stream);
/* ---- the feathered composite (generate --guide-mask, generate_patchnn --guide-mask): out takes volume a inside a hole, volume b
 * far from it and an exact integer blend in between.  a, b, out: [T][H][W][3] uint8; mask: [T][H][W] uint8, nonzero = hole;
 * radius = (rt, rh, rw): host array of 3 ints, each in [0, 64].  All volumes on the device, at any byte offset.
 *   box(v) = the voxels u of the volume with |u_ax - v_ax| <= r_ax on every axis (clipped at the borders);
 *   dil(u) = 1 iff some voxel of box(u) is a hole, else 0;
 *   c(v) = the number of u in box(v) with dil(u) = 1;  n(v) = |box(v)|;
 *   out = (2 (c a + (n - c) b) + n) / (2 n) per channel, in integer arithmetic: the weighted mean, halves rounded up.
 * So out = a on every hole voxel (every u of box(v) has v in box(u): c = n); out = b on every voxel farther than 2 r_ax from
 * every hole voxel along some axis (c = 0); radius (0, 0, 0) is the hard composite (a on the hole, b elsewhere); an empty mask
 * returns b and a full mask a.  The numerator fits 32 bits: n <= 129^3 and 129^3 * 255 * 2 + 129^3 < 2^31.
 *   Dilation (a maximum) and the box count (a sum) are separable: the work is 1-D passes through the workspace, a pass of radius
 * 0 is skipped, and the last pass sums along t and blends.  No atomics, no host synchronisation, every launch on `stream`
 * (capturable), and the result is a function of the arguments alone - not of launch geometry, stream or timing.
 *   HPVG_ERR_ARG: a side < 1, a radius outside [0, 64], a null a / b / mask / out / radius, out overlapping a, b or mask.
 * HPVG_ERR_UNSUPPORTED: a volume of 2^31 voxels or more.  HPVG_ERR_WORKSPACE: ws null, not 16-byte aligned or shorter than
 * hpvg_mask_blend_ws_bytes() (radius (0, 0, 0) needs no workspace and takes a null one).  Refusals come before any launch. */
/* host only: bytes of workspace (two byte planes and two uint16 planes of the volume; 0 for radius (0, 0, 0) and for arguments
 * hpvg_mask_blend_u8 refuses) */
size_t hpvg_mask_blend_ws_bytes(int T, int H, int W, const int* radius);
int hpvg_mask_blend_u8(const unsigned char* a, const unsigned char* b, const unsigned char* mask, int T, int H, int W,
                       const int* radius, unsigned char* out, void* ws, size_t ws_bytes, void* stream);
/* The copied regions ("chunks") of a nearest-neighbour field (evaluate --chunks).  nn: int32 [Nq] on the device over the query
 * patch grid qgrid = (gT, gH, gW), raster order (t, y, x), holding indices into the key patch grid rgrid = (kT, kH, kW),
 * Nr = kT kH kW; d2: int32 [Nq] or NULL.  qgrid / rgrid / qstride / rstride: host arrays of 3 ints.  Patch i at grid coordinate
 * a with nn[i] at key coordinate b has the displacement b * rstride - a * qstride (per axis, in voxels).  It is KEPT iff
 * 0 <= nn[i] < Nr and (d2 == NULL or 0 <= d2[i] <= max_d2), so the -1 entries of hpvg_patchnn_subset_u8 never are.  Two grid
 * patches that differ by +1 along exactly one axis are a pair (no pair joins the end of a row or plane to the start of the
 * next); a pair is coherent iff both are kept and their displacements are equal; the chunks are the connected components of
 * the kept patches under coherent pairs.  labels: int32 [Nq], the smallest flat index of the patch's chunk, -1 where not kept.
 * sizes: int32 [Nq], the chunk's size where labels[i] == i, 0 elsewhere.  stats: int64 [6] = kept, in_place (kept with
 * displacement 0), coherent_pairs, chunks, largest size, sum of size^2.  Integer work throughout: exact, a function of the
 * inputs alone, independent of launch geometry and timing.  nn is only decoded arithmetically - nothing is read through it.
 * sizes and stats are cleared by the call itself; no workspace (labels holds the union-find forest meanwhile), no host
 * synchronisation.  HPVG_ERR_ARG, before any device work: a null nn / labels / sizes / stats or geometry array, a grid entry
 * < 1, a stride < 1, Nq or Nr >= 2^31, max_d2 < 0 with a non-null d2. */
int hpvg_nnf_chunks_i32(const int* nn, const int* d2 /*nullable*/, int max_d2, const int* qgrid, const int* rgrid,
                        const int* qstride, const int* rstride, int* labels, int* sizes, long long* stats, void* stream);

/* ---- evaluation: exact sliced Wasserstein distance between the patch distributions of two uint8 volumes (the SWD of PGGAN /
 * GPNN / GPDM with integer directions).  Patches, patch and stride as above.  dirs: int8 [P][D] on the device, entries in
 * {-1, 0, +1}.  proj(i, p) = sum_k dirs[p][k] * (byte[i][k] - 128) lies in [-128 D, +128 D]; hist[p][proj + 128 D] counts the
 * patches of the volume, int32 [P][NB] with NB = 256 D + 1 bins.  The contraction runs on the i8 matrix cores, the counts are
 * integer atomic adds: exact, and independent of launch geometry and timing.  hist is cleared by the call itself.  An entry
 * outside {-1, 0, +1} is the caller's error: projections that leave the bin range are not counted. */
/* host only: NB for a patch; 0 for a patch hpvg_patchproj_hist_u8 refuses */
size_t hpvg_patchproj_bins(const int* patch);
/* host only: bytes of workspace (the packed int8 patch matrix and the packed directions); 0 for arguments the call refuses */
size_t hpvg_patchproj_ws_bytes(int T, int H, int W, const int* patch, const int* stride, int P);
/* HPVG_ERR_ARG: the geometry refusals of hpvg_patchnn_u8, P < 1, hist not 4-byte aligned; ws as for hpvg_patchnn_u8 */
int hpvg_patchproj_hist_u8(const unsigned char* vol, int T, int H, int W, const int* patch, const int* stride, const signed char* dirs,
                           int P, int* hist, void* ws, size_t ws_bytes, void* stream);
/* num[p] = sum_b |Nb * cA_p(b) - Na * cB_p(b)| over the cumulative counts of histA / histB [P][NB]: Na * Nb * W1 of the two
 * empirical distributions of direction p, int64 [P], exact.  Na / Nb: the patch counts (each row's sum).  HPVG_ERR_ARG: P < 1,
 * Na or Nb outside [1, 2^31), NB not 256 D + 1 for a D = 3 pt ph pw that hpvg_patchproj_bins accepts, Na * Nb * 256 D >= 2^63. */
int hpvg_hist_w1_i32(const int* histA, long Na, const int* histB, long Nb, int P, long NB, long long* num, void* stream);

/* ---- evaluation: the two searches of improved precision / recall (Kynkaanniemi et al. 2019) and density / coverage (Naeem et
 * al. 2020) on patch sets (evaluate --prdc; ops.patch_knn_self / ops.patch_ball_count).  Volumes, patches, strides and the exact
 * int32 squared distance d2 are those of hpvg_patchnn_u8; both run on its i8 matrix-core tile, never store the products, and
 * their results are functions of the inputs alone, independent of launch geometry and timing.
 * Self k-nearest: kth[i][0..k) = the k smallest d2(i, j) over the patches j != i of the SAME volume's strided grid (N patches),
 * ascending and with multiplicity - the exclusion is by index, so another patch at distance 0 counts, each once.  kth: int32
 * [N][k] on the device.  One pass over the N x N products whatever k is.  HPVG_ERR_ARG: k < 1, k > 8, N <= k, and whatever
 * hpvg_patchnn_counts refuses. */
/* host only: bytes of workspace (the packed int8 patch matrix, its squared norms, the partial lists of the column splits); 0
 * for arguments hpvg_patchknn_self_u8 refuses */
size_t hpvg_patchknn_self_ws_bytes(int T, int H, int W, const int* patch, const int* stride, int k);
/* ws as for hpvg_patchnn_u8 */
int hpvg_patchknn_self_u8(const unsigned char* vol, int T, int H, int W, const int* patch, const int* stride, int k,
                          int* kth /* [N][k] ascending */, void* ws, size_t ws_bytes, void* stream);
/* Ball count: count[i] = #{j < Nr : d2(q_i, r_j) <= ref_radius[j]}, int32 [Nq], with an int32 radius per reference patch on the
 * device, every one >= 0 (the caller's contract; a negative radius counts nothing).  count is cleared by the call itself, so a
 * second call on the same output gives the same result; count[i] > 0 is "some ball holds q_i".  HPVG_ERR_ARG: what
 * hpvg_patchnn_counts refuses, a null pointer, count not 4-byte aligned. */
/* host only: bytes of workspace (both packed int8 patch matrices and their squared norms); 0 for arguments the call refuses */
size_t hpvg_patch_ball_count_ws_bytes(int Tq, int Hq, int Wq, int Tr, int Hr, int Wr, const int* patch, const int* qstride,
                                      const int* rstride);
/* ws as for hpvg_patchnn_u8 */
int hpvg_patch_ball_count_u8(const unsigned char* q, int Tq, int Hq, int Wq, const unsigned char* r, int Tr, int Hr, int Wr,
                             const int* patch, const int* qstride, const int* rstride, const int* ref_radius /* [Nr], >= 0 */,
                             int* count /* [Nq] */, void* ws, size_t ws_bytes, void* stream);

/* ---- spectral norm (nn.utils.spectral_norm, networks_3d.py:63): one power iteration, sigma, 1/sigma; backward through sigma */
int hpvg_sn_power_iter_f32(const float* w, float* u, float* v, float* sigma, float* inv_sigma, float* uv_copy, int Co, int K,
                           int do_iter, float eps, void* ws, size_t ws_bytes, void* stream);
/* the same for n <= HPVG_SN_BATCH_MAX independent layers in one launch (one workgroup per layer, e.g. the six SN convs of
 * WDiscriminator3D at the start of a forward), also writing w_eff[i] = w[i] / sigma_i.  The pointer / size arrays live on
 * the host; sig[i] -> 2 floats (sigma, 1/sigma); uv_copy may be NULL or hold NULLs; ws: sum(Co) floats. */
#define HPVG_SN_BATCH_MAX 8
int hpvg_sn_power_iter_batch_f32(int n, const float* const* w, float* const* u, float* const* v, float* const* sig,
                                 float* const* uv_copy, float* const* w_eff, const int* Co, const int* K, int do_iter, float eps,
                                 void* ws, size_t ws_bytes, void* stream);
/* out = x / s[0]: weight = weight_orig / sigma (torch SpectralNorm.compute_weight) */
int hpvg_div_scalar_f32(const float* x, const float* s, float* out, long n, void* stream);
/* dworig (+)= dweff/sigma - (sum(dweff .* worig)/sigma^2) u v^T  (backward of weight_orig -> weight) */
size_t hpvg_sn_bwd_ws_bytes(int Co, int K);
/* n layers in two launches (host arrays as above; uv[i] = the forward's (u, v) copy; ws: sum of hpvg_sn_bwd_ws_bytes) */
int hpvg_sn_bwd_batch_f32(int n, const float* const* dweff, const float* const* worig, const float* const* uv,
                          const float* const* sigma, float* const* dworig, const int* accumulate, const int* Co, const int* K,
                          void* ws, size_t ws_bytes, void* stream);
int hpvg_sn_bwd_f32(const float* dweff, const float* worig, const float* u, const float* v, const float* sigma, float* dworig,
                    int accumulate, void* ws, size_t ws_bytes, int Co, int K, void* stream);

/* ---- optimizer: clip_grad_norm_ (train_video.py:201) and optim.Adam (train_video.py:55,88) over flat arenas */
int hpvg_clip_scale_f32(float* g, long n, const float* sqsum, float max_norm, float* coef_out /*nullable, 2 floats*/,
                        void* stream);
/* step: 1-based count from the host, or step_dev (device int, non-NULL) for hipGraph replays */
int hpvg_adam_step_f32(float* p, const float* g, float* m, float* v, long n, float lr, float beta1, float beta2, float eps,
                       int step, const int* step_dev, void* stream);
int hpvg_counter_inc_i32(int* counter, void* stream);
/* ---- state digest (snapshot.py: a resume refuses a state that is not the one saved).  words: n 32-bit words on the device at
 * any 4-byte offset; acc: one 64-bit device word that the call ADDS to (the caller clears it):
 *   acc[0] += sum over i in [0, n) of fmix(((salt + i) * 0x9E3779B97F4A7C15) ^ word[i])   mod 2^64, word zero-extended,
 *   fmix(z): z ^= z >> 30; z *= 0xBF58476D1CE4E5B9; z ^= z >> 27; z *= 0x94D049BB133111EB; z ^= z >> 31   (splitmix64).
 * The sum is commutative: exact, a function of the words and the salt alone, independent of launch geometry and timing.  Calls
 * with salts 0 and n1 over two buffers equal one call over their concatenation.  One kernel node, no workspace, capturable.
 * n == 0 enqueues nothing.  HPVG_ERR_ARG: n < 0, a null acc, a null or misaligned words with n > 0. */
int hpvg_state_digest_u32(const void* words, long n, unsigned long long salt, unsigned long long* acc, void* stream);

/* ---- variant models (no trainer of the reference drives them; module-surface completeness): Encode3DVAE_nb / Encode2DVAE_nb
 * (networks_3d.py:110-138, networks_2d.py:115-143), GeneratorVAE_nb (networks_3d.py:409-485), reparameterize_bern
 * (networks_3d.py:38-45), kl_bern_criterion (losses.py:12-14).  Tensors [B][C][S], S = T*H*W. */
/* bern[b][s] = sigmoid(logit[b][s]); out = bern * f (broadcast over channels); backward: df, dlogit from dout and the gradient
 * arriving at bern itself (either may be NULL) */
int hpvg_gate_fwd_f32(const float* f, const float* logit, float* out, float* bern, int B, int C, long S, void* stream);
int hpvg_gate_bwd_f32(const float* dout, const float* f, const float* bern, const float* dbern_ext, float* df, float* dlogit, int B,
                      int C, long S, void* stream);
/* out[b][c] = scale * sum_s x[b][c][s] * (w ? w[b][s] : 1): nn.AdaptiveAvgPool3d(1) with scale = 1/S, and d(outer)/d(code) */
int hpvg_rowsum_f32(const float* x, const float* w, float* out, float scale, int B, int C, long S, void* stream);
/* out[b][c][s] = g[b][c] * (w ? w[b][s] : scale): code x map (z_vae_norm * z_vae_bern) and the average pool's backward */
int hpvg_outer_f32(const float* g, const float* w, float* out, float scale, int B, int C, long S, void* stream);
/* out[b][s] = sum_c a[b][c][s] * v[b][c]: d(outer)/d(map) */
int hpvg_colsum_f32(const float* a, const float* v, float* out, int B, int C, long S, void* stream);
int hpvg_reparam_bern_fwd_f32(const float* x, const float* eps, float* z, long n, void* stream);
int hpvg_reparam_bern_bwd_f32(const float* dz, const float* x, float* dx, long n, void* stream);
int hpvg_kl_bern_fwd_f32(const float* x, float* out, void* ws, size_t ws_bytes, long n, void* stream);
int hpvg_kl_bern_bwd_f32(const float* gout, const float* x, float* dx, long n, void* stream);

/* ---- hipGraph replay of the iteration (host only): node census of a captured graph, counts[t] per hipGraphNodeType t
 * (0 kernel, 1 memcpy, 2 memset, ...; child graphs included).  The trainers refuse a captured iteration that holds
 * memcpy / memset nodes: those are not reliably ordered against kernel nodes on this runtime. */
int hpvg_graph_node_census(void* graph, int* counts, int ntypes);

#ifdef __cplusplus
}
#endif
#endif /* HPVG_H */
