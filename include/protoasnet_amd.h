/*
 * protoasnet_amd.h -- C-ABI of the MI355X (gfx950) ProtoASNet hot path.
 *
 * The reference (hooman007/ProtoASNet) has no FFI / operator registry: its hot path is a
 * stack of torch.nn calls inside three nn.Modules.  This header is
 * the boundary a replacement exports *under* that nn.Module surface: one entry point per
 * fused stage, each citing the reference call site(s) it replaces.  The Python host side
 * (the protoasnet_amd Python package) binds these with ctypes and keeps the reference's module surface
 * (forward / push_forward / compute_occurence_map / state_dict keys) on top.
 *
 * Conventions
 *   - extern "C", plain pointers and sizes; no torch / C++ types.
 *   - Every pointer is DEVICE memory owned by the caller (torch's caching allocator).  The
 *     library never allocates, frees or retains device memory.  Workspaces are passed in.
 *   - Work is enqueued asynchronously on the caller's HIP stream (`stream`, a hipStream_t);
 *     no internal streams, no host synchronisation, safe to capture into a hipGraph.
 *   - Return 0 on success; non-zero = error, message via pasn_last_error() (thread-local).
 *   - dtype: PASN_F32 = 0, PASN_BF16 = 1.  Arithmetic always accumulates in fp32.
 *   - Activations are CHANNELS-LAST: [N][T][H][W][Cp] (T = 1 for images) with the channel
 *     stride Cp a multiple of 8 and channels >= C stored as zeros.  A logical NC(T)HW view
 *     of such a buffer is what the nn.Module surface hands back to reference callers.
 */
#ifndef PROTOASNET_AMD_H
#define PROTOASNET_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PASN_VERSION 100 /* round 1 */

enum { PASN_F32 = 0, PASN_BF16 = 1, PASN_U8 = 2 /* input clips of the *_gray_fwd entry points and pasn_clip_augment only */,
       PASN_I32 = 3 /* pasn_clip_augment parameter tables only */ };
enum { PASN_ACT_NONE = 0, PASN_ACT_RELU = 1, PASN_ACT_SIGMOID = 2, PASN_ACT_SWISH = 3, PASN_ACT_ABS = 4 };
enum { PASN_OK = 0, PASN_ERR_ARG = 1, PASN_ERR_LAUNCH = 2, PASN_ERR_UNSUPPORTED = 3 };

int pasn_version(void);
const char* pasn_last_error(void);

/* Tuning switches (csrc/tuning.h).  The reference has no counterpart: its kernels are cuDNN's, picked by `cudnn.benchmark = True`
 * (src/agents/base.py:20).  Here the routing of a layer onto a kernel is a pure function of its descriptor and of the PASN_* switches
 * that were set in the environment WHEN THE LIBRARY FIRST LOOKED (one snapshot; registered names only).  pasn_tuning_reload() takes a new
 * snapshot (tests and A/B tools call it after changing the environment); pasn_tuning_get() returns a switch's value in the snapshot or
 * NULL; pasn_tuning_report() writes "NAME=VALUE" lines of the switches in force (+ an "unknown: ..." line for PASN_* names the library
 * does not know, + the registry "name<TAB>class<TAB>meaning" when with_registry != 0) and returns the length needed. */
void pasn_tuning_reload(void);
const char* pasn_tuning_get(const char* name);
int pasn_tuning_report(char* buf, int cap, int with_registry);

/* Geometry of one convolution / pooling window over channels-last activations. */
typedef struct pasn_conv_desc {
    int32_t N, Ti, Hi, Wi;    /* input extent                                              */
    int32_t Cin, Cin_p;       /* input channels, input channel stride (elements)           */
    int32_t To, Ho, Wo;       /* output extent                                             */
    int32_t Cout, Cout_p;     /* output channels, output channel stride (elements)         */
    int32_t kt, kh, kw;       /* window                                                    */
    int32_t st, sh, sw;       /* stride                                                    */
    int32_t pt, ph, pw;       /* zero padding (max-pool: -inf padding)                     */
    int32_t act;              /* PASN_ACT_* applied after scale/bias (+ residual)          */
    int32_t in_swish;         /* conv3d: apply x*sigmoid(x) to the INPUT while loading it  */
    int32_t w_kc;             /* conv3d: per-tap K extent of the packed weight (elements)  */
    int32_t w_rows;           /* conv3d: rows of the packed weight / scale / bias arrays   */
    int32_t w_frag;           /* conv3d: 0 = w is [w_rows][taps][w_kc]; 1 = MFMA-fragment-major
                                 [w_rows/32][taps*w_kc/KSTEP][2][32][CH] (KSTEP/CH = 16/8 bf16, 8/4 fp32; K = (tap, channel)):
                                 only where pasn_conv3d_variant() reports 2500..5999 or >= 7000 */
} pasn_conv_desc;

/*
 * First layer: planar (N,3,T,H,W) clip -> channels-last activation, window (1,kh,kw), fused
 * per-channel scale/bias (folded eval-mode BatchNorm) and activation.
 * Replaces: resnet_features.py:203-205 (conv1+bn1+relu), torchvision R2Plus1dStem conv 0-2
 * (call site resnet_features.py:316-320), X3D stem conv_xy.
 *   x      : in_dtype  [N][3][Ti][Hi][Wi]
 *   w      : fp32 [3*kh*kw][Cout_p]  (tap-major, channel-minor; rows ordered ci, r, s)
 *   scale, bias : fp32 [Cout_p]
 *   y      : out_dtype [N][To][Ho][Wo][Cout_p]
 */
int pasn_first_conv_fwd(const void* x, const float* w, const float* scale, const float* bias, void* y,
                        const pasn_conv_desc* d, int in_dtype, int out_dtype, void* stream);

/*
 * Fused X3D stem: (1,3,3) stride-(1,2,2) conv 3->24 -> depthwise (5,1,1) temporal conv -> BN -> ReLU in one launch
 * (a thread marches along T with a 5-frame register ring; the 24-channel tensor between the two convs never reaches
 * HBM).  Bit-identical to pasn_first_conv_fwd (no norm, no activation) followed by pasn_dwconv3d_fwd.
 *   d    : geometry of the (1,3,3) conv as for pasn_first_conv_fwd; pasn_x3d_stem_supported(d) says whether it fits
 *   w_xy : fp32 [27][24] (rows ordered ci, r, s);  w_t : fp32 [5][24];  scale, bias : fp32 [24] (BN after the temporal conv)
 */
int pasn_x3d_stem_supported(const pasn_conv_desc* d);
int pasn_x3d_stem_fwd(const void* x, const float* w_xy, const float* w_t, const float* scale, const float* bias, void* y,
                      const pasn_conv_desc* d, int in_dtype, int out_dtype, void* stream);

/*
 * The same stem on the matrix cores, bf16 activations out, Wi % 4 == 0 (pasn_x3d_stem_mfma_supported says when): conv_xy and conv_t as
 * ONE linear map over 5 frames x Cin x 3 rows x 4-wide window slots, weights multiplied together by the caller:
 *   wq : bf16 [2*ceil(5*Cin*3/4)][32][8], K row R = (kt*Cin + ci)*3 + r:  wq[R/2][co][4*(R%2) + 1 + s] = w_t[co][kt] * w_xy[co][ci][r][s],
 *        zero elsewhere
 * d->Cin = 3 or 1 (grey clip, taps summed over the input channels); x' = x * in_a + in_b while staging (1, 0 = none).  A bf16 tolerance
 * path (no rounding of the 24-channel intermediate): fp32 activations keep pasn_x3d_stem_fwd.
 */
int pasn_x3d_stem_mfma_supported(const pasn_conv_desc* d, int in_dtype, int out_dtype);
int pasn_x3d_stem_mfma_fwd(const void* x, const void* wq, const float* scale, const float* bias, void* y, const pasn_conv_desc* d,
                           int in_dtype, float in_a, float in_b, void* stream);

/*
 * Device side of the input pipeline.  The reference dataloader resizes a single-channel cine on the host,
 * normalises it ((x - 0.099) / 0.171, as_dataloader.py:180-182), repeats it to 3 identical channels (:168-170) and ships fp32
 * (N,3,T,H,W).  These two entry points take the SINGLE channel instead -- planar [N][1][Ti][Hi][Wi], fp32 / bf16 / uint8 -- apply
 * x' = x * in_a + in_b while loading (in_a = 1/std or 1/(255 std), in_b = -mean/std; 1, 0 for an already normalised clip) and use
 * first-conv weights summed over the three input channels: w [kh*kw][Cout_p] / w_xy [9][24].  Zero padding pads the normalised
 * tensor, as in the reference.  Same outputs as the 3-channel entry points fed the expanded clip, up to fp32 summation order.
 * d->Cin must be 1.
 */
/*
 * The same first layer on the matrix cores, bf16 activations out: (1,kh,kw <= 7) windows, stride (1,2,2) -- the 7x7 stems of
 * R(2+1)D-18 and ResNet-18 (resnet_features.py:203-205, :316-320); d->Cin = 3 (the reference's clip) or 1 (grey clip, taps summed,
 * as for pasn_first_conv_gray_fwd).  Instances exist for ceil(Cin*kh/2) in {11, 5, 4, 2} (the 7x7 and 3x3 windows), kh >= 2.
 * pasn_first_conv_mfma_slot returns -1 when the layer is not covered (use pasn_first_conv_fwd / pasn_first_conv_gray_fwd), else
 * the slot o of tap 0 in the 8-wide window the weights must be laid out for:
 *   wq : bf16 [2*ceil(Cin*kh/2)][32*ceil(Cout_p/32)][8],  wq[ci*kh + r][co][o + s] = w[co][ci][r][s], zero elsewhere
 *   x' = x * in_a + in_b is applied while the clip is staged (1, 0 = none); zero padding pads the normalised tensor.
 */
int pasn_first_conv_mfma_slot(const pasn_conv_desc* d, int in_dtype, int out_dtype);
int pasn_first_conv_mfma_fwd(const void* x, const void* wq, const float* scale, const float* bias, void* y, const pasn_conv_desc* d,
                             int in_dtype, float in_a, float in_b, void* stream);
int pasn_first_conv_gray_fwd(const void* x, const float* w, const float* scale, const float* bias, void* y,
                             const pasn_conv_desc* d, int in_dtype, int out_dtype, float in_a, float in_b, void* stream);
int pasn_x3d_stem_gray_fwd(const void* x, const float* w_xy, const float* w_t, const float* scale, const float* bias, void* y,
                           const pasn_conv_desc* d, int in_dtype, int out_dtype, float in_a, float in_b, void* stream);

/*
 * Dense convolution as an implicit GEMM on the matrix cores (MFMA), channels-last, groups=1, any
 * window/stride/padding, fused epilogue  y = act(acc*scale + bias [+ residual]).
 * Optional fused input transform (X3D project conv): x' = swish(x * gate[n][ci]).
 * Replaces: every nn.Conv2d/Conv3d + BatchNorm (+ReLU, + residual add) of the trunks
 * (resnet_features.py:49-66,202-213; torchvision Conv2Plus1D/BasicBlock at :316-320), the 1x1(x1)
 * add-on convs of PPNet (ProtoPNet.py:117-130) and the X3D expand / project / shortcut convs.
 *   x     : dtype [N][Ti][Hi][Wi][Cin_p]
 *   w     : dtype [w_rows][kt*kh*kw][w_kc] (or fragment-major, see w_frag), zero padded (w_rows multiple of 128, w_kc multiple of
 *           16 (bf16) / 8 (fp32) and >= Cin_p)
 *   scale, bias : fp32 [w_rows]
 *   residual : dtype [N][To][Ho][Wo][Cout_p] or NULL
 *   gate  : fp32 [N][Cin_p] or NULL
 *   y     : dtype [N][To][Ho][Wo][Cout_p]
 */
int pasn_conv3d_fwd(const void* x, const void* w, const float* scale, const float* bias, const void* residual,
                    const float* gate, void* y, const pasn_conv_desc* d, int dtype, void* stream);
/*
 * Two chained 1x1x1 convs on the same positions (bf16): y1 = act1(scale1 * (w1 . x') + bias1 + residual) with the optional
 * fused input transform x' = swish(x * gate), then y2 = act2(scale2 * (w2 . y1) + bias2) computed from y1 while it is
 * still on chip (y1 is written too).  The X3D pattern: a block's project conv (ResBlock.conv_c + BN + residual + ReLU)
 * and the next block's expand conv (conv_a + BN + ReLU).  Both weights fragment-major (w_frag = 1).
 * pasn_conv3d_pair_supported() says whether the geometry is covered; otherwise call pasn_conv3d_fwd twice.
 */
int pasn_conv3d_pair_supported(const pasn_conv_desc* d1, const pasn_conv_desc* d2, int dtype);
/* Which kernel the pair takes: 0 none, 1 pwconv_xpair_kernel (a block per 64-position tile), 2 pwconv_ws_kernel in pair mode (persistent
 * blocks, both weight sets in registers).  flags bit 0: a gate tensor will be passed.  For profilers and benchmarks. */
int pasn_conv3d_pair_variant(const pasn_conv_desc* d1, const pasn_conv_desc* d2, int dtype, int flags);
/* The chained pair whose first conv's squeeze-excite gate is computed in the launch's prologue from the stencil's pool partial rows
 * (arguments as pasn_conv3d_se_fwd + pasn_conv3d_pair_fwd): stencil -> ONE launch -> next stencil for an X3D SE block that is followed by a
 * block without shortcut.  _supported() = 0: pasn_se_gate_fwd + pasn_conv3d_pair_fwd. */
int pasn_conv3d_pair_se_supported(const pasn_conv_desc* d1, const pasn_conv_desc* d2, int dtype, int Cse);
int pasn_conv3d_pair_se_fwd(const void* x, const void* w1, const float* scale1, const float* bias1, const void* residual,
                            const float* pool_partial, int pool_blocks, int positions, const float* fc1_w, const float* fc1_b,
                            const float* fc2_w, const float* fc2_b, int Cse, void* y1, const pasn_conv_desc* d1, const void* w2,
                            const float* scale2, const float* bias2, void* y2, const pasn_conv_desc* d2, int dtype, void* stream);
int pasn_conv3d_pair_fwd(const void* x, const void* w1, const float* scale1, const float* bias1, const void* residual,
                         const float* gate, void* y1, const pasn_conv_desc* d1, const void* w2, const float* scale2,
                         const float* bias2, void* y2, const pasn_conv_desc* d2, int dtype, void* stream);

/*
 * pasn_conv3d_fwd with the squeeze-excite gate of its input transform computed IN THE SAME LAUNCH (bf16, fragment-major weights): every
 * block derives the gate rows of the (at most two) clips its rows touch from the stencil's pool partial rows -- mean over positions,
 * fc1 + ReLU, fc2 + sigmoid, as pasn_se_gate_fwd -- while its first tiles are in flight, then x' = swish(x * gate) as usual.  Replaces the
 * stand-alone pasn_se_gate_fwd launch between the stencil and the project conv of an X3D SE block (and the gate tensor).
 *   pool_partial : fp32 [N][pool_blocks][Cin_p] (pasn_dwconv3d_fwd's partial sums), positions = T*H*W of the pooled tensor
 *   fc1_w : fp32 [Cse][Cin], fc1_b : [Cse], fc2_w : [Cin][Cse], fc2_b : [Cin];  d->in_swish says whether Swish follows the gate
 * _supported() = 0: call pasn_se_gate_fwd + pasn_conv3d_fwd.
 */
int pasn_conv3d_se_supported(const pasn_conv_desc* d, int dtype, int Cse, int has_residual);
int pasn_conv3d_se_fwd(const void* x, const void* w, const float* scale, const float* bias, const void* residual,
                       const float* pool_partial, int pool_blocks, int positions, const float* fc1_w, const float* fc1_b,
                       const float* fc2_w, const float* fc2_b, int Cse, void* y, const pasn_conv_desc* d, int dtype, void* stream);

/*
 * A 1x1x1 stride-1 conv + norm with the block's STRIDED 1x1x1 shortcut conv + norm accumulated in the same launch (bf16; the first
 * project conv of an X3D stage, whose residual is the strided shortcut of the block input):
 *     y = act(scale * (w . x') + scale2 * (w2 . x2[strided position]) + bias),   x' = swish(x * gate) as in pasn_conv3d_fwd,
 * bias = the two norms' shifts, summed by the caller.  d = the stride-1 conv, d2 = the shortcut conv (same N, To, Ho, Wo, Cout_p;
 * kt = kh = kw = 1, st = 1, any sh / sw; row-major weights).  Replaces the pair of launches pasn_conv3d_fwd(shortcut) ->
 * pasn_conv3d_fwd(project, residual = shortcut) and the shortcut tensor between them.  _supported() = 0: use that pair.
 */
int pasn_conv3d_short_supported(const pasn_conv_desc* d, const pasn_conv_desc* d2, int dtype);
int pasn_conv3d_short_fwd(const void* x, const void* w, const float* scale, const float* bias, const float* gate, const void* x2,
                          const void* w2, const float* scale2, void* y, const pasn_conv_desc* d, const pasn_conv_desc* d2, int dtype,
                          void* stream);

/*
 * Which kernel instance a fused launch runs, read from the geometry its launch reads (host only, nothing is launched; the arguments are
 * those of the matching _supported() probe).  0 = not covered.
 *   pasn_conv3d_se_variant       7000 + KS*10 + MT            pwconv_ws_kernel<KS, MT, true, residual>[se]     (pasn_conv3d_se_fwd)
 *   pasn_conv3d_short_variant    KS*100 + NT*10 + KS2         pwconv_persist_kernel<bf16, KS, NT, false, KS2>  (pasn_conv3d_short_fwd)
 *   pasn_conv3d_pair_instance    arm*10000 + KS1*100 + KS2    arm = pasn_conv3d_pair_variant's answer: 1 pwconv_xpair_kernel<KS1, KS2, transform>,
 *                                                             2 pwconv_ws_kernel<KS1, 1, transform, true, KS2>  (pasn_conv3d_pair_fwd; flags as there)
 *   pasn_conv3d_pair_se_variant  20000 + KS1*100 + KS2        pwconv_ws_kernel<KS1, 1, true, true, KS2>[se]     (pasn_conv3d_pair_se_fwd)
 *   pasn_x3d_pe_variant          KSC*1000 + KSA*10 + MT       x3d_pe_kernel<KSC, KSA, gate, MT>                 (pasn_x3d_pe_fwd; MT: PASN_PE_MT)
 *   pasn_x3d_edp_variant         KSA*100 + KSC                x3d_edp_kernel<KSA, KSC, next expand>             (pasn_x3d_edp_fwd)
 */
int pasn_conv3d_se_variant(const pasn_conv_desc* d, int dtype, int Cse, int has_residual);
int pasn_conv3d_short_variant(const pasn_conv_desc* d, const pasn_conv_desc* d2, int dtype);
int pasn_conv3d_pair_instance(const pasn_conv_desc* d1, const pasn_conv_desc* d2, int dtype, int flags);
int pasn_conv3d_pair_se_variant(const pasn_conv_desc* d1, const pasn_conv_desc* d2, int dtype, int Cse);
int pasn_x3d_pe_variant(const pasn_conv_desc* d1, const pasn_conv_desc* d2, int dtype, int Cse);
int pasn_x3d_edp_variant(const pasn_conv_desc* d_a, const pasn_conv_desc* d_dw, const pasn_conv_desc* d_c, const pasn_conv_desc* d_n, int dtype);

/* Which kernel instance pasn_conv3d_fwd picks for this geometry: 1000 + KS*10 + NT = pwconv_persist_kernel<dtype, KS, NT>
 * (1x1x1 stride-1 convs whose weights fit 64 VGPRs per lane); 2500 + 2*KS (+1 with in_swish) = pwconv_xtile_kernel<dtype, KS, ..>
 * (1x1x1 stride-1 convs with Cin_p >= 64: whole-K position tiles in LDS); 2000 / 2001 = gemm_conv_kernel<dtype, pointwise /
 * windowed> (LDS-tiled implicit GEMM); otherwise NT*10 + MT = conv3d_mfma_kernel<dtype, NT, MT> (output-channel /
 * position tiles per wave); 7000 + KS*10 + MT = pwconv_ws_kernel<KS, MT, ..> (bf16 1x1x1 stride-1 convs with Cin_p >= 48:
 * weight-stationary persistent blocks, LDS-DMA stage ring; fragment-major weights like 2500+); 9000 + KSF = tconv_ws_kernel<KSF, ..>
 * (bf16 (3,1,1) stride-1 convs with Cin_p = 16 KSF in {48, 64, 144} and up to 64 output channels -- torchvision's Conv2Plus1D temporal half as
 * resnet_features.py's r2plus1d_18 trunk instantiates it: weight-stationary, T-marching LDS ring; fragment-major weights over K = 3 Cin_p);
 * 0 on a bad descriptor.
 * flags: bit 0 = `gate` will be non-NULL, bit 1 = `residual` will be non-NULL (the choice between the pointwise kernels and
 * their tile sizes depend on both).  For profilers, benchmarks and the weight packing (w_frag). */
int pasn_conv3d_variant(const pasn_conv_desc* d, int dtype, int flags);

/*
 * Depthwise convolution (groups = C), channels-last, fused scale/bias/activation; optionally also
 * emits per-block partial channel sums of the (pre-activation) output for the squeeze-excite pool.
 * Replaces: X3D stem conv_t + BN + ReLU and X3D conv_b + BN (+Swish); HBM-bound stencil.
 *   w     : fp32 [kt*kh*kw][Cp]
 *   pool_partial : fp32 [N][pool_blocks][Cp] or NULL; pool_blocks = pasn_dwconv3d_pool_blocks(d, dtype)
 */
int pasn_dwconv3d_pool_blocks(const pasn_conv_desc* d, int dtype);
/* Kernel instance for this geometry: 3000 + WT*10 + SW = dwconv3d_march_kernel<SW, WT> (bf16, 3x3x3, stride (1,s,s));
 * WT*100 + KW*10 + SW = dwconv3d_strip_kernel<dtype, WT, KW, SW>; 50001 = dwconv3d_mfma_kernel (stride-1 3x3x3 on the matrix cores);
 * 60001 = dwconv3d_tz_kernel (stride-1 3x3x3, planes 9 .. 14 wide: Toeplitz form); 70000 + kt = dwconv_t_kernel<dtype, kt> ((kt,1,1),
 * kt = 3 / 5, stride 1, taken when pool_partial is NULL: the X3D stem's conv_t as a launch of its own); 0 = generic kernel. */
int pasn_dwconv3d_variant(const pasn_conv_desc* d, int dtype);
/* The instance of the launch WITH pool partial rows (pool_partial != NULL), same codes: differs from pasn_dwconv3d_variant only on the
 * (kt,1,1) layers, which the strip kernel <dtype, WT, 1, 1> runs then (dwconv_t_kernel writes no pool rows). */
int pasn_dwconv3d_pool_variant(const pasn_conv_desc* d, int dtype);
/* The same stencil with the squeeze-excite gate of the block fused into the launch (X3D conv_b + SE: global average pool ->
 * fc1 + ReLU -> fc2 + sigmoid): every block writes its pool partial row, the clip's last-arriving block reduces them and computes
 * gate[n][:].  Same results as pasn_dwconv3d_fwd followed by pasn_se_gate_fwd up to fp32 summation order (fixed: repeat runs are
 * bitwise equal).  counter: int32 [N], zero before the FIRST launch (the kernel leaves it zero).  Supported only where
 * pasn_dwconv3d_se_supported returns 1 (bf16 3x3x3 layers on the T-marching kernel). */
int pasn_dwconv3d_se_supported(const pasn_conv_desc* d, int dtype, int Cse);
int pasn_dwconv3d_se_pool_blocks(const pasn_conv_desc* d, int dtype); /* rows of pool_partial per clip for pasn_dwconv3d_se_fwd */
int pasn_dwconv3d_se_fwd(const void* x, const float* w, const float* scale, const float* bias, void* y, float* pool_partial,
                         const pasn_conv_desc* d, int dtype, const float* fc1_w, const float* fc1_b, const float* fc2_w,
                         const float* fc2_b, int Cse, float* gate, int32_t* counter, void* stream);
int pasn_dwconv3d_fwd(const void* x, const float* w, const float* scale, const float* bias, void* y,
                      float* pool_partial, const pasn_conv_desc* d, int dtype, void* stream);

/*
 * Squeeze-excite gate: mean over positions (from the partial sums above, fixed summation order),
 * fc1 + ReLU, fc2 + sigmoid.   gate : fp32 [N][Cp].
 *   w1 : fp32 [Cse][C], b1 : fp32 [Cse], w2 : fp32 [C][Cse], b2 : fp32 [C]
 */
int pasn_se_gate_fwd(const float* pool_partial, int pool_blocks, int positions, const float* w1, const float* b1,
                     const float* w2, const float* b2, float* gate, int N, int C, int Cp, int Cse, void* stream);

/* Max pooling, channels-last.  Replaces nn.MaxPool2d(3,2,1) at resnet_features.py:206. */
int pasn_maxpool3d_fwd(const void* x, void* y, const pasn_conv_desc* d, int dtype, void* stream);

/*
 * Head A -- PPNet prototype layer.  Replaces PPNet._l2_convolution (ProtoPNet.py:189-207: the ones-conv
 * for ||x||^2, the prototype conv for x.p, relu), the global min pooling + distance_2_similarity + last_layer
 * of PPNet.forward (ProtoPNet.py:236-241), and the distance map of push_forward (ProtoPNet.py:245-249).
 *   z        : dtype [N][S][Dp]      add-on output (after Sigmoid), channels-last
 *   protos   : fp32 [P][D]
 *   fc_w     : fp32 [K][P]           last_layer.weight
 *   dist     : fp32 [N][P][S] or NULL  (full map, planar like the reference's (N,P,H,W))
 *   min_dist : fp32 [N][P]
 *   argmin   : int32 [N][P] or NULL  first s attaining the minimum
 *   logits   : fp32 [N][K]
 *   activation: 0 = log((d+1)/(d+eps)), 1 = linear (-d)
 */
int pasn_l2_head_fwd(const void* z, const float* protos, const float* fc_w, float* dist, float* min_dist,
                     int32_t* argmin, float* logits, int N, int S, int D, int Dp, int P, int K, int dtype,
                     int activation, float eps, void* stream);

/*
 * Head B -- XProtoNet / Video_XProtoNet ("ProtoASNet") prototype layer: add-on convs, occurrence module + abs,
 * occurrence-weighted pooling WITHOUT materialising the (N,P,D,S) broadcast product of Video_XProtoNet.py:87 /
 * XProtoNet.py:56, cosine similarity (torch semantics: each vector divided by max(norm, 1e-8) first), (s+1)/2,
 * last layer.  Replaces everything after the trunk in Video_XProtoNet.forward / push_forward
 * (Video_XProtoNet.py:82-130), XProtoNet.forward / push_forward (XProtoNet.py:51-106) and, with mode = 1,
 * the head part of compute_occurence_map (Video_XProtoNet.py:100-109, XProtoNet.py:69-85).
 *   x      : dtype [N][S][Cbp]  trunk features, channels-last
 *   a1,a2  : add_on_layers.{0,2}.weight;  o1,o2,o3 : occurrence_module.{0,2,4}.weight -- each packed like a
 *            pasn_conv3d_fwd weight with one tap: dtype [round_up(Cout_p,128)][round_up(Cin_p, 16|8)], zero padded
 *   a1b,a2b,o1b,o2b : fp32 biases [round_up(Cout_p,128)], zero padded (o3 has no bias)
 *   protos : fp32 [P][D];  fc_w : fp32 [K][P]
 *   occ    : fp32 [N][P][S]   planar, i.e. the reference's (N,P,1,[T,]H,W)
 *   feat   : fp32 [N][P][D]   features_extracted;   sim : fp32 [N][P];   logits : fp32 [N][K]
 *   ws     : workspace of pasn_xproto_head_workspace_bytes() bytes, 256-byte aligned
 *   mode   : 0 = full forward, 1 = occurrence map only (feat / sim / logits may be NULL)
 */
typedef struct pasn_xproto_desc {
    int32_t N, S;
    int32_t Cb, Cbp;   /* trunk channels and channel stride        */
    int32_t D, Dp;     /* prototype depth, round_up(D, 8)          */
    int32_t Hd, Hp;    /* D / 2 (hidden width of the occurrence module), round_up(Hd, 8) */
    int32_t P, Pp;     /* prototypes, round_up(P, 8)               */
    int32_t K;         /* classes                                   */
    int32_t mode;
} pasn_xproto_desc;

/*
 * Front half of an X3D stage's first block in ONE launch (bf16): conv_a (1x1x1) + norm_a + ReLU -> conv_b (depthwise 3x3x3, stride
 * (1,2,2), pad 1) + norm_b (+ the descriptor's activation, + squeeze-excite pool partial rows), pytorchvideo's BottleneckTransform as
 * instantiated by the reference's x3d trunks; replaces pasn_conv3d_fwd + pasn_dwconv3d_fwd for that pair -- the expanded activation (2.25x
 * the block width at the input resolution) stays in LDS.
 *   x  : block input, channels-last [N][T][H][W][de->Cin_p];   y : [N][T][Ho][Wo][d->Cout_p]
 *   wa : conv_a weights FRAGMENT-MAJOR (w_frag = 1), scale_a / bias_a: folded norm_a [de->w_rows] (zero beyond the channels).
 *        scale_a == NULL: the caller has folded norm_a's scale into wa (W * scale, rounded to bf16 once); bias_a then initialises the
 *        fp32 accumulators and the expand epilogue is ReLU + rounding only (what the plan compiler passes)
 *   w  : conv_b weights fp32 [27][Cp], scale / bias: folded norm_b [Cp]
 *   pool_partial : NULL or fp32 [N][pasn_x3d_expdw_pool_blocks()][Cp] (sums of the pre-activation output over positions, fixed order)
 * _supported() == 0: issue the two launches.
 */
int pasn_x3d_expdw_supported(const pasn_conv_desc* de, const pasn_conv_desc* d, int dtype);
int pasn_x3d_expdw_pool_blocks(const pasn_conv_desc* de, const pasn_conv_desc* d, int dtype);
/* which kernel pasn_x3d_expdw_fwd runs for the pair: 0 = block-diagonal stencil operands (x3d_expdw.hip), 1 = per-channel Toeplitz operands on a
 * channel-planar image (x3d_expdw_tz.hip, stride 1, round 5), -1 = pair not covered.  Same arguments, same results up to fp32 summation order. */
int pasn_x3d_expdw_variant(const pasn_conv_desc* de, const pasn_conv_desc* d, int dtype);
int pasn_x3d_expdw_fwd(const void* x, const void* wa, const float* scale_a, const float* bias_a, const float* w, const float* scale,
                       const float* bias, void* y, float* pool_partial, const pasn_conv_desc* de, const pasn_conv_desc* d, int dtype,
                       void* stream);

/*
 * A WHOLE X3D residual block without squeeze-excite on 7 x 7 planes (the last stage: block width 192, inner width 432) in ONE launch (bf16):
 * conv_a (1x1x1) + norm_a + ReLU -> conv_b (depthwise 3x3x3, pad 1) + norm_b + Swish -> conv_c (1x1x1) + norm_c + x + ReLU, optionally followed by
 * the NEXT block's conv_a + norm_a + ReLU (pytorchvideo's ResBlock / BottleneckTransform as the x3d trunks instantiate them).  Replaces
 * pasn_conv3d_fwd + pasn_dwconv3d_fwd + pasn_conv3d_fwd (/ pasn_x3d_pe_fwd): the expanded activation and the stencil's output exist only as LDS
 * images of a (clip, two frames) tile; results are bit-identical to those launches.
 *   x        : block input = residual, channels-last [N][T][7][7][d_a->Cin_p];   y : block output, same shape
 *   w_a, w_c : fragment-major (w_frag = 1); d_a->w_kc = Cin_p, d_c->w_kc = 32 * ceil(Cin_p / 32) (K zero-padded to an even number of steps)
 *   w_dw     : conv_b weights as the stencil's matrix-core operands: uint16 [ceil(Cp / 16)][2][64][8], row (16-channel tile, half, lane):
 *              entry e = kt * 5 + j (half e >> 3, slot e & 7; entry 15 unused) = bf16 bits (round-to-nearest-even) of tap
 *              kt * 9 + 2 j + (lane >> 5) of channel 16 tile + (lane & 15), for lanes with ((lane >> 3) & 1) == ((lane >> 4) & 1), a tap index
 *              < 9 and a real channel; 0 otherwise -- the one possibly nonzero element per lane of the block-diagonal A operands that
 *              pasn_dwconv3d_fwd's matrix-core kernel builds in its own prologue; scale / bias: the folded norms
 *   w_n ...  : the next block's conv_a in w_a's form and its output e_next [N][T][7][7][d_n->Cout_p]; all NULL (with d_n == NULL): none
 * _supported() == 0: issue the separate launches.
 */
int pasn_x3d_edp_supported(const pasn_conv_desc* d_a, const pasn_conv_desc* d_dw, const pasn_conv_desc* d_c, const pasn_conv_desc* d_n, int dtype);
int pasn_x3d_edp_fwd(const void* x, const void* w_a, const float* scale_a, const float* bias_a, const void* w_dw, const float* scale_dw,
                     const float* bias_dw, const void* w_c, const float* scale_c, const float* bias_c, void* y, const void* w_n,
                     const float* scale_n, const float* bias_n, void* e_next, const pasn_conv_desc* d_a, const pasn_conv_desc* d_dw,
                     const pasn_conv_desc* d_c, const pasn_conv_desc* d_n, int dtype, void* stream);

/*
 * An X3D block's conv_c (1x1x1) + norm_c + residual + ReLU chained with the NEXT block's conv_a (1x1x1) + norm_a + ReLU in ONE launch for the
 * 432-channel stage (bf16; inner width 432 -> block width 192 -> 432), with the block's squeeze-excite gate -- when it has one -- computed in the
 * launch's prologue from the stencil's pool partial rows: same contract and results (bit-identical) as pasn_conv3d_pair_se_fwd /
 * pasn_conv3d_pair_fwd, which do not cover this width (both weight sets do not fit a wave's registers); the weights are streamed per row tile
 * instead.  Differences in the operands: w1 is fragment-major with K zero-padded to an EVEN number of 16-wide steps (d1->w_kc = 32 *
 * ceil(Cin_p / 32)); pool_partial == NULL (with Cse = 0): no gate, x is the block's final stencil output (d1->in_swish = 0).
 * _supported() == 0: issue the separate launches.
 */
int pasn_x3d_pe_supported(const pasn_conv_desc* d1, const pasn_conv_desc* d2, int dtype, int Cse);
int pasn_x3d_pe_fwd(const void* x, const void* w1, const float* scale1, const float* bias1, const void* residual, const float* pool_partial,
                    int pool_blocks, int positions, const float* fc1_w, const float* fc1_b, const float* fc2_w, const float* fc2_b, int Cse,
                    void* y1, const pasn_conv_desc* d1, const void* w2, const float* scale2, const float* bias2, void* y2,
                    const pasn_conv_desc* d2, int dtype, void* stream);



int pasn_xproto_head_splits(const pasn_xproto_desc* d);
size_t pasn_xproto_head_workspace_bytes(const pasn_xproto_desc* d, int dtype);
int pasn_xproto_head_fwd(const void* x, const void* a1, const float* a1b, const void* a2, const float* a2b,
                         const void* o1, const float* o1b, const void* o2, const float* o2b, const void* o3,
                         const float* protos, const float* fc_w, float* occ, float* feat, float* sim, float* logits,
                         void* ws, const pasn_xproto_desc* d, int dtype, void* stream);

/*
 * Head B in two launches (csrc/head_chain.hip + the finish kernel): same contract and outputs as pasn_xproto_head_fwd (replaces
 * Video_XProtoNet.forward, Video_XProtoNet.py:66-98, after the trunk), for bf16 with D = 256, Hd = 128, P <= 64 and a trunk channel
 * stride <= 256 (the X3D heads of BASELINE configs 2, 3 and 5; the reference's own R(2+1)D-18[:-3] video trunk).  A block keeps a tile of <= 104 positions of one clip in LDS through the
 * five convs and adds the tile's share of the occurrence-weighted pooling; no intermediate map reaches memory.
 *   a1 .. o3 : conv weights FRAGMENT-MAJOR, [rows / 32][kc / 16][64][8] bf16 (the w_frag = 1 layout of pasn_conv3d_fwd)
 *   ws       : pasn_xproto_chain_workspace_bytes() bytes, 256-byte aligned (the pooling slabs [N][tiles][P][D] fp32; mode 1: unused)
 * pasn_xproto_chain_supported() == 0: use pasn_xproto_head_fwd.
 */
int pasn_xproto_chain_supported(const pasn_xproto_desc* d, int dtype);
size_t pasn_xproto_chain_workspace_bytes(const pasn_xproto_desc* d);
int pasn_xproto_chain_fwd(const void* x, const void* a1, const float* a1b, const void* a2, const float* a2b,
                          const void* o1, const float* o1b, const void* o2, const float* o2b, const void* o3,
                          const float* protos, const float* fc_w, float* occ, float* feat, float* sim, float* logits,
                          void* ws, const pasn_xproto_desc* d, int dtype, void* stream);

/*
 * Push sweep, XProtoNet / Video rule (push_abs_revision.py:288-307): per prototype j, over the clips of
 * this batch whose label matches class(j) (or all clips when class_mask[j] == 0): batch min of
 * proto_dist[:, j], first index; accepted when min <= best (a later batch wins ties).  State stays on the device.
 *   proto_dist : fp32 [B][P]   (1 - similarity)
 *   feat       : fp32 [B][P][D]
 *   labels     : int64 [B]
 *   proto_class: int32 [P]     argmax of prototype_class_identity
 *   class_mask : int32 [P]     1 = class specific
 *   best_dist  : fp32 [P]  (init +inf);  best_index : int64 [P] (init -1; global clip index = index_base + b)
 *   best_feat  : fp32 [P][D]
 */
int pasn_push_xproto_update(const float* proto_dist, const float* feat, const int64_t* labels, const int32_t* proto_class,
                            const int32_t* class_mask, float* best_dist, int64_t* best_index, float* best_feat, int B, int P,
                            int D, int64_t index_base, void* stream);

/*
 * Push sweep, PPNet rule (push_ProtoPNet.py:198-235): per prototype j, argmin over the flattened (n_c,h,w) of the
 * distance map restricted to images of class(j) (all images when class_specific == 0); accepted on strict '<'
 * (the first batch wins ties); the winning 1x1 patch of the add-on output is copied.
 *   dist : fp32 [B][P][S];  z : dtype [B][S][Dp] channels-last add-on output
 *   best_dist fp32 [P] (+inf), best_index int64 [P][2] = (global image index, s) (-1), best_patch fp32 [P][D]
 */
int pasn_push_ppnet_update(const float* dist, const void* z, const int64_t* labels, const int32_t* proto_class,
                           int class_specific, float* best_dist, int64_t* best_index, float* best_patch, int B, int P, int S,
                           int D, int Dp, int dtype, int64_t index_base, void* stream);

/* =====================================================================================================================
 * Training path (train-mode forward with batch statistics + backward).  The reference trains through the same modules
 * (`loss.backward()` through forward / compute_occurence_map: Video_XProtoNet_e2e.py:118-141, XProtoNet_e2e.py); these
 * entry points are what an autograd.Function under that nn.Module surface calls.  A conv + norm + activation "unit" is
 *     y = conv(x)            (pasn_conv3d_fwd / pasn_dwconv3d_fwd / pasn_first_conv_fwd with scale = 1, bias = 0, no activation)
 *     stat = batch statistics of y                                                        (pasn_bn_stats_fwd)
 *     a = act((y * sc + sh + residual) * gate)                                            (pasn_affine_act_fwd)
 * and its backward is pasn_unit_bwd_reduce (+ pasn_bn_bwd_apply), the conv's dgrad (the forward conv kernels with the
 * transposed weight, pasn_scatter_strided for strided 1x1x1 convs, pasn_dwconv3d_dgrad) and its wgrad
 * (pasn_conv3d_wgrad / pasn_first_conv_wgrad / pasn_dwconv3d_wgrad).  Tensors are channels-last rows [N][S][Cp] in `dtype`;
 * statistics, reductions and parameter gradients are fp32; every reduction except the split-K of pasn_conv3d_wgrad /
 * pasn_first_conv_wgrad (fp32 atomics) has a fixed summation order.
 * ===================================================================================================================== */

/* Row chunks per clip used by the reduction passes below: their `ws` is fp32 [N][chunks][2][Cp]. */
int pasn_train_chunks(int N, int S, int Cp);

/* torch.nn.BatchNorm{2,3}d, training=True (resnet_features.py:140,180; every norm layer of the trunks): per-channel batch
 * mean / biased variance of y, running-estimate update (unbiased variance, `momentum`), and the affine folded to
 *   stat : fp32 [4][Cp] = (mean, invstd, sc = gamma*invstd, sh = beta - mean*sc)        (channels >= C: zeros)
 *   pool_u : fp32 [N][Cp] or NULL -- per-clip mean over positions of y*sc + sh (the squeeze-excite pool)
 *   gamma / beta / running_* : fp32 [C] or NULL */
int pasn_bn_stats_fwd(const void* y, float* ws, const float* gamma, const float* beta, float* running_mean, float* running_var,
                      float momentum, float eps, float* stat, float* pool_u, int N, int S, int C, int Cp, int dtype, void* stream);

/* Squeeze-excite unit backward in ONE pass over (d, y) -- the analytic form of modes 1 + 2:
 *   pasn_unit_bwd_reduce(mode 4, ...): d <- d' = d * act'((y*sc + sh) * gate); ws fp32 [N][chunks][3][Cp] = per-clip partials of
 *       (sum d', sum d' yhat, sum yhat)            (gate required; coef / dgamma / dbeta unused)
 *   pasn_se_gate_bwd_stat: the gate's gradient sum d' u = gamma sum d' yhat + beta sum d' per clip, the two FCs' backward (add[n][c],
 *       parameter gradients, as pasn_se_gate_bwd) and, because d'' = d' gate + add is affine in d' per clip, the norm's
 *       coef = (sum d'' / R, sum d'' yhat / R), dgamma, dbeta WITHOUT a second pass over the tensor (ws is updated in place)
 *   pasn_bn_bwd_apply_se: dy = sc (d' gate + add - m1 - yhat m2), d'' formed on the fly (dy may alias d).
 * Same arithmetic as modes 1 + 2 + pasn_bn_bwd_apply up to fp32 summation order; fixed order. */
int pasn_se_gate_bwd_stat(float* ws3, const float* pool_u, const float* stat, const float* gate, const float* fc1_w, const float* fc1_b,
                          const float* fc2_w, const float* fc2_b, float* add, float* pn, float* dfc1_w, float* dfc1_b, float* dfc2_w,
                          float* dfc2_b, float* coef, float* dgamma, float* dbeta, int N, int S, int C, int Cp, int Cse, void* stream);
int pasn_bn_bwd_apply_se(const void* d, const void* y, const float* stat, const float* coef, const float* gate, const float* add, void* dy,
                         int N, int S, int C, int Cp, int dtype, void* stream);

/* Depthwise conv (raw output, as pasn_dwconv3d_fwd with pool_partial = NULL) AND the batch statistics of its output in one pass over
 * y: replaces pasn_dwconv3d_fwd + pasn_bn_stats_fwd for the X3D conv_b units (Video_XProtoNet trunks: every block's 3x3x3 depthwise conv
 * is followed by a BatchNorm3d).  `ws` is fp32 [N][rows][2][Cp] with rows = pasn_dwconv3d_stats_rows(d, dtype); rows = 0: the layer is
 * not covered (caller issues the two separate calls).  Statistics are taken from the fp32 outputs before they are rounded to `dtype`;
 * fixed summation order.  scale / bias: per-channel epilogue constants of the stencil (1 and 0 for a BatchNorm'd unit). */
int pasn_dwconv3d_stats_rows(const pasn_conv_desc* d, int dtype);
int pasn_dwconv3d_stats_fwd(const void* x, const float* w, const float* scale, const float* bias, void* y, float* ws, const float* gamma,
                            const float* beta, float* running_mean, float* running_var, float momentum, float eps, float* stat, float* pool_u,
                            const pasn_conv_desc* d, int dtype, void* stream);

/* dx of a stride-1 "same" depthwise conv (dy correlated with the reversed taps `w_flipped`, the forward stencil) AND, from the same fp32
 * outputs, the backward sums of the unit that produced the conv's input x = act_prev(y_prev * sc + sh): coef = (sum d' / R, sum d' yhat / R),
 * dgamma, dbeta with d' = dx * act_prev'(.) -- what pasn_unit_bwd_reduce(mode 3) would compute from (dx, y_prev) in a second pass.  The
 * caller then runs pasn_bn_bwd_apply(dx, y_prev, stat_prev, coef, ..., act_prev) as after mode 3.  Only when dx is that unit's WHOLE output
 * gradient (one consumer).  `ws`: fp32 [N][rows][2][Cp], rows = pasn_dwconv3d_dgrad_reduce_rows(d, dtype) (0: not covered). */
int pasn_dwconv3d_dgrad_reduce_rows(const pasn_conv_desc* d, int dtype);
int pasn_dwconv3d_dgrad_reduce(const void* dy, const float* w_flipped, const float* scale, const float* bias, void* dx, const void* y_prev,
                               const float* stat_prev, int act_prev, float* ws, float* coef, float* dgamma, float* dbeta,
                               const pasn_conv_desc* d, int dtype, void* stream);

/* a = act((y*sc + sh + residual) * gate[n][c]);  residual (dtype [N][S][Cp]) and gate (fp32 [N][Cp]) may be NULL.
 * A unit without a norm layer passes stat = (0, 1, 1, bias). */
int pasn_affine_act_fwd(const void* y, const float* stat, const void* residual, const float* gate, void* a, int N, int S, int C, int Cp,
                        int act, int dtype, void* stream);

/* One backward pass over a unit, IN PLACE on d (the gradient w.r.t. the unit's output a):
 *   mode 0:  d <- d * act'(y*sc + sh + residual);   coef = (sum d / R, sum d*yhat / R), dgamma = sum d*yhat, dbeta = sum d
 *   mode 1:  d <- d * act'((y*sc + sh) * gate);     ws partials of sum_s d*(y*sc + sh) per clip (gradient of the gate)
 *   mode 2:  d <- d * gate + add[n][c];             coef / dgamma / dbeta as mode 0
 *   mode 3:  the sums of mode 0 WITHOUT writing d back (no residual branch needs it): pasn_bn_bwd_apply is then called with
 *            the unit's `act` and differentiates on the fly -- one tensor write less per unit
 *   mode 4:  mode 1 with the per-clip sums of the analytic squeeze-excite backward (pasn_se_gate_bwd_stat below); ws is [N][chunks][3][Cp]
 * (yhat = (y - mean) * invstd, R = N*S; after mode 0 the buffer d is also the gradient of `residual`.) */
int pasn_unit_bwd_reduce(int mode, void* d, const void* y, const float* stat, const void* residual, const float* gate, const float* add,
                         float* ws, float* coef, float* dgamma, float* dbeta, int N, int S, int C, int Cp, int act, int dtype, void* stream);

/* Batch-norm input gradient: dy = sc * (d' - coef[0] - yhat * coef[1]) with d' = d (act = PASN_ACT_NONE: d was differentiated in
 * place by mode 0 / 2) or d' = d * act'(y*sc + sh) (after mode 3);  dy may alias d. */
int pasn_bn_bwd_apply(const void* d, const void* y, const float* stat, const float* coef, void* dy, int N, int S, int C, int Cp, int act,
                      int dtype, void* stream);

/* Statistics GROUPS (round 4).  The `_g` forms of the entry points above take `groups`: the batch is `groups` runs of N / groups consecutive
 * clips, each normalised with its OWN batch statistics -- stat is [groups][4][Cp], coef [groups][2][Cp]; the running estimates are updated
 * group by group in order (num_batches_tracked is the caller's: + groups); dgamma / dbeta are the parameter's (summed over the groups).
 * groups = 2 runs the two trunk passes of the reference's loss recipe (model(x), then model.compute_occurence_map(warp(x)): loss.py:302)
 * as ONE pass over [clips, warped clips] with exactly the statistics two passes would have used.  groups = 1 == the plain entry point.
 * 1 <= groups <= 4, N % groups == 0. */
int pasn_bn_stats_fwd_g(const void* y, float* ws, const float* gamma, const float* beta, float* running_mean, float* running_var,
                        float momentum, float eps, float* stat, float* pool_u, int N, int S, int C, int Cp, int dtype, int groups, void* stream);
int pasn_dwconv3d_stats_fwd_g(const void* x, const float* w, const float* scale, const float* bias, void* y, float* ws, const float* gamma,
                              const float* beta, float* running_mean, float* running_var, float momentum, float eps, float* stat, float* pool_u,
                              const pasn_conv_desc* d, int dtype, int groups, void* stream);
int pasn_affine_act_fwd_g(const void* y, const float* stat, const void* residual, const float* gate, void* a, int N, int S, int C, int Cp,
                          int act, int dtype, int groups, void* stream);
int pasn_unit_bwd_reduce_g(int mode, void* d, const void* y, const float* stat, const void* residual, const float* gate, const float* add,
                           float* ws, float* coef, float* dgamma, float* dbeta, int N, int S, int C, int Cp, int act, int dtype, int groups,
                           void* stream);
int pasn_bn_bwd_apply_g(const void* d, const void* y, const float* stat, const float* coef, void* dy, int N, int S, int C, int Cp, int act,
                        int dtype, int groups, void* stream);
int pasn_se_gate_bwd_stat_g(float* ws3, const float* pool_u, const float* stat, const float* gate, const float* fc1_w, const float* fc1_b,
                            const float* fc2_w, const float* fc2_b, float* add, float* pn, float* dfc1_w, float* dfc1_b, float* dfc2_w,
                            float* dfc2_b, float* coef, float* dgamma, float* dbeta, int N, int S, int C, int Cp, int Cse, int groups,
                            void* stream);
int pasn_bn_bwd_apply_se_g(const void* d, const void* y, const float* stat, const float* coef, const float* gate, const float* add, void* dy,
                           int N, int S, int C, int Cp, int dtype, int groups, void* stream);

/* Squeeze-excite backward: from the mode-1 partials `ws` and the pooled input `pool_u`, through sigmoid / fc2 / ReLU / fc1:
 *   add : fp32 [N][Cp] = dpool / S (the term mode 2 adds);  dw1 [Cse][C], db1 [Cse], dw2 [C][Cse], db2 [C]
 *   pn  : workspace of pasn_se_bwd_workspace_floats(N, C, Cse) floats */
size_t pasn_se_bwd_workspace_floats(int N, int C, int Cse);
int pasn_se_gate_bwd(const float* ws, const float* pool_u, const float* w1, const float* b1, const float* w2, const float* b2, float* add,
                     float* pn, float* dw1, float* db1, float* dw2, float* db2, int N, int S, int C, int Cp, int Cse, void* stream);

/* dst[n][t*st][h*sh][w*sw][:] (+)= src[n][t][h][w][:] with src [N][To][Ho][Wo][Cin_p], dst [N][Ti][Hi][Wi][Cin_p]; without
 * `accumulate` every other element of dst is zeroed (the input gradient of a strided 1x1x1 conv; zero insertion). */
int pasn_scatter_strided(const void* src, void* dst, const pasn_conv_desc* d, int accumulate, int dtype, void* stream);
int pasn_add_inplace(void* a, const void* b, size_t elements, int dtype, void* stream);
/* Max-pool backward (resnet_features.py:206 in training): dx receives dy of every window whose first maximum (scan order t, h, w:
 * the index torch records) the element is; x is the pooling INPUT, d the forward descriptor. */
int pasn_maxpool3d_bwd(const void* x, const void* dy, void* dx, const pasn_conv_desc* d, int dtype, void* stream);

/* Weight gradients.  dw is fp32 in the PARAMETER layout and must be zeroed by the caller for the two MFMA kernels:
 *   pasn_conv3d_wgrad      dw [Cout][Cin][kt*kh*kw]  += sum_rows dy[row][co] * x[in(row, tap)][ci]
 *   pasn_first_conv_wgrad  dw [Cout][3][kh*kw]       (x planar in_dtype [N][3][T][Hi][Wi])
 *   pasn_dwconv3d_wgrad    dw [C][kt*kh*kw]          (kh*kw <= 9; ws of pasn_dwconv3d_wgrad_workspace_floats(d) floats)
 * pasn_dwconv3d_dgrad: dx[n,ti,hi,wi,c] = sum_taps dy[n,to,ho,wo,c] * w[tap][c], w fp32 [taps][Cp] as for pasn_dwconv3d_fwd. */
int pasn_conv3d_wgrad(const void* x, const void* dy, float* dw, const pasn_conv_desc* d, int dtype, void* stream);
/* The same with a workspace of pasn_conv3d_wgrad_workspace_bytes(d, dtype) bytes (0 = this layer has no workspace path: ws may be NULL and
 * the call is pasn_conv3d_wgrad).  Non-zero for the stride-1 "same" (1,3,3) / (3,1,1) convs in bf16 (R(2+1)D-18, ResNet-18): the
 * gradient is then accumulated per row partition into ws and the partitions are summed in index order -- deterministic, no atomics. */
size_t pasn_conv3d_wgrad_workspace_bytes(const pasn_conv_desc* d, int dtype);
int pasn_conv3d_wgrad_ws(const void* x, const void* dy, float* dw, const pasn_conv_desc* d, int dtype, void* ws, void* stream);
/* Which kernel instance pasn_conv3d_wgrad (has_ws = 0) / pasn_conv3d_wgrad_ws with a workspace (has_ws = 1) runs for this geometry:
 * arm * 100000 + mode * 10000 + A * 100 + B with
 *   arm 1 = conv_wgrad_kernel<T, PW>           A = dtype (0 fp32, 1 bf16), B = 1 where the window map is the identity   (atomics)
 *   arm 2 = pw_wgrad_bf16_kernel<KT, TPW>      A = KT (128 | 32 rows per step), B = TPW (tiles per wave: 1 | 2 | 4 | 8)  (atomics)
 *   arm 3 = pw_wgrad_tile_kernel<COT, CIT>     A = COT, B = CIT (tiles per wave along co / ci: 101 | 201 | 102)          (atomics)
 *   arm 4 = conv_wgrad_halo_kernel<COT, PW>    A = COT (1..3), B = PW (1..3); mode 0 = (1,3,3) taps, 1 = (3,1,1) taps    (partial buffer)
 *   arm 5 = conv_wgrad_gather_kernel                                                                                    (partial buffer)
 * e.g. 212804 = pw_wgrad_bf16_kernel<128, 4>, 410301 = the halo kernel <3, 1> on temporal taps; 0 on a NULL descriptor.
 * pasn_conv3d_wgrad_row_parts: bits 0..31 = the row partitions of that launch -- the fp32 adds every dw element receives in the
 * atomic arms (up to 2 the sum has one value whatever order the atomics take), the partitions summed in index order in the
 * partial-buffer arms; bits 32.. = the blocks of the launch's grid.  For tests, profilers and benchmarks. */
int pasn_conv3d_wgrad_variant(const pasn_conv_desc* d, int dtype, int has_ws);
long pasn_conv3d_wgrad_row_parts(const pasn_conv_desc* d, int dtype, int has_ws);
/* ws: NULL, or pasn_first_conv_wgrad_workspace_bytes(d, dtype) bytes (non-zero for bf16): the clip's windows are then gathered once
 * into im2col rows and the gradient runs on the LDS-transposed bf16 MFMA kernel instead of the per-element gather. */
size_t pasn_first_conv_wgrad_workspace_bytes(const pasn_conv_desc* d, int dtype);
int pasn_first_conv_wgrad(const void* x, const void* dy, float* dw, const pasn_conv_desc* d, int in_dtype, int dtype, void* ws, void* stream);
size_t pasn_dwconv3d_wgrad_workspace_floats(const pasn_conv_desc* d);
int pasn_dwconv3d_wgrad(const void* x, const void* dy, float* ws, float* dw, const pasn_conv_desc* d, int dtype, void* stream);
int pasn_dwconv3d_dgrad(const void* dy, const float* w, void* dx, const pasn_conv_desc* d, int dtype, void* stream);

/* Head B tail in training (Video_XProtoNet.py:82-98): z = add-on output [N][S][Dp], r = occurrence-module output BEFORE the
 * abs [N][S][Pp] (both dtype) -> occ fp32 [N][P][S], feat fp32 [N][P][D], sim fp32 [N][P], logits fp32 [N][K].
 * Backward: dlogits [N][K], optional dsim [N][P] and docc [N][P][S] (NULL = none) -> dz, dr (dtype), dprotos [P][D],
 * dfc_w [K][P]; dfeat fp32 [N][P][D] is scratch.
 * z == NULL selects the occurrence-map-only mode of compute_occurence_map (Video_XProtoNet.py:100-109): forward writes occ
 * alone, backward is dr = sign(r) * docc (every other pointer but r / occ / docc / dr may be NULL). */
int pasn_xproto_tail_fwd(const void* z, const void* r, const float* protos, const float* fc_w, float* occ, float* feat, float* sim,
                         float* logits, const pasn_xproto_desc* d, int dtype, void* stream);
/* pasn_xproto_tail_fwd with a workspace of pasn_xproto_tail_workspace_bytes(d) bytes (0: no workspace path, ws may be NULL): the pooling
 * then runs on the matrix cores split over S, as in pasn_xproto_head_fwd. */
size_t pasn_xproto_tail_workspace_bytes(const pasn_xproto_desc* d);
int pasn_xproto_tail_fwd_ws(const void* z, const void* r, const float* protos, const float* fc_w, float* occ, float* feat, float* sim,
                            float* logits, const pasn_xproto_desc* d, int dtype, void* ws, void* stream);
int pasn_xproto_tail_bwd(const void* z, const void* r, const float* protos, const float* fc_w, const float* feat, const float* sim,
                         const float* dlogits, const float* dsim, const float* docc, float* dfeat, void* dz, void* dr, float* dprotos,
                         float* dfc_w, const pasn_xproto_desc* d, int dtype, void* stream);

/* Head A (ProtoPNet) backward of pasn_l2_head_fwd (ProtoPNet.py:189-243 under autograd): only the arg-min position of each
 * (image, prototype) carries gradient.  dlogits [N][K], dmin [N][P] or NULL (the cluster / separation costs act on
 * min_distances) -> dz dtype [N][S][Dp] (fully written), dprotos [P][D], dfc_w [K][P]; coef fp32 [N][P] is scratch. */
int pasn_l2_head_bwd(const void* z, const float* protos, const float* fc_w, const float* min_dist, const int32_t* argmin,
                     const float* dlogits, const float* dmin, void* dz, float* coef, float* dprotos, float* dfc_w, int N, int S, int D,
                     int Dp, int P, int K, int dtype, int activation, float eps, void* stream);

/* The affine warp of TransformLoss (loss.py:257-320): torchvision.transforms.functional.affine with
 * translate = 0, shear = 0, bilinear, fill = 0, applied to every H x W plane of a planar tensor ((N,3,T,H,W) clips: N*3*T planes;
 * (N,P,T',H',W') occurrence maps: N*P*T' planes).  bwd is the adjoint on fp32 (dx zeroed by the caller; fp32 atomics). */
int pasn_affine_warp_fwd(const void* x, void* y, long planes, int H, int W, float angle_deg, float scale, int dtype, void* stream);
int pasn_affine_warp_bwd(const float* dy, float* dx, long planes, int H, int W, float angle_deg, float scale, void* stream);

/* The train-split augmentation and normalisation of the reference's dataset, on the device (as_dataloader.py:127-133 + 221-224,
 * replacing torchvision's RandomResizedCropVideo(size=(Ho,Wo), scale=(min_crop_ratio, 1)), video_transforms.RandomRotateVideo(degrees)
 * and bin_to_norm, which run per clip and frame on the host there).  One launch maps the single-channel batch x (N,1,T,H,W) or
 * (N,1,H,W) (T = 1), in_dtype PASN_F32 / PASN_BF16 / PASN_U8, to y (N,1,T,Ho,Wo) in out_dtype PASN_F32 / PASN_BF16.  Per clip,
 * params[n] = {i, j, h, w, cos t, sin t}: param_dtype PASN_F32 (six floats) or PASN_I32 (four int32, then cos / sin as fp32 bit patterns).
 * Per output pixel, in the reference's order:
 *   crop x[..., i:i+h, j:j+w] + F.interpolate(size=(Ho,Wo), bilinear, align_corners=False, no antialias);
 *   torchvision F.rotate(t, NEAREST, expand=False, fill=0) of the Ho x Wo result (source index rounded half to even; outside -> 0);
 *   (v * scale - mean) / std (scale 1/255 for uint8; mean 0.099, std 0.171, or 0 and 1 for an unnormalised clip).
 * Identity parameters {0, 0, H, W, 1, 0} with Ho = H, Wo = W give (x * scale - mean) / std in fp32, bit for bit.  Crop indices outside
 * the clip are clamped to its border (no out-of-bounds read). */
int pasn_clip_augment(const void* x, void* y, const void* params, int N, int T, int H, int W, int Ho, int Wo, float scale, float mean,
                      float stdev, int in_dtype, int out_dtype, int param_dtype, void* stream);

/* Local explanation, ranking (local_explainability.py:88-91 contributions, :112-125 per-class sort; explainability_utils.py:69-72 the
 * prediction over the non-abstain logits).  One workgroup per clip, N clips per launch:
 *   sim [N][P] (1 - proto_dist), fc_w [K][P], logits [N][K]: fp32.  P % K == 0, G = P / K prototypes per class block, P <= 16384.
 *   contrib [N][K][P] or NULL: fc_w[k][p] * sim[n][p], one fp32 product (numpy's, bit for bit)
 *   totals  [N][K] or NULL:    sim @ fc_w.T (exact products summed in fp64, one rounding to fp32)
 *   order   [N][P] int32:      per class block c, the prototype indices c*G .. c*G+G-1 by DESCENDING similarity; equal similarities: the
 *                              HIGHER index first (the reversed stable ascending argsort; the reference's np.argsort quicksort leaves
 *                              ties unspecified).  NaN similarities give an unspecified order.
 *   rank    [N][P] int32 or NULL: position of p inside its block's order (the inverse permutation)
 *   pred    [N] int32:         argmax of logits[n][0 .. K_real) (K_real = K - 1 with an abstain class), the lowest index on ties, NaN
 *                              counts as the largest value (torch.argmax)
 *   sel     [N][k_sel] int32 or NULL: the first k_sel (1 <= k_sel <= G) entries of the predicted class's block of order */
int pasn_explain_rank(const float* sim, const float* fc_w, const float* logits, int N, int P, int K, int K_real, int k_sel,
                      float* contrib, float* totals, int32_t* order, int32_t* rank, int32_t* pred, int32_t* sel, void* stream);

/* Local explanation, heat maps (explainability_utils.py:158-174 get_normalized_upsample_occurence_maps, :177-200 get_heatmap,
 * local_explainability.py:76 / :104 the 0.3 overlay).  Two launches on `stream` (stats, write); `workspace` holds
 * pasn_explain_maps_workspace_bytes(...) bytes (8-byte aligned) and needs no initialisation.
 *   occ [N][P][Ti][Hi][Wi] fp32 (push_forward's occurrence maps; Ti = 1 for images), sel [N][k] int32 prototype indices or NULL (= all
 *   P in index order, k == P).  Per selected map: torch.nn.Upsample(size=(To,Ho,Wo), trilinear; bilinear when Ti = To = 1,
 *   align_corners=False) with torch's CPU arithmetic (explain.hip's header), min / max over the map's To*Ho*Wo voxels,
 *   v = (u - min) / ((max - min) + 1e-7f), IEEE division.
 *   maps [N][k][To][Ho][Wo] or NULL: maps_dtype PASN_F32 (v) or PASN_U8 ((uint8)(255.0f * v), truncated as numpy's np.uint8)
 *   overlay [N][k][To][Ho][Wo][3] fp32 or NULL: (src * std + mean) + alpha * lut[(uint8)(255 v)][c]; src [N][src_channels][To][Ho][Wo]
 *           (PASN_F32 / PASN_BF16; one channel counts as three identical ones), lut [256][3] fp32 (the caller's colour table)
 *   maps and overlay 16-byte aligned.  2 * Hi * Wo * 4 > 64 KiB returns PASN_ERR_UNSUPPORTED (no slow path). */
size_t pasn_explain_maps_workspace_bytes(int N, int P, int k, int Ti, int Hi, int Wi, int To, int Ho, int Wo);
int pasn_explain_maps(const float* occ, const int32_t* sel, int N, int P, int k, int Ti, int Hi, int Wi, int To, int Ho, int Wo,
                      void* maps, int maps_dtype, float* overlay, const void* src, int src_dtype, int src_channels, const float* lut,
                      float mean, float stdv, float alpha, void* workspace, void* stream);

/* Evaluation statistics of one batch (Video_XProtoNet_e2e.py:114-117 the real-class probabilities, :157 SparsityMetric, :159-171 the
 * diversity counters, :173 the similarity sums; src/utils/metrics.py:16-25; XProtoNet_Base.py:416-432).  One launch on `stream`, no
 * host synchronisation; accumulates into the caller's epoch state (zeroed by the caller at the start of an epoch):
 *   logits [N][K] fp32, sim [N][P] fp32, target [N] int64; K_real <= K real classes (K - 1 with an abstain class); the prototypes of the
 *   real classes are [0, P_cls), the abstention prototypes [P_cls, P).  Rows n land at epoch row row_offset + n < capacity.
 *   probs    [capacity][K_real] fp32 or NULL: softmax(logits[n][0 .. K_real))
 *   labels   [capacity] int32 or NULL:         (int32) target[n]
 *   logits_out [capacity][K] fp32 or NULL:     a copy of logits[n]
 *   sparsity [2] int64 or NULL:  += {sum of the per-row results, N}.  Per row: norm = sim / s (s = the row sum in fp64, rounded once to
 *                                fp32; IEEE division), sorted descending, prefix sums in fp64 each rounded to fp32; the result is the
 *                                first index whose prefix is >= level, 0 when there is none (argmax of an all-false mask: all-zero or NaN
 *                                rows).  An index, not a count, as the reference computes it.
 *   div_counts [P] int64 or NULL: += 1 for each prototype among the row's top min(k_cls, P_cls) of [0, P_cls) and its top
 *                                min(k_abs, P - P_cls) of [P_cls, P) by similarity; ties: the lower index first (stable descending sort).
 *                                Rows holding NaN: unspecified.
 *   sim_sums [P] fp64 or NULL:   += the column sums; one thread per column adds the rows in order (bitwise reproducible).
 *   P > 4096 returns PASN_ERR_UNSUPPORTED (no slow path). */
int pasn_eval_batch_stats(const float* logits, const float* sim, const int64_t* target, int N, int K, int K_real, int P, int P_cls, int k_cls,
                          int k_abs, float level, long row_offset, long capacity, float* probs, int32_t* labels, float* logits_out,
                          int64_t* sparsity, int64_t* div_counts, double* sim_sums, void* stream);

/* Weighted one-vs-rest ROC AUC (Video_XProtoNet_e2e.py:256-266 roc_auc_score(average="weighted", multi_class="ovr",
 * labels=range(K_real)) with its `except ValueError: AUC = 0`; XProtoNet_Base.py:515-525).  probs [M][K_real] fp32, labels [M] int32;
 * label < 0 is a padding row and is ignored.  Per class k, over the valid rows:
 *   U2_k = sum over positives i (label k), negatives j (label != k) of 2 [s_j < s_i] + [s_j == s_i]   (s = probs[.][k]; int64)
 *   auc_per_class[k] = U2_k / (2 n_pos n_neg) in fp64 (sklearn's trapezoidal AUC: the Mann-Whitney statistic with ties counted 1/2)
 *   auc[0] = sum_k n_pos_k auc_k / sum_k n_pos_k
 * If a class has no positive or no negative row, a label is >= K_real or a probability of a valid row is NaN, auc[0] = 0.0 (sklearn
 * raises) and the classes without a defined AUC -- every class, for NaN or a bad label -- hold NaN.  Two launches (tiled pairwise count,
 * finish) on `stream`; `workspace` holds pasn_roc_auc_workspace_bytes(M, K_real) bytes (4-byte aligned) and needs no initialisation.
 * 2 <= K_real <= 16, 1 <= M <= 2^24.  auc and auc_per_class are device memory (fp64). */
size_t pasn_roc_auc_workspace_bytes(long M, int K_real);
int pasn_roc_auc_ovr(const float* probs, const int32_t* labels, long M, int K_real, double* auc, double* auc_per_class, void* workspace,
                     void* stream);

/* Selective prediction (selective.py): what the abstention output is for.  The reference trains it (src/loss/loss.py:323-371) and has no
 * code that evaluates it, so the definitions here are the specification.  Every call is stream-ordered: no host synchronisation.
 *
 * Uncertainty score of each row of logits [M][K] fp32 into u [M] fp32:
 *   mode 0 (maxprob):         1 - max_k softmax(logits[.][0 .. K_real))[k]; bitwise 1.0f - the largest entry of the probs row that
 *                             pasn_eval_batch_stats stores for the same logits (the same expf / division sequence)
 *   mode 1 (alpha, joined):   softmax(logits[.][0 .. K))[K - 1] (loss.py:356); needs K == K_real + 1
 *   mode 2 (alpha, separate): sigmoid(logits[.][K - 1]) (loss.py:358); needs K > K_real
 * 2 <= K_real <= 16, K_real <= K <= 17, M >= 1; anything else returns PASN_ERR_ARG before any launch. */
int pasn_uncertainty_scores(const float* logits, long M, int K, int K_real, int mode, float* u, void* stream);

/* One prediction per group of rows (per cine, of its clips).  probs [M][K_real] fp32, u [M] fp32, labels [M] int32; the groups are CSR:
 * group g owns the rows group_rows[group_offsets[g] .. group_offsets[g + 1]) (int32 row indices in [0, M), ascending within a group, not
 * necessarily contiguous; offsets int64 [G + 1]).  The row indices are NOT checked: they are the caller's.  Per group of n rows, every sum
 * in fp64 in the listed order, each add and multiply rounded on its own (two calls are bitwise equal):
 *   p_mean [G][K_real] = sum p_i / n
 *   p_conf [G][K_real] = sum (1 - u_i) p_i / sum (1 - u_i); p_mean where that denominator is 0
 *   u_mean [G]         = sum u_i / n
 *   g_label [G] int32  = the label of the group's first row (-1 for an empty group, whose means are NaN); g_count [G] int32 = n
 *   status [2] int32   = {groups whose rows disagree on the label, rows holding a NaN}; zeroed by the call.  Nothing branches on them:
 *                        a conflicting group is still averaged, and whoever reads the results decides.
 * One launch: a wave per group of up to 64 rows, the block for a larger one.  G >= 1, 2 <= K_real <= 16. */
int pasn_group_predictions(const float* probs, const float* u, const int32_t* labels, const int64_t* group_offsets,
                           const int32_t* group_rows, int G, int K_real, double* p_mean, double* p_conf, double* u_mean, int32_t* g_label,
                           int32_t* g_count, int32_t* status, void* stream);

/* Risk-coverage curve.  probs [M][K_real] fp32, labels [M] int32, u [M] fp32.  A row with label < 0 is padding and is ignored, as in
 * pasn_roc_auc_ovr (so is a row with label >= K_real); Mv is the number of the others.  The valid rows are ordered by ascending u; equal
 * u (-0 = +0): the lower row index first; NaN u last, again by index.  A row's prediction is the first largest of its K_real
 * probabilities.  For m = 1 .. Mv, with cm the confusion matrix [true][predicted] of the first m rows in that order:
 *   order [M] int32      order[m - 1] = the row index of the m-th row
 *   threshold [M] fp32   threshold[m - 1] = its u
 *   acc [M] fp64         trace(cm) / m
 *   bal_acc [M] fp64     the mean over the classes with support > 0 of tp_k / support_k
 *   f1_mean [M] fp64     (1 / K_real) sum_k 2 tp_k / (support_k + predicted_k), 0 for a zero denominator
 *   aurc [1] fp64        (1 / Mv) sum_m (1 - acc[m - 1]), added in a fixed tree order; NaN when Mv = 0
 *   counts [2] int64     {Mv, valid rows whose u is NaN}
 * Entries at and past Mv are left unwritten.  All prefix counts are integers (per-block histograms, block bases, a local scan): two calls
 * are bitwise equal.  Five launches on `stream`; `workspace` holds pasn_risk_coverage_workspace_bytes(M, K_real) bytes (8-byte
 * aligned) and needs no initialisation.  1 <= M <= 2^20 (the order is a rank by counting: M^2 comparisons), 2 <= K_real <= 16;
 * anything else, or a NULL pointer, returns PASN_ERR_ARG before any launch (the size query returns 0). */
size_t pasn_risk_coverage_workspace_bytes(long M, int K_real);
int pasn_risk_coverage(const float* probs, const int32_t* labels, const float* u, long M, int K_real, int32_t* order, double* acc,
                       double* bal_acc, double* f1_mean, float* threshold, double* aurc, int64_t* counts, void* workspace, void* stream);

/* Grouped bootstrap of the evaluation statistics (bootstrap.py): B replicates of accuracy, balanced accuracy, mean F1, weighted
 * one-vs-rest AUC, risk-coverage area and error-detection AUROC, resampling GROUPS of rows (the clips of one cine are correlated: the
 * unit is the cine, or whatever key the caller grouped by).  The reference has no code for it; these definitions are the specification.
 *
 * Draws.  Philox4x32-10 (multipliers 0xD2511F53, 0xCD9E8D57; key increments 0x9E3779B9, 0xBB67AE85), key = (seed & 0xffffffff,
 * seed >> 32).  Replicate b draws G units, G the number of groups: draw d (0 <= d < G) takes output word d & 3 of the call with counter
 * (d >> 2, b, 0, 0) as a uint32 r, and the unit drawn is g = ((uint64) r * G) >> 32 (multiply-shift: a bias of at most G / 2^32, accepted).
 * counts[b][g] is the number of draws that landed on g; a row of counts sums to G.  A replicate depends on (seed, b, G) and on nothing
 * else: not on B, not on another replicate.
 *
 * pasn_bootstrap_counts: counts [B][G] int32 of the replicates b0 .. b0 + B.  1 <= G <= 2^20, 1 <= B <= 65 536, b0 >= 0.  One launch
 * (G <= PASN_BOOTSTRAP_LDS_MAX_G: a block per replicate, the histogram in LDS) or a memset and one launch (above: global integer atomics);
 * pasn_bootstrap_lds_max_groups() returns that bound.
 *
 * A replicate is the multiset of rows in which every row of group g appears counts[b][g] times, the rows in ascending row index.  Rows
 * with label < 0 or >= K_real are padding and never enter (as in pasn_risk_coverage); neither does a row that no group lists.  Each
 * statistic is the project's existing one applied to that expanded row list:
 *   cm [K_real][K_real] int64   the confusion matrix [true][predicted]; a row's prediction is the first largest probability
 *   acc, bal_acc, f1_mean       pasn_risk_coverage's formulas at full coverage (trace / W; the mean over the classes with support > 0 of
 *                               tp / support; the mean over all classes of 2 tp / (support + predicted), 0 for a zero denominator)
 *   u2 [K_real] int64           U2_k = sum over i positive (label k), j negative of w_i w_j (2 [s_j < s_i] + [s_j == s_i]), s = probs[.][k],
 *                               w = the row's number of copies; n_pos_k, n_neg_k the weighted counts
 *   auc                         sum_k n_pos_k (U2_k / (2 n_pos_k n_neg_k)) / sum_k n_pos_k: pasn_roc_auc_ovr on the expanded rows -- except
 *                               that a replicate in which a class has no positive or no negative weight has auc = NaN, not 0.0 (a 0
 *                               would poison an interval)
 *   aurc (u given)              (1 / W) sum_m (1 - acc[m]) over the expanded rows in pasn_risk_coverage's order: ascending u, equal u to
 *                               the lower row index (the copies of a row are adjacent), NaN last.  Each thread adds its positions in
 *                               order, the threads in a fixed tree.
 *   error_auroc (u given)       the AUROC of u as a detector of the wrong predictions: U2 / (2 W_wrong W_right); NaN when every row is
 *                               right, every row is wrong, or a row of the replicate has a NaN u
 * The point estimate is the same with every count equal to 1.
 *
 * pasn_bootstrap_metrics: probs [M][K_real] fp32, labels [M] int32, u [M] fp32 or NULL; the groups CSR as in pasn_group_predictions
 * (int64 offsets [G + 1], int32 rows; the indices are the caller's and every row is listed at most once), or both NULL: every row is its
 * own group and G == M.  Outputs (device memory), row b < B = replicate b, row B = the point estimate:
 *   stats [B + 1][6] fp64 = acc, bal_acc, f1_mean, auc, aurc, error_auroc (the last two NaN without u)
 *   cm [B + 1][K_real][K_real], u2 [B + 1][K_real], n_pos [B + 1][K_real], n_neg [B + 1][K_real] int64
 * The expanded rows of a replicate must number less than 2^31 (G times the largest group does: the Python wrapper checks that).  NaN
 * probabilities: unspecified.  2 <= K_real <= 16, 1 <= M <= 2^20, 1 <= G <= M, 1 <= B <= 65 536; anything else, or a NULL required
 * pointer, returns PASN_ERR_ARG before any launch (the size query returns 0).  Stream-ordered, no host synchronisation: up to three
 * memsets and six launches whatever B is -- the orders (a rank by counting per class column and for u) are shared by all replicates; a
 * block owns a replicate: counts in LDS for G <= PASN_BOOTSTRAP_LDS_MAX_G, above in a slice of the workspace, the blocks looping over
 * the replicates.  Two calls are bitwise equal.  `workspace`: pasn_bootstrap_workspace_bytes(M, G, K_real, B) bytes, 16-byte aligned,
 * no initialisation. */
#define PASN_BOOTSTRAP_LDS_MAX_G 16384
int pasn_bootstrap_lds_max_groups(void);
int pasn_bootstrap_counts(int32_t* counts, long G, int B, uint64_t seed, int b0, void* stream);
size_t pasn_bootstrap_workspace_bytes(long M, long G, int K_real, int B);
int pasn_bootstrap_metrics(const float* probs, const int32_t* labels, const float* u, const int64_t* group_offsets,
                           const int32_t* group_rows, long M, long G, int K_real, int B, uint64_t seed, double* stats, int64_t* cm,
                           int64_t* u2, int64_t* n_pos, int64_t* n_neg, void* workspace, void* stream);

/* Calibration (calibration.py): are the numbers probabilities?  Reliability bins and the statistics read from them, for the sample and
 * for grouped-bootstrap replicates of it, and temperature scaling.  The reference has no code for it; these definitions are the
 * specification.  Every call is stream-ordered: no host synchronisation.
 *
 * Rows.  probs [M][K_real] fp32, labels [M] int32.  A row is valid when 0 <= label < K_real; every other row is padding and never
 * enters.  A row's prediction is its first largest probability.
 * Weights.  Output row r = B is the point estimate: w_i = 1.  Output row b < B is replicate b: w_i = counts[b][unit_i], with
 * unit_i = row_unit[i] (int32 [M]), or unit_i = i and G == M for row_unit == NULL.  A row whose unit is not in [0, G) (-1: no group
 * lists it) never enters, the point estimate included, as in pasn_bootstrap_metrics.  counts [B][G] int32 holds the resamples exactly as
 * pasn_bootstrap_counts defines them; this call reads them, it does not draw.  NULL exactly when B == 0.
 * Confidence and bin.  c_i = conf[i] when conf [M] fp32 is given, else the row's largest probability.  A valid row with c NaN, c < 0 or
 * c > 1 is not binned: it is counted, weighted, in skipped[r].  Bin j = min(n_bins - 1, (int)((double)c * n_bins)): intervals [lo, hi),
 * c = 1 in the last bin.  q_i = (uint64)((double)c * 4294967296.0); every sum below is an integer sum, exact and independent of order.
 * The expanded rows of a replicate number less than 2^31 (as for the bootstrap), so qsum stays below 2^63.
 *   n, hit [B + 1][n_bins] int64     sum w, sum w [pred == label];   qsum [B + 1][n_bins] uint64   sum w q
 *   cn, cpos [B + 1][K_real][n_bins] int64, cq uint64: the same per class k with the confidence probs[i][k] (never `conf`) and the
 *                                    positives label == k; a probability outside [0, 1] is not binned (NaN: unspecified)
 *   skipped [B + 1] int64
 *   stats [B + 1][6] fp64, with conf_j = (double)qsum_j * 0x1p-32, W = sum_j n_j and Wv = W + skipped (the weight of all valid rows):
 *     ece      sum_j |hit_j - conf_j| / W, j ascending
 *     mce      the largest |hit_j - conf_j| / n_j over the bins with n_j > 0
 *     cw_ece   (1 / K_real) sum_k sum_j |cpos_kj - cconf_kj| / Wv
 *     brier    sum_i w_i sum_k (p_ik - [label_i == k])^2 / Wv, every term fp64
 *     nll      -sum_i w_i log(max(p_i,label, FLT_MIN)) / Wv, fp64 log
 *     conf_gap sum_j (conf_j - hit_j) / W; positive: over-confident
 *   W == 0 gives NaN for ece, mce and conf_gap, Wv == 0 for the other three.  The brier and nll sums run in a fixed order (each thread
 *   its rows in order, the threads in a fixed tree): two calls are bitwise equal in every output.
 * Two launches whatever B is: the row words shared by all replicates, then a block per output row (the blocks loop past 2048 rows), its
 * histogram in LDS (64-bit integer LDS atomics).  Output row B is written last in memory order only: a caller that splits its replicates
 * into chunks passes the chunk's counts and output pointers advanced by the chunk's first replicate, and the next chunk overwrites the
 * point row this one left behind.  `workspace`: pasn_calibration_workspace_bytes(...) bytes, 16-byte aligned, no initialisation.
 * 2 <= K_real <= 16, 1 <= M <= 2^20, 1 <= G <= M, 1 <= n_bins <= 64, 0 <= B <= 65 536; anything else, or a NULL required pointer,
 * returns PASN_ERR_ARG before any launch (the size query returns 0).
 *
 * Temperature.  Over the valid rows, z = logits[.][0 .. K_real) widened to fp64 (logits [M][K] fp32, K_real <= K <= 17):
 *   g(beta) = sum_i [logsumexp_k(beta z_ik) - beta z_i,label],  beta = 1 / T in [1/64, 64]
 * g is convex: g' = sum_i (E_beta[z_i] - z_i,label), g'' = sum_i Var_beta[z_i] >= 0.  fit [4] fp64 = {beta, g(1) / Mv, g(beta) / Mv, status}:
 *   status 3  no valid row: beta = 1 (both means NaN)
 *   status 1  g'(1/64) >= 0 (this includes rows that are all flat): beta = 1/64
 *   status 2  g'(64) <= 0 (separable data): beta = 64
 *   status 0  otherwise: the root of g', by safeguarded Newton from beta = 1 in PASN_TEMPERATURE_STEPS steps whatever the data: a step
 *             evaluates (g', g'') at beta, shrinks the bracket by the sign of g' (g' == 0 closes it) and takes the Newton point where it
 *             lies strictly inside the bracket and g'' > 0, else the midpoint.
 * Per-row terms are fp64; the rows of a block are added in a fixed tree, the blocks' partials in index order: two calls are bitwise
 * equal.  3 + PASN_TEMPERATURE_STEPS + 1 launches; the iteration crosses launch boundaries and no block ever waits for another.
 * `workspace`: pasn_temperature_workspace_bytes(M, K_real) bytes, 16-byte aligned, no initialisation.
 *
 * pasn_temperature_probs: probs [M][K_real] fp32, p_k = exp(beta (z_k - z_max)) / sum_k exp(beta (z_k - z_max)) in fp64, rounded once to
 * fp32; u [M] fp32 (or NULL) = 1.0f - the row's largest p, bitwise.  beta [1] fp64 is DEVICE memory (fit, or the caller's 1 / T). */
#define PASN_TEMPERATURE_STEPS 48
size_t pasn_calibration_workspace_bytes(long M, long G, int K_real, int n_bins, int B);
int pasn_calibration_bins(const float* probs, const int32_t* labels, const float* conf, const int32_t* row_unit, const int32_t* counts,
                          long M, long G, int K_real, int n_bins, int B, int64_t* n, int64_t* hit, uint64_t* qsum, int64_t* cn,
                          int64_t* cpos, uint64_t* cq, int64_t* skipped, double* stats, void* workspace, void* stream);
size_t pasn_temperature_workspace_bytes(long M, int K_real);
int pasn_temperature_fit(const float* logits, const int32_t* labels, long M, int K, int K_real, double* fit, void* workspace, void* stream);
int pasn_temperature_probs(const float* logits, long M, int K, int K_real, const double* beta, float* probs, float* u, void* stream);

/* Conformal prediction (conformal.py): which classes can NOT be ruled out for a row, at a stated error rate?  Split conformal prediction:
 * thresholds calibrated on one split, and on another a set of classes per row that holds the true one with probability >= 1 - alpha (for
 * exchangeable rows).  The reference has no code for it; these definitions are the specification.  Every call is stream-ordered: no host
 * synchronisation, no block waiting on another.
 *
 * Rows.  probs [M][K_real] fp32, labels [M] int32.  A row is valid when 0 <= label < K_real and none of its K_real probabilities is NaN.
 * Padding rows (any other label) enter nothing; NaN rows enter nothing and are counted in nan_rows.
 * Scores.  s(i, k) for every class k of row i, in fp64 from the fp32 probabilities, every operation rounded on its own (no FMA), then
 * rounded once to fp32:
 *   PASN_CONFORMAL_LAC   1.0 - p[k]
 *   PASN_CONFORMAL_APS   rank the row's classes by descending probability, the lower class first on ties; s = acc + U p[k], acc the
 *                        running fp64 sum, in rank order from 0.0, of the probabilities ranked strictly before k.  U = 1.0 unless
 *                        `randomized`; then one uniform per row: word 0 of philox4x32_10 with the counter (i & 0xFFFFFFFF, i >> 32, salt,
 *                        0) and the key (seed & 0xFFFFFFFF, seed >> 32), U = word * 2^-32
 *   PASN_CONFORMAL_RAPS  the APS value, then + lam * max(0, rank - k_reg), rank the 1-based rank of k
 *   Every score of a NaN row is NaN.  probabilities outside [0, 1] are ranked and added as they are.
 * pasn_conformal_scores: scores [M][K_real] fp32; with labels also own [M] fp32 = s(i, label_i) (NaN for a row that is not valid) and
 * stratum [M] int32 = the label of a valid row, -1 for a padding row, -2 for a NaN row.  labels, own and stratum are given together or
 * not at all.  One launch, one thread per row.
 *
 * Thresholds.  Stratum 0 is all valid rows, stratum 1 + c the valid rows of label c; each holds n own-label scores.  For every alpha
 * (host array of A doubles, each in (0, 1)): r = ceil((double)(n + 1) * (1.0 - alpha)) in fp64 on the device, and qhat is the r-th
 * smallest of the stratum's scores -- a value, so the order among ties cannot matter --, +inf when r > n (n = 0 included).  The selection
 * is exact: an element of the input (a score is never -0.0).
 * pasn_conformal_quantiles: qhat [1 + K_real][A] fp32, n [1 + K_real] int64, r [1 + K_real][A] int64 from own and stratum as
 * pasn_conformal_scores wrote them.  A byte-wise radix select on an order-preserving 32-bit key: one memset, four counting launches (a
 * block counts the rows of its own stratum into 256 LDS bins per alpha, then integer atomics) and a finish, whatever M is; work linear
 * in M.  `workspace`: pasn_conformal_workspace_bytes(M, K_real, A) bytes, 16-byte aligned, no initialisation.
 *
 * Sets.  Class k is in row i's set at level a iff s(i, k) <= qhat[0][a] (marginal) or s(i, k) <= qhat[1 + k][a] (`mondrian`), compared in
 * fp32; +inf admits every class; a row whose scores hold a NaN gets the empty set.
 * pasn_conformal_sets: masks [A][M] uint16 (bit k: class k) for every row, and tallies [A][T] int64, T = pasn_conformal_tally_words(K_real)
 * = 3 + 4 (K_real + 1) + 2 K_real, per level in this order:
 *   rows, covered, nan_rows                      rows that enter; of them, the label is in the set; rows with a NaN score
 *   size_hist, covered_by_size [K_real + 1]      by set size
 *   u_by_size (uint64), u_rows_by_size [K_real + 1]  with u [M] fp32 (or NULL): the sum of q = (uint64)((double)u * 4294967296.0) and the
 *                                                number of rows, over the rows that enter with u in [0, 1]
 *   class_n, class_covered [K_real]              by label
 * With labels the rows that enter are the valid ones; with labels == NULL every row without a NaN score enters and covered,
 * covered_by_size, class_n and class_covered stay 0.  All integer sums: exact and independent of order.  One memset and one launch;
 * LDS counters per block, then integer atomics.
 * 2 <= K_real <= 16, 1 <= M <= 2^20, 1 <= A <= PASN_CONFORMAL_MAX_ALPHAS, lam >= 0, k_reg >= 0; anything else, or a NULL required
 * pointer, returns PASN_ERR_ARG before any launch (the size queries return 0). */
#define PASN_CONFORMAL_MAX_ALPHAS 8
#define PASN_CONFORMAL_LAC 0
#define PASN_CONFORMAL_APS 1
#define PASN_CONFORMAL_RAPS 2
int pasn_conformal_scores(const float* probs, const int32_t* labels, long M, int K_real, int kind, int randomized, uint64_t seed,
                          uint32_t salt, double lam, int k_reg, float* scores, float* own, int32_t* stratum, void* stream);
size_t pasn_conformal_workspace_bytes(long M, int K_real, int A);
int pasn_conformal_quantiles(const float* own, const int32_t* stratum, long M, int K_real, int A, const double* alphas, float* qhat,
                             int64_t* n, int64_t* r, void* workspace, void* stream);
int pasn_conformal_tally_words(int K_real);
int pasn_conformal_sets(const float* scores, const float* qhat, const int32_t* labels, const float* u, long M, int K_real, int A,
                        int mondrian, uint16_t* masks, int64_t* tallies, void* stream);

/* Ordinal evaluation (ordinal.py): the statistics that use the ORDER of the classes.  Class index = grade (the reference's class_labels
 * are listed in ascending severity: No AS < Early AS < Significant AS).  The reference has no code for it; these definitions are the
 * specification, tests/ordinal_cases.py their restatement.  Every call is stream-ordered: no host synchronisation, no block waiting on
 * another, no floating-point atomics; two calls are bitwise equal.  The file is compiled so that every fp64 operation is rounded on its
 * own (fp contract(off)).
 *
 * Rows.  probs [M][K_real] fp32, labels [M] int32.  A row with label < 0 or label >= K_real is padding and never enters.  A row's
 * prediction is its first largest probability.  NaN probabilities: unspecified, as in pasn_bootstrap_metrics.  2 <= K_real <= 16 and
 * 1 <= M <= 2^20; anything else, or a NULL required pointer, returns PASN_ERR_ARG before any launch (the size query returns 0).
 *
 * Agreement.  From a confusion matrix cm [true][pred] int64 with row sums r_i, column sums c_j and total n.  All sums are int64 and each
 * result is one fp64 expression of them, so a result is a function of the matrix alone (bitwise):
 *   mae             (double)(sum |i - j| cm_ij) / (double)n
 *   within_one      (double)(sum_{|i - j| <= 1} cm_ij) / (double)n
 *   under           (double)(sum_{j < i} cm_ij) / (double)n         predicted grade below the true one
 *   over            (double)(sum_{j > i} cm_ij) / (double)n
 *   kappa_linear, kappa_quadratic   1.0 - ((double)n * (double)A) / (double)E, with A = sum w_ij cm_ij, E = sum w_ij r_i c_j, and
 *                   w_ij = |i - j| (linear) or (i - j)^2 (quadratic) as integers
 * NaN for a kappa whose E is 0 (all weight in one row class and the same column class); all six NaN when n == 0.  E stays inside int64
 * for n < 2^27 (225 n^2 < 2^63); above that the kappas are unspecified.
 * pasn_ordinal_agreement: cm [R][K_real][K_real] int64 -> out [R][6] fp64 in the order above, one launch (a thread per matrix),
 * 1 <= R <= 65 537.  Given pasn_bootstrap_metrics' cm it yields all replicates and the point estimate at once.
 * pasn_ordinal_confusion: cm [K_real][K_real] int64 of the rows (one memset, one launch; integer atomics).
 *
 * Cuts.  For c = 1 .. K_real - 1 (output index c - 1) the positive class is label >= c, the score is
 *   s_c = p[c] + p[c + 1] + ... + p[K_real - 1]   in fp32, added in that order (a sum of its own per cut, from p[c] upwards),
 * and the decision at threshold theta is "positive iff s_c >= theta".  pasn_ordinal_cut_scores writes scores [K_real - 1][M] fp32.
 * Scores compare as floats do, -0 equal to +0; a reported theta that is zero is +0.
 *
 * Weights.  w_i = the row's number of copies: 1 for the sample (output row B), counts[b][unit(i)] for replicate b (output row b < B).
 * Draws, units and the groups CSR are exactly those of pasn_bootstrap_counts / pasn_bootstrap_metrics, so replicate b of this call and of
 * pasn_bootstrap_metrics with the same (seed, G) is the same multiset of rows; a row that no group lists never enters.  The expanded
 * rows of a replicate must number less than 2^31.
 *
 * Per output row and cut:
 *   pn [2] int64    P, N: the weight of the positives and of the negatives
 *   u2 int64        U2 = sum over i positive, j negative of w_i w_j (2 [s_j < s_i] + [s_j == s_i]), as in pasn_roc_auc_ovr with weights
 *   stats [2] fp64  auc = (double)U2 / (2.0 * (double)P * (double)N);
 *                   ap = sum over the distinct score values v that carry positive weight of ((double)tp_v / (double)P) *
 *                   ((double)TP_v / (double)(TP_v + FP_v)), tp_v the positive weight at exactly v, TP_v and FP_v the positive and
 *                   negative weight at scores >= v; values without positive weight add nothing.  Summation order: the positions of the
 *                   ascending order are dealt out in chunks of 2048, eight consecutive positions per thread; a term belongs to the
 *                   position behind its value's last row; each of the 256 threads adds its terms in position order, chunk after chunk,
 *                   and the threads are added in the tree of the other evaluation kernels (a butterfly within each wave of 64, then
 *                   (w0 + w1) + (w2 + w3)).  A restatement that sums in another order agrees within M 2^-50 (a term is at most 1 and
 *                   carries three roundings; at most M terms and M adds of partial sums <= 1 on each side).
 *   Candidate thresholds: the distinct scores of the rows with w > 0, and +inf (nobody positive: TP = FP = 0).
 *   Operating points, T = n_spec + n_sens + 1 per cut, in this order:
 *     specificity tau   the SMALLEST candidate theta with (double)(N - FP_theta) / (double)N >= tau  (+inf always qualifies)
 *     sensitivity tau   the LARGEST candidate theta with (double)TP_theta / (double)P >= tau         (the lowest candidate always does)
 *     Youden            the candidate maximising TP_theta N - FP_theta P as int64, ties to the larger theta (+inf scores 0)
 *   op_theta [T] fp32 and op_tally [T][2] int64 = TP_theta, FP_theta.
 *   fix_tally [F][2] int64 = TP_theta, FP_theta for the caller's thresholds fixed [K_real - 1][F] fp32 (device memory; a NaN threshold
 *   admits nobody).  This is how a fit from another split is applied, and how a decision curve is read.
 * A cut with P == 0 or N == 0 has auc, ap and every op_theta NaN and its op_tally 0; pn, u2 (= 0) and fix_tally are written as usual,
 * and no other cut or output row is disturbed.
 * Sensitivity TP / P, specificity (N - FP) / N, PPV, NPV and net benefit TP / n - (FP / n) pt / (1 - pt) (treat-all: P / n - (N / n)
 * pt / (1 - pt)) are host arithmetic on these tallies (ordinal.py).
 *
 * pasn_ordinal_screen: groups as in pasn_bootstrap_metrics (both NULL: every row its own group, G == M); specificities / sensitivities
 * are HOST arrays of n_spec / n_sens doubles, each in (0, 1), 0 <= n <= PASN_ORDINAL_MAX_TARGETS each; 0 <= n_fixed <=
 * PASN_ORDINAL_MAX_FIXED; 0 <= B <= 65 536 (B == 0: the point estimate only), 1 <= G <= M.  Outputs are [B + 1][K_real - 1][...] as
 * above.  Up to four memsets and six launches whatever B is: the order of each cut's scores (a rank by counting, order_key.h) is shared
 * by all replicates; a block owns a replicate, the unit counts in LDS for G <= PASN_BOOTSTRAP_LDS_MAX_G and in a slice of the workspace
 * above that (the blocks looping over the replicates), and settles U2, ap, every operating point and every fixed tally of a cut in ONE
 * pass over its sorted rows (packed wave scans).  `workspace`: pasn_ordinal_workspace_bytes(M, G, K_real, B) bytes, 16-byte aligned, no
 * initialisation. */
#define PASN_ORDINAL_MAX_TARGETS 8
#define PASN_ORDINAL_MAX_FIXED 32
int pasn_ordinal_agreement(const int64_t* cm, long R, int K_real, double* out, void* stream);
int pasn_ordinal_confusion(const float* probs, const int32_t* labels, long M, int K_real, int64_t* cm, void* stream);
int pasn_ordinal_cut_scores(const float* probs, long M, int K_real, float* scores, void* stream);
size_t pasn_ordinal_workspace_bytes(long M, long G, int K_real, int B);
int pasn_ordinal_screen(const float* probs, const int32_t* labels, const int64_t* group_offsets, const int32_t* group_rows, long M, long G,
                        int K_real, int B, uint64_t seed, const double* specificities, int n_spec, const double* sensitivities, int n_sens,
                        const float* fixed, int n_fixed, int64_t* pn, int64_t* u2, double* stats, float* op_theta, int64_t* op_tally,
                        int64_t* fix_tally, void* workspace, void* stream);

/* Out-of-distribution detection (ood.py): does a row look like anything the model was trained on?  A HIGHER score means MORE
 * out-of-distribution.  The reference has no code for it; these definitions are the specification.  Every call is stream-ordered: no
 * host synchronisation, no block waiting on another, no floating-point atomics.  The file is compiled without contraction: "rounded on
 * its own" below means exactly that (no FMA).
 *
 * pasn_ood_head_scores: scores that need no fit, from sim [M][P] fp32 (the prototype similarities the last layer sees) and logits [M][K]
 * fp32, one launch.  maxsim [M] fp32 = 1.0f - max_p sim[p]; a row with a NaN in sim gives NaN.  energy [M] fp32, in fp64 from the first
 * K_real logits: m = max_k l_k, -(m + log(sum_k exp(l_k - m))), the sum taken in class order from 0.0, rounded once to fp32; a row with a
 * NaN among them gives NaN.  Either output (with its input) may be NULL, not both.  1 <= M <= 2^20, 1 <= P <= 4096, 1 <= K_real <= K <=
 * 4096.
 *
 * pasn_ood_knn: the k nearest rows of bank [Mb][E] fp32 for every row of q [Mq][E] fp32, exact.
 *   Distance.  d(i, m) is accumulated in fp32 from 0.0f for j = 0 .. E - 1 in that order: t = q[i][j] - bank[m][j], acc = acc + t * t; the
 *   subtraction, the product and the add each rounded on their own.  A function of the two rows only: two calls are bitwise equal
 *   however the work is tiled.
 *   Eligibility.  Bank row m is eligible for query i unless it holds a NaN, or self_base >= 0 and m == self_base + i (leave-one-out: the
 *   queries are themselves rows self_base .. of the bank), or d(i, m) is NaN (inf - inf in some coordinate).
 *   dist [Mq][k] fp32 and index [Mq][k] int32: the k eligible rows of smallest d in ascending d, the lower bank index first on ties;
 *   entries past the number of eligible rows are +inf / -1; a query holding a NaN gets NaN / -1 throughout.  status [2] int64 = {bank
 *   rows holding a NaN, query rows holding a NaN}; the call zeroes it.  The detector's score is dist[i][k - 1].
 *   One memset and two launches whatever the sizes: the bank is split across blocks, each leaves per-query partial lists in
 *   `workspace` (pasn_ood_knn_workspace_bytes(Mq, Mb, E, k) bytes, 16-byte aligned, no initialisation), a finish merges them in bank order.
 *   1 <= E <= 1024, 1 <= k <= 64, 1 <= Mq <= 2^20, 1 <= Mb <= 2^24, -1 <= self_base <= Mb.
 * pasn_ood_rows_normalize: y [M][E] = the rows of x [M][E] over their norm, one launch: n2 the fp32 sum of squares in j order from 0.0f
 *   (product and add rounded on their own), y[j] = x[j] / sqrtf(n2), both correctly rounded; a row with n2 == 0 is copied unchanged.  y may
 *   be x.  1 <= M <= 2^24, 1 <= E <= 1024.
 *
 * pasn_ood_moments: the sufficient statistics of class-conditional Gaussians with a shared covariance, from x [M][E] fp32 and labels [M]
 *   int32.  A row is valid when 0 <= label < K and it holds no NaN; the others are skipped and counted.  n [K] int64 the valid rows per
 *   class, sum [K][E] fp64 their sums, scatter [E][E] fp64 = sum x x^T over the valid rows, skipped [2] int64 = {rows with a label out
 *   of range, rows with a label in range holding a NaN}.  Every term is exact in fp64; the order of the additions is fixed: the rows are
 *   cut into chunks of pasn_ood_moment_chunk() consecutive rows (skipped rows included in the cut), a chunk is summed from 0.0 in row
 *   order, and the chunk partials are added in chunk order from 0.0.  With accumulate != 0 the call's result is then added to what the
 *   outputs hold (one addition); otherwise it overwrites them.  One memset and two launches.  `workspace`:
 *   pasn_ood_moments_workspace_bytes(M, E, K) bytes, 16-byte aligned.  1 <= M <= 2^24, 1 <= E <= 256, 1 <= K <= 16.
 * pasn_ood_mahalanobis: m [M][K] fp64, m_c = || W (x - mu_c) ||^2 from x [M][E] fp32, mu [K][E] fp64 and W [E][E] fp64 lower triangular
 *   (the entries above the diagonal are not read), in fp64; the order of the sums inside is NOT defined (held to a bound, not bitwise).
 *   score [M] fp32 = (float) min_c m_c over the classes with a finite mean (mu[c][0] finite), argclass [M] int32 that class, the lower
 *   one on ties; NaN / -1 when no class qualifies.  One launch.  1 <= M <= 2^20, 1 <= E <= 256, 1 <= K <= 16.
 *
 * pasn_ood_tally: flags [A][M] uint8 and tallies [A][8] int64 from scores [M] fp32, kind [M] int32 (0 in-distribution, 1 shifted,
 *   anything else a padding row), correct [M] int32 (or NULL) and tau [A] fp32.  A row is flagged iff score > tau or the score is NaN
 *   (padding rows get their flag too).  Per level: id_rows, id_flagged, ood_rows, ood_flagged, nan_rows (rows of kind 0 or 1 with a NaN
 *   score), id_correct_kept, id_kept, id_correct_flagged (the last three stay 0 without `correct`).  One memset and one launch; LDS
 *   counters per block, then integer atomics.  1 <= M <= 2^20, 1 <= A <= 8.
 *
 * Anything else, or a NULL required pointer, returns PASN_ERR_ARG before any launch (the size queries return 0). */
int pasn_ood_head_scores(const float* sim, const float* logits, long M, int P, int K, int K_real, float* maxsim, float* energy, void* stream);
size_t pasn_ood_knn_workspace_bytes(long Mq, long Mb, int E, int k);
int pasn_ood_knn(const float* q, const float* bank, long Mq, long Mb, int E, int k, long self_base, float* dist, int32_t* index,
                 int64_t* status, void* workspace, void* stream);
int pasn_ood_rows_normalize(const float* x, long M, int E, float* y, void* stream);
int pasn_ood_moment_chunk(void);
size_t pasn_ood_moments_workspace_bytes(long M, int E, int K);
int pasn_ood_moments(const float* x, const int32_t* labels, long M, int E, int K, int accumulate, int64_t* n, double* sum, double* scatter,
                     int64_t* skipped, void* workspace, void* stream);
int pasn_ood_mahalanobis(const float* x, const double* mu, const double* W, long M, int E, int K, double* m, float* score, int32_t* argclass,
                         void* stream);
int pasn_ood_tally(const float* scores, const int32_t* kind, const int32_t* correct, const float* tau, long M, int A, uint8_t* flags,
                   int64_t* tallies, void* stream);

/* Explanation faithfulness (faithfulness.py): deletion and insertion curves.  Do the voxels an occurrence map marks carry the prototype
 * similarity and the class probability?  The clip's voxels are removed (deletion) or inserted into a baseline (insertion) in the order of
 * the map, a step at a time, and the model is run on every perturbed copy.  The reference has no code for it; these definitions are the
 * specification.  Every call is stream-ordered: no host synchronisation, no global atomics, no block waiting on another.
 *
 * pasn_perturb_steps: when does a voxel change sides?  maps [M][V] uint8 (M = N k maps of V = To Ho Wo voxels, pasn_explain_maps' uint8
 * output), counts [S1] int32 in DEVICE memory, non-decreasing, 0 <= counts[s] <= V (anything else: unspecified steps, no out-of-bounds
 * access).  The voxels of one map are ordered by (level DESCENDING, flat index ASCENDING); pos(v) in [0, V) is a voxel's position.
 *   steps [M][V] uint8: steps[v] = the number of s with counts[s] <= pos(v): the first step whose top set {pos < counts[s]} holds the
 *   voxel, S1 when none does.  For every s exactly counts[s] voxels have steps <= s.
 * Integers only: the output is exact and does not depend on the launch geometry.  Three launches: 256-bin histograms of 4096-voxel tiles
 * (in LDS, then in the workspace); per map the level totals, the step of every level whose voxels share one, the at most S1 levels that
 * straddle a count and their exclusive prefixes across the tiles; the write pass, in which a straddling level's voxels get their rank
 * inside the tile from a block scan.  Rows are not 16-byte aligned when V is odd: the tiles are laid on the 16-byte grid of the row's
 * address, whole 16-byte words are loaded and stored, a row's head and tail go byte by byte.  maps and steps 16-byte aligned;
 * `workspace`: pasn_perturb_steps_workspace_bytes(M, V, S1) bytes, 16-byte aligned, no initialisation.
 * 1 <= M <= 65 535, 1 <= V < 2^31, 1 <= S1 <= 64; anything else, or a NULL pointer, returns PASN_ERR_ARG before any launch (the size
 * query returns 0).
 *
 * pasn_perturb_apply: the perturbed clips of a chunk of steps.  x [N][C][V] (dtype PASN_F32 / PASN_BF16), steps [N][k][V] as above,
 * step_ids [Sc] int32 in DEVICE memory (any subset of the steps, any order), baseline [N][C][V] of the same dtype or NULL (then every
 * baseline element is `fill`, rounded to the dtype once, to nearest even).  mode 0 (deletion): out = steps[v] <= s ? baseline : x;
 * mode 1 (insertion): out = steps[v] <= s ? x : baseline, s = step_ids[.].
 *   out [N][k][Sc][C][V]: a bitwise copy of the element selected.  Deletion at a step with counts[s] = 0 is x, at counts[s] = V the baseline.
 * One launch; a block owns 4096 voxels of one (n, j, s), reads their steps once into an LDS mask and walks the C channels.  16-byte
 * stores wherever the output address allows (a row's head and tail element by element), 16-byte loads where the input addresses allow.
 * 1 <= N k Sc <= 2^31 - 1 blocks along two grid axes (N k <= 65 535, Sc <= 65 535), 1 <= C <= 64, 1 <= V < 2^31.
 *
 * pasn_perturb_curves: one launch, one block, after the model has run on the perturbed batch in [n][j][s] order with ALL S1 steps,
 * B = N k S1 rows: sim [B][P] fp32 (1 - proto_dist), logits [B][K] fp32; sel [N][k] int32 (the prototype of map j), cls [N] int32 (the
 * class whose probability is followed, normally the prediction on the clean clip), counts [S1] int32 as above.
 *   curve_sim  [N][k][S1] fp32: sim[b][sel[n][j]], a copy
 *   curve_prob [N][k][S1] fp32: softmax(logits[b][0 .. K_real))[cls[n]]: the largest logit subtracted, expf, the sum in column order,
 *                               one IEEE division, all fp32
 *   auc [N][k][2] fp64 (similarity, probability): sum_{s >= 1} (x_s - x_{s-1}) (y_s + y_{s-1}) / 2 with x_s = (double)counts[s] / V and
 *                               y the fp32 curve value widened, s ascending, every operation rounded on its own
 *   acc [2 k S1 + 2 k + 1] fp64 or NULL, the caller's running sums over the clips of a sweep (zeroed by the caller):
 *                               += sum_n curve_sim [k][S1], += sum_n curve_prob [k][S1], += sum_n auc [k][2], += N; n ascending
 * An entry of sel outside [0, P) or of cls outside [0, K_real) gives NaN curves for that clip, nothing is read out of bounds.
 * 1 <= N k S1 <= 2^20, 1 <= S1 <= 64, 1 <= K_real <= 16, K_real <= K <= 17, P >= 1, 1 <= V < 2^31. */
size_t pasn_perturb_steps_workspace_bytes(long M, long V, int S1);
int pasn_perturb_steps(const uint8_t* maps, const int32_t* counts, long M, long V, int S1, uint8_t* steps, void* workspace, void* stream);
int pasn_perturb_apply(const void* x, const uint8_t* steps, const int32_t* step_ids, const void* baseline, float fill, int N, int C, int k,
                       long V, int Sc, int mode, int dtype, void* out, void* stream);
int pasn_perturb_curves(const float* sim, const float* logits, const int32_t* sel, const int32_t* cls, const int32_t* counts, int N, int k,
                        int S1, int P, int K, int K_real, long V, float* curve_sim, float* curve_prob, double* auc, double* acc,
                        void* stream);

/* Black-box saliency (saliency.py): RISE (Petsiuk, Das, Saenko, BMVC 2018) as the baseline the occurrence maps' faithfulness is compared
 * with.  The model is run on many randomly masked copies of a clip and the masks are averaged, weighted by the score.  The masks are never
 * stored: a mask is a function of (seed, clip id, mask index) through Philox and is regenerated wherever it is needed, and every sum runs
 * in a fixed order, so a map is reproducible bit for bit and does not depend on which batch the clip arrived in.  The reference has no
 * code for it; these definitions are the specification (tests/saliency_cases.py restates them in numpy).  Every call is stream-ordered:
 * no host synchronisation, no global atomics, no block waiting on another.
 *
 * Geometry.  A clip has V = T H W voxels (images: T = 1).  A coarse grid (gt, gh, gw) gives the cells ct = ceil(T / gt), ch = ceil(H / gh),
 * cw = ceil(W / gw) and a lattice of (gt + 2)(gh + 2)(gw + 2) points.  keep is a uint32, min(2^32 - 1, floor(p 2^32)) of the keep
 * probability p, computed by the host.  seed: 64 bits, the Philox key is (seed & 0xffffffff, seed >> 32).  clip = clip0 + n (mod 2^32) is
 * the caller's id of clip n of the call.
 *   lattice bit   of point c = (it (gh + 2) + iy)(gw + 2) + ix of mask m: word c & 3 of philox4x32_10(counter (c >> 2, m, clip, 0), key);
 *                 1.0f iff that word < keep, else 0.0f
 *   shift         of mask m: the words w of philox4x32_10((0, m, clip, 1), key); st = (w0 ct) >> 32, sh = (w1 ch) >> 32, sw = (w2 cw) >> 32
 *                 (the multiply-shift of the bootstrap's draws)
 *   mask value    at voxel (t, y, x), all fp32, every multiply and add rounded on its own (no contraction, as the OOD distances):
 *                 px = x + sw, ix = px / cw (integers), fx = (float)(px - ix cw) / (float)cw (IEEE division); the same along H and T;
 *                 lerp(a, b, f) = a + (b - a) f; first along W (four times), then along H (twice), then along T.
 *                 ix + 1 <= gw + 1 (the lattice has g + 2 points per axis for that), the value lies in [0, 1]; T = 1 gives ft = 0 and
 *                 the lower plane exactly.
 *
 * pasn_rise_apply: the masked copies of the clips for the masks m0 .. m0 + Mc - 1.  x [N][C][V] (PASN_F32 / PASN_BF16), baseline of the
 * same shape and dtype or NULL (then every baseline element is `fill`, rounded to the dtype once, to nearest even).
 *   out [N][Mc][C][V] = b + (x - b) mask: x and b widened to fp32, every operation rounded on its own, the result rounded to the dtype
 *   once, to nearest even; a NaN result is the canonical quiet NaN (0x7fc00000 / 0x7fc0).  One mask serves the C channels of a voxel.
 * One launch; a block owns 4096 voxels of one (n, m): it generates the mask's lattice in LDS, computes the 4096 mask values once and walks
 * the C channels.  16-byte stores wherever the output address allows (a row's head and tail element by element), 16-byte loads where the
 * input addresses allow.  1 <= N <= 65 535, 0 <= m0, 1 <= Mc, m0 + Mc <= 65 535, 1 <= C <= 64.
 *
 * pasn_rise_scores: after the model has run on the masked copies, in [n][m] order with ALL M masks: sim [N M][P] fp32, logits [N M][K] fp32.
 *   scores [N][M][k] fp32.  target 0 (prototype): sim[row][sel[n][j]], a copy (sel [N][k] int32; logits, cls may be NULL).
 *   target 1 (class), k = 1: softmax(logits[row][0 .. K_real))[cls[n]] with pasn_perturb_curves' arithmetic (the largest logit
 *   subtracted, expf, the sum in column order, one IEEE division; cls [N] int32; sim, sel may be NULL), K_real <= 16, K_real <= K <= 17.
 * An entry of sel outside [0, P) or of cls outside [0, K_real) gives NaN, nothing is read out of bounds.
 *
 * pasn_rise_maps: S[n][j][v] = sum_m (double)scores[n][m][j] (double)mask_m[v] and Cov[n][v] = sum_m (double)mask_m[v], both with m
 * ascending in fp64 (the product of two fp32 values is exact in fp64, so contracting it into the sum cannot change the result).
 *   norm 0 (coverage): S / Cov, 0 where Cov == 0;  norm 1 (expected): S / ((double)M ((double)keep / 4294967296.0)); rounded to fp32 once.
 *   saliency [N][k][V] fp32 (or NULL), cov [N][V] fp64 (or NULL), maps [N][k][V] uint8 (or NULL) by pasn_explain_maps' rule, so that both
 *   kinds of map are on one scale: min / max over the map's V fp32 values, v = (s - min) / ((max - min) + 1e-7f), (uint8)(255.0f v)
 *   truncated.  A map that holds a NaN has an unspecified uint8 map.
 * Launches: the lattices and shifts of all (n, m) into the workspace; per group of at most four maps one launch in which a thread owns a
 * voxel and walks the masks (staged in LDS, pasn_rise_stage_masks(gt, gh, gw) at a time) with one fp64 accumulator per map and one for
 * the coverage, and leaves the block's extrema in the workspace; one launch that combines the extrema and quantises.
 * `workspace`: pasn_rise_maps_workspace_bytes(...) bytes, 16-byte aligned, no initialisation.  1 <= M <= 65 535, N k <= 65 535.
 *
 * Everywhere: 1 <= gt <= 16, 1 <= gh, gw <= 32, at most 8 192 lattice points, T, H, W >= 1, V < 2^31, keep >= 1; anything else, or a NULL
 * required pointer, returns PASN_ERR_ARG before any launch (the size queries return 0). */
int pasn_rise_apply(const void* x, const void* baseline, float fill, int N, int C, int T, int H, int W, int gt, int gh, int gw,
                    uint32_t keep, uint64_t seed, uint32_t clip0, int m0, int Mc, int dtype, void* out, void* stream);
int pasn_rise_scores(const float* sim, const float* logits, const int32_t* sel, const int32_t* cls, int N, int M, int k, int P, int K,
                     int K_real, int target, float* scores, void* stream);
int pasn_rise_stage_masks(int gt, int gh, int gw);
size_t pasn_rise_maps_workspace_bytes(int N, int k, int M, int T, int H, int W, int gt, int gh, int gw);
int pasn_rise_maps(const float* scores, int N, int k, int M, int T, int H, int W, int gt, int gh, int gw, uint32_t keep, uint64_t seed,
                   uint32_t clip0, int norm, float* saliency, uint8_t* maps, double* cov, void* workspace, void* stream);

/* Robustness (robustness.py): echo-style corruptions of a clip, and the stability of the prediction and of its explanation under them.
 * Does the prototype explanation survive the perturbations the class prediction survives?  The reference has no code for it; these
 * definitions are the specification.  Every call is stream-ordered: no host synchronisation, no allocation, no global atomics, no block
 * waiting on another.
 *
 * pasn_clip_corrupt: one launch, normalised clip in, corrupted normalised clip out.  x, y [N][C][T][H][W] (planar, the model's input;
 * T = 1 for images), C = 1 or 3, dtype PASN_F32 / PASN_BF16 on both sides.  The descriptor holds the optional stages; a stage that is
 * NULL or zero is off:
 *   src_t [N][T] int32 in DEVICE memory or NULL   frame hold: output frame t is computed from input frame src_t[n][t], clamped to [0, T)
 *   taps [2R+1] fp32 in DEVICE memory, 0 <= R <= 8  separable blur over H and W with edge replication (R = 0: off, taps may be NULL)
 *   row_a, row_b [H] fp32 in DEVICE memory or NULL  photometric stage per image row (row = depth): gain, contrast, depth attenuation;
 *                                                 it is on when either is given, a NULL row_a then counts as ones, a NULL row_b as zeros
 *   sigma_add, sigma_mul fp32                     additive noise, multiplicative speckle
 *   seed uint64; mean, stdv fp32                  the noise stream; the clip's normalisation
 * Per output element (n, c, t, h, w), every fp32 operation rounded on its own (no contraction):
 *   1. ts = src_t ? clamp(src_t[n][t], 0, T - 1) : t
 *   2. blur, photometric stage and both sigmas all off: y is a bitwise copy of x[n][c][ts][h][w]; steps 3 - 8 are skipped
 *   3. pixel domain: v(h', w') = widen(x[n][c][ts][h'][w']) * stdv + mean
 *   4. blur (R > 0): row pass g(h', w) = sum_{i = -R .. R} taps[i + R] * v(h', clamp(w + i, 0, W - 1)), accumulated from 0.0f with i
 *      ascending as acc = acc + (tap * v); column pass: the same over h on g.  H or W smaller than R is legal.
 *   5. photometric: v = row_a[h] * v + row_b[h]
 *   6. noise: z is shared by the C channels of a voxel (a grey clip stays grey): Philox4x32-10 with key (seed lo, seed hi) and counter
 *      (q lo, q hi, n, 0), q = (t H + h) W + w of the OUTPUT voxel, gives r0 .. r3;
 *        z = (float)(int32)((r0 >> 8) + (r1 >> 8) + (r2 >> 8) + (r3 >> 8) - 33554430) * c,  c = the fp32 nearest sqrt(3) * 2^-24.
 *      z is an Irwin-Hall(4) variate of unit variance bounded at +-3.47: it is NOT a Gaussian (no tails).  Only integers and one
 *      conversion go into it, so numpy reproduces it bit for bit.  Then v = v + sigma_add * z (when sigma_add != 0), and after that
 *      v = v + (sigma_mul * z) * v (when sigma_mul != 0).
 *   7. v = fminf(fmaxf(v, 0), 1); NaN gives 0
 *   8. y = (v - mean) / stdv, IEEE division, rounded once to the dtype (to nearest even)
 * A block owns a 32 x 64 tile of one (n, t) with its R-wide halo in LDS, the row pass goes into LDS, the column pass reads it; the block
 * walks the C channels.  16-byte stores where the output address allows, element by element at a row's head and tail.  Instances: blur
 * on / off x dtype.  NULL x, y or descriptor, R outside [0, 8], R > 0 without taps, C not 1 or 3, a size <= 0, another dtype or
 * more than 2^31 - 1 tiles return PASN_ERR_ARG before any launch.
 *
 * pasn_stability_stats: compare the clean (a) and the corrupted (b) forward of the same clips.  logits_a, logits_b [N][K], sim_a, sim_b
 * [N][P], occ_a, occ_b [N][P][S] fp32 (push_forward's occurrence maps on the feature grid (Ti, Hi, Wi), S = Ti Hi Wi), labels [N] int32
 * or NULL.  P % K == 0, G = P / K, 1 <= k <= G, 1 <= m <= S.  pred_a, pred_b: the argmax over [0, K_real) with pasn_explain_rank's rule
 * (lowest index on ties, NaN largest).  sel_a: the first k of pred_a's class block by sim_a in pasn_explain_rank's order (descending,
 * the higher index first on ties); sel_b: the first k of THE SAME block by sim_b.
 *   clip [N][4] fp64:    flip (pred_b != pred_a as 0 / 1); tv = 0.5 sum_c |p_a - p_b| with the softmax over K_real in fp64 (largest logit
 *                        subtracted, sums in class order); p_a[pred_a] - p_b[pred_a]; |sel_a and sel_b| / k
 *   correct [N][2] int32 (pred_a == label, pred_b == label), written when labels is given (then required)
 *   sel [N][k] int32:    sel_a
 *   pair [N][k][4] fp64, for p = sel_a[n][j]:
 *     dsim   (double)sim_b[n][p] - (double)sim_a[n][p]
 *     corr   Pearson correlation of the two maps over S: mean = (sum in index order) / S; saa = sum (a - mean_a)^2, sbb, sab likewise,
 *            fp64 in index order; corr = sab / sqrt(saa * sbb); 1 when saa and sbb are both exactly 0, 0 when exactly one is
 *     iou    of the two top-m sets, a map's top set being its m voxels first in (value DESCENDING, index ASCENDING):
 *            (double)inter / (double)(2 m - inter), integers in, so exact
 *     shift  sqrt(dt^2 + dh^2 + dw^2) / sqrt((Ti-1)^2 + (Hi-1)^2 + (Wi-1)^2) between the two argmax positions (lowest index on ties) in
 *            (t, h, w) grid units; 0 when S = 1
 *   acc [6 + 4 k + 1] fp64 or NULL, the caller's running sums (zeroed by the caller), added with n ascending: the 4 clip statistics, the
 *                        2 correct counts (0 without labels), pair [k][4], N
 * Two calls are bitwise equal.  Maps holding NaN give unspecified statistics (nothing is read out of bounds).  At most three launches:
 * one wave per clip; one block per (n, j) that holds both maps in LDS and ranks them by counting; one block for acc.
 * S > 4096 returns PASN_ERR_UNSUPPORTED (no slow path); 1 <= N <= 65 535, 1 <= K_real <= K, P <= 16 384, k <= 4096; anything else, or a NULL
 * pointer among the required ones, returns PASN_ERR_ARG before any launch. */
typedef struct pasn_corrupt_desc {
    const int32_t* src_t;
    const float* taps;
    const float* row_a;
    const float* row_b;
    uint64_t seed;
    int32_t R;
    float sigma_add, sigma_mul, mean, stdv;
} pasn_corrupt_desc;
int pasn_clip_corrupt(const void* x, void* y, int N, int C, int T, int H, int W, int dtype, const pasn_corrupt_desc* desc, void* stream);
int pasn_stability_stats(const float* logits_a, const float* logits_b, const float* sim_a, const float* sim_b, const float* occ_a,
                         const float* occ_b, const int32_t* labels, int N, int K, int K_real, int P, int Ti, int Hi, int Wi, int k, int m,
                         double* clip, int32_t* correct, int32_t* sel, double* pair, double* acc, void* stream);

/* Global explanations: the k nearest clips of a split per prototype, kept on the device while a loader is swept (global_explain.py).
 * The reference ships only the raw material, the whole (clips, P) similarity matrix "for ranking prototypes"
 * (XProtoNet_Base.py:613-656 get_sim_scores / load_sim_scores; explain_global is a stub); the selection rule per batch is the push's
 * (push_abs_revision.py:288-307: the clips of the prototype's class, or all clips), kept for k winners instead of one.
 *
 * pasn_topk_xproto_update: one launch per batch, no host synchronisation, one wave per prototype.  Per prototype j the batch's eligible
 * clips (labels[b] == proto_class[j] where class_mask[j] != 0, every clip otherwise) are merged into row j of the caller's state:
 *   proto_dist [B][P] fp32, labels [B] int64, proto_class [P] int32, class_mask [P] int32
 *   top_dist  [P][k] fp32   (init +inf)   ascending
 *   top_index [P][k] int64  (init -1)     global clip index = index_base + b
 *   top_slot  [P][k] int32  (init 0 .. k-1 per row): the payload slot of each entry; a new entry takes over the slot of the entry it
 *                           evicts, so every row stays a permutation of 0 .. k-1 and payload rows never move
 * Order: ascending (distance, global index) -- equal distances put the LOWER global index first, whatever the batch boundaries (the
 * push keeps the LATER clip on a tie; the two rules differ by design).  Fewer than k eligible clips leave the tail at (+inf, -1).
 * A clip index must be fed once per sweep.  NaN distances give an unspecified row.
 * 1 <= k <= 64, 1 <= P <= 4096, B >= 1; anything else, or a NULL pointer, returns PASN_ERR_ARG before any launch (no slow path). */
int pasn_topk_xproto_update(const float* proto_dist, const int64_t* labels, const int32_t* proto_class, const int32_t* class_mask,
                            float* top_dist, int64_t* top_index, int32_t* top_slot, int B, int P, int k, int64_t index_base,
                            void* stream);

/* The winners' payload follows them without a host round trip: called once per payload kind after pasn_topk_xproto_update of the same
 * batch (the records push_abs_revision.py:300-307 keeps for one winner, for k).  Every (j, e) with
 * index_base <= top_index[j][e] < index_base + B copies row b = top_index[j][e] - index_base of `payload` to store[j][top_slot[j][e]]
 * (every entry of the updated row whose index lies in this batch arrived in this batch, so no "fresh" flag is needed).
 *   payload : per_proto != 0: [B][P][row_elems] (occurrence maps), row (b, j);  per_proto == 0: [B][row_elems] (logits, labels), row b
 *   store   : [P][k][row_elems];  elem_bytes in {1, 2, 4, 8}: the copy is bitwise, in 16-byte accesses where row size and both base
 *             addresses allow, else 8 / 4 / elem_bytes.  Same argument limits as the update. */
int pasn_topk_gather(const int64_t* top_index, const int32_t* top_slot, const void* payload, void* store, int B, int P, int k,
                     long row_elems, int elem_bytes, int per_proto, int64_t index_base, void* stream);

/* Ranking statistics of one batch (what a consumer of the reference's saved sim_scores / targets, XProtoNet_Base.py:613-656, computes
 * from the whole matrix): class_sim_sum [P][K] fp64 += (double)(1.0f - proto_dist[b][p]) grouped by labels[b]; class_count [K] int64 +=
 * the rows per label.  One thread per prototype adds the rows in index order (as sim_sums of pasn_eval_batch_stats): two sweeps over the
 * same batches are bitwise equal.  Labels outside [0, K) are skipped.  1 <= K <= 64, 1 <= P <= 4096, B >= 1. */
int pasn_proto_class_stats(const float* proto_dist, const int64_t* labels, int B, int P, int K, double* class_sim_sum,
                           int64_t* class_count, void* stream);

/* The reference dataset's clip resize on the device (as_dataloader.py:204-207, skimage.transform.resize(window, (T, H, W)) of
 * scikit-image >= 0.19 with its defaults: uint8 / 255, Gaussian anti-aliasing (sigma = max(0, (f - 1) / 2), mode 'mirror', truncate 4)
 * on the shrinking axes, linear zoom with grid_mode (source (o + 0.5) f - 0.5, mode 'mirror')).  That operator is separable,
 * A_T (x) A_H (x) A_W, each axis a banded table the host builds in float64 and rounds to fp32 once (protoasnet_amd/resample.py).
 * One launch over a RAGGED batch of N windows:
 *   src      the flat source buffer (device, 16-byte aligned, src_bytes a multiple of 16), uint8 (in_dtype PASN_U8) or fp32 (PASN_F32)
 *   desc     int64 [N][8]: {byte offset of the source cine in src, first frame of the window, T_w, H0, W0 (window of the cine
 *            (T_src, H0, W0) stored C-contiguous), offsets (int32 units) into bands of the T, H and W tables}
 *   bands    int32 [bands_len]: tables {n_in, n_out, S, start[n_out], weights[n_out][S] as fp32 bits}; starts non-decreasing
 *   y        (N, T, H, W) in out_dtype PASN_F32 / PASN_BF16: (A v * scale - mean) / std, fp32 accumulation (mean 0, std 1: the clip)
 * Geometry: a workgroup owns tile_h x tile_w output pixels (at most pasn_cine_resize_pixels_per_block(T)) of one clip; tmp_rows >= the
 * largest H-band union of a tile, raw_pitch (a multiple of 16) >= its W-band union in bytes + 15, chunk_rows rows staged at a time,
 * band_floats >= tile_w (S_W + 1) + tile_h (S_H + 1) over the batch's tables (the tile's bands, staged in LDS).
 * A clip whose descriptor, tables or source range disagree with the launch is not read: its outputs are NaN. */
int pasn_cine_resize_pixels_per_block(int T);
int pasn_cine_resize(const void* src, long src_bytes, const long long* desc, const int* bands, long bands_len, void* y, int N, int T, int H,
                     int W, int tile_h, int tile_w, int tmp_rows, int raw_pitch, int chunk_rows, int band_floats, float mean, float stdev,
                     int in_dtype, int out_dtype, void* stream);

/*
 * The training loss recipe in the library (csrc/proto_loss.hip): the seven terms of XProtoNet_Base.py:54-81 as
 * Video_XProtoNet_e2e.py:86-110 applies them -- the classes of src/loss/loss.py:23-254 and :323-371 -- and the per-batch statistics of
 * Video_XProtoNet_e2e.py:112-153, replacing their eager tensor expressions and what autograd replays for them.  A term whose weight is 0
 * is skipped, as the reference returns before computing it, and its slot is 0.  reduction: 0 = 'mean' (batch mean, then the sum over
 * classes / prototypes), 1 = 'sum'.
 *   ce_mode 0: CeLoss (loss.py:23-34) on logits [N][K];  1 / 2: CeLossAbstain (loss.py:323-371) with the 'joined' / 'separate' logit path,
 *              K - 1 >= 2 real classes and the abstention output in column K - 1; ab_weight as there
 *   scores [N][P]: ClusterRoiFeat / SeparationRoiFeat (loss.py:98-186) on similarities -- the per-class MAXIMUM over the C class-major
 *              prototype groups of P / C; sep_abstain: class C - 1 is never penalised.  patch = 1: ClusterPatch / SeparationPatch
 *              (loss.py:37-95) on min_distances -- the per-class MINIMUM and the opposite signs
 *   protos [P][D]: OrthogonalityLoss (loss.py:189-231), ortho_mode 0 = 'per_class' (the same C groups), 1 = 'all': the upper triangle of
 *              the pairwise cosine similarities, each vector divided by max(|v|, 1e-8) as torch.nn.functional.cosine_similarity does
 *   occ [N][P][S], map_dtype PASN_F32 / PASN_BF16: L_norm (loss.py:234-254) with map_p = 1 / 2 over each row of S map elements
 *   fc_w [fc_rows][P] (+ fc_mask of the same shape, or NULL): L_norm with fc_p = 1 / 2 over the whole masked weight
 * Labels outside the classes are clamped into them (the eager path raises a device assertion there).
 */
typedef struct pasn_proto_loss_desc {
    int32_t N, K, K_real;            /* rows; logit columns; real classes of the confusion matrix (<= K) */
    int32_t P, D, C, fc_rows;        /* prototypes, prototype depth, prototype classes (groups), rows of the last layer's weight */
    int64_t S;                       /* elements of one (clip, prototype) map row */
    int32_t ce_mode, ce_reduction, cluster_reduction, sep_reduction, sep_abstain, patch, ortho_mode, map_p, map_reduction, fc_p, map_dtype;
    float w_ce, ab_weight, w_cluster, w_sep, w_ortho, w_map, w_fc;
} pasn_proto_loss_desc;

/* Forward, at most two launches, no host synchronisation.  terms [7] fp32: the weighted terms in the trainer's order (cross entropy,
 * cluster, separation, orthogonality, map norm, transform, last-layer norm); loss [1]: their sum, added in that order.  transform_term:
 * the already weighted TransformLoss value (losses.py / warp.hip) as a device scalar, NULL = 0.  workspace: N * P + P floats, written
 * here and read by the backward (row norms, per-prototype orthogonality sums); may be NULL when w_map and w_ortho are 0.  Optional epoch
 * statistics, accumulated in the same launch: cm [K_real][K_real] int64 += 1 at (label clamped to [0, K_real), first largest of the
 * K_real real-class logits); loss_sum [7] fp32 += terms.  Every sum runs in a fixed order: two calls are bitwise equal. */
int pasn_proto_loss_fwd(const float* logits, const float* scores, const int64_t* target, const float* protos, const void* occ,
                        const float* fc_w, const float* fc_mask, const float* transform_term, float* terms, float* loss, float* workspace,
                        int64_t* cm, float* loss_sum, const pasn_proto_loss_desc* d, void* stream);

/* Backward of pasn_proto_loss_fwd for the upstream gradient grad_loss, a DEVICE scalar; at most two launches.  Every non-NULL output is
 * fully written (zeros where its terms are off); NULL skips that gradient (a frozen parameter).  d_occ has the maps' dtype.  Subgradients
 * as autograd takes them: sign(0) = 0, an all-zero row or weight under p = 2 gets zero, a tied per-class maximum / minimum sends its
 * gradient to the first index.  The transform term's gradient is grad_loss itself and is left to the caller. */
int pasn_proto_loss_bwd(const float* grad_loss, const float* logits, const float* scores, const int64_t* target, const float* protos,
                        const void* occ, const float* fc_w, const float* fc_mask, const float* workspace, float* d_logits, float* d_scores,
                        float* d_protos, void* d_occ, float* d_fc_w, const pasn_proto_loss_desc* d, void* stream);

/*
 * Training: all conv weights of a step packed from the live fp32 parameters into the layouts the forward kernels read, in ONE launch
 * (replaces the per-parameter torch expressions of the host side: the reference has no counterpart -- cuDNN reads the parameters as they
 * are, model/XProtoNet.py keeps nn.Conv modules).  `jobs`, `block_job`, `block_chunk` are DEVICE arrays: block b packs destination
 * elements [block_chunk[b], block_chunk[b] + 1) x pasn_pack_chunk() of job block_job[b]; every destination element is written.
 *   mode 0: dense forward   dst[row = co][tap][k = ci]  = src[co][ci][tap]              (src [cout][cin][taps], dst [rows][taps][kc])
 *   mode 1: dense dX        dst[row = ci][tap][k = co]  = src[co][ci][taps - 1 - tap]   (transposed, taps reversed)
 *   mode 2 / 3: depthwise   dst[tap][c] = src[c][tap] / src[c][taps - 1 - tap]          (fp32 dst [taps][kc = Cp])
 *   frag = 1 (taps == 1): dst is fragment-major [rows/32][kc/kstep][2][32][ch] (the x-tile pointwise kernels, w_frag = 1)
 */
typedef struct pasn_pack_job {
    const float* src;
    void* dst;
    long n;  /* destination elements */
    int mode, cout, cin, taps, rows, kc, frag, bf16, kstep, ch;
} pasn_pack_job;
int pasn_pack_chunk(void);
int pasn_pack_weights(const pasn_pack_job* jobs, const int* block_job, const int* block_chunk, int nblocks, void* stream);

/*
 * Training: the optimizer side of a step, ONE launch each (csrc/optim.hip).  Tables as for pasn_pack_weights: `jobs`, `block_job` and
 * `block_chunk` are DEVICE arrays, block b works on elements [block_chunk[b], block_chunk[b] + 1) x pasn_optim_chunk() of job
 * block_job[b].  `jobs_host` is the same job table in host memory: it is checked before the launch (a NULL pointer, n <= 0, a group index
 * out of range, more than PASN_OPTIM_MAX_GROUPS groups, or an `nblocks` that is not the sum of the jobs' chunk counts returns
 * PASN_ERR_ARG and launches nothing).  The check reads the host copy ONLY: that the device table holds the same jobs is the caller's
 * business (build both from one array, as optim.py does).  Both calls are stream-ordered: no host synchronisation, no allocation, no pointer kept after the
 * return.  16-byte accesses when every pointer of a job is 16-byte aligned, 4-byte accesses otherwise (views at odd storage offsets).
 *
 * pasn_adam_step replaces `optimizer.step()` of the reference's loop (Video_XProtoNet_e2e.py:137-142) for torch.optim.Adam with
 * amsgrad = maximize = decoupled_weight_decay = False, over the parameter groups of XProtoNet_e2e.py:36-82, per parameter:
 *   t += 1;  g += wd p;  m = b1 m + (1 - b1) g;  v = b2 v + (1 - b2) g^2;  p -= (lr / (1 - b1^t)) m / (sqrt(v) / sqrt(1 - b2^t) + eps)
 * in torch's order of fp32 operations (lerp, mul + addcmul, sqrt / div / add, addcdiv), the scalars formed in double.  A parameter
 * without a gradient has no job: its moments and its t do not move.  `groups` is read at the call (host memory, passed to the kernel by
 * value): a learning rate a scheduler rewrote between two steps is seen by the next one.
 *   step : one 8-byte word per parameter in device memory, zero before the first step: t in the low 32 bits; the high 32 bits hold
 *          the `stamp` of the call that last advanced it.  The kernel advances t itself.  `stamp` must be non-zero and differ from
 *          the previous call's (a call counter): it is how the blocks of one job agree on t while one of them stores t + 1.
 *
 * pasn_grad_accumulate: dst[i] += src[i] (one fp32 add per element, bitwise `dst.add_(src)`) for every job: the reference's undivided
 * accumulation over micro-batches (Video_XProtoNet_e2e.py:137-142) for the gradients that do not lie in one flat span (those take
 * pasn_add_inplace).
 */
#define PASN_OPTIM_MAX_GROUPS 8
typedef struct pasn_adam_group {
    double lr, beta1, beta2, eps, weight_decay;
} pasn_adam_group;
typedef struct pasn_adam_job {
    float* param;
    const float* grad;
    float* exp_avg;
    float* exp_avg_sq;
    unsigned long long* step;
    long n;
    int group, reserved;
} pasn_adam_job;
typedef struct pasn_accum_job {
    float* dst;
    const float* src;
    long n;
} pasn_accum_job;
int pasn_optim_chunk(void);
int pasn_adam_step(const pasn_adam_job* jobs, const pasn_adam_job* jobs_host, int njobs, const int* block_job, const int* block_chunk,
                   int nblocks, const pasn_adam_group* groups, int ngroups, unsigned stamp, void* stream);
int pasn_grad_accumulate(const pasn_accum_job* jobs, const pasn_accum_job* jobs_host, int njobs, const int* block_job, const int* block_chunk,
                         int nblocks, void* stream);

/* Prototype pruning (prune.py): what does the prediction lose when a prototype goes, and which prototypes can go?  The last layer is
 * linear without a bias, so the logits of "the model without prototype p" follow from the similarities of ONE sweep: an M x P x K problem.
 *
 * Inputs: sim [M][P] fp32, fc_w [K][P] fp32 (the last layer), labels [M] int32 (a row whose label is < 0 or >= K_real is SKIPPED by every
 * tally; its z is still kept), proto_class [P] int32, floor [K_real] int32.  1 <= M <= 2^24, 1 <= P <= PASN_PRUNE_MAX_P, 2 <= K_real <= K
 * <= 16; every input finite.  The abstention logit, if any (K = K_real + 1), is the last one and takes no part in anything below.
 *
 *   base logits     z[n][k]  = the fp64 sum of (double)fc_w[k][j] * (double)sim[n][j] (exact products: 24 + 24 bits), sequential, j ascending
 *                              from 0.0, no contraction; z is [M][K_real] fp64.  Every prototype is kept at the start.
 *   ablated logits  za[n][k] = z[n][k] - (double)fc_w[k][p] * (double)sim[n][p] for candidate p: one rounding.
 *   prediction      the argmax over k < K_real, the LOWEST k on ties.
 *   margin          z[n][y] - max_{k != y} z[n][k], y the row's label.
 *   tallies of p    over the rows with a label: wrong (prediction != y), wrong per true class, flips (the ablated prediction differs from the
 *                   current model's), margin_sum (fp64).  The same for the current model, nothing removed (flips = 0).
 *   margin_sum      the rows are cut into chunks of pasn_prune_chunk() consecutive rows (skipped rows included in the cut), a chunk is summed
 *                   from 0.0 in row order, the chunk sums are added from 0.0 in ascending chunk order.  No result depends on the launch
 *                   geometry or on the number of CUs.
 *
 * One elimination round: the candidates are the kept prototypes with proto_class[p] < K_real whose class has MORE kept prototypes than
 * floor[class]; the one with the smallest (wrong, -margin_sum, index) is taken.  With `accept` != 0 it is removed only if wrong <= wrong_0 +
 * max_extra_errors and (use_margin != 0) margin_sum >= fl(margin_fraction * margin_sum_0), wrong_0 / margin_sum_0 the tallies of the
 * model before round 0.  If it is not removed (or there is no candidate) a stop flag is set in device memory: this round and every later one
 * record removed = -1 and repeat the tallies of the model as it stands.  After a removal z becomes the za of the removed prototype -- the
 * subtract chain, not a recomputation: a round is one pass over sim.  With |w| <= 2, |sim| <= 1, P <= 256 the chain stays within 1e-9 of the
 * in-order sum over the kept prototypes (P roundings of at most ulp(2 P) / 2).
 *
 * pasn_prune_eliminate: one memset, one launch that builds z and the round-0 tallies (one wave per chunk, lanes over candidates, rows walked
 * in order), then per round two launches: a one-block select (it adds the chunk sums in order, picks, records) and the pass that applies
 * the removal to z and tallies the next round's candidates (after the last round it only applies).  rounds = 0: the building launch and the
 * select launch's summing half.  No block waits for another, nothing is read back.
 *   table_i [P + 1][2 + K_real] int64: per prototype (row P: the unpruned model) wrong, flips, wrong per class; table_m [P + 1] fp64 margin_sum
 *   removed [rounds] int32; trace_i [rounds][1 + K_real] int64 (wrong, wrong per class) and trace_m [rounds] fp64 of the model AFTER the round
 *   kept [P] int32 (1 / 0) at the end; z [M][K_real] fp64 the logits of the model at the end.
 * `workspace`: pasn_prune_workspace_bytes(M, P, K_real) bytes (0: sizes out of range), 16-byte aligned, no initialisation. */
#define PASN_PRUNE_MAX_P 256
#define PASN_PRUNE_MAX_ROWS (1L << 24)
int pasn_prune_chunk(void);
size_t pasn_prune_workspace_bytes(long M, int P, int K_real);
int pasn_prune_eliminate(const float* sim, const float* fc_w, const int32_t* labels, const int32_t* proto_class, const int32_t* floor, long M,
                         int P, int K, int K_real, int rounds, int accept, int64_t max_extra_errors, int use_margin, double margin_fraction,
                         double* z, int64_t* table_i, double* table_m, int32_t* removed, int64_t* trace_i, double* trace_m, int32_t* kept,
                         void* workspace, void* stream);

/*
 * Data-parallel gradient exchange on RCCL (xGMI), without torch.distributed in the data path: ONE in-place sum all-reduce of the
 * flat fp32 gradient bucket per optimizer step.  The reference trains on one GPU and has no collective
 * (SURVEY section 0); these four calls are what a trainer needs around protoasnet_amd/dp.py.  librccl.so is resolved at run time.
 *   pasn_comm_unique_id : rank 0 fills PASN_COMM_ID_BYTES bytes; the caller ships them to the other ranks (any side channel)
 *   pasn_comm_init      : every rank, with its HIP device current; *comm_out is an opaque handle
 *   pasn_allreduce      : buf[count] (dtype PASN_F32 / PASN_BF16) summed over the ranks in place, asynchronous on `stream`
 */
#define PASN_COMM_ID_BYTES 128
int pasn_comm_unique_id(void* id_out);
int pasn_comm_init(const void* id, int world_size, int rank, void** comm_out);
int pasn_allreduce(void* comm, void* buf, size_t count, int dtype, void* stream);
int pasn_comm_destroy(void* comm);

#ifdef __cplusplus
}
#endif
#endif /* PROTOASNET_AMD_H */
