/* ctrlora_hip.h -- C ABI of libctrlora_hip.so: the MI355X (gfx950) kernels behind the
 * CtrLoRA hot path (SD1.5 UNet + ControlNet + condition-LoRA forward/backward, DDIM step).
 *
 * The reference (xyfJASON/ctrlora) has no FFI: the hot path sits behind Python class
 * contracts (cldm.*), and every operator below replaces the ATen kernel(s) that the cited
 * reference lines issue.  The Python host side (ctrlora_amd/, cldm/, ldm/) binds these
 * entry points with ctypes; INTEGRATION.md shows the binding.
 *
 * Conventions
 *   - every function returns 0 on success, CL_EINVAL (1) for an unsupported shape /
 *     alignment, CL_ELAUNCH (2) for a HIP launch failure.  Nothing is allocated, nothing
 *     synchronises; all work is enqueued on `stream` (a hipStream_t) and is hipGraph-capture safe.
 *   - dtype: 0 = bf16 storage (fp32 accumulate, fp32 statistics/softmax),
 *            1 = fp32 storage ("parity mode": f32-input MFMA, exact fmaf chains).
 *   - activations are token-major ("NHWC"): a [rows, C] matrix with an explicit row stride
 *     (ld, in elements) so that operators can read/write column slices of wider buffers
 *     (decoder concat buffers, fused QKV).  rows = b*H*W + y*W + x.
 *   - channel counts / K dimensions must be multiples of 32 (bf16) or 16 (fp32); N and all
 *     ld's multiples of 8.  Base pointers 16-byte aligned.
 */
#ifndef CTRLORA_HIP_H
#define CTRLORA_HIP_H

#ifdef __cplusplus
extern "C" {
#endif

#ifndef CTRLORA_HIP_INTERNAL  /* the library's own sources carry these as C++ enums */
#define CL_OK 0
#define CL_EINVAL 1
#define CL_ELAUNCH 2
#define CL_BF16 0
#define CL_F32 1
#endif

/* the version this header describes; cl_abi_version() returns the one the loaded library was built from */
#define CL_ABI_VERSION 7
int cl_abi_version(void);
/* the hipError_t behind the most recent CL_ELAUNCH return (diagnostics) */
int cl_last_hip_error(void);

/* Scratch for the deterministic split-K path of the contraction kernels (fp32 partial slabs for
 * the deep-K / small-MN products of the 8x8 and 16x16 UNet levels).  The library never allocates:
 * the host (torch) owns the buffer and registers it once per process; without one, split-K is off.
 * 64 MiB covers every CtrLoRA shape at batch 16.  Used stream-ordered on the launching stream.
 * The same scratch carries the per-workgroup column-sum partials of cl_colsum and of cl_layernorm_bwd's
 * dgamma / dbeta (partials + a finishing launch instead of same-cache-line atomics); without a registered
 * buffer those two fall back to fp32 atomics.  (NULL, 0) unregisters. */
int cl_set_workspace(void* device_ptr, long bytes);
/* A second (third, fourth) scratch region bound to one stream: contractions launched on that stream use it
 * instead of the default, so concurrent streams never share split-K slabs. */
int cl_set_stream_workspace(void* stream, void* device_ptr, long bytes);
/* tuning hook: force a tile configuration (-1 = built-in heuristic).  The ids are the rows of the table kCfgs in
 * csrc/gemm.hip: kernel family, tile, waves, ring, GEGLU wave pair, fall-back conditions, one line per id */
int cl_gemm_force_config(int cfg);
/* tuning hook: impose the split-K factor of the workspace path on every following contraction (0 = built-in rule) */
int cl_gemm_force_splitk(int splitk);
/* Measured launch table: the contraction with this signature (dtype CL_BF16/CL_F32, cl_gemm_mode, M, N, K1, K2,
 * geglu = GEGLU epilogue (act 2)) is launched with tile configuration `cfg` and split-K factor `splitk` (0 = built-in rule
 * for the factor) instead of the built-in choice.  The host loads ctrlora_amd/gemm_tuned_gfx950.json (written by
 * tools/gemm_autotune.py from timings on an MI355X) through this entry at start-up; signatures not in the table
 * keep the built-in rules, and every configuration re-checks its own preconditions at launch. */
int cl_gemm_tune_set(int dtype, int mode, int M, int N, int K1, int K2, int geglu, int cfg, int splitk);
int cl_gemm_tune_clear(void);
int cl_gemm_tune_size(void);
/* (Schedule / launch-form A-B switches that do not change results live in ctrlora_amd/csrc/debug_hooks.h, outside this
 * boundary.) */

/* ---- dense contractions -------------------------------------------------------------
 * One MFMA kernel family (csrc/gemm.hip) behind all of them:
 *   out[M,N] = act( A1.W1^T + A2.W2^T + bias[n] + rowbias[m / rows_per_batch, n] ) * alpha
 *              + beta * residual[m, n]
 */
enum cl_gemm_mode {
  CL_GEMM_LINEAR = 0,   /* A1 row-major [M,K1]                                              */
  CL_GEMM_CONV_S1 = 1,  /* A1 = NHWC [B,Hin,Win,K1]; 3x3 stride 1 pad 1                      */
  CL_GEMM_CONV_S2 = 2,  /* 3x3 stride 2 pad 1                                                */
  CL_GEMM_CONV_UP2 = 3, /* 3x3 over nearest-x2 upsampled input                               */
  CL_GEMM_CONV_T2 = 4,  /* 3x3 over zero-stuffed x2 grid: data-gradient of CL_GEMM_CONV_S2   */
  CL_GEMM_CONV_S2A = 5, /* 3x3 stride 2, pad (0,1,0,1): AutoencoderKL's Downsample
                           (ldm/modules/diffusionmodules/model.py:80-84)                        */
  /* Phase-decomposed forms of UP2 / T2 with the same results (Upsample.forward, openaimodel.py:108-118; the data gradient of
   * Downsample's stride-2 conv, :150): output pixel (2y + a, 2x + b) depends on a 2 x 2 (UP2) / (1 + a) x (1 + b) (T2) window
   * of source pixels only, so the four phases (a, b) are stride-1 window products 4 K1 / on average 2.25 K1 deep instead
   * of 9 K1.  A1 = source NHWC [B,Hin,Win,K1]; M = 4 B Hin Win (B Hin Win a multiple of 128), Hout = 2 Hin, Wout = 2 Win;
   * C / residual / rowbias rows are OUTPUT pixels (the kernel interleaves the phases); W1 = phase-packed weights
   * (ctrlora_amd/engine/packing.py: Conv3W.phase_weights), ldw1 ignored.  bf16 / fp32, K1 whole 128-byte lines, no K2.   */
  CL_GEMM_CONV_UP2P = 6,
  CL_GEMM_CONV_T2P = 7,
  /* 4x4 window, stride 2, pad 1: the data gradient of CL_GEMM_CONV_UP2 formed on the source grid (each source pixel receives
   * from upsampled rows / columns 2y - 1 .. 2y + 2; coincident 3x3 taps summed) -- 16 K1 deep at M / 4 rows instead of a
   * stride-1 data gradient on the upsampled grid plus a 2x2 sum pool.  A1 = dy NHWC [B,Hin,Win,K1] (upsampled grid),
   * Hout = Hin / 2, Wout = Win / 2, M = B Hout Wout, W1 = [N][4][4][K1], ldw1 = 16 K1 (Conv3W.phase_weights("up2d")).       */
  CL_GEMM_CONV_S2K4 = 8
};

typedef struct cl_gemm_params {
  const void* A1; long lda1; int K1;
  const void* W1; long ldw1;          /* [N, taps*K1], K contiguous (taps = 9 in conv modes: ky,kx,c) */
  const void* A2; long lda2; int K2;  /* optional second K segment                           */
  const void* W2; long ldw2;
  int M, N;
  int mode;
  int B, Hin, Win, Hout, Wout;        /* conv geometry                                       */
  const void* zero_page;              /* zeros on the device for conv halos: >= 4*K1 + 128 bytes (16 KiB is enough for every
                                         CtrLoRA shape); the stride-1 conv path walks it like an image row     */
  const float* bias;                  /* fp32 [N] or NULL                                    */
  const void* rowbias; long ldrb; int rows_per_batch;
  const void* residual; long ldr;
  float alpha, beta;
  int act;                            /* 0 none, 1 SiLU, 2 GEGLU (value / gate rows of W interleaved per 160-row tile, C is
                                         [M, N/2]: ldm/modules/attention.py:49-56 fused into the projection; no-grad forwards),
                                         3 (ABI 7) the same fusion with W's rows in their natural [value | gate] order:
                                         bf16, K1 in {320, 640}, K2 in {0, 128}, N % 64 == 0 only -- CL_EINVAL otherwise
                                         (the full list: "x-stationary-only forms" below),
                                         4 (added in ABI 7, compatible) exact GELU 0.5 x (1 + erf(x / sqrt 2)) of the fp32 sum
                                         A1.W1^T [+ A2.W2^T] + bias [+ rowbias], before alpha and beta * residual: CLIPMLP.fc1 +
                                         activation_fn (transformers/models/clip/modeling_clip.py:346-350, hidden_act "gelu") */
  void* C; long ldc;
  int out_f32;                        /* store fp32 regardless of dtype                      */
  int atomic;                         /* fp32 atomicAdd into C (gradient accumulation)       */
  int splitk;                         /* K splits in atomic mode; otherwise chosen internally */
  /* Grouped K segments (linear mode; ABI 5): G LoRA linears that share their input (to_q | to_k | to_v of one
   * CrossAttention, cldm/lora.py:285-291 x3) as ONE product with the outputs side by side.  a2_group_n = width of one
   * linear's output: columns [g*a2_group_n, (g+1)*a2_group_n) read their second segment from columns [g*K2, (g+1)*K2)
   * of A2 (A2 = [x Aq^T | x Ak^T | x Av^T], W2 = [Bq; Bk; Bv]).  a1_group_n: the same for the FIRST segment
   * (u = [dq Bq | dk Bk | dv Bv] from dy = [dq | dk | dv]: A1 columns [g*K1, (g+1)*K1)).  0 = ungrouped. */
  int a1_group_n, a2_group_n;
  /* ABI 6: alpha multiplies output columns [0, alpha_n) only (0 = every column; a multiple of 8).  The q | k | v
   * projection of a CrossAttention writes q * (d_head^-0.5 * log2 e) and plain k, v in ONE launch: the pre-scaled-Q
   * contract of cl_attention_*_v2 (CL_ATTN_Q_PRESCALED). */
  int alpha_n;
  /* ABI 7: LayerNorm as a prologue of the product (ldm/modules/attention.py:271-275: x + attn(norm(x)) -- the norm never
   * exists in memory).  ln_gamma != NULL: A1 holds the UN-normalised rows and the kernel forms (row - mean) * rstd * gamma
   * + beta over the K1 columns before the contraction (fp32 statistics; rounded to `dtype` like cl_layernorm_fwd's output).
   * ln_stats (may be NULL): [M][2] fp32 {mean, rstd} for cl_layernorm_bwd.  bf16, linear mode, K1 in {320, 640}, K2 = 0,
   * no rowbias / residual only -- CL_EINVAL otherwise (the caller then runs cl_layernorm_fwd itself; the full list:
   * "x-stationary-only forms" below). */
  const float* ln_gamma; const float* ln_beta; float ln_eps; float* ln_stats;
  /* Argument restrictions (CL_EINVAL otherwise; checked before any tile configuration is chosen, so they hold for every
   * configuration alike -- tests/test_gpu_gemm_conformance.py):
   *   - N % 8 == 0 and ldc % 8 == 0 (outputs are stored as whole 8-element vectors); K1 > 0;
   *   - K1 and K2 multiples of 32 (bf16) / 16 (fp32): one 64-byte substep row;
   *   - splitk > 1 only with atomic (without it the split factor is the library's choice); with atomic and splitk > 1 no
   *     activation (act == 0): every split adds its partial product, bias / rowbias / residual enter once;
   *   - rowbias needs rows_per_batch > 0; conv modes need zero_page;
   *   - act 2 (GEGLU): N % 160 == 0, no rowbias, no residual, no atomic, alpha == 1 and alpha_n == 0;
   *   - act 4 (GELU): no atomic, no LayerNorm prologue; the split factor stays the library's choice, and the activation is
   *     applied to the reduced sum (in the split-K reduce), never per split.  Every tile configuration honours it in both
   *     dtypes; a forced / tabled configuration of the x-stationary or the loader / consumer kernel hands the product to the
   *     rules (those two kernels have no GELU epilogue), so no configuration returns an un-activated product;
   *   - a second K segment (K2 > 0) and grouped segments exist in CL_GEMM_LINEAR only;
   *   - alpha_n a multiple of 8 in [0, N]; a group width divides N, a2_group_n needs K2 > 0, and some tile width (64, 128
   *     or 160 columns) must divide every group width: a tile never straddles two groups.
   * x-stationary-only forms: act 3 and the LayerNorm prologue (ln_gamma != NULL) have one kernel (csrc/gemm_xs.hip) and no
   * fall-back, so what that kernel's launcher refuses is CL_EINVAL for the call (tests/test_gemm_xs_reference_model.py holds
   * the table).  Both, beyond the restrictions above (the alpha_n and group ranges included):
   *   - bf16 storage, CL_GEMM_LINEAR, no atomic, no out_f32, no rowbias, no a1_group_n;
   *   - M >= 128 (a workgroup owns 128 rows; rows past M repeat row M - 1);
   *   - K1 in {320, 640};
   *   - lda1, ldw1, ldc (and lda2, ldw2 with K2, ldr with a residual) multiples of 8: every access is a 16-byte vector;
   *   - alpha_n a multiple of 32 (alpha changes between 32-column output blocks);
   *   - a2_group_n a multiple of 32 that divides N, with K2 > 0.
   * act 3 only: N % 64 == 0 (C is [M, N / 2], whole 32-column blocks), K2 in {0, 128}, no residual, alpha == 1,
   *   alpha_n == 0, a2_group_n == 0.
   * LayerNorm prologue only: act 0 (N % 32 == 0) or act 3; ln_beta != NULL; K2 == 0; no residual.
   * (Products WITH a fall-back never see these as refusals: where the x-stationary kernel is forced or tabled for a plain or
   * residual product it does not take, the tile kernels run it.)  C == residual (in place) is part of the contract for every
   * configuration: an element is read and written by its owner only.  (It needs C stored in `dtype`, like the residual: a bf16
   * product with out_f32 has no element that is both.)  tests/test_gpu_gemm_conformance.py launches every configuration in
   * place -- linear, a second K segment, rowbias + SiLU, forced split-K (the reduce reads the residual and writes C), conv S1 and
   * CL_GEMM_CONV_S2A -- and asserts the bits of the out-of-place launch; tests/test_gpu_gemm_xs_conformance.py does the same for
   * the x-stationary forms.  CL_GEMM_CONV_S2A is in the same file's Layer C (even and odd grids; the full-line and the
   * loader / consumer kernel at a size they take themselves) against tests/gemm_ref.py's fp64 model of the mode.
   * rowbias and residual are read in `dtype` ([M / rows_per_batch, N] and [M, N]); with atomic, C is fp32 and the product is
   * added onto what it holds. */
} cl_gemm_params;

/* Generic entry; the named operators below are thin fillers of cl_gemm_params. */
int cl_gemm(const cl_gemm_params* p, int dtype, void* stream);

/* LoRACompatibleLinear.forward (cldm/lora.py:285-291): y = x W^T + b + (x A^T) B^T (+ residual).
 * t = x A^T (LoRALinearLayer.down, cldm/lora.py:74) is produced by cl_lora_down and kept for
 * the backward pass; the up-projection is folded into the main MFMA chain as a second K segment.
 * W [N,K], A [r,K], Bup [N,r] row-major in `dtype`; pass t = NULL / r = 0 for a plain nn.Linear. */
int cl_lora_down(int dtype, const void* x, long ldx, const void* A, int r, void* t, long ldt,
                 int M, int K, void* stream);
int cl_lora_linear_fwd(int dtype, const void* x, long ldx, const void* W, const float* bias,
                       const void* t, long ldt, const void* Bup, int r,
                       const void* residual, long ldr, int act, void* y, long ldy,
                       int M, int N, int K, void* stream);
/* data gradient: dx = dy W + (dy B) A (+ accum).  Wt = W^T [K,N], At = A^T [K,r], Bt = B^T [r,N];
 * u = dy B [M,r] is written to `u` (needed again for dA).  No dW is ever formed for frozen W. */
int cl_lora_linear_bwd_data(int dtype, const void* dy, long lddy, const void* Wt, const void* At,
                            const void* Bt, int r, void* u, long ldu, const void* accum, long ldacc,
                            void* dx, long lddx, int M, int N, int K, void* stream);
/* weight gradient of a (LoRA / zero-conv) matrix: dW[N,K] += dyT[N,Mp] . xT[K,Mp]^T, fp32 atomics.
 * dyT / xT are the zero-padded transposes produced by cl_transpose (Mp multiple of 32). */
int cl_weight_grad(int dtype, const void* dyT, long lddyt, const void* xT, long ldxt, float* dW,
                   long lddw, int N, int K, int Mp, float scale, void* stream);

/* the same weight gradient without materialised transposes (bf16 only): dW[N,K] += scale * dy[M,N]^T . x[M,K],
 * both operands row-major as the forward/backward pass left them; fragments are built with the gfx950 LDS
 * transpose read (csrc/wgrad.hip).  zero_page: >= 64 zero bytes on the device (rows past M; >= 64 bytes). */
int cl_weight_grad_tn(int dtype, const void* dy, long lddy, const void* x, long ldx, float* dW, long lddw,
                      int M, int N, int K, float scale, const void* zero_page, void* stream);

/* grouped form: n independent weight gradients in ONE launch (+ one slab-reduce launch).  The LoRA
 * matrices are small, so a single problem cannot fill the chip; the engine queues the problems of a
 * transformer block and flushes them together.  `descs` is a HOST array (copied into the kernel arguments,
 * hipGraph-replayable). */
typedef struct cl_wgrad_desc {
  const void* dy; long lddy;      /* [M, N] row-major bf16 */
  const void* x; long ldx;        /* [M, K] row-major bf16 */
  float* dW; long lddw;           /* [N, K] fp32, accumulated */
  int M, N, K; float scale;
  /* tap >= 0: ONE TAP of a 3x3 convolution's weight gradient (Base-ControlNet pre-training trains the conv weights,
   * cldm/cldm_ctrlora_pretrain.py:174-182).  x is then the NHWC input [B*Hin*Win, K]; row m = (b, oy, ox) of dy pairs
   * with input pixel (oy*stride + tap/3 - pad, ox*stride + tap%3 - pad), zero outside the image; dW points at the tap's
   * [N, K] slice of a [N][3][3][K] gradient (lddw = 9 K).  tap = -1: plain dy^T x (the other fields are ignored).
   * tap = 16 + ky (stride 1, pad 1, Wout a multiple of 32 or 8 or 16, M a multiple of 32): the THREE taps (ky, 0..2) of a
   * kernel row from one problem -- dW points at tap (ky, 0), taps kx = 1, 2 lie K and 2 K floats further on in each row. */
  int tap, Hin, Win, Hout, Wout, stride, pad, reserved;
} cl_wgrad_desc;
/* Refused with CL_EINVAL (cl_weight_grad_tn as the one-descriptor case with tap = -1): dtype not bf16; zero_page null; descs null or
 * n > 4096; N or K not a multiple of 8 or below 8; lddy / ldx not multiples of 8, lddw not a multiple of 4; lddy < N, ldx < K,
 * lddw < K (lddw < 3 K for tap >= 16); dy, x or dW null, dW not 16-byte aligned; tap in 9 .. 15 or above 18; with tap >= 0: Hin, Win,
 * Hout or Wout outside 1 .. 32767, pad outside 0 .. 32767, stride not 1 or 2, M not a multiple of Hout Wout; with tap >= 16 also:
 * stride != 1, pad != 1, Hin != Hout, Win != Wout, M not a multiple of 32, Wout neither a multiple of 32 nor 8 nor 16 (Wout = 4, 2, 1
 * were accepted before and computed a wrong gradient).  Every descriptor is checked before anything is launched: a refused call has
 * accumulated into NO dW of the group.  Descriptors with M, N or K <= 0 are skipped. */
int cl_weight_grad_tn_group(int dtype, int n, const cl_wgrad_desc* descs, const void* zero_page, void* stream);

/* 3x3 convolutions of ResBlock / Downsample / Upsample / input conv / out conv
 * (ldm/modules/diffusionmodules/openaimodel.py:108-118,150,203,229,729; cldm/cldm.py:141):
 * out = conv(x) + bias + emb[b, :] (openaimodel.py:272) + residual (openaimodel.py:274).
 * Wp = [Cout][ky][kx][Cin] in `dtype`.  mode is one of CL_GEMM_CONV_*. */
int cl_conv3x3_fwd(int dtype, int mode, const void* x, long ldx, const void* Wp, const float* bias,
                   const void* emb, long ldemb, const void* residual, long ldr, void* y, long ldy,
                   int B, int Hin, int Win, int Cin, int Cout, const void* zero_page, void* stream);
/* data gradient: same kernel on the tap-flipped, in/out-swapped weights Wd = [Cin][2-ky][2-kx][Cout]
 * (mode CL_GEMM_CONV_S1 for stride-1 convs, CL_GEMM_CONV_T2 for the stride-2 Downsample). */
int cl_conv3x3_bwd_data(int dtype, int mode, const void* dy, long lddy, const void* Wd,
                        const void* accum, long ldacc, void* dx, long lddx,
                        int B, int Hdy, int Wdy, int Cout, int Cin, const void* zero_page, void* stream);

/* 1x1 convs (SpatialTransformer.proj_in/out, ResBlock.skip_connection, ControlNet zero convs,
 * cldm/cldm.py:281-282) with the ControlNet residual injection fused in
 * (cldm_ctrlora_finetune.py:79, cldm/cldm.py:35,41):  y = (x W^T + b) * scale + beta * residual. */
int cl_conv1x1_fwd(int dtype, const void* x, long ldx, const void* W, const float* bias, float scale,
                   const void* residual, long ldr, float beta, void* y, long ldy,
                   int M, int Cin, int Cout, void* stream);

/* ---- normalisation ------------------------------------------------------------------- */
/* GroupNorm32(groups, C) [+ SiLU] in fp32 statistics (util.py:217-219; openaimodel.py:201-202) over token-major
 * [B * HW, C] operands.  cl_groupnorm_ws_floats(B, HW, C) floats of scratch in `ws` (either direction).
 * cl_groupnorm_silu_fwd: y = silu?(gamma (x - mean) rstd + beta); stats [B][groups][2] = {mean, rstd} in fp32 is always
 * written (the backward reads it).  Argument restrictions (CL_EINVAL otherwise, nothing launched, nothing written --
 * tests/test_gpu_norm_conformance.py):
 *   - C % 8 == 0, C % groups == 0, C <= 8192, and C / 8 <= 320 or a multiple of 320: C <= 2560, or C in {5120, 7680}
 *     (C = 4096 is refused);
 *   - ldx % 8 == 0 and ldy % 8 == 0 (rows are read and written as 16-byte vectors; x and y may be column slices of wider
 *     buffers at an offset that is a multiple of 8 elements, and 16-byte aligned). */
long cl_groupnorm_ws_floats(int B, int HW, int C);
int cl_groupnorm_silu_fwd(int dtype, const void* x, long ldx, void* y, long ldy, const float* gamma,
                          const float* beta, int B, int HW, int C, int groups, float eps, int silu,
                          float* stats, float* ws, void* stream);
/* cl_groupnorm_silu_bwd: dx = (accum ? accum : 0) + grad of the forward at dy, from x and the forward's stats; dgamma /
 * dbeta (both or neither; fp32 [C]) are ACCUMULATED onto what they hold (fp32 atomics: not bit-reproducible).
 * Argument restrictions (CL_EINVAL otherwise, nothing launched, nothing written):
 *   - those of the forward on C and groups;
 *   - ldx, lddy, lddx % 8 == 0, and ldacc % 8 == 0 when accum != NULL;
 *   - dgamma and dbeta both NULL or both given. */
int cl_groupnorm_silu_bwd(int dtype, const void* x, long ldx, const void* dy, long lddy,
                          const void* accum, long ldacc, void* dx, long lddx, const float* gamma,
                          const float* beta, const float* stats, int B, int HW, int C, int groups,
                          int silu, float* dgamma, float* dbeta, float* ws, void* stream);
/* nn.LayerNorm over the last dim (attention.py:263-265), two-pass fp32 statistics; stats (may be NULL) = [M][2] fp32
 * {mean, rstd} for the backward.  Argument restrictions (CL_EINVAL otherwise, nothing launched, nothing written):
 *   - D % 8 == 0 and D <= 1536 (a row lives in the registers of one wave);
 *   - ldx % 8 == 0 and ldy % 8 == 0. */
int cl_layernorm_fwd(int dtype, const void* x, long ldx, void* y, long ldy, const float* gamma,
                     const float* beta, int M, int D, float eps, float* stats, void* stream);
/* dx = (accum ? accum : 0) + grad; dgamma / dbeta (both or neither; fp32 [D]) are ACCUMULATED onto what they hold: through
 * the registered scratch + a finishing launch (deterministic) or, without one, fp32 atomics (cl_set_workspace).
 * Argument restrictions (CL_EINVAL otherwise, nothing launched, nothing written):
 *   - D % 8 == 0 and D <= 1536;
 *   - ldx, lddy, lddx % 8 == 0, and ldacc % 8 == 0 when accum != NULL;
 *   - dgamma and dbeta both NULL or both given. */
int cl_layernorm_bwd(int dtype, const void* x, long ldx, const void* dy, long lddy, const void* accum,
                     long ldacc, void* dx, long lddx, const float* gamma, const float* stats, int M,
                     int D, float* dgamma, float* dbeta, void* stream);

/* ---- attention ----------------------------------------------------------------------- */
/* CrossAttention.forward core (attention.py:171-192): softmax(q k^T d^-1/2) v per head, fp32
 * scores/softmax, never materialising the score matrix.  Vt / Qt / dOt / Kt are the
 * [B][H*dh][pad64] transposes made with cl_transpose.  LSE (may be NULL in the forwards) is
 * [B][H][lse_stride] fp32 with lse_stride a multiple of 64 and >= N; CL_EINVAL otherwise, in every entry point. */
int cl_attention_fwd(int dtype, const void* Q, long ldq, const void* K, long ldk, const void* Vt,
                     int nkv_pad, void* O, long ldo, float* LSE, int lse_stride, int B, int H, int N,
                     int Nkv, int dh, float scale, void* stream);
int cl_attention_bwd(int dtype, const void* Q, long ldq, const void* K, long ldk, const void* V,
                     long ldv, const void* O, long ldo, const void* dO, long lddo, const void* Qt,
                     const void* dOt, int n_pad, const void* Kt, int nkv_pad, const float* LSE,
                     float* Delta, int lse_stride, void* dQ, long lddq, void* dK, long lddk, void* dV,
                     long lddv, int B, int H, int N, int Nkv, int dh, float scale, void* stream);

/* bf16 variants without any materialised transposes (csrc/attention_tr.hip): every tile is staged
 * row-major as the projections wrote it and the P.V-type operands are built with the gfx950 LDS
 * transpose read.  V is [B*Nkv, ldv] like K.  fp32 parity mode keeps the entry points above.
 * flags (ABI 6): CL_ATTN_Q_PRESCALED -- Q holds q * scale * log2(e): the to_q projection applied the factor in its own
 * fp32 epilogue (cl_gemm_params.alpha / alpha_n), so the kernels read log2-domain scores straight off the matrix
 * product (for d_head 40 the forward also carries -max through a spare contraction slot: no per-score multiply-add
 * at all).  `scale` is still d_head^-0.5; O, LSE, dQ, dK, dV mean the same with or without the flag (gradients are
 * those of the TRUE q, k, v).  An explicit argument of every call -- no process-global state selects it. */
enum { CL_ATTN_Q_PRESCALED = 1 };
int cl_attention_fwd_v2(int dtype, const void* Q, long ldq, const void* K, long ldk, const void* V, long ldv,
                        void* O, long ldo, float* LSE, int lse_stride, int B, int H, int N, int Nkv, int dh,
                        float scale, int flags, void* stream);
int cl_attention_bwd_v2(int dtype, const void* Q, long ldq, const void* K, long ldk, const void* V, long ldv,
                        const void* O, long ldo, const void* dO, long lddo, const float* LSE, float* Delta,
                        int lse_stride, void* dQ, long lddq, void* dK, long lddk, void* dV, long lddv,
                        int B, int H, int N, int Nkv, int dh, float scale, int flags, void* row_ws, void* stream);
/* Decoupled image-prompt cross-attention forward (IP-Adapter, ldm/modules/attention_ip.py IPCrossAttention):
 *   O = softmax(scale q K^T) V + ip_scale * softmax(scale q Kip^T) Vip
 * two separate softmaxes, fp32 scores, one launch (Q read once, O written once).  Kip / Vip hold Nip (1..64) keys per
 * batch sample, Kip [B*Nip, ldkip].  V / Vip follow the plain forward of the dtype: bf16 as cl_attention_fwd_v2 (row-major,
 * ldv / ldvip are row pitches; CL_ATTN_Q_PRESCALED allowed), fp32 as cl_attention_fwd (transposed [B][H*dh][pad] and zero
 * padded: ldv / ldvip are the key pitches, multiples of 64).  Forward only, no LSE.  Added in ABI 7 (compatible). */
int cl_attention_fwd_ip(int dtype, const void* Q, long ldq, const void* K, long ldk, const void* V, long ldv,
                        const void* Kip, long ldkip, const void* Vip, long ldvip, void* O, long ldo, int B, int H,
                        int N, int Nkv, int Nip, int dh, float scale, float ip_scale, int flags, void* stream);
/* Causal self-attention forward (CLIPTextTransformer: the causal mask of modeling_clip.py added to CLIPAttention's scores),
 * added in ABI 7 (compatible):   O[b, i, h] = softmax_{j <= i}(scale q_i . k_j) v_j,   N queries = N keys, no LSE.
 * Q / K / V / O are row-major [B*N, ld] with head h at columns [h*dh, (h+1)*dh), as in cl_attention_fwd_v2; bf16 or fp32.
 * fp32 scores and softmax; the unnormalised P is rounded to `dtype` before P.V, O once on the store.  CL_EINVAL, nothing
 * launched, for dh != 64, N < 1 or N > 128, a row pitch that is not a multiple of 16 bytes or is narrower than H*dh, a
 * null or not 16-byte aligned pointer. */
int cl_attention_causal_fwd(int dtype, const void* Q, long ldq, const void* K, long ldk, const void* V, long ldv,
                            void* O, long ldo, int B, int H, int N, int dh, float scale, void* stream);
/* row_ws (ABI 6; may be NULL): scratch of B * H * lse_stride * 32 bytes, 16-byte aligned.  With CL_ATTN_Q_PRESCALED and
 * d_head 40 the backward kernels keep (-lse, -delta) of every query row there as bf16 triples and feed them through spare
 * contraction slots of the matrix products, which then deliver s - lse and dP - delta (attention.py:171-192's backward with
 * 3 instead of 5 vector instructions per score pair).  Results are the same with or without it. */

/* ---- elementwise / layout ------------------------------------------------------------ */
/* Every entry point below decides its refusals on the host: CL_EINVAL, nothing launched, nothing written.  Common to all of them:
 * a dtype other than CL_BF16 / CL_F32 where there is a dtype argument, and a null required pointer (optional ones are named; a call
 * with nothing to do -- n == 0, M == 0 -- returns CL_OK whatever its pointers).  The rest is listed per entry point. */
/* cl_geglu_fwd / _bwd: F % 8, a leading dimension % 8, ldh < 2 F, ldo (lddo) < F, lddh < 2 F, M < 0, a base pointer not 16-byte aligned.
 * cl_silu_fwd / _bwd: n % 8, n < 0, a pointer not 16-byte aligned.  cl_axpby: C % 8, ldx / ldy % 8 or < C, M < 0, a pointer not
 * 16-byte aligned; y is not read when b == 0. */
int cl_geglu_fwd(int dtype, const void* h, long ldh, void* out, long ldo, long M, int F, void* stream); /* attention.py:55-56 */
int cl_geglu_bwd(int dtype, const void* h, long ldh, const void* dout, long lddo, void* dh, long lddh, long M, int F, void* stream);
int cl_silu_fwd(int dtype, const void* x, void* y, long n, void* stream);
int cl_silu_bwd(int dtype, const void* x, const void* dy, void* dx, long n, void* stream);
int cl_axpby(int dtype, const void* x, long ldx, void* y, long ldy, long M, int C, float a, float b, void* stream);
/* cl_transpose ([Bt][R][C] -> [Bt][C][Rpad], rows [R, Rpad) zero), cl_nchw_to_tok, cl_tok_to_nchw: a dtype pair other than
 * fp32 -> bf16, fp32 -> fp32, bf16 -> bf16; Rpad < R, ldo < Rpad (Cpad < Cin, ldo < Cpad); a batch outside 1 .. 65535 (it is grid.z); an
 * empty dimension (R, C, Cin, HW < 1); more than 65535 column tiles.  cl_tok_to_nchw does not read out when beta == 0. */
int cl_transpose(int in_dtype, int out_dtype, const void* in, long ldi, long bsi, void* out, long ldo,
                 long bso, int Bt, int R, int C, int Rpad, void* stream);
int cl_nchw_to_tok(int dtype, const float* in, void* out, long ldo, int B, int Cin, int Cpad, int HW, void* stream);
int cl_tok_to_nchw(int dtype, const void* in, long ldi, float* out, int B, int C, int HW, float alpha, float beta, void* stream);
/* cl_colsum: B outside 1 .. 65535, HW < 1, C < 8, C % 8, ldi % 8, ldi < C, ldo < C, in not 16-byte aligned.
 * cl_pool2x2: C % 8, ldi / ldo % 8 or < C, a negative dimension, a pointer not 16-byte aligned; out is not read when accumulate == 0.
 * cl_pack2d: Cpad < C, ldo < Cpad, ldi < C, R < 0. */
/* out[b][c] += scale * sum_p in[b*HW + p][c]  (zero-conv bias gradients, time-embedding gradients) */
int cl_colsum(int dtype, const void* in, long ldi, float* out, long ldo, int B, int HW, int C, float scale, void* stream);
int cl_pool2x2(int dtype, const void* in, long ldi, void* out, long ldo, int B, int H, int W, int C, int accumulate, void* stream);
int cl_pack2d(int dtype, const float* in, long ldi, void* out, long ldo, long R, int C, int Cpad, void* stream);
/* CLIPVisionEmbeddings.forward (transformers/models/clip/modeling_clip.py:202-218, transformers 5.x), added in ABI 7 (compatible).
 * cl_vit_patch_rows: NCHW fp32 pixel_values [B, C, S, S] -> patch rows [B (S/P)^2, Kpad] in `dtype` (row stride ldo); row
 * (b, gy, gx), columns ordered (c, py, px) as nn.Conv2d's weight [hidden, C, P, P] flattens, columns [C P P, Kpad) zero
 * (Kpad = C P P rounded up to the K granularity of cl_gemm, a multiple of 8: 588 -> 608).  The patch embedding -- a stride-P
 * P x P convolution without bias (:148-154 patch_embedding) -- is then ONE CL_GEMM_LINEAR product against the zero-padded
 * flattened weight.  S % P == 0; pixels and out 16-byte aligned.
 * cl_vit_tokens: out[b, 0, :] = cls + pos[0], out[b, 1 + i, :] = patch[b (T - 1) + i, :] + pos[1 + i] (:212-217: the class
 * embedding concatenated in front, + position_embedding): cls [D], pos [T, D] fp32, patch / out in `dtype`, the add in fp32,
 * one rounding.  D % 8 == 0.  A launch of its own rather than an epilogue of the patch product: rowbias indexes by sample,
 * not by token, and the class rows shift every sample's output rows, so the epilogue form would need a class-row kernel as
 * well -- two launches either way, and this one leaves cl_gemm as it is. */
int cl_vit_patch_rows(int dtype, const float* pixels, void* out, long ldo, int B, int C, int S, int P, int Kpad, void* stream);
int cl_vit_tokens(int dtype, const void* patch, long ldp, const float* cls, const float* pos, void* out, long ldo, int B, int T,
                  int D, void* stream);
/* CLIPTextEmbeddings.forward (modeling_clip.py: token_embedding(input_ids) + position_embedding), added in ABI 7 (compatible):
 * out[b T + t, :] = tok[ids[b, t], :] + pos[t, :]; ids [B, T] int64, tok [vocab, D] and pos [>= T, D] fp32, out in `dtype`, the
 * add in fp32, one rounding.  D % 8 == 0.  An id outside [0, vocab) is clamped in the kernel: it never reads out of range.
 * cl_gather_rows: dst[r, :] = src[rows[r], :] for r < R (the pooled end-of-text rows); rows int64 on the device, an index
 * outside [0, nsrc) clamped.  D % 8 == 0, pitches multiples of 8 elements, pointers 16-byte aligned (ids / rows 8-byte). */
int cl_clip_text_embed(int dtype, const long* ids, const float* tok, const float* pos, void* out, long ldo, int B, int T, int D,
                       int vocab, void* stream);
int cl_gather_rows(int dtype, const void* src, long lds, const long* rows, void* dst, long ldd, int R, int D, int nsrc, void* stream);
/* One-launch refresh of the engine's storage-dtype copies of all trainable matrices from the flat fp32
 * master buffer after an optimizer step.  desc = device table of 8 longs per matrix {src offset in floats,
 * rows << 32 | cols, dst [rows][cols] or 0, dst^T [cols][rows] or 0, source row stride (0 = cols), dst row stride
 * (0 = cols), dst^T row stride (0 = rows), reserved}; the strides let one 3x3-conv weight [O][9][I] be re-packed tap
 * by tap into [O][9][I_pad] and the tap-flipped data-gradient form [I][9][O_pad].  tile_prefix[i] = number of 32x32
 * tiles before matrix i (ndesc + 1 entries). */
int cl_repack(int dtype, const float* flat, const long* desc, const int* tile_prefix, int ndesc,
              int total_tiles, void* stream);
/* Both embeddings refuse B < 1, half < 1, B half > INT_MAX and ldo < 2 half. */
/* timestep_embedding (util.py:154-174); freqs = the fp32 table exp(-ln(1e4) * arange(half)/half) */
int cl_timestep_embedding(int dtype, const long* t, const float* freqs, void* out, long ldo, int B, int half, void* stream);
/* The same embedding at floating-point times (added in ABI 7, compatible): the argument is t[b] * freqs[j] in fp32, cos | sin
 * rounded once into `dtype`; an integer-valued t gives the bits of cl_timestep_embedding.  The DPM-Solver++ time grid
 * (ldm/models/diffusion/dpm_solver) is not integer: 999, 949.05, 899.1, ... for 20 steps. */
int cl_timestep_embedding_f(int dtype, const float* t, const float* freqs, void* out, long ldo, int B, int half, void* stream);

/* out[m, :] = x[pixel(m, tap), :] (zero outside the image), m = (b, oy, ox), pixel = (oy*stride + tap/3 - pad,
 * ox*stride + tap%3 - pad): the shifted operand of one tap of a 3x3 conv weight gradient, materialised (fp32 parity
 * mode; the bf16 weight-gradient kernel gathers in its own addressing, see cl_wgrad_desc.tap). */
/* Refused: C % 8, C < 8, ldx / ldo % 8 or < C, tap outside 0 .. 8, stride < 1, an empty dimension (B, Hin, Win, Hout, Wout < 1), a
 * pointer not 16-byte aligned. */
int cl_conv_tap_gather(int dtype, const void* x, long ldx, void* out, long ldo, int B, int Hin, int Win, int Hout,
                       int Wout, int C, int tap, int stride, int pad, void* stream);
/* Row softmax for the VAE's single-head attention (ldm/modules/diffusionmodules/model.py:183-186): fp32 scores
 * S [M, N] (row stride lds) -> `dtype` probabilities P [M, N] (row stride ldp), P = softmax(S * scale) per row. */
/* Refused: N % 4, N < 4, N > 8192, lds / ldp % 4 or < N, M < 1, S not 16-byte aligned, P not 8-byte (bf16) / 16-byte (fp32) aligned. */
int cl_softmax_rows(int dtype, const float* S, long lds, void* P, long ldp, long M, int N, float scale, void* stream);

/* ---- diffusion bookkeeping ------------------------------------------------------------ */
/* Forward process (q_sample, alone or blended into a masked sampling step), the first-stage posterior sample, the losses, the
 * fused sampler updates and the optimizer step.
 * Refusals of the entry points below, besides null required pointers (optional: d_eps, e_u, noise, pred_x0, lvlb, per_sample): a
 * negative n / B / per_sample; cl_p_losses_mse B outside 1 .. 65535, per_sample_elems < 1, lvlb without t; cl_ddim_step index < 0;
 * cl_adamw_dev needs hyper and step even when n == 0.  cl_zero(p, 0) is CL_OK.  cl_qsample_blend lists its own. */
/* DDPM.q_sample (ddpm.py:356-359): out = sqrt_ac[t_b] * z + sqrt_1mac[t_b] * noise */
int cl_qsample(const float* z, const float* noise, const long* t, const float* sqrt_ac, const float* sqrt_1mac,
               float* out, int B, long per_sample, void* stream);
/* One masked sampling step's blend (cldm/ddim_hacked.py:154-157 with ddpm.py q_sample), added in ABI 7 (compatible):
 *   out[b, c, p] = (sqrt_ac[t_b] * x0 + sqrt_1mac[t_b] * noise) * m + (1 - m) * x,  m = mask[(mask_per_batch ? b : 0),
 *   (mask_per_channel ? c : 0), p] -- the four mask layouts (B | 1, C | 1, H, W); x0 / noise / x / out = [B][C][HW] fp32; t_b is
 * clamped to [0, T - 1] (the tables hold T entries).  Every torch fp32 op rounded once, no FMA: q = rn(rn(sa x0) + rn(s1 noise)),
 * out = rn(rn(q m) + rn(rn(1 - m) x)) -- the bits of cl_qsample followed by the three torch ops.  out may be x (in place).
 * 16-byte loads and stores where HW % 4 == 0 and x0 / noise / mask / x / out are 16-byte aligned, scalar otherwise.  No host
 * synchronisation, no allocation; the time comes from device memory, so a captured launch replays unchanged.
 * Refused: B < 0, C < 1, HW < 1, T < 1; with B > 0 a null pointer, out overlapping x0 / noise / mask, out overlapping x without
 * being x.  B == 0 is CL_OK. */
int cl_qsample_blend(const float* x0, const float* noise, const long* t, const float* sqrt_ac, const float* sqrt_1mac,
                     int T, const float* mask, int mask_per_batch, int mask_per_channel, const float* x, float* out,
                     int B, int C, long HW, void* stream);
/* LatentDiffusion.get_first_stage_encoding on a stored posterior (ddpm.py:655-662, distributions.py:35-37), added in ABI 7
 * (compatible): out = scale * (mean + std * e), fp32, for one tensor or for two of the same shape in ONE launch (target and
 * condition of a training batch).  mom_* = [B][2 per_sample] (mean, then std, of each sample); e_* and out_* = [B][per_sample].
 * A rounded product, a rounded sum, a rounded product, no FMA: the bits of the three torch fp32 ops.  16-byte loads and stores
 * where per_sample % 4 == 0 and every pointer is 16-byte aligned, scalar otherwise.  No host synchronisation, no allocation.
 * Refused: a null mom_a / e_a / out_a, B < 1, per_sample < 1, a second tensor given in part (mom_b, e_b, out_b: all or none). */
int cl_posterior_sample_pair(const float* mom_a, const float* e_a, float* out_a, const float* mom_b, const float* e_b,
                             float* out_b, int B, long per_sample, float scale, void* stream);
/* p_losses MSE (ddpm.py:902-918): *loss = mean((eps - target)^2); d_eps = 2 (eps - target) / n * gscale */
int cl_mse_loss(const float* eps, const float* target, float* d_eps, float* loss, long n, float gscale, void* stream);
/* LatentDiffusion.p_losses' reduction, deterministic (ddpm.py:902-918, eps-parameterisation, logvar == 0):
 *   out[0] = loss_simple = mean_b mean_chw (eps - target)^2        out[1] = loss_vlb = mean_b lvlb[t_b] * (per-sample mean)
 *   out[2] = loss = w_simple * loss_simple + w_elbo * loss_vlb     per_sample[B] (optional) = per-sample means
 *   d_eps (optional) = d (w_simple * loss_simple) / d eps * gscale.  scratch: 16 * B floats.  lvlb may be NULL. */
int cl_p_losses_mse(const float* eps, const float* target, float* d_eps, const long* t, const float* lvlb, float* out,
                    float* per_sample, float* scratch, int B, long per_sample_elems, float gscale, float w_simple,
                    float w_elbo, void* stream);
/* The same reduction with a per-timestep weight and a choice of loss, added in ABI 7 (compatible).  Not in the reference: wt is
 * meant for Min-SNR-gamma weights min(SNR_t, gamma) / SNR_t, kind 1 is torch.nn.functional.huber_loss.  With d = eps - target:
 *   kind 0 (l2)     rho(d) = d^2,                                              rho'(d) = 2 d
 *   kind 1 (Huber)  rho(d) = |d| <= delta ? d^2 / 2 : delta (|d| - delta / 2), rho'(d) = clamp(d, -delta, delta)
 *   l_b = mean_chw rho(d)        per_sample[b] (optional) = l_b        (both unweighted)
 *   out[0] = loss_simple = mean_b l_b (unweighted)      out[1] = loss_vlb = mean_b lvlb[t_b] l_b
 *   out[2] = loss = w_simple * mean_b (wt[t_b] l_b) + w_elbo * loss_vlb
 *   d_eps (optional) = gscale * w_simple * wt[t_b] * rho'(d) / (per_sample_elems * B)   (the elbo term is not differentiated)
 * wt = fp32 [T] indexed by t_b, NULL = all ones; lvlb may be NULL; delta is read for kind 1 only.  t_b is not range-checked: the
 * caller's tables hold an entry for every t it passes.  Deterministic (no float atomics, fixed summation order), no host
 * synchronisation, no allocation; t, wt and lvlb are read from device memory, so a captured launch follows values that change
 * between replays.  scratch: 16 * B floats.  With wt == NULL and kind == 0 every output has the bits of cl_p_losses_mse.
 * Refused before anything is launched: what cl_p_losses_mse refuses (a null eps / target / out / scratch, B outside 1 .. 65535,
 * per_sample_elems < 1, lvlb without t), wt without t, kind outside {0, 1}, kind 1 with a delta that is not finite or <= 0. */
int cl_p_losses_w(const float* eps, const float* target, float* d_eps, const long* t, const float* lvlb, float* out,
                  float* per_sample, float* scratch, int B, long per_sample_elems, float gscale, float w_simple,
                  float w_elbo, const float* wt, int kind, float delta, void* stream);
/* The per-sample losses of a p_losses call broken down by timestep band, added in ABI 7 (compatible).  Not in the reference
 * (its validation_step, ddpm.py:457-463, logs one mean at random t):
 *   acc = device double [nbands + 1][3], row k = {count, sum, sum of squares} of band k, row nbands = of all samples
 *   band(t) = min(clamp(t, 0, T - 1) * nbands / T, nbands - 1)     (64-bit integer arithmetic)
 * The launch ADDS to what acc holds (clear it with cl_zero).  n_valid = NULL: all B samples count; else a device int, read on
 * the device: the first clamp(*n_valid, 0, B) samples count (a ragged last batch padded to a captured shape replays unchanged).
 * Sums and squares are formed in fp64 from the fp32 loss and added in index order within each row by one workgroup: no
 * atomics, no waiting, no host synchronisation, no allocation; the bits of the sequential fp64 loop on every launch and
 * replay.  A non-finite per_sample[b] reaches its own band's row and the total row only.
 * Refused before anything is launched: a null per_sample / t / acc, B outside 1 .. 65535, T < 1, nbands outside
 * 1 .. min(T, 64), acc not 8-byte aligned. */
int cl_loss_bands(const float* per_sample, const long* t, int B, int T, int nbands, const int* n_valid, double* acc,
                  void* stream);
/* optimizer.zero_grad() / accumulator clears without an ATen launch: a fill KERNEL on `stream` (not hipMemsetAsync: memset
   nodes of small buffers were mis-ordered when a step is replayed as several consecutive hipGraphs) */
int cl_zero(void* p, long nbytes, void* stream);
/* DDIMSampler.p_sample_ddim update (cldm/ddim_hacked.py:192,203-231); coef = device [S][4] fp32 table
 * {a_t, a_prev, sigma_t, sqrt(1-a_t)}; e_u = NULL disables classifier-free guidance. */
int cl_ddim_step(const float* x, const float* e_c, const float* e_u, const float* noise, const float* coef,
                 int index, float scale, float* x_prev, float* pred_x0, long n, void* stream);
/* torch.optim.AdamW step over one flat fp32 buffer (cldm_ctrlora_finetune.py:105) */
int cl_adamw(float* p, const float* g, float* m, float* v, long n, float lr, float beta1, float beta2,
             float eps, float weight_decay, int step, float grad_scale, void* stream);

/* ---- device-resident step state: what a captured hipGraph needs --------------------------
 * A replayed graph re-issues the same kernel arguments, so per-step scalars live in device memory.
 * cl_tick: *counter += 1.  cl_adamw_dev: AdamW with hyper = device {lr, beta1, beta2, eps, weight_decay,
 * grad_scale} and a device step counter that the CALLER advances with cl_tick once per optimizer step, before the
 * first cl_adamw_dev of that step (one tick however many parameter banks follow; torch increments first too).  cl_ddim_set_t / cl_ddim_step_dev:
 * the DDIM loop body with a device cursor i (iteration number): index = S-1-i, ts[:] = ddim_timesteps[index]
 * (cldm/ddim_hacked.py:157-160,203-231); x_prev may alias x. */
int cl_tick(int* counter, void* stream);
int cl_adamw_dev(float* p, const float* g, float* m, float* v, long n, const float* hyper, int* step, void* stream);
/* Global gradient norm and clip coefficient on the device, added in ABI 7 (compatible): torch.nn.utils.clip_grad_norm_ (L2,
 * error_if_nonfinite=False) over nbuf (1 .. 16) flat fp32 buffers, with no host round trip, so that it replays inside a hipGraph.
 * bufs / counts are HOST arrays of nbuf device pointers / element counts (copied into the launch); hyper is cl_adamw_dev's table.
 *   out[0] = hyper[5] * sqrt(sum over all buffers of g^2)     -- grad_scale: the norm of the gradient AdamW applies
 *   out[1] = coef:  1.0f exactly when max_norm is NULL or *max_norm <= 0 (tracking only); otherwise, in fp32,
 *            c = *max_norm / (out[0] + 1e-6f),  coef = c < 1 ? c : (c != c ? c : 1.0f)   -- torch.clamp(c, max=1.0), NaN kept
 * Two launches: workgroups stride over the buffers (16-byte loads from each buffer's first 16-byte boundary, scalar head and
 * tail) and leave one fp64 partial each in scratch; one finishing workgroup adds them in index order.  Squares and sums are fp64
 * from the first product on.  No atomics, no waiting: the same bits on every launch and replay.  A non-finite element gives a
 * non-finite norm (NaN -> coef NaN, +-inf -> coef 0), as torch propagates it.  scratch: cl_grad_norm_scratch_floats(nbuf) floats,
 * 8-byte aligned (0 for an nbuf outside 1 .. 16).
 * Refused, before anything is launched: nbuf outside 1 .. 16, a negative count, a null buffer with a positive count, a buffer not
 * 4-byte aligned, a null bufs / counts / hyper / out / scratch, scratch not 8-byte aligned.  A count of 0 is fine (the norm of
 * nothing is 0).
 * cl_adamw_dev_clip: cl_adamw_dev with gi = g[i] * (hyper[5] * clip[1]), clip = the out of cl_grad_norm; the two scalars are
 * multiplied first, so clip[1] == 1.0f gives cl_adamw_dev's bits.  Refusals as cl_adamw_dev, and a null clip. */
long cl_grad_norm_scratch_floats(int nbuf);
int cl_grad_norm(const float* const* bufs, const long* counts, int nbuf, const float* hyper, const float* max_norm, float* out,
                 float* scratch, void* stream);
int cl_adamw_dev_clip(float* p, const float* g, float* m, float* v, long n, const float* hyper, int* step, const float* clip,
                      void* stream);
/* Parameter groups and a learning-rate schedule for cl_adamw_dev, on the device, added in ABI 7 (compatible).  Not in the
 * reference's fine-tuning path (one group, constant lr); torch.optim.AdamW's param_groups and LambdaLR's indexing.
 * cl_adamw_dev_groups: one AdamW launch over a flat fp32 buffer of n elements whose 64-float chunks belong to ngroups (1 .. 8)
 * parameter groups.
 *   hyper_table  fp32 [ngroups][6]: cl_adamw_dev's {lr, beta1, beta2, eps, weight_decay, grad_scale}, one row per group
 *   chunk_group  uint8 [n / 64]: the group of elements [64 c, 64 c + 64).  An entry >= ngroups is clamped to ngroups - 1 in the
 *                kernel, so nothing is read beyond the table; a caller should not rely on it.
 *   step         the shared device counter, advanced with cl_tick before the launch; the bias corrections are per group
 *   clip         NULL, or the out of cl_grad_norm: gi = g[i] * (hyper[5] * clip[1]) with the group's own hyper[5], the two
 *                scalars multiplied first, as cl_adamw_dev_clip does
 * Every element gets the expression of cl_adamw_dev (cl_adamw_dev_clip with clip) with its group's row: the same bits as that
 * launch over the chunk's span with that row as hyper.  g, the table and the map are only read.  A wave reads and writes whole
 * 256-byte chunks and looks the group up once per chunk: 28 + 1 / 64 bytes per element.
 * Refused, before anything is launched: a null p / g / m / v / hyper_table / chunk_group / step, n <= 0, n not a multiple of
 * 64, ngroups outside 1 .. 8.
 * cl_lr_schedule: hyper_table[gidx][0] = lr_table[min(*step - 1, T - 1)][gidx] for every group, one small launch.  lr_table is
 * fp32 [T][ngroups]; *step is the counter AFTER cl_tick, so optimizer step s (from 1) takes row s - 1 -- LambdaLR's indexing, the
 * lambda at 0 feeds the first step -- and the last row holds past the end (a counter below 1 takes row 0).  Columns 1 .. 5 of
 * the table are not touched.  Launch it after cl_tick and before the step's first AdamW launch.
 * Refused, before anything is launched: a null hyper_table / lr_table / step, T < 1, ngroups outside 1 .. 8. */
int cl_adamw_dev_groups(float* p, const float* g, float* m, float* v, long n, const float* hyper_table, int ngroups,
                        const unsigned char* chunk_group, int* step, const float* clip, void* stream);
int cl_lr_schedule(float* hyper_table, int ngroups, const float* lr_table, int T, const int* step, void* stream);
/* Exponential moving average of trained weights on the device, added in ABI 7 (compatible): LitEma.forward
 * (ldm/modules/ema.py) for one flat fp32 buffer, with no host round trip, so that it replays inside a hipGraph.
 *   u = *num_updates (already advanced by cl_tick, like cl_adamw_dev's step)
 *   d = u >= 0 ? min(*decay, (float)(1 + u) / (float)(10 + u)) : *decay       -- u < 0: LitEma without the warm-up
 *   omd = 1.0f - d;   shadow[i] = shadow[i] - omd * (shadow[i] - p[i])
 * all in fp32, every operation rounded once, nothing contracted: the bits of torch's s.sub_(omd * (s - p)) on the CPU.  min is
 * Python's: the warm-up term is taken only where it is smaller, a NaN decay stays.  p is only read; NaN / inf propagate; the zero
 * padding between the tensors of a flat buffer stays zero.  Any n; pointers need 4-byte alignment only, and shadow and p may
 * sit at different distances from a 16-byte boundary (at equal distances the launch uses 16-byte accesses).
 * Refused, before anything is launched: n < 0, a null decay / num_updates, a null shadow / p with n > 0, a pointer that is not
 * 4-byte aligned, shadow and p overlapping.  n == 0 is CL_OK.
 * cl_swap exchanges two fp32 buffers in place (the EMA scope: shadow into the masters and back, no third copy, no address
 * moves).  a == b is CL_OK and changes nothing; overlapping but different a and b are refused, and so are n < 0, a null a / b
 * with n > 0 and a pointer that is not 4-byte aligned. */
int cl_ema_update(float* shadow, const float* p, long n, const float* decay, const int* num_updates, void* stream);
int cl_swap(float* a, float* b, long n, void* stream);
int cl_ddim_set_t(const long* table, const int* cursor, int S, long* ts, int n, void* stream);
int cl_ddim_step_dev(const float* x, const float* e_c, const float* e_u, const float* noise, const float* coef,
                     const int* cursor, int S, float scale, float* x_prev, float* pred_x0, long n, void* stream);

/* ---- DPM-Solver++ (multistep, data prediction), added in ABI 7 (compatible) ----------------
 * One sampler step after the model evaluation, as one launch.  coef = device [S][8] fp32 table, row i =
 * {alpha_i, sigma_i, cx_i, c0_i, c1_i, c2_i, t_in_i, 0}; hist = device [3][n] fp32 ring of x0 predictions, model value k in
 * slot k % 3.  Step i:
 *   e = e_u ? e_u + scale (e_c - e_u) : e_c          m = (x - sigma_i e) / alpha_i          hist[i % 3] = m
 *   x_next = cx_i x + c0_i m + c1_i hist[(i + 2) % 3] + c2_i hist[(i + 1) % 3]
 * A term whose coefficient is exactly 0 is not read (those slots are uninitialised in the first steps).  x_next may alias x;
 * pred_x0 may be NULL and receives m.  cl_dpmpp_step takes the row from the host and returns 1 for S < 1 or an index outside
 * [0, S); cl_dpmpp_step_dev takes it from a device cursor (clamped to [0, S - 1]) so that the step replays as a hipGraph; both
 * run the same device code and give the same bits.  cl_dpm_set_t: ts[0 .. n) = coef[min(cursor, S - 1)][6], the model's
 * (float) input time of the step the cursor points at.  The caller advances the cursor with cl_tick. */
int cl_dpmpp_step(const float* x, const float* e_c, const float* e_u, const float* coef, int index, int S, float scale,
                  float* hist, float* x_next, float* pred_x0, long n, void* stream);
int cl_dpmpp_step_dev(const float* x, const float* e_c, const float* e_u, const float* coef, const int* cursor, int S,
                      float scale, float* hist, float* x_next, float* pred_x0, long n, void* stream);
int cl_dpm_set_t(const float* coef, const int* cursor, int S, float* ts, int n, void* stream);

/* ---- PLMS (pseudo linear multistep, Liu et al., arXiv:2202.09778), added in ABI 7 (compatible) ----
 * One sampler update after a model evaluation, as one launch.  coef = DDIM's device [S][4] fp32 table
 * {a_t, a_prev, sigma_t, sqrt(1-a_t)}; iteration `iter` (0 .. S-1) uses row S-1-iter.  hist = device [4][n] fp32 ring: the
 * guided eps of iteration k lives in slot k % 4.  e = e_u ? e_u + scale (e_c - e_u) : e_c, and upd(x, e') is
 *   pred_x0 = (x - sqrt(1-a_t) e') / sqrt(a_t)        x_prev = sqrt(a_prev) pred_x0 + sqrt(1 - a_prev - sigma_t^2) e'
 * phase 0, multistep (iter >= 1): hist[iter % 4] = e; with o_j = hist[(iter - j) % 4],
 *     e' = (3 e - o1) / 2  |  (23 e - 16 o1 + 5 o2) / 12  |  (55 e - 59 o1 + 37 o2 - 9 o3) / 24   for iter = 1 | 2 | >= 3;
 *     x_out, pred_x0 = upd(x, e').  A slot that is not part of the order is not read.
 * phase 1, start (iter == 0): hist[0] = e; x_out = upd(x, e).x_prev, the predictor; pred_x0 is not written.  x_out must not be
 *     x (phase 2 needs the iteration's input): pointer equality is refused.
 * phase 2, finish the start (iter == 0): e_c / e_u are the evaluation at (predictor, t_next) and x is the iteration's ORIGINAL
 *     input; e' = (hist[0] + e) / 2; hist is not written; x_out, pred_x0 = upd(x, e').
 * x_out may alias x in phases 0 and 2; pred_x0 may be NULL.  cl_plms_step_dev is phase 0 with iter = clamp(*cursor, 1, S-1), so
 * that the step replays as a hipGraph (time: cl_ddim_set_t, cursor: cl_tick); both run the same device code and give the same
 * bits.  Refused (1), before anything is launched: S < 1 (S < 2 for _dev), iter outside [0, S), phase outside 0..2, phase 1 or 2
 * with iter != 0, phase 0 with iter == 0, a null x / e_c / coef / hist / x_out / cursor, n < 0.  n == 0 is CL_OK. */
int cl_plms_step(const float* x, const float* e_c, const float* e_u, const float* coef, int iter, int S, int phase,
                 float scale, float* hist, float* x_out, float* pred_x0, long n, void* stream);
int cl_plms_step_dev(const float* x, const float* e_c, const float* e_u, const float* coef, const int* cursor, int S,
                     float scale, float* hist, float* x_out, float* pred_x0, long n, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CTRLORA_HIP_H */
