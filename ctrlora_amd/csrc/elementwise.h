// Host launchers of the elementwise / layout kernels (elementwise.hip).
#pragma once
#include "common.h"

namespace cl {

// Read-only record of what the last elementwise / layout entry point launched (csrc/debug_hooks.h: cl_debug_ew_last_launch).
// Every launcher resets it on entry and ew_done() (elementwise.hip) writes it after the launch check, so a refused or failed
// call leaves id = 0.  form / aux: colsum 1 = block partials + finishing kernel, 2 = atomics, aux = pixel chunks; zero: bit 0 =
// head bytes, bit 1 = tail bytes, aux = 16-byte vectors; vit_patch_rows: 1 = float2 (PAIR) loads; mse_loss: aux = workgroups;
// transpose: form = the input's dtype; plms_step: form = phase; posterior_sample_pair: form 1 = 16-byte loads and stores, 0 = scalar, aux = tensors (1 or 2);
// qsample_blend: form as posterior_sample_pair, aux bit 0 = mask per sample, bit 1 = mask per channel; grad_norm: the partial
// launch's grid, aux = buffers; plosses: form 0 = cl_p_losses_mse, 4 | kind << 1 | (table given) = cl_p_losses_w; ema_update / swap: form 1 = 16-byte accesses with scalar head and tail (aux = vectors), 0 = scalar;
// adamw_dev_groups: form 1 = with a clip coefficient, aux = groups; lr_schedule: aux = groups; loss_bands: form 1 = with n_valid,
// aux = bands.
enum {
  EW_GEGLU_FWD = 1, EW_GEGLU_BWD, EW_SILU_FWD, EW_SILU_BWD, EW_AXPBY, EW_TRANSPOSE, EW_NCHW_TO_TOK, EW_TOK_TO_NCHW,
  EW_TIMESTEP, EW_TIMESTEP_F, EW_QSAMPLE, EW_MSE, EW_PLOSSES, EW_ZERO, EW_CONV_TAP, EW_SOFTMAX, EW_DDIM_STEP, EW_TICK,
  EW_ADAMW_DEV, EW_DDIM_SET_T, EW_DDIM_STEP_DEV, EW_DPMPP_STEP, EW_DPMPP_STEP_DEV, EW_DPM_SET_T, EW_ADAMW, EW_POOL2X2,
  EW_COLSUM, EW_REPACK, EW_PACK2D, EW_VIT_PATCH_ROWS, EW_VIT_TOKENS,
  EW_CLIP_TEXT_EMBED, EW_GATHER_ROWS, EW_POSTERIOR_PAIR, EW_PLMS_STEP, EW_PLMS_STEP_DEV,
  EW_QSAMPLE_BLEND, EW_GRAD_NORM, EW_ADAMW_DEV_CLIP, EW_EMA_UPDATE, EW_SWAP,
  EW_ADAMW_DEV_GROUPS, EW_LR_SCHEDULE
};
static_assert(EW_SWAP == 41 && EW_LR_SCHEDULE == 43, "the ids are read by number through cl_debug_ew_last_launch: append only");
// the enumeration is closed at 43 (the tests of the step pin its last member): later records continue the numbering as constants
constexpr int EW_LOSS_BANDS = 44;
struct EwLaunchRec {
  int id;        // EW_* of the entry point, 0 = nothing launched
  int dtype;     // CL_BF16 / CL_F32 of the typed launchers (transpose: the output's), -1 where there is no dtype argument
  int gx, gy, gz, threads;   // grid and workgroup size of the (main) kernel
  int form, aux;
};
extern EwLaunchRec g_ew_last;
inline void ew_rec_begin() { g_ew_last = EwLaunchRec{}; }

int geglu_fwd(int dtype, const void* h, long ldh, void* out, long ldo, long M, int F, hipStream_t st);
int geglu_bwd(int dtype, const void* h, long ldh, const void* dout, long lddo, void* dh, long lddh, long M, int F, hipStream_t st);
int silu_fwd(int dtype, const void* x, void* y, long n, hipStream_t st);
int silu_bwd(int dtype, const void* x, const void* dy, void* dx, long n, hipStream_t st);
int axpby(int dtype, const void* x, long ldx, void* y, long ldy, long M, int C, float a, float b, hipStream_t st);
int transpose(int in_dtype, int out_dtype, const void* in, long ldi, long bsi, void* out, long ldo, long bso,
              int Bt, int R, int C, int Rpad, hipStream_t st);
int nchw_to_tok(int dtype, const float* in, void* out, long ldo, int B, int Cin, int Cpad, int HW, hipStream_t st);
int tok_to_nchw(int dtype, const void* in, long ldi, float* out, int B, int C, int HW, float alpha, float beta, hipStream_t st);
int timestep_embed(int dtype, const long* t, const float* freqs, void* out, long ldo, int B, int half, hipStream_t st);
int timestep_embed_f(int dtype, const float* t, const float* freqs, void* out, long ldo, int B, int half, hipStream_t st);
int qsample(const float* z, const float* noise, const long* t, const float* sqrt_ac, const float* sqrt_1mac,
            float* out, int B, long per, hipStream_t st);
// q_sample(x0, t) * mask + (1 - mask) * x of a masked sampling step in one launch; out may be x (elementwise.hip)
int qsample_blend(const float* x0, const float* noise, const long* t, const float* sqrt_ac, const float* sqrt_1mac, int T,
                  const float* mask, int mask_per_batch, int mask_per_channel, const float* x, float* out, int B, int C, long HW,
                  hipStream_t st);
// scale * (mean + std * e) of one or two cached posteriors in one launch (LatentDiffusion.get_first_stage_encoding)
int posterior_sample_pair(const float* mom_a, const float* e_a, float* out_a, const float* mom_b, const float* e_b, float* out_b,
                          int B, long per, float scale, hipStream_t st);
int mse_loss(const float* eps, const float* target, float* d_eps, float* loss, long n, float gscale, hipStream_t st);
int plosses_mse(const float* eps, const float* target, float* d_eps, const long* t, const float* lvlb, float* out,
                float* per_sample, float* scratch, int B, long per, float gscale, float w_simple, float w_elbo,
                hipStream_t st);
// the same reduction with a per-timestep weight table (wt, optional) and rho = l2 (kind 0) or Huber (kind 1, delta);
// EwLaunchRec: id = EW_PLOSSES, form = 4 | kind << 1 | (wt given)  (elementwise.hip)
int plosses_w(const float* eps, const float* target, float* d_eps, const long* t, const float* lvlb, const float* wt, float* out,
              float* per_sample, float* scratch, int B, long per, int kind, float delta, float gscale, float w_simple,
              float w_elbo, hipStream_t st);
// {count, sum, sum of squares} of the per-sample losses by timestep band, added to a device double [nbands + 1][3] in index
// order by one workgroup (elementwise.hip)
int loss_bands(const float* per_sample, const long* t, int B, int T, int nbands, const int* n_valid, double* acc,
               hipStream_t st);
int zero_bytes(void* p, long nbytes, hipStream_t st);
int conv_tap_gather(int dtype, const void* x, long ldx, void* out, long ldo, int B, int Hin, int Win, int Hout, int Wout,
                    int C, int tap, int stride, int pad, hipStream_t st);
int softmax_rows(int dtype, const float* S, long lds_, void* P, long ldp, long M, int N, float scale, hipStream_t st);
int ddim_step(const float* x, const float* e_c, const float* e_u, const float* noise, const float* coef, int index,
              float scale, float* x_prev, float* pred_x0, long n, hipStream_t st);
int tick(int* counter, hipStream_t st);
int adamw_dev(float* p, const float* g, float* m, float* v, long n, const float* hyper, int* step, hipStream_t st);
// global L2 norm of up to 16 flat fp32 buffers times hyper[5], and torch's clip coefficient, to out[0..1]; AdamW on the
// clipped gradient (elementwise.hip)
long grad_norm_scratch_floats(int nbuf);
int grad_norm(const float* const* bufs, const long* counts, int nbuf, const float* hyper, const float* max_norm, float* out,
              float* scratch, hipStream_t st);
int adamw_dev_clip(float* p, const float* g, float* m, float* v, long n, const float* hyper, int* step, const float* clip,
                   hipStream_t st);
// AdamW over one flat buffer whose 64-float chunks belong to 1 .. 8 parameter groups (hyper_table [ngroups][6], chunk_group
// [n / 64]; clip may be NULL); the groups' learning rates of this step from a device [T][ngroups] table (elementwise.hip)
int adamw_dev_groups(float* p, const float* g, float* m, float* v, long n, const float* hyper_table, int ngroups,
                     const unsigned char* chunk_group, int* step, const float* clip, hipStream_t st);
int lr_schedule(float* hyper_table, int ngroups, const float* lr_table, int T, const int* step, hipStream_t st);
// LitEma.forward over one flat fp32 buffer with device-resident decay and update count; exchange of two flat fp32 buffers
// (elementwise.hip)
int ema_update(float* shadow, const float* p, long n, const float* decay, const int* num_updates, hipStream_t st);
int swap_buffers(float* a, float* b, long n, hipStream_t st);
int ddim_set_t(const long* table, const int* cursor, int S, long* ts, int n, hipStream_t st);
int ddim_step_dev(const float* x, const float* e_c, const float* e_u, const float* noise, const float* coef,
                  const int* cursor, int S, float scale, float* x_prev, float* pred_x0, long n, hipStream_t st);
// DPM-Solver++ multistep update over a [S][8] coefficient table and a [3][n] ring of x0 predictions (elementwise.hip)
int dpmpp_step(const float* x, const float* e_c, const float* e_u, const float* coef, int index, int S, float scale,
               float* hist, float* x_next, float* pred_x0, long n, hipStream_t st);
int dpmpp_step_dev(const float* x, const float* e_c, const float* e_u, const float* coef, const int* cursor, int S,
                   float scale, float* hist, float* x_next, float* pred_x0, long n, hipStream_t st);
int dpm_set_t(const float* coef, const int* cursor, int S, float* ts, int n, hipStream_t st);
// PLMS update over DDIM's [S][4] table and a [4][n] ring of guided eps; phase 0 multistep, 1 start, 2 finish the start
// (elementwise.hip; EwLaunchRec.form = phase)
int plms_step(const float* x, const float* e_c, const float* e_u, const float* coef, int iter, int S, int phase, float scale,
              float* hist, float* x_out, float* pred_x0, long n, hipStream_t st);
int plms_step_dev(const float* x, const float* e_c, const float* e_u, const float* coef, const int* cursor, int S,
                  float scale, float* hist, float* x_out, float* pred_x0, long n, hipStream_t st);
int adamw(float* p, const float* g, float* m, float* v, long n, float lr, float beta1, float beta2, float eps,
          float wd, int step, float gscale, hipStream_t st);
int pool2x2(int dtype, const void* in, long ldi, void* out, long ldo, int B, int H, int W, int C, int accumulate, hipStream_t st);
int colsum(int dtype, const void* in, long ldi, float* out, long ldo, int B, int HW, int C, float scale, hipStream_t st);
int repack(int dtype, const float* flat, const long* desc, const int* tile_prefix, int ndesc, int total_tiles,
           hipStream_t st);
int pack2d(int dtype, const float* in, long ldi, void* out, long ldo, long R, int C, int Cpad, hipStream_t st);
// CLIPVisionEmbeddings: NCHW fp32 pixels -> zero-padded patch rows; class / patch rows + position embedding -> tokens
int vit_patch_rows(int dtype, const float* pixels, void* out, long ldo, int B, int C, int S, int P, int Kpad, hipStream_t st);
int vit_tokens(int dtype, const void* patch, long ldp, const float* cls, const float* pos, void* out, long ldo, int B, int T,
               int D, hipStream_t st);
// CLIPTextEmbeddings: token rows gathered by id (clamped to [0, vocab)) + position embedding; rows gathered by index (clamped)
int clip_text_embed(int dtype, const long* ids, const float* tok, const float* pos, void* out, long ldo, int B, int T, int D, int vocab,
                    hipStream_t st);
int gather_rows(int dtype, const void* src, long lds_, const long* rows, void* dst, long ldd, int R, int D, int nsrc, hipStream_t st);

}  // namespace cl
