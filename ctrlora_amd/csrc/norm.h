// Argument blocks of the normalisation kernels (norm.hip).
#pragma once
#include "common.h"

namespace cl {

extern int g_gn_three_pass;   // A/B hook: 1 = partial -> finalize -> apply for every GroupNorm
extern int g_gn_one_pass;     // A/B hook: 0 = never the one-launch register-resident forms
extern int g_gn_group;        // one workgroup per (sample, group): 0 never, 1 by rule (default), 2 whenever the slab fits; + 4 = naive id mapping

struct GnArgs {
  const void* x; long ldx;      // [B*HW, C] token-major (NHWC), row stride ldx
  void* y; long ldy;
  const float* gamma; const float* beta;
  int B, HW, C, G; float eps; int silu;
  float* stats;                 // out [B][G][2] = mean, rstd (kept for backward)
  float* ws;                    // gn_ws_floats(B,HW,C) floats of scratch
};

struct GnBwdArgs {
  const void* x; long ldx; const void* dy; long lddy;
  const void* accum; long ldacc;  // optional: dx = accum + grad (gradient fan-in fused)
  void* dx; long lddx;
  const float* gamma; const float* beta; const float* stats;
  int B, HW, C, G; int silu;
  float* dgamma; float* dbeta;    // optional fp32 accumulators (trainable norms only)
  float* ws;
};

struct LnArgs {
  const void* x; long ldx; void* y; long ldy;
  const float* gamma; const float* beta; int M, D; float eps;
  float* stats;                 // out [M][2] = mean, rstd (may be null at inference)
};

struct LnBwdArgs {
  const void* x; long ldx; const void* dy; long lddy;
  const void* accum; long ldacc; void* dx; long lddx;
  const float* gamma; const float* stats; int M, D;
  float* dgamma; float* dbeta;
};

// Read-only record of what the last normalisation entry point launched (csrc/debug_hooks.h: cl_debug_norm_last_launch).
// Host side only: every launcher of norm.hip fills it once CL_CHECK_LAUNCH has passed (norm_coop.hip only names its form); an
// entry point that refuses its arguments, or whose launch fails (CL_ELAUNCH), leaves kind = 0.  No kernel, launch or argument
// depends on it.
enum { NORM_GN_FWD = 1, NORM_GN_BWD = 2, NORM_LN_FWD = 3, NORM_LN_BWD = 4 };
enum { NORM_FORM_ONE = 1, NORM_FORM_TWO = 2, NORM_FORM_THREE = 3, NORM_FORM_COOP = 4, NORM_FORM_GROUP = 5 };
struct NormLaunchRec {
  int kind;          // 0 nothing launched (refused), NORM_GN_* / NORM_LN_*
  int form;          // NORM_FORM_*: launches of the call (LayerNorm backward: 2 = kernel + ln_bwd_finish_kernel)
  int dtype;
  int nv;            // 16-byte vectors per lane held in registers (gn1_* / ln_*; 0 for the chunked GroupNorm forms); gng_*: vectors of
                     // gcd(16, C / G * 2) bytes per lane and operand
  int lpr_rpi;       // gn1_*: lanes per pixel row; gng_*: vectors per pixel row; chunked GroupNorm: PY; LayerNorm: rows per wave iteration
  int threads;       // gn1_*: waves per workgroup; every other form: threads per workgroup
  int cb_vx;         // gn1_*: channels per block CB; gng_*: channels per workgroup C / G; chunked GroupNorm: VX; LayerNorm: D / 8
  int chunks;        // pixel chunks per sample (chunked GroupNorm forms)
  int grid_x, grid_y;
  int colsum;        // dgamma / dbeta of the LayerNorm backward: 0 none, 1 workspace + finish, 2 atomics
  int passes;        // channel passes per lane (C / 8 / VX; 1 everywhere else)
};
extern NormLaunchRec g_norm_last;
inline void norm_rec_begin() { g_norm_last = NormLaunchRec{}; }

long gn_ws_floats(int B, int HW, int C);
// one-launch, one-pass cooperative form (norm_coop.hip); CL_EINVAL = not its case
extern int g_gn_coop;
int gnc_fwd(const GnArgs& a, int dtype, hipStream_t st);
int gnc_bwd(const GnBwdArgs& a, int dtype, hipStream_t st);
unsigned gnc_timeouts();
int gn_fwd(const GnArgs& a, int dtype, hipStream_t st);
int gn_bwd(const GnBwdArgs& a, int dtype, hipStream_t st);
int ln_fwd(const LnArgs& a, int dtype, hipStream_t st);
int ln_bwd(const LnBwdArgs& a, int dtype, hipStream_t st);

}  // namespace cl
