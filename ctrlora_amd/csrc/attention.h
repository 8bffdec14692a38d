// Argument blocks of the fused attention kernels (attention_fwd.hip / attention_bwd.hip).
#pragma once
#include "common.h"

namespace cl {

// Layouts (T = bf16 or float), heads h in [0,H), head dim DH, inner = H*DH:
//   Q  : [B*N,   ldq]  row b*N+n,   head h at columns [h*DH, (h+1)*DH)
//   K  : [B*Nkv, ldk]
//   V  : [B*Nkv, ldv]                       (backward only)
//   Vt : [B][inner][nkv_pad]  transposed V, zero padded to a multiple of 64 keys (forward)
//   O  : [B*N,   ldo]
//   LSE: [B][H][lse_stride] fp32, log2-domain log-sum-exp of scale*log2(e)*q.k (saved for
//        backward); lse_stride = a multiple of 64, >= N (N rounded up, or more): forward and backward refuse anything else
struct AttnFwdArgs {
  const void* Q; long ldq;
  const void* K; long ldk;
  const void* Vt; int nkv_pad;
  void* O; long ldo;
  float* LSE; int lse_stride;
  int B, H, N, Nkv, DH;
  float scale;   // d_head^-0.5 (ldm/modules/attention.py:151)
  // 1: Q holds q * scale * log2(e) (the producing projection applied the factor in ITS fp32 epilogue: one rounding, like any
  // stored q) -- the kernels then take scores straight from the matrix product (log2 domain).  bf16 kernels only.
  int q_prescaled;
};

// Decoupled image-prompt attention (cl_attention_fwd_ip): O gains ip_scale * softmax(scale q K2^T) V2 over Nip <= 64 keys
// of a second, per-sample context -- a softmax of its own, one masked 64-key tile.  K2 [B*Nip, ldk2]; V2 like V of the
// same kernel family: bf16 [B*Nip, ldv2] row-major, fp32 [B][inner][ldv2] transposed and zero padded (ldv2 % 64 == 0).
// A separate kernel argument, so that the plain forwards keep their argument layout.
struct AttnIpArgs {
  const void* K2; long ldk2;
  const void* V2; long ldv2;
  int Nip;
  float ip_scale;
};

struct AttnBwdArgs {
  const void* Q; long ldq; const void* K; long ldk; const void* V; long ldv;
  const void* O; long ldo; const void* dO; long lddo;
  const void* Qt; const void* dOt; int n_pad;     // [B][inner][n_pad]   transposes over queries
  const void* Kt; int nkv_pad;                    // [B][inner][nkv_pad] transpose over keys
  const float* LSE; float* Delta; int lse_stride; // [B][H][lse_stride]
  void* dQ; long lddq; void* dK; long lddk; void* dV; long lddv;  // dK/dV may be null (frozen context)
  int B, H, N, Nkv, DH;
  float scale;
  int q_prescaled;   // as in AttnFwdArgs; dQ / dK / dV are the gradients of the TRUE q, k, v either way
  // Optional scratch of B * H * lse_stride * 32 bytes (16-byte aligned): with a pre-scaled Q and d_head 40 the dQ kernel
  // leaves (-lse, -delta) of every query row there, split into three bf16 pieces each, and the dK/dV kernel stages them as
  // the pad columns of its Q / dO tiles: the matrix products then deliver s - lse and dP - delta (see attention_tr.hip).
  void* row_ws;
};

int attn_fwd(const AttnFwdArgs& a, int dtype, hipStream_t st);
int attn_bwd(const AttnBwdArgs& a, int dtype, hipStream_t st);
// bf16, no materialised transposes (attention_tr.hip): Vt / Qt / dOt / Kt of the argument blocks are ignored
int attn_fwd_tr(const AttnFwdArgs& a, const void* V, long ldv, hipStream_t st);
// the same two forwards with the image-prompt tile (AttnFwdArgs::K2 / V2); no LSE
int attn_fwd_ip(const AttnFwdArgs& a, const AttnIpArgs& ip, int dtype, hipStream_t st);
int attn_fwd_tr_ip(const AttnFwdArgs& a, const void* V, long ldv, const AttnIpArgs& ip, hipStream_t st);
int attn_bwd_tr(const AttnBwdArgs& a, hipStream_t st);
extern int g_attn_fuse_delta;   // 1 = the dQ kernel forms delta (default), 0 = separate attn_delta launch
extern int g_attn_variant_dkv4;
extern int g_attn_variant;   // probe hook: 0 = heuristic, 1 = tile-synchronous kernels only (no ping-pong schedule)
// pre-scaled-Q forward for d_head 40 (attention_fwd40.hip)
bool attn_fwd40_applies(const AttnFwdArgs& a);
int attn_fwd40(const AttnFwdArgs& a, const void* V, long ldv, hipStream_t st);
int attn_delta(const AttnBwdArgs& a, hipStream_t st);   // delta[q] = sum_d dO[q,d] O[q,d]  (bf16)
// causal self-attention forward, d_head 64, N <= 128 (attention_causal.hip): Q / K / V / O row-major [B*N, ld], no LSE
int attn_causal_fwd(int dtype, const void* Q, long ldq, const void* K, long ldk, const void* V, long ldv, void* O, long ldo, int B, int H,
                    int N, int dh, float scale, hipStream_t st);

// Read-only record of what the last attention entry point launched (csrc/debug_hooks.h: cl_debug_attention_last_launch).
// Host side only: every launcher of the attention files fills it next to its hipLaunchKernelGGL; an entry point that
// refuses its arguments leaves kind = 0.  No kernel, launch or argument depends on it.
enum { ATTN_FAM_TR = 1, ATTN_FAM_TR_IP = 2, ATTN_FAM_HYB = 3, ATTN_FAM_FWD40 = 4, ATTN_FAM_FOLD = 5, ATTN_FAM_TRANSPOSED = 6,
       ATTN_FAM_CAUSAL = 7 };
enum { ATTN_BIT_TAIL = 1, ATTN_BIT_TQ = 2, ATTN_BIT_TK = 4, ATTN_BIT_PRIO = 8 };
struct AttnLaunchRec {
  int kind;          // 0 nothing launched, 1 forward, 2 backward
  int family;        // ATTN_FAM_*
  int dtype, dh;
  int fwd_frags, dq_frags, dkv_frags;   // 64-row fragments per workgroup pass (0 = that kernel did not run)
  int bits;          // ATTN_BIT_*: the TAIL / TQ / TK template forms, s_setprio form
  int lookahead, remap;                 // hybrid / fwd40 forward
  int delta_launch, dkv_ran;            // backward: separate delta kernel, dK/dV kernel
  int grid_fwd, grid_dq, grid_dkv;      // workgroups
  int tile;          // keys / queries per staged tile along the looped dimension
};
extern AttnLaunchRec g_attn_last;
inline void attn_rec_begin() { g_attn_last = AttnLaunchRec{}; }
inline void attn_rec(int kind, int family, int dtype, int dh) {
  g_attn_last.kind = kind; g_attn_last.family = family; g_attn_last.dtype = dtype; g_attn_last.dh = dh; g_attn_last.tile = 64;
}

}  // namespace cl
