// GroupNorm(32)+SiLU and LayerNorm, forward and backward, for NHWC / token-major
// activations on gfx950.  HBM-bound kernels: 16-byte vector loads, fp32
// statistics (GroupNorm32 computes in fp32, ldm/modules/diffusionmodules/util.py:217-219),
// wave64 shuffle reductions, SiLU fused into the normalisation pass.
//
//   GroupNorm fwd : gn_partial (per-channel sum / sumsq per pixel chunk)
//                   -> gn_finalize (per-(b,group) mean/rstd, per-(b,channel) scale/shift)
//                   -> gn_apply   (y = silu?(x*scale + shift))
//   GroupNorm bwd : gn_bwd_partial -> gn_bwd_finalize (+ dgamma/dbeta) -> gn_bwd_apply
//   one launch    : gn1_* (sample, channel block) and gng_* (sample, group) keep their slab in registers
//   LayerNorm     : one wave per row, row kept in registers (D <= 2048)
//
// Reference ops replaced: ResBlock in_layers[0:2]/out_layers[0:2]
// (openaimodel.py:201-202,225-226; eps 1e-5), SpatialTransformer.norm
// (attention.py:88-89,295; eps 1e-6, no SiLU), BasicTransformerBlock.norm1-3
// (attention.py:263-265; eps 1e-5), UNetModel.out[0:2] (openaimodel.py:726-728).
#include <algorithm>
#include "norm.h"
#include "gemm.h"

namespace cl {

static constexpr int GN_MAX_THREADS = 512;

NormLaunchRec g_norm_last{};   // probe record (norm.h)

struct GnGeom { int VX, PY, threads, nchunk, ppc; };

static GnGeom gn_geom(int B, int HW, int C) {
  GnGeom g;
  const int C8 = C / 8;
  g.VX = C8 < 320 ? C8 : 320;
  if (g.VX > GN_MAX_THREADS) g.VX = GN_MAX_THREADS;
  g.PY = 256 / g.VX; if (g.PY < 1) g.PY = 1;
  g.threads = g.VX * g.PY;
  // enough blocks to fill 256 CUs a few times over, at least 4 pixels per py lane
  int want = (1024 + B - 1) / B;
  int maxc = HW / (g.PY * 4); if (maxc < 1) maxc = 1;
  g.nchunk = want < maxc ? want : maxc;
  if (g.nchunk > 256) g.nchunk = 256;
  g.ppc = (HW + g.nchunk - 1) / g.nchunk;
  g.nchunk = (HW + g.ppc - 1) / g.ppc;
  return g;
}

long gn_ws_floats(int B, int HW, int C) {
  GnGeom g = gn_geom(B, HW, C);
  return (long)B * g.nchunk * C * 2 + (long)B * C * 4;
}

// ------------------------------------------------------------------ forward

template <typename T>
__global__ void gn_partial_kernel(const T* __restrict__ x, long ldx, int HW, int C, int VX, int PY,
                                  int ppc, int nchunk, float* __restrict__ partial) {
  extern __shared__ float red[];  // [PY][VX][16]
  const int C8 = C / 8;
  const int vx = threadIdx.x % VX, py = threadIdx.x / VX;
  const int b = blockIdx.y, chunk = blockIdx.x;
  const int p0 = chunk * ppc, p1 = min(HW, p0 + ppc);
  for (int v = vx; v < C8; v += VX) {
    float s[8], q[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) { s[e] = 0.f; q[e] = 0.f; }
  #pragma unroll 4
  for (int p = p0 + py; p < p1; p += PY) {
      float f[8];
      load8(x + ((long)b * HW + p) * ldx + v * 8, f);
#pragma unroll
      for (int e = 0; e < 8; ++e) { s[e] += f[e]; q[e] += f[e] * f[e]; }
    }
    float* r = red + (py * VX + vx) * 16;
#pragma unroll
    for (int e = 0; e < 8; ++e) { r[e] = s[e]; r[8 + e] = q[e]; }
    __syncthreads();
    if (py == 0) {
      for (int k = 1; k < PY; ++k) {
        const float* o = red + (k * VX + vx) * 16;
#pragma unroll
        for (int e = 0; e < 8; ++e) { s[e] += o[e]; q[e] += o[8 + e]; }
      }
      float* dst = partial + (((long)b * nchunk + chunk) * C + v * 8) * 2;
#pragma unroll
      for (int e = 0; e < 8; ++e) { dst[2 * e] = s[e]; dst[2 * e + 1] = q[e]; }
    }
    __syncthreads();
  }
}

// block-wide sum of two doubles (256 threads = 4 waves); result valid in every thread
__device__ __forceinline__ void block_sum2(double& a, double& b, double* red /*[8]*/) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { a += __shfl_xor(a, o, 64); b += __shfl_xor(b, o, 64); }
  const int wave = threadIdx.x >> 6;
  __syncthreads();
  if ((threadIdx.x & 63) == 0) { red[wave] = a; red[4 + wave] = b; }
  __syncthreads();
  a = red[0] + red[1] + red[2] + red[3];
  b = red[4] + red[5] + red[6] + red[7];
}

// per-(b,group) mean/rstd and per-(b,channel) scale/shift
__global__ __launch_bounds__(256) void gn_finalize_kernel(const float* __restrict__ partial, int nchunk, int HW, int C,
                                                          int G, float eps, const float* __restrict__ gamma,
                                                          const float* __restrict__ beta,
                                                          float* __restrict__ stats /*[B][G][2]*/,
                                                          float* __restrict__ coef /*[B][C][2]*/) {
  // one workgroup per (sample, group): 256 threads sweep the group's (chunk, channel) partials, coalesced
  __shared__ double red[8];
  const int g = blockIdx.x, b = blockIdx.y, cg = C / G, tid = threadIdx.x;
  double s = 0, q = 0;
  const int total = nchunk * cg;
  for (int i = tid; i < total; i += 256) {
    const int k = i / cg, c = g * cg + (i - k * cg);
    const float2 p = *reinterpret_cast<const float2*>(partial + (((long)b * nchunk + k) * C + c) * 2);
    s += p.x; q += p.y;
  }
  block_sum2(s, q, red);
  const double n = (double)HW * cg;
  const double mean = s / n;
  double var = q / n - mean * mean;
  if (var < 0) var = 0;
  const double rstd = 1.0 / sqrt(var + (double)eps);
  if (tid == 0) {
    stats[((long)b * G + g) * 2] = (float)mean;
    stats[((long)b * G + g) * 2 + 1] = (float)rstd;
  }
  for (int c = g * cg + tid; c < (g + 1) * cg; c += 256) {
    const double sc = rstd * (double)gamma[c];
    coef[((long)b * C + c) * 2] = (float)sc;
    coef[((long)b * C + c) * 2 + 1] = (float)((double)beta[c] - mean * sc);
  }
}

template <typename T, bool SILU>
__global__ void gn_apply_kernel(const T* __restrict__ x, long ldx, T* __restrict__ y, long ldy, int HW, int C,
                                int VX, int PY, int ppc, const float* __restrict__ coef) {
  const int C8 = C / 8;
  const int vx = threadIdx.x % VX, py = threadIdx.x / VX;
  const int b = blockIdx.y, chunk = blockIdx.x;
  const int p0 = chunk * ppc, p1 = min(HW, p0 + ppc);
  for (int v = vx; v < C8; v += VX) {
    float sc[8], sh[8];
    const float* cf = coef + ((long)b * C + v * 8) * 2;
#pragma unroll
    for (int e = 0; e < 8; ++e) { sc[e] = cf[2 * e]; sh[e] = cf[2 * e + 1]; }
  #pragma unroll 4
  for (int p = p0 + py; p < p1; p += PY) {
      float f[8];
      const long row = (long)b * HW + p;
      load8(x + row * ldx + v * 8, f);
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        float z = f[e] * sc[e] + sh[e];
        f[e] = SILU ? silu_f(z) : z;
      }
      store8(y + row * ldy + v * 8, f);
    }
  }
}

// ---- two-launch forms (no finalize launch).  The statistics pass reduces its chunk to per-GROUP sums
// ([B][nchunk][G][2] floats); every workgroup of the apply pass then sums the nchunk partials of its sample itself
// (fp64, fixed order: deterministic) -- G * nchunk * 8 bytes from L2, a microsecond -- instead of a third launch whose
// ~6 us are almost all launch latency (149 such launches per training step).  Needs one channel pass per lane
// (C <= 2560) and G <= 64.

// LDS layout helper: channel totals [C][2] floats reuse the py-reduction scratch
template <typename T>
__global__ void gn_gpartial_kernel(const T* __restrict__ x, long ldx, int HW, int C, int G, int VX, int PY, int ppc,
                                   int nchunk, float* __restrict__ gpartial) {
  extern __shared__ float red[];  // max([PY][VX][16], [C][2]) floats
  const int vx = threadIdx.x % VX, py = threadIdx.x / VX;
  const int b = blockIdx.y, chunk = blockIdx.x;
  const int p0 = chunk * ppc, p1 = min(HW, p0 + ppc);
  float s[8], q[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) { s[e] = 0.f; q[e] = 0.f; }
#pragma unroll 4
  for (int p = p0 + py; p < p1; p += PY) {
    float f[8];
    load8(x + ((long)b * HW + p) * ldx + vx * 8, f);
#pragma unroll
    for (int e = 0; e < 8; ++e) { s[e] += f[e]; q[e] += f[e] * f[e]; }
  }
  float* r = red + (py * VX + vx) * 16;
#pragma unroll
  for (int e = 0; e < 8; ++e) { r[e] = s[e]; r[8 + e] = q[e]; }
  __syncthreads();
  if (py == 0) {
    for (int k = 1; k < PY; ++k) {
      const float* o = red + (k * VX + vx) * 16;
#pragma unroll
      for (int e = 0; e < 8; ++e) { s[e] += o[e]; q[e] += o[8 + e]; }
    }
  }
  __syncthreads();
  if (py == 0) {
    float* ch = red + vx * 16;
#pragma unroll
    for (int e = 0; e < 8; ++e) { ch[2 * e] = s[e]; ch[2 * e + 1] = q[e]; }
  }
  __syncthreads();
  if ((int)threadIdx.x < G) {
    const int cg = C / G, c0 = threadIdx.x * cg;
    float S = 0.f, Q = 0.f;
    for (int c = c0; c < c0 + cg; ++c) { S += red[2 * c]; Q += red[2 * c + 1]; }
    float* dst = gpartial + (((long)b * nchunk + chunk) * G + threadIdx.x) * 2;
    dst[0] = S; dst[1] = Q;
  }
}

// sum the nchunk group partials of sample b: every thread group (g = tid % G, lane kl = tid / G) takes chunks
// kl, kl + KL, ...; result per group in tot[g][0..1] (double), valid after the trailing barrier
__device__ __forceinline__ void gn_group_totals(const float* __restrict__ gpartial, int b, int nchunk, int G,
                                                double (*part)[64][2], double (*tot)[2]) {
  const int tid = threadIdx.x;
  int KL = blockDim.x / G; if (KL > 8) KL = 8;
  const int g = tid % G, kl = tid / G;
  if (kl < KL) {
    // four independent L2 loads in flight per lane: this walk (nchunk / KL ~ 18 partials) is the prologue of every apply
    // workgroup and, one load at a time, cost about as long as the workgroup's whole pixel loop
    double s = 0, q = 0;
    const float2* src = reinterpret_cast<const float2*>(gpartial) + (long)b * nchunk * G + g;
    int k = kl;
    for (; k + 3 * KL < nchunk; k += 4 * KL) {
      const float2 p0 = src[(long)k * G], p1 = src[(long)(k + KL) * G];
      const float2 p2 = src[(long)(k + 2 * KL) * G], p3 = src[(long)(k + 3 * KL) * G];
      s += ((double)p0.x + (double)p1.x) + ((double)p2.x + (double)p3.x);
      q += ((double)p0.y + (double)p1.y) + ((double)p2.y + (double)p3.y);
    }
    for (; k < nchunk; k += KL) {
      const float2 p = src[(long)k * G];
      s += p.x; q += p.y;
    }
    part[kl][g][0] = s; part[kl][g][1] = q;
  }
  __syncthreads();
  if (tid < G) {
    double s = 0, q = 0;
    for (int k = 0; k < KL; ++k) { s += part[k][tid][0]; q += part[k][tid][1]; }
    tot[tid][0] = s; tot[tid][1] = q;
  }
  __syncthreads();
}

template <typename T, bool SILU>
__global__ void gn_gapply_kernel(const T* __restrict__ x, long ldx, T* __restrict__ y, long ldy, int HW, int C, int G,
                                 int VX, int PY, int ppc, int nchunk, float eps, const float* __restrict__ gamma,
                                 const float* __restrict__ beta, const float* __restrict__ gpartial,
                                 float* __restrict__ stats /*[B][G][2]*/) {
  __shared__ double part[8][64][2];
  __shared__ double tot[64][2];
  const int b = blockIdx.y, chunk = blockIdx.x, cg = C / G;
  gn_group_totals(gpartial, b, nchunk, G, part, tot);
  if ((int)threadIdx.x < G) {
    const double n = (double)HW * cg;
    const double mean = tot[threadIdx.x][0] / n;
    double var = tot[threadIdx.x][1] / n - mean * mean;
    if (var < 0) var = 0;
    const double rstd = 1.0 / sqrt(var + (double)eps);
    tot[threadIdx.x][0] = mean; tot[threadIdx.x][1] = rstd;
    if (chunk == 0) {
      stats[((long)b * G + threadIdx.x) * 2] = (float)mean;
      stats[((long)b * G + threadIdx.x) * 2 + 1] = (float)rstd;
    }
  }
  __syncthreads();
  const int vx = threadIdx.x % VX, py = threadIdx.x / VX;
  const int p0 = chunk * ppc, p1 = min(HW, p0 + ppc);
  float sc[8], sh[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const int c = vx * 8 + e, gi = c / cg;
    const double scd = tot[gi][1] * (double)gamma[c];
    sc[e] = (float)scd;
    sh[e] = (float)((double)beta[c] - tot[gi][0] * scd);
  }
#pragma unroll 4
  for (int p = p0 + py; p < p1; p += PY) {
    float f[8];
    const long row = (long)b * HW + p;
    load8(x + row * ldx + vx * 8, f);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      float z = f[e] * sc[e] + sh[e];
      f[e] = SILU ? silu_f(z) : z;
    }
    store8(y + row * ldy + vx * 8, f);
  }
}

int g_gn_three_pass = 0;   // A/B hook: 1 = always the partial -> finalize -> apply form

// ------------------------------------------------------------------ one-launch GroupNorm (register-resident slab)
// At the 32x32 / 16x16 / 8x8 levels the two-launch form above is bound by launch and dependency latency, not bytes:
// both of its kernels last ~9 us whatever the tensor size (88 forward + 61 backward GroupNorms per training step).
// Here ONE workgroup owns (sample b, channel block of CB = lcm(C / G, 8) channels = whole groups, 16-byte aligned) and
// keeps the block's [HW][CB] slab in registers between the statistics and the apply: the tensor is read once and written
// once, in one launch (the forward stores mean / rstd for the backward as before).  Lanes are laid out LPR (8 or 16) per
// pixel row -- CB / 8 of them active -- so that the per-channel sums reduce over the pixels of a wave with shuffles and
// over the waves through a small LDS array.  Taken when the grid (B * C / CB workgroups of up to 1024 threads) is at
// least GN1_MIN_WG and the slab fits NV vectors per lane; everything else (the 64x64 level, whose groups span 4096
// pixels) stays on the two-launch form.  The backward handles trainable norms too (dgamma / dbeta: one float atomic per
// channel and sample, as the three-launch form did).
static constexpr int GN1_MIN_WG = 96;
int g_gn_one_pass = 1;        // A/B hook (cl_debug_groupnorm_form): 0 = never take the one-launch form

template <typename T> struct Pack8;
template <> struct Pack8<bf16_t> {
  uint4 v;
  __device__ __forceinline__ void load(const bf16_t* p) { v = *reinterpret_cast<const uint4*>(p); }
  __device__ __forceinline__ void get(float f[8]) const {
    f[0] = __uint_as_float(v.x << 16); f[1] = __uint_as_float(v.x & 0xffff0000u);
    f[2] = __uint_as_float(v.y << 16); f[3] = __uint_as_float(v.y & 0xffff0000u);
    f[4] = __uint_as_float(v.z << 16); f[5] = __uint_as_float(v.z & 0xffff0000u);
    f[6] = __uint_as_float(v.w << 16); f[7] = __uint_as_float(v.w & 0xffff0000u);
  }
};
template <> struct Pack8<float> {
  float4 a, b;
  __device__ __forceinline__ void load(const float* p) { a = reinterpret_cast<const float4*>(p)[0]; b = reinterpret_cast<const float4*>(p)[1]; }
  __device__ __forceinline__ void get(float f[8]) const {
    f[0] = a.x; f[1] = a.y; f[2] = a.z; f[3] = a.w; f[4] = b.x; f[5] = b.y; f[6] = b.z; f[7] = b.w;
  }
};

struct Gn1Geom { int CB, VX, LPR, NW, NV, nblk; bool ok; };

static void gn_rec1(int kind, int dtype, const Gn1Geom& g, int B) {
  g_norm_last = NormLaunchRec{kind, NORM_FORM_ONE, dtype, g.NV, g.LPR, g.NW, g.CB, 0, g.nblk, B, 0, 1};
}
static void gn_rec(int kind, int form, int dtype, const GnGeom& g, int B, int C) {
  g_norm_last = NormLaunchRec{kind, form, dtype, 0, g.PY, g.threads, g.VX, g.nchunk, g.nchunk, B, 0, (C / 8 + g.VX - 1) / g.VX};
}

static Gn1Geom gn1_geom(int B, int HW, int C, int G, int esize, bool bwd) {
  Gn1Geom g{}; g.ok = false;
  if (!g_gn_one_pass || g_gn_three_pass || C % G) return g;
  const int cg = C / G;
  int cb = cg;
  while (cb % 8) cb += cg;                 // lcm(cg, 8)
  if (cb > 128 || C % cb) return g;
  g.CB = cb; g.VX = cb / 8; g.LPR = g.VX <= 8 ? 8 : 16;
  const int ppw = 64 / g.LPR;
  // forward: up to 16 waves (128 VGPRs per lane); backward: up to 8 waves (256 VGPRs: x AND dy stay in registers next to
  // ~80 registers of per-channel coefficients)
  const int maxw = bwd ? 8 : 16;
  int nw = (HW + ppw - 1) / ppw; if (nw > maxw) nw = maxw;
  // the per-channel reduction (gn1_block_channel_sums) and the dgamma / dbeta atomics need one THREAD per channel of the
  // block: at least ceil(CB / 64) waves even when HW is tiny (C = 2560 at 2x2: CB = 80, HW = 4).  Padding waves own pixels
  // p >= HW and contribute zeros.
  const int minw = (cb + 63) / 64;
  if (nw < minw) nw = minw;
  g.NW = nw;
  const int per_iter = nw * ppw;
  const int nv = (HW + per_iter - 1) / per_iter;
  g.NV = nv <= 1 ? 1 : nv <= 2 ? 2 : nv <= 4 ? 4 : nv <= 8 ? 8 : 16;
  g.nblk = C / cb;
  g.ok = nv <= (esize == 2 ? 16 : 8) && (long)g.nblk * B >= GN1_MIN_WG;
  return g;
}

// per-channel sums of two quantities over the workgroup's pixels; result valid for lanes / threads that read chs afterwards
//   s[e], q[e]: this lane's sums for its 8 channels (lane % LPR = vector index; inactive lanes hold zeros)
__device__ __forceinline__ void gn1_block_channel_sums(float s[8], float q[8], int LPR, int NW, float* red /*[NW][16][16]*/,
                                                       float* chs /*[128][2]*/, int VX) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int o = 32; o >= 8; o >>= 1) {
    if (o >= LPR) {
#pragma unroll
      for (int e = 0; e < 8; ++e) { s[e] += __shfl_xor(s[e], o, 64); q[e] += __shfl_xor(q[e], o, 64); }
    }
  }
  if (lane < LPR) {
    float* r = red + (wave * 16 + lane) * 16;
#pragma unroll
    for (int e = 0; e < 8; ++e) { r[e] = s[e]; r[8 + e] = q[e]; }
  }
  __syncthreads();
  const int t = threadIdx.x;
  if (t < VX * 8) {                        // one thread per channel of the block
    const int vx = t >> 3, e = t & 7;
    float a = 0.f, b = 0.f;
    for (int w = 0; w < NW; ++w) { a += red[(w * 16 + vx) * 16 + e]; b += red[(w * 16 + vx) * 16 + 8 + e]; }
    chs[2 * t] = a; chs[2 * t + 1] = b;
  }
  __syncthreads();
}

template <typename T, bool SILU, int NV>
__global__ __launch_bounds__(1024) void gn1_fwd_kernel(const T* __restrict__ x, long ldx, T* __restrict__ y, long ldy, int HW,
                                                       int C, int G, int CB, int VX, int LPR, int NW, float eps,
                                                       const float* __restrict__ gamma, const float* __restrict__ beta,
                                                       float* __restrict__ stats) {
  __shared__ float red[16 * 16 * 16];
  __shared__ float chs[128 * 2];
  __shared__ float gst[16 * 2];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int vx = lane % LPR, pl = lane / LPR, ppw = 64 / LPR;
  const int b = blockIdx.y, c0 = blockIdx.x * CB, cg = C / G;
  const bool act = vx < VX;
  const int step = NW * ppw;
  Pack8<T> d[NV];
  float s[8], q[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) { s[e] = 0.f; q[e] = 0.f; }
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int p = wave * ppw + pl + i * step;
    if (act && p < HW) d[i].load(x + ((long)b * HW + p) * ldx + c0 + vx * 8);
  }
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int p = wave * ppw + pl + i * step;
    if (act && p < HW) {
      float f[8]; d[i].get(f);
#pragma unroll
      for (int e = 0; e < 8; ++e) { s[e] += f[e]; q[e] += f[e] * f[e]; }
    }
  }
  gn1_block_channel_sums(s, q, LPR, NW, red, chs, VX);
  const int ng = CB / cg;
  if ((int)threadIdx.x < ng) {
    double S = 0, Q = 0;
    for (int c = threadIdx.x * cg; c < (threadIdx.x + 1) * cg; ++c) { S += chs[2 * c]; Q += chs[2 * c + 1]; }
    const double n = (double)HW * cg, mean = S / n;
    double var = Q / n - mean * mean;
    if (var < 0) var = 0;
    const double rstd = 1.0 / sqrt(var + (double)eps);
    gst[2 * threadIdx.x] = (float)mean; gst[2 * threadIdx.x + 1] = (float)rstd;
    const int gg = c0 / cg + threadIdx.x;
    stats[((long)b * G + gg) * 2] = (float)mean;
    stats[((long)b * G + gg) * 2 + 1] = (float)rstd;
  }
  __syncthreads();
  if (!act) return;
  float sc[8], sh[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const int cl = vx * 8 + e, gi = cl / cg;
    const double scd = (double)gst[2 * gi + 1] * (double)gamma[c0 + cl];
    sc[e] = (float)scd;
    sh[e] = (float)((double)beta[c0 + cl] - (double)gst[2 * gi] * scd);
  }
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int p = wave * ppw + pl + i * step;
    if (p < HW) {
      float f[8]; d[i].get(f);
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const float z = f[e] * sc[e] + sh[e];
        f[e] = SILU ? silu_f(z) : z;
      }
      store8(y + ((long)b * HW + p) * ldy + c0 + vx * 8, f);
    }
  }
}

template <typename T, bool SILU, int NV>
__global__ __launch_bounds__(512) void gn1_bwd_kernel(const T* __restrict__ x, long ldx, const T* __restrict__ dy, long lddy,
                                                       const T* __restrict__ accum, long ldacc, T* __restrict__ dx, long lddx,
                                                       int HW, int C, int G, int CB, int VX, int LPR, int NW,
                                                       const float* __restrict__ gamma, const float* __restrict__ beta,
                                                       const float* __restrict__ stats, float* __restrict__ dgamma,
                                                       float* __restrict__ dbeta) {
  __shared__ float red[16 * 16 * 16];
  __shared__ float chs[128 * 2];
  __shared__ float gst[16 * 2];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int vx = lane % LPR, pl = lane / LPR, ppw = 64 / LPR;
  const int b = blockIdx.y, c0 = blockIdx.x * CB, cg = C / G;
  const bool act = vx < VX;
  const int step = NW * ppw;
  Pack8<T> dxv[NV], ddv[NV];
  float ga[8], be[8], mu[8], rs[8], s[8], q[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const int cl = (act ? vx : 0) * 8 + e, gi = (c0 + cl) / cg;
    ga[e] = gamma[c0 + cl]; be[e] = beta[c0 + cl];
    mu[e] = stats[((long)b * G + gi) * 2]; rs[e] = stats[((long)b * G + gi) * 2 + 1];
    s[e] = 0.f; q[e] = 0.f;
  }
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int p = wave * ppw + pl + i * step;
    if (act && p < HW) {
      dxv[i].load(x + ((long)b * HW + p) * ldx + c0 + vx * 8);
      ddv[i].load(dy + ((long)b * HW + p) * lddy + c0 + vx * 8);
    }
  }
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int p = wave * ppw + pl + i * step;
    if (act && p < HW) {
      float f[8], d[8]; dxv[i].get(f); ddv[i].get(d);
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const float xh = (f[e] - mu[e]) * rs[e];
        float dz = d[e];
        if (SILU) dz *= dsilu_f(xh * ga[e] + be[e]);
        s[e] += dz; q[e] += dz * xh;
      }
    }
  }
  gn1_block_channel_sums(s, q, LPR, NW, red, chs, VX);
  const int ng = CB / cg;
  if (dgamma && (int)threadIdx.x < CB) {
    atomicAdd(dgamma + c0 + threadIdx.x, chs[2 * threadIdx.x + 1]);
    atomicAdd(dbeta + c0 + threadIdx.x, chs[2 * threadIdx.x]);
  }
  if ((int)threadIdx.x < ng) {
    double s1 = 0, s2 = 0;
    for (int c = threadIdx.x * cg; c < (threadIdx.x + 1) * cg; ++c) {
      s1 += (double)gamma[c0 + c] * chs[2 * c]; s2 += (double)gamma[c0 + c] * chs[2 * c + 1];
    }
    gst[2 * threadIdx.x] = (float)s1; gst[2 * threadIdx.x + 1] = (float)s2;   // gamma-weighted group sums
  }
  __syncthreads();
  if (!act) return;
  const double n = (double)HW * cg;
  float k1[8], k2[8], k3[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const int cl = vx * 8 + e, gi = cl / cg;
    const double rstd = rs[e];
    k1[e] = (float)(rstd * ga[e]);
    k2[e] = (float)(rstd * (double)gst[2 * gi] / n);
    k3[e] = (float)(rstd * (double)gst[2 * gi + 1] / n);
  }
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int p = wave * ppw + pl + i * step;
    if (p < HW) {
      float f[8], d[8], ac[8]; dxv[i].get(f); ddv[i].get(d);
      const long row = (long)b * HW + p;
      if (accum) load8(accum + row * ldacc + c0 + vx * 8, ac);
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const float xh = (f[e] - mu[e]) * rs[e];
        float dz = d[e];
        if (SILU) dz *= dsilu_f(xh * ga[e] + be[e]);
        float r = dz * k1[e] - k2[e] - xh * k3[e];
        if (accum) r += ac[e];
        f[e] = r;
      }
      store8(dx + row * lddx + c0 + vx * 8, f);
    }
  }
}

template <typename T, bool SILU>
static void gn1_fwd_launch(const GnArgs& a, const Gn1Geom& g, hipStream_t st) {
  dim3 grid(g.nblk, a.B), blk(g.NW * 64);
#define GN1F(N_) hipLaunchKernelGGL((gn1_fwd_kernel<T, SILU, N_>), grid, blk, 0, st, (const T*)a.x, a.ldx, (T*)a.y, a.ldy, a.HW, a.C, \
                                    a.G, g.CB, g.VX, g.LPR, g.NW, a.eps, a.gamma, a.beta, a.stats)
  switch (g.NV) { case 1: GN1F(1); break; case 2: GN1F(2); break; case 4: GN1F(4); break; case 8: GN1F(8); break; default: GN1F(16); }
#undef GN1F
}

template <typename T, bool SILU>
static void gn1_bwd_launch(const GnBwdArgs& a, const Gn1Geom& g, hipStream_t st) {
  dim3 grid(g.nblk, a.B), blk(g.NW * 64);
#define GN1B(N_) hipLaunchKernelGGL((gn1_bwd_kernel<T, SILU, N_>), grid, blk, 0, st, (const T*)a.x, a.ldx, (const T*)a.dy, a.lddy,  \
                                    (const T*)a.accum, a.ldacc, (T*)a.dx, a.lddx, a.HW, a.C, a.G, g.CB, g.VX, g.LPR, g.NW, a.gamma, \
                                    a.beta, a.stats, a.dgamma, a.dbeta)
  switch (g.NV) { case 1: GN1B(1); break; case 2: GN1B(2); break; case 4: GN1B(4); break; case 8: GN1B(8); break; default: GN1B(16); }
#undef GN1B
}

// ------------------------------------------------------------------ one-launch GroupNorm, one workgroup per (sample, group)
// gn1_* needs channel blocks of whole 16-byte vectors (CB = lcm(C / G, 8)): at C = 320 / 640 that quarters / halves its grid and
// leaves 3 of every 8 lanes idle.  Here ONE workgroup owns ONE (sample, group) pair -- B * G workgroups, 256 at B = 8, G = 32,
// one per CU -- and keeps the pair's [HW][C / G] slab (the backward: x and dy) in registers between the statistics and the
// apply: the tensor is read once and written once by one launch, and no workgroup waits for another.  A row segment of a
// group is C / G * 2 bytes (bf16 only), aligned to VW * 4 = gcd(16, C / G * 2) bytes and no more, so the vectors are 4, 8 or
// 16 bytes: VPR = segment / vector of them per pixel row.  The (pixel, vector) index is flattened over the lanes,
// idx = tid + i * threads, with threads = 64 * NW a multiple of VPR: no lane is idle and every lane keeps ONE vector position
// v = tid % VPR, hence 2 * VW channels whose coefficients it holds in registers.  The whole workgroup is one group, so the
// statistics are two workgroup-wide sums: fp32 per lane and channel (chains of at most NV terms), then fp64 in a fixed order
// (xor tree over the lanes, the waves in sequence) and the fp64 finalisation of gn1_fwd_kernel.  Trainable norms reduce the
// per-channel sums through LDS in a fixed order and add them with one float atomic per channel and sample, as gn1_bwd_kernel.
//
// Budget: NW <= 16 waves, i.e. up to 1024 threads = 4 waves per SIMD = 128 VGPRs per lane (VPR = 5 or 15 at the SD1.5 widths
// gives NW = 15, 960 threads).  Of those the slab may take GNG_FWD_DW = GNG_BWD_DW = 64 dwords (the backward: x and dy
// together; at 88 the compiler spills); tests/test_gpu_groupnorm_group.py compiles the listing and asserts no scratch, no
// spills and 4 waves per SIMD.  So the forward holds up to 61440 vectors ([8, 960, 4096]: 240 KB of 491 KB of registers), the
// backward up to [8, 1920, 1024] (240 KB); the backward of C = 640 / 960 at 64x64 (320 / 480 KB) does not fit and stays on
// the two-launch form.  NV, the vectors per lane and operand, is one of 6, 16, 22, 64; the backward stops at GNG_BWD_NV = 16:
// at [8, 320, 4096] (22 four-byte vectors of x, dy and accum each) it was 2 us faster than the two-launch form on buffers
// that stay in the Infinity Cache and 10 us slower from HBM (profiles/gn_group), so that class is left where it was.
//
// The rule (mode 1) takes a shape with HW >= GNG_MIN_HW and B * G >= GNG_MIN_WG workgroups whose slab fits: every class of
// the SD1.5 step at B = 8 from 16x16 to 64x64 measured faster than gn1_* / the two-launch form by more than the spread of
// repeated medians, the backward classes above excepted.  Below 192 workgroups gn1_* keeps its shapes.
//
// Workgroups are dealt to the 8 XCDs round-robin by linear id.  Neighbouring groups of a sample share 128-byte lines (a
// segment is 20 bytes at C = 320), so where B * G is a multiple of 8 the ids are mapped such that one XCD gets a contiguous
// run of (sample, group) pairs and neighbours are adjacent in id (B = 8: sample = id % 8, group = id / 8): a line is then
// fetched into one L2, and the partial-line stores of neighbours meet there.
static constexpr int GNG_MAX_WAVES = 16, GNG_FWD_DW = 64, GNG_BWD_DW = 64, GNG_MAX_CG = 128;
static constexpr int GNG_BWD_NV = 16, GNG_MIN_HW = 256, GNG_MIN_WG = 192;
int g_gn_group = 1;   // cl_debug_groupnorm_group: 0 never, 1 by rule, 2 whenever the slab fits; + 4 = naive id mapping

struct GngGeom { int cg, VW, VPR, NW, NV, remap; bool ok; };

static GngGeom gng_geom(int B, int HW, int C, int G, bool bwd) {
  GngGeom g{}; g.ok = false;
  const int mode = g_gn_group & 3;
  if (!mode || !g_gn_one_pass || g_gn_three_pass || C % G) return g;
  const int cg = C / G;
  if ((cg & 1) || cg > GNG_MAX_CG) return g;
  if (mode == 1 && (HW < GNG_MIN_HW || (long)B * G < GNG_MIN_WG)) return g;
  g.cg = cg;
  g.VW = cg % 8 == 0 ? 4 : cg % 4 == 0 ? 2 : 1;      // dwords per vector: gcd(16, cg * 2) / 4
  g.VPR = cg / (2 * g.VW);
  int nw = GNG_MAX_WAVES;
  while (nw > 0 && (64 * nw) % g.VPR) --nw;
  if (!nw) return g;
  g.NW = nw;
  const long total = (long)HW * g.VPR, T = 64 * nw;
  const long nv = (total + T - 1) / T;
  g.NV = nv <= 6 ? 6 : nv <= 16 ? 16 : nv <= 22 ? 22 : nv <= 64 ? 64 : 0;
  if (!g.NV || g.NV * g.VW * (bwd ? 2 : 1) > (bwd ? GNG_BWD_DW : GNG_FWD_DW) || (bwd && g.NV > GNG_BWD_NV)) return g;
  g.remap = !(g_gn_group & 4) && ((long)B * G) % 8 == 0;
  g.ok = true;
  return g;
}

template <int VW> __device__ __forceinline__ void gng_ld(const bf16_t* p, uint32_t* d) {
  if constexpr (VW == 4) { const uint4 r = *reinterpret_cast<const uint4*>(p); d[0] = r.x; d[1] = r.y; d[2] = r.z; d[3] = r.w; }
  else if constexpr (VW == 2) { const uint2 r = *reinterpret_cast<const uint2*>(p); d[0] = r.x; d[1] = r.y; }
  else d[0] = *reinterpret_cast<const uint32_t*>(p);
}
template <int VW> __device__ __forceinline__ void gng_get(const uint32_t* d, float* f) {
#pragma unroll
  for (int j = 0; j < VW; ++j) { f[2 * j] = __uint_as_float(d[j] << 16); f[2 * j + 1] = __uint_as_float(d[j] & 0xffff0000u); }
}
template <int VW> __device__ __forceinline__ void gng_st(bf16_t* p, const float* f) {
  if constexpr (VW == 4) {
    uint4 r; r.x = pack2bf(f[0], f[1]); r.y = pack2bf(f[2], f[3]); r.z = pack2bf(f[4], f[5]); r.w = pack2bf(f[6], f[7]);
    *reinterpret_cast<uint4*>(p) = r;
  } else if constexpr (VW == 2) {
    uint2 r; r.x = pack2bf(f[0], f[1]); r.y = pack2bf(f[2], f[3]);
    *reinterpret_cast<uint2*>(p) = r;
  } else *reinterpret_cast<uint32_t*>(p) = pack2bf(f[0], f[1]);
}

// Between the statistics and the apply pass the slab stays PACKED: without this the compiler keeps the unpacked floats of the
// first pass alive for the second (common subexpressions), which doubles the registers of the slab.  Emits no instruction.
template <int NV, int VW> __device__ __forceinline__ void gng_keep_packed(uint32_t (&d)[NV][VW]) {
#pragma unroll
  for (int i = 0; i < NV; ++i) {
#pragma unroll
    for (int j = 0; j < VW; ++j) asm volatile("" : "+v"(d[i][j]));
  }
}

// the (sample, group) pair of this workgroup
__device__ __forceinline__ void gng_owner(int B, int G, int remap, int& b, int& g) {
  int id = blockIdx.x;
  if (remap) id = (id & 7) * ((B * G) >> 3) + (id >> 3);
  b = id / G; g = id - b * G;
}

// workgroup-wide sums of two doubles in a fixed order (xor tree over the lanes, then the waves in sequence); valid in every thread
__device__ __forceinline__ void gng_block_sum2(double& a, double& b, double (*red)[GNG_MAX_WAVES]) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { a += __shfl_xor(a, o, 64); b += __shfl_xor(b, o, 64); }
  const int wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
  if ((threadIdx.x & 63) == 0) { red[0][wave] = a; red[1][wave] = b; }
  __syncthreads();
  a = 0; b = 0;
  for (int w = 0; w < nw; ++w) { a += red[0][w]; b += red[1][w]; }
}

template <bool SILU, int VW, int NV>
__global__ __launch_bounds__(1024) void gng_fwd_kernel(const bf16_t* __restrict__ x, long ldx, bf16_t* __restrict__ y, long ldy,
                                                        int B, int HW, int G, int cg, int VPR, int remap, float eps,
                                                        const float* __restrict__ gamma, const float* __restrict__ beta,
                                                        float* __restrict__ stats) {
  constexpr int EPV = 2 * VW;
  __shared__ double red[2][GNG_MAX_WAVES];
  int b, g; gng_owner(B, G, remap, b, g);
  const int tid = threadIdx.x, PL = blockDim.x / VPR;
  const int p0 = tid / VPR, v = tid - p0 * VPR, c0 = g * cg + v * EPV;
  int cnt = p0 < HW ? (HW - p0 + PL - 1) / PL : 0;           // this lane's pixels: p0, p0 + PL, ...
  // every load is issued, straight-line: slots past the lane's last pixel re-read that pixel (a lane without pixels: the
  // sample's last row), in bounds and served by L1, and count for nothing below
  const bf16_t* xp = x + ((long)b * HW + min(p0, HW - 1)) * ldx + c0;
  const long xs = (long)PL * ldx;
  uint32_t d[NV][VW];
#pragma unroll
  for (int i = 0; i < NV; ++i) { gng_ld<VW>(xp, d[i]); if (i + 1 < cnt) xp += xs; }
  asm volatile("" : "+v"(cnt));            // the NV comparisons with cnt are made again in every pass, not kept in scalar registers
  float s[EPV], q[EPV];
#pragma unroll
  for (int e = 0; e < EPV; ++e) { s[e] = 0.f; q[e] = 0.f; }
#pragma unroll
  for (int i = 0; i < NV; ++i)
    if (i < cnt) {
      float f[EPV]; gng_get<VW>(d[i], f);
#pragma unroll
      for (int e = 0; e < EPV; ++e) { s[e] += f[e]; q[e] += f[e] * f[e]; }
    }
  double S = 0, Q = 0;
#pragma unroll
  for (int e = 0; e < EPV; ++e) { S += s[e]; Q += q[e]; }
  gng_block_sum2(S, Q, red);
  const double n = (double)HW * cg, mean = S / n;
  double var = Q / n - mean * mean;
  if (var < 0) var = 0;
  const float mean_f = (float)mean, rstd_f = (float)(1.0 / sqrt(var + (double)eps));
  if (tid == 0) { stats[((long)b * G + g) * 2] = mean_f; stats[((long)b * G + g) * 2 + 1] = rstd_f; }
  gng_keep_packed<NV, VW>(d);
  asm volatile("" : "+v"(cnt));
  float sc[EPV], sh[EPV];
#pragma unroll
  for (int e = 0; e < EPV; ++e) {
    const double scd = (double)rstd_f * (double)gamma[c0 + e];
    sc[e] = (float)scd;
    sh[e] = (float)((double)beta[c0 + e] - (double)mean_f * scd);
  }
  bf16_t* yp = y + ((long)b * HW + p0) * ldy + c0;
  const long ys = (long)PL * ldy;
#pragma unroll
  for (int i = 0; i < NV; ++i)
    if (i < cnt) {
      float f[EPV]; gng_get<VW>(d[i], f);
#pragma unroll
      for (int e = 0; e < EPV; ++e) {
        const float z = f[e] * sc[e] + sh[e];
        f[e] = SILU ? silu_f(z) : z;
      }
      gng_st<VW>(yp, f); yp += ys;
    }
}

// per-channel totals of one quantity over the workgroup's pixels, added onto dst[0 .. cg) with one float atomic per channel.
// Lane t holds val[e] for channel (t % VPR) * EPV + e; lsum is [EPV][threads], lpart [cg][8].  Fixed order: deterministic.
template <int EPV>
__device__ __forceinline__ void gng_channel_atomics(const float* val, int cg, int VPR, float* lsum, float* lpart, float* dst) {
  const int tid = threadIdx.x, T = blockDim.x, PL = T / VPR;
  __syncthreads();
#pragma unroll
  for (int e = 0; e < EPV; ++e) lsum[e * T + tid] = val[e];
  __syncthreads();
  for (int i = tid; i < cg * 8; i += T) {
    const int cl = i >> 3, v = cl / EPV, e = cl - v * EPV;
    float a = 0.f;
    for (int j = i & 7; j < PL; j += 8) a += lsum[e * T + v + VPR * j];
    lpart[i] = a;
  }
  __syncthreads();
  if (tid < cg) {
    float a = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) a += lpart[tid * 8 + j];
    atomicAdd(dst + tid, a);
  }
}

template <bool SILU, int VW, int NV>
__global__ __launch_bounds__(1024) void gng_bwd_kernel(const bf16_t* __restrict__ x, long ldx, const bf16_t* __restrict__ dy, long lddy,
                                                        const bf16_t* __restrict__ accum, long ldacc, bf16_t* __restrict__ dx, long lddx,
                                                        int B, int HW, int G, int cg, int VPR, int remap,
                                                        const float* __restrict__ gamma, const float* __restrict__ beta,
                                                        const float* __restrict__ stats, float* __restrict__ dgamma,
                                                        float* __restrict__ dbeta) {
  constexpr int EPV = 2 * VW;
  __shared__ double red[2][GNG_MAX_WAVES];
  __shared__ float lsum[EPV * 64 * GNG_MAX_WAVES];
  __shared__ float lpart[GNG_MAX_CG * 8];
  int b, g; gng_owner(B, G, remap, b, g);
  const int tid = threadIdx.x, PL = blockDim.x / VPR;
  const int p0 = tid / VPR, v = tid - p0 * VPR, c0 = g * cg + v * EPV;
  int cnt = p0 < HW ? (HW - p0 + PL - 1) / PL : 0;
  const long row0 = (long)b * HW + min(p0, HW - 1);          // loads past the lane's last pixel: as gng_fwd_kernel
  const bf16_t* xp = x + row0 * ldx + c0;
  const bf16_t* dp = dy + row0 * lddy + c0;
  const long xs = (long)PL * ldx, ds = (long)PL * lddy;
  uint32_t dxv[NV][VW], ddv[NV][VW];
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    gng_ld<VW>(xp, dxv[i]); gng_ld<VW>(dp, ddv[i]);
    if (i + 1 < cnt) { xp += xs; dp += ds; }
  }
  asm volatile("" : "+v"(cnt));
  const float mu = stats[((long)b * G + g) * 2], rs = stats[((long)b * G + g) * 2 + 1];
  float ga[EPV], be[EPV], s[EPV], q[EPV];
#pragma unroll
  for (int e = 0; e < EPV; ++e) { ga[e] = gamma[c0 + e]; be[e] = beta[c0 + e]; s[e] = 0.f; q[e] = 0.f; }
#pragma unroll
  for (int i = 0; i < NV; ++i)
    if (i < cnt) {
      float f[EPV], d[EPV]; gng_get<VW>(dxv[i], f); gng_get<VW>(ddv[i], d);
#pragma unroll
      for (int e = 0; e < EPV; ++e) {
        const float xh = (f[e] - mu) * rs;
        float dz = d[e];
        if (SILU) dz *= dsilu_f(xh * ga[e] + be[e]);
        s[e] += dz; q[e] += dz * xh;
      }
    }
  double s1 = 0, s2 = 0;                   // gamma-weighted group sums
#pragma unroll
  for (int e = 0; e < EPV; ++e) { s1 += (double)ga[e] * s[e]; s2 += (double)ga[e] * q[e]; }
  gng_block_sum2(s1, s2, red);
  if (dgamma) {
    gng_channel_atomics<EPV>(q, cg, VPR, lsum, lpart, dgamma + g * cg);
    gng_channel_atomics<EPV>(s, cg, VPR, lsum, lpart, dbeta + g * cg);
  }
  gng_keep_packed<NV, VW>(dxv);
  gng_keep_packed<NV, VW>(ddv);
  asm volatile("" : "+v"(cnt));
  const double n = (double)HW * cg, rstd = rs;
  const float k2 = (float)(rstd * s1 / n), k3 = (float)(rstd * s2 / n);
  float k1[EPV];
#pragma unroll
  for (int e = 0; e < EPV; ++e) k1[e] = (float)(rstd * ga[e]);
  bf16_t* op = dx + row0 * lddx + c0;
  const bf16_t* ap = accum ? accum + row0 * ldacc + c0 : nullptr;
  const long os = (long)PL * lddx, as = (long)PL * ldacc;
#pragma unroll
  for (int i = 0; i < NV; ++i)
    if (i < cnt) {
      float f[EPV], d[EPV], ac[EPV]; gng_get<VW>(dxv[i], f); gng_get<VW>(ddv[i], d);
      if (accum) { uint32_t av[VW]; gng_ld<VW>(ap, av); gng_get<VW>(av, ac); ap += as; }
#pragma unroll
      for (int e = 0; e < EPV; ++e) {
        const float xh = (f[e] - mu) * rs;
        float dz = d[e];
        if (SILU) dz *= dsilu_f(xh * ga[e] + be[e]);
        float r = dz * k1[e] - k2 - xh * k3;
        if (accum) r += ac[e];
        f[e] = r;
      }
      gng_st<VW>(op, f); op += os;
    }
}

static void gng_rec(int kind, const GngGeom& g, int B, int G) {
  g_norm_last = NormLaunchRec{kind, NORM_FORM_GROUP, CL_BF16, g.NV, g.VPR, g.NW * 64, g.cg, 0, B * G, 1, 0, 1};
}

// every (VW, NV) pair the budgets admit: X(VW, NV)
#define GNG_FWD_FORMS(X) X(1, 6) X(1, 16) X(1, 22) X(1, 64) X(2, 6) X(2, 16) X(2, 22) X(4, 6) X(4, 16)
#define GNG_BWD_FORMS(X) X(1, 6) X(1, 16) X(2, 6) X(2, 16) X(4, 6)

template <bool SILU>
static int gng_fwd_launch(const GnArgs& a, const GngGeom& g, hipStream_t st) {
  const dim3 grid(a.B * a.G), blk(g.NW * 64);
#define GNG_F(VW_, NV_)                                                                                                          \
  if (g.VW == VW_ && g.NV == NV_)                                                                                                \
    hipLaunchKernelGGL((gng_fwd_kernel<SILU, VW_, NV_>), grid, blk, 0, st, (const bf16_t*)a.x, a.ldx, (bf16_t*)a.y, a.ldy, a.B, \
                       a.HW, a.G, g.cg, g.VPR, g.remap, a.eps, a.gamma, a.beta, a.stats);
  GNG_FWD_FORMS(GNG_F)
#undef GNG_F
  CL_CHECK_LAUNCH();
  gng_rec(NORM_GN_FWD, g, a.B, a.G);
  return CL_OK;
}

template <bool SILU>
static int gng_bwd_launch(const GnBwdArgs& a, const GngGeom& g, hipStream_t st) {
  const dim3 grid(a.B * a.G), blk(g.NW * 64);
#define GNG_B(VW_, NV_)                                                                                                          \
  if (g.VW == VW_ && g.NV == NV_)                                                                                                \
    hipLaunchKernelGGL((gng_bwd_kernel<SILU, VW_, NV_>), grid, blk, 0, st, (const bf16_t*)a.x, a.ldx, (const bf16_t*)a.dy,      \
                       a.lddy, (const bf16_t*)a.accum, a.ldacc, (bf16_t*)a.dx, a.lddx, a.B, a.HW, a.G, g.cg, g.VPR, g.remap,    \
                       a.gamma, a.beta, a.stats, a.dgamma, a.dbeta);
  GNG_BWD_FORMS(GNG_B)
#undef GNG_B
  CL_CHECK_LAUNCH();
  gng_rec(NORM_GN_BWD, g, a.B, a.G);
  return CL_OK;
}

static bool gn_two_pass_ok(const GnGeom& g, int C, int G) {
  return !g_gn_three_pass && C / 8 == g.VX && G <= 64 && g.threads >= G && g.threads >= 64;
}

template <typename T>
static int gn_fwd_t(const GnArgs& a, hipStream_t st) {
  const Gn1Geom g1 = gn1_geom(a.B, a.HW, a.C, a.G, (int)sizeof(T), false);
  if (g1.ok) {
    if (a.silu) gn1_fwd_launch<T, true>(a, g1, st); else gn1_fwd_launch<T, false>(a, g1, st);
    CL_CHECK_LAUNCH();
    gn_rec1(NORM_GN_FWD, sizeof(T) == 2 ? CL_BF16 : CL_F32, g1, a.B);
    return CL_OK;
  }
  const GnGeom g = gn_geom(a.B, a.HW, a.C);
  if (gn_two_pass_ok(g, a.C, a.G)) {
    dim3 grid(g.nchunk, a.B);
    const int lds = std::max(g.threads * 64, a.C * 8);
    hipLaunchKernelGGL((gn_gpartial_kernel<T>), grid, dim3(g.threads), lds, st, (const T*)a.x, a.ldx, a.HW, a.C, a.G,
                       g.VX, g.PY, g.ppc, g.nchunk, a.ws);
    if (a.silu)
      hipLaunchKernelGGL((gn_gapply_kernel<T, true>), grid, dim3(g.threads), 0, st, (const T*)a.x, a.ldx, (T*)a.y, a.ldy,
                         a.HW, a.C, a.G, g.VX, g.PY, g.ppc, g.nchunk, a.eps, a.gamma, a.beta, a.ws, a.stats);
    else
      hipLaunchKernelGGL((gn_gapply_kernel<T, false>), grid, dim3(g.threads), 0, st, (const T*)a.x, a.ldx, (T*)a.y, a.ldy,
                         a.HW, a.C, a.G, g.VX, g.PY, g.ppc, g.nchunk, a.eps, a.gamma, a.beta, a.ws, a.stats);
    CL_CHECK_LAUNCH();
    gn_rec(NORM_GN_FWD, NORM_FORM_TWO, sizeof(T) == 2 ? CL_BF16 : CL_F32, g, a.B, a.C);
    return CL_OK;
  }
  float* partial = a.ws;
  float* coef = a.ws + (long)a.B * g.nchunk * a.C * 2;
  dim3 grid(g.nchunk, a.B);
  hipLaunchKernelGGL((gn_partial_kernel<T>), grid, dim3(g.threads), g.threads * 64, st,
                     (const T*)a.x, a.ldx, a.HW, a.C, g.VX, g.PY, g.ppc, g.nchunk, partial);
  hipLaunchKernelGGL(gn_finalize_kernel, dim3(a.G, a.B), dim3(256), 0, st,
                     partial, g.nchunk, a.HW, a.C, a.G, a.eps, a.gamma, a.beta, a.stats, coef);
  if (a.silu)
    hipLaunchKernelGGL((gn_apply_kernel<T, true>), grid, dim3(g.threads), 0, st,
                       (const T*)a.x, a.ldx, (T*)a.y, a.ldy, a.HW, a.C, g.VX, g.PY, g.ppc, coef);
  else
    hipLaunchKernelGGL((gn_apply_kernel<T, false>), grid, dim3(g.threads), 0, st,
                       (const T*)a.x, a.ldx, (T*)a.y, a.ldy, a.HW, a.C, g.VX, g.PY, g.ppc, coef);
  CL_CHECK_LAUNCH();
  gn_rec(NORM_GN_FWD, NORM_FORM_THREE, sizeof(T) == 2 ? CL_BF16 : CL_F32, g, a.B, a.C);
  return CL_OK;
}

int gn_fwd(const GnArgs& a, int dtype, hipStream_t st) {
  norm_rec_begin();
  if (a.C % 8 || a.C % a.G || a.ldx % 8 || a.ldy % 8 || a.C > 8192) return CL_EINVAL;
  if (a.C / 8 > 320 && (a.C / 8) % 320) return CL_EINVAL;  // uniform trip count across the block
  if (gnc_fwd(a, dtype, st) == CL_OK) return CL_OK;        // groups spanning >= 1024 pixels: one launch, one pass (norm_coop.hip)
  if (dtype == CL_BF16) {                                  // one workgroup per (sample, group), where the rule takes the shape
    const GngGeom gg = gng_geom(a.B, a.HW, a.C, a.G, false);
    if (gg.ok) return a.silu ? gng_fwd_launch<true>(a, gg, st) : gng_fwd_launch<false>(a, gg, st);
  }
  return dtype == CL_BF16 ? gn_fwd_t<bf16_t>(a, st) : gn_fwd_t<float>(a, st);
}

// ------------------------------------------------------------------ backward

template <typename T, bool SILU>
__global__ void gn_bwd_partial_kernel(const T* __restrict__ x, long ldx, const T* __restrict__ dy, long lddy,
                                      int HW, int C, int G, int VX, int PY, int ppc, int nchunk,
                                      const float* __restrict__ gamma, const float* __restrict__ beta,
                                      const float* __restrict__ stats, float* __restrict__ partial) {
  extern __shared__ float red[];
  const int C8 = C / 8, cg = C / G;
  const int vx = threadIdx.x % VX, py = threadIdx.x / VX;
  const int b = blockIdx.y, chunk = blockIdx.x;
  const int p0 = chunk * ppc, p1 = min(HW, p0 + ppc);
  for (int v = vx; v < C8; v += VX) {
    float ga[8], be[8], mu[8], rs[8], s[8], q[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int c = v * 8 + e, g = c / cg;
      ga[e] = gamma[c]; be[e] = beta[c];
      mu[e] = stats[((long)b * G + g) * 2]; rs[e] = stats[((long)b * G + g) * 2 + 1];
      s[e] = 0.f; q[e] = 0.f;
    }
  #pragma unroll 4
  for (int p = p0 + py; p < p1; p += PY) {
      float f[8], d[8];
      const long row = (long)b * HW + p;
      load8(x + row * ldx + v * 8, f);
      load8(dy + row * lddy + v * 8, d);
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const float xh = (f[e] - mu[e]) * rs[e];
        float dz = d[e];
        if (SILU) dz *= dsilu_f(xh * ga[e] + be[e]);
        s[e] += dz; q[e] += dz * xh;
      }
    }
    float* r = red + (py * VX + vx) * 16;
#pragma unroll
    for (int e = 0; e < 8; ++e) { r[e] = s[e]; r[8 + e] = q[e]; }
    __syncthreads();
    if (py == 0) {
      for (int k = 1; k < PY; ++k) {
        const float* o = red + (k * VX + vx) * 16;
#pragma unroll
        for (int e = 0; e < 8; ++e) { s[e] += o[e]; q[e] += o[8 + e]; }
      }
      float* dst = partial + (((long)b * nchunk + chunk) * C + v * 8) * 2;
#pragma unroll
      for (int e = 0; e < 8; ++e) { dst[2 * e] = s[e]; dst[2 * e + 1] = q[e]; }
    }
    __syncthreads();
  }
}

// per (b, group): channel sums -> group sums -> apply coefficients; optional dgamma/dbeta accumulation
__global__ __launch_bounds__(256) void gn_bwd_finalize_kernel(const float* __restrict__ partial, int nchunk, int HW,
                                                              int C, int G, const float* __restrict__ gamma,
                                                              const float* __restrict__ stats,
                                                              float* __restrict__ bcoef /*[B][C][4]: k1,k2,k3,_*/,
                                                              float* __restrict__ dgamma, float* __restrict__ dbeta) {
  // one workgroup per (sample, group).  Thread t owns channel t % CL of the group and the chunks
  // k = t / CL, t / CL + 256 / CL, ...  (CL = channels rounded up to a power of two <= 256); per-channel
  // totals are combined through LDS so that dgamma / dbeta need one atomic per channel.
  __shared__ double red[8];
  __shared__ double chs[256], chq[256];
  const int g = blockIdx.x, b = blockIdx.y, cg = C / G, tid = threadIdx.x;
  int CL = 1;
  while (CL < cg && CL < 256) CL <<= 1;
  const int KL = 256 / CL;                         // chunk lanes per channel
  const int cl = tid % CL, kl = tid / CL;
  double s1 = 0, s2 = 0;
  for (int c0 = 0; c0 < cg; c0 += CL) {            // one round unless cg > 256
    const int c = g * cg + c0 + cl;
    double s = 0, q = 0;
    if (c0 + cl < cg) {
      for (int k = kl; k < nchunk; k += KL) {
        const float2 p = *reinterpret_cast<const float2*>(partial + (((long)b * nchunk + k) * C + c) * 2);
        s += p.x; q += p.y;
      }
    }
    __syncthreads();
    chs[tid] = s; chq[tid] = q;
    __syncthreads();
    if (kl == 0 && c0 + cl < cg) {
      for (int k = 1; k < KL; ++k) { s += chs[k * CL + cl]; q += chq[k * CL + cl]; }
      if (dgamma) { atomicAdd(dgamma + c, (float)q); atomicAdd(dbeta + c, (float)s); }
      s1 += (double)gamma[c] * s; s2 += (double)gamma[c] * q;
    }
  }
  block_sum2(s1, s2, red);
  const double n = (double)HW * cg;
  const double rstd = stats[((long)b * G + g) * 2 + 1];
  const float k2 = (float)(rstd * s1 / n), k3 = (float)(rstd * s2 / n);
  for (int c = g * cg + tid; c < (g + 1) * cg; c += 256) {
    float* o = bcoef + ((long)b * C + c) * 4;
    o[0] = (float)(rstd * gamma[c]); o[1] = k2; o[2] = k3; o[3] = 0.f;
  }
}

template <typename T, bool SILU>
__global__ void gn_bwd_apply_kernel(const T* __restrict__ x, long ldx, const T* __restrict__ dy, long lddy,
                                    const T* __restrict__ accum, long ldacc, T* __restrict__ dx, long lddx,
                                    int HW, int C, int G, int VX, int PY, int ppc,
                                    const float* __restrict__ gamma, const float* __restrict__ beta,
                                    const float* __restrict__ stats, const float* __restrict__ bcoef) {
  const int C8 = C / 8, cg = C / G;
  const int vx = threadIdx.x % VX, py = threadIdx.x / VX;
  const int b = blockIdx.y, chunk = blockIdx.x;
  const int p0 = chunk * ppc, p1 = min(HW, p0 + ppc);
  for (int v = vx; v < C8; v += VX) {
    float ga[8], be[8], mu[8], rs[8], k1[8], k2[8], k3[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int c = v * 8 + e, g = c / cg;
      ga[e] = gamma[c]; be[e] = beta[c];
      mu[e] = stats[((long)b * G + g) * 2]; rs[e] = stats[((long)b * G + g) * 2 + 1];
      const float* o = bcoef + ((long)b * C + c) * 4;
      k1[e] = o[0]; k2[e] = o[1]; k3[e] = o[2];
    }
  #pragma unroll 4
  for (int p = p0 + py; p < p1; p += PY) {
      float f[8], d[8], ac[8];
      const long row = (long)b * HW + p;
      load8(x + row * ldx + v * 8, f);
      load8(dy + row * lddy + v * 8, d);
      if (accum) load8(accum + row * ldacc + v * 8, ac);
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const float xh = (f[e] - mu[e]) * rs[e];
        float dz = d[e];
        if (SILU) dz *= dsilu_f(xh * ga[e] + be[e]);
        float r = dz * k1[e] - k2[e] - xh * k3[e];
        if (accum) r += ac[e];
        f[e] = r;
      }
      store8(dx + row * lddx + v * 8, f);
    }
  }
}

// two-launch backward for FROZEN norms (no dgamma / dbeta): the statistics pass forms the gamma-weighted group sums
// s1 = sum_c gamma_c sum dz, s2 = sum_c gamma_c sum dz xhat of its chunk; the apply pass totals them itself.
template <typename T, bool SILU>
__global__ void gn_bwd_gpartial_kernel(const T* __restrict__ x, long ldx, const T* __restrict__ dy, long lddy, int HW,
                                       int C, int G, int VX, int PY, int ppc, int nchunk,
                                       const float* __restrict__ gamma, const float* __restrict__ beta,
                                       const float* __restrict__ stats, float* __restrict__ gpartial) {
  extern __shared__ float red[];
  const int cg = C / G;
  const int vx = threadIdx.x % VX, py = threadIdx.x / VX;
  const int b = blockIdx.y, chunk = blockIdx.x;
  const int p0 = chunk * ppc, p1 = min(HW, p0 + ppc);
  float ga[8], be[8], mu[8], rs[8], s[8], q[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const int c = vx * 8 + e, gi = c / cg;
    ga[e] = gamma[c]; be[e] = beta[c];
    mu[e] = stats[((long)b * G + gi) * 2]; rs[e] = stats[((long)b * G + gi) * 2 + 1];
    s[e] = 0.f; q[e] = 0.f;
  }
#pragma unroll 4
  for (int p = p0 + py; p < p1; p += PY) {
    float f[8], d[8];
    const long row = (long)b * HW + p;
    load8(x + row * ldx + vx * 8, f);
    load8(dy + row * lddy + vx * 8, d);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const float xh = (f[e] - mu[e]) * rs[e];
      float dz = d[e];
      if (SILU) dz *= dsilu_f(xh * ga[e] + be[e]);
      s[e] += dz; q[e] += dz * xh;
    }
  }
  float* r = red + (py * VX + vx) * 16;
#pragma unroll
  for (int e = 0; e < 8; ++e) { r[e] = s[e]; r[8 + e] = q[e]; }
  __syncthreads();
  if (py == 0) {
    for (int k = 1; k < PY; ++k) {
      const float* o = red + (k * VX + vx) * 16;
#pragma unroll
      for (int e = 0; e < 8; ++e) { s[e] += o[e]; q[e] += o[8 + e]; }
    }
  }
  __syncthreads();
  if (py == 0) {
    float* ch = red + vx * 16;
#pragma unroll
    for (int e = 0; e < 8; ++e) { ch[2 * e] = ga[e] * s[e]; ch[2 * e + 1] = ga[e] * q[e]; }
  }
  __syncthreads();
  if ((int)threadIdx.x < G) {
    const int c0 = threadIdx.x * cg;
    float S = 0.f, Q = 0.f;
    for (int c = c0; c < c0 + cg; ++c) { S += red[2 * c]; Q += red[2 * c + 1]; }
    float* dst = gpartial + (((long)b * nchunk + chunk) * G + threadIdx.x) * 2;
    dst[0] = S; dst[1] = Q;
  }
}

template <typename T, bool SILU>
__global__ void gn_bwd_gapply_kernel(const T* __restrict__ x, long ldx, const T* __restrict__ dy, long lddy,
                                     const T* __restrict__ accum, long ldacc, T* __restrict__ dx, long lddx, int HW,
                                     int C, int G, int VX, int PY, int ppc, int nchunk, const float* __restrict__ gamma,
                                     const float* __restrict__ beta, const float* __restrict__ stats,
                                     const float* __restrict__ gpartial) {
  __shared__ double part[8][64][2];
  __shared__ double tot[64][2];
  const int b = blockIdx.y, chunk = blockIdx.x, cg = C / G;
  gn_group_totals(gpartial, b, nchunk, G, part, tot);
  const double n = (double)HW * cg;
  const int vx = threadIdx.x % VX, py = threadIdx.x / VX;
  const int p0 = chunk * ppc, p1 = min(HW, p0 + ppc);
  float ga[8], be[8], mu[8], rs[8], k1[8], k2[8], k3[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const int c = vx * 8 + e, gi = c / cg;
    ga[e] = gamma[c]; be[e] = beta[c];
    mu[e] = stats[((long)b * G + gi) * 2]; rs[e] = stats[((long)b * G + gi) * 2 + 1];
    const double rstd = rs[e];
    k1[e] = (float)(rstd * ga[e]);
    k2[e] = (float)(rstd * tot[gi][0] / n);
    k3[e] = (float)(rstd * tot[gi][1] / n);
  }
#pragma unroll 4
  for (int p = p0 + py; p < p1; p += PY) {
    float f[8], d[8], ac[8];
    const long row = (long)b * HW + p;
    load8(x + row * ldx + vx * 8, f);
    load8(dy + row * lddy + vx * 8, d);
    if (accum) load8(accum + row * ldacc + vx * 8, ac);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const float xh = (f[e] - mu[e]) * rs[e];
      float dz = d[e];
      if (SILU) dz *= dsilu_f(xh * ga[e] + be[e]);
      float r = dz * k1[e] - k2[e] - xh * k3[e];
      if (accum) r += ac[e];
      f[e] = r;
    }
    store8(dx + row * lddx + vx * 8, f);
  }
}

template <typename T>
static int gn_bwd_t(const GnBwdArgs& a, hipStream_t st) {
  const Gn1Geom g1 = gn1_geom(a.B, a.HW, a.C, a.G, (int)sizeof(T), true);
  if (g1.ok) {
    if (a.silu) gn1_bwd_launch<T, true>(a, g1, st); else gn1_bwd_launch<T, false>(a, g1, st);
    CL_CHECK_LAUNCH();
    gn_rec1(NORM_GN_BWD, sizeof(T) == 2 ? CL_BF16 : CL_F32, g1, a.B);
    return CL_OK;
  }
  const GnGeom g = gn_geom(a.B, a.HW, a.C);
  if (!a.dgamma && gn_two_pass_ok(g, a.C, a.G)) {
    dim3 grid(g.nchunk, a.B);
    const int lds = std::max(g.threads * 64, a.C * 8);
#define GN_BWD_G(S)                                                                                                \
    hipLaunchKernelGGL((gn_bwd_gpartial_kernel<T, S>), grid, dim3(g.threads), lds, st, (const T*)a.x, a.ldx,        \
                       (const T*)a.dy, a.lddy, a.HW, a.C, a.G, g.VX, g.PY, g.ppc, g.nchunk, a.gamma, a.beta, a.stats, \
                       a.ws);                                                                                       \
    hipLaunchKernelGGL((gn_bwd_gapply_kernel<T, S>), grid, dim3(g.threads), 0, st, (const T*)a.x, a.ldx,            \
                       (const T*)a.dy, a.lddy, (const T*)a.accum, a.ldacc, (T*)a.dx, a.lddx, a.HW, a.C, a.G, g.VX,  \
                       g.PY, g.ppc, g.nchunk, a.gamma, a.beta, a.stats, a.ws);
    if (a.silu) { GN_BWD_G(true) } else { GN_BWD_G(false) }
#undef GN_BWD_G
    CL_CHECK_LAUNCH();
    gn_rec(NORM_GN_BWD, NORM_FORM_TWO, sizeof(T) == 2 ? CL_BF16 : CL_F32, g, a.B, a.C);
    return CL_OK;
  }
  float* partial = a.ws;
  float* bcoef = a.ws + (long)a.B * g.nchunk * a.C * 2;
  dim3 grid(g.nchunk, a.B);
#define GN_BWD_LAUNCH(S)                                                                                       \
  hipLaunchKernelGGL((gn_bwd_partial_kernel<T, S>), grid, dim3(g.threads), g.threads * 64, st, (const T*)a.x,   \
                     a.ldx, (const T*)a.dy, a.lddy, a.HW, a.C, a.G, g.VX, g.PY, g.ppc, g.nchunk, a.gamma,       \
                     a.beta, a.stats, partial);                                                                \
  hipLaunchKernelGGL(gn_bwd_finalize_kernel, dim3(a.G, a.B), dim3(256), 0, st,                                    \
                     partial, g.nchunk, a.HW, a.C, a.G, a.gamma, a.stats, bcoef, a.dgamma, a.dbeta);            \
  hipLaunchKernelGGL((gn_bwd_apply_kernel<T, S>), grid, dim3(g.threads), 0, st, (const T*)a.x, a.ldx,           \
                     (const T*)a.dy, a.lddy, (const T*)a.accum, a.ldacc, (T*)a.dx, a.lddx, a.HW, a.C, a.G,      \
                     g.VX, g.PY, g.ppc, a.gamma, a.beta, a.stats, bcoef);
  if (a.silu) { GN_BWD_LAUNCH(true) } else { GN_BWD_LAUNCH(false) }
#undef GN_BWD_LAUNCH
  CL_CHECK_LAUNCH();
  gn_rec(NORM_GN_BWD, NORM_FORM_THREE, sizeof(T) == 2 ? CL_BF16 : CL_F32, g, a.B, a.C);
  return CL_OK;
}

int gn_bwd(const GnBwdArgs& a, int dtype, hipStream_t st) {
  norm_rec_begin();
  if (a.C % 8 || a.C % a.G || a.ldx % 8 || a.lddy % 8 || a.lddx % 8 || a.C > 8192) return CL_EINVAL;
  if (a.C / 8 > 320 && (a.C / 8) % 320) return CL_EINVAL;
  if (a.accum && a.ldacc % 8) return CL_EINVAL;
  if ((a.dgamma == nullptr) != (a.dbeta == nullptr)) return CL_EINVAL;
  if (gnc_bwd(a, dtype, st) == CL_OK) return CL_OK;
  if (dtype == CL_BF16) {
    const GngGeom gg = gng_geom(a.B, a.HW, a.C, a.G, true);
    if (gg.ok) return a.silu ? gng_bwd_launch<true>(a, gg, st) : gng_bwd_launch<false>(a, gg, st);
  }
  return dtype == CL_BF16 ? gn_bwd_t<bf16_t>(a, st) : gn_bwd_t<float>(a, st);
}

// ------------------------------------------------------------------ LayerNorm

static constexpr int LN_MAXV = 3;  // vectors of 8 per lane -> D <= 1536 (SD1.5: 320 / 640 / 1280)

template <typename T>
__global__ __launch_bounds__(256) void ln_fwd_kernel(const T* __restrict__ x, long ldx, T* __restrict__ y,
                                                     long ldy, int M, int D, float eps,
                                                     const float* __restrict__ gamma,
                                                     const float* __restrict__ beta,
                                                     float* __restrict__ stats /*[M][2]*/) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int D8 = D / 8;
  for (long row = (long)blockIdx.x * 4 + wave; row < M; row += (long)gridDim.x * 4) {
    float f[LN_MAXV][8];
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < LN_MAXV; ++k) {
      const int v = lane + 64 * k;
      if (v < D8) {
        load8(x + row * ldx + v * 8, f[k]);
#pragma unroll
        for (int e = 0; e < 8; ++e) s += f[k][e];
      }
    }
    const float mean = wave_sum(s) / D;
    float q = 0.f;
#pragma unroll
    for (int k = 0; k < LN_MAXV; ++k) {
      const int v = lane + 64 * k;
      if (v < D8) {
#pragma unroll
        for (int e = 0; e < 8; ++e) { const float d = f[k][e] - mean; q += d * d; }
      }
    }
    const float rstd = rsqrtf(wave_sum(q) / D + eps);
    if (lane == 0 && stats) { stats[row * 2] = mean; stats[row * 2 + 1] = rstd; }
#pragma unroll
    for (int k = 0; k < LN_MAXV; ++k) {
      const int v = lane + 64 * k;
      if (v < D8) {
        float o[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) o[e] = (f[k][e] - mean) * rstd * gamma[v * 8 + e] + beta[v * 8 + e];
        store8(y + row * ldy + v * 8, o);
      }
    }
  }
}

// (Round 3 tried RPI = 4 / 2 / 1 rows per wave in flight in the FORWARD as the backward does: measured slower -- 21.2 us
// instead of 14.7 us for the 42 MB of a 64x64 LayerNorm, 1.04 instead of 0.72 ms per step -- and removed:
// profiles/r03_final/ln_rows_negative.txt.  With one row per wave the grid already keeps 32 waves per CU streaming.)
// dx = rstd * (dyh - mean(dyh) - xh * mean(dyh * xh)),  dyh = dy * gamma ; optional (+ accum)
// WG: dgamma += sum_rows dy * xh ; dbeta += sum_rows dy  (per-lane column sums -> LDS across the 4 waves
// -> block partial row, or one fp32 atomic per column per workgroup)
// NV = 16-byte vectors per lane (D <= 512 NV); RPI = rows per wave iteration, all kept in registers between
// the statistics pass and the output pass.  A row is only D * 2 bytes per operand (40 of 64 lanes at D = 320),
// so one row per wave leaves the kernel bound by the load -> reduce -> store latency chain; RPI rows in flight
// per wave (4 / 2 / 1 at NV = 1 / 2 / 3, ~96 data registers each way) is what fills the memory pipeline.
// A row past the end is clamped for its loads, contributes nothing and is not stored.
template <typename T, bool WG, int NV, int RPI>
__global__ __launch_bounds__(256) void ln_bwd_kernel(const T* __restrict__ x, long ldx, const T* __restrict__ dy,
                                                     long lddy, const T* __restrict__ accum, long ldacc,
                                                     T* __restrict__ dx, long lddx, int M, int D,
                                                     const float* __restrict__ gamma,
                                                     const float* __restrict__ stats,
                                                     float* __restrict__ dgamma, float* __restrict__ dbeta,
                                                     float* __restrict__ partial) {
  // per-wave column sums (plain 16-byte LDS stores; LDS float atomics measured ~20 us per workgroup here)
  __shared__ __attribute__((aligned(16))) float red[WG ? 4 * 2 * NV * 512 : 4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int D8 = D / 8;
  float gsum[WG ? NV : 1][8], bsum[WG ? NV : 1][8];
  if (WG) {
#pragma unroll
    for (int k = 0; k < NV; ++k)
#pragma unroll
      for (int e = 0; e < 8; ++e) { gsum[k][e] = 0.f; bsum[k][e] = 0.f; }
  }
  float gam[NV][8];
#pragma unroll
  for (int k = 0; k < NV; ++k) {
    const int v = lane + 64 * k;
#pragma unroll
    for (int e = 0; e < 8; ++e) gam[k][e] = v < D8 ? gamma[v * 8 + e] : 0.f;
  }
  const long rstride = (long)gridDim.x * 4;
  for (long row0 = (long)blockIdx.x * 4 + wave; row0 < M; row0 += RPI * rstride) {
    long rows[RPI];
    bool ok[RPI];
    float mean[RPI], rstd[RPI], c1[RPI], c2[RPI];
    float f[RPI][NV][8], d[RPI][NV][8], o[RPI][NV][8];
#pragma unroll
    for (int r = 0; r < RPI; ++r) {
      rows[r] = row0 + r * rstride;
      ok[r] = rows[r] < M;
      if (!ok[r]) rows[r] = row0;
#pragma unroll
      for (int k = 0; k < NV; ++k) {
        const int v = lane + 64 * k;
        if (v < D8) {
          load8(x + rows[r] * ldx + v * 8, f[r][k]);
          load8(dy + rows[r] * lddy + v * 8, d[r][k]);
          if (accum) load8(accum + rows[r] * ldacc + v * 8, o[r][k]);
        }
      }
      mean[r] = stats[rows[r] * 2]; rstd[r] = stats[rows[r] * 2 + 1];
      c1[r] = 0.f; c2[r] = 0.f;
    }
#pragma unroll
    for (int r = 0; r < RPI; ++r) {
      const float live = ok[r] ? 1.f : 0.f;
#pragma unroll
      for (int k = 0; k < NV; ++k) {
        const int v = lane + 64 * k;
        if (v < D8) {
#pragma unroll
          for (int e = 0; e < 8; ++e) {
            const float xh = (f[r][k][e] - mean[r]) * rstd[r];
            const float de = d[r][k][e] * live;
            if (WG) { gsum[k][e] += de * xh; bsum[k][e] += de; }
            const float dh = de * gam[k][e];
            c1[r] += dh; c2[r] += dh * xh;
            f[r][k][e] = xh; d[r][k][e] = dh;
          }
        }
      }
    }
#pragma unroll
    for (int r = 0; r < RPI; ++r) { c1[r] = wave_sum(c1[r]) / D; c2[r] = wave_sum(c2[r]) / D; }
#pragma unroll
    for (int r = 0; r < RPI; ++r) {
      if (!ok[r]) continue;
#pragma unroll
      for (int k = 0; k < NV; ++k) {
        const int v = lane + 64 * k;
        if (v < D8) {
#pragma unroll
          for (int e = 0; e < 8; ++e) {
            const float g = rstd[r] * (d[r][k][e] - c1[r] - f[r][k][e] * c2[r]);
            o[r][k][e] = accum ? o[r][k][e] + g : g;
          }
          store8(dx + rows[r] * lddx + v * 8, o[r][k]);
        }
      }
    }
  }
  if (WG) {
    constexpr int WS = 2 * NV * 512;   // floats per wave: [dgamma NV*512 | dbeta NV*512]
#pragma unroll
    for (int k = 0; k < NV; ++k) {
      const int v = lane + 64 * k;
      if (v < D8) {
        float4* pg = reinterpret_cast<float4*>(&red[wave * WS + v * 8]);
        float4* pb = reinterpret_cast<float4*>(&red[wave * WS + NV * 512 + v * 8]);
        pg[0] = make_float4(gsum[k][0], gsum[k][1], gsum[k][2], gsum[k][3]);
        pg[1] = make_float4(gsum[k][4], gsum[k][5], gsum[k][6], gsum[k][7]);
        pb[0] = make_float4(bsum[k][0], bsum[k][1], bsum[k][2], bsum[k][3]);
        pb[1] = make_float4(bsum[k][4], bsum[k][5], bsum[k][6], bsum[k][7]);
      }
    }
    __syncthreads();
    float* dst = partial ? partial + (long)blockIdx.x * 2 * D : nullptr;
    for (int c = threadIdx.x; c < D; c += 256) {
      const float g = (red[c] + red[WS + c]) + (red[2 * WS + c] + red[3 * WS + c]);
      const float b = (red[NV * 512 + c] + red[WS + NV * 512 + c]) +
                      (red[2 * WS + NV * 512 + c] + red[3 * WS + NV * 512 + c]);
      if (dst) { dst[c] = g; dst[D + c] = b; }   // block partials [grid][2 D]; ln_bwd_finish_kernel adds them up
      else { atomicAdd(dgamma + c, g); atomicAdd(dbeta + c, b); }
    }
  }
}

// dgamma[c] += sum_blocks partial[blk][c] ; dbeta[c] += sum_blocks partial[blk][D + c]
// 32 columns x 32 block lanes per 1024-thread workgroup (few columns: the depth of each lane's loop is what counts)
__global__ __launch_bounds__(1024) void ln_bwd_finish_kernel(const float* __restrict__ partial, int nblk, int D,
                                                             float* __restrict__ dgamma, float* __restrict__ dbeta) {
  __shared__ float red[1024];
  const int cl = threadIdx.x & 31, kl = threadIdx.x >> 5;
  const int c = blockIdx.x * 32 + cl;   // column of the [2 D] partial row
  float s = 0.f;
  if (c < 2 * D)
#pragma unroll 8
    for (int k = kl; k < nblk; k += 32) s += partial[(long)k * 2 * D + c];
  red[threadIdx.x] = s;
  __syncthreads();
  if (kl == 0 && c < 2 * D) {
    float t = 0.f;
#pragma unroll
    for (int k = 0; k < 32; ++k) t += red[k * 32 + cl];
    if (c < D) dgamma[c] += t; else dbeta[c - D] += t;
  }
}

static int ln_grid(int M) {
  int g = (M + 3) / 4;
  return g < 2048 ? g : 2048;
}

int ln_fwd(const LnArgs& a, int dtype, hipStream_t st) {
  norm_rec_begin();
  if (a.D % 8 || a.D > 64 * LN_MAXV * 8 || a.ldx % 8 || a.ldy % 8) return CL_EINVAL;
  if (dtype == CL_BF16)
    hipLaunchKernelGGL((ln_fwd_kernel<bf16_t>), dim3(ln_grid(a.M)), dim3(256), 0, st, (const bf16_t*)a.x, a.ldx,
                       (bf16_t*)a.y, a.ldy, a.M, a.D, a.eps, a.gamma, a.beta, a.stats);
  else
    hipLaunchKernelGGL((ln_fwd_kernel<float>), dim3(ln_grid(a.M)), dim3(256), 0, st, (const float*)a.x, a.ldx,
                       (float*)a.y, a.ldy, a.M, a.D, a.eps, a.gamma, a.beta, a.stats);
  CL_CHECK_LAUNCH();
  g_norm_last = NormLaunchRec{NORM_LN_FWD, NORM_FORM_ONE, dtype == CL_BF16 ? CL_BF16 : CL_F32, (a.D / 8 + 63) / 64, 1, 256, a.D / 8, 0,
                              ln_grid(a.M), 1, 0, 1};
  return CL_OK;
}

int ln_bwd(const LnBwdArgs& a, int dtype, hipStream_t st) {
  norm_rec_begin();
  if (a.D % 8 || a.D > 64 * LN_MAXV * 8 || a.ldx % 8 || a.lddy % 8 || a.lddx % 8) return CL_EINVAL;
  if (a.accum && a.ldacc % 8) return CL_EINVAL;   // accum is read as 16-byte vectors like every other operand
  if ((a.dgamma == nullptr) != (a.dbeta == nullptr)) return CL_EINVAL;
  const int rpi = a.D <= 512 ? 4 : a.D <= 1024 ? 2 : 1;   // rows per wave iteration (see ln_bwd_kernel)
  int grid = (a.M + 4 * rpi - 1) / (4 * rpi);
  if (grid > 2048) grid = 2048;
  float* partial = nullptr;
  if (a.dgamma) {
    // column sums: block partials through the stream's registered scratch + a finishing kernel when there is
    // one (grid 1024); otherwise fp32 atomics with the grid bounded to 512 (same-address contention)
    void* wsp = nullptr; long wsb = 0;
    gemm_get_workspace_for(st, &wsp, &wsb);
    if (grid > 1024) grid = 1024;
    if (wsp && (long)grid * 2 * a.D * 4 <= wsb) partial = (float*)wsp;
    else if (grid > 512) grid = 512;
  }
#define LN_BWD_LAUNCH2(TT, WG, NV, RPI)                                                                         \
  hipLaunchKernelGGL((ln_bwd_kernel<TT, WG, NV, RPI>), dim3(grid), dim3(256), 0, st, (const TT*)a.x, a.ldx,     \
                     (const TT*)a.dy, a.lddy, (const TT*)a.accum, a.ldacc, (TT*)a.dx, a.lddx, a.M, a.D, a.gamma, \
                     a.stats, a.dgamma, a.dbeta, partial)
#define LN_BWD_LAUNCH(TT, WG)                                                                                   \
  do {                                                                                                          \
    if (a.D <= 512) LN_BWD_LAUNCH2(TT, WG, 1, 4);                                                               \
    else if (a.D <= 1024) LN_BWD_LAUNCH2(TT, WG, 2, 2);                                                         \
    else LN_BWD_LAUNCH2(TT, WG, 3, 1);                                                                          \
  } while (0)
  if (dtype == CL_BF16) { if (a.dgamma) LN_BWD_LAUNCH(bf16_t, true); else LN_BWD_LAUNCH(bf16_t, false); }
  else { if (a.dgamma) LN_BWD_LAUNCH(float, true); else LN_BWD_LAUNCH(float, false); }
#undef LN_BWD_LAUNCH2
#undef LN_BWD_LAUNCH
  if (partial)
    hipLaunchKernelGGL(ln_bwd_finish_kernel, dim3((2 * a.D + 31) / 32), dim3(1024), 0, st, partial, grid, a.D,
                       a.dgamma, a.dbeta);
  CL_CHECK_LAUNCH();
  g_norm_last = NormLaunchRec{NORM_LN_BWD, partial ? NORM_FORM_TWO : NORM_FORM_ONE, dtype == CL_BF16 ? CL_BF16 : CL_F32,
                              a.D <= 512 ? 1 : a.D <= 1024 ? 2 : 3, rpi, 256, a.D / 8, 0, grid, 1, a.dgamma ? (partial ? 1 : 2) : 0, 1};
  return CL_OK;
}

}  // namespace cl
