// HBM-bound elementwise / layout kernels of the CtrLoRA hot path (gfx950).
// All activations are token-major [rows, C] with an explicit row stride so they
// can address column slices of wider buffers (decoder concat, fused QKV).
#include "elementwise.h"
#include "gemm.h"

namespace cl {

static inline int ew_grid(long nvec, int threads = 256) {
  long g = (nvec + threads - 1) / threads;
  if (g < 1) g = 1;
  return (int)(g < 4096 ? g : 4096);
}

// ---------------------------------------------------------------- GEGLU (attention.py:49-56)
template <typename T>
__global__ void geglu_fwd_kernel(const T* __restrict__ h, long ldh, T* __restrict__ out, long ldo, long M, int F) {
  const int F8 = F / 8;
  const long n = M * F8;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    const long r = i / F8; const int v = (int)(i - r * F8);
    float a[8], g[8];
    load8(h + r * ldh + v * 8, a);
    load8(h + r * ldh + F + v * 8, g);
#pragma unroll
    for (int e = 0; e < 8; ++e) a[e] *= gelu_f(g[e]);
    store8(out + r * ldo + v * 8, a);
  }
}
template <typename T>
__global__ void geglu_bwd_kernel(const T* __restrict__ h, long ldh, const T* __restrict__ dout, long lddo,
                                 T* __restrict__ dh, long lddh, long M, int F) {
  const int F8 = F / 8;
  const long n = M * F8;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    const long r = i / F8; const int v = (int)(i - r * F8);
    float a[8], g[8], d[8], da[8], dg[8];
    load8(h + r * ldh + v * 8, a);
    load8(h + r * ldh + F + v * 8, g);
    load8(dout + r * lddo + v * 8, d);
#pragma unroll
    for (int e = 0; e < 8; ++e) { da[e] = d[e] * gelu_f(g[e]); dg[e] = d[e] * a[e] * dgelu_f(g[e]); }
    store8(dh + r * lddh + v * 8, da);
    store8(dh + r * lddh + F + v * 8, dg);
  }
}

// ---------------------------------------------------------------- SiLU on small [rows, C] (emb path)
template <typename T>
__global__ void silu_fwd_kernel(const T* __restrict__ x, T* __restrict__ y, long n8) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n8; i += (long)gridDim.x * blockDim.x) {
    float f[8]; load8(x + i * 8, f);
#pragma unroll
    for (int e = 0; e < 8; ++e) f[e] = silu_f(f[e]);
    store8(y + i * 8, f);
  }
}
template <typename T>
__global__ void silu_bwd_kernel(const T* __restrict__ x, const T* __restrict__ dy, T* __restrict__ dx, long n8) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n8; i += (long)gridDim.x * blockDim.x) {
    float f[8], d[8]; load8(x + i * 8, f); load8(dy + i * 8, d);
#pragma unroll
    for (int e = 0; e < 8; ++e) d[e] *= dsilu_f(f[e]);
    store8(dx + i * 8, d);
  }
}

// ---------------------------------------------------------------- y = a*x + b*y over [rows, C] with strides
template <typename T>
__global__ void axpby_kernel(const T* __restrict__ x, long ldx, T* __restrict__ y, long ldy, long M, int C,
                             float a, float b) {
  const int C8 = C / 8;
  const long n = M * C8;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    const long r = i / C8; const int v = (int)(i - r * C8);
    float f[8], g[8];
    load8(x + r * ldx + v * 8, f);
    if (b != 0.f) {
      load8(y + r * ldy + v * 8, g);
#pragma unroll
      for (int e = 0; e < 8; ++e) f[e] = a * f[e] + b * g[e];
    } else {
#pragma unroll
      for (int e = 0; e < 8; ++e) f[e] = a * f[e];
    }
    store8(y + r * ldy + v * 8, f);
  }
}

// ---------------------------------------------------------------- batched transpose with zero padding
// in [Bt][R][C] (row stride ldi, batch stride bsi) -> out [Bt][C][Rpad] (row stride ldo >= Rpad, batch stride bso)
template <typename U, typename T>
__global__ __launch_bounds__(256) void transpose_kernel(const U* __restrict__ in, long ldi, long bsi,
                                                        T* __restrict__ out, long ldo, long bso, int R, int C,
                                                        int Rpad) {
  __shared__ float tile[64][65];
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  const int r0 = blockIdx.x * 64, c0 = blockIdx.y * 64;
  const U* ib = in + (long)blockIdx.z * bsi;
  T* ob = out + (long)blockIdx.z * bso;
#pragma unroll 4
  for (int k = 0; k < 16; ++k) {
    const int r = r0 + ty + 4 * k, c = c0 + tx;
    tile[ty + 4 * k][tx] = (r < R && c < C) ? to_f<U>(ib[(long)r * ldi + c]) : 0.f;
  }
  __syncthreads();
#pragma unroll 4
  for (int k = 0; k < 16; ++k) {
    const int c = c0 + ty + 4 * k, r = r0 + tx;
    if (c < C && r < Rpad) ob[(long)c * ldo + r] = from_f<T>(tile[tx][ty + 4 * k]);
  }
}

// ---------------------------------------------------------------- NCHW fp32 <-> token-major T
// in [B, Cin, HW] fp32 -> out [B*HW, ldo] T, channels [Cin, Cpad) zero filled
template <typename T>
__global__ __launch_bounds__(256) void nchw_to_tok_kernel(const float* __restrict__ in, T* __restrict__ out,
                                                          long ldo, int Cin, int Cpad, int HW) {
  __shared__ float tile[64][65];
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  const int p0 = blockIdx.x * 64, c0 = blockIdx.y * 64, b = blockIdx.z;
#pragma unroll 4
  for (int k = 0; k < 16; ++k) {
    const int c = c0 + ty + 4 * k, p = p0 + tx;
    tile[ty + 4 * k][tx] = (c < Cin && p < HW) ? in[((long)b * Cin + c) * HW + p] : 0.f;
  }
  __syncthreads();
#pragma unroll 4
  for (int k = 0; k < 16; ++k) {
    const int p = p0 + ty + 4 * k, c = c0 + tx;
    if (p < HW && c < Cpad) out[((long)b * HW + p) * ldo + c] = from_f<T>(tile[tx][ty + 4 * k]);
  }
}
// in [B*HW, ldi] T -> out [B, C, HW] fp32  (out = alpha*in + beta*out)
template <typename T>
__global__ __launch_bounds__(256) void tok_to_nchw_kernel(const T* __restrict__ in, long ldi,
                                                          float* __restrict__ out, int C, int HW, float alpha,
                                                          float beta) {
  __shared__ float tile[64][65];
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  const int p0 = blockIdx.x * 64, c0 = blockIdx.y * 64, b = blockIdx.z;
#pragma unroll 4
  for (int k = 0; k < 16; ++k) {
    const int p = p0 + ty + 4 * k, c = c0 + tx;
    tile[ty + 4 * k][tx] = (p < HW && c < C) ? to_f<T>(in[((long)b * HW + p) * ldi + c]) : 0.f;
  }
  __syncthreads();
#pragma unroll 4
  for (int k = 0; k < 16; ++k) {
    const int c = c0 + ty + 4 * k, p = p0 + tx;
    if (c < C && p < HW) {
      float* o = out + ((long)b * C + c) * HW + p;
      const float v = alpha * tile[tx][ty + 4 * k];
      *o = beta != 0.f ? v + beta * *o : v;
    }
  }
}

// ---------------------------------------------------------------- timestep embedding (util.py:154-174)
// out[b, i] = cos(t_b * f_i), out[b, half + i] = sin(t_b * f_i); freqs is the fp32 table the host
// builds exactly as the reference does (exp(-ln(1e4) * arange(half) / half)).
template <typename T>
__global__ void timestep_embed_kernel(const long* __restrict__ t, const float* __restrict__ freqs,
                                      T* __restrict__ out, long ldo, int B, int half) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= B * half) return;
  const int b = i / half, k = i - b * half;
  const float arg = (float)t[b] * freqs[k];
  out[(long)b * ldo + k] = from_f<T>(cosf(arg));
  out[(long)b * ldo + half + k] = from_f<T>(sinf(arg));
}

// timestep_embedding at a FLOATING-POINT time (the DPM-Solver++ time grid is not integer: 949.05, 899.1, ...): the
// argument is t[b] * freqs[k] in fp32, so an integer-valued t gives the bits of timestep_embed_kernel
template <typename T>
__global__ void timestep_embed_f_kernel(const float* __restrict__ t, const float* __restrict__ freqs,
                                        T* __restrict__ out, long ldo, int B, int half) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= B * half) return;
  const int b = i / half, k = i - b * half;
  const float arg = t[b] * freqs[k];
  out[(long)b * ldo + k] = from_f<T>(cosf(arg));
  out[(long)b * ldo + half + k] = from_f<T>(sinf(arg));
}

// ---------------------------------------------------------------- q_sample + MSE (ddpm.py:356-359,902)
// x_noisy = sqrt_ac[t_b] * z + sqrt_1mac[t_b] * noise       (fp32, any layout; per = elems per sample)
__global__ void qsample_kernel(const float* __restrict__ z, const float* __restrict__ noise,
                               const long* __restrict__ t, const float* __restrict__ sqrt_ac,
                               const float* __restrict__ sqrt_1mac, float* __restrict__ out, long per, long n) {
  // two rounded products and a rounded sum, as torch evaluates a * z + b * noise: with the default contraction the sum
  // becomes an FMA and differs from the reference's x_noisy / stochastic_encode in the last bit of some elements
#pragma clang fp contract(off)
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    const long tb = t[i / per];
    const float a = sqrt_ac[tb] * z[i], b = sqrt_1mac[tb] * noise[i];
    out[i] = a + b;
  }
}
// ---------------------------------------------------------------- q_sample + mask blend (cldm/ddim_hacked.py:154-157)
// out = (sqrt_ac[t_b] * x0 + sqrt_1mac[t_b] * noise) * m + (1 - m) * x, m = mask[(per_b ? b : 0), (per_c ? c : 0), p]: the known
// region of a masked sampling step re-noised to this step's time, the rest kept.  x0 / noise / x / out = [B][C][HW] fp32, t_b
// clamped to [0, T - 1].  out may alias x (element-wise: every work item reads its own elements before it writes them), so
// neither is __restrict__.  W = elements per work item (4: 16-byte loads and stores, 1: scalar); nw = B C HW / W work items.
template <int W>
__global__ void qsample_blend_kernel(const float* __restrict__ x0, const float* __restrict__ noise, const long* __restrict__ t,
                                     const float* __restrict__ sqrt_ac, const float* __restrict__ sqrt_1mac, int T,
                                     const float* __restrict__ mask, int per_b, int per_c, const float* x, float* out,
                                     int C, long HW, long nw) {
  // every torch op of q_sample(x0, t) * mask + (1. - mask) * img rounded once: two products and a sum (qsample_kernel), then a
  // product, a difference, a product and a sum.  A contracted sum would differ from the eager loop in the last bit of some elements
#pragma clang fp contract(off)
  const long hw = HW / W;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < nw; i += (long)gridDim.x * blockDim.x) {
    const long bc = i / hw, j = (i - bc * hw) * W;
    const long b = bc / C, c = bc - b * C;
    long tb = t[b];
    tb = tb < 0 ? 0 : (tb >= T ? T - 1 : tb);
    const float sa = sqrt_ac[tb], s1 = sqrt_1mac[tb];
    const long mrow = (per_b ? b : 0) * (per_c ? C : 1) + (per_c ? c : 0);
    const long e = bc * HW + j, me = mrow * HW + j;
    if constexpr (W == 4) {
      const float4 z = *reinterpret_cast<const float4*>(x0 + e), n = *reinterpret_cast<const float4*>(noise + e);
      const float4 m = *reinterpret_cast<const float4*>(mask + me), v = *reinterpret_cast<const float4*>(x + e);
      float4 a, p, q, k, o;
      a.x = sa * z.x; a.y = sa * z.y; a.z = sa * z.z; a.w = sa * z.w;
      p.x = s1 * n.x; p.y = s1 * n.y; p.z = s1 * n.z; p.w = s1 * n.w;
      q.x = a.x + p.x; q.y = a.y + p.y; q.z = a.z + p.z; q.w = a.w + p.w;
      q.x = q.x * m.x; q.y = q.y * m.y; q.z = q.z * m.z; q.w = q.w * m.w;
      k.x = 1.0f - m.x; k.y = 1.0f - m.y; k.z = 1.0f - m.z; k.w = 1.0f - m.w;
      k.x = k.x * v.x; k.y = k.y * v.y; k.z = k.z * v.z; k.w = k.w * v.w;
      o.x = q.x + k.x; o.y = q.y + k.y; o.z = q.z + k.z; o.w = q.w + k.w;
      *reinterpret_cast<float4*>(out + e) = o;
    } else {
      const float a = sa * x0[e], p = s1 * noise[e];
      const float q = a + p;
      const float m = mask[me];
      const float qm = q * m, k = 1.0f - m;
      const float kx = k * x[e];
      out[e] = qm + kx;
    }
  }
}
// ---------------------------------------------------------------- posterior sample (ddpm.py:655-662, distributions.py:35-37)
// out = scale * (mean + std * e) for one or two tensors in ONE launch: mom = [B][2 per] (mean | std), e / out = [B][per], fp32.
// work items [0, nw) belong to tensor a, [nw, 2 nw) to tensor b; W = elements per work item (4: 16-byte loads and stores, 1: scalar)
template <int W>
__global__ void posterior_sample_pair_kernel(const float* __restrict__ mom_a, const float* __restrict__ e_a, float* __restrict__ out_a,
                                             const float* __restrict__ mom_b, const float* __restrict__ e_b, float* __restrict__ out_b,
                                             long per, long nw, int ntensors, float scale) {
  // a rounded product, a rounded sum, a rounded product, as torch evaluates scale_factor * (mean + std * randn): a contracted
  // std * e + mean is an FMA and differs from DiagonalGaussianDistribution.sample in the last bit of some elements
#pragma clang fp contract(off)
  const long perw = per / W, total = nw * ntensors;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const bool second = i >= nw;
    const long w = second ? i - nw : i;
    const float* mom = second ? mom_b : mom_a;
    const float* e = second ? e_b : e_a;
    float* out = second ? out_b : out_a;
    const long b = w / perw, j = (w - b * perw) * W;
    const float* mean = mom + b * 2 * per + j;
    if constexpr (W == 4) {
      const float4 m = *reinterpret_cast<const float4*>(mean), s = *reinterpret_cast<const float4*>(mean + per);
      const float4 n = *reinterpret_cast<const float4*>(e + w * 4);
      float4 p, z, o;
      p.x = s.x * n.x; p.y = s.y * n.y; p.z = s.z * n.z; p.w = s.w * n.w;
      z.x = m.x + p.x; z.y = m.y + p.y; z.z = m.z + p.z; z.w = m.w + p.w;
      o.x = scale * z.x; o.y = scale * z.y; o.z = scale * z.z; o.w = scale * z.w;
      *reinterpret_cast<float4*>(out + w * 4) = o;
    } else {
      const float p = mean[per] * e[w];
      const float z = mean[0] + p;
      out[w] = scale * z;
    }
  }
}
// loss += sum((eps - target)^2) / n ; d_eps = 2 (eps - target) / n * gscale
__global__ __launch_bounds__(256) void mse_kernel(const float* __restrict__ eps, const float* __restrict__ target,
                                                  float* __restrict__ d_eps, float* __restrict__ loss, long n,
                                                  float gscale) {
  __shared__ float red[4];
  float acc = 0.f;
  const float inv = 1.0f / (float)n;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    const float d = eps[i] - target[i];
    acc += d * d;
    if (d_eps) d_eps[i] = 2.0f * d * inv * gscale;
  }
  acc = wave_sum(acc);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) atomicAdd(loss, (red[0] + red[1] + red[2] + red[3]) * inv);
}

// ---------------------------------------------------------------- 3x3-conv tap gather (fp32 parity mode of the conv dW)
// out[m, :] = x[pixel(m, tap), :] or 0 outside the image, m = (b, oy, ox): the shifted operand of one tap of a conv
// weight gradient.  The bf16 path does this inside wgrad_tn_kernel's DMA addressing; the fp32 parity mode, whose
// weight-gradient kernel wants explicit transposes anyway, materialises it.
template <typename T>
__global__ void conv_tap_gather_kernel(const T* __restrict__ x, long ldx, T* __restrict__ out, long ldo, int Hin, int Win,
                                       int Hout, int Wout, int C8, int tap, int stride, int pad, long total) {
  const int ky = tap / 3, kx = tap - 3 * ky;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const long m = i / C8; const int c = (int)(i - m * C8) * 8;
    const int ox = (int)(m % Wout); const long t2 = m / Wout; const int oy = (int)(t2 % Hout); const long ob = t2 / Hout;
    const int iy = oy * stride + ky - pad, ix = ox * stride + kx - pad;
    float f[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if ((unsigned)iy < (unsigned)Hin && (unsigned)ix < (unsigned)Win) load8(x + ((ob * Hin + iy) * Win + ix) * ldx + c, f);
    store8(out + m * ldo + c, f);
  }
}

// ---------------------------------------------------------------- row softmax (VAE mid-block attention)
// one workgroup per row; N <= 256 * 32: the row lives in registers (16-byte loads), fp32 math, exp2 with the
// scale folded in
template <typename T>
__global__ __launch_bounds__(256) void softmax_rows_kernel(const float* __restrict__ S, long lds_, T* __restrict__ P,
                                                           long ldp, int N, float scale) {
  __shared__ float red[8];
  const float* s = S + (long)blockIdx.x * lds_;
  T* o = P + (long)blockIdx.x * ldp;
  constexpr int MAXV = 8;                       // 8 x float4 per thread = 8192 columns
  float4 v[MAXV];
  const float sl2 = scale * 1.4426950408889634f;
  float mx = -INFINITY;
#pragma unroll
  for (int i = 0; i < MAXV; ++i) {
    const int c = (i * 256 + threadIdx.x) * 4;
    if (c < N) {
      v[i] = *reinterpret_cast<const float4*>(s + c);
      mx = fmaxf(mx, fmaxf(fmaxf(v[i].x, v[i].y), fmaxf(v[i].z, v[i].w)));
    }
  }
  mx = wave_max(mx);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = mx;
  __syncthreads();
  mx = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3])) * sl2;
  float sum = 0.f;
#pragma unroll
  for (int i = 0; i < MAXV; ++i) {
    const int c = (i * 256 + threadIdx.x) * 4;
    if (c < N) {
      v[i].x = __builtin_amdgcn_exp2f(v[i].x * sl2 - mx); v[i].y = __builtin_amdgcn_exp2f(v[i].y * sl2 - mx);
      v[i].z = __builtin_amdgcn_exp2f(v[i].z * sl2 - mx); v[i].w = __builtin_amdgcn_exp2f(v[i].w * sl2 - mx);
      sum += (v[i].x + v[i].y) + (v[i].z + v[i].w);
    }
  }
  sum = wave_sum(sum);
  if ((threadIdx.x & 63) == 0) red[4 + (threadIdx.x >> 6)] = sum;
  __syncthreads();
  const float inv = 1.0f / ((red[4] + red[5]) + (red[6] + red[7]));
#pragma unroll
  for (int i = 0; i < MAXV; ++i) {
    const int c = (i * 256 + threadIdx.x) * 4;
    if (c < N) {
      const float w[4] = {v[i].x * inv, v[i].y * inv, v[i].z * inv, v[i].w * inv};
      store4(o + c, w);
    }
  }
}

// ---------------------------------------------------------------- p_losses reduction (ddpm.py:902-918)
// Deterministic (no float atomics): block (chunk, b) reduces one slice of sample b into scratch[b][chunk] and writes d_eps; the
// finishing block sums the slices in a fixed order.  One kernel pair serves cl_p_losses_mse (l2, no table) and cl_p_losses_w (a
// per-timestep weight table `wt`, NULL = weight 1, and a choice of rho):
//   KIND 0 (l2)     rho(d) = d^2,                                                   rho'(d) = 2 d   (the 2 is in gmul)
//   KIND 1 (Huber)  rho(d) = |d| <= delta ? d^2 / 2 : delta (|d| - delta / 2),      rho'(d) = clamp(d, -delta, delta)
//   l_b = mean rho(d) of sample b (unweighted: scratch, per_sample, out[0], out[1]);  d_eps = rho'(d) * gmul * wt[t_b]
//   out[0] = loss_simple = mean_b l_b                              (logvar == 0)
//   out[1] = loss_vlb    = mean_b lvlb[t_b] * l_b
//   out[2] = loss        = w_simple * mean_b (wt[t_b] l_b) + w_elbo * out[1]
// t and wt are read on the device, once per workgroup: a captured launch follows both.
constexpr int PL_CHUNKS = 16;
template <int KIND>
__global__ __launch_bounds__(256) void plosses_w_partial_kernel(const float* __restrict__ eps,
                                                                const float* __restrict__ target,
                                                                float* __restrict__ d_eps, float* __restrict__ scratch,
                                                                const long* __restrict__ t, const float* __restrict__ wt,
                                                                long per, float gmul, float delta) {
  __shared__ float red[4];
  const int b = blockIdx.y, chunk = blockIdx.x;
  const long base = (long)b * per;
  const long c0 = per * chunk / PL_CHUNKS, c1 = per * (chunk + 1) / PL_CHUNKS;
  const float g = wt ? gmul * wt[t[b]] : gmul;
  float acc = 0.f;
  for (long i = c0 + threadIdx.x; i < c1; i += 256) {
    const float d = eps[base + i] - target[base + i];
    if (KIND == 0) {
      acc += d * d;
      if (d_eps) d_eps[base + i] = d * g;
    } else {
      const float a = fabsf(d);
      acc += a <= delta ? 0.5f * d * d : delta * (a - 0.5f * delta);
      if (d_eps) d_eps[base + i] = fminf(fmaxf(d, -delta), delta) * g;
    }
  }
  acc = wave_sum(acc);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) scratch[b * PL_CHUNKS + chunk] = (red[0] + red[1]) + (red[2] + red[3]);
}
__global__ __launch_bounds__(64) void plosses_w_finish_kernel(const float* __restrict__ scratch, const long* __restrict__ t,
                                                              const float* __restrict__ lvlb, const float* __restrict__ wt,
                                                              float* __restrict__ out, float* __restrict__ per_sample, int B,
                                                              long per, float w_simple, float w_elbo) {
  if (threadIdx.x != 0) return;
  float ls = 0.f, lv = 0.f, lw = 0.f;
  for (int b = 0; b < B; ++b) {
    float s = 0.f;
    for (int c = 0; c < PL_CHUNKS; ++c) s += scratch[b * PL_CHUNKS + c];
    s /= (float)per;
    if (per_sample) per_sample[b] = s;
    ls += s;
    if (lvlb) lv += lvlb[t[b]] * s;
    if (wt) lw += wt[t[b]] * s;
  }
  ls /= (float)B; lv /= (float)B; lw /= (float)B;
  if (!wt) lw = ls;               // weight 1: the weighted mean is the plain one, summed once
  out[0] = ls; out[1] = lv; out[2] = w_simple * lw + w_elbo * lv;
}

// ---------------------------------------------------------------- per-sample losses by timestep band (not in the reference)
// acc = double [nbands + 1][3] = {count, sum, sum of squares} per band, row nbands = all samples; the launch ADDS to it.
//   band(t) = min(clamp(t, 0, T - 1) * nbands / T, nbands - 1)   (64-bit integers)
// One workgroup: the samples are staged LB_CHUNK at a time in LDS (their band and their loss), then thread r < nbands walks
// the chunk in index order for row r and thread nbands for the total row, each in fp64 registers -- no atomics, one writer per
// row, the bits of the sequential loop.  A non-finite loss reaches its own band and the total only.  *n_valid (optional) is
// read on the device, so a captured launch follows it.
constexpr int LB_CHUNK = 1024, LB_THREADS = 128;
__global__ __launch_bounds__(LB_THREADS) void loss_bands_kernel(const float* __restrict__ per_sample, const long* __restrict__ t,
                                                                int B, int T, int nbands, const int* __restrict__ n_valid,
                                                                double* __restrict__ acc) {
  __shared__ float loss_s[LB_CHUNK];
  __shared__ unsigned char band_s[LB_CHUNK];
  int nv = B;
  if (n_valid) { nv = *n_valid; nv = nv < 0 ? 0 : nv > B ? B : nv; }
  const int row = threadIdx.x;
  const bool owner = row <= nbands;
  double cnt = 0.0, s1 = 0.0, s2 = 0.0;
  if (owner) { cnt = acc[row * 3 + 0]; s1 = acc[row * 3 + 1]; s2 = acc[row * 3 + 2]; }
  for (int c0 = 0; c0 < nv; c0 += LB_CHUNK) {
    const int n = nv - c0 < LB_CHUNK ? nv - c0 : LB_CHUNK;
    for (int i = threadIdx.x; i < n; i += LB_THREADS) {
      long tt = t[c0 + i];
      tt = tt < 0 ? 0 : tt > T - 1 ? T - 1 : tt;
      const long k = tt * nbands / T;
      band_s[i] = (unsigned char)(k < nbands - 1 ? k : nbands - 1);
      loss_s[i] = per_sample[c0 + i];
    }
    __syncthreads();
    if (owner) {
      for (int i = 0; i < n; ++i) {
        if (row == nbands || band_s[i] == row) {
          const double x = (double)loss_s[i];
          cnt += 1.0; s1 += x; s2 += x * x;
        }
      }
    }
    __syncthreads();
  }
  if (owner) { acc[row * 3 + 0] = cnt; acc[row * 3 + 1] = s1; acc[row * 3 + 2] = s2; }
}

// ---------------------------------------------------------------- DDIM update (ddim_hacked.py:192,203-231)
// coef = device table [S][4] = {a_t, a_prev, sigma_t, sqrt(1 - a_t)} (fp32), row `index` is used.  x_prev may alias x
// (element-wise), so neither is __restrict__.  One body for the host-index and the device-cursor launch (below): an eager
// and a replayed step give the same bits.
__device__ __forceinline__ void ddim_step_body(const float* x, const float* __restrict__ e_c,
                                               const float* __restrict__ e_u, const float* __restrict__ noise,
                                               const float* __restrict__ coef, int index, float scale, float* x_prev,
                                               float* __restrict__ pred_x0, long n) {
  const float a_t = coef[index * 4 + 0], a_prev = coef[index * 4 + 1];
  const float sigma = coef[index * 4 + 2], s1m = coef[index * 4 + 3];
  const float sqrt_at = sqrtf(a_t), sqrt_ap = sqrtf(a_prev), dir = sqrtf(1.0f - a_prev - sigma * sigma);
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    float e = e_c[i];
    if (e_u) { const float u = e_u[i]; e = u + scale * (e - u); }
    const float p0 = (x[i] - s1m * e) / sqrt_at;
    float xp = sqrt_ap * p0 + dir * e;
    if (noise) xp += sigma * noise[i];
    x_prev[i] = xp;
    if (pred_x0) pred_x0[i] = p0;
  }
}
__global__ void ddim_step_kernel(const float* x, const float* __restrict__ e_c, const float* __restrict__ e_u,
                                 const float* __restrict__ noise, const float* __restrict__ coef, int index, float scale,
                                 float* x_prev, float* __restrict__ pred_x0, long n) {
  ddim_step_body(x, e_c, e_u, noise, coef, index, scale, x_prev, pred_x0, n);
}

// ---------------------------------------------------------------- fused AdamW over one flat fp32 buffer
// torch.optim.AdamW defaults (cldm_ctrlora_finetune.py:105): decoupled decay, bias correction.  The update is written once:
// adam_group() derives a step's scalars from {lr, beta1, beta2, eps, weight_decay, grad_scale} and the step count, adam_elem()
// updates one element, and every AdamW entry point runs its elements through them.  Contraction is off in both and the two
// operations that are fused are written as fmaf, so the bits are stated here and not left to the compiler's heuristics --
//     1 - lr wd           = fma(-lr, wd, 1)
//     m' = b1 m + (1 - b1) gi = fma(1 - b1, gi, b1 m)
//     v' = b2 v + ((1 - b2) gi) gi,  p' = (1 - lr wd) p - ((lr / bc1) m') / (sqrt(v') / bc2_sqrt + eps):  every operation rounded
// (tests/golden/step_bits.pt holds every entry point to the bits it had when each kernel carried its own copy of the expression).
struct AdamGroup { float decay, beta1, omb1, beta2, omb2, bc2_sqrt, eps, lr_bc1, gscale; };
__host__ __device__ inline AdamGroup adam_group(float lr, float beta1, float beta2, float eps, float wd, float gscale, float st) {
#pragma clang fp contract(off)
  const float bc1 = 1.0f - powf(beta1, st), bc2_sqrt = sqrtf(1.0f - powf(beta2, st));
  return AdamGroup{__builtin_fmaf(-lr, wd, 1.0f), beta1, 1.0f - beta1, beta2, 1.0f - beta2, bc2_sqrt, eps, lr / bc1, gscale};
}
__device__ __forceinline__ void adam_elem(const AdamGroup& h, float& pi, float g, float& mi, float& vi) {
#pragma clang fp contract(off)
  const float gi = g * h.gscale;
  const float pd = pi * h.decay;
  mi = __builtin_fmaf(h.omb1, gi, h.beta1 * mi);
  vi = h.beta2 * vi + h.omb2 * gi * gi;
  const float denom = sqrtf(vi) / h.bc2_sqrt + h.eps;
  pi = pd - h.lr_bc1 * mi / denom;
}
// cl_adamw: the scalars by value, the bias corrections formed on the host (the launcher builds `h`)
__global__ void adamw_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                             float* __restrict__ v, long n, const AdamGroup h) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    float pi = p[i], mi = m[i], vi = v[i];
    adam_elem(h, pi, g[i], mi, vi);
    p[i] = pi; m[i] = mi; v[i] = vi;
  }
}

// ---------------------------------------------------------------- device-resident step state (hipGraph replay)
// A captured graph replays the SAME kernel arguments, so anything that changes from step to step must
// live in device memory: the optimizer step count / hyper-parameters and the DDIM loop cursor.
__global__ void tick_kernel(int* c) { *c += 1; }

// ---------------------------------------------------------------- global gradient norm + clip coefficient
// torch.nn.utils.clip_grad_norm_ (norm_type 2, error_if_nonfinite=False) over up to GN_MAX_BUFS flat fp32 buffers, in two
// launches and no atomics (the plosses pattern above): workgroup w strides over every buffer in turn and leaves ONE fp64 partial
// in scratch[w]; the finishing workgroup adds the partials in index order.  The squares are formed and summed in fp64 from the
// first product on: g^2 neither overflows nor underflows, and the rounding of the sum stays far below one fp32 ulp for any n the
// engine can hold, so the result does not depend on how the elements were split over threads beyond that.  The order is fixed by
// the launch geometry alone: a replay gives the same bits.  The kernel is bound by its 4 B / element read.
//   out[0] = hyper[5] * sqrt(sum g^2)      (grad_scale: the norm of the gradient AdamW applies)
//   out[1] = coef = max_norm <= 0 ? 1 : clamp(max_norm / (out[0] + 1e-6), max = 1), NaN kept as torch.clamp keeps it
// A buffer is read with 16-byte loads from its first 16-byte boundary on; the elements before it (head) and the last n % 4 after
// the vectors (tail) are read one by one by the first threads of the grid, as zero_kernel does.
constexpr int GN_MAX_BUFS = 16;
constexpr int GN_MAX_GROUPS = 512;     // workgroups of the partial launch = fp64 partials the finishing workgroup adds
struct GradNormBufs {
  const float* p[GN_MAX_BUFS];
  long n[GN_MAX_BUFS];
};
__device__ __forceinline__ double gn_sq4(const float4 a) {
  return ((double)a.x * (double)a.x + (double)a.y * (double)a.y) + ((double)a.z * (double)a.z + (double)a.w * (double)a.w);
}
__global__ __launch_bounds__(256) void grad_norm_partial_kernel(const GradNormBufs bufs, int nbuf, double* __restrict__ scratch) {
  __shared__ double red[4];
  const long gid = (long)blockIdx.x * 256 + threadIdx.x, stride = (long)gridDim.x * 256;
  double acc = 0.0;
  for (int b = 0; b < nbuf; ++b) {
    const float* __restrict__ p = bufs.p[b];
    const long n = bufs.n[b];
    long head = (long)(((16 - (reinterpret_cast<uintptr_t>(p) & 15)) & 15) >> 2);
    if (head > n) head = n;
    const long nvec = (n - head) >> 2, tail = n - head - (nvec << 2);
    const float4* __restrict__ body = reinterpret_cast<const float4*>(p + head);
    long i = gid;
    for (; i + 3 * stride < nvec; i += 4 * stride) {     // four independent 16-byte loads in flight per thread
      const float4 a0 = body[i], a1 = body[i + stride], a2 = body[i + 2 * stride], a3 = body[i + 3 * stride];
      acc += (gn_sq4(a0) + gn_sq4(a1)) + (gn_sq4(a2) + gn_sq4(a3));
    }
    for (; i < nvec; i += stride) acc += gn_sq4(body[i]);
    if (gid < head) { const double g = (double)p[gid]; acc += g * g; }
    if (gid < tail) { const double g = (double)p[head + (nvec << 2) + gid]; acc += g * g; }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) scratch[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}
__global__ __launch_bounds__(256) void grad_norm_finish_kernel(const double* __restrict__ scratch, int groups,
                                                               const float* __restrict__ hyper,
                                                               const float* __restrict__ max_norm, float* __restrict__ out) {
  __shared__ double part[GN_MAX_GROUPS];
  for (int i = threadIdx.x; i < groups; i += 256) part[i] = scratch[i];
  __syncthreads();
  if (threadIdx.x != 0) return;
  double s = 0.0;
  for (int i = 0; i < groups; ++i) s += part[i];
  const float norm = (float)((double)hyper[5] * sqrt(s));
  float coef = 1.0f;
  const float mx = max_norm ? *max_norm : 0.0f;
  if (!(mx <= 0.0f)) {
    const float c = mx / (norm + 1e-6f);
    coef = c < 1.0f ? c : (c != c ? c : 1.0f);
  }
  out[0] = norm; out[1] = coef;
}

// ---------------------------------------------------------------- AdamW from device-resident state, with parameter groups
// One kernel behind cl_adamw_dev, cl_adamw_dev_clip and cl_adamw_dev_groups.  table = [ngroups][6] rows of {lr, beta1, beta2, eps,
// weight_decay, grad_scale} (a one-group launch passes its `hyper` as a table of one row), *step was already incremented for this
// step, clip = grad_norm_finish_kernel's out or NULL: gi = g[i] * (grad_scale * coef), the two scalars multiplied FIRST, so a
// coefficient of 1.0f gives the bits of no clipping.  chunk_group[c] = the group of elements [64 c, 64 c + 64), or NULL: every
// chunk is group 0.  The flat buffers align every tensor to 64 floats (packing.TrainableSet.materialize), so a chunk never holds
// two tensors.  A wave owns one chunk per trip: its 64 lanes read and write one whole 256-byte line of each of the four streams
// (lane = consecutive float; with 256 threads that is element blockIdx * 256 + tid and a stride of gridDim * 256, a grid-stride
// loop over elements), and the group is ONE byte load per wave and trip (all lanes read the same address, made wave-uniform with
// readfirstlane) -- 1 / 64 byte per element next to the 28 the streams move.  The first `ngroups` threads of a workgroup derive
// their group's scalars once and leave them in LDS.  An entry >= ngroups is clamped to the last group: nothing is read beyond the
// table.  The last chunk may be ragged (n % 64 != 0, one-group launches only): lanes at or beyond n do nothing.
constexpr int AG_MAX_GROUPS = 8;
__global__ __launch_bounds__(256) void adamw_dev_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                        float* __restrict__ m, float* __restrict__ v, long n,
                                                        const float* __restrict__ table, int ngroups,
                                                        const unsigned char* __restrict__ chunk_group,
                                                        const int* __restrict__ step, const float* __restrict__ clip) {
  __shared__ AdamGroup hp[AG_MAX_GROUPS];
  if ((int)threadIdx.x < ngroups) {
    const float* __restrict__ h = table + 6 * threadIdx.x;
    hp[threadIdx.x] = adam_group(h[0], h[1], h[2], h[3], h[4], clip ? h[5] * clip[1] : h[5], (float)*step);
  }
  __syncthreads();
  const int lane = threadIdx.x & 63;
  const long wave = (long)blockIdx.x * 4 + (threadIdx.x >> 6), nwaves = (long)gridDim.x * 4;
  for (long c = wave; (c << 6) < n; c += nwaves) {
    int grp = 0;
    if (chunk_group) {
      grp = __builtin_amdgcn_readfirstlane((int)chunk_group[c]);
      grp = grp < ngroups ? grp : ngroups - 1;
    }
    const AdamGroup h = hp[grp];
    const long i = (c << 6) + lane;
    if (i < n) {
      float pi = p[i], mi = m[i], vi = v[i];
      adam_elem(h, pi, g[i], mi, vi);
      p[i] = pi; m[i] = mi; v[i] = vi;
    }
  }
}

// table[gidx][0] = lr_table[min(*step - 1, T - 1)][gidx]: the learning rate of optimizer step *step (counted from 1, already
// advanced by tick_kernel) from a device [T][ngroups] table -- LambdaLR's indexing, the last row holds past the end.
__global__ void lr_schedule_kernel(float* __restrict__ table, int ngroups, const float* __restrict__ lr_table, int T,
                                   const int* __restrict__ step) {
  const int gidx = threadIdx.x;
  if (gidx >= ngroups) return;
  int row = *step - 1;
  row = row < 0 ? 0 : (row < T - 1 ? row : T - 1);
  table[6 * gidx] = lr_table[(long)row * ngroups + gidx];
}

// ---------------------------------------------------------------- EMA of the trained weights (ldm/modules/ema.py: LitEma.forward)
// shadow -= (1 - d) * (shadow - p) over one flat fp32 buffer, d = min(*decay, (1 + u) / (10 + u)) with u = *num_updates already
// advanced by tick_kernel, or *decay itself for u < 0 (LitEma without the warm-up).  Decay and count are read from device memory:
// a replayed graph follows them.  Every fp32 operation is rounded once and none is contracted, so the bits are those of torch's
// s.sub_(omd * (s - p)) on the CPU; min() is Python's (the warm-up term wins only where it is smaller, a NaN decay stays).
// W = 4: shadow and p share their offset from a 16-byte boundary -- 16-byte accesses from that boundary on, the elements before
// it (head) and the last n % 4 (tail) one by one by the first threads of the grid, as zero_kernel does.  W = 1: plain grid stride.
__device__ __forceinline__ float ema_one_minus_decay(const float* __restrict__ decay, const int* __restrict__ num_updates) {
#pragma clang fp contract(off)
  const int u = *num_updates;
  float d = *decay;
  if (u >= 0) {
    const float w = (float)(1 + u) / (float)(10 + u);      // IEEE division: hipcc's default for fp32
    d = w < d ? w : d;
  }
  return 1.0f - d;
}
__device__ __forceinline__ float ema_elem(float s, float p, float omd) {
#pragma clang fp contract(off)
  const float diff = s - p;
  const float step = omd * diff;
  return s - step;
}
template <int W>
__global__ __launch_bounds__(256) void ema_update_kernel(float* __restrict__ shadow, const float* __restrict__ p, long head,
                                                         long nvec, long tail, const float* __restrict__ decay,
                                                         const int* __restrict__ num_updates) {
#pragma clang fp contract(off)
  const float omd = ema_one_minus_decay(decay, num_updates);
  const long i0 = (long)blockIdx.x * blockDim.x + threadIdx.x, stride = (long)gridDim.x * blockDim.x;
  if constexpr (W == 4) {
    float4* __restrict__ sb = reinterpret_cast<float4*>(shadow + head);
    const float4* __restrict__ pb = reinterpret_cast<const float4*>(p + head);
    for (long i = i0; i < nvec; i += stride) {
      float4 s = sb[i];
      const float4 q = pb[i];
      s.x = ema_elem(s.x, q.x, omd); s.y = ema_elem(s.y, q.y, omd); s.z = ema_elem(s.z, q.z, omd); s.w = ema_elem(s.w, q.w, omd);
      sb[i] = s;
    }
    if (i0 < head) shadow[i0] = ema_elem(shadow[i0], p[i0], omd);
    if (i0 < tail) { const long e = head + (nvec << 2) + i0; shadow[e] = ema_elem(shadow[e], p[e], omd); }
  } else {
    for (long i = i0; i < nvec; i += stride) shadow[i] = ema_elem(shadow[i], p[i], omd);
  }
}
// a <-> b over two disjoint fp32 buffers, the same two forms (ema_scope: shadow into the masters and back, no third copy)
template <int W>
__global__ __launch_bounds__(256) void swap_kernel(float* __restrict__ a, float* __restrict__ b, long head, long nvec, long tail) {
  const long i0 = (long)blockIdx.x * blockDim.x + threadIdx.x, stride = (long)gridDim.x * blockDim.x;
  if constexpr (W == 4) {
    float4* __restrict__ av = reinterpret_cast<float4*>(a + head);
    float4* __restrict__ bv = reinterpret_cast<float4*>(b + head);
    for (long i = i0; i < nvec; i += stride) { const float4 x = av[i], y = bv[i]; av[i] = y; bv[i] = x; }
    if (i0 < head) { const float x = a[i0]; a[i0] = b[i0]; b[i0] = x; }
    if (i0 < tail) { const long e = head + (nvec << 2) + i0; const float x = a[e]; a[e] = b[e]; b[e] = x; }
  } else {
    for (long i = i0; i < nvec; i += stride) { const float x = a[i]; a[i] = b[i]; b[i] = x; }
  }
}

// DDIM loop with a device cursor i = 0..S-1 (ddim_hacked.py:157-160): index = S-1-i, ts = ddim_timesteps[index]
__global__ void ddim_set_t_kernel(const long* __restrict__ table, const int* __restrict__ cursor, int S,
                                  long* __restrict__ ts, int n) {
  const int index = max(0, S - 1 - *cursor);
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) ts[i] = table[index];
}
__global__ void ddim_step_dev_kernel(const float* x, const float* __restrict__ e_c, const float* __restrict__ e_u,
                                     const float* __restrict__ noise, const float* __restrict__ coef,
                                     const int* __restrict__ cursor, int S, float scale, float* x_prev,
                                     float* __restrict__ pred_x0, long n) {
  ddim_step_body(x, e_c, e_u, noise, coef, max(0, S - 1 - *cursor), scale, x_prev, pred_x0, n);
}

// ---------------------------------------------------------------- DPM-Solver++ multistep update (data prediction)
// coef = device table [S][8] fp32, row i = {alpha_i, sigma_i, cx_i, c0_i, c1_i, c2_i, t_in_i, 0}; hist = [3][n] fp32 ring,
// model value k lives in slot k % 3.  Step i:  e = guided eps;  m = (x - sigma_i e) / alpha_i;  hist[i % 3] = m;
//   x_next = cx_i x + c0_i m + c1_i hist[(i + 2) % 3] + c2_i hist[(i + 1) % 3]
// A term whose coefficient is exactly 0 is not read (the start-up steps would read uninitialised slots).  x_next may
// alias x (element-wise), so neither is __restrict__.  One body for the host-index and the device-cursor launch: an
// eager and a replayed step give the same bits.
__device__ __forceinline__ void dpmpp_step_body(const float* x, const float* __restrict__ e_c,
                                                const float* __restrict__ e_u, const float* __restrict__ coef,
                                                int index, float scale, float* hist, float* x_next,
                                                float* __restrict__ pred_x0, long n) {
  const float* row = coef + (long)index * 8;
  const float alpha = row[0], sigma = row[1], cx = row[2], c0 = row[3], c1 = row[4], c2 = row[5];
  float* h0 = hist + (long)(index % 3) * n;
  const float* h1 = hist + (long)((index + 2) % 3) * n;
  const float* h2 = hist + (long)((index + 1) % 3) * n;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    float e = e_c[i];
    if (e_u) { const float u = e_u[i]; e = u + scale * (e - u); }
    const float xi = x[i];
    const float m = (xi - sigma * e) / alpha;
    float xn = cx * xi + c0 * m;
    if (c1 != 0.0f) xn += c1 * h1[i];
    if (c2 != 0.0f) xn += c2 * h2[i];
    h0[i] = m;
    x_next[i] = xn;
    if (pred_x0) pred_x0[i] = m;
  }
}
__global__ void dpmpp_step_kernel(const float* x, const float* __restrict__ e_c, const float* __restrict__ e_u,
                                  const float* __restrict__ coef, int index, float scale, float* hist, float* x_next,
                                  float* __restrict__ pred_x0, long n) {
  dpmpp_step_body(x, e_c, e_u, coef, index, scale, hist, x_next, pred_x0, n);
}
// device cursor i = 0..S-1 = the table row (clamped, so a replay past the end cannot index outside the table)
__global__ void dpmpp_step_dev_kernel(const float* x, const float* __restrict__ e_c, const float* __restrict__ e_u,
                                      const float* __restrict__ coef, const int* __restrict__ cursor, int S, float scale,
                                      float* hist, float* x_next, float* __restrict__ pred_x0, long n) {
  const int index = min(max(*cursor, 0), S - 1);
  dpmpp_step_body(x, e_c, e_u, coef, index, scale, hist, x_next, pred_x0, n);
}
// ts[:] = t_in of row min(cursor, S - 1): the (float) model time of the step the cursor points at
__global__ void dpm_set_t_kernel(const float* __restrict__ coef, const int* __restrict__ cursor, int S,
                                 float* __restrict__ ts, int n) {
  const int index = min(max(*cursor, 0), S - 1);
  const float t = coef[(long)index * 8 + 6];
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) ts[i] = t;
}

// ---------------------------------------------------------------- PLMS update (pseudo linear multistep, arXiv:2202.09778)
// coef = DDIM's device table [S][4] fp32 {a_t, a_prev, sigma_t, sqrt(1 - a_t)}; iteration `iter` uses row S - 1 - iter.
// hist = [4][n] fp32 ring, the guided eps of iteration k lives in slot k % 4.  upd(x, e') is DDIM's update:
//   pred_x0 = (x - sqrt(1 - a_t) e') / sqrt(a_t),   x_prev = sqrt(a_prev) pred_x0 + sqrt(1 - a_prev - sigma_t^2) e'
// phase PLMS_MULTISTEP (iter >= 1): e = guided eps, hist[iter % 4] = e, e' = Adams-Bashforth over e and the last
//   min(iter, 3) slots ((3 e - o1) / 2, (23 e - 16 o1 + 5 o2) / 12, (55 e - 59 o1 + 37 o2 - 9 o3) / 24), upd(x, e').
// phase PLMS_START (iter 0): hist[0] = e, x_out = upd(x, e).x_prev (the predictor; pred_x0 is not written).
// phase PLMS_FINISH (iter 0): e_n = guided eps at the predictor, e' = (hist[0] + e_n) / 2, upd(x, e'); hist is not written.
// A slot that is not part of the order is not read (it is uninitialised in the first iterations).  x_out may alias x
// (element-wise), so neither is __restrict__.  One body for the host-index and the device-cursor launch: an eager and a
// replayed step give the same bits.
enum { PLMS_MULTISTEP = 0, PLMS_START = 1, PLMS_FINISH = 2 };
__device__ __forceinline__ void plms_step_body(const float* x, const float* __restrict__ e_c,
                                               const float* __restrict__ e_u, const float* __restrict__ coef, int iter,
                                               int S, int phase, float scale, float* hist, float* x_out,
                                               float* __restrict__ pred_x0, long n) {
  const float* row = coef + (long)(S - 1 - iter) * 4;
  const float a_t = row[0], a_prev = row[1], sigma = row[2], s1m = row[3];
  const float sqrt_at = sqrtf(a_t), sqrt_ap = sqrtf(a_prev), dir = sqrtf(1.0f - a_prev - sigma * sigma);
  const int order = phase == PLMS_MULTISTEP ? min(iter, 3) : 0;      // how many older slots enter e'
  float* hw = hist + (long)(iter % 4) * n;
  const float* o1 = hist + (long)((iter + 3) % 4) * n;
  const float* o2 = hist + (long)((iter + 2) % 4) * n;
  const float* o3 = hist + (long)((iter + 1) % 4) * n;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    float e = e_c[i];
    if (e_u) { const float u = e_u[i]; e = u + scale * (e - u); }
    float ep = e;
    if (phase == PLMS_FINISH) ep = (hw[i] + e) / 2.0f;
    else if (order == 1) ep = (3.0f * e - o1[i]) / 2.0f;
    else if (order == 2) ep = (23.0f * e - 16.0f * o1[i] + 5.0f * o2[i]) / 12.0f;
    else if (order == 3) ep = (55.0f * e - 59.0f * o1[i] + 37.0f * o2[i] - 9.0f * o3[i]) / 24.0f;
    if (phase != PLMS_FINISH) hw[i] = e;
    const float p0 = (x[i] - s1m * ep) / sqrt_at;
    x_out[i] = sqrt_ap * p0 + dir * ep;
    if (pred_x0 && phase != PLMS_START) pred_x0[i] = p0;
  }
}
__global__ void plms_step_kernel(const float* x, const float* __restrict__ e_c, const float* __restrict__ e_u,
                                 const float* __restrict__ coef, int iter, int S, int phase, float scale, float* hist,
                                 float* x_out, float* __restrict__ pred_x0, long n) {
  plms_step_body(x, e_c, e_u, coef, iter, S, phase, scale, hist, x_out, pred_x0, n);
}
// device cursor = the iteration number, clamped to the multistep range [1, S - 1] (the start iteration never replays,
// and a replay past the end cannot index outside the table)
__global__ void plms_step_dev_kernel(const float* x, const float* __restrict__ e_c, const float* __restrict__ e_u,
                                     const float* __restrict__ coef, const int* __restrict__ cursor, int S, float scale,
                                     float* hist, float* x_out, float* __restrict__ pred_x0, long n) {
  const int iter = min(max(*cursor, 1), S - 1);
  plms_step_body(x, e_c, e_u, coef, iter, S, PLMS_MULTISTEP, scale, hist, x_out, pred_x0, n);
}

// ---------------------------------------------------------------- 2x2 sum pool (data-gradient of nearest x2)
// in [B, 2H, 2W, C] (ldi) -> out [B, H, W, C] (ldo), out (+)= sum of the 2x2 block
template <typename T>
__global__ void pool2x2_kernel(const T* __restrict__ in, long ldi, T* __restrict__ out, long ldo, int B, int H,
                               int W, int C, int accumulate) {
  const int C8 = C / 8;
  const long n = (long)B * H * W * C8;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    const int v = (int)(i % C8); long r = i / C8;
    const int x = (int)(r % W); r /= W; const int y = (int)(r % H); const int b = (int)(r / H);
    float s[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) s[e] = 0.f;
    const long orow = ((long)b * H + y) * W + x;
    if (accumulate) load8(out + orow * ldo + v * 8, s);
#pragma unroll
    for (int dy = 0; dy < 2; ++dy)
#pragma unroll
      for (int dx = 0; dx < 2; ++dx) {
        float f[8];
        load8(in + (((long)b * 2 * H + 2 * y + dy) * 2 * W + 2 * x + dx) * ldi + v * 8, f);
#pragma unroll
        for (int e = 0; e < 8; ++e) s[e] += f[e];
      }
    store8(out + orow * ldo + v * 8, s);
  }
}

// ---------------------------------------------------------------- per-sample column sums
// out[b, c] += sum_p in[b*HW + p, c]   (fp32 atomics; data-gradient of the `h + emb_out[:, :, None, None]`
// broadcast, openaimodel.py:272, and bias gradients of the zero convs)
template <typename T>
__global__ void colsum_kernel(const T* __restrict__ in, long ldi, float* __restrict__ out, long ldo, int HW, int C,
                              int ppc, float scale, float* __restrict__ partial) {
  // partial != nullptr: the block's column sums go to partial[(b * nchunk + chunk) * C + c] and a second kernel
  // adds them up (one writer per column: deterministic, and no same-cache-line atomics -- 512 blocks x 320
  // atomics onto ten cache lines cost ~25 us, five times the 21 MB read itself)
  __shared__ float red[256 * 8];
  const int C8 = C / 8;
  const int b = blockIdx.y, p0 = blockIdx.x * ppc, p1 = min(HW, p0 + ppc);
  const int VX = blockDim.x < C8 ? blockDim.x : C8;
  const int PY = blockDim.x / VX;
  const int vx = threadIdx.x % VX, py = threadIdx.x / VX;
  const bool live = py < PY;
  // uniform trip count (C8 <= VX, or C8 a multiple of VX is NOT required: guard inside)
  for (int v0 = 0; v0 < C8; v0 += VX) {
    const int v = v0 + vx;
    float s[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) s[e] = 0.f;
    if (live && v < C8) {
      const T* src = in + ((long)b * HW) * ldi + v * 8;
      int p = p0 + py;
      for (; p + 3 * PY < p1; p += 4 * PY) {   // four independent loads in flight
        float f0[8], f1[8], f2[8], f3[8];
        load8(src + (long)p * ldi, f0);
        load8(src + (long)(p + PY) * ldi, f1);
        load8(src + (long)(p + 2 * PY) * ldi, f2);
        load8(src + (long)(p + 3 * PY) * ldi, f3);
#pragma unroll
        for (int e = 0; e < 8; ++e) s[e] += (f0[e] + f1[e]) + (f2[e] + f3[e]);
      }
      for (; p < p1; p += PY) {
        float f[8];
        load8(src + (long)p * ldi, f);
#pragma unroll
        for (int e = 0; e < 8; ++e) s[e] += f[e];
      }
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) red[threadIdx.x * 8 + e] = s[e];
    __syncthreads();
    if (py == 0 && v < C8) {
      for (int k = 1; k < PY; ++k)
#pragma unroll
        for (int e = 0; e < 8; ++e) s[e] += red[(k * VX + vx) * 8 + e];
      if (partial) {
        float* dst = partial + ((long)b * gridDim.x + blockIdx.x) * C + v * 8;
#pragma unroll
        for (int e = 0; e < 8; ++e) dst[e] = s[e];
      } else {
#pragma unroll
        for (int e = 0; e < 8; ++e) atomicAdd(out + (long)b * ldo + v * 8 + e, s[e] * scale);
      }
    }
    __syncthreads();
  }
}

// out[b][c] += scale * sum_k partial[(b * nchunk + k) * C + c]; 32 columns x 32 chunk lanes per workgroup
__global__ __launch_bounds__(1024) void colsum_finish_kernel(const float* __restrict__ partial, int nchunk, int C,
                                                             float* __restrict__ out, long ldo, float scale) {
  __shared__ float red[1024];
  const int b = blockIdx.y, cl = threadIdx.x & 31, kl = threadIdx.x >> 5;
  const int c = blockIdx.x * 32 + cl;
  float s = 0.f;
  if (c < C)
#pragma unroll 8
    for (int k = kl; k < nchunk; k += 32) s += partial[((long)b * nchunk + k) * C + c];
  red[threadIdx.x] = s;
  __syncthreads();
  if (kl == 0 && c < C) {
    float t = 0.f;
#pragma unroll
    for (int k = 0; k < 32; ++k) t += red[k * 32 + cl];
    out[(long)b * ldo + c] += scale * t;
  }
}

// ---------------------------------------------------------------- strided 2-D convert fp32 -> T
template <typename T>
__global__ void pack_kernel(const float* __restrict__ in, long ldi, T* __restrict__ out, long ldo, long R, int C,
                            int Cpad) {
  const long n = R * Cpad;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    const long r = i / Cpad; const int c = (int)(i - r * Cpad);
    out[r * ldo + c] = from_f<T>(c < C ? in[r * ldi + c] : 0.f);
  }
}

// ---------------------------------------------------------------- ViT patch rows / token assembly (CLIPVisionEmbeddings)
// NCHW fp32 pixels [B, C, S, S] -> patch rows [B (S/P)^2, Kpad]: row (b, gy, gx), column (c, py, px) = pixel
// (b, c, gy P + py, gx P + px), columns [C P P, Kpad) zero.  One lane per 8 output columns (one 16-byte store in bf16, two in
// fp32); PAIR: P and S even, so columns (2j, 2j + 1) are neighbours of one pixel row at an 8-byte aligned address -- float2 loads.
template <typename T, bool PAIR>
__global__ void vit_patch_rows_kernel(const float* __restrict__ px, T* __restrict__ out, long ldo, int B, int C, int S, int P,
                                      int Kpad) {
  const int G = S / P, K = C * P * P, K8 = Kpad / 8;
  const long n = (long)B * G * G * K8;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    const long row = i / K8; const int k0 = (int)(i - row * K8) * 8;
    const int b = (int)(row / (G * G)), g = (int)(row - (long)b * G * G), gy = g / G, gx = g - gy * G;
    float v[8];
#pragma unroll
    for (int e = 0; e < 8; e += PAIR ? 2 : 1) {
      const int k = k0 + e;
      const int c = k / (P * P), r = k - c * P * P, py = r / P, pxl = r - py * P;
      const long src = (((long)b * C + c) * S + gy * P + py) * S + gx * P + pxl;
      if constexpr (PAIR) {
        const float2 t = k < K ? *reinterpret_cast<const float2*>(px + src) : make_float2(0.f, 0.f);   // (K even: a pair is whole)
        v[e] = t.x; v[e + 1] = t.y;
      } else {
        v[e] = k < K ? px[src] : 0.f;
      }
    }
    store8(out + row * ldo + k0, v);
  }
}

// out[b, 0, :] = cls + pos[0];  out[b, 1 + i, :] = patch[b (T - 1) + i, :] + pos[1 + i]: fp32 add, one rounding to T
template <typename T>
__global__ void vit_tokens_kernel(const T* __restrict__ patch, long ldp, const float* __restrict__ cls,
                                  const float* __restrict__ pos, T* __restrict__ out, long ldo, int B, int Tn, int D) {
  const int D8 = D / 8;
  const long n = (long)B * Tn * D8;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    const long row = i / D8; const int c = (int)(i - row * D8) * 8;
    const int b = (int)(row / Tn), t = (int)(row - (long)b * Tn);
    float v[8], p[8];
    if (t == 0) load8(cls + c, v);
    else load8(patch + ((long)b * (Tn - 1) + t - 1) * ldp + c, v);
    load8(pos + (long)t * D + c, p);
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] += p[e];
    store8(out + row * ldo + c, v);
  }
}

// CLIPTextEmbeddings: out[b T + t, :] = tok[ids[b, t]] + pos[t] (fp32 tables, fp32 add, one rounding to T).  An id outside
// [0, vocab) is clamped: nothing is read out of range whatever the ids hold.
template <typename T>
__global__ void clip_text_embed_kernel(const long* __restrict__ ids, const float* __restrict__ tok, const float* __restrict__ pos,
                                       T* __restrict__ out, long ldo, int B, int Tn, int D, int vocab) {
  const int D8 = D / 8;
  const long n = (long)B * Tn * D8;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    const long row = i / D8; const int c = (int)(i - row * D8) * 8;
    const int t = (int)(row % Tn);
    long id = ids[row];
    id = id < 0 ? 0 : (id >= vocab ? vocab - 1 : id);
    float v[8], p[8];
    load8(tok + id * D + c, v);
    load8(pos + (long)t * D + c, p);
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] += p[e];
    store8(out + row * ldo + c, v);
  }
}
// dst[r, :] = src[rows[r], :] (the pooled rows of CLIPTextTransformer); a row index outside [0, nsrc) is clamped
template <typename T>
__global__ void gather_rows_kernel(const T* __restrict__ src, long lds_, const long* __restrict__ rows, T* __restrict__ dst, long ldd,
                                   int R, int D, int nsrc) {
  const int D8 = D / 8;
  const long n = (long)R * D8;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    const long r = i / D8; const int c = (int)(i - r * D8) * 8;
    long s = rows[r];
    s = s < 0 ? 0 : (s >= nsrc ? nsrc - 1 : s);
    float v[8];
    load8(src + s * lds_ + c, v);
    store8(dst + r * ldd + c, v);
  }
}

// ================================================================= host launchers
// Every launcher decides its refusals (CL_EINVAL; listed per entry point in include/ctrlora_hip.h) on the host before anything is
// launched, and keeps a read-only record of what it launched (elementwise.h: EwLaunchRec): reset on entry, written by ew_done()
// after the launch check.  Null pointers are refused only where the call has work to do: an empty call (n == 0, what an empty
// tensor's null data pointer comes with) stays CL_OK.
EwLaunchRec g_ew_last{};

static inline bool bad_dtype(int dtype) { return dtype != CL_BF16 && dtype != CL_F32; }
static inline bool mis16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) != 0; }
static int ew_done(int id, int dtype, dim3 grid, int threads, int form = 0, long aux = 0) {
  CL_CHECK_LAUNCH();
  g_ew_last = EwLaunchRec{id, dtype, (int)grid.x, (int)grid.y, (int)grid.z, threads, form, (int)(aux < 0x7fffffffL ? aux : 0x7fffffffL)};
  return CL_OK;
}

int vit_patch_rows(int dtype, const float* pixels, void* out, long ldo, int B, int C, int S, int P, int Kpad, hipStream_t st) {
  ew_rec_begin();
  if (bad_dtype(dtype) || !pixels || !out) return CL_EINVAL;
  if (B < 1 || C < 1 || P < 1 || S < P || S % P || Kpad % 8 || Kpad < C * P * P || ldo < Kpad || ldo % 8) return CL_EINVAL;
  if (mis16(pixels) || mis16(out)) return CL_EINVAL;
  const dim3 grid(ew_grid((long)B * (S / P) * (S / P) * (Kpad / 8)));
  const bool pair = P % 2 == 0 && S % 2 == 0;
#define VIT_PR(T, PAIR) hipLaunchKernelGGL((vit_patch_rows_kernel<T, PAIR>), grid, dim3(256), 0, st, pixels, (T*)out, ldo, B, C, S, P, Kpad)
  if (dtype == CL_BF16) { if (pair) VIT_PR(bf16_t, true); else VIT_PR(bf16_t, false); }
  else { if (pair) VIT_PR(float, true); else VIT_PR(float, false); }
#undef VIT_PR
  return ew_done(EW_VIT_PATCH_ROWS, dtype, grid, 256, pair ? 1 : 0);
}
int vit_tokens(int dtype, const void* patch, long ldp, const float* cls, const float* pos, void* out, long ldo, int B, int T,
               int D, hipStream_t st) {
  ew_rec_begin();
  if (bad_dtype(dtype) || !patch || !cls || !pos || !out) return CL_EINVAL;
  if (B < 1 || T < 2 || D < 8 || D % 8 || ldp % 8 || ldo % 8 || ldp < D || ldo < D) return CL_EINVAL;
  if (mis16(patch) || mis16(cls) || mis16(pos) || mis16(out)) return CL_EINVAL;
  const dim3 grid(ew_grid((long)B * T * (D / 8)));
  if (dtype == CL_BF16) hipLaunchKernelGGL((vit_tokens_kernel<bf16_t>), grid, dim3(256), 0, st, (const bf16_t*)patch, ldp, cls, pos, (bf16_t*)out, ldo, B, T, D);
  else hipLaunchKernelGGL((vit_tokens_kernel<float>), grid, dim3(256), 0, st, (const float*)patch, ldp, cls, pos, (float*)out, ldo, B, T, D);
  return ew_done(EW_VIT_TOKENS, dtype, grid, 256);
}
int clip_text_embed(int dtype, const long* ids, const float* tok, const float* pos, void* out, long ldo, int B, int T, int D, int vocab,
                    hipStream_t st) {
  ew_rec_begin();
  if (bad_dtype(dtype) || !ids || !tok || !pos || !out) return CL_EINVAL;
  if (B < 1 || T < 1 || vocab < 1 || D < 8 || D % 8 || ldo % 8 || ldo < D) return CL_EINVAL;
  if ((reinterpret_cast<uintptr_t>(ids) & 7) || mis16(tok) || mis16(pos) || mis16(out)) return CL_EINVAL;
  const dim3 grid(ew_grid((long)B * T * (D / 8)));
  if (dtype == CL_BF16) hipLaunchKernelGGL((clip_text_embed_kernel<bf16_t>), grid, dim3(256), 0, st, ids, tok, pos, (bf16_t*)out, ldo, B, T, D, vocab);
  else hipLaunchKernelGGL((clip_text_embed_kernel<float>), grid, dim3(256), 0, st, ids, tok, pos, (float*)out, ldo, B, T, D, vocab);
  return ew_done(EW_CLIP_TEXT_EMBED, dtype, grid, 256);
}
int gather_rows(int dtype, const void* src, long lds_, const long* rows, void* dst, long ldd, int R, int D, int nsrc, hipStream_t st) {
  ew_rec_begin();
  if (bad_dtype(dtype) || !src || !rows || !dst) return CL_EINVAL;
  if (R < 1 || nsrc < 1 || D < 8 || D % 8 || lds_ % 8 || ldd % 8 || lds_ < D || ldd < D) return CL_EINVAL;
  if ((reinterpret_cast<uintptr_t>(rows) & 7) || mis16(src) || mis16(dst)) return CL_EINVAL;
  const dim3 grid(ew_grid((long)R * (D / 8)));
  if (dtype == CL_BF16) hipLaunchKernelGGL((gather_rows_kernel<bf16_t>), grid, dim3(256), 0, st, (const bf16_t*)src, lds_, rows, (bf16_t*)dst, ldd, R, D, nsrc);
  else hipLaunchKernelGGL((gather_rows_kernel<float>), grid, dim3(256), 0, st, (const float*)src, lds_, rows, (float*)dst, ldd, R, D, nsrc);
  return ew_done(EW_GATHER_ROWS, dtype, grid, 256);
}
int geglu_fwd(int dtype, const void* h, long ldh, void* out, long ldo, long M, int F, hipStream_t st) {
  ew_rec_begin();
  if (bad_dtype(dtype) || M < 0 || F < 0 || F % 8 || ldh % 8 || ldo % 8 || ldh < 2L * F || ldo < F) return CL_EINVAL;
  if (M * F > 0 && (!h || !out)) return CL_EINVAL;
  if (mis16(h) || mis16(out)) return CL_EINVAL;
  const dim3 grid(ew_grid(M * (F / 8)));
  if (dtype == CL_BF16) hipLaunchKernelGGL((geglu_fwd_kernel<bf16_t>), grid, dim3(256), 0, st, (const bf16_t*)h, ldh, (bf16_t*)out, ldo, M, F);
  else hipLaunchKernelGGL((geglu_fwd_kernel<float>), grid, dim3(256), 0, st, (const float*)h, ldh, (float*)out, ldo, M, F);
  return ew_done(EW_GEGLU_FWD, dtype, grid, 256);
}
int geglu_bwd(int dtype, const void* h, long ldh, const void* dout, long lddo, void* dh, long lddh, long M, int F, hipStream_t st) {
  ew_rec_begin();
  if (bad_dtype(dtype) || M < 0 || F < 0 || F % 8 || ldh % 8 || lddo % 8 || lddh % 8 || ldh < 2L * F || lddo < F || lddh < 2L * F) return CL_EINVAL;
  if (M * F > 0 && (!h || !dout || !dh)) return CL_EINVAL;
  if (mis16(h) || mis16(dout) || mis16(dh)) return CL_EINVAL;
  const dim3 grid(ew_grid(M * (F / 8)));
  if (dtype == CL_BF16) hipLaunchKernelGGL((geglu_bwd_kernel<bf16_t>), grid, dim3(256), 0, st, (const bf16_t*)h, ldh, (const bf16_t*)dout, lddo, (bf16_t*)dh, lddh, M, F);
  else hipLaunchKernelGGL((geglu_bwd_kernel<float>), grid, dim3(256), 0, st, (const float*)h, ldh, (const float*)dout, lddo, (float*)dh, lddh, M, F);
  return ew_done(EW_GEGLU_BWD, dtype, grid, 256);
}
int silu_fwd(int dtype, const void* x, void* y, long n, hipStream_t st) {
  ew_rec_begin();
  if (bad_dtype(dtype) || n < 0 || n % 8) return CL_EINVAL;
  if (n > 0 && (!x || !y)) return CL_EINVAL;
  if (mis16(x) || mis16(y)) return CL_EINVAL;
  const dim3 grid(ew_grid(n / 8));
  if (dtype == CL_BF16) hipLaunchKernelGGL((silu_fwd_kernel<bf16_t>), grid, dim3(256), 0, st, (const bf16_t*)x, (bf16_t*)y, n / 8);
  else hipLaunchKernelGGL((silu_fwd_kernel<float>), grid, dim3(256), 0, st, (const float*)x, (float*)y, n / 8);
  return ew_done(EW_SILU_FWD, dtype, grid, 256);
}
int silu_bwd(int dtype, const void* x, const void* dy, void* dx, long n, hipStream_t st) {
  ew_rec_begin();
  if (bad_dtype(dtype) || n < 0 || n % 8) return CL_EINVAL;
  if (n > 0 && (!x || !dy || !dx)) return CL_EINVAL;
  if (mis16(x) || mis16(dy) || mis16(dx)) return CL_EINVAL;
  const dim3 grid(ew_grid(n / 8));
  if (dtype == CL_BF16) hipLaunchKernelGGL((silu_bwd_kernel<bf16_t>), grid, dim3(256), 0, st, (const bf16_t*)x, (const bf16_t*)dy, (bf16_t*)dx, n / 8);
  else hipLaunchKernelGGL((silu_bwd_kernel<float>), grid, dim3(256), 0, st, (const float*)x, (const float*)dy, (float*)dx, n / 8);
  return ew_done(EW_SILU_BWD, dtype, grid, 256);
}
int axpby(int dtype, const void* x, long ldx, void* y, long ldy, long M, int C, float a, float b, hipStream_t st) {
  ew_rec_begin();
  if (bad_dtype(dtype) || M < 0 || C < 0 || C % 8 || ldx % 8 || ldy % 8 || ldx < C || ldy < C) return CL_EINVAL;
  if (M * C > 0 && (!x || !y)) return CL_EINVAL;
  if (mis16(x) || mis16(y)) return CL_EINVAL;
  const dim3 grid(ew_grid(M * (C / 8)));
  if (dtype == CL_BF16) hipLaunchKernelGGL((axpby_kernel<bf16_t>), grid, dim3(256), 0, st, (const bf16_t*)x, ldx, (bf16_t*)y, ldy, M, C, a, b);
  else hipLaunchKernelGGL((axpby_kernel<float>), grid, dim3(256), 0, st, (const float*)x, ldx, (float*)y, ldy, M, C, a, b);
  return ew_done(EW_AXPBY, dtype, grid, 256);
}
// the 64-tile kernels put the batch in grid.z (at most 65535) and the column tiles in grid.y
static inline bool bad_tile_grid(int batch, int rows, int cols) {
  return batch < 1 || batch > 65535 || rows < 1 || cols < 1 || (cols + 63) / 64 > 65535;
}
int transpose(int in_dtype, int out_dtype, const void* in, long ldi, long bsi, void* out, long ldo, long bso,
              int Bt, int R, int C, int Rpad, hipStream_t st) {
  ew_rec_begin();
  if (Rpad < R || ldo < Rpad || bad_tile_grid(Bt, R, C) || !in || !out) return CL_EINVAL;
  const dim3 grid((Rpad + 63) / 64, (C + 63) / 64, Bt);
  if (in_dtype == CL_F32 && out_dtype == CL_BF16) hipLaunchKernelGGL((transpose_kernel<float, bf16_t>), grid, dim3(256), 0, st, (const float*)in, ldi, bsi, (bf16_t*)out, ldo, bso, R, C, Rpad);
  else if (in_dtype == CL_F32 && out_dtype == CL_F32) hipLaunchKernelGGL((transpose_kernel<float, float>), grid, dim3(256), 0, st, (const float*)in, ldi, bsi, (float*)out, ldo, bso, R, C, Rpad);
  else if (in_dtype == CL_BF16 && out_dtype == CL_BF16) hipLaunchKernelGGL((transpose_kernel<bf16_t, bf16_t>), grid, dim3(256), 0, st, (const bf16_t*)in, ldi, bsi, (bf16_t*)out, ldo, bso, R, C, Rpad);
  else return CL_EINVAL;
  return ew_done(EW_TRANSPOSE, out_dtype, grid, 256, in_dtype);
}
int nchw_to_tok(int dtype, const float* in, void* out, long ldo, int B, int Cin, int Cpad, int HW, hipStream_t st) {
  ew_rec_begin();
  if (bad_dtype(dtype) || Cpad < Cin || ldo < Cpad || bad_tile_grid(B, HW, Cpad) || Cin < 1 || !in || !out) return CL_EINVAL;
  const dim3 grid((HW + 63) / 64, (Cpad + 63) / 64, B);
  if (dtype == CL_BF16) hipLaunchKernelGGL((nchw_to_tok_kernel<bf16_t>), grid, dim3(256), 0, st, in, (bf16_t*)out, ldo, Cin, Cpad, HW);
  else hipLaunchKernelGGL((nchw_to_tok_kernel<float>), grid, dim3(256), 0, st, in, (float*)out, ldo, Cin, Cpad, HW);
  return ew_done(EW_NCHW_TO_TOK, dtype, grid, 256);
}
int tok_to_nchw(int dtype, const void* in, long ldi, float* out, int B, int C, int HW, float alpha, float beta, hipStream_t st) {
  ew_rec_begin();
  if (bad_dtype(dtype) || bad_tile_grid(B, HW, C) || !in || !out) return CL_EINVAL;
  const dim3 grid((HW + 63) / 64, (C + 63) / 64, B);
  if (dtype == CL_BF16) hipLaunchKernelGGL((tok_to_nchw_kernel<bf16_t>), grid, dim3(256), 0, st, (const bf16_t*)in, ldi, out, C, HW, alpha, beta);
  else hipLaunchKernelGGL((tok_to_nchw_kernel<float>), grid, dim3(256), 0, st, (const float*)in, ldi, out, C, HW, alpha, beta);
  return ew_done(EW_TOK_TO_NCHW, dtype, grid, 256);
}
// both embeddings index with int: B half must be in [1, INT_MAX]
static inline bool bad_embed(int dtype, const void* t, const float* freqs, const void* out, long ldo, int B, int half) {
  return bad_dtype(dtype) || B < 1 || half < 1 || (long)B * half > 0x7fffffffL || ldo < 2L * half || !t || !freqs || !out;
}
int timestep_embed(int dtype, const long* t, const float* freqs, void* out, long ldo, int B, int half, hipStream_t st) {
  ew_rec_begin();
  if (bad_embed(dtype, t, freqs, out, ldo, B, half)) return CL_EINVAL;
  const int n = B * half;
  const dim3 grid((n + 255) / 256);
  if (dtype == CL_BF16) hipLaunchKernelGGL((timestep_embed_kernel<bf16_t>), grid, dim3(256), 0, st, t, freqs, (bf16_t*)out, ldo, B, half);
  else hipLaunchKernelGGL((timestep_embed_kernel<float>), grid, dim3(256), 0, st, t, freqs, (float*)out, ldo, B, half);
  return ew_done(EW_TIMESTEP, dtype, grid, 256);
}
int timestep_embed_f(int dtype, const float* t, const float* freqs, void* out, long ldo, int B, int half, hipStream_t st) {
  ew_rec_begin();
  if (bad_embed(dtype, t, freqs, out, ldo, B, half)) return CL_EINVAL;
  const int n = B * half;
  const dim3 grid((n + 255) / 256);
  if (dtype == CL_BF16) hipLaunchKernelGGL((timestep_embed_f_kernel<bf16_t>), grid, dim3(256), 0, st, t, freqs, (bf16_t*)out, ldo, B, half);
  else hipLaunchKernelGGL((timestep_embed_f_kernel<float>), grid, dim3(256), 0, st, t, freqs, (float*)out, ldo, B, half);
  return ew_done(EW_TIMESTEP_F, dtype, grid, 256);
}
int qsample(const float* z, const float* noise, const long* t, const float* sqrt_ac, const float* sqrt_1mac,
            float* out, int B, long per, hipStream_t st) {
  ew_rec_begin();
  if (B < 0 || per < 0) return CL_EINVAL;
  const long n = (long)B * per;
  if (n > 0 && (!z || !noise || !t || !sqrt_ac || !sqrt_1mac || !out)) return CL_EINVAL;
  const dim3 grid(ew_grid(n));
  hipLaunchKernelGGL(qsample_kernel, grid, dim3(256), 0, st, z, noise, t, sqrt_ac, sqrt_1mac, out, per, n);
  return ew_done(EW_QSAMPLE, -1, grid, 256);
}
static inline bool overlaps(const float* a, long na, const float* b, long nb) {
  const uintptr_t a0 = reinterpret_cast<uintptr_t>(a), b0 = reinterpret_cast<uintptr_t>(b);
  return a0 < b0 + (uintptr_t)nb * sizeof(float) && b0 < a0 + (uintptr_t)na * sizeof(float);
}
int qsample_blend(const float* x0, const float* noise, const long* t, const float* sqrt_ac, const float* sqrt_1mac, int T,
                  const float* mask, int mask_per_batch, int mask_per_channel, const float* x, float* out, int B, int C, long HW,
                  hipStream_t st) {
  ew_rec_begin();
  if (B < 0 || C < 1 || HW < 1 || T < 1) return CL_EINVAL;
  if (B == 0) return CL_OK;
  if (!x0 || !noise || !t || !sqrt_ac || !sqrt_1mac || !mask || !x || !out) return CL_EINVAL;
  const int pb = mask_per_batch ? 1 : 0, pc = mask_per_channel ? 1 : 0;
  const long n = (long)B * C * HW, nm = (long)(pb ? B : 1) * (pc ? C : 1) * HW;
  // out is written while other work items still read x0 / noise / mask: only x may be out itself (the same element, in place)
  if (overlaps(out, n, x0, n) || overlaps(out, n, noise, n) || overlaps(out, n, mask, nm)) return CL_EINVAL;
  if (out != x && overlaps(out, n, x, n)) return CL_EINVAL;
  const bool vec = HW % 4 == 0 && !mis16(x0) && !mis16(noise) && !mis16(mask) && !mis16(x) && !mis16(out);
  const long nw = vec ? n / 4 : n;
  const dim3 grid(ew_grid(nw));
  if (vec) hipLaunchKernelGGL((qsample_blend_kernel<4>), grid, dim3(256), 0, st, x0, noise, t, sqrt_ac, sqrt_1mac, T, mask, pb, pc, x, out, C, HW, nw);
  else hipLaunchKernelGGL((qsample_blend_kernel<1>), grid, dim3(256), 0, st, x0, noise, t, sqrt_ac, sqrt_1mac, T, mask, pb, pc, x, out, C, HW, nw);
  return ew_done(EW_QSAMPLE_BLEND, -1, grid, 256, vec ? 1 : 0, pb | (pc << 1));
}
int posterior_sample_pair(const float* mom_a, const float* e_a, float* out_a, const float* mom_b, const float* e_b, float* out_b,
                          int B, long per, float scale, hipStream_t st) {
  ew_rec_begin();
  if (B < 1 || per < 1 || !mom_a || !e_a || !out_a) return CL_EINVAL;
  const int given_b = (mom_b ? 1 : 0) + (e_b ? 1 : 0) + (out_b ? 1 : 0);
  if (given_b != 0 && given_b != 3) return CL_EINVAL;              // a half-given second tensor
  const int nt = given_b ? 2 : 1;
  const bool vec = per % 4 == 0 && !mis16(mom_a) && !mis16(e_a) && !mis16(out_a) &&
                   (!given_b || (!mis16(mom_b) && !mis16(e_b) && !mis16(out_b)));
  const long nw = (long)B * (vec ? per / 4 : per);
  const dim3 grid(ew_grid(nw * nt));
  if (vec) hipLaunchKernelGGL((posterior_sample_pair_kernel<4>), grid, dim3(256), 0, st, mom_a, e_a, out_a, mom_b, e_b, out_b, per, nw, nt, scale);
  else hipLaunchKernelGGL((posterior_sample_pair_kernel<1>), grid, dim3(256), 0, st, mom_a, e_a, out_a, mom_b, e_b, out_b, per, nw, nt, scale);
  return ew_done(EW_POSTERIOR_PAIR, -1, grid, 256, vec ? 1 : 0, nt);
}
int mse_loss(const float* eps, const float* target, float* d_eps, float* loss, long n, float gscale, hipStream_t st) {
  ew_rec_begin();
  if (n < 0 || !loss || (n > 0 && (!eps || !target))) return CL_EINVAL;
  if (int rc = zero_bytes(loss, sizeof(float), st)) return rc;
  ew_rec_begin();
  const dim3 grid(ew_grid(n) < 256 ? ew_grid(n) : 256);
  hipLaunchKernelGGL(mse_kernel, grid, dim3(256), 0, st, eps, target, d_eps, loss, n, gscale);
  return ew_done(EW_MSE, -1, grid, 256, 0, grid.x);
}
int ddim_step(const float* x, const float* e_c, const float* e_u, const float* noise, const float* coef, int index,
              float scale, float* x_prev, float* pred_x0, long n, hipStream_t st) {
  ew_rec_begin();
  if (n < 0 || index < 0 || !coef || (n > 0 && (!x || !e_c || !x_prev))) return CL_EINVAL;
  const dim3 grid(ew_grid(n));
  hipLaunchKernelGGL(ddim_step_kernel, grid, dim3(256), 0, st, x, e_c, e_u, noise, coef, index, scale, x_prev, pred_x0, n);
  return ew_done(EW_DDIM_STEP, -1, grid, 256);
}
int adamw(float* p, const float* g, float* m, float* v, long n, float lr, float beta1, float beta2, float eps,
          float wd, int step, float gscale, hipStream_t st) {
  ew_rec_begin();
  if (n < 0 || (n > 0 && (!p || !g || !m || !v))) return CL_EINVAL;
  const dim3 grid(ew_grid(n));
  hipLaunchKernelGGL(adamw_kernel, grid, dim3(256), 0, st, p, g, m, v, n, adam_group(lr, beta1, beta2, eps, wd, gscale, (float)step));
  return ew_done(EW_ADAMW, -1, grid, 256);
}
int plosses_mse(const float* eps, const float* target, float* d_eps, const long* t, const float* lvlb, float* out,
                float* per_sample, float* scratch, int B, long per, float gscale, float w_simple, float w_elbo,
                hipStream_t st) {
  ew_rec_begin();
  if (B < 1 || B > 65535 || per < 1) return CL_EINVAL;
  if (!eps || !target || !out || !scratch || (lvlb && !t)) return CL_EINVAL;
  // d loss / d eps with loss = w_simple * mean(...) (the elbo term is not differentiated: weight 0 in every config)
  const float gmul = 2.0f * gscale * w_simple / ((float)per * (float)B);
  const dim3 grid(PL_CHUNKS, B);
  hipLaunchKernelGGL((plosses_w_partial_kernel<0>), grid, dim3(256), 0, st, eps, target, d_eps, scratch, t, nullptr, per, gmul, 0.f);
  hipLaunchKernelGGL(plosses_w_finish_kernel, dim3(1), dim3(64), 0, st, scratch, t, lvlb, nullptr, out, per_sample, B, per, w_simple, w_elbo);
  return ew_done(EW_PLOSSES, -1, grid, 256);
}
int plosses_w(const float* eps, const float* target, float* d_eps, const long* t, const float* lvlb, const float* wt, float* out,
              float* per_sample, float* scratch, int B, long per, int kind, float delta, float gscale, float w_simple,
              float w_elbo, hipStream_t st) {
  ew_rec_begin();
  if (B < 1 || B > 65535 || per < 1) return CL_EINVAL;
  if (!eps || !target || !out || !scratch || ((lvlb || wt) && !t)) return CL_EINVAL;
  if (kind != 0 && kind != 1) return CL_EINVAL;
  if (kind == 1 && !(std::isfinite(delta) && delta > 0.f)) return CL_EINVAL;
  // rho' carries the 2 of l2 here; the table's factor is applied on the device (elementwise.hip: plosses_w_partial_kernel)
  const float gmul = (kind == 0 ? 2.0f : 1.0f) * gscale * w_simple / ((float)per * (float)B);
  const dim3 grid(PL_CHUNKS, B);
  hipLaunchKernelGGL((kind == 1 ? plosses_w_partial_kernel<1> : plosses_w_partial_kernel<0>), grid, dim3(256), 0, st, eps, target, d_eps,
                     scratch, t, wt, per, gmul, delta);
  hipLaunchKernelGGL(plosses_w_finish_kernel, dim3(1), dim3(64), 0, st, scratch, t, lvlb, wt, out, per_sample, B, per, w_simple, w_elbo);
  return ew_done(EW_PLOSSES, -1, grid, 256, 4 | (kind << 1) | (wt ? 1 : 0));
}
int loss_bands(const float* per_sample, const long* t, int B, int T, int nbands, const int* n_valid, double* acc,
               hipStream_t st) {
  ew_rec_begin();
  if (!per_sample || !t || !acc || (reinterpret_cast<uintptr_t>(acc) & 7)) return CL_EINVAL;
  if (B < 1 || B > 65535 || T < 1 || nbands < 1 || nbands > 64 || nbands > T) return CL_EINVAL;
  hipLaunchKernelGGL(loss_bands_kernel, dim3(1), dim3(LB_THREADS), 0, st, per_sample, t, B, T, nbands, n_valid, acc);
  return ew_done(EW_LOSS_BANDS, -1, dim3(1), LB_THREADS, n_valid ? 1 : 0, nbands);
}
int conv_tap_gather(int dtype, const void* x, long ldx, void* out, long ldo, int B, int Hin, int Win, int Hout, int Wout,
                    int C, int tap, int stride, int pad, hipStream_t st) {
  ew_rec_begin();
  if (bad_dtype(dtype) || C % 8 || ldx % 8 || ldo % 8 || tap < 0 || tap > 8) return CL_EINVAL;
  if (stride < 1 || B < 1 || Hin < 1 || Win < 1 || Hout < 1 || Wout < 1 || C < 8 || ldx < C || ldo < C) return CL_EINVAL;
  if (!x || !out || mis16(x) || mis16(out)) return CL_EINVAL;
  const long total = (long)B * Hout * Wout * (C / 8);
  const dim3 grid(ew_grid(total));
  if (dtype == CL_BF16) hipLaunchKernelGGL((conv_tap_gather_kernel<bf16_t>), grid, dim3(256), 0, st, (const bf16_t*)x, ldx, (bf16_t*)out, ldo, Hin, Win, Hout, Wout, C / 8, tap, stride, pad, total);
  else hipLaunchKernelGGL((conv_tap_gather_kernel<float>), grid, dim3(256), 0, st, (const float*)x, ldx, (float*)out, ldo, Hin, Win, Hout, Wout, C / 8, tap, stride, pad, total);
  return ew_done(EW_CONV_TAP, dtype, grid, 256);
}
int softmax_rows(int dtype, const float* S, long lds_, void* P, long ldp, long M, int N, float scale, hipStream_t st) {
  ew_rec_begin();
  if (bad_dtype(dtype) || N % 4 || N < 4 || N > 8192 || lds_ % 4 || ldp % 4 || lds_ < N || ldp < N || M <= 0 || M > 0x7fffffffL) return CL_EINVAL;
  // float4 loads of S; a row of P is stored 4 elements at a time: 8 bytes in bf16, 16 in fp32
  if (!S || !P || mis16(S) || (reinterpret_cast<uintptr_t>(P) & (dtype == CL_BF16 ? 7 : 15))) return CL_EINVAL;
  const dim3 grid((unsigned)M);
  if (dtype == CL_BF16) hipLaunchKernelGGL((softmax_rows_kernel<bf16_t>), grid, dim3(256), 0, st, S, lds_, (bf16_t*)P, ldp, N, scale);
  else hipLaunchKernelGGL((softmax_rows_kernel<float>), grid, dim3(256), 0, st, S, lds_, (float*)P, ldp, N, scale);
  return ew_done(EW_SOFTMAX, dtype, grid, 256);
}
// Clears are KERNEL nodes, not hipMemsetAsync: a step captured as SEVERAL consecutive hipGraphs in one memory pool
// (the data-parallel segments, train.py) replayed memset nodes of small buffers out of order with their neighbours on
// ROCm 7.2 -- garbage in exactly the gradients that are accumulated into freshly cleared scratch
// (tests/tools/debug_segmented.py).  A fill kernel is ordered like every other launch and costs the same bytes.
__global__ __launch_bounds__(256) void zero_kernel(unsigned char* __restrict__ p, long head, long nvec, long tail) {
  const long i0 = (long)blockIdx.x * blockDim.x + threadIdx.x;
  uint4* body = reinterpret_cast<uint4*>(p + head);
  const uint4 z = make_uint4(0u, 0u, 0u, 0u);
  for (long i = i0; i < nvec; i += (long)gridDim.x * blockDim.x) body[i] = z;
  if (i0 < head) p[i0] = 0;
  if (i0 < tail) p[head + nvec * 16 + i0] = 0;
}
int zero_bytes(void* p, long nbytes, hipStream_t st) {
  ew_rec_begin();
  if (nbytes <= 0) return CL_OK;
  if (!p) return CL_EINVAL;
  long head = (long)((16 - ((uintptr_t)p & 15)) & 15);
  if (head > nbytes) head = nbytes;
  const long nvec = (nbytes - head) / 16, tail = nbytes - head - nvec * 16;
  const dim3 grid(ew_grid(nvec > 16 ? nvec : 16));
  hipLaunchKernelGGL(zero_kernel, grid, dim3(256), 0, st, (unsigned char*)p, head, nvec, tail);
  return ew_done(EW_ZERO, -1, grid, 256, (head ? 1 : 0) | (tail ? 2 : 0), nvec);
}
int tick(int* counter, hipStream_t st) {
  ew_rec_begin();
  if (!counter) return CL_EINVAL;
  hipLaunchKernelGGL(tick_kernel, dim3(1), dim3(1), 0, st, counter);
  return ew_done(EW_TICK, -1, dim3(1), 1);
}
int adamw_dev(float* p, const float* g, float* m, float* v, long n, const float* hyper, int* step, hipStream_t st) {
  ew_rec_begin();
  if (n < 0 || !hyper || !step || (n > 0 && (!p || !g || !m || !v))) return CL_EINVAL;
  const dim3 grid(ew_grid(n));
  hipLaunchKernelGGL(adamw_dev_kernel, grid, dim3(256), 0, st, p, g, m, v, n, hyper, 1, nullptr, step, nullptr);
  return ew_done(EW_ADAMW_DEV, -1, grid, 256);
}
long grad_norm_scratch_floats(int nbuf) {
  if (nbuf < 1 || nbuf > GN_MAX_BUFS) return 0;
  return 2L * GN_MAX_GROUPS;      // one fp64 partial per workgroup, whatever the number of buffers
}
int grad_norm(const float* const* bufs, const long* counts, int nbuf, const float* hyper, const float* max_norm, float* out,
              float* scratch, hipStream_t st) {
  ew_rec_begin();
  if (nbuf < 1 || nbuf > GN_MAX_BUFS || !bufs || !counts || !hyper || !out || !scratch) return CL_EINVAL;
  if (reinterpret_cast<uintptr_t>(scratch) & 7) return CL_EINVAL;        // the partials are fp64
  GradNormBufs a{};
  long total = 0;
  for (int b = 0; b < nbuf; ++b) {
    if (counts[b] < 0 || (counts[b] > 0 && !bufs[b]) || (reinterpret_cast<uintptr_t>(bufs[b]) & 3)) return CL_EINVAL;
    a.p[b] = bufs[b]; a.n[b] = counts[b];
    total += counts[b];
  }
  long groups = (total + 1023) / 1024;             // a workgroup's trip covers 256 x 4 elements
  groups = groups < 1 ? 1 : groups > GN_MAX_GROUPS ? GN_MAX_GROUPS : groups;
  const dim3 grid((unsigned)groups);
  hipLaunchKernelGGL(grad_norm_partial_kernel, grid, dim3(256), 0, st, a, nbuf, reinterpret_cast<double*>(scratch));
  hipLaunchKernelGGL(grad_norm_finish_kernel, dim3(1), dim3(256), 0, st, reinterpret_cast<const double*>(scratch), (int)groups,
                     hyper, max_norm, out);
  return ew_done(EW_GRAD_NORM, -1, grid, 256, 0, nbuf);
}
int adamw_dev_clip(float* p, const float* g, float* m, float* v, long n, const float* hyper, int* step, const float* clip,
                   hipStream_t st) {
  ew_rec_begin();
  if (n < 0 || !hyper || !step || !clip || (n > 0 && (!p || !g || !m || !v))) return CL_EINVAL;
  const dim3 grid(ew_grid(n));
  hipLaunchKernelGGL(adamw_dev_kernel, grid, dim3(256), 0, st, p, g, m, v, n, hyper, 1, nullptr, step, clip);
  return ew_done(EW_ADAMW_DEV_CLIP, -1, grid, 256);
}
int adamw_dev_groups(float* p, const float* g, float* m, float* v, long n, const float* hyper_table, int ngroups,
                     const unsigned char* chunk_group, int* step, const float* clip, hipStream_t st) {
  ew_rec_begin();
  if (!p || !g || !m || !v || !hyper_table || !chunk_group || !step) return CL_EINVAL;      // clip may be NULL: no clipping
  if (n <= 0 || n % 64 != 0 || ngroups < 1 || ngroups > AG_MAX_GROUPS) return CL_EINVAL;
  const dim3 grid(ew_grid(n));                 // a wave per 64-float chunk and trip: n / 64 chunks over 4 waves a workgroup
  hipLaunchKernelGGL(adamw_dev_kernel, grid, dim3(256), 0, st, p, g, m, v, n, hyper_table, ngroups, chunk_group, step, clip);
  return ew_done(EW_ADAMW_DEV_GROUPS, -1, grid, 256, clip ? 1 : 0, ngroups);
}
int lr_schedule(float* hyper_table, int ngroups, const float* lr_table, int T, const int* step, hipStream_t st) {
  ew_rec_begin();
  if (!hyper_table || !lr_table || !step || T < 1 || ngroups < 1 || ngroups > AG_MAX_GROUPS) return CL_EINVAL;
  hipLaunchKernelGGL(lr_schedule_kernel, dim3(1), dim3(64), 0, st, hyper_table, ngroups, lr_table, T, step);
  return ew_done(EW_LR_SCHEDULE, -1, dim3(1), 64, 0, ngroups);
}
// The two-buffer streaming launches: form 1 = 16-byte accesses (both buffers the same distance from a 16-byte boundary) with a
// scalar head and tail, form 0 = one element per work item; aux = the 16-byte vectors.
struct PairSplit { bool vec; long head, nvec, tail; };
static inline PairSplit pair_split(const float* a, const float* b, long n) {
  const uintptr_t oa = reinterpret_cast<uintptr_t>(a) & 15, ob = reinterpret_cast<uintptr_t>(b) & 15;
  if (oa != ob) return {false, 0, n, 0};
  long head = (long)(((16 - oa) & 15) >> 2);
  if (head > n) head = n;
  const long nvec = (n - head) >> 2;
  return {true, head, nvec, n - head - (nvec << 2)};
}
static inline bool mis4(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3) != 0; }
int ema_update(float* shadow, const float* p, long n, const float* decay, const int* num_updates, hipStream_t st) {
  ew_rec_begin();
  if (n < 0 || !decay || !num_updates || (n > 0 && (!shadow || !p))) return CL_EINVAL;
  if (n == 0) return CL_OK;
  if (mis4(shadow) || mis4(p) || overlaps(shadow, n, p, n)) return CL_EINVAL;
  const PairSplit s = pair_split(shadow, p, n);
  const dim3 grid(ew_grid(s.nvec));
  if (s.vec) hipLaunchKernelGGL((ema_update_kernel<4>), grid, dim3(256), 0, st, shadow, p, s.head, s.nvec, s.tail, decay, num_updates);
  else hipLaunchKernelGGL((ema_update_kernel<1>), grid, dim3(256), 0, st, shadow, p, 0L, n, 0L, decay, num_updates);
  return ew_done(EW_EMA_UPDATE, -1, grid, 256, s.vec ? 1 : 0, s.vec ? s.nvec : 0);
}
int swap_buffers(float* a, float* b, long n, hipStream_t st) {
  ew_rec_begin();
  if (n < 0 || (n > 0 && (!a || !b))) return CL_EINVAL;
  if (n == 0 || a == b) return CL_OK;
  if (mis4(a) || mis4(b) || overlaps(a, n, b, n)) return CL_EINVAL;
  const PairSplit s = pair_split(a, b, n);
  const dim3 grid(ew_grid(s.nvec));
  if (s.vec) hipLaunchKernelGGL((swap_kernel<4>), grid, dim3(256), 0, st, a, b, s.head, s.nvec, s.tail);
  else hipLaunchKernelGGL((swap_kernel<1>), grid, dim3(256), 0, st, a, b, 0L, n, 0L);
  return ew_done(EW_SWAP, -1, grid, 256, s.vec ? 1 : 0, s.vec ? s.nvec : 0);
}
int ddim_set_t(const long* table, const int* cursor, int S, long* ts, int n, hipStream_t st) {
  ew_rec_begin();
  if (!table || !cursor || (n > 0 && !ts)) return CL_EINVAL;
  hipLaunchKernelGGL(ddim_set_t_kernel, dim3(1), dim3(256), 0, st, table, cursor, S, ts, n);
  return ew_done(EW_DDIM_SET_T, -1, dim3(1), 256);
}
int ddim_step_dev(const float* x, const float* e_c, const float* e_u, const float* noise, const float* coef,
                  const int* cursor, int S, float scale, float* x_prev, float* pred_x0, long n, hipStream_t st) {
  ew_rec_begin();
  if (n < 0 || !coef || !cursor || (n > 0 && (!x || !e_c || !x_prev))) return CL_EINVAL;
  const dim3 grid(ew_grid(n));
  hipLaunchKernelGGL(ddim_step_dev_kernel, grid, dim3(256), 0, st, x, e_c, e_u, noise, coef, cursor, S, scale, x_prev, pred_x0, n);
  return ew_done(EW_DDIM_STEP_DEV, -1, grid, 256);
}
int dpmpp_step(const float* x, const float* e_c, const float* e_u, const float* coef, int index, int S, float scale,
               float* hist, float* x_next, float* pred_x0, long n, hipStream_t st) {
  ew_rec_begin();
  if (S < 1 || index < 0 || index >= S || n < 1) return CL_EINVAL;
  if (!x || !e_c || !coef || !hist || !x_next) return CL_EINVAL;
  const dim3 grid(ew_grid(n));
  hipLaunchKernelGGL(dpmpp_step_kernel, grid, dim3(256), 0, st, x, e_c, e_u, coef, index, scale, hist, x_next, pred_x0, n);
  return ew_done(EW_DPMPP_STEP, -1, grid, 256);
}
int dpmpp_step_dev(const float* x, const float* e_c, const float* e_u, const float* coef, const int* cursor, int S,
                   float scale, float* hist, float* x_next, float* pred_x0, long n, hipStream_t st) {
  ew_rec_begin();
  if (S < 1 || n < 1) return CL_EINVAL;
  if (!x || !e_c || !coef || !cursor || !hist || !x_next) return CL_EINVAL;
  const dim3 grid(ew_grid(n));
  hipLaunchKernelGGL(dpmpp_step_dev_kernel, grid, dim3(256), 0, st, x, e_c, e_u, coef, cursor, S, scale, hist, x_next, pred_x0, n);
  return ew_done(EW_DPMPP_STEP_DEV, -1, grid, 256);
}
int dpm_set_t(const float* coef, const int* cursor, int S, float* ts, int n, hipStream_t st) {
  ew_rec_begin();
  if (S < 1 || n < 1 || !coef || !cursor || !ts) return CL_EINVAL;
  hipLaunchKernelGGL(dpm_set_t_kernel, dim3(1), dim3(256), 0, st, coef, cursor, S, ts, n);
  return ew_done(EW_DPM_SET_T, -1, dim3(1), 256);
}
int plms_step(const float* x, const float* e_c, const float* e_u, const float* coef, int iter, int S, int phase, float scale,
              float* hist, float* x_out, float* pred_x0, long n, hipStream_t st) {
  ew_rec_begin();
  if (S < 1 || iter < 0 || iter >= S || n < 0) return CL_EINVAL;
  if (phase < PLMS_MULTISTEP || phase > PLMS_FINISH || (phase == PLMS_MULTISTEP) == (iter == 0)) return CL_EINVAL;
  if (!x || !e_c || !coef || !hist || !x_out) return CL_EINVAL;
  if (phase == PLMS_START && x_out == x) return CL_EINVAL;      // PLMS_FINISH updates the iteration's ORIGINAL input
  if (n == 0) return CL_OK;
  const dim3 grid(ew_grid(n));
  hipLaunchKernelGGL(plms_step_kernel, grid, dim3(256), 0, st, x, e_c, e_u, coef, iter, S, phase, scale, hist, x_out, pred_x0, n);
  return ew_done(EW_PLMS_STEP, -1, grid, 256, phase);
}
int plms_step_dev(const float* x, const float* e_c, const float* e_u, const float* coef, const int* cursor, int S,
                  float scale, float* hist, float* x_out, float* pred_x0, long n, hipStream_t st) {
  ew_rec_begin();
  if (S < 2 || n < 0) return CL_EINVAL;
  if (!x || !e_c || !coef || !cursor || !hist || !x_out) return CL_EINVAL;
  if (n == 0) return CL_OK;
  const dim3 grid(ew_grid(n));
  hipLaunchKernelGGL(plms_step_dev_kernel, grid, dim3(256), 0, st, x, e_c, e_u, coef, cursor, S, scale, hist, x_out, pred_x0, n);
  return ew_done(EW_PLMS_STEP_DEV, -1, grid, 256);
}
int pool2x2(int dtype, const void* in, long ldi, void* out, long ldo, int B, int H, int W, int C, int accumulate, hipStream_t st) {
  ew_rec_begin();
  if (bad_dtype(dtype) || B < 0 || H < 0 || W < 0 || C < 0 || C % 8 || ldi % 8 || ldo % 8 || ldi < C || ldo < C) return CL_EINVAL;
  const long n = (long)B * H * W * (C / 8);
  if (n > 0 && (!in || !out)) return CL_EINVAL;
  if (mis16(in) || mis16(out)) return CL_EINVAL;
  const dim3 grid(ew_grid(n));
  if (dtype == CL_BF16) hipLaunchKernelGGL((pool2x2_kernel<bf16_t>), grid, dim3(256), 0, st, (const bf16_t*)in, ldi, (bf16_t*)out, ldo, B, H, W, C, accumulate);
  else hipLaunchKernelGGL((pool2x2_kernel<float>), grid, dim3(256), 0, st, (const float*)in, ldi, (float*)out, ldo, B, H, W, C, accumulate);
  return ew_done(EW_POOL2X2, dtype, grid, 256);
}
int colsum(int dtype, const void* in, long ldi, float* out, long ldo, int B, int HW, int C, float scale, hipStream_t st) {
  ew_rec_begin();
  // (B and HW divide below; B is grid.y)
  if (bad_dtype(dtype) || B < 1 || B > 65535 || HW < 1 || C < 8 || C % 8 || ldi % 8 || ldi < C || ldo < C) return CL_EINVAL;
  if (!in || !out || mis16(in)) return CL_EINVAL;
  int nchunk = (HW + 63) / 64;
  int want = (512 + B - 1) / B;
  if (nchunk > want) nchunk = want;
  const int ppc = (HW + nchunk - 1) / nchunk;
  nchunk = (HW + ppc - 1) / ppc;
  dim3 grid(nchunk, B);
  // block partials through the stream's registered scratch (cl_set_workspace) when there is one; otherwise
  // fp32 atomics straight into out
  void* wsp = nullptr; long wsb = 0;
  gemm_get_workspace_for(st, &wsp, &wsb);
  float* partial = (nchunk > 1 && wsp && (long)B * nchunk * C * 4 <= wsb) ? (float*)wsp : nullptr;
  if (dtype == CL_BF16) hipLaunchKernelGGL((colsum_kernel<bf16_t>), grid, dim3(256), 0, st, (const bf16_t*)in, ldi, out, ldo, HW, C, ppc, scale, partial);
  else hipLaunchKernelGGL((colsum_kernel<float>), grid, dim3(256), 0, st, (const float*)in, ldi, out, ldo, HW, C, ppc, scale, partial);
  if (partial)
    hipLaunchKernelGGL(colsum_finish_kernel, dim3((C + 31) / 32, B), dim3(1024), 0, st, partial, nchunk, C, out, ldo, scale);
  return ew_done(EW_COLSUM, dtype, grid, 256, partial ? 1 : 2, nchunk);
}
int pack2d(int dtype, const float* in, long ldi, void* out, long ldo, long R, int C, int Cpad, hipStream_t st) {
  ew_rec_begin();
  if (bad_dtype(dtype) || R < 0 || C < 0 || Cpad < C || ldo < Cpad || ldi < C) return CL_EINVAL;
  if (R * Cpad > 0 && (!out || (C > 0 && !in))) return CL_EINVAL;
  const dim3 grid(ew_grid(R * Cpad));
  if (dtype == CL_BF16) hipLaunchKernelGGL((pack_kernel<bf16_t>), grid, dim3(256), 0, st, in, ldi, (bf16_t*)out, ldo, R, C, Cpad);
  else hipLaunchKernelGGL((pack_kernel<float>), grid, dim3(256), 0, st, in, ldi, (float*)out, ldo, R, C, Cpad);
  return ew_done(EW_PACK2D, dtype, grid, 256);
}

// ------------------------------------------------------------------ fused re-pack of the trainables
// After every optimizer step the engine needs its storage-dtype copies of the trainable matrices
// (LoRA down/up, zero convs) in both orientations (W for the forward NT product, W^T for the data
// gradient).  Round 0 issued one pack + one transpose launch per matrix (~500 launches / 2.6 ms per
// step); this is ONE launch over a device-resident descriptor table: workgroup -> (matrix, 32x32 tile)
// by binary search in the tile prefix, fp32 tile in, straight and transposed tiles out.
//   desc[i] = {src offset (floats) in the flat master, rows << 32 | cols, dst pointer, dst^T pointer (or 0),
//              src row stride, dst row stride, dst^T row stride (0 = dense), reserved}
template <typename T>
__global__ __launch_bounds__(256) void repack_kernel(const float* __restrict__ flat, const long* __restrict__ desc,
                                                     const int* __restrict__ tile_prefix, int ndesc) {
  __shared__ float tile[32][33];
  int lo = 0, hi = ndesc - 1;
  const int blk = blockIdx.x;
  while (lo < hi) {                       // first matrix whose prefix end exceeds blk
    const int mid = (lo + hi) >> 1;
    if (tile_prefix[mid + 1] > blk) hi = mid; else lo = mid + 1;
  }
  const long* d = desc + (long)lo * 8;
  const long src = d[0];
  const int R = (int)(d[1] >> 32), C = (int)(d[1] & 0xffffffff);
  T* dst = reinterpret_cast<T*>(d[2]);
  T* dstT = reinterpret_cast<T*>(d[3]);
  const long lds_ = d[4] ? d[4] : C, ldd = d[5] ? d[5] : C, ldt = d[6] ? d[6] : R;
  const int t = blk - tile_prefix[lo];
  const int tc = (C + 31) / 32;
  const int r0 = (t / tc) * 32, c0 = (t % tc) * 32;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;   // 32 x 8
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int r = r0 + ty + 8 * i, c = c0 + tx;
    const float v = (r < R && c < C) ? flat[src + (long)r * lds_ + c] : 0.f;
    tile[ty + 8 * i][tx] = v;
    if (dst && r < R && c < C) dst[(long)r * ldd + c] = from_f<T>(v);
  }
  if (!dstT) return;
  __syncthreads();
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int c = c0 + ty + 8 * i, r = r0 + tx;
    if (r < R && c < C) dstT[(long)c * ldt + r] = from_f<T>(tile[tx][ty + 8 * i]);
  }
}

int repack(int dtype, const float* flat, const long* desc, const int* tile_prefix, int ndesc, int total_tiles,
           hipStream_t st) {
  ew_rec_begin();
  if (bad_dtype(dtype)) return CL_EINVAL;
  if (ndesc <= 0 || total_tiles <= 0) return CL_OK;
  if (!flat || !desc || !tile_prefix) return CL_EINVAL;
  const dim3 grid(total_tiles);
  if (dtype == CL_BF16) hipLaunchKernelGGL((repack_kernel<bf16_t>), grid, dim3(256), 0, st, flat, desc, tile_prefix, ndesc);
  else hipLaunchKernelGGL((repack_kernel<float>), grid, dim3(256), 0, st, flat, desc, tile_prefix, ndesc);
  return ew_done(EW_REPACK, dtype, grid, 256);
}

}  // namespace cl
