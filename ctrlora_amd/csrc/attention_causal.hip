// Causal self-attention forward for short sequences (CLIP text: d_head 64, N <= 128 tokens).
//
//   O[b, i, h] = softmax_{j <= i}(scale q_i . k_j) v_j        (transformers/models/clip/modeling_clip.py: CLIPTextTransformer
//                                                              builds the causal mask, CLIPAttention adds it to the scores)
//
// One workgroup of four waves per (64-query block r, head, sample); wave w owns query rows r 64 + 16 w .. + 15.  A head's K and
// V of 128 tokens are 16 KB each in bf16 (32 KB in fp32), so the workgroup stages every key it needs ONCE -- keys [0, 64 (r + 1)):
// block r visits key tiles 0 .. r only -- K row-major and V transposed (a plain transposing LDS write: the staging is a few KB
// and not a hot path), rows and keys >= N as zeros.  There is no key loop and no online rescaling: the whole score row of a
// query (at most 128 keys = 8 accumulator fragments) lives in registers.
//
// Matrix layouts (mma.h): S^T = K Q^T, so a lane holds ONE query (lane & 15) and keys 16 f + 4 (lane >> 4) + {0..3} of fragment
// f: the row maximum and sum are two butterflies over the lane groups, and the accumulator IS the B operand of O^T = V^T P^T
// (PFrag).  Key fragments wholly above a wave's diagonal (f > 4 r + w) are skipped, wave-uniformly; the others are masked per
// element (key > query -> -inf) BEFORE the row maximum.  Every query row sees its own diagonal key, so no row is empty: no NaN
// guard.  Keys >= N lie above the diagonal of every stored row (i < N): the causal mask itself excludes them.  Query rows >= N
// compute on zeros and are not stored.
//
// Roundings: scores, maximum, exponentials and the denominator (the sum of the UNROUNDED exponentials) are fp32; the
// unnormalised P = 2^(s - max) is rounded to the compute type before P V, as in the other attention kernels; O = (P V) / sum is
// rounded once on the store.
#include "attn_common.h"

namespace cl {

namespace {

constexpr int CA_DH = 64, CA_THREADS = 256;

template <typename T, int NT> struct CausalGeom {
  static constexpr int EB = AttnTraits<T>::EB;
  static constexpr int E16 = 16 / EB;                  // elements per 16-byte chunk
  static constexpr int NK = 64 * NT;                   // keys the LDS image has room for
  static constexpr int KROW = CA_DH * EB + 16;         // bytes per staged K row (+16: consecutive rows start 4 banks apart)
  static constexpr int VROW = NK * EB + 16;            // bytes per V^T row (one d, NK keys)
  static constexpr int LDS = NK * KROW + CA_DH * VROW;
};

template <typename T, int NT>
__global__ __launch_bounds__(CA_THREADS) void attn_causal_kernel(const T* __restrict__ Q, long ldq, const T* __restrict__ K, long ldk,
                                                                 const T* __restrict__ V, long ldv, T* __restrict__ O, long ldo, int N,
                                                                 float c) {
  using G = CausalGeom<T, NT>;
  constexpr int EB = G::EB, E16 = G::E16, NK = G::NK, KROW = G::KROW, VROW = G::VROW;
  constexpr int KS = Mma<T>::K;                        // contraction length of one matrix step: 32 (bf16) / 16 (fp32)
  constexpr int NF = NK / 16;                          // score fragments (16 keys each)
  constexpr int FR = PFrag<T>::FRAGS;                  // score fragments per P V step
  constexpr int QSTEPS = CA_DH / KS, PSTEPS = NK / KS, CPR = CA_DH / E16;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* sK = smem;
  char* sV = smem + NK * KROW;

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int g = lane >> 4, c16 = lane & 15;
  const int r = blockIdx.x, h = blockIdx.y, b = blockIdx.z;
  const long row0 = (long)b * N;
  const T* Kb = K + row0 * ldk + h * CA_DH;
  const T* Vb = V + row0 * ldv + h * CA_DH;

  // stage keys [0, 64 (r + 1)): K row-major, V transposed; keys >= N as zeros
  const int nstage = 64 * (r + 1);
  for (int i = tid; i < nstage * CPR; i += CA_THREADS) {
    const int key = i / CPR, ch = i - key * CPR;
    u32x4_t kv = {0u, 0u, 0u, 0u}, vv = {0u, 0u, 0u, 0u};
    if (key < N) {
      kv = *reinterpret_cast<const u32x4_t*>(Kb + (long)key * ldk + ch * E16);
      vv = *reinterpret_cast<const u32x4_t*>(Vb + (long)key * ldv + ch * E16);
    }
    *reinterpret_cast<u32x4_t*>(sK + key * KROW + ch * 16) = kv;
    T ve[E16];
    __builtin_memcpy(ve, &vv, 16);
#pragma unroll
    for (int j = 0; j < E16; ++j) reinterpret_cast<T*>(sV + (ch * E16 + j) * VROW)[key] = ve[j];
  }

  // this lane's query row as the B operand of S^T = K Q^T: d chunk s KS + g E16 of step s
  const int q0 = 64 * r + 16 * wave;                   // first query row of the wave
  const int qi = q0 + c16;
  u32x4_t qf[QSTEPS];
#pragma unroll
  for (int s = 0; s < QSTEPS; ++s) {
    qf[s] = u32x4_t{0u, 0u, 0u, 0u};
    if (qi < N) qf[s] = *reinterpret_cast<const u32x4_t*>(Q + (row0 + qi) * ldq + h * CA_DH + s * KS + g * E16);
  }
  __syncthreads();

  // scores: fragment f holds keys 16 f + 4 g + {0..3} of query qi; fragments above the wave's diagonal stay at p = 0
  const int fdiag = 4 * r + wave;
  f32x4_t p[NF];
  float mx = -INFINITY;
#pragma unroll
  for (int f = 0; f < NF; ++f) {
    p[f] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    if (f <= fdiag) {
#pragma unroll
      for (int s = 0; s < QSTEPS; ++s) {
        const u32x4_t a = *reinterpret_cast<const u32x4_t*>(sK + (f * 16 + c16) * KROW + (s * KS + g * E16) * EB);
        Mma<T>::run(a, qf[s], p[f]);
      }
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int key = f * 16 + 4 * g + e;
        p[f][e] = key <= qi ? p[f][e] * c : -INFINITY;
        mx = fmaxf(mx, p[f][e]);
      }
    }
  }
  mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
  mx = fmaxf(mx, __shfl_xor(mx, 32, 64));              // finite: key 0 <= qi in the g = 0 lane of every query
  float sum = 0.f;
#pragma unroll
  for (int f = 0; f < NF; ++f) {
    if (f <= fdiag) {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        p[f][e] = exp2f(p[f][e] - mx);
        sum += p[f][e];
      }
    }
  }
  sum += __shfl_xor(sum, 16, 64);
  sum += __shfl_xor(sum, 32, 64);

  // O^T = V^T P^T: A = V^T rows (d = 16 df + c16), keys as PFrag groups them; P rounded to T here
  u32x4_t pb[PSTEPS];
#pragma unroll
  for (int st = 0; st < PSTEPS; ++st) pb[st] = PFrag<T>::make(&p[st * FR]);
  T* Ob = O + (row0 + qi) * ldo + h * CA_DH;
#pragma unroll
  for (int df = 0; df < CA_DH / 16; ++df) {
    f32x4_t acc = {0.f, 0.f, 0.f, 0.f};
    const char* vrow = sV + (df * 16 + c16) * VROW;
#pragma unroll
    for (int st = 0; st < PSTEPS; ++st) {
      if (st * KS <= q0 + 15) {                        // (wave-uniform) later keys carry p = 0 for every query of the wave
        u32x4_t a;
        if constexpr (EB == 2) {
          const u32x2_t lo = *reinterpret_cast<const u32x2_t*>(vrow + (st * 32 + 4 * g) * 2);
          const u32x2_t hi = *reinterpret_cast<const u32x2_t*>(vrow + (st * 32 + 16 + 4 * g) * 2);
          a = u32x4_t{lo.x, lo.y, hi.x, hi.y};
        } else {
          a = *reinterpret_cast<const u32x4_t*>(vrow + (st * 16 + 4 * g) * 4);
        }
        Mma<T>::run(a, pb[st], acc);
      }
    }
    if (qi < N) {
      float o[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) o[e] = acc[e] / sum;
      store4(Ob + df * 16 + 4 * g, o);
    }
  }
}

template <typename T, int NT>
int launch_causal(const void* Q, long ldq, const void* K, long ldk, const void* V, long ldv, void* O, long ldo, int B, int H, int N,
                  float scale, hipStream_t st) {
  using G = CausalGeom<T, NT>;
  auto kern = &attn_causal_kernel<T, NT>;
  static bool lds_raised = false;                      // once per kernel: the first forward of an executor runs eagerly, captures later
  if (G::LDS > 65536 && !lds_raised) {
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, G::LDS) != hipSuccess) {
      g_last_hip_error = (int)hipGetLastError();
      return CL_ELAUNCH;
    }
    lds_raised = true;
  }
  hipLaunchKernelGGL(kern, dim3(NT, H, B), dim3(CA_THREADS), G::LDS, st, (const T*)Q, ldq, (const T*)K, ldk, (const T*)V, ldv, (T*)O, ldo, N,
                     scale * 1.4426950408889634f);
  return CL_OK;
}

inline bool mis16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) != 0; }

}  // namespace

int attn_causal_fwd(int dtype, const void* Q, long ldq, const void* K, long ldk, const void* V, long ldv, void* O, long ldo, int B, int H,
                    int N, int dh, float scale, hipStream_t st) {
  if ((dtype != CL_BF16 && dtype != CL_F32) || !Q || !K || !V || !O) return CL_EINVAL;
  if (dh != CA_DH || N < 1 || N > 128 || B < 1 || B > 65535 || H < 1 || H > 65535) return CL_EINVAL;
  const long eb = dtype == CL_BF16 ? 2 : 4, inner = (long)H * dh;
  for (long ldx : {ldq, ldk, ldv, ldo})
    if (ldx < inner || (ldx * eb) % 16) return CL_EINVAL;
  if (mis16(Q) || mis16(K) || mis16(V) || mis16(O)) return CL_EINVAL;
  const int nt = (N + 63) / 64;
  int rc;
  if (dtype == CL_BF16) rc = nt == 1 ? launch_causal<bf16_t, 1>(Q, ldq, K, ldk, V, ldv, O, ldo, B, H, N, scale, st)
                                     : launch_causal<bf16_t, 2>(Q, ldq, K, ldk, V, ldv, O, ldo, B, H, N, scale, st);
  else rc = nt == 1 ? launch_causal<float, 1>(Q, ldq, K, ldk, V, ldv, O, ldo, B, H, N, scale, st)
                    : launch_causal<float, 2>(Q, ldq, K, ldk, V, ldv, O, ldo, B, H, N, scale, st);
  if (rc != CL_OK) return rc;
  attn_rec(1, ATTN_FAM_CAUSAL, dtype, dh);
  g_attn_last.fwd_frags = 1; g_attn_last.grid_fwd = nt * H * B;
  CL_CHECK_LAUNCH();
  return CL_OK;
}

}  // namespace cl
