// mea_kernels.hip -- maximum expected accuracy structures under the motif model (rule in mea_rules.h).
// k_pair_mea runs on the P scratch and PairArgs of k_pair_seq, right behind it on the same stream: one workgroup per sequence,
//   1. the banded table M(i, d), one diagonal d = 1 .. W at a time with the lanes over i (one barrier per diagonal), into the
//      slot's M scratch, with the choice of every cell;
//   2. the exterior chain F(i), i = L-1 .. 0, on the first wave: the lanes over e, a butterfly for the first greatest candidate,
//      F(i+1 .. i+W) in an LDS window of W+1 values;
//   3. the traceback on one lane with an explicit LDS stack, writing '(' ')' '.' at seq_base and the score F(0).
#include <hip/hip_runtime.h>

#include "kernels.h"
#include "mea_rules.h"

namespace elemdp {

constexpr int kWave = 64;

__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
}

__global__ __launch_bounds__(kThreads) void k_pair_mea(PairArgs a) {
  extern __shared__ double s_mea[];   // F window [W+1], then the traceback stack [(W/2 + 2) (i, d) int pairs]
  const int g = blockIdx.x, tid = threadIdx.x;
  const int n = a.idx[g];
  if (a.skip_flagged && a.seq_out[(size_t)n * a.out_stride + 4] != 0.) return;
  const SeqPlan p = a.plans[n];
  const int L = p.L, W = p.W;
  const size_t R = (size_t)(W + 1);
  const uint32_t* ok = a.okbits + p.bits_base;
  const double* P = a.P + (size_t)g * a.p_stride;
  const double* q = a.unpaired + p.seq_base;
  double* M = a.mea_M + (size_t)g * a.p_stride;
  int32_t* ch = a.mea_ch + (size_t)g * a.mea_ch_stride;   // [i][d] choices of M, then the exterior chain's at (L+1)(W+1) + i
  int32_t* chF = ch + (size_t)(L + 1) * R;
  const double gamma2 = a.mea_gamma2;

  // 1. the banded table
  for (int i = tid; i <= L; i += kThreads) M[(size_t)i * R] = 0.;
  __syncthreads();
  for (int d = 1; d <= W; ++d) {
    for (int i = tid; i + d <= L; i += kThreads) {
      double v;
      const int c = mea_band_cell(P, M, q, ok, W, gamma2, i, d, &v);
      M[(size_t)i * R + d] = v;
      ch[(size_t)i * R + d] = c;
    }
    __syncthreads();
  }
  if (tid >= kWave) return;

  // 2. the exterior chain: F(k) at window slot k mod (W+1)
  double* Fw = s_mea;
  const int lane = tid;
  if (lane == 0) Fw[L % (W + 1)] = 0.;
  double F = 0.;
  wave_sync();
  for (int i = L - 1; i >= 0; --i) {
    const int emax = min(W, L - i), base = i % (W + 1);
    const double qi = q[i];
    double best = -HUGE_VAL;
    int be = 0;
    for (int e = 2 + lane; e <= emax; e += kWave) {
      if (!pair_kept(ok, i, e, W)) continue;
      const int k = base + e > W ? base + e - (W + 1) : base + e;
      const double v = mea_pair(gamma2, P[(size_t)i * R + e], M[(size_t)(i + 1) * R + (e - 2)], Fw[k]);
      if (v > best) { best = v; be = e; }
    }
    for (int off = kWave / 2; off > 0; off >>= 1) mea_merge(best, be, __shfl_xor(best, off), __shfl_xor(be, off));
    const int k1 = base + 1 > W ? 0 : base + 1;
    F = Fw[k1] + qi;
    int c = 0;
    if (best > F) { F = best; c = be; }
    wave_sync();   // (every lane has read the window before slot i mod (W+1) = F(i+W+1) is overwritten)
    if (lane == 0) { Fw[base] = F; chF[i] = c; }
    wave_sync();
  }
  if (lane != 0) return;

  // 3. the traceback
  char* s = a.mea_s + p.seq_base;
  int2* stack = reinterpret_cast<int2*>(s_mea + (W + 1));
  const int cap = W / 2 + 2;
  for (int i = 0; i < L;) {
    const int e = chF[i];
    if (e == 0) { s[i++] = '.'; continue; }
    s[i] = '('; s[i + e - 1] = ')';
    int sp = 0;
    int ci = i + 1, cd = e - 2;
    i += e;
    for (;;) {
      if (cd == 0) {
        if (sp == 0) break;
        --sp; ci = stack[sp].x; cd = stack[sp].y;
        continue;
      }
      const int c = ch[(size_t)ci * R + cd];
      if (c == 0) { s[ci] = '.'; ++ci; --cd; continue; }
      s[ci] = '('; s[ci + c - 1] = ')';
      if (cd > c && sp < cap) stack[sp++] = make_int2(ci + c, cd - c);   // (nested intervals of a span <= W: depth < W/2 + 2)
      ci += 1; cd = c - 2;
    }
  }
  a.mea_score[n] = F;
}

size_t pair_mea_lds(int Wmax) { return sizeof(double) * (size_t)(Wmax + 1) + sizeof(int2) * (size_t)(Wmax / 2 + 2); }

hipError_t launch_pair_mea(const PairArgs& a, int G, int Wmax, hipStream_t st) {
  if (G <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_pair_mea, dim3(G), dim3(kThreads), pair_mea_lds(Wmax), st, a);
  return hipGetLastError();
}

}  // namespace elemdp
