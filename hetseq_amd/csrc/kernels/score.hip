// Validation scoring of the pre-training heads: masked-LM loss / top-1 / top-k and NSP loss /
// accuracy from the logits the fused head already produced, read from HBM once.
//
// Row kernel: one block per fp32 logit row (256 threads, 64 when V < 1024: xent.hip's rule).  The
// label's logit x[lab] is read first (block-uniform); one pass over the row then keeps the online
// (max, sum-exp) of xent.hip -- loss = lse - x[lab] -- and counts
//   rank = #{j : x[j] > x[lab]} + #{j < lab : x[j] == x[lab]},
// the label's position in a stable descending sort (ties go to the lowest index), so top-k is
// rank < k.  Rows whose label is ignored (== ignore, < 0, >= V) leave before any barrier with
// loss 0, rank -1.  Columns V..ldv are never read.
// Reduce kernel: one block sums the row losses in fp64, counts the labelled / rank 0 / rank < k
// rows, scores the [B, 2] NSP rows, and ADDS the eight sums into a persistent device accumulator
//   acc[8] = {mlm_loss_sum, mlm_n, mlm_top1, mlm_topk, nsp_loss_sum, nsp_n, nsp_correct, nsentences}
// in a fixed order (no atomics: the same inputs give the same bits), so a validation pass
// accumulates every batch on the device and reads the result once.
#include "common.h"

namespace hs {

// one logit against the label's: it sorts before the label when greater, or equal at a lower index
HS_DEVICE int score_before(float v, float xl, int idx, int lab) { return (idx < lab ? v >= xl : v > xl) ? 1 : 0; }

HS_DEVICE void score_one(float v, float xl, int idx, int lab, float& m, float& s, int& c) {
  if (v > m) {
    s = s * __expf(m - v) + 1.f;
    m = v;
  } else {
    s += __expf(v - m);
  }
  c += score_before(v, xl, idx, lab);
}

HS_DEVICE int wave_count(bool p) { return __popcll(__ballot(p)); }

// Four logits of lane-consecutive quads (lane l of the wave holds elements ia .. ia + 3, ia = the first
// active lane's + 4 per lane).  The count costs one compare per element: a wave whose 256 elements all lie
// before the label (or all after it) counts v >= x[lab] (v > x[lab]) with the compare's lane mask and a
// scalar population count into the wave-uniform cw; only the one wave holding the label takes the
// per-element rule, into the lane's own c.
HS_DEVICE void score_quad(const float4 a, float xl, int ia, int lab, float& m, float& s, int& c, int& cw) {
  const float mq = fmaxf(fmaxf(a.x, a.y), fmaxf(a.z, a.w));
  if (mq > m) {
    s *= __expf(m - mq);  // (m = -inf at the start: s = 0)
    m = mq;
  }
  s += (__expf(a.x - m) + __expf(a.y - m)) + (__expf(a.z - m) + __expf(a.w - m));
  const int base = __builtin_amdgcn_readfirstlane(ia);  // the lowest element index among the active lanes
  if (base + 255 < lab) {
    cw += (wave_count(a.x >= xl) + wave_count(a.y >= xl)) + (wave_count(a.z >= xl) + wave_count(a.w >= xl));
  } else if (base > lab) {
    cw += (wave_count(a.x > xl) + wave_count(a.y > xl)) + (wave_count(a.z > xl) + wave_count(a.w > xl));
  } else {
    c += (score_before(a.x, xl, ia, lab) + score_before(a.y, xl, ia + 1, lab)) +
         (score_before(a.z, xl, ia + 2, lab) + score_before(a.w, xl, ia + 3, lab));
  }
}

// the block's (max, sum-exp, count) combined through LDS (xent.hip's cross-wave reduction); thread 0
// writes the row's loss and rank.  c: per-lane counts; cw: a count the whole wave already shares.
HS_DEVICE void score_finish(float m, float s, int c, int cw, float xl, int row, float* __restrict__ row_loss,
                            int32_t* __restrict__ rank) {
  __shared__ float sm[4], ss[4];
  __shared__ int sc[4];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float m2 = __shfl_xor(m, o, 64), s2 = __shfl_xor(s, o, 64);
    const float mm = fmaxf(m, m2);
    s = (m == -INFINITY ? 0.f : s * __expf(m - mm)) + (m2 == -INFINITY ? 0.f : s2 * __expf(m2 - mm));
    m = mm;
    c += __shfl_xor(c, o, 64);
  }
  if (lane == 0) {
    sm[w] = m;
    ss[w] = s;
    sc[w] = c + cw;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    const int nw = (int)(blockDim.x >> 6);
    float M = sm[0];
    for (int i = 1; i < nw; ++i) M = fmaxf(M, sm[i]);
    float Ssum = 0.f;
    int C = 0;
    for (int i = 0; i < nw; ++i) {
      Ssum += ss[i] * __expf(sm[i] - M);
      C += sc[i];
    }
    row_loss[row] = M + __logf(Ssum) - xl;
    rank[row] = C;
  }
}

// an ignored label: the whole block leaves (block-uniform, before any barrier)
HS_DEVICE bool score_ignored(int64_t lab, int V, int ignore, int row, float* __restrict__ row_loss,
                             int32_t* __restrict__ rank) {
  if (!(lab == ignore || lab < 0 || lab >= V)) return false;
  if (threadIdx.x == 0) {
    row_loss[row] = 0.f;
    rank[row] = -1;
  }
  return true;
}

__global__ void __launch_bounds__(256) score_row_kernel(const float* __restrict__ logits,
                                                        const int64_t* __restrict__ labels, int V, int64_t ldv,
                                                        int ignore, float* __restrict__ row_loss,
                                                        int32_t* __restrict__ rank) {
  const int row = blockIdx.x;
  const int64_t lab64 = labels[row];
  if (score_ignored(lab64, V, ignore, row, row_loss, rank)) return;
  const int lab = (int)lab64;
  const float* x = logits + (int64_t)row * ldv;
  const float xl = x[lab];
  float m = -INFINITY, s = 0.f;
  int c = 0;
  for (int i = threadIdx.x; i < V; i += blockDim.x) score_one(x[i], xl, i, lab, m, s, c);
  score_finish(m, s, c, 0, xl, row, row_loss, rank);
}

// fp32 rows with 16-B aligned starts (ldv % 4 == 0): float4 loads, two independent (max, sum) chains
// per thread as in xent_fwd_vec_kernel, the last V % 4 elements one per thread
__global__ void __launch_bounds__(256) score_row_vec_kernel(const float* __restrict__ logits,
                                                            const int64_t* __restrict__ labels, int V, int64_t ldv,
                                                            int ignore, float* __restrict__ row_loss,
                                                            int32_t* __restrict__ rank) {
  const int row = blockIdx.x;
  const int64_t lab64 = labels[row];
  if (score_ignored(lab64, V, ignore, row, row_loss, rank)) return;
  const int lab = (int)lab64;
  const float* x = logits + (int64_t)row * ldv;
  const float4* x4 = reinterpret_cast<const float4*>(x);
  const float xl = x[lab];
  const int n4 = V >> 2, bd = blockDim.x;
  float m0 = -INFINITY, s0 = 0.f, m1 = -INFINITY, s1 = 0.f;
  int c0 = 0, c1 = 0, cw = 0;
  // Four 16-byte loads in flight per lane and iteration (a row's block is latency-bound: 640 rows are
  // 2.5 blocks per CU).  cw is read from lane 0 of each wave, so lane 0 takes part in every score_quad
  // its wave runs: the main loop runs whole waves only (the bound is the wave's last lane's), and in
  // the four tail quads the active lanes are a prefix of the wave (after the loop iw + 4 * bd > n4:
  // nothing else is left)
  const int lane = threadIdx.x & 63;
  int i = threadIdx.x;
  for (; (i - lane) + 63 + 3 * bd < n4; i += 4 * bd) {
    const float4 a = x4[i], b = x4[i + bd], c = x4[i + 2 * bd], d = x4[i + 3 * bd];
    score_quad(a, xl, 4 * i, lab, m0, s0, c0, cw);
    score_quad(b, xl, 4 * (i + bd), lab, m1, s1, c1, cw);
    score_quad(c, xl, 4 * (i + 2 * bd), lab, m0, s0, c0, cw);
    score_quad(d, xl, 4 * (i + 3 * bd), lab, m1, s1, c1, cw);
  }
  if (i < n4) score_quad(x4[i], xl, 4 * i, lab, m0, s0, c0, cw);
  if (i + bd < n4) score_quad(x4[i + bd], xl, 4 * (i + bd), lab, m1, s1, c1, cw);
  if (i + 2 * bd < n4) score_quad(x4[i + 2 * bd], xl, 4 * (i + 2 * bd), lab, m0, s0, c0, cw);
  if (i + 3 * bd < n4) score_quad(x4[i + 3 * bd], xl, 4 * (i + 3 * bd), lab, m1, s1, c1, cw);
  const int t = (n4 << 2) + threadIdx.x;  // the last V % 4 elements
  if (t < V) score_one(x[t], xl, t, lab, m1, s1, c1);
  const float m = fmaxf(m0, m1);
  const float s = (m0 == -INFINITY ? 0.f : s0 * __expf(m0 - m)) + (m1 == -INFINITY ? 0.f : s1 * __expf(m1 - m));
  score_finish(m, s, c0 + c1, cw, xl, row, row_loss, rank);
}

// eight doubles per thread summed over the block in a fixed order (wave shuffles, then the waves
// through LDS), added into acc by thread 0
__global__ void __launch_bounds__(256) score_reduce_kernel(const float* __restrict__ row_loss,
                                                           const int32_t* __restrict__ rank, int rows, int k,
                                                           const float* __restrict__ nsp_logits,
                                                           const int64_t* __restrict__ nsp_labels, int B,
                                                           double* __restrict__ acc) {
  double v[8] = {0., 0., 0., 0., 0., 0., 0., 0.};
  for (int i = threadIdx.x; i < rows; i += blockDim.x) {
    const int r = rank[i];
    if (r >= 0) {
      v[0] += (double)row_loss[i];
      v[1] += 1.;
      v[2] += r == 0 ? 1. : 0.;
      v[3] += r < k ? 1. : 0.;
    }
  }
  for (int b = threadIdx.x; b < B; b += blockDim.x) {
    const float x0 = nsp_logits[2 * b], x1 = nsp_logits[2 * b + 1];
    const int64_t lab = nsp_labels[b];
    v[7] += 1.;
    if (lab == 0 || lab == 1) {
      const float m = fmaxf(x0, x1);
      const float lse = m + logf(expf(x0 - m) + expf(x1 - m));
      v[4] += (double)(lse - (lab == 0 ? x0 : x1));
      v[5] += 1.;
      v[6] += (x1 > x0 ? 1 : 0) == (int)lab ? 1. : 0.;  // the lowest-index argmax
    }
  }
  __shared__ double red[4][8];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const double t = wave_sum_d(v[j]);
    if (lane == 0) red[w][j] = t;
  }
  __syncthreads();
  if (threadIdx.x < 8) {
    double t = 0.;
    for (int i = 0; i < (int)(blockDim.x >> 6); ++i) t += red[i][threadIdx.x];
    acc[threadIdx.x] += t;
  }
}

}  // namespace hs

using namespace hs;

// dtype 0 (fp32 logits) only; -1 otherwise (the caller scores those in torch).  row_loss / rank:
// [rows] scratch the row kernel fills and the reduce kernel reads.
int launch_mlm_nsp_score(int dtype, const void* logits, const int64_t* labels, int rows, int V, int64_t ldv, int ignore,
                         int k, const float* nsp_logits, const int64_t* nsp_labels, int B, float* row_loss,
                         int32_t* rank, double* acc, hipStream_t st) {
  if (dtype != 0) return -1;
  if (rows > 0) {
    const int threads = V >= 1024 ? 256 : 64;
    const bool vec = threads == 256 && ldv % 4 == 0 && (reinterpret_cast<uintptr_t>(logits) & 15) == 0;
    if (vec)
      hipLaunchKernelGGL(score_row_vec_kernel, dim3(rows), dim3(threads), 0, st, (const float*)logits, labels, V, ldv,
                         ignore, row_loss, rank);
    else
      hipLaunchKernelGGL(score_row_kernel, dim3(rows), dim3(threads), 0, st, (const float*)logits, labels, V, ldv,
                         ignore, row_loss, rank);
  }
  if (rows > 0 || B > 0)
    hipLaunchKernelGGL(score_reduce_kernel, dim3(1), dim3(256), 0, st, row_loss, rank, rows < 0 ? 0 : rows, k,
                       nsp_logits, nsp_labels, B < 0 ? 0 : B, acc);
  return 0;
}
