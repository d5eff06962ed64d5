// loss_rows.h — the per-row machinery every fused loss kernel shares: the
// TD-target value, the task of a row and its loss weight, the batch-wide
// weight sum in its one fixed association order, the wave sum, the bf16
// store conversion, and the body of the actor/alpha forward+backward kernel
// as a template over the critic head (scalar twin minimum, or the mean of 2M
// quantile atoms).  Included by dsac_kernels.hip and tqc.hip; every function
// is inline or a template, so each translation unit compiles its own copy.
#pragma once

#include <hip/hip_runtime.h>

// twin minimum that keeps a NaN: fminf alone returns the other operand, so
// a poisoned critic output would leave here as a valid number (torch.min
// propagates it).  Every non-NaN pair gives fminf's bits.
__device__ __forceinline__ float dsac_min_nan(float a, float b) {
  return a != a ? a : (b != b ? b : fminf(a, b));
}

// y for one row, with the operation sequence spelled out (one fused
// multiply-add for min - alpha*lp, then two products and a sum) so that
// every kernel that inlines it rounds alike whatever the contraction
// heuristics make of the surrounding code.
__device__ __forceinline__ float td_target_value(float rs, float r,
                                                 float gamma, float d,
                                                 float qmin, float alpha,
                                                 float lp) {
#pragma clang fp contract(off)
  const float x = __builtin_fmaf(-alpha, lp, qmin);
  return rs * r + gamma * (1.f - d) * x;
}

__device__ __forceinline__ int task_of_row(const float* __restrict__ onehot,
                                           long i, int oh_stride, int T) {
  if (T <= 1) return 0;
  int t_i = 0;
  float best = -1e30f;
  for (int t = 0; t < T; ++t) {
    const float v = onehot[i * oh_stride + t];
    if (v > best) { best = v; t_i = t; }
  }
  return t_i;
}

// thread 0 fills smw[0..T) with softmax(-exp(log_alpha)); call before use,
// followed by __syncthreads().
__device__ __forceinline__ void fill_task_weights(
    float* __restrict__ smw, const float* __restrict__ la, int T) {
  if (threadIdx.x == 0) {
    float mx = -1e30f;
    for (int t = 0; t < T; ++t) mx = fmaxf(mx, -__expf(la[t]));
    float den = 0.f;
    for (int t = 0; t < T; ++t) {
      smw[t] = __expf(-__expf(la[t]) - mx);
      den += smw[t];
    }
    for (int t = 0; t < T; ++t) smw[t] /= den;
  }
}

// wavefront sum: 6 DPP/shuffle steps, no LDS, no barrier
__device__ inline float wave_sum64(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

__device__ __forceinline__ unsigned short f32_bf16_rne_d(float f) {
  // native v_cvt_pk_bf16_f32: round to nearest even, and a NaN stays a
  // NaN (the integer rounding add carried some into Inf or zero)
  return __builtin_bit_cast(unsigned short, (__bf16)f);
}

// Batch-wide sum of the per-row task weights — the wsum that the last block
// of k_*_loss_fwd_mb finalizes — recomputed by EVERY block so the backward
// coefficient needs no wait on other blocks.  Association order is the
// multi-block forward's at grid = ceil(B/256) <= 32: one row per thread,
// wave_sum64, the four wave partials left to right, blocks in index order.
// The one-hot scan runs t-outer over KR blocks' rows so its loads overlap;
// own_t receives the task of this thread's own row (blockIdx.x*256 + tid).
// Ends with a barrier; wpart may be reused afterwards.
struct __attribute__((packed, aligned(4))) OneHot4 { float v[4]; };
struct __attribute__((packed, aligned(4))) OneHot2 { float v[2]; };

__device__ __forceinline__ float batch_weight_sum(
    const float* __restrict__ smw, const float* __restrict__ onehot,
    float (*wpart)[4], int B, int T, int oh_stride, int nblk, int& own_t) {
  const int tid = threadIdx.x, wid = tid >> 6, lane = tid & 63;
  constexpr int KR = 8;
  for (int b0 = 0; b0 < nblk; b0 += KR) {
    float best[KR];
    int ti[KR];
    long row[KR];
#pragma unroll
    for (int k = 0; k < KR; ++k) {
      const int i = (b0 + k) * 256 + tid;
      row[k] = (long)(i < B ? i : B - 1);
      best[k] = -1e30f;
      ti[k] = 0;
    }
    if (T > 1) {
      // a lane's row is its own cache line, so a load instruction costs the
      // address path 64 lines whatever its width: read four (then two, then
      // one) tasks per load.  The suffix is only 4-byte aligned.
      int t = 0;
#pragma unroll 2
      for (; t + 4 <= T; t += 4) {
#pragma unroll
        for (int k = 0; k < KR; ++k) {
          const OneHot4 q = *reinterpret_cast<const OneHot4*>(
              onehot + row[k] * oh_stride + t);
#pragma unroll
          for (int c = 0; c < 4; ++c)
            if (q.v[c] > best[k]) { best[k] = q.v[c]; ti[k] = t + c; }
        }
      }
      if (t + 2 <= T) {
#pragma unroll
        for (int k = 0; k < KR; ++k) {
          const OneHot2 q = *reinterpret_cast<const OneHot2*>(
              onehot + row[k] * oh_stride + t);
#pragma unroll
          for (int c = 0; c < 2; ++c)
            if (q.v[c] > best[k]) { best[k] = q.v[c]; ti[k] = t + c; }
        }
        t += 2;
      }
      if (t < T) {
#pragma unroll
        for (int k = 0; k < KR; ++k) {
          const float v = onehot[row[k] * oh_stride + t];
          if (v > best[k]) { best[k] = v; ti[k] = t; }
        }
      }
    }
    // the KR wave sums step together so their shuffles pipeline; each is
    // the wave_sum64 sequence (rows past B and blocks past nblk add 0)
    float w[KR];
#pragma unroll
    for (int k = 0; k < KR; ++k) {
      const int i = (b0 + k) * 256 + tid;
      w[k] = i < B ? smw[ti[k]] : 0.f;
      if (b0 + k == (int)blockIdx.x) own_t = ti[k];
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
      for (int k = 0; k < KR; ++k) w[k] += __shfl_xor(w[k], off, 64);
    }
#pragma unroll
    for (int k = 0; k < KR; ++k)
      if (lane == 0 && b0 + k < nblk) wpart[b0 + k][wid] = w[k];
  }
  __syncthreads();
  float r = 0.f;
  for (int b = 0; b < nblk; ++b)
    r += wpart[b][0] + wpart[b][1] + wpart[b][2] + wpart[b][3];
  return r;
}

// K6 actor/alpha forward + backward in one launch (k_actor_alpha_loss_fwd_mb
// + the workspace path of k_actor_alpha_loss_bwd2).  ws = ticket, 32*4
// metric slots, then gridDim*T alpha-gradient slots; ONE ticket serves both
// finalizations.  dla[0..T) is stored as 0.f + r (the replaced pair zeroes
// it and then adds r), dla[T..dla_n) as 0.f.  grid = ceil(B/256) <= 32.
//
// QUANT = false: aq1/aq2 are [B], Q = min(aq1, aq2), daq [2, B] carries the
// whole dL/dQ at the smaller head.  QUANT = true (truncated quantile
// critics): aq1/aq2 are [B, M], Q = the mean of the row's 2M atoms (aq1's
// left to right, then aq2's, one division), daq [2, B, M] carries
// dL/dQ / (2M) in every atom.  Everything else is shared.
//
// The body of both kernels, inlined into a plain __global__ wrapper in each
// file (k_actor_alpha_loss_fwd_bwd, k_tqc_actor_alpha_loss_fwd_bwd), so the
// scalar kernel keeps its signature and its place in the code object.
template <bool QUANT>
__device__ __forceinline__ void actor_alpha_loss_fwd_bwd_body(
    const float* __restrict__ aq1, const float* __restrict__ aq2,
    const float* __restrict__ lp, const float* __restrict__ ls,
    const float* __restrict__ onehot, const float* __restrict__ log_alpha,
    float* __restrict__ out, float* __restrict__ ws,
    unsigned short* __restrict__ daq, float* __restrict__ dlp,
    float* __restrict__ dla, int dla_n, const float* __restrict__ wsum_in,
    int B, int T, int A, int oh_stride, int use_w, float H_bar, int M) {
  __shared__ float part[4][4];
  __shared__ float smw[32];
  __shared__ float wpart[32][4];
  __shared__ float s_val[256];
  __shared__ int s_t[256];
  __shared__ int s_last;
  __shared__ float s_fin[32 * 4];
  __shared__ float s_g[32 * 32];
  const int tid = threadIdx.x;
  constexpr float CE = 1.4189385332046727f;  // 0.5*(1+log(2*pi))
  const int i = blockIdx.x * 256 + tid;
  // the row's operands first (row clamped, so the loads are unconditional
  // and in flight during the weight-sum recompute)
  const long ic = i < B ? i : B - 1;
  float aq1v, aq2v;
  if (QUANT) {
    // all 2M loads in flight before the first add (M <= 32; an atom past M
    // re-reads the last one and is not added)
    float v1[32], v2[32];
#pragma unroll
    for (int m = 0; m < 32; ++m) {
      const int mc = m < M ? m : M - 1;
      v1[m] = aq1[ic * M + mc];
      v2[m] = aq2[ic * M + mc];
    }
    float s = 0.f;
#pragma unroll
    for (int m = 0; m < 32; ++m) if (m < M) s += v1[m];
#pragma unroll
    for (int m = 0; m < 32; ++m) if (m < M) s += v2[m];
    aq1v = aq2v = s / (float)(2 * M);
  } else {
    aq1v = aq1[ic]; aq2v = aq2[ic];
  }
  const float lpv = lp[ic];
  float ent = CE * A;
  for (int a = 0; a < A; ++a) ent += ls[ic * A + a];
  int t_i = 0;
  float wsum = 1.f;
  if (use_w) {
    fill_task_weights(smw, log_alpha, T);
    __syncthreads();
  }
  if (use_w && wsum_in == nullptr) {
    wsum = batch_weight_sum(smw, onehot, wpart, B, T, oh_stride,
                            (int)gridDim.x, t_i);
  } else {
    // wsum_in: the same sum, already finalized by a critic-loss kernel of
    // this update over the same one-hots and log_alpha
    if (use_w) wsum = wsum_in[0];
    t_i = task_of_row(onehot, ic, oh_stride, T);
  }
  float s_pl = 0.f, s_w = 0.f, s_al = 0.f, s_en = 0.f;
  s_t[tid] = -1;
  s_val[tid] = 0.f;
  if (i < B) {
    s_t[tid] = t_i;
    s_val[tid] = -(lpv + H_bar) / (float)B;
    const float la = log_alpha[t_i];
    const float alpha_i = __expf(la);
    const float w_raw = use_w ? smw[t_i] : 1.f;
    s_w += w_raw;
    const float qmin = QUANT ? aq1v : dsac_min_nan(aq1v, aq2v);
    s_pl += w_raw * -(qmin - alpha_i * lpv);
    s_al += la * (lpv + H_bar);
    s_en += ent;
    const float coeff = (use_w ? w_raw / wsum : 1.f) / (float)B;
    if (QUANT) {
      const unsigned short g = f32_bf16_rne_d(coeff * -1.f / (float)(2 * M));
      for (int m = 0; m < M; ++m) {
        daq[(long)i * M + m] = g;
        daq[((long)B + i) * M + m] = g;
      }
    } else {
      const bool first = aq1v <= aq2v;
      daq[i] = f32_bf16_rne_d(first ? coeff * -1.f : 0.f);
      daq[B + i] = f32_bf16_rne_d(first ? 0.f : coeff * -1.f);
    }
    dlp[i] = coeff * alpha_i;
  }
  s_pl = wave_sum64(s_pl); s_w = wave_sum64(s_w);
  s_al = wave_sum64(s_al); s_en = wave_sum64(s_en);
  const int wid = tid >> 6, lane = tid & 63;
  if (lane == 0) {
    part[0][wid] = s_pl; part[1][wid] = s_w;
    part[2][wid] = s_al; part[3][wid] = s_en;
  }
  __syncthreads();
  float* mslots = ws + 1;
  float* gslots = ws + 1 + 32 * 4;
  // per-task sums of this block's 256 rows, as k_actor_alpha_loss_bwd2:
  // wave w takes tasks w, w+4, ...; four at a time so the shuffles pipeline
  for (int t0 = wid; t0 < T; t0 += 16) {
    float v[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int t = t0 + 4 * j;   // t >= T matches no row: v = 0, not stored
      v[j] = ((s_t[lane] == t ? s_val[lane] : 0.f) +
              (s_t[lane + 64] == t ? s_val[lane + 64] : 0.f)) +
             ((s_t[lane + 128] == t ? s_val[lane + 128] : 0.f) +
              (s_t[lane + 192] == t ? s_val[lane + 192] : 0.f));
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
      for (int j = 0; j < 4; ++j) v[j] += __shfl_xor(v[j], off, 64);
    }
    if (lane == 0) {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (t0 + 4 * j < T) gslots[(long)blockIdx.x * T + t0 + 4 * j] = v[j];
      __threadfence();
    }
  }
  __syncthreads();
  if (tid == 0) {
#pragma unroll
    for (int k = 0; k < 4; ++k)
      mslots[blockIdx.x * 4 + k] =
          part[k][0] + part[k][1] + part[k][2] + part[k][3];
    __threadfence();
    const unsigned old = atomicAdd((unsigned*)ws, 1u);
    s_last = (old == (unsigned)gridDim.x - 1u);
    if (s_last) { *(unsigned*)ws = 0u; __threadfence(); }
  }
  __syncthreads();
  if (!s_last) return;
  // last block: parallel reads of every slot into LDS (a serial scan costs
  // a memory round trip per slot), then the sums in block order
  const int nb = (int)gridDim.x;
  if (tid < nb * 4) s_fin[tid] = ((const volatile float*)mslots)[tid];
  for (int k = tid; k < nb * T; k += 256)
    s_g[k] = ((const volatile float*)gslots)[k];
  __syncthreads();
  if (tid < dla_n) {
    float g = 0.f;
    if (tid < T) {
      float rsum = 0.f;
      for (int b = 0; b < nb; ++b) rsum += s_g[b * T + tid];
      g = 0.f + rsum;
    }
    dla[tid] = g;
  }
  if (tid == 0) {
    float r0 = 0.f, r1 = 0.f, r2 = 0.f, r3 = 0.f;
    for (int b = 0; b < nb; ++b) {
      r0 += s_fin[b * 4 + 0]; r1 += s_fin[b * 4 + 1];
      r2 += s_fin[b * 4 + 2]; r3 += s_fin[b * 4 + 3];
    }
    const float wfin = use_w ? r1 : 1.f;
    out[4] = r0; out[5] = r1; out[6] = r2; out[7] = r3;
    out[0] = r0 / (wfin * (float)B);
    out[1] = wfin;
    out[2] = -r2 / (float)B;
    out[3] = r3 / (float)B;
  }
}
