// ln_chain.hip — whole-chain kernels for LayerNorm MLPs (gfx950): every
// hidden layer is Linear -> LayerNorm(gamma, beta, biased variance) -> ReLU,
// the output layer is linear (docs/KERNELS.md "LayerNorm critics"; the
// oracle is torch_ref.ln_mlp_forward).
//
// A workgroup of the chain kernels owns 16 COMPLETE rows of every hidden
// activation, so the row statistics of LayerNorm need no traffic between
// workgroups and no launch of their own.  The GEMM part is the packed 16-wave
// pair mapping of k_bf16_chain_fwd_pipe / _dx_pipe (packed_kloop<2, 4> over
// the fragment-packed mirrors pack_weights_frag writes); what is new is what
// happens between two GEMMs.
//
// LDS (99,328 B of gfx950's 160 KB): the two bf16 activation buffers
// [2][16][CPAD] of the ReLU chain (49,664 B) plus ONE fp32 staging tile
// [16][CPAD] (49,664 B).  MFMA accumulators are spread over waves by column
// tile; the statistics run along rows.  The epilogue therefore writes the
// fp32 pre-norm values (never rounded to bf16) to the staging tile, and after
// the layer barrier the work is re-dealt BY ROW: wave w owns row w, lane l the
// columns l, l + 64, ... (<= 12 values, held in registers).  Waves that own
// no column tile of a layer (3 of 16 at width 400) still own a row.
//
// k_bf16_chain_ln_fwd, row phase of a hidden layer of width N:
//   mu = sum z / N, then var = sum (z - mu)^2 / N — two passes over the
//   registers, each a per-lane sum in column order and a 6-step xor butterfly
//   (every lane ends with the same bits); rstd = 1 / sqrt(var + eps);
//   xhat = (z - mu) rstd; h = relu(xhat gamma + beta).  Only columns < N are
//   read, so the pad columns of a partial last tile never enter the sums.
//   h (bf16) goes to the next activation buffer, whose stale tail is zeroed
//   for the next layer's MFMA; xhat (bf16) is written over the wave's own
//   staging row, and the wave then saves h, xhat (16-byte chunks from LDS)
//   and rstd (fp32) of its row.  gamma, beta and the biases are fp32 reads
//   of the flat master buffer.
//
// k_bf16_chain_ln_dx walks the chain top-down.  The GEMM dA = dz_l W_l leaves
// fp32 dA (the gradient at h of layer l - 1) in the staging tile; row phase:
//   dh = dA [h > 0]; g = dh gamma; m1 = sum g / N; m2 = sum g xhat / N;
//   dz = rstd (g - m1 - xhat m2)
//   with the saved bf16 h and xhat and the saved fp32 rstd.  dz (bf16) goes
//   to the other dy buffer (the next GEMM's A operand) and, with want_dw, to
//   HBM for dwdb_grouped_arena.  For the parameter gradients the wave leaves
//   dh (fp32) in its staging row and xhat in the dy buffer the GEMM just
//   consumed; after a barrier thread c sums column c over the 16 rows in row
//   order: d beta = sum dh, d gamma = sum dh xhat — one partial per workgroup
//   in part[l][block][g][2][N], no atomics.  want_dw = 0 (the actor pass
//   through the frozen critic) skips all of that and ends with dx0.
//
// k_ln_dgb_fold (one launch, all layers and groups): arena row s at the
// parameters' flat-gradient offsets = the block partials of rows
// [s chunk, (s + 1) chunk), added in block order from 0.f.  Every one of the
// S rows is written (a row with no block gets 0): the arena is uninitialized
// memory and k_reduce_arena adds all S rows.

#include <hip/hip_runtime.h>
#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>
#include <c10/hip/HIPStream.h>

#include <algorithm>
#include <vector>

#include "chain_frag.h"

// Packed fp32 ops are kept out of these kernels (see tqc.hip).
#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute push(                                             \
    __attribute__((target("no-packed-fp32-ops"))), apply_to = function)
#endif

namespace lnchain {

using chain::bf16x8;
using chain::CMAX;
using chain::CPAD;
using chain::f32_to_bf16_rne3;
using chain::f32x4;
using chain::packed_kloop;
using chain::u16;

static constexpr int WAVES = 16, NT = WAVES * 64;   // threads per workgroup
static constexpr int TQ = 2, DEPTH = 4;             // as the _pipe kernels
static constexpr int TM = 16;                       // rows per workgroup
static constexpr int NV = CMAX / 64;                // row values per lane
static constexpr int MAXL = 6;

static inline hipStream_t cur_stream() {
  return c10::hip::getCurrentHIPStream().stream();
}

__device__ __forceinline__ float bf16_bits_to_f32(u16 h) {
  return __builtin_bit_cast(float, (unsigned)h << 16);
}

// Sum over the 64 lanes; every lane returns the same bits.
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// The wave's LDS writes are complete and visible to its other lanes.
__device__ __forceinline__ void wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// One LDS row of n bf16 -> global, by one wave: 16-byte chunks where the
// global row is 16-byte aligned (n % 8 == 0), else element by element.
__device__ __forceinline__ void wave_save_row(u16* __restrict__ dst,
                                              const u16* src, int n,
                                              int lane) {
  if ((n & 7) == 0) {
    for (int c = lane * 8; c < n; c += 64 * 8)
      *(uint4*)&dst[c] = *(const uint4*)&src[c];
  } else {
    for (int c = lane; c < n; c += 64) dst[c] = src[c];
  }
}

// The lane's bp[] of packed_kloop for column tiles t0 .. t0 + TQ - 1 of a
// packed operand with NTp tiles of KS k-steps (surplus slots re-read the
// last valid tile; their accumulators are never stored).
__device__ __forceinline__ void tile_bases(long (&bp)[TQ], int t0, int nq,
                                           int NTp, int KS, int g,
                                           int lane) {
#pragma unroll
  for (int j = 0; j < TQ; ++j) {
    int tt = t0 + (j < nq ? j : nq - 1);
    if (tt >= NTp) tt = NTp - 1;
    bp[j] = (((long)g * NTp + tt) * KS) * 512 + lane * 8;
  }
}

// ---------------------------------------------------------------------------
// forward
// ---------------------------------------------------------------------------
struct LnFwdDesc {
  const u16* wp[MAXL];       // fragment-packed W_l (forward pack)
  const float* b[MAXL];      // [G, N_l]
  const float* gamma[MAXL];  // [G, N_l], hidden layers
  const float* beta[MAXL];
  u16* h[MAXL];              // saved relu output [G, M, N_l] (null = skip)
  u16* xhat[MAXL];           // saved normalized value [G, M, N_l]
  float* rstd[MAXL];         // [G, M]
  int N[MAXL];
  int L;
};

__global__ __launch_bounds__(NT) void k_bf16_chain_ln_fwd(
    const void* __restrict__ x1, const void* __restrict__ x2,
    int C1, int C2, int x1f, int x2f, int rowcat, int M1,
    u16* __restrict__ xsave, LnFwdDesc d, void* __restrict__ y, int M,
    int out_f32, float eps) {
  __shared__ u16 sa[2][TM][CPAD];
  __shared__ float sz[TM][CPAD];
  const int g = blockIdx.z;
  const int m0 = blockIdx.x * TM;
  const int tid = threadIdx.x;
  const int lane = tid & 63, wid = tid >> 6;
  const int fi = lane & 15, fk = lane >> 4;
  const int rowlim = (M - m0 < TM ? M - m0 : TM);
  const int K0 = rowcat ? C1 : C1 + C2;

  // zero both activation buffers (pads must read 0 in the MFMA A-frags)
  {
    unsigned* p = (unsigned*)sa;
    for (int i = tid; i < 2 * TM * CPAD / 2; i += NT) p[i] = 0u;
  }
  __syncthreads();

  // input tile -> sa[0] as bf16; rowcat: x = [x1 ; x2] over rows, else
  // x = [x1 || x2] over columns
  {
    const int r = tid >> 5;
    const int lc = tid & 31;
    for (int rr = r; rr < rowlim; rr += NT / 32) {
      const long row = m0 + rr;
      for (int c = lc; c < K0; c += 32) {
        float v;
        if (rowcat) {
          const bool top = row < M1;
          const long rr2 = top ? row : row - M1;
          const int f_ = top ? x1f : x2f;
          v = f_ ? ((const float*)(top ? x1 : x2))[rr2 * C1 + c]
                 : (float)((const __bf16*)(top ? x1 : x2))[rr2 * C1 + c];
        } else if (c < C1) {
          v = x1f ? ((const float*)x1)[row * C1 + c]
                  : (float)((const __bf16*)x1)[row * C1 + c];
        } else {
          v = x2f ? ((const float*)x2)[row * C2 + (c - C1)]
                  : (float)((const __bf16*)x2)[row * C2 + (c - C1)];
        }
        sa[0][rr][c] = f32_to_bf16_rne3(v);
      }
    }
  }
  __syncthreads();
  // the bf16 input, for the dW kernel: one wave per row
  if (xsave != nullptr && g == 0) {
    for (int r = wid; r < rowlim; r += WAVES)
      wave_save_row(xsave + (long)(m0 + r) * K0, &sa[0][r][0], K0, lane);
  }

  int cur = 0;
  int pw[2] = {K0, 0};   // written widths of the two buffers
  int K = K0;
  for (int li = 0; li < d.L; ++li) {
    const int N = d.N[li];
    const bool last = li == d.L - 1;
    const float* bb = d.b[li] + (long)g * N;
    const int ntiles = (N + 15) >> 4;
    const int KS = (K + 31) >> 5;
    const int nb = cur ^ 1;

    for (int t0 = wid * TQ; t0 < ntiles; t0 += TQ * WAVES) {
      const int nq = (ntiles - t0 < TQ) ? (ntiles - t0) : TQ;
      f32x4 acc[TQ];
#pragma unroll
      for (int j = 0; j < TQ; ++j) acc[j] = f32x4{};
      long bp[TQ];
      tile_bases(bp, t0, nq, ntiles, KS, g, lane);
      packed_kloop<TQ, DEPTH>(
          d.wp[li], bp, KS, [&](const bf16x8 (&bset)[TQ], int kk) {
            const bf16x8 a_ = *(const bf16x8*)&sa[cur][fi][kk + fk * 8];
#pragma unroll
            for (int j = 0; j < TQ; ++j)
              acc[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                  a_, bset[j], acc[j], 0, 0, 0);
          });
      // epilogue: C/D map col = lane & 15, row = (lane >> 4) * 4 + r
#pragma unroll
      for (int q = 0; q < TQ; ++q) {
        if (q >= nq) break;
        const int col = (t0 + q) * 16 + fi;
        if (col < N) {
          const float bias = bb[col];
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int row = fk * 4 + r;
            const float v = acc[q][r] + bias;
            if (!last) {
              sz[row][col] = v;   // fp32, not rounded
            } else if (row < rowlim) {
              const long o = ((long)g * M + m0 + row) * N + col;
              if (out_f32) ((float*)y)[o] = v;
              else ((u16*)y)[o] = f32_to_bf16_rne3(v);
            }
          }
        }
      }
    }
    if (last) break;
    __syncthreads();

    // ---- row phase: wave w owns row w ----------------------------------
    const float* gam = d.gamma[li] + (long)g * N;
    const float* bet = d.beta[li] + (long)g * N;
    const float inv_n = 1.0f / (float)N;
    for (int r = wid; r < TM; r += WAVES) {
      float zv[NV];
      float s = 0.f;
#pragma unroll
      for (int i = 0; i < NV; ++i) {
        const int c = lane + 64 * i;
        zv[i] = c < N ? sz[r][c] : 0.f;
        s += zv[i];
      }
      const float mu = wave_sum(s) * inv_n;
      float q = 0.f;
#pragma unroll
      for (int i = 0; i < NV; ++i) {
        const float dv = zv[i] - mu;
        if (lane + 64 * i < N) q += dv * dv;
      }
      const float rstd = 1.0f / sqrtf(wave_sum(q) * inv_n + eps);
      // xhat (bf16) over the wave's own staging row: every lane holds its
      // z in registers by now
      u16* xrow = (u16*)&sz[r][0];
#pragma unroll
      for (int i = 0; i < NV; ++i) {
        const int c = lane + 64 * i;
        if (c < N) {
          const float xh = (zv[i] - mu) * rstd;
          sa[nb][r][c] = f32_to_bf16_rne3(fmaxf(xh * gam[c] + bet[c], 0.f));
          xrow[c] = f32_to_bf16_rne3(xh);
        }
      }
      // the stale tail of the next buffer must read 0 in the next MFMA
      for (int c = N + lane; c < pw[nb]; c += 64) sa[nb][r][c] = 0;
      if (d.h[li] != nullptr && r < rowlim) {
        wave_lds_sync();
        const long row = (long)g * M + m0 + r;
        wave_save_row(d.h[li] + row * N, &sa[nb][r][0], N, lane);
        wave_save_row(d.xhat[li] + row * N, xrow, N, lane);
        if (lane == 0) d.rstd[li][row] = rstd;
      }
    }
    pw[nb] = N;
    __syncthreads();
    cur = nb;
    K = N;
  }
}

// ---------------------------------------------------------------------------
// backward: the dx walk
// ---------------------------------------------------------------------------
struct LnDxDesc {
  const u16* wp[MAXL];       // fragment-packed W_l^T (dx pack)
  const u16* h[MAXL];        // saved relu output of hidden layer l
  const u16* xhat[MAXL];
  const float* rstd[MAXL];
  const float* gamma[MAXL];
  u16* dz[MAXL];             // [G, M, N_l], hidden layers (want_dw)
  float* part[MAXL];         // [blocks, G, 2, N_l]: d beta | d gamma
  int N[MAXL];
  int L;
  int K0;
  int dx0_lo;                // -1 = no input gradient
  int want_dw;
};

__global__ __launch_bounds__(NT) void k_bf16_chain_ln_dx(
    const u16* __restrict__ dy_last, LnDxDesc d, float* __restrict__ dx0,
    int M) {
  __shared__ u16 sd[2][TM][CPAD];
  __shared__ float sg[TM][CPAD];
  const int g = blockIdx.z, G = gridDim.z;
  const int m0 = blockIdx.x * TM;
  const int tid = threadIdx.x;
  const int lane = tid & 63, wid = tid >> 6;
  const int fi = lane & 15, fk = lane >> 4;
  const int rowlim = (M - m0 < TM ? M - m0 : TM);

  {
    unsigned* p = (unsigned*)sd;
    for (int i = tid; i < 2 * TM * CPAD / 2; i += NT) p[i] = 0u;
  }
  __syncthreads();
  const int NL = d.N[d.L - 1];
  {
    const int r = tid >> 5;
    const int lc = tid & 31;
    const u16* src = dy_last + (long)g * M * NL;
    for (int rr = r; rr < rowlim; rr += NT / 32)
      for (int c = lc; c < NL; c += 32)
        sd[0][rr][c] = src[(long)(m0 + rr) * NL + c];
  }
  __syncthreads();

  int cur = 0;
  int pw[2] = {NL, 0};
  for (int li = d.L - 1; li >= 0; --li) {
    const int N = d.N[li];
    const int K = li > 0 ? d.N[li - 1] : d.K0;
    const bool want_dx0 = li == 0;
    if (want_dx0 && d.dx0_lo < 0) break;

    // ---- GEMM: dA[16, K] = dz_l[16, N] W_l (packed W^T) ----------------
    const int col_lo = want_dx0 ? d.dx0_lo : 0;
    const int ntiles = (K + 15) >> 4;
    const int KS = (N + 31) >> 5;
    const int nb = cur ^ 1;
    float* dx0g = want_dx0 ? dx0 + (long)g * M * (K - col_lo) : nullptr;
    for (int t0 = (col_lo >> 4) + wid * TQ; t0 < ntiles; t0 += TQ * WAVES) {
      const int nq = (ntiles - t0 < TQ) ? (ntiles - t0) : TQ;
      f32x4 acc[TQ];
#pragma unroll
      for (int j = 0; j < TQ; ++j) acc[j] = f32x4{};
      long bp[TQ];
      tile_bases(bp, t0, nq, ntiles, KS, g, lane);
      packed_kloop<TQ, DEPTH>(
          d.wp[li], bp, KS, [&](const bf16x8 (&bset)[TQ], int kk) {
            const bf16x8 a_ = *(const bf16x8*)&sd[cur][fi][kk + fk * 8];
#pragma unroll
            for (int j = 0; j < TQ; ++j)
              acc[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                  a_, bset[j], acc[j], 0, 0, 0);
          });
#pragma unroll
      for (int q = 0; q < TQ; ++q) {
        if (q >= nq) break;
        const int col = (t0 + q) * 16 + fi;
        if (col < K) {
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int row = fk * 4 + r;
            if (!want_dx0)
              sg[row][col] = acc[q][r];
            else if (row < rowlim && col >= col_lo)
              dx0g[(long)(m0 + row) * (K - col_lo) + (col - col_lo)] =
                  acc[q][r];
          }
        }
      }
    }
    if (want_dx0) break;
    __syncthreads();

    // ---- row phase of hidden layer ln = li - 1 (width K) ---------------
    const int ln = li - 1;
    const float* gam = d.gamma[ln] + (long)g * K;
    const float inv_n = 1.0f / (float)K;
    for (int r = wid; r < TM; r += WAVES) {
      const bool live = r < rowlim;
      const long row = (long)g * M + m0 + (live ? r : 0);
      const u16* hrow = d.h[ln] + row * K;
      const u16* xr = d.xhat[ln] + row * K;
      float gv[NV], dhv[NV];
      u16 xb[NV];
      float s1 = 0.f, s2 = 0.f;
#pragma unroll
      for (int i = 0; i < NV; ++i) {
        const int c = lane + 64 * i;
        gv[i] = 0.f;
        dhv[i] = 0.f;
        xb[i] = 0;
        if (c < K && live) {
          const u16 hh = hrow[c];
          xb[i] = xr[c];
          // h is a relu output: positive unless it is +-0
          dhv[i] = (hh & 0x7fff) != 0 ? sg[r][c] : 0.f;
          gv[i] = dhv[i] * gam[c];
          s1 += gv[i];
          s2 += gv[i] * bf16_bits_to_f32(xb[i]);
        }
      }
      const float m1 = wave_sum(s1) * inv_n;
      const float m2 = wave_sum(s2) * inv_n;
      const float rs = live ? d.rstd[ln][row] : 0.f;
#pragma unroll
      for (int i = 0; i < NV; ++i) {
        const int c = lane + 64 * i;
        if (c < K) {
          const float dz = rs * (gv[i] - m1 - bf16_bits_to_f32(xb[i]) * m2);
          sd[nb][r][c] = f32_to_bf16_rne3(dz);
          if (d.want_dw) {
            sg[r][c] = dhv[i];       // the lane's own element
            sd[cur][r][c] = xb[i];   // the GEMM is done with this buffer
          }
        }
      }
      for (int c = K + lane; c < pw[nb]; c += 64) sd[nb][r][c] = 0;
      if (d.want_dw && live) {
        wave_lds_sync();
        wave_save_row(d.dz[ln] + row * K, &sd[nb][r][0], K, lane);
      }
    }
    pw[nb] = K;
    if (d.want_dw && K > pw[cur]) pw[cur] = K;
    __syncthreads();

    // ---- column phase: this block's partials of d beta and d gamma -----
    if (d.want_dw) {
      float* pb = d.part[ln] + ((long)blockIdx.x * G + g) * 2 * K;
      for (int c = tid; c < K; c += NT) {
        float sb = 0.f, sgm = 0.f;
#pragma unroll
        for (int r = 0; r < TM; ++r) {
          const float dh = sg[r][c];
          sb += dh;
          sgm += dh * bf16_bits_to_f32(sd[cur][r][c]);
        }
        pb[c] = sb;
        pb[K + c] = sgm;
      }
      __syncthreads();   // the next GEMM's epilogue writes sg
    }
    cur = nb;
  }
}

// ---------------------------------------------------------------------------
// fold of the d beta / d gamma block partials into the split-K arena
// ---------------------------------------------------------------------------
struct LnFoldDesc {
  const float* part[MAXL];
  long g_off[MAXL], b_off[MAXL];   // flat-gradient offsets of gamma / beta
  int N[MAXL];
  int cum[MAXL + 1];               // cumulative 2 G N_l
  int L;
};

__global__ __launch_bounds__(256) void k_ln_dgb_fold(
    LnFoldDesc d, float* __restrict__ arena, long stride, int chunk,
    int nblk, int G) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= d.cum[d.L]) return;
  const int s = blockIdx.y;
  int l = 0;
  while (l + 1 < d.L && i >= d.cum[l + 1]) ++l;
  const int N = d.N[l];
  const int local = i - d.cum[l];
  const int c = local % N, which = (local / N) & 1, g = local / (2 * N);
  const long b0 = (long)s * chunk / TM;
  long b1 = ((long)s + 1) * chunk / TM;
  if (b1 > nblk) b1 = nblk;
  float acc = 0.f;
  for (long b = b0; b < b1; ++b)
    acc += d.part[l][((b * G + g) * 2 + which) * N + c];
  const long off = which ? d.g_off[l] : d.b_off[l];
  arena[(long)s * stride + off + (long)g * N + c] = acc;
}

// ---------------------------------------------------------------------------
// host
// ---------------------------------------------------------------------------
#define LN_CHECK(t, dt, what)                                             \
  TORCH_CHECK((t).is_cuda() && (t).scalar_type() == (dt)                  \
                  && (t).is_contiguous(),                                 \
              "ln chain: " #t " must be a contiguous " what " HIP tensor")

// [y, x_bf16 (empty without save_acts) (, h_0 .., xhat_0 .., rstd_0 ..)] =
// mlp_chain_ln_fwd_bf16(
//     x1, x2_or_empty, wps, bs, gammas, betas, G, out_f32, rowcat,
//     save_acts, eps)
// wps[l]: the forward fragment pack of W_l [G, N_l, K_l]; bs[l] f32 [G, N_l];
// gammas / betas: f32 [G, N_l] for the L - 1 hidden layers.  The inputs are
// those of mlp_chain_fwd_bf16.  With save_acts the L - 1 hidden layers'
// h and xhat ([M, N] for G = 1, else [G, M, N], bf16) and rstd ([G, M] f32)
// follow, what mlp_chain_ln_dx_bf16 consumes.
static std::vector<torch::Tensor> mlp_chain_ln_fwd_bf16(
    torch::Tensor x1, torch::Tensor x2, std::vector<torch::Tensor> wps,
    std::vector<torch::Tensor> bs, std::vector<torch::Tensor> gammas,
    std::vector<torch::Tensor> betas, long G, long out_f32, long rowcat,
    long save_acts, double eps) {
  const int L = (int)wps.size();
  TORCH_CHECK(L >= 2 && L <= MAXL && (int)bs.size() == L
                  && (int)gammas.size() == L - 1
                  && (int)betas.size() == L - 1 && G >= 1,
              "ln chain fwd: 2..6 layers, gamma/beta per hidden layer");
  TORCH_CHECK(x1.is_cuda() && x1.dim() == 2);
  auto is_in = [](const torch::Tensor& t) {
    return t.scalar_type() == torch::kFloat32
           || t.scalar_type() == torch::kBFloat16;
  };
  TORCH_CHECK(is_in(x1), "ln chain fwd: inputs are fp32 or bf16");
  const bool has2 = x2.numel() > 0;
  auto x1c = x1.contiguous();
  auto x2c = x2;
  if (has2) {
    TORCH_CHECK(x2.is_cuda() && x2.dim() == 2 && is_in(x2));
    TORCH_CHECK(rowcat ? x2.size(1) == x1.size(1) : x2.size(0) == x1.size(0),
                "ln chain fwd: the two inputs do not fit together");
    x2c = x2.contiguous();
  }
  TORCH_CHECK(!rowcat || has2, "rowcat needs two inputs");
  const long M1 = x1c.size(0);
  const long M = rowcat ? M1 + x2c.size(0) : M1;
  const long C1 = x1c.size(1), C2 = has2 ? x2c.size(1) : 0;
  const long K0 = rowcat ? C1 : C1 + C2;
  TORCH_CHECK(M >= 1 && K0 >= 1 && K0 <= CMAX,
              "ln chain fwd: input width must be in 1..", CMAX);

  LnFwdDesc d{};
  d.L = L;
  auto bopts = x1c.options().dtype(torch::kBFloat16);
  auto fopts = x1c.options().dtype(torch::kFloat32);
  std::vector<torch::Tensor> out(2), hs, xhs, rs;
  // a forward nobody differentiates keeps no bf16 copy of its input
  out[1] = save_acts ? torch::empty({M, K0}, bopts)
                     : torch::empty({0}, bopts);
  long K = K0;
  for (int i = 0; i < L; ++i) {
    LN_CHECK(wps[i], torch::kBFloat16, "bf16");
    LN_CHECK(bs[i], torch::kFloat32, "fp32");
    const long N = bs[i].numel() / G;
    TORCH_CHECK(N >= 1 && N <= CMAX && N * G == bs[i].numel(),
                "ln chain fwd: layer width must be in 1..", CMAX);
    TORCH_CHECK(wps[i].numel() == G * ((N + 15) / 16) * ((K + 31) / 32) * 512,
                "ln chain fwd: packed weights of layer ", i,
                " do not fit [", G, ", ", N, ", ", K, "]");
    d.wp[i] = (const u16*)wps[i].data_ptr();
    d.b[i] = bs[i].data_ptr<float>();
    d.N[i] = (int)N;
    if (i < L - 1) {
      LN_CHECK(gammas[i], torch::kFloat32, "fp32");
      LN_CHECK(betas[i], torch::kFloat32, "fp32");
      TORCH_CHECK(gammas[i].numel() == G * N && betas[i].numel() == G * N,
                  "ln chain fwd: gamma/beta of layer ", i, " must be [G, N]");
      d.gamma[i] = gammas[i].data_ptr<float>();
      d.beta[i] = betas[i].data_ptr<float>();
      if (save_acts) {
        auto shape = G == 1 ? std::vector<long>{M, N}
                            : std::vector<long>{G, M, N};
        hs.push_back(torch::empty(shape, bopts));
        xhs.push_back(torch::empty(shape, bopts));
        rs.push_back(torch::empty({G, M}, fopts));
        d.h[i] = (u16*)hs.back().data_ptr();
        d.xhat[i] = (u16*)xhs.back().data_ptr();
        d.rstd[i] = rs.back().data_ptr<float>();
      }
    }
    K = N;
  }
  auto yopts = out_f32 ? fopts : bopts;
  out[0] = G == 1 ? torch::empty({M, K}, yopts)
                  : torch::empty({G, M, K}, yopts);
  for (auto* v : {&hs, &xhs, &rs}) out.insert(out.end(), v->begin(), v->end());
  dim3 grid((M + TM - 1) / TM, 1, G);
  hipLaunchKernelGGL(
      k_bf16_chain_ln_fwd, grid, dim3(NT), 0, cur_stream(),
      x1c.data_ptr(), has2 ? x2c.data_ptr() : nullptr, (int)C1, (int)C2,
      x1c.scalar_type() == torch::kFloat32 ? 1 : 0,
      has2 && x2c.scalar_type() == torch::kFloat32 ? 1 : 0, (int)rowcat,
      (int)M1, save_acts ? (u16*)out[1].data_ptr() : nullptr, d,
      out[0].data_ptr(), (int)M,
      (int)out_f32, (float)eps);
  return out;
}

// [dz_0 .. dz_{L-1}, part_0 .. part_{L-2}] (want_dw) [, dx0] =
// mlp_chain_ln_dx_bf16(dy_last, wps, hs, xhats, rstds, gammas, K0, G,
//                      want_dw, dx0_lo)
// wps[l]: the dx fragment pack of W_l (l = 0 is read only for dx0); hs,
// xhats, rstds: what the forward saved; dy_last bf16 [G, M, N_{L-1}] (or
// [M, N] for G = 1).  dz_l [G, M, N_l] is the gradient at layer l's linear
// output (dz_{L-1} is dy_last itself), part_l [ceil(M/16), G, 2, N_l] the
// block partials of d beta | d gamma for ln_dgb_fold, dx0 the fp32 input
// gradient of columns >= dx0_lo per group [G, M, K0 - dx0_lo].
static std::vector<torch::Tensor> mlp_chain_ln_dx_bf16(
    torch::Tensor dy_last, std::vector<torch::Tensor> wps,
    std::vector<torch::Tensor> hs, std::vector<torch::Tensor> xhats,
    std::vector<torch::Tensor> rstds, std::vector<torch::Tensor> gammas,
    long K0, long G, long want_dw, long dx0_lo) {
  const int L = (int)wps.size();
  TORCH_CHECK(L >= 2 && L <= MAXL && (int)hs.size() == L - 1
                  && (int)xhats.size() == L - 1 && (int)rstds.size() == L - 1
                  && (int)gammas.size() == L - 1 && G >= 1,
              "ln chain dx: 2..6 layers, saved tensors per hidden layer");
  TORCH_CHECK(dy_last.is_cuda() && dy_last.scalar_type() == torch::kBFloat16
              && dy_last.dim() == (G == 1 ? 2 : 3));
  TORCH_CHECK(K0 >= 1 && K0 <= CMAX && dx0_lo < K0);
  auto dyc = dy_last.contiguous();
  const long M = dyc.size(-2), NLast = dyc.size(-1);
  TORCH_CHECK(M >= 1 && (G == 1 || dyc.size(0) == G));
  const long nblk = (M + TM - 1) / TM;
  LnDxDesc d{};
  d.L = L;
  d.K0 = (int)K0;
  d.dx0_lo = (int)dx0_lo;
  d.want_dw = want_dw ? 1 : 0;
  auto bopts = dyc.options();
  auto fopts = dyc.options().dtype(torch::kFloat32);
  std::vector<torch::Tensor> dzs, parts;
  long K = K0;
  for (int i = 0; i < L; ++i) {
    const long N = i < L - 1 ? gammas[i].numel() / G : NLast;
    TORCH_CHECK(N >= 1 && N <= CMAX);
    // layer 0's W^T is read for dx0 only
    if (i > 0 || dx0_lo >= 0) {
      LN_CHECK(wps[i], torch::kBFloat16, "bf16");
      TORCH_CHECK(
          wps[i].numel() == G * ((K + 15) / 16) * ((N + 31) / 32) * 512,
          "ln chain dx: packed weights of layer ", i, " do not fit [", G,
          ", ", N, ", ", K, "]^T");
      d.wp[i] = (const u16*)wps[i].data_ptr();
    }
    d.N[i] = (int)N;
    if (i < L - 1) {
      LN_CHECK(hs[i], torch::kBFloat16, "bf16");
      LN_CHECK(xhats[i], torch::kBFloat16, "bf16");
      LN_CHECK(rstds[i], torch::kFloat32, "fp32");
      LN_CHECK(gammas[i], torch::kFloat32, "fp32");
      TORCH_CHECK(hs[i].numel() == G * M * N && xhats[i].numel() == G * M * N
                  && rstds[i].numel() == G * M && gammas[i].numel() == G * N,
                  "ln chain dx: saved tensors of layer ", i,
                  " do not fit [", G, ", ", M, ", ", N, "]");
      d.h[i] = (const u16*)hs[i].data_ptr();
      d.xhat[i] = (const u16*)xhats[i].data_ptr();
      d.rstd[i] = rstds[i].data_ptr<float>();
      d.gamma[i] = gammas[i].data_ptr<float>();
      if (want_dw) {
        dzs.push_back(torch::empty({G, M, N}, bopts));
        parts.push_back(torch::empty({nblk, G, 2, N}, fopts));
        d.dz[i] = (u16*)dzs.back().data_ptr();
        d.part[i] = parts.back().data_ptr<float>();
      }
    }
    K = N;
  }
  std::vector<torch::Tensor> out;
  if (want_dw) {
    out = dzs;
    out.push_back(dyc.view({G, M, NLast}));
    out.insert(out.end(), parts.begin(), parts.end());
  }
  torch::Tensor dx0;
  if (dx0_lo >= 0) {
    dx0 = torch::empty({G, M, K0 - dx0_lo}, fopts);
    out.push_back(dx0);
  }
  dim3 grid(nblk, 1, G);
  hipLaunchKernelGGL(k_bf16_chain_ln_dx, grid, dim3(NT), 0, cur_stream(),
                     (const u16*)dyc.data_ptr(), d,
                     dx0_lo >= 0 ? dx0.data_ptr<float>() : nullptr, (int)M);
  return out;
}

// ln_dgb_fold(parts, arena, g_offs, b_offs, G, S, chunk, M): arena[s] at
// g_offs[l] / b_offs[l] (+ g N_l) = the partials of the 16-row blocks inside
// rows [s chunk, (s + 1) chunk), for every s < S.
static void ln_dgb_fold(std::vector<torch::Tensor> parts, torch::Tensor arena,
                        std::vector<long> g_offs, std::vector<long> b_offs,
                        long G, long S, long chunk, long M) {
  const int L = (int)parts.size();
  TORCH_CHECK(L >= 1 && L < MAXL && (int)g_offs.size() == L
              && (int)b_offs.size() == L);
  LN_CHECK(arena, torch::kFloat32, "fp32");
  TORCH_CHECK(arena.dim() == 2 && arena.size(0) >= S && S >= 1);
  TORCH_CHECK(chunk >= TM && chunk % TM == 0,
              "ln_dgb_fold: the arena's row chunk (", chunk,
              ") must be a multiple of ", TM);
  TORCH_CHECK(S * chunk >= M, "ln_dgb_fold: S * chunk must cover the batch");
  const long stride = arena.size(1);
  const long nblk = (M + TM - 1) / TM;
  LnFoldDesc d{};
  d.L = L;
  int cum = 0;
  for (int i = 0; i < L; ++i) {
    LN_CHECK(parts[i], torch::kFloat32, "fp32");
    TORCH_CHECK(parts[i].dim() == 4 && parts[i].size(0) == nblk
                && parts[i].size(1) == G && parts[i].size(2) == 2);
    const long N = parts[i].size(3);
    TORCH_CHECK(g_offs[i] >= 0 && b_offs[i] >= 0
                && g_offs[i] + G * N <= stride && b_offs[i] + G * N <= stride,
                "ln_dgb_fold: offsets of layer ", i, " leave the arena row");
    d.part[i] = parts[i].data_ptr<float>();
    d.g_off[i] = g_offs[i];
    d.b_off[i] = b_offs[i];
    d.N[i] = (int)N;
    d.cum[i] = cum;
    cum += (int)(2 * G * N);
  }
  d.cum[L] = cum;
  hipLaunchKernelGGL(k_ln_dgb_fold, dim3((cum + 255) / 256, S), dim3(256), 0,
                     cur_stream(), d, arena.data_ptr<float>(), stride,
                     (int)chunk, (int)nblk, (int)G);
}

}  // namespace lnchain

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif

void register_ln_chain(pybind11::module_& m) {
  m.def("mlp_chain_ln_fwd_bf16", &lnchain::mlp_chain_ln_fwd_bf16,
        pybind11::arg("x1"), pybind11::arg("x2"), pybind11::arg("wps"),
        pybind11::arg("bs"), pybind11::arg("gammas"), pybind11::arg("betas"),
        pybind11::arg("G"), pybind11::arg("out_f32") = 1,
        pybind11::arg("rowcat") = 0, pybind11::arg("save_acts") = 1,
        pybind11::arg("eps") = 1e-5);
  m.def("mlp_chain_ln_dx_bf16", &lnchain::mlp_chain_ln_dx_bf16,
        pybind11::arg("dy_last"), pybind11::arg("wps"), pybind11::arg("hs"),
        pybind11::arg("xhats"), pybind11::arg("rstds"),
        pybind11::arg("gammas"), pybind11::arg("K0"), pybind11::arg("G"),
        pybind11::arg("want_dw"), pybind11::arg("dx0_lo"));
  m.def("ln_dgb_fold", &lnchain::ln_dgb_fold);
}
