// dsac_kernels.hip — CDNA4 (gfx950) kernels for the SAC hot path.
//
// Replaces the PyTorch op-sequences inventoried in SURVEY.md §2.6:
//   K1  linear_act_fwd[_g]   — GEMM + bias + ReLU (MFMA f32 16x16x4),
//                              grouped over grid.z (twin critics in one
//                              launch, shared activations)
//   K8  linear_bwd_dx/dwdb   — backward GEMMs with fused ReLU masking;
//                              dW/db is split-K over the batch (partials +
//                              reduce) so the grid fills 256 CUs
//   K4  squashed_gaussian_*  — fused clamp/exp/rsample/tanh/log-prob (+bwd)
//   K5  td_target            — Bellman backup elementwise
//   K6  critic/actor/alpha loss — single-workgroup fused loss reductions
//                              (incl. softmax(-alpha) task weights, per-task
//                              alpha gather, entropy) with analytic backward
//   K9  k_adam_groups        — fused Adam over up to three flat parameter
//                              buffers (+ arena fold, clipping, Polyak range)
//   K10 polyak_              — fused soft target update over flat buffers
//   K12 replay_sample        — stratified gather from the HBM-resident
//                              sharded replay in ONE kernel
//       replay_sample_norepl — the same gather drawing without replacement
//                              (keyed permutation evaluated per row)
//
// Design notes (see /opt/skills guides):
// - fp32 end-to-end like the reference; GEMMs use the exact f32-input MFMA
//   v_mfma_f32_16x16x4_f32 (155 TF peak — these latency-bound tiny GEMMs
//   are grid/launch-bound, not FLOP-bound, so exact fp32 costs nothing).
// - tiles are 64x64x32 with LDS staging; row pads chosen so the MFMA
//   fragment gathers are LDS-bank-conflict-free (+2 on 32-wide rows:
//   bank = (34*r + k) % 32 = (2r + k) % 32 distinct for r<16, k<2;
//   +16 on 64-wide rows: (80*m + j) % 32 = (16m + j) % 32 distinct).
// - one workgroup = 4 waves (wave64), each wave owns a 32x32 output
//   sub-tile as a 2x2 grid of 16x16 MFMA fragments.
// - everything is hipGraph-capturable: no host-side state in the hot path
//   (Adam step counter lives on-device).

#include <hip/hip_runtime.h>
#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>
#include <c10/hip/HIPStream.h>

#include <cmath>
#include <vector>

using f32x4 = __attribute__((__vector_size__(4 * sizeof(float)))) float;

static constexpr int BM = 64;   // batch-tile rows
static constexpr int BN = 64;   // out-tile cols
static constexpr int BK = 32;   // reduction tile
static constexpr int PAD_K = BK + 2;   // 34: conflict-free [*][BK] frag reads
static constexpr int PAD_N = 80;       // 64+16: conflict-free [BK][*] frag reads

#define CHECK_IN(t) TORCH_CHECK((t).is_cuda() && (t).scalar_type() == torch::kFloat32, \
                                #t " must be a fp32 HIP tensor")

static inline hipStream_t cur_stream() {
  return c10::hip::getCurrentHIPStream().stream();
}

// ---------------------------------------------------------------------------
// K1: y[g,M,N] = act(x[M,K] @ w[g,N,K]^T + b[g,N])   act: 0=none, 1=relu
// x is SHARED across groups (twin critics consume the same activations).
// grid: (ceil(M/64), ceil(N/64), G)
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_linear_act_fwd(
    const float* __restrict__ x, const float* __restrict__ w,
    const float* __restrict__ b, float* __restrict__ y,
    int M, int N, int K, int act, long xgs) {
  // double-buffered: global loads for tile t+1 issue BEFORE the MFMAs of
  // tile t (HBM latency hides under compute — guide T14); ds_writes into
  // the other buffer, ONE barrier per K-tile.
  __shared__ float sx[2][BM][PAD_K];
  __shared__ float sw[2][BN][PAD_K];
  const long g = blockIdx.z;
  x += g * xgs;            // 0 = activations shared across groups
  w += g * (long)N * K;
  b += g * (long)N;
  y += g * (long)M * N;
  const int m0 = blockIdx.x * BM, n0 = blockIdx.y * BN;
  const int tid = threadIdx.x;
  const int lane = tid & 63, wid = tid >> 6;
  const int wr = (wid >> 1) * 32, wc = (wid & 1) * 32;
  const int fi = lane & 15, fk = lane >> 4;  // fragment row / k index
  f32x4 acc00{}, acc01{}, acc10{}, acc11{};

  const int lr = (tid * 8) >> 5, lc = (tid * 8) & 31;  // this thread's slot
  // 2-tiles-ahead prefetch: two register sets; loads for tile t+2 issue
  // while tile t computes, so each load gets ~2 MFMA phases of latency
  // cover (the 1-deep version stalled: HBM latency > one MFMA phase).
  float rxa[8], rwa[8], rxb[8], rwb[8];
#define LOAD_TILE_FWD(k0, rx, rw)                                           \
  _Pragma("unroll") for (int j = 0; j < 8; ++j) {                           \
    const int gk = (k0) + lc + j;                                           \
    rx[j] = (m0 + lr < M && gk < K) ? x[(long)(m0 + lr) * K + gk] : 0.f;    \
    rw[j] = (n0 + lr < N && gk < K) ? w[(long)(n0 + lr) * K + gk] : 0.f;    \
  }
#define STORE_TILE_FWD(buf, rx, rw)                                         \
  _Pragma("unroll") for (int j = 0; j < 8; ++j) {                           \
    sx[buf][lr][lc + j] = rx[j];                                            \
    sw[buf][lr][lc + j] = rw[j];                                            \
  }
  LOAD_TILE_FWD(0, rxa, rwa)
  STORE_TILE_FWD(0, rxa, rwa)
  if (BK < K) LOAD_TILE_FWD(BK, rxa, rwa)
  __syncthreads();
  int cur = 0;
  for (int k0 = 0; k0 < K; k0 += BK) {
    // issue loads for tile t+2 into the register set whose data for tile
    // t+1 has NOT yet been written to LDS?  No: set A holds t+1 (issued
    // last iter / prologue); set B receives t+2 now; at loop end we write
    // t+1 (set A) into the other LDS buffer and swap the sets.
    const bool have_next = k0 + BK < K;
    const bool have_next2 = k0 + 2 * BK < K;
    if (have_next2) LOAD_TILE_FWD(k0 + 2 * BK, rxb, rwb)
#pragma unroll
    for (int kk = 0; kk < BK; kk += 4) {
      const float a0 = sx[cur][wr + fi][kk + fk];
      const float a1 = sx[cur][wr + 16 + fi][kk + fk];
      const float b0 = sw[cur][wc + fi][kk + fk];
      const float b1 = sw[cur][wc + 16 + fi][kk + fk];
      acc00 = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, b0, acc00, 0, 0, 0);
      acc01 = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, b1, acc01, 0, 0, 0);
      acc10 = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, b0, acc10, 0, 0, 0);
      acc11 = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, b1, acc11, 0, 0, 0);
    }
    if (have_next) {
      STORE_TILE_FWD(cur ^ 1, rxa, rwa)
#pragma unroll
      for (int j = 0; j < 8; ++j) {  // swap register sets (compiled away)
        const float tx = rxa[j], tw = rwa[j];
        rxa[j] = rxb[j]; rwa[j] = rwb[j];
        rxb[j] = tx; rwb[j] = tw;
      }
    }
    __syncthreads();
    cur ^= 1;
  }
  // epilogue: C/D layout col = lane&15, row = (lane>>4)*4 + reg
  const f32x4* accs[2][2] = {{&acc00, &acc01}, {&acc10, &acc11}};
#pragma unroll
  for (int mi = 0; mi < 2; ++mi)
#pragma unroll
    for (int ni = 0; ni < 2; ++ni) {
      const f32x4 a = *accs[mi][ni];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = m0 + wr + mi * 16 + fk * 4 + r;
        const int col = n0 + wc + ni * 16 + fi;
        if (row < M && col < N) {
          float v = a[r] + b[col];
          if (act == 1) v = fmaxf(v, 0.f);
          y[(long)row * N + col] = v;
        }
      }
    }
}

// ---------------------------------------------------------------------------
// K8a: dx[M,K] = sum_g (dy*mask)[g,M,N] @ w[g,N,K]  (mask = yout>0 if act)
// The G-sum is the twin-critic case: both Qs consume the same x, so dL/dx
// accumulates over groups inside the K-loop (no extra kernel or atomics).
// grid: (ceil(M/64), ceil(K/64))
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_linear_bwd_dx(
    const float* __restrict__ dy, const float* __restrict__ w,
    const float* __restrict__ yout, float* __restrict__ dx,
    int M, int N, int K, int act, int G, int S) {
  __shared__ float sdy[2][BM][PAD_K];   // [m][n-slice]
  __shared__ float sw[2][BK][PAD_N];     // [n-slice][k]
  // grid.z = Gz*S: Gz per-group slots (1 in summed mode), S slices over
  // the flattened (g, n0) reduction-tile loop (split-reduce fills the
  // chip for narrow-K layers; partials folded by k_reduce_partials).
  const long z = blockIdx.z;
  const long gz = z / S, sl = z % S;
  dy += gz * (long)M * N;
  w += gz * (long)N * K;
  yout += gz * (long)M * N;
  dx += z * (long)M * K;   // one output slab per (gz, slice)
  const int m0 = blockIdx.x * BM, c0 = blockIdx.y * BN;  // c over K
  const int tid = threadIdx.x;
  const int lane = tid & 63, wid = tid >> 6;
  const int wr = (wid >> 1) * 32, wc = (wid & 1) * 32;
  const int fi = lane & 15, fk = lane >> 4;
  f32x4 acc00{}, acc01{}, acc10{}, acc11{};

  const int nt_per_g = (N + BK - 1) / BK;
  const int nt_all = G * nt_per_g;
  const int per_s = (nt_all + S - 1) / S;
  const int t_lo = (int)sl * per_s;
  const int nt = min(nt_all, t_lo + per_s);
  const int ar = (tid * 8) >> 5, ac = (tid * 8) & 31;  // dy slot (64x32)
  const int br = (tid * 8) >> 6, bc = (tid * 8) & 63;  // w slot (32x64)
  float rdy[8], rw[8];
#define LOAD_TILE_DX(ti)                                                    \
  {                                                                         \
    const int g_ = (ti) / nt_per_g;                                         \
    const int n0_ = ((ti) % nt_per_g) * BK;                                 \
    const float* dyg = dy + (long)g_ * M * N;                               \
    const float* wg = w + (long)g_ * N * K;                                 \
    const float* yg = yout + (long)g_ * M * N;                              \
    _Pragma("unroll") for (int j = 0; j < 8; ++j) {                         \
      const int gm = m0 + ar, gn = n0_ + ac + j;                            \
      float v = 0.f;                                                        \
      if (gm < M && gn < N) {                                               \
        v = dyg[(long)gm * N + gn];                                         \
        if (act == 1 && yg[(long)gm * N + gn] <= 0.f) v = 0.f;              \
      }                                                                     \
      rdy[j] = v;                                                           \
      const int wn = n0_ + br, wk = c0 + bc + j;                            \
      rw[j] = (wn < N && wk < K) ? wg[(long)wn * K + wk] : 0.f;             \
    }                                                                       \
  }
#define STORE_TILE_DX(buf)                                                  \
  _Pragma("unroll") for (int j = 0; j < 8; ++j) {                           \
    sdy[buf][ar][ac + j] = rdy[j];                                          \
    sw[buf][br][bc + j] = rw[j];                                            \
  }
  if (t_lo >= nt) {  // empty slice: still must write zeros
#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
      for (int ni = 0; ni < 2; ++ni)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int row = m0 + wr + mi * 16 + fk * 4 + r;
          const int col = c0 + wc + ni * 16 + fi;
          if (row < M && col < K) dx[(long)row * K + col] = 0.f;
        }
    return;
  }
  LOAD_TILE_DX(t_lo)
  STORE_TILE_DX(0)
  __syncthreads();
  int cur = 0;
  for (int ti = t_lo; ti < nt; ++ti) {
    const bool more = ti + 1 < nt;
    if (more) LOAD_TILE_DX(ti + 1)
#pragma unroll
    for (int kk = 0; kk < BK; kk += 4) {
      const float a0 = sdy[cur][wr + fi][kk + fk];
      const float a1 = sdy[cur][wr + 16 + fi][kk + fk];
      const float b0 = sw[cur][kk + fk][wc + fi];
      const float b1 = sw[cur][kk + fk][wc + 16 + fi];
      acc00 = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, b0, acc00, 0, 0, 0);
      acc01 = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, b1, acc01, 0, 0, 0);
      acc10 = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, b0, acc10, 0, 0, 0);
      acc11 = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, b1, acc11, 0, 0, 0);
    }
    if (more) STORE_TILE_DX(cur ^ 1)
    __syncthreads();
    cur ^= 1;
  }
  const f32x4* accs[2][2] = {{&acc00, &acc01}, {&acc10, &acc11}};
#pragma unroll
  for (int mi = 0; mi < 2; ++mi)
#pragma unroll
    for (int ni = 0; ni < 2; ++ni) {
      const f32x4 a = *accs[mi][ni];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = m0 + wr + mi * 16 + fk * 4 + r;
        const int col = c0 + wc + ni * 16 + fi;
        if (row < M && col < K) dx[(long)row * K + col] = a[r];
      }
    }
}

// ---------------------------------------------------------------------------
// K8b: dw[g,N,K] = (dy*mask)^T @ x per group, SPLIT-K over the batch:
// grid.z = G*S; slice s covers batch rows [s*chunk, (s+1)*chunk).  Partials
// land in ws[g*S+s][N][K] / ws_db[g*S+s][N]; k_reduce_partials folds S.
// This turns the 49-block (or 7-block, for head layers) serial-1280-batch
// kernel that dominated the baseline profile (104 us, 46% of GPU time —
// profiles/r01_baseline_NOTES.md) into a chip-filling grid.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_linear_bwd_dwdb_splitk(
    const float* __restrict__ dy, const float* __restrict__ x,
    const float* __restrict__ yout, float* __restrict__ ws,
    float* __restrict__ ws_db, int M, int N, int K, int act, int S,
    int chunk, long xgs) {
  __shared__ float sa[2][BN][PAD_K];   // dy^T tile: [n][m-slice]
  __shared__ float sb[2][BK][PAD_N];    // x tile:    [m-slice][k]
  const int gs = blockIdx.z;        // g*S + s
  const int g = gs / S, s = gs % S;
  const float* dyg = dy + (long)g * M * N;
  const float* yg = yout + (long)g * M * N;
  const float* xg = x + (long)g * xgs;
  float* wsp = ws + (long)gs * N * K;
  float* dbp = ws_db + (long)gs * N;
  const int m_lo = s * chunk;
  const int m_hi = min(M, m_lo + chunk);
  const int n0 = blockIdx.x * BM, c0 = blockIdx.y * BN;
  const int tid = threadIdx.x;
  const int lane = tid & 63, wid = tid >> 6;
  const int wr = (wid >> 1) * 32, wc = (wid & 1) * 32;
  const int fi = lane & 15, fk = lane >> 4;
  const bool do_db = (blockIdx.y == 0);
  float db_acc = 0.f;
  f32x4 acc00{}, acc01{}, acc10{}, acc11{};

  const int an = (tid * 8) & 63, am = (tid * 8) >> 6;  // dy slot (n fast)
  const int bm = (tid * 8) >> 6, bc = (tid * 8) & 63;  // x slot (k fast)
  float rdy[8], rx[8];
#define LOAD_TILE_DW(m0_)                                                   \
  _Pragma("unroll") for (int j = 0; j < 8; ++j) {                           \
    const int gm = (m0_) + am, gn = n0 + an + j;                            \
    float v = 0.f;                                                          \
    if (gm < m_hi && gn < N) {                                              \
      v = dyg[(long)gm * N + gn];                                           \
      if (act == 1 && yg[(long)gm * N + gn] <= 0.f) v = 0.f;                \
    }                                                                       \
    rdy[j] = v;                                                             \
    const int xm = (m0_) + bm, xk = c0 + bc + j;                            \
    rx[j] = (xm < m_hi && xk < K) ? xg[(long)xm * K + xk] : 0.f;            \
  }
#define STORE_TILE_DW(buf)                                                  \
  _Pragma("unroll") for (int j = 0; j < 8; ++j) {                           \
    sa[buf][an + j][am] = rdy[j];                                           \
    sb[buf][bm][bc + j] = rx[j];                                            \
  }
  LOAD_TILE_DW(m_lo)
  STORE_TILE_DW(0)
  __syncthreads();
  int cur = 0;
  for (int m0 = m_lo; m0 < m_hi; m0 += BK) {
    const bool more = m0 + BK < m_hi;
    if (more) LOAD_TILE_DW(m0 + BK)
    if (do_db && tid < BN) {
#pragma unroll
      for (int m = 0; m < BK; ++m) db_acc += sa[cur][tid][m];
    }
#pragma unroll
    for (int kk = 0; kk < BK; kk += 4) {
      const float a0 = sa[cur][wr + fi][kk + fk];
      const float a1 = sa[cur][wr + 16 + fi][kk + fk];
      const float b0 = sb[cur][kk + fk][wc + fi];
      const float b1 = sb[cur][kk + fk][wc + 16 + fi];
      acc00 = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, b0, acc00, 0, 0, 0);
      acc01 = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, b1, acc01, 0, 0, 0);
      acc10 = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, b0, acc10, 0, 0, 0);
      acc11 = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, b1, acc11, 0, 0, 0);
    }
    if (more) STORE_TILE_DW(cur ^ 1)
    __syncthreads();
    cur ^= 1;
  }
  if (do_db && tid < BN && n0 + tid < N) dbp[n0 + tid] = db_acc;
  const f32x4* accs[2][2] = {{&acc00, &acc01}, {&acc10, &acc11}};
#pragma unroll
  for (int mi = 0; mi < 2; ++mi)
#pragma unroll
    for (int ni = 0; ni < 2; ++ni) {
      const f32x4 a = *accs[mi][ni];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = n0 + wr + mi * 16 + fk * 4 + r;
        const int col = c0 + wc + ni * 16 + fi;
        if (row < N && col < K) wsp[(long)row * K + col] = a[r];
      }
    }
}

// fold S split-K partials: out[g][i] = sum_s ws[(g*S+s)*stride + i]
__global__ __launch_bounds__(256) void k_reduce_partials(
    const float* __restrict__ ws, float* __restrict__ out, long stride,
    int S, long n_per_g) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const int g = blockIdx.y;
  if (i >= n_per_g) return;
  const float* base = ws + ((long)g * S) * stride + i;
  float acc = 0.f;
  for (int s = 0; s < S; ++s) acc += base[(long)s * stride];
  out[(long)g * n_per_g + i] = acc;
}

// ---------------------------------------------------------------------------
// K12: stratified replay sample — ONE kernel replaces the per-shard
// index_select/cat chains (~65 torch kernels per update in the baseline
// profile).  Fields are stacked [T, cap, D]; output row i draws from shard
// t = i / (B/T) at index floor(rand[i] * size[t]).
// ---------------------------------------------------------------------------
// counter-based device RNG (splitmix64 hash of (counter, index, salt)):
// every RNG-consuming kernel derives its noise from one persistent int64
// counter that k_adam_prolog_many bumps ONCE per update
// (single-block kernels, so the bump is race-free by stream ordering).
// Replaces the per-update
// torch rand/randn launches AND the hipGraph RNG-offset bookkeeping
// kernels torch inserts around them.
__device__ __forceinline__ unsigned long long dsac_sm64(
    unsigned long long x) {
  x += 0x9E3779B97F4A7C15ull;
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}
__device__ __forceinline__ float dsac_u01(unsigned long long h) {
  // top 24 bits + 1 -> uniform in (0, 1]
  return (float)((h >> 40) + 1ull) * 5.9604644775390625e-8f;
}

__global__ __launch_bounds__(256) void k_replay_sample(
    const float* __restrict__ states, const float* __restrict__ actions,
    const float* __restrict__ rewards, const float* __restrict__ next_states,
    const float* __restrict__ dones, const float* __restrict__ sizes,
    const float* __restrict__ rnd, const long long* __restrict__ rng,
    float* __restrict__ o_states,
    float* __restrict__ o_actions, float* __restrict__ o_rewards,
    float* __restrict__ o_next_states, float* __restrict__ o_dones,
    int B, int T, int per, long cap, int Ds, int Da) {
  // one wave per batch row: lanes stride the row's columns (coalesced on
  // both the gathered source row and the packed destination row)
  const int i = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (i >= B) return;
  const int t = min(i / per, T - 1);
  float u;
  if (rng != nullptr) {
    const unsigned long long c = (unsigned long long)rng[0];
    u = dsac_u01(dsac_sm64(c * 0x100000001ull
                           + (unsigned long long)i * 2ull + 0x2ull));
    u = u < 1.f ? u : 0.99999994f;  // keep floor(u*size) < size
  } else {
    u = rnd[i];
  }
  const long idx = (long)(u * sizes[t]);
  const long src = (long)t * cap + idx;
  for (int j = lane; j < Ds; j += 64) {
    o_states[(long)i * Ds + j] = states[src * Ds + j];
    o_next_states[(long)i * Ds + j] = next_states[src * Ds + j];
  }
  for (int j = lane; j < Da; j += 64)
    o_actions[(long)i * Da + j] = actions[src * Da + j];
  if (lane == 0) {
    o_rewards[i] = rewards[src];
    o_dones[i] = dones[src];
  }
}

// ---------------------------------------------------------------------------
// K12c: stratified replay sample WITHOUT replacement (opt-in; the
// reference's random.sample semantics).  Row j of shard t (size n, read on
// the device) gathers index (P(j mod n) + rot) mod n, where P is a keyed
// bijection of [0, n) and rot a keyed offset (docs/KERNELS.md "replay
// permutation"; the exact oracle is torch_ref.replay_sample_indices_norepl).
// P: NR_ROUNDS alternating unbalanced XOR-Feistel rounds over
// b = max(6, ceil(log2 n)) bits (low half b/2 bits, high half the rest),
// cycle-walked while the value is >= n.  The walk stays on one cycle of a
// bijection of [0, 2^b) that contains the start value (< n), so it returns
// below n after at most 2^b - n + 1 applications — the loop has no cap, a
// cap would break bijectivity.
//
// Key = dsac_sm64(c * 0x100000001 + 2^63 + t).  k_replay_sample hashes
// c * 0x100000001 + 2 i + 2 and k_squash_fwd hashes c * 0x100000001 + 2 idx
// + 1, with 2 i + 2 and 2 idx + 1 below 2^32: for counters below 2^31 - 2
// (the counter starts below 2^31 and grows by one per update) those hash
// inputs stay below 2^63 and these are at or above it, and dsac_sm64 is a
// bijection of the 64-bit words, so the key can equal none of their draws'
// hashes by sharing an input.  Round and offset values hash key + (r << 32)
// + v, a second hash level the other streams do not have.
// ---------------------------------------------------------------------------
constexpr int NR_ROUNDS = 8;

__device__ __forceinline__ unsigned dsac_norepl_index(
    unsigned long long c, unsigned t, unsigned j, unsigned n) {
  const unsigned long long key = dsac_sm64(
      c * 0x100000001ull + 0x8000000000000000ull + (unsigned long long)t);
  const unsigned rot = (unsigned)(dsac_sm64(key) >> 32) % n;
  const int b = n <= 64u ? 6 : 32 - __clz((int)(n - 1u));
  const int bl = b >> 1;
  const unsigned ml = (1u << bl) - 1u, mh = (1u << (b - bl)) - 1u;
  unsigned x = j % n;
  do {
    unsigned lo = x & ml, hi = x >> bl;
#pragma unroll
    for (int r = 0; r < NR_ROUNDS; ++r) {
      const unsigned long long kr = key + ((unsigned long long)(r + 1) << 32);
      if ((r & 1) == 0)
        lo ^= (unsigned)(dsac_sm64(kr + hi) >> 32) & ml;
      else
        hi ^= (unsigned)(dsac_sm64(kr + lo) >> 32) & mh;
    }
    x = (hi << bl) | lo;
  } while (x >= n);
  x += rot;                      // x, rot < n <= 2^31: no wrap
  return x >= n ? x - n : x;
}

__global__ __launch_bounds__(256) void k_replay_sample_norepl(
    const float* __restrict__ states, const float* __restrict__ actions,
    const float* __restrict__ rewards, const float* __restrict__ next_states,
    const float* __restrict__ dones, const float* __restrict__ sizes,
    const long long* __restrict__ rng, float* __restrict__ o_states,
    float* __restrict__ o_actions, float* __restrict__ o_rewards,
    float* __restrict__ o_next_states, float* __restrict__ o_dones,
    long long* __restrict__ idx_out, int B, int T, int per, long cap, int Ds,
    int Da) {
  // one wave per batch row, as k_replay_sample.  The row is the same for
  // all 64 lanes; readfirstlane lets the compiler see that, so the index
  // (hashes, walk loop) is computed once per wave on the scalar unit and
  // the loop cannot diverge.
  const int i = __builtin_amdgcn_readfirstlane(
      (int)(blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6)));
  const int lane = threadIdx.x & 63;
  if (i >= B) return;
  const int t = min(i / per, T - 1);
  // an empty shard reads row 0 (n = 1); a size beyond the storage cannot
  // index past it
  unsigned n = (unsigned)fmaxf(sizes[t], 1.f);
  n = (long)n > cap ? (unsigned)cap : n;
  const long idx = (long)dsac_norepl_index(
      (unsigned long long)rng[0], (unsigned)t, (unsigned)(i - t * per), n);
  const long src = (long)t * cap + idx;
  for (int j = lane; j < Ds; j += 64) {
    o_states[(long)i * Ds + j] = states[src * Ds + j];
    o_next_states[(long)i * Ds + j] = next_states[src * Ds + j];
  }
  for (int j = lane; j < Da; j += 64)
    o_actions[(long)i * Da + j] = actions[src * Da + j];
  if (lane == 0) {
    o_rewards[i] = rewards[src];
    o_dones[i] = dones[src];
    if (idx_out != nullptr) idx_out[i] = idx;
  }
}

// ---------------------------------------------------------------------------
// K12b: packed replay ingest — the write path of the [T, cap, D] rings.
// One launch scatters a whole packed batch (docs/KERNELS.md "packed replay
// batch"): header words [n_desc, T, total_rows, used], T float sizes, then
// 8-word descriptors {task, n, first, rows, offset, dst_row, row_base, 0}
// and the block payloads in ring-slot layout.  The host validates every
// descriptor and guarantees that no two rows of one batch share a
// destination, so plain stores suffice.
// ---------------------------------------------------------------------------
constexpr int PK_HDR = 4;    // header words before the sizes
constexpr int PK_DESC = 8;   // words per descriptor

__global__ __launch_bounds__(256) void k_replay_ingest(
    const float* __restrict__ pk, float* __restrict__ states,
    float* __restrict__ actions, float* __restrict__ rewards,
    float* __restrict__ next_states, float* __restrict__ dones,
    float* __restrict__ sizes, int n_desc, int total_rows, int T, long cap,
    int Ds, int Da) {
  if (blockIdx.x == 0)
    for (int t = threadIdx.x; t < T; t += blockDim.x)
      sizes[t] = pk[PK_HDR + t];
  // one wave per ingested row: lanes stride the row's columns
  const int i = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (i >= total_rows) return;
  const int* desc = reinterpret_cast<const int*>(pk) + PK_HDR + T;
  // last descriptor with row_base <= i (row_base is a running sum of rows)
  int lo = 0, hi = n_desc - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (desc[mid * PK_DESC + 6] <= i) lo = mid; else hi = mid - 1;
  }
  const int* d = desc + lo * PK_DESC;
  const long t = d[0], n = d[1];
  const long r = i - d[6];
  const long srow = d[2] + r;
  const long drow = t * cap + (d[5] + r) % cap;
  const float* p = pk + d[4];
  const float* p_s = p + srow * Ds;
  const float* p_a = p + n * Ds + srow * Da;
  const float* p_r = p + n * (Ds + Da) + srow;
  const float* p_ns = p + n * (Ds + Da + 1) + srow * Ds;
  const float* p_d = p + n * (2L * Ds + Da + 1) + srow;
  for (int j = lane; j < Ds; j += 64) {
    states[drow * Ds + j] = p_s[j];
    next_states[drow * Ds + j] = p_ns[j];
  }
  for (int j = lane; j < Da; j += 64)
    actions[drow * Da + j] = p_a[j];
  if (lane == 0) {
    rewards[drow] = p_r[0];
    dones[drow] = p_d[0];
  }
}

// ---------------------------------------------------------------------------
// K4: fused tanh-squashed Gaussian sample + log-prob (fwd + bwd).
// One thread per batch row; A = action_dim <= 32.
// ---------------------------------------------------------------------------
// d clamp(x, -20, 2) / dx for the backward: 1 inside, 0 outside, and the
// NaN itself for a NaN x, so that it reaches the gradient
__device__ __forceinline__ float dsac_clamp_mask(float raw) {
  return (raw >= -20.f && raw <= 2.f) ? 1.f : (raw != raw ? raw : 0.f);
}

__global__ __launch_bounds__(256) void k_squash_fwd(
    const float* __restrict__ mu, const float* __restrict__ lsr,
    float* __restrict__ eps, float* __restrict__ act,
    float* __restrict__ logp, float* __restrict__ tanh_u,
    float* __restrict__ ls_out, const long long* __restrict__ rng,
    long mu_ld, long ls_ld, int B, int A, float k) {
  // mu/lsr may be strided row views (the (mu|lsr) head output sliced in
  // half) — reading through the stride kills the .contiguous() copies
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= B) return;
  constexpr float C = 0.9189385332046727f;  // 0.5*log(2*pi)
  float lp = 0.f;
  for (int a = 0; a < A; ++a) {
    const long idx = (long)i * A + a;
    // fminf/fmaxf return the other operand for a NaN: a NaN log-std must
    // stay one (torch.clamp), or it leaves here as a finite logp
    const float raw = lsr[(long)i * ls_ld + a];
    const float ls = raw != raw ? raw : fminf(fmaxf(raw, -20.f), 2.f);
    const float s = __expf(ls);
    float e;
    if (rng != nullptr) {
      // Box-Muller from two hashed uniforms; eps SAVED for the backward
      const unsigned long long c = (unsigned long long)rng[0];
      const unsigned long long h1 = dsac_sm64(
          c * 0x100000001ull + (unsigned long long)idx * 2ull + 0x1ull);
      const unsigned long long h2 = dsac_sm64(h1);
      e = sqrtf(-2.f * __logf(dsac_u01(h1)))
          * __cosf(6.283185307179586f * dsac_u01(h2));
      eps[idx] = e;
    } else {
      e = eps[idx];
    }
    const float u = mu[(long)i * mu_ld + a] + s * e;
    const float t = tanhf(u);
    act[idx] = k * t;
    tanh_u[idx] = t;
    ls_out[idx] = ls;
    lp += -0.5f * e * e - ls - C - __logf(k * (1.f - t * t + 1e-6f));
  }
  logp[i] = lp;
}

__global__ __launch_bounds__(256) void k_squash_bwd(
    const float* __restrict__ ga, const float* __restrict__ gl,
    const float* __restrict__ lsr, const float* __restrict__ ls,
    const float* __restrict__ eps, const float* __restrict__ tanh_u,
    float* __restrict__ dmu, float* __restrict__ dlsr,
    int B, int A, float k) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= B) return;
  const float g = gl[i];
  for (int a = 0; a < A; ++a) {
    const long idx = (long)i * A + a;
    const float t = tanh_u[idx];
    const float omt2 = 1.f - t * t;
    const float dlp_du = 2.f * t * omt2 / (omt2 + 1e-6f);
    const float s = __expf(ls[idx]);
    const float e = eps[idx];
    const float du = ga[idx] * k * omt2 + g * dlp_du;   // dL/du
    dmu[idx] = du;
    const float raw = lsr[idx];
    const float mask = dsac_clamp_mask(raw);
    dlsr[idx] = mask * (du * e * s - g);
  }
}

// ---------------------------------------------------------------------------
// K5: y = rs*r + gamma*(1-d)*(min(q1,q2) - alpha*lp).
// alpha comes per-sample from log_alpha[t_i] (one_hots suffix of mtobs) —
// no separate gather matmul (reference learner.get_log_alpha).
// ---------------------------------------------------------------------------
// twin minimum that keeps a NaN: fminf alone returns the other operand, so
// a poisoned critic output would leave here as a valid number (torch.min
// propagates it).  Every non-NaN pair gives fminf's bits.
__device__ __forceinline__ float dsac_min_nan(float a, float b) {
  return a != a ? a : (b != b ? b : fminf(a, b));
}

__global__ __launch_bounds__(256) void k_td_target(
    const float* __restrict__ r, const float* __restrict__ d,
    const float* __restrict__ q1, const float* __restrict__ q2,
    const float* __restrict__ lp, const float* __restrict__ alpha,
    float* __restrict__ y, int n, float gamma, float rs) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  y[i] = rs * r[i] + gamma * (1.f - d[i])
      * (dsac_min_nan(q1[i], q2[i]) - alpha[i] * lp[i]);
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

// K5b: MT variant — per-sample alpha computed in-kernel from
// log_alpha[t_i] (one-hot suffix), removing the gather matmul
// (reference learner.get_log_alpha, MT10…MTSAC/src/learner.py:213-233).
__global__ __launch_bounds__(256) void k_td_target_mt(
    const float* __restrict__ r, const float* __restrict__ d,
    const float* __restrict__ q1, const float* __restrict__ q2,
    const float* __restrict__ lp, const float* __restrict__ onehot,
    const float* __restrict__ log_alpha, float* __restrict__ y,
    int n, int T, int oh_stride, float gamma, float rs) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  int t_i = 0;
  if (T > 1) {
    float best = -1e30f;
    for (int t = 0; t < T; ++t) {
      const float v = onehot[(long)i * oh_stride + t];
      if (v > best) { best = v; t_i = t; }
    }
  }
  const float alpha = __expf(log_alpha[t_i]);
  y[i] = td_target_value(rs, r[i], gamma, d[i],
                         dsac_min_nan(q1[i], q2[i]), alpha, lp[i]);
}

// ---------------------------------------------------------------------------
// K6: fused SAC loss reductions.  Single 256-thread workgroup loops the
// batch; LDS tree reductions.  T <= 32 tasks.
//
// Task machinery (matches reference MT10_Distributed_MTSAC/src/model.py:
// 99-116 and learner.py:213-233 exactly):
//   t_i      = argmax over one-hot suffix of states rows
//   alpha_i  = exp(log_alpha[t_i])           (per-sample temperature)
//   w_raw_i  = softmax(-exp(log_alpha))[t_i] (weighted-loss path)
//   coeff_i  = use_w ? (w_raw_i/sum w_raw)/B : 1/B
//
// The critic loss runs BEFORE the critic Adam step and the actor/alpha
// losses AFTER it (reference update_SAC ordering), so they are separate
// kernel pairs.
// ---------------------------------------------------------------------------

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

// softmax(-exp(log_alpha)) gathered at task t (recomputed per thread; T<=32)
__device__ __forceinline__ float task_weight(const float* __restrict__ la,
                                             int T, int t_i) {
  float mx = -1e30f;
  for (int t = 0; t < T; ++t) mx = fmaxf(mx, -__expf(la[t]));
  float den = 0.f;
  for (int t = 0; t < T; ++t) den += __expf(-__expf(la[t]) - mx);
  return __expf(-__expf(la[t_i]) - mx) / den;
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




// single-workgroup fused variant: 1024 threads cover B<=few-thousand rows
// in <=4 strides, LDS tree reduce, thread 0 writes the FINALIZED values —
// one launch replaces zero + multi-block-atomic fwd + finalize (the
// multi-block version was only ever launch-bound at these batch sizes)
// wavefront sum: 6 DPP/shuffle steps, no LDS, no barrier
__device__ inline float wave_sum64(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

__global__ __launch_bounds__(256) void k_critic_loss_fwd_1wg(
    const float* __restrict__ q1, const float* __restrict__ q2,
    const float* __restrict__ y, const float* __restrict__ onehot,
    const float* __restrict__ log_alpha, float* __restrict__ out,
    int B, int T, int oh_stride, int use_w) {
  __shared__ float part[3][4];
  __shared__ float smw[32];
  const int tid = threadIdx.x;
  if (use_w) fill_task_weights(smw, log_alpha, T);
  if (use_w) __syncthreads();
  float s_l1 = 0.f, s_l2 = 0.f, s_w = 0.f;
  for (int i = tid; i < B; i += 256) {
    const int t_i = task_of_row(onehot, i, oh_stride, T);
    const float w_raw = use_w ? smw[t_i] : 1.f;
    s_w += w_raw;
    const float d1 = y[i] - q1[i], d2 = y[i] - q2[i];
    s_l1 += w_raw * d1 * d1;
    s_l2 += w_raw * d2 * d2;
  }
  // wave-level shuffles + ONE barrier (a 256-thread LDS reduce tree
  // measured 16-19 us from barrier latency alone on one CU)
  s_l1 = wave_sum64(s_l1); s_l2 = wave_sum64(s_l2); s_w = wave_sum64(s_w);
  const int wid = tid >> 6;
  if ((tid & 63) == 0) {
    part[0][wid] = s_l1; part[1][wid] = s_l2; part[2][wid] = s_w;
  }
  __syncthreads();
  if (tid == 0) {
    const float r0 = part[0][0] + part[0][1] + part[0][2] + part[0][3];
    const float r1 = part[1][0] + part[1][1] + part[1][2] + part[1][3];
    const float r2 = part[2][0] + part[2][1] + part[2][2] + part[2][3];
    const float wsum = use_w ? r2 : 1.f;
    const float denom = wsum * (float)B;
    out[3] = r0; out[4] = r1; out[5] = r2;
    out[0] = r0 / denom;
    out[1] = r1 / denom;
    out[2] = wsum;
    out[6] = (r0 + r1) / denom;
  }
}

// bf16 stacked-output variant for the manual backward: dq[2,B] bf16
__global__ __launch_bounds__(256) void k_critic_loss_bwd2(
    const float* __restrict__ q1, const float* __restrict__ q2,
    const float* __restrict__ y, const float* __restrict__ onehot,
    const float* __restrict__ log_alpha, const float* __restrict__ saved,
    unsigned short* __restrict__ dq, int B, int T, int oh_stride,
    int use_w) {
  __shared__ float smw[32];
  if (use_w) fill_task_weights(smw, log_alpha, T);
  __syncthreads();
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= B) return;
  const int t_i = task_of_row(onehot, i, oh_stride, T);
  const float w_raw = use_w ? smw[t_i] : 1.f;
  const float coeff = (use_w ? w_raw / saved[2] : 1.f) / (float)B;
  auto cvt = [](float f) -> unsigned short {
    // native v_cvt_pk_bf16_f32: round to nearest even, and a NaN stays a
    // NaN (the integer rounding add carried some into Inf or zero)
    return __builtin_bit_cast(unsigned short, (__bf16)f);
  };
  dq[i] = cvt(coeff * -2.f * (y[i] - q1[i]));
  dq[B + i] = cvt(coeff * -2.f * (y[i] - q2[i]));
}

// dq1_i = g1 * coeff_i * -2 (y_i - q1_i);  dq2 likewise with g2
__global__ __launch_bounds__(256) void k_critic_loss_bwd(
    const float* __restrict__ q1, const float* __restrict__ q2,
    const float* __restrict__ y, const float* __restrict__ onehot,
    const float* __restrict__ log_alpha, const float* __restrict__ saved,
    const float* __restrict__ gscale, float* __restrict__ dq1,
    float* __restrict__ dq2, int B, int T, int oh_stride, int use_w) {
  __shared__ float smw[32];
  if (use_w) fill_task_weights(smw, log_alpha, T);
  __syncthreads();
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= B) return;
  const int t_i = task_of_row(onehot, i, oh_stride, T);
  const float w_raw = use_w ? smw[t_i] : 1.f;
  const float coeff = (use_w ? w_raw / saved[2] : 1.f) / (float)B;
  dq1[i] = gscale[0] * coeff * -2.f * (y[i] - q1[i]);
  dq2[i] = gscale[1] * coeff * -2.f * (y[i] - q2[i]);
}



// single-workgroup fused variant (see k_critic_loss_fwd_1wg); writes
// finalized out[0..3] + raw sums out[4..7] in one launch.  If dla is
// non-null its first dla_n floats are zeroed here — the alpha gradient
// buffer the subsequent k_actor_alpha_loss_bwd* kernels add their
// fixed-order per-task sums to — so the engine needs no separate fill
// launch either.
// multi-block variant: each block reduces its stripe with wave shuffles
// (one barrier), writes a private partial slot in ws, and the LAST block
// (ticket in ws[0], self-resetting so graph replays stay correct) sums
// the slots and writes the finalized outputs.  One launch, full CU
// parallelism — the 1wg variant above is the fallback when no workspace
// is provided (eager/legacy callers) and is latency-bound at ~4 waves.
__global__ __launch_bounds__(256) void k_critic_loss_fwd_mb(
    const float* __restrict__ q1, const float* __restrict__ q2,
    const float* __restrict__ y, const float* __restrict__ onehot,
    const float* __restrict__ log_alpha, float* __restrict__ out,
    float* __restrict__ ws, int B, int T, int oh_stride, int use_w) {
  __shared__ float part[3][4];
  __shared__ float smw[32];
  const int tid = threadIdx.x;
  if (use_w) fill_task_weights(smw, log_alpha, T);
  if (use_w) __syncthreads();
  float s_l1 = 0.f, s_l2 = 0.f, s_w = 0.f;
  for (int i = blockIdx.x * 256 + tid; i < B; i += 256 * gridDim.x) {
    const int t_i = task_of_row(onehot, i, oh_stride, T);
    const float w_raw = use_w ? smw[t_i] : 1.f;
    s_w += w_raw;
    const float d1 = y[i] - q1[i], d2 = y[i] - q2[i];
    s_l1 += w_raw * d1 * d1;
    s_l2 += w_raw * d2 * d2;
  }
  s_l1 = wave_sum64(s_l1); s_l2 = wave_sum64(s_l2); s_w = wave_sum64(s_w);
  const int wid = tid >> 6;
  if ((tid & 63) == 0) {
    part[0][wid] = s_l1; part[1][wid] = s_l2; part[2][wid] = s_w;
  }
  __syncthreads();
  if (tid == 0) {
    float* slots = ws + 1;
    slots[blockIdx.x * 3 + 0] =
        part[0][0] + part[0][1] + part[0][2] + part[0][3];
    slots[blockIdx.x * 3 + 1] =
        part[1][0] + part[1][1] + part[1][2] + part[1][3];
    slots[blockIdx.x * 3 + 2] =
        part[2][0] + part[2][1] + part[2][2] + part[2][3];
    __threadfence();
    const unsigned old = atomicAdd((unsigned*)ws, 1u);
    if (old == (unsigned)gridDim.x - 1u) {
      *(unsigned*)ws = 0u;  // reset the ticket for the next replay
      __threadfence();
      float r0 = 0.f, r1 = 0.f, r2 = 0.f;
      for (int b = 0; b < (int)gridDim.x; ++b) {
        r0 += slots[b * 3 + 0];
        r1 += slots[b * 3 + 1];
        r2 += slots[b * 3 + 2];
      }
      const float wsum = use_w ? r2 : 1.f;
      const float denom = wsum * (float)B;
      out[3] = r0; out[4] = r1; out[5] = r2;
      out[0] = r0 / denom;
      out[1] = r1 / denom;
      out[2] = wsum;
      out[6] = (r0 + r1) / denom;  // logged sum (no separate add launch)
    }
  }
}

__global__ __launch_bounds__(256) void k_actor_alpha_loss_fwd_mb(
    const float* __restrict__ aq1, const float* __restrict__ aq2,
    const float* __restrict__ lp, const float* __restrict__ ls,
    const float* __restrict__ onehot, const float* __restrict__ log_alpha,
    float* __restrict__ out, float* __restrict__ ws,
    float* __restrict__ dla, int dla_n,
    int B, int T, int A, int oh_stride, int use_w, float H_bar) {
  __shared__ float part[4][4];
  __shared__ float smw[32];
  const int tid = threadIdx.x;
  if (blockIdx.x == 0 && dla != nullptr && tid < dla_n) dla[tid] = 0.f;
  if (use_w) fill_task_weights(smw, log_alpha, T);
  if (use_w) __syncthreads();
  constexpr float CE = 1.4189385332046727f;  // 0.5*(1+log(2*pi))
  float s_pl = 0.f, s_w = 0.f, s_al = 0.f, s_en = 0.f;
  for (int i = blockIdx.x * 256 + tid; i < B; i += 256 * gridDim.x) {
    const int t_i = task_of_row(onehot, i, oh_stride, T);
    const float la = log_alpha[t_i];
    const float alpha_i = __expf(la);
    const float w_raw = use_w ? smw[t_i] : 1.f;
    s_w += w_raw;
    const float qmin = dsac_min_nan(aq1[i], aq2[i]);
    s_pl += w_raw * -(qmin - alpha_i * lp[i]);
    s_al += la * (lp[i] + H_bar);
    float ent = CE * A;
    for (int a = 0; a < A; ++a) ent += ls[(long)i * A + a];
    s_en += ent;
  }
  s_pl = wave_sum64(s_pl); s_w = wave_sum64(s_w);
  s_al = wave_sum64(s_al); s_en = wave_sum64(s_en);
  const int wid = tid >> 6;
  if ((tid & 63) == 0) {
    part[0][wid] = s_pl; part[1][wid] = s_w;
    part[2][wid] = s_al; part[3][wid] = s_en;
  }
  __syncthreads();
  if (tid == 0) {
    float* slots = ws + 1;
#pragma unroll
    for (int r = 0; r < 4; ++r)
      slots[blockIdx.x * 4 + r] =
          part[r][0] + part[r][1] + part[r][2] + part[r][3];
    __threadfence();
    const unsigned old = atomicAdd((unsigned*)ws, 1u);
    if (old == (unsigned)gridDim.x - 1u) {
      *(unsigned*)ws = 0u;
      __threadfence();
      float r0 = 0.f, r1 = 0.f, r2 = 0.f, r3 = 0.f;
      for (int b = 0; b < (int)gridDim.x; ++b) {
        r0 += slots[b * 4 + 0]; r1 += slots[b * 4 + 1];
        r2 += slots[b * 4 + 2]; r3 += slots[b * 4 + 3];
      }
      const float wsum = use_w ? r1 : 1.f;
      out[4] = r0; out[5] = r1; out[6] = r2; out[7] = r3;
      out[0] = r0 / (wsum * (float)B);
      out[1] = wsum;
      out[2] = -r2 / (float)B;
      out[3] = r3 / (float)B;
    }
  }
}

__global__ __launch_bounds__(256) void k_actor_alpha_loss_fwd_1wg(
    const float* __restrict__ aq1, const float* __restrict__ aq2,
    const float* __restrict__ lp, const float* __restrict__ ls,
    const float* __restrict__ onehot, const float* __restrict__ log_alpha,
    float* __restrict__ out, float* __restrict__ dla, int dla_n,
    int B, int T, int A, int oh_stride, int use_w, float H_bar) {
  __shared__ float part[4][4];
  __shared__ float smw[32];
  const int tid = threadIdx.x;
  if (dla != nullptr && tid < dla_n) dla[tid] = 0.f;
  if (use_w) fill_task_weights(smw, log_alpha, T);
  if (use_w) __syncthreads();
  constexpr float CE = 1.4189385332046727f;  // 0.5*(1+log(2*pi))
  float s_pl = 0.f, s_w = 0.f, s_al = 0.f, s_en = 0.f;
  for (int i = tid; i < B; i += 256) {
    const int t_i = task_of_row(onehot, i, oh_stride, T);
    const float la = log_alpha[t_i];
    const float alpha_i = __expf(la);
    const float w_raw = use_w ? smw[t_i] : 1.f;
    s_w += w_raw;
    const float qmin = dsac_min_nan(aq1[i], aq2[i]);
    s_pl += w_raw * -(qmin - alpha_i * lp[i]);
    s_al += la * (lp[i] + H_bar);
    float ent = CE * A;
    for (int a = 0; a < A; ++a) ent += ls[(long)i * A + a];
    s_en += ent;
  }
  s_pl = wave_sum64(s_pl); s_w = wave_sum64(s_w);
  s_al = wave_sum64(s_al); s_en = wave_sum64(s_en);
  const int wid = tid >> 6;
  if ((tid & 63) == 0) {
    part[0][wid] = s_pl; part[1][wid] = s_w;
    part[2][wid] = s_al; part[3][wid] = s_en;
  }
  __syncthreads();
  if (tid == 0) {
    const float r0 = part[0][0] + part[0][1] + part[0][2] + part[0][3];
    const float r1 = part[1][0] + part[1][1] + part[1][2] + part[1][3];
    const float r2 = part[2][0] + part[2][1] + part[2][2] + part[2][3];
    const float r3 = part[3][0] + part[3][1] + part[3][2] + part[3][3];
    const float wsum = use_w ? r1 : 1.f;
    out[4] = r0; out[5] = r1; out[6] = r2; out[7] = r3;
    out[0] = r0 / (wsum * (float)B);
    out[1] = wsum;
    out[2] = -r2 / (float)B;
    out[3] = r3 / (float)B;
  }
}

// Per-task alpha gradient dla[t] += gal * -(1/B) sum_{i in t}(lp_i + H_bar),
// reduced by ONE 256-thread block over all B rows in a fixed order, so the
// result is bit-identical from run to run (float atomics are not: their
// order varies, and the last-bit difference in log_alpha then feeds every
// later update).  Each thread adds its rows (stride 256, ascending) into a
// private LDS column; each task's 256 columns are then summed by one wave
// in a fixed tree.  The k_actor_alpha_loss_bwd* kernels run it in one
// extra block (the last of the grid), beside the elementwise blocks.
// T <= 32 (checked on the host); the columns live in dynamic LDS, T*256
// floats given at launch (none when the workspace path is taken).
__device__ __forceinline__ void alpha_grad_block(
    const float* __restrict__ lp, const float* __restrict__ onehot,
    float* __restrict__ dla, float gal, int B, int T, int oh_stride,
    float H_bar) {
  extern __shared__ float s_acc[];
  const int tid = threadIdx.x;
  for (int t = 0; t < T; ++t) s_acc[t * 256 + tid] = 0.f;
  // KR rows per thread at a time, the task argmax (same rule as
  // task_of_row: first maximum wins) scanned t-outer / row-inner so the
  // loads of one step are independent and overlap: the block takes a few
  // memory round trips, not B/256 * T of them.  Rows past B are clamped
  // for the loads and contribute +0.
  constexpr int KR = 8;
  for (int base = 0; base < B; base += 256 * KR) {
    float best[KR], term[KR];
    int ti[KR];
    long row[KR];
#pragma unroll
    for (int k = 0; k < KR; ++k) {
      const int i = base + k * 256 + tid;
      row[k] = (long)(i < B ? i : B - 1);
      term[k] = i < B ? gal * -(lp[row[k]] + H_bar) / (float)B : 0.f;
      best[k] = -1e30f;
      ti[k] = 0;
    }
    if (T > 1) {
#pragma unroll 4
      for (int t = 0; t < T; ++t) {
#pragma unroll
        for (int k = 0; k < KR; ++k) {
          const float v = onehot[row[k] * oh_stride + t];
          if (v > best[k]) { best[k] = v; ti[k] = t; }
        }
      }
    }
#pragma unroll
    for (int k = 0; k < KR; ++k) s_acc[ti[k] * 256 + tid] += term[k];
  }
  __syncthreads();
  const int wid = tid >> 6, lane = tid & 63;
  for (int t = wid; t < T; t += 4) {
    const float* c = s_acc + t * 256;
    float v = (c[lane] + c[lane + 64]) + (c[lane + 128] + c[lane + 192]);
    v = wave_sum64(v);
    if (lane == 0) dla[t] += v;
  }
}

// daq1_i = gp*coeff_i*-(aq1<=aq2); daq2_i = gp*coeff_i*-(aq2<aq1)
// dlp_i  = gp*coeff_i*alpha_i      (alpha detached in actor loss)
// dla[t] = gal * -(1/B) sum_{i in t}(lp_i + H_bar)   (lp detached)
// grid = ceil(B/256) elementwise blocks + 1 alpha-gradient block
__global__ __launch_bounds__(256) void k_actor_alpha_loss_bwd(
    const float* __restrict__ aq1, const float* __restrict__ aq2,
    const float* __restrict__ lp, const float* __restrict__ onehot,
    const float* __restrict__ log_alpha, const float* __restrict__ saved,
    const float* __restrict__ gscale, float* __restrict__ daq1,
    float* __restrict__ daq2, float* __restrict__ dlp,
    float* __restrict__ dla, int B, int T, int oh_stride, int use_w,
    float H_bar) {
  if (blockIdx.x == gridDim.x - 1) {
    alpha_grad_block(lp, onehot, dla, gscale[1], B, T, oh_stride, H_bar);
    return;
  }
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  __shared__ float smw[32];
  if (use_w) fill_task_weights(smw, log_alpha, T);
  __syncthreads();
  if (i < B) {
    const float gp = gscale[0];
    const int t_i = task_of_row(onehot, i, oh_stride, T);
    const float alpha_i = __expf(log_alpha[t_i]);
    const float w_raw = use_w ? smw[t_i] : 1.f;
    const float coeff = (use_w ? w_raw / saved[1] : 1.f) / (float)B;
    const bool first = aq1[i] <= aq2[i];
    daq1[i] = first ? gp * coeff * -1.f : 0.f;
    daq2[i] = first ? 0.f : gp * coeff * -1.f;
    dlp[i] = gp * coeff * alpha_i;
  }
}

// manual-backward actor/alpha variant: daq[2,B] bf16 stacked, dlp fp32,
// dla accumulated into the caller buffer (zeroed by caller).  Without a
// workspace: same grid as above (extra alpha-gradient block).  With ws
// (1 ticket + gridDim*T floats, ticket zero on entry and self-resetting
// like k_*_loss_fwd_mb): grid = ceil(B/256); every block reduces its own
// 256 rows per task in a fixed order into its ws slots — reusing the task
// index it needs anyway — and the LAST block adds the slots to dla in
// block order.  Also bit-identical from run to run, with no serial scan.
__global__ __launch_bounds__(256) void k_actor_alpha_loss_bwd2(
    const float* __restrict__ aq1, const float* __restrict__ aq2,
    const float* __restrict__ lp, const float* __restrict__ onehot,
    const float* __restrict__ log_alpha, const float* __restrict__ saved,
    unsigned short* __restrict__ daq, float* __restrict__ dlp,
    float* __restrict__ dla, float* __restrict__ ws, int B, int T,
    int oh_stride, int use_w, float H_bar) {
  if (ws == nullptr && blockIdx.x == gridDim.x - 1) {
    alpha_grad_block(lp, onehot, dla, 1.f, B, T, oh_stride, H_bar);
    return;
  }
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  const int tid = threadIdx.x;
  __shared__ float smw[32];
  __shared__ float s_val[256];
  __shared__ int s_t[256];
  __shared__ int s_last;
  if (use_w) fill_task_weights(smw, log_alpha, T);
  if (ws != nullptr) {
    s_t[tid] = -1;
    s_val[tid] = 0.f;
    if (i < B) {
      s_t[tid] = task_of_row(onehot, i, oh_stride, T);
      s_val[tid] = -(lp[i] + H_bar) / (float)B;
    }
  }
  __syncthreads();
  // elementwise part first: its loads overlap the reduction below
  if (i < B) {
    const int t_i = ws != nullptr ? s_t[tid]
                                  : task_of_row(onehot, i, oh_stride, T);
    const float alpha_i = __expf(log_alpha[t_i]);
    const float w_raw = use_w ? smw[t_i] : 1.f;
    const float coeff = (use_w ? w_raw / saved[1] : 1.f) / (float)B;
    const bool first = aq1[i] <= aq2[i];
    auto cvt = [](float f) -> unsigned short {
      // native v_cvt_pk_bf16_f32: round to nearest even, and a NaN stays a
      // NaN (the integer rounding add carried some into Inf or zero)
      return __builtin_bit_cast(unsigned short, (__bf16)f);
    };
    daq[i] = cvt(first ? coeff * -1.f : 0.f);
    daq[B + i] = cvt(first ? 0.f : coeff * -1.f);
    dlp[i] = coeff * alpha_i;
  }
  if (ws != nullptr) {
    float* slots = ws + 1 + (long)blockIdx.x * T;
    const int wid = tid >> 6, lane = tid & 63;
    for (int t = wid; t < T; t += 4) {
      float v = ((s_t[lane] == t ? s_val[lane] : 0.f) +
                 (s_t[lane + 64] == t ? s_val[lane + 64] : 0.f)) +
                ((s_t[lane + 128] == t ? s_val[lane + 128] : 0.f) +
                 (s_t[lane + 192] == t ? s_val[lane + 192] : 0.f));
      v = wave_sum64(v);
      if (lane == 0) { slots[t] = v; __threadfence(); }
    }
    __syncthreads();
    if (tid == 0) {
      __threadfence();
      const unsigned old = atomicAdd((unsigned*)ws, 1u);
      s_last = (old == (unsigned)gridDim.x - 1u);
      if (s_last) { *(unsigned*)ws = 0u; __threadfence(); }
    }
    __syncthreads();
    if (s_last && tid < T) {
      const volatile float* all = ws + 1;
      float r = 0.f;
      for (int b = 0; b < (int)gridDim.x; ++b) r += all[(long)b * T + tid];
      dla[tid] += r;
    }
  }
}

// squash backward emitting the joined actor-head gradient [B, 2A] bf16
// ([dmu | dlog_std_raw] — the mu_log_std_layer output layout)
__global__ __launch_bounds__(256) void k_squash_bwd2(
    const float* __restrict__ ga, const float* __restrict__ gl,
    const float* __restrict__ lsr, const float* __restrict__ ls,
    const float* __restrict__ eps, const float* __restrict__ tanh_u,
    unsigned short* __restrict__ dhead, long lsr_ld, int ga_twin, int B,
    int A, float k) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= B) return;
  const float g = gl[i];
  auto cvt = [](float f) -> unsigned short {
    // native v_cvt_pk_bf16_f32: round to nearest even, and a NaN stays a
    // NaN (the integer rounding add carried some into Inf or zero)
    return __builtin_bit_cast(unsigned short, (__bf16)f);
  };
  for (int a = 0; a < A; ++a) {
    const long idx = (long)i * A + a;
    const float t = tanh_u[idx];
    const float omt2 = 1.f - t * t;
    const float dlp_du = 2.f * t * omt2 / (omt2 + 1e-6f);
    const float s = __expf(ls[idx]);
    const float e = eps[idx];
    // ga_twin: ga is the [2,B,A] action-column grad straight from the
    // twin-critic chain backward; summing the two heads here kills the
    // dx0[0]+dx0[1] add launch
    const float gav = ga_twin ? ga[idx] + ga[(long)B * A + idx] : ga[idx];
    const float du = gav * k * omt2 + g * dlp_du;
    const float raw = lsr[(long)i * lsr_ld + a];
    const float mask = dsac_clamp_mask(raw);
    dhead[(long)i * 2 * A + a] = cvt(du);
    dhead[(long)i * 2 * A + A + a] = cvt(mask * (du * e * s - g));
  }
}

__device__ __forceinline__ unsigned short f32_bf16_rne_d(float f) {
  // native v_cvt_pk_bf16_f32: round to nearest even, and a NaN stays a
  // NaN (the integer rounding add carried some into Inf or zero)
  return __builtin_bit_cast(unsigned short, (__bf16)f);
}

// ---------------------------------------------------------------------------
// Fused tail kernels: each folds a chain of strictly dependent neighbours
// above into one launch.  The arithmetic and every reduction order are
// those of the kernels they replace, so the results are bit-identical.
// ---------------------------------------------------------------------------

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

// K5b + K6 critic forward + backward in one launch: TD target, weighted MSE
// sums (per-block slots, self-resetting ticket, last block finalizes in
// block order — as k_critic_loss_fwd_mb) and dq[2,B] bf16 (as
// k_critic_loss_bwd2).  grid = ceil(B/256) <= 32, i.e. B <= 8192.
__global__ __launch_bounds__(256) void k_critic_td_loss(
    const float* __restrict__ r, const float* __restrict__ d,
    const float* __restrict__ q1t, const float* __restrict__ q2t,
    const float* __restrict__ nlp, const float* __restrict__ q1,
    const float* __restrict__ q2, const float* __restrict__ onehot,
    const float* __restrict__ log_alpha, float* __restrict__ out,
    float* __restrict__ ws, unsigned short* __restrict__ dq,
    int B, int T, int oh_stride, int use_w, float gamma, float rs) {
  __shared__ float part[3][4];
  __shared__ float smw[32];
  __shared__ float wpart[32][4];
  __shared__ float s_fin[32 * 3];
  __shared__ int s_last;
  const int tid = threadIdx.x;
  const int i = blockIdx.x * 256 + tid;
  // the row's operands first (row clamped, so the loads are unconditional
  // and in flight during the weight-sum recompute)
  const long ic = i < B ? i : B - 1;
  const float rv = r[ic], dv = d[ic], q1tv = q1t[ic], q2tv = q2t[ic];
  const float lpv = nlp[ic], q1v = q1[ic], q2v = q2[ic];
  int t_i = 0;
  float wsum = 1.f;
  if (use_w) {
    fill_task_weights(smw, log_alpha, T);
    __syncthreads();
    wsum = batch_weight_sum(smw, onehot, wpart, B, T, oh_stride,
                            (int)gridDim.x, t_i);
  } else {
    t_i = task_of_row(onehot, ic, oh_stride, T);
  }
  float s_l1 = 0.f, s_l2 = 0.f, s_w = 0.f;
  if (i < B) {
    const float alpha = __expf(log_alpha[t_i]);
    const float y = td_target_value(rs, rv, gamma, dv,
                                    dsac_min_nan(q1tv, q2tv), alpha, lpv);
    const float w_raw = use_w ? smw[t_i] : 1.f;
    s_w += w_raw;
    const float d1 = y - q1v, d2 = y - q2v;
    s_l1 += w_raw * d1 * d1;
    s_l2 += w_raw * d2 * d2;
    const float coeff = (use_w ? w_raw / wsum : 1.f) / (float)B;
    dq[i] = f32_bf16_rne_d(coeff * -2.f * (y - q1v));
    dq[B + i] = f32_bf16_rne_d(coeff * -2.f * (y - q2v));
  }
  s_l1 = wave_sum64(s_l1); s_l2 = wave_sum64(s_l2); s_w = wave_sum64(s_w);
  const int wid = tid >> 6;
  if ((tid & 63) == 0) {
    part[0][wid] = s_l1; part[1][wid] = s_l2; part[2][wid] = s_w;
  }
  __syncthreads();
  float* slots = ws + 1;
  if (tid == 0) {
    slots[blockIdx.x * 3 + 0] =
        part[0][0] + part[0][1] + part[0][2] + part[0][3];
    slots[blockIdx.x * 3 + 1] =
        part[1][0] + part[1][1] + part[1][2] + part[1][3];
    slots[blockIdx.x * 3 + 2] =
        part[2][0] + part[2][1] + part[2][2] + part[2][3];
    __threadfence();
    const unsigned old = atomicAdd((unsigned*)ws, 1u);
    s_last = (old == (unsigned)gridDim.x - 1u);
    if (s_last) {
      *(unsigned*)ws = 0u;  // reset the ticket for the next replay
      __threadfence();
    }
  }
  __syncthreads();
  if (!s_last) return;
  // last block: one parallel read of every slot (a serial scan costs a
  // memory round trip per slot), then the sums in block order
  const int nb = (int)gridDim.x;
  if (tid < nb * 3) s_fin[tid] = ((const volatile float*)slots)[tid];
  __syncthreads();
  if (tid == 0) {
    float r0 = 0.f, r1 = 0.f, r2 = 0.f;
    for (int b = 0; b < nb; ++b) {
      r0 += s_fin[b * 3 + 0];
      r1 += s_fin[b * 3 + 1];
      r2 += s_fin[b * 3 + 2];
    }
    const float wfin = use_w ? r2 : 1.f;
    const float denom = wfin * (float)B;
    out[3] = r0; out[4] = r1; out[5] = r2;
    out[0] = r0 / denom;
    out[1] = r1 / denom;
    out[2] = wfin;
    out[6] = (r0 + r1) / denom;
  }
}

// ---------------------------------------------------------------------------
// Prioritized replay (opt-in; docs/KERNELS.md "Prioritized replay"; the exact
// oracle is torch_ref.per_*).  Leaves prio[T, cap] (0 = never written), block
// sums bsum[T, nb] over PER_BLOCK leaves each, total[T], max_prio[T].  Sums
// are only ever RECOMPUTED from what they cover, in one fixed order, so
// "bsum = fixed-order sum of its leaves, total = fixed-order sum of the
// shard's bsum" holds bit for bit.
//
// The fixed order over n values, by one 256-thread block: thread i adds
// v[i], v[i + 256], v[i + 512], ... in that order, then the 256 partials
// fold by halves (i with i + 128, then + 64, ... + 1).
// ---------------------------------------------------------------------------
constexpr int PER_BLOCK = 1024;

// fold of 256 per-thread partials; the result is valid in thread 0.  Every
// thread of the block must call it.
__device__ __forceinline__ float per_fold256(float acc, float* s) {
  const int tid = threadIdx.x;
  __syncthreads();   // a previous fold may still be reading s
  s[tid] = acc;
  __syncthreads();
  float v = 0.f;
  if (tid < 64) {
    v = (s[tid] + s[tid + 128]) + (s[tid + 64] + s[tid + 192]);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  }
  return v;
}

// The same fixed order by ONE wave, without LDS: lane l forms the partials
// l, l + 64, l + 128, l + 192 itself, folds them ((l, l + 128) and
// (l + 64, l + 192) are the first two halvings), then the wave folds by
// halves.  The result is valid in lane 0.
template <bool VOLATILE>
__device__ __forceinline__ float per_wave_fixed_sum(const float* p, int n,
                                                    int lane) {
  float a[4] = {0.f, 0.f, 0.f, 0.f};
  // 1024 values at a time: 16 independent loads per lane (values past n
  // read as 0, which adds exactly), then the adds in the fixed order
  for (int s0 = 0; s0 < n; s0 += 1024) {
    float vv[4][4];
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int k = s0 + r * 256 + q * 64 + lane;
        vv[r][q] = k >= n ? 0.f
            : (VOLATILE ? ((const volatile float*)p)[k] : p[k]);
      }
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
      for (int q = 0; q < 4; ++q) a[q] += vv[r][q];
  }
  float v = (a[0] + a[2]) + (a[1] + a[3]);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  return v;
}

// Non-blocking "last block finalises": every block counts itself in after
// its bsum stores; the last one recomputes total[t0 .. t0 + nt) from the
// block sums (one wave per shard) and resets the ticket.  Every thread of
// the block must call it; any block size that is a multiple of 64.
__device__ __forceinline__ void per_finish_totals(
    const float* bsum, float* total, unsigned* ticket, int nb, int t0, int nt,
    int* s_last) {
  const int tid = threadIdx.x;
  __syncthreads();
  if (tid == 0) {
    __threadfence();
    const unsigned old = atomicAdd(ticket, 1u);
    *s_last = (old == gridDim.x * gridDim.y - 1u);
    if (*s_last) {
      *ticket = 0u;
      __threadfence();
    }
  }
  __syncthreads();
  if (!*s_last) return;
  const int lane = tid & 63;
  for (int t = t0 + (tid >> 6); t < t0 + nt; t += (int)(blockDim.x >> 6)) {
    const float v = per_wave_fixed_sum<true>(bsum + (long)t * nb, nb, lane);
    if (lane == 0) total[t] = v;
  }
}

// Hillis-Steele inclusive scan over the wave (lane l adds lane l - off for
// off = 1, 2, 4, ... 32): the association torch_ref._hs_scan64 reproduces.
__device__ __forceinline__ float per_wave_scan(float v, int lane) {
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const float o = __shfl_up(v, off, 64);
    if (lane >= off) v = __fadd_rn(v, o);
  }
  return v;
}

// First k in [0, n) with p[k] > 0 whose inclusive prefix sum exceeds x, by
// the whole wave: chunks of 64 coalesced loads, a wave scan each, a running
// base.  Returns -1 if there is none; then last_nz is the last k with
// p[k] > 0 (-1: none).  On a hit, excl is the prefix before k and val p[k].
// All arguments and results are wave-uniform.
__device__ __forceinline__ int per_wave_search(const float* p, int n, float x,
                                               int lane, float& excl,
                                               float& val, int& last_nz) {
  float base = 0.f;
  last_nz = -1;
  // 16 chunks are loaded at once (independent loads, one memory latency
  // instead of one per chunk), then scanned in order
  for (int s0 = 0; s0 < n; s0 += 16 * 64) {
    float vv[16];
#pragma unroll
    for (int c = 0; c < 16; ++c) {
      const int k = s0 + c * 64 + lane;
      vv[c] = k < n ? p[k] : 0.f;
    }
#pragma unroll
    for (int c = 0; c < 16; ++c) {
      const int c0 = s0 + c * 64;
      if (c0 >= n) break;
      const float v = vv[c];
      const float incl = __fadd_rn(base, per_wave_scan(v, lane));
      const unsigned long long nz = __ballot(v > 0.f);
      const unsigned long long hit = __ballot(incl > x && v > 0.f);
      if (hit != 0ull) {
        const int l = __ffsll((long long)hit) - 1;
        const float prev = __shfl(incl, l > 0 ? l - 1 : 0, 64);
        excl = l > 0 ? prev : base;
        val = __shfl(v, l, 64);
        return c0 + l;
      }
      if (nz != 0ull) last_nz = c0 + 63 - __clzll((long long)nz);
      base = __shfl(incl, 63, 64);
    }
  }
  return -1;
}

// K12d: stratified PROPORTIONAL draw + gather.  One wave per batch row, as
// k_replay_sample; the row index is wave-uniform (readfirstlane), so the two
// searches cannot diverge.  Row j of shard t draws from the j-th of `per`
// equal slices of the shard's priority mass:
//   x = (float(j) + u) * (total_t / float(per))      (fp32, RN, this order)
// with u the uniform k_replay_sample derives for batch row i.  It gathers
// the first row whose inclusive prefix sum exceeds x: first the block (scan
// of bsum), then, with x minus the prefix before that block, the leaf.  When
// rounding leaves no such block / leaf, the last one with a non-zero sum /
// priority is taken.  Raw IS weight (n_t * p / total_t) ** -beta.  An empty
// shard yields row 0 and weight 1.
__global__ __launch_bounds__(256) void k_replay_sample_per(
    const float* __restrict__ states, const float* __restrict__ actions,
    const float* __restrict__ rewards, const float* __restrict__ next_states,
    const float* __restrict__ dones, const float* __restrict__ sizes,
    const float* __restrict__ prio, const float* __restrict__ bsum,
    const float* __restrict__ total, const float* __restrict__ beta,
    const long long* __restrict__ rng, float* __restrict__ o_states,
    float* __restrict__ o_actions, float* __restrict__ o_rewards,
    float* __restrict__ o_next_states, float* __restrict__ o_dones,
    long long* __restrict__ idx_out, float* __restrict__ w_out, int B, int T,
    int per, long cap, int nb, int Ds, int Da) {
  const int i = __builtin_amdgcn_readfirstlane(
      (int)(blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6)));
  const int lane = threadIdx.x & 63;
  if (i >= B) return;
  const int t = min(i / per, T - 1);
  const int j = i - t * per;
  const unsigned long long c = (unsigned long long)rng[0];
  float u = dsac_u01(dsac_sm64(c * 0x100000001ull
                               + (unsigned long long)i * 2ull + 0x2ull));
  u = u < 1.f ? u : 0.99999994f;
  const float n = fminf(sizes[t], (float)cap);
  const float tot = total[t];
  long idx = 0;
  float w = 1.f;
  if (n >= 1.f && tot > 0.f) {
    const float x = __fmul_rn(__fadd_rn((float)j, u),
                              __fdiv_rn(tot, (float)per));
    float excl = 0.f, val = 0.f;
    int last = -1;
    int b = per_wave_search(bsum + (long)t * nb, nb, x, lane, excl, val,
                            last);
    float xr;
    if (b < 0) {
      b = last > 0 ? last : 0;
      xr = INFINITY;
    } else {
      xr = __fsub_rn(x, excl);
    }
    const long base = (long)b * PER_BLOCK;
    const int nl = (int)(cap - base < PER_BLOCK ? cap - base : PER_BLOCK);
    const float* lp = prio + (long)t * cap + base;
    int l = per_wave_search(lp, nl, xr, lane, excl, val, last);
    if (l < 0) {
      l = last > 0 ? last : 0;
      val = lp[l];
    }
    idx = base + l;
    if (val > 0.f)
      w = powf(__fdiv_rn(__fmul_rn(n, val), tot), -beta[0]);
  }
  const long src = (long)t * cap + idx;
  for (int k = lane; k < Ds; k += 64) {
    o_states[(long)i * Ds + k] = states[src * Ds + k];
    o_next_states[(long)i * Ds + k] = next_states[src * Ds + k];
  }
  for (int k = lane; k < Da; k += 64)
    o_actions[(long)i * Da + k] = actions[src * Da + k];
  if (lane == 0) {
    o_rewards[i] = rewards[src];
    o_dones[i] = dones[src];
    idx_out[i] = src;
    w_out[i] = w;
  }
}

// k_critic_td_loss with importance-sampling weights: every per-row squared
// error and dq coefficient is multiplied by isw[i] / max_j isw[j] (each block
// recomputes the batch maximum: <= 8192 floats, order-independent).  The
// task-weight normaliser (out[2], out[5]) is the unweighted one, so equal
// IS weights reproduce k_critic_td_loss bit for bit.  Also writes each row's
// new priority (0.5 (|y - q1| + |y - q2|) + eps) ** alpha and, given the
// leaves and the rows' flat indices, zeroes the sampled leaves so that
// k_per_max can max the new values in.
__global__ __launch_bounds__(256) void k_critic_td_loss_per(
    const float* __restrict__ r, const float* __restrict__ d,
    const float* __restrict__ q1t, const float* __restrict__ q2t,
    const float* __restrict__ nlp, const float* __restrict__ q1,
    const float* __restrict__ q2, const float* __restrict__ onehot,
    const float* __restrict__ log_alpha, float* __restrict__ out,
    float* __restrict__ ws, unsigned short* __restrict__ dq,
    int B, int T, int oh_stride, int use_w, float gamma, float rs,
    const float* __restrict__ isw, float* __restrict__ newp,
    float* __restrict__ prio, const long long* __restrict__ idx, long n_prio,
    float per_alpha, float per_eps) {
  __shared__ float part[3][4];
  __shared__ float smw[32];
  __shared__ float wpart[32][4];
  __shared__ float s_fin[32 * 3];
  __shared__ float s_max[4];
  __shared__ int s_last;
  const int tid = threadIdx.x;
  const int i = blockIdx.x * 256 + tid;
  const long ic = i < B ? i : B - 1;
  const float rv = r[ic], dv = d[ic], q1tv = q1t[ic], q2tv = q2t[ic];
  const float lpv = nlp[ic], q1v = q1[ic], q2v = q2[ic];
  const float iswv = isw[ic];
  float m = 0.f;
  for (int k = tid; k < B; k += 256) m = fmaxf(m, isw[k]);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1)
    m = fmaxf(m, __shfl_xor(m, off, 64));
  if ((tid & 63) == 0) s_max[tid >> 6] = m;
  __syncthreads();
  const float wmax = fmaxf(fmaxf(s_max[0], s_max[1]),
                           fmaxf(s_max[2], s_max[3]));
  const float isn = wmax > 0.f ? iswv / wmax : 1.f;
  int t_i = 0;
  float wsum = 1.f;
  if (use_w) {
    fill_task_weights(smw, log_alpha, T);
    __syncthreads();
    wsum = batch_weight_sum(smw, onehot, wpart, B, T, oh_stride,
                            (int)gridDim.x, t_i);
  } else {
    t_i = task_of_row(onehot, ic, oh_stride, T);
  }
  float s_l1 = 0.f, s_l2 = 0.f, s_w = 0.f;
  if (i < B) {
    const float alpha = __expf(log_alpha[t_i]);
    const float y = td_target_value(rs, rv, gamma, dv,
                                    dsac_min_nan(q1tv, q2tv), alpha, lpv);
    const float w_raw = use_w ? smw[t_i] : 1.f;
    s_w += w_raw;
    const float wi = w_raw * isn;
    const float d1 = y - q1v, d2 = y - q2v;
    s_l1 += wi * d1 * d1;
    s_l2 += wi * d2 * d2;
    const float coeff = (use_w ? wi / wsum : isn) / (float)B;
    dq[i] = f32_bf16_rne_d(coeff * -2.f * (y - q1v));
    dq[B + i] = f32_bf16_rne_d(coeff * -2.f * (y - q2v));
    newp[i] = powf(0.5f * (fabsf(d1) + fabsf(d2)) + per_eps, per_alpha);
    if (prio != nullptr) {
      const long flat = idx[i];
      if (flat >= 0 && flat < n_prio) prio[flat] = 0.f;
    }
  }
  s_l1 = wave_sum64(s_l1); s_l2 = wave_sum64(s_l2); s_w = wave_sum64(s_w);
  const int wid = tid >> 6;
  if ((tid & 63) == 0) {
    part[0][wid] = s_l1; part[1][wid] = s_l2; part[2][wid] = s_w;
  }
  __syncthreads();
  float* slots = ws + 1;
  if (tid == 0) {
    slots[blockIdx.x * 3 + 0] =
        part[0][0] + part[0][1] + part[0][2] + part[0][3];
    slots[blockIdx.x * 3 + 1] =
        part[1][0] + part[1][1] + part[1][2] + part[1][3];
    slots[blockIdx.x * 3 + 2] =
        part[2][0] + part[2][1] + part[2][2] + part[2][3];
    __threadfence();
    const unsigned old = atomicAdd((unsigned*)ws, 1u);
    s_last = (old == (unsigned)gridDim.x - 1u);
    if (s_last) {
      *(unsigned*)ws = 0u;  // reset the ticket for the next replay
      __threadfence();
    }
  }
  __syncthreads();
  if (!s_last) return;
  const int nb = (int)gridDim.x;
  if (tid < nb * 3) s_fin[tid] = ((const volatile float*)slots)[tid];
  __syncthreads();
  if (tid == 0) {
    float r0 = 0.f, r1 = 0.f, r2 = 0.f;
    for (int b = 0; b < nb; ++b) {
      r0 += s_fin[b * 3 + 0];
      r1 += s_fin[b * 3 + 1];
      r2 += s_fin[b * 3 + 2];
    }
    const float wfin = use_w ? r2 : 1.f;
    const float denom = wfin * (float)B;
    out[3] = r0; out[4] = r1; out[5] = r2;
    out[0] = r0 / denom;
    out[1] = r1 / denom;
    out[2] = wfin;
    out[6] = (r0 + r1) / denom;
  }
}

// Priority write-back, three steps in stream order: the sampled leaves are
// zeroed (k_critic_td_loss_per, or k_per_zero), k_per_max maxes the new
// values in (non-negative floats order as their bit patterns, so an unsigned
// atomicMax is exact and order-independent: a row drawn twice ends with the
// larger value) and raises max_prio, k_per_resum re-sums the touched blocks.
__global__ __launch_bounds__(256) void k_per_zero(
    float* __restrict__ prio, const long long* __restrict__ idx, int B,
    long n_prio) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= B) return;
  const long flat = idx[i];
  if (flat >= 0 && flat < n_prio) prio[flat] = 0.f;
}

__global__ __launch_bounds__(256) void k_per_max(
    float* __restrict__ prio, float* __restrict__ maxp,
    const long long* __restrict__ idx, const float* __restrict__ newp, int B,
    long cap, long n_prio) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  const long flat = i < B ? idx[i] : -1;
  const bool ok = flat >= 0 && flat < n_prio;
  float v = ok ? newp[i] : 0.f;
  v = v > 0.f ? v : 0.f;            // a NaN must not win the bit-pattern max
  if (ok) atomicMax((unsigned*)prio + flat, __float_as_uint(v));
  // max_prio: B atomics on T words would serialise, so each wave first
  // folds its rows shard by shard (a sampled batch is shard-major: one or
  // two shards per wave) and issues one atomic per shard it holds
  const int lane = threadIdx.x & 63;
  int t = ok ? (int)(flat / cap) : -1;
  unsigned long long todo = __ballot(ok);
  while (todo != 0ull) {
    const int cur = __shfl(t, __ffsll((long long)todo) - 1, 64);
    float m = t == cur ? v : 0.f;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1)
      m = fmaxf(m, __shfl_xor(m, off, 64));
    if (lane == 0) atomicMax((unsigned*)maxp + cur, __float_as_uint(m));
    todo &= ~__ballot(t == cur);
  }
}

// one wave per batch row, PER_RESUM_ROWS rows per workgroup (few workgroups:
// the ticket is one atomic per workgroup on one word): re-sums the block the
// row's leaf lies in (a block touched by several rows is re-summed by each,
// to the same bits), then the last workgroup to finish recomputes every
// shard's total.
constexpr int PER_RESUM_ROWS = 16;

__global__ __launch_bounds__(PER_RESUM_ROWS * 64) void k_per_resum(
    const float* prio, float* bsum, float* total, const long long* idx,
    unsigned* ticket, int B, int T, long cap, int nb, long n_prio) {
  __shared__ int s_last;
  const int lane = threadIdx.x & 63;
  const int i = __builtin_amdgcn_readfirstlane(
      (int)(blockIdx.x * PER_RESUM_ROWS + (threadIdx.x >> 6)));
  if (i < B) {
    long flat = idx[i];
    flat = flat < 0 ? 0 : (flat >= n_prio ? n_prio - 1 : flat);
    const long t = flat / cap;
    const long b = (flat - t * cap) / PER_BLOCK;
    const long base = b * PER_BLOCK;
    const int n = (int)(cap - base < PER_BLOCK ? cap - base : PER_BLOCK);
    const float v = per_wave_fixed_sum<false>(prio + t * cap + base, n, lane);
    if (lane == 0) bsum[t * nb + b] = v;
  }
  per_finish_totals(bsum, total, ticket, nb, 0, T, &s_last);
}

// Ingest hook: rows written by ingest receive max_prio[t] of their shard.
// grid = (nb, nt): block (b, y) owns leaf block b of shard t0 + y; if a
// written range meets it, it stores max_prio[t] to the covered leaves and
// re-sums the block from the values it holds.  Ranges: the descriptors of a
// staged packed batch on the device (pk != nullptr: task d[0], rows d[3],
// first row d[5], wrapping), or the one range (t0, r_start, r_rows).
__device__ __forceinline__ bool per_in_range(long row, long start, long rows,
                                             long cap) {
  long d = row - start;
  if (d < 0) d += cap;
  return d < rows;
}

__global__ __launch_bounds__(256) void k_per_ingest(
    const float* __restrict__ pk, int n_desc, int t_hdr, int t0, int r_start,
    int r_rows, float* prio, float* bsum, float* total,
    const float* __restrict__ maxp, unsigned* ticket, long cap, int nb) {
  __shared__ float s[256];
  __shared__ int s_last;
  __shared__ int s_hit;
  const int tid = threadIdx.x;
  const int t = t0 + (int)blockIdx.y;
  const long base = (long)blockIdx.x * PER_BLOCK;
  const int n = (int)(cap - base < PER_BLOCK ? cap - base : PER_BLOCK);
  const int* desc = pk != nullptr
      ? reinterpret_cast<const int*>(pk) + PK_HDR + t_hdr : nullptr;
  const int nd = pk != nullptr ? n_desc : 1;
  if (tid == 0) s_hit = 0;
  __syncthreads();
  for (int k = tid; k < nd; k += 256) {
    const int task = desc ? desc[k * PK_DESC] : t0;
    const long rows = desc ? desc[k * PK_DESC + 3] : r_rows;
    const long start = desc ? desc[k * PK_DESC + 5] : r_start;
    if (task != t || rows < 1) continue;
    // [start, start + rows) mod cap meets [base, base + n)?
    const long end = start + rows;
    const bool a = start < base + n && (end < cap ? end : cap) > base;
    const bool w = end > cap && end - cap > base;
    if (a || w) s_hit = 1;
  }
  __syncthreads();
  if (s_hit) {
    const float mp = maxp[t];
    float acc = 0.f;
    for (int k = tid; k < n; k += 256) {
      const long row = base + k;
      bool in = false;
      for (int q = 0; q < nd && !in; ++q) {
        const int task = desc ? desc[q * PK_DESC] : t0;
        const long rows = desc ? desc[q * PK_DESC + 3] : r_rows;
        const long start = desc ? desc[q * PK_DESC + 5] : r_start;
        in = task == t && per_in_range(row, start, rows, cap);
      }
      float v;
      if (in) {
        prio[(long)t * cap + row] = mp;
        v = mp;
      } else {
        v = prio[(long)t * cap + row];
      }
      acc += v;
    }
    const float v = per_fold256(acc, s);
    if (tid == 0) bsum[(long)t * nb + blockIdx.x] = v;
  }
  per_finish_totals(bsum, total, ticket, nb, t0, (int)gridDim.y, &s_last);
}

// K6 actor/alpha forward + backward in one launch (k_actor_alpha_loss_fwd_mb
// + the workspace path of k_actor_alpha_loss_bwd2).  ws = ticket, 32*4
// metric slots, then gridDim*T alpha-gradient slots; ONE ticket serves both
// finalizations.  dla[0..T) is stored as 0.f + r (the replaced pair zeroes
// it and then adds r), dla[T..dla_n) as 0.f.  grid = ceil(B/256) <= 32.
__global__ __launch_bounds__(256) void k_actor_alpha_loss_fwd_bwd(
    const float* __restrict__ aq1, const float* __restrict__ aq2,
    const float* __restrict__ lp, const float* __restrict__ ls,
    const float* __restrict__ onehot, const float* __restrict__ log_alpha,
    float* __restrict__ out, float* __restrict__ ws,
    unsigned short* __restrict__ daq, float* __restrict__ dlp,
    float* __restrict__ dla, int dla_n, const float* __restrict__ wsum_in,
    int B, int T, int A, int oh_stride, int use_w, float H_bar) {
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
  const float aq1v = aq1[ic], aq2v = aq2[ic], lpv = lp[ic];
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
    const float qmin = dsac_min_nan(aq1v, aq2v);
    s_pl += w_raw * -(qmin - alpha_i * lpv);
    s_al += la * (lpv + H_bar);
    s_en += ent;
    const float coeff = (use_w ? w_raw / wsum : 1.f) / (float)B;
    const bool first = aq1v <= aq2v;
    daq[i] = f32_bf16_rne_d(first ? coeff * -1.f : 0.f);
    daq[B + i] = f32_bf16_rne_d(first ? 0.f : coeff * -1.f);
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

// ---------------------------------------------------------------------------
// K9 / K10 / K11: the optimizer tail.  adam_elem and polyak_elem are the
// ONLY definitions of the two element updates; every path (host step size,
// device step state, split-K arena, several groups, clipping, Polyak alone
// or appended) calls them, so the paths cannot drift apart by a bit.
// ---------------------------------------------------------------------------

// torch.optim.Adam numerics on one element.  The rounding points are
// explicit: left as plain C++, which product fuses into which fma is the
// compiler's choice per kernel.
__device__ __forceinline__ void adam_elem(
    float* p, float* m, float* v, unsigned short* mir, long i, float gi,
    float step_size, float inv_sqrt_bc2, float b1, float b2, float eps) {
  const float m0 = m[i], v0 = v[i], p0 = p[i];   // loads ahead of the stores
  const float mi = __fmaf_rn(1.f - b1, gi, b1 * m0);
  const float vi = __fmaf_rn(gi, (1.f - b2) * gi, b2 * v0);
  m[i] = mi;
  v[i] = vi;
  const float pn =
      p0 - step_size * mi / __fmaf_rn(sqrtf(vi), inv_sqrt_bc2, eps);
  p[i] = pn;
  // the group's bf16 compute mirror, refreshed by the same thread: no
  // separate full-buffer cast launch
  if (mir != nullptr) mir[i] = f32_bf16_rne_d(pn);
}

// t = (1-tau)*t + tau*s, + bf16 mirror
__device__ __forceinline__ void polyak_elem(
    float* t, const float* s, unsigned short* mir, long i, float tau) {
  const float tn = __fmaf_rn(1.f - tau, t[i], tau * s[i]);
  t[i] = tn;
  if (mir != nullptr) mir[i] = f32_bf16_rne_d(tn);
}

// Split-K partials of one gradient, [>=S, stride]: element i is their sum
// from 0.f in s order (k_reduce_arena).
struct Arena { const float* ptr; long stride; int S; };

__device__ __forceinline__ float arena_fold(const Arena& a, long i) {
  float acc = 0.f;
#pragma unroll 8
  for (int s = 0; s < a.S; ++s) acc += a.ptr[(long)s * a.stride + i];
  return acc;
}

// K9 with the step size from the host: the first Adam kernel, which no
// engine steps through any more (adam_step_ is kept for tools and tests).
// The one exception to adam_elem: as plain C++ this kernel was compiled
// with b1*m, not (1-b1)*g, as the fused product of m, and with v as the
// unfused sum of two rounded products.  Its results are kept, so it spells
// out that sequence (profiles/adam_family.md).
__global__ __launch_bounds__(256) void k_adam(
    float* __restrict__ p, const float* __restrict__ g,
    float* __restrict__ m, float* __restrict__ v, long n,
    float b1, float b2, float step_size, float inv_sqrt_bc2, float eps) {
#pragma clang fp contract(off)
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float gi = g[i];
  const float mi = __fmaf_rn(b1, m[i], (1.f - b1) * gi);
  const float vi = b2 * v[i] + ((1.f - b2) * gi) * gi;
  m[i] = mi;
  v[i] = vi;
  p[i] -= step_size * mi / __fmaf_rn(sqrtf(vi), inv_sqrt_bc2, eps);
}

// K10 alone
__global__ __launch_bounds__(256) void k_polyak(
    float* __restrict__ t, const float* __restrict__ s, long n, float tau,
    unsigned short* __restrict__ mir) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  polyak_elem(t, s, mir, i, tau);
}

// Graph-capturable Adam keeps {step, step_size, inv_sqrt_bc2} on-device so
// a captured update's bias correction advances across hipGraph replays.
// One launch advances the state of up to 4 optimizers (a null state is
// skipped) and bumps the device RNG counter: the engine calls it once at
// the top of seg2 and the steppers then skip their own prologs.
__global__ void k_adam_prolog_many(long long* rng,
                                   float* s0, float* s1, float* s2,
                                   float* s3,
                                   float lr0, float lr1, float lr2,
                                   float lr3, float b1, float b2) {
  if (rng != nullptr && threadIdx.x == 0) rng[0] += 1;
  const int i = threadIdx.x;
  float* sv[4] = {s0, s1, s2, s3};
  const float lrv[4] = {lr0, lr1, lr2, lr3};
  if (i >= 4 || sv[i] == nullptr) return;
  float* st = sv[i];
  const float step = st[0] + 1.f;
  st[0] = step;
  st[1] = lrv[i] / (1.f - __powf(b1, step));         // step_size
  st[2] = 1.f / sqrtf(1.f - __powf(b2, step));       // inv_sqrt_bc2
}

// K11: sum of squares of up to three flat gradients, one launch.  Grid
// (GN_SLOTS, ranges) is FIXED, so the summation order depends on n alone:
// block b of a range owns elements b*256+tid + k*GN_SLOTS*256 (k ascending,
// one fp32 accumulator per thread), then wave_sum64, then the four wave
// partials left to right, written to slot [range][b].  GN_SLOTS = 256 blocks
// per range: 64 of them left three quarters of the CUs idle and made the
// flagship's critic fold 100 us long.  No atomics; the launch boundary
// orders the slots for K9.  Range 0 may come as a split-K arena: the folded
// value is stored to the flat gradient and squared.
constexpr int GN_SLOTS = 256;

__global__ __launch_bounds__(256) void k_grad_sumsq(
    float* g0, long n0, const float* g1, long n1, const float* g2, long n2,
    const Arena arena0, float* __restrict__ slots) {
  __shared__ float s_w[4];
  const int r = blockIdx.y, tid = threadIdx.x;
  const float* g = r == 0 ? g0 : (r == 1 ? g1 : g2);
  const long n = r == 0 ? n0 : (r == 1 ? n1 : n2);
  const bool fold = r == 0 && arena0.ptr != nullptr;
  float acc = 0.f;
  for (long i = (long)blockIdx.x * 256 + tid; i < n;
       i += (long)GN_SLOTS * 256) {
    float x;
    if (fold) g0[i] = x = arena_fold(arena0, i);
    else x = g[i];
    acc += x * x;
  }
  acc = wave_sum64(acc);
  if ((tid & 63) == 0) s_w[tid >> 6] = acc;
  __syncthreads();
  if (tid == 0)
    slots[r * GN_SLOTS + blockIdx.x] = ((s_w[0] + s_w[1]) + s_w[2]) + s_w[3];
}

// Everything one k_adam_groups launch works on, passed by value.
struct AdamGroup {
  float* p; float* g; float* m; float* v; const float* st;   // st: state
  unsigned short* mir; long n;
};
struct AdamTable {
  AdamGroup grp[3];          // unused groups: n = 0
  float b1, b2, eps;
  Arena arena0;              // optional: group 0's gradient, folded here
  float* pt; const float* psrc; unsigned short* pmir;   // optional trailing
  long np; float tau;                                   // Polyak range
  // CLIP only: K11's slots, thresholds, published {norm, coef, s}, counters
  const float* slots; float c[3]; float* cs[3]; int* sk[3];
};

template <typename T>
__device__ __forceinline__ T sel3(int k, T a0, T a1, T a2) {
  return k == 0 ? a0 : (k == 1 ? a1 : a2);
}

// K9 (+K10): thread i takes one element of the concatenation of <= 3 Adam
// groups and a trailing Polyak range (whose buffers must not be stepped by
// this launch).  With arena0 set, group 0's gradient is folded from its
// split-K partials and written back to the flat gradient for callers that
// read .grad.
//
// CLIP: the gradients were measured by K11 (which also did the fold).
// Every block re-sums each group's GN_SLOTS slots the same way (lane l adds
// slots l, l+64, l+128, l+192 in that order, then wave_sum64), so all
// blocks derive the same bits: s not finite -> the group's threads leave
// p, m, v and the mirror alone; else coef = min(1, c / (sqrtf(s) + 1e-6))
// (torch clip_grad_norm_) and Adam runs on coef * g.  The flat gradient is
// only read.  Block 0 publishes cs = {norm, coef, s} and bumps the group's
// skip counter.  LDS, the barrier and the atomic exist in this
// instantiation alone, which is why CLIP is not a runtime flag.
//
// ONE: group 0 is all there is (the critic's step).  The group is then the
// same for every lane, so its pointers and its state stay in scalar
// registers; through the general dispatch that launch measured 0.1-0.3 us
// longer (profiles/adam_family.md).
template <bool CLIP, bool ONE>
__global__ __launch_bounds__(256) void k_adam_groups(const AdamTable T) {
  __shared__ float s_coef[3];   // < 0: skip
  const int tid = threadIdx.x;
  if constexpr (CLIP) {
    const int wv = tid >> 6;
    if (wv < 3 && sel3(wv, T.grp[0].n, T.grp[1].n, T.grp[2].n) > 0) {
      const float* sl = T.slots + wv * GN_SLOTS + (tid & 63);   // wave-uniform
      const float s = wave_sum64(((sl[0] + sl[64]) + sl[128]) + sl[192]);
      if ((tid & 63) == 0) {
        const float c = sel3(wv, T.c[0], T.c[1], T.c[2]);
        const bool ok = fabsf(s) <= 3.402823466e+38f;   // false for NaN
        const float norm = sqrtf(s);
        const float coef = ok ? fminf(1.f, c / (norm + 1e-6f)) : -1.f;
        s_coef[wv] = coef;
        if (blockIdx.x == 0) {
          float* cs = sel3(wv, T.cs[0], T.cs[1], T.cs[2]);
          cs[0] = norm; cs[1] = ok ? coef : 0.f; cs[2] = s;
          // groups of one launch may share a counter: the three bumps are
          // lanes of different waves, so go through the atomic unit
          if (!ok) atomicAdd(sel3(wv, T.sk[0], T.sk[1], T.sk[2]), 1);
        }
      }
    }
    __syncthreads();
  }
  long i = (long)blockIdx.x * blockDim.x + tid;
  AdamGroup G;
  int k;
  if constexpr (ONE) {
    if (i >= T.grp[0].n) return;
    G = T.grp[0]; k = 0;
  }
  else if (i < T.grp[0].n) { G = T.grp[0]; k = 0; }
  else if ((i -= T.grp[0].n) < T.grp[1].n) { G = T.grp[1]; k = 1; }
  else if ((i -= T.grp[1].n) < T.grp[2].n) { G = T.grp[2]; k = 2; }
  else {
    if ((i -= T.grp[2].n) < T.np) polyak_elem(T.pt, T.psrc, T.pmir, i, T.tau);
    return;
  }
  float gi;
  if constexpr (CLIP) {
    const float coef = s_coef[k];
    if (coef < 0.f) return;
    gi = coef * G.g[i];
  } else {
    if (k == 0 && T.arena0.ptr != nullptr)
      G.g[i] = gi = arena_fold(T.arena0, i);
    else
      gi = G.g[i];
  }
  adam_elem(G.p, G.m, G.v, G.mir, i, gi, G.st[1], G.st[2], T.b1, T.b2, T.eps);
}

// ===========================================================================
// Host wrappers
// ===========================================================================

static torch::Tensor linear_act_fwd_g(torch::Tensor x, torch::Tensor w,
                                      torch::Tensor b, long act, long G) {
  CHECK_IN(x); CHECK_IN(w); CHECK_IN(b);
  auto xc = x.contiguous(); auto wc = w.contiguous(); auto bc = b.contiguous();
  const bool per_group_x = xc.dim() == 3;  // [G,B,K] vs shared [B,K]
  const long M = per_group_x ? xc.size(1) : xc.size(0);
  const long K = xc.size(-1);
  const long N = wc.numel() / (G * K);
  TORCH_CHECK(wc.numel() == G * N * K && bc.numel() == G * N,
              "grouped weight shape mismatch");
  const long xgs = per_group_x ? M * K : 0;
  auto y = G == 1 ? torch::empty({M, N}, xc.options())
                  : torch::empty({G, M, N}, xc.options());
  dim3 grid((M + BM - 1) / BM, (N + BN - 1) / BN, G);
  hipLaunchKernelGGL(k_linear_act_fwd, grid, dim3(256), 0, cur_stream(),
                     xc.data_ptr<float>(), wc.data_ptr<float>(),
                     bc.data_ptr<float>(), y.data_ptr<float>(),
                     (int)M, (int)N, (int)K, (int)act, xgs);
  return y;
}

static torch::Tensor linear_act_fwd(torch::Tensor x, torch::Tensor w,
                                    torch::Tensor b, long act) {
  return linear_act_fwd_g(x, w, b, act, 1);
}

static torch::Tensor linear_bwd_dx_g(torch::Tensor dy, torch::Tensor w,
                                     torch::Tensor yout, long act, long G,
                                     long sum_over_g) {
  CHECK_IN(dy); CHECK_IN(w); CHECK_IN(yout);
  auto dyc = dy.contiguous(); auto wc = w.contiguous();
  auto yc = yout.contiguous();
  const long M = G == 1 ? dyc.size(0) : dyc.size(1);
  const long N = G == 1 ? dyc.size(1) : dyc.size(2);
  const long K = wc.size(-1);
  // sum mode: one grid, g-loop accumulates (shared-x layer).  per-group
  // mode: grid.z = G independent dx outputs [G,M,K].
  const long Gz = (G == 1 || sum_over_g) ? 1 : G;
  const int Gin = (int)((G > 1 && sum_over_g) ? G : 1);
  const long nbx = (M + BM - 1) / BM, nby = (K + BN - 1) / BN;
  const long nt_all = Gin * ((N + BK - 1) / BK);
  // split-reduce the tile loop when the grid underfills the 256-CU chip
  long S = 1;
  const long base_blocks = nbx * nby * Gz;
  if (base_blocks < 256) {
    S = std::min<long>(nt_all, std::max<long>(1, 512 / base_blocks));
  }
  auto dx = Gz == 1 ? torch::empty({M, K}, dyc.options())
                    : torch::empty({Gz, M, K}, dyc.options());
  auto out = dx;
  if (S > 1) out = torch::empty({Gz * S, M, K}, dyc.options());
  dim3 grid(nbx, nby, Gz * S);
  hipLaunchKernelGGL(k_linear_bwd_dx, grid, dim3(256), 0, cur_stream(),
                     dyc.data_ptr<float>(), wc.data_ptr<float>(),
                     yc.data_ptr<float>(), out.data_ptr<float>(),
                     (int)M, (int)N, (int)K, (int)act, Gin, (int)S);
  if (S > 1) {
    const long nmk = M * K;
    dim3 g1((nmk + 255) / 256, Gz);
    hipLaunchKernelGGL(k_reduce_partials, g1, dim3(256), 0, cur_stream(),
                       out.data_ptr<float>(), dx.data_ptr<float>(), nmk,
                       (int)S, nmk);
  }
  return dx;
}

static torch::Tensor linear_bwd_dx(torch::Tensor dy, torch::Tensor w,
                                   torch::Tensor yout, long act) {
  return linear_bwd_dx_g(dy, w, yout, act, 1, 1);
}

static std::vector<torch::Tensor> linear_bwd_dwdb_g(torch::Tensor dy,
                                                    torch::Tensor x,
                                                    torch::Tensor yout,
                                                    long act, long G) {
  CHECK_IN(dy); CHECK_IN(x); CHECK_IN(yout);
  auto dyc = dy.contiguous(); auto xc = x.contiguous();
  auto yc = yout.contiguous();
  const long M = G == 1 ? dyc.size(0) : dyc.size(1);
  const long N = G == 1 ? dyc.size(1) : dyc.size(2);
  const long K = xc.size(-1);
  const long xgs = xc.dim() == 3 ? M * K : 0;
  // split-K over the batch: pick S so total blocks ~ 2x CU count (just
  // enough to fill the chip; larger S doubles the partial-slab traffic)
  const long nbx = (N + BM - 1) / BM, nby = (K + BN - 1) / BN;
  long S = std::max<long>(1, 512 / std::max<long>(1, nbx * nby * G));
  S = std::min<long>(S, (M + BK - 1) / BK);
  const int chunk = (int)(((M + S - 1) / S + BK - 1) / BK * BK);
  S = (M + chunk - 1) / chunk;
  auto ws = torch::empty({G * S, N, K}, dyc.options());
  auto ws_db = torch::empty({G * S, N}, dyc.options());
  dim3 grid((N + BM - 1) / BM, (K + BN - 1) / BN, G * S);
  hipLaunchKernelGGL(k_linear_bwd_dwdb_splitk, grid, dim3(256), 0,
                     cur_stream(), dyc.data_ptr<float>(), xc.data_ptr<float>(),
                     yc.data_ptr<float>(), ws.data_ptr<float>(),
                     ws_db.data_ptr<float>(), (int)M, (int)N, (int)K,
                     (int)act, (int)S, chunk, xgs);
  auto dw = G == 1 ? torch::empty({N, K}, dyc.options())
                   : torch::empty({G, N, K}, dyc.options());
  auto db = G == 1 ? torch::empty({N}, dyc.options())
                   : torch::empty({G, N}, dyc.options());
  if (S == 1) {
    dw.copy_(ws.view_as(dw));
    db.copy_(ws_db.view_as(db));
  } else {
    const long nw = N * K;
    dim3 g1((nw + 255) / 256, G);
    hipLaunchKernelGGL(k_reduce_partials, g1, dim3(256), 0, cur_stream(),
                       ws.data_ptr<float>(), dw.data_ptr<float>(), nw,
                       (int)S, nw);
    dim3 g2((N + 255) / 256, G);
    hipLaunchKernelGGL(k_reduce_partials, g2, dim3(256), 0, cur_stream(),
                       ws_db.data_ptr<float>(), db.data_ptr<float>(), N,
                       (int)S, N);
  }
  return {dw, db};
}

static std::vector<torch::Tensor> linear_bwd_dwdb(torch::Tensor dy,
                                                  torch::Tensor x,
                                                  torch::Tensor yout,
                                                  long act) {
  return linear_bwd_dwdb_g(dy, x, yout, act, 1);
}

static std::vector<torch::Tensor> replay_sample(
    torch::Tensor states, torch::Tensor actions, torch::Tensor rewards,
    torch::Tensor next_states, torch::Tensor dones, torch::Tensor sizes,
    torch::Tensor rnd, long B,
    c10::optional<torch::Tensor> rng = c10::nullopt) {
  CHECK_IN(states); CHECK_IN(sizes);
  const bool krng = rng.has_value() && rng->numel() > 0;
  if (!krng) CHECK_IN(rnd);
  TORCH_CHECK(!krng || rng->scalar_type() == torch::kInt64,
              "rng counter must be int64");
  const long T = states.size(0), cap = states.size(1);
  const long Ds = states.size(2), Da = actions.size(2);
  const int per = (int)(B / T);
  TORCH_CHECK(per * T == B, "batch must divide by num_tasks");
  auto opt = states.options();
  auto o_s = torch::empty({B, Ds}, opt);
  auto o_a = torch::empty({B, Da}, opt);
  auto o_r = torch::empty({B, 1}, opt);
  auto o_ns = torch::empty({B, Ds}, opt);
  auto o_d = torch::empty({B, 1}, opt);
  hipLaunchKernelGGL(k_replay_sample, dim3((B + 3) / 4), dim3(256), 0,
                     cur_stream(), states.data_ptr<float>(),
                     actions.data_ptr<float>(), rewards.data_ptr<float>(),
                     next_states.data_ptr<float>(), dones.data_ptr<float>(),
                     sizes.data_ptr<float>(),
                     krng ? nullptr : rnd.data_ptr<float>(),
                     krng ? (const long long*)rng->data_ptr<long>()
                          : nullptr,
                     o_s.data_ptr<float>(), o_a.data_ptr<float>(),
                     o_r.data_ptr<float>(), o_ns.data_ptr<float>(),
                     o_d.data_ptr<float>(), (int)B, (int)T, per, cap,
                     (int)Ds, (int)Da);
  return {o_s, o_a, o_r, o_ns, o_d};
}

// Without-replacement draw (k_replay_sample_norepl).  `idx_out`, if given,
// receives the B drawn in-shard indices; the captured update passes none.
static std::vector<torch::Tensor> replay_sample_norepl(
    torch::Tensor states, torch::Tensor actions, torch::Tensor rewards,
    torch::Tensor next_states, torch::Tensor dones, torch::Tensor sizes,
    long B, torch::Tensor rng,
    c10::optional<torch::Tensor> idx_out = c10::nullopt) {
  CHECK_IN(states); CHECK_IN(actions); CHECK_IN(rewards);
  CHECK_IN(next_states); CHECK_IN(dones); CHECK_IN(sizes);
  TORCH_CHECK(rng.is_cuda() && rng.scalar_type() == torch::kInt64
              && rng.numel() >= 1, "rng counter must be an int64 HIP tensor");
  TORCH_CHECK(states.dim() == 3 && states.is_contiguous(),
              "states must be a contiguous [T, cap, Ds] tensor");
  const long T = states.size(0), cap = states.size(1);
  const long Ds = states.size(2);
  TORCH_CHECK(T >= 1 && cap >= 1 && cap < (1L << 31),
              "replay geometry out of range");
  TORCH_CHECK(actions.dim() == 3 && actions.is_contiguous()
              && actions.size(0) == T && actions.size(1) == cap,
              "actions must be a contiguous [T, cap, Da] tensor");
  const long Da = actions.size(2);
  TORCH_CHECK(next_states.is_contiguous()
              && next_states.sizes() == states.sizes(),
              "next_states must match states");
  TORCH_CHECK(rewards.is_contiguous() && rewards.numel() == T * cap
              && dones.is_contiguous() && dones.numel() == T * cap,
              "rewards/dones must be contiguous [T, cap, 1] tensors");
  TORCH_CHECK(sizes.is_contiguous() && sizes.numel() == T,
              "sizes must hold one entry per task");
  TORCH_CHECK(B >= 1 && B < (1L << 31) && B % T == 0,
              "batch must be positive and divide by num_tasks");
  const int per = (int)(B / T);
  long long* idx_p = nullptr;
  if (idx_out.has_value()) {
    TORCH_CHECK(idx_out->is_cuda() && idx_out->scalar_type() == torch::kInt64
                && idx_out->is_contiguous() && idx_out->numel() == B,
                "idx_out must be a contiguous int64 HIP tensor of B entries");
    idx_p = (long long*)idx_out->data_ptr<long>();
  }
  auto opt = states.options();
  auto o_s = torch::empty({B, Ds}, opt);
  auto o_a = torch::empty({B, Da}, opt);
  auto o_r = torch::empty({B, 1}, opt);
  auto o_ns = torch::empty({B, Ds}, opt);
  auto o_d = torch::empty({B, 1}, opt);
  hipLaunchKernelGGL(k_replay_sample_norepl, dim3((B + 3) / 4), dim3(256), 0,
                     cur_stream(), states.data_ptr<float>(),
                     actions.data_ptr<float>(), rewards.data_ptr<float>(),
                     next_states.data_ptr<float>(), dones.data_ptr<float>(),
                     sizes.data_ptr<float>(),
                     (const long long*)rng.data_ptr<long>(),
                     o_s.data_ptr<float>(), o_a.data_ptr<float>(),
                     o_r.data_ptr<float>(), o_ns.data_ptr<float>(),
                     o_d.data_ptr<float>(), idx_p, (int)B, (int)T, per, cap,
                     (int)Ds, (int)Da);
  return {o_s, o_a, o_r, o_ns, o_d};
}

// Packed ingest: `header` is the HOST copy of the batch (at least its
// header words), `staging` the device copy the kernel reads.  Every
// descriptor is re-validated here so a bad one raises on the host and
// never reaches the kernel.  Returns the number of rows scattered.
static long replay_ingest(torch::Tensor staging, torch::Tensor header,
                          torch::Tensor states, torch::Tensor actions,
                          torch::Tensor rewards, torch::Tensor next_states,
                          torch::Tensor dones, torch::Tensor sizes) {
  CHECK_IN(staging); CHECK_IN(states); CHECK_IN(actions); CHECK_IN(rewards);
  CHECK_IN(next_states); CHECK_IN(dones); CHECK_IN(sizes);
  TORCH_CHECK(header.device().is_cpu() &&
                  header.scalar_type() == torch::kFloat32 &&
                  header.is_contiguous() && staging.is_contiguous(),
              "header must be a contiguous fp32 host tensor");
  TORCH_CHECK(states.is_contiguous() && actions.is_contiguous() &&
                  rewards.is_contiguous() && next_states.is_contiguous() &&
                  dones.is_contiguous() && sizes.is_contiguous(),
              "replay fields must be contiguous");
  TORCH_CHECK(states.dim() == 3 && actions.dim() == 3, "fields are [T,cap,D]");
  const long T = states.size(0), cap = states.size(1);
  const long Ds = states.size(2), Da = actions.size(2);
  TORCH_CHECK(actions.size(0) == T && actions.size(1) == cap &&
                  rewards.numel() == T * cap && dones.numel() == T * cap &&
                  next_states.numel() == T * cap * Ds && sizes.numel() == T,
              "replay field shapes disagree");
  const long hn = header.numel();
  TORCH_CHECK(hn >= PK_HDR + T, "packed header truncated");
  const int32_t* h = reinterpret_cast<const int32_t*>(
      header.data_ptr<float>());
  const long n_desc = h[0], total_rows = h[2], used = h[3];
  TORCH_CHECK(h[1] == T, "packed batch built for another task count");
  TORCH_CHECK(n_desc >= 1 && PK_HDR + T + n_desc * PK_DESC <= hn,
              "packed descriptor count out of range");
  const long pay0 = PK_HDR + T + n_desc * PK_DESC;
  TORCH_CHECK(used >= pay0 && used <= staging.numel(),
              "packed batch larger than the staging buffer");
  const float* hs = header.data_ptr<float>() + PK_HDR;
  for (long t = 0; t < T; ++t)
    TORCH_CHECK(hs[t] >= 0.f && hs[t] <= (float)cap,
                "packed size outside [0, cap]");
  std::vector<long> per_task(T, 0);
  long base = 0;
  for (long k = 0; k < n_desc; ++k) {
    const int32_t* d = h + PK_HDR + T + k * PK_DESC;
    const long task = d[0], n = d[1], first = d[2], rows = d[3];
    const long off = d[4], dst = d[5];
    TORCH_CHECK(task >= 0 && task < T, "packed descriptor: task out of range");
    TORCH_CHECK(n >= 1 && rows >= 1 && rows <= cap && first >= 0 &&
                    first + rows <= n,
                "packed descriptor: rows out of range");
    TORCH_CHECK(off >= pay0 && off + n * (2 * Ds + Da + 2) <= used,
                "packed descriptor: payload outside the staging buffer");
    TORCH_CHECK(dst >= 0 && dst < cap, "packed descriptor: bad dst row");
    TORCH_CHECK(d[6] == base, "packed descriptor: bad row_base");
    base += rows;
    per_task[task] += rows;
    TORCH_CHECK(per_task[task] <= cap,
                "packed batch aliases rows of one task (rows > cap)");
  }
  TORCH_CHECK(base == total_rows, "packed row total disagrees");
  hipLaunchKernelGGL(k_replay_ingest, dim3((total_rows + 3) / 4), dim3(256),
                     0, cur_stream(), staging.data_ptr<float>(),
                     states.data_ptr<float>(), actions.data_ptr<float>(),
                     rewards.data_ptr<float>(),
                     next_states.data_ptr<float>(), dones.data_ptr<float>(),
                     sizes.data_ptr<float>(), (int)n_desc, (int)total_rows,
                     (int)T, cap, (int)Ds, (int)Da);
  return total_rows;
}

static std::vector<torch::Tensor> squashed_gaussian_fwd(
    torch::Tensor mu, torch::Tensor lsr, torch::Tensor eps, double k,
    c10::optional<torch::Tensor> rng = c10::nullopt) {
  CHECK_IN(mu); CHECK_IN(lsr); CHECK_IN(eps);
  const bool krng = rng.has_value() && rng->numel() > 0;
  TORCH_CHECK(!krng || (rng->scalar_type() == torch::kInt64
                        && eps.is_contiguous()),
              "krng mode needs an int64 counter and a contiguous eps out");
  const bool mu_ok = mu.dim() == 2 && mu.stride(1) == 1;
  const bool ls_ok = lsr.dim() == 2 && lsr.stride(1) == 1;
  auto muc = mu_ok ? mu : mu.contiguous();
  auto lc = ls_ok ? lsr : lsr.contiguous();
  auto ec = eps.contiguous();
  const long B = muc.size(0), A = muc.size(1);
  const long mu_ld = mu_ok ? mu.stride(0) : A;
  const long ls_ld = ls_ok ? lsr.stride(0) : A;
  TORCH_CHECK(A <= 32, "action_dim too large for fused kernel");
  auto opt = muc.options();
  auto act = torch::empty({B, A}, opt);
  auto logp = torch::empty({B, 1}, opt);
  auto tanh_u = torch::empty({B, A}, opt);
  auto ls_out = torch::empty({B, A}, opt);
  const int grid = (B + 255) / 256;
  hipLaunchKernelGGL(k_squash_fwd, dim3(grid), dim3(256), 0, cur_stream(),
                     muc.data_ptr<float>(), lc.data_ptr<float>(),
                     ec.data_ptr<float>(), act.data_ptr<float>(),
                     logp.data_ptr<float>(), tanh_u.data_ptr<float>(),
                     ls_out.data_ptr<float>(),
                     krng ? (const long long*)rng->data_ptr<long>()
                          : nullptr,
                     mu_ld, ls_ld, (int)B, (int)A, (float)k);
  return {act, logp, tanh_u, ls_out};
}

static std::vector<torch::Tensor> squashed_gaussian_bwd(
    torch::Tensor ga, torch::Tensor gl, torch::Tensor lsr, torch::Tensor ls,
    torch::Tensor eps, torch::Tensor tanh_u, double k) {
  CHECK_IN(ga); CHECK_IN(gl);
  auto gac = ga.contiguous(); auto glc = gl.contiguous();
  auto lsrc = lsr.contiguous(); auto lsc = ls.contiguous();
  auto ec = eps.contiguous(); auto tc = tanh_u.contiguous();
  const long B = gac.size(0), A = gac.size(1);
  auto dmu = torch::empty_like(gac);
  auto dlsr = torch::empty_like(gac);
  const int grid = (B + 255) / 256;
  hipLaunchKernelGGL(k_squash_bwd, dim3(grid), dim3(256), 0, cur_stream(),
                     gac.data_ptr<float>(), glc.data_ptr<float>(),
                     lsrc.data_ptr<float>(), lsc.data_ptr<float>(),
                     ec.data_ptr<float>(), tc.data_ptr<float>(),
                     dmu.data_ptr<float>(), dlsr.data_ptr<float>(),
                     (int)B, (int)A, (float)k);
  return {dmu, dlsr};
}

static torch::Tensor td_target(torch::Tensor r, torch::Tensor d,
                               torch::Tensor q1, torch::Tensor q2,
                               torch::Tensor lp, torch::Tensor alpha,
                               double gamma, double rs) {
  CHECK_IN(r);
  auto rc = r.contiguous(); auto dc = d.contiguous();
  auto q1c = q1.contiguous(); auto q2c = q2.contiguous();
  auto lpc = lp.contiguous(); auto ac = alpha.contiguous();
  const long n = rc.numel();
  TORCH_CHECK(ac.numel() == n, "alpha must be per-sample");
  auto y = torch::empty_like(rc);
  hipLaunchKernelGGL(k_td_target, dim3((n + 255) / 256), dim3(256), 0,
                     cur_stream(), rc.data_ptr<float>(), dc.data_ptr<float>(),
                     q1c.data_ptr<float>(), q2c.data_ptr<float>(),
                     lpc.data_ptr<float>(), ac.data_ptr<float>(),
                     y.data_ptr<float>(), (int)n, (float)gamma, (float)rs);
  return y;
}

// Argument checks shared by the K5-K7 bindings below (those of
// critic_td_loss / actor_alpha_loss_fwd_bwd): the kernels take raw pointers
// and read them with stride 1, so a view with other strides, a short
// vector, T > 32 (smw[32]) or a dla longer than the 256 threads that zero
// it must stop here, before any launch.
static const float* loss_onehot_arg(const torch::Tensor& states,
                                    const torch::Tensor& log_alpha, long B,
                                    long T, const char* who) {
  CHECK_IN(states); CHECK_IN(log_alpha);
  TORCH_CHECK(B >= 1, who, ": B >= 1");
  TORCH_CHECK(T >= 1 && T <= 32 && log_alpha.numel() >= T
              && log_alpha.is_contiguous(), who,
              ": 1 <= T <= 32 and T <= log_alpha.numel(), contiguous");
  TORCH_CHECK(states.dim() == 2 && states.is_contiguous()
              && states.size(0) == B && states.size(1) >= T, who,
              ": states must be a contiguous [B, >= T] tensor");
  return states.data_ptr<float>() + (states.size(1) - T);
}

static const float* loss_vec_arg(const torch::Tensor& t, long n,
                                 const char* who, const char* name) {
  TORCH_CHECK(t.is_cuda() && t.scalar_type() == torch::kFloat32
              && t.is_contiguous() && t.numel() == n, who, ": ", name,
              " must be a contiguous fp32 HIP tensor of ", n, " elements");
  return t.data_ptr<float>();
}

static torch::Tensor td_target_mt(torch::Tensor r, torch::Tensor d,
                                  torch::Tensor q1, torch::Tensor q2,
                                  torch::Tensor lp, torch::Tensor states,
                                  torch::Tensor log_alpha, long T,
                                  double gamma, double rs) {
  const char* who = "td_target_mt";
  const long n = r.numel();
  const float* oh = loss_onehot_arg(states, log_alpha, n, T, who);
  const long oh_stride = states.size(1);
  const float* r_p = loss_vec_arg(r, n, who, "r");
  const float* d_p = loss_vec_arg(d, n, who, "d");
  const float* q1_p = loss_vec_arg(q1, n, who, "q1");
  const float* q2_p = loss_vec_arg(q2, n, who, "q2");
  const float* lp_p = loss_vec_arg(lp, n, who, "lp");
  auto y = torch::empty_like(r);
  hipLaunchKernelGGL(k_td_target_mt, dim3((n + 255) / 256), dim3(256), 0,
                     cur_stream(), r_p, d_p, q1_p, q2_p, lp_p, oh,
                     log_alpha.data_ptr<float>(), y.data_ptr<float>(),
                     (int)n, (int)T, (int)oh_stride, (float)gamma,
                     (float)rs);
  return y;
}

static std::vector<torch::Tensor> critic_loss_fwd(
    torch::Tensor q1, torch::Tensor q2, torch::Tensor y,
    torch::Tensor states, torch::Tensor log_alpha, long T, long use_w,
    c10::optional<torch::Tensor> ws = c10::nullopt) {
  const char* who = "critic_loss_fwd";
  const long B = q1.numel();
  const float* oh = loss_onehot_arg(states, log_alpha, B, T, who);
  const long oh_stride = states.size(1);
  const float* q1_p = loss_vec_arg(q1, B, who, "q1");
  const float* q2_p = loss_vec_arg(q2, B, who, "q2");
  const float* y_p = loss_vec_arg(y, B, who, "y");
  auto out = torch::empty({8}, q1.options());
  if (ws.has_value() && ws->numel() >= 1 + 32 * 3) {
    CHECK_IN(*ws);
    TORCH_CHECK(ws->is_contiguous(), who, ": ws must be contiguous");
    // persistent zero-initialized workspace -> multi-block one-launch
    // path with last-block finalize (ticket self-resets per launch)
    const int nblk = (int)std::min<long>((B + 255) / 256, 32);
    hipLaunchKernelGGL(k_critic_loss_fwd_mb, dim3(nblk), dim3(256), 0,
                       cur_stream(), q1_p, q2_p, y_p, oh,
                       log_alpha.data_ptr<float>(), out.data_ptr<float>(),
                       ws->data_ptr<float>(), (int)B, (int)T,
                       (int)oh_stride, (int)use_w);
  } else {
    hipLaunchKernelGGL(k_critic_loss_fwd_1wg, dim3(1), dim3(256), 0,
                       cur_stream(), q1_p, q2_p, y_p, oh,
                       log_alpha.data_ptr<float>(), out.data_ptr<float>(),
                       (int)B, (int)T, (int)oh_stride, (int)use_w);
  }
  return {out};
}

static std::vector<torch::Tensor> critic_loss_bwd(
    torch::Tensor q1, torch::Tensor q2, torch::Tensor y,
    torch::Tensor states, torch::Tensor log_alpha, torch::Tensor saved,
    torch::Tensor gscale, long T, long use_w) {
  const char* who = "critic_loss_bwd";
  const long B = q1.numel();
  const float* oh = loss_onehot_arg(states, log_alpha, B, T, who);
  const long oh_stride = states.size(1);
  const float* q1_p = loss_vec_arg(q1, B, who, "q1");
  const float* q2_p = loss_vec_arg(q2, B, who, "q2");
  const float* y_p = loss_vec_arg(y, B, who, "y");
  const float* saved_p = loss_vec_arg(saved, 8, who, "saved");
  const float* gscale_p = loss_vec_arg(gscale, 2, who, "gscale");
  auto dq1 = torch::empty_like(q1);
  auto dq2 = torch::empty_like(q2);
  hipLaunchKernelGGL(k_critic_loss_bwd, dim3((B + 255) / 256), dim3(256), 0,
                     cur_stream(), q1_p, q2_p, y_p, oh,
                     log_alpha.data_ptr<float>(), saved_p, gscale_p,
                     dq1.data_ptr<float>(), dq2.data_ptr<float>(), (int)B,
                     (int)T, (int)oh_stride, (int)use_w);
  return {dq1, dq2};
}

static torch::Tensor actor_alpha_loss_fwd(
    torch::Tensor aq1, torch::Tensor aq2, torch::Tensor lp, torch::Tensor ls,
    torch::Tensor states, torch::Tensor log_alpha, long T, long use_w,
    double H_bar,
    c10::optional<torch::Tensor> dla = c10::nullopt,
    c10::optional<torch::Tensor> ws = c10::nullopt) {
  const char* who = "actor_alpha_loss_fwd";
  const long B = aq1.numel();
  const float* oh = loss_onehot_arg(states, log_alpha, B, T, who);
  const long oh_stride = states.size(1);
  const float* aq1_p = loss_vec_arg(aq1, B, who, "aq1");
  const float* aq2_p = loss_vec_arg(aq2, B, who, "aq2");
  const float* lp_p = loss_vec_arg(lp, B, who, "lp");
  TORCH_CHECK(ls.dim() == 2 && ls.size(0) == B, who, ": ls must be [B, A]");
  const long A = ls.size(1);
  const float* ls_p = loss_vec_arg(ls, B * A, who, "ls");
  auto out = torch::empty({8}, aq1.options());
  float* dla_p = nullptr;
  int dla_n = 0;
  if (dla.has_value() && dla->numel() > 0) {
    CHECK_IN(*dla);
    TORCH_CHECK(dla->numel() <= 256 && dla->is_contiguous(), who,
                ": dla must be contiguous, at most 256 elements");
    dla_p = dla->data_ptr<float>();
    dla_n = (int)dla->numel();
  }
  if (ws.has_value() && ws->numel() >= 1 + 32 * 4) {
    CHECK_IN(*ws);
    TORCH_CHECK(ws->is_contiguous(), who, ": ws must be contiguous");
    const int nblk = (int)std::min<long>((B + 255) / 256, 32);
    hipLaunchKernelGGL(k_actor_alpha_loss_fwd_mb, dim3(nblk), dim3(256), 0,
                       cur_stream(), aq1_p, aq2_p, lp_p, ls_p, oh,
                       log_alpha.data_ptr<float>(),
                       out.data_ptr<float>(), ws->data_ptr<float>(), dla_p,
                       dla_n, (int)B, (int)T, (int)A, (int)oh_stride,
                       (int)use_w, (float)H_bar);
  } else {
    hipLaunchKernelGGL(k_actor_alpha_loss_fwd_1wg, dim3(1), dim3(256), 0,
                       cur_stream(), aq1_p, aq2_p, lp_p, ls_p, oh,
                       log_alpha.data_ptr<float>(),
                       out.data_ptr<float>(), dla_p, dla_n, (int)B, (int)T,
                       (int)A, (int)oh_stride, (int)use_w, (float)H_bar);
  }
  return out;
}

static std::vector<torch::Tensor> actor_alpha_loss_bwd(
    torch::Tensor aq1, torch::Tensor aq2, torch::Tensor lp,
    torch::Tensor states, torch::Tensor log_alpha, torch::Tensor saved,
    torch::Tensor gscale, long T, long use_w, double H_bar) {
  const char* who = "actor_alpha_loss_bwd";
  const long B = aq1.numel();
  const float* oh = loss_onehot_arg(states, log_alpha, B, T, who);
  const long oh_stride = states.size(1);
  const float* aq1_p = loss_vec_arg(aq1, B, who, "aq1");
  const float* aq2_p = loss_vec_arg(aq2, B, who, "aq2");
  const float* lp_p = loss_vec_arg(lp, B, who, "lp");
  const float* saved_p = loss_vec_arg(saved, 8, who, "saved");
  const float* gscale_p = loss_vec_arg(gscale, 2, who, "gscale");
  auto daq1 = torch::empty_like(aq1);
  auto daq2 = torch::empty_like(aq2);
  auto dlp = torch::empty_like(lp);
  auto dla = torch::zeros_like(log_alpha);
  hipLaunchKernelGGL(k_actor_alpha_loss_bwd, dim3((B + 255) / 256 + 1), dim3(256),
                     (size_t)T * 256 * sizeof(float), cur_stream(),
                     aq1_p, aq2_p, lp_p, oh, log_alpha.data_ptr<float>(),
                     saved_p, gscale_p, daq1.data_ptr<float>(),
                     daq2.data_ptr<float>(), dlp.data_ptr<float>(),
                     dla.data_ptr<float>(), (int)B, (int)T, (int)oh_stride,
                     (int)use_w, (float)H_bar);
  return {daq1, daq2, dlp, dla};
}

static torch::Tensor critic_loss_bwd2(
    torch::Tensor q1, torch::Tensor q2, torch::Tensor y,
    torch::Tensor states, torch::Tensor log_alpha, torch::Tensor saved,
    long T, long use_w) {
  const char* who = "critic_loss_bwd2";
  const long B = q1.numel();
  const float* oh = loss_onehot_arg(states, log_alpha, B, T, who);
  const long oh_stride = states.size(1);
  const float* q1_p = loss_vec_arg(q1, B, who, "q1");
  const float* q2_p = loss_vec_arg(q2, B, who, "q2");
  const float* y_p = loss_vec_arg(y, B, who, "y");
  const float* saved_p = loss_vec_arg(saved, 8, who, "saved");
  auto dq = torch::empty({2, B, 1}, q1.options().dtype(torch::kBFloat16));
  hipLaunchKernelGGL(k_critic_loss_bwd2, dim3((B + 255) / 256), dim3(256), 0,
                     cur_stream(), q1_p, q2_p, y_p, oh,
                     log_alpha.data_ptr<float>(), saved_p,
                     (unsigned short*)dq.data_ptr(), (int)B, (int)T,
                     (int)oh_stride, (int)use_w);
  return dq;
}

static std::vector<torch::Tensor> actor_alpha_loss_bwd2(
    torch::Tensor aq1, torch::Tensor aq2, torch::Tensor lp,
    torch::Tensor states, torch::Tensor log_alpha, torch::Tensor saved,
    torch::Tensor dla_out, long T, long use_w, double H_bar,
    c10::optional<torch::Tensor> ws = c10::nullopt) {
  const char* who = "actor_alpha_loss_bwd2";
  CHECK_IN(dla_out);
  const long B = aq1.numel();
  const float* oh = loss_onehot_arg(states, log_alpha, B, T, who);
  const long oh_stride = states.size(1);
  const float* aq1_p = loss_vec_arg(aq1, B, who, "aq1");
  const float* aq2_p = loss_vec_arg(aq2, B, who, "aq2");
  const float* lp_p = loss_vec_arg(lp, B, who, "lp");
  const float* saved_p = loss_vec_arg(saved, 8, who, "saved");
  TORCH_CHECK(dla_out.numel() >= T && dla_out.is_contiguous(), who,
              ": dla_out must be contiguous with at least T elements");
  auto daq = torch::empty({2, B, 1}, aq1.options().dtype(torch::kBFloat16));
  auto dlp = torch::empty_like(lp);
  const long nblk = (B + 255) / 256;
  float* ws_p = nullptr;   // ticket path only if the workspace is big enough
  if (ws.has_value() && ws->numel() >= 1 + nblk * T) {
    CHECK_IN(*ws);
    TORCH_CHECK(ws->is_contiguous(), who, ": ws must be contiguous");
    ws_p = ws->data_ptr<float>();
  }
  hipLaunchKernelGGL(k_actor_alpha_loss_bwd2,
                     dim3(ws_p ? nblk : nblk + 1),
                     dim3(256),
                     ws_p ? 0 : (size_t)T * 256 * sizeof(float),
                     cur_stream(), aq1_p, aq2_p, lp_p, oh,
                     log_alpha.data_ptr<float>(), saved_p,
                     (unsigned short*)daq.data_ptr(), dlp.data_ptr<float>(),
                     dla_out.data_ptr<float>(), ws_p, (int)B, (int)T,
                     (int)oh_stride, (int)use_w, (float)H_bar);
  return {daq, dlp};
}

// td_target_mt + critic_loss_fwd(ws) + critic_loss_bwd2 in one launch.
// Returns {closs[8], dq[2,B,1] bf16}; ws as for critic_loss_fwd.
static std::vector<torch::Tensor> critic_td_loss(
    torch::Tensor r, torch::Tensor d, torch::Tensor q1t, torch::Tensor q2t,
    torch::Tensor nlp, torch::Tensor q1, torch::Tensor q2,
    torch::Tensor states, torch::Tensor log_alpha, long T, long use_w,
    double gamma, double rs, torch::Tensor ws) {
  CHECK_IN(r); CHECK_IN(d); CHECK_IN(q1t); CHECK_IN(q2t); CHECK_IN(nlp);
  CHECK_IN(q1); CHECK_IN(q2); CHECK_IN(states); CHECK_IN(log_alpha);
  CHECK_IN(ws);
  const long B = q1.size(0);
  const long nblk = (B + 255) / 256;
  TORCH_CHECK(B >= 1 && nblk <= 32, "critic_td_loss: 1 <= B <= 8192");
  TORCH_CHECK(T >= 1 && T <= 32 && log_alpha.numel() >= T, "T <= 32");
  TORCH_CHECK(ws.numel() >= 1 + 32 * 3, "workspace too small");
  TORCH_CHECK(states.dim() == 2 && states.is_contiguous()
              && states.size(0) == B && states.size(1) >= T);
  auto rc = r.contiguous(); auto dc = d.contiguous();
  auto q1tc = q1t.contiguous(); auto q2tc = q2t.contiguous();
  auto lpc = nlp.contiguous();
  auto q1c = q1.contiguous(); auto q2c = q2.contiguous();
  TORCH_CHECK(rc.numel() == B && dc.numel() == B && q1tc.numel() == B
              && q2tc.numel() == B && lpc.numel() == B && q1c.numel() == B
              && q2c.numel() == B, "critic_td_loss: B elements per input");
  const long oh_stride = states.size(1);
  const float* oh = states.data_ptr<float>() + (oh_stride - T);
  auto out = torch::empty({8}, q1.options());
  auto dq = torch::empty({2, B, 1}, q1.options().dtype(torch::kBFloat16));
  hipLaunchKernelGGL(k_critic_td_loss, dim3(nblk), dim3(256), 0,
                     cur_stream(), rc.data_ptr<float>(),
                     dc.data_ptr<float>(), q1tc.data_ptr<float>(),
                     q2tc.data_ptr<float>(), lpc.data_ptr<float>(),
                     q1c.data_ptr<float>(), q2c.data_ptr<float>(), oh,
                     log_alpha.data_ptr<float>(), out.data_ptr<float>(),
                     ws.data_ptr<float>(), (unsigned short*)dq.data_ptr(),
                     (int)B, (int)T, (int)oh_stride, (int)use_w,
                     (float)gamma, (float)rs);
  return {out, dq};
}

// actor_alpha_loss_fwd(ws, dla) + actor_alpha_loss_bwd2(ws) in one launch.
// Returns {al[8], daq[2,B,1] bf16, dlp}; dla (the alpha flat gradient) is
// overwritten.  ws: 1 + 32*4 + ceil(B/256)*T floats, ticket zero on entry.
// wsum (optional, 1 float): the weighted-loss normalizer a critic-loss
// kernel finalized (closs[2]) over the SAME states and log_alpha with the
// same B — the value this kernel's forward would compute; given it, the
// blocks skip recomputing it for the backward coefficient.
static std::vector<torch::Tensor> actor_alpha_loss_fwd_bwd(
    torch::Tensor aq1, torch::Tensor aq2, torch::Tensor lp, torch::Tensor ls,
    torch::Tensor states, torch::Tensor log_alpha, torch::Tensor dla,
    long T, long use_w, double H_bar, torch::Tensor ws,
    c10::optional<torch::Tensor> wsum = c10::nullopt) {
  CHECK_IN(aq1); CHECK_IN(aq2); CHECK_IN(lp); CHECK_IN(ls);
  CHECK_IN(states); CHECK_IN(log_alpha); CHECK_IN(dla); CHECK_IN(ws);
  const float* wsum_p = nullptr;
  if (wsum.has_value() && wsum->defined() && wsum->numel() > 0) {
    CHECK_IN(*wsum);
    wsum_p = wsum->data_ptr<float>();
  }
  const long B = aq1.size(0);
  const long nblk = (B + 255) / 256;
  TORCH_CHECK(B >= 1 && nblk <= 32,
              "actor_alpha_loss_fwd_bwd: 1 <= B <= 8192");
  TORCH_CHECK(T >= 1 && T <= 32 && log_alpha.numel() >= T
              && dla.numel() >= T && dla.numel() <= 256
              && dla.is_contiguous(), "alpha gradient: T <= 32");
  TORCH_CHECK(ws.numel() >= 1 + 32 * 4 + nblk * T, "workspace too small");
  TORCH_CHECK(states.dim() == 2 && states.is_contiguous()
              && states.size(0) == B && states.size(1) >= T);
  auto aq1c = aq1.contiguous(); auto aq2c = aq2.contiguous();
  auto lpc = lp.contiguous(); auto lsc = ls.contiguous();
  TORCH_CHECK(aq1c.numel() == B && aq2c.numel() == B && lpc.numel() == B
              && lsc.dim() == 2 && lsc.size(0) == B,
              "actor_alpha_loss_fwd_bwd: B rows per input");
  const long A = lsc.size(1);
  const long oh_stride = states.size(1);
  const float* oh = states.data_ptr<float>() + (oh_stride - T);
  auto out = torch::empty({8}, aq1.options());
  auto daq = torch::empty({2, B, 1}, aq1.options().dtype(torch::kBFloat16));
  auto dlp = torch::empty_like(lpc);
  hipLaunchKernelGGL(k_actor_alpha_loss_fwd_bwd, dim3(nblk), dim3(256), 0,
                     cur_stream(), aq1c.data_ptr<float>(),
                     aq2c.data_ptr<float>(), lpc.data_ptr<float>(),
                     lsc.data_ptr<float>(), oh, log_alpha.data_ptr<float>(),
                     out.data_ptr<float>(), ws.data_ptr<float>(),
                     (unsigned short*)daq.data_ptr(), dlp.data_ptr<float>(),
                     dla.data_ptr<float>(), (int)dla.numel(), wsum_p, (int)B,
                     (int)T, (int)A, (int)oh_stride, (int)use_w,
                     (float)H_bar);
  return {out, daq, dlp};
}

static torch::Tensor squashed_gaussian_bwd2(
    torch::Tensor ga, torch::Tensor gl, torch::Tensor lsr, torch::Tensor ls,
    torch::Tensor eps, torch::Tensor tanh_u, double k) {
  CHECK_IN(ga);
  auto gac = ga.contiguous(); auto glc = gl.contiguous();
  const bool lsr_ok = lsr.dim() == 2 && lsr.stride(1) == 1;
  auto lsrc = lsr_ok ? lsr : lsr.contiguous();
  auto lsc = ls.contiguous();
  auto ec = eps.contiguous(); auto tc = tanh_u.contiguous();
  const int ga_twin = (gac.dim() == 3 && gac.size(0) == 2) ? 1 : 0;
  const long B = ga_twin ? gac.size(1) : gac.size(0);
  const long A = ga_twin ? gac.size(2) : gac.size(1);
  const long lsr_ld = lsr_ok ? lsr.stride(0) : A;
  auto dhead = torch::empty({B, 2 * A},
                            gac.options().dtype(torch::kBFloat16));
  hipLaunchKernelGGL(k_squash_bwd2, dim3((B + 255) / 256), dim3(256), 0,
                     cur_stream(), gac.data_ptr<float>(),
                     glc.data_ptr<float>(), lsrc.data_ptr<float>(),
                     lsc.data_ptr<float>(), ec.data_ptr<float>(),
                     tc.data_ptr<float>(),
                     (unsigned short*)dhead.data_ptr(), lsr_ld, ga_twin,
                     (int)B, (int)A, (float)k);
  return dhead;
}

// -- optimizer tail: the shared marshalling of the Adam/Polyak bindings ----
using OptTensor = c10::optional<torch::Tensor>;

static bool given(const OptTensor& t) {
  return t.has_value() && t->defined() && t->numel() > 0;
}

static unsigned short* opt_mirror(const OptTensor& mir, long n) {
  if (!given(mir)) return nullptr;
  TORCH_CHECK(mir->is_cuda() && mir->numel() == n && mir->is_contiguous()
              && mir->scalar_type() == torch::kBFloat16,
              "mirror must be a bf16 HIP tensor of the group's numel");
  return (unsigned short*)mir->data_ptr();
}

// optional [>=S, numel] split-K partials of the flat gradient g
static Arena opt_arena(const OptTensor& arena, long S, const torch::Tensor& g) {
  if (!given(arena)) return Arena{nullptr, 0, 0};
  CHECK_IN(*arena); CHECK_IN(g);
  TORCH_CHECK(arena->dim() == 2 && arena->is_contiguous() && g.is_contiguous()
              && arena->size(1) == g.numel() && S >= 1 && S <= arena->size(0),
              "arena must be [>=S, numel of the first gradient]");
  return Arena{arena->data_ptr<float>(), g.numel(), (int)S};
}

// <= 3 Adam groups into a table; returns it with everything optional unset
static AdamTable fill_groups(const std::vector<torch::Tensor>& ps,
                             const std::vector<torch::Tensor>& gs,
                             const std::vector<torch::Tensor>& ms,
                             const std::vector<torch::Tensor>& vs,
                             const std::vector<torch::Tensor>& states,
                             const std::vector<torch::Tensor>& mirs,
                             double b1, double b2, double eps) {
  const size_t G = ps.size();
  TORCH_CHECK(G >= 1 && G <= 3, "1..3 groups");
  TORCH_CHECK(gs.size() == G && ms.size() == G && vs.size() == G
              && states.size() == G && mirs.size() <= G,
              "one entry per group");
  AdamTable T{};
  T.b1 = (float)b1; T.b2 = (float)b2; T.eps = (float)eps;
  for (size_t k = 0; k < G; ++k) {
    CHECK_IN(ps[k]); CHECK_IN(gs[k]); CHECK_IN(ms[k]); CHECK_IN(vs[k]);
    CHECK_IN(states[k]);
    const long n = ps[k].numel();
    TORCH_CHECK(gs[k].numel() == n && ms[k].numel() == n
                && vs[k].numel() == n && ps[k].is_contiguous()
                && gs[k].is_contiguous() && ms[k].is_contiguous()
                && vs[k].is_contiguous() && states[k].numel() >= 3,
                "bad Adam group: p, g, m, v contiguous of one numel, "
                "state = {step, step_size, inv_sqrt_bc2}");
    T.grp[k] = AdamGroup{
        ps[k].data_ptr<float>(), gs[k].data_ptr<float>(),
        ms[k].data_ptr<float>(), vs[k].data_ptr<float>(),
        states[k].data_ptr<float>(),
        k < mirs.size() ? opt_mirror(mirs[k], n) : nullptr, n};
  }
  return T;
}

// optional Polyak range behind the Adam groups
static void opt_polyak(AdamTable& T, const std::vector<torch::Tensor>& ps,
                       const OptTensor& t, const OptTensor& s, double tau,
                       const OptTensor& mir) {
  if (!given(t)) return;
  TORCH_CHECK(s.has_value(), "polyak source missing");
  CHECK_IN(*t); CHECK_IN(*s);
  TORCH_CHECK(s->numel() == t->numel() && t->is_contiguous()
              && s->is_contiguous(), "polyak buffers must match");
  for (const auto& p : ps)
    TORCH_CHECK(s->data_ptr() != p.data_ptr() && t->data_ptr() != p.data_ptr(),
                "polyak buffers must not be stepped in the same launch");
  T.pt = t->data_ptr<float>();
  T.psrc = s->data_ptr<float>();
  T.np = t->numel();
  T.tau = (float)tau;
  T.pmir = opt_mirror(mir, T.np);
}

template <bool CLIP>
static void launch_groups(const AdamTable& T) {
  const long total = T.grp[0].n + T.grp[1].n + T.grp[2].n + T.np;
  const dim3 grid((total + 255) / 256);
  if (!CLIP && total == T.grp[0].n)
    hipLaunchKernelGGL((k_adam_groups<false, true>), grid, dim3(256), 0,
                       cur_stream(), T);
  else
    hipLaunchKernelGGL((k_adam_groups<CLIP, false>), grid, dim3(256), 0,
                       cur_stream(), T);
}

static void adam_prolog_many(std::vector<torch::Tensor> states,
                             std::vector<double> lrs, double b1, double b2,
                             OptTensor rng) {
  const size_t G = states.size();
  TORCH_CHECK(G >= 1 && G <= 4 && lrs.size() == G, "1..4 states");
  float* S[4] = {nullptr, nullptr, nullptr, nullptr};
  float L[4] = {0.f, 0.f, 0.f, 0.f};
  for (size_t g = 0; g < G; ++g) {
    CHECK_IN(states[g]);
    TORCH_CHECK(states[g].numel() >= 3,
                "state = {step, step_size, inv_sqrt_bc2}");
    S[g] = states[g].data_ptr<float>();
    L[g] = (float)lrs[g];
  }
  long long* rng_p = given(rng) ? (long long*)rng->data_ptr<long>() : nullptr;
  hipLaunchKernelGGL(k_adam_prolog_many, dim3(1), dim3(4), 0, cur_stream(),
                     rng_p, S[0], S[1], S[2], S[3], L[0], L[1], L[2], L[3],
                     (float)b1, (float)b2);
}

static void adam_step_(torch::Tensor p, torch::Tensor g, torch::Tensor m,
                       torch::Tensor v, long step, double lr, double b1,
                       double b2, double eps) {
  CHECK_IN(p);
  const long n = p.numel();
  const double bc1 = 1.0 - std::pow(b1, (double)step);
  const double bc2 = 1.0 - std::pow(b2, (double)step);
  const float step_size = (float)(lr / bc1);
  const float inv_sqrt_bc2 = (float)(1.0 / std::sqrt(bc2));
  hipLaunchKernelGGL(k_adam, dim3((n + 255) / 256), dim3(256), 0,
                     cur_stream(), p.data_ptr<float>(), g.data_ptr<float>(),
                     m.data_ptr<float>(), v.data_ptr<float>(), n,
                     (float)b1, (float)b2, step_size, inv_sqrt_bc2,
                     (float)eps);
}

// one group; arena: optional [>=S, n] split-K partials folded into g
static void adam_step_dev_(torch::Tensor p, torch::Tensor g, torch::Tensor m,
                           torch::Tensor v, torch::Tensor state, double lr,
                           double b1, double b2, double eps,
                           OptTensor mir_opt, long skip_prolog = 0,
                           OptTensor arena = c10::nullopt, long S = 0) {
  AdamTable T = fill_groups({p}, {g}, {m}, {v}, {state},
                            {given(mir_opt) ? *mir_opt : torch::Tensor()},
                            b1, b2, eps);
  T.arena0 = opt_arena(arena, S, g);
  if (!skip_prolog) adam_prolog_many({state}, {lr}, b1, b2, c10::nullopt);
  launch_groups<false>(T);
}

// <= 3 groups [+ arena0 folded into gs[0]] [+ Polyak range]: [prolog,] K9
static void adam_step_multi_(std::vector<torch::Tensor> ps,
                             std::vector<torch::Tensor> gs,
                             std::vector<torch::Tensor> ms,
                             std::vector<torch::Tensor> vs,
                             std::vector<torch::Tensor> states,
                             std::vector<double> lrs, double b1, double b2,
                             double eps, std::vector<torch::Tensor> mirs,
                             OptTensor rng = c10::nullopt,
                             long skip_prolog = 0,
                             OptTensor arena0 = c10::nullopt, long S0 = 0,
                             OptTensor polyak_t = c10::nullopt,
                             OptTensor polyak_s = c10::nullopt,
                             double tau = 0.0,
                             OptTensor polyak_mir = c10::nullopt) {
  AdamTable T = fill_groups(ps, gs, ms, vs, states, mirs, b1, b2, eps);
  T.arena0 = opt_arena(arena0, S0, gs[0]);
  opt_polyak(T, ps, polyak_t, polyak_s, tau, polyak_mir);
  if (!skip_prolog) adam_prolog_many(states, lrs, b1, b2, rng);
  launch_groups<false>(T);
}

// K11 alone: slots[r*GN_SLOTS + b] for r < gs.size(); arena0 as in
// adam_step_multi_ (folded into gs[0], which is then written).
static void grad_sumsq_(std::vector<torch::Tensor> gs, torch::Tensor slots,
                        OptTensor arena0 = c10::nullopt, long S0 = 0) {
  const size_t G = gs.size();
  TORCH_CHECK(G >= 1 && G <= 3, "1..3 ranges");
  CHECK_IN(slots);
  TORCH_CHECK(slots.is_contiguous() && slots.numel() >= 3 * GN_SLOTS,
              "slots must hold 3 * 256 floats");
  float* Gp[3] = {nullptr, nullptr, nullptr};
  long N[3] = {0, 0, 0};
  for (size_t g = 0; g < G; ++g) {
    CHECK_IN(gs[g]);
    TORCH_CHECK(gs[g].is_contiguous(), "flat gradients must be contiguous");
    Gp[g] = gs[g].data_ptr<float>();
    N[g] = gs[g].numel();
  }
  hipLaunchKernelGGL(k_grad_sumsq, dim3(GN_SLOTS, (unsigned)G), dim3(256), 0,
                     cur_stream(), Gp[0], N[0], Gp[1], N[1], Gp[2], N[2],
                     opt_arena(arena0, S0, gs[0]), slots.data_ptr<float>());
}

// adam_step_multi_ with gradient-norm clipping: [prolog,] K11, K9<CLIP>.
// maxn[g]: the group's threshold (inf = guard only); clip_states[g]: fp32
// {norm, coef, s}; skips[g]: int32 counter (groups may share one).
static void adam_step_clip_(std::vector<torch::Tensor> ps,
                            std::vector<torch::Tensor> gs,
                            std::vector<torch::Tensor> ms,
                            std::vector<torch::Tensor> vs,
                            std::vector<torch::Tensor> states,
                            std::vector<double> lrs, double b1, double b2,
                            double eps, std::vector<torch::Tensor> mirs,
                            torch::Tensor slots, std::vector<double> maxn,
                            std::vector<torch::Tensor> clip_states,
                            std::vector<torch::Tensor> skips,
                            OptTensor rng = c10::nullopt,
                            long skip_prolog = 0,
                            OptTensor arena0 = c10::nullopt, long S0 = 0,
                            OptTensor polyak_t = c10::nullopt,
                            OptTensor polyak_s = c10::nullopt,
                            double tau = 0.0,
                            OptTensor polyak_mir = c10::nullopt) {
  AdamTable T = fill_groups(ps, gs, ms, vs, states, mirs, b1, b2, eps);
  const size_t G = ps.size();
  TORCH_CHECK(maxn.size() == G && clip_states.size() == G
              && skips.size() == G, "one entry per group");
  for (size_t k = 0; k < G; ++k) {
    CHECK_IN(clip_states[k]);
    TORCH_CHECK(clip_states[k].numel() >= 3 && skips[k].is_cuda()
                && skips[k].numel() >= 1
                && skips[k].scalar_type() == torch::kInt32
                && maxn[k] > 0.0, "bad clipped Adam group");
    T.c[k] = (float)maxn[k];
    T.cs[k] = clip_states[k].data_ptr<float>();
    T.sk[k] = skips[k].data_ptr<int>();
  }
  opt_polyak(T, ps, polyak_t, polyak_s, tau, polyak_mir);
  if (!skip_prolog) adam_prolog_many(states, lrs, b1, b2, rng);
  grad_sumsq_(gs, slots, arena0, S0);   // checks slots; folds arena0
  T.slots = slots.data_ptr<float>();
  launch_groups<true>(T);
}

static void polyak_(torch::Tensor t, torch::Tensor s, double tau,
                    OptTensor mir_opt) {
  CHECK_IN(t); CHECK_IN(s);
  const long n = t.numel();
  TORCH_CHECK(s.numel() == n && t.is_contiguous() && s.is_contiguous(),
              "polyak buffers must match");
  hipLaunchKernelGGL(k_polyak, dim3((n + 255) / 256), dim3(256), 0,
                     cur_stream(), t.data_ptr<float>(), s.data_ptr<float>(),
                     n, (float)tau, opt_mirror(mir_opt, n));
}

// -- prioritized replay ------------------------------------------------------
// Shared validation of the priority state: prio [T, cap], bsum [T, nb] with
// nb = ceil(cap / PER_BLOCK), total [T], maxp [T]; ws holds the two tickets.
static void per_check_state(const torch::Tensor& prio,
                            const torch::Tensor& bsum,
                            const torch::Tensor& total, long T, long cap) {
  CHECK_IN(prio); CHECK_IN(bsum); CHECK_IN(total);
  const long nb = (cap + PER_BLOCK - 1) / PER_BLOCK;
  TORCH_CHECK(T >= 1 && cap >= 1 && cap <= (1L << 24),
              "prioritized replay: geometry out of range");
  TORCH_CHECK(prio.is_contiguous() && prio.numel() == T * cap,
              "priorities must be a contiguous [T, cap] tensor");
  TORCH_CHECK(bsum.is_contiguous() && bsum.numel() == T * nb,
              "block sums must be a contiguous [T, ceil(cap / PER_BLOCK)] "
              "tensor");
  TORCH_CHECK(total.is_contiguous() && total.numel() == T,
              "totals must hold one entry per task");
}

static void per_check_ws(const torch::Tensor& ws) {
  TORCH_CHECK(ws.is_cuda() && ws.scalar_type() == torch::kInt32
              && ws.is_contiguous() && ws.numel() >= 2,
              "prioritized replay workspace must be an int32 HIP tensor of "
              "at least 2 words");
}

// Proportional draw + gather (k_replay_sample_per).  idx_out receives the B
// flat row indices (t * cap + row), w_out the raw IS weights.
static std::vector<torch::Tensor> replay_sample_per(
    torch::Tensor states, torch::Tensor actions, torch::Tensor rewards,
    torch::Tensor next_states, torch::Tensor dones, torch::Tensor sizes,
    torch::Tensor prio, torch::Tensor bsum, torch::Tensor total,
    torch::Tensor beta, long B, torch::Tensor rng, torch::Tensor idx_out,
    torch::Tensor w_out) {
  CHECK_IN(states); CHECK_IN(actions); CHECK_IN(rewards);
  CHECK_IN(next_states); CHECK_IN(dones); CHECK_IN(sizes); CHECK_IN(beta);
  CHECK_IN(w_out);
  TORCH_CHECK(rng.is_cuda() && rng.scalar_type() == torch::kInt64
              && rng.numel() >= 1, "rng counter must be an int64 HIP tensor");
  TORCH_CHECK(states.dim() == 3 && states.is_contiguous(),
              "states must be a contiguous [T, cap, Ds] tensor");
  const long T = states.size(0), cap = states.size(1);
  const long Ds = states.size(2);
  per_check_state(prio, bsum, total, T, cap);
  TORCH_CHECK(actions.dim() == 3 && actions.is_contiguous()
              && actions.size(0) == T && actions.size(1) == cap,
              "actions must be a contiguous [T, cap, Da] tensor");
  const long Da = actions.size(2);
  TORCH_CHECK(next_states.is_contiguous()
              && next_states.sizes() == states.sizes(),
              "next_states must match states");
  TORCH_CHECK(rewards.is_contiguous() && rewards.numel() == T * cap
              && dones.is_contiguous() && dones.numel() == T * cap,
              "rewards/dones must be contiguous [T, cap, 1] tensors");
  TORCH_CHECK(sizes.is_contiguous() && sizes.numel() == T,
              "sizes must hold one entry per task");
  TORCH_CHECK(beta.numel() >= 1, "beta must hold one element");
  TORCH_CHECK(B >= 1 && B <= 8192 && B % T == 0,
              "batch must be in [1, 8192] and divide by num_tasks");
  TORCH_CHECK(idx_out.is_cuda() && idx_out.scalar_type() == torch::kInt64
              && idx_out.is_contiguous() && idx_out.numel() == B,
              "idx_out must be a contiguous int64 HIP tensor of B entries");
  TORCH_CHECK(w_out.is_contiguous() && w_out.numel() == B,
              "w_out must be a contiguous fp32 tensor of B entries");
  const int per = (int)(B / T);
  const long nb = (cap + PER_BLOCK - 1) / PER_BLOCK;
  auto opt = states.options();
  auto o_s = torch::empty({B, Ds}, opt);
  auto o_a = torch::empty({B, Da}, opt);
  auto o_r = torch::empty({B, 1}, opt);
  auto o_ns = torch::empty({B, Ds}, opt);
  auto o_d = torch::empty({B, 1}, opt);
  hipLaunchKernelGGL(k_replay_sample_per, dim3((B + 3) / 4), dim3(256), 0,
                     cur_stream(), states.data_ptr<float>(),
                     actions.data_ptr<float>(), rewards.data_ptr<float>(),
                     next_states.data_ptr<float>(), dones.data_ptr<float>(),
                     sizes.data_ptr<float>(), prio.data_ptr<float>(),
                     bsum.data_ptr<float>(), total.data_ptr<float>(),
                     beta.data_ptr<float>(),
                     (const long long*)rng.data_ptr<long>(),
                     o_s.data_ptr<float>(), o_a.data_ptr<float>(),
                     o_r.data_ptr<float>(), o_ns.data_ptr<float>(),
                     o_d.data_ptr<float>(),
                     (long long*)idx_out.data_ptr<long>(),
                     w_out.data_ptr<float>(), (int)B, (int)T, per, cap,
                     (int)nb, (int)Ds, (int)Da);
  return {o_s, o_a, o_r, o_ns, o_d};
}

// critic_td_loss with IS weights `isw` (raw, [B]).  Returns {closs[8],
// dq[2,B,1] bf16, new_prio[B]}.  Given `prio` (the [T, cap] leaves) and `idx`
// (the rows' flat indices, int64 [B]) it also zeroes the sampled leaves, the
// first step of the write-back (per_update with zeroed = true follows).
static std::vector<torch::Tensor> critic_td_loss_per(
    torch::Tensor r, torch::Tensor d, torch::Tensor q1t, torch::Tensor q2t,
    torch::Tensor nlp, torch::Tensor q1, torch::Tensor q2,
    torch::Tensor states, torch::Tensor log_alpha, long T, long use_w,
    double gamma, double rs, torch::Tensor ws, torch::Tensor isw,
    double per_alpha, double per_eps,
    c10::optional<torch::Tensor> prio = c10::nullopt,
    c10::optional<torch::Tensor> idx = c10::nullopt) {
  CHECK_IN(r); CHECK_IN(d); CHECK_IN(q1t); CHECK_IN(q2t); CHECK_IN(nlp);
  CHECK_IN(q1); CHECK_IN(q2); CHECK_IN(states); CHECK_IN(log_alpha);
  CHECK_IN(ws); CHECK_IN(isw);
  const long B = q1.size(0);
  const long nblk = (B + 255) / 256;
  TORCH_CHECK(B >= 1 && nblk <= 32, "critic_td_loss_per: 1 <= B <= 8192");
  TORCH_CHECK(T >= 1 && T <= 32 && log_alpha.numel() >= T, "T <= 32");
  TORCH_CHECK(ws.numel() >= 1 + 32 * 3, "workspace too small");
  TORCH_CHECK(states.dim() == 2 && states.is_contiguous()
              && states.size(0) == B && states.size(1) >= T);
  TORCH_CHECK(isw.is_contiguous() && isw.numel() == B,
              "IS weights must be a contiguous fp32 tensor of B entries");
  TORCH_CHECK(per_alpha >= 0.0 && per_eps >= 0.0,
              "per_alpha and per_eps must not be negative");
  TORCH_CHECK(prio.has_value() == idx.has_value(),
              "give both prio and idx, or neither");
  float* prio_p = nullptr;
  const long long* idx_p = nullptr;
  long n_prio = 0;
  if (prio.has_value()) {
    CHECK_IN(*prio);
    TORCH_CHECK(prio->is_contiguous(), "priorities must be contiguous");
    TORCH_CHECK(idx->is_cuda() && idx->scalar_type() == torch::kInt64
                && idx->is_contiguous() && idx->numel() == B,
                "idx must be a contiguous int64 HIP tensor of B entries");
    prio_p = prio->data_ptr<float>();
    idx_p = (const long long*)idx->data_ptr<long>();
    n_prio = prio->numel();
  }
  auto rc = r.contiguous(); auto dc = d.contiguous();
  auto q1tc = q1t.contiguous(); auto q2tc = q2t.contiguous();
  auto lpc = nlp.contiguous();
  auto q1c = q1.contiguous(); auto q2c = q2.contiguous();
  TORCH_CHECK(rc.numel() == B && dc.numel() == B && q1tc.numel() == B
              && q2tc.numel() == B && lpc.numel() == B && q1c.numel() == B
              && q2c.numel() == B, "critic_td_loss_per: B elements per input");
  const long oh_stride = states.size(1);
  const float* oh = states.data_ptr<float>() + (oh_stride - T);
  auto out = torch::empty({8}, q1.options());
  auto dq = torch::empty({2, B, 1}, q1.options().dtype(torch::kBFloat16));
  auto newp = torch::empty({B}, q1.options());
  hipLaunchKernelGGL(k_critic_td_loss_per, dim3(nblk), dim3(256), 0,
                     cur_stream(), rc.data_ptr<float>(),
                     dc.data_ptr<float>(), q1tc.data_ptr<float>(),
                     q2tc.data_ptr<float>(), lpc.data_ptr<float>(),
                     q1c.data_ptr<float>(), q2c.data_ptr<float>(), oh,
                     log_alpha.data_ptr<float>(), out.data_ptr<float>(),
                     ws.data_ptr<float>(), (unsigned short*)dq.data_ptr(),
                     (int)B, (int)T, (int)oh_stride, (int)use_w,
                     (float)gamma, (float)rs, isw.data_ptr<float>(),
                     newp.data_ptr<float>(), prio_p, idx_p, n_prio,
                     (float)per_alpha, (float)per_eps);
  return {out, dq, newp};
}

// Priority write-back: leaves[idx] = max over duplicates of newp, max_prio
// raised, touched blocks and all totals re-summed.  zeroed: the sampled
// leaves were already zeroed (critic_td_loss_per did it).
static void per_update(torch::Tensor prio, torch::Tensor bsum,
                       torch::Tensor total, torch::Tensor maxp,
                       torch::Tensor idx, torch::Tensor newp,
                       torch::Tensor ws, bool zeroed) {
  TORCH_CHECK(prio.dim() == 2, "priorities must be [T, cap]");
  const long T = prio.size(0), cap = prio.size(1);
  per_check_state(prio, bsum, total, T, cap);
  per_check_ws(ws);
  CHECK_IN(maxp); CHECK_IN(newp);
  TORCH_CHECK(maxp.is_contiguous() && maxp.numel() == T,
              "max_prio must hold one entry per task");
  const long B = idx.numel();
  TORCH_CHECK(idx.is_cuda() && idx.scalar_type() == torch::kInt64
              && idx.is_contiguous(),
              "indices must be a contiguous int64 HIP tensor");
  TORCH_CHECK(newp.is_contiguous() && newp.numel() == B,
              "one new priority per index");
  TORCH_CHECK(B <= 8192, "per_update: at most 8192 rows");
  if (B == 0) return;
  const long nb = (cap + PER_BLOCK - 1) / PER_BLOCK;
  const long long* ip = (const long long*)idx.data_ptr<long>();
  auto st = cur_stream();
  if (!zeroed)
    hipLaunchKernelGGL(k_per_zero, dim3((B + 255) / 256), dim3(256), 0, st,
                       prio.data_ptr<float>(), ip, (int)B, T * cap);
  hipLaunchKernelGGL(k_per_max, dim3((B + 255) / 256), dim3(256), 0, st,
                     prio.data_ptr<float>(), maxp.data_ptr<float>(), ip,
                     newp.data_ptr<float>(), (int)B, cap, T * cap);
  hipLaunchKernelGGL(k_per_resum,
                     dim3((B + PER_RESUM_ROWS - 1) / PER_RESUM_ROWS),
                     dim3(PER_RESUM_ROWS * 64), 0, st,
                     prio.data_ptr<float>(), bsum.data_ptr<float>(),
                     total.data_ptr<float>(), ip,
                     (unsigned*)ws.data_ptr<int>(), (int)B, (int)T, cap,
                     (int)nb, T * cap);
}

// Ingest hook, one shard: rows [start, start + rows) mod cap of shard t
// receive max_prio[t].
static void per_ingest_range(torch::Tensor prio, torch::Tensor bsum,
                             torch::Tensor total, torch::Tensor maxp,
                             torch::Tensor ws, long t, long start,
                             long rows) {
  TORCH_CHECK(prio.dim() == 2, "priorities must be [T, cap]");
  const long T = prio.size(0), cap = prio.size(1);
  per_check_state(prio, bsum, total, T, cap);
  per_check_ws(ws);
  CHECK_IN(maxp);
  TORCH_CHECK(maxp.is_contiguous() && maxp.numel() == T,
              "max_prio must hold one entry per task");
  TORCH_CHECK(t >= 0 && t < T && start >= 0 && start < cap && rows >= 0
              && rows <= cap, "per_ingest_range: range outside the shard");
  if (rows == 0) return;
  const long nb = (cap + PER_BLOCK - 1) / PER_BLOCK;
  hipLaunchKernelGGL(k_per_ingest, dim3(nb, 1), dim3(256), 0, cur_stream(),
                     (const float*)nullptr, 0, 0, (int)t, (int)start,
                     (int)rows, prio.data_ptr<float>(),
                     bsum.data_ptr<float>(), total.data_ptr<float>(),
                     maxp.data_ptr<float>(),
                     (unsigned*)ws.data_ptr<int>() + 1, cap, (int)nb);
}

// Ingest hook of the packed path: one launch per batch, reading the
// descriptors of the staged batch on the device.  `header` is the host copy
// (checked here, as replay_ingest does).
static void per_ingest_packed(torch::Tensor staging, torch::Tensor header,
                              torch::Tensor prio, torch::Tensor bsum,
                              torch::Tensor total, torch::Tensor maxp,
                              torch::Tensor ws) {
  CHECK_IN(staging);
  TORCH_CHECK(prio.dim() == 2, "priorities must be [T, cap]");
  const long T = prio.size(0), cap = prio.size(1);
  per_check_state(prio, bsum, total, T, cap);
  per_check_ws(ws);
  CHECK_IN(maxp);
  TORCH_CHECK(maxp.is_contiguous() && maxp.numel() == T,
              "max_prio must hold one entry per task");
  TORCH_CHECK(header.device().is_cpu() &&
                  header.scalar_type() == torch::kFloat32 &&
                  header.is_contiguous() && staging.is_contiguous(),
              "header must be a contiguous fp32 host tensor");
  const long hn = header.numel();
  TORCH_CHECK(hn >= PK_HDR + T, "packed header truncated");
  const int32_t* h = reinterpret_cast<const int32_t*>(
      header.data_ptr<float>());
  const long n_desc = h[0];
  TORCH_CHECK(h[1] == T, "packed batch built for another task count");
  TORCH_CHECK(n_desc >= 1 && PK_HDR + T + n_desc * PK_DESC <= hn
              && PK_HDR + T + n_desc * PK_DESC <= staging.numel(),
              "packed descriptor count out of range");
  for (long k = 0; k < n_desc; ++k) {
    const int32_t* d = h + PK_HDR + T + k * PK_DESC;
    TORCH_CHECK(d[0] >= 0 && d[0] < T && d[3] >= 1 && d[3] <= cap
                && d[5] >= 0 && d[5] < cap,
                "packed descriptor out of range");
  }
  const long nb = (cap + PER_BLOCK - 1) / PER_BLOCK;
  hipLaunchKernelGGL(k_per_ingest, dim3(nb, T), dim3(256), 0, cur_stream(),
                     staging.data_ptr<float>(), (int)n_desc, (int)T, 0, 0, 0,
                     prio.data_ptr<float>(), bsum.data_ptr<float>(),
                     total.data_ptr<float>(), maxp.data_ptr<float>(),
                     (unsigned*)ws.data_ptr<int>() + 1, cap, (int)nb);
}

void register_shm_ring(pybind11::module_& m);
void register_bf16(pybind11::module_& m);
void register_chain(pybind11::module_& m);

PYBIND11_MODULE(TORCH_EXTENSION_NAME, mod) {
  register_shm_ring(mod);
  register_bf16(mod);
  register_chain(mod);
  mod.def("linear_act_fwd", &linear_act_fwd, "fused GEMM+bias+act forward");
  mod.def("linear_act_fwd_g", &linear_act_fwd_g, "grouped (twin) variant");
  mod.def("linear_bwd_dx", &linear_bwd_dx, "GEMM backward dX (fused mask)");
  mod.def("linear_bwd_dx_g", &linear_bwd_dx_g, "grouped, sums over G");
  mod.def("linear_bwd_dwdb", &linear_bwd_dwdb, "split-K backward dW+db");
  mod.def("linear_bwd_dwdb_g", &linear_bwd_dwdb_g, "grouped split-K dW+db");
  mod.def("replay_sample", &replay_sample, "stratified replay gather",
          pybind11::arg("states"), pybind11::arg("actions"),
          pybind11::arg("rewards"), pybind11::arg("next_states"),
          pybind11::arg("dones"), pybind11::arg("sizes"),
          pybind11::arg("rnd"), pybind11::arg("B"),
          pybind11::arg("rng") = pybind11::none());
  mod.def("replay_sample_norepl", &replay_sample_norepl,
          "stratified replay gather, without replacement",
          pybind11::arg("states"), pybind11::arg("actions"),
          pybind11::arg("rewards"), pybind11::arg("next_states"),
          pybind11::arg("dones"), pybind11::arg("sizes"),
          pybind11::arg("B"), pybind11::arg("rng"),
          pybind11::arg("idx_out") = pybind11::none());
  mod.def("replay_ingest", &replay_ingest, "packed replay scatter",
          pybind11::arg("staging"), pybind11::arg("header"),
          pybind11::arg("states"), pybind11::arg("actions"),
          pybind11::arg("rewards"), pybind11::arg("next_states"),
          pybind11::arg("dones"), pybind11::arg("sizes"));
  mod.def("replay_sample_per", &replay_sample_per,
          "stratified proportional (prioritized) replay gather",
          pybind11::arg("states"), pybind11::arg("actions"),
          pybind11::arg("rewards"), pybind11::arg("next_states"),
          pybind11::arg("dones"), pybind11::arg("sizes"),
          pybind11::arg("prio"), pybind11::arg("bsum"),
          pybind11::arg("total"), pybind11::arg("beta"), pybind11::arg("B"),
          pybind11::arg("rng"), pybind11::arg("idx_out"),
          pybind11::arg("w_out"));
  mod.def("critic_td_loss_per", &critic_td_loss_per,
          pybind11::arg("r"), pybind11::arg("d"), pybind11::arg("q1t"),
          pybind11::arg("q2t"), pybind11::arg("nlp"), pybind11::arg("q1"),
          pybind11::arg("q2"), pybind11::arg("states"),
          pybind11::arg("log_alpha"), pybind11::arg("T"),
          pybind11::arg("use_w"), pybind11::arg("gamma"),
          pybind11::arg("rs"), pybind11::arg("ws"), pybind11::arg("isw"),
          pybind11::arg("per_alpha"), pybind11::arg("per_eps"),
          pybind11::arg("prio") = pybind11::none(),
          pybind11::arg("idx") = pybind11::none());
  mod.def("per_update", &per_update, "prioritized replay write-back",
          pybind11::arg("prio"), pybind11::arg("bsum"),
          pybind11::arg("total"), pybind11::arg("maxp"), pybind11::arg("idx"),
          pybind11::arg("newp"), pybind11::arg("ws"),
          pybind11::arg("zeroed") = false);
  mod.def("per_ingest_range", &per_ingest_range,
          pybind11::arg("prio"), pybind11::arg("bsum"),
          pybind11::arg("total"), pybind11::arg("maxp"), pybind11::arg("ws"),
          pybind11::arg("t"), pybind11::arg("start"), pybind11::arg("rows"));
  mod.def("per_ingest_packed", &per_ingest_packed,
          pybind11::arg("staging"), pybind11::arg("header"),
          pybind11::arg("prio"), pybind11::arg("bsum"),
          pybind11::arg("total"), pybind11::arg("maxp"), pybind11::arg("ws"));
  mod.def("squashed_gaussian_fwd", &squashed_gaussian_fwd,
          pybind11::arg("mu"), pybind11::arg("lsr"),
          pybind11::arg("eps"), pybind11::arg("k"),
          pybind11::arg("rng") = pybind11::none());
  mod.def("squashed_gaussian_bwd", &squashed_gaussian_bwd);
  mod.def("td_target", &td_target);
  mod.def("td_target_mt", &td_target_mt);
  mod.def("critic_loss_fwd", &critic_loss_fwd,
          pybind11::arg("q1"), pybind11::arg("q2"),
          pybind11::arg("y"), pybind11::arg("states"),
          pybind11::arg("log_alpha"), pybind11::arg("T"),
          pybind11::arg("use_w"),
          pybind11::arg("ws") = pybind11::none());
  mod.def("critic_loss_bwd", &critic_loss_bwd);
  mod.def("actor_alpha_loss_fwd", &actor_alpha_loss_fwd,
          pybind11::arg("aq1"), pybind11::arg("aq2"),
          pybind11::arg("lp"), pybind11::arg("ls"),
          pybind11::arg("states"), pybind11::arg("log_alpha"),
          pybind11::arg("T"), pybind11::arg("use_w"),
          pybind11::arg("H_bar"),
          pybind11::arg("dla") = pybind11::none(),
          pybind11::arg("ws") = pybind11::none());
  mod.def("actor_alpha_loss_bwd", &actor_alpha_loss_bwd);
  mod.def("critic_loss_bwd2", &critic_loss_bwd2);
  mod.def("actor_alpha_loss_bwd2", &actor_alpha_loss_bwd2,
          pybind11::arg("aq1"), pybind11::arg("aq2"), pybind11::arg("lp"),
          pybind11::arg("states"), pybind11::arg("log_alpha"),
          pybind11::arg("saved"), pybind11::arg("dla_out"),
          pybind11::arg("T"), pybind11::arg("use_w"), pybind11::arg("H_bar"),
          pybind11::arg("ws") = pybind11::none());
  mod.def("critic_td_loss", &critic_td_loss,
          pybind11::arg("r"), pybind11::arg("d"), pybind11::arg("q1t"),
          pybind11::arg("q2t"), pybind11::arg("nlp"), pybind11::arg("q1"),
          pybind11::arg("q2"), pybind11::arg("states"),
          pybind11::arg("log_alpha"), pybind11::arg("T"),
          pybind11::arg("use_w"), pybind11::arg("gamma"),
          pybind11::arg("rs"), pybind11::arg("ws"));
  mod.def("actor_alpha_loss_fwd_bwd", &actor_alpha_loss_fwd_bwd,
          pybind11::arg("aq1"), pybind11::arg("aq2"), pybind11::arg("lp"),
          pybind11::arg("ls"), pybind11::arg("states"),
          pybind11::arg("log_alpha"), pybind11::arg("dla"),
          pybind11::arg("T"), pybind11::arg("use_w"), pybind11::arg("H_bar"),
          pybind11::arg("ws"), pybind11::arg("wsum") = pybind11::none());
  mod.def("squashed_gaussian_bwd2", &squashed_gaussian_bwd2);
  mod.def("adam_step_", &adam_step_);
  mod.def("adam_step_dev_", &adam_step_dev_,
          pybind11::arg("p"), pybind11::arg("g"), pybind11::arg("m"),
          pybind11::arg("v"), pybind11::arg("state"), pybind11::arg("lr"),
          pybind11::arg("b1"), pybind11::arg("b2"), pybind11::arg("eps"),
          pybind11::arg("mir") = pybind11::none(),
          pybind11::arg("skip_prolog") = 0,
          pybind11::arg("arena") = pybind11::none(),
          pybind11::arg("S") = 0);
  mod.def("adam_step_multi_", &adam_step_multi_,
          pybind11::arg("ps"), pybind11::arg("gs"), pybind11::arg("ms"),
          pybind11::arg("vs"), pybind11::arg("states"), pybind11::arg("lrs"),
          pybind11::arg("b1"), pybind11::arg("b2"), pybind11::arg("eps"),
          pybind11::arg("mirs") = std::vector<torch::Tensor>(),
          pybind11::arg("rng") = pybind11::none(),
          pybind11::arg("skip_prolog") = 0,
          pybind11::arg("arena0") = pybind11::none(),
          pybind11::arg("S0") = 0,
          pybind11::arg("polyak_t") = pybind11::none(),
          pybind11::arg("polyak_s") = pybind11::none(),
          pybind11::arg("tau") = 0.0,
          pybind11::arg("polyak_mir") = pybind11::none());
  mod.def("grad_sumsq_", &grad_sumsq_,
          pybind11::arg("gs"), pybind11::arg("slots"),
          pybind11::arg("arena0") = pybind11::none(),
          pybind11::arg("S0") = 0);
  mod.def("adam_step_clip_", &adam_step_clip_,
          pybind11::arg("ps"), pybind11::arg("gs"), pybind11::arg("ms"),
          pybind11::arg("vs"), pybind11::arg("states"), pybind11::arg("lrs"),
          pybind11::arg("b1"), pybind11::arg("b2"), pybind11::arg("eps"),
          pybind11::arg("mirs"), pybind11::arg("slots"),
          pybind11::arg("maxn"), pybind11::arg("clip_states"),
          pybind11::arg("skips"),
          pybind11::arg("rng") = pybind11::none(),
          pybind11::arg("skip_prolog") = 0,
          pybind11::arg("arena0") = pybind11::none(),
          pybind11::arg("S0") = 0,
          pybind11::arg("polyak_t") = pybind11::none(),
          pybind11::arg("polyak_s") = pybind11::none(),
          pybind11::arg("tau") = 0.0,
          pybind11::arg("polyak_mir") = pybind11::none());
  mod.def("adam_prolog_many", &adam_prolog_many,
          pybind11::arg("states"), pybind11::arg("lrs"),
          pybind11::arg("b1"), pybind11::arg("b2"),
          pybind11::arg("rng") = pybind11::none());
  mod.def("polyak_", &polyak_,
          pybind11::arg("t"), pybind11::arg("s"), pybind11::arg("tau"),
          pybind11::arg("mir") = pybind11::none());
}
