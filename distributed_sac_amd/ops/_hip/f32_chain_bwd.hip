// f32_chain_bwd.hip — whole-chain fp32 MLP backward on
// v_mfma_f32_16x16x4_f32 (gfx950): one dx-walk launch and one grouped
// split-K dW/db launch per MLP, where the per-layer path takes up to five
// launches per layer.  Same rules as f32_chain.hip: weights are read in
// place as [G, N, K] k-minor views of the flat parameter buffer (no mirror,
// no packing pass), every width <= 768, <= 6 layers, every check in the
// binding, descriptors by value, no host sync, no atomics.
//
// k_f32_chain_dx — grid (ceil(M/16), 1, G), 512 threads.  A workgroup owns
// 16 batch rows of one group and walks l = L-1 .. 1:
//     dy_{l-1} = (dy_l @ W_l), 0 where a_{l-1} <= 0
// (k_linear_bwd_dx's comparison: a NaN activation keeps its gradient).  The
// running gradient lives in two ping-pong LDS buffers float[16][772]; after
// each layer's barrier one coalesced pass masks the tile in place against
// a_{l-1} (read from global as float4) and stores dy_{l-1} for the dW
// kernel.  With an input gradient, layer 0 lands in a third LDS tile:
//     dx0 [M, K_0 - lo] = sum_g dy_0[g] @ W_0[g][:, lo:]
// For G > 1 that launch is (ceil(M/16), 1, 1) and the workgroup walks the
// groups one after another; group g > 0 starts its layer-0 accumulators
// from the tile group g - 1 left, so the sum is made in group order with no
// float atomics and no second launch.  3 * 16 * 772 * 4 = 148,224 B static
// LDS (gfx950 has 160 KB per CU), one workgroup per CU as in the forward.
//
// Operand mapping: the reduction runs over n and W's minor dimension is
// the OUTPUT column, the forward's mapping transposed.  Per 16-wide n-step
// lane (fj = lane & 15, fk = lane >> 4) reads dy[fj][n0 + 4 fk .. +3] as
// one ds_read_b128 and, for s = 0..3, W[n0 + 4 fk + s][c0 + 4 fj .. +3] as
// one float4 — 4 weight rows x 256 contiguous bytes per load instruction —
// and issues 16 MFMAs into four accumulators; accumulator q, column fj, is
// output column c0 + 4 fj + q.  That permutation inside a wave's 64-column
// block is undone for free by the epilogue: a lane holds four CONSECUTIVE
// columns of each of its rows and stores them as one ds_write_b128.
//
// Branch-free body as in the forward: out-of-range columns are clamped to a
// valid address and written as 0 by the epilogue (which thereby zeroes the
// pad [K, ceil64(K)) the next layer's n-tail reads), the n-tail's weight
// rows are clamped and selected to 0, and rows that are not 16-byte aligned
// (K % 4 != 0, the 57-wide layer 0, an unaligned view or column offset)
// take an index-clamped per-element loader.
//
// k_f32_chain_dwdb — grid (jobs, S), 64 threads.  Both operands of
// dW_l[n][k] = sum_m dy_l[m][n] a_l[m][k] are batch-major, so neither needs
// LDS or a transpose: per 4-row m-step lane (fi, fk) reads
// dy[m0 + fk][n0 + 4 fi .. +3] and a[m0 + fk][c0 + 4 fi .. +3], one float4
// each, and issues the 16 MFMAs of a 64 x 64 output tile (4 x 4 permuted
// 16-tiles, 64 accumulator VGPRs); loads are double-buffered.  A by-value
// prefix table maps blockIdx.x to a (layer, group, n-block, k-block) job,
// blockIdx.y is the split-K slice, and every layer of the chain shares the
// grid.  db is the row sum of the dy tile, made by the k-block 0 job of
// each n-block as four more MFMAs against a column of ones.  The partials
// go to an arena [S, total] that k_reduce_arena folds in slice order.

#include <hip/hip_runtime.h>
#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>
#include <c10/hip/HIPStream.h>

#include <cstdint>
#include <tuple>
#include <vector>

namespace f32chainbwd {

using f32x4 = __attribute__((__vector_size__(4 * sizeof(float)))) float;

static constexpr int FMAX = 768;        // max layer / input width
static constexpr int FPAD = FMAX + 4;   // LDS row stride: 772 = 4 mod 64
static constexpr int FROWS = 16;        // batch rows per workgroup
static constexpr int FTHR = 512;        // 8 waves
static constexpr int FLAYERS = 6;
static constexpr int DWT = 64;          // dW tile edge

struct F32DxDesc {
  const float* w[FLAYERS];      // [G, N_l, K_l] fp32, k-minor
  const float* mask[FLAYERS];   // l >= 1: a_{l-1} [G, M, K_l]
  float* dys[FLAYERS];          // l >= 1: dy_{l-1} [G, M, K_l]
  int N[FLAYERS];
  int K0;
  int L;
};

struct F32DwDesc {
  const float* dy[FLAYERS];     // masked dy_l [G, M, N_l]
  const float* a[FLAYERS];      // layer input [G, M, K_l] or shared [M, K_l]
  long ags[FLAYERS];            // group stride of a (0: shared)
  long woff[FLAYERS];           // dW_l [G, N_l, K_l] inside a slice
  long boff[FLAYERS];           // db_l [G, N_l] inside a slice
  int N[FLAYERS];
  int K[FLAYERS];
  int jend[FLAYERS];            // tile jobs of layers 0 .. l
  int L;
};

// Packed fp32 ops stay out of these kernels (see f32_chain.hip).
#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute push(                                             \
    __attribute__((target("no-packed-fp32-ops"))), apply_to = function)
#endif

// p[c .. c + 3] of one row of width lim.  Elements at or past lim, and the
// whole vector when !rok, come back as 0; every address is clamped into the
// row, so nothing is branched around.  vec: one 16-byte load (the caller
// has checked lim % 4 == 0 and the row's alignment).
__device__ __forceinline__ f32x4 ld4(const float* __restrict__ p, int c,
                                     int lim, bool vec, bool rok) {
  f32x4 v;
  if (vec) {
    const bool ok = rok && c < lim;
    v = *(const f32x4*)&p[c < lim ? c : 0];
    v = ok ? v : f32x4{0.f, 0.f, 0.f, 0.f};
  } else {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int cc = c + q;
      const float x = p[cc < lim ? cc : 0];
      v[q] = (rok && cc < lim) ? x : 0.f;
    }
  }
  return v;
}

// dst[16][0 .. ceil64(Kw)) (+)= src[16][N] @ wg[N][0 .. Kw), wg's row
// stride ldw.  src's columns [N, ceil16(N)) are zero.  dst's columns at or
// past Kw are written as 0.  accum: the accumulators start from dst.
__device__ __forceinline__ void dx_gemm(
    const float (*__restrict__ src)[FPAD], float (*__restrict__ dst)[FPAD],
    const float* __restrict__ wg, int N, int Kw, int ldw, bool accum,
    int wid, int fj, int fk) {
  const bool vec = ((ldw | Kw) & 3) == 0 && ((uintptr_t)wg & 15) == 0;
  const int nbody = vec ? (N & ~15) : 0;
  for (int c0 = wid * 64; c0 < Kw; c0 += 64 * (FTHR / 64)) {
    const int cb = c0 + 4 * fj;      // this lane's four output columns
    f32x4 acc[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) acc[q] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (accum) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const f32x4 t = *(const f32x4*)&dst[4 * fk + r][cb];
#pragma unroll
        for (int q = 0; q < 4; ++q) acc[q][r] = t[q];
      }
    }

#define DX_MF4(As, Bs)                                                    \
    {                                                                     \
      _Pragma("unroll") for (int s = 0; s < 4; ++s)                       \
        _Pragma("unroll") for (int q = 0; q < 4; ++q)                     \
          acc[q] = __builtin_amdgcn_mfma_f32_16x16x4f32(                  \
              As[s], Bs[s][q], acc[q], 0, 0, 0);                          \
    }

    if (nbody > 0) {
      // an out-of-range lane loads column 0; its result is never kept
      const float* __restrict__ wp =
          wg + (long)(4 * fk) * ldw + (cb < Kw ? cb : 0);
#define DX_LOAD(As, Bs, nn)                                               \
      {                                                                   \
        _Pragma("unroll") for (int s = 0; s < 4; ++s)                     \
          Bs[s] = *(const f32x4*)&wp[(long)((nn) + s) * ldw];             \
        As = *(const f32x4*)&src[fj][(nn) + 4 * fk];                      \
      }
      f32x4 A0, A1, B0[4], B1[4];
      int n = 0;
      DX_LOAD(A0, B0, 0)
      while (n + 32 <= nbody) {
        DX_LOAD(A1, B1, n + 16)
        DX_MF4(A0, B0)
        if (n + 32 < nbody) DX_LOAD(A0, B0, n + 32)
        DX_MF4(A1, B1)
        n += 32;
      }
      if (n < nbody) DX_MF4(A0, B0)
#undef DX_LOAD
    }
    // n-tail (N % 16 rows) and every step of an unaligned layer: clamped
    // rows, values selected to 0 so a non-finite weight cannot meet a pad
    for (int n0 = nbody; n0 < N; n0 += 16) {
      f32x4 At, Bt[4];
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        const int nr = n0 + 4 * fk + s;
        const bool rok = nr < N;
        Bt[s] = ld4(wg + (long)(rok ? nr : N - 1) * ldw, cb, Kw, vec, rok);
      }
      At = *(const f32x4*)&src[fj][n0 + 4 * fk];
      DX_MF4(At, Bt)
    }
#undef DX_MF4

    // C/D map: col = lane & 15, row = (lane >> 4) * 4 + r, so acc[0..3][r]
    // are columns cb .. cb + 3 of row 4 fk + r: one 16-byte LDS store
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      f32x4 v;
#pragma unroll
      for (int q = 0; q < 4; ++q) v[q] = (cb + q < Kw) ? acc[q][r] : 0.f;
      *(f32x4*)&dst[4 * fk + r][cb] = v;
    }
  }
}

__global__ __launch_bounds__(FTHR) void k_f32_chain_dx(
    const float* __restrict__ dy, F32DxDesc d, float* __restrict__ dx0,
    int lo, int M, int G, int serial) {
  // [0], [1]: the running gradient; [2]: the dx0 tile
  __shared__ __attribute__((aligned(16))) float sa[3][FROWS][FPAD];
  const int m0 = blockIdx.x * FROWS;
  const int tid = threadIdx.x;
  const int lane = tid & 63, wid = tid >> 6;
  const int fj = lane & 15, fk = lane >> 4;
  const int rowlim = (M - m0 < FROWS) ? M - m0 : FROWS;
  const int g_lo = serial ? 0 : (int)blockIdx.z;
  const int g_hi = serial ? G : g_lo + 1;
  const int NL = d.N[d.L - 1];

  for (int g = g_lo; g < g_hi; ++g) {
    // ---- dy tile -> sa[0]; rows >= rowlim and columns [NL, ceil16(NL))
    // are written as zeros.  32 threads per row.
    {
      const int r = tid >> 5, lc = tid & 31;
      const long row = (long)g * M + m0 + r;
      const int npad = (NL + 15) & ~15;
      for (int c = lc; c < npad; c += 32)
        sa[0][r][c] = (r < rowlim && c < NL) ? dy[row * NL + c] : 0.f;
    }
    __syncthreads();

    int cur = 0;
    for (int l = d.L - 1; l >= 1; --l) {
      const int N = d.N[l], K = d.N[l - 1];
      dx_gemm(sa[cur], sa[cur ^ 1], d.w[l] + (long)g * N * K, N, K, K,
              false, wid, fj, fk);
      __syncthreads();
      cur ^= 1;
      // mask against a_{l-1} in place and store dy_{l-1}, coalesced
      const long off = ((long)g * M + m0) * K;
      const float* __restrict__ ag = d.mask[l] + off;
      float* __restrict__ og = d.dys[l] + off;
      if ((K & 3) == 0 && (((uintptr_t)ag | (uintptr_t)og) & 15) == 0) {
        const int n4 = K >> 2;
        for (int i = tid; i < rowlim * n4; i += FTHR) {
          const int r = i / n4, c = (i - r * n4) * 4;
          const f32x4 a = *(const f32x4*)&ag[(long)r * K + c];
          f32x4 v = *(const f32x4*)&sa[cur][r][c];
#pragma unroll
          for (int q = 0; q < 4; ++q) v[q] = (a[q] <= 0.f) ? 0.f : v[q];
          *(f32x4*)&sa[cur][r][c] = v;
          *(f32x4*)&og[(long)r * K + c] = v;
        }
      } else {
        for (int i = tid; i < rowlim * K; i += FTHR) {
          const int r = i / K, c = i - r * K;
          float v = sa[cur][r][c];
          v = (ag[(long)r * K + c] <= 0.f) ? 0.f : v;
          sa[cur][r][c] = v;
          og[(long)r * K + c] = v;
        }
      }
      __syncthreads();
    }
    if (dx0 != nullptr)
      dx_gemm(sa[cur], sa[2], d.w[0] + (long)g * d.N[0] * d.K0 + lo,
              d.N[0], d.K0 - lo, d.K0, g > g_lo, wid, fj, fk);
    __syncthreads();   // the next group's loader overwrites sa[0]
  }

  if (dx0 != nullptr) {
    const int Kw = d.K0 - lo;
    float* __restrict__ og = dx0 + (long)m0 * Kw;
    if ((Kw & 3) == 0 && ((uintptr_t)og & 15) == 0) {
      const int n4 = Kw >> 2;
      for (int i = tid; i < rowlim * n4; i += FTHR) {
        const int r = i / n4, c = (i - r * n4) * 4;
        *(f32x4*)&og[(long)r * Kw + c] = *(const f32x4*)&sa[2][r][c];
      }
    } else {
      for (int i = tid; i < rowlim * Kw; i += FTHR) {
        const int r = i / Kw, c = i - r * Kw;
        og[(long)r * Kw + c] = sa[2][r][c];
      }
    }
  }
}

__global__ __launch_bounds__(64) void k_f32_chain_dwdb(
    F32DwDesc d, float* __restrict__ arena, long total, int M, int chunk) {
  int job = blockIdx.x;
  int l = 0;
  while (l < d.L - 1 && job >= d.jend[l]) ++l;
  if (l > 0) job -= d.jend[l - 1];
  const int N = d.N[l], K = d.K[l];
  const int nbk = (K + DWT - 1) / DWT;
  const int per_g = ((N + DWT - 1) / DWT) * nbk;
  const int g = job / per_g;
  const int rem = job - g * per_g;
  const int nb = rem / nbk, kb = rem - nb * nbk;
  const int lane = threadIdx.x;
  const int fi = lane & 15, fk = lane >> 4;
  const int cn = nb * DWT + 4 * fi;   // this lane's dy columns (dW rows)
  const int ck = kb * DWT + 4 * fi;   // this lane's a columns (dW columns)
  const float* __restrict__ dyg = d.dy[l] + (long)g * M * N;
  const float* __restrict__ ag = d.a[l] + g * d.ags[l];
  const bool vdy = (N & 3) == 0 && ((uintptr_t)dyg & 15) == 0;
  const bool va = (K & 3) == 0 && ((uintptr_t)ag & 15) == 0;
  const bool do_db = kb == 0;

  // slice s covers rows [s chunk, (s + 1) chunk), cut at M
  const long lo_l = (long)blockIdx.y * chunk;
  const int m_lo = lo_l < M ? (int)lo_l : M;
  const int m_hi = (M - m_lo < chunk) ? M : m_lo + chunk;

  f32x4 acc[4][4], accb[4];
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    accb[p] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int q = 0; q < 4; ++q) acc[p][q] = f32x4{0.f, 0.f, 0.f, 0.f};
  }

  // a row at or past m_hi is clamped to a valid one and read as zeros
#define DW_LOAD(Dv, Av, mm)                                               \
  {                                                                       \
    const int row_ = (mm) + fk;                                           \
    const bool rok_ = row_ < m_hi;                                        \
    const long rc_ = rok_ ? row_ : M - 1;                                 \
    Dv = ld4(dyg + rc_ * N, cn, N, vdy, rok_);                            \
    Av = ld4(ag + rc_ * K, ck, K, va, rok_);                              \
  }
#define DW_MF(Dv, Av)                                                     \
  {                                                                       \
    _Pragma("unroll") for (int p = 0; p < 4; ++p)                         \
      _Pragma("unroll") for (int q = 0; q < 4; ++q)                       \
        acc[p][q] = __builtin_amdgcn_mfma_f32_16x16x4f32(                 \
            Dv[p], Av[q], acc[p][q], 0, 0, 0);                            \
    if (do_db) {                                                          \
      _Pragma("unroll") for (int p = 0; p < 4; ++p)                       \
        accb[p] = __builtin_amdgcn_mfma_f32_16x16x4f32(                   \
            Dv[p], 1.f, accb[p], 0, 0, 0);                                \
    }                                                                     \
  }
  if (m_lo < m_hi) {
    f32x4 D0, A0, D1, A1;
    DW_LOAD(D0, A0, m_lo)
    for (int m = m_lo; m < m_hi; m += 8) {
      DW_LOAD(D1, A1, m + 4)
      DW_MF(D0, A0)
      DW_LOAD(D0, A0, m + 8)
      DW_MF(D1, A1)
    }
  }
#undef DW_LOAD
#undef DW_MF

  // acc[p][q][r] of lane (fi, fk) is dW[nb 64 + 16 fk + 4 r + p][ck + q]
  float* __restrict__ out = arena + (long)blockIdx.y * total;
  float* __restrict__ wo = out + d.woff[l] + (long)g * N * K;
  const bool vst = (K & 3) == 0 && ((uintptr_t)wo & 15) == 0;
#pragma unroll
  for (int p = 0; p < 4; ++p)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = nb * DWT + 16 * fk + 4 * r + p;
      if (row >= N) continue;
      if (vst) {
        if (ck < K)
          *(f32x4*)&wo[(long)row * K + ck] =
              f32x4{acc[p][0][r], acc[p][1][r], acc[p][2][r], acc[p][3][r]};
      } else {
#pragma unroll
        for (int q = 0; q < 4; ++q)
          if (ck + q < K) wo[(long)row * K + ck + q] = acc[p][q][r];
      }
      // every column of accb holds the row sum; column 0's lanes store it
      if (do_db && fi == 0) out[d.boff[l] + (long)g * N + row] = accb[p][r];
    }
}

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif

static inline hipStream_t cur_stream5() {
  return c10::hip::getCurrentHIPStream().stream();
}

#define F32B_CHECK(t)                                                     \
  TORCH_CHECK((t).is_cuda() && (t).scalar_type() == torch::kFloat32       \
              && (t).is_contiguous(),                                     \
              #t " must be a contiguous fp32 HIP tensor")

// The checks both bindings share.  ws[l]: [G, N_l, K_l] ([N_l, K_l] for
// G = 1); acts[l], the input of layer l: G * M * K_l elements (acts[0] may
// be one [M, K_0] shared by every group).  Fills N and K.
static void check_chain(const std::vector<torch::Tensor>& acts, long G,
                        long M, const torch::Device& dev, int L,
                        const long* N, long* K) {
  TORCH_CHECK((int)acts.size() == L, "f32 chain bwd: ", L,
              " layers need acts = [x, a_0 .. a_{L-2}], got ", acts.size());
  TORCH_CHECK(M >= 1 && M < (1L << 31) - 64, "f32 chain bwd: bad M");
  for (int l = 0; l < L; ++l) {
    F32B_CHECK(acts[l]);
    TORCH_CHECK(acts[l].device() == dev, "f32 chain bwd: acts[", l,
                "] is on another device");
    TORCH_CHECK(acts[l].dim() == 2 || acts[l].dim() == 3,
                "f32 chain bwd: acts[", l, "] must be [G, M, K] or [M, K]");
    K[l] = acts[l].size(-1);
    TORCH_CHECK(l == 0 || K[l] == N[l - 1], "f32 chain bwd: acts[", l,
                "] has width ", K[l], ", expected N of the layer before = ",
                l ? N[l - 1] : 0);
    TORCH_CHECK(K[l] >= 1 && K[l] <= FMAX && N[l] >= 1 && N[l] <= FMAX,
                "f32 chain bwd: layer ", l, " width ", N[l], " x ", K[l],
                " outside [1, ", FMAX, "]");
    const bool shared = l == 0 && acts[l].numel() == M * K[l];
    TORCH_CHECK(shared || acts[l].numel() == G * M * K[l],
                "f32 chain bwd: acts[", l, "] needs ", G * M * K[l],
                " elements");
    TORCH_CHECK(acts[l].size(-2) == M, "f32 chain bwd: acts[", l, "] has ",
                acts[l].size(-2), " rows, expected ", M);
  }
}

// ---------------------------------------------------------------------------
// (dys, dx0) = mlp_chain_bwd_dx_f32(dy, ws, acts, G, dx0_lo)
// dy [G, M, N_{L-1}] ([M, N] for G = 1); acts = [x, a_0 .. a_{L-2}] as the
// forward saves them.  dys = [dy_0 .. dy_{L-2}], dy_l shaped like a_l, the
// masked gradients.  dx0_lo < 0: dx0 is None; else dx0 is
// [M, K_0 - dx0_lo], summed over the groups in group order.
// ---------------------------------------------------------------------------
static std::tuple<std::vector<torch::Tensor>, c10::optional<torch::Tensor>>
mlp_chain_bwd_dx_f32(torch::Tensor dy, std::vector<torch::Tensor> ws,
                     std::vector<torch::Tensor> acts, long G, long dx0_lo) {
  const int L = (int)ws.size();
  TORCH_CHECK(L >= 1 && L <= FLAYERS, "f32 chain bwd: 1 <= L <= ", FLAYERS);
  TORCH_CHECK(G >= 1 && G <= 65535, "f32 chain bwd: bad G");
  F32B_CHECK(dy);
  TORCH_CHECK(dy.dim() == 3 || (G == 1 && dy.dim() == 2),
              "f32 chain bwd: dy must be [G, M, N]");
  const long M = dy.size(-2);
  long N[FLAYERS], K[FLAYERS];
  for (int l = 0; l < L; ++l) {
    F32B_CHECK(ws[l]);
    TORCH_CHECK(ws[l].device() == dy.device(), "f32 chain bwd: ws[", l,
                "] is on another device");
    TORCH_CHECK(ws[l].dim() == 3 || (G == 1 && ws[l].dim() == 2),
                "f32 chain bwd: ws[", l, "] must be [G, N, K]");
    TORCH_CHECK(ws[l].dim() == 2 || ws[l].size(0) == G,
                "f32 chain bwd: ws[", l, "] has ", ws[l].size(0),
                " groups, expected ", G);
    N[l] = ws[l].size(-2);
  }
  check_chain(acts, G, M, dy.device(), L, N, K);
  for (int l = 0; l < L; ++l)
    TORCH_CHECK(ws[l].size(-1) == K[l], "f32 chain bwd: ws[", l,
                "] has K = ", ws[l].size(-1), ", expected acts[", l,
                "]'s width ", K[l]);
  TORCH_CHECK(dy.size(-1) == N[L - 1] && dy.numel() == G * M * N[L - 1],
              "f32 chain bwd: dy must be [", G, ", ", M, ", ", N[L - 1],
              "]");
  TORCH_CHECK(dx0_lo <= K[0], "f32 chain bwd: dx0_lo = ", dx0_lo,
              " past the input width ", K[0]);

  F32DxDesc d{};
  d.L = L;
  d.K0 = (int)K[0];
  std::vector<torch::Tensor> dys;
  for (int l = 0; l < L; ++l) {
    d.w[l] = ws[l].data_ptr<float>();
    d.N[l] = (int)N[l];
    if (l >= 1) {
      dys.push_back(torch::empty_like(acts[l]));
      d.mask[l] = acts[l].data_ptr<float>();
      d.dys[l] = dys.back().data_ptr<float>();
    }
  }
  c10::optional<torch::Tensor> dx0;
  float* dx0p = nullptr;
  if (dx0_lo >= 0) {
    dx0 = torch::empty({M, K[0] - dx0_lo}, dy.options());
    if (dx0_lo < K[0]) dx0p = dx0->data_ptr<float>();
  }
  if (L == 1 && dx0p == nullptr) return {dys, dx0};   // nothing to compute
  const bool serial = dx0p != nullptr && G > 1;
  dim3 grid((unsigned)((M + FROWS - 1) / FROWS), 1,
            serial ? 1u : (unsigned)G);
  hipLaunchKernelGGL(k_f32_chain_dx, grid, dim3(FTHR), 0, cur_stream5(),
                     dy.data_ptr<float>(), d, dx0p,
                     dx0p ? (int)dx0_lo : 0, (int)M, (int)G, (int)serial);
  C10_HIP_KERNEL_LAUNCH_CHECK();
  return {dys, dx0};
}

// ---------------------------------------------------------------------------
// arena = mlp_chain_bwd_dwdb_f32(dys_and_dy, acts, G, S)
// dys_and_dy = [dy_0 .. dy_{L-2}, dy], dy_l [G, M, N_l]; acts as above.
// arena [S, total]: slice s holds the partial sums over batch rows
// [s chunk, (s + 1) chunk), chunk = ceil(M / S) rounded up to 4 (a slice
// past M holds zeros), laid out as
//     dW_0 [G, N_0, K_0] .. dW_{L-1} [G, N_{L-1}, K_{L-1}],
//     db_0 [G, N_0] .. db_{L-1} [G, N_{L-1}]
// reduce_arena(arena, flat, S) folds it.
// ---------------------------------------------------------------------------
static torch::Tensor mlp_chain_bwd_dwdb_f32(
    std::vector<torch::Tensor> dys, std::vector<torch::Tensor> acts, long G,
    long S) {
  const int L = (int)dys.size();
  TORCH_CHECK(L >= 1 && L <= FLAYERS, "f32 chain bwd: 1 <= L <= ", FLAYERS);
  TORCH_CHECK(G >= 1 && S >= 1 && S <= 65535,
              "f32 chain bwd: G >= 1 and 1 <= S <= 65535");
  long N[FLAYERS], K[FLAYERS];
  for (int l = 0; l < L; ++l) {
    F32B_CHECK(dys[l]);
    TORCH_CHECK(dys[l].device() == dys[0].device(), "f32 chain bwd: dys[",
                l, "] is on another device");
    TORCH_CHECK(dys[l].dim() == 3 || (G == 1 && dys[l].dim() == 2),
                "f32 chain bwd: dys[", l, "] must be [G, M, N]");
    N[l] = dys[l].size(-1);
  }
  const long M = dys[0].size(-2);
  check_chain(acts, G, M, dys[0].device(), L, N, K);
  F32DwDesc d{};
  d.L = L;
  long total = 0, jobs = 0;
  for (int l = 0; l < L; ++l) {
    TORCH_CHECK(dys[l].numel() == G * M * N[l], "f32 chain bwd: dys[", l,
                "] needs ", G * M * N[l], " elements");
    d.dy[l] = dys[l].data_ptr<float>();
    d.a[l] = acts[l].data_ptr<float>();
    d.ags[l] = acts[l].numel() == G * M * K[l] ? M * K[l] : 0;
    d.N[l] = (int)N[l];
    d.K[l] = (int)K[l];
    d.woff[l] = total;
    total += G * N[l] * K[l];
    jobs += G * ((N[l] + DWT - 1) / DWT) * ((K[l] + DWT - 1) / DWT);
    TORCH_CHECK(jobs < (1L << 31), "f32 chain bwd: too many tile jobs");
    d.jend[l] = (int)jobs;
  }
  for (int l = 0; l < L; ++l) {
    d.boff[l] = total;
    total += G * N[l];
  }
  const long chunk = ((M + S - 1) / S + 3) & ~3L;
  auto arena = torch::empty({S, total}, dys[0].options());
  hipLaunchKernelGGL(k_f32_chain_dwdb, dim3((unsigned)jobs, (unsigned)S),
                     dim3(64), 0, cur_stream5(), d,
                     arena.data_ptr<float>(), total, (int)M, (int)chunk);
  C10_HIP_KERNEL_LAUNCH_CHECK();
  return arena;
}

}  // namespace f32chainbwd

void register_f32_chain_bwd(pybind11::module_& m) {
  m.def("mlp_chain_bwd_dx_f32", &f32chainbwd::mlp_chain_bwd_dx_f32,
        "whole-chain fp32 MFMA MLP backward: the dx walk",
        pybind11::arg("dy"), pybind11::arg("ws"), pybind11::arg("acts"),
        pybind11::arg("G"), pybind11::arg("dx0_lo"));
  m.def("mlp_chain_bwd_dwdb_f32", &f32chainbwd::mlp_chain_bwd_dwdb_f32,
        "whole-chain fp32 MFMA MLP backward: grouped split-K dW/db partials",
        pybind11::arg("dys_and_dy"), pybind11::arg("acts"),
        pybind11::arg("G"), pybind11::arg("S"));
}
