// pcgrad.hip — PCGrad gradient surgery (Yu et al., 2020) in coefficient
// space, on the per-task split-K arena of the manual bf16 update
// (docs/KERNELS.md "PCGrad"; the oracle is torch_ref.pcgrad_*).
//
// With S = T splits of B / T rows, arena row t is the gradient g_t of task
// t's share of the loss.  Every projected gradient of PCGrad is a linear
// combination of the g_t, so all of its decisions need only the T x T Gram
// matrix G = g g^T, and its result sum_i g_i^PC is sum_t w_t * arena[t].
//
// k_pcgrad_gram_solve — G, then w, in one launch:
//   Gram.  One 16x16 fp32 accumulator tile per wave, tasks are the 16 rows
//   (rows >= T are zero and never loaded).  v_mfma_f32_16x16x4_f32 computes
//   D += A B with lane (i = lane & 15, k = lane >> 4) holding A[i][k] and
//   B[k][i]; passing ONE register for both gives G += A A^T, so every arena
//   element is read from HBM once and used as both operands.  A lane loads a
//   float4 at column p + 4 k of row i: one wave load reads 16 floats = 64
//   contiguous bytes of each task row, and element e of the float4 feeds
//   MFMA e (column p + 4 k + e at k-slot k, the same slot for both
//   operands).  Waves stride over the 16-column steps, eight loads in flight
//   and four independent accumulators per wave (blocks of 8 waves).  The
//   unaligned head and tail of [lo, lo + n), and everything when the rows
//   are not 16-byte aligned, take scalar loads guarded per element, 4
//   columns per MFMA.
//   Reduction.  The four accumulators are added in index order, the block's
//   eight wave tiles go through LDS and are added in wave order to one
//   [256] partial in ws[1 + block * 256 ...]; the last block to take the
//   self-resetting ticket ws[0] adds the partials in block order.  No float
//   atomics; the grid depends on n alone, so a result repeats bit for bit.
//   Solve.  In that last block, wave 0: lane i owns a_i = e_i (LDS).  For j
//   in task i's visiting order: d = sum_k a_i[k] G[k][j] (fma chain, k
//   ascending); if d < 0 and G[j][j] > 0, a_i[j] -= d / G[j][j].  Then
//   w[t] = sum_i a_i[t], i ascending.
//   Visiting order of task i: the j != i sorted by
//   dsac_sm64(c * 0x100000001 + 2^63 + 256 + 256 group + 16 i + j), ties by
//   j.  With o the offset added to c * 0x100000001 + 2^63, the inputs of
//   k_replay_sample_norepl have o = t < 32 and these have 256 <= o < 768;
//   (c, o) -> c * 0x100000001 + o is one-to-one for o < 2^32 + 1, and for
//   counters below 2^31 - 2 nothing wraps, so no input here is an input
//   there.  The replay, prioritized and squash streams hash inputs below
//   2^63 (see dsac_norepl_index), these are at or above it.
//
// k_pcgrad_fold — flat_grad[lo + i] = sum_t w[t] * arena[t][lo + i], an fma
// chain from 0.f in t order: k_reduce_arena with weights, float4 loads and
// stores where the rows are 16-byte aligned.
//
// out (fp32, PC_OUT words): w[16] | visited, projected, mean off-diagonal
// cosine, projected / visited | G[16][16] | order[16][16] (as floats, -1 =
// unused).

#include <hip/hip_runtime.h>
#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>
#include <c10/hip/HIPStream.h>

#include <algorithm>

// Packed fp32 ops are kept out of these kernels (see tqc.hip).
#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute push(                                             \
    __attribute__((target("no-packed-fp32-ops"))), apply_to = function)
#endif

namespace pcgrad {

typedef float f32x4 __attribute__((ext_vector_type(4)));

static constexpr int MAXT = 16;
static constexpr int NTHR = 512, NWAVE = NTHR / 64;
static constexpr int INFL = 8;                  // float4 loads in flight
static constexpr int MAXBLK = 128;              // partial slots in ws
static constexpr int WS_WORDS = 1 + MAXBLK * 256;
static constexpr int OUT_W = 0, OUT_M = 16, OUT_G = 20, OUT_ORD = 276;
static constexpr int PC_OUT = 532;
static constexpr int STEPS_PER_WAVE = 16;       // grid sizing target

__device__ __forceinline__ unsigned long long sm64(unsigned long long x) {
  x += 0x9E3779B97F4A7C15ull;                   // dsac_sm64
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}

__device__ __forceinline__ f32x4 mfma4(float a, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x4f32(a, a, c, 0, 0, 0);
}

// body: [body0, body0 + 16 nsteps), rows 16-byte aligned there; guarded:
// [lo, body0) and [body0 + 16 nsteps, hi)
__global__ __launch_bounds__(NTHR) void k_pcgrad_gram_solve(
    const float* __restrict__ arena, long stride, int T, long lo, long hi,
    long body0, long nsteps, const long long* __restrict__ rng, int group,
    float* ws, float* __restrict__ out) {
  __shared__ float tile[NWAVE][256];
  __shared__ float sG[MAXT][MAXT + 1];
  __shared__ float sa[MAXT][MAXT + 1];
  __shared__ float s_nrm[MAXT], s_cs[MAXT];
  __shared__ int sord[MAXT][MAXT];
  __shared__ int s_cnt[MAXT];
  __shared__ int s_last;
  const int tid = threadIdx.x, wid = tid >> 6, lane = tid & 63;
  const int i = lane & 15, k = lane >> 4;
  const bool row = i < T;
  const long nw = (long)gridDim.x * NWAVE;
  const long gw = (long)blockIdx.x * NWAVE + wid;
  const float* __restrict__ rp = arena + (long)(row ? i : 0) * stride;
  const f32x4 z4 = {0.f, 0.f, 0.f, 0.f};
  f32x4 acc0 = z4, acc1 = z4, acc2 = z4, acc3 = z4;

  // ---- Gram, aligned body: INFL steps of 16 columns in flight per wave
  for (long s = gw; s < nsteps; s += INFL * nw) {
    f32x4 v[INFL];
#pragma unroll
    for (int u = 0; u < INFL; ++u) {
      const long su = s + u * nw;
      v[u] = (row && su < nsteps)
                 ? *(const f32x4*)(rp + body0 + su * 16 + 4 * k) : z4;
    }
#pragma unroll
    for (int u = 0; u < INFL; ++u) {
      acc0 = mfma4(v[u][0], acc0);
      acc1 = mfma4(v[u][1], acc1);
      acc2 = mfma4(v[u][2], acc2);
      acc3 = mfma4(v[u][3], acc3);
    }
  }
  // ---- guarded head and tail: 4 columns per step, one per k-slot
#pragma unroll
  for (int r = 0; r < 2; ++r) {
    const long g0 = r == 0 ? lo : body0 + nsteps * 16;
    const long g1 = r == 0 ? body0 : hi;
    for (long q = g0 + 4 * gw; q < g1; q += 4 * nw) {
      const long col = q + k;
      const float v = (row && col < g1) ? rp[col] : 0.f;
      acc0 = mfma4(v, acc0);
    }
  }
  // ---- block partial: accumulators in index order, waves in wave order.
  // lane holds G[4 k + r][i], r = 0..3
  const f32x4 acc = (acc0 + acc1) + (acc2 + acc3);
#pragma unroll
  for (int r = 0; r < 4; ++r) tile[wid][(4 * k + r) * 16 + i] = acc[r];
  __syncthreads();
  float* slots = ws + 1;
  if (tid < 256) {
    float p = tile[0][tid];
#pragma unroll
    for (int wv = 1; wv < NWAVE; ++wv) p += tile[wv][tid];
    slots[(long)blockIdx.x * 256 + tid] = p;
    __threadfence();
  }
  __syncthreads();
  if (tid == 0) {
    const unsigned old = atomicAdd((unsigned*)ws, 1u);
    s_last = (old == (unsigned)gridDim.x - 1u);
    if (s_last) {
      *(unsigned*)ws = 0u;  // reset the ticket for the next replay
      __threadfence();
    }
  }
  __syncthreads();
  if (!s_last) return;
  // ---- last block: partials in block order.  The fence orders the plain
  // loads below after the ticket (every writer fenced before taking it)
  __threadfence();
  if (tid < 256) {
    float g = 0.f;
    const int nb = (int)gridDim.x;
    // 32 independent loads in flight, added in block order (a slot past
    // the grid adds 0.f)
    for (int b = 0; b < nb; b += 32) {
      float v[32];
#pragma unroll
      for (int u = 0; u < 32; ++u)
        v[u] = b + u < nb ? slots[(long)(b + u) * 256 + tid] : 0.f;
#pragma unroll
      for (int u = 0; u < 32; ++u) g += v[u];
    }
    sG[tid >> 4][tid & 15] = g;
    out[OUT_G + tid] = g;
  }
  __syncthreads();
  if (wid != 0) return;
  // ---- solve, one wave: lane i < T owns a_i
  if (lane < T) {
    const int me = lane;
    const unsigned long long base =
        (unsigned long long)rng[0] * 0x100000001ull + 0x8000000000000000ull
        + 256ull + 256ull * (unsigned long long)group
        + 16ull * (unsigned long long)me;
    unsigned long long key[MAXT];
#pragma unroll
    for (int j = 0; j < MAXT; ++j) key[j] = sm64(base + (unsigned long long)j);
    // rank of j among the j != me: keys ascending, ties by j
#pragma unroll
    for (int j = 0; j < MAXT; ++j) {
      if (j >= T || j == me) continue;
      int rank = 0;
#pragma unroll
      for (int q = 0; q < MAXT; ++q) {
        if (q >= T || q == me || q == j) continue;
        rank += (key[q] < key[j] || (key[q] == key[j] && q < j)) ? 1 : 0;
      }
      sord[me][rank] = j;
    }
    for (int t = 0; t < T; ++t) sa[me][t] = t == me ? 1.f : 0.f;
    int proj = 0;
    for (int s = 0; s < T - 1; ++s) {
      const int j = sord[me][s];
      float d = 0.f;
      for (int t = 0; t < T; ++t) d = __fmaf_rn(sa[me][t], sG[t][j], d);
      const float gjj = sG[j][j];
      if (d < 0.f && gjj > 0.f) {
        sa[me][j] = __fsub_rn(sa[me][j], __fdiv_rn(d, gjj));
        ++proj;
      }
      out[OUT_ORD + me * 16 + s] = (float)j;
    }
    s_cnt[me] = proj;
  }
  if (lane < MAXT)
    for (int s = lane < T ? T - 1 : 0; s < MAXT; ++s)
      out[OUT_ORD + lane * 16 + s] = -1.f;
  // one wave in lockstep (the other waves have left): the fences keep the
  // LDS writes above ahead of the reads below
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
  if (lane < MAXT) {
    float w = 0.f;
    if (lane < T)
      for (int t = 0; t < T; ++t) w += sa[t][lane];
    out[OUT_W + lane] = w;
    s_nrm[lane] = lane < T ? sqrtf(sG[lane][lane]) : 0.f;
  }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
  if (lane < T) {     // row sums of the off-diagonal cosines, b ascending
    float cs = 0.f;
    for (int b = 0; b < T; ++b) {
      const float den = s_nrm[lane] * s_nrm[b];
      if (b != lane && den > 0.f) cs += sG[lane][b] / den;
    }
    s_cs[lane] = cs;
  }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
  if (lane == 0) {
    int proj = 0;
    float cs = 0.f;
    for (int a = 0; a < T; ++a) {
      proj += s_cnt[a];
      cs += s_cs[a];
    }
    const float visited = (float)(T * (T - 1));
    out[OUT_M + 0] = visited;
    out[OUT_M + 1] = (float)proj;
    out[OUT_M + 2] = cs / visited;
    out[OUT_M + 3] = (float)proj / visited;
  }
}

// thread q owns columns [4 q', 4 q' + 4) of the range rounded down to a
// multiple of 4; a group fully inside [lo, hi) with aligned rows moves as
// float4, any other element by element
__global__ __launch_bounds__(256) void k_pcgrad_fold(
    const float* __restrict__ arena, long stride, int T,
    const float* __restrict__ w, float* __restrict__ flat, long lo, long hi,
    int vec) {
  __shared__ float sw[MAXT];
  const int tx = threadIdx.x;
  if (tx < MAXT) sw[tx] = tx < T ? w[tx] : 0.f;
  __syncthreads();
  const long c0 = (lo & ~3l) + 4 * ((long)blockIdx.x * 256 + tx);
  if (c0 >= hi) return;
  if (vec && c0 >= lo && c0 + 4 <= hi) {
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    for (int t = 0; t < T; ++t) {
      const f32x4 a = *(const f32x4*)(arena + (long)t * stride + c0);
      const float wt = sw[t];
#pragma unroll
      for (int e = 0; e < 4; ++e) acc[e] = __fmaf_rn(wt, a[e], acc[e]);
    }
    *(f32x4*)(flat + c0) = acc;
    return;
  }
  for (long c = c0 > lo ? c0 : lo; c < c0 + 4 && c < hi; ++c) {
    float acc = 0.f;
    for (int t = 0; t < T; ++t)
      acc = __fmaf_rn(sw[t], arena[(long)t * stride + c], acc);
    flat[c] = acc;
  }
}

}  // namespace pcgrad

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif

static inline hipStream_t pcgrad_stream() {
  return c10::hip::getCurrentHIPStream().stream();
}

static void pcgrad_check_arena(const torch::Tensor& arena, long T, long lo,
                               long n) {
  TORCH_CHECK(arena.is_cuda() && arena.scalar_type() == torch::kFloat32
              && arena.dim() == 2 && arena.is_contiguous(),
              "pcgrad: arena is a contiguous [T, P] fp32 HIP tensor");
  TORCH_CHECK(T >= 2 && T <= pcgrad::MAXT && arena.size(0) >= T,
              "pcgrad: 2 <= T <= 16 arena rows, got T = ", T);
  TORCH_CHECK(lo >= 0 && n >= 1 && lo + n <= arena.size(1),
              "pcgrad: the range [lo, lo + n) lies inside the arena row");
}

// Gram matrix of arena rows 0..T-1 over columns [lo, lo + n), then the
// PCGrad weights.  rng: the int64 device counter; group: the salt of the
// visiting orders; ws: 1 + 128 * 256 floats, ticket zero on entry; out: 532
// floats (layout above).
static void pcgrad_gram_solve(torch::Tensor arena, long T, long lo, long n,
                              torch::Tensor rng, long group,
                              torch::Tensor ws, torch::Tensor out) {
  pcgrad_check_arena(arena, T, lo, n);
  TORCH_CHECK(rng.is_cuda() && rng.scalar_type() == torch::kInt64
              && rng.numel() >= 1, "pcgrad: rng is the int64 device counter");
  TORCH_CHECK(group >= 0 && group <= 1, "pcgrad: group salt is 0 or 1");
  for (const torch::Tensor* t : {&ws, &out})
    TORCH_CHECK(t->is_cuda() && t->scalar_type() == torch::kFloat32
                && t->is_contiguous(), "pcgrad: ws/out fp32 HIP, contiguous");
  TORCH_CHECK(ws.numel() >= pcgrad::WS_WORDS, "pcgrad: workspace too small");
  TORCH_CHECK(out.numel() >= pcgrad::PC_OUT, "pcgrad: out too small");
  const long stride = arena.size(1), hi = lo + n;
  const bool vec = stride % 4 == 0
      && reinterpret_cast<uintptr_t>(arena.data_ptr<float>()) % 16 == 0;
  const long body0 = vec ? std::min((lo + 3) / 4 * 4, hi) : lo;
  const long nsteps = vec ? (hi - body0) / 16 : 0;
  const long gsteps = (body0 - lo + 3) / 4 + (hi - body0 - nsteps * 16 + 3) / 4;
  const long per_blk = pcgrad::NWAVE * pcgrad::STEPS_PER_WAVE;
  long nblk = (std::max(nsteps, gsteps) + per_blk - 1) / per_blk;
  nblk = std::min<long>(std::max<long>(nblk, 1), pcgrad::MAXBLK);
  hipLaunchKernelGGL(pcgrad::k_pcgrad_gram_solve, dim3(nblk),
                     dim3(pcgrad::NTHR), 0,
                     pcgrad_stream(), arena.data_ptr<float>(), stride, (int)T,
                     lo, hi, body0, nsteps,
                     (const long long*)rng.data_ptr<int64_t>(), (int)group,
                     ws.data_ptr<float>(), out.data_ptr<float>());
}

// flat[lo + i] = sum_t w[t] * arena[t][lo + i], i < n (t order)
static void pcgrad_fold(torch::Tensor arena, torch::Tensor w,
                        torch::Tensor flat, long T, long lo, long n) {
  pcgrad_check_arena(arena, T, lo, n);
  TORCH_CHECK(w.is_cuda() && w.scalar_type() == torch::kFloat32
              && w.is_contiguous() && w.numel() >= T, "pcgrad: w [>= T] fp32");
  TORCH_CHECK(flat.is_cuda() && flat.scalar_type() == torch::kFloat32
              && flat.is_contiguous() && flat.numel() <= arena.size(1)
              && lo + n <= flat.numel(),
              "pcgrad: flat is the group's fp32 gradient, [lo, lo + n) inside");
  const long stride = arena.size(1), hi = lo + n;
  const bool vec = stride % 4 == 0
      && reinterpret_cast<uintptr_t>(arena.data_ptr<float>()) % 16 == 0
      && reinterpret_cast<uintptr_t>(flat.data_ptr<float>()) % 16 == 0;
  const long ngrp = (hi - (lo & ~3l) + 3) / 4;
  hipLaunchKernelGGL(pcgrad::k_pcgrad_fold, dim3((ngrp + 255) / 256),
                     dim3(256), 0, pcgrad_stream(), arena.data_ptr<float>(),
                     stride, (int)T, w.data_ptr<float>(),
                     flat.data_ptr<float>(), lo, hi, (int)vec);
}

void register_pcgrad(pybind11::module_& m) {
  m.def("pcgrad_gram_solve", &pcgrad_gram_solve,
        "Gram matrix of the per-task arena rows + PCGrad weights, one launch");
  m.def("pcgrad_fold", &pcgrad_fold,
        "flat gradient = weighted fold of the per-task arena rows");
}
