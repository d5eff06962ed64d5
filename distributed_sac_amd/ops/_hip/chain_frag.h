// chain_frag.h — what the MLP-chain kernel files share: the LDS tile
// geometry, the bf16 conversion and the k-loop over fragment-packed weights
// (k_bf16_pack_frag's layout).  Used by chain_gemm.hip and ln_chain.hip.
#pragma once

#include <hip/hip_runtime.h>

namespace chain {

using f32x4 = __attribute__((__vector_size__(4 * sizeof(float)))) float;
using bf16x8 = __attribute__((ext_vector_type(8))) __bf16;
using u16 = unsigned short;

static constexpr int CMAX = 768;  // max layer width / input width
                                  // (768 = the RoBERTa context width)
static constexpr int CPAD = 776;  // LDS row stride (u16): 388 dwords ≡ 4 mod 64
                                  // -> 16-lane b128 A-fragment groups hit
                                  // all 64 banks exactly once
static constexpr int NTHR = 512;  // 8 waves: the parent mapping's block

__device__ __forceinline__ u16 f32_to_bf16_rne3(float f) {
  // native v_cvt_pk_bf16_f32: round to nearest even, and a NaN stays a
  // NaN (the integer rounding add carried some into Inf or zero)
  return __builtin_bit_cast(u16, (__bf16)f);
}

// k-loop of the FRAGMENT-PACKED path, shared by the forward and the dx
// body: a rotating software pipeline over DEPTH + 1 fragment sets of TQ
// tiles.  The loads of k-step ks + DEPTH are issued before the MFMAs of
// k-step ks, so DEPTH * TQ 1-KiB loads are in flight per wave.  bp[j] is
// the lane's element offset of tile j's k-step 0; one k-step is 512 u16.
// Correct for every KS >= 1, shorter than DEPTH included: no load reaches
// past step KS - 1, and mf(set, k) runs once per step in ascending order,
// so each accumulator sums exactly as with any other DEPTH.
//
// DEPTH == 2 is the 8-wave quad kernels' ladder, kept as it was: its
// look-ahead loads sit under (uniform) branches, and the compiler's
// wait-count merge over those branches drains all loads at the loop head,
// once per three k-steps.  Every other DEPTH runs branch-free: a
// look-ahead past the last step re-reads step KS - 1 (a cache hit nobody
// consumes, DEPTH - KS % (DEPTH + 1) of them per pass) so the waits inside
// the loop leave DEPTH * TQ loads outstanding.  The pair launch, two
// workgroups per CU, measured 0.8 us slower with those extra loads and
// stays on the ladder.
template <int TQ, int DEPTH, class MF>
__device__ __forceinline__ void packed_kloop(const u16* __restrict__ wpl,
                                             const long (&bp)[TQ], int KS,
                                             MF mf) {
  constexpr int NS = DEPTH + 1;
  bf16x8 S[NS][TQ];
#define LOADP(set, ks_)                                                   \
  _Pragma("unroll") for (int j = 0; j < TQ; ++j)                          \
    S[set][j] = *(const bf16x8*)&wpl[bp[j] + (long)(ks_) * 512];
  if constexpr (DEPTH == 2) {
    LOADP(0, 0)
    if (1 < KS) LOADP(1, 1)
    int ks = 0;
    while (ks + 3 <= KS) {
      LOADP(2, ks + 2)
      mf(S[0], ks * 32);
      if (ks + 3 < KS) {
        LOADP(0, ks + 3)
      }
      mf(S[1], (ks + 1) * 32);
      if (ks + 4 < KS) {
        LOADP(1, ks + 4)
      }
      mf(S[2], (ks + 2) * 32);
      ks += 3;
    }
    if (KS - ks == 1) {
      mf(S[0], ks * 32);
    } else if (KS - ks == 2) {
      mf(S[0], ks * 32);
      mf(S[1], (ks + 1) * 32);
    }
  } else {
    const int last = KS - 1;
#define LOADC(set, ks_) LOADP(set, (ks_) < last ? (ks_) : last)
#pragma unroll
    for (int s = 0; s < DEPTH; ++s) LOADC(s, s)
    int ks = 0;
    for (; ks + NS <= KS; ks += NS) {
#pragma unroll
      for (int s = 0; s < NS; ++s) {
        // refill the set the previous step consumed
        LOADC((s + DEPTH) % NS, ks + s + DEPTH)
        mf(S[s], (ks + s) * 32);
      }
    }
    // the last KS % NS steps sit in sets 0 .. KS % NS - 1
#pragma unroll
    for (int s = 0; s < DEPTH; ++s)
      if (ks + s < KS) mf(S[s], (ks + s) * 32);
#undef LOADC
  }
#undef LOADP
}

}  // namespace chain
