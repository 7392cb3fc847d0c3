// What the register-resident attention forwards share (transformer.hip: bf16 operands; attn_mx.hip: block-scaled
// e4m3 operands): the head dim, the padded LDS row of a [keys][head dim] tile and the transposed, key-permuted
// fragment read of V.
#pragma once
#include "common.h"

namespace pcmp {

constexpr int AD = 64;       // head dim
constexpr int ADP = AD + 8;  // padded LDS row (bf16 elements) for [*][d] tiles

// bf16 fragment of X^T for an LDS tile stored row-major X[k][m] over the permuted reduction order of the
// forwards' P^T operand: M index mbase + (lane & 15), slots i < 4 -> k = kbase + 4g + i, slots i >= 4 ->
// k = kbase + 16 + 4g + i - 4 (g = lane >> 4), read with two ds_read_b64_tr_b16.
__device__ __forceinline__ bf16x8 frag_tr_perm(const __bf16* X, int ld, int kbase, int mbase) {
  typedef short s16x4 __attribute__((ext_vector_type(4)));
  typedef __attribute__((address_space(3))) s16x4 lds_s16x4_t;
  const int lane = threadIdx.x & 63;
  const int row = kbase + 4 * (lane >> 4) + ((lane >> 2) & 3), col = mbase + (lane & 3) * 4;
  const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4_t*)(X + row * ld + col));
  const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4_t*)(X + (row + 16) * ld + col));
  return __builtin_bit_cast(bf16x8, __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7));
}

}  // namespace pcmp
