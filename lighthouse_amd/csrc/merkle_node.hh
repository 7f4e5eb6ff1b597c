// A merkle node in device memory is 32 bytes, i.e. 8 big-endian words for
// the hasher; in registers and LDS it is kept as 8 host-order words
// (sha256_node's form). The pointer is 4-byte aligned.
#pragma once
#include "sha256.hh"

namespace m3x {

__device__ __forceinline__ void load_node(const uint8_t *p, uint32_t w[8]) {
  const uint32_t *src = reinterpret_cast<const uint32_t *>(p);
#pragma unroll
  for (int i = 0; i < 8; i++) w[i] = __builtin_bswap32(src[i]);
}

__device__ __forceinline__ void store_node(uint8_t *p, const uint32_t w[8]) {
  uint32_t *dst = reinterpret_cast<uint32_t *>(p);
#pragma unroll
  for (int i = 0; i < 8; i++) dst[i] = __builtin_bswap32(w[i]);
}

} // namespace m3x
