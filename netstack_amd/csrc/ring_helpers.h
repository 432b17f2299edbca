// The small inline helpers the ring kernels share (rx_ring.hip, tx_ring.hip):
// the W-sum arithmetic of a range that starts at an even address, the masked
// sum over a packet's LDS row, and the buffer resource and 16-B load of a
// wave's slots.  See rx_ring.hip's opening comment for the arithmetic.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace nsk {
namespace {

__device__ __forceinline__ uint32_t rx_fold(uint32_t v) {  // ChecksumCombine, checksum.go:104-107
  const uint32_t s = (v & 0xFFFFu) + (v >> 16);
  return (s + (s >> 16)) & 0xFFFFu;
}

// A W total of a range starting at an even address, as a value with the fold
// behaviour of Go's S (the byte swap of W, mod 65535; zero iff W is).
__device__ __forceinline__ uint32_t rx_class(uint32_t W) { return rx_fold(rx_fold(W) << 8); }

__device__ __forceinline__ uint32_t rx_wsum4(const uint4 v) {
  uint32_t acc = __builtin_amdgcn_sad_u16(v.x, 0u, 0u);
  acc = __builtin_amdgcn_sad_u16(v.y, 0u, acc);
  acc = __builtin_amdgcn_sad_u16(v.z, 0u, acc);
  return __builtin_amdgcn_sad_u16(v.w, 0u, acc);
}

__device__ __forceinline__ uint32_t rx_below(int c) {  // bytes [0, c) of a dword, c clamped to [0, 4]
  c = c < 0 ? 0 : (c > 4 ? 4 : c);
  return c >= 4 ? 0xFFFFFFFFu : ((1u << (8 * c)) - 1u);
}

// The W sum of row bytes [x, y) of a packet's LDS row (x even; y may be
// odd): dwords with halfword masks, the odd last byte on its own.  Every
// range the receive path sums from the row starts at an even offset, so a
// boundary never splits a halfword except at an odd end.
template <int MAXD>
__device__ __forceinline__ uint32_t rx_row_wsum(const uint8_t* row, uint32_t x, uint32_t y) {
  const uint32_t* D = reinterpret_cast<const uint32_t*>(row);
  const uint32_t ye = y & ~1u;
  const uint32_t len = ye > x ? ye - x : 0u;
  const uint32_t d0 = x >> 2;
  const uint32_t nd = len ? ((ye + 3) >> 2) - d0 : 0u;
  uint32_t w = 0;
  // a wave-uniform trip count (the longest lane's), the lanes past their own
  // end masked: no divergent branch per dword
  for (uint32_t k = 0; k < MAXD && __builtin_amdgcn_ballot_w64(k < nd) != 0; ++k) {
    const uint32_t o = 4u * (d0 + k);
    const uint32_t m = ((o - x) < len ? 0x0000FFFFu : 0u) | ((o + 2u - x) < len ? 0xFFFF0000u : 0u);
    w = __builtin_amdgcn_sad_u16(D[k < nd ? d0 + k : 0u] & m, 0u, w);
  }
  if ((y & 1u) && y > x) w += row[y - 1];  // a lone byte at an even offset: the low byte of its word
  return w;
}

__device__ __forceinline__ __amdgpu_buffer_rsrc_t rx_srd(uint64_t base, uint32_t nrec) {
  const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((uint32_t)base);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_readfirstlane((uint32_t)(base >> 32));
  return __builtin_amdgcn_make_buffer_rsrc((void*)(((uint64_t)hi << 32) | (uint64_t)lo), (short)0,
                                           (int)__builtin_amdgcn_readfirstlane(nrec), 0x00020000);
}

template <int AUX>
__device__ __forceinline__ uint4 rx_load(__amdgpu_buffer_rsrc_t r, uint32_t off) {
  auto x = __builtin_amdgcn_raw_buffer_load_b128(r, (int)off, 0, AUX);
  return *reinterpret_cast<uint4*>(&x);
}

}  // namespace
}  // namespace nsk
