// tx_ring_variants.hip — the transmit-ring kernel (tx_ring.hip) with either
// store policy, and the stores alone, for tools/tx_ring_probe.py.
// txrv_launch(geo, stream, k):
//   0 the field stores at the default cache policy
//   1 the field stores nt sc1 (tcp_tx's header-pass policy)
//   2 the stores alone (txr_store_floor): one thread per slot reads the two
//     fields of an IPv4/TCP frame without options (+10, +36) and stores them
//     back, nothing else: what the scattered 2-byte stores cost without the
//     frames' line loads in flight (timing only)
//   3 the same with the transport field only (as NS_TXR_L4_ONLY)
// 0 and 1 compute the product's bytes, status and sums.  Not part of the ABI.
#include "../netstack_amd/csrc/tx_ring.hip"

namespace nsk {

template <int BOTH>
__global__ __launch_bounds__(256) void txr_store_floor(TxRingGeo g) {
  const uint64_t s = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (s >= g.n || g.frame_at + g.link + 38u > g.stride) return;
  // 2-byte aligned: ring and stride are multiples of 16, frame_at + link is even
  uint16_t* ip = reinterpret_cast<uint16_t*>(g.ring + s * g.stride + g.frame_at + g.link);
  uint32_t a = BOTH ? ip[5] : 0u, b = ip[18];
  asm volatile("" : "+v"(a), "+v"(b));  // opaque: the stores below are not folded away
  if (BOTH) ip[5] = (uint16_t)a;
  ip[18] = (uint16_t)b;
}

}  // namespace nsk

extern "C" int txrv_launch(const nsk::TxRingGeo* g, void* stream, int k) {
  if (g->n == 0) return 0;
  hipStream_t s = (hipStream_t)stream;
  if (k == 2 || k == 3) {
    const dim3 grid((g->n + 255u) / 256u), block(256);
    if (k == 2) hipLaunchKernelGGL(nsk::txr_store_floor<1>, grid, block, 0, s, *g);
    else hipLaunchKernelGGL(nsk::txr_store_floor<0>, grid, block, 0, s, *g);
    return (int)hipGetLastError();
  }
  return (int)(k == 1 ? nsk::launch_tx_ring_p<18>(*g, s) : nsk::launch_tx_ring_p<0>(*g, s));
}
