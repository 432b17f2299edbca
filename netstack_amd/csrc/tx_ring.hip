// tx_ring.hip — the checksum fields of a fixed-stride ring of outgoing frames,
// filled on the device (ns_csum_tx_ring, include/netstack_csum.h; DESIGN.md
// §4.10).  The transmit mirror of rx_ring.hip: no descriptor table and no host
// planning; the kernel reads each slot's length, parses the frame's headers
// itself and writes the fields a link that advertises
// CapabilityTXChecksumOffload owes the wire (TCP and UDP leave theirs zero
// then: transport/tcp/connect.go:661, transport/udp/endpoint.go:809).
//
// What one slot goes through:
//   gate     exactly rx_ring's malformed rules with the frame as one view
//            (oracle/packets.py verify_frame, first_view = 0): a malformed
//            slot is left byte for byte as it was.
//   IPv4     the field at +10 = ^Checksum(ip[:IHL*4]) with the field read as
//            zero (network/ipv4/ipv4.go:236; fragments :159-160).
//   TCP      +16 (transport/tcp/connect.go:653-663); UDP +6, the datagram as
//            one view, a sum of 0xffff writing 0x0000 (transport/udp/
//            endpoint.go:808-815); ICMPv4 of any type +2 (network/ipv4/
//            icmp.go:99-100); ICMPv6 +2 (header/icmpv6.go:202-221).  The
//            transport range is [IHL*4, TotalLength) / [40, 40 +
//            PayloadLength): frame bytes past it (Ethernet padding) are never
//            summed.
//
// Shape: rx_ring's (8-lane groups, one per slot; every line load issued from
// the length alone; lines 0-1 to a 96-B LDS row; a select-based parse; W-only
// accumulation and a 3-step DPP reduction).  Three things differ:
//   - UDP and every ICMPv4 type are summed kinds;
//   - a field is read as zero by SUBTRACTING its halfword, read from the LDS
//     row, from W: W is an exact integer sum of little-endian halfwords and
//     every field sits at an even address, so no chunk needs a mask.  The
//     deepest field is IPv4 IHL 15 + TCP's at 60 + 16 = 76 < 96 - 14;
//   - lane 0 of the group stores the two 2-byte fields.
//
// Slots share 128-B lines (at stride 80 one line holds parts of three
// frames), so another group may be storing its fields into a line this group
// reads.  Two properties make that harmless and are to be kept:
//   1. every byte a group loads lies in its own slot: loads are gated per
//      16-B chunk to the chunks holding frame bytes (off_of / klast), and
//      16-B chunks never straddle 16-B-aligned slots;
//   2. a frame's stores issue after all of its own loads have returned, the
//      tail-chunk and padded-frame re-reads included: the values depend on
//      the group's reduction, and the stores sit behind a vmcnt(0) wait.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "csum_kernels.h"
#include "ring_helpers.h"

namespace nsk {
namespace {

constexpr uint32_t kTxrRowBytes = 96;  // LDS bytes per packet: [floor16(pa), +96)
constexpr uint32_t kTxrWaves = 4;      // waves per workgroup
constexpr uint32_t kTxrMaxIp = 65576;  // the longest IP packet any header can describe (40 + 65535), + 1

constexpr int kTxrStoreAux = 0;        // the field stores' cache policy (buffer aux): default

constexpr uint32_t kTxrNone = 0, kTxrL4 = 1, kTxrL3 = 2, kTxrMalformed = 3;  // NS_TXR_*

}  // namespace

// NB = lines per load batch (line 0 included); a packet longer than NB lines
// takes further batches of 4 lines.  SP = the stores' cache policy as a
// buffer aux (0 default; 18 = nt sc1, tcp_tx's header-pass policy).  Line 0
// is loaded with the default policy (its first bytes may belong to the slot
// before), the rest nontemporal.
template <int NB, int SP>
__global__ __launch_bounds__(64 * kTxrWaves) void tx_ring(TxRingGeo g) {
  constexpr uint32_t U = 128u, US = 7u, KR = 2u, PW = 8u;
  constexpr int A0 = 0, AN = 2;
  __shared__ uint4 tx_lds[kTxrWaves * PW * kTxrRowBytes / 16];
  const uint32_t lane = threadIdx.x & 63u, grp = lane >> 3, li = lane & 7u;
  const uint32_t wv = (uint32_t)__builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint64_t s0 = ((uint64_t)blockIdx.x * kTxrWaves + wv) * PW;  // the wave's first slot
  if (s0 >= g.n) return;  // a whole wave leaves together
  const uint64_t s = s0 + grp;
  const bool live = s < g.n;

  const uint32_t rlen = live ? g.len[s] : 0u;
  const uint32_t pre = g.frame_at + g.link;
  const uint64_t slot = g.ring + s * g.stride;
  // Wave-relative 32-bit coordinates: one buffer resource from the 128-B line
  // of the wave's first packet over its slots (< 8 strides + a line).  Loads
  // and stores past it read zeros and write nothing.
  const uint64_t wbase = (g.ring + s0 * g.stride + pre) & ~127ull;
  const uint64_t s_end = s0 + PW < g.n ? s0 + PW : g.n;
  const uint32_t nrec = (uint32_t)(g.ring + s_end * g.stride - wbase);
  const __amdgpu_buffer_rsrc_t rsrc = rx_srd(wbase, nrec);
  const uint32_t pa = (uint32_t)(slot + pre - wbase);  // the IP packet's first byte
  const uint32_t po = pa & 15u;                         // its offset in its 16-B chunk (even)
  const uint32_t cl = (pa & ~(U - 1u)) + 16u * li;      // lane li's chunk of line 0
  uint4 v[NB];
  const bool over = (uint64_t)rlen > g.stride;
  const uint32_t P = (!over && rlen > pre) ? rlen - pre : 0u;  // the IP packet's bytes in the frame
  const uint32_t Pl = P < kTxrMaxIp ? P : kTxrMaxIp;            // bytes any header can cover
  // chunk at o: loaded only where it holds packet bytes (all in this slot),
  // else the range check returns zeros without touching memory
  const uint32_t lim = Pl ? Pl + 15u : 0u;
  auto off_of = [&](uint32_t o) -> uint32_t { return (o + 15u - pa) < lim ? o : nrec; };
  const uint32_t pe = pa + Pl;
  const uint32_t klast = Pl && pe > cl ? (pe - 1u - cl) >> US : 0u;
  const bool any1 = Pl && pe > cl + U;  // some line k >= 1 holds packet bytes for this lane
  const uint32_t cl1 = any1 ? cl : nrec;

  v[0] = rx_load<A0>(rsrc, off_of(cl));
  auto line = [&](int k) { v[k] = rx_load<AN>(rsrc, ((uint32_t)k <= klast ? cl1 : nrec) + U * k); };
  line(1);
  // The EtherType (the link header's bytes 12-13, pa - 2): a buffer load on
  // a resource one line lower (pa - 2 may precede wbase).
  uint32_t etype = 0;
  if (g.link) {
    const __amdgpu_buffer_rsrc_t re = rx_srd(wbase - 128u, nrec + 128u);
    const uint32_t e = (uint32_t)__builtin_amdgcn_raw_buffer_load_b16(re, (int)(P ? pa + 126u : nrec + 128u), 0, 0);
    etype = ((e & 0xFFu) << 8) | ((e >> 8) & 0xFFu);
  }
#pragma unroll
  for (int k = 2; k < NB; ++k) line(k);
  uint32_t w2 = 0;  // every loaded chunk of lines >= 2
#pragma unroll
  for (int k = KR; k < NB; ++k) {
    w2 = __builtin_amdgcn_sad_u16(v[k].x, 0u, w2);
    w2 = __builtin_amdgcn_sad_u16(v[k].y, 0u, w2);
    w2 = __builtin_amdgcn_sad_u16(v[k].z, 0u, w2);
    w2 = __builtin_amdgcn_sad_u16(v[k].w, 0u, w2);
  }

  // The first 96 B from the packet's 16-B chunk into the group's LDS row.
  uint8_t* row = reinterpret_cast<uint8_t*>(tx_lds) + (wv * PW + grp) * kTxrRowBytes;
  const uint32_t f16 = pa & ~15u;
#pragma unroll
  for (int k = 0; k < (int)KR; ++k) {
    const uint32_t o = cl + U * k - f16;
    if (o < kTxrRowBytes) *reinterpret_cast<uint4*>(row + o) = v[k];
  }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");

  // Parse (every lane of the group, same LDS bytes), rx_ring's rules with the
  // frame as one view.  h(i) = IP byte i; selects, no divergent branches;
  // every byte read lies in the row, and a field only decides anything where
  // the rule that reads it has passed its length checks.
  auto h = [&](uint32_t i) -> uint32_t { return row[po + i]; };
  const uint32_t h0 = h(0), h2 = h(2), h3 = h(3), h4 = h(4), h5 = h(5), h6 = h(6), h7 = h(7), h9 = h(9);
  const uint32_t ver = h0 >> 4;
  const uint32_t np = g.link ? (etype == 0x0800u ? 4u : etype == 0x86DDu ? 6u : 0u) : ver;
  // IPv4 IsValid against the whole frame (header/ipv4.go:280-296)
  const uint32_t hlen = (h0 & 15u) * 4u, tlen = (h2 << 8) | h3;
  const bool v4 = np == 4 && P >= 20 && hlen >= 20 && hlen <= tlen && tlen <= P && ver == 4;
  const uint32_t foff = ((((h6 & 0x1Fu) << 8) | h7) << 3) & 0xFFFFu;
  const bool frag = v4 && ((h6 & 0x20u) || foff);
  const uint32_t fsize = (tlen - hlen) & 0xFFFFu;
  const bool fragbad = tlen == hlen || ((foff + fsize - 1u) & 0xFFFFu) < foff;  // ipv4.go:355-373
  // IPv6 IsValid (header/ipv6.go:207-222)
  const uint32_t plen = (h4 << 8) | h5;
  const bool v6 = np == 6 && P >= 40 && plen <= P - 40 && ver == 6;
  const bool ip = (v4 && !frag) || v6;
  const uint32_t proto = v4 ? h9 : h6;
  const uint32_t a = v4 ? hlen : 40u;  // the transport range [a, tend)
  const uint32_t tend = v4 ? tlen : 40u + plen;
  const uint32_t tsize = tend - a;
  const uint32_t toff = (h(a + 12) >> 4) * 4u;
  const bool tcp = ip && proto == 6, udp = ip && proto == 17, icmp4 = ip && v4 && proto == 1,
             icmp6 = ip && !v4 && proto == 58;
  const bool tcp_bad = tsize < 20 || toff < 20 || toff > tsize;
  // kind: 1 TCP, 2 ICMPv4 (any type), 3 ICMPv6, 4 UDP; fo = the field's offset in the transport header
  const uint32_t kind = tcp && !tcp_bad ? 1u : icmp4 && tsize >= 8 ? 2u : icmp6 && tsize >= 8 ? 3u
                        : udp && tsize >= 8 ? 4u : 0u;
  const uint32_t fo = kind == 1 ? 16u : kind == 4 ? 6u : 2u;
  const bool malformed = !P || (g.link ? np != 0 && !v4 && !v6 : !v4 && !v6) || (frag && fragbad) ||
                         (tcp && tcp_bad) || (udp && tsize < 8) || (icmp4 && tsize < 8) || (icmp6 && tsize < 8);
  const bool l3 = v4 && !malformed && !(g.flags & 1u);  // the IPv4 field is written
  const uint32_t b = kind ? tend : 0u;
  const uint32_t asz = v4 ? 8u : 32u;

  // The transport range splits at 16-B chunk boundaries (offsets r with
  // (r + po) % 16 == 0) into a head [a, min(b, A)) summed from the LDS row,
  // whole chunks [A, B) summed from the registers, and a tail [B, b) re-read
  // by one lane.
  const uint32_t A = ((a + po + 15u) & ~15u) - po, B = ((b + po) & ~15u) - po;
  const uint32_t span = kind && B > A ? B - A : 0u;
  // lanes 0, 1, 2: the IPv4 header, the pseudo-header's addresses, the head
  uint32_t x = 0, y = 0;
  if (li == 0 && v4) {
    x = po;
    y = po + hlen;
  } else if (li == 1 && kind) {
    x = po + (asz == 8 ? 12u : 8u);
    y = x + asz;
  } else if (li == 2 && kind) {
    x = po + a;
    y = po + (b < A ? b : A);
  }
  // The last loaded chunk (its offset from pa) and the first of line 2.
  const uint32_t rl = Pl ? ((pa + Pl - 1u) & ~15u) - pa : 0u;
  const uint32_t r2 = (pa & ~(U - 1u)) + KR * U - pa;
  // A frame padded past its transport's end with loaded chunks beyond the
  // transport's last chunk in lines >= 2 (their bytes are in w2): the whole
  // wave sums lines >= 2 again with the range check.
  const bool slow = kind && rl >= r2 && (rl > B || (rl == B && b == B));
  const bool wslow = __builtin_amdgcn_ballot_w64(slow) != 0;
  uint32_t tail = 0;
  if (li == 3 && kind && b > B && B >= A) {  // bytes [B, b): one 16-B chunk of this slot, an L2 hit
    const uint4 t = rx_load<0>(rsrc, pa + B);
    const int c = (int)(b - B);
    tail = rx_wsum4(make_uint4(t.x & rx_below(c), t.y & rx_below(c - 4), t.z & rx_below(c - 8),
                               t.w & rx_below(c - 12)));
    // in line >= 2 this chunk is in w2 whole; take its bytes past b back out
    if (B >= r2 && !wslow) tail -= rx_wsum4(t);
  }
  uint32_t rs = rx_row_wsum<16>(row, x, y);
  // The fields as they stand (halfwords at even addresses, inside the row):
  // W counts each once; reading them as zero is taking them back out.
  const uint32_t f4 = v4 ? *reinterpret_cast<const uint16_t*>(row + po + 10u) : 0u;
  const uint32_t ft = kind ? *reinterpret_cast<const uint16_t*>(row + po + a + fo) : 0u;
  if (li == 0) rs -= f4;

  // The whole chunks: chunk at o (lane li, line k) counts iff A <= o - pa < B.
  uint32_t w = (li == 2 ? rs : 0u) + tail;
  const uint32_t d = cl - pa - A;
#pragma unroll
  for (int k = 0; k < (int)KR; ++k) {
    const uint32_t t = rx_wsum4(v[k]);
    w += (d + U * k) < span ? t : 0u;
  }
  if (wslow) {  // a padded frame in this wave: lines >= 2 re-read, range-checked
    w2 = 0;
    for (uint32_t k0 = KR; __builtin_amdgcn_ballot_w64((d + U * k0) < span) != 0; k0 += 4) {
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const uint32_t t = rx_wsum4(rx_load<AN>(rsrc, off_of(cl + U * (k0 + k))));
        w2 += (d + U * (k0 + k)) < span ? t : 0u;
      }
    }
  } else {
    for (uint32_t k0 = NB; __builtin_amdgcn_ballot_w64(k0 <= klast && kind) != 0; k0 += 4) {
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const uint4 x4 = rx_load<AN>(rsrc, ((k0 + k) <= klast ? cl1 : nrec) + U * (k0 + k));
        w2 = __builtin_amdgcn_sad_u16(x4.x, 0u, w2);
        w2 = __builtin_amdgcn_sad_u16(x4.y, 0u, w2);
        w2 = __builtin_amdgcn_sad_u16(x4.z, 0u, w2);
        w2 = __builtin_amdgcn_sad_u16(x4.w, 0u, w2);
      }
    }
  }
  w += w2;
  w += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)w, 0xB1, 0xF, 0xF, false);   // quad_perm 1,0,3,2
  w += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)w, 0x4E, 0xF, 0xF, false);   // quad_perm 2,3,0,1
  w += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)w, 0x141, 0xF, 0xF, false);  // row_half_mirror
  const uint32_t addr = (uint32_t)__builtin_amdgcn_mov_dpp((int)rs, 0x55, 0xF, 0xF, false);  // lane 1's

  // Every load of this wave has returned before any of its stores issues.
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  if (li == 0 && live) {
    const uint32_t net = l3 ? rx_class(rs) : 0u;  // the IPv4 header's sum, its field read as zero
    const bool l4 = kind && !malformed;  // the transport field is written
    uint32_t tr = 0;
    if (l4) {
      const uint32_t wt = rx_class(w - ft);
      // PseudoHeaderChecksum(proto, src, dst, uint16(size)) (checksum.go:112-122) for all but ICMPv4
      const uint32_t pn = kind == 1 ? 6u : kind == 4 ? 17u : 58u;
      tr = kind == 2 ? wt : rx_fold(rx_fold(rx_class(addr) + (tsize & 0xFFFFu) + pn) + wt);
    }
    // The fields, big-endian on the wire: ^sum byte-swapped is the halfword
    // to store.  Both lie in [pa, pa + P), inside this slot and the resource.
    if (l3) {
      const uint32_t f = ~net & 0xFFFFu;
      __builtin_amdgcn_raw_buffer_store_b16((short)(((f & 0xFFu) << 8) | (f >> 8)), rsrc, (int)(pa + 10u), 0, SP);
    }
    if (l4) {
      const uint32_t f = ~tr & 0xFFFFu;
      __builtin_amdgcn_raw_buffer_store_b16((short)(((f & 0xFFu) << 8) | (f >> 8)), rsrc, (int)(pa + a + fo), 0, SP);
    }
    const uint32_t status = malformed ? kTxrMalformed : l4 ? kTxrL4 : l3 ? kTxrL3 : kTxrNone;
    if (g.status) g.status[s] = (uint8_t)status;
    if (g.sums) {
      g.sums[2 * s] = (uint16_t)net;
      g.sums[2 * s + 1] = (uint16_t)tr;
    }
    if (g.at) g.at[s] = (uint8_t)(l4 ? a + fo : 0u);
    if (over) atomicAdd(g.err, 1ull);
  }
}

// Lines per batch for the ring's longest frame, as rx_ring's: every line of
// an MTU packet (13 lines) in one batch, 16 at most.
static int tx_batch_lines(const TxRingGeo& g) {
  const uint64_t cap = (uint64_t)kTxrMaxIp + g.frame_at + g.link;
  const uint64_t longest = g.stride < cap ? g.stride : cap;
  const uint64_t lines = (longest + 126 + 127) / 128;
  return lines <= 2 ? 2 : lines <= 4 ? 4 : lines <= 8 ? 8 : lines <= 13 ? 13 : 16;
}

template <int NB, int SP>
static hipError_t launch_tx_ring_t(const TxRingGeo& g, hipStream_t stream) {
  const uint64_t per_wg = (uint64_t)kTxrWaves * 8u;
  hipLaunchKernelGGL((tx_ring<NB, SP>), dim3((uint32_t)((g.n + per_wg - 1) / per_wg)), dim3(64 * kTxrWaves), 0,
                     stream, g);
  return hipGetLastError();
}

template <int SP>
static hipError_t launch_tx_ring_p(const TxRingGeo& g, hipStream_t stream) {
  switch (tx_batch_lines(g)) {
    case 2: return launch_tx_ring_t<2, SP>(g, stream);
    case 4: return launch_tx_ring_t<4, SP>(g, stream);
    case 8: return launch_tx_ring_t<8, SP>(g, stream);
    case 13: return launch_tx_ring_t<13, SP>(g, stream);
    default: return launch_tx_ring_t<16, SP>(g, stream);
  }
}

// The product's store policy (kTxrStoreAux; DESIGN.md §4.10 has both figures,
// tools/tx_ring_variants.hip times the other).
hipError_t launch_tx_ring(const TxRingGeo& g, hipStream_t stream) {
  if (g.n == 0) return hipSuccess;
  return launch_tx_ring_p<kTxrStoreAux>(g, stream);
}

}  // namespace nsk
