// nsh::tx_ring_patch (host_logic.h) — the stores ns_csum_tx_ring_host makes
// into the caller's ring from what the device reported — as a stand-alone
// program under ASan + UBSan (netstack_amd/csrc/Makefile, tx_ring_patch_test;
// run by tests/test_tx_ring_abi.py).  The ring is an exact-size heap block, so
// any store outside it is an ASan report; inside it, every byte is compared
// with a model that allows only the two fields of slots whose report passes
// frame_at + link_hdr + at + 2 <= len <= stride.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "netstack_csum.h"
#include "host_logic.h"

namespace {

int failures = 0;
#define CHECK(c)                                                  \
  do {                                                            \
    if (!(c)) {                                                   \
      std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); \
      ++failures;                                                 \
    }                                                             \
  } while (0)

struct Case {
  uint64_t stride;
  uint32_t pre, n;
  std::vector<uint32_t> len;
  std::vector<uint16_t> sums;
  std::vector<uint8_t> at;
};

// Runs the patch over [first, first + count) and checks every byte.
void run(const Case& c, uint32_t first, uint32_t count, std::mt19937& rng) {
  const size_t bytes = (size_t)c.n * c.stride;
  uint8_t* ring = static_cast<uint8_t*>(std::malloc(bytes ? bytes : 1));  // exact size: ASan guards both ends
  for (size_t i = 0; i < bytes; ++i) ring[i] = (uint8_t)rng();
  std::vector<uint8_t> want(ring, ring + bytes);
  uint64_t stores = 0;
  for (uint32_t k = 0; k < count; ++k) {
    const uint64_t s = (uint64_t)first + k, L = c.len[s];
    auto put = [&](uint64_t off, uint16_t sum) {
      if (L > c.stride || c.pre + off + 2 > L) return;
      const uint16_t f = (uint16_t)~sum;
      want[s * c.stride + c.pre + off] = (uint8_t)(f >> 8);
      want[s * c.stride + c.pre + off + 1] = (uint8_t)f;
      ++stores;
    };
    if (c.sums[2 * k]) put(10, c.sums[2 * k]);
    if (c.at[k]) put(c.at[k], c.sums[2 * k + 1]);
  }
  const uint64_t got = nsh::tx_ring_patch(ring, c.stride, c.pre, c.len.data(), first, count, c.sums.data(), c.at.data());
  CHECK(got == stores);
  CHECK(std::memcmp(ring, want.data(), bytes) == 0);
  std::free(ring);
}

}  // namespace

int main() {
  std::mt19937 rng(20260);
  uint64_t total = 0;
  // in-range reports: every store lands, big-endian, complemented
  {
    Case c{1504, 14, 8, {}, {}, {}};
    for (uint32_t k = 0; k < c.n; ++k) {
      c.len.push_back(14 + 20 + 20 + k);
      c.sums.push_back((uint16_t)(0x1234 + k));
      c.sums.push_back((uint16_t)(0xFFFF - k));
      c.at.push_back(36);
    }
    std::vector<uint8_t> ring(c.n * c.stride, 0xAA);
    const uint64_t st = nsh::tx_ring_patch(ring.data(), c.stride, c.pre, c.len.data(), 0, c.n, c.sums.data(), c.at.data());
    CHECK(st == 2ull * c.n);
    for (uint32_t k = 0; k < c.n; ++k) {
      const uint8_t* ip = ring.data() + k * c.stride + 14;
      const uint16_t f4 = (uint16_t)~c.sums[2 * k], ft = (uint16_t)~c.sums[2 * k + 1];
      CHECK(ip[10] == (f4 >> 8) && ip[11] == (f4 & 0xFF) && ip[36] == (ft >> 8) && ip[37] == (ft & 0xFF));
      CHECK(ip[9] == 0xAA && ip[12] == 0xAA && ip[35] == 0xAA && ip[38] == 0xAA);
    }
    run(c, 0, c.n, rng);
    run(c, 3, 4, rng);  // a later chunk: slots from `first`, reports from 0
  }
  // out-of-range reports: a field past the frame's length, a length over the
  // stride, a field in the slot's last bytes (the last one allowed) and one
  // byte further (refused)
  {
    Case c{80, 0, 6, {40, 81, 80, 80, 0, 11}, {1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12}, {76, 36, 78, 79, 22, 0}};
    run(c, 0, c.n, rng);
    std::vector<uint8_t> ring(c.n * c.stride, 0);
    const uint64_t st = nsh::tx_ring_patch(ring.data(), c.stride, c.pre, c.len.data(), 0, c.n, c.sums.data(), c.at.data());
    // slot 0: IPv4 only (76 + 2 > 40); 1: none (len > stride); 2: both (78 + 2 == 80); 3: IPv4 only; 4, 5: none
    CHECK(st == 1 + 0 + 2 + 1 + 0 + 0);
  }
  // garbage: random offsets, lengths, sums, strides and link prefixes
  for (int it = 0; it < 4000; ++it) {
    Case c;
    c.stride = 16 * (1 + rng() % 24);
    c.pre = rng() % 3 == 0 ? rng() % 300 : (rng() % 2 ? 14 : 0);
    c.n = 1 + rng() % 9;
    for (uint32_t k = 0; k < c.n; ++k) {
      const uint32_t r = rng() % 8;
      c.len.push_back(r == 0 ? 0xFFFFFFFFu : r == 1 ? (uint32_t)c.stride + 1 : r == 2 ? (uint32_t)c.stride
                                                                                       : rng() % (2 * c.stride));
    }
    const uint32_t first = rng() % c.n, count = 1 + rng() % (c.n - first);
    for (uint32_t k = 0; k < count; ++k) {
      c.sums.push_back(rng() % 4 ? (uint16_t)rng() : 0);
      c.sums.push_back((uint16_t)rng());
      c.at.push_back(rng() % 4 ? (uint8_t)rng() : 0);
    }
    run(c, first, count, rng);
    total += count;
  }
  if (failures) {
    std::fprintf(stderr, "tx_ring_patch_test: %d failures\n", failures);
    return 1;
  }
  std::printf("tx_ring_patch_test ok: %llu random slots, in-range, out-of-range and garbage reports\n",
              (unsigned long long)total);
  return 0;
}
