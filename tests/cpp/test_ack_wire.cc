// test_ack_wire.cc — WriteAckFrame / ParseAckFrame (quic_fec_wire.h) as a
// stand-alone program for the AddressSanitizer + UBSan build of the CPU suite.
// Every frame is written into a heap buffer of exactly `cap` bytes, so a byte
// past the room is a sanitizer report; every frame parses back into the content
// that went in; every prefix of a frame, and random bytes, are refused or
// parsed without a read past the end.  The bytes themselves are pinned to the
// reference framer by tests/test_ackwire_rule.py.
#include <cstdint>
#include <cstdio>
#include <memory>
#include <string>
#include <vector>

#include "quic_fec_wire.h"

using namespace net;

namespace {

int g_checks = 0, g_failures = 0;
#define CHECK(c)                                                  \
  do {                                                            \
    ++g_checks;                                                   \
    if (!(c)) {                                                   \
      ++g_failures;                                               \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); \
    }                                                             \
  } while (0)

uint64_t g_state = 0x9E3779B97F4A7C15ull;
uint64_t Next() {  // xorshift64*
  g_state ^= g_state >> 12;
  g_state ^= g_state << 25;
  g_state ^= g_state >> 27;
  return g_state * 0x2545F4914F6CDD1Dull;
}
uint64_t Below(uint64_t n) { return Next() % n; }

uint8_t EntropyUpTo(void* user, QuicPacketNumber pn) {
  return static_cast<uint8_t>(*static_cast<uint8_t*>(user) ^ (pn * 37));
}

AckFrameFields RandomAck() {
  static const uint64_t kTops[] = {300, 70000, 1ull << 33, (1ull << 48) - 2};
  static const uint64_t kLengths[] = {1, 1, 2, 5, 255, 256, 257, 513};
  static const uint64_t kGaps[] = {2, 2, 3, 9, 256, 70000};
  AckFrameFields f;
  f.largest_observed = kTops[Below(4)];
  f.entropy_hash = static_cast<uint8_t>(Next());
  f.ack_delay_us = Below(5) == 0 ? UINT64_MAX : Next() >> Below(60);
  f.truncated = Below(4) == 0;
  const size_t n = Below(3) == 0 ? 0 : 1 + Below(Below(4) == 0 ? 255 : 12);
  uint64_t last = f.largest_observed - 1 - Below(20);  // the highest missing number
  std::vector<std::pair<QuicPacketNumber, QuicPacketNumber>> down;
  for (size_t i = 0; i < n; ++i) {
    const uint64_t len = kLengths[Below(8)];
    if (last < len + 1) break;
    down.emplace_back(last - len + 1, last + 1);
    const uint64_t gap = kGaps[Below(6)];
    if (last - len + 1 <= gap) break;
    last = last - len + 1 - gap;
  }
  f.missing.assign(down.rbegin(), down.rend());
  for (const auto& iv : f.missing)
    if (Below(3) == 0 && f.revived.size() < 300) f.revived.push_back(iv.first);
  return f;
}

void RoundTrip(const AckFrameFields& f, size_t cap) {
  std::unique_ptr<uint8_t[]> buf(new uint8_t[cap ? cap : 1]);
  uint8_t base = 0x5A;
  AckFrameFields w;
  const size_t n = WriteAckFrame(f, EntropyUpTo, &base, buf.get(), cap, &w);
  CHECK(n <= cap);
  if (n == 0) return;
  AckFrameFields p;
  std::string err;
  std::unique_ptr<uint8_t[]> exact(new uint8_t[n]);  // (a read past the frame is a report)
  std::copy(buf.get(), buf.get() + n, exact.get());
  CHECK(ParseAckFrame(exact.get(), n, &p, &err) == n);
  CHECK(p.largest_observed == w.largest_observed && p.entropy_hash == w.entropy_hash);
  CHECK(p.truncated == w.truncated && p.ack_delay_us == AckUFloat16(f.ack_delay_us));
  CHECK(w.largest_observed <= f.largest_observed);
  if (w.largest_observed != f.largest_observed)
    CHECK(w.truncated && w.entropy_hash == EntropyUpTo(&base, w.largest_observed));
  // the missing numbers below the largest written, and the newest revived
  std::vector<std::pair<QuicPacketNumber, QuicPacketNumber>> want;
  for (const auto& iv : f.missing)
    if (iv.first <= w.largest_observed)
      want.emplace_back(iv.first, std::min(iv.second, w.largest_observed + 1));
  CHECK(p.missing == want);
  std::vector<QuicPacketNumber> listed;
  for (QuicPacketNumber r : f.revived)
    if (r <= w.largest_observed) listed.push_back(r);
  CHECK(p.revived.size() <= listed.size() && p.revived.size() <= 255);
  if (p.revived.size() <= listed.size())
    CHECK(std::equal(p.revived.begin(), p.revived.end(), listed.end() - p.revived.size()));
  for (size_t cut = 0; cut < n; cut += 1 + n / 40) {  // cut short: refused
    std::unique_ptr<uint8_t[]> part(new uint8_t[cut ? cut : 1]);
    std::copy(buf.get(), buf.get() + cut, part.get());
    CHECK(ParseAckFrame(part.get(), cut, &p, &err) == 0);
  }
}

}  // namespace

int main() {
  for (int i = 0; i < 3000; ++i) {
    const AckFrameFields f = RandomAck();
    std::vector<uint8_t> big(4096);
    uint8_t base = 0x5A;  // (more than 255 ranges are cut at any room)
    const size_t full = WriteAckFrame(f, EntropyUpTo, &base, big.data(), big.size(), nullptr);
    CHECK(full != 0);
    const size_t caps[] = {full + Below(50), full, full - 1, full / 2, full / 3 + 7, 7, 4, 0};
    for (size_t cap : caps) RoundTrip(f, cap);
  }
  for (int i = 0; i < 20000; ++i) {  // anything at all: no read past the end
    const size_t n = Below(40);
    std::unique_ptr<uint8_t[]> junk(new uint8_t[n ? n : 1]);
    for (size_t b = 0; b < n; ++b) junk[b] = static_cast<uint8_t>(Next());
    if (n) junk[0] = static_cast<uint8_t>(0x40 | (junk[0] & 0x3F));
    AckFrameFields p;
    std::string err;
    CHECK(ParseAckFrame(junk.get(), n, &p, &err) <= n);
  }
  CHECK(AckUFloat16(4095) == 4095 && AckUFloat16(4096) == 4096 && AckUFloat16(4097) == 4096);
  CHECK(AckUFloat16(kAckUFloat16Max - 1) == 0xFFFE && AckUFloat16(kAckUFloat16Max) == 0xFFFF);
  CHECK(AckUFloat16(UINT64_MAX) == 0xFFFF);
  std::printf("%d checks, %d failures\n", g_checks, g_failures);
  return g_failures != 0;
}
