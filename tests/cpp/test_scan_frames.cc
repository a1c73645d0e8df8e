// test_scan_frames.cc — ScanFrames (quic_fec_wire.h) as a stand-alone program
// for the AddressSanitizer + UBSan build of the CPU suite.  Every body sits in a
// heap buffer of exactly its length, so a read past the end is a sanitizer
// report: packets made of well-formed frames, every prefix of them, and random
// bytes.  What the walk reports is pinned to the reference framer by
// tests/test_frames_rule.py; here a whole packet must list the frames that went
// in, a prefix must never list more than the whole, and nothing may be read
// outside the body.
#include <cstdint>
#include <cstdio>
#include <memory>
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

void Put(std::vector<uint8_t>* b, uint64_t v, size_t n) {
  for (size_t i = 0; i < n; ++i) b->push_back(static_cast<uint8_t>(v >> (8 * (i % 8))));
}

// One well-formed frame that is not the packet's last (a stream frame carries
// its length; no padding); returns its type as ScanFrames reports it.
uint8_t AppendFrame(std::vector<uint8_t>* b, int version, uint64_t pn, size_t pn_len) {
  static const size_t kLengths[4] = {1, 2, 4, 6};
  switch (Below(10)) {
    case 0: {
      const size_t id_len = 1 + Below(4), off_bits = Below(8), n = Below(40);
      b->push_back(static_cast<uint8_t>(0xA0 | (Below(2) << 6) | (off_bits << 2) | (id_len - 1)));
      Put(b, Next(), id_len);
      Put(b, Next(), off_bits ? off_bits + 1 : 0);
      Put(b, n, 2);
      for (size_t i = 0; i < n; ++i) b->push_back(static_cast<uint8_t>(Next()));
      return kFrameTypeStream;
    }
    case 1: {
      const size_t l = Below(4), m = Below(4), ranges = Below(3) ? Below(6) : 255;
      const bool truncated = Below(4) == 0, nacks = Below(3) != 0;
      b->push_back(static_cast<uint8_t>(0x40 | (nacks << 5) | (truncated << 4) | (l << 2) | m));
      b->push_back(static_cast<uint8_t>(Next()));
      Put(b, Next(), kLengths[l]);
      Put(b, Next(), 2);
      if (!truncated) {
        const size_t times = Below(4);
        b->push_back(static_cast<uint8_t>(times));
        for (size_t i = 0; times && i < 5 + 3 * (times - 1); ++i) b->push_back(0x11);
      }
      if (nacks) {
        b->push_back(static_cast<uint8_t>(ranges));
        for (size_t i = 0; i < ranges * (kLengths[m] + 1); ++i) b->push_back(1);
        if (version <= 31) {
          const size_t revived = Below(4);
          b->push_back(static_cast<uint8_t>(revived));
          for (size_t i = 0; i < revived * kLengths[l]; ++i) b->push_back(2);
        }
      }
      return kFrameTypeAck;
    }
    case 2:
      b->push_back(1);
      Put(b, Next(), 16);
      return 1;
    case 3:
    case 4: {
      const uint8_t t = b->size() % 2 ? 2 : 3;
      const size_t n = Below(30);
      b->push_back(t);
      Put(b, Next(), t == 2 ? 4 : 8);
      Put(b, n, 2);
      for (size_t i = 0; i < n; ++i) b->push_back('x');
      return t;
    }
    case 5:
      b->push_back(4);
      Put(b, Next(), 12);
      return 4;
    case 6:
      b->push_back(5);
      Put(b, Next(), 4);
      return 5;
    case 7: {
      const uint64_t top = pn_len == 6 ? pn : (pn < (1ull << (8 * pn_len)) ? pn : 0);
      b->push_back(6);
      b->push_back(static_cast<uint8_t>(Next()));
      Put(b, top ? Below(top + 1) : 0, pn_len);
      return 6;
    }
    case 8:
      b->push_back(7);
      return 7;
    default:
      b->push_back(8);
      b->push_back(static_cast<uint8_t>(Next()));
      return 8;
  }
}

FrameScanStatus Scan(const std::vector<uint8_t>& body, size_t len, int version, uint64_t pn,
                     size_t pn_len, size_t max_frames, std::vector<ScannedFrame>* walked) {
  std::unique_ptr<uint8_t[]> exact(new uint8_t[len ? len : 1]);  // (a read past len is a report)
  std::copy(body.begin(), body.begin() + len, exact.get());
  return ScanFrames(len ? exact.get() : nullptr, len, version, pn, pn_len, max_frames, walked);
}

}  // namespace

int main() {
  static const size_t kPnLengths[4] = {1, 2, 4, 6};
  static const uint64_t kNumbers[5] = {1, 200, 60000, 1ull << 31, (1ull << 47) + 3};
  for (int i = 0; i < 1500; ++i) {
    const int version = Below(2) ? 31 : 33;
    const size_t pn_len = kPnLengths[Below(4)];
    const uint64_t pn = kNumbers[Below(5)];
    std::vector<uint8_t> body;
    std::vector<uint8_t> types;
    const size_t n = 1 + Below(7);
    for (size_t k = 0; k < n; ++k) types.push_back(AppendFrame(&body, version, pn, pn_len));
    if (Below(3) == 0) {  // padding last
      body.insert(body.end(), Below(9) + 1, 0);
      types.push_back(0);
    }
    std::vector<ScannedFrame> walked, part;
    CHECK(Scan(body, body.size(), version, pn, pn_len, 255, &walked) == kFrmOk);
    CHECK(walked.size() == types.size());
    for (size_t k = 0; k < walked.size() && k < types.size(); ++k) {
      CHECK(walked[k].type == types[k]);
      CHECK(walked[k].off <= body.size() && walked[k].off + walked[k].len <= body.size());
    }
    // one frame too many for the table is a result, and the frames before it stand
    if (types.size() > 1) {
      CHECK(Scan(body, body.size(), version, pn, pn_len, types.size() - 1, &part) == kFrmTooMany);
      CHECK(part.size() == types.size() - 1);
    }
    for (size_t cut = 0; cut < body.size(); ++cut) {  // every prefix
      const FrameScanStatus s = Scan(body, cut, version, pn, pn_len, 255, &part);
      CHECK(part.size() <= walked.size());
      CHECK((cut == 0) == (s == kFrmNoFrames));
      for (size_t k = 0; k < part.size(); ++k)
        CHECK(part[k].off <= cut && part[k].off + part[k].len <= cut);
    }
  }
  for (int i = 0; i < 40000; ++i) {  // anything at all: no read past the end
    const size_t n = Below(48);
    std::vector<uint8_t> junk(n);
    for (size_t b = 0; b < n; ++b) junk[b] = static_cast<uint8_t>(Next());
    if (n && Below(2)) junk[0] = static_cast<uint8_t>(Below(9));
    std::vector<ScannedFrame> walked;
    const size_t max_frames = 1 + Below(255);
    const FrameScanStatus s = Scan(junk, n, Below(2) ? 31 : 33, Next() >> Below(64),
                                   kPnLengths[Below(4)], max_frames, &walked);
    CHECK(s <= kFrmTooMany && s != kFrmSkipped && walked.size() <= max_frames);
    for (const ScannedFrame& f : walked) CHECK(f.off <= n && f.off + f.len <= n);
  }
  std::printf("%d checks, %d failures\n", g_checks, g_failures);
  return g_failures != 0;
}
