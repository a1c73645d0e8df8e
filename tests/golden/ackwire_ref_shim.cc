// One C entry point over the reference's own QuicFramer, for
// tests/golden/make_golden_ackwire.py: BuildDataPacket with a single v<=31 ack
// frame at a chosen capacity; what comes back is the frame's bytes behind the
// packet header.  The entropy calculator the framer asks when it truncates is
// fed from the case: the packets received with the entropy flag set are listed,
// every other received packet has flag 0.  Nothing of the framer is restated.
#include <stdint.h>

#include <cstring>
#include <limits>
#include <vector>

#include "net/quic/core/quic_data_writer.h"
#include "net/quic/core/quic_framer.h"

namespace {

class ListedEntropy : public net::QuicReceivedEntropyHashCalculatorInterface {
 public:
  ListedEntropy(uint8_t base, const uint64_t* flagged, size_t n)
      : base_(base), flagged_(flagged, flagged + n) {}
  net::QuicPacketEntropyHash EntropyHash(net::QuicPacketNumber packet_number) const override {
    uint8_t h = base_;
    for (uint64_t pn : flagged_)
      if (pn <= packet_number) h ^= static_cast<uint8_t>(1u << (pn % 8));
    return h;
  }

 private:
  uint8_t base_;
  std::vector<uint64_t> flagged_;
};

}  // namespace

// Returns the frame's length (its bytes in out), 0 where the framer failed.
// cap is the room behind the packet header; delay_us UINT64_MAX is infinite.
extern "C" __attribute__((visibility("default"))) size_t ackwire_ref_frame(
    uint64_t largest_observed, uint8_t entropy_hash, const uint64_t* miss_lo,
    const uint64_t* miss_hi, size_t n_miss, uint64_t delay_us, size_t cap, uint8_t base_hash,
    const uint64_t* flagged, size_t n_flagged, uint8_t* out, size_t out_cap) {
  net::QuicFramer framer(net::AllSupportedVersions(), net::QuicTime::Zero(),
                         net::Perspective::IS_SERVER);
  framer.set_version(net::QUIC_VERSION_31);
  ListedEntropy entropy(base_hash, flagged, n_flagged);
  framer.set_received_entropy_calculator(&entropy);
  net::QuicPacketHeader header;
  header.public_header.connection_id = 0x0102030405060708ull;
  header.public_header.connection_id_length = net::PACKET_8BYTE_CONNECTION_ID;
  header.public_header.reset_flag = false;
  header.public_header.version_flag = false;
  header.public_header.packet_number_length = net::PACKET_6BYTE_PACKET_NUMBER;
  header.packet_number = 7;
  char head[64];
  net::QuicDataWriter head_writer(sizeof(head), head);
  if (!framer.AppendPacketHeader(header, &head_writer)) return 0;
  const size_t head_len = head_writer.length();

  net::QuicAckFrame ack;
  ack.largest_observed = largest_observed;
  ack.entropy_hash = entropy_hash;
  ack.missing = true;
  ack.ack_delay_time = delay_us == std::numeric_limits<uint64_t>::max()
                           ? net::QuicTime::Delta::Infinite()
                           : net::QuicTime::Delta::FromMicroseconds(static_cast<int64_t>(delay_us));
  for (size_t i = 0; i < n_miss; ++i) ack.packets.Add(miss_lo[i], miss_hi[i]);
  net::QuicFrames frames;
  frames.push_back(net::QuicFrame(&ack));
  std::vector<char> packet(head_len + cap);
  const size_t n = framer.BuildDataPacket(header, frames, packet.data(), packet.size());
  if (n <= head_len || n - head_len > out_cap) return 0;
  std::memcpy(out, packet.data() + head_len, n - head_len);
  return n - head_len;
}
