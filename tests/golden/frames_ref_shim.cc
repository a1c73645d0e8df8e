// Two C entry points over the reference's own QuicFramer, for
// tests/golden/make_golden_frames.py.  frames_ref_build has BuildDataPacket
// write a packet from a list of frame descriptions and returns the bytes behind
// the private flags; frames_ref_process puts any bytes behind a packet header
// the framer wrote itself, NULL-encrypts the packet (EncryptInPlace) and hands
// it to ProcessPacket with a visitor that records every frame it is shown and
// always returns true.  Nothing of the framer is restated.
#include <stdint.h>

#include <cstring>
#include <string>
#include <vector>

#include "net/quic/core/quic_data_writer.h"
#include "net/quic/core/quic_framer.h"

using namespace net;

namespace {

// what a visitor call carried; the columns of the fixture
struct Seen {
  uint32_t type;   // the wire value 0..8, 0x80 stream, 0x40 ack
  uint32_t flags;  // stream: 1 fin; ack: 1 truncated
  uint32_t len;    // stream data, reason text, padding bytes; ack: missing packets
  uint32_t id;
  uint64_t val;
  uint32_t code;
  uint32_t sum;  // FNV-1a of the stream data or the text
};

uint32_t Fnv(const char* p, size_t n) {
  uint32_t h = 2166136261u;
  for (size_t i = 0; i < n; ++i) h = (h ^ static_cast<uint8_t>(p[i])) * 16777619u;
  return h;
}

class Recorder : public QuicFramerVisitorInterface {
 public:
  std::vector<Seen> seen;
  uint64_t packet_number = 0;
  bool complete = false;
  void OnError(QuicFramer*) override {}
  bool OnProtocolVersionMismatch(QuicVersion) override { return false; }
  void OnPacket() override {}
  void OnPublicResetPacket(const QuicPublicResetPacket&) override {}
  void OnVersionNegotiationPacket(const QuicVersionNegotiationPacket&) override {}
  bool OnUnauthenticatedPublicHeader(const QuicPacketPublicHeader&) override { return true; }
  bool OnUnauthenticatedHeader(const QuicPacketHeader&) override { return true; }
  void OnDecryptedPacket(EncryptionLevel) override {}
  bool OnPacketHeader(const QuicPacketHeader& h) override {
    packet_number = h.packet_number;
    return true;
  }
  bool OnStreamFrame(const QuicStreamFrame& f) override {
    seen.push_back({0x80, f.fin ? 1u : 0u, f.data_length, f.stream_id, f.offset, 0,
                    Fnv(f.data_buffer, f.data_length)});
    return true;
  }
  bool OnAckFrame(const QuicAckFrame& f) override {
    seen.push_back({0x40, f.is_truncated ? 1u : 0u,
                    static_cast<uint32_t>(f.packets.NumPacketsSlow()), 0, f.largest_observed,
                    f.entropy_hash, 0});
    return true;
  }
  bool OnStopWaitingFrame(const QuicStopWaitingFrame& f) override {
    seen.push_back({6, 0, 0, 0, f.least_unacked, f.entropy_hash, 0});
    return true;
  }
  bool OnPaddingFrame(const QuicPaddingFrame& f) override {
    seen.push_back({0, 0, static_cast<uint32_t>(f.num_padding_bytes), 0, 0, 0, 0});
    return true;
  }
  bool OnPingFrame(const QuicPingFrame&) override {
    seen.push_back({7, 0, 0, 0, 0, 0, 0});
    return true;
  }
  bool OnRstStreamFrame(const QuicRstStreamFrame& f) override {
    seen.push_back({1, 0, 0, f.stream_id, f.byte_offset, static_cast<uint32_t>(f.error_code), 0});
    return true;
  }
  bool OnConnectionCloseFrame(const QuicConnectionCloseFrame& f) override {
    seen.push_back({2, 0, static_cast<uint32_t>(f.error_details.size()), 0, 0,
                    static_cast<uint32_t>(f.error_code),
                    Fnv(f.error_details.data(), f.error_details.size())});
    return true;
  }
  bool OnGoAwayFrame(const QuicGoAwayFrame& f) override {
    seen.push_back({3, 0, static_cast<uint32_t>(f.reason_phrase.size()), f.last_good_stream_id, 0,
                    static_cast<uint32_t>(f.error_code),
                    Fnv(f.reason_phrase.data(), f.reason_phrase.size())});
    return true;
  }
  bool OnWindowUpdateFrame(const QuicWindowUpdateFrame& f) override {
    seen.push_back({4, 0, 0, f.stream_id, f.byte_offset, 0, 0});
    return true;
  }
  bool OnBlockedFrame(const QuicBlockedFrame& f) override {
    seen.push_back({5, 0, 0, f.stream_id, 0, 0, 0});
    return true;
  }
  bool OnPathCloseFrame(const QuicPathCloseFrame& f) override {
    seen.push_back({8, 0, 0, f.path_id, 0, 0, 0});
    return true;
  }
  void OnPacketComplete() override { complete = true; }
};

class FixedEntropy : public QuicReceivedEntropyHashCalculatorInterface {
 public:
  QuicPacketEntropyHash EntropyHash(QuicPacketNumber packet_number) const override {
    return static_cast<uint8_t>(packet_number * 37 + 11);
  }
};

QuicPacketNumberLength PnLength(int n) {
  switch (n) {
    case 1: return PACKET_1BYTE_PACKET_NUMBER;
    case 2: return PACKET_2BYTE_PACKET_NUMBER;
    case 4: return PACKET_4BYTE_PACKET_NUMBER;
    default: return PACKET_6BYTE_PACKET_NUMBER;
  }
}

QuicPacketHeader MakeHeader(uint64_t pn, int pn_len) {
  QuicPacketHeader h;
  h.public_header.connection_id = 0x0102030405060708ull;
  h.public_header.connection_id_length = PACKET_8BYTE_CONNECTION_ID;
  h.public_header.reset_flag = false;
  h.public_header.version_flag = false;
  h.public_header.packet_number_length = PnLength(pn_len);
  h.packet_number = pn;
  h.entropy_flag = false;
  return h;
}

// the header with its private flags byte, as AppendPacketHeader writes it
size_t WriteHeader(QuicFramer* framer, uint64_t pn, int pn_len, char* buf, size_t cap) {
  QuicDataWriter writer(cap, buf);
  if (!framer->AppendPacketHeader(MakeHeader(pn, pn_len), &writer)) return 0;
  return writer.length();
}

}  // namespace

#define REF_API extern "C" __attribute__((visibility("default")))

// QUIC_LAST_ERROR and QUIC_STREAM_LAST_ERROR, to which the framer clamps, and
// the twelve error codes ProcessFrameData can leave, in the order of the
// fixture's verdict classes.
REF_API void frames_ref_limits(uint32_t* last_error, uint32_t* stream_last_error,
                               uint32_t* codes) {
  *last_error = QUIC_LAST_ERROR;
  *stream_last_error = QUIC_STREAM_LAST_ERROR;
  const QuicErrorCode order[12] = {QUIC_NO_ERROR,
                                   QUIC_MISSING_PAYLOAD,
                                   QUIC_INVALID_FRAME_DATA,
                                   QUIC_INVALID_STREAM_DATA,
                                   QUIC_INVALID_ACK_DATA,
                                   QUIC_INVALID_RST_STREAM_DATA,
                                   QUIC_INVALID_CONNECTION_CLOSE_DATA,
                                   QUIC_INVALID_GOAWAY_DATA,
                                   QUIC_INVALID_WINDOW_UPDATE_DATA,
                                   QUIC_INVALID_BLOCKED_DATA,
                                   QUIC_INVALID_STOP_WAITING_DATA,
                                   QUIC_INVALID_PATH_CLOSE_DATA};
  for (int i = 0; i < 12; ++i) codes[i] = order[i];
}

// BuildDataPacket over n frames; kind[i] is the fixture's type value and a, b,
// c, d its parameters:
//   0x80 stream   a id, b offset, c data length, d fin
//   0x40 ack      a largest observed, b missing packets (largest - 2, - 4, ...),
//                 c receipt times, d entropy hash
//   0 padding (to room)   1 rst: a id, b offset, c code   2 close: c code, d text
//   length   3 goaway: a last good stream, c code, d text length   4 window
//   update: a id, b offset   5 blocked: a id   6 stop waiting: a least unacked,
//   d hash   7 ping   8 path close: a path id
// room is what the packet may hold behind its header.  Returns the length of
// the bytes behind the private flags, copied to out; 0 where the framer failed.
REF_API size_t frames_ref_build(int version, uint64_t pn, int pn_len, size_t n,
                                const uint32_t* kind, const uint64_t* a, const uint64_t* b,
                                const uint64_t* c, const uint64_t* d, size_t room, uint8_t* out,
                                size_t out_cap) {
  QuicFramer framer(AllSupportedVersions(), QuicTime::Zero(), Perspective::IS_CLIENT);
  framer.set_version(static_cast<QuicVersion>(version));
  FixedEntropy entropy;
  framer.set_received_entropy_calculator(&entropy);
  char head[64];
  const size_t head_len = WriteHeader(&framer, pn, pn_len, head, sizeof(head));
  if (head_len == 0) return 0;
  const QuicPacketHeader header = MakeHeader(pn, pn_len);

  // the frames' owners: QuicFrame holds pointers
  std::vector<std::unique_ptr<QuicStreamFrame>> streams;
  std::vector<std::unique_ptr<QuicAckFrame>> acks;
  std::vector<std::unique_ptr<QuicRstStreamFrame>> rsts;
  std::vector<std::unique_ptr<QuicConnectionCloseFrame>> closes;
  std::vector<std::unique_ptr<QuicGoAwayFrame>> goaways;
  std::vector<std::unique_ptr<QuicWindowUpdateFrame>> updates;
  std::vector<std::unique_ptr<QuicBlockedFrame>> blockeds;
  std::vector<std::unique_ptr<QuicStopWaitingFrame>> waits;
  std::vector<std::unique_ptr<QuicPathCloseFrame>> paths;
  std::vector<std::string> texts;
  texts.reserve(n);
  QuicFrames frames;
  for (size_t i = 0; i < n; ++i) {
    std::string text;
    const size_t text_len = kind[i] == 0x80 ? c[i] : (kind[i] == 2 || kind[i] == 3) ? d[i] : 0;
    for (size_t j = 0; j < text_len; ++j) text.push_back(static_cast<char>(i * 31 + j * 7 + 1));
    texts.push_back(text);
    switch (kind[i]) {
      case 0x80:
        streams.emplace_back(new QuicStreamFrame(static_cast<QuicStreamId>(a[i]), d[i] != 0, b[i],
                                                 base::StringPiece(texts.back())));
        frames.push_back(QuicFrame(streams.back().get()));
        break;
      case 0x40: {
        std::unique_ptr<QuicAckFrame> ack(new QuicAckFrame);
        ack->largest_observed = a[i];
        ack->entropy_hash = static_cast<uint8_t>(d[i]);
        ack->missing = true;
        ack->ack_delay_time = QuicTime::Delta::FromMicroseconds(1000 + i);
        for (uint64_t k = 0; k < b[i]; ++k) ack->packets.Add(a[i] - 2 * (b[i] - k));
        for (uint64_t k = 0; k < c[i]; ++k)
          ack->received_packet_times.push_back(std::make_pair(
              a[i] - (c[i] - 1 - k) * 2,
              QuicTime::Zero() + QuicTime::Delta::FromMicroseconds(5000 + 300 * k)));
        acks.push_back(std::move(ack));
        frames.push_back(QuicFrame(acks.back().get()));
        break;
      }
      case 0:
        frames.push_back(QuicFrame(QuicPaddingFrame()));
        break;
      case 1:
        rsts.emplace_back(new QuicRstStreamFrame(static_cast<QuicStreamId>(a[i]),
                                                 static_cast<QuicRstStreamErrorCode>(c[i]), b[i]));
        frames.push_back(QuicFrame(rsts.back().get()));
        break;
      case 2:
        closes.emplace_back(new QuicConnectionCloseFrame);
        closes.back()->error_code = static_cast<QuicErrorCode>(c[i]);
        closes.back()->error_details = texts.back();
        frames.push_back(QuicFrame(closes.back().get()));
        break;
      case 3:
        goaways.emplace_back(new QuicGoAwayFrame(static_cast<QuicErrorCode>(c[i]),
                                                 static_cast<QuicStreamId>(a[i]), texts.back()));
        frames.push_back(QuicFrame(goaways.back().get()));
        break;
      case 4:
        updates.emplace_back(new QuicWindowUpdateFrame(static_cast<QuicStreamId>(a[i]), b[i]));
        frames.push_back(QuicFrame(updates.back().get()));
        break;
      case 5:
        blockeds.emplace_back(new QuicBlockedFrame(static_cast<QuicStreamId>(a[i])));
        frames.push_back(QuicFrame(blockeds.back().get()));
        break;
      case 6:
        waits.emplace_back(new QuicStopWaitingFrame);
        waits.back()->least_unacked = a[i];
        waits.back()->entropy_hash = static_cast<uint8_t>(d[i]);
        frames.push_back(QuicFrame(waits.back().get()));
        break;
      case 7:
        frames.push_back(QuicFrame(QuicPingFrame()));
        break;
      case 8:
        paths.emplace_back(new QuicPathCloseFrame(static_cast<QuicPathId>(a[i])));
        frames.push_back(QuicFrame(paths.back().get()));
        break;
      default:
        return 0;
    }
  }
  std::vector<char> packet(head_len + room);
  const size_t total = framer.BuildDataPacket(header, frames, packet.data(), packet.size());
  if (total <= head_len || total - head_len > out_cap) return 0;
  std::memcpy(out, packet.data() + head_len, total - head_len);
  return total - head_len;
}

// ProcessPacket on [header][private flags 0][body], NULL-encrypted, by a server
// at `version`.  Returns the frames the visitor saw (at most cap are stored, one
// per column entry); *error the framer's QuicErrorCode, *accepted ProcessPacket's
// answer, *complete OnPacketComplete, *packet_number what OnPacketHeader carried.
REF_API size_t frames_ref_process(int version, uint64_t pn, int pn_len, const uint8_t* body,
                                  size_t body_len, int32_t* error, int32_t* accepted,
                                  int32_t* complete, uint64_t* packet_number, char* detailed,
                                  size_t detailed_cap, size_t cap, uint32_t* type, uint32_t* flags,
                                  uint32_t* len, uint32_t* id, uint64_t* val, uint32_t* code,
                                  uint32_t* sum) {
  QuicFramer writer(AllSupportedVersions(), QuicTime::Zero(), Perspective::IS_CLIENT);
  writer.set_version(static_cast<QuicVersion>(version));
  std::vector<char> packet(64 + body_len + 64);
  const size_t head_len = WriteHeader(&writer, pn, pn_len, packet.data(), 64);
  if (head_len == 0) return static_cast<size_t>(-1);
  if (body_len) std::memcpy(packet.data() + head_len, body, body_len);
  const size_t ad_len = head_len - 1;  // (the private flags byte is encrypted)
  const size_t sealed = writer.EncryptInPlace(ENCRYPTION_NONE, kDefaultPathId, pn, ad_len,
                                              head_len + body_len, packet.size(), packet.data());
  if (sealed == 0) return static_cast<size_t>(-1);

  QuicFramer framer(AllSupportedVersions(), QuicTime::Zero(), Perspective::IS_SERVER);
  framer.set_version(static_cast<QuicVersion>(version));
  Recorder visitor;
  framer.set_visitor(&visitor);
  QuicEncryptedPacket encrypted(packet.data(), sealed, false);
  *accepted = framer.ProcessPacket(encrypted) ? 1 : 0;
  *error = framer.error();
  *complete = visitor.complete ? 1 : 0;
  *packet_number = visitor.packet_number;
  std::strncpy(detailed, framer.detailed_error().c_str(), detailed_cap - 1);
  detailed[detailed_cap - 1] = 0;
  for (size_t k = 0; k < visitor.seen.size() && k < cap; ++k) {
    const Seen& s = visitor.seen[k];
    type[k] = s.type;
    flags[k] = s.flags;
    len[k] = s.len;
    id[k] = s.id;
    val[k] = s.val;
    code[k] = s.code;
    sum[k] = s.sum;
  }
  return visitor.seen.size();
}
