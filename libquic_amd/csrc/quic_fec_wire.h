// quic_fec_wire.h — the v<=31 FEC wire vestiges of libquic, restated so FEC
// packets produced by the GPU path can be framed and parsed (SURVEY.md §8(f)
// rank 1).  Host C++; no payload bytes are touched here.
//
//   * Private flags byte + 1-byte first_fec_protected_packet_offset:
//     write mirrors the v<=31 header that QuicFramer::ProcessAuthenticatedHeader
//     parses (quic_framer.cc:1102-1141); flag values quic_protocol.h:343-358.
//   * Ack-frame revived-packets list (v<=31): count byte + N packet numbers of
//     the largest-observed length, little-endian (quic_framer.cc:1477-1493
//     parse, :2307-2317 write; kNumberOfRevivedPacketsSize quic_framer.h:64-65).
//   * The ack frame itself (v<=31), written and parsed: the host mirror of
//     qfec_write_ack_frames.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include <string>
#include <utility>
#include <vector>

#include "quic_fec_group.h"
#ifdef QFEC_WITH_LIBQUIC
#include "net/quic/core/quic_framer.h"
#endif

namespace net {

#ifndef QFEC_WITH_LIBQUIC
// Standalone build: the reference's values (a libquic build takes them from
// quic_protocol.h / quic_framer.h).
enum QuicPacketPrivateFlags : uint8_t {  // quic_protocol.h:343-358
  PACKET_PRIVATE_FLAGS_NONE = 0,
  PACKET_PRIVATE_FLAGS_ENTROPY = 1 << 0,
  PACKET_PRIVATE_FLAGS_FEC_GROUP = 1 << 1,
  PACKET_PRIVATE_FLAGS_FEC = 1 << 2,
  PACKET_PRIVATE_FLAGS_MAX = (1 << 3) - 1,
  PACKET_PRIVATE_FLAGS_MAX_VERSION_32 = (1 << 1) - 1,
};

const size_t kNumberOfRevivedPacketsSize = 1;  // quic_framer.h:64-65
#endif

const int kQuicVersion31 = 31;  // last version with FEC (quic_protocol.h:371-373)

struct FecHeaderFields {
  bool entropy_flag = false;
  bool fec_flag = false;      // payload is redundancy, not frames
  bool in_fec_group = false;  // payload is protected by a group
  uint8_t fec_group_offset = 0;  // packet_number - fec_group (first protected packet)
};

// Writes the private flags byte (+ offset byte when in a group).  Returns the
// bytes written, 0 if `cap` is too small or the fields are inconsistent
// (fec_flag without a group).
size_t WriteFecPrivateHeader(const FecHeaderFields& f, uint8_t* buf, size_t cap);

// Parses what WriteFecPrivateHeader wrote, with QuicFramer's checks: flags
// above the version's maximum are illegal (v > 31: only the entropy bit), the
// offset must be < packet_number.  Returns bytes consumed or 0 and sets
// *detailed_error (QUIC_INVALID_PACKET_HEADER in the framer).
size_t ParseFecPrivateHeader(const uint8_t* buf, size_t len, int quic_version,
                             QuicPacketNumber packet_number, FecHeaderFields* out,
                             std::string* detailed_error);

// Fills a QuicPacketHeader's FEC fields from parsed private flags.
void ApplyFecHeader(const FecHeaderFields& f, QuicPacketHeader* header);

// Ack-frame revived packets list.
size_t WriteRevivedPackets(const std::vector<QuicPacketNumber>& revived,
                           size_t packet_number_length, uint8_t* buf, size_t cap);
size_t ParseRevivedPackets(const uint8_t* buf, size_t len, size_t packet_number_length,
                           std::vector<QuicPacketNumber>* revived, std::string* detailed_error);

// The v<=31 ack frame (QuicFramer::AppendAckFrameAndTypeByte, quic_framer.cc:
// 2172-2320, GetAckFrameInfo :1005-1033, with the revived tail of
// integration/libquic_fec.patch; ProcessAckFrame :1400-1495 the other way).
struct AckFrameFields {
  QuicPacketNumber largest_observed = 0;
  uint8_t entropy_hash = 0;
  // Missing packets, half-open [first, second), ascending and disjoint.
  std::vector<std::pair<QuicPacketNumber, QuicPacketNumber>> missing;
  std::vector<QuicPacketNumber> revived;  // ascending
  uint64_t ack_delay_us = UINT64_MAX;     // UINT64_MAX: infinite (parsed: the ufloat16)
  bool truncated = false;                 // cut already (the build's max_ranges)
};

const size_t kMaxAckNackRanges = 255;  // kMaxNackRanges, one count byte
const uint64_t kAckUFloat16Max = UINT64_C(0x3FFC0000000);  // kUFloat16MaxValue

// QuicDataWriter::WriteUFloat16 (quic_data_writer.cc:47-84).
uint16_t AckUFloat16(uint64_t value);
// GetMinSequenceNumberLength: 1, 2, 4 or 6 bytes.
size_t AckNumberLength(QuicPacketNumber n);

// Writes f into buf[0..cap); cap is the room at the frame's first byte.  Every
// interval is split into nack ranges of at most 256 numbers; with more ranges
// than fit, the lowest are kept, the largest observed becomes (first one
// dropped) - 1 and the hash entropy_up_to(that number).  *written (nullable)
// receives the largest observed, the hash and the truncated bit of the frame.
// Receipt times are not written: the timestamp count of a frame that is not
// truncated is 0.  Returns the frame's length, 0 where the reference writer
// fails (no room for a mandatory byte) -- nothing is stored then.
typedef uint8_t (*AckEntropyUpTo)(void* user, QuicPacketNumber packet_number);
size_t WriteAckFrame(const AckFrameFields& f, AckEntropyUpTo entropy_up_to, void* user,
                     uint8_t* buf, size_t cap, AckFrameFields* written);

// Parses one ack frame at buf[0] (its type byte).  The nack ranges are merged
// back into maximal half-open intervals, ascending; ack_delay_us receives the
// ufloat16 as written.  Returns the bytes consumed or 0 and *detailed_error.
size_t ParseAckFrame(const uint8_t* buf, size_t len, AckFrameFields* out,
                     std::string* detailed_error);

// One packet's frames (QuicFramer::ProcessFrameData, quic_framer.cc:1168-1342,
// with a visitor that always returns true): the host mirror of
// qfec_scan_frames.  Verdicts, the QFEC_FRM_* of include/qfec.h.
enum FrameScanStatus : uint8_t {
  kFrmOk = 0,
  kFrmSkipped = 1,        // (the device call's: not accepted, or an FEC packet)
  kFrmNoFrames = 2,       // "Packet has no frames."
  kFrmIllegalType = 3,    // "Illegal frame type."
  kFrmStream = 4,         // QUIC_INVALID_STREAM_DATA
  kFrmAck = 5,            // QUIC_INVALID_ACK_DATA
  kFrmRst = 6,            // QUIC_INVALID_RST_STREAM_DATA
  kFrmClose = 7,          // QUIC_INVALID_CONNECTION_CLOSE_DATA
  kFrmGoaway = 8,         // QUIC_INVALID_GOAWAY_DATA
  kFrmWindowUpdate = 9,   // QUIC_INVALID_WINDOW_UPDATE_DATA
  kFrmBlocked = 10,       // QUIC_INVALID_BLOCKED_DATA
  kFrmStopWaiting = 11,   // QUIC_INVALID_STOP_WAITING_DATA
  kFrmPathClose = 12,     // QUIC_INVALID_PATH_CLOSE_DATA
  kFrmBadLeast = 13,      // STOP_WAITING delta above the packet number
  kFrmTooMany = 14,       // more than max_frames frames
  kFrmPnLen = 15,         // (the device call's: pkt_pn_len not 1, 2, 4 or 6)
  kFrmRange = 16,         // (the device call's: connection out of range)
};
const uint8_t kFrameTypeStream = 0x80, kFrameTypeAck = 0x40;  // frm_type beside the wire's 0..8

struct ScannedFrame {
  uint8_t type = 0;   // the wire value 0..8, kFrameTypeStream, kFrameTypeAck
  uint8_t flags = 0;  // stream: 1 fin, 2 had a length; ack: the type byte's low six bits
  uint32_t off = 0;   // from the body's first byte: stream data, the ack's type byte, the reason
                      // text of a close or goaway, the bytes behind a padding's type byte
  uint16_t len = 0;   // stream data, the whole ack frame, the text, the padding
  uint32_t id = 0;    // stream id; goaway: last good stream; path close: path id
  uint64_t val = 0;   // stream offset; rst, window update: byte offset; stop waiting: least
                      // unacked; ack: largest observed
  uint32_t code = 0;  // rst, close, goaway: the error code as read; stop waiting, ack: the hash
};

// Walks body[0..len) (len <= 65535), the bytes behind the private header, for
// quic_version 1..33 and a packet number length of 1, 2, 4 or 6.  *walked
// receives the frames read before the verdict was reached, whatever it is (at
// most max_frames); a packet lists its frames only under kFrmOk.  Multi-byte
// values are little-endian, as QuicDataReader reads them.  The ack is stepped
// over: its ranges are bounds-checked, not looked at.  No byte at or beyond len
// is read.
FrameScanStatus ScanFrames(const uint8_t* body, size_t len, int quic_version,
                           QuicPacketNumber packet_number, size_t packet_number_length,
                           size_t max_frames, std::vector<ScannedFrame>* walked);

// Serialise a complete FEC packet body for the send side: private header
// (FEC | FEC_GROUP, offset = packet_number - fec_group) followed by the
// redundancy (QuicFecGroup::PayloadParity()).  Returns bytes written or 0.
size_t SerializeFecPacketBody(QuicPacketNumber packet_number, QuicFecGroupNumber fec_group,
                              bool entropy_flag, StringPiece redundancy, uint8_t* buf,
                              size_t cap);

}  // namespace net
