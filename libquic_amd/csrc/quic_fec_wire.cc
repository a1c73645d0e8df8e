// quic_fec_wire.cc — see quic_fec_wire.h.
#include "quic_fec_wire.h"

#include <algorithm>
#include <cstring>

namespace net {

size_t WriteFecPrivateHeader(const FecHeaderFields& f, uint8_t* buf, size_t cap) {
  if (f.fec_flag && !f.in_fec_group) return 0;  // an FEC packet always names its group
  const size_t need = f.in_fec_group ? 2 : 1;
  if (cap < need) return 0;
  uint8_t flags = PACKET_PRIVATE_FLAGS_NONE;
  if (f.entropy_flag) flags |= PACKET_PRIVATE_FLAGS_ENTROPY;
  if (f.in_fec_group) flags |= PACKET_PRIVATE_FLAGS_FEC_GROUP;
  if (f.fec_flag) flags |= PACKET_PRIVATE_FLAGS_FEC;
  buf[0] = flags;
  if (f.in_fec_group) buf[1] = f.fec_group_offset;
  return need;
}

size_t ParseFecPrivateHeader(const uint8_t* buf, size_t len, int quic_version,
                             QuicPacketNumber packet_number, FecHeaderFields* out,
                             std::string* detailed_error) {
  if (len < 1) {
    *detailed_error = "Unable to read private flags.";
    return 0;
  }
  const uint8_t flags = buf[0];
  const uint8_t max =
      quic_version > kQuicVersion31 ? PACKET_PRIVATE_FLAGS_MAX_VERSION_32 : PACKET_PRIVATE_FLAGS_MAX;
  if (flags > max) {
    *detailed_error = "Illegal private flags value.";
    return 0;
  }
  FecHeaderFields f;
  f.entropy_flag = (flags & PACKET_PRIVATE_FLAGS_ENTROPY) != 0;
  f.fec_flag = (flags & PACKET_PRIVATE_FLAGS_FEC) != 0;
  f.in_fec_group = (flags & PACKET_PRIVATE_FLAGS_FEC_GROUP) != 0;
  size_t used = 1;
  if (f.in_fec_group) {
    if (len < 2) {
      *detailed_error = "Unable to read first fec protected packet offset.";
      return 0;
    }
    f.fec_group_offset = buf[1];
    if (f.fec_group_offset >= packet_number) {
      *detailed_error =
          "First fec protected packet offset must be less than the packet number.";
      return 0;
    }
    used = 2;
  }
  *out = f;
  return used;
}

void ApplyFecHeader(const FecHeaderFields& f, QuicPacketHeader* header) {
  header->entropy_flag = f.entropy_flag;
  header->fec_flag = f.fec_flag;
  header->is_in_fec_group = f.in_fec_group ? IN_FEC_GROUP : NOT_IN_FEC_GROUP;
  header->fec_group = f.in_fec_group ? header->packet_number - f.fec_group_offset : 0;
}

size_t WriteRevivedPackets(const std::vector<QuicPacketNumber>& revived,
                           size_t packet_number_length, uint8_t* buf, size_t cap) {
  if (revived.size() > 255 || packet_number_length < 1 || packet_number_length > 8) return 0;
  const size_t need = kNumberOfRevivedPacketsSize + revived.size() * packet_number_length;
  if (cap < need) return 0;
  buf[0] = static_cast<uint8_t>(revived.size());
  size_t o = 1;
  for (QuicPacketNumber p : revived) {
    if (packet_number_length < 8 && (p >> (8 * packet_number_length)) != 0) return 0;
    for (size_t b = 0; b < packet_number_length; ++b) buf[o++] = static_cast<uint8_t>(p >> (8 * b));
  }
  return o;
}

size_t ParseRevivedPackets(const uint8_t* buf, size_t len, size_t packet_number_length,
                           std::vector<QuicPacketNumber>* revived, std::string* detailed_error) {
  if (len < kNumberOfRevivedPacketsSize) {
    *detailed_error = "Unable to read num revived packets.";
    return 0;
  }
  const size_t n = buf[0];
  size_t o = 1;
  revived->clear();
  for (size_t i = 0; i < n; ++i) {
    if (o + packet_number_length > len) {
      *detailed_error = "Unable to read revived packet.";
      return 0;
    }
    QuicPacketNumber p = 0;
    for (size_t b = 0; b < packet_number_length; ++b)
      p |= static_cast<QuicPacketNumber>(buf[o++]) << (8 * b);
    revived->push_back(p);
  }
  return o;
}

uint16_t AckUFloat16(uint64_t value) {
  if (value < (UINT64_C(1) << 12)) return static_cast<uint16_t>(value);  // exponent 0
  if (value >= kAckUFloat16Max) return 0xFFFF;
  uint16_t exponent = 0;
  for (uint16_t offset = 16; offset > 0; offset /= 2) {
    if (value >= (UINT64_C(1) << (11 + offset))) {
      exponent += offset;
      value >>= offset;
    }
  }
  return static_cast<uint16_t>(value + (static_cast<uint64_t>(exponent) << 11));
}

size_t AckNumberLength(QuicPacketNumber n) {
  return n < (UINT64_C(1) << 8) ? 1 : n < (UINT64_C(1) << 16) ? 2 : n < (UINT64_C(1) << 32) ? 4 : 6;
}

namespace {

void PutNumber(uint8_t* p, size_t length, uint64_t v) {
  for (size_t b = 0; b < length; ++b) p[b] = static_cast<uint8_t>(v >> (8 * b));
}

uint64_t GetNumber(const uint8_t* p, size_t length) {
  uint64_t v = 0;
  for (size_t b = 0; b < length; ++b) v |= static_cast<uint64_t>(p[b]) << (8 * b);
  return v;
}

// nack ranges of the interval [lo, hi): ceil((hi - lo) / 256)
uint64_t RunsOf(QuicPacketNumber lo, QuicPacketNumber hi) { return hi > lo ? (hi - lo + 255) >> 8 : 0; }

}  // namespace

size_t WriteAckFrame(const AckFrameFields& f, AckEntropyUpTo entropy_up_to, void* user,
                     uint8_t* buf, size_t cap, AckFrameFields* written) {
  // GetAckFrameInfo: the ranges and the largest gap, before any truncation
  uint64_t n_runs = 0, max_delta = 0;
  QuicPacketNumber last_missing = 0;
  for (const auto& iv : f.missing) {
    if (iv.second <= iv.first) return 0;
    n_runs += RunsOf(iv.first, iv.second);
    if (last_missing != 0) max_delta = std::max<uint64_t>(max_delta, iv.first - last_missing);
    last_missing = iv.second - 1;
  }
  max_delta = std::max<uint64_t>(max_delta, f.largest_observed - last_missing);
  if (f.missing.empty()) max_delta = 0;
  const size_t ll = AckNumberLength(f.largest_observed), mm = AckNumberLength(max_delta);
  // (the reference's unsigned subtraction: with no room for the minimum it
  // wraps, every range "fits" and a write fails further down)
  const size_t fixed = 1 + (4 + ll) + kNumberOfRevivedPacketsSize;
  const size_t max_num =
      cap < fixed ? kMaxAckNackRanges : std::min(kMaxAckNackRanges, (cap - fixed) / (mm + 1));
  const bool cut = n_runs > max_num;
  const bool truncated = f.truncated || cut;
  const size_t kept = cut ? max_num : static_cast<size_t>(n_runs);
  const size_t head = 4 + ll + (truncated ? 0 : 1);
  const size_t mandatory = n_runs == 0 ? head : head + 1 + kept * (mm + 1) + 1;
  if (mandatory > cap) return 0;

  // The kept ranges, lowest first; the first one dropped names the largest.
  struct Run { QuicPacketNumber start; uint32_t length; };
  std::vector<Run> runs;
  runs.reserve(kept);
  QuicPacketNumber largest = f.largest_observed;
  bool done = false;
  for (auto iv = f.missing.begin(); iv != f.missing.end() && !done; ++iv) {
    for (uint64_t j = 0, n = RunsOf(iv->first, iv->second); j < n; ++j) {
      const QuicPacketNumber s = iv->first + 256 * j;
      if (runs.size() == kept) {
        if (cut) largest = s - 1;
        done = true;
        break;
      }
      runs.push_back({s, static_cast<uint32_t>(std::min<uint64_t>(256, iv->second - s))});
    }
  }
  uint8_t hash = f.entropy_hash;
  if (cut) hash = entropy_up_to ? entropy_up_to(user, largest) : 0;

  size_t o = 0;
  buf[o++] = static_cast<uint8_t>(0x40 | (n_runs != 0 ? 0x20 : 0) | (truncated ? 0x10 : 0) |
                                  ((ll >> 1) << 2) | (mm >> 1));
  buf[o++] = hash;
  PutNumber(buf + o, ll, largest);
  o += ll;
  PutNumber(buf + o, 2, AckUFloat16(f.ack_delay_us));
  o += 2;
  if (!truncated) buf[o++] = 0;  // no receipt times
  if (written) {
    written->largest_observed = largest;
    written->entropy_hash = hash;
    written->truncated = truncated;
  }
  if (n_runs == 0) return o;
  buf[o++] = static_cast<uint8_t>(kept);
  QuicPacketNumber last_written = largest;
  for (size_t k = kept; k-- > 0;) {
    const QuicPacketNumber end = runs[k].start + runs[k].length - 1;
    PutNumber(buf + o, mm, last_written - end);
    o += mm;
    buf[o++] = static_cast<uint8_t>(runs[k].length - 1);
    last_written = runs[k].start - 1;
  }
  // the revived tail: the newest at or below the largest written, as many as fit
  const size_t room = cap - o;  // (>= 1: mandatory <= cap)
  const size_t max_revived = std::min<size_t>(255, (room - kNumberOfRevivedPacketsSize) / ll);
  std::vector<QuicPacketNumber> revived;
  for (auto it = f.revived.rbegin(); it != f.revived.rend() && revived.size() < max_revived; ++it)
    if (*it <= largest) revived.push_back(*it);
  const size_t n = WriteRevivedPackets(revived, ll, buf + o, room);
  if (n == 0) return 0;  // (cannot happen: counted above)
  return o + n;
}

size_t ParseAckFrame(const uint8_t* buf, size_t len, AckFrameFields* out,
                     std::string* detailed_error) {
  static const size_t kLengths[4] = {1, 2, 4, 6};
  if (len < 1 || (buf[0] & 0xC0) != 0x40) {
    *detailed_error = "Not an ack frame.";
    return 0;
  }
  const uint8_t type = buf[0];
  const size_t mm = kLengths[type & 3], ll = kLengths[(type >> 2) & 3];
  AckFrameFields f;
  f.truncated = (type & 0x10) != 0;
  const bool has_nacks = (type & 0x20) != 0;
  size_t o = 1;
  if (o + 1 > len) {
    *detailed_error = "Unable to read entropy hash for received packets.";
    return 0;
  }
  f.entropy_hash = buf[o++];
  if (o + ll > len) {
    *detailed_error = "Unable to read largest observed.";
    return 0;
  }
  f.largest_observed = GetNumber(buf + o, ll);
  o += ll;
  if (o + 2 > len) {
    *detailed_error = "Unable to read ack delay time.";
    return 0;
  }
  f.ack_delay_us = GetNumber(buf + o, 2);
  o += 2;
  if (!f.truncated) {  // ProcessTimestampsInAckFrame: skipped over
    if (o + 1 > len) {
      *detailed_error = "Unable to read num received packets.";
      return 0;
    }
    const size_t n_times = buf[o++];
    const size_t bytes = n_times == 0 ? 0 : 5 + (n_times - 1) * 3;
    if (o + bytes > len) {
      *detailed_error = "Unable to read time delta in received packets.";
      return 0;
    }
    o += bytes;
  }
  if (has_nacks) {
    if (o + 1 > len) {
      *detailed_error = "Unable to read num missing packet ranges.";
      return 0;
    }
    const size_t n_ranges = buf[o++];
    QuicPacketNumber last = f.largest_observed;
    for (size_t i = 0; i < n_ranges; ++i) {
      if (o + mm + 1 > len) {
        *detailed_error = o + mm > len ? "Unable to read missing packet number delta."
                                       : "Unable to read missing packet number range.";
        return 0;
      }
      const uint64_t delta = GetNumber(buf + o, mm);
      const uint64_t range_length = buf[o + mm];
      o += mm + 1;
      if (delta > last || range_length >= last - delta) {
        *detailed_error = "Invalid missing packet range.";  // (below packet number 1)
        return 0;
      }
      last -= delta;
      const QuicPacketNumber lo = last - range_length, hi = last + 1;
      if (!f.missing.empty() && f.missing.back().first == hi) f.missing.back().first = lo;
      else f.missing.emplace_back(lo, hi);
      last -= range_length + 1;
    }
    std::reverse(f.missing.begin(), f.missing.end());
    std::string err;
    const size_t n = ParseRevivedPackets(buf + o, len - o, ll, &f.revived, &err);
    if (n == 0) {
      *detailed_error = err;
      return 0;
    }
    std::reverse(f.revived.begin(), f.revived.end());  // (written newest first)
    o += n;
  }
  *out = f;
  return o;
}

FrameScanStatus ScanFrames(const uint8_t* body, size_t len, int quic_version,
                           QuicPacketNumber packet_number, size_t packet_number_length,
                           size_t max_frames, std::vector<ScannedFrame>* walked) {
  static const size_t kLengths[4] = {1, 2, 4, 6};
  walked->clear();
  if (len == 0) return kFrmNoFrames;
  size_t o = 0;
  // CanRead(n) of the reader at o
  const auto can = [&](size_t n) { return len - o >= n; };
  const auto get = [&](size_t n) {
    const uint64_t v = GetNumber(body + o, n);
    o += n;
    return v;
  };
  while (o < len) {
    if (walked->size() == max_frames) return kFrmTooMany;
    const size_t at = o;
    const uint8_t t = body[o++];
    ScannedFrame f;
    if (t & 0x80) {  // ProcessStreamFrame: 1 fin len ooo ss
      const size_t id_len = (t & 3) + 1, off_bits = (t >> 2) & 7;
      const size_t off_len = off_bits ? off_bits + 1 : 0;
      const bool has_len = (t & 0x20) != 0;
      if (!can(id_len + off_len + (has_len ? 2 : 0))) return kFrmStream;
      f.type = kFrameTypeStream;
      f.flags = static_cast<uint8_t>(((t & 0x40) ? 1 : 0) | (has_len ? 2 : 0));
      f.id = static_cast<uint32_t>(get(id_len));
      f.val = get(off_len);
      const size_t n = has_len ? static_cast<size_t>(get(2)) : len - o;
      if (!can(n)) return kFrmStream;
      f.off = static_cast<uint32_t>(o);
      f.len = static_cast<uint16_t>(n);
      o += n;
    } else if (t & 0x40) {  // ProcessAckFrame, stepped over
      const size_t mm = kLengths[t & 3], ll = kLengths[(t >> 2) & 3];
      if (!can(1 + ll + 2)) return kFrmAck;
      f.type = kFrameTypeAck;
      f.flags = t & 0x3F;
      f.code = static_cast<uint32_t>(get(1));
      f.val = get(ll);
      o += 2;
      if (!(t & 0x10)) {  // ProcessTimestampsInAckFrame
        if (!can(1)) return kFrmAck;
        const size_t n = static_cast<size_t>(get(1));
        const size_t bytes = n ? 5 + (n - 1) * 3 : 0;
        if (!can(bytes)) return kFrmAck;
        o += bytes;
      }
      if (t & 0x20) {
        if (!can(1)) return kFrmAck;
        const size_t ranges = static_cast<size_t>(get(1)) * (mm + 1);
        if (!can(ranges)) return kFrmAck;
        o += ranges;
        if (quic_version <= 31) {
          if (!can(1)) return kFrmAck;
          const size_t revived = static_cast<size_t>(get(1)) * ll;
          if (!can(revived)) return kFrmAck;
          o += revived;
        }
      }
      f.off = static_cast<uint32_t>(at);
      f.len = static_cast<uint16_t>(o - at);
    } else if (t & 0x20) {
      return kFrmIllegalType;
    } else {
      f.type = t;
      switch (t) {
        case 0:  // PADDING: the rest of the packet
          f.off = static_cast<uint32_t>(o);
          f.len = static_cast<uint16_t>(len - o);
          o = len;
          break;
        case 1:  // RST_STREAM
          if (!can(16)) return kFrmRst;
          f.id = static_cast<uint32_t>(get(4));
          f.val = get(8);
          f.code = static_cast<uint32_t>(get(4));
          break;
        case 2:    // CONNECTION_CLOSE
        case 3: {  // GOAWAY
          const FrameScanStatus bad = t == 2 ? kFrmClose : kFrmGoaway;
          if (!can(t == 2 ? 6 : 10)) return bad;
          f.code = static_cast<uint32_t>(get(4));
          if (t == 3) f.id = static_cast<uint32_t>(get(4));
          const size_t n = static_cast<size_t>(get(2));
          if (!can(n)) return bad;
          f.off = static_cast<uint32_t>(o);
          f.len = static_cast<uint16_t>(n);
          o += n;
          break;
        }
        case 4:  // WINDOW_UPDATE
          if (!can(12)) return kFrmWindowUpdate;
          f.id = static_cast<uint32_t>(get(4));
          f.val = get(8);
          break;
        case 5:  // BLOCKED
          if (!can(4)) return kFrmBlocked;
          f.id = static_cast<uint32_t>(get(4));
          break;
        case 6: {  // STOP_WAITING (the entropy byte: every version up to 33)
          if (!can(1 + packet_number_length)) return kFrmStopWaiting;
          f.code = static_cast<uint32_t>(get(1));
          const uint64_t delta = get(packet_number_length);
          if (delta > packet_number) return kFrmBadLeast;
          f.val = packet_number - delta;
          break;
        }
        case 7:  // PING
          break;
        case 8:  // PATH_CLOSE
          if (!can(1)) return kFrmPathClose;
          f.id = static_cast<uint32_t>(get(1));
          break;
        default:
          return kFrmIllegalType;
      }
    }
    walked->push_back(f);
  }
  return kFrmOk;
}

size_t SerializeFecPacketBody(QuicPacketNumber packet_number, QuicFecGroupNumber fec_group,
                              bool entropy_flag, StringPiece redundancy, uint8_t* buf,
                              size_t cap) {
  if (fec_group == 0 || fec_group > packet_number || packet_number - fec_group > 255) return 0;
  if (redundancy.size() > kMaxPacketSize) return 0;
  FecHeaderFields f;
  f.entropy_flag = entropy_flag;
  f.fec_flag = true;
  f.in_fec_group = true;
  f.fec_group_offset = static_cast<uint8_t>(packet_number - fec_group);
  const size_t h = WriteFecPrivateHeader(f, buf, cap);
  if (h == 0 || cap - h < redundancy.size()) return 0;
  std::memcpy(buf + h, redundancy.data(), redundancy.size());
  return h + redundancy.size();
}

}  // namespace net
