// C entry points over the reference's own QuicReceivedPacketManager, for
// tests/golden/make_golden_ack.py: a packet goes through IsAwaitingPacket and
// RecordPacketReceived as QuicConnection::ProcessValidatedPacket sends it, a
// STOP_WAITING through UpdatePacketInformationSentByPeer, and an ack comes out
// of GetUpdatedAckFrame.  Nothing of the manager is restated here.
#include <stdint.h>

#include "net/quic/core/quic_connection_stats.h"
#include "net/quic/core/quic_protocol.h"
#include "net/quic/core/quic_received_packet_manager.h"

namespace {
struct Receiver {
  net::QuicConnectionStats stats;
  net::QuicReceivedPacketManager manager;
  uint64_t clock_us = 1;
  Receiver() : manager(&stats) { manager.SetVersion(net::QUIC_VERSION_31); }
  net::QuicTime now() {
    return net::QuicTime::Zero() + net::QuicTime::Delta::FromMicroseconds(clock_us++);
  }
};
}  // namespace

#define ACKREF_API extern "C" __attribute__((visibility("default")))

ACKREF_API void* ackref_new() { return new Receiver; }
ACKREF_API void ackref_free(void* r) { delete static_cast<Receiver*>(r); }

// 1: the packet was awaited and is recorded; 0: dropped (a duplicate, or old)
ACKREF_API int ackref_receive(void* r, uint64_t packet_number, int entropy_flag) {
  Receiver* rc = static_cast<Receiver*>(r);
  if (!rc->manager.IsAwaitingPacket(packet_number)) return 0;
  net::QuicPacketHeader header;
  header.packet_number = packet_number;
  header.entropy_flag = entropy_flag != 0;
  // QuicFramer::GetPacketEntropyHash
  header.entropy_hash = static_cast<uint8_t>((entropy_flag != 0) << (packet_number % 8));
  rc->manager.RecordPacketReceived(1200, header, rc->now());
  return 1;
}

ACKREF_API void ackref_stop_waiting(void* r, uint64_t least_unacked, uint8_t entropy_hash) {
  net::QuicStopWaitingFrame frame;
  frame.least_unacked = least_unacked;
  frame.entropy_hash = entropy_hash;
  static_cast<Receiver*>(r)->manager.UpdatePacketInformationSentByPeer(frame);
}

// The ack as the manager hands it to the framer; returns the number of missing
// intervals (all of them; the first `cap` are stored, half-open).
ACKREF_API int ackref_ack(void* r, uint64_t* largest_observed, uint8_t* entropy_hash,
                          uint64_t* lo, uint64_t* hi, int cap) {
  Receiver* rc = static_cast<Receiver*>(r);
  const net::QuicFrame frame = rc->manager.GetUpdatedAckFrame(rc->now());
  const net::QuicAckFrame& ack = *frame.ack_frame;
  *largest_observed = ack.largest_observed;
  *entropy_hash = ack.entropy_hash;
  int n = 0;
  for (auto it = ack.packets.begin(); it != ack.packets.end(); ++it, ++n) {
    if (n < cap) {
      lo[n] = it->min();
      hi[n] = it->max();
    }
  }
  return n;
}
