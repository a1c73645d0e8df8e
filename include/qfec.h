/*
 * qfec.h — C-ABI of the MI355X-native QUIC forward-error-correction path.
 *
 * The boundary replaces libquic's FEC group (XOR parity encode + single-packet
 * revive).  The reference's implementation is absent from the snapshot
 * (/root/reference/Makefile:5332-5384 still lists the removed
 * src/net/quic/quic_fec_group.cc and quic_fec_group_interface.cc;
 * src/net/quic/core/quic_protocol.h:373 "FEC related fields are removed from
 * wire format"), so each entry point cites the historical member it replaces
 * and the in-tree hook site that called it:
 *
 *   qfec_encode_batch / _strided / qfec_encode_ragged
 *       replaces QuicFecGroup::UpdateParity + QuicFecGroupInterface::XorBuffers
 *       over every data packet of a group, then QuicFecGroup::PayloadParity().
 *       Send-side hook: QuicPacketCreator::SerializePacket between
 *       QuicFramer::BuildDataPacket and EncryptInPlace
 *       (src/net/quic/core/quic_packet_creator.cc:517-563, :530, :549).
 *   qfec_accumulate_ragged
 *       is UpdateParity's per-turn form: the packets at hand folded into one
 *       running row per open group (on a receiver Update / UpdateFec as well:
 *       the row is then what Revive() copies out).
 *   qfec_emit_accumulated / qfec_revive_accumulated
 *       close such rows: PayloadParity() hands the finished row to the FEC
 *       packet; NumMissingPackets() + CanRevive() + Revive() decide from the
 *       receive map and copy the row out as the revived packet.
 *   qfec_admit_ragged / qfec_revive_tracked
 *       keep that receive map (the group's received_packets_) on the device:
 *       Update()'s duplicate check and the drop of a packet that failed to
 *       decrypt, before the fold; the close then reads the map by slot.
 *   qfec_bin_arrivals
 *       is QuicConnection::GetFecGroup handing each arriving packet to its
 *       group (the receive path at quic_connection.cc:1388-1392), for a whole
 *       turn: per-packet records in arrival order become the per-slot CSR
 *       tables the admit reads.
 *   qfec_assign_slots
 *       is the lookup inside that same GetFecGroup: group_map_ searched for
 *       the packet's group and a new group inserted when there is none
 *       (quic_connection.cc:1388-1392), for a whole turn: per-packet 64-bit
 *       group keys become the per-packet slots the bin reads.
 *   qfec_retire_groups
 *       is what bounds that map: QuicFecReceiver::CloseFecGroupsBefore (a
 *       STOP_WAITING's threshold drops every group waiting for a packet below
 *       it, for good) and GetFecGroup's kMaxFecGroups eviction, for a whole
 *       turn in front of the assign: per-connection watermarks.
 *   qfec_parse_opened / qfec_write_private_headers
 *       are QuicFramer::ProcessAuthenticatedHeader (quic_framer.cc:1102-1141,
 *       run over the DECRYPTED buffer: the private flags and the FEC group
 *       offset byte are encrypted) and its writer, for a whole turn: the
 *       opened packets' first bytes become the keys, positions and body
 *       tables the calls above read.
 *   qfec_scan_frames
 *       is QuicFramer::ProcessFrameData (quic_framer.cc:1168-1342) and
 *       QuicConnection's STOP_WAITING bookkeeping, for a whole turn behind the
 *       parse: a table of the turn's frames, and per connection the newest
 *       STOP_WAITING, which the retire and the record take as their raises.
 *   qfec_record_received / qfec_build_acks
 *       are QuicReceivedPacketManager with its EntropyTracker
 *       (RecordPacketReceived, the patch's RecordPacketRevived,
 *       UpdatePacketInformationSentByPeer; GetUpdatedAckFrame and EntropyHash),
 *       for a whole turn behind the revive: the parse's verdicts and entropy
 *       bits and the revive's results become the ack frames' content.
 *   qfec_write_ack_frames
 *       is QuicFramer::AppendAckFrameAndTypeByte (v<=31, with the patch's
 *       revived tail) over the built acks: the frames' wire bytes, where the
 *       seal reads them.
 *   qfec_recover_batch / _strided / qfec_recover_ragged
 *       replaces QuicFecGroup::UpdateFec + Update(received) + CanRevive() +
 *       Revive().  Receive-side hook: QuicConnection::ProcessValidatedPacket
 *       "Drop any FEC packet." (src/net/quic/core/quic_connection.cc:1388-1392).
 *   qfec_xor_into
 *       replaces QuicFecGroupInterface::XorBuffers(input, size, output).
 *
 * Semantics: parity[j] = XOR over packets with
 * j < len_i of p_i[j]; parity_len = max len_i (zero padding, PADDING_FRAME = 0,
 * quic_protocol.h:259; quic_data_writer.cc:136-143).  Revive output is
 * parity_len bytes; bytes past the lost packet's own length are 0 and parse as
 * one PADDING frame (quic_framer.cc:1224-1231).
 *
 * Errors mirror the framer's bool + RaiseError(code) + detailed string
 * (quic_framer.cc:1128-1135): every call returns 0 on success or a negative
 * QuicErrorCode (quic_protocol.h:530-550); qfec_last_error() returns the
 * detailed string.  Nothing aborts.
 *
 * Ownership mirrors the reference's caller-owned ALIGNAS(64) packet buffers
 * (quic_framer.cc:573, quic_packet_creator.cc:351,401) and non-owning
 * StringPiece views: every buffer is borrowed for the duration of the call
 * (device-pointer calls: until the work queued on the context stream has
 * completed — see qfec_sync).  The context owns its device scratch, pinned
 * staging and streams; the library never frees caller memory.
 *
 * Threading: the reference connection is single-threaded
 * (quic_connection.h:14 "this class is not thread-safe"); a qfec_ctx is
 * likewise thread-compatible — one context per host thread / device, no global
 * locks on the hot path.
 */
#ifndef QFEC_H_
#define QFEC_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define QFEC_ABI_VERSION 1

/* Limits (quic_protocol.h:56, :66; quic_framer.cc:1126-1136). */
#define QFEC_DEFAULT_MAX_PACKET_SIZE 1350u /* kDefaultMaxPacketSize */
#define QFEC_MAX_PACKET_SIZE 1452u         /* kMaxPacketSize */
#define QFEC_MAX_GROUP_PACKETS 255u        /* uint8 first_fec_protected_packet_offset */

/* Return codes: 0 or -QuicErrorCode (quic_protocol.h). */
#define QFEC_OK 0
#define QFEC_ERR_INTERNAL (-1)         /* -QUIC_INTERNAL_ERROR: HIP failure, bad ctx */
#define QFEC_ERR_INVALID_FEC_DATA (-5) /* -QUIC_INVALID_FEC_DATA */

/* flags */
#define QFEC_PTR_DEVICE 0u  /* all buffer arguments are device pointers (default) */
#define QFEC_PTR_HOST 1u    /* all buffer arguments are host pointers: the call
                               stages through the context (pinned, chunked,
                               overlapped H2D / kernel / D2H) and returns when the
                               results are back in host memory */
#define QFEC_CACHED 2u      /* fixed-shape device calls: use the default cache
                               policy instead of non-temporal (nt) loads and
                               stores — for small batches whose output is
                               consumed straight away from L2 / MALL */
#define QFEC_PTR_MAPPED 4u  /* FEC calls (fixed, ragged, xor_into): the payload
                               buffers (rows / bytes, parity, parity_out / out) are
                               pinned, device-mapped host memory (qfec_host_alloc,
                               qfec_host_register, or any hipHostMalloc'd memory) that the
                               kernels read and write IN PLACE over PCIe — no
                               staging copy, the packets cross the link once; the
                               index arrays (pkt_off, pkt_len, grp_ptr, parity_off,
                               parity_len, missing_idx, out_off, parity_len_out)
                               are ordinary host memory, staged by the call.
                               Returns when the results are in host memory. */
#define QFEC_ONE_PASS 8u    /* fixed-shape device calls: always the one-pass
                               kernel.  Without it a large nt batch (>= 6 phases,
                               about 184K groups at L = 1350 on 256 CUs) runs the
                               phased kernel: one workgroup per CU, reads and
                               parity writes in separate grid-wide phases, which
                               keeps its rate independent of where the buffers
                               sit in the DRAM.  Same results either way. */
#define QFEC_ASYNC 16u      /* with QFEC_PTR_MAPPED, ragged calls: return as soon
                               as the work is queued (index arrays staged, kernel
                               launched) instead of when it is done; the outputs
                               (payload bytes and parity_len_out) are valid once
                               qfec_complete() has returned QFEC_OK, and every
                               buffer stays borrowed until then.  A batch whose
                               index tables exceed one staging slot (64 MiB) runs
                               synchronously.  Up to 3 calls may be in flight on
                               a context; any other call that stages through the
                               context completes them first.  Ignored by other
                               calls.  (The event-loop form: launch the turn's
                               FEC work, serve sockets, complete it next turn.) */
#define QFEC_SCRATCH_OUTPUT 32u /* decrypt / open calls (NULL, ChaCha20-Poly1305,
                               AES-128-GCM-12; device pointers): the output of a
                               packet whose tag fails may hold its unverified
                               plaintext (ok[p] = 0 still), so the kernel reads
                               the ciphertext once (hash and copy together)
                               instead of twice.  QuicFramer::DecryptPayload
                               decrypts into a scratch buffer, retries the
                               alternative decrypter into the same buffer and
                               drops the packet on failure
                               (quic_framer.cc:1884-1930), so this is a drop-in
                               for that caller; without the flag the output is
                               untouched on failure, as NullDecrypter leaves it
                               (crypto/null_decrypter.cc:57-62). */
#define QFEC_SMALL_GROUPS 64u /* ragged device calls (round 6): a hint that the
                                * batch's groups carry few payload bytes each
                                * (under ~4 KiB on average: short packets or
                                * k <= 4), so a large batch runs two groups per
                                * wave instead of eight per block (+8-14% there,
                                * DESIGN.md §4 band table).  Host-pointer and
                                * mapped batches choose by themselves (the host
                                * holds their tables); results are identical. */

/* qfec_complete() with wait == 0: the QFEC_ASYNC work is still running. */
#define QFEC_PENDING 1

typedef struct qfec_ctx qfec_ctx;

/* ---- context ---------------------------------------------------------- */
/* Create a context bound to HIP device `device`.  NULL on failure (no device,
 * HIP error); the reason is then available from qfec_last_error(NULL). */
qfec_ctx* qfec_create(int device);
void qfec_destroy(qfec_ctx* ctx);
/* Use an existing hipStream_t (e.g. torch's current stream) for device-pointer
 * calls; NULL is HIP's null (default) stream, as in the HIP API.  A new
 * context uses a non-blocking stream of its own, returned by
 * qfec_own_stream() (pass it back to restore it). */
int qfec_set_stream(qfec_ctx* ctx, void* hip_stream);
void* qfec_get_stream(qfec_ctx* ctx);
void* qfec_own_stream(qfec_ctx* ctx);
/* Wait for all queued work; returns the first error latched by a kernel
 * (e.g. a missing index >= k or a ragged length > kMaxPacketSize found on the
 * device) since the previous qfec_sync, then clears it. */
int qfec_sync(qfec_ctx* ctx);
/* Finish the context's QFEC_ASYNC calls in issue order.  wait != 0 blocks
 * until all are done; wait == 0 returns QFEC_PENDING while one is still
 * running.  Returns the first error of the calls it finished (the same codes
 * the synchronous call would have returned), else QFEC_OK. */
int qfec_complete(qfec_ctx* ctx, int wait);
/* The ticket of the last ragged call on this context if it was queued
 * asynchronously (QFEC_ASYNC honoured), else 0. */
uint64_t qfec_async_ticket(const qfec_ctx* ctx);
/* Finish ONE queued op: wait blocks, otherwise QFEC_PENDING while it runs.
 * Returns that op's own code only (an op finished early by another call --
 * its staging slot reused, a synchronous call -- keeps its code for this);
 * QFEC_ERR_INTERNAL for an unknown or already claimed ticket.  The codes of
 * the last 4096 tickets stay claimable once each, also after qfec_complete
 * finished their ops (which reports an op's error once, to one of the two). */
int qfec_complete_ticket(qfec_ctx* ctx, uint64_t ticket, int wait);
/* Small-batch service hint (round 5; no counterpart in the reference): make
 * sure the context's resident worker runs.  An event loop that calls it when
 * a turn starts collecting groups finds the worker resident at the turn's
 * flush instead of relaunching it there (the worker leaves after 100 us
 * without work; a relaunch costs the calling thread 3-5 us and the flush
 * ~20 us).  One load when the worker runs; a no-op with the service off.
 * Returns a qfec_* code (a failed launch turns the service off for the
 * context, as a failed relaunch in a batch call does). */
int qfec_service_warm(qfec_ctx* ctx);
const char* qfec_strerror(int code);
/* Pinned, device-mapped host memory for QFEC_PTR_MAPPED payloads (the
 * registered receive / send buffers of a QUIC server: the GPU reads packets
 * where the socket wrote them).  NULL on failure (qfec_last_error(NULL)). */
void* qfec_host_alloc(size_t bytes);
void qfec_host_free(void* p);
/* Pin and device-map EXISTING host memory [p, p + bytes) for QFEC_PTR_MAPPED
 * calls (e.g. a server's recvmmsg ring allocated by the application), the
 * registration counterpart of qfec_host_alloc; the memory stays the caller's.
 * The GPU addresses it at the same virtual address as the host (the mapped
 * calls pass pointers through unchanged); a platform where that is not so is
 * refused (QFEC_ERR_INTERNAL).  Unregister before freeing the memory. */
int qfec_host_register(void* p, size_t bytes);
int qfec_host_unregister(void* p);
const char* qfec_last_error(const qfec_ctx* ctx);
int qfec_abi_version(void);

/* ---- fixed-shape batches ---------------------------------------------- */
/* rows:    n_groups x k x L bytes, group g row i at rows + g*k*L + i*L
 * parity:  n_groups x L bytes
 * Encode:  parity[g] = XOR_i rows[g][i]. */
int qfec_encode_batch(qfec_ctx* ctx, const uint8_t* rows, uint32_t k, uint32_t L,
                      uint64_t n_groups, uint8_t* parity_out, uint32_t flags);

/* Recover: out[g] = parity[g] XOR_{i != missing[g]} rows[g][i].
 * rows[g][missing[g]] is never read (the lost packet's slot).  missing[g] < k. */
int qfec_recover_batch(qfec_ctx* ctx, const uint8_t* rows, const uint8_t* parity,
                       const uint8_t* missing_idx, uint32_t k, uint32_t L, uint64_t n_groups,
                       uint8_t* out, uint32_t flags);

/* In-slot recover: the receiver has written the FEC packet's redundancy
 * (L bytes) into row missing_idx[g] of group g -- the slot of the lost packet,
 * where the framer would have put it -- so the lost packet is the XOR of the
 * group's k rows.  The kernels then read ONE contiguous stream of k rows per
 * group (qfec_recover_batch reads k-1 rows around the lost row's hole plus a
 * separate parity stream); the same 14,850 B per group at 10 x 1350 B.
 *   out != NULL: out[g] = XOR_i rows[g][i]; missing_idx is not read (may be
 *                NULL); the rows are not written.  Any pointer mode (flags).
 *   out == NULL: in place, rows[g][missing_idx[g]] receives the lost packet
 *                (missing_idx[g] < k, else -QUIC_INVALID_FEC_DATA as
 *                qfec_recover_batch); device pointers only.  Applying it twice
 *                restores the redundancy.
 * Replaces the same historical QuicFecGroup::UpdateFec + Revive as
 * qfec_recover_batch, at the receive hook QuicConnection::ProcessValidatedPacket
 * (src/net/quic/core/quic_connection.cc:1388-1392). */
int qfec_recover_inslot_batch(qfec_ctx* ctx, uint8_t* rows, const uint8_t* missing_idx, uint32_t k,
                              uint32_t L, uint64_t n_groups, uint8_t* out, uint32_t flags);

/* Strided forms (padding study: row_stride >= L, group_stride >= k*row_stride,
 * parity/out strides >= L; all in bytes). */
int qfec_encode_batch_strided(qfec_ctx* ctx, const uint8_t* rows, uint32_t k, uint32_t L,
                              uint64_t row_stride, uint64_t group_stride, uint64_t n_groups,
                              uint8_t* parity_out, uint64_t parity_stride, uint32_t flags);
int qfec_recover_batch_strided(qfec_ctx* ctx, const uint8_t* rows, const uint8_t* parity,
                               const uint8_t* missing_idx, uint32_t k, uint32_t L,
                               uint64_t row_stride, uint64_t group_stride,
                               uint64_t parity_stride, uint64_t n_groups, uint8_t* out,
                               uint64_t out_stride, uint32_t flags);
int qfec_recover_inslot_batch_strided(qfec_ctx* ctx, uint8_t* rows, const uint8_t* missing_idx,
                                      uint32_t k, uint32_t L, uint64_t row_stride,
                                      uint64_t group_stride, uint64_t n_groups, uint8_t* out,
                                      uint64_t out_stride, uint32_t flags);

/* ---- revive from receive maps ------------------------------------------- */
/* The receiver's decision and the revive in one call, for a batch that stays
 * on the device: which groups are finished, which lost exactly one protected
 * packet and hold their FEC packet (those are rebuilt), which are beyond
 * repair.  Replaces QuicFecGroup::NumMissingPackets() + IsFinished() +
 * CanRevive() + Revive() over a batch of groups, at the receive hook
 * QuicConnection::ProcessValidatedPacket
 * (src/net/quic/core/quic_connection.cc:1388-1392); the recover calls above
 * take that decision as an input (missing_idx) and read every group.
 *
 * received: one receive map per group, map_stride bytes apart
 *   (map_stride >= ceil((k + 1) / 8); the dense form uses exactly that).  Bit i
 *   of a map is (map[i / 8] >> (i % 8)) & 1: bits 0 .. k-1 say whether data
 *   packet i arrived, bit k whether the FEC packet arrived; bits above k in
 *   the last byte are ignored.  rows / parity: as qfec_recover_batch.
 * With miss = k - popcount(data bits):
 *   miss == 0                      QFEC_GROUP_COMPLETE, whatever the FEC bit
 *   miss == 1 and the FEC bit set  QFEC_GROUP_REVIVED, m = the clear data bit
 *   anything else                  QFEC_GROUP_UNREVIVABLE
 * An unrevivable group is a result, not an error (as an invalid ack is for
 * qfec_entropy_validate_batch).
 *
 * Outputs (status is required, every other one may be NULL):
 *   status[g]        one of the three codes
 *   revived_idx[g]   m for revived groups, 0xFF otherwise
 *   out != NULL:     out + g*out_stride receives the L revived bytes of revived
 *                    groups only, parity[g] XOR_{i != m} rows[g][i]; the out
 *                    rows of other groups are not written
 *   out == NULL:     in place, rows[g][m] receives the revived packet; no other
 *                    byte of rows is written
 *   revived_list     room for n_groups entries: the indices of the revived
 *                    groups in ascending order (what the framer walks for the
 *                    ack's revived packets); entries from the count on are not
 *                    written
 *   counts[0..2]     groups per status; counts[1] is the length of the list
 * Reads: the slot of a missing packet and the parity row of a group without
 * its FEC packet are never read; rows and parity of complete and unrevivable
 * groups are not read at all -- a batch with 5% of its groups to revive moves
 * about 5% of the dense recover's bytes plus the maps.
 *
 * Device pointers only (QFEC_PTR_HOST, QFEC_PTR_MAPPED and QFEC_ASYNC are
 * refused); QFEC_CACHED as for the fixed-shape calls.  The call queues its
 * kernels on the context's stream and returns: it never waits for the device
 * and never reads the revived count back; results are valid after qfec_sync.
 * Its intermediate state (per-workgroup counts, the packed list of revivable
 * groups) lives in context-owned device scratch, grown on demand (an
 * outgrown block is released by the next qfec_sync, so growing does not wait
 * either) and freed by qfec_destroy.
 * Limits and codes as qfec_recover_batch_strided (1 <= k <= 255,
 * 1 <= L <= 1452, strides >= L, else -QUIC_INVALID_FEC_DATA), and the same
 * code for a map_stride below ceil((k + 1) / 8); a NULL rows, parity (even if
 * no group would read it), received or status and the refused pointer flags
 * return QFEC_ERR_INTERNAL.  A refused call launches nothing and writes
 * nothing.  n_groups == 0 succeeds (counts, if given, receives three
 * zeroes) and, as for qfec_recover_batch, is decided before the buffers are
 * looked at: NULL buffers pass with it. */
#define QFEC_GROUP_COMPLETE 0u    /* every data packet arrived (IsFinished): nothing to do */
#define QFEC_GROUP_REVIVED 1u     /* one data packet missing, FEC packet present (CanRevive): rebuilt */
#define QFEC_GROUP_UNREVIVABLE 2u /* two or more data packets missing, or one missing and no FEC packet */
int qfec_revive_batch(qfec_ctx* ctx, uint8_t* rows, const uint8_t* parity, const uint8_t* received,
                      uint32_t k, uint32_t L, uint64_t n_groups, uint8_t* out, uint8_t* status,
                      uint8_t* revived_idx, uint64_t* revived_list, uint64_t* counts,
                      uint32_t flags);
int qfec_revive_batch_strided(qfec_ctx* ctx, uint8_t* rows, const uint8_t* parity,
                              const uint8_t* received, uint32_t k, uint32_t L,
                              uint64_t row_stride, uint64_t group_stride,
                              uint64_t parity_stride, uint64_t map_stride, uint64_t n_groups,
                              uint8_t* out, uint64_t out_stride, uint8_t* status,
                              uint8_t* revived_idx, uint64_t* revived_list, uint64_t* counts,
                              uint32_t flags);

/* ---- ragged batches (CSR) ---------------------------------------------- */
/* Group g holds packets p in [grp_ptr[g], grp_ptr[g+1]) (1..255 of them);
 * packet p is pkt_len[p] (1..1452) bytes at bytes + pkt_off[p].
 * Encode writes parity_len_out[g] = max len and that many parity bytes at
 * parity_out + parity_off[g]. */
int qfec_encode_ragged(qfec_ctx* ctx, const uint8_t* bytes, const uint64_t* pkt_off,
                       const uint16_t* pkt_len, const uint32_t* grp_ptr, uint64_t n_groups,
                       uint8_t* parity_out, const uint64_t* parity_off,
                       uint16_t* parity_len_out, uint32_t flags);
/* Recover writes parity_len[g] bytes at out + out_off[g]:
 * parity XOR every received packet of the group (zero padded).  The lost
 * packet's pkt_off / pkt_len entries (index grp_ptr[g] + missing_idx[g]) are
 * never read.  Every received packet must satisfy len <= parity_len[g]. */
int qfec_recover_ragged(qfec_ctx* ctx, const uint8_t* bytes, const uint64_t* pkt_off,
                        const uint16_t* pkt_len, const uint32_t* grp_ptr, uint64_t n_groups,
                        const uint8_t* parity, const uint64_t* parity_off,
                        const uint16_t* parity_len, const uint8_t* missing_idx, uint8_t* out,
                        const uint64_t* out_off, uint32_t flags);
/* qfec_revive_batch for a ragged batch: the receiver's decision and the revive
 * in one call, with k per group from grp_ptr.  bytes .. parity_len, out and
 * out_off are exactly as for qfec_recover_ragged; group g has
 * k_g = grp_ptr[g+1] - grp_ptr[g] packets, its slot i is packet grp_ptr[g] + i.
 * received: the map of group g is map_stride bytes at received + g*map_stride,
 *   bits as for qfec_revive_batch: bits 0 .. k_g-1 the data packets, bit k_g
 *   the FEC packet, higher bits ignored.  map_stride is one value for the
 *   batch (32 holds any legal group, 2 every group of k <= 15).
 * The rule, the three QFEC_GROUP_* codes and status (required), revived_idx,
 * revived_list and counts (each may be NULL) are those of qfec_revive_batch:
 * revived_idx is 0xFF for groups not revived, revived_list is ascending and
 * not written from the count on, counts[1] is its length.
 * A revived group receives parity_len[g] bytes at out + out_off[g]: the parity
 * XOR every received packet, zero padded -- byte for byte what
 * qfec_recover_ragged writes for it with missing_idx[g] = m.  There is no
 * in-place form (a lost ragged packet has no slot of its own): out and out_off
 * are required.
 * Never read: the pkt_off / pkt_len entries of a revived group's lost packet;
 * every pkt_off, pkt_len, parity_off, parity_len and out_off entry and every
 * payload and parity byte of a complete or unrevivable group; the map of an
 * invalid group (below).  Never written: out bytes of groups not revived, and
 * out bytes outside [out_off[g], out_off[g] + parity_len[g]) of revived ones.
 * Latched on the device and returned by the next qfec_sync as
 * -QUIC_INVALID_FEC_DATA: a group with k_g = 0, k_g > 255 (a grp_ptr that is
 * not monotone shows up as that) or k_g / 8 + 1 > map_stride -- it gets status
 * QFEC_GROUP_UNREVIVABLE and revived_idx 0xFF and is counted as unrevivable;
 * and, for a revived group, a bad parity_len or a received pkt_len of 0 or
 * above parity_len[g], exactly as qfec_recover_ragged latches them -- its
 * status stays QFEC_GROUP_REVIVED (the status states the map), its out bytes
 * are unspecified, and every other group's outputs are right.
 * Refused on the host (nothing launched, nothing written): map_stride == 0
 * (-QUIC_INVALID_FEC_DATA); QFEC_PTR_HOST, QFEC_PTR_MAPPED or QFEC_ASYNC; a
 * NULL required buffer; n_groups >= 2^32, packet indices being 32 bits
 * (QFEC_ERR_INTERNAL).  n_groups == 0 succeeds before the buffers are looked
 * at (counts, if given, receives three zeroes).  QFEC_CACHED and
 * QFEC_SMALL_GROUPS are accepted and change nothing: the ragged device kernels
 * are nontemporal only, and one body (eight list entries per 4-wave block) is
 * built.  Like qfec_revive_batch the call only queues kernels on the
 * context's stream, never waits, never reads the revived count back, and uses
 * the same context-owned scratch. */
int qfec_revive_ragged(qfec_ctx* ctx, const uint8_t* bytes, const uint64_t* pkt_off,
                       const uint16_t* pkt_len, const uint32_t* grp_ptr, uint64_t n_groups,
                       const uint8_t* parity, const uint64_t* parity_off,
                       const uint16_t* parity_len, const uint8_t* received, uint64_t map_stride,
                       uint8_t* out, const uint64_t* out_off, uint8_t* status,
                       uint8_t* revived_idx, uint64_t* revived_list, uint64_t* counts,
                       uint32_t flags);

/* The running accumulator of QuicFecGroup::UpdateParity (and, on a receiver,
 * Update / UpdateFec), batched: fold this turn's packets of every open group
 * into one row per group, so the packets' buffers can be recycled before the
 * group closes.  bytes, pkt_off, pkt_len and grp_ptr are the CSR tables of
 * qfec_encode_ragged and list, per group, the packets to fold NOW: data
 * packets and, on a receiver, the FEC packet's redundancy (just another
 * packet).  Group g folds into accumulator s = slot[g] (slot == NULL: s = g,
 * lockstep batches): the row acc + s * acc_stride, its length acc_len[s] read
 * on entry and written on exit.
 * The rule, per group, with old = acc_len[s] and
 * new = max(old, max pkt_len of the group's packets):
 *   for j < new: acc[s][j] = (j < old ? acc[s][j] : 0)
 *                            XOR (XOR over this turn's packets with j < len_i of p_i[j]);
 *   acc_len[s] = new.
 * Row bytes at or beyond old count as zero whatever they hold: acc_len[s] == 0
 * is a fresh slot and needs no clearing.  A sender's row is the FEC packet's
 * redundancy (qfec_encode_ragged's parity and length) once the group's packets
 * have been folded; a receiver's row is the revived packet
 * (qfec_recover_ragged's output, length parity_len) once the k-1 received data
 * packets and the redundancy have been folded -- in any order, over any number
 * of calls.
 * A group with no packets this turn (k_g = 0) is valid and a no-op: its row
 * and length keep their values.
 * Never read: a row whose old length is 0; row bytes at or beyond old; rows and
 * lengths of slots that no group names.  Never written: row bytes at or beyond
 * new; rows and lengths of slots that no group names.
 * The caller guarantees, unchecked: the slots named in one call are distinct
 * (results for a slot named twice are unspecified), and no acc row overlaps
 * bytes.
 * Latched on the device and returned by the next qfec_sync as
 * -QUIC_INVALID_FEC_DATA: k_g > 255 (a grp_ptr that is not monotone shows up
 * as that); slot[g] >= n_slots (its acc_len is then not read);
 * acc_len[s] > min(1452, acc_stride); a pkt_len of 0 or above
 * min(1452, acc_stride).  The offending group's row and length are left
 * untouched and every other group's outputs are right.
 * Refused on the host (nothing launched, nothing written): acc_stride == 0
 * (-QUIC_INVALID_FEC_DATA); QFEC_PTR_HOST, QFEC_PTR_MAPPED or QFEC_ASYNC; a
 * NULL bytes, pkt_off, pkt_len, grp_ptr, acc or acc_len; n_groups >= 2^32 or
 * n_slots >= 2^32; slot == NULL with n_slots < n_groups (QFEC_ERR_INTERNAL).
 * n_groups == 0 succeeds before the buffers are looked at.  QFEC_CACHED and
 * QFEC_SMALL_GROUPS are accepted and change nothing.  Device pointers only; the
 * call only queues kernels on the context's stream, never waits and never
 * reads anything back; results are valid after qfec_sync, and two calls queued
 * back to back on one stream see each other's rows (turn t+1 reads what turn
 * t wrote). */
int qfec_accumulate_ragged(qfec_ctx* ctx, const uint8_t* bytes, const uint64_t* pkt_off,
                           const uint16_t* pkt_len, const uint32_t* grp_ptr, uint64_t n_groups,
                           uint8_t* acc, uint64_t acc_stride, uint16_t* acc_len,
                           const uint32_t* slot, uint64_t n_slots, uint32_t flags);

/* Close running rows: the two exits of qfec_accumulate_ragged.  In both,
 * group g's row is acc + s * acc_stride with s = slot[g] (slot == NULL: s = g),
 * len = acc_len[s] and lim = min(1452, acc_stride), exactly as
 * qfec_accumulate_ragged states them.
 *
 * qfec_emit_accumulated is the sender's PayloadParity(), or any "hand me these
 * rows".  For every group: out_len[g] = len, and len bytes of the row are
 * copied to out + out_off[g] at any byte alignment (the FEC packet's body
 * behind its private header).  len == 0 is valid and copies nothing.
 * release != 0 then sets acc_len[s] = 0: the slot is fresh for the next
 * qfec_accumulate_ragged.
 *
 * qfec_revive_accumulated is the receiver's NumMissingPackets() / CanRevive()
 * / Revive(), after which the group is deleted.  group_k[g] is the number of
 * protected packets (1..255); the map of group g is map_stride bytes at
 * received + g * map_stride, its bits, the rule and the three QFEC_GROUP_*
 * codes those of qfec_revive_ragged -- the map says which packets HAVE BEEN
 * FOLDED into the row.  status is required; revived_idx, revived_list
 * (ascending, not written from the count on) and counts behave as in
 * qfec_revive_ragged.  A QFEC_GROUP_REVIVED group gets out_len[g] = len and
 * len bytes of the row at out + out_off[g]: byte for byte what
 * qfec_recover_ragged writes for the group from its payloads.  out == NULL is
 * allowed: the revived packet then IS the row, nothing is copied, out_off is
 * not read and out_len is still written.  Every other group gets
 * out_len[g] = 0, nothing copied, and its out_off entry is never read.
 * release_mask: bit st set = groups whose status is st get acc_len[s] = 0
 * (0b011 closes finished and revived groups and leaves unrevivable ones open
 * for later packets, 0b111 closes all, 0 none).
 *
 * Never read: rows and lengths of slots no group names; row bytes at or beyond
 * len; rows of groups that are not copied; the map of an invalid group.  Never
 * written: acc rows, ever; acc_len of slots that are not released; out bytes
 * outside [out_off[g], out_off[g] + len) of copied groups.
 * The caller guarantees, unchecked: the slots named in one call are distinct,
 * out does not overlap acc, and out ranges do not overlap each other.
 * Latched on the device and returned by the next qfec_sync as
 * -QUIC_INVALID_FEC_DATA: slot[g] >= n_slots (its acc_len is not read);
 * group_k[g] == 0 or group_k[g] / 8 + 1 > map_stride; a group to copy with
 * len > lim; a revived group with len == 0 (the map claims folds the row never
 * saw).  A group with a bad slot or a bad group_k has status
 * QFEC_GROUP_UNREVIVABLE and revived_idx 0xFF and is counted as unrevivable;
 * a revived group with a bad length keeps its status, its place in
 * revived_list and its count (the status states the map).  Every offending
 * group gets out_len[g] = 0, nothing copied and no release; every other
 * group's outputs are right.
 * Refused on the host (nothing launched, nothing written): acc_stride == 0 or
 * map_stride == 0 (-QUIC_INVALID_FEC_DATA); QFEC_PTR_HOST, QFEC_PTR_MAPPED or
 * QFEC_ASYNC; a NULL acc, acc_len or out_len, a NULL out_off when out is
 * given, for the emit a NULL out, for the revive a NULL group_k, received or
 * status; n_groups >= 2^32 or n_slots >= 2^32; slot == NULL with
 * n_slots < n_groups; release_mask > 7 (QFEC_ERR_INTERNAL).  n_groups == 0
 * succeeds before the buffers are looked at (counts, if given, receives three
 * zeroes).  QFEC_CACHED and QFEC_SMALL_GROUPS are accepted and change nothing.
 * Device pointers only; both calls only queue kernels on the context's stream,
 * never wait and never read anything back, and the revive uses the
 * context-owned scratch of qfec_revive_batch.  Queued behind a
 * qfec_accumulate_ragged on one stream they see its rows, and an accumulate
 * queued behind them sees the released slots as fresh. */
int qfec_emit_accumulated(qfec_ctx* ctx, const uint8_t* acc, uint64_t acc_stride,
                          uint16_t* acc_len, const uint32_t* slot, uint64_t n_slots,
                          uint64_t n_groups, uint8_t* out, const uint64_t* out_off,
                          uint16_t* out_len, int release, uint32_t flags);
int qfec_revive_accumulated(qfec_ctx* ctx, const uint8_t* acc, uint64_t acc_stride,
                            uint16_t* acc_len, const uint32_t* slot, uint64_t n_slots,
                            const uint8_t* group_k, const uint8_t* received, uint64_t map_stride,
                            uint64_t n_groups, uint8_t* out, const uint64_t* out_off,
                            uint16_t* out_len, uint8_t* status, uint8_t* revived_idx,
                            uint64_t* revived_list, uint64_t* counts, uint32_t release_mask,
                            uint32_t flags);

/* The group's received_packets_ set on the device: one running receive map per
 * SLOT, consulted before the fold and read by the close.  qfec_revive_accumulated
 * holds only while the host knows which packets were folded; it does not for a
 * packet opened on the device, whose verdict ok[p] lies in device memory
 * (QuicFramer::DecryptPayload drops a packet whose tag fails before the FEC
 * group sees it), nor for a duplicate (QuicFecGroup::Update returns false for
 * a packet number already in received_packets_; folded twice it cancels out of
 * the row).  A receiver's turn is open -> qfec_admit_ragged ->
 * qfec_accumulate_ragged -> qfec_revive_tracked on one stream, with no sync
 * and no host decision in between.  The position is the FEC group offset byte,
 * which lies in the encrypted part of the packet: qfec_parse_opened (below)
 * reads it on the device; the slot is the host's lookup, or qfec_assign_slots'
 * (below),
 * which also lists what then remains with the host.
 *
 * qfec_admit_ragged never reads a payload byte.  pkt_off, pkt_len and grp_ptr
 * list the turn's CANDIDATES per group as qfec_accumulate_ragged's tables do;
 * pkt_idx[p] is the candidate's position in its group (0 .. K-1 a data packet,
 * K the FEC packet) and pkt_ok[p] the open call's ok[p] (pkt_ok == NULL: all
 * verified).  With s = slot[g] (slot == NULL: s = g), K = slot_k[s] (protected
 * packets, 1..255) and lim = min(1452, acc_stride), the slot's map is the
 * first K / 8 + 1 bytes at acc_map + s * map_stride, bits as for
 * qfec_revive_ragged.
 * Fresh slot: if acc_len[s] == 0 the map counts as all clear whatever it holds
 * (as row bytes beyond old do for the accumulate), so a slot released by
 * qfec_revive_accumulated, qfec_revive_tracked or qfec_emit_accumulated needs
 * no clearing.  Otherwise base = the map's bits 0 .. K; higher bits are ignored.
 * The group's candidates are taken in CSR order (INVALID over FAILED over
 * DUPLICATE):
 *   pkt_idx[p] > K                          QFEC_PKT_INVALID (latched, below)
 *   pkt_len[p] == 0 or > lim                QFEC_PKT_INVALID (latched)
 *   pkt_ok given and pkt_ok[p] == 0         QFEC_PKT_FAILED, a result
 *   its bit set in base, or by an earlier
 *   candidate of this group in this call    QFEC_PKT_DUPLICATE, a result
 *   anything else                           QFEC_PKT_ADMITTED, and its bit is set
 * The first candidate of an index wins: deterministic, and nothing is sorted.
 * Outputs: verdict[p] for every candidate of a group with k_g <= 255;
 * grp_ptr_out[0] = 0 and grp_ptr_out[g+1] - grp_ptr_out[g] = the packets
 * admitted for g; pkt_off_out / pkt_len_out at grp_ptr_out[g] + r the r-th
 * admitted packet of g in CSR order -- the tables qfec_accumulate_ragged then
 * folds; entries from grp_ptr_out[n_groups] on are not written.  If g admitted
 * at least one packet its map's K / 8 + 1 bytes become base | new with zero
 * bits above K; otherwise no byte of its map is written.  Map bytes beyond
 * K / 8 + 1 and the maps of slots no group names are never read or written.
 * counts[0..3] (may be NULL): the verdicts written, per code.
 * Invalid group: each of its packets is QFEC_PKT_INVALID, none is admitted
 * and its map is untouched -- k_g > 255 (its verdicts are not written and not
 * counted: a grp_ptr that is not monotone shows up as that); s >= n_slots
 * (slot_k, acc_len and the map are then not read); K == 0 or
 * K / 8 + 1 > map_stride; acc_len[s] > lim.  These and the two invalid-packet
 * cases are latched on the device and returned by the next qfec_sync as
 * -QUIC_INVALID_FEC_DATA; every other group's outputs are right.
 * The caller guarantees, unchecked: the slots named in one call are distinct;
 * the output tables have room for grp_ptr[n_groups] - grp_ptr[0] entries (no
 * entry is written past that); each admit is followed on the same stream by a
 * qfec_accumulate_ragged over its output tables with the same slot, n_slots,
 * acc_stride and acc_len, before the next admit or close that names those
 * slots.  With that the accumulate cannot latch for an admitted group, and a
 * slot with a set bit has acc_len > 0.  A group with K = 255 whose 256 packets
 * all arrive in one turn needs two calls (k_g <= 255).
 * Refused on the host (nothing launched, nothing written): acc_stride == 0 or
 * map_stride == 0 (-QUIC_INVALID_FEC_DATA); QFEC_PTR_HOST, QFEC_PTR_MAPPED or
 * QFEC_ASYNC; a NULL buffer other than pkt_ok, slot and counts;
 * n_groups >= 2^32 or n_slots >= 2^32; slot == NULL with n_slots < n_groups
 * (QFEC_ERR_INTERNAL).  n_groups == 0 succeeds before the buffers are looked at
 * (counts, if given, receives four zeroes; grp_ptr_out is not written).
 * QFEC_CACHED and QFEC_SMALL_GROUPS are accepted and change nothing.  Device
 * pointers only; the call only queues kernels on the context's stream, never
 * waits and never reads anything back; its intermediate state (per-group and
 * per-tile counts, scanned offsets) lives in the context-owned scratch of
 * qfec_revive_batch.
 *
 * qfec_revive_tracked is qfec_revive_accumulated with two differences: K and
 * the map are read by slot, slot_k[s] and acc_map + s * map_stride, and a slot
 * with acc_len[s] == 0 counts as an all-clear map, so it is
 * QFEC_GROUP_UNREVIVABLE (a result, not an error; its map is not read) -- the
 * case "revived but length 0" cannot arise from a stale map.  For every group
 * whose slot is in range the outputs (status, revived_idx, revived_list,
 * counts, out_len, copied bytes, releases) are byte for byte what
 * qfec_revive_accumulated gives when handed group_k[g] = slot_k[slot[g]] and
 * the by-slot maps gathered by group, zeroed where the slot is fresh.  A slot
 * out of range is unrevivable and latched like there; its slot_k, map and
 * length are not read.  Refusals, out == NULL, release_mask and the "never
 * read / never written" lists are those of qfec_revive_accumulated (slot_k and
 * acc_map in the place of group_k and received). */
#define QFEC_PKT_ADMITTED 0u  /* to be folded: its bit was clear and is now set */
#define QFEC_PKT_FAILED 1u    /* pkt_ok[p] == 0: its protection did not verify */
#define QFEC_PKT_DUPLICATE 2u /* its bit was already set in the slot's map, or an
                                 earlier packet of this group in this call set it */
#define QFEC_PKT_INVALID 3u   /* bad index or length, or its group is invalid */
int qfec_admit_ragged(qfec_ctx* ctx, const uint64_t* pkt_off, const uint16_t* pkt_len,
                      const uint8_t* pkt_idx, const uint8_t* pkt_ok, const uint32_t* grp_ptr,
                      uint64_t n_groups, const uint32_t* slot, uint64_t n_slots,
                      const uint8_t* slot_k, uint8_t* acc_map, uint64_t map_stride,
                      const uint16_t* acc_len, uint64_t acc_stride, uint32_t* grp_ptr_out,
                      uint64_t* pkt_off_out, uint16_t* pkt_len_out, uint8_t* verdict,
                      uint64_t* counts, uint32_t flags);
int qfec_revive_tracked(qfec_ctx* ctx, const uint8_t* acc, uint64_t acc_stride, uint16_t* acc_len,
                        const uint8_t* acc_map, uint64_t map_stride, const uint8_t* slot_k,
                        const uint32_t* slot, uint64_t n_slots, uint64_t n_groups, uint8_t* out,
                        const uint64_t* out_off, uint16_t* out_len, uint8_t* status,
                        uint8_t* revived_idx, uint64_t* revived_list, uint64_t* counts,
                        uint32_t release_mask, uint32_t flags);

/* The turn's CSR tables built on the device: QuicConnection::GetFecGroup
 * handing each arriving packet to its group (the receive path at
 * quic_connection.cc:1388-1392), for a whole turn at once.  Sockets deliver
 * packets in arrival order, interleaved across connections and groups;
 * qfec_admit_ragged wants them listed per group.  What the host knows per
 * packet without grouping anything -- the slot its group holds, its position
 * in the group, where its plaintext will lie and how long it is -- goes to the
 * device as flat records in arrival order, and this call bins them by slot: a
 * stable counting sort.  The turn is open (in arrival order) ->
 * qfec_bin_arrivals -> qfec_admit_ragged -> qfec_accumulate_ragged ->
 * qfec_revive_tracked on one stream, with no sync and no host decision in
 * between.  The slots come from the host or from qfec_assign_slots (below);
 * the position is the FEC group offset byte, encrypted on the wire and read
 * from the opened packet by qfec_parse_opened (below), whose body_off_out,
 * body_len_out and pkt_idx_out this call takes as pkt_off, pkt_len and pkt_idx.
 *
 * Inputs, n_packets records in arrival order: pkt_slot[p] the slot of the
 * packet's group, or QFEC_NO_SLOT for a packet that is no candidate
 * (unprotected, or its group already evicted); pkt_off, pkt_len, pkt_idx and
 * pkt_ok per packet as qfec_admit_ragged defines them.  pkt_ok may be NULL:
 * pkt_ok_out is then not written and may be NULL.  The call never dereferences
 * pkt_off and never reads a payload byte; offsets, lengths and indices are
 * carried, not judged (the admit judges them).
 * Outputs, in lockstep with the slots -- group s is slot s, so the tables feed
 * qfec_admit_ragged and qfec_accumulate_ragged with slot == NULL and n_groups
 * == n_slots: grp_ptr_out[0] = 0 and grp_ptr_out[s+1] - grp_ptr_out[s] = the
 * packets with pkt_slot == s (a slot nobody names gets an empty group, which
 * both calls define as a no-op -- but the admit judges the slot of every group,
 * an empty one's too, so a slot no group holds keeps a legal slot_k and
 * acc_len); at grp_ptr_out[s] + r lies the r-th packet of
 * slot s in ARRIVAL order (ascending p): its pkt_off, pkt_len, pkt_idx, its
 * pkt_ok if given, and in src_out (may be NULL) its arrival index p, which
 * maps the admit's verdict[q] back to a packet.  Entries from
 * grp_ptr_out[n_slots] on are not written; the caller guarantees room for
 * n_packets entries in each output table and n_slots + 1 in grp_ptr_out.
 * The outputs are a pure function of the inputs, with one exception: a slot
 * named by more than 255 packets in the call.  Its entries are exactly its
 * packets, each once, the five tables consistent per entry, in unspecified
 * order; the admit refuses such a group (k_g > 255) and latches, so this call
 * does not, and it spends no more than linear time on it.
 * counts[0..2] (may be NULL): packets binned, packets with QFEC_NO_SLOT (a
 * result), packets with any other pkt_slot >= n_slots.  The last are skipped
 * and latched on the device like qfec_accumulate_ragged's slot >= n_slots, and
 * returned by the next qfec_sync as -QUIC_INVALID_FEC_DATA; every other
 * packet's outputs are right.
 * Refused on the host (nothing launched, nothing written): QFEC_PTR_HOST,
 * QFEC_PTR_MAPPED or QFEC_ASYNC; a NULL buffer other than pkt_ok, pkt_ok_out
 * without pkt_ok, src_out and counts; pkt_ok given without pkt_ok_out;
 * n_packets >= 2^32 or n_slots >= 2^32 (QFEC_ERR_INTERNAL).  n_slots == 0
 * succeeds before the buffers are looked at (counts, if given, receives three
 * zeroes; nothing else is written).  n_packets == 0 with n_slots > 0 is an
 * ordinary call: grp_ptr_out is required and receives n_slots + 1 zeroes,
 * counts three, and no other table is looked at.
 * QFEC_CACHED and QFEC_SMALL_GROUPS are accepted and change nothing.  Device
 * pointers only; the call only queues work on the context's stream, never
 * waits and never reads anything back.  Its intermediate state lives in the
 * context-owned scratch of qfec_revive_batch: 20 bytes per packet (a 16-byte
 * record and a provisional rank), 4 bytes per slot (a counter), 4 bytes per
 * 256 slots and 48 bytes.  An admit that follows on the same stream reuses
 * the block; stream order makes that safe, as between admit and revive. */
#define QFEC_NO_SLOT 0xFFFFFFFFu /* pkt_slot value: this packet is in no open group */
int qfec_bin_arrivals(qfec_ctx* ctx, const uint32_t* pkt_slot, const uint64_t* pkt_off,
                      const uint16_t* pkt_len, const uint8_t* pkt_idx, const uint8_t* pkt_ok,
                      uint64_t n_packets, uint64_t n_slots, uint32_t* grp_ptr_out,
                      uint64_t* pkt_off_out, uint16_t* pkt_len_out, uint8_t* pkt_idx_out,
                      uint8_t* pkt_ok_out, uint32_t* src_out, uint64_t* counts, uint32_t flags);

/* Slots found or opened on the device: the group_map_ lookup and insert of
 * QuicConnection::GetFecGroup (quic_connection.cc:1388-1392), for a whole turn
 * at once.  Every packet has one 64-bit group key (suggested: connection index
 * << 40 | group number, the group number being the cleartext packet number
 * minus the FEC group offset byte; that byte is encrypted, so the key is
 * qfec_parse_opened's to build, below, or the host's where the protection is
 * NULL); this call resolves every key to the slot of its open group, or opens
 * a group in a free slot, and writes the pkt_slot array qfec_bin_arrivals
 * reads.  The turn is open -> qfec_assign_slots -> qfec_bin_arrivals ->
 * qfec_admit_ragged -> qfec_accumulate_ragged -> qfec_revive_tracked on one
 * stream, with no sync and no host decision in between.  No state is added:
 * which slots are open is acc_len[s] > 0, and by the fresh-slot rule of the
 * accumulate, the admit and the tracked revive a slot of length 0 is FREE
 * whatever slot_key[s] holds.  A slot released by any close call is free for
 * the next assign with nothing cleared: no free list, no tombstone.
 *
 * Inputs, n_packets records in arrival order: pkt_key[p] an opaque 64-bit name
 * of the packet's group (never interpreted), or QFEC_NO_KEY for a packet in no
 * FEC group; pkt_k[p] the group's K as the host knows it, read only for a
 * packet that opens a group and carried, not judged (the admit judges K == 0
 * and a map beyond map_stride).  Per slot: slot_key[s], the key the slot's
 * group was opened under, read where acc_len[s] > 0 and written where the call
 * opens a group; slot_k[s], the admit's table, written where the call opens a
 * group; acc_len, read only.
 * The rule, stated sequentially; the outputs are exactly these, a pure function
 * of the inputs (no scheduling, atomic order or hash shows in them):
 *   index maps each key to the LOWEST slot s with acc_len[s] > 0 and
 *     slot_key[s] == key (two open slots under one key cannot arise from this
 *     call's own outputs; if they do the lower wins and nothing is latched); an
 *     open slot holding QFEC_NO_KEY, a group the host opened itself, matches no
 *     packet;
 *   free is the ascending list of the slots with acc_len[s] == 0;
 *   packets are taken in ascending p:
 *     pkt_key[p] == QFEC_NO_KEY: pkt_slot_out[p] = QFEC_NO_SLOT, counts[2]++;
 *     the key is in index: pkt_slot_out[p] = that slot, counts[0]++;
 *     the key was opened earlier in this call: that slot, counts[1]++;
 *     otherwise, free not used up: s = the next entry of free, slot_key[s] =
 *       key, slot_k[s] = pkt_k[p], pkt_slot_out[p] = s, counts[1]++ and
 *       counts[3]++ (groups opened);
 *     otherwise: pkt_slot_out[p] = QFEC_NO_SLOT, counts[4]++ -- turned away,
 *       as the reference refuses a group beyond kMaxFecGroups: a result, not an
 *       error (later packets of that key in the call are turned away too).
 * Equivalently the r-th new key by FIRST arrival gets free[r] if r < |free|,
 * else none, and its K from its first packet.  Nothing is latched.
 * Never written: slot_key / slot_k of slots the call does not open; acc_len;
 * anything past pkt_slot_out[n_packets - 1].
 * A group opened here has length 0 until its first packet is folded, so each
 * assign is followed on its stream by bin -> admit -> accumulate over the same
 * acc_len before the next assign: until then the slot still counts as free.
 * If every candidate of a new group fails its tag nothing was folded, and the
 * slot is free again with nothing lost.
 * What stays with the host: which packets are candidates at all, expressed
 * through QFEC_NO_KEY (the key and the position, pkt_idx, come from the
 * encrypted private header: qfec_parse_opened, below).  A late duplicate of a released group would open it anew under
 * its key: the per-connection watermark below which a group is never reopened,
 * the forced closes and the bound on a connection's open groups are
 * qfec_retire_groups' (below), which runs in front of this call and hands it
 * the keys it passes.
 * Refused on the host (nothing launched, nothing written): QFEC_PTR_HOST,
 * QFEC_PTR_MAPPED or QFEC_ASYNC; a NULL buffer other than counts; n_packets >=
 * 2^32 or n_slots >= 2^32, or more than 2^30 of both together
 * (QFEC_ERR_INTERNAL).  n_packets == 0 succeeds before the buffers are looked
 * at (counts, if given, receives five zeroes).  n_slots == 0 with packets
 * present is an ordinary call: every keyed packet is turned away.
 * QFEC_CACHED and QFEC_SMALL_GROUPS are accepted and change nothing.  Device
 * pointers only; the call only queues work on the context's stream, never
 * waits and never reads anything back.  Its intermediate state lives in the
 * context-owned scratch of qfec_revive_batch and is rebuilt by every call: a
 * table of 16-byte entries, a power of two of them and at least twice
 * n_packets + n_slots, so between 36 and 68 bytes per packet and per slot,
 * plus 4 bytes per 256 of either and 272 bytes.  The calls that follow on the
 * same stream reuse the block; stream order makes that safe. */
#define QFEC_NO_KEY 0xFFFFFFFFFFFFFFFFull /* pkt_key value: this packet is in no FEC group */
int qfec_assign_slots(qfec_ctx* ctx, const uint64_t* pkt_key, const uint8_t* pkt_k,
                      uint64_t n_packets, uint64_t* slot_key, uint8_t* slot_k,
                      const uint16_t* acc_len, uint64_t n_slots, uint32_t* pkt_slot_out,
                      uint64_t* counts, uint32_t flags);

/* Group retention and forced closes on the device: the other half of the
 * connection's group map.  QuicFecReceiver::CloseFecGroupsBefore drops every
 * group below a STOP_WAITING's threshold and never recreates it; GetFecGroup,
 * with kMaxFecGroups groups open on a connection, drops the lowest and refuses
 * a group older than all it keeps.  This call applies both to a whole turn, in
 * front of the assign: the turn is open -> qfec_retire_groups ->
 * qfec_assign_slots -> qfec_bin_arrivals -> qfec_admit_ragged ->
 * qfec_accumulate_ragged -> qfec_revive_tracked (-> qfec_record_received ->
 * qfec_build_acks -> qfec_write_ack_frames, below) on one stream, with no sync and
 * no host decision in between.  Per packet the host supplies what the header
 * gives, per connection only the STOP_WAITING thresholds of the turn -- or not
 * even those: qfec_scan_frames, below, reads them out of the opened packets.
 *
 * This is the only call that interprets a key.  A key other than QFEC_NO_KEY
 * reads conn = key >> key_shift and number = key & ((1 << key_shift) - 1),
 * key_shift in 1..63 (connection index << 40 | group number: key_shift = 40).
 * conn_mark[c] is connection c's watermark: a group of c with number <
 * conn_mark[c] is dead; a mark of 0 kills nothing.  A group's number being its
 * first protected packet number, number < mark is
 * QuicFecGroup::IsWaitingForPacketBefore(mark).
 * The rule, stated sequentially; the outputs are exactly these, a pure function
 * of the inputs (no scheduling, atomic order or hash shows in them):
 *   1 raise: for i in 0 .. n_raise - 1, conn_mark[raise_conn[i]] = max(itself,
 *     raise_mark[i]) -- the turn's STOP_WAITING thresholds.  A connection may
 *     appear several times; a threshold below the mark changes nothing;
 *     n_raise == 0 with NULL tables is allowed.
 *   2 retain, only with max_groups > 0: for every connection c let L_c be the
 *     DISTINCT numbers >= conn_mark[c] among the open keyed slots of c
 *     (acc_len[s] > 0 and slot_key[s] != QFEC_NO_KEY; a free slot's stale key
 *     does not count) and the call's keyed packets of c.  If |L_c| >
 *     max_groups, conn_mark[c] becomes the max_groups-th largest element of
 *     L_c: the map holds the max_groups highest groups seen, and everything
 *     below the lowest kept one is refused.  max_groups == 0: no bound.
 *   3 close: every open keyed slot with number < conn_mark[conn] gets
 *     acc_len[s] = 0 and is listed, in ascending s, in closed_list (may be
 *     NULL; else room for n_slots entries; entries from the count on are not
 *     written).  Two open slots under one key are both closed.  slot_key,
 *     slot_k, the maps and the rows are never written: the slot is free by the
 *     fresh-slot rule, as after any other close, and slot_key[closed_list[i]]
 *     still names the group that went.
 *   4 filter: pkt_key_out[p] = QFEC_NO_KEY if pkt_key[p] is QFEC_NO_KEY or its
 *     number is below its connection's mark, else pkt_key[p].  pkt_key_out ==
 *     pkt_key (in place) is allowed.  The assign then reads pkt_key_out.
 * counts[0..4] (may be NULL): slots closed; packets refused, below their mark;
 * packets that came in as QFEC_NO_KEY; packets passed; keys (of packets and of
 * open slots) and raises with a connection out of range.  The first four are
 * results, and every packet is counted in exactly one of [1], [2], [3], [4].
 * Connection out of range (conn >= n_conns): such a packet's key goes out as
 * QFEC_NO_KEY and it takes no part in step 2; such an open slot is left alone;
 * such a raise is skipped.  Each is latched on the device and returned by the
 * next qfec_sync as -QUIC_INVALID_FEC_DATA; every other output is right.  An
 * open slot holding QFEC_NO_KEY (a group the host opened itself) takes part in
 * nothing.
 * Ordering: the retire runs before the assign of the same turn on the same
 * stream.  The assign sees the slots closed here as free and reuses them with
 * nothing cleared; between the two the host does nothing.
 * What stays with the host: the packet number and the connection from the
 * cleartext public header (the key and the position come from the encrypted
 * private header, through qfec_parse_opened, below); which packets are
 * candidates at all; and raising a mark past a group
 * that finished or was revived ahead of older open ones, for which it has
 * revived_list and status and feeds the raise list.
 * Where the turn differs from the per-packet reference: packets of a group
 * evicted later in the same turn are not folded first (the reference would
 * have folded them, and might have revived the group before evicting it); and
 * the mark is monotone (after a kept group finishes, the reference would again
 * create a never-seen group below the lowest kept one; the mark refuses it).
 * Refused on the host (nothing launched, nothing written): QFEC_PTR_HOST,
 * QFEC_PTR_MAPPED or QFEC_ASYNC; NULL slot_key or acc_len with n_slots > 0;
 * NULL pkt_key or pkt_key_out with n_packets > 0; NULL conn_mark with n_conns >
 * 0; NULL raise tables with n_raise > 0; key_shift outside 1..63; max_groups >
 * 16; n_packets, n_slots, n_conns or n_raise >= 2^32 (QFEC_ERR_INTERNAL, in
 * that order).  n_packets == 0 with slots present is an ordinary call, the
 * pure CloseFecGroupsBefore, and n_slots == 0 with packets present is one too;
 * only when n_packets, n_slots and n_raise are all 0 does the call succeed
 * before the buffers are looked at (counts, if given, receives five zeroes).
 * QFEC_CACHED and QFEC_SMALL_GROUPS are accepted and change nothing.  Device
 * pointers only; the call only queues work on the context's stream, never
 * waits and never reads anything back.  Its intermediate state lives in the
 * context-owned scratch of qfec_revive_batch and is rebuilt by every call: 64
 * bytes, 4 bytes per 256 slots and, with max_groups > 0, 8 * (max_groups + 1)
 * bytes per connection; nothing per packet.  The calls that follow on the same
 * stream reuse the block; stream order makes that safe. */
int qfec_retire_groups(qfec_ctx* ctx, const uint64_t* pkt_key, uint64_t n_packets,
                       const uint64_t* slot_key, uint16_t* acc_len, uint64_t n_slots,
                       uint64_t* conn_mark, uint64_t n_conns, uint32_t key_shift,
                       uint32_t max_groups, const uint32_t* raise_conn,
                       const uint64_t* raise_mark, uint64_t n_raise, uint64_t* pkt_key_out,
                       uint32_t* closed_list, uint64_t* counts, uint32_t flags);

/* Private headers on the device: QuicFramer::ProcessAuthenticatedHeader
 * (quic_framer.cc:1102-1141) for a whole turn.  The framer decrypts first
 * (ProcessDataPacket, quic_framer.cc:605-629) and parses the private flags and
 * the FEC group offset from the DECRYPTED buffer: GetStartOfEncryptedData puts
 * both inside the encrypted region.  For a packet opened on the device
 * (qfec_chacha20poly1305_open_batch, qfec_aes128gcm_open_batch) whether it is
 * in a group, which group (packet number - offset), its position (the offset)
 * and whether it is the FEC packet therefore lie in device memory.  This call
 * reads them there, and the turn is open -> qfec_parse_opened ->
 * qfec_retire_groups -> qfec_assign_slots -> qfec_bin_arrivals ->
 * qfec_admit_ragged -> qfec_accumulate_ragged -> qfec_revive_tracked (->
 * qfec_record_received -> qfec_build_acks, which read hdr_out and entropy_out)
 * on one stream, with no sync and no host decision in between; the bin reads
 * body_off_out, body_len_out, pkt_idx_out and pkt_ok.
 *
 * Inputs, n_packets records in arrival order: packet p's plaintext is
 * pkt_len[p] bytes at bytes + pkt_off[p] (the open call's out and out_off, with
 * in_len - 12), packet_number[p] its full packet number (what the open call
 * was given), pkt_conn[p] its connection index, pkt_ok[p] the open call's
 * verdict (pkt_ok NULL: all verified).
 * The rule, per packet, checked in this order; hdr_out[p] is the class:
 *   pkt_ok given and pkt_ok[p] == 0        QFEC_HDR_FAILED.  No payload byte of
 *                                          the packet is read (the open left
 *                                          stale bytes there).
 *   pkt_len[p] == 0                        QFEC_HDR_NO_FLAGS ("Unable to read
 *                                          private flags.")
 *   flags byte above the version's maximum QFEC_HDR_ILLEGAL_FLAGS (7 for
 *                                          quic_version <= 31, 1 above)
 *   FEC_GROUP bit (2) set and, in turn:
 *     pkt_len[p] < 2                       QFEC_HDR_NO_OFFSET
 *     offset >= packet_number[p]           QFEC_HDR_BAD_OFFSET
 *     pkt_len[p] == 2                      QFEC_HDR_EMPTY: the framer's "Packet
 *                                          has no frames."; the admit would
 *                                          otherwise latch on a length of 0
 *     pkt_conn[p] >> (64 - key_shift) != 0, (packet_number[p] - offset) >>
 *     key_shift != 0, or the key built
 *     equals QFEC_NO_KEY                   QFEC_HDR_RANGE: a caller error,
 *                                          latched on the device and returned
 *                                          by the next qfec_sync as
 *                                          -QUIC_INVALID_FEC_DATA, as
 *                                          qfec_retire_groups latches a
 *                                          connection out of range
 *   otherwise                              the flags byte itself, 0..7: accepted
 * The outputs follow from the class, a pure function of the inputs:
 *   accepted, in a group: pkt_key_out[p] = pkt_conn[p] << key_shift |
 *     (packet_number[p] - offset); pkt_idx_out[p] = offset, the position (0 ..
 *     K - 1 a data packet, K the FEC packet); body_off_out[p] = pkt_off[p] + 2,
 *     body_len_out[p] = pkt_len[p] - 2: what QuicFecGroup::Update folds, and an
 *     FEC packet's redundancy.
 *   accepted, in no group (flags 4 and 5, FEC without a group, included: the
 *     reference framer accepts them): pkt_key_out[p] = QFEC_NO_KEY,
 *     pkt_idx_out[p] = 0, body_off_out[p] = pkt_off[p] + 1, body_len_out[p] =
 *     pkt_len[p] - 1.
 *   every other class: pkt_key_out[p] = QFEC_NO_KEY, pkt_idx_out[p] = 0,
 *     body_off_out[p] = pkt_off[p], body_len_out[p] = 0.
 *   entropy_out[p] (may be NULL) = (flags & 1) << (packet_number[p] % 8) when
 *     accepted, else 0: GetPacketEntropyHash, as qfec_entropy_cumulative_batch
 *     reads it.
 * counts[0..5] (may be NULL), written, not added to: data packets in a group;
 * FEC packets in a group; accepted outside any group; FAILED; headers rejected
 * (NO_FLAGS, ILLEGAL_FLAGS, NO_OFFSET, BAD_OFFSET, EMPTY); RANGE.  Every packet
 * is counted in exactly one.
 * No byte outside [pkt_off[p], pkt_off[p] + pkt_len[p]) is read, whatever the
 * alignment of pkt_off[p].
 * Where this differs from the reference: a rejected header is a per-packet
 * result here (the framer raises QUIC_INVALID_PACKET_HEADER and the connection
 * closes; that policy stays with the host, which has hdr_out and counts[4]);
 * EMPTY is the framer's verdict one step later, taken here because a body of 0
 * bytes must not reach the admit.
 * What stays with the host: the packet number and the connection, which come
 * from the genuinely cleartext public header; K, the negotiated group size, in
 * pkt_k; and policy.
 * Refused on the host (nothing launched, nothing written): QFEC_PTR_HOST,
 * QFEC_PTR_MAPPED or QFEC_ASYNC; a NULL buffer other than pkt_ok, entropy_out
 * and counts; key_shift outside 1..63; quic_version outside 1..33; n_packets
 * >= 2^32 (QFEC_ERR_INTERNAL, in that order).  n_packets == 0 succeeds before
 * the buffers are looked at (counts, if given, receives six zeroes).
 * QFEC_CACHED and QFEC_SMALL_GROUPS are accepted and change nothing.  Device
 * pointers only; the call only queues work on the context's stream (a memset
 * of counts and one kernel), never waits, never reads anything back and needs
 * no scratch. */
#define QFEC_HDR_FAILED 0x80u        /* hdr_out: pkt_ok[p] == 0, nothing read */
#define QFEC_HDR_NO_FLAGS 0x81u      /* no private flags byte */
#define QFEC_HDR_ILLEGAL_FLAGS 0x82u /* flags above the version's maximum */
#define QFEC_HDR_NO_OFFSET 0x83u     /* FEC_GROUP set, no offset byte */
#define QFEC_HDR_BAD_OFFSET 0x84u    /* offset >= packet number */
#define QFEC_HDR_RANGE 0x85u         /* connection or group number does not fit the key */
#define QFEC_HDR_EMPTY 0x86u         /* in a group, nothing behind the header */
int qfec_parse_opened(qfec_ctx* ctx, const uint8_t* bytes, const uint64_t* pkt_off,
                      const uint16_t* pkt_len, const uint64_t* packet_number,
                      const uint32_t* pkt_conn, const uint8_t* pkt_ok, uint64_t n_packets,
                      int quic_version, uint32_t key_shift, uint64_t* pkt_key_out,
                      uint8_t* pkt_idx_out, uint64_t* body_off_out, uint16_t* body_len_out,
                      uint8_t* hdr_out, uint8_t* entropy_out, uint64_t* counts, uint32_t flags);

/* The sender's mirror: WriteFecPrivateHeader over a batch, in front of the
 * seal.  hdr[p] (the private flags byte: 1 entropy, 2 FEC_GROUP, 4 FEC) is
 * written at bytes + pkt_off[p] and, where the FEC_GROUP bit (2) is set,
 * fec_offset[p] behind it; body_off_out[p] (may be NULL) = pkt_off[p] + 1 or +
 * 2: where the frames go, or where qfec_emit_accumulated is to put the
 * redundancy.  A record that WriteFecPrivateHeader refuses -- FEC without a
 * group, or flags above the version's maximum (7 for quic_version <= 31, 1
 * above) -- writes no byte, gets body_off_out[p] = pkt_off[p], and is latched
 * (the next qfec_sync returns -QUIC_INVALID_FEC_DATA).  counts[0..1] (may be
 * NULL), written, not added to: records written, records refused.  Two
 * records must not overlap.  Refusals on the host, n_packets == 0, the flags
 * and the queueing as qfec_parse_opened; only body_off_out and counts may be
 * NULL. */
int qfec_write_private_headers(qfec_ctx* ctx, uint8_t* bytes, const uint64_t* pkt_off,
                               const uint8_t* hdr, const uint8_t* fec_offset,
                               uint64_t n_packets, int quic_version, uint64_t* body_off_out,
                               uint64_t* counts, uint32_t flags);

/* Frames on the device: QuicFramer::ProcessFrameData (quic_framer.cc:1168-1342)
 * for a whole turn, with a visitor that always returns true, and the
 * STOP_WAITING bookkeeping of QuicConnection (quic_connection.cc:765-792,
 * :1009-1016).  The frames lie behind the private header, in the encrypted part
 * of the packet: for a packet opened on the device they exist only in device
 * memory, as the private flags did.  The call sits behind qfec_parse_opened and
 * in front of qfec_retire_groups, and its STOP_WAITING result is what the retire
 * and the record take as their raises: no host decision is left in the turn.
 * The rule per packet is qfec_wire_scan_frames', below.
 *
 * Inputs, n_packets records in arrival order: packet p's frame area is
 * body_len[p] bytes at bytes + body_off[p] (the parse's body_off_out and
 * body_len_out), packet_number[p] and pkt_conn[p] as the parse was given them,
 * pkt_pn_len[p] the packet number's length on the wire (1, 2, 4 or 6, from the
 * cleartext public header; STOP_WAITING's delta has that length), hdr[p] the
 * parse's hdr_out (hdr NULL: every packet an accepted data packet).
 * frm_status[p], checked in this order:
 *   hdr[p] >= 0x80 or hdr[p] & 4           QFEC_FRM_SKIPPED: not accepted, or an
 *                                          FEC packet, whose body is redundancy.
 *                                          No byte of the packet is read.
 *   pkt_pn_len[p] not 1, 2, 4 or 6         QFEC_FRM_PN_LEN, a caller error: nothing
 *                                          read, latched (the next qfec_sync
 *                                          returns -QUIC_INVALID_FEC_DATA)
 *   pkt_conn[p] >= n_conns                 QFEC_FRM_RANGE: nothing read, latched
 *   otherwise                              the walk's verdict, QFEC_FRM_OK ..
 *                                          QFEC_FRM_TOO_MANY
 * Only a packet with QFEC_FRM_OK lists frames and takes part in the
 * STOP_WAITING step.  frm_ptr (n_packets + 1 words) receives the true prefix
 * sums of the frames listed: packet p's are entries [frm_ptr[p], frm_ptr[p +
 * 1]) of the table, in the order they lie in the packet, and frm_ptr[n_packets]
 * is the total whether or not it fits.
 * The table, struct-of-arrays with room for frm_cap entries; per entry e:
 *   frm_pkt[e]    the packet's index p
 *   frm_type[e]   the wire value 0..8, QFEC_FRAME_STREAM, QFEC_FRAME_ACK
 *   frm_flags[e]  stream: bit 0 fin, bit 1 the frame had a data length; ack: the
 *                 type byte's low six bits (nacks 0x20, truncated 0x10, lengths)
 *   frm_off[e]    an offset into bytes: the stream data; the ack's type byte;
 *                 the reason text of a close or goaway; the bytes behind a
 *                 padding's type byte
 *   frm_len[e]    the stream data's length; the ack frame's whole length, so
 *                 that qfec_wire_parse_ack_frame(bytes + frm_off, frm_len, ...)
 *                 takes it as it lies; the text's length; the padding's, which
 *                 is the rest of the packet (QuicPaddingFrame(BytesRemaining()))
 *   frm_id[e]     stream, rst, window update, blocked: the stream id; goaway:
 *                 the last good stream; path close: the path id
 *   frm_val[e]    stream: the stream offset; rst, window update: the byte
 *                 offset; stop waiting: least_unacked = packet number - delta;
 *                 ack: the largest observed
 *   frm_code[e]   rst, close, goaway: the error code as read; stop waiting, ack:
 *                 the entropy hash
 * and 0 in every field a kind does not name.  Nothing is stored at or beyond
 * frm_cap; with frm_cap == 0 the eight table pointers may be NULL.
 * STOP_WAITING state, caller-allocated, all zero = a new connection, per
 * connection c < n_conns: sw_seen[c] is largest_seen_packet_with_stop_waiting_,
 * sw_least[c] and sw_hash[c] are last_stop_waiting_frame_; sw_conn[c] = c is
 * written by every call with n_packets > 0.  A packet holds a STOP_WAITING if
 * the last such frame in it has least_unacked > 0 (the reference lets a later
 * frame overwrite and acts only on a least_unacked above 0).  Among the call's
 * packets of c with QFEC_FRM_OK that hold one and have packet_number[p] >
 * sw_seen[c], the one with the largest packet number wins, among copies of that
 * number the earliest in arrival order; its packet number, least_unacked and
 * hash become sw_seen[c], sw_least[c] and sw_hash[c].  Every other connection
 * keeps its three.  The outputs are a pure function of the inputs.  The turn
 * then passes raise_conn = sw_conn, raise_mark = raise_least = sw_least,
 * raise_hash = sw_hash with n_raise = n_conns to qfec_retire_groups and
 * qfec_record_received: a threshold fed again changes nothing in either.
 * counts[0..12] (may be NULL), written, not added to: packets OK; SKIPPED;
 * rejected by the walk (NO_FRAMES .. BAD_LEAST); TOO_MANY; PN_LEN or RANGE;
 * frames listed that are stream, ack, stop waiting, any other kind; the total,
 * frm_ptr[n_packets]; the entries that did not fit in frm_cap; connections
 * whose frame was replaced; of those, the ones whose new least_unacked is below
 * the old sw_least (ValidateStopWaitingFrame's first test: policy, the host's).
 * No byte outside [body_off[p], body_off[p] + body_len[p]) is read, whatever
 * the alignment, and at most max_frames frames of a packet are walked.
 * Where this differs from the reference: a packet whose walk fails lists no
 * frame (the framer has delivered the ones before the error) and closing the
 * connection stays with the host, which has frm_status; BAD_LEAST is a verdict
 * where the reference trips a DCHECK; TOO_MANY is a result, not an error, and
 * the walk stops at the type byte of frame max_frames + 1 without judging it;
 * error codes come out raw (the host clamps them to QUIC_LAST_ERROR and
 * QUIC_STREAM_LAST_ERROR); the reference applies every newer STOP_WAITING in
 * arrival order, the turn applies the newest one.
 * Refused on the host (nothing launched, nothing written), in this order:
 * QFEC_PTR_HOST, QFEC_PTR_MAPPED or QFEC_ASYNC; a NULL buffer other than hdr
 * and counts, the tables with frm_cap == 0 and the state with n_conns == 0;
 * quic_version outside 1..33; max_frames outside 1..255; n_packets, n_conns,
 * frm_cap or n_packets * max_frames >= 2^32 (QFEC_ERR_INTERNAL).  n_packets == 0
 * succeeds before the buffers are looked at (counts, if given, receives
 * thirteen zeroes, frm_ptr[0], if given, one).  Device pointers only; the call
 * only queues work on the context's stream (four kernels in the revive calls'
 * scratch), never waits and never reads anything back. */
#define QFEC_FRM_OK 0u
#define QFEC_FRM_SKIPPED 1u        /* not accepted by the parse, or an FEC packet */
#define QFEC_FRM_NO_FRAMES 2u      /* "Packet has no frames." */
#define QFEC_FRM_ILLEGAL_TYPE 3u   /* "Illegal frame type." */
#define QFEC_FRM_STREAM 4u         /* QUIC_INVALID_STREAM_DATA */
#define QFEC_FRM_ACK 5u            /* QUIC_INVALID_ACK_DATA */
#define QFEC_FRM_RST 6u            /* QUIC_INVALID_RST_STREAM_DATA */
#define QFEC_FRM_CLOSE 7u          /* QUIC_INVALID_CONNECTION_CLOSE_DATA */
#define QFEC_FRM_GOAWAY 8u         /* QUIC_INVALID_GOAWAY_DATA */
#define QFEC_FRM_WINDOW_UPDATE 9u  /* QUIC_INVALID_WINDOW_UPDATE_DATA */
#define QFEC_FRM_BLOCKED 10u       /* QUIC_INVALID_BLOCKED_DATA */
#define QFEC_FRM_STOP_WAITING 11u  /* QUIC_INVALID_STOP_WAITING_DATA */
#define QFEC_FRM_PATH_CLOSE 12u    /* QUIC_INVALID_PATH_CLOSE_DATA */
#define QFEC_FRM_BAD_LEAST 13u     /* STOP_WAITING delta above the packet number */
#define QFEC_FRM_TOO_MANY 14u      /* more than max_frames frames */
#define QFEC_FRM_PN_LEN 15u        /* pkt_pn_len not 1, 2, 4 or 6 (latched) */
#define QFEC_FRM_RANGE 16u         /* connection out of range (latched) */
#define QFEC_FRAME_STREAM 0x80u    /* frm_type, beside the wire's 0..8 */
#define QFEC_FRAME_ACK 0x40u
int qfec_scan_frames(qfec_ctx* ctx, const uint8_t* bytes, const uint64_t* body_off,
                     const uint16_t* body_len, const uint64_t* packet_number,
                     const uint32_t* pkt_conn, const uint8_t* pkt_pn_len, const uint8_t* hdr,
                     uint64_t n_packets, int quic_version, uint32_t max_frames,
                     uint8_t* frm_status, uint32_t* frm_ptr, uint32_t* frm_pkt, uint8_t* frm_type,
                     uint8_t* frm_flags, uint64_t* frm_off, uint16_t* frm_len, uint32_t* frm_id,
                     uint64_t* frm_val, uint32_t* frm_code, uint64_t frm_cap, uint64_t* sw_seen,
                     uint64_t* sw_least, uint8_t* sw_hash, uint32_t* sw_conn, uint64_t n_conns,
                     uint64_t* counts, uint32_t flags);

/* Ack state on the device: QuicReceivedPacketManager and its EntropyTracker
 * (quic_received_packet_manager.cc:40-131, :144-193, :222-286) for a whole
 * turn.  A packet's entropy bit (qfec_parse_opened's entropy_out), the verdict
 * that it verified and its header was accepted (hdr_out) and the fact that a
 * packet was revived (qfec_revive_tracked's status and revived_idx) lie in
 * device memory, and all three are for the receiver's ack.  These two calls end
 * the turn where the reference's ends, with the ack frame's content: open ->
 * qfec_parse_opened -> qfec_retire_groups -> qfec_assign_slots ->
 * qfec_bin_arrivals -> qfec_admit_ragged -> qfec_accumulate_ragged ->
 * qfec_revive_tracked -> qfec_record_received -> qfec_build_acks ->
 * qfec_write_ack_frames on one stream, and the frames go to the seal where they
 * lie; the only copy back is the sealed ack packets.
 *
 * State, caller-allocated device memory, all zero = a new connection.  Per
 * connection c < n_conns, window a power of two, 64 <= window <= 65536:
 *   rcv_cells[c * window + (pn & (window - 1))]  one byte per packet number:
 *     QFEC_CELL_RECEIVED (1), QFEC_CELL_ENTROPY (2, the entropy flag),
 *     QFEC_CELL_REVIVED (4, revived at some time); a packet counts as revived
 *     while the REVIVED bit is set and the RECEIVED bit is clear.  Cells are only OR-ed into, or
 *     cleared when the window passes over them.  rcv_cells is 4-byte aligned.
 *   rcv_least[c]    peer_least_packet_awaiting_ack_; below, lo = max(it, 1)
 *   rcv_largest[c]  largest_observed
 *   rcv_hash[c]     the cumulative entropy of everything below lo
 * Only cells of pn in [lo, rcv_largest[c]] are live; every other cell's
 * content is unspecified and is never read as state.  The ack's entropy hash is
 * rcv_hash[c] ^ XOR{ e(pn) << (pn % 8) : pn live and received }.
 *
 * qfec_record_received: one turn into the state.  The outputs are a pure
 * function of the inputs (no atomic order shows in them); the rule, stated
 * sequentially, L = rcv_least[c], G = rcv_largest[c]:
 *   1 arrivals, n_packets records in arrival order (packet_number, pkt_conn;
 *     hdr = the parse's hdr_out, NULL: all accepted; entropy = its
 *     entropy_out, any non-zero value is flag 1, NULL: all 0), each classified
 *     against the state as it was BEFORE the call; first match wins and
 *     rcv_out[p] is the class:
 *       hdr[p] >= 0x80                     QFEC_RCV_NOT_ACCEPTED
 *       pkt_conn[p] >= n_conns             QFEC_RCV_RANGE, latched: the next
 *                                          qfec_sync returns
 *                                          -QUIC_INVALID_FEC_DATA
 *       pn == 0 or pn < L                  QFEC_RCV_STALE
 *       pn - max(L, 1) >= window           QFEC_RCV_OVERFLOW: a result, not an
 *                                          error; the host closes the
 *                                          connection, as the reference does at
 *                                          kMaxTrackedPackets
 *       pn <= G, its cell has RECEIVED    QFEC_RCV_DUPLICATE
 *       otherwise                          QFEC_RCV_RECORDED
 *     Then G' = max(G, the largest RECORDED pn of c); the cells of (max(G, lo -
 *     1), G'] are cleared; every RECORDED packet ORs 1 | flag << 1 into its
 *     cell.  Copies of one packet inside one call are each RECORDED, and where
 *     they disagree on the flag it stays 1.
 *   2 revived, n_groups groups of the turn's qfec_revive_tracked (status,
 *     revived_idx, slot -- NULL: group g has slot g -- with the assign's
 *     slot_key and the retire's key_shift; n_groups == 0 skips the step): for
 *     every group with status QFEC_GROUP_REVIVED and slot[g] < n_slots, key =
 *     slot_key[slot[g]], c = key >> key_shift, pn = (key & ((1 << key_shift) -
 *     1)) + revived_idx[g].  If key != QFEC_NO_KEY, c < n_conns, lo <= pn < G'
 *     and the cell lacks RECEIVED, 4 is OR-ed into the cell
 *     (RecordPacketRevived's IsMissing test in integration/libquic_fec.patch);
 *     otherwise nothing is written and the group counts as "revived, not
 *     missing".  The call is queued after the turn's qfec_revive_tracked and
 *     before the next qfec_assign_slots: a released slot's slot_key names its
 *     group until the slot is reused.
 *   3 raises, the turn's STOP_WAITING frames (raise_conn, raise_least,
 *     raise_hash; at most one per connection per call: the caller's guarantee,
 *     unchecked, as the admit's distinct slots are).  For L' = raise_least[i] >
 *     L: with L' <= G' + 1, if some pn in [lo, L') lacks RECEIVED rcv_hash =
 *     raise_hash[i] (SetCumulativeEntropyUpTo after RemoveUpTo returned true),
 *     else rcv_hash ^= the hashes of the pn in [lo, L') (the reference keeps its
 *     own hash); with L' > G' + 1, a jump, rcv_hash = raise_hash[i] whatever
 *     was received.  In both cases rcv_least = L'.  raise_conn[i] >= n_conns is
 *     skipped and latched; L' <= L changes nothing.
 * counts[0..11] (may be NULL), written, not added to: [0..5] the packets of
 * classes QFEC_RCV_NOT_ACCEPTED .. QFEC_RCV_RECORDED (the class is the index;
 * every packet in exactly one); [6] cells newly set (RECORDED less the copies
 * inside the call); [7] revived groups recorded; [8] revived groups not
 * missing; [9] raises applied (L' > L, jumps included); [10] raises that
 * dropped a missing packet; [11] jumps.
 *
 * qfec_build_acks: GetUpdatedAckFrame for the connections ack_conn[a], a <
 * n_acks (repeats allowed); the state is only read.  max_ranges in 1..255,
 * max_revived in 0..255.  Per ack: if G < lo, largest_observed[a] = G,
 * entropy_hash[a] = rcv_hash and nothing else.  Otherwise the missing packets
 * are the pn in [lo, G) lacking RECEIVED, as maximal half-open intervals in
 * ascending order: range_lo / range_hi under range_ptr (uint32, n_acks + 1
 * entries), the form qfec_entropy_validate_batch reads.  With more than
 * max_ranges intervals the lowest max_ranges are kept, largest_observed[a] =
 * (range_lo of the first one dropped) - 1 and truncated[a] = 1: the framer's
 * truncation (quic_framer.cc:2222-2236), counted in queue intervals; the wire
 * writer's split into runs of at most 256 is qfec_write_ack_frames'.  entropy_hash[a] =
 * rcv_hash ^ the hashes of the received pn in [lo, largest_observed[a]]
 * (EntropyTracker::EntropyHash).  The revived list, rev_pn under rev_ptr, is
 * the highest max_revived revived pn in [lo, largest_observed[a]], ascending
 * (the patched ack writer lists the newest at or below the written largest
 * observed).  The tables have room for n_acks * max_ranges and n_acks *
 * max_revived entries; nothing is written past range_ptr[n_acks] and
 * rev_ptr[n_acks].  ack_conn[a] >= n_conns gives a zero ack with no entries and
 * is latched.
 *
 * Where the two differ from the reference: a turn is the reference fed the
 * turn's accepted arrivals in arrival order, then the revived packets, then the
 * raises; the interleaving inside a turn is gone, as qfec_retire_groups
 * explains for groups.  Copies inside one call are both RECORDED and the flag
 * is OR-ed (the reference lets the first copy win).  A packet with G < pn < L
 * can only exist after a jump and is STALE here (the reference moves
 * largest_observed and sometimes records its entropy).  A jump always adopts
 * the frame's hash (the reference trips DCHECK_LE(packet_number,
 * largest_observed_) there).  What stays with the host: receipt times and
 * ack_delay_time; the reordering statistics; when to send an ack
 * (ack_frame_updated_; HasNewMissingPackets can be read off the built ack).  The
 * wire writer is qfec_write_ack_frames; the frame's timestamp block stays with
 * the receipt times, on the host.
 * Refused on the host (nothing launched, nothing written), both calls:
 * QFEC_PTR_HOST, QFEC_PTR_MAPPED or QFEC_ASYNC; a NULL buffer other than hdr,
 * entropy, slot and counts (record) or rev_pn with max_revived == 0 (build)
 * -- the tables of a count that is 0 may be NULL too; key_shift outside 1..63
 * with n_groups > 0 (record); max_ranges outside 1..255 or max_revived above
 * 255 (build); a window that is not a power of two in 64..65536, or rcv_cells
 * not 4-byte aligned; a count >= 2^32, or n_acks * max(max_ranges,
 * max_revived) >= 2^32; slot == NULL with n_slots < n_groups
 * (QFEC_ERR_INTERNAL, in that order).  A record with n_packets, n_groups and
 * n_raise all 0 succeeds before the buffers are looked at (counts, if given,
 * receives twelve zeroes); a build with n_acks == 0 does too (range_ptr[0] and
 * rev_ptr[0], where given, receive 0).  QFEC_CACHED and QFEC_SMALL_GROUPS are
 * accepted and change nothing.  Device pointers only; the calls only queue work
 * on the context's stream, never wait and never read anything back.  Their
 * intermediate state lives in the context-owned scratch of qfec_revive_batch
 * and is rebuilt by every call: 8 bytes per connection (record), 8 bytes per
 * ack (build). */
#define QFEC_RCV_NOT_ACCEPTED 0u /* rcv_out: hdr[p] >= 0x80 */
#define QFEC_RCV_RANGE 1u        /* connection out of range (latched) */
#define QFEC_RCV_STALE 2u        /* packet number 0 or below the least awaited */
#define QFEC_RCV_OVERFLOW 3u     /* beyond the window: the host closes the connection */
#define QFEC_RCV_DUPLICATE 4u    /* received in an earlier call */
#define QFEC_RCV_RECORDED 5u     /* recorded */
#define QFEC_CELL_RECEIVED 1u
#define QFEC_CELL_ENTROPY 2u
#define QFEC_CELL_REVIVED 4u
int qfec_record_received(qfec_ctx* ctx, const uint64_t* packet_number, const uint32_t* pkt_conn,
                         const uint8_t* hdr, const uint8_t* entropy, uint64_t n_packets,
                         const uint8_t* status, const uint8_t* revived_idx, const uint32_t* slot,
                         const uint64_t* slot_key, uint64_t n_groups, uint64_t n_slots,
                         uint32_t key_shift, const uint32_t* raise_conn,
                         const uint64_t* raise_least, const uint8_t* raise_hash, uint64_t n_raise,
                         uint8_t* rcv_cells, uint64_t* rcv_least, uint64_t* rcv_largest,
                         uint8_t* rcv_hash, uint64_t n_conns, uint32_t window, uint8_t* rcv_out,
                         uint64_t* counts, uint32_t flags);
int qfec_build_acks(qfec_ctx* ctx, const uint32_t* ack_conn, uint64_t n_acks,
                    const uint8_t* rcv_cells, const uint64_t* rcv_least,
                    const uint64_t* rcv_largest, const uint8_t* rcv_hash, uint64_t n_conns,
                    uint32_t window, uint32_t max_ranges, uint32_t max_revived,
                    uint64_t* largest_observed, uint8_t* entropy_hash, uint8_t* truncated,
                    uint32_t* range_ptr, uint64_t* range_lo, uint64_t* range_hi,
                    uint32_t* rev_ptr, uint64_t* rev_pn, uint32_t flags);

/* qfec_write_ack_frames: the built acks as v<=31 ack frames, the bytes of
 * QuicFramer::AppendAckFrameAndTypeByte (quic_framer.cc:2172-2320, GetAckFrameInfo
 * :1005-1033) with the revived tail of integration/libquic_fec.patch -- the rule
 * is qfec_wire_write_ack_frame's, below, and the turn ends build -> write -> seal
 * on one stream, with one copy back of finished packets.  Inputs: ack_conn and
 * the eight outputs of qfec_build_acks (rev_pn may be NULL where rev_ptr lists
 * nothing); ack_delay_us[a] in microseconds, UINT64_MAX or a NULL array:
 * infinite; the ring rcv_cells with window and n_conns, only read.  Ack a's
 * frame goes to out + out_off[a] (any alignment) and has out_cap[a] bytes of
 * room there, the writer's capacity at the frame's first byte.  Every interval
 * is split into nack ranges of at most 256 numbers; with more of them than the
 * room holds the writer cuts the ack as the framer does: the lowest ranges that
 * fit are kept, the largest observed written is (first range dropped) - 1, and
 * the hash is entropy_hash[a] ^ the hashes of the received numbers in (largest
 * written, largest_observed[a]], read from the cells' QFEC_CELL_ENTROPY bits.
 * An ack with truncated[a] set is written as the frame it is (its lengths and
 * largest gap taken from the intervals given, the truncated bit set, no
 * timestamp byte) and may be cut further.  The timestamp count of a frame that
 * is not truncated is 0: receipt times stay with the host.
 * Outputs: out_len[a] = prefix_len + the frame's length, or 0 where nothing was
 * written -- with in_off[a] = out_off[a] - prefix_len (the packet header and
 * private flags in front of the frame) the seal calls take it as their in_len;
 * wire_largest[a] and wire_hash[a], the two as written (as given where nothing
 * was); ack_status[a]; counts[0..3] (may be NULL), written, not added to: the
 * acks per status.  ack_conn[a] >= n_conns gives length 0 and QFEC_ACKW_RANGE
 * and is latched, as in the build.  The tables are the caller's guarantee;
 * whatever they hold, no byte is stored outside [out_off[a], out_off[a] +
 * out_cap[a]), no cell is read outside the ring, at most 255 intervals and 255
 * revived numbers of an ack are read and every walk over cells is at most
 * window long.
 * Refused on the host (nothing launched, nothing written), in this order:
 * QFEC_PTR_HOST, QFEC_PTR_MAPPED or QFEC_ASYNC; a NULL buffer other than
 * ack_delay_us, rev_pn and counts (rcv_cells may be NULL with n_conns == 0); a
 * window that is not a power of two in 64..65536 or rcv_cells not 4-byte
 * aligned; n_acks or n_conns >= 2^32; prefix_len > 64 (QFEC_ERR_INTERNAL).
 * n_acks == 0 succeeds before the buffers are looked at (counts, if given,
 * receives four zeroes).  One kernel on the context's stream, no scratch; the
 * call never waits and never reads anything back. */
#define QFEC_ACKW_WRITTEN 0u /* ack_status: the frame holds all that was given */
#define QFEC_ACKW_CUT 1u     /* written, cut further by the writer */
#define QFEC_ACKW_NO_ROOM 2u /* no room for a mandatory byte: nothing written */
#define QFEC_ACKW_RANGE 3u   /* connection out of range (latched): nothing written */
int qfec_write_ack_frames(qfec_ctx* ctx, const uint32_t* ack_conn, uint64_t n_acks,
                          const uint64_t* largest_observed, const uint8_t* entropy_hash,
                          const uint8_t* truncated, const uint32_t* range_ptr,
                          const uint64_t* range_lo, const uint64_t* range_hi,
                          const uint32_t* rev_ptr, const uint64_t* rev_pn,
                          const uint64_t* ack_delay_us, const uint8_t* rcv_cells,
                          uint64_t n_conns, uint32_t window, uint8_t* out,
                          const uint64_t* out_off, const uint16_t* out_cap, uint32_t prefix_len,
                          uint16_t* out_len, uint64_t* wire_largest, uint8_t* wire_hash,
                          uint8_t* ack_status, uint64_t* counts, uint32_t flags);

/* ---- single buffer ------------------------------------------------------ */
/* out[j] ^= in[j] for j < n (QuicFecGroupInterface::XorBuffers). */
int qfec_xor_into(qfec_ctx* ctx, const uint8_t* in, uint64_t n, uint8_t* out, uint32_t flags);

/* ---- v<=31 FEC wire format (host memory; no device involved) ----------- */
/* What an FFI user (e.g. a cgo binding) needs around the parity bytes:
 *   private flags byte + 1-byte first_fec_protected_packet_offset, with the
 *   checks of QuicFramer::ProcessAuthenticatedHeader (quic_framer.cc:1102-1141:
 *   flags above the version's maximum are illegal — v > 31 allows only the
 *   entropy bit, quic_protocol.h:343-358 — and the offset must be below the
 *   packet number; the group is packet_number - offset);
 *   the ack frame's revived-packets list (count byte + N packet numbers of the
 *   largest-observed length, little-endian: quic_framer.cc:1477-1493 read,
 *   :2307-2317 write, kNumberOfRevivedPacketsSize quic_framer.h:64-65);
 *   an FEC packet body: private header (FEC | FEC_GROUP, offset) + redundancy.
 * Each returns the bytes written / consumed, or 0 on failure with the
 * framer's detailed error string in qfec_last_error(NULL). */
typedef struct qfec_fec_header {
  uint8_t entropy_flag;     /* PACKET_PRIVATE_FLAGS_ENTROPY */
  uint8_t fec_flag;         /* PACKET_PRIVATE_FLAGS_FEC: the payload is redundancy */
  uint8_t in_fec_group;     /* PACKET_PRIVATE_FLAGS_FEC_GROUP: offset byte follows */
  uint8_t fec_group_offset; /* packet_number - first protected packet number */
} qfec_fec_header;

size_t qfec_wire_write_private_header(const qfec_fec_header* h, uint8_t* buf, size_t cap);
size_t qfec_wire_parse_private_header(const uint8_t* buf, size_t len, int quic_version,
                                      uint64_t packet_number, qfec_fec_header* out);
size_t qfec_wire_write_revived(const uint64_t* revived, size_t n, size_t packet_number_length,
                               uint8_t* buf, size_t cap);
/* Parses into revived[0 .. *n_out) (at most 255 entries: size the array so). */
size_t qfec_wire_parse_revived(const uint8_t* buf, size_t len, size_t packet_number_length,
                               uint64_t* revived, size_t* n_out);
size_t qfec_wire_fec_packet_body(uint64_t packet_number, uint64_t fec_group, int entropy_flag,
                                 const uint8_t* redundancy, size_t redundancy_len, uint8_t* buf,
                                 size_t cap);
/* The v<=31 ack frame, the host mirror of qfec_write_ack_frames
 * (AppendAckFrameAndTypeByte with GetAckFrameInfo, and ProcessAckFrame,
 * quic_framer.cc:1400-1495).  The write takes the largest observed and its
 * entropy hash, the missing packets as n_ranges half-open intervals [range_lo[i],
 * range_hi[i]), ascending, the revived numbers, ascending, the ack delay in
 * microseconds (UINT64_MAX: infinite) and whether the ack was cut already, and
 * writes the frame into buf[0..cap), cap being the room at the frame's first
 * byte:
 *   every interval is split into nack ranges of at most 256 numbers; max_delta
 *     is the largest gap between two intervals or from the last missing number
 *     to the largest observed, taken before any truncation; ll and mm are the
 *     minimal lengths (1, 2, 4, 6) of the largest observed and of max_delta;
 *   max_num_ranges = min(255, (cap - 1 - (4 + ll) - 1) / (mm + 1)); with more
 *     ranges the lowest max_num_ranges are kept, the largest observed written is
 *     (start of the first one dropped) - 1, the hash is entropy_up_to(user, that
 *     number) and the truncated bit is set; ll stays;
 *   type 0x40 | nacks << 5 | truncated << 4 | flags(ll) << 2 | flags(mm), hash,
 *     largest (ll bytes, little-endian), the delay as ufloat16, a timestamp
 *     count of 0 unless truncated; with no range the frame ends there; else the
 *     range count, the ranges from the highest down as (missing_delta in mm
 *     bytes, length - 1), the revived count and, ll bytes each, the newest
 *     revived numbers at or below the largest written, newest first, at most
 *     min(255, (room - 1) / ll).
 * wire_largest, wire_hash and wire_truncated (each may be NULL) receive what the
 * frame says.  Returns the frame's length; 0, with nothing stored, where the
 * reference writer fails for want of room for a mandatory byte.  The parse is
 * the inverse: the ranges merged back into maximal intervals (the CSR form of
 * qfec_entropy_validate_batch; range_lo, range_hi and revived have room for 255
 * entries), the delay as the ufloat16 written, a timestamp block skipped over.
 * Returns the bytes consumed, or 0 and the framer's error string in
 * qfec_last_error(NULL). */
typedef uint8_t (*qfec_entropy_up_to_fn)(void* user, uint64_t packet_number);
size_t qfec_wire_write_ack_frame(uint64_t largest_observed, uint8_t entropy_hash,
                                 const uint64_t* range_lo, const uint64_t* range_hi,
                                 size_t n_ranges, const uint64_t* revived, size_t n_revived,
                                 uint64_t ack_delay_us, int truncated,
                                 qfec_entropy_up_to_fn entropy_up_to, void* user, uint8_t* buf,
                                 size_t cap, uint64_t* wire_largest, uint8_t* wire_hash,
                                 int* wire_truncated);
size_t qfec_wire_parse_ack_frame(const uint8_t* buf, size_t len, uint64_t* largest_observed,
                                 uint8_t* entropy_hash, uint16_t* delay_ufloat16, int* truncated,
                                 uint64_t* range_lo, uint64_t* range_hi, size_t* n_ranges,
                                 uint64_t* revived, size_t* n_revived);
/* One packet's frames, the host mirror of qfec_scan_frames' walk
 * (QuicFramer::ProcessFrameData with a visitor that always returns true): body
 * is the len <= 65535 bytes behind the private header, quic_version 1..33,
 * pn_len 1, 2, 4 or 6.  Frame types as the reference reads them, every
 * multi-byte value little-endian as QuicDataReader reads it:
 *   1 f d ooo ss  STREAM: id in ss + 1 bytes, offset in 0 or ooo + 1 bytes, with
 *                 d a 16-bit data length, without it data to the packet's end
 *   0 1 n t ll mm ACK (the format of versions up to 33), stepped over: hash,
 *                 largest in ll bytes, ufloat16 delay; unless t a timestamp
 *                 count k and, k > 0, 5 + 3 (k - 1) bytes; with n a range count
 *                 times mm + 1 bytes and, version <= 31, a revived count times
 *                 ll.  The ranges are bounds-checked, not looked at.
 *   0 0 1 .....   "Illegal frame type."
 *   0 PADDING, which ends the packet; 1 RST_STREAM 4 + 8 + 4; 2 CONNECTION_CLOSE
 *   4 + a string with a 16-bit length; 3 GOAWAY 4 + 4 + a string; 4
 *   WINDOW_UPDATE 4 + 8; 5 BLOCKED 4; 6 STOP_WAITING hash + pn_len bytes of
 *   delta; 7 PING; 8 PATH_CLOSE 1; 9..31 illegal.
 * *status receives the verdict, QFEC_FRM_OK or NO_FRAMES .. TOO_MANY; the
 * arrays, each with room for max_frames entries, the frames read before the
 * verdict was reached, *n_walked of them, with frm_off counted from body[0].
 * Returns the frames the packet lists: *n_walked under QFEC_FRM_OK, else 0.
 * (size_t)-1 and qfec_last_error(NULL) for a NULL pointer, a length above
 * 65535, a version, pn_len or max_frames (1..255) out of range. */
size_t qfec_wire_scan_frames(const uint8_t* body, size_t len, int quic_version,
                             uint64_t packet_number, size_t pn_len, size_t max_frames,
                             uint8_t* status, size_t* n_walked, uint8_t* frm_type,
                             uint8_t* frm_flags, uint32_t* frm_off, uint16_t* frm_len,
                             uint32_t* frm_id, uint64_t* frm_val, uint32_t* frm_code);

/* ---- packet protection around FEC (ENCRYPTION_NONE) -------------------- */
/* The NULL packet protection libquic applies before the handshake completes:
 * a 12-byte FNV-1a-128 tag of header || payload written in front of the
 * payload.  Batched over a CSR layout (one lane per packet on the device):
 * packet p's associated data (its packet header) is ad_len[p] bytes at
 * bytes + ad_off[p]; its payload in_len[p] bytes at bytes + in_off[p].
 *
 * qfec_null_encrypt_batch replaces NullEncrypter::EncryptPacket
 *   (src/net/quic/core/crypto/null_encrypter.cc:28-47), called per packet by
 *   QuicPacketCreator::SerializePacket -> EncryptInPlace
 *   (quic_packet_creator.cc:549): out + out_off[p] receives in_len[p] + 12
 *   bytes, tag first.  out + out_off[p] may equal bytes + in_off[p] (in place,
 *   as EncryptInPlace does) or must not overlap any input.
 * qfec_null_decrypt_batch replaces NullDecrypter::DecryptPacket
 *   (crypto/null_decrypter.cc:38-64), called by QuicFramer::DecryptPayload
 *   (quic_framer.cc:1884): ok[p] = 1 and in_len[p] - 12 payload bytes at
 *   out + out_off[p] when the tag verifies; ok[p] = 0 and the output untouched
 *   when it does not (or in_len[p] < 12; with QFEC_SCRATCH_OUTPUT a failed
 *   packet's output holds its unverified plaintext).  Output must not overlap
 *   the input.
 * flags: QFEC_PTR_DEVICE / QFEC_PTR_HOST as above, QFEC_SCRATCH_OUTPUT. */
int qfec_null_encrypt_batch(qfec_ctx* ctx, const uint8_t* bytes, const uint64_t* ad_off,
                            const uint16_t* ad_len, const uint64_t* in_off,
                            const uint16_t* in_len, uint64_t n_packets, uint8_t* out,
                            const uint64_t* out_off, uint32_t flags);
int qfec_null_decrypt_batch(qfec_ctx* ctx, const uint8_t* bytes, const uint64_t* ad_off,
                            const uint16_t* ad_len, const uint64_t* in_off,
                            const uint16_t* in_len, uint64_t n_packets, uint8_t* out,
                            const uint64_t* out_off, uint8_t* ok, uint32_t flags);

/* ChaCha20-Poly1305 packet protection (the AEAD libquic negotiates, 12-byte
 * tags), batched like the NULL forms above.  Packet p is protected under key
 * key_idx[p]: keys holds 32 bytes per key, prefixes the 4-byte nonce prefix
 * per key; the 12-byte nonce is prefix || LE64(path_id[p] << 56 |
 * packet_number[p]) (path_id may be NULL: all 0).
 * qfec_chacha20poly1305_seal_batch replaces ChaCha20Poly1305Encrypter::
 *   EncryptPacket (AeadBaseEncrypter::EncryptPacket,
 *   src/net/quic/core/crypto/aead_base_encrypter.cc:107-134 -> BoringSSL
 *   EVP_aead_chacha20_poly1305): out + out_off[p] receives in_len[p] + 12
 *   bytes, ciphertext then tag; it may equal bytes + in_off[p] (in place).
 * qfec_chacha20poly1305_open_batch replaces ChaCha20Poly1305Decrypter::
 *   DecryptPacket (aead_base_decrypter.cc): ok[p] = 1 and in_len[p] - 12
 *   plaintext bytes at out + out_off[p] when the tag verifies; ok[p] = 0 and
 *   the output untouched otherwise.  Output must not overlap the input. */
int qfec_chacha20poly1305_seal_batch(qfec_ctx* ctx, const uint8_t* keys, const uint8_t* prefixes,
                                     const uint32_t* key_idx, const uint64_t* packet_number,
                                     const uint8_t* path_id, const uint8_t* bytes,
                                     const uint64_t* ad_off, const uint16_t* ad_len,
                                     const uint64_t* in_off, const uint16_t* in_len,
                                     uint64_t n_packets, uint8_t* out, const uint64_t* out_off,
                                     uint32_t flags);
int qfec_chacha20poly1305_open_batch(qfec_ctx* ctx, const uint8_t* keys, const uint8_t* prefixes,
                                     const uint32_t* key_idx, const uint64_t* packet_number,
                                     const uint8_t* path_id, const uint8_t* bytes,
                                     const uint64_t* ad_off, const uint16_t* ad_len,
                                     const uint64_t* in_off, const uint16_t* in_len,
                                     uint64_t n_packets, uint8_t* out, const uint64_t* out_off,
                                     uint8_t* ok, uint32_t flags);

/* AES-128-GCM packet protection (12-byte tags), same batch form as the
 * ChaCha20-Poly1305 calls above with 16-byte keys (keys holds 16 bytes per
 * key).  Replaces Aes128Gcm12Encrypter::EncryptPacket / Aes128Gcm12Decrypter::
 * DecryptPacket (crypto/aes_128_gcm_12_encrypter.cc -> AeadBaseEncrypter,
 * BoringSSL EVP_aead_aes_128_gcm).  Throughput is best when runs of 64
 * consecutive packets share a key (one GHASH table per wave); mixed-key runs
 * are correct but take a bit-serial GHASH. */
int qfec_aes128gcm_seal_batch(qfec_ctx* ctx, const uint8_t* keys, const uint8_t* prefixes,
                              const uint32_t* key_idx, const uint64_t* packet_number,
                              const uint8_t* path_id, const uint8_t* bytes, const uint64_t* ad_off,
                              const uint16_t* ad_len, const uint64_t* in_off,
                              const uint16_t* in_len, uint64_t n_packets, uint8_t* out,
                              const uint64_t* out_off, uint32_t flags);
int qfec_aes128gcm_open_batch(qfec_ctx* ctx, const uint8_t* keys, const uint8_t* prefixes,
                              const uint32_t* key_idx, const uint64_t* packet_number,
                              const uint8_t* path_id, const uint8_t* bytes, const uint64_t* ad_off,
                              const uint16_t* ad_len, const uint64_t* in_off,
                              const uint16_t* in_len, uint64_t n_packets, uint8_t* out,
                              const uint64_t* out_off, uint8_t* ok, uint32_t flags);

/* ---- packet-entropy bookkeeping (QUIC <= v33) --------------------------- */
/* The 1-byte entropy hashes the sender records per packet and checks acks
 * against, batched over connections.  Connection c
 * holds the hashes of its packets first_pn[c] .. first_pn[c] + n_c - 1 at
 * entropy[conn_ptr[c] .. conn_ptr[c+1]) — QuicSentEntropyManager's deque after
 * ClearEntropyBefore(first_pn[c]) — and cum_base[c] is the cumulative entropy
 * through first_pn[c] - 1 (NULL: 0).  A packet's hash is
 * entropy_flag << (packet_number % 8) (QuicFramer::GetPacketEntropyHash,
 * quic_framer.cc:351-354).
 *
 * qfec_entropy_cumulative_batch: cum[i] = cum_base[c] ^ entropy[conn_ptr[c]]
 *   ^ ... ^ entropy[i] — QuicSentEntropyManager::GetCumulativeEntropy for every
 *   packet (quic_sent_entropy_manager.cc:33-41, :57-66); with 0 for packets not
 *   received it is the receiver's EntropyTracker::EntropyHash
 *   (quic_received_packet_manager.cc:40-56).  n_packets = conn_ptr[n_conns] -
 *   conn_ptr[0] is a launch-shape hint (lanes per connection from the mean
 *   window); 0 = unknown.  It never changes the result.
 * qfec_entropy_validate_batch: ack a of connection ack_conn[a] with
 *   largest_observed[a], missing packets as the disjoint intervals
 *   [range_lo[r], range_hi[r]), r in range_ptr[a] .. range_ptr[a+1] (the
 *   PacketNumberQueue), and the claimed hash: ok[a] = IsValidEntropy(...)
 *   (quic_sent_entropy_manager.cc:68-96, called by QuicConnection::
 *   ValidateAckFrame, quic_connection.cc:854), given `cum` from the first call.
 *   Where the reference's behaviour is undefined — a missing packet above the
 *   largest recorded one, largest_observed below the window, ack_conn out of
 *   range — ok[a] = 0.  An invalid ack is a result (ok = 0), not an error. */
int qfec_entropy_cumulative_batch(qfec_ctx* ctx, const uint8_t* entropy, const uint64_t* conn_ptr,
                                  const uint8_t* cum_base, uint64_t n_conns, uint64_t n_packets,
                                  uint8_t* cum, uint32_t flags);
int qfec_entropy_validate_batch(qfec_ctx* ctx, const uint8_t* cum, const uint64_t* conn_ptr,
                                const uint64_t* first_pn, const uint8_t* cum_base,
                                uint64_t n_conns, const uint32_t* ack_conn,
                                const uint64_t* largest_observed, const uint8_t* claimed,
                                const uint32_t* range_ptr, const uint64_t* range_lo,
                                const uint64_t* range_hi, uint64_t n_acks, uint8_t* ok,
                                uint32_t flags);

/* ---- measurement support (bench.py, device pointers) ------------------- */
/* Streaming bandwidth probe over n bytes of src (n rounded down to 16):
 * mode 0 = read only (nt loads, XOR-folded; dst receives at most 16 bytes),
 * mode 1 = copy src -> dst (nt loads + nt stores).  The measured ceilings the
 * FEC kernels' rates are compared with. */
int qfec_stream_probe(qfec_ctx* ctx, const uint8_t* src, uint64_t n, uint8_t* dst, int mode);
/* Number of phased fixed-shape launches on this context that gave up their
 * grid-wide meetings (a workgroup waited > 200 us: the GPU shared with other
 * work, so not every workgroup was resident) and ran to the end without them
 * — same results, one-pass-like speed.  Waits for the context's stream. */
int qfec_phase_abandons(qfec_ctx* ctx, uint32_t* count);
/* Large fixed-shape batches left to run with the one-pass kernel because a
 * phased launch of this context was abandoned (the GPU is contended: the
 * context then uses the one-pass kernel for the next 16 such batches and
 * tries the phased one again).  -1 for a null context. */
int qfec_phase_backoff(qfec_ctx* ctx);
/* Which kernel the context's last device-pointer fixed-shape call ran: 1 the
 * phased kernel, 0 the one-pass kernel, -1 none yet (or a null context).
 * The measurement names its roofline kernel from this, not from a copy of
 * the library's size rule. */
int qfec_last_fixed_phased(const qfec_ctx* ctx);
/* Test hook: the workgroup count of the last device fixed-shape launch if it
 * ran phased (one per CU, less the CUs other contexts' resident small-batch
 * workers hold), else 0. */
uint32_t qfec_debug_last_phase_grid(const qfec_ctx* ctx);
/* Test hook: launch `extra` workgroups beyond one per CU in phased launches
 * (0..64; they cannot all be resident, so the first meeting times out — the
 * abandon path; the backoff does not apply while extra > 0), and with
 * reset_backoff clear the contention backoff (forgetting abandoned launches
 * so far).  Waits for the stream. */
int qfec_debug_phase(qfec_ctx* ctx, uint32_t extra, int reset_backoff);
/* Test hook: fixed-shape batches of at least `min_phases` phases (a phase is
 * one workgroup per CU x 8 steps x the groups per workgroup step) run the
 * phased kernel; 0 restores the default (6 phases, about 184K headline
 * groups).  1 forces it for any batch, 0xFFFFFFFF never. */
int qfec_debug_phase_min(qfec_ctx* ctx, uint32_t min_phases);
/* Test hook: on == 0 runs phased launches without their register-held steps
 * (40 LDS steps per phase only, more phases); 1 restores the default.  For
 * the per-group-size A/B; results are identical. */
int qfec_debug_phase_regsteps(qfec_ctx* ctx, int on);
/* Test hook: the load batch of the runtime-k phased body (group sizes above
 * 16): 16 or 32 (0 restores the library's measured per-operation choice:
 * encode 16, recover 32 up to k = 32).  For the per-group-size A/B
 * (DESIGN.md §4); results are identical. */
int qfec_debug_phase_rtbatch(qfec_ctx* ctx, uint32_t batch);
/* Test hook: phased launches leave `cus` more CUs out of their grid (0..64),
 * as if other contexts' small-batch workers held them -- the A/B of the
 * round-6 CU arbitration; results are identical. */
int qfec_debug_phase_reserve(qfec_ctx* ctx, uint32_t cus);
/* Test hook: the CUs a phased launch on ctx would leave to other contexts'
 * small-batch workers now; *why (nullable) gets why they count (bit 0 a job
 * or warm in the last 2 ms, bit 1 a worker alive, bit 2 its stream busy). */
uint32_t qfec_debug_other_service_cus(qfec_ctx* ctx, uint32_t* why);
/* Test hook: mode 1 makes every key of qfec_assign_slots start probing at the
 * LAST entry of the call's table (one chain through the wrap to entry 0: the
 * longest probe and the wrap, which no choice of keys reaches from outside);
 * mode 0 restores the hash.  Results are identical. */
int qfec_debug_assign_probe(qfec_ctx* ctx, int mode);
/* Test hook: fail != 0 makes every ragged call on this context fail with
 * QFEC_ERR_INTERNAL before touching the device (the GPU-failure path of the
 * connection integration: groups go without FEC). */
int qfec_debug_fail_launches(qfec_ctx* ctx, int on);

/* Small-batch service (round 4): QFEC_PTR_MAPPED ragged batches of at most 16
 * groups are taken by a resident worker kernel from a ring in host-mapped
 * memory instead of a kernel launch each; the worker leaves after 100 us
 * without work (or before a phased launch of its context) and is relaunched
 * by the next such batch.  on = 1 / 0
 * enables / disables it (0 also makes a running worker leave; -1 leaves the
 * setting; 2 enables it and writes the NEXT job's ring entry with a wrong job
 * number -- a malformed ring, whose job must fail with QFEC_ERR_INTERNAL and
 * turn the service off rather than report stale output); stats (may be NULL)
 * receives {worker launches, jobs finished, worker alive}; on = 3 leaves the
 * setting and fills stats[0..5] with those plus {worker stream busy, us since
 * the context's last service job or warm (the view the phased launches of
 * other contexts take of it), workers stopped for their 2-ms residency bound}.  Test / measurement hook; the service is on by
 * default.  Any failed service job turns the service off for the context
 * (small batches then launch). */
int qfec_debug_service(qfec_ctx* ctx, int on, uint64_t* stats);
/* Measurement hook of the service: on = 1 / 0 makes the worker record
 * 100-MHz wall-clock stamps of each job it finishes (-1 leaves the
 * setting); stamps (may be NULL, 6 entries) receives the last job's: work
 * seen, ring entry and tables in LDS, wave 0's first group done, every group
 * done, outputs made visible, token stored.  (Worker launched by a later
 * job picks the setting up at its start.) */
int qfec_debug_service_stamps(qfec_ctx* ctx, int on, uint64_t* stamps);
/* Measurement hook (round 6; stamps on through qfec_debug_service_stamps):
 * the last service job end to end, 44 words: [0..5] the leader's stamps as
 * above, [6] when the token was stored and [7] by which workgroup; [8 + 4w ..]
 * workgroup w's share: entry in LDS, groups done, outputs visible, counted
 * (100-MHz ticks); [40..43] the host's steady-clock ns of the last service
 * call: entry, job published, token seen, return. */
int qfec_debug_service_trace(qfec_ctx* ctx, uint64_t* out);
/* Measurement hook (round 6): on = 1 starts a native thread that owns ctx
 * (the caller must not use ctx until it is stopped) and flushes one-group
 * mapped batches of 10 x 1350 B in loop turns 20 us apart, warming the
 * small-batch worker at each turn's start; on = 0 stops it and returns its code, with stats
 * (nullable) = {batches flushed, batches whose parity was wrong}. */
int qfec_debug_service_feed(qfec_ctx* ctx, int on, uint64_t* stats);
/* Test hook: hold != 0 keeps the service's follower workgroups waiting at
 * their start (as if dispatched late behind another kernel) until it is
 * cleared; the leader runs on.  A split job's token then waits for them. */
int qfec_debug_service_hold(qfec_ctx* ctx, int hold);
/* Test hook (round 6): the small-batch worker's residency bound, ns (default
 * 2,000,000; 0 rotates the worker at every job published while it runs --
 * the successor queued behind it, no wait); returns the previous bound, or 0
 * for a null ctx. */
uint64_t qfec_debug_service_resident(qfec_ctx* ctx, uint64_t ns);
/* Test hook (round 6): the small-batch worker's idle time in us (default
 * 100), for workers launched from now on; returns the previous value, or 0
 * for a null ctx.  (A test that holds the followers back keeps the leader
 * resident with it: a leader that idles out meanwhile has its successor
 * queued behind the held kernel.) */
uint64_t qfec_debug_service_idle(qfec_ctx* ctx, uint64_t us);

/* ---- synthetic inputs (bench / parity-test support, device pointers) ---- */
/* Counter-based bytes: byte j of packet (g, i) is little-endian byte j%8 of
 * splitmix64(seed ^ ((g*256 + i) << 32) ^ (j/8)) — generated on the device so
 * that host and device agree without a 14 GB transfer.
 * Fills groups g0 .. g0+n_groups-1 into rows[(g-g0)*group_stride + i*row_stride]. */
int qfec_synth_fixed(qfec_ctx* ctx, uint8_t* rows, uint32_t k, uint32_t L, uint64_t row_stride,
                     uint64_t group_stride, uint64_t g0, uint64_t n_groups, uint64_t seed);
/* Fill the packets of a ragged CSR batch whose group g (global index g0+g)
 * packet i has pkt_len[grp_ptr[g]+i] bytes at pkt_off[...]. */
int qfec_synth_ragged(qfec_ctx* ctx, uint8_t* bytes, const uint64_t* pkt_off,
                      const uint16_t* pkt_len, const uint32_t* grp_ptr, uint64_t g0,
                      uint64_t n_groups, uint64_t seed);

#ifdef __cplusplus
}
#endif
#endif /* QFEC_H_ */
