// qfec_internal.h — launch interface between the C-ABI (qfec_capi.cpp) and
// the gfx950 kernels (qfec_kernels.hip: the XOR path; qturn_kernels.hip: the
// table passes of the receiver's turn; qpp_kernels.hip, qent_kernels.hip).
// Host and device compilers both read it: no device intrinsics here (the
// device code that kernel files share is in qfec_device.h).  Not installed; not
// part of the ABI.
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace qfec {

// Bits latched into the context's device error word by kernels.
enum : uint32_t {
  kErrMissingIndex = 1u,  // missing_idx >= k; accumulate: slot >= n_slots; admit: slot >=
                          // n_slots or pkt_idx > K; tracked revive: slot >= n_slots
  kErrPacketLength = 2u,  // ragged packet length 0 or > kMaxPacketSize, or > parity_len
                          // (accumulate, admit: > min(kMaxPacketSize, acc_stride))
  kErrGroupSize = 4u,     // ragged group with 0 or > 255 packets (accumulate, admit: > 255);
                          // admit, tracked revive: slot_k 0 or its map beyond map_stride
  kErrParityLength = 8u,  // ragged parity_len 0 or > kMaxPacketSize; accumulate, admit:
                          // acc_len > min(kMaxPacketSize, acc_stride)
};

// Fixed-shape encode / recover.  parity == nullptr selects encode.
// Most workgroups of 256 lanes per launch: an AQL dispatch packet's grid size
// is a 32-bit count of work-items (2^32 / 256 = 2^24 workgroups).
constexpr uint64_t kMaxBlocks256 = (1ull << 24) - 1;

struct FixedArgs {
  const uint8_t* rows;
  const uint8_t* parity;   // recover only: parity rows
  const uint8_t* missing;  // recover only: lost slot per group
  uint8_t* out;
  uint64_t row_stride;
  uint64_t group_stride;
  uint64_t parity_stride;
  uint64_t out_stride;
  uint64_t n_groups;
  uint32_t k;
  uint32_t L;
  uint32_t* err;
  // large nt batches: 19 x 256 B of zeroed sync words for the phased kernel
  // (phase_xor_kernel); nullptr: always the one-pass fixed kernel
  uint32_t* phase_sync = nullptr;
  // phased kernel: the device's CU count (cached by the context: one
  // workgroup per CU), extra workgroups beyond it (test hook: forces the
  // abandon path), and a host-mapped word the last workgroup out copies the
  // abandoned-launch count into (nullable) — the context reads it at the next
  // launch without a synchronisation
  uint32_t ncu = 0;
  uint32_t phase_extra = 0;
  uint32_t* phase_host = nullptr;
  // minimum phase count for the phased kernel (0: kPhMinPhases, about 184K
  // headline groups); test hook qfec_debug_phase_min, for the band study
  uint32_t phase_min = 0;
  // steps per phase of the launch (set by launch_fixed: the batch spread
  // evenly over its phases); 0 = the kernel's full phase
  uint32_t phase_steps = 0;
  // test hook (qfec_debug_phase_regsteps): phased launches without the
  // register-held steps (the A/B of DESIGN.md §4's per-k table)
  uint32_t no_regsteps = 0;
  // CUs held by resident small-batch service workers of OTHER contexts on the
  // device (round 6): the phased grid leaves them free
  uint32_t svc_cus = 0;
  // test hook (qfec_debug_phase_rtbatch): the runtime-k phased body's load
  // batch (0: the per-operation choice, phase_rt_batch; 16 or 32)
  uint32_t rt_batch = 0;
  // in-slot recover written in place (qfec_recover_inslot_batch with out ==
  // NULL; encode form, parity == nullptr): group g's output row is its own
  // row inplace_missing[g], which holds the redundancy on entry; nullptr: out
  const uint8_t* inplace_missing = nullptr;
};

// Revive from per-group receive maps (qfec_revive_batch; layout as
// include/qfec.h).  The scratch pointers are context-owned device memory laid
// out by revive_scratch_bytes: nothing of a call's intermediate state (the
// revived count included) ever reaches the host.
constexpr uint32_t kReviveTile = 256;    // groups per classify workgroup (one lane each)
constexpr uint32_t kReviveListPad = 8;   // work-list entries readable past the revived count
struct ReviveArgs {
  uint8_t* rows;
  const uint8_t* parity;
  const uint8_t* received;
  uint8_t* out;  // nullptr: in place, rows[g][m] receives the revived packet
  uint64_t row_stride;
  uint64_t group_stride;
  uint64_t parity_stride;
  uint64_t map_stride;
  uint64_t out_stride;
  uint64_t n_groups;
  uint32_t k;
  uint32_t L;
  uint8_t* status;
  uint8_t* revived_idx;    // nullable
  uint64_t* revived_list;  // nullable
  uint64_t* counts;        // nullable: [complete, revived, unrevivable]
  // scratch: per classify tile its packed counts (revived | complete << 16)
  // and the revived groups before it; the three totals; the work list, entry
  // i = g << 8 | m of the i-th revived group, n_groups + kReviveListPad long
  uint32_t* tile_cnt;
  uint64_t* tile_off;
  uint64_t* totals;
  uint64_t* work;
  uint32_t ncu;  // the device's CU count (sizes the revive grid)
};
inline uint64_t revive_tiles(uint64_t n_groups) {
  return (n_groups + kReviveTile - 1) / kReviveTile;
}
// Bytes of scratch for n_groups, and the four pointers into a block of them
// (Args: any of the revive argument structs; they name the four alike).
inline uint64_t revive_scratch_bytes(uint64_t n_groups) {
  return 32 + (n_groups + kReviveListPad) * 8 + revive_tiles(n_groups) * 12;
}
template <typename Args>
inline void revive_scratch_layout(Args& a, void* block) {
  uint8_t* p = static_cast<uint8_t*>(block);
  a.totals = reinterpret_cast<uint64_t*>(p);
  a.work = reinterpret_cast<uint64_t*>(p + 32);
  a.tile_off = a.work + a.n_groups + kReviveListPad;
  a.tile_cnt = reinterpret_cast<uint32_t*>(a.tile_off + revive_tiles(a.n_groups));
}
// Four launches on s (classify, scan, emit, revive), ordered by the stream
// alone.  n_groups > 0.
hipError_t launch_revive(const ReviveArgs& a, bool nontemporal, hipStream_t s);

// True if launch_fixed(a, nontemporal, ...) runs the phased kernel; *grid
// (nullable): its workgroup count.
bool fixed_uses_phases(const FixedArgs& a, bool nontemporal, uint32_t* grid = nullptr);

struct RaggedArgs {
  const uint8_t* bytes;
  const uint64_t* pkt_off;
  const uint16_t* pkt_len;
  const uint32_t* grp_ptr;
  const uint8_t* parity;      // recover: parity bytes
  const uint64_t* parity_off; // encode: where to write; recover: where to read
  const uint16_t* parity_len; // recover: lengths in
  uint16_t* parity_len_out;   // encode: lengths out
  const uint8_t* missing;     // recover
  uint8_t* out;               // encode: parity_out; recover: revived packets
  const uint64_t* out_off;    // recover
  uint64_t n_groups;
  uint32_t* err;
  // launch_ragged_latency only (nullptr: none): the last workgroup to finish
  // stores done_token into done_flag (mapped host memory, system scope) after
  // every output is visible; done_count is a zeroed device word it resets
  uint32_t* done_count;
  uint32_t* done_flag;
  uint32_t done_token;
};

// Revive from per-group receive maps over a ragged CSR batch
// (qfec_revive_ragged): the RaggedArgs tables of a recover, the maps and the
// outputs / scratch of ReviveArgs.  A struct of its own: a field added to
// ReviveArgs would move the kernarg offsets of the fixed-shape revive kernels.
struct ReviveRaggedArgs {
  const uint8_t* bytes;
  const uint64_t* pkt_off;
  const uint16_t* pkt_len;
  const uint32_t* grp_ptr;
  const uint8_t* parity;
  const uint64_t* parity_off;
  const uint16_t* parity_len;
  uint8_t* out;
  const uint64_t* out_off;
  const uint8_t* received;
  uint64_t map_stride;
  uint64_t n_groups;  // < 2^32 (packet indices are 32 bits)
  uint8_t* status;
  uint8_t* revived_idx;    // nullable
  uint64_t* revived_list;  // nullable
  uint64_t* counts;        // nullable: [complete, revived, unrevivable]
  // scratch, as ReviveArgs (revive_scratch_bytes(n_groups))
  uint32_t* tile_cnt;
  uint64_t* tile_off;
  uint64_t* totals;
  uint64_t* work;
  uint32_t* err;
  uint32_t ncu;
};
// Four launches on s (classify, scan, emit, the ragged block body over the
// work list), ordered by the stream alone.  n_groups > 0.
hipError_t launch_revive_ragged(const ReviveRaggedArgs& a, hipStream_t s);

// Fold a turn's packets into running group parities (qfec_accumulate_ragged):
// the CSR tables of an encode; group g folds into row acc + s * acc_stride of
// length acc_len[s], s = slot[g] (slot == nullptr: s = g).  A struct of its
// own, like ReviveRaggedArgs: RaggedArgs keeps its kernarg layout.
struct AccumulateRaggedArgs {
  const uint8_t* bytes;
  const uint64_t* pkt_off;
  const uint16_t* pkt_len;
  const uint32_t* grp_ptr;
  uint8_t* acc;
  uint64_t acc_stride;
  uint16_t* acc_len;     // read on entry, written on exit
  const uint32_t* slot;  // nullable
  uint64_t n_groups;     // < 2^32
  uint32_t n_slots;
  uint32_t lim;          // min(kMaxPacket, acc_stride): longest packet / row
  uint32_t* err;
  // set by launch_accumulate_ragged (a batch beyond one grid is launched in
  // parts): the identity slot of the part's group 0
  uint32_t slot_base = 0;
};
// The ragged block body, 8 groups per block: one launch on s per
// 8 * kMaxBlocks256 groups.  n_groups > 0.
hipError_t launch_accumulate_ragged(const AccumulateRaggedArgs& a, hipStream_t s);

// Close running rows (qfec_emit_accumulated / qfec_revive_accumulated): group
// g's row is acc + s * acc_stride of length acc_len[s], s = slot[g] (slot ==
// nullptr: s = g), as AccumulateRaggedArgs names it.  A struct of its own:
// ReviveArgs, ReviveRaggedArgs and AccumulateRaggedArgs keep their kernarg
// layouts.  The emit reads acc .. slot, n_groups, out .. out_len, err, n_slots,
// lim and release (a flag); the revive all of it (release: bit st set = groups
// of status st are released).
// Work-list entry of the revive: g << 8 | m as ReviveRaggedArgs's, and the
// length to copy (11 bits; 0: copy nothing) from bit kCloseLenShift on -- the
// pass that releases a slot is the one that captures its length.
constexpr uint32_t kCloseLenShift = 40;
struct CloseArgs {
  const uint8_t* acc;
  uint64_t acc_stride;
  uint16_t* acc_len;     // read; zeroed for released slots
  const uint32_t* slot;  // nullable
  // K and the receive maps, map_stride apart.  CloseArgs: per GROUP
  // (group_k[g], received + g * map_stride).  TrackedCloseArgs: per SLOT
  // (the call's slot_k[s] and acc_map + s * map_stride)
  const uint8_t* group_k;
  const uint8_t* received;
  uint64_t map_stride;
  uint64_t n_groups;  // < 2^32
  uint8_t* out;       // revive: nullable (the revived packet is the row)
  const uint64_t* out_off;
  uint16_t* out_len;
  uint8_t* status;
  uint8_t* revived_idx;    // nullable
  uint64_t* revived_list;  // nullable
  uint64_t* counts;        // nullable: [complete, revived, unrevivable]
  // scratch, as ReviveArgs (revive_scratch_bytes(n_groups))
  uint32_t* tile_cnt;
  uint64_t* tile_off;
  uint64_t* totals;
  uint64_t* work;
  uint32_t* err;
  uint32_t n_slots;
  uint32_t lim;  // min(kMaxPacket, acc_stride): longest row
  uint32_t release;
  uint32_t ncu;
};
// One launch on s: the gather over every group.  n_groups > 0.
hipError_t launch_close_emit(const CloseArgs& a, hipStream_t s);
// Four launches on s (classify, scan, emit, the gather over the work list;
// three when out == nullptr), ordered by the stream alone.  n_groups > 0.
hipError_t launch_close_revive(const CloseArgs& a, hipStream_t s);

// qfec_revive_tracked: CloseArgs's revive with K and the map read by SLOT
// (group_k[s], received + s * map_stride) and a slot of length 0 counting as
// an all-clear map.  The same layout under a type of its own, which selects
// the by-slot classify hooks; the gather over the work list is CloseArgs's own
// kernel and takes these arguments as the CloseArgs they are.
struct TrackedCloseArgs : CloseArgs {};
// Launches as launch_close_revive.  n_groups > 0.
hipError_t launch_tracked_revive(const TrackedCloseArgs& a, hipStream_t s);

// The first three launches of the four revives above (classify, scan, emit):
// the work list and its length, left on the device.  Defined with the turn
// passes (qturn_kernels.hip); the launch_*revive* functions call it and then
// launch their own kernel over the list (qfec_kernels.hip).  n_groups > 0.
hipError_t launch_revive_passes(const ReviveArgs& a, hipStream_t s);
hipError_t launch_revive_passes(const ReviveRaggedArgs& a, hipStream_t s);
hipError_t launch_revive_passes(const CloseArgs& a, hipStream_t s);
hipError_t launch_revive_passes(const TrackedCloseArgs& a, hipStream_t s);

// qfec_admit_ragged: filter a turn's candidates against the per-slot running
// maps and the open call's ok flags, and write the CSR tables the accumulate
// folds (layout and rule as include/qfec.h).  Verdict codes: QFEC_PKT_*.
// Scratch, inside a revive_scratch_bytes(n_groups) block: per group its
// admitted count (in the work list's place, which also holds the four verdict
// counts of every tile of kReviveTile groups behind them), per tile the
// admitted packets of the tiles before it.
struct AdmitArgs {
  const uint64_t* pkt_off;
  const uint16_t* pkt_len;
  const uint8_t* pkt_idx;
  const uint8_t* pkt_ok;  // nullable: all verified
  const uint32_t* grp_ptr;
  const uint32_t* slot;  // nullable
  const uint8_t* slot_k;
  uint8_t* acc_map;
  uint64_t map_stride;
  const uint16_t* acc_len;
  uint64_t n_groups;  // < 2^32
  uint32_t* grp_ptr_out;
  uint64_t* pkt_off_out;
  uint16_t* pkt_len_out;
  uint8_t* verdict;
  uint64_t* counts;  // nullable: [admitted, failed, duplicate, invalid]
  uint32_t* grp_cnt;   // scratch: n_groups
  uint32_t* tile_v;    // scratch: 4 per tile
  uint64_t* tile_off;  // scratch: 1 per tile
  uint32_t* err;
  uint32_t n_slots;
  uint32_t lim;  // min(kMaxPacket, acc_stride): longest packet / row
};
inline void admit_scratch_layout(AdmitArgs& a, void* block) {
  uint8_t* p = static_cast<uint8_t*>(block);
  a.grp_cnt = reinterpret_cast<uint32_t*>(p + 32);
  a.tile_v = a.grp_cnt + a.n_groups;
  a.tile_off = reinterpret_cast<uint64_t*>(p + 32) + a.n_groups + kReviveListPad;
}
// the work list's (n_groups + kReviveListPad) * 8 bytes hold both tables: a
// full tile's 16 bytes fit the 4 bytes per group its counts leave, the last
// tile's fit the pad
static_assert(kReviveTile * 4 >= 16 && kReviveListPad * 8 >= 16,
              "n_groups * 4 + tiles * 16 <= (n_groups + kReviveListPad) * 8");
// Three launches on s (decide, scan, scatter), ordered by the stream alone.
// n_groups > 0.
hipError_t launch_admit_ragged(const AdmitArgs& a, hipStream_t s);

// qfec_bin_arrivals: a turn's per-packet records in arrival order to the
// per-slot CSR tables the admit reads (layout and rule as include/qfec.h).
// Scratch, a block of bin_scratch_bytes(n_packets, n_slots) in the revive
// calls' allocation: the three tallies (binned, no slot, out of range) and a
// counter per slot, zeroed together in front of the kernels; a 16-byte record
// and a provisional rank per packet; a word per tile of kReviveTile slots.
constexpr uint32_t kBinNoSlot = 0xFFFFFFFFu;  // QFEC_NO_SLOT
struct BinArgs {
  const uint32_t* pkt_slot;
  const uint64_t* pkt_off;  // carried, never dereferenced
  const uint16_t* pkt_len;
  const uint8_t* pkt_idx;
  const uint8_t* pkt_ok;  // nullable: pkt_ok_out is not written
  uint64_t n_packets;     // 0 < n_packets < 2^32
  uint32_t n_slots;       // > 0
  uint32_t* grp_ptr_out;
  uint64_t* pkt_off_out;
  uint16_t* pkt_len_out;
  uint8_t* pkt_idx_out;
  uint8_t* pkt_ok_out;
  uint32_t* src_out;  // nullable
  uint64_t* counts;   // nullable: [binned, no slot, out of range]
  unsigned long long* tally;  // scratch: 3 (+ 1 of padding)
  uint32_t* cnt;              // scratch: n_slots
  uint4* rec;                 // scratch: n_packets, 16-byte aligned
  uint32_t* rank;             // scratch: n_packets
  uint32_t* tile_off;         // scratch: 1 per tile of slots
  uint32_t* err;
  uint32_t ncu;
};
// the tallies and the counters: what the memset in front of the kernels clears
inline uint64_t bin_scratch_zeroed(uint64_t n_slots) { return 32 + n_slots * 4; }
inline uint64_t bin_scratch_bytes(uint64_t n_packets, uint64_t n_slots) {
  return ((bin_scratch_zeroed(n_slots) + 15) & ~15ull) + n_packets * 20 +
         revive_tiles(n_slots) * 4;
}
inline void bin_scratch_layout(BinArgs& a, void* block) {
  uint8_t* p = static_cast<uint8_t*>(block);
  a.tally = reinterpret_cast<unsigned long long*>(p);
  a.cnt = reinterpret_cast<uint32_t*>(p + 32);
  a.rec = reinterpret_cast<uint4*>(p + ((bin_scratch_zeroed(a.n_slots) + 15) & ~15ull));
  a.rank = reinterpret_cast<uint32_t*>(a.rec + a.n_packets);
  a.tile_off = a.rank + a.n_packets;
}
// One memset and six launches on s (count, tile, scan, ptr, scatter, order),
// ordered by the stream alone.  n_packets > 0, n_slots > 0.
hipError_t launch_bin_arrivals(const BinArgs& a, hipStream_t s);

// qfec_assign_slots: every packet's 64-bit group key to the slot of its open
// group, or to a free slot it opens (rule as include/qfec.h).  Scratch, a block
// of assign_scratch_bytes(n_packets, n_slots) in the revive calls' allocation:
// an open-addressing table of 16-byte entries (key, value, first arrival) that
// one memset to 0xFF empties in front of the kernels and nothing keeps between
// calls; the entry index per packet; the ascending list of free slots; a word
// per tile of kReviveTile slots and per tile of kReviveTile packets; 16 bytes
// of totals.
constexpr unsigned long long kAssignNoKey = 0xFFFFFFFFFFFFFFFFull;  // QFEC_NO_KEY, an empty entry
constexpr uint32_t kAssignNone = 0xFFFFFFFFu;  // no value, no first arrival, no entry
struct AssignArgs {
  const unsigned long long* pkt_key;
  const uint8_t* pkt_k;
  uint64_t n_packets;  // 0 < n_packets < 2^32
  unsigned long long* slot_key;
  uint8_t* slot_k;
  const uint16_t* acc_len;
  uint32_t n_slots;  // may be 0
  uint32_t* pkt_slot_out;
  unsigned long long* counts;  // nullable: [open, new, no key, opened, turned away]
  unsigned long long* table;   // scratch: 2 words per entry (key; value | first << 32)
  uint32_t cap_mask;           // entries - 1, entries a power of two
  uint32_t probe_last;         // test hook: every probe starts at the last entry
  uint32_t* ent;               // scratch: n_packets
  uint32_t* free_list;         // scratch: n_slots
  uint32_t* free_tile;         // scratch: 1 per tile of slots
  uint32_t* open_tile;         // scratch: 1 per tile of packets
  uint32_t* totals;            // scratch: [free slots] (+ 3 of padding)
  uint32_t* err;
  uint32_t ncu;
};
// entries: a power of two, at least 16 and at least twice the keys that can be
// inserted (every open slot's and every packet's); 0 if that passes 2^31 entries
inline uint64_t assign_table_entries(uint64_t n_packets, uint64_t n_slots) {
  uint64_t cap = 16;
  while (cap < 2 * (n_packets + n_slots)) cap <<= 1;
  return cap <= (1ull << 31) ? cap : 0;
}
inline uint64_t assign_scratch_bytes(uint64_t n_packets, uint64_t n_slots) {
  return assign_table_entries(n_packets, n_slots) * 16 + (n_packets + n_slots) * 4 +
         (revive_tiles(n_packets) + revive_tiles(n_slots)) * 4 + 16;
}
inline void assign_scratch_layout(AssignArgs& a, void* block) {
  const uint64_t cap = assign_table_entries(a.n_packets, a.n_slots);
  a.table = static_cast<unsigned long long*>(block);
  a.cap_mask = (uint32_t)(cap - 1);
  a.ent = reinterpret_cast<uint32_t*>(a.table + 2 * cap);
  a.free_list = a.ent + a.n_packets;
  a.free_tile = a.free_list + a.n_slots;
  a.open_tile = a.free_tile + revive_tiles(a.n_slots);
  a.totals = a.open_tile + revive_tiles(a.n_packets);
}
// One memset and seven launches on s (slots, probe, tile, scan, free, open,
// emit), ordered by the stream alone.  n_packets > 0.
hipError_t launch_assign_slots(const AssignArgs& a, hipStream_t s);

// qfec_retire_groups: per-connection watermarks raised, the max_groups highest
// groups of every connection kept, the open slots below their mark closed and
// the packets below it masked, in front of the assign (rule as include/qfec.h).
// Scratch, a block of retire_scratch_bytes(n_conns, n_slots, max_groups) in the
// revive calls' allocation: eight tallies and, with max_groups > 0, max_groups
// + 1 words per connection (round r's word: the r-th largest live number + 1,
// 0 = none), zeroed together in front of the kernels; a word per tile of
// kReviveTile slots.
constexpr uint32_t kRetireMaxGroups = 16;
constexpr uint64_t kRetireTallyBytes = 64;
struct RetireArgs {
  const unsigned long long* pkt_key;  // nullable with n_packets == 0
  uint64_t n_packets;                 // < 2^32
  const unsigned long long* slot_key;
  uint16_t* acc_len;
  uint32_t n_slots;  // may be 0
  unsigned long long* conn_mark;
  uint32_t n_conns;     // may be 0: every key is out of range
  uint32_t key_shift;   // 1..63
  uint32_t max_groups;  // <= kRetireMaxGroups; 0: no bound
  uint32_t round;       // the retain pass this launch runs, 0 .. max_groups
  const uint32_t* raise_conn;
  const unsigned long long* raise_mark;
  uint32_t n_raise;
  unsigned long long* pkt_key_out;  // may be pkt_key
  uint32_t* closed_list;            // nullable
  unsigned long long* counts;  // nullable: [closed, refused, no key, passed, out of range]
  unsigned long long* tally;   // scratch: 8, [1..4] as counts
  unsigned long long* top;     // scratch: (max_groups + 1) * n_conns, round-major
  uint32_t* tile_off;          // scratch: 1 per tile of slots
  uint32_t* err;
  uint32_t ncu;
};
// the tallies and the round words: what the memset in front of the kernels clears
inline uint64_t retire_scratch_zeroed(uint64_t n_conns, uint32_t max_groups) {
  return kRetireTallyBytes + (max_groups ? (uint64_t)(max_groups + 1) * n_conns * 8 : 0);
}
inline uint64_t retire_scratch_bytes(uint64_t n_conns, uint64_t n_slots, uint32_t max_groups) {
  return retire_scratch_zeroed(n_conns, max_groups) + revive_tiles(n_slots) * 4;
}
inline void retire_scratch_layout(RetireArgs& a, void* block) {
  uint8_t* p = static_cast<uint8_t*>(block);
  a.tally = reinterpret_cast<unsigned long long*>(p);
  a.top = reinterpret_cast<unsigned long long*>(p + kRetireTallyBytes);
  a.tile_off = reinterpret_cast<uint32_t*>(p + retire_scratch_zeroed(a.n_conns, a.max_groups));
}
// One memset and up to max_groups + 7 launches on s (raise, the retain rounds,
// mark, filter, classify, scan, close), ordered by the stream alone.  Not all
// of n_packets, n_slots and n_raise are 0.
hipError_t launch_retire_groups(const RetireArgs& a, hipStream_t s);

// qfec_parse_opened: QuicFramer::ProcessAuthenticatedHeader over the opened
// packets of a turn, in front of the retire (rule as include/qfec.h).  No
// scratch: the six tallies are added into counts, zeroed in front of the pass.
constexpr uint32_t kHdrFailed = 0x80, kHdrNoFlags = 0x81, kHdrIllegalFlags = 0x82,
                   kHdrNoOffset = 0x83, kHdrBadOffset = 0x84, kHdrRange = 0x85, kHdrEmpty = 0x86;
constexpr uint32_t kPrivateFlagEntropy = 1, kPrivateFlagFecGroup = 2, kPrivateFlagFec = 4;
struct ParseArgs {
  const uint8_t* bytes;
  const uint64_t* pkt_off;
  const uint16_t* pkt_len;
  const unsigned long long* packet_number;
  const uint32_t* pkt_conn;
  const uint8_t* pkt_ok;  // nullable: all verified
  uint64_t n_packets;     // 0 < n_packets < 2^32
  uint32_t max_flags;     // the version's highest legal flags byte: 7 or 1
  uint32_t key_shift;     // 1..63
  unsigned long long* pkt_key_out;
  uint8_t* pkt_idx_out;
  uint64_t* body_off_out;
  uint16_t* body_len_out;
  uint8_t* hdr_out;
  uint8_t* entropy_out;        // nullable
  unsigned long long* counts;  // nullable: [data, FEC, no group, failed, rejected, range]
  uint32_t* err;
  uint32_t ncu;
};
// One memset (with counts) and one launch on s.  n_packets > 0.
hipError_t launch_parse_opened(const ParseArgs& a, hipStream_t s);

// qfec_write_private_headers: WriteFecPrivateHeader over a batch.
struct WriteHeadersArgs {
  uint8_t* bytes;
  const uint64_t* pkt_off;
  const uint8_t* hdr;
  const uint8_t* fec_offset;
  uint64_t n_packets;  // 0 < n_packets < 2^32
  uint32_t max_flags;
  uint64_t* body_off_out;      // nullable
  unsigned long long* counts;  // nullable: [written, refused]
  uint32_t* err;
  uint32_t ncu;
};
hipError_t launch_write_private_headers(const WriteHeadersArgs& a, hipStream_t s);

// qfec_record_received / qfec_build_acks: QuicReceivedPacketManager and its
// EntropyTracker for a whole turn, behind the revive (rule as include/qfec.h).
// The state is the caller's: per connection a ring of `window` one-byte cells
// (kCellReceived | kCellEntropy | kCellRevived), the least packet awaited, the
// largest observed and the hash of everything below the least.
constexpr uint32_t kCellReceived = 1, kCellEntropy = 2, kCellRevived = 4;
constexpr uint32_t kRcvNotAccepted = 0, kRcvRange = 1, kRcvStale = 2, kRcvOverflow = 3,
                   kRcvDuplicate = 4, kRcvRecorded = 5;
constexpr uint32_t kRecordCounts = 12;  // the six classes, then [6] cells newly set, [7] revived
                                        // recorded, [8] revived not missing, [9] raises applied,
                                        // [10] raises that dropped a missing packet, [11] jumps
constexpr uint32_t kAckMinWindow = 64, kAckMaxWindow = 65536;
// Scratch of the record, a block of record_scratch_bytes(n_conns) in the revive
// calls' allocation: per connection the largest RECORDED packet number of the
// call, zeroed in front of the kernels.
struct RecordArgs {
  const unsigned long long* packet_number;  // nullable with n_packets == 0, as pkt_conn
  const uint32_t* pkt_conn;
  const uint8_t* hdr;      // nullable: all accepted
  const uint8_t* entropy;  // nullable: all 0
  uint64_t n_packets;      // < 2^32
  const uint8_t* status;   // the revive's outputs; nullable with n_groups == 0
  const uint8_t* revived_idx;
  const uint32_t* slot;  // nullable: group g has slot g
  const unsigned long long* slot_key;
  uint32_t n_groups;
  uint32_t n_slots;
  uint32_t key_shift;  // 1..63
  const uint32_t* raise_conn;  // nullable with n_raise == 0
  const unsigned long long* raise_least;
  const uint8_t* raise_hash;
  uint32_t n_raise;
  uint8_t* rcv_cells;
  unsigned long long* rcv_least;
  unsigned long long* rcv_largest;
  uint8_t* rcv_hash;
  uint32_t n_conns;  // may be 0: every connection is out of range
  uint32_t window;   // a power of two, kAckMinWindow .. kAckMaxWindow
  uint8_t* rcv_out;            // nullable with n_packets == 0
  unsigned long long* counts;  // nullable: kRecordCounts words
  unsigned long long* seen;    // scratch: n_conns
  uint32_t* err;
  uint32_t ncu;
};
inline uint64_t record_scratch_bytes(uint64_t n_conns) { return n_conns * 8; }
inline void record_scratch_layout(RecordArgs& a, void* block) {
  a.seen = static_cast<unsigned long long*>(block);
}
// Up to two memsets and five launches on s (classify, advance, set, revived,
// raises), ordered by the stream alone.  Not all of n_packets, n_groups and
// n_raise are 0.
hipError_t launch_record_received(const RecordArgs& a, hipStream_t s);

// Scratch of the build, a block of acks_scratch_bytes(n_acks): per ack the
// intervals it keeps and the revived packets at or below its largest.
struct AcksArgs {
  const uint32_t* ack_conn;
  uint32_t n_acks;  // > 0, and n_acks * max(max_ranges, max_revived) < 2^32
  const uint8_t* rcv_cells;
  const unsigned long long* rcv_least;
  const unsigned long long* rcv_largest;
  const uint8_t* rcv_hash;
  uint32_t n_conns;
  uint32_t window;
  uint32_t max_ranges;   // 1..255
  uint32_t max_revived;  // 0..255
  unsigned long long* largest_observed;
  uint8_t* entropy_hash;
  uint8_t* truncated;
  uint32_t* range_ptr;  // n_acks + 1
  unsigned long long* range_lo;
  unsigned long long* range_hi;
  uint32_t* rev_ptr;  // n_acks + 1
  unsigned long long* rev_pn;  // nullable with max_revived == 0
  uint32_t* n_rng;  // scratch: n_acks
  uint32_t* n_rev;  // scratch: n_acks (all the revived at or below the largest, not the kept)
  uint32_t* err;
  uint32_t ncu;
};
inline uint64_t acks_scratch_bytes(uint64_t n_acks) { return n_acks * 8; }
inline void acks_scratch_layout(AcksArgs& a, void* block) {
  a.n_rng = static_cast<uint32_t*>(block);
  a.n_rev = a.n_rng + a.n_acks;
}
// Three launches on s (count, scan, fill), ordered by the stream alone.
hipError_t launch_build_acks(const AcksArgs& a, hipStream_t s);

// The built acks as v<=31 ack frames (qfec_write_ack_frames): the build's
// outputs and the ring, read only.
constexpr uint32_t kAckWireCounts = 4;      // the acks per QFEC_ACKW_* status
constexpr uint32_t kAckWireMaxPrefix = 64;  // prefix_len: a packet header and private flags
struct AckWireArgs {
  const uint32_t* ack_conn;
  uint32_t n_acks;  // > 0
  const unsigned long long* largest_observed;
  const uint8_t* entropy_hash;
  const uint8_t* truncated;
  const uint32_t* range_ptr;  // n_acks + 1
  const unsigned long long* range_lo;
  const unsigned long long* range_hi;
  const uint32_t* rev_ptr;              // n_acks + 1
  const unsigned long long* rev_pn;     // nullable: no ack has a revived number
  const unsigned long long* ack_delay_us;  // nullable: all infinite
  const uint8_t* rcv_cells;             // nullable with n_conns == 0
  uint32_t n_conns;
  uint32_t window;
  uint8_t* out;
  const unsigned long long* out_off;
  const uint16_t* out_cap;
  uint32_t prefix_len;  // <= kAckWireMaxPrefix
  uint16_t* out_len;
  unsigned long long* wire_largest;
  uint8_t* wire_hash;
  uint8_t* ack_status;
  unsigned long long* counts;  // nullable: kAckWireCounts words
  uint32_t* err;
  uint32_t ncu;
};
// One memset (counts) and one launch on s.
hipError_t launch_write_ack_frames(const AckWireArgs& a, hipStream_t s);

// qfec_scan_frames: QuicFramer::ProcessFrameData over the turn's packets, behind
// the parse, and the STOP_WAITING state per connection (rule as include/qfec.h).
// Scratch, a block of frames_scratch_bytes(n_packets, n_conns): per packet the
// frames it lists and its last STOP_WAITING, per connection the largest packet
// number that holds a newer one and the earliest packet with that number.
constexpr uint32_t kFrmOk = 0, kFrmSkipped = 1, kFrmNoFrames = 2, kFrmIllegalType = 3,
                   kFrmStream = 4, kFrmAck = 5, kFrmRst = 6, kFrmClose = 7, kFrmGoaway = 8,
                   kFrmWindowUpdate = 9, kFrmBlocked = 10, kFrmStopWaiting = 11,
                   kFrmPathClose = 12, kFrmBadLeast = 13, kFrmTooMany = 14, kFrmPnLen = 15,
                   kFrmRange = 16;
constexpr uint32_t kFrameStream = 0x80, kFrameAck = 0x40, kFrameStopWaiting = 6;
constexpr uint32_t kFramesCounts = 13;  // (order as include/qfec.h)
struct FramesArgs {
  const uint8_t* bytes;
  const uint64_t* body_off;
  const uint16_t* body_len;
  const unsigned long long* packet_number;
  const uint32_t* pkt_conn;
  const uint8_t* pkt_pn_len;
  const uint8_t* hdr;   // nullable: all accepted data packets
  uint64_t n_packets;   // 0 < n_packets < 2^32, n_packets * max_frames < 2^32
  uint32_t revived_tail;  // the ack has its revived tail: quic_version <= 31
  uint32_t max_frames;    // 1..255
  uint8_t* frm_status;
  uint32_t* frm_ptr;  // n_packets + 1
  uint32_t* frm_pkt;  // the table: all nullable with frm_cap == 0
  uint8_t* frm_type;
  uint8_t* frm_flags;
  uint64_t* frm_off;
  uint16_t* frm_len;
  uint32_t* frm_id;
  unsigned long long* frm_val;
  uint32_t* frm_code;
  uint32_t frm_cap;
  unsigned long long* sw_seen;  // the state: nullable with n_conns == 0
  unsigned long long* sw_least;
  uint8_t* sw_hash;
  uint32_t* sw_conn;
  uint32_t n_conns;
  unsigned long long* counts;    // nullable: kFramesCounts words
  unsigned long long* top;       // scratch: n_conns, zeroed
  unsigned long long* pkt_least; // scratch: n_packets (written where a packet holds one)
  uint32_t* pick;                // scratch: n_conns, all ones
  uint32_t* n_frm;               // scratch: n_packets
  uint32_t* tile_off;            // scratch: the frames of every kReviveTile packets, then scanned
  uint8_t* pkt_hash;             // scratch: n_packets
  uint32_t* err;
  uint32_t ncu;
};
inline uint64_t frames_scratch_bytes(uint64_t n_packets, uint64_t n_conns) {
  return n_conns * 12 + n_packets * 13 + revive_tiles(n_packets) * 4 + 8;
}
inline void frames_scratch_layout(FramesArgs& a, void* block) {
  a.top = static_cast<unsigned long long*>(block);
  a.pkt_least = a.top + a.n_conns;
  a.pick = reinterpret_cast<uint32_t*>(a.pkt_least + a.n_packets);
  a.n_frm = a.pick + a.n_conns;
  a.tile_off = a.n_frm + a.n_packets;
  a.pkt_hash = reinterpret_cast<uint8_t*>(a.tile_off + revive_tiles(a.n_packets));
}
// Up to three memsets and four launches on s (count and maximum, scan, fill and
// pick, set), ordered by the stream alone.  n_packets > 0.
hipError_t launch_scan_frames(const FramesArgs& a, hipStream_t s);

// Small-batch service (round 4): one resident workgroup that takes mapped
// ragged batches from a ring in host-mapped memory instead of a kernel launch
// per batch (the launch is most of a small flush's connection-thread cost).
// The host writes a job, then publishes pub_end (the groups published so
// far); the worker processes every published group (one wave per group, the
// small-batch kernel's body), stores each job's token into its slot's flag
// and `consumed`, and exits after idle_ticks without work (alive = 0, then one
// more look at pub_end: the host, after publishing, relaunches it if it
// reads alive == 0 -- each side writes, fences, then reads the other's word).
// Round 5: the job's index tables are written INLINE (tab, at the t_*
// offsets, the direct path's Tab layout), so the worker copies the entry --
// header and tables -- into LDS in one PCIe round trip.  a's table pointers
// are not used by the worker.
constexpr uint32_t kSvcTab = 16384 - 256;  // inline table bytes (64 groups of up to 16 packets)
struct SvcJob {
  RaggedArgs a;       // bytes / parity / out: the mapped payload buffers
  uint64_t start;     // the job's first group in the global group sequence
  uint32_t seq;       // job number (ring index = seq % kSvcRing)
  uint32_t recover;
  uint32_t flag_slot; // index into the context's host-mapped flags
  uint32_t token;
  uint32_t tab_bytes; // table bytes in tab (<= kSvcTab)
  uint32_t t_off, t_len, t_ptr, t_poff, t_plen, t_miss, t_ooff;  // offsets into tab
  // Round 5: svc_head_hash of the entry's first min(entry size, kSvcHead)
  // bytes (this word excluded), stored by the host LAST; the leader reads
  // those bytes in every poll of the ring.  A job it finds whole there (hash,
  // seq and start agree) needs no second PCIe round trip for its entry when
  // it fits them; a larger job's header is then known from the poll, so its
  // size is too, and the rest of its tables is copied in one pass (the
  // followers copy it whole, announced with that size).  0 while the host
  // writes the entry.
  uint64_t head_sum;
  alignas(16) uint8_t tab[kSvcTab];
};
constexpr uint32_t kSvcHead = 1024;  // bytes of the entry read with every poll (64 x 16 B)
constexpr uint32_t kSvcHeadSumWord = (uint32_t)(offsetof(SvcJob, head_sum) / 8u);
static_assert(offsetof(SvcJob, head_sum) % 8u == 0u, "head_sum on a word");
static_assert(offsetof(SvcJob, tab) < kSvcHead, "the header fits the polled bytes");
// Order-free sum over the 8-byte words [0, nbytes / 8) of the entry but
// head_sum's own: each word mixed with its index (splitmix64 finalizer), so a
// torn read -- some 16-B pieces from before the host's writes -- does not sum
// to the stored value (host and device compute the same function).
__host__ __device__ inline uint64_t svc_head_word(uint64_t w, uint32_t i) {
  uint64_t z = w ^ (0x9E3779B97F4A7C15ull * (uint64_t)(i + 1u));
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
inline uint64_t svc_head_hash(const SvcJob& j, uint32_t nbytes) {
  const uint64_t* w = reinterpret_cast<const uint64_t*>(&j);
  uint64_t h = 0;
  for (uint32_t i = 0; i < nbytes / 8u; ++i)
    if (i != kSvcHeadSumWord) h += svc_head_word(w[i], i);
  return h | 1ull;  // never 0 (0 = no hash)
}
struct SvcShared {
  // the host's words (the worker reads them) on a cache line of their own:
  // the worker's per-turn stores below would otherwise take the line from
  // the host's cache before every publish
  alignas(64) uint64_t pub_end;  // host: groups published
  uint32_t alive;     // host: 1 when it launches a worker; worker: 1 when it starts,
                      // 0 on its way out
  uint32_t quit;      // host: exit now (context destroyed)
  uint32_t stamp_on;  // host (measurement hook): the worker records stamps[] for each job
  uint32_t hold;      // host (test hook qfec_debug_service_hold): followers wait at
                      // their start while it is 1 (a follower dispatched late)
  uint32_t rotate;    // host: a worker whose launch epoch is at most this leaves at
                      // its next look, published jobs or not -- its successor is
                      // already queued behind it (svc_submit's residency bound)
  uint32_t warm;      // host: bumped by qfec_service_warm on a running worker -- a
                      // batch is coming; the worker's idle time restarts from it
  // the worker's words, stored every turn
  alignas(64) uint64_t consumed;  // worker: groups finished (a new worker starts here)
  uint64_t jobs;      // worker: jobs finished (stats)
  uint32_t fault;     // worker: a published group lay in no ring entry; it left
                      // without finishing (no token for any job of that turn)
  // 100-MHz wall-clock stamps of the last job (qfec_debug_service_stamps):
  // [0] work seen, [1] entry in LDS, [2] wave 0's first group done, [3] every
  // group done, [4] outputs visible (fence), [5] the leader's count / token
  // stored; [6] the token stored (by the last workgroup of a split job), [7]
  // that workgroup (round 6, qfec_debug_service_trace)
  alignas(64) uint64_t stamps[8];
  // round 6: every workgroup's stamps of its share of the last job: [0] its
  // entry in LDS, [1] its groups done, [2] its outputs visible, [3] counted
  uint64_t wg_stamps[8][4];
};
constexpr uint32_t kSvcRing = 8;
// Round 5: the worker is kSvcWgs workgroups.  Workgroup 0 (the leader) polls
// the host's pub_end, walks the published jobs and runs the alive / exit
// protocol above, so only the leader's decisions reach the host.  A job of
// more groups than one workgroup has waves is split over every workgroup;
// each adds itself to its ring entry's done counter after making its outputs
// visible and the last one stores the token.  Smaller jobs are the leader's
// alone.
// Round 6: the leader ANNOUNCES each split job to the followers
// through SvcDev (job number and entry size, in order); a follower takes the
// announcements one by one from its own count `taken`, which outlives the
// launch, and reads no other ring entry.  A follower dispatched late (the CUs
// held by another kernel) therefore still does every split job's share, and
// a split job's entry, whose token waits for every follower, is never reused
// under it.  At most kSlots (3) jobs are outstanding, so kSvcRing
// announcement words never wrap onto one not yet taken.
constexpr uint32_t kSvcWgs = 8;
static_assert(sizeof(SvcShared::wg_stamps) / sizeof(SvcShared::wg_stamps[0]) == kSvcWgs,
              "one stamp row per service workgroup");
struct SvcDev {
  uint32_t exit;             // leader: this launch's epoch when it leaves (after its
                             // last announcement)
  uint32_t done[kSvcRing];   // workgroups finished per ring entry's split job (the
                             // last resets it before the token)
  uint64_t nsplit;           // leader: split jobs announced so far
  uint64_t split[kSvcRing];  // announcement i at i % kSvcRing: job << 32 | entry bytes / 16
  uint64_t taken[kSvcWgs];   // follower w: announcements taken (w = 0 unused)
};
// (the host zeroes SvcDev when it creates the service and when it abandons it)
hipError_t launch_ragged_service(SvcShared* sh, SvcDev* dv, const SvcJob* ring, uint32_t* flags,
                                 uint64_t idle_ticks, uint32_t epoch, hipStream_t s);

// Packet protection batch (qpp_kernels.hip): packet p's associated data (the
// packet header) is ad_len[p] bytes at bytes + ad_off[p], its input payload
// in_len[p] bytes at bytes + in_off[p], its output at out + out_off[p].
struct ProtectArgs {
  const uint8_t* bytes;
  const uint64_t* ad_off;
  const uint16_t* ad_len;
  const uint64_t* in_off;
  const uint16_t* in_len;
  uint8_t* out;
  const uint64_t* out_off;
  uint8_t* ok;  // decrypt: 1 = tag verified and payload written
  uint64_t n;
  // decrypt with QFEC_SCRATCH_OUTPUT: one pass, the output of a packet whose
  // tag fails holds its unverified plaintext (else untouched, two passes)
  uint32_t scratch_out = 0;
};

hipError_t launch_null_protect(const ProtectArgs& a, bool decrypt, hipStream_t s);

// ChaCha20-Poly1305 (QUIC: 12-byte tag, nonce = prefix || LE64(path<<56|pn)).
// Packet p is protected with key key_idx[p] (keys: 32 B each, prefixes: 4 B
// each), packet number packet_number[p], path id path_id[p] (nullptr: 0).
struct AeadArgs {
  ProtectArgs io;
  const uint8_t* keys;
  const uint8_t* prefixes;
  const uint32_t* key_idx;
  const uint64_t* packet_number;
  const uint8_t* path_id;
};

hipError_t launch_chacha20poly1305(const AeadArgs& a, bool decrypt, hipStream_t s);
// AES-128-GCM (QUIC: 12-byte tag; keys are 16 B each).
hipError_t launch_aes128gcm(const AeadArgs& a, bool decrypt, hipStream_t s);

// Packet-entropy bookkeeping (qent_kernels.hip); layout as include/qfec.h.
struct EntropyScanArgs {
  const uint8_t* entropy;
  const uint64_t* conn_ptr;  // n_conns + 1
  const uint8_t* cum_base;   // nullable: 0
  uint64_t n_conns;
  uint8_t* cum;
};

struct EntropyValidateArgs {
  const uint8_t* cum;
  const uint64_t* conn_ptr;
  const uint64_t* first_pn;
  const uint8_t* cum_base;  // nullable: 0
  uint64_t n_conns;
  const uint32_t* ack_conn;
  const uint64_t* largest_observed;
  const uint8_t* claimed;
  const uint32_t* range_ptr;  // n_acks + 1
  const uint64_t* range_lo;
  const uint64_t* range_hi;
  uint64_t n_acks;
  uint8_t* ok;
};

// total_bytes = conn_ptr[n_conns] - conn_ptr[0] (host-known: picks lanes per
// connection), or 0 when unknown.
hipError_t launch_entropy_scan(const EntropyScanArgs& a, hipStream_t s, uint64_t total_bytes);
hipError_t launch_entropy_validate(const EntropyValidateArgs& a, hipStream_t s);

// nontemporal: nt loads and stores (the streaming default; see qfec.h QFEC_CACHED)
hipError_t launch_fixed(const FixedArgs& a, bool nontemporal, hipStream_t s);
// small_groups: the batch's groups carry few bytes each (round 6's band
// table: below kRaggedSmallGroupBytes on average): two groups per wave
// (ragged_multi_kernel) instead of the block kernel.
hipError_t launch_ragged(const RaggedArgs& a, bool recover, hipStream_t s, bool small_groups = false);
// average payload bytes per group below which a large ragged batch runs two
// groups per wave (launch_ragged small_groups; tools/tune/tune_rblock.hip
// mode 2, profiles/round6/ragged_band_r6h.txt)
constexpr uint64_t kRaggedSmallGroupBytes = 4096;
// Small batches whose payloads are read over PCIe (mapped host memory): one
// wave per group, all of a group's loads in flight at once.
hipError_t launch_ragged_latency(const RaggedArgs& a, bool recover, hipStream_t s);
hipError_t launch_stream_probe(const uint8_t* src, uint64_t n, uint8_t* dst, bool copy,
                               hipStream_t s);
hipError_t launch_xor_into(const uint8_t* in, uint64_t n, uint8_t* out, hipStream_t s);
hipError_t launch_synth_fixed(uint8_t* rows, uint32_t k, uint32_t L, uint64_t row_stride,
                              uint64_t group_stride, uint64_t g0, uint64_t n, uint64_t seed,
                              hipStream_t s);
hipError_t launch_synth_ragged(uint8_t* bytes, const uint64_t* pkt_off, const uint16_t* pkt_len,
                               const uint32_t* grp_ptr, uint64_t g0, uint64_t n, uint64_t seed,
                               hipStream_t s);

}  // namespace qfec
