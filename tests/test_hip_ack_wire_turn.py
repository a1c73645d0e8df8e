"""The receiver's turn closed on the device: test_hip_ack_turn's turn (sealed
packets -> ... -> qfec_record_received -> qfec_build_acks) goes on with
qfec_write_ack_frames -> qfec_write_private_headers (the ack packets' private
byte) -> seal -> open (the peer), all queued on one stream with ONE qfec_sync.

Checked: the peer, which sees nothing but the opened bytes, parses every frame
on the host (qfec_wire_parse_ack_frame) and the parsed acks validate against
the sender's own entropy bookkeeping (qfec_entropy_validate_batch) -- the acks
the writer cut for want of room included, whose hash the writer recomputed from
the ring; and the parsed content is the built ack's, below the largest written."""
import numpy as np
import pytest
import torch

import ack_device as D
import ack_rule as A
import ackwire_rule as R
import assign_turns as T
from libquic_amd import qfec
from test_hip_accumulate_ragged import dview
from test_hip_ack_turn import ACK_CONNS, WINDOW, Unsynced, sender_entropy, turn  # noqa: F401
from test_hip_parse_turn import AD, KLEN, N_SLOTS, TAG, VERSION, device_turn
from test_hip_retire_turn import N_CONNS, P64, SHIFT, Device

gpu = pytest.mark.gpu
U64 = np.uint64
SLOT, GUARD = 1024, 0x5C  # an ack packet's place in the arena and on the wire


@gpu
@pytest.mark.parametrize("cipher,max_ranges,out_cap", [("chacha20poly1305", 255, 900),
                                                       ("aes128gcm", 255, 900),
                                                       ("aes128gcm", 255, 14),
                                                       ("chacha20poly1305", 4, 13)])
def test_turn_to_sealed_acks(ctx, turn, cipher, max_ranges, out_cap):  # noqa: F811
    t, m, n = turn, turn.m, ACK_CONNS
    first, ptr, ent = sender_entropy(t)
    state = A.new_state(ACK_CONNS, WINDOW)
    state["least"][:] = first
    ack = D.DevState(state)
    everyone = np.arange(n, dtype=np.uint32)
    conn = dview(everyone)
    dev = Device(ctx, T.KeyState(9301, N_SLOTS), np.append(np.zeros(N_CONNS, U64), P64))
    d = device_turn(Unsynced(ctx), cipher, t, dev)
    ctx.record_received(*ack.args(), packet_number=d["a_pn"], pkt_conn=d["a_conn"], n_packets=m,
                        rcv_out=dview(np.zeros(m, np.uint8)), hdr=d["hdr"], entropy=d["entropy"],
                        status=d["st"], revived_idx=d["ridx"], slot_key=dev.key, n_groups=N_SLOTS,
                        n_slots=N_SLOTS, key_shift=SHIFT)
    o = dict(largest=dview(np.zeros(n, U64)), hash=dview(np.zeros(n, np.uint8)),
             truncated=dview(np.zeros(n, np.uint8)), range_ptr=dview(np.zeros(n + 1, np.uint32)),
             range_lo=dview(np.zeros(n * max_ranges, U64)),
             range_hi=dview(np.zeros(n * max_ranges, U64)),
             rev_ptr=dview(np.zeros(n + 1, np.uint32)), rev_pn=dview(np.zeros(n * 255, U64)))
    ctx.build_acks(conn, n, *ack.args(), max_ranges, 255, o["largest"], o["hash"], o["truncated"],
                   o["range_ptr"], o["range_lo"], o["range_hi"], o["rev_ptr"], o["rev_pn"])
    # ---- the ack packets: [associated data][private flags][the frame], one to a slot
    rng = np.random.default_rng(77)
    arena = np.full(n * SLOT, GUARD, np.uint8)
    ads = rng.integers(0, 256, (n, AD), dtype=np.uint8)
    ad_off = np.arange(n, dtype=U64) * U64(SLOT) + U64(7)
    for a in range(n):
        arena[int(ad_off[a]):int(ad_off[a]) + AD] = ads[a]
    wire_h = arena.copy()  # (the associated data travels in the clear)
    d_arena, wire = dview(arena), dview(wire_h)
    opened = dview(np.full(n * SLOT, GUARD, np.uint8))
    priv_off, frame_off = dview(ad_off + U64(AD)), dview(ad_off + U64(AD + 1))
    w = dict(out_len=dview(np.zeros(n, np.uint16)), largest=dview(np.zeros(n, U64)),
             hash=dview(np.zeros(n, np.uint8)), status=dview(np.full(n, 0xA5, np.uint8)),
             counts=dview(np.zeros(4, U64)))
    delay = np.array([0, 5000, R.INFINITE, 1 << 22, 4096, 77, 1, 2], U64)
    ctx.write_ack_frames(conn, n, o["largest"], o["hash"], o["truncated"], o["range_ptr"],
                         o["range_lo"], o["range_hi"], o["rev_ptr"], o["rev_pn"], ack.cells,
                         ACK_CONNS, WINDOW, d_arena, frame_off, dview(np.full(n, out_cap, np.uint16)),
                         w["out_len"], w["largest"], w["hash"], w["status"],
                         ack_delay_us=dview(delay), prefix_len=1, counts=w["counts"])
    flags = (everyone & 1).astype(np.uint8)  # the ack packets' own entropy flags
    ctx.write_private_headers(d_arena, priv_off, dview(flags), dview(np.zeros(n, np.uint8)), n,
                              VERSION)
    keys = dview(np.ascontiguousarray(t.table[:, :KLEN[cipher]]).ravel())
    prefixes = dview(np.ascontiguousarray(t.table[:, 32:]).ravel())
    key_idx, pn = dview(everyone % 6), dview(np.arange(9000, 9000 + n, dtype=U64))
    path, ad_len = dview(np.zeros(n, np.uint8)), dview(np.full(n, AD, np.uint16))
    d_ad = dview(ad_off)
    # out_len is the seal's in_len as it lies, in_off = out_off - prefix_len
    getattr(ctx, cipher + "_seal")(keys, prefixes, key_idx, pn, path, d_arena, d_ad, ad_len,
                                   priv_off, w["out_len"], n, wire, priv_off)
    ct_len = (w["out_len"].to(torch.int32) + TAG).to(torch.int16)  # (the peer reads it off the datagram)
    ok = dview(np.full(n, 0xA5, np.uint8))
    getattr(ctx, cipher + "_open")(keys, prefixes, key_idx, pn, path, wire, d_ad, ad_len, priv_off,
                                   ct_len, n, opened, priv_off, ok)
    assert ctx.sync() == qfec.QFEC_OK  # the turn's only one
    # ---- the peer: nothing but the opened bytes
    assert D.host(ok, np.uint8).tolist() == [1] * n
    plain, out_len = D.host(opened, np.uint8), D.host(w["out_len"], np.uint16)
    status = D.host(w["status"], np.uint8)
    got = {k: D.host(v, dt) for (k, v), dt in zip(o.items(), (
        U64, np.uint8, np.uint8, np.uint32, U64, U64, np.uint32, U64))}
    p_big, p_hash, p_ptr, p_lo, p_hi = [], [], [0], [], []
    for a in range(n):
        at = int(ad_off[a]) + AD
        assert plain[at] == flags[a] and out_len[a] > 1
        used, p = qfec.wire_parse_ack_frame(bytes(plain[at + 1:at + out_len[a]]))
        assert used == out_len[a] - 1 and (plain[at + out_len[a]:at + out_len[a] + 40] == GUARD).all()
        # the built ack's content, below the largest the frame carries
        r0, r1 = got["range_ptr"][a], got["range_ptr"][a + 1]
        v0, v1 = got["rev_ptr"][a], got["rev_ptr"][a + 1]
        top = p["largest"]
        assert p["largest"] == D.host(w["largest"], U64)[a] and p["hash"] == D.host(w["hash"], np.uint8)[a]
        assert p["ranges"] == [(int(x), min(int(y), top + 1)) for x, y in
                               zip(got["range_lo"][r0:r1], got["range_hi"][r0:r1]) if x <= top]
        listed = [int(x) for x in got["rev_pn"][v0:v1] if x <= top]
        assert p["revived"] == listed[len(listed) - len(p["revived"]):]
        assert p["truncated"] == bool(got["truncated"][a] or status[a] == qfec.QFEC_ACKW_CUT)
        assert p["delay"] == R.ufloat16(int(delay[a]))
        assert top == got["largest"][a] or status[a] == qfec.QFEC_ACKW_CUT
        p_big.append(top), p_hash.append(p["hash"])
        p_lo += [x for x, _ in p["ranges"]]
        p_hi += [y for _, y in p["ranges"]]
        p_ptr.append(len(p_lo))
    cnt = D.host(w["counts"], U64).tolist()
    assert cnt[2:] == [0, 0] and cnt[0] + cnt[1] == n
    if out_cap < 100:  # connections 0..5 have more missing ranges than fit
        assert (status[:6] == qfec.QFEC_ACKW_CUT).all() and cnt[1] >= 6
        assert got["truncated"][:6].all() == (max_ranges == 4)
    else:
        assert cnt == [n, 0, 0, 0] and len(p_lo) > 12
    # the sender validates what it parsed (device tables throughout)
    cum, valid = dview(np.zeros(ent.size, np.uint8)), dview(np.full(n, 0xA5, np.uint8))
    d_ptr, d_first = dview(ptr), dview(first)
    ctx.entropy_cumulative(dview(ent), d_ptr, None, ACK_CONNS, cum, n_packets=ent.size)
    ctx.entropy_validate(cum, d_ptr, d_first, None, ACK_CONNS, conn, dview(np.array(p_big, U64)),
                         dview(np.array(p_hash, np.uint8)), dview(np.array(p_ptr, np.uint32)),
                         dview(np.array(p_lo + [0], U64)), dview(np.array(p_hi + [0], U64)), n, valid)
    assert ctx.sync() == qfec.QFEC_OK
    assert D.host(valid, np.uint8)[:6].tolist() == [1] * 6  # (6 and 7 never heard anything)
