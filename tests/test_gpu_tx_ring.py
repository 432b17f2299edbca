"""GPU: a transmit ring filled on the device (ns_csum_tx_ring, the transmit
mirror of ns_csum_rx_ring).  The expected arena is computed
frame by frame with the oracle (tests/txcases.py: packets.verify_frame as the
gate, both fields zeroed, packets.fill as the writer) and compared with the
device's: status, both sums and EVERY byte of the arena — the random preamble
before ring_off, the slot padding and the trailing bytes included.  Both
fields of every frame hold random bytes before the call (a reused ring)."""
import struct

import numpy as np
import pytest

import txcases as T
from pktgen import ethernet, frag_packet, random_packet, short_message, valid_packet

pytestmark = pytest.mark.gpu


def _run(engine, arena, lens, ring, calls=1):
    """The arena, status and sums after `calls` ns_csum_tx_ring calls."""
    import torch

    dev = torch.device("cuda", 0)
    a = torch.from_numpy(arena).to(dev)
    ln = torch.from_numpy(lens.view(np.int32)).to(dev)
    for _ in range(calls):
        status, sums = engine.tx_ring(a, ring, ln)
    torch.cuda.synchronize()
    n = ring["n"]
    return a.cpu().numpy(), status[:n].cpu().numpy(), sums[:2 * n].cpu().numpy().view(np.uint16)


def _check(engine, frames, stride, frame_at=0, link_hdr=0, ring_off=0, lens=None, seed=0, flags=0):
    arena, ln = T.build_ring(frames, stride, frame_at, link_hdr, ring_off, seed, lens)
    ring = dict(ring_off=ring_off, stride=stride, n=len(frames), frame_at=frame_at, link_hdr=link_hdr, flags=flags)
    got, status, sums = _run(engine, arena, ln, ring)
    return T.assert_ring(got, status, sums, arena, ln, ring).tolist()


@pytest.fixture(scope="module")
def mixed():
    """The mixed rings and their expected results, computed once."""
    out = {}
    for (link_hdr, frame_at), seed in zip(T.MIXED, T.MIXED_SEEDS):
        arena, lens, ring = T.mixed_ring(seed, link_hdr, frame_at)
        out[(link_hdr, frame_at)] = (arena, lens, ring, T.expected_ring(arena, lens, ring))
    return out


@pytest.mark.parametrize("link_hdr,frame_at", T.MIXED)
def test_mixed_ring_matches_oracle(engine, mixed, link_hdr, frame_at):
    arena, lens, ring, (want, wst, wsums) = mixed[(link_hdr, frame_at)]
    got, status, sums = _run(engine, arena, lens, ring)
    assert status.tolist() == wst.tolist()
    assert sums.tolist() == wsums.tolist()
    assert np.array_equal(got, want), np.nonzero(got != want)[0][:8]
    if link_hdr:
        assert status[5] == T.NONE  # EtherType 0x0806
        assert set(status.tolist()) == {T.NONE, T.L4, T.L3, T.MALFORMED}
    else:
        assert {T.L4, T.L3, T.MALFORMED} <= set(status.tolist())
    assert not np.array_equal(got, arena)  # the scrambled fields were rewritten


def test_second_call_changes_nothing(engine, mixed):
    arena, lens, ring, (want, wst, wsums) = mixed[(14, 10)]
    got, status, sums = _run(engine, arena, lens, ring, calls=2)
    assert np.array_equal(got, want) and status.tolist() == wst.tolist() and sums.tolist() == wsums.tolist()


def test_l4_only_leaves_the_ipv4_field(engine, mixed):
    for key in ((0, 0), (14, 0)):
        arena, lens, ring, _ = mixed[key]
        ring = dict(ring, flags=T.L4_ONLY)
        got, status, sums = _run(engine, arena, lens, ring)
        T.assert_ring(got, status, sums, arena, lens, ring)
        assert T.L3 not in set(status.tolist()) and T.L4 in set(status.tolist())
        assert not sums[0::2].any()
        off, stride, at = ring["ring_off"], ring["stride"], ring["frame_at"] + ring["link_hdr"] + 10
        for k in range(ring["n"]):  # the bytes where an IPv4 field would be, untouched in every slot
            lo = off + k * stride + at
            assert bytes(got[lo:lo + 2]) == bytes(arena[lo:lo + 2]), k


def test_round_trip_through_rx_ring(engine, mixed):
    """rx_ring over the filled ring: VALID for every TCP, ICMPv4-echo and
    ICMPv6 slot the fill wrote, INVALID nowhere."""
    import torch

    import packets as P

    for key in ((0, 4), (14, 0)):
        arena, lens, ring, (want, wst, _) = mixed[key]
        a = torch.from_numpy(want).cuda()
        ln = torch.from_numpy(lens.view(np.int32)).cuda()
        rr = dict(ring_off=ring["ring_off"], stride=ring["stride"], n=ring["n"], frame_at=ring["frame_at"],
                  link_hdr=ring["link_hdr"])
        verdict, _ = engine.rx_ring(a, rr, ln)
        torch.cuda.synchronize()
        verdict = verdict[:ring["n"]].cpu().numpy()
        assert P.INVALID not in set(verdict.tolist())
        checked = 0
        for k in range(ring["n"]):
            lo = ring["ring_off"] + k * ring["stride"]
            slot = bytes(want[lo:lo + ring["stride"]])
            _, ft, kind = T.fields(slot, int(lens[k]), ring["frame_at"], ring["link_hdr"])
            ip = slot[ring["frame_at"] + ring["link_hdr"]:]
            echo = kind == "icmp4" and ip[(ip[0] & 15) * 4] == 8
            if kind in ("tcp", "icmp6") or echo:
                assert verdict[k] == P.VALID and wst[k] == T.L4, (k, kind)
                checked += 1
            assert (verdict[k] == P.MALFORMED) == (wst[k] == T.MALFORMED), k
        assert checked > 100


def _short_frames(rng, n, limit):
    """Frames of at most `limit` bytes of every kind that fits."""
    out = []
    while len(out) < n:
        r = int(rng.integers(0, 10))
        if r < 6:
            p = valid_packet(rng, ("tcp4", "udp4", "icmp4", "icmp6", "udp6", "tcp6")[r], int(rng.integers(0, 25)))
        elif r == 6:
            p = frag_packet(rng, int(rng.integers(0, 6)), int(rng.integers(0, 20)))
        elif r == 7:
            k = ("tcp", "udp", "icmp4", "icmp6")[int(rng.integers(0, 4))]
            p = short_message(rng, k, int(rng.integers(0, 11)), None if k.startswith("icmp") else bool(rng.integers(0, 2)))
        elif r == 8:
            p = valid_packet(rng, "udp4", int(rng.integers(0, 20)))
            p[9] = 47  # another protocol: the IPv4 header only
        else:
            p = valid_packet(rng, "tcp4", int(rng.integers(0, 8)))
            p += bytes(rng.integers(0, 256, int(rng.integers(1, 12)), dtype=np.uint8))  # trailing padding
        if len(p) <= limit:
            out.append(bytes(p))
    return out


@pytest.mark.parametrize("stride,link_hdr,frame_at", [(80, 0, 0), (80, 14, 0), (96, 0, 16), (96, 14, 10), (80, 0, 6)])
def test_short_slots_share_lines(engine, stride, link_hdr, frame_at):
    """Frames of at most 64 B in 80- and 96-B slots: one 128-B line holds
    parts of up to three frames, so neighbouring groups store into lines this
    group reads.  The ring starts 16 B (not a line) into the arena."""
    rng = np.random.default_rng(7200 + stride + link_hdr + frame_at)
    pk = _short_frames(rng, 333, 64 - link_hdr)
    frames = [ethernet(p) for p in pk] if link_hdr else pk
    assert max(len(f) for f in frames) <= 64
    st = _check(engine, frames, stride, frame_at, link_hdr, ring_off=16, seed=stride)
    assert {T.L4, T.L3, T.MALFORMED} <= set(st)


@pytest.mark.parametrize("stride,link_hdr", [(1504, 0), (2048, 14), (2048, 0)])
def test_mtu_slots(engine, stride, link_hdr):
    rng = np.random.default_rng(7300 + stride + link_hdr)
    pk = [random_packet(rng, 1400) for _ in range(150)]
    pk += [valid_packet(rng, k, 1500 - h) for k, h in (("tcp4", 40), ("udp4", 28), ("udp6", 48), ("icmp6", 48))]
    pk = [p for p in pk if len(p) + link_hdr <= stride]
    frames = [ethernet(bytes(p)) for p in pk] if link_hdr else [bytes(p) for p in pk]
    _check(engine, frames, stride, 0, link_hdr, seed=stride)


@pytest.mark.parametrize("n", [1, 7, 9])
def test_slot_counts_around_a_wave(engine, n):
    rng = np.random.default_rng(7400 + n)
    frames = [bytes(valid_packet(rng, ("tcp4", "udp6", "icmp4")[k % 3], int(rng.integers(0, 1400)))) for k in range(n)]
    assert _check(engine, frames, 1504, seed=n) == [T.L4] * n


def test_jumbo_frames(engine):
    rng = np.random.default_rng(7500)
    pk = [valid_packet(rng, k, 9000 - h) for k, h in (("udp4", 28), ("udp6", 48), ("icmp4", 28), ("icmp6", 48))]
    pk += [valid_packet(rng, "tcp4", 8900), valid_packet(rng, "tcp6", 8901), frag_packet(rng, 0, 8000)]
    pk += [valid_packet(rng, "udp4", 8972) + bytes(rng.integers(0, 256, 200, dtype=np.uint8)), valid_packet(rng, "tcp4", 1)]
    assert max(len(p) for p in pk) <= 9216 - 14
    st = _check(engine, [ethernet(bytes(p)) for p in pk], 9216, 0, 14, seed=75)
    assert st == [T.L4] * 6 + [T.L3] + [T.L4] * 2


@pytest.mark.parametrize("kind,plen,stride", [("udp4", 65507, 65536), ("udp6", 65527, 65584), ("icmp4", 65505, 65536)])
def test_longest_packets(engine, kind, plen, stride):
    """One 65,535-B IPv4 packet (TotalLength 0xffff), an odd-length one, and
    the longest IPv6 packet a header can describe (PayloadLength 0xffff)."""
    rng = np.random.default_rng(7600)
    p = bytes(valid_packet(rng, kind, plen))
    assert len(p) == {"udp4": 65535, "udp6": 65575, "icmp4": 65533}[kind]
    assert _check(engine, [p], stride, seed=76) == [T.L4]


def test_length_over_the_stride_is_malformed_counted_and_untouched(engine):
    rng = np.random.default_rng(7700)
    frames = [bytes(valid_packet(rng, "tcp4", 100)) for _ in range(5)]
    arena, ln = T.build_ring(frames, 160, seed=77)
    ln[3] = 161
    ring = dict(stride=160, n=5)
    engine.sync()
    got, status, sums = _run(engine, arena, ln, ring)
    assert engine.sync() == 1
    T.assert_ring(got, status, sums, arena, ln, ring)
    assert status.tolist() == [T.L4, T.L4, T.L4, T.MALFORMED, T.L4]
    assert bytes(got[3 * 160:4 * 160]) == bytes(arena[3 * 160:4 * 160])


def _deep_headers(rng, plen):
    """IPv4 with IHL 15 and TCP with DataOffset 15: the deepest fields."""
    ip = bytearray(rng.integers(0, 256, 60, dtype=np.uint8))
    ip[0] = 0x4F
    struct.pack_into(">H", ip, 2, 120 + plen)
    ip[6] = ip[7] = 0
    ip[9] = 6
    tcp = bytearray(rng.integers(0, 256, 60, dtype=np.uint8))
    tcp[12] = 0xF0
    return bytes(ip + tcp + bytes(rng.integers(0, 256, plen, dtype=np.uint8)))


@pytest.mark.parametrize("link_hdr,frame_at", [(0, 0), (14, 0), (0, 14), (14, 10)])
def test_deepest_fields_and_payload_edges(engine, link_hdr, frame_at):
    """IHL 15 + DataOffset 15 (the TCP field 76 B into the packet, the packet
    up to 14 B into its 16-B chunk), zero-length and odd-length payloads, and
    Ethernet padding past TotalLength."""
    rng = np.random.default_rng(7800 + link_hdr + frame_at)
    pk = [_deep_headers(rng, plen) for plen in (0, 1, 2, 15, 16, 17, 333)]
    for kind in ("tcp4", "tcp6", "udp4", "udp6", "icmp4", "icmp6"):
        pk += [bytes(valid_packet(rng, kind, plen)) for plen in (0, 1, 2, 3, 31, 32, 33, 127, 255)]
    pad = [p + bytes(rng.integers(0, 256, max(46 - len(p), 3), dtype=np.uint8)) for p in pk[7::5]]
    pk += pad + [p + bytes(rng.integers(0, 256, 300, dtype=np.uint8)) for p in pk[:7]]
    frames = [ethernet(p) for p in pk] if link_hdr else pk
    st = _check(engine, frames, 800, frame_at, link_hdr, seed=78)
    assert st == [T.L4] * len(frames)


@pytest.mark.parametrize("kind", ["udp4", "udp6", "tcp4", "tcp6"])
def test_a_sum_of_ffff_writes_zero(engine, kind):
    """The reference writes ^0xffff = 0x0000 (for UDP too: it does not write
    RFC 768's 0xffff)."""
    rng = np.random.default_rng(7900)
    p = bytes(T.sum_to_ffff(valid_packet(rng, kind, 64)))
    arena, ln = T.build_ring([p, p], 192, seed=79)
    ring = dict(stride=192, n=2)
    got, status, sums = _run(engine, arena, ln, ring)
    T.assert_ring(got, status, sums, arena, ln, ring)
    _, ft, _ = T.fields(bytes(arena[:192]), int(ln[0]), 0, 0)
    assert sums[1] == 0xFFFF and bytes(got[ft:ft + 2]) == b"\0\0" and status[0] == T.L4


def test_an_all_zero_icmp_message_gets_ffff(engine):
    """An ICMPv4 message of zeros sums to 0: the field becomes 0xffff and the
    slot still reports NS_TXR_L4 with a transport sum of 0."""
    rng = np.random.default_rng(7950)
    p = valid_packet(rng, "icmp4", 0)
    p[20:28] = bytes(8)  # an echo reply, identifier and sequence 0
    arena, ln = T.build_ring([bytes(p)], 48, seed=7)
    got, status, sums = _run(engine, arena, ln, dict(stride=48, n=1))
    T.assert_ring(got, status, sums, arena, ln, dict(stride=48, n=1))
    assert status[0] == T.L4 and sums[1] == 0 and bytes(got[22:24]) == b"\xff\xff"


def test_agrees_with_fill_packet_buffers(engine):
    """The well-formed frames through ns_csum_packet_buffers(NS_PKB_FILL),
    Header = the IP and transport headers, Data = the payload: the same
    bytes and the same sums."""
    from netstack_amd.buffer import NewPrependableFromView, NewVectorisedView, View
    from netstack_amd.packet import PacketBuffer, fill_packet_buffers

    rng = np.random.default_rng(8000)
    kinds = ("tcp4", "tcp6", "udp4", "udp6", "icmp4", "icmp6")
    pk = [bytearray(valid_packet(rng, kinds[k % 6], int(rng.integers(0, 1400)))) for k in range(120)]
    arena, ln = T.build_ring([bytes(p) for p in pk], 1504, seed=80)
    ring = dict(stride=1504, n=len(pk))
    got, status, sums = _run(engine, arena, ln, ring)
    assert status.tolist() == [T.L4] * len(pk)
    pkts = []
    for k, p in enumerate(pk):
        z = bytearray(p)
        f4, ft, kind = T.fields(bytes(p), len(p), 0, 0)
        z[ft:ft + 2] = b"\0\0"
        if f4 is not None:
            z[f4:f4 + 2] = b"\0\0"
        hlen = (z[0] & 15) * 4 if z[0] >> 4 == 4 else 40
        hl = hlen + ((z[hlen + 12] >> 4) * 4 if kind == "tcp" else 8)
        pkts.append(PacketBuffer(Data=NewVectorisedView(len(z) - hl, [View(bytearray(z[hl:]))]),
                                 Header=NewPrependableFromView(View(bytearray(z[:hl])))))
    s2 = fill_packet_buffers(pkts, engine)
    assert sums.tolist() == np.asarray(s2, dtype=np.uint16).tolist()
    for k, pkb in enumerate(pkts):
        h = bytes(pkb.Header.View())
        assert bytes(got[k * 1504:k * 1504 + len(h)]) == h, k


def test_error_codes(engine):
    import torch

    from netstack_amd._lib import ChecksumError, NS_ERANGE

    a = torch.zeros(16 + 4 * 1504, dtype=torch.uint8, device="cuda")
    ln = torch.zeros(8, dtype=torch.int32, device="cuda")
    ok = dict(ring_off=16, stride=1504, n=4)
    engine.tx_ring(a, ok, ln)
    for bad in (dict(stride=0), dict(stride=1 << 24), dict(stride=1500), dict(ring_off=8), dict(frame_at=1),
                dict(frame_at=1504), dict(link_hdr=12), dict(link_hdr=14, frame_at=3), dict(flags=2),
                dict(flags=0x80000001), dict(pad=1)):
        with pytest.raises(ValueError):
            engine.tx_ring(a, dict(ok, **bad), ln)
    for bad in (dict(n=5), dict(ring_off=32), dict(ring_off=1 << 40)):
        with pytest.raises(ChecksumError) as e:
            engine.tx_ring(a, dict(ok, **bad), ln)
        assert e.value.status == NS_ERANGE
    # both outputs may be NULL (the stores are the result); NULL lengths may not
    import ctypes

    from netstack_amd import _lib

    r = _lib.NsTxRing(16, 1504, 4, 0, 0, 0, 0)
    L = _lib.lib()
    assert L.ns_csum_tx_ring(engine._h, a.data_ptr(), a.numel(), ctypes.byref(r), ln.data_ptr(), None, None, None) == 0
    assert L.ns_csum_tx_ring(engine._h, a.data_ptr(), a.numel(), ctypes.byref(r), None, None, None, None) == _lib.NS_EINVAL
    torch.cuda.synchronize()
    assert engine.sync() == 0


def test_mid_size_ring_fields_scrambled_on_the_device(engine):
    """65,536 MTU frames (workloads.rx_ring_batch_sized), both fields
    scrambled on the device: after the call rx_ring says VALID for all, and
    the arena differs from the original only at the field offsets."""
    import torch

    from netstack_amd import workloads as W
    from netstack_amd._lib import NS_PKB_VALID

    n = 65536
    for eth, v6 in ((False, False), (True, True)):
        arena, lens, _, stride = W.rx_ring_batch_sized(n, 1500, 81, "cuda:0", v6=v6, eth=eth, stride=1504 + (16 if eth else 0))
        lh, ipl = (14 if eth else 0), (40 if v6 else 20)
        orig = arena.clone()
        slots = arena.view(n, stride)
        cols = [lh + ipl + 16, lh + ipl + 17] + ([] if v6 else [lh + 10, lh + 11])
        g = torch.Generator(device="cuda").manual_seed(82)
        for c in cols:
            slots[:, c] = torch.randint(0, 256, (n,), dtype=torch.uint8, device="cuda", generator=g)
        ring = dict(stride=stride, n=n, link_hdr=lh)
        status, sums = engine.tx_ring(arena, ring, lens)
        verdict, _ = engine.rx_ring(arena, ring, lens)
        torch.cuda.synchronize()
        assert bool((status[:n] == T.L4).all())
        assert bool((verdict[:n] == NS_PKB_VALID).all())
        diff = (arena != orig).view(n, stride)
        keep = torch.ones(stride, dtype=torch.bool, device="cuda")
        keep[cols] = False
        assert not bool(diff[:, keep].any())
        # the batch's own fields were valid: the fill restores them exactly
        assert torch.equal(arena, orig)
