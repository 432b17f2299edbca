"""Shared helpers of the transmit-ring tests (ns_csum_tx_ring, _tx_ring_host,
netstack_amd.tx): the expected ring computed frame by frame with the oracle
(oracle/packets.py verify_frame as the gate, fill as the writer), and the
rings the tests run.  Nothing here touches the engine."""
import struct

import numpy as np

NONE, L4, L3, MALFORMED = 0, 1, 2, 3
L4_ONLY = 1


def fields(slot: bytes, rlen: int, frame_at: int, link_hdr: int):
    """(IPv4 field offset or None, transport field offset or None, kind) of a
    slot's frame, offsets from the slot's first byte; (None, None, None) for a
    frame the gate refuses or that is not IP.  kind: 'tcp', 'udp', 'icmp4',
    'icmp6', 'l3' (an IPv4 fragment or another protocol) or 'none'."""
    import packets as P

    if P.verify_frame(slot, rlen, frame_at, link_hdr, 0)[0] == P.MALFORMED:
        return None, None, None
    frame = slot[frame_at:rlen]
    if link_hdr and ((frame[12] << 8) | frame[13]) not in (0x0800, 0x86DD):
        return None, None, "none"
    at = frame_at + link_hdr
    ip = frame[link_hdr:]
    if ip[0] >> 4 == 4:
        hlen, proto = (ip[0] & 15) * 4, ip[9]
        frag = (ip[6] & 0x20) or (((ip[6] & 0x1F) << 8) | ip[7])
        if not frag and proto in (6, 17, 1):
            return at + 10, at + hlen + {6: 16, 17: 6, 1: 2}[proto], {6: "tcp", 17: "udp", 1: "icmp4"}[proto]
        return at + 10, None, "l3"
    proto = ip[6]
    if proto in (6, 17, 58):
        return None, at + 40 + {6: 16, 17: 6, 58: 2}[proto], {6: "tcp", 17: "udp", 58: "icmp6"}[proto]
    return None, None, "none"


def expected_slot(slot: bytes, rlen: int, frame_at: int, link_hdr: int, flags: int = 0):
    """What ns_csum_tx_ring leaves of one slot: (slot bytes, status, IPv4 sum,
    transport sum).  The gate is verify_frame(first_view=0); both fields are
    zeroed in a copy; packets.fill writes a summed frame (Header = the IP and
    transport headers, Data = the payload up to the IP length as one view); a
    fragment or another IPv4 protocol gets ^c_checksum(header) only."""
    import oracle as O
    import packets as P

    f4, ft, kind = fields(slot, rlen, frame_at, link_hdr)
    if kind is None:
        return bytes(slot), MALFORMED, 0, 0
    if kind == "none":
        return bytes(slot), NONE, 0, 0
    out = bytearray(slot)
    at = frame_at + link_hdr
    ip = bytearray(slot[at:rlen])
    keep4 = bytes(ip[10:12])
    if f4 is not None:
        ip[10:12] = b"\0\0"
    if kind == "l3":
        if flags & L4_ONLY:
            return bytes(slot), NONE, 0, 0
        hlen = (ip[0] & 15) * 4
        net = O.c_checksum(bytes(ip[:hlen]), 0)
        struct.pack_into(">H", out, f4, (~net) & 0xFFFF)
        return bytes(out), L3, net, 0
    ip[ft - at:ft - at + 2] = b"\0\0"
    if ip[0] >> 4 == 4:
        hlen, tlen = (ip[0] & 15) * 4, (ip[2] << 8) | ip[3]
    else:
        hlen, tlen = 40, 40 + ((ip[4] << 8) | ip[5])
    thl = (ip[hlen + 12] >> 4) * 4 if kind == "tcp" else 8
    hdr, net, tr = P.fill(bytes(ip[:hlen + thl]), [bytes(ip[hlen + thl:tlen])], tlen - hlen - thl)
    out[at:at + hlen + thl] = hdr
    if flags & L4_ONLY and f4 is not None:
        out[f4:f4 + 2] = keep4
        net = 0
    return bytes(out), L4, net, tr


def expected_ring(arena: np.ndarray, lens, ring: dict):
    """The arena ns_csum_tx_ring leaves, with status (n) and sums (2n)."""
    off, stride, n = ring.get("ring_off", 0), ring["stride"], ring["n"]
    want = arena.copy()
    status = np.zeros(n, dtype=np.uint8)
    sums = np.zeros(2 * n, dtype=np.uint16)
    for k in range(n):
        lo = off + k * stride
        s, st, a, b = expected_slot(bytes(arena[lo:lo + stride]), int(lens[k]), ring.get("frame_at", 0),
                                    ring.get("link_hdr", 0), ring.get("flags", 0))
        want[lo:lo + stride] = np.frombuffer(s, dtype=np.uint8)
        status[k], sums[2 * k], sums[2 * k + 1] = st, a, b
    return want, status, sums


def build_ring(frames, stride, frame_at=0, link_hdr=0, ring_off=0, seed=0, lens=None, scramble=True):
    """The arena: ring_off random bytes, one slot of `stride` random bytes per
    frame with the frame at frame_at, 64 random bytes after; lens[k] = frame_at
    + the frame's length unless given.  scramble: both checksum fields of
    every frame that has them overwritten with random bytes first."""
    rng = np.random.default_rng(seed)
    n = len(frames)
    arena = rng.integers(0, 256, ring_off + n * stride + 64, dtype=np.uint8)
    out_lens = np.zeros(max(n, 1), dtype=np.uint32)
    for k, f in enumerate(frames):
        at = ring_off + k * stride + frame_at
        f = bytes(f)[:max(stride - frame_at, 0)]
        arena[at:at + len(f)] = np.frombuffer(f, dtype=np.uint8)
        out_lens[k] = frame_at + len(f)
    if lens is not None:
        out_lens[:n] = np.asarray(lens, dtype=np.uint32)
    if scramble:
        for k in range(n):
            lo = ring_off + k * stride
            f4, ft, _ = fields(bytes(arena[lo:lo + stride]), int(out_lens[k]), frame_at, link_hdr)
            for f in (f4, ft):
                if f is not None:
                    arena[lo + f:lo + f + 2] = rng.integers(0, 256, 2, dtype=np.uint8)
    return arena, out_lens


MIXED = [(0, 0), (14, 0), (14, 10), (0, 4)]  # (link_hdr, frame_at)
MIXED_SEEDS = range(7100, 7104)
RING_OFF = 4112


def mixed_ring(seed, link_hdr, frame_at, ring_off=RING_OFF, flags=0):
    """300 random_packet(rng, 3000) frames plus 10 valid UDP/IPv6 datagrams;
    on Ethernet rings frame 5 carries EtherType 0x0806.  Returns (arena,
    lens, ring)."""
    from pktgen import ethernet, random_packet, valid_packet

    rng = np.random.default_rng(seed)
    pk = [random_packet(rng, 3000) for _ in range(300)]
    pk += [valid_packet(rng, "udp6", int(rng.integers(0, 1400))) for _ in range(10)]
    frames = [ethernet(bytes(p)) for p in pk] if link_hdr else [bytes(p) for p in pk]
    if link_hdr:
        frames[5] = ethernet(bytes(pk[5]), 0x0806)
    stride = (max(len(f) for f in frames) + frame_at + 15) // 16 * 16
    arena, lens = build_ring(frames, stride, frame_at, link_hdr, ring_off, seed)
    ring = dict(ring_off=ring_off, stride=stride, n=len(frames), frame_at=frame_at, link_hdr=link_hdr, flags=flags)
    return arena, lens, ring


def assert_ring(got_arena, status, sums, arena, lens, ring):
    """Status, both sums and every byte of the arena against the oracle."""
    want, wst, wsums = expected_ring(arena, lens, ring)
    n = ring["n"]
    for k in range(n):
        got = (int(status[k]), int(sums[2 * k]), int(sums[2 * k + 1]))
        w = (int(wst[k]), int(wsums[2 * k]), int(wsums[2 * k + 1]))
        assert got == w, (k, got, w, int(lens[k]))
    diff = np.nonzero(got_arena != want)[0]
    assert diff.size == 0, (diff[:8].tolist(), ring)
    return wst


def sum_to_ffff(pkt: bytearray, link_hdr: int = 0) -> bytearray:
    """A TCP or UDP packet (a payload of >= 2 bytes) whose last aligned
    payload halfword is rewritten so that the transport sum is 0xffff (the
    field then written is 0x0000)."""
    p = bytearray(pkt)
    _, _, _, tr = expected_slot(bytes(p), len(p), 0, link_hdr)
    ip0 = link_hdr
    hlen = (p[ip0] & 15) * 4 if p[ip0] >> 4 == 4 else 40
    tlen = ((p[ip0 + 2] << 8) | p[ip0 + 3]) if p[ip0] >> 4 == 4 else 40 + ((p[ip0 + 4] << 8) | p[ip0 + 5])
    at = ip0 + hlen + ((tlen - hlen - 2) & ~1)  # an even offset from the transport's start
    x0 = (p[at] << 8) | p[at + 1]

    def fold(v):
        v = (v & 0xFFFF) + (v >> 16)
        return (v + (v >> 16)) & 0xFFFF

    others = fold(tr + ((~x0) & 0xFFFF))
    struct.pack_into(">H", p, at, (~others) & 0xFFFF)
    return p
