"""A link endpoint with TX checksum offload, in Python: the frames it queued
for sendmmsg (ACKs, UDP datagrams, ICMP replies, non-GSO TCP of many
endpoints; link/fdbased/endpoint.go:443-556) packed into a staged host ring
and filled by ns_csum_tx_ring_host.  With CapabilityTXChecksumOffload the
transports leave their checksum fields zero (transport/tcp/connect.go:661,
transport/udp/endpoint.go:809) and the link owes the full checksum, pseudo-
header included; the parse and the sums run on the device, nothing is planned
or summed here.
"""
from __future__ import annotations

import numpy as np

from . import _lib
from .engine import Engine, default_engine


def fill_frames(frames, link_hdr: int = 0, engine: Engine | None = None, l4_only: bool = False):
    """Fill the checksum fields of complete outgoing frames: `frames` a list
    of byte strings (each starting with its link header of `link_hdr` bytes,
    0 or 14).  Returns (filled frames, status): the frames as byte strings
    with the fields written, and a uint8 array of NS_TXR_* per frame
    (NS_TXR_MALFORMED frames come back unchanged).  l4_only: leave the IPv4
    header checksum as it is (NS_TXR_L4_ONLY)."""
    eng = engine if engine is not None else default_engine()
    n = len(frames)
    if n == 0:
        return [], np.zeros(0, dtype=np.uint8)
    # one ring of 16-B-rounded slots, as long as the longest frame
    stride = max(16, (max(len(f) for f in frames) + 15) & ~15)
    stage = eng.stage_acquire(n * stride)
    try:
        ring = stage[:n * stride].reshape(n, stride)
        lens = np.empty(n, dtype=np.uint32)
        for k, f in enumerate(frames):
            ring[k, :len(f)] = np.frombuffer(f, dtype=np.uint8)
            ring[k, len(f):] = 0
            lens[k] = len(f)
        status, _ = eng.tx_ring_host(stage, dict(stride=stride, n=n, link_hdr=link_hdr,
                                                 flags=_lib.NS_TXR_L4_ONLY if l4_only else 0), lens)
        out = [ring[k, :int(lens[k])].tobytes() for k in range(n)]
    finally:
        eng.stage_release(stage)
    return out, status
