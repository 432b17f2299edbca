"""GPU: ns_csum_tx_ring_host — a transmit ring in HOST memory (the frames a
link endpoint queued for sendmmsg, link/fdbased/endpoint.go:443-556), parsed
and summed on the device with no host planning, the fields then written into
the host ring from the device's report.  The same mixed rings as
tests/test_gpu_tx_ring.py against the oracle (tests/txcases.py), byte for
byte: from pageable memory and from stage_acquire'd memory, with a staging
budget of a few slots (chunks cycling through the four pipeline slots), at
unaligned ring offsets, and netstack_amd.tx.fill_frames."""
import ctypes

import numpy as np
import pytest

import txcases as T

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mixed():
    out = {}
    for (link_hdr, frame_at), seed in zip(T.MIXED, T.MIXED_SEEDS):
        arena, lens, ring = T.mixed_ring(seed, link_hdr, frame_at)
        out[(link_hdr, frame_at)] = (arena, lens, ring, T.expected_ring(arena, lens, ring))
    return out


def _same(got, status, sums, want):
    w, wst, wsums = want
    assert status.tolist() == wst.tolist()
    assert sums.tolist() == wsums.tolist()
    assert np.array_equal(got, w), np.nonzero(got != w)[0][:8]


@pytest.mark.parametrize("link_hdr,frame_at", T.MIXED)
def test_pageable_ring_matches_oracle(engine, mixed, link_hdr, frame_at):
    arena, lens, ring, want = mixed[(link_hdr, frame_at)]
    host = arena.copy()
    status, sums = engine.tx_ring_host(host, ring, lens)
    _same(host, status, sums, want)
    # a second call changes nothing
    status, sums = engine.tx_ring_host(host, ring, lens)
    _same(host, status, sums, want)


@pytest.mark.parametrize("link_hdr,frame_at", [(14, 0), (0, 4)])
def test_staged_ring_matches_oracle(engine, mixed, link_hdr, frame_at):
    arena, lens, ring, want = mixed[(link_hdr, frame_at)]
    stage = engine.stage_acquire(arena.size)
    try:
        stage[:] = arena
        status, sums = engine.tx_ring_host(stage, ring, lens)
        _same(np.array(stage), status, sums, want)
    finally:
        engine.stage_release(stage)


@pytest.mark.parametrize("ring_off", [0, 3, 1001])
def test_small_staging_and_unaligned_ring(oracle_mod, ring_off):
    """A staging budget of 7 slots: the ring goes up in chunks that cycle
    through the four pipeline slots; the host ring need not be 16-B aligned."""
    from netstack_amd import Engine

    arena, lens, ring = T.mixed_ring(7110 + ring_off, 14, 0, ring_off=ring_off)
    want = T.expected_ring(arena, lens, ring)
    host = arena.copy()
    with Engine(0, staging_bytes=7 * ring["stride"]) as eng:
        status, sums = eng.tx_ring_host(host, ring, lens)
        assert eng.sync() == 0
    _same(host, status, sums, want)
    assert {T.NONE, T.L4, T.L3, T.MALFORMED} <= set(status.tolist())


def test_l4_only_and_short_slots(engine):
    """NS_TXR_L4_ONLY through the host ring, and 80-B slots (several frames
    per line of the staged copy)."""
    from pktgen import valid_packet

    arena, lens, ring = T.mixed_ring(7120, 0, 0, ring_off=7, flags=T.L4_ONLY)
    host = arena.copy()
    status, sums = engine.tx_ring_host(host, ring, lens)
    _same(host, status, sums, T.expected_ring(arena, lens, ring))
    assert T.L3 not in set(status.tolist()) and not sums[0::2].any()
    rng = np.random.default_rng(7121)
    frames = [bytes(valid_packet(rng, ("tcp4", "udp4", "icmp4", "udp6")[k % 4], int(rng.integers(0, 17))))
              for k in range(500)]
    arena, lens = T.build_ring(frames, 80, ring_off=2, seed=5)
    ring = dict(ring_off=2, stride=80, n=len(frames))
    host = arena.copy()
    status, sums = engine.tx_ring_host(host, ring, lens)
    _same(host, status, sums, T.expected_ring(arena, lens, ring))


def test_length_over_the_stride_is_counted_and_untouched(engine):
    from pktgen import valid_packet

    rng = np.random.default_rng(7130)
    frames = [bytes(valid_packet(rng, "udp4", 100)) for _ in range(6)]
    arena, lens = T.build_ring(frames, 144, seed=6)
    lens[2] = 145
    ring = dict(stride=144, n=6)
    host = arena.copy()
    engine.sync()
    status, sums = engine.tx_ring_host(host, ring, lens)
    assert engine.sync() == 1
    _same(host, status, sums, T.expected_ring(arena, lens, ring))
    assert status[2] == T.MALFORMED


def test_outputs_may_be_null_and_errors(engine, mixed):
    from netstack_amd import _lib

    arena, lens, ring, want = mixed[(0, 0)]
    host = arena.copy()
    L, h = _lib.lib(), engine._h
    r = _lib.NsTxRing(ring["ring_off"], ring["stride"], ring["n"], 0, 0, 0, 0)
    assert L.ns_csum_tx_ring_host(h, host.ctypes.data, host.size, ctypes.byref(r), lens.ctypes.data, None,
                                  None) == _lib.NS_OK  # the stores are the result
    assert np.array_equal(host, want[0])
    assert L.ns_csum_tx_ring_host(h, host.ctypes.data, host.size, ctypes.byref(r), None, None,
                                  None) == _lib.NS_EINVAL  # no lengths
    with pytest.raises(ValueError):  # stride not a multiple of 16
        engine.tx_ring_host(host, dict(ring, stride=1500), lens)
    with pytest.raises(ValueError):  # an unknown flag
        engine.tx_ring_host(host, dict(ring, flags=4), lens)
    with pytest.raises(ValueError):
        engine.tx_ring_host(host, dict(ring, pad=1), lens)
    with pytest.raises(_lib.ChecksumError) as e:  # past the arena
        engine.tx_ring_host(host[:ring["ring_off"] + ring["stride"] * ring["n"] - 1], ring, lens)
    assert e.value.status == _lib.NS_ERANGE
    s0, u0 = engine.tx_ring_host(host, dict(ring, n=0), lens)
    assert s0.size == 0 and u0.size == 0
    assert np.array_equal(host, want[0])


@pytest.mark.parametrize("link_hdr,l4_only", [(0, False), (14, False), (14, True)])
def test_fill_frames_matches_oracle(engine, link_hdr, l4_only):
    from netstack_amd import fill_frames
    from pktgen import ethernet, random_packet, valid_packet

    rng = np.random.default_rng(7140 + link_hdr)
    pk = [bytes(random_packet(rng, 1400)) for _ in range(200)]
    pk += [bytes(valid_packet(rng, "udp6", int(rng.integers(0, 1400)))) for _ in range(8)]
    frames = [ethernet(p) for p in pk] if link_hdr else pk
    if link_hdr:
        frames[3] = ethernet(pk[3], 0x0806)
    frames = [f for f in frames if len(f) > 0]
    # checksum offload: the transports left their fields zero
    clean = []
    for f in frames:
        b = bytearray(f)
        f4, ft, _ = T.fields(bytes(b), len(b), 0, link_hdr)
        for at in (f4, ft):
            if at is not None and not (l4_only and at == f4):
                b[at:at + 2] = b"\0\0"
        clean.append(bytes(b))
    out, status = fill_frames(clean, link_hdr=link_hdr, engine=engine, l4_only=l4_only)
    assert len(out) == len(clean) and status.shape == (len(clean),)
    for k, f in enumerate(clean):
        w, st, _, _ = T.expected_slot(f, len(f), 0, link_hdr, T.L4_ONLY if l4_only else 0)
        assert out[k] == w and status[k] == st, k
    assert {T.L4, T.MALFORMED} <= set(status.tolist())
    assert fill_frames([], engine=engine)[0] == []
