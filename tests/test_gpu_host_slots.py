"""GPU: the four host DMA pipelines (ns_csum_rx_ring_host, ns_csum_tx_ring_host,
ns_csum_tcp_tx_host, ns_csum_batch_host) with 1, 2 and 3 chunks in flight.
Every other test runs the default four slots; NS_CSUM_HOST_SLOTS is read per
context in ns_csum_init, so it is set before an Engine is made.  Each case is
the smallest whose chunks outnumber the slots (the rotation of
nsh::run_slots reuses every slot), compared bit for bit with the oracle."""

import numpy as np
import pytest

import txcases as T
from test_gpu_rx_ring import _frames, _ring
from test_gpu_rx_ring_host import _want as _rx_want
from test_gpu_tx_host import _check as _tx_check
from test_gpu_tx_host import _layout as _tx_layout
from test_gpu_tx_host import _want as _tx_want

pytestmark = pytest.mark.gpu

STRIDE, NRING = 96, 50


@pytest.fixture(params=[1, 2, 3])
def slots(request, monkeypatch):
    monkeypatch.setenv("NS_CSUM_HOST_SLOTS", str(request.param))
    return request.param


@pytest.fixture(scope="module")
def rx_case():
    rng = np.random.default_rng(8100)
    _, frames = _frames(rng, NRING, 0, max_payload=24)
    arena, lens = _ring(frames, STRIDE, ring_off=3)
    ring = dict(ring_off=3, stride=STRIDE, n=NRING)
    return arena, lens, ring, _rx_want(arena, lens, ring)


@pytest.fixture(scope="module")
def tx_ring_case():
    from pktgen import random_packet

    rng = np.random.default_rng(8200)
    frames = [bytes(random_packet(rng, 24)) for _ in range(NRING)]
    arena, lens = T.build_ring(frames, STRIDE, ring_off=5, seed=8200)
    ring = dict(ring_off=5, stride=STRIDE, n=NRING)
    return arena, lens, ring, T.expected_ring(arena, lens, ring)


@pytest.fixture(scope="module")
def tcp_tx_case(oracle_mod):
    geos, a = _tx_layout(13 + 4096)
    return geos, a, _tx_want(oracle_mod, a, geos)


@pytest.fixture(scope="module")
def batch_cases(oracle_mod):
    """6,000 descriptors, lengths in [0, 400), unaligned starts, random
    initial values: plain, and with NS_DESC_CONT runs."""
    rng = np.random.default_rng(8300)
    n = 6000
    lengths = rng.integers(0, 400, n).astype(np.uint32)
    off = np.zeros(n, np.uint64)
    pos = 3
    for k in range(n):
        pos = (pos // 16) * 16 + int(rng.integers(0, 16))
        off[k] = pos
        pos += int(lengths[k]) + int(rng.integers(0, 40))
    arena = rng.integers(0, 256, pos + 64, dtype=np.uint8)
    out = []
    for chained in (False, True):
        d = np.zeros(n, dtype=oracle_mod.DESC_DTYPE)
        d["off"], d["len"] = off, lengths
        d["initial"] = rng.integers(0, 65536, n)
        d["flags"] = rng.integers(0, 2, n)
        if chained:
            d["flags"] |= (2 * (rng.random(n) < 0.4)).astype(np.uint16)
        want, bad = oracle_mod.c_batch(arena, d, chained=chained)
        assert bad == 0
        out.append((d, chained, want))
    return arena, out


def test_rx_ring_host(slots, rx_case):
    from netstack_amd import Engine

    arena, lens, ring, (wv, ws) = rx_case
    with Engine(0, staging_bytes=7 * STRIDE) as eng:  # 8 chunks
        verdict, sums = eng.rx_ring_host(arena, ring, lens)
        assert eng.sync() == 0
    assert np.array_equal(verdict, wv) and np.array_equal(sums, ws)
    assert len(set(wv.tolist())) > 1


def test_tx_ring_host(slots, tx_ring_case):
    from netstack_amd import Engine

    arena, lens, ring, (want, wst, wsums) = tx_ring_case
    host = arena.copy()
    with Engine(0, staging_bytes=7 * STRIDE) as eng:  # 8 chunks
        status, sums = eng.tx_ring_host(host, ring, lens)
        assert eng.sync() == 0
    assert np.array_equal(status, wst) and np.array_equal(sums, wsums)
    assert np.array_equal(host, want), np.flatnonzero(host != want)[:8]
    assert len(set(wst.tolist())) > 1


def test_tcp_tx_host(slots, tcp_tx_case):
    from netstack_amd import Engine

    geos, a, (want, ws) = tcp_tx_case
    got = a.copy()
    with Engine(0, staging_bytes=4096) as eng:
        sums = eng.tcp_tx_host(got, geos)
        assert eng.sync() == 0
    _tx_check(got, sums, want, ws, f"{slots} slots")


def test_batch_host(slots, batch_cases, monkeypatch):
    from netstack_amd import Engine

    monkeypatch.setenv("NS_CSUM_HOST_CHUNK", "1024")  # the smallest ns_csum_init accepts: 6 chunks
    arena, cases = batch_cases
    assert arena.nbytes > 1 << 20  # past the zero-copy pass (kStageBytes): the DMA pipeline
    with Engine(0) as eng:
        for d, chained, want in cases:
            got = eng.batch_host(arena, d, chained=chained)
            assert np.array_equal(got, want), (chained, np.flatnonzero(got != want)[:8])
        assert eng.sync() == 0
