#!/usr/bin/env python3
"""The transmit-ring kernel (ns_csum_tx_ring, tx_ring.hip) beside the
receive-ring kernel (ns_csum_rx_ring, the yardstick: the same bytes read,
plus two 2-byte stores per frame) on the same rings in the same run, and the
TX stores at either cache policy (tools/tx_ring_variants.hip, libns_txrv.so)
and with NS_TXR_L4_ONLY (one store per frame instead of two), and the stores
alone (one thread per slot re-storing the fields, no frame loads).
Rings from workloads.rx_ring_batch_sized, two of them alternating so that no
launch re-reads what the one before left in the Infinity Cache:
  mtu      1M x 1500-B IPv4/TCP frames in 1504-B slots
  mtu_eth  the same behind Ethernet headers (1514 B in 1520-B slots)
  short    64-B IPv4/TCP frames in 80-B slots (several slots per 128-B line)
Rounds of back-to-back launches per kernel, interleaved; hipEvent medians in
microseconds per launch, the fraction of 8 TB/s over the algorithmic bytes
(per slot: frame + 4-B length + 1-B status + 4-B sums + the two 2-byte
fields), and TX / RX.  The fill must leave every frame VALID for rx_ring.
One JSON line per workload.
  python tools/tx_ring_probe.py [--rounds 7] [--reps 20] [--only mtu,short]
"""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from netstack_amd import Engine  # noqa: E402
from netstack_amd import workloads as W  # noqa: E402


class TxRingGeo(ctypes.Structure):
    _fields_ = [("ring", ctypes.c_uint64), ("stride", ctypes.c_uint64), ("len", ctypes.c_void_p),
                ("sums", ctypes.c_void_p), ("status", ctypes.c_void_p), ("at", ctypes.c_void_p),
                ("err", ctypes.c_void_p), ("n", ctypes.c_uint32), ("frame_at", ctypes.c_uint32),
                ("link", ctypes.c_uint32), ("flags", ctypes.c_uint32)]


WORKLOADS = {  # name: (slots, frame bytes, Ethernet, stride)
    "mtu": (1 << 20, 1500, False, 1504),
    "mtu_eth": (1 << 20, 1500, True, 1520),
    "short": (1 << 23, 64, False, 80),
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--only", default="")
    ap.add_argument("--scale", type=float, default=1.0, help="slots per ring, as a fraction of the full size")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev)
    eng = Engine(0)
    lib = ctypes.CDLL(os.path.join(ROOT, "netstack_amd", "lib", "libns_txrv.so"))
    lib.txrv_launch.argtypes = [ctypes.POINTER(TxRingGeo), ctypes.c_void_p, ctypes.c_int]
    lib.txrv_launch.restype = ctypes.c_int
    err = torch.zeros(1, dtype=torch.int64, device=dev)
    for name in (args.only.split(",") if args.only else WORKLOADS):
        n, frame, eth, stride = WORKLOADS[name]
        n = max(64, int(n * args.scale))
        lh = 14 if eth else 0
        rings = [W.rx_ring_batch_sized(n, frame, 11 + j, dev, eth=eth, stride=stride) for j in range(2)]
        lens = rings[0][1]
        ring = dict(stride=stride, n=n, link_hdr=lh)
        status = torch.empty(n, dtype=torch.uint8, device=dev)
        verdict = torch.empty(n, dtype=torch.uint8, device=dev)
        sums = torch.empty(2 * n, dtype=torch.int16, device=dev)
        geos = [TxRingGeo(r[0].data_ptr(), stride, lens.data_ptr(), sums.data_ptr(), status.data_ptr(), None,
                          err.data_ptr(), n, 0, lh, 0) for r in rings]

        def rx(j):
            eng.rx_ring(rings[j][0], ring, lens, sums=sums, verdict=verdict, stream=stream)

        def tx(k):
            return lambda j: lib.txrv_launch(ctypes.byref(geos[j]), stream.cuda_stream, k)

        def product(j):
            eng.tx_ring(rings[j][0], ring, lens, sums=sums, status=status, stream=stream)

        geos1 = [TxRingGeo(r[0].data_ptr(), stride, lens.data_ptr(), sums.data_ptr(), status.data_ptr(), None,
                           err.data_ptr(), n, 0, lh, 1) for r in rings]  # NS_TXR_L4_ONLY: one store per frame

        def l4_only(j):
            lib.txrv_launch(ctypes.byref(geos1[j]), stream.cuda_stream, 0)

        runs = {"rx_ring": rx, "tx_ring_product": product, "tx_ring_default_stores": tx(0),
                "tx_ring_nt_sc1_stores": tx(1), "tx_ring_l4_only_default_stores": l4_only,
                "stores_alone_both_fields": tx(2), "stores_alone_transport_field": tx(3)}
        # parity: scramble ring 0's fields, fill, and the receive side must say VALID for all
        ok = {}
        cols = [lh + 10, lh + 11, lh + 36, lh + 37]
        for k in ("tx_ring_product", "tx_ring_default_stores", "tx_ring_nt_sc1_stores"):
            before = rings[0][0].clone()
            for c in cols:
                rings[0][0].view(n, stride)[:, c] ^= 0x5A
            runs[k](0)
            rx(0)
            torch.cuda.synchronize()
            ok[k] = bool((verdict == 1).all()) and bool((status == 1).all()) and bool(torch.equal(rings[0][0], before))
            del before
        res = {k: [] for k in runs}
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        for _ in range(args.rounds):
            for k, fn in runs.items():
                for j in range(3):
                    fn(j % 2)
                ev[0].record(stream)
                for j in range(args.reps):
                    fn(j % 2)
                ev[1].record(stream)
                torch.cuda.synchronize()
                res[k].append(ev[0].elapsed_time(ev[1]) * 1e3 / args.reps)
        algo = n * (frame + lh + 4 + 1 + 4 + 4)
        out = {}
        for k in runs:
            us = float(np.median(res[k]))
            out[k] = {"us": round(us, 2), "min_us": round(min(res[k]), 2), "max_us": round(max(res[k]), 2),
                      "frac_of_8TBps": round(algo / us / 1e3 / 8000, 4)}
            if k in ok:
                out[k]["parity"] = ok[k]
        rxus = out["rx_ring"]["us"]
        print(json.dumps({"workload": f"{name}: {n} x {frame + lh}-B IPv4/TCP frames in {stride}-B slots, 2 rotating rings",
                          "rounds": args.rounds, "reps": args.reps, "algo_bytes": algo, "kernels": out,
                          "tx_over_rx": {k: round(out[k]["us"] / rxus, 4) for k in out if k != "rx_ring"}}), flush=True)
        del rings, geos, geos1, status, verdict, sums
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
