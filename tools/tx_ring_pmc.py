#!/usr/bin/env python3
"""Workload for rocprofv3 --pmc passes over ONE ring kernel (tools/
tx_ring_pmc.sh): the 16-lane-group calibration read of a known byte count,
then REPS launches of ns_csum_rx_ring (--kernel rx) or ns_csum_tx_ring
(--kernel tx) over two alternating rings of 1M x 1500-B IPv4/TCP frames in
1504-B slots (tools/tx_ring_probe.py's `mtu`).  LABEL lines as tools/
pmc_run.py prints them, for tools/pmc_parse.py."""
import argparse
import ctypes
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from netstack_amd import Engine  # noqa: E402
from netstack_amd import workloads as W  # noqa: E402

REPS = 3
CAL_BYTES = (1 << 31) - 4096


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernel", required=True, choices=("rx", "tx", "tx_l4_only"))
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    L = ctypes.CDLL(os.path.join(ROOT, "netstack_amd", "lib", "libns_tune.so"))
    L.nsk_calib_launch.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p,
                                   ctypes.c_uint32, ctypes.c_void_p]
    sp = torch.cuda.current_stream(dev).cuda_stream
    buf = torch.ones(CAL_BYTES, dtype=torch.uint8, device=dev)
    outb = torch.zeros(65536, dtype=torch.int32, device=dev)
    for _ in range(REPS):
        assert L.nsk_calib_launch(2164, buf.data_ptr(), CAL_BYTES, outb.data_ptr(), 8192, sp) == 0
    torch.cuda.synchronize()
    print(f"LABEL calib2164 bytes={CAL_BYTES}", flush=True)
    del buf
    torch.cuda.empty_cache()
    eng = Engine(0)
    n, frame, stride = 1 << 20, 1500, 1504
    rings = [W.rx_ring_batch_sized(n, frame, 11 + j, dev, stride=stride) for j in range(2)]
    lens = rings[0][1]
    out8 = torch.empty(n, dtype=torch.uint8, device=dev)
    sums = torch.empty(2 * n, dtype=torch.int16, device=dev)
    ring = dict(stride=stride, n=n, flags=1 if args.kernel == "tx_l4_only" else 0)
    torch.cuda.synchronize()
    for j in range(REPS):
        if args.kernel == "rx":
            eng.rx_ring(rings[j % 2][0], dict(stride=stride, n=n), lens, sums=sums, verdict=out8)
        else:
            eng.tx_ring(rings[j % 2][0], ring, lens, sums=sums, status=out8)
    torch.cuda.synchronize()
    print(f"LABEL {args.kernel}_ring algorithmic_bytes={n * (frame + 13)} payload={n * frame} arena={n * stride} "
          f"n={n} shape=calib2164 rotated=2", flush=True)


if __name__ == "__main__":
    main()
