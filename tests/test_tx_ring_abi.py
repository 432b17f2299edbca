"""CPU: the transmit ring's boundary (ns_csum_tx_ring, ns_csum_tx_ring_host;
include/netstack_csum.h): both symbols exported, the struct's layout, argument
errors before any device call, the kernel's resource report, and the host
ring's patch loop (nsh::tx_ring_patch, host_logic.h) as a stand-alone program
under ASan + UBSan."""
import ctypes
import os
import re
import subprocess

from conftest import ROOT
from netstack_amd import _lib

CSRC = os.path.join(ROOT, "netstack_amd", "csrc")
LIB = os.path.join(ROOT, "netstack_amd", "lib")


def test_both_symbols_are_exported_and_bound():
    L = _lib.lib()
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    for s in ("ns_csum_tx_ring", "ns_csum_tx_ring_host"):
        assert s in _lib.EXPORTED
        assert re.search(rf"\bT {s}\b", out), f"{s} not exported with C linkage"
        assert getattr(L, s).argtypes is not None
    assert L.ns_csum_abi_version() == 9  # two symbols added, nothing changed


def test_struct_layout_and_constants():
    assert ctypes.sizeof(_lib.NsTxRing) == 32
    assert [(_lib.NsTxRing.ring_off.offset, _lib.NsTxRing.stride.offset, _lib.NsTxRing.n.offset,
             _lib.NsTxRing.frame_at.offset, _lib.NsTxRing.link_hdr.offset, _lib.NsTxRing.flags.offset,
             _lib.NsTxRing.pad.offset)] == [(0, 8, 16, 20, 22, 24, 28)]
    txt = open(os.path.join(ROOT, "include", "netstack_csum.h")).read()
    for name, val in (("NS_TXR_L4_ONLY", 1), ("NS_TXR_NONE", 0), ("NS_TXR_L4", 1), ("NS_TXR_L3", 2),
                      ("NS_TXR_MALFORMED", 3)):
        m = re.search(rf"#define {name} (0x)?(\d+)u", txt)
        assert m and int(m.group(2)) == val == getattr(_lib, name), name


def test_null_context_and_bad_arguments_are_einval_without_a_device():
    L = _lib.lib()
    r = _lib.NsTxRing(0, 1504, 1, 0, 0, 0, 0)
    buf = (ctypes.c_uint8 * 4096)()
    u32 = (ctypes.c_uint32 * 4)()
    assert L.ns_csum_tx_ring(None, buf, 4096, ctypes.byref(r), u32, None, None, None) == _lib.NS_EINVAL
    assert L.ns_csum_tx_ring_host(None, buf, 4096, ctypes.byref(r), u32, None, None) == _lib.NS_EINVAL


def test_kernel_resource_report_has_no_scratch():
    tx = {}
    cur = None
    for line in open(os.path.join(LIB, "tx_ring.resources.txt")).read().splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = m.group(1)
            tx[cur] = {}
            continue
        m = re.search(r"(ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|VGPRs): (\d+)", line)
        if m and cur:
            tx[cur][m.group(1).split()[0]] = int(m.group(2))
    assert len(tx) >= 1 and all("tx_ring" in k for k in tx), sorted(tx)
    for k, v in tx.items():
        assert v["ScratchSize"] == 0, (k, v)


def test_patch_loop_under_address_and_undefined_behaviour_sanitizers():
    """tests/cpp/tx_ring_patch_test.cc: in-range, out-of-range and garbage
    offsets and lengths; only the permitted bytes change and nothing outside
    the ring is touched."""
    subprocess.run(["make", "-s", "-C", CSRC, "tx_ring_patch_test"], check=True, timeout=600)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    p = subprocess.run([os.path.join(LIB, "tx_ring_patch_asan")], capture_output=True, text=True, env=env, timeout=300)
    out = p.stdout + p.stderr
    assert p.returncode == 0, out[-4000:]
    assert "ERROR: AddressSanitizer" not in out and "runtime error" not in out, out[-4000:]
    assert "tx_ring_patch_test ok" in p.stdout
