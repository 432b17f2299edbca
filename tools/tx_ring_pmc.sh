#!/bin/bash
# rocprofv3 --pmc passes over the receive-ring and the transmit-ring kernel on
# the same rings (tools/tx_ring_pmc.py): FETCH_SIZE and WRITE_SIZE, each
# counter and each kernel in a run of its own, counters never combined with
# tracing domains.  Summaries (tools/pmc_parse.py) under OUTDIR (default:
# build/pmc_tx_ring, git-ignored).
#   tools/tx_ring_pmc.sh [OUTDIR]
set -euo pipefail
R=$(cd "$(dirname "$0")/.." && pwd)
OUT=${1:-$R/build/pmc_tx_ring}
mkdir -p "$OUT"
export TMPDIR=/tmp
cd "$R"
run() {  # kernel, counter
  local name=$1_$2
  timeout -k 10 240 rocprofv3 --pmc "$2" -d "$OUT/$name" -o run --output-format csv \
    -- python3 tools/tx_ring_pmc.py --kernel "$1" > "$OUT/$name.log" 2>&1
  python3 tools/pmc_parse.py "$OUT/$name" "$OUT/$name.log" > "$OUT/${name}_summary.json"
}
run rx FETCH_SIZE
run rx WRITE_SIZE
run tx FETCH_SIZE
run tx WRITE_SIZE
run tx_l4_only WRITE_SIZE
echo "pmc tx_ring done"
