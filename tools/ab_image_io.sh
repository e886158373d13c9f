#!/bin/bash
# A/B on ONE box for the image path: tools/image_io_bench.py with every row on this tree, then its evaluation step alone (--eval-only),
# alternating an earlier tree (_old/, through LVAE_TREE) and this one, N times each (default 5).  One JSON line per run on stdout.
# _old/ is scratch (git-excluded): git worktree add _old <commit> && (cd _old && python lossy-vae_amd/build_native.py)
# Every run has its own time limit; the first failing run ends the script.
#   tools/ab_image_io.sh [N] [STEPS]
set -o pipefail
R=$(cd "$(dirname "$0")/.." && pwd)
N=${1:-5}
STEPS=${2:-30}
run() {
  local out
  out=$(timeout -k 10 300 "$@" 2>/dev/null | tail -1) || { echo "FAILED: $*"; exit 1; }
  [ -n "$out" ] || { echo "FAILED (no output): $*"; exit 1; }
  echo "$out"
}
cd "$R" || exit 1
run python tools/image_io_bench.py --steps "$STEPS" --tag new_all_rows
for i in $(seq 1 "$N"); do
  run env LVAE_TREE="$R/_old" python tools/image_io_bench.py --steps "$STEPS" --eval-only --tag "old_$i"
  run python tools/image_io_bench.py --steps "$STEPS" --eval-only --tag "new_$i"
done
