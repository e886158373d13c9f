#!/bin/bash
# A/B on ONE box: an earlier tree (_old/) vs the current tree, alternating processes of the default bench, then of --batch 1 (where the
# per-launch host time weighs most).  _old/ is scratch (git-excluded): the earlier commit's files with its library built in place
# (git archive <commit> | tar -x -C _old && python _old/lossy-vae_amd/build_native.py).
#   tools/ab_bench.sh [processes per tree and setting, default 2]
# Prints one row per process -- tag, Mpixels/s, ms per step, encode ms, decode ms -- and stops at the first process that fails.
set -eo pipefail
R=$(cd "$(dirname "$0")/.." && pwd)
N=${1:-2}
run() {
  local tag=$1 dir=$2; shift 2
  (cd "$dir" && timeout -k 10 300 python bench.py "$@" 2>/dev/null) | python -c "import sys,json; j=json.loads(sys.stdin.read()); print('$tag', j['value'], j['ms_per_step'], j['enc_ms_per_step'], j['dec_ms_per_step'])"
}
for i in $(seq "$N"); do run OLD "$R/_old"; run NEW "$R"; done
for i in $(seq "$N"); do run 'OLD b1' "$R/_old" --batch 1; run 'NEW b1' "$R" --batch 1; done
