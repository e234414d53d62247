#!/bin/bash
# GPU session script (one parametrised script instead of a file per run).   tools/gpu_session.sh <tag> <what...>
#   what: new   -- the tests round 6 added / touched        full  -- the whole GPU suite + smoke + the full bench line
#         train -- tools/bench_train.py (bf16 + fp32 step)  bench -- the full bench line only (bench.py --full)     k=<expr> -- pytest -k <expr>
# Records go to $WN_RESULTS (default: results/ in the repository root).
TAG=$1; shift
cd "$(dirname "$0")/.."
OUT=${WN_RESULTS:-results}
mkdir -p "$OUT"
# every GPU step runs under a time limit of its own; the first step that fails, faults or times out ends the session
set -o pipefail
for what in "$@"; do
  case $what in
    new)
      ( time timeout -k 10 1500 python -m pytest tests/test_gpu_train_cfg5.py tests/test_gpu_convergence.py -m gpu -q -s 2>&1 | grep -v "^$" | tail -150 ) 2>&1 | tee "$OUT"/pytest_new_$TAG.txt || exit 1
      ( time timeout -k 10 900 python -m pytest tests/test_gpu_training.py -m gpu -q -x 2>&1 | tail -8 ) 2>&1 | tee -a "$OUT"/pytest_new_$TAG.txt || exit 1
      ( time timeout -k 10 900 python -m pytest tests/test_gpu_parity.py -m gpu -q -x -s -k "busy or resident or taken" 2>&1 | tail -12 ) 2>&1 | tee -a "$OUT"/pytest_new_$TAG.txt || exit 1 ;;
    full) bash tools/gpu_validate.sh $TAG || exit 1 ;;
    train) ( timeout -k 10 600 python tools/bench_train.py 32 16000 --no-torch --reps=5 2>&1 | tail -6 ) | tee "$OUT"/train_$TAG.txt || exit 1 ;;
    traindet) ( WN_DETERMINISTIC=1 timeout -k 10 600 python tools/bench_train.py 32 16000 --no-torch --reps=5 2>&1 | tail -6 ) | tee "$OUT"/traindet_$TAG.txt || exit 1 ;;
    cfg5) ( time timeout -k 10 1500 python -m pytest tests/test_gpu_train_cfg5.py -m gpu -q -s 2>&1 | grep -v "^$" | tail -150 ) 2>&1 | tee "$OUT"/pytest_cfg5_$TAG.txt || exit 1 ;;
    bench) ( time timeout -k 10 900 python bench.py --full 2> "$OUT"/bench_$TAG.err | tail -1 > "$OUT"/bench_$TAG.json ) 2>&1 | tail -3 || { tail -3 "$OUT"/bench_$TAG.err; exit 1; }; tail -3 "$OUT"/bench_$TAG.err ;;
    k=*) ( time timeout -k 10 1500 python -m pytest tests -m gpu -q -x -s -k "${what#k=}" 2>&1 | tail -30 ) 2>&1 | tee "$OUT"/pytest_k_$TAG.txt || exit 1 ;;
    *) echo "unknown: $what" ;;
  esac
done
