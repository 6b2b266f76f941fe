#!/bin/bash
# GPU box check: build, pytest -m gpu, bench, rocprofv3 kernel stats (+ optional PMC passes).
# usage: bash tools/gpu_check.sh [tests] [smoke] [bench] [prof] [multi] [pmc]   (default: tests bench prof)
# Logs and results go to $CODEC_CHECK_OUT (default: build/check under the repository, git-ignored).
R="$(cd "$(dirname "${BASH_SOURCE[0]}")/.." && pwd)"
cd "$R" || exit 9
OUT="${CODEC_CHECK_OUT:-$R/build/check}"
mkdir -p "$OUT"
STAGES="${*:-tests bench prof}"
has() { [[ " $STAGES " == *" $1 "* ]]; }
python -c "import __graft_entry__ as g; g.build()" > "$OUT/build.log" 2>&1 || { echo build failed; tail "$OUT/build.log"; exit 3; }
if has tests; then
  timeout -k 10 900 python -u -m pytest tests -m gpu -q --maxfail=8 -p no:cacheprovider --timeout 120 --timeout-method thread > "$OUT/pytest_gpu.log" 2>&1; rc=$?
  echo "pytest rc=$rc"; tail -25 "$OUT/pytest_gpu.log"
  [ $rc -le 1 ] || exit $rc
fi
if has smoke; then
  timeout -k 10 300 python __graft_entry__.py smoke > "$OUT/smoke.log" 2>&1; rc=$?; echo "smoke rc=$rc"; tail -5 "$OUT/smoke.log"
  [ $rc -eq 0 ] || exit $rc
fi
if has bench; then
  # --full: every side leg, check and baseline in the JSON line (a plain run times the headline step only)
  timeout -k 10 600 python bench.py --full > "$OUT/bench.json" 2> "$OUT/bench.err"; rc=$?
  echo "bench rc=$rc"; cat "$OUT/bench.json"; tail -5 "$OUT/bench.err"
  [ $rc -eq 0 ] || exit $rc
fi
if has prof; then
  ( cd /tmp && export TMPDIR=/tmp && timeout -k 10 400 rocprofv3 --kernel-trace --stats --output-format csv \
      -d "$OUT/prof" -o run -- python3 "$R/bench.py" --full --steps 10 --warmup 2 --cpu-seconds 0 --c3 0 --c2 0 \
      > "$OUT/prof_bench.json" 2> "$OUT/prof.log" ); rc=$?
  echo "rocprof rc=$rc"; tail -3 "$OUT/prof.log"
  find "$OUT/prof" -name "*stats*" | head
  [ $rc -eq 0 ] || exit $rc
fi
if has multi; then
  # 2-rank rehearsal of the N>1 path on a 1-GPU box (gloo: RCCL needs distinct GPUs)
  timeout -k 10 400 python -m torch.distributed.run --nnodes=1 --nproc-per-node 2 --master-addr 127.0.0.1 \
      --master-port 29533 bench.py --full --gpus 2 --steps 5 --warmup 1 --batch 64 --backend gloo --cpu-seconds 0 \
      > "$OUT/bench_multi.json" 2> "$OUT/bench_multi.err"; rc=$?
  echo "multi rc=$rc"; cat "$OUT/bench_multi.json"; tail -5 "$OUT/bench_multi.err"
  [ $rc -eq 0 ] || exit $rc
fi
if has pmc; then
  for C in FETCH_SIZE WRITE_SIZE; do
    ( cd /tmp && export TMPDIR=/tmp && timeout -k 10 400 rocprofv3 --pmc $C --kernel-trace --output-format csv \
        -d "$OUT/pmc_$C" -o run -- python3 "$R/bench.py" --full --steps 3 --warmup 1 --cpu-seconds 0 --no-profile --c3 0 --c2 0 \
        > "$OUT/pmc_$C.log" 2>&1 ); rc=$?
    echo "pmc $C rc=$rc"; tail -2 "$OUT/pmc_$C.log"
    [ $rc -eq 0 ] || exit $rc
  done
fi
