# Round-5 final verification: determinism (alone + co-run), the whole GPU suite, smoke, the bench line
# (with the CPU baseline), config 5's bench line, kernel-trace stats of the one-lane pass, HBM traffic PMC
# passes at the roofline's configuration (one lane: Bt = 256 per launch), training steps and the DDIM
# kernel trace.
set -o pipefail
cd "$(dirname "$0")/../.."
export TMPDIR=/tmp
OUT=${OUT:-bench_out}
mkdir -p "$OUT"
T=${1:-r05_fin}
timeout -k 10 200 python -u tools/determinism_probe.py > $OUT/${T}_det.log 2>&1 && \
timeout -k 10 200 python -u tools/determinism_probe.py --corun > $OUT/${T}_corun.log 2>&1 && \
grep -q "^deterministic" $OUT/${T}_det.log && grep -q "^deterministic" $OUT/${T}_corun.log && \
timeout -k 10 900 python -u -m pytest tests -m gpu -x -q --timeout 400 --timeout-method thread > $OUT/${T}_gpu_tests.log 2>&1 && \
timeout -k 10 300 python -u -c "import __graft_entry__ as g; g.smoke(); print('smoke ok')" > $OUT/${T}_smoke.log 2>&1 && \
timeout -k 10 500 python -u bench.py --full > $OUT/${T}_bench.log 2>&1 && \
timeout -k 10 300 python -u bench.py --full --img-size 256 --batch 64 --precision bf16 --no-cpu-baseline --steps 1 --warmup 1 > $OUT/${T}_c5.log 2>&1 && \
timeout -k 10 300 rocprofv3 --kernel-trace --stats -d $OUT/${T}_prof -o run -- python3 bench.py --steps 1 --warmup 1 --no-cpu-baseline --lanes 1 --fp32-passes 0 > $OUT/${T}_prof.log 2>&1 && \
timeout -s KILL 240 rocprofv3 --pmc FETCH_SIZE --output-format csv -d $OUT/${T}_fetch -o p -- python3 bench.py --n-steps 2 --steps 1 --warmup 0 --no-cpu-baseline --fp32-passes 0 --lanes 1 > $OUT/${T}_fetch.log 2>&1 && \
timeout -s KILL 240 rocprofv3 --pmc WRITE_SIZE --output-format csv -d $OUT/${T}_write -o p -- python3 bench.py --n-steps 2 --steps 1 --warmup 0 --no-cpu-baseline --fp32-passes 0 --lanes 1 > $OUT/${T}_write.log 2>&1 && \
python3 tools/pmc_traffic.py $OUT/${T}_fetch $OUT/${T}_write > $OUT/${T}_pmc_traffic.txt 2>&1 && \
STEPS=10 WARM=3 timeout -k 10 300 python -u tools/train_bench.py score vae prior ddim > $OUT/${T}_train.log 2>&1 && \
STEPS=3 WARM=1 timeout -k 10 300 rocprofv3 --kernel-trace --stats -d $OUT/${T}_ddim -o run -- python3 tools/train_bench.py ddim > $OUT/${T}_ddim.log 2>&1
