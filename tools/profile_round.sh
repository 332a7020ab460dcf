# Round profile of bench.py --full (every kernel of the side measurements too) on the GPU box,
# run from the repo root; output under $PROFILE_OUT (default: profile_out/ in the repo root):
#   1. rocprofv3 --kernel-trace --stats  -> prof/bench_results.db (+ the bench line)
#   2. rocprofv3 --pmc FETCH_SIZE         -> pmc_fetch/  (separate pass)
#   3. rocprofv3 --pmc WRITE_SIZE         -> pmc_write/  (separate pass)
# Summaries: tools/prof_summary.py and tools/pmc_summary.py (on the CPU side).
set -e
R=${GRAFT_REPO_ROOT:-$(pwd)}
O=${PROFILE_OUT:-$R/profile_out}
cd /tmp && export TMPDIR=/tmp
mkdir -p $O
timeout -k 10 300 rocprofv3 --kernel-trace --stats -d $O/prof -o bench -- python3 $R/bench.py --full --no-cpu > $O/prof_bench.log 2>&1
timeout -k 10 300 rocprofv3 --pmc FETCH_SIZE --output-format csv -d $O/pmc_fetch -o run -- python3 $R/bench.py --full --no-cpu --steps 3 --warmup 1 > $O/pmc_fetch.log 2>&1
timeout -k 10 300 rocprofv3 --pmc WRITE_SIZE --output-format csv -d $O/pmc_write -o run -- python3 $R/bench.py --full --no-cpu --steps 3 --warmup 1 > $O/pmc_write.log 2>&1
