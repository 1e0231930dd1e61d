#!/bin/bash
# round 4, final job (the tree as committed last): full GPU suite, default bench line, kernel stats of the same bench, hardware
# counters of the three dominant kernels ON THIS TREE: SQ counters and FETCH_SIZE / WRITE_SIZE of the Fr and M128
# transforms (tools/timing/ntt_only.py {0,1} 20) and of the KZG commit (tools/timing/commit_only.py 20 40), small-size latency,
# the many-commit shapes.  Every rocprofv3 run has the program directly after `--`, counters in runs of their own.
R=${GRAFT_REPO_ROOT:-/root/repo}
O=$R/gpurun_out
T=${1:-r04final}
mkdir -p $O
cd $R
( time timeout 2400 python -m pytest tests -m gpu -x -q --durations=8 ) > $O/${T}_pytest.log 2>&1
echo "pytest rc=$?" >> $O/${T}_pytest.log
timeout 1200 python bench.py --full > $O/${T}_bench.json 2> $O/${T}_bench.err
echo "bench rc=$?" >> $O/${T}_pytest.log
python tools/timing/small_latency.py > $O/${T}_small_latency.txt 2>&1
python tools/timing/many_commit.py 10:256,10:256:1:10,10:256:1:12,12:64,12:64:1:10,8:1024,8:1024:1:10,14:16 > $O/${T}_many_commit.txt 2>&1
bash tools/gpu_jobs/r04_many_trace.sh > $O/${T}_many_commit_kernel_trace.txt 2>&1
cd /tmp && export TMPDIR=/tmp
BENCH="$R/bench.py --full --steps 10 --warmup 2 --skip-cpu --extra-sizes= --e2e-log2n 0 --strong-log2n 0 --strong-ntt-log2n 0 --no-two-in-flight"
timeout 900 rocprofv3 --kernel-trace --stats --output-format csv -d $O/${T}_prof -- python3 $BENCH > $O/${T}_bench_under_rocprof.json 2> $O/${T}_prof.err
find $O/${T}_prof -name "*kernel_stats.csv" -exec cp {} $O/${T}_bench_kernel_stats.csv \;
python3 $R/tools/timing/prof_split.py $(find $O/${T}_prof -name "*kernel_trace.csv" | head -1) > $O/${T}_per_msm_kernel_budget.txt 2>&1
SQ="SQ_WAVES SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_INSTS_VALU SQ_ACTIVE_INST_VALU SQ_WAIT_INST_ANY SQ_INSTS_LDS"
run_pmc() {   # tag, program and arguments...
  local tag=$1; shift
  timeout 300 rocprofv3 --kernel-trace --pmc $SQ --output-format csv -d $O/${T}_${tag}_SQ -- python3 "$@" > $O/${T}_${tag}_SQ.log 2>&1
  for c in FETCH_SIZE WRITE_SIZE; do
    timeout 300 rocprofv3 --kernel-trace --pmc $c --output-format csv -d $O/${T}_${tag}_$c -- python3 "$@" > $O/${T}_${tag}_$c.log 2>&1
  done
}
run_pmc nttfr $R/tools/timing/ntt_only.py 0 20
run_pmc nttm128 $R/tools/timing/ntt_only.py 1 20
run_pmc commit $R/tools/timing/commit_only.py 20 40
{
  echo "== KZG commit 2^20, default window width (commit_only.py 20 40)"; python3 $R/tools/timing/pmc_summary.py $O/${T}_commit_FETCH_SIZE $O/${T}_commit_WRITE_SIZE
  echo "== NTT Fr 2^20 (ntt_only.py 0 20)"; python3 $R/tools/timing/pmc_summary.py $O/${T}_nttfr_FETCH_SIZE $O/${T}_nttfr_WRITE_SIZE | grep k_ntt
  echo "== NTT M128 2^20 (ntt_only.py 1 20)"; python3 $R/tools/timing/pmc_summary.py $O/${T}_nttm128_FETCH_SIZE $O/${T}_nttm128_WRITE_SIZE | grep k_ntt
} > $O/${T}_hbm_traffic_pmc.txt 2>&1
{
  echo "== NTT Fr 2^20"; python3 $R/tools/timing/pmc_sq_summary.py $O/${T}_nttfr_SQ k_ntt
  echo "== NTT M128 2^20"; python3 $R/tools/timing/pmc_sq_summary.py $O/${T}_nttm128_SQ k_ntt
  echo "== KZG commit 2^20"; python3 $R/tools/timing/pmc_sq_summary.py $O/${T}_commit_SQ k_seg_accumulate k_seg_combine k_fine_scatter k_coarse_scatter k_reduce_tail
} > $O/${T}_sq_counters.txt 2>&1
cd $R
find $O -name "*.csv" -size +4M -delete
tail -16 $O/${T}_pytest.log; head -c 600 $O/${T}_bench.json; echo; head -30 $O/${T}_per_msm_kernel_budget.txt; cat $O/${T}_hbm_traffic_pmc.txt | cut -c1-160 | head -40; cat $O/${T}_sq_counters.txt | head -80; grep -v amdgpu $O/${T}_small_latency.txt; grep -v amdgpu $O/${T}_many_commit.txt | cut -c1-200
