#!/bin/bash
# usage (GPU box): tools/final_profiles.sh -- the judged artefacts of a round: PMC traffic of the GEMM kernel, the kernel table of the default bench,
# the default bench line.  Outputs under $OUT (default tool_out/; copied into profiles/ by hand).
R=$(cd "$(dirname "$0")/.." && pwd); export OUT=${OUT:-tool_out}; mkdir -p $R/$OUT
tools/pmc_bench.sh poisson3d_128 > $OUT/final_pmc.log 2>&1 || { tail -5 $OUT/final_pmc.log; exit 1; }
tail -1 $OUT/final_pmc.log | cut -c1-400
cp $OUT/r03_poisson3d_128_gemm_pmc_traffic.json profiles/r03_poisson3d_128_gemm_pmc_traffic.json  # the bench line below reports it (same head, same launch count)
cd /tmp; export TMPDIR=/tmp; rm -rf $R/$OUT/prof_final; mkdir -p $R/$OUT/prof_final; cd $R
timeout -k 10 900 rocprofv3 --kernel-trace --stats -d $OUT/prof_final -- python3 bench.py --full --no-cpu-baseline --no-oneshot --metric-workload "" --steps 3 --warmup 1 > $OUT/prof_final/bench.log 2>&1 || { tail -5 $OUT/prof_final/bench.log; exit 1; }
DB=$(find $OUT/prof_final -name "*results.db" | head -1)
python3 tools/rocpd_top_kernels.py $DB $OUT/final_kernel_stats.csv
rm -rf $OUT/prof_final
head -8 $OUT/final_kernel_stats.csv | cut -c1-160
timeout -k 10 900 python bench.py --full --steps 3 --warmup 1 > $OUT/final_bench_default.json 2> $OUT/final_bench_default.err || { tail -5 $OUT/final_bench_default.err; exit 1; }
tail -c 1500 $OUT/final_bench_default.json
