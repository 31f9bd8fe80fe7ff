# one-off: L2 hit / miss and request counters of the bench kernels (GPU box)
OUT=${OUT:-prof_out}   # output folder of the runs below, relative to the repository root
cd /tmp && export TMPDIR=/tmp && cd $GRAFT_REPO_ROOT
for c in "TCC_HIT_sum TCC_MISS_sum" "TCC_REQ_sum TCC_READ_sum" "TCP_TCC_READ_REQ_sum TCP_TOTAL_CACHE_ACCESSES_sum"; do
  tag=$(echo $c | tr ' ' '_')
  rm -rf $OUT/pmcx_$tag
  timeout -k 10 400 rocprofv3 --kernel-trace --pmc $c --output-format csv -d $OUT/pmcx_$tag -- python bench.py --steps 1 --warmup 1 --full --no-cpu-baseline > $OUT/pmcx_$tag.json 2> $OUT/pmcx_$tag.err
  python tools/pmc_summary.py $OUT/pmcx_$tag > $OUT/pmcx_$tag.txt 2>&1
done
cat $OUT/pmcx_*.txt | grep "k_hsc\|k_build_edges\|k_schur\|k_backsubst\|k_errors\|=="
