cd /tmp && export TMPDIR=/tmp; cd $GRAFT_REPO_ROOT
out=${OUT_DIR:-bench_out}; mkdir -p $out      # where this script's files go
python bench.py --full > $out/bench_default.json 2> $out/bench_default.err
for e in dc_gan gan_stability_r1 hologan wgan_gp; do
  rm -rf /tmp/prof_$e
  timeout 400 rocprofv3 --kernel-trace --stats --output-format csv -d /tmp/prof_$e -- python bench.py --full --expt $e --steps 10 --warmup 2 --no-cpu-baseline --no-bs128 > $out/${e}_prof_line.json 2>/dev/null
  cp $(find /tmp/prof_$e -name "*kernel_stats.csv" | head -1) $out/r01i_${e}_kernel_stats.csv
  python tools/kstats.py $out/r01i_${e}_kernel_stats.csv 13 3
done
bash tools/bench_all.sh
cat $out/bench_default.json | cut -c1-1200
