# does the roofline timing cost anything on the refined mesh?  same box, sampling on (default) / off
# usage: bash tools/refine_sampling_ab.sh <refine> <steps> <output directory>
cd /tmp && export TMPDIR=/tmp && cd $GRAFT_REPO_ROOT
out=$3; mkdir -p $out
for rep in 1 2; do
  for ev in 4 1000000; do
    GMPNP_BENCH_SAMPLE_EVERY=$ev python bench.py --full --refine $1 --steps $2 --warmup 1 --no-cpu-baseline > $out/rsab_$ev.$rep.json 2> $out/rsab_$ev.$rep.err
    python -c "import json; d=json.load(open('$out/rsab_$ev.$rep.json')); r=d['roofline']; print('every $ev', $rep, 'its/s %.3f' % d['value'], 'mean us %.1f' % r['mean_launch_us'], 'sampled', r['launches_sampled'], 'of', r['launches_total'])"
  done
done
