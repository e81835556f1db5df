set -e
cd "$(dirname "$0")/.."
out=${OUT:-prof_out}
export TMPDIR=/tmp
mkdir -p $out/prof
python bench.py --full --steps 50 --warmup 10 > $out/bench_full.json 2> $out/bench_full.err
rocprofv3 --kernel-trace --stats -d $out/prof -o v20 --output-format csv -- python3 bench.py --full --steps 20 --warmup 5 --no-cpu-baseline > $out/bench_prof.json 2> $out/bench_prof.err
ls -R $out/prof | head -20
cat $out/bench_full.json
