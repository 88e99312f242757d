o=${1:-runs/devin}; mkdir -p $o
TNML_SPEC_SPLIT=0 TNML_SVD_PRINT=-1 python bench.py --full --no-cpu-baseline --plain --steps 60 --warmup 5 > $o/full.json 2> $o/full.err
TNML_SPEC_SPLIT=0 TNML_SVD_PRINT=-1 python bench.py --full --no-cpu-baseline --plain --images 7500 --steps 100 > $o/shard.json 2> $o/shard.err
TNML_SPEC_SPLIT=0 TNML_SVD_PRINT=-1 python bench.py --full --no-cpu-baseline --plain --workload 8d --steps 200 > $o/w8d.json 2> $o/w8d.err
for f in full shard w8d; do echo $f; grep svd_check $o/$f.err | wc -l; grep svd_check $o/$f.err | tail -40 | cut -c1-150; done
