cd /tmp && export TMPDIR=/tmp && cd $GRAFT_REPO_ROOT
out=${OARD_OUT:?set OARD_OUT to the folder that receives the results}
python bench.py --full --mode train --steps 10 --warmup 3 > $out/r3_train_b.json 2> $out/r3_train_b.err
python bench.py --full --mode train --batch 14 --steps 10 --warmup 3 > $out/r3_train_b14.json 2>> $out/r3_train_b.err
timeout 600 rocprofv3 --kernel-trace --stats -d $out/r3t_ttrace -o t -- python bench.py --mode train --steps 3 --warmup 1 > $out/r3t_ttrace.log 2>&1
python tools/prof_summary.py $out/r3t_ttrace/t_results.db > $out/r3t_train_kernel_trace_summary.txt
rm -rf $out/r3t_ttrace
OARD_TRAIN_PROFILE=1 python bench.py --mode train --steps 3 --warmup 1 2>&1 | grep "backward sweep" | tail -3
