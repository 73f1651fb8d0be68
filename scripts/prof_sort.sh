# The query sort's kernels on the headline step, one engine build: [PROF_OUT=<dir>] bash scripts/prof_sort.sh <tag> [engine .so]
#   pass 1: counters alone (no tracing), pass 2: kernel trace alone; each under its own time limit, the second only if the first ended well.
# Output under $PROF_OUT/prof_sort_<tag> (default build/, which git ignores); the summary (mean per launch, grouped by kernel and grid
# size) is printed and kept there: python scripts/collect_sort_prof.py <that directory>
TAG=$1
SO=$2
OUT=${PROF_OUT:-build}/prof_sort_$TAG
ARGS="--gpus 1 --full --steps 10 --warmup 2 --cpu-queries 0 --stream-probe 0 --replan-probe 0 --c4-probe 0 --clustered-probe 0"
mkdir -p $OUT
[ -n "$SO" ] && export PCT_ENGINE_SO=$SO
timeout -k 10 240 rocprofv3 --pmc SQ_INSTS_VALU SQ_ACTIVE_INST_VALU SQ_WAVE_CYCLES SQ_WAIT_ANY SQ_WAVES GRBM_GUI_ACTIVE SQ_BUSY_CYCLES SQ_INSTS_SALU \
    --output-format csv -d $OUT/pmc -- python3 bench.py $ARGS > $OUT/pmc.log 2>&1 || { echo "pmc pass failed rc=$?"; tail -5 $OUT/pmc.log; exit 1; }
timeout -k 10 240 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/trace -- python3 bench.py $ARGS > $OUT/trace.log 2>&1 || { echo "trace pass failed rc=$?"; tail -5 $OUT/trace.log; exit 1; }
python3 scripts/collect_sort_prof.py $OUT | tee $OUT/summary.txt
