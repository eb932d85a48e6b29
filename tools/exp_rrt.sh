# dev experiment: RRT* leg vs batches in flight / queries per launch (log: $LOG, default build/rrt.log)
set -e
LOG=${LOG:-build/rrt.log}
mkdir -p $(dirname $LOG)
: > $LOG
for cfg in "3 256" "4 256" "6 256" "3 512"; do
  set -- $cfg
  echo "streams=$1 queries=$2" >> $LOG
  timeout -k 10 300 python -u bench.py --full --legs rrt --no-cpu-baseline --steps 1 --warmup 1 --rrt-streams $1 --rrt-queries $2 --rrt-steps 8 >> $LOG 2>&1
done
