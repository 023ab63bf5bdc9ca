#!/bin/bash
# A/B of environment switches on one GPU box:
#   WL=c3 tools/ab_env.sh "TAG1:VAR=1 VAR2=x" "TAG2:" ...   (TAG: with nothing = product defaults)
wl=${WL:-c3}
steps=${STEPS:-20}
O=${OUT:-tool_out}   # where the records go
mkdir -p $O
for spec in "$@"; do
  tag=${spec%%:*}
  envs=${spec#*:}
  env $envs python bench.py --full --workload $wl --steps $steps --warmup 5 --no-extra --no-cpu-baseline --detail $O/ab_${wl}_${tag}.json > $O/ab_${wl}_${tag}.line 2> $O/ab_${wl}_${tag}.err
  python tools/ab_row.py $O/ab_${wl}_${tag}.json "$tag" "$envs"
done
