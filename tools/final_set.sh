#!/bin/bash
# The evidence set of a round on an MI355X box (~6 GPU-minutes): tools/final_set.sh <tag> <out dir>
#   <out dir>/<tag>_bench_line.json             bench.py --full (CPU baseline + drop-in-caller figures)
#   gpurun_out/prof_<tag>/ + profiles/<tag>_*    tools/profile.sh: kernel stats, timeline, PMC passes
#   <out dir>/<tag>_gpu_profiler_configs.jsonl  the other BASELINE configurations through gpu_profiler
#   <out dir>/<tag>_lone_latency.txt            tools/lone_latency.py
set -u
tag=${1:-final}
O=$(mkdir -p "${2:?usage: tools/final_set.sh <tag> <out dir>}" && cd "$2" && pwd)
R=${GRAFT_REPO_ROOT:-/root/repo}
cd $R
# the counter passes first: bench.py replays roofline.traffic from profiles/pmc_traffic.json only while that file
# belongs to the kernel source it runs (kernel_source_sha256), so the file is refreshed before the evidence line is taken
bash tools/profile.sh $tag && cp gpurun_out/prof_$tag/summary/${tag}_pmc.json profiles/pmc_traffic.json && \
python bench.py --full > $O/${tag}_bench_line.json 2> $O/${tag}_bench.err && echo "bench ok" && \
{ cd $R/metal-msm-gpu-acceleration_amd
  ./gpu_profiler 24 1 gpu_resident 5 --layout ark --warmup 4 --json 2>/dev/null | grep '^{'
  ./gpu_profiler 18 1 gpu_resident 30 --warmup 4 --json 2>/dev/null | grep '^{'
  ./gpu_profiler 18 40 gpu_resident 5 --warmup 2 --json 2>/dev/null | grep '^{'
  ./gpu_profiler 16 40 gpu_resident 5 --warmup 2 --json 2>/dev/null | grep '^{'
  ./gpu_profiler 16 1 cpu 5 --json 2>/dev/null | grep '^{'
} > $O/${tag}_gpu_profiler_configs.jsonl && echo "configs ok" && \
cd $R && python tools/lone_latency.py 10,12,14,16,18,20,22 30 > $O/${tag}_lone_latency.txt 2>/dev/null && echo "lone ok" && \
for v in "--persistent-bases" "--precomputed-tables"; do python bench.py $v --no-cpu-baseline --no-extras 2>/dev/null; done > $O/${tag}_bench_tables_persistent.jsonl && echo "variants ok"
