set -x
cd $GRAFT_REPO_ROOT
P="${1:?usage: collect_profiles.sh <output directory>}"
mkdir -p "$P"
python bench.py --full > "$P/bench.json" 2> "$P/bench.err"
tail -c 600 "$P/bench.json"
export TMPDIR=/tmp
rocprofv3 --kernel-trace --stats --output-format csv -d "$P/kt" -- python bench.py > "$P/kt.log" 2>&1
rocprofv3 -i tools/pmc_hbm.txt --kernel-trace --output-format csv -d "$P/pmc" -- python tools/conv_bench.py --B 24 --iters 3 > "$P/pmc.log" 2>&1
rocprofv3 -i tools/pmc_hbm.txt --kernel-trace --output-format csv -d "$P/pmcw" -- python tools/conv_bench.py --B 44 --k 1 --H 10 --W 15 --z 64 --iters 3 > "$P/pmcw.log" 2>&1
find "$P" -name "*.csv" | head -30
