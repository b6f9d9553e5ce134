# Round-end check on the GPU box: the whole -m gpu suite, the full bench line, the round profile.
#   bash tools/round_check.sh <tag> <output dir>
cd /tmp && export TMPDIR=/tmp && cd $GRAFT_REPO_ROOT
T=${1:-r02}
O=${2:?usage: bash tools/round_check.sh <tag> <output dir>}
mkdir -p $O
python -m pytest tests -m gpu -q --timeout 1500 -p no:cacheprovider > $O/${T}_gputests.log 2>&1
grep -n "^E  \|^FAILED\|passed\|failed" $O/${T}_gputests.log | cut -c1-300 | tail -20
python bench.py --full > $O/${T}_bench.json 2> $O/${T}_bench.err
tail -c 300 $O/${T}_bench.err
bash tools/profile_round.sh $T > $O/${T}_prof.log 2>&1
tail -2 $O/${T}_prof.log
rocprofv3 --kernel-trace --output-format csv -d $O/trace_$T -- python tools/trace_loop.py > /dev/null 2>&1
python tools/trace_loop.py --parse $O/trace_$T > $O/${T}_loop_census.txt 2>&1
rm -rf $O/trace_$T
head -3 $O/${T}_loop_census.txt
