# round 6: full evidence set of the current tree: smoke, the whole GPU suite, the default bench line, rocprofv3 trace + PMC passes
O=${O:-out/r06full}; mkdir -p $O
python -c "import __graft_entry__ as g; g.smoke(); print('smoke ok')" > $O/smoke.log 2>&1; tail -2 $O/smoke.log
timeout 3000 python -m pytest tests -m gpu -q -x --durations=15 > $O/gputests.log 2>&1; echo "gpu tests rc $?"; tail -25 $O/gputests.log
timeout 1200 python bench.py --full > $O/bench_default.json 2> $O/bench_default.err; echo "bench rc $?"; tail -c 3000 $O/bench_default.json
bash profiles/pmc_r06.sh > $O/pmc.log 2>&1; tail -5 $O/pmc.log
