O=${O:-out/r05full}; mkdir -p $O
python -c "import __graft_entry__ as g; g.smoke(); print('smoke ok')" > $O/smoke.log 2>&1; tail -2 $O/smoke.log
timeout 3000 python -m pytest tests -m gpu -q -x --durations=15 > $O/gputests.log 2>&1; echo "gpu tests rc $?"; tail -25 $O/gputests.log
timeout 900 python bench.py --full > $O/bench_default.json 2> $O/bench_default.err; echo "bench rc $?"; tail -c 3000 $O/bench_default.json
