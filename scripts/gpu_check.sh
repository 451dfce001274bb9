set -x
cd $GRAFT_REPO_ROOT
out=${1:-$(mktemp -d)}; mkdir -p $out   # logs: the folder given, else a fresh temporary one
rocminfo | grep -E "Marketing Name|gfx" | head -4
timeout 600 python -m pytest tests -x -q -m gpu 2>&1 | tail -30 > $out/pytest_gpu.log; cat $out/pytest_gpu.log
timeout 300 python -c "import __graft_entry__ as g; g.smoke()" 2>&1 | tail -5
timeout 600 python bench.py --full --steps 200 --warmup 20 2>&1 | tail -3 | tee $out/bench1.json
