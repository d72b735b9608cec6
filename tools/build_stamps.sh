#!/bin/bash
# Diagnostic build of the library with the fill kernel's wait counters (never shipped): writes
# pagan2-msa_amd/libpagan_dp_stats.so beside the product library; select it with PAGAN_DP_LIB=<that path>.
# The sources and the base flags are build.py's: there is one list.
set -e
cd "$(dirname "$0")/.."
python - <<'PY'
import importlib.util, os
spec = importlib.util.spec_from_file_location("_b", "pagan2-msa_amd/build.py"); m = importlib.util.module_from_spec(spec); spec.loader.exec_module(m)
m.FLAGS += ["-DPG_PIPE_STATS", "-DPG_TILE_STATS"] + os.environ.get("PG_STATS_EXTRA", "").split()
print(m.build(force=True, out=m.HERE + "/libpagan_dp_stats.so"))
PY
