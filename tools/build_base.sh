#!/bin/bash
# usage: bash tools/build_base.sh [REV]  -> ts-pws_amd/lib/variant_base.so = the library of REV (default HEAD), for
# side-by-side timing against the working tree's build (tools/variants.sh), and lib/variant_base_sweeps.so = its build with the
# tuning / test switches (tools/batch_ab.py compares the engines they select)
set -e
REV=${1:-HEAD}
R=$(cd "$(dirname "$0")/.." && pwd)
rm -rf /tmp/tspws_base && git -C $R worktree add -f /tmp/tspws_base $REV -q
make -C /tmp/tspws_base/ts-pws_amd -j6 lib sweeps > /dev/null
cp /tmp/tspws_base/ts-pws_amd/lib/libtspws_hip.so $R/ts-pws_amd/lib/variant_base.so
cp /tmp/tspws_base/ts-pws_amd/lib/libtspws_hip_sweeps.so $R/ts-pws_amd/lib/variant_base_sweeps.so
git -C $R worktree remove --force /tmp/tspws_base
echo built variant_base.so and variant_base_sweeps.so from $REV
