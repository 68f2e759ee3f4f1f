#!/bin/bash
# usage: ab_env.sh "VAR=a VAR2=b" "VAR=c" ...   -- tools/step_only.py 100 under each environment, twice, interleaved
# (the product's own switches -- tools/README.md -- work on libdbm.so; the work-skipping ones exist only in libdbm_measure.so:
#  add DBM_LIB=$PWD/deepbedmap_amd/libdbm_measure.so to the environments that set them.  The launch-size rules and kernel-form
#  choices that were tuning switches until round 6 are constants of the sources: an A/B of one of them is a patch)
cd "${GRAFT_REPO_ROOT:-$(dirname "$0")/../..}"
for rep in 1 2; do
  for e in "$@"; do
    echo "[$e] $(env $e timeout 200 python3 tools/step_only.py 100 2>&1 | tail -1)"
  done
done
