#!/bin/bash
# tools/ab_env.sh "<VAR=value> ..." <bench args...> -- interleaved runs of the default library with and without environment switches
# (arm "default" = none set; one arm per quoted assignment), two rounds
ARMS=$1; shift
cd /tmp && export TMPDIR=/tmp; cd $GRAFT_REPO_ROOT
for round in 1 2; do
  for arm in default $ARMS; do
    if [ $arm = default ]; then E=""; else E=$arm; fi
    LINE=$(env $E timeout 600 python bench.py "$@" --full --no-cpu --no-secondary --no-power 2>/dev/null | tail -1) python -c "
import json, os; d=json.loads(os.environ['LINE']); print('$arm', d['value'], d.get('spread'), d['parity'][:20], d['kernels_ms_per_step'])"
  done
done
