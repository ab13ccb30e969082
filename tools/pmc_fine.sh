#!/bin/bash
# Counter summary of the fine kernel (run on the GPU box): tools/pmc_fine.sh <commit-id> [bench.py args...] = tools/lab.py fine-counters
python3 "$(dirname "$0")/lab.py" fine-counters "$@"
