#!/bin/bash
# One GPU-box pass that produces everything tools/refresh_profiles.py turns into profiles/ (round tag as $1, default r02): the bench
# line of `bench.py --full` (with its own PMC child passes), the rocprofv3 kernel trace of the same command (minus the CPU leg and the
# one-pair bitstream extra), one SQ-counter pass, and kernel traces of the training step / the CQE forward.
# Output goes to $PROFILE_OUT under the repo root (default profile_out/), where refresh_profiles.py reads it.
# usage (from the repo root, on the GPU box): bash tools/profile_round.sh r02
set -o pipefail
TAG=${1:-r02}
R=${GRAFT_REPO_ROOT:-$(pwd)}
O="$R/${PROFILE_OUT:-profile_out}"
mkdir -p "$O"
rm -rf "$O/prof_$TAG" "$O/pmc_sq" "$O/prof_train" "$O/prof_cqe" "$O/prof_cqetrain"
cd "$R"
timeout -k 10 700 python bench.py --full > "$O/bench_n1.json" 2> "$O/bench_n1.err" || echo "bench failed"
cd /tmp && export TMPDIR=/tmp
timeout -k 10 500 rocprofv3 --kernel-trace --stats -d "$O/prof_$TAG" -o $TAG -- python3 "$R/bench.py" --full --no-cpu-baseline --no-codec --no-pmc > "$O/prof_bench.log" 2>&1 || echo "trace failed"
SQ="SQ_VALU_MFMA_BUSY_CYCLES SQ_BUSY_CYCLES SQ_WAVE_CYCLES SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_WAIT_INST_LDS SQ_LDS_BANK_CONFLICT SQ_LDS_IDX_ACTIVE"
timeout -k 10 300 rocprofv3 --pmc $SQ --output-format csv -d "$O/pmc_sq" -o s -- python3 "$R/bench.py" --pmc-child > "$O/pmc_sq.log" 2>&1 || echo "sq failed"
timeout -k 10 300 rocprofv3 --kernel-trace -d "$O/prof_train" -o tr -- python3 "$R/tools/train_prof.py" bf16 > "$O/prof_train.log" 2>&1 || echo "train trace failed"
timeout -k 10 300 rocprofv3 --kernel-trace -d "$O/prof_cqe" -o c -- python3 "$R/tools/cqe_prof.py" bf16 > "$O/prof_cqe.log" 2>&1 || echo "cqe trace failed"
timeout -k 10 300 rocprofv3 --kernel-trace -d "$O/prof_cqetrain" -o ct -- python3 "$R/tools/cqe_prof.py" bf16 train > "$O/prof_cqetrain.log" 2>&1 || echo "cqe train trace failed"
cd "$R"
# keep the merge small: the trace databases and the counter CSVs are all refresh_profiles.py reads
find "$O/prof_$TAG" "$O/pmc_sq" "$O/prof_train" "$O/prof_cqe" "$O/prof_cqetrain" -type f ! -name '*results.db' ! -name '*counter_collection.csv' -delete
ls -la "$O/prof_$TAG" "$O/pmc_sq"
tail -c 400 "$O/bench_n1.json"
