#!/bin/bash
# MobileNet step, per-class table, under environment switches on the EXPERIMENT libraries: mob_classes.sh "" "BCNN_HIP_DWM_PF=4" ...
cd ${GRAFT_REPO_ROOT:-.}
export BCNN_LIB=$PWD/bcnn_amd/lib/libbcnn_exp.so BCNN_HIP_LIB=$PWD/bcnn_amd/lib/libbcnn_hip_exp.so
for sw in "$@"; do
  env $sw python bench.py --full --workload mobilenet --steps 8 --warmup 2 --no-cpu-baseline 2>/dev/null | tail -1 \
    | python -c "import sys,json; d=json.loads(sys.stdin.read()); k=d['kernel_classes']; print('[$sw]', d['ms_per_step'], {c: (round(k[c]['ms_per_step'],3), k[c]['frac_hbm']) for c in k})"
done
