#!/bin/bash
# gfx950 assembly of one csrc/*.hip with the product flags: bash profiles/isa_dump.sh out.s [UNIT.hip] [-DNAME ...]
# UNIT defaults to salp_rollout_f1_std.hip, the one-food literal-constant kernels (the bench kernel among them);
# salp_vec.hip compiles the service kernels (salp_service_kernels.h).  Feed to profiles/isa_regs.py / isa_stats.py / isa_ophist.py / isa_cndruns.py;
# profiles/isa_kernel_diff.py compares the kernels of two sets of dumps.
set -e
OUT=$1; shift
UNIT=salp_rollout_f1_std.hip
case "$1" in *.hip) UNIT=$1; shift;; esac
cd "$(dirname "$0")/../underwater-swimmer_rl_amd/csrc"
/opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off -fno-fast-math -Wno-unused-function \
  -mllvm -disable-machine-licm "$@" -S --cuda-device-only -o "$OUT" "$UNIT"
