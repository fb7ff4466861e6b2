#!/bin/bash
# build_alt.sh <name> <extra hipcc flags...>: builds cuda-pathtrace_amd/alt/<name>/libptcore.so for A/B experiments
# ALT_SRCS / ALT_LIB: another source list / library name (tools/primary_exclusion_mutants.py builds lab libraries with them)
set -e
cd "$(dirname "$0")/.."
N=$1; shift
mkdir -p cuda-pathtrace_amd/alt/$N
cd cuda-pathtrace_amd/csrc
/opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off -fno-fast-math -fno-slp-vectorize "$@" -shared -o ../alt/$N/${ALT_LIB:-libptcore.so} ${ALT_SRCS:-pt_kernel.hip pt_fast.hip pt_capi.hip pt_mgpu.hip pt_display.hip pt_host.cpp} -ldl -lpthread
