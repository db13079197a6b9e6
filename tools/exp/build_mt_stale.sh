#!/bin/bash
# experiment: the product library whose draw ring is filled once and then left stale (-DACAV_MT_ABL_STALE: no generator or jump
# launches after the first two superblocks, the events still go round) -> tools/exp/libacav_hip_mtstale.so.  The selection is
# wrong by construction; against the product library the loop's ACAV_MI_TIMING line shows what the generator costs by running
# beside the position kernels:
#   ACAV_LIB_PATH=tools/exp/libacav_hip_mtstale.so ACAV_MI_TIMING=1 python tools/bench_mi.py 1000000 256 2 0 20000
# (needs build/obj/*.o of a normal build: python __graft_entry__.py)
cd "$(dirname "$0")/../.."
F="--offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off -fhip-fp32-correctly-rounded-divide-sqrt -fno-fast-math -fvisibility=hidden -Wno-unused-function -Wno-inline-asm -I include"
hipcc $F -DACAV_EXPERIMENT_BUILD -DACAV_MT_ABL_STALE -c acav100m_amd/csrc/acav_mi.hip -o build/acav_mi_stale.o || exit 1
objs=$(ls build/obj/*.o | grep -v "acav_mi.o\|acav_mi_empty.o")
hipcc --offload-arch=gfx950 -shared -fPIC -fvisibility=hidden -o tools/exp/libacav_hip_mtstale.so $objs build/acav_mi_stale.o
