#!/bin/bash
# Usage (build container, repo root): tools/build_exp.sh  -> tools/bin/libvppx_exp.so
# The library with the experiment hooks compiled in (-DVPPX_EXPERIMENT: VPPX_EXP_*, vppx_exp_*, VPPX_V3_IGNORE_LOST, the
# EXP-only VPPX_VARIANT tokens), next to the shipped one and never in its place; tools load it with VPPX_LIB=tools/bin/libvppx_exp.so.
# Every csrc/*.hip is compiled, and recompiled when it or any csrc/*.h or include/vppx.h is newer than its object.
set -e
cd "$(dirname "$0")/.."
mkdir -p tools/bin/exp_obj
src=vppstereo_amd/csrc
objs=()
pids=()
for hip in $src/*.hip; do
    o=tools/bin/exp_obj/$(basename $hip .hip).o
    objs+=($o)
    for dep in $hip $src/*.h include/vppx.h; do
        if [ $dep -nt $o ]; then # also when $o is not there yet
            /opt/rocm/bin/hipcc -O3 -std=c++17 -fPIC --offload-arch=gfx950 -ffp-contract=off -DVPPX_EXPERIMENT -Wno-unused-function -Wno-unused-variable -c $hip -o $o &
            pids+=($!)
            break
        fi
    done
done
for pid in "${pids[@]}"; do wait $pid; done
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o tools/bin/libvppx_exp.so "${objs[@]}"
ls -la tools/bin/libvppx_exp.so
