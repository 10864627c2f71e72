#!/bin/bash
# Build a variant of libtavhip.so into build/ab/<name>.so (git-ignored) for a same-box A/B of a modified tree:
#   tools/ab_build.sh base                           -> build/ab/base.so   (this tree's sources, the Makefile's flags)
#   tools/ab_build.sh o2 -O2                         -> build/ab/o2.so     (extra compiler flags after the name; the last -O wins)
#   git worktree add ../tav_parent HEAD~1 && ../tav_parent/tools/ab_build.sh parent
#                                                    -> ../tav_parent/build/ab/parent.so  (another revision, built from its own tree)
# then on the GPU box:  TAV_LIB=build/ab/base.so python tools/gpu_ab.py attn ; TAV_LIB=build/ab/o2.so python tools/gpu_ab.py attn
# The kernels carry no compile-time experiment switches: an experiment is a change to the sources on a branch or in a second worktree.
set -e
name=$1; shift
root="$(cd "$(dirname "$0")/.." && pwd)"
out="$root/build/ab"; mkdir -p "$out/obj_$name"
cd "$root/multi-modal-emotion_amd/csrc"
for src in *.hip; do          # every source, as the Makefile's SRCS
  /opt/rocm/bin/hipcc -O3 -std=c++17 -fPIC --offload-arch=gfx950 -Wall -Wno-unused-function -Wno-unused-variable -I../../include "$@" -c "$src" -o "$out/obj_$name/${src%.hip}.o" &
done
wait
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC "$out/obj_$name"/*.o -ldl -o "$out/$name.so"
echo "$out/$name.so"
