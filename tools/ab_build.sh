# Build the engine library of a git revision (or the working tree, "wt") into ab/lib<name>.so
# for A/B timing on one GPU box (tools/ab.sh).  usage: [AB_DEFS=-DX=1] tools/ab_build.sh <name> [rev | wt | dir]
# The sources are whatever *.cpp and *.hip the tree being built holds in clonos_amd/csrc/, as in
# clonos_amd/build.py, so one script builds revisions with different file layouts.
set -euo pipefail
root=$(cd "$(dirname "$0")/.." && pwd)
name=$1; rev=${2:-wt}
mkdir -p "$root/ab"
if [ "$rev" = wt ]; then
  src=$root
elif [ -d "$rev" ]; then  # a directory holding clonos_amd/ and include/
  src=$rev
else
  src=/tmp/ab_wt_$name; rm -rf "$src"; mkdir -p "$src"
  git -C "$root" archive "$rev" clonos_amd include | tar -x -C "$src"
fi
objs=(); pids=(); waited=0
for p in $(ls "$src"/clonos_amd/csrc/*.cpp "$src"/clonos_amd/csrc/*.hip | LC_ALL=C sort); do
  o=/tmp/ab_${name}_$(basename "$p").o
  if [ $((${#pids[@]} - waited)) -ge 16 ]; then wait "${pids[$waited]}"; waited=$((waited + 1)); fi  # 16 compiles in flight at most
  /opt/rocm/bin/hipcc -x hip --offload-arch=gfx950 -O3 -std=c++17 -fPIC -w ${AB_DEFS:-} -I "$src/include" -c "$p" -o "$o" &
  pids+=($!); objs+=("$o")
done
for pid in "${pids[@]:$waited}"; do wait "$pid"; done
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o "$root/ab/lib$name.so" "${objs[@]}"
echo "$root/ab/lib$name.so"
