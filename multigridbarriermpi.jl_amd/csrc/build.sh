#!/bin/bash
# Build libmgb_hip.so for gfx950 (MI355X).  hipcc cross-compiles without a GPU.
set -euo pipefail
HERE="$(cd "$(dirname "${BASH_SOURCE[0]}")" && pwd)"
OUT="$HERE/../lib"
mkdir -p "$OUT" "$HERE/_obj"
HIPCC="${HIPCC:-/opt/rocm/bin/hipcc}"
CXXFLAGS="-O3 -std=c++17 -fPIC -mavx2 -mfma -Wall -Wno-unused-result"
# kernel arguments preloaded into SGPRs at wave launch (gfx940+): the chain kernels start with descriptor -> data, not
# argument pointer -> descriptor -> data
PRELOAD="-mllvm -amdgpu-kernarg-preload-count=16"
HDRS=("$HERE"/*.hpp "$HERE/../../include/mgb_hip.h")
pids=()
# compile <object> <command...>: rebuild when the source or any header is newer; a stale object never survives a failed
# compile (it is deleted first), and every background job's exit status is checked
compile() {
  local obj="$1" src="$2"; shift 2
  local stale=0
  [ -f "$obj" ] || stale=1
  if [ $stale -eq 0 ]; then
    for f in "$src" "${HDRS[@]}"; do [ "$f" -nt "$obj" ] && stale=1; done
  fi
  if [ $stale -eq 1 ]; then
    rm -f "$obj"
    "$@" -c "$src" -o "$obj" &
    pids+=($!)
  fi
}
compile "$HERE/_obj/geometry.o" "$HERE/geometry.cpp" g++ $CXXFLAGS
compile "$HERE/_obj/mfchol.o" "$HERE/mfchol.cpp" g++ $CXXFLAGS
compile "$HERE/_obj/bwd_fused.o" "$HERE/bwd_fused.cpp" g++ $CXXFLAGS
compile "$HERE/_obj/chol_premap.o" "$HERE/chol_premap.cpp" g++ $CXXFLAGS
compile "$HERE/_obj/chol_plan.o" "$HERE/chol_plan.cpp" g++ $CXXFLAGS
compile "$HERE/_obj/kernels.o" "$HERE/kernels.hip" "$HIPCC" --offload-arch=gfx950 $CXXFLAGS
compile "$HERE/_obj/kernels_f32.o" "$HERE/kernels_f32.hip" "$HIPCC" --offload-arch=gfx950 $CXXFLAGS
compile "$HERE/_obj/mg.o" "$HERE/mg.hip" "$HIPCC" --offload-arch=gfx950 $CXXFLAGS
compile "$HERE/_obj/interp.o" "$HERE/interp.hip" "$HIPCC" --offload-arch=gfx950 $CXXFLAGS
compile "$HERE/_obj/reduce.o" "$HERE/reduce.hip" "$HIPCC" --offload-arch=gfx950 $CXXFLAGS
compile "$HERE/_obj/norms.o" "$HERE/norms.hip" "$HIPCC" --offload-arch=gfx950 $CXXFLAGS
compile "$HERE/_obj/energy.o" "$HERE/energy.hip" "$HIPCC" --offload-arch=gfx950 $CXXFLAGS
# levelset.hip holds the kernels AND the host restatement of the level sets: both sides run the same IEEE operations, so
# nothing in it may fuse (the basis of interp.hpp included)
compile "$HERE/_obj/levelset.o" "$HERE/levelset.hip" "$HIPCC" --offload-arch=gfx950 $CXXFLAGS -ffp-contract=off
# isosurface.hip: the same for the isosurfaces of 3-D fields (isosurface.hpp, interp.hpp's lagrange)
compile "$HERE/_obj/isosurface.o" "$HERE/isosurface.hip" "$HIPCC" --offload-arch=gfx950 $CXXFLAGS -ffp-contract=off
# flowline.hip: the same for the flow lines (flowline.hpp on top of interp.hpp's locator and bases)
compile "$HERE/_obj/flowline.o" "$HERE/flowline.hip" "$HIPCC" --offload-arch=gfx950 $CXXFLAGS -ffp-contract=off
# section.hip: the same for the plane sections (section.hpp on top of levelset.hpp, isosurface.hpp and flowline.hpp)
compile "$HERE/_obj/section.o" "$HERE/section.hip" "$HIPCC" --offload-arch=gfx950 $CXXFLAGS -ffp-contract=off
# pathline.hip: the same for the path lines (pathline.hpp on top of flowline.hpp); its object goes last on the link line
compile "$HERE/_obj/pathline.o" "$HERE/pathline.hip" "$HIPCC" --offload-arch=gfx950 $CXXFLAGS -ffp-contract=off
# ray.hip: the same for the line integrals (ray.hpp on top of section.hpp and flowline.hpp); its object goes last on the link line
compile "$HERE/_obj/ray.o" "$HERE/ray.hip" "$HIPCC" --offload-arch=gfx950 $CXXFLAGS -ffp-contract=off
# timestat.hip: the same for the time statistics (timestat.hpp); its object goes last on the link line
compile "$HERE/_obj/timestat.o" "$HERE/timestat.hip" "$HIPCC" --offload-arch=gfx950 $CXXFLAGS -ffp-contract=off
compile "$HERE/_obj/boundary.o" "$HERE/boundary.hip" "$HIPCC" --offload-arch=gfx950 $CXXFLAGS
compile "$HERE/_obj/estimate.o" "$HERE/estimate.hip" "$HIPCC" --offload-arch=gfx950 $CXXFLAGS
compile "$HERE/_obj/parabolic.o" "$HERE/parabolic.hip" "$HIPCC" --offload-arch=gfx950 $CXXFLAGS
compile "$HERE/_obj/amg_mg.o" "$HERE/amg_mg.cpp" "$HIPCC" --offload-arch=gfx950 $CXXFLAGS -x hip
compile "$HERE/_obj/gpuchol.o" "$HERE/gpuchol.hip" "$HIPCC" --offload-arch=gfx950 $CXXFLAGS $PRELOAD
compile "$HERE/_obj/amg.o" "$HERE/amg.cpp" "$HIPCC" --offload-arch=gfx950 $CXXFLAGS -x hip
compile "$HERE/_obj/comm.o" "$HERE/comm.cpp" "$HIPCC" --offload-arch=gfx950 $CXXFLAGS -x hip
compile "$HERE/_obj/capi.o" "$HERE/capi.cpp" "$HIPCC" --offload-arch=gfx950 $CXXFLAGS -x hip
for pid in "${pids[@]}"; do
  wait "$pid" || { echo "build.sh: a compile job failed" >&2; exit 1; }
done
rm -f "$OUT/libmgb_hip.so"
"$HIPCC" --offload-arch=gfx950 -shared -fPIC -o "$OUT/libmgb_hip.so" "$HERE"/_obj/{geometry,mfchol,bwd_fused,chol_premap,chol_plan,kernels,kernels_f32,mg,interp,reduce,norms,energy,levelset,isosurface,boundary,estimate,parabolic,gpuchol,amg,amg_mg,comm,capi,flowline,section,pathline,ray,timestat}.o -lpthread -ldl
echo "built $OUT/libmgb_hip.so"
