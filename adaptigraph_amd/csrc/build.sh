#!/usr/bin/env bash
# Build libadaptigraph_hip.so for gfx950 (MI355X), in-tree.  hipcc cross-compiles without a GPU.
#   build.sh         the product library, and libadaptigraph_hip_cma.so: the CMA-ES search (ag_cma.hip, ag_api_cma.hip;
#                    include/adaptigraph_amd_cma.h), a library of its own that needs no engine context, and
#                    libadaptigraph_hip_cells.so: the cell-list edge builder, the rollout over its graphs, the tiled Chamfer cost and
#                    the cell-pruned farthest-point sampler (ag_cells.hip, ag_chamfer_tiled.hip, ag_fps_grid.hip, ag_api_cells.hip;
#                    include/adaptigraph_amd_cells.h), a library of its own that works on the engine's contexts and links against it
#   build.sh diag    also libadaptigraph_hip_diag.so: the same sources with -DAG_DIAG (in-kernel clock / phase probes and the
#                    injected-failure hook, ag_diag.hip) - used by tools/ and one test, never loaded by the product package
#   build.sh experiment <name> <flags...>   only libadaptigraph_hip_<name>.so: the same sources with extra flags, own object
#                    dir (tools/build_experiment.sh) - loaded with ADAPTIGRAPH_AMD_LIB by tools/ only
# In front of any of the three:
#   -n               dry run: print "compile <object>" / "link <library>" for what would be done, and do nothing
#   --newer <file>   treat <file> (a path as the compiler names it: ag_model.h, ../../include/adaptigraph_amd.h) as newer than
#                    every object; may be repeated.  Nothing in the tree is touched.
# And one form that builds nothing:
#   build.sh asm <product|cma|cells|diag> <dir>   the device assembly of every source of that library, with the library's own flags,
#                    as <dir>/<source>.s; <dir> must lie outside the repository
#
# What is rebuilt.  Every compile leaves, beside its object, the dependency file the compiler wrote (.d: the source and the headers
# it actually read) and the command line it ran (.cmd).  An object is stale when it or either of the two is missing, when a file of
# its dependency list is newer or gone, or when the command it would be compiled with now differs from the recorded one - so a new
# flag rebuilds, an edit to this file that changes no command does not.  The stale objects of all requested libraries compile side by
# side: MAX_JOBS at a time if set, else one per processor, 16 at the most.
set -euo pipefail
cd "$(dirname "$0")"
HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}
FLAGS="-O3 -std=c++17 -fPIC --offload-arch=gfx950 -ffp-contract=off -Wall -Wno-unused-function ${AG_EXTRA_FLAGS:-}"
# per-file extras: the fused MLP chains are scheduled for ILP (hipcc's default strategy leaves ~0.9 % on k_edge_enc and
# ~0.5 % on k_node_prop: A/B on the same box); scheduling only, results are bit-identical
declare -A PERFILE=( [ag_mlp]="-mllvm -amdgpu-sched-strategy=max-ilp" )
ENGINE_SRCS="ag_edges ag_rules ag_mlp ag_lat ag_graph ag_cost ag_setloss ag_emd ag_mppi ag_train ag_optim ag_ppm ag_dataset ag_eval ag_api ag_api_edges ag_api_rollout ag_api_train ag_api_dataset ag_api_eval"

# ---- the libraries: object dir, extra flags, output, sources, extra link arguments
declare -A V_DIR V_FLAGS V_OUT V_SRCS V_LINK
variant() { V_DIR[$1]=$2; V_FLAGS[$1]=$3; V_OUT[$1]=$4; V_SRCS[$1]=$5; V_LINK[$1]=${6:-}; }
variant product build "" libadaptigraph_hip.so "$ENGINE_SRCS"
variant cma build/cma "" libadaptigraph_hip_cma.so "ag_cma ag_api_cma"
# The cells library calls the engine's internal C++ helpers (begin_call, fail, the slab of ag_host.h) and reads ag_ctx's layout across
# the shared-object boundary: the two are always built together, here, from one tree.  The diag and experiment variants get none.
variant cells build/cells "" libadaptigraph_hip_cells.so "ag_cells ag_chamfer_tiled ag_fps_grid ag_api_cells" "-L. -ladaptigraph_hip -Wl,-rpath,\$ORIGIN"
variant diag build/diag "-DAG_DIAG" libadaptigraph_hip_diag.so "$ENGINE_SRCS ag_diag"

DRY=0; NEWER=" "
while true; do
  case "${1:-}" in
    -n) DRY=1; shift ;;
    --newer) NEWER="$NEWER$2 "; shift 2 ;;
    *) break ;;
  esac
done
compile_cmd() {   # $1 = variant, $2 = source: the command that makes its object, minus the bookkeeping arguments
  echo "$HIPCC $FLAGS ${V_FLAGS[$1]} ${PERFILE[$2]:-} -c $2.hip -o ${V_DIR[$1]}/$2.o"
}

if [ "${1:-}" = "asm" ]; then
  v=${2:?asm: which library}; out=${3:?asm: which directory}
  [ -n "${V_DIR[$v]:-}" ] || { echo "asm: no library '$v'" >&2; exit 2; }
  mkdir -p "$out"
  case "$(cd "$out" && pwd -P)/" in "$(cd ../.. && pwd -P)"/*) echo "asm: $out lies inside the repository" >&2; exit 2 ;; esac
  JOBS=${MAX_JOBS:-$(nproc)}; [ "$JOBS" -le 16 ] || JOBS=16
  n=0; rc=0
  for f in ${V_SRCS[$v]}; do
    $HIPCC $FLAGS ${V_FLAGS[$v]} ${PERFILE[$f]:-} --offload-device-only -S $f.hip -o "$out/$f.s" &
    n=$((n + 1)); if [ $n -ge "$JOBS" ]; then wait -n || rc=1; n=$((n - 1)); fi
  done
  while [ $n -gt 0 ]; do wait -n || rc=1; n=$((n - 1)); done
  exit $rc
fi
if [ "${1:-}" = "experiment" ]; then
  name=$2; shift 2
  variant "$name" "build/$name" "$*" "libadaptigraph_hip_$name.so" "$ENGINE_SRCS"
  WANT="$name"
elif [ "${1:-}" = "diag" ]; then
  WANT="product cma cells diag"
else
  WANT="product cma cells"
fi

stale() {   # $1 = variant, $2 = source
  local o=${V_DIR[$1]}/$2.o d
  [ -f $o ] && [ -f $o.d ] && [ -f $o.cmd ] || return 0
  [ "$(cat $o.cmd)" = "$(compile_cmd $1 $2)" ] || return 0
  for d in $(sed -e 's/^[^:]*://' -e 's/\\$//' $o.d); do
    [ -f $d ] && [ ! $d -nt $o ] || return 0
    case "$NEWER" in *" $d "*) return 0 ;; esac
  done
  return 1
}
compile() {   # $1 = variant, $2 = source; output kept in the object's .log
  local o=${V_DIR[$1]}/$2.o cmd
  cmd=$(compile_cmd $1 $2)
  rm -f $o $o.cmd
  $cmd -MMD -MF $o.d > $o.log 2>&1 && echo "$cmd" > $o.cmd
}

# the sources with per-file extras are the long compiles: they start first
TODO=""; LATER=""
for v in $WANT; do
  [ $DRY = 1 ] || mkdir -p ${V_DIR[$v]}
  for f in ${V_SRCS[$v]}; do
    if stale $v $f; then
      if [ -n "${PERFILE[$f]:-}" ]; then TODO="$TODO $v:$f"; else LATER="$LATER $v:$f"; fi
    fi
  done
done
TODO="$TODO$LATER"
JOBS=${MAX_JOBS:-$(nproc)}; [ "$JOBS" -le 16 ] || JOBS=16
n=0; rc=0
for t in $TODO; do
  v=${t%%:*}; f=${t#*:}
  if [ $DRY = 1 ]; then echo "compile ${V_DIR[$v]}/$f.o"; continue; fi
  compile $v $f &
  n=$((n + 1)); if [ $n -ge "$JOBS" ]; then wait -n || rc=1; n=$((n - 1)); fi
done
while [ $n -gt 0 ]; do wait -n || rc=1; n=$((n - 1)); done
for t in $TODO; do   # what the compiler said, warnings included, in the order of the list
  v=${t%%:*}; f=${t#*:}; o=${V_DIR[$v]}/$f.o
  [ $DRY = 1 ] || [ ! -s $o.log ] || { echo "---- $o"; cat $o.log; }
  [ $DRY = 1 ] || [ -f $o.cmd ] || echo "FAILED: $o" >&2
done
[ $rc = 0 ] || exit 1

for v in $WANT; do
  objs=""; relink=0
  [ -f ${V_OUT[$v]} ] || relink=1
  for f in ${V_SRCS[$v]}; do
    o=${V_DIR[$v]}/$f.o; objs="$objs $o"
    case " $TODO " in *" $v:$f "*) relink=1 ;; esac
    [ ! $o -nt ${V_OUT[$v]} ] || relink=1
  done
  [ $relink = 1 ] || continue
  if [ $DRY = 1 ]; then echo "link ${V_OUT[$v]}"; continue; fi
  $HIPCC -shared -fPIC --offload-arch=gfx950 $objs ${V_LINK[$v]} -o ${V_OUT[$v]}
  echo "built $(pwd)/${V_OUT[$v]}"
done
