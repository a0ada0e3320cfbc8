#!/usr/bin/env bash
# Build libadaptigraph_hip.so for gfx950 (MI355X), in-tree.  hipcc cross-compiles without a GPU.
#   build.sh         the product library, and libadaptigraph_hip_cma.so: the CMA-ES search (ag_cma.hip, ag_api_cma.hip;
#                    include/adaptigraph_amd_cma.h), a library of its own that needs no engine context, and
#                    libadaptigraph_hip_cells.so: the cell-list edge builder (ag_cells.hip, ag_api_cells.hip;
#                    include/adaptigraph_amd_cells.h), a library of its own that works on the engine's contexts and links against it
#   build.sh diag    also libadaptigraph_hip_diag.so: the same sources with -DAG_DIAG (in-kernel clock / phase probes and the
#                    injected-failure hook, ag_diag.hip) - used by tools/ and one test, never loaded by the product package
#   build.sh experiment <name> <flags...>   only libadaptigraph_hip_<name>.so: the same sources with extra flags, own object
#                    dir (tools/build_experiment.sh) - loaded with ADAPTIGRAPH_AMD_LIB by tools/ only
set -euo pipefail
cd "$(dirname "$0")"
HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}
FLAGS="-O3 -std=c++17 -fPIC --offload-arch=gfx950 -ffp-contract=off -Wall -Wno-unused-function ${AG_EXTRA_FLAGS:-}"
# per-file extras: the fused MLP chains are scheduled for ILP (hipcc's default strategy leaves ~0.9 % on k_edge_enc and
# ~0.5 % on k_node_prop: A/B on the same box); scheduling only, results are bit-identical
declare -A PERFILE=( [ag_mlp]="-mllvm -amdgpu-sched-strategy=max-ilp" )
ENGINE_SRCS="ag_edges ag_rules ag_mlp ag_lat ag_graph ag_cost ag_setloss ag_emd ag_mppi ag_train ag_optim ag_ppm ag_dataset ag_eval ag_api ag_api_edges ag_api_rollout ag_api_train ag_api_dataset ag_api_eval"
SRCS=$ENGINE_SRCS
build_variant() {   # $1 = object dir, $2 = extra flags, $3 = output, $4 = extra sources
  mkdir -p "$1"
  local objs=""
  for f in $SRCS $4; do
    if [ ! -f $1/$f.o ] || [ $f.hip -nt $1/$f.o ] || [ ag_common.h -nt $1/$f.o ] || [ ag_host.h -nt $1/$f.o ] || [ ag_edge_select.h -nt $1/$f.o ] || [ ../../include/adaptigraph_amd.h -nt $1/$f.o ] || [ ../../include/adaptigraph_amd_cma.h -nt $1/$f.o ] || [ build.sh -nt $1/$f.o ]; then
      rm -f $1/$f.o
    fi
    for d in ${DEPS_EXTRA:-}; do [ -f $1/$f.o ] && [ $d -nt $1/$f.o ] && rm -f $1/$f.o; done   # headers only this library includes
    [ -f $1/$f.o ] || $HIPCC $FLAGS $2 ${PERFILE[$f]:-} -c $f.hip -o $1/$f.o
    objs="$objs $1/$f.o"
  done
  $HIPCC -shared -fPIC --offload-arch=gfx950 $objs ${LINK_EXTRA:-} -o $3
  echo "built $(pwd)/$3"
}
if [ "${1:-}" = "experiment" ]; then
  name=$2; shift 2
  build_variant build/$name "$*" libadaptigraph_hip_$name.so ""
  exit 0
fi
build_variant build "" libadaptigraph_hip.so ""
SRCS="ag_cma ag_api_cma"
build_variant build/cma "" libadaptigraph_hip_cma.so ""
# The cells library calls the engine's internal C++ helpers (begin_call, fail, the slab of ag_host.h) and reads ag_ctx's layout across
# the shared-object boundary: the two are always built together, here, from one tree.  The diag and experiment variants get none.
SRCS="ag_cells ag_api_cells"
DEPS_EXTRA="ag_cells.h ../../include/adaptigraph_amd_cells.h" LINK_EXTRA="-L. -ladaptigraph_hip -Wl,-rpath,\$ORIGIN" build_variant build/cells "" libadaptigraph_hip_cells.so ""
if [ "${1:-}" = "diag" ]; then
  SRCS=$ENGINE_SRCS
  build_variant build/diag "-DAG_DIAG" libadaptigraph_hip_diag.so "ag_diag"
fi
